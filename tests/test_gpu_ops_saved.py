"""What the autograd Functions of nefes_amd/ops.py that share a forward / backward body keep for their backward, counted under
torch.autograd.graph.saved_tensors_hooks, and what they raise where a pass has no backward.

The unified convolution (ops.Conv2dSame behind frozen_conv2d and conv2d_same_train) saves its output only where a ReLU follows and its
input only where the weight or the bias asks for a gradient, so the refinement loop (frozen FusionNet) keeps one tensor per ReLU layer.
Every frozen-field Function (FieldFromRays, FieldFromPoints, FieldFromEncoding, FieldFromRaysHashGrid, FieldFromRaysFH, and RenderFineFH
on the same bodies) saves nothing, and asks the kernel for no ReLU masks, when no differentiable input requires a gradient or the mode
has no backward; otherwise the inputs its backward launch reads again, raw_t and the masks.

Shapes: the convolution at B = 1, Cin = 3, Cout = 4, 5 x 7 pixels, 3 x 3 and 5 x 5 kernels; the field at 3 rays x 50 samples (one full
128-sample tile and a ragged one) on the width-128 / C = 128 pack (with its factored-head pack) and a generic pack (W = 64, D = 6), and --
for the two Functions those cannot run -- on a generic pack for a supplied encoding (W = 96, D = 5) and the width-256 / C = 16 pack for
one (the hash grid's)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, S = 3, 50

NO_SIGMA_BWD = ("nefes_amd: the sigma-only field pass has no backward (the reference evaluates it without gradients at test time: "
                "nerfh_nff.py:192-202)")
NO_ENC_BWD = "nefes_amd: field backward is built for the FULL (fine) mode only"


class saved:
    """`with saved() as kept`: the tensors autograd nodes created inside saved for their backward."""

    def __enter__(self):
        self.kept = []
        self.hooks = torch.autograd.graph.saved_tensors_hooks(lambda t: self.kept.append(t) or t, lambda t: t)
        self.hooks.__enter__()
        return self.kept

    def __exit__(self, *exc):
        return self.hooks.__exit__(*exc)


# ---- the convolution -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("relu", [True, False])
def test_convolution_saves_its_output_for_a_relu_and_its_input_for_trainable_weights(k, relu):
    from nefes_amd import ops
    for cls in (ops.FrozenConv2d, ops.TrainConv2d):                  # one Function behind both entries: the two names add nothing to it
        assert issubclass(cls, ops.Conv2dSame) and "forward" not in vars(cls) and "backward" not in vars(cls)
    g = torch.Generator().manual_seed(k)
    x = torch.randn(1, 3, 5, 7, generator=g).to(DEV)
    w = (torch.randn(4, 3, k, k, generator=g) / (3 * k * k) ** 0.5).to(DEV)
    b = (torch.randn(4, generator=g) * 0.1).to(DEV)
    same = lambda a, t: a.data_ptr() == t.data_ptr() and a.shape == t.shape
    # frozen weights, nothing to differentiate: nothing is recorded at all
    with saved() as kept:
        y0 = ops.frozen_conv2d(x, w, b, relu=relu)
    assert kept == [] and y0.grad_fn is None
    # frozen weights (the refinement loop): the output where a ReLU follows, nothing otherwise -- through either entry
    for entry in (ops.frozen_conv2d, ops.conv2d_same_train):
        xr = x.clone().requires_grad_()
        with saved() as kept:
            y = entry(xr, w, b, relu=relu)
        assert len(kept) == (1 if relu else 0) and all(same(t, y) for t in kept), [tuple(t.shape) for t in kept]
        assert torch.equal(y, y0)
        y.sum().backward()
        assert xr.grad.shape == x.shape and bool(torch.isfinite(xr.grad).all())
    # trainable weight and bias, or either alone: the input as well
    for train_w, train_b in ((True, True), (True, False), (False, True)):
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(train_w), b.clone().requires_grad_(train_b)
        with saved() as kept:
            y = ops.conv2d_same_train(xr, wr, br, relu=relu)
        assert len(kept) == (2 if relu else 1) and same(kept[0], xr) and all(same(t, y) for t in kept[1:]), [tuple(t.shape) for t in kept]
        assert torch.equal(y, y0)
        y.sum().backward()
        assert xr.grad.shape == x.shape and (wr.grad is not None) == train_w and (br.grad is not None) == train_b
        with pytest.raises(ValueError, match="frozen_conv2d is for weights without gradient"):
            ops.frozen_conv2d(xr, wr, br, relu=relu)
    # ... and without a bias
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    with saved() as kept:
        y = ops.conv2d_same_train(xr, wr, None, relu=relu)
    assert len(kept) == (2 if relu else 1) and same(kept[0], xr)
    y.sum().backward()
    assert wr.grad.shape == w.shape


# ---- the frozen field ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    """Packs and inputs, made once and never modified: {name: ...}."""
    from nefes_amd import ops
    from nefes_amd.field import NeRFH_NFF
    net = lambda **kw: NeRFH_NFF('fine', encode_transient=True, **kw).requires_grad_(False).to(DEV)
    tuned, ext = net(W=128, f_dim=128, encode_appearance=True), net(W=256, f_dim=16, in_channels_xyz=32)
    g = torch.Generator().manual_seed(3)
    o = (torch.randn(N, 3, generator=g) * 0.3).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(DEV)
    z = torch.sort(torch.rand(N, S, generator=g) * 4, -1)[0].to(DEV)
    grid = ops.HashGrid(8.0, log2_hashmap_size=14, device=DEV)
    f = dict(tuned=tuned.packed(), fh=tuned.packed_fh(), generic=net(D=6, W=64, f_dim=16).packed_generic(),
             generic_ext=net(D=5, W=96, f_dim=128, in_channels_xyz=32).packed_generic(), ext=ext.packed(), grid=grid,
             rays=(o, d, d.clone(), z), pts=((o[:, None] + d[:, None] * z[..., None]).contiguous(), d.clone()),
             enc=((torch.randn(N, S, 32, generator=g) * 0.5).to(DEV), d.clone()))
    assert f["tuned"].width == 128 and f["tuned"].feat_dim == 128 and ops.is_generic(f["generic"]) and ops.is_generic(f["generic_ext"])
    assert ops.hashgrid_fused_ok(f["ext"], grid)
    return f


# (Function, its input tensors in `field`, how many of them are differentiable, the pack, {mode: the number of tensors it saves when
#  one of them requires a gradient, or the message of the NotImplementedError its backward raises -- and then it saves nothing})
def _field_cases():
    from nefes_amd import lib as L
    SIGMA, STATIC, FULL = L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL
    cases = []
    for pack in ("tuned", "generic"):
        cases += [("FieldFromRays", "rays", 3, pack, {SIGMA: NO_SIGMA_BWD, STATIC: 6, FULL: 6}),
                  ("FieldFromPoints", "pts", 2, pack, {SIGMA: NO_SIGMA_BWD, STATIC: 4, FULL: 4})]
    cases += [("FieldFromEncoding", "enc", 2, "generic_ext", {SIGMA: NO_ENC_BWD, STATIC: 3, FULL: 3}),
              ("FieldFromEncoding", "enc", 2, "ext", {SIGMA: NO_ENC_BWD, STATIC: NO_ENC_BWD, FULL: 3}),
              ("FieldFromRaysHashGrid", "rays", 3, "ext", {SIGMA: NO_SIGMA_BWD, FULL: 6})]
    return [(fn, inputs, n_diff, pack, mode, want) for fn, inputs, n_diff, pack, modes in cases for mode, want in modes.items()]


@pytest.mark.parametrize("fn,inputs,n_diff,pack,mode,want", _field_cases(), ids=[f"{c[0]}-{c[3]}-mode{c[4]}" for c in _field_cases()])
def test_field_functions_save_only_what_a_backward_will_read(field, fn, inputs, n_diff, pack, mode, want):
    from nefes_amd import ops
    more = (field[pack], mode) + ((field["grid"],) if fn == "FieldFromRaysHashGrid" else ())
    apply = getattr(ops, fn).apply
    # no input requires a gradient: nothing saved, no node
    with saved() as kept:
        raw0 = apply(*field[inputs], *more)
    assert kept == [] and raw0.grad_fn is None and raw0.shape == (N, field[pack].n_raw(mode), S)
    leaves = [t.clone().requires_grad_(i < n_diff) for i, t in enumerate(field[inputs])]
    with saved() as kept:
        raw = apply(*leaves, *more)
    assert torch.equal(raw, raw0)
    if isinstance(want, str):                      # the mode has no backward: nothing saved, and the backward says so
        assert kept == []
        with pytest.raises(NotImplementedError, match=re.escape(want)):
            raw.sum().backward()
        return
    assert len(kept) == want, [tuple(t.shape) for t in kept]
    raw.sum().backward()
    for t in leaves[:n_diff]:
        assert t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all())
    # a gradient asked of the depths alone is no reason to save anything either: they carry none (rendering.py:139 detaches them)
    if inputs == "rays":
        o, d, v, z = field["rays"]
        with saved() as kept:
            raw = apply(o, d, v, z.clone().requires_grad_(), *more)
        assert kept == []
        with pytest.raises(NotImplementedError, match=re.escape(NO_SIGMA_BWD)):
            raw.sum().backward()


def test_factored_head_functions_save_only_what_a_backward_will_read(field):
    """FieldFromRaysFH, and RenderFineFH on the same bodies: nothing without a differentiable input; with one, the rays, raw_t and the
    masks (RenderFineFH: the head's matrix and bias too).  Without a backward FieldFromRaysFH returns None for every input, where its
    siblings raise."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    pk, w_f, w_f_t, b_f = field["fh"]
    o, d, v, z = field["rays"]
    fine = lambda *rays: ops.RenderFineFH.apply(*rays, pk, w_f, w_f_t, b_f, L.COMP_TRANSIENT, 0.1)
    with saved() as kept:
        raw0 = ops.FieldFromRaysFH.apply(o, d, v, z, pk)
        maps0 = fine(o, d, v, z)
    assert kept == [] and raw0.grad_fn is None and all(m.grad_fn is None for m in maps0)
    leaves = [t.clone().requires_grad_() for t in (o, d, v)]
    with saved() as kept:
        raw = ops.FieldFromRaysFH.apply(*leaves, z, pk)
    assert len(kept) == 6 and torch.equal(raw, raw0)
    raw.sum().backward()
    assert all(t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) for t in leaves)
    leaves = [t.clone().requires_grad_() for t in (o, d, v)]
    with saved() as kept:
        maps = fine(*leaves, z)
    assert len(kept) == 8 and all(torch.equal(a, b) for a, b in zip(maps, maps0))
    (maps[0].sum() + maps[1].sum()).backward()
    assert all(t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) for t in leaves)
    # the depths alone: nothing saved, and a backward that hands every input None
    for run in (lambda zz: ops.FieldFromRaysFH.apply(o, d, v, zz, pk), lambda zz: fine(o, d, v, zz)[0]):
        zr = z.clone().requires_grad_()
        with saved() as kept:
            out = run(zr)
        assert kept == []
        out.sum().backward()
        assert zr.grad is None
