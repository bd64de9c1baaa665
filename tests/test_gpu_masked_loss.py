"""The masked feature-loss kernels (`--semantic`; csrc/feature_loss.hip MASKED instances; the `mask=` keyword of ops.cosine_feature_loss,
ops.upsampled_cosine_loss, ops.pixel_cosine_loss, ops.upsampled_pixel_cosine_loss) against the reference's expression -- compact both maps
to the valid pixels (`fr[:, valid]`), then CosineSimilarity -- in float64 on the CPU from the same fp32 inputs.

"Equal to float64" is the shared rule parity_log.check(tol=T, factor=1.5): e_hip <= max(T, 1.5 e_ref), e_ref the distance of the SAME
expression in float32 on the CPU from that truth, T = 3e-7 absolute for the loss and 2e-6 of the max-norm for gradients (the floors of the
unmasked twins, tests/test_gpu_pixcos.py).  The upstream gradient is 3.0.  Every group (image) is held to the rule on its own.

The up-sampled inputs carry an offset of 3 in the first channel of every group, so that no up-sampled pixel's vector a_p nearly cancels.
The per-pixel gradient scales with 1 / |a_p|, and at a non-integer scale the fp32 tap weights alone are ~3e-6 off (the CPU's
F.interpolate in float32 against float64 on (3, 9, 11) -> (31, 45): 2.8e-6 absolute in the up-sampled values); at a pixel of plain
randn input with |a_p| = 0.12 that moves the float32 CPU gradient itself by 4-6e-6 of the max-norm and any other legitimate fp32 order
by as much again -- there e_ref is one draw of rounding noise, not a yardstick.  The clamped and near-zero pixels have their own tests in
tests/test_gpu_pixcos.py, on the unmasked kernels whose arithmetic the masked instances share (all-ones test below: bit for bit).

One valid pixel, channel-wise: every cosine is +-1 and the true gradient is identically 0 (a cancellation of two equal terms), so its
max-norm is no unit; there the gradient is held to T_GRAD of the size of the cancelling terms, UP / (Cg |a_cp|)."""
import functools

import numpy as np
import pytest
import torch

from tests import parity_log as P
from tests.test_refine50_oracle import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_LOSS, T_GRAD, UP = 3e-7, 2e-6, 3.0
F = torch.nn.functional
FORMS = ("channel", "pixel")
MASKS = ("random", "single", "row", "ones")
LOW_SHAPES = [(1, 16, 192), (1, 3, 1000), (1, 141, 65), (3, 5, 257)]                     # (G, Cg, P)
UP_SHAPES = [(1, 5, 15, 20, 60, 80, 10), (1, 3, 9, 11, 31, 45, 3), (1, 2, 8, 8, 32, 32, 0), (1, 4, 6, 70, 24, 280, 1),
             (3, 5, 15, 20, 60, 80, 10)]                                                # (G, Cg, h, w, OH, OW, crop)
LOOP_SHAPE = (1, 128, 60, 80, 240, 320, 10)


def make_mask(kind, G, CH, CW, seed=0):
    """uint8 [G, CH, CW]: random at about 60 % valid with a different seed per group; one valid pixel (another one per group); one full
    row invalid; all ones."""
    m = torch.ones(G, CH, CW, dtype=torch.uint8)
    for g in range(G):
        if kind == "random":
            m[g] = (torch.rand(CH, CW, generator=torch.Generator().manual_seed(7919 * seed + 31 * g + 1)) < 0.6).to(torch.uint8)
        elif kind == "single":
            m[g] = 0
            m[g, (CH // 2 + g) % CH, (CW // 3 + 2 * g) % CW] = 1
        elif kind == "row":
            m[g, (CH // 3 + g) % CH] = 0
    return m


def low_grid(Pn):
    """The low-resolution maps are [.., P]; their masks are made on an (rows, cols) grid with rows * cols = P (257 is prime: one row
    -- "a full row invalid" would be an empty group, so there a run of 40 pixels is)."""
    for r in (12, 25, 5):
        if Pn % r == 0:
            return r, Pn // r
    return 1, Pn


@functools.lru_cache(maxsize=None)
def low_case(G, C, Pn, kind):
    g = torch.Generator().manual_seed(1000 * G + 10 * C + Pn)
    a = torch.randn(G * C, Pn, generator=g)
    b = torch.randn(G * C, Pn, generator=g) + 0.7 * a
    r, c = low_grid(Pn)
    m = make_mask(kind, G, r, c, seed=Pn).reshape(G, Pn)
    if r == 1 and kind == "row":
        m = torch.ones(G, Pn, dtype=torch.uint8)
        for k in range(G):
            m[k, 60 + 7 * k:100 + 7 * k] = 0
    return a, b, m.contiguous()


@functools.lru_cache(maxsize=None)
def up_case(G, C, h, w, OH, OW, crop, kind):
    g = torch.Generator().manual_seed(C * 1000 + h * 10 + w + G)
    x = torch.randn(G * C, h, w, generator=g)
    x[::C] += 3.0                                     # well-conditioned per pixel: see the module docstring
    up = F.interpolate(x[None], size=(OH, OW), mode="bicubic")[0][:, crop:OH - crop, crop:OW - crop]
    t = (torch.randn(up.shape, generator=g) + 0.5 * up).contiguous()
    return x, t, make_mask(kind, G, OH - 2 * crop, OW - 2 * crop, seed=OH)


def truth(x, target, mask, dtype, per_pixel, size=None, crop=0):
    """(loss, UP * d loss / d x) of the reference's expression for ONE group on the CPU in `dtype`: x [C, ...] (with `size`: [C,h,w],
    up-sampled and cropped), mask [...] of the compared pixels."""
    xs = x.to(dtype).clone().requires_grad_()
    a = xs
    if size is not None:
        a = F.interpolate(xs[None], size=size, mode="bicubic")[0]
        if crop:
            a = a[:, crop:-crop, crop:-crop]
    valid = torch.nonzero(mask.reshape(-1) > 0, as_tuple=True)[0]
    fr, ft = a.reshape(a.shape[0], -1)[:, valid], target.to(dtype).reshape(a.shape[0], -1)[:, valid]
    loss = 1 - torch.nn.CosineSimilarity(dim=0 if per_pixel else 1, eps=1e-6)(fr, ft).mean()
    (UP * loss).backward()
    return float(loss.detach()), xs.grad.numpy()


def op_of(form, geom):
    from nefes_amd import ops
    if geom is None:
        return ops.pixel_cosine_loss if form == "pixel" else ops.cosine_feature_loss
    f = ops.upsampled_pixel_cosine_loss if form == "pixel" else ops.upsampled_cosine_loss
    return lambda x, t, **kw: f(x, t, geom[:2], crop=geom[2], **kw)


def hip(form, geom, x, t, mask=None, G=1, **kw):
    """(loss, cos, UP * d loss / d x) of one of the four ops on the device; mask None: the unmasked one-pass op."""
    xd = x.to(DEV).requires_grad_()
    more = {} if mask is None else dict(mask=mask.to(DEV))
    loss, cos = op_of(form, geom)(xd, t.to(DEV), groups=G, return_cos=True, **more, **kw)
    (UP * loss).backward()
    return loss.detach().clone(), cos.clone(), xd.grad


def group_loss(form, cos, k, C):
    """The float64 loss of group k from the cosines the forward kept."""
    return 1.0 - float(cos[k]) if form == "pixel" else 1.0 - float(cos[k * C:(k + 1) * C].mean())


def check_groups(tag, form, kind, G, C, loss, cos, grad, x, t, m, geom=None):
    size, crop = (None, 0) if geom is None else (geom[:2], geom[2])
    pp = form == "pixel"
    assert cos.dtype == torch.float64 and tuple(cos.shape) == ((G,) if pp else (G * C,)) and not cos.requires_grad
    tot64 = tot32 = 0.0
    for k in range(G):
        sl = slice(k * C, (k + 1) * C)
        l64, g64 = truth(x[sl], t[sl], m[k], torch.float64, pp, size, crop)
        l32, g32 = truth(x[sl], t[sl], m[k], torch.float32, pp, size, crop)
        tot64, tot32 = tot64 + l64, tot32 + l32
        lk, gh = group_loss(form, cos, k, C), grad[sl].cpu().numpy()
        print(f"[{tag}][group {k}] loss: hip {abs(lk - l64):.2e} fp32 {abs(l32 - l64):.2e}; gradient: hip {rel(gh, g64):.2e} fp32 {rel(g32, g64):.2e}")
        P.check(f"{tag}[group {k}]", "loss (abs) vs float64 torch on the CPU", abs(lk - l64), abs(l32 - l64), abs(lk - l32), tol=T_LOSS, factor=1.5)
        assert np.isfinite(gh).all()
        if kind == "single" and not pp:
            # the true gradient is 0: T_GRAD of the cancelling terms' size (module docstring), not of its own max-norm
            a = x[sl].double()
            if geom is not None:
                a = F.interpolate(a[None], size=size, mode="bicubic")[0][:, crop:size[0] - crop, crop:size[1] - crop]
            ap = a.reshape(C, -1)[:, m[k].reshape(-1) > 0].abs()
            assert float(np.abs(g64).max()) < 1e-12 and float(np.abs(gh).max()) <= T_GRAD * UP / C * float((1 / ap).max()), (tag, k)
        else:
            P.check(f"{tag}[group {k}]", "d loss / d input (max-norm) vs float64 torch on the CPU", rel(gh, g64), rel(g32, g64), rel(gh, g32),
                    tol=T_GRAD, factor=1.5)
    P.check(tag, "loss of all groups (abs) vs float64", abs(float(loss) - tot64), abs(tot32 - tot64), tol=T_LOSS * G, factor=1.5)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("G,C,Pn", LOW_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_low_resolution_masked_loss_matches_float64(form, G, C, Pn, kind):
    """Value and gradient per group by the rule; d loss / d a exactly 0 at masked-out pixels."""
    a, b, m = low_case(G, C, Pn, kind)
    loss, cos, grad = hip(form, None, a, b, m, G)
    check_groups(f"masked_{form}_loss[{G},{C},{Pn}][{kind}]", form, kind, G, C, loss, cos, grad, a, b, m)
    out = (m == 0).to(DEV).repeat_interleave(C, 0)
    assert float(grad[out].abs().max() if out.any() else 0.0) == 0.0
    if not (kind == "single" and form == "channel"):
        assert float(grad[~out].abs().min()) > 0.0


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("G,C,h,w,OH,OW,crop", UP_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_upsampled_masked_loss_matches_float64(form, G, C, h, w, OH, OW, crop, kind):
    x, t, m = up_case(G, C, h, w, OH, OW, crop, kind)
    loss, cos, grad = hip(form, (OH, OW, crop), x, t, m, G)
    assert tuple(grad.shape) == (G * C, h, w)
    check_groups(f"masked_up_{form}_loss[{G},{C},{h},{w},{OH},{OW},{crop}][{kind}]", form, kind, G, C, loss, cos, grad, x, t, m, (OH, OW, crop))


@pytest.mark.parametrize("form", FORMS)
def test_masked_loss_at_the_loops_shape(form):
    G, C, h, w, OH, OW, crop = LOOP_SHAPE
    x, t, m = up_case(G, C, h, w, OH, OW, crop, "random")
    loss, cos, grad = hip(form, (OH, OW, crop), x, t, m, G)
    check_groups(f"masked_up_{form}_loss[loop shape][random]", form, "random", G, C, loss, cos, grad, x, t, m, (OH, OW, crop))


def _cases():
    return [(None, s) for s in LOW_SHAPES] + [("up", s) for s in UP_SHAPES]


def _load(where, shape, kind):
    """(x, target, mask, G, C, geom) of a low-resolution or an up-sampled case."""
    if where is None:
        return low_case(*shape, kind) + (shape[0], shape[1], None)
    return up_case(*shape, kind) + (shape[0], shape[1], shape[4:])


@pytest.mark.parametrize("where,shape", _cases())
@pytest.mark.parametrize("form", FORMS)
def test_all_ones_equals_the_unmasked_one_pass_kernel(form, where, shape):
    """Bit for bit: loss, cosines and gradient.  Several groups: each group against the unmasked call on that group alone (the unmasked
    channel-wise op has no groups; its value for the batch is another expression)."""
    x, t, m, G, C, geom = _load(where, shape, "ones")
    loss, cos, grad = hip(form, geom, x, t, m, G)
    for k in range(G):
        sl = slice(k * C, (k + 1) * C)
        l0, c0, g0 = hip(form, geom, x[sl], t[sl])
        ck = cos[k:k + 1] if form == "pixel" else cos[sl]
        assert torch.equal(c0, ck) and torch.equal(g0, grad[sl])
        if G == 1:
            assert torch.equal(l0, loss)
    assert float(grad.abs().max()) > 0


@pytest.mark.parametrize("kind", ["random", "single", "row"])
@pytest.mark.parametrize("where,shape", [(None, LOW_SHAPES[1]), (None, LOW_SHAPES[3]), ("up", UP_SHAPES[1]), ("up", UP_SHAPES[4])])
@pytest.mark.parametrize("form", FORMS)
def test_values_at_masked_out_pixels_are_never_used(form, where, shape, kind):
    """The target -- and, low resolution, the input -- overwritten at the masked-out pixels with NaN, Inf and 1e30: loss, cosines and
    gradient bit-equal to the clean run and finite.  A product with the mask instead of a select fails here (0 * Inf)."""
    x, t, m, G, C, geom = _load(where, shape, kind)
    clean = hip(form, geom, x, t, m, G)
    out = (m == 0).repeat_interleave(C, 0).reshape(t.shape)
    assert out.any() and all(torch.isfinite(v).all() for v in clean)
    for junk in (float("nan"), float("inf"), 1e30):
        tj, xj = t.clone(), x.clone()
        tj[out] = junk
        if where is None:
            xj[out] = -junk
        dirty = hip(form, geom, xj, tj, m, G)
        for u, v in zip(clean, dirty):
            assert torch.equal(u, v), (form, where, kind, junk)


@pytest.mark.parametrize("kind", ["random", "row"])
@pytest.mark.parametrize("shape", [UP_SHAPES[0], UP_SHAPES[1]])
@pytest.mark.parametrize("form", FORMS)
def test_upsampled_kernel_equals_separate_kernels(form, shape, kind):
    """The up-sampled masked op against the low-resolution masked op on ops.bicubic_upsample(x, crop): both obey the rule against float64,
    their direct distance is recorded."""
    from nefes_amd import ops
    x, t, m, G, C, geom = _load("up", shape, kind)
    OH, OW, crop = geom
    one = hip(form, geom, x, t, m)
    xd = x.to(DEV).requires_grad_()
    l2, c2 = op_of(form, None)(ops.bicubic_upsample(xd[None], (OH, OW), crop=crop)[0], t.to(DEV), mask=m.to(DEV), return_cos=True)
    (UP * l2).backward()
    two = (l2.detach(), c2, xd.grad)
    pp = form == "pixel"
    l64, g64 = truth(x, t, m[0], torch.float64, pp, (OH, OW), crop)
    l32, g32 = truth(x, t, m[0], torch.float32, pp, (OH, OW), crop)
    tag = f"masked_up_{form}_vs_separate[{','.join(str(v) for v in shape)}][{kind}]"
    for name, (loss, _, grad) in (("one pass", one), ("separate kernels", two)):
        P.check(tag, f"{name}: loss (abs) vs float64", abs(float(loss) - l64), abs(l32 - l64), tol=T_LOSS, factor=1.5)
        P.check(tag, f"{name}: d loss / d x vs float64", rel(grad.cpu().numpy(), g64), rel(g32, g64), tol=T_GRAD, factor=1.5)
    P.record(tag, "one pass vs separate kernels: loss (abs); d loss / d x (max-norm)", direct=abs(float(one[0]) - float(two[0])),
             e_hip=rel(one[2].cpu().numpy(), two[2].cpu().numpy()), bound=None)


@pytest.mark.parametrize("where,shape", [(None, LOW_SHAPES[3]), ("up", UP_SHAPES[4])])
@pytest.mark.parametrize("form", FORMS)
def test_three_groups_equal_three_single_calls(form, where, shape):
    """groups = 3 with three different masks: every group's cosines and gradient bit-equal to the call on that group alone (the
    group-to-mask-plane indexing), the value the sum of the three; and two calls give the same bits (no atomics, fixed order)."""
    x, t, m, G, C, geom = _load(where, shape, "random")
    assert G == 3 and not torch.equal(m[0], m[1])
    loss, cos, grad = hip(form, geom, x, t, m, G)
    total = 0.0
    for k in range(G):
        sl = slice(k * C, (k + 1) * C)
        l1, c1, g1 = hip(form, geom, x[sl], t[sl], m[k:k + 1])
        assert torch.equal(c1, cos[k:k + 1] if form == "pixel" else cos[sl]) and torch.equal(g1, grad[sl])
        total += group_loss(form, c1, 0, C)
        assert abs(float(l1) - group_loss(form, c1, 0, C)) <= 6e-8       # half an ulp of a float32 below 1
    # one rounding of a float64 sum below 4 (half an ulp: 2.4e-7); per pixel the kernel adds the groups' terms as written here: exact
    assert float(loss) == np.float32(total) if form == "pixel" else abs(float(loss) - total) <= 2.4e-7
    again = hip(form, geom, x, t, m, G)
    assert all(torch.equal(u, v) for u, v in zip((loss, cos, grad), again))
    if where == "up":                                                   # the [1, G*C, h, w] layout the refinement loop hands over
        l4, c4, g4 = hip(form, geom, x[None], t, m, G)
        assert torch.equal(l4, loss) and torch.equal(c4, cos) and torch.equal(g4[0], grad)


@pytest.mark.parametrize("where,shape", [(None, LOW_SHAPES[0]), ("up", UP_SHAPES[0])])
@pytest.mark.parametrize("form", FORMS)
def test_masked_losses_write_their_value_into_the_callers_buffer(form, where, shape):
    x, t, m, G, C, geom = _load(where, shape, "random")
    plain = hip(form, geom, x, t, m)
    buf = torch.full((), -7.0, device=DEV)
    into = hip(form, geom, x, t, m, out=buf)
    assert torch.equal(buf, plain[0]) and all(torch.equal(u, v) for u, v in zip(plain, into)) and not buf.requires_grad
    xd = x.to(DEV).requires_grad_()
    l = op_of(form, geom)(xd, t.to(DEV), mask=m.to(DEV), out=buf)
    assert l.data_ptr() == buf.data_ptr() and l.requires_grad
    for bad in (torch.zeros(1, device=DEV), torch.zeros((), device=DEV, dtype=torch.float64)):
        with pytest.raises(ValueError, match="`out`"):
            op_of(form, geom)(xd, t.to(DEV), mask=m.to(DEV), out=bad)


@pytest.mark.parametrize("where,shape", [(None, LOW_SHAPES[3]), ("up", UP_SHAPES[4])])
@pytest.mark.parametrize("form", FORMS)
def test_a_group_without_a_valid_pixel(form, where, shape):
    """Kernel level, as the reference's expression: channel-wise every cosine of the group is 0 (loss contribution 1) and its gradient
    0; per pixel the group's mean and the loss are NaN (0 / 0).  The other groups are what they are alone."""
    x, t, m, G, C, geom = _load(where, shape, "random")
    m = m.clone()
    m[1] = 0
    loss, cos, grad = hip(form, geom, x, t, m, G)
    if form == "pixel":
        assert torch.isnan(loss) and torch.isnan(cos[1]) and torch.isfinite(cos[[0, 2]]).all()
    else:
        assert float(cos[C:2 * C].abs().max()) == 0.0
        others = sum(group_loss(form, cos, k, C) for k in (0, 2))
        assert abs(float(loss) - (1.0 + others)) <= 2.4e-7
    assert float(grad[C:2 * C].abs().max()) == 0.0
    for k in (0, 2):
        sl = slice(k * C, (k + 1) * C)
        _, c1, g1 = hip(form, geom, x[sl], t[sl], m[k:k + 1])
        assert torch.equal(g1, grad[sl]) and torch.equal(c1, cos[k:k + 1] if form == "pixel" else cos[sl])
