"""The train-loss kernels (csrc/losses.hip, ops.TrainLoss, nefes_amd/losses.py) against float64.

Truth: the reference's own float64 run where the fixture tests/golden/losses.npz has the case, tests/loss_ref.py in float64 (pinned on
that fixture by tests/test_losses_golden.py) at every other shape.  Bound: tests/parity_log.py's max(tol, 1.5 e_ref) with e_ref the
distance of the float32 torch expressions from float64 and tol = 1e-6 -- of the value for a scalar, of the tensor's largest float64
gradient magnitude for a gradient.  The kernels round a float64 result to float32 once (6e-8); the reference's float32 run sits 1e-8 ..
9e-8 from its float64 run at N = 6144, C = S = 128, so 1e-6 leaves an order of magnitude and hides nothing."""
import os
import types

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-6

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))
BASE = {k[3:]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("in.")}
CASES = R.fixture_cases(Z)


def _module(name, kw):
    from nefes_amd import losses
    ctor = dict(coef=kw.get("coef", 1))
    if name in ("nerfw", "color_feat_fusion_nerfw"):
        ctor["lambda_u"] = kw.get("lambda_u", 0.01)
    if name != "color" and name != "nerfw":
        ctor["L1_loss"] = kw.get("L1_loss", False)
    if name == "color_feat_fusion":
        ctor["cos_loss"] = kw.get("cos_loss", False)
    return losses.loss_dict[name](**ctor)


def _call(fn, name, kw, inputs, rgb_t, feat_t):
    """The module called the way run_nefes.py:237-251 calls it; always a tuple."""
    if name in ("color", "nerfw"):
        ret = fn(inputs, rgb_t)
    elif name == "color_feat":
        ret = fn(inputs, {"rgb": rgb_t, "feat": feat_t})
    else:
        targets = {"rgb": rgb_t} if kw.get("color_only_switch") else {"rgb": rgb_t, "feat": feat_t}      # feature keys must not be touched
        ret = fn(inputs, targets, switch_on=kw.get("switch_on", True), color_only_switch=kw.get("color_only_switch", False))
    return ret if isinstance(ret, tuple) else (ret,)


def _hip(name, kw, base, keys, weights=R.WEIGHTS):
    inputs = {k: base[k].detach().to(DEV).clone().requires_grad_() for k in R.NAMES if k in keys}
    ret = _call(_module(name, kw), name, kw, inputs, base["rgb_target"].to(DEV), base["feat_target"].to(DEV))
    R.total(ret, weights).backward()
    return [r.detach() for r in ret], {k: v.grad for k, v in inputs.items() if v.grad is not None}


def _hold(tag, what, got, ref32, ref64, scale=None):
    got, ref32, ref64 = (np.asarray(torch.as_tensor(v).detach().cpu().double().numpy()) for v in (got, ref32, ref64))
    assert got.shape == ref64.shape, (tag, what, got.shape, ref64.shape)
    sc = float(np.abs(ref64).max()) if scale is None else scale
    if sc == 0:                                                        # a gradient that is zero everywhere (every element a tie)
        assert float(np.abs(got).max()) == 0, (tag, what)
        return
    e_hip, e_ref = float(np.abs(got - ref64).max()) / sc, float(np.abs(ref32 - ref64).max()) / sc
    print(f"{tag}: {what}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} bound {P.bound(e_ref, TOL):.3e}")
    P.check(tag, what, e_hip, e_ref, direct=float(np.abs(got - ref32).max()) / sc, tol=TOL)


def _compare(tag, got, ref32, ref64, scales=None):
    (ret, grads), (ret32, grads32), (ret64, grads64) = got, ref32, ref64
    assert len(ret) == len(ret64)
    for i, r in enumerate(ret):
        assert r.dim() == 0 and r.dtype == torch.float32
        _hold(tag, f"scalar {i}", r, ret32[i], ret64[i])
    assert set(grads) == set(grads64), (tag, set(grads) ^ set(grads64))
    for k in grads64:
        _hold(tag, f"d {k}", grads[k], grads32[k], grads64[k], None if scales is None else scales.get(k))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_fixture_cases(case):
    """Every case the reference wrote: scalars and every gradient against its float64 run; e_ref is its own float32 run."""
    i, name, kw, keys = case
    got = _hip(name, kw, BASE, keys)
    pick = lambda tag: ([torch.tensor(v) for v in Z[f"case{i}.out{tag}"]],
                        {k[len(f"case{i}.g."):len(k) - len(tag)]: torch.from_numpy(Z[k]) for k in Z.files
                         if k.startswith(f"case{i}.g.") and k.endswith("_f64") == bool(tag)})
    _compare(f"losses_fixture[{i}-{name}]", got, pick(""), pick("_f64"))


def _random_base(N, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    b = {"rgb_fine": torch.rand(N, 3, generator=g), "rgb_coarse": torch.rand(N, 3, generator=g), "rgb_target": torch.rand(N, 3, generator=g),
         "beta": 0.3 + torch.rand(N, generator=g), "transient_sigmas": 2.0 * torch.rand(N, S, generator=g),
         "feat_fine": torch.randn(N, C, generator=g), "feat_coarse": torch.randn(N, C, generator=g),
         "feat_fusion": torch.randn(N, C, generator=g), "feat_target": torch.randn(N, C, generator=g)}
    if N * C > 2:                                                     # exact ties for L1, first and last element
        b["feat_fine"][0, 0] = b["feat_target"][0, 0]
        b["feat_fusion"][N - 1, C - 1] = b["feat_target"][N - 1, C - 1]
    return b


ROWS = 16           # lib.TRAIN_LOSS_ROWS (asserted below): rays per block of the kernels
SHAPES = [(1, 1, 1), (1, 141, 192), (ROWS - 1, 16, 64), (ROWS, 141, 1), (ROWS + 1, 1, 192), (ROWS + 1, 16, 64), (65, 141, 192), (65, 16, 1),
          (6144, 128, 128)]
KINDS = [("color_feat_fusion_nerfw", dict(coef=1, L1_loss=True, lambda_u=0.01), R.NAMES),
         ("color_feat_fusion_nerfw", dict(coef=1, L1_loss=False, lambda_u=0.01), R.NAMES),
         ("color_feat_fusion", dict(coef=1, cos_loss=True), [n for n in R.NAMES if n not in ("beta", "transient_sigmas")])]


@pytest.mark.parametrize("N,C,S", SHAPES)
def test_shapes_where_a_reduction_or_a_tail_can_go_wrong(N, C, S):
    """One ray, one below / at / one above the kernels' block of rays, several blocks, the reference's batch; channel and sample counts
    of 1, below, at and above a wave's 64 lanes.  All three feature kinds (L1 and MSE share the element loop, COS has its own rows)."""
    from nefes_amd import lib as L
    assert L.TRAIN_LOSS_ROWS == ROWS
    base = _random_base(N, C, S, 1000 + N + C + S)
    for name, kw, keys in KINDS:
        ref32, ref64 = R.run(name, kw, base, keys, dtype=torch.float32), R.run(name, kw, base, keys, dtype=torch.float64)
        scales = None
        if kw.get("cos_loss") and C == 1:
            # one channel: cos = +-1 and its gradient b / (|a||b|) - (a.b) a / (|a|^3 |b|) is zero in exact arithmetic, so what any
            # implementation returns is the rounding residue of two cancelling terms of size w / (N |a_n|) each: that is the scale
            scales = {k: float((0.02 / (N * base[k].double().abs())).max()) for k in ("feat_fine", "feat_coarse", "feat_fusion")}
        _compare(f"losses_shape[{N},{C},{S},{name},{'l1' if kw.get('L1_loss') else 'cos' if kw.get('cos_loss') else 'mse'}]",
                 _hip(name, kw, base, keys), ref32, ref64, scales)


@pytest.mark.parametrize("N,C,S,Rr,ch", [(ROWS + 1, 16, 64, 9, 7), (65, 5, 7, 3, 2)])
def test_strided_sigmas_are_read_in_place_and_their_gradient_is_one_number(N, C, S, Rr, ch):
    """transient_sigmas as render() hands it out: raw[:, ch, :] of an [N, R, S] tensor (row stride R S).  No copy: the tensor the
    kernels read is the view's own memory; the gradient reaches the view as a stride-0 expansion of one float.  rgb_fine is a
    non-contiguous column slice: the wrapper makes it contiguous, it does not refuse."""
    base = _random_base(N, C, S, 7)
    name, kw, keys = KINDS[0]
    ref32, ref64 = R.run(name, kw, base, keys, dtype=torch.float32), R.run(name, kw, base, keys, dtype=torch.float64)
    raw = torch.rand(N, Rr, S, generator=torch.Generator().manual_seed(3)).to(DEV)
    raw[:, ch, :] = base["transient_sigmas"].to(DEV)
    raw.requires_grad_()
    wide = torch.rand(N, 4).to(DEV)
    wide[:, :3] = base["rgb_fine"].to(DEV)
    wide.requires_grad_()
    inputs = {k: base[k].to(DEV).clone().requires_grad_() for k in keys if k not in ("transient_sigmas", "rgb_fine")}
    view, rgb_fine = raw[:, ch, :], wide[:, :3]
    assert not view.is_contiguous() and view.stride() == (Rr * S, 1) and not rgb_fine.is_contiguous()
    inputs["transient_sigmas"], inputs["rgb_fine"] = view, rgb_fine
    seen = []
    view.register_hook(lambda g: seen.append((tuple(g.shape), g.stride(), g.untyped_storage().nbytes())))
    ret = _call(_module(name, kw), name, kw, inputs, base["rgb_target"].to(DEV), base["feat_target"].to(DEV))
    read = ret[0].grad_fn.tensors[4]                                  # what ops.TrainLoss handed to the kernels
    assert read.data_ptr() == view.data_ptr() == raw.data_ptr() + 4 * ch * S and read.stride() == (Rr * S, 1)
    R.total(ret).backward()
    assert seen == [((N, S), (0, 0), 4)], seen
    g_raw = raw.grad.clone()
    g_sig = g_raw[:, ch, :].clone()
    g_raw[:, ch, :] = 0
    assert float(g_raw.abs().max()) == 0.0                            # the other channels of raw got nothing
    grads = {k: v.grad for k, v in inputs.items() if v.is_leaf}
    grads["transient_sigmas"], grads["rgb_fine"] = g_sig, wide.grad[:, :3]
    assert float(wide.grad[:, 3].abs().max()) == 0.0
    _compare(f"losses_strided[{N},{C},{S}]", ([r.detach() for r in ret], grads), ref32, ref64)


def test_outputs_can_be_modified_in_place():
    """`loss += ...` on a returned loss (the reference's own classes write that) works: the outputs are not views of one another."""
    name, kw, keys = KINDS[0]
    base = _random_base(33, 16, 64, 11)
    inputs = {k: base[k].to(DEV).clone().requires_grad_() for k in keys}
    loss, loss_f, loss_fusion = _call(_module(name, kw), name, kw, inputs, base["rgb_target"].to(DEV), base["feat_target"].to(DEV))
    before = float(loss_f), float(loss_fusion)
    want = float(loss) + 0.02 * before[0]
    loss_f *= 0.02
    loss += loss_f
    assert abs(float(loss) - want) <= 1e-6 * abs(want) and float(loss_fusion) == before[1]
    loss.backward()
    ref = _hip(name, kw, base, keys, weights=(1.0, 0.02))[1]
    for k in ref:
        assert torch.equal(inputs[k].grad, ref[k]), k


def test_non_float32_and_cpu_inputs_raise():
    from nefes_amd import losses
    fn = losses.ColorLoss()
    t = torch.rand(5, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        fn({"rgb_fine": torch.rand(5, 3)}, t)
    with pytest.raises(RuntimeError, match="float32"):
        fn({"rgb_fine": torch.rand(5, 3, dtype=torch.float64, device=DEV)}, t.to(DEV))
    with pytest.raises(KeyError):
        losses.NerfWLoss()({"rgb_fine": t.to(DEV)}, t.to(DEV))          # rgb_coarse is required, as in the reference


def test_upstream_gradients_and_an_unused_output():
    """Weights (1, 0.04, 0.02) on the three outputs, coef != 1, lambda_u != 0.01; then loss_fusion left out of the total: a None reaches
    the backward, feat_fusion gets no gradient at all (not a zero-filled one) and everything else is unchanged."""
    base = _random_base(33, 16, 64, 11)
    name, keys = "color_feat_fusion_nerfw", R.NAMES
    kw = dict(coef=0.7, L1_loss=True, lambda_u=0.05)
    w = (1.0, 0.04, 0.02)
    ref32, ref64 = R.run(name, kw, base, keys, dtype=torch.float32, weights=w), R.run(name, kw, base, keys, dtype=torch.float64, weights=w)
    _compare("losses_upstream[1,0.04,0.02]", _hip(name, kw, base, keys, weights=w), ref32, ref64)
    w2 = (1.0, 0.04)                                                    # zip() stops there: loss_fusion is unused
    got = _hip(name, kw, base, keys, weights=w2)
    assert "feat_fusion" not in got[1] and len(got[0]) == 3
    drop = lambda run: (run[0], {k: v for k, v in run[1].items() if k != "feat_fusion"})
    r32, r64 = (R.run(name, kw, base, keys, dtype=d, weights=(1.0, 0.04, 0.0)) for d in (torch.float32, torch.float64))
    _compare("losses_upstream[1,0.04,unused]", got, drop(r32), drop(r64))
    # loss_f alone: the colour inputs and feat_fusion get no gradient at all
    inputs = {k: base[k].to(DEV).clone().requires_grad_() for k in keys}
    ret = _call(_module(name, kw), name, kw, inputs, base["rgb_target"].to(DEV), base["feat_target"].to(DEV))
    (0.04 * ret[1]).backward()
    assert {k for k, v in inputs.items() if v.grad is not None} == {"feat_fine", "feat_coarse"}
    for k in ("feat_fine", "feat_coarse"):
        assert torch.equal(inputs[k].grad, got[1][k])


def _bits(run):
    ret, grads = run
    return [r.cpu().numpy().tobytes() for r in ret] + [grads[k].contiguous().cpu().numpy().tobytes() for k in sorted(grads)]


@pytest.mark.parametrize("which", [0, 2])
def test_same_bits_from_call_to_call_and_from_a_captured_graph(which):
    """Fixed-order sums: the same call twice gives the same bits; one forward + backward captured on one stream and replayed once gives
    the eager bits too (no host read, no allocation outside torch's allocator in either direction)."""
    name, kw, keys = KINDS[which]
    base = _random_base(6144, 128, 128, 5)
    first = _hip(name, kw, base, keys)
    assert _bits(first) == _bits(_hip(name, kw, base, keys))
    leaves = {k: base[k].to(DEV).clone().requires_grad_() for k in keys}
    rgb_t, feat_t = base["rgb_target"].to(DEV), base["feat_target"].to(DEV)
    fn = _module(name, kw)

    def step():
        ret = _call(fn, name, kw, leaves, rgb_t, feat_t)
        return ret, torch.autograd.grad(R.total(ret), [leaves[k] for k in keys])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ret, grads = step()
    for t in list(ret) + list(grads):
        if t.is_contiguous():
            t.detach().zero_()                                          # what the replay writes is what is compared
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(([r.detach() for r in ret], dict(zip(keys, grads)))) == _bits(first)


def test_one_training_step_through_render():
    """run_nefes.py's ray stage in small: a train-mode render() of 64 rays, 16 + 16 samples, width 128, NeRF-W on, then
    ColorFeatureFusionNerfWLoss of nefes_amd.losses; the same step again (same weights, perturb = 0: the same forward) with the torch
    expressions of tests/loss_ref.py in float32 on the GPU, which is what the step runs without the kernels.  The loss within 1e-6; every
    weight gradient within the suite's train-mode rule (tests/test_gpu_train.py: 2e-4 of the gradient's own largest magnitude)."""
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.render import render
    from oracle import ref_cpu as O
    H, W, focal, Nc, Ni, Wd, C = 8, 8, 12.0, 16, 16, 128, 128
    torch.manual_seed(0)
    coarse = NeRFH_NFF('coarse', W=Wd, f_dim=C).to(DEV)
    fine = NeRFH_NFF('fine', W=Wd, f_dim=C, encode_appearance=True, encode_transient=True).to(DEV)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True)
    kwr = dict(network_query_fn=None, perturb=0., N_importance=Ni, N_samples=Nc, network_fn=coarse, network_fine=fine,
               use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=False, args=args, ndc=False, lindisp=False)
    rays_o, rays_d = O.ray_bundle(H, W, focal, O.bench_pose())
    gen = torch.Generator().manual_seed(4)
    t_rgb, t_feat = torch.rand(H * W, 3, generator=gen).to(DEV), torch.randn(H * W, C, generator=gen).to(DEV)
    kw = dict(coef=1, L1_loss=True, lambda_u=0.01, switch_on=False)
    fn = _module("color_feat_fusion_nerfw", kw)
    params = [(n, p) for net in (coarse, fine) for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]

    def step(kernels):
        for _, p in params:
            p.grad = None
        rgb, _, _, ex = render(H, W, focal, rays=(rays_o.to(DEV), rays_d.to(DEV)), near=0., far=4., **kwr)
        results = {"rgb_fine": rgb, "rgb_coarse": ex["rgb0"], "feat_fine": ex["feat_map"], "beta": ex["beta"],
                   "transient_sigmas": ex["transient_sigmas"]}
        assert ex["transient_sigmas"].shape == (H * W, Nc + Ni) and not ex["transient_sigmas"].is_contiguous()
        if kernels:
            loss, loss_f = fn(results, {"rgb": t_rgb, "feat": t_feat}, switch_on=False, color_only_switch=False)
        else:
            loss, loss_f = R.evaluate("color_feat_fusion_nerfw", results, t_rgb, t_feat, **kw)
        total = loss + 0.04 * loss_f                                    # run_nefes.py:246-248
        total.backward()
        return float(total.detach()), {i: p.grad.clone() for i, (_, p) in enumerate(params) if p.grad is not None}

    la, ga = step(True)
    lb, gb = step(False)
    print(f"train step: loss {la!r} (kernels) {lb!r} (torch fp32)")
    assert abs(la - lb) <= 1e-6 * abs(lb)
    assert set(ga) == set(gb) and len(gb) >= 24
    worst = ("", 0.0)
    for i, g in gb.items():
        if float(g.abs().max()) > 0:
            worst = max(worst, (params[i][0], float((ga[i] - g).abs().max() / g.abs().max())), key=lambda t_: t_[1])
    print("train step: worst weight gradient", worst)
    P.record("losses_train_step", "worst weight gradient, kernels vs torch fp32 losses", direct=worst[1], bound=2e-4)
    assert worst[1] < 2e-4, worst
