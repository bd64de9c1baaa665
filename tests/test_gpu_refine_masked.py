"""PoseRefiner(masked=True) -- the reference's masked_feature_loss (`--semantic`, dm/DFM_pose_refine.py:257-288) -- on the library's
masked loss kernels in every form the loop has: low resolution, up-sampled, per pixel / per channel, `pose_model=`, images=B, two
streams.  The 30 x 40-ray fixture and the helpers of tests/test_gpu_refine_pp.py (refine50_pp.npz)."""
import numpy as np
import pytest
import torch

from tests import parity_log as P
from tests.test_gpu_refine_pp import DEV, T, TinyAPR, errors, nets, photo_of, refiner, rel, target_full

pytestmark = pytest.mark.gpu
T_LOSS, T_GRAD = 3e-7, 2e-6


def random_mask(shape, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < 0.6).to(torch.uint8)


def low_job(g, k=0, mask=None, target=None):
    return (T(g["init_c2w"][k]), T(g["target_low"]) if target is None else target, T(g["hist"])) + (() if mask is None else (mask,))


def up_target(g):
    return target_full(g)[:, 10:-10, 10:-10].contiguous()


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("upsample", [False, True])
def test_masked_iteration_with_the_kernels_equals_the_torch_glue(golden, upsample, per_pixel):
    """One iteration at a random mask.  The loss and d loss / d (fused features) of the kernel route against refine.masked_feature_loss
    (what fused_glue=False runs) on the same features in float64 on the CPU, by the rule (3e-7 absolute, 2e-6 of the max-norm, factor 1.5
    on the float32 CPU evaluation); then the whole iteration -- loss and (r, t) gradient -- against the fused_glue=False iteration: the
    loss by the assertion of tests/test_gpu_refine_pp.py's twin, the gradient within 1e-3 of its max-norm, the yardstick
    tests/test_gpu_refine50.py holds two fp32 evaluations of THIS scene's (r, t) gradient to (the two iterations differ in every glue
    kernel, not only in the loss: on this scene's sharp surfaces a handful of ReLU units and importance samples land on the other side of
    a kink; the twin's 2e-4 was set on the smooth 12 x 16 scene of refine.npz).  The same distance of the UNMASKED refiner is recorded
    beside it.  The masked kernels ARE taken: their timer keys are hit on the fused side only."""
    from nefes_amd import ops
    from nefes_amd.refine import masked_feature_loss
    g = golden("refine50_pp")
    shared = nets(g)
    tgt = up_target(g) if upsample else T(g["target_low"])
    mask = random_mask(tgt.shape[1:], 3)
    res = []
    for fused in (True, False):
        ref = refiner(g, graph=False, networks=shared, masked=True, per_pixel=per_pixel, upsample=upsample)
        ref.fused_glue = fused
        ref._reset(T(g["init_c2w"][0]).to(DEV), tgt.to(DEV), T(g["hist"]).to(DEV), mask)
        assert not ref._uses_prepared_target() and torch.equal(ref.mask[0].cpu(), mask)
        ops.TIMERS = {}
        try:
            loss = float(ref.loss_and_grad())
            keys = set(ops.TIMERS)
        finally:
            ops.TIMERS = None
        key = ("up" if upsample else "") + ("pixcos" if per_pixel else "cos" if upsample else "cosine") + "_loss_masked"
        assert ((key + "_fwd") in keys) == fused and ((key + "_bwd") in keys) == fused, (fused, sorted(keys))
        assert not ({"upcos_loss_fwd", "upcos_gram_fwd", "pixcos_loss_fwd", "uppixcos_loss_fwd"} & keys)
        if fused:
            assert loss == float(ref.loss)
        res.append((loss, torch.cat([ref.model.r.grad[0], ref.model.t.grad[0]]).cpu().numpy()))
        if fused:                                                       # the loss on its own, at this iteration's features
            feat = ref._fused().detach().requires_grad_()
            ref._fused = lambda: feat
            l_hip, _ = ref._loss()
            l_hip.backward()
            up = (lambda f: torch.nn.functional.interpolate(f, size=(ref.H, ref.W), mode="bicubic")[:, :, 10:-10, 10:-10]) if upsample else (lambda f: f)
            cpu = {}
            for dt in (torch.float64, torch.float32):
                f = feat.detach().cpu().to(dt).requires_grad_()
                l = masked_feature_loss(up(f)[0], tgt.to(dt), mask, per_pixel=per_pixel)
                l.backward()
                cpu[dt] = (float(l), f.grad.numpy())
            (l64, g64), (l32, g32) = cpu[torch.float64], cpu[torch.float32]
            tag = f"masked_refine_iteration[upsample={upsample},per_pixel={per_pixel}]"
            P.check(tag, "loss (abs) vs float64 torch on the CPU", abs(float(l_hip) - l64), abs(l32 - l64), tol=T_LOSS, factor=1.5)
            P.check(tag, "d loss / d fused features (max-norm)", rel(feat.grad.cpu().numpy(), g64), rel(g32, g64), tol=T_GRAD, factor=1.5)
    plain = []
    for fused in (True, False):
        ref = refiner(g, graph=False, networks=shared, per_pixel=per_pixel, upsample=upsample)
        ref.fused_glue = fused
        ref._reset(T(g["init_c2w"][0]).to(DEV), tgt.to(DEV), T(g["hist"]).to(DEV))
        ref.loss_and_grad()
        plain.append(torch.cat([ref.model.r.grad[0], ref.model.t.grad[0]]).cpu().numpy())
    (la, ga), (lb, gb) = res
    print(f"masked iteration, upsample={upsample}, per_pixel={per_pixel}: kernels {la:.8f} torch {lb:.8f}; gradient distance {rel(ga, gb):.2e} "
          f"(unmasked refiner: {rel(plain[0], plain[1]):.2e})")
    P.record(tag, "d loss / d (r, t), kernels vs torch glue (max-norm): masked; the unmasked refiner", direct=rel(ga, gb), e_ref=rel(plain[0], plain[1]),
             bound=1e-3)
    assert abs(la - lb) < 2e-4 * abs(lb) + 1e-7, (la, lb)
    assert rel(ga, gb) < 1e-3, (ga, gb)


def _job(g, form, mask_low, mask_full):
    """(refiner kwargs, call(refiner, iterations, target=None, masked=True)) of one of the loop's forms on the refine50_pp scene."""
    if form == "pose_model":
        return dict(apr=TinyAPR(g["m2_weight"][0], g["m2_bias"][0])), \
            lambda r, n, tgt=None, mask=True: r.refine_apr(photo_of(g), target_full(g) if tgt is None else tgt, T(g["hist"]), n,
                                                           **(dict(mask=mask_full) if mask else {}))[:2]
    if form == "upsampled":
        return dict(upsample=True), lambda r, n, tgt=None, mask=True: r.refine(T(g["init_c2w"][0]), up_target(g) if tgt is None else tgt[:, 10:-10, 10:-10],
                                                                               T(g["hist"]), n, **(dict(mask=mask_full) if mask else {}))
    return {}, lambda r, n, tgt=None, mask=True: r.refine(T(g["init_c2w"][0]), T(g["target_low"]) if tgt is None else tgt, T(g["hist"]), n,
                                                          **(dict(mask=mask_low) if mask else {}))


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("form", ["low_resolution", "upsampled", "pose_model"])
def test_masked_graph_equals_eager(golden, form, per_pixel):
    """8 iterations eager and as one replayed HIP graph per iteration at a random mask: poses and loss curves bit for bit."""
    g = golden("refine50_pp")
    shared = nets(g)
    H, W = (int(v) for v in g["hwf"][:2])
    ml, mf = random_mask(T(g["target_low"]).shape[1:], 5), random_mask((H - 20, W - 20), 6)
    out = {}
    for graph in (False, True):
        kw, call = _job(g, form, ml, mf)
        ref = refiner(g, graph=graph, networks=shared, masked=True, per_pixel=per_pixel, **kw)
        pose, losses = call(ref, 8)
        assert (getattr(ref, "apr_graph" if form == "pose_model" else "graph") is not None) == graph
        out[graph] = (pose.cpu().numpy(), losses.cpu().numpy())
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][1], out[True][1])
    assert np.isfinite(out[True][1]).all() and out[True][1][-1] < out[True][1][0]


def occluder(g, full):
    """(corrupted target, mask) -- a rectangle of randn features over about 25 % of the target and the mask of exactly that rectangle,
    at low resolution or (full) at full resolution with the mask in the cropped form."""
    tgt = (target_full(g) if full else T(g["target_low"])).clone()
    Hh, Ww = tgt.shape[1:]
    y0, y1, x0, x1 = Hh // 4, Hh // 4 + Hh // 2, Ww // 3, Ww // 3 + Ww // 2
    tgt[:, y0:y1, x0:x1] = torch.randn(tgt.shape[0], y1 - y0, x1 - x0, generator=torch.Generator().manual_seed(17))
    mask = torch.ones(Hh, Ww, dtype=torch.uint8)
    mask[y0:y1, x0:x1] = 0
    assert 0.2 < 1 - float(mask.float().mean()) < 0.3
    return tgt, (mask[10:-10, 10:-10].contiguous() if full else mask)


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("form", ["low_resolution", "pose_model"])
def test_masked_run_does_not_see_an_occluder(golden, form, per_pixel):
    """The masked run against the corrupted target is the masked run against the clean target: poses and losses torch.equal over 8
    iterations, in both modes (one captured refiner: the second image follows in place)."""
    g = golden("refine50_pp")
    full = form == "pose_model"
    bad, mask = occluder(g, full)
    kw, call = _job(g, form, mask, mask)
    shared = nets(g)
    ref = refiner(g, graph=True, networks=shared, masked=True, per_pixel=per_pixel, **kw)
    clean = [t.clone() for t in call(ref, 8)]
    dirty = call(ref, 8, tgt=bad)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1]) and torch.isfinite(clean[1]).all()
    blind = refiner(g, graph=True, networks=shared, per_pixel=per_pixel, **kw)            # the unmasked loop does see it
    assert not torch.equal(call(blind, 8, tgt=bad, mask=False)[1], clean[1])


@pytest.mark.parametrize("per_pixel", [False, True])
def test_occluder_pose_error_is_recorded(golden, per_pixel):
    """50 iterations from the fixture's perturbed start against the corrupted low-resolution target: the final pose error of the unmasked
    run beside the masked one's.  Recorded (DESIGN.md 4.7 quotes it), not asserted -- beyond both runs staying finite."""
    g = golden("refine50_pp")
    shared = nets(g)
    bad, mask = occluder(g, False)
    runs = {}
    for masked in (False, True):
        ref = refiner(g, graph=True, networks=shared, masked=masked, per_pixel=per_pixel)
        pose, losses = ref.refine(*low_job(g, 0, None, bad), iters=50, mask=mask if masked else None)
        assert torch.isfinite(pose).all() and torch.isfinite(losses).all()
        runs[masked] = errors(g, [pose[:3, :4].cpu().numpy()])[0]
    tag = f"masked_refine_occluder[per_pixel={per_pixel}]"
    for j, name in enumerate(("translation error [m]", "rotation error [deg]")):
        P.record(tag, name + " after 50 iterations against a target with a 25 % occluder", unmasked=runs[False][j], masked=runs[True][j],
                 initial=g["init_err"][0, j], bound=None)
    print(f"[{tag}] initial {g['init_err'][0]}  unmasked {runs[False]}  masked {runs[True]}")


@pytest.mark.parametrize("per_pixel,upsample", [(False, False), (True, True), (False, True)])
def test_masked_batch_of_two_equals_one_image_at_a_time(golden, per_pixel, upsample):
    """PoseRefiner(images=2, masked=True) with two different masks: each image walks the trajectory it walks alone with its own mask, by
    the rule of tests/test_gpu_refine_pp.py's twin (the batched convolutions are another fp32 rounding of the loop: losses equal to 2e-4
    over four iterations, poses to 2e-3) -- and NOT the trajectory of the other image's mask."""
    g = golden("refine50_pp")
    shared = nets(g)
    n = 4
    tgt = up_target(g) if upsample else T(g["target_low"])
    inits = torch.stack([T(g["init_c2w"][0]), T(g["init_c2w"][1])])
    targets = torch.stack([tgt, tgt + 0.05 * torch.randn(tgt.shape, generator=torch.Generator().manual_seed(11))])
    hists = torch.cat([T(g["hist"]), T(g["hist"]).flip(1)])
    masks = torch.stack([random_mask(tgt.shape[1:], 21), random_mask(tgt.shape[1:], 22)])
    masks[1, :tgt.shape[1] // 3] = 0                                    # (and the second image's top third is invalid)
    mk = lambda images: refiner(g, graph=True, networks=shared, masked=True, per_pixel=per_pixel, upsample=upsample, images=images)
    single, batch = mk(1), mk(2)
    alone = [[t.clone() for t in single.refine(inits[b], targets[b], hists[b][None], n, mask=masks[b])] for b in range(2)]
    swapped = single.refine(inits[0], targets[0], hists[0][None], n, mask=masks[1])[1].clone()
    poses, losses = batch.refine(inits, targets, hists, n, mask=masks)
    assert poses.shape == (2, 4, 4) and losses.shape == (n, 2)
    for b in range(2):
        p1, l1 = alone[b]
        assert rel(losses[:, b].cpu().numpy(), l1.cpu().numpy()) < 2e-4, (b, losses[:, b], l1)
        assert float((poses[b] - p1).abs().max()) < 2e-3, (b, (poses[b] - p1).abs().max())
    assert rel(losses[:, 0].cpu().numpy(), swapped.cpu().numpy()) > 2e-3          # the masks are not interchangeable at this tolerance


@pytest.mark.parametrize("form", ["low_resolution", "pose_model"])
def test_no_mask_on_a_masked_refiner_means_all_valid(golden, form):
    g = golden("refine50_pp")
    H, W = (int(v) for v in g["hwf"][:2])
    ones_l, ones_f = torch.ones(T(g["target_low"]).shape[1:]), torch.ones(H - 20, W - 20, dtype=torch.bool)
    kw, call = _job(g, form, ones_l, ones_f)
    ref = refiner(g, graph=True, networks=nets(g), masked=True, **kw)
    some = random_mask(ref.mask.shape[1:], 4)
    with_ones = [t.clone() for t in call(ref, 6)]
    ref._set_mask(some)                                                  # (a stale mask in the buffer must not survive mask=None)
    without = call(ref, 6, mask=False)
    assert torch.equal(with_ones[0], without[0]) and torch.equal(with_ones[1], without[1]) and bool(ref.mask.all())
    with pytest.raises(ValueError, match="no valid pixel"):
        ref._set_mask(torch.zeros(ref.mask.shape[1:]))


def test_one_captured_refiner_follows_the_masks_in_place(golden):
    """Two images with different masks alternate on ONE captured refiner: each gets the result a fresh refiner gives it -- the graph
    reads the mask buffer in place (and was captured once)."""
    g = golden("refine50_pp")
    shared = nets(g)
    tl = T(g["target_low"])
    masks = [random_mask(tl.shape[1:], 31), random_mask(tl.shape[1:], 32)]
    jobs = [low_job(g, k, masks[k]) for k in (0, 1)]
    fresh = []
    for job in jobs:
        r = refiner(g, graph=True, networks=shared, masked=True)
        fresh.append([t.clone() for t in r.refine(*job[:3], iters=6, mask=job[3])])
    one = refiner(g, graph=True, networks=shared, masked=True)
    graph = None
    for k in (0, 1, 0, 1):
        pose, losses = one.refine(*jobs[k][:3], iters=6, mask=jobs[k][3])
        assert torch.equal(pose, fresh[k][0]) and torch.equal(losses, fresh[k][1])
        assert graph is None or one.graph is graph
        graph = one.graph
    assert not torch.equal(fresh[0][1], fresh[1][1])


def test_two_masked_refiners_on_two_streams_equal_their_solo_runs(golden):
    """refine_concurrently with four-element jobs (the mask last): poses and loss curves identical to PoseRefiner.refine alone; a
    three-element job on a masked refiner means all valid."""
    from nefes_amd.refine import refine_concurrently
    g = golden("refine50_pp")
    shared = nets(g)
    tl = T(g["target_low"])
    n = 8
    refs = [refiner(g, graph=True, networks=shared, bn_running_stats=False, masked=True) for _ in (0, 1)]
    jobs = [low_job(g, k, random_mask(tl.shape[1:], 41 + k)) for k in (0, 1)]
    solo = [[t.clone() for t in r.refine(*job[:3], iters=n, mask=job[3])] for r, job in zip(refs, jobs)]
    outs = refine_concurrently(refs, jobs, iters=n)
    for (p, l), (ps, ls) in zip(outs, solo):
        assert torch.equal(p, ps) and torch.equal(l, ls)
    assert not torch.equal(solo[0][1], solo[1][1])
    plain = [[t.clone() for t in r.refine(*job[:3], iters=n)] for r, job in zip(refs, jobs)]
    for (p, l), (ps, ls) in zip(refine_concurrently(refs, [job[:3] for job in jobs], iters=n), plain):
        assert torch.equal(p, ps) and torch.equal(l, ls)
