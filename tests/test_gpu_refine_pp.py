"""PoseRefiner(per_pixel=True) -- the reference's `--per_pixel` feature loss (dm/options.py:73, FeatureLoss(per_pixel=True)) -- on the
library's own kernels (ops.pixel_cosine_loss / ops.upsampled_pixel_cosine_loss) in every form the loop has: low resolution, up-sampled,
`pose_model=` (train_on_batch, the shipped default mode), images=B, two streams.  Fixtures: refine.npz, refine50.npz (the scene) and
refine50_pp.npz -- two starts x 50 iterations of the reference's own per-pixel `train_on_batch` (tests/test_refine50_pp_oracle.py pins
it and measures the yardstick D_l, D_g used below: the float32 oracle's own distance from the reference's numbers)."""
import numpy as np
import pytest
import torch

from oracle import refine_cpu as RC
from tests import branch as B
from tests import parity_log as P
from tests.test_gpu_refine50 import LOOP_SUFFIX, TinyAPR, conv_audit, errors, nets, refiner, target_full
from tests.test_refine50_oracle import photo_of, problem, rel
from tests.test_refine50_pp_oracle import ITERATIONS, oracle_distances, per_pixel_oracle, weights_before

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))


def test_per_pixel_iteration_with_the_kernels_equals_the_torch_glue(golden):
    """One PoseRefiner iteration with the glue kernels == the same iteration with the torch expressions (fused_glue=False keeps
    refine.feature_loss(per_pixel=True)), low resolution and up-sampled + 10 px crop: loss and (r, t) gradient, by the assertions of
    tests/test_gpu_refine.py::test_fused_glue_iteration_equals_torch_glue -- and the kernel path IS taken: the new forward's timer key
    was hit on the fused side and not on the other (before the kernels existed both sides ran the torch loss)."""
    from nefes_amd import ops
    from tests.test_gpu_refine import refiner as refiner12
    g = golden("refine")
    H, W, _ = g["hwf"].tolist()
    for up in (False, True):
        res = []
        for fused in (True, False):
            ref = refiner12(g, graph=False)
            ref.fused_glue, ref.upsample, ref.per_pixel = fused, up, True
            tgt = T(g["target"]).to(DEV)
            if up:
                tgt = ops.bicubic_upsample(tgt[None], (int(H), int(W)), crop=10)[0]
                ref.target = torch.zeros_like(tgt)
            ref._reset(T(g["init_c2w"]).to(DEV), tgt, T(g["hist"]).to(DEV))
            with torch.no_grad():
                ref.model.r.copy_(T(g["r"][3]).reshape(1, 3))
                ref.model.t.copy_(T(g["t"][3]).reshape(1, 3))
            assert not ref._uses_prepared_target()
            ops.TIMERS = {}
            try:
                loss = float(ref.loss_and_grad())
                keys = set(ops.TIMERS)
            finally:
                ops.TIMERS = None
            key = "uppixcos_loss" if up else "pixcos_loss"
            assert ((key + "_fwd") in keys) == fused and ((key + "_bwd") in keys) == fused, (up, fused, sorted(keys))
            assert not ({"upcos_loss_fwd", "upcos_gram_fwd"} & keys)
            if fused:
                assert loss == float(ref.loss)                           # (`out=`: the kernel wrote the refiner's static buffer)
            res.append((loss, torch.cat([ref.model.r.grad[0], ref.model.t.grad[0]]).cpu().numpy()))
        (la, ga), (lb, gb) = res
        print(f"per-pixel iteration, upsample={up}: kernels {la:.8f} torch {lb:.8f}; gradient distance {rel(ga, gb):.2e}")
        assert abs(la - lb) < 2e-4 * abs(lb) + 1e-7, (up, la, lb)
        assert rel(ga, gb) < 2e-4, (up, ga, gb)


def _job(g, form):
    """(refiner kwargs, call) of one of the loop's forms on the refine50 scene."""
    if form == "pose_model":
        return dict(apr=TinyAPR(g["m2_weight"][0], g["m2_bias"][0])), lambda r, n: r.refine_apr(photo_of(g), target_full(g), T(g["hist"]), n)[:2]
    if form == "upsampled":
        tgt = target_full(g)[:, 10:-10, 10:-10].contiguous()
        return dict(upsample=True), lambda r, n: r.refine(T(g["init_c2w"][0]), tgt, T(g["hist"]), n)
    return {}, lambda r, n: r.refine(T(g["init_c2w"][0]), T(g["target_low"]), T(g["hist"]), n)


@pytest.mark.parametrize("form", ["low_resolution", "upsampled", "pose_model"])
def test_per_pixel_graph_equals_eager(golden, form):
    """12 iterations eager and as one replayed HIP graph per iteration, LearnPose mode (both resolutions) and `pose_model` mode: the same
    arithmetic -- poses and loss curves bit for bit; the loss falls."""
    g = golden("refine50_pp")
    out = {}
    for graph in (False, True):
        kw, call = _job(g, form)
        ref = refiner(g, graph=graph, per_pixel=True, **kw)
        pose, losses = call(ref, 12)
        assert (getattr(ref, "apr_graph" if form == "pose_model" else "graph") is not None) == graph
        out[graph] = (pose.cpu().numpy(), losses.cpu().numpy())
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][1], out[True][1])
    losses = out[True][1]
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses
    if form == "pose_model":                                            # ... and it is the reference's curve
        assert rel(losses, g["m2_loss"][0, :12]) < 2e-3


@pytest.mark.parametrize("graph,upsample", [(False, False), (True, True)])
def test_per_pixel_batch_of_two_equals_one_image_at_a_time(golden, graph, upsample):
    """PoseRefiner(images=2, per_pixel=True): two query images (different initial poses, targets, histograms) side by side walk the
    trajectories they walk alone, by the rule of tests/test_gpu_refine.py::test_batched_refinement_equals_one_image_at_a_time (the
    batched convolutions are another fp32 rounding of the loop: losses equal to 2e-4 over four iterations, poses to 2e-3 after four and
    to 2e-5 after two); the per-image losses come back as [iters, 2]."""
    from nefes_amd import ops
    from nefes_amd.refine import PoseRefiner
    from tests.test_gpu_refine import refiner as refiner12
    g = golden("refine")
    Bn, n = 2, 4
    gen = torch.Generator().manual_seed(11)
    inits = T(g["init_c2w"])[None].repeat(Bn, 1, 1).clone()
    inits[1, :3, 3] += torch.tensor([0.05, -0.02, 0.03])
    targets = T(g["target"])[None].repeat(Bn, 1, 1, 1).clone()
    targets[1] += 0.05 * torch.randn(targets[1].shape, generator=gen)
    hists = torch.stack([T(g["hist"])[0], T(g["hist"])[0].flip(0)])
    base = refiner12(g, graph=False)
    if upsample:
        targets = ops.bicubic_upsample(targets.to(DEV), (base.H, base.W), crop=10).cpu()
    mk = lambda images: PoseRefiner(base.kw, base.args, (base.H, base.W, base.focal * (base.H // base.h)), base.near, base.far,
                                    tinyscale=base.H // base.h, lr_r=float(g["lr"][0]), lr_t=float(g["lr"][1]), world_setup=base.world_setup,
                                    graph=graph, device=DEV, images=images, per_pixel=True, upsample=upsample)
    single, batch = mk(1), mk(Bn)
    alone = [single.refine(inits[b], targets[b], hists[b][None], n) for b in range(Bn)]
    alone = [(p.clone(), l.clone()) for p, l in alone]
    poses, losses = batch.refine(inits, targets, hists, n)
    assert poses.shape == (Bn, 4, 4) and losses.shape == (n, Bn)
    for b in range(Bn):
        p1, l1 = alone[b]
        assert rel(losses[:, b].cpu().numpy(), l1.cpu().numpy()) < 2e-4, (b, losses[:, b], l1)
        assert float((poses[b] - p1).abs().max()) < 2e-3, (b, (poses[b] - p1).abs().max())
    assert not torch.equal(losses[:, 0], losses[:, 1])
    poses2, _ = batch.refine(inits, targets, hists, 2)                  # re-uses the captured graph
    for b in range(Bn):
        p1, _ = single.refine(inits[b], targets[b], hists[b][None], 2)
        assert float((poses2[b] - p1).abs().max()) < 2e-5, (b, (poses2[b] - p1).abs().max())


def test_per_pixel_mode2_iterations_match_reference_along_its_trajectory(golden):
    """Teacher-forced `train_on_batch` with FeatureLoss(per_pixel=True), start 0, all 50 iterations of tests/golden/refine50_pp.npz, the
    oracle's loss wrapped to per-pixel.  At iterations 0, 20, 49: the loss by the rule (tol 2e-4, factor 3) against float64, the gradient
    to the twelve regressed numbers branch-pinned (tests/branch.py: e_hip <= max(1e-4, 1.5 e_ref), in units of |g| at iteration 0, the
    oracle at the twelve numbers the kernels' pose came from).  Over all iterations against the reference's own fp32 numbers: loss within
    max(1e-3, 3 D_l), gradient within max(1e-3, 3 D_g) in first-iteration units -- D_l, D_g the float32 ORACLE's distances from the same
    fixture (tests/test_refine50_pp_oracle.oracle_distances, recomputed here on the CPU: never taken from the code under test)."""
    g = golden("refine50_pp")
    k = 0
    _, D_l, D_g = oracle_distances()
    bound_l, bound_g = max(1e-3, 3 * D_l), max(1e-3, 3 * D_g)
    apr = TinyAPR(g["m2_weight"][k], g["m2_bias"][k])
    ref = refiner(g, apr=apr, per_pixel=True)
    photo, tgt = photo_of(g), target_full(g)
    ref.refine_apr(photo, tgt, T(g["hist"]), iters=0, verification=False)          # loads the image's buffers
    probs = {dt: problem(g, dt, k, 2) for dt in (torch.float64, torch.float32)}
    Wd = int(g["Wd"])
    g0 = float(np.abs(g["m2_grad"][k, 0]).max())                     # the loop's gradient unit: max-norm at its first iteration
    worst_g = worst_l = worst_abs = 0.
    with per_pixel_oracle():
        for i in range(g["m2_loss"].shape[1]):
            Wn, bn = weights_before(g, k, i)
            with torch.no_grad():
                ref.apr.fc.weight.copy_(T(Wn))
                ref.apr.fc.bias.copy_(T(bn))
            with B.tapped() as tap:
                loss, _ = ref._loss()
            loss.backward()
            grad = ref.apr.raw.grad[0].cpu().numpy()
            lossf = float(loss.detach())
            direct = rel(grad, g["m2_grad"][k, i])
            dl = abs(lossf - float(g["m2_loss"][k, i])) / float(g["m2_loss"][k, i])
            worst_g, worst_l = max(worst_g, direct), max(worst_l, dl)
            worst_abs = max(worst_abs, float(np.abs(grad - g["m2_grad"][k, i]).max()) / g0)
            if i in ITERATIONS:
                raw_hip = ref.apr.raw.detach()[0].cpu()
                conv_pos, aud = [(y > 0).cpu() for y in tap["conv_relu"][-3:]], {}

                def oracle_at(dt, act=None, zf=None):
                    r = raw_hip.to(dt).clone().requires_grad_()
                    pin = {} if act is None else dict(fine_act=act, z_fine=zf, conv_pos=conv_pos, conv_audit=aud if dt == torch.float64 else None)
                    l = probs[dt].loss_at_pose(RC.svd_reg(r.reshape(3, 4)), **pin)
                    return l.detach(), torch.autograd.grad(l, r)[0]
                l64, g64 = oracle_at(torch.float64)
                tag = f"refine50_pp_mode2_iteration[{k},{i}]"
                P.record(tag, "d loss / d (12 regressed numbers), UNPINNED", e_hip=rel(grad, g64.numpy()), e_ref=rel(g["m2_grad"][k, i], g64.numpy()),
                         direct=direct, bound=None)
                P.check(tag, "loss", abs(lossf - float(l64)) / float(l64), abs(float(g["m2_loss"][k, i]) - float(l64)) / float(l64), dl, tol=2e-4,
                        factor=3.0)
                B.pinned_gradients(tag, {"d loss / d (12 regressed numbers)": torch.from_numpy(grad)}, tap, Wd,
                                   lambda dt, act, zf: {"d loss / d (12 regressed numbers)": oracle_at(dt, act, zf)[1]}, scale=g0,
                                   suffix=LOOP_SUFFIX)
                conv_audit(tag, aud)
    P.record(f"refine50_pp_mode2_iteration[{k},all]", "worst over 50 iterations vs the reference's fp32: gradient in units of |g| at iteration 0; "
             "gradient relative to its own norm (unbounded); loss", direct=worst_abs, e_hip=worst_g, e_ref=worst_l, bound=bound_g)
    print(f"per-pixel mode 2, teacher-forced, worst of 50 iterations vs the reference: loss {worst_l:.2e} (bound {bound_l:.1e}; D_l {D_l:.1e}), gradient "
          f"{worst_abs:.2e} of |g| at iteration 0 (bound {bound_g:.1e}; D_g {D_g:.1e}), {worst_g:.2e} of its own norm")
    assert worst_l <= bound_l and worst_abs <= bound_g, (worst_l, worst_abs, worst_g, D_l, D_g)


@pytest.mark.parametrize("graph", [False, True])
def test_per_pixel_mode2_free_running_runs(golden, graph):
    """Free-running per-pixel `train_on_batch` x 50 + the roll-back rule from both starts of refine50_pp, eager and as one replayed graph:
    no retreat (as the reference on this fixture), the loss curve within max(1e-3, 3 D_l) of the reference's (max-norm of the curve, as
    the free-running tests of tests/test_gpu_refine50.py), the final pose within max(1e-3, 1.5 e_ref) of the float64 oracle's, and the
    reference's pose-error metric within 1 % of the reference's run PER START (two starts: a median would say nothing)."""
    g = golden("refine50_pp")
    _, D_l, _ = oracle_distances()
    photo, tgt, n = photo_of(g), target_full(g), g["m2_loss"].shape[1]
    tag = f"refine50_pp_mode2[{'graph' if graph else 'eager'}]"
    ref = None
    for k in range(len(g["init_c2w"])):
        apr = TinyAPR(g["m2_weight"][k], g["m2_bias"][k])
        if ref is None:
            ref = refiner(g, apr=apr, graph=graph, per_pixel=True)
        else:
            ref.apr_base = apr
        pose, losses, info = ref.refine_apr(photo, tgt, T(g["hist"]), n)
        assert (ref.apr_graph is not None) == graph
        pose, losses = pose.cpu().numpy(), losses.cpu().numpy()
        assert info["retreat"] is False and not bool(g["m2_retreat"][k])
        assert abs(info["psnr"][0] - g["m2_psnr"][k, 0]) < 2e-3 and abs(info["psnr"][1] - g["m2_psnr"][k, -1]) < 5e-2, (info, g["m2_psnr"][k, [0, -1]])
        el = rel(losses, g["m2_loss"][k])
        P.record(f"{tag}[start {k}]", "loss curve (50 iterations) vs the reference's: max-norm; worst single iteration relative to its own value",
                 direct=el, e_hip=float(np.abs(losses / g["m2_loss"][k] - 1).max()), e_ref=None, bound=max(1e-3, 3 * D_l))
        assert el <= max(1e-3, 3 * D_l), (k, el)
        f64 = g["m2_final_f64"][k]
        P.check(f"{tag}[start {k}]", "refined pose (abs, 3x4)", float(np.abs(pose - f64).max()), float(np.abs(g["m2_final"][k] - f64).max()),
                float(np.abs(pose - g["m2_final"][k]).max()), tol=1e-3, factor=1.5)
        e_hip, e_ref = errors(g, [pose])[0], g["m2_err"][k]
        for j, name in enumerate(("translation error [m]", "rotation error [deg]")):
            P.record(f"{tag}[start {k}]", name, hip=e_hip[j], reference=e_ref[j], initial=g["init_err"][k, j], direct=abs(e_hip[j] - e_ref[j]) / e_ref[j],
                     bound=0.01)
            assert abs(e_hip[j] - e_ref[j]) <= 0.01 * e_ref[j], (k, name, e_hip, e_ref)


def test_two_per_pixel_refiners_on_two_streams_equal_their_solo_runs(golden):
    """refine_apr_concurrently with two PoseRefiner(pose_model=..., per_pixel=True) on two streams (the fixture's 30 x 40 rays, 8
    iterations, the two starts' regression networks): pose, loss curve and the verification record identical to refine_apr alone."""
    from nefes_amd.refine import refine_apr_concurrently
    g = golden("refine50_pp")
    shared = nets(g)
    photo, tgt, hist = photo_of(g), target_full(g), T(g["hist"])
    n = 8
    refs = [refiner(g, graph=True, apr=TinyAPR(g["m2_weight"][k], g["m2_bias"][k]), networks=shared, bn_running_stats=False, per_pixel=True)
            for k in (0, 1)]
    jobs = [(photo, tgt, hist)] * 2
    solo = [r.refine_apr(*job, iters=n) for r, job in zip(refs, jobs)]
    solo = [(p.clone(), l.clone(), dict(i)) for p, l, i in solo]
    outs = refine_apr_concurrently(refs, jobs, iters=n)
    for (p, l, info), (ps, ls, infos) in zip(outs, solo):
        assert torch.equal(p, ps) and torch.equal(l, ls) and info == infos
    assert not torch.equal(solo[0][0], solo[1][0]) and rel(solo[0][1].cpu().numpy(), g["m2_loss"][0, :n]) < 2e-3
