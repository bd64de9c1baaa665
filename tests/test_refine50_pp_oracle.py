"""tests/golden/refine50_pp.npz: the refinement loop's shipped default mode (`train_on_batch`, pose_only 2) with the reference's own
`--per_pixel` flag set -- FeatureLoss(per_pixel=True): the cosine similarity over the CHANNELS of every pixel -- two perturbed starts
x 50 iterations executed by the reference's functions on the CPU
(`tools/make_golden_refine50.py --per-pixel --modes 2 --k 2 --out tests/golden/refine50_pp.npz`; mode 3 hard-codes per_pixel=False, its
arrays would repeat refine50.npz and are not stored).  The oracle's feature_loss is wrapped to per_pixel=True for these tests
(`per_pixel_oracle`: Problem.loss_at_pose looks the name up at call time).  CPU only; the GPU twin is tests/test_gpu_refine_pp.py, which
takes its yardstick -- the float32 oracle's own distance from the fixture -- from `oracle_distances` below."""
import contextlib
import functools
import os

import numpy as np
import torch

from oracle import refine_cpu as RC
from tests.test_refine50_oracle import photo_of, problem, rel

ITERATIONS = (0, 20, 49)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@contextlib.contextmanager
def per_pixel_oracle():
    """oracle.refine_cpu.feature_loss with per_pixel=True for the duration of the block."""
    plain = RC.feature_loss
    RC.feature_loss = lambda x, y, per_pixel=False: plain(x, y, per_pixel=True)
    try:
        yield
    finally:
        RC.feature_loss = plain


def weights_before(g, k, i):
    """The regression network's (weight, bias) as the reference held them before iteration i of start k."""
    return (g["m2_weight"][k], g["m2_bias"][k]) if i == 0 else (g["m2_w_traj"][k, i - 1], g["m2_b_traj"][k, i - 1])


@functools.lru_cache(maxsize=None)
def oracle_distances():
    """The float32 oracle against the fixture, teacher-forced at ITERATIONS of start 0: {i: (relative loss distance, gradient distance in
    units of |g| at iteration 0, gradient distance relative to its own norm)} and the two maxima (D_l, D_g) -- how far two fp32
    evaluations of this loop are apart, the yardstick of the GPU test."""
    g = dict(np.load(os.path.join(GOLDEN, "refine50_pp.npz")))
    k = 0
    p = problem(g, torch.float32, k, 2)
    desc = RC.image_descriptor(photo_of(g))
    g0 = float(np.abs(g["m2_grad"][k, 0]).max())
    per = {}
    with per_pixel_oracle():
        for i in ITERATIONS:
            Wn, bn = weights_before(g, k, i)
            raw = (torch.from_numpy(Wn) @ desc + torch.from_numpy(bn)).requires_grad_()
            loss = p.loss_at_pose(RC.svd_reg(raw.reshape(3, 4)))
            graw, = torch.autograd.grad(loss, raw)
            ref_l = float(g["m2_loss"][k, i])
            per[i] = (abs(float(loss.detach()) - ref_l) / ref_l, float(np.abs(graw.numpy() - g["m2_grad"][k, i]).max()) / g0,
                      rel(graw.numpy(), g["m2_grad"][k, i]))
    return per, max(v[0] for v in per.values()), max(v[1] for v in per.values())


def test_fixture_holds_the_per_pixel_mode2_runs(golden):
    """Arrays only, under 1 MB, two starts x 50 iterations of mode 2 and no mode-3 arrays; the loss differs from the per-channel
    fixture's at the same start (the flag was honoured)."""
    path = os.path.join(GOLDEN, "refine50_pp.npz")
    assert os.path.getsize(path) < 1_000_000
    g, base = golden("refine50_pp"), golden("refine50")
    assert not any(k.startswith("m3_") for k in g) and all(v.dtype != object for v in g.values())
    assert g["m2_loss"].shape == (2, 50) and g["m2_grad"].shape == (2, 50, 12) and g["m2_w_traj"].shape == (2, 50, 12, 12)
    assert g["m2_final_f64"].shape == (2, 3, 4)
    for key in ("init_c2w", "target_low", "photo_u8", "hist", "exposure_params", "true_c2w"):
        assert np.array_equal(g[key], base[key][:2] if key == "init_c2w" else base[key]), key      # the same scene and starts
    assert np.array_equal(g["m2_weight"], base["m2_weight"][:2]) and abs(g["m2_loss"][0, 0] / base["m2_loss"][0, 0] - 1) > 0.05


def test_reference_converges_and_keeps_the_refined_pose(golden):
    """From both starts the reference's per-pixel `train_on_batch` converges and the verification step does not roll back -- a
    property of the reference on this fixture that the GPU test asserts of the library's loop."""
    g = golden("refine50_pp")
    assert g["m2_retreat"].dtype == bool and not g["m2_retreat"].any()
    assert (g["m2_err"] < g["init_err"] / 3).all(), (g["m2_err"], g["init_err"])
    assert (g["m2_loss"][:, -1] < g["m2_loss"][:, 0] / 50).all() and (g["m2_psnr"][:, -1] > g["m2_psnr"][:, 0] + 15).all()
    for k in range(2):
        t, r = RC.pose_error(g["true_c2w"], g["m2_final"][k])
        assert abs(t - g["m2_err"][k, 0]) < 1e-6 and abs(r - g["m2_err"][k, 1]) < 1e-4
        e64 = RC.pose_error(g["true_c2w"], g["m2_final_f64"][k])             # the float64 oracle's run ends where the reference's ends
        assert abs(e64[0] - t) < 0.01 * t and abs(e64[1] - r) < 0.01 * r, (k, e64, t, r)


def test_oracle_mode2_per_pixel_iteration_matches_reference():
    """Teacher-forced at iterations 0, 20 and 49 of start 0: the fp32 oracle with its loss wrapped to per-pixel returns the reference's
    loss and its gradient to the network's twelve outputs, within the bounds tests/test_refine50_oracle.py holds the per-channel runs to.
    Measured on the CPU: loss 5.6e-07, 0, 0 (relative: D_l = 5.6e-07); gradient 5.5e-06, 5.4e-06, 2.1e-06 in units of |g| at iteration 0
    (D_g = 5.5e-06), i.e. 5.5e-06, 1.5e-05, 1.7e-05 of its own norm."""
    per, D_l, D_g = oracle_distances()
    for i, (dl, dg0, dg) in per.items():
        print(f"refine50_pp fp32 oracle vs reference, iteration {i}: loss {dl:.2e} (relative), gradient {dg0:.2e} of |g| at iteration 0, {dg:.2e} of its own norm")
        assert dl < 2e-4 and dg < 2e-4 and dg0 < 2e-4, (i, dl, dg0, dg)
    assert D_l == max(v[0] for v in per.values()) and D_g == max(v[1] for v in per.values())
