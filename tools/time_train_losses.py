#!/usr/bin/env python3
"""The training step's losses: the library's kernels (nefes_amd/losses.py: two launches forward, one backward) against the torch
expressions of tests/loss_ref.py in float32 on the GPU, which is what a step runs without them (the reference's models/losses.py).

  pair    loss forward + backward alone, on leaves:
            ray stage    N = 6144 (1536 x 4 random rays), C = 128, S = 128, NeRF-W + L1, loss + 0.04 loss_f       (run_nefes.py:244-248)
            patch stage  N = 7168 (4 x 7 patches of 16 x 16), the same with the fusion term, + 0.02 loss_f + 0.02 loss_fusion (:238-243)
          transient_sigmas is a contiguous [N, S] leaf here (through render()'s strided view both sides pay autograd's zero fill of the
          whole raw tensor, which is not the losses' time)
  step    train-mode render() of the ray-stage batch (two networks of 8 x 128, 64 + 64 samples, NeRF-W on) + loss + backward to every
          weight, with either loss implementation

Windows alternate torch / kernels / torch / kernels in one process, each after a warm-up and a device synchronise, timed by device events
around the whole window (so launch gaps count, as they do for a user).  Launches and the sum of kernel times of ONE pair come from a
torch.profiler run of its own, after the timed windows.

    python tools/time_train_losses.py [out.md]          prints a markdown report (and writes it to out.md)
"""
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nefes_amd import losses  # noqa: E402
from tests import loss_ref as R  # noqa: E402

DEV = "cuda"
C, S = 128, 128
KW = dict(coef=1, L1_loss=True, lambda_u=0.01)
STAGES = {"ray stage (N = 6144)": (6144, False, (1.0, 0.04)), "patch stage (N = 7168, fusion term)": (7168, True, (1.0, 0.02, 0.02))}
WARM, ITERS, ROUNDS = 20, 500, 2
STEP_WARM, STEP_ITERS = 5, 30


def leaves(N, fusion):
    g = torch.Generator().manual_seed(N)
    t = {"rgb_fine": torch.rand(N, 3, generator=g), "rgb_coarse": torch.rand(N, 3, generator=g), "beta": 0.3 + torch.rand(N, generator=g),
         "transient_sigmas": 2.0 * torch.rand(N, S, generator=g), "feat_fine": torch.randn(N, C, generator=g)}
    if fusion:
        t["feat_fusion"] = torch.randn(N, C, generator=g)
    inputs = {k: v.to(DEV).requires_grad_() for k, v in t.items()}
    return inputs, torch.rand(N, 3, generator=g).to(DEV), torch.randn(N, C, generator=g).to(DEV)


def loss_of(kernels, fn, inputs, rgb_t, feat_t, fusion, weights):
    if kernels:
        ret = fn(inputs, {"rgb": rgb_t, "feat": feat_t}, switch_on=fusion, color_only_switch=False)
    else:
        ret = R.evaluate("color_feat_fusion_nerfw", inputs, rgb_t, feat_t, switch_on=fusion, **KW)
    return R.total(ret, weights)


def make_step(fn, inputs, rgb_t, feat_t, fusion, weights):
    def step(kernels):
        for v in inputs.values():
            v.grad = None
        loss_of(kernels, fn, inputs, rgb_t, feat_t, fusion, weights).backward()
    return step


def window(fn_step, warm, iters):
    for _ in range(warm):
        fn_step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn_step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def ab(step, warm, iters):
    times = {False: [], True: []}
    for _ in range(ROUNDS):
        for kernels in (False, True):
            times[kernels].append(window(lambda: step(kernels), warm, iters))
    return times


def profile_once(fn_step):
    """(kernel launches, sum of kernel times in us) of one call, or None where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn_step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn_step()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not ev:
            return None
        dur = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0) or 0.0
        return len(ev), sum(dur(e) for e in ev)
    except Exception as exc:      # a report without this column is still a report
        return f"profiler failed: {type(exc).__name__}"


def main():
    fn = losses.ColorFeatureFusionNerfWLoss(**KW)
    out = [f"Device: {torch.cuda.get_device_name(0)}; {time.strftime('%Y-%m-%d %H:%M:%S')} (the box's clock); torch {torch.__version__}.", "",
           f"## Loss forward + backward alone (C = {C}, S = {S}, NeRF-W + L1; {ITERS} iterations per window after {WARM} warm-up, "
           "windows alternated torch / kernels / torch / kernels)", "",
           "| shape | torch expressions, ms per pair (each window) | library kernels, ms per pair (each window) |", "|---|---|---|"]
    steps = {}
    for tag, (N, fusion, weights) in STAGES.items():
        inputs, rgb_t, feat_t = leaves(N, fusion)
        step = make_step(fn, inputs, rgb_t, feat_t, fusion, weights)
        # the two sides agree before anything is timed
        step(False)
        ga = {k: v.grad.clone() for k, v in inputs.items()}
        step(True)
        for k, v in inputs.items():
            assert float((v.grad - ga[k]).abs().max()) <= 1e-5 * float(ga[k].abs().max()), k
        t = ab(step, WARM, ITERS)
        out.append(f"| {tag} | " + " / ".join(f"{x:.4f}" for x in t[False]) + " | " + " / ".join(f"{x:.4f}" for x in t[True]) + " |")
        steps[tag] = step

    # ---- the whole step at the ray-stage batch -------------------------------------------------------------------------------
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.render import render
    from oracle import ref_cpu as O
    H, W, focal = 64, 96, 80.0
    torch.manual_seed(0)
    coarse = NeRFH_NFF('coarse', W=128, f_dim=C).to(DEV)
    fine = NeRFH_NFF('fine', W=128, f_dim=C, encode_appearance=True, encode_transient=True).to(DEV)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True)
    kwr = dict(network_query_fn=None, perturb=1., N_importance=64, N_samples=64, network_fn=coarse, network_fine=fine, use_viewdirs=True,
               white_bkgd=False, raw_noise_std=0., test_time=False, args=args, ndc=False, lindisp=False)
    ro, rd = O.ray_bundle(H, W, focal, O.bench_pose())
    ro, rd = ro.reshape(-1, 3).to(DEV), rd.reshape(-1, 3).to(DEV)
    g = torch.Generator().manual_seed(9)
    rgb_t, feat_t = torch.rand(H * W, 3, generator=g).to(DEV), torch.randn(H * W, C, generator=g).to(DEV)
    params = [p for net in (coarse, fine) for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]

    def train_step(kernels):
        for p in params:
            p.grad = None
        rgb, _, _, ex = render(H, W, focal, rays=(ro, rd), near=0., far=4., **kwr)
        results = {"rgb_fine": rgb, "rgb_coarse": ex["rgb0"], "feat_fine": ex["feat_map"], "beta": ex["beta"],
                   "transient_sigmas": ex["transient_sigmas"]}
        loss_of(kernels, fn, results, rgb_t, feat_t, False, (1.0, 0.04)).backward()

    t = ab(train_step, STEP_WARM, STEP_ITERS)
    out += ["", f"## Whole step: train-mode render() of {H * W} rays (8 x 128 networks, 64 + 64 samples, C = {C}, NeRF-W) + loss + backward "
            f"({STEP_ITERS} steps per window after {STEP_WARM} warm-up)", "",
            "| losses | ms per step (each window) |", "|---|---|",
            "| torch expressions | " + " / ".join(f"{x:.3f}" for x in t[False]) + " |",
            "| library kernels | " + " / ".join(f"{x:.3f}" for x in t[True]) + " |",
            "", "## Launches of one loss forward + backward (torch.profiler, a run of its own; the library's side includes the torch glue",
            "around its three kernels: the weighted sum of the losses and its backward)", "",
            "| shape | torch expressions: launches, sum of kernel times (us) | library kernels: launches, sum of kernel times (us) |", "|---|---|---|"]
    prof = {tag: {k: profile_once(lambda k=k, step=step: step(k)) for k in (False, True)} for tag, step in steps.items()}
    show = lambda p: "not measured" if p is None else (p if isinstance(p, str) else f"{p[0]}, {p[1]:.1f}")
    for tag, p in prof.items():
        out.append(f"| {tag} | {show(p[False])} | {show(p[True])} |")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
