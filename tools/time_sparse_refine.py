"""ms per iteration and final pose error of the refinement loop on the 60 x 80 refinement scene (tests/golden/refine50_60x80.npz, the scene
of bench.py's refinement workloads): the dense loop (mode 3: 4800 rays, colour transform, FusionNet, feature loss at 1/4 resolution) and
the sparse loop PoseRefiner(sparse=K) at K = 256, 1024 and 4800 drawn pixels.

Target: SYNTHETIC -- the library's own features at the fixture's true pose (dense: the fused features; sparse: the field's feat_map as a
[C, 60, 80] frame), so the loss's minimum is that pose.  Starts: 8 poses perturbed from it by the fixture's own start error (0.138 in
translation, 4.75 degrees, directions drawn from seed 0).  Per run 50 captured iterations (HIP graph replays) per start; a run's time is
the host clock around the 8 x 50 iterations, ending in a device synchronise, after one untimed image (capture, plans, allocator).
`--repeats` runs per configuration, every run printed: their spread is the run-to-run spread on this box.

Where the tree has PoseRefiner(sparse=K, redraw=R) the sparse loops also run with a new device-side draw every R iterations
(`--redraw`, K below the whole frame), every loop's per-image set-up (the job and the state, host clock ending in a synchronise) is timed
with and without a 75 % mask, and `--draw` times ops.draw_pixels alone by device events (`--draw-calls` calls after a warm-up) at
`DRAW_SHAPES`, next to the time the bytes it cannot avoid -- the mask and the list -- would take at `--hbm-tbs` TB/s.

`--root DIR` times another checkout of this project (e.g. the parent commit) with this same script; a tree without PoseRefiner(sparse=)
runs the dense loop only.  Prints one JSON line per configuration."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time
import types

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--pixels", type=int, nargs="*", default=[256, 1024, 4800])
ap.add_argument("--redraw", type=int, nargs="*", default=[1, 5])
ap.add_argument("--setups", type=int, default=40, help="per-image set-ups timed per configuration")
ap.add_argument("--draw", action="store_true", help="time ops.draw_pixels alone as well")
ap.add_argument("--draw-calls", type=int, default=200)
ap.add_argument("--hbm-tbs", type=float, default=6.29, help="HBM rate the bound is stated at (a measured float4 copy on MI355X)")
ap.add_argument("--tag", default="this")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, ROOT)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402

import bench                                           # noqa: E402  (the scene's construction and the reference's pose-error metric)
from nefes_amd.field import NeRFH_NFF                  # noqa: E402
from nefes_amd.refine import PoseRefiner               # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
dev = "cuda"
g = dict(np.load(os.path.join(ROOT, "tests", "golden", "refine50_60x80.npz")))
T = lambda v: torch.from_numpy(np.asarray(v))
Wd, C = int(g["Wd"]), int(g["C"])
H, W, focal = int(g["hwf"][0]), int(g["hwf"][1]), float(g["hwf"][2])
ts = int(g["tinyscale"])
h, w = H // ts, W // ts
coarse = NeRFH_NFF('coarse', W=Wd, f_dim=C)
fine = NeRFH_NFF('fine', W=Wd, f_dim=C, encode_appearance=True, encode_transient=True)
with torch.no_grad():
    coarse.exposure_embedding.params.copy_(T(g["exposure_params"]))
for net in (coarse, fine):
    bench._structure_scene(dict(net.named_parameters()), *(float(v) for v in g["scene"]))
coarse, fine = coarse.requires_grad_(False).to(dev), fine.requires_grad_(False).to(dev)
args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, netchunk=1 << 21, encode_hist=True)
kw = dict(network_query_fn=None, perturb=False, N_importance=int(g["Ni"]), N_samples=int(g["Nc"]), network_fn=coarse, network_fine=fine,
          use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False, lindisp=False)
world = dict(pose_scale=float(g["pose_scale"]), pose_scale2=float(g["pose_scale2"]), move_all_cam_vec=g["move_all_cam_vec"].tolist())
common = dict(tinyscale=ts, lr_r=float(g["lr"][0]), lr_t=float(g["lr"][1]), world_setup=world, device=dev, graph=True)
hist = T(g["hist"]).to(dev)
true = T(g["true_c2w"]).float()


def perturbed(n, dt, deg, seed=0):
    """n poses at distance dt and angle deg from the true one, directions drawn from `seed`."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        axis = torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0)
        th = np.radians(deg)
        Kx = torch.tensor([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]], dtype=torch.float64)
        R = torch.eye(3, dtype=torch.float64) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
        p = true.double().clone()
        p[:3, :3] = R @ p[:3, :3]
        p[:3, 3] += dt * torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0)
        out.append(p.float().to(dev))
    return out


starts = perturbed(8, float(g["init_err"][0][0]), float(g["init_err"][0][1]))


mask75 = (torch.rand(h, w, generator=torch.Generator().manual_seed(0)) < 0.75).to(torch.uint8)


def setup_us(r, target, mask):
    """Median microseconds of one image's set-up on refiner r -- the job (a sparse refiner without redraw= draws its pixels here, on the
    host) and the state written in place -- host clock, ending in a device synchronise."""
    m, more, us = r._mode(), ({} if mask is None else {"mask": mask}), []
    for k in range(a.setups + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.set_state(*m.on_device(r._job(starts[k % len(starts)], target, hist, **more)))
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(us[3:]), 1)


def measure(name, make, target, extra, masked_setup=True):
    """`a.repeats` runs of 8 starts x a.iters iterations on one refiner: ms per iteration of each run, pose errors of the last; then the
    per-image set-up alone, without a mask and (a refiner built with masked=True) with a 75 % one."""
    r = make()
    r.refine(starts[0], target, hist, a.iters)                               # capture, plans, allocator: not timed
    ms, errs = [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses = [r.refine(s, target, hist, a.iters)[0] for s in starts]
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / (len(starts) * a.iters))
        errs = [bench._pose_error(true.numpy(), p[:3, :4].cpu().numpy()) for p in poses]
    if a.setups > 0:
        extra = dict(extra, setup_us=setup_us(r, target, None),
                     setup_us_masked=setup_us(make(masked=True), target, mask75) if masked_setup else None)
    rec = dict(tag=a.tag, loop=name, iters=a.iters, starts=len(starts), ms_per_iteration=[round(v, 4) for v in ms],
               median_ms=round(statistics.median(ms), 4), spread_ms=round(max(ms) - min(ms), 4),
               start_error=[round(float(v), 4) for v in g["init_err"][0]],
               final_dt_median=round(statistics.median(e[0] for e in errs), 4), final_deg_median=round(statistics.median(e[1] for e in errs), 3),
               final_dt_max=round(max(e[0] for e in errs), 4), final_deg_max=round(max(e[1] for e in errs), 3), **extra)
    print(json.dumps(rec), flush=True)


base = lambda **more: PoseRefiner(kw, args, (H, W, focal), float(g["near"]), float(g["far"]), **common, **more)
probe = base()
probe._reset(true.to(dev), torch.zeros(C, h, w, device=dev), hist)
measure("dense 60x80", base, probe.features()[0], dict(rays=h * w))
del probe

params = inspect.signature(PoseRefiner.__init__).parameters
if "sparse" in params:
    n = h * w
    grid = torch.stack([torch.arange(n) % w, torch.arange(n) // w], -1).float().to(dev)
    probe = base(sparse=n)
    probe._reset(true.to(dev), torch.zeros(C, h, w, device=dev), hist, None, grid)
    frame = probe.features().reshape(C, h, w)                                # the field's feat_map at the true pose, as a frame
    del probe
    for K in a.pixels:
        measure(f"sparse K={K}", lambda **more: base(sparse=K, seed=0, **more), frame, dict(rays=K),
                masked_setup=K <= int(mask75.sum()))                             # (more pixels than the mask has valid ones: refused)
        for every in (a.redraw if "redraw" in params and K < n else []):
            measure(f"sparse K={K} redraw={every}", lambda **more: base(sparse=K, seed=0, redraw=every, **more), frame,
                    dict(rays=K, redraw=every))

# ---- the draw alone: device events around a.draw_calls calls, after a warm-up ---------------------------------------------------
DRAW_SHAPES = ((1, 60, 80, 256), (1, 240, 427, 1024), (1, 480, 854, 4096), (8, 120, 213, 1536))
if a.draw:
    from nefes_amd import ops
    for B, dh, dw, K in DRAW_SHAPES:
        for masked in (False, True):
            m = (torch.rand(B, dh, dw, generator=torch.Generator().manual_seed(1)) < 0.75).to(torch.uint8).to(dev) if masked else None
            state, out = ops.draw_state(0, dev), torch.empty(B, K, 2, device=dev)
            call = lambda: ops.draw_pixels(dh, dw, K, state, B=B, mask=m, out=out)
            for _ in range(20):
                call()
            us = []
            for _ in range(3):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.draw_calls):
                    call()
                t1.record()
                torch.cuda.synchronize()
                us.append(round(t0.elapsed_time(t1) * 1e3 / a.draw_calls, 2))
            nbytes = (B * dh * dw if masked else 0) + B * K * 8              # the mask read once, the list written once
            print(json.dumps(dict(tag=a.tag, draw=[B, dh, dw, K], masked=masked, calls=a.draw_calls, us_per_call=us,
                                  mask_and_list_bytes=nbytes, us_of_those_bytes_at_hbm_rate=round(nbytes / (a.hbm_tbs * 1e12) * 1e6, 4),
                                  hbm_tbs=a.hbm_tbs)), flush=True)
