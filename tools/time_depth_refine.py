"""ms per iteration, launches per iteration and final pose error of the refinement loop with and without the depth term
(PoseRefiner(depth_weight=)), on the 60 x 80 refinement scene (tests/golden/refine50_60x80.npz), by tools/time_sparse_refine.py's protocol:
the dense loop (mode 3: 4800 rays) and the sparse loop at K = 256 drawn pixels.

Targets: SYNTHETIC -- the library's own features at the fixture's true pose (dense: the fused features; sparse: the field's feat_map as
a frame) and, for the depth term, its own 1 / disp_map there as a [60, 80] frame with a block of holes (zeros) punched into it: both
terms' minimum is the true pose.  Starts: 8 poses perturbed from it by the fixture's own start error (directions from seed 0).  Per run
50 captured iterations (HIP graph replays) per start; a run's time is the host clock around the 8 x 50 iterations, ending in a device
synchronise, after one untimed image (capture, plans, allocator).  `--repeats` runs per configuration, every run printed: their spread is
the run-to-run spread on this box.  The launches of one EAGER iteration are counted with torch.profiler.

`--root DIR` times another checkout of this project (e.g. the parent commit) with this same script; a tree without
PoseRefiner(depth_weight=) runs the loops without the term only.  Prints one JSON line per configuration, poses with every digit."""
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
ap.add_argument("--pixels", type=int, default=256)
ap.add_argument("--depth-weight", type=float, default=1.0)
ap.add_argument("--depth-huber", type=float, default=0.1)
ap.add_argument("--tag", default="this")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, ROOT)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
from torch.profiler import ProfilerActivity, profile   # noqa: E402

import bench                                           # noqa: E402  (the scene's construction and the reference's pose-error metric)
from nefes_amd.field import NeRFH_NFF                  # noqa: E402
from nefes_amd.refine import PoseRefiner               # noqa: E402
from nefes_amd.render import render                    # noqa: E402

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
    """n poses at distance dt and angle deg from the true one, directions drawn from `seed` (tools/time_sparse_refine.py's starts)."""
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


def launches(r):
    """GPU launches of one eager iteration at the refiner's current state."""
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        r._iteration()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def measure(name, make, target, more, extra):
    r = make()
    r.refine(starts[0], target, hist, a.iters, **more)                       # capture, plans, allocator: not timed
    ms, errs, poses = [], [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses = [r.refine(s, target, hist, a.iters, **more)[0] for s in starts]
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / (len(starts) * a.iters))
        errs = [bench._pose_error(true.numpy(), p[:3, :4].cpu().numpy()) for p in poses]
    depth_term = getattr(r, "depth_loss", None)
    eager = make(graph=False)
    m = eager._mode()
    m.set_state(*m.on_device(eager._job(starts[0], target, hist, **more)))
    eager._iteration()
    rec = dict(tag=a.tag, loop=name, iters=a.iters, starts=len(starts), ms_per_iteration=[round(v, 4) for v in ms],
               median_ms=round(statistics.median(ms), 4), spread_ms=round(max(ms) - min(ms), 4), launches_per_eager_iteration=launches(eager),
               start_error=[round(float(v), 4) for v in g["init_err"][0]],
               final_dt_median=round(statistics.median(e[0] for e in errs), 4), final_deg_median=round(statistics.median(e[1] for e in errs), 3),
               final_dt_max=round(max(e[0] for e in errs), 4), final_deg_max=round(max(e[1] for e in errs), 3),
               final_depth_term=None if depth_term is None else float(depth_term),
               last_pose_of_start_0=[repr(float(v)) for v in poses[0][:3, :4].reshape(-1).cpu()], **extra)
    print(json.dumps(rec), flush=True)


def base(**more):
    return PoseRefiner(kw, args, (H, W, focal), float(g["near"]), float(g["far"]), **dict(common, **more))


probe = base(graph=False)
probe._reset(true.to(dev), torch.zeros(C, h, w, device=dev), hist)
fused = probe.features()[0]                                                  # dense target: the fused features at the true pose
with torch.no_grad():
    _, disp, _, ex = render(probe.h, probe.w, probe.focal, c2w=probe._composed_pose().reshape(3, 4), near=probe.near, far=probe.far,
                            img_idx=probe.hist, **kw)
frame = ex["feat_map"].t().reshape(C, h, w).contiguous()                     # sparse target: the field's feat_map there, as a frame
depth = (1.0 / disp).reshape(h, w).clone()
depth[20:40, 30:55] = 0.0                                                    # a block of sensor holes
holes = int((~(torch.isfinite(depth) & (depth > 0))).sum())
del probe

has_depth = "depth_weight" in inspect.signature(PoseRefiner.__init__).parameters
term = dict(depth_weight=a.depth_weight, depth_huber=a.depth_huber)
K = a.pixels
measure("dense 60x80", base, fused, {}, dict(rays=h * w, depth_term=False))
measure(f"sparse K={K}", lambda **m: base(sparse=K, seed=0, **m), frame, {}, dict(rays=K, depth_term=False))
if has_depth:
    measure("dense 60x80 + depth", lambda **m: base(**term, **m), fused, dict(depth=depth), dict(rays=h * w, depth_term=True, holes=holes, **term))
    measure(f"sparse K={K} + depth", lambda **m: base(sparse=K, seed=0, **term, **m), frame, dict(depth=depth),
            dict(rays=K, depth_term=True, holes=holes, **term))
