#!/usr/bin/env python3
"""ms per iteration of the refinement loop at the reference's shape (bench.py --workload loop50's geometry: bench.refinement_loop, the
scene of tests/golden/refine50_60x80.npz, 60 x 80 rays, 240 x 320 image, 3 images x 50 iterations per figure after warm-up and capture)
with PoseRefiner(masked=True) and no mask given -- all pixels valid -- or without it: what leaving the prepared-target (Gram) form of
the up-sampled channel-wise loss costs, and what the mask reads cost where there never was one (mode 3's low-resolution loss, per_pixel).

    python tools/time_masked_loop.py [--masked] [--per-pixel] [--modes upsampled 2 3] [--repeats 2]

bench.py is not changed: the constructor bench.refinement_loop imports is wrapped with the extra keywords for the duration of the call.
Without --masked and --per-pixel nothing is wrapped, so the same file times an earlier commit (copy it there).  One JSON line per figure."""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--per-pixel", action="store_true")
    ap.add_argument("--modes", nargs="+", default=["upsampled", "2", "3"], choices=["upsampled", "2", "3"])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import bench
    from nefes_amd import refine
    if not torch.cuda.is_available():
        raise SystemExit("time_masked_loop.py needs the GPU")
    extra = dict(masked=True) if a.masked else {}
    if a.per_pixel:
        extra["per_pixel"] = True
    plain = refine.PoseRefiner
    for mode in a.modes:
        for rep in range(a.repeats):
            if extra:
                refine.PoseRefiner = functools.partial(plain, **extra)
            try:
                sec, _, err = bench.refinement_loop(torch.device("cuda"), iters=a.iters, mode=mode)
            finally:
                refine.PoseRefiner = plain
            print(json.dumps({"label": a.label, "mode": mode, "masked": a.masked, "per_pixel": a.per_pixel, "repeat": rep,
                              "ms_per_iteration": round(sec / a.iters * 1e3, 4), "ms_per_image": round(sec * 1e3, 2), "pose_error": err["hip"]}),
                  flush=True)


if __name__ == "__main__":
    main()
