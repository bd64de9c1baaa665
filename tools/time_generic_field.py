#!/usr/bin/env python3
"""Times of the generic field kernels (csrc/field_generic.hip): forward (FULL, masks written) and backward-to-inputs at the reference
frame (80x60 rays, 64 + 64 samples) and the BASELINE frame (640x480, 64 + 128) for a few network shapes, as a fraction of the
fp32-MFMA bound bench.py uses for its strict-fp32 anchor (157.3 TFLOP/s), and at (256, 8) next to the tuned instance.

Usage:  python tools/time_generic_field.py [--frames ref,baseline] [--reps 5]
        rocprofv3 --kernel-trace --stats -- python tools/time_generic_field.py --reps 1     (per-kernel times)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import lib as L, ops                      # noqa: E402
from nefes_amd.field import NeRFH_NFF                    # noqa: E402

FP32_MFMA_TFLOPS = 157.3
FRAMES = {"ref": (80 * 60, 128), "baseline": (640 * 480, 192)}


def flops_per_sample(W, D, C):
    H = W // 2
    macs = 63 * W + (D - 1) * W * W + (63 * W if D > 4 else 0) + W + W * W + 2 * (W + 27) * H + (3 + C) * H + 2 * H * H + 5 * H
    return 2 * macs


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="ref,baseline")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(1)
    for frame in a.frames.split(","):
        N, S = FRAMES[frame]
        o = (torch.rand(N, 3, generator=gen) - .5).to(dev)
        d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
        z = torch.sort(torch.rand(N, S, generator=gen) * 4, -1)[0].to(dev)
        for (W, D) in [(64, 6), (256, 8), (512, 8)]:
            net = NeRFH_NFF('fine', D=D, W=W, f_dim=16, encode_transient=True).requires_grad_(False).to(dev)
            packs = [("generic", net.packed_generic())] + ([("tuned", net.packed())] if net._supported() else [])
            for kind, pk in packs:
                oo = o.clone().requires_grad_()
                raw = ops.field_from_rays(oo, d, d, z, pk, L.FIELD_FULL)
                g = torch.randn_like(raw)
                fwd = time_ms(lambda: ops.field_from_rays(oo, d, d, z, pk, L.FIELD_FULL), a.reps)
                both = time_ms(lambda: torch.autograd.grad(ops.field_from_rays(oo, d, d, z, pk, L.FIELD_FULL), oo, g), a.reps)
                fl = flops_per_sample(W, D, 16) * N * S
                print(json.dumps({"frame": frame, "W": W, "D": D, "kernels": kind, "fwd_ms": round(fwd, 3), "bwd_ms": round(both - fwd, 3),
                                  "fwd_fraction_of_fp32_mfma_bound": round(fl / (fwd * 1e-3) / (FP32_MFMA_TFLOPS * 1e12), 4)}))


if __name__ == "__main__":
    main()
