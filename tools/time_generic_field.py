#!/usr/bin/env python3
"""Times of the generic field kernels (csrc/field_generic.hip): forward (FULL, masks written) and backward-to-inputs at the reference
frame (80x60 rays, 64 + 64 samples) and the BASELINE frame (640x480, 64 + 128) for a few network shapes, as a fraction of the
fp32-MFMA bound bench.py uses for its strict-fp32 anchor (157.3 TFLOP/s), and at (256, 8) next to the tuned instance.

--ext: the instances on a SUPPLIED 32-feature encoding (hash-grid fields: gen_fwd_kernel / gen_bwd_kernel<NCB, GenArgsExt>) instead:
FieldFromEncoding forward + backward at 4096 rays x 192 samples, (256, 8, 16) generic against tuned alternating in the same run,
(128, 8, 128) and (64, 6, 16) generic alone; per shape a warm-up, --reps repetitions of each, median and spread (min..max), the
sustained clock of the device beside them (nefes_probe_mfma_clock).

Usage:  python tools/time_generic_field.py [--frames ref,baseline] [--reps 5]
        python tools/time_generic_field.py --ext [--reps 7]
        rocprofv3 --kernel-trace --stats -- python tools/time_generic_field.py --reps 1     (per-kernel times)
"""
import argparse
import ctypes as C
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


def flops_per_sample_ext(W, D, C):
    return flops_per_sample(W, D, C) - 2 * (63 - 32) * W * (2 if D > 4 else 1)


def once_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main_ext(reps, dev):
    """One JSON line per (shape, kernels): median and min..max of `reps` forwards and of `reps` forward + backward passes."""
    ghz, tf = C.c_double(), C.c_double()
    L.check(L.load().nefes_probe_mfma_clock(1, 40, C.byref(ghz), C.byref(tf), None), "nefes_probe_mfma_clock")
    N, S = 4096, 192
    gen = torch.Generator().manual_seed(1)
    enc = ((torch.rand(N, S, 32, generator=gen) * 2 - 1) * 0.4).to(dev).requires_grad_()
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
    med = lambda x: sorted(x)[len(x) // 2]
    for (W, D, Cf) in [(256, 8, 16), (128, 8, 128), (64, 6, 16)]:
        net = NeRFH_NFF('fine', D=D, W=W, f_dim=Cf, in_channels_xyz=32, encode_transient=True).requires_grad_(False).to(dev)
        packs = [("generic", net.packed_generic())] + ([("tuned", net.packed())] if net._supported() else [])
        g = torch.randn(N, 9 + Cf, S, device=dev)
        fwd = {k: (lambda pk=pk: ops.FieldFromEncoding.apply(enc, v, pk, L.FIELD_FULL)) for k, pk in packs}
        both = {k: (lambda f=f: torch.autograd.grad(f(), enc, g)) for k, f in fwd.items()}
        t = {(k, w): [] for k, _ in packs for w in ("fwd", "both")}
        for k, _ in packs:                                   # warm-up: every shape and direction the timed window uses
            both[k]()
        torch.cuda.synchronize()
        for _ in range(reps):                                # alternating: the kernels compared share whatever else the box is doing
            for k, _ in packs:
                t[k, "fwd"].append(once_ms(fwd[k]))
                t[k, "both"].append(once_ms(both[k]))
        for k, _ in packs:
            f, b = t[k, "fwd"], [x - med(t[k, "fwd"]) for x in t[k, "both"]]
            fl = flops_per_sample_ext(W, D, Cf) * N * S
            print(json.dumps({"ext": True, "rays": N, "samples": S, "W": W, "D": D, "C": Cf, "kernels": k, "reps": reps,
                              "fwd_ms_median": round(med(f), 3), "fwd_ms_min_max": [round(min(f), 3), round(max(f), 3)],
                              "bwd_ms_median": round(med(b), 3), "bwd_ms_min_max": [round(min(b), 3), round(max(b), 3)],
                              "fwd_fraction_of_fp32_mfma_bound": round(fl / (med(f) * 1e-3) / (FP32_MFMA_TFLOPS * 1e12), 4),
                              "sustained_clock_ghz": round(ghz.value, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="ref,baseline")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ext", action="store_true", help="the instances on a supplied 32-feature encoding (FieldFromEncoding)")
    a = ap.parse_args()
    dev = "cuda:0"
    if a.ext:
        return main_ext(a.reps, dev)
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
