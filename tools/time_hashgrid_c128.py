#!/usr/bin/env python3
"""Fine forward and backward-to-inputs of a width-256 network on a supplied 32-feature encoding (a hash grid's), C = 16 (head class 0)
against C = 128 (head class 1), alternating in one process: HIP events around ops.field_fwd_x6(FULL, xyz_enc=...) and ops.field_bwd,
the wrappers' output / mask allocations included; median (min .. max) over the timed repetitions.
    python tools/time_hashgrid_c128.py [--rays 4096] [--samples 192] [--reps 10] [--warmup 2] [--json out.json]
The figures of profiles/hashgrid_c128/README.md were taken with the defaults."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nefes_amd import lib as L, ops  # noqa: E402
from nefes_amd.field import NeRFH_NFF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev, N, S = "cuda", a.rays, a.samples
    g = torch.Generator().manual_seed(0)
    enc = ((torch.rand(N, S, 32, generator=g) * 2 - 1) * 0.4).to(dev)
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(dev)
    cs = (16, 128)
    nets = {C: NeRFH_NFF('fine', W=256, f_dim=C, in_channels_xyz=32, encode_appearance=True, encode_transient=True).requires_grad_(False).to(dev)
            for C in cs}
    G = {C: torch.randn(N, 9 + C, S, generator=g).to(dev) for C in cs}
    times = {(C, w): [] for C in cs for w in ("fwd", "bwd")}
    for rep in range(a.warmup + a.reps):
        for C in cs:
            pk = nets[C].packed()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            raw, masks = ops.field_fwd_x6(pk, L.FIELD_FULL, N, S, xyz_enc=enc.reshape(-1, 32), viewdirs=v, want_masks=True)
            e1.record()
            ops.field_bwd(pk, N, S, raw, G[C], masks, viewdirs=v)
            e2.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[C, "fwd"].append(e0.elapsed_time(e1))
                times[C, "bwd"].append(e1.elapsed_time(e2))
    out = {}
    for (C, w), t in times.items():
        out[f"C{C}_{w}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        print(f"C = {C:3d} {w}: {statistics.median(t):.3f} ms ({min(t):.3f} .. {max(t):.3f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rays": N, "samples": S, **out}, f, indent=1)


if __name__ == "__main__":
    main()
