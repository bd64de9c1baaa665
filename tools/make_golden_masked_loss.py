#!/usr/bin/env python3
"""Generate tests/golden/masked_loss.npz by running the REFERENCE's own masked_feature_loss (dm/DFM_pose_refine.py:257-288; the loss
behind `--semantic`) on the CPU, imported the way tools/make_golden_refine.py imports that module.

Per case (C, H, W) in ((5, 6, 7), (16, 15, 20)): two feature maps and three masks -- random at about 60 % valid, a single valid pixel,
all ones -- and, for both forms (per channel / per pixel), the reference's loss from the float32 maps (`ref32`) and from the same maps
in float64 (`ref64`), both indexed [case, mask, per_pixel].  The maps are stored as int8 q with value q / 4 (exact in float32), so the file stays a few KB; it holds data
only.  tests/test_masked_loss_ref.py compares nefes_amd.refine.masked_feature_loss (the select form the loop can replay) with it.

Usage:  python tools/make_golden_masked_loss.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_refine import import_reference  # noqa: E402

CASES = ((5, 6, 7), (16, 15, 20))
MASKS = ("random", "single", "ones")
SCALE = 4.0


def make_mask(kind, H, W, g):
    if kind == "random":
        return (torch.rand(1, H, W, generator=g) < 0.6).to(torch.uint8)
    if kind == "ones":
        return torch.ones(1, H, W, dtype=torch.uint8)
    m = torch.zeros(1, H, W, dtype=torch.uint8)
    m[0, H // 2, W // 3] = 1
    return m


def main():
    DR, _ = import_reference()
    out = {"scale": np.float32(SCALE), "cases": np.array(CASES, dtype=np.int32), "masks": np.array(MASKS)}
    ref32, ref64 = np.zeros((len(CASES), len(MASKS), 2), np.float32), np.zeros((len(CASES), len(MASKS), 2), np.float64)
    for ci, (C, H, W) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 * C + H + 1)
        qa = torch.randint(-8, 9, (C, H, W), generator=g)
        qb = (qa + torch.randint(-5, 6, (C, H, W), generator=g)).clamp(-127, 127)
        key = f"{C}x{H}x{W}"
        out[f"a_{key}"], out[f"b_{key}"] = qa.numpy().astype(np.int8), qb.numpy().astype(np.int8)
        a, b = qa.float() / SCALE, qb.float() / SCALE
        for mi, kind in enumerate(MASKS):
            m = make_mask(kind, H, W, g)
            out[f"mask_{kind}_{key}"] = m.numpy()
            for pp in (False, True):
                l32 = DR.masked_feature_loss(a, b, m, img_in=True, per_pixel=pp)
                l64 = DR.masked_feature_loss(a.double(), b.double(), m, img_in=True, per_pixel=pp)
                tag = f"{'pixel' if pp else 'channel'}_{kind}_{key}"
                ref32[ci, mi, int(pp)], ref64[ci, mi, int(pp)] = float(l32), float(l64)
                print(f"{tag:32s} valid {int(m.sum()):4d}  ref32 {float(l32):.8f}  ref64 {float(l64):.15f}")
    path = os.path.join(ROOT, "tests", "golden", "masked_loss.npz")
    np.savez_compressed(path, ref32=ref32, ref64=ref64, **out)      # ref*[case, mask, per_pixel]
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
