#!/usr/bin/env python3
"""Generate tests/golden/fusion_train.npz by running the REFERENCE's own FusionNet (script/models/nerfh_nff.py:356-418) in TRAIN mode
with every parameter trainable, on the CPU (the reference never travels -- these vectors do): what the fusion part of the reference's
third training stage computes (script/run_nefes.py:78-108,150-160: run_fusion_net on patches, an L1 loss on the fused features).

    FusionNet(16) under manual_seed(0);  x = cat(rgb, feat) for 3 images of 6 x 8;  loss = L1(fused, target);  backward

Stored (numeric arrays only): the inputs (rgb [144,3], feat [144,16] in run_fusion_net's pixel-major form, target), the ten parameters,
`fused`, the loss, d rgb / d feat, the gradient of every parameter, and the BatchNorm buffers after the call.
tests/test_fusion_train_golden.py pins oracle/refine_cpu.fusion_net on it; the GPU tests take that oracle as their truth.

Usage:  python tools/make_golden_fusion_train.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, import_reference, npy  # noqa: E402

B, H, W, C = 3, 6, 8, 16


def main():
    _, M, _ = import_reference()
    torch.set_num_threads(1)
    torch.manual_seed(0)
    net = M.FusionNet(C).train()
    g = torch.Generator().manual_seed(77)
    rgb = torch.rand(B * H * W, 3, generator=g).requires_grad_()
    feat = torch.randn(B * H * W, C, generator=g).requires_grad_()
    target = torch.randn(B, C, H, W, generator=g)
    # run_fusion_net's reshaping (nerfh_nff.py:578-603); forward() normalises the colour channels of this tensor in place
    x = torch.cat([rgb.reshape(B, H, W, 3).permute(0, 3, 1, 2), feat.reshape(B, H, W, C).permute(0, 3, 1, 2)], 1)
    out = {"rgb": npy(rgb), "feat": npy(feat), "target": npy(target)}
    out.update({"param." + k: npy(v).copy() for k, v in net.named_parameters()})
    fused = net(x)
    loss = torch.nn.functional.l1_loss(fused, target)
    loss.backward()
    out.update({"fused": npy(fused), "loss": npy(loss), "d_rgb": npy(rgb.grad), "d_feat": npy(feat.grad)})
    out.update({"grad." + k: npy(v.grad) for k, v in net.named_parameters()})
    out.update({"buffer." + k: npy(v) for k, v in net.named_buffers()})
    assert len([k for k in out if k.startswith("grad.")]) == 10
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "fusion_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
