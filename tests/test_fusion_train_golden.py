"""oracle/refine_cpu.fusion_net with TRAINABLE weights against the reference's own FusionNet in train mode (tests/golden/fusion_train.npz,
made by tools/make_golden_fusion_train.py from script/models/nerfh_nff.py:356-418): fused features, the gradient to the rendered maps
and the gradient of all ten parameters of  L1(fused, target).  The GPU tests of the training kernels (tests/test_gpu_fusion_train.py)
take this oracle as their truth; here it is tied to the reference."""
import os

import numpy as np
import pytest
import torch

from oracle import refine_cpu as RC
from tests.branch import rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_train.npz")
B, H, W, C = 3, 6, 8, 16
PARAMS = [f"net.{k}.{s}" for k in (0, 2, 4, 6, 7) for s in ("weight", "bias")]


def cancelling_scale(sd, rgb, feat, H, W, B, loss_fn, conv_pos=None):
    """The scale on which the gradient of net.6.bias -- the bias of the convolution in front of the BatchNorm -- is measured.  That
    gradient is zero in exact arithmetic (the normalisation removes a per-channel constant): what any evaluation returns is the rounding
    residue of a cancelling sum over the pixels, 1e-10 in fp32 and 1e-18 in float64, and its own size is no unit.  The unit is the sum
    it cancels in: max over channels of sum over pixels of |d loss / d h|, h the BatchNorm's input, from the float64 oracle."""
    dt = torch.float64
    conv = {k: v.detach().to(dt) for k, v in sd.items() if not k.startswith("net.7")}
    h = RC.fusion_net(conv, rgb.detach().to(dt), feat.detach().to(dt), H, W, B, conv_pos=conv_pos).requires_grad_()
    mu = h.mean(dim=(0, 2, 3), keepdim=True)
    y = (h - mu) / torch.sqrt(((h - mu) ** 2).mean(dim=(0, 2, 3), keepdim=True) + 1e-5)
    y = y * sd["net.7.weight"].detach().to(dt)[None, :, None, None] + sd["net.7.bias"].detach().to(dt)[None, :, None, None]
    g_h, = torch.autograd.grad(loss_fn(y), h)
    return float(g_h.abs().sum(dim=(0, 2, 3)).max())


def scale_of(name, g):
    if name != "grad.net.6.bias":
        return None                                                   # its own largest element
    return cancelling_scale({k: g["param." + k] for k in PARAMS}, g["rgb"], g["feat"], H, W, B,
                            lambda y: torch.nn.functional.l1_loss(y, g["target"].double()))


def load():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(GOLDEN).items()}


def oracle_run(g, dt, conv_pos=None, audit=None):
    """-> {name: tensor}: fused, d rgb, d feat and the ten parameter gradients of L1(fused, target), oracle in dtype dt."""
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_()      # (a copy: .to() of the same dtype would mark the fixture's own tensor)
    sd = {k: leaf(g["param." + k]) for k in PARAMS}
    rgb, feat = leaf(g["rgb"]), leaf(g["feat"])
    fused = RC.fusion_net(sd, rgb, feat, H, W, B, conv_pos=conv_pos, audit=audit)
    loss = torch.nn.functional.l1_loss(fused, g["target"].to(dt))
    grads = torch.autograd.grad(loss, [rgb, feat] + [sd[k] for k in PARAMS])
    out = {"fused": fused.detach(), "d_rgb": grads[0], "d_feat": grads[1]}
    out.update({"grad." + k: v for k, v in zip(PARAMS, grads[2:])})
    return out


def test_fixture_holds_what_the_tool_says():
    g = load()
    assert g["fused"].shape == (B, C, H, W) and g["rgb"].shape == (B * H * W, 3) and g["feat"].shape == (B * H * W, C)
    assert sorted(k[5:] for k in g if k.startswith("grad.")) == sorted(PARAMS)
    assert all(g["grad." + k].shape == g["param." + k].shape and float(g["grad." + k].abs().max()) > 0 for k in PARAMS)
    assert int(g["buffer.net.7.num_batches_tracked"]) == 1
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("dt,tol", [(torch.float64, 1e-5), (torch.float32, 1e-4)], ids=["float64", "float32"])
def test_oracle_matches_the_reference_in_train_mode(dt, tol):
    g = load()
    got = oracle_run(g, dt)
    err = {k: rel(v, g[k], scale_of(k, g)) for k, v in got.items()}
    print({k: f"{e:.1e}" for k, e in err.items()})
    assert len(err) == 13 and all(e < tol for e in err.values()), err
    # the running statistics torch's BatchNorm2d left behind are those of the oracle's last convolution (momentum 0.1, unbiased variance)
    if dt == torch.float64:
        sd = {k: g["param." + k].double() for k in PARAMS if not k.startswith("net.7")}
        h = RC.fusion_net(sd, g["rgb"].double(), g["feat"].double(), H, W, B)
        assert rel(0.1 * h.mean(dim=(0, 2, 3)), g["buffer.net.7.running_mean"]) < 1e-5
        assert rel(0.9 + 0.1 * h.var(dim=(0, 2, 3), unbiased=True), g["buffer.net.7.running_var"]) < 1e-5
