"""Shared helpers of tests/test_generic_field.py and tests/test_gpu_generic_field.py (the generic field kernels,
nefes_amd/csrc/field_generic.hip): networks of any width / depth, the oracle at that depth, the kernels' mask words decoded."""
import contextlib
import functools
import types

import numpy as np
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import parity_log as P

SHAPES = [(64, 6), (192, 8), (512, 8), (128, 4), (256, 2), (96, 5), (32, 1)]
CASES = [f"w{W}d{D}c{C}" for (W, D) in SHAPES for C in (16, 128)] + ["w64d6c16_reduced"]


def modules(Wd, D, C, in_xyz=63, in_dir=27, device=None):
    from nefes_amd.field import NeRFH_NFF
    coarse = NeRFH_NFF('coarse', D=D, W=Wd, skips=[4], in_channels_xyz=in_xyz, in_channels_dir=in_dir, f_dim=C).requires_grad_(False)
    fine = NeRFH_NFF('fine', D=D, W=Wd, skips=[4], in_channels_xyz=in_xyz, in_channels_dir=in_dir, encode_appearance=True,
                     encode_transient=True, in_channels_a=50, in_channels_t=20, f_dim=C).requires_grad_(False)
    if device is not None:
        coarse, fine = coarse.to(device), fine.to(device)
    return coarse, fine


def oracle_params(net, dtype):
    return {k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items() if not k.startswith(("fusion_net", "exposure_embedding"))}


@contextlib.contextmanager
def oracle_depth(D):
    """oracle/ref_cpu.py's field_forward takes D and skip, its query_field / render do not pass them on: give them the depth."""
    orig = O.field_forward
    O.field_forward = functools.partial(orig, D=D, skip=4)
    try:
        yield
    finally:
        O.field_forward = orig


def render_kwargs(coarse, fine, Nc, Ni, transient_at_test=True, test_time=True):
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=transient_at_test, netchunk=1 << 21)
    return dict(network_query_fn=None, perturb=False, N_importance=Ni, N_samples=Nc, network_fn=coarse, network_fine=fine,
                use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=test_time, args=args, ndc=False, lindisp=False)


def rho(h, r):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def mask_slots(Wd, D):
    """(tag, first row block, row blocks, units) of every hidden layer in a tile's mask words (csrc/field_generic.hip gen_layout)."""
    H = Wd // 2
    out, rb = [], 0
    for i in range(D):
        out.append((f"L{i + 1}", rb, Wd // 32, Wd))
        rb += Wd // 32
    for t in ("DIR", "T0", "T1", "T2"):
        out.append((t, rb, (H + 31) // 32, H))
        rb += (H + 31) // 32
    return out, rb


def decode_masks_generic(masks, M, Wd, D):
    """int32 words [tiles][words][64 lanes] -> {tag: bool [M, units]}, True = pre-activation not positive (ReLU derivative 0).
    Bit 16 c + r of a word = accumulator r of column block c: sample 32 c + lane % 32 of the tile, feature 32 rb + rho(lane / 32, r)."""
    TS = 64 if Wd <= 256 else 32
    slots, words = mask_slots(Wd, D)
    a = masks.detach().cpu().numpy().view(np.uint32).reshape(-1, words, 64)
    tiles = (M + TS - 1) // TS
    a = a[:tiles]
    lane = np.arange(64)
    l31, half = lane & 31, lane >> 5
    out = {}
    for tag, rb0, nrb, units in slots:
        up = ((units + 31) // 32) * 32
        neg = np.zeros((tiles * TS, up), bool)
        for rb in range(nrb):
            word = a[:, rb0 + rb, :]                                      # [tiles, 64]
            for c in range(TS // 32):
                for r in range(16):
                    act = ((word >> np.uint32(16 * c + r)) & np.uint32(1)).astype(bool)
                    rows = np.arange(tiles)[:, None] * TS + 32 * c + l31[None, :]
                    feat = (32 * rb + rho(half, r))[None, :].repeat(tiles, 0)
                    neg[rows, feat] = ~act
        out[tag] = neg[:M, :units]
    return out


class GenericPinned(B.Pinned):
    """tests/branch.py Pinned from the generic kernels' tap entry (ops.TAP['masks_generic'])."""

    def __init__(self, tap, index=-1):
        masks, N, S, pk, mode = tap["masks_generic"][index]
        self.N, self.S = N, S
        self.neg = {k: torch.from_numpy(v) for k, v in decode_masks_generic(masks, N * S, pk.width, pk.depth).items()}
        self.z_fine = tap["z_fine"][-1].detach().cpu() if tap.get("z_fine") and tap["z_fine"][-1] is not None else None
        self.audit = {}


def pinned_gradients_generic(tag, hip, tap, oracle_run, tol=P.NORTH_STAR_TOL, audit="same_inputs"):
    """tests/branch.py pinned_gradients for the generic kernels' masks: same audit, same rule e_hip <= max(tol, 1.5 e_ref)."""
    pin = GenericPinned(tap)
    g64 = oracle_run(torch.float64, pin.act(True), pin.z_fine)
    g32 = oracle_run(torch.float32, pin.act(False), pin.z_fine)
    flips, units, worst = pin.summary()
    print(f"[{tag}] ReLU branch pattern vs float64: {flips} of {units} units differ, worst |pre-activation| / layer max {worst:.1e}")
    P.record(tag, "relu branch flips vs float64", flips=flips, units=units, worst_preact_rel=worst)
    audit_tol = B.AUDIT_CLASSES[audit]
    assert worst < audit_tol and flips <= max(8, units // 100000) * (audit_tol / 2e-5), (flips, units, worst)
    return {name: B.three_way(tag, name + " [branch-pinned]", hip[name], g32[name], g64[name], tol=tol) for name in hip}
