"""What a CPU can check of the FusionNet training entry points (csrc/conv.hip nefes_conv2d_wgrad, csrc/refine.hip
nefes_bn_train_bwd_affine): the exports, the workspace size, and every argument check -- those return before any HIP call, so the
pointers here are dummies that are never dereferenced."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from nefes_amd import lib as L

BADARG, UNSUPPORTED = -1, -2
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, Cin, Cout, k, relu, H, W): the shapes of tests/test_gpu_fusion_train.py
SHAPES = [(1, 19, 64, 3, True, 6, 8), (3, 64, 64, 3, True, 5, 7), (2, 64, 16, 5, False, 6, 8), (2, 131, 64, 3, True, 16, 16),
          (1, 3, 5, 5, True, 2, 3), (7, 64, 128, 5, False, 16, 16), (2, 7, 33, 3, True, 9, 33), (1, 1, 1, 5, False, 3, 3)]


def test_names_are_declared_and_exported():
    lib = L.load()
    for name in ("nefes_conv2d_wgrad_workspace", "nefes_conv2d_wgrad", "nefes_bn_train_bwd_affine"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.nefes_version() == 20 == L.ABI_VERSION


def _wgrad(B=2, Cin=19, Cout=64, H=6, W=8, k=3, x=PTR, gy=PTR, mask=None, gw=PTR, gb=PTR, ws=PTR):
    return L.load().nefes_conv2d_wgrad(B, Cin, Cout, H, W, k, x, gy, mask, gw, gb, ws, None)


def test_wgrad_error_codes():
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=-1), dict(H=0), dict(W=0), dict(x=None), dict(gy=None), dict(gw=None), dict(ws=None)):
        assert _wgrad(**kw) == BADARG, kw
    for k in (0, 1, 2, 4, 7):
        assert _wgrad(k=k) == UNSUPPORTED, k
    assert _wgrad(k=4, x=None) == BADARG                              # (null pointers first, as nefes_conv2d_same)
    # a grid that is too large: 2^31 pixels; an image too wide for the tile staged in LDS
    assert _wgrad(B=1 << 15, H=1 << 8, W=1 << 8) == UNSUPPORTED
    assert _wgrad(H=2, W=112, k=5) == UNSUPPORTED and _wgrad(H=2, W=225, k=3) == UNSUPPORTED


def test_bn_affine_error_codes():
    lib = L.load()

    def call(B=3, Cc=7, P=45, x=PTR, w=PTR, save=PTR, gy=PTR, gx=PTR, gw=PTR, gb=PTR):
        return lib.nefes_bn_train_bwd_affine(B, Cc, P, x, w, save, gy, gx, gw, gb, None)
    for kw in (dict(B=0), dict(Cc=0), dict(P=0), dict(P=-3), dict(x=None), dict(save=None), dict(gy=None), dict(gw=None), dict(gb=None)):
        assert call(**kw) == BADARG, kw


def test_workspace_size():
    lib = L.load()
    ws = lib.nefes_conv2d_wgrad_workspace
    assert ws(2, 19, 64, 6, 8, 4) == 0 and ws(2, 19, 64, 6, 8, 1) == 0
    assert ws(0, 19, 64, 6, 8, 3) == 0 and ws(2, 19, 64, 2, 112, 5) == 0 and ws(1 << 15, 1, 1, 1 << 8, 1 << 8, 3) == 0
    assert ws(2, 19, 64, 2, 111, 5) > 0 and ws(2, 19, 64, 2, 224, 3) > 0
    for (B, Cin, Cout, k, _, H, W) in SHAPES:
        n = ws(B, Cin, Cout, H, W, k)
        assert n > 0 and n == ws(B, Cin, Cout, H, W, k), (B, Cin, Cout, k, H, W)
        chunks = (B * H * W + 255) // 256                              # the chunk count depends on (B, H, W, ksize) only
        assert n == chunks * (Cout * Cin * k * k + Cout) * 4


def test_switch_is_off_by_default():
    """NEFES_HIP_FUSION_TRAIN unset: ops.FUSION_TRAIN is False; "1" turns it on (a fresh interpreter: the switch is read at import)."""
    env = {k: v for k, v in os.environ.items() if k != "NEFES_HIP_FUSION_TRAIN"}
    code = ("import os, importlib; from nefes_amd import ops; print(ops.FUSION_TRAIN); os.environ['NEFES_HIP_FUSION_TRAIN'] = '1'; "
            "print(importlib.reload(ops).FUSION_TRAIN)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["False", "True"]
