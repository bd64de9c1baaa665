"""What a CPU can check of the per-pixel feature loss (`--per_pixel`; csrc/feature_loss.hip pixcos_* / uppixcos_*): the exports, the scratch
queries, every refusal of the entry points (they return before any HIP call: the pointers are dummies that are never dereferenced),
the `out=` validation of the two ops functions, and that PoseRefiner no longer refuses per_pixel=True with pose_model= or images=B.
The GPU twins are tests/test_gpu_pixcos.py and tests/test_gpu_refine_pp.py."""
import ctypes as C
import os
import types

import pytest
import torch

from nefes_amd import lib as L

BADARG = -1
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_pixcos_scratch_doubles", "nefes_pixcos_loss_fwd", "nefes_pixcos_loss_bwd", "nefes_uppixcos_scratch_doubles",
         "nefes_uppixcos_loss_fwd", "nefes_uppixcos_loss_bwd")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.nefes_version() == L.ABI_VERSION == 20


def test_scratch_queries_are_monotone():
    q, qu = L.load().nefes_pixcos_scratch_doubles, L.load().nefes_uppixcos_scratch_doubles
    assert q(0, 10) == 0 and q(1, 0) == 0 and q(-1, 5) == 0 and qu(0, 8, 8, 0) == 0 and qu(1, 20, 20, 10) == 0 and qu(1, 8, 8, -1) == 0
    sizes = (1, 63, 64, 65, 255, 256, 257, 4800, 66000, 1 << 20)
    for G in (1, 2, 3, 8):
        vals = [q(G, P) for P in sizes]
        assert all(a < b for a, b in zip(vals, vals[1:])), (G, vals)
        assert all(q(G, P) < q(G + 1, P) for P in sizes)
        assert all(q(G, P) >= G * (3 * P + 2) for P in sizes)            # three numbers per pixel, a mean and >= one partial per group
    assert q(1, 4800) == 1 + 3 * 4800 + 75                               # mean | stats [3][P] | one partial per 64 pixels
    # the up-sampled form: three numbers per window pixel, one partial per 64 columns of a window row, one mean -- per group
    for G, OH, OW, crop in ((1, 240, 320, 10), (3, 60, 80, 10), (1, 31, 45, 3), (2, 32, 32, 0)):
        CH, CW = OH - 2 * crop, OW - 2 * crop
        assert qu(G, OH, OW, crop) == G * (1 + 3 * CH * CW + CH * -(-CW // 64))
        assert qu(G, OH, OW, crop) < qu(G + 1, OH, OW, crop) and qu(G, OH, OW, crop) < qu(G, OH + 1, OW, crop) < qu(G, OH + 1, OW + 1, crop)


def test_refusals():
    lib = L.load()
    fwd = lambda G=1, Cc=4, P=100, a=PTR, b=PTR, s=PTR, l=PTR: lib.nefes_pixcos_loss_fwd(G, Cc, P, a, b, s, l, None)
    bwd = lambda G=1, Cc=4, P=100, a=PTR, b=PTR, s=PTR, g=PTR, o=PTR: lib.nefes_pixcos_loss_bwd(G, Cc, P, a, b, s, g, o, None)
    for call in (fwd, bwd):
        for kw in (dict(G=0), dict(G=-1), dict(G=65536), dict(Cc=0), dict(P=0), dict(P=-7), dict(a=None), dict(b=None), dict(s=None)):
            assert call(**kw) == BADARG, kw
    assert fwd(l=None) == BADARG and bwd(g=None) == BADARG and bwd(o=None) == BADARG
    geo = dict(G=1, Cc=4, h=6, w=8, OH=24, OW=32, crop=2)
    ufwd = lambda x=PTR, t=PTR, s=PTR, l=PTR, **kw: lib.nefes_uppixcos_loss_fwd(*{**geo, **kw}.values(), x, t, s, l, None)

    def ubwd(x=PTR, t=PTR, s=PTR, g=PTR, tabs=(PTR,) * 6, T=20, tmp=PTR, gx=PTR, **kw):
        return lib.nefes_uppixcos_loss_bwd(*{**geo, **kw}.values(), x, t, s, g, *tabs, T, tmp, gx, None)
    for call in (ufwd, ubwd):
        for kw in (dict(G=0), dict(G=65536), dict(Cc=0), dict(h=0), dict(w=-1), dict(crop=-1), dict(crop=12), dict(OW=4), dict(x=None), dict(t=None),
                   dict(s=None)):
            assert call(**kw) == BADARG, kw
    assert ufwd(l=None) == BADARG
    for kw in (dict(g=None), dict(tmp=None), dict(gx=None), dict(T=0), dict(tabs=(None,) + (PTR,) * 5), dict(tabs=(PTR,) * 5 + (None,))):
        assert ubwd(**kw) == BADARG, kw


def test_out_is_validated_before_anything_is_launched():
    """`out=` goes through ops._loss_buffer as for the per-channel functions: a buffer of the wrong kind is a ValueError (raised before
    the first device pointer is taken, so CPU tensors show it)."""
    from nefes_amd import ops
    a, b = torch.randn(4, 50), torch.randn(4, 50)
    x, t = torch.randn(4, 5, 6), torch.randn(4, 20, 24)
    for bad in (torch.zeros(1), torch.zeros((), dtype=torch.float64), torch.zeros(()).requires_grad_(), 1.0):
        with pytest.raises(ValueError, match="`out`"):
            ops.pixel_cosine_loss(a, b, out=bad)
        with pytest.raises(ValueError, match="`out`"):
            ops.upsampled_pixel_cosine_loss(x, t, (20, 24), out=bad)
    with pytest.raises(ValueError, match="groups"):
        ops.pixel_cosine_loss(a, b, groups=3)
    with pytest.raises(ValueError, match="groups"):
        ops.upsampled_pixel_cosine_loss(x, t, (20, 24), groups=3)
    with pytest.raises(ValueError, match="different shapes"):
        ops.pixel_cosine_loss(a, b[:, :49])
    with pytest.raises(RuntimeError, match="no CPU path"):               # and a good buffer gets as far as the device check: no eager fall-back
        ops.pixel_cosine_loss(a, b, out=torch.zeros(()))


def test_refiner_accepts_per_pixel_in_every_form():
    """PoseRefiner(pose_model=..., per_pixel=True) and PoseRefiner(images=2, per_pixel=True) raised NotImplementedError; lietorch and
    fused_glue=False with images > 1 still do.  (Construction only, on the CPU device: it allocates buffers and launches nothing.)"""
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    make = lambda **more: PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", per_pixel=True, **more)
    apr = torch.nn.Linear(12, 12)
    for ref in (make(), make(upsample=True), make(pose_model=apr, svd_reg=True), make(images=2), make(images=2, upsample=True)):
        assert ref.per_pixel and not ref._uses_prepared_target()
    assert make(pose_model=apr).upsample and tuple(make(images=2, upsample=True).target.shape) == (2, 16, 20, 40)
    for more in (dict(images=2, lietorch=True), dict(images=2, fused_glue=False), dict(images=2, pose_model=apr)):
        with pytest.raises(NotImplementedError):
            make(**more)
