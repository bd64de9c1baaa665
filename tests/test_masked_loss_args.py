"""What a CPU can check of the masked feature losses (`--semantic`; csrc/feature_loss.hip MASKED instances): the exports, the scratch queries,
every refusal of the entry points (they return before any HIP call: the pointers are dummies that are never dereferenced), the mask
validation of the four ops functions (raised before the first device pointer is taken, so CPU tensors show it), and PoseRefiner's
`masked=` / `mask=`.  The GPU twins are tests/test_gpu_masked_loss.py and tests/test_gpu_refine_masked.py."""
import ctypes as C
import os
import types

import pytest
import torch

from nefes_amd import lib as L

BADARG = -1
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_cosine_loss_masked_fwd", "nefes_cosine_loss_masked_bwd", "nefes_upcos_loss_masked_fwd", "nefes_upcos_loss_masked_bwd",
         "nefes_pixcos_masked_scratch_doubles", "nefes_pixcos_loss_masked_fwd", "nefes_pixcos_loss_masked_bwd",
         "nefes_uppixcos_masked_scratch_doubles", "nefes_uppixcos_loss_masked_fwd", "nefes_uppixcos_loss_masked_bwd")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    # the unmasked entry points keep their signatures
    assert len(L.SIGNATURES["nefes_cosine_loss_fwd"][1]) == 7 and len(L.SIGNATURES["nefes_pixcos_loss_fwd"][1]) == 8
    assert len(L.SIGNATURES["nefes_upcos_loss_fwd"][1]) == 11 and len(L.SIGNATURES["nefes_uppixcos_loss_fwd"][1]) == 12


def test_scratch_queries_are_monotone():
    lib = L.load()
    q, qm, qu, qum = (lib.nefes_pixcos_scratch_doubles, lib.nefes_pixcos_masked_scratch_doubles, lib.nefes_uppixcos_scratch_doubles,
                      lib.nefes_uppixcos_masked_scratch_doubles)
    assert qm(0, 10) == 0 and qm(1, 0) == 0 and qm(-1, 5) == 0 and qum(0, 8, 8, 0) == 0 and qum(1, 20, 20, 10) == 0 and qum(1, 8, 8, -1) == 0
    sizes = (1, 63, 64, 65, 255, 256, 257, 4800, 66000, 1 << 20)
    for G in (1, 2, 3, 8):
        vals = [qm(G, P) for P in sizes]
        assert all(a < b for a, b in zip(vals, vals[1:])), (G, vals)
        assert all(qm(G, P) < qm(G + 1, P) for P in sizes)
        # the unmasked layout, one count per partial and one count per group
        assert all(qm(G, P) == q(G, P) + G * (1 + -(-P // 64)) for P in sizes)
    for G, OH, OW, crop in ((1, 240, 320, 10), (3, 60, 80, 10), (1, 31, 45, 3), (2, 32, 32, 0)):
        CH, CW = OH - 2 * crop, OW - 2 * crop
        assert qum(G, OH, OW, crop) == qu(G, OH, OW, crop) + G * (1 + CH * -(-CW // 64))
        assert qum(G, OH, OW, crop) < qum(G + 1, OH, OW, crop) and qum(G, OH, OW, crop) < qum(G, OH + 1, OW, crop) < qum(G, OH + 1, OW + 1, crop)


def test_refusals():
    lib = L.load()
    low = dict(G=1, Cc=4, P=100)
    common = (dict(G=0), dict(G=-1), dict(Cc=0), dict(P=0), dict(P=-7), dict(a=None), dict(b=None), dict(m=None), dict(s=None))
    for stem, more in (("cosine", ()), ("pixcos", (dict(G=65536),))):
        fwd_f, bwd_f = getattr(lib, f"nefes_{stem}_loss_masked_fwd"), getattr(lib, f"nefes_{stem}_loss_masked_bwd")
        fwd = lambda a=PTR, b=PTR, m=PTR, s=PTR, l=PTR, **kw: fwd_f(*{**low, **kw}.values(), a, b, m, s, l, None)
        bwd = lambda a=PTR, b=PTR, m=PTR, s=PTR, g=PTR, o=PTR, **kw: bwd_f(*{**low, **kw}.values(), a, b, m, s, g, o, None)
        for call in (fwd, bwd):
            for kw in common + more:
                assert call(**kw) == BADARG, (stem, kw)
        assert fwd(l=None) == BADARG and bwd(g=None) == BADARG and bwd(o=None) == BADARG
    geo = dict(G=1, Cc=4, h=6, w=8, OH=24, OW=32, crop=2)
    ucommon = (dict(G=0), dict(Cc=0), dict(h=0), dict(w=-1), dict(crop=-1), dict(crop=12), dict(OW=4), dict(x=None), dict(t=None), dict(m=None),
               dict(s=None))
    for stem, more in (("upcos", ()), ("uppixcos", (dict(G=65536),))):
        fwd_f, bwd_f = getattr(lib, f"nefes_{stem}_loss_masked_fwd"), getattr(lib, f"nefes_{stem}_loss_masked_bwd")
        ufwd = lambda x=PTR, t=PTR, m=PTR, s=PTR, l=PTR, **kw: fwd_f(*{**geo, **kw}.values(), x, t, m, s, l, None)

        def ubwd(x=PTR, t=PTR, m=PTR, s=PTR, g=PTR, tabs=(PTR,) * 6, T=20, tmp=PTR, gx=PTR, **kw):
            return bwd_f(*{**geo, **kw}.values(), x, t, m, s, g, *tabs, T, tmp, gx, None)
        for call in (ufwd, ubwd):
            for kw in ucommon + more:
                assert call(**kw) == BADARG, (stem, kw)
        assert ufwd(l=None) == BADARG
        for kw in (dict(g=None), dict(tmp=None), dict(gx=None), dict(T=0), dict(tabs=(None,) + (PTR,) * 5), dict(tabs=(PTR,) * 5 + (None,))):
            assert ubwd(**kw) == BADARG, (stem, kw)


def test_masks_are_validated_before_anything_is_launched():
    from nefes_amd import ops
    a, b = torch.randn(6, 5, 10), torch.randn(6, 5, 10)
    x, t = torch.randn(6, 5, 6), torch.randn(6, 20, 24)
    ok_low, ok_up = torch.ones(1, 5, 10, dtype=torch.uint8), torch.ones(1, 20, 24, dtype=torch.uint8)
    low_fns = (ops.cosine_feature_loss, ops.pixel_cosine_loss)
    up_fns = (ops.upsampled_cosine_loss, ops.upsampled_pixel_cosine_loss)
    calls = [(lambda m, f=f, **kw: f(a, b, mask=m, **kw), ok_low) for f in low_fns] + \
            [(lambda m, f=f, **kw: f(x, t, (20, 24), mask=m, **kw), ok_up) for f in up_fns]
    for call, ok in calls:
        with pytest.raises(ValueError, match="uint8"):
            call(ok.bool())
        with pytest.raises(ValueError, match="uint8"):
            call(ok.float())
        with pytest.raises(ValueError, match="shape"):
            call(ok[:, :, :-1].contiguous())
        with pytest.raises(ValueError, match="shape"):
            call(torch.ones((6,) + tuple(ok.shape[1:]), dtype=torch.uint8))           # one plane per CHANNEL is not the layout
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.ones(1, ok.shape[2], ok.shape[1], dtype=torch.uint8).transpose(1, 2))
        with pytest.raises(ValueError, match="not a tensor"):
            call([[1]])
        with pytest.raises(ValueError, match="groups"):
            call(ok, groups=4)
        with pytest.raises(ValueError, match="shape"):
            call(ok, groups=2)                                                        # two groups need two planes
        with pytest.raises(ValueError, match="`out`"):
            call(ok, out=torch.zeros(1))
        if torch.cuda.is_available():
            with pytest.raises(ValueError, match="is on"):
                call(ok.cuda())
        with pytest.raises(RuntimeError, match="no CPU path"):           # a good mask gets as far as the device check: no eager fall-back
            call(ok)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(torch.ones(2, *ok.shape[1:], dtype=torch.uint8), groups=2)
    # groups= on the two channel-wise functions without a mask: validated, then today's kernels
    with pytest.raises(ValueError, match="groups"):
        ops.cosine_feature_loss(a, b, groups=4)
    with pytest.raises(ValueError, match="groups"):
        ops.upsampled_cosine_loss(x, t, (20, 24), groups=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cosine_feature_loss(a, b, groups=2)


def _make(**more):
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    return PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", **more)


def test_refiner_constructs_masked_in_every_form():
    """Construction only, on the CPU device: it allocates buffers and launches nothing."""
    apr = torch.nn.Linear(12, 12)
    forms = [dict(), dict(upsample=True), dict(per_pixel=True), dict(per_pixel=True, upsample=True), dict(pose_model=apr, svd_reg=True),
             dict(pose_model=apr, per_pixel=True), dict(images=2), dict(images=2, upsample=True), dict(images=2, per_pixel=True, upsample=True),
             dict(intrinsics=(12., 12., 7.5, 5.)), dict(learn_focal=True), dict(fused_glue=False), dict(fused_glue=False, per_pixel=True)]
    for form in forms:
        ref = _make(masked=True, **form)
        B = form.get("images", 1)
        th, tw = (20, 40) if ref.upsample else (10, 15)
        assert ref.masked and not ref._uses_prepared_target(), form
        assert ref.mask.dtype == torch.uint8 and tuple(ref.mask.shape) == (B, th, tw) and bool(ref.mask.all()) and ref.mask.is_contiguous(), form
        assert tuple(ref.target.shape[-2:]) == (th, tw)
    assert _make().mask is None and not _make().masked
    for more in (dict(images=2, lietorch=True), dict(images=2, fused_glue=False), dict(images=2, pose_model=apr)):
        with pytest.raises(NotImplementedError):
            _make(masked=True, **more)


def test_masks_reach_the_refiner_buffer_or_are_refused():
    ref = _make(masked=True)
    buf = ref.mask.data_ptr()
    m = torch.zeros(10, 15)
    m[2:5, 3:9] = 0.5
    for form in (m, m[None], m > 0, (m > 0).to(torch.uint8)[None], m.double() * 4):
        ref.mask.fill_(7)
        ref._set_mask(form)
        assert ref.mask.data_ptr() == buf and torch.equal(ref.mask[0], (m > 0).to(torch.uint8))
    ref._set_mask(None)
    assert bool((ref.mask == 1).all())
    with pytest.raises(ValueError, match="no valid pixel"):
        ref._set_mask(torch.zeros(10, 15))
    assert bool((ref.mask == 1).all())                                   # a refused mask leaves the buffer alone
    with pytest.raises(ValueError, match="shape"):
        ref._set_mask(torch.ones(15, 10))
    two = _make(masked=True, images=2)
    mm = torch.stack([m, 1 - m])
    two._set_mask(mm)
    assert torch.equal(two.mask, (mm > 0).to(torch.uint8))
    two._set_mask(mm[:, None])
    with pytest.raises(ValueError, match=r"image\(s\) \[1\]"):
        two._set_mask(torch.stack([m, torch.zeros_like(m)]))
    with pytest.raises(ValueError, match="shape"):
        two._set_mask(m)


def test_mask_on_an_unmasked_refiner_names_the_flag():
    ref = _make()
    z = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="masked=True"):
        ref.refine(torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(1, 10), iters=0, mask=torch.ones(10, 15))
    apr = _make(pose_model=torch.nn.Linear(12, 12))
    with pytest.raises(ValueError, match="masked=True"):
        apr.refine_apr(torch.zeros(1, 3, 40, 60), torch.zeros(16, 40, 60), torch.zeros(1, 10), iters=0, mask=torch.ones(20, 40))
    # an image without a valid pixel is refused when the mask is set, before anything runs
    with pytest.raises(ValueError, match="no valid pixel"):
        _make(masked=True).refine(torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(1, 10), iters=0, mask=torch.zeros(10, 15))
