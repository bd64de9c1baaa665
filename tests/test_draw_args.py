"""CPU-side tests of the device-side pixel draw (nefes_draw_pixels, ops.draw_pixels, PoseRefiner(sparse=K, redraw=R)): the ABI's names and
refusals, the numpy reference of its contract (tests/draw_ref.py: known answers, distinctness, uniformity, masks) and the refiner's
argument handling.  What the kernels compute is compared with that reference in tests/test_gpu_draw.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from tests import draw_ref as R

BADARG = -1
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_draw_pixels_workspace", "nefes_draw_pixels")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.nefes_version() == L.ABI_VERSION == 20


def test_refusals_come_before_any_hip_call():
    """Dummy pointers, no GPU: every refusal returns NEFES_E_BADARG."""
    lib = L.load()

    def call(B=2, H=12, W=16, mask=PTR, K=48, period=1, state=PTR, advance=1, px=PTR, n_valid=PTR, ws=PTR):
        return lib.nefes_draw_pixels(B, H, W, mask, K, period, state, advance, px, n_valid, ws, None)
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-3), dict(K=0), dict(K=-5), dict(period=0), dict(period=-2),
               dict(K=12 * 16 + 1), dict(H=4096, W=4097), dict(H=1 << 16, W=1 << 16), dict(state=None), dict(px=None), dict(ws=None),
               dict(mask=None, state=None), dict(n_valid=None, px=None)):
        assert call(**kw) == BADARG, kw


def test_workspace_is_positive_and_monotone():
    q = L.load().nefes_draw_pixels_workspace
    assert q(1, 1, 1) > 0
    base = (2, 33, 65)
    for axis in range(3):
        last = 0
        for v in (1, 2, 3, 31, 32, 33, 64, 65, 127, 128, 129, 480, 854, 4096):
            a = list(base)
            a[axis] = v
            assert q(*a) >= last and q(*a) > 0, (axis, v)
            last = q(*a)
    # the keys alone are 8 bytes per pixel, and 1 << 24 pixels are accepted
    assert q(3, 60, 80) >= 3 * 60 * 80 * 8 and q(1, 4096, 4096) >= (1 << 24) * 8


def test_reference_reproduces_philox_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert tuple(int(x) for x in R.philox(*counter, *key)) == want, [hex(int(x)) for x in R.philox(*counter, *key)]
    # ... on arrays as on scalars
    cols = [np.array([kat[0][k] for kat in R.KNOWN_ANSWERS[:1] * 3], np.uint64) for k in range(4)]
    assert [int(o[2]) for o in R.philox(*cols, 0, 0)] == list(R.KNOWN_ANSWERS[0][2])


def _counts(H, W, K, seed, epochs, mask=None):
    cnt = np.zeros(H * W, int)
    for e in range(epochs):
        sel, nv = R.draw_indices(H, W, K, seed, e, mask=mask)
        assert len(sel) == K and (np.diff(sel) > 0).all() and sel[0] >= 0 and sel[-1] < H * W, (seed, e)   # distinct, ascending, in frame
        if mask is not None:
            assert nv == int((mask != 0).sum()) and (mask.reshape(-1)[sel] != 0).all(), (seed, e)
        cnt[sel] += 1
    return cnt


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_reference_draws_are_distinct_and_uniform(seed):
    """12 x 16, K = 48, epochs 0..1999: every pixel's inclusion count within 5 sd of 500, sd = sqrt(2000 * 0.25 * 0.75) = 19.36.  A
    selection that is biased (the first K, a truncated key) misses that by a wide margin."""
    cnt = _counts(12, 16, 48, seed, 2000)
    sd = (2000 * 0.25 * 0.75) ** 0.5
    worst = np.abs(cnt - 500).max() / sd
    print(f"seed {seed}: worst deviation {worst:.2f} sd")
    assert worst <= 5.0, worst


def holed_checkerboard():
    m = np.zeros((12, 16), np.uint8)
    m[::2, ::2] = 1
    m[1::2, 1::2] = 1
    m[3:9, 4:12] = 0
    return m


def test_reference_respects_a_mask():
    m = holed_checkerboard()
    nv = int(m.sum())
    assert nv == 72
    cnt = _counts(12, 16, 24, 7, 2000, mask=m)
    assert cnt[m.reshape(-1) == 0].sum() == 0
    p = 24 / nv
    sd = (2000 * p * (1 - p)) ** 0.5
    worst = np.abs(cnt[m.reshape(-1) != 0] - 2000 * p).max() / sd
    print(f"masked: worst deviation {worst:.2f} sd")
    assert worst <= 5.0, worst


def test_reference_repeats_too_few_valid_pixels_cyclically():
    m = np.zeros((12, 16), np.uint8)
    m[5, 3:8] = 1
    sel, nv = R.draw_indices(12, 16, 12, 7, 0, mask=m)
    assert nv == 5 and sel.tolist() == [5 * 16 + 3 + j % 5 for j in range(12)]
    px, n = R.draw(1, 12, 16, 12, 7, 0, mask=m[None])
    assert n.tolist() == [5] and px[0, :, 1].tolist() == [5.] * 12 and px[0, :, 0].tolist() == [3. + j % 5 for j in range(12)]
    px, n = R.draw(2, 12, 16, 12, 7, 0, mask=np.stack([np.zeros_like(m), m]))
    assert n.tolist() == [0, 5] and not px[0].any()
    # the epoch is tick // period, and an image's draw depends on its index
    assert np.array_equal(R.draw(1, 12, 16, 12, 7, 5, period=3)[0], R.draw(1, 12, 16, 12, 7, 1)[0])
    two = R.draw(2, 12, 16, 12, 7, 0)[0]
    assert not np.array_equal(two[0], two[1])


def test_draw_state_and_draw_pixels_arguments():
    from nefes_amd import ops
    s = ops.draw_state(2 ** 40 + 3, "cpu")
    assert s.dtype == torch.int64 and s.tolist() == [2 ** 40 + 3, 0]
    assert ops.draw_state(2 ** 63 - 1, "cpu").tolist() == [2 ** 63 - 1, 0]
    for bad in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="seed"):
            ops.draw_state(bad, "cpu")
    for kw in (dict(K=0), dict(K=193), dict(period=0), dict(B=0)):
        with pytest.raises(ValueError, match="draw_pixels"):
            ops.draw_pixels(12, 16, **dict(dict(K=4, state=s), **kw))
    with pytest.raises(RuntimeError, match="mask"):
        ops.draw_pixels(12, 16, 4, s, mask=torch.ones(12, 16))
    with pytest.raises(RuntimeError, match="mask"):
        ops.draw_pixels(12, 16, 4, s, mask=torch.ones(2, 12, 16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out"):
        ops.draw_pixels(12, 16, 4, s, out=torch.zeros(5, 2))


def _make_refiner():
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    return lambda **more: PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", **more)


def test_redraw_refiner_arguments():
    """Construction only, on the CPU device: it allocates buffers and launches nothing."""
    make = _make_refiner()
    with pytest.raises(ValueError, match="redraw"):
        make(redraw=2)                                                        # without sparse=
    for bad in (0, -3):
        with pytest.raises(ValueError, match="redraw"):
            make(sparse=7, redraw=bad)
    r = make(sparse=7, redraw=2, seed=11)
    assert r.redraw == 2 and r.draw_state.dtype == torch.int64 and r.draw_state.tolist() == [11, 0]
    assert r._mask_u8 is None and r.mask is None and tuple(r.pixels.shape) == (7, 2)
    m = make(sparse=7, redraw=1, masked=True)
    assert tuple(m._mask_u8.shape) == (1, 10, 15) and m._mask_u8.dtype == torch.uint8 and bool(m._mask_u8.all())
    assert tuple(m.mask.shape) == (1, 7) and bool(m.mask.all())
    with pytest.raises(ValueError, match="redraw"):
        r.set_pixels(torch.zeros(7, 2))
    with pytest.raises(ValueError, match="pixels="):
        r.refine(torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(10), 0, pixels=torch.zeros(7, 2))
    # what the sparse refusals pinned stays refused with redraw= next to them
    for more in (dict(images=2), dict(upsample=True), dict(fused_glue=False), dict(lietorch=True)):
        with pytest.raises(NotImplementedError, match="sparse"):
            make(sparse=7, redraw=1, **more)


def test_sparse_refiner_without_redraw_draws_on_the_host_as_before():
    make = _make_refiner()
    r = make(sparse=7)
    assert r.redraw is None and not hasattr(r, "draw_state") and not hasattr(r, "_mask_u8")
    h, w = 10, 15
    g = torch.Generator().manual_seed(0)
    valid = torch.arange(h * w)
    idx = valid[torch.randperm(valid.numel(), generator=g)[:7]]
    assert torch.equal(r._draw_pixels(None), torch.stack([idx % w, idx // w], -1))
    # ... among a mask's valid pixels (a second draw of the same generator, as a second image's would be)
    fm = torch.zeros(h, w, dtype=torch.bool)
    fm[2:7, 3:11] = True
    valid = fm.reshape(-1).nonzero().flatten()
    idx = valid[torch.randperm(valid.numel(), generator=g)[:7]]
    assert torch.equal(r._draw_pixels(fm), torch.stack([idx % w, idx // w], -1))
    with pytest.raises(ValueError, match="valid ones"):
        r._draw_pixels(torch.zeros(h, w, dtype=torch.bool))
