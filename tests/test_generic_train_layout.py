"""Train mode of the generic field kernels (csrc/field_generic.hip TRAIN instances), the part a CPU can check: the row map of the
acts / dacts buffers, the argument checks of the new calls, the opt-in switch."""
import ctypes as C

import pytest

from nefes_amd import lib as L
from nefes_amd import ops

SHAPES = [(32, 1), (64, 6), (96, 5), (128, 4), (288, 2), (512, 8)]


def _desc(W, D, C_, fine):
    return L.NefesGenericNetDesc(W, D, 4 if D > 4 else -1, C_, 1 if fine else 0)


def _block_sizes(W, D, C_, fine):
    """Rows of every block NEFES_TB_* computed from (W, D, Hp, Mp) alone."""
    Hp, Mp = (W // 2 + 31) // 32 * 32, (3 + C_ + 31) // 32 * 32
    size = {L.TB_E: 64, L.TB_DV: 32, L.TB_FINAL: W, L.TB_DIR: Hp, L.TB_RGB: Mp, L.TB_SIG: 32, L.TB_TH: 32 if fine else 0}
    for i in range(8):
        size[L.TB_L1 + i] = W if i < D else 0
    for b in (L.TB_T0, L.TB_T1, L.TB_T2):
        size[b] = Hp if fine else 0
    return size


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("C_", [16, 128])
@pytest.mark.parametrize("W,D", SHAPES)
def test_row_map(W, D, C_, fine):
    lib = L.load()
    d = _desc(W, D, C_, fine)
    rows = int(lib.nefes_generic_train_rows(C.byref(d)))
    off = [int(lib.nefes_generic_train_row_offset(C.byref(d), b)) for b in range(L.TB_END + 1)]
    size = _block_sizes(W, D, C_, fine)
    assert all(o >= 0 and o % 32 == 0 for o in off), off
    assert off[0] == 0 and off[L.TB_END] == rows == sum(size.values())
    spans = sorted((off[b], off[b] + size[b]) for b in range(L.TB_END) if size[b])
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, spans                                             # blocks do not overlap
    assert spans[-1][1] <= rows
    for b in range(L.TB_END):
        assert off[b + 1] - off[b] == size[b], (b, off, size)              # ... and follow the enumeration without gaps
    assert rows % 32 == 0


def test_row_map_rejects_bad_arguments():
    lib = L.load()
    d = _desc(64, 6, 16, True)
    assert lib.nefes_generic_train_row_offset(C.byref(d), -1) == -1
    assert lib.nefes_generic_train_row_offset(C.byref(d), L.TB_END + 1) == -1
    bad = L.NefesGenericNetDesc(48, 6, 4, 16, 1)
    assert lib.nefes_generic_train_rows(C.byref(bad)) == 0
    assert lib.nefes_generic_train_row_offset(C.byref(bad), 0) == -2


def test_switch_is_off_by_default_and_shapes_unchanged():
    assert ops.GENERIC_TRAIN is False
    assert "NEFES_GENERIC_TRAIN" in L.GENERIC_SET
    ok = ops.generic_shape_ok
    assert ok(64, 6, [4], 16) and ok(512, 8, [4], 141) and ok(32, 1, [4], 1) and ok(128, 4, [], 16)
    assert not ok(48, 6, [4], 16) and not ok(544, 8, [4], 16) and not ok(64, 9, [4], 16) and not ok(64, 6, [2], 16) and not ok(64, 6, [4], 0)


def test_train_calls_reject_sigma_mode_and_null_buffers():
    """Checked before any launch: these run without a GPU (every pointer is a dummy that is never dereferenced)."""
    lib = L.load()
    d, dc = _desc(64, 6, 16, True), _desc(64, 6, 16, False)
    p = C.c_void_p(4096)
    fwd = lambda desc, mode, **nul: lib.nefes_field_fwd_train_generic(
        C.byref(desc), nul.get("packed", p), mode, 2, 8, nul.get("rays_o", p), p, nul.get("z", p), nul.get("viewdirs", p),
        nul.get("raw_t", p), nul.get("acts", p), nul.get("masks", p), None)
    bwd = lambda desc, mode, **nul: lib.nefes_field_bwd_train_generic(
        C.byref(desc), nul.get("packed", p), mode, 2, 8, p, p, p, nul.get("viewdirs", p), nul.get("raw_t", p), nul.get("g_raw_t", p),
        nul.get("masks", p), nul.get("dacts", p), nul.get("g_pts", p), nul.get("g_vs", p), None)
    assert fwd(d, L.FIELD_SIGMA) == -1 and bwd(d, L.FIELD_SIGMA) == -1
    assert fwd(dc, L.FIELD_FULL) == -1 and bwd(dc, L.FIELD_FULL) == -1     # FULL without a transient head
    for k in ("packed", "rays_o", "z", "viewdirs", "raw_t", "acts", "masks"):
        assert fwd(d, L.FIELD_FULL, **{k: None}) == -1, k
    for k in ("packed", "viewdirs", "raw_t", "g_raw_t", "masks", "dacts", "g_pts", "g_vs"):
        assert bwd(d, L.FIELD_FULL, **{k: None}) == -1, k
    bad = L.NefesGenericNetDesc(48, 6, 4, 16, 1)
    assert fwd(bad, L.FIELD_FULL) == -2 and bwd(bad, L.FIELD_FULL) == -2
    ptrs = (C.c_void_p * 32)(*([4096] * 32))
    assert lib.nefes_generic_pack_device(C.byref(d), ptrs, 32, None, 1 << 30, None) == -1
    assert lib.nefes_generic_pack_device(C.byref(d), None, 32, p, 1 << 30, None) == -1
    assert lib.nefes_generic_pack_device(C.byref(d), ptrs, 30, p, 1 << 30, None) == -1            # 2 * (6 + 10) tensors
    assert lib.nefes_generic_pack_device(C.byref(d), ptrs, 32, p, 16, None) == -1                  # blob too small


def test_blob_header_carries_the_blob_format_not_the_abi_version():
    """The tuned blob's second header word is NEFES_BLOB_FORMAT: it moves with the blob's layout, not with every new call, so packed
    blobs stay byte-identical across an ABI bump (tests/test_pack_ext_c128.py pins their digests)."""
    import os
    import re

    import numpy as np

    from oracle import ref_cpu as O
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nefes_hip.h")).read()
    fmt = int(re.search(r"#define NEFES_BLOB_FORMAT (\d+)", hdr).group(1))
    abi = int(re.search(r"#define NEFES_ABI_VERSION (\d+)", hdr).group(1))
    assert fmt == 17 and abi == L.ABI_VERSION >= 18
    lib = L.load()
    p = O.make_field_params("coarse", 128, 16)
    d = L.NefesNetDesc(128, 16, 0, 0)
    info = L.NefesBlobInfo()
    assert lib.nefes_blob_info(d, info) == 0
    arrs = []
    for n, _, _ in O.field_param_shapes("coarse", 128, 16):
        arrs += [np.ascontiguousarray(p[n + ".weight"].numpy()), np.ascontiguousarray(p[n + ".bias"].numpy())]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    blob = np.zeros(info.total_bytes, np.uint8)
    assert lib.nefes_pack_weights(d, ptrs, len(arrs), blob.ctypes.data, blob.nbytes) == 0
    words = blob[:8].view(np.uint32)
    assert words[0] == 0x5346454e and words[1] == fmt
