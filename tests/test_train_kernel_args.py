"""What a CPU can check of the training-backward entry points (csrc/train.hip): the buffer-layout helper the GPU tests build their
operands with, the mirror of the weight-gradient instance table, and every argument check -- those return before any launch, so the
pointers here are dummies that are never dereferenced."""
import ctypes as C

import pytest
import torch

from nefes_amd import lib as L
from nefes_amd import train as TR
from tests import train_kernel_cases as K
from tests.train_layout import from_device, to_device, train_off

BADARG, UNSUPPORTED = -1, -2
PTR = C.c_void_p(4096)


def test_layout_helper_against_rows_view_and_the_offset_formula():
    g = torch.Generator().manual_seed(0)
    b = torch.randn(3, 96, 128, generator=g)
    assert torch.equal(from_device(b), TR.rows_view(b))
    assert torch.equal(to_device(from_device(b)), b) and torch.equal(from_device(to_device(b)), b)
    # ... and both against nefes_train_off written out per element (layout.h), not against a second reshape
    row, smp = torch.meshgrid(torch.arange(96), torch.arange(128), indexing="ij")
    off = train_off(row, smp)
    assert sorted(off.flatten().tolist()) == list(range(96 * 128))
    x = from_device(b)
    for t in range(3):
        assert torch.equal(b[t].flatten()[off], x[t])
        assert torch.equal(to_device(x)[t].flatten()[off], x[t])
    assert train_off(37, 21) == (1 * 8 + 1) * 512 + 5 * 16 + 5


@pytest.mark.parametrize("inst,shape", K.SHAPES, ids=[K.dw_case_id(ot, it, "x6") for _, (ot, it) in K.SHAPES])
def test_dw_grid_mirrors_the_instance_table(inst, shape):
    """train._dw_grid's workgroup count is that of the instance the case is meant for (bf16 kernel: the table of train_dw_impl)."""
    (nto, nti), (ot, it) = inst, shape
    assert K.instance(ot, it, "x6") == (nto, nti)
    assert ot % nto == 0 and it % nti == 0
    assert TR._dw_grid(ot, it)[0] == (ot // nto) * (it // nti)
    assert TR._dw_grid(ot, it)[1] == (1024 if (nto, nti) in ((4, 4), (5, 2), (4, 2)) else 2048)


def test_every_instance_has_a_shape():
    assert {i for i, _ in K.SHAPES} == {(4, 4), (5, 2), (4, 2), (2, 4), (2, 2), (2, 1), (1, 4), (1, 2), (1, 1)}
    assert {K.instance(ot, it, "f32") for _, (ot, it) in K.SHAPES} == {(2, 4), (2, 2), (2, 1), (1, 4), (1, 2), (1, 1)}


def _dw(bias, n_tiles=4, rows=256, g0=0, n_out=64, x0=64, n_in=64, relu=0, splits=2, stride=0, dacts=PTR, acts=PTR, partial=PTR):
    lib = L.load()
    if bias:
        return lib.nefes_train_dw_bias(n_tiles, rows, dacts, g0, n_out, acts, x0, n_in, relu, splits, stride, partial, None)
    return lib.nefes_train_dw(n_tiles, rows, dacts, g0, n_out, acts, x0, n_in, relu, splits, partial, None)


@pytest.mark.parametrize("bias", [0, 1])
def test_dw_rejects_rows_the_kernels_cannot_address(bias):
    """Both weight-gradient kernels address whole 32-row blocks (row0 >> 5) of tiles of `rows` rows."""
    for kw in (dict(g0=8), dict(g0=33), dict(x0=16), dict(x0=95), dict(rows=250), dict(rows=255),
               dict(g0=224), dict(g0=256), dict(x0=224), dict(x0=1 << 30), dict(g0=(1 << 31) - 32),
               dict(rows=96), dict(g0=192, n_out=96), dict(x0=128, n_in=160)):
        assert _dw(bias, **kw) == BADARG, kw
    # (the checks that were there before)
    for kw in (dict(n_tiles=0), dict(rows=0), dict(dacts=None), dict(acts=None), dict(partial=None), dict(splits=0), dict(splits=5),
               dict(n_out=0), dict(n_out=48), dict(n_in=0), dict(n_in=40), dict(g0=-32), dict(x0=-32)):
        assert _dw(bias, **kw) == BADARG, kw
    assert _dw(1, stride=64 * 65 - 1) == BADARG


def _dx(n_tiles=4, rows=512, g0=0, n_out=64, ldw=64, n_in=128, d0=64, accumulate=0, mask=0, dacts_in=PTR, wt=PTR, acts=PTR, dacts_out=PTR):
    return L.load().nefes_train_dx(n_tiles, rows, dacts_in, g0, n_out, wt, ldw, n_in, acts, d0, accumulate, mask, dacts_out, None)


def test_dx_error_codes():
    assert _dx(n_in=96) == UNSUPPORTED and _dx(n_in=32) == UNSUPPORTED and _dx(n_in=512, rows=1024) == UNSUPPORTED
    for kw in (dict(n_out=12, ldw=16), dict(n_out=4, ldw=8), dict(ldw=56), dict(ldw=63), dict(n_out=64, ldw=66), dict(mask=1, acts=None),
               dict(n_tiles=0), dict(rows=0), dict(dacts_in=None), dict(wt=None), dict(dacts_out=None), dict(n_out=0), dict(g0=-1), dict(d0=-1)):
        assert _dx(**kw) == BADARG, kw
    # both row ranges inside the tile
    for kw in (dict(g0=449), dict(g0=512), dict(g0=(1 << 31) - 8), dict(d0=385), dict(d0=(1 << 31) - 1), dict(rows=191), dict(rows=63, d0=0),
               dict(n_in=256, d0=257)):
        assert _dx(**kw) == BADARG, kw
    assert _dx(n_in=96, d0=417) == BADARG                 # (range check first: an unsupported width outside the tile is a bad argument)


def test_head_grad_error_codes():
    lib = L.load()
    fine, coarse = L.NefesNetDesc(256, 16, 1, 0, 0), L.NefesNetDesc(256, 16, 0, 0, 0)
    call = lambda d, mode, N=5, S=33, raw=PTR, g=PTR, dacts=PTR: lib.nefes_train_head_grad(C.byref(d), mode, N, S, raw, g, dacts, None)
    assert call(coarse, L.FIELD_FULL) == BADARG           # the full head of a network without a transient head
    assert call(fine, L.FIELD_SIGMA) == UNSUPPORTED and call(fine, 3) == UNSUPPORTED
    for kw in (dict(N=0), dict(S=0), dict(raw=None), dict(g=None), dict(dacts=None)):
        assert call(fine, L.FIELD_FULL, **kw) == BADARG, kw
    assert lib.nefes_train_head_grad(None, L.FIELD_FULL, 5, 33, PTR, PTR, PTR, None) == BADARG
