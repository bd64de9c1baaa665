"""The hash-grid kernels of csrc/hashgrid.hip -- nefes_hashgrid_fwd, nefes_hashgrid_bwd_x, nefes_hashgrid_bwd_table in both scatter forms --
against the float64 reference of tests/hashgrid_ref.py, PER ELEMENT, at six geometries (all levels dense, all hashed, level counts 1, 3, 5,
16), on both sides of the bound, at launch shapes ragged against every tile (M = 1, 3, 63, 64, 65, 257, 1000):

    |kernel - float64| <= budget     for every element, no factor on top;

the budget of every element comes from the reference's own derivatives (tests/hashgrid_ref.py states each term and the rounding it
accounts for; tests/test_hashgrid_ref.py shows on the CPU that an fp32 restatement of the kernels stays inside 0.75 x budget and that ten
wrong references are more than 10 x budget away).  Every launch writes into buffers with sentinel-filled tails, compared bit for bit
afterwards.  The last test repeats the fused-kernel comparison of tests/test_gpu_cam.py at a second geometry with a third of the samples
outside the bound.  The reference of a (geometry, set, M) is computed once and shared by the tests that need it."""
import ctypes
import functools
import itertools

import pytest
import torch

from tests import hashgrid_ref as R
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 8                          # sentinel rows behind every output
SENTINEL = -7.25
GEOS = list(R.GEOMETRIES)
CASES = [(g, k, m) for g in GEOS for k in R.SETS for m in R.MS]
IDS = [f"{g}-{k}-{m}" for g, k, m in CASES]


@functools.lru_cache(maxsize=None)
def tables(geo_name):
    """(fp32 table on the GPU, the same values in float64 on the CPU), built once per geometry"""
    t = R.make_table(R.geometry(geo_name))
    return t.to(DEV).contiguous(), t.double()


@functools.lru_cache(maxsize=None)
def inputs(geo_name, kind, M):
    x, g_enc = R.positions(geo_name, kind, M), R.upstream(R.geometry(geo_name), M)
    return x, g_enc, x.to(DEV).contiguous(), g_enc.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def table_truth(geo_name, kind, M, calls):
    x, g_enc, _, _ = inputs(geo_name, kind, M)
    return R.grad_table(R.geometry(geo_name), x, g_enc, calls=calls)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def padded(rows, cols):
    return torch.full((rows + PAD, cols), SENTINEL, device=DEV)


def tail_intact(buf, rows):
    return bool((buf[rows:] == SENTINEL).all()) and not bool((buf[:rows] == SENTINEL).any())


@pytest.mark.parametrize("geo_name,kind,M", CASES, ids=IDS)
def test_forward(geo_name, kind, M):
    from nefes_amd import lib as L
    from nefes_amd import ops
    geo = R.geometry(geo_name)
    table, table64 = tables(geo_name)
    x, _, x_d, _ = inputs(geo_name, kind, M)
    enc = padded(M, 2 * geo.n_levels)
    L.check(L.load().nefes_hashgrid_fwd(ctypes.byref(geo.desc()), ptr(table), M, ptr(x_d), ptr(enc), ops._stream()), "nefes_hashgrid_fwd")
    want, budget = R.encode(geo, x, table64, want_budget=True)
    assert tail_intact(enc, M), "written past M, or an element below M left unwritten"
    r = R.ratio((enc[:M].cpu().double() - want).abs(), budget)
    P.record(f"hashgrid_fwd[{geo_name},{kind},{M}]", "worst error / budget", e_hip=r, e_ref=None, bound=1.0)
    assert r <= 1, r


@pytest.mark.parametrize("geo_name,kind,M", CASES, ids=IDS)
def test_backward_x(geo_name, kind, M):
    """N(0, 1) upstream, and an upstream that is zero on all but one level (the level cycles with M: a level whose term is dropped or
    doubled in the sixteen-lane reduction cannot hide behind the others)."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    geo = R.geometry(geo_name)
    table, table64 = tables(geo_name)
    x, g_enc, x_d, g_enc_d = inputs(geo_name, kind, M)
    one = M % geo.n_levels
    for name, ge, ge_d in (("all levels", g_enc, g_enc_d), (f"level {one} alone", R.upstream(geo, M, only_level=one), None)):
        ge_d = ge.to(DEV).contiguous() if ge_d is None else ge_d
        g_x = padded(M, 3)
        L.check(L.load().nefes_hashgrid_bwd_x(ctypes.byref(geo.desc()), ptr(table), M, ptr(x_d), ptr(ge_d), ptr(g_x), ops._stream()),
                "nefes_hashgrid_bwd_x")
        want, budget = R.grad_x(geo, x, table64, ge)
        assert tail_intact(g_x, M), "written past M, or an element below M left unwritten"
        r = R.ratio((g_x[:M].cpu().double() - want).abs(), budget)
        P.record(f"hashgrid_bwd_x[{geo_name},{kind},{M}]", "worst error / budget, " + ("all levels" if name == "all levels" else "one level alone"),
                 e_hip=r, e_ref=None, bound=1.0)
        assert r <= 1, (name, r)


@pytest.mark.parametrize("form", ["merged", "atomic"])
@pytest.mark.parametrize("geo_name,kind,M", CASES, ids=IDS)
def test_backward_table(geo_name, kind, M, form, monkeypatch):
    """Both scatter forms: every touched entry within its budget, every other entry (and PAD rows behind the table) exactly 0.0, the
    workspace's tail untouched, a second call into the same buffer within the budget of the doubled list of terms; on `repeats`, the
    entries of a repeated sample carry the whole run (the reference without the run's last sample is far outside the budget)."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    monkeypatch.setenv("NEFES_HG_TABLE_ATOMIC", "1" if form == "atomic" else "0")
    geo, lib = R.geometry(geo_name), L.load()
    x, g_enc, x_d, g_enc_d = inputs(geo_name, kind, M)
    d = geo.desc()
    ws_bytes = int(lib.nefes_hashgrid_bwd_table_workspace(ctypes.byref(d)))
    assert ws_bytes == 16 * geo.n_dense
    ws = torch.full((ws_bytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    g_table = torch.zeros(geo.total + PAD, 2, device=DEV)
    for calls in (1, 2):
        L.check(lib.nefes_hashgrid_bwd_table(ctypes.byref(d), M, ptr(x_d), ptr(g_enc_d), ptr(g_table), ptr(ws) if ws_bytes else None,
                                             ops._stream()), "nefes_hashgrid_bwd_table")
        rows, value, budget, n_terms = table_truth(geo_name, kind, M, calls)
        got = g_table[rows.to(DEV)]
        assert bool((ws[ws_bytes:] == 0xA5).all()), "the workspace's tail was written"
        assert int(g_table.count_nonzero()) == int(got.count_nonzero()), "an entry no sample touches is not 0.0"
        got = got.cpu().double()
        r = R.ratio((got - value).abs(), budget)
        P.record(f"hashgrid_bwd_table[{geo_name},{kind},{M},{form}]", f"worst error / budget, call {calls}", e_hip=r, e_ref=None, bound=1.0)
        assert r <= 1, (calls, r)
        if kind == "repeats" and calls == 1:
            runs = [len(list(grp)) for _, grp in itertools.groupby(map(tuple, x.tolist()))]
            assert int(n_terms.max()) >= max(runs)                                    # some entry collects a whole run
            rows_m, value_m, _, _ = R.grad_table(geo, x, g_enc, "drop_run_tail")
            short = torch.zeros(geo.total, 2, dtype=torch.float64).index_put_((rows_m,), value_m)[rows]
            assert R.ratio((got - short).abs(), budget) > 10


def test_fused_field_kernels_at_a_second_geometry():
    """tests/test_gpu_cam.py::test_fused_hashgrid_kernels_equal_the_separate_launches, its assertions repeated at 16 levels, 2^14 entries,
    8 -> 512, bound 4, with about a third of the samples outside the bound on both sides (negative cells included): the field kernels'
    prologue / epilogue call the same device functions as the stand-alone kernels, at the same corner order."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from tests.branch import rel, tapped
    from tests.test_gpu_cam import C as C_FEAT
    from tests.test_gpu_cam import TABLE_GAIN, nets
    BOUND = 4.0
    coarse, fine = nets()
    grid = ops.HashGrid(BOUND, n_levels=16, log2_hashmap_size=14, base_resolution=8, max_resolution=512)
    grid.table.mul_(TABLE_GAIN)                                      # O(0.3) features, so that the MLP sees the position
    g = torch.Generator().manual_seed(5)
    N, S = 37, 75                                                   # ragged: 2 775 samples, a partial last tile
    o_c = (torch.rand(N, 3, generator=g) - .5) * 2.0 * BOUND
    d_c = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    v_c = d_c.clone()
    d_c = d_c * (0.5 + torch.rand(N, 1, generator=g))
    z_c = torch.sort(torch.rand(N, S, generator=g) * BOUND, -1)[0]
    pts = o_c[:, None, :] + d_c[:, None, :] * z_c[..., None]
    outside = float((pts.abs() > BOUND).any(-1).float().mean())
    assert 0.25 <= outside <= 0.45 and float(pts.abs().max()) <= 4 * BOUND, outside
    assert float((pts < -BOUND).any(-1).float().mean()) > 0.08 and float((pts > BOUND).any(-1).float().mean()) > 0.08
    o, d, v = o_c.to(DEV).requires_grad_(), d_c.to(DEV).requires_grad_(), v_c.to(DEV).requires_grad_()
    z = z_c.to(DEV)
    G = torch.randn(N, 3 + C_FEAT + 6, S, generator=g).to(DEV)
    pk_c, pk_f = coarse.packed(), fine.packed()
    assert ops.hashgrid_fused_ok(pk_f, grid) and ops.hashgrid_fused_ok(pk_c, grid)

    def separate(pk, mode):
        p = o[:, None, :] + d[:, None, :] * z[..., None]
        return ops.FieldFromEncoding.apply(grid(p), v, pk, mode)

    ops.TIMERS = timers = {}
    try:
        with tapped() as tap:
            sig_f = ops.FieldFromRaysHashGrid.apply(o, d, v, z, pk_c, L.FIELD_SIGMA, grid)
            raw_f = ops.FieldFromRaysHashGrid.apply(o, d, v, z, pk_f, L.FIELD_FULL, grid)
            gf = torch.autograd.grad((raw_f * G).sum(), (o, d, v))
            sig_s = separate(pk_c, L.FIELD_SIGMA)
            raw_s = separate(pk_f, L.FIELD_FULL)
            gs = torch.autograd.grad((raw_s * G).sum(), (o, d, v))
    finally:
        ops.TIMERS = None
    assert {"field_fwd[sigma,h3,hashgrid]", "field_fwd[full,h3,hashgrid]", "field_bwd[h3,hashgrid]", "hashgrid_fwd", "hashgrid_bwd_x"} <= set(timers), sorted(timers)
    assert torch.equal(sig_f, sig_s) and torch.equal(raw_f, raw_s)
    assert float(raw_f.std()) > 0
    m_f, m_s = tap["masks"][0][0], tap["masks"][1][0]
    assert torch.equal(m_f, m_s)                                    # same ReLU-mask words
    for name, a, b in zip(("d rays_o", "d rays_d", "d viewdirs"), gf, gs):
        e = rel(a, b)
        P.record("hashgrid_fused[16 levels, 2^14, 8->512, bound 4]", f"{name}: fused kernels vs separate launches", direct=e, bound=1e-5)
        assert e < 1e-5, (name, e)
