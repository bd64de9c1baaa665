"""tests/hashgrid_ref.py, the yardstick of tests/test_gpu_hashgrid.py, checked on the CPU: the float64 reference against statements it did
not compute itself (oracle/hashgrid_ref.py at the one geometry that file knows, gradcheck, autograd through the table, the library's own
geometry queries -- the library loads without a GPU), every input set against the condition it is drawn under, the budgets against an
fp32 restatement of the kernels' arithmetic (inside 0.75 x budget: the budgets are not too tight to mean something), and against ten
wrong references (outside 10 x budget: they are not too loose to see a fault)."""
import ctypes as C
import functools

import pytest
import torch

from oracle import hashgrid_ref as HG
from tests import hashgrid_ref as R

GEOS = list(R.GEOMETRIES)
E_BADARG, E_UNSUPPORTED = -1, -2          # include/nefes_hip.h NEFES_E_BADARG, NEFES_E_UNSUPPORTED
M_CPU = 1000


@functools.lru_cache(maxsize=None)
def case(geo_name, kind, M=M_CPU):
    """positions, table, upstream and the unmutated float64 results, computed once and shared (never modified)"""
    geo = R.geometry(geo_name)
    x, table, g_enc = R.positions(geo_name, kind, M), table_of(geo_name), R.upstream(geo, M)
    enc, b_enc = R.encode(geo, x, table, want_budget=True)
    g_x, b_x = R.grad_x(geo, x, table, g_enc)
    return dict(x=x, table=table, g_enc=g_enc, enc=enc, b_enc=b_enc, g_x=g_x, b_x=b_x, g_table=R.grad_table(geo, x, g_enc))


@functools.lru_cache(maxsize=None)
def table_of(geo_name):
    return R.make_table(R.geometry(geo_name))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_default_geometry_equals_the_oracle_inside_the_bound():
    """Two independent statements of the same encoding, both float64, where both are defined."""
    geo = R.geometry("default")
    assert geo.total == HG.table_entries() and geo.n_dense == sum(e for _, _, e, _, h in HG.level_geometry()[0] if not h)
    x, table = R.positions("default", "inside", 500), table_of("default").double()
    got, want = R.encode(geo, x, table), HG.encode(x.double(), table, geo.bound)
    assert float((got - want).abs().max()) <= 1e-13


def test_x_gradient_passes_gradcheck_and_table_gradient_is_autograd():
    geo = R.geometry("three")
    x = R.positions("three", "both_sides", 9)
    table, g_enc = table_of("three").double(), R.upstream(geo, 9).double()
    assert torch.autograd.gradcheck(lambda p: R.encode(geo, p, table), (x.double().requires_grad_(),), eps=1e-7, atol=1e-6)
    p = x.double().requires_grad_()
    t = table.clone().requires_grad_()
    gx_want, gt_want = torch.autograd.grad((R.encode(geo, p, t) * g_enc).sum(), (p, t))
    gx, _ = R.grad_x(geo, x, table, g_enc)
    assert float((gx - gx_want).abs().max()) <= 1e-12
    rows, value, _, n_terms = R.grad_table(geo, x, g_enc)
    full = torch.zeros_like(table).index_put_((rows,), value)
    assert float((full - gt_want).abs().max()) <= 1e-13 and int(n_terms.sum()) == 9 * geo.n_levels * 8
    _, twice, _, n2 = R.grad_table(geo, x, g_enc, calls=2)
    assert torch.equal(twice, 2 * value) and torch.equal(n2, 2 * n_terms)


def test_negative_cells_wrap_in_uint32():
    """The contract below -bound, worked by hand at one dense level: cell (-1, 0, 0) at res 3, 32 entries -> corner 0 is row
    (2^32 - 1) mod 32 = 31, not the signed index's (-1) mod 32 = 31 ... which agrees only because 32 divides 2^32; at 40 entries they part."""
    import numpy as np
    cell = np.array([[-1, 0, 0]], np.int64)
    for entries in (32, 40):
        L = dict(res=3, entries=entries, offset=0, hashed=False)
        assert R.level_index(L, cell)[0, 0] == (2 ** 32 - 1) % entries
        assert R.level_index(L, cell, "no_wrap")[0, 0] == entries - 1
        assert R.level_index(L, cell)[0, 1] == 0                                                       # corner (+1, 0, 0): back at cell 0
    Lh = dict(res=99, entries=1 << 8, offset=16, hashed=True)
    want = ((2 ** 32 - 1) ^ (5 * 2654435761 % 2 ** 32) ^ ((2 ** 32 - 7) * 805459861 % 2 ** 32)) % 256
    assert R.level_index(Lh, np.array([[-1, 5, -7]], np.int64))[0, 0] == 16 + want


# ---- geometry against the library ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo_name", GEOS)
def test_geometry_equals_the_librarys(geo_name):
    from nefes_amd import lib as L
    geo, lib = R.geometry(geo_name), L.load()
    d = geo.desc()
    assert lib.nefes_hashgrid_table_entries(C.byref(d)) == geo.total
    assert lib.nefes_hashgrid_bwd_table_workspace(C.byref(d)) == 16 * geo.n_dense
    dense = [not lv["hashed"] for lv in geo.levels]
    assert dense == sorted(dense, reverse=True)                          # the dense levels are a prefix


def test_geometries_reach_what_they_are_there_for():
    n_dense_levels = {n: sum(not lv["hashed"] for lv in R.geometry(n).levels) for n in GEOS}
    assert n_dense_levels == {"default": 5, "small": 2, "all_dense": 16, "all_hashed": 0, "three": n_dense_levels["three"], "one": 1}
    assert R.geometry("all_hashed").n_dense == 0 and R.geometry("all_dense").n_dense == R.geometry("all_dense").total
    assert R.geometry("one").levels[0]["scale"] == R.GEOMETRIES["one"][2] - 1
    # a dense level whose res^3 is no multiple of 8 (the round-up shifts every later level)
    assert all(any(not lv["hashed"] and lv["res"] % 2 for lv in R.geometry(n).levels[:-1]) for n in ("default", "all_dense", "three"))


def test_library_refuses_what_it_does_not_serve():
    from nefes_amd import lib as L
    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)                                         # never dereferenced: every call below returns before a launch
    good = R.geometry("small")

    def desc(**kw):
        d = good.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def calls(d, M=4):
        """only ever called with a refused description or a refused M: nothing is launched"""
        return (lib.nefes_hashgrid_fwd(C.byref(d), p, M, p, p, None), lib.nefes_hashgrid_bwd_x(C.byref(d), p, M, p, p, p, None),
                lib.nefes_hashgrid_bwd_table(C.byref(d), M, p, p, p, p, None))

    bad = [dict(n_levels=0), dict(n_levels=17), dict(n_features=1), dict(n_features=4), dict(log2_hashmap_size=0),
           dict(log2_hashmap_size=25), dict(bound=0.0), dict(bound=-1.0), dict(bound=float("nan"))]
    for kw in bad:
        d = desc(**kw)
        assert lib.nefes_hashgrid_table_entries(C.byref(d)) == 0 and lib.nefes_hashgrid_bwd_table_workspace(C.byref(d)) == 0, kw
        assert calls(d) == (E_UNSUPPORTED,) * 3, kw
    assert lib.nefes_hashgrid_table_entries(None) == 0 and lib.nefes_hashgrid_bwd_table_workspace(None) == 0
    for M in (0, -1):
        assert calls(good.desc(), M=M) == (E_BADARG,) * 3, M
    # one null pointer at a time, and only at the entry point that takes it: a call with every argument in place would launch
    d = good.desc()
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert lib.nefes_hashgrid_fwd(C.byref(d), a[0], 4, a[1], a[2], None) == E_BADARG, i
    for i in range(4):
        a = [p, p, p, p]
        a[i] = None
        assert lib.nefes_hashgrid_bwd_x(C.byref(d), a[0], 4, a[1], a[2], a[3], None) == E_BADARG, i
    for i in range(4):                                                  # `small` has dense levels: the workspace is required
        a = [p, p, p, p]
        a[i] = None
        assert lib.nefes_hashgrid_bwd_table(C.byref(d), 4, a[0], a[1], a[2], a[3], None) == E_BADARG, i
    assert lib.nefes_hashgrid_fwd(None, p, 4, p, p, None) == E_UNSUPPORTED


def test_hashgrid_of_one_level():
    """ops.HashGrid(n_levels=1) is supported: one level of scale base_resolution - 1 (it used to divide by zero before asking the library)."""
    from nefes_amd import ops
    geo = R.geometry("one")
    n_levels, log2, base, max_res, bound = R.GEOMETRIES["one"]
    grid = ops.HashGrid(bound, n_levels=1, log2_hashmap_size=log2, base_resolution=base, max_resolution=max_res, device="cpu")
    assert grid.n_out == 2 and tuple(grid.table.shape) == (geo.total, 2) and grid.desc.per_level_scale == geo.per_level_scale == 1.0
    with pytest.raises(RuntimeError, match="unsupported hash-grid"):
        ops.HashGrid(bound, n_levels=0, device="cpu")
    with pytest.raises(RuntimeError, match="unsupported hash-grid"):
        ops.HashGrid(bound, n_levels=17, device="cpu")


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.SETS)
@pytest.mark.parametrize("geo_name", GEOS)
def test_inputs(geo_name, kind):
    geo = R.geometry(geo_name)
    worst = 0.
    for M in R.MS:
        x, dr = R.positions(geo_name, kind, M, want_draw=True)
        assert x.dtype == torch.float32 and x.shape == (M, 3) and float(x.abs().max()) <= 4 * geo.bound
        assert not bool(R.ambiguous(geo, x).any())
        assert torch.equal(x, R.positions(geo_name, kind, M))                                          # seeded
        if dr.drawn >= 500:
            worst = max(worst, dr.discarded)
    print(f"inputs {geo_name} {kind}: worst share discarded {worst:.4f}")
    assert worst <= 0.02
    x = R.positions(geo_name, kind, M_CPU)
    below = float((x < -geo.bound).any(1).float().mean())
    if kind == "inside":
        assert float(x.abs().max()) <= 0.999 * geo.bound
    elif kind == "both_sides":
        assert 0.5 <= below <= 0.7 and bool((x > geo.bound).any())
    elif kind == "rays":
        inside = (x.abs() <= geo.bound).all(1)
        assert below > 0.05 and bool((x > geo.bound).any()) and 0.2 < float(inside.float().mean()) < 0.9
    else:
        runs, m = [], 0
        while m < M_CPU:
            n = 1
            while m + n < M_CPU and torch.equal(x[m + n], x[m]):
                n += 1
            runs.append(n)
            m += n
        assert runs[:10] == list(R.REPEATS) * 2 and below > 0.2
    if kind in ("rays", "repeats") and geo_name != "all_hashed":
        # consecutive samples share a coarse-level entry: the merged kernel's runs exist
        rows = R.level_terms(geo, 0, x)["idx"][:, 0]
        assert int((rows[1:] == rows[:-1]).sum()) >= M_CPU // 4


# ---- the budgets mean something: the kernels' arithmetic in fp32 stays inside 0.75 x budget ------------------------------------------
@pytest.mark.parametrize("kind", R.SETS)
@pytest.mark.parametrize("geo_name", GEOS)
def test_fp32_restatement_stays_inside_the_budgets(geo_name, kind):
    geo, c = R.geometry(geo_name), case(geo_name, kind)
    rows, value, budget, _ = c["g_table"]
    for fma in (False, True):
        enc, g_x, g_table = R.fp32_restatement(geo, c["x"], c["table"], c["g_enc"], fma)
        r = (R.ratio((enc.double() - c["enc"]).abs(), c["b_enc"]), R.ratio((g_x.double() - c["g_x"]).abs(), c["b_x"]),
             R.ratio((g_table[rows].double() - value).abs(), budget))
        print(f"fp32 restatement {geo_name} {kind} fma={fma}: error / budget forward {r[0]:.3f}, x-gradient {r[1]:.3f}, table gradient {r[2]:.3f}")
        assert max(r) <= 0.75, r
        untouched = torch.ones(geo.total, dtype=torch.bool)
        untouched[rows] = False
        assert not bool(g_table[untouched].any())


# ---- the tests have power: every wrong reference is more than 10 x budget away somewhere -----------------------------------------------
def applies(mutation, geo_name, kind):
    geo = R.geometry(geo_name)
    if mutation == "no_wrap":                       # differs only for negative cells at a dense level whose entry count does not divide 2^32
        return kind in R.NEGATIVE_SETS and any(not lv["hashed"] and lv["entries"] & (lv["entries"] - 1) for lv in geo.levels)
    if mutation == "primes":
        return geo.n_dense < geo.total
    if mutation == "offsets":
        return geo.n_levels > 1
    if mutation == "no_round8":                     # a dense level with res^3 no multiple of 8 that is followed by another level
        return any(not lv["hashed"] and lv["res"] % 2 for lv in geo.levels[:-1])
    return True


MUTATIONS = ["no_wrap", "swap_xz", "primes", "offsets", "flip_w", "scale_no_minus1", "pos_no_half", "drop_s", "drop_run_tail", "no_round8"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutation_is_outside_ten_budgets(mutation):
    seen = 0
    for geo_name in GEOS:
        geo = R.geometry(geo_name)
        for kind in R.SETS:
            if not applies(mutation, geo_name, kind):
                continue
            c = case(geo_name, kind)
            if mutation == "drop_s":
                got, _ = R.grad_x(geo, c["x"], c["table"], c["g_enc"], mutation)
                r = {"x-gradient": R.ratio((got - c["g_x"]).abs(), c["b_x"])}
            elif mutation == "drop_run_tail":
                rows, value, budget, _ = c["g_table"]
                rows_m, value_m, _, _ = R.grad_table(geo, c["x"], c["g_enc"], mutation)
                full = torch.zeros(geo.total, 2, dtype=torch.float64).index_put_((rows_m,), value_m)
                r = {"table gradient": R.ratio((full[rows] - value).abs(), budget)}
            else:
                # the forward, and with it what the two backward tests see of the same fault
                enc = R.encode(geo, c["x"], c["table"], mutation)
                got, _ = R.grad_x(geo, c["x"], c["table"], c["g_enc"], mutation)
                rows, value, budget, _ = c["g_table"]
                rows_m, value_m, _, _ = R.grad_table(geo, c["x"], c["g_enc"], mutation)
                full = torch.zeros(geo.total, 2, dtype=torch.float64).index_put_((rows_m,), value_m)
                r = {"forward": R.ratio((enc - c["enc"]).abs(), c["b_enc"]), "x-gradient": R.ratio((got - c["g_x"]).abs(), c["b_x"]),
                     "table gradient": R.ratio((full[rows] - value).abs(), budget)}
            print(f"mutation {mutation} {geo_name} {kind}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
            assert min(r.values()) > 10, (mutation, geo_name, kind, r)
            seen += 1
    assert seen >= 4
