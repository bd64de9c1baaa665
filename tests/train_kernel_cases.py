"""Cases that drive the training-backward kernels of nefes_amd/csrc/train.hip directly (ctypes, plain buffers in the layout of
csrc/layout.h) -- shared by tests/test_gpu_train_kernels.py, which runs them in its own process, and by a child process it starts
once with the other setting of NEFES_TRAIN_DW (the library reads that variable once per process):

    python tests/train_kernel_cases.py OUT.json      every weight-gradient case on the kernel this process selects -> OUT.json

Every function returns plain numbers / strings (JSON), never asserts on a kernel's result: the test asserts.  A launch that returns an
error code is reported in the outcome and the next configuration runs (nothing was launched); a HIP error raised at the synchronize
is not caught here: it ends the child process, and in the test process the test that ran the case remembers it."""
import ctypes as C
import functools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.train_layout import from_device, to_device  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SPARE = 8192                                     # floats behind every output buffer that must stay untouched

# (NTO, NTI) instance of train_dw_impl's table -> the (ot, it) = (n_out / 32, n_in / 32) shapes that run it on the bf16 kernel:
# asymmetric, two or more output blocks and two or more input blocks of the instance where its selection rule allows
SHAPES = [((4, 4), (8, 4)), ((4, 4), (4, 8)), ((5, 2), (5, 2)), ((4, 2), (8, 2)), ((2, 4), (6, 8)), ((2, 2), (6, 2)), ((2, 2), (2, 6)),
          ((2, 1), (4, 1)), ((2, 1), (2, 3)), ((1, 4), (5, 4)), ((1, 4), (3, 8)), ((1, 2), (3, 2)), ((1, 2), (1, 6)), ((1, 1), (3, 3)),
          ((1, 1), (1, 5))]
KERNELS = ("x6", "f32")                          # train_dw_x6_kernel (default) / train_dw_kernel (NEFES_TRAIN_DW=f32)


def this_kernel():
    return "f32" if os.environ.get("NEFES_TRAIN_DW", "")[:1] == "f" else "x6"


def instance(ot, it, kernel):
    """(NTO, NTI) that train_dw_impl (csrc/train.hip) launches for an ot x it-tile product: the three big blocks are the bf16
    kernel's alone.  A copy of that table made by reading it, as train._dw_grid is: the instance in a case's id is the one the case
    is INTENDED for, nothing observes at run time which kernel object served a launch (no test inspects compiled code).  With
    NEFES_TRAIN_DW=f32 the table never picks <4,4>, <5,2> or <4,2>, so the fp32 kernels of those three have no caller and no case."""
    if kernel == "x6":
        if ot % 4 == 0 and it % 4 == 0:
            return 4, 4
        if ot == 5 and it == 2:
            return 5, 2
        if ot % 4 == 0 and it == 2:
            return 4, 2
    return (2 if ot % 2 == 0 else 1), (4 if it % 4 == 0 else (2 if it % 2 == 0 else 1))


def dw_case_id(ot, it, kernel, bias=None, relu=None):
    nto, nti = instance(ot, it, kernel)
    s = f"i{nto}{nti}-{ot}x{it}"
    if bias is not None:
        s += "-" + ("dw_bias" if bias else "dw")
    if relu is not None:
        s += f"-relu{relu}"
    return s


def _dev_buf(logical):
    """Device copy, in device order, of a [T, rows, 128] buffer given in (row, sample) order, with one spare tile of NaN behind it."""
    T, rows, _ = logical.shape
    flat = torch.full(((T + 1) * rows * 128,), NAN, device=DEV)
    flat[:T * rows * 128] = to_device(logical).reshape(-1).to(DEV)
    return flat


def _placed(T, rows, *blocks):
    """[T, rows, 128] of NaN with every (row0, values [T, n, 128]) block put at its rows: a kernel that reads any other row shows."""
    buf = torch.full((T, rows, 128), NAN)
    for row0, v in blocks:
        buf[:, row0:row0 + v.shape[1]] = v.float()
    return buf


def _dw_call(lib, bias, T, rows, bg, g0, op, bx, x0, ip, relu, splits, stride, part_ptr):
    if bias:
        return lib.nefes_train_dw_bias(T, rows, bg.data_ptr(), g0, op, bx.data_ptr(), x0, ip, relu, splits, stride, part_ptr, None)
    return lib.nefes_train_dw(T, rows, bg.data_ptr(), g0, op, bx.data_ptr(), x0, ip, relu, splits, part_ptr, None)


def _shares(T, splits):
    return [(T * sp // splits, T * (sp + 1) // splits) for sp in range(splits)]


# ---- dW, exact: integer operands -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dw_ints(ot, it):
    g = torch.Generator().manual_seed(1000 * ot + it)
    return torch.randint(-4, 5, (5, 32 * ot, 128), generator=g), torch.randint(-4, 5, (5, 32 * it, 128), generator=g)


@functools.lru_cache(maxsize=4)
def _dw_tile_products(ot, it, relu):
    """per tile: G f(X)^T [5, op, ip] and the row sums of G [5, op], int64."""
    G, X = _dw_ints(ot, it)
    return torch.einsum("tos,tis->toi", G, X.clamp_min(0) if relu else X), G.sum(-1)


def dw_configs(ot, it, bias):
    """(tiles, shares): all in one, 5 in 3 (uneven), one tile per share (the prefetch's last step ends a share every tile).  Row
    offsets zero and non-zero, `rows` exact and larger than the rows in use, G and X in two buffers or in one (gbuf == xbuf), the
    partials back to back or (nefes_train_dw_bias) as one product among others in a wide buffer."""
    op, ip = 32 * ot, 32 * it
    wide = (1056, 4160) if bias else None                   # columns of the products before / behind this one
    return [dict(name="3 tiles, 1 share", T=3, splits=1, g0=0, x0=0, rows=max(op, ip), same=False, wide=None),
            dict(name="5 tiles, 3 shares, one buffer, wide", T=5, splits=3, g0=32, x0=op + 96, rows=op + ip + 160, same=True, wide=wide),
            dict(name="5 tiles, 5 shares, X below G", T=5, splits=5, g0=ip + 64, x0=32, rows=op + ip + 96, same=False, wide=None),
            dict(name="3 tiles, 3 shares, one buffer", T=3, splits=3, g0=ip, x0=0, rows=op + ip, same=True, wide=wide)]


def run_dw_exact(lib, ot, it, bias, relu):
    op, ip = 32 * ot, 32 * it
    G, X = _dw_ints(ot, it)
    prod, rowsum = _dw_tile_products(ot, it, relu)
    largest = int(max(prod.abs().sum(0).max(), rowsum.abs().sum(0).max()))          # bounds every share's every partial sum
    fails = []
    for cfg in dw_configs(ot, it, bias):
        T, splits, g0, x0, rows = cfg["T"], cfg["splits"], cfg["g0"], cfg["x0"], cfg["rows"]
        if cfg["same"]:
            bg = bx = _dev_buf(_placed(T, rows, (g0, G[:T]), (x0, X[:T])))
        else:
            bg, bx = _dev_buf(_placed(T, rows, (g0, G[:T]))), _dev_buf(_placed(T, rows, (x0, X[:T])))
        ld = ip + (1 if bias else 0)
        n = op * ld
        c0, c1 = cfg["wide"] or (0, 0)
        stride = c0 + n + c1
        part = torch.full((splits * stride + SPARE,), NAN, device=DEV)
        rc = _dw_call(lib, bias, T, rows, bg, g0, op, bx, x0, ip, relu, splits, stride if cfg["wide"] else 0, part.data_ptr() + 4 * c0)
        torch.cuda.synchronize()
        if rc != 0:
            fails.append(f"{cfg['name']}: returned {rc}")
            continue
        got = part.cpu()
        want = torch.full_like(got, NAN)
        for sp, (lo, hi) in enumerate(_shares(T, splits)):
            e = prod[lo:hi].sum(0)
            if bias:
                e = torch.cat([e, rowsum[lo:hi].sum(0)[:, None]], 1)
            want[sp * stride + c0:sp * stride + c0 + n] = e.float().reshape(-1)
        if not torch.equal(got.isnan(), want.isnan()):
            extra, missing = int((want.isnan() & ~got.isnan()).sum()), int((got.isnan() & ~want.isnan()).sum())
            fails.append(f"{cfg['name']}: {extra} elements written outside the product's {op} x {ld} per share, {missing} of them not written")
        for sp in range(splits):
            a, b = got[sp * stride + c0:sp * stride + c0 + n].view(op, ld), want[sp * stride + c0:sp * stride + c0 + n].view(op, ld)
            if not torch.equal(a, b):
                bad = (a != b).nonzero()
                o, i = (int(v) for v in bad[0])
                fails.append(f"{cfg['name']}: share {sp}: {len(bad)} of {n} differ, first at ({o}, {i}): {float(a[o, i])} != {float(b[o, i])}"
                             f"; bias column wrong in {int((a[:, ip:] != b[:, ip:]).sum())} rows")
    return {"ok": not fails, "fails": fails, "largest": largest}


# ---- dW, split completeness: operands with a middle and a low bf16 part ----------------------------------------------------------
def run_dw_completeness(lib, ot, it):
    """Every operand +-2^a (1 + 2^-8 + 2^-16), a per (tile, row), one sign per row; one tile per share (K = 128).  -> the worst
    |hip - exact| / |exact| over both settings of x_relu, and whether an exactly-zero product came back non-zero."""
    op, ip = 32 * ot, 32 * it
    T = splits = 2
    g = torch.Generator().manual_seed(77 * ot + it)
    c = 1. + 2. ** -8 + 2. ** -16

    def operand(n):
        a = torch.randint(-6, 7, (T, n, 1), generator=g).double()
        sign = (torch.randint(0, 2, (1, n, 1), generator=g) * 2 - 1).double()
        return (sign * 2. ** a * c).expand(T, n, 128).contiguous()
    G, X = operand(op), operand(ip)
    assert torch.equal(G.float().double(), G) and torch.equal(X.float().double(), X)
    rows = max(op, ip)
    bg, bx = _dev_buf(_placed(T, rows, (0, G))), _dev_buf(_placed(T, rows, (0, X)))
    worst, nonzero = 0., 0
    for relu in (0, 1):
        exact = torch.cat([torch.einsum("tos,tis->toi", G, X.clamp_min(0) if relu else X), G.sum(-1, keepdim=True)], 2)   # exact in float64
        part = torch.full((splits * op * (ip + 1) + SPARE,), NAN, device=DEV)
        rc = lib.nefes_train_dw_bias(T, rows, bg.data_ptr(), 0, op, bx.data_ptr(), 0, ip, relu, splits, 0, part.data_ptr(), None)
        torch.cuda.synchronize()
        if rc != 0:
            return {"rc": rc, "worst": NAN, "nonzero": -1}
        got = part[:splits * op * (ip + 1)].cpu().double().view(splits, op, ip + 1)
        zero = exact == 0
        nonzero += int((got[zero] != 0).sum())
        worst = max(worst, float(((got - exact).abs()[~zero] / exact.abs()[~zero]).max()))
    return {"rc": 0, "worst": worst, "nonzero": nonzero}


# ---- dW, general floats ----------------------------------------------------------------------------------------------------------
GENERAL_SHAPES = [(8, 4), (5, 2), (2, 6), (3, 3)]
GENERAL_K = 256


def run_dw_general(lib, ot, it):
    """Operands |N(0,1)| 2^U{-6..6}, two tiles per share.  -> e_hip, e_ref (torch fp32 matmul on the host) against float64, both
    normalised element by element with sum_s |g| |x| (the bias column: sum_s |g|)."""
    op, ip = 32 * ot, 32 * it
    T, splits = 4, 2
    g = torch.Generator().manual_seed(5 * ot + it)
    rnd = lambda n: (torch.randn(T, n, 128, generator=g).abs() * 2. ** torch.randint(-6, 7, (T, n, 128), generator=g).float())
    G, X = rnd(op), rnd(ip)
    rows = max(op, ip)
    bg, bx = _dev_buf(_placed(T, rows, (0, G))), _dev_buf(_placed(T, rows, (0, X)))
    part = torch.full((splits * op * (ip + 1) + SPARE,), NAN, device=DEV)
    rc = lib.nefes_train_dw_bias(T, rows, bg.data_ptr(), 0, op, bx.data_ptr(), 0, ip, 0, splits, 0, part.data_ptr(), None)
    torch.cuda.synchronize()
    if rc != 0:
        return {"rc": rc}
    got = part[:splits * op * (ip + 1)].cpu().double().view(splits, op, ip + 1)
    e_hip = e_ref = 0.
    for sp, (lo, hi) in enumerate(_shares(T, splits)):
        g32 = G[lo:hi].permute(1, 0, 2).reshape(op, -1)                     # [op, K]
        x32 = X[lo:hi].permute(1, 0, 2).reshape(ip, -1)
        assert g32.shape[1] == GENERAL_K
        g64, x64 = g32.double(), x32.double()
        truth = torch.cat([g64 @ x64.t(), g64.sum(1, keepdim=True)], 1)
        scale = torch.cat([g64.abs() @ x64.abs().t(), g64.abs().sum(1, keepdim=True)], 1)
        ref = torch.cat([g32 @ x32.t(), g32.sum(1, keepdim=True)], 1).double()
        e_hip = max(e_hip, float(((got[sp] - truth).abs() / scale).max()))
        e_ref = max(e_ref, float(((ref - truth).abs() / scale).max()))
    return {"rc": 0, "e_hip": e_hip, "e_ref": e_ref}


def dw_exact_cases():
    return [(ot, it, bias, relu) for _, (ot, it) in SHAPES for relu in (0, 1) for bias in (0, 1)]


def run_all_dw(lib, kernel):
    """Every weight-gradient case, keyed like the test ids."""
    out = {}
    for ot, it, bias, relu in dw_exact_cases():
        out["exact/" + dw_case_id(ot, it, kernel, bias, relu)] = run_dw_exact(lib, ot, it, bias, relu)
    for _, (ot, it) in SHAPES:
        out["completeness/" + dw_case_id(ot, it, kernel)] = run_dw_completeness(lib, ot, it)
    for ot, it in GENERAL_SHAPES:
        out["general/" + dw_case_id(ot, it, kernel)] = run_dw_general(lib, ot, it)
    return out


# ---- dX, exact -------------------------------------------------------------------------------------------------------------------
def run_dx_exact(lib, n_in, n_out):
    """G, Wt integers in [-2, 2]; every flag combination at two placements: two buffers with zero offsets, and one buffer
    (dacts_out == dacts_in) with non-zero offsets that are no multiples of 32 and disjoint row ranges.  The destination holds
    integers (so that accumulate stays exact) and NaN outside the block; every row outside the block must keep its bits."""
    T, ldw = 3, n_out + 4
    g = torch.Generator().manual_seed(3 * n_in + n_out)
    G = torch.randint(-2, 3, (T, n_out, 128), generator=g)
    wt = torch.full((n_in, ldw), NAN)                                              # the padding columns are never read
    Wt = torch.randint(-2, 3, (n_in, n_out), generator=g)
    wt[:, :n_out] = Wt.float()
    prev = torch.randint(-8, 9, (T, n_in, 128), generator=g)
    act = torch.randint(-2, 3, (T, n_in, 128), generator=g).float()                # two fifths positive, a fifth exact zeros
    act[:, ::7, ::5] = -0.0
    prod = torch.einsum("io,tos->tis", Wt, G)
    assert int(prod.abs().max()) + 8 < 2 ** 24
    wt_d = wt.to(DEV)
    fails = []
    pad = lambda n: (n + 31) // 32 * 32
    for same, g0, d0, rows in ((False, 0, 0, pad(max(n_in, n_out))), (True, 40, 40 + n_out + 12, pad(52 + n_out + n_in) + 32)):
        for accumulate in (0, 1):
            for mask in (0, 1):
                name = f"{'one buffer' if same else 'two buffers'} accumulate={accumulate} mask={mask}"
                before = _placed(T, rows, (d0, prev), *(((g0, G),) if same else ()))
                b_out = _dev_buf(before)
                b_in = b_out if same else _dev_buf(_placed(T, rows, (g0, G)))
                b_act = _dev_buf(_placed(T, rows, (d0, act)))
                rc = lib.nefes_train_dx(T, rows, b_in.data_ptr(), g0, n_out, wt_d.data_ptr(), ldw, n_in, b_act.data_ptr() if mask else None,
                                        d0, accumulate, mask, b_out.data_ptr(), None)
                torch.cuda.synchronize()
                if rc != 0:
                    fails.append(f"{name}: returned {rc}")
                    continue
                flat = b_out.cpu()
                got = from_device(flat[:T * rows * 128].view(T, rows, 128))
                v = prod + prev if accumulate else prod
                if mask:
                    v = torch.where(act > 0, v, torch.zeros_like(v))
                want = before.clone()
                want[:, d0:d0 + n_in] = v.float()
                if not torch.equal(got[:, d0:d0 + n_in], want[:, d0:d0 + n_in]):
                    bad = (got[:, d0:d0 + n_in] != want[:, d0:d0 + n_in]).nonzero()
                    t, i, s = (int(x) for x in bad[0])
                    fails.append(f"{name}: {len(bad)} elements differ, first at tile {t} row {i} sample {s}: "
                                 f"{float(got[t, d0 + i, s])} != {float(want[t, d0 + i, s])}")
                outside = torch.ones(rows, dtype=torch.bool)
                outside[d0:d0 + n_in] = False
                if not torch.equal(got[:, outside].view(torch.int32), want[:, outside].view(torch.int32)):
                    fails.append(f"{name}: rows outside the destination block changed")
                if not flat[T * rows * 128:].isnan().all():
                    fails.append(f"{name}: written behind the last tile")
    return {"ok": not fails, "fails": fails}


def main(out_path):
    from nefes_amd import lib as L
    res = run_all_dw(L.load(), this_kernel())
    with open(out_path, "w") as f:
        json.dump({"kernel": this_kernel(), "cases": res}, f)


if __name__ == "__main__":
    main(sys.argv[1])
