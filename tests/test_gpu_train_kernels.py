"""The training-backward kernels of csrc/train.hip called directly (lib.load() / ctypes) on plain buffers in the layout of
csrc/layout.h, each against an exact or float64 expectation of the same operation.

    dW, exact         integer operands: every product and every partial sum is exact in fp32 and in the top bf16 part, so the
                      expected partials are an int64 matrix product and the comparison is torch.equal, in any summation order;
                      every (NTO, NTI) instance of train_dw_impl's table, both kernels, both entry points
    dW, completeness  operands with a middle and a low bf16 part: the six kept cross terms of the three-way split, derived bound
    dW, general       random floats against float64, beside torch's fp32 matmul
    dX, exact         integer operands, every flag
    head_grad         against float64

The weight-gradient kernel is chosen by NEFES_TRAIN_DW, read once per process: the cases of the kernel this process does not select
run in ONE child process (tests/train_kernel_cases.py) that is started the first time one of them is asked for, and never again:
its outcome, a failure included, serves every later test."""
import contextlib
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import parity_log as P
from tests import train_kernel_cases as K
from tests.train_layout import from_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_child = {}


def _other_kernel_results(tmp_path_factory):
    """The child's results {case id: outcome} on the kernel this process does not run.  The child is started ONCE per test process
    whatever becomes of it: if it fails, faults or runs out of time, that outcome is kept and every test that asks for its results
    fails from it -- nothing is started a second time on a GPU that a child may just have faulted or hung."""
    if not _child:
        _child["error"], _child["cases"] = "the child process did not finish", None      # (kept if anything below raises)
        out = str(tmp_path_factory.mktemp("train_dw") / "cases.json")
        env = dict(os.environ, NEFES_PARITY_LOG=os.devnull)
        if K.this_kernel() == "x6":
            env["NEFES_TRAIN_DW"] = "f32"
        else:
            env.pop("NEFES_TRAIN_DW")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_kernel_cases.py"), out], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                _child["error"] = f"the child process ended with {r.returncode}: {r.stderr[-2000:]}"
            else:
                with open(out) as f:
                    got = json.load(f)
                if got["kernel"] == K.this_kernel():
                    _child["error"] = f"the child process ran the {got['kernel']} kernel too"
                else:
                    _child["error"], _child["cases"] = None, got["cases"]
        except Exception as e:                                                            # TimeoutExpired, no or broken JSON, ...
            _child["error"] = f"the child process: {e!r}"
    assert _child["error"] is None, _child["error"]
    return _child["cases"]


_raised = []


@contextlib.contextmanager
def _gpu():
    """A launch of this file's own that raised (a HIP error at the synchronize: the context is gone) is remembered: the tests after it
    fail from that record and launch nothing more."""
    assert not _raised, f"an earlier launch of this file raised: {_raised[0]}"
    try:
        yield
    except Exception as e:
        _raised.append(repr(e))
        raise


def _outcome(kernel, key, tmp_path_factory, run):
    if kernel == K.this_kernel():
        from nefes_amd import lib as L
        with _gpu():
            return run(L.load())
    return _other_kernel_results(tmp_path_factory)[key]


def _ids(cases):
    return [c[2] + "-" + K.dw_case_id(*c) for c in cases]             # kernel, the instance that serves it, shape, entry point, x_relu


EXACT = [(ot, it, kernel, bias, relu) for kernel in K.KERNELS for ot, it, bias, relu in K.dw_exact_cases()]
PER_SHAPE = [(ot, it, kernel) for kernel in K.KERNELS for _, (ot, it) in K.SHAPES]
GENERAL = [(ot, it, kernel) for kernel in K.KERNELS for ot, it in K.GENERAL_SHAPES]


@pytest.mark.parametrize("ot,it,kernel,bias,relu", EXACT, ids=_ids(EXACT))
def test_dw_exact(ot, it, kernel, bias, relu, tmp_path_factory):
    """partial[share] == sum over the share's tiles of G f(X)^T (and G's row sums in column n_in), bit for bit, G and X integers in
    [-4, 4]; at every (tiles, shares), row offset, buffer arrangement and partial stride of train_kernel_cases.dw_configs; exactly the
    product's elements written into a buffer of NaN; every row of the operand buffers that is not an operand is NaN."""
    from nefes_amd import train as TR
    nto, nti = K.instance(ot, it, kernel)
    if kernel == "x6":
        assert TR._dw_grid(ot, it)[0] == (ot // nto) * (it // nti)
    res = _outcome(kernel, "exact/" + K.dw_case_id(ot, it, kernel, bias, relu), tmp_path_factory,
                   lambda lib: K.run_dw_exact(lib, ot, it, bias, relu))
    assert res["largest"] < 2 ** 24                       # the exactness condition: every partial sum is an integer below 2^24
    assert res["ok"], res["fails"]


@pytest.mark.parametrize("ot,it,kernel", PER_SHAPE, ids=_ids(PER_SHAPE))
def test_dw_split_completeness(ot, it, kernel, tmp_path_factory):
    """Operands +-2^a (1 + 2^-8 + 2^-16): the truncation split gives h, m, l = 1, 2^-8, 2^-16 times the scale, all three parts
    non-zero.  The six kept terms (hh, hm, mh, mm, lh, hl) sum to 1 + 2^-7 + 2^-15 + 2^-16 per product, the three dropped ones to
    2^-23 + 2^-32; one sign per row, so the 128 products of a share do not cancel.  Bound, derived: |hip - exact| <= 2^-17 |exact|
    -- half of what the smallest kept term moves the result by (without l.h or h.l: 2^-16 / (1 + 2^-7) = 1.51e-5 against the bound's
    7.63e-6; without m.m the same; without m.h or h.m 2^-8), and above 64 accumulate steps each one ulp off (64 x 2^-24 = 3.8e-6).
    The fp32 kernel is held to the same bound.  A product that is exactly zero (ReLU of a negative row) is exactly zero."""
    res = _outcome(kernel, "completeness/" + K.dw_case_id(ot, it, kernel), tmp_path_factory, lambda lib: K.run_dw_completeness(lib, ot, it))
    assert res["rc"] == 0
    print(f"[train_dw {kernel} {ot}x{it}] split completeness: worst |hip - exact| / |exact| = {res['worst']:.3e}  (bound {2. ** -17:.3e})")
    P.record(f"train_dw_completeness[{kernel},{K.dw_case_id(ot, it, kernel)}]", "dW, worst element / |exact|", e_hip=res["worst"], e_ref=None,
             bound=2. ** -17)
    assert res["nonzero"] == 0
    assert res["worst"] <= 2. ** -17


@pytest.mark.parametrize("ot,it,kernel", GENERAL, ids=_ids(GENERAL))
def test_dw_general_floats(ot, it, kernel, tmp_path_factory):
    """Operands |N(0,1)| 2^U{-6..6}, K = 256 samples per share: distance from float64, normalised per element with sum_s |g| |x|,
    within (K + 6) 2^-24 -- the worst case of an fp32 accumulation of K products -- or 1.5 x torch's fp32 matmul's own."""
    res = _outcome(kernel, "general/" + K.dw_case_id(ot, it, kernel), tmp_path_factory, lambda lib: K.run_dw_general(lib, ot, it))
    assert res["rc"] == 0
    print(f"[train_dw {kernel} {ot}x{it}] general floats vs float64: hip {res['e_hip']:.3e}  torch fp32 {res['e_ref']:.3e}")
    P.check(f"train_dw_general[{kernel},{K.dw_case_id(ot, it, kernel)}]", "dW / sum |g||x|", res["e_hip"], res["e_ref"],
            tol=(K.GENERAL_K + 6) * 2. ** -24)


@pytest.mark.parametrize("n_out", [8, 24, 136, 256])
@pytest.mark.parametrize("n_in", [64, 128, 256])
def test_dx_exact(n_in, n_out):
    """D[i, s] (+)= sum_o Wt[i, o] G[g_row0 + o, s], masked with acts > 0 (an exact zero masks), G and Wt integers in [-2, 2]:
    bit for bit, every row outside the destination block untouched (train_kernel_cases.run_dx_exact)."""
    from nefes_amd import lib as L
    with _gpu():
        res = K.run_dx_exact(L.load(), n_in, n_out)
    assert res["ok"], res["fails"]


# ---- head_grad -------------------------------------------------------------------------------------------------------------------
N_RAYS, N_SMP = 5, 33                    # 165 samples: the second tile is ragged


@pytest.mark.parametrize("mode", ["static", "full", "static_no_transient"])
@pytest.mark.parametrize("Cf", [0, 16, 29, 30, 128])             # 3 + C = 3, 19, exactly one tile, one row more, 131
@pytest.mark.parametrize("Wd", [128, 256])
def test_head_grad_vs_float64(Wd, Cf, mode):
    """d raw -> the head blocks of dacts: feature rows copied bit for bit; sigma, transient sigma and beta g (1 - exp(-y)), transient
    rgb g y (1 - y), within 2^-22 |g| (two ulps of a factor in [0, 1]) of float64; padding rows and samples beyond N S exactly zero;
    every other row keeps its bits."""
    from nefes_amd import lib as L
    lib = L.load()
    full = mode == "full"
    desc = L.NefesNetDesc(Wd, Cf, 0 if mode == "static_no_transient" else 1, 0, 0)
    C3, M = 3 + Cf, N_RAYS * N_SMP
    R = C3 + (6 if full else 1)
    g = torch.Generator().manual_seed(Wd + Cf)
    raw = torch.rand(N_RAYS, R, N_SMP, generator=g) * 0.998 + 0.001                                 # rgb, features, transient rgb in (0, 1)
    softplus = lambda n: torch.exp(torch.rand(N_RAYS, n, N_SMP, generator=g) * (math.log(20.) - math.log(1e-4)) + math.log(1e-4))
    raw[:, C3:C3 + 1] = softplus(1)                                                                 # 1e-4 .. 20
    raw[0, C3, :2] = torch.tensor([1e-4, 20.])
    if full:
        raw[:, C3 + 4:] = softplus(2)
    G = torch.randn(N_RAYS, R, N_SMP, generator=g)
    rows = int(lib.nefes_train_rows(C.byref(desc)))
    off = {b: int(lib.nefes_train_row_offset(C.byref(desc), b)) for b in (L.TB_RGB, L.TB_SIG, L.TB_TH, L.TB_END)}
    assert off[L.TB_END] == rows and rows % 32 == 0
    ntr = 1 if C3 <= 32 else 5                                                                      # the two head classes (layout.h nefes_head_ntr)
    assert off[L.TB_SIG] - off[L.TB_RGB] == 32 * ntr and off[L.TB_TH] - off[L.TB_SIG] == 32 and rows - off[L.TB_TH] == 32
    n_tiles = (M + 127) // 128
    before = torch.randn(n_tiles, rows, 128, generator=g)
    before[:, ::3] = float("nan")
    buf = torch.full(((n_tiles + 1) * rows * 128,), float("nan"), device=DEV)
    buf[:n_tiles * rows * 128] = before.reshape(-1).to(DEV)
    mode_id = L.FIELD_FULL if full else L.FIELD_STATIC
    with _gpu():
        raw_d, G_d = raw.to(DEV), G.to(DEV)
        rc = lib.nefes_train_head_grad(C.byref(desc), mode_id, N_RAYS, N_SMP, raw_d.data_ptr(), G_d.data_ptr(), buf.data_ptr(), None)
        torch.cuda.synchronize()
    assert rc == 0
    flat = buf.cpu()
    assert flat[n_tiles * rows * 128:].isnan().all()
    got = from_device(flat[:n_tiles * rows * 128].view(n_tiles, rows, 128))
    old = from_device(before)
    by_sample = lambda blk, n: got[:, off[blk]:off[blk] + n].permute(1, 0, 2).reshape(n, -1)        # [n rows, tiles * 128 samples]
    cols = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], M)                                      # [N, c, S] -> [c, N S]
    rgb, sig = by_sample(L.TB_RGB, 32 * ntr), by_sample(L.TB_SIG, 32)
    assert torch.equal(rgb[:C3, :M], cols(G[:, :C3]))                                               # copied
    assert not rgb[C3:].any() and not rgb[:, M:].any() and not sig[1:].any() and not sig[:, M:].any()
    y, gs = cols(raw).double(), cols(G).double()

    def close(name, have, want, gg):
        err = float(((have.double() - want).abs() / gg.abs()).max())
        print(f"[head_grad {Wd},{Cf},{mode}] {name}: worst |err| / |g| = {err:.3e}  (bound {2. ** -22:.3e})")
        P.record(f"train_head_grad[{Wd},{Cf},{mode}]", name, e_hip=err, e_ref=None, bound=2. ** -22)
        assert err <= 2. ** -22, name
    close("sigma", sig[0, :M], gs[C3] * (1 - torch.exp(-y[C3])), gs[C3])
    touched = torch.zeros(rows, dtype=torch.bool)
    touched[off[L.TB_RGB]:off[L.TB_TH]] = True
    if full:
        th = by_sample(L.TB_TH, 32)
        assert not th[5:].any() and not th[:, M:].any()
        yt, gt = y[C3 + 1:], gs[C3 + 1:]
        close("transient rgb", th[:3, :M], gt[:3] * (yt[:3] * (1 - yt[:3])), gt[:3])
        close("transient sigma, beta", th[3:5, :M], gt[3:] * (1 - torch.exp(-yt[3:])), gt[3:])
        touched[off[L.TB_TH]:] = True
    assert torch.equal(got[:, ~touched].view(torch.int32), old[:, ~touched].view(torch.int32))      # (the TH block too in static mode)
