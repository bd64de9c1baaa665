"""The packer's fold of xyz_encoding_final into the head matrices (NefesNetDesc.fold_final, nefes_amd/csrc/pack.cpp fold_head).

xyz_encoding_final is a Linear with no activation behind it, read by dir_encoding.0 and transient_encoding.0 only, so for frozen
weights  head(cat[final, d]) = (W_head[:, :W] W_fin) relu(h8) + W_head[:, W:] d + (W_head[:, :W] b_fin + b_head).  With the option set
the fp16 two-part full / static streams carry the folded head and no FINAL segment; with 0 the blob is the unfolded one, byte for byte.
Stream reading helpers are those of tests/test_pack_stream.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from oracle import ref_cpu as O
from tests.test_pack_stream import (H3B, H3F, StreamH3, _h3_slab_kib, abs_max, acc_to_vec, compact, emb_slot, emb_vector, emb_vector_T,
                                    relu_max, rho, softplus, tau_of)

# segment / bias-block ordinals of the folded streams (layout.h NEFES_H3FF_* / NEFES_H3FBB_* / NEFES_H3BF_*): FINAL taken out
H3FF = {k: (v if v < H3F["FINAL"] else v - 1) for k, v in H3F.items() if k != "FINAL"}
H3BF = {k: (v if v < H3B["FINAL"] else v - 1) for k, v in H3B.items() if k != "FINAL"}
BBF = dict(L1=0, SIG=8, DIR=9, RGB=10, T0=11, T1=12, T2=13, TH=14)
H3_STREAMS = (L.STREAM_FWD_FULL_H3, L.STREAM_BWD_FULL_H3, L.STREAM_FWD_STATIC_H3, L.STREAM_BWD_STATIC_H3)


def _desc(Wd, Cf, tr, enc=0, fold=None):
    return L.NefesNetDesc(Wd, Cf, 1 if tr else 0, enc) if fold is None else L.NefesNetDesc(Wd, Cf, 1 if tr else 0, enc, fold)


def _pack_tensors(desc, arrs):
    lib = L.load()
    info = L.NefesBlobInfo()
    assert lib.nefes_blob_info(desc, info) == 0
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    blob = np.zeros(info.total_bytes, np.uint8)
    assert lib.nefes_pack_weights(desc, ptrs, len(arrs), blob.ctypes.data, blob.nbytes) == 0
    return info, blob


def _params(Wd, Cf, typ="fine", final_scale=1.0):
    p = O.make_field_params(typ, Wd, Cf)
    if final_scale != 1.0:
        p = dict(p)
        p["xyz_encoding_final.weight"] = p["xyz_encoding_final.weight"] * final_scale
    names = [n for n, _, _ in O.field_param_shapes(typ, Wd, Cf)]
    arrs = []
    for n in names:
        arrs += [np.ascontiguousarray(p[n + ".weight"].numpy()), np.ascontiguousarray(p[n + ".bias"].numpy())]
    return p, arrs


def _info_tuple(info):
    return (info.total_bytes,) + tuple((s.slab_off, s.n_slabs, s.bias_floats, s.bias_off, s.scale_off, s.scale_count) for s in info.stream)


@pytest.mark.parametrize("Wd,Cf,tr,enc", [(128, 128, False, 0), (128, 128, True, 0), (256, 16, True, 0), (256, 16, True, 1),
                                         (256, 128, True, 0), (128, 16, False, 0), (256, 77, True, 0)])
def test_fold_zero_is_the_unfolded_blob(Wd, Cf, tr, enc):
    """fold_final = 0 written out and the field left at its zero initialisation give the same geometry, blob, slot map and reduction
    plan; fold_final = 1 changes the four fp16 head streams only (every other stream's bytes are the unfolded ones) and has no slot
    map / plan (the device re-pack cannot refresh a product of parameters)."""
    lib = L.load()
    n = 36 if tr else 24
    elems = (C.c_int64 * 36)()
    d0, dz, d1 = _desc(Wd, Cf, tr, enc, 0), _desc(Wd, Cf, tr, enc), _desc(Wd, Cf, tr, enc, 1)
    assert C.sizeof(d0) == 20
    info0 = L.NefesBlobInfo()
    assert lib.nefes_blob_info(d0, info0) == 0
    m = [np.zeros(info0.total_bytes // 2, np.uint32) for _ in range(2)]
    plans = []
    for d, mm in ((d0, m[0]), (dz, m[1])):
        assert lib.nefes_pack_map(d, mm.ctypes.data_as(C.c_void_p), mm.size, C.cast(elems, C.c_void_p)) == 0
        need = C.c_size_t(0)
        assert lib.nefes_pack_h3_plan(d, None, 0, C.byref(need)) == 0
        plan = np.zeros(need.value, np.int32)
        assert lib.nefes_pack_h3_plan(d, plan.ctypes.data_as(C.c_void_p), plan.size, None) == 0
        plans.append(plan)
    assert np.array_equal(m[0], m[1]) and np.array_equal(plans[0], plans[1])
    rng = np.random.default_rng(Wd + Cf + enc)
    tens = [np.ascontiguousarray((rng.standard_normal(s) * 0.1).astype(np.float32)) for s in list(elems)[:n]]
    (i0, b0), (iz, bz), (i1, b1) = (_pack_tensors(d, tens) for d in (d0, dz, d1))
    assert _info_tuple(i0) == _info_tuple(iz) == _info_tuple(info0)
    assert np.array_equal(b0, bz)
    assert b0[8:24].tobytes() == bytes(d0)[:16] and not b0[24:32].any()      # header: the description, fold_final = 0 where zeros were
    slab = lambda d, k: int(lib.nefes_stream_slab_bytes(d, k))
    for k in range(13):
        s0, s1 = i0.stream[k], i1.stream[k]
        if k in H3_STREAMS and s0.n_slabs:
            nt_final = Wd // 32
            ups = slab(d0, k) // 2048
            assert s0.n_slabs - s1.n_slabs == (nt_final * (Wd // 16) + ups - 1) // ups      # exactly the FINAL segment's slabs
            continue
        assert (s0.n_slabs, s0.bias_floats, s0.scale_off, s0.scale_count) == (s1.n_slabs, s1.bias_floats, s1.scale_off, s1.scale_count)
        if s0.n_slabs:
            nb = s0.n_slabs * slab(d0, k)
            assert np.array_equal(b0[s0.slab_off:s0.slab_off + nb], b1[s1.slab_off:s1.slab_off + nb]), k
            assert np.array_equal(b0[s0.bias_off:s0.bias_off + 4 * s0.bias_floats], b1[s1.bias_off:s1.bias_off + 4 * s1.bias_floats]), k
    mm = np.zeros(i1.total_bytes // 2, np.uint32)
    assert lib.nefes_pack_map(d1, mm.ctypes.data_as(C.c_void_p), mm.size, C.cast(elems, C.c_void_p)) == -2
    assert lib.nefes_pack_h3_plan(d1, None, 0, C.byref(C.c_size_t(0))) == -2


def _folded64(p, head):
    """float64 [W/2, W + 27] folded matrix and [W/2] folded bias of dir_encoding.0 / transient_encoding.0"""
    Wh, bh = p[head + ".weight"].double().numpy(), p[head + ".bias"].double().numpy()
    Wf, bf = p["xyz_encoding_final.weight"].double().numpy(), p["xyz_encoding_final.bias"].double().numpy()
    Wd = Wf.shape[0]
    return np.concatenate([Wh[:, :Wd] @ Wf, Wh[:, Wd:]], 1), Wh[:, :Wd] @ bf + bh


def _fwd_shapes(Wd, Cf, full=True):
    """(nt, k16) of the folded forward stream's segments in order"""
    NTW, NTH, NTR = Wd // 32, Wd // 64, (1 if 3 + Cf <= 32 else 5)
    ndt = 2 * NTH if full else NTH
    s = [(NTW, 4)] + [(NTW, Wd // 16)] * 4 + [(NTW, 4)] + [(NTW, Wd // 16)] * 3 + [(1, Wd // 16), (ndt, Wd // 16), (ndt, 2), (NTR, Wd // 32)]
    return s + ([(NTH, Wd // 32), (NTH, Wd // 32), (1, Wd // 32)] if full else [])


def _decode(st, first_slab, nt, k16):
    """(hi + lo) of an fp16 segment as [nt * 32 accumulator rows][16 k16 slots s = 8q + i][2 halves]"""
    out = np.zeros((nt * 32, 8 * k16, 2))
    for u in range(k16 * nt):
        sl, uu = first_slab + u // st.ups, u % st.ups
        q, t = u // nt, u % nt
        unit = st.raw[sl, uu * 1024:(uu + 1) * 1024].reshape(2, 64, 8)
        val = unit[0].view(np.float16).astype(np.float64) + unit[1].view(np.float16).astype(np.float64)
        for lane in range(64):
            out[32 * t + (lane & 31), 8 * q:8 * q + 8, lane >> 5] = val[lane]
    return out


def _slab_of(st, shapes, seg):
    return sum((nt * k + st.ups - 1) // st.ups for nt, k in shapes[:seg])


@pytest.mark.parametrize("Wd,Cf,scale", [(256, 16, 1.0), (256, 128, 1.0), (128, 128, 1.0), (256, 16, 2.0 ** 10), (256, 16, 2.0 ** -10)])
def test_folded_segments_decode_to_the_float64_product(Wd, Cf, scale):
    """The folded head segments, forward and transposed, decode to (W_head[:, :W] W_fin | W_head[:, W:]) computed in float64: per entry
    within 2^-21 of the folded matrix' largest entry (a 22-bit split of the scaled value) plus the entry's own fp32 rounding; the
    folded biases to one fp32 ulp; row bounds and bias maxima of the scale table bound the float64 values.  scale = 2^+-10 on
    xyz_encoding_final.weight puts the folded columns and the direction columns of the head ten binades apart either way: they share
    one weight exponent (pack.cpp assign_weight_exponents) and the smaller group keeps the same bound."""
    p, arrs = _params(Wd, Cf, "fine", scale)
    info, blob = _pack_tensors(_desc(Wd, Cf, True, 0, 1), arrs)
    blob = blob.tobytes()
    NTW, NTH = Wd // 32, Wd // 64
    Fd, bd = _folded64(p, "dir_encoding.0")
    Ft, bt = _folded64(p, "transient_encoding.0")
    F = np.concatenate([Fd, Ft], 0)                                 # stacked [dir ; t0]
    wmax = np.abs(F).max()
    tol = lambda ref: 2.0 ** -21 * wmax + 2.0 ** -24 * np.abs(ref)
    # ---- forward: DT_H (natural slots) and DT_D (direction-embedding slots) ----
    si = info.stream[L.STREAM_FWD_FULL_H3]
    n_segs = len(H3FF)
    assert si.scale_count == (2 * n_segs + len(BBF) + 7 + 3) // 4 * 4   # 16 segments, 15 bias blocks (L1..L8 = 8): no FINAL
    st = StreamH3(blob, si, _h3_slab_kib("FWD", Wd), n_segs)
    shapes = _fwd_shapes(Wd, Cf)
    assert sum((nt * k + st.ups - 1) // st.ups for nt, k in shapes) == si.n_slabs
    e = int(st.wexp[H3FF["DT_H"]])
    assert e == int(st.wexp[H3FF["DT_D"]]) and 2.0 ** 14 <= wmax * 2.0 ** e < 2.0 ** 15
    got = _decode(st, _slab_of(st, shapes, H3FF["DT_H"]), 2 * NTH, Wd // 16) * 2.0 ** -e
    for s in range(Wd // 2):
        for g in range(2):
            col = 32 * (s >> 4) + rho(g, s & 15)
            assert np.all(np.abs(got[:, s, g] - F[:, col]) <= tol(F[:, col])), (s, g)
    got = _decode(st, _slab_of(st, shapes, H3FF["DT_D"]), 2 * NTH, 2) * 2.0 ** -e
    for s in range(16):
        for g in range(2):
            k = emb_slot(4, s, g)
            ref = F[:, Wd + k] if k >= 0 else np.zeros(F.shape[0])
            assert np.all(np.abs(got[:, s, g] - ref) <= tol(ref)), (s, g)
    # biases (blocks L1..L8, SIG, DIR, RGB, T0): one ulp of fp32; scale table: upper bounds of the float64 values
    NTR = 1 if 3 + Cf <= 32 else 5
    o_dir = 8 * Wd + 32
    o_t0 = o_dir + Wd // 2 + 32 * NTR
    for off, ref in ((o_dir, bd), (o_t0, bt)):
        b = st.bias[off:off + Wd // 2].astype(np.float64)
        assert np.all(np.abs(b - ref) <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    assert st.rowb[H3FF["DT_H"]] >= np.abs(F[:, :Wd]).sum(1).max() and st.rowb[H3FF["DT_D"]] >= np.abs(F[:, Wd:]).sum(1).max()
    assert st.rowb[H3FF["DT_H"]] <= 1.001 * np.abs(F[:, :Wd]).sum(1).max()
    assert st.bmax[BBF["DIR"]] >= np.abs(bd).max() and st.bmax[BBF["T0"]] >= np.abs(bt).max()
    assert st.bmax[BBF["DIR"]] <= np.abs(bd).max() * (1 + 2.0 ** -22)
    # ---- backward: T0^T and DIR^T (tile 0 = d direction-embedding slots, tiles 1.. = d h8), then SIG: no FINAL^T ----
    si = info.stream[L.STREAM_BWD_FULL_H3]
    sb = StreamH3(blob, si, _h3_slab_kib("BWD", Wd), len(H3BF))
    KR16 = 2 if 3 + Cf <= 32 else 9
    bshapes = [(NTH, KR16), None, (NTH, Wd // 32), (NTH, Wd // 32), (NTW + 1, Wd // 32), (NTW + 1, Wd // 32)]
    pos = (NTH * KR16 + sb.ups - 1) // sb.ups + 1                   # RGB^T, then the fp32 transient-head segment (3 k-steps: one slab)
    pos += 2 * ((NTH * (Wd // 32) + sb.ups - 1) // sb.ups)           # T2^T, T1^T
    assert all(int(sb.wexp[H3BF[k]]) == e for k in ("T0", "DIR"))
    for name, Fm in (("T0", Ft), ("DIR", Fd)):
        got = _decode(sb, pos, NTW + 1, Wd // 32) * 2.0 ** -e
        pos += ((NTW + 1) * (Wd // 32) + sb.ups - 1) // sb.ups
        for s in range(Wd // 4):
            for g in range(2):
                k = 32 * (s >> 4) + rho(g, s & 15)                  # row of the head matrix = k-value of its transposed product
                assert np.all(np.abs(got[32:, s, g] - Fm[k, :Wd]) <= tol(Fm[k, :Wd])), (name, s, g)
                for i in range(32):
                    c = emb_slot(4, (i & 3) + 4 * (i >> 3), (i >> 2) & 1)
                    ref = Fm[k, Wd + c] if c >= 0 else 0.0
                    assert abs(got[i, s, g] - ref) <= tol(ref), (name, s, g, i)
        rb = sb.rowb[H3BF[name]]
        assert rb >= np.abs(Fm).sum(0).max() and rb <= 1.001 * np.abs(Fm).sum(0).max()
    # what follows is static_sigma^T (fp32, exponent 0) and layer 8: the table has 15 segments
    assert int(sb.wexp[H3BF["SIG"]]) == 0 and si.scale_count == (2 * len(H3BF) + 3) // 4 * 4
    # ---- static streams: dir_encoding alone ----
    si = info.stream[L.STREAM_FWD_STATIC_H3]
    ss = StreamH3(blob, si, _h3_slab_kib("FWD", Wd), H3FF["RGB"] + 1)
    sshapes = _fwd_shapes(Wd, Cf, False)
    assert sum((nt * k + ss.ups - 1) // ss.ups for nt, k in sshapes) == si.n_slabs and int(ss.wexp[H3FF["DT_H"]]) == e
    got = _decode(ss, _slab_of(ss, sshapes, H3FF["DT_H"]), NTH, Wd // 16) * 2.0 ** -e
    for s in range(Wd // 2):
        for g in range(2):
            col = 32 * (s >> 4) + rho(g, s & 15)
            assert np.all(np.abs(got[:, s, g] - Fd[:, col]) <= tol(Fd[:, col]))


@pytest.mark.parametrize("Wd,Cf,scale", [(256, 16, 1.0), (256, 128, 1.0), (128, 128, 1.0), (256, 16, 2.0 ** 10), (256, 16, 2.0 ** -10)])
def test_folded_streams_reproduce_the_mlp(Wd, Cf, scale):
    """The folded streams consumed in kernel order (field_fwd_h3.hip / field_bwd_h3.hip FOLD) with the kernels' scale bookkeeping:
    the trunk ends with layer 8, static_sigma and the stacked head read relu(h8), the head's bound is rowbound(folded) max relu(h8) +
    rowbound(direction part) max |d| + max |b|; backward, the transposed head products give d h8 and static_sigma^T joins them at
    their exponent.  Forward against the float64 oracle and backward against float64 autograd, to the bounds
    tests/test_pack_stream.py::test_h3_streams_reproduce_the_mlp holds the unfolded streams to; ReLU masks are the trunk's own."""
    n = 12
    g = torch.Generator().manual_seed(8)
    pts = (torch.rand(n, 3, generator=g) - .5) * 5
    pts[0] *= 1e-3
    pts[1] *= 6.
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    e63, e27 = O.freq_encode(pts, 10), O.freq_encode(dirs, 4)
    NTW, NTH, NTR = Wd // 32, Wd // 64, (1 if 3 + Cf <= 32 else 5)
    E, D = emb_vector(e63.numpy(), 10, 32), emb_vector(e27.numpy(), 4, 16)
    mE = np.maximum(1.0, np.abs(pts.numpy()).max(1)).astype(np.float32)
    zeros = np.zeros(n, np.int64)
    p, arrs = _params(Wd, Cf, "fine", scale)
    info, blob = _pack_tensors(_desc(Wd, Cf, True, 0, 1), arrs)
    blob = blob.tobytes()
    st = StreamH3(blob, info.stream[L.STREAM_FWD_FULL_H3], _h3_slab_kib("FWD", Wd), len(H3FF))
    b = {f"L{l}": st.bias_tiles(NTW, n) for l in range(1, 9)}
    for name, nt in (("SIG", 1), ("DIR", NTH), ("RGB", NTR), ("T0", NTH), ("T1", NTH), ("T2", NTH), ("TH", 1)):
        b[name] = st.bias_tiles(nt, n)
    w, rb, bm = st.wexp, st.rowb, st.bmax
    masks, out = {}, {}
    tau = tau_of(mE, w[H3FF["L1"]])
    es = tau + w[H3FF["L1"]]
    acc = b["L1"] * np.exp2(es)[None, None, :]
    st.mma(NTW, E, tau, acc)
    M = rb[H3FF["L1"]] * mE + bm[BBF["L1"]]
    for l in range(2, 9):
        seg = H3FF["L5H"] if l == 5 else H3FF[f"L{l}"]
        assert np.all(relu_max(acc, es) <= M), "row bound violated"
        masks[f"L{l - 1}"] = acc > 0
        H = acc_to_vec(np.maximum(acc, 0).astype(np.float32))
        mx = relu_max(acc, es)
        tau = tau_of(np.maximum(M, mE) if l == 5 else M, w[seg])
        es_new = tau + w[seg]
        nxt = b[f"L{l}"] * np.exp2(es_new)[None, None, :]
        st.mma(NTW, H, tau - es, nxt)
        M = rb[seg] * mx + bm[l - 1]
        if l == 5:
            st.mma(NTW, E, tau, nxt)
            M = M + rb[H3FF["L5E"]] * mE
        acc, es = nxt, es_new
    # acc = layer 8's pre-activation: static_sigma, then the stacked folded head, both on relu(h8)
    assert np.all(relu_max(acc, es) <= M)
    masks["L8"] = acc > 0
    H8 = acc_to_vec(np.maximum(acc, 0).astype(np.float32))
    tau = tau_of(M, w[H3FF["SIG"]])
    e_sg = tau + w[H3FF["SIG"]]
    sg = b["SIG"] * np.exp2(e_sg)[None, None, :]
    st.mma(1, H8, tau - es, sg)
    out["sigma"] = softplus(sg[0, 0] * np.exp2(-e_sg))
    mD = np.abs(D).max((0, 1)).astype(np.float32)
    ew = w[H3FF["DT_H"]]
    assert w[H3FF["DT_D"]] == ew
    tau = tau_of(np.maximum(M, mD), ew)
    es_dt = tau + ew
    dt = np.concatenate([b["DIR"], b["T0"]], 0) * np.exp2(es_dt)[None, None, :]
    mx = relu_max(acc, es)
    st.mma(2 * NTH, H8, tau - es, dt)
    st.mma(2 * NTH, D, tau, dt)
    M = rb[H3FF["DT_H"]] * mx + rb[H3FF["DT_D"]] * mD + max(bm[BBF["DIR"]], bm[BBF["T0"]])
    assert np.all(abs_max(dt, es_dt) <= M)
    masks["DIR"], masks["T0"] = dt[:NTH] > 0, dt[NTH:] > 0
    tau = tau_of(M, w[H3FF["RGB"]])
    es_ar = tau + w[H3FF["RGB"]]
    ar = b["RGB"] * np.exp2(es_ar)[None, None, :]
    st.mma(NTR, acc_to_vec(np.maximum(dt[:NTH], 0).astype(np.float32)), tau - es_dt, ar)
    out["rgbfeat"] = (ar * np.exp2(-es_ar)[None, None, :]).reshape(NTR * 32, n)[:3 + Cf].T
    src, es_s = dt[NTH:], es_dt
    for name in ("T1", "T2"):
        tau = tau_of(M, w[H3FF[name]])
        es_n = tau + w[H3FF[name]]
        acc2 = b[name] * np.exp2(es_n)[None, None, :]
        mx = relu_max(src, es_s)
        st.mma(NTH, acc_to_vec(np.maximum(src, 0).astype(np.float32)), tau - es_s, acc2)
        M = rb[H3FF[name]] * mx + bm[BBF[name]]
        assert np.all(relu_max(acc2, es_n) <= M)
        masks[name] = acc2 > 0
        src, es_s = acc2, es_n
    tau = tau_of(M, w[H3FF["TH"]])
    es_th = tau + w[H3FF["TH"]]
    th = b["TH"] * np.exp2(es_th)[None, None, :]
    st.mma(1, acc_to_vec(np.maximum(src, 0).astype(np.float32)), tau - es_s, th)
    th = th * np.exp2(-es_th)[None, None, :]
    sig = lambda x: 1 / (1 + np.exp(-x))
    out["t_rgb"], out["t_sigma"], out["t_beta"] = sig(th[0, :3]).T, softplus(th[0, 3]), softplus(th[0, 4])
    assert st.pos == st.raw.shape[0] and st.bpos == st.bias.shape[0]      # every slab and bias block consumed: no FINAL anywhere
    print(f"folded forward: least fp16 headroom of any operand (binades below 2^16): {st.headroom:.1f}")

    p64 = {k: v.double() for k, v in p.items()}
    emb = torch.cat([e63, e27], 1).double().requires_grad_()
    raw = O.field_forward(p64, emb, output_transient=True)
    r = raw.detach().numpy()
    C3 = 3 + Cf
    got = np.concatenate([out["rgbfeat"], out["sigma"][:, None], out["t_rgb"], out["t_sigma"][:, None], out["t_beta"][:, None]], 1)
    err = np.abs(got - r).max(0) / np.abs(r).max(0)
    print(f"folded forward vs float64: worst channel {err.max():.2e}")
    assert err.max() <= 3e-6, err

    # ---- backward-to-inputs on the folded stream, against float64 autograd ----
    g_raw = torch.randn(raw.shape, generator=g).double()
    (g_emb,) = torch.autograd.grad(raw, emb, g_raw)
    gr = g_raw.numpy()
    d_pre = {"rgbfeat": gr[:, :C3], "sigma": gr[:, C3] * (1 - np.exp(-r[:, C3])),
             "t_rgb": gr[:, C3 + 1:C3 + 4] * r[:, C3 + 1:C3 + 4] * (1 - r[:, C3 + 1:C3 + 4]),
             "t_sigma": gr[:, C3 + 4] * (1 - np.exp(-r[:, C3 + 4])), "t_beta": gr[:, C3 + 5] * (1 - np.exp(-r[:, C3 + 5]))}
    st = StreamH3(blob, info.stream[L.STREAM_BWD_FULL_H3], _h3_slab_kib("BWD", Wd), len(H3BF))
    w, rb = st.wexp, st.rowb
    assert st.bias.size == 0 and w[H3BF["T0"]] == w[H3BF["DIR"]] and all(w[H3BF[k]] == 0 for k in ("TH", "SIG"))
    Z = lambda nt: np.zeros((nt, 32, n), np.float64)
    f32v = lambda v: v.astype(np.float32)
    G2 = Z(NTH)
    KR16 = 2 if C3 <= 32 else 9
    dr = np.zeros((8 * KR16, 2, n), np.float32)
    for e in range(8 * KR16):
        for h in range(2):
            ch = 32 * (e >> 4) + rho(h, e & 15)
            if ch < C3:
                dr[e, h] = d_pre["rgbfeat"][:, ch]
    M_dr = np.abs(d_pre["rgbfeat"]).max(1).astype(np.float32)
    tau = tau_of(M_dr, w[H3BF["RGB"]])
    es_g2 = tau + w[H3BF["RGB"]]
    st.mma(NTH, dr, tau, G2)
    M_g2 = rb[H3BF["RGB"]] * M_dr
    T3 = Z(NTH)
    dth = [d_pre["t_rgb"][:, 0], d_pre["t_rgb"][:, 1], d_pre["t_rgb"][:, 2], d_pre["t_sigma"], d_pre["t_beta"]]
    st.mma32(NTH, compact(dth, 3), T3)
    M = rb[H3BF["TH"]] * np.abs(np.stack(dth, 1)).max(1).astype(np.float32)
    src, es = T3, zeros
    for name in ("T2", "T1"):
        tau = tau_of(M, w[H3BF[name]])
        dst = Z(NTH)
        mx = abs_max(src * masks[name], es)
        st.mma(NTH, acc_to_vec(f32v(src * masks[name])), tau - es, dst)
        M = rb[H3BF[name]] * mx
        src, es = dst, tau + w[H3BF[name]]
    tau = tau_of(np.maximum(M, M_g2), w[H3BF["T0"]])
    es_dt = tau + w[H3BF["T0"]]
    a9 = Z(NTW + 1)
    mt, mg = abs_max(src * masks["T0"], es), abs_max(G2 * masks["DIR"], es_g2)
    st.mma(NTW + 1, acc_to_vec(f32v(src * masks["T0"])), tau - es, a9)
    st.mma(NTW + 1, acc_to_vec(f32v(G2 * masks["DIR"])), tau - es_g2, a9)
    M = rb[H3BF["T0"]] * mt + rb[H3BF["DIR"]] * mg
    assert np.all(abs_max(a9, es_dt) <= M)
    dD = acc_to_vec(f32v(a9), 0, 1) * np.exp2(-es_dt)[None, None, :]
    # tiles 1.. ARE d h8 (before layer 8's mask); static_sigma^T accumulates onto them at their exponent
    acc, es = a9[1:].copy(), es_dt
    st.mma32(NTW, compact([d_pre["sigma"] * np.exp2(es)], 1), acc)
    M = M + rb[H3BF["SIG"]] * np.abs(d_pre["sigma"]).astype(np.float32)
    accE, es_e = None, None
    for l in range(8, 1, -1):
        assert np.all(abs_max(acc, es) <= M)
        tau = tau_of(M, w[H3BF[f"L{l}"]])
        masked = acc * masks[f"L{l}"]
        mx = abs_max(masked, es)
        Hm = acc_to_vec(f32v(masked))
        es_new = tau + w[H3BF[f"L{l}"]]
        if l == 5:
            a10 = Z(NTW + 2)
            st.mma(NTW + 2, Hm, tau - es, a10)
            accE, es_e, acc = a10[:2].copy(), es_new, a10[2:]
        else:
            acc = Z(NTW)
            st.mma(NTW, Hm, tau - es, acc)
        M = rb[H3BF[f"L{l}"]] * mx
        es = es_new
    tau = tau_of(M, w[H3BF["L1"]])
    es1 = tau + w[H3BF["L1"]]
    accE = accE * np.exp2(es1 - es_e)[None, None, :]
    st.mma(2, acc_to_vec(f32v(acc * masks["L1"])), tau - es, accE)
    assert st.pos == st.raw.shape[0]
    print(f"folded backward: least fp16 headroom of any operand: {st.headroom:.1f} binades")
    g63 = emb_vector_T(acc_to_vec(f32v(accE * np.exp2(-es1)[None, None, :])), 10, 63)
    g27 = emb_vector_T(f32v(dD[:14]), 4, 27)
    scale_g = np.abs(g_emb.numpy()).max(1, keepdims=True)
    e63_, e27_ = (np.abs(g63 - g_emb.numpy()[:, :63]) / scale_g).max(), (np.abs(g27 - g_emb.numpy()[:, 63:]) / scale_g).max()
    print(f"folded backward vs float64 autograd: d xyz-embedding {e63_:.2e}, d dir-embedding {e27_:.2e}")
    assert e63_ <= 5e-6 and e27_ <= 5e-6
