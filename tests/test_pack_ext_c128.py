"""The packer for hash-grid networks with the 128-channel feature head (width 256, NEFES_XYZ_EXTERNAL32, head class 1: 30 <= C <= 141),
without a GPU:

 * the fp16 two-part streams of such a network (sigma-only, full, full backward, static, static backward) exist, and -- consumed with
   numpy in the kernels' order, with the kernels' scale bookkeeping (tests/test_pack_stream.py StreamH3) -- reproduce the float64 field:
   forward sigma-only and full, backward to the 32-feature encoding and the view direction;
 * the device re-pack's slot map and reduction plan cover the new streams (expanded in numpy they give the host packer's blob);
 * the blobs of the shapes that packed before are byte-identical: sha256 digests taken from a build of the commit before this feature.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from oracle import ref_cpu as O
from tests.test_pack_stream import (H3B, H3F, StreamH3, _h3_slab_kib, abs_max, acc_to_vec, compact, emb_vector, emb_vector_T, relu_max,
                                    rho, softplus, tau_of)
from tests.test_pack_stream import test_pack_map_reproduces_host_pack as _pack_map_check

WD = 256
H3_STREAMS = ("STREAM_FWD_SIGMA_H3", "STREAM_FWD_FULL_H3", "STREAM_BWD_FULL_H3", "STREAM_FWD_STATIC_H3", "STREAM_BWD_STATIC_H3")


def pack(Wd, Cf, typ, enc):
    """(parameters, blob info, blob bytes) of the oracle's network (seed 0) on the frequency embedding (enc 0) or an external one (1)."""
    lib = L.load()
    in_xyz = 32 if enc else 63
    p = O.make_field_params(typ, Wd, Cf, in_xyz=in_xyz)
    d = L.NefesNetDesc(Wd, Cf, 1 if typ == "fine" else 0, enc)
    info = L.NefesBlobInfo()
    rc = lib.nefes_blob_info(d, info)
    assert rc == 0, rc
    arrs = []
    for n, _, _ in O.field_param_shapes(typ, Wd, Cf, in_xyz=in_xyz):
        arrs += [np.ascontiguousarray(p[n + ".weight"].numpy()), np.ascontiguousarray(p[n + ".bias"].numpy())]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    blob = np.zeros(info.total_bytes, np.uint8)
    assert lib.nefes_pack_weights(d, ptrs, len(arrs), blob.ctypes.data, blob.nbytes) == 0
    return p, info, blob.tobytes()


# sha256 of the blobs the library of the parent commit (0478530) packs for the oracle's seed-0 networks
PARENT_DIGESTS = {
    (256, 16, "coarse", 1): "06be392bc6fc85be558561c6d79f5b04674ba011a1e301a78a721595f4cdb374",
    (256, 16, "fine", 1): "b933f971fb7169789c0c9a409f93535e21b4dcaefda07b0bbb08ff59c0f3ce3c",
    (256, 128, "coarse", 0): "70153c7dbc69b7849cf257ac57e81e740af7fa520e1276679a138ad55a3a595c",
    (256, 128, "fine", 0): "fa80a871002cba26bf944db79614c68c846011eae5d0d5b52e91d93ccdb18109",
}


@pytest.mark.parametrize("key", sorted(PARENT_DIGESTS), ids=lambda k: f"W{k[0]}-C{k[1]}-{k[2]}-{'ext' if k[3] else 'freq'}")
def test_blobs_that_packed_before_are_byte_identical(key):
    _, _, blob = pack(*key)
    assert hashlib.sha256(blob).hexdigest() == PARENT_DIGESTS[key]


@pytest.mark.parametrize("Cf", [30, 128, 141])
def test_class1_external_network_has_fp16_streams(Cf):
    """Every fp16 two-part stream is there for both network types (the coarse one has no transient streams); the head is padded to the
    class: 5 tiles of bias rows, 9 k-steps of 16 channels in the transposed product."""
    for typ in ("coarse", "fine"):
        _, info, _ = pack(WD, Cf, typ, 1)
        have = {k: info.stream[getattr(L, k)].n_slabs > 0 for k in H3_STREAMS}
        want = {k: typ == "fine" or "FULL" not in k for k in H3_STREAMS}
        assert have == want, f"no fp16 streams: {typ} {have}"
    si = info.stream[L.STREAM_FWD_FULL_H3]
    # bias rows: 8 trunk layers + final (256 each), sigma (32), dir / t0 / t1 / t2 (128 each), rgb+feature (5 x 32), transient heads (32)
    assert si.scale_off == 9 * 256 + 32 + 4 * 128 + 5 * 32 + 32
    # a folded pack stays refused for external encodings of this class
    d = L.NefesNetDesc(WD, Cf, 1, 1, 1)
    assert L.load().nefes_blob_info(d, L.NefesBlobInfo()) != 0


@pytest.mark.parametrize("Cf,tr", [(128, True), (141, False), (30, True)])
def test_device_repack_plan_covers_the_new_streams(Cf, tr):
    """nefes_pack_map + nefes_pack_h3_plan of the class-1 external network, expanded in numpy as pack_device.hip does, give the host
    packer's blob -- the five (three without the transient part) fp16 streams and their scale tables included."""
    d = L.NefesNetDesc(WD, Cf, 1 if tr else 0, 1)
    info = L.NefesBlobInfo()
    assert L.load().nefes_blob_info(d, info) == 0
    n_h3 = sum(1 for k in H3_STREAMS if info.stream[getattr(L, k)].n_slabs)
    assert n_h3 == (5 if tr else 3), f"no fp16 streams to re-pack: {n_h3}"
    _pack_map_check(WD, Cf, tr, 1)


@pytest.mark.parametrize("Cf", [30, 128, 141])
def test_class1_external_streams_reproduce_the_mlp(Cf):
    """tests/test_pack_stream.py::test_h3_streams_reproduce_the_mlp for the external 32-feature encoding: compact slots (s, h) = feature
    2s + h in 16 k-steps for layers 1 and 5, the rgb+feature head padded to 5 tiles / 9 k-steps of 16, and d encoding out of tile 0 of the
    two embedding tiles (tile 1 is padding).  Forward against the float64 field to 3e-6 of each channel's max-norm, backward-to-inputs
    against float64 autograd to 5e-6 of each sample's largest gradient (the bounds of that test)."""
    n = 12
    g = torch.Generator().manual_seed(8)
    enc = (torch.rand(n, 32, generator=g) * 2 - 1) * 0.4
    enc[0] *= 1e-3                                                 # a sample with a tiny encoding
    enc[1] *= 6.                                                   # and a large one
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    e27 = O.freq_encode(dirs, 4)
    NTW, NTH, NTR = WD // 32, WD // 64, 5
    E = np.zeros((16, 2, n), np.float32)
    for s in range(16):
        for h in range(2):
            E[s, h] = enc[:, 2 * s + h].numpy()
    D = emb_vector(e27.numpy(), 4, 16)
    mE = np.abs(enc.numpy()).max(1).astype(np.float32)
    zeros = np.zeros(n, np.int64)

    def trunk(st, full):
        b = {f"L{l}": st.bias_tiles(NTW, n) for l in range(1, 9)}
        b["SIG"] = st.bias_tiles(1, n)
        if full:
            for name, nt in (("FINAL", NTW), ("DIR", NTH), ("RGB", NTR), ("T0", NTH), ("T1", NTH), ("T2", NTH), ("TH", 1)):
                b[name] = st.bias_tiles(nt, n)
        w, rb, bm = st.wexp, st.rowb, st.bmax
        BB = dict(L1=0, SIG=8, FINAL=9, DIR=10, RGB=11, T0=12, T1=13, T2=14, TH=15)
        masks, out = {}, {}
        tau = tau_of(mE, w[H3F["L1"]])
        es = tau + w[H3F["L1"]]
        acc = b["L1"] * np.exp2(es)[None, None, :]
        st.mma(NTW, E, tau, acc)
        M = rb[H3F["L1"]] * mE + bm[BB["L1"]]

        def sigma(acc, es, M):
            H = acc_to_vec(np.maximum(acc, 0).astype(np.float32))
            tau = tau_of(M, w[H3F["SIG"]])
            e_sg = tau + w[H3F["SIG"]]
            sg = b["SIG"] * np.exp2(e_sg)[None, None, :]
            st.mma(1, H, tau - es, sg)
            out["sigma"] = softplus(sg[0, 0] * np.exp2(-e_sg))

        for l in range(2, 10 if full else 9):
            name = f"L{l}" if l <= 8 else "FINAL"
            seg = H3F["L5H"] if l == 5 else H3F[name]
            assert np.all(relu_max(acc, es) <= M), "row bound violated"
            masks[f"L{l - 1}"] = acc > 0
            if l == 9:
                sigma(acc, es, M)
            H = acc_to_vec(np.maximum(acc, 0).astype(np.float32))
            mx = relu_max(acc, es)
            tau = tau_of(np.maximum(M, mE) if l == 5 else M, w[seg])
            es_new = tau + w[seg]
            nxt = b[name] * np.exp2(es_new)[None, None, :]
            st.mma(NTW, H, tau - es, nxt)
            M = rb[seg] * mx + bm[BB["FINAL"] if l == 9 else l - 1]
            if l == 5:
                assert w[H3F["L5E"]] == w[H3F["L5H"]]
                st.mma(NTW, E, tau, nxt)
                M = M + rb[H3F["L5E"]] * mE
            acc, es = nxt, es_new
        if not full:
            assert np.all(relu_max(acc, es) <= M)
            sigma(acc, es, M)
            assert st.pos == st.raw.shape[0] and st.bpos == st.bias.shape[0]
            return out, masks
        assert np.all(abs_max(acc, es) <= M)
        mD = np.abs(D).max((0, 1)).astype(np.float32)
        ew = w[H3F["DT_H"]]
        assert w[H3F["DT_D"]] == ew
        tau = tau_of(np.maximum(M, mD), ew)
        es_dt = tau + ew
        dt = np.concatenate([b["DIR"], b["T0"]], 0) * np.exp2(es_dt)[None, None, :]
        mx = abs_max(acc, es)
        st.mma(2 * NTH, acc_to_vec(acc.astype(np.float32)), tau - es, dt)
        st.mma(2 * NTH, D, tau, dt)
        M = rb[H3F["DT_H"]] * mx + rb[H3F["DT_D"]] * mD + max(bm[BB["DIR"]], bm[BB["T0"]])
        assert np.all(abs_max(dt, es_dt) <= M)
        masks["DIR"], masks["T0"] = dt[:NTH] > 0, dt[NTH:] > 0
        tau = tau_of(M, w[H3F["RGB"]])
        es_ar = tau + w[H3F["RGB"]]
        ar = b["RGB"] * np.exp2(es_ar)[None, None, :]
        st.mma(NTR, acc_to_vec(np.maximum(dt[:NTH], 0).astype(np.float32)), tau - es_dt, ar)
        ar = ar * np.exp2(-es_ar)[None, None, :]
        assert not ar.reshape(NTR * 32, n)[3 + Cf:].any()           # the padding rows of the head class: zero weights, zero bias
        out["rgbfeat"] = ar.reshape(NTR * 32, n)[:3 + Cf].T
        src, es_s = dt[NTH:], es_dt
        for name in ("T1", "T2"):
            tau = tau_of(M, w[H3F[name]])
            es_n = tau + w[H3F[name]]
            acc2 = b[name] * np.exp2(es_n)[None, None, :]
            mx = relu_max(src, es_s)
            st.mma(NTH, acc_to_vec(np.maximum(src, 0).astype(np.float32)), tau - es_s, acc2)
            M = rb[H3F[name]] * mx + bm[BB[name]]
            assert np.all(relu_max(acc2, es_n) <= M)
            masks[name] = acc2 > 0
            src, es_s = acc2, es_n
        tau = tau_of(M, w[H3F["TH"]])
        es_th = tau + w[H3F["TH"]]
        th = b["TH"] * np.exp2(es_th)[None, None, :]
        st.mma(1, acc_to_vec(np.maximum(src, 0).astype(np.float32)), tau - es_s, th)
        th = th * np.exp2(-es_th)[None, None, :]
        sig = lambda x: 1 / (1 + np.exp(-x))
        out["t_rgb"], out["t_sigma"], out["t_beta"] = sig(th[0, :3]).T, softplus(th[0, 3]), softplus(th[0, 4])
        assert st.pos == st.raw.shape[0] and st.bpos == st.bias.shape[0]
        return out, masks

    # sigma-only stream of the coarse network
    pc, info_c, blob_c = pack(WD, Cf, "coarse", 1)
    si = info_c.stream[L.STREAM_FWD_SIGMA_H3]
    assert si.n_slabs > 0, "no fp16 streams"
    out, _ = trunk(StreamH3(blob_c, si, _h3_slab_kib("FWD", WD), 10), False)
    ref = O.field_forward({k: v.double() for k, v in pc.items()}, enc.double(), sigma_only=True, in_xyz=32)[:, 0].numpy()
    assert np.abs(out["sigma"] - ref).max() <= 2e-6 * np.abs(ref).max()

    # full stream of the fine network
    pf, info_f, blob_f = pack(WD, Cf, "fine", 1)
    assert info_f.stream[L.STREAM_FWD_FULL_H3].n_slabs > 0, "no fp16 streams"
    st = StreamH3(blob_f, info_f.stream[L.STREAM_FWD_FULL_H3], _h3_slab_kib("FWD", WD), 17)
    out, masks = trunk(st, True)
    p64 = {k: v.double() for k, v in pf.items()}
    emb = torch.cat([enc, e27], 1).double().requires_grad_()
    raw = O.field_forward(p64, emb, output_transient=True, in_xyz=32)
    r = raw.detach().numpy()
    C3 = 3 + Cf
    got = np.concatenate([out["rgbfeat"], out["sigma"][:, None], out["t_rgb"], out["t_sigma"][:, None], out["t_beta"][:, None]], 1)
    err = np.abs(got - r).max(0) / np.abs(r).max(0)
    assert err.max() <= 3e-6, err

    # backward-to-inputs on the fp16 stream, against float64 autograd
    g_raw = torch.randn(raw.shape, generator=g).double()
    (g_emb,) = torch.autograd.grad(raw, emb, g_raw)
    gr = g_raw.numpy()
    d_pre = {"rgbfeat": gr[:, :C3], "sigma": gr[:, C3] * (1 - np.exp(-r[:, C3])),
             "t_rgb": gr[:, C3 + 1:C3 + 4] * r[:, C3 + 1:C3 + 4] * (1 - r[:, C3 + 1:C3 + 4]),
             "t_sigma": gr[:, C3 + 4] * (1 - np.exp(-r[:, C3 + 4])), "t_beta": gr[:, C3 + 5] * (1 - np.exp(-r[:, C3 + 5]))}
    st = StreamH3(blob_f, info_f.stream[L.STREAM_BWD_FULL_H3], _h3_slab_kib("BWD", WD), 16)
    w, rb = st.wexp, st.rowb
    assert st.bias.size == 0 and w[H3B["T0"]] == w[H3B["DIR"]] and all(w[H3B[k]] == 0 for k in ("TH", "SIG"))
    Z = lambda nt: np.zeros((nt, 32, n), np.float64)
    f32v = lambda v: v.astype(np.float32)
    G2 = Z(NTH)
    KR16 = 9
    dr = np.zeros((8 * KR16, 2, n), np.float32)
    for e in range(8 * KR16):
        for h in range(2):
            ch = 32 * (e >> 4) + rho(h, e & 15)
            if ch < C3:
                dr[e, h] = d_pre["rgbfeat"][:, ch]
    M_dr = np.abs(d_pre["rgbfeat"]).max(1).astype(np.float32)
    tau = tau_of(M_dr, w[H3B["RGB"]])
    es_g2 = tau + w[H3B["RGB"]]
    st.mma(NTH, dr, tau, G2)
    M_g2 = rb[H3B["RGB"]] * M_dr
    assert np.all(abs_max(G2, es_g2) <= M_g2)
    T3 = Z(NTH)
    dth = [d_pre["t_rgb"][:, 0], d_pre["t_rgb"][:, 1], d_pre["t_rgb"][:, 2], d_pre["t_sigma"], d_pre["t_beta"]]
    st.mma32(NTH, compact(dth, 3), T3)
    M = rb[H3B["TH"]] * np.abs(np.stack(dth, 1)).max(1).astype(np.float32)
    src, es = T3, zeros
    for name in ("T2", "T1"):                                       # transient_encoding.4^T, .2^T
        assert np.all(abs_max(src, es) <= M)
        tau = tau_of(M, w[H3B[name]])
        dst = Z(NTH)
        mx = abs_max(src * masks[name], es)
        st.mma(NTH, acc_to_vec(f32v(src * masks[name])), tau - es, dst)
        M = rb[H3B[name]] * mx
        src, es = dst, tau + w[H3B[name]]
    tau = tau_of(np.maximum(M, M_g2), w[H3B["T0"]])
    es_dt = tau + w[H3B["T0"]]
    a9 = Z(NTW + 1)
    mt, mg = abs_max(src * masks["T0"], es), abs_max(G2 * masks["DIR"], es_g2)
    st.mma(NTW + 1, acc_to_vec(f32v(src * masks["T0"])), tau - es, a9)
    st.mma(NTW + 1, acc_to_vec(f32v(G2 * masks["DIR"])), tau - es_g2, a9)
    M = rb[H3B["T0"]] * mt + rb[H3B["DIR"]] * mg
    assert np.all(abs_max(a9, es_dt) <= M)
    dD = acc_to_vec(f32v(a9), 0, 1) * np.exp2(-es_dt)[None, None, :]
    tau = tau_of(M, w[H3B["FINAL"]])
    es = tau + w[H3B["FINAL"]]
    acc = Z(NTW)
    mx = abs_max(a9[1:], es_dt)
    st.mma(NTW, acc_to_vec(f32v(a9), 1, NTW), tau - es_dt, acc)
    st.mma32(NTW, compact([d_pre["sigma"] * np.exp2(es)], 1), acc)
    M = rb[H3B["FINAL"]] * mx + rb[H3B["SIG"]] * np.abs(d_pre["sigma"]).astype(np.float32)
    accE, es_e = None, None
    for l in range(8, 1, -1):
        assert np.all(abs_max(acc, es) <= M)
        tau = tau_of(M, w[H3B[f"L{l}"]])
        masked = acc * masks[f"L{l}"]
        mx = abs_max(masked, es)
        Hm = acc_to_vec(f32v(masked))
        es_new = tau + w[H3B[f"L{l}"]]
        if l == 5:
            a10 = Z(NTW + 2)
            st.mma(NTW + 2, Hm, tau - es, a10)
            accE, es_e, acc = a10[:2].copy(), es_new, a10[2:]
        else:
            acc = Z(NTW)
            st.mma(NTW, Hm, tau - es, acc)
        M = rb[H3B[f"L{l}"]] * mx
        es = es_new
    tau = tau_of(M, w[H3B["L1"]])
    es1 = tau + w[H3B["L1"]]
    accE = accE * np.exp2(es1 - es_e)[None, None, :]
    st.mma(2, acc_to_vec(f32v(acc * masks["L1"])), tau - es, accE)
    assert st.pos == st.raw.shape[0]
    assert not accE[1].any()                                        # the second embedding tile is padding
    ge = acc_to_vec(f32v(accE * np.exp2(-es1)[None, None, :]), 0, 1)     # [16, 2, n]: slot (s, h) = feature 2s + h
    g32 = np.zeros((n, 32), np.float32)
    for s in range(16):
        for h in range(2):
            g32[:, 2 * s + h] = ge[s, h]
    g27 = emb_vector_T(f32v(dD[:14]), 4, 27)
    scale = np.abs(g_emb.numpy()).max(1, keepdims=True)
    assert (np.abs(g32 - g_emb.numpy()[:, :32]) / scale).max() <= 5e-6
    assert (np.abs(g27 - g_emb.numpy()[:, 32:]) / scale).max() <= 5e-6
