"""Generic field kernels on a SUPPLIED 32-feature encoding (nefes_amd/csrc/field_generic.hip, the gen_{fwd,bwd}_kernel<NCB, GenArgsExt> instances;
NEFES_XYZ_EXTERNAL32 in NefesGenericNetDesc), host side: the packer's layout against a numpy restatement of the kernels' addressing
and the float64 oracle, the refusals that need no device, and the routing (ops.field_route, NeRFH_NFF's predicates)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from oracle import ref_cpu as O
from tests import generic_util as G


def _nets(Wd, D, Cf):
    return G.modules(Wd, D, Cf, in_xyz=32)


def _pack(net, enc):
    from nefes_amd import ops
    lib = L.load()
    skip = 4 if net.D > 4 else -1
    desc = L.NefesGenericNetDesc(net.W, net.D, skip, net.W_features, 1 if net.encode_transient else 0, enc)
    n = int(lib.nefes_generic_blob_bytes(desc))
    assert n > 0
    sd = net.state_dict()
    host = []
    for name in ops.PackedGeneric.layer_names(net.D, net.encode_transient):
        host += [sd[name + ".weight"].float().contiguous(), sd[name + ".bias"].float().contiguous()]
    ptrs = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
    blob = np.zeros(n // 4, np.float32)
    assert lib.nefes_generic_pack(desc, ptrs, len(host), C.c_void_p(blob.ctypes.data), n) == 0
    return blob, skip


def _layers(Wd, D, skip, Cf, fine, er):
    """csrc/field_generic.hip gen_layout restated for an E region of `er` rows: {tag: (M, Mp, Kp, wt, wb, bias)} in floats."""
    H = Wd // 2
    spec = [(f"L{i + 1}", Wd, er if i == 0 else (er + Wd if i == skip else Wd)) for i in range(D)]
    spec += [("FINAL", Wd, Wd), ("SIGMA", 1, Wd), ("DIR", H, Wd + 32), ("RGB", 3 + Cf, H)]
    if fine:
        spec += [("T0", H, Wd + 32), ("T1", H, H), ("T2", H, H), ("TH", 5, H)]
    out, off = {}, 0
    for tag, M, Kp in spec:
        Mp = (M + 31) // 32 * 32
        out[tag] = (M, Mp, Kp, off, off + Kp * Mp, off + 2 * Kp * Mp)
        off += 2 * Kp * Mp + Mp
    return out, off + 64


def _forward(blob, lay, D, skip, e32, e27):
    """The FULL forward as the kernel addresses the blob's wt arrays: E = the 32 supplied rows, hidden columns of the skip layer
    from row 32 on.  -> (raw [n, R], the ReLU derivative of every hidden layer)."""
    n = e32.shape[0]
    E = e32.T.astype(np.float64)
    DV = np.zeros((32, n), np.float64); DV[:27] = e27.T
    keep = {}

    def prod(tag, x):
        M, Mp, Kp, wt, wb, bias = lay[tag]
        assert x.shape[0] == Kp, (tag, x.shape, Kp)
        w = blob[wt:wt + Kp * Mp].reshape(Kp, Mp).astype(np.float64)
        return (w.T @ x + blob[bias:bias + Mp].astype(np.float64)[:, None])[:M]

    def relu(tag, x):
        keep[tag] = x > 0
        return np.maximum(x, 0)

    h = relu("L1", prod("L1", E))
    for i in range(1, D):
        h = relu(f"L{i + 1}", prod(f"L{i + 1}", np.concatenate([E, h]) if i == skip else h))
    softplus = lambda x: np.log1p(np.exp(x))
    sigma = softplus(prod("SIGMA", h))
    fin = prod("FINAL", h)
    g = relu("DIR", prod("DIR", np.concatenate([fin, DV])))
    t = relu("T0", prod("T0", np.concatenate([fin, DV])))
    t = relu("T1", prod("T1", t))
    t = relu("T2", prod("T2", t))
    th = prod("TH", t)
    raw = np.concatenate([prod("RGB", g), sigma, 1 / (1 + np.exp(-th[:3])), softplus(th[3:4]), softplus(th[4:5])])
    return raw.T, keep


def _backward(blob, lay, Wd, D, skip, Cf, raw, keep, G_raw):
    """The transposed chain from the blob's wb arrays alone, in the kernel's order: d sum(raw * G_raw) / d encoding [n, 32]."""
    H = Wd // 2

    def tprod(tag, g, col0, cols):             # W[:, col0:col0+cols]^T g, W = wb[Mp][Kp]
        M, Mp, Kp, wt, wb, bias = lay[tag]
        w = blob[wb:wb + Kp * Mp].reshape(Mp, Kp).astype(np.float64)
        gp = np.zeros((Mp, g.shape[1])); gp[:g.shape[0]] = g
        return w[:, col0:col0 + cols].T @ gp

    Gt = G_raw.T.astype(np.float64)
    rt = raw.T
    sp = lambda y: 1 - np.exp(-y)                                           # softplus' in terms of its output
    g_rgb, g_sig = Gt[:3 + Cf], Gt[3 + Cf:4 + Cf] * sp(rt[3 + Cf:4 + Cf])
    y = rt[4 + Cf:7 + Cf]
    g_th = np.concatenate([Gt[4 + Cf:7 + Cf] * y * (1 - y), Gt[7 + Cf:9 + Cf] * sp(rt[7 + Cf:9 + Cf])])
    g_t2 = tprod("TH", g_th, 0, H) * keep["T2"]
    g_t1 = tprod("T2", g_t2, 0, H) * keep["T1"]
    g_t0 = tprod("T1", g_t1, 0, H) * keep["T0"]
    g_dir = tprod("RGB", g_rgb, 0, H) * keep["DIR"]
    g_fin = tprod("DIR", g_dir, 0, Wd) + tprod("T0", g_t0, 0, Wd)
    g_h = (tprod("FINAL", g_fin, 0, Wd) + tprod("SIGMA", g_sig, 0, Wd)) * keep[f"L{D}"]
    gE = np.zeros((32, Gt.shape[1]))
    for i in range(D - 1, 0, -1):
        hoff = 32 if i == skip else 0
        if i == skip:
            gE += tprod(f"L{i + 1}", g_h, 0, 32)
        g_h = tprod(f"L{i + 1}", g_h, hoff, Wd) * keep[f"L{i}"]
    gE += tprod("L1", g_h, 0, 32)
    return gE.T


@pytest.mark.parametrize("Wd,D,Cf", [(64, 6, 16), (96, 3, 30)])
def test_ext_blob_reproduces_the_mlp_forward_and_backward(Wd, D, Cf):
    """(64, 6): the skip layer reads [32 features, h]; (96, 3): no skip.  Forward from wt and the input gradient from wb against the
    float64 oracle on 50 random encodings, 1e-5; the blob is smaller than the frequency one by exactly the dropped embedding rows."""
    _, fine = _nets(Wd, D, Cf)
    blob, skip = _pack(fine, L.XYZ_EXTERNAL32)
    lay, total = _layers(Wd, D, skip, Cf, True, 32)
    assert total == blob.size
    for tag, (M, Mp, Kp, wt, wb, bias) in lay.items():          # the backward's copy is the transpose, everywhere
        np.testing.assert_array_equal(blob[wb:wb + Kp * Mp].reshape(Mp, Kp).T, blob[wt:wt + Kp * Mp].reshape(Kp, Mp))
    gen = torch.Generator().manual_seed(5)
    enc = (torch.rand(50, 32, generator=gen, dtype=torch.float64) * 2 - 1) * 0.4
    dirs = torch.nn.functional.normalize(torch.randn(50, 3, generator=gen, dtype=torch.float64), dim=-1)
    G_raw = torch.randn(50, 9 + Cf, generator=gen, dtype=torch.float64)
    e27 = O.freq_encode(dirs, 4)
    got, keep = _forward(blob, lay, D, skip, enc.numpy(), e27.numpy())
    e = enc.clone().requires_grad_()
    ref = O.field_forward(G.oracle_params(fine, torch.float64), torch.cat([e, e27], 1), in_xyz=32, D=D, skip=4)
    np.testing.assert_allclose(got, ref.detach().numpy(), rtol=1e-5, atol=1e-5 * float(ref.detach().abs().max()))
    (g_ref,) = torch.autograd.grad((ref * G_raw).sum(), e)
    g_got = _backward(blob, lay, Wd, D, skip, Cf, got, keep, G_raw.numpy())
    np.testing.assert_allclose(g_got, g_ref.numpy(), rtol=0, atol=1e-5 * float(g_ref.abs().max()))
    # against the frequency blob of the same shape: layer 1 and the skip layer lose 64 - 32 embedding rows, in both copies
    lib = L.load()
    freq = int(lib.nefes_generic_blob_bytes(L.NefesGenericNetDesc(Wd, D, skip, Cf, 1)))
    dropped = (64 - 32) * Wd * 2 * 4 * (2 if skip > 0 else 1)
    assert freq - blob.size * 4 == dropped
    n = 50
    assert lib.nefes_generic_mask_bytes(L.NefesGenericNetDesc(Wd, D, skip, Cf, 1, L.XYZ_EXTERNAL32), n) == \
        lib.nefes_generic_mask_bytes(L.NefesGenericNetDesc(Wd, D, skip, Cf, 1), n) > 0


def test_five_positional_values_still_mean_the_frequency_embedding():
    d = L.NefesGenericNetDesc(64, 6, 4, 16, 1)
    assert d.xyz_encoding == L.XYZ_FREQ10 == 0 and L.XYZ_EXTERNAL32 == 1
    assert C.sizeof(L.NefesGenericNetDesc) == 24
    assert L.ABI_VERSION == 20 == L.load().nefes_version()


def test_refusals_without_a_device():
    """Every refusal below is decided before a launch: the pointers are never read."""
    lib = L.load()
    p = C.c_void_p(16)
    freq, ext = L.NefesGenericNetDesc(64, 6, 4, 16, 1), L.NefesGenericNetDesc(64, 6, 4, 16, 1, L.XYZ_EXTERNAL32)
    U, BAD = -2, -1
    # an ext description into the entry points that take positions
    assert lib.nefes_field_fwd_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, None, p, p, None, None) == U
    assert lib.nefes_field_bwd_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, None, p, p, p, p, p, p, None) == U
    assert lib.nefes_field_fwd_train_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, p, None) == U
    assert lib.nefes_field_bwd_train_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, p, p, p, p, None) == U
    # a frequency description into the _ext entry points
    assert lib.nefes_field_fwd_generic_ext(freq, p, L.FIELD_FULL, 1, 1, p, p, p, None, None) == U
    assert lib.nefes_field_bwd_generic_ext(freq, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, None) == U
    # no train instances on a supplied encoding
    assert lib.nefes_generic_train_rows(ext) == 0 and lib.nefes_generic_train_rows(freq) > 0
    assert lib.nefes_generic_train_row_offset(ext, L.TB_END) == U and lib.nefes_generic_train_row_offset(freq, L.TB_END) > 0
    # an encoding that does not exist, and the shapes neither encoding has
    for bad in (L.NefesGenericNetDesc(64, 6, 4, 16, 1, 2), L.NefesGenericNetDesc(64, 6, 4, 16, 1, -1),
                L.NefesGenericNetDesc(48, 8, 4, 16, 1, 1), L.NefesGenericNetDesc(64, 9, 4, 16, 1, 1)):
        assert lib.nefes_generic_blob_bytes(bad) == 0 and lib.nefes_generic_mask_bytes(bad, 100) == 0
        assert lib.nefes_generic_pack(bad, None, 0, None, 0) == U
        assert lib.nefes_field_fwd_generic_ext(bad, p, L.FIELD_FULL, 1, 1, p, p, p, None, None) == U
        assert lib.nefes_field_bwd_generic_ext(bad, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, None) == U
    # null required pointers, modes the calls do not have
    assert lib.nefes_field_fwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, None, p, p, None, None) == BAD          # xyz_enc
    assert lib.nefes_field_fwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, p, None, p, None, None) == BAD          # viewdirs, not sigma
    assert lib.nefes_field_fwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, p, p, None, None, None) == BAD          # raw_t
    assert lib.nefes_field_fwd_generic_ext(ext, None, L.FIELD_FULL, 1, 1, p, p, p, None, None) == BAD          # packed
    assert lib.nefes_field_fwd_generic_ext(ext, p, 7, 1, 1, p, p, p, None, None) == BAD
    assert lib.nefes_field_fwd_generic_ext(ext, p, L.FIELD_FULL, 0, 1, p, p, p, None, None) == BAD
    assert lib.nefes_field_fwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, C.c_void_p(8), p, p, None, None) == BAD   # 16-byte loads
    coarse = L.NefesGenericNetDesc(64, 6, 4, 16, 0, L.XYZ_EXTERNAL32)
    assert lib.nefes_field_fwd_generic_ext(coarse, p, L.FIELD_FULL, 1, 1, p, p, p, None, None) == BAD          # no transient head
    for hole in range(6):                                                  # viewdirs, raw_t, g_raw_t, masks, g_xyz_enc, g_viewdirs_s
        args = [p] * 6
        args[hole] = None
        assert lib.nefes_field_bwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, *args, None) == BAD, hole
    assert lib.nefes_field_bwd_generic_ext(ext, p, L.FIELD_SIGMA, 1, 1, p, p, p, p, p, p, None) == BAD
    assert lib.nefes_field_bwd_generic_ext(ext, p, L.FIELD_FULL, 1, 1, p, p, p, p, C.c_void_p(8), p, None) == BAD


def _mock_pack(width, feat_dim, has_transient, enc):
    """tools/make_golden_field_routes.py generic_pack, with the encoding as an argument."""
    return types.SimpleNamespace(width=width, depth=8, skip=4, feat_dim=feat_dim, xyz_encoding=enc, has_transient=has_transient,
                                 h3_valid=False, fold=False, generic=True)


@pytest.mark.parametrize("width,feat_dim", [(64, 16), (128, 128), (256, 16)])
def test_routes_of_a_generic_pack_on_a_supplied_encoding(width, feat_dim):
    from nefes_amd import ops
    pk = _mock_pack(width, feat_dim, True, L.XYZ_EXTERNAL32)
    for mode, name in ((L.FIELD_SIGMA, "sigma"), (L.FIELD_STATIC, "static"), (L.FIELD_FULL, "full")):
        for M in (1, 1 << 20, ops.H3_MAX_SAMPLES + 5):
            rt = ops.field_route(pk, mode, False, "enc", M)
            assert rt == ops.Route("nefes_field_fwd_generic_ext", f"field_fwd[{name},generic,ext]", "nefes_field_fwd_generic_ext", False)
            rt = ops.field_route(pk, mode, True, "enc", M)
            assert rt == ops.Route("nefes_field_bwd_generic_ext", f"field_bwd[{name},generic,ext]", "nefes_field_bwd_generic_ext", True)
        for kind in ("rays", "points", "hashgrid", "zrow"):
            for backward in (False, True):
                with pytest.raises(RuntimeError, match=f"W={width}, D=8, f_dim={feat_dim}.*supplied 32-feature encoding.*'{kind}'"):
                    ops.field_route(pk, mode, backward, kind, 1000)
    freq = _mock_pack(width, feat_dim, True, L.XYZ_FREQ10)
    for backward in (False, True):
        with pytest.raises(RuntimeError, match=f"W={width}, D=8, f_dim={feat_dim}.*frequency embedding.*'enc'"):
            ops.field_route(freq, L.FIELD_FULL, backward, "enc", 1000)
        assert ops.field_route(freq, L.FIELD_FULL, backward, "rays", 1000).entry == f"nefes_field_{'bwd' if backward else 'fwd'}_generic"
        assert not ops.field_route(freq, L.FIELD_FULL, backward, "points", 1000).g_enc
    for name in ("nefes_field_fwd_generic_ext", "nefes_field_bwd_generic_ext"):
        assert name in L.SIGNATURES and hasattr(L.load(), name)


@pytest.mark.parametrize("Wd,D,ext,tuned", [(64, 6, True, False), (128, 8, True, False), (256, 8, True, True), (512, 8, True, False),
                                            (48, 8, False, False), (64, 9, False, False)])
def test_predicates_on_32_inputs(Wd, D, ext, tuned, monkeypatch):
    from nefes_amd import ops
    from nefes_amd.field import NeRFH_NFF
    net = NeRFH_NFF('fine', D=D, W=Wd, f_dim=16, in_channels_xyz=32, encode_transient=True)
    assert net._generic_ext_supported() == ext
    assert not net._generic_supported()                      # keeps its meaning: the frequency embedding
    assert net._supported() == tuned
    for flag in (False, True):                               # NEFES_FIELD_GENERIC does not redirect a tuned hash-grid network
        monkeypatch.setattr(ops, "FIELD_GENERIC", flag)
        assert net.uses_generic() == (not tuned)
    if not ext:
        with pytest.raises(RuntimeError, match=f"D={D}.*W={Wd}.*in_channels_xyz=32"):
            net.packed_generic()
    # the frequency embedding's predicate is not widened either
    freq = NeRFH_NFF('fine', D=D, W=Wd, f_dim=16, encode_transient=True)
    assert not freq._generic_ext_supported()
    assert not NeRFH_NFF('fine', D=6, W=64, f_dim=16, in_channels_xyz=32, in_channels_dir=26)._generic_ext_supported()
    assert not NeRFH_NFF('fine', D=6, W=64, f_dim=142, in_channels_xyz=32)._generic_ext_supported()


def test_packed_still_serves_the_tuned_instances_only():
    from nefes_amd.field import NeRFH_NFF
    net = NeRFH_NFF('fine', D=8, W=128, f_dim=128, in_channels_xyz=32, encode_transient=True)
    with pytest.raises(RuntimeError, match="W=128.*in_channels_xyz=32.*Compiled: fp16 two-part instances.*external 32-feature embedding"):
        net.packed()
    assert "NEFES_GENERIC_TRAIN" in L.GENERIC_SET and "frozen weights only" in L.GENERIC_SET
