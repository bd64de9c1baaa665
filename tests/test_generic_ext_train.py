"""Train mode of the generic field kernels on a SUPPLIED 32-feature encoding (csrc/field_generic.hip gen_{fwd,bwd}_kernel<NCB,
GenArgsExtTrain>, nefes_field_{fwd,bwd}_train_generic_ext), the part a CPU can check: the row map of the acts / dacts buffers against the frequency
map of the same shape, the argument checks of the two calls, the library surface and the opt-in switch, and the fp32 oracle on the
fixture the reference itself produced (tools/make_golden_generic_ext_train.py), so that the fixture is checked without a GPU too."""
import ctypes as C

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from oracle import ref_cpu as O
from tests import generic_util as G

# (W, D, C) of tests/test_gpu_generic_ext.py SHAPES (tests/test_gpu_generic_ext_train.py asserts that the two lists agree)
SHAPES = [(64, 6, 16), (128, 8, 128), (128, 4, 30), (32, 1, 16), (320, 7, 29), (512, 8, 16), (96, 5, 141)]
U, BAD = -2, -1
GOLDEN_TAGS = ["w64d6c16", "w96d5c128"]


def _descs(W, D, C_, fine):
    skip = 4 if D > 4 else -1
    return (L.NefesGenericNetDesc(W, D, skip, C_, 1 if fine else 0),
            L.NefesGenericNetDesc(W, D, skip, C_, 1 if fine else 0, L.XYZ_EXTERNAL32))


@pytest.mark.parametrize("fine", [False, True])
@pytest.mark.parametrize("W,D,C_", SHAPES)
def test_row_map_of_a_supplied_encoding(W, D, C_, fine):
    """The E block is the 32 supplied features: blocks up to E start where the frequency map has them, every later one 32 rows earlier."""
    lib = L.load()
    freq, ext = _descs(W, D, C_, fine)
    blocks = range(L.TB_END + 1)
    rows_f = int(lib.nefes_generic_train_rows(freq))
    off_f = [int(lib.nefes_generic_train_row_offset(freq, b)) for b in blocks]
    rows_x = int(lib.nefes_generic_train_rows_ext(ext))
    off_x = [int(lib.nefes_generic_train_row_offset_ext(ext, b)) for b in blocks]
    assert rows_f > 0 and rows_x == rows_f - 32 == off_x[L.TB_END]
    for b in blocks:
        assert off_x[b] == (off_f[b] if b <= L.TB_E else off_f[b] - 32), (b, off_x, off_f)
        assert off_x[b] % 32 == 0
    assert off_x[L.TB_E] == 0 and off_x[L.TB_DV] == 32 and off_x[L.TB_L1] == 64
    assert all((off_x[b + 1] - off_x[b]) % 32 == 0 and off_x[b + 1] >= off_x[b] for b in range(L.TB_END))
    # each pair serves one encoding
    assert lib.nefes_generic_train_rows_ext(freq) == 0
    assert all(lib.nefes_generic_train_row_offset_ext(freq, b) == U for b in blocks)
    assert lib.nefes_generic_train_rows(ext) == 0
    assert all(lib.nefes_generic_train_row_offset(ext, b) == U for b in blocks)
    for pair, d in ((lib.nefes_generic_train_row_offset_ext, ext), (lib.nefes_generic_train_row_offset, freq)):
        assert pair(d, -1) == BAD and pair(d, L.TB_END + 1) == BAD
    # the old pair on the frequency description, restated: E 64, DV 32, then the layers
    assert off_f[L.TB_E] == 0 and off_f[L.TB_DV] == 64 and off_f[L.TB_L1] == 96 and off_f[L.TB_END] == rows_f
    bad = L.NefesGenericNetDesc(48, 6, 4, 16, 1, L.XYZ_EXTERNAL32)
    assert lib.nefes_generic_train_rows_ext(bad) == 0 and lib.nefes_generic_train_row_offset_ext(bad, 0) == U


def test_entry_points_refuse_before_any_launch():
    """Every refusal below is decided on the host: the pointers are dummies that are never read."""
    lib = L.load()
    p = C.c_void_p(4096)
    freq, ext = _descs(64, 6, 16, True)
    _, coarse = _descs(64, 6, 16, False)
    fwd_names = ("packed", "xyz_enc", "viewdirs", "raw_t", "acts", "masks")
    bwd_names = ("packed", "viewdirs", "raw_t", "g_raw_t", "masks", "dacts", "g_xyz_enc", "g_viewdirs_s")

    def fwd(desc, mode, N=2, S=8, **a):
        v = [a.get(k, p) for k in fwd_names]
        return lib.nefes_field_fwd_train_generic_ext(desc, v[0], mode, N, S, *v[1:], None)

    def bwd(desc, mode, N=2, S=8, **a):
        v = [a.get(k, p) for k in bwd_names]
        return lib.nefes_field_bwd_train_generic_ext(desc, v[0], mode, N, S, *v[1:], None)

    for call, names in ((fwd, fwd_names), (bwd, bwd_names)):
        for k in names:
            assert call(ext, L.FIELD_FULL, **{k: None}) == BAD, k
        assert call(ext, L.FIELD_SIGMA) == BAD and call(ext, 7) == BAD
        assert call(coarse, L.FIELD_FULL) == BAD                               # FULL without a transient head
        assert call(ext, L.FIELD_FULL, N=0) == BAD and call(ext, L.FIELD_FULL, S=0) == BAD
        assert call(freq, L.FIELD_FULL) == U and call(freq, L.FIELD_STATIC) == U
        assert call(L.NefesGenericNetDesc(48, 6, 4, 16, 1, L.XYZ_EXTERNAL32), L.FIELD_FULL) == U
    off4 = C.c_void_p(4096 + 4)                                                # 16-byte loads and stores
    assert fwd(ext, L.FIELD_FULL, xyz_enc=off4) == BAD and fwd(coarse, L.FIELD_STATIC, xyz_enc=off4) == BAD
    assert bwd(ext, L.FIELD_FULL, g_xyz_enc=off4) == BAD and bwd(coarse, L.FIELD_STATIC, g_xyz_enc=off4) == BAD
    assert fwd(ext, L.FIELD_FULL, acts=off4) == BAD and bwd(ext, L.FIELD_FULL, dacts=off4) == BAD
    # the frequency train pair keeps refusing an ext description
    assert lib.nefes_field_fwd_train_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, p, None) == U
    assert lib.nefes_field_bwd_train_generic(ext, p, L.FIELD_FULL, 1, 1, p, p, p, p, p, p, p, p, p, p, None) == U


# Pointer arguments of the eight generic entry points behind (desc, packed, mode, N, S), in order; the stream follows.
ENTRY_PTRS = {
    "fwd_generic": ("rays_o", "rays_d", "z", "pts", "viewdirs", "raw_t", "masks"),
    "bwd_generic": ("rays_o", "rays_d", "z", "pts", "viewdirs", "raw_t", "g_raw_t", "masks", "g_pts", "g_viewdirs_s"),
    "fwd_generic_ext": ("xyz_enc", "viewdirs", "raw_t", "masks"),
    "bwd_generic_ext": ("viewdirs", "raw_t", "g_raw_t", "masks", "g_xyz_enc", "g_viewdirs_s"),
    "fwd_train_generic": ("rays_o", "rays_d", "z", "viewdirs", "raw_t", "acts", "masks"),
    "bwd_train_generic": ("rays_o", "rays_d", "z", "viewdirs", "raw_t", "g_raw_t", "masks", "dacts", "g_pts", "g_viewdirs_s"),
    "fwd_train_generic_ext": ("xyz_enc", "viewdirs", "raw_t", "acts", "masks"),
    "bwd_train_generic_ext": ("viewdirs", "raw_t", "g_raw_t", "masks", "dacts", "g_xyz_enc", "g_viewdirs_s"),
}
EXT_ENTRIES = {"fwd_generic_ext": "xyz_enc", "bwd_generic_ext": "g_xyz_enc", "fwd_train_generic_ext": "xyz_enc",
               "bwd_train_generic_ext": "g_xyz_enc"}      # entry -> the pointer it moves as float4
TRAIN_BUF = {"fwd_train_generic_ext": "acts", "bwd_train_generic_ext": "dacts"}


def _precedence_cases():
    """(entry, description, mode, {pointer: "off4" | None}, expected): TWO reasons to refuse in every call, so which code comes back
    says which test runs first.  `other` = a valid description of the encoding the entry point does not serve, `width48` = an invalid
    one of its own encoding, `other_coarse` = `other` without the transient head."""
    out = []
    for e in ENTRY_PTRS:
        train, ext = "train" in e, e in EXT_ENTRIES
        # the entry point's own test (null, mode of a train call, SIGMA into a backward) comes first ...
        out.append((e, "other", L.FIELD_FULL, {"packed": None}, BAD))
        out.append((e, "width48", 7, {}, BAD if train else U))                   # ... then the description, then the mode
        out.append((e, "other", 7, {}, BAD if train else U))
        out.append((e, "other_coarse", L.FIELD_FULL, {}, U))                     # encoding before FULL-without-the-head
        if e != "fwd_generic" and e != "fwd_generic_ext":
            out.append((e, "other", L.FIELD_SIGMA, {}, BAD))
        if ext:                                                                    # alignment last
            out.append((e, "other", L.FIELD_FULL, {EXT_ENTRIES[e]: "off4"}, U))
            out.append((e, "width48", L.FIELD_FULL, {EXT_ENTRIES[e]: "off4"}, U))
            out.append((e, "own_coarse", L.FIELD_FULL, {EXT_ENTRIES[e]: "off4"}, BAD))
            out.append((e, "own", 7, {EXT_ENTRIES[e]: "off4"}, BAD))
        if e in TRAIN_BUF:
            out.append((e, "other", L.FIELD_FULL, {TRAIN_BUF[e]: "off4"}, U))
            out.append((e, "width48", L.FIELD_STATIC, {TRAIN_BUF[e]: "off4"}, U))
    return out


@pytest.mark.parametrize("entry,desc,mode,ptrs,expected", _precedence_cases(),
                         ids=[f"{e}-{d}-mode{m}-" + ",".join(f"{k}={x}" for k, x in p.items()) for e, d, m, p, _ in _precedence_cases()])
def test_refusal_precedence_of_every_entry_point(entry, desc, mode, ptrs, expected):
    """The order of the refusals of the eight entry points, where two apply at once: the call's own null / size / mode test, then the
    description (invalid, or of the other encoding: UNSUPPORTED), then the mode and FULL without a transient head, then the row map,
    then the alignment of a supplied encoding's buffers.  The expected codes are what the library returned before the entry points
    shared one launcher.  Every call is refused on the host: the pointers are dummies that are never read."""
    lib = L.load()
    ext = entry in EXT_ENTRIES
    enc = {True: L.XYZ_EXTERNAL32, False: L.XYZ_FREQ10}
    d = {"own": L.NefesGenericNetDesc(64, 6, 4, 16, 1, enc[ext]), "own_coarse": L.NefesGenericNetDesc(64, 6, 4, 16, 0, enc[ext]),
         "other": L.NefesGenericNetDesc(64, 6, 4, 16, 1, enc[not ext]), "other_coarse": L.NefesGenericNetDesc(64, 6, 4, 16, 0, enc[not ext]),
         "width48": L.NefesGenericNetDesc(48, 6, 4, 16, 1, enc[ext])}[desc]
    p = {"off4": C.c_void_p(4096 + 4), None: None}
    args = [p[ptrs[k]] if k in ptrs else C.c_void_p(4096) for k in ("packed",) + ENTRY_PTRS[entry]]
    assert getattr(lib, "nefes_field_" + entry)(d, args[0], mode, 2, 8, *args[1:], None) == expected


def test_library_surface_and_switch():
    from nefes_amd import ops
    from nefes_amd import train as TR
    lib = L.load()
    for name in ("nefes_generic_train_rows_ext", "nefes_generic_train_row_offset_ext", "nefes_field_fwd_train_generic_ext",
                 "nefes_field_bwd_train_generic_ext"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["nefes_field_fwd_train_generic_ext"][1]) == 11
    assert len(L.SIGNATURES["nefes_field_bwd_train_generic_ext"][1]) == 13
    assert L.ABI_VERSION == 20 == lib.nefes_version()
    assert ops.GENERIC_TRAIN_EXT is False and ops.GENERIC_TRAIN is False
    assert "NEFES_GENERIC_TRAIN_EXT" in L.GENERIC_SET and "frozen weights only" in L.GENERIC_SET
    assert callable(TR.field_train_generic_encoded) and issubclass(TR.FieldTrainGenericEncoded, torch.autograd.Function)


def test_refusal_names_both_switches():
    from nefes_amd.field import NeRFH_NFF
    net = NeRFH_NFF('fine', D=6, W=64, f_dim=16, in_channels_xyz=32, encode_transient=True)
    with pytest.raises(NotImplementedError, match=r"train mode.*D=6.*W=64.*in_channels_xyz=32.*NEFES_GENERIC_TRAIN=1.*NEFES_GENERIC_TRAIN_EXT=1"):
        net.require_frozen_for_generic("train mode (weight gradients)")


# ---- the reference's fixture ------------------------------------------------------------------------------------------------------
def golden_case(g, tag, device=None):
    """-> (the network of the fixture's case with trainable field weights, its checksums verified; enc [N,S,32], viewdirs [N,3],
    G [N,R,S] as torch tensors; the case's dict of reference arrays by short name)."""
    t = f"get.{tag}."
    Wd, D, C_, fine, N, S = (int(x) for x in g[t + "cfg"])
    coarse, fine_net = G.modules(Wd, D, C_, in_xyz=32, device=device)
    net = fine_net if fine else coarse
    ref = {k[len(t):]: v for k, v in g.items() if k.startswith(t)}
    for k, v in net.state_dict().items():                                # the seed reproduces the reference's parameters
        if "sum." + k in ref:
            v = v.cpu()
            np.testing.assert_allclose(np.array([v.double().sum().item(), v.double().abs().sum().item(), float(v.flatten()[0])]),
                                       ref["sum." + k], rtol=0, atol=0, err_msg=k)
    names = [n for n, _ in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]
    assert sorted(names) == sorted(k[len("grad."):] for k in ref if k.startswith("grad."))     # every parameter's gradient is stored
    for n, p in net.named_parameters():
        p.requires_grad_(n in names)
    enc = torch.from_numpy(ref["enc"]).reshape(N, S, 32)
    v = torch.from_numpy(ref["viewdirs"])
    G_up = torch.from_numpy(ref["G"]).reshape(N, S, -1).permute(0, 2, 1).contiguous()
    return net, (Wd, D, C_, bool(fine), N, S), enc, v, G_up, ref


def oracle_on_case(net, D, fine, enc, v, G_up, dt):
    """The oracle's field on the fixture's inputs -> raw [M, R], {parameter: gradient}, d enc [M, 32], d viewdirs [N, 3] of sum(raw G)."""
    N, S = enc.shape[:2]
    p = {n: t.detach().cpu().to(dt).clone().requires_grad_(t.requires_grad) for n, t in net.named_parameters()
         if not n.startswith(("fusion_net", "exposure_embedding"))}
    e = enc.reshape(-1, 32).to(dt).clone().requires_grad_()
    vv = v.to(dt).clone().requires_grad_()
    ed = O.freq_encode(vv[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    raw = O.field_forward(p, torch.cat([e, ed], 1), output_transient=fine, in_xyz=32, D=D, skip=4)
    (raw * G_up.permute(0, 2, 1).reshape(N * S, -1).to(dt)).sum().backward()
    return raw.detach(), {n: t.grad for n, t in p.items()}, e.grad, vv.grad


def reference_input_grads(ref, v, N, S):
    """The reference's d x [M, 59] as (d enc [M, 32], d viewdirs [N, 3]): the direction columns through the embedding's own chain."""
    dx = torch.from_numpy(ref["dx"]).double()
    vv = v.double().clone().requires_grad_()
    ed = O.freq_encode(vv[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    (g_v,) = torch.autograd.grad(ed, vv, grad_outputs=dx[:, 32:])
    return dx[:, :32], g_v


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_fp32_oracle_on_the_reference_fixture(golden, tag):
    """The fp32 oracle is the reference's own arithmetic restated (same torch ops, same dtype): raw outputs within 2e-5 (the project's
    bound for raw_t), every parameter gradient and d x under the rules of the reference fixtures (1e-3 of the max-norm, cosine >
    0.9995).  The float64 oracle next to it gives e_ref for the record."""
    g = golden("generic_ext_train")
    net, (Wd, D, C_, fine, N, S), enc, v, G_up, ref = golden_case(g, tag)
    assert (N, S) == (5, 33) and ref["raw"].shape == (N * S, (9 if fine else 4) + C_) and ref["dx"].shape == (N * S, 59)
    raw32, g32, ge32, gv32 = oracle_on_case(net, D, fine, enc, v, G_up, torch.float32)
    raw64, g64, ge64, gv64 = oracle_on_case(net, D, fine, enc, v, G_up, torch.float64)
    e_raw = rel(raw32, ref["raw"])
    print(f"[generic_ext_train_golden[{tag}]] fp32 oracle raw vs the reference {e_raw:.2e}; reference vs float64 {rel(ref['raw'], raw64):.2e}")
    assert e_raw < 2e-5 and rel(ref["raw"], raw64) < 2e-5
    ref_ge, ref_gv = reference_input_grads(ref, v, N, S)
    pairs = [(n, g32[n], torch.from_numpy(ref["grad." + n])) for n in g32] + [("d enc", ge32, ref_ge), ("d viewdirs", gv32, ref_gv)]
    n_cmp = 0
    for name, a, b in pairs:
        assert a is not None and tuple(a.shape) == tuple(b.shape), name
        a, b = a.double().reshape(-1), b.double().reshape(-1)
        assert float(b.abs().max()) > 0, name
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))
        assert rel(a, b) < 1e-3 and cos > 0.9995, (name, rel(a, b), cos)
        n_cmp += 1
    assert n_cmp == 2 * (D + (10 if fine else 4)) + 2
