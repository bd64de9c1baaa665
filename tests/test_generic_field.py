"""Generic field kernels (nefes_amd/csrc/field_generic.hip), host side: the packer's layout against a numpy restatement of the
kernels' addressing, the routing between tuned and generic packs, checkpoints saved under --multi_gpu, and the new kernels in the
shipped library's disassembly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from oracle import ref_cpu as O
from tests import generic_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack(net):
    from nefes_amd import ops
    lib = L.load()
    skip = 4 if net.D > 4 else -1
    desc = L.NefesGenericNetDesc(net.W, net.D, skip, net.W_features, 1 if net.encode_transient else 0)
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


def _layers(Wd, D, skip, Cf, fine):
    """csrc/field_generic.hip gen_layout restated: [(tag, M, Mp, Kp, wt, wb, bias)] in floats."""
    H = Wd // 2
    spec = [(f"L{i + 1}", Wd, 64 if i == 0 else (64 + Wd if i == skip else Wd)) for i in range(D)]
    spec += [("FINAL", Wd, Wd), ("SIGMA", 1, Wd), ("DIR", H, Wd + 32), ("RGB", 3 + Cf, H)]
    if fine:
        spec += [("T0", H, Wd + 32), ("T1", H, H), ("T2", H, H), ("TH", 5, H)]
    out, off = {}, 0
    for tag, M, Kp in spec:
        Mp = (M + 31) // 32 * 32
        out[tag] = (M, Mp, Kp, off, off + Kp * Mp, off + 2 * Kp * Mp)
        off += 2 * Kp * Mp + Mp
    return out, off + 64


def _emulate(blob, lay, Wd, D, skip, Cf, e63, e27, full):
    """The forward as the kernel addresses the blob: out[m] = bias[m] + sum_k wt[k * Mp + m] in[k] over the K-segments, embeddings padded
    to 64 / 32 rows."""
    n = e63.shape[0]
    E = np.zeros((64, n), np.float64); E[:63] = e63.T
    DV = np.zeros((32, n), np.float64); DV[:27] = e27.T

    def prod(tag, x):
        M, Mp, Kp, wt, wb, bias = lay[tag]
        assert x.shape[0] == Kp
        w = blob[wt:wt + Kp * Mp].reshape(Kp, Mp).astype(np.float64)
        wbm = blob[wb:wb + Kp * Mp].reshape(Mp, Kp)
        np.testing.assert_array_equal(wbm.T, blob[wt:wt + Kp * Mp].reshape(Kp, Mp))     # the backward's copy is the transpose
        return (w.T @ x + blob[bias:bias + Mp].astype(np.float64)[:, None])[:M]

    h = np.maximum(prod("L1", E), 0)
    for i in range(1, D):
        h = np.maximum(prod(f"L{i + 1}", np.concatenate([E, h]) if i == skip else h), 0)
    softplus = lambda x: np.log1p(np.exp(x))
    sigma = softplus(prod("SIGMA", h))
    fin = prod("FINAL", h)
    g = np.maximum(prod("DIR", np.concatenate([fin, DV])), 0)
    out = [prod("RGB", g), sigma]
    if full:
        t = np.maximum(prod("T0", np.concatenate([fin, DV])), 0)
        t = np.maximum(prod("T1", t), 0)
        t = np.maximum(prod("T2", t), 0)
        th = prod("TH", t)
        out += [1 / (1 + np.exp(-th[:3])), softplus(th[3:4]), softplus(th[4:5])]
    return np.concatenate(out).T


@pytest.mark.parametrize("Wd,D,Cf", [(64, 6, 16), (96, 5, 128), (32, 1, 16), (128, 4, 141), (192, 8, 16)])
def test_generic_pack_reproduces_the_mlp(Wd, D, Cf):
    _, fine = G.modules(Wd, D, Cf)
    blob, skip = _pack(fine)
    lay, total = _layers(Wd, D, skip, Cf, True)
    assert total == blob.size
    gen = torch.Generator().manual_seed(3)
    pts = (torch.rand(9, 3, generator=gen) - .5) * 4
    dirs = torch.nn.functional.normalize(torch.randn(9, 3, generator=gen), dim=-1)
    e63, e27 = O.freq_encode(pts.double(), 10), O.freq_encode(dirs.double(), 4)
    got = _emulate(blob, lay, Wd, D, skip, Cf, e63.numpy(), e27.numpy(), True)
    ref = O.field_forward(G.oracle_params(fine, torch.float64), torch.cat([e63, e27], 1), D=D, skip=4).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-10)


def test_generic_pack_refuses_bad_shapes():
    lib = L.load()
    for (Wd, D, skip, Cf) in [(48, 8, 4, 16), (64, 9, 4, 16), (544, 8, 4, 16), (64, 6, 6, 16), (64, 6, 4, 0), (64, 6, 4, 142), (0, 1, -1, 16)]:
        desc = L.NefesGenericNetDesc(Wd, D, skip, Cf, 1)
        assert lib.nefes_generic_blob_bytes(desc) == 0
        assert lib.nefes_generic_mask_bytes(desc, 1000) == 0
        assert lib.nefes_generic_pack(desc, None, 0, None, 0) == -2
        assert lib.nefes_field_fwd_generic(desc, C.c_void_p(8), 0, 1, 1, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None, None,
                                           C.c_void_p(8), None, None) == -2


@pytest.mark.parametrize("Wd,D,Cf,tuned,generic", [
    (256, 8, 16, True, True), (128, 8, 128, True, True), (256, 8, 141, True, True), (64, 6, 16, False, True), (192, 8, 128, False, True),
    (512, 8, 16, False, True), (128, 4, 16, False, True), (256, 2, 16, False, True), (96, 5, 16, False, True), (32, 1, 128, False, True),
    (48, 8, 16, False, False), (64, 9, 16, False, False), (544, 8, 16, False, False), (64, 6, 142, False, False)])
def test_routing_decisions(Wd, D, Cf, tuned, generic, monkeypatch):
    from nefes_amd import ops
    from nefes_amd.field import NeRFH_NFF
    net = NeRFH_NFF('fine', D=D, W=Wd, f_dim=Cf, encode_transient=True)
    assert net._supported() == tuned and net._generic_supported() == generic
    monkeypatch.setattr(ops, "FIELD_GENERIC", False)
    assert net.uses_generic() == (not tuned)
    monkeypatch.setattr(ops, "FIELD_GENERIC", True)
    assert net.uses_generic() == (generic or not tuned)
    if not tuned and not generic:
        with pytest.raises(RuntimeError, match=f"D={D}.*W={Wd}.*f_dim={Cf}"):
            net.packed_generic()
    if not tuned:                       # packed() keeps serving the tuned instances only
        with pytest.raises(RuntimeError, match=f"W={Wd}.*Compiled: fp16 two-part instances"):
            net.packed()


def test_external_encoding_and_reduce_mode_2_stay_out():
    from nefes_amd.field import NeRFH_NFF, get_embedder
    assert not NeRFH_NFF('coarse', D=6, W=64, in_channels_xyz=32, f_dim=16)._generic_supported()
    with pytest.raises(NotImplementedError, match="reduce_embedding=2"):
        get_embedder(10, 0, 2)


def test_module_prefixed_checkpoint_loads(tmp_path, monkeypatch):
    """--multi_gpu checkpoints carry `module.` in front of every key (run_nefes.py:378-382)."""
    from nefes_amd.field import NeRFH_NFF, strip_module_prefix
    src = NeRFH_NFF('fine', D=6, W=64, f_dim=16, encode_transient=True)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.25)
    sd = {"module." + k: v for k, v in src.state_dict().items()}
    dst = NeRFH_NFF('fine', D=6, W=64, f_dim=16, encode_transient=True)
    dst.load_state_dict(strip_module_prefix(sd))
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    plain = src.state_dict()
    assert strip_module_prefix(plain) is plain


def test_generic_kernels_are_in_the_library_and_clean(tmp_path):
    """The library's gfx950 code holds the sixteen generic kernels; they use the fp32 MFMA, no scratch and no packed-fp32
    op_sel:[0,1] form and tools/hazard_lint.py has no finding in them (the library-wide checks of
    tests/test_hazard_lint.py and tests/test_pack_stream.py read them too)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hazard_lint as H
    tools = [os.path.join(H.BIN, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not installed")
    viol, kernels, insts = H.lint(L.LIB_PATH)
    assert kernels > 150
    assert not [v for v in viol if " gen_fwd_kernel<" in v[0] or " gen_bwd_kernel<" in v[0]]
    fat = tmp_path / "fatbin.bin"
    subprocess.check_call([tools[0], "-O", "binary", "--only-section=.hip_fatbin", L.LIB_PATH, str(fat)])
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    seen, mfma, bad = set(), 0, []
    for i, a in enumerate(starts):
        piece = tmp_path / f"bundle{i}.bin"
        piece.write_bytes(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        if b"gen_fwd_kernel" not in piece.read_bytes():
            continue
        co = tmp_path / f"code{i}.o"
        subprocess.check_call([tools[1], "--unbundle", "--type=o", f"--input={piece}", f"--output={co}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], stderr=subprocess.DEVNULL)
        if co.stat().st_size == 0:
            continue
        dis = subprocess.run([tools[2], "-d", "-C", "--no-show-raw-insn", str(co)], capture_output=True, text=True, check=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
                continue
            if name and (" gen_fwd_kernel<" in name or " gen_bwd_kernel<" in name):
                seen.add(name.split("(")[0])
                mfma += "v_mfma_f32_32x32x2_f32" in line
                if re.search(r"v_pk_(mul|add|fma)_f32\b.*op_sel:\[0,1", line) or "scratch_" in line:
                    bad.append((name[:60], line.strip()))
    assert len(seen) == 16, seen
    assert mfma > 100 and not bad, (mfma, bad[:4])
