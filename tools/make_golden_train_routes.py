#!/usr/bin/env python3
"""Fixture of what the HOST does in train mode (nefes_amd/train.py): every C call with its arguments, every timer key, and the
mapping from the weight-gradient partials to named parameter gradients -- tests/golden/train_routes.json, replayed by
tests/test_train_routes.py.

Runs on the CPU.  L.load() hands out a proxy around the real library: the host queries (row maps, mask sizes) pass through, every
other call is recorded as `name(args)` and returns 0 -- ints verbatim, pointers as p / 0 (null), descriptors as D, by the argument
types of lib.SIGNATURES.  ops._timed records its key ("t:"), ops._stream returns None, ops._chk returns the tensor's address.  The
networks are real NeRFH_NFF modules on the CPU whose packed() / packed_generic() hand out a stand-in pack (a real descriptor, a
16-byte blob), and train._generic_buffers_fit, which asks the device, is a no-op.

The recorded nefes_train_dw_bias also FILLS its partials (they are host memory here): split 0 of the product's op * (ip + 1) floats
receives a counter that starts at 1 per backward and runs on through the products in launch order, every other split 0 -- all below
2^24, exact in fp32.  After backward() the outcome carries one sha256 over every parameter gradient in param_names order and the
count of gradients shaped like their parameter: the column offsets into the wide buffer, the embedding slices, the skip concatenation,
the 3 | 1 | 1 split of the transient head and shrink_grads are all in that digest.

Only names that the four Functions' callers use are called, so the same generator replays on any later revision; the fixture is
written from the revision BEFORE a change to train.py and must come out byte-identical after it.

Usage:  python tools/make_golden_train_routes.py [out.json]     (default: tests/golden/train_routes.json of the tree it is run in)
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nefes_amd import lib as L          # noqa: E402
from nefes_amd import ops               # noqa: E402
from nefes_amd import train as T        # noqa: E402
from nefes_amd import field as F        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_routes.json")
N, S = 3, 50                            # one full 128-sample tile and a ragged one (tools/ab_identical.py)
STATIC, FULL, SIGMA = L.FIELD_STATIC, L.FIELD_FULL, L.FIELD_SIGMA

PASS_THROUGH = {"nefes_train_rows", "nefes_train_row_offset", "nefes_generic_train_rows", "nefes_generic_train_row_offset",
                "nefes_generic_train_rows_ext", "nefes_generic_train_row_offset_ext", "nefes_field_mask_bytes", "nefes_generic_mask_bytes"}
SWITCHES = ((ops, "SPLIT"), (ops, "USE_X6"), (ops, "GENERIC_TRAIN"), (ops, "GENERIC_TRAIN_EXT"), (ops, "TAP"), (T, "FUSED_DX"), (T, "DEBUG"))
DEFAULTS = {"SPLIT": "h3", "USE_X6": True, "GENERIC_TRAIN": False, "GENERIC_TRAIN_EXT": False, "TAP": None, "FUSED_DX": True, "DEBUG": None}

EVENTS = []
COUNTER = [1]


def _is_null(a):
    if isinstance(a, C.c_void_p):
        a = a.value
    return a is None or a == 0


def _fill_dw(args):
    """the fake nefes_train_dw_bias: args = (n_tiles, rows, G, g_off, op, X, x_off, ip, relu, splits, split_stride, out, stream)"""
    op, ip, splits, stride, out = args[4], args[7], args[9], args[10], args[11]
    n = op * (ip + 1)
    for s in range(splits):
        dst = np.ctypeslib.as_array((C.c_float * n).from_address(out + 4 * s * stride))
        dst[:] = np.arange(COUNTER[0], COUNTER[0] + n, dtype=np.float32) if s == 0 else 0.
    COUNTER[0] += n
    assert COUNTER[0] < 1 << 24


class _Lib:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in PASS_THROUGH:
            return getattr(self._real, name)
        argtypes = L.SIGNATURES[name][1]

        def fn(*args):
            if len(args) != len(argtypes):
                raise TypeError(f"{name}: {len(args)} arguments for {len(argtypes)}")
            rec = []
            for a, t in zip(args, argtypes):
                if t is C.c_void_p:
                    rec.append("0" if _is_null(a) else "p")
                elif isinstance(t, type) and issubclass(t, C._Pointer):
                    rec.append("D")
                else:
                    rec.append(str(int(a)))
            EVENTS.append(f"{name}({','.join(rec)})")
            if name == "nefes_train_dw_bias":
                _fill_dw(args)
            return 0
        return fn


class _Timed:
    def __init__(self, name):
        EVENTS.append("t:" + name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@contextlib.contextmanager
def patched():
    """The replacements of the module docstring, undone on exit (the test suite shares the process)."""
    saved = (L.load, ops._chk, ops._stream, ops._timed, T._generic_buffers_fit, [getattr(m, k) for m, k in SWITCHES])
    lib = _Lib(L.load())
    L.load, ops._stream, ops._timed = (lambda: lib), (lambda: None), _Timed
    ops._chk = lambda t, name, dtype=None: None if t is None else t.data_ptr()
    T._generic_buffers_fit = lambda *a, **k: None
    try:
        yield
    finally:
        L.load, ops._chk, ops._stream, ops._timed, T._generic_buffers_fit = saved[:5]
        for (m, k), v in zip(SWITCHES, saved[5]):
            setattr(m, k, v)


def set_switches(sw):
    for m, k in SWITCHES:
        setattr(m, k, sw.get(k, DEFAULTS[k]))


# ------------------------------------------------------------------------------------------------------------------------------
# networks and stand-in packs
# ------------------------------------------------------------------------------------------------------------------------------
def tuned_pack(net, h3_valid=True):
    pk = object.__new__(ops.PackedField)
    enc = L.XYZ_EXTERNAL32 if net.in_channels_xyz == 32 else L.XYZ_FREQ10
    pk.desc = L.NefesNetDesc(net.W, net.W_features, int(net.encode_transient), enc, 0)
    pk.width, pk.feat_dim, pk.has_transient, pk.xyz_encoding, pk.fold = net.W, net.W_features, bool(net.encode_transient), enc, False
    pk.blob, pk.generation, pk.h3_valid = torch.zeros(16, dtype=torch.uint8), 0, h3_valid
    return pk


def generic_pack(net, ext=None):
    pk = object.__new__(ops.PackedGeneric)
    enc = L.XYZ_EXTERNAL32 if (net.in_channels_xyz == 32 if ext is None else ext) else L.XYZ_FREQ10
    skip = 4 if (4 in net.skips and net.D > 4) else -1
    pk.desc = L.NefesGenericNetDesc(net.W, net.D, skip, net.W_features, int(net.encode_transient), enc)
    pk.width, pk.depth, pk.skip, pk.feat_dim, pk.has_transient, pk.xyz_encoding = net.W, net.D, skip, net.W_features, bool(net.encode_transient), enc
    pk.blob, pk.generation, pk.tile = torch.zeros(16, dtype=torch.uint8), 0, 64 if net.W <= 256 else 32
    return pk


_NETS = {}


def network(W, C_, fine, D=8, xyz=63, dirs=27):
    """The (cached) CPU module; its packs are set per case."""
    key = (W, C_, fine, D, xyz, dirs)
    if key not in _NETS:
        _NETS[key] = F.NeRFH_NFF("fine" if fine else "coarse", D=D, W=W, f_dim=C_, encode_transient=bool(fine), in_channels_xyz=xyz,
                                 in_channels_dir=dirs)
    return _NETS[key]


def _field_params(net):
    return [p for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]


def prepare(net, frozen=False, h3_valid=True, generic_ext=None):
    for p in net.parameters():
        p.grad = None
    for p in _field_params(net):
        p.requires_grad_(not frozen)
    tp, gp = tuned_pack(net, h3_valid), generic_pack(net, generic_ext)
    net.packed, net.packed_generic = (lambda: tp), (lambda: gp)
    return net


def rays(grad=False, z_grad=False, device="cpu"):
    g = torch.Generator().manual_seed(3)
    mk = lambda *shape, gr=False: torch.rand(*shape, generator=g).to(device).requires_grad_(gr)
    return mk(N, 3, gr=grad), mk(N, 3, gr=grad), mk(N, 3, gr=grad), mk(N, S, gr=z_grad)


class _Grid:
    """An xyz encoder for field_train*_encoded: a fixed [N, S, 32] encoding that asks for a gradient."""

    def __call__(self, pts):
        self.enc = torch.zeros(pts.shape[0], pts.shape[1], 32, requires_grad=True)
        return self.enc


# ------------------------------------------------------------------------------------------------------------------------------
# one case: forward, backward, what came out
# ------------------------------------------------------------------------------------------------------------------------------
def grads_digest(net, mode, names_fn):
    names = names_fn(net, mode)
    sd = dict(net.named_parameters())
    h, same, have = hashlib.sha256(), 0, 0
    for n in names:
        g = sd[n].grad
        if g is None:
            h.update(b"-")
            continue
        have += 1
        same += int(g.shape == sd[n].shape)
        h.update(n.encode() + str(tuple(g.shape)).encode() + g.detach().contiguous().numpy().astype(np.float32).tobytes())
    return f"grads:{h.hexdigest()}:{same}/{have}/{len(names)}"


def run(call, net, mode, names_fn, sw):
    """call(net, mode) -> (raw_t, the inputs that may receive a gradient); backward with an upstream of ones when anything asks for a
    gradient.  -> the outcome's event list."""
    del EVENTS[:]
    COUNTER[0] = 1
    set_switches(sw)
    if sw.get("DEBUG") is not None:
        T.DEBUG, ops.TAP = {}, {}
    try:
        raw, inputs = call(net, mode)
        EVENTS.append(f"raw:{tuple(raw.shape)}")
        if raw.requires_grad:
            raw.backward(torch.ones_like(raw))
            EVENTS.append("in:" + "".join("-" if (t is None or t.grad is None) else str(len(t.grad.shape)) for t in inputs))
            EVENTS.append(grads_digest(net, mode, names_fn))
        if sw.get("DEBUG") is not None:
            d = T.DEBUG
            EVENTS.append(f"debug:{sorted(d)}:rows={d.get('rows')}:acts={tuple(d['acts'].shape)}:off={sorted(d.get('off', {}).items())}")
            EVENTS.append("tap:" + ";".join(f"{k}={[(a[1], a[2], a[3] if isinstance(a[3], int) else 'pk', a[4]) for a in v]}"
                                            for k, v in sorted(ops.TAP.items())))
    except Exception as e:       # noqa: BLE001  (the class name is the record)
        EVENTS.append("!" + type(e).__name__)
    return list(EVENTS)


def _sw_id(sw):
    return ",".join(f"{k}={'on' if (k == 'DEBUG' and sw[k] is not None) else sw[k]}" for k in sorted(sw)) or "defaults"


def cases():
    """Every case as (case id, thunk -> event list); run inside patched()."""
    out = []

    def add(cid, sw, net_args, mode, call, names_fn=None, **prep):
        def thunk():
            return run(call, prepare(network(*net_args[0], **net_args[1]), **prep), mode, names_fn or T.param_names, sw)
        out.append((f"{cid} | {_sw_id(sw)}", thunk))

    def by_rays(f, grad=False, z_grad=False):
        def call(net, mode):
            o, d, v, z = rays(grad, z_grad)
            return f(net, mode, o, d, v, z), (o, d, v, z)
        return call

    def by_grid(f, grad=False):
        def call(net, mode):
            o, d, v, z = rays(grad)
            grid = _Grid()
            raw = f(net, mode, grid, o, d, v, z)
            return raw, (grid.enc, v)
        return call

    def by_enc(Fn, names_fn, enc_grad=True, v_grad=True, shape=None, device="cpu"):
        def call(net, mode):
            sd = dict(net.named_parameters())
            enc = torch.zeros(*(shape or (N, S, 32)), device=device, requires_grad=enc_grad)
            v = torch.zeros(enc.shape[0], 3, device=device, requires_grad=v_grad)
            return Fn.apply(enc, v, net, mode, *[sd[n] for n in names_fn(net, mode)]), (enc, v)
        return call

    A = lambda *a, **k: (a, k)
    mname = {STATIC: "static", FULL: "full", SIGMA: "sigma"}
    # ---- tuned, frequency embedding ----
    shapes = ((128, 128), (256, 16), (256, 128), (128, 16))
    variants = (("coarse", 0, STATIC), ("fine", 1, FULL), ("fine", 1, STATIC))
    for (W, C_) in shapes:
        for typ, fine, mode in variants:
            for split in ("h3", "f32"):
                for g in (False, True):
                    add(f"tuned,W={W},C={C_},{typ},{mname[mode]},rays_grad={int(g)}", {"SPLIT": split}, A(W, C_, fine), mode,
                        by_rays(T.field_train, g))
        add(f"tuned,W={W},C={C_},fine,full,h3_valid=0", {"SPLIT": "h3"}, A(W, C_, 1), FULL, by_rays(T.field_train), h3_valid=False)
    add("tuned,W=256,C=16,fine,full,debug", {"DEBUG": 1}, A(256, 16, 1), FULL, by_rays(T.field_train, True))
    # ---- the layered dX chain ----
    for (W, C_) in ((128, 128), (256, 16)):
        for typ, fine, mode in variants[:2]:
            for g in (False, True):
                add(f"layered,W={W},C={C_},{typ},{mname[mode]},rays_grad={int(g)}", {"SPLIT": "f32", "FUSED_DX": False}, A(W, C_, fine), mode,
                    by_rays(T.field_train, g))
    add("layered,W=128,C=128,fine,full,SPLIT=h3", {"FUSED_DX": False}, A(128, 128, 1), FULL, by_rays(T.field_train))
    # ---- a reduced embedding ----
    red = A(128, 128, 1, xyz=33, dirs=15)
    for mode in (FULL, STATIC):
        for split in ("h3", "f32"):
            add(f"reduced,W=128,C=128,fine,{mname[mode]}", {"SPLIT": split}, red, mode, by_rays(T.field_train, True))
    add("reduced,W=128,C=128,fine,full,layered", {"SPLIT": "f32", "FUSED_DX": False}, red, FULL, by_rays(T.field_train))
    # ---- tuned on a supplied encoding ----
    enc_names = T.param_names
    for C_ in (16, 128):
        ext = A(256, C_, 1, xyz=32)
        for mode in (FULL, STATIC):
            add(f"tuned-ext,W=256,C={C_},{mname[mode]},grid", {}, ext, mode, by_grid(T.field_train_encoded, True))
            add(f"tuned-ext,W=256,C={C_},{mname[mode]},enc", {}, ext, mode, by_enc(T.FieldTrainEncoded, enc_names))
            add(f"tuned-ext,W=256,C={C_},{mname[mode]},frozen", {}, ext, mode, by_enc(T.FieldTrainEncoded, enc_names), frozen=True)
            add(f"tuned-ext,W=256,C={C_},{mname[mode]},viewdirs only", {}, ext, mode, by_enc(T.FieldTrainEncoded, enc_names, enc_grad=False))
            add(f"tuned-ext,W=256,C={C_},{mname[mode]},frozen,viewdirs only", {}, ext, mode,
                by_enc(T.FieldTrainEncoded, enc_names, enc_grad=False), frozen=True)
        add(f"tuned-ext,W=256,C={C_},full,SPLIT=f32", {"SPLIT": "f32"}, ext, FULL, by_enc(T.FieldTrainEncoded, enc_names))
        add(f"tuned-ext,W=256,C={C_},full,h3_valid=0", {}, ext, FULL, by_enc(T.FieldTrainEncoded, enc_names), h3_valid=False)
    add("tuned-ext,W=256,C=16,full,debug", {"DEBUG": 1}, A(256, 16, 1, xyz=32), FULL, by_enc(T.FieldTrainEncoded, enc_names))
    add("tuned-ext,W=128,C=16,full", {}, A(128, 16, 1, xyz=32), FULL, by_enc(T.FieldTrainEncoded, enc_names))
    add("tuned-ext,W=256,C=16,full,M at the bound", {}, A(256, 16, 1, xyz=32), FULL,
        by_enc(T.FieldTrainEncoded, enc_names, shape=(1 << 21, 1 << 10, 32), device="meta"))
    # ---- generic ----
    gen = {"GENERIC_TRAIN": True, "GENERIC_TRAIN_EXT": True}
    gnames = T.param_names_generic
    for (W, D, C_, fine) in ((32, 1, 16, 0), (64, 6, 16, 1), (96, 5, 128, 1), (288, 5, 128, 1), (512, 8, 16, 1)):
        tag = f"W={W},D={D},C={C_},fine={fine}"
        for mode in (STATIC, FULL):
            for g in (False, True):
                add(f"generic,{tag},{mname[mode]},rays_grad={int(g)}", gen, A(W, C_, fine, D=D), mode, by_rays(T.field_train_generic, g), gnames)
                add(f"generic-ext,{tag},{mname[mode]},grid,rays_grad={int(g)}", gen, A(W, C_, fine, D=D, xyz=32), mode,
                    by_grid(T.field_train_generic_encoded, g), gnames)
            add(f"generic-ext,{tag},{mname[mode]},enc", gen, A(W, C_, fine, D=D, xyz=32), mode, by_enc(T.FieldTrainGenericEncoded, gnames), gnames)
            add(f"generic-ext,{tag},{mname[mode]},frozen", gen, A(W, C_, fine, D=D, xyz=32), mode, by_enc(T.FieldTrainGenericEncoded, gnames),
                gnames, frozen=True)
            add(f"generic-ext,{tag},{mname[mode]},viewdirs only", gen, A(W, C_, fine, D=D, xyz=32), mode,
                by_enc(T.FieldTrainGenericEncoded, gnames, enc_grad=False), gnames)
    add("generic,W=64,D=6,C=16,full,debug", dict(gen, DEBUG=1), A(64, 16, 1, D=6), FULL, by_rays(T.field_train_generic, True), gnames)
    add("generic-ext,W=96,D=5,C=128,full,debug", dict(gen, DEBUG=1), A(96, 128, 1, D=5, xyz=32), FULL, by_enc(T.FieldTrainGenericEncoded, gnames), gnames)
    add("generic,W=128,D=8,C=128,full (a tuned shape)", gen, A(128, 128, 1), FULL, by_rays(T.field_train_generic, True), gnames)
    add("generic,W=128,D=8,C=128,full,reduced", gen, red, FULL, by_rays(T.field_train_generic, True), gnames)
    # ---- refusals ----
    sig_names = lambda net, mode: T.param_names(net, STATIC)
    full_names = lambda net, mode: T.param_names_generic(net, STATIC)
    add("refusal,sigma,FieldTrain", {}, A(256, 16, 1), SIGMA, by_rays(lambda net, mode, *r: T.FieldTrain.apply(*r, net, mode)), sig_names)
    add("refusal,sigma,FieldTrainEncoded", {}, A(256, 16, 1, xyz=32), SIGMA, by_enc(T.FieldTrainEncoded, sig_names), sig_names)
    add("refusal,sigma,FieldTrainGeneric", gen, A(64, 16, 1, D=6), SIGMA, by_rays(lambda net, mode, *r: T.FieldTrainGeneric.apply(*r, net, mode)), full_names)
    add("refusal,sigma,FieldTrainGenericEncoded", gen, A(64, 16, 1, D=6, xyz=32), SIGMA, by_enc(T.FieldTrainGenericEncoded, full_names), full_names)
    add("refusal,full without a transient head,generic", gen, A(64, 16, 0, D=6), FULL,
        by_rays(lambda net, mode, *r: T.FieldTrainGeneric.apply(*r, net, mode)), full_names)
    add("refusal,full without a transient head,generic-ext", gen, A(64, 16, 0, D=6, xyz=32), FULL, by_enc(T.FieldTrainGenericEncoded, full_names),
        full_names)
    add("refusal,z asks for a gradient,tuned", {}, A(256, 16, 1), FULL, by_rays(T.field_train, True, True))
    add("refusal,z asks for a gradient,generic", gen, A(64, 16, 1, D=6), FULL, by_rays(T.field_train_generic, True, True), gnames)
    add("refusal,a frequency-embedding pack on FieldTrainGenericEncoded", gen, A(64, 16, 1, D=6, xyz=32), FULL,
        by_enc(T.FieldTrainGenericEncoded, gnames), gnames, generic_ext=False)
    add("refusal,field_train_generic with GENERIC_TRAIN off", {}, A(64, 16, 1, D=6), FULL, by_rays(T.field_train_generic), gnames)
    add("refusal,field_train_generic with GENERIC_TRAIN_EXT alone", {"GENERIC_TRAIN_EXT": True}, A(64, 16, 1, D=6), FULL,
        by_rays(T.field_train_generic), gnames)
    return out


def record():
    """-> {"events": [distinct events], "cases": [[index into events, ...] per case, in cases() order], "n": count, "ids_sha256":
    digest of the case ids in that order}, [case ids]"""
    table, rows, ids = {}, [], []
    with patched():
        for cid, thunk in cases():
            rows.append([table.setdefault(e, len(table)) for e in thunk()])
            ids.append(cid)
    return {"events": list(table), "cases": rows, "n": len(rows), "ids_sha256": hashlib.sha256("\n".join(ids).encode()).hexdigest()}, ids


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec, ids = record()
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    with open(out, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    print(f"{out}: {rec['n']} cases, {len(rec['events'])} distinct events, {os.path.getsize(out)} bytes, sha256 {digest}")


if __name__ == "__main__":
    main()
