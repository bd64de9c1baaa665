"""Digests of what the fp16 two-part field kernels write, on fixed inputs, for A/B builds that must not change a bit.
    NEFES_HIP_LIB=<lib> python tools/ab_identical.py
prints one sha256 per output of every public fp16 entry point at every row of csrc/field_h3_instances.h it can reach: forward raw_t
and ReLU masks (TRAIN rows: `acts` too), backward g_pts / g_xyz_enc and g_viewdirs_s (TRAIN rows: `dacts` too).  3 rays x 50 samples =
one full 128-sample tile and a ragged one, S a multiple of nothing; one shared-depth-row case for _zrow and _hashgrid; fixed seeds.
Run it once per library and compare the lines that do not start with '#': a re-arrangement of the host code, or a re-scheduling of the
same arithmetic, gives the same digests.  Only entry points that older libraries export as well are called, and an older library's
ABI number is accepted, so the same script runs on both sides.
    NEFES_HIP_LIB=<lib> python tools/ab_identical.py --generic
prints, instead, the digests of every output of the eight generic entry points (csrc/field_generic.hip) and of both packers, at
GENERIC_SHAPES on the frequency embedding and on a supplied encoding.  Every output buffer is filled with a fixed non-zero pattern
before the call and digested whole, so what a kernel must not touch is compared as well.
    NEFES_HIP_LIB=<lib> python tools/ab_identical.py --train
prints, instead, the digests of one train-mode forward + backward through the four autograd Functions of nefes_amd/train.py (raw_t,
every parameter gradient, the gradients of the rays or of the encoding and viewdirs) at TRAIN_CASES: for A/B revisions of the HOST code
on one library.  37 rays x 24 samples = seven tiles, the last ragged.
    NEFES_HIP_LIB=<lib> python tools/ab_identical.py --refine
prints, instead, the digests of what the refinement loop of nefes_amd/refine.py returns (pose, loss curve, the numbers of `info`) at
REFINE_CASES, 6 iterations each, on the scene of tests/golden/refine50.npz (30 x 40 rays, 64 + 64 samples, 8 x 128 networks, C = 128):
for A/B revisions of the HOST code on one library.  Only PoseRefiner's constructor, refine, refine_apr, refine_concurrently and
refine_apr_concurrently are called.
    NEFES_HIP_LIB=<lib> python tools/ab_identical.py --composite
prints, instead, the digests of every output of nefes_composite_fwd and nefes_composite_bwd (csrc/composite.hip) at every run of
tests/composite_ref.py's case list -- ragged, deep, four-per-lane, every upstream alone, the channel split, and the misaligned cases on
each of their three pointer offsets: every forward map and the whole g_raw_t -- and of every output of ops.coarse_sample (csrc/sample_pdf.hip)
at Nc = 64, 128, 256 on a shared depth row and on per-ray depths.  Output buffers carry eight rays of padding, are filled with a fixed
pattern before the call and digested whole, byte for byte (NaN sign and payload bits included).
    python tools/ab_identical.py --feature-loss [--time]
prints, instead, the digests of the loss, the cosines and the whole gradient of the four feature losses (ops.cosine_feature_loss,
upsampled_cosine_loss, pixel_cosine_loss, upsampled_pixel_cosine_loss; csrc/feature_loss.hip) at LOW_SHAPES / UP_SHAPES of
tests/test_gpu_masked_loss.py and the loop's shape -- one shape of each has three groups -- without a mask, with a random one and with
all ones, and of ops.upsampled_cosine_loss_prepared at four shapes.  Only those five functions are called, so the same file runs in an
earlier commit's tree (copy it there).  --time: then, per op at the loop's shape, the median and min / max of 200 calls' device time
each way, around the entry-point call (ops.TIMERS) and around the whole eager call ('# time' lines).
    python tools/ab_identical.py --rays
prints, instead, the digests of every output of the nine ray-generation entry points (csrc/rays.hip: the focal, intrinsics and pixel-list
pairs) and of the six ops.raygen_* functions over them at RAY_GRIDS -- the focal pair at the centred camera, the intrinsics pair at a
centred and an off-centre one, the list pair on each grid's row-major integer pixels -- and at the sub-pixel lists of
tests/test_gpu_pixels.py (RAY_LISTS): the forward, and the backward with all three upstream gradients and with each alone, with and
without the camera's gradient.  The C ABI's buffers, the workspace included, are filled with a fixed pattern before the call and digested
whole.  Only those names are called, so the same file runs in an earlier commit's tree (copy it there)."""
import ctypes as C
import hashlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import lib as L

_raw = C.CDLL(L.LIB_PATH)                      # A/B against a library of an earlier commit: bind what it has, under its own ABI number
L.SIGNATURES = {k: v for k, v in L.SIGNATURES.items() if hasattr(_raw, k)}
L.ABI_VERSION = _raw.nefes_version()
from nefes_amd import ops

lib = L.load()
dev = torch.device('cuda')
N, S = 3, 50
M = N * S
SIGMA, STATIC, FULL = L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL
g = torch.Generator(device='cpu').manual_seed(1)
rnd = lambda *shape: torch.randn(*shape, generator=g)
o = (rnd(N, 3) * 0.3).to(dev)
d = torch.nn.functional.normalize(rnd(N, 3), dim=-1).to(dev)
z = torch.sort(torch.rand(N, S, generator=g) * 4, -1)[0].to(dev)
z_row = z[0].contiguous()
enc = (rnd(M, 32) * 0.5).to(dev)
grid = L.NefesHashGridDesc(16, 2, 14, 16, 1.3819, 8.0)
table = (rnd(int(lib.nefes_hashgrid_table_entries(C.byref(grid))), 2) * 0.5).to(dev)
P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
reached = set()


def network(width, c, ext, fold):
    """PackedField of a random network (the tensors of nerfh_nff.py:452-505); activations spread over a few octaves so that the
    exponent picks differ per sample"""
    gw = torch.Generator(device='cpu').manual_seed(width + c)
    w2, k_in = width // 2, 32 if ext else 63
    shapes = [(width, k_in)] + [(width, width)] * 3 + [(width, width + k_in)] + [(width, width)] * 3 + \
             [(width, width), (w2, width + 27), (1, width), (3 + c, w2), (w2, width + 27), (w2, w2), (w2, w2), (1, w2), (3, w2), (1, w2)]
    sd = {}
    for i, (name, (n_out, n_in)) in enumerate(zip(ops.PackedField.LAYERS_FINE, shapes)):
        s = (1.0 + 0.5 * ((i * 7) % 5)) / n_in ** 0.5
        sd[name + ".weight"] = (torch.rand(n_out, n_in, generator=gw) * 2 - 1) * s * 1.7
        sd[name + ".bias"] = (torch.rand(n_out, generator=gw) * 2 - 1) * 0.1
    return ops.PackedField(sd, width, c, True, dev, xyz_encoding=L.XYZ_EXTERNAL32 if ext else L.XYZ_FREQ10, fold_final=fold)


def dig(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def note(pk, backward, mode, flags):
    if "nefes_field_h3_instance" in L.SIGNATURES:
        name = C.create_string_buffer(96)
        assert lib.nefes_field_h3_instance(C.byref(pk.desc), backward, mode, flags, name, len(name)) == 0
        reached.add(name.value.decode())
        print("#", name.value.decode())


def out(tag, **tensors):
    torch.cuda.synchronize()
    print(f"{tag:58s}", "  ".join(f"{k} {dig(t)}" for k, t in tensors.items()), flush=True)


def buffers(pk, R, train):
    raw = torch.zeros(N, R, S, device=dev)
    masks = torch.zeros(pk.mask_bytes(M) // 4, dtype=torch.int32, device=dev)
    acts = torch.zeros((M + 127) // 128, int(lib.nefes_train_rows(C.byref(pk.desc))), 128, device=dev) if train else None
    return raw, masks, acts


def run(pk, what):
    """every entry point that serves this network: forward, then the backward of its outputs"""
    ds, blob, c, tag = C.byref(pk.desc), P(pk.blob), pk.feat_dim, f"W{pk.width} C{pk.feat_dim} {what}"
    ext = pk.xyz_encoding == L.XYZ_EXTERNAL32
    upstream = lambda R: (torch.randn(N, R, S, generator=torch.Generator(device='cpu').manual_seed(R)) * 0.1).to(dev)
    grads = lambda: (torch.zeros(M, 32 if ext else 3, device=dev), torch.zeros(M, 3, device=dev))
    if what == "fh":
        R = 3 + (pk.width // 2 + 1) + 6
        raw, masks, _ = buffers(pk, R, False)
        note(pk, 0, FULL, L.H3_REQ_FH)
        L.check(lib.nefes_field_fwd_h3_fh(ds, blob, FULL, N, S, P(o), P(d), P(z), P(d), P(raw), P(masks), None), tag)
        out(tag + " fwd_h3_fh", raw=raw, masks=masks)
        note(pk, 1, FULL, L.H3_REQ_FH)
        gmap = (torch.randn(N, pk.width // 2 + 1, generator=torch.Generator(device='cpu').manual_seed(5)) * 0.1).to(dev)
        for name, gm in (("bwd_h3_fh", None), ("bwd_h3_fh gmap", gmap)):
            gx, gv = grads()
            L.check(lib.nefes_field_bwd_h3_fh(ds, blob, N, S, P(o), P(d), P(z), P(d), P(raw), P(upstream(R)), P(gm), P(masks), P(gx), P(gv), None), tag)
            out(f"{tag} {name}", g_pts=gx, g_viewdirs_s=gv)
        return
    modes = (FULL,) if what == "fold" else ((SIGMA, FULL) if ext else (SIGMA, STATIC, FULL))
    for mode in modes:
        R = 1 if mode == SIGMA else 3 + c + (1 if mode == STATIC else 6)
        raw, masks, _ = buffers(pk, R, False)
        note(pk, 0, mode, 0)
        L.check(lib.nefes_field_fwd_h3(ds, blob, mode, N, S, None if ext else P(o), None if ext else P(d), None if ext else P(z), None,
                                       P(enc) if ext else None, P(d), P(raw), P(masks), None), tag)
        out(f"{tag} fwd_h3 mode {mode}", raw=raw, masks=masks)
        if mode == SIGMA:
            continue
        gx, gv = grads()
        if mode == FULL:
            note(pk, 1, mode, 0)
            L.check(lib.nefes_field_bwd_h3(ds, blob, N, S, P(o), P(d), P(z), None, P(d), P(raw), P(upstream(R)), P(masks),
                                           None if ext else P(gx), P(gx) if ext else None, P(gv), None), tag)
            out(f"{tag} bwd_h3", **{"g_xyz_enc" if ext else "g_pts": gx, "g_viewdirs_s": gv})
        else:
            note(pk, 1, mode, L.H3_REQ_STATIC_BWD)
            L.check(lib.nefes_field_bwd_static_h3(ds, blob, N, S, P(o), P(d), P(z), None, P(d), P(raw), P(upstream(R)), P(masks), P(gx), P(gv), None), tag)
            out(f"{tag} bwd_static_h3", g_pts=gx, g_viewdirs_s=gv)
    if what == "fold":
        return
    if what == "zrow":                          # one row of depths shared by every ray
        raw, masks, _ = buffers(pk, 1, False)
        note(pk, 0, SIGMA, L.H3_REQ_ZROW)
        L.check(lib.nefes_field_fwd_h3_zrow(ds, blob, SIGMA, N, S, P(o), P(d), P(z_row), P(d), P(raw), P(masks), None), tag)
        out(f"{tag} fwd_h3_zrow mode {SIGMA}", raw=raw, masks=masks)
    if ext and c <= 29:                         # the hash grid gathered by the kernels themselves
        for mode, row in ((SIGMA, 1), (SIGMA, 0), (FULL, 0)):
            R = 1 if mode == SIGMA else 3 + c + 6
            raw, masks, _ = buffers(pk, R, False)
            note(pk, 0, mode, L.H3_REQ_HASHGRID)
            L.check(lib.nefes_field_fwd_h3_hashgrid(ds, blob, C.byref(grid), P(table), mode, N, S, P(o), P(d), P(z_row if row else z), row, P(d),
                                                    P(raw), P(masks), None), tag)
            out(f"{tag} fwd_h3_hashgrid mode {mode} z_is_row {row}", raw=raw, masks=masks)
        gx, gv = torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev)
        note(pk, 1, FULL, L.H3_REQ_HASHGRID)
        L.check(lib.nefes_field_bwd_h3_hashgrid(ds, blob, C.byref(grid), P(table), N, S, P(o), P(d), P(z), P(d), P(raw), P(upstream(R)), P(masks),
                                                P(gx), P(gv), None), tag)
        out(f"{tag} bwd_h3_hashgrid", g_pts=gx, g_viewdirs_s=gv)
    for mode in (STATIC, FULL):                 # train mode
        R = 3 + c + (1 if mode == STATIC else 6)
        raw, masks, acts = buffers(pk, R, True)
        dacts, (gx, gv) = torch.zeros_like(acts), grads()
        flags = L.H3_REQ_TRAIN | (L.H3_REQ_EXT if ext else 0)
        note(pk, 0, mode, flags)
        note(pk, 1, mode, flags)
        if ext:
            L.check(lib.nefes_field_fwd_train_h3_ext(ds, blob, mode, N, S, P(enc), P(d), P(raw), P(acts), P(masks), None), tag)
            out(f"{tag} fwd_train_h3_ext mode {mode}", raw=raw, masks=masks, acts=acts)
            L.check(lib.nefes_field_bwd_train_h3_ext(ds, blob, mode, N, S, P(d), P(raw), P(upstream(R)), P(masks), P(dacts), P(gx), P(gv), None), tag)
            out(f"{tag} bwd_train_h3_ext mode {mode}", g_xyz_enc=gx, g_viewdirs_s=gv, dacts=dacts)
        else:
            L.check(lib.nefes_field_fwd_train_h3(ds, blob, mode, N, S, P(o), P(d), P(z), None, P(d), P(raw), P(acts), P(masks), None), tag)
            out(f"{tag} fwd_train_h3 mode {mode}", raw=raw, masks=masks, acts=acts)
            L.check(lib.nefes_field_bwd_train_h3(ds, blob, mode, N, S, P(o), P(d), P(z), P(d), P(raw), P(upstream(R)), P(masks), P(dacts),
                                                 P(gx), P(gv), None), tag)
            out(f"{tag} bwd_train_h3 mode {mode}", g_pts=gx, g_viewdirs_s=gv, dacts=dacts)


# (W, D, C, transient head), skip = 4 where D > 4: depth 1, a skip layer and none, row-block counts that are no multiple of the four
# waves, W below and above the head's 160 rows, both head paddings, both tile sizes (64 samples up to W = 256, 32 above).  With
# N x S = 3 x 50 the last tile is ragged at both sizes and the train launches have tiles wholly past the last sample.
GENERIC_SHAPES = ((32, 1, 16, False), (64, 6, 16, True), (96, 5, 128, True), (288, 5, 128, True))


def generic_network(W, D, c, fine, ext):
    """(host state dict, PackedGeneric) of a random network of that shape"""
    gw = torch.Generator(device='cpu').manual_seed(W + D + c)
    skip, H, k_in = (4 if D > 4 else -1), W // 2, 32 if ext else 63
    shapes = [(W, k_in if i == 0 else (W + k_in if i == skip else W)) for i in range(D)] + [(W, W), (H, W + 27), (1, W), (3 + c, H)]
    if fine:
        shapes += [(H, W + 27), (H, H), (H, H), (1, H), (3, H), (1, H)]
    sd = {}
    for i, (name, (n_out, n_in)) in enumerate(zip(ops.PackedGeneric.layer_names(D, fine), shapes)):
        sc = (1.0 + 0.5 * ((i * 7) % 5)) / n_in ** 0.5
        sd[name + ".weight"] = (torch.rand(n_out, n_in, generator=gw) * 2 - 1) * sc * 1.7
        sd[name + ".bias"] = (torch.rand(n_out, generator=gw) * 2 - 1) * 0.1
    return sd, ops.PackedGeneric(sd, W, D, skip, c, fine, dev, xyz_encoding=L.XYZ_EXTERNAL32 if ext else L.XYZ_FREQ10)


def run_generic(W, D, c, fine, ext):
    sd, pk = generic_network(W, D, c, fine, ext)
    ds, blob, tag = pk.desc, P(pk.blob), f"W{W} D{D} C{c} {'ext' if ext else 'freq'}"
    sfx, first = ("_ext", "g_xyz_enc") if ext else ("", "g_pts")
    call = lambda name, *a: L.check(getattr(lib, f"nefes_field_{name}{sfx}")(ds, blob, *a, None), f"{tag} {name}{sfx}")
    fill = lambda *shape: torch.full(shape, 0.123, device=dev)
    words = lambda: torch.full((pk.mask_bytes(M) // 4,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    upstream = lambda R: (torch.randn(N, R, S, generator=torch.Generator(device='cpu').manual_seed(R)) * 0.1).to(dev)
    rays = (P(enc),) if ext else (P(o), P(d), P(z))
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(M, 3).contiguous()
    # the two packers: the host's into a patterned buffer (it clears the whole blob), the device's over a patterned blob (it leaves
    # the padding alone)
    names = ops.PackedGeneric.layer_names(D, fine)
    host = [sd[n + k].contiguous() for n in names for k in (".weight", ".bias")]
    hblob = torch.full((pk.blob.numel(),), 0x5a, dtype=torch.uint8)
    L.check(lib.nefes_generic_pack(ds, (C.c_void_p * len(host))(*[t.data_ptr() for t in host]), len(host), P(hblob), hblob.numel()), tag)
    devt = [t.to(dev) for t in host]
    dblob = torch.full((pk.blob.numel(),), 0x5a, dtype=torch.uint8, device=dev)
    L.check(lib.nefes_generic_pack_device(ds, (C.c_void_p * len(devt))(*[t.data_ptr() for t in devt]), len(devt), P(dblob), dblob.numel(), None), tag)
    out(f"{tag} pack", host=hblob, device=dblob, used=pk.blob)
    top = FULL if fine else STATIC
    for mode in (SIGMA, STATIC, FULL) if fine else (SIGMA, STATIC):
        R = pk.n_raw(mode)
        raw, masks = fill(N, R, S), words()
        call("fwd_generic", mode, N, S, *rays, *(() if ext else (None,)), P(d), P(raw), P(masks))
        out(f"{tag} fwd_generic{sfx} mode {mode}", raw=raw, masks=masks)
        if mode == top and not ext:                  # the caller's points in the place of rays
            raw_p, masks_p = fill(N, R, S), words()
            call("fwd_generic", mode, N, S, None, None, None, P(pts), P(d), P(raw_p), P(masks_p))
            out(f"{tag} fwd_generic mode {mode} pts", raw=raw_p, masks=masks_p)
        if mode == SIGMA:
            continue
        g_up, gx, gv = upstream(R), fill(M, 32 if ext else 3), fill(M, 3)
        call("bwd_generic", mode, N, S, *(() if ext else rays + (None,)), P(d), P(raw), P(g_up), P(masks), P(gx), P(gv))
        out(f"{tag} bwd_generic{sfx} mode {mode}", **{first: gx, "g_viewdirs_s": gv})
        raw, masks = fill(N, R, S), words()
        acts, gx, gv = fill((M + 127) // 128, pk.train_rows()[0], 128), fill(M, 32 if ext else 3), fill(M, 3)
        dacts = torch.full_like(acts, 0.123)
        call("fwd_train_generic", mode, N, S, *rays, P(d), P(raw), P(acts), P(masks))
        out(f"{tag} fwd_train_generic{sfx} mode {mode}", raw=raw, masks=masks, acts=acts)
        call("bwd_train_generic", mode, N, S, *(() if ext else rays), P(d), P(raw), P(g_up), P(masks), P(dacts), P(gx), P(gv))
        out(f"{tag} bwd_train_generic{sfx} mode {mode}", **{first: gx, "g_viewdirs_s": gv, "dacts": dacts})


# (tag, NeRFH_NFF arguments, mode, NEFES_SPLIT, generic kernels): both tuned pipes, a supplied encoding, a reduced embedding (33 / 15
# inputs), and the generic kernels on either input
TRAIN_CASES = (("tuned W128 C128 fine h3", dict(typ="fine", W=128, f_dim=128, encode_transient=True), FULL, "h3", False),
               ("tuned W256 C16 coarse f32", dict(typ="coarse", W=256, f_dim=16), STATIC, "f32", False),
               ("tuned W256 C16 fine ext", dict(typ="fine", W=256, f_dim=16, encode_transient=True, in_channels_xyz=32), FULL, "h3", False),
               ("tuned W128 C128 fine reduced", dict(typ="fine", W=128, f_dim=128, encode_transient=True, in_channels_xyz=33, in_channels_dir=15),
                FULL, "h3", False),
               ("generic W64 D6 C16 fine", dict(typ="fine", D=6, W=64, f_dim=16, encode_transient=True), FULL, "h3", True),
               ("generic W96 D5 C128 fine ext", dict(typ="fine", D=5, W=96, f_dim=128, encode_transient=True, in_channels_xyz=32), FULL, "h3", True))


def run_train():
    from nefes_amd import field as F, train as T
    Nt, St = 37, 24
    gt = torch.Generator(device='cpu').manual_seed(7)
    leaf = lambda t: t.to(dev).requires_grad_()
    for tag, kw, mode, split, generic in TRAIN_CASES:
        ops.SPLIT, ops.GENERIC_TRAIN, ops.GENERIC_TRAIN_EXT = split, True, True
        net = F.NeRFH_NFF(**kw).to(dev)
        ext = kw.get("in_channels_xyz") == 32
        names = (T.param_names_generic if generic else T.param_names)(net, mode)
        sd = dict(net.named_parameters())
        ro, rd = leaf(torch.randn(Nt, 3, generator=gt) * 0.3), leaf(torch.nn.functional.normalize(torch.randn(Nt, 3, generator=gt), dim=-1))
        rv = leaf(torch.nn.functional.normalize(torch.randn(Nt, 3, generator=gt), dim=-1))
        rz = torch.sort(torch.rand(Nt, St, generator=gt) * 3.5 + 0.2, -1)[0].to(dev)
        if ext:
            e = leaf(torch.randn(Nt, St, 32, generator=gt) * 0.5)
            raw = (T.FieldTrainGenericEncoded if generic else T.FieldTrainEncoded).apply(e, rv, net, mode, *[sd[n] for n in names])
            inputs = {"enc": e, "viewdirs": rv}
        else:
            raw = (T.field_train_generic if generic else T.field_train)(net, mode, ro, rd, rv, rz)
            inputs = {"rays_o": ro, "rays_d": rd, "viewdirs": rv}
        raw.backward((torch.randn(raw.shape, generator=gt) * 0.1).to(dev))
        torch.cuda.synchronize()
        for k, t in [("raw_t", raw)] + [(n, sd[n].grad) for n in names] + [("d " + k, t.grad) for k, t in inputs.items()]:
            print(f"{tag:30s} {k:34s} {tuple(t.shape)!s:18s} {dig(t)}", flush=True)


# (tag, PoseRefiner arguments, what is run): both modes replayed and eager, every route of the up-sampled loss, the torch glue, a batch,
# a second image through an existing graph (state reset in place), both stream drivers (rounds of two included), and the per-pixel and
# masked losses on the up-sampled one-pass kernels and at low resolution
REFINE_CASES = (("mode3 graph", dict(graph=True), "twice"),
                ("mode3 eager", dict(graph=False), "once"),
                ("mode3 upsample prepared", dict(graph=True, upsample=True, plain=True, prepared=True), "once"),
                ("mode3 upsample one-pass", dict(graph=True, upsample=True, plain=True, prepared=False), "once"),
                ("mode3 upsample hist world", dict(graph=True, upsample=True), "once"),
                ("mode3 torch glue", dict(graph=False, fused_glue=False), "once"),
                ("mode3 upsample per_pixel", dict(graph=True, upsample=True, plain=True, per_pixel=True), "once"),
                ("mode3 upsample masked", dict(graph=True, upsample=True, plain=True, masked=True), "once"),
                ("mode3 masked per_pixel", dict(graph=True, masked=True, per_pixel=True), "once"),
                ("mode3 images=2", dict(graph=True, images=2), "batch"),
                ("mode2 graph", dict(graph=True, apr=0), "apr twice"),
                ("mode2 eager", dict(graph=False, apr=0), "apr twice"),
                ("mode3 two streams", dict(graph=True, bn_running_stats=False), "streams"),
                ("mode2 two streams", dict(graph=True, apr=0, bn_running_stats=False), "apr streams"))


def run_refine():
    import types
    import numpy as np
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner, refine_apr_concurrently, refine_concurrently
    from oracle import refine_cpu as RC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gd = dict(np.load(os.path.join(root, "tests", "golden", "refine50.npz")))
    T = lambda a: torch.from_numpy(np.asarray(a))
    iters, (H, W, focal) = 6, gd["hwf"].tolist()
    H, W = int(H), int(W)

    class TinyAPR(torch.nn.Module):            # the fixture's stand-in regression network (tests/test_gpu_refine50.py)
        def __init__(self, k):
            super().__init__()
            self.fc = torch.nn.Linear(12, 12)
            with torch.no_grad():
                self.fc.weight.copy_(T(gd["m2_weight"][k]))
                self.fc.bias.copy_(T(gd["m2_bias"][k]))

        def forward(self, x):
            return self.fc(torch.nn.functional.adaptive_avg_pool2d(x, 2).reshape(x.shape[0], -1))

    def nets():
        coarse = NeRFH_NFF('coarse', W=int(gd["Wd"]), f_dim=int(gd["C"]))
        fine = NeRFH_NFF('fine', W=int(gd["Wd"]), f_dim=int(gd["C"]), encode_appearance=True, encode_transient=True)
        gain, decay, sg = (float(v) for v in gd["scene"])
        with torch.no_grad():
            coarse.exposure_embedding.params.copy_(T(gd["exposure_params"]))
            for n in (coarse, fine):
                RC.structure_scene(dict(n.named_parameters()), gain, decay, sg)
        return coarse.requires_grad_(False).to(dev), fine.requires_grad_(False).to(dev)

    def refiner(networks, apr=None, plain=False, prepared=None, **more):
        coarse, fine = networks
        args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=not plain)
        kw = dict(network_query_fn=None, perturb=0., N_importance=int(gd["Ni"]), N_samples=int(gd["Nc"]), network_fn=coarse, network_fine=fine,
                  use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False, lindisp=False)
        world = None if plain else dict(pose_scale=float(gd["pose_scale"]), pose_scale2=float(gd["pose_scale2"]),
                                        move_all_cam_vec=gd["move_all_cam_vec"].tolist())
        if apr is not None:
            more.update(pose_model=TinyAPR(apr), svd_reg=True, learning_rate=float(gd["m2_lr"]))
        if prepared is not None:
            PoseRefiner.PREPARED_TARGET = prepared
        return PoseRefiner(kw, args, (H, W, focal), float(gd["near"]), float(gd["far"]), tinyscale=int(gd["tinyscale"]), lr_r=float(gd["lr"][0]),
                           lr_t=float(gd["lr"][1]), world_setup=world, device=dev, **more)

    def show(tag, result):
        torch.cuda.synchronize()
        pose, losses, info = (tuple(result) + ({},))[:3]
        nums = torch.tensor([float(v) for k in sorted(info) for v in (info[k] if isinstance(info[k], tuple) else (info[k],))], dtype=torch.float64)
        print(f"{tag:44s} pose {dig(pose)}  losses {dig(losses)}  info {dig(nums)}", flush=True)

    full = torch.nn.functional.interpolate(T(gd["target_low"])[None], size=(H, W), mode="bicubic")[0]       # on the CPU, as the fixture's generator
    photo, hist = T(gd["photo_u8"]).float()[None] / 255., T(gd["hist"])
    default_prepared = PoseRefiner.PREPARED_TARGET
    shared = nets()
    for tag, kw, what in REFINE_CASES:
        PoseRefiner.PREPARED_TARGET = default_prepared
        target = full[:, 10:-10, 10:-10] if kw.get("upsample") else T(gd["target_low"])
        job = lambda k: (T(gd["init_c2w"][k]), target, hist)
        if what in ("once", "twice"):
            r = refiner(shared, **kw)
            # (a masked refiner gets a mask: about 60 % of the target's pixels valid)
            mask = (torch.rand(target.shape[-2:], generator=torch.Generator().manual_seed(5)) < 0.6) if kw.get("masked") else None
            show(tag, r.refine(*job(0), iters=iters, **({} if mask is None else {"mask": mask})))
            if what == "twice":
                show(tag + ", next image", r.refine(*job(3), iters=iters))
        elif what == "batch":
            r = refiner(shared, **kw)
            show(tag, r.refine(T(gd["init_c2w"][[0, 3]]), torch.stack([target, target.flip(-1)]), torch.stack([hist.reshape(-1)] * 2), iters=iters))
        elif what == "apr twice":
            r = refiner(shared, **kw)
            show(tag, r.refine_apr(photo, full, hist, iters=iters, verification=True))
            r.apr_base = TinyAPR(3)
            show(tag + ", next image", r.refine_apr(photo, full, hist, iters=iters, verification=True))
        elif what == "streams":
            rs = [refiner(shared, **kw) for _ in range(2)]
            for n_jobs, starts in ((2, (0, 3)), (3, (3, 0, 5))):
                for j, out in enumerate(refine_concurrently(rs, [job(k) for k in starts], iters=iters)):
                    show(f"{tag}, {n_jobs} jobs [{j}]", out)
        elif what == "apr streams":
            rs = [refiner(shared, **dict(kw, apr=k)) for k in (0, 3)]
            for j, out in enumerate(refine_apr_concurrently(rs, [(photo, full, hist)] * 2, iters=iters)):
                show(f"{tag} [{j}]", out)
    PoseRefiner.PREPARED_TARGET = default_prepared


def run_composite():
    from tests import composite_ref as R
    PAD, FILL = 8, 0.123

    def offset(t):                              # the tensor 4 bytes into a larger buffer: a pointer that is not 16-byte aligned
        buf = torch.zeros(t.numel() + 8, device=dev)
        buf[1:1 + t.numel()] = t.reshape(-1)
        return buf[1:1 + t.numel()].view(t.shape)

    runs = [(c, only, ()) for c, only in R.all_runs()]
    runs += [(R.misaligned_case(tag, S), None, mis) for tag, S in R.MISALIGNED for mis in (("raw_t",), ("z",), ("raw_t", "z"))]
    for case, only, mis in runs:
        tag, n, s, c = case["tag"], case["N"], case["S"], case["C"]
        flags, rows = R.FLAGS[tag] | (R.WHITE_BKGD if case["white"] else 0), R.n_rows(tag, c)
        raw_t, zz = case["raw"].permute(0, 2, 1).contiguous().to(dev), case["z"].to(dev)
        raw_t, zz = (offset(raw_t) if "raw_t" in mis else raw_t), (offset(zz) if "z" in mis else zz)
        full = lambda *sh: torch.full((n + PAD, *sh), FILL, device=dev)
        outs = {"acc": full(), "weights": full(s)}
        if tag != "D":
            outs.update(rgb=full(3), feat=full(c), disp=full(), depth=full(), beta=full())
        ups = {k: v.contiguous().to(dev) for k, v in case["ups"].items() if k in R.maps_of(case) and only in (None, k)}
        g_raw_t = full(rows, s)
        o, u = (lambda k: P(outs.get(k))), (lambda k: P(ups.get(k)))
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.nefes_composite_fwd(n, s, c, flags, 0.1, P(raw_t), P(zz), o("rgb"), o("feat"), o("disp"), o("acc"), o("depth"), o("weights"),
                                        o("beta"), st), "nefes_composite_fwd")
        L.check(lib.nefes_composite_bwd(n, s, c, flags, P(raw_t), P(zz), u("rgb"), u("feat"), u("disp"), u("acc"), u("depth"), u("weights"),
                                        u("beta"), P(g_raw_t), st), "nefes_composite_bwd")
        name = f"{tag}{'w' if case['white'] else ''} S{s} N{n} C{c} seed {case['seed']}" + (f" only {only}" if only else "") + \
               (" misaligned " + "+".join(mis) if mis else "")
        out(name, **outs, g_raw_t=g_raw_t)
    gs = torch.Generator(device='cpu').manual_seed(11)
    n, ni = 37, 128
    for nc in (64, 128, 256):
        centre = torch.rand(n, 1, generator=gs) * nc
        sig = (4.0 * torch.exp(-0.5 * ((torch.arange(nc)[None] - centre) / 3.0) ** 2)).contiguous().to(dev)
        z_rays = torch.sort(torch.rand(n, nc, generator=gs) * 4, -1)[0].to(dev)
        for what, zz in (("shared depth row", ops.coarse_depth_row(nc, 0., 4., False, dev)), ("per-ray depths", z_rays)):
            z_fine, z_samples, weights = ops.coarse_sample(sig, zz, ni, want_samples=True, want_weights=True)
            out(f"coarse_sample Nc{nc} Ni{ni} N{n} {what}", z_fine=z_fine, z_samples=z_samples, weights=weights)


def run_feature_loss(timed):
    os.environ.setdefault("NEFES_PARITY_LOG", os.devnull)      # (the test modules' shared helpers record parity numbers; not here)
    from tests.test_gpu_masked_loss import LOOP_SHAPE, LOW_SHAPES, UP_SHAPES, low_case, up_case
    UPSTREAM, FILL = 3.0, 0.123
    loop_low = (LOOP_SHAPE[0], LOOP_SHAPE[1], (LOOP_SHAPE[4] - 2 * LOOP_SHAPE[6]) * (LOOP_SHAPE[5] - 2 * LOOP_SHAPE[6]))
    low_ops = (("cosine", ops.cosine_feature_loss), ("pixcos", ops.pixel_cosine_loss))
    up_ops = (("upcos", ops.upsampled_cosine_loss), ("uppixcos", ops.upsampled_pixel_cosine_loss))

    def calls():
        """(tag, function of the features alone -> (loss, cos), features) of every case: each form at every shape (one of them three
        groups) without a mask, with a random one and with all ones; the prepared form at four shapes"""
        for shapes, fns, case in ((LOW_SHAPES + [loop_low], low_ops, low_case), (UP_SHAPES + [LOOP_SHAPE], up_ops, up_case)):
            for shape in shapes:
                for kind in (None, "random", "ones"):
                    x, t, m = (v.to(dev) for v in case(*shape, kind or "ones"))
                    kw = dict(groups=shape[0], return_cos=True, mask=None if kind is None else m)
                    if len(shape) == 7:
                        kw.update(size=shape[4:6], crop=shape[6])
                    for name, fn in fns:
                        yield f"{name} {shape} mask {kind}", (lambda v, fn=fn, t=t, kw=kw: fn(v, t, **kw)), x
        for shape in UP_SHAPES[:3] + [LOOP_SHAPE]:
            x, t, _ = (v.to(dev) for v in up_case(*shape, "ones"))
            prep = ops.UpcosTarget(*shape[1:], dev)
            if not prep.fits:
                print(f"# prepared {shape}: beyond the Gram kernel's LDS ceiling")
                continue
            prep.update(t)
            yield f"prepared {shape}", (lambda v, prep=prep: ops.upsampled_cosine_loss_prepared(v, prep, return_cos=True)), x

    def both_ways(fn, x):
        """(loss, cos, the whole gradient buffer, was it pre-filled?).  The ops allocate their gradient themselves, so the pre-fill is
        best effort: a block of the gradient's size is filled with FILL and freed just before the backward, and where the caching
        allocator hands the backward that very block (checked by address) what its kernels leave unwritten shows in the digest."""
        xr = x.clone().requires_grad_()
        loss, cos = fn(xr)
        up = torch.tensor(UPSTREAM, device=dev)
        pattern = torch.full_like(x, FILL)
        where = pattern.data_ptr()
        del pattern
        (grad,) = torch.autograd.grad(loss, xr, up)
        return loss, cos, grad, grad.data_ptr() == where

    for tag, fn, x in calls():
        loss, cos, grad, filled = both_ways(fn, x)
        if not filled:
            print(f"# {tag}: the gradient came in another block than the pre-filled one")
        out(tag, loss=loss, cos=cos, grad=grad)
    if not timed:
        return
    # per op at the loop's shape, 200 calls after 20, two brackets of HIP events each way: the one ops.TIMERS records around the
    # entry-point call (the unmasked channel-wise loss has no key), and one around the whole eager call -- the same work on any two
    # revisions of the host code, Python included.  Two decimals: the event clock's step shows in the min / max columns.
    WARM, CALLS = 20, 200
    for tag, fn, x in calls():
        if str(LOOP_SHAPE) not in tag and str(loop_low) not in tag or "ones" in tag:
            continue
        ops.TIMERS, whole = {}, {"whole call fwd": [], "whole call bwd": []}
        up = torch.tensor(UPSTREAM, device=dev)
        for _ in range(WARM + CALLS):
            xr = x.clone().requires_grad_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            loss, _ = fn(xr)
            ev[1].record()
            ev[2].record()
            torch.autograd.grad(loss, xr, up)
            ev[3].record()
            whole["whole call fwd"].append((ev[0], ev[1]))
            whole["whole call bwd"].append((ev[2], ev[3]))
        torch.cuda.synchronize()
        timers, ops.TIMERS = ops.TIMERS, None
        for key, pairs in sorted(timers.items()) + sorted(whole.items()):
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs[-CALLS:])
            print(f"# time {tag:48s} {key:28s} median {us[len(us) // 2]:8.2f} us  min {us[0]:8.2f}  max {us[-1]:8.2f}", flush=True)


# (H, W, focal, row shards): one block, row shards, nine blocks and a one-row shard, more rays than the 1024-block cap holds at once
RAY_GRIDS = ((6, 8, 7.3, ((0, 6),)), (10, 7, 9.1, ((0, 3), (3, 3), (6, 4), (0, 10))), (33, 65, 58.0, ((11, 1), (0, 33))), (513, 512, 400.0, ((0, 513),)))
RAY_LISTS = (1, 15, 257, 2305)


def run_rays():
    os.environ.setdefault("NEFES_PARITY_LOG", os.devnull)
    from oracle import ref_cpu as O
    from tests import pixels_ref as R
    from tests.test_gpu_intrinsics import centred, off_centre, upstream
    from tests.test_gpu_pixels import subpixel_list
    PAD, FILL = 8, 0.123
    c2w = O.bench_pose().to(dev)
    full = lambda *shape: torch.full(shape, FILL, device=dev)
    names = ("rays_o", "rays_d", "viewdirs")

    def pair(tag, stem, n, head, tail, ops_fwd, ops_bwd, camera):
        """Forward and every backward of one entry-point pair: through the C ABI on patterned buffers PAD rays (numbers) longer than
        what the kernels write, the workspace included, and through the ops.raygen_* functions of the same name."""
        ups_all = [t.to(dev) for t in upstream(n)]
        o, d, v = full(n + PAD, 3), full(n + PAD, 3), full(n + PAD, 3)
        L.check(getattr(lib, stem + "_fwd")(*head, P(c2w), *tail, P(o), P(d), P(v), None), tag)
        out(f"{tag} fwd", rays_o=o, rays_d=d, viewdirs=v)
        out(f"{tag} fwd ops", **dict(zip(names, ops_fwd())))
        ws_bytes = getattr(lib, stem + "_bwd_workspace")(n)
        for present in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            ups = [t if p else None for t, p in zip(ups_all, present)]
            for want in ((True, False) if camera else (None,)):
                ws = torch.full((ws_bytes + 64,), 0x5a, dtype=torch.uint8, device=dev)
                g12, g4 = full(12 + PAD), full(4 + PAD)
                more = (P(g4) if want else None,) if camera else ()
                L.check(getattr(lib, stem + "_bwd")(*head, P(c2w), *tail, *(P(t) for t in ups), P(ws), P(g12), *more, None), tag)
                got = ops_bwd(*ups) if not camera else ops_bwd(*ups, want_intr=want)
                got = (got, None) if torch.is_tensor(got) else got
                zero = torch.zeros(0)
                out(f"{tag} bwd {present} want_intr {want}", g_c2w=g12, g_intr=g4, workspace=ws, ops_g_c2w=got[0],
                    ops_g_intr=zero if got[1] is None else got[1])

    def list_pair(tag, px, K):
        n = px.shape[0]
        pair(tag, "nefes_raygen_px", n, (n, P(px), P(K)), (), lambda: ops.raygen_px_fwd(px, K, c2w),
             lambda *g, **kw: ops.raygen_px_bwd(px, K, c2w, *g, **kw), True)

    for H, W, f, shards in RAY_GRIDS:
        Kc, Ko = centred(H, W, f).to(dev), off_centre(H, W, f).to(dev)
        for row0, nr in shards:
            tag = f"{H}x{W} rows {row0}+{nr}"
            pair(f"raygen {tag}", "nefes_raygen", nr * W, (H, W, f), (row0, nr), lambda: ops.raygen_fwd(H, W, f, c2w, row0, nr),
                 lambda *g: ops.raygen_bwd(H, W, f, c2w, row0, nr, *g), False)
            for name, K in (("centred", Kc), ("off-centre", Ko)):
                pair(f"raygen_k {tag} {name}", "nefes_raygen_k", nr * W, (H, W, P(K)), (row0, nr), lambda: ops.raygen_k_fwd(H, W, K, c2w, row0, nr),
                     lambda *g, **kw: ops.raygen_k_bwd(H, W, K, c2w, row0, nr, *g, **kw), True)
            list_pair(f"raygen_px {tag} integer list", R.grid_pixels(W, row0, nr).to(dev), Ko)
    H, W, f = 33, 65, 58.0
    for n in RAY_LISTS:
        list_pair(f"raygen_px sub-pixel list n={n}", subpixel_list(n, H, W, seed=n).to(dev), off_centre(H, W, f).to(dev))


print("# lib", os.environ.get("NEFES_HIP_LIB") or "shipped", "ABI", L.ABI_VERSION)
if "--rays" in sys.argv[1:]:
    run_rays()
    sys.exit(0)
if "--feature-loss" in sys.argv[1:]:
    run_feature_loss("--time" in sys.argv[1:])
    sys.exit(0)
if "--composite" in sys.argv[1:]:
    run_composite()
    sys.exit(0)
if "--refine" in sys.argv[1:]:
    run_refine()
    sys.exit(0)
if "--train" in sys.argv[1:]:
    run_train()
    sys.exit(0)
if "--generic" in sys.argv[1:]:
    for shape in GENERIC_SHAPES:
        for ext in (False, True):
            run_generic(*shape, ext)
    sys.exit(0)
for width, c, ext, fold, what in ((256, 16, 0, 0, "zrow"), (256, 128, 0, 0, "freq"), (128, 16, 0, 0, "freq"), (128, 128, 0, 0, "freq"),
                                  (128, 0, 0, 0, "fh"), (256, 16, 0, 1, "fold"), (256, 128, 0, 1, "fold"), (256, 16, 1, 0, "ext"),
                                  (256, 128, 1, 0, "ext")):
    run(network(width, c, bool(ext), bool(fold)), what)
if reached:
    print(f"# table rows reached: {len(reached)}")
