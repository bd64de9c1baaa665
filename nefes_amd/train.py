"""Train mode of the field MLP: forward with saved pre-activations + weight gradients.

What `loss.backward()` does in script/run_nefes.py:42-108 for the NeRF weights, on the HIP path:

    forward   nefes_field_fwd_train   the fused forward kernel (TRAIN instance) also writes every hidden layer's
                                      pre-activation and both embeddings to `acts` [tiles][rows][128]
    backward  nefes_train_head_grad   d raw -> head pre-activation gradients
              nefes_train_dx          G_{l-1} = relu'(pre_{l-1}) * W_l^T G_l, layer by layer (MFMA)
              nefes_train_dw          dW_l = G_l act(X_{l-1})^T over all samples (MFMA, split over sample tiles)
              bias gradients          row sums of `dacts`

The layer graph below is the reference's NeRFH_NFF.forward (models/nerfh_nff.py:525-576): trunk 1..8 with the
skip `cat([input_xyz, h])` at layer 5, static_sigma on h8, xyz_encoding_final (no activation),
dir_encoding / transient_encoding.0 on `cat([final, dir_emb])`, static_rgb, transient_encoding.{2,4}, transient heads.
Gradients w.r.t. the rays are not produced here (training rays are data; the pose-refinement path uses field_bwd).
"""
import ctypes as C

import torch

from . import lib as L
from . import ops

EMB_XYZ, EMB_DIR = 63, 27
DEBUG = None          # tests may set this to a dict to receive the acts / dacts buffers of the last backward pass


def rows_view(buf):
    """[tiles, rows, 128] copy of an acts / dacts buffer in (row, sample) order.  The device layout stores, inside a tile, blocks
    of 32 rows x 16 samples contiguously (csrc/layout.h nefes_train_off): [row / 32][sample / 16][row % 32][sample % 16]."""
    T, rows, _ = buf.shape
    return buf.reshape(T, rows // 32, 8, 32, 16).permute(0, 1, 3, 2, 4).reshape(T, rows, 128)


def _emb_slot(n_freq, s, h):
    """layout.h nefes_emb_slot: embedding slot (s, h) -> index in the reference's embedding order, -1 = padding."""
    if s < 3 * n_freq:
        return 3 + 6 * (s // 3) + 3 * h + (s % 3)
    if s == 3 * n_freq:
        return h
    if s == 3 * n_freq + 1:
        return 2 if h == 0 else -1
    return -1


def _slot_rows(n_freq, n_rows, n_nat, device):
    """index tensor: natural embedding feature -> row of the slot-ordered block."""
    idx = [-1] * n_nat
    for row in range(n_rows):
        k = _emb_slot(n_freq, row // 2, row % 2)
        if k >= 0:
            idx[k] = row
    assert min(idx) >= 0
    return torch.tensor(idx, device=device)


def _pad_t(w, n_in_pad, k_pad):
    """[out, in] weight -> transposed, zero-padded [n_in_pad, k_pad] contiguous (A operand of nefes_train_dx)."""
    out, inn = w.shape
    wt = torch.zeros(n_in_pad, k_pad, device=w.device, dtype=torch.float32)
    wt[:inn, :out] = w.detach().t()
    return wt


def _dw_grid(ot, it):
    """(workgroups per share of the sample tiles, waves wanted per launch) for an ot x it-tile weight gradient: mirrors the
    block shapes nefes_train_dw picks (csrc/train.hip).  The big blocks hold 128-256 accumulator registers: one wave per SIMD,
    1024 SIMDs; the small ones run two or three waves per SIMD."""
    if ot % 4 == 0 and it % 4 == 0:
        return (ot // 4) * (it // 4), 1024
    if ot == 5 and it == 2:
        return 1, 1024
    if ot % 4 == 0 and it == 2:
        return ot // 4, 1024
    nto = 2 if ot % 2 == 0 else 1
    nti = 4 if it % 4 == 0 else (2 if it % 2 == 0 else 1)
    return (ot // nto) * (it // nti), 2048


class _Pass:
    def __init__(self, net, desc, n_tiles, acts, dacts):
        self.lib, self.desc, self.n_tiles = L.load(), desc, n_tiles
        self.acts, self.dacts = acts, dacts
        self.rows = int(self.lib.nefes_train_rows(C.byref(desc)))
        self.offsets = [int(self.lib.nefes_train_row_offset(C.byref(desc), b)) for b in range(L.TB_END + 1)]
        self.stream = ops._stream()
        self.dev = acts.device
        self.db = {}                                                  # block -> bias gradient (filled by run)
        self.jobs, self.cols = [], 0                                  # declared weight-gradient products, columns of the wide partial buffer

    def off(self, block):                                             # (a method, not a closure: no reference cycle
        return self.offsets[block]                                    #  may keep the multi-GB buffers alive)

    def dx(self, g_block, n_out, w, n_in, dst_block, accumulate, mask, g_rows=None):
        k = (n_out + 7) // 8 * 8
        wt = _pad_t(w, n_in, k)
        L.check(self.lib.nefes_train_dx(self.n_tiles, self.rows, self.dacts.data_ptr(), self.off(g_block), k, wt.data_ptr(), k,
                                        n_in, self.acts.data_ptr(), self.off(dst_block), int(accumulate), int(mask),
                                        self.dacts.data_ptr(), self.stream), "nefes_train_dx")
        return wt                                                     # kept alive by the caller until the stream is done

    def dw(self, g_block, n_out, x_block, n_in, relu, bias=True):
        """Declares sum_s G[o][s] f(X[i][s]) -> handle; handle.v = [n_out_pad, n_in_pad] after run().  The row sums of G (the
        Linear's bias gradient) ride along as one more column of every product's partials; bias=True keeps them in
        self.db[g_block]."""
        op, ip = (n_out + 31) // 32 * 32, (n_in + 31) // 32 * 32
        h = _Product(g_block, op, x_block, ip, bool(relu), bool(bias), self.cols)
        self.cols += op * (ip + 1)
        self.jobs.append(h)
        return h

    def run(self):
        """Launches every declared product into ONE wide partial buffer [splits][all products' columns] (same number of shares
        for all, nefes_train_dw_bias' split_stride) and sums the shares with a single reduction, in a fixed order."""
        big = [_dw_grid(h.op // 32, h.ip // 32)[0] for h in self.jobs if _dw_grid(h.op // 32, h.ip // 32)[1] == 1024]
        splits = max(1, min(self.n_tiles, 1024 // max(big + [1])))
        wide = torch.empty(splits, self.cols, device=self.dev)
        for h in self.jobs:
            L.check(self.lib.nefes_train_dw_bias(self.n_tiles, self.rows, self.dacts.data_ptr(), self.off(h.g_block), h.op,
                                                 self.acts.data_ptr(), self.off(h.x_block), h.ip, int(h.relu), splits, self.cols,
                                                 wide.data_ptr() + 4 * h.col, self.stream), "nefes_train_dw_bias")
        red = wide.sum(0)
        for h in self.jobs:
            out = red[h.col:h.col + h.op * (h.ip + 1)].view(h.op, h.ip + 1)
            h.v = out[:, :h.ip]
            if h.bias:
                self.db[h.g_block] = out[:, h.ip]
        self.jobs = []


class _Product:
    __slots__ = ("g_block", "op", "x_block", "ip", "relu", "bias", "col", "v")

    def __init__(self, g_block, op, x_block, ip, relu, bias, col):
        self.g_block, self.op, self.x_block, self.ip, self.relu, self.bias, self.col, self.v = g_block, op, x_block, ip, relu, bias, col, None


def param_names(net, mode):
    names = [f"xyz_encoding_{i}.0" for i in range(1, 9)] + ["xyz_encoding_final", "dir_encoding.0", "static_sigma.0",
                                                             "static_rgb.0"]
    if mode == L.FIELD_FULL:
        names += ["transient_encoding.0", "transient_encoding.2", "transient_encoding.4", "transient_sigma.0",
                  "transient_rgb.0", "transient_beta.0"]
    return [n + s for n in names for s in (".weight", ".bias")]


def fp16_pipe(pk):
    """The train-mode forward (and the fused dX chain) run on the fp16 two-part instances when ops.SPLIT selects them, the
    network's fp16 streams are current, and the shape has them (both widths x both head classes, frequency embedding): the
    static head's condition."""
    return ops.static_h3(pk)


def ext_pipe(pk):
    """The train-mode instances of a network on an external 32-feature encoding (a hash grid): fp16 two-part pipe, width 256, either
    head class (the TRAIN rows with EXTERNAL32 of csrc/field_h3_instances.h)."""
    return ops.h3_serves(pk) and pk.xyz_encoding == L.XYZ_EXTERNAL32        # (h3_shape: width 256 is the external encoding's only width)


FUSED_DX = True       # one fused backward launch (nefes_field_bwd_train) instead of the layer-by-layer nefes_train_dx chain


def weight_grads(net, pk, mode, N, S, raw_t, g_raw_t, acts, fused=None, ext=False, want_w=True):
    """-> dict parameter name -> gradient (fp32, parameter shape) for every parameter on the path of `mode`.
    fused = (rays_o, rays_d, viewdirs, z, masks): run the dX chain as one fused kernel launch.
    ext: a network on an external 32-feature encoding; fused = (viewdirs, masks), and "__rays__" holds (d encoding [N*S, 32],
    d viewdirs per sample) instead of the per-sample ray gradients.  want_w=False: the dX chain alone (no parameter gradients)."""
    lib, desc = L.load(), pk.desc
    W, Cf = net.W, net.W_features
    C3, H2 = 3 + Cf, W // 2
    full = mode == L.FIELD_FULL
    n_tiles = acts.shape[0]
    dacts = torch.empty_like(acts)
    if not (fused is not None and (ext or fp16_pipe(pk))):    # (the fp16 dX kernel writes the head blocks itself)
        L.check(lib.nefes_train_head_grad(C.byref(desc), mode, N, S, raw_t.data_ptr(), g_raw_t.data_ptr(), dacts.data_ptr(),
                                          ops._stream()), "nefes_train_head_grad")
    P = _Pass(net, desc, n_tiles, acts, dacts)
    sd = dict(net.named_parameters())
    w = lambda name: sd[name + ".weight"]
    keep = []
    TB = lambda l: L.TB_L1 + (l - 1)
    # ---- backward through the layers: dacts rows of every hidden block become d loss / d pre-activation ----
    if ext:
        v, masks = fused
        g_pts, g_vs = torch.empty(N * S, 32, device=acts.device), torch.empty(N * S, 3, device=acts.device)     # (g_pts: d encoding)
        L.check(lib.nefes_field_bwd_train_h3_ext(C.byref(desc), pk.blob.data_ptr(), mode, N, S, v.data_ptr(), raw_t.data_ptr(),
                                                 g_raw_t.data_ptr(), masks.data_ptr(), dacts.data_ptr(), g_pts.data_ptr(), g_vs.data_ptr(),
                                                 ops._stream()), "nefes_field_bwd_train_h3_ext")
    elif fused is not None:
        o, d, v, zz, masks = fused
        g_pts, g_vs = torch.empty(N * S, 3, device=acts.device), torch.empty(N * S, 3, device=acts.device)
        bwd = lib.nefes_field_bwd_train_h3 if fp16_pipe(pk) else lib.nefes_field_bwd_train
        L.check(bwd(C.byref(desc), pk.blob.data_ptr(), mode, N, S, o.data_ptr(), d.data_ptr(), zz.data_ptr(), v.data_ptr(),
                    raw_t.data_ptr(), g_raw_t.data_ptr(), masks.data_ptr(), dacts.data_ptr(), g_pts.data_ptr(), g_vs.data_ptr(),
                    ops._stream()), "nefes_field_bwd_train")
    else:
        if net._embedding_columns():
            # the layer-by-layer chain slices the network's OWN weights at the paper-default embedding widths (63 / 27); a network on
            # fewer octaves has narrower layer-5 / dir_encoding inputs and would hand P.dx the wrong block
            raise NotImplementedError("nefes_amd: networks on a reduced embedding (--reduce_embedding / smaller --multires) train on the "
                                      "fused dX chain only (train.FUSED_DX = True, frequency embedding)")
        if full:
            w_th = torch.cat([w("transient_rgb.0"), w("transient_sigma.0"), w("transient_beta.0")], 0)     # raw channel order
            keep.append(P.dx(L.TB_TH, 5, w_th, H2, L.TB_T2, False, True))
            keep.append(P.dx(L.TB_T2, H2, w("transient_encoding.4"), H2, L.TB_T1, False, True))
            keep.append(P.dx(L.TB_T1, H2, w("transient_encoding.2"), H2, L.TB_T0, False, True))
        keep.append(P.dx(L.TB_RGB, C3, w("static_rgb.0"), H2, L.TB_DIR, False, True))
        keep.append(P.dx(L.TB_DIR, H2, w("dir_encoding.0")[:, :W], W, L.TB_FINAL, False, False))
        if full:
            keep.append(P.dx(L.TB_T0, H2, w("transient_encoding.0")[:, :W], W, L.TB_FINAL, True, False))
        keep.append(P.dx(L.TB_FINAL, W, w("xyz_encoding_final"), W, TB(8), False, False))
        keep.append(P.dx(L.TB_SIG, 1, w("static_sigma.0"), W, TB(8), True, True))
        for l in range(8, 1, -1):
            wl = w(f"xyz_encoding_{l}.0")
            keep.append(P.dx(TB(l), W, wl[:, EMB_XYZ:] if l == 5 else wl, W, TB(l - 1), False, True))
    g = {}
    if not want_w:
        g["__rays__"] = (g_pts, g_vs)
        return g
    # ---- weight gradients ----
    # E block: the frequency embedding's 63 features in slot order (64 rows), or an external encoding's 32 in natural order
    e_idx = torch.arange(32, device=acts.device) if ext else _slot_rows(10, 64, EMB_XYZ, acts.device)
    n_e = 32 if ext else 64
    d_idx = _slot_rows(4, 28, EMB_DIR, acts.device)
    h1 = P.dw(TB(1), W, L.TB_E, n_e, False)
    hl = {l: P.dw(TB(l), W, TB(l - 1), W, True) for l in range(2, 9)}
    h5e = P.dw(TB(5), W, L.TB_E, n_e, False, bias=False)
    hsig, hfin = P.dw(L.TB_SIG, 1, TB(8), W, True), P.dw(L.TB_FINAL, W, TB(8), W, True)
    hdir, hdird = P.dw(L.TB_DIR, H2, L.TB_FINAL, W, False), P.dw(L.TB_DIR, H2, L.TB_DV, 32, False, bias=False)
    hrgb = P.dw(L.TB_RGB, C3, L.TB_DIR, H2, True)
    if full:
        ht0, ht0d = P.dw(L.TB_T0, H2, L.TB_FINAL, W, False), P.dw(L.TB_T0, H2, L.TB_DV, 32, False, bias=False)
        ht1, ht2 = P.dw(L.TB_T1, H2, L.TB_T0, H2, True), P.dw(L.TB_T2, H2, L.TB_T1, H2, True)
        hth = P.dw(L.TB_TH, 5, L.TB_T2, H2, True)
    P.run()
    g["xyz_encoding_1.0.weight"] = h1.v[:W][:, e_idx]
    for l in range(2, 9):
        dh = hl[l].v[:W, :W]
        if l == 5:
            dh = torch.cat([h5e.v[:W][:, e_idx], dh], 1)
        g[f"xyz_encoding_{l}.0.weight"] = dh
    g["static_sigma.0.weight"] = hsig.v[:1, :W]
    g["xyz_encoding_final.weight"] = hfin.v[:W, :W]
    g["dir_encoding.0.weight"] = torch.cat([hdir.v[:H2, :W], hdird.v[:H2][:, d_idx]], 1)
    g["static_rgb.0.weight"] = hrgb.v[:C3, :H2]
    if full:
        g["transient_encoding.0.weight"] = torch.cat([ht0.v[:H2, :W], ht0d.v[:H2][:, d_idx]], 1)
        g["transient_encoding.2.weight"] = ht1.v[:H2, :H2]
        g["transient_encoding.4.weight"] = ht2.v[:H2, :H2]
        d_th = hth.v[:5, :H2]
        g["transient_rgb.0.weight"], g["transient_sigma.0.weight"], g["transient_beta.0.weight"] = d_th[:3], d_th[3:4], d_th[4:5]
    # ---- bias gradients: row sums of the gradient blocks over all samples, summed inside the dW launches ----
    blk = lambda b, n: P.db[b][:n]
    for l in range(1, 9):
        g[f"xyz_encoding_{l}.0.bias"] = blk(TB(l), W)
    g["xyz_encoding_final.bias"], g["dir_encoding.0.bias"] = blk(L.TB_FINAL, W), blk(L.TB_DIR, H2)
    g["static_sigma.0.bias"], g["static_rgb.0.bias"] = blk(L.TB_SIG, 1), blk(L.TB_RGB, C3)
    if full:
        g["transient_encoding.0.bias"], g["transient_encoding.2.bias"] = blk(L.TB_T0, H2), blk(L.TB_T1, H2)
        g["transient_encoding.4.bias"] = blk(L.TB_T2, H2)
        th = blk(L.TB_TH, 5)
        g["transient_rgb.0.bias"], g["transient_sigma.0.bias"], g["transient_beta.0.bias"] = th[:3], th[3:4], th[4:5]
    if DEBUG is not None:
        DEBUG.update(acts=rows_view(acts), dacts=rows_view(dacts), rows=P.rows, off={b: P.off(b) for b in range(19)})
    del keep
    if fused is not None:
        g["__rays__"] = (g_pts, g_vs)          # per-sample d pts / d viewdirs of the fused dX chain (joint pose + weight gradients)
    return g


class FieldTrain(torch.autograd.Function):
    """raw_t [N,R,S] of the field at samples z along the rays, differentiable w.r.t. the network parameters
    (passed as *params in `param_names` order so autograd routes their gradients)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, net, mode, *params):
        pk = net.packed()
        lib = L.load()
        if mode not in (L.FIELD_STATIC, L.FIELD_FULL):
            raise ValueError("nefes_amd: train mode evaluates the static or the full head")
        o, d, v, zz = ops._f32(rays_o), ops._f32(rays_d), ops._f32(viewdirs), ops._f32(z)
        N, S = zz.shape
        R = 3 + pk.feat_dim + (1 if mode == L.FIELD_STATIC else 6)
        n_tiles = (N * S + 127) // 128
        rows = int(lib.nefes_train_rows(C.byref(pk.desc)))
        raw_t = torch.empty(N, R, S, device=zz.device)
        acts = torch.empty(n_tiles, rows, 128, device=zz.device)
        fused = FUSED_DX and pk.xyz_encoding == L.XYZ_FREQ10
        masks = torch.empty(pk.mask_bytes(N * S) // 4, dtype=torch.int32, device=zz.device) if fused else None
        h3 = fused and fp16_pipe(pk)
        if not h3:
            ops.require_instance(pk, "the fp32-MFMA train-mode forward")
            if not ops.canonical_shape(pk):
                raise RuntimeError(f"nefes_amd: train mode for W={pk.width}, f_dim={pk.feat_dim} runs on the fused fp16 two-part "
                                   f"instances only (train.FUSED_DX, NEFES_SPLIT=h3).  Compiled: {ops.COMPILED_SET}")
        fwd = lib.nefes_field_fwd_train_h3 if h3 else lib.nefes_field_fwd_train
        with ops._timed("field_fwd_train[h3]" if h3 else "field_fwd_train"):
            L.check(fwd(C.byref(pk.desc), pk.blob.data_ptr(), mode, N, S, ops._chk(o, "rays_o"), ops._chk(d, "rays_d"),
                        ops._chk(zz, "z"), None, ops._chk(v, "viewdirs"), raw_t.data_ptr(), acts.data_ptr(),
                        None if masks is None else masks.data_ptr(), ops._stream()), "nefes_field_fwd_train")
        if fused:
            ops._tap("masks", (masks, N, S, pk.width, mode))
            ctx.save_for_backward(raw_t, acts, o, d, v, zz, masks)
        else:
            ctx.save_for_backward(raw_t, acts)
        ctx.fused = fused
        if DEBUG is not None:
            DEBUG.update(acts=rows_view(acts), rows=rows, off={b: int(lib.nefes_train_row_offset(C.byref(pk.desc), b)) for b in range(19)})
        ctx.net, ctx.pk, ctx.mode, ctx.NS, ctx.pk_gen = net, pk, mode, (N, S), pk.generation
        return raw_t

    @staticmethod
    def backward(ctx, g_raw_t):
        want_rays = any(ctx.needs_input_grad[:3])
        if ctx.needs_input_grad[3] or (want_rays and not ctx.fused):
            raise NotImplementedError("nefes_amd: gradients w.r.t. the rays in train mode come from the fused dX chain "
                                      "(train.FUSED_DX, frequency embedding); the depths z carry no gradient (rendering.py:139 detaches them)")
        ctx.pk.check_generation(ctx.pk_gen)
        raw_t, acts = ctx.saved_tensors[:2]
        N, S = ctx.NS
        with ops._timed("field_bwd_train[h3]" if (ctx.fused and fp16_pipe(ctx.pk)) else "field_bwd_train"):
            g = weight_grads(ctx.net, ctx.pk, ctx.mode, N, S, raw_t, ops._f32(g_raw_t), acts,
                             fused=tuple(ctx.saved_tensors[2:]) if ctx.fused else None)
        names = param_names(ctx.net, ctx.mode)
        g = ctx.net.shrink_grads(g)            # a network on fewer embedding octaves: drop the columns the kernels padded (field.py)
        g_rays = (None, None, None)
        if want_rays:
            # joint pose + weight gradients (e.g. BARF-style training): the fused dX chain wrote d pts / d viewdirs per sample anyway
            zz = ctx.saved_tensors[5]
            g_pts, g_vs = g["__rays__"]
            g_rays = ops.ray_grad_reduce(N, S, zz, g_pts, g_vs)
        return g_rays + (None,) * 3 + tuple(g[n].contiguous() for n in names)


def field_train(net, mode, rays_o, rays_d, viewdirs, z):
    sd = dict(net.named_parameters())
    return FieldTrain.apply(rays_o, rays_d, viewdirs, z, net, mode, *[sd[n] for n in param_names(net, mode)])


class FieldTrainEncoded(torch.autograd.Function):
    """FieldTrain for a network on an external 32-feature xyz encoding (a hash grid, BASELINE configs[3]): raw_t [N,R,S] from
    enc [N,S,32] and viewdirs [N,3], differentiable w.r.t. enc (-> the grid's table and the sample positions, HashGridEncode),
    viewdirs and the network parameters (*params in `param_names` order).  fp16 two-part train instances, width 256, both head classes."""

    @staticmethod
    def forward(ctx, enc, viewdirs, net, mode, *params):
        pk = net.packed()
        lib = L.load()
        if mode not in (L.FIELD_STATIC, L.FIELD_FULL):
            raise ValueError("nefes_amd: train mode evaluates the static or the full head")
        if not ext_pipe(pk):
            raise NotImplementedError(f"nefes_amd: train mode on an external (hash-grid) encoding is built for width 256 with 3 + f_dim <= 144 "
                                      f"on the fp16 two-part instances (NEFES_SPLIT=h3); got W={pk.width}, f_dim={pk.feat_dim}, "
                                      f"NEFES_SPLIT={ops.SPLIT}.  Compiled: {ops.COMPILED_SET}")
        N, S = enc.shape[0], enc.shape[1]
        if N * S >= ops.H3_MAX_SAMPLES:
            raise RuntimeError("nefes_amd: too many samples for one launch of the fp16 two-part kernels (32-bit sample index)")
        e, v = ops._f32(enc).reshape(N * S, 32), ops._f32(viewdirs)
        R = 3 + pk.feat_dim + (1 if mode == L.FIELD_STATIC else 6)
        n_tiles = (N * S + 127) // 128
        rows = int(lib.nefes_train_rows(C.byref(pk.desc)))
        raw_t = torch.empty(N, R, S, device=e.device)
        acts = torch.empty(n_tiles, rows, 128, device=e.device)
        masks = torch.empty(pk.mask_bytes(N * S) // 4, dtype=torch.int32, device=e.device)
        with ops._timed("field_fwd_train[h3,ext]"):
            L.check(lib.nefes_field_fwd_train_h3_ext(C.byref(pk.desc), pk.blob.data_ptr(), mode, N, S, ops._chk(e, "enc"),
                                                     ops._chk(v, "viewdirs"), raw_t.data_ptr(), acts.data_ptr(), masks.data_ptr(),
                                                     ops._stream()), "nefes_field_fwd_train_h3_ext")
        ops._tap("masks", (masks, N, S, pk.width, mode))
        ctx.save_for_backward(raw_t, acts, v, masks)
        if DEBUG is not None:
            DEBUG.update(acts=rows_view(acts), rows=rows, off={b: int(lib.nefes_train_row_offset(C.byref(pk.desc), b)) for b in range(19)})
        ctx.net, ctx.pk, ctx.mode, ctx.NS, ctx.pk_gen = net, pk, mode, (N, S), pk.generation
        return raw_t

    @staticmethod
    def backward(ctx, g_raw_t):
        ctx.pk.check_generation(ctx.pk_gen)
        raw_t, acts, v, masks = ctx.saved_tensors
        N, S = ctx.NS
        want_w = any(ctx.needs_input_grad[4:])
        with ops._timed("field_bwd_train[h3,ext]"):
            g = weight_grads(ctx.net, ctx.pk, ctx.mode, N, S, raw_t, ops._f32(g_raw_t), acts, fused=(v, masks), ext=True, want_w=want_w)
        g_enc, g_vs = g.pop("__rays__")
        g_v = None
        if ctx.needs_input_grad[1]:
            _, _, g_v = ops.ray_grad_reduce(N, S, torch.zeros(N, S, device=v.device), g_vs, g_vs)
        g_params = (None,) * (len(ctx.needs_input_grad) - 4)
        if want_w:
            g = ctx.net.shrink_grads(g)
            g_params = tuple(g[n].contiguous() if need else None
                             for n, need in zip(param_names(ctx.net, ctx.mode), ctx.needs_input_grad[4:]))
        return (g_enc.reshape(N, S, 32) if ctx.needs_input_grad[0] else None, g_v, None, None) + g_params


def field_train_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z):
    """Train-mode field of a network behind an xyz encoder (ops.HashGrid): pts = o + d z (rendering.py:114,142) -> grid(pts) ->
    FieldTrainEncoded.  Gradients reach the network's parameters, the grid's table (if it requires grad) and the rays (through
    nefes_hashgrid_bwd_x) in one backward."""
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]
    sd = dict(net.named_parameters())
    return FieldTrainEncoded.apply(grid(pts), viewdirs, net, mode, *[sd[n] for n in param_names(net, mode)])


# ---------------------------------------------------------------------------------------------------------------------------------
# Train mode on the generic kernels (csrc/field_generic.hip TRAIN instances): any --netwidth / --netdepth.  Opt-in: ops.GENERIC_TRAIN,
# and ops.GENERIC_TRAIN_EXT behind an xyz encoder (a hash grid).
# ---------------------------------------------------------------------------------------------------------------------------------
class _GenericPass(_Pass):
    """_Pass on the generic row map (nefes_generic_train_row_offset): same declarations, same launches."""

    def __init__(self, pk, n_tiles, acts, dacts):
        self.lib, self.desc, self.n_tiles = L.load(), pk.desc, n_tiles
        self.acts, self.dacts = acts, dacts
        self.rows, self.offsets = pk.train_rows()
        self.stream = ops._stream()
        self.dev = acts.device
        self.db = {}
        self.jobs, self.cols = [], 0


def param_names_generic(net, mode):
    """param_names for a network of any depth: the parameters on the path of `mode`, in nefes_generic_pack's order."""
    names = ops.PackedGeneric.layer_names(net.D, mode == L.FIELD_FULL)
    return [n + s for n in names for s in (".weight", ".bias")]


def generic_train_bytes(pk, M):
    """bytes of the acts + dacts buffers of M samples."""
    return 2 * ((M + 127) // 128) * pk.train_rows()[0] * 128 * 4


def _generic_buffers_fit(pk, N, S, dev):
    need = generic_train_bytes(pk, N * S)
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need > free:
        per_ray = generic_train_bytes(pk, 128 * S) / 128.
        raise RuntimeError(f"nefes_amd: train mode of the generic kernels at W={pk.width}, D={pk.depth} keeps {need} bytes of activations and "
                           f"gradients for {N} rays x {S} samples ({need // (N * S)} per sample); {free} are free.  About "
                           f"{int(free / per_ray)} rays of {S} samples would fit: render fewer rays per step (chunk)")


def _param_grads_generic(pk, mode, acts, dacts):
    """dW = G X^T per layer on nefes_train_dw_bias from the buffers of a generic train-mode forward + backward, for either encoding:
    the E block is the frequency embedding's 63 features in 64 rows, or a supplied encoding's 32 in 32 (pk.xyz_encoding).  `acts` holds
    layer OUTPUTS (after ReLU) and the embeddings in the reference's order: x_relu = 0 everywhere, no slot permutation."""
    W, D, Cf, skip = pk.width, pk.depth, pk.feat_dim, pk.skip
    C3, H2 = 3 + Cf, W // 2
    full = mode == L.FIELD_FULL
    e_rows, n_e = (32, 32) if pk.xyz_encoding == L.XYZ_EXTERNAL32 else (64, EMB_XYZ)
    P = _GenericPass(pk, acts.shape[0], acts, dacts)
    TB = lambda l: L.TB_L1 + (l - 1)
    h = {1: P.dw(TB(1), W, L.TB_E, e_rows, False)}
    he = None
    for l in range(2, D + 1):
        h[l] = P.dw(TB(l), W, TB(l - 1), W, False)
        if l - 1 == skip:                                              # the layer that reads cat([embedding, h]); its bias once
            he = P.dw(TB(l), W, L.TB_E, e_rows, False, bias=False)
    hsig, hfin = P.dw(L.TB_SIG, 1, TB(D), W, False), P.dw(L.TB_FINAL, W, TB(D), W, False)
    hdir, hdird = P.dw(L.TB_DIR, H2, L.TB_FINAL, W, False), P.dw(L.TB_DIR, H2, L.TB_DV, 32, False, bias=False)
    hrgb = P.dw(L.TB_RGB, C3, L.TB_DIR, H2, False)
    if full:
        ht0, ht0d = P.dw(L.TB_T0, H2, L.TB_FINAL, W, False), P.dw(L.TB_T0, H2, L.TB_DV, 32, False, bias=False)
        ht1, ht2 = P.dw(L.TB_T1, H2, L.TB_T0, H2, False), P.dw(L.TB_T2, H2, L.TB_T1, H2, False)
        hth = P.dw(L.TB_TH, 5, L.TB_T2, H2, False)
    P.run()
    g = {"xyz_encoding_1.0.weight": h[1].v[:W, :n_e]}
    for l in range(2, D + 1):
        dh = h[l].v[:W, :W]
        if l - 1 == skip:
            dh = torch.cat([he.v[:W, :n_e], dh], 1)
        g[f"xyz_encoding_{l}.0.weight"] = dh
    g["static_sigma.0.weight"] = hsig.v[:1, :W]
    g["xyz_encoding_final.weight"] = hfin.v[:W, :W]
    g["dir_encoding.0.weight"] = torch.cat([hdir.v[:H2, :W], hdird.v[:H2, :EMB_DIR]], 1)
    g["static_rgb.0.weight"] = hrgb.v[:C3, :H2]
    blk = lambda b, n: P.db[b][:n]
    for l in range(1, D + 1):
        g[f"xyz_encoding_{l}.0.bias"] = blk(TB(l), W)
    g["xyz_encoding_final.bias"], g["dir_encoding.0.bias"] = blk(L.TB_FINAL, W), blk(L.TB_DIR, H2)
    g["static_sigma.0.bias"], g["static_rgb.0.bias"] = blk(L.TB_SIG, 1), blk(L.TB_RGB, C3)
    if full:
        g["transient_encoding.0.weight"] = torch.cat([ht0.v[:H2, :W], ht0d.v[:H2, :EMB_DIR]], 1)
        g["transient_encoding.2.weight"] = ht1.v[:H2, :H2]
        g["transient_encoding.4.weight"] = ht2.v[:H2, :H2]
        d_th, b_th = hth.v[:5, :H2], blk(L.TB_TH, 5)                   # nefes_generic_pack's rows: rgb (3) | sigma | beta
        g["transient_rgb.0.weight"], g["transient_sigma.0.weight"], g["transient_beta.0.weight"] = d_th[:3], d_th[3:4], d_th[4:5]
        g["transient_rgb.0.bias"], g["transient_sigma.0.bias"], g["transient_beta.0.bias"] = b_th[:3], b_th[3:4], b_th[4:5]
        g["transient_encoding.0.bias"], g["transient_encoding.2.bias"] = blk(L.TB_T0, H2), blk(L.TB_T1, H2)
        g["transient_encoding.4.bias"] = blk(L.TB_T2, H2)
    if DEBUG is not None:
        DEBUG.update(acts=rows_view(acts), dacts=rows_view(dacts), rows=P.rows, off={b: P.off(b) for b in range(L.TB_END + 1)})
    return g


def _generic_entry(direction, ext):
    """(C entry point, timer key) of the train-mode launch of `direction` ("fwd" / "bwd") on the frequency embedding or a supplied encoding"""
    return f"nefes_field_{direction}_train_generic" + ("_ext" if ext else ""), f"field_{direction}_train[generic" + (",ext]" if ext else "]")


def _generic_train_pack(net, mode, ext):
    """net.packed_generic() once train mode can evaluate `mode` on it (ext: on a supplied encoding)."""
    pk = net.packed_generic()
    L.load()
    if mode not in (L.FIELD_STATIC, L.FIELD_FULL):
        raise ValueError("nefes_amd: train mode evaluates the static or the full head")
    if mode == L.FIELD_FULL and not pk.has_transient:
        raise ValueError("nefes_amd: the full head of a network without a transient head")
    if ext and pk.xyz_encoding != L.XYZ_EXTERNAL32:
        raise RuntimeError(f"nefes_amd: train mode on a supplied encoding needs a network with in_channels_xyz=32; got {net._shape()}")
    return pk


def _generic_train_forward(ctx, net, pk, mode, N, S, ext, inputs, save):
    """The forward of both generic train Functions: one launch on `inputs` ((name, tensor) in the entry point's order) -> raw_t
    [N,R,S]; ctx keeps (raw_t, acts, *save, masks) for the backward."""
    dev = inputs[0][1].device
    entry, key = _generic_entry("fwd", ext)
    _generic_buffers_fit(pk, N, S, dev)
    rows, off = pk.train_rows()
    raw_t = torch.empty(N, pk.n_raw(mode), S, device=dev)
    acts = torch.empty((N * S + 127) // 128, rows, 128, device=dev)
    masks = torch.empty(pk.mask_bytes(N * S) // 4, dtype=torch.int32, device=dev)
    with ops._timed(key):
        L.check(getattr(L.load(), entry)(pk.desc, pk.blob.data_ptr(), mode, N, S, *[ops._chk(t, n) for n, t in inputs], raw_t.data_ptr(),
                                         acts.data_ptr(), masks.data_ptr(), ops._stream()), entry)
    ops._tap("masks_generic", (masks, N, S, pk, mode))
    ctx.save_for_backward(raw_t, acts, *save, masks)
    if DEBUG is not None:
        DEBUG.update(acts=rows_view(acts), rows=rows, off=dict(enumerate(off)))
    ctx.net, ctx.pk, ctx.mode, ctx.NS, ctx.pk_gen = net, pk, mode, (N, S), pk.generation
    return raw_t


def _generic_train_backward(ctx, g_raw_t, ext, inputs, want_w=True):
    """The backward of both: one fused launch on `inputs` (in the entry point's order; input gradients + every layer's
    pre-activation gradient to `dacts`), then the weight gradients of _param_grads_generic unless want_w is false.  -> (those,
    d loss / d positions [N*S, 3] or d encoding [N*S, 32], d viewdirs per sample)."""
    raw_t, acts, masks = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[-1]
    pk, mode, (N, S), dev = ctx.pk, ctx.mode, ctx.NS, acts.device
    entry, key = _generic_entry("bwd", ext)
    with ops._timed(key):
        g_raw_t = ops._f32(g_raw_t)
        dacts = torch.empty_like(acts)
        g_in, g_vs = torch.empty(N * S, 32 if ext else 3, device=dev), torch.empty(N * S, 3, device=dev)
        L.check(getattr(L.load(), entry)(pk.desc, pk.blob.data_ptr(), mode, N, S, *[t.data_ptr() for t in inputs], raw_t.data_ptr(),
                                         g_raw_t.data_ptr(), masks.data_ptr(), dacts.data_ptr(), g_in.data_ptr(), g_vs.data_ptr(),
                                         ops._stream()), entry)
        g = _param_grads_generic(pk, mode, acts, dacts) if want_w else {}
    return g, g_in, g_vs


class FieldTrainGeneric(torch.autograd.Function):
    """FieldTrain on the generic kernels: raw_t [N,R,S], differentiable w.r.t. the network parameters (*params in
    `param_names_generic` order) and, when asked, the rays."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, net, mode, *params):
        pk = _generic_train_pack(net, mode, ext=False)
        o, d, v, zz = ops._f32(rays_o), ops._f32(rays_d), ops._f32(viewdirs), ops._f32(z)
        N, S = zz.shape
        return _generic_train_forward(ctx, net, pk, mode, N, S, False, (("rays_o", o), ("rays_d", d), ("z", zz), ("viewdirs", v)),
                                      save=(o, d, v, zz))

    @staticmethod
    def backward(ctx, g_raw_t):
        if ctx.needs_input_grad[3]:
            raise NotImplementedError("nefes_amd: the depths z carry no gradient in train mode (rendering.py:139 detaches them)")
        ctx.pk.check_generation(ctx.pk_gen)
        _, _, o, d, v, zz, _ = ctx.saved_tensors
        g, g_pts, g_vs = _generic_train_backward(ctx, g_raw_t, False, (o, d, zz, v))
        N, S = ctx.NS
        g = ctx.net.shrink_grads(g)    # a network on fewer embedding octaves: drop the columns packed_generic padded
        g_rays = (None, None, None)
        if any(ctx.needs_input_grad[:3]):
            g_rays = ops.ray_grad_reduce(N, S, zz, g_pts, g_vs)
        return g_rays + (None,) * 3 + tuple(g[n].contiguous() for n in param_names_generic(ctx.net, ctx.mode))


def field_train_generic(net, mode, rays_o, rays_d, viewdirs, z):
    if not ops.GENERIC_TRAIN:
        net.require_frozen_for_generic("train mode (weight gradients)")
    sd = dict(net.named_parameters())
    return FieldTrainGeneric.apply(rays_o, rays_d, viewdirs, z, net, mode, *[sd[n] for n in param_names_generic(net, mode)])


class FieldTrainGenericEncoded(torch.autograd.Function):
    """FieldTrainEncoded on the generic kernels (net.packed_generic() of a network with in_channels_xyz=32: any width / depth): raw_t
    [N,R,S] from enc [N,S,32] and viewdirs [N,3], differentiable w.r.t. enc (-> the grid's table and the sample positions,
    HashGridEncode), viewdirs and the network parameters (*params in `param_names_generic` order)."""

    @staticmethod
    def forward(ctx, enc, viewdirs, net, mode, *params):
        pk = _generic_train_pack(net, mode, ext=True)
        N, S = enc.shape[0], enc.shape[1]
        e, v = ops._f32(enc).reshape(N * S, 32), ops._f32(viewdirs)
        return _generic_train_forward(ctx, net, pk, mode, N, S, True, (("enc", e), ("viewdirs", v)), save=(v,))

    @staticmethod
    def backward(ctx, g_raw_t):
        ctx.pk.check_generation(ctx.pk_gen)
        v, want_w = ctx.saved_tensors[2], any(ctx.needs_input_grad[4:])
        g, g_enc, g_vs = _generic_train_backward(ctx, g_raw_t, True, (v,), want_w=want_w)
        N, S = ctx.NS
        g_v = None
        if ctx.needs_input_grad[1]:
            _, _, g_v = ops.ray_grad_reduce(N, S, torch.zeros(N, S, device=v.device), g_vs, g_vs)
        g_params = (None,) * (len(ctx.needs_input_grad) - 4)
        if want_w:
            g = ctx.net.shrink_grads(g)
            g_params = tuple(g[n].contiguous() if need else None
                             for n, need in zip(param_names_generic(ctx.net, ctx.mode), ctx.needs_input_grad[4:]))
        return (g_enc.reshape(N, S, 32) if ctx.needs_input_grad[0] else None, g_v, None, None) + g_params


def field_train_generic_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z):
    """field_train_encoded for a network of any width / depth (ops.GENERIC_TRAIN_EXT): pts = o + d z -> grid(pts) ->
    FieldTrainGenericEncoded.  Gradients reach the network's parameters, the grid's table (if it requires grad) and the rays in one
    backward."""
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]
    sd = dict(net.named_parameters())
    return FieldTrainGenericEncoded.apply(grid(pts), viewdirs, net, mode, *[sd[n] for n in param_names_generic(net, mode)])
