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

Four families of kernels run it -- the tuned instances on the fp32 or the fp16 pipe, the tuned instances on a supplied encoding, and
the generic kernels on either input (any width / depth) -- behind four autograd Functions.  Each thing is said once for all of them:
train_route (which entry point), _train_forward / _train_backward (buffers, launches), _dx_fused / _dx_layered (the dX step),
_layer_grads (the layer graph as weight-gradient products; _family holds what the families differ in).
"""
import collections

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
    """The acts / dacts buffers of one backward pass on a pack's row map (pk.train_rows()), the layer-by-layer dX launches and the
    weight-gradient products declared on them."""

    def __init__(self, rows, offsets, n_tiles, acts, dacts):
        self.lib, self.rows, self.offsets, self.n_tiles = L.load(), rows, offsets, n_tiles
        self.acts, self.dacts = acts, dacts
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
        grids = [_dw_grid(h.op // 32, h.ip // 32) for h in self.jobs]
        big = [groups for groups, waves in grids if waves == 1024]
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
    """The parameters on the path of `mode` for a network of any depth, in the packers' order (ops.PackedGeneric.layer_names; depth 8
    gives ops.PackedField.LAYERS_*)."""
    names = ops.PackedGeneric.layer_names(net.D, mode == L.FIELD_FULL)
    return [n + s for n in names for s in (".weight", ".bias")]


param_names_generic = param_names


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


def train_route(pk, direction, ext=False, fused=None):
    """Which kernel serves a train-mode launch -> (the C entry point's name, the timer key).  direction: "fwd" / "bwd"; ext: the input
    is a supplied 32-feature encoding (a hash grid in front); fused: the dX step is one fused launch -- None: what FUSED_DX says now (a
    forward), or what the forward decided (its backward: ctx.fused).  Pure, like ops.field_route: SPLIT and the pack's h3_valid are
    read at call time.  Whether an instance serves the pack at all is _train_pack's question.

        tuned, fp32 MFMA                   nefes_field_{fwd,bwd}_train               field_{fwd,bwd}_train
        tuned, fp16 (fp16_pipe(pk))        nefes_field_{fwd,bwd}_train_h3            field_{fwd,bwd}_train[h3]
        tuned on an encoding               nefes_field_{fwd,bwd}_train_h3_ext        field_{fwd,bwd}_train[h3,ext]
        generic                            nefes_field_{fwd,bwd}_train_generic       field_{fwd,bwd}_train[generic]
        generic on an encoding             nefes_field_{fwd,bwd}_train_generic_ext   field_{fwd,bwd}_train[generic,ext]

    The layer-by-layer dX chain (not fused) reads what the fp32 forward saves: it keeps a tuned network off the fp16 row."""
    if ops.is_generic(pk):
        tags = ("generic", "ext") if ext else ("generic",)
    elif ext:
        tags = ("h3", "ext")
    else:
        tags = ("h3",) if (FUSED_DX if fused is None else fused) and fp16_pipe(pk) else ()
    return "_".join((f"nefes_field_{direction}_train",) + tags), f"field_{direction}_train" + (f"[{','.join(tags)}]" if tags else "")


# ---------------------------------------------------------------------------------------------------------------------------------
# The layer graph: one weight-gradient product per Linear, for every family of kernels
# ---------------------------------------------------------------------------------------------------------------------------------
# What a family of train-mode kernels leaves in `acts`, as far as the weight gradients care:
#   preact     the hidden blocks hold PRE-activations (the tuned kernels): a product whose X block is an activated layer applies the
#              ReLU itself.  False: they hold layer outputs (the generic kernels).
#   e_rows     rows of the E block: the frequency embedding's 63 features in 64, or a supplied encoding's 32 in 32
#   n_e        features of the xyz embedding (columns of xyz_encoding_1 and of the skip layer's first block)
#   xyz_cols, dir_cols   natural embedding feature -> row of the E / DV block (the tuned kernels keep the frequency embeddings in slot
#              order, _slot_rows), or None: the reference's order
#   skip_last  the skip layer's embedding product is declared after the trunk's last layer (tuned) instead of right behind the skip
#              layer's own (generic).  The order decides each product's columns in the wide buffer and the launch order, nothing else.
_Family = collections.namedtuple("_Family", "preact e_rows n_e xyz_cols dir_cols skip_last")
_ACTIVATED = set(range(L.TB_L1, L.TB_FINAL)) | {L.TB_DIR, L.TB_T0, L.TB_T1, L.TB_T2}        # blocks of a Linear with a ReLU behind it


def _family(pk, dev):
    e_rows, n_e = (32, 32) if pk.xyz_encoding == L.XYZ_EXTERNAL32 else (64, EMB_XYZ)
    if ops.is_generic(pk):
        return _Family(False, e_rows, n_e, None, None, False)
    return _Family(True, e_rows, n_e, _slot_rows(10, 64, EMB_XYZ, dev) if n_e == EMB_XYZ else None, _slot_rows(4, 28, EMB_DIR, dev), True)


def _layer_grads(P, fam, W, D, skip, Cf, full):
    """-> {parameter name: gradient (fp32, the kernels' shape)} for every parameter on the path: dW = G X^T per Linear on
    nefes_train_dw_bias from the buffers of a train-mode forward + dX chain, for a trunk of D layers of width W whose layer skip + 1
    reads cat([embedding, h]) (skip < 0: none), a head of 3 + Cf channels and, when `full`, the transient head."""
    C3, H2 = 3 + Cf, W // 2
    TB = lambda l: L.TB_L1 + (l - 1)
    dw = lambda g_block, n_out, x_block, n_in, bias=True: P.dw(g_block, n_out, x_block, n_in, fam.preact and x_block in _ACTIVATED, bias)
    skip_e = lambda: dw(TB(skip + 1), W, L.TB_E, fam.e_rows, bias=False)        # the layer that reads cat([embedding, h]); its bias once
    h, he = {1: dw(TB(1), W, L.TB_E, fam.e_rows)}, None
    for l in range(2, D + 1):
        h[l] = dw(TB(l), W, TB(l - 1), W)
        if l == skip + 1 and not fam.skip_last:
            he = skip_e()
    if skip >= 0 and fam.skip_last:
        he = skip_e()
    hsig, hfin = dw(L.TB_SIG, 1, TB(D), W), dw(L.TB_FINAL, W, TB(D), W)
    hdir, hdird = dw(L.TB_DIR, H2, L.TB_FINAL, W), dw(L.TB_DIR, H2, L.TB_DV, 32, bias=False)
    hrgb = dw(L.TB_RGB, C3, L.TB_DIR, H2)
    if full:
        ht0, ht0d = dw(L.TB_T0, H2, L.TB_FINAL, W), dw(L.TB_T0, H2, L.TB_DV, 32, bias=False)
        ht1, ht2 = dw(L.TB_T1, H2, L.TB_T0, H2), dw(L.TB_T2, H2, L.TB_T1, H2)
        hth = dw(L.TB_TH, 5, L.TB_T2, H2)
    P.run()
    xyz = lambda p: p.v[:W, :fam.n_e] if fam.xyz_cols is None else p.v[:W][:, fam.xyz_cols]
    dirs = lambda p: p.v[:H2, :EMB_DIR] if fam.dir_cols is None else p.v[:H2][:, fam.dir_cols]
    g = {"xyz_encoding_1.0.weight": xyz(h[1])}
    for l in range(2, D + 1):
        dh = h[l].v[:W, :W]
        g[f"xyz_encoding_{l}.0.weight"] = torch.cat([xyz(he), dh], 1) if l == skip + 1 else dh
    g["static_sigma.0.weight"] = hsig.v[:1, :W]
    g["xyz_encoding_final.weight"] = hfin.v[:W, :W]
    g["dir_encoding.0.weight"] = torch.cat([hdir.v[:H2, :W], dirs(hdird)], 1)
    g["static_rgb.0.weight"] = hrgb.v[:C3, :H2]
    # ---- bias gradients: row sums of the gradient blocks over all samples, summed inside the dW launches ----
    blk = lambda b, n: P.db[b][:n]
    for l in range(1, D + 1):
        g[f"xyz_encoding_{l}.0.bias"] = blk(TB(l), W)
    g["xyz_encoding_final.bias"], g["dir_encoding.0.bias"] = blk(L.TB_FINAL, W), blk(L.TB_DIR, H2)
    g["static_sigma.0.bias"], g["static_rgb.0.bias"] = blk(L.TB_SIG, 1), blk(L.TB_RGB, C3)
    if full:
        g["transient_encoding.0.weight"] = torch.cat([ht0.v[:H2, :W], dirs(ht0d)], 1)
        g["transient_encoding.2.weight"] = ht1.v[:H2, :H2]
        g["transient_encoding.4.weight"] = ht2.v[:H2, :H2]
        d_th, b_th = hth.v[:5, :H2], blk(L.TB_TH, 5)                   # the packers' rows (raw channel order): rgb (3) | sigma | beta
        g["transient_rgb.0.weight"], g["transient_sigma.0.weight"], g["transient_beta.0.weight"] = d_th[:3], d_th[3:4], d_th[4:5]
        g["transient_rgb.0.bias"], g["transient_sigma.0.bias"], g["transient_beta.0.bias"] = b_th[:3], b_th[3:4], b_th[4:5]
        g["transient_encoding.0.bias"], g["transient_encoding.2.bias"] = blk(L.TB_T0, H2), blk(L.TB_T1, H2)
        g["transient_encoding.4.bias"] = blk(L.TB_T2, H2)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# The dX step: dacts rows of every hidden block become d loss / d pre-activation
# ---------------------------------------------------------------------------------------------------------------------------------
def _head_grad(pk, mode, N, S, raw_t, g_raw_t, dacts):
    """d raw -> the head blocks of dacts, for the fp32 tuned chains (every other fused kernel writes the head blocks itself)."""
    L.check(L.load().nefes_train_head_grad(pk.desc, mode, N, S, raw_t.data_ptr(), g_raw_t.data_ptr(), dacts.data_ptr(), ops._stream()),
            "nefes_train_head_grad")


def _dx_fused(pk, entry, mode, N, S, ext, inputs, raw_t, g_raw_t, masks, dacts):
    """One fused launch of `entry` (train_route) on `inputs` (tensors in the entry point's order): every layer's pre-activation
    gradient to `dacts` -> (d loss / d positions [N*S, 3] or d encoding [N*S, 32], d viewdirs per sample [N*S, 3])."""
    if entry == "nefes_field_bwd_train":
        _head_grad(pk, mode, N, S, raw_t, g_raw_t, dacts)
    g_in, g_vs = torch.empty(N * S, 32 if ext else 3, device=dacts.device), torch.empty(N * S, 3, device=dacts.device)
    L.check(getattr(L.load(), entry)(pk.desc, pk.blob.data_ptr(), mode, N, S, *[t.data_ptr() for t in inputs], raw_t.data_ptr(),
                                     g_raw_t.data_ptr(), masks.data_ptr(), dacts.data_ptr(), g_in.data_ptr(), g_vs.data_ptr(),
                                     ops._stream()), entry)
    return g_in, g_vs


def _dx_layered(P, net, pk, mode, N, S, raw_t, g_raw_t):
    """The same gradients layer by layer (FUSED_DX off; tuned networks on the fp32 forward): nefes_train_head_grad, then one
    nefes_train_dx per Linear, G_{l-1} = relu'(pre_{l-1}) * W_l^T G_l.  No gradients w.r.t. the rays.  -> the padded weights the
    launches read, to be kept alive until the stream is done."""
    _head_grad(pk, mode, N, S, raw_t, g_raw_t, P.dacts)
    if net._embedding_columns():
        # the layer-by-layer chain slices the network's OWN weights at the paper-default embedding widths (63 / 27); a network on
        # fewer octaves has narrower layer-5 / dir_encoding inputs and would hand P.dx the wrong block
        raise NotImplementedError("nefes_amd: networks on a reduced embedding (--reduce_embedding / smaller --multires) train on the "
                                  "fused dX chain only (train.FUSED_DX = True, frequency embedding)")
    W, C3, H2 = net.W, 3 + net.W_features, net.W // 2
    full = mode == L.FIELD_FULL
    sd = dict(net.named_parameters())
    w = lambda name: sd[name + ".weight"]
    TB = lambda l: L.TB_L1 + (l - 1)
    keep = []
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
    return keep


# ---------------------------------------------------------------------------------------------------------------------------------
# One forward and one backward for the four Functions
# ---------------------------------------------------------------------------------------------------------------------------------
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


def _train_pack(net, mode, ext, generic):
    """net.packed() / net.packed_generic() once train mode can evaluate `mode` on it (ext: on a supplied encoding)."""
    pk = net.packed_generic() if generic else net.packed()
    L.load()
    if mode not in (L.FIELD_STATIC, L.FIELD_FULL):
        raise ValueError("nefes_amd: train mode evaluates the static or the full head")
    if generic:
        if mode == L.FIELD_FULL and not pk.has_transient:
            raise ValueError("nefes_amd: the full head of a network without a transient head")
        if ext and pk.xyz_encoding != L.XYZ_EXTERNAL32:
            raise RuntimeError(f"nefes_amd: train mode on a supplied encoding needs a network with in_channels_xyz=32; got {net._shape()}")
    elif ext:
        if not ext_pipe(pk):
            raise NotImplementedError(f"nefes_amd: train mode on an external (hash-grid) encoding is built for width 256 with 3 + f_dim <= 144 "
                                      f"on the fp16 two-part instances (NEFES_SPLIT=h3); got W={pk.width}, f_dim={pk.feat_dim}, "
                                      f"NEFES_SPLIT={ops.SPLIT}.  Compiled: {ops.COMPILED_SET}")
    elif train_route(pk, "fwd")[0] == "nefes_field_fwd_train":
        ops.require_instance(pk, "the fp32-MFMA train-mode forward")
        if not ops.canonical_shape(pk):
            raise RuntimeError(f"nefes_amd: train mode for W={pk.width}, f_dim={pk.feat_dim} runs on the fused fp16 two-part "
                               f"instances only (train.FUSED_DX, NEFES_SPLIT=h3).  Compiled: {ops.COMPILED_SET}")
    return pk


def _train_forward(ctx, net, pk, mode, N, S, ext, inputs, save):
    """The forward of all four Functions: one launch of train_route's entry point on `inputs` ((name, tensor or None) in its order)
    -> raw_t [N,R,S]; ctx keeps (raw_t, acts, *save, masks) for the backward.  The layer-by-layer dX chain (FUSED_DX off, a tuned
    network on the frequency embedding) takes no ReLU masks: it reads the signs of the saved pre-activations."""
    dev = inputs[0][1].device
    entry, key = train_route(pk, "fwd", ext)
    fused = ops.is_generic(pk) or ext or (FUSED_DX and pk.xyz_encoding == L.XYZ_FREQ10)
    if ops.is_generic(pk):
        _generic_buffers_fit(pk, N, S, dev)
    rows, off = pk.train_rows()
    raw_t = torch.empty(N, pk.n_raw(mode), S, device=dev)
    acts = torch.empty((N * S + 127) // 128, rows, 128, device=dev)
    masks = torch.empty(pk.mask_bytes(N * S) // 4, dtype=torch.int32, device=dev) if fused else None
    with ops._timed(key):
        L.check(getattr(L.load(), entry)(pk.desc, pk.blob.data_ptr(), mode, N, S, *[ops._chk(t, n) for n, t in inputs], raw_t.data_ptr(),
                                         acts.data_ptr(), None if masks is None else masks.data_ptr(), ops._stream()), entry)
    ops._tap_masks(pk, masks, N, S, mode)
    ctx.save_for_backward(raw_t, acts, *save, *(() if masks is None else (masks,)))
    if DEBUG is not None:
        DEBUG.update(acts=rows_view(acts), rows=rows, off=dict(enumerate(off)))
    ctx.net, ctx.pk, ctx.mode, ctx.NS, ctx.pk_gen, ctx.fused = net, pk, mode, (N, S), pk.generation, fused
    return raw_t


def _train_backward(ctx, g_raw_t, ext, inputs, want_w=True):
    """The backward of all four: the dX step (one fused launch on `inputs`, in the entry point's order, or the layered chain), then
    the weight gradients of _layer_grads unless want_w is false.  -> ({parameter name: gradient}, d loss / d positions [N*S, 3] or
    d encoding [N*S, 32], d viewdirs per sample; the last two None after the layered chain)."""
    raw_t, acts = ctx.saved_tensors[:2]
    net, pk, mode, (N, S) = ctx.net, ctx.pk, ctx.mode, ctx.NS
    entry, key = train_route(pk, "bwd", ext, ctx.fused)
    with ops._timed(key):
        g_raw_t = ops._f32(g_raw_t)
        dacts = torch.empty_like(acts)
        rows, off = pk.train_rows()
        P = _Pass(rows, off, acts.shape[0], acts, dacts)
        if ctx.fused:
            keep, (g_in, g_vs) = None, _dx_fused(pk, entry, mode, N, S, ext, inputs, raw_t, g_raw_t, ctx.saved_tensors[-1], dacts)
        else:
            keep, g_in, g_vs = _dx_layered(P, net, pk, mode, N, S, raw_t, g_raw_t), None, None
        g = {}
        if want_w:
            D, skip = (pk.depth, pk.skip) if ops.is_generic(pk) else (8, 4)
            g = _layer_grads(P, _family(pk, acts.device), pk.width, D, skip, pk.feat_dim, mode == L.FIELD_FULL)
            if DEBUG is not None:
                DEBUG.update(acts=rows_view(acts), dacts=rows_view(dacts), rows=rows, off=dict(enumerate(off)))
        del keep
    return g, g_in, g_vs


def _rays_forward(ctx, generic, rays_o, rays_d, viewdirs, z, net, mode):
    pk = _train_pack(net, mode, False, generic)
    o, d, v, zz = ops._f32(rays_o), ops._f32(rays_d), ops._f32(viewdirs), ops._f32(z)
    N, S = zz.shape
    pts = () if generic else (("pts", None),)          # (the tuned ray prototype has a slot for the caller's points)
    return _train_forward(ctx, net, pk, mode, N, S, False, (("rays_o", o), ("rays_d", d), ("z", zz), *pts, ("viewdirs", v)), save=(o, d, v, zz))


def _rays_backward(ctx, g_raw_t):
    want_rays = any(ctx.needs_input_grad[:3])
    if ctx.needs_input_grad[3] or (want_rays and not ctx.fused):
        raise NotImplementedError("nefes_amd: gradients w.r.t. the rays in train mode come from the fused dX chain "
                                  "(train.FUSED_DX, frequency embedding); the depths z carry no gradient (rendering.py:139 detaches them)")
    ctx.pk.check_generation(ctx.pk_gen)
    o, d, v, zz = ctx.saved_tensors[2:6]
    g, g_pts, g_vs = _train_backward(ctx, g_raw_t, False, (o, d, zz, v))
    N, S = ctx.NS
    g = ctx.net.shrink_grads(g)            # a network on fewer embedding octaves: drop the columns the packers padded (field.py)
    g_rays = (None, None, None)
    if want_rays:
        # joint pose + weight gradients (e.g. BARF-style training): the fused dX chain wrote d pts / d viewdirs per sample anyway
        g_rays = ops.ray_grad_reduce(N, S, zz, g_pts, g_vs)
    return g_rays + (None,) * 3 + tuple(g[n].contiguous() for n in param_names(ctx.net, ctx.mode))


def _encoded_forward(ctx, generic, enc, viewdirs, net, mode):
    pk = _train_pack(net, mode, True, generic)
    N, S = enc.shape[0], enc.shape[1]
    if not generic and N * S >= ops.H3_MAX_SAMPLES:
        raise RuntimeError("nefes_amd: too many samples for one launch of the fp16 two-part kernels (32-bit sample index)")
    e, v = ops._f32(enc).reshape(N * S, 32), ops._f32(viewdirs)
    return _train_forward(ctx, net, pk, mode, N, S, True, (("enc", e), ("viewdirs", v)), save=(v,))


def _encoded_backward(ctx, g_raw_t):
    ctx.pk.check_generation(ctx.pk_gen)
    v, want_w = ctx.saved_tensors[2], any(ctx.needs_input_grad[4:])
    g, g_enc, g_vs = _train_backward(ctx, g_raw_t, True, (v,), want_w=want_w)
    N, S = ctx.NS
    g_v = None
    if ctx.needs_input_grad[1]:
        _, _, g_v = ops.ray_grad_reduce(N, S, torch.zeros(N, S, device=v.device), g_vs, g_vs)
    g_params = (None,) * (len(ctx.needs_input_grad) - 4)
    if want_w:
        g = ctx.net.shrink_grads(g)
        g_params = tuple(g[n].contiguous() if need else None
                         for n, need in zip(param_names(ctx.net, ctx.mode), ctx.needs_input_grad[4:]))
    return (g_enc.reshape(N, S, 32) if ctx.needs_input_grad[0] else None, g_v, None, None) + g_params


class FieldTrain(torch.autograd.Function):
    """raw_t [N,R,S] of the field at samples z along the rays, differentiable w.r.t. the network parameters
    (passed as *params in `param_names` order so autograd routes their gradients) and, on the fused dX chain, the rays."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, net, mode, *params):
        return _rays_forward(ctx, False, rays_o, rays_d, viewdirs, z, net, mode)

    backward = staticmethod(_rays_backward)


class FieldTrainEncoded(torch.autograd.Function):
    """FieldTrain for a network on an external 32-feature xyz encoding (a hash grid, BASELINE configs[3]): raw_t [N,R,S] from
    enc [N,S,32] and viewdirs [N,3], differentiable w.r.t. enc (-> the grid's table and the sample positions, HashGridEncode),
    viewdirs and the network parameters (*params in `param_names` order).  fp16 two-part train instances, width 256, both head classes."""

    @staticmethod
    def forward(ctx, enc, viewdirs, net, mode, *params):
        return _encoded_forward(ctx, False, enc, viewdirs, net, mode)

    backward = staticmethod(_encoded_backward)


# Train mode on the generic kernels (csrc/field_generic.hip TRAIN instances): any --netwidth / --netdepth.  Opt-in: ops.GENERIC_TRAIN,
# and ops.GENERIC_TRAIN_EXT behind an xyz encoder (a hash grid).
class FieldTrainGeneric(torch.autograd.Function):
    """FieldTrain on the generic kernels (net.packed_generic()): same inputs, outputs and gradients."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, net, mode, *params):
        return _rays_forward(ctx, True, rays_o, rays_d, viewdirs, z, net, mode)

    backward = staticmethod(_rays_backward)


class FieldTrainGenericEncoded(torch.autograd.Function):
    """FieldTrainEncoded on the generic kernels (net.packed_generic() of a network with in_channels_xyz=32: any width / depth)."""

    @staticmethod
    def forward(ctx, enc, viewdirs, net, mode, *params):
        return _encoded_forward(ctx, True, enc, viewdirs, net, mode)

    backward = staticmethod(_encoded_backward)


def _params(net, mode):
    sd = dict(net.named_parameters())
    return [sd[n] for n in param_names(net, mode)]


def _require_generic_train(net, ext):
    """The generic kernels' train mode is opt-in: ops.GENERIC_TRAIN, or, behind an xyz encoder, ops.GENERIC_TRAIN_EXT alone."""
    if not (ops.GENERIC_TRAIN_EXT if ext else ops.GENERIC_TRAIN):
        net.require_frozen_for_generic("train mode (weight gradients)")


def field_train(net, mode, rays_o, rays_d, viewdirs, z):
    return FieldTrain.apply(rays_o, rays_d, viewdirs, z, net, mode, *_params(net, mode))


def field_train_generic(net, mode, rays_o, rays_d, viewdirs, z):
    _require_generic_train(net, False)
    return FieldTrainGeneric.apply(rays_o, rays_d, viewdirs, z, net, mode, *_params(net, mode))


def _behind_grid(Function, net, mode, grid, rays_o, rays_d, viewdirs, z):
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]         # rendering.py:114,142
    return Function.apply(grid(pts), viewdirs, net, mode, *_params(net, mode))


def field_train_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z):
    """Train-mode field of a network behind an xyz encoder (ops.HashGrid): pts = o + d z -> grid(pts) -> FieldTrainEncoded.  Gradients
    reach the network's parameters, the grid's table (if it requires grad) and the rays (through nefes_hashgrid_bwd_x) in one backward."""
    return _behind_grid(FieldTrainEncoded, net, mode, grid, rays_o, rays_d, viewdirs, z)


def field_train_generic_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z):
    """field_train_encoded for a network of any width / depth (ops.GENERIC_TRAIN_EXT), on FieldTrainGenericEncoded."""
    return _behind_grid(FieldTrainGenericEncoded, net, mode, grid, rays_o, rays_d, viewdirs, z)


def field_train_any(net, pk, mode, grid, rays_o, rays_d, viewdirs, z):
    """The train-mode field on whichever kernels `pk` was packed for (NeRFH_NFF.packed_any), behind the xyz encoder `grid` or, with
    None, on the frequency embedding: what render() calls for a network that trains."""
    if ops.is_generic(pk):
        if grid is None:
            return field_train_generic(net, mode, rays_o, rays_d, viewdirs, z)
        _require_generic_train(net, True)
        return field_train_generic_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z)
    if grid is None:
        return field_train(net, mode, rays_o, rays_d, viewdirs, z)
    return field_train_encoded(net, mode, grid, rays_o, rays_d, viewdirs, z)
