"""Per-sample float64 statement of the field network for the fp16 two-part inference instances (nefes_amd/csrc/field_h3_instances.h):
inputs whose points are exact in fp32, the networks, the per-sample scales, a CPU emulation of the split products with mutants, and the
census of rows.  tests/test_field_ref.py checks this file on the CPU; tests/test_gpu_field_samples.py holds every TRAIN = 0 row to it.
No GPU and no nefes_amd.ops here.

The rule (both tests): for every output group g, pooled over all samples of a case,

    E_x[g] = max_m |x - float64| / s[m, g]          x = the kernels (E_hip), the fp32 oracle (E_ref), the emulation (E_emu)
    E_hip[g] <= F * E_ref[g],  F = 3                (the factor tests/test_gpu_h3.py applies to these kernels), no absolute floor.

Exact points.  rays_o are multiples of 2^-7, rays_d of 2^-6, z of 2^-5 (times one power of two per ray), so o + d z is exact in fp32 and
the float64 oracle sees the kernels' own points bit for bit: what is left is the arithmetic of the network, not the rounding of the
points amplified 2^9 by the embedding.  exact() asserts it for every case.

Scales.  For channel c of sample m with final product W h + b:  s_pre[m, c] = sum_j |W[c, j]| |h[m, j]| + |b[c]|  in float64.
  static head (no activation)       s = max_c s_pre[m, c]
  softplus / sigmoid channels       s = f'(pre) s_pre + |out|     first-order image of a pre-activation error + the scale of the
                                    (+ TINY, below)               activation's own fp32 rounding
  d pts, coordinate a               sum_k 2^k (|cos 2^k x_a| |g_sin,k,a| + |sin 2^k x_a| |g_cos,k,a|) + |g_id,a|, max over a
  d viewdirs                        the same with four frequencies
  d enc                             sum_j |W1[j, f]| |g_pre1[m, j]| + the skip layer's share, max over f
Derived to first order, never measured on the kernels."""
import collections
import re

import torch
import torch.nn.functional as Fn

from oracle import ref_cpu as O
from tests.test_h3_instances import table_rows

F = 3.0
# fp32 keeps 24 bits only down to 2^-126: below it a result is a subnormal or flushed, an ABSOLUTE error of up to 2^-126 = u 2^-102 with
# u = 2^-24.  Added to the scale of the activated channels, whose softplus / sigmoid outputs reach that range when saturated.
TINY = 2.0 ** -102
SHAPES = ((1, 1), (3, 43), (5, 64), (7, 33))       # 129 = one past a 128-sample tile, 320 = 2 1/2 tiles, 231 ragged against 128 and 32
INPUT_SETS = ("plain", "tiny_and_far")             # + "one": the (1, 1) shape of either
EDITS = ("plain", "sigma40", "rescale", "dead3")
HIDDEN = tuple(f"L{i}" for i in range(1, 9)) + ("DIR", "T0", "T1", "T2")
LAYER_OF = dict({f"L{i}": f"xyz_encoding_{i}.0" for i in range(1, 9)}, DIR="dir_encoding.0", T0="transient_encoding.0",
                T1="transient_encoding.2", T2="transient_encoding.4")
# (C, edit) per head class of csrc/layout.h: 29 / 30 / 141 put the last feature channel in the partial k-group of the class.
# C = 0 is left out: NeRFH_NFF itself refuses a network without a feature head (field.py _supported), only the factored-head pack has
# feat_dim 0, and that one is the FH row's.
NETS_OF_CLASS = {0: ((16, "plain"), (1, "sigma40"), (29, "rescale"), (16, "dead3")),
                 1: ((128, "plain"), (30, "sigma40"), (141, "rescale"), (128, "dead3")),
                 "fh": ((128, "plain"), (141, "sigma40"), (96, "rescale"), (128, "dead3"))}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def exact(o, d, z):
    """pts [N, S, 3] fp32 = o + d z, asserted equal to the float64 value for every sample."""
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    p64 = o.double()[:, None, :] + d.double()[:, None, :] * z.double()[..., None]
    assert pts.dtype == torch.float32 and torch.equal(pts.double(), p64), "o + d z is not exact in fp32: the inputs left the dyadic grid"
    return pts


def _dyadic(g, shape, lo, hi, step_log2):
    n = torch.randint(int(lo * 2 ** -step_log2), int(hi * 2 ** -step_log2) + 1, shape, generator=g)
    return n.float() * 2.0 ** step_log2


def rays(kind, N, S, seed=0, dyadic_z=True):
    """(rays_o [N,3], rays_d [N,3], z [N,S] sorted, viewdirs [N,3]) fp32 on the dyadic grid.  plain: |pts| <= 6.  tiny_and_far: rays
    0, 3, 6.. scaled by 2^-13 (o and z), rays 1, 4, 7.. moved out to |o| in [5, 69] (tests/test_gpu_h3.py's stress inputs with powers
    of two).  dyadic_z=False draws z off the grid (tests/test_field_ref.py: exact() must refuse it).  viewdirs are arbitrary fp32 unit vectors, handed identically to both sides."""
    g = torch.Generator().manual_seed(7000 + 131 * N + S + 100003 * seed + (17 if kind != "plain" else 0))
    o, d = _dyadic(g, (N, 3), -2, 2, -7), _dyadic(g, (N, 3), -1, 1, -6)
    z = torch.sort(_dyadic(g, (N, S), 0, 4, -5) if dyadic_z else torch.rand(N, S, generator=g) * 4, -1)[0]
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    if kind == "tiny_and_far":
        o[0::3] *= 2.0 ** -13
        z[0::3] *= 2.0 ** -13
        o[1::3] = torch.where(o[1::3] < 0, -5 - 32 * o[1::3].abs(), 5 + 32 * o[1::3].abs())
    elif kind != "plain":
        raise KeyError(kind)
    return o, d, z, v


def encodings(kind, N, S, seed=0):
    """(enc [N*S, 32], viewdirs [N, 3]) for the rows on a SUPPLIED encoding: arbitrary fp32 values; tiny_and_far: a third of the rays
    at 2^-13 (a hash grid's initialisation scale), a third at 2^8."""
    g = torch.Generator().manual_seed(9000 + 131 * N + S + 100003 * seed)
    enc = (torch.randn(N, S, 32, generator=g) * 0.5)
    if kind == "tiny_and_far":
        enc[0::3] *= 2.0 ** -13
        enc[1::3] *= 2.0 ** 8
    return enc.reshape(N * S, 32).contiguous(), torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)


# ---- networks -------------------------------------------------------------------------------------------------------------------------
def make_net(Wd, C, has_t, ext, edit, seed=0):
    """oracle.ref_cpu.make_field_params (fp32) + one edit of tests/test_gpu_h3.py: static_sigma x 40 (sigma spans [0, 50]), the per-layer
    1e3 / 1e-3 rescale (activations from 1e-9 to 1e9 through the trunk), layer 3 dead (every unit negative)."""
    p = O.make_field_params("fine" if has_t else "coarse", Wd, C, seed=seed, in_xyz=32 if ext else 63)
    if edit == "sigma40":
        p["static_sigma.0.weight"] *= 40.
        p["static_sigma.0.bias"] *= 40.
    elif edit == "rescale":
        for i, f in zip(range(1, 9), (1e3, 1e-3, 1e3, 1e3, 1e-3, 1e-3, 1e3, 1e-3)):
            p[f"xyz_encoding_{i}.0.weight"] *= f
            p[f"xyz_encoding_{i}.0.bias"] *= f if i > 1 else 1.
        p["dir_encoding.0.weight"] *= 1e-2
        if has_t:
            p["transient_encoding.2.weight"] *= 1e3
    elif edit == "dead3":
        p["xyz_encoding_3.0.bias"].fill_(-1e3)
    elif edit != "plain":
        raise KeyError(edit)
    return p


def to(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


def embed(pts, dirs):
    """the 10 / 4-frequency embeddings of flat points [M, 3] and per-sample view directions [M, 3], in their dtype"""
    return O.freq_encode(pts, 10), O.freq_encode(dirs, 4)


def per_sample(v, S):
    return v[:, None, :].expand(v.shape[0], S, 3).reshape(-1, 3)


# ---- the network on embedded inputs, every pre-activation and hidden activation collected ------------------------------------------------
Run = collections.namedtuple("Run", "out pre act")


def run(p, e_xyz, e_dir, mode, neg=None, fh=False, keep_grads=False):
    """O.field_forward (what O.query_field calls after embedding) with its `act` hook: out [M, R] in the kernels' channel order, pre /
    act: {tag: [M, units]}.  neg: {tag: bool [M, units]} evaluates the network ON that ReLU pattern (True = unit off).  fh: the factored
    head's layout rgb | relu(dir_encoding) | ones | sigma | transient (5) (csrc/field_fwd_h3.hip FH), p holding three static_rgb rows."""
    pre, act = {}, {}

    def hook(tag, x):
        if keep_grads:
            x.retain_grad()
        pre[tag] = x
        act[tag] = torch.relu(x) if neg is None else x * (~neg[tag]).to(x.dtype)
        return act[tag]
    x = e_xyz if mode == "SIGMA" else torch.cat([e_xyz, e_dir], 1)
    out = O.field_forward(p, x, sigma_only=mode == "SIGMA", output_transient=mode == "FULL", in_xyz=e_xyz.shape[1], in_dir=27, act=hook)
    if fh:
        out = torch.cat([out[:, :3], act["DIR"], torch.ones_like(out[:, :1]), out[:, 3:]], 1)
    return Run(out, pre, act)


def _abs_lin(p, name, x):
    return x.abs() @ p[name + ".weight"].abs().t() + p[name + ".bias"].abs()


def _lin(p, name, x):
    return Fn.linear(x, p[name + ".weight"], p[name + ".bias"])


def layer_inputs(p, r, e_xyz, e_dir):
    """{tag: the input of that hidden layer's product} from a run's activations"""
    a = r.act
    x = {"L1": e_xyz}
    for i in range(2, 9):
        x[f"L{i}"] = torch.cat([e_xyz, a["L4"]], 1) if i == 5 else a[f"L{i - 1}"]
    if "DIR" in a:
        x["DIR"] = torch.cat([_lin(p, "xyz_encoding_final", a["L8"]), e_dir], 1)
    if "T0" in a:
        x.update(T0=x["DIR"], T1=a["T0"], T2=a["T1"])
    return x


def hidden_scales(p, r, e_xyz, e_dir):
    """{tag: s_pre [M, units]} of every hidden product (float64 run)"""
    return {t: _abs_lin(p, LAYER_OF[t], x) for t, x in layer_inputs(p, r, e_xyz, e_dir).items()}


def forward_groups(p, r, mode, fh=False, e_dir=None):
    """[(group, channel slice of out, s [M, channels or 1])] of a float64 run -- the five output groups (+ the FH row's g channels)."""
    a = r.act
    sp, sg = lambda x: torch.sigmoid(x), lambda x: torch.sigmoid(x) * (1 - torch.sigmoid(x))
    pre_s, s_pre_s = _lin(p, "static_sigma.0", a["L8"]), _abs_lin(p, "static_sigma.0", a["L8"])
    s_sigma = sp(pre_s) * s_pre_s + Fn.softplus(pre_s) + TINY
    if mode == "SIGMA":
        return [("static_sigma", slice(0, 1), s_sigma)]
    H = p["static_rgb.0.weight"].shape[0]
    groups = [("static_head", slice(0, H), _abs_lin(p, "static_rgb.0", a["DIR"]).amax(1, keepdim=True))]
    at = H
    if fh:
        G = a["DIR"].shape[1]
        x_dir = torch.cat([_lin(p, "xyz_encoding_final", a["L8"]), e_dir], 1)
        groups.append(("g", slice(H, H + G), _abs_lin(p, "dir_encoding.0", x_dir).amax(1, keepdim=True)))
        at = H + G + 1                                           # the ones channel is asserted exactly, not scaled
    groups.append(("static_sigma", slice(at, at + 1), s_sigma))
    if mode == "FULL":
        t = a["T2"]
        for name, lay, n, d1, f in (("transient_rgb", "transient_rgb.0", 3, sg, torch.sigmoid), ("transient_sigma", "transient_sigma.0", 1, sp, Fn.softplus),
                                    ("transient_beta", "transient_beta.0", 1, sp, Fn.softplus)):
            pre = _lin(p, lay, t)
            groups.append((name, slice(at + 1, at + 1 + n), d1(pre) * _abs_lin(p, lay, t) + f(pre).abs() + TINY))
            at += n
    return groups


def errors(x, truth, groups):
    """{group: max_m max_c |x - truth| / s}"""
    return {g: float(((x[:, sl].double() - truth[:, sl]).abs() / s).max()) for g, sl, s in groups}


class Case64:
    """One network on one batch: float64 truth + fp32 oracle of the forward, and the backward of either on a GIVEN ReLU pattern."""

    def __init__(self, p32, mode, pts=None, enc=None, dirs=None, fh=False):
        self.p32, self.p64, self.mode, self.fh, self.ext = p32, to(p32, torch.float64), mode, fh, enc is not None
        self.x32, self.dirs32 = (enc if self.ext else pts), dirs
        self.M = self.x32.shape[0]
        self.e64 = self._embed(torch.float64)
        self.e32 = self._embed(torch.float32)
        with torch.no_grad():
            self.r64, self.r32 = self._run(self.p64, self.e64), self._run(self.p32, self.e32)
            self.groups = forward_groups(self.p64, self.r64, mode, fh, self.e64[1])
            self.s_hidden = hidden_scales(self.p64, self.r64, *self.e64)
        self.truth = self.r64.out
        self.e_ref = errors(self.r32.out, self.truth, self.groups)
        # E_ref of every hidden layer's pre-activations, for the mask words
        self.e_ref_layer = {t: float(((self.r32.pre[t].double() - self.r64.pre[t]).abs() / s).max()) for t, s in self.s_hidden.items()}

    def _embed(self, dtype):
        x = self.x32.to(dtype)
        if self.mode == "SIGMA":
            return (x if self.ext else O.freq_encode(x, 10)), None
        return (x if self.ext else O.freq_encode(x, 10)), O.freq_encode(self.dirs32.to(dtype), 4)

    def _run(self, p, e, neg=None, keep_grads=False):
        return run(p, e[0], e[1], self.mode, neg, self.fh, keep_grads)

    def mask_flips(self, neg):
        """units whose mask bit differs from the sign of the float64 pre-activation -> (count, worst |pre| / (F E_ref_layer s_pre))"""
        n, worst = 0, 0.0
        for t, s in self.s_hidden.items():
            pre = self.r64.pre[t]
            flip = (pre < 0) != neg[t]
            if bool(flip.any()):
                n += int(flip.sum())
                worst = max(worst, float((pre.abs() / (F * self.e_ref_layer[t] * s))[flip].max()))
        return n, worst

    ACTIVATED = {"static_sigma": ("static_sigma.0", "L8", "softplus"), "transient_rgb": ("transient_rgb.0", "T2", "sigmoid"),
                 "transient_sigma": ("transient_sigma.0", "T2", "softplus"), "transient_beta": ("transient_beta.0", "T2", "softplus")}

    def backward(self, dtype, neg, G, raw=None):
        """d sum(G * out) / d (pts | enc) and / d viewdirs per sample on the pattern `neg`, with the embedding a leaf:
        {name: (value [M, k], scale [M, 1] (float64 only))}.
        raw [M, R] fp32: the forward outputs the backward under test is HANDED.  The activation derivatives are then formed from them,
        in `dtype`: sigmoid' = y (1 - y), softplus' = -expm1(-y) -- the statement of a backward whose inputs are (upstream, raw, masks),
        as exact points are the statement of a forward whose inputs are fp32.  Without it the derivative comes from the oracle's own
        pre-activation, and where an activation saturates (y rounds to 1) no function of the fp32 output can follow that: the fp32
        oracle's own autograd, which also forms y (1 - y), then sits at E_ref ~ 1 and the rule accepts anything."""
        p = self.p64 if dtype == torch.float64 else self.p32
        x = self.x32.detach().to(dtype, copy=True).requires_grad_()
        dirs = self.dirs32.detach().to(dtype, copy=True).requires_grad_()
        e_x = x if self.ext else O.freq_encode(x, 10)
        e_d = O.freq_encode(dirs, 4)
        lx, ld = (e_x if self.ext else e_x.detach().requires_grad_()), e_d.detach().requires_grad_()
        r = self._run(p, (lx, ld), neg, keep_grads=True)
        out_ = r.out
        if raw is not None:
            cols = [out_[:, i] for i in range(out_.shape[1])]
            for g, sl, _ in self.groups:
                if g in self.ACTIVATED:
                    lay, tag, kind = self.ACTIVATED[g]
                    y = raw[:, sl].to(dtype)
                    d = y * (1 - y) if kind == "sigmoid" else -torch.expm1(-y)
                    pre = _lin(p, lay, r.act[tag])
                    for j, i in enumerate(range(sl.start, sl.stop)):
                        cols[i] = pre[:, j] * d[:, j]                # linear in the pre-activation, with the handed derivative
            out_ = torch.stack(cols, 1)
        (out_ * G.to(dtype)).sum().backward()
        out = {}
        gd = ld.grad
        (g_dirs,) = torch.autograd.grad(e_d, dirs, gd)
        out["d_viewdirs"] = (g_dirs.detach(), _embedding_scale(dirs.detach(), gd, 4))
        if self.ext:
            w1, w5 = p["xyz_encoding_1.0.weight"].abs(), p["xyz_encoding_5.0.weight"].abs()[:, :32]
            s = r.pre["L1"].grad.abs() @ w1 + r.pre["L5"].grad.abs() @ w5
            out["d_enc"] = (x.grad.detach(), s.amax(1, keepdim=True))
        else:
            (g_pts,) = torch.autograd.grad(e_x, x, lx.grad)
            out["d_pts"] = (g_pts.detach(), _embedding_scale(x.detach(), lx.grad, 10))
        return out


def _embedding_scale(x, g_e, n_freq):
    s = g_e[:, :3].abs()
    for k in range(n_freq):
        gs, gc = g_e[:, 3 + 6 * k:6 + 6 * k].abs(), g_e[:, 6 + 6 * k:9 + 6 * k].abs()
        s = s + 2.0 ** k * (torch.cos(2.0 ** k * x).abs() * gs + torch.sin(2.0 ** k * x).abs() * gc)
    return s.amax(1, keepdim=True)


def grad_errors(got, truth):
    """{name: max_m max_a |got - truth| / s[m]}, 0 / 0 = 0 (a sample no gradient reaches)"""
    out = {}
    for k, (t, s) in truth.items():
        err = (got[k].double() - t).abs().amax(1, keepdim=True)
        out[k] = float(torch.where(err == 0, torch.zeros_like(err), err / s).max())
    return out


def upstreams(M, R, feat, sigma, seed=0, dead=None):
    """[(name, G [M, R])]: dense random, then one channel at a time: the first and last feature channel (feat = (first, last)), the first
    colour channel, sigma and every transient channel behind it (tests/test_gpu_hashgrid_c128.py::
    test_backward_one_upstream_channel_at_a_time at every row).  dead: a channel that carries no gradient (the FH row's ones)."""
    g = torch.Generator().manual_seed(4000 + seed + R)
    dense = torch.randn(M, R, generator=g)
    if dead is not None:
        dense[:, dead] = 0
    out = [("dense", dense)]
    for c in dict.fromkeys([feat[0], feat[1], 0, sigma] + list(range(sigma + 1, R))):
        one = torch.zeros(M, R)
        one[:, c] = torch.randn(M, generator=g)
        out.append((f"ch{c}", one))
    return out


# ---- the fp16 two-part products emulated on the CPU (csrc/field_h3.h lines 4-24; tools/fp16x3_accuracy.py) -------------------------------
def _pow2(amax, target):
    return torch.exp2(target - torch.floor(torch.log2(amax.clamp_min(2.0 ** -100))))


def _split(x, truncate):
    h = x.to(torch.float16).float()
    r = x - h
    if truncate:                                                   # the lo part cut to eleven bits, not rounded
        r = (r.view(torch.int32) & ~0x1FFF).view(torch.float32)
    return h, r.to(torch.float16).float()


def product(X, W, mut=()):
    """X [M, K] @ W [K', K]^T in fp32 as hh + hl + lh of RNE fp16 parts: W scaled per matrix (max |w| -> [2^14, 2^15)), X per sample
    three binades lower (the loose bound of field_h3.h:13-19).  mut: the mutations that apply to THIS product."""
    if "shift_sample" in mut:
        X = torch.roll(X, -1, 0)
    sw = _pow2(W.abs().max(), 14)
    amax = X.abs().amax(1, keepdim=True)
    if "scale_per_tile" in mut:                                    # one exponent for 32 samples
        M = X.shape[0]
        pad = torch.cat([amax, amax.new_zeros((-M) % 32, 1)]).view(-1, 32).amax(1, keepdim=True)
        amax = pad.expand(-1, 32).reshape(-1, 1)[:M]
    sx = _pow2(amax, 11)
    wh, wl = _split(W * sw, "truncate_lo" in mut)
    xh, xl = _split(X * sx, "truncate_lo" in mut)
    y = xh @ wh.t() + xl @ wh.t()
    if "drop_lh" not in mut:
        y = y + xh @ wl.t()
    return y / sw / sx


MUTATIONS = ("drop_lh", "truncate_lo", "scale_per_tile", "shift_sample")
MUTATED_LAYERS = ("xyz_encoding_5.0", "static_sigma.0", "static_rgb.0", "transient_encoding.2")
# (mutation, layer) the rule does NOT tell apart on any input set (tests/test_field_ref.py asserts detection of every other one and
# records these; profiles/field_samples/README.md says why):
#   truncate_lo       x - hi has at most 13 significant bits, cutting it to 11 moves a product by 2^-22 of ONE term, with random sign
#                     over 128..319 terms: under the fp32 oracle's own error relative to the abs-sum
#   scale_per_tile    fp16 parts are floating point: a sample 2^-k below its tile's maximum loses bits only through the subnormal
#                     floor (2^-24 absolute), i.e. for k > 13.  Hidden activations of neighbouring samples never differ that much (the
#                     embedding holds cos terms of size 1 for every sample).  A SUPPLIED encoding does (tiny next to large rays) and the
#                     first layer's product is then further from float64 on the small samples -- but that product sits under the
#                     layer's bias and seven more layers, and the outputs move by less than the fp32 oracle's own error.
NOT_TOLD_APART = frozenset((m, l) for m in ("truncate_lo", "scale_per_tile") for l in MUTATED_LAYERS + ("ext:xyz_encoding_1.0",))


def emulate(p, inputs, mode="FULL", mutation=None, G=None, neg=None):
    """The network in fp32 with every product emulated.  inputs: (e_xyz, e_dir) fp32 embedded; mutation: None or (kind, layer name);
    -> Run, and with an upstream G also {d_e_xyz, d_e_dir}: the backward (G @ W split the same way) on the pattern `neg` (default: the
    emulated forward's own)."""
    e_xyz, e_dir = inputs
    kind, layer = mutation if mutation else (None, None)
    mut = lambda name: (kind,) if name == layer else ()
    lin = lambda name, x: product(x, p[name + ".weight"], mut(name)) + p[name + ".bias"]
    pre, act = {}, {}

    def hidden(tag, x):
        pre[tag] = lin(LAYER_OF[tag], x)
        act[tag] = torch.relu(pre[tag]) if neg is None else pre[tag] * (~neg[tag]).float()
        return act[tag]
    h = e_xyz
    for i in range(1, 9):
        h = hidden(f"L{i}", torch.cat([e_xyz, h], 1) if i == 5 else h)
    pre_sigma = lin("static_sigma.0", h)
    outs = [Fn.softplus(pre_sigma)]
    if mode != "SIGMA":
        x_dir = torch.cat([lin("xyz_encoding_final", h), e_dir], 1)
        outs = [lin("static_rgb.0", hidden("DIR", x_dir))] + outs
    if mode == "FULL":
        t = hidden("T2", hidden("T1", hidden("T0", x_dir)))
        pre_t = torch.cat([lin("transient_rgb.0", t), lin("transient_sigma.0", t), lin("transient_beta.0", t)], 1)
        outs += [torch.sigmoid(pre_t[:, :3]), Fn.softplus(pre_t[:, 3:])]
    r = Run(torch.cat(outs, 1), pre, act)
    if G is None:
        return r
    # backward: the same products transposed, on the forward's pattern
    on = {t: (pre[t] >= 0).float() if neg is None else (~neg[t]).float() for t in pre}
    back = lambda name, g: product(g, p[name + ".weight"].t().contiguous(), mut(name))
    H = p["static_rgb.0.weight"].shape[0]
    g_sigma = G[:, H:H + 1] * torch.sigmoid(pre_sigma)
    g_xdir = back("dir_encoding.0", back("static_rgb.0", G[:, :H]) * on["DIR"])
    if mode == "FULL":
        s3 = torch.sigmoid(pre_t[:, :3])
        g_pre_t = torch.cat([G[:, H + 1:H + 4] * s3 * (1 - s3), G[:, H + 4:] * torch.sigmoid(pre_t[:, 3:])], 1)
        g_t = (back("transient_rgb.0", g_pre_t[:, :3]) + back("transient_sigma.0", g_pre_t[:, 3:4]) + back("transient_beta.0", g_pre_t[:, 4:5]))
        g_t = back("transient_encoding.2", back("transient_encoding.4", g_t * on["T2"]) * on["T1"])
        g_xdir = g_xdir + back("transient_encoding.0", g_t * on["T0"])
    Wd = h.shape[1]
    g_h = back("xyz_encoding_final", g_xdir[:, :Wd]) + back("static_sigma.0", g_sigma)
    g_e = torch.zeros_like(e_xyz)
    for i in range(8, 0, -1):
        g_in = back(f"xyz_encoding_{i}.0", g_h * on[f"L{i}"])
        if i == 5:
            g_e, g_h = g_e + g_in[:, :e_xyz.shape[1]], g_in[:, e_xyz.shape[1]:]
        elif i == 1:
            g_e = g_e + g_in
        else:
            g_h = g_in
    return r, {"d_e_xyz": g_e, "d_e_dir": g_xdir[:, Wd:]}


def emulate_backward(case, mutation, G, neg):
    """emulate() on a Case64's fp32 inputs -> the same dict Case64.backward returns the values of"""
    x = case.x32.clone().requires_grad_()
    dirs = case.dirs32.clone().requires_grad_()
    e_x, e_d = (x if case.ext else O.freq_encode(x, 10)), O.freq_encode(dirs, 4)
    with torch.no_grad():
        _, g = emulate(case.p32, (e_x.detach(), e_d.detach()), case.mode, mutation, G, neg)
    out = {"d_viewdirs": torch.autograd.grad(e_d, dirs, g["d_e_dir"])[0]}
    if case.ext:
        out["d_enc"] = g["d_e_xyz"]
    else:
        out["d_pts"] = torch.autograd.grad(e_x, x, g["d_e_xyz"])[0]
    return out


# ---- the census ---------------------------------------------------------------------------------------------------------------------
# What launches a row follows from the row itself: "fh" (nefes_field_{fwd,bwd}_h3_fh) for the FH flag, "hashgrid" (the grid gathered in
# the kernel) for HASHGRID_FUSED, "enc" (a supplied encoding) for EXTERNAL32, else "rays" (ops._field_fwd / _field_bwd on rays and pts=).
# A combination that kind_of does not know -- a new encoding, a new flag -- raises, and the counts of
# tests/test_field_ref.py::test_census_covers_every_inference_row pin the table's size.
def kind_of(row):
    args = [x.strip() for x in row.split(" ", 2)[2].strip("<>").split(",")]
    enc = args[1] if row.startswith("fwd") else args[2]
    if args[-1] == "1":
        assert enc == "FREQ10", row
        return "fh"
    return {"FREQ10": "rays", "EXTERNAL32": "enc", "HASHGRID_FUSED": "hashgrid"}[enc]


Case = collections.namedtuple("Case", "row network mode kind shapes")
Network = collections.namedtuple("Network", "width head_class ext has_transient fold fh nets")


def inference_rows():
    """the TRAIN = 0 rows of both tables, as nefes_field_h3_instance spells them"""
    return [r for r in table_rows() if re.search(r"<(.*)>", r).group(1).split(",")[-2] == "0"]


def parse_row(row):
    """row string -> (backward, Network, mode)"""
    d, _, args = row.split(" ", 2)
    a = [x.strip() for x in args.strip("<>").split(",")]
    if d == "fwd":
        mode, enc, w, ntr, fh = a[0], a[1], int(a[2]), int(a[3]), int(a[5])
        fold, has_t, cls = mode == "FULL_FOLD", mode in ("FULL", "FULL_FOLD"), {1: 0, 5: 1}[ntr]
        mode = "FULL" if fold else mode
    else:
        w, kr, enc, has_t, fh = int(a[0]), a[1], a[2], bool(int(a[3])), int(a[5])
        fold, cls = "NEFES_H3B_FOLD" in kr, {2: 0, 9: 1}[int(kr.split("|")[0])]
        mode = "FULL" if has_t else "STATIC"
    nets = NETS_OF_CLASS["fh" if fh else cls]
    return d == "bwd", Network(w, cls, enc != "FREQ10", bool(has_t), fold, bool(fh), nets), mode


def cases():
    """[Case(row, network, mode, kind, shapes)] -- one per TRAIN = 0 row of the table."""
    out = []
    for row in inference_rows():
        _, net, mode = parse_row(row)
        kind = kind_of(row)
        # the fused gather takes points away from the cell faces, one per ray: tests/hashgrid_ref.py's `inside` set
        out.append(Case(row, net, mode, kind, ((130, 1),) if kind == "hashgrid" else SHAPES))
    return out


def selects(case, C):
    """(NefesNetDesc arguments, backward, mode name, request flag names) with which nefes_field_h3_instance must answer case.row"""
    backward = case.row.startswith("bwd")
    flags = {"hashgrid": ("HASHGRID",), "fh": ("FH",)}.get(case.kind, ())
    if backward and case.mode == "STATIC":
        flags += ("STATIC_BWD",)
    n = case.network
    return (n.width, 0 if n.fh else C, int(n.has_transient), int(n.ext), int(n.fold)), backward, case.mode, flags


def pooled(kind, ext=False, shapes=SHAPES, seed=0):
    """every shape of one input set as ONE flat batch (the CPU checks): (pts [M, 3] | enc [M, 32], per-sample viewdirs [M, 3])"""
    xs, vs = [], []
    for N, S in shapes:
        if ext:
            x, v = encodings(kind, N, S, seed)
        else:
            o, d, z, v = rays(kind, N, S, seed)
            x = exact(o, d, z).reshape(-1, 3)
        xs.append(x)
        vs.append(per_sample(v, S))
    return torch.cat(xs), torch.cat(vs)
