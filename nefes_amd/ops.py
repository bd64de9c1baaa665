"""torch-facing wrappers of the C ABI (include/nefes_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation on the hot
path is a HIP kernel in libnefes_hip.so.  All tensors are fp32 CUDA(=HIP) tensors; wrappers
check dtype/contiguity/device and raise rather than silently converting on a different path.
"""
import collections
import ctypes as C
from typing import Optional

import os

import torch

from . import lib as L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-kernel timing (bench.py): when TIMERS is a dict, every C-ABI launch is bracketed by HIP events
# recorded on the launch stream (torch's current stream is the stream the kernels are launched on).
TIMERS = None


class _timed:
    """`with _timed(key)`: the launches inside go under TIMERS[key]; a key of None records nothing."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if TIMERS is not None and self.name is not None:
            self.t0 = torch.cuda.Event(enable_timing=True)
            self.t1 = torch.cuda.Event(enable_timing=True)
            self.t0.record()

    def __exit__(self, *exc):
        if TIMERS is not None and self.name is not None:
            self.t1.record()
            TIMERS.setdefault(self.name, []).append((self.t0, self.t1))
        return False


# Test tap: when TAP is a dict, the forward passes that save ReLU masks append (masks, N, S, width) under "masks" and the
# hierarchical sampler appends its merged depths under "z_fine" -- so that a test can evaluate the float64 oracle on exactly
# the samples and the ReLU branch pattern the kernels used (tests/branch.py).  Never set on the product path.
TAP = None


def _tap(key, value):
    if TAP is not None:
        TAP.setdefault(key, []).append(value)


def _chk(t: Optional[torch.Tensor], name: str, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"nefes_amd: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"nefes_amd: `{name}` must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"nefes_amd: `{name}` must be contiguous")
    return C.c_void_p(t.data_ptr())


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()             # (the usual case asks twice and converts nothing: .to and .contiguous each cost a dispatch)
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------
def _raygen_call(camera, pixels):
    """Which of the three entry-point pairs serves (camera, pixels): (their stem, the number of rays, the arguments before c2w, the
    arguments after it).  `camera`: a Python float (the focal length of a centred camera, a launch argument) or the float32 [4] device
    tensor (fx, fy, cx, cy) the kernels read when they run (as_intrinsics).  `pixels`: (H, W, row0, nrows), rows of the frame's grid, or
    the float32 [K, 2] device tensor of (x, y) (as_pixels)."""
    if torch.is_tensor(pixels):
        if not torch.is_tensor(camera):
            raise ValueError("nefes_amd: the rays of a pixel list take their camera from device memory, not a focal length: pass "
                             "intr=ops.as_intrinsics((focal, focal, W / 2, H / 2), device)")
        n = pixels.shape[0]
        return "nefes_raygen_px", n, (n, _px(pixels), _intr(camera)), ()
    H, W, row0, nrows = pixels
    if torch.is_tensor(camera):
        return "nefes_raygen_k", nrows * W, (H, W, _intr(camera)), (row0, nrows)
    return "nefes_raygen", nrows * W, (H, W, float(camera)), (row0, nrows)


def _raygen_fwd(c2w, camera, pixels):
    """-> (rays_o, rays_d, viewdirs), each [n, 3]."""
    name, n, head, tail = _raygen_call(camera, pixels)
    c2w = _f32(c2w[:3, :4])
    o = torch.empty(n, 3, device=c2w.device)
    d = torch.empty_like(o)
    v = torch.empty_like(o)
    L.check(getattr(L.load(), name + "_fwd")(*head, _chk(c2w, "c2w"), *tail, _chk(o, "o"), _chk(d, "d"), _chk(v, "v"), _stream()),
            name + "_fwd")
    return o, d, v


def _raygen_bwd(c2w, camera, pixels, g_o, g_d, g_v, want_intr=True):
    """-> (g_c2w [3,4], g_intr [4] or None): None for a focal length, and for a device camera when it is not wanted (the kernel then
    gets g_intr = NULL)."""
    name, n, head, tail = _raygen_call(camera, pixels)
    lib = L.load()
    c2w = _f32(c2w[:3, :4])
    ws = torch.empty(getattr(lib, name + "_bwd_workspace")(n), dtype=torch.uint8, device=c2w.device)
    g = torch.empty(3, 4, device=c2w.device)
    device_camera = torch.is_tensor(camera)
    gk = torch.empty(4, device=c2w.device) if want_intr and device_camera else None
    g_o, g_d, g_v = (None if t is None else _f32(t) for t in (g_o, g_d, g_v))
    L.check(getattr(lib, name + "_bwd")(*head, _chk(c2w, "c2w"), *tail, _chk(g_o, "g_o"), _chk(g_d, "g_d"), _chk(g_v, "g_v"),
                                        _chk(ws, "ws", torch.uint8), _chk(g, "g_c2w"), *((_chk(gk, "g_intr"),) if device_camera else ()),
                                        _stream()), name + "_bwd")
    return g, gk


def raygen_fwd(H, W, focal, c2w, row0=0, nrows=None):
    return _raygen_fwd(c2w, float(focal), (H, W, row0, H - row0 if nrows is None else nrows))


def raygen_bwd(H, W, focal, c2w, row0, nrows, g_o, g_d, g_v):
    return _raygen_bwd(c2w, float(focal), (H, W, row0, nrows), g_o, g_d, g_v)[0]


class RayGen(torch.autograd.Function):
    """get_rays + viewdirs (ray_utils.py:5-16, rendering.py:217) for every camera and pixel set (`rays` below), with the backward to the
    pose and -- when `intr` asks for it -- to (fx, fy, cx, cy).  The pixels are positions, not parameters: no gradient reaches them."""

    @staticmethod
    def forward(ctx, c2w, intr, px, focal, grid):
        ctx.save_for_backward(c2w, intr, px)
        ctx.focal, ctx.grid = focal, grid
        return _raygen_fwd(c2w, focal if intr is None else intr, grid if px is None else px)

    @staticmethod
    def backward(ctx, g_o, g_d, g_v):
        c2w, intr, px = ctx.saved_tensors
        g, gk = _raygen_bwd(c2w, ctx.focal if intr is None else intr, ctx.grid if px is None else px, g_o, g_d, g_v,
                            want_intr=ctx.needs_input_grad[1])
        if not (tuple(c2w.shape) == (3, 4) and c2w.dtype == torch.float32):     # (the refinement loop's 3x4 float32 pose: no zero
            out = torch.zeros_like(c2w)                                         #  fill + copy for a row that is not there)
            out[:3, :4] = g
            g = out
        return g, gk, None, None, None


def rays(c2w, H, W, focal=None, intr=None, px=None, row0=0, nrows=None):
    """(rays_o, rays_d, viewdirs), each [n, 3], of the pose c2w ([3,4] or [4,4]), differentiable w.r.t. it.  The camera is `intr`, the
    float32 [4] device tensor (fx, fy, cx, cy) of as_intrinsics -- read from device memory by the kernels, and handed a gradient when it
    requires one -- or, without it, the centred camera of the focal length `focal`.  The rays are those of the pixel list `px` (as_pixels;
    needs `intr`) or, without it, of rows [row0, row0 + nrows) of the H x W frame, row-major."""
    if intr is None and focal is None:
        raise ValueError("nefes_amd: rays() needs a camera: focal= or intr=")
    return RayGen.apply(c2w, intr, px, None if intr is not None else float(focal), (H, W, row0, H - row0 if nrows is None else nrows))


def as_intrinsics(x, device):
    """A pinhole camera (fx, fy, cx, cy) as the float32 [4] tensor on `device` that the raygen_k kernels READ FROM DEVICE MEMORY when they
    run (so that a captured graph follows in-place updates of it and a gradient can reach it).  Three forms:
      - a float32 [4] tensor already on `device`: used as is -- no copy, no sync, no check of its values (they are on the device);
      - a 4-sequence of numbers (fx, fy, cx, cy);
      - a 3 x 3 matrix K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]].
    Host-side values are validated: finite, fx and fy positive, no skew, last row 0 0 1 (ValueError names the offending value)."""
    dev = torch.device(device)
    if torch.is_tensor(x):
        here = x.device.type == dev.type and (dev.index is None or x.device.index == dev.index)
        if here and x.dtype == torch.float32 and tuple(x.shape) == (4,) and x.is_contiguous():
            return x
        if x.device.type != "cpu":          # (reading it back to validate or convert it would be a host sync)
            raise ValueError(f"nefes_amd: intrinsics on a device must be a contiguous float32 [4] tensor (fx, fy, cx, cy) on {dev}; got "
                             f"{x.dtype} {tuple(x.shape)} on {x.device}")
    import numpy as np
    a = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)
    if a.shape == (3, 3):
        for (i, j), want in (((0, 1), 0.), ((1, 0), 0.), ((2, 0), 0.), ((2, 1), 0.), ((2, 2), 1.)):
            if not a[i, j] == want:
                what = "skew is not supported" if (i, j) == (0, 1) else f"expected {want:g}"
                raise ValueError(f"nefes_amd: intrinsics K[{i}][{j}] = {float(a[i, j])!r}: {what} (K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]])")
        a = np.array([a[0, 0], a[1, 1], a[0, 2], a[1, 2]])
    if a.shape != (4,):
        raise ValueError(f"nefes_amd: intrinsics must be (fx, fy, cx, cy) or a 3 x 3 K; got shape {a.shape}")
    for name, v in zip(("fx", "fy", "cx", "cy"), a):
        if not np.isfinite(v):
            raise ValueError(f"nefes_amd: intrinsics {name} = {float(v)!r} is not finite")
    for name, v in zip(("fx", "fy"), a[:2]):
        if not v > 0:
            raise ValueError(f"nefes_amd: intrinsics {name} = {float(v)!r} must be positive")
    return torch.tensor(a, dtype=torch.float32, device=dev)


def _intr(intr):
    if tuple(intr.shape) != (4,):
        raise RuntimeError(f"nefes_amd: `intr` must be [4] (fx, fy, cx, cy); got {tuple(intr.shape)}")
    return _chk(intr.detach(), "intr")


def raygen_k_fwd(H, W, intr, c2w, row0=0, nrows=None):
    """raygen_fwd for the camera intr = (fx, fy, cx, cy), a float32 [4] DEVICE tensor the kernel reads when it runs."""
    return _raygen_fwd(c2w, intr, (H, W, row0, H - row0 if nrows is None else nrows))


def raygen_k_bwd(H, W, intr, c2w, row0, nrows, g_o, g_d, g_v, want_intr=True):
    """-> (g_c2w [3,4], g_intr [4] or None)."""
    return _raygen_bwd(c2w, intr, (H, W, row0, nrows), g_o, g_d, g_v, want_intr)


def as_pixels(x, device):
    """A pixel set as the float32 [K, 2] tensor of (x, y) = (column, row) on `device` that the raygen_px / sample_px kernels READ FROM DEVICE
    MEMORY when they run (a captured graph follows in-place updates of it).  get_rays' own convention: an integer coordinate is that
    pixel, there is no half-pixel offset; fractional coordinates and points outside the frame are legal.  Forms:
      - a contiguous float32 [K, 2] tensor already on `device`: used as is -- no copy, no sync, no check of its values;
      - an integer tensor [K, 2] (any device): converted on its device, no host read;
      - a host sequence, numpy array or host tensor [K, 2]: converted; the values must be finite.
    Anything else on a device raises (reading it back to convert it would be a host sync)."""
    dev = torch.device(device)
    if torch.is_tensor(x):
        ok_shape = x.dim() == 2 and x.shape[1] == 2 and x.shape[0] > 0
        here = x.device.type == dev.type and (dev.index is None or x.device.index == dev.index)
        if here and x.dtype == torch.float32 and ok_shape and x.is_contiguous():
            return x
        integer = not (x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool)
        if ok_shape and integer:
            return x.detach().to(dev, torch.float32).contiguous()
        if x.device.type != "cpu":
            raise ValueError(f"nefes_amd: pixels on a device must be a contiguous float32 (or an integer) [K, 2] tensor of (x, y) on {dev}; got "
                             f"{x.dtype} {tuple(x.shape)} on {x.device}")
    import numpy as np
    a = np.asarray(x.detach().numpy() if torch.is_tensor(x) else x, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0:
        raise ValueError(f"nefes_amd: pixels must be [K, 2] rows of (x, y) = (column, row); got shape {a.shape}")
    if not np.isfinite(a).all():
        k = int(np.argwhere(~np.isfinite(a))[0][0])
        raise ValueError(f"nefes_amd: pixel {k} = ({float(a[k, 0])!r}, {float(a[k, 1])!r}) is not finite")
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _px(px):
    if px.dim() != 2 or px.shape[1] != 2 or px.shape[0] == 0:
        raise RuntimeError(f"nefes_amd: `px` must be [K, 2] rows of (x, y); got {tuple(px.shape)}")
    return _chk(px.detach(), "px")


def raygen_px_fwd(px, intr, c2w):
    """raygen_k_fwd at the pixel list px (as_pixels) instead of the frame's grid: (rays_o, rays_d, viewdirs), each [K, 3].  px and intr are
    float32 DEVICE tensors the kernel reads when it runs."""
    return _raygen_fwd(c2w, intr, px)


def raygen_px_bwd(px, intr, c2w, g_o, g_d, g_v, want_intr=True):
    """-> (g_c2w [3,4], g_intr [4] or None): raygen_k_bwd's 12 + 4 sums over the rays of px."""
    return _raygen_bwd(c2w, intr, px, g_o, g_d, g_v, want_intr)


def sample_pixels(map, px, out=None, nearest=False):
    """Bilinear sample of a [C, H, W] float32 map at the pixel list px (as_pixels): [C, K], channel-major as the feature-loss kernels read
    it.  Coordinates are clamped to the frame; at an integer coordinate the value is the map's own, exactly.  No gradient (it samples
    targets).  `out`: a contiguous float32 [C, K] tensor on the map's device that the kernel writes (None: a fresh one).
    `nearest`: the one tap at (clamp(floor(x + 0.5), 0, W-1), clamp(floor(y + 0.5), 0, H-1)) instead (nefes_sample_px_nearest): for maps
    that must not be blended, such as a depth frame with holes in it."""
    if map.dim() != 3:
        raise RuntimeError(f"nefes_amd: sample_pixels: `map` must be [C, H, W]; got {tuple(map.shape)}")
    Cc, H, W = (int(v) for v in map.shape)
    n = px.shape[0]
    if out is None:
        out = torch.empty(Cc, n, device=map.device)
    elif tuple(out.shape) != (Cc, n):
        raise RuntimeError(f"nefes_amd: sample_pixels: `out` must be [{Cc}, {n}]; got {tuple(out.shape)}")
    name = "nefes_sample_px_nearest" if nearest else "nefes_sample_px"
    L.check(getattr(L.load(), name)(Cc, H, W, _chk(map.detach(), "map"), n, _px(px), _chk(out, "out"), _stream()), name)
    return out


def draw_state(seed, device):
    """The {seed, tick} words of a draw sequence (draw_pixels): the int64 [2] tensor {seed, 0} on `device`.  0 <= seed < 2^63."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 63:
        raise ValueError(f"nefes_amd: draw_state: seed = {seed} must be in [0, 2^63)")
    return torch.tensor([seed, 0], dtype=torch.int64, device=torch.device(device))


def _draw_workspace(state, B, H, W):
    """draw_pixels' workspace, allocated once per (B, H, W, device) -- and per draw sequence: it is kept ON the state tensor, not in a
    table of the module, because two sequences may run on two streams at once (refine_concurrently: one refiner, one state each), and
    a captured graph holds its address for as long as it holds the state's."""
    cache = getattr(state, "_nefes_draw_workspace", None)
    if cache is None:
        cache = state._nefes_draw_workspace = {}
    key = (int(B), int(H), int(W), str(state.device))
    ws = cache.get(key)
    if ws is None:
        nbytes = int(L.load().nefes_draw_pixels_workspace(B, H, W))
        if nbytes <= 0:
            raise ValueError(f"nefes_amd: draw_pixels: B, H, W = {B}, {H}, {W} must be positive with H * W <= 2^24")
        ws = cache[key] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=state.device)
    return ws


def draw_pixels(H, W, K, state, B=1, mask=None, period=1, advance=True, out=None, n_valid=None):
    """K distinct pixels of the H x W frame for each of B images, drawn ON THE DEVICE, uniform among the valid pixels of `mask`:
    float32 [B, K, 2] rows (x, y), ascending in y*W + x, contiguous -- px[b] is a legal `pixels=` list (render, sample_pixels) without a
    copy.  Nothing here reads the device, so the call can sit in a captured graph.
    state: draw_state's int64 [2] {seed, tick}, read by the kernels when they run: the draw is a function of (seed, tick // period, b,
    mask[b]) alone (include/nefes_hip.h gives the keys; tests/draw_ref.py restates them).  advance: the tick is incremented behind the
    draw, so the next call -- or the next replay of a graph that holds this one -- draws a new batch every `period` calls.
    mask: a uint8 or bool [B, H, W] (or [H, W] for B = 1) device tensor, read in place, valid where != 0; None: every pixel.  An image
    with fewer than K valid pixels gets them all, repeated cyclically; with none, rows of (0, 0): n_valid tells.
    out: a contiguous float32 [B, K, 2] (or, B = 1, [K, 2]) tensor written in place;  n_valid: an int32 [B] tensor that receives the
    number of valid pixels per image.  No gradient: pixel indices carry none."""
    B, H, W, K, period = int(B), int(H), int(W), int(K), int(period)
    if tuple(state.shape) != (2,):
        raise RuntimeError(f"nefes_amd: draw_pixels: `state` must be the int64 [2] tensor of draw_state; got {tuple(state.shape)}")
    dev = state.device
    if min(B, H, W, K, period) <= 0 or K > H * W or H * W > 1 << 24:
        raise ValueError(f"nefes_amd: draw_pixels: B, H, W, K, period = {B}, {H}, {W}, {K}, {period} must be positive with K <= H * W "
                         f"<= 2^24")
    if mask is not None:
        if mask.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError(f"nefes_amd: draw_pixels: `mask` must be uint8 or bool (got {mask.dtype})")
        if tuple(mask.shape) != (B, H, W) and not (B == 1 and tuple(mask.shape) == (H, W)):
            raise RuntimeError(f"nefes_amd: draw_pixels: `mask` must be [{B}, {H}, {W}]; got {tuple(mask.shape)}")
        if mask.device != dev:
            raise RuntimeError(f"nefes_amd: draw_pixels: `mask` is on {mask.device}, the state on {dev}")
    if out is None:
        out = torch.empty(B, K, 2, device=dev)
        res = out
    else:
        if tuple(out.shape) != (B, K, 2) and not (B == 1 and tuple(out.shape) == (K, 2)):
            raise RuntimeError(f"nefes_amd: draw_pixels: `out` must be [{B}, {K}, 2]; got {tuple(out.shape)}")
        if out.device != dev:
            raise RuntimeError(f"nefes_amd: draw_pixels: `out` is on {out.device}, the state on {dev}")
        res = out.view(B, K, 2) if out.is_contiguous() else out
    if n_valid is not None and (tuple(n_valid.shape) != (B,) or n_valid.device != dev):
        raise RuntimeError(f"nefes_amd: draw_pixels: `n_valid` must be int32 [{B}] on {dev}; got {tuple(n_valid.shape)} on {n_valid.device}")
    ws = _draw_workspace(state, B, H, W)
    L.check(L.load().nefes_draw_pixels(B, H, W, _chk(mask, "mask", torch.bool if mask is not None and mask.dtype == torch.bool else torch.uint8),
                                       K, period, _chk(state, "state", torch.int64), int(bool(advance)), _chk(out, "out"),
                                       _chk(n_valid, "n_valid", torch.int32), _chk(ws, "workspace", torch.int64), _stream()),
            "nefes_draw_pixels")
    return res


class NdcRays(torch.autograd.Function):
    """ndc_rays (ray_utils.py:27-44)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, H, W, focal, near):
        o, d = _f32(rays_o).reshape(-1, 3), _f32(rays_d).reshape(-1, 3)
        oo, od = torch.empty_like(o), torch.empty_like(d)
        L.check(L.load().nefes_ndc_fwd(H, W, float(focal), float(near), o.shape[0], _chk(o, "o"), _chk(d, "d"),
                                       _chk(oo, "oo"), _chk(od, "od"), _stream()), "nefes_ndc_fwd")
        ctx.save_for_backward(o, d)
        ctx.geom = (H, W, focal, near, rays_o.shape)
        return oo.reshape(rays_o.shape), od.reshape(rays_d.shape)

    @staticmethod
    def backward(ctx, g_oo, g_od):
        o, d = ctx.saved_tensors
        H, W, focal, near, shape = ctx.geom
        go, gd = torch.empty_like(o), torch.empty_like(d)
        g_oo = None if g_oo is None else _f32(g_oo).reshape(-1, 3)
        g_od = None if g_od is None else _f32(g_od).reshape(-1, 3)
        L.check(L.load().nefes_ndc_bwd(H, W, float(focal), float(near), o.shape[0], _chk(o, "o"), _chk(d, "d"),
                                       _chk(g_oo, "g_oo"), _chk(g_od, "g_od"), _chk(go, "go"), _chk(gd, "gd"), _stream()),
                "nefes_ndc_bwd")
        return go.reshape(shape), gd.reshape(shape), None, None, None, None


_LINSPACE = {}


def _linspace01(n, device):
    """torch.linspace(0, 1, n) on the device, built once per (n, device): rendering.py:33,95 create it on every call."""
    key = (int(n), str(device))
    t = _LINSPACE.get(key)
    if t is None:
        t = _LINSPACE[key] = torch.linspace(0., 1., steps=int(n), device=device)
    return t


def coarse_depths(N, Nc, near, far, lindisp=False, t_rand=None, device="cuda", bounds=None):
    """rendering.py:95-112.  `bounds` = a float32 CUDA tensor whose rows start with (near, far) per ray (any row stride,
    e.g. columns 6:8 of the reference's packed ray batch); then the scalars are ignored."""
    t = _linspace01(Nc, device)                                    # rendering.py:95 (torch's own two-sided formula)
    z = torch.empty(N, Nc, device=device)
    t_rand = None if t_rand is None else _f32(t_rand)
    if bounds is not None:
        if not (bounds.is_cuda and bounds.dtype == torch.float32 and bounds.dim() == 2 and bounds.shape[0] == N
                and bounds.shape[1] >= 2 and bounds.stride(1) == 1):
            raise RuntimeError("nefes_amd: `bounds` must be a float32 CUDA tensor [N, >=2] with unit column stride")
        L.check(L.load().nefes_coarse_depths_rays(N, Nc, C.c_void_p(bounds.data_ptr()), int(bounds.stride(0)),
                                                  int(bool(lindisp)), _chk(t, "t"), _chk(t_rand, "t_rand"), _chk(z, "z"),
                                                  _stream()), "nefes_coarse_depths_rays")
        return z
    L.check(L.load().nefes_coarse_depths(N, Nc, float(near), float(far), int(bool(lindisp)), _chk(t, "t"),
                                         _chk(t_rand, "t_rand"), _chk(z, "z"), _stream()), "nefes_coarse_depths")
    return z


_ZROW = {}
_ZROW_MAX = 64


def coarse_depth_row(Nc, near, far, lindisp=False, device="cuda"):
    """The ONE row of coarse depths every ray shares when near / far are scalars and nothing is jittered (rendering.py:96-100:
    z_vals = near (1 - t) + far t, expanded to [N_rays, N_samples]): [Nc], computed once per (Nc, near, far, lindisp, device) by the
    same kernel as coarse_depths, so the expanded tensor never exists (field_sigma_row, coarse_sample)."""
    key = (int(Nc), float(near), float(far), bool(lindisp), str(device))
    z = _ZROW.get(key)
    if z is not None:
        _ZROW[key] = _ZROW.pop(key)                # most recently used last
        return z
    z = coarse_depths(1, Nc, near, far, lindisp, None, device=device).reshape(-1)
    # A row first computed while a HIP graph is being captured lives in the graph's private pool and is filled on replay only:
    # it must not be handed to later eager renders, so it is not cached.  Per-image near / far values would grow the
    # cache without limit: the least recently used rows go.
    if not torch.cuda.is_current_stream_capturing():
        _ZROW[key] = z
        while len(_ZROW) > _ZROW_MAX:
            _ZROW.pop(next(iter(_ZROW)))
    return z


def fused_coarse_pass_ok(pk, Nc, Ni, N=0, grid=None):
    """The coarse pass as two launches (sigma-only field kernel on a shared depth row + coarse_sample) instead of four: fp16 two-part
    instances, frequency embedding (or a hash grid the field kernel gathers itself: hashgrid_fused_ok), Nc = 64 / 128 / 256,
    Nc + Ni <= 512 (csrc/sample_pdf.hip coarse_sample_kernel)."""
    enc_ok = pk.xyz_encoding == L.XYZ_FREQ10 if grid is None else hashgrid_fused_ok(pk, grid)
    return (FUSED_COARSE and h3_serves(pk) and enc_ok and Nc in (64, 128, 256)
            and Ni > 0 and Nc + Ni <= 512 and N * Nc < H3_MAX_SAMPLES)      # (beyond the 32-bit sample index: the four-launch path)


def field_sigma_row(pk, rays_o, rays_d, z_row, grid=None):
    """sigma [N,1,Nc] of the coarse network along rays whose depths are ONE shared row (no gradient: nerfh_nff.py:192-202).
    grid: an ops.HashGrid whose encoding the kernel evaluates itself (hashgrid_fused_ok)."""
    rays_o, rays_d = _f32(rays_o), _f32(rays_d)
    return _field_fwd(pk, L.FIELD_SIGMA, rays_o.shape[0], z_row.numel(), rays_o=rays_o, rays_d=rays_d, z=z_row, grid=grid)[0]


def coarse_sample(sigma, z, Ni, u=None, want_samples=True, want_weights=False):
    """Compositing variant D + sample_pdf + sort(cat) of the coarse pass in ONE launch (csrc/sample_pdf.hip coarse_sample_kernel;
    nerfh_nff.py:83-89, rendering.py:23-66,132-141).  sigma [N,1,Nc] or [N,Nc]; z [N,Nc], or [Nc] = one row shared by every ray.
    -> (z_fine [N,Nc+Ni], z_samples [N,Ni] or None[, weights [N,Nc]]); bit-identical to composite_fwd(COMP_SIGMA_ONLY) +
    sample_pdf_merge."""
    sigma, z = _f32(sigma), _f32(z)
    N, Nc = sigma.shape[0], sigma.shape[-1]
    dev = sigma.device
    if u is None:
        u = _linspace01(Ni, dev)
    u = _f32(u)
    z_fine = torch.empty(N, Nc + Ni, device=dev)
    z_samples = torch.empty(N, Ni, device=dev) if want_samples else None
    weights = torch.empty(N, Nc, device=dev) if want_weights else None
    with _timed("coarse_sample"):
        L.check(L.load().nefes_coarse_sample(N, Nc, Ni, _chk(sigma, "sigma"), _chk(z, "z"), 1 if z.dim() == 1 else 0, _chk(u, "u"),
                                             1 if u.dim() == 2 else 0, _chk(z_fine, "z_fine"), _chk(z_samples, "z_samples"),
                                             _chk(weights, "weights"), _stream()), "nefes_coarse_sample")
    _tap("z_fine", z_fine)
    _tap("z_samples", z_samples)
    return (z_fine, z_samples, weights) if want_weights else (z_fine, z_samples)


# ---------------------------------------------------------------------------------------------
# field MLP
# ---------------------------------------------------------------------------------------------
class PackedField:
    """Device-resident fragment streams of one NeRFH_NFF network (nefes_pack_weights)."""

    LAYERS_COARSE = [f"xyz_encoding_{i}.0" for i in range(1, 9)] + ["xyz_encoding_final", "dir_encoding.0",
                                                                    "static_sigma.0", "static_rgb.0"]
    LAYERS_FINE = LAYERS_COARSE + ["transient_encoding.0", "transient_encoding.2", "transient_encoding.4",
                                   "transient_sigma.0", "transient_rgb.0", "transient_beta.0"]

    def __init__(self, state_dict, width, feat_dim, has_transient, device, xyz_encoding=0, fold_final=False):
        lib = L.load()
        self.desc = L.NefesNetDesc(int(width), int(feat_dim), 1 if has_transient else 0, int(xyz_encoding), 1 if fold_final else 0)
        self.fold = bool(fold_final)  # xyz_encoding_final multiplied into the head matrices of the fp16 streams (frozen networks; fold_shape)
        self.xyz_encoding = int(xyz_encoding)
        self.width, self.feat_dim, self.has_transient = int(width), int(feat_dim), bool(has_transient)
        info = L.NefesBlobInfo()
        L.check(lib.nefes_blob_info(self.desc, info), "nefes_blob_info")
        names = self.LAYERS_FINE if has_transient else self.LAYERS_COARSE
        host = []
        for n in names:
            host.append(state_dict[n + ".weight"].detach().to("cpu", torch.float32).contiguous())
            host.append(state_dict[n + ".bias"].detach().to("cpu", torch.float32).contiguous())
        ptrs = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
        blob = torch.zeros(info.total_bytes, dtype=torch.uint8)
        L.check(lib.nefes_pack_weights(self.desc, ptrs, len(host), C.c_void_p(blob.data_ptr()), blob.numel()),
                "nefes_pack_weights")
        self.blob = blob.to(device)
        self.info = info
        self.generation = 0          # bumped by repack(); autograd nodes refuse to run backward across it
        self.h3_valid = True         # False once a re-pack WITHOUT the fp16 plan left the fp16 two-part streams stale (REPACK_H3 = False)
        self._map = None

    def repack(self, params):
        """Re-pack every stream on the device from the current parameter values (`params`: (weight, bias) per layer in
        LAYERS order, CUDA tensors): one concatenation + one launch (nefes_pack_device), no host copy, no sync."""
        lib = L.load()
        if self.fold:
            raise RuntimeError("nefes_amd: a folded pack (fold_final) holds products of parameters and is not re-packed on the device; "
                               "trainable networks take NeRFH_NFF.packed()")
        if self._map is None:
            n = self.info.total_bytes // 2
            host_map = torch.zeros(n, dtype=torch.int32)
            elems = (C.c_int64 * 36)()
            L.check(lib.nefes_pack_map(self.desc, C.c_void_p(host_map.data_ptr()), n, C.cast(elems, C.c_void_p)), "nefes_pack_map")
            self._map = host_map.to(self.blob.device)
            self._elems = list(elems)[:36 if self.has_transient else 24]
            # reductions the fp16 two-part streams need (one exponent per weight matrix, row bounds, bias maxima)
            need = C.c_size_t(0)
            L.check(lib.nefes_pack_h3_plan(self.desc, None, 0, C.byref(need)), "nefes_pack_h3_plan")
            plan = torch.zeros(int(need.value), dtype=torch.int32)
            L.check(lib.nefes_pack_h3_plan(self.desc, C.c_void_p(plan.data_ptr()), plan.numel(), None), "nefes_pack_h3_plan")
            self._plan_jobs = int(plan[0])
            self._plan = plan.to(self.blob.device)
            self._plan_scratch = torch.zeros(32, dtype=torch.int32, device=self.blob.device)
        if [int(p.numel()) for p in params] != self._elems:
            raise RuntimeError("nefes_amd: parameter shapes do not match the packed network description")
        flat = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32)
        h3 = REPACK_H3 and self._plan_jobs > 0
        L.check(lib.nefes_pack_device(flat.data_ptr(), flat.numel(), self._map.data_ptr(), self._map.numel(),
                                      self._plan.data_ptr() if h3 else None, self._plan_jobs if h3 else 0,
                                      self._plan_scratch.data_ptr() if h3 else None, self.blob.data_ptr(), _stream()),
                "nefes_pack_device")
        self.generation += 1
        if not h3:
            self.h3_valid = False    # the kernels fall back to the bf16x6 instances for this network from here on

    def h3_byte_ranges(self):
        """[(begin, end)] byte ranges of the fp16 two-part units and their scale tables (refreshed by repack() only with the
        fp16 plan, REPACK_H3)."""
        out = []
        for k in (L.STREAM_FWD_SIGMA_H3, L.STREAM_FWD_FULL_H3, L.STREAM_BWD_FULL_H3, L.STREAM_FWD_STATIC_H3, L.STREAM_BWD_STATIC_H3):
            si = self.info.stream[k]
            if si.n_slabs:
                slab = int(L.load().nefes_stream_slab_bytes(self.desc, k))        # per stream: forward and backward rings differ
                out.append((int(si.slab_off), int(si.slab_off + si.n_slabs * slab)))
                out.append((int(si.bias_off + 4 * si.scale_off), int(si.bias_off + 4 * si.bias_floats)))
        return out

    def check_generation(self, gen):
        if gen != self.generation:
            raise RuntimeError("nefes_amd: the network weights were modified (re-packed) between this forward pass and its "
                               "backward pass")

    def mask_bytes(self, M):
        return L.load().nefes_field_mask_bytes(self.desc, M)

    def train_rows(self):
        """(rows per tile, first row of block L.TB_*) of the train-mode acts / dacts buffers (nefes_train_row_offset)."""
        lib = L.load()
        return int(lib.nefes_train_rows(self.desc)), [int(lib.nefes_train_row_offset(self.desc, b)) for b in range(L.TB_END + 1)]

    def n_raw(self, mode):
        return 1 if mode == L.FIELD_SIGMA else (3 + self.feat_dim + (1 if mode == L.FIELD_STATIC else 6))


# Which matrix-core arithmetic the field kernels use where an instance exists (width 256 / C = 16, width 128 / C = 128):
#   "h3"  (default) fp16 two-part split products, three cross terms on v_mfma_f32_32x32x16_f16 (csrc/field_h3.h): fp32-level
#         accuracy at half the matrix-core work of bf16x6; tests/test_gpu_h3.py against the float64 oracle
#   "x6"  bf16x6 split products (csrc/field_x6.h): the round-1 default; also what trainable / re-packed networks use
#   "f32" the plain fp32-MFMA kernels (NEFES_X6=0 selects them too)
SPLIT = os.environ.get("NEFES_SPLIT", "h3")
# repack() also refreshes the fp16 two-part streams on the device (csrc/pack_device.hip h3_scales_kernel); "0": leave them stale and
# let re-packed networks run on the bf16x6 instances (the round-2 behaviour)
REPACK_H3 = os.environ.get("NEFES_REPACK_H3", "1") != "0"
USE_X6 = os.environ.get("NEFES_X6", "1") != "0"
# the coarse pass at test time as two launches instead of four (coarse_depth_row / field_sigma_row / coarse_sample); "0": the separate
# coarse_depths, sigma field, composite D and sample_pdf_merge launches (the tests compare the two bit for bit)
FUSED_COARSE = os.environ.get("NEFES_FUSED_COARSE", "1") != "0"
# Frozen networks on the fp16 pipe: xyz_encoding_final (a Linear with no activation behind it) is multiplied into dir_encoding /
# transient_encoding.0 by the packer and its W x W product leaves the fine pass's forward and backward kernels (csrc/field_fwd_h3.hip
# FOLD; NeRFH_NFF.packed_folded).  "0": the unfolded kernels for every network.
FOLD_FINAL = os.environ.get("NEFES_FOLD_FINAL", "1") != "0"
# The factored feature head (csrc/field_fwd_h3.hip FH, nefes_amd/render.py): a frozen width-128 fine network emits g = relu(dir_encoding)
# instead of its 128 feature channels and the head's matrix is applied once per ray to the composited g; "0": the plain kernels.
FACTORED_HEAD = os.environ.get("NEFES_FACTORED_HEAD", "1") != "0"
# "1": networks the tuned instances DO serve run on the generic kernels (csrc/field_generic.hip) too (off by default; so that the two
# can be compared on the same weights).  Networks the tuned instances do not serve always take the generic kernels.
FIELD_GENERIC = os.environ.get("NEFES_FIELD_GENERIC", "0") == "1"
# BASELINE configs[3] with the hash grid evaluated INSIDE the field kernels (csrc/hashgrid.h, nefes_field_fwd_h3_hashgrid /
# nefes_field_bwd_h3_hashgrid); "0": the separate launches HashGridEncode + FieldFromEncoding (the tests compare the two)
FUSED_HASHGRID = os.environ.get("NEFES_FUSED_HASHGRID", "1") != "0"

# FusionNet with TRAINABLE weights on a GPU (the reference's third training stage, run_nefes.py:78-108,150-160) on the library's kernels:
# the convolutions' weight / bias gradients (csrc/conv.hip conv2d_wgrad) and BatchNorm's affine gradients (csrc/refine.hip) instead of
# torch / MIOpen -- deterministic, fp32 MFMA, a fixed summation order.  Opt-in (NEFES_HIP_FUSION_TRAIN=1): off, such a net runs on torch
# as it always has.  Read at call time (field.FusionNet).
FUSION_TRAIN = os.environ.get("NEFES_HIP_FUSION_TRAIN", "0") == "1"


HEAD_MAX_C = 141          # csrc/layout.h NEFES_HEAD_MAX_C: the larger head class serves 3 + C <= 144
COMPILED_SET = L.COMPILED_SET
H3_MAX_SAMPLES = (1 << 31) - 256      # the fp16 two-part kernels index the samples of one launch with 32 bits
MODE_NAMES = ("sigma", "static", "full")


def head_class(C):
    """csrc/layout.h nefes_head_class: the rgb+feature head's compile-time shape class (0: 3+C <= 32, 1: 3+C <= 144, -1: none)."""
    return -1 if C < 0 else (0 if 3 + C <= 32 else (1 if 3 + C <= 144 else -1))


# -- the primitives every routing decision below is built from: canonical_shape, h3_shape, _h3 ---------------------------------
def canonical_shape(pk):
    """Shapes that ALSO have bf16x6 and fp32-MFMA instances: width 256 / C = 16 (either xyz encoding) and the reference-default
    width 128 / C = 128 (frequency embedding)."""
    return (pk.width == 256 and pk.feat_dim == 16) or (pk.width == 128 and pk.feat_dim == 128 and pk.xyz_encoding == L.XYZ_FREQ10)


def h3_shape(pk):
    """Shapes with fp16 two-part instances (csrc/field_fwd_h3.hip nefes_field_fwd_h3): both widths x both head classes with the
    frequency embedding; width 256 x both head classes with an external embedding."""
    cls = head_class(pk.feat_dim)
    if pk.width not in (128, 256) or cls < 0:
        return False
    return True if pk.xyz_encoding == L.XYZ_FREQ10 else pk.width == 256


def _h3(pk):
    """The fp16 two-part pipe is selected and this network's fp16 streams are current."""
    if SPLIT not in ("h3", "x6", "f32"):
        raise ValueError("nefes_amd.ops.SPLIT must be 'h3', 'x6' or 'f32'")
    return SPLIT == "h3" and pk.h3_valid


def h3_serves(pk):
    """fp16 two-part instances serve this pack: pipe selected, streams current, shape compiled."""
    return _h3(pk) and h3_shape(pk)


def static_h3(pk):
    """The static-head instances of the fp16 two-part kernels apply (the STATIC rows of csrc/field_h3_instances.h, nefes_field_bwd_static_h3;
    the train-mode instances too: train.fp16_pipe): every compiled (width, head class) pair with the frequency embedding."""
    return h3_serves(pk) and pk.xyz_encoding == L.XYZ_FREQ10


def _has_instance(pk):
    return canonical_shape(pk) or h3_serves(pk)


def x6_supported(pk, mode):
    """A split-product instance (fp16 two-part or bf16x6) serves this network and mode: sigma-only or full, forward and backward --
    and, on the fp16 two-part instances with the frequency embedding, the static head alone (round 5: a frozen coarse network with
    test_time False, a fine network with NeRFW off)."""
    if mode == L.FIELD_STATIC:
        return static_h3(pk)
    return _has_instance(pk) and (mode == L.FIELD_SIGMA or (mode == L.FIELD_FULL and pk.has_transient))


def require_instance(pk, what):
    """Fail loudly, naming the compiled set, before a launch that no kernel instance serves."""
    if _has_instance(pk):
        return
    raise RuntimeError(f"nefes_amd: no kernel instance serves {what} for W={pk.width}, f_dim={pk.feat_dim}, "
                       f"xyz_encoding={pk.xyz_encoding} with NEFES_SPLIT={SPLIT}"
                       f"{'' if pk.h3_valid else ' (fp16 streams stale: NEFES_REPACK_H3=0)'}.  Compiled: {COMPILED_SET}")


def fold_shape(width, feat_dim, xyz_encoding=L.XYZ_FREQ10):
    """Shapes with folded instances (the FULL_FOLD rows of csrc/field_h3_instances.h): width 256, both head classes, frequency embedding, full pass."""
    return width == 256 and head_class(feat_dim) >= 0 and xyz_encoding == L.XYZ_FREQ10


def fold_serves(width, feat_dim, xyz_encoding):
    """A frozen fine network of this shape renders on a folded pack (NeRFH_NFF.fold_ok adds the network's own conditions)."""
    return FOLD_FINAL and SPLIT == "h3" and USE_X6 and not FIELD_GENERIC and fold_shape(width, feat_dim, xyz_encoding)


def factored_head_serves(width, feat_dim):
    """A frozen fine network of this shape on the frequency embedding renders with the factored head (NeRFH_NFF.factored_head_ok):
    width 128 and a head with more channels than g = relu(dir_encoding) has features (+ the ones channel).  (NEFES_X6 is not asked.)"""
    return FACTORED_HEAD and SPLIT == "h3" and not FIELD_GENERIC and width == 128 and 3 + feat_dim > 3 + width // 2 + 1


def is_generic(pk):
    return bool(getattr(pk, "generic", False))


def hashgrid_fused_ok(pk, grid):
    """The fp16 two-part field kernels can gather this hash grid themselves: width 256, head class 0, sixteen levels x two features.
    (Head class 1 -- the 128-channel feature head -- has instances on a SUPPLIED encoding only -- csrc/field_h3_instances.h, the note
    at the backward's <256, 9, EXTERNAL32> row: its
    renders take HashGridEncode + FieldFromEncoding, and with them the four-launch coarse pass.)"""
    return (FUSED_HASHGRID and isinstance(grid, HashGrid) and h3_serves(pk) and pk.xyz_encoding == L.XYZ_EXTERNAL32
            and head_class(pk.feat_dim) == 0 and grid.desc.n_levels == 16 and grid.desc.n_features == 2)


Route = collections.namedtuple("Route", "entry key label g_enc")


def field_route(pk, mode, backward=False, kind="rays", M=0, override=None):
    """Which kernel serves one field pass -> Route(entry: the C entry point's name, key: the timer key, label: what L.check prints,
    g_enc: the backward hands back d loss / d encoding [M, 32] in the place of d loss / d pts).  Pure: no tensors, no library, no
    device work; SPLIT, USE_X6 and the packs' h3_valid are read at call time.

    pk: a pack's attributes (width, feat_dim, xyz_encoding, has_transient, h3_valid, fold, generic); mode: L.FIELD_*; kind: "rays",
    "points", "enc" (a supplied 32-feature encoding), "hashgrid" (gathered in the kernel) or "zrow" (rays that share one row of
    depths: field_sigma_row); M = N * S samples; override (forward only): None -- the switches decide, what the autograd Functions
    do; "split" -- a split-product instance whatever NEFES_X6 / NEFES_SPLIT=f32 say (field_fwd_x6); "f32" -- the strict fp32-MFMA
    entry point (field_fwd).  DESIGN.md 4.1.1 is this function as a table.  The decisions, each as it has been since its family
    of instances arrived:

    * hashgrid / zrow: fp16 two-part instances only, M below H3_MAX_SAMPLES; no static head.  Whether they serve the pack at all is
      the caller's question (hashgrid_fused_ok, fused_coarse_pass_ok) and is not asked again here.
    * a generic pack (NeRFH_NFF.packed_generic): nefes_field_fwd_generic / nefes_field_bwd_generic, every mode, any M -- on the
      frequency embedding, for rays or points.  Packed for a supplied encoding (xyz_encoding == XYZ_EXTERNAL32) it takes kind "enc"
      alone, on nefes_field_fwd_generic_ext / nefes_field_bwd_generic_ext (g_enc on the backward, FULL or STATIC).  Either pack with
      a kind of the other one is refused, naming the shape; so is a pack for a supplied encoding with kind hashgrid / zrow (the callers
      ask hashgrid_fused_ok / fused_coarse_pass_ok first, which say no: h3_valid is False).
    * forward, switches decide: the split route when USE_X6, SPLIT != "f32" and x6_supported(pk, mode) -- and, for POINTS input,
      only with the frequency embedding.  Otherwise the strict route.
    * forward, split route: fp16 two-part when h3_serves(pk) and M < H3_MAX_SAMPLES.  Otherwise the STATIC head falls to the strict
      route; sigma / full drop to bf16x6 on canonical shapes and are refused elsewhere (which is what happens to a non-canonical
      shape at M >= H3_MAX_SAMPLES).  A folded pack serves FULL on fp16 only.
    * forward, strict route: nefes_field_fwd, canonical shapes only.
    * backward, STATIC: fp16 when USE_X6, SPLIT != "f32", static_h3(pk) and M < H3_MAX_SAMPLES; else nefes_field_bwd_static,
      canonical shapes only.
    * backward, any other mode is the FULL head: a split instance when USE_X6, SPLIT != "f32" and x6_supported(pk, FULL) -- fp16 when
      _h3(pk), else bf16x6, which refuses a folded pack.  Otherwise nefes_field_bwd, WITHOUT a shape check (the C side refuses).  So
      a folded pack under SPLIT = "f32" lands on the strict entry point: that stream of a folded blob is the unfolded one and raw_t /
      masks are the same (tests/test_gpu_fold.py relies on it).
    * the FULL backward does not look at M at all: at M >= H3_MAX_SAMPLES it still names the fp16 instance.  Known, kept as it is
      (it cannot be reached at test sizes; changing it is a change of behaviour).
    """
    name = MODE_NAMES[mode]
    d = "bwd" if backward else "fwd"
    switched = USE_X6 and SPLIT != "f32"
    route = lambda entry, key, g_enc=False: Route(entry, key, entry, g_enc)
    gen_ext = is_generic(pk) and pk.xyz_encoding == L.XYZ_EXTERNAL32
    if is_generic(pk) and (kind == "enc") != gen_ext:
        raise RuntimeError(f"nefes_amd: the generic field kernels of W={pk.width}, D={pk.depth}, f_dim={pk.feat_dim} were packed for "
                           f"{'a supplied 32-feature encoding' if gen_ext else 'the frequency embedding'} (xyz_encoding={pk.xyz_encoding}) "
                           f"and cannot take input of kind '{kind}'")
    if kind in ("hashgrid", "zrow"):
        if M >= H3_MAX_SAMPLES:
            raise RuntimeError("nefes_amd: too many samples for one launch of the fp16 two-part kernels (32-bit sample index)")
        if kind == "zrow":
            return route("nefes_field_fwd_h3_zrow", "field_fwd[sigma,h3]")
        if backward:
            return route("nefes_field_bwd_h3_hashgrid", "field_bwd[h3,hashgrid]")
        if mode == L.FIELD_STATIC:
            raise NotImplementedError("nefes_amd: the hash-grid field kernels evaluate the sigma-only or the full head")
        return route("nefes_field_fwd_h3_hashgrid", f"field_fwd[{name},h3,hashgrid]")
    if is_generic(pk):
        if gen_ext:
            return route(f"nefes_field_{d}_generic_ext", f"field_{d}[{name},generic,ext]", backward)
        return route(f"nefes_field_{d}_generic", f"field_{d}[{name},generic]")
    fold = getattr(pk, "fold", False)
    if not backward:
        if override is None:
            split = switched and x6_supported(pk, mode) and (kind != "points" or pk.xyz_encoding == L.XYZ_FREQ10)
        else:
            split = override == "split"
        if split:
            h3 = h3_serves(pk) and M < H3_MAX_SAMPLES
            if h3 or mode != L.FIELD_STATIC:
                if not h3 and not canonical_shape(pk):
                    raise RuntimeError(f"nefes_amd: {M} samples in one launch exceed the fp16 two-part kernels' 32-bit sample index and "
                                       f"W={pk.width}, f_dim={pk.feat_dim} has no other instance; render fewer rays per launch")
                if fold and not (h3 and mode == L.FIELD_FULL):
                    raise RuntimeError("nefes_amd: a folded pack serves the full pass on the fp16 two-part kernels only")
                return route("nefes_field_fwd_h3" if h3 else "nefes_field_fwd_x6",
                             f"field_fwd[{name},{'h3' if h3 else 'x6'}{',fold' if fold else ''}]")
        if not canonical_shape(pk):
            raise RuntimeError(f"nefes_amd: the {name} forward of W={pk.width}, f_dim={pk.feat_dim} was routed to "
                               f"the fp32-MFMA instances (NEFES_SPLIT={SPLIT}; or a frozen network's static head with test_time=False), "
                               f"which exist for the canonical shapes only.  Compiled: {COMPILED_SET}")
        return route("nefes_field_fwd", f"field_fwd[{name}]")
    if mode == L.FIELD_STATIC:
        if switched and static_h3(pk) and M < H3_MAX_SAMPLES:
            return route("nefes_field_bwd_static_h3", "field_bwd[static,h3]")
        if not canonical_shape(pk):
            raise RuntimeError(f"nefes_amd: the static-head backward of W={pk.width}, f_dim={pk.feat_dim} was routed to the fp32-MFMA "
                               f"instances (NEFES_SPLIT={SPLIT}), which exist for the canonical shapes only.  Compiled: {COMPILED_SET}")
        return route("nefes_field_bwd_static", "field_bwd[static]")
    ext = pk.xyz_encoding == L.XYZ_EXTERNAL32
    if switched and x6_supported(pk, L.FIELD_FULL):
        h3 = _h3(pk)
        if fold and not h3:
            raise RuntimeError("nefes_amd: a folded pack serves the fp16 two-part kernels only")
        return route("nefes_field_bwd_h3" if h3 else "nefes_field_bwd_x6",
                     ("field_bwd[h3,fold]" if fold else "field_bwd[h3]") if h3 else "field_bwd[x6]", ext)
    return route("nefes_field_bwd", "field_bwd", ext)


def _blob(pk):
    return _chk(pk.blob, "blob", torch.uint8)


def _alloc_masks(pk, M, dev, want):
    return torch.empty(pk.mask_bytes(M) // 4, dtype=torch.int32, device=dev) if want else None


def _tap_masks(pk, masks, N, S, mode):
    if masks is not None and is_generic(pk):
        _tap("masks_generic", (masks, N, S, pk, mode))
    elif masks is not None:
        _tap("masks", (masks, N, S, pk.width, mode))


def _input_kind(z, pts, xyz_enc, grid):
    if grid is not None:
        return "hashgrid"
    if z is not None and z.dim() == 1:
        return "zrow"
    return "points" if pts is not None else ("enc" if xyz_enc is not None else "rays")


def _field_fwd(pk, mode, N, S, rays_o=None, rays_d=None, z=None, pts=None, xyz_enc=None, viewdirs=None, want_masks=False, grid=None,
               override=None):
    """THE forward launcher: the kernel field_route names, on freshly allocated raw_t [N, R, S] (+ the ReLU masks a backward needs).
    Inputs: rays_o / rays_d [N,3] with z [N,S] (or z [S]: one row shared by every ray), or pts [N*S,3], or xyz_enc [N*S,32];
    grid: an ops.HashGrid the kernel gathers itself."""
    rt = field_route(pk, mode, False, _input_kind(z, pts, xyz_enc, grid), N * S, override)
    dev = pk.blob.device
    raw_t = torch.empty(N, pk.n_raw(mode), S, device=dev)
    masks = _alloc_masks(pk, N * S, dev, want_masks)
    o, d, zz, v = _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(z, "z"), _chk(viewdirs, "viewdirs")
    if rt.entry == "nefes_field_fwd_generic":
        args = (mode, N, S, o, d, zz, _chk(pts, "pts"), v)
    elif rt.entry == "nefes_field_fwd_generic_ext":
        args = (mode, N, S, _chk(xyz_enc, "xyz_enc"), v)
    elif rt.entry == "nefes_field_fwd_h3_hashgrid":
        args = (grid.desc, _chk(grid.table, "table"), mode, N, S, o, d, zz, 1 if z.dim() == 1 else 0, v)
    elif rt.entry == "nefes_field_fwd_h3_zrow":
        args = (mode, N, S, o, d, zz, v)
    else:                                             # nefes_field_fwd, nefes_field_fwd_x6, nefes_field_fwd_h3: one prototype
        args = (mode, N, S, o, d, zz, _chk(pts, "pts"), _chk(xyz_enc, "xyz_enc"), v)
    with _timed(rt.key):
        L.check(getattr(L.load(), rt.entry)(pk.desc, _blob(pk), *args, _chk(raw_t, "raw_t"), _chk(masks, "masks", torch.int32), _stream()),
                rt.label)
    _tap_masks(pk, masks, N, S, mode)
    return raw_t, masks


def _field_bwd(pk, mode, N, S, raw_t, g_raw_t, masks, rays_o=None, rays_d=None, z=None, pts=None, viewdirs=None, grid=None, enc=False):
    """THE backward launcher: the kernel field_route names -> (d loss / d pts [N*S,3] -- or d loss / d encoding [N*S,32] for a pack on
    an external encoding --, d loss / d viewdirs per sample [N*S,3]).  enc: the forward's input was a supplied encoding."""
    rt = field_route(pk, mode, True, _input_kind(z, pts, True if enc else None, grid), N * S)
    dev = pk.blob.device
    g_in, g_vs = torch.empty(N * S, 32 if rt.g_enc else 3, device=dev), torch.empty(N * S, 3, device=dev)
    o, d, zz, v = _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(z, "z"), _chk(viewdirs, "viewdirs")
    out = (_chk(raw_t, "raw_t"), _chk(g_raw_t, "g_raw_t"), _chk(masks, "masks", torch.int32))
    if rt.entry == "nefes_field_bwd_generic":
        args = (mode, N, S, o, d, zz, _chk(pts, "pts"), v, *out, _chk(g_in, "g_pts"))
    elif rt.entry == "nefes_field_bwd_generic_ext":
        args = (mode, N, S, v, *out, _chk(g_in, "g_enc"))
    elif rt.entry == "nefes_field_bwd_h3_hashgrid":
        args = (grid.desc, _chk(grid.table, "table"), N, S, o, d, zz, v, *out, _chk(g_in, "g_pts"))
    elif rt.entry.startswith("nefes_field_bwd_static"):       # nefes_field_bwd_static, nefes_field_bwd_static_h3
        args = (N, S, o, d, zz, _chk(pts, "pts"), v, *out, _chk(g_in, "g_pts"))
    else:                                             # nefes_field_bwd, nefes_field_bwd_x6, nefes_field_bwd_h3: g_pts AND g_enc
        args = (N, S, o, d, zz, _chk(pts, "pts"), v, *out, None if rt.g_enc else _chk(g_in, "g_pts"), _chk(g_in, "g_enc") if rt.g_enc else None)
    with _timed(rt.key):
        L.check(getattr(L.load(), rt.entry)(pk.desc, _blob(pk), *args, _chk(g_vs, "g_vs"), _stream()), rt.label)
    return g_in, g_vs


def field_fwd(pk, mode, N, S, rays_o=None, rays_d=None, z=None, pts=None, viewdirs=None, want_masks=False, xyz_enc=None):
    """The strict fp32-MFMA forward (canonical shapes) -> (raw_t, masks)."""
    return _field_fwd(pk, mode, N, S, rays_o, rays_d, z, pts, xyz_enc, viewdirs, want_masks, override="f32")


def field_fwd_x6(pk, mode, N, S, rays_o=None, rays_d=None, z=None, viewdirs=None, want_masks=False, xyz_enc=None, pts=None):
    """field_fwd on the split-product instances (same outputs, same mask words): fp16 two-part (default) or bf16x6, with the
    fallbacks of field_route's split route."""
    return _field_fwd(pk, mode, N, S, rays_o, rays_d, z, pts, xyz_enc, viewdirs, want_masks, override="split")


def field_bwd(pk, N, S, raw_t, g_raw_t, masks, rays_o=None, rays_d=None, z=None, pts=None, viewdirs=None, mode=L.FIELD_FULL):
    return _field_bwd(pk, mode, N, S, raw_t, g_raw_t, masks, rays_o, rays_d, z, pts, viewdirs)


def field_fwd_generic(pk, mode, N, S, rays_o=None, rays_d=None, z=None, pts=None, viewdirs=None, want_masks=False):
    return _field_fwd(pk, mode, N, S, rays_o, rays_d, z, pts, None, viewdirs, want_masks)


def field_bwd_generic(pk, mode, N, S, raw_t, g_raw_t, masks, rays_o=None, rays_d=None, z=None, pts=None, viewdirs=None):
    return _field_bwd(pk, mode, N, S, raw_t, g_raw_t, masks, rays_o, rays_d, z, pts, viewdirs)


def ray_grad_reduce(N, S, z, g_pts, g_vs):
    dev = g_pts.device
    g_o, g_d, g_v = (torch.empty(N, 3, device=dev) for _ in range(3))
    with _timed("ray_grad_reduce"):
      L.check(L.load().nefes_ray_grad_reduce(N, S, _chk(z, "z"), _chk(g_pts, "g_pts"), _chk(g_vs, "g_vs"), _chk(g_o, "g_o"),
                                           _chk(g_d, "g_d"), _chk(g_v, "g_v"), _stream()), "nefes_ray_grad_reduce")
    return g_o, g_d, g_v


_NO_SIGMA_BWD = ("nefes_amd: the sigma-only field pass has no backward (the reference evaluates it without gradients at test time: "
                 "nerfh_nff.py:192-202)")


def _fh_fwd(pk, rays_o, rays_d, viewdirs, z, want_masks):
    """The factored-head forward launch -> (raw_t [N, 3 + (W/2 + 1) + 6, S] = rgb | g | ones | sigma | transient (5), masks)."""
    N, S = z.shape
    raw_t = torch.empty(N, 3 + pk.width // 2 + 1 + 6, S, device=z.device)
    masks = _alloc_masks(pk, N * S, z.device, want_masks)
    with _timed("field_fwd[full,h3,fh]"):
        L.check(L.load().nefes_field_fwd_h3_fh(pk.desc, _blob(pk), L.FIELD_FULL, N, S, _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"),
                                               _chk(z, "z"), _chk(viewdirs, "viewdirs"), _chk(raw_t, "raw_t"),
                                               _chk(masks, "masks", torch.int32), _stream()), "nefes_field_fwd_h3_fh")
    _tap_masks(pk, masks, N, S, L.FIELD_FULL)
    return raw_t, masks


def _fh_bwd(pk, rays_o, rays_d, viewdirs, z, raw_t, g_raw_t, g_gmap, masks):
    """The factored-head backward launch -> (d loss / d pts, d loss / d viewdirs), per sample [N*S, 3].  g_gmap [N, W/2 + 1]: the per-ray
    gradient of the composited g channels (the kernel forms d loss / d g = w_s g_gmap[ray] itself), or None: g_raw_t holds it."""
    N, S = z.shape
    g_pts, g_vs = torch.empty(N * S, 3, device=z.device), torch.empty(N * S, 3, device=z.device)
    with _timed("field_bwd[h3,fh]"):
        L.check(L.load().nefes_field_bwd_h3_fh(pk.desc, _blob(pk), N, S, _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(z, "z"),
                                               _chk(viewdirs, "viewdirs"), _chk(raw_t, "raw_t"), _chk(g_raw_t, "g_raw_t"),
                                               _chk(g_gmap, "g_gmap"), _chk(masks, "masks", torch.int32), _chk(g_pts, "g_pts"),
                                               _chk(g_vs, "g_vs"), _stream()), "nefes_field_bwd_h3_fh")
    return g_pts, g_vs


# What tells the kinds of frozen-field Function apart; everything else they do is _field_forward / _field_backward.
#   inputs:  the launchers' keyword of each tensor input, in apply()'s order; the first n_diff are differentiable (z is not)
#   saved:   the inputs the backward launch reads again (raw_t and the ReLU masks always are)
#   modes:   (pk, mode) -> this pass has a backward
#   refusal: what backward() raises where it has none; None: it returns None for every input
#   per_ray: the per-sample gradients are reduced along each ray with its depths -> (g_o, g_d, g_v).  Otherwise the first input's
#            gradient is returned per sample and g_v comes from the same reduction on zero depths
#   n_args:  apply()'s argument count, the length of what backward() returns
FieldKind = collections.namedtuple("FieldKind", "inputs n_diff saved modes refusal per_ray n_args")
_RAY_INPUTS = ("rays_o", "rays_d", "viewdirs", "z")
_full_or_static = lambda pk, mode: mode in (L.FIELD_FULL, L.FIELD_STATIC)
_RAYS = FieldKind(_RAY_INPUTS, 3, _RAY_INPUTS, _full_or_static, _NO_SIGMA_BWD, True, 6)
_POINTS = FieldKind(("pts", "viewdirs"), 2, ("pts", "viewdirs"), _full_or_static, _NO_SIGMA_BWD, False, 4)
# (the generic backward on a supplied encoding has a STATIC mode -- a coarse network with test_time False --, the tuned instances do not)
_ENC = FieldKind(("xyz_enc", "viewdirs"), 2, ("viewdirs",), lambda pk, mode: mode == L.FIELD_FULL or (mode == L.FIELD_STATIC and is_generic(pk)),
                 "nefes_amd: field backward is built for the FULL (fine) mode only", False, 4)
_HASHGRID = FieldKind(_RAY_INPUTS, 3, _RAY_INPUTS, lambda pk, mode: mode == L.FIELD_FULL, _NO_SIGMA_BWD, True, 7)
_FH = FieldKind(_RAY_INPUTS, 3, _RAY_INPUTS, lambda pk, mode: True, None, True, 5)      # (launched by _fh_fwd / _fh_bwd)


def _field_forward(ctx, kind, pk, mode, N, S, *tensors, grid=None, also_save=()):
    """The forward of every frozen-field Function: `tensors` (kind.inputs, shaped as the launcher takes them) cast to fp32, one launch
    -> raw_t.  The ReLU masks are written, and ctx keeps (kind.saved, raw_t, masks, *also_save), only where a backward can follow."""
    x = {k: _f32(t) for k, t in zip(kind.inputs, tensors)}
    need = kind.modes(pk, mode) and any(ctx.needs_input_grad[:kind.n_diff])
    if kind is _FH:
        raw_t, masks = _fh_fwd(pk, want_masks=need, **x)
    else:
        raw_t, masks = _field_fwd(pk, mode, N, S, want_masks=need, grid=grid, **x)
    ctx.kind, ctx.pk, ctx.mode, ctx.NS, ctx.grid, ctx.have, ctx.pk_gen = kind, pk, mode, (N, S), grid, need, pk.generation
    if need:
        ctx.save_for_backward(*(x[k] for k in kind.saved), raw_t, masks, *also_save)
    return raw_t


def _field_backward(ctx, g_raw_t, g_gmap=None):
    """The backward of every frozen-field Function -> one entry per argument of apply().  g_gmap: _fh_bwd's."""
    kind, pk, (N, S) = ctx.kind, ctx.pk, ctx.NS
    if not ctx.have:
        if kind.refusal is None:
            return (None,) * kind.n_args
        raise NotImplementedError(kind.refusal)
    saved, n = ctx.saved_tensors, len(kind.saved)
    x, (raw_t, masks) = dict(zip(kind.saved, saved)), saved[n:n + 2]
    pk.check_generation(ctx.pk_gen)
    if kind is _FH:
        g_in, g_vs = _fh_bwd(pk, raw_t=raw_t, g_raw_t=_f32(g_raw_t), g_gmap=g_gmap, masks=masks, **x)
    else:
        g_in, g_vs = _field_bwd(pk, ctx.mode, N, S, raw_t, _f32(g_raw_t), masks, grid=ctx.grid, enc=kind is _ENC, **x)
    if kind.per_ray:
        grads = ray_grad_reduce(N, S, x["z"], g_in, g_vs)
    else:
        zeros = torch.zeros(N, S, device=raw_t.device)
        # (the reduction reads [N*S, 3] in g_pts' place and its g_o, g_d are dropped: an encoding's [N*S, 32] gradient does not go there)
        grads = g_in.reshape(N, S, -1), ray_grad_reduce(N, S, zeros, g_vs if kind is _ENC else g_in, g_vs)[2]
    return grads + (None,) * (kind.n_args - len(grads))


class FieldFromRays(torch.autograd.Function):
    """Fused pts = o + d*z -> embed -> MLP (rendering.py:142 + nerfh_nff.py:217-231, :525-576) on whichever kernels field_route names
    for `pk` (a tuned or a generic pack).  Returns raw_t [N, R, S].  Differentiable w.r.t. rays_o, rays_d, viewdirs in FULL and
    STATIC mode (frozen weights)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, pk, mode):
        return _field_forward(ctx, _RAYS, pk, mode, *z.shape, rays_o, rays_d, viewdirs, z)

    backward = staticmethod(_field_backward)


class FieldFromPoints(torch.autograd.Function):
    """run_network_NeRFH_NFF call surface: explicit pts [N,S,3] (+ viewdirs [N,3]) -> raw_t [N,R,S], on a tuned or a generic pack."""

    @staticmethod
    def forward(ctx, pts, viewdirs, pk, mode):
        N, S = pts.shape[0], pts.shape[1]
        viewdirs = torch.zeros(N, 3, device=pts.device) if viewdirs is None else viewdirs
        return _field_forward(ctx, _POINTS, pk, mode, N, S, pts.reshape(-1, 3), viewdirs)

    backward = staticmethod(_field_backward)


class FieldFromEncoding(torch.autograd.Function):
    """Field MLP on a caller-supplied 32-feature xyz embedding (hash grid, BASELINE config 4): enc [N,S,32], viewdirs [N,3]
    -> raw_t [N,R,S]; backward to enc and viewdirs: FULL mode on a tuned pack, FULL and STATIC on a generic one (packed_generic of a
    network with in_channels_xyz=32: any width / depth)."""

    @staticmethod
    def forward(ctx, enc, viewdirs, pk, mode):
        N, S = enc.shape[0], enc.shape[1]
        viewdirs = torch.zeros(N, 3, device=enc.device) if viewdirs is None else viewdirs
        return _field_forward(ctx, _ENC, pk, mode, N, S, enc.reshape(-1, 32), viewdirs)

    backward = staticmethod(_field_backward)


class FieldFromRaysHashGrid(torch.autograd.Function):
    """pts = o + d z -> hash-grid encoding -> MLP in ONE launch each way (rendering.py:114,142 + nerfh_tcnn.py:151-182): raw_t [N, R, S];
    differentiable w.r.t. rays_o, rays_d, viewdirs in FULL mode (frozen weights, frozen table).  Forward bit-identical to
    HashGridEncode + FieldFromEncoding.  The caller asks hashgrid_fused_ok first (NEFES_FUSED_HASHGRID: "0" = those separate launches)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, pk, mode, grid):
        return _field_forward(ctx, _HASHGRID, pk, mode, *z.shape, rays_o, rays_d, viewdirs, z, grid=grid)

    backward = staticmethod(_field_backward)


class FieldFromRaysFH(torch.autograd.Function):
    """FieldFromRays for the factored head: raw_t [N, 3 + (W/2 + 1) + 6, S] = rgb | g | ones | sigma | transient (5); pk = the network packed
    without its feature rows (NeRFH_NFF.packed_fh).  Differentiable w.r.t. rays_o, rays_d, viewdirs (frozen weights)."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, pk):
        if z.shape[0] * z.shape[1] >= H3_MAX_SAMPLES:
            raise RuntimeError("nefes_amd: too many samples for one launch of the fp16 two-part kernels (32-bit sample index)")
        return _field_forward(ctx, _FH, pk, L.FIELD_FULL, *z.shape, rays_o, rays_d, viewdirs, z)

    backward = staticmethod(_field_backward)


def _feat_head_fwd(gmap, w_t, b):
    """feat [N, C] = gmap[:, :F] W^T + gmap[:, F:] b (csrc/refine.hip feat_head_fwd_kernel); w_t [F, C], the head's matrix transposed."""
    N, C = gmap.shape[0], w_t.shape[1]
    feat = torch.empty(N, C, device=gmap.device)
    with _timed("feat_head_fwd"):
        L.check(L.load().nefes_feat_head_fwd(N, C, gmap.shape[1] - 1, _chk(gmap, "gmap"), _chk(w_t, "w_t"), _chk(b, "b"), _chk(feat, "feat"), _stream()),
                "nefes_feat_head_fwd")
    return feat


def _feat_head_bwd(g_feat, w, b):
    """g_gmap [N, F + 1] of _feat_head_fwd (feat_head_bwd_kernel); w [C, F]."""
    N, (C, F) = g_feat.shape[0], w.shape
    g_gmap = torch.empty(N, F + 1, device=g_feat.device)
    with _timed("feat_head_bwd"):
        L.check(L.load().nefes_feat_head_bwd(N, C, F, _chk(g_feat, "g_feat"), _chk(w, "w"), _chk(b, "b"), _chk(g_gmap, "g_gmap"), _stream()),
                "nefes_feat_head_bwd")
    return g_gmap


class FeatHead(torch.autograd.Function):
    """The factored head's per-ray part: feat [N, C] = gmap[:, :F] W^T + gmap[:, F:] b (csrc/refine.hip feat_head_*_kernel; W, b frozen)."""

    @staticmethod
    def forward(ctx, gmap, w, w_t, b):
        ctx.save_for_backward(w, b)
        return _feat_head_fwd(_f32(gmap), w_t, b)

    @staticmethod
    def backward(ctx, g_feat):
        return _feat_head_bwd(_f32(g_feat), *ctx.saved_tensors), None, None, None


class RenderFineFH(torch.autograd.Function):
    """The fine pass of a frozen width-128 network at test time with the factored head, as ONE autograd node: field forward (g channels) ->
    compositing -> per-ray feature head; and back: feature head -> compositing backward, which leaves the static weight where the g
    channels' gradient would go (COMP_FEAT_WEIGHTS_ONLY) -> field backward, which forms d loss / d g = w_s g_gmap[ray] itself.  One node
    because that backward hands TWO tensors from the compositor's stage to the field's (g_raw_t and the per-ray g_gmap).
    -> (rgb [N,3], feat [N,C], disp [N], acc [N]); differentiable w.r.t. rays_o, rays_d, viewdirs.
    `want_depth`: a fifth output, the compositor's depth [N] = sum_s w_s z_s over the weights the variant uses, with its gradient
    handed to the compositing backward (g_depth); without it the node returns and launches exactly what it did before."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, z, pk, w_f, w_f_t, b_f, flags, beta_min, emit_gmap=False, want_depth=False):
        z = _f32(z)                   # (the compositor reads it too)
        Cg = pk.width // 2
        raw_t = _field_forward(ctx, _FH, pk, L.FIELD_FULL, *z.shape, rays_o, rays_d, viewdirs, z, also_save=(w_f, b_f))
        rgb, gmap, disp, acc, depth, _, _ = composite_fwd(raw_t, z, Cg + 1, flags, beta_min)
        # emit_gmap: the caller applies the feature head itself, folded into whatever linear layer consumes the features (the refinement
        # loop: FusionNet's first convolution, FusionNet.forward_prepared_gmap): feat = [N, Cg + 1] = (sum_s w_s g_s, sum_s w_s)
        feat = gmap if emit_gmap else _feat_head_fwd(gmap, w_f_t, b_f)
        ctx.set_materialize_grads(False)
        ctx.cfg, ctx.emit_gmap = (Cg, int(flags)), bool(emit_gmap)
        return (rgb, feat, disp, acc, depth) if want_depth else (rgb, feat, disp, acc)

    @staticmethod
    def backward(ctx, g_rgb, g_feat, g_disp, g_acc, g_depth=None):
        if not ctx.have:
            return (None,) * 12
        z, raw_t, _, w_f, b_f = ctx.saved_tensors[3:]      # (_field_forward's layout: _FH.saved = the four ray inputs, raw_t, masks, also_save)
        N, S = ctx.NS
        ctx.pk.check_generation(ctx.pk_gen)        # (before the head and the compositor are launched, not only before the field)
        Cg, flags = ctx.cfg
        fix = lambda g: None if (g is None or g.numel() == 0) else _f32(g)
        g_rgb, g_feat, g_disp, g_acc, g_depth = fix(g_rgb), fix(g_feat), fix(g_disp), fix(g_acc), fix(g_depth)
        if g_feat is None:
            g_gmap = torch.zeros(N, Cg + 1, device=z.device)
        else:                                                # (with emit_gmap it already is d loss / d (sum_s w_s g_s, sum_s w_s))
            g_gmap = g_feat if ctx.emit_gmap else _feat_head_bwd(g_feat, w_f, b_f)
        g_raw_t = torch.empty_like(raw_t)          # (the g channels' rows beyond the first are neither written nor read)
        with _timed("composite_bwd"):
            L.check(L.load().nefes_composite_bwd(N, S, Cg + 1, flags | L.COMP_FEAT_WEIGHTS_ONLY, _chk(raw_t, "raw_t"), _chk(z, "z"),
                                                 _chk(g_rgb, "g_rgb"), None, _chk(g_disp, "g_disp"), _chk(g_acc, "g_acc"), _chk(g_depth, "g_depth"),
                                                 None, None, _chk(g_raw_t, "g_raw_t"), _stream()), "nefes_composite_bwd")
        return _field_backward(ctx, g_raw_t, g_gmap) + (None,) * 7


# ---------------------------------------------------------------------------------------------
# generic field kernels (csrc/field_generic.hip): any --netwidth / --netdepth, frozen weights
# ---------------------------------------------------------------------------------------------
# "1": a trainable network on the generic kernels trains (train.field_train_generic: their train-mode instances + the weight-gradient
# kernels of csrc/train.hip).  Off by default: such a network is refused, as before the train-mode instances existed.
GENERIC_TRAIN = os.environ.get("NEFES_GENERIC_TRAIN", "0") == "1"
# "1": the same for a trainable network behind an xyz encoder (a hash grid; train.field_train_generic_encoded, the train-mode instances
# on a supplied encoding).  A switch of its own, off by default and sufficient alone: GENERIC_TRAIN does not reach such a network.
GENERIC_TRAIN_EXT = os.environ.get("NEFES_GENERIC_TRAIN_EXT", "0") == "1"
GENERIC_SET = L.GENERIC_SET


def generic_shape_ok(width, depth, skips, feat_dim):
    """csrc/field_generic.hip gen_desc_ok with the reference's skip rule (nerfh_nff.py:469-477,549-553: skips=[4] acts when D > 4)."""
    skips = [s for s in skips if 0 <= s < depth]
    return (width % 32 == 0 and 32 <= width <= 512 and 1 <= depth <= 8 and skips in ([], [4])
            and 0 < feat_dim <= HEAD_MAX_C)


class PackedGeneric:
    """Device-resident weights of one NeRFH_NFF network in the generic kernels' layout (nefes_generic_pack): per layer the matrix
    transposed, the matrix, the bias -- plain padded fp32.  Packed on the host once; repack() refreshes the same blob on the device
    (a trainable network after an optimiser step: no host copy, no sync)."""

    generic = True
    h3_valid = False             # (never on the fp16 two-part instances: fused_coarse_pass_ok and friends say no)

    @staticmethod
    def layer_names(depth, has_transient):
        names = [f"xyz_encoding_{i}.0" for i in range(1, depth + 1)] + ["xyz_encoding_final", "dir_encoding.0", "static_sigma.0", "static_rgb.0"]
        if has_transient:
            names += PackedField.LAYERS_FINE[len(PackedField.LAYERS_COARSE):]
        return names

    def __init__(self, state_dict, width, depth, skip, feat_dim, has_transient, device, xyz_encoding=L.XYZ_FREQ10):
        lib = L.load()
        self.desc = L.NefesGenericNetDesc(int(width), int(depth), int(skip), int(feat_dim), 1 if has_transient else 0, int(xyz_encoding))
        self.xyz_encoding = int(xyz_encoding)      # XYZ_EXTERNAL32: xyz_encoding_1 / the skip layer take 32 supplied features, unpadded
        self.width, self.depth, self.skip = int(width), int(depth), int(skip)
        self.feat_dim, self.has_transient = int(feat_dim), bool(has_transient)
        n = int(lib.nefes_generic_blob_bytes(self.desc))
        if n == 0:
            raise RuntimeError(f"nefes_amd: no field kernel serves W={width}, D={depth}, skip={skip}, f_dim={feat_dim}, "
                               f"xyz_encoding={xyz_encoding}.  "
                               f"Compiled: {COMPILED_SET}")
        host = []
        for name in self.layer_names(self.depth, self.has_transient):
            host.append(state_dict[name + ".weight"].detach().to("cpu", torch.float32).contiguous())
            host.append(state_dict[name + ".bias"].detach().to("cpu", torch.float32).contiguous())
        ptrs = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
        blob = torch.zeros(n, dtype=torch.uint8)
        L.check(lib.nefes_generic_pack(self.desc, ptrs, len(host), C.c_void_p(blob.data_ptr()), blob.numel()), "nefes_generic_pack")
        self.blob = blob.to(device)
        self.generation = 0
        self.tile = 64 if self.width <= 256 else 32

    def repack(self, state_dict):
        """Same blob (same pointer, same shapes) from the current values of the parameters, on the device (nefes_generic_pack_device:
        bit-identical to the host packer; the blob's padding was zeroed at allocation and is never written)."""
        dev = self.blob.device
        t = []
        for name in self.layer_names(self.depth, self.has_transient):
            t.append(state_dict[name + ".weight"].detach().to(dev, torch.float32).contiguous())
            t.append(state_dict[name + ".bias"].detach().to(dev, torch.float32).contiguous())
        ptrs = (C.c_void_p * len(t))(*[x.data_ptr() for x in t])
        L.check(L.load().nefes_generic_pack_device(self.desc, ptrs, len(t), C.c_void_p(self.blob.data_ptr()), self.blob.numel(), _stream()),
                "nefes_generic_pack_device")
        self.generation += 1
        del t            # (stream-ordered allocator: temporaries made above stay valid for the launches already queued)

    def check_generation(self, gen):
        if gen != self.generation:
            raise RuntimeError("nefes_amd: the network weights were re-packed between this forward pass and its backward pass")

    def mask_bytes(self, M):
        return L.load().nefes_generic_mask_bytes(self.desc, M)

    def train_rows(self):
        """(rows per tile, first row of block L.TB_*) of the train-mode acts / dacts buffers (nefes_generic_train_row_offset, or its
        _ext twin for a pack on a supplied encoding: the E block is that encoding's 32 rows)."""
        lib = L.load()
        rows, offset = lib.nefes_generic_train_rows, lib.nefes_generic_train_row_offset
        if self.xyz_encoding == L.XYZ_EXTERNAL32:
            rows, offset = lib.nefes_generic_train_rows_ext, lib.nefes_generic_train_row_offset_ext
        return int(rows(self.desc)), [int(offset(self.desc, b)) for b in range(L.TB_END + 1)]

    def n_raw(self, mode):
        return 1 if mode == L.FIELD_SIGMA else (3 + self.feat_dim + (1 if mode == L.FIELD_STATIC else 6))


def field_from_rays(rays_o, rays_d, viewdirs, z, pk, mode):
    """The field along rays on whichever kernels `pk` was packed for (NeRFH_NFF.packed_any)."""
    return FieldFromRays.apply(rays_o, rays_d, viewdirs, z, pk, mode)


def field_from_points(pts, viewdirs, pk, mode):
    return FieldFromPoints.apply(pts, viewdirs, pk, mode)


# ---------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------
def composite_fwd(raw_t, z, C_feat, flags, beta_min=0.1):
    N, _, S = raw_t.shape
    dev = raw_t.device
    sigma_only = bool(flags & L.COMP_SIGMA_ONLY)
    acc = torch.empty(N, device=dev)
    weights = torch.empty(N, S, device=dev)
    if sigma_only:
        rgb = feat = disp = depth = beta = None
    else:
        rgb, feat = torch.empty(N, 3, device=dev), torch.empty(N, C_feat, device=dev)
        disp, depth, beta = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    with _timed("composite_fwd[D]" if sigma_only else "composite_fwd"):
      L.check(L.load().nefes_composite_fwd(N, S, C_feat, flags, float(beta_min), _chk(raw_t, "raw_t"), _chk(z, "z"),
                                         _chk(rgb, "rgb"), _chk(feat, "feat"), _chk(disp, "disp"), _chk(acc, "acc"),
                                         _chk(depth, "depth"), _chk(weights, "weights"), _chk(beta, "beta"), _stream()),
            "nefes_composite_fwd")
    return rgb, feat, disp, acc, depth, weights, beta


class Composite(torch.autograd.Function):
    """raw2outputs_NeRFH_NFF (nerfh_nff.py:25-166) on raw_t [N,R,S]; z carries no gradient (detached in the reference)."""

    @staticmethod
    def forward(ctx, raw_t, z, C_feat, flags, beta_min):
        raw_t, z = _f32(raw_t), _f32(z)
        outs = composite_fwd(raw_t, z, C_feat, flags, beta_min)
        ctx.set_materialize_grads(False)      # maps nobody differentiates arrive as None, not as freshly zero-filled tensors
        ctx.save_for_backward(raw_t, z)
        ctx.cfg = (C_feat, flags)
        if flags & L.COMP_SIGMA_ONLY:
            _, _, _, acc, _, weights, _ = outs
            dummy = raw_t.new_zeros(0)
            return dummy, dummy, dummy, acc, dummy, weights, dummy
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_feat, g_disp, g_acc, g_depth, g_weights, g_beta):
        raw_t, z = ctx.saved_tensors
        C_feat, flags = ctx.cfg
        N, R, S = raw_t.shape
        g_raw_t = torch.empty_like(raw_t)
        so = bool(flags & L.COMP_SIGMA_ONLY)
        fix = lambda g, ok=True: None if (g is None or not ok or g.numel() == 0) else _f32(g)
        g_rgb, g_feat, g_disp, g_depth, g_beta = (fix(g, not so) for g in (g_rgb, g_feat, g_disp, g_depth, g_beta))
        g_acc, g_weights = fix(g_acc), fix(g_weights)
        with _timed("composite_bwd"):
          L.check(L.load().nefes_composite_bwd(N, S, C_feat, flags, _chk(raw_t, "raw_t"), _chk(z, "z"), _chk(g_rgb, "g_rgb"),
                                             _chk(g_feat, "g_feat"), _chk(g_disp, "g_disp"), _chk(g_acc, "g_acc"),
                                             _chk(g_depth, "g_depth"), _chk(g_weights, "g_weights"), _chk(g_beta, "g_beta"),
                                             _chk(g_raw_t, "g_raw_t"), _stream()), "nefes_composite_bwd")
        return g_raw_t, None, None, None, None


# ---------------------------------------------------------------------------------------------
# hierarchical sampling
# ---------------------------------------------------------------------------------------------
def sample_pdf_merge(z_coarse, weights, Ni, u=None, cdf=None, want_debug=False, bins_layout=False):
    """sample_pdf + sort(cat) (rendering.py:23-66,132-141).  u=None -> deterministic linspace(0,1,Ni).
    bins_layout=True: (z_coarse, weights) are the reference's (bins, weights) arguments; no merge."""
    z_coarse, weights = _f32(z_coarse), _f32(weights)
    N, Nc = z_coarse.shape
    if bins_layout:
        Nc += 1
    dev = z_coarse.device
    if u is None:
        u = _linspace01(Ni, dev)                                     # rendering.py:33 bits
    u = _f32(u)
    per_ray = 1 if u.dim() == 2 else 0
    z_fine = None if bins_layout else torch.empty(N, Nc + Ni, device=dev)
    z_samples = torch.empty(N, Ni, device=dev)
    inds = torch.empty(N, Ni, dtype=torch.int32, device=dev) if want_debug else None
    cdf_out = torch.empty(N, Nc - 1, device=dev) if want_debug else None
    cdf = None if cdf is None else _f32(cdf)
    with _timed("sample_pdf_merge"):
      L.check(L.load().nefes_sample_pdf_merge(N, Nc, Ni, 1 if bins_layout else 0, _chk(z_coarse, "z_coarse"), _chk(weights, "weights"), _chk(u, "u"),
                                            per_ray, _chk(cdf, "cdf"), _chk(z_fine, "z_fine"), _chk(z_samples, "z_samples"),
                                            _chk(inds, "inds", torch.int32), _chk(cdf_out, "cdf_out"), _stream()),
            "nefes_sample_pdf_merge")
    _tap("z_fine", z_fine)
    _tap("z_samples", z_samples)
    if want_debug:
        return z_fine, z_samples, inds, cdf_out
    return z_fine, z_samples


# ---------------------------------------------------------------------------------------------
# hash-grid encoding (BASELINE config 4; parity unpinned, see oracle/hashgrid_ref.py)
# ---------------------------------------------------------------------------------------------
class HashGrid:
    """Table + geometry of a tiny-cuda-nn style multiresolution hash grid (nerfh_tcnn.py:60-75).

    `table` is a plain fp32 tensor [entries, 2] that does not require grad: the grid is frozen and every path runs as it always did.
    `grid.table.requires_grad_(True)` makes it trainable -- HashGridEncode then returns d loss / d table (nefes_hashgrid_bwd_table),
    render() routes the grid through the separate encode + field launches, and `grid.parameters()` hands it to an optimiser.
    `n_levels=1` is one level of scale `base_resolution - 1`; a geometry the library refuses raises RuntimeError."""

    def __init__(self, bound, table=None, n_levels=16, log2_hashmap_size=19, base_resolution=16, max_resolution=2048,
                 device="cuda"):
        import math
        # a single level has no growth factor: its scale is base_resolution - 1 and max_resolution is not used
        growth = math.exp(math.log(max_resolution / base_resolution) / (n_levels - 1)) if n_levels > 1 else 1.0
        self.desc = L.NefesHashGridDesc(n_levels, 2, log2_hashmap_size, base_resolution, growth, float(bound))
        self.n_out = 2 * n_levels
        n = L.load().nefes_hashgrid_table_entries(self.desc)
        if n == 0:
            raise RuntimeError("nefes_amd: unsupported hash-grid configuration")
        if table is None:
            g = torch.Generator().manual_seed(0)
            table = (torch.rand(n, 2, generator=g) * 2 - 1) * 1e-4
        if tuple(table.shape) != (n, 2):
            raise RuntimeError(f"nefes_amd: hash-grid table must be [{n}, 2]")
        self.table = table.to(device, torch.float32).contiguous()

    def __call__(self, x):
        return HashGridEncode.apply(x, self.table, self)

    def parameters(self):
        """[table] -- for torch.optim, e.g. Adam([*net.parameters(), *grid.parameters()]) after table.requires_grad_(True)."""
        return [self.table]

    @property
    def trainable(self):
        """autograd records a gradient for the table in the current context."""
        return torch.is_grad_enabled() and self.table.requires_grad


def hashgrid_bwd_table(grid, x, g_enc, g_table=None):
    """g_table [entries, 2] (+)= d loss / d table for enc = grid(x), x [M, 3], g_enc [M, 32] (atomics: reproducible to rounding, not
    bitwise; the dense levels are summed in fp64 and rounded once).  g_table=None: a fresh zeroed buffer; otherwise the call adds into
    the one given."""
    lib = L.load()
    if g_table is None:
        g_table = torch.zeros_like(grid.table, dtype=torch.float32)
    ws = torch.empty(max(1, int(lib.nefes_hashgrid_bwd_table_workspace(grid.desc))), dtype=torch.uint8, device=g_table.device)
    with _timed("hashgrid_bwd_table"):
        L.check(lib.nefes_hashgrid_bwd_table(grid.desc, x.shape[0], _chk(x, "x"), _chk(g_enc, "g_enc"), _chk(g_table, "g_table"),
                                             C.c_void_p(ws.data_ptr()), _stream()), "nefes_hashgrid_bwd_table")
    return g_table


class HashGridEncode(torch.autograd.Function):
    """enc = grid(x): x [..., 3] -> [..., 32]; differentiable w.r.t. x (nefes_hashgrid_bwd_x) and, when it requires grad, the table
    (nefes_hashgrid_bwd_table).  `table` is grid.table, passed as an input so that autograd routes its gradient."""

    @staticmethod
    def forward(ctx, x, table, grid):
        shape = x.shape
        xf = _f32(x).reshape(-1, 3)
        enc = torch.empty(xf.shape[0], grid.n_out, device=xf.device)
        with _timed("hashgrid_fwd"):
            L.check(L.load().nefes_hashgrid_fwd(grid.desc, _chk(table, "table"), xf.shape[0], _chk(xf, "x"),
                                                _chk(enc, "enc"), _stream()), "nefes_hashgrid_fwd")
        ctx.save_for_backward(xf)
        ctx.grid, ctx.shape = grid, shape
        return enc.reshape(*shape[:-1], grid.n_out)

    @staticmethod
    def backward(ctx, g_enc):
        (xf,) = ctx.saved_tensors
        g = _f32(g_enc).reshape(-1, ctx.grid.n_out)
        g_x = g_table = None
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(xf)
            with _timed("hashgrid_bwd_x"):
                L.check(L.load().nefes_hashgrid_bwd_x(ctx.grid.desc, _chk(ctx.grid.table, "table"), xf.shape[0], _chk(xf, "x"),
                                                      _chk(g, "g_enc"), _chk(g_x, "g_x"), _stream()), "nefes_hashgrid_bwd_x")
            g_x = g_x.reshape(ctx.shape)
        if ctx.needs_input_grad[1]:
            g_table = hashgrid_bwd_table(ctx.grid, xf, g)
        return g_x, g_table, None


_CONV_PACK = {}     # (id(weight), backward) -> (weakref to the weight, its version, packed [Cin even][K*K][Cout multiple of 32])


def _pack_conv(w, backward):
    """Packed A operands of nefes_conv2d_same for a frozen Conv2d weight [Cout, Cin, K, K]; backward: the flipped, transposed
    weights (gradient w.r.t. the layer's input).  Cached per weight tensor and version (the entry holds a weak reference: an
    address re-used by another tensor is not a hit)."""
    import weakref
    key = (id(w), backward)
    hit = _CONV_PACK.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version:
        return hit[2]
    wd = w.detach().to(torch.float32)
    if backward:
        wd = wd.flip(2, 3).transpose(0, 1)
    co, ci, k, _ = wd.shape
    pk = torch.zeros((ci + 1) // 2 * 2, k * k, (co + 31) // 32 * 32, device=w.device)
    pk[:ci, :, :co] = wd.permute(1, 2, 3, 0).reshape(ci, k * k, co)
    for dead in [kk for kk, v in _CONV_PACK.items() if v[0]() is None]:
        del _CONV_PACK[dead]
    _CONV_PACK[key] = (weakref.ref(w), w._version, pk)
    return pk


def _conv2d_same(x, wp, cout, ksize, bias, relu, mask=None):
    B, cin, H, W = x.shape
    y = torch.empty(B, cout, H, W, device=x.device)
    with _timed("conv2d_same"):
        L.check(L.load().nefes_conv2d_same(B, cin, cout, H, W, ksize, _chk(x, "x"), _chk(mask, "mask"), _chk(wp, "w_packed"),
                                           _chk(bias, "bias"), int(relu), y.data_ptr(), _stream()), "nefes_conv2d_same")
    return y


def _conv2d_wgrad(x, gy, mask, cout, ksize, want_bias):
    """(g_w [cout, cin, k, k], g_bias [cout] or None) of nefes_conv2d_wgrad; mask: the layer's output after ReLU, or None."""
    B, cin, H, W = x.shape
    lib = L.load()
    nbytes = lib.nefes_conv2d_wgrad_workspace(B, cin, cout, H, W, ksize)
    if nbytes == 0:
        L.check(-2, "nefes_conv2d_wgrad")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    g_w = torch.empty(cout, cin, ksize, ksize, device=x.device)
    g_b = torch.empty(cout, device=x.device) if want_bias else None
    with _timed("conv2d_wgrad"):
        L.check(lib.nefes_conv2d_wgrad(B, cin, cout, H, W, ksize, _chk(x, "x"), _chk(gy, "g_y"), _chk(mask, "mask"), _chk(g_w, "g_w"),
                                       _chk(g_b, "g_bias"), C.c_void_p(ws.data_ptr()), _stream()), "nefes_conv2d_wgrad")
    return g_w, g_b


class Conv2dSame(torch.autograd.Function):
    """Conv2d(stride 1, "same" zero padding, 3x3 or 5x5) [+ ReLU], differentiable w.r.t. its input and -- where they require it -- its
    weight and bias.  Forward and the input gradient are the same implicit-GEMM kernel (csrc/conv.hip); the ReLU derivative is applied
    to the incoming gradient inside the gradient launches (mask = this layer's saved output).
    FROZEN weight and bias (FusionNet's layers in the refinement loop, nerfh_nff.py:356-418): nothing else is saved or launched.
    TRAINABLE ones (FusionNet in the reference's third training stage): the input is saved too, and their gradients come from
    nefes_conv2d_wgrad (fp32 MFMA, partial sums per pixel chunk added in a fixed order -- no atomics, bit-identical from call to call)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        xc = _f32(x)
        y = _conv2d_same(xc, _pack_conv(weight, False), weight.shape[0], weight.shape[-1], None if bias is None else _f32(bias), relu)
        ctx.weight, ctx.relu, ctx.trains = weight, relu, any(ctx.needs_input_grad[1:3])
        ctx.save_for_backward(*([xc] if ctx.trains else []), *([y] if relu else []))
        if relu:
            _tap("conv_relu", y)             # tests: the ReLU branch pattern of this layer (y > 0), tests/branch.py's rule for FusionNet
        return y

    @staticmethod
    def backward(ctx, g):
        w, gf = ctx.weight, _f32(g)
        y = ctx.saved_tensors[-1] if ctx.relu else None
        gx = g_w = g_b = None
        if ctx.needs_input_grad[0]:
            gx = _conv2d_same(gf, _pack_conv(w, True), w.shape[1], w.shape[-1], None, False, mask=y)
        if ctx.trains:
            g_w, g_b = _conv2d_wgrad(ctx.saved_tensors[0], gf, y, w.shape[0], w.shape[-1], ctx.needs_input_grad[2])
            if not ctx.needs_input_grad[1]:
                g_w = None
        return gx, g_w, g_b, None


class FrozenConv2d(Conv2dSame):
    """Conv2dSame under the name its node has in the graphs of the refinement loop (FrozenConv2dBackward): what frozen_conv2d applies."""


class TrainConv2d(Conv2dSame):
    """Conv2dSame under the name its node has in the graph of a FusionNet that trains (TrainConv2dBackward): what conv2d_same_train applies."""


def frozen_conv2d(x, weight, bias, relu=False):
    if weight.requires_grad or (bias is not None and bias.requires_grad):
        raise ValueError("nefes_amd: frozen_conv2d is for weights without gradient (use torch's conv2d to train them)")
    return FrozenConv2d.apply(x, weight, bias, relu)


def conv2d_same_train(x, weight, bias, relu=False):
    """Conv2d(stride 1, "same" zero padding, 3x3 or 5x5) [+ ReLU], differentiable w.r.t. input, weight and bias (Conv2dSame)."""
    return TrainConv2d.apply(x, weight, bias, relu)


class BicubicUpsample(torch.autograd.Function):
    """torch.nn.Upsample(size=(OH, OW), mode='bicubic') on a contiguous [B,C,h,w] image (DFM_APR_refine.py:114,118), optionally
    only the window `crop` pixels inside every border (the loop's `[:, :, 10:-10, 10:-10]`, :115,119: the cropped-away pixels are
    never computed and the slice's backward -- a 39 MB fill plus a copy -- disappears); the backward is a separable gather
    instead of the library's atomic scatter."""

    @staticmethod
    def forward(ctx, x, OH, OW, crop):
        B, Cc, h, w = x.shape
        xf = _f32(x)
        CH, CW = OH - 2 * crop, OW - 2 * crop
        out = torch.empty(B, Cc, CH, CW, device=xf.device)
        with _timed("bicubic_up_fwd"):
            L.check(L.load().nefes_bicubic_up_fwd(B * Cc, h, w, OH, OW, crop, crop, CH, CW, _chk(xf, "x"), _chk(out, "out"), _stream()),
                    "nefes_bicubic_up_fwd")
        ctx.dims = (B, Cc, h, w, OH, OW, crop, CH, CW)
        return out

    @staticmethod
    def backward(ctx, g_out):
        B, Cc, h, w, OH, OW, crop, CH, CW = ctx.dims
        g = _f32(g_out)
        tmp = torch.empty(B * Cc, h, CW, device=g.device)
        g_in = torch.empty(B, Cc, h, w, device=g.device)
        with _timed("bicubic_up_bwd"):
            L.check(L.load().nefes_bicubic_up_bwd(B * Cc, h, w, OH, OW, crop, crop, CH, CW, _chk(g, "g_out"), _chk(tmp, "tmp"),
                                                  _chk(g_in, "g_in"), _stream()), "nefes_bicubic_up_bwd")
        return g_in, None, None, None


def bicubic_upsample(x, size, crop=0):
    return BicubicUpsample.apply(x, int(size[0]), int(size[1]), int(crop))


class PoseCompose(torch.autograd.Function):
    """LearnPose.forward (models/poses.py:43-50, lietorch=False) + fix_coord_supp (dm/direct_pose_model.py:224-231) in one
    launch each way: (r [n,3], t [n,3]) -> c2w [n,3,4] in NeRF coordinates.  `init_c2w` [n,4,4] on the device, no gradient."""

    @staticmethod
    def forward(ctx, r, t, init_c2w, pose_scale, move, pose_scale2, grad_into=None):
        rf, tf, i0 = _f32(r).reshape(-1, 3), _f32(t).reshape(-1, 3), _f32(init_c2w).reshape(-1, 4, 4)
        ctx.grad_into = grad_into             # (g_r, g_t) buffers the backward writes (the parameters' .grad: no copy afterwards)
        n = rf.shape[0]
        if tf.shape[0] != n or i0.shape[0] != n:
            raise ValueError("nefes_amd: pose_compose needs as many translations and initial poses as rotations")
        mv = (C.c_float * 3)(*[float(v) for v in move])
        out = torch.empty(n, 3, 4, device=rf.device)
        L.check(L.load().nefes_pose_compose_fwd(n, _chk(rf, "r"), _chk(tf, "t"), _chk(i0, "init_c2w"), float(pose_scale), mv,
                                                float(pose_scale2), _chk(out, "c2w"), _stream()), "nefes_pose_compose_fwd")
        ctx.save_for_backward(rf, tf, i0)
        ctx.consts = (float(pose_scale), mv, float(pose_scale2), r.shape, t.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        rf, tf, i0 = ctx.saved_tensors
        sc, mv, sc2, r_shape, t_shape = ctx.consts
        gf = _f32(g)
        if ctx.grad_into is not None:
            g_r, g_t = (b.reshape(rf.shape) for b in ctx.grad_into)
        else:
            g_r, g_t = torch.empty_like(rf), torch.empty_like(tf)
        L.check(L.load().nefes_pose_compose_bwd(rf.shape[0], _chk(rf, "r"), _chk(tf, "t"), _chk(i0, "init_c2w"), sc, mv, sc2,
                                                _chk(gf, "g_c2w"), _chk(g_r, "g_r"), _chk(g_t, "g_t"), _stream()),
                "nefes_pose_compose_bwd")
        return g_r.reshape(r_shape), g_t.reshape(t_shape), None, None, None, None, None


def pose_compose(r, t, init_c2w, pose_scale=1.0, move=(0., 0., 0.), pose_scale2=1.0, grad_into=None):
    """[n,3,4] for n cameras; [3,4] when r is a single 3-vector.  grad_into = (g_r, g_t): buffers the backward writes."""
    out = PoseCompose.apply(r, t, init_c2w, pose_scale, move, pose_scale2, grad_into)
    return out[0] if r.dim() == 1 else out


def _bn_train_fwd(xf, w, b, bn, per_image, track_stats):
    """The forward launch of both BatchNorm Functions on xf [B,C,H,W] with the affine parameters w, b (or None) -> (y, save: the float64
    statistics the backward reads, one set per image with per_image).  Updates bn's running statistics and batch counter as the
    module does, unless track_stats is off or the statistics are every image's own."""
    B, Cc = xf.shape[0], xf.shape[1]
    y = torch.empty_like(xf)
    groups = B if per_image else 1
    save = torch.empty(groups * Cc * 2, dtype=torch.float64, device=xf.device)
    track = bool(track_stats) and (not per_image) and bn.track_running_stats and bn.running_mean is not None
    momentum = 0.1
    if track:
        if bn.momentum is None:
            raise NotImplementedError("nefes_amd: BatchNorm with momentum=None (cumulative average) takes the torch module")
        momentum = float(bn.momentum)
    L.check(L.load().nefes_bn_train_fwd(B, Cc, xf.numel() // (B * Cc), 1 if per_image else 0, _chk(xf, "x"), _chk(w, "weight"), _chk(b, "bias"),
                                        float(bn.eps), momentum,
                                        _chk(bn.running_mean, "running_mean") if track else None, _chk(bn.running_var, "running_var") if track else None,
                                        _chk(bn.num_batches_tracked, "num_batches_tracked", torch.int64) if track and bn.num_batches_tracked is not None else None,
                                        _chk(y, "y"), _chk(save, "save", torch.float64), _stream()), "nefes_bn_train_fwd")
    return y, save


class BatchNormTrainFrozen(torch.autograd.Function):
    """torch.nn.BatchNorm2d in TRAIN mode with frozen affine parameters on [B,C,H,W] (FusionNet's last layer in the refinement loop,
    nerfh_nff.py:356-418): output normalised by the batch's statistics (running statistics and the batch counter updated as the module
    does), or by every image's own (`per_image`: torch's instance_norm with the BatchNorm's affine parameters, what the reference's
    one-image-at-a-time loop computes; running statistics untouched).  csrc/refine.hip bn_train_*: float64 sums, gradient to x only."""

    @staticmethod
    def forward(ctx, x, bn, per_image, track_stats=True):
        xf = _f32(x)
        w = None if bn.weight is None else _f32(bn.weight)
        b = None if bn.bias is None else _f32(bn.bias)
        y, save = _bn_train_fwd(xf, w, b, bn, per_image, track_stats)
        ctx.save_for_backward(xf, save)
        ctx.w, ctx.per_image = w, bool(per_image)
        return y

    @staticmethod
    def backward(ctx, g):
        xf, save = ctx.saved_tensors
        gf = _f32(g)
        B, Cc = xf.shape[0], xf.shape[1]
        g_x = torch.empty_like(xf)
        L.check(L.load().nefes_bn_train_bwd(B, Cc, xf.numel() // (B * Cc), 1 if ctx.per_image else 0, _chk(xf, "x"), _chk(ctx.w, "weight"),
                                            _chk(save, "save", torch.float64), _chk(gf, "g_y"), _chk(g_x, "g_x"), _stream()), "nefes_bn_train_bwd")
        return g_x, None, None, None


def batch_norm_train_frozen(x, bn, per_image=False, track_stats=True):
    """bn(x) for a torch.nn.BatchNorm2d in train mode whose weight and bias carry no gradient (see BatchNormTrainFrozen).
    track_stats=False: the module's running statistics and batch counter are left alone (the outputs do not depend on them in train
    mode): what a caller passes whose launches run on several streams at once over ONE shared module -- the update is a plain
    read-modify-write of the module's buffers (nefes_amd.refine.refine_concurrently)."""
    if not bn.training or any(p is not None and p.requires_grad for p in (bn.weight, bn.bias)):
        raise ValueError("nefes_amd: batch_norm_train_frozen is for a BatchNorm in train mode with frozen affine parameters")
    return BatchNormTrainFrozen.apply(x, bn, bool(per_image), bool(track_stats))


class BatchNormTrain(torch.autograd.Function):
    """BatchNormTrainFrozen for TRAINABLE affine parameters, statistics over the whole batch: the same forward (running statistics,
    momentum, batch counter), and a backward that also returns the gradients of bn.weight and bn.bias (nefes_bn_train_bwd_affine: the
    two float64 sums the input gradient is made of)."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, track_stats):
        xf, w = _f32(x), _f32(weight)
        y, save = _bn_train_fwd(xf, w, _f32(bias), bn, False, track_stats)
        ctx.save_for_backward(xf, save, w)
        return y

    @staticmethod
    def backward(ctx, g):
        xf, save, w = ctx.saved_tensors
        gf = _f32(g)
        B, Cc = xf.shape[0], xf.shape[1]
        g_x = torch.empty_like(xf) if ctx.needs_input_grad[0] else None
        g_w, g_b = torch.empty_like(w), torch.empty_like(w)
        L.check(L.load().nefes_bn_train_bwd_affine(B, Cc, xf.numel() // (B * Cc), _chk(xf, "x"), _chk(w, "weight"), _chk(save, "save", torch.float64),
                                                   _chk(gf, "g_y"), _chk(g_x, "g_x"), _chk(g_w, "g_weight"), _chk(g_b, "g_bias"), _stream()),
                "nefes_bn_train_bwd_affine")
        return g_x, g_w if ctx.needs_input_grad[1] else None, g_b if ctx.needs_input_grad[2] else None, None, None


def batch_norm_train(x, bn, track_stats=True):
    """bn(x) for a torch.nn.BatchNorm2d in train mode with affine parameters, differentiable w.r.t. x, bn.weight and bn.bias
    (BatchNormTrain; batch statistics over all images).  track_stats as in batch_norm_train_frozen."""
    if not bn.training or bn.weight is None or bn.bias is None:
        raise ValueError("nefes_amd: batch_norm_train is for a BatchNorm in train mode with affine parameters")
    return BatchNormTrain.apply(x, bn.weight, bn.bias, bn, bool(track_stats))


class SvdReg(torch.autograd.Function):
    """svd_reg (dm/DFM_pose_refine.py:119-129) on [..., 3, 4] poses: rotation block -> U V^T, one launch each way (csrc/refine.hip
    svd_reg_*; float64 inside; the backward is the polar factor's derivative, not autograd through an SVD)."""

    @staticmethod
    def forward(ctx, pose):
        pf = _f32(pose).reshape(-1, 3, 4)
        n = pf.shape[0]
        out = torch.empty_like(pf)
        save = torch.empty(n, 21, dtype=torch.float64, device=pf.device)
        L.check(L.load().nefes_svd_reg_fwd(n, _chk(pf, "pose"), _chk(out, "out"), _chk(save, "save", torch.float64), _stream()), "nefes_svd_reg_fwd")
        ctx.save_for_backward(save)
        ctx.shape = pose.shape
        return out.reshape(pose.shape)

    @staticmethod
    def backward(ctx, g):
        (save,) = ctx.saved_tensors
        gf = _f32(g).reshape(-1, 3, 4)
        g_pose = torch.empty_like(gf)
        L.check(L.load().nefes_svd_reg_bwd(gf.shape[0], _chk(save, "save", torch.float64), _chk(gf, "g_out"), _chk(g_pose, "g_pose"), _stream()),
                "nefes_svd_reg_bwd")
        return g_pose.reshape(ctx.shape)


def svd_reg(pose):
    """[..., 3, 4] poses with the 3x3 block replaced by its nearest orthogonal matrix U V^T (include/nefes_hip.h nefes_svd_reg_fwd)."""
    return SvdReg.apply(pose)


class RegressedPose(torch.autograd.Function):
    """svd_reg (optional) + fix_coord_supp on [..., 3, 4] regressed poses, one launch each way (include/nefes_hip.h
    nefes_regressed_pose_fwd): what train_on_batch does to the regression network's output before it renders (DFM_APR_refine.py:91-97)."""

    @staticmethod
    def forward(ctx, pose, do_svd, t_scale, move):
        pf = _f32(pose).reshape(-1, 3, 4)
        n = pf.shape[0]
        out = torch.empty_like(pf)
        save = torch.empty(n, 21, dtype=torch.float64, device=pf.device) if do_svd else None
        L.check(L.load().nefes_regressed_pose_fwd(n, _chk(pf, "pose"), 1 if do_svd else 0, float(t_scale), float(move[0]), float(move[1]), float(move[2]),
                                                  _chk(out, "out"), _chk(save, "save", torch.float64), _stream()), "nefes_regressed_pose_fwd")
        if do_svd:
            ctx.save_for_backward(save)
        ctx.shape, ctx.do_svd, ctx.t_scale = pose.shape, bool(do_svd), float(t_scale)
        return out.reshape(pose.shape)

    @staticmethod
    def backward(ctx, g):
        save = ctx.saved_tensors[0] if ctx.do_svd else None
        gf = _f32(g).reshape(-1, 3, 4)
        g_pose = torch.empty_like(gf)
        L.check(L.load().nefes_regressed_pose_bwd(gf.shape[0], _chk(save, "save", torch.float64), 1 if ctx.do_svd else 0, ctx.t_scale,
                                                  _chk(gf, "g_out"), _chk(g_pose, "g_pose"), _stream()), "nefes_regressed_pose_bwd")
        return g_pose.reshape(ctx.shape), None, None, None


def regressed_pose(pose, do_svd, world_setup=None):
    """[..., 3, 4] regressed poses -> svd_reg (if do_svd) -> fix_coord_supp(world_setup) (identity translation map when None)."""
    if world_setup is None:
        sc, mv = 1.0, (0., 0., 0.)
    else:
        s1, s2 = float(world_setup["pose_scale"]), float(world_setup["pose_scale2"])
        sc, mv = s1 * s2, tuple(float(v) * s2 for v in world_setup["move_all_cam_vec"])
    return RegressedPose.apply(pose, bool(do_svd), sc, mv)


def _loss_buffer(out, device):
    """Where a feature-loss Function's forward kernel writes its value: the caller's `out=` (PoseRefiner passes its static loss buffer, so
    that an iteration needs no separate 4-byte copy kernel to leave the value there) or, with None, a fresh tensor."""
    if out is None:
        return torch.empty((), device=device)
    wrong = ("is not a tensor" if not torch.is_tensor(out) else f"is {out.dim()}-d" if out.dim() != 0
             else f"is {out.dtype}" if out.dtype != torch.float32
             else f"is on {out.device}, the inputs on {device}" if out.device != torch.device(device)
             else "requires grad" if out.requires_grad else None)
    if wrong:
        raise ValueError(f"nefes_amd: the loss's `out` must be a 0-d float32 tensor on the inputs' device that does not require grad: this one {wrong}")
    return out.detach()            # (a new tensor object on the same storage: autograd attaches this call's history to it, not to the buffer)


def _groups_of(planes, groups, what):
    G = int(groups)
    if G < 1 or planes % G:
        raise ValueError(f"nefes_amd: {what}: {planes} leading channels do not split into {groups} groups")
    return G


def _loss_mask(mask, G, spatial, device, what):
    """The validity mask of a feature loss as the kernels read it: uint8 [G, pixels] on the inputs' device, contiguous -- one byte per
    pixel and group (image), shared by the group's channels; valid iff != 0.  Checked BEFORE anything is launched; nothing is converted
    or copied here (PoseRefiner thresholds an image's mask once, into its own buffer)."""
    spatial = tuple(int(v) for v in spatial)
    P = 1
    for v in spatial:
        P *= v
    ok_shapes = {(G,) + spatial, (G, P), (G, 1) + spatial} | ({spatial, (P,)} if G == 1 else set())
    wrong = ("is not a tensor" if not torch.is_tensor(mask)
             else f"is on {mask.device}, the inputs on {device}" if mask.device != torch.device(device)
             else f"is {mask.dtype} (one uint8 per pixel: threshold it once, e.g. (m > 0).to(torch.uint8))" if mask.dtype != torch.uint8
             else f"has shape {tuple(mask.shape)}, not {(G,) + spatial} (one plane per group, shared by its channels)"
             if tuple(mask.shape) not in ok_shapes
             else "is not contiguous" if not mask.is_contiguous() else None)
    if wrong:
        raise ValueError(f"nefes_amd: {what}: the mask {wrong}")
    return mask.detach().reshape(G, P)


# One of the four feature losses (csrc/feature_loss.hip), unmasked or masked, as FeatureLoss reads it: the public function's name, on
# the up-sampled map?, per pixel?, its entry points and scratch query, its ops.TIMERS keys.
_LossForm = collections.namedtuple("_LossForm", "what up per_pixel fwd bwd query timer_fwd timer_bwd")


def _loss_form(stem, what, up, per_pixel, masked):
    m = "_masked" if masked else ""
    keyed = masked or stem != "cosine"                    # (the unmasked channel-wise pair has never had a TIMERS key)
    return _LossForm(what, up, per_pixel, f"nefes_{stem}_loss{m}_fwd", f"nefes_{stem}_loss{m}_bwd",
                     f"nefes_{stem}{m}_scratch_doubles" if per_pixel else "nefes_cosine_loss_scratch_doubles",
                     f"{stem}_loss{m}_fwd" if keyed else None, f"{stem}_loss{m}_bwd" if keyed else None)


_LOSS_FORMS = {(stem, masked): _loss_form(stem, what, up, per_pixel, masked) for masked in (False, True)
               for stem, what, up, per_pixel in (("cosine", "cosine_feature_loss", False, False), ("upcos", "upsampled_cosine_loss", True, False),
                                                 ("pixcos", "pixel_cosine_loss", False, True),
                                                 ("uppixcos", "upsampled_pixel_cosine_loss", True, True))}


def _loss_outputs(ctx, loss, scratch, per_pixel, G, GC):
    """(loss, cos) as a feature-loss Function returns them.  `cos`: the float64 cosines the forward kernel left at the head of its
    scratch (a view, no gradient) -- per channel [GC], column 3 of the stats [GC][4], or per pixel the mean per group [G]."""
    cos = scratch[:G] if per_pixel else scratch[3:4 * GC:4]
    ctx.set_materialize_grads(False)                      # no zero-filled gradient for `cos` in the backward
    ctx.mark_non_differentiable(cos)
    return loss, cos


def _loss_maps(form, af, bf, mk, scratch):
    """What every entry point of a form takes after its sizes: the two maps, the mask if there is one, the scratch -- checked."""
    maps = (_chk(af, "x"), _chk(bf, "target")) if form.up else (_chk(af, "a"), _chk(bf, "b"))
    if mk is not None:
        maps += (_chk(mk, "mask", torch.uint8),)
    return maps + (_chk(scratch, "scratch", torch.float64),)


class FeatureLoss(torch.autograd.Function):
    """The feature loss of the reference's refinement loop in one of its forms (`form`: a row of _LOSS_FORMS):
    feature_loss / masked_feature_loss (dm/DFM_pose_refine.py:211-233, :257-288) on maps a, b [G*C, ...pixels] -- per group (image)
    1 - mean over its channels of the cosine similarity over its (valid) pixels, or per pixel 1 - mean over its (valid) pixels of the
    cosine similarity over its channels, summed over the G groups -- and the same of the bicubically up-sampled, cropped a [G*C, h, w]
    (or [1, ., h, w]) against b [G*C, OH-2crop, OW-2crop] without the up-sampled image (`geom` = (OH, OW, crop); None: not up-sampled).
    `mask`: uint8, one plane per group (_loss_mask); None: the unmasked entry points -- the channel-wise ones take all G*C channels as
    ONE group (1 - their mean: the caller multiplies by G).  Two launches forward, one (up-sampled: two) backward, to `a` only: the
    target carries no gradient.  Returns (loss, cos) (_loss_outputs).  Every check runs before anything is launched."""

    @staticmethod
    def forward(ctx, how, a, b, mask, out):
        form, geom, groups = how
        GC = a.shape[-3] if form.up else a.shape[0]
        G = _groups_of(GC, groups, form.what)
        one_group = mask is None and not form.per_pixel
        if one_group and G > 1 and out is not None:
            raise ValueError(f"nefes_amd: {form.what}: `out` takes the kernel's own value; with groups > 1 and no mask the sum over the "
                             "groups is formed after it")
        af = _f32(a)
        if form.up:
            h, w = af.shape[-2:]
            if af.numel() != GC * h * w:
                raise ValueError(f"nefes_amd: {form.what}: features {tuple(a.shape)} are not [C,h,w] (or [1,C,h,w]) maps")
            OH, OW, crop = geom
            spatial = (OH - 2 * crop, OW - 2 * crop)
            af, bf = af.reshape(GC, h, w), _f32(b).reshape((GC,) + spatial)
            sizes = (h, w, OH, OW, crop)
        else:
            af, bf = af.reshape(GC, -1), _f32(b).reshape(GC, -1)
            if af.shape != bf.shape:
                raise ValueError(f"nefes_amd: {form.what}: feature maps of different shapes: {tuple(a.shape)} vs {tuple(b.shape)}")
            spatial, sizes = a.shape[1:], (af.shape[1],)
        mk = None if mask is None else _loss_mask(mask, G, spatial, af.device, form.what)
        loss = _loss_buffer(out, af.device)
        lib = L.load()
        doubles = getattr(lib, form.query)(G, *(geom if form.up else sizes)) if form.per_pixel else lib.nefes_cosine_loss_scratch_doubles(GC)
        scratch = torch.empty(doubles, dtype=torch.float64, device=af.device)
        sizes = ((GC,) if one_group else (G, GC // G)) + sizes
        with _timed(form.timer_fwd):
            L.check(getattr(lib, form.fwd)(*sizes, *_loss_maps(form, af, bf, mk, scratch), _chk(loss, "loss"), _stream()), form.fwd)
        ctx.save_for_backward(af, bf, mk, scratch)
        ctx.cfg = (form, a.shape, sizes)
        return _loss_outputs(ctx, loss, scratch, form.per_pixel, G, GC)

    @staticmethod
    def backward(ctx, g, _g_cos):
        if g is None:
            return (None,) * 5
        af, bf, mk, scratch = ctx.saved_tensors
        form, shape, sizes = ctx.cfg
        gf = _f32(g).reshape(1)
        if form.up:                                         # the row gradients are gathered along x into tmp, then along y into g_a
            h, w, OH, OW, crop = sizes[-5:]
            tmp = torch.empty(af.shape[0], OH - 2 * crop, w, device=af.device)
            (fx, cx, wx, T), (fy, cy, wy, _) = bicubic_gather_tables(h, w, OH, OW, crop, af.device)
        g_a = torch.empty_like(af)
        with _timed(form.timer_bwd):
            tables = (fx.data_ptr(), cx.data_ptr(), wx.data_ptr(), fy.data_ptr(), cy.data_ptr(), wy.data_ptr(), T, _chk(tmp, "tmp")) if form.up else ()
            L.check(getattr(L.load(), form.bwd)(*sizes, *_loss_maps(form, af, bf, mk, scratch), _chk(gf, "g_loss"), *tables, _chk(g_a, "g_a"),
                                                _stream()), form.bwd)
        return None, g_a.reshape(shape), None, None, None


def _feature_loss(stem, a, b, geom, groups, mask, out, return_cos):
    form = _LOSS_FORMS[stem, mask is not None]
    loss, cos = FeatureLoss.apply((form, geom, groups), a, b, mask, out)
    if mask is None and not form.per_pixel and int(groups) > 1:
        loss = loss * float(int(groups))
    return (loss, cos) if return_cos else loss


def cosine_feature_loss(a, b, return_cos=False, out=None, groups=1, mask=None):
    """1 - mean over the leading (channel) dimension of the cosine similarity over everything else; `return_cos` adds the
    per-channel similarities (float64, no gradient) -- per-image losses of a batch folded into the channel dimension.
    `out`: a 0-d float32 tensor on the inputs' device that does not require grad; the forward kernel writes the value there and the
    returned loss shares its storage (None: a fresh tensor).
    `groups` = G > 1: the leading dimension is G groups (images) of C channels and the value is the SUM over the groups of each one's
    loss.  `mask`: uint8 [G, ...pixels] on the inputs' device, one plane per group shared by its channels -- the sums of every channel
    run over the pixels with mask != 0 only (the reference's masked_feature_loss); values at the others are never read and their
    gradient is exactly 0.  None: the unmasked kernels (G > 1: their mean over all G*C channels times G -- the same number; no `out`)."""
    return _feature_loss("cosine", a, b, None, groups, mask, out, return_cos)


def upsampled_cosine_loss(x, target, size, crop=0, return_cos=False, out=None, groups=1, mask=None):
    """1 - mean over channels of the cosine similarity (over pixels) between the bicubically up-sampled, cropped x and target.
    `out`, `groups` and `mask` (uint8 [groups, OH-2crop, OW-2crop]: of the up-sampled, cropped pixels) as in cosine_feature_loss.
    One-pass kernels; a masked loss has no prepared-target (Gram) form: sum_p m_p up_p^2 does not separate into the two axes."""
    return _feature_loss("upcos", x, target, (int(size[0]), int(size[1]), int(crop)), groups, mask, out, return_cos)


def pixel_cosine_loss(a, b, groups=1, return_cos=False, out=None, mask=None):
    """The per-pixel feature loss (`--per_pixel`): a, b [groups * C, ...]; per group 1 - mean over pixels of the cosine similarity over
    its C channels (torch.nn.CosineSimilarity(dim=0, eps=1e-6)), summed over the groups -- every group's value and gradient are what a
    call on that group alone gives.  `return_cos` adds the per-group mean cosines (float64, no gradient); `out` as in
    cosine_feature_loss.  `mask`: uint8 [groups, ...pixels]; the mean is over the group's pixels with mask != 0 (values at the others are
    never read, their gradient is exactly 0; a group without one gives NaN, as the reference's mean of an empty tensor); None: the
    unmasked kernels."""
    return _feature_loss("pixcos", a, b, None, groups, mask, out, return_cos)


def upsampled_pixel_cosine_loss(x, target, size, crop=0, groups=1, return_cos=False, out=None, mask=None):
    """pixel_cosine_loss of the bicubically up-sampled, cropped x against target, one pass each way.  `out` as in cosine_feature_loss;
    `mask` (uint8 [groups, OH-2crop, OW-2crop]: of the up-sampled, cropped pixels) as in pixel_cosine_loss.  There is no prepared-target
    form of this loss: the normalisation is per pixel."""
    return _feature_loss("uppixcos", x, target, (int(size[0]), int(size[1]), int(crop)), groups, mask, out, return_cos)


class DepthLoss(torch.autograd.Function):
    """depth_loss below as one autograd node: one launch forward (nefes_depth_loss_fwd), one backward (nefes_depth_loss_bwd), to
    `disp` only.  Returns (loss, per_group): per_group the float64 values L_g [G] at the head of the kernel's scratch (weight not
    applied; a view, no gradient).  Every check runs before anything is launched."""

    @staticmethod
    def forward(ctx, disp, target, mask, cfg, out):
        delta, weight, accumulate = cfg
        df = _f32(disp)
        if df.dim() == 0 or df.numel() == 0:
            raise ValueError(f"nefes_amd: depth_loss: `disp` must be [P] or [G, ...pixels]; got {tuple(disp.shape)}")
        G = 1 if df.dim() == 1 else int(df.shape[0])
        df = df.reshape(G, -1)
        P = int(df.shape[1])
        if not torch.is_tensor(target) or target.numel() != G * P or target.dtype != torch.float32:
            raise ValueError(f"nefes_amd: depth_loss: `target` must be a float32 tensor of disp's {G * P} elements ({tuple(disp.shape)}); got "
                             + (f"{target.dtype} {tuple(target.shape)}" if torch.is_tensor(target) else type(target).__name__))
        tf = target.detach().reshape(G, P)
        mk = None if mask is None else _loss_mask(mask, G, disp.shape[1:] if disp.dim() > 1 else disp.shape, df.device, "depth_loss")
        if accumulate and out is None:
            raise ValueError("nefes_amd: depth_loss(accumulate=True) adds the term to the value it finds in `out`: pass out=")
        loss = _loss_buffer(out, df.device)
        lib = L.load()
        scratch = torch.empty(lib.nefes_depth_loss_scratch_doubles(G), dtype=torch.float64, device=df.device)
        with _timed("depth_loss_fwd"):
            L.check(lib.nefes_depth_loss_fwd(G, P, _chk(df, "disp"), _chk(tf, "target"), _chk(mk, "mask", torch.uint8), delta, weight,
                                             int(accumulate), _chk(scratch, "scratch", torch.float64), _chk(loss, "loss"), _stream()),
                    "nefes_depth_loss_fwd")
        ctx.save_for_backward(df, tf, mk, scratch)
        ctx.cfg = (G, P, delta, weight, disp.shape)
        per_group = scratch[:G]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(per_group)
        return loss, per_group

    @staticmethod
    def backward(ctx, g, _g_groups):
        if g is None:
            return (None,) * 5
        df, tf, mk, scratch = ctx.saved_tensors
        G, P, delta, weight, shape = ctx.cfg
        gf = _f32(g).reshape(1)
        g_disp = torch.empty_like(df)
        with _timed("depth_loss_bwd"):
            L.check(L.load().nefes_depth_loss_bwd(G, P, _chk(df, "disp"), _chk(tf, "target"), _chk(mk, "mask", torch.uint8), delta, weight,
                                                  _chk(scratch, "scratch", torch.float64), _chk(gf, "g_loss"), _chk(g_disp, "g_disp"),
                                                  _stream()), "nefes_depth_loss_bwd")
        return g_disp.reshape(shape), None, None, None, None


def depth_loss(disp, target, mask=None, delta=0.1, weight=1.0, out=None, accumulate=False, return_groups=False):
    """A Huber loss between NORMALISED rendered depth and a measured depth map (csrc/depth_loss.hip).  disp [P] or [G, ...pixels]: a
    render's disp_map -- 1 / disp is depth / (sum of the weights the variant normalises by), z-depth in the scene's units; target: float32,
    the same number of elements, in those units; mask: uint8 [G, ...pixels] or None.  A pixel is valid iff target is finite and > 0 (sensor
    holes are 0, Inf or NaN), disp is finite and > 0, and its mask byte is != 0: a select -- an invalid pixel's values are never combined
    and its gradient is exactly 0.  e = 1 / disp - target; rho = e^2 / (2 delta) for |e| <= delta, |e| - delta / 2 beyond
    (torch.nn.SmoothL1Loss(beta=delta)); per group the mean of rho over its valid pixels (0 when it has none); the value is
    weight * their sum over the groups.  Arithmetic in double, one rounding to float32.
    `out` as in cosine_feature_loss; `accumulate=True`: the value written is what `out` held plus the term, rounded once -- so a total
    of several losses lands in one buffer without an add of its own (differentiate the losses together:
    torch.autograd.grad([feature, total], ...)).  `return_groups` adds the per-group values L_g [G] (float64, weight not applied, no
    gradient).  The gradient goes to `disp`; the target carries none."""
    delta, weight = float(delta), float(weight)
    if not (delta > 0 and delta != float("inf")):
        raise ValueError(f"nefes_amd: depth_loss: delta = {delta!r} must be positive and finite (the Huber threshold, in the scene's units)")
    if weight != weight or weight in (float("inf"), float("-inf")):
        raise ValueError(f"nefes_amd: depth_loss: weight = {weight!r} must be finite")
    loss, groups = DepthLoss.apply(disp, target, mask, (delta, weight, bool(accumulate)), out)
    return (loss, groups) if return_groups else loss


def psnr_ssim(x, y):
    """The verification step's two numbers (DFM_APR_refine.py:117-128, :146-150) of two [C,H,W] fp32 images on the GPU:
    (mse2psnr(img2mse(x, y)), SSIM()(x, y).mean()) as 0-d tensors -- two launches (csrc/refine.hip psnr_ssim_*) where the torch
    expressions take ~25.  Rows must be dense (stride 1 along W); row and plane strides are free, so a cropped view is not copied."""
    for name, t in (("x", x), ("y", y)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1):
            raise RuntimeError(f"nefes_amd: psnr_ssim: `{name}` must be a [C,H,W] float32 GPU tensor with dense rows (got {tuple(t.shape)}, "
                               f"strides {t.stride()}, {t.dtype}, {t.device})")
    if x.shape != y.shape:
        raise RuntimeError(f"nefes_amd: psnr_ssim: shapes differ ({tuple(x.shape)} vs {tuple(y.shape)})")
    lib = L.load()
    Cc, H, W = (int(v) for v in x.shape)
    ws = torch.empty(lib.nefes_psnr_ssim_workspace(Cc, H, W), dtype=torch.uint8, device=x.device)
    out = torch.empty(2, device=x.device)
    x, y = x.detach(), y.detach()
    L.check(lib.nefes_psnr_ssim(Cc, H, W, C.c_void_p(x.data_ptr()), x.stride(1), x.stride(0), C.c_void_p(y.data_ptr()), y.stride(1),
                                y.stride(0), _chk(ws, "workspace", torch.uint8), _chk(out, "out"), _stream()), "nefes_psnr_ssim")
    return out[0], out[1]


_GATHER_TABLES = {}


def _gather_T(n_in, n_out):
    return 4 * ((n_out + n_in - 1) // n_in) + 8


def bicubic_gather_table(n_in, n_out, o0, n_win, device, T=None):
    """(first, count, wt, T) of one axis (include/nefes_hip.h nefes_bicubic_gather_table), built once per geometry and device.  T: row
    length of `wt` (default: what this axis needs; the kernels that take the tables of BOTH axes take one T: `bicubic_gather_tables`)."""
    T = _gather_T(n_in, n_out) if T is None else int(T)
    key = (int(n_in), int(n_out), int(o0), int(n_win), T, str(device))
    t = _GATHER_TABLES.get(key)
    if t is None:
        first = torch.zeros(n_in, dtype=torch.int32, device=device)
        count = torch.zeros(n_in, dtype=torch.int32, device=device)
        wt = torch.zeros(n_in, T, device=device)
        L.check(L.load().nefes_bicubic_gather_table(n_in, n_out, o0, n_win, T, first.data_ptr(), count.data_ptr(), wt.data_ptr(), _stream()),
                "nefes_bicubic_gather_table")
        t = _GATHER_TABLES[key] = (first, count, wt, T)
    return t


def bicubic_gather_tables(h, w, OH, OW, crop, device):
    """The x and y tables with ONE row length (nefes_upcos_loss_bwd / nefes_upcos_prepare take a single T): until round 5 the y table was
    built with its own T and read with the x table's -- the same number for the loop's integer scale, not for OH / h != OW / w."""
    T = max(_gather_T(w, OW), _gather_T(h, OH))
    return (bicubic_gather_table(w, OW, crop, OW - 2 * crop, device, T), bicubic_gather_table(h, OH, crop, OH - 2 * crop, device, T))


_GRAMS = {}


def bicubic_gram(n_in, n_out, o0, n_win, device):
    """(G [n_in, n_in] float64, half band width) of one axis' window (include/nefes_hip.h nefes_bicubic_gram), once per geometry."""
    key = (int(n_in), int(n_out), int(o0), int(n_win), str(device))
    t = _GRAMS.get(key)
    if t is None:
        G = torch.zeros(n_in, n_in, dtype=torch.float64, device=device)
        L.check(L.load().nefes_bicubic_gram(n_in, n_out, o0, n_win, G.data_ptr(), _stream()), "nefes_bicubic_gram")
        nz = G.nonzero()
        band = int((nz[:, 0] - nz[:, 1]).abs().max()) if nz.numel() else 0
        t = _GRAMS[key] = (G, band)
    return t


UPCOS_GRAM_LDS_MAX = 96 * 1024          # csrc/feature_loss.hip NEFES_UPCOS_GRAM_LDS_MAX


class UpcosTarget:
    """What upsampled_cosine_loss needs of a FIXED target [C, OH-2crop, OW-2crop] (the refinement loop's: one target for all
    iterations of an image): Tt = Uy^T target Ux [C,h,w], |target|^2 per channel, and the Gram matrices of the two axes.  `update(target)`
    refills the same buffers (a captured graph keeps reading them).  csrc/feature_loss.hip upcos_prep_* / upcos_gram_*."""

    def __init__(self, C, h, w, OH, OW, crop, device):
        self.C, self.h, self.w, self.OH, self.OW, self.crop = int(C), int(h), int(w), int(OH), int(OW), int(crop)
        CH, CW = self.OH - 2 * self.crop, self.OW - 2 * self.crop
        self.tt = torch.zeros(self.C, self.h, self.w, dtype=torch.float64, device=device)
        self.dbb = torch.zeros(self.C, dtype=torch.float64, device=device)
        self.gx, bx = bicubic_gram(self.w, self.OW, self.crop, CW, device)
        self.gy, by = bicubic_gram(self.h, self.OH, self.crop, CH, device)
        self.band = max(bx, by)
        self.tx, self.ty = bicubic_gather_tables(self.h, self.w, self.OH, self.OW, self.crop, device)
        self.device = device
        # one workgroup of the Gram-form forward holds a band of rows in LDS: geometries beyond its ceiling (h ~ 240 with w ~ 427, or
        # a wide band from a non-integer scale) stay on the one-pass kernels -- decided HERE, not by an error in the middle of a loop
        self.fits = int(L.load().nefes_upcos_gram_lds_bytes(self.h, self.w, self.band)) <= UPCOS_GRAM_LDS_MAX

    def update(self, target):
        CH, CW = self.OH - 2 * self.crop, self.OW - 2 * self.crop
        tf = _f32(target).reshape(self.C, CH, CW)
        tmp = torch.empty(self.C, CH, self.w, dtype=torch.float64, device=tf.device)
        (fx, cx, wx, T), (fy, cy, wy, _) = self.tx, self.ty
        L.check(L.load().nefes_upcos_prepare(self.C, self.h, self.w, self.OH, self.OW, self.crop, _chk(tf, "target"), fx.data_ptr(), cx.data_ptr(),
                                             wx.data_ptr(), fy.data_ptr(), cy.data_ptr(), wy.data_ptr(), T, _chk(tmp, "tmp", torch.float64),
                                             _chk(self.tt, "tt", torch.float64), _chk(self.dbb, "dbb", torch.float64), _stream()),
                "nefes_upcos_prepare")
        return self


class UpsampledCosineLossPrepared(torch.autograd.Function):
    """upsampled_cosine_loss (FeatureLoss, "upcos") against a prepared target (UpcosTarget): two small launches forward, one backward, on [C,h,w] data only."""

    @staticmethod
    def forward(ctx, x, prep, out=None):
        xf = _f32(x)
        if tuple(xf.shape[-3:]) != (prep.C, prep.h, prep.w) or xf.numel() != prep.C * prep.h * prep.w:
            raise ValueError(f"nefes_amd: features {tuple(x.shape)} do not match the prepared target ({prep.C}, {prep.h}, {prep.w})")
        xf = xf.reshape(prep.C, prep.h, prep.w)
        lib = L.load()
        scratch = torch.empty(lib.nefes_cosine_loss_scratch_doubles(prep.C), dtype=torch.float64, device=xf.device)
        pmat = torch.empty(prep.C, prep.h, prep.w, dtype=torch.float64, device=xf.device)
        loss = _loss_buffer(out, xf.device)
        with _timed("upcos_gram_fwd"):
            L.check(lib.nefes_upcos_gram_fwd(prep.C, prep.h, prep.w, _chk(xf, "x"), _chk(prep.tt, "tt", torch.float64),
                                             _chk(prep.dbb, "dbb", torch.float64), _chk(prep.gx, "gram_x", torch.float64),
                                             _chk(prep.gy, "gram_y", torch.float64), prep.band, _chk(scratch, "scratch", torch.float64),
                                             _chk(pmat, "pmat", torch.float64), _chk(loss, "loss"), _stream()), "nefes_upcos_gram_fwd")
        ctx.save_for_backward(scratch, pmat)
        ctx.prep, ctx.shape = prep, x.shape
        return _loss_outputs(ctx, loss, scratch, False, 1, prep.C)

    @staticmethod
    def backward(ctx, g, _g_cos):
        if g is None:
            return (None,) * 3
        scratch, pmat = ctx.saved_tensors
        prep = ctx.prep
        gf = _f32(g).reshape(1)
        g_x = torch.empty(prep.C, prep.h, prep.w, device=pmat.device)
        with _timed("upcos_gram_bwd"):
            L.check(L.load().nefes_upcos_gram_bwd(prep.C, prep.h, prep.w, _chk(prep.tt, "tt", torch.float64), _chk(pmat, "pmat", torch.float64),
                                                  _chk(scratch, "scratch", torch.float64), _chk(gf, "g_loss"), _chk(g_x, "g_x"), _stream()),
                    "nefes_upcos_gram_bwd")
        return g_x.reshape(ctx.shape), None, None


def upsampled_cosine_loss_prepared(x, prep, return_cos=False, out=None):
    """upsampled_cosine_loss(x, target, (OH, OW), crop) for the target `prep` (an UpcosTarget) was last updated with.  `out` as in
    cosine_feature_loss."""
    loss, cos = UpsampledCosineLossPrepared.apply(x, prep, out)
    return (loss, cos) if return_cos else loss


class FusionInput(torch.autograd.Function):
    """The rendered maps -> FusionNet's input in one launch (csrc/refine.hip fusion_input): affine colour transform with the image's
    12 exposure coefficients (or none), colour normalisation, [N,3] / [N,C] -> [B,3+C,H,W].  Gradients to rgb and feat; the
    coefficients are constants here (a trainable exposure network takes the torch path)."""

    @staticmethod
    def forward(ctx, rgb, feat, affine, B, H, W, mean, std):
        rgb, feat = _f32(rgb).reshape(-1, 3), _f32(feat)
        Cf = feat.shape[-1]
        feat = feat.reshape(-1, Cf)
        HW = int(H) * int(W)
        x = torch.empty(B, 3 + Cf, int(H), int(W), device=rgb.device)
        y = torch.empty_like(rgb) if affine is not None else None
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
        L.check(L.load().nefes_fusion_input_fwd(B, HW, Cf, _chk(rgb, "rgb"), _chk(feat, "feat"), _chk(affine, "affine"), m3, s3,
                                                _chk(x, "x"), _chk(y, "y"), _stream()), "nefes_fusion_input_fwd")
        ctx.save_for_backward(affine, y)
        ctx.cfg = (B, HW, Cf, s3)
        return x

    @staticmethod
    def backward(ctx, g_x):
        affine, y = ctx.saved_tensors
        B, HW, Cf, s3 = ctx.cfg
        g = _f32(g_x)
        g_rgb = torch.empty(B * HW, 3, device=g.device) if ctx.needs_input_grad[0] else None
        g_feat = torch.empty(B * HW, Cf, device=g.device) if ctx.needs_input_grad[1] else None
        L.check(L.load().nefes_fusion_input_bwd(B, HW, Cf, _chk(g, "g_x"), _chk(affine, "affine"), _chk(y, "y"), s3, _chk(g_rgb, "g_rgb"),
                                                _chk(g_feat, "g_feat"), _stream()), "nefes_fusion_input_bwd")
        return g_rgb, g_feat, None, None, None, None, None, None


def fusion_input(rgb, feat, affine, B, H, W, mean, std):
    return FusionInput.apply(rgb, feat, affine, int(B), int(H), int(W), tuple(mean), tuple(std))


class FusedAdam:
    """torch.optim.Adam (defaults: no weight decay, no amsgrad) over a few small fp32 parameters with a learning rate per
    parameter, as ONE launch per step (csrc/refine.hip adam_kernel): the parameters are views into one flat buffer, so are their
    .grad tensors, and the state (m, v, step) lives on the device -- capturable in a HIP graph by construction."""

    def __init__(self, params_and_lrs, betas=(0.9, 0.999), eps=1e-8):
        self.params = [p for p, _ in params_and_lrs]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, device=dev)
        self.grad = torch.zeros(n, device=dev)
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.step_t = torch.zeros(1, device=dev)
        self.lr = torch.cat([torch.full((p.numel(),), float(lr), dtype=torch.float64) for p, lr in params_and_lrs]).to(dev)
        self.betas, self.eps = betas, eps
        off = 0
        with torch.no_grad():
            for p in self.params:                     # re-home each parameter (and its gradient) as a view of the flat buffers
                k = p.numel()
                self.flat[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat[off:off + k].view(p.shape)
                p.grad = self.grad[off:off + k].view(p.shape)
                off += k

    def zero_state(self):
        self.m.zero_(); self.v.zero_(); self.step_t.zero_(); self.grad.zero_()

    def step(self):
        L.check(L.load().nefes_adam_step(self.flat.numel(), self.flat.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                         self.step_t.data_ptr(), self.lr.data_ptr(), float(self.betas[0]), float(self.betas[1]),
                                         float(self.eps), _stream()), "nefes_adam_step")


# ---------------------------------------------------------------------------------------------
# the training step's losses (script/models/losses.py; csrc/losses.hip)
# ---------------------------------------------------------------------------------------------
def _loss_in(t, name, shape):
    """A loss input as the kernels read it: float32 on the GPU (anything else raises -- no CPU path, no silent cast), made contiguous."""
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"nefes_amd: train loss: `{name}` must be a float32 GPU tensor (got {getattr(t, 'dtype', type(t))}, "
                           f"{getattr(t, 'device', None)}); there is no CPU path")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"nefes_amd: train loss: `{name}` must be {tuple(shape)} (got {tuple(t.shape)})")
    return _f32(t)


class TrainLoss(torch.autograd.Function):
    """The five loss classes of script/models/losses.py as two launches forward and one backward (csrc/losses.hip).

    apply(rgb_fine, rgb_coarse, rgb_target, beta, transient_sigmas, feat_fine, feat_coarse, feat_fusion, feat_target, nerfw, feat_kind,
          coef, lambda_u) -> (colour loss, loss_f, loss_fusion, terms[8])
    A tensor that is None is absent.  `transient_sigmas` [N,S] is read in place through its row stride (render()'s raw[:, ch, :] view);
    its gradient is one number on the device, returned as a stride-0 [N,S] view.  `terms` carries no gradient."""

    @staticmethod
    def forward(ctx, rgb_fine, rgb_coarse, rgb_target, beta, sigmas, feat_fine, feat_coarse, feat_fusion, feat_target, nerfw, feat_kind,
                coef, lambda_u):
        if rgb_target is None:
            raise RuntimeError("nefes_amd: train loss: `rgb_target` is required")
        N = int(rgb_target.shape[0])
        rgb_target = _loss_in(rgb_target, "rgb_target", (N, 3))
        rgb_fine, rgb_coarse = _loss_in(rgb_fine, "rgb_fine", (N, 3)), _loss_in(rgb_coarse, "rgb_coarse", (N, 3))
        Cc = int(feat_target.shape[-1]) if feat_target is not None else 0
        feat_target = _loss_in(feat_target, "feat_target", (N, Cc))
        feat_fine, feat_coarse = _loss_in(feat_fine, "feat_fine", (N, Cc)), _loss_in(feat_coarse, "feat_coarse", (N, Cc))
        feat_fusion = _loss_in(feat_fusion, "feat_fusion", (N, Cc))
        beta = _loss_in(beta, "beta", (N,))
        S, stride = 0, 0
        if beta is not None:
            if sigmas is None or sigmas.dim() != 2 or sigmas.shape[0] != N:
                raise RuntimeError("nefes_amd: train loss: `beta` needs `transient_sigmas` [N,S]")
            S = int(sigmas.shape[1])
            if not (sigmas.is_cuda and sigmas.dtype == torch.float32):
                raise RuntimeError(f"nefes_amd: train loss: `transient_sigmas` must be a float32 GPU tensor (got {sigmas.dtype}, {sigmas.device})")
            sigmas = sigmas.detach()
            if not ((sigmas.stride(1) == 1 or S == 1) and sigmas.stride(0) >= S):
                sigmas = sigmas.contiguous()                                # (any other layout; render()'s view is read in place)
            stride = int(sigmas.stride(0))
        else:
            sigmas = None
        present = ((L.LOSS_HAS_RGB_FINE if rgb_fine is not None else 0) | (L.LOSS_HAS_RGB_COARSE if rgb_coarse is not None else 0)
                   | (L.LOSS_HAS_BETA if beta is not None else 0) | (L.LOSS_HAS_FEAT_FINE if feat_fine is not None else 0)
                   | (L.LOSS_HAS_FEAT_COARSE if feat_coarse is not None else 0) | (L.LOSS_HAS_FEAT_FUSION if feat_fusion is not None else 0)
                   | (L.LOSS_NERFW if nerfw else 0))
        desc = L.NefesTrainLossDesc(N, Cc, S, int(feat_kind), present, float(coef), float(lambda_u), stride)
        lib = L.load()
        dev = rgb_target.device
        scratch = torch.empty(lib.nefes_train_loss_scratch_doubles(N), dtype=torch.float64, device=dev)
        out = torch.empty(11, device=dev)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with _timed("train_loss_fwd"):
            L.check(lib.nefes_train_loss_fwd(C.byref(desc), _chk(rgb_fine, "rgb_fine"), _chk(rgb_coarse, "rgb_coarse"),
                                             _chk(rgb_target, "rgb_target"), _chk(beta, "beta"), ptr(sigmas), _chk(feat_fine, "feat_fine"),
                                             _chk(feat_coarse, "feat_coarse"), _chk(feat_fusion, "feat_fusion"),
                                             _chk(feat_target, "feat_target"), _chk(scratch, "scratch", torch.float64), _chk(out, "out"),
                                             C.c_void_p(out.data_ptr() + 32), _stream()), "nefes_train_loss_fwd")
        ctx.desc = desc
        ctx.tensors = (rgb_fine, rgb_coarse, rgb_target, beta, sigmas, feat_fine, feat_coarse, feat_fusion, feat_target)
        ctx.set_materialize_grads(False)               # an output nobody used arrives as None: a null pointer, no zero-filled scalar
        # four tensors on the one buffer, not views of it: an output that is a view of a multi-output function cannot be modified in
        # place (`loss += ...`, as the reference's own classes write)
        store = out.untyped_storage()
        part = lambda off, shape: torch.empty(0, device=dev).set_(store, off, shape)
        terms = part(0, (8,))
        ctx.mark_non_differentiable(terms)
        return part(8, ()), part(9, ()), part(10, ()), terms

    @staticmethod
    def backward(ctx, g_color, g_f, g_fusion, _g_terms):
        rgb_fine, rgb_coarse, rgb_target, beta, sigmas, feat_fine, feat_coarse, feat_fusion, feat_target = ctx.tensors
        need = ctx.needs_input_grad
        fix = lambda g: None if g is None else _f32(g).reshape(1)
        g_color, g_f, g_fusion = fix(g_color), fix(g_f), fix(g_fusion)
        want = lambda i, t, g: torch.empty_like(t) if (need[i] and t is not None and g is not None) else None
        o_rf, o_rc, o_b = want(0, rgb_fine, g_color), want(1, rgb_coarse, g_color), want(3, beta, g_color)
        o_s = torch.empty(1, device=rgb_target.device) if (need[4] and sigmas is not None and g_color is not None) else None
        o_ff, o_fc, o_fu = want(5, feat_fine, g_f), want(6, feat_coarse, g_f), want(7, feat_fusion, g_fusion)
        outs = (o_rf, o_rc, o_b, o_s, o_ff, o_fc, o_fu)
        if all(o is None for o in outs):
            return (None,) * 13
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with _timed("train_loss_bwd"):
            L.check(L.load().nefes_train_loss_bwd(C.byref(ctx.desc), _chk(g_color, "g_color"), _chk(g_f, "g_loss_f"),
                                                  _chk(g_fusion, "g_loss_fusion"), ptr(rgb_fine), ptr(rgb_coarse), ptr(rgb_target), ptr(beta),
                                                  ptr(sigmas), ptr(feat_fine), ptr(feat_coarse), ptr(feat_fusion), ptr(feat_target),
                                                  *[_chk(o, "gradient") for o in outs], _stream()), "nefes_train_loss_bwd")
        if o_s is not None:
            o_s = o_s.reshape(1, 1).expand(ctx.desc.N, ctx.desc.S)           # one number for every element: no [N,S] tensor
        return o_rf, o_rc, None, o_b, o_s, o_ff, o_fc, o_fu, None, None, None, None, None
