"""numpy restatement of nefes_draw_pixels' contract (include/nefes_hip.h): the Philox-4x32-10 sort keys and the selection.

Pixel i = y*W + x of image b: key = (o0 << 32) | o1 of Philox at counter (i, b, epoch lo, epoch hi), key (seed lo, seed hi),
epoch = tick // period.  The draw: the K valid pixels with the smallest (key, i), in ascending i; fewer than K valid: all of them,
repeated cyclically; none: rows of (0, 0)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)

# (counter, key) -> output, from the issue that specified the draw
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on arrays (or scalars) of 32-bit words held in uint64: -> [o0, o1, o2, o3]."""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(W0)) & _M32, (k1 + np.uint64(W1)) & _M32
    return c


def keys(n, seed, epoch, b=0):
    """The n pixels' 64-bit sort keys of image b: uint64 [n]."""
    i = np.arange(n, dtype=np.uint64)
    full = lambda v: np.full(n, v, np.uint64)
    o = philox(i, full(b), full(epoch & 0xFFFFFFFF), full(epoch >> 32), seed & 0xFFFFFFFF, seed >> 32)
    return (o[0] << _32) | o[1]


def draw_indices(H, W, K, seed, epoch, b=0, mask=None):
    """-> (the K drawn pixel indices i = y*W + x in the order the kernel writes them, or None when no pixel is valid; n_valid)."""
    n = H * W
    key = keys(n, seed, epoch, b)
    valid = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    idx = np.nonzero(valid)[0]
    if len(idx) == 0:
        return None, 0
    if len(idx) < K:
        return np.resize(idx, K), len(idx)
    order = idx[np.lexsort((idx, key[idx]))]                 # by key, ties by the lower index
    return np.sort(order[:K]), len(idx)


def draw(B, H, W, K, seed, tick, period=1, mask=None):
    """What nefes_draw_pixels writes: (px float32 [B, K, 2] rows (x, y), n_valid int32 [B]).  mask: [B, H, W] or None."""
    px, nv = np.zeros((B, K, 2), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        sel, nv[b] = draw_indices(H, W, K, seed, tick // period, b, None if mask is None else np.asarray(mask)[b])
        if sel is not None:
            px[b, :, 0], px[b, :, 1] = sel % W, sel // W
    return px, nv
