"""Float64 references for pixel lists px [K, 2] of (x, y) = (column, row): the rays through them and the bilinear sample of a map at them.
Shared by tests/test_pixels_args.py (CPU) and tests/test_gpu_pixels.py."""
import torch


def rays_at(px, K, c2w):
    """The three lines of tests/test_gpu_intrinsics.py::rays_of with the pixel list in place of the meshgrid, in K's dtype:
    (rays_o, rays_d, viewdirs), each [len(px), 3]; differentiable w.r.t. the pose and the camera K = (fx, fy, cx, cy)."""
    ii, jj = px[:, 0].to(K.dtype), px[:, 1].to(K.dtype)
    d = torch.sum(torch.stack([(ii - K[2]) / K[0], -(jj - K[3]) / K[1], -torch.ones_like(ii)], -1)[..., None, :] * c2w[:3, :3], -1).reshape(-1, 3)
    return c2w[:3, 3].expand(d.shape), d, d / torch.norm(d, dim=-1, keepdim=True)


def bilinear(map, px):
    """map [C, H, W] sampled at px in float64 -> [C, K]: the float32 pixel values cast up, clamped to [0, W-1] x [0, H-1], split into cell
    and fraction, the second tap's index clamped to the last column / row."""
    m = map.double()
    H, W = m.shape[1:]
    p = px.float().double()
    x, y = p[:, 0].clamp(0, W - 1), p[:, 1].clamp(0, H - 1)
    x0, y0 = x.floor().long(), y.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    fx, fy = x - x0, y - y0
    top = m[:, y0, x0] * (1 - fx) + m[:, y0, x1] * fx
    bot = m[:, y1, x0] * (1 - fx) + m[:, y1, x1] * fx
    return top * (1 - fy) + bot * fy


def grid_pixels(W, row0, nrows):
    """The row-major integer pixels of rows [row0, row0 + nrows) of a frame W wide: float32 [nrows * W, 2]."""
    jj, ii = torch.meshgrid(torch.arange(row0, row0 + nrows), torch.arange(W), indexing="ij")
    return torch.stack([ii, jj], -1).reshape(-1, 2).float()
