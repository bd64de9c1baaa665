"""The per-pixel feature loss kernels (`--per_pixel`; csrc/feature_loss.hip pixcos_* / uppixcos_*, ops.pixel_cosine_loss /
ops.upsampled_pixel_cosine_loss) against the torch expression in float64 on the CPU.

"Equal to float64" throughout is the shared rule parity_log.check(tol=T, factor=1.5): e_hip <= max(T, 1.5 e_ref), where the truth is
F.interpolate(mode="bicubic") -> crop -> refine.feature_loss(per_pixel=True) in float64 from the same fp32 inputs, e_ref the distance
of the SAME expression in float32 on the CPU from that truth, and T the floor of the per-channel twins: 3e-7 absolute for the loss
(a float32 number near 1: half an ulp is 6e-8, the reduction order a few more), 2e-6 of the max-norm for gradients.  The upstream
gradient is 3.0, not 1."""
import functools

import numpy as np
import pytest
import torch

from tests import parity_log as P
from tests.test_refine50_oracle import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_LOSS, T_GRAD, UP = 3e-7, 2e-6, 3.0
F = torch.nn.functional


def torch_expression(x, target, dtype, size=None, crop=0):
    """(loss, UP * d loss / d x) of the torch expression on the CPU in `dtype`; x [C, ...] (with `size`: [C,h,w], up-sampled and cropped)."""
    from nefes_amd.refine import feature_loss
    xs = x.to(dtype).clone().requires_grad_()
    a = xs
    if size is not None:
        a = F.interpolate(xs[None], size=size, mode="bicubic")[0]
        if crop:
            a = a[:, crop:-crop, crop:-crop]
    loss = feature_loss(a, target.to(dtype), per_pixel=True)
    (UP * loss).backward()
    return float(loss.detach()), xs.grad.numpy()


def hip(fn, x, *rest, **kw):
    """(loss tensor, cos, UP * d loss / d x) of one of the two ops on the device."""
    xd = x.to(DEV).requires_grad_()
    loss, cos = fn(xd, *rest, return_cos=True, **kw)
    (UP * loss).backward()
    return loss.detach(), cos, xd.grad


def check(tag, loss, grad, x, target, size=None, crop=0, grad_cols=None):
    """The rule for the value and the gradient of one group; grad_cols: compare these columns of a [C,P] gradient only."""
    l64, g64 = torch_expression(x, target, torch.float64, size, crop)
    l32, g32 = torch_expression(x, target, torch.float32, size, crop)
    P.check(tag, "loss (abs) vs float64 torch on the CPU", abs(float(loss) - l64), abs(l32 - l64), abs(float(loss) - l32), tol=T_LOSS, factor=1.5)
    gh = grad.cpu().numpy()
    if grad_cols is not None:
        gh, g64, g32 = gh[:, grad_cols], g64[:, grad_cols], g32[:, grad_cols]
    P.check(tag, "d loss / d input (max-norm) vs float64 torch on the CPU", rel(gh, g64), rel(g32, g64), rel(gh, g32), tol=T_GRAD, factor=1.5)
    assert np.isfinite(gh).all() and np.isfinite(float(loss))


@functools.lru_cache(maxsize=None)
def low_case(G, C, Pn):
    g = torch.Generator().manual_seed(1000 * G + 10 * C + Pn)
    a = torch.randn(G * C, Pn, generator=g)
    return a, torch.randn(G * C, Pn, generator=g) + 0.7 * a


@pytest.mark.parametrize("G,C,Pn", [(1, 128, 4800), (1, 16, 192), (1, 3, 1000), (1, 141, 65), (3, 5, 257)])
def test_pixel_cosine_loss_matches_float64(G, C, Pn):
    """ops.pixel_cosine_loss on [G*C, P]: the loop's own low-resolution shape, small ones, the largest head with P no multiple of a
    wave, and three groups -- each group held to the rule on its own and bit-equal to its own single-group call; the grouped value is
    the sum of the groups' (in float64, rounded once)."""
    from nefes_amd import ops
    a, b = low_case(G, C, Pn)
    loss, cos, grad = hip(ops.pixel_cosine_loss, a, b.to(DEV), groups=G)
    assert cos.dtype == torch.float64 and tuple(cos.shape) == (G,) and not cos.requires_grad
    singles = []
    for k in range(G):
        sl = slice(k * C, (k + 1) * C)
        l1, c1, g1 = (loss, cos, grad) if G == 1 else hip(ops.pixel_cosine_loss, a[sl], b[sl].to(DEV))
        check(f"pixel_cosine_loss[{G},{C},{Pn}][group {k}]", l1, g1, a[sl], b[sl])
        assert torch.equal(c1[0], cos[k]) and torch.equal(g1, grad[sl])
        singles.append(1.0 - float(c1[0]))
        assert float(l1) == np.float32(singles[-1])
    assert float(loss) == np.float32(sum(singles))


def test_pixel_cosine_loss_at_clamped_pixels():
    """(1, 16, 192) with pixel 0: a = 0, pixel 1: b = 0, pixel 2: both zero (torch clamps each norm at eps = 1e-6; a clamped norm is a
    constant).  Everything finite; columns 1 and 2 of the gradient exactly 0; column 0 = -g b / (eps |b| P) by the rule relative to its
    own max -- about 1e6 times the other columns, hence compared apart from columns 3 onward."""
    from nefes_amd import ops
    a, b = (t.clone() for t in low_case(1, 16, 192))
    a[:, 0] = 0
    b[:, 1] = 0
    a[:, 2] = 0
    b[:, 2] = 0
    loss, cos, grad = hip(ops.pixel_cosine_loss, a, b.to(DEV))
    assert torch.isfinite(grad).all() and torch.isfinite(loss) and torch.isfinite(cos).all()
    assert float(grad[:, 1].abs().max()) == 0.0 and float(grad[:, 2].abs().max()) == 0.0
    check("pixel_cosine_loss[clamp] column 0", loss, grad, a, b, grad_cols=slice(0, 1))
    check("pixel_cosine_loss[clamp] columns 3..", loss, grad, a, b, grad_cols=slice(3, None))
    expect = -UP * b[:, 0].double() / (1e-6 * b[:, 0].double().norm() * 192)
    assert rel(grad[:, 0].cpu().numpy(), expect.numpy()) < T_GRAD
    assert float(grad[:, 0].abs().max()) > 1e5 * float(grad[:, 3:].abs().max())


def test_pixel_cosine_loss_with_one_channel():
    """C = 1: every cosine is +-1 and the gradient a cancellation to zero -- the value by the rule, the gradient finite (its `rel` is
    undefined and not asserted)."""
    from nefes_amd import ops
    a, b = low_case(1, 1, 300)
    loss, cos, grad = hip(ops.pixel_cosine_loss, a, b.to(DEV))
    l64, _ = torch_expression(a, b, torch.float64)
    l32, _ = torch_expression(a, b, torch.float32)
    P.check("pixel_cosine_loss[1,1,300]", "loss (abs) vs float64 torch on the CPU", abs(float(loss) - l64), abs(l32 - l64), abs(float(loss) - l32),
            tol=T_LOSS, factor=1.5)
    assert torch.isfinite(grad).all() and float(grad.abs().max()) < 1e-6


UP_SHAPES = [(128, 60, 80, 240, 320, 10, False), (5, 15, 20, 60, 80, 10, False), (3, 9, 11, 31, 45, 3, False), (2, 8, 8, 32, 32, 0, False),
             (4, 6, 70, 24, 280, 1, False), (5, 15, 20, 60, 80, 10, True)]


@functools.lru_cache(maxsize=None)
def up_case(C, h, w, OH, OW, crop, patch, seed=0):
    """x [C,h,w] with its last channel all zeros (and, `patch`, a 7 x 8 source patch zeroed across all channels: the up-sampled pixels
    whose sixteen taps lie inside it are exactly 0 and hit the |a_p| clamp), target = randn + 0.5 up."""
    g = torch.Generator().manual_seed(C * 1000 + h * 10 + w + seed)
    x = torch.randn(C, h, w, generator=g)
    x[C - 1] = 0
    if patch:
        x[:, 4:11, 6:14] = 0
    up = F.interpolate(x[None], size=(OH, OW), mode="bicubic")[0]
    up = up[:, crop:OH - crop, crop:OW - crop]
    return x, (torch.randn(up.shape, generator=g) + 0.5 * up).contiguous()


@pytest.mark.parametrize("C,h,w,OH,OW,crop,patch", UP_SHAPES)
def test_upsampled_pixel_cosine_loss_matches_float64(C, h, w, OH, OW, crop, patch):
    """ops.upsampled_pixel_cosine_loss: the loop's shape, small ones, a non-integer scale, no crop, a wide flat map; one source channel
    all zeros everywhere, and one case with a block of up-sampled pixels at the |a_p| clamp."""
    from nefes_amd import ops
    x, t = up_case(C, h, w, OH, OW, crop, patch)
    loss, cos, grad = hip(ops.upsampled_pixel_cosine_loss, x, t.to(DEV), (OH, OW), crop=crop)
    assert abs((1.0 - float(cos[0])) - float(loss)) < 1e-6 and tuple(grad.shape) == (C, h, w)
    if patch:
        up = ops.bicubic_upsample(x.to(DEV)[None], (OH, OW), crop=crop)[0]
        assert int((up.abs().amax(0) == 0).sum()) >= 100                 # the clamp is really hit
    check(f"upsampled_pixel_cosine_loss[{C},{h},{w},{OH},{OW},{crop}{',patch' if patch else ''}]", loss, grad, x, t, (OH, OW), crop)


@pytest.mark.parametrize("C,h,w,OH,OW,crop,patch", [UP_SHAPES[1], UP_SHAPES[2], UP_SHAPES[5]])
def test_upsampled_kernel_equals_separate_kernels(C, h, w, OH, OW, crop, patch):
    """upsampled_pixel_cosine_loss(x, t) against pixel_cosine_loss(bicubic_upsample(x, crop), t): both obey the rule against float64 (the
    interpolated values are the same bits; the sums run over rows here and over blocks of 256 pixels there), their direct distance is
    recorded."""
    from nefes_amd import ops
    x, t = up_case(C, h, w, OH, OW, crop, patch)
    td = t.to(DEV)
    one = hip(ops.upsampled_pixel_cosine_loss, x, td, (OH, OW), crop=crop)
    two = hip(lambda xd, tt, **kw: ops.pixel_cosine_loss(ops.bicubic_upsample(xd[None], (OH, OW), crop=crop)[0], tt, **kw), x, td)
    l64, g64 = torch_expression(x, t, torch.float64, (OH, OW), crop)
    l32, g32 = torch_expression(x, t, torch.float32, (OH, OW), crop)
    tag = f"uppixcos_vs_separate[{C},{h},{w},{OH},{OW},{crop}{',patch' if patch else ''}]"
    for name, (loss, _, grad) in (("one pass", one), ("separate kernels", two)):
        P.check(tag, f"{name}: loss (abs) vs float64", abs(float(loss) - l64), abs(l32 - l64), tol=T_LOSS, factor=1.5)
        P.check(tag, f"{name}: d loss / d x vs float64", rel(grad.cpu().numpy(), g64), rel(g32, g64), tol=T_GRAD, factor=1.5)
    P.record(tag, "one pass vs separate kernels: loss (abs); d loss / d x (max-norm)", direct=abs(float(one[0]) - float(two[0])),
             e_hip=rel(one[2].cpu().numpy(), two[2].cpu().numpy()), bound=None)


def test_batched_upsampled_loss_equals_single_calls():
    """groups = 3 on (5, 15, 20, 60, 80, 10): per-group mean cosines and gradients bit-equal to three single calls (the same arithmetic per
    group is required), the value the float64 sum of the three."""
    from nefes_amd import ops
    cases = [up_case(5, 15, 20, 60, 80, 10, False, seed=s) for s in range(3)]
    x, t = torch.cat([c[0] for c in cases]), torch.cat([c[1] for c in cases])
    loss, cos, grad = hip(ops.upsampled_pixel_cosine_loss, x, t.to(DEV), (60, 80), crop=10, groups=3)
    total = 0.0
    for k, (xk, tk) in enumerate(cases):
        l1, c1, g1 = hip(ops.upsampled_pixel_cosine_loss, xk, tk.to(DEV), (60, 80), crop=10)
        assert torch.equal(c1[0], cos[k]) and torch.equal(g1, grad[5 * k:5 * k + 5]) and float(l1) == np.float32(1.0 - float(c1[0]))
        total += 1.0 - float(c1[0])
    assert float(loss) == np.float32(total)
    # and the [1, G*C, h, w] layout the refinement loop hands over gives the same bits
    l4, c4, g4 = hip(ops.upsampled_pixel_cosine_loss, x[None], t.to(DEV), (60, 80), crop=10, groups=3)
    assert torch.equal(l4, loss) and torch.equal(c4, cos) and torch.equal(g4[0], grad)


def _low_call(ops):
    a, b = low_case(3, 5, 257)
    bd = b.to(DEV)
    return (lambda xd, out=None: ops.pixel_cosine_loss(xd, bd, groups=3, out=out)), a


def _up_call(ops):
    x, t = up_case(5, 15, 20, 60, 80, 10, False)
    td = t.to(DEV)
    return (lambda xd, out=None: ops.upsampled_pixel_cosine_loss(xd, td, (60, 80), crop=10, out=out)), x


CALLS = {"low": _low_call, "up": _up_call}       # ops -> (f(x on the device, out=None) -> loss, x on the CPU)


def _run(f, x):
    xd = x.to(DEV).requires_grad_()
    loss = f(xd)
    (UP * loss).backward()
    return loss.detach().clone(), xd.grad.clone()


@pytest.mark.parametrize("which", ["low", "up"])
def test_two_calls_give_the_same_bits(which):
    """No atomics, a fixed summation order: loss and gradient of two calls on the same inputs are bit-equal."""
    from nefes_amd import ops
    f, x = CALLS[which](ops)
    (l1, g1), (l2, g2) = _run(f, x), _run(f, x)
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and float(g1.abs().max()) > 0


@pytest.mark.parametrize("which", ["low", "up"])
def test_captured_call_equals_the_eager_call(which):
    """Forward and backward captured in a torch.cuda.graph and replayed twice equal the eager call bit for bit."""
    from nefes_amd import ops
    f, x = CALLS[which](ops)
    l_eager, g_eager = _run(f, x)
    xs = x.to(DEV).requires_grad_()
    seed = torch.full((), UP, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up: gather tables, allocator
        torch.autograd.grad(f(xs), xs, grad_outputs=seed)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = f(xs)
        grad, = torch.autograd.grad(loss, xs, grad_outputs=seed)
    for _ in range(2):
        loss.detach().fill_(-1.0)
        grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l_eager) and torch.equal(grad, g_eager)


@pytest.mark.parametrize("which", ["low", "up"])
def test_pixel_losses_write_their_value_into_the_callers_buffer(which):
    """`out=` as tests/test_gpu_refine.py::test_feature_losses_write_their_value_into_the_callers_buffer holds the per-channel functions
    to: the forward kernel writes into the caller's 0-d fp32 buffer, the returned loss shares its storage, value and gradient are
    bit-equal to the call without `out`, a later call without `out` leaves the buffer alone, a buffer of the wrong kind is refused."""
    from nefes_amd import ops
    f, x0 = CALLS[which](ops)
    x = x0.to(DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    plain = f(xa)
    (2.0 * plain).backward()
    buf = torch.full((), -7.0, device=DEV)
    into = f(xb, out=buf)
    (2.0 * into).backward()
    assert torch.equal(buf, plain.detach()) and torch.equal(into.detach(), plain.detach())
    assert into.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() and into.data_ptr() == buf.data_ptr()
    assert not buf.requires_grad and torch.equal(xa.grad, xb.grad) and float(xa.grad.abs().max()) > 0
    kept = buf.clone()
    other = f(-x.roll(1, -1))                          # another value, no `out`: a fresh tensor
    assert not torch.equal(other, kept) and other.data_ptr() != buf.data_ptr() and torch.equal(buf, kept)
    for bad in (torch.zeros(1, device=DEV), torch.zeros((), device=DEV, dtype=torch.float64), torch.zeros((), device=DEV).requires_grad_()):
        with pytest.raises(ValueError, match="`out`"):
            f(x, out=bad)
