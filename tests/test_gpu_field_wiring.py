"""The autograd Functions that serve tuned AND generic packs (ops.FieldFromRays / ops.FieldFromPoints behind field_from_rays /
field_from_points) against the launchers called by hand on the same pack: the same kernels on the same inputs, so raw_t and every
gradient are bit-identical, and the timer keys show that no launch was gained or lost.  N = 5 rays x S = 64 samples = 320 samples: a
ragged last 128-sample tile."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, S = 5, 64


@pytest.fixture(autouse=True)
def _default_switches():
    from nefes_amd import ops
    old = ops.SPLIT, ops.USE_X6, ops.FIELD_GENERIC
    ops.SPLIT, ops.USE_X6, ops.FIELD_GENERIC = "h3", True, False
    yield
    ops.SPLIT, ops.USE_X6, ops.FIELD_GENERIC = old


@pytest.fixture(scope="module")
def packs():
    from nefes_amd.field import NeRFH_NFF
    out = {}
    for kind, (W, D) in (("tuned", (128, 8)), ("generic", (64, 2))):
        net = NeRFH_NFF('fine', D=D, W=W, skips=[4], encode_appearance=True, encode_transient=True, in_channels_a=50, in_channels_t=20,
                        f_dim=16).requires_grad_(False).to(DEV)
        assert net.uses_generic() == (kind == "generic")
        out[kind] = (net, net.packed_any())           # (the module owns the pack's cache: keep both)
    return out


@pytest.fixture(scope="module")
def inputs():
    gen = torch.Generator().manual_seed(5)
    o = torch.rand(N, 3, generator=gen) - .5
    d = torch.randn(N, 3, generator=gen)
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(N, S, generator=gen) * 3.5 + .25, -1).values
    return tuple(t.to(DEV) for t in (o, d, v, z))


def _counted(fn):
    from nefes_amd import ops
    ops.TIMERS = {}
    try:
        out = fn()
        return out, {k: len(t) for k, t in ops.TIMERS.items()}
    finally:
        ops.TIMERS = None


def _direct(kind):
    """(forward, backward) launchers called by hand: what the Functions wrapped before they served both kinds of pack."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    if kind == "generic":
        return ops.field_fwd_generic, lambda pk, *a, **k: ops.field_bwd_generic(pk, L.FIELD_FULL, *a, **k)
    return (lambda pk, mode, n, s, **k: ops.field_fwd_x6(pk, mode, n, s, **k)), lambda pk, *a, **k: ops.field_bwd(pk, *a, **k)


def _same(name, a, b):
    assert a.shape == b.shape and torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("kind", ["tuned", "generic"])
def test_field_from_rays_is_the_direct_sequence(packs, inputs, kind):
    from nefes_amd import lib as L
    from nefes_amd import ops
    _, pk = packs[kind]
    assert ops.is_generic(pk) == (kind == "generic")
    o, d, v, z = inputs
    G = torch.randn(N, pk.n_raw(L.FIELD_FULL), S, generator=torch.Generator().manual_seed(6)).to(DEV)
    oa, da, va = (t.clone().requires_grad_() for t in (o, d, v))

    def through_autograd():
        raw = ops.field_from_rays(oa, da, va, z, pk, L.FIELD_FULL)
        raw.backward(G)
        return raw.detach(), oa.grad, da.grad, va.grad

    fwd, bwd = _direct(kind)

    def by_hand():
        raw, masks = fwd(pk, L.FIELD_FULL, N, S, rays_o=o, rays_d=d, z=z, viewdirs=v, want_masks=True)
        g_pts, g_vs = bwd(pk, N, S, raw, G, masks, rays_o=o, rays_d=d, z=z, viewdirs=v)
        return (raw,) + tuple(ops.ray_grad_reduce(N, S, z, g_pts, g_vs))

    got, keys = _counted(through_autograd)
    want, keys_direct = _counted(by_hand)
    print(f"[field_wiring rays {kind}] launches {keys}")
    assert keys == keys_direct and sorted(keys.values()) == [1, 1, 1], (keys, keys_direct)
    assert any(k.startswith("field_fwd[full") and ("generic" in k) == (kind == "generic") for k in keys), keys
    for name, a, b in zip(("raw_t", "d rays_o", "d rays_d", "d viewdirs"), got, want):
        _same(f"{kind} {name}", a, b)
    assert bool(torch.isfinite(got[0]).all()) and float(got[1].abs().max()) > 0


@pytest.mark.parametrize("kind", ["tuned", "generic"])
def test_field_from_points_is_the_direct_sequence(packs, inputs, kind):
    from nefes_amd import lib as L
    from nefes_amd import ops
    _, pk = packs[kind]
    o, d, v, z = inputs
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).contiguous()
    G = torch.randn(N, pk.n_raw(L.FIELD_FULL), S, generator=torch.Generator().manual_seed(7)).to(DEV)
    pa, va = pts.clone().requires_grad_(), v.clone().requires_grad_()

    def through_autograd():
        raw = ops.field_from_points(pa, va, pk, L.FIELD_FULL)
        raw.backward(G)
        return raw.detach(), pa.grad, va.grad

    fwd, bwd = _direct(kind)

    def by_hand():
        flat = pts.reshape(-1, 3)
        raw, masks = fwd(pk, L.FIELD_FULL, N, S, pts=flat, viewdirs=v, want_masks=True)
        g_pts, g_vs = bwd(pk, N, S, raw, G, masks, pts=flat, viewdirs=v)
        _, _, g_v = ops.ray_grad_reduce(N, S, torch.zeros(N, S, device=DEV), g_pts, g_vs)
        return raw, g_pts.reshape(N, S, 3), g_v

    got, keys = _counted(through_autograd)
    want, keys_direct = _counted(by_hand)
    print(f"[field_wiring points {kind}] launches {keys}")
    assert keys == keys_direct and sorted(keys.values()) == [1, 1, 1], (keys, keys_direct)
    for name, a, b in zip(("raw_t", "d pts", "d viewdirs"), got, want):
        _same(f"{kind} {name}", a, b)
    assert bool(torch.isfinite(got[0]).all()) and float(got[1].abs().max()) > 0
