"""Train mode of the generic field kernels (nefes_amd/csrc/field_generic.hip TRAIN instances, train.field_train_generic): weight
gradients of networks of any --netwidth / --netdepth against the float64 oracle on the kernels' own ReLU branches, the two traps of
the shared train layout (the unwritten remainder of the last 128-sample tile, the dead samples of a tile), the device re-pack, the
route through render() and the opt-in switch.  Tolerances are tests/test_gpu_train.py's."""
import ctypes as C
import types

import pytest
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import generic_util as G
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_RAYS, N_S = 5, 33                 # M = 165 = 128 + 37: three 64-sample (six 32-sample) tiles leave the second train tile part covered


def _nets(Wd, D, C_, typ, in_xyz=63):
    coarse, fine = G.modules(Wd, D, C_, in_xyz=in_xyz, device=DEV)
    net = coarse if typ == "coarse" else fine
    for n, p in net.named_parameters():
        if not n.startswith(("fusion_net", "exposure_embedding")):
            p.requires_grad_(True)
    return net


def _oracle_params(net, names, dtype):
    p = {}
    for n, t in net.named_parameters():
        if not n.startswith(("fusion_net", "exposure_embedding")):
            p[n] = t.detach().cpu().to(dtype).clone().requires_grad_(n in names)
    return p


def _inputs(seed=2, N=N_RAYS, S=N_S):
    g = torch.Generator().manual_seed(seed)
    rays_o = torch.randn(N, 3, generator=g) * 0.3
    rays_d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    z = torch.sort(torch.rand(N, S, generator=g) * 3.5 + 0.2, -1)[0]
    return rays_o, rays_d, z, g


def _run(net, mode, rays_o, rays_d, z, Gr=None, gen=None):
    """One train-mode forward (+ backward against the cotangent Gr) -> raw_t, Gr, debug buffers, tap."""
    from nefes_amd import train as TR
    TR.DEBUG = {}
    try:
        with B.tapped() as tap:
            raw_t = TR.field_train_generic(net, mode, rays_o.to(DEV), rays_d.to(DEV), rays_d.to(DEV), z.to(DEV))
            if Gr is None:
                Gr = torch.randn(raw_t.shape, generator=gen)
            (raw_t * Gr.to(DEV)).sum().backward()
        dbg = dict(TR.DEBUG)
    finally:
        TR.DEBUG = None
    return raw_t, Gr, dbg, tap


CASES = [(64, 6, 16, "coarse"), (64, 6, 16, "fine"), (96, 5, 128, "fine"), (32, 1, 16, "fine"), (128, 4, 16, "coarse"),
         (288, 2, 16, "fine"), (512, 8, 16, "fine")]


@pytest.mark.parametrize("Wd,D,C_,typ", CASES)
def test_field_train_generic_weight_grads(Wd, D, C_, typ, monkeypatch):
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    monkeypatch.setattr(ops, "TIMERS", {})
    mode = L.FIELD_STATIC if typ == "coarse" else L.FIELD_FULL
    net = _nets(Wd, D, C_, typ)
    rays_o, rays_d, z, gen = _inputs()
    N, S, M = N_RAYS, N_S, N_RAYS * N_S
    raw_t, Gr, dbg, tap = _run(net, mode, rays_o, rays_d, z, gen=gen)
    assert set(ops.TIMERS) == {"field_fwd_train[generic]", "field_bwd_train[generic]"}, set(ops.TIMERS)
    acts, off = dbg["acts"], dbg["off"]
    tag = f"generic_train[{Wd},{D},{C_},{typ}]"
    names = TR.param_names_generic(net, mode)
    # ---- the saved hidden outputs of the trunk against relu(pre) of a float64 forward; the fp32 oracle is the yardstick ----
    skip = 4 if D > 4 else -1
    trunk = {}
    for dt in (torch.float64, torch.float32):
        p = _oracle_params(net, (), dt)
        pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]).to(dt)
        e = O.freq_encode(pts.reshape(-1, 3), 10)
        h, outs = e, []
        for l in range(1, D + 1):
            if l - 1 == skip:
                h = torch.cat([e, h], 1)
            h = torch.relu(torch.nn.functional.linear(h, p[f"xyz_encoding_{l}.0.weight"], p[f"xyz_encoding_{l}.0.bias"]))
            outs.append(h)
        trunk[dt] = [e] + outs
    blocks = [(L.TB_E, 63)] + [(L.TB_L1 + l, Wd) for l in range(D)]
    for (b, n), ref64, ref32 in zip(blocks, trunk[torch.float64], trunk[torch.float32]):
        got = acts[:, off[b]:off[b] + n, :].permute(0, 2, 1).reshape(-1, n)[:M].cpu()
        B.three_way(tag, f"saved output of block {b}", got, ref32, ref64)
    # ... and the blocks behind the trunk: DV, FINAL, the outputs of DIR and T0..T2 with their zero padding rows
    H2, Hp = Wd // 2, (Wd // 2 + 31) // 32 * 32
    heads = {}
    for dt in (torch.float64, torch.float32):
        p = _oracle_params(net, (), dt)
        lin = lambda name, x: torch.nn.functional.linear(x, p[name + ".weight"], p[name + ".bias"])
        dv = O.freq_encode(rays_d.to(dt), 4)[:, None, :].expand(N, S, 27).reshape(M, 27)
        fin = lin("xyz_encoding_final", trunk[dt][-1])
        x = torch.cat([fin, dv], 1)
        out = {L.TB_DV: dv, L.TB_FINAL: fin, L.TB_DIR: torch.relu(lin("dir_encoding.0", x))}
        if typ == "fine":
            out[L.TB_T0] = torch.relu(lin("transient_encoding.0", x))
            out[L.TB_T1] = torch.relu(lin("transient_encoding.2", out[L.TB_T0]))
            out[L.TB_T2] = torch.relu(lin("transient_encoding.4", out[L.TB_T1]))
        heads[dt] = out
    for b, ref64 in heads[torch.float64].items():
        n = ref64.shape[1]
        blk = acts[:, off[b]:off[b + 1], :].permute(0, 2, 1).reshape(-1, off[b + 1] - off[b])[:M].cpu()
        B.three_way(tag, f"saved output of block {b}", blk[:, :n], heads[torch.float32][b], ref64)
        assert off[b + 1] - off[b] == {L.TB_DV: 32, L.TB_FINAL: Wd}.get(b, Hp)
        assert bool((blk[:, n:] == 0).all()), b                           # rows 27..31 of DV, rows W / 2 .. Hp of the half-width layers
    # ---- gradients: the float64 oracle on the kernels' ReLU branches (tests/branch.py), after auditing those branches ----
    pin = G.GenericPinned(tap)
    p = _oracle_params(net, names, torch.float64)
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]).double()
    with G.oracle_depth(D):
        raw = O.query_field(p, pts, rays_d.double(), typ, typ == "fine", False, act=pin.act(True))
    flips, units, worst_pre = pin.summary()
    P.record(tag, "relu branch flips vs float64", flips=flips, units=units, worst_preact_rel=worst_pre)
    assert worst_pre < 2e-5 and flips <= max(8, units // 100000), (flips, units, worst_pre)
    e_raw = B.rel(raw_t.permute(0, 2, 1), raw)
    print(f"[{tag}] raw_t vs float64: {e_raw:.2e}")
    assert e_raw < 2e-5
    (raw * Gr.permute(0, 2, 1).double()).sum().backward()
    sd = dict(net.named_parameters())
    worst = ("", 0.)
    for n in names:
        assert sd[n].grad is not None and sd[n].grad.shape == sd[n].shape, n
        worst = max(worst, (n, B.rel(sd[n].grad, p[n].grad)), key=lambda t: t[1])
    print(f"[{tag}] worst parameter gradient vs float64 [branch-pinned]: {worst[1]:.2e} ({worst[0]})")
    P.record(tag, "worst parameter gradient [branch-pinned]", e_hip=worst[1], e_ref=None, bound=1e-4)
    assert worst[1] < 1e-4, worst


def test_padding_rows_and_dead_samples_are_zero(monkeypatch):
    """(96, 5): W / 2 = 48 in 64 rows, the 131-row head in 160, SIG 1 of 32, TH 5 of 32; M = 165 of 256 buffer columns."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    Wd, D, C_ = 96, 5, 128
    net = _nets(Wd, D, C_, "fine")
    rays_o, rays_d, z, gen = _inputs()
    M = N_RAYS * N_S
    _, Gr, dbg, _ = _run(net, L.FIELD_FULL, rays_o, rays_d, z, gen=gen)
    dacts, off, rows = dbg["dacts"], dbg["off"], dbg["rows"]
    flat = dacts.permute(1, 0, 2).reshape(rows, -1)                      # [rows, 256 buffer columns]
    assert flat.shape[1] == 256
    g_rows = slice(off[L.TB_L1], rows)
    assert bool((flat[g_rows, M:] == 0).all())                           # dead samples of a tile AND the tiles no sample reaches
    assert bool(flat[g_rows, :M].isfinite().all())
    real = {L.TB_DIR: 48, L.TB_T0: 48, L.TB_T1: 48, L.TB_T2: 48, L.TB_RGB: 3 + C_, L.TB_SIG: 1, L.TB_TH: 5}
    for b, n in real.items():
        assert off[b + 1] - off[b] > n
        assert bool((flat[off[b] + n:off[b + 1]] == 0).all()), b
        assert float(flat[off[b]:off[b] + n, :M].abs().max()) > 0, b
    acts = dbg["acts"].permute(1, 0, 2).reshape(rows, -1)
    assert bool(acts[:off[L.TB_RGB]].isfinite().all())                   # every X operand column is written (0 * NaN would poison dW)
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    # the same step on buffers that start as NaN / -1 instead of whatever torch.empty returns: bit-identical gradients
    real_torch = torch

    class Poisoned:
        def __getattr__(self, k):
            return getattr(real_torch, k)

        @staticmethod
        def empty(*a, **kw):
            t = real_torch.empty(*a, **kw)
            return t.fill_(float("nan") if t.is_floating_point() else -1)

        @staticmethod
        def empty_like(x, **kw):
            t = real_torch.empty_like(x, **kw)
            return t.fill_(float("nan") if t.is_floating_point() else -1)

    monkeypatch.setattr(TR, "torch", Poisoned())
    for p in net.parameters():
        p.grad = None
    _run(net, L.FIELD_FULL, rays_o, rays_d, z, Gr=Gr)
    for n, p in net.named_parameters():
        if n in grads:
            assert bool(p.grad.isfinite().all()), n
            assert torch.equal(p.grad, grads[n]), n


@pytest.mark.parametrize("Wd,D,C_,typ,in_xyz", [(64, 6, 16, "coarse", 63), (96, 5, 128, "fine", 63), (64, 6, 16, "fine", 33)])
def test_device_repack_bit_identical(Wd, D, C_, typ, in_xyz, monkeypatch):
    from nefes_amd import ops
    net = _nets(Wd, D, C_, typ, in_xyz=in_xyz)
    pk = net.packed_generic()
    ptr, gen0 = pk.blob.data_ptr(), pk.generation
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.01)
    host_calls = []
    lib = ops.L.load()

    class Counting:
        def __getattr__(self, k):
            if k == "nefes_generic_pack":
                host_calls.append(k)
            return getattr(lib, k)

    monkeypatch.setattr(ops.L, "load", lambda: Counting())
    pk2 = net.packed_generic()
    assert pk2 is pk and pk.blob.data_ptr() == ptr and pk.generation == gen0 + 1 and not host_calls
    monkeypatch.undo()
    net._pk_gen = None
    fresh = net.packed_generic()                                         # the host packer on the same values
    assert fresh is not pk and torch.equal(fresh.blob, pk.blob)


def _render_kw(coarse, fine, Nc, Ni):
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True)
    return dict(network_query_fn=None, perturb=0., N_importance=Ni, N_samples=Nc, network_fn=coarse, network_fine=fine,
                use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=False, args=args, ndc=False, lindisp=False)


def test_training_steps_through_render(monkeypatch):
    """Eight Adam steps of the stage-1 + feature loss on a (64, 6) coarse + fine pair: the first loss is the fp32 oracle's, the loss
    falls, the host packer never runs again, and a backward across a re-pack raises."""
    from nefes_amd import ops
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    H, W, focal, Nc, Ni, C_ = 16, 16, 24.0, 32, 16, 16
    coarse, fine = _nets(64, 6, C_, "coarse"), _nets(64, 6, C_, "fine")
    kw = _render_kw(coarse, fine, Nc, Ni)
    ro, rd = O.ray_bundle(H, W, focal, O.bench_pose())
    gen = torch.Generator().manual_seed(1)
    t_rgb, t_feat = torch.rand(H * W, 3, generator=gen), torch.randn(H * W, C_, generator=gen)

    def loss_of(rgb, ex):
        return (((rgb - t_rgb.to(rgb)) ** 2).mean() + ((ex["feat_map"] - t_feat.to(rgb)) ** 2).mean()
                + ((ex["rgb0"] - t_rgb.to(rgb)) ** 2).mean())

    # the fp32 oracle's first loss (same weights, before any step)
    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni, perturb=0., test_time=False, transient_at_test=True, NeRFW=True)
    with torch.no_grad(), G.oracle_depth(6):
        rgb_r, _, _, ex_r = O.render(H, W, focal, G.oracle_params(coarse, torch.float32), G.oracle_params(fine, torch.float32), cfg,
                                     rays=(ro, rd), near=0., far=4.)
        loss_ref = float(loss_of(rgb_r, ex_r))
    prm = [p for net in (coarse, fine) for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]
    opt = torch.optim.Adam(prm, lr=5e-4)
    coarse.packed_generic(), fine.packed_generic()                      # packed on the host once, here
    host_calls = []
    lib = ops.L.load()

    class Counting:
        def __getattr__(self, k):
            if k == "nefes_generic_pack":
                host_calls.append(k)
            return getattr(lib, k)

    monkeypatch.setattr(ops.L, "load", lambda: Counting())
    rays = (ro.reshape(-1, 3).to(DEV), rd.reshape(-1, 3).to(DEV))
    losses = []
    for _ in range(8):
        rgb, _, _, ex = render(H, W, focal, rays=rays, near=0., far=4., **kw)
        loss = loss_of(rgb, ex)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"[generic_train_render] losses {losses}, fp32 oracle's first {loss_ref}")
    assert not host_calls
    assert abs(losses[0] - loss_ref) < 1e-5 * abs(loss_ref), (losses[0], loss_ref)
    assert losses[-1] < losses[0], losses
    # a backward across a re-pack raises
    rgb, _, _, ex = render(H, W, focal, rays=rays, near=0., far=4., **kw)
    with torch.no_grad():
        for p in prm:
            p.add_(1e-3)
    coarse.packed_generic(), fine.packed_generic()
    with pytest.raises(RuntimeError, match="re-packed"):
        loss_of(rgb, ex).backward()


def test_joint_ray_and_weight_gradients(monkeypatch):
    """Asking for the ray gradients as well leaves the weight gradients unchanged, and the ray gradients are the frozen generic
    path's on the same weights (the same backward chain)."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    net = _nets(64, 6, 16, "fine")
    rays_o, rays_d, z, gen = _inputs()
    _, Gr, _, _ = _run(net, L.FIELD_FULL, rays_o, rays_d, z, gen=gen)
    base = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    for p in net.parameters():
        p.grad = None
    o, d, v = (t.to(DEV).clone().requires_grad_(True) for t in (rays_o, rays_d, rays_d))
    raw_t = TR.field_train_generic(net, L.FIELD_FULL, o, d, v, z.to(DEV))
    (raw_t * Gr.to(DEV)).sum().backward()
    for n, p in net.named_parameters():
        if n in base:
            assert torch.equal(p.grad, base[n]), n
    o2, d2, v2 = (t.to(DEV).clone().requires_grad_(True) for t in (rays_o, rays_d, rays_d))
    net.requires_grad_(False)
    raw_f = ops.field_from_rays(o2, d2, v2, z.to(DEV), net.packed_generic(), L.FIELD_FULL)
    (raw_f * Gr.to(DEV)).sum().backward()
    assert B.rel(raw_f, raw_t) < 1e-6
    for a, b, name in ((o, o2, "rays_o"), (d, d2, "rays_d"), (v, v2, "viewdirs")):
        assert float(b.grad.abs().max()) > 0
        assert B.rel(a.grad, b.grad) < 1e-6, name


def test_comparison_mode_against_the_tuned_train_path(monkeypatch):
    """FIELD_GENERIC and GENERIC_TRAIN both on: a (128, 8, C = 128) fine network trains on the generic kernels; its gradients and the
    tuned fp16 train path's, same weights and inputs, are both within the pinned 1e-4 of float64."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    Wd, D, C_ = 128, 8, 128
    net = _nets(Wd, D, C_, "fine")
    rays_o, rays_d, z, gen = _inputs()
    names = TR.param_names_generic(net, L.FIELD_FULL)
    assert names == TR.param_names(net, L.FIELD_FULL)
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]).double()
    errs, Gr = {}, None
    for which in ("generic", "tuned"):
        for p in net.parameters():
            p.grad = None
        monkeypatch.setattr(ops, "FIELD_GENERIC", which == "generic")
        monkeypatch.setattr(ops, "GENERIC_TRAIN", which == "generic")
        assert net.uses_generic() == (which == "generic")
        with B.tapped() as tap:
            fn = TR.field_train_generic if which == "generic" else TR.field_train
            raw_t = fn(net, L.FIELD_FULL, rays_o.to(DEV), rays_d.to(DEV), rays_d.to(DEV), z.to(DEV))
            if Gr is None:
                Gr = torch.randn(raw_t.shape, generator=gen)
            (raw_t * Gr.to(DEV)).sum().backward()
        pin = G.GenericPinned(tap) if which == "generic" else B.Pinned(tap, Wd)
        p = _oracle_params(net, names, torch.float64)
        raw = O.query_field(p, pts, rays_d.double(), "fine", True, False, act=pin.act(True))
        flips, units, worst_pre = pin.summary()
        assert worst_pre < 2e-5 and flips <= max(8, units // 100000), (which, flips, units, worst_pre)
        (raw * Gr.permute(0, 2, 1).double()).sum().backward()
        sd = dict(net.named_parameters())
        errs[which] = max(B.rel(sd[n].grad, p[n].grad) for n in names)
        P.record("generic_train_comparison[128,8,128]", f"worst parameter gradient, {which} train path [branch-pinned]",
                 e_hip=errs[which], e_ref=None, bound=1e-4)
    print(f"[generic_train_comparison] worst gradient error vs float64: {errs}")
    assert errs["generic"] < 1e-4 and errs["tuned"] < 1e-4, errs


def test_switch_off_refuses_naming_the_shape_and_the_switch():
    from nefes_amd import ops
    from nefes_amd.render import render
    assert ops.GENERIC_TRAIN is False
    coarse, fine = _nets(96, 5, 16, "coarse"), _nets(96, 5, 16, "fine")
    ro, rd = O.ray_bundle(4, 4, 6.0, O.bench_pose())
    with pytest.raises(NotImplementedError, match=r"train mode.*D=5.*W=96.*NEFES_GENERIC_TRAIN"):
        render(4, 4, 6.0, rays=(ro.reshape(-1, 3).to(DEV), rd.reshape(-1, 3).to(DEV)), near=0., far=4., **_render_kw(coarse, fine, 8, 8))


@pytest.mark.parametrize("tag", ["w64d6c16", "w96d5c128"])
def test_generic_train_vs_reference_golden(golden, tag, monkeypatch):
    """One train step through render() against tensors captured from the reference itself (tools/make_golden_generic_train.py):
    the rules of tests/test_gpu_train.py check_train_golden -- maps 2e-5, extras 5e-5, loss 1e-5 rel, every gradient within 1e-3 of
    the reference's with cosine > 0.9995, and the unpinned three-way bound P.bound(e_ref, tol=1e-3)."""
    import numpy as np
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    g = golden("generic_train")
    t = f"gt.{tag}"
    Wd, D, C_, Nc, Ni, H, W, focal = g[f"{t}.cfg"]
    Wd, D, C_, Nc, Ni, H, W, focal = int(Wd), int(D), int(C_), int(Nc), int(Ni), int(H), int(W), float(focal)
    coarse, fine = _nets(Wd, D, C_, "coarse"), _nets(Wd, D, C_, "fine")
    for typ, m in (("coarse", coarse), ("fine", fine)):                  # the seed reproduces the reference's parameters
        for k, v in m.state_dict().items():
            key = f"{t}.sum.{typ}.{k}"
            if key in g:
                v = v.cpu()
                np.testing.assert_allclose(np.array([v.double().sum().item(), v.double().abs().sum().item(), float(v.flatten()[0])]),
                                           g[key], rtol=0, atol=0, err_msg=key)
    assert coarse.uses_generic() and fine.uses_generic()
    rays_o, rays_d = O.ray_bundle(H, W, focal, torch.from_numpy(g[f"{t}.c2w"])[:3, :4])
    rgb, disp, acc, ex = render(H, W, focal, rays=(rays_o.to(DEV), rays_d.to(DEV)), near=0., far=4., **_render_kw(coarse, fine, Nc, Ni))
    rel = lambda a, b: float(np.abs(a.detach().cpu().numpy() - b).max() / max(np.abs(b).max(), 1e-12))
    e_maps = {"rgb": rel(rgb, g[f"{t}.rgb"]), "acc": rel(acc, g[f"{t}.acc"]), "disp": rel(disp, g[f"{t}.disp"])}
    print(f"[generic_train_golden[{tag}]] maps vs the reference: {e_maps}")
    assert max(e_maps.values()) < 2e-5, e_maps
    for k in [k for k in g if k.startswith(f"{t}.ex.")]:
        e = rel(ex[k.split(".ex.")[1]], g[k])
        assert e < 5e-5, (k, e)
    t_rgb, t_feat = torch.from_numpy(g[f"{t}.t_rgb"]).to(DEV), torch.from_numpy(g[f"{t}.t_feat"]).to(DEV)
    loss_of = lambda rgb_, ex_, a, b: ((rgb_ - a) ** 2).mean() + ((ex_["feat_map"] - b) ** 2).mean() + ((ex_["rgb0"] - a) ** 2).mean()
    loss = loss_of(rgb, ex, t_rgb, t_feat)
    print(f"[generic_train_golden[{tag}]] loss {float(loss.detach())} reference {float(g[f'{t}.loss'])}")
    assert abs(float(loss.detach()) - float(g[f"{t}.loss"])) < 1e-5 * float(g[f"{t}.loss"])
    loss.backward()
    # the float64 oracle on ITS OWN branches (unpinned) for the three-way record
    pc = _oracle_params(coarse, TR.param_names_generic(coarse, L.FIELD_STATIC), torch.float64)
    pf = _oracle_params(fine, TR.param_names_generic(fine, L.FIELD_FULL), torch.float64)
    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni, perturb=0., test_time=False, transient_at_test=True, NeRFW=True)
    with G.oracle_depth(D):
        rgb_r, _, _, ex_r = O.render(H, W, focal, pc, pf, cfg, rays=(rays_o.double(), rays_d.double()), near=0., far=4.)
        loss_of(rgb_r, ex_r, t_rgb.cpu().double(), t_feat.cpu().double()).backward()
    n, worst = 0, {"e_hip": 0., "e_ref": 0., "direct": 0.}
    keys = [k for k in g if k.startswith(f"{t}.grad.")]
    assert len(keys) == 2 * (D + 4) + 2 * (D + 10)                       # every parameter of both networks
    for k in keys:
        net, name = k[len(f"{t}.grad."):].split(".", 1)
        got = dict((coarse if net == "coarse" else fine).named_parameters())[name].grad
        assert got is not None and tuple(got.shape) == g[k].shape, k
        a, b = got.detach().cpu().double().reshape(-1), torch.from_numpy(g[k]).double().reshape(-1)
        if float(b.abs().max()) == 0.:                                   # e.g. transient_beta: beta is not in this loss
            assert float(a.abs().max()) == 0., k
            continue
        direct = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        t64 = (pc if net == "coarse" else pf)[name].grad
        if t64 is not None and float(t64.abs().max()) > 0:
            t64 = t64.reshape(-1)
            sc = t64.abs().max()
            worst["e_hip"] = max(worst["e_hip"], float((a - t64).abs().max() / sc))
            worst["e_ref"] = max(worst["e_ref"], float((b - t64).abs().max() / sc))
        worst["direct"] = max(worst["direct"], direct)
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))
        assert direct < 1e-3 and cos > 0.9995, (k, direct, cos)
        n += 1
    bound = P.bound(worst["e_ref"], tol=1e-3)
    print(f"[generic_train_golden[{tag}]] worst gradient: {worst}, bound {bound}, {n} gradients compared")
    P.record(f"generic_train_golden[{tag}]", "worst parameter gradient, UNPINNED: hip / reference fp32 vs float64 on its own branches",
             bound=bound, **worst)
    assert worst["e_hip"] <= bound, worst
    assert n >= 2 * (D + 4) + 2 * (D + 10) - 8


def test_pose_gradient_through_render_with_trainable_weights(monkeypatch):
    """Joint pose + weight step through render() at (64, 6): d c2w from the train path (trainable weights) against the frozen generic
    path's on the same weights and the float64 oracle on the kernels' branches and depths, under the pinned three-way rule with the frozen path
    in the place of the fp32 reference; asking for d c2w leaves the weight gradients unchanged."""
    from nefes_amd import ops
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN", True)
    H, W, focal, Nc, Ni, C_ = 6, 6, 9.0, 32, 16, 16
    coarse, fine = _nets(64, 6, C_, "coarse"), _nets(64, 6, C_, "fine")
    kw = _render_kw(coarse, fine, Nc, Ni)
    gen = torch.Generator().manual_seed(3)
    t_rgb, t_feat = torch.rand(H * W, 3, generator=gen), torch.randn(H * W, C_, generator=gen)
    loss_of = lambda rgb, ex: (((rgb - t_rgb.to(rgb)) ** 2).mean() + ((ex["feat_map"] - t_feat.to(rgb)) ** 2).mean()
                               + ((ex["rgb0"] - t_rgb.to(rgb)) ** 2).mean())
    nets = (coarse, fine)
    wgrads = lambda: {(i, n): p.grad.clone() for i, m in enumerate(nets) for n, p in m.named_parameters() if p.grad is not None}

    def clear():
        for m in nets:
            for p in m.parameters():
                p.grad = None

    # weights alone (rays from a constant pose)
    c0 = O.bench_pose()[:3, :4].to(DEV)
    ro, rd = O.ray_bundle(H, W, focal, c0.cpu())
    rgb, _, _, ex = render(H, W, focal, rays=(ro.to(DEV), rd.to(DEV)), near=0., far=4., **kw)
    loss_of(rgb, ex).backward()
    base = wgrads()
    assert len(base) >= 2 * 10 + 2 * 16
    clear()
    # weights and pose
    c2w = c0.clone().requires_grad_(True)
    with B.tapped() as tap:
        rgb, _, _, ex = render(H, W, focal, c2w=c2w, near=0., far=4., **kw)
    loss_of(rgb, ex).backward()
    joint = wgrads()
    assert c2w.grad is not None and float(c2w.grad.abs().max()) > 0
    for k, v in base.items():
        assert B.rel(joint[k], v) < 1e-6, k                              # (rays built from c2w in the kernels vs on the host: same values)
    # frozen weights, same pose: the generic backward-to-rays path
    clear()
    for m in nets:
        m.requires_grad_(False)
    c2w_f = c0.clone().requires_grad_(True)
    rgb, _, _, ex = render(H, W, focal, c2w=c2w_f, near=0., far=4., **kw)
    loss_of(rgb, ex).backward()
    # float64 oracle on the fine pass' branches and depths
    pin_c, pin = G.GenericPinned(tap, 0), G.GenericPinned(tap, 1)
    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni, perturb=0., test_time=False, transient_at_test=True, NeRFW=True)
    c64 = c0.cpu().double().clone().requires_grad_(True)
    with G.oracle_depth(6):
        rgb_r, _, _, ex_r = O.render(H, W, focal, G.oracle_params(coarse, torch.float64), G.oracle_params(fine, torch.float64), cfg,
                                     c2w=c64, near=0., far=4., coarse_act=pin_c.act(True), fine_act=pin.act(True), z_fine=pin.z_fine)
    loss_of(rgb_r, ex_r).backward()
    for pn in (pin_c, pin):
        flips, units, worst_pre = pn.summary()
        assert worst_pre < 2e-5 and flips <= max(8, units // 100000), (flips, units, worst_pre)
    B.three_way("generic_train_pose[64,6]", "d c2w, trainable weights [branch-pinned]", c2w.grad, c2w_f.grad, c64.grad)
