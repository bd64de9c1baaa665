"""Training FusionNet on the library's kernels (ops.FUSION_TRAIN, opt-in): the convolutions' weight / bias gradients (csrc/conv.hip
conv2d_wgrad), BatchNorm's affine gradients (csrc/refine.hip bn_train_bwd_affine), the whole net against the reference's fixture
(tests/golden/fusion_train.npz through the oracle that tests/test_fusion_train_golden.py pins on it) and a stage-3 step through render().

Truth is float64 on the CPU, evaluated on the HIP forward's own ReLU pattern (tests/branch.py's rule); the bound is tests/parity_log.py's
max(tol, 1.5 e_ref), e_ref = the fp32 CPU evaluation's distance from float64 on the same inputs and pattern."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from oracle import refine_cpu as RC
from tests import branch as B
from tests import parity_log as P
from tests import test_fusion_train_golden as G
from tests.test_conv_train_args import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
rel = B.rel


def _conv_case(Bn, Cin, Cout, k, H, W):
    g = torch.Generator().manual_seed(Bn * 1000 + Cin + k)
    x = torch.randn(Bn, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    gy = torch.randn(Bn, Cout, H, W, generator=g)
    return x, w, b, gy


def _conv_ref(x, w, b, gy, k, pos, dt, dev):
    """y, d x, d w, d b of (y * gy).sum(), y = conv2d(x, w, b) [times the given ReLU pattern], torch autograd in dtype dt on dev."""
    xx, ww, bb = (t.to(dev, dt).requires_grad_() for t in (x, w, b))
    y = F.conv2d(xx, ww, bb, padding=k // 2)
    if pos is not None:
        y = y * pos.to(dev, dt)
    gx, gw, gb = torch.autograd.grad((y * gy.to(dev, dt)).sum(), [xx, ww, bb])
    return {"y": y.detach().cpu().double(), "d x": gx.cpu().double(), "d w": gw.cpu().double(), "d b": gb.cpu().double()}


# ---- 1. one layer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,Cin,Cout,k,relu,H,W", SHAPES)
def test_conv_train_matches_float64(Bn, Cin, Cout, k, relu, H, W):
    """ops.conv2d_same_train: output, input, weight and bias gradient against torch's convolution in float64 on the CPU, on the HIP
    forward's ReLU pattern; e_ref = torch's fp32 CPU convolution on the same pattern.  MIOpen's fp32 result on the GPU is recorded
    beside it, not asserted.  Shapes: odd Cin, channel counts that are no multiple of 32 (131, 19, 16, 7, 5, 3, 1), Cout one past a
    tile (33), pixel counts that are no multiple of the 256-pixel chunk or of 32, 35-pixel images (chunks meet image borders inside
    a chunk), 16 x 16 images (one chunk = one image: borders ON chunk borders), an image smaller than the 5 x 5 kernel."""
    from nefes_amd import ops
    x, w, b, gy = _conv_case(Bn, Cin, Cout, k, H, W)
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    y = ops.conv2d_same_train(xd, wd, bd, relu=relu)
    (y * gy.to(DEV)).sum().backward()
    got = {"y": y.detach(), "d x": xd.grad, "d w": wd.grad, "d b": bd.grad}
    assert wd.grad.shape == w.shape and bd.grad.shape == b.shape
    pos = (y.detach() > 0).cpu() if relu else None
    r64, r32 = _conv_ref(x, w, b, gy, k, pos, torch.float64, "cpu"), _conv_ref(x, w, b, gy, k, pos, torch.float32, "cpu")
    mi = _conv_ref(x, w, b, gy, k, pos, torch.float32, DEV)
    tag = f"conv_train[{Bn},{Cin},{Cout},{k},{H}x{W}]"
    for name in ("y", "d x", "d w", "d b"):
        e_hip, e_ref, e_mi = rel(got[name], r64[name]), rel(r32[name], r64[name]), rel(mi[name], r64[name])
        print(f"[{tag}] {name}: hip {e_hip:.2e}  torch fp32 cpu {e_ref:.2e}  MIOpen fp32 {e_mi:.2e}")
        P.record(tag, name + " vs float64: MIOpen fp32 on the GPU (measured, not asserted)", e_hip=e_mi, e_ref=e_ref, bound=None)
        P.check(tag, name + " vs float64 [branch-pinned]", e_hip, e_ref, tol=1e-5)


# ---- 2. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,Cin,Cout,k,relu,H,W", [SHAPES[3], SHAPES[5]])
def test_wgrad_is_bit_identical_and_overwrites(Bn, Cin, Cout, k, relu, H, W):
    """Two calls on the same inputs return the same bits; output buffers and workspace pre-filled with NaN change nothing: the kernels
    overwrite g_w / g_bias and read of the workspace only what they wrote in this call."""
    import ctypes as C
    from nefes_amd import lib as L
    from nefes_amd import ops
    x, w, b, gy = _conv_case(Bn, Cin, Cout, k, H, W)
    xd, gyd = x.to(DEV), gy.to(DEV)
    mask = torch.relu(torch.randn(Bn, Cout, H, W, generator=torch.Generator().manual_seed(5))).to(DEV) if relu else None
    gw1, gb1 = ops._conv2d_wgrad(xd, gyd, mask, Cout, k, True)
    gw2, gb2 = ops._conv2d_wgrad(xd, gyd, mask, Cout, k, True)
    assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2) and bool(torch.isfinite(gw1).all()) and float(gw1.abs().max()) > 0
    lib = L.load()
    nbytes = lib.nefes_conv2d_wgrad_workspace(Bn, Cin, Cout, H, W, k)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    gw3, gb3 = torch.full_like(gw1, float("nan")), torch.full_like(gb1, float("nan"))
    L.check(lib.nefes_conv2d_wgrad(Bn, Cin, Cout, H, W, k, xd.data_ptr(), gyd.data_ptr(), None if mask is None else mask.data_ptr(),
                                   gw3.data_ptr(), gb3.data_ptr(), ws.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "nefes_conv2d_wgrad")
    assert torch.equal(gw1, gw3) and torch.equal(gb1, gb3)
    gw4, none = ops._conv2d_wgrad(xd, gyd, mask, Cout, k, False)              # no bias gradient asked for
    assert none is None and torch.equal(gw1, gw4)


# ---- 3. BatchNorm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,C,H,W", [(3, 7, 5, 9), (7, 128, 16, 16)])
def test_batch_norm_train_with_trainable_affine_matches_torch_in_float64(Bn, C, H, W):
    """ops.batch_norm_train == torch.nn.BatchNorm2d in train mode in float64: output, d x, d weight, d bias, running statistics
    (unbiased variance) and the batch counter after two calls.  Bounds: test_batch_norm_train_kernels_match_torch_in_float64's."""
    import copy
    from nefes_amd import ops
    g = torch.Generator().manual_seed(Bn * C + H)
    x = torch.randn(Bn, C, H, W, generator=g) * 2.0 + 0.3
    Gy = torch.randn(Bn, C, H, W, generator=g)
    bn64 = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn64.weight.copy_(torch.randn(C, generator=g).double())
        bn64.bias.copy_(torch.randn(C, generator=g).double())
    bn = copy.deepcopy(bn64).float().to(DEV).train()
    for rep in range(2):
        bn64.zero_grad(), bn.zero_grad()
        xd = x.double().requires_grad_()
        (bn64(xd) * Gy.double()).sum().backward()
        xh = x.to(DEV).requires_grad_()
        yh = ops.batch_norm_train(xh, bn)
        (yh * Gy.to(DEV)).sum().backward()
        e = {"y": rel(yh, _bn_out(bn64, x)),
             "d x": rel(xh.grad, xd.grad), "d weight": rel(bn.weight.grad, bn64.weight.grad), "d bias": rel(bn.bias.grad, bn64.bias.grad)}
        print(rep, {k_: f"{v:.1e}" for k_, v in e.items()})
        assert e["y"] < 1e-6 and e["d x"] < 2e-6 and e["d weight"] < 2e-6 and e["d bias"] < 2e-6, (rep, e)
    P.record(f"batch_norm_train_affine[{Bn},{C},{H},{W}]", "output / d x / d weight / d bias vs float64 torch", e_hip=max(e.values()), e_ref=None,
             direct=max(e.values()), bound=2e-6)
    assert int(bn.num_batches_tracked) == 2 == int(bn64.num_batches_tracked)
    assert rel(bn.running_mean, bn64.running_mean) < 1e-6 and rel(bn.running_var, bn64.running_var) < 1e-6
    # the input carries no gradient: the parameters' gradients alone
    bn.zero_grad()
    (ops.batch_norm_train(x.to(DEV), bn, track_stats=False) * Gy.to(DEV)).sum().backward()
    assert rel(bn.weight.grad, bn64.weight.grad) < 2e-6 and rel(bn.bias.grad, bn64.bias.grad) < 2e-6 and int(bn.num_batches_tracked) == 2


def _bn_out(bn64, x):
    """Train-mode output of bn64 on x in float64 without touching its running statistics."""
    return F.batch_norm(x.double(), None, None, bn64.weight.detach(), bn64.bias.detach(), True, 0.0, bn64.eps)


# ---- 4. the whole net against the reference's fixture -----------------------------------------------------------------------------------------
def _fusion_net_from_fixture(g):
    from nefes_amd.field import FusionNet
    net = FusionNet(G.C)
    net.load_state_dict({k: g["param." + k] for k in G.PARAMS}, strict=False)
    return net.to(DEV).train()


def _graph_nodes(t):
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo += [n for n, _ in f.next_functions]
    return names


def test_fusion_net_trains_on_the_kernels_against_the_reference_fixture(monkeypatch):
    from nefes_amd import ops
    g = G.load()
    net = _fusion_net_from_fixture(g)
    Bn, H, W, C = G.B, G.H, G.W, G.C
    target = g["target"].to(DEV)

    def run(entry="parts"):
        net.zero_grad()
        rgb, feat = g["rgb"].detach().to(DEV).requires_grad_(), g["feat"].detach().to(DEV).requires_grad_()
        r, f = rgb.reshape(Bn, H, W, 3).permute(0, 3, 1, 2), feat.reshape(Bn, H, W, C).permute(0, 3, 1, 2)
        fused = net.forward_parts(r, f) if entry == "parts" else net(torch.cat([r, f], 1))
        F.l1_loss(fused, target).backward()
        out = {"fused": fused.detach(), "d_rgb": rgb.grad, "d_feat": feat.grad}
        out.update({"grad." + k: p.grad.clone() for k, p in net.net.named_parameters(prefix="net")})
        return fused, out

    # the switch off: today's behaviour, torch's layers
    monkeypatch.setattr(ops, "FUSION_TRAIN", False)
    monkeypatch.setattr(ops, "TIMERS", {})
    fused, off = run()
    assert "conv2d_same" not in ops.TIMERS and "conv2d_wgrad" not in ops.TIMERS
    assert sum(n.startswith("ConvolutionBackward") for n in _graph_nodes(fused)) == 4
    # ... and on
    with torch.no_grad():
        net.net[7].running_mean.zero_(), net.net[7].running_var.fill_(1.0), net.net[7].num_batches_tracked.zero_()
    monkeypatch.setattr(ops, "FUSION_TRAIN", True)
    monkeypatch.setattr(ops, "TIMERS", {})
    with B.tapped() as tap:
        fused, got = run()
    assert len(ops.TIMERS["conv2d_wgrad"]) == 4 and len(ops.TIMERS["conv2d_same"]) == 8, {k: len(v) for k, v in ops.TIMERS.items()}
    nodes = _graph_nodes(fused)
    assert not any("Convolution" in n or "NativeBatchNorm" in n for n in nodes), nodes
    assert sum(n == "TrainConv2dBackward" for n in nodes) == 4 and sum(n == "BatchNormTrainBackward" for n in nodes) == 1, nodes
    bn = net.net[7]
    assert int(bn.num_batches_tracked) == 1
    assert rel(bn.running_mean, g["buffer.net.7.running_mean"]) < 1e-5 and rel(bn.running_var, g["buffer.net.7.running_var"]) < 1e-5
    conv_pos, aud = [(y > 0).cpu() for y in tap["conv_relu"][-3:]], {}
    t64, t32 = G.oracle_run(g, torch.float64, conv_pos, aud), G.oracle_run(g, torch.float32, conv_pos)
    print("relu pattern vs float64:", aud)
    assert aud.get("worst", 0.0) < B.AUDIT_CLASSES["same_inputs"] and aud.get("flips", 0) <= 8, aud
    assert set(got) == set(t64) and len(got) == 13
    for name in got:
        B.three_way("fusion_train[fixture]", name + " [branch-pinned]", got[name], t32[name], t64[name], scale=G.scale_of(name, g))
        # ... and, loosely, the reference's own fp32 arrays (its own ReLU pattern: a handful of units within rounding of zero may differ)
        assert rel(got[name], g[name], G.scale_of(name, g)) < 2e-2, name
    # forward(x), the reference's entry with its in-place colour normalisation: the same launches on the same values
    _, got2 = run("forward")
    for name in got:
        assert rel(got2[name], got[name], G.scale_of(name, g)) < 1e-6, name
    # the other two architectures the reference can build
    for kw in (dict(fusion_residule=True), dict(no_BN=True)):
        _check_variant(kw, g, monkeypatch)


def _check_variant(kw, g, monkeypatch):
    """fusion_residule / no_BN on the kernels == the same module on torch's layers in float64 on the CPU, ReLU pattern pinned by hooks."""
    import copy
    from nefes_amd import ops
    from nefes_amd.field import FusionNet
    Bn, H, W, C = G.B, G.H, G.W, G.C
    torch.manual_seed(3)
    net = FusionNet(C, **kw).to(DEV).train()
    net64 = copy.deepcopy(net).cpu().double()
    r = g["rgb"].reshape(Bn, H, W, 3).permute(0, 3, 1, 2).contiguous()
    f = g["feat"].reshape(Bn, H, W, C).permute(0, 3, 1, 2).contiguous()
    monkeypatch.setattr(ops, "TIMERS", {})
    with B.tapped() as tap:
        rd, fd = r.to(DEV).requires_grad_(), f.to(DEV).requires_grad_()
        F.l1_loss(net.forward_parts(rd, fd), g["target"].to(DEV)).backward()
    assert len(ops.TIMERS["conv2d_wgrad"]) == 4
    pos = [(y > 0).cpu() for y in tap["conv_relu"][-3:]]
    hooks = [net64.net[i].register_forward_hook(lambda m, a, out, p=p: a[0] * p.double()) for i, p in zip((1, 3, 5), pos)]
    r64, f64 = r.double().requires_grad_(), f.double().requires_grad_()
    F.l1_loss(net64.forward_parts(r64, f64), g["target"].double()).backward()
    for h in hooks:
        h.remove()
    assert rel(rd.grad, r64.grad) < 1e-4 and rel(fd.grad, f64.grad) < 1e-4, kw
    for (n, p), p64 in zip(net.named_parameters(), net64.parameters()):
        # (the bias in front of a BatchNorm has a gradient of zero: tests/test_fusion_train_golden.py cancelling_scale; the weight
        #  gradient of its layer is a generous unit here, 1e-5 of it what the reference's own fp32 residue measured)
        scale = float(net64.net[6].weight.grad.abs().max()) if n == "net.6.bias" and not net.no_BN else None
        assert rel(p.grad, p64.grad, scale) < 1e-4, (kw, n)


# ---- 5. a stage-3 step through render() ------------------------------------------------------------------------------------------------------
def test_stage3_step_through_render(monkeypatch):
    """render() in train mode (everything trainable) -> run_fusion_net on two 6 x 8 patches -> mse(rgb) + L1(fused): (a) the gradient
    that reaches the rendered maps and the fusion parameters against the float64 oracle from the maps on; (b) the NeRF weights receive
    exactly that gradient (the same autograd graph fed with the float64 d rgb / d feat_map); (c) two Adam steps re-pack the
    convolutions."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    from nefes_amd.field import FusionNet, NeRFH_NFF
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "FUSION_TRAIN", True)
    Wd, C, H, W, focal, Nc, Ni, Bn = 128, 16, 6, 8, 9.0, 64, 64, 2
    coarse = NeRFH_NFF('coarse', W=Wd, f_dim=C).to(DEV)
    fine = NeRFH_NFF('fine', W=Wd, f_dim=C, encode_appearance=True, encode_transient=True).to(DEV)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True)
    kw = dict(network_query_fn=None, perturb=0., N_importance=Ni, N_samples=Nc, network_fn=coarse, network_fine=fine,
              use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=False, args=args, ndc=False, lindisp=False)
    poses = [O.bench_pose(), O.se3_exp_pose((0.05, 0.15, -0.10), (-0.20, 0.10, 0.25), torch.float32)]
    rays = [O.ray_bundle(H, W, focal, p) for p in poses]
    rays_o = torch.cat([r[0].reshape(-1, 3) for r in rays]).to(DEV)
    rays_d = torch.cat([r[1].reshape(-1, 3) for r in rays]).to(DEV)
    gen = torch.Generator().manual_seed(8)
    t_rgb, t_fused = torch.rand(Bn * H * W, 3, generator=gen), torch.randn(Bn, C, H, W, generator=gen)

    def loss_of(rgb, fused):
        return ((rgb - t_rgb.to(rgb)) ** 2).mean() + F.l1_loss(fused, t_fused.to(rgb))

    def step():
        rgb, _, _, ex = render(Bn * H, W, focal, rays=(rays_o, rays_d), near=0., far=4., **kw)
        _, _, fused = coarse.run_fusion_net(rgb, ex["feat_map"], H, W, Bn)
        return rgb, ex["feat_map"], fused

    monkeypatch.setattr(ops, "TIMERS", {})
    with B.tapped() as tap:
        rgb, feat, fused = step()
    assert rgb.shape == (96, 3) and feat.shape == (96, C) and fused.shape == (Bn, C, H, W)
    rgb.retain_grad(), feat.retain_grad()
    loss = loss_of(rgb, fused)
    # (a) the oracle from the rendered maps on, on the kernels' ReLU pattern
    conv_pos, aud = [(y > 0).cpu() for y in tap["conv_relu"][-3:]], {}
    fsd = {k: v.detach().cpu() for k, v in coarse.fusion_net.state_dict().items() if k in G.PARAMS}

    def oracle(dt, audit=None):
        leaf = lambda t: t.detach().cpu().to(dt).clone().requires_grad_()
        sd = {k: leaf(v) for k, v in fsd.items()}
        r, f = leaf(rgb), leaf(feat)
        fu = RC.fusion_net(sd, r, f, H, W, Bn, conv_pos=conv_pos, audit=audit)
        gr = torch.autograd.grad(loss_of(r, fu), [r, f] + [sd[k] for k in G.PARAMS])
        out = {"fused": fu.detach(), "d rgb": gr[0], "d feat_map": gr[1]}
        out.update({"grad." + k: v for k, v in zip(G.PARAMS, gr[2:])})
        return out
    t64, t32 = oracle(torch.float64, aud), oracle(torch.float32)
    assert aud.get("worst", 0.0) < B.AUDIT_CLASSES["same_inputs"] and aud.get("flips", 0) <= 8, aud
    nerf = [(n, p) for net, mode in ((coarse, L.FIELD_STATIC), (fine, L.FIELD_FULL)) for n, p in net.named_parameters()
            if n in TR.param_names(net, mode)]
    loss.backward(retain_graph=True)
    assert len(ops.TIMERS["conv2d_wgrad"]) == 4
    got = {"fused": fused.detach(), "d rgb": rgb.grad.clone(), "d feat_map": feat.grad.clone()}      # (before the second pass below)
    fed = torch.autograd.grad([rgb, feat], [p for _, p in nerf], [t64["d rgb"].float().to(DEV), t64["d feat_map"].float().to(DEV)],
                              allow_unused=True)
    got.update({"grad." + k: p.grad for k, p in coarse.fusion_net.net.named_parameters(prefix="net")})
    cancel = G.cancelling_scale(fsd, rgb.cpu(), feat.cpu(), H, W, Bn, lambda y: F.l1_loss(y, t_fused.double()), conv_pos)
    e_ref_a = 0.0
    for name in got:
        _, e_ref, _ = B.three_way("fusion_train[stage3]", name + " [branch-pinned]", got[name], t32[name], t64[name],
                                  scale=cancel if name == "grad.net.6.bias" else None)
        if name in ("d rgb", "d feat_map"):
            e_ref_a = max(e_ref_a, e_ref)
    # (b) the field's train-mode backward received what the new kernels produced.  Parameters the loss does not reach (the coarse field:
    # the loss has no rgb0 term and the sampler detaches; heads this loss does not read) have no gradient on either side.
    reached = 0
    for (n, p), ref in zip(nerf, fed):
        if ref is None or float(ref.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
        P.check("fusion_train[stage3]", f"{n}.grad vs the graph fed with the float64 d rgb / d feat_map", rel(p.grad, ref), e_ref_a)
        reached += 1
    assert reached >= 24, reached
    # (c) two Adam steps over everything, then a third forward: a stale convolution pack would show
    opt = torch.optim.Adam([*coarse.parameters(), *fine.parameters()], lr=1e-3)
    before = {k: v.clone() for k, v in coarse.fusion_net.state_dict().items()}
    for i in range(2):
        if i:
            rgb, feat, fused = step()
            loss_of(rgb, fused).backward()
        opt.step()
        opt.zero_grad()
    assert all(not torch.equal(before[k], v) for k, v in coarse.fusion_net.state_dict().items() if k.endswith(("weight", "bias")))
    rgb, feat, fused = step()
    fresh = FusionNet(C).to(DEV).train()
    sd = {k: v.clone() for k, v in coarse.fusion_net.state_dict().items()}
    fresh.load_state_dict(sd)
    r, f = rgb.detach().reshape(Bn, H, W, 3).permute(0, 3, 1, 2), feat.detach().reshape(Bn, H, W, C).permute(0, 3, 1, 2)
    assert rel(fused, fresh.forward_parts(r, f)) < 1e-6


# ---- 6. refusals and unchanged paths ------------------------------------------------------------------------------------------------------------
def test_refusals_and_unchanged_paths(monkeypatch):
    from nefes_amd import ops
    from nefes_amd.field import FusionNet
    monkeypatch.setattr(ops, "FUSION_TRAIN", True)
    x = torch.randn(1, 19, 6, 8, device=DEV)
    conv = torch.nn.Conv2d(19, 64, 3, 1, 1).to(DEV)
    with pytest.raises(ValueError, match="frozen_conv2d"):
        ops.frozen_conv2d(x, conv.weight, conv.bias, relu=True)
    bn = torch.nn.BatchNorm2d(19).to(DEV).train()
    with pytest.raises(ValueError, match="batch_norm_train_frozen"):
        ops.batch_norm_train_frozen(x, bn)
    torch.manual_seed(1)
    net = FusionNet(16).to(DEV).train()
    with pytest.raises(RuntimeError, match="forward_prepared_gmap"):
        net.forward_prepared_gmap(torch.randn(1, 3 + 8 + 1, 6, 8, device=DEV), torch.randn(16, 8, device=DEV), torch.randn(16, device=DEV))
    # per-image statistics with trainable affine parameters: the BatchNorm stays on torch, the convolutions take the kernels
    monkeypatch.setattr(ops, "TIMERS", {})
    xb = torch.randn(2, 19, 6, 8, device=DEV)
    y = net.forward_prepared(xb, per_image_norm=True)
    assert len(ops.TIMERS["conv2d_same"]) == 4 and type(y.grad_fn).__name__ != "BatchNormTrainBackward"
    # frozen weights: the switch changes nothing
    net.requires_grad_(False)
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "FUSION_TRAIN", on)
        xg = xb.clone().requires_grad_()
        with torch.no_grad():
            net.net[7].running_mean.zero_(), net.net[7].running_var.fill_(1.0)
        y = net.forward_prepared(xg)
        (y * y).sum().backward()
        outs[on] = (y.detach().clone(), xg.grad.clone(), type(y.grad_fn).__name__)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1]) and outs[True][2] == outs[False][2]
