"""The folded fp16 field kernels (csrc/field_fwd_h3.hip / field_bwd_h3.hip FOLD; NefesNetDesc.fold_final; NeRFH_NFF.packed_folded):
xyz_encoding_final multiplied into dir_encoding / transient_encoding.0 by the packer, its W x W product gone from the fine pass of
frozen networks.  Every bound here is one the unfolded fp16 kernels are held to in tests/test_gpu_h3.py, test_gpu_parity.py and
test_gpu_shapes.py; the unfolded kernels' error on the same inputs is recorded beside the folded one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import parity_log as P
from tests.test_gpu_h3 import _net, _per_channel_err, _rays, _timer_keys

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "field_fwd[full,h3,fold]", "field_bwd[h3,fold]"


@pytest.fixture(autouse=True)
def _fp16_instances():
    from nefes_amd import ops
    old = ops.SPLIT, ops.USE_X6, ops.FOLD_FINAL
    ops.SPLIT, ops.USE_X6, ops.FOLD_FINAL = "h3", True, True
    yield
    ops.SPLIT, ops.USE_X6, ops.FOLD_FINAL = old


def _stress(net, o, z, case):
    with torch.no_grad():
        if case == "tiny_and_far":
            o[:16] *= 1e-4
            z[:16] *= 1e-4
            o[16:32] = o[16:32] * 30 + 5.
        elif case == "weights_1e3_1e-3":
            for i, f in zip(range(1, 9), (1e3, 1e-3, 1e3, 1e3, 1e-3, 1e-3, 1e3, 1e-3)):
                getattr(net, f"xyz_encoding_{i}")[0].weight.mul_(f)
                getattr(net, f"xyz_encoding_{i}")[0].bias.mul_(f if i > 1 else 1.)
            net.transient_encoding[2].weight.mul_(1e3)
            net.dir_encoding[0].weight.mul_(1e-2)
        elif case == "dead_layer":
            net.xyz_encoding_3[0].bias.fill_(-1e3)
        elif case == "final_2^10":
            net.xyz_encoding_final.weight.mul_(2.0 ** 10)
        elif case == "final_2^-10":
            net.xyz_encoding_final.weight.mul_(2.0 ** -10)
    net.invalidate_packed()


CASES = [(256, 16, 41, 24, "plain"), (256, 16, 300, 64, "plain"), (256, 128, 61, 32, "plain"), (256, 16, 129, 192, "plain"),
         (256, 128, 7, 33, "plain"), (256, 16, 1, 1, "plain"),
         (256, 16, 48, 32, "tiny_and_far"), (256, 16, 48, 32, "weights_1e3_1e-3"), (256, 16, 48, 32, "dead_layer"),
         (256, 128, 48, 32, "weights_1e3_1e-3"), (256, 128, 48, 32, "tiny_and_far"),
         (256, 16, 48, 32, "final_2^10"), (256, 16, 48, 32, "final_2^-10")]


@pytest.mark.parametrize("Wd,C,N,S,case", CASES)
def test_folded_forward_and_cross_fed_backward(Wd, C, N, S, case):
    """Raw outputs of the folded forward against the float64 oracle (rule of test_gpu_h3.py: max(3e-6, 3 e_ref) of the channel's scale,
    and no worse than 1.5 x the fp32-MFMA kernel on the stress sets), the unfolded kernel's error beside it; the sigma channel and the
    mask words of layers 1-8 bit-identical to the unfolded forward's; backward cross-fed -- folded forward state into the unfolded fp16
    and the strict-fp32 backward, unfolded state into the folded backward -- against the fp32-MFMA backward on the same state (the rule
    test_gpu_h3.py holds the fp16 backward to: 1e-5, 2e-5 on the stress sets)."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    net = _net("fine", Wd, C)
    o, d, z, g = _rays(N, S, 21 if case != "plain" else 9)
    _stress(net, o, z, case)
    pk, pkf = net.packed(), net.packed_folded()
    assert pkf.fold and not pk.fold and net.fold_ok()
    od, dd, zd = o.to(DEV), d.to(DEV), z.to(DEV)
    (hf, mf), keys = _timer_keys(lambda: ops.field_fwd_x6(pkf, L.FIELD_FULL, N, S, od, dd, zd, viewdirs=dd, want_masks=True))
    assert keys == {FWD}, keys
    (hu, mu), keys = _timer_keys(lambda: ops.field_fwd_x6(pk, L.FIELD_FULL, N, S, od, dd, zd, viewdirs=dd, want_masks=True))
    assert keys == {"field_fwd[full,h3]"}, keys
    f32, m32 = ops.field_fwd(pk, L.FIELD_FULL, N, S, rays_o=od, rays_d=dd, z=zd, viewdirs=dd, want_masks=True) if C == 16 else (None, None)
    assert torch.isfinite(hf).all()
    p = {k: v.detach().cpu().double() for k, v in net.named_parameters()}
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    ref = O.query_field(p, pts.double(), d.double(), "fine", True, True)
    ref32 = O.query_field({k: v.float() for k, v in p.items()}, pts, d, "fine", True, True)
    e_f, e_u, e_ref = _per_channel_err(hf, ref), _per_channel_err(hu, ref), _per_channel_err(ref32.permute(0, 2, 1), ref)
    e_f32 = _per_channel_err(f32, ref) if f32 is not None else 0.0
    bound = max(3e-6, 3 * e_ref) if case == "plain" else max(3e-6, 3 * e_ref, 1.5 * (e_f32 if f32 is not None else e_u))
    print(f"[fold/{Wd},{C},{N},{S},{case}] raw vs float64 (worst channel): folded {e_f:.2e}  unfolded {e_u:.2e}  fp32-MFMA {e_f32:.2e}  "
          f"torch fp32 {e_ref:.2e}  bound {bound:.2e}")
    P.record(f"fold_full[{Wd},{C},{N},{S},{case}]", "raw (worst channel)", e_hip=e_f, e_ref=e_ref, direct=e_u, bound=bound)
    assert e_f <= bound
    # same trunk, same arithmetic: sigma channel and the mask words of layers 1..8 bit for bit
    assert torch.equal(hf[:, 3 + C], hu[:, 3 + C])
    words, wt = 8 * (Wd // 64) + 4 * (Wd // 128), 8 * (Wd // 64)
    n32 = (N * S) // 32
    a, b = mf.view(-1, words, 64)[:n32], mu.view(-1, words, 64)[:n32]
    assert torch.equal(a[:, :wt], b[:, :wt])
    diff = int(sum(bin(int(v) & 0xffffffff).count("1") for v in (a[:, wt:] ^ b[:, wt:]).flatten().cpu().tolist() if v))
    print(f"[fold] head ReLU-mask bits differing from the unfolded kernel: {diff} of {a[:, wt:].numel() * 32}")
    assert diff <= max(4, a[:, wt:].numel() * 32 // 100000)
    # backward, cross-fed
    G = torch.randn(N, 9 + C, S, generator=g).to(DEV)
    tol = 1e-5 if case == "plain" else 2e-5
    bwd = lambda pack, raw, masks: ops.field_bwd(pack, N, S, raw, G, masks, rays_o=od, rays_d=dd, z=zd, viewdirs=dd)
    if C == 16:
        try:
            ops.SPLIT = "f32"
            (t_f, keys1) = _timer_keys(lambda: bwd(pk, hf, mf))              # folded forward -> strict-fp32 backward
            (t_u, keys2) = _timer_keys(lambda: bwd(pk, hu, mu))
        finally:
            ops.SPLIT = "h3"
        assert keys1 == keys2 == {"field_bwd"}
    else:                                                                   # (no fp32-MFMA instance at C = 128: the unfolded fp16 backward)
        t_f, t_u = bwd(pk, hf, mf), bwd(pk, hu, mu)
    (ff, keys) = _timer_keys(lambda: bwd(pkf, hf, mf))                      # folded -> folded
    assert keys == {BWD}, keys
    (fu, keys) = _timer_keys(lambda: bwd(pk, hf, mf))                       # folded forward -> unfolded fp16 backward
    assert keys == {"field_bwd[h3]"}, keys
    uf = bwd(pkf, hu, mu)                                                   # unfolded forward -> folded backward
    for got, want, name in ((ff, t_f, "folded->folded"), (fu, t_f, "folded->unfolded"), (uf, t_u, "unfolded->folded")):
        for x, y, what in zip(got, want, ("g_pts", "g_viewdirs")):
            assert torch.isfinite(x).all()
            e = float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
            print(f"[fold/{case}] backward {name} {what} vs {'fp32-MFMA' if C == 16 else 'unfolded fp16'} on the same state: {e:.2e}")
            P.record(f"fold_full[{Wd},{C},{N},{S},{case}]", f"backward {name} {what}", e_hip=e, e_ref=None, bound=tol)
            assert e < tol, (name, what)


@pytest.mark.parametrize("Wd,C", [(256, 16), (256, 128)])
def test_input_gradients_against_float64(Wd, C):
    """d raw -> d pts, d viewdirs of the folded pair (forward + backward) against float64 autograd through the oracle: within the 1e-5 tests/test_gpu_h3.py
    holds the fp16 backward to, a fixed bound that does not move with the unfolded kernels; their error on the same inputs is recorded beside it."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    N, S = 37, 24
    net = _net("fine", Wd, C)
    o, d, z, g = _rays(N, S, 33)
    G = torch.randn(N, 9 + C, S, generator=g)
    p = {k: v.detach().cpu().double() for k, v in net.named_parameters()}
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).double().requires_grad_()
    v64 = d.double().requires_grad_()
    ref = O.query_field(p, pts, v64, "fine", True, True)
    t_p, t_v = torch.autograd.grad((ref * G.permute(0, 2, 1).double()).sum(), (pts, v64))
    od, dd, zd, Gd = o.to(DEV), d.to(DEV), z.to(DEV), G.to(DEV)
    err = {}
    for name, pk in (("folded", net.packed_folded()), ("unfolded", net.packed())):
        raw, masks = ops.field_fwd_x6(pk, L.FIELD_FULL, N, S, od, dd, zd, viewdirs=dd, want_masks=True)
        g_pts, g_vs = ops.field_bwd(pk, N, S, raw, Gd, masks, rays_o=od, rays_d=dd, z=zd, viewdirs=dd)
        e_p = float((g_pts.view(N, S, 3).cpu().double() - t_p).abs().max() / t_p.abs().max())
        e_v = float((g_vs.view(N, S, 3).sum(1).cpu().double() - t_v).abs().max() / t_v.abs().max())
        err[name] = (e_p, e_v)
    print(f"[fold/{Wd},{C}] input gradients vs float64: folded d pts {err['folded'][0]:.2e} d viewdirs {err['folded'][1]:.2e}; "
          f"unfolded {err['unfolded'][0]:.2e} {err['unfolded'][1]:.2e}")
    for i, what in enumerate(("d pts", "d viewdirs")):
        P.record(f"fold_grad[{Wd},{C}]", what, e_hip=err["folded"][i], e_ref=None, direct=err["unfolded"][i], bound=1e-5)
        assert err["folded"][i] <= 1e-5


@pytest.mark.parametrize("which,tag", [("end_to_end", "metric"), ("end_to_end", "metric_B"), ("shapes", "w256c128"), ("shapes", "w256c128_B")])
def test_render_end_to_end_runs_the_folded_kernels(golden, which, tag):
    """The committed end-to-end cases at width 256 (frozen networks): render() takes the folded kernels and the existing rules hold --
    maps within 1e-4 of the reference fixture, d c2w under the branch-pinned three-way rule (tests/test_gpu_parity.py check_end_to_end)."""
    from tests.test_gpu_parity import check_end_to_end
    g = golden(which)
    if which == "end_to_end":
        Wd, C, Ni, tat, sscale, H, W, focal = g[f"{tag}.cfg"]
        run = lambda: check_end_to_end(g, tag, int(Wd), int(C), 64, int(Ni), bool(tat), float(sscale), int(H), int(W), float(focal))
    else:
        Wd, C, Nc, Ni, tat, H, W, focal = g[f"e2e.{tag}.cfg"]
        run = lambda: check_end_to_end(g, f"e2e.{tag}", int(Wd), int(C), int(Nc), int(Ni), bool(tat), 1.0, int(H), int(W), float(focal))
    assert int(Wd) == 256
    _, keys = _timer_keys(run)
    assert {FWD, BWD} <= keys and not {"field_fwd[full,h3]", "field_bwd[h3]"} & keys, sorted(keys)


def _render(fine, coarse, grad=True):
    import types
    from nefes_amd.render import render
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, netchunk=1 << 21)
    kw = dict(network_query_fn=None, perturb=False, N_importance=32, N_samples=16, network_fn=coarse, network_fine=fine,
              use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False, lindisp=False)
    c2w = O.bench_pose().to(DEV).requires_grad_(grad)

    def run():
        rgb, disp, acc, ex = render(6, 8, 8 * 525.505 / 640., c2w=c2w, near=0., far=4., **kw)
        if grad:
            (gc,) = torch.autograd.grad(O.bench_loss(rgb, ex["feat_map"]), c2w)
            return rgb.detach(), ex["feat_map"].detach(), gc
        return rgb.detach(), ex["feat_map"].detach(), None
    return _timer_keys(run)


def test_routing_follows_requires_grad_and_weight_edits():
    """Decided per render: a frozen network takes the folded kernels; one trainable field parameter sends the next render to the
    train-mode instances (never the fold) and, without autograd, to the unfolded inference kernels; frozen again, folded again.  An
    in-place weight edit re-folds: the next render equals a fresh network's with the edited weights."""
    from nefes_amd.field import NeRFH_NFF
    coarse, fine = _net("coarse"), _net("fine")
    (rgb0, feat0, g0), keys = _render(fine, coarse)
    assert {FWD, BWD} <= keys, sorted(keys)
    for rep in range(2):
        fine.xyz_encoding_final.bias.requires_grad_(True)
        assert not fine.fold_ok()
        _, keys = _render(fine, coarse)
        assert not any("fold" in k for k in keys) and not {"field_fwd[full,h3]", "field_bwd[h3]"} & keys, sorted(keys)   # train-mode instances
        with torch.no_grad():
            _, keys = _render(fine, coarse, grad=False)
        assert "field_fwd[full,h3]" in keys and not any("fold" in k for k in keys), sorted(keys)
        fine.requires_grad_(False)
        (rgb1, feat1, g1), keys = _render(fine, coarse)
        assert {FWD, BWD} <= keys, sorted(keys)
        assert torch.equal(rgb1, rgb0) and torch.equal(feat1, feat0) and torch.equal(g1, g0)
    pk_before = fine.packed_folded()
    with torch.no_grad():
        fine.xyz_encoding_final.weight.mul_(1.25)
        fine.dir_encoding[0].bias.add_(0.05)
    (rgb2, feat2, g2), keys = _render(fine, coarse)
    assert {FWD, BWD} <= keys and fine.packed_folded() is not pk_before
    assert float((feat2 - feat0).abs().max()) > 1e-4
    fresh = NeRFH_NFF('fine', W=256, f_dim=16, encode_appearance=True, encode_transient=True).requires_grad_(False).to(DEV)
    fresh.load_state_dict(fine.state_dict())
    (rgb3, feat3, g3), _ = _render(fresh, coarse)
    assert torch.equal(rgb2, rgb3) and torch.equal(feat2, feat3) and torch.equal(g2, g3)
    with pytest.raises(RuntimeError):
        fine.packed_folded().repack([])                                 # a folded pack is never refreshed by the device re-pack


def test_train_mode_never_takes_the_fold(golden):
    """A trainable network's results are the ones train.npz pins (tests/test_gpu_shapes.py test_train_mode_vs_reference_golden at
    width 256), with the fold enabled and no folded kernel in its timers."""
    from tests.test_gpu_shapes import test_train_mode_vs_reference_golden as run
    _, keys = _timer_keys(lambda: run(golden, "w256c128"))
    assert keys and not any("fold" in k for k in keys), sorted(keys)


def test_environment_switch_selects_the_unfolded_kernels():
    """NEFES_FOLD_FINAL=0 (read once at import): the same render runs on the unfolded kernels' timer keys."""
    code = ("import torch, sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_fold import _render\nfrom tests.test_gpu_h3 import _net\n"
            "_, keys = _render(_net('fine'), _net('coarse'))\nprint('KEYS', sorted(keys))\n" % ROOT)
    out = {}
    for val in ("0", "1"):
        env = dict(os.environ, NEFES_FOLD_FINAL=val, NEFES_PARITY_LOG=os.devnull)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[val] = next(l for l in r.stdout.splitlines() if l.startswith("KEYS"))
    assert "field_fwd[full,h3]" in out["0"] and "field_bwd[h3]" in out["0"] and "fold" not in out["0"], out["0"]
    assert FWD in out["1"] and BWD in out["1"], out["1"]


def test_graph_replay_and_two_streams_on_a_256_16_network(golden):
    """A (256, 16) PoseRefiner on the folded kernels: iterations replayed from a captured graph give the eager run's poses and losses bit
    for bit, and two refiners on two streams walk their solo trajectories (what tests/test_gpu_refine.py / test_gpu_streams.py demand
    of the unfolded kernels on the width-128 fixtures)."""
    from nefes_amd.refine import refine_concurrently
    from tests.test_gpu_refine import T, refiner
    g = dict(golden("refine"))
    g["Wd"], g["C"] = np.int64(256), np.int64(16)
    n = 6
    out = {}
    target = None                                   # (the fixture's feature target has the width-128 network's 128 channels)
    for graph in (False, True):
        ref = refiner(g, graph=graph)
        assert ref.kw["network_fine"].fold_ok()
        if target is None:
            target = torch.randn(tuple(ref.target.shape), generator=torch.Generator().manual_seed(3))
        (pose, losses), keys = _timer_keys(lambda: ref.refine(T(g["init_c2w"]), target, T(g["hist"]), n))
        if not graph:
            assert {FWD, BWD} <= keys, sorted(keys)
        out[graph] = (pose.clone(), losses.clone())
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])
    refs = [refiner(g, graph=True), refiner(g, graph=True)]
    init2 = T(g["init_c2w"]).clone()
    init2[:3, 3] += 0.02
    jobs = [(T(g["init_c2w"]), target, T(g["hist"])), (init2, target, T(g["hist"]))]
    solo = [tuple(x.clone() for x in r.refine(*job, iters=n)) for r, job in zip(refs, jobs)]
    for rep in range(2):
        outs = refine_concurrently(refs, jobs, iters=n)
        torch.cuda.synchronize()
        for (p, l), (ps, ls) in zip(outs, solo):
            assert torch.equal(p, ps) and torch.equal(l, ls), rep
    assert not torch.equal(solo[0][0], solo[1][0])
