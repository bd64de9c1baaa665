"""Generic field kernels on the GPU (nefes_amd/csrc/field_generic.hip): any --netwidth / --netdepth at test time.

Fixture tests/golden/generic.npz (tools/make_golden_generic.py: the reference's own render() at every shape); gradients three-way
against the float64 oracle on the kernels' own ReLU branches (tests/generic_util.py decodes the generic mask words); the generic
kernels against the tuned fp16 two-part ones on the same weights (NEFES_FIELD_GENERIC=1 in a child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import generic_util as G
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.asarray(a)).float()


def _case(g, tag):
    Wd, D, C, Nc, Ni, H, W, focal, in_xyz, in_dir = g[f"gen.{tag}.cfg"]
    return int(Wd), int(D), int(C), int(Nc), int(Ni), int(H), int(W), float(focal), int(in_xyz), int(in_dir)


def test_generic_network_renders_through_the_dropin():
    """A (64, 6) network through models.rendering.render: raised RuntimeError before the generic kernels existed."""
    sys.path.insert(0, os.path.join(ROOT, "nefes_amd", "dropin"))
    from models.rendering import render
    coarse, fine = G.modules(64, 6, 16, device=DEV)
    kw = G.render_kwargs(coarse, fine, 64, 64)
    rgb, disp, acc, ex = render(4, 6, 525.505 * 6 / 640., c2w=O.bench_pose().to(DEV), near=0., far=4., **kw)
    assert rgb.shape == (24, 3) and ex["feat_map"].shape == (24, 16)
    assert all(bool(torch.isfinite(t).all()) for t in (rgb, disp, acc, ex["feat_map"]))


@pytest.mark.parametrize("tag", G.CASES)
def test_render_vs_reference_and_pose_gradient(golden, tag):
    """Maps within 1e-4 of the reference's (the gate of tests/test_gpu_parity.py); d loss / d c2w three-way against the float64 oracle
    on the kernels' own ReLU branches and depths, e_hip <= max(1e-4, 1.5 e_ref)."""
    from nefes_amd.render import render
    g = golden("generic")
    Wd, D, C, Nc, Ni, H, W, focal, in_xyz, in_dir = _case(g, tag)
    coarse, fine = G.modules(Wd, D, C, in_xyz, in_dir)
    for typ, m in (("coarse", coarse), ("fine", fine)):             # the seed reproduces the reference's parameters
        for k, v in m.state_dict().items():
            key = f"gen.{tag}.sum.{typ}.{k}"
            if key in g:
                np.testing.assert_allclose(np.array([v.double().sum().item(), v.double().abs().sum().item(), float(v.flatten()[0])]),
                                           g[key], rtol=0, atol=0, err_msg=key)
    assert fine.uses_generic() and coarse.uses_generic()
    coarse, fine = coarse.to(DEV), fine.to(DEV)
    kw = G.render_kwargs(coarse, fine, Nc, Ni)
    c2w = T(g[f"gen.{tag}.c2w"]).to(DEV).requires_grad_()
    with B.tapped() as tap:
        rgb, disp, acc, ex = render(H, W, focal, c2w=c2w, near=0., far=4., **kw)
    feat = ex["feat_map"]
    name = f"generic_render[{tag}]"
    errs = {"rgb": B.rel(rgb, g[f"gen.{tag}.rgb"]), "feat": B.rel(feat, g[f"gen.{tag}.feat"]), "disp": B.rel(disp, g[f"gen.{tag}.disp"]),
            "acc": B.rel(acc, g[f"gen.{tag}.acc"])}
    for k, e in errs.items():
        print(f"[{name}] {k} vs reference fixture: {e:.2e}")
        P.record(name, f"{k} vs reference fixture", e_hip=e, e_ref=None, bound=P.NORTH_STAR_TOL)
    ((feat ** 2).mean() + (rgb ** 2).mean()).backward()
    P.record(name, "d c2w vs the reference's fp32 gradient [unpinned]", e_hip=B.rel(c2w.grad.cpu(), g[f"gen.{tag}.g_c2w_loss"][:3]), e_ref=None,
             bound=None)
    assert all(e < P.NORTH_STAR_TOL for e in errs.values()), errs

    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni, n_freq_xyz=(in_xyz - 3) // 6, n_freq_dir=(in_dir - 3) // 6)

    def oracle_run(dt, act, zf):
        c = T(g[f"gen.{tag}.c2w"]).to(dt).requires_grad_()
        with G.oracle_depth(D):
            r, _, _, e = O.render(H, W, focal, G.oracle_params(coarse, dt), G.oracle_params(fine, dt), cfg, c2w=c[:3, :4], near=0., far=4.,
                                  fine_act=act, z_fine=zf)
        return {"d c2w": torch.autograd.grad((e["feat_map"] ** 2).mean() + (r ** 2).mean(), c)[0]}

    G.pinned_gradients_generic(name, {"d c2w": c2w.grad}, tap, oracle_run)


def _field_inputs(N, S, R, seed=23):
    gen = torch.Generator().manual_seed(seed)
    o = (torch.rand(N, 3, generator=gen) - .5)
    d = torch.randn(N, 3, generator=gen)
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(N, S, generator=gen) * 4, -1)[0]
    return o, d, v, z, torch.randn(N, S, R, generator=gen)


def _oracle_field(params, D, o, d, v, z, g_raw, dt, typ, transient, act=None, sigma=False):
    oo, dd, vv = (t.to(dt).clone().requires_grad_() for t in (o, d, v))
    pts = oo[:, None, :] + dd[:, None, :] * z.to(dt)[..., None]
    with G.oracle_depth(D):
        raw = O.query_field({k: w.to(dt) for k, w in params.items()}, pts, vv, typ, transient, sigma, act=act)
    if g_raw is None:
        return raw.detach(), None
    raw.backward(g_raw.to(dt))
    return raw.detach(), {"d rays_o": oo.grad, "d rays_d": dd.grad, "d viewdirs": vv.grad}


@pytest.mark.parametrize("Wd,D,C,N,S", [(64, 6, 16, 7, 33), (512, 8, 16, 3, 192), (96, 5, 141, 5, 1), (32, 1, 16, 2, 512), (128, 4, 30, 11, 17),
                                        (320, 7, 29, 4, 50)])
def test_field_from_rays_generic_vs_oracle(Wd, D, C, N, S):
    """Ragged tiles (N S not a multiple of the tile), S = 1 / 192 / 512, every mode: raw_t three-way; gradients of the FULL and the
    STATIC backward on the kernels' own branches."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    coarse, fine = G.modules(Wd, D, C, device=DEV)
    pf, pc = G.oracle_params(fine, torch.float32), G.oracle_params(coarse, torch.float32)
    tag = f"generic_field[{Wd},{D},{C},{N},{S}]"
    o, d, v, z, g_raw = _field_inputs(N, S, 3 + C + 6)
    res = {dt: _oracle_field(pf, D, o, d, v, z, None, dt, "fine", True)[0] for dt in (torch.float64, torch.float32)}
    oh, dh, vh = (t.to(DEV).clone().requires_grad_() for t in (o, d, v))
    with B.tapped() as tap:
        raw_t = ops.field_from_rays(oh, dh, vh, z.to(DEV), fine.packed_any(), L.FIELD_FULL)
    assert tap.get("masks_generic") and not tap.get("masks")
    raw_t.backward(g_raw.permute(0, 2, 1).contiguous().to(DEV))
    B.three_way(tag, "raw full", raw_t.permute(0, 2, 1), res[torch.float32], res[torch.float64])
    G.pinned_gradients_generic(tag, {"d rays_o": oh.grad, "d rays_d": dh.grad, "d viewdirs": vh.grad}, tap,
                               lambda dt, act, _: _oracle_field(pf, D, o, d, v, z, g_raw, dt, "fine", True, act=act)[1])
    # static head of the coarse network (test_time False), forward and backward
    gs = g_raw[..., :3 + C + 1].contiguous()
    res = {dt: _oracle_field(pc, D, o, d, v, z, None, dt, "coarse", False)[0] for dt in (torch.float64, torch.float32)}
    oh, dh, vh = (t.to(DEV).clone().requires_grad_() for t in (o, d, v))
    with B.tapped() as tap:
        raw_s = ops.field_from_rays(oh, dh, vh, z.to(DEV), coarse.packed_any(), L.FIELD_STATIC)
    raw_s.backward(gs.permute(0, 2, 1).contiguous().to(DEV))
    B.three_way(tag, "raw static", raw_s.permute(0, 2, 1), res[torch.float32], res[torch.float64])
    G.pinned_gradients_generic(tag + " static", {"d rays_o": oh.grad, "d rays_d": dh.grad, "d viewdirs": vh.grad}, tap,
                               lambda dt, act, _: _oracle_field(pc, D, o, d, v, z, gs, dt, "coarse", False, act=act)[1])
    # sigma only
    sig = ops.field_from_rays(o.to(DEV), d.to(DEV), v.to(DEV), z.to(DEV), coarse.packed_any(), L.FIELD_SIGMA)
    res = {dt: _oracle_field(pc, D, o, d, v, z, None, dt, "coarse", False, sigma=True)[0] for dt in (torch.float64, torch.float32)}
    B.three_way(tag, "raw sigma", sig.permute(0, 2, 1), res[torch.float32], res[torch.float64])


@pytest.mark.parametrize("Wd,D", [(48, 8), (64, 9)])
def test_unsupported_shapes_raise_naming_the_shape(Wd, D):
    from nefes_amd.render import render
    coarse, fine = G.modules(Wd, D, 16, device=DEV)
    with pytest.raises(RuntimeError, match=f"D={D}.*W={Wd}"):
        render(2, 2, 2.0, c2w=O.bench_pose().to(DEV), near=0., far=4., **G.render_kwargs(coarse, fine, 64, 64))


def test_train_mode_is_refused_naming_the_shape():
    from nefes_amd.render import render
    coarse, fine = G.modules(64, 6, 16, device=DEV)
    fine.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="train mode.*D=6.*W=64"):
        render(2, 2, 2.0, c2w=O.bench_pose().to(DEV), near=0., far=4., **G.render_kwargs(coarse, fine, 64, 64, test_time=False))


def test_tuned_shapes_launch_no_generic_kernel():
    """Without NEFES_FIELD_GENERIC a W = 128 / 256, D = 8 network stays on the tuned instances: no generic launch is timed or tapped."""
    from nefes_amd import ops
    from nefes_amd.render import render
    assert not ops.FIELD_GENERIC
    for Wd, C in ((256, 16), (128, 128)):
        coarse, fine = G.modules(Wd, 8, C, device=DEV)
        assert not fine.uses_generic() and not coarse.uses_generic()
        c2w = O.bench_pose().to(DEV).requires_grad_()
        ops.TIMERS = {}
        try:
            with B.tapped() as tap:
                rgb, _, _, ex = render(4, 6, 525.505 * 6 / 640., c2w=c2w, near=0., far=4., **G.render_kwargs(coarse, fine, 64, 64))
                (rgb.sum() + ex["feat_map"].sum()).backward()
            names = list(ops.TIMERS)
        finally:
            ops.TIMERS = None
        assert not tap.get("masks_generic")
        assert names and not [n for n in names if "generic" in n], names


def test_two_streams_give_identical_results():
    from nefes_amd import lib as L
    from nefes_amd import ops
    _, fine = G.modules(64, 6, 16, device=DEV)
    pk = fine.packed_any()
    o, d, v, z, g_raw = (t.to(DEV) for t in _field_inputs(301, 96, 3 + 16 + 6))
    g_raw = g_raw.permute(0, 2, 1).contiguous()

    def run():
        oo, dd = o.clone().requires_grad_(), d.clone().requires_grad_()
        raw = ops.field_from_rays(oo, dd, v, z, pk, L.FIELD_FULL)
        raw.backward(g_raw)
        return raw.detach().clone(), oo.grad.clone(), dd.grad.clone()

    base = run()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    outs = []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(run())
    torch.cuda.synchronize()
    for out in outs:
        assert all(torch.equal(a, b) for a, b in zip(base, out))


_CHILD = r"""
import json, sys, torch
sys.path.insert(0, {root!r})
from nefes_amd import lib as L, ops
from tests import generic_util as G
from tests.test_gpu_generic_field import _field_inputs
Wd = int(sys.argv[1])
assert ops.FIELD_GENERIC == (sys.argv[2] == "1")
coarse, fine = G.modules(Wd, 8, 16, device="cuda:0")
assert fine.uses_generic() == ops.FIELD_GENERIC
o, d, v, z, g_raw = (t.to("cuda:0") for t in _field_inputs(9, 40, 3 + 16 + 6))
out = {{}}
for mode, net, R in ((L.FIELD_FULL, fine, 25), (L.FIELD_STATIC, coarse, 20), (L.FIELD_SIGMA, coarse, 1)):
    oo, dd, vv = (t.clone().requires_grad_() for t in (o, d, v))
    raw = ops.field_from_rays(oo, dd, vv, z, net.packed_any(), mode)
    out[f"raw{{mode}}"] = raw.permute(0, 2, 1).cpu()
    if mode != L.FIELD_SIGMA:
        raw.backward(g_raw[..., :R].permute(0, 2, 1).contiguous())
        out[f"g_o{{mode}}"], out[f"g_d{{mode}}"], out[f"g_v{{mode}}"] = oo.grad.cpu(), dd.grad.cpu(), vv.grad.cpu()
torch.save(out, sys.argv[3])
"""


@pytest.mark.parametrize("Wd", [128, 256])
def test_generic_against_tuned_on_the_same_weights(Wd, tmp_path):
    """raw_t of the three modes and the ray gradients, generic (NEFES_FIELD_GENERIC=1, child process) and tuned fp16 two-part kernels,
    both against float64 (gradients: the float64 oracle's own branches, identical inputs): the generic error may not exceed 1.5 x the
    tuned one or 1e-6 relative, whichever is larger."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    got = {}
    for flag in ("0", "1"):
        env = dict(os.environ, NEFES_FIELD_GENERIC=flag)
        out = tmp_path / f"out{flag}.pt"
        subprocess.run([sys.executable, str(script), str(Wd), flag, str(out)], check=True, env=env, cwd=ROOT, timeout=600)
        got[flag] = torch.load(out)
    coarse, fine = G.modules(Wd, 8, 16)
    o, d, v, z, g_raw = _field_inputs(9, 40, 3 + 16 + 6)
    pf, pc = G.oracle_params(fine, torch.float64), G.oracle_params(coarse, torch.float64)
    truth = {}
    raw, gr = _oracle_field(pf, 8, o, d, v, z, g_raw, torch.float64, "fine", True)
    truth.update({"raw2": raw, "g_o2": gr["d rays_o"], "g_d2": gr["d rays_d"], "g_v2": gr["d viewdirs"]})
    raw, gr = _oracle_field(pc, 8, o, d, v, z, g_raw[..., :20].contiguous(), torch.float64, "coarse", False)
    truth.update({"raw1": raw, "g_o1": gr["d rays_o"], "g_d1": gr["d rays_d"], "g_v1": gr["d viewdirs"]})
    truth["raw0"] = _oracle_field(pc, 8, o, d, v, z, None, torch.float64, "coarse", False, sigma=True)[0]
    bad = []
    for k in sorted(truth):
        e_t, e_g = B.rel(got["0"][k], truth[k]), B.rel(got["1"][k], truth[k])
        print(f"[generic_vs_tuned[{Wd}]] {k}: tuned-vs-f64 {e_t:.2e}  generic-vs-f64 {e_g:.2e}")
        P.record(f"generic_vs_tuned[{Wd}]", k, e_hip=e_g, e_ref=e_t, bound=max(1.5 * e_t, 1e-6))
        if e_g > max(1.5 * e_t, 1e-6):
            bad.append((k, e_t, e_g))
    assert not bad, bad


def test_refinement_loop_on_a_generic_network_graph_equals_eager(golden):
    """PoseRefiner on a (64, 6) network: a few iterations eager and as a captured, replayed graph walk the same poses and losses bit
    for bit (geometry, target and learning rates of tests/golden/refine.npz; the target only has to have the network's C channels)."""
    import types
    from nefes_amd.refine import PoseRefiner
    g = golden("refine")
    C = int(g["C"])
    out = {}
    for graph in (False, True):
        coarse, fine = G.modules(64, 6, C, device=DEV)
        assert fine.uses_generic()
        with torch.no_grad():
            coarse.exposure_embedding.params.copy_(T(g["exposure_params"]))
        args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
        kw = dict(network_query_fn=None, perturb=0., N_importance=int(g["Ni"]), N_samples=int(g["Nc"]), network_fn=coarse,
                  network_fine=fine, use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False,
                  lindisp=False)
        world = dict(pose_scale=float(g["pose_scale"]), pose_scale2=float(g["pose_scale2"]), move_all_cam_vec=g["move_all_cam_vec"].tolist())
        H, W, focal = g["hwf"].tolist()
        ref = PoseRefiner(kw, args, (H, W, focal), float(g["near"]), float(g["far"]), tinyscale=int(g["tinyscale"]),
                          lr_r=float(g["lr"][0]), lr_t=float(g["lr"][1]), world_setup=world, graph=graph, device=DEV)
        pose, losses = ref.refine(T(g["init_c2w"]), T(g["target"]), T(g["hist"]), 4)
        out[graph] = (pose[:3, :4].cpu().numpy(), losses.cpu().numpy())
    assert np.isfinite(out[True][1]).all() and out[True][1][0] != out[True][1][-1]
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][1], out[True][1])
