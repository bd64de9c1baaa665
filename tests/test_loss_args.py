"""What a CPU can check of the train-loss entry points (csrc/losses.hip): the exports, the scratch size, every refusal -- those return
before any HIP call, so the pointers here are dummies that are never dereferenced -- and the opt-in plumbing: nefes_amd.losses.install
replaces the five values of a module's loss_dict and nothing else, and the launcher does not call it unless NEFES_HIP_LOSSES=1."""
import ctypes as C
import os
import subprocess
import sys
import types

from nefes_amd import lib as L

BADARG, UNSUPPORTED = -1, -2
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (L.LOSS_HAS_RGB_FINE | L.LOSS_HAS_RGB_COARSE | L.LOSS_HAS_BETA | L.LOSS_HAS_FEAT_FINE | L.LOSS_HAS_FEAT_COARSE
       | L.LOSS_HAS_FEAT_FUSION | L.LOSS_NERFW)
IN = ("rgb_fine", "rgb_coarse", "rgb_target", "beta", "sigmas", "feat_fine", "feat_coarse", "feat_fusion", "feat_target")
OUT = ("g_rgb_fine", "g_rgb_coarse", "g_beta", "g_sigma", "g_feat_fine", "g_feat_coarse", "g_feat_fusion")


def _desc(N=37, Cc=5, S=7, kind=L.LOSS_FEAT_L1, present=ALL, coef=1.0, lam=0.01, stride=None):
    return L.NefesTrainLossDesc(N, Cc, S, kind, present, coef, lam, S if stride is None else stride)


def _fwd(desc=None, scratch=PTR, terms=PTR, losses=PTR, **kw):
    ptrs = [kw.get(k, PTR) for k in IN]
    return L.load().nefes_train_loss_fwd(C.byref(desc or _desc()), *ptrs, scratch, terms, losses, None)


def _bwd(desc=None, g=(PTR, PTR, PTR), **kw):
    ptrs = [kw.get(k, PTR) for k in IN] + [kw.get(k, PTR) for k in OUT]
    return L.load().nefes_train_loss_bwd(C.byref(desc or _desc()), *g, *ptrs, None)


def test_names_are_declared_and_exported():
    lib = L.load()
    for name in ("nefes_train_loss_scratch_doubles", "nefes_train_loss_fwd", "nefes_train_loss_bwd"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    assert f"#define NEFES_TRAIN_LOSS_ROWS {L.TRAIN_LOSS_ROWS}\n" in hdr
    assert C.sizeof(L.NefesTrainLossDesc) == 40 and L.NefesTrainLossDesc.sigma_row_stride.offset == 32


def test_scratch_query():
    q = L.load().nefes_train_loss_scratch_doubles
    assert q(0) == 0 and q(-5) == 0
    for N in (1, L.TRAIN_LOSS_ROWS - 1, L.TRAIN_LOSS_ROWS, L.TRAIN_LOSS_ROWS + 1, 65, 6144, 7168):
        assert q(N) == 8 * -(-N // L.TRAIN_LOSS_ROWS), N                    # eight doubles per block of TRAIN_LOSS_ROWS rays


def test_forward_refusals():
    for call in (_fwd, _bwd):
        assert call(_desc(N=0)) == BADARG and call(_desc(N=-3)) == BADARG
        assert call(rgb_target=None) == BADARG
        for k in ("rgb_fine", "rgb_coarse", "beta", "sigmas", "feat_fine", "feat_coarse", "feat_fusion", "feat_target"):
            assert call(**{k: None}) == BADARG, k                           # its presence bit is on
        for kind in (-1, 3, 99):
            assert call(_desc(kind=kind)) == BADARG, kind
        assert call(_desc(present=ALL | 128)) == BADARG                     # a bit outside the mask
        assert call(_desc(Cc=0)) == BADARG and call(_desc(S=0)) == BADARG and call(_desc(stride=6)) == BADARG
        # the class's required colour: NeRF-W needs rgb_coarse, the plain form rgb_fine; beta belongs to NeRF-W with rgb_fine
        assert call(_desc(present=L.LOSS_NERFW | L.LOSS_HAS_RGB_FINE)) == BADARG
        assert call(_desc(present=L.LOSS_HAS_RGB_COARSE)) == BADARG
        assert call(_desc(present=L.LOSS_HAS_RGB_FINE | L.LOSS_HAS_BETA)) == BADARG
        assert call(_desc(present=L.LOSS_NERFW | L.LOSS_HAS_RGB_COARSE | L.LOSS_HAS_BETA)) == BADARG
        assert call(_desc(Cc=(1 << 20) + 1)) == UNSUPPORTED and call(_desc(S=(1 << 20) + 1, stride=1 << 21)) == UNSUPPORTED
    for k in ("scratch", "terms", "losses"):
        assert _fwd(**{k: None}) == BADARG, k


def test_backward_refusals():
    none = {k: None for k in OUT}
    assert _bwd(**none) == BADARG                                           # no gradient wanted at all
    plain = _desc(present=L.LOSS_HAS_RGB_FINE)
    rest = dict(rgb_coarse=None, beta=None, sigmas=None, feat_fine=None, feat_coarse=None, feat_fusion=None, feat_target=None)
    for k in OUT[1:]:
        assert _bwd(plain, **rest, **{**none, "g_rgb_fine": PTR, k: PTR}) == BADARG, k      # a gradient for an input that is absent


def test_install_replaces_the_five_values_only():
    from nefes_amd import losses
    sentinel = object()
    d = {k: sentinel for k in losses.loss_dict}
    d["extra"] = sentinel
    stub = types.ModuleType("stub_losses")
    stub.__file__ = "/somewhere/script/models/losses.py"
    stub.loss_dict = d
    stub.compute_depth_loss = sentinel
    assert losses.install(stub) is stub
    assert stub.loss_dict is d and stub.__file__ == "/somewhere/script/models/losses.py" and stub.compute_depth_loss is sentinel
    assert set(d) == set(losses.loss_dict) | {"extra"} and d["extra"] is sentinel
    assert sorted(losses.loss_dict) == ['color', 'color_feat', 'color_feat_fusion', 'color_feat_fusion_nerfw', 'nerfw']
    for k, cls in losses.loss_dict.items():
        assert d[k] is cls and cls.__module__ == "nefes_amd.losses"
    assert [c.__name__ for c in (d['color'], d['color_feat'], d['nerfw'], d['color_feat_fusion'], d['color_feat_fusion_nerfw'])] == [
        'ColorLoss', 'ColorFeatureLoss', 'NerfWLoss', 'ColorFeatureFusionLoss', 'ColorFeatureFusionNerfWLoss']


def test_launcher_installs_only_with_the_switch(tmp_path):
    """python -m nefes_amd.run_reference on a script that prints who made models.losses.loss_dict's classes, from a directory whose
    models/losses.py stands for the reference's: unset and "0" leave it alone, "1" installs."""
    script_dir = tmp_path / "script"
    (script_dir / "models").mkdir(parents=True)
    (script_dir / "models" / "losses.py").write_text("class A: pass\nloss_dict = {k: A for k in ('color', 'color_feat', 'nerfw', "
                                                     "'color_feat_fusion', 'color_feat_fusion_nerfw')}\n")
    (script_dir / "probe.py").write_text("import sys\nfrom models.losses import loss_dict\nimport models.losses as m\n"
                                         "print(sorted({v.__module__ for v in loss_dict.values()}), m.__file__, 'nefes_amd.losses' in sys.modules)\n")
    env = {k: v for k, v in os.environ.items() if k != "NEFES_HIP_LOSSES"}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = lambda e: subprocess.run([sys.executable, "-m", "nefes_amd.run_reference", "probe.py"], cwd=script_dir, env=e, capture_output=True,
                                   text=True, check=True).stdout.split()
    own = str(script_dir / "models" / "losses.py")
    assert run(env) == ["['models.losses']", own, "False"]
    assert run({**env, "NEFES_HIP_LOSSES": "0"}) == ["['models.losses']", own, "False"]
    assert run({**env, "NEFES_HIP_LOSSES": "1"}) == ["['nefes_amd.losses']", own, "True"]
