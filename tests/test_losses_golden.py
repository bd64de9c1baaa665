"""tests/loss_ref.py (the GPU tests' yardstick for the train-loss kernels) against tests/golden/losses.npz, which the reference's own
loss classes wrote (tools/make_golden_losses.py): in float64 to 1e-12 of the reference's float64 run, in float32 to 1e-6 of its float32
run -- scalars relative to the value, gradients relative to the tensor's largest magnitude."""
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as R

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))
BASE = {k[3:]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("in.")}
CASES = R.fixture_cases(Z)


def test_fixture_covers_the_issue():
    assert BASE["rgb_fine"].shape == (37, 3) and BASE["feat_fine"].shape == (37, 5) and BASE["transient_sigmas"].shape == (37, 7)
    assert all(v.dtype == torch.float32 for v in BASE.values())
    assert {name for _, name, _, _ in CASES} == set(R.CLASSES)
    fused = [(kw, keys) for _, name, kw, keys in CASES if name.startswith("color_feat_fusion")]
    for l1 in (True, False):
        assert {(kw["switch_on"], kw["color_only_switch"]) for kw, _ in fused if kw["L1_loss"] == l1} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(kw["cos_loss"] for kw, _ in fused)
    for key in ("rgb_coarse", "feat_coarse", "beta"):
        assert any(key in keys for _, _, _, keys in CASES) and any(key not in keys for _, _, _, keys in CASES)
    assert sum(int((BASE[k] == BASE["feat_target"]).sum()) for k in ("feat_fine", "feat_coarse", "feat_fusion")) >= 3      # planted ties


@pytest.mark.parametrize("dtype,tag,tol", [(torch.float64, "_f64", 1e-12), (torch.float32, "", 1e-6)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_restatement_matches_the_reference(case, dtype, tag, tol):
    i, name, kw, keys = case
    ret, grads = R.run(name, kw, BASE, keys, dtype=dtype)
    want = Z[f"case{i}.out{tag}"]
    assert len(ret) == len(want)
    for r, w in zip(ret, want):
        assert abs(float(r) - float(w)) <= tol * abs(float(w)), (name, kw, float(r), float(w))
    stored = {k[len(f"case{i}.g."):] for k in Z.files if k.startswith(f"case{i}.g.")}
    assert {k + tag for k in grads} == {k for k in stored if k.endswith("_f64") == bool(tag)}
    for k, g in grads.items():
        w = Z[f"case{i}.g.{k}{tag}"].astype(np.float64)
        assert np.abs(g.double().numpy() - w).max() <= tol * np.abs(w).max(), (name, kw, k)
