"""tests/glue_ref.py, the yardstick of tests/test_gpu_glue.py, checked on the CPU: the float64 references against something they did not
compute themselves (torch.optim.Adam, gradcheck, an explicit o + d z autograd), and every input set against the bound the GPU test
asserts -- the same expression in fp32 torch stays inside it, so the inputs are conditioned well enough for the bound to mean something."""
import pytest
import torch

from tests import glue_ref as R


# ---- the references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(R.ADAM_SIZES))
def test_adam_is_torch_optim_adam_in_float64(n):
    want, got = R.torch_adam(n, torch.float64), R.adam_truth(n)
    for t in R.ADAM_CHECK:
        for name, a, b in zip("pmv", got[t], want[t]):
            assert R.rel_elem(a, b) <= 1e-14, (n, t, name, R.rel_elem(a, b))


def test_adam_step_one_tells_the_bias_corrections_apart():
    """With beta^(t-1) in place of beta^t the first step divides by 1 - beta^0 = 0."""
    case = R.adam_case(6)
    p1 = R.adam_truth(6)[1][0]
    want = case["p0"].double() - case["lr"] * torch.sign(case["grads"][0].double())        # |step 1| = lr where |g| >> eps
    big = case["grads"][0].abs() > 1e-4
    assert bool(big.sum() >= 4) and R.rel_elem(p1[big], want[big]) < 1e-4


def test_fusion_input_gradcheck():
    g = torch.Generator().manual_seed(0)
    B, H, W, C = 2, 2, 3, 2
    rgb = torch.rand(B * H * W, 3, generator=g, dtype=torch.float64).requires_grad_()
    feat = torch.randn(B * H * W, C, generator=g, dtype=torch.float64).requires_grad_()
    affine = torch.randn(B, 12, generator=g, dtype=torch.float64)
    for a in (None, affine):
        assert torch.autograd.gradcheck(lambda r, f: R.fusion_input(r, f, a, B, H, W, R.MEAN, R.STD), (rgb, feat))
    x = R.fusion_input(rgb, feat, affine, B, H, W, R.MEAN, R.STD)
    assert x.shape == (B, 3 + C, H, W)
    assert torch.equal(x[1, 3:, 1, 2], feat[1 * H * W + 1 * W + 2])                  # image 1, pixel (1, 2): its feature row
    y = torch.sigmoid(affine[1, :9].reshape(3, 3) @ rgb[H * W] + affine[1, 9:])      # image 1, pixel (0, 0): K rgb + b with ITS affine
    assert torch.allclose(x[1, :3, 0, 0], (y - torch.tensor(R.MEAN, dtype=torch.float64)) / torch.tensor(R.STD, dtype=torch.float64), rtol=1e-14, atol=0)


def test_feat_head_gradcheck_and_its_backward():
    g = torch.Generator().manual_seed(1)
    gmap = torch.randn(3, 5, generator=g, dtype=torch.float64).requires_grad_()
    w, b = torch.randn(4, 4, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda m: R.feat_head(m, w, b), (gmap,))
    g_feat = torch.randn(3, 4, generator=g, dtype=torch.float64)
    got, = torch.autograd.grad(R.feat_head(gmap, w, b), gmap, g_feat)
    assert torch.allclose(got, R.feat_head_bwd(g_feat, w, b), rtol=1e-14, atol=1e-15)
    assert bool((R.feat_head_abs(gmap, w, b) >= R.feat_head(gmap, w, b).abs()).all())


def test_ray_reduce_is_the_autograd_of_o_plus_d_z():
    case = {k: v.double() for k, v in R.reduce_case(5, 21).items()}
    o, d, v = (torch.randn(5, 3, dtype=torch.float64).requires_grad_() for _ in range(3))
    pts = o[:, None, :] + d[:, None, :] * case["z"][..., None]
    vs = v[:, None, :].expand(5, 21, 3)
    want = torch.autograd.grad((pts * case["g_pts"]).sum() + (vs * case["g_vs"]).sum(), (o, d, v))
    got = R.ray_reduce(case["z"], case["g_pts"], case["g_vs"])
    for a, b in zip(got[:3], want):
        assert torch.allclose(a, b, rtol=1e-13, atol=1e-14)
    assert all(bool((a >= s.abs()).all()) for s, a in zip(got[:3], got[3:]))
    assert torch.equal(R.ray_reduce(case["z"], case["g_pts"], None)[2], torch.zeros(5, 3, dtype=torch.float64))


# ---- the inputs: fp32 torch stays inside the bound the GPU test asserts -------------------------------------------------------------
@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("shape", R.FUSION_SHAPES)
def test_fusion_inputs(shape, with_affine):
    case = R.fusion_case(*shape)
    assert 0 <= float(case["rgb"].min()) and float(case["rgb"].max()) <= 1
    k, b = case["affine"][:, :9].reshape(-1, 1, 3, 3).double(), case["affine"][:, 9:].double()
    lin = (k @ case["rgb"].reshape(shape[0], -1, 3, 1).double()).squeeze(-1) + b[:, None, :]
    assert float(lin.abs().max()) <= R.LIN_MAX and float(lin.abs().max()) > 1
    assert shape[0] == 1 or not torch.equal(case["affine"][0], case["affine"][1])
    x64, g64 = R.fusion_eval(case, shape, with_affine, torch.float64)
    x32, g32 = R.fusion_eval(case, shape, with_affine, torch.float32)
    e_x, e_g = R.rel_max(x32, x64), R.rel_max(g32, g64)
    print(f"fusion_input {shape} affine={with_affine}: fp32 torch x {e_x:.2e}, g_rgb {e_g:.2e}")
    assert e_x <= R.TOL_FP32 and e_g <= R.TOL_FP32


@pytest.mark.parametrize("shape", R.HEAD_SHAPES)
def test_feat_head_inputs(shape):
    case = R.head_case(*shape)
    d = {k: v.double() for k, v in case.items()}
    b_fwd, b_bwd = R.head_bounds(case)
    r_f = R.ratio(R.feat_head(case["gmap"], case["w"], case["b"]), R.feat_head(d["gmap"], d["w"], d["b"]), b_fwd)
    r_b = R.ratio(R.feat_head_bwd(case["g_feat"], case["w"], case["b"]), R.feat_head_bwd(d["g_feat"], d["w"], d["b"]), b_bwd)
    print(f"feat_head {shape}: fp32 torch / bound forward {r_f:.3f}, backward {r_b:.3f}")
    assert r_f <= 1 and r_b <= 1
    # what the bound is there to see: one dropped term is far outside it
    F = shape[2]
    dropped = R.feat_head(d["gmap"], d["w"], d["b"]) - d["gmap"][:, F - 1:F] * d["w"][:, F - 1]
    assert R.ratio(dropped, R.feat_head(d["gmap"], d["w"], d["b"]), b_fwd) > 100


@pytest.mark.parametrize("n", list(R.ADAM_SIZES))
def test_adam_inputs(n):
    case, truth, got = R.adam_case(n), R.adam_truth(n), R.torch_adam(n, torch.float32)
    assert float(case["lr"].min()) >= 1e-5 and float(case["lr"].max()) <= 1e-2
    if n >= 3:
        g = case["grads"]
        assert bool((g[:, R.ADAM_ZERO] == 0).all()) and 4e-13 < float(g[:, R.ADAM_TINY].abs().min()) and float(g[:, R.ADAM_TINY].abs().max()) < 2e-12
        assert float(g[:, R.ADAM_HUGE].abs().min()) > 4e5
        assert torch.equal(truth[60][0][R.ADAM_ZERO], case["p0"][R.ADAM_ZERO].double())      # the denominator is eps alone: 0 / eps
    for t in R.ADAM_CHECK:
        for name, a, b in zip("pmv", got[t], truth[t]):
            e = R.rel_elem(a, b)
            print(f"adam n={n} step {t} {name}: fp32 torch.optim.Adam {e:.2e}")
            assert e <= R.TOL_FP32, (n, t, name, e)


@pytest.mark.parametrize("shape", R.REDUCE_SHAPES)
def test_ray_reduce_inputs(shape):
    case = R.reduce_case(*shape)
    ref = R.ray_reduce(*(case[k].double() for k in ("z", "g_pts", "g_vs")))
    got = R.ray_reduce(case["z"].double(), case["g_pts"].double(), case["g_vs"].double())
    gz = (case["g_pts"] * case["z"][..., None]).double().sum(1)                       # the kernel's order: fp32 product, float64 sum
    assert R.ratio(got[0].float(), ref[0], 2 * R.U * ref[3]) <= 1 and R.ratio(got[2].float(), ref[2], 2 * R.U * ref[5]) <= 1
    assert R.ratio(gz.float(), ref[1], 3 * R.U * ref[4]) <= 1


@pytest.mark.parametrize("per_ray", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("Nc", R.DEPTH_NC)
def test_depth_inputs(Nc, lindisp, jitter, per_ray):
    case = R.depth_case(Nc)
    assert float(case["batch"][:, 6].min()) >= 0.25 and len(set(case["batch"][:, 6].tolist())) == R.DEPTH_N
    z64, _, _ = R.depth_ref(Nc, lindisp, jitter, per_ray, torch.float64)
    z32, near, far = R.depth_ref(Nc, lindisp, jitter, per_ray, torch.float32)
    e = R.rel_elem(z32, z64)
    print(f"coarse_depths Nc={Nc} lindisp={lindisp} jitter={jitter} per_ray={per_ray}: fp32 oracle {e:.2e}")
    # six roundings in the lindisp chain: the fp32 oracle itself can sit just above 2e-7 (2.25e-7 at Nc = 37, per ray), where the rule's
    # other arm, 1.5 e_ref, is the bound -- never more than 2.25 x the tolerance on these inputs
    assert e <= 1.5 * R.TOL_DEPTH
    assert R.depth_rows_ok(z32, near, far)


@pytest.mark.parametrize("geom", R.NDC_GEOM)
@pytest.mark.parametrize("n", R.NDC_N)
def test_ndc_inputs(n, geom):
    case = R.ndc_case(n, geom[3])
    o, d = case["o"].double(), case["d"].double()
    t = -(geom[3] + o[:, 2]) / d[:, 2]
    assert float(d[:, 2].abs().min()) >= R.NDC_MIN_Z and float((o[:, 2] + t * d[:, 2]).abs().min()) >= R.NDC_MIN_Z
    for which in ("both", "o", "d"):
        r64, r32 = R.ndc_eval(n, geom, torch.float64, which), R.ndc_eval(n, geom, torch.float32, which)
        errs = [R.rel_max(a, b) for a, b in zip(r32, r64)]
        print(f"ndc n={n} {geom} upstream={which}: fp32 oracle {['%.1e' % e for e in errs]}")
        assert max(errs) <= R.TOL_NDC

