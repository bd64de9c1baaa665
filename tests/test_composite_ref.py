"""tests/composite_ref.py, the yardstick of tests/test_gpu_composite.py, checked on the CPU: its two tolerance constants are what
the fp32 oracle really does on the case list, the inputs keep that below 1e-5, nothing but the zero-density ray's disp (and what a
disp upstream makes of it) is left out, and the comparison SEES the mistakes a compositing kernel can make -- five float64 copies
of the oracle with one rule changed each (plain torch, written here) land at least 10 x over the bound."""
import pytest
import torch

from tests import composite_ref as R

RUNS = R.all_runs()


@pytest.fixture(scope="module")
def ref_errors():
    """[(case, only, {group: e_ref})]: the fp32 oracle against the float64 oracle, per run."""
    out = []
    for case, only in RUNS:
        m32, g32 = R.run_oracle(case, torch.float32, only)
        out.append((case, only, {k: v[0] for k, v in R.errors(case, m32, g32, only).items()}))
    return out


def test_the_constants_are_what_the_fp32_oracle_does(ref_errors):
    e_maps = max(e for _, _, d in ref_errors for k, e in d.items() if R.is_map(k))
    e_grads = max(e for _, _, d in ref_errors for k, e in d.items() if not R.is_map(k))
    print(f"fp32 oracle vs float64, per ray: maps {e_maps:.3e} (E_MAPS {R.E_MAPS:.1e}), gradient rows {e_grads:.3e} (E_GRADS {R.E_GRADS:.1e})")
    assert R.E_MAPS / 2 <= e_maps <= R.E_MAPS, e_maps
    assert R.E_GRADS / 2 <= e_grads <= R.E_GRADS, e_grads


def test_the_inputs_keep_fp32_within_1e_5():
    """A condition on the INPUTS (tests/composite_ref.py make_case): 4 E stays under the project's 1e-4."""
    assert R.E_MAPS <= 1e-5 and R.E_GRADS <= 1e-5


def test_only_the_zero_density_rays_disp_is_left_out():
    """NaN in float64 = left out of the comparison (R.errors).  That is disp of NAN_RAY, one ray of N, and -- only when a disp
    upstream is part of the loss -- that ray's two sigma rows: 0 x NaN, the reference's own arithmetic, in float64 and fp32 alike
    (indexing the ray out of the loss hands the division a zero gradient, and the division multiplies it by NaN)."""
    seen = 0
    for case, only in RUNS:
        q64 = R.quantities(case, *R.run_oracle(case, torch.float64, only))
        q32 = R.quantities(case, *R.run_oracle(case, torch.float32, only))
        has_ray, with_disp = case["N"] > R.NAN_RAY and case["tag"] != "D", "disp" in R.present(case, only)
        for k, v in q64.items():
            nan = torch.isnan(v)
            assert torch.equal(nan, torch.isnan(q32[k])), (case["key"], only, k)
            assert bool(torch.isfinite(v[~nan]).all()) and bool(torch.isfinite(q32[k][~nan]).all())
            rows = nan.reshape(nan.shape[0], -1).any(1).nonzero().flatten().tolist()
            if k == "map disp":
                assert rows == ([R.NAN_RAY] if has_ray else []), (case["key"], only, k, rows)
                seen += has_ray
            elif k in ("d sigma", "d t_sigma"):
                assert rows in ([], [R.NAN_RAY]) and (not rows or (has_ray and with_disp)), (case["key"], only, k, rows)
            else:
                assert rows == [], (case["key"], only, k, rows)
        if has_ray and with_disp:
            assert bool(torch.isnan(q64["d sigma"][R.NAN_RAY]).all())
    assert seen > 50


def test_the_clamp_ray_is_on_the_clamp_branch():
    for case, only in RUNS:
        if case["N"] > R.CLAMP_RAY and case["tag"] != "D":
            for dt in (torch.float64, torch.float32):
                m, g = R.run_oracle(case, dt, only)
                assert float(m["disp"][R.CLAMP_RAY]) == 1e10 and float(m["depth"][R.CLAMP_RAY]) == 0.
                if only == "disp":
                    assert not bool(g[R.CLAMP_RAY].any())


# ---- the comparison has teeth ----------------------------------------------------------------------------------------------
def _excl(om):
    return torch.cumprod(torch.cat([torch.ones_like(om[:, :1]), om], -1)[:, :-1], -1)


def restated(mut=None):
    """raw2outputs_NeRFH_NFF once more in plain torch (equal to oracle/ref_cpu.py composite bit for bit when mut is None), with one
    rule changed (the gradients: autograd sums them in another order, so to 1e-12 of the scales):  a  delta at sample 63 taken as 1e2 (a pass boundary treated as the ray's end);  b  the transmittance restarted
    at 1 from sample 64;  c  variant B, d disp / d sum(w_only) dropped;  d  feature channel c >= 64 read from channel c - 64;
    e  the last sample's weight left out of acc."""
    def forward(case, raw, z):
        tag, C, S = case["tag"], case["C"], case["S"]
        trans = tag in ("A", "B")
        i_s = 0 if tag == "D" else 3 + C
        delta = torch.cat([z[:, 1:] - z[:, :-1], 1e2 * torch.ones_like(z[:, :1])], -1)
        if mut == "a" and S > 64:
            delta = delta.clone()
            delta[:, 63] = 1e2
        T_of = (lambda al: torch.cat([_excl(1 - al[:, :64]), _excl(1 - al[:, 64:])], -1)) if (mut == "b" and S > 64) else (lambda al: _excl(1 - al))
        s_sig = raw[..., i_s]
        if trans:
            t_sig, t_col, t_beta = raw[..., i_s + 4], raw[..., i_s + 1:i_s + 4], raw[..., i_s + 5]
            a_s, a_t, a = 1 - torch.exp(-delta * s_sig), 1 - torch.exp(-delta * t_sig), 1 - torch.exp(-delta * (s_sig + t_sig))
        else:
            a = 1 - torch.exp(-delta * (s_sig + torch.zeros_like(s_sig)))
        T = T_of(a)
        w = a * T
        acc = w[:, :-1].sum(-1) if mut == "e" else w.sum(-1)
        if tag == "D":
            return {"acc": acc, "weights": w}
        col, f = raw[..., :3], raw[..., 3:3 + C]
        if mut == "d" and C > 64:
            f = torch.cat([f[..., :64], f[..., :C - 64]], -1)
        if tag == "B":
            w_only = a_s * T_of(a_s)
            depth = (w_only * z).sum(-1)
            sw = torch.sum(w_only, -1)
            disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / (sw.detach() if mut == "c" else sw))
            return {"rgb": (w_only[..., None] * col).sum(1), "feat": (w_only.detach()[..., None] * f).sum(1), "disp": disp, "acc": acc,
                    "depth": depth, "weights": w_only, "beta": torch.zeros_like(acc)}
        if tag == "A":
            w_s, w_t = a_s * T, a_t * T
            rgb_s = (w_s[..., None] * col).sum(1)
            feat = (w_s.detach()[..., None] * f).sum(1)
            if case["white"]:
                rgb_s = rgb_s + (1 - acc[:, None])
            rgb = rgb_s + (w_t[..., None] * t_col).sum(1)
            beta = (w_t * t_beta).sum(-1) + 0.1
        else:
            rgb = (w[..., None] * col).sum(1)
            feat = (w.detach()[..., None] * f).sum(1)
            beta = torch.zeros_like(acc)
        depth = torch.sum(w * z, -1)
        disp = 1. / torch.max(1e-10 * torch.ones_like(depth), depth / torch.sum(w, -1))
        return {"rgb": rgb, "feat": feat, "disp": disp, "acc": acc, "depth": depth, "weights": w, "beta": beta}
    return forward


def test_the_restatement_is_the_oracle():
    for case, only in RUNS:
        m, g = R.run_forward(case, torch.float64, only, restated())
        m64, g64 = R.run_oracle(case, torch.float64, only)
        same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.), torch.nan_to_num(b, nan=-7.))
        assert all(same(m[k], m64[k]) for k in m64), (case["key"], only)
        assert max(v[0] for v in R.errors(case, m, g, only).values()) <= 1e-12, (case["key"], only)


@pytest.mark.parametrize("mut", ["a", "b", "c", "d", "e"])
def test_a_changed_rule_lands_ten_times_over_the_bound(mut):
    """... on the case list as a whole (where the rays with a role, whose scales can be tiny, carry the largest figures), AND on an
    ORDINARY ray -- none of R.ROLE_RAYS -- in a named group: the cancel x U scale leaves the sigma rows of a normal ray sensitive."""
    worst, ordinary = (0., None), (0., None)
    plain = torch.tensor([n not in R.ROLE_RAYS for n in range(64)])
    for case, only in RUNS:
        if (mut in "ab" and case["S"] <= 64) or (mut == "c" and case["tag"] != "B") or (mut == "d" and case["C"] <= 64):
            continue
        m, g = R.run_forward(case, torch.float64, only, restated(mut))
        try:
            e = R.ray_errors(case, m, g, only)
        except AssertionError:               # a NaN where float64 has none (or none where it has one) fails the comparison outright
            worst = (float("inf"), (case["key"], only, "NaN pattern"))
            continue
        e_ref = R.errors(case, *R.run_oracle(case, torch.float32, only), only)
        for k, (v, where) in e.items():
            ratio = v / R.bound(e_ref[k][0], R.E_MAPS if R.is_map(k) else R.E_GRADS)
            n = int(ratio.argmax())
            if float(ratio[n]) > worst[0]:
                worst = (float(ratio[n]), (case["key"], only, k, (n, int(where[n]))))
            ratio = torch.where(plain[:case["N"]], ratio, torch.zeros_like(ratio))
            n = int(ratio.argmax())
            if float(ratio[n]) > ordinary[0]:
                ordinary = (float(ratio[n]), (case["key"], only, k, (n, int(where[n]))))
    print(f"rule {mut}: {worst[0]:.3g} x the bound at {worst[1]}; on an ordinary ray {ordinary[0]:.3g} x at {ordinary[1]}")
    assert worst[0] >= 10., worst
    assert ordinary[0] >= 10., ordinary
