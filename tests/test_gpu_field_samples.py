"""Every fp16 two-part INFERENCE instance (the TRAIN = 0 rows of nefes_amd/csrc/field_h3_instances.h) against float64, per sample.

The census, the inputs (points exact in fp32), the networks, the per-sample scales and the rule are tests/field_ref.py's:

    E_hip[g] = max_m |hip - float64| / s[m, g]  <=  F * E_ref[g],   E_ref[g] the same of the fp32 oracle, F = 3, no absolute floor,

pooled over the shapes (1,1), (3,43), (5,64), (7,33) of one network and input set (681 samples).  Forward rows: the five output groups,
finite outputs, rays path == pts= path, a sample alone == the same sample inside a batch, the mask words against the float64
pre-activations.  Backward rows: d pts / d enc and d viewdirs per sample on the row's own forward's masks and raw, for a dense upstream
and for one upstream channel at a time.  The fused-gather rows add the hash grid's documented budget (tests/hashgrid_ref.py) through
the pinned float64 network's abs-Jacobian.  Every pair is recorded under field_samples[<row>] (tests/parity_log.py);
profiles/field_samples/README.md holds the table."""
import ctypes as C
import functools

import pytest
import torch

from tests import field_ref as R
from tests import hashgrid_ref as HG
from tests import parity_log as P
from tests.branch import decode_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = R.cases()
FWD = [c for c in CASES if c.row.startswith("fwd")]
BWD = [c for c in CASES if c.row.startswith("bwd")]
ALONE = (0, 100, 130, 230)                 # samples of the (7, 33) shape also evaluated alone: first / second tile, last sample
ALONE_FUSED = (0, 64, 129)                 # and of the fused-gather rows' one shape (130 rays of one sample)
ONE_CHANNEL_SHAPE = (5, 64)
# The fp32 oracle's gradient error stays at rounding level: 1e-5 is the largest seen in any case (d viewdirs of the rescaled network,
# tests/test_field_ref.py), fp32 rounding through twenty products; a reference further away than ten times that is not one.
E_REF_MAX = 1e-4


@pytest.fixture(autouse=True)
def _fp16_pipe():
    from nefes_amd import ops
    old = ops.SPLIT, ops.USE_X6, ops.FUSED_HASHGRID
    ops.SPLIT, ops.USE_X6, ops.FUSED_HASHGRID = "h3", True, True
    yield
    ops.SPLIT, ops.USE_X6, ops.FUSED_HASHGRID = old


# ---- networks, packs, inputs (shared by a forward row and its backward row) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network(Wd, Cf, has_t, ext, fold, fh, edit):
    """(fp32 parameters of the network the float64 side evaluates, its PackedField)"""
    from nefes_amd import lib as L
    from nefes_amd import ops
    p = R.make_net(Wd, Cf, has_t, ext, edit)
    if fh:                          # NeRFH_NFF.packed_fh: the pack without its feature rows; the kernel emits g = relu(dir_encoding)
        p["static_rgb.0.weight"], p["static_rgb.0.bias"] = p["static_rgb.0.weight"][:3].contiguous(), p["static_rgb.0.bias"][:3].contiguous()
    pk = ops.PackedField(p, Wd, 0 if fh else Cf, has_t, DEV, L.XYZ_EXTERNAL32 if ext else L.XYZ_FREQ10, fold_final=fold)
    return p, pk


@functools.lru_cache(maxsize=None)
def grid():
    from nefes_amd import ops
    geo = HG.geometry("default")
    table = HG.make_table(geo)
    return geo, table, ops.HashGrid(geo.bound, table=table, n_levels=geo.n_levels, log2_hashmap_size=geo.log2, base_resolution=geo.base,
                                    max_resolution=geo.max_res)


@functools.lru_cache(maxsize=None)
def inputs(kind, kset, N, S):
    """host inputs of one launch: dict(o, d, z, v, pts [M,3] | enc [M,32], dirs [M,3] per sample)"""
    if kind == "enc":
        enc, v = R.encodings(kset, N, S)
        return dict(enc=enc, v=v, dirs=R.per_sample(v, S))
    if kind == "hashgrid":          # one point per ray, away from the cell faces: o = x, d = 0, z = 0
        x = HG.positions("default", "inside", N)
        g = torch.Generator().manual_seed(77)
        o, d, z, v = x, torch.zeros(N, 3), torch.zeros(N, 1), torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    else:
        o, d, z, v = R.rays(kset, N, S)
    return dict(o=o, d=d, z=z, v=v, pts=R.exact(o, d, z).reshape(-1, 3), dirs=R.per_sample(v, S))


@functools.lru_cache(maxsize=None)
def truth(case_i, net_i, kset, N, S):
    """the float64 / fp32-oracle side of one launch (tests/field_ref.py Case64); a fused-gather row: on tests/hashgrid_ref.py's float64
    encoding, with its per-element budget"""
    case = CASES[case_i]
    n = case.network
    Cf, edit = n.nets[net_i]
    p, _ = network(n.width, Cf, n.has_transient, n.ext, n.fold, n.fh, edit)
    x = inputs(case.kind, kset, N, S)
    dirs = None if case.mode == "SIGMA" else x["dirs"]
    if case.kind == "hashgrid":
        geo, table, _ = grid()
        enc64, bud = HG.encode(geo, x["pts"].double(), table, want_budget=True)
        c = R.Case64(p, case.mode, enc=enc64, dirs=dirs)
        c.enc_budget = bud
        return c
    return R.Case64(p, case.mode, fh=n.fh, dirs=dirs, **({"enc": x["enc"]} if case.kind == "enc" else {"pts": x["pts"]}))


def _dev(t):
    return None if t is None else t.to(DEV)


def _modes():
    from nefes_amd import lib as L
    return {"SIGMA": L.FIELD_SIGMA, "STATIC": L.FIELD_STATIC, "FULL": L.FIELD_FULL}


def launch_fwd(case, pk, x, N, S, via_pts=False, keys=None):
    """the row's forward through its ops launcher -> (raw [M, R] on the host, masks); keys: filled with the timer keys that ran"""
    from nefes_amd import ops
    mode = _modes()[case.mode]
    v = None if case.mode == "SIGMA" else _dev(x["v"])
    want = case.mode != "SIGMA"
    ops.TIMERS = {}
    try:
        if case.kind == "fh":
            raw_t, masks = ops._fh_fwd(pk, _dev(x["o"]), _dev(x["d"]), v, _dev(x["z"]), True)
        elif case.kind == "enc":
            raw_t, masks = ops._field_fwd(pk, mode, N, S, xyz_enc=_dev(x["enc"]), viewdirs=v, want_masks=want)
        elif via_pts:
            raw_t, masks = ops._field_fwd(pk, mode, N, S, pts=_dev(x["pts"]), viewdirs=v, want_masks=want)
        else:
            raw_t, masks = ops._field_fwd(pk, mode, N, S, rays_o=_dev(x["o"]), rays_d=_dev(x["d"]), z=_dev(x["z"]), viewdirs=v, want_masks=want,
                                          grid=grid()[2] if case.kind == "hashgrid" else None)
        if keys is not None:
            keys.update(ops.TIMERS)
    finally:
        ops.TIMERS = None
    return raw_t, masks


def launch_bwd(case, pk, x, N, S, raw_t, G, masks, keys=None):
    """the row's backward -> {d_pts | d_enc, d_viewdirs} per sample on the host.  G [M, R]."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    g_t = G.reshape(N, S, -1).permute(0, 2, 1).contiguous().to(DEV)
    v = _dev(x["v"])
    ops.TIMERS = {}
    try:
        if case.kind == "fh":       # the entry point itself (what ops._fh_bwd launches), for the per-sample gradients
            g_in, g_vs = torch.empty(N * S, 3, device=DEV), torch.empty(N * S, 3, device=DEV)
            ptr, o, d, z = ops._chk, _dev(x["o"]), _dev(x["d"]), _dev(x["z"])          # (named: they must outlive the launch)
            with ops._timed("field_bwd[h3,fh]"):
                L.check(L.load().nefes_field_bwd_h3_fh(pk.desc, ops._blob(pk), N, S, ptr(o, "rays_o"), ptr(d, "rays_d"),
                                                       ptr(z, "z"), ptr(v, "viewdirs"), ptr(raw_t, "raw_t"), ptr(g_t, "g_raw_t"), None,
                                                       ptr(masks, "masks", torch.int32), ptr(g_in, "g_pts"), ptr(g_vs, "g_vs"), ops._stream()),
                        "nefes_field_bwd_h3_fh")
        elif case.kind == "enc":
            g_in, g_vs = ops._field_bwd(pk, _modes()[case.mode], N, S, raw_t, g_t, masks, viewdirs=v, enc=True)
        else:
            g_in, g_vs = ops._field_bwd(pk, _modes()[case.mode], N, S, raw_t, g_t, masks, rays_o=_dev(x["o"]), rays_d=_dev(x["d"]), z=_dev(x["z"]),
                                        viewdirs=v, grid=grid()[2] if case.kind == "hashgrid" else None)
        if keys is not None:
            keys.update(ops.TIMERS)
    finally:
        ops.TIMERS = None
    return {"d_enc" if case.kind == "enc" else "d_pts": g_in.cpu(), "d_viewdirs": g_vs.cpu()}


def flat(raw_t):
    return raw_t.permute(0, 2, 1).reshape(-1, raw_t.shape[1]).cpu()


def expect_route(case, pk, backward, M):
    """(timer key, entry point) the row must run through, from ops.field_route -- the FH pair has its own launchers"""
    from nefes_amd import ops
    if case.kind == "fh":
        return ("field_bwd[h3,fh]", "nefes_field_bwd_h3_fh") if backward else ("field_fwd[full,h3,fh]", "nefes_field_fwd_h3_fh")
    kind = {"rays": "rays", "enc": "enc", "hashgrid": "hashgrid"}[case.kind]
    rt = ops.field_route(pk, _modes()[case.mode], backward, kind, M)
    return rt.key, rt.entry


def assert_selects(case, Cf, pk):
    """nefes_field_h3_instance, asked with the PACK's own description (what the launch hands over), names the case's row"""
    from nefes_amd import lib as L
    desc, backward, mode, flags = R.selects(case, Cf)
    d = pk.desc
    assert (d.width, d.feat_dim, d.has_transient, d.xyz_encoding, d.fold_final) == desc, (case.row, desc)
    fl = 0
    for f in flags:
        fl |= getattr(L, "H3_REQ_" + f)
    name = C.create_string_buffer(96)
    rc = L.load().nefes_field_h3_instance(C.byref(pk.desc), int(backward), _modes()[mode], fl, name, len(name))
    assert rc == 0 and name.value.decode() == case.row, (case.row, Cf, rc, name.value)


ENTRY_OF = {("rays", False): "nefes_field_fwd_h3", ("enc", False): "nefes_field_fwd_h3", ("hashgrid", False): "nefes_field_fwd_h3_hashgrid",
            ("rays", True): "nefes_field_bwd_h3", ("enc", True): "nefes_field_bwd_h3", ("hashgrid", True): "nefes_field_bwd_h3_hashgrid"}


def check_route(case, pk, backward, M, keys):
    key, entry = expect_route(case, pk, backward, M)
    if case.kind != "fh":
        want = "nefes_field_bwd_static_h3" if backward and case.mode == "STATIC" else ENTRY_OF[case.kind, backward]
        assert entry == want, (case.row, entry)
    assert set(keys) == {key}, (case.row, sorted(keys), key)


def masks_of(case, masks, M):
    neg = decode_masks(masks, M, case.network.width)
    return {t: torch.from_numpy(v) for t, v in neg.items()}


def sets_and_shapes(case):
    if case.kind == "hashgrid":
        return [("inside", N, S) for N, S in case.shapes]
    return [(k, N, S) for k in R.INPUT_SETS for N, S in case.shapes]


def jacobian_budget(c, neg, wrt_budget):
    """sum_f |d out[m, c] / d enc[m, f]| E_f [M, R]: the first-order image of the encoding's budget, from the float64 network on the
    pattern `neg` (one backward pass per output channel)."""
    enc = c.e64[0].clone().requires_grad_()
    r = R.run(c.p64, enc, c.e64[1], c.mode, neg)
    cols = []
    for ch in range(r.out.shape[1]):
        (g,) = torch.autograd.grad(r.out[:, ch].sum(), enc, retain_graph=True)
        cols.append((g.abs() * wrt_budget).sum(1))
    return torch.stack(cols, 1)


# ---- forward rows -----------------------------------------------------------------------------------------------------------------------
GROUPS_OF = {"SIGMA": ("static_sigma",), "STATIC": ("static_head", "static_sigma"),
             "FULL": ("static_head", "static_sigma", "transient_rgb", "transient_sigma", "transient_beta")}


def groups_of(case):
    return GROUPS_OF[case.mode] + (("g",) if case.network.fh else ())


@functools.lru_cache(maxsize=None)
def forward_results(case_i, net_i):
    """One network of one forward row, every input set and shape launched ONCE -> dict(structure: [what broke], flips, units,
    groups: {group: [(input set, E_hip, E_ref, worst error / bound)]}).  The tests below each assert one part of it."""
    case = CASES[case_i]
    n = case.network
    Cf, edit = n.nets[net_i]
    broke, flips_total, units_total = [], 0, 0
    if net_i == 0 and not n.fh:
        print(f"[field_samples] {case.row}: C = 0 skipped -- NeRFH_NFF refuses a network without a feature head (field.py _supported); "
              f"the only pack with feat_dim 0 is the factored head's, which is the FH row")
    _, pk = network(n.width, Cf, n.has_transient, n.ext, n.fold, n.fh, edit)
    assert_selects(case, Cf, pk)
    pooled = {}
    for kset, N, S in sets_and_shapes(case):
        x, c = inputs(case.kind, kset, N, S), truth(case_i, net_i, kset, N, S)
        where = (kset, N, S)
        keys = {}
        raw_t, masks = launch_fwd(case, pk, x, N, S, keys=keys)
        check_route(case, pk, False, N * S, keys)
        hip = flat(raw_t)
        assert hip.shape == c.truth.shape
        if not bool(torch.isfinite(hip).all()):
            broke.append((where, "not finite"))
        if n.fh and not bool((hip[:, 3 + n.width // 2] == 1).all()):
            broke.append((where, "the ones channel is not 1"))
        neg = masks_of(case, masks, N * S) if masks is not None else None
        extra = 0
        if case.kind == "hashgrid":
            extra = jacobian_budget(c, None if neg is None else {t: neg[t] for t in c.s_hidden}, c.enc_budget)
            # the documented identity: the fused gather == nefes_hashgrid_fwd followed by the EXTERNAL32 instance, bit for bit
            from nefes_amd import ops
            enc = grid()[2](_dev(x["pts"]))
            two, masks2 = ops._field_fwd(pk, _modes()[case.mode], N, S, xyz_enc=enc, viewdirs=None if case.mode == "SIGMA" else _dev(x["v"]),
                                         want_masks=masks is not None)
            if not torch.equal(two, raw_t):
                broke.append((where, "fused gather differs from nefes_hashgrid_fwd + the EXTERNAL32 instance"))
            # ... and so are the mask words, which the EXTERNAL32 rows hold to the float64 signs on a SUPPLIED encoding (here the
            # float64 side sees another encoding, inside the grid's budget: a sign near zero is not comparable)
            if masks is not None and not torch.equal(masks2, masks):
                broke.append((where, "fused gather: mask words differ from the EXTERNAL32 instance's"))
            neg = None
        e = pooled.setdefault(kset, {"M": 0, "hip": {}, "ref": dict.fromkeys([g for g, _, _ in c.groups], 0.0)})
        e["M"] += N * S
        for g, sl, s in c.groups:
            e["hip"].setdefault(g, []).append(((hip[:, sl].double() - c.truth[:, sl]).abs(), s, extra[:, sl] if torch.is_tensor(extra) else 0))
            e["ref"][g] = max(e["ref"][g], c.e_ref[g])
        # rays path == pts= path, on the exact grid
        if case.kind == "rays":
            raw_p, _ = launch_fwd(case, pk, x, N, S, via_pts=True)
            if not torch.equal(raw_p, raw_t):
                broke.append((where, "rays path != pts= path"))
        # tile position must not matter: a sample alone == the same sample in the batch
        if (N, S) == (7, 33) or case.kind == "hashgrid":
            for m in (ALONE if case.kind != "hashgrid" else ALONE_FUSED):
                ray, smp = divmod(m, S)
                one = {k: (v[m:m + 1] if k in ("pts", "enc", "dirs") else (v[ray:ray + 1, smp:smp + 1] if k == "z" else v[ray:ray + 1]))
                       for k, v in x.items()}
                raw_1, _ = launch_fwd(case, pk, one, 1, 1)
                if not torch.equal(raw_1[0, :, 0], raw_t[ray, :, smp]):
                    broke.append((where, f"sample {m} alone != in the batch"))
        # mask words against the float64 pre-activations: |pre_f64| <= F E_ref_layer s_pre wherever the bit differs from its sign
        if neg is not None:
            k, worst = c.mask_flips(neg)
            flips_total += k
            units_total += sum(c.s_hidden[t].numel() for t in c.s_hidden)
            if worst > 1:
                broke.append((where, f"mask bit flipped at |pre| = {worst:.2f} x (F E_ref s_pre)"))
    groups = {}
    for kset, e in pooled.items():
        if e["M"] < 300 and case.kind != "hashgrid":
            broke.append((kset, f"only {e['M']} samples pooled"))
        for g in e["ref"]:
            e_ref = e["ref"][g]
            # E_hip <= F E_ref (+ the encoding's budget, fused gather only), per element so that the budget adds where it applies
            e_hip = max(float((err / s).max()) for err, s, _ in e["hip"][g])
            over = max(float((err / (R.F * e_ref * s + ex)).max()) for err, s, ex in e["hip"][g])
            print(f"[field_samples] {case.row} C={Cf} {edit} {kset} {g}: E_hip {e_hip:.2e}  E_ref {e_ref:.2e}  ratio {e_hip / e_ref:.2f}  "
                  f"worst error / bound {over:.2f}")
            P.record(f"field_samples[{case.row}]", f"C={Cf} {edit} {kset}: {g}", e_hip=e_hip, e_ref=e_ref, bound=R.F * e_ref, worst_over_bound=over)
            groups.setdefault(g, []).append((kset, e_hip, e_ref, over))
    print(f"[field_samples] {case.row} C={Cf} {edit}: {flips_total} of {units_total} mask bits differ from the float64 sign")
    P.record(f"field_samples[{case.row}]", f"C={Cf} {edit}: mask bits differing from the float64 sign", flips=flips_total, units=units_total)
    return dict(structure=broke, groups=groups, flips=flips_total, units=units_total)


def _params(cases, parts_of):
    out = []
    for case in cases:
        for net_i, (Cf, edit) in enumerate(case.network.nets):
            for part in parts_of(case):
                out.append(pytest.param(CASES.index(case), net_i, part, id=f"{case.row}-C{Cf}-{edit}-{part}"))
    return out


@pytest.mark.parametrize("case_i,net_i,part", _params(FWD, lambda c: ("launch",)))
def test_forward_row_launches_and_masks(case_i, net_i, part):
    """the row's own entry point and instance ran; outputs finite; rays path == pts= path; a sample alone == in the batch; the fused
    gather == nefes_hashgrid_fwd + the EXTERNAL32 instance; mask words within F E_ref s_pre of the float64 signs"""
    r = forward_results(case_i, net_i)
    assert not r["structure"], (CASES[case_i].row, r["structure"])


@pytest.mark.parametrize("case_i,net_i,part", _params(FWD, groups_of))
def test_forward_row_per_sample(case_i, net_i, part):
    """E_hip[g] <= F E_ref[g], F = 3, per output group, pooled over the shapes of each input set"""
    r = forward_results(case_i, net_i)
    bad = [x for x in r["groups"][part] if x[3] > 1]
    assert not bad, (CASES[case_i].row, part, "(input set, E_hip, E_ref, worst error / bound)", bad)


# ---- backward rows ----------------------------------------------------------------------------------------------------------------------
def fwd_case_of(case):
    """the forward row whose masks and raw this backward row is handed"""
    n = case.network
    for i, c in enumerate(CASES):
        m = c.network
        if (c.row.startswith("fwd") and c.mode == case.mode and c.kind == case.kind and
                (m.width, m.head_class, m.ext, m.fold, m.fh) == (n.width, n.head_class, n.ext, n.fold, n.fh)):
            return i, c
    raise KeyError(case.row)


@functools.lru_cache(maxsize=None)
def backward_results(case_i, net_i):
    """One network of one backward row -> dict(structure: [..], outputs: {d_pts | d_enc | d_viewdirs: [(input set, upstream, E_hip,
    E_ref, worst error / bound)]})."""
    case = CASES[case_i]
    n = case.network
    fwd_i, fwd = fwd_case_of(case)
    assert fwd.network.nets == n.nets
    Cf, edit = n.nets[net_i]
    broke = []
    _, pk = network(n.width, Cf, n.has_transient, n.ext, n.fold, n.fh, edit)
    assert_selects(case, Cf, pk)
    pooled = {}
    for kset, N, S in sets_and_shapes(case):
        x, c = inputs(case.kind, kset, N, S), truth(fwd_i, net_i, kset, N, S)
        raw_t, masks = launch_fwd(fwd, pk, x, N, S)
        neg = masks_of(case, masks, N * S)
        neg = {t: neg[t] for t in c.s_hidden}
        Rn = raw_t.shape[1]
        if n.fh:
            Gn = n.width // 2
            ups = R.upstreams(N * S, Rn, (3, 2 + Gn), 4 + Gn, dead=3 + Gn)
        else:
            ups = R.upstreams(N * S, Rn, (3, 2 + Cf), 3 + Cf)
        # one channel at a time: on the plain inputs of one shape; the fused-gather row (one shape, a float64 grid gradient per
        # upstream) on its first network and on the one whose last feature channel sits in the partial k-group (C = 29)
        if not (((N, S) == ONE_CHANNEL_SHAPE and kset == "plain") or (case.kind == "hashgrid" and Cf in (16, 29) and edit != "dead3")):
            ups = ups[:1]
        for name, G in ups:
            keys = {}
            hip = launch_bwd(case, pk, x, N, S, raw_t, G, masks, keys=keys)
            check_route(case, pk, True, N * S, keys)
            raw = flat(raw_t)                              # the backward is handed the forward's outputs: so are both oracles
            t64, t32 = c.backward(torch.float64, neg, G, raw), c.backward(torch.float32, neg, G, raw)
            for k in hip:
                if not bool(torch.isfinite(hip[k]).all()):
                    broke.append((kset, N, S, name, k, "not finite"))
            ref = R.grad_errors({k: v[0] for k, v in t32.items()}, t64)
            for k, e_ref in ref.items():                   # a reference that has lost its own accuracy would accept anything
                if not e_ref < E_REF_MAX:
                    broke.append((kset, N, S, name, k, f"degenerate reference: E_ref {e_ref:.2e}"))
            if case.kind == "hashgrid":
                fused_vs_two_launches(case, pk, x, N, S, raw_t, G, masks, hip, broke, (kset, name))
            extra = {k: 0 for k in hip}
            if case.kind == "hashgrid":
                ref["d_pts"] = ref.pop("d_enc")              # the network's share of d pts: E_ref of d enc
                t64, extra = hashgrid_chain(x, t64)
            for k in hip:
                tv, s = t64[k]
                e = pooled.setdefault((kset, name, k), {"hip": [], "ref": 0.0})
                e["hip"].append(((hip[k].double() - tv).abs(), s, extra[k]))
                e["ref"] = max(e["ref"], ref[k])
    outputs = {}
    z = lambda a, b: torch.where(a == 0, torch.zeros_like(a), a / b)
    for (kset, name, k), e in pooled.items():
        e_ref = e["ref"]
        e_hip = max(float(z(err, s).max()) for err, s, _ in e["hip"])
        over = max(float(z(err, R.F * e_ref * s + ex).max()) for err, s, ex in e["hip"])
        print(f"[field_samples] {case.row} C={Cf} {edit} {kset} upstream {name} {k}: E_hip {e_hip:.2e}  E_ref {e_ref:.2e}  "
              f"ratio {e_hip / max(e_ref, 1e-300):.2f}  worst error / bound {over:.2f}")
        P.record(f"field_samples[{case.row}]", f"C={Cf} {edit} {kset} upstream {name}: {k}", e_hip=e_hip, e_ref=e_ref, bound=R.F * e_ref,
                 worst_over_bound=over)
        outputs.setdefault(k, []).append((kset, name, e_hip, e_ref, over))
    return dict(structure=broke, outputs=outputs)


def outputs_of(case):
    return ("d_enc" if case.kind == "enc" else "d_pts", "d_viewdirs")


@pytest.mark.parametrize("case_i,net_i,part", _params(BWD, lambda c: ("launch",)))
def test_backward_row_launches(case_i, net_i, part):
    r = backward_results(case_i, net_i)
    assert not r["structure"], (CASES[case_i].row, r["structure"])


@pytest.mark.parametrize("case_i,net_i,part", _params(BWD, outputs_of))
def test_backward_row_per_sample(case_i, net_i, part):
    """E_hip <= F E_ref per sample for d pts / d enc and d viewdirs, on the row's own forward's masks and raw: a dense upstream at every
    shape and input set, one upstream channel at a time on the plain (5, 64) batch"""
    r = backward_results(case_i, net_i)
    bad = [x for x in r["outputs"][part] if x[4] > 1]
    assert not bad, (CASES[case_i].row, part, "(input set, upstream, E_hip, E_ref, worst error / bound)", bad)


def fused_vs_two_launches(case, pk, x, N, S, raw_t, G, masks, hip, broke, where):
    """The fused backward against what it replaces: the EXTERNAL32 instance's d enc chained through nefes_hashgrid_bwd_x, on the same
    raw and masks.  Recorded whether bit-identical; held to the grid gradient's own budget (both sides carry it once), which is what
    tells a wrong NETWORK share apart here: the bound of the float64 comparison is dominated by that budget."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    geo, table, g = grid()
    g_t = G.reshape(N, S, -1).permute(0, 2, 1).contiguous().to(DEV)
    g_enc, g_vs = ops._field_bwd(pk, L.FIELD_FULL, N, S, raw_t, g_t, masks, viewdirs=_dev(x["v"]), enc=True)
    pts = _dev(x["pts"])
    g_x = torch.empty_like(pts)
    L.check(L.load().nefes_hashgrid_bwd_x(g.desc, ops._chk(g.table, "table"), N * S, ops._chk(pts, "x"), ops._chk(g_enc, "g_enc"),
                                          ops._chk(g_x, "g_x"), ops._stream()), "nefes_hashgrid_bwd_x")
    same = torch.equal(g_x.cpu(), hip["d_pts"]) and torch.equal(g_vs.cpu(), hip["d_viewdirs"])
    _, bud = HG.grad_x(geo, x["pts"].double(), table, g_enc.cpu().double())
    over = float(((g_x.cpu().double() - hip["d_pts"].double()).abs() / (2 * bud)).max())
    P.record(f"field_samples[{case.row}]", f"{where}: fused d pts vs EXTERNAL32 backward + nefes_hashgrid_bwd_x", bit_identical=float(same),
             worst_over_two_budgets=over)
    print(f"[field_samples] {case.row} {where}: fused backward vs two launches: bit-identical {same}, worst difference / (2 x grid budget) {over:.3f}")
    if not torch.equal(g_vs.cpu(), hip["d_viewdirs"]):
        broke.append((where, "fused d viewdirs differs from the EXTERNAL32 instance's"))
    if over > 1:
        broke.append((where, f"fused d pts {over:.2f} x two grid budgets away from EXTERNAL32 backward + nefes_hashgrid_bwd_x"))


def hashgrid_chain(x, t64):
    """The fused backward hands back d pts = (d enc) chained through the grid.  Truth: tests/hashgrid_ref.py's float64 grad_x of the float64
    d enc.  The network's share of the bound, F E_ref s_enc per element of d enc, reaches coordinate k of d pts through
    sum_f |d g_x[k] / d g_enc[f]| (grad_x is linear in g_enc: _grid_gain); grad_x's own budget is added to it."""
    geo, table, _ = grid()
    pts = x["pts"].double()
    gx64, bud = HG.grad_x(geo, pts, table, t64["d_enc"][0])
    return {"d_pts": (gx64, t64["d_enc"][1] * _grid_gain(pts.shape[0])), "d_viewdirs": t64["d_viewdirs"]}, {"d_pts": bud, "d_viewdirs": 0}


@functools.lru_cache(maxsize=None)
def _grid_gain(N):
    """sum_f |d g_x[k] / d g_enc[f]| [M, 3] at the fused-gather rows' points (it does not depend on the upstream)"""
    geo, table, _ = grid()
    pts = inputs("hashgrid", "inside", N, 1)["pts"].double()
    gain = torch.zeros(N, 3, dtype=torch.float64)
    for l in range(geo.n_levels):               # HG.grad_x's g_l, one unit upstream feature at a time, without the thirty-two calls
        t = HG.level_terms(geo, l, pts)
        f = table.double()[t["idx"]]                                      # [M, 8, 2]
        for k in range(3):
            gain[:, k] += t["s"] * ((t["sg"][None, :, k] * HG._others(t["a"], k))[..., None] * f).sum(1).abs().sum(-1)
    return gain
