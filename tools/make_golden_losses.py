#!/usr/bin/env python3
"""Generate tests/golden/losses.npz by running the REFERENCE's own loss classes (script/models/losses.py:4-173) on the CPU: every class
of its loss_dict, every switch, with and without the optional inputs, once in float32 and once on the same inputs in float64.

    N = 37 rays, C = 5 feature channels, S = 7 transient samples; a few exact ties a == b planted for the L1 loss

One set of inputs serves every case (`in.<name>`, float32).  Per case i (numeric arrays only):
    case<i>.cfg     [class index in CLASSES, coef, L1_loss, cos_loss, lambda_u, switch_on, color_only_switch]
    case<i>.keys    bit k set = NAMES[k] is in the `inputs` dict
    case<i>.out     the returned scalars (float32 run);  case<i>.out_f64  the float64 run
    case<i>.g.<name> / case<i>.g.<name>_f64   gradient of  loss + 0.02 loss_f + 0.02 loss_fusion  (run_nefes.py:240-243) to that input
tests/test_losses_golden.py pins tests/loss_ref.py on it; the GPU tests compare the kernels with the *_f64 values.

Usage:  python tools/make_golden_losses.py [reference root]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, REF  # noqa: E402

N, C, S = 37, 5, 7
CLASSES = ['color', 'color_feat', 'nerfw', 'color_feat_fusion', 'color_feat_fusion_nerfw']       # tests/loss_ref.py has the same lists
NAMES = ['rgb_fine', 'rgb_coarse', 'beta', 'transient_sigmas', 'feat_fine', 'feat_coarse', 'feat_fusion']
ALL = set(NAMES)


def cases():
    """(class, ctor kwargs, forward kwargs, keys left out of `inputs`)"""
    out = []
    nw = {'beta', 'transient_sigmas'}
    for coef, drop in ((1, set()), (0.7, {'rgb_coarse'})):
        out.append(('color', dict(coef=coef), {}, drop | nw))
    for l1 in (False, True):
        for drop in (set(), {'rgb_coarse', 'feat_coarse'}):
            out.append(('color_feat', dict(coef=1, L1_loss=l1), {}, drop | nw))
    out += [('nerfw', dict(coef=1, lambda_u=0.01), {}, set()), ('nerfw', dict(coef=0.5, lambda_u=0.03), {}, set()),
            ('nerfw', dict(coef=1, lambda_u=0.01), {}, nw), ('nerfw', dict(coef=2.0, lambda_u=0.01), {}, {'rgb_fine'})]
    switches = [dict(switch_on=True, color_only_switch=False), dict(switch_on=False, color_only_switch=False),
                dict(switch_on=False, color_only_switch=True), dict(switch_on=True, color_only_switch=True)]
    for kind in (dict(L1_loss=True), dict(), dict(cos_loss=True)):
        for k, sw in enumerate(switches):
            drop = {'feat_coarse'} if k == 1 else ({'rgb_coarse'} if k == 2 else set())
            out.append(('color_feat_fusion', dict(coef=1, **kind), sw, drop | nw))
    out.append(('color_feat_fusion', dict(coef=1, cos_loss=True), switches[0], {'feat_coarse', 'rgb_coarse'} | nw))
    for l1 in (True, False):
        for k, sw in enumerate(switches):
            drop = {'feat_coarse'} if k == 1 else (nw if k == 3 else set())
            out.append(('color_feat_fusion_nerfw', dict(coef=1 if l1 else 0.8, L1_loss=l1, lambda_u=0.01 if l1 else 0.02), sw, drop))
    out.append(('color_feat_fusion_nerfw', dict(coef=1, L1_loss=True, lambda_u=0.01), switches[0], nw | {'feat_coarse'}))
    return out


def run(mod, case, base, dtype):
    name, ctor, fwd, drop = case
    inputs = {k: base[k].to(dtype).clone().requires_grad_() for k in NAMES if k not in drop}
    rgb_t, feat_t = base['rgb_target'].to(dtype), base['feat_target'].to(dtype)
    fn = mod.loss_dict[name](**ctor)
    if name in ('color', 'nerfw'):
        ret = fn(inputs, rgb_t)
    else:
        ret = fn(inputs, {'rgb': rgb_t} if fwd.get('color_only_switch') else {'rgb': rgb_t, 'feat': feat_t}, **fwd)
    ret = ret if isinstance(ret, tuple) else (ret,)
    total = ret[0] + sum(0.02 * r for r in ret[1:])
    total.backward()
    return [r.detach() for r in ret], {k: v.grad for k, v in inputs.items() if v.grad is not None}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(ref, "script", "models", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.stdout, keep = open(os.devnull, "w"), sys.stdout          # the constructors print which feature loss they use
    try:
        spec.loader.exec_module(mod)
        torch.set_num_threads(1)
        g = torch.Generator().manual_seed(2024)
        base = {'rgb_fine': torch.rand(N, 3, generator=g), 'rgb_coarse': torch.rand(N, 3, generator=g), 'rgb_target': torch.rand(N, 3, generator=g),
                'beta': 0.3 + torch.rand(N, generator=g), 'transient_sigmas': 2.0 * torch.rand(N, S, generator=g),
                'feat_fine': torch.randn(N, C, generator=g), 'feat_coarse': torch.randn(N, C, generator=g),
                'feat_fusion': torch.randn(N, C, generator=g), 'feat_target': torch.randn(N, C, generator=g)}
        for k, (r, c) in (('feat_fine', (0, 0)), ('feat_fine', (36, 4)), ('feat_coarse', (5, 2)), ('feat_fusion', (17, 3)), ('feat_fusion', (36, 0))):
            base[k][r, c] = base['feat_target'][r, c]              # exact ties: L1's gradient there is 0
        out = {"in." + k: v.numpy() for k, v in base.items()}
        for i, case in enumerate(cases()):
            name, ctor, fwd, drop = case
            out[f"case{i}.cfg"] = np.array([CLASSES.index(name), ctor.get('coef', 1), ctor.get('L1_loss', False), ctor.get('cos_loss', False),
                                            ctor.get('lambda_u', 0.01), fwd.get('switch_on', True), fwd.get('color_only_switch', False)], np.float64)
            out[f"case{i}.keys"] = np.array(sum(1 << k for k, n in enumerate(NAMES) if n not in drop), np.int64)
            for dtype, tag in ((torch.float32, ""), (torch.float64, "_f64")):
                ret, grads = run(mod, case, base, dtype)
                out[f"case{i}.out{tag}"] = torch.stack(ret).numpy()
                for k, v in grads.items():
                    out[f"case{i}.g.{k}{tag}"] = v.numpy()
    finally:
        sys.stdout = keep
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(cases()), "cases")


if __name__ == "__main__":
    main()
