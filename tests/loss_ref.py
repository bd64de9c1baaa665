"""The training step's five losses as plain torch expressions, in whatever dtype and on whatever device the inputs have: the yardstick
of the train-loss kernels (csrc/losses.hip) at shapes the fixture tests/golden/losses.npz does not hold.  tests/test_losses_golden.py
holds this file to that fixture, which the reference's own classes wrote.

    t = rgb target; every mean runs over all elements of its tensor
    color                     coef (mse(rgb_fine, t) [+ mse(rgb_coarse, t)])
    color_feat                (mse fine [+ mse coarse],  f(feat_fine) [+ f(feat_coarse)])                 coef unused
    color_feat_fusion         the same; color_only_switch: the colour alone; switch_on: + f(feat_fusion)
                              f = L1, MSE, or with cos_loss 1 - mean_n cos(a_n, b_n) over the channels (each norm clamped at 1e-8)
    nerfw                     coef (c_l + f_l [+ b_l + s_l]):  c_l = mean((rgb_coarse - t)^2) / 2;  f_l = mean((rgb_fine - t)^2) / 2, or
                              with beta mean((rgb_fine - t)^2 / (2 beta^2)), b_l = 3 + mean(log beta), s_l = lambda_u mean(transient_sigmas)
    color_feat_fusion_nerfw   nerfw for the colour, L1 / MSE feature terms as color_feat_fusion
"""
import torch
import torch.nn.functional as F

CLASSES = ['color', 'color_feat', 'nerfw', 'color_feat_fusion', 'color_feat_fusion_nerfw']
NAMES = ['rgb_fine', 'rgb_coarse', 'beta', 'transient_sigmas', 'feat_fine', 'feat_coarse', 'feat_fusion']
WEIGHTS = (1.0, 0.02, 0.02)           # run_nefes.py:240-243: loss + 0.02 loss_f + 0.02 loss_fusion


def mse(a, b):
    return ((a - b) ** 2).mean()


def feat_term(kind, a, b):
    if kind == 'l1':
        return (a - b).abs().mean()
    if kind == 'cos':
        return 1 - F.cosine_similarity(a, b, dim=1, eps=1e-8).mean()
    return mse(a, b)


def plain_colour(inputs, t):
    loss = mse(inputs['rgb_fine'], t)
    if 'rgb_coarse' in inputs:
        loss = loss + mse(inputs['rgb_coarse'], t)
    return loss


def nerfw_colour(inputs, t, coef=1, lambda_u=0.01):
    terms = [0.5 * mse(inputs['rgb_coarse'], t)]
    if 'rgb_fine' in inputs:
        sq = (inputs['rgb_fine'] - t) ** 2
        if 'beta' not in inputs:
            terms.append(0.5 * sq.mean())
        else:
            beta = inputs['beta']
            terms += [(sq / (2 * beta.unsqueeze(1) ** 2)).mean(), 3 + torch.log(beta).mean(), lambda_u * inputs['transient_sigmas'].mean()]
    return sum(coef * v for v in terms)


def evaluate(name, inputs, rgb_t, feat_t=None, coef=1, L1_loss=False, cos_loss=False, lambda_u=0.01, switch_on=True, color_only_switch=False):
    """What loss_dict[name](...)(inputs, targets, ...) returns, always as a tuple."""
    if name == 'color':
        return (coef * plain_colour(inputs, rgb_t),)
    if name == 'nerfw':
        return (nerfw_colour(inputs, rgb_t, coef, lambda_u),)
    colour = nerfw_colour(inputs, rgb_t, coef, lambda_u) if name == 'color_feat_fusion_nerfw' else plain_colour(inputs, rgb_t)
    if name != 'color_feat' and color_only_switch:
        return (colour,)
    kind = 'l1' if L1_loss else ('cos' if (cos_loss and name == 'color_feat_fusion') else 'mse')
    loss_f = feat_term(kind, inputs['feat_fine'], feat_t)
    if 'feat_coarse' in inputs:
        loss_f = loss_f + feat_term(kind, inputs['feat_coarse'], feat_t)
    if name != 'color_feat' and switch_on:
        return colour, loss_f, feat_term(kind, inputs['feat_fusion'], feat_t)
    return colour, loss_f


def total(ret, weights=WEIGHTS):
    return sum(w * r for w, r in zip(weights, ret))


def run(name, kw, base, keys, dtype=None, device=None, weights=WEIGHTS):
    """evaluate() on fresh leaves made of base[k] for k in keys, and the gradients of total(): (returned scalars, {name: gradient})."""
    conv = lambda v: v.detach().to(device=device, dtype=dtype).clone()
    inputs = {k: conv(base[k]).requires_grad_() for k in NAMES if k in keys}
    feat_t = conv(base['feat_target']) if 'feat_target' in base else None
    ret = evaluate(name, inputs, conv(base['rgb_target']), feat_t, **kw)
    total(ret, weights).backward()
    return [r.detach() for r in ret], {k: v.grad for k, v in inputs.items() if v.grad is not None}


def fixture_cases(z):
    """The cases of tests/golden/losses.npz: (index, class name, evaluate() keywords, names of the inputs present)."""
    out = []
    i = 0
    while f"case{i}.cfg" in z:
        cls, coef, l1, cos, lam, sw, co = [float(v) for v in z[f"case{i}.cfg"]]
        mask = int(z[f"case{i}.keys"])
        keys = [n for k, n in enumerate(NAMES) if mask >> k & 1]
        name = CLASSES[int(cls)]
        kw = dict(coef=coef, L1_loss=bool(l1), cos_loss=bool(cos), lambda_u=lam, switch_on=bool(sw), color_only_switch=bool(co))
        out.append((i, name, kw, keys))
        i += 1
    return out
