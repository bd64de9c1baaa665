"""The loss classes of the reference's training step (script/models/losses.py:4-173) on the library's kernels: two launches forward and
one backward per call (ops.TrainLoss, csrc/losses.hip) where the torch expressions take several dozen.

Same class names, constructor and forward signatures and return arity as the reference's, and a `loss_dict` with its five keys:

    from nefes_amd.losses import loss_dict
    loss_func = loss_dict['color_feat_fusion_nerfw'](coef=1, L1_loss=True)
    loss_rgb, loss_f, loss_fusion = loss_func(results, {'rgb': target_s, 'feat': target_f}, switch_on=True)

`install()` puts these classes into the reference's own `models.losses.loss_dict`, so an unmodified training script picks them up;
`python -m nefes_amd.run_reference` does that when NEFES_HIP_LOSSES=1 (off by default: nothing changes anywhere).  Inputs are float32
GPU tensors; there is no CPU path.  Sums are float64 in a fixed order: the same inputs give the same bits.
"""
import importlib
import os

from torch import nn

from . import lib as L
from . import ops

ENABLED = os.environ.get("NEFES_HIP_LOSSES", "0") == "1"


def _rows(t, width=None):
    if t is None:
        return None
    return t.reshape(-1) if width is None else t.reshape(-1, width)


def _launch(inputs, rgb_target, feat_target, nerfw, feat_kind, coef, lambda_u, feats, fusion):
    """One ops.TrainLoss call on the reference's `inputs` dict.  feats / fusion: whether loss_f / loss_fusion are asked for; the feature
    keys are not touched otherwise."""
    if nerfw:
        rgb_coarse = inputs['rgb_coarse']                               # required, as in the reference (KeyError)
        rgb_fine = inputs.get('rgb_fine')
        beta = inputs['beta'] if (rgb_fine is not None and 'beta' in inputs) else None
        sigmas = inputs['transient_sigmas'] if beta is not None else None
    else:
        rgb_fine = inputs['rgb_fine']
        rgb_coarse = inputs.get('rgb_coarse')
        beta = sigmas = None
    f_fine = f_coarse = f_fusion = f_target = None
    Cc = None
    if feats:
        f_fine = inputs['feat_fine']
        Cc = f_fine.shape[-1]
        f_target = _rows(feat_target, Cc)
        f_coarse = inputs.get('feat_coarse')
        if fusion:
            f_fusion = inputs['feat_fusion']
    if sigmas is not None and sigmas.dim() != 2:
        sigmas = sigmas.reshape(-1, sigmas.shape[-1])
    return ops.TrainLoss.apply(_rows(rgb_fine, 3), _rows(rgb_coarse, 3), _rows(rgb_target, 3), _rows(beta), sigmas, _rows(f_fine, Cc),
                               _rows(f_coarse, Cc), _rows(f_fusion, Cc), f_target, bool(nerfw), feat_kind, coef, lambda_u)


def _feat_kind(L1_loss, cos_loss=False):
    return L.LOSS_FEAT_L1 if L1_loss else (L.LOSS_FEAT_COS if cos_loss else L.LOSS_FEAT_MSE)


class ColorLoss(nn.Module):
    """coef (mse(rgb_fine, t) [+ mse(rgb_coarse, t)])"""

    def __init__(self, coef=1):
        super().__init__()
        self.coef = coef

    def forward(self, inputs, targets):
        return _launch(inputs, targets, None, False, L.LOSS_FEAT_MSE, self.coef, 0.0, False, False)[0]


class ColorFeatureLoss(nn.Module):
    """(mse fine [+ mse coarse], f(feat_fine) [+ f(feat_coarse)]), f = L1 or MSE; `coef` is unused, as in the reference"""

    def __init__(self, coef=1, L1_loss=False):
        super().__init__()
        self.coef = coef
        self.feat_kind = _feat_kind(L1_loss)

    def forward(self, inputs, targets):
        loss, loss_f, _, _ = _launch(inputs, targets['rgb'], targets['feat'], False, self.feat_kind, 1.0, 0.0, True, False)
        return loss, loss_f


class ColorFeatureFusionLoss(nn.Module):
    """Colour as ColorFeatureLoss; f = L1, or the cosine loss 1 - mean_n cos(a_n, b_n), or MSE.  color_only_switch: the colour loss alone;
    switch_on: the fusion term too.  Both L1_loss and cos_loss set is `1 - L1` in the reference, which no script asks for: refused."""

    def __init__(self, coef=1, L1_loss=False, cos_loss=False):
        super().__init__()
        if L1_loss and cos_loss:
            raise ValueError("nefes_amd.losses.ColorFeatureFusionLoss: L1_loss and cos_loss together are not supported")
        self.coef = coef
        self.cos_loss = cos_loss
        self.feat_kind = _feat_kind(L1_loss, cos_loss)

    def forward(self, inputs, targets, switch_on=True, color_only_switch=False):
        if color_only_switch == True:  # noqa: E712  (the reference's comparison: a truthy non-bool does not count)
            return _launch(inputs, targets['rgb'], None, False, self.feat_kind, 1.0, 0.0, False, False)[0]
        loss, loss_f, loss_fusion, _ = _launch(inputs, targets['rgb'], targets['feat'], False, self.feat_kind, 1.0, 0.0, True,
                                               bool(switch_on))
        return (loss, loss_f, loss_fusion) if switch_on else (loss, loss_f)


class NerfWLoss(nn.Module):
    """Equation 13 of NeRF-W: coef (c_l + f_l [+ b_l + s_l]); `rgb_coarse` is required."""

    def __init__(self, coef=1, lambda_u=0.01):
        super().__init__()
        self.coef = coef
        self.lambda_u = lambda_u

    def forward(self, inputs, targets, loss_mode=0):
        return _launch(inputs, targets, None, True, L.LOSS_FEAT_MSE, self.coef, self.lambda_u, False, False)[0]


class ColorFeatureFusionNerfWLoss(nn.Module):
    """NerfWLoss for the colour, then L1 / MSE feature terms as ColorFeatureFusionLoss."""

    def __init__(self, coef=1, L1_loss=False, lambda_u=0.01):
        super().__init__()
        self.coef = coef
        self.lambda_u = lambda_u
        self.feat_kind = _feat_kind(L1_loss)

    def forward(self, inputs, targets, switch_on=True, color_only_switch=False):
        if color_only_switch == True:  # noqa: E712
            return _launch(inputs, targets['rgb'], None, True, self.feat_kind, self.coef, self.lambda_u, False, False)[0]
        loss, loss_f, loss_fusion, _ = _launch(inputs, targets['rgb'], targets['feat'], True, self.feat_kind, self.coef, self.lambda_u, True,
                                               bool(switch_on))
        return (loss, loss_f, loss_fusion) if switch_on else (loss, loss_f)


loss_dict = {'color': ColorLoss,
             'color_feat': ColorFeatureLoss,
             'nerfw': NerfWLoss,
             'color_feat_fusion': ColorFeatureFusionLoss,
             'color_feat_fusion_nerfw': ColorFeatureFusionNerfWLoss}


def install(module=None):
    """Replace the VALUES of `module.loss_dict` (default: the reference's `models.losses`, as the search path resolves it) by the classes
    above, in place: `from models.losses import loss_dict` in an unmodified script then constructs the kernel classes.  The module object,
    its file and everything else in it stay the reference's.  Returns the module."""
    if module is None:
        module = importlib.import_module("models.losses")
    target = module.loss_dict
    missing = set(loss_dict) - set(target)
    if missing:
        raise RuntimeError(f"nefes_amd.losses.install: {module.__name__}.loss_dict has no {sorted(missing)}")
    for k, cls in loss_dict.items():
        target[k] = cls
    return module
