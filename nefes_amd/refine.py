"""Per-image pose refinement loop around the HIP render path.

Mirrors the inner loop of script/dm/DFM_pose_refine.py:290-348 (`DFM_optimization_NFF`, `--pose_only 3`) and of
script/dm/DFM_APR_refine.py:84-156 (`train_on_batch`):

    LearnPose(cam) -> fix_coord_supp -> render(H/ts, W/ts, focal/ts, c2w) -> affine_color_transform(hist)
        -> run_fusion_net -> [bicubic upsample + 10 px crop] -> 1 - mean cosine similarity -> backward -> Adam

The reference runs the 50 iterations of one image as 50 eager Python passes (~150 launches each).  `PoseRefiner`
captures ONE iteration -- forward, backward and the Adam update -- into a HIP graph on first use and replays it, so the
loop's cost is the kernels' and not the host's; per-image state (pose delta, Adam moments, target features, histogram)
lives in static device buffers that are reset in place.  The bicubic up-sampling runs on ops.BicubicUpsample (gather
backward; the library's atomic scatter backward was 40 % of an iteration).  No CPU fallback anywhere on the path.
"""
import os
import typing

import torch
import torch.nn as nn

from . import ops
from .pose import LearnPose
from .render import render, render_poses


def fix_coord_supp(pose, world_setup_dict, device=None):
    """dm/direct_pose_model.py:210-232: APR/COLMAP translation -> NeRF scale, `t' = (t*sc + move)*sc2`.
    Out of place (the reference mutates a clone), constants as device scalars so the chain is graph-capturable."""
    sc, sc2 = float(world_setup_dict['pose_scale']), float(world_setup_dict['pose_scale2'])
    mv = [float(v) * sc2 for v in world_setup_dict['move_all_cam_vec']]
    t = pose[..., :3, 3] * (sc * sc2)
    t = torch.stack([t[..., 0] + mv[0], t[..., 1] + mv[1], t[..., 2] + mv[2]], -1)
    return torch.cat([pose[..., :3, :3], t[..., None]], -1)


def feature_loss(feature_rgb, feature_target, img_in=True, per_pixel=False):
    """dm/DFM_pose_refine.py:211-233: 1 - mean cosine similarity (per channel over pixels, or per pixel over channels)."""
    if img_in:
        C = feature_rgb.shape[0]
        feature_rgb, feature_target = feature_rgb.reshape(C, -1), feature_target.reshape(C, -1)
    cos = nn.CosineSimilarity(dim=0 if per_pixel else 1, eps=1e-6)
    return 1 - cos(feature_rgb, feature_target).mean()


def masked_feature_loss(feature_rgb, feature_target, mask, img_in=True, per_pixel=False):
    """dm/DFM_pose_refine.py:257-288 (`--semantic`): feature_loss over the pixels with mask > 0 only -- in SELECT form: the reference
    compacts both maps with torch.nonzero (a host read, and shapes that change per image: nothing a captured loop can replay); here the
    masked-out pixels are replaced by zeros, which add nothing to the three sums of a channel (per channel: the same value), and the
    per-pixel mean is sum_p m_p cos_p / sum_p m_p.  Values at masked-out pixels never reach the result or a gradient (torch.where
    selects, forward and backward).  No valid pixel: 1 per channel-wise (every cosine is 0 / eps^2), NaN per pixel (0 / 0), as the
    reference.  mask: [1,H,W], [H,W] or flat, any dtype."""
    if img_in:
        C = feature_rgb.shape[0]
        feature_rgb, feature_target = feature_rgb.reshape(C, -1), feature_target.reshape(C, -1)
    valid = (mask.reshape(1, -1) > 0).to(feature_rgb.device)
    fr = torch.where(valid, feature_rgb, torch.zeros((), dtype=feature_rgb.dtype, device=feature_rgb.device))
    ft = torch.where(valid, feature_target, torch.zeros((), dtype=feature_target.dtype, device=feature_target.device))
    if not per_pixel:
        return 1 - nn.CosineSimilarity(dim=1, eps=1e-6)(fr, ft).mean()
    cos = nn.CosineSimilarity(dim=0, eps=1e-6)(fr, ft)
    cos = torch.where(valid[0], cos, torch.zeros((), dtype=cos.dtype, device=cos.device))
    return 1 - cos.sum() / valid.sum().to(cos.dtype)


def full_resolution_mask(mask_lowres, size, crop=10):
    """The loader's (H/ts, W/ts) mask of static pixels in the form the `upsample=True` loop compares at: nearest-neighbour up-sampling
    to size = (H, W), `crop` pixels dropped on every side, thresholded (> 0) to uint8 [H-2crop, W-2crop] (a leading batch dimension is
    kept).  Plain torch, once per image."""
    H, W = int(size[0]), int(size[1])
    m = torch.as_tensor(mask_lowres)
    lead = m.shape[:-2]
    m = (m.reshape((-1, 1) + tuple(m.shape[-2:])) > 0).float()
    m = nn.functional.interpolate(m, size=(H, W), mode="nearest")[:, 0, crop:H - crop, crop:W - crop]
    return (m > 0).to(torch.uint8).reshape(tuple(lead) + tuple(m.shape[-2:])).contiguous()


HIP_SVD_REG = os.environ.get("NEFES_HIP_SVD_REG", "1") != "0"


def svd_reg(pose):
    """dm/DFM_pose_refine.py:119-129: the 3x3 block of a regressed [B,3,4] pose replaced by its nearest rotation U V^T.
    Out of place (the reference writes into its argument).  fp32 poses on the GPU take ops.svd_reg (one launch each way, float64 inside,
    the polar factor's own derivative -- torch.svd there is a solver call plus a backward that divides by sigma_i^2 - sigma_j^2, ~0 for
    a near-rotation, and nothing of it can be captured into the iteration's graph); HIP_SVD_REG = False keeps the torch expression."""
    if HIP_SVD_REG and pose.is_cuda and pose.dtype == torch.float32:
        return ops.svd_reg(pose)
    u, _, v = torch.svd(pose[..., :3, :3])
    return torch.cat([u @ v.transpose(-2, -1), pose[..., :3, 3:]], -1)


def img2mse(x, y):
    return torch.mean((x - y) ** 2)


def mse2psnr(x):
    """models/nerfh.py: -10 log10(mse)."""
    return -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))


def ssim_map(x, y):
    """utils/utils.py:15-49 (`SSIM`): 7x7 mean filters on reflection-padded images, clamped to [0, 1]."""
    F = nn.functional
    x, y = F.pad(x, (3, 3, 3, 3), mode="reflect"), F.pad(y, (3, 3, 3, 3), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 7, 1)
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x ** 2) - mx ** 2, pool(y ** 2) - my ** 2, pool(x * y) - mx * my
    n = (2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)
    d = (mx ** 2 + my ** 2 + 0.01 ** 2) * (sx + sy + 0.03 ** 2)
    return torch.clamp(n / d, 0, 1)


class FeatureLoss(nn.Module):
    """dm/DFM_pose_refine.py:236-255."""

    def __init__(self, img_in=True, per_pixel=False):
        super().__init__()
        self.img_in, self.per_pixel = img_in, per_pixel

    def forward(self, feature_rgb, feature_target):
        return feature_loss(feature_rgb, feature_target, self.img_in, self.per_pixel)


class PoseRefiner:
    """`refine(init_c2w, feature_target, hist, iters)` -> (refined 4x4 c2w, losses [iters]) for one query image, or for
    `images=B` of them side by side (see refine()).

    hwf: full-resolution (H, W, focal); the render runs at 1/tinyscale.  `upsample=True` is the APR variant (bicubic
    upsample of the fused features to (H, W) and a 10-pixel crop; `feature_target` is [C, H, W]); False is the
    DFM_pose_refine variant (`feature_target` is [C, H/ts, W/ts]).  `world_setup` = dict(pose_scale, pose_scale2,
    move_all_cam_vec) or None.  `graph=True` replays one captured HIP graph per iteration.

    `pose_model=` selects `train_on_batch` proper (DFM_APR_refine.py:84-156, `pose_only=2`): the pose is what a regression
    network predicts from the query image (`pose_model(img)` -> [1,12] or [1,3,4]; `svd_reg=True` as config_stairs_DFM.txt:22),
    the optimizer is Adam(lr=`learning_rate`) over a deep copy of that network per image (:209-212), and `refine_apr` returns what
    `DFM_post_processing` records for the image: the refined network's pose, or the initial one when the verification step
    finds PSNR or SSIM of the up-sampled render lower after the loop than before (:233-250).  The network itself is the
    caller's (a CNN outside this path); implies `upsample=True`.

    `masked=True` is the reference's `--semantic` (masked_feature_loss, dm/DFM_pose_refine.py:257-288): the feature loss runs over the
    pixels of the image's mask that are > 0 -- `refine(..., mask=)` / `refine_apr(..., mask=)`, in the target's spatial shape -- on the
    masked loss kernels, in every form of the loop; no mask given means all valid.

    `sparse=K` is the mode the reference announces as `--sparse_feature` and never built (dm/options.py:131-136): the LearnPose loop over K
    pixels instead of a frame -- pose -> render(pixels=self.pixels) -> feat_map [K, C] -> [C, K] -> feature loss against the target's
    features sampled at the same pixels; no colour transform and no FusionNet (the reference's non-fusion branch,
    DFM_pose_refine.py:330-333, with img_in=False).  `refine(..., pixels=)` takes the [K, 2] points (x, y) of the rendered (h, w) frame
    (None: K distinct integer pixels drawn with a generator seeded by `seed=`, among the mask's valid ones on a masked refiner);
    `set_pixels` moves them in place, and a captured iteration follows.

    `redraw=R` (with sparse=K) draws a fresh batch every R iterations, as iNeRF-style optimisers do: the iteration begins with
    ops.draw_pixels -- K distinct pixels, uniform among the mask's valid ones, drawn on the device from the persistent words
    `draw_state` = {seed, tick} -- and a re-sample of the target there, both inside the captured graph: no host read per image or per
    iteration.  Every image starts from {seed=, 0}: its batches depend on (seed, mask) alone.  Such a refiner takes no `pixels=` and no
    `set_pixels`.  None (default): the fixed list described above.

    `depth_weight=lambda` (with `depth_huber=delta`, the Huber threshold in the scene's units; None: 0.1) adds the geometric term of an
    RGB-D query to the loss: lambda * ops.depth_loss(the iteration's disp_map, the image's measured depth) -- `refine(..., depth=)` /
    `refine_apr(..., depth=)`, z-depth in the units of near / far at the rendered frame's resolution [h, w] (images=B: [B, h, w]; holes
    are 0, Inf or NaN; a sparse refiner samples the frame at its pixels, nearest, with redraw=R inside the captured iteration).  Only
    depth validity counts for it -- `mask=` stays the feature term's.  `refiner.loss` is the total, `refiner.depth_loss` the term's last
    value (float64, lambda not applied).  None (default): exactly the refiner without the term."""

    FUSED_UPSAMPLED_LOSS = True      # False: bicubic up-sampling and cosine loss as separate kernels (the tests compare the two)
    # The loop's target is fixed for all iterations of an image: its share of the up-sampled loss (Uy^T target Ux, |target|^2) is
    # computed when the target is set and an iteration runs on [C,h,w] data only (ops.UpcosTarget; csrc/feature_loss.hip upcos_gram_*).
    # False: the one-pass kernels that read the whole target every iteration (the tests compare the two).
    PREPARED_TARGET = os.environ.get("NEFES_PREPARED_TARGET", "1") != "0"
    # Where the factored feature head renders the fine pass (ops.RenderFineFH: frozen width-128 network at test time), the head is not
    # applied per ray at all: render() hands over its input (65 channels) and FusionNet's first convolution runs on weights composed with
    # the head's (FusionNet.forward_prepared_gmap) -- the only consumer of the rendered features in this loop is that linear layer.
    GMAP_CONV0 = os.environ.get("NEFES_GMAP_CONV0", "1") != "0"
    # Mode 2: svd_reg + fix_coord_supp behind the regression network as one launch each way (ops.regressed_pose).  False: ops.svd_reg
    # followed by fix_coord_supp's torch expression (the tests compare the two and tap the pose in between).
    FUSED_REGRESSED_POSE = True
    FUSED_VERIFICATION = True       # PSNR + SSIM of the verification step as ops.psnr_ssim (False: the torch expressions)

    def __init__(self, render_kwargs, args, hwf, near, far, tinyscale=4, lr_r=0.01, lr_t=0.1, lietorch=False,
                 upsample=False, per_pixel=False, world_setup=None, graph=True, device="cuda", adam_capturable=None,
                 fused_glue=True, images=1, pose_model=None, svd_reg=False, learning_rate=1e-5, bn_running_stats=True,
                 intrinsics=None, learn_focal=False, lr_f=1e-3, masked=False, sparse=None, seed=0, redraw=None, depth_weight=None,
                 depth_huber=None):
        self.kw, self.args = dict(render_kwargs), args
        self.depth_weight, self.depth_huber = _depth_term(depth_weight, depth_huber, fused_glue)
        self.sparse = None if sparse is None else int(sparse)
        if self.sparse is not None:
            _refuse_sparse(self.sparse, pose_model, images, upsample, fused_glue, lietorch)
        self.redraw = None if redraw is None else int(redraw)
        if self.redraw is not None:
            if self.sparse is None:
                raise ValueError(f"nefes_amd: PoseRefiner(redraw={redraw}) redraws the pixels of a sparse refiner: it needs sparse=K")
            if self.redraw < 1:
                raise ValueError(f"nefes_amd: PoseRefiner(redraw={redraw}): the number of iterations per draw must be at least 1")
        # False: FusionNet's train-mode BatchNorm leaves its running statistics and batch counter alone in this refiner's iterations
        # (nothing in the loop reads them; the reference never puts the net in eval mode).  REQUIRED for refiners that share a
        # FusionNet and run at the same time (refine_concurrently): the update is a read-modify-write of the shared module's buffers.
        self.bn_running_stats = bool(bn_running_stats)
        self.use_graph, self.fused_glue = bool(graph), bool(fused_glue)        # (read by _apr_adam below)
        H, W, focal = hwf
        self.H, self.W = int(H), int(W)
        self.h, self.w, self.focal = int(H // tinyscale), int(W // tinyscale), float(focal) / tinyscale
        self.near, self.far = float(near), float(far)
        self.upsample, self.per_pixel, self.world_setup = upsample, per_pixel, world_setup
        self.coarse = self.kw["network_fn"]
        self.C = self.coarse.W_features
        self.dev = torch.device(device)
        # images = B > 1: B query images refined side by side in ONE launch sequence per iteration (render_poses, a batched
        # FusionNet with per-image normalisation, per-image losses summed).  Every image's loss depends on its own six numbers
        # only and Adam is element-wise, so each image walks the trajectory it would walk alone; what is shared is the launch
        # overhead and the GPU (an 80x60 frame is 19 sample tiles per CU).  The reference refines one image at a time.
        self.B = int(images)
        if self.B > 1 and (not fused_glue or lietorch):
            raise NotImplementedError("nefes_amd: batched refinement runs on the fused glue kernels (fused_glue=True, "
                                      "lietorch=False)")
        self.apr = None
        if pose_model is not None:
            if self.B > 1:
                raise NotImplementedError("nefes_amd: the regression-network variant refines one image at a time")
            import copy
            self.upsample = upsample = True
            self.apr_base, self.svd_reg = pose_model, bool(svd_reg)
            self.apr = copy.deepcopy(pose_model).to(self.dev).train()           # DFM_post_processing :209 (`pp_model`)
            self.photo = torch.zeros(1, 3, self.H, self.W, device=self.dev)
            self.apr_opt = self._apr_adam(learning_rate)
            self._rgb = self._x_rgb = None
        self.model = LearnPose(self.B, True, True, init_c2w=torch.eye(4)[None].repeat(self.B, 1, 1), lietorch=lietorch).to(self.dev)
        # intrinsics: the camera (fx, fy, cx, cy) of the RENDERED (h, w) image (resized_intrinsics maps a full-resolution K there), one
        # for all images or [B, 4]; None = (focal / ts, centred), on the focal kernels.  It lives in ONE persistent float32 device tensor,
        # self.intrinsics, which the ray kernels read from memory when they run: a captured iteration follows in-place updates of it.
        self.intrinsics, self.log_f = None, None
        if learn_focal:
            if pose_model is not None or self.B > 1:
                raise NotImplementedError("nefes_amd: learn_focal is built for LearnPose mode with one image (no pose_model=, images=1)")
            if not self.fused_glue or lietorch:
                raise NotImplementedError("nefes_amd: learn_focal is optimised by ops.FusedAdam (fused_glue=True, lietorch=False)")
        if (learn_focal or self.sparse is not None) and intrinsics is None:
            # (sparse: the pixel-list ray kernel reads its camera from memory in any case; this is the centred one it would build)
            intrinsics = (self.focal, self.focal, float(self.w * .5), float(self.h * .5))
        if intrinsics is not None:
            if not self.fused_glue:
                raise NotImplementedError("nefes_amd: PoseRefiner(intrinsics=...) runs on the fused glue kernels (fused_glue=True)")
            self.intrinsics = _camera_buffer(intrinsics, self.B, self.dev)
        if learn_focal:
            # NeRF--'s LearnFocal next to LearnPose: one scalar, the rendered camera is (fx e^log_f, fy e^log_f, cx, cy)
            self.log_f = nn.Parameter(torch.zeros(1, device=self.dev))
            self._f_mask = torch.tensor([1., 1., 0., 0.], device=self.dev)
        # fused_glue: the pose chain, the crop and the feature loss as library kernels (ops.pose_compose, the windowed
        # ops.bicubic_upsample, ops.cosine_feature_loss) and one fused Adam launch -- ~80 launches per iteration instead of ~215.
        # False keeps the torch expressions (the tests compare the two).
        # fused glue: Adam over (r, t) with (lr_r, lr_t) as ONE launch (ops.FusedAdam: the two parameters and their gradients are
        # views of flat buffers, the pose kernel's backward writes the gradients there); otherwise torch.optim.Adam, two groups
        if self.fused_glue and not lietorch:
            self.opt = ops.FusedAdam([(self.model.r, lr_r), (self.model.t, lr_t)] + ([(self.log_f, lr_f)] if learn_focal else []))
        else:
            self.opt = torch.optim.Adam([{"params": [self.model.r], "lr": lr_r}, {"params": [self.model.t], "lr": lr_t}],
                                        capturable=bool(graph) if adam_capturable is None else bool(adam_capturable),
                                        fused=True if self.fused_glue else None)
        th, tw = (self.H - 20, self.W - 20) if upsample else (self.h, self.w)
        self.target = torch.zeros(self.C, th, tw, device=self.dev) if self.B == 1 else torch.zeros(self.B, self.C, th, tw, device=self.dev)
        self.hist = torch.zeros(self.B, 10, device=self.dev)
        self.loss = torch.zeros((), device=self.dev) if self.B == 1 else torch.zeros(self.B, device=self.dev)
        # masked (`--semantic`, masked_feature_loss): the feature loss runs over the pixels of self.mask that are != 0 -- ONE persistent
        # uint8 buffer [B, th, tw] (the target's spatial shape, one plane per image shared by its channels) that the masked loss kernels
        # read in place on every iteration: a captured graph follows refine(..., mask=) from image to image.  The routes are the masked
        # ones from construction on (all ones until a mask is given), and there is no prepared-target form of them
        # (_uses_prepared_target), so what is captured does not depend on the images.
        self.masked = bool(masked)
        self.mask = torch.ones(self.B, th, tw, dtype=torch.uint8, device=self.dev) if self.masked else None
        if self.sparse is not None:
            # sparse: ONE persistent pixel list [K, 2] that the ray kernel reads from memory on every iteration, the target's features
            # sampled there [C, K] and -- masked -- the mask sampled there (nearest) [1, K]; set_pixels writes all three in place.  The
            # image's whole feature frame (and mask) is kept for that: self._frame, self._frame_mask.
            K = self.sparse
            self.pixels = torch.zeros(K, 2, device=self.dev)
            self.target = torch.zeros(self.C, K, device=self.dev)
            self.mask = torch.ones(1, K, dtype=torch.uint8, device=self.dev) if self.masked else None
            self._frame, self._frame_mask = None, None
            self._draw = torch.Generator().manual_seed(int(seed))
            if self.redraw is not None:
                # redraw=R: the iteration itself begins with ops.draw_pixels into self.pixels (a new batch every R iterations, from the
                # persistent {seed, tick} words self.draw_state, which _reset rewrites per image) and a re-sample of the target there.
                # The draw reads the image's mask from ONE persistent uint8 frame, all ones until a mask is given; a drawn pixel is
                # valid by construction, so self.mask [1, K] stays all ones.
                self.draw_state = ops.draw_state(int(seed), self.dev)
                self._state0 = self.draw_state.clone()     # (what _reset copies over draw_state: a device-to-device write)
                self._mask_u8 = torch.ones(1, self.h, self.w, dtype=torch.uint8, device=self.dev) if self.masked else None
        # depth_weight=lambda: the image's measured depth at the rendered frame's pixels in ONE persistent float32 buffer [B, h*w] (sparse:
        # [1, K], sampled -- nearest -- from the frame kept in self._depth_frame) that the depth-loss kernels read in place, and the disp_map
        # of the iteration's own render (self._disp, kept by _fused / _sparse_features).  self.depth_loss: the term's last value (float64,
        # lambda not applied; [B] with images=B) -- the head of the kernel's scratch, which a captured iteration keeps at one address.
        self.depth_loss, self._disp = None, None
        if self.depth_weight is not None:
            self.depth_target = torch.zeros(self.B, self.h * self.w if self.sparse is None else self.sparse, device=self.dev)
            self._depth_frame = torch.zeros(1, self.h, self.w, device=self.dev) if self.sparse is not None else None
            self.depth_loss = torch.zeros((), dtype=torch.float64, device=self.dev) if self.B == 1 else \
                torch.zeros(self.B, dtype=torch.float64, device=self.dev)
        self._affine = None            # static [1,12] buffer with the image's colour transform when the exposure network is frozen
        self.graph, self.apr_graph = None, None

    # one iteration on the static buffers -------------------------------------------------------------------------
    def _camera(self):
        """{} (the focal kernels), or render()'s `intrinsics=` keyword: self.intrinsics itself, or with learn_focal its first two
        entries times e^log_f (three element-wise torch launches; exp(0) = 1 and x * 1 = x, so the principal point passes exactly)."""
        if self.intrinsics is None:
            return {}
        if self.log_f is None:
            return {"intrinsics": self.intrinsics}
        return {"intrinsics": self.intrinsics * torch.exp(self.log_f * self._f_mask)}

    def features(self):
        """The fused features [B, C, h, w] the loss compares with the target, at the refiner's current state (pose, camera, log_f):
        what a caller renders a synthetic target with."""
        with torch.no_grad():
            return (self._sparse_features() if self.sparse is not None else self._fused()).detach().clone()

    def _composed_pose(self):
        """LearnPose + fix_coord_supp as one launch each way (ops.pose_compose): [B, 3, 4]; with the fused Adam its backward writes the
        parameters' .grad itself."""
        ws = self.world_setup or {"pose_scale": 1.0, "pose_scale2": 1.0, "move_all_cam_vec": (0., 0., 0.)}
        into = (self.model.r.grad, self.model.t.grad) if isinstance(self.opt, ops.FusedAdam) else None
        return ops.pose_compose(self.model.r, self.model.t, self.model.init_c2w, ws["pose_scale"], ws["move_all_cam_vec"],
                                ws["pose_scale2"], grad_into=into)

    def _sparse_features(self):
        """sparse: pose -> render(pixels=self.pixels) -> feat_map [K, C] -> [C, K], the layout the loss kernels read (a torch
        transposition: plumbing).  With sparse= in place of the frame, what features() returns."""
        c2w = self._composed_pose()
        _, disp, _, ex = render(self.h, self.w, self.focal, c2w=c2w.reshape(3, 4), near=self.near, far=self.far, img_idx=self.hist,
                                pixels=self.pixels, **self.kw, **self._camera())
        self._disp = disp if self.depth_weight is not None else None       # (the depth term's input: _with_depth_term)
        return ex["feat_map"].t()

    def _fused(self):
        """pose -> render -> affine colour transform -> fusion CNN: the fused features [B, C, h, w] of the current state."""
        B = self.B
        track = self.bn_running_stats                      # this refiner's calls only: the shared FusionNet's own setting is not touched
        if self.apr is not None:                           # train_on_batch :91-97
            c2w = self.apr(self.photo).reshape(1, 3, 4)
            if self.fused_glue and self.FUSED_REGRESSED_POSE and HIP_SVD_REG and c2w.is_cuda and c2w.dtype == torch.float32:
                c2w = ops.regressed_pose(c2w, self.svd_reg, self.world_setup)          # svd_reg + fix_coord_supp: one launch each way
            else:
                if self.svd_reg:
                    c2w = svd_reg(c2w)
                if self.world_setup is not None:
                    c2w = fix_coord_supp(c2w, self.world_setup)
        elif self.fused_glue and not self.model.lietorch:
            c2w = self._composed_pose()                    # [B,3,4]
        else:
            c2w = self.model(0)[None, :3, :4]
            if self.world_setup is not None:
                c2w = fix_coord_supp(c2w, self.world_setup)
        enc = bool(getattr(self.args, "encode_hist", False))
        fnet = self.coarse.fusion_net
        fused_input = self.fused_glue and (not enc or self._affine is not None) and fnet._use_hip(self.hist)
        kw = self.kw
        if fused_input and self.GMAP_CONV0 and not fnet.fusion_residule and kw.get("network_fine", None) is not None:
            kw = dict(kw, feat_as_gmap=True)               # honoured only where render() takes the factored head (extras["feat_is_gmap"])
        if B == 1:
            # (a view, not c2w[0]: indexing costs a zero fill and a copy in the backward)
            rgb, disp, _, ex = render(self.h, self.w, self.focal, c2w=c2w.reshape(3, 4), near=self.near, far=self.far, img_idx=self.hist, **kw,
                                      **self._camera())
            feat = ex["feat_map"]
        else:
            rgb, disp, _, ex = render_poses(self.h, self.w, self.focal, c2w, near=self.near, far=self.far, **kw, **self._camera())
            rgb, feat = rgb.reshape(-1, 3), ex["feat_map"].reshape(-1, ex["feat_map"].shape[-1])
        self._disp = disp if self.depth_weight is not None else None       # (the depth term's input: _with_depth_term)
        gmap = bool(ex.get("feat_is_gmap", False))
        if fused_input:
            # colour transform + normalisation + the NCHW concatenation as one launch each way (ops.fusion_input)
            x = ops.fusion_input(rgb, feat, self._affine if enc else None, B, self.h, self.w, fnet.mean, fnet.std)
            if self.apr is not None:
                self._x_rgb = x.detach()[:, :3]            # the verification step's image, still normalised (:117-118)
            if gmap:
                _, w_f, _, b_f = kw["network_fine"].packed_fh()
                fused = fnet.forward_prepared_gmap(x, w_f, b_f, per_image_norm=B > 1, track_stats=track)
            else:
                fused = fnet.forward_prepared(x, per_image_norm=B > 1, track_stats=track)
        else:
            if enc:
                if self._affine is not None:               # frozen exposure network: its 12 numbers were computed once per image
                    rgb = self.coarse.apply_affine(self._affine, rgb, B)
                else:
                    rgb = self.coarse.affine_color_transform(self.args, rgb, self.hist, B)
            if self.apr is not None:
                self._rgb, self._x_rgb = rgb.detach(), None
            _, _, fused = self.coarse.run_fusion_net(rgb, feat, self.h, self.w, B, per_image_norm=B > 1, track_stats=track)
        return fused

    def _loss(self):
        """The iteration's loss: the feature term (_feature_term) and, on a PoseRefiner(depth_weight=), the depth term on the disp_map
        the same render returned.  Returns (what to differentiate -- a scalar, or the tuple of scalars whose sum is the loss --, per-image
        totals [B] or the total itself)."""
        loss, per_image = self._feature_term()
        if self.depth_weight is None:
            return loss, per_image
        return self._with_depth_term(loss, per_image)

    def _with_depth_term(self, loss, per_image):
        """lambda * ops.depth_loss(disp_map, the image's depth; one group per image) next to the feature term: the two scalars are
        differentiated together -- they meet in the render's own node, as g_feat and g_disp -- and never added by torch.  One image: the
        feature kernel left its value in self.loss and the depth kernel adds its term there (`accumulate`): one launch forward, one
        backward, no arithmetic launch.  images=B: the per-image totals are formed from the kernel's per-group values (torch glue).
        Only depth validity counts (target and disp): the feature term's mask is not the depth term's."""
        disp, self._disp = self._disp.reshape(self.B, -1), None            # (not kept: it would hold the iteration's autograd graph)
        if self.B == 1:
            total, groups = ops.depth_loss(disp, self.depth_target, delta=self.depth_huber, weight=self.depth_weight, out=self.loss,
                                           accumulate=True, return_groups=True)
            self.depth_loss = groups.reshape(())
            return (loss, total), total.detach()
        term, groups = ops.depth_loss(disp, self.depth_target, delta=self.depth_huber, weight=self.depth_weight, return_groups=True)
        self.depth_loss = groups
        return (loss, term), per_image + (groups * self.depth_weight).float()

    def _feature_term(self):
        """DFM_optimization_NFF (:310-337): pose -> render -> affine colour transform -> fusion CNN -> feature loss.
        Returns (scalar to differentiate, per-image losses [B] or the same scalar).  One image on the fused glue: the library's loss
        kernel writes its value straight into the static buffer self.loss (`out=`: no 4-byte copy launch per iteration); everything
        else (images=B, the torch expressions) returns its own tensor and the callers copy it."""
        if self.sparse is not None:
            # the K rendered features [C, K] against self.target [C, K]; masked: over the pixels with self.mask != 0
            return self._library_loss(self._sparse_features(), self.target, self.mask, self.loss)
        B, C = self.B, self.C
        fused = self._fused()
        if not self.fused_glue:                            # one image, the torch expressions
            if self.upsample:
                fused = ops.bicubic_upsample(fused, (self.H, self.W))[:, :, 10:-10, 10:-10]
            if self.masked:
                loss = masked_feature_loss(fused[0], self.target, self.mask, per_pixel=self.per_pixel)
            else:
                # (a view where possible: fused[0] costs a 34 MB zero fill and a copy in the backward)
                fused = fused.view(fused.shape[1:]) if fused.is_contiguous() else fused[0]
                loss = feature_loss(fused, self.target, per_pixel=self.per_pixel)
            return loss, loss.detach()
        out = self.loss if B == 1 else None
        if self._uses_prepared_target():
            mean_loss, cos = ops.upsampled_cosine_loss_prepared(fused.reshape(B * C, self.h, self.w), self._sync_upcos(), return_cos=True, out=out)
            if B > 1:
                return mean_loss * float(B), (1.0 - cos.view(B, C).mean(1)).float()
            return mean_loss, mean_loss.detach()
        if self.upsample and self.FUSED_UPSAMPLED_LOSS:
            # up-sampling, crop and feature loss in one pass each way: the 34 MB up-sampled image is never written
            return self._library_loss(fused.reshape(B * C, self.h, self.w), self.target.reshape(B * C, self.H - 20, self.W - 20), self.mask, out,
                                      upsampled=True)
        if self.upsample:
            fused = ops.bicubic_upsample(fused, (self.H, self.W), crop=10)
        return self._library_loss(fused.reshape(B * C, -1), self.target.reshape(B * C, -1), None if self.mask is None else self.mask.view(B, -1), out)

    def _library_loss(self, feats, target, mask, out, upsampled=False):
        """_loss's last step on the library's one-pass loss kernels, in the form the loop runs: per channel or per pixel
        (self.per_pixel), of feats [B*C, pixels] or -- `upsampled` -- of feats [B*C, h, w] up-sampled and cropped inside the kernels,
        over all pixels or those with mask != 0.  `groups=B`: the value is already the sum over the images.  self.target (and the
        mask) are read on every iteration: no form here has a prepared target (csrc/feature_loss.hip says why)."""
        B = self.B
        if upsampled:
            op = ops.upsampled_pixel_cosine_loss if self.per_pixel else ops.upsampled_cosine_loss
            loss, cos = op(feats, target, (self.H, self.W), crop=10, groups=B, return_cos=True, out=out, mask=mask)
        else:
            op = ops.pixel_cosine_loss if self.per_pixel else ops.cosine_feature_loss
            loss, cos = op(feats, target, groups=B, return_cos=True, out=out, mask=mask)
        if B == 1:
            return loss, loss.detach()
        return loss, (1.0 - (cos if self.per_pixel else cos.view(B, self.C).mean(1))).float()

    def _set_mask(self, mask):
        """The image's validity mask into self.mask, IN PLACE (a captured iteration keeps reading the same buffer): thresholded `> 0`
        once, from bool / uint8 / float, [th,tw] or [1,th,tw] (images=B: [B,th,tw] or [B,1,th,tw]); None: all valid.  An image without
        a valid pixel is refused here -- one host read per call, outside the loop."""
        if not self.masked:
            if mask is not None:
                raise ValueError("nefes_amd: this PoseRefiner was built without a mask buffer; construct it with PoseRefiner(..., masked=True) "
                                 "to pass mask=")
            return
        with torch.no_grad():
            if mask is None:
                self.mask.fill_(1)
                return
            m = torch.as_tensor(mask)
            th, tw = self.mask.shape[1:]
            if tuple(m.shape) not in ({(th, tw), (1, th, tw), (1, 1, th, tw)} if self.B == 1 else {(self.B, th, tw), (self.B, 1, th, tw)}):
                raise ValueError(f"nefes_amd: the mask has shape {tuple(m.shape)}; this refiner compares at {(th, tw)} "
                                 f"({self.B} image(s): one plane each; refine.full_resolution_mask makes the up-sampled, cropped form)")
            m = (m.to(self.dev) > 0).reshape(self.mask.shape)
            empty = (~m.reshape(self.B, -1).any(1)).nonzero().flatten().tolist()
            if empty:
                raise ValueError(f"nefes_amd: the mask of image(s) {empty} has no valid pixel (mask > 0): nothing to refine against")
            self.mask.copy_(m)

    def _ensure_upcos(self):
        """self._upcos (ops.UpcosTarget) with the target buffer's shape, built when there is none or the shape moved -- never under
        capture: its set-up launches would be replayed with every iteration."""
        if getattr(self, "_upcos", None) is None or self._upcos_shape != tuple(self.target.shape):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("nefes_amd: the refinement target changed without PoseRefiner._sync_upcos() before graph capture")
            self._upcos = ops.UpcosTarget(self.B * self.C, self.h, self.w, self.H, self.W, 10, self.dev)
            self._upcos_shape, self._upcos_key = tuple(self.target.shape), None
        return self._upcos

    def _sync_upcos(self):
        """The prepared form of self.target (ops.UpcosTarget), recomputed whenever the target buffer was written since (tensor version
        counter).  _reset / _apr_image_state call this after copying an image's target in, i.e. before a captured graph is replayed; under
        capture the buffers must already be current (a re-computation would be replayed with every iteration)."""
        key = (self.target.data_ptr(), self.target._version)
        upcos = self._ensure_upcos()
        if self._upcos_key != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("nefes_amd: the refinement target changed without PoseRefiner._sync_upcos() before graph capture")
            with torch.no_grad():
                upcos.update(self.target.reshape(self.B * self.C, self.H - 20, self.W - 20))
            self._upcos_key = key
        return upcos

    def _uses_prepared_target(self):
        """The Gram-form loss against the prepared target -- where the loop takes the fused up-sampled loss at all AND the geometry fits
        the Gram kernel's LDS (ops.UpcosTarget.fits, known once the buffers exist); otherwise the one-pass kernels, which read
        self.target itself on every iteration."""
        if not (self.upsample and self.fused_glue and not self.per_pixel and self.FUSED_UPSAMPLED_LOSS and self.PREPARED_TARGET):
            return False
        if self.masked:                                    # sum_p m_p up_p^2 does not separate into the two axes: no Gram form
            return False
        return bool(self._ensure_upcos().fits)

    def _one_like(self, loss):
        """The root gradient, once: autograd otherwise fills a new one per iteration."""
        if getattr(self, "_one", None) is None or self._one.shape != loss.shape:
            self._one = torch.ones_like(loss)
        return self._one

    def _ones_for(self, loss):
        """_one_like for what _loss returns to differentiate: a scalar, or a tuple of scalars (one root gradient each, the same tensor)."""
        return tuple(self._one_like(l) for l in loss) if isinstance(loss, tuple) else self._one_like(loss)

    def loss_and_grad(self):
        """Loss at the current (r, t) and its gradient, written into the parameters' static .grad buffers (no optimizer step).
        The gradients are copied over the previous ones: nothing has to be zeroed between iterations."""
        loss, per_image = self._loss()
        params = [self.model.r, self.model.t] + ([] if self.log_f is None else [self.log_f])
        for p, g in zip(params, torch.autograd.grad(loss, params, grad_outputs=self._ones_for(loss))):
            if p.grad is None:
                p.grad = torch.empty_like(p)
            if g.data_ptr() != p.grad.data_ptr():          # (the fused pose kernel writes the parameters' .grad itself)
                p.grad.copy_(g)
        if per_image.data_ptr() != self.loss.data_ptr():   # (the fused loss kernels wrote it there themselves: `out=` in _loss)
            self.loss.copy_(per_image)
        return self.loss

    def _redraw(self):
        """redraw=R: a new batch of pixels into self.pixels -- every R calls, the tick in self.draw_state is advanced by the draw itself
        -- and the image's target sampled there: two launch sequences with no host read, captured with the iteration behind them."""
        with torch.no_grad():
            ops.draw_pixels(self.h, self.w, self.sparse, self.draw_state, mask=self._mask_u8, period=self.redraw, advance=True,
                            out=self.pixels)
            ops.sample_pixels(self._frame, self.pixels, out=self.target)
            if self.depth_weight is not None:              # (a drawn pixel without a valid depth just does not count: no host read)
                ops.sample_pixels(self._depth_frame, self.pixels, out=self.depth_target, nearest=True)

    def _iteration(self):
        if self.redraw is not None:
            self._redraw()
        self.loss_and_grad()
        self.opt.step()

    def _exposure_into_affine(self):
        """Frozen exposure network: the image's twelve colour-transform numbers, computed once per image from self.hist and written IN
        PLACE into the static buffer self._affine (a captured graph keeps reading the same buffer)."""
        expo = getattr(self.coarse, "exposure_embedding", None)
        if (self.fused_glue and getattr(self.args, "encode_hist", False) and expo is not None
                and not any(p.requires_grad for p in expo.parameters())):
            a = self.coarse.exposure_coefficients(self.hist)
            if self._affine is None:
                self._affine = a.clone()
            else:
                self._affine.copy_(a)

    def _frame_mask_of(self, mask):
        """sparse: the image's mask as bool [h, w] on the device (None: no mask)."""
        h, w = self.h, self.w
        if mask is None:
            return None
        if not self.masked:
            raise ValueError("nefes_amd: this PoseRefiner was built without a mask buffer; construct it with PoseRefiner(..., masked=True) "
                             "to pass mask=")
        m = torch.as_tensor(mask)
        if m.numel() != h * w or tuple(m.shape[-2:]) != (h, w):
            raise ValueError(f"nefes_amd: the mask has shape {tuple(m.shape)}; a sparse refiner samples it from the rendered frame {(h, w)}")
        return (m.to(self.dev) > 0).reshape(h, w)

    def _draw_pixels(self, frame_mask):
        """sparse: K distinct integer pixels (x, y) of the rendered frame, uniform among the mask's valid ones, from the generator of the
        constructor's seed: int64 [K, 2] on the host.  One host read of the mask, outside the loop."""
        h, w = self.h, self.w
        valid = torch.arange(h * w) if frame_mask is None else frame_mask.reshape(-1).nonzero().flatten().cpu()
        if valid.numel() < self.sparse:
            raise ValueError(f"nefes_amd: {self.sparse} distinct pixels asked for, the frame {(h, w)} has {valid.numel()} valid ones")
        idx = valid[torch.randperm(valid.numel(), generator=self._draw)[:self.sparse]]
        return torch.stack([idx % w, idx // w], -1)

    def _set_frame(self, feature_target, mask, pixels):
        """sparse: the image's feature frame [C, h, w] and mask (kept for set_pixels), then its pixels -- the given [K, 2] list, or drawn
        (_draw_pixels)."""
        h, w = self.h, self.w
        frame = feature_target.to(self.dev, torch.float32)
        if frame.numel() != self.C * h * w:
            raise ValueError(f"nefes_amd: a sparse refiner samples its target from the rendered frame's features [{self.C}, {h}, {w}]; got "
                             f"{tuple(feature_target.shape)}")
        if self.redraw is not None:
            return self._set_redrawn_frame(frame.reshape(self.C, h, w), self._frame_mask_of(mask), pixels)
        self._frame, self._frame_mask = frame.reshape(self.C, h, w).contiguous(), self._frame_mask_of(mask)
        self.set_pixels(self._draw_pixels(self._frame_mask) if pixels is None else pixels)

    def _set_redrawn_frame(self, frame, frame_mask, pixels):
        """redraw=R: the image's state IN PLACE, where the captured draw and re-sample read it: the feature frame, the mask as the uint8
        frame the draw selects from (all ones without one), and {seed, 0} in self.draw_state -- which also undoes the ticks that the
        warm-up iterations of a first capture consumed: an image's batches depend on (seed, mask) and not on what the refiner did
        before.  With a mask, one host read per image, outside the loop: fewer than K valid pixels are refused as _draw_pixels does."""
        if pixels is not None:
            raise ValueError("nefes_amd: pixels= on a PoseRefiner(redraw=R): it draws its pixels itself, every R iterations; build it "
                             "without redraw= to refine at a given list")
        if frame_mask is not None:
            valid = int(frame_mask.sum())
            if valid < self.sparse:
                raise ValueError(f"nefes_amd: {self.sparse} distinct pixels asked for, the frame {(self.h, self.w)} has {valid} valid ones")
        with torch.no_grad():
            if self._frame is None:
                self._frame = torch.empty(self.C, self.h, self.w, device=self.dev)
            self._frame.copy_(frame)
            self._frame_mask = frame_mask
            if self.masked:
                if frame_mask is None:
                    self._mask_u8.fill_(1)
                else:
                    self._mask_u8.copy_(frame_mask.reshape(self._mask_u8.shape))
            self.draw_state.copy_(self._state0)

    def set_pixels(self, px):
        """sparse: new pixels [K, 2] (ops.as_pixels) into self.pixels IN PLACE, and the image's target -- and mask, nearest -- re-sampled
        there in place: a captured iteration reads all three from memory and follows without a re-capture."""
        if self.sparse is None:
            raise RuntimeError("nefes_amd: set_pixels needs a PoseRefiner(sparse=K)")
        if self.redraw is not None:
            raise ValueError("nefes_amd: set_pixels on a PoseRefiner(redraw=R): it draws its pixels itself, every R iterations")
        if self._frame is None:
            raise RuntimeError("nefes_amd: set_pixels re-samples the image's target: give the refiner an image first (refine)")
        px = ops.as_pixels(px, self.dev)
        if tuple(px.shape) != (self.sparse, 2):
            raise ValueError(f"nefes_amd: this refiner was built for {self.sparse} pixels [{self.sparse}, 2]; got {tuple(px.shape)}")
        with torch.no_grad():
            self.pixels.copy_(px)
            ops.sample_pixels(self._frame, self.pixels, out=self.target)
            if self.depth_weight is not None:              # (nearest: a depth must not be blended across a hole or an edge)
                ops.sample_pixels(self._depth_frame, self.pixels, out=self.depth_target, nearest=True)
            if self.masked:
                if self._frame_mask is None:
                    self.mask.fill_(1)
                else:
                    xi = self.pixels[:, 0].round().clamp_(0, self.w - 1).long()
                    yi = self.pixels[:, 1].round().clamp_(0, self.h - 1).long()
                    self.mask.copy_(self._frame_mask[yi, xi].reshape(1, -1))
                    if not bool(self.mask.any()):
                        raise ValueError("nefes_amd: none of the pixels is valid in the image's mask (mask > 0): nothing to refine against")

    def _reset(self, init_c2w, feature_target, hist, mask=None, pixels=None, depth=None):
        if self.sparse is None:
            self._set_mask(mask)
        self._set_depth(depth)                             # (before the pixels: set_pixels samples the depth frame at them)
        with torch.no_grad():
            self.model.r.zero_()
            self.model.t.zero_()
            if self.log_f is not None:
                self.log_f.zero_()
            self.model.init_c2w.copy_(init_c2w.reshape(self.B, 4, 4))
            if self.sparse is not None:
                self._set_frame(feature_target, mask, pixels)
            else:
                self.target.copy_(feature_target.reshape(self.target.shape))
            if self._uses_prepared_target():
                self._sync_upcos()
            self.hist.copy_(hist.reshape(self.B, 10))
            self._exposure_into_affine()
            if isinstance(self.opt, ops.FusedAdam):
                self.opt.zero_state()
            else:
                _zero_optimizer_state(self.opt)
                for p in (self.model.r, self.model.t):
                    if p.grad is not None:
                        p.grad.zero_()

    def _refined_pose(self):
        with torch.no_grad():
            idx = 0 if self.B == 1 else torch.arange(self.B, device=self.dev)
            return self.model(idx).detach().clone()

    # ---- the loop, written once for both modes ---------------------------------------------------------------------------
    def _mode(self, apr=False, verification=True):
        """The _Mode record of `refine` (mode 3) or, apr=True, of `refine_apr` (mode 2) on this refiner."""
        first_use = lambda m: self.use_graph and getattr(self, m.slot) is None
        if not apr:
            return _Mode(False, on_device=lambda job: tuple(t if t is None else t.to(self.dev) for t in job), set_state=self._reset,
                         iteration=self._iteration,
                         prepare=lambda m, job: first_use(m) and self._run(m, job, iters=0), read=self._refined_pose,
                         read_own=self._refined_pose,
                         finish=lambda pose, _, __, losses: ((pose, losses) if self.log_f is None
                                                             else (pose, losses, self.log_f.detach().clone())))
        if self.apr is None:
            raise RuntimeError("nefes_amd: PoseRefiner was built without pose_model=")

        def before_capture():
            for p in self.apr.parameters():
                p.grad = None                              # the captured backward allocates them in the graph's pool and keeps them there
            self._captured_apr_opt = self.apr_opt          # (the graph updates THIS optimizer's state tensors)

        def check(i, iters):                               # (tensors, read after the loop: no host sync behind iteration 0)
            return self._verification(as_tensors=True) if verification and i in (0, iters - 1) else None
        return _Mode(True, on_device=tuple, set_state=self._apr_set_state, iteration=self._apr_iteration,
                     prepare=lambda m, job: (m.set_state(*job), first_use(m) and self._capture(m)), read=self.predicted_pose,
                     read_own=lambda: self.predicted_pose().detach().clone(), finish=self._apr_result, before_capture=before_capture,
                     before=self.predicted_pose, check=check)

    def _capture(self, m):
        """One iteration of mode `m` (forward, backward, optimizer step; mode 2: regression network, svd_reg, ..., torch's Adam over its
        weights) as ONE HIP graph in the mode's slot, after a warm-up on a side stream (allocator, MIOpen plans, Adam state).  The caller
        re-writes the image's state afterwards: the warm-up steps moved it."""
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                m.iteration()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        m.before_capture()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.iteration()
        setattr(self, m.slot, g)

    def replay(self, apr=False):
        """One iteration as the captured graph -- after a HOST check that what the graph reads in place is current: the prepared form of
        self.target (ops.UpcosTarget) is refreshed when the target buffer was written since (its tensor version moved).  Code that
        writes refiner.target itself and replays refiner.graph directly optimises against the OLD target without any error (the
        one-pass kernels read self.target on every iteration; the prepared form cannot); this is the call to use instead."""
        if self._uses_prepared_target():
            self._sync_upcos()
        (self.apr_graph if apr else self.graph).replay()

    def _step(self, m, i, iters, losses, checks):
        """Iteration i of `iters` on the current stream: replayed or eager, its loss into losses[i], what the mode records behind it."""
        if self.use_graph and getattr(self, m.slot) is not None:
            self.replay(apr=m.apr)
        else:
            m.iteration()
        losses[i] = self.loss
        seen = m.check(i, iters)
        if seen is not None:
            checks.append(seen)

    def _run(self, m, job, iters):
        """One image (or one batch) through mode `m` on the current stream: state, capture on first use and the state again, `iters`
        iterations, the mode's result."""
        job = m.on_device(job)
        m.set_state(*job)
        if self.use_graph and getattr(self, m.slot) is None:
            self._capture(m)
            m.set_state(*job)
        before = m.before()
        losses, checks = torch.empty((iters,) + tuple(self.loss.shape), device=self.dev), []
        for i in range(iters):
            self._step(m, i, iters, losses, checks)
        return m.finish(m.read(), before, checks, losses)

    def _job(self, *job, mask=None, pixels=None, depth=None, apr=False):
        """The job tuple of an image (_job_without_depth) and, on a PoseRefiner(depth_weight=), the image's measured depth behind it: the
        sixth element (mode 2, `apr`: the fifth), the ones before it filled with None."""
        job = self._job_without_depth(*job, mask=mask, pixels=pixels)
        if self.depth_weight is None:
            if depth is not None:
                raise ValueError("nefes_amd: depth= needs a PoseRefiner(depth_weight=...): this one was built without the depth term")
            return job
        if depth is None:
            raise ValueError("nefes_amd: this PoseRefiner was built with depth_weight=: pass the image's measured depth, depth=[h, w] "
                             f"= {(self.h, self.w)}, the rendered frame's resolution")
        n = 4 if apr else 5
        return job + (None,) * (n - len(job)) + (self._checked_depth(depth),)

    def _checked_depth(self, depth):
        """The image's measured depth as float32 [B, h, w]; a shape other than the rendered frame's is refused, naming both."""
        if depth is None:
            raise ValueError("nefes_amd: this PoseRefiner was built with depth_weight=: pass the image's measured depth (depth=)")
        d = torch.as_tensor(depth)
        h, w = self.h, self.w
        ok = {(h, w), (1, h, w)} if self.B == 1 else {(self.B, h, w)}
        if tuple(d.shape) not in ok:
            raise ValueError(f"nefes_amd: the depth frame has shape {tuple(d.shape)}; this refiner renders {(h, w)}"
                             + (f" for each of {self.B} images: [{self.B}, {h}, {w}]" if self.B > 1 else "")
                             + " (refine.resized_depth brings a full-resolution sensor frame there)")
        return d.to(torch.float32).reshape(self.B, h, w)

    def _set_depth(self, depth):
        """The image's measured depth into the static buffers, IN PLACE (a captured iteration keeps reading them).  A frame without a
        valid pixel (finite and > 0) is refused -- one host read per image, outside the loop.  sparse: the frame is kept and sampled,
        nearest, at the refiner's pixels (set_pixels; with redraw=R by the captured iteration itself)."""
        if self.depth_weight is None:
            if depth is not None:
                raise ValueError("nefes_amd: depth= needs a PoseRefiner(depth_weight=...): this one was built without the depth term")
            return
        d = self._checked_depth(depth).to(self.dev)
        empty = (~(torch.isfinite(d) & (d > 0)).reshape(self.B, -1).any(1)).nonzero().flatten().tolist()
        if empty:
            raise ValueError(f"nefes_amd: the depth frame of image(s) {empty} has no valid pixel (finite and > 0): nothing to compare with")
        with torch.no_grad():
            if self.sparse is None:
                self.depth_target.copy_(d.reshape(self.depth_target.shape))
            else:
                self._depth_frame.copy_(d)

    def _job_without_depth(self, *job, mask=None, pixels=None):
        """The job tuple of an image: with a fourth element, its mask, on a masked refiner (None: all valid); on a sparse refiner a
        fourth and a fifth, mask and pixels (None: drawn)."""
        if self.sparse is not None:
            if self.redraw is not None:                    # (nothing is drawn here: the iteration draws)
                if pixels is not None:
                    raise ValueError("nefes_amd: pixels= on a PoseRefiner(redraw=R): it draws its pixels itself, every R iterations; "
                                     "build it without redraw= to refine at a given list")
                return job + (None if mask is None else torch.as_tensor(mask), None)
            # (drawn HERE, once per image: _run writes the image's state twice around a first capture)
            px = self._draw_pixels(self._frame_mask_of(mask)) if pixels is None else pixels
            return job + (None if mask is None else torch.as_tensor(mask), ops.as_pixels(px, self.dev))
        if pixels is not None:
            raise ValueError("nefes_amd: pixels= needs a PoseRefiner(sparse=K)")
        if not self.masked:
            self._set_mask(mask)                           # (raises for mask= on an unmasked refiner)
            return job
        return job + (None if mask is None else torch.as_tensor(mask),)

    def refine(self, init_c2w, feature_target, hist, iters=50, mask=None, pixels=None, depth=None):
        """One image (images=1): (refined 4x4 c2w, losses [iters]) -- with learn_focal (refined c2w, losses, log_f [1]).
        A batch (images=B): init_c2w [B,4,4], feature_target [B,C,h,w], hist [B,10] -> (refined poses [B,4,4], losses [iters,B]), each image as if refined alone.
        mask (PoseRefiner(masked=True)): the image's valid pixels, > 0, in the target's spatial shape [th,tw] or [1,th,tw] (a batch:
        [B,th,tw]); None: all valid.
        pixels (PoseRefiner(sparse=K)): the [K, 2] points (x, y) of the rendered (h, w) frame to match at; feature_target is that frame's
        features [C, h, w], sampled there once.  None: K distinct integer pixels are drawn.
        depth (PoseRefiner(depth_weight=)): the image's measured z-depth in the scene's units at the RENDERED frame's resolution, [h,w]
        (a batch: [B,h,w]; a sparse refiner takes the frame too and samples it, nearest, at its pixels); holes are 0, Inf or NaN
        (resized_depth brings a full-resolution sensor frame here).  The losses returned are the totals, feature + lambda * depth."""
        return self._run(self._mode(), self._job(init_c2w, feature_target, hist, mask=mask, pixels=pixels, depth=depth), iters)

    refine_batch = refine

    # ---- train_on_batch / DFM_post_processing (pose_only=2) ------------------------------------------------------------
    def apr_loss_and_grad(self):
        """Loss at the working network's current parameters; gradients into their .grad (no optimizer step)."""
        loss, _ = self._loss()
        params = [p for p in self.apr.parameters() if p.requires_grad]
        # loss.backward() in the reference (train_on_batch, DFM_pose_refine.py:318) tolerates parameters the loss never touches --
        # DFNet's adaptation_layers with return_feature=False (feature/dfnet.py:142): their .grad stays None and Adam skips them
        for p, g in zip(params, torch.autograd.grad(loss, params, grad_outputs=self._ones_for(loss), allow_unused=True)):
            p.grad = g
        if isinstance(loss, tuple):                        # (feature term, total: the depth kernel added its term in self.loss)
            loss = loss[-1]
        if loss.data_ptr() != self.loss.data_ptr():
            self.loss.copy_(loss.detach())
        return self.loss

    def _verification(self, as_tensors=False):
        """PSNR and mean SSIM of the up-sampled, cropped render against the cropped query image (:117-128, :146-150)."""
        if self._x_rgb is not None:                        # de-normalise FusionNet's colour channels
            fnet = self.coarse.fusion_net
            mean, std = fnet._mean_std(self._x_rgb)
            img = self._x_rgb * std[:, None, None] + mean[:, None, None]
        else:
            img = self._rgb.reshape(1, self.h, self.w, 3).permute(0, 3, 1, 2)
        img = nn.functional.interpolate(img, size=(self.H, self.W), mode="bicubic")[:, :, 10:-10, 10:-10]
        gt = self.photo[:, :, 10:-10, 10:-10]
        if self.fused_glue and self.FUSED_VERIFICATION and img.is_cuda and img.dtype == torch.float32 and img.shape[0] == 1:
            ps, ss = ops.psnr_ssim(img[0], gt[0])          # two launches for PSNR + SSIM (torch: ~25); the crops stay views
        else:
            ps, ss = mse2psnr(img2mse(img, gt)).reshape(()), ssim_map(img, gt).mean().reshape(())
        if as_tensors:                                     # (no host read: the callers convert after their last replay)
            return ps, ss
        return float(ps), float(ss)

    def predicted_pose(self, net=None):
        """inference_pose_regression (DFM_pose_refine.py:131-160) of the working (or given) network on the query image: [3,4]."""
        with torch.no_grad():
            pose = (self.apr if net is None else net)(self.photo).reshape(1, 3, 4)
            return (svd_reg(pose) if self.svd_reg else pose)[0]

    def _apr_image_state(self, photo, feature_target, hist, mask=None, depth=None):
        """Per-image state of train_on_batch, written IN PLACE (a captured iteration keeps reading the same buffers): the query image, its
        cropped features (:125), a fresh copy of the regression network (:209), the histogram and the colour transform's twelve numbers;
        on a masked refiner the image's mask of the cropped pixels."""
        dev = self.dev
        self._set_mask(mask)
        self._set_depth(depth)
        with torch.no_grad():
            self.photo.copy_(photo.to(dev).reshape(self.photo.shape))
            self.target.copy_(feature_target.to(dev).reshape(self.C, self.H, self.W)[:, 10:-10, 10:-10])
            if self._uses_prepared_target():
                self._sync_upcos()
            for pw, pb in zip(self.apr.parameters(), self.apr_base.parameters()):
                pw.copy_(pb.to(dev))                                       # a fresh copy of the network per image (:209)
            for bw, bb in zip(self.apr.buffers(), self.apr_base.buffers()):
                bw.copy_(bb.to(dev))                                       # deepcopy resets BatchNorm statistics too
            self.hist.copy_(hist.to(dev).reshape(1, 10))
            self._exposure_into_affine()

    def _apr_set_state(self, photo, feature_target, hist, mask=None, depth=None):
        self._apr_image_state(photo, feature_target, hist, mask, depth)
        self._apr_fresh_adam()

    def _apr_iteration(self):
        self.apr_loss_and_grad()
        self.apr_opt.step()

    def _apr_adam(self, lr):
        """torch.optim.Adam over the regression network's parameters (DFM_APR_refine.py:212).  On the GPU its multi-tensor form
        (`fused=True`: ONE launch for all parameters + one for the step counters; same update, same rounding order per element) instead
        of the default for-each form's ten element-wise launches per step -- the network is the caller's, so is the number of its
        parameter tensors (DFNet: ~100)."""
        params = list(self.apr.parameters())
        on_gpu = all(p.is_cuda for p in params)
        return torch.optim.Adam(params, lr=lr, capturable=bool(self.use_graph) and on_gpu, fused=True if (on_gpu and self.fused_glue) else None)

    def _apr_fresh_adam(self):
        """torch.optim.Adam(pp_model.parameters(), lr) per image (:212).  Under a graph the optimizer object is the captured one and its
        state is zeroed in place instead -- the same thing to Adam (step 0, zero moments)."""
        if self.apr_graph is None:
            self.apr_opt = self._apr_adam(self.apr_opt.param_groups[0]["lr"])
        else:
            _zero_optimizer_state(self.apr_opt)

    def _apr_result(self, pose, first, checks, losses):
        """What DFM_post_processing records for the image (:233-250): the refined network's pose, or the one from before the loop when the
        verification step (iterations 0 and iters - 1) finds PSNR or SSIM lower after the loop than before it."""
        info = {"retreat": False}
        if len(checks) == 2:
            (p0, s0), (p1, s1) = [(float(a), float(b)) for a, b in checks]
            info = {"psnr": (p0, p1), "ssim": (s0, s1), "retreat": p1 < p0 or s1 < s0}       # :242-250
            if info["retreat"]:
                pose = first
        return pose.detach().clone(), losses, info

    def refine_apr(self, photo, feature_target, hist, iters=50, verification=True, mask=None, depth=None):
        """One query image, `pose_only=2`: `photo` [1,3,H,W], `feature_target` [C,H,W] (the query image's features at full
        resolution; cropped here as :125 does).  Returns (pose [3,4] in the regression network's coordinates, losses [iters],
        info = dict(psnr=(first, last), ssim=(first, last), retreat=bool)).  PoseRefiner(graph=True): the iteration is captured on
        first use and replayed (the regression network must be capturable: no host reads, static shapes).
        mask (PoseRefiner(masked=True)): the valid pixels of the CROPPED full-resolution image, [H-20, W-20] (full_resolution_mask);
        the verification step's PSNR / SSIM stay unmasked, as in the reference."""
        return self._run(self._mode(apr=True, verification=verification),
                         self._job(photo, feature_target, hist, mask=mask, depth=depth, apr=True), iters)


def _refuse_sparse(K, pose_model, images, upsample, fused_glue, lietorch):
    """What PoseRefiner(sparse=K) cannot be combined with, said by the constructor."""
    if K < 1:
        raise ValueError(f"nefes_amd: PoseRefiner(sparse={K}): the number of pixels must be positive")
    for bad, what in ((pose_model is not None, "pose_model=: its verification step compares an image, and a sparse refiner renders none"),
                      (int(images) > 1, "images > 1: one image at a time"),
                      (bool(upsample), "upsample=True: there is no frame to up-sample; tinyscale=1 gives full-resolution pixels"),
                      (not fused_glue, "fused_glue=False: the sparse loss runs on the library's loss kernels"),
                      (bool(lietorch), "lietorch=True: the pose chain is ops.pose_compose")):
        if bad:
            raise NotImplementedError("nefes_amd: PoseRefiner(sparse=K) with " + what)


def _camera_buffer(intrinsics, B, device):
    """PoseRefiner's persistent camera: float32 [4] on the device, or [B, 4] for a table of one camera per image.  A device tensor of
    that form is kept as it is (the caller's in-place updates reach the captured iteration); host values are validated
    (ops.as_intrinsics)."""
    if not torch.is_tensor(intrinsics):
        import numpy as np
        intrinsics = torch.from_numpy(np.asarray(intrinsics, dtype=np.float64))
    if intrinsics.dim() == 2 and tuple(intrinsics.shape) != (3, 3):
        if tuple(intrinsics.shape) != (B, 4):
            raise ValueError(f"nefes_amd: PoseRefiner(intrinsics=...) takes one camera or [{B}, 4], one per image; got {tuple(intrinsics.shape)}")
        if intrinsics.device.type != "cpu":
            if intrinsics.dtype != torch.float32 or not intrinsics.is_contiguous():
                raise ValueError("nefes_amd: a table of intrinsics on the device must be contiguous float32")
            return intrinsics.detach()
        return torch.stack([ops.as_intrinsics(r, device) for r in intrinsics.unbind(0)])
    return ops.as_intrinsics(intrinsics, device).detach()


def resized_intrinsics(K, from_hw, to_hw):
    """The camera (fx, fy, cx, cy) of an image resized from (H, W) to (h, w) under the align_corners=False convention of F.interpolate
    and of the loop's bicubic up-sampling -- pixel x of the small image looks where (x + 0.5) W / w - 0.5 of the large one does:
        fx' = fx w / W,  cx' = (cx + 0.5) w / W - 0.5,  and fy', cy' likewise with h / H.
    K: (fx, fy, cx, cy) or a 3 x 3 matrix, host values.  Returns a tuple of four floats (float64 arithmetic)."""
    import numpy as np
    a = np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float64)
    fx, fy, cx, cy = (a[0, 0], a[1, 1], a[0, 2], a[1, 2]) if a.shape == (3, 3) else a
    (H, W), (h, w) = from_hw, to_hw
    sx, sy = float(w) / float(W), float(h) / float(H)
    return (float(fx * sx), float(fy * sy), float((cx + 0.5) * sx - 0.5), float((cy + 0.5) * sy - 0.5))


def resized_depth(D, from_hw, to_hw):
    """A sensor's depth frame [..., H, W] at the rendered resolution (h, w): at each rendered pixel the NEAREST source pixel to its centre,
    under resized_intrinsics' convention -- the centre of pixel x of the small image lies at (x + 0.5) W / w of the large one's continuous
    axis, i.e. in source pixel floor((x + 0.5) W / w) (integer arithmetic).  Nothing is blended: holes stay holes and a depth edge stays
    an edge.  Plain torch indexing, set-up only; the values are not touched (convert units and mark holes before or after)."""
    D = torch.as_tensor(D)
    (H, W), (h, w) = (int(v) for v in from_hw), (int(v) for v in to_hw)
    if tuple(D.shape[-2:]) != (H, W):
        raise ValueError(f"nefes_amd: resized_depth: the frame has shape {tuple(D.shape)}, from_hw says {(H, W)}")
    ys = ((2 * torch.arange(h, device=D.device) + 1) * H).div(2 * h, rounding_mode="floor").clamp_(max=H - 1)
    xs = ((2 * torch.arange(w, device=D.device) + 1) * W).div(2 * w, rounding_mode="floor").clamp_(max=W - 1)
    return D[..., ys[:, None], xs[None, :]]


def _depth_term(depth_weight, depth_huber, fused_glue):
    """PoseRefiner(depth_weight=lambda, depth_huber=delta) validated: (lambda, delta) as floats, or (None, None) without the term.
    delta: the Huber threshold in the scene's units (None: 0.1)."""
    if depth_weight is None:
        if depth_huber is not None:
            raise ValueError(f"nefes_amd: PoseRefiner(depth_huber={depth_huber}) without depth_weight=: there is no depth term to apply it to")
        return None, None
    lam, delta = float(depth_weight), 0.1 if depth_huber is None else float(depth_huber)
    if not (lam > 0 and lam != float("inf")):
        raise ValueError(f"nefes_amd: PoseRefiner(depth_weight={depth_weight}): the weight of the depth term must be positive and finite "
                         "(None: no depth term)")
    if not (delta > 0 and delta != float("inf")):
        raise ValueError(f"nefes_amd: PoseRefiner(depth_huber={depth_huber}): the Huber threshold must be positive and finite, in the "
                         "scene's units")
    if not fused_glue:
        raise NotImplementedError("nefes_amd: PoseRefiner(depth_weight=...) runs on the library's loss kernels (fused_glue=True)")
    return lam, delta


_nothing = lambda *args: None


class _Mode(typing.NamedTuple):
    """What PoseRefiner's two loops differ in -- mode 3 (`refine`: optimise (r, t)) and mode 2 (`refine_apr`: train a copy of a regression
    network) -- as bound methods of one refiner (PoseRefiner._mode).  Capture (_capture), loop (_run, _step) and stream driver (_drive)
    are written once on top of it; where the modes order their device work differently, the difference is a field here."""
    apr: bool                   # mode 2; its captured iteration lives in `apr_graph` (mode 3: `graph`)
    on_device: typing.Callable  # job -> job with its tensors on the device (mode 2 copies inside set_state instead)
    set_state: typing.Callable  # (*job): the image's state and a fresh optimizer state, written in place
    iteration: typing.Callable  # (): one eager iteration -- what is warmed up, captured, and run where nothing is replayed
    prepare: typing.Callable    # (mode, job): what _drive has the refiner do on the CALLER'S stream first (capture on first use)
    read: typing.Callable       # () -> the result on the device
    read_own: typing.Callable   # the same on a refiner's own stream (mode 2 copies it there)
    finish: typing.Callable     # (read(), before(), [check() ...], losses) -> what the caller gets
    before_capture: typing.Callable = _nothing      # (): between warm-up and capture
    before: typing.Callable = _nothing              # () -> recorded in front of the loop (mode 2: the regression network's first pose)
    check: typing.Callable = _nothing               # (i, iters) -> recorded behind iteration i, or None (mode 2: the verification pair)
    slot = property(lambda self: "apr_graph" if self.apr else "graph")


def _zero_optimizer_state(opt):
    """A torch optimizer back to step 0 with zero moments, IN PLACE: a captured graph keeps updating the same state tensors."""
    with torch.no_grad():
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()


def _apr_kernels_bit_stable(r, photo, feature_target, hist, mask=None, depth=None, trials=6):
    """EMPIRICAL guard for refine_apr_concurrently.  The regression network, its backward, torch's Adam and the verification step are the
    CALLER'S / torch's kernels; next to another stream's field kernels such code is exposed to the packed-fp32 finding of DESIGN.md 4.7
    (hipcc vectorises torch's kernels the way it vectorised ours) -- whether a given network's kernels contain the affected forms cannot be
    read off its Python.  So it is tried: two eager iterations + the verification step from the image's initial state, alone on the
    device and `trials` times with this library's fine-field forward running on a second stream, every result compared bit for bit
    (loss, every parameter of the working network, PSNR, SSIM).  The affected instructions go wrong in 0.05-0.35 % of their executions on
    a quarter of the lanes: a kernel that carries one does not survive six trials of this.  Cached on the network object."""
    key = "_nefes_bit_stable_next_to_field_kernels"
    if getattr(r.apr_base, key, None) is not None:
        return getattr(r.apr_base, key)
    from . import lib as L
    dev = r.dev
    fine = r.kw["network_fine"]
    pk = fine.packed_any()
    g = torch.Generator().manual_seed(5)
    N, S = 4800, 128
    ro = (torch.randn(N, 3, generator=g) * 0.1).to(dev)
    rd = nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(dev)
    z = (torch.rand(N, S, generator=g).sort(-1).values * 3 + 0.2).to(dev)
    side = torch.cuda.Stream(device=dev)

    def run(storm):
        r._apr_set_state(photo, feature_target, hist, mask, depth)
        torch.cuda.synchronize(dev)
        keep = []
        if storm:
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(8):                         # ~5 ms of field kernels: longer than the sequence under test
                    keep.append(ops.field_from_rays(ro, rd, rd, z, pk, L.FIELD_FULL))
        r._apr_iteration()
        r._apr_iteration()
        ps, ss = r._verification(as_tensors=True)
        out = [r.loss.detach().clone(), ps.detach().clone(), ss.detach().clone()] + [p.detach().clone() for p in r.apr.parameters()]
        torch.cuda.synchronize(dev)
        return out

    was_graph = r.apr_graph
    views = (r._rgb, r._x_rgb)                             # (a captured iteration's views of ITS static buffers: eager calls re-point them)
    r.apr_graph = None                                     # (eager iterations; _apr_fresh_adam then builds a fresh optimizer per run)
    try:
        solo = run(False)
        ok = all(all(torch.equal(a, b) for a, b in zip(solo, run(True))) for _ in range(trials))
    finally:
        r.apr_graph = was_graph
        if was_graph is not None:                          # the captured optimizer object and buffer views must be the live ones again
            r.apr_opt = r._captured_apr_opt
            r._rgb, r._x_rgb = views
    setattr(r.apr_base, key, bool(ok))
    return bool(ok)


def _check_concurrent(refiners, apr=False):
    """What refine_concurrently's guarantees rest on, checked instead of assumed.
    (1) No shared mutable state between streams: refiners that share a FusionNet must not update its BatchNorm's running statistics
        (a read-modify-write of the module's buffers from several streams: lost counter increments, non-deterministic statistics).
    (2) Every kernel of an iteration is this library's: the bit-identity of concurrent and solo trajectories holds for kernels built
        without the packed-fp32 op_sel:[0,1] forms; MIOpen / ATen kernels next to another stream's MFMA kernels are
        exposed to it.  A refiner on the torch glue, torch convolutions / BatchNorm or torch.optim.Adam is refused here."""
    shared = {}
    for r in refiners:
        fnet = r.coarse.fusion_net
        bn_tracks = (not fnet.no_BN) and r.B == 1 and fnet.net[-1].training and fnet.net[-1].track_running_stats
        other = shared.setdefault(id(fnet), r)
        if other is not r and bn_tracks and (r.bn_running_stats or other.bn_running_stats):
            raise ValueError("nefes_amd: refine_concurrently: these refiners share one FusionNet whose BatchNorm would update its running "
                             "statistics from several streams at once; construct them with PoseRefiner(..., bn_running_stats=False)")
        # (apr: the regression network and its optimizer are torch's by construction; refine_apr_concurrently tries them instead)
        in_house = (r.fused_glue and (apr or isinstance(r.opt, ops.FusedAdam)) and fnet.HIP_CONVS and (fnet.no_BN or fnet.HIP_BATCHNORM)
                    and fnet._use_hip(r.hist))
        if not in_house:
            raise ValueError("nefes_amd: refine_concurrently needs every refiner on the library's own kernels (fused_glue=True, "
                             "lietorch=False, FusionNet.HIP_CONVS / HIP_BATCHNORM, frozen FusionNet on the GPU): torch's kernels next to "
                             "another stream's field kernels are exposed to the packed-fp32 finding of DESIGN.md 4.7; run such "
                             "refiners one after the other (PoseRefiner.refine)")




def _drive(name, refiners, jobs, iters, mode_of, guard=None, sync=False):
    """The stream driver of refine_concurrently / refine_apr_concurrently: rounds of len(refiners) jobs; per round the checks, capture on
    first use (one refiner at a time, on the caller's stream), every refiner's own stream behind the caller's, the image's state written
    on it, the iterations issued round-robin, the results read on the own streams, and the caller's stream behind them all."""
    if not refiners or not jobs:
        raise ValueError(f"nefes_amd: {name} needs at least one PoseRefiner and one job")
    if len({id(r) for r in refiners}) != len(refiners):
        raise ValueError(f"nefes_amd: {name} needs DISTINCT PoseRefiner objects (each owns the static buffers of its image)")
    modes = [mode_of(r) for r in refiners]                 # (mode 2 refuses a refiner built without pose_model= here)
    if len(jobs) > len(refiners):
        return [out for k in range(0, len(jobs), len(refiners))
                for out in _drive(name, refiners[:len(jobs[k:k + len(refiners)])], jobs[k:k + len(refiners)], iters, mode_of, guard, sync)]
    refiners, modes = refiners[:len(jobs)], modes[:len(jobs)]
    dev = refiners[0].dev
    _check_concurrent(refiners, apr=modes[0].apr)
    if guard is not None:
        guard(refiners, jobs)
    jobs = [m.on_device(job) for m, job in zip(modes, jobs)]
    for m, job in zip(modes, jobs):
        m.prepare(m, job)
    cur = torch.cuda.current_stream(dev)
    for r in refiners:
        if getattr(r, "_own_stream", None) is None:
            r._own_stream = torch.cuda.Stream(device=dev)
        r._own_stream.wait_stream(cur)
    losses = [torch.empty((iters,) + tuple(r.loss.shape), device=dev) for r in refiners]
    before, checks, raw = [], [[] for _ in refiners], []
    for r, m, job in zip(refiners, modes, jobs):
        with torch.cuda.stream(r._own_stream):
            m.set_state(*job)
            before.append(m.before())
    for i in range(iters):
        for r, m, l, c in zip(refiners, modes, losses, checks):
            with torch.cuda.stream(r._own_stream):
                r._step(m, i, iters, l, c)
    for r, m in zip(refiners, modes):
        with torch.cuda.stream(r._own_stream):
            raw.append(m.read_own())
    for r in refiners:
        cur.wait_stream(r._own_stream)
    if sync:
        torch.cuda.synchronize(dev)
    return [m.finish(*done) for m, done in zip(modes, zip(raw, before, checks, losses))]


def refine_concurrently(refiners, jobs, iters=50):
    """K query images refined AT THE SAME TIME: one PoseRefiner (its own static buffers and captured graph; the frozen networks can be
    shared) and one HIP stream per image, replays issued round-robin.  An iteration is ~1.45 ms of field kernels, which hold the whole
    chip at its power limit, and ~0.3 ms of FusionNet convolutions, loss and pose kernels that are bound by launch and L2 latency on a
    fraction of the CUs: alone on the device those 0.3 ms are idle silicon, next to another image's field kernels they are nearly
    free (two images: -8 % per image; tools/two_streams.py).  Every image walks exactly the trajectory it walks alone -- bit for bit
    (tests/test_gpu_streams.py; that test is also what found the packed-fp32 op_sel instruction of DESIGN.md 4.7).
    jobs = [(init_c2w, feature_target, hist), ...] as PoseRefiner.refine takes them -> [(refined c2w, losses [iters]), ...] in job order;
    a job for a PoseRefiner(masked=True) may carry the image's mask as a fourth element.
    More jobs than refiners: rounds of len(refiners) images (the last one smaller).
    Refiners that share a FusionNet are constructed with bn_running_stats=False, and every refiner runs on the library's own kernels
    (_check_concurrent refuses anything else: see there)."""
    return _drive("refine_concurrently", refiners, jobs, iters, lambda r: r._mode())


def refine_apr_concurrently(refiners, jobs, iters=50, verification=True, verify_kernels=True):
    """refine_apr for K query images at the same time (the shipped default mode, `pose_only = 2`): one PoseRefiner(pose_model=...) and
    one HIP stream per image, iterations replayed round-robin like refine_concurrently.  jobs = [(photo, feature_target, hist), ...] ->
    [(pose [3,4], losses [iters], info), ...] in job order, each identical to what refine_apr returns for that image alone; a fourth
    element of a job is the image's mask (PoseRefiner(masked=True)).
    The regression network's kernels are the caller's: `verify_kernels` first TRIES them next to this library's field kernels
    (_apr_kernels_bit_stable) and raises if a result moves -- run such a network's images one after the other (refine_apr)."""
    def guard(refiners, jobs):
        for r, job in zip(refiners, jobs):
            if not _apr_kernels_bit_stable(r, *job):
                raise RuntimeError("nefes_amd: this regression network's kernels (or torch's Adam / the verification step) do not give "
                                   "bit-identical results next to another stream's field kernels (DESIGN.md 4.7): refine its images "
                                   "one after the other with PoseRefiner.refine_apr")
    return _drive("refine_apr_concurrently", refiners, jobs, iters, lambda r: r._mode(apr=True, verification=verification),
                  guard=guard if verify_kernels else None, sync=True)
