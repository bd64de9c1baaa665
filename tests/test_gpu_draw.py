"""The device-side pixel draw on the GPU: nefes_draw_pixels against the numpy restatement of its contract (tests/draw_ref.py), bit for bit,
at every geometry where the kernels take another turn; under graph replay; handed to render_poses; and PoseRefiner(sparse=K, redraw=R).
Scene, cameras and the refiner factory are those of tests/test_gpu_intrinsics.py, the sparse chain by hand is tests/test_gpu_pixels.py's;
the CPU twin is tests/test_draw_args.py."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import draw_ref as D
from tests import parity_log as P
from tests import pixels_ref as R
from tests.test_gpu_intrinsics import C, DEV, FOCAL, RH, RW, T, job, maps_of, refiner, scene       # noqa: F401  (scene: a fixture)
from tests.test_gpu_pixels import by_hand, frame_mask, frame_points, pose_error

pytestmark = pytest.mark.gpu

SEEDS = (0, 2 ** 40 + 3)
TICKS = (0, 7, 2 ** 33 + 1)                      # the last: the epoch's high word is non-zero


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


def state_at(seed, tick):
    return torch.tensor([seed, tick], dtype=torch.int64, device=DEV)


def case_mask(B, H, W, kind):
    if kind is None:
        return None
    m = np.zeros((B, H, W), np.uint8)
    if kind == "full-4-none":                     # one image fully valid, one with 4 valid pixels, one with none
        m[0] = 1
        m[1].reshape(-1)[[5, 17, 18, 62]] = 1
    else:                                         # a random 70 % mask, values other than 1 among the valid ones
        rng = np.random.default_rng(3)
        m[:] = (rng.random((B, H, W)) < 0.7) * rng.integers(1, 256, (B, H, W))
    return m


# one pixel; every pixel of a frame smaller than a wave; part of a chunk; three images of which one has too few and one no valid pixel;
# two chunks per image and every pixel drawn; the refiner's frame (three chunks); fifty chunks, masked; eight images, K near n
GEOMETRIES = [(1, 1, 1, 1, None), (1, 3, 5, 15, None), (1, 12, 16, 48, None), (3, 7, 9, 10, "full-4-none"), (2, 33, 65, 2145, None),
              (1, 60, 80, 256, None), (1, 240, 427, 1024, "random"), (8, 30, 53, 1536, None)]


@pytest.mark.parametrize("B,H,W,K,kind", GEOMETRIES)
def test_draw_is_the_reference_bit_for_bit(ops, B, H, W, K, kind):
    mask = case_mask(B, H, W, kind)
    mask_dev = None if mask is None else torch.from_numpy(mask).to(DEV)
    for seed in SEEDS:
        for tick in TICKS:
            state = state_at(seed, tick)
            n_valid = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            px = ops.draw_pixels(H, W, K, state, B=B, mask=mask_dev, advance=False, n_valid=n_valid)
            want_px, want_n = D.draw(B, H, W, K, seed, tick, mask=mask)
            assert px.dtype == torch.float32 and tuple(px.shape) == (B, K, 2) and px.is_contiguous()
            assert np.array_equal(n_valid.cpu().numpy(), want_n), (seed, tick, n_valid.tolist(), want_n.tolist())
            assert torch.equal(px.cpu(), torch.from_numpy(want_px)), (seed, tick)
            assert state.tolist() == [seed, tick]                             # advance=False leaves the state alone
            again = ops.draw_pixels(H, W, K, state, B=B, mask=mask_dev, advance=True)      # n_valid NULL; two launches of one state
            assert torch.equal(again, px) and state.tolist() == [seed, tick + 1]
    if kind == "full-4-none":
        assert want_n.tolist() == [63, 4, 0] and not want_px[2].any()


def test_period_advance_and_in_place_outputs(ops):
    H, W, K, seed = 12, 16, 48, 12345
    state = state_at(seed, 3)
    out = torch.zeros(K, 2, device=DEV)                                       # B = 1: a [K, 2] list is written in place
    draws = []
    for tick in (3, 4, 5, 6):
        assert state.tolist() == [seed, tick]
        res = ops.draw_pixels(H, W, K, state, period=3, out=out)
        assert res.data_ptr() == out.data_ptr() and tuple(res.shape) == (1, K, 2)
        draws.append(out.clone().cpu())
    assert state.tolist() == [seed, 7]
    epoch1, epoch2 = (torch.from_numpy(D.draw(1, H, W, K, seed, e)[0][0]) for e in (1, 2))
    assert all(torch.equal(d, epoch1) for d in draws[:3]) and torch.equal(draws[3], epoch2) and not torch.equal(epoch1, epoch2)
    # a bool [H, W] mask is read in place like a uint8 [1, H, W] one
    m = torch.from_numpy(D.draw(1, H, W, 100, 1, 0)[0][0]).long()
    mask = torch.zeros(H, W, dtype=torch.bool)
    mask[m[:, 1], m[:, 0]] = True
    want = torch.from_numpy(D.draw(1, H, W, K, seed, 2, mask=mask[None].numpy())[0])
    for form in (mask.to(DEV), mask[None].to(torch.uint8).to(DEV)):
        assert torch.equal(ops.draw_pixels(H, W, K, state_at(seed, 2), mask=form, advance=False).cpu(), want)


def test_a_replayed_graph_draws_the_next_batch(ops):
    B, H, W, K, seed, t0 = 2, 33, 65, 40, 2 ** 40 + 3, 2 ** 33 - 2            # (the epoch's high word changes on the way)
    state, out, n_valid = state_at(seed, t0), torch.zeros(B, K, 2, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.draw_pixels(H, W, K, state, B=B, out=out, n_valid=n_valid)            # (warm-up: the workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.draw_pixels(H, W, K, state, B=B, out=out, n_valid=n_valid)
    state.copy_(state_at(seed, t0))
    for k in range(4):
        g.replay()
        assert torch.equal(out.cpu(), torch.from_numpy(D.draw(B, H, W, K, seed, t0 + k)[0])), k
        assert state.tolist() == [seed, t0 + k + 1] and n_valid.tolist() == [H * W] * B


def test_render_poses_takes_the_drawn_lists(ops, scene):
    from nefes_amd.render import render, render_poses
    px = ops.draw_pixels(RH, RW, 8, ops.draw_state(4, DEV), B=2)
    assert not torch.equal(px[0], px[1])
    poses = torch.stack([O.bench_pose(), O.se3_exp_pose((0.05, 0.15, -0.1), (0.2, 0.1, 0.25))]).to(DEV)
    both = maps_of(render_poses(RH, RW, FOCAL, poses, near=0., far=4., pixels=px, **scene))
    for b in range(2):
        one = maps_of(render(RH, RW, FOCAL, c2w=poses[b], near=0., far=4., pixels=px[b], **scene))
        assert all(torch.equal(one[k], both[k][b]) for k in one), b


# ---- PoseRefiner(sparse=K, redraw=R) ----------------------------------------------------------------------------------------------
KP, SEED = 40, 5


def frame_hw(g):
    H, W, _ = g["hwf"].tolist()
    ts = int(g["tinyscale"])
    return int(H // ts), int(W // ts)


def drawn(g, epoch, K=KP, seed=SEED, mask=None):
    h, w = frame_hw(g)
    return torch.from_numpy(D.draw(1, h, w, K, seed, epoch, mask=None if mask is None else mask.numpy()[None])[0][0]).to(DEV)


@pytest.mark.parametrize("per_pixel,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_redrawn_iteration_is_the_chain_by_hand_at_the_epochs_draw(golden, per_pixel, masked):
    g = golden("refine")
    init, target, hist = job(g)
    mask = frame_mask(g) if masked else None
    r = refiner(g, False, sparse=KP, redraw=1, seed=SEED, per_pixel=per_pixel, masked=masked)
    r._reset(init, target, hist, mask, None)
    lists = []
    for epoch in range(5):
        px = drawn(g, epoch, mask=mask)
        want = by_hand(r, target, px, per_pixel, mask)                        # at the state the iteration starts from
        r._iteration()
        assert torch.equal(r.pixels, px), epoch
        assert torch.equal(r.loss, want[0]), (epoch, float(r.loss), float(want[0]))
        lists.append(px)
        if masked:
            assert bool((mask.to(DEV)[px[:, 1].long(), px[:, 0].long()] > 0).all()) and bool(r.mask.all()) and tuple(r.mask.shape) == (1, KP)
    assert r.draw_state.tolist() == [SEED, 5] and not torch.equal(lists[0], lists[1])
    assert torch.equal(r.features(), r._sparse_features().detach())           # the features at the list currently in self.pixels


def test_redrawn_loop_graph_equals_eager_and_images_are_independent(golden):
    g = golden("refine")
    first, R_ = job(g), 2
    eager, graph = refiner(g, False, sparse=KP, redraw=R_, seed=SEED), refiner(g, True, sparse=KP, redraw=R_, seed=SEED)
    a, b = eager.refine(*first, 2 * R_ + 1), graph.refine(*first, 2 * R_ + 1)
    print("[redraw graph vs eager] losses", [f"{float(v):.6f}" for v in a[1]])
    assert graph.graph is not None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for r in (eager, graph):
        assert torch.equal(r.pixels, drawn(g, 2)) and r.draw_state.tolist() == [SEED, 2 * R_ + 1]
    # a second image on the same refiners walks the trajectory of a fresh refiner: the state is rewritten per image
    second = (T(g["true_c2w"]).float().to(DEV),) + first[1:]
    fresh = refiner(g, False, sparse=KP, redraw=R_, seed=SEED).refine(*second, 3)
    for r in (eager, graph):
        again = r.refine(*second, 3)
        assert torch.equal(again[0], fresh[0]) and torch.equal(again[1], fresh[1])
    assert not torch.equal(fresh[1], a[1][:3])


def test_a_draw_that_never_changes_is_the_fixed_list(golden):
    g = golden("refine")
    never = refiner(g, False, sparse=KP, redraw=10 ** 9, seed=SEED).refine(*job(g), 4)
    fixed = refiner(g, False, sparse=KP).refine(*job(g), 4, pixels=drawn(g, 0))
    assert torch.equal(never[0], fixed[0]) and torch.equal(never[1], fixed[1])


def test_redraw_refusals_on_the_device(golden):
    g = golden("refine")
    h, w = frame_hw(g)
    r = refiner(g, False, sparse=KP, redraw=1, masked=True)
    few = torch.zeros(h, w, dtype=torch.uint8)
    few.reshape(-1)[:KP - 1] = 1
    with pytest.raises(ValueError, match=f"{KP - 1} valid ones"):
        r.refine(*job(g), 1, mask=few)
    few.reshape(-1)[KP - 1] = 1                                               # exactly K valid pixels: every one of them, each iteration
    r.refine(*job(g), 2, mask=few)
    assert torch.equal(r.pixels, R.grid_pixels(w, 0, h)[:KP].to(DEV))
    with pytest.raises(ValueError, match="redraw"):
        r.set_pixels(torch.zeros(KP, 2))
    with pytest.raises(ValueError, match="pixels="):
        r.refine(*job(g), 1, pixels=torch.zeros(KP, 2))


def test_redrawn_refinement_descends_like_the_fixed_list(golden):
    """The setting of test_gpu_pixels.py::test_sparse_refinement_descends -- the library's own features at the true pose as the target, 96
    points, 20 iterations from the fixture's perturbed start -- with a fixed list and with redraw=1 (there the target FRAME is the
    features of every pixel at the true pose, which the iteration samples at its draw).  The redrawn run's final rotation error is at
    most twice the fixed run's: a draw whose target and pixels do not pair up leaves the error at the start's, 3.4 x the fixed list's
    (profiles/sparse_refine/README.md); gradient noise from changing batches is not expected to cost a factor of two."""
    g = golden("refine")
    init, frame, hist = job(g)
    h, w = frame_hw(g)
    true = T(g["true_c2w"]).float().to(DEV)
    px = frame_points(g, 96, seed=9)
    fixed = refiner(g, False, sparse=96)
    fixed._reset(true, frame, hist, None, px)
    target = fixed.features()
    fixed._reset(init, frame, hist, None, px)
    with torch.no_grad():
        fixed.target.copy_(target)
    whole = refiner(g, False, sparse=h * w)                                   # every pixel's features at the true pose: [C, h, w]
    whole._reset(true, frame, hist, None, R.grid_pixels(w, 0, h).to(DEV))
    true_frame = whole.features().reshape(-1, h, w).contiguous()
    redrawn = refiner(g, False, sparse=96, redraw=1, seed=9)
    redrawn._reset(init, true_frame, hist, None, None)
    start = pose_error(fixed._refined_pose(), true)
    end = {}
    for name, r in (("fixed", fixed), ("redraw=1", redrawn)):
        losses = []
        for _ in range(20):
            r._iteration()
            losses.append(float(r.loss))
        end[name] = pose_error(r._refined_pose(), true)
        print(f"[redraw descent] {name}: loss {losses[0]:.4e} -> {losses[-1]:.4e}; |dt| {start[0]:.4f} -> {end[name][0]:.4f}; "
              f"angle {start[1]:.3f} -> {end[name][1]:.3f} deg")
    P.record("redraw_refine", "20 iterations at 96 points, fixed list vs redraw=1", deg_first=start[1], deg_fixed=end["fixed"][1],
             deg_redrawn=end["redraw=1"][1], dt_first=start[0], dt_fixed=end["fixed"][0], dt_redrawn=end["redraw=1"][0])
    assert end["redraw=1"][1] <= 2 * end["fixed"][1], (end, start)
