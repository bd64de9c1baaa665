"""Digests of the autograd Functions of nefes_amd/ops.py that tools/ab_identical.py reaches in none of its modes, for A/B revisions of
the HOST code on one library:
    NEFES_HIP_LIB=<lib> python tools/ab_ops_functions.py
prints one sha256 per forward output and per input gradient of FieldFromRays, FieldFromPoints, FieldFromEncoding, FieldFromRaysHashGrid
and FieldFromRaysFH in every mode that has a backward (the forward alone where it has none), of FeatHead, of RenderFineFH with the head
applied inside (ab_identical.py --refine reaches it with emit_gmap) and with the depth output, of conv2d_same_train with trainable and
with frozen parameters, and of batch_norm_train / batch_norm_train_frozen (running statistics included).  3 rays x 50 samples = one full
128-sample tile and a ragged one; fixed seeds.  Only names an earlier commit's ops.py has as well are called, so the same file runs in
its tree (copy it there).  Compare the lines that do not start with '#'."""
import hashlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import lib as L
from nefes_amd import ops
from nefes_amd.field import NeRFH_NFF

dev = torch.device('cuda')
N, S = 3, 50
SIGMA, STATIC, FULL = L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL
g = torch.Generator(device='cpu').manual_seed(1)
rnd = lambda *shape: torch.randn(*shape, generator=g)
o = (rnd(N, 3) * 0.3).to(dev)
d = torch.nn.functional.normalize(rnd(N, 3), dim=-1).to(dev)
v = torch.nn.functional.normalize(rnd(N, 3), dim=-1).to(dev)
z = torch.sort(torch.rand(N, S, generator=g) * 4, -1)[0].to(dev)
pts = (o[:, None] + d[:, None] * z[..., None]).contiguous()
enc = (rnd(N, S, 32) * 0.5).to(dev)


def dig(t):
    return "none" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def out(tag, **tensors):
    torch.cuda.synchronize()
    print(f"{tag:58s}", "  ".join(f"{k} {dig(t)}" for k, t in tensors.items()), flush=True)


def both_ways(tag, fn, inputs, backward=True):
    """fn(*leaves) -> the outputs; digests of them and, after a fixed upstream on each, of every leaf's gradient"""
    leaves = {k: t.clone().requires_grad_(backward) for k, t in inputs.items()}
    outs = fn(*leaves.values())
    outs = (outs,) if torch.is_tensor(outs) else tuple(outs)
    grads = {}
    if backward:
        up = [(torch.randn(y.shape, generator=torch.Generator(device='cpu').manual_seed(7 + i)) * 0.1).to(dev) for i, y in enumerate(outs)]
        sum((y * u).sum() for y, u in zip(outs, up)).backward()
        grads = {"d " + k: t.grad for k, t in leaves.items()}
    out(tag, **{f"out{i}": y for i, y in enumerate(outs)}, **grads)


net = lambda **kw: NeRFH_NFF('fine', encode_transient=True, **kw).requires_grad_(False).to(dev)
tuned, ext = net(W=128, f_dim=128, encode_appearance=True), net(W=256, f_dim=16, in_channels_xyz=32)
grid = ops.HashGrid(8.0, log2_hashmap_size=14, device=dev)
grid.table.copy_((rnd(*grid.table.shape) * 0.5).to(dev))
packs = (("W128 C128", tuned.packed()), ("generic W64 D6 C16", net(D=6, W=64, f_dim=16).packed_generic()))
packs_ext = (("W256 C16 ext", ext.packed(), (FULL,)), ("generic W96 D5 C128 ext", net(D=5, W=96, f_dim=128, in_channels_xyz=32).packed_generic(), (STATIC, FULL)))
rays = dict(rays_o=o, rays_d=d, viewdirs=v)
print("# lib", os.environ.get("NEFES_HIP_LIB") or "shipped", "ABI", L.ABI_VERSION)
for name, pk in packs:
    for mode in (SIGMA, STATIC, FULL):
        both_ways(f"{name} FieldFromRays mode {mode}", lambda a, b, c: ops.FieldFromRays.apply(a, b, c, z, pk, mode), rays, mode != SIGMA)
        both_ways(f"{name} FieldFromPoints mode {mode}", lambda p, c: ops.FieldFromPoints.apply(p, c, pk, mode), dict(pts=pts, viewdirs=v), mode != SIGMA)
    both_ways(f"{name} FieldFromPoints mode {SIGMA} no viewdirs", lambda p: ops.FieldFromPoints.apply(p, None, pk, SIGMA), dict(pts=pts), False)
for name, pk, with_backward in packs_ext:
    for mode in (SIGMA, STATIC, FULL):
        if mode == STATIC and STATIC not in with_backward:
            continue
        both_ways(f"{name} FieldFromEncoding mode {mode}", lambda e, c: ops.FieldFromEncoding.apply(e, c, pk, mode), dict(enc=enc, viewdirs=v),
                  mode in with_backward)
    both_ways(f"{name} FieldFromEncoding mode {SIGMA} no viewdirs", lambda e: ops.FieldFromEncoding.apply(e, None, pk, SIGMA), dict(enc=enc), False)
assert ops.hashgrid_fused_ok(ext.packed(), grid)
for mode in (SIGMA, FULL):
    both_ways(f"W256 C16 ext FieldFromRaysHashGrid mode {mode}", lambda a, b, c: ops.FieldFromRaysHashGrid.apply(a, b, c, z, ext.packed(), mode, grid),
              rays, mode == FULL)
pk_fh, w_f, w_f_t, b_f = tuned.packed_fh()
both_ways("W128 FieldFromRaysFH", lambda a, b, c: ops.FieldFromRaysFH.apply(a, b, c, z, pk_fh), rays)
both_ways("W128 FeatHead", lambda m: ops.FeatHead.apply(m, w_f, w_f_t, b_f), dict(gmap=(rnd(N, 65) * 0.5).to(dev)))
for tag, more in (("head inside", ()), ("emit_gmap", (True,)), ("head inside, depth", (False, True)), ("emit_gmap, depth", (True, True))):
    both_ways(f"W128 RenderFineFH {tag}", lambda a, b, c: ops.RenderFineFH.apply(a, b, c, z, pk_fh, w_f, w_f_t, b_f, L.COMP_TRANSIENT, 0.1, *more), rays)
both_ways("W128 RenderFineFH rgb alone", lambda a, b, c: ops.RenderFineFH.apply(a, b, c, z, pk_fh, w_f, w_f_t, b_f, L.COMP_TRANSIENT, 0.1)[0], rays)

# (B, Cin, Cout, k, H, W): the smallest layer, and one with more than one tile of output channels and of pixels
for B, cin, cout, k, H, W in ((1, 3, 4, 3, 5, 7), (1, 3, 4, 5, 5, 7), (2, 19, 33, 3, 16, 17), (2, 19, 33, 5, 16, 17)):
    x, w, b = rnd(B, cin, H, W).to(dev), (rnd(cout, cin, k, k) / (cin * k * k) ** 0.5).to(dev), (rnd(cout) * 0.1).to(dev)
    for relu in (True, False):
        tag = f"conv {B}x{cin}x{H}x{W} -> {cout}, k {k}, relu {int(relu)}"
        both_ways(tag + " train", lambda a, ww, bb: ops.conv2d_same_train(a, ww, bb, relu=relu), dict(x=x, weight=w, bias=b))
        both_ways(tag + " train, no bias", lambda a, ww: ops.conv2d_same_train(a, ww, None, relu=relu), dict(x=x, weight=w))
        both_ways(tag + " train, frozen weights", lambda a: ops.conv2d_same_train(a, w, b, relu=relu), dict(x=x))
        both_ways(tag + " frozen", lambda a: ops.frozen_conv2d(a, w, b, relu=relu), dict(x=x))

for B, Cc, H, W in ((1, 6, 5, 7), (3, 128, 9, 11)):
    x = rnd(B, Cc, H, W).to(dev)
    bn = torch.nn.BatchNorm2d(Cc).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(rnd(Cc).to(dev) * 0.3 + 1), bn.bias.copy_(rnd(Cc).to(dev) * 0.1)
    stats = lambda: dict(running_mean=bn.running_mean, running_var=bn.running_var, batches=bn.num_batches_tracked)
    tag = f"batch norm {B}x{Cc}x{H}x{W}"
    both_ways(tag + " train", lambda a: ops.batch_norm_train(a, bn), dict(x=x))
    out(tag + " train: parameters", d_weight=bn.weight.grad, d_bias=bn.bias.grad, **stats())
    both_ways(tag + " train, statistics left alone", lambda a: ops.batch_norm_train(a, bn, track_stats=False), dict(x=x))
    out(tag + " train, statistics left alone: statistics", **stats())
    bn.requires_grad_(False)
    for per_image, track in ((False, True), (True, True), (False, False)):
        both_ways(f"{tag} frozen per_image {int(per_image)} track {int(track)}",
                  lambda a: ops.batch_norm_train_frozen(a, bn, per_image=per_image, track_stats=track), dict(x=x))
        out(f"{tag} frozen per_image {int(per_image)} track {int(track)}: statistics", **stats())
