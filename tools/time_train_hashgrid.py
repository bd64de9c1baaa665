"""Train-mode step of the hash-grid field (BASELINE configs[3]: 16 levels x 2 features, 2^19 entries, bound 25, fine 8x256 C=16 with
the transient head), 4096 rays x 192 samples, table + MLP weights trainable: forward (encode + train-mode field), field backward,
weight gradients, the table-gradient scatter in both forms (wave-merged default / plain atomics, NEFES_HG_TABLE_ATOMIC) and a torch
Adam step over the table, in ms (HIP events; median of 5 after 2 warm-up steps)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import lib as L, ops, train as TR        # noqa: E402
from nefes_amd.field import NeRFH_NFF                  # noqa: E402
from oracle import hashgrid_ref as HG                  # noqa: E402

dev = "cuda"
N, S, BOUND = 4096, 192, 25.0
M = N * S
fine = NeRFH_NFF('fine', W=256, f_dim=16, in_channels_xyz=32, encode_appearance=True, encode_transient=True).to(dev)
grid = ops.HashGrid(BOUND, table=HG.make_table(0) * 3e3)
grid.table.requires_grad_(True)
g = torch.Generator().manual_seed(0)
o = ((torch.rand(N, 3, generator=g) - .5) * 10).to(dev)
d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(dev)
z = torch.sort(torch.rand(N, S, generator=g) * 20, -1)[0].to(dev)
G = torch.randn(N, 25, S, generator=g).to(dev)
names = TR.param_names(fine, L.FIELD_FULL)
sd = dict(fine.named_parameters())
opt = torch.optim.Adam(grid.parameters(), lr=1e-2)


def timed(fn, reps=5, warm=2):
    out = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


# one whole step, per launch (ops.TIMERS brackets every C-ABI launch with events)
steps = []
for it in range(7):
    ops.TIMERS = {}
    for p in fine.parameters():
        p.grad = None
    grid.table.grad = None
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    raw = TR.FieldTrainEncoded.apply(grid(pts), d, fine, L.FIELD_FULL, *[sd[n] for n in names])
    (raw * G).sum().backward()
    torch.cuda.synchronize()
    steps.append({k: sum(a.elapsed_time(b) for a, b in v) for k, v in ops.TIMERS.items()})
ops.TIMERS = None
med = {k: statistics.median(s[k] for s in steps[2:]) for k in steps[-1]}

# the field backward alone (the fused dX kernel), to split field_bwd_train into the dX launch and the weight gradients
pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
enc = torch.empty(M, 32, device=dev)
L.check(L.load().nefes_hashgrid_fwd(grid.desc, grid.table.data_ptr(), M, pts.data_ptr(), enc.data_ptr(), ops._stream()), "fwd")


def field_bwd_only():
    enc_r = enc.view(N, S, 32).detach().requires_grad_(True)
    raw_ = TR.FieldTrainEncoded.apply(enc_r, d, fine, L.FIELD_FULL, *[p.detach() for p in (sd[n] for n in names)])
    torch.autograd.grad((raw_ * G).sum(), enc_r)


t_fwd_bwd_nodw = timed(field_bwd_only)
t_fwd_only = timed(lambda: TR.FieldTrainEncoded.apply(enc.view(N, S, 32), d, fine, L.FIELD_FULL,
                                                        *[p.detach() for p in (sd[n] for n in names)]))
g_enc = torch.randn(M, 32, device=dev)


def table_kernel(form):
    os.environ["NEFES_HG_TABLE_ATOMIC"] = "1" if form == "atomic" else "0"
    buf = torch.zeros_like(grid.table.detach())
    ws = torch.empty(int(L.load().nefes_hashgrid_bwd_table_workspace(grid.desc)), dtype=torch.uint8, device=dev)
    t = timed(lambda: L.check(L.load().nefes_hashgrid_bwd_table(grid.desc, M, pts.data_ptr(), g_enc.data_ptr(), buf.data_ptr(),
                                                                   ws.data_ptr(), ops._stream()), "bwd_table"))
    os.environ.pop("NEFES_HG_TABLE_ATOMIC", None)
    return t


t_merged, t_atomic = table_kernel("merged"), table_kernel("atomic")
grid.table.grad = torch.randn_like(grid.table)
t_adam = timed(lambda: opt.step())

added = M * 16 * 8 * 2 * 4                               # bytes added into the table per step
t_field_bwd = t_fwd_bwd_nodw - t_fwd_only
t_dw = med["field_bwd_train[h3,ext]"] - t_field_bwd
print(f"hash-grid train step, fine 8x256 C=16, {N} rays x {S} samples = {M} samples, bound {BOUND}")
print(f"  forward: hashgrid_fwd {med['hashgrid_fwd']:.2f} ms + field_fwd_train[h3,ext] {med['field_fwd_train[h3,ext]']:.2f} ms")
print(f"  field backward (fused dX kernel) {t_field_bwd:.2f} ms, weight gradients {t_dw:.2f} ms "
      f"(field_bwd_train[h3,ext] = {med['field_bwd_train[h3,ext]']:.2f} ms)")
print(f"  table gradient: merged {t_merged:.3f} ms ({added / t_merged / 1e9:.2f} TB/s added), "
      f"plain atomics {t_atomic:.3f} ms ({added / t_atomic / 1e9:.2f} TB/s added); {added / 1e6:.0f} MB of corner adds; "
      f"in the step: {med['hashgrid_bwd_table']:.3f} ms")
print(f"  torch Adam step over the table ({grid.table.numel()} floats): {t_adam:.3f} ms")
print("  per-launch medians:", {k: round(v, 3) for k, v in sorted(med.items())})
