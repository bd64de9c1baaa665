#!/usr/bin/env python3
"""Times of one train step of the field on the generic kernels (csrc/field_generic.hip TRAIN instances, train.field_train_generic):
HIP-event times of the train-mode forward, the fused backward launch, the weight-gradient launches (nefes_train_dw_bias + their
reduction) and the device re-pack, 4096 rays x 192 samples, fine network (full head, C = 16), at (64, 6), (192, 8), (512, 8); and at
(256, 8) next to the tuned fp16 train step of the same build (comparison mode).  Medians of --reps after --warmup; one JSON line
per shape, then a markdown table.  Next to the store times the bytes the two train buffers take per step, and the time those bytes
would take at --write-gbs (full 128-byte lines write 5.2-6.0 TB/s here), so that the cost of the LDS -> HBM copies can be read off against the
inference instances of the same kernels (tools/time_generic_field.py measures those).

--ext: the same step behind a hash grid (train.field_train_generic_encoded, the train-mode instances on a supplied encoding): grid
encode + train-mode forward, and the whole backward (fused launch, weight gradients, table gradient) with a trainable table, at
(128, 8, C = 128) and at (256, 8, C = 16) next to the tuned FieldTrainEncoded step of the same build; the field's own launches are
timed on a given encoding as well.

Usage:  python tools/time_generic_train.py [--ext] [--rays 4096] [--samples 192] [--reps 7] [--warmup 2] [--write-gbs 5200] [--md FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import lib as L, ops                      # noqa: E402
from nefes_amd import train as TR                        # noqa: E402
from nefes_amd.field import NeRFH_NFF                    # noqa: E402


def median_ms(fn, reps, warmup, sync_before=None):
    out = []
    for i in range(warmup + reps):
        if sync_before is not None:
            sync_before()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(t0.elapsed_time(t1))
    return statistics.median(out)


def main_ext(a):
    dev = "cuda:0"
    ops.GENERIC_TRAIN_EXT = True
    lib = L.load()
    N, S = a.rays, a.samples
    gen = torch.Generator().manual_seed(1)
    o = ((torch.rand(N, 3, generator=gen) - .5) * 10).to(dev)                # inside bound 25 with depths up to 12
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
    z = torch.sort(torch.rand(N, S, generator=gen) * 12, -1)[0].to(dev)
    grid = ops.HashGrid(25.0, table=(torch.rand(ops.HashGrid(25.0).table.shape, generator=gen) * 2 - 1) * 0.3)
    grid.table.requires_grad_(True)
    ghz, tf = C.c_double(), C.c_double()
    L.check(lib.nefes_probe_mfma_clock(1, 40, C.byref(ghz), C.byref(tf), None), "nefes_probe_mfma_clock")
    rows = []
    for (W, D, Cf, compare) in [(128, 8, 128, False), (256, 8, 16, True)]:
        net = NeRFH_NFF('fine', D=D, W=W, f_dim=Cf, in_channels_xyz=32, encode_appearance=True, encode_transient=True).to(dev)
        sd = dict(net.named_parameters())
        for kind in (("generic", "tuned") if compare else ("generic",)):
            step = TR.field_train_generic_encoded if kind == "generic" else TR.field_train_encoded
            Fn = TR.FieldTrainGenericEncoded if kind == "generic" else TR.FieldTrainEncoded
            names = TR.param_names_generic(net, L.FIELD_FULL) if kind == "generic" else TR.param_names(net, L.FIELD_FULL)
            pk = net.packed_generic() if kind == "generic" else net.packed()
            state = {}

            def fwd():
                state["raw"] = step(net, L.FIELD_FULL, grid, o, d, d, z)

            fwd()
            g = torch.randn_like(state["raw"])
            rec = {"W": W, "D": D, "C": Cf, "kernels": kind, "rays": N, "samples": S}
            rec["fwd_ms"] = median_ms(fwd, a.reps, a.warmup)                 # grid encode + train-mode forward
            rec["bwd_ms"] = median_ms(lambda: state["raw"].backward(g), a.reps, a.warmup, sync_before=fwd)      # ... + dW + table gradient
            state.clear()
            with torch.no_grad():
                enc = grid((o[:, None, :] + d[:, None, :] * z[..., None])).detach()
            enc.requires_grad_(True)

            def field_fwd():
                state["raw"] = Fn.apply(enc, d, net, L.FIELD_FULL, *[sd[n] for n in names])

            rec["field_fwd_ms"] = median_ms(field_fwd, a.reps, a.warmup)
            rec["field_bwd_ms"] = median_ms(lambda: state["raw"].backward(g), a.reps, a.warmup, sync_before=field_fwd)
            if kind == "generic":
                field_fwd()
                raw_t, acts, vv, masks = state["raw"].grad_fn.saved_tensors
                dacts = torch.empty_like(acts)
                g_enc, g_vs = torch.empty(N * S, 32, device=dev), torch.empty(N * S, 3, device=dev)
                rec["bwd_kernel_ms"] = median_ms(lambda: L.check(lib.nefes_field_bwd_train_generic_ext(
                    pk.desc, pk.blob.data_ptr(), L.FIELD_FULL, N, S, vv.data_ptr(), raw_t.data_ptr(), g.data_ptr(), masks.data_ptr(),
                    dacts.data_ptr(), g_enc.data_ptr(), g_vs.data_ptr(), ops._stream()), "bwd"), a.reps, a.warmup)
                rec["dw_ms"] = rec["field_bwd_ms"] - rec["bwd_kernel_ms"]
                rec["buffer_gb_each"] = TR.generic_train_bytes(pk, N * S) / 2 / 1e9
                del dacts, g_enc, g_vs
            rec["grid_fwd_ms"] = rec["fwd_ms"] - rec["field_fwd_ms"]
            rec["grid_bwd_ms"] = rec["bwd_ms"] - rec["field_bwd_ms"]          # table gradient + d positions
            rec["step_ms"] = rec["fwd_ms"] + rec["bwd_ms"]
            state.clear()
            for p_ in list(sd.values()) + [grid.table]:
                p_.grad = None
            rec = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            del enc
            torch.cuda.empty_cache()
    cols = ["W", "D", "C", "kernels", "step_ms", "fwd_ms", "bwd_ms", "field_fwd_ms", "field_bwd_ms", "bwd_kernel_ms", "dw_ms", "grid_fwd_ms",
            "grid_bwd_ms", "buffer_gb_each"]
    by = {(r["W"], r["kernels"]): r for r in rows}
    ratio = by[(256, "generic")]["step_ms"] / by[(256, "tuned")]["step_ms"]
    md = [f"sustained clock {ghz.value:.3f} GHz (nefes_probe_mfma_clock, dense 16-bit MFMA {tf.value:.0f} TFLOP/s); {N} rays x {S} samples; "
          f"medians of {a.reps} after {a.warmup} warm-up; (256, 8) generic step / tuned step = {ratio:.2f}", "",
          "| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    md += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    return md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ext", action="store_true")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--write-gbs", type=float, default=5200.)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    md = main_ext(a) if a.ext else main_freq(a)
    print("\n".join(md))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("\n".join(md) + "\n")


def main_freq(a):
    dev = "cuda:0"
    ops.GENERIC_TRAIN = True
    lib = L.load()
    N, S = a.rays, a.samples
    gen = torch.Generator().manual_seed(1)
    o = (torch.rand(N, 3, generator=gen) - .5).to(dev)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
    z = torch.sort(torch.rand(N, S, generator=gen) * 4, -1)[0].to(dev)
    ghz, tf = C.c_double(), C.c_double()
    L.check(lib.nefes_probe_mfma_clock(1, 40, C.byref(ghz), C.byref(tf), None), "nefes_probe_mfma_clock")
    rows = []
    for (W, D, compare) in [(64, 6, False), (192, 8, False), (512, 8, False), (256, 8, True)]:
        net = NeRFH_NFF('fine', D=D, W=W, f_dim=16, encode_appearance=True, encode_transient=True).to(dev)
        prm = [p for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]
        for kind in (("generic", "tuned") if compare else ("generic",)):
            ops.FIELD_GENERIC = compare and kind == "generic"
            field = TR.field_train_generic if kind == "generic" else TR.field_train
            pk = net.packed_generic() if kind == "generic" else net.packed()
            state = {}

            def fwd():
                state["raw"] = field(net, L.FIELD_FULL, o, d, d, z)

            fwd()
            g = torch.randn_like(state["raw"])
            rec = {"W": W, "D": D, "kernels": kind, "rays": N, "samples": S}
            rec["fwd_ms"] = median_ms(fwd, a.reps, a.warmup)
            # the whole backward (fused dX launch + weight-gradient launches + reduction), on a graph made outside the timed region
            rec["bwd_ms"] = median_ms(lambda: state["raw"].backward(g), a.reps, a.warmup, sync_before=fwd)
            if kind == "generic":
                # the fused backward launch alone, on buffers of its own
                fwd()                                                        # (the timed backward freed the last graph)
                fn = state["raw"].grad_fn
                raw_t, acts, oo, dd, vv, zz, masks = fn.saved_tensors
                dacts = torch.empty_like(acts)
                g_pts, g_vs = torch.empty(N * S, 3, device=dev), torch.empty(N * S, 3, device=dev)
                rec["bwd_kernel_ms"] = median_ms(lambda: L.check(lib.nefes_field_bwd_train_generic(
                    pk.desc, pk.blob.data_ptr(), L.FIELD_FULL, N, S, oo.data_ptr(), dd.data_ptr(), zz.data_ptr(), vv.data_ptr(), raw_t.data_ptr(),
                    g.data_ptr(), masks.data_ptr(), dacts.data_ptr(), g_pts.data_ptr(), g_vs.data_ptr(), ops._stream()), "bwd"), a.reps, a.warmup)
                rec["dw_ms"] = rec["bwd_ms"] - rec["bwd_kernel_ms"]          # nefes_train_dw_bias launches + the reduction of their shares
                del dacts, g_pts, g_vs
                # the inference instances on the same input: what the train-mode stores add
                pk_f = pk
                rec["fwd_infer_ms"] = median_ms(lambda: ops.field_fwd_generic(pk_f, L.FIELD_FULL, N, S, rays_o=o, rays_d=d, z=z, viewdirs=d,
                                                                              want_masks=True), a.reps, a.warmup)
                raw_i, masks_i = ops.field_fwd_generic(pk_f, L.FIELD_FULL, N, S, rays_o=o, rays_d=d, z=z, viewdirs=d, want_masks=True)
                rec["bwd_infer_ms"] = median_ms(lambda: ops.field_bwd_generic(pk_f, L.FIELD_FULL, N, S, raw_i, g, masks_i, rays_o=o, rays_d=d,
                                                                              z=z, viewdirs=d), a.reps, a.warmup)
                buf = TR.generic_train_bytes(pk, N * S) / 2
                rec["buffer_gb_each"] = buf / 1e9
                rec["store_ms_at_write_rate"] = buf / (a.write_gbs * 1e9) * 1e3
                rec["fwd_store_cost_ms"] = rec["fwd_ms"] - rec["fwd_infer_ms"]
                rec["bwd_store_cost_ms"] = rec["bwd_kernel_ms"] - rec["bwd_infer_ms"]
                del raw_i, masks_i

            def repack():
                with torch.no_grad():
                    prm[0].add_(0.)
                (net.packed_generic() if kind == "generic" else net.packed())

            state.clear()
            rec["repack_ms"] = median_ms(repack, a.reps, a.warmup)
            rec = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            torch.cuda.empty_cache()
        ops.FIELD_GENERIC = False
    cols = ["W", "D", "kernels", "fwd_ms", "bwd_ms", "bwd_kernel_ms", "dw_ms", "repack_ms", "fwd_infer_ms", "bwd_infer_ms",
            "fwd_store_cost_ms", "bwd_store_cost_ms", "buffer_gb_each", "store_ms_at_write_rate"]
    md = [f"sustained clock {ghz.value:.3f} GHz (nefes_probe_mfma_clock, dense 16-bit MFMA {tf.value:.0f} TFLOP/s); {N} rays x {S} samples; "
          f"medians of {a.reps} after {a.warmup} warm-up; write rate assumed {a.write_gbs:.0f} GB/s", "",
          "| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    md += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    return md


if __name__ == "__main__":
    main()
