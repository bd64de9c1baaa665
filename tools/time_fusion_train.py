#!/usr/bin/env python3
"""FusionNet forward + backward with TRAINABLE weights at the reference's stage-3 patch shape [28, 3 + 128, 16, 16] (batch_size 4 x 7
patches: script/models/options.py:80, script/run_nefes.py:86-87): the switch off (torch / MIOpen) against ops.FUSION_TRAIN on (the
library's kernels), A/B/A/B in one process, each window after a warm-up and a device synchronise, timed by device events.  Also: the
per-launch times of the four conv2d_wgrad calls, each side's distance from float64 (d x, the convolution weights' gradients; float64 on
the CPU, evaluated on that side's own ReLU pattern) and whether each side's gradients are bit-stable over ten calls.

    python tools/time_fusion_train.py [out.md]          prints a markdown table (and writes it to out.md)
"""
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nefes_amd import ops  # noqa: E402
from nefes_amd.field import FusionNet  # noqa: E402

B, C, H, W = 28, 128, 16, 16
WARM, ITERS, ROUNDS = 10, 100, 2


def main():
    dev = "cuda"
    torch.manual_seed(0)
    net = FusionNet(C).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x0 = torch.cat([torch.rand(B, 3, H, W, generator=g), torch.randn(B, C, H, W, generator=g)], 1)
    G = torch.randn(B, C, H, W, generator=g)
    xd, Gd = x0.to(dev), G.to(dev)
    names = [n for n, _ in net.named_parameters()]

    def step(on, relu_out=None):
        """One forward + backward; -> (d x, {name: gradient}).  relu_out: list that receives the three ReLU outputs."""
        ops.FUSION_TRAIN = on
        net.zero_grad(set_to_none=True)
        x = xd.clone().requires_grad_()
        hooks = []
        if relu_out is not None and not on:
            hooks = [net.net[i].register_forward_hook(lambda m, a, out: relu_out.append(out.detach())) for i in (1, 3, 5)]
        if relu_out is not None and on:
            ops.TAP = {}
        y = net.forward_prepared(x)
        if relu_out is not None and on:
            relu_out.extend(ops.TAP["conv_relu"][-3:])
            ops.TAP = None
        for h in hooks:
            h.remove()
        (y * Gd).sum().backward()
        return x.grad, {n: p.grad for n, p in net.named_parameters()}

    def window(on):
        for _ in range(WARM):
            step(on)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(ITERS):
            step(on)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / ITERS

    times = {False: [], True: []}
    for _ in range(ROUNDS):
        for on in (False, True):
            times[on].append(window(on))

    # per-launch times of the library's side (events around every C-ABI launch: a run of its own, not the timed windows)
    ops.TIMERS = {}
    step(True)
    torch.cuda.synchronize()
    launches = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ops.TIMERS.items()}
    ops.TIMERS = None

    # bit stability over ten calls
    stable = {}
    for on in (False, True):
        ref = step(on)
        same = True
        for _ in range(9):
            gx, gp = step(on)
            same = same and torch.equal(gx, ref[0]) and all(torch.equal(gp[n], ref[1][n]) for n in names)
        stable[on] = same

    # distance from float64 (CPU), each side on its own ReLU pattern
    net64 = copy.deepcopy(net).cpu().double()
    rel = lambda a, t: float((a.detach().cpu().double() - t).abs().max() / t.abs().max())
    err = {}
    for on in (False, True):
        relu = []
        gx, gp = step(on, relu)
        pos = [(r > 0).cpu().double() for r in relu]
        hooks = [net64.net[i].register_forward_hook(lambda m, a, out, p=p: a[0] * p) for i, p in zip((1, 3, 5), pos)]
        net64.zero_grad()
        x64 = x0.double().requires_grad_()
        (net64.forward_prepared(x64) * G.double()).sum().backward()
        for h in hooks:
            h.remove()
        p64 = dict(net64.named_parameters())
        err[on] = {"d x": rel(gx, x64.grad)}
        err[on].update({n: rel(gp[n], p64[n].grad) for n in names if n.endswith("weight") and not n.startswith("net.7")})
    ops.FUSION_TRAIN = False

    side = {False: "switch off (torch / MIOpen)", True: "switch on (library kernels)"}
    out = [f"FusionNet forward + backward, all parameters trainable, x = [{B}, {3 + C}, {H}, {W}] fp32, {ITERS} iterations per window "
           f"after {WARM} warm-up iterations, windows alternated off / on / off / on in one process, device events.", "",
           "| side | ms per forward + backward (each window) | gradients bit-stable over 10 calls | d x vs float64 | "
           + " | ".join(f"d {n} vs float64" for n in err[True] if n != "d x") + " |", "|---|---|---|---|" + "---|" * (len(err[True]) - 1)]
    for on in (False, True):
        out.append(f"| {side[on]} | " + " / ".join(f"{t:.3f}" for t in times[on]) + f" | {'yes' if stable[on] else 'NO'} | "
                   + " | ".join(f"{v:.1e}" for v in err[on].values()) + " |")
    out += ["", "Per-launch times of the library's side (one event pair per C-ABI call, in launch order, us):", ""]
    for k, v in launches.items():
        out.append(f"- `{k}`: " + ", ".join(f"{t:.1f}" for t in v))
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
