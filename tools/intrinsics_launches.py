"""GPU launches of ONE refinement iteration (mode 3, the tests/golden/refine.npz scene) without a camera, with PoseRefiner(intrinsics=)
and with learn_focal=True: the count eager and as one replay of the captured graph, and the names of the launches the camera adds
(listed the way tools/mode2_sequence.py lists mode 2's)."""
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch.profiler import profile, ProfilerActivity

from tests.test_gpu_intrinsics import job, refiner, rendered_centred

g = dict(np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "refine.npz")))


def launches(fn):
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return collections.Counter(e.name[:90] for e in ev)


base = None
for title, more in (("no camera (focal kernels)", {}), ("intrinsics=", dict(intrinsics=rendered_centred(g).to("cuda"))),
                    ("learn_focal=True", dict(learn_focal=True))):
    r = refiner(g, True, **more)
    r.refine(*job(g), 2)
    eager, replay = launches(r._iteration), launches(r.replay)
    print(f"---- {title}: {sum(eager.values())} launches eager, {sum(replay.values())} in one replay of the captured iteration")
    if base is None:
        base = eager
    else:
        for name in sorted(set(eager) | set(base)):
            if eager[name] != base[name]:
                print(f"    {eager[name] - base[name]:+d}  {name}")
