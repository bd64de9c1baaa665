"""ms per image of the shipped default mode (`train_on_batch`, bench.refinement_loop mode "2"), eager and as a replayed graph.
python tools/time_mode2.py [--per-pixel]     --per-pixel: PoseRefiner(per_pixel=True), the reference's `--per_pixel` feature loss"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
if "--per-pixel" in sys.argv[1:]:
    import functools
    from nefes_amd import refine as R
    R.PoseRefiner.__init__ = functools.partialmethod(R.PoseRefiner.__init__, per_pixel=True)
dev = torch.device("cuda", 0); torch.cuda.set_device(0)
for graph in (False, True):
    sec, rays, err = bench.refinement_loop(dev, graph=graph, mode="2")
    print("mode 2", "per-pixel" if "--per-pixel" in sys.argv[1:] else "per-channel", "graph" if graph else "eager", round(sec * 1e3, 2), "ms per image", err)
