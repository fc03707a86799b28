"""tools/strict_cost.py's method on two builds of the library: the single-call render of a 128 x 128 frame (64 + 128, fp32) in
alternating rounds parent / branch / parent (a second copy of the parent's library: the spread of the parent against itself),
device events around each turn of 5 calls, medians in ms per call.

    python tools/ab/render_two_libs.py PARENT.so PARENT_COPY.so BRANCH.so [--pairs 20]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from smpl_nerf_amd import _lib
from smpl_nerf_amd import synthetic as syn
from smpl_nerf_amd.nets import RenderRayNet
from smpl_nerf_amd.ops import PositionalEncoder
from smpl_nerf_amd.pipelines import NerfPipeline, PipelineArgs

dev = torch.device("cuda:0")
paths = [os.path.abspath(p) for p in sys.argv[1:4]]
pairs = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 20
handles = []
for p in paths:
    _lib._lib, _lib.LIB_PATH = None, p
    handles.append(_lib.load())
assert len({id(h) for h in handles}) == 3 and len({h._handle for h in handles}) == 3


def net(p):
    m = RenderRayNet(8, 256, 60, 24, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.to(dev)


pc, pf = syn.make_scene_nets(101)
frame = [torch.from_numpy(x).to(dev) for x in syn.frame_batch(128, 128, seed=7)]
pipes = []
for h in handles:                       # a pipeline of its own per library, so that nothing one library packed is read by another
    _lib._lib = h
    pipes.append(NerfPipeline(net(pc), net(pf), PipelineArgs(), PositionalEncoder(10, 0), PositionalEncoder(4, 0)).eval())


def render(k):
    _lib._lib = handles[k]
    with torch.no_grad():
        return pipes[k](frame)


outs = []
for k in range(3):
    for _ in range(3):
        o = render(k)
    outs.append([t.cpu().numpy() for t in o])
torch.cuda.synchronize()
print("parent copy == parent bits:", all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])))
print("branch against parent, max|diff| per output:", [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(outs[0], outs[2])])
res = ([], [], [])
for _ in range(pairs):
    for k in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _lib._lib = handles[k]
        e0.record()
        for _ in range(5):
            render(k)
        e1.record()
        e1.synchronize()
        res[k].append(e0.elapsed_time(e1) / 5)
for name, r in zip(("parent", "parent (copy)", "branch"), res):
    print(f"render 128x128 (64+128, fp32, one call) {name:14s}: median {np.median(r):.4f} ms  min {np.min(r):.4f}  max {np.max(r):.4f}  ({pairs} turns of 5)")
p, p2, b = (float(np.median(r)) for r in res)
print(f"branch / parent {b / p:.4f}   parent (copy) / parent {p2 / p:.4f}")
