"""Seeded dump of the MLP backward for an A/B of two trees: every weight-gradient kernel and edge once, outputs as .npy.

    python tools/ab/dump_bwd.py OUTDIR            # run under each tree: writes OUTDIR/<case>.<flat_grad|dy|d_x|d_dirs>.npy
    python tools/ab/dump_bwd.py --compare A B     # numpy.array_equal file by file; exit status 1 on any difference

Calls snerf_mlp_bwd_f32 / snerf_mlp_bwd_inputs_f32 and their _bf16_ twins through _lib on zero-filled buffers (the kernels
leave padding unwritten), so with the fixed summation order of the partial / reduce scheme two builds of the same arithmetic
give the same bits.  Cases: the default 8x256 net at n = 70 (one ragged stage past a 32-sample boundary) and n = 2101 (several
chunks, the last ragged, no multiple of 16) in fp32 / bf16x6 / bf16x3 / f16x3 with and without input gradients; width 512
(wide jobs in more than one output-tile group); width 64 (every pair narrow); width 64 with 4000 additional-input columns
(141 narrow jobs: more than the host's job table holds, so the kernel finds its job itself); the warp net's two-layer plan
with a 7-k-block input layer (partial 4x4 blocks) through WarpFieldNet's autograd.  Directions are per ray; d_dirs is [n, 3]
all the same, as in nets._FusedMlpFn.backward (the kernel writes a row per sample).  The tool uses nets' private
_launch_forward / _train_sizes so that the same file runs under an older tree.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    bad = 0 if names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")) else 1
    if bad:
        print("BAD  the two directories do not hold the same files")
    for f in names:
        if not os.path.exists(os.path.join(b, f)):
            continue
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        ok = x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        if ".dy." not in f:      # (an f16x3 step keeps integer statistics behind the rows of dy: not floats)
            ok = ok and bool(np.isfinite(x).all())
        bad += not ok
        print(("ok   " if ok else "BAD  ") + f"{f}: {x.size} values, max |finite value| {float(np.abs(x[np.isfinite(x)]).max(initial=0.0)):.3e}")
    print("bad:", bad)
    return 1 if bad else 0


def dump(out):
    import torch
    from smpl_nerf_amd import _lib
    from smpl_nerf_amd._lib import check, current_stream, ptr
    from smpl_nerf_amd.nets import RenderRayNet, WarpFieldNet, _launch_forward, _train_sizes
    from smpl_nerf_amd.ops import PositionalEncoder

    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    pe, de = PositionalEncoder(10, False), PositionalEncoder(4, False)

    def save(case, **arrays):
        for k, v in arrays.items():
            np.save(os.path.join(out, f"{case}.{k}.npy"), v.detach().float().cpu().numpy())
        print("wrote", case, flush=True)

    def one(case, net, prec, n, spr, input_grad):
        net.precision = prec
        ns = {"fp32": 0, "bf16x6": 3, "bf16x3": 2, "f16x3": _lib.SPLIT_F16X3}[prec]
        desc = net.desc_for_encoders(pe, de)
        g = torch.Generator(device="cpu").manual_seed(1234 + n)
        x = (torch.randn(n, 3, generator=g) * 0.7).to(dev)
        d = (torch.randn(n // spr, 3, generator=g) + torch.tensor([0.0, 0.0, -1.0])).to(dev)
        add = torch.randn(n // spr, net.additional_input_dim, generator=g).to(dev) if net.additional_input_dim else None
        d_raw = torch.randn(n, 4, generator=g).to(dev)
        sizes = _train_sizes(desc, n)
        raw = torch.empty((n, 4), device=dev)
        act = torch.zeros(sizes[0], device=dev)
        net._begin_training_forward()
        _launch_forward(net, desc, ns, x, d, 0, spr, add, raw, act)
        packed_t = net.packed_weights_t_bf16(desc, ns, input_grad) if ns else net.packed_weights_t(desc, input_grad)
        dy, gpart = torch.zeros(sizes[1], device=dev), torch.zeros(sizes[2], device=dev)
        flat = torch.zeros(lib.snerf_mlp_param_floats(desc), device=dev)
        d_x, d_d = torch.zeros(n, 3, device=dev), torch.zeros(n, 3, device=dev)
        s = current_stream()
        if input_grad and ns:
            check(lib.snerf_mlp_bwd_inputs_bf16_f32(desc, ptr(packed_t), ns, ptr(act), ptr(d_raw), ptr(x), ptr(d), 0, spr, n, ptr(dy),
                                                    ptr(gpart), ptr(flat), ptr(d_x), ptr(d_d), s), "snerf_mlp_bwd_inputs_bf16_f32")
        elif input_grad:
            check(lib.snerf_mlp_bwd_inputs_f32(desc, ptr(packed_t), ptr(act), ptr(d_raw), ptr(x), ptr(d), 0, spr, n, ptr(dy),
                                               ptr(gpart), ptr(flat), ptr(d_x), ptr(d_d), s), "snerf_mlp_bwd_inputs_f32")
        elif ns:
            check(lib.snerf_mlp_bwd_bf16_f32(desc, ptr(packed_t), ns, ptr(act), ptr(d_raw), n, ptr(dy), ptr(gpart), ptr(flat), s),
                  "snerf_mlp_bwd_bf16_f32")
        else:
            check(lib.snerf_mlp_bwd_f32(desc, ptr(packed_t), ptr(act), ptr(d_raw), n, ptr(dy), ptr(gpart), ptr(flat), s),
                  "snerf_mlp_bwd_f32")
        torch.cuda.synchronize()
        save(case, flat_grad=flat, dy=dy, d_x=d_x, d_dirs=d_d)

    torch.manual_seed(7)
    net = RenderRayNet(8, 256, 60, 24, skips=[4]).to(dev).train()
    for prec in ("fp32", "bf16x6", "bf16x3", "f16x3"):
        for n, spr in ((70, 7), (2101, 11)):
            for ig in (False, True):
                one(f"w256_{prec}_n{n}_{'inputs' if ig else 'plain'}", net, prec, n, spr, ig)
    one("w512_fp32_n70_plain", RenderRayNet(8, 512, 60, 24, skips=[4]).to(dev).train(), "fp32", 70, 7, False)
    one("w64_fp32_n70_plain", RenderRayNet(8, 64, 60, 24, skips=[4]).to(dev).train(), "fp32", 70, 7, False)
    one("w64_add4000_fp32_n70_plain", RenderRayNet(8, 64, 60, 24, additional_input_dim=4000, skips=[4]).to(dev).train(), "fp32",
        70, 7, False)
    # the warp net: linear1 (100 inputs = 7 k-blocks) -> relu -> linear2
    mw = WarpFieldNet(8, 256, 60, 40).to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(99)
    for n in (70, 2101):
        xi = torch.randn(n, 100, generator=g).to(dev).requires_grad_(True)
        w = torch.randn(n, 3, generator=g).to(dev)
        for p in mw.parameters():
            p.grad = None
        (mw(xi) * w).sum().backward()
        torch.cuda.synchronize()
        save(f"warp256_n{n}", flat_grad=torch.cat([p.grad.reshape(-1) for p in mw.parameters()]), dy=xi.grad,
             d_x=torch.zeros(1), d_dirs=torch.zeros(1))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
