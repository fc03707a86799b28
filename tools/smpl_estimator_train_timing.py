"""Measurement: SmplEstimator's training on the device - per block each new kernel entry of csrc/conv_train.hip (batch statistics,
apply, the block backward, the weight gradient with the bias gradient, the input gradient), forward + backward of
ops.conv3x3_bn_block, and the module's training forward + backward, at N = 16 and N = 100 images of 3 x 128 x 128.  Every figure is
a CALL time: the median of per-call device-event times after warm-up calls, with the spread (min .. max) of the same calls - one
event pair around one call on preallocated tensors (the entries) or around forward + backward (the op, the module), so it holds the
launches and the host's enqueue beside the kernels.  The weight gradient's FLOP are 2 Co Ci 9 N H W; its time is set against the
fp32 matrix peak of 157.3 TFLOP/s.

Yardstick: the same module's torch branch with autograd (eager torch ops, training mode: what the module ran before the device
path existed) on the same GPU in the same run, in a child process with its own time limit (the first call of a convolution in a
vendor library may search for an algorithm); reported as a ratio, or as not measured.

    python tools/smpl_estimator_train_timing.py [--out FILE] [--batches 16 100] [--reps 15] [--yardstick-seconds 150]

Quoted in DESIGN.md section 8i; a run is kept in profiles/smpl_estimator_train_timing.txt."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from smpl_nerf_amd import _lib, estimator, ops

PEAK_TFLOPS = 157.3
CHANNELS, POOL = estimator.CHANNELS, estimator.POOL


def timed(fn, reps, warmup=3):
    """(median, min, max) ms over `reps` calls, one device-event pair per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), min(ms), max(ms)


def model_on(dev, seed=1):
    torch.manual_seed(seed)
    return estimator.SmplEstimator(69).to(dev).train()


def step(m, forward, x, dout):
    """forward + backward of the module through `forward`, the gradients dropped afterwards"""
    for p in m.parameters():
        p.grad = None
    forward(x).backward(dout)


def eager_child(batches, reps):
    """The torch branch of the module in training mode with autograd: one JSON line per batch size."""
    dev = torch.device("cuda:0")
    m = model_on(dev)
    out = {}
    for N in batches:
        x, dout = torch.rand(N, 3, 128, 128, device=dev), torch.randn(N, 69, device=dev)
        out[str(N)] = timed(lambda: step(m, m._forward_torch, x, dout), reps)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 100])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--yardstick-seconds", type=float, default=150.0)
    ap.add_argument("--eager-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 15:
        raise SystemExit("smpl_estimator_train_timing: at least 15 timed calls per figure")
    if not torch.cuda.is_available():
        raise SystemExit("smpl_estimator_train_timing: needs the GPU (a CPU timing says nothing about it)")
    if a.eager_child:
        return eager_child(a.batches, a.reps)
    dev = torch.device("cuda:0")
    m, lib = model_on(dev), _lib.load()
    fmt = lambda t: f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"      # noqa: E731
    lines = [f"SmplEstimator training, {torch.cuda.get_device_name(0)}; CALL times in ms (launches and host enqueue included): the median of "
             f"{a.reps} device-event-timed calls (min .. max) after 3 warm-up calls.  Peak: {PEAK_TFLOPS} TFLOP/s fp32 matrix."]
    whole = {}
    for N in a.batches:
        x = torch.rand(N, 3, 128, 128, device=dev)
        dout = torch.randn(N, 69, device=dev)
        lines.append(f"N = {N}")
        h, side = x, 128
        s = torch.cuda.current_stream().cuda_stream
        for i, (conv, bn) in enumerate(m._blocks()):
            ci, co, pool = CHANNELS[i], CHANNELS[i + 1], int(POOL[i])
            out_side = side // 2 if pool else side
            new = lambda *shape: torch.empty(shape, device=dev)      # noqa: E731
            z, y, dz, dx = new(N, co, side, side), new(N, co, out_side, out_side), new(N, co, side, side), new(N, ci, side, side)
            mean, invstd, dg, db, dbias, dw = new(co), new(co), new(co), new(co), new(co), torch.empty_like(conv.weight)
            dy = torch.randn(N, co, out_side, out_side, device=dev)
            ones = torch.ones(co, device=dev)
            w, b, g, bt = (t.detach() for t in (conv.weight, conv.bias, bn.weight, bn.bias))
            rm, rv = bn.running_mean.clone(), bn.running_var.clone()
            sc = [new(max(int(q), 2)) for q in (lib.snerf_bn_stats_scratch_floats(N, co, side, side),
                                               lib.snerf_bn_relu_pool_bwd_scratch_floats(N, co, side, side, pool),
                                               lib.snerf_conv3x3_bwd_weight_scratch_floats(N, ci, side, side, co),
                                               lib.snerf_conv3x3_bwd_input_scratch_floats(ci, co))]
            P = lambda t: t.data_ptr()      # noqa: E731
            assert lib.snerf_conv3x3_block_f32(P(h), N, ci, side, side, P(w), P(ones), P(b), co, 0, 0, P(z), s) == 0
            entries = [
                ("raw map (forward kernel)", lambda: lib.snerf_conv3x3_block_f32(P(h), N, ci, side, side, P(w), P(ones), P(b), co, 0, 0, P(z), s)),
                ("batch statistics", lambda: lib.snerf_bn_stats_f32(P(z), N, co, side, side, bn.eps, 0.1, P(rm), P(rv), P(mean), P(invstd), P(sc[0]), s)),
                ("apply", lambda: lib.snerf_bn_relu_pool_fwd_f32(P(z), N, co, side, side, P(mean), P(invstd), P(g), P(bt), 1, pool, P(y), s)),
                ("block backward", lambda: lib.snerf_bn_relu_pool_bwd_f32(P(z), P(dy), N, co, side, side, P(mean), P(invstd), P(g), P(bt), 1, pool,
                                                                         P(dz), P(dg), P(db), P(sc[1]), s)),
                ("weight + bias gradient", lambda: lib.snerf_conv3x3_bwd_weight_f32(P(dz), P(h), N, ci, co, side, side, P(dw), P(dbias), P(sc[2]), s)),
                ("input gradient", lambda: lib.snerf_conv3x3_bwd_input_f32(P(dz), N, co, side, side, P(w), ci, P(dx), P(sc[3]), s)),
            ]
            lines.append(f"  block {i + 1}  {ci:3d} -> {co:3d}, {side:3d} x {side:3d}{', pool' if pool else ''}")
            for name, fn in entries:
                assert fn() == 0, lib.snerf_last_error_string()
                t = timed(fn, a.reps)
                extra = ""
                if name.startswith("weight"):
                    flop = 2.0 * N * co * ci * 9 * side * side
                    extra = (f"   {flop / 1e9:8.3f} GFLOP = {flop / t[0] / 1e9:7.2f} TFLOP/s = {flop / t[0] / 1e9 / PEAK_TFLOPS:.3f} of the matrix peak "
                             f"({lib.snerf_conv3x3_bwd_weight_slices(N, ci, side, side, co)} slices)")
                lines.append(f"    {name:26s} {fmt(t)}{extra}")
            xin = h.detach().clone().requires_grad_(i > 0)      # block 1's images never require grad

            def op_step():
                for t_ in (conv.weight, conv.bias, bn.weight, bn.bias, xin):
                    t_.grad = None
                ops.conv3x3_bn_block(xin, conv.weight, conv.bias, bn.weight, bn.bias, rm, rv, momentum=0.1, eps=bn.eps, relu=True,
                                     pool=bool(pool)).backward(dy)
            lines.append(f"    {'op, forward + backward':26s} {fmt(timed(op_step, a.reps))}")
            h = y
            side = out_side
        t = timed(lambda: step(m, m, x, dout), a.reps)
        whole[N] = t
        lines.append(f"  module, training forward + backward (device path)   {fmt(t)}")
    # the yardstick, in a process of its own under its own time limit
    cmd = [sys.executable, os.path.abspath(__file__), "--eager-child", "--reps", str(a.reps), "--batches"] + [str(n) for n in a.batches]
    text, note = "", ""
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=a.yardstick_seconds).stdout
    except subprocess.TimeoutExpired as e:
        text = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        note = f" (stopped at its time limit of {a.yardstick_seconds:.0f} s)"
    rows = [ln for ln in text.splitlines() if ln.startswith("{")]
    eager = json.loads(rows[-1]) if rows else {}
    lines.append(f"yardstick: the module's torch branch with autograd (eager torch ops, training mode) on the same GPU{note}")
    for N in a.batches:
        if str(N) in eager:
            t = eager[str(N)]
            lines.append(f"  N = {N:3d}   {fmt(t)}   = {t[0] / whole[N][0]:.2f} x the device path")
        else:
            lines.append(f"  N = {N:3d}   not measured")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
