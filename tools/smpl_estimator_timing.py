"""Measurement: SmplEstimator's inference on the device - each fused conv-BN-ReLU-pool block (snerf_conv3x3_block_f32) and the whole
network in one call (estimator.SmplEstimator in eval mode under no_grad = snerf_smpl_estimator_fwd_f32) at N = 1, 16 and 100
images of 3 x 128 x 128.  Every figure is a CALL time: the median of per-call device-event times after warm-up calls, with the
spread (min .. max) of the same calls - one event pair around one call of the C entry on preallocated tensors (the blocks) or of
the module (the whole network), so it holds the launch and the host's enqueue beside the kernel; below about 0.05 ms that fixed
part is most of the figure, and the shares printed there say how far the CALL is from a bound, not the kernel.  FLOP and bytes are
counted from the shapes (2 Co Ci 9 H W per image and block; input, output and weights once), and each time is set against the
fp32 matrix peak of 157.3 TFLOP/s and against 8 TB/s of HBM: the larger of the two least times over the call time.

Yardstick: the same module's torch branch (eager torch ops, eval mode) on the same GPU, in a child process with its own time limit
(the first call of a convolution in a vendor library may search for an algorithm); reported as a ratio, or as not measured.

    python tools/smpl_estimator_timing.py [--out FILE] [--batches 1 16 100] [--reps 15] [--yardstick-seconds 150]

Quoted in DESIGN.md section 8h; a run is kept in profiles/smpl_estimator_timing.txt."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from smpl_nerf_amd import _lib, estimator

PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0
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
    m = estimator.SmplEstimator(69)
    with torch.no_grad():
        for i in range(1, 6):      # running statistics as after training, not the initial 0 and 1
            getattr(m, f"bn{i}").running_mean.uniform_(-0.2, 0.2)
            getattr(m, f"bn{i}").running_var.uniform_(0.5, 2.0)
    return m.to(dev).eval()


def eager_child(batches, reps):
    """The torch branch of the module (what forward() runs with grad enabled), under no_grad for a fair yardstick: one JSON line."""
    dev = torch.device("cuda:0")
    m = model_on(dev)
    out = {}
    with torch.no_grad():
        for N in batches:
            x = torch.rand(N, 3, 128, 128, device=dev)
            out[str(N)] = timed(lambda: m._forward_torch(x), reps)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 100])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--yardstick-seconds", type=float, default=150.0)
    ap.add_argument("--eager-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 15:
        raise SystemExit("smpl_estimator_timing: at least 15 timed calls per figure")
    if not torch.cuda.is_available():
        raise SystemExit("smpl_estimator_timing: needs the GPU (a CPU timing says nothing about it)")
    if a.eager_child:
        return eager_child(a.batches, a.reps)
    dev = torch.device("cuda:0")
    m, lib = model_on(dev), _lib.load()
    fmt = lambda t: f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"      # noqa: E731
    lines = [f"SmplEstimator inference, {torch.cuda.get_device_name(0)}; CALL times in ms (launch and host enqueue included): the median of "
             f"{a.reps} device-event-timed calls (min .. max) after 3 warm-up calls.  Peaks: {PEAK_TFLOPS} TFLOP/s fp32 matrix, {PEAK_TBS} TB/s HBM."]
    whole = {}
    with torch.no_grad():
        for N in a.batches:
            x = torch.rand(N, 3, 128, 128, device=dev)
            lines.append(f"N = {N}")
            h, side, total_ms, total_flop = x, 128, 0.0, 0.0
            for i, (conv, bn) in enumerate(m._blocks()):
                ci, co = CHANNELS[i], CHANNELS[i + 1]
                scale, shift = estimator.fold_bn(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
                inp, out_side = h, side // 2 if POOL[i] else side
                h = torch.empty((N, co, out_side, out_side), device=dev)
                args = (inp.data_ptr(), N, ci, side, side, conv.weight.data_ptr(), scale.data_ptr(), shift.data_ptr(), co, 1, int(POOL[i]),
                        h.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert lib.snerf_conv3x3_block_f32(*args) == 0, lib.snerf_last_error_string()
                t = timed(lambda: lib.snerf_conv3x3_block_f32(*args), a.reps)
                flop = 2.0 * N * co * ci * 9 * side * side
                nbytes = 4.0 * (inp.numel() + h.numel() + conv.weight.numel())
                t_mat, t_mem = flop / (PEAK_TFLOPS * 1e12) * 1e3, nbytes / (PEAK_TBS * 1e12) * 1e3
                lines.append(f"  block {i + 1}  {ci:3d} -> {co:3d}, {side:3d} x {side:3d}{', pool' if POOL[i] else '      '}  K = {9 * ci:3d}   {fmt(t)}   "
                             f"{flop / 1e9:8.3f} GFLOP = {flop / t[0] / 1e9:7.2f} TFLOP/s = {flop / t[0] / 1e9 / PEAK_TFLOPS:.3f} of the matrix peak;   "
                             f"{nbytes / 1e6:8.2f} MB = {nbytes / t[0] / 1e9:.3f} TB/s;   nearer bound: {'matrix' if t_mat >= t_mem else 'memory'}, "
                             f"the call at {max(t_mat, t_mem) / t[0]:.3f} of it")
                total_ms, total_flop = total_ms + t[0], total_flop + flop
                if POOL[i]:
                    side //= 2
            total_flop += 2.0 * N * (8192 * 500 + 500 * 69)
            t = timed(lambda: m(x), a.reps)
            whole[N] = t
            lines.append(f"  whole network, one call                         {fmt(t)}   {total_flop / 1e9:8.3f} GFLOP = {total_flop / t[0] / 1e9:7.2f} TFLOP/s = "
                         f"{total_flop / t[0] / 1e9 / PEAK_TFLOPS:.3f} of the matrix peak   (the five blocks alone, summed: {total_ms:.4f} ms)")
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
    lines.append(f"yardstick: the module's torch branch (eager torch ops, eval mode, no_grad) on the same GPU{note}")
    for N in a.batches:
        if str(N) in eager:
            t = eager[str(N)]
            lines.append(f"  N = {N:3d}   {fmt(t)}   = {t[0] / whole[N][0]:.2f} x the one call")
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
