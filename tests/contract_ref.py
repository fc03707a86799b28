"""CPU restatement of the input-gradient contraction (csrc/contract.hip, snerf_dy_contract_f32), used ONLY by tests.

    out[s, c] = sum_f dY[s, f] w[f, col0 + c]          (include/smplnerf.h:315-324; summed over each ray's `spr` consecutive rows when spr > 0)

  * pack_tile_rows(): dense dY [n, n_feat] -> the tile-row-major buffer the dgrad kernels leave behind (include/smplnerf.h:311-312);
  * contract64():     the definition in float64 (the truth);
  * contract32():     the same in fp32 in the order the kernel documents - products added over f in ascending order, then the rows
                      of a ray in ascending order - as a plain numpy loop (no BLAS, no pairwise sum: what fp32 can be asked for);
  * relative_error(): E(y) = max|y - y64| / max|y64|, the measure of tests/vertex_warp_ref.py.
Also here: the cases of tests/test_gpu_contract.py and their inputs, so that tests/test_contract_host.py can check on the CPU what
the GPU tests take for granted (the integer cases are exact in fp32 in any order, the real-valued ones have a yardstick above 0).
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
PAD_VALUE = 1000.0            # finite: the kernel multiplies the pad features of the last tile-row by zero weights
GUARD = float("nan")          # tile-rows / weight columns / weight rows that do not belong to the call
INT_LIMIT = 2 ** 24           # integers below it are exact in fp32


# ------------------------------------------------------------------------------------------------ the op
def tile_rows(n_feat):
    return (n_feat + 15) // 16


def pack_tile_rows(dense, first_row, total_rows, n, pad_value, guard_value):
    """dense [n, n_feat] -> fp32 [total_rows, n, 16] with dY[s, f] at [first_row + f // 16, s, f % 16]; the features
    f >= n_feat of the layer's last tile-row hold pad_value, every other tile-row guard_value."""
    dense = np.asarray(dense)
    n_feat = dense.shape[1]
    rows = tile_rows(n_feat)
    assert dense.shape[0] == n and first_row >= 0 and first_row + rows <= total_rows
    buf = np.full((total_rows, n, 16), guard_value, dtype=F32)
    layer = np.full((n, rows * 16), pad_value, dtype=F32)
    layer[:, :n_feat] = dense
    buf[first_row:first_row + rows] = layer.reshape(n, rows, 16).transpose(1, 0, 2)
    return buf


def _sum_rays(y, spr):
    """rows of a ray added in ascending order, in the dtype of y"""
    if spr <= 0:
        return y
    n, c = y.shape
    assert n % spr == 0
    y = y.reshape(n // spr, spr, c)
    acc = y[:, 0].copy()
    for k in range(1, spr):
        acc += y[:, k]
    return acc


def contract64(dense, w, col0, ncols, spr):
    """float64 [n or n / spr, ncols]; w [>= n_feat, w_stride] - only rows < n_feat and columns col0 .. col0 + ncols - 1 are read."""
    d = np.asarray(dense, np.float64)
    wc = np.asarray(w)[:d.shape[1], col0:col0 + ncols].astype(np.float64)
    return _sum_rays(d @ wc, spr)


def contract32(dense, w, col0, ncols, spr):
    """The same in fp32: every product rounded, added over f in ascending order, then the rows of a ray in ascending order."""
    d = np.asarray(dense, F32)
    wc = np.ascontiguousarray(np.asarray(w)[:d.shape[1], col0:col0 + ncols], dtype=F32)
    acc = np.zeros((d.shape[0], ncols), F32)
    for f in range(d.shape[1]):
        acc += d[:, f:f + 1] * wc[f:f + 1, :]
    assert acc.dtype == F32
    return _sum_rays(acc, spr)


def relative_error(y, y64):
    """E(y) = max|y - y64| / max|y64| (0 when both are all zero)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    scale = np.abs(y64).max() if y64.size else 0.0
    err = np.abs(y - y64).max() if y64.size else 0.0
    return 0.0 if err == 0.0 else err / scale


def scratch_floats(n, ncols, spr):
    """what snerf_dy_contract_scratch_floats documents"""
    return 0 if spr == 0 else (n // 16 if spr % 16 == 0 else n) * ncols


# ------------------------------------------------------------------------------------------------ the cases
# dense: w_stride = ncols and out_stride = ncols (col0 = out_col0 = 0); otherwise both rows are wider than the call's columns and
# the columns outside hold NaN (w) / canaries (out).  n < 0: sized on the device (grid_stride_n).
Case = namedtuple("Case", "name n n_feat ncols spr first_row col0 out_col0 accumulate dense seed")
MODES = [(0, 37), (16, 80), (7, 63)]          # (spr, n): per sample / per ray with 16-sample lane reduction / per ray, a row per sample


def _case(name, n, n_feat, ncols, spr, accumulate, offsets=True, seed=1):
    return Case(name, n, n_feat, ncols, spr, 3 if offsets else 0, 5 if offsets else 0, 2 if offsets else 0, int(accumulate), not offsets, seed)


def instance_cases():
    """every (column tiles, k-blocks) instance in every output mode; accumulate alternates so that both values meet every mode"""
    out = []
    for a, ncols in enumerate((16, 17, 63, 69, 97)):
        for b, n_feat in enumerate((40, 100, 250)):
            for c, (spr, n) in enumerate(MODES):
                out.append(_case(f"inst-c{ncols}-f{n_feat}-spr{spr}", n, n_feat, ncols, spr, (a + b + c) % 2))
    return out


def edge_cases():
    """one axis at a time around (n 48, n_feat 40, ncols 16, per sample); dense strides, no offsets"""
    out = []
    for k, n_feat in enumerate((1, 16, 17, 64, 65, 128, 129, 256)):
        out.append(_case(f"edge-f{n_feat}", 48, n_feat, 16, 0, k % 2, offsets=False))
    for k, ncols in enumerate((1, 32, 33, 64, 65, 96, 128)):
        out.append(_case(f"edge-c{ncols}", 48, 40, ncols, 0, k % 2, offsets=False))
    for k, n in enumerate((1, 15, 16, 17, 63, 64, 65, 130)):
        out.append(_case(f"edge-n{n}", n, 40, 16, 0, k % 2, offsets=False))
    for k, spr in enumerate((1, 3, 16, 64, 192, 100)):
        out.append(_case(f"edge-spr{spr}", 2 * spr, 40, 16, spr, k % 2, offsets=False))
    out.append(_case("edge-one-ray-37", 37, 40, 16, 37, 0, offsets=False))
    out.append(_case("edge-one-ray-48", 48, 40, 16, 48, 1, offsets=False))
    return out


def pass_cases():
    """more than one pass of 128 columns: 128 + 1, 128 + 72, 10 x 128 + 100"""
    return [_case(f"pass-c{ncols}-spr{spr}", n, 256, ncols, spr, (a + c) % 2)
            for a, ncols in enumerate((129, 200, 1380)) for c, (spr, n) in enumerate(MODES)]


def split_cases():
    """257 .. 512 features: two calls, the second accumulating"""
    return [_case(f"split-f{n_feat}-spr{spr}-acc{acc}", n, n_feat, 69, spr, acc)
            for n_feat in (257, 300, 512) for spr, n in MODES for acc in (0, 1)]


# the grid-stride loop: n depends on the device (grid_stride_n); (name, n_feat, ncols, spr)
GRID_STRIDE = [_case("stride-f64-c16", -1, 64, 16, 0, 0), _case("stride-f256-c128", -1, 256, 128, 0, 1),
               _case("stride-f256-c128-spr16", -1, 256, 128, 16, 0)]


def workgroups_per_cu(n_feat, ncols):
    """the launcher's rule (csrc/contract.hip: `per_cu`): two workgroups per CU while the W^T block is at most 72 KiB of LDS"""
    tiles = next(t for t in (1, 2, 4, 6, 8) if t >= (min(128, ncols) + 15) // 16)
    kb = 16 if n_feat > 128 else 8 if n_feat > 64 else 4
    return 2 if tiles * 16 * (kb * 16 + 4) * 4 <= 72 * 1024 else 1


def grid_stride_n(case, n_cu):
    """more sample tiles than two rounds of the capped grid (4 waves per workgroup), ragged so that the sample clamp is met too;
    a multiple of 16 for the lane-reduced per-ray mode"""
    n_tiles = 2 * (4 * workgroups_per_cu(case.n_feat, case.ncols) * n_cu) + 3
    n = 16 * n_tiles - 5
    return n // 16 * 16 if case.spr else n


def integer_cases():
    return instance_cases() + edge_cases() + pass_cases() + split_cases()


# two calls, same bits: each mode, below and through the 256-feature split
REPEAT_CASES = [_case(f"repeat-f{n_feat}-spr{spr}", n, n_feat, 69, spr, 1) for n_feat in (250, 300) for spr, n in MODES]


# real-valued quality: the workload's own layer shapes at small n (n_feat, ncols, spr, rays or samples)
REAL_CASES = [_case("real-f256-c69-spr192", 3 * 192, 256, 69, 192, 0, seed=1), _case("real-f256-c84", 100, 256, 84, 0, 0, seed=2),
              _case("real-f512-c128-spr100", 2 * 100, 512, 128, 100, 0, seed=3), _case("real-f64-c16-spr16", 5 * 16, 64, 16, 16, 0, seed=1),
              _case("real-f250-c200-spr7", 9 * 7, 250, 200, 7, 0, seed=2), _case("real-f256-c1380-spr64", 2 * 64, 256, 1380, 64, 0, seed=3)]


def strides(case):
    """(w_stride, out_stride)"""
    if case.dense:
        return case.ncols, case.ncols
    return case.col0 + case.ncols + 4, case.out_col0 + case.ncols + 3


def out_rows(case, n):
    return n // case.spr if case.spr else n


def integer_inputs(case, n):
    """(dY [n, n_feat], w columns [n_feat, ncols], prior contents of out [rows, ncols]) - integers as fp32: dY, w in -3 .. 3, out in
    -5 .. 5, so that every product and partial sum is an integer of magnitude <= 9 n_feat max(spr, 1) + 5"""
    rng = np.random.default_rng([case.seed, n, case.n_feat, case.ncols, case.spr])
    dense = rng.integers(-3, 4, (n, case.n_feat)).astype(F32)
    wc = rng.integers(-3, 4, (case.n_feat, case.ncols)).astype(F32)
    prior = rng.integers(-5, 6, (out_rows(case, n), case.ncols)).astype(F32)
    return dense, wc, prior


def integer_bound(case):
    return 9 * case.n_feat * max(case.spr, 1) + 5


def real_inputs(case, n):
    """dY ~ N(0, 1), w ~ N(0, 1) / sqrt(n_feat)"""
    rng = np.random.default_rng([case.seed, n, case.n_feat, case.ncols, case.spr])
    dense = rng.normal(size=(n, case.n_feat)).astype(F32)
    wc = (rng.normal(size=(case.n_feat, case.ncols)) / np.sqrt(case.n_feat)).astype(F32)
    return dense, wc


def walked_rows(n_feat):
    """weight rows the kernel's instance walks: k-blocks 4 / 8 / 16 of 16 features, twice for the split above 256"""
    if n_feat > 256:
        return 256 + walked_rows(n_feat - 256)
    return 256 if n_feat > 128 else 128 if n_feat > 64 else 64


def weight_block(case, wc):
    """w [rows, w_stride]: the call's columns at col0, NaN in every other column and in the guard rows after row n_feat - 1 - at
    least one, and as many as the instance's k-blocks walk, so that a kernel that lost its row guard reads NaN inside the buffer"""
    w_stride, _ = strides(case)
    w = np.full((max(case.n_feat + 1, walked_rows(case.n_feat)), w_stride), GUARD, dtype=F32)
    w[:case.n_feat, case.col0:case.col0 + case.ncols] = wc
    return w
