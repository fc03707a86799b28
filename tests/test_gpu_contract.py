"""The input-gradient contraction (csrc/contract.hip, snerf_dy_contract_f32) against float64, branch by branch, through the C entry as
nets._contract calls it.

Two kinds of input (tests/contract_ref.py; tests/test_contract_host.py checks their premises on the CPU):
  * integer cases: dY, w in -3 .. 3 and the prior contents of out in -5 .. 5.  Every product and partial sum is an integer below 2^24,
    so the kernel must equal the float64 definition EXACTLY whatever its summation order: a wrong row, column, offset, tile, pass or
    half shows, and there is no tolerance to argue about;
  * real cases: dY ~ N(0, 1), w ~ N(0, 1) / sqrt(n_feat) at the workload's layer shapes, held to E(kernel) <= 8 E(fp32 CPU restatement)
    with E(y) = max|y - y64| / max|y64| - measure and factor of tests/test_gpu_vertex_warp.py; both figures are computed here and
    printed before the assert (pytest -s; profiles/contract_errors.txt holds a run).

Every call runs inside guards of the test's own buffers, so that a stray access shows in the result and never leaves an allocation:
dy has two NaN tile-rows before tile-row 0 of the call (and NaN in the tile-rows before first_row) and two after the layer's last one,
and 1000.0 in the pad features of the last tile-row; w is cut from a NaN buffer with NaN in every column outside the call's and in a
guard row after the last; out has a canary in every column outside the call's and in two guard rows; the scratch is exactly
snerf_dy_contract_scratch_floats() floats of NaN between canaries.

Measured on an MI355X (profiles/contract_errors.txt has every figure): E kernel is 1.6e-7 .. 5.1e-7 over the six real cases against
1.5e-7 .. 5.2e-7 for the fp32 CPU restatement, a ratio of 0.62 .. 1.07.

What the dgrad kernels leave in the pad features of a layer whose width is no multiple of 16 (read from mlp_train.hip,
mlp_train_bf16.hip and warp.hip, nothing was run for it): zeros.  Such a layer runs zero-padded inside the next kernel width
(mlp_plan.h), and every stored d Y tile is one of three things.  (a) A ReLU layer's tile goes through a select on the forward's sign
mask (mask_bits_into / mask_into, `m > 0 ? src : 0`; mask_store in the split-precision kernel ANDs the bits with 0): the pad
activations are relu(0 x + 0) = 0, their mask bit is clear, and the stored value is +0 whatever the accumulator held.  (b) The two
layers without activation (additional_linear_layer, directional_input) store accumulators of zero transposed-weight rows (the packers
write 0 where bwd_slab_src is -1) times the gradient above them, plus a zero sigma-head entry times d sigma: +-0 as long as that
gradient is finite.  (c) The heads store literal zeros beside their 3 + 1 values, as does the warp net's head.  So a pad can be
non-finite only where a real feature of the same sample already is, and the kernel's zero weights against the pads (0 x 0) are
sound; no NaN-pad case is added.  The 1000.0 pads here check that the weights against them are zero."""
import ctypes

import numpy as np
import pytest
import torch

import contract_ref as CR

pytestmark = pytest.mark.gpu
FACTOR = 8.0
CANARY = 12345.0
OK, E_BADARG, E_ALIGN = 0, -1, -2
DY_GUARD_ROWS = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Call:
    """One snerf_dy_contract_f32 call inside its guards: device buffers, pointers, and the checks of what must not have changed."""

    def __init__(self, dev, case, n, dense, wc, prior):
        from smpl_nerf_amd import _lib
        self.lib, self.case, self.n = _lib.load(), case, n
        self.w_stride, self.out_stride = CR.strides(case)
        rows = CR.tile_rows(case.n_feat)
        lead = DY_GUARD_ROWS + case.first_row
        dy = CR.pack_tile_rows(dense, lead, lead + rows + DY_GUARD_ROWS, n, CR.PAD_VALUE, CR.GUARD)
        self.dy_all = torch.from_numpy(dy).to(dev)
        self.dy = self.dy_all[DY_GUARD_ROWS:]                     # tile-row 0 of the call: 16-byte aligned (a tile-row is n x 64 bytes)
        self.w_np = CR.weight_block(case, wc)
        w_all = np.full((8 + self.w_np.size + 8,), CR.GUARD, np.float32)
        w_all[8:8 + self.w_np.size] = self.w_np.reshape(-1)
        self.w_all = torch.from_numpy(w_all).to(dev)
        self.w = self.w_all[8:]
        self.rows_out = CR.out_rows(case, n)
        out = np.full((self.rows_out + 2, self.out_stride), CANARY, np.float32)
        out[:self.rows_out, case.out_col0:case.out_col0 + case.ncols] = prior
        self.out_before = out
        self.out = torch.from_numpy(out).to(dev)
        self.n_scratch = int(self.lib.snerf_dy_contract_scratch_floats(n, case.ncols, case.spr))
        assert self.n_scratch == CR.scratch_floats(n, case.ncols, case.spr)
        self.scratch_all = torch.full((16 + self.n_scratch + 16,), CANARY, device=dev)
        self.scratch_all[16:16 + self.n_scratch] = float("nan")
        self.scratch = self.scratch_all[16:] if self.n_scratch else None

    def run(self, **over):
        from smpl_nerf_amd._lib import current_stream, ptr
        c = self.case
        a = dict(dy=ptr(self.dy), n=self.n, first_row=c.first_row, n_feat=c.n_feat, w=ptr(self.w), w_stride=self.w_stride, col0=c.col0,
                 ncols=c.ncols, spr=c.spr, out=ptr(self.out), out_stride=self.out_stride, out_col0=c.out_col0, accumulate=c.accumulate,
                 scratch=ptr(self.scratch))
        a.update(over)
        with torch.cuda.device(self.out.device):
            rc = self.lib.snerf_dy_contract_f32(a["dy"], a["n"], a["first_row"], a["n_feat"], a["w"], a["w_stride"], a["col0"], a["ncols"],
                                                a["spr"], a["out"], a["out_stride"], a["out_col0"], a["accumulate"], a["scratch"],
                                                current_stream())
        torch.cuda.synchronize()
        return rc

    def result(self):
        """the call's block of out, after checking every canary of out and around the scratch"""
        c = self.case
        out = self.out.cpu().numpy()
        block = (slice(0, self.rows_out), slice(c.out_col0, c.out_col0 + c.ncols))
        outside = np.ones(out.shape, bool)
        outside[block] = False
        assert np.array_equal(out[outside], self.out_before[outside]), f"{c.name}: a canary of out was overwritten"
        s = self.scratch_all.cpu().numpy()
        assert np.all(s[:16] == CANARY) and np.all(s[16 + self.n_scratch:] == CANARY), f"{c.name}: a canary beside the scratch was overwritten"
        return out[block]

    def untouched(self):
        s = self.scratch_all.cpu().numpy()
        return (np.array_equal(self.out.cpu().numpy(), self.out_before) and np.all(s[:16] == CANARY) and np.all(s[16 + self.n_scratch:] == CANARY)
                and np.isnan(s[16:16 + self.n_scratch]).all())


def hold_integer(dev, case, n=None):
    n = case.n if n is None else n
    dense, wc, prior = CR.integer_inputs(case, n)
    call = Call(dev, case, n, dense, wc, prior)
    assert call.run() == OK, call.lib.snerf_last_error_string()
    got = call.result()
    want = CR.contract64(dense, call.w_np, case.col0, case.ncols, case.spr) + (prior.astype(np.float64) if case.accumulate else 0.0)
    assert np.abs(want).max() < CR.INT_LIMIT
    assert not np.isnan(got).any(), f"{case.name}: NaN in the output: a guard or an unwritten partial was read"
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, (f"{case.name}: {len(bad)} of {want.size} elements differ from float64, the first at (row, column) {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


@pytest.mark.parametrize("case", CR.instance_cases(), ids=lambda c: c.name)
def test_every_instance_in_every_mode(dev, case):
    """column tiles 1 / 2 / 4 / 6 / 8 x k-blocks 4 / 8 / 16 (none of the widths a multiple of 16: pad features, and fewer real
    k-blocks than the instance walks) x the three output modes, at first_row 3, col0 5, out_col0 2."""
    hold_integer(dev, case)


@pytest.mark.parametrize("case", CR.edge_cases(), ids=lambda c: c.name)
def test_edges_of_one_axis_at_a_time(dev, case):
    """features around the k-block counts, columns around the tile counts, samples around the 16-sample tile and the 64-sample
    workgroup, rays of 1 .. 192 samples and a single ray; dense strides, no offsets."""
    hold_integer(dev, case)


@pytest.mark.parametrize("case", CR.pass_cases(), ids=lambda c: c.name)
def test_column_passes(dev, case):
    """more than 128 columns: c_begin offsets into the weights, the partial rows and the output."""
    hold_integer(dev, case)


@pytest.mark.parametrize("case", CR.split_cases(), ids=lambda c: c.name)
def test_split_above_256_features(dev, case):
    """two calls, the second from tile-row first_row + 16 and weight row 256, accumulating; with accumulate = 0 the prior contents of
    out (-5 .. 5) must not survive."""
    hold_integer(dev, case)


@pytest.mark.parametrize("case", CR.GRID_STRIDE, ids=lambda c: c.name)
def test_grid_stride_loop(dev, case):
    """more sample tiles than two rounds of the capped grid (1 or 2 workgroups per CU): the loop, its prefetch of the next tile,
    the re-read of the last one and, with the ragged n, the sample clamp."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    n = CR.grid_stride_n(case, n_cu)
    assert (n + 15) // 16 > 2 * 4 * CR.workgroups_per_cu(case.n_feat, case.ncols) * n_cu
    hold_integer(dev, case, n)


@pytest.mark.parametrize("case", CR.REAL_CASES, ids=lambda c: c.name)
def test_real_valued_quality(dev, case):
    dense, wc = CR.real_inputs(case, case.n)
    prior = np.full((CR.out_rows(case, case.n), case.ncols), np.nan, np.float32)      # (accumulate = 0: must be overwritten)
    call = Call(dev, case, case.n, dense, wc, prior)
    assert call.run() == OK, call.lib.snerf_last_error_string()
    got = call.result()
    y64 = CR.contract64(dense, call.w_np, case.col0, case.ncols, case.spr)
    ek = CR.relative_error(got, y64)
    ec = CR.relative_error(CR.contract32(dense, call.w_np, case.col0, case.ncols, case.spr), y64)
    print(f"{case.name}: E kernel {ek:.3e}  E fp32 CPU {ec:.3e}  ratio {ek / ec:.2f}  max|y64| {np.abs(y64).max():.3e}")
    assert np.isfinite(got).all(), f"{case.name}: non-finite values"
    assert ek <= FACTOR * ec, f"{case.name}: E kernel {ek:.3e} > {FACTOR} x E fp32 CPU {ec:.3e}"


@pytest.mark.parametrize("case", CR.REPEAT_CASES, ids=lambda c: c.name)
def test_two_calls_give_the_same_bits(dev, case):
    """fixed summation order, no atomics (the header of csrc/contract.hip), in each mode and through the split."""
    dense, wc = CR.real_inputs(case, case.n)
    prior = np.random.default_rng(5).normal(size=(CR.out_rows(case, case.n), case.ncols)).astype(np.float32)
    outs = []
    for _ in range(2):
        call = Call(dev, case, case.n, dense, wc, prior)
        assert call.run() == OK
        outs.append(call.result())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------- refusals
def _refusal_call(dev, spr=16, n=80):
    case = CR._case("refusal", n, 40, 17, spr, 0)
    dense, wc, prior = CR.integer_inputs(case, n)
    return Call(dev, case, n, dense, wc, prior)


@pytest.mark.parametrize("name,spr,over", [
    ("n % spr != 0", 7, dict(n=79)),
    ("col0 + ncols > w_stride", 0, dict(w_stride=5 + 17 - 1)),
    ("out_col0 + ncols > out_stride", 0, dict(out_stride=2 + 17 - 1)),
    ("n_feat = 513", 16, dict(n_feat=513)),
    ("n_feat = 0", 16, dict(n_feat=0)),
    ("null scratch with spr > 0", 16, dict(scratch=None)),
    ("null scratch with spr > 0, a row per sample", 7, dict(scratch=None, n=77)),
])
def test_refusals_return_before_any_launch(dev, name, spr, over):
    call = _refusal_call(dev, spr)
    assert call.run(**over) == E_BADARG, name
    assert call.lib.snerf_last_error_string()
    assert call.untouched(), f"{name}: the refused call wrote something"


@pytest.mark.parametrize("spr", [0, 16])
def test_misaligned_dy_is_refused(dev, spr):
    call = _refusal_call(dev, spr)
    assert call.run(dy=call.dy.data_ptr() + 4) == E_ALIGN
    assert call.untouched()


@pytest.mark.parametrize("spr", [0, 16, 7])
def test_no_samples_is_ok_and_writes_nothing(dev, spr):
    call = _refusal_call(dev, spr)
    assert call.run(n=0) == OK
    assert call.untouched()


def test_scratch_floats(dev):
    from smpl_nerf_amd import _lib
    f = _lib.load().snerf_dy_contract_scratch_floats
    for n, ncols in ((80, 69), (1600, 1380), (16, 1)):
        assert f(n, ncols, 0) == 0
        assert f(n, ncols, 16) == n // 16 * ncols
        assert f(n, ncols, 5) == n * ncols and f(n, ncols, 1) == n * ncols
    assert f(2 ** 31, 1380, 7) == 2 ** 31 * 1380          # (64-bit)
    assert f(-1, 4, 0) == E_BADARG and f(4, 0, 0) == E_BADARG and f(4, 4, -1) == E_BADARG
    assert ctypes.sizeof(ctypes.c_int64) == 8
