"""The fused training kernels - training forward, dgrad, wide and narrow split-K wgrad with its reducer (csrc/mlp_train.hip,
csrc/mlp_wgrad_jobs.h, csrc/mlp_lat.hip), the warp net's pair (csrc/warp.hip), the input-gradient contractions behind them and
the split-precision backward (csrc/mlp_train_bf16.hip) - held to float64 EXACTLY, element by element, on whole integer networks.

tests/exact_net_ref.py makes the networks: sparse weights in {-1, 0, +1}, integer biases, rows and output gradients, sized so that
the sum of the absolute terms of every sum stays below 2^24 (tests/test_exact_net_host.py checks that on the float64 reference
alone, and that a float32 CPU run equals float64; profiles/mlp_exact_cases.txt has every case's headroom).  Every partial sum in any
order is then an integer fp32 holds exactly, so raw / warp, every parameter gradient and the gradient of the input rows must equal
the float64 reference bit for bit - no tolerance, and no ReLU kink: a pre-activation of exactly 0 (every case has some) is masked
the same on both sides.  A wrong bias sum, one wrong 16 x 16 tile, a mis-decoded job or a double-counted ragged chunk changes an
integer and fails; the message names the tensor, the first index, its tile and got / want.  Every buffer the Python layer allocates
with torch.empty starts as NaN here (nan_filled_empty), so a partial or a tile-row that is read without having been written fails
as well.

Paths: RenderRayNet.forward(x_enc) and WarpFieldNet.forward(rows) under autograd (snerf_mlp_fwd_encoded_train_f32, snerf_mlp_bwd_f32,
snerf_dy_contract_f32; snerf_warp_fwd_train_f32, snerf_warp_bwd_f32), WarpFieldNet.forward_fused with an identity-only position
encoder, and snerf_mlp_bwd_bf16_f32 through ctypes on the `act` of the fp32 encoded training forward.

Cases whose generator parameters differ from the default (4 non-zeros per weight row, balanced signs) and why: tests/exact_net_ref.py
above NET_DEFAULT - the single-sample net, the 64 x 16 net (3 per row, not 2) and the split-precision net (3 per row, not 2) miss a
coverage condition on the reference otherwise.  No shape was replaced: the Python classes accept every one the cases name.  One
case more than the shapes' list: the default net at n = 4111, where the wide and the narrow jobs are split into different numbers of
chunks (test_default_net_with_two_chunk_counts_is_exact).

Split precision: every weight of every case HERE is in {-1, 0, +1} and every operand of test_split_precision_backward_is_exact fits
the first bf16 part, so this module holds only the products (part 0) x (part 0) of the split kernels.  The further parts - weight
parts 1 and 2 of the streams of snerf_mlp_pack_bf16 / snerf_mlp_pack_t_bf16, the terms (A1,B0), (A2,B0), (A1,B1), (A0,B1), (A0,B2) of
Terms<2> / Terms<3> in the training forward snerf_mlp_fwd_train_bf16_f32, the dgrad and the wide wgrad jobs, and the whole f16x3
training path with its weight exponents, per-sample operand scales, layer statistics and job scales (wgrad_f16_scales,
mlp_wgrad_f16_kernel, mlp_wgrad_direct_f16_kernel) - are held exactly by tests/test_gpu_mlp_split_exact.py.  Still held by tolerance
only (tests/test_gpu_grad.py, test_gpu_round*.py): the split kernels on real-valued data, whose operands do not recombine from their
parts and whose sums round; the sin / cos columns; snerf_mlp_bwd_inputs_bf16_f32."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_net_ref as E

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from smpl_nerf_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    return _dev()


@contextlib.contextmanager
def nan_filled_empty():
    """Inside, torch.empty / torch.empty_like give NaN-filled float tensors on the GPU (what SNERF_TEST_POISON_EMPTY does for a whole
    run, tests/conftest.py): activations, d Y, the wgrad partials and the gradient sink of smpl_nerf_amd/nets.py start as NaN, not as
    whatever the allocator hands out - often zeros, which a sum over a partial nobody wrote would not notice."""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(NAN) if t.is_cuda and t.dtype.is_floating_point and t.numel() else t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


@pytest.fixture(autouse=True)
def _nan_filled_empty():
    with nan_filled_empty():
        yield


def _hold(case, pairs):
    """every (name, got, float64 reference) exactly; all tensors that differ are reported, from the output towards the input"""
    misses = []
    for name, got, want in pairs:
        try:
            E.assert_exact(f"{case.name}: {name}", got.detach().cpu().numpy() if torch.is_tensor(got) else got, want)
        except AssertionError as e:
            misses.append(str(e))
    assert not misses, f"{len(misses)} of {len(pairs)} tensors differ from float64:\n" + "\n".join(misses)


# ---- RenderRayNet.forward(x_enc) under autograd -------------------------------------------------------------------------------------
def _render_net(dev, case):
    from smpl_nerf_amd.nets import RenderRayNet
    state, rows, d_raw = E.render_net_data(case)
    net = RenderRayNet(**E.net_kw(case))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev)
    net.activation_budget_bytes = 0          # everything saved by the forward: one backward pass
    return net, torch.from_numpy(rows).to(dev), torch.from_numpy(d_raw).to(dev)


def _run_render_net(dev, case, budget=None):
    """raw, parameter gradients and x_enc.grad of loss = sum(raw * d_raw) against the float64 reference; returns the launches' names"""
    from smpl_nerf_amd import _lib
    net, x, d_raw = _render_net(dev, case)
    if budget is not None:
        net.activation_budget_bytes = budget(net)
    x.requires_grad_()
    with _lib.profile() as prof:
        raw = net(x)
        (raw * d_raw).sum().backward()
    torch.cuda.synchronize()
    ref = E.render_net_reference(case)
    names = [k for k, _ in net.named_parameters()]
    assert names == list(ref.grads)
    _hold(case, [("raw", raw, ref.out)] + [(f"d {k}", p.grad, ref.grads[k]) for k, p in reversed(list(net.named_parameters()))] +
          [("d x_enc", x.grad, ref.d_rows)])
    return [r[0] for r in prof.records]


@pytest.mark.parametrize("case", E.NET_CASES[:4], ids=IDS)
def test_default_net_is_exact(dev, case):
    """width 256, depth 8, skip 4, 60 + 24 columns: both wgrad folds (the direction columns and the sigma head ride with
    directional_input's wide job); n = 1, 77, 333, 1100 are 1, 1, 3 and 9 chunks of at most 128 samples with a ragged last one"""
    _run_render_net(dev, case)


def test_default_net_with_two_chunk_counts_is_exact(dev):
    """n = 4111: on 256 CUs the wide jobs run in 26 chunks of 160 samples and the narrow ones in 33 of 128 (exact_net_ref.wgrad_splits,
    a restatement of launch_wgrad's rule), so the reducer has to sum the wide pairs and the two folded ones - sigma head, direction
    columns - over 26 partials and the direct ones over 33; up to n = 3584 the two counts are equal"""
    print("compute units:", torch.cuda.get_device_properties(dev).multi_processor_count, "- splits on 256:", E.wgrad_splits(4111))
    _run_render_net(dev, E.NET_TWO_SPLITS)


@pytest.mark.parametrize("case", E.NET_WIDTHS, ids=IDS)
def test_other_widths_are_exact(dev, case):
    """128 x 4 with skip 1; 64 x 16 with skips 3 and 9; 512 x 3 with skip 1, whose wide pairs have 2 x 2 job groups (ib > 0); 320 x 2;
    100 x 2 with 63 position columns, zero-padded inside 128; depth 1 - each at n = 333"""
    _run_render_net(dev, case)


@pytest.mark.parametrize("case", E.NET_INPUTS, ids=IDS)
def test_additional_inputs_and_no_directional_input_are_exact(dev, case):
    """69 additional columns (no multiple of 16: narrow jobs of their own, in layer 0 and in the skip layer); use_directional_input = 0
    (the 24 direction columns of the rows are not read: their gradient is exactly zero)"""
    _run_render_net(dev, case)
    if not case.use_directional_input:
        assert not E.render_net_reference(case).d_rows[:, -case.directions_dim:].any()


def test_block_wise_backward_is_exact(dev):
    """an activation budget of 120 samples: the backward walks n = 333 in blocks of 120, 120 and 93 - training forward recomputed,
    dgrad, wgrad, reduce per block, flat.add_ over the blocks - and is exact all the same"""
    from smpl_nerf_amd import nets
    case = E.NET_DEFAULT[333]

    def budget(net):
        per_sample = 4.0 * sum(nets._train_sizes(net.desc_for_encoded(), case.n)) / case.n
        return int(120.5 * per_sample)

    launches = _run_render_net(dev, case, budget)
    blocks = [int(k[len("mlp_bwd[n="):-1]) for k in launches if k.startswith("mlp_bwd[n=")]
    print("blocks of the backward:", blocks)
    assert len(blocks) >= 3 and sum(blocks) == case.n and max(blocks) < case.n, launches
    assert sum(k.startswith("mlp_fwd_train[") for k in launches) == len(blocks)


# ---- the same with SNERF_LAT=0: the throughput dgrad ---------------------------------------------------------------------------------
LAT0_CASES = [E.NET_DEFAULT[333], E.NET_DEFAULT[1100]]


def _lat0_cases():
    assert os.environ.get("SNERF_LAT") == "0"
    dev = _dev()
    for case in LAT0_CASES:
        with nan_filled_empty():
            _run_render_net(dev, case)
        print(f"ok {case.name}")


@pytest.fixture(scope="module")
def lat0_output():
    from conftest import ROOT
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            "import test_gpu_mlp_exact as M; M._lat0_cases()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, SNERF_LAT="0"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("case", LAT0_CASES, ids=IDS)
def test_throughput_dgrad_is_exact(lat0_output, case):
    """calls this small otherwise run the latency-class dgrad (csrc/mlp_lat.hip); one child process with SNERF_LAT=0 runs both"""
    assert f"ok {case.name}" in lat0_output.splitlines()


# ---- WarpFieldNet ---------------------------------------------------------------------------------------------------------------------
def _warp_net(dev, case, positions_dim):
    from smpl_nerf_amd.nets import WarpFieldNet
    state, rows, d_out = E.warp_net_data(case)
    net = WarpFieldNet(width=case.width, positions_dim=positions_dim, pose_dim=case.row_len - positions_dim)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.to(dev), rows, d_out


@pytest.mark.parametrize("case", E.WARP_CASES, ids=IDS)
def test_warp_net_rows_are_exact(dev, case):
    """WarpFieldNet.forward(rows): descriptor (width, 0, 0, row length) - widths 256, 128 and 100 (zero-padded inside 128), rows of 40
    and 69 floats, n = 1, 77, 333: warp, the four parameter gradients and rows.grad"""
    net, rows, d_warp = _warp_net(dev, case, 0)
    x = torch.from_numpy(rows).to(dev).requires_grad_()
    warp = net(x)
    (warp * torch.from_numpy(d_warp).to(dev)).sum().backward()
    torch.cuda.synchronize()
    ref = E.warp_net_reference(case)
    _hold(case, [("warp", warp, ref.out)] + [(f"d {k}", p.grad, ref.grads[k]) for k, p in reversed(list(net.named_parameters()))] +
          [("d rows", x.grad, ref.d_rows)])


def test_fused_warp_net_with_identity_encoder_is_exact(dev):
    """forward_fused with PositionalEncoder(0, identity): PE(x) = x, 83 rays of 4 samples, the 40 pose columns per-ray constants.
    warped = x + warp and sdirs = warped - o are integer sums and exact as well; the pose gradient is summed over a ray's samples."""
    from smpl_nerf_amd.ops import PositionalEncoder
    case = E.WARP_FUSED
    net, (x, pose, o), d_out = _warp_net(dev, case, 3)
    x, pose, o = (torch.from_numpy(v).to(dev) for v in (x, pose, o))
    pose.requires_grad_()
    warp, warped, sdirs = net.forward_fused(x, pose, o, case.spr, PositionalEncoder(0, True))
    g = [torch.from_numpy(v).to(dev) for v in d_out]
    (warp * g[0] + warped * g[1] + sdirs * g[2]).sum().backward()
    torch.cuda.synchronize()
    ref = E.warp_net_reference(case)
    _hold(case, [("warp", warp, ref.out), ("warped", warped, ref.extra["warped"]), ("sdirs", sdirs, ref.extra["sdirs"])] +
          [(f"d {k}", p.grad, ref.grads[k]) for k, p in reversed(list(net.named_parameters()))] + [("d pose", pose.grad, ref.d_rows)])


# ---- the split-precision backward through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [3, 2])
def test_split_precision_backward_is_exact(dev, nsplit):
    """snerf_mlp_bwd_bf16_f32 (stream from snerf_mlp_pack_t_bf16) on the `act` of the fp32 encoded training forward - a mix the header
    allows.  Every layer input and every d Y_l of the case is an integer of at most 255 (asserted on the reference), so it is its own
    first bf16 part, the further parts and every cross term are zero, and the fp32 accumulation is exact as before: flat_grad equals
    float64 exactly with 3 parts and with 2.  (Operands with further parts, the split training forward and f16x3 with the statistics
    of its own forward: tests/test_gpu_mlp_split_exact.py.)"""
    from smpl_nerf_amd import _lib, nets
    lib = _lib.load()
    case = E.NET_SPLIT
    E.assert_preconditions(case, E.SPLIT_MAX_OPERAND)
    ref = E.render_net_reference(case)
    net, x, d_raw = _render_net(dev, case)
    desc, n, s = net.desc_for_encoded(), case.n, _lib.current_stream()
    act_floats, dy_floats, gpart_floats = nets._train_sizes(desc, n)
    raw = torch.full((n, 4), NAN, device=dev)
    act = torch.empty(act_floats, device=dev)
    packed = net.packed_weights(desc, training=True)
    _lib.check(lib.snerf_mlp_fwd_encoded_train_f32(desc, _lib.ptr(packed), _lib.ptr(x), n, x.shape[1], _lib.ptr(raw), _lib.ptr(act), s),
               "snerf_mlp_fwd_encoded_train_f32")
    params = net._ordered_params()
    flatp = nets.flat_parameter_vector(params).contiguous()
    n_params = int(lib.snerf_mlp_param_floats(desc))
    assert flatp.numel() == n_params
    nbytes = int(lib.snerf_mlp_packed_t_bf16_bytes(desc, nsplit, 0))
    assert nbytes > 0
    packed_t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.snerf_mlp_pack_t_bf16(desc, _lib.ptr(flatp), _lib.ptr(packed_t), nsplit, 0, s), "snerf_mlp_pack_t_bf16")
    dy, gpart = torch.empty(dy_floats, device=dev), torch.empty(gpart_floats, device=dev)
    flat = torch.full((n_params,), NAN, device=dev)
    _lib.check(lib.snerf_mlp_bwd_bf16_f32(desc, _lib.ptr(packed_t), nsplit, _lib.ptr(act), _lib.ptr(d_raw), n, _lib.ptr(dy),
                                          _lib.ptr(gpart), _lib.ptr(flat), s), "snerf_mlp_bwd_bf16_f32")
    torch.cuda.synchronize()
    names = [k for k, _ in net.named_parameters()]
    assert [p.data_ptr() for _, p in net.named_parameters()] == [p.data_ptr() for p in params]      # flat_grad is in this order
    grads = nets._grads_from_flat(flat, [p.shape for p in params])
    _hold(case, [("raw", raw, ref.out)] + [(f"d {k} (nsplit {nsplit})", g, ref.grads[k]) for k, g in reversed(list(zip(names, grads)))])
