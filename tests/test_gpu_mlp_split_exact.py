"""The split-precision kernels of the render MLP and of the warp net held to float64 EXACTLY on operands whose LOW parts are not zero:
the weight streams of snerf_mlp_pack_bf16 / snerf_mlp_pack_t_bf16 / snerf_warp_pack_bf16 with the f16x3 table of weight exponents,
the inference and the training forward (snerf_mlp_fwd_bf16_f32, snerf_mlp_fwd_train_bf16_f32), the dgrad and the wide wgrad jobs on
the 16-bit matrix cores (snerf_mlp_bwd_bf16_f32: mlp_bwd_bf16_kernel, mlp_wgrad_bf16_kernel), the whole f16x3 training path - the
per-sample operand scales, the statistics behind the activation and d Y rows, wgrad_f16_scales, mlp_wgrad_f16_kernel and
mlp_wgrad_direct_f16_kernel - and snerf_warp_fwd_bf16_f32.

tests/test_gpu_mlp_exact.py and tests/test_gpu_mlp_infer_exact.py stop at the first part: their weights are +-1.  Here one layer l* of
a net has weights +-q, q a constant that needs the mode's further parts (257 = 256 + 1, 131329 = 131072 + 256 + 1, 2049 = 2048 + 1),
and inputs / output gradients may be multiples of 257 (2049); every other layer is a signed selection, so nothing grows
(tests/exact_net_ref.py, "split precision: the low parts").  Families are named by the products they make non-zero:
  bf16x6  W3    3-part weights x 1-part operands at l*: (A1,B0), (A2,B0) in the forward and the dgrad; 3-part activations behind l* and
                3-part d Y in front of it against +-1: (A0,B2); in the wgrad 3-part d Y x 1-part X in front of l*, the reverse behind it;
          W65793  the same with q = 65793, which has TWO parts under round-to-nearest-even, the second negative (below);
          W2X2  inputs in multiples of 257 and q = 257: all four products of (A1,B1) in the forward of l*; 2-part d Y x 2-part X in the
                wgrad in front of l*;
          W2G2  output gradients in multiples of 257 and q = 257: (A1,B1) in the dgrad of l* (W2X2 cannot reach it: its d Y behind l*
                has one part), 2-part d Y x 2-part X in the wgrad behind l*;
          G2X2  no rich layer, inputs and output gradients in multiples of 257: (A1,B1) in every wide wgrad job;
  bf16x3, f16x3 (Terms<2> drops part 1 x part 1: rich x rich is not exact there and not asked for)
          W2    2-part weights x 1-part operands;  X2  2-part activations x +-1;  G2  2-part d Y x 1-part X and +-1 weights.
l* sweeps positions_pose_input, positional_net.1, the skip layer, additional_linear_layer, directional_input, directional_net.0 and
rgb_out_layer of the default net, and the skip layer of a 4-layer net; n = 77 and 333.  No family had to be dropped for any l*.

The constant first proposed for three parts was q = 65793 = 65536 + 256 + 1.  Under round-to-nearest-even that number has
TWO parts - 66048 - 255: the remainder 257 is above half a unit of 512 - and so has every integer below 2^17 (after the first part at most
256 is left, which fits 8 bits).  The smallest three-part integer is 131329 = 2^17 + 2^8 + 1, and that is the q of W3; 65793 stays as
the family W65793.  Likewise 257 x 257 k has two parts, so W2X2 is named for (A1,B1) alone and (A0,B2) is W3's.

tests/test_exact_net_host.py checks on the CPU, on the float64 reference alone and with the operand split RESTATED from the kernels,
that every operand recombines exactly from the parts the mode keeps, that every product outside the mode's term table is zero, that
every sum of absolute part-products is below 2^24 (so every partial sum in any order is an integer fp32 holds), that each family
makes its terms non-zero at l* and in each kind of GEMM, and that dropping any kept term from the emulation changes the result
(profiles/mlp_split_exact_cases.txt).  So a kernel that loses a term, a pack kernel that drops a low part or puts it into the wrong
tile, a wrong weight exponent, a wrong `delta` between two layers, a wrong job scale cannot pass: there is no tolerance here either.
One line per case is printed before its comparison (pytest -s; profiles/mlp_split_exact.txt holds a run).

Which entries ran: _lib.profile() has the launches (mlp_fwd_train / mlp_bwd, no mlp_bwd_inputs), and a spy on the ctypes handle has
the entries with their `nsplit`: 2, 3 or SPLIT_F16X3.  With SPLIT_F16X3 launch_wgrad (csrc/mlp_train.hip) launches mlp_wgrad_f16_kernel
for the wide and mlp_wgrad_direct_f16_kernel for the narrow jobs; the kernels' names are not visible from here, the argument is.  In
the bf16 modes the narrow jobs run the fp32 kernels.

Teeth on the device: W3 and W2X2 cases run with net.precision = "bf16x3" - a valid mode that drops their terms - differ from float64,
and the host emulation of bf16x3 predicts raw and every gradient of the device bit for bit: the restated split is the kernels' split.

Out of scope, and held by the tolerance tests only: the sin / cos columns of the fused encoder (not integers); the input-gradient
variant snerf_mlp_bwd_inputs_bf16_f32 (with identity columns _launch_backward takes the fp32 dgrad); the one-call training step and the
data-parallel entries (they launch these same kernels); widths other than 256 (they run exact fp32).  Real-valued data - rounding in
the accumulators, the error of a split of values that do NOT recombine - stays with test_mlp_backward_full_net,
test_relu_mask_flips_are_counted_and_everything_else_is_tight and test_f16x3_backward_is_homogeneous."""
import contextlib

import numpy as np
import pytest
import torch

import exact_net_ref as E
from test_gpu_mlp_exact import _dev, _hold, _nan_filled_empty, dev, nan_filled_empty  # noqa: F401  (the two fixtures: by name)

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name
SPIED = ("snerf_mlp_fwd_bf16_f32", "snerf_mlp_fwd_train_bf16_f32", "snerf_mlp_bwd_bf16_f32", "snerf_mlp_bwd_inputs_bf16_f32",
         "snerf_mlp_fwd_train_f32", "snerf_mlp_bwd_f32", "snerf_mlp_fwd_ws_f32", "snerf_mlp_fwd_infer_f32", "snerf_warp_fwd_bf16_f32",
         "snerf_warp_fwd_ws_f32")


@contextlib.contextmanager
def entries():
    """the C entries called inside, as (name, nsplit or None): every entry of SPIED is wrapped on the ctypes handle that
    smpl_nerf_amd/nets.py calls through"""
    from smpl_nerf_amd import _lib
    lib, calls, real = _lib.load(), [], {}

    def wrap(name, fn):
        def call(*args):
            calls.append((name, int(args[2]) if "bf16" in name and "warp" not in name else None))
            return fn(*args)
        return call
    for name in SPIED:
        real[name] = getattr(lib, name)
        setattr(lib, name, wrap(name, real[name]))
    try:
        yield calls
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)


def _render_net(dev, case, precision):
    from smpl_nerf_amd.nets import RenderRayNet
    state = E.rich_data(case)[0]
    net = RenderRayNet(**E.net_kw(case.net))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).train()
    net.precision = precision
    net.activation_budget_bytes = 0          # everything saved by the forward: one backward pass
    return net


def _inputs(dev, case):
    _, inp, _, d_raw = E.rich_data(case)
    return torch.from_numpy(inp["x"]).to(dev), torch.from_numpy(inp["d"]).to(dev), torch.from_numpy(d_raw).to(dev)


def _train(dev, case, precision, budget=None):
    """one training step through forward_fused: (raw, {name: gradient}, entries called, launches' names)"""
    from smpl_nerf_amd import _lib
    from smpl_nerf_amd.ops import PositionalEncoder
    pe = PositionalEncoder(0, True)
    net = _render_net(dev, case, precision)
    if budget is not None:
        net.activation_budget_bytes = budget(net, pe)
    x, d, d_raw = _inputs(dev, case)
    assert _lib.precision_code((net,)) == _lib.PRECISIONS[precision] != 0
    with entries() as calls, _lib.profile() as prof:
        raw = net.forward_fused(x, d, 1, pe, pe)
        (raw * d_raw).sum().backward()
    torch.cuda.synchronize()
    return raw.detach(), {k: p.grad for k, p in net.named_parameters()}, calls, [r[0] for r in prof.records]


def _premises(case):
    m = E.assert_rich_premises(case)
    cov = sorted({f"{k}{'/' + j if j else ''}:A{t[0]}B{t[1]}" for k, j, _, t in m["covered"] if t != (0, 0)})
    return (f"non-zero last part A {m['last_a']:.3f} B {m['last_b']:.3f}  sum of |part products| {m['max_abs_sum'] / E.INT_LIMIT:.3f} of 2^24  "
            f"{' '.join(cov)}")


def _split_entries_only(calls, mode, want):
    from smpl_nerf_amd import _lib
    assert [c[0] for c in calls] == want and all(c[1] == _lib.PRECISIONS[mode] for c in calls), (calls, want)


def _pairs(raw, grads, want_raw, want_grads):
    assert list(grads) == list(want_grads)
    return [("raw", raw, want_raw)] + [(f"d {k}", g, want_grads[k]) for k, g in reversed(list(grads.items()))]


# ---- training -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.ALL_RICH_CASES, ids=IDS)
def test_training_step_with_low_parts_is_exact(dev, case):
    """forward_fused + backward of loss = sum(raw * d_raw) with net.precision = the case's mode: raw and every parameter gradient equal
    float64; the launches are snerf_mlp_fwd_train_bf16_f32 and snerf_mlp_bwd_bf16_f32 with the mode's nsplit and nothing else"""
    line = _premises(case)
    raw, grads, calls, launches = _train(dev, case, case.mode)
    print(f"split-exact train {case.name:52s} {line}")
    _split_entries_only(calls, case.mode, ["snerf_mlp_fwd_train_bf16_f32", "snerf_mlp_bwd_bf16_f32"])
    assert launches == [f"mlp_fwd_train[n={case.net.n}]", f"mlp_bwd[n={case.net.n}]"], launches
    ref = E.rich_reference(case)
    _hold(case, _pairs(raw, grads, ref.out, ref.grads))


BLOCK_WISE = [next(c for c in E.RICH_CASES[mode] if c.rich == "positional_net.4" and c.net.n == 333) for mode in sorted(E.RICH_CASES)]


@pytest.mark.parametrize("case", BLOCK_WISE, ids=IDS)
def test_block_wise_backward_with_low_parts_is_exact(dev, case):
    """an activation budget of 120 samples: the forward is the split inference kernel, the backward recomputes the split training
    forward block by block (120, 120, 93 samples - the f16x3 statistics and job scales are then per block), flat.add_ over the blocks"""
    from smpl_nerf_amd import nets

    def budget(net, pe):
        per_sample = 4.0 * sum(nets._train_sizes(net.desc_for_encoders(pe, pe, False), case.net.n)) / case.net.n
        return int(120.5 * per_sample)

    raw, grads, calls, launches = _train(dev, case, case.mode, budget)
    blocks = [int(k[len("mlp_bwd[n="):-1]) for k in launches if k.startswith("mlp_bwd[n=")]
    print(f"split-exact train {case.name:52s} block-wise: {blocks}")
    assert len(blocks) >= 3 and sum(blocks) == case.net.n and max(blocks) < case.net.n, launches
    _split_entries_only(calls, case.mode, ["snerf_mlp_fwd_bf16_f32"] + ["snerf_mlp_fwd_train_bf16_f32", "snerf_mlp_bwd_bf16_f32"] * len(blocks))
    ref = E.rich_reference(case)
    _hold(case, _pairs(raw, grads, ref.out, ref.grads))


@pytest.mark.parametrize("case", [E.RICH_CASES[mode][2] for mode in sorted(E.RICH_CASES)], ids=IDS)
def test_two_runs_give_the_same_bits(dev, case):
    a, b = _train(dev, case, case.mode), _train(dev, case, case.mode)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


# ---- inference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.ALL_RICH_CASES, ids=IDS)
def test_inference_with_low_parts_is_exact(dev, case):
    """the same nets under no_grad through snerf_mlp_fwd_bf16_f32, in train() and in eval() mode (a split mode has one stream for both)"""
    from smpl_nerf_amd.ops import PositionalEncoder
    pe = PositionalEncoder(0, True)
    line = _premises(case)
    net = _render_net(dev, case, case.mode)
    x, d, _ = _inputs(dev, case)
    for mode in ("train", "eval"):
        net = net.train() if mode == "train" else net.eval()
        with torch.no_grad(), entries() as calls:
            raw = net.forward_fused(x, d, 1, pe, pe)
        torch.cuda.synchronize()
        print(f"split-exact infer {mode:5s} {case.name:46s} {line}")
        _split_entries_only(calls, case.mode, ["snerf_mlp_fwd_bf16_f32"])
        _hold(case, [(f"raw ({mode})", raw, E.rich_reference(case).out)])


@pytest.mark.parametrize("case", E.RICH_WARP_CASES, ids=IDS)
def test_fused_warp_net_with_low_parts_is_exact(dev, case):
    """snerf_warp_fwd_bf16_f32 (always three bf16 parts): 3-part weights in linear1 or linear2, and inputs in multiples of 257 against
    weights of +-257; 83 rays of 4 samples, warped = x + warp and sdirs = warped - o"""
    from smpl_nerf_amd.nets import WarpFieldNet
    from smpl_nerf_amd.ops import PositionalEncoder
    line = _premises(case)
    state, rows = E.rich_warp_data(case)
    wc = case.warp
    net = WarpFieldNet(width=wc.width, positions_dim=3, pose_dim=wc.row_len - 3)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev)
    net.precision = "bf16x6"
    with torch.no_grad(), entries() as calls:
        warp, warped, sdirs = net.forward_fused(*(torch.from_numpy(v).to(dev) for v in rows), wc.spr, PositionalEncoder(0, True))
    torch.cuda.synchronize()
    print(f"split-exact warp        {case.name:46s} {line}")
    assert [c[0] for c in calls] == ["snerf_warp_fwd_bf16_f32"], calls
    ref = E.warp_split_emulate(case)[2]
    _hold(case, [("warp", warp, ref["warp"]), ("warped", warped, ref["warped"]), ("sdirs", sdirs, ref["sdirs"])])


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.RICH_TEETH, ids=IDS)
def test_two_parts_lose_what_three_parts_hold_and_the_emulation_predicts_it(dev, case):
    """bf16x6 cases W3 and W2X2 with net.precision = "bf16x3": that mode drops (A2,B0), (A0,B2) and (A1,B1) - raw differs from
    float64, and equals the host emulation of bf16x3 bit for bit, as does every parameter gradient (two-part forward, dgrad and wide
    wgrad jobs, fp32 narrow jobs)"""
    ref = E.rich_reference(case)
    want_raw, want_grads, _ = E.split_emulate(case, "bf16x3")
    raw, grads, calls, _ = _train(dev, case, "bf16x3")
    wrong = int((raw.cpu().numpy().astype(np.float64) != ref.out).sum())
    print(f"split-exact teeth {case.name:52s} bf16x3: {wrong} of {ref.out.size} entries of raw differ from float64; the emulation "
          f"has {int((want_raw != ref.out).sum())}")
    _split_entries_only(calls, "bf16x3", ["snerf_mlp_fwd_train_bf16_f32", "snerf_mlp_bwd_bf16_f32"])
    assert wrong > 0 and not np.array_equal(want_raw, ref.out)
    _hold(case, _pairs(raw, grads, want_raw, want_grads))
