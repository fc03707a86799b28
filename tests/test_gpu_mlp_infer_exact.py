"""The inference kernels of the render MLP and of the warp net - the TRAIN = false instances of csrc/mlp.hip with FwdPipe's DMA ring
and kblock_deep(), the composed stream (mlp_compose_*_kernel, make_plan_infer), the per-ray fold (mlp_add_fold_kernel,
mlp_fwd_fold_kernel), the latency-class kernels in every launch form of lat_split (csrc/mlp_lat.hip), the hybrid launch, the widths
above 256, the layer-by-layer net above 512 (smpl_nerf_amd/layered.py over snerf_linear_fwd_f32), the split-precision inference
(csrc/mlp_bf16.hip) and the warp net's three no-grad entries (csrc/warp.hip) - held to float64 EXACTLY on integer networks, like the
training kernels in tests/test_gpu_mlp_exact.py, whose helpers this module imports.

tests/exact_net_ref.py makes the cases and tests/test_exact_net_host.py checks on the CPU what is taken for granted here: every
forward sum of absolute terms below 2^24 (through the composed maps and over the composition's own sums too), composed entries that
are integers, no weight tile without an entry, every ReLU feature active on some row and inactive on another, a zero
pre-activation in every case; profiles/mlp_infer_exact_cases.txt is the record.  The expected `raw` is always that of the UNCOMPOSED
float64 network.  No tolerance anywhere: a wrong k-block of one tile on a ragged width, a composed bias that is off by one, a
mis-addressed fold slot changes an integer and fails, and the message names tensor, index, 16 x 16 tile and got / want.  One line per
case is printed before its comparison (pytest -s; profiles/mlp_infer_exact.txt holds a run).

Entries: RenderRayNet.forward(rows) under no_grad (snerf_mlp_fwd_encoded_f32; above width 512 layered.render_ray_net);
forward_fused with PositionalEncoder(0, True) twice in train() mode (snerf_mlp_fwd_ws_f32, the regular stream) and in eval() mode
(snerf_mlp_fwd_infer_f32, the composed stream), with the fold where snerf_mlp_fold_workspace_bytes is non-zero; net.precision =
bf16x3 / bf16x6 / f16x3 (snerf_mlp_fwd_bf16_f32); WarpFieldNet.forward(rows) (snerf_warp_fwd_f32) and forward_fused
(snerf_warp_fwd_ws_f32, snerf_warp_fwd_bf16_f32).  Which kernels a size runs on is restated in exact_net_ref (launch_form) and
asserted for the device's compute-unit count, from which the sizes are derived; one child process with SNERF_LAT=0 runs the
throughput form of what small calls otherwise run on the latency kernels.

Not reachable with integers, and left to the tolerance tests (tests/test_gpu_infer_compose.py, test_gpu_weight_ring.py): the sin / cos
columns of the fused encoder (sin(2^k x) is an integer only at x = 0) - the fused cases cover the identity slots, the direction
normalisation, the per-ray broadcast and the fold, the 60 + 24-column k-block layout is covered through the encoded entry - and the
one-call render entries, which run these kernels behind expf and the sampler.

Split precision: every mode forms the products (weight part 0) x (operand part s) for every s it keeps (mlp_bf16_device.h: Terms<2>,
Terms<3>), and a weight of +-1 is its own part 0, so no mode drops a product these operands make non-zero: both cases run in all
three modes.  What the cases HERE hold exactly is therefore (A0,B0), (A0,B1) and (A0,B2) of snerf_mlp_fwd_bf16_f32 with the per-sample
f16x3 operand scale, and (A0,B0) of snerf_warp_fwd_bf16_f32.  The weights' further parts - parts 1 and 2 of every slab of
snerf_mlp_pack_bf16 / snerf_warp_pack_bf16, the f16x3 table of weight exponents above 2^14, the terms (A1,B0), (A2,B0), (A1,B1) of both
inference kernels - are held exactly by tests/test_gpu_mlp_split_exact.py, which runs its rich-weight cases through these same no-grad
entries.  Held by tolerance only (test_split_bf16_stress_against_fp32_kernel and the compose / weight-ring tests): real-valued
operands, which do not recombine from their parts, and the sin / cos columns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_net_ref as E
from test_gpu_mlp_exact import _dev, _hold, _nan_filled_empty, dev, nan_filled_empty  # noqa: F401  (the two fixtures: by name)

pytestmark = pytest.mark.gpu
IDS = lambda c: c.name
COMPOSED_CASES = [E.FUSED_POOL] + E.FUSED_RAYS + E.FUSED_ADD + E.FUSED_NETS          # widths up to 256


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _render_net(dev, case, composed=False, precision=None):
    """the case's net on the device: train() mode - its no-grad calls run on the regular stream - or eval() - the composed one"""
    from smpl_nerf_amd.nets import RenderRayNet
    state, _, _ = E.infer_data(case)
    net = RenderRayNet(**E.net_kw(case.net))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev)
    if precision is not None:
        net.precision = precision
    return net.eval() if composed else net.train()


def _fold_bytes(net, case, n):
    from smpl_nerf_amd import _lib
    from smpl_nerf_amd.ops import PositionalEncoder
    pe = PositionalEncoder(0, True)
    return int(_lib.load().snerf_mlp_fold_workspace_bytes(net.desc_for_encoders(pe, pe, bool(case.add_first)), n, case.spr))


def _run(dev, case, net, inputs=None, idx=None, form=""):
    """one no-grad call of the case's entry on `inputs` (default: the case's own rows) against the float64 reference, exactly"""
    from smpl_nerf_amd.ops import PositionalEncoder
    if inputs is None:
        inputs, idx = E.infer_data(case)[1], np.arange(case.net.n)
    want = E.infer_reference(case).out[idx]
    to = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    stream = "regular" if net.training else "composed"
    with torch.no_grad():
        if case.entry == "encoded":
            entry = "layered" if net._layered else "encoded"
            raw = net(to(inputs["rows"]))
        else:
            pe = PositionalEncoder(0, True)
            entry = "fused" if net.precision == "fp32" else f"fused {net.precision}"
            if net.precision != "fp32":
                stream = "split"
            elif not net.training:
                assert net.packed_weights_infer(net.desc_for_encoders(pe, pe, bool(case.add_first))) is not None
            if case.net.additional_input_dim and net.precision == "fp32":
                form = (form + " " if form else "") + ("fold" if _fold_bytes(net, case, len(idx)) else "no fold")
            raw = net.forward_fused(to(inputs["x"]), to(inputs["d"]), case.spr, pe, pe, additional=to(inputs["add"]),
                                    add_first=bool(case.add_first))
    torch.cuda.synchronize()
    print(f"infer-exact {entry:12s} {stream:8s} {case.name:34s} n={len(idx):6d} {form}")
    _hold(case, [("raw", raw, want)])


# ---- the regular stream -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.INFER_CASES, ids=IDS)
def test_encoded_rows_are_exact(dev, case):
    """RenderRayNet.forward(rows) under no_grad: the default net at n = 1, 77, 333, 1100; widths 64, 100 (63 position columns), 128,
    200, 256 x 1, 320, 384, 448, 512 and 576 (layer by layer); 69 additional columns; no directional input"""
    _run(dev, case, _render_net(dev, case))


@pytest.mark.parametrize("case", E.FUSED_CASES, ids=IDS)
def test_fused_calls_on_the_regular_stream_are_exact(dev, case):
    """forward_fused of a net in train() mode under no_grad: identity encoders, directions s e_i per ray (4 and 24 samples) and per
    sample, per-ray additional inputs first / last with the fold (24 samples per ray) and without (4), the structures and widths"""
    net = _render_net(dev, case)
    if case in E.FUSED_ADD:
        assert (_fold_bytes(net, case, case.net.n) > 0) == (case.spr == 24)
    _run(dev, case, net)


# ---- the composed stream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", COMPOSED_CASES, ids=IDS)
def test_fused_calls_on_the_composed_stream_are_exact(dev, case):
    """the same nets of width up to 256 in eval() mode: sigma' and dir-net' composed in float64 on the device and rounded once - to the
    integers they are - against the UNCOMPOSED float64 network; depths 1, 2, 4, 8, 10, no directional input, widths 64, 128, 200, the
    four forms of per-ray additional inputs"""
    net = _render_net(dev, case, composed=True)
    if case in E.FUSED_ADD:
        assert (_fold_bytes(net, case, case.net.n) > 0) == (case.spr == 24)
    _run(dev, case, net)


def test_widths_above_256_have_no_composed_stream(dev):
    """(and no fused cases here: with fewer than 17 input columns in a layer the kernels above width 256 refuse the descriptor)"""
    for case in E.INFER_WIDTHS:
        if 256 < case.net.width <= 512:
            net = _render_net(dev, case, composed=True)
            assert net.packed_weights_infer(net.desc_for_encoded()) is None


# ---- launch forms of the default net: the latency kernels, the hybrid launch ---------------------------------------------------------
@pytest.fixture(scope="module")
def pool_nets(dev):
    with nan_filled_empty():
        return {False: _render_net(dev, E.FUSED_POOL), True: _render_net(dev, E.FUSED_POOL, composed=True)}


LAT_LABELS = [label for label, _, _ in E.lat_sizes(256)]


@pytest.mark.parametrize("k", range(len(LAT_LABELS)), ids=[f"{i}-{l.replace(' ', '-')}" for i, l in enumerate(LAT_LABELS)])
def test_latency_launch_forms_are_exact(dev, pool_nets, k):
    """sizes derived from the device's CU count c that reach each branch of lat_split: at most one tile per CU (n = 1, 77, 1100), 16 x 2c
    (two paired workgroups per CU), 16 x 3c (the mixed launch), 16 (4c + 5) (a paired main launch and a remainder launch) and
    16 (2c + 3) - 5 (ragged, the mixed launch as remainder); rows drawn from the pool of 1100, both streams"""
    c = _cus(dev)
    label, n, kinds = E.lat_sizes(c)[k]
    assert E.launch_form(n, c) == (1, kinds, 0), (c, n, E.launch_form(n, c))
    inputs, idx = E.big_rows(E.FUSED_POOL, n, 11 + k)
    for composed in (False, True):
        _run(dev, E.FUSED_POOL, pool_nets[composed], inputs, idx, f"latency {' + '.join(kinds)} ({label}, {c} CUs)")


def test_hybrid_launch_is_exact(dev, pool_nets):
    """128 c + 16 c - 7 samples: lat_choose returns 2 - one whole round of 128-sample tiles on the throughput kernel, the ragged rest
    of c tiles on the latency kernels"""
    c = _cus(dev)
    n = E.hybrid_size(c)
    assert E.launch_form(n, c) == (2, ["single"], 128) and E.lat_choose_infer(n, c) == (2, 128 * c)
    inputs, idx = E.big_rows(E.FUSED_POOL, n, 23)
    for composed in (False, True):
        _run(dev, E.FUSED_POOL, pool_nets[composed], inputs, idx, f"hybrid: throughput {128 * c} + latency single ({c} CUs)")


# ---- the throughput form of small calls: one child process with SNERF_LAT=0 --------------------------------------------------------------
# (320 and 512: the encoded entry - no fused case above width 256, exact_net_ref.FUSED_CASES - which runs the throughput kernels anyway)
LAT0_WIDTHS = [c for c in E.FUSED_NETS + E.INFER_WIDTHS if c.net.name in ("fused-64x8", "fused-128x4-skip1", "fused-200x8",
                                                                           "infer-320x2", "infer-512x3-skip1")]
LAT0_FOLD = E.FUSED_ADD[:2]
LAT0_KEYS = [f"default {label} {s}" for label in ("333", "1100", "one tile per workgroup", "wrapped, ragged") for s in ("regular", "composed")] + \
            [f"{c.name} {s}" for c in LAT0_WIDTHS for s in (("regular", "composed") if c.net.width <= 256 else ("regular",))] + \
            [f"{c.name} {size} {s}" for c in LAT0_FOLD for size in ("pool", "wrapped") for s in ("regular", "composed")]


def _lat0_cases():
    assert os.environ.get("SNERF_LAT") == "0"
    dev = _dev()
    c = _cus(dev)
    with nan_filled_empty():
        nets = {False: _render_net(dev, E.FUSED_POOL), True: _render_net(dev, E.FUSED_POOL, composed=True)}
        for (label, n), key in zip(E.throughput_sizes(c), ("333", "1100", "one tile per workgroup", "wrapped, ragged")):
            tile = E.launch_form(n, c, lat=False)[2]
            inputs, idx = E.big_rows(E.FUSED_POOL, n, 31)
            for composed in (False, True):
                _run(dev, E.FUSED_POOL, nets[composed], inputs, idx, f"throughput, {tile}-sample tiles, {label} ({c} CUs)")
                print(f"ok default {key} {'composed' if composed else 'regular'}")
        for case in LAT0_WIDTHS:
            for composed in ((False, True) if case.net.width <= 256 else (False,)):
                _run(dev, case, _render_net(dev, case, composed=composed), form="throughput")
                print(f"ok {case.name} {'composed' if composed else 'regular'}")
        for case in LAT0_FOLD:
            wrapped = ((2 * c + 1) * 128 - 37) // 24 * 24              # whole rays of 24; the last 128-sample tile is ragged
            assert wrapped % 128 and wrapped > 2 * c * 128
            for composed in (False, True):
                net = _render_net(dev, case, composed=composed)
                for size, n in (("pool", case.net.n), ("wrapped", wrapped)):
                    assert _fold_bytes(net, case, n) > 0
                    inputs, idx = E.big_rows(case, n, 37)
                    _run(dev, case, net, inputs, idx, f"throughput {size}")
                    print(f"ok {case.name} {size} {'composed' if composed else 'regular'}")


@pytest.fixture(scope="module")
def lat0_output():
    from conftest import ROOT
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            "import test_gpu_mlp_infer_exact as M; M._lat0_cases()")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, SNERF_LAT="0"))
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("key", LAT0_KEYS, ids=[k.replace(" ", "-").replace(",", "") for k in LAT0_KEYS])
def test_throughput_form_is_exact(lat0_output, key):
    """with SNERF_LAT=0 (one child process runs them all): the default net at 333 and 1100 samples (64-sample tiles), c x 128 (one
    128-sample tile per workgroup) and (2c + 1) x 128 - 37 (every workgroup wraps its weight stream, last tile ragged); widths 64, 128,
    200 (fused) and 320, 512 (encoded rows) at 333; the fold at 336 samples and wrapped - each on the regular and, up to width 256, on the composed stream"""
    assert f"ok {key}" in lat0_output.splitlines()


# ---- split-precision inference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first-part", "last-part"])
@pytest.mark.parametrize("mode", sorted(E.SPLIT_MODES))
def test_split_precision_inference_is_exact(dev, mode, which):
    """snerf_mlp_fwd_bf16_f32 through net.precision, width 256, identity encoders.  first-part: every layer input is at most 255 - its
    own first part in every mode.  last-part: the positions carry a multiplier (31, 3001, 301) that takes the layer inputs past what
    the parts before the last hold; tests/test_exact_net_host.py asserts on the reference, with the split restated from
    mlp_bf16_device.h, that every layer input recombines exactly from the mode's parts and that some need the last one.  The
    operand scaling of f16x3 is by powers of two, the accumulation fp32 below 2^24: exact all the same."""
    from smpl_nerf_amd import _lib
    case = E.SPLIT_FIRST if which == "first-part" else E.SPLIT_LAST[mode]
    premise = E.split_premise(case, mode)
    assert premise["exact"] and premise["max_abs_sum"] < E.INT_LIMIT and (premise["last_share"] > 0) == (which == "last-part")
    net = _render_net(dev, case, precision=mode)
    assert _lib.precision_code((net,)) == _lib.PRECISIONS[mode] != 0
    _run(dev, case, net, form=f"{which}: non-zero last part {premise['last_share']:.5f}")


# ---- the warp net ---------------------------------------------------------------------------------------------------------------------
def _warp_net(dev, case, positions_dim):
    from smpl_nerf_amd.nets import WarpFieldNet
    state, rows, _ = E.warp_net_data(case)
    net = WarpFieldNet(width=case.width, positions_dim=positions_dim, pose_dim=case.row_len - positions_dim)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.to(dev), rows


@pytest.mark.parametrize("case", E.WARP_CASES, ids=IDS)
def test_warp_net_rows_are_exact(dev, case):
    """WarpFieldNet.forward(rows) under no_grad (snerf_warp_fwd_f32): widths 256, 128, 100, rows of 40 and 69 floats, n = 1, 77, 333"""
    net, rows = _warp_net(dev, case, 0)
    with torch.no_grad():
        warp = net(torch.from_numpy(rows).to(dev))
    torch.cuda.synchronize()
    print(f"infer-exact warp rows             {case.name:34s} n={case.n:6d}")
    _hold(case, [("warp", warp, E.warp_net_reference(case).out)])


@pytest.mark.parametrize("precision", ["fp32", "bf16x6"])
@pytest.mark.parametrize("case", E.WARP_INFER_FUSED, ids=IDS)
def test_fused_warp_net_is_exact(dev, case, precision):
    """forward_fused under no_grad with PE(x) = x: snerf_warp_fwd_ws_f32 at 4 samples per ray (no fold: csrc/warp.hip folds the pose
    columns per ray from 8 samples per ray) and at 8 (fold), and snerf_warp_fwd_bf16_f32 through net.precision (three bf16 parts; every
    input is at most 10, its own first part): warp, warped = x + warp and sdirs = warped - o"""
    from smpl_nerf_amd import _lib
    from smpl_nerf_amd.ops import PositionalEncoder
    pe = PositionalEncoder(0, True)
    net, (x, pose, o) = _warp_net(dev, case, 3)
    net.precision = precision
    fold = int(_lib.load().snerf_warp_fold_workspace_bytes(net.desc_for_encoder(pe), case.n, case.spr))
    assert (fold > 0) == (case.spr >= 8)
    with torch.no_grad():
        warp, warped, sdirs = net.forward_fused(*(torch.from_numpy(v).to(dev) for v in (x, pose, o)), case.spr, pe)
    torch.cuda.synchronize()
    form = "split" if precision != "fp32" else "fold" if fold else "no fold"
    print(f"infer-exact warp fused {precision:6s}     {case.name:34s} n={case.n:6d} {form}")
    ref = E.warp_net_reference(case)
    _hold(case, [("warp", warp, ref.out), ("warped", warped, ref.extra["warped"]), ("sdirs", sdirs, ref.extra["sdirs"])])
