"""Integer networks on which the fused training kernels must equal float64 bit for bit, used ONLY by tests.

The training forward, the dgrad, the split-K wgrad with its reducer (csrc/mlp_train.hip, csrc/mlp_wgrad_jobs.h) and the warp net's
pair of kernels (csrc/warp.hip) add fp32 products in an order of their own.  On real-valued data two such orders differ by round-off
and may disagree on the sign of a pre-activation that is zero to round-off, so a comparison needs a tolerance and a ReLU-kink
adjudicator (tests/torch_ref.py).  Here every operand is a small integer: sparse weights in {-1, 0, +1}, integer biases, input rows
and output gradients.  As long as the sum of the ABSOLUTE values of the terms of every sum stays below 2^24, every partial sum in any
order is an integer that fp32 holds exactly, so the kernels must give the float64 result exactly - every forward output, every
parameter gradient, every input-row gradient - and a pre-activation of exactly 0 is masked identically on both sides.

  * render_net_data() / warp_net_data(): the generator - every weight row has exactly `r` entries of +-1 (more only where r rows x
    n_out cannot reach every input column: ceil(n_in / n_out) then, the smallest count that can), the 1- and 3-row heads are dense
    +-1, every input column of every layer meets a non-zero, biases in 0 .. 2, rows and output gradients in -2 .. 2;
  * render_net_reference() / warp_net_reference(): float64 - torch_ref.render_ray_net under autograd for the results, and the same
    network layer by layer in numpy for every layer's input, pre-activation and output gradient (checked against autograd);
  * preconditions() / assert_preconditions(): computed on the float64 reference alone - the exactness bound, and the coverage
    conditions that keep an exact comparison from passing vacuously;
  * assert_exact(): the comparison, naming tensor, first mismatching index, its 16 x 16 tile, got / want;
  * the cases of tests/test_gpu_mlp_exact.py, so that tests/test_exact_net_host.py checks on the CPU what the GPU tests take for
    granted.  `python tests/exact_net_ref.py` rewrites profiles/mlp_exact_cases.txt.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (run as a script: tests/conftest.py is not there to do it)
    sys.path.insert(0, ROOT)

import torch_ref as R  # noqa: E402

F32 = np.float32
INT_LIMIT = 2 ** 24           # integers below it are exact in fp32


# ------------------------------------------------------------------------------------------------ the generator
def _sparse_rows(rng, n_out, n_in, r, p_plus):
    """[n_out, n_in] fp32: k = max(r, ceil(n_in / n_out)) entries of +-1 per row (+1 with probability p_plus), no empty column"""
    k = min(n_in, max(r, -(-n_in // n_out)))
    cols = np.stack([rng.choice(n_in, k, replace=False) for _ in range(n_out)])
    count = np.bincount(cols.ravel(), minlength=n_in)
    for c in np.nonzero(count == 0)[0]:           # move an entry of a column that has a second one (c is in no row yet)
        spare = np.argwhere(count[cols] > 1)
        i, j = spare[rng.integers(len(spare))]
        count[cols[i, j]] -= 1
        cols[i, j] = c
        count[c] = 1
    w = np.zeros((n_out, n_in), F32)
    w[np.arange(n_out)[:, None], cols] = np.where(rng.random((n_out, k)) < p_plus, 1.0, -1.0)
    assert ((w != 0).sum(1) == k).all() and (w != 0).any(0).all()
    return w


def _dense_rows(rng, n_out, n_in, p_plus):
    return np.where(rng.random((n_out, n_in)) < p_plus, 1.0, -1.0).astype(F32)


def render_net_shapes(n_layers, width, positions_dim, directions_dim, additional_input_dim, skips, use_directional_input):
    """(name, n_out, n_in) of every nn.Linear of RenderRayNet in state_dict order"""
    pin = positions_dim + additional_input_dim
    out = [("positions_pose_input", width, pin)]
    out += [(f"positional_net.{i}", width, width + pin if i in skips else width) for i in range(n_layers - 1)]
    out += [("additional_linear_layer", width, width), ("sigma_out_layer", 1, width),
            ("directional_input", width // 2, width + (directions_dim if use_directional_input else 0)),
            ("directional_net.0", width // 2, width // 2), ("rgb_out_layer", 3, width // 2)]
    return out


NetCase = namedtuple("NetCase", "name n_layers width positions_dim directions_dim additional_input_dim skips use_directional_input "
                                "n r p_plus seed")
WarpCase = namedtuple("WarpCase", "name width row_len n spr r p_plus seed")


def net_kw(case):
    return dict(n_layers=case.n_layers, width=case.width, positions_dim=case.positions_dim, directions_dim=case.directions_dim,
                additional_input_dim=case.additional_input_dim, skips=list(case.skips),
                use_directional_input=case.use_directional_input)


def _state(rng, shapes, r, p_plus):
    state = {}
    for name, n_out, n_in in shapes:
        state[name + ".weight"] = _dense_rows(rng, n_out, n_in, p_plus) if n_out <= 3 else _sparse_rows(rng, n_out, n_in, r, p_plus)
        state[name + ".bias"] = rng.integers(0, 3, n_out).astype(F32)
    return state


def render_net_data(case):
    """(state dict, encoded rows [n, positions + additional + directions], d_raw [n, 4]) as fp32 arrays of integers"""
    rng = np.random.default_rng([case.seed, case.width, case.n_layers, case.n])
    state = _state(rng, render_net_shapes(*case[1:8]), case.r, case.p_plus)
    rows = rng.integers(-2, 3, (case.n, case.positions_dim + case.additional_input_dim + case.directions_dim)).astype(F32)
    d_raw = rng.integers(-2, 3, (case.n, 4)).astype(F32)
    return state, rows, d_raw


def warp_net_data(case):
    """(state dict of linear1 / linear2, rows, d_warp [n, 3]).  spr = 0: rows [n, row_len], WarpFieldNet.forward(rows).  spr > 0, the
    fused form with PE(x) = x: rows = (x [n, 3], pose [n / spr, row_len - 3], o [n / spr, 3]) and d_warp = (d_warp, d_warped, d_sdirs)."""
    rng = np.random.default_rng([case.seed, case.width, case.row_len, case.n])
    state = _state(rng, [("linear1", case.width, case.row_len), ("linear2", 3, case.width)], case.r, case.p_plus)
    draw = lambda *shape: rng.integers(-2, 3, shape).astype(F32)
    if not case.spr:
        return state, draw(case.n, case.row_len), draw(case.n, 3)
    assert case.n % case.spr == 0
    rays = case.n // case.spr
    return state, (draw(case.n, 3), draw(rays, case.row_len - 3), draw(rays, 3)), (draw(case.n, 3), draw(case.n, 3), draw(case.n, 3))


# ------------------------------------------------------------------------------------------------ float64
class Layer:
    """one nn.Linear of the reference: input a [n, n_in], pre-activation z [n, n_out], gradient dz of z, float64"""

    def __init__(self, name, a, w, b, relu):
        self.name, self.a, self.w, self.b, self.relu = name, a, w, b, relu
        self.z = a @ w.T + b
        self.abs_fwd = np.abs(a) @ np.abs(w).T + np.abs(b)          # sum of the absolute terms of every pre-activation
        self.out = np.maximum(self.z, 0.0) if relu else self.z
        self.dz = None

    def back(self, d_out, abs_d_out):
        """d_out: gradient of the layer's output (abs_d_out: the sum of the absolute terms that made it) -> gradient of its input"""
        self.abs_dout = abs_d_out
        self.dz = np.where(self.z > 0, d_out, 0.0) if self.relu else d_out
        self.dw, self.db = self.dz.T @ self.a, self.dz.sum(0)
        self.abs_dw, self.abs_db = np.abs(self.dz).T @ np.abs(self.a), np.abs(self.dz).sum(0)
        return self.dz @ self.w, np.abs(self.dz) @ np.abs(self.w)


Reference = namedtuple("Reference", "out grads d_rows layers extra")


def _f64(state):
    return {k: np.asarray(v, np.float64) for k, v in state.items()}


def _render_layers(case, P, x, d_raw):
    """the network of torch_ref.render_ray_net layer by layer, forward and backward, in float64 numpy"""
    W, pin, ddim = case.width, case.positions_dim + case.additional_input_dim, case.directions_dim
    lay = lambda name, a, relu: Layer(name, a, P[name + ".weight"], P[name + ".bias"], relu)
    pp, dd = x[:, :pin], x[:, x.shape[1] - ddim:]
    layers = [lay("positions_pose_input", pp, True)]
    for i in range(case.n_layers - 1):
        o = layers[-1].out
        layers.append(lay(f"positional_net.{i}", np.concatenate([o, pp], 1) if i in case.skips else o, True))
    add = lay("additional_linear_layer", layers[-1].out, False)
    sigma = lay("sigma_out_layer", add.out, False)
    din = lay("directional_input", np.concatenate([add.out, dd], 1) if case.use_directional_input else add.out, False)
    dnet = lay("directional_net.0", din.out, True)
    rgb = lay("rgb_out_layer", dnet.out, False)
    raw = np.concatenate([rgb.out, sigma.out], 1)
    # backward
    d_rows, abs_rows = np.zeros_like(x), np.zeros_like(x)
    g, ag = rgb.back(d_raw[:, :3], np.abs(d_raw[:, :3]))
    g, ag = dnet.back(g, ag)
    g, ag = din.back(g, ag)
    if case.use_directional_input:
        d_rows[:, x.shape[1] - ddim:] += g[:, W:]
        abs_rows[:, x.shape[1] - ddim:] += ag[:, W:]
    gs, ags = sigma.back(d_raw[:, 3:], np.abs(d_raw[:, 3:]))
    g, ag = add.back(g[:, :W] + gs, ag[:, :W] + ags)
    for l in layers[::-1]:
        g, ag = l.back(g, ag)
        if g.shape[1] > W or l is layers[0]:
            d_rows[:, :pin] += g[:, g.shape[1] - pin:]
            abs_rows[:, :pin] += ag[:, g.shape[1] - pin:]
            g, ag = g[:, :W], ag[:, :W]
    return raw, layers + [add, sigma, din, dnet, rgb], d_rows, abs_rows


@functools.lru_cache(maxsize=None)
def render_net_reference(case):
    """float64: raw, every parameter gradient and the gradient of the rows of loss = sum(raw * d_raw) from torch_ref.render_ray_net
    under autograd; the layers from the numpy restatement, which must agree with autograd exactly"""
    state, rows, d_raw = render_net_data(case)
    P = {k: torch.from_numpy(v).double().requires_grad_() for k, v in state.items()}
    x = torch.from_numpy(rows).double().requires_grad_()
    raw = R.render_ray_net(P, x, **{k: (tuple(v) if k == "skips" else v) for k, v in net_kw(case).items() if k != "width"})
    (raw * torch.from_numpy(d_raw).double()).sum().backward()
    grads = {k: v.grad.numpy() for k, v in P.items()}
    raw_np, layers, d_rows, abs_rows = _render_layers(case, _f64(state), rows.astype(np.float64), d_raw.astype(np.float64))
    assert np.array_equal(raw_np, raw.detach().numpy()) and np.array_equal(d_rows, x.grad.numpy())
    for l in layers:
        assert np.array_equal(l.dw, grads[l.name + ".weight"]) and np.array_equal(l.db, grads[l.name + ".bias"]), l.name
    return Reference(raw.detach().numpy(), grads, x.grad.numpy(), layers, {"abs_rows": abs_rows})


def _warp_rows(case, rows):
    if not case.spr:
        return rows
    x, pose, _ = rows
    return np.concatenate([x, np.repeat(pose, case.spr, 0)], 1)


@functools.lru_cache(maxsize=None)
def warp_net_reference(case):
    """float64: warp = linear2(relu(linear1(rows))) written plainly under autograd, and the same two layers in numpy.  The fused
    form (spr > 0): rows = [x | pose of the ray], warped = x + warp, sdirs = warped - o, loss = sum(warp g0 + warped g1 + sdirs g2);
    d_rows is then the gradient of the per-ray pose rows."""
    state, rows, d_out = warp_net_data(case)
    P = {k: torch.from_numpy(v).double().requires_grad_() for k, v in state.items()}
    extra = {}
    if case.spr:
        x, pose, o = (torch.from_numpy(v).double() for v in rows)
        leaf = pose.requires_grad_()
        full = torch.cat([x, leaf.repeat_interleave(case.spr, 0)], 1)
    else:
        leaf = full = torch.from_numpy(rows).double().requires_grad_()
    h = torch.relu(full @ P["linear1.weight"].T + P["linear1.bias"])
    warp = h @ P["linear2.weight"].T + P["linear2.bias"]
    if case.spr:
        warped = x + warp
        sdirs = warped - o.repeat_interleave(case.spr, 0)
        g = [torch.from_numpy(v).double() for v in d_out]
        (warp * g[0] + warped * g[1] + sdirs * g[2]).sum().backward()
        extra = {"warped": warped.detach().numpy(), "sdirs": sdirs.detach().numpy()}
        d_warp = sum(v.astype(np.float64) for v in d_out)
        abs_d = sum(np.abs(v).astype(np.float64) for v in d_out)
    else:
        (warp * torch.from_numpy(d_out).double()).sum().backward()
        d_warp = d_out.astype(np.float64)
        abs_d = np.abs(d_warp)
    grads = {k: v.grad.numpy() for k, v in P.items()}
    S = _f64(state)
    l1 = Layer("linear1", _warp_rows(case, rows).astype(np.float64), S["linear1.weight"], S["linear1.bias"], True)
    l2 = Layer("linear2", l1.out, S["linear2.weight"], S["linear2.bias"], False)
    g, ag = l1.back(*l2.back(d_warp, abs_d))
    if case.spr:           # the pose columns, summed over the samples of a ray
        g, ag = (v[:, 3:].reshape(case.n // case.spr, case.spr, -1).sum(1) for v in (g, ag))
    assert np.array_equal(l2.out, warp.detach().numpy()) and np.array_equal(g, leaf.grad.numpy())
    for l in (l1, l2):
        assert np.array_equal(l.dw, grads[l.name + ".weight"]) and np.array_equal(l.db, grads[l.name + ".bias"]), l.name
    extra["abs_rows"] = ag
    if case.spr:           # |x| + |warp terms| + |o|: warped and sdirs are integer sums as well
        extra["abs_sdirs"] = np.abs(rows[0]) + l2.abs_fwd + np.abs(np.repeat(rows[2], case.spr, 0))
    return Reference(warp.detach().numpy(), grads, leaf.grad.numpy(), [l1, l2], extra)


def reference(case):
    return render_net_reference(case) if isinstance(case, NetCase) else warp_net_reference(case)


# ------------------------------------------------------------------------------------------------ preconditions
def _tiles_without_nonzero(g):
    g = np.atleast_2d(g) != 0
    r, c = -(-g.shape[0] // 16) * 16, -(-g.shape[1] // 16) * 16
    pad = np.zeros((r, c), bool)
    pad[:g.shape[0], :g.shape[1]] = g
    return int((~pad.reshape(r // 16, 16, c // 16, 16).any(axis=(1, 3))).sum())


def preconditions(case):
    """Measured on the float64 reference alone:
      max_act, max_dy: largest |layer input| and |gradient of a layer's output|;
      max_abs_sum:     the largest sum of absolute terms over every forward pre-activation, every dgrad sum (rows included), every
                       weight- and bias-gradient sum, bias and all samples included - below 2^24 every order is exact in fp32;
      min_w_share, empty_tiles, min_b_share: smallest share of non-zero entries over the weight gradients, number of origin-aligned
                       16 x 16 tiles of a weight gradient without a non-zero, smallest non-zero share over the bias gradients;
      relu_min, relu_max: range over the ReLU layers of the share of active (sample, feature) outputs;
      zero_preacts:    ReLU pre-activations that are exactly 0."""
    ref = reference(case)
    m = dict(max_act=0.0, max_dy=0.0, max_abs_sum=0.0, min_w_share=1.0, empty_tiles=0, min_b_share=1.0, relu_min=1.0, relu_max=0.0,
             zero_preacts=0)
    for l in ref.layers:
        m["max_act"] = max(m["max_act"], float(np.abs(l.a).max()))
        m["max_dy"] = max(m["max_dy"], float(np.abs(l.dz).max()))
        m["max_abs_sum"] = max([m["max_abs_sum"]] + [float(v.max()) for v in (l.abs_fwd, l.abs_dout, l.abs_dw, l.abs_db)])
        m["min_w_share"] = min(m["min_w_share"], float((l.dw != 0).mean()))
        m["min_b_share"] = min(m["min_b_share"], float((l.db != 0).mean()))
        m["empty_tiles"] += _tiles_without_nonzero(l.dw)
        if l.relu:
            active = float((l.z > 0).mean())
            m["relu_min"], m["relu_max"] = min(m["relu_min"], active), max(m["relu_max"], active)
            m["zero_preacts"] += int((l.z == 0).sum())
    m["max_abs_sum"] = max([m["max_abs_sum"]] + [float(v.max()) for k, v in ref.extra.items() if k.startswith("abs_")])
    return m


def assert_preconditions(case, max_operand=None):
    """max_operand: additionally max|layer input| and max|d Y_l| of every layer at most this (the split-precision backward: 255, so
    that every operand fits the first bf16 part)"""
    m = preconditions(case)
    assert m["max_abs_sum"] < INT_LIMIT, (case.name, m)
    assert m["min_w_share"] >= 1 / 3 and m["empty_tiles"] == 0 and m["min_b_share"] >= 0.5, (case.name, m)
    assert case.n < 16 or (0.25 <= m["relu_min"] and m["relu_max"] <= 0.75), (case.name, m)
    assert m["zero_preacts"] >= 1, (case.name, m)
    if max_operand is not None:
        assert m["max_act"] <= max_operand and m["max_dy"] <= max_operand, (case.name, m)
    return m


def describe(case):
    m = preconditions(case)
    return (f"{case.name:28s} max|act| {m['max_act']:6.0f}  max|dY| {m['max_dy']:7.0f}  largest sum of |terms| {m['max_abs_sum']:9.0f} "
            f"({m['max_abs_sum'] / INT_LIMIT:.5f} of 2^24)  non-zero share dW >= {m['min_w_share']:.3f} db >= {m['min_b_share']:.3f}  "
            f"empty tiles {m['empty_tiles']}  ReLU active {m['relu_min']:.3f} .. {m['relu_max']:.3f}  zero pre-activations {m['zero_preacts']}")


# ------------------------------------------------------------------------------------------------ the comparison
def assert_exact(what, got, want64):
    """got (fp32, from the kernels) equals the float64 reference exactly: the reference survives the cast to fp32 unchanged (and is
    finite), and got is the cast entry for entry - so finite as well.  The message names the first mismatching index, its 16 x 16 tile and got / want."""
    got, want64 = np.asarray(got), np.asarray(want64, np.float64)
    assert got.dtype == F32 and got.shape == want64.shape, f"{what}: {got.dtype} {got.shape} against {want64.shape}"
    want = want64.astype(F32)
    assert np.isfinite(want64).all() and np.array_equal(want.astype(np.float64), want64), \
        f"{what}: the float64 reference is not representable in fp32"
    if np.array_equal(got, want):          # (NaN equals nothing: a non-finite entry is a mismatch, and want is finite)
        return
    bad = np.argwhere(got != want)
    idx = tuple(int(v) for v in bad[0])
    tile = tuple(v // 16 for v in idx[-2:])
    tiles = sorted({tuple(int(v) // 16 for v in b[-2:]) for b in bad})
    finite = "" if np.isfinite(got).all() else f" ({int((~np.isfinite(got)).sum())} non-finite values)"
    raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ{finite}, first at {idx} (16 x 16 tile {tile}): got {got[idx]!r}, "
                         f"want {want[idx]!r}; tiles with a mismatch ({len(tiles)}): {tiles[:12]}")


# ------------------------------------------------------------------------------------------------ the cases
def _net(name, n, n_layers=8, width=256, positions_dim=60, additional_input_dim=0, skips=(4,), use_directional_input=1, r=4,
         p_plus=0.5, seed=1):
    return NetCase(name, n_layers, width, positions_dim, 24, additional_input_dim, tuple(skips), use_directional_input, n, r, p_plus,
                   seed)


# r, sign balance and seeds: 4 entries per row, signs balanced, seed 1 unless the float64 reference alone misses a condition of
# preconditions() with them (measured; nothing here was chosen by what a kernel gives):
#   * one sample (n = 1): a gradient is one outer product, so a third of dW and half of db non-zero need about 0.6 of the features
#     active with a non-zero gradient; balanced signs give 0.5 (dW 0.16, db 0.16, 8 empty tiles).  70 % of the signs +1 and seed 2:
#     dW 0.42, db 0.62.  (The 25 .. 75 % ReLU condition does not apply below 16 samples.)
#   * 64 x 16: r = 2 leaves dW 0.14 / db 0.17 non-zero; r = 3 gives 0.41 / 0.55 with max|activation| 806.
#   * the split-precision case: r = 2 leaves db 0.45 .. 0.48 non-zero over four seeds; r = 3 with seed 2 gives 0.78 and
#     max|activation| 246, max|dY| 251 <= 255.
NET_DEFAULT = {n: _net(f"net-256x8-n{n}", n) for n in (77, 333, 1100)}
NET_DEFAULT[1] = _net("net-256x8-n1", 1, p_plus=0.7, seed=2)
NET_WIDTHS = [_net("net-128x4-skip1", 333, n_layers=4, width=128, skips=(1,)),
              _net("net-64x16-skip3-9-r3", 333, n_layers=16, width=64, skips=(3, 9), r=3),
              _net("net-512x3-skip1", 333, n_layers=3, width=512, skips=(1,)),
              _net("net-320x2", 333, n_layers=2, width=320, skips=()),
              _net("net-100x2-pos63", 333, n_layers=2, width=100, positions_dim=63, skips=()),
              _net("net-256x1", 333, n_layers=1, skips=())]
NET_INPUTS = [_net("net-256x8-add69", 333, additional_input_dim=69), _net("net-256x8-nodir", 333, use_directional_input=0)]
NET_SPLIT = _net("net-256x8-n333-r3", 333, r=3, seed=2)  # the split-precision backward: every operand fits the first bf16 part
SPLIT_MAX_OPERAND = 255
# Beyond the list of shapes above: up to n = 3584 the wide and the narrow wgrad jobs of the default net are split into the same number
# of chunks, so the reducer's choice between the two counts (a folded pair is summed over the WIDE jobs' chunks) is never put to the
# test.  At n = 4111 on 256 CUs they differ: wgrad_splits() below.  (3 per row: 0.19 of 2^24; 4 per row would use 0.90.)
NET_TWO_SPLITS = _net("net-256x8-n4111-r3", 4111, r=3)
NET_CASES = [NET_DEFAULT[n] for n in (1, 77, 333, 1100)] + NET_WIDTHS + NET_INPUTS + [NET_SPLIT, NET_TWO_SPLITS]
WIDE_512 = NET_WIDTHS[2]


def wgrad_splits(n, wide_jobs=9, narrow_jobs=14, n_cu=256):
    """(chunks of the wide jobs, chunks of the narrow jobs) of a weight-gradient launch: the rule of launch_wgrad (csrc/mlp_train.hip)
    restated - chunks of 1024 samples, shortened to fill one round of the chip (wide: a workgroup per CU; narrow: three), never
    below 128 (narrow: 64) samples, whole rounds when there are more workgroups than that; the chunk is a multiple of 16 samples and
    trailing empty chunks are not launched.  Defaults: the default net with both folds (9 wide, 20 - 6 narrow jobs) on an MI355X."""
    chunks = lambda per: min(128, max(1, -(-n // per)))
    g_wide = g_narrow = chunks(1024)
    slots = 3 * n_cu
    if narrow_jobs * g_narrow > slots:
        g_narrow = min(g_narrow, max(1, narrow_jobs * g_narrow // slots * slots // narrow_jobs))
    else:
        g_narrow = max(g_narrow, min(chunks(128), (n + 63) // 64, max(1, slots // narrow_jobs)))
    if wide_jobs * g_wide > n_cu:
        g_wide = min(g_wide, max(1, wide_jobs * g_wide // n_cu * n_cu // wide_jobs))
    else:
        g_wide = max(g_wide, min(chunks(128), max(1, n_cu // wide_jobs)))
    launched = lambda g: -(-n // ((-(-n // g) + 15) // 16 * 16))
    return launched(g_wide), launched(g_narrow)


def _warp(width, row_len, n, spr=0, r=4, p_plus=0.5, seed=1):
    name = f"warp-{width}-row{row_len}-n{n}" + (f"-spr{spr}" if spr else "")
    return WarpCase(name, width, row_len, n, spr, r, p_plus, seed)


# (one sample: seed 2 where seed 1 leaves less than a third of d linear1.weight or half of d linear1.bias non-zero)
_WARP_SEED = {(256, 69, 1): 2, (128, 40, 1): 2, (100, 69, 1): 2}
WARP_CASES = [_warp(width, row_len, n, seed=_WARP_SEED.get((width, row_len, n), 1))
              for width in (256, 128, 100) for row_len in (40, 69) for n in (1, 77, 333)]
WARP_FUSED = _warp(256, 43, 332, spr=4)                  # x (PE(x) = x: 3 columns) | 40 pose columns, 83 rays of 4 samples
ALL_CASES = NET_CASES + WARP_CASES + [WARP_FUSED]

PROFILE = os.path.join(ROOT, "profiles", "mlp_exact_cases.txt")
PROFILE_HEAD = ("# tests/exact_net_ref.py: what the float64 reference of every case of tests/test_gpu_mlp_exact.py measures (CPU; rewritten by\n"
                "# `python tests/exact_net_ref.py`, compared by tests/test_exact_net_host.py).  Every sum of |terms| is below 2^24 = 16777216.\n")


def profile_text():
    return PROFILE_HEAD + "".join(describe(c) + "\n" for c in ALL_CASES)


if __name__ == "__main__":
    with open(PROFILE, "w") as f:
        f.write(profile_text())
    print(profile_text())
