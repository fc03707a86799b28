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
    granted.  `python tests/exact_net_ref.py` rewrites profiles/mlp_exact_cases.txt;
  * the inference cases of tests/test_gpu_mlp_infer_exact.py (second half of this file): the same networks through the no-grad
    entries - infer_data() / infer_reference() / infer_preconditions(), the composed maps of the inference stream restated
    (composed_maps()), big_rows() for large calls, the launch rule of the latency kernels (launch_form()) and the operand split of the
    split-precision kernels (split_parts()) restated; their record is profiles/mlp_infer_exact_cases.txt;
  * the cases of tests/test_gpu_mlp_split_exact.py (third part of this file): nets with a "rich" layer whose weights need the further
    parts of a split mode - rich_data() / rich_reference(), the weight split and the wgrad scales restated (weight_parts(),
    operand_parts()), split_emulate(): the sum over a mode's terms of the restated parts for every GEMM of a training step, and
    rich_premises(): the conditions under which that sum is the float64 sum; their record is profiles/mlp_split_exact_cases.txt.
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
def _sparse_rows(rng, n_out, n_in, r, p_plus, fill_tiles=0):
    """[n_out, n_in] fp32: k = max(r, ceil(n_in / n_out)) entries of +-1 per row (+1 with probability p_plus), no empty column;
    fill_tiles: no origin-aligned 16 x 16 tile without an entry either (_fill_tiles)"""
    k = min(n_in, max(r, -(-n_in // n_out)))
    cols = np.stack([rng.choice(n_in, k, replace=False) for _ in range(n_out)])
    count = np.bincount(cols.ravel(), minlength=n_in)
    for c in np.nonzero(count == 0)[0]:           # move an entry of a column that has a second one (c is in no row yet)
        spare = np.argwhere(count[cols] > 1)
        i, j = spare[rng.integers(len(spare))]
        count[cols[i, j]] -= 1
        cols[i, j] = c
        count[c] = 1
    extra = _fill_tiles(rng, cols, n_in) if fill_tiles else []
    w = np.zeros((n_out, n_in), F32)
    signs = np.where(rng.random((n_out, k)) < p_plus, 1.0, -1.0)
    if fill_tiles and k > 1:
        # as many +1 as -1 in every row (one more of either where k is odd), whatever p_plus: the outputs of a ReLU layer share a positive
        # mean, and a row that does not cancel it is active on nearly every sample (one sign only: on every sample or on none)
        plus = k // 2 + (rng.random(n_out) < 0.5) * (k % 2)
        signs = np.where(rng.permuted(np.tile(np.arange(k), (n_out, 1)), axis=1) < plus[:, None], 1.0, -1.0)
    w[np.arange(n_out)[:, None], cols] = signs
    for i, c in extra:
        w[i, c] = 1.0 if rng.random() < p_plus else -1.0
    assert ((w != 0).sum(1) == k + np.bincount([i for i, _ in extra], minlength=n_out)).all() and (w != 0).any(0).all()
    return w


def _fill_tiles(rng, cols, n_in):
    """cols [n_out, k] (column indices, distinct per row), in place: every origin-aligned 16 x 16 tile of the [n_out, n_in] matrix
    gets an entry - into an empty tile moves an entry of one of its rows that sits in a tile with a second entry and in a column
    with a second entry (so no tile and no column is emptied), to a column of the empty tile drawn at random.  Where a tile-row has
    no such entry (the last two rows of a 50-row matrix: 8 entries for 8 tiles) the tile gets an entry MORE: returns those (row, column)"""
    extra = []
    n_out, tc = cols.shape[0], -(-n_in // 16)
    tiles = np.zeros((-(-n_out // 16), tc), np.int64)
    np.add.at(tiles, (np.arange(n_out)[:, None] // 16, cols // 16), 1)
    count = np.bincount(cols.ravel(), minlength=n_in)
    for ti, tj in np.argwhere(tiles == 0):
        rows = np.arange(16 * ti, min(n_out, 16 * ti + 16))
        spare = np.argwhere((tiles[ti][cols[rows] // 16] > 1) & (count[cols[rows]] > 1))
        c = int(rng.integers(16 * tj, min(n_in, 16 * tj + 16)))          # (no entry of the tile-row is in this tile: it is empty)
        if not len(spare):
            extra.append((int(rows[rng.integers(len(rows))]), c))
            tiles[ti, tj] += 1
            count[c] += 1
            continue
        i, j = spare[rng.integers(len(spare))]
        i = rows[i]
        tiles[ti, cols[i, j] // 16] -= 1
        count[cols[i, j]] -= 1
        cols[i, j] = c
        tiles[ti, tj] += 1
        count[c] += 1
    assert (tiles > 0).all() and (count > 0).all()
    return extra


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
                                "n r p_plus seed fill_tiles", defaults=(0,))
WarpCase = namedtuple("WarpCase", "name width row_len n spr r p_plus seed")


def net_kw(case):
    return dict(n_layers=case.n_layers, width=case.width, positions_dim=case.positions_dim, directions_dim=case.directions_dim,
                additional_input_dim=case.additional_input_dim, skips=list(case.skips),
                use_directional_input=case.use_directional_input)


def _state(rng, shapes, r, p_plus, fill_tiles=0):
    state = {}
    for name, n_out, n_in in shapes:
        state[name + ".weight"] = _dense_rows(rng, n_out, n_in, p_plus) if n_out <= 3 else \
            _sparse_rows(rng, n_out, n_in, r, p_plus, fill_tiles)
        state[name + ".bias"] = rng.integers(0, 3, n_out).astype(F32)
    return state


def render_net_data(case):
    """(state dict, encoded rows [n, positions + additional + directions], d_raw [n, 4]) as fp32 arrays of integers"""
    rng = np.random.default_rng([case.seed, case.width, case.n_layers, case.n])
    state = _state(rng, render_net_shapes(*case[1:8]), case.r, case.p_plus, case.fill_tiles)
    rows = rng.integers(-2, 3, (case.n, case.positions_dim + case.additional_input_dim + case.directions_dim)).astype(F32)
    d_raw = rng.integers(-2, 3, (case.n, 4)).astype(F32)
    if case.fill_tiles:
        _make_two_sided(case, state, rows, rng)
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


def _make_two_sided(case, state, rows, rng):
    """The inference cases, n >= 77: a hidden feature of a ReLU layer that the float64 forward finds active on every row or on none
    gets its signs (as many +1 as -1, on the same columns) and its bias (0 .. 2) drawn again, up to 32 times, until it is active on
    some row and inactive on another; layer by layer from the input, each on the inputs the layers before it now give.  In place."""
    if case.n < 77:
        return
    x, zero = rows.astype(np.float64), np.zeros((case.n, 4))
    for name in ["positions_pose_input"] + [f"positional_net.{i}" for i in range(case.n_layers - 1)] + ["directional_net.0"]:
        l = next(l for l in _render_layers(case, _f64(state), x, zero)[1] if l.name == name)
        on = l.z > 0
        for f in np.nonzero(on.all(0) | ~on.any(0))[0]:
            nz = np.nonzero(state[name + ".weight"][f])[0]
            for _ in range(32):
                signs = np.where(rng.permutation(len(nz)) < len(nz) // 2 + (rng.random() < 0.5) * (len(nz) % 2), 1.0, -1.0)
                bias = float(rng.integers(0, 3))
                z = l.a[:, nz] @ signs + bias
                if (z > 0).any() and (z <= 0).any():
                    state[name + ".weight"][f, nz], state[name + ".bias"][f] = signs, bias
                    break


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
         p_plus=0.5, seed=1, directions_dim=24, fill_tiles=0):
    return NetCase(name, n_layers, width, positions_dim, directions_dim, additional_input_dim, tuple(skips), use_directional_input, n, r,
                   p_plus, seed, fill_tiles)


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


# ================================================================================================ inference
# The cases of tests/test_gpu_mlp_infer_exact.py: the same integer networks through the no-grad entries.  Only forward sums count
# here (no sum crosses samples), so the bound has two orders of magnitude of headroom and the coverage conditions are about the
# forward: every 16 x 16 tile of every weight matrix holds an entry (fill_tiles: a skipped or mis-addressed tile changes an integer),
# every ReLU feature is seen on both sides, the outputs vary.  An InferCase names a net (a NetCase), the entry and the call's form:
#   entry "encoded": RenderRayNet.forward(rows), rows = render_net_data(net)[1];
#   entry "fused":   RenderRayNet.forward_fused with PositionalEncoder(0, True) twice (positions_dim = directions_dim = 3): integer
#                    positions, directions s * e_i (s in +-1, +-2, +-4: the kernels' sqrtf of an fp32 sum of squares and __fdiv_rn give
#                    exactly +-e_i, direction_premise()), per ray (spr samples each) or per sample, per-ray additional inputs in front
#                    of (add_first) or behind the position columns; mult: a multiplier on positions and additional inputs.
InferCase = namedtuple("InferCase", "name net entry spr per_sample add_first mult", defaults=(1, 0, 0, 1))


def _as_infer(base, **kw):
    """the shape and generator parameters of a case of the training tests, every weight tile occupied"""
    return base._replace(name="infer-" + base.name[len("net-"):], fill_tiles=1, **kw)


def _enc(net):
    return InferCase(net.name, net, "encoded")


def _fused(name, n, spr=1, per_sample=0, add_first=0, mult=1, **kw):
    net = _net("fused-" + name, n, positions_dim=3, directions_dim=3, fill_tiles=1, **kw)
    assert n % spr == 0
    return InferCase(net.name, net, "fused", spr, per_sample, add_first, mult)


INFER_DEFAULT = {n: _enc(_as_infer(NET_DEFAULT[n])) for n in (1, 77, 333, 1100)}
INFER_WIDTHS = [_enc(_as_infer(c)) for c in NET_WIDTHS] + [
    _enc(_net("infer-200x3-skip1", 333, n_layers=3, width=200, skips=(1,), fill_tiles=1)),          # padded inside 256
    _enc(_net("infer-384x2", 333, n_layers=2, width=384, skips=(), fill_tiles=1)),                   # one wave per SIMD: 320, 384,
    _enc(_net("infer-448x2-skip0", 333, n_layers=2, width=448, skips=(0,), fill_tiles=1)),           # 448, 512
    _enc(_net("infer-576x2-skip0-layered", 333, n_layers=2, width=576, skips=(0,), fill_tiles=1))]   # smpl_nerf_amd/layered.py
INFER_INPUTS = [_enc(_as_infer(c)) for c in NET_INPUTS]
INFER_CASES = [INFER_DEFAULT[n] for n in (1, 77, 333, 1100)] + INFER_WIDTHS + INFER_INPUTS
LAYERED = INFER_WIDTHS[-1]

FUSED_POOL = _fused("256x8-n1100", 1100)                          # the pool of rows of the launch forms (big_rows)
FUSED_RAYS = [_fused("256x8-ray4", 332, spr=4), _fused("256x8-ray24", 336, spr=24), _fused("256x8-sample4", 332, spr=4, per_sample=1)]
# the four forms of tests/test_gpu_infer_compose.NETS with per-ray additional inputs: 24 samples per ray fold, 4 do not
FUSED_ADD = [_fused("add69-first-fold", 336, spr=24, add_first=1, additional_input_dim=69),
             _fused("add69-last-fold", 336, spr=24, additional_input_dim=69),
             _fused("add69-first-nofold", 332, spr=4, add_first=1, additional_input_dim=69),
             _fused("add69-last-nofold", 332, spr=4, additional_input_dim=69)]
# the structures of tests/test_gpu_infer_compose.NETS (composed stream: widths up to 256) and the narrow widths of the throughput form
FUSED_NETS = [_fused("256x1", 333, n_layers=1, skips=()), _fused("256x2", 333, n_layers=2, skips=()),
              _fused("256x4-skip1", 333, n_layers=4, skips=(1,)), _fused("256x10-skips257", 333, n_layers=10, skips=(2, 5, 7)),
              _fused("256x8-nodir", 333, use_directional_input=0), _fused("64x8", 333, width=64), _fused("200x8", 333, width=200),
              _fused("128x4-skip1", 333, n_layers=4, width=128, skips=(1,))]
# (no fused cases above width 256: those kernels want at least 17 input columns in every layer - csrc/mlp_plan.h refuses the 3 of an
# identity-only encoder - so the widths 320 .. 512 are reached through the encoded entry, INFER_WIDTHS)
FUSED_CASES = [FUSED_POOL] + FUSED_RAYS + FUSED_ADD + FUSED_NETS
# split-precision inference (snerf_mlp_fwd_bf16_f32, width 256): per mode a case whose every layer input is at most 255 - its own first
# part in every mode - and one whose largest layer inputs need the mode's last part (split_premise(); the multiplier is the knob:
# 31 keeps every input inside two bf16 parts = 16 bits, 301 takes them past one fp16 part = 11 bits and keeps them inside two, 3001
# takes some past 2^16 and keeps every sum of absolute terms below 2^24)
SPLIT_FIRST = _fused("256x4-skip1-r3-first-part", 333, n_layers=4, skips=(1,), r=3)
SPLIT_LAST = {"bf16x3": _fused("256x8-x31", 333, mult=31), "bf16x6": _fused("256x8-x3001", 333, mult=3001),
              "f16x3": _fused("256x8-x301", 333, mult=301)}
SPLIT_MODES = {"bf16x3": (2, "bf16"), "bf16x6": (3, "bf16"), "f16x3": (2, "f16")}           # parts per operand, format
ALL_INFER_CASES = INFER_CASES + FUSED_CASES + [SPLIT_FIRST, SPLIT_LAST["bf16x3"], SPLIT_LAST["bf16x6"]]
# the warp net's no-grad entries: WARP_CASES through forward(rows); forward_fused at 4 samples per ray (no fold: the per-ray pose
# fold of csrc/warp.hip: warp_fold_bytes applies from 8 samples per ray) and at 8 (fold)
WARP_FUSED_FOLD = _warp(256, 43, 336, spr=8)
WARP_INFER_FUSED = [WARP_FUSED, WARP_FUSED_FOLD]


def direction_premise(d):
    """fp32, on the CPU, operation by operation as the kernels do it (csrc/mlp.hip: mlp_fwd_body; no fast-math anywhere in build.py):
    nrm = sqrtf((ux ux + uy uy) + uz uz), d / nrm.  Returns the normalised directions; for s * e_i they are exactly sign(s) e_i."""
    d = np.asarray(d, F32)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2], dtype=F32)
    return (d / nrm[:, None]).astype(F32)


def infer_data(case):
    """(state dict, inputs, rows): inputs = {"rows"} (encoded) or {"x" [n, 3], "d" [n or n / spr, 3], "add" [n / spr, A] or None};
    rows [n, positions + additional + directions] are the encoded rows the float64 reference evaluates"""
    net = case.net
    if case.entry == "encoded":
        state, rows, _ = render_net_data(net)
        return state, {"rows": rows}, rows
    rng = np.random.default_rng([net.seed, net.width, net.n_layers, net.n, case.spr, case.per_sample, case.add_first, 17])
    state = _state(rng, render_net_shapes(*net[1:8]), net.r, net.p_plus, net.fill_tiles)
    n, rays = net.n, net.n // case.spr
    x = (case.mult * rng.integers(-2, 3, (n, 3))).astype(F32)
    nd = n if case.per_sample else rays
    d = np.zeros((nd, 3), F32)
    d[np.arange(nd), rng.integers(0, 3, nd)] = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], nd)
    add = (case.mult * rng.integers(-2, 3, (rays, net.additional_input_dim))).astype(F32) if net.additional_input_dim else None
    per_sample = lambda v: v if len(v) == n else np.repeat(v, case.spr, 0)
    cols = [x] if add is None else [per_sample(add), x] if case.add_first else [x, per_sample(add)]
    rows = np.concatenate(cols + [per_sample(np.sign(d))], 1).astype(F32)
    _make_two_sided(net, state, rows, rng)
    return state, {"x": x, "d": d, "add": add}, rows


Composed = namedtuple("Composed", "sigma dnet rgb raw own_abs_sum entries")
InferRef = namedtuple("InferRef", "out layers composed")


def composed_maps(net, P):
    """mlp_compose_mid_kernel / mlp_compose_out_kernel (csrc/mlp.hip) restated in float64 numpy: sigma' = w_s W_a with bias
    w_s b_a + b_s; dir-net' = W_n [W_d[:, :W] W_a | W_d[:, W:]] with bias W_n (W_d[:, :W] b_a + b_d) + b_n.  Returns
    (sigma' weight, bias, dir-net' weight, bias, the largest sum of absolute terms of the composition's own sums)."""
    W, A = net.width, np.abs
    Wa, ba = P["additional_linear_layer.weight"], P["additional_linear_layer.bias"]
    ws, bs = P["sigma_out_layer.weight"], P["sigma_out_layer.bias"]
    Wd, bd = P["directional_input.weight"], P["directional_input.bias"]
    Wn, bn = P["directional_net.0.weight"], P["directional_net.0.bias"]
    Wd1, Wd2 = Wd[:, :W], Wd[:, W:]
    mid_w, mid_b = Wd1 @ Wa, Wd1 @ ba + bd
    own = [A(ws) @ A(Wa), A(ws) @ A(ba) + A(bs), A(Wd1) @ A(Wa), A(Wd1) @ A(ba) + A(bd), A(Wn) @ A(mid_w), A(Wn) @ A(Wd2),
           A(Wn) @ A(mid_b) + A(bn)]
    return (ws @ Wa, ws @ ba + bs, np.concatenate([Wn @ mid_w, Wn @ Wd2], 1), Wn @ mid_b + bn,
            max(float(v.max()) for v in own if v.size))


@functools.lru_cache(maxsize=None)
def infer_reference(case):
    """float64: raw of the UNCOMPOSED network on the case's rows (the numpy layers, checked against torch_ref.render_ray_net), every
    layer, and for widths up to 256 the same rows through the composed maps - which must give the same raw"""
    net = case.net
    state, _, rows = infer_data(case)
    P, x = _f64(state), rows.astype(np.float64)
    raw, layers, _, _ = _render_layers(net, P, x, np.zeros((net.n, 4)))
    with torch.no_grad():
        want = R.render_ray_net({k: torch.from_numpy(v) for k, v in P.items()}, torch.from_numpy(x),
                                **{k: (tuple(v) if k == "skips" else v) for k, v in net_kw(net).items() if k != "width"})
    assert np.array_equal(raw, want.numpy())
    composed = None
    if net.width <= 256:
        sw, sb, dw, db, own = composed_maps(net, P)
        h, dd = layers[net.n_layers - 1].out, x[:, x.shape[1] - net.directions_dim:]
        sigma = Layer("sigma'", h, sw, sb, False)
        dnet = Layer("dir-net'", np.concatenate([h, dd], 1) if net.use_directional_input else h, dw, db, True)
        rgb = Layer("rgb_out_layer", dnet.out, P["rgb_out_layer.weight"], P["rgb_out_layer.bias"], False)
        composed = Composed(sigma, dnet, rgb, np.concatenate([rgb.out, sigma.out], 1), own, [sw, sb, dw, db])
        assert np.array_equal(composed.raw, raw)
    return InferRef(raw, layers, composed)


def infer_preconditions(case):
    """Measured on the float64 reference alone:
      max_abs_sum:   the largest sum of absolute terms over every forward pre-activation, through the composed maps too, and over the
                     composition's own sums - below 2^24 every order is exact in fp32;
      composed_ok:   every composed entry and bias is an integer that fp32 holds;
      zero_preacts, relu_min, relu_max: as preconditions();
      one_sided:     hidden features of a ReLU layer that are active on every row or on none;
      empty_tiles:   origin-aligned 16 x 16 tiles without a non-zero over every weight matrix, the composed maps included;
      min_distinct:  the smallest number of distinct values one of the four output columns takes over the rows."""
    ref = infer_reference(case)
    m = dict(max_abs_sum=0.0, composed_ok=True, zero_preacts=0, relu_min=1.0, relu_max=0.0, one_sided=0, empty_tiles=0,
             min_distinct=min(len(np.unique(ref.out[:, j])) for j in range(4)), max_act=0.0)
    for l in ref.layers + (list(ref.composed[:3]) if ref.composed else []):
        m["max_abs_sum"] = max(m["max_abs_sum"], float(l.abs_fwd.max()))
        m["max_act"] = max(m["max_act"], float(np.abs(l.a).max()))
        m["empty_tiles"] += _tiles_without_nonzero(l.w)
    for l in ref.layers:
        if l.relu:
            on = l.z > 0
            m["relu_min"], m["relu_max"] = min(m["relu_min"], float(on.mean())), max(m["relu_max"], float(on.mean()))
            m["zero_preacts"] += int((l.z == 0).sum())
            m["one_sided"] += int((on.all(0) | ~on.any(0)).sum())
    if ref.composed:
        m["max_abs_sum"] = max(m["max_abs_sum"], ref.composed.own_abs_sum)
        m["composed_ok"] = all(np.array_equal(v, np.rint(v)) and np.abs(v).max() < INT_LIMIT for v in ref.composed.entries)
    return m


def assert_infer_preconditions(case):
    m, n = infer_preconditions(case), case.net.n
    assert m["max_abs_sum"] < INT_LIMIT and m["composed_ok"] and m["empty_tiles"] == 0 and m["zero_preacts"] >= 1, (case.name, m)
    assert n < 16 or (0.25 <= m["relu_min"] and m["relu_max"] <= 0.75), (case.name, m)
    assert n < 77 or (m["one_sided"] == 0 and m["min_distinct"] >= 8), (case.name, m)
    return m


def describe_infer(case):
    m = infer_preconditions(case)
    form = case.entry if case.entry == "encoded" else \
        f"fused spr {case.spr} {'per-sample' if case.per_sample else 'per-ray'} dirs" + (" add first" if case.add_first else "")
    return (f"{case.name:34s} {form:34s} max|act| {m['max_act']:8.0f}  largest sum of |terms| {m['max_abs_sum']:9.0f} "
            f"({m['max_abs_sum'] / INT_LIMIT:.5f} of 2^24)  composed {'integers' if infer_reference(case).composed else 'none':8s}  "
            f"empty tiles {m['empty_tiles']}  ReLU active {m['relu_min']:.3f} .. {m['relu_max']:.3f}  zero pre-activations "
            f"{m['zero_preacts']}  one-sided features {m['one_sided']}  distinct outputs >= {m['min_distinct']}")


def big_rows(case, n, seed):
    """A call of n samples made of the case's own rows (the pool): whole rays drawn with replacement.  Returns (inputs as
    infer_data gives them, index [n] into the pool's samples); no forward sum crosses samples, so the expected output is
    infer_reference(case).out[index]."""
    _, inputs, _ = infer_data(case)
    assert n % case.spr == 0
    pool_rays = case.net.n // case.spr
    ray = np.arange(pool_rays) if n == case.net.n else np.random.default_rng([seed, n]).integers(0, pool_rays, n // case.spr)
    idx = (ray[:, None] * case.spr + np.arange(case.spr)).ravel()
    if case.entry == "encoded":
        return {"rows": inputs["rows"][idx]}, idx
    return {"x": inputs["x"][idx], "d": inputs["d"][idx if case.per_sample else ray],
            "add": None if inputs["add"] is None else inputs["add"][ray]}, idx


# ---- which kernels a fused fp32 inference call of a width-256 net runs on (csrc/mlp_lat.hip: lat_lds, lat_split, lat_cost, lat_choose;
# csrc/mlp.hip: launch_fwd), restated the way wgrad_splits() restates the wgrad rule
def encoder_kblocks(freqs, identity):
    per_lane = (3 * identity + 3 * freqs + 3) // 4
    return (2 * per_lane + 3) // 4


def lat_limits(pos_nkb=1, dir_nkb=1, add_nkb=0):
    """(s_max, pair_s): the most 16-sample tiles per pass whose LDS fits 160 KiB, and the most of which two workgroups fit a CU"""
    pad = lambda k: -(-k // 4) * 4
    lds = lambda s: s * (2 * 16384 + (pad(pos_nkb + add_nkb) + pad(16 + dir_nkb) - 16) * 1024)
    s_max = max([s for s in (1, 2, 3, 4) if lds(s) <= 160 * 1024], default=0)
    return s_max, max([h for h in (1, 2) if 2 * lds(h) <= 160 * 1024], default=0)


def lat_split(n16, n_cu, s_max, pair_s=0, mixed_ok=False):
    """the launches of n16 tiles: dicts of kind ("single": one workgroup per CU; "paired": two of S tiles per CU; "mixed": a two-tile
    and a one-tile workgroup per CU), S, grid, passes, tile_off, tile_end"""
    out, done = [], 0
    S = min(s_max, -(-n16 // n_cu))
    per_round = S * n_cu
    passes = n16 // per_round

    def mixed(first, tiles):
        n_a = min(n_cu, tiles // 2)
        return dict(kind="mixed", S=3, grid=n_a + tiles - 2 * n_a, passes=1, tile_off=first, tile_end=first + tiles)
    if passes > 0:
        if passes == 1 and S % 2 == 0 and S // 2 <= pair_s:
            out.append(dict(kind="paired", S=S // 2, grid=2 * n_cu, passes=1, tile_off=0, tile_end=per_round))
        elif passes == 1 and S == 3 and mixed_ok and pair_s >= 2:
            out.append(mixed(0, per_round))
        else:
            out.append(dict(kind="single", S=S, grid=n_cu, passes=passes, tile_off=0, tile_end=per_round * passes))
        done = per_round * passes
    r = n16 - done
    if r > 0:
        S2 = min(s_max, -(-r // n_cu))
        if S2 == 3 and mixed_ok and pair_s >= 2:
            return out + [mixed(done, r)]
        kind = "single"
        if S2 % 2 == 0 and S2 // 2 <= pair_s:
            S2, kind = S2 // 2, "paired"
        out.append(dict(kind=kind, S=S2, grid=-(-r // S2), passes=1, tile_off=done, tile_end=n16))
    return out


def lat_cost(n16, n_cu, s_max, fixed=21.0, per_tile=41.0):
    return sum(fixed + q["passes"] * (4.0 + per_tile * q["S"]) for q in lat_split(n16, n_cu, s_max))


def lat_choose_infer(n, n_cu, s_max=4):
    """(mode, n_main) of lat_choose for inference: 0 the throughput kernel alone, 1 the latency kernels alone, 2 the throughput kernel
    on the first n_main samples - whole rounds of 128 samples per CU - and the latency kernels on the rest"""
    n16, per_round = (n + 15) // 16, 128 * n_cu
    t_best = 178.0 if n <= 64 * n_cu else -(-n // per_round) * 295.0
    best = (0, 0)
    if n16 <= 64 * n_cu:
        t = lat_cost(n16, n_cu, s_max)
        if t < t_best:
            t_best, best = t, (1, 0)
    rounds = n // per_round
    rem = n - rounds * per_round
    if 1 <= rounds <= 64 and rem > 0 and rounds * 295.0 + lat_cost((rem + 15) // 16, n_cu, s_max) < 0.98 * t_best:
        best = (2, rounds * per_round)
    return best


def launch_form(n, n_cu, lat=True):
    """what a fused fp32 inference call of n samples of a width-256 net with identity encoders and no additional inputs runs as:
    (mode, the kinds of the latency launches in order, throughput tile of 64 or 128 samples or 0)"""
    s_max, pair_s = lat_limits()
    mode, n_main = lat_choose_infer(n, n_cu, s_max) if lat else (0, 0)
    kinds = [q["kind"] for q in lat_split((n + 15) // 16 - n_main // 16, n_cu, s_max, pair_s, True)] if mode else []
    return mode, kinds, 0 if mode == 1 else 128 if mode == 2 or n > 64 * n_cu else 64


def lat_sizes(n_cu):
    """sizes that reach each branch of lat_split on n_cu compute units, derived from the count: [(label, n, kinds wanted)]"""
    c = n_cu
    return [("single", 1, ["single"]), ("single", 77, ["single"]), ("single", min(1100, 16 * c - 4), ["single"]),
            ("paired", 16 * 2 * c, ["paired"]), ("mixed", 16 * 3 * c, ["mixed"]),
            ("paired + remainder", 16 * (4 * c + 5), ["paired", "single"]), ("ragged mixed remainder", 16 * (2 * c + 3) - 5, ["mixed"])]


def hybrid_size(n_cu):
    return 128 * n_cu + 16 * n_cu - 7          # one throughput round and a ragged latency remainder of n_cu tiles


def throughput_sizes(n_cu):
    """[(label, n)] of the SNERF_LAT=0 child: 64-sample tiles, one 128-sample tile per workgroup, and a call in which every workgroup
    wraps its weight stream and the last tile is ragged"""
    return [("a ragged tile", 333), ("a ragged tile", 1100), ("one tile per workgroup", 128 * n_cu),
            ("wrapped, ragged", (2 * n_cu + 1) * 128 - 37)]


# ---- the operand split of the split-precision kernels (csrc/mlp_bf16_device.h: split_pair_into), restated
def _bf16_rne(v):
    b = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(F32)


def _f16_rtz(v):
    """fp16 by truncation (v_cvt_pkrtz_f16_f32): 11 significant bits, none below 2^-24; |v| < 2^16"""
    a = np.abs(np.asarray(v, np.float64))
    assert (a < 65536).all()
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    q = 2.0 ** np.maximum(e - 10, -24)
    return (np.sign(v) * np.floor(a / q) * q).astype(F32)


def split_parts(a, mode):
    """the parts of the B operand a [n, k] (float64 integers) as the mode's kernels form them, as float64 in a's own scale.
    bf16x3 / bf16x6: 2 / 3 bf16 parts, each the round-to-nearest-even bf16 of what the ones before leave (split_pair_into).  f16x3: the
    sample's row scaled by a power of two that takes its largest |value| - at least 1 where encoder or additional columns enter, as
    here in every layer that has any - into [2^14, 2^15) (operand_scale16, kx_pos), then 2 fp16 parts by truncation."""
    ns, fmt = SPLIT_MODES[mode]
    a = np.asarray(a, np.float64)
    scale = np.ones((a.shape[0], 1))
    if fmt == "f16":
        top = np.maximum(np.abs(a).max(1, keepdims=True), 1.0)
        scale = 2.0 ** (14 - np.floor(np.log2(top)))
    rest, parts = (a * scale).astype(F32), []
    assert np.array_equal(rest.astype(np.float64), a * scale)
    for _ in range(ns):
        p = _bf16_rne(rest) if fmt == "bf16" else _f16_rtz(rest)
        parts.append(p.astype(np.float64) / scale)
        rest = (rest - p).astype(F32)
    return parts


def split_premise(case, mode):
    """On the reference alone: does every layer input recombine exactly from the parts the mode keeps (weights of +-1 are their own
    first part, so every product weight x part is one of the cross terms the kernels form - mlp_bf16_device.h: Terms<2>, Terms<3>
    hold (A 0, B s) for every s); the share of non-zero layer inputs with a non-zero LAST part; the largest sum of absolute terms
    when each input enters as its parts"""
    ref = infer_reference(case)
    exact, last, total, abs_sum = True, 0, 0, 0.0
    for l in ref.layers:
        parts = split_parts(l.a, mode)
        exact = exact and np.array_equal(sum(parts), l.a)
        last += int((parts[-1] != 0).sum())
        total += int((l.a != 0).sum())
        abs_sum = max(abs_sum, float((sum(np.abs(p) for p in parts) @ np.abs(l.w).T + np.abs(l.b)).max()))
    return dict(exact=bool(exact), last_share=last / total, max_abs_sum=abs_sum)


INFER_PROFILE = os.path.join(ROOT, "profiles", "mlp_infer_exact_cases.txt")
INFER_PROFILE_HEAD = ("# tests/exact_net_ref.py: what the float64 reference of every case of tests/test_gpu_mlp_infer_exact.py measures (CPU;\n"
                      "# rewritten by `python tests/exact_net_ref.py`, compared by tests/test_exact_net_host.py).  Forward sums only.\n")


def _describe_split(mode, case):
    m, p = infer_preconditions(case), split_premise(case, mode)
    return (f"split {mode:7s} {case.name:34s} max|layer input| {m['max_act']:8.0f}  recombines exactly {p['exact']}  non-zero last part "
            f"{p['last_share']:.5f}  largest sum of |terms| over the parts {p['max_abs_sum']:9.0f}")


def infer_profile_text():
    return (INFER_PROFILE_HEAD + "".join(describe_infer(c) + "\n" for c in ALL_INFER_CASES) +
            "".join(_describe_split(mode, c) + "\n" for mode in SPLIT_MODES for c in (SPLIT_FIRST, SPLIT_LAST[mode])) +
            describe(WARP_FUSED_FOLD) + "\n")


# ================================================================================================ split precision: the low parts
# The cases of tests/test_gpu_mlp_split_exact.py.  In every case above a weight is +-1 - its own first part - so weight parts 1 and 2 of
# every stream are zeros, and in the training cases every operand is.  Here one layer l* of a net is "rich": its non-zero weights are
# +-q, q a constant that needs the mode's further parts (RICH_Q), and inputs / output gradients may be multiples of a two-part constant
# (TWO_PART_Q).  Every other layer is a signed selection - one +-1 per row, every input column used by about as many rows as any other
# (the 1- and 3-row heads: HEAD_ENTRIES per row) - so values do not grow on the way forward or back.  A weight gradient sums over the
# samples: with a q of 18 bits (or 257 x 257) it is q times a sum that has to stay below 2^24 / q = 127 (254), so in those families
# only every g_every-th sample has a non-zero output gradient.  Every sum of absolute part-products then stays below 2^24
# (rich_premises()).  Width 256, the fused entry with PositionalEncoder(0, True) twice, as SPLIT_FIRST / SPLIT_LAST.
#
# Restated from the kernels (smpl_nerf_amd/csrc), not guessed:
#   TERMS                  mlp_bf16_device.h: Terms<2>, Terms<3> - (A part, B part) of the products a mode forms.  Forward and dgrad
#                          (mlp_bf16.hip, mlp_train_bf16.hip: mlp_bwd_bf16_kernel): A = the weights, B = the layer input / d Y;
#                          wgrad (mlp_wgrad_bf16_kernel, mlp_wgrad_f16_kernel, mlp_wgrad_direct_f16_kernel): A = d Y, B = X;
#   weight_parts()         mlp_pack_bf16_kernel / mlp_pack_t_bf16_kernel: bf16 parts by round-to-nearest-even; f16x3: the whole layer
#                          times 2^we, we = min(14 - exponent of its largest |w|, 50) (layer_weight_exp), then two fp16 parts, both by
#                          round-to-nearest-even (the pack kernels cast; only the OPERANDS are truncated);
#   split_parts(a, mode)   forward and dgrad operands: per sample, operand_scale16(sample_exp16(..)) with the cap where input columns
#                          enter (kx_pos, KX_PE) - on integers min(14 - e, cap) is 14 - exponent of max(largest |value| of the row, 1)
#                          in the forward (cap 64) and in the dgrad (cap 40) alike;
#   split_parts(a, mode, stat_exp)   wgrad operands: bf16 parts of X and d Y as they are; f16x3: times 2^(14 - stat_exp), stat_exp
#                          the exponent of the largest value over ALL samples (wgrad_f16_scales; wgrad_stat_exps(): the hidden input
#                          of the layer, max(1, largest |position|) for position columns - layer 0 has no hidden input and reads that
#                          one too - 0 for direction columns, the largest |d Y_l|), clamped to +-100;
#   wgrad_is_wide()        mlp_wgrad_jobs.h: wgrad_wide - at least 8 output tiles and 16 input k-blocks of 16 columns.  In the bf16 modes
#                          the narrow jobs run the fp32 kernels (launch_wgrad), in f16x3 the two-part direct kernel; nothing is folded;
#   the sigma head's share of d o is an fp32 product of fp32 values in every mode (mlp_bwd_bf16_kernel: the aux block).
TERMS = {2: ((1, 0), (0, 1), (0, 0)), 3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))}
# q of the rich layer.  Three bf16 parts: 131329 = 2^17 + 2^8 + 1 is the smallest integer that has three under round-to-nearest-even.
# 65793 = 2^16 + 2^8 + 1 - the constant first proposed for these cases - has two, 66048 - 255 (the remainder 257 is above half a unit of
# 512; below 2^17 at most 256 is left behind the first part, which fits 8 bits): it is kept as a family of its own, W65793, whose second
# part is negative.
RICH_Q = {"bf16x3": 257, "bf16x6": 131329, "f16x3": 2049}         # 256 + 1; 131072 + 256 + 1; 2048 + 1
TWO_PART_Q = {"bf16x3": 257, "bf16x6": 257, "f16x3": 2049}
HEAD_ENTRIES = 16
RichCase = namedtuple("RichCase", "name mode family net rich q x_mult g_mult g_every")
RichWarpCase = namedtuple("RichWarpCase", "name mode family warp rich q x_mult")


def _selection(rng, n_out, n_in, width, k):
    """[n_out, k] column indices, distinct within a row: consecutive runs of k of a cyclic order of the columns - the columns behind
    the hidden ones (the input columns of a skip layer, the directions) first, then the hidden ones at random - dealt to the rows at random"""
    hidden = min(width, n_in)
    pool = np.resize(np.concatenate([np.arange(hidden, n_in), rng.permutation(hidden)]), n_out * k).reshape(n_out, k)
    return pool[rng.permutation(n_out)]


def _rich_layer(rng, name, n_out, a, width, q, relu):
    """(weight, bias) of one layer for the input a [n, n_in] (float64) it will see.
      a selection layer: one +-1 per row; where a ReLU follows, the pre-activation is a - min(a) or max(a) - a over the rows of the
        selected column a: exactly zero (inactive) where a is at that end and active elsewhere, so a feature is two-sided wherever its
        column varies, values do not grow, and a multiple of a two- or three-part constant stays one; elsewhere the bias is in 0 .. 2;
      a head (1 or 3 rows): HEAD_ENTRIES entries per row;
      the rich layer (q > 1): two entries per row, (+q, -q) with a bias in 0 .. 2 where a ReLU follows - a feature that is active on
        every row or on none gets its two columns drawn again, up to 256 times - the heads HEAD_ENTRIES entries +-q."""
    n_in, head = a.shape[1], n_out <= 3
    k = min(n_in, HEAD_ENTRIES if head else 2 if q > 1 else 1)
    cols = _selection(rng, n_out, n_in, width, k)
    signs = np.where(rng.random((n_out, k)) < 0.5, 1.0, -1.0)
    bias = rng.integers(0, 3, n_out).astype(np.float64)
    if relu and q > 1:
        signs = np.tile([1.0, -1.0], (n_out, 1))
        for f in range(n_out):
            for _ in range(256):
                z = q * (a[:, cols[f, 0]] - a[:, cols[f, 1]]) + bias[f]
                if (z > 0).any() and (z <= 0).any():
                    break
                cols[f] = rng.choice(n_in, 2, replace=False)
    elif relu:
        sel = a[:, cols[:, 0]]
        bias = -signs[:, 0] * np.where(signs[:, 0] > 0, sel.min(0), sel.max(0))
    w = np.zeros((n_out, n_in), F32)
    w[np.arange(n_out)[:, None], cols] = signs * q
    return w, bias.astype(F32)


def _rich_state(rng, net, rich, q, rows):
    """the layers in forward order, each made for the input the ones before it give on `rows` (float64)"""
    W, nh = net.width, net.n_layers - 1
    pp, dd = rows[:, :3], rows[:, 3:]
    state, out = {}, {}

    def make(name, n_out, a, relu):
        w, b = _rich_layer(rng, name, n_out, a, W, q if name == rich else 1, relu)
        state[name + ".weight"], state[name + ".bias"] = w, b
        z = a @ w.astype(np.float64).T + b
        return np.maximum(z, 0.0) if relu else z
    h = make("positions_pose_input", W, pp, True)
    for i in range(nh):
        h = make(f"positional_net.{i}", W, np.concatenate([h, pp], 1) if i in net.skips else h, True)
    o = make("additional_linear_layer", W, h, False)
    make("sigma_out_layer", 1, o, False)
    h1 = make("directional_input", W // 2, np.concatenate([o, dd], 1), False)
    h2 = make("directional_net.0", W // 2, h1, True)
    make("rgb_out_layer", 3, h2, False)
    return {k + s: state[k + s] for k, _, _ in render_net_shapes(*net[1:8]) for s in (".weight", ".bias")}


@functools.lru_cache(maxsize=None)
def rich_data(case):
    """(state dict, inputs {"x" [n, 3], "d" [n, 3], "add": None}, rows [n, 6], d_raw [n, 4]): positions in -1 .. 1 times x_mult,
    directions s e_i (one ray per sample), output gradients in -1 .. 1 times g_mult on every g_every-th sample and zero on the others"""
    net = case.net
    shapes = render_net_shapes(*net[1:8])
    rich = [n for n, _, _ in shapes].index(case.rich) if case.rich else 99
    rng = np.random.default_rng([net.seed, net.n_layers, net.n, rich, case.q, case.x_mult, case.g_mult, case.g_every, 23])
    n = net.n
    x = (case.x_mult * rng.integers(-1, 2, (n, 3))).astype(F32)
    d = np.zeros((n, 3), F32)
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], n)
    rows = np.concatenate([x, np.sign(d)], 1).astype(F32)
    d_raw = (case.g_mult * rng.integers(-1, 2, (n, 4))).astype(F32)
    d_raw[np.arange(n) % case.g_every != case.g_every // 2] = 0
    state = _rich_state(rng, net, case.rich, case.q, rows.astype(np.float64))
    return state, {"x": x, "d": d, "add": None}, rows, d_raw


@functools.lru_cache(maxsize=None)
def rich_reference(case):
    """float64: raw, parameter gradients of loss = sum(raw * d_raw) from torch_ref.render_ray_net under autograd, and the layers"""
    net = case.net
    state, _, rows, d_raw = rich_data(case)
    P = {k: torch.from_numpy(v).double().requires_grad_() for k, v in state.items()}
    x = torch.from_numpy(rows).double()
    raw = R.render_ray_net(P, x, **{k: (tuple(v) if k == "skips" else v) for k, v in net_kw(net).items() if k != "width"})
    (raw * torch.from_numpy(d_raw).double()).sum().backward()
    grads = {k: v.grad.numpy() for k, v in P.items()}
    raw_np, layers, d_rows, abs_rows = _render_layers(net, _f64(state), rows.astype(np.float64), d_raw.astype(np.float64))
    assert np.array_equal(raw_np, raw.detach().numpy())
    for l in layers:
        assert np.array_equal(l.dw, grads[l.name + ".weight"]) and np.array_equal(l.db, grads[l.name + ".bias"]), l.name
    return Reference(raw.detach().numpy(), grads, d_rows, layers, {})


def _exponent(v):
    """floor(log2 v) of the largest |entry| of v, or None if v is all zeros"""
    top = float(np.abs(v).max()) if np.size(v) else 0.0
    return int(np.frexp(top)[1]) - 1 if top > 0 else None


def weight_parts(w, mode):
    """the parts of a whole layer's weights w [n_out, n_in] as the pack kernels form them, float64 in w's own scale"""
    ns, fmt = SPLIT_MODES[mode]
    w = np.asarray(w, np.float64)
    rest = w.astype(F32)
    assert np.array_equal(rest.astype(np.float64), w)
    if fmt == "bf16":
        parts = []
        for _ in range(ns):
            p = _bf16_rne(rest)
            parts.append(p.astype(np.float64))
            rest = (rest - p).astype(F32)
        return parts
    e = _exponent(w)
    we = 0 if e is None else min(14 - e, 50)
    ws = (w * 2.0 ** we).astype(F32)
    assert np.array_equal(ws.astype(np.float64), w * 2.0 ** we) and np.abs(ws).max() < 65520
    h0 = ws.astype(np.float16).astype(F32)                   # (numpy casts to fp16 by round-to-nearest-even, as the pack kernels do)
    h1 = (ws - h0).astype(F32).astype(np.float16).astype(F32)
    return [h0.astype(np.float64) / 2.0 ** we, h1.astype(np.float64) / 2.0 ** we]


def operand_parts(a, mode, stat_exp=None):
    """split_parts() with the wgrad's scale: f16x3 and stat_exp given - the exponent of the job's largest value over all samples, None
    if there is none (the statistic is then never raised: clamped to -100) - one scale 2^(14 - stat_exp) for every sample"""
    ns, fmt = SPLIT_MODES[mode]
    if fmt == "bf16" or stat_exp is None:
        return split_parts(a, mode)
    a = np.asarray(a, np.float64)
    scale = 2.0 ** (14 - min(max(stat_exp, -100), 100))
    rest, parts = (a * scale).astype(F32), []
    assert np.array_equal(rest.astype(np.float64), a * scale)
    for _ in range(ns):
        p = _f16_rtz(rest)
        parts.append(p.astype(np.float64) / scale)
        rest = (rest - p).astype(F32)
    return parts


def wgrad_is_wide(n_out, n_cols):
    return -(-n_out // 16) >= 8 and -(-n_cols // 16) >= 16


class _Emulation:
    """the GEMMs of one forward + backward in float64, each the sum over the mode's terms of the restated parts; drop = (kind, term)
    leaves that term out of every GEMM of that kind ("fwd", "dgrad", "wgrad").  self.gemms records every GEMM for premises()."""

    def __init__(self, mode, drop=None):
        self.mode, self.ns, self.drop, self.gemms = mode, SPLIT_MODES[mode][0], drop, []

    def split(self, kind, layer, A, B, Ap, Bp, bias=None, job=None):
        """sum over the terms of A_i B_j^T, A [m, k] (weights; d Y^T in the wgrad), B [p, k] -> [m, p]"""
        out = sum(Ap[i] @ Bp[j].T for i, j in TERMS[self.ns] if self.drop != (kind, (i, j)))
        self.gemms.append(dict(kind=kind, layer=layer, job=job, split=True, A=A, B=B, Ap=Ap, Bp=Bp, bias=bias))
        return out if not np.isscalar(out) else np.zeros((A.shape[0], B.shape[0]))

    def fp32(self, kind, layer, A, B, bias=None, job=None):
        """a GEMM the mode leaves to fp32 arithmetic: one product per term"""
        self.gemms.append(dict(kind=kind, layer=layer, job=job, split=False, A=A, B=B, Ap=[A], Bp=[B], bias=bias))
        return A @ B.T


def _as_fp32(what, v):
    assert np.array_equal(v.astype(F32).astype(np.float64), v) and np.abs(v).max(initial=0) < INT_LIMIT, f"{what}: not an fp32 integer"
    return v


def split_emulate(case, mode, drop=None):
    """What the split kernels of `mode` compute on the case, if the restatement above is theirs: (raw, parameter gradients by
    state-dict name, the emulation with its GEMMs).  Every accumulator is checked to be an integer fp32 holds."""
    net = case.net
    state, _, rows, d_raw = rich_data(case)
    P, x, g_raw = _f64(state), rows.astype(np.float64), d_raw.astype(np.float64)
    W, nh, fmt = net.width, net.n_layers - 1, SPLIT_MODES[mode][1]
    pp, dd = x[:, :3], x[:, 3:]
    E = _Emulation(mode, drop)
    wp = {name: weight_parts(P[name + ".weight"], mode) for name, _, _ in render_net_shapes(*net[1:8])}
    relu = lambda z: np.maximum(z, 0.0)
    saved = {}                                               # name -> (layer input, pre-activation)

    def fwd(name, a):
        z = _as_fp32(name, E.split("fwd", name, P[name + ".weight"], a, wp[name], split_parts(a, mode), P[name + ".bias"]).T +
                     P[name + ".bias"])
        saved[name] = (a, z)
        return z
    h = relu(fwd("positions_pose_input", pp))
    for i in range(nh):
        h = relu(fwd(f"positional_net.{i}", np.concatenate([h, pp], 1) if i in net.skips else h))
    o = fwd("additional_linear_layer", h)
    sigma = fwd("sigma_out_layer", o)
    h1 = fwd("directional_input", np.concatenate([o, dd], 1))
    h2 = relu(fwd("directional_net.0", h1))
    raw = np.concatenate([fwd("rgb_out_layer", h2), sigma], 1)

    def dgrad(name, dz):                                     # d (hidden input) = d Y W[:, :W]
        Wt = P[name + ".weight"][:, :W].T
        return _as_fp32("d " + name, E.split("dgrad", name, Wt, dz, [p[:, :W].T for p in wp[name]], split_parts(dz, mode)).T)
    dY = {"rgb_out_layer": g_raw[:, :3], "sigma_out_layer": g_raw[:, 3:]}
    dY["directional_net.0"] = np.where(saved["directional_net.0"][1] > 0, dgrad("rgb_out_layer", dY["rgb_out_layer"]), 0.0)
    dY["directional_input"] = dgrad("directional_net.0", dY["directional_net.0"])
    dY["additional_linear_layer"] = _as_fp32("d o", dgrad("directional_input", dY["directional_input"]) + E.fp32(
        "dgrad", "sigma_out_layer", P["sigma_out_layer.weight"].T, dY["sigma_out_layer"]).T)
    g = dgrad("additional_linear_layer", dY["additional_linear_layer"])
    for i in range(nh - 1, -1, -1):
        dY[f"positional_net.{i}"] = np.where(saved[f"positional_net.{i}"][1] > 0, g, 0.0)
        g = dgrad(f"positional_net.{i}", dY[f"positional_net.{i}"])
    dY["positions_pose_input"] = np.where(saved["positions_pose_input"][1] > 0, g, 0.0)

    grads = {}
    for name, n_out, n_in in render_net_shapes(*net[1:8]):
        a, dz = saved[name][0], dY[name]
        dw = np.zeros((n_out, n_in))
        if name == "positions_pose_input":
            segs = [(0, n_in, "pos")]
        elif n_in > W:                                       # a skip layer, directional_input: the input columns are a pair of their own
            segs = [(0, W, "hidden"), (W, n_in, "dir" if name == "directional_input" else "pos")]
        else:
            segs = [(0, n_in, "hidden")]
        for c0, c1, typ in segs:
            job = "wide" if wgrad_is_wide(n_out, c1 - c0) else "narrow"
            if fmt == "bf16" and job == "narrow":
                dw[:, c0:c1] = E.fp32("wgrad", name, dz.T, a[:, c0:c1].T, job=job)
                continue
            ex = {"hidden": _exponent(a[:, c0:c1]), "pos": _exponent(np.maximum(np.abs(pp), 1.0)), "dir": 0}[typ]
            ex, ey = (-100 if ex is None else ex), (-100 if _exponent(dz) is None else _exponent(dz))
            dw[:, c0:c1] = E.split("wgrad", name, dz.T, a[:, c0:c1].T, [p.T for p in operand_parts(dz, mode, ey)],
                                   [p.T for p in operand_parts(a[:, c0:c1], mode, ex)], job=job)
        E.fp32("bias", name, np.ones((1, dz.shape[0])), dz.T)
        grads[name + ".weight"], grads[name + ".bias"] = _as_fp32("d " + name + ".weight", dw), _as_fp32("d " + name + ".bias", dz.sum(0))
    return raw, grads, E


def _gemm_figures(gemms, ns, rich):
    """(a), (b), (c) over recorded GEMMs: figures as rich_premises() returns them"""
    m = dict(max_operand=0.0, max_abs_sum=0.0, last_a=[0, 0], last_b=[0, 0], covered=set(), exact=True, outside=0)
    for g in gemms:
        A, B, Ap, Bp = g["A"], g["B"], g["Ap"], g["Bp"]
        m["max_operand"] = max(m["max_operand"], float(np.abs(A).max(initial=0)), float(np.abs(B).max(initial=0)))
        total = np.abs(g["bias"])[:, None] if g["bias"] is not None else 0.0
        if not g["split"]:
            m["max_abs_sum"] = max(m["max_abs_sum"], float((np.abs(A) @ np.abs(B).T + total).max()))
            continue
        m["exact"] = m["exact"] and np.array_equal(sum(Ap), A) and np.array_equal(sum(Bp), B) and \
            all(np.array_equal(p, np.rint(p)) for p in Ap + Bp)
        for key, parts, full in (("last_a", Ap, A), ("last_b", Bp, B)):
            m[key][0] += int((parts[-1] != 0).sum())
            m[key][1] += int((full != 0).sum())
        any_a, any_b = [p.any() for p in Ap], [p.any() for p in Bp]
        where = "l*" if g["layer"] == rich else "elsewhere"
        for i in range(ns):
            for j in range(ns):
                if not (any_a[i] and any_b[j]):
                    continue
                prod = np.abs(Ap[i]) @ np.abs(Bp[j]).T
                if not prod.any():
                    continue
                if (i, j) in TERMS[ns]:
                    total = total + prod
                    m["covered"].add((g["kind"], g["job"], where, (i, j)))
                else:
                    m["outside"] += 1
        m["max_abs_sum"] = max(m["max_abs_sum"], float(np.max(total)))
    m["last_a"], m["last_b"] = (v[0] / max(v[1], 1) for v in (m["last_a"], m["last_b"]))
    return m


@functools.lru_cache(maxsize=None)
def rich_premises(case, mode=None):
    """Conditions (a) - (e) of the split-precision cases, on the float64 reference alone: the emulation's GEMMs are evaluated with no
    term dropped, and every operand of every GEMM must be the reference's own (so nothing below depends on an emulated value).
      (a) every operand of a split GEMM recombines exactly from the parts the mode keeps, and every part is an integer;
      (b) every product (A part i) x (B part j) outside the mode's term table is zero;
      (c) the sum of the absolute part-products (and the bias) of every output element is below 2^24 - the parts are integers, so
          the lowest set bit among the terms is at least 1 and this is the stricter form of the bound;
      (e) a ReLU pre-activation is exactly zero somewhere, and every feature of a rich ReLU layer is active on some row and inactive
          on another.
    Returns the figures: largest operand, share of non-zero last parts on either side over the split GEMMs, the largest sum of (c), the
    terms with a non-zero product as (kind, wgrad job, at the rich layer or elsewhere, term), and whether the sum over the kept terms of the
    restated parts is the float64 reference (the first half of (f))."""
    mode = mode or case.mode
    if isinstance(case, RichWarpCase):
        raw, E, ref = warp_split_emulate(case)
        m = _gemm_figures(E.gemms, 3, case.rich)
        z1 = ref["z1"]
        m["zero_preacts"] = int((z1 == 0).sum())
        m["one_sided"] = int(((z1 > 0).all(0) | ~(z1 > 0).any(0)).sum()) if case.rich == "linear1" else 0
        m["emulation_is_float64"] = bool(all(np.array_equal(raw[k], ref[k]) for k in raw))
        m["max_abs_sum"] = max(m["max_abs_sum"], ref["abs_sdirs"])
        return m
    ref = rich_reference(case)
    raw, grads, E = split_emulate(case, mode)
    by_name, W = {l.name: l for l in ref.layers}, case.net.width
    for g in E.gemms:
        l, A, B = by_name[g["layer"]], g["A"], g["B"]
        if g["kind"] == "fwd":
            assert np.array_equal(A, l.w) and np.array_equal(B, l.a), (case.name, g["layer"], "forward operands")
        elif g["kind"] == "dgrad":
            assert np.array_equal(A, l.w[:, :W].T) and np.array_equal(B, l.dz), (case.name, g["layer"], "dgrad operands")
        else:
            assert np.array_equal(A if g["kind"] == "wgrad" else B, l.dz.T), (case.name, g["layer"], "wgrad operands")
    m = _gemm_figures(E.gemms, SPLIT_MODES[mode][0], case.rich)
    m["zero_preacts"], m["one_sided"] = 0, 0
    for l in ref.layers:
        if l.relu:
            m["zero_preacts"] += int((l.z == 0).sum())
            if l.name == case.rich:
                on = l.z > 0
                m["one_sided"] = int((on.all(0) | ~on.any(0)).sum())
    m["emulation_is_float64"] = bool(np.array_equal(raw, ref.out) and all(np.array_equal(grads[k], ref.grads[k]) for k in ref.grads))
    return m


# ---- the warp net's split forward (warp_bf16.hip: always three bf16 parts, no scaling): linear1 on [x | pose of the ray], linear2
@functools.lru_cache(maxsize=None)
def rich_warp_data(case):
    """(state dict, (x [n, 3], pose [rays, row_len - 3], o [rays, 3])): integers in -1 .. 1, x and pose times x_mult"""
    wc = case.warp
    rich = {"linear1": 1, "linear2": 2}[case.rich]
    rng = np.random.default_rng([wc.seed, wc.row_len, wc.n, rich, case.q, case.x_mult, 29])
    rays = wc.n // wc.spr
    x = (case.x_mult * rng.integers(-1, 2, (wc.n, 3))).astype(F32)
    pose = (case.x_mult * rng.integers(-1, 2, (rays, wc.row_len - 3))).astype(F32)
    o = rng.integers(-1, 2, (rays, 3)).astype(F32)
    rows = np.concatenate([x, np.repeat(pose, wc.spr, 0)], 1).astype(np.float64)
    w1, b1 = _rich_layer(rng, "linear1", wc.width, rows, wc.row_len, case.q if rich == 1 else 1, True)
    h = np.maximum(rows @ w1.astype(np.float64).T + b1, 0.0)
    w2, b2 = _rich_layer(rng, "linear2", 3, h, wc.width, case.q if rich == 2 else 1, False)
    return {"linear1.weight": w1, "linear1.bias": b1, "linear2.weight": w2, "linear2.bias": b2}, (x, pose, o)


def warp_split_emulate(case, ns=3, drop=None):
    """({warp, warped, sdirs} of the emulation with ns bf16 parts, the emulation, the float64 reference with z1 and abs_sdirs)"""
    wc, mode = case.warp, {3: "bf16x6", 2: "bf16x3"}[ns]
    state, (x, pose, o) = rich_warp_data(case)
    P = _f64(state)
    x64, o64 = x.astype(np.float64), np.repeat(o, wc.spr, 0).astype(np.float64)
    rows = np.concatenate([x64, np.repeat(pose, wc.spr, 0).astype(np.float64)], 1)
    E = _Emulation(mode, drop)
    out = {}
    a = rows
    for name in ("linear1", "linear2"):
        z = _as_fp32(name, E.split("fwd", name, P[name + ".weight"], a, weight_parts(P[name + ".weight"], mode), split_parts(a, mode),
                                   P[name + ".bias"]).T + P[name + ".bias"])
        a = np.maximum(z, 0.0)
    out["warp"] = z
    out["warped"] = _as_fp32("warped", x64 + z)
    out["sdirs"] = _as_fp32("sdirs", out["warped"] - o64)
    z1 = rows @ P["linear1.weight"].T + P["linear1.bias"]
    warp = np.maximum(z1, 0.0) @ P["linear2.weight"].T + P["linear2.bias"]
    ref = dict(warp=warp, warped=x64 + warp, sdirs=x64 + warp - o64, z1=z1,
               abs_sdirs=float((np.abs(x64) + np.abs(np.maximum(z1, 0.0)) @ np.abs(P["linear2.weight"]).T + np.abs(P["linear2.bias"]) +
                                np.abs(o64)).max()))
    return out, E, ref


def assert_rich_premises(case):
    m = rich_premises(case)
    assert m["exact"], (case.name, "(a): an operand does not recombine from the parts the mode keeps")
    assert m["outside"] == 0, (case.name, "(b): a product outside the mode's term table is non-zero", m["outside"])
    assert m["max_abs_sum"] < INT_LIMIT, (case.name, "(c)", m["max_abs_sum"])
    assert m["zero_preacts"] >= 1 and m["one_sided"] == 0, (case.name, "(e)", m["zero_preacts"], m["one_sided"])
    assert m["emulation_is_float64"], (case.name, "(f): the sum over the kept terms is not the float64 reference")
    return m


# (d) the terms a family is named for.  RICH_AT_LSTAR: non-zero in the GEMM of the rich layer itself, in every case of the family
# (positions_pose_input has no dgrad: no input gradients here).  rich_over_sweep(): non-zero in some case of the family's sweep, as
# (kind, wgrad job, term); the narrow wgrad jobs are split in f16x3 only (in the bf16 modes they run the fp32 kernels).
RICH_AT_LSTAR = {"W3": {"fwd": ((1, 0), (2, 0)), "dgrad": ((1, 0), (2, 0))}, "W65793": {"fwd": ((1, 0),), "dgrad": ((1, 0),)}, "W2X2": {"fwd": ((1, 1),)}, "W2G2": {"dgrad": ((1, 1),)},
                 "W2": {"fwd": ((1, 0),), "dgrad": ((1, 0),)}}


def rich_over_sweep(mode, family):
    narrow = lambda *terms: [("wgrad", "narrow", t) for t in terms] if mode == "f16x3" else []
    return {"W3": [("fwd", None, (0, 2)), ("dgrad", None, (0, 2)), ("wgrad", "wide", (1, 0)), ("wgrad", "wide", (2, 0)), ("wgrad", "wide", (0, 2))],
            "W65793": [("fwd", None, (0, 1)), ("dgrad", None, (0, 1)), ("wgrad", "wide", (1, 0)), ("wgrad", "wide", (0, 1))],
            "W2X2": [("wgrad", "wide", (1, 1))], "W2G2": [("wgrad", "wide", (1, 1))],
            "G2X2": [("fwd", None, (0, 1)), ("dgrad", None, (0, 1)), ("wgrad", "wide", (1, 1))],
            "W2": [("wgrad", "wide", (1, 0))] + narrow((1, 0)),
            "X2": [("fwd", None, (0, 1)), ("wgrad", "wide", (0, 1))] + narrow((0, 1)),
            "G2": [("dgrad", None, (0, 1)), ("wgrad", "wide", (1, 0))] + narrow((1, 0))}[family]


# (f) the family in which the emulation must leave the float64 reference when (kind, term) is dropped from it
RICH_SENSITIVE = {3: {("fwd", (1, 1)): "W2X2", ("dgrad", (1, 1)): "W2G2", ("wgrad", (1, 1)): "G2X2", ("fwd", (0, 1)): "G2X2",
                      ("dgrad", (0, 1)): "G2X2", ("wgrad", (0, 1)): "G2X2"},
                  2: {("fwd", (1, 0)): "W2", ("dgrad", (1, 0)): "W2", ("wgrad", (1, 0)): "G2", ("fwd", (0, 1)): "X2", ("dgrad", (0, 1)): "G2",
                      ("wgrad", (0, 1)): "X2", ("fwd", (0, 0)): "W2", ("dgrad", (0, 0)): "W2", ("wgrad", (0, 0)): "W2"}}
RICH_SENSITIVE[3].update({(kind, t): "W3" for kind in ("fwd", "dgrad", "wgrad") for t in ((2, 0), (1, 0), (0, 2), (0, 0))})


def emulation_is_reference(case, mode, drop=None):
    ref = rich_reference(case)
    raw, grads, _ = split_emulate(case, mode, drop)
    return bool(np.array_equal(raw, ref.out) and all(np.array_equal(grads[k], ref.grads[k]) for k in ref.grads))


def _rich_net(n, n_layers=8, skips=(4,)):
    return _net(f"rich-256x{n_layers}-n{n}", n, n_layers=n_layers, positions_dim=3, directions_dim=3, skips=skips)


# l* over layers that land in different kernels or jobs: input columns (a narrow wgrad job), a hidden layer before the skip and the
# skip layer (wide jobs, the concatenated operand), additional_linear_layer, directional_input (the hidden columns ride with the
# direction columns and, in the dgrad, with the sigma head's row), directional_net.0 (the 128 x 128 narrow job), rgb_out_layer; n = 333
# and 77 in turn.  And a 4-layer net with skip 1 whose rich layer is the skip layer.
RICH_SWEEP = [("positions_pose_input", 333, 8), ("positional_net.1", 77, 8), ("positional_net.4", 333, 8),
              ("additional_linear_layer", 77, 8), ("directional_input", 333, 8), ("directional_net.0", 77, 8), ("rgb_out_layer", 333, 8),
              ("positional_net.1", 77, 4)]


def _rich_case(mode, family, rich, n, n_layers, q=1, x_mult=1, g_mult=1, g_every=1):
    net = _rich_net(n, n_layers, (4,) if n_layers == 8 else (1,))
    name = f"{mode}-{family}-{rich or 'none'}-x{n_layers}-n{n}"
    return RichCase(name, mode, family, net, rich, q if rich else 1, x_mult, g_mult, g_every)


def _family(mode, family, sweep=RICH_SWEEP, **kw):
    return [_rich_case(mode, family, rich, n, depth, **kw) for rich, n, depth in sweep]


_NO_RICH = [(None, 77, 8), (None, 333, 8)]
_SHORT = [RICH_SWEEP[1], RICH_SWEEP[4], RICH_SWEEP[5]]
RICH_CASES = {
    "bf16x6": _family("bf16x6", "W3", q=131329, g_every=16) + _family("bf16x6", "W65793", q=65793, g_every=16) + _family("bf16x6", "W2X2", q=257, x_mult=257, g_every=4) +
    _family("bf16x6", "W2G2", _SHORT, q=257, g_mult=257, g_every=8) + _family("bf16x6", "G2X2", _NO_RICH, x_mult=257, g_mult=257, g_every=4),
    "bf16x3": _family("bf16x3", "W2", q=257) + _family("bf16x3", "X2", _NO_RICH, x_mult=257) + _family("bf16x3", "G2", _NO_RICH, g_mult=257),
    "f16x3": _family("f16x3", "W2", q=2049) + _family("f16x3", "X2", _NO_RICH, x_mult=2049) + _family("f16x3", "G2", _NO_RICH, g_mult=2049)}
ALL_RICH_CASES = [c for mode in ("bf16x6", "bf16x3", "f16x3") for c in RICH_CASES[mode]]
# teeth: these bf16x6 cases run with two parts lose the terms they are named for
RICH_TEETH = [c for c in RICH_CASES["bf16x6"] if c.family in ("W3", "W2X2") and c.rich in ("positional_net.1", "directional_input")
              and c.net.n_layers == 8]


_RICH_WARP = _warp(256, 43, 332, spr=4)
RICH_WARP_CASES = [RichWarpCase(f"warp-{family}-{rich}-n332-spr4", "bf16x6", family, _RICH_WARP, rich, q, x_mult)
                   for family, q, x_mult in (("W3", 131329, 1), ("W2X2", 257, 257)) for rich in ("linear1", "linear2")]


def describe_rich(case):
    m = rich_premises(case)
    cov = sorted({f"{k}{'/' + j if j else ''}@{w}:A{t[0]}B{t[1]}" for k, j, w, t in m["covered"] if t != (0, 0)})
    return (f"{case.name:52s} max|operand| {m['max_operand']:9.0f}  non-zero last part A {m['last_a']:.5f} B {m['last_b']:.5f}  "
            f"largest sum of |part products| {m['max_abs_sum']:9.0f} ({m['max_abs_sum'] / INT_LIMIT:.5f} of 2^24)  "
            f"zero pre-activations {m['zero_preacts']}  terms: {' '.join(cov)}")


SPLIT_PROFILE = os.path.join(ROOT, "profiles", "mlp_split_exact_cases.txt")
SPLIT_PROFILE_HEAD = ("# tests/exact_net_ref.py: what the float64 reference of every case of tests/test_gpu_mlp_split_exact.py measures (CPU;\n"
                      "# rewritten by `python tests/exact_net_ref.py`, compared by tests/test_exact_net_host.py).  terms: GEMM kind / wgrad job @\n"
                      "# the rich layer l* or elsewhere : (A part, B part) with a non-zero product, part 0 x part 0 left out.\n")


def split_profile_text():
    return SPLIT_PROFILE_HEAD + "".join(describe_rich(c) + "\n" for c in ALL_RICH_CASES + RICH_WARP_CASES)


if __name__ == "__main__":
    with open(PROFILE, "w") as f:
        f.write(profile_text())
    with open(INFER_PROFILE, "w") as f:
        f.write(infer_profile_text())
    with open(SPLIT_PROFILE, "w") as f:
        f.write(split_profile_text())
    print(profile_text() + infer_profile_text() + split_profile_text())
