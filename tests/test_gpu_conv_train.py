"""The training-mode convolution block on the GPU (csrc/conv_train.hip): the C entries on integer data, ops.conv3x3_bn_block on random
data, and SmplEstimator's training forward and backward - against tests/conv_train_ref.py.

  exact cases    x and dz integers in [-4, 4], weights integers in [-2, 2]: every partial sum of dW (at most 16 N H W < 2^24), of dx
                 (at most 72 Co) and of db is an integer below 2^24, so fp32 is exact in ANY order - the entries must equal the float64
                 convolution gradients bit for bit.  Shapes [N, Ci, H, W, Co]: all halo; ragged in every dimension; one tile, one
                 channel group; block 5 of the network; 45 slices of one job; 303 slices of two jobs.
  ties, masks    integer z with mean = 0, invstd = gamma = 1, beta = 0 on odd extents: dbeta = s1 and dgamma = s2 are integers and
                 must be exact; g is recovered from dz as rint(dz + s1 / M + z s2 / M) and must equal the written-out routing exactly.
  random cases   E = max|y - y64| / max|y64| per tensor; E(kernel) <= 8 E(fp32 CPU restatement) (DESIGN.md section 8g's rule).  The
                 seeds are chosen on the CPU so that the fp32 and the float64 restatement select the same ReLU mask and the same
                 window argmax (asserted before the GPU is touched): a flip is a discrete event, not a rounding error.
  conv bias      its true gradient under batch statistics is 0, so it is tested at the entry on a given dz:
                 |db - sum64 dz| <= 2^-23 sum|dz| (one fp32 rounding of a float64 sum)
Every figure is printed before it is asserted (pytest -s; profiles/conv_train_errors.txt holds a run on an MI355X)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_train_ref as CR
import smpl_estimator_ref as ER
from smpl_nerf_amd import _lib, estimator, layered, ops

pytestmark = pytest.mark.gpu
EXACT = [(2, 1, 1, 1, 1), (3, 5, 17, 33, 17), (1, 8, 16, 16, 16), (2, 64, 16, 16, 128), (5, 4, 48, 48, 8), (5, 2, 176, 176, 4)]
SLICES = {(2, 1, 1, 1, 1): 2, (3, 5, 17, 33, 17): 18, (1, 8, 16, 16, 16): 1, (2, 64, 16, 16, 128): 2, (5, 4, 48, 48, 8): 45, (5, 2, 176, 176, 4): 303}
# [N, Ci, H, W, Co, pool] -> the seed for which fp32 and float64 agree on every mask and argmax (found on the CPU; asserted below)
RANDOM = {(2, 3, 18, 34, 16, 1): 1, (3, 5, 17, 33, 17, 0): 1, (2, 16, 32, 32, 32, 1): 1, (2, 64, 16, 16, 128, 1): 1}
NAMES = ("y", "mean", "invstd", "running_mean", "running_var", "dx", "dw", "dgamma", "dbeta")


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


def gpu(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrays)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, _lib.load().snerf_last_error_string()


# ---- the entries on integer data ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(shape):
    N, Ci, H, W, Co = shape
    rng = np.random.default_rng(100 + sum(shape))
    x, dz = rng.integers(-4, 5, (N, Ci, H, W)).astype(np.float32), rng.integers(-4, 5, (N, Co, H, W)).astype(np.float32)
    w = rng.integers(-2, 3, (Co, Ci, 3, 3)).astype(np.float32)
    xt, wt = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(w).double().requires_grad_(True)
    F.conv2d(xt, wt, None, padding=1).backward(torch.from_numpy(dz).double())
    return x, w, dz, xt.grad.numpy(), wt.grad.numpy(), dz.astype(np.float64).sum((0, 2, 3))


@pytest.mark.parametrize("shape", EXACT, ids=ids(EXACT))
def test_conv_gradients_exact_on_integer_inputs(dev, shape):
    N, Ci, H, W, Co = shape
    x, w, dz, dx64, dw64, db64 = exact_case(shape)
    assert max(np.abs(dw64).max(), np.abs(dx64).max(), np.abs(db64).max()) < 2 ** 24 and 16 * N * H * W < 2 ** 24
    lib = _lib.load()
    slices = lib.snerf_conv3x3_bwd_weight_slices(N, Ci, H, W, Co)
    red = lib.snerf_bn_stats_scratch_floats(N, 1, H, W) // 4 if N * H * W > 1 else 1
    need = lib.snerf_conv3x3_bwd_weight_scratch_floats(N, Ci, H, W, Co)
    assert slices == SLICES[shape] and need == 4 * Co * red + slices * Co * Ci * 9      # the slice count, through the scratch query
    xt, wt, dzt = gpu(dev, x, w, dz)
    nan = float("nan")
    dw, db, dx = torch.full((Co, Ci, 3, 3), nan, device=dev), torch.full((Co,), nan, device=dev), torch.full((N, Ci, H, W), nan, device=dev)
    scratch = torch.full((need,), nan, device=dev)
    ok(lib.snerf_conv3x3_bwd_weight_f32(dzt.data_ptr(), xt.data_ptr(), N, Ci, Co, H, W, dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), stream()))
    scratch2 = torch.full((lib.snerf_conv3x3_bwd_input_scratch_floats(Ci, Co),), nan, device=dev)
    ok(lib.snerf_conv3x3_bwd_input_f32(dzt.data_ptr(), N, Co, H, W, wt.data_ptr(), Ci, dx.data_ptr(), scratch2.data_ptr(), stream()))
    np.testing.assert_array_equal(dw.cpu().numpy().astype(np.float64), dw64)
    np.testing.assert_array_equal(db.cpu().numpy().astype(np.float64), db64)
    np.testing.assert_array_equal(dx.cpu().numpy().astype(np.float64), dx64)
    # each output alone: the same bits
    dw2, db2 = torch.full_like(dw, nan), torch.full_like(db, nan)
    ok(lib.snerf_conv3x3_bwd_weight_f32(dzt.data_ptr(), xt.data_ptr(), N, Ci, Co, H, W, dw2.data_ptr(), None, scratch.data_ptr(), stream()))
    ok(lib.snerf_conv3x3_bwd_weight_f32(dzt.data_ptr(), None, N, Ci, Co, H, W, None, db2.data_ptr(), scratch.data_ptr(), stream()))
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pool", [1, 0])
def test_ties_and_masks_exact_on_integer_maps(dev, relu, pool):
    """Windows of equal positive values, of zeros and of negatives; odd H and W with pooling; two reduction slices would need 8192
    windows - the slice walk is covered by the exact and random cases."""
    N, C, H, W = 3, 4, 7, 9
    rng = np.random.default_rng(20 + 2 * relu + pool)
    z = rng.integers(-2, 3, (N, C, H, W)).astype(np.float32)
    z[0, 0, :2, :2], z[0, 0, :2, 2:4], z[0, 0, :2, 4:6] = 1.0, 0.0, -1.0
    dy = rng.integers(-4, 5, (N, C, H // 2, W // 2) if pool else (N, C, H, W)).astype(np.float32)
    g64, s1, s2, dz64 = CR.bn_pool_bwd64(z, dy, relu, pool)
    M = N * H * W
    zt, dyt, zero, one = gpu(dev, z, dy, np.zeros(C), np.ones(C))
    lib = _lib.load()
    nan = float("nan")
    y = torch.full(tuple(dy.shape), nan, device=dev)
    ok(lib.snerf_bn_relu_pool_fwd_f32(zt.data_ptr(), N, C, H, W, zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(), relu, pool,
                                      y.data_ptr(), stream()))
    a = torch.from_numpy(z).double()
    a = torch.relu(a) if relu else a
    np.testing.assert_array_equal(y.cpu().numpy().astype(np.float64), (F.max_pool2d(a, 2, 2) if pool else a).numpy())
    dz, dg, db = torch.full((N, C, H, W), nan, device=dev), torch.full((C,), nan, device=dev), torch.full((C,), nan, device=dev)
    scratch = torch.full((lib.snerf_bn_relu_pool_bwd_scratch_floats(N, C, H, W, pool),), nan, device=dev)
    ok(lib.snerf_bn_relu_pool_bwd_f32(zt.data_ptr(), dyt.data_ptr(), N, C, H, W, zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                      relu, pool, dz.data_ptr(), dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), stream()))
    np.testing.assert_array_equal(db.cpu().numpy().astype(np.float64), s1)          # dbeta = s1 = sum g
    np.testing.assert_array_equal(dg.cpu().numpy().astype(np.float64), s2)          # dgamma = s2 = sum g xhat
    got = dz.cpu().numpy().astype(np.float64)
    g = np.rint(got + s1[None, :, None, None] / M + z * s2[None, :, None, None] / M)
    np.testing.assert_array_equal(g, g64)
    assert np.abs(got - dz64).max() <= 2.0 ** -23 * np.abs(dz64).max()              # one fp32 rounding of the float64 expression
    if pool:
        assert (g64[:, :, :6, :8] != 0).any() and not g[:, :, 6].any() and not g[:, :, :, 8].any()
        assert np.abs(got[:, :, 6]).max() > 0      # ... but their dz is not 0: the batch statistics reach every pixel
    # dgamma and dbeta alone, and dz alone: the same bits
    dg2, db2, dz2 = torch.full_like(dg, nan), torch.full_like(db, nan), torch.full_like(dz, nan)
    ok(lib.snerf_bn_relu_pool_bwd_f32(zt.data_ptr(), dyt.data_ptr(), N, C, H, W, zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                      relu, pool, None, dg2.data_ptr(), db2.data_ptr(), scratch.data_ptr(), stream()))
    ok(lib.snerf_bn_relu_pool_bwd_f32(zt.data_ptr(), dyt.data_ptr(), N, C, H, W, zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                      relu, pool, dz2.data_ptr(), None, None, scratch.data_ptr(), stream()))
    assert torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(dz2, dz)


def test_batch_statistics_on_integer_maps_and_two_slices(dev):
    """M = 2 x 64 x 128 = 2^14 integers per channel: two reduction slices; mean and the variance are exact in float64, so mean and the
    running mean equal numpy's float64 values rounded once; invstd and the running variance pass through a square root and a quotient
    and are held to one fp32 ulp."""
    N, C, H, W = 2, 3, 64, 128
    rng = np.random.default_rng(5)
    z = rng.integers(-8, 9, (N, C, H, W)).astype(np.float32)
    rm, rv = rng.integers(-2, 3, C).astype(np.float32), rng.integers(1, 4, C).astype(np.float32)
    lib = _lib.load()
    assert lib.snerf_bn_stats_scratch_floats(N, C, H, W) == 4 * C * 2
    zt, rmt, rvt = gpu(dev, z, rm, rv)
    nan = float("nan")
    mean, invstd = torch.full((C,), nan, device=dev), torch.full((C,), nan, device=dev)
    scratch = torch.full((4 * C * 2,), nan, device=dev)
    ok(lib.snerf_bn_stats_f32(zt.data_ptr(), N, C, H, W, 0.0, 0.25, rmt.data_ptr(), rvt.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                              scratch.data_ptr(), stream()))
    M = N * H * W
    z64 = z.astype(np.float64)
    mu, var = z64.mean((0, 2, 3)), z64.var((0, 2, 3))
    np.testing.assert_array_equal(mean.cpu().numpy(), mu.astype(np.float32))
    np.testing.assert_array_equal(rmt.cpu().numpy(), (0.75 * rm + 0.25 * mu).astype(np.float32))
    assert np.abs(invstd.cpu().numpy() - 1 / np.sqrt(var)).max() <= 2.0 ** -23 * (1 / np.sqrt(var)).max()
    want = 0.75 * rv + 0.25 * var * M / (M - 1)
    assert np.abs(rvt.cpu().numpy() - want).max() <= 2.0 ** -23 * want.max()
    # without running statistics: the same mean and invstd
    mean2, invstd2 = torch.full_like(mean, nan), torch.full_like(invstd, nan)
    ok(lib.snerf_bn_stats_f32(zt.data_ptr(), N, C, H, W, 0.0, 0.25, None, None, mean2.data_ptr(), invstd2.data_ptr(), scratch.data_ptr(), stream()))
    assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd)


def test_conv_bias_gradient_is_one_rounding_of_the_float64_sum(dev):
    N, Ci, H, W, Co = 3, 5, 40, 72, 17      # 8640 terms per channel: two slices
    dz = np.random.default_rng(9).standard_normal((N, Co, H, W)).astype(np.float32)
    lib = _lib.load()
    dzt, = gpu(dev, dz)
    db = torch.full((Co,), float("nan"), device=dev)
    scratch = torch.full((lib.snerf_conv3x3_bwd_weight_scratch_floats(N, Ci, H, W, Co),), float("nan"), device=dev)
    ok(lib.snerf_conv3x3_bwd_weight_f32(dzt.data_ptr(), None, N, Ci, Co, H, W, None, db.data_ptr(), scratch.data_ptr(), stream()))
    want, scale = dz.astype(np.float64).sum((0, 2, 3)), np.abs(dz.astype(np.float64)).sum((0, 2, 3))
    err = np.abs(db.cpu().numpy().astype(np.float64) - want)
    print(f"db: max |db - sum64 dz| / sum|dz| = {(err / scale).max():.3e}   bound {2.0 ** -23:.3e}")
    assert (err <= 2.0 ** -23 * scale).all()


# ---- the op on random data -----------------------------------------------------------------------------------------------------------
def random_inputs(shape, seed):
    N, Ci, H, W, Co, pool = shape
    rng = np.random.default_rng(seed + 1000 * sum(shape))
    f32 = np.float32
    return dict(x=rng.standard_normal((N, Ci, H, W)).astype(f32), w=(rng.standard_normal((Co, Ci, 3, 3)) / np.sqrt(9 * Ci)).astype(f32),
                b=rng.uniform(-0.1, 0.1, Co).astype(f32), gamma=rng.uniform(0.5, 1.5, Co).astype(f32), beta=rng.uniform(-0.1, 0.1, Co).astype(f32),
                rm=rng.uniform(-0.2, 0.2, Co).astype(f32), rv=rng.uniform(0.5, 2.0, Co).astype(f32),
                dy=rng.standard_normal((N, Co, H // 2, W // 2) if pool else (N, Co, H, W)).astype(f32))


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """inputs, block64 and block32 of a case, computed once and shared (read-only)"""
    a = random_inputs(shape, RANDOM[shape])
    args = (a["x"], a["w"], a["b"], a["gamma"], a["beta"], a["rm"], a["rv"], a["dy"])
    return a, CR.block64(*args, relu=True, pool=bool(shape[5])), CR.block32(*args, relu=True, pool=bool(shape[5]))


def run_op(dev, a, pool, grads=(True,) * 5):
    """ops.conv3x3_bn_block forward and backward; `grads`: which of x, w, b, gamma, beta require grad"""
    x, w, b, gamma, beta, rm, rv, dy = gpu(dev, a["x"], a["w"], a["b"], a["gamma"], a["beta"], a["rm"], a["rv"], a["dy"])
    leaves = [t.requires_grad_(r) for t, r in zip((x, w, b, gamma, beta), grads)]
    calls = _lib.CALLS
    y = ops.conv3x3_bn_block(*leaves, rm, rv, momentum=CR.MOMENTUM, eps=ER.EPS, relu=True, pool=pool)
    saved = y.grad_fn.saved_tensors
    y.backward(dy)
    assert _lib.CALLS - calls == 2
    out = {"y": y.detach(), "z": saved[4], "mean": saved[5], "invstd": saved[6], "running_mean": rm, "running_var": rv}
    out.update({k: t.grad for k, t in zip(("dx", "dw", "db", "dgamma", "dbeta"), leaves)})
    return out


@pytest.mark.parametrize("shape", list(RANDOM), ids=ids(RANDOM))
def test_random_inputs_within_8x_the_fp32_cpu_error(dev, shape):
    a, r64, r32 = random_case(shape)
    assert CR.same_choices(r32, r64), "the seed's fp32 and float64 restatements differ in a ReLU mask or a window argmax: pick another"
    got = run_op(dev, a, bool(shape[5]))
    for name in NAMES:
        e, e32 = ER.E(got[name].cpu().numpy(), r64[name]), ER.E(r32[name], r64[name])
        print(f"conv3x3_bn_block {list(shape)} {name:13s}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32) if e32 else 0.0:.3f}")
    for name in NAMES:
        e, e32 = ER.E(got[name].cpu().numpy(), r64[name]), ER.E(r32[name], r64[name])
        assert e <= ER.FACTOR * e32, (shape, name, e, e32)
    # the conv bias: its true gradient is 0; the entry returns the float64 sum of ITS dz, which cancels to rounding noise
    assert float(got["db"].abs().max()) <= 2.0 ** -20 * np.abs(r64["dz"]).sum((0, 2, 3)).max()


def test_two_calls_and_grad_subsets_give_the_same_bits(dev):
    shape = (2, 16, 32, 32, 32, 1)
    a, _, _ = random_case(shape)
    full = run_op(dev, a, True)
    again = run_op(dev, a, True)
    for k, v in full.items():
        assert torch.equal(v, again[k]), k
    for grads in ((False, True, True, True, True), (True, False, False, True, True), (False, False, False, True, False),
                  (False, False, True, False, False), (True, False, False, False, False)):
        part = run_op(dev, a, True, grads)
        for k, need in zip(("dx", "dw", "db", "dgamma", "dbeta"), grads):
            assert (part[k] is None) == (not need) and (not need or torch.equal(part[k], full[k])), (grads, k)
        assert torch.equal(part["y"], full["y"]) and torch.equal(part["running_var"], full["running_var"])
    # no running statistics, and under no_grad: the same y
    x, w, b, gamma, beta = gpu(dev, a["x"], a["w"], a["b"], a["gamma"], a["beta"])
    with torch.no_grad():
        assert torch.equal(ops.conv3x3_bn_block(x, w, b, gamma, beta, pool=True), full["y"])
    with pytest.raises(RuntimeError, match="M = N H W = 1"):
        ops.conv3x3_bn_block(x[:1, :, :1, :1], w, b, gamma, beta)
    with pytest.raises(RuntimeError, match="momentum"):
        ops.conv3x3_bn_block(x, w, b, gamma, beta, momentum=None)


# ---- the network -------------------------------------------------------------------------------------------------------------------------
def model_on(dev, s, hs, p=0.0):
    m = estimator.SmplEstimator(hs)
    m.load_state_dict(ER.tensors(s))
    m.dropout.p = p
    return m.to(dev).train()


def graph_nodes(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return seen
    seen.add(fn)
    for nxt, _ in fn.next_functions:
        graph_nodes(nxt, seen)
    return seen


@functools.lru_cache(maxsize=None)
def network_case(hs):
    x = ER.images(ER.GOLDEN_IMAGE_SEED, ER.GOLDEN_N)
    s = ER.state(ER.GOLDEN_SEED, hs)
    dout = np.random.default_rng(77).standard_normal((ER.GOLDEN_N, hs)).astype(np.float32)
    return x, s, dout, CR.network(s, x, dout, torch.float64), CR.network(s, x, dout, torch.float32)


@pytest.mark.parametrize("hs", [2, 69])
def test_network_training_forward_and_backward(dev, hs):
    x, s, dout, r64, r32 = network_case(hs)
    m = model_on(dev, s, hs)
    xt, dt = gpu(dev, x, dout)
    calls = _lib.CALLS
    with _lib.profile() as prof:
        out = m(xt)
        out.backward(dt)
    names = sorted(prof.summary())
    print("library calls:", names)
    assert _lib.CALLS - calls == 5 + 5 + 2 + 2
    assert sum(n.startswith("conv3x3_bn_block_fwd") for n in names) == 5 and sum(n.startswith("conv3x3_bn_block_bwd") for n in names) == 5
    # no torch convolution, BatchNorm or pool ran: the graph holds the library's functions
    kinds = {type(f).__name__ for f in graph_nodes(out.grad_fn)}
    print("graph nodes:", sorted(kinds))
    assert not any(k.startswith(("Convolution", "NativeBatchNorm", "CudnnBatchNorm", "MiopenBatchNorm", "MaxPool", "Addmm", "Mm")) for k in kinds), kinds
    assert sum(type(f).__name__ == "_ConvBnBlockFnBackward" for f in graph_nodes(out.grad_fn)) == 5
    sd = m.state_dict()
    assert all(int(sd[f"bn{i}.num_batches_tracked"]) == 8 for i in range(1, 6))
    results = [("out", out.detach().cpu().numpy(), r64["out"], r32["out"])]
    results += [(k, sd[k].cpu().numpy(), r64["stats"][k], r32["stats"][k]) for k in r64["stats"]]
    results += [(k + ".grad", p.grad.cpu().numpy(), r64["grads"][k], r32["grads"][k]) for k, p in m.named_parameters()
                if not (k.startswith("conv") and k.endswith("bias"))]
    flips = sum(int((a != b).sum()) for a, b in zip(r32["masks"], r64["masks"])) + \
        sum(int((a != b).sum()) for a, b in zip(r32["argmaxes"], r64["argmaxes"]) if a is not None)
    print(f"human_size {hs}: mask / argmax differences between the fp32 and the float64 restatement: {flips}")
    failed = []
    for name, got, y64, y32 in results:
        e, e32 = ER.E(got, y64), ER.E(y32, y64)
        print(f"  {name:22s}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32) if e32 else 0.0:.3f}")
        if not e <= ER.FACTOR * e32:
            failed.append((name, e, e32))
    # the conv biases: true gradient 0 under batch statistics (tested at the entry); here finite, and noise beside the weights' gradients
    for i in range(1, 6):
        db, dw = getattr(m, f"conv{i}").bias.grad, getattr(m, f"conv{i}").weight.grad
        print(f"  conv{i}.bias.grad      : max |db| {float(db.abs().max()):.3e}   (max |dw| {float(dw.abs().max()):.3e})")
        assert bool(torch.isfinite(db).all())
    assert not failed, failed


def test_module_is_the_five_ops_and_two_linears(dev):
    x, s, dout, _, _ = network_case(2)
    m = model_on(dev, s, 2)
    xt, dt = gpu(dev, x, dout)
    out = m(xt)
    out.backward(dt)
    other = model_on(dev, s, 2)
    h = xt
    for i, (conv, bn) in enumerate(other._blocks()):
        h = ops.conv3x3_bn_block(h, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=0.1, eps=1e-5,
                                 relu=True, pool=ER.POOL[i])
    h = layered.linear([(h.reshape(-1, 8192), other.fc1.weight)], other.fc1.bias, relu=True)
    by_hand = layered.linear([(h, other.fc2.weight)], other.fc2.bias)
    by_hand.backward(dt)
    assert torch.equal(by_hand, out)
    for (k, p), (_, q) in zip(m.named_parameters(), other.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for k in ("bn1.running_mean", "bn5.running_var"):
        assert torch.equal(m.state_dict()[k], other.state_dict()[k])
    # eval mode under no_grad keeps its one call; eval mode with grad keeps the torch branch
    m.eval()
    calls = _lib.CALLS
    with torch.no_grad():
        m(xt)
    assert _lib.CALLS - calls == 1
    calls = _lib.CALLS
    assert m(xt).grad_fn is not None and _lib.CALLS == calls


def test_dropout_is_live_and_train_epoch_runs(dev):
    x, s, _, _, _ = network_case(2)
    m = model_on(dev, s, 2, p=0.25)
    xt, = gpu(dev, x)
    with torch.no_grad():
        assert not torch.equal(m(xt), m(xt))
    truth = torch.from_numpy(np.random.default_rng(6).uniform(-0.5, 0.5, (4, 69)).astype(np.float32))
    images = torch.from_numpy(ER.images(ER.GOLDEN_IMAGE_SEED, 4))
    loader = [(images[:2], truth[:2]), (images[2:], truth[2:])]      # CPU batches, as a DataLoader hands them over
    before = m.fc2.weight.detach().clone()
    calls = _lib.CALLS
    got = estimator.train_epoch(m.eval(), loader, torch.optim.Adam(m.parameters(), lr=1e-4))
    assert isinstance(got, float) and np.isfinite(got) and m.training
    assert _lib.CALLS - calls == 2 * 14 and not torch.equal(m.fc2.weight, before)
    assert int(m.bn1.num_batches_tracked) == 7 + 2 + 2
