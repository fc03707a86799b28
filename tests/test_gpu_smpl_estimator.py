"""SmplEstimator's one-call forward on the GPU (snerf_smpl_estimator_fwd_f32 through estimator.SmplEstimator in eval mode under
no_grad) against tests/smpl_estimator_ref.py and the reference's own outputs (tests/golden/g24_smpl_estimator.npz).

Bounds, with E = max|y - forward64| / max|forward64|:
  against forward64    E(kernel) <= 8 E(forward32)                       (DESIGN.md section 8g's rule)
  against the golden   max|kernel - golden| / max|forward64| <= 8 E(forward32): the same rule, with the reference's own fp32 CPU run
                       in the place of forward64
Both CPU restatements are computed once per human_size and shared.  The torch branch of the module (training mode, grad, CPU) is
ordinary torch and is not exercised here."""
import numpy as np
import pytest
import torch

import smpl_estimator_ref as ER
from conftest import load_golden
from smpl_nerf_amd import _lib, estimator, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    """Four images (the first two are the golden's), and per human_size the state and both CPU restatements."""
    x = ER.images(ER.GOLDEN_IMAGE_SEED, 4)
    assert np.array_equal(x[:2], ER.images(ER.GOLDEN_IMAGE_SEED, ER.GOLDEN_N))
    out = {"x": x}
    for hs in (2, 69):
        s = ER.state(ER.GOLDEN_SEED, hs)
        out[hs] = (s, ER.forward64(s, x)[0], ER.forward32(s, x)[0])
    return out


def model_on(dev, s, hs):
    m = estimator.SmplEstimator(hs)
    m.load_state_dict(ER.tensors(s))
    return m.to(dev).eval()


def run(m, x):
    calls = _lib.CALLS
    with torch.no_grad():
        y = m(x)
    assert _lib.CALLS - calls == 1 and y.grad_fn is None      # one library call
    return y


@pytest.mark.parametrize("hs", [2, 69])
def test_one_call_forward_against_float64_and_the_reference(dev, case, hs):
    s, y64, y32 = case[hs]
    m = model_on(dev, s, hs)
    assert m.is_cuda
    got = run(m, torch.from_numpy(case["x"][:2]).to(dev)).cpu().numpy()
    golden = load_golden(ER.GOLDEN)[f"out/{hs}"]
    assert got.shape == golden.shape == (2, hs) and got.dtype == np.float32
    e, e32, eg = ER.E(got, y64[:2]), ER.E(y32[:2], y64[:2]), ER.E(golden, y64[:2])
    d = float(np.abs(got.astype(np.float64) - golden).max() / np.abs(y64[:2]).max())
    print(f"smpl_estimator_fwd human_size {hs}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f};   "
          f"|kernel - golden| {d:.3e}   E golden {eg:.3e}")
    assert e <= ER.FACTOR * e32
    assert d <= ER.FACTOR * e32


def test_rows_do_not_depend_on_the_batch_and_calls_repeat(dev, case):
    s, _, _ = case[69]
    m = model_on(dev, s, 69)
    x = torch.from_numpy(case["x"]).to(dev)
    whole = run(m, x)
    assert torch.equal(run(m, x), whole)                          # two calls, identical bits
    assert torch.equal(run(m, x[2:3]), whole[2:3])                # N = 1
    assert torch.equal(run(m, x[1:4]), whole[1:4])                # N = 3
    assert sorted(n for _, n in m._workspaces) == [1, 3, 4]       # one cached workspace per batch size
    assert tuple(run(m, x[:0]).shape) == (0, 69)
    assert not bool(torch.isnan(whole).any())


def test_replay_from_a_captured_graph(dev, case):
    s, _, _ = case[2]
    m = model_on(dev, s, 2)
    x = torch.from_numpy(case["x"][:2]).to(dev)
    want = run(m, x).clone()
    static_x = x.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(m, static_x)                                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        y = run(m, static_x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    static_x.copy_(torch.from_numpy(case["x"][2:4]).to(dev))       # new images into the captured input: the replay computes their rows
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, run(m, torch.from_numpy(case["x"][2:4]).to(dev)))


def test_a_parameter_changed_in_place_is_seen_by_the_next_call(dev, case):
    """The fold of BatchNorm and bias happens on the device in every call: nothing stale after an optimiser step or a load."""
    s, _, _ = case[2]
    m = model_on(dev, s, 2)
    x = torch.from_numpy(case["x"][:2]).to(dev)
    before = run(m, x)
    changed = {k: v.copy() for k, v in s.items()}
    changed["bn3.running_var"] = (changed["bn3.running_var"] * 1.5).astype(np.float32)
    changed["conv2.bias"] = (changed["conv2.bias"] + 0.25).astype(np.float32)
    changed["bn5.weight"] = (changed["bn5.weight"] * 0.5).astype(np.float32)
    with torch.no_grad():
        for k in ("bn3.running_var", "conv2.bias", "bn5.weight"):
            m.state_dict()[k].copy_(torch.from_numpy(changed[k]))
    after = run(m, x)
    fresh = run(model_on(dev, changed, 2), x)
    assert not torch.equal(after, before) and torch.equal(after, fresh)
    y64 = ER.forward64(changed, case["x"][:2])[0]
    assert ER.E(after.cpu().numpy(), y64) <= ER.FACTOR * ER.E(ER.forward32(changed, case["x"][:2])[0], y64)


def test_block_by_block_gives_the_bits_of_the_one_call(dev, case):
    """Five ops.conv3x3_block calls on estimator.fold_bn's scale and shift (float64 on the host, rounded once - what the entry's fold
    kernel computes), then snerf_linear_fwd_f32 twice: the one call's bits."""
    s, _, _ = case[69]
    m = model_on(dev, s, 69)
    x = torch.from_numpy(case["x"][:3]).to(dev)
    want = run(m, x)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        h = x
        for i, (conv, bn) in enumerate(m._blocks()):
            scale, shift = estimator.fold_bn(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            ref_scale, ref_shift = ER.fold64(s, i + 1)
            assert np.array_equal(scale.cpu().numpy(), ref_scale) and np.array_equal(shift.cpu().numpy(), ref_shift)
            h = ops.conv3x3_block(h, conv.weight, scale, shift, relu=True, pool=ER.POOL[i])
        assert tuple(h.shape) == (3, 128, 8, 8)
        flat = h.view(-1, 8 * 8 * 128)
        h1 = torch.full((3, 500), float("nan"), device=dev)
        out = torch.full((3, 69), float("nan"), device=dev)
        assert lib.snerf_linear_fwd_f32(flat.data_ptr(), 3, 8192, 8192, m.fc1.weight.data_ptr(), 8192, 500, m.fc1.bias.data_ptr(), 0, 1,
                                        h1.data_ptr(), 500, stream) == 0
        assert lib.snerf_linear_fwd_f32(h1.data_ptr(), 3, 500, 500, m.fc2.weight.data_ptr(), 500, 69, m.fc2.bias.data_ptr(), 0, 0,
                                        out.data_ptr(), 69, stream) == 0
    assert torch.equal(out, want)
    # ... and each block against the reference's own block outputs for image 0, with the rule's bound per block
    g = load_golden(ER.GOLDEN)
    _, b64 = ER.forward64(s, case["x"][:1])
    _, b32 = ER.forward32(s, case["x"][:1])
    with torch.no_grad():
        h = x[:1]
        for i, (conv, bn) in enumerate(m._blocks()):
            h = ops.conv3x3_block(h, conv.weight, *estimator.fold_bn(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps),
                                  relu=True, pool=ER.POOL[i])
            e, e32 = ER.E(h.cpu().numpy(), b64[i]), ER.E(b32[i], b64[i])
            cut = h[0, :, ::8, ::8].cpu().numpy()
            d = float(np.abs(cut.astype(np.float64) - g[f"block/{i + 1}"]).max() / np.abs(b64[i]).max())
            print(f"block {i + 1}: E kernel {e:.3e}   E fp32 CPU {e32:.3e}   kernel / bound {e / (ER.FACTOR * e32):.3f};   |kernel - golden| {d:.3e}")
            assert e <= ER.FACTOR * e32 and d <= ER.FACTOR * e32


def test_validate_on_a_synthetic_loader(dev, case):
    s, y64, y32 = case[2]
    m = model_on(dev, s, 2).train()                               # validate() runs in eval mode and restores the mode
    x = torch.from_numpy(case["x"])
    truth = torch.from_numpy(np.random.default_rng(5).uniform(-0.2, 0.2, (4, 69)).astype(np.float32))
    loader = [(x[:3], truth[:3]), (x[3:], truth[3:])]             # CPU batches, as a DataLoader hands them over
    calls = _lib.CALLS
    got = estimator.validate(m, loader)
    assert _lib.CALLS - calls == 2 and m.training

    def loss(y):
        t = truth[:, [38, 41]].double().numpy()
        return float(np.mean([np.mean((y[:3] - t[:3]) ** 2), np.mean((y[3:] - t[3:]) ** 2)]))

    want = loss(y64)
    # The outputs are held to delta = 8 E(forward32) max|forward64| per element.  A term (y - t)^2 of the loss then moves by at most
    # 2 |y - t| delta + delta^2, and so does their mean; MSELoss itself runs in fp32: the subtraction, the square, a sum of at most six
    # terms and the division, under 16 roundings of 2^-24 relative.
    delta = ER.FACTOR * ER.E(y32, y64) * np.abs(y64).max()
    bound = 2 * np.abs(y64 - truth[:, [38, 41]].double().numpy()).max() * delta + delta ** 2 + 16 * 2.0 ** -24 * want
    print(f"validate: loss {got:.9e}   float64 {want:.9e}   |error| {abs(got - want):.3e}   bound {bound:.3e}")
    assert abs(got - want) <= bound
