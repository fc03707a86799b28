"""The training-mode convolution block without a GPU: the restatement the GPU tests measure with (tests/conv_train_ref.py) against
torch's own nn modules on the CPU, the written-out pool / ReLU routing against torch's autograd on windows full of ties, the
host-side argument checks of the C entries of csrc/conv_train.hip, and estimator.train_epoch on the CPU (the torch branch).

Bounds.  The restatement and the nn modules compute the same function in the same precision but not in the same operation order
(F.batch_norm folds invstd and gamma), so they are compared in float64, where an order costs a few ulp of 2^-53: 1e-12 relative
to the largest magnitude of a tensor holds with five orders of magnitude to spare and fails for any other function."""
import numpy as np
import pytest
import torch

import conv_train_ref as CR
import smpl_estimator_ref as ER
from smpl_nerf_amd import _lib, build, estimator

BAD, ALIGN = -1, -2      # SNERF_E_BADARG, SNERF_E_ALIGN
TIGHT = 1e-12


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.abs(got - want).max() <= TIGHT * max(np.abs(want).max(), 1e-30), (name, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("shape", [(2, 3, 6, 7, 4, 1), (3, 2, 5, 5, 3, 0)], ids=["pool", "nopool"])
def test_block_restatement_against_nn_modules_in_float64(shape):
    N, Ci, H, W, Co, pool = shape
    rng = np.random.default_rng(sum(shape))
    x, w, b = rng.standard_normal((N, Ci, H, W)), rng.standard_normal((Co, Ci, 3, 3)) / 3, rng.uniform(-0.1, 0.1, Co)
    gamma, beta, rm, rv = rng.uniform(0.5, 1.5, Co), rng.uniform(-0.1, 0.1, Co), rng.uniform(-0.2, 0.2, Co), rng.uniform(0.5, 2, Co)
    dy = rng.standard_normal((N, Co, H // 2, W // 2) if pool else (N, Co, H, W))
    got = CR.block64(x, w, b, gamma, beta, rm, rv, dy, relu=True, pool=bool(pool))
    conv, bn = torch.nn.Conv2d(Ci, Co, 3, padding=1).double(), torch.nn.BatchNorm2d(Co).double()
    with torch.no_grad():
        for t, v in ((conv.weight, w), (conv.bias, b), (bn.weight, gamma), (bn.bias, beta), (bn.running_mean, rm), (bn.running_var, rv)):
            t.copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).requires_grad_(True)
    y = torch.relu(bn(conv(xt)))
    y = torch.nn.functional.max_pool2d(y, 2, 2) if pool else y
    y.backward(torch.from_numpy(dy))
    for name, want in (("y", y), ("dx", xt.grad), ("dw", conv.weight.grad), ("dgamma", bn.weight.grad), ("dbeta", bn.bias.grad),
                       ("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        close(name, got[name], want.detach().numpy())
    assert int(bn.num_batches_tracked) == 1
    # the conv bias gradient is 0 in exact arithmetic (the batch mean takes the bias out again): rounding noise on both sides
    assert np.abs(got["db"]).max() <= 1e-12 * np.abs(got["dz"]).sum() and np.abs(conv.bias.grad.numpy()).max() <= 1e-12 * np.abs(got["dz"]).sum()
    assert np.allclose(got["db"], got["dz"].sum((0, 2, 3)), rtol=0, atol=1e-12 * np.abs(got["dz"]).sum())
    assert np.allclose(got["mean"], got["z"].mean((0, 2, 3)), rtol=1e-12, atol=1e-14)
    assert np.allclose(got["invstd"], 1 / np.sqrt(got["z"].var((0, 2, 3)) + ER.EPS), rtol=1e-12)


def test_network_restatement_against_the_module_in_float64():
    s = ER.state(31, 2)
    x = ER.images(32, 2)
    dout = np.random.default_rng(33).standard_normal((2, 2))
    got = CR.network(s, x, dout, torch.float64)
    model = estimator.SmplEstimator(2)
    model.load_state_dict(ER.tensors(s))
    model.double().train()
    model.dropout.p = 0.0
    out = model(torch.from_numpy(x).double())
    out.backward(torch.from_numpy(dout))
    close("out", got["out"], out.detach().numpy())
    for name, p in model.named_parameters():
        if name.startswith("conv") and name.endswith("bias"):      # (true value 0: noise against noise)
            assert np.abs(got["grads"][name]).max() <= 1e-9 and float(p.grad.abs().max()) <= 1e-9, name
        else:
            close(name, got["grads"][name], p.grad.numpy())
    sd = model.state_dict()
    for k, v in got["stats"].items():
        close(k, v, sd[k].numpy())
    assert all(int(sd[f"bn{i}.num_batches_tracked"]) == 8 for i in range(1, 6))
    assert CR.same_choices(got, got) and got["argmaxes"][0] is None and got["argmaxes"][1].shape == (2, 32, 64, 64)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pool", [1, 0])
def test_written_out_routing_equals_torch_autograd_on_ties(relu, pool):
    """Integer maps in [-2, 2] on odd extents: most windows hold their maximum more than once, many are all zeros or all negative."""
    rng = np.random.default_rng(10 * relu + pool)
    z = rng.integers(-2, 3, (3, 4, 7, 9)).astype(np.float64)
    z[0, 0, :2, :2] = 1.0      # equal positive values, all zeros, all negative: the three kinds by hand as well
    z[0, 0, :2, 2:4] = 0.0
    z[0, 0, :2, 4:6] = -1.0
    dy = rng.integers(-4, 5, (3, 4, 3, 4) if pool else (3, 4, 7, 9)).astype(np.float64)
    g, s1, s2, dz = CR.bn_pool_bwd64(z, dy, relu, pool)
    zt = torch.from_numpy(z).requires_grad_(True)
    a = torch.relu(zt) if relu else zt
    y = torch.nn.functional.max_pool2d(a, 2, 2) if pool else a
    y.backward(torch.from_numpy(dy))
    assert np.array_equal(g, zt.grad.numpy())
    if pool:
        assert g[0, 0, 0, 0] == dy[0, 0, 0, 0] and not g[0, 0, :2, :2].ravel()[1:].any()      # the tie goes to (0, 0)
        assert not g[:, :, 6].any() and not g[:, :, :, 8].any()                                # pixels in no window
        if relu:
            assert not g[0, 0, :2, 2:6].any()                                                  # all zeros / all negative: held back
    assert np.array_equal(s1, g.sum((0, 2, 3))) and np.array_equal(s2, (g * z).sum((0, 2, 3)))
    assert dz.shape == z.shape


def test_symbols_are_exported_and_prototyped(lib):
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name, nargs in (("snerf_bn_stats_scratch_floats", 4), ("snerf_bn_stats_f32", 13), ("snerf_bn_relu_pool_fwd_f32", 13),
                        ("snerf_bn_relu_pool_bwd_scratch_floats", 5), ("snerf_bn_relu_pool_bwd_f32", 17),
                        ("snerf_conv3x3_bwd_input_scratch_floats", 2), ("snerf_conv3x3_bwd_input_f32", 10),
                        ("snerf_conv3x3_bwd_weight_slices", 5), ("snerf_conv3x3_bwd_weight_scratch_floats", 5),
                        ("snerf_conv3x3_bwd_weight_f32", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in text
    assert lib.snerf_version() == 109


def _stats(lib, z=8, N=1, C=4, H=4, W=4, eps=1e-5, momentum=0.1, rm=8, rv=8, mean=8, invstd=8, scratch=8):
    return lib.snerf_bn_stats_f32(z, N, C, H, W, eps, momentum, rm, rv, mean, invstd, scratch, None)


def _fwd(lib, z=8, N=1, C=4, H=4, W=4, mean=8, invstd=8, gamma=8, beta=8, relu=1, pool=0, y=8):
    return lib.snerf_bn_relu_pool_fwd_f32(z, N, C, H, W, mean, invstd, gamma, beta, relu, pool, y, None)


def _bwd(lib, z=8, dy=8, N=1, C=4, H=4, W=4, mean=8, invstd=8, gamma=8, beta=8, relu=1, pool=0, dz=8, dgamma=8, dbeta=8, scratch=8):
    return lib.snerf_bn_relu_pool_bwd_f32(z, dy, N, C, H, W, mean, invstd, gamma, beta, relu, pool, dz, dgamma, dbeta, scratch, None)


def _dgrad(lib, dz=8, N=1, Co=4, H=4, W=4, w=8, Ci=3, dx=8, scratch=8):
    return lib.snerf_conv3x3_bwd_input_f32(dz, N, Co, H, W, w, Ci, dx, scratch, None)


def _wgrad(lib, dz=8, x=8, N=1, Ci=3, Co=4, H=4, W=4, dw=8, dbias=8, scratch=8):
    return lib.snerf_conv3x3_bwd_weight_f32(dz, x, N, Ci, Co, H, W, dw, dbias, scratch, None)


def test_argument_validation_happens_on_the_host(lib):
    """Every refusal comes before anything touches a device: this runs where there is none.  (The non-null pointers are the number 8:
    nothing may read through them.)"""
    err = lib.snerf_last_error_string
    for call in (_stats, _fwd, _bwd):
        for bad in (0, 257, -1):
            assert call(lib, C=bad) == BAD and f"= {bad}".encode() in err(), (call.__name__, bad)
        assert call(lib, H=0) == BAD and call(lib, W=0) == BAD and call(lib, N=-1) == BAD and b"N = -1" in err()
        assert call(lib, N=2 ** 20, C=2, H=32, W=32) == BAD and b"2^31" in err()
        assert call(lib, N=0, C=0) == BAD
    # one value per channel: refused as torch refuses it; two are enough
    assert _stats(lib, N=1, H=1, W=1) == BAD and b"M = N H W = 1" in err()
    assert _bwd(lib, N=1, H=1, W=1) == BAD and b"M = N H W = 1" in err()
    assert lib.snerf_bn_stats_scratch_floats(1, 4, 1, 1) == BAD and lib.snerf_bn_relu_pool_bwd_scratch_floats(1, 4, 1, 1, 0) == BAD
    assert lib.snerf_bn_stats_scratch_floats(2, 4, 1, 1) == 16 and lib.snerf_bn_stats_scratch_floats(1, 4, 1, 2) == 16
    assert _fwd(lib, pool=1, H=1) == BAD and b"H = 1" in err() and _bwd(lib, pool=1, W=1) == BAD and b"W = 1" in err()
    assert _stats(lib, eps=-1e-5) == BAD and b"eps" in err() and _stats(lib, eps=float("nan")) == BAD
    assert _stats(lib, momentum=float("inf")) == BAD and b"momentum" in err()
    for name in ("z", "mean", "invstd", "scratch"):
        assert _stats(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    for name in ("z", "mean", "invstd", "gamma", "beta", "y"):
        assert _fwd(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    for name in ("z", "dy", "mean", "invstd", "gamma", "beta", "scratch"):
        assert _bwd(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _stats(lib, scratch=4) == ALIGN and _bwd(lib, scratch=4) == ALIGN and _wgrad(lib, scratch=4) == ALIGN and b"8-byte" in err()
    # N = 0 is a no-op whatever the pointers are; nothing asked for is a no-op too
    assert _stats(lib, N=0, z=None, mean=None, invstd=None, scratch=None) == 0
    assert _fwd(lib, N=0, z=None, y=None) == 0 and _bwd(lib, N=0, z=None, dy=None, scratch=None) == 0
    assert _bwd(lib, dz=None, dgamma=None, dbeta=None) == 0 and _wgrad(lib, dw=None, dbias=None) == 0
    # the convolution's gradients: conv_check's limits
    for call in (_dgrad, _wgrad):
        for bad in (0, 257):
            assert call(lib, Ci=bad) == BAD and f"Ci = {bad}".encode() in err()
            assert call(lib, Co=bad) == BAD and f"Co = {bad}".encode() in err()
        assert call(lib, N=-1) == BAD and call(lib, H=0) == BAD and call(lib, N=2 ** 20, Ci=2, H=32, W=32) == BAD
    for name in ("dz", "w", "dx", "scratch"):
        assert _dgrad(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    for name in ("dz", "x", "scratch"):
        assert _wgrad(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _dgrad(lib, N=0, dz=None, w=None, dx=None, scratch=None) == 0 and _wgrad(lib, N=0, dz=None, x=None, scratch=None) == 0
    # scratch sizes: a function of the shapes alone
    assert lib.snerf_conv3x3_bwd_input_scratch_floats(3, 16) == 3 * 16 * 9 + 6 and lib.snerf_conv3x3_bwd_input_scratch_floats(0, 16) == BAD
    assert lib.snerf_conv3x3_bwd_weight_slices(5, 4, 48, 48, 8) == 45 and lib.snerf_conv3x3_bwd_weight_slices(0, 4, 48, 48, 8) == 0
    assert lib.snerf_conv3x3_bwd_weight_slices(2, 64, 16, 16, 128) == 2         # two jobs
    assert lib.snerf_conv3x3_bwd_weight_slices(5, 2, 176, 176, 4) == 303       # 605 jobs, two per slice
    assert lib.snerf_conv3x3_bwd_weight_slices(100, 64, 16, 16, 128) == 25     # 100 jobs, 16 column groups: 4 per slice
    assert lib.snerf_conv3x3_bwd_weight_scratch_floats(5, 4, 48, 48, 8) == 4 * 8 * 2 + 45 * 8 * 4 * 9      # 11520 terms: 2 slices for db
    assert lib.snerf_conv3x3_bwd_weight_scratch_floats(1, 300, 4, 4, 8) == BAD
    assert lib.snerf_bn_stats_scratch_floats(16, 16, 128, 128) == 4 * 16 * 32 and lib.snerf_bn_stats_scratch_floats(100, 16, 128, 128) == 4 * 16 * 128
    assert lib.snerf_bn_relu_pool_bwd_scratch_floats(2, 8, 5, 7, 1) == 4 * 8 + 4 * 8


def test_train_epoch_on_the_cpu_branch():
    torch.manual_seed(4)
    s = ER.state(41, 2)
    model = estimator.SmplEstimator(2)
    model.load_state_dict(ER.tensors(s))
    model.eval()
    x = torch.from_numpy(ER.images(42, 3))
    truth = torch.from_numpy(np.random.default_rng(43).uniform(-0.5, 0.5, (3, 69)).astype(np.float32))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    optim = torch.optim.SGD(model.parameters(), lr=1e-3)
    got = estimator.train_epoch(model, [(x[:2], truth[:2]), (x[2:], truth[2:])], optim, log_iterations=1)
    assert isinstance(got, float) and np.isfinite(got) and got > 0 and model.training
    after = model.state_dict()
    assert int(after["bn1.num_batches_tracked"]) == 9
    assert all(not torch.equal(after[k], before[k]) for k in ("conv1.weight", "fc2.bias", "bn3.weight", "bn5.running_var"))
    assert estimator.train_epoch(model, [], optim) == 0.0


def test_cpu_tensors_are_refused_by_the_op_and_kept_on_the_torch_branch_by_the_module():
    from smpl_nerf_amd import ops
    x, w, a = torch.rand(2, 3, 8, 8), torch.rand(16, 3, 3, 3), torch.ones(16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv3x3_bn_block(x, w, a, a, a)
    model = estimator.SmplEstimator(2)
    calls = _lib.CALLS
    assert model.training and model(torch.rand(2, 3, 128, 128)).grad_fn is not None and _lib.CALLS == calls
