"""SmplEstimator without a GPU: the restatement the GPU tests measure with (tests/smpl_estimator_ref.py) and the module's torch path
against what the reference itself computed (tests/golden/g24_smpl_estimator.npz); the module's state_dict against the reference's;
the training-mode path; and the host-side argument checks of the three C entries (csrc/conv_block.hip).

Bound, for the outputs and for every block slice: |y - golden| <= 8 |forward64 - forward32|, each side normalised by the largest
|forward64| - the golden is the reference's own fp32 CPU run, so a float64 restatement of another function fails here before it
misjudges a kernel.  Measured: forward32 reproduces the golden bit for bit (E 2.0e-7 .. 4.1e-7 on both sides)."""
import ctypes

import numpy as np
import pytest
import torch

import smpl_estimator_ref as ER
from conftest import load_golden
from smpl_nerf_amd import _lib, build, estimator, io

BAD = -1      # SNERF_E_BADARG


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden_case():
    """The golden's inputs and both CPU restatements on them, computed once and shared (read-only)."""
    x = ER.images(ER.GOLDEN_IMAGE_SEED, ER.GOLDEN_N)
    case = {}
    for hs in (2, 69):
        s = ER.state(ER.GOLDEN_SEED, hs)
        case[hs] = (s, ER.forward64(s, x), ER.forward32(s, x))
    return x, case


def hold(name, y, golden, y64, y32):
    assert np.shape(y) == golden.shape == y64.shape
    e, e32 = float(np.abs(np.asarray(y, np.float64) - golden).max() / np.abs(y64).max()), ER.E(y32, y64)
    print(f"{name}: |y - golden| / max|y64| {e:.3e}   E(forward32) {e32:.3e}   bound {ER.FACTOR * e32:.3e}")
    assert e32 > 0 and e <= ER.FACTOR * e32, (name, e, e32)


@pytest.mark.parametrize("hs", [2, 69])
def test_restatement_against_the_reference_outputs(golden_case, hs):
    g = load_golden(ER.GOLDEN)
    _, case = golden_case
    _, (o64, b64), (o32, b32) = case[hs]
    assert g[f"out/{hs}"].shape == (ER.GOLDEN_N, hs) and g[f"out/{hs}"].dtype == np.float32
    hold(f"out/{hs}", o64, g[f"out/{hs}"], o64, o32)
    if hs == 69:
        for i in range(5):
            hold(f"block/{i + 1}", b64[i][0, :, ::8, ::8], g[f"block/{i + 1}"], b64[i][0, :, ::8, ::8], b32[i][0, :, ::8, ::8])


@pytest.mark.parametrize("hs", [2, 69])
def test_module_cpu_eval_path_against_the_reference_outputs(golden_case, hs):
    g = load_golden(ER.GOLDEN)
    x, case = golden_case
    s, (o64, _), (o32, _) = case[hs]
    model = estimator.SmplEstimator(hs)
    model.load_state_dict(ER.tensors(s))
    model.eval()
    with torch.no_grad():
        out = model(torch.from_numpy(x))
    assert out.shape == (ER.GOLDEN_N, hs)
    hold(f"module out/{hs}", out.numpy(), g[f"out/{hs}"], o64, o32)
    assert not model.is_cuda


def test_state_dict_is_the_references_and_round_trips(tmp_path):
    g = load_golden(ER.GOLDEN)
    model = estimator.SmplEstimator()
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]] == ER.KEYS
    assert [list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()] == g["shapes"].tolist()
    assert estimator.SmplEstimator(2).state_dict()["fc2.weight"].shape == (2, 500)
    s = ER.state(5, 69)
    model.load_state_dict(ER.tensors(s))
    io.save_run(str(tmp_path), [model], ["model_smpl_estimator.pt"])
    other = estimator.SmplEstimator()
    io.load_run(str(tmp_path), [other], ["model_smpl_estimator.pt"])
    for k, v in other.state_dict().items():
        assert np.array_equal(v.numpy(), s[k]), k
    model.save(str(tmp_path / "whole.model"))      # the reference's save(): the whole module


def test_train_mode_reaches_all_parameters_and_moves_the_running_statistics():
    torch.manual_seed(3)
    s = ER.state(11, 2)
    model = estimator.SmplEstimator(2)
    model.load_state_dict(ER.tensors(s))
    assert model.training
    x = torch.from_numpy(ER.images(12, 3))
    bn1 = torch.nn.BatchNorm2d(16)      # a BatchNorm2d of its own, given what bn1 is given
    bn1.load_state_dict({k[4:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items() if k.startswith("bn1.")})
    with torch.no_grad():
        bn1(torch.nn.functional.conv2d(x, torch.from_numpy(s["conv1.weight"]), torch.from_numpy(s["conv1.bias"]), padding=1))
    out = model(x)
    assert out.shape == (3, 2) and out.grad_fn is not None
    out.square().sum().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    sd = model.state_dict()
    for i in range(1, 6):
        assert int(sd[f"bn{i}.num_batches_tracked"]) == 8
        assert not np.array_equal(sd[f"bn{i}.running_mean"].numpy(), s[f"bn{i}.running_mean"])
        assert not np.array_equal(sd[f"bn{i}.running_var"].numpy(), s[f"bn{i}.running_var"])
    assert torch.equal(sd["bn1.running_mean"], bn1.running_mean) and torch.equal(sd["bn1.running_var"], bn1.running_var)
    # dropout is live in training mode (two forwards differ) and off in eval mode (they agree, and the statistics stay)
    with torch.no_grad():
        assert not torch.equal(model(x), model(x))
        model.eval()
        before = {k: v.clone() for k, v in model.state_dict().items()}
        assert torch.equal(model(x), model(x))
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_symbols_are_exported_and_prototyped(lib):
    text = open(_lib.HERE + "/../include/smplnerf.h").read()
    for name, nargs in (("snerf_conv3x3_block_f32", 13), ("snerf_smpl_estimator_workspace_bytes", 2), ("snerf_smpl_estimator_fwd_f32", 7)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name + "(" in text
    assert "typedef struct snerf_smpl_estimator {" in text and "typedef struct snerf_conv_bn {" in text
    # the ctypes mirrors have the C structs' layout: 6 pointers and a double; 5 of those, 4 pointers, an int32 padded to 8
    assert ctypes.sizeof(_lib.ConvBn) == 56 and ctypes.sizeof(_lib.SmplEstimatorNet) == 5 * 56 + 4 * 8 + 8
    assert lib.snerf_version() == 109


def _conv(lib, x=8, N=1, Ci=3, H=8, W=8, w=8, scale=8, shift=8, Co=16, relu=1, pool=0, y=8):
    return lib.snerf_conv3x3_block_f32(x, N, Ci, H, W, w, scale, shift, Co, relu, pool, y, None)


def _net(human_size=69, eps=1e-5, **null):
    net = _lib.SmplEstimatorNet()
    for i in range(5):
        net.block[i] = _lib.ConvBn(8, 8, 8, 8, 8, 8, eps[i] if isinstance(eps, (list, tuple)) else eps)
    net.fc1_weight = net.fc1_bias = net.fc2_weight = net.fc2_bias = 8
    net.human_size = human_size
    for name in null:
        if name.startswith("block"):
            setattr(net.block[int(name[5])], name[7:], None)
        else:
            setattr(net, name, None)
    return net


def _fwd(lib, net, images=8, N=1, out=8, ws=16, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.snerf_smpl_estimator_workspace_bytes(N, max(net.human_size, 1)), 0)
    return lib.snerf_smpl_estimator_fwd_f32(net, images, N, out, ws, ws_bytes, None)


def test_argument_validation_happens_on_the_host(lib):
    """Every refusal comes before anything touches a device: this runs where there is none.  (The non-null pointers are the numbers 8 and 16:
    nothing may read through them.)"""
    err = lib.snerf_last_error_string
    for bad in (0, 257, -1):
        assert _conv(lib, Ci=bad) == BAD and f"Ci = {bad}".encode() in err()
        assert _conv(lib, Co=bad) == BAD and f"Co = {bad}".encode() in err()
    assert _conv(lib, pool=1, H=1) == BAD and b"H = 1" in err() and b"pool" in err()
    assert _conv(lib, pool=1, W=1) == BAD and b"W = 1" in err()
    assert _conv(lib, H=0) == BAD and _conv(lib, W=0) == BAD and _conv(lib, N=-1) == BAD and b"N = -1" in err()
    for name in ("x", "w", "scale", "shift", "y"):
        assert _conv(lib, **{name: None}) == BAD and f"({name})".encode() in err(), name
    assert _conv(lib, N=2 ** 20, Ci=2, H=32, W=32) == BAD and b"2^31" in err()            # 2^31 input elements
    assert _conv(lib, N=2 ** 20, Ci=1, Co=2, H=32, W=32) == BAD                           # 2^31 elements before the pool
    assert _conv(lib, H=2 ** 31) == BAD and _conv(lib, N=2 ** 40) == BAD
    # N = 0 is a no-op whatever the pointers are; a bad scalar is an error whatever N is
    assert _conv(lib, N=0, x=None, w=None, scale=None, shift=None, y=None) == 0
    assert _conv(lib, N=0, Ci=0) == BAD and _conv(lib, N=0, pool=1, H=1) == BAD

    need = lib.snerf_smpl_estimator_workspace_bytes(1, 69)
    assert need == 4 * (1024 + 16 * 128 * 128 + 32 * 64 * 64) and lib.snerf_smpl_estimator_workspace_bytes(0, 2) == 4096
    assert lib.snerf_smpl_estimator_workspace_bytes(3, 2) == 4096 + 3 * (need - 4096)
    assert lib.snerf_smpl_estimator_workspace_bytes(-1, 69) == BAD and lib.snerf_smpl_estimator_workspace_bytes(1, 0) == BAD
    assert lib.snerf_smpl_estimator_workspace_bytes(8192, 69) == BAD and lib.snerf_smpl_estimator_workspace_bytes(8191, 69) > 0
    assert lib.snerf_smpl_estimator_fwd_f32(None, 8, 1, 8, 16, need, None) == BAD
    assert _fwd(lib, _net(human_size=0)) == BAD and b"human_size = 0" in err()
    assert _fwd(lib, _net(eps=-1e-5)) == BAD and b"eps" in err()
    assert _fwd(lib, _net(eps=[1e-5, 1e-5, float("nan"), 1e-5, 1e-5])) == BAD and b"bn3" in err()
    assert _fwd(lib, _net(eps=float("inf"))) == BAD
    assert _fwd(lib, _net(), ws_bytes=need - 1) == BAD and b"workspace" in err()
    assert _fwd(lib, _net(), ws=None) == BAD and b"workspace" in err()
    assert _fwd(lib, _net(), ws=8) == -2 and b"16-byte aligned" in err()                                # SNERF_E_ALIGN
    assert _fwd(lib, _net(), images=None) == BAD and _fwd(lib, _net(), out=None) == BAD
    for name in ("block0_weight", "block2_bias", "block4_running_var", "block1_bn_weight", "block3_bn_bias", "block0_running_mean",
                 "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias"):
        assert _fwd(lib, _net(**{name: True})) == BAD and b"null pointer" in err(), name
    assert _fwd(lib, _net(), N=-1) == BAD
    assert _fwd(lib, _net(fc1_weight=True), N=0, images=None, out=None, ws=None, ws_bytes=0) == 0      # N = 0: a no-op
    assert _fwd(lib, _net(eps=-1.0), N=0) == BAD


def test_cpu_tensors_are_refused_by_the_op():
    from smpl_nerf_amd import ops
    x, w, a = torch.rand(1, 3, 8, 8), torch.rand(16, 3, 3, 3), torch.ones(16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv3x3_block(x, w, a, a)


def test_normalize_image_and_validate_on_the_cpu():
    frames = np.random.default_rng(0).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    t = estimator.normalize_image(frames)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 128, 128)
    assert np.array_equal(t.numpy(), (frames / 255.).astype(np.float32).transpose(0, 3, 1, 2))
    one = estimator.normalize_image(frames[0])
    assert tuple(one.shape) == (3, 128, 128) and torch.equal(one, t[0])
    with pytest.raises(ValueError):
        estimator.normalize_image(frames[..., :2])
    # validate: the mean over the batches of the loss on columns 38 and 41, in eval mode, the mode restored afterwards
    s = ER.state(21, 2)
    model = estimator.SmplEstimator(2)
    model.load_state_dict(ER.tensors(s))
    truth = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (2, 69)).astype(np.float32))
    loader = [(t[:1], truth[:1]), (t[1:], truth[1:])]
    got = estimator.validate(model, loader)
    o64, _ = ER.forward64(s, t.numpy())
    want = np.mean([np.mean((o64[i] - truth[i, [38, 41]].double().numpy()) ** 2) for i in range(2)])
    assert model.training and abs(got - want) <= 1e-5 * want, (got, want)
    assert estimator.validate(model, []) == 0.0
