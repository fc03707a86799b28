"""Restatement of SmplEstimator's eval-mode forward (models/smpl_estimator.py:32-47) and of one fused block of it, in torch CPU
ops - the yardstick of tests/test_smpl_estimator_host.py, test_gpu_conv_block.py and test_gpu_smpl_estimator.py.

  state(seed, human_size)   a numpy-seeded fp32 parameter set under the state_dict's names
  images(seed, N)           uniform [0, 1) fp32 [N,3,128,128]
  block64 / block32         y = [maxpool2x2](relu(scale conv3x3_pad1(x, w) + shift)): the library's fused block, unfused, in
                            float64 / in fp32 (the product by scale, then the sum with shift, as the kernel's epilogue)
  forward64 / forward32     the network: convolution with bias, BatchNorm on the running statistics, ReLU, pool, flatten, fc1, ReLU,
                            fc2 - unfused and in the reference's op order, in float64 / in fp32.  Returns (out, [the five block outputs]).

Accuracy rule (as for the other fused ops): E = max|y - y64| / max|y64|; a kernel's E may be at most
FACTOR = 8 times the E of the fp32 CPU restatement on the same inputs."""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (3, 16, 32, 64, 64, 128)
POOL = (False, True, True, True, True)
EPS = 1e-5           # nn.BatchNorm2d's default
FACTOR = 8.0
KEYS = [f"{m}{i}.{k}" for i in range(1, 6) for m, ks in (("conv", ("weight", "bias")),
                                                          ("bn", ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")))
        for k in ks] + ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def state(seed, human_size=69):
    """conv / fc weights normal with std 1 / sqrt(fan_in), biases within +-0.1, BN weight in [0.5, 1.5], bias within +-0.1,
    running_mean within +-0.2, running_var in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    s = {}
    for i in range(5):
        ci, co = CHANNELS[i], CHANNELS[i + 1]
        s[f"conv{i + 1}.weight"] = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(f32)
        s[f"conv{i + 1}.bias"] = rng.uniform(-0.1, 0.1, co).astype(f32)
        s[f"bn{i + 1}.weight"] = rng.uniform(0.5, 1.5, co).astype(f32)
        s[f"bn{i + 1}.bias"] = rng.uniform(-0.1, 0.1, co).astype(f32)
        s[f"bn{i + 1}.running_mean"] = rng.uniform(-0.2, 0.2, co).astype(f32)
        s[f"bn{i + 1}.running_var"] = rng.uniform(0.5, 2.0, co).astype(f32)
        s[f"bn{i + 1}.num_batches_tracked"] = np.array(7, np.int64)
    for name, (fo, fi) in (("fc1", (500, 8 * 8 * 128)), ("fc2", (human_size, 500))):
        s[f"{name}.weight"] = (rng.standard_normal((fo, fi)) / np.sqrt(fi)).astype(f32)
        s[f"{name}.bias"] = rng.uniform(-0.1, 0.1, fo).astype(f32)
    assert list(s) == KEYS
    return s


def images(seed, N):
    return np.random.default_rng(seed).uniform(0, 1, (N, 3, 128, 128)).astype(np.float32)


def tensors(s):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}


def _block(x, w, scale, shift, relu, pool, dtype):
    x, w, scale, shift = (torch.as_tensor(a).to(dtype) for a in (x, w, scale, shift))
    with torch.no_grad():
        y = F.conv2d(x, w, None, padding=1)
        y = y * scale[None, :, None, None]
        y = y + shift[None, :, None, None]
        if relu:
            y = F.relu(y)
        if pool:
            y = F.max_pool2d(y, 2, 2)
    return y.numpy()


def block64(x, w, scale, shift, relu=True, pool=False):
    return _block(x, w, scale, shift, relu, pool, torch.float64)


def block32(x, w, scale, shift, relu=True, pool=False):
    return _block(x, w, scale, shift, relu, pool, torch.float32)


def _forward(s, x, dtype):
    p = {k: torch.as_tensor(v).to(dtype) for k, v in s.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(x).to(dtype)
    blocks = []
    with torch.no_grad():
        for i in range(1, 6):
            x = F.conv2d(x, p[f"conv{i}.weight"], p[f"conv{i}.bias"], padding=1)
            x = F.batch_norm(x, p[f"bn{i}.running_mean"], p[f"bn{i}.running_var"], p[f"bn{i}.weight"], p[f"bn{i}.bias"], False, 0.1, EPS)
            x = F.relu(x)
            if POOL[i - 1]:
                x = F.max_pool2d(x, 2, 2)
            blocks.append(x.numpy())
        x = x.reshape(-1, 8 * 8 * 128)
        x = F.relu(F.linear(x, p["fc1.weight"], p["fc1.bias"]))
        x = F.linear(x, p["fc2.weight"], p["fc2.bias"])
    return x.numpy(), blocks


def forward64(s, x):
    return _forward(s, x, torch.float64)


def forward32(s, x):
    return _forward(s, x, torch.float32)


def fold64(s, i):
    """(scale, shift) of block i = 1 .. 5 in float64, rounded once to fp32: what the one-call entry computes on the device."""
    g, b, m, v, cb = (s[k].astype(np.float64) for k in (f"bn{i}.weight", f"bn{i}.bias", f"bn{i}.running_mean", f"bn{i}.running_var", f"conv{i}.bias"))
    scale = g / np.sqrt(v + EPS)
    return scale.astype(np.float32), (b + (cb - m) * scale).astype(np.float32)


def E(y, y64):
    """max abs error over max abs of the float64 result (0 where both are empty or the result is all zeros and so is y)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    assert y.shape == y64.shape, (y.shape, y64.shape)
    if y64.size == 0:
        return 0.0
    top = np.abs(y64).max()
    err = np.abs(y - y64).max()
    return float(err / top) if top > 0 else float(err)


GOLDEN = "g24_smpl_estimator.npz"
GOLDEN_SEED, GOLDEN_IMAGE_SEED, GOLDEN_N = 2401, 2402, 2
