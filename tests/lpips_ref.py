"""LPIPS restated in torch CPU ops (util/scores.py:286-456 as LPIPS() configures ContentLoss) - the yardstick of
tests/test_lpips_host.py and tests/test_gpu_lpips.py - and the seeded weights both they and tests/golden/make_golden_lpips.py use.

  weights(seed, channels)     np.random.RandomState(seed): per convolution a He-scaled normal weight [Co,Ci,3,3] (std sqrt(2 / (9 Ci)))
                              and a bias 0.1 x normal [Co], in VGG16 order; then per stage lin = |normal| [C].  fp32.
  checksum(w)                 the float64 sum of all of them: a drift of the recipe shows here, not as a parity failure
  images(seed, N, H, W)       x, y uniform [0, 1) fp32 [N,3,H,W]
  tap64 / tap32               (relu(conv3x3_pad1(x, w) scale + shift), its 2 x 2 max) in float64 / fp32
  distance64 / distance32     one tap's term: mean_p sum_c wl[c] (x^ - y^)^2, x^ = fx / (sqrt(sum_c fx^2) + 1e-10) with normalize
  metric64 / metric32         the whole metric -> layers [N,5] (their sum over the stages is the reference's per-image loss); the
                              standardisation, 13 convolutions with bias and ReLU, pools after the first four taps (pool5's output is
                              unused and not computed, so frames from 16 x 16 run)

Accuracy rule: E = max|v - v64| / max|v64|; a kernel's E may be at most smpl_estimator_ref.FACTOR = 8 times
the E of the fp32 restatement on the same inputs."""
import numpy as np
import torch
import torch.nn.functional as F

STAGES = (2, 2, 3, 3, 3)
FULL = (64, 128, 256, 512, 512)
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # in torchvision's vgg16().features
TAPS = ('3', '8', '15', '22', '29')                                  # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]
EPS = 1e-10

GOLDEN = "g26_lpips.npz"
# name -> (channels, H, W, N, weight seed, image seed, x == y)
CASES = {
    "odd": ((3, 5, 7, 9, 11), 32, 47, 3, 2601, 2611, False),
    "mid": ((8, 16, 24, 40, 40), 35, 50, 2, 2602, 2612, False),
    "full32": (FULL, 32, 32, 1, 2603, 2613, False),
    "full": (FULL, 33, 48, 2, 2604, 2614, False),
    "same": ((3, 5, 7, 9, 11), 32, 47, 2, 2601, 2615, True),
}


def weights(seed, channels):
    """{"conv": [(w, b)] x 13, "lin": [v] x 5}"""
    rng = np.random.RandomState(seed)
    convs, ci = [], 3
    for co, n in zip(channels, STAGES):
        for _ in range(n):
            w = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2. / (9 * ci))).astype(np.float32)
            b = (0.1 * rng.standard_normal(co)).astype(np.float32)
            convs.append((w, b))
            ci = co
    return {"conv": convs, "lin": [np.abs(rng.standard_normal(co)).astype(np.float32) for co in channels]}


def checksum(w):
    return float(sum(a.astype(np.float64).sum() + b.astype(np.float64).sum() for a, b in w["conv"]) + sum(v.astype(np.float64).sum() for v in w["lin"]))


def images(seed, N, H, W, same=False):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    y = x.copy() if same else rng.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    return x, y


def features_state(w):
    """The state_dict of the equivalent nn.Sequential (torchvision's .features keys: '<i>.weight', '<i>.bias')."""
    s = {}
    for i, (a, b) in zip(CONV_INDEX, w["conv"]):
        s[f"{i}.weight"], s[f"{i}.bias"] = torch.from_numpy(a), torch.from_numpy(b)
    return s


def _tap(x, w, scale, shift, relu, dtype):
    x, w, scale, shift = (torch.as_tensor(a).to(dtype) for a in (x, w, scale, shift))
    with torch.no_grad():
        y = F.conv2d(x, w, None, padding=1)
        y = y * scale[None, :, None, None]
        y = y + shift[None, :, None, None]
        if relu:
            y = F.relu(y)
        p = F.max_pool2d(y, 2, 2) if min(y.shape[-2:]) >= 2 else None
    return y.numpy(), (None if p is None else p.numpy())


def tap64(x, w, scale, shift, relu=True):
    return _tap(x, w, scale, shift, relu, torch.float64)


def tap32(x, w, scale, shift, relu=True):
    return _tap(x, w, scale, shift, relu, torch.float32)


def _normalize(x):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + EPS)      # scores.py:410-411


def _distance(fx, fy, wl, normalize, dtype):
    fx, fy, wl = (torch.as_tensor(a).to(dtype) for a in (fx, fy, wl))
    with torch.no_grad():
        if normalize:
            fx, fy = _normalize(fx), _normalize(fy)
        d = (fx - fy) ** 2                                                       # nn.MSELoss(reduction='none')
        return (d * wl.view(1, -1, 1, 1)).mean(dim=[2, 3]).sum(dim=1).numpy()   # scores.py:372


def distance64(fx, fy, wl, normalize=True):
    return _distance(fx, fy, wl, normalize, torch.float64)


def distance32(fx, fy, wl, normalize=True):
    return _distance(fx, fy, wl, normalize, torch.float32)


def standardize(x, dtype=torch.float32, mean=MEAN, std=STD):
    x = torch.as_tensor(x).to(dtype)
    return (x - torch.tensor(mean).view(1, -1, 1, 1).to(x)) / torch.tensor(std).view(1, -1, 1, 1).to(x)      # scores.py:348-351, 394


def _metric(w, x, y, dtype, mean=MEAN, std=STD):
    def feats(v):
        v = standardize(v, dtype, mean, std)
        out, i = [], 0
        for l, n in enumerate(STAGES):
            for _ in range(n):
                a, b = w["conv"][i]
                v = F.relu(F.conv2d(v, torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype), padding=1))
                i += 1
            out.append(_normalize(v))
            if l < 4:
                v = F.max_pool2d(v, 2, 2)
        return out
    with torch.no_grad():
        fx, fy = feats(x), feats(y)
        cols = [(((a - b) ** 2) * torch.from_numpy(v).to(dtype).view(1, -1, 1, 1)).mean(dim=[2, 3]).sum(dim=1) for a, b, v in zip(fx, fy, w["lin"])]
        return torch.stack(cols, dim=1).numpy()


def metric64(w, x, y, **kw):
    return _metric(w, x, y, torch.float64, **kw)


def metric32(w, x, y, **kw):
    return _metric(w, x, y, torch.float32, **kw)


def E(v, v64):
    """max abs error over max abs of the float64 result (the plain max abs error where that result is all zeros)."""
    v, v64 = np.asarray(v, np.float64), np.asarray(v64, np.float64)
    assert v.shape == v64.shape, (v.shape, v64.shape)
    if v64.size == 0:
        return 0.0
    top, err = np.abs(v64).max(), np.abs(v - v64).max()
    return float(err / top) if top > 0 else float(err)
