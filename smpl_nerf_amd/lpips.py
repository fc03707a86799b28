"""LPIPS on the device (util/scores.py:423-456): the weights of VGG16's feature stack and of the reference's lpips_weights.pt as a
module that ops.lpips, ops.image_scores and DataParallelTrainer.validate_scores take.

The reference's LPIPS() downloads both sets of weights in its constructor.  Nothing is downloaded here: the weights come from files
the user already has - torchvision's vgg16 checkpoint (or the state_dict of its .features) and lpips_weights.pt.

    net = VggLpips.from_files("vgg16-397923af.pth", "lpips_weights.pt").cuda()
    ops.lpips(x, y, net)                      # x, y [N,3,H,W] in [0, 1]
    ops.image_scores(renders, truths, lpips=net)["lpips"]
    net.loss(render, truth).backward()        # ops.lpips_loss: the same value as a training loss, differentiable to the frames
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib

IMAGENET_MEAN = [0.485, 0.456, 0.406]      # scores.py:175-176
IMAGENET_STD = [0.229, 0.224, 0.225]
VGG16_STAGES = (2, 2, 3, 3, 3)             # convolutions per stage
# the convolutions' indices in torchvision's vgg16().features (scores.py:182-201); the taps follow the last convolution of a stage
VGG16_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)


class VggLpips(nn.Module):
    """The 13 convolutions (buffers conv<i>_weight [Co,Ci,3,3], conv<i>_bias [Co], i = 0 .. 12 in VGG16 order), the five channel
    weights lin<l> [channels[l]] and the input standardisation.  Any channel count of 1 .. 512 per stage: the real net is
    64, 128, 256, 512, 512.  The tensors are buffers, nothing here is trained: forward() is the score, loss() the same value under autograd."""

    def __init__(self, convs, lin, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        super().__init__()
        if len(convs) != 13 or len(lin) != 5:
            raise ValueError(f"VggLpips: 13 convolutions and 5 lin vectors, got {len(convs)} and {len(lin)}")
        channels, ci, i = [], 3, 0
        for l, n in enumerate(VGG16_STAGES):
            co = int(convs[i][0].shape[0])
            for _ in range(n):
                w, b = convs[i]
                if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
                    raise ValueError(f"VggLpips: convolution {i} of stage {l + 1} must be [{co},{ci},3,3] with bias [{co}], got "
                                     f"{tuple(w.shape)} and {tuple(b.shape)}")
                self.register_buffer(f"conv{i}_weight", w.detach().to(torch.float32).contiguous().clone())
                self.register_buffer(f"conv{i}_bias", b.detach().to(torch.float32).contiguous().clone())
                ci, i = co, i + 1
            if not 1 <= co <= 512:
                raise ValueError(f"VggLpips: stage {l + 1} has {co} channels, outside 1 .. 512")
            v = torch.as_tensor(lin[l]).detach().to(torch.float32).reshape(-1).contiguous().clone()
            if v.numel() != co:
                raise ValueError(f"VggLpips: lin[{l}] must flatten to [{co}], got {tuple(torch.as_tensor(lin[l]).shape)}")
            self.register_buffer(f"lin{l}", v)
            channels.append(co)
        self.channels = tuple(channels)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("VggLpips: mean and std have three values each")

    @classmethod
    def from_state(cls, vgg_state, lin_weights, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """vgg_state: torchvision's vgg16 checkpoint (keys features.<i>.weight / .bias; classifier.* is ignored) or the state_dict
        of its .features (keys <i>.weight / .bias).  lin_weights: the list of five tensors of the reference's lpips_weights.pt, in
        any shape that flattens to [C] ([C], [1,C,1,1], [C,1,1])."""
        prefix = "features." if any(k.startswith("features.") for k in vgg_state) else ""
        convs = []
        for i in VGG16_CONV_INDEX:
            kw, kb = f"{prefix}{i}.weight", f"{prefix}{i}.bias"
            if kw not in vgg_state or kb not in vgg_state:
                raise KeyError(f"VggLpips.from_state: the VGG16 state has no `{kw}` / `{kb}`")
            convs.append((torch.as_tensor(vgg_state[kw]), torch.as_tensor(vgg_state[kb])))
        lin = list(lin_weights.values()) if isinstance(lin_weights, dict) else list(lin_weights)
        return cls(convs, lin, mean, std)

    @classmethod
    def from_files(cls, vgg_path, lin_path, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """from_state on two local files (torch.load with weights_only=True).  Nothing is downloaded: a missing file is an error."""
        for what, path in (("the VGG16 checkpoint", vgg_path), ("the LPIPS linear weights", lin_path)):
            if not os.path.isfile(path):
                raise FileNotFoundError(f"VggLpips.from_files: {what} `{path}` does not exist (nothing is downloaded: torchvision's "
                                        "vgg16 checkpoint and the reference's lpips_weights.pt must be local files)")
        return cls.from_state(torch.load(vgg_path, map_location="cpu", weights_only=True),
                              torch.load(lin_path, map_location="cpu", weights_only=True), mean, std)

    def record(self, device):
        """struct snerf_vgg_lpips over this module's buffers, which must live on `device`."""
        rec = _lib.VggLpipsNet()
        for name, t in self.named_buffers():
            if t.device != device:
                raise RuntimeError(f"VggLpips: `{name}` is on {t.device}, the frames on {device}")
        for i in range(13):
            rec.conv[i] = _lib.ConvWb(getattr(self, f"conv{i}_weight").data_ptr(), getattr(self, f"conv{i}_bias").data_ptr())
        for l in range(5):
            rec.channels[l] = self.channels[l]
            rec.lin[l] = getattr(self, f"lin{l}").data_ptr()
            if l < 3:
                rec.mean[l], rec.std[l] = self.mean[l], self.std[l]
        return rec

    def forward(self, x, y, reduction: str = 'mean'):
        from . import ops
        return ops.lpips(x, y, self, reduction=reduction)

    def loss(self, x, y, reduction: str = 'mean'):
        """ops.lpips_loss: the same value, differentiable with respect to the frames; the buffers here stay constants."""
        from . import ops
        return ops.lpips_loss(x, y, self, reduction=reduction)
