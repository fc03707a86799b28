"""SmplEstimator (models/smpl_estimator.py:6-47): image [N,3,128,128] -> pose [N,human_size].

The module has the reference's parameter and buffer names, so a model_smpl_estimator.pt written by the reference's save_run loads
with io.load_run, and the other way round.  On the GPU, in eval() mode with grad disabled, forward is ONE call of the library
(snerf_smpl_estimator_fwd_f32: the BatchNorm fold, five fused conv-BN-ReLU-pool launches, fc1, fc2).  On the GPU in training mode -
the only mode the reference's solver ever runs in - it is five ops.conv3x3_bn_block (csrc/conv_train.hip: batch statistics, the
weight and input gradients, the pool / ReLU / BatchNorm backward), nn.Dropout as torch ops on the [N,8192] and [N,500] rows, and
layered.linear for fc1 and fc2.  Everywhere else - CPU tensors, eval mode with grad enabled, momentum=None,
other dtypes - it is the reference's expression in torch ops.

train_epoch() and validate() are the two halves of SmplEstimatorSolver.train (solver/smpl_estimator_solver.py:52-68, :70-84);
normalize_image restates the data set's transform (datasets/transforms.py NormalizeRGBImage, smpl_estimator_dataset.py:78-80);
rendered_batches is a loader that renders its (image, pose) pairs on the spot (create_dataset.BodyRenderer).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, layered, ops
from ._lib import check, current_stream, ptr

CHANNELS = (3, 16, 32, 64, 64, 128)      # features in front of and behind each of the five blocks
POOL = (False, True, True, True, True)    # which blocks end in the 2 x 2 max pool
SIDE = 128                                # image extent: five blocks and four pools leave 8 x 8 x 128 = FLAT features
FLAT, HIDDEN = 8 * 8 * CHANNELS[-1], 500


def fold_bn(conv_bias, bn_weight, bn_bias, running_mean, running_var, eps):
    """(scale, shift) of ops.conv3x3_block for an eval-mode BatchNorm2d behind a convolution with bias, as the one-call entry folds
    them: float64, rounded once.  scale = gamma / sqrt(var + eps), shift = beta + (b - mean) scale."""
    scale = bn_weight.detach().double() / torch.sqrt(running_var.detach().double() + eps)
    shift = bn_bias.detach().double() + (conv_bias.detach().double() - running_mean.detach().double()) * scale
    return scale.float(), shift.float()


class SmplEstimator(nn.Module):

    def __init__(self, human_size=69):
        super().__init__()
        self.pool = nn.MaxPool2d(2, 2)
        for i in range(5):
            setattr(self, f"conv{i + 1}", nn.Conv2d(CHANNELS[i], CHANNELS[i + 1], 3, padding=1))
            setattr(self, f"bn{i + 1}", nn.BatchNorm2d(CHANNELS[i + 1]))
        self.fc1 = nn.Linear(FLAT, HIDDEN)
        self.dropout = nn.Dropout(0.25)
        self.fc2 = nn.Linear(HIDDEN, human_size)
        self.human_size = human_size
        self._workspaces = {}      # (device, N) -> uint8 workspace of the one-call forward

    def _blocks(self):
        return [(getattr(self, f"conv{i}"), getattr(self, f"bn{i}")) for i in range(1, 6)]

    def _forward_torch(self, images):
        """The network in torch ops, for every case the device path does not take.  In training mode BatchNorm2d normalises with the
        batch statistics and moves the running ones, and the dropout acts on the flattened features and on fc1's output."""
        h = images
        for (conv, bn), pooled in zip(self._blocks(), POOL):
            h = torch.relu(bn(conv(h)))
            if pooled:
                h = self.pool(h)
        h = self.dropout(h.reshape(-1, FLAT))      # [N, 128, 8, 8] -> [N, 8192], channel-major
        h = self.dropout(torch.relu(self.fc1(h)))
        return self.fc2(h)

    def _net(self):
        """struct snerf_smpl_estimator of the parameters as they lie now (pointers only: the fold happens on the device, per call)."""
        net = _lib.SmplEstimatorNet()
        for i, (conv, bn) in enumerate(self._blocks()):
            tensors = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
            for t in tensors:
                if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError("SmplEstimator: the device path needs contiguous fp32 GPU parameters and BatchNorm2d with "
                                       "affine weights and running statistics")
            net.block[i] = _lib.ConvBn(*(ptr(t) for t in tensors), float(bn.eps))
        for t in (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("SmplEstimator: the device path needs contiguous fp32 GPU parameters")
        net.fc1_weight, net.fc1_bias, net.fc2_weight, net.fc2_bias = (ptr(t) for t in (self.fc1.weight, self.fc1.bias, self.fc2.weight,
                                                                                       self.fc2.bias))
        net.human_size = self.fc2.out_features
        return net

    def _forward_device(self, x):
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, SIDE, SIDE) or x.dtype != torch.float32:
            raise RuntimeError(f"SmplEstimator: the device path takes fp32 images [N,3,{SIDE},{SIDE}], got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        N, hs = x.shape[0], self.fc2.out_features
        lib = _lib.load()
        key = (x.device, N)
        if key not in self._workspaces:
            nbytes = lib.snerf_smpl_estimator_workspace_bytes(N, hs)
            if nbytes < 0:
                check(-1, "snerf_smpl_estimator_workspace_bytes")
            self._workspaces[key] = torch.empty((nbytes,), device=x.device, dtype=torch.uint8)
        ws = self._workspaces[key]
        out = torch.empty((N, hs), device=x.device, dtype=torch.float32)
        net = self._net()
        with torch.cuda.device(x.device), _lib.timed(f"smpl_estimator_fwd[{N}]"):
            check(lib.snerf_smpl_estimator_fwd_f32(net, ptr(x), N, ptr(out), ptr(ws), ws.numel(), current_stream()),
                  "snerf_smpl_estimator_fwd_f32")
        return out

    def _trains_on_device(self, x):
        """Whether the training-mode device path takes x: fp32 GPU images [N,3,128,128], N >= 1, contiguous fp32 GPU parameters,
        BatchNorm2d with affine weights, running statistics and a float momentum."""
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, SIDE, SIDE) or x.shape[0] < 1 or x.dtype != torch.float32:
            return False
        for conv, bn in self._blocks():
            if bn.momentum is None or not bn.track_running_stats or not bn.affine:
                return False
            for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var):
                if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                    return False
        return all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                   for t in (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias))

    def _forward_train_device(self, x):
        """Training mode on the library's kernels: per block one ops.conv3x3_bn_block (which moves the running statistics) and the
        step of num_batches_tracked that nn.BatchNorm2d makes; the dropout of the reference's two places in torch ops."""
        h = x.contiguous()
        for (conv, bn), pooled in zip(self._blocks(), POOL):
            h = ops.conv3x3_bn_block(h, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=bn.momentum,
                                     eps=bn.eps, relu=True, pool=pooled)
            bn.num_batches_tracked.add_(1)
        h = self.dropout(h.reshape(-1, FLAT))
        h = self.dropout(layered.linear([(h, self.fc1.weight)], self.fc1.bias, relu=True))
        return layered.linear([(h, self.fc2.weight)], self.fc2.bias)

    def forward(self, x):
        if x.is_cuda and not self.training and not torch.is_grad_enabled():
            return self._forward_device(x)
        if x.is_cuda and self.training and self._trains_on_device(x):
            return self._forward_train_device(x)
        return self._forward_torch(x)

    @property
    def is_cuda(self):
        """True when the parameters live on a GPU (the attribute the reference's solvers ask a model for)."""
        return self.fc2.weight.is_cuda

    def save(self, path):
        """Pickles the WHOLE module to `path`, as the reference's models do in their save(); io.save_run writes the state_dict."""
        print(f"SmplEstimator: writing the module to {path}")
        torch.save(self, path)

    def __getstate__(self):      # (the cached workspaces are not part of a saved model)
        state = self.__dict__.copy()
        state["_workspaces"] = {}
        return state


def normalize_image(frames):
    """The data set's transform for this model: 8-bit frames [H,W,3] or [F,H,W,3] (io.load_dataset's BGR frames; the channel order
    stays, as in the reference) -> float32 tensor [3,H,W] or [F,3,H,W] with values in [0, 1].  The quotient by 255 is taken in
    float64 and rounded once, which is what the reference's numpy expression does."""
    frames = np.asarray(frames)
    if frames.ndim not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError(f"normalize_image: expected [H,W,3] or [F,H,W,3], got {frames.shape}")
    unit = np.true_divide(frames, 255.0, dtype=np.float64).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(unit, -1, -3)))


def rendered_batches(renderer, pose_sampler, transforms, betas, batch_size: int, steps: int):
    """An endless-data-set stand-in for the loader of train_epoch: `steps` batches of (images [batch_size,3,H,W] fp32, poses
    [batch_size,69] fp32), both on the renderer's device, rendered on the spot - no disk, no host copy of a frame.  renderer: a
    create_dataset.BodyRenderer; pose_sampler(batch_size) -> body poses [batch_size,69] (array or tensor); transforms [n,4,4]: the
    camera path, walked cyclically frame by frame.  The images are what normalize_image makes of the frames as io.load_dataset would
    read them back: BGR, the quotient by 255 taken in float64 and rounded once."""
    transforms = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
    for step in range(int(steps)):
        poses = pose_sampler(int(batch_size))
        poses = torch.as_tensor(np.asarray(poses) if not isinstance(poses, torch.Tensor) else poses, dtype=torch.float32,
                                device=renderer.device).reshape(int(batch_size), -1)
        cams = transforms[(step * int(batch_size) + np.arange(int(batch_size))) % len(transforms)]
        rgb = renderer.frames(cams, poses, betas)[0]
        yield rgb.flip(-1).permute(0, 3, 1, 2).double().div_(255.0).float().contiguous(), poses


def train_epoch(model, loader, optim, loss_func=None, log_iterations=None):
    """The training loop of SmplEstimatorSolver.train (:52-68) for one epoch: per batch the forward in training mode, zero_grad, the
    loss (nn.MSELoss unless given), backward and the step of `optim` (any torch optimiser over model.parameters()), on the model's
    device - on the GPU the forward and the backward run on the library's kernels.  A model with two outputs is scored against
    columns 38 and 41 of the 69-vector truth (:56).  Every log_iterations-th batch prints the reference's line.  The model is put
    into train() mode and stays there.  Returns the mean loss over the batches as a float (0.0 for an empty loader)."""
    criterion = nn.MSELoss() if loss_func is None else loss_func
    device = model.fc2.weight.device
    two_angles = model.fc2.out_features == 2
    model.train()
    total, batches = 0.0, 0
    for i, (images, truth) in enumerate(loader):
        images, truth = images.to(device), truth.to(device)
        if two_angles:
            truth = truth[:, [38, 41]]
        pose = model(images)
        optim.zero_grad()
        loss = criterion(pose, truth)
        loss.backward()
        item = loss.item()
        optim.step()
        if log_iterations and i % log_iterations == log_iterations - 1:
            print('[Iteration %5d] TRAIN loss: %.7f' % (i + 1, item))
        total += item
        batches += 1
    return total / max(batches, 1)


def validate(model, loader, loss_func=None):
    """The validation loop of SmplEstimatorSolver.train (:70-84): the mean over the loader's batches of loss_func(model(images), truth)
    under no_grad, on the model's device.  The model is put into eval() mode for the loop and back afterwards (the reference never
    leaves training mode, so its validation draws dropout masks and moves the running statistics; a validation loss should do
    neither), so on the GPU every batch is one library call.  A model with two outputs is scored against columns 38 and 41 of the
    69-vector truth (:79).  Returns a float (0.0 for an empty loader)."""
    criterion = nn.MSELoss() if loss_func is None else loss_func
    device = model.fc2.weight.device
    two_angles = model.fc2.out_features == 2
    total, batches, was_training = 0.0, 0, model.training
    model.eval()
    try:
        with torch.no_grad():
            for images, truth in loader:
                images, truth = images.to(device), truth.to(device)
                if two_angles:
                    truth = truth[:, [38, 41]]
                total += float(criterion(model(images), truth))
                batches += 1
    finally:
        model.train(was_training)
    return total / max(batches, 1)
