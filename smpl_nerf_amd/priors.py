"""The SMPLify pose priors that keep a silhouette fit plausible (Bogo et al. 2016, "Keep it SMPL"), with the call signatures of the
reference's util/prior.py, written from the formulas in torch ops - a [B, 6, 69] problem is no kernel:

  MaxMixturePrior    min_m ( 1/2 (pose - mean_m)^T P_m (pose - mean_m) - log w'_m ),  P_m = inverse(cov_m),
                     w'_m = weight_m / ((2 pi)^(D/2) sqrt(det cov_m) / min_k sqrt(det cov_k)),  D = 69                       -> [B]
  SMPLifyAnglePrior  exp(sign pose[:, idx])^2 for the four bending angles of elbows and knees: idx = (55, 58, 12, 15) of the pose
                     with the global orientation in front, 3 less without; signs (+, -, -, -)                                 -> [B,4]
  L2Prior            sum(x^2)                                                                                                 -> scalar

Only the merged form of the mixture prior is built; use_merged=False is refused.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch


class L2Prior(torch.nn.Module):
    def __init__(self, dtype=torch.float32, reduction="sum", **kwargs):
        super().__init__()

    def forward(self, module_input, *args):
        return module_input.pow(2).sum()


class SMPLifyAnglePrior(torch.nn.Module):
    def __init__(self, dtype=torch.float32, **kwargs):
        super().__init__()
        self.register_buffer("angle_prior_idxs", torch.tensor([55, 58, 12, 15], dtype=torch.long))
        self.register_buffer("angle_prior_signs", torch.tensor([1, -1, -1, -1], dtype=dtype))

    def forward(self, pose, with_global_pose=False):
        idx = self.angle_prior_idxs if with_global_pose else self.angle_prior_idxs - 3
        return torch.exp(pose[:, idx] * self.angle_prior_signs).pow(2)


class MaxMixturePrior(torch.nn.Module):
    """MaxMixturePrior(prior_folder, num_gaussians) reads prior_folder/gmm_{num_gaussians:02d}.pkl as the reference does;
    from_file(path) reads any `.npz` or `.pkl` that holds means [M,D], covars [M,D,D] and weights [M]; from_arrays takes them
    directly.  Precisions, determinants and the merged weights are computed on the host as the reference's constructor computes
    them - the inverse in the working dtype's numpy type, the determinants in float64 - and then held in `dtype`."""

    def __init__(self, prior_folder="prior", num_gaussians=6, dtype=torch.float32, epsilon=1e-16, use_merged=True, **kwargs):
        super().__init__()
        if "_arrays" in kwargs:
            means, covars, weights = kwargs["_arrays"]
        else:
            means, covars, weights = self._read(os.path.join(prior_folder, "gmm_{:02d}.pkl".format(num_gaussians)))
        if not use_merged:
            raise NotImplementedError("MaxMixturePrior: only the merged form (use_merged=True) is built")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"MaxMixturePrior: dtype must be float32 or float64, got {dtype}")
        np_dtype = np.float32 if dtype == torch.float32 else np.float64
        means, covars, weights = np.asarray(means), np.asarray(covars), np.asarray(weights)
        if means.ndim != 2 or covars.shape != (means.shape[0], means.shape[1], means.shape[1]) or weights.shape != (means.shape[0],):
            raise ValueError(f"MaxMixturePrior: means {means.shape}, covars {covars.shape} and weights {weights.shape} must be [M,D], [M,D,D], [M]")
        self.num_gaussians, self.epsilon, self.use_merged = means.shape[0], epsilon, True
        self.random_var_dim = means.shape[1]
        covs = covars.astype(np_dtype)
        self.register_buffer("means", torch.tensor(means.astype(np_dtype), dtype=dtype))
        self.register_buffer("covs", torch.tensor(covs, dtype=dtype))
        self.register_buffer("precisions", torch.tensor(np.stack([np.linalg.inv(c) for c in covs]).astype(np_dtype), dtype=dtype))
        sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in covars])
        const = (2 * np.pi) ** (self.random_var_dim / 2.)
        self.register_buffer("nll_weights", torch.tensor(np.asarray(weights / (const * (sqrdets / sqrdets.min()))), dtype=dtype)[None])
        self.register_buffer("weights", torch.tensor(weights, dtype=dtype)[None])

    @staticmethod
    def _read(path):
        path = str(path)
        if not os.path.exists(path):
            raise FileNotFoundError(f"MaxMixturePrior: the mixture file {path} does not exist")
        if path.endswith(".npz"):
            d = dict(np.load(path, allow_pickle=False))
        else:
            with open(path, "rb") as f:
                d = pickle.load(f, encoding="latin1")
        if not isinstance(d, dict) or any(k not in d for k in ("means", "covars", "weights")):
            raise ValueError(f"MaxMixturePrior: {path} must hold a dict of means, covars and weights")
        return d["means"], d["covars"], d["weights"]

    @classmethod
    def from_arrays(cls, means, covars, weights, dtype=torch.float32, epsilon=1e-16):
        return cls(dtype=dtype, epsilon=epsilon, _arrays=(means, covars, weights))

    @classmethod
    def from_file(cls, path, dtype=torch.float32, epsilon=1e-16):
        return cls.from_arrays(*cls._read(path), dtype=dtype, epsilon=epsilon)

    def get_mean(self):
        return self.weights @ self.means

    def merged_log_likelihood(self, pose, betas=None):
        d = pose[:, None] - self.means                                             # [B,M,D]
        quad = (torch.einsum("mij,bmj->bmi", self.precisions, d) * d).sum(-1)      # [B,M]
        return (0.5 * quad - torch.log(self.nll_weights)).min(1).values

    def forward(self, pose, betas=None):
        return self.merged_log_likelihood(pose, betas)


def create_prior(prior_type, **kwargs):
    """'gmm' -> MaxMixturePrior, 'l2' -> L2Prior, 'angle' -> SMPLifyAnglePrior, 'none' / None -> a function that returns 0.0."""
    if prior_type == "gmm":
        return MaxMixturePrior(**kwargs)
    if prior_type == "l2":
        return L2Prior(**kwargs)
    if prior_type == "angle":
        return SMPLifyAnglePrior(**kwargs)
    if prior_type == "none" or prior_type is None:
        return lambda *args, **kwargs: 0.0
    raise ValueError(f"Prior {prior_type} is not implemented")
