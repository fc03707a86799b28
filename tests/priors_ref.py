"""The seeded inputs of the prior tests (tests/test_priors_host.py) and of their golden's generator (tests/golden/make_golden_priors.py)."""
import hashlib

import numpy as np

SEED, M, D, B = 27, 6, 69, 5


def priors_mixture(seed=SEED):
    """(means [6,69], covars [6,69,69], weights [6]) float64: well-conditioned covariances of different determinants."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, D, D)) * 0.08
    covars = A @ A.transpose(0, 2, 1) + (0.04 + 0.02 * np.arange(M))[:, None, None] * np.eye(D)
    weights = rng.random(M) + 0.2
    return rng.standard_normal((M, D)) * 0.3, covars, weights / weights.sum()


def priors_poses(seed=SEED):
    """pose [B,72] float64 (global orientation in front), betas [B,10]"""
    rng = np.random.default_rng(seed + 1)
    return rng.standard_normal((B, D + 3)) * 0.4, rng.standard_normal((B, 10))


def checksum(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in arrays)).hexdigest()
