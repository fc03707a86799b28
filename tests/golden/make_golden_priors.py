#!/usr/bin/env python3
"""Golden vectors for the SMPLify priors (smpl_nerf_amd/priors.py) from the reference's own classes (util/prior.py).
    python tests/golden/make_golden_priors.py    # writes g27_priors.npz
A seeded 6 x 69 mixture (tests/priors_ref.py; the file the reference's constructor reads is written to a temporary folder) and
seeded poses go through MaxMixturePrior (merged form), SMPLifyAnglePrior with and without the global pose and L2Prior, in fp32 and
in float64.  Stored: the seed, a checksum of the mixture, the poses, the outputs and the pose gradients of the summed outputs.  The
mixture itself is rebuilt from the seed by the test."""
import os
import pickle
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

from make_golden import REF
from priors_ref import SEED, M, checksum, priors_mixture, priors_poses

def main():
    sys.path.insert(0, REF)
    from util import prior as P
    means, covars, weights = priors_mixture()
    pose72, betas = priors_poses()
    g = {"seed": np.array(SEED), "checksum": np.array(checksum((means, covars, weights))), "pose": pose72, "betas": betas}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "gmm_06.pkl"), "wb") as f:
            pickle.dump({"means": means, "covars": covars, "weights": weights}, f)
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            gmm = P.create_prior("gmm", prior_folder=tmp, num_gaussians=M, dtype=dt)
            angle, l2 = P.create_prior("angle", dtype=dt), P.create_prior("l2", dtype=dt)
            cases = {"gmm": lambda x: gmm(x[:, 3:], torch.from_numpy(betas).to(dt)), "angle": lambda x: angle(x[:, 3:]),
                     "angle_global": lambda x: angle(x, with_global_pose=True), "l2": lambda x: l2(x[:, 3:])}
            for name, fn in cases.items():
                x = torch.from_numpy(pose72).to(dt).requires_grad_(True)
                y = fn(x)
                y.sum().backward()
                g[f"{name}_{tag}"], g[f"{name}_grad_{tag}"] = y.detach().numpy(), x.grad.numpy()
    np.savez(os.path.join(HERE, "g27_priors.npz"), **g)
    print({k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
