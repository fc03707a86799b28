"""The SMPLify priors (smpl_nerf_amd/priors.py) against the reference's own classes: tests/golden/g27_priors.npz holds what
util/prior.py returns, in fp32 and in float64, for the seeded mixture and poses of tests/priors_ref.py.  float64 must agree to
1e-12; fp32 to 8 times the reference's own fp32-to-float64 error.  No GPU needed."""
import os
import pickle

import numpy as np
import pytest
import torch

import priors_ref as PR
from conftest import load_golden
from smpl_nerf_amd import priors as P

DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def g():
    g = load_golden("g27_priors.npz")
    assert int(g["seed"]) == PR.SEED and str(g["checksum"]) == PR.checksum(PR.priors_mixture())     # the mixture the golden was made on
    assert np.array_equal(g["pose"], PR.priors_poses()[0])
    return g


def rel(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


def cases(dt):
    gmm = P.MaxMixturePrior.from_arrays(*PR.priors_mixture(), dtype=dt)
    angle, l2 = P.create_prior("angle", dtype=dt), P.create_prior("l2", dtype=dt)
    betas = torch.from_numpy(PR.priors_poses()[1]).to(dt)
    return {"gmm": lambda x: gmm(x[:, 3:], betas), "angle": lambda x: angle(x[:, 3:]),
            "angle_global": lambda x: angle(x, with_global_pose=True), "l2": lambda x: l2(x[:, 3:])}


@pytest.mark.parametrize("name", ["gmm", "angle", "angle_global", "l2"])
def test_against_the_reference(g, name):
    for tag, dt in DTYPES.items():
        x = torch.from_numpy(g["pose"]).to(dt).requires_grad_(True)
        y = cases(dt)[name](x)
        y.sum().backward()
        for what, got, key in (("value", y.detach().numpy(), f"{name}_{tag}"), ("gradient", x.grad.numpy(), f"{name}_grad_{tag}")):
            assert got.shape == g[key].shape and got.dtype == g[key].dtype
            ref64 = g[key.replace("_f32", "_f64")]
            bound = 1e-12 if tag == "f64" else 8 * rel(g[key], ref64)
            err = rel(got, ref64)
            print(f"{name} {what} {tag}: E {err:.3e}  bound {bound:.3e}")
            assert err <= bound
    assert tuple(g["gmm_f32"].shape) == (5,) and tuple(g["angle_f32"].shape) == (5, 4) and g["l2_f32"].shape == ()


def test_the_mixture_prior_picks_different_components(g):
    gmm = P.MaxMixturePrior.from_arrays(*PR.priors_mixture(), dtype=torch.float64)
    means = gmm.means
    d = means[:, None] - means[None]
    quad = 0.5 * (torch.einsum("mij,bmj->bmi", gmm.precisions, d) * d).sum(-1) - torch.log(gmm.nll_weights)
    assert len(set(quad.argmin(1).tolist())) >= 3                               # (the min is live: near mean m, component m wins)
    assert torch.allclose(gmm(means), quad.min(1).values) and tuple(gmm.get_mean().shape) == (1, 69)


def test_create_prior():
    assert isinstance(P.create_prior("angle"), P.SMPLifyAnglePrior) and isinstance(P.create_prior("l2"), P.L2Prior)
    assert P.create_prior("none")(1, 2) == 0.0 and P.create_prior(None)() == 0.0
    with pytest.raises(ValueError, match="not implemented"):
        P.create_prior("vposer")
    with pytest.raises(NotImplementedError, match="merged"):
        P.MaxMixturePrior(use_merged=False, _arrays=PR.priors_mixture())


def test_files(tmp_path):
    means, covars, weights = PR.priors_mixture()
    x = torch.from_numpy(PR.priors_poses()[0][:, 3:]).float()
    want = P.MaxMixturePrior.from_arrays(means, covars, weights)(x)
    np.savez(tmp_path / "mix.npz", means=means, covars=covars, weights=weights)
    with open(tmp_path / "gmm_06.pkl", "wb") as f:
        pickle.dump({"means": means, "covars": covars, "weights": weights}, f)
    assert torch.equal(P.MaxMixturePrior.from_file(tmp_path / "mix.npz")(x), want)
    assert torch.equal(P.MaxMixturePrior.from_file(str(tmp_path / "gmm_06.pkl"))(x), want)
    assert torch.equal(P.create_prior("gmm", prior_folder=str(tmp_path), num_gaussians=6)(x, None), want)
    missing = os.path.join(str(tmp_path), "nowhere", "gmm_08.pkl")
    with pytest.raises(FileNotFoundError) as e:
        P.create_prior("gmm", prior_folder=os.path.dirname(missing), num_gaussians=8)
    assert missing in str(e.value)
    with pytest.raises(FileNotFoundError, match="absent.npz"):
        P.MaxMixturePrior.from_file(tmp_path / "absent.npz")
    with open(tmp_path / "other.pkl", "wb") as f:
        pickle.dump([1, 2], f)
    with pytest.raises(ValueError, match="means, covars and weights"):
        P.MaxMixturePrior.from_file(tmp_path / "other.pkl")
