"""Torch (CPU) restatement of the reference's GaussianMixture.pdf (utils.py:72-111) and of SmplNerfSolver's three-term loss
(solver/smpl_nerf_solver.py:35-43), used ONLY by tests.

    pdf(x) = factor / V sum_v exp(-|x - mu_v|^2 / (2 std^2))        factor = 1 / sqrt((2 pi)^3 std^6)

mixture_pdf() is the reference's own operations in its order, in the dtype of its inputs and differentiable by autograd - but in
chunks of samples, so that the [.., V, 3] tensor of the reference only ever exists for a few rows.  In float64 it is the truth the GPU
tests measure against, in fp32 what fp32 arithmetic can be asked for; tests/test_gmm_host.py pins the fp32 form to what the
reference itself computed (tests/golden/g18_gmm_loss.npz).  Also here: the seeded inputs of that fixture (it stores outputs, and of
the inputs only the means of its pipeline case, which the generator derives from a first pass of the reference) and the error
measure of the tests.
"""
import numpy as np
import torch

F32 = np.float32
STDS = (0.07, 0.01)                                # the parser's gmm_std (config_parser.py) and a narrow one
SHAPES = [(1, 1, 1), (2, 7, 63), (3, 64, 65), (2, 65, 1000), (1, 100, 6890), (5, 64, 257)]
G18_OP_SHAPES = [s for s in SHAPES if s[2] <= 1000]      # what the reference can afford: it builds [B, S, V, 3]
G18 = dict(op_seed=18, net_seeds=(101, 103), frame=dict(h=128, w=128, phi=5.0, theta=15.0, seed=9), means_seed=181, V=1000,
           means_noise=0.05, gmm_std=0.07)


def factor_var(std, dim=3):
    """utils.py:84-86, the same Python expressions."""
    var = std ** 2
    cov_det = var ** dim
    return 1 / np.sqrt(((2 * np.pi) ** dim * cov_det)), var


def mixture_pdf(samples, means, std, rows=None):
    """utils.py:102-111 on samples [..., 3], means [V, 3] -> [...]; `rows` samples at a time (default: about 2^21 pairs)."""
    factor, var = factor_var(std, means.shape[-1])
    x = samples.reshape(-1, samples.shape[-1])
    rows = rows or max(1, (1 << 21) // means.shape[0])
    out = []
    for i in range(0, x.shape[0], rows):
        diff = x[i:i + rows, None, :] - means[None, :, :]
        probs = factor * torch.exp(-0.5 * torch.sum(diff ** 2, dim=-1) / var)
        out.append(torch.sum(probs, dim=-1) / probs.shape[-1])
    return torch.cat(out).reshape(samples.shape[:-1])


def relative_error(y, y64):
    """E(y) = max|y - y64| / max|y64| (0 when both are all zero)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    err = np.abs(y - y64).max() if y64.size else 0.0
    return 0.0 if err == 0.0 else err / np.abs(y64).max()


# ------------------------------------------------------------------------------------------------ inputs
def op_inputs(B, S, V, std, seed, plant="both", spread=0.3):
    """means ~ N(0, spread) [V, 3]; samples [B, S, 3]: every other one near a mean (mean + N(0, std)), the others uniform in the
    means' box; the target d [B, S] of mse_loss(pdf, d); fp32 numpy.  Planted: the FIRST sample lies exactly on a mean, the LAST one
    50 units away from everything, where the density underflows (`plant`: "both", or "mean" / "far" alone - a one-sample case runs
    once with each)."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0, spread, (V, 3)).astype(F32)
    samples = rng.uniform(-2 * spread, 2 * spread, (B, S, 3))
    near = means[rng.integers(0, V, (B, S))] + rng.normal(0, std, (B, S, 3))
    mask = (np.arange(S)[None, :] + np.arange(B)[:, None]) % 2 == 0
    samples[mask] = near[mask]
    samples = samples.astype(F32).reshape(-1, 3)
    if plant in ("both", "far"):
        samples[-1] = means[V // 2] + np.array([50.0, 0.0, 0.0], F32)
    if plant in ("both", "mean"):
        samples[0] = means[V // 2]
    d = (rng.uniform(0, 1, (B, S)) * 0.05 * factor_var(std)[0]).astype(F32)
    return samples.reshape(B, S, 3), means, d


def restated(samples, means, d, std, dtype):
    """pdf and d mse_loss(pdf, d) / d samples of the restatement on the CPU in `dtype`: dict of numpy arrays."""
    x = torch.from_numpy(samples).to(dtype).requires_grad_(True)
    pdf = mixture_pdf(x, torch.from_numpy(means).to(dtype), std)
    torch.nn.functional.mse_loss(pdf, torch.from_numpy(d).to(dtype)).backward()
    return {"pdf": pdf.detach().numpy(), "d_samples": x.grad.numpy()}


def g18_batch():
    """The g6 / g11 batch (64 rays, 64 + 128 samples) and the three nets' parameters of tests/golden/make_golden_smpl_grad.py:
    (batch as fp32 numpy arrays [ray_samples, ray_translation, ray_direction, z_vals, goal_pose, rgb_truth], coarse, fine, warp)."""
    import os
    from smpl_nerf_amd import synthetic as syn
    g6 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g6_smpl_nerf_pipeline.npz"))
    data = syn.frame_batch(**G18["frame"])
    sub = g6["sub"]
    batch = [a[sub] for a in data[:4]] + [g6["goal_pose"], data[4][sub]]
    pc, pf = syn.make_scene_nets(G18["net_seeds"][0])
    return batch, pc, pf, syn.make_warp_field_params(G18["net_seeds"][1], out_scale=0.3)


def g18_means(warped_fine):
    """The 1000 means of the pipeline case: a seeded subset of the warped fine samples of a first pass [64, 192, 3] plus N(0, 0.05)
    noise (the generator stores the result, since the first pass is the reference's)."""
    rng = np.random.default_rng(G18["means_seed"])
    pts = np.asarray(warped_fine, np.float64).reshape(-1, 3)
    pick = rng.choice(pts.shape[0], G18["V"], replace=False)
    return (pts[pick] + rng.normal(0, G18["means_noise"], (G18["V"], 3))).astype(F32)
