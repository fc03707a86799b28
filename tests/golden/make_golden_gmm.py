#!/usr/bin/env python3
"""Golden vectors for the canonical-density loss (utils.GaussianMixture, utils.py:72-111; SmplNerfSolver.smpl_nerf_loss with
use_gmm_loss = 1, solver/smpl_nerf_solver.py:35-43) from the reference itself.
    python tests/golden/make_golden_gmm.py    # writes g18_gmm_loss.npz
(a) operator cases op/B_S_V_std/...: the reference's GaussianMixture.pdf and the autograd gradient of mse_loss(pdf, d) with respect
    to the samples, on the seeded inputs of tests/gmm_ref.py (op_inputs; V <= 1000: the reference builds [B, S, V, 3]), with the
    object's factor and var.
(b) the pipeline case: the g6 / g11 batch and nets (make_golden_smpl_grad.py, white_background = 0) through the reference's
    SmplNerfPipeline and its solver's loss with gmm_std = 0.07 - the three loss values, the mixture term, pdf [64, 192], the gradient
    digests of the three nets and the warp net's full gradients.  The 1000 means are a seeded subset of the warped fine samples of a
    first pass plus noise (gmm_ref.g18_means) and are stored, so that the term is live."""
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import gmm_ref as GR
import make_golden as MG
import make_golden_grad as GG

t = MG.t


def main():
    U, RenderRayNet, _, SmplNerfPipeline, WarpFieldNet = MG._import_reference()
    torch.set_grad_enabled(True)
    cpu = torch.device("cpu")
    g = {"config": np.array(json.dumps(GR.G18))}

    # ---- (a) the operator ----------------------------------------------------------------------------------------
    for std in GR.STDS:
        for B, S, V in GR.G18_OP_SHAPES:
            samples, means, d = GR.op_inputs(B, S, V, std, GR.G18["op_seed"])
            mix = U.GaussianMixture(means, std, cpu)
            x = t(samples).requires_grad_(True)
            pdf = mix.pdf(x)
            torch.nn.functional.mse_loss(pdf, t(d)).backward()
            key = f"op/{B}_{S}_{V}_{std}"
            g[key + "/pdf"], g[key + "/d_samples"] = pdf.detach().numpy(), x.grad.numpy()
            g[key + "/factor_var"] = np.array([mix.factor, mix.var], np.float64)
            print(key, "max pdf", float(pdf.max()), "max |d_samples|", float(x.grad.abs().max()))

    # ---- (b) the pipeline ----------------------------------------------------------------------------------------
    try:
        from solver.smpl_nerf_solver import SmplNerfSolver
        loss_of = SmplNerfSolver.smpl_nerf_loss
        print("loss: the reference's SmplNerfSolver.smpl_nerf_loss")
    except Exception as e:          # the solver module does not import under the stubs: its three lines composed here
        print("solver module not importable (%s): U.GaussianMixture composed with torch.nn.MSELoss" % e)

        def loss_of(self, rgb, rgb_fine, rgb_truth, warp, densities, ray_samples):
            lc, lf = self.loss_func(rgb, rgb_truth), self.loss_func(rgb_fine, rgb_truth)
            return lc + lf + self.loss_func(self.canonical_mixture.pdf(ray_samples), densities), lc, lf
    batch_np, pc, pf, pw = GR.g18_batch()
    batch = [t(a) for a in batch_np]
    pe, de, he = U.PositionalEncoder(10, 0), U.PositionalEncoder(4, 0), U.PositionalEncoder(10, 0)
    args = MG.Args(white_background=0, use_gmm_loss=1, restrict_gmm_loss=0, gmm_std=GR.G18["gmm_std"])

    def nets():
        return (MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), pc), MG.load_params(RenderRayNet(8, 256, 60, 24, skips=[4]), pf),
                MG.load_params(WarpFieldNet(8, 256, 60, 40), pw))

    with torch.no_grad():
        mc, mf, mw = nets()
        first = SmplNerfPipeline(mc, mf, mw, args, pe, de, he)(batch)
    means = GR.g18_means(first[4].numpy())
    g["means"] = means
    mc, mf, mw = nets()
    out = SmplNerfPipeline(mc, mf, mw, args, pe, de, he)(batch)
    me = SimpleNamespace(loss_func=torch.nn.MSELoss(), args=args, canonical_mixture=U.GaussianMixture(means, args.gmm_std, cpu))
    loss, loss_coarse, loss_fine = loss_of(me, out[0], out[1], batch[-1], out[2], out[5], out[4])
    loss.backward()
    pdf = me.canonical_mixture.pdf(out[4]).detach()
    term = torch.nn.functional.mse_loss(pdf, out[5].detach())
    g["loss"] = np.array([loss.item(), loss_coarse.item(), loss_fine.item()])
    g["term"] = np.array([term.item()])
    g["pdf"] = pdf.numpy()
    g["factor_var"] = np.array([me.canonical_mixture.factor, me.canonical_mixture.var], np.float64)
    for name, m in (("coarse", mc), ("fine", mf), ("warp", mw)):
        for k, v in GG.param_digest((f"{name}.{k}", p.grad) for k, p in m.named_parameters()).items():
            g[f"grad/{k}"] = v
        if name == "warp":
            for k, p in m.named_parameters():
                g[f"warpfull/{k}"] = p.grad.numpy()
    # the term must matter, or a silently missing term would pass the pipeline test
    g11 = np.load(os.path.join(HERE, "g11_smpl_grads.npz"))
    norm = np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in mw.parameters()))
    norm11 = np.sqrt(sum(float((g11[k].astype(np.float64) ** 2).sum()) for k in g11.files if k.startswith("warpfull_wb0/")))
    print(f"loss {loss.item():.8f} = {loss_coarse.item():.8f} + {loss_fine.item():.8f} + {term.item():.8f}; max pdf {float(pdf.max()):.4f}, "
          f"max density {float(out[5].max()):.4f}; warp-net gradient norm {norm:.6e} (g11: {norm11:.6e})")
    assert abs(loss.item() - (loss_coarse.item() + loss_fine.item() + term.item())) <= 1e-6 * loss.item()
    assert term.item() >= 0.1 * loss.item(), "the mixture term is not a tenth of the loss"
    assert abs(norm - norm11) >= 0.1 * norm11, "the warp net's gradient hardly differs from g11's"
    MG.save("g18_gmm_loss.npz", **g)


if __name__ == "__main__":
    main()
