"""sha256 of every output array of a fixed, seeded table of calls into the Python front end: the eight pipelines, the trainer and
the nets alone.

    python tools/pipeline_digest.py > digest.txt          (--calls: a line per call, to find where two outputs part;
                                                            --list: build every row on the CPU and print its tag, call nothing)

The table reaches the decisions smpl_nerf_amd/pipelines.py, nets.py and trainer.py take in front of the C ABI: single call or launch
by launch, which weight stream, which precision code, which rows a net reads, in which order the sigma noise is drawn.  It uses
only names that mean the same at every commit since the composed inference stream - the constructors, pipe(data), render_rays,
_forward_calls, set_precision, DataParallelTrainer.step, the nets' forward / forward_fused / forward_rays - so the same file runs in
a checkout of another commit: two commits compute the same bits iff their outputs are the same text.  Every call is made twice, each
time on a fresh deep copy of a template that is never called itself, and an array whose two digests differ is marked UNSTABLE.
One line per group of calls (the inference calls of one pipeline, form, mode and precision; every other call alone): the sha256
over the calls' lines, each of which is the call's tag and name=digest of every array; --calls prints those lines themselves.
Shapes are small (6 rays, 8 coarse + 6 fine samples, width 256, depth 8 unless a row says otherwise): none of those decisions
depends on the batch size, save the block-wise backward that activation_budget_bytes = 1 forces.
"""
import copy
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from smpl_nerf_amd import synthetic as syn  # noqa: E402
from smpl_nerf_amd.nets import AppendVerticesNet, RenderRayNet, WarpFieldNet  # noqa: E402
from smpl_nerf_amd.ops import PositionalEncoder  # noqa: E402
from smpl_nerf_amd import pipelines as P  # noqa: E402
from smpl_nerf_amd.synthetic_smpl import IndexPoseEstimator, LinearBodyModel  # noqa: E402
from smpl_nerf_amd.trainer import DataParallelTrainer  # noqa: E402

LIST = "--list" in sys.argv
DEV = torch.device("cpu" if LIST else "cuda:0")
B, NC, NF = 6, 8, 6
PRECISIONS = ("fp32", "bf16x6", "bf16x3", "f16x3")
HEX = 24      # hex digits of an array's sha256 in a call's line
# (white_background, sigma_noise_std, strict_cumsum): each switch alone, then all together
SWITCHES = ((0, 0.0, 0), (1, 0.0, 0), (0, 1.0, 0), (0, 0.0, 1), (1, 1.0, 1))
ENC = (PositionalEncoder(10, 0), PositionalEncoder(4, 0))
POSE_ENC = PositionalEncoder(10, 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def net_params(seed, **kw):
    """Seeded parameters with heads scaled, and a density bias, so that densities and colours are not trivial
    (synthetic.make_render_ray_net_params; the bias as in synthetic.make_append_vertices_params)."""
    p = syn.make_render_ray_net_params(seed, sigma_scale=30.0, rgb_scale=10.0, **kw)
    p["sigma_out_layer.bias"] = p["sigma_out_layer.bias"] + np.float32(2.0)
    return {k: torch.from_numpy(v) for k, v in p.items()}


def render_net(seed, add_dim=0, width=256, n_layers=8):
    m = RenderRayNet(n_layers, width, 60, 24, add_dim, skips=[4])
    m.load_state_dict(net_params(seed, n_layers=n_layers, width=width, additional_input_dim=add_dim))
    return m.to(DEV)


def warp_net(seed, positions_dim=60, pose_dim=40, width=256):
    m = WarpFieldNet(8, width, positions_dim, pose_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in
                       syn.make_warp_field_params(seed, positions_dim=positions_dim, pose_dim=pose_dim, width=width, out_scale=0.3).items()})
    return m.to(DEV)


def vertices_net(seed):
    m = AppendVerticesNet(8, 256, 60, 24, 6890, additional_input_layers=1, skips=[4])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_append_vertices_params(seed).items()})
    return m.to(DEV)


def rays():
    """[ray_samples [B,NC,3], origins, directions, z_vals, rgb_truth] of B rays of a 4 x 4 frame."""
    pick = np.array([0, 3, 5, 6, 9, 12])
    return [a[pick] for a in syn.frame_batch(4, 4, phi=5.0, theta=15.0, n_coarse=NC, seed=7)]


def poses():
    return syn.human_poses()[np.arange(B) % 10].astype(np.float32)


def estimator_and_body():
    est = IndexPoseEstimator(torch.from_numpy(syn.human_poses((41, 38), 0, 60, 60)), torch.zeros(1, 10)).to(DEV)
    return est, LinearBodyModel(seed=3).to(DEV)


def batch(kind):
    r = rays()
    rng = np.random.default_rng(21)
    if kind == "pose":
        fifth = [poses()]
    elif kind == "images":
        fifth = [(np.arange(B) * 7 % 60).astype(np.int64)]
    elif kind == "warp":
        fifth = [rng.normal(0, 0.05, (B, NC, 3)).astype(np.float32)]
    elif kind == "single":      # [ray_sample [B,3], origins, directions, goal_pose, warp [B,3], rgb_truth]
        return [T(a) for a in (r[0][:, 3], r[1], r[2], poses(), rng.normal(0, 0.05, (B, 3)).astype(np.float32), r[4])]
    else:
        fifth = []
    return [T(a) for a in r[:4] + fifth + r[4:]]


def args(**kw):
    return P.PipelineArgs(number_fine_samples=NF, **kw)


# name -> (batch kind, has a fine pass, build(args) -> (pipeline, the models a trainer optimises))
def _nerf(a):
    n = [render_net(101), render_net(102)]
    return P.NerfPipeline(n[0], n[1], a, *ENC), n


def _smpl(a):
    n = [render_net(101), render_net(102)]
    w = warp_net(103) if a.human_pose_encoding else warp_net(103, 3, 2)
    return P.SmplNerfPipeline(n[0], n[1], w, a, *ENC, POSE_ENC), n + [w]


def _append_smpl_params(a):
    a.human_pose_encoding = 0
    n = [render_net(301, 69), render_net(303, 69)]
    return P.AppendSmplParamsPipeline(n[0], n[1], a, *ENC, POSE_ENC), n


def _append_to_nerf(a):      # the two joints, encoded: 2 * 20 additional inputs
    n = [render_net(311, 40), render_net(313, 40)]
    return P.AppendToNerfPipeline(n[0], n[1], a, *ENC, POSE_ENC), n


def _append_vertices(a):
    n = [vertices_net(201), vertices_net(202)]
    return P.AppendVerticesPipeline(n[0], n[1], *estimator_and_body(), a, *ENC), n


def _dynamic(a):
    a.warp_radius, a.warp_temperature = 0.5, 10.0
    n = render_net(101)
    return P.DynamicPipeline(n, n, *estimator_and_body(), a, *ENC), [n]


def _vertex_sphere(a):
    n = render_net(101)
    return P.VertexSpherePipeline(n, n, a, *ENC), [n]


def _single_sample(a):
    n = render_net(101)
    return P.SingleSamplePipeline(n, a, *ENC), [n]


PIPELINES = {
    "NerfPipeline": ("plain", True, _nerf),
    "SmplNerfPipeline": ("pose", True, _smpl),
    "AppendSmplParamsPipeline": ("pose", True, _append_smpl_params),
    "AppendToNerfPipeline": ("pose", True, _append_to_nerf),
    "AppendVerticesPipeline": ("images", True, _append_vertices),
    "DynamicPipeline": ("images", False, _dynamic),
    "VertexSpherePipeline": ("warp", False, _vertex_sphere),
    "SingleSamplePipeline": ("single", False, _single_sample),
}
TRAINED = ("NerfPipeline", "SmplNerfPipeline", "AppendSmplParamsPipeline", "AppendToNerfPipeline", "AppendVerticesPipeline")


def digest(t):
    if t is None:
        return "none"
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:HEX] + ("" if bool((t != 0).any()) else "(all-zero)")


class Out:
    def __init__(self):
        self.lines, self.groups = [], {}

    def run(self, tag, call, group=None):
        """call() -> {name: tensor}, made twice; a call that raises is a row of its own (the error's type and text)."""
        self.groups.setdefault(group or tag, []).append(len(self.lines))
        if LIST:
            self.lines.append(tag)
            return
        both = []
        for _ in range(2):
            try:
                res = call()
                torch.cuda.synchronize()
                both.append({k: digest(v) for k, v in res.items()})
            except (RuntimeError, NotImplementedError) as e:
                if "HIP" in str(e) or "hip" in str(e) or "illegal" in str(e):      # a device fault: nothing more runs on it
                    raise
                both.append({"raised": hashlib.sha256(f"{type(e).__name__}: {e}".encode()).hexdigest()[:HEX]})
        a, b = both
        self.lines.append(tag + ": " + " ".join(f"{name}={a[name]}{'' if a[name] == b.get(name) else '(UNSTABLE)'}" for name in a))

    def text(self):
        if LIST or "--calls" in sys.argv:
            return "\n".join(self.lines)
        rows = []
        for group, idx in self.groups.items():
            mine = [self.lines[i] for i in idx]
            marks = [f"{what} in: {'; '.join(ln.split(': ')[0] for ln in mine if what in ln)}" for what in ("UNSTABLE", "all-zero")
                     if any(what in ln for ln in mine)]
            rows.append(f"{group}: {len(mine)} calls, {sum(ln.count('=') for ln in mine)} arrays, sha256 "
                        f"{hashlib.sha256(chr(10).join(mine).encode()).hexdigest()}{''.join('  ' + m for m in marks)}")
        return "\n".join(rows)


def named(out, prefix="out"):
    return {f"{prefix}{i}": t for i, t in enumerate(out)}


def set_mode(models, mode):
    for m in models:
        m.train() if mode == "train" else m.eval()


def fresh(template):
    """A deep copy of (pipeline, models, batch): nets with empty stream caches and a new weights epoch."""
    return copy.deepcopy(template)


def inference_rows(out, name):
    kind, has_fine, build = PIPELINES[name]
    data = batch(kind)
    fines = (1, 0) if has_fine else (0,)
    pose_modes = ((1, None), (0, 0)) if name == "SmplNerfPipeline" else ((1, None),)
    for hpe, only_fine in pose_modes:
        for run_fine, (wb, std, strict) in itertools.product(fines, SWITCHES):
            if only_fine is not None and run_fine != only_fine:
                continue
            a = args(run_fine=run_fine, white_background=wb, sigma_noise_std=std, strict_cumsum=strict, human_pose_encoding=hpe)
            pipe, models = build(a)
            for mode, precision in itertools.product(("eval", "train"), PRECISIONS):
                set_mode(models, mode)
                pipe.set_precision(precision)
                for form in ("pipe", "_forward_calls"):
                    def call(form=form):
                        p, d = fresh((pipe, data))
                        with torch.no_grad():
                            torch.manual_seed(1234)      # just before the call: holds the order of the noise draws
                            return named(p(d) if form == "pipe" else p._forward_calls(d))
                    out.run(f"{name} {form} {mode} {precision} fine {run_fine} wb {wb} noise {std} strict {strict} hpe {hpe}", call,
                            group=f"{name} {form} {mode} {precision}")


def loss_of(o, truth):
    return torch.nn.functional.mse_loss(o[0], truth) + torch.nn.functional.mse_loss(o[1], truth)


def autograd_rows(out, name):
    kind, has_fine, build = PIPELINES[name]
    data = batch(kind)
    posed = kind == "pose"
    cases = [("", False, None)] + ([(" goal_pose.requires_grad", True, None)] if posed else []) + [(" activation_budget_bytes 1", False, 1)]
    for precision, (label, pose_grad, budget) in itertools.product(("fp32", "bf16x6"), cases):
        pipe, models = build(args(run_fine=1 if has_fine else 0, sigma_noise_std=1.0))
        set_mode(models, "train")
        pipe.set_precision(precision)
        if budget is not None:
            for m in models:
                m.activation_budget_bytes = budget

        def call(pose_grad=pose_grad):
            p, d = fresh((pipe, data))
            if pose_grad:
                d[4].requires_grad_()
            torch.manual_seed(1234)
            o = p(d)
            loss_of(o, d[-1]).backward()
            res = named(o)
            res["loss"] = loss_of(o, d[-1])
            res.update({f"grad {k}": v.grad for k, v in p.named_parameters()})
            if pose_grad:
                res["grad goal_pose"] = d[4].grad
            return res
        out.run(f"{name} autograd {precision}{label}", call)


def trainer_rows(out, name):
    kind, _, build = PIPELINES[name]
    data = batch(kind)
    for one_call, precision, run_fine in itertools.product((None, False), ("fp32", "bf16x6"), (1, 0)):
        pipe, models = build(args(run_fine=run_fine, sigma_noise_std=1.0))
        set_mode(models, "train")
        pipe.set_precision(precision)

        def call(one_call=one_call):
            p, ms, d = fresh((pipe, models, data))
            tr = DataParallelTrainer(p, ms, lr=1e-3, one_call=one_call)
            torch.manual_seed(1234)
            res = {}
            for k in range(3):
                res[f"loss {k}"] = tr.step(d).detach().clone()
                res[f"params {k}"] = torch.cat([q.detach().reshape(-1) for q in tr.params]).clone()
            set_mode(ms, "eval")
            with torch.no_grad():      # the streams must be current after the last step
                res.update(named(p(d), "render"))
            tr.close()
            return res
        out.run(f"{name} trainer one_call {one_call} {precision} fine {run_fine}", call)


def net_rows(out):
    rng = np.random.default_rng(31)
    rows = T(rng.uniform(-1, 1, (70, 84)).astype(np.float32))
    wrows = T(rng.uniform(-1, 1, (70, 100)).astype(np.float32))
    x, d = T(rng.uniform(-2, 2, (B * NC, 3)).astype(np.float32)), T(rng.normal(size=(B, 3)).astype(np.float32))
    for mode, grad in itertools.product(("eval", "train"), (False, True)):
        for label, net, inp in (("RenderRayNet.forward", render_net(101), rows), ("WarpFieldNet.forward", warp_net(103), wrows)):
            set_mode([net], mode)

            def call(net=net, inp=inp):
                m, r = fresh((net, inp))
                if not grad:
                    with torch.no_grad():
                        return {"out": m(r)}
                r.requires_grad_()
                o = m(r)
                o.square().sum().backward()
                res = {"out": o, "grad rows": r.grad}
                res.update({f"grad {k}": v.grad for k, v in m.named_parameters()})
                return res
            out.run(f"{label} encoded rows {mode} grad {grad}", call)
    vn, vrows = vertices_net(201), T(rng.uniform(-1, 1, (B, 60)).astype(np.float32))
    narrow, layered = render_net(401, width=128), render_net(402, width=32, n_layers=17)
    narrow.precision = "bf16x6"      # (other widths than 256 run fp32)
    for mode in ("eval", "train"):
        for label, net, fn in (("AppendVerticesNet.forward_rays", vn, lambda m: m.forward_rays(vrows, d, NC, B * NC)),
                               ("RenderRayNet.forward_fused width 128 bf16x6", narrow, lambda m: m.forward_fused(x, d, NC, *ENC)),
                               ("RenderRayNet.forward_fused 17 layers width 32", layered, lambda m: m.forward_fused(x, d, NC, *ENC))):
            for precision in (PRECISIONS if net is vn else (None,)):
                set_mode([net], mode)
                if precision:
                    net.precision = precision

                def call(net=net, fn=fn):
                    with torch.no_grad():
                        return {"raw": fn(fresh(net))}
                out.run(f"{label} {mode} {precision or ''}", call)
    # a render, an in-place edit of p.data with mark_weights_changed(), another render
    for name in ("NerfPipeline", "SmplNerfPipeline", "AppendVerticesPipeline"):
        kind, _, build = PIPELINES[name]
        pipe, models = build(args())
        set_mode(models, "eval")
        data = batch(kind)

        def call():
            p, ms, dd = fresh((pipe, models, data))
            with torch.no_grad():
                res = named(p(dd), "before")
                for m in ms:
                    for q in m.parameters():
                        q.data.mul_(1.01)
                    m.mark_weights_changed()
                res.update(named(p(dd), "after"))
            return res
        out.run(f"{name} render, p.data edit + mark_weights_changed, render", call)


def main():
    out = Out()
    for name in PIPELINES:
        print(f"# {name}", file=sys.stderr, flush=True)
        inference_rows(out, name)
        autograd_rows(out, name)
    for name in TRAINED:
        trainer_rows(out, name)
    net_rows(out)
    print(out.text())
    print(f"# {len(out.lines)} calls, {sum(ln.count('=') for ln in out.lines)} arrays, {sum(ln.count('UNSTABLE') for ln in out.lines)} unstable",
          file=sys.stderr)


if __name__ == "__main__":
    main()
