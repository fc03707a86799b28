"""NerfPipeline drop-in (models/nerf_pipeline.py:8-67).

Same constructor, same `forward(data)` contract - `data` is the list
[ray_samples[B,Nc,3], ray_translation[B,3], ray_direction[B,3], z_vals[B,Nc], rgb_truth[B,3]] a Solver
hands over (solver/nerf_solver.py:77-81) and the result is the 4-tuple
(rgb, rgb_fine, ray_samples_fine, densities) - but the whole march is five HIP launches:

    fused encode+MLP (coarse)  ->  composite  ->  inverse-CDF sampler+merge+points
                               ->  fused encode+MLP (fine)  ->  composite

No [B*N, 84] encoded input, no [B*N, 256] activation and no [B, 128, 63] gather operand is ever
materialised in HBM.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
from torch import nn

from . import _lib
from . import ops
from ._lib import check, current_stream, ptr


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NULL = _NullCtx()


def _on_device(dev):
    """torch.cuda.device(dev), or nothing when `dev` is already current (the usual case; the context manager costs ~10 us per call,
    a fifth of the host time of a small render)."""
    return _NULL if torch.cuda.current_device() == (dev.index or 0) else torch.cuda.device(dev)


def _render_outputs(B, N, n_sample_tensors, dev):
    """rgb [B,3], rgb_fine [B,3], n_sample_tensors x [B,N,3], densities [B,N] as views of ONE allocation (16-byte aligned each)."""
    sizes = [B * 3, B * 3] + [B * N * 3] * n_sample_tensors + [B * N]
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (n + 3) & ~3
    buf = torch.empty(off, device=dev, dtype=torch.float32)
    shapes = [(B, 3), (B, 3)] + [(B, N, 3)] * n_sample_tensors + [(B, N)]
    return [buf[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]


class PipelineArgs:
    """The fields of the reference's argparse namespace (config_parser.py) that the pipelines read.  Any object with these
    attributes works as `args` (the reference's own namespace included).

    The defaults here are the deterministic, runnable settings - NOT the reference's parser defaults in two fields:
    sigma_noise_std is 0 (config_parser.py:87 has 1: Gaussian noise on sigma, drawn even in eval mode, quirk Q3) and
    human_pose_encoding is 1 (config_parser.py:72 has 0, with which the reference's own smpl_nerf fine branch crashes,
    quirk Q5).  PipelineArgs.reference_defaults() returns the parser's values.

    strict_cumsum (not a reference field): 1 = the hierarchical sampler takes its normalising sums in the order
    of torch's CPU kernel, like the reference's CPU path, so that the sample indices equal the reference's bit for bit from
    the same weights (ops.reference_normalising_sum: on the device where ops.device_reference_sum_ok(), with the single-call
    render and the one-call training step; a host round trip per call elsewhere)."""

    def __init__(self, **kw):
        self.sigma_noise_std = 0.0
        self.white_background = 0
        self.run_fine = 1
        self.number_fine_samples = 128
        self.human_pose_encoding = 1
        self.strict_cumsum = 0
        self.warp_radius = 0.01          # config_parser.py:47-49: DynamicPipeline's attention radius and temperature
        self.warp_temperature = 10000
        self.vertex_sphere_radius = 0.01          # config_parser.py:35-45: the vertex_sphere model (vertex_sphere.VertexSphereRays)
        self.warp_by_vertex_mean = 0
        self.coarse_samples_from_prior = 0
        self.coarse_samples_from_intersect = 0
        self.std_dev_coarse_sample_prior = 0.03
        self.u = None  # optional explicit linspace(0, 1, number_fine_samples) buffer (ops.uniform_u)
        self.__dict__.update(kw)

    @classmethod
    def reference_defaults(cls, **kw):
        """config_parser.py:27,71,72,87,89."""
        d = dict(sigma_noise_std=1.0, white_background=0, run_fine=1, number_fine_samples=128, human_pose_encoding=0)
        d.update(kw)
        return cls(**d)


def joints_38_41(goal_pose):
    """The two joint angles the reference hard-codes (models/smpl_nerf_pipeline.py:28, append_to_nerf_pipeline.py:26)."""
    return torch.stack([goal_pose[:, 38], goal_pose[:, 41]], axis=-1)


class NerfPipeline(nn.Module):

    def __init__(self, model_coarse, model_fine, args, position_encoder, direction_encoder):
        super().__init__()
        self.device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")  # singe_sample_pipeline.py:11
        self.args = args
        self.model_coarse = model_coarse
        self.model_fine = model_fine
        self.position_encoder = position_encoder
        self.direction_encoder = direction_encoder

    def set_precision(self, precision: str):
        """Matrix-core arithmetic of every net of the pipeline: "fp32" (exact fp32 MFMA), "bf16x6" (split-bf16, fp32-class
        accuracy - the parity mode on the bf16 matrix cores) or "bf16x3" (split-bf16, ~2^-16 relative)."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        for m in self.modules():
            if hasattr(m, "precision") and m is not self:
                m.precision = precision
        return self

    def _noise(self, shape, device):
        # utils.py:171-173: drawn whenever sigma_noise_std > 0, also in eval mode (quirk Q3)
        std = getattr(self.args, "sigma_noise_std", 0.)
        return torch.normal(0, std, shape, device=device) if std > 0. else None

    def _net_desc(self, net):
        """The descriptor of the fused (encode + MLP) path of one of the pipeline's two nets - what its launches, its single-call
        entry and the one-call training step (trainer.py) all pass."""
        return net.desc_for_encoders(self.position_encoder, self.direction_encoder, False)

    # keep_fine = True (checkers only: tools/ab/fuzz_*.py): forward() leaves the merged depths and the hierarchical sample points
    # - which are not outputs of the reference's forward - in `last_fine`; off by default (a [B, N, 3] tensor pinned
    # between calls, 38 MB for a 128 x 128 frame)
    keep_fine = False
    last_fine = None
    _pose_in_batch = 0      # 1: data[4] is a goal pose, which the single-call entry reads through a raw fp32 device pointer

    def _single_call_ok(self, data) -> bool:
        """Inference (autograd off) goes through the single C-ABI call of render_rays() - what inference.py:251-252's
        `pipeline(data)` costs a host then is one call instead of five; same kernels, same results (tools/ab/fuzz_render.py holds
        them bit for bit).  The five-call form stays for autograd, for a _lib.profile() (which brackets every launch with an
        event pair: bench.py's roofline), for the checkers' keep_fine and for the strict sampler on hosts where it is a host
        round trip (ops.device_reference_sum_ok() false)."""
        if self._single_call is None or torch.is_grad_enabled() or _lib._PROFILE is not None or self.keep_fine:
            return False
        if getattr(self.args, "strict_cumsum", 0) and not ops.device_reference_sum_ok():
            return False
        nets = [self.model_coarse, self.model_fine] + ([self.model_warp_field] if hasattr(self, "model_warp_field") else [])
        if len({getattr(m, "precision", "fp32") for m in nets}) != 1 or any(getattr(m, "_layered", False) for m in nets):
            return False      # (nets above the fused kernels' widths run layer by layer: layered.py)
        return all(torch.is_tensor(t) and t.is_cuda and (t.dtype == torch.float32) for t in data[:4 + self._pose_in_batch])

    def forward(self, data):
        if self._single_call_ok(data):
            return self.render_rays(data)
        return self._forward_calls(data)

    def _march(self, data, stage, coarse_only=False):
        """The ray march every pipeline with a compositing runs, launch by launch (models/nerf_pipeline.py:29-67): coarse stage ->
        composite -> hierarchical samples on the un-warped ray -> fine stage -> composite.  What a pipeline adds is its stage:

            stage(samples, samples per ray, fine: bool) -> (raw [B * n, 4], per-sample directions or None, (warp, warped) or ())
            (warp and warped come back in the shape of the samples; a stage may leave them flat, [B * n, 3])

        The coarse compositing scales the distances by the stage's per-sample directions where it returns some and by the ray
        direction otherwise; the fine one always by the ray direction (models/smpl_nerf_pipeline.py:63 against :95-98).  A stage
        that warps returns (warp, warped), and the result carries them around the samples: (rgb, rgb_fine, warp, samples, warped,
        densities) instead of (rgb, rgb_fine, samples, densities).  The sigma noise of a compositing is drawn after its stage's
        launch.  coarse_only: no fine pass whatever args.run_fine says, and the coarse weights are not asked for."""
        ray_samples, ray_translation, ray_direction, z_vals = data[:4]
        args = self.args
        B, Nc = z_vals.shape
        wb = bool(args.white_background)
        dev = ray_samples.device

        def outputs(rgb_fine, samples, densities, extra):
            if not extra:
                return rgb, rgb_fine, samples, densities
            warp, warped = (t if t.shape == samples.shape else t.view(samples.shape) for t in extra)
            return rgb, rgb_fine, warp, samples, warped, densities

        raw, sdirs, extra = stage(ray_samples, Nc, False)
        rgb, weights, densities = ops.composite(raw.view(B, Nc, 4), z_vals, ray_direction if sdirs is None else sdirs.view(B, Nc, 3),
                                                wb, self._noise((B, Nc), dev), want_weights=not coarse_only)
        if coarse_only or not args.run_fine:
            return outputs(rgb, ray_samples, densities, extra)      # (the same tensor twice and the caller's own samples, quirk Q10)
        hs = ops.hierarchical_samples(ray_translation, ray_direction, z_vals, weights, args.number_fine_samples,
                                      strict=bool(getattr(args, "strict_cumsum", 0)))
        z_fine, ray_samples_fine = hs["z_fine"], hs["pts"]
        if self.keep_fine:
            self.last_fine = (z_fine, ray_samples_fine)
        N = z_fine.shape[1]
        raw_fine, _, extra = stage(ray_samples_fine, N, True)
        rgb_fine, _, densities_fine = ops.composite(raw_fine.view(B, N, 4), z_fine, ray_direction, wb, self._noise((B, N), dev),
                                                    want_weights=False)
        return outputs(rgb_fine, ray_samples_fine, densities_fine, extra)

    def _forward_calls(self, data):
        ray_direction = data[2]

        def stage(samples, n, fine):      # the net on the given samples (:29-41) / on the hierarchical ones (:49-60)
            net = self.model_fine if fine else self.model_coarse
            return net.forward_fused(samples, ray_direction, n, self.position_encoder, self.direction_encoder), None, ()

        return self._march(data, stage)      # :42-44, :47, :65-67

    def render_rays(self, data):
        """forward(data) for inference through the pipeline's single C-ABI call (include/smplnerf.h: _single_call): same outputs,
        one host call instead of five - the entry point a non-Python host binds.  No autograd.  A pipeline without such an entry,
        and nets above the fused kernels' widths (layered.py), run forward()'s launches under no_grad - the same kernels, the same
        results."""
        if self._single_call is None or any(getattr(m, "_layered", False) for m in self.children()):
            with torch.no_grad():
                return self._forward_calls(data)
        return self._single_call(data)

    def _render_setup(self, data, nets, workspace_entry, workspace_takes_descs=False, n_sample_tensors=1):
        """What the single-call entries share.  `nets`: the coarse and the fine net, then whatever else must run in their precision.
        Returns a record of the arguments in the entries' order - head (the two nets' descriptors and streams), mid (precision,
        samples, origins, directions, depths), tail (u, coarse and fine sigma noise, B, Nc, Nf, white_background, workspace), outs
        (_render_outputs) - with prec, the nets' precision code.  fp32 calls of nets in eval mode run on the composed inference
        streams (nets.RenderRayNet.packed_weights_infer): SNERF_FP32_INFER and those streams when every net has one, else the
        regular fp32 streams.  Both noise tensors are drawn here, coarse then fine, in front of the call."""
        ray_samples, ray_translation, ray_direction, z_vals = data[:4]
        args = self.args
        B, Nc = z_vals.shape
        Nf = int(args.number_fine_samples) if args.run_fine else 0
        N = Nc + Nf
        dev = ray_samples.device
        prec = _lib.precision_code(nets, "render_rays")
        descs = [self._net_desc(m) for m in nets[:2]]
        if prec:
            packed = [m.packed_weights_bf16(d, prec) for m, d in zip(nets, descs)]
        else:
            packed = [m.packed_weights_infer(d) for m, d in zip(nets, descs)]
            if any(p is None for p in packed):
                packed = [m.packed_weights(d) for m, d in zip(nets, descs)]
            else:
                prec = _lib.FP32_INFER
        lib = _lib.load()
        need = int(getattr(lib, workspace_entry)(*(descs if workspace_takes_descs else ()), B, Nc, Nf))
        if need < 0:
            check(need, workspace_entry)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        outs = _render_outputs(B, N, n_sample_tensors, dev)
        u = ops.uniform_u(Nf, dev) if Nf else None
        nc, nf = self._noise((B, Nc), dev), (self._noise((B, N), dev) if Nf else None)
        x, o, d, z = (t.contiguous() for t in (ray_samples, ray_translation, ray_direction, z_vals))
        # the precision argument: SNERF_REFERENCE_SUM ORed in when strict mode's sum runs on the device
        strict = _lib.REFERENCE_SUM if getattr(args, "strict_cumsum", 0) and ops.device_reference_sum_ok() else 0
        return SimpleNamespace(
            lib=lib, dev=dev, prec=prec, outs=outs, head=(descs[0], ptr(packed[0]), descs[1], ptr(packed[1])),
            mid=(prec | strict, ptr(x), ptr(o), ptr(d), ptr(z)),
            tail=(ptr(u), ptr(nc), ptr(nf), B, Nc, Nf, 1 if args.white_background else 0, ptr(ws)),
            keep=(packed, ws, u, nc, nf, x, o, d, z))      # (what only the pointers above refer to, alive until the call is enqueued)

    def _render_result(self, data, r):
        """The entry's outputs as forward() returns them; run_fine = 0: the coarse colour twice and the caller's own samples
        (models/nerf_pipeline.py:43-44, append_smpl_params_pipeline.py:56-57, quirk Q10)."""
        if self.args.run_fine:
            return tuple(r.outs)
        return r.outs[0], r.outs[0], data[0], r.outs[-1]

    def ray_maps(self, data, out):
        """The opacity, the expected depth and the expected point of every ray of `data` from out = forward(data):
        ops.RayMaps(acc [B], depth [B], point [B, 3]) - the acc_map and depth_map the reference's raw2outputs computes and drops
        (utils.py:184, :187), of the compositing whose colour is out[1].  Reads the `samples` and `densities` of the 4-tuple or of
        the 6-tuple (with a warp stage: the un-warped samples, on the ray) and the ray's origin and direction, data[1] and data[2].
        `depth` is the ray parameter t of o + t d: with the generated rays (raygen, d = a camera-space direction of z = -1) the
        z-depth ops.render_mesh returns as `t`; depth * |d| is the Euclidean distance single_sample.SingleSampleRays.depth holds.
        Differentiable in the densities: under autograd a loss on depth or acc trains the nets."""
        samples, densities = (out[2], out[3]) if len(out) == 4 else (out[3], out[5])
        return ops.ray_maps(densities, data[1], data[2], samples=samples)

    def _single_call(self, data):
        """snerf_render_rays_f32."""
        r = self._render_setup(data, (self.model_coarse, self.model_fine), "snerf_render_rays_workspace_bytes")
        with _on_device(r.dev), _lib.timed("render_rays"):
            check(r.lib.snerf_render_rays_f32(*r.head, *r.mid, *r.tail, *map(ptr, r.outs), current_stream()), "snerf_render_rays_f32")
        return self._render_result(data, r)


class SmplNerfPipeline(NerfPipeline):
    """models/smpl_nerf_pipeline.py:7-100 drop-in: NerfPipeline with a pose-conditioned warp of the samples.

    data = [ray_samples, ray_translation, ray_direction, z_vals, goal_pose[B,69], rgb_truth]; returns
    (rgb, rgb_fine, warp_fine, ray_samples_fine, warped_samples_fine, densities_fine) or, with
    run_fine = 0, (rgb, rgb, warp, ray_samples, warped_samples, densities).  Quirks kept: joints 38 and 41
    are hard-coded (:28); the coarse compositing scales distances by |x' - o| per sample (:63) while the
    fine one uses the ray direction (:95-98); hierarchical samples are drawn on the un-warped ray (:68).
    human_pose_encoding = 0 (the parser default, config_parser.py:72): the warp net reads [x | two joint angles] un-encoded
    (:40-45; WarpFieldNet(positions_dim=3, pose_dim=2), train.py:111-114) - the fused warp kernel with an identity-only
    position "encoder".  The fine branch always builds encoded rows (:71-77), so with run_fine = 1 that mode fails at
    the fine warp evaluation exactly like the reference (quirk Q5: a RuntimeError from the 5-column linear1)."""

    class _RawPositions:
        """PositionalEncoder(0, True): the identity columns only (warp-net input of human_pose_encoding = 0)."""
        number_frequencies, include_identity, output_dim = 0, True, 1

    _pose_in_batch = 1

    def __init__(self, model_coarse, model_fine, model_warp_field, args, position_encoder, direction_encoder,
                 human_pose_encoder):
        super().__init__(model_coarse, model_fine, args, position_encoder, direction_encoder)
        self.human_pose_encoder = human_pose_encoder
        self.model_warp_field = model_warp_field

    def _joint_pose(self, goal_pose):
        """(the two joint angles [B, 2], their encoding): :28, :30 - what the warp net reads per ray."""
        two = joints_38_41(goal_pose).contiguous()
        return two, self.human_pose_encoder.encode(two).contiguous()

    def _warp_desc(self):
        """The warp net's descriptor with the encoded pose (the single-call entry and the one-call training step)."""
        return self.model_warp_field.desc_for_encoder(self.position_encoder)

    def _single_call_ok(self, data) -> bool:
        # (the one-call entry covers the full coarse + fine march with the encoded pose)
        return bool(self.args.human_pose_encoding and self.args.run_fine) and super()._single_call_ok(data)

    def _forward_calls(self, data):
        ray_translation = data[1]
        two, pose_enc = self._joint_pose(data[4])

        def stage(samples, n, fine):
            # the coarse stage of human_pose_encoding = 0 reads the raw angles beside un-encoded positions (:40-45); every other
            # one the encoded pose (:37-39, :71-77)
            raw_pose = not fine and not self.args.human_pose_encoding
            warp, warped, sdirs = self.model_warp_field.forward_fused(
                samples, two if raw_pose else pose_enc, ray_translation, n, self._RawPositions if raw_pose else self.position_encoder)
            net = self.model_fine if fine else self.model_coarse
            return net.forward_fused(warped, sdirs, n, self.position_encoder, self.direction_encoder), sdirs, (warp, warped)

        return self._march(data, stage)      # :63-65, :68, :95-100

    def _single_call(self, data):
        """snerf_render_rays_smpl_f32.  The entry covers the full coarse + fine march with the encoded pose; run_fine = 0 and
        human_pose_encoding = 0 (three launches instead of eight) go through forward()'s launches under no_grad."""
        if not self.args.human_pose_encoding or not self.args.run_fine:
            with torch.no_grad():
                return self._forward_calls(data)
        mw = self.model_warp_field
        pose_enc = self._joint_pose(data[4])[1]
        r = self._render_setup(data, (self.model_coarse, self.model_fine, mw), "snerf_render_rays_smpl_workspace_bytes",
                               n_sample_tensors=3)
        wdesc = self._warp_desc()
        wpacked = mw._packed(wdesc) if r.prec in (0, _lib.FP32_INFER) else mw._packed_bf16(wdesc)
        with _on_device(r.dev), _lib.timed("render_rays_smpl"):
            check(r.lib.snerf_render_rays_smpl_f32(*r.head, wdesc, ptr(wpacked), *r.mid, ptr(pose_enc), *r.tail, *map(ptr, r.outs),
                                                   current_stream()), "snerf_render_rays_smpl_f32")
        return tuple(r.outs)


class AppendVerticesPipeline(NerfPipeline):
    """models/append_vertices_pipeline.py:7-94 drop-in.  data = [ray_samples, ray_translation, ray_direction,
    z_vals, images (estimator input, e.g. image indices), rgb_truth]; `smpl_estimator(images)` returns
    (goal_poses, betas) and `smpl_model(betas=, return_verts=True, body_pose=, global_orient=)` an object
    with `.vertices [B, 6890, 3]` (smplx in the reference; any callable with that contract here).

    The reference concatenates the 20 670 vertex floats IN FRONT of every sample's encoding (:56-58) and the
    net reads its "positions" from the first positions_dim columns (models/append_vertices_net.py:44-47), so
    the effective network input is a per-ray constant: the first positions_dim vertex floats and the encoded
    ray direction.  That is what is evaluated here - without materialising the
    [B*N, 20754] fp32 input rows (83 KB per sample in the reference)."""

    _single_call = None      # (estimator and body model are torch modules in front of the nets: no single-call entry)

    def __init__(self, model_coarse, model_fine, smpl_estimator, smpl_model, args, position_encoder,
                 direction_encoder):
        super().__init__(model_coarse, model_fine, args, position_encoder, direction_encoder)
        self.smpl_estimator = smpl_estimator
        self.smpl_model = smpl_model

    def _net_desc(self, net):
        return net.desc_for_rows()

    def _vertex_rows(self, images, B, dev):
        """Estimator -> body model -> the vertex floats the nets read, [B, positions_dim] (:30-41 and quirk Q7)."""
        goal_poses, betas = self.smpl_estimator(images)                                            # :30
        global_orient = torch.zeros([1, 3], device=dev).expand(B, -1)                              # :13, :36
        goal_models = self.smpl_model(betas=betas, return_verts=True, body_pose=goal_poses,
                                      global_orient=global_orient)                                 # :38-39
        vertices_flat = goal_models.vertices.reshape(B, -1)                                        # :41
        return vertices_flat[:, :self.model_coarse.positions_dim]          # the columns AppendVerticesNet.forward actually reads

    def _forward_calls(self, data):
        ray_direction = data[2]
        B = data[3].shape[0]
        ray_inputs = self._vertex_rows(data[4], B, data[0].device)

        def stage(samples, n, fine):
            net = self.model_fine if fine else self.model_coarse
            return net.forward_rays(ray_inputs, ray_direction, n, B * n), None, ()

        return self._march(data, stage)      # :65-67, :70, :92-94


class DynamicPipeline(NerfPipeline):
    """models/dynamic_pipeline.py:10-83 drop-in: the warp comes from the body model itself.  data = [ray_samples,
    ray_translation, ray_direction, z_vals, images (estimator input), rgb_truth]; `smpl_estimator(images)` returns (goal_poses,
    betas) and `smpl_model(betas=, return_verts=True, body_pose=, global_orient=)` an object with `.vertices [B, V, 3]` - the
    contract of AppendVerticesPipeline.  The body is posed twice, in the goal pose and in the zero ("canonical") pose (:45-50),
    and every sample moves by the attention-weighted canonical - goal of the goal vertices within args.warp_radius
    (ops.vertex_attention_warp: :51-70 in one launch, no [B, S, V] tensor).  Then the coarse net on the warped samples with
    per-sample view directions and the compositing that scales distances by |x' - o| (:81) - coarse only, whatever
    args.run_fine says (:83).  Returns (rgb, rgb, warp [B,S,3], ray_samples, warped [B,S,3], densities).  The loss reaches the
    estimator's poses through the warp (solver/dynamic_solver.py): both kernels are differentiable."""

    _single_call = None      # (estimator and body model are torch modules in front of the warp: no single-call entry)

    def __init__(self, model_coarse, model_fine, smpl_estimator, smpl_model, args, position_encoder, direction_encoder):
        super().__init__(model_coarse, model_fine, args, position_encoder, direction_encoder)
        self.smpl_estimator = smpl_estimator
        self.smpl_model = smpl_model

    def _forward_calls(self, data):
        ray_samples, ray_translation, ray_direction, z_vals, images, _ = data
        args = self.args
        B = z_vals.shape[0]
        dev = ray_samples.device
        goal_poses, betas = self.smpl_estimator(images)                                            # :36
        global_orient = torch.zeros([1, 3], device=dev).expand(B, -1)                              # :18, :42
        canonical_pose = torch.zeros([1, 69], device=dev).expand(B, -1)                            # :19, :43
        canonical = self.smpl_model(betas=betas, return_verts=True, body_pose=canonical_pose,
                                    global_orient=global_orient).vertices                          # :45-47
        goal = self.smpl_model(betas=betas, return_verts=True, body_pose=goal_poses,
                               global_orient=global_orient).vertices                               # :48-50
        warp, warped, sdirs = ops.vertex_attention_warp(ray_samples, goal, canonical.expand_as(goal), ray_translation,
                                                        args.warp_radius, args.warp_temperature)   # :51-70

        def stage(samples, n, fine):      # :68-78
            return self.model_coarse.forward_fused(warped, sdirs, n, self.position_encoder, self.direction_encoder), sdirs, (warp, warped)

        return self._march(data, stage, coarse_only=True)      # :81, :83


class ImageWisePipeline(NerfPipeline):
    """The forward of solver/image_wise_solver.py:73-116 (--model_type image_wise_dynamic; the reference has no pipeline class for
    it, its solver carries the forward) with DynamicPipeline's return tuple.  ONE body per image: pose_image() asks the estimator
    for the image's pose - `smpl_estimator(1)` returns (goal_pose [1, 69], betas) - and poses the body model in the zero pose and
    in the goal pose, without a global_orient as the reference does (:77-79); the two [1, V, 3] vertex tensors stay with the
    pipeline and every ray batch of that image is warped with them, autograd graph included: the trainer's
    backward(retain_graph=True) of every batch flows through the same, by then stale, vertices into the estimator (:121).
    forward(data), data = [ray_samples, ray_translation, ray_direction, z_vals, rgb_truth]: every sample moves by the
    linear-attention sum of canonical - goal over the goal vertices within args.warp_radius (ops.image_wise_warp: :89-101 in one
    launch, no [B, S, V] and no [B, V, 3] tensor), then the coarse net on the warped samples with per-sample view directions and
    the compositing that scales distances by |x' - o| (:103-116) - coarse only.  z_vals may be [S]: the reference hands ONE row of
    depths to raw2outputs for the whole batch (datasets/image_wise_dataset.py:154).  Returns (rgb, rgb, warp [B,S,3],
    ray_samples, warped [B,S,3], densities)."""

    _single_call = None      # (the body comes from torch modules in front of the warp: no single-call entry)
    warp_eps = 1e-5          # image_wise_solver.py:96

    def __init__(self, model_coarse, model_fine, smpl_estimator, smpl_model, args, position_encoder, direction_encoder):
        super().__init__(model_coarse, model_fine, args, position_encoder, direction_encoder)
        self.smpl_estimator = smpl_estimator
        self.smpl_model = smpl_model
        self.goal_vertices = self.canonical_vertices = None

    def pose_image(self):
        """Poses the body for the next image (:73-81) under the caller's grad mode; returns (goal, canonical), each [1, V, 3]."""
        goal_pose, betas = self.smpl_estimator(1)                                                  # :73
        canonical = self.smpl_model(betas=betas, return_verts=True, body_pose=torch.zeros_like(goal_pose)).vertices   # :29, :77
        goal = self.smpl_model(betas=betas, return_verts=True, body_pose=goal_pose).vertices       # :79
        self.goal_vertices, self.canonical_vertices = goal, canonical
        return goal, canonical

    def _forward_calls(self, data):
        ray_samples, ray_translation, _, z_vals, _ = data
        if self.goal_vertices is None:
            raise RuntimeError("ImageWisePipeline: pose_image() has to be called once per image before its ray batches")
        B, S = ray_samples.shape[:2]
        if z_vals.dim() == 1:
            z_vals = z_vals[None, :].expand(B, S).contiguous()
        warp, warped, sdirs = ops.image_wise_warp(ray_samples, self.goal_vertices, self.canonical_vertices, ray_translation,
                                                  self.args.warp_radius, self.warp_eps)            # :89-105

        def stage(samples, n, fine):      # :103-115
            return self.model_coarse.forward_fused(warped, sdirs, n, self.position_encoder, self.direction_encoder), sdirs, (warp, warped)

        return self._march([ray_samples, ray_translation, data[2], z_vals], stage, coarse_only=True)      # :116


class VertexSpherePipeline(NerfPipeline):
    """models/vertex_sphere_pipeline.py:7-50 drop-in: the deterministic-warp ("true warp") model.  The warp is not learned and
    not computed here: it arrives with the batch, data = [ray_samples, ray_translation, ray_direction, z_vals, warp, rgb_truth]
    (vertex_sphere.VertexSphereRays computes it from the posed body with ops.vertex_sphere_warp), and a plain NeRF is trained in
    canonical space.  warped = ray_samples + warp (:28), per-sample view directions warped - o (:31), the coarse net on them and
    the compositing that scales distances by |warped - o| (:42) - DynamicPipeline's tail.  Returns (rgb, rgb, warp, ray_samples,
    warped [B,S,3], densities); with args.run_fine the reference's NotImplementedError (:50), raised before any launch."""

    _single_call = None      # (no single-call entry takes a warp from the batch)

    def _forward_calls(self, data):
        ray_samples, ray_translation, _, _, warp, _ = data
        if self.args.run_fine:
            raise NotImplementedError('calculating the deterministic/true warp for the fine samples in not implemented yet')   # :50
        warped = ray_samples + warp                                                                # :28
        sdirs = warped - ray_translation[:, None, :]                                               # :31

        def stage(samples, n, fine):      # :29-41
            return self.model_coarse.forward_fused(warped, sdirs, n, self.position_encoder, self.direction_encoder), sdirs, (warp, warped)

        return self._march(data, stage, coarse_only=True)      # :42, :48


class SingleSamplePipeline(NerfPipeline):
    """models/singe_sample_pipeline.py:6-40 drop-in (SmplPipeline; the module name is the reference's spelling): a surface colour
    field.  Every ray carries ONE sample, placed on the body, and its true warp (single_sample.SingleSampleRays computes both with
    ops.ray_mesh_first_hit): data = [ray_sample [B,3], ray_translation, ray_direction, goal_pose, warp [B,3], rgb_truth].
    warped = ray_sample + warp (:29), the view direction warped - o (:32), the coarse net on their encodings (the fused
    encode + MLP with one sample per ray) and rgb = sigmoid(raw[..., :3]) (:39): no density, no compositing.  Returns (rgb, rgb).
    The constructor is the reference's: there is no fine net."""

    _single_call = None      # (no single-call entry renders without compositing)

    def __init__(self, model_coarse, args, position_encoder, direction_encoder):
        super().__init__(model_coarse, model_coarse, args, position_encoder, direction_encoder)

    def _forward_calls(self, data):
        ray_sample, ray_translation, _, _, warp, _ = data
        warped = ray_sample + warp                                                                 # :29
        raw = self.model_coarse.forward_fused(warped, warped - ray_translation, 1, self.position_encoder,
                                              self.direction_encoder)                              # :30-38
        rgb = torch.sigmoid(raw[..., :3])                                                          # :39
        return rgb, rgb                                                                            # :40

    def ray_maps(self, data, out):
        """NerfPipeline.ray_maps for the one sample of every ray: there is no density, so alpha = 1 as in raw2outputs' early
        return for a single sample (utils.py:170-171) - acc = 1, depth = the parameter of the un-warped sample data[0] on its ray
        (depth * |d|: SingleSampleRays.depth where the ray hits, the far bound where it misses), point = that sample."""
        ray_sample = data[0]
        ones = torch.ones((ray_sample.shape[0], 1), device=ray_sample.device, dtype=torch.float32)
        return ops.ray_maps(ones, data[1], data[2], samples=ray_sample[:, None, :])


class AppendSmplParamsPipeline(NerfPipeline):
    """models/append_smpl_params_pipeline.py:7-91 drop-in (the paper's headline model): NerfPipeline whose nets
    read [pose | PE(x) | PE(d)] rows, the pose being the 69 SMPL body-pose parameters of the ray's frame,
    optionally encoded (args.human_pose_encoding).  The pose columns are per-ray constants: they are read as
    the fused kernel's `additional` input (weight columns in front of the position encoding) instead of
    being expanded to every sample."""

    _pose_in_batch = 1

    def __init__(self, model_coarse, model_fine, args, position_encoder, direction_encoder, human_pose_encoder):
        super().__init__(model_coarse, model_fine, args, position_encoder, direction_encoder)
        self.human_pose_encoder = human_pose_encoder

    def _select(self, goal_pose):
        return goal_pose

    def _net_desc(self, net):
        return net.desc_for_encoders(self.position_encoder, self.direction_encoder, True)

    def _pose_rows(self, goal_pose):
        """The per-ray rows the nets read as additional inputs, [B, additional_input_dim] fp32 (:29-37)."""
        goal_pose = self._select(goal_pose).contiguous()
        pose = self.human_pose_encoder.encode(goal_pose) if self.args.human_pose_encoding else goal_pose
        return pose.reshape(pose.shape[0], -1).contiguous().float()

    def _forward_calls(self, data):
        ray_direction = data[2]
        pose = self._pose_rows(data[4])

        def stage(samples, n, fine):      # :49-52, :77-81
            net = self.model_fine if fine else self.model_coarse
            return net.forward_fused(samples, ray_direction, n, self.position_encoder, self.direction_encoder, additional=pose,
                                     add_first=True), None, ()

        return self._march(data, stage)      # :55-57, :60, :89-91

    def _single_call(self, data):
        """snerf_render_rays_add_f32: the pose rows as the nets' per-ray additional inputs, folded per ray inside the call in fp32."""
        pose = self._pose_rows(data[4])
        r = self._render_setup(data, (self.model_coarse, self.model_fine), "snerf_render_rays_add_workspace_bytes", True)
        with _on_device(r.dev), _lib.timed("render_rays_add"):
            check(r.lib.snerf_render_rays_add_f32(*r.head, *r.mid, ptr(pose), *r.tail, *map(ptr, r.outs), current_stream()),
                  "snerf_render_rays_add_f32")
        return self._render_result(data, r)


class AppendToNerfPipeline(AppendSmplParamsPipeline):
    """models/append_to_nerf_pipeline.py:7-90 drop-in: the same with only joints 38 and 41 of the pose (:26)."""

    def _select(self, goal_pose):
        return joints_38_41(goal_pose)
