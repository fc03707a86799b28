"""Drop-in operators with the reference's names, signatures and error behaviour, running on the
HIP library (include/smplnerf.h).  Reference counterparts:

    searchsorted        torchsearchsorted/src/torchsearchsorted/searchsorted.py:20-53
    PositionalEncoder   utils.py:114-131
    raw2outputs         utils.py:134-191
    ray_maps            utils.py:184, :187 (depth_map and acc_map, which raw2outputs computes and drops) and the expected point
    sample_pdf         utils.py:194-228
    fine_sampling       utils.py:231-264
    vertex_attention_warp   models/dynamic_pipeline.py:51-70 (the attention warp of DynamicPipeline as one operator)
    GaussianMixture / gaussian_mixture_pdf   utils.py:72-111 (the canonical-density term of SmplNerfSolver's loss)
    smpl_lbs            the body model the reference takes from smplx (train.py:214): SMPL linear blend skinning
    ray_mesh_hits / vertex_sphere_warp   datasets/vertex_sphere_dataset.py:84-116 (trimesh's intersector) and :128-159 (the true warp)
    ray_mesh_first_hit                   render.py:222-319 (get_warp: the depth and the true warp of the single-sample model)
    render_mesh                          render.py:322-367 (render_scene: the textured, lit frames create_dataset.py saves; Lambert, not pyrender's shader)
    ssim / image_scores util/scores.py:88-173 (ssim) and :11-48 (img2mse, img2psnr): the scores of print_scores, on the device
    conv3x3_block       models/smpl_estimator.py:35-39: one conv - BatchNorm (eval) - ReLU - pool block of SmplEstimator, inference only
    conv3x3_bn_block    the same block under nn.Module.train(): BatchNorm on the batch statistics, differentiable to every input
    lpips               util/scores.py:286-456 (ContentLoss as LPIPS() configures it) on the weights of a lpips.VggLpips; its parts:
                        conv3x3_block_tap (the block's un-pooled and pooled maps from one launch) and feature_distance
    lpips_loss          the same ContentLoss as the _Loss it is: differentiable to both frames, the weights frozen (:340); its parts:
                        feature_distance_bwd, relu_pool_bwd and lpips_bwd (the whole backward, one call)

Every function takes CUDA (ROCm) fp32 tensors and launches on PyTorch's current stream.  There is
no CPU implementation here: a CPU tensor is an error, like a missing library.
"""
from __future__ import annotations

import collections
import ctypes
import math
import platform
import weakref
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr


def _need_cuda(name: str, t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError(f"smpl_nerf_amd: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"smpl_nerf_amd: `{name}` must be float32 (got {t.dtype})")


# ------------------------------------------------------------------------------------------------
# a6 searchsorted
# ------------------------------------------------------------------------------------------------
def searchsorted(a: torch.Tensor, v: torch.Tensor, out: Optional[torch.LongTensor] = None,
                 side="left") -> torch.LongTensor:
    """Same contract as torchsearchsorted.searchsorted (searchsorted.py:20-53): 2-D `a` (sorted rows)
    and `v`, equal row counts or one of them a single row, int64 result of shape
    (max(rows), v.shape[1]); `out` may be supplied."""
    # the reference's preconditions (searchsorted.py:21-36) as AssertionErrors, in this package's own words
    assert a.dim() == 2, f"searchsorted: `a` must have two dimensions (rows of sorted values), got {a.dim()}"
    assert v.dim() == 2, f"searchsorted: `v` must have two dimensions (rows of queries), got {v.dim()}"
    assert a.shape[0] == v.shape[0] or a.shape[0] == 1 or v.shape[0] == 1, (
        f"searchsorted: `a` has {a.shape[0]} rows and `v` {v.shape[0]}: the counts must match, or one side must be a single row "
        "that is broadcast")
    assert a.device == v.device, f"searchsorted: `a` is on {a.device} but `v` on {v.device}"
    result_shape = (max(a.shape[0], v.shape[0]), v.shape[1])
    if out is not None:
        assert out.device == a.device, f"searchsorted: `out` is on {out.device}, the inputs on {a.device}"
        assert out.dtype == torch.long, f"searchsorted: `out` must be int64 (torch.long), got {out.dtype}"
        assert out.shape == result_shape, f"searchsorted: `out` has shape {tuple(out.shape)}, the result has {result_shape}"
    else:
        out = torch.empty(result_shape, device=v.device, dtype=torch.long)
    for nm, t in (("a", a), ("v", v)):
        if not t.is_cuda:
            raise RuntimeError(f"smpl_nerf_amd: `{nm}` must live on the GPU (got {t.device}); there is no CPU path")
    code = _SEARCHSORTED_DTYPES.get(a.dtype)
    if code is None:     # the reference dispatches AT_DISPATCH_ALL_TYPES (searchsorted_cpu_wrapper.cpp:100): no half / bool
        raise RuntimeError(f"searchsorted: unsupported dtype {a.dtype}")
    if v.dtype != a.dtype:   # the reference reads `v` through a's scalar type and fails on a mismatch (:103)
        raise RuntimeError(f"searchsorted: `a` ({a.dtype}) and `v` ({v.dtype}) must have the same dtype")
    if not a.is_contiguous() or not v.is_contiguous() or not out.is_contiguous():
        # the reference's CUDA wrapper asserts contiguity (searchsorted_cuda_wrapper.cpp:5-7)
        raise RuntimeError("searchsorted: a, v and out must be contiguous")
    lib = _lib.load()
    with torch.cuda.device(a.device):
        check(lib.snerf_searchsorted(code, ptr(a), a.shape[0], a.shape[1], ptr(v), v.shape[0], v.shape[1], ptr(out),
                                     1 if side == "left" else 0, current_stream()), "snerf_searchsorted")
    return out


# torch dtype -> SNERF_DTYPE_* (include/smplnerf.h)
_SEARCHSORTED_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3, torch.int16: 4, torch.int8: 5,
                        torch.uint8: 6}


# ------------------------------------------------------------------------------------------------
# a1 PositionalEncoder
# ------------------------------------------------------------------------------------------------
class PositionalEncoder:
    """utils.py:114-131.  `output_dim` counts embedding functions per input channel exactly like the
    reference (train.py multiplies it by 3)."""

    def __init__(self, number_frequencies, include_identity):
        self.number_frequencies = int(number_frequencies)
        self.include_identity = include_identity
        self.output_dim = (1 if include_identity else 0) + 2 * self.number_frequencies

    def encode(self, coordinate: torch.Tensor) -> torch.Tensor:
        _need_cuda("coordinate", coordinate)
        if torch.is_grad_enabled() and coordinate.requires_grad:     # differentiable like utils.py:123-131
            return _PosEncFn.apply(coordinate, self.number_frequencies, 1 if self.include_identity else 0)
        return self._encode(coordinate)

    def _encode(self, coordinate: torch.Tensor) -> torch.Tensor:
        x = coordinate.contiguous()
        c = x.shape[-1]
        n = x.numel() // c if c else 0
        out = torch.empty(x.shape[:-1] + (c * self.output_dim,), device=x.device, dtype=torch.float32)
        if out.numel() == 0:
            return out
        lib = _lib.load()
        with torch.cuda.device(x.device):
            check(lib.snerf_posenc_f32(ptr(x), n, c, self.number_frequencies, 1 if self.include_identity else 0,
                                       ptr(out), current_stream()), "snerf_posenc_f32")
        return out


class _PosEncFn(torch.autograd.Function):
    """encode() under autograd: snerf_posenc_f32 forward, snerf_posenc_bwd_f32 backward."""

    @staticmethod
    def forward(ctx, x, L, identity):
        x = x.detach().contiguous()
        ctx.save_for_backward(x)
        ctx.cfg = (int(L), int(identity))
        return PositionalEncoder(L, bool(identity))._encode(x)

    @staticmethod
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        L, identity = ctx.cfg
        c = x.shape[-1]
        n = x.numel() // c if c else 0
        d_x = torch.zeros_like(x)
        if n == 0 or (identity + 2 * L) == 0:
            return d_x, None, None
        d_out = d_out.contiguous().float()
        lib = _lib.load()
        with torch.cuda.device(x.device):
            check(lib.snerf_posenc_bwd_f32(ptr(x), ptr(d_out), n, c, L, identity, ptr(d_x), current_stream()),
                  "snerf_posenc_bwd_f32")
        return d_x, None, None


# ------------------------------------------------------------------------------------------------
# a4 raw2outputs
# ------------------------------------------------------------------------------------------------
def _directions_arg(samples_directions: torch.Tensor, B: int, N: int):
    """(tensor, per_sample flag).  The pipelines pass ray directions as an expanded [B,N,3] view
    (models/nerf_pipeline.py:30-32); a zero stride over the sample axis is consumed as [B,3]."""
    d = samples_directions
    if d.dim() == 2 and d.shape == (B, 3):
        return d.contiguous(), 0
    if d.dim() == 3 and d.shape == (B, N, 3):
        if N == 1 or d.stride(1) == 0:
            return d[:, 0, :].contiguous(), 0
        return d.contiguous(), 1
    if d.dim() == 1 and d.shape[0] == 3:
        return d.expand(B, 3).contiguous(), 0
    raise RuntimeError(f"raw2outputs: samples_directions of shape {tuple(d.shape)} does not match raw [B={B}, N={N}]")


class _CompositeFn(torch.autograd.Function):
    """Differentiable alpha compositing, all of utils.py:134-191 under autograd: gradients arriving at rgb, weights and
    alpha (SmplNerfSolver's density loss reads the returned alpha, solver/smpl_nerf_solver.py:40) flow to raw and, where the
    caller's graph asks, to the directions (per-sample: SmplNerfPipeline's x' - o; per-ray) and to z_vals
    (snerf_composite_bwd_all_f32)."""

    @staticmethod
    def forward(ctx, raw, z_vals, dirs, per_sample, white_background, noise, want_weights, want_alpha):
        rgb, weights, alpha = _composite_launch(raw, z_vals, dirs, per_sample, white_background, noise,
                                                want_weights, want_alpha)
        ctx.save_for_backward(raw, z_vals, dirs, noise)
        ctx.cfg = (per_sample, white_background, bool(ctx.needs_input_grad[1]), bool(ctx.needs_input_grad[2]))
        ctx.set_materialize_grads(False)
        return rgb, weights, alpha

    @staticmethod
    def backward(ctx, d_rgb, d_w, d_a):
        raw, z_vals, dirs, noise = ctx.saved_tensors
        per_sample, wb, want_dz, want_ddirs = ctx.cfg
        if d_rgb is None and d_w is None and d_a is None:
            return (None,) * 8
        B, N = z_vals.shape
        d_rgb, d_w, d_a = (None if g is None else g.contiguous().float() for g in (d_rgb, d_w, d_a))
        d_raw = torch.empty_like(raw)
        d_dirs = torch.empty_like(dirs) if want_ddirs else None
        d_z = torch.empty_like(z_vals) if want_dz else None
        lib = _lib.load()
        with torch.cuda.device(raw.device), _lib.timed(f"composite_bwd[N={N}]"):
            check(lib.snerf_composite_bwd_all_f32(ptr(raw), ptr(z_vals), ptr(dirs), per_sample, ptr(noise), B, N,
                                                  1 if wb else 0, ptr(d_rgb), ptr(d_w), ptr(d_a), ptr(d_raw), ptr(d_dirs),
                                                  ptr(d_z), current_stream()), "snerf_composite_bwd_all_f32")
        return (d_raw, d_z, d_dirs) + (None,) * 5


def composite(raw, z_vals, samples_directions, white_background: bool, noise=None,
              want_weights=True, want_alpha=True):
    B, N = z_vals.shape
    for nm, t in (("raw", raw), ("z_vals", z_vals), ("samples_directions", samples_directions), ("noise", noise)):
        if t is not None:
            _need_cuda(nm, t)
    dirs, per_sample = _directions_arg(samples_directions, B, N)
    raw = raw.contiguous()
    z_vals = z_vals.contiguous()
    if noise is not None:
        noise = noise.contiguous()
    if torch.is_grad_enabled() and (raw.requires_grad or z_vals.requires_grad or dirs.requires_grad):
        return _CompositeFn.apply(raw.view(B, N, 4), z_vals, dirs, per_sample, bool(white_background), noise, want_weights,
                                  want_alpha)
    return _composite_launch(raw, z_vals, dirs, per_sample, white_background, noise, want_weights, want_alpha)


def _composite_launch(raw, z_vals, dirs, per_sample, white_background, noise, want_weights, want_alpha):
    B, N = z_vals.shape
    dev = raw.device
    rgb = torch.empty((B, 3), device=dev, dtype=torch.float32)
    weights = torch.empty((B, N), device=dev, dtype=torch.float32) if want_weights else None
    alpha = torch.empty((B, N), device=dev, dtype=torch.float32) if want_alpha else None
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"composite_fwd[N={N}]"):
        check(lib.snerf_composite_fwd_f32(ptr(raw), ptr(z_vals), ptr(dirs), per_sample, ptr(noise), B, N,
                                          1 if white_background else 0, ptr(rgb), ptr(weights), ptr(alpha),
                                          current_stream()), "snerf_composite_fwd_f32")
    return rgb, weights, alpha


def raw2outputs(raw: torch.Tensor, z_vals: torch.Tensor, samples_directions: torch.Tensor,
                args) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """utils.py:134-191: returns (rgb [B,3], weights [B,N], density/alpha [B,N]).  Reads
    args.sigma_noise_std and args.white_background; the Gaussian sigma noise is drawn here with
    torch.normal exactly where the reference draws it (utils.py:171-173) - also in eval mode."""
    for nm, t in (("raw", raw), ("z_vals", z_vals), ("samples_directions", samples_directions)):
        _need_cuda(nm, t)
    noise = None
    if z_vals.shape[-1] > 1 and args.sigma_noise_std > 0.:
        noise = torch.normal(0, args.sigma_noise_std, raw[..., 3].shape, device=raw.device)
    return composite(raw, z_vals, samples_directions, bool(args.white_background), noise)


# ------------------------------------------------------------------------------------------------
# ray maps: acc_map, depth_map (utils.py:184, :187) and the expected point
# ------------------------------------------------------------------------------------------------
RayMaps = collections.namedtuple("RayMaps", "acc depth point")


class _RayMapsFn(torch.autograd.Function):
    """ray_maps() under autograd: snerf_ray_maps_fwd_f32 forward, snerf_ray_maps_bwd_f32 backward, differentiable in alpha alone
    (the sample positions are detached in the reference, utils.py:260).  Its d alpha is what _CompositeFn takes as d_a."""

    @staticmethod
    def forward(ctx, alpha, o, d, z_vals, samples):
        ctx.save_for_backward(alpha, o, d, z_vals, samples)
        ctx.set_materialize_grads(False)
        return _ray_maps_launch(alpha, o, d, z_vals, samples)

    @staticmethod
    def backward(ctx, d_acc, d_depth, d_point):
        alpha, o, d, z_vals, samples = ctx.saved_tensors
        if d_acc is None and d_depth is None and d_point is None:
            return (None,) * 5
        B, N = alpha.shape
        d_acc, d_depth, d_point = (None if g is None else g.contiguous().float() for g in (d_acc, d_depth, d_point))
        d_alpha = torch.empty_like(alpha)
        if B == 0:
            return d_alpha, None, None, None, None
        lib = _lib.load()
        with torch.cuda.device(alpha.device), _lib.timed(f"ray_maps_bwd[N={N}]"):
            check(lib.snerf_ray_maps_bwd_f32(ptr(alpha), ptr(z_vals), ptr(samples), ptr(o), ptr(d), B, N, ptr(d_acc), ptr(d_depth),
                                             ptr(d_point), ptr(d_alpha), current_stream()), "snerf_ray_maps_bwd_f32")
        return d_alpha, None, None, None, None


def ray_maps(alpha, ray_translation, ray_direction, z_vals=None, samples=None) -> RayMaps:
    """The maps raw2outputs computes and drops (utils.py:184, :187) and the expected point, from the per-sample alpha [B, N] of a
    compositing (composite()'s third result, a pipeline's `densities`): RayMaps(acc [B] = sum of the weights, depth [B] = sum of
    weights * t, point [B, 3] = sum of weights * samples, or None without samples).  Exactly one of z_vals [B, N] (t = z_vals, the
    reference's expression) and samples [B, N, 3] (t = ((p - o) . d) / (d . d): for callers who hold the points o + t d but not
    the depths, like the results of a pipeline).  The weights are rebuilt from alpha with the compositing kernel's own rounding
    (include/smplnerf.h).  Differentiable in alpha: a loss on depth or acc reaches the nets through composite()'s alpha."""
    for nm, t in (("alpha", alpha), ("ray_translation", ray_translation), ("ray_direction", ray_direction), ("z_vals", z_vals),
                  ("samples", samples)):
        if t is not None:
            _need_cuda(nm, t)
    if (z_vals is None) == (samples is None):
        raise RuntimeError("ray_maps: exactly one of z_vals and samples must be given")
    if alpha.dim() != 2:
        raise RuntimeError(f"ray_maps: alpha must be [B, N], got {tuple(alpha.shape)}")
    B, N = alpha.shape
    for nm, t, shape in (("ray_translation", ray_translation, (B, 3)), ("ray_direction", ray_direction, (B, 3)),
                         ("z_vals", z_vals, (B, N)), ("samples", samples, (B, N, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise RuntimeError(f"ray_maps: {nm} of shape {tuple(t.shape)} does not match alpha [B={B}, N={N}]: expected {shape}")
    alpha, o, d = alpha.contiguous(), ray_translation.detach().contiguous(), ray_direction.detach().contiguous()
    z_vals = None if z_vals is None else z_vals.detach().contiguous()
    samples = None if samples is None else samples.detach().contiguous()
    if torch.is_grad_enabled() and alpha.requires_grad:
        return RayMaps(*_RayMapsFn.apply(alpha, o, d, z_vals, samples))
    return RayMaps(*_ray_maps_launch(alpha.detach(), o, d, z_vals, samples))


def _ray_maps_launch(alpha, o, d, z_vals, samples):
    B, N = alpha.shape
    dev = alpha.device
    acc = torch.empty((B,), device=dev, dtype=torch.float32)
    depth = torch.empty((B,), device=dev, dtype=torch.float32)
    point = torch.empty((B, 3), device=dev, dtype=torch.float32) if samples is not None else None
    if B == 0:      # (an empty tensor has no address to tell z_vals from samples by)
        return acc, depth, point
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"ray_maps_fwd[N={N}]"):
        check(lib.snerf_ray_maps_fwd_f32(ptr(alpha), ptr(z_vals), ptr(samples), ptr(o), ptr(d), B, N, ptr(acc), ptr(depth),
                                         ptr(point), current_stream()), "snerf_ray_maps_fwd_f32")
    return acc, depth, point


# ------------------------------------------------------------------------------------------------
# a5 sample_pdf / fine_sampling
# ------------------------------------------------------------------------------------------------
_U_CACHE = {}


def uniform_u(n: int, device) -> torch.Tensor:
    """u = torch.linspace(0., 1., steps=n) (utils.py:206), evaluated by the same torch CPU kernel the
    reference's CPU path uses, then kept on the device."""
    key = (int(n), str(device))
    u = _U_CACHE.get(key)
    if u is None:
        u = torch.linspace(0., 1., steps=int(n)).to(device)
        _U_CACHE[key] = u
    return u


# the rows device_reference_sum_ok() holds the library's order against torch.sum with
_REFSUM_PROBE_LENGTHS = (1, 7, 8, 9, 31, 32, 33, 62, 63, 126, 190, 511, 512, 513, 1022)
_REFSUM_MAX_N = 32767          # include/smplnerf.h snerf_reference_sum_f32
_REFSUM_OK = None


def _reference_sum_probe() -> bool:
    """True when torch.sum on this host follows the order of snerf_reference_sum_*_f32 (csrc/refsum.h): an x86_64 machine, a
    capability whose float sum runs on 8-lane vectors (DEFAULT, AVX2, AVX512) and a CPU-only comparison of the host entry
    with torch.sum on fixed seeded rows.  No device work, so it is safe under graph capture."""
    if platform.machine().lower() not in ("x86_64", "amd64"):
        return False
    if torch.backends.cpu.get_cpu_capability() not in ("DEFAULT", "AVX2", "AVX512"):
        return False
    lib = _lib.load()
    g = torch.Generator().manual_seed(2026)
    for n in _REFSUM_PROBE_LENGTHS:
        x = torch.pow(10.0, torch.rand((4, n), generator=g) * 6 - 3).float().contiguous()
        for add in (0.0, 1e-5):
            got = torch.empty(4, dtype=torch.float32)
            check(lib.snerf_reference_sum_host_f32(x.data_ptr(), n, 4, n, add, got.data_ptr()), "snerf_reference_sum_host_f32")
            if not torch.equal(torch.sum(x + add, -1).view(torch.int32), got.view(torch.int32)):
                return False
    return True


def device_reference_sum_ok() -> bool:
    """Whether the device can stand in for torch's CPU sum in strict mode (decided once per process, _reference_sum_probe)."""
    global _REFSUM_OK
    if _REFSUM_OK is None:
        _REFSUM_OK = _reference_sum_probe()
    return _REFSUM_OK


def _host_normalising_sum(interior_weights: torch.Tensor) -> torch.Tensor:
    """The sum by torch's own CPU kernel: a device -> host -> device round trip and a sync (hosts whose torch.sum takes
    another order than the library's, see device_reference_sum_ok)."""
    w = interior_weights.detach().to("cpu", torch.float32)
    return torch.sum(w + 1e-5, -1).to(interior_weights.device).contiguous()


def reference_normalising_sum(interior_weights: torch.Tensor) -> torch.Tensor:
    """torch.sum(weights + 1e-5, -1) of utils.py:200-201 bit for bit as torch's CPU kernel evaluates it - exactly what the
    reference's CPU path computes (ATen's fp32 cascade over 8-lane vectors: one order on every x86 host, restated in
    csrc/refsum.h) - returned on the weights' device.  Where device_reference_sum_ok(), snerf_reference_sum_f32 computes it on
    the device (no sync; graph-capturable); elsewhere torch computes it on the host.  Used in strict mode (args.strict_cumsum)."""
    w = interior_weights.detach()
    if w.dim() != 2 or not w.is_cuda or w.dtype != torch.float32 or w.shape[1] > _REFSUM_MAX_N or not device_reference_sum_ok():
        return _host_normalising_sum(interior_weights)
    if w.shape[1] > 1 and w.stride(1) != 1 or w.shape[0] > 1 and w.stride(0) < w.shape[1]:
        w = w.contiguous()
    B, n = w.shape
    out = torch.empty(B, device=w.device, dtype=torch.float32)
    lib = _lib.load()
    with torch.cuda.device(w.device), _lib.timed("reference_sum"):
        check(lib.snerf_reference_sum_f32(ptr(w), w.stride(0) if B > 1 else n, B, n, 1e-5, ptr(out), current_stream()),
              "snerf_reference_sum_f32")
    return out


def hierarchical_samples(ray_translation, ray_direction, z_vals, weights, number_fine_samples: int,
                         want_inds=False, want_samples=False, tot=None, strict=False):
    """One launch of snerf_sample_pdf_f32 -> dict(z_fine, pts, [inds], [z_samples]).  strict (or an explicit `tot` [B]):
    the normalising sums in the order of torch's CPU kernel (reference_normalising_sum), so the indices equal the reference's
    bit for bit from the same weights (snerf_sample_pdf_strict_f32)."""
    B, Nc = z_vals.shape
    Nf = int(number_fine_samples)
    dev = z_vals.device
    for nm, t in (("ray_translation", ray_translation), ("ray_direction", ray_direction), ("z_vals", z_vals),
                  ("weights", weights)):
        _need_cuda(nm, t)
    z_vals, weights = z_vals.contiguous(), weights.contiguous()
    o, d = ray_translation.contiguous(), ray_direction.contiguous()
    u = uniform_u(Nf, dev)
    z_fine = torch.empty((B, Nc + Nf), device=dev, dtype=torch.float32)
    pts = torch.empty((B, Nc + Nf, 3), device=dev, dtype=torch.float32)
    inds = torch.empty((B, Nf), device=dev, dtype=torch.long) if want_inds else None
    zs = torch.empty((B, Nf), device=dev, dtype=torch.float32) if want_samples else None
    lib = _lib.load()
    if tot is None and strict:
        tot = reference_normalising_sum(weights[:, 1:-1])
    if tot is not None:
        _need_cuda("tot", tot)
        tot = tot.reshape(-1).contiguous()
        if tot.shape[0] != B:
            raise RuntimeError(f"hierarchical_samples: tot must have one entry per ray ({B}), got {tot.shape[0]}")
        with torch.cuda.device(dev), _lib.timed("sample_pdf"):
            check(lib.snerf_sample_pdf_strict_f32(ptr(z_vals), ptr(weights), ptr(u), ptr(o), ptr(d), ptr(tot), B, Nc, Nf,
                                                  ptr(inds), ptr(zs), ptr(z_fine), ptr(pts), current_stream()),
                  "snerf_sample_pdf_strict_f32")
        return dict(z_fine=z_fine, pts=pts, inds=inds, z_samples=zs)
    with torch.cuda.device(dev), _lib.timed("sample_pdf"):
        check(lib.snerf_sample_pdf_f32(ptr(z_vals), ptr(weights), ptr(u), ptr(o), ptr(d), B, Nc, Nf, ptr(inds),
                                       ptr(zs), ptr(z_fine), ptr(pts), current_stream()), "snerf_sample_pdf_f32")
    return dict(z_fine=z_fine, pts=pts, inds=inds, z_samples=zs)


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, args) -> torch.Tensor:
    """utils.py:194-228 with the reference's calling convention: bins [B,Nb] (the coarse midpoints),
    weights [B,Nb-1] (the interior coarse weights).  Returns the Nf samples [B, Nf]."""
    _need_cuda("bins", bins)
    _need_cuda("weights", weights)
    B, Nb = bins.shape
    assert weights.shape == (B, Nb - 1), "weights must have one entry less than bins"
    Nf = int(args.number_fine_samples)
    want_grad = torch.is_grad_enabled() and (bins.requires_grad or weights.requires_grad)
    bins_in, weights_in = bins, weights
    bins, weights = bins.detach().contiguous(), weights.detach().contiguous()
    u = uniform_u(Nf, bins.device)
    zs = torch.empty((B, Nf), device=bins.device, dtype=torch.float32)
    inds = torch.empty((B, Nf), device=bins.device, dtype=torch.long) if want_grad else None
    lib = _lib.load()
    tot = None
    with torch.cuda.device(bins.device):
        if getattr(args, "strict_cumsum", 0):
            tot = reference_normalising_sum(weights)
            check(lib.snerf_sample_pdf_bins_strict_f32(ptr(bins), ptr(weights), ptr(u), ptr(tot), B, Nb, Nf, ptr(inds), ptr(zs),
                                                       current_stream()), "snerf_sample_pdf_bins_strict_f32")
        else:
            check(lib.snerf_sample_pdf_bins_f32(ptr(bins), ptr(weights), ptr(u), B, Nb, Nf, ptr(inds), ptr(zs),
                                                current_stream()), "snerf_sample_pdf_bins_f32")
    if not want_grad:
        return zs
    return _SamplePdfGrad.apply(bins_in, weights_in, zs, inds, u, tot)


class _SamplePdfGrad(torch.autograd.Function):
    """sample_pdf under autograd (the reference's fine_sampling detaches the result, utils.py:260, but sample_pdf itself is
    differentiable w.r.t. bins and weights, utils.py:200-228).  The values are the forward kernel's; the gradient is the
    reference's with the searchsorted indices held fixed (integers carry no gradient there either) - a piecewise-linear map
    whose pieces the kernel's `inds` select, differentiated by snerf_sample_pdf_bins_bwd_f32."""

    @staticmethod
    def forward(ctx, bins, weights, zs, inds, u, tot):
        # dense copies: the backward kernel walks [B, Nb] / [B, Nb - 1] rows by pointer, and the reference's own caller passes a
        # strided view (`weights[..., 1:-1]`, utils.py:259)
        ctx.save_for_backward(bins.detach().contiguous(), weights.detach().contiguous(), inds, u, tot)
        return zs

    @staticmethod
    def backward(ctx, d_zs):
        bins, weights, inds, u, tot = ctx.saved_tensors
        B, Nb = bins.shape
        d_zs = d_zs.contiguous().float()
        gb = torch.empty(bins.shape, device=bins.device, dtype=torch.float32)
        gw = torch.empty(weights.shape, device=bins.device, dtype=torch.float32)
        lib = _lib.load()
        with torch.cuda.device(bins.device):
            check(lib.snerf_sample_pdf_bins_bwd_f32(ptr(bins), ptr(weights), ptr(u), ptr(inds), ptr(tot), ptr(d_zs), B, Nb, inds.shape[1],
                                                    ptr(gb), ptr(gw), current_stream()), "snerf_sample_pdf_bins_bwd_f32")
        return gb, gw, None, None, None, None


def fine_sampling(ray_translation: torch.Tensor, samples_directions: torch.Tensor, z_vals: torch.Tensor,
                  weights: torch.Tensor, args) -> Tuple[torch.Tensor, torch.Tensor]:
    """utils.py:231-264 -> (z_vals [B,Nc+Nf] ascending, ray_samples_fine [B,Nc+Nf,3]); the samples are
    detached like in the reference (utils.py:260)."""
    for nm, t in (("ray_translation", ray_translation), ("samples_directions", samples_directions),
                  ("z_vals", z_vals), ("weights", weights)):
        _need_cuda(nm, t)
    r = hierarchical_samples(ray_translation.detach(), samples_directions.detach(), z_vals.detach(),
                             weights.detach(), args.number_fine_samples, strict=bool(getattr(args, "strict_cumsum", 0)))
    return r["z_fine"], r["pts"]


# ------------------------------------------------------------------------------------------------
# DynamicPipeline's vertex-attention warp (models/dynamic_pipeline.py:53-70)
# ------------------------------------------------------------------------------------------------
def _vertex_warp_launch(samples, goal, canon, ray_o, radius, temperature, want_stats):
    B, S, _ = samples.shape
    V = goal.shape[1]
    dev = samples.device
    warp, warped, sdirs = (torch.empty((B * S, 3), device=dev, dtype=torch.float32) for _ in range(3))
    stats = torch.empty((B * S, 2), device=dev, dtype=torch.float32) if want_stats else None
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"vertex_warp_fwd[V={V}]"):
        check(lib.snerf_vertex_warp_fwd_f32(ptr(samples), ptr(goal), ptr(canon), ptr(ray_o), B, S, V, radius, temperature,
                                            ptr(warp), ptr(warped), ptr(sdirs), ptr(stats), current_stream()),
              "snerf_vertex_warp_fwd_f32")
    return warp, warped, sdirs, stats


class _VertexWarpFn(torch.autograd.Function):
    """snerf_vertex_warp_fwd_f32 / snerf_vertex_warp_bwd_f32 under autograd.  warped = samples + warp and sdirs = warped - o,
    so the three incoming gradients add up to d loss / d warp; the samples also receive d warped + d sdirs directly and the
    ray origins -sum_s d sdirs."""

    @staticmethod
    def forward(ctx, samples, goal, canon, ray_o, radius, temperature):
        warp, warped, sdirs, stats = _vertex_warp_launch(samples, goal, canon, ray_o, radius, temperature, True)
        ctx.save_for_backward(samples, goal, canon, warp, stats)
        ctx.cfg = (radius, temperature)
        ctx.set_materialize_grads(False)
        return warp, warped, sdirs

    @staticmethod
    def backward(ctx, d_warp, d_warped, d_sdirs):
        if d_warp is None and d_warped is None and d_sdirs is None:
            return (None,) * 6
        samples, goal, canon, warp, stats = ctx.saved_tensors
        radius, temperature = ctx.cfg
        B, S, _ = samples.shape
        V = goal.shape[1]
        d_warp, d_warped, d_sdirs = (None if g is None else g.contiguous().float() for g in (d_warp, d_warped, d_sdirs))
        want_samples, want_o = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        d_samples = torch.empty_like(samples) if want_samples else None
        d_goal, d_canon = torch.empty_like(goal), torch.empty_like(canon)
        lib = _lib.load()
        with torch.cuda.device(samples.device), _lib.timed(f"vertex_warp_bwd[V={V}]"):
            check(lib.snerf_vertex_warp_bwd_f32(ptr(samples), ptr(goal), ptr(canon), ptr(warp), ptr(stats), ptr(d_warp),
                                                ptr(d_warped), ptr(d_sdirs), B, S, V, radius, temperature, ptr(d_samples),
                                                ptr(d_goal), ptr(d_canon), current_stream()), "snerf_vertex_warp_bwd_f32")
        d_o = None
        for g in (d_warped, d_sdirs):          # the identity paths around the attention
            if g is not None and want_samples:
                d_samples = d_samples + g.view(B, S, 3)
        if want_o and d_sdirs is not None:
            d_o = -d_sdirs.view(B, S, 3).sum(1)
        return d_samples, d_goal, d_canon, d_o, None, None


def vertex_attention_warp(ray_samples, goal_vertices, canonical_vertices, ray_translation, radius, temperature):
    """models/dynamic_pipeline.py:51-70 in one launch: every sample of ray b moves by the attention-weighted sum of
    canonical - goal over the vertices of body b within `radius` (modified_softmax of temperature * relu(radius - distance),
    utils.py:57-60).  ray_samples [B,S,3], goal_vertices / canonical_vertices [B,V,3], ray_translation [B,3] ->
    (warp, warped, sdirs), each [B*S, 3] like WarpFieldNet.forward_fused.  Differentiable with respect to both vertex
    tensors and, where they require grad, the samples and the ray origins; with autograd off the call keeps nothing for a
    backward.  No [B,S,V] tensor is built."""
    for nm, t in (("ray_samples", ray_samples), ("goal_vertices", goal_vertices), ("canonical_vertices", canonical_vertices),
                  ("ray_translation", ray_translation)):
        _need_cuda(nm, t)
    if ray_samples.dim() != 3 or ray_samples.shape[-1] != 3:
        raise RuntimeError(f"vertex_attention_warp: ray_samples must be [B, S, 3], got {tuple(ray_samples.shape)}")
    B, S = ray_samples.shape[:2]
    if goal_vertices.dim() != 3 or goal_vertices.shape[0] != B or goal_vertices.shape[-1] != 3 or \
            canonical_vertices.shape != goal_vertices.shape or tuple(ray_translation.shape) != (B, 3):
        raise RuntimeError(f"vertex_attention_warp: goal {tuple(goal_vertices.shape)}, canonical {tuple(canonical_vertices.shape)} "
                           f"and ray_translation {tuple(ray_translation.shape)} do not match ray_samples [B={B}, S={S}, 3]")
    if S < 1 or goal_vertices.shape[1] < 1:
        raise RuntimeError("vertex_attention_warp: needs at least one sample per ray and one vertex")
    x, g, c, o = (t.contiguous() for t in (ray_samples, goal_vertices, canonical_vertices, ray_translation))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, g, c, o)):
        return _VertexWarpFn.apply(x, g, c, o, float(radius), float(temperature))
    return _vertex_warp_launch(x, g, c, o, float(radius), float(temperature), False)[:3]


# ------------------------------------------------------------------------------------------------
# The image-wise model's linear-attention warp, one body per image (solver/image_wise_solver.py:89-105)
# ------------------------------------------------------------------------------------------------
def _image_warp_launch(samples, goal, canon, ray_o, radius, eps, want_stats):
    B, S, _ = samples.shape
    V = goal.shape[-2]
    dev = samples.device
    warp, warped, sdirs = (torch.empty((B * S, 3), device=dev, dtype=torch.float32) for _ in range(3))
    stats = torch.empty((B * S, 4), device=dev, dtype=torch.float64) if want_stats else None      # D and the unrounded warp
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"image_warp_fwd[V={V}]"):
        check(lib.snerf_image_warp_fwd_f32(ptr(samples), ptr(goal), ptr(canon), ptr(ray_o), B, S, V, radius, eps,
                                           ptr(warp), ptr(warped), ptr(sdirs), ptr(stats), current_stream()),
              "snerf_image_warp_fwd_f32")
    return warp, warped, sdirs, stats


class _ImageWarpFn(torch.autograd.Function):
    """snerf_image_warp_fwd_f32 / snerf_image_warp_bwd_f32 under autograd: _VertexWarpFn with one body for all rays.  The three
    incoming gradients add up to d loss / d warp; the samples also receive d warped + d sdirs directly (inside the kernel, which
    rounds their gradient once) and the ray origins -sum_s d sdirs.  The vertex gradients are sums over every sample of the batch,
    taken on the device in a fixed order."""

    @staticmethod
    def forward(ctx, samples, goal, canon, ray_o, radius, eps):
        warp, warped, sdirs, stats = _image_warp_launch(samples, goal, canon, ray_o, radius, eps, True)
        ctx.save_for_backward(samples, goal, canon, stats)
        ctx.radius = radius
        ctx.set_materialize_grads(False)
        return warp, warped, sdirs

    @staticmethod
    def backward(ctx, d_warp, d_warped, d_sdirs):
        if d_warp is None and d_warped is None and d_sdirs is None:
            return (None,) * 6
        samples, goal, canon, stats = ctx.saved_tensors
        B, S, _ = samples.shape
        V = goal.shape[-2]
        d_warp, d_warped, d_sdirs = (None if g is None else g.contiguous().float() for g in (d_warp, d_warped, d_sdirs))
        want_samples, want_o = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        d_samples = torch.empty_like(samples) if want_samples else None
        d_goal, d_canon = torch.empty_like(goal), torch.empty_like(canon)
        lib = _lib.load()
        nbytes = lib.snerf_image_warp_bwd_workspace_bytes(B * S, V)
        if nbytes < 0:
            check(-1, "snerf_image_warp_bwd_workspace_bytes")
        ws = torch.empty((nbytes // 8,), device=samples.device, dtype=torch.float64)
        with torch.cuda.device(samples.device), _lib.timed(f"image_warp_bwd[V={V}]"):
            check(lib.snerf_image_warp_bwd_f32(ptr(samples), ptr(goal), ptr(canon), ptr(stats), ptr(d_warp), ptr(d_warped),
                                               ptr(d_sdirs), B, S, V, ctx.radius, ptr(ws), nbytes, ptr(d_samples), ptr(d_goal),
                                               ptr(d_canon), current_stream()), "snerf_image_warp_bwd_f32")
        d_o = -d_sdirs.view(B, S, 3).sum(1) if want_o and d_sdirs is not None else None
        return d_samples, d_goal, d_canon, d_o, None, None


def image_wise_warp(ray_samples, goal_vertices, canonical_vertices, ray_translation, radius, eps=1e-5):
    """solver/image_wise_solver.py:89-105 in one launch: every sample moves by the attention-weighted sum of canonical - goal over
    the vertices of the image's ONE body within `radius`, with the linear attention relu(radius - distance) / (its sum over the
    vertices + eps) - no softmax, no temperature.  ray_samples [B,S,3], goal_vertices / canonical_vertices [V,3] or [1,V,3] (what
    the body model returns for one pose), ray_translation [B,3] -> (warp, warped, sdirs), each [B*S, 3] like
    vertex_attention_warp.  Differentiable with respect to both vertex tensors (the gradients are summed over all B*S samples on
    the device, in a fixed order) and, where they require grad, the samples and the ray origins; with autograd off the call
    keeps nothing for a backward.  No [B,S,V] and no [B,V,3] tensor is built."""
    for nm, t in (("ray_samples", ray_samples), ("goal_vertices", goal_vertices), ("canonical_vertices", canonical_vertices),
                  ("ray_translation", ray_translation)):
        _need_cuda(nm, t)
    if ray_samples.dim() != 3 or ray_samples.shape[-1] != 3:
        raise RuntimeError(f"image_wise_warp: ray_samples must be [B, S, 3], got {tuple(ray_samples.shape)}")
    B, S = ray_samples.shape[:2]
    gs = tuple(goal_vertices.shape)
    if not (len(gs) in (2, 3) and gs[-1] == 3 and (len(gs) == 2 or gs[0] == 1)) or canonical_vertices.shape != goal_vertices.shape \
            or tuple(ray_translation.shape) != (B, 3):
        raise RuntimeError(f"image_wise_warp: goal {gs} and canonical {tuple(canonical_vertices.shape)} must be one body, [V, 3] or "
                           f"[1, V, 3], and ray_translation {tuple(ray_translation.shape)} must match ray_samples [B={B}, S={S}, 3]")
    if S < 1 or gs[-2] < 1:
        raise RuntimeError("image_wise_warp: needs at least one sample per ray and one vertex")
    x, g, c, o = (t.contiguous() for t in (ray_samples, goal_vertices, canonical_vertices, ray_translation))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, g, c, o)):
        return _ImageWarpFn.apply(x, g, c, o, float(radius), float(eps))
    return _image_warp_launch(x, g, c, o, float(radius), float(eps), False)[:3]


# ------------------------------------------------------------------------------------------------
# GaussianMixture.pdf (utils.py:72-111): the canonical-density term of SmplNerfSolver's loss
# ------------------------------------------------------------------------------------------------
def _gmm_launch(samples, means, std, want_grad):
    n, V, dev = samples.numel() // 3, means.shape[0], samples.device
    pdf = torch.empty(samples.shape[:-1], device=dev, dtype=torch.float32)
    dpdf = torch.empty(samples.shape, device=dev, dtype=torch.float32) if want_grad else None
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"gmm_pdf[V={V}]"):
        check(lib.snerf_gmm_pdf_f32(ptr(samples), ptr(means), n, V, std, ptr(pdf), ptr(dpdf), current_stream()), "snerf_gmm_pdf_f32")
    return pdf, dpdf


class _GmmPdfFn(torch.autograd.Function):
    """snerf_gmm_pdf_f32 under autograd: the forward also writes dpdf = d pdf / d samples (it is asked for only when this Function
    runs, i.e. when the samples want a gradient), so the backward is a product per sample and no second pass over the pairs."""

    @staticmethod
    def forward(ctx, samples, means, std):
        pdf, dpdf = _gmm_launch(samples, means, std, True)
        ctx.save_for_backward(dpdf)
        return pdf

    @staticmethod
    def backward(ctx, d_pdf):
        dpdf, = ctx.saved_tensors
        return d_pdf[..., None] * dpdf, None, None


def gaussian_mixture_pdf(samples, means, std):
    """utils.py:102-111 in one launch: the density of samples [..., 3] under the equal-weight mixture of V isotropic Gaussians
    with centres means [V, 3] and standard deviation std -> [...].  Differentiable with respect to the samples; the means are
    constants (as in the reference) and must not require a gradient.  Under no_grad, or when the samples do not require a
    gradient, the derivative is neither allocated nor computed.  No [..., V, 3] tensor is built."""
    _need_cuda("samples", samples)
    _need_cuda("means", means)
    if means.dim() != 2 or means.shape[-1] != 3 or means.shape[0] < 1:
        raise RuntimeError(f"gaussian_mixture_pdf: means must be [V >= 1, 3], got {tuple(means.shape)}")
    if samples.dim() < 1 or samples.shape[-1] != 3:
        raise RuntimeError(f"gaussian_mixture_pdf: samples must be [..., 3], got {tuple(samples.shape)}")
    if means.requires_grad:
        raise RuntimeError("gaussian_mixture_pdf: the means are constants (utils.py:83); `means` must not require a gradient")
    if means.device != samples.device:
        raise RuntimeError(f"gaussian_mixture_pdf: samples on {samples.device}, means on {means.device}")
    x, mu = samples.contiguous(), means.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _GmmPdfFn.apply(x, mu, float(std))
    return _gmm_launch(x.detach(), mu, float(std), False)[0]


class GaussianMixture:
    """utils.GaussianMixture (utils.py:72-111): the reference's constructor `(means: np.ndarray [V, 3], std, device)` and its
    attributes `means` (tensor on `device`), `var = std ** 2` and `factor` (computed as in utils.py:85-86); `pdf(samples)` is
    gaussian_mixture_pdf = snerf_gmm_pdf_f32.  The kernels are fp32: a float64 `means` array (what the reference's SMPL loader
    hands over) is stored as fp32, where the reference keeps its dtype and then fails on fp32 samples or promotes them.  A
    tensor is accepted as well as an array."""

    def __init__(self, means, std, device):
        import numpy as np
        if isinstance(means, torch.Tensor):
            means = means.detach().cpu().numpy()
        means = np.asarray(means)
        self.means = torch.from_numpy(np.ascontiguousarray(means, dtype=np.float32)).to(device)
        self._std = float(std)
        self.var = std ** 2
        cov_det = self.var ** means.shape[-1]
        self.factor = 1 / np.sqrt(((2 * np.pi) ** means.shape[-1] * cov_det))

    def pdf(self, samples):
        if samples.shape[-1] != self.means.shape[-1]:
            raise ValueError("Dimension of samples is ", samples.shape[-1], " while dimension of gaussians is ",
                             self.means.shape[-1])
        if self.means.shape[-1] != 3:
            raise ValueError(f"GaussianMixture.pdf: the kernel is written for 3-dimensional Gaussians, got {self.means.shape[-1]}")
        return gaussian_mixture_pdf(samples, self.means, self._std)


# ------------------------------------------------------------------------------------------------
# The SMPL body model: linear blend skinning (csrc/smpl_lbs.hip; body_model.SmplBodyModel is the module on top)
# ------------------------------------------------------------------------------------------------
_SMPL_ARRAYS = ("v_template", "blend", "J_template", "J_dirs", "weights")


def _smpl_record(mb):
    """(struct snerf_smpl_model, what keeps its pointers alive, V, J, NB) of a mapping with the arrays of include/smplnerf.h:
    v_template [V,3], blend [NB + 9(J-1), 3V], J_template [J,3], J_dirs [J,3,NB], weights [V,J] (fp32, on the GPU, contiguous) and
    parents (J ints on the host)."""
    import ctypes
    arrs = [mb[k] for k in _SMPL_ARRAYS]
    for k, t in zip(_SMPL_ARRAYS, arrs):
        _need_cuda(k, t)
        if not t.is_contiguous():
            raise RuntimeError(f"smpl_lbs: `{k}` must be contiguous")
    V, J, NB = arrs[0].shape[0], arrs[4].shape[1], arrs[3].shape[2]
    K = NB + 9 * (J - 1)
    want = {"v_template": (V, 3), "blend": (K, 3 * V), "J_template": (J, 3), "J_dirs": (J, 3, NB), "weights": (V, J)}
    for k, t in zip(_SMPL_ARRAYS, arrs):
        if tuple(t.shape) != want[k]:
            raise RuntimeError(f"smpl_lbs: `{k}` has shape {tuple(t.shape)}, expected {want[k]} (V={V}, J={J}, NB={NB})")
    parents = [int(p) for p in mb["parents"]]
    if len(parents) != J:
        raise RuntimeError(f"smpl_lbs: {len(parents)} parents for {J} joints")
    host = (ctypes.c_int32 * J)(*parents)
    rec = _lib.SmplModel(V, J, NB, *(ptr(t) for t in arrs), host)
    return rec, (arrs, host), V, J, NB


def _smpl_fwd(mb, betas, body_pose, global_orient):
    import ctypes
    rec, keep, V, J, NB = _smpl_record(mb)
    B, dev = body_pose.shape[0], body_pose.device
    vertices = torch.empty((B, V, 3), device=dev, dtype=torch.float32)
    joints = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    rig = torch.empty((B, 12 * J + NB + 9 * (J - 1)), device=dev, dtype=torch.float32)
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"smpl_lbs_fwd[V={V}]"):
        check(lib.snerf_smpl_lbs_fwd_f32(ctypes.byref(rec), ptr(betas), betas.shape[0], ptr(body_pose), ptr(global_orient), B,
                                         ptr(vertices), ptr(joints), ptr(rig), current_stream()), "snerf_smpl_lbs_fwd_f32")
    return vertices, joints, rig


class _SmplLbsFn(torch.autograd.Function):
    """snerf_smpl_lbs_fwd_f32 / snerf_smpl_lbs_bwd_f32 under autograd.  What is kept for the backward is the inputs and the
    per-pose rig record [B, 12 J + K]; nothing of size B V."""

    @staticmethod
    def forward(ctx, mb, betas, body_pose, global_orient):
        vertices, joints, rig = _smpl_fwd(mb, betas, body_pose, global_orient)
        ctx.mb = mb
        ctx.has_orient = global_orient is not None
        ctx.save_for_backward(betas, body_pose, rig, *([global_orient] if ctx.has_orient else []))
        ctx.set_materialize_grads(False)
        return vertices, joints

    @staticmethod
    def backward(ctx, d_vertices, d_joints):
        import ctypes
        if d_vertices is None and d_joints is None:
            return None, None, None, None
        betas, body_pose, rig = ctx.saved_tensors[:3]
        global_orient = ctx.saved_tensors[3] if ctx.has_orient else None
        d_vertices, d_joints = (None if g is None else g.contiguous().float() for g in (d_vertices, d_joints))
        rec, keep, V, J, NB = _smpl_record(ctx.mb)
        B, dev = body_pose.shape[0], body_pose.device
        need = ctx.needs_input_grad
        d_betas = torch.empty_like(betas) if need[1] else None
        d_pose = torch.empty_like(body_pose) if need[2] else None
        d_orient = torch.empty_like(global_orient) if ctx.has_orient and need[3] else None
        if B == 0:
            return None, None if d_betas is None else torch.zeros_like(betas), d_pose, d_orient
        lib = _lib.load()
        nbytes = lib.snerf_smpl_lbs_bwd_workspace_bytes(ctypes.byref(rec), B)
        if nbytes < 0:
            check(-1, "snerf_smpl_lbs_bwd_workspace_bytes")
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev), _lib.timed(f"smpl_lbs_bwd[V={V}]"):
            check(lib.snerf_smpl_lbs_bwd_f32(ctypes.byref(rec), ptr(betas), betas.shape[0], ptr(body_pose), ptr(global_orient),
                                             ptr(rig), ptr(d_vertices), ptr(d_joints), B, ptr(ws), nbytes, ptr(d_betas), ptr(d_pose),
                                             ptr(d_orient), current_stream()), "snerf_smpl_lbs_bwd_f32")
        return None, d_betas, d_pose, d_orient


def smpl_lbs(model_buffers, betas, body_pose, global_orient=None):
    """SMPL linear blend skinning in two launches (include/smplnerf.h lists the ten steps): (vertices [B,V,3], joints [B,J,3]).
    model_buffers: a mapping with the arrays of struct snerf_smpl_model - v_template, blend, J_template, J_dirs, weights as fp32 GPU
    tensors and parents as J host ints (SmplBodyModel.kernel_buffers()).  betas [1 or B, NB], body_pose [B, 3(J-1)],
    global_orient [B,3] or None (= zeros).  Differentiable with respect to betas, body_pose and global_orient; the model arrays
    are constants.  No [B,V,4,4] transform tensor and no [B,V,3] temporary exists, forward or backward."""
    for nm, t in (("betas", betas), ("body_pose", body_pose)) + ((("global_orient", global_orient),) if global_orient is not None else ()):
        _need_cuda(nm, t)
    J, NB = model_buffers["weights"].shape[1], model_buffers["J_dirs"].shape[2]
    if body_pose.dim() != 2 or body_pose.shape[1] != 3 * (J - 1):
        raise RuntimeError(f"smpl_lbs: body_pose must be [B, {3 * (J - 1)}], got {tuple(body_pose.shape)}")
    B = body_pose.shape[0]
    if betas.dim() != 2 or betas.shape[1] != NB or betas.shape[0] not in (1, B):
        raise RuntimeError(f"smpl_lbs: betas must be [1 or {B}, {NB}], got {tuple(betas.shape)}")
    if global_orient is not None and tuple(global_orient.shape) != (B, 3):
        raise RuntimeError(f"smpl_lbs: global_orient must be [{B}, 3], got {tuple(global_orient.shape)}")
    if betas.shape[0] == B and B > 1 and betas.stride(0) == 0:
        betas = betas[:1]          # one row shared by the batch (estimator.betas.expand(B, -1)): read as such, d_betas summed by the kernel
    b, p = betas.contiguous(), body_pose.contiguous()
    g = None if global_orient is None else global_orient.contiguous()
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (b, p, g)):
        return _SmplLbsFn.apply(model_buffers, b, p, g)
    return _smpl_fwd(model_buffers, b, p, g)[:2]


# ------------------------------------------------------------------------------------------------
# The vertex_sphere model (datasets/vertex_sphere_dataset.py:84-160): ray-mesh hits and the sphere warp
# ------------------------------------------------------------------------------------------------
def _ray_mesh_inputs(op, origins, directions, vertices, faces, faces_checked):
    """The checks of both ray-mesh operators, in one order -> (o, d, vertices, faces) detached and contiguous."""
    # the table's own checks come first and need no device: a bad table is refused wherever it lives
    if faces.dtype != torch.int32:
        raise RuntimeError(f"{op}: `faces` must be int32 (got {faces.dtype})")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise RuntimeError(f"{op}: vertices {tuple(vertices.shape)} must be [V >= 1, 3] and faces {tuple(faces.shape)} [F >= 1, 3]")
    V = vertices.shape[0]
    if not faces_checked:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        if lo < 0 or hi >= V:
            raise RuntimeError(f"{op}: faces index vertices {lo} .. {hi}, outside [0, {V})")
    for nm, t in (("origins", origins), ("directions", directions), ("vertices", vertices)):
        _need_cuda(nm, t)
    if not faces.is_cuda:
        raise RuntimeError(f"smpl_nerf_amd: `faces` must live on the GPU (got {faces.device}); there is no CPU path")
    if origins.dim() != 2 or origins.shape[1] != 3 or directions.shape != origins.shape:
        raise RuntimeError(f"{op}: origins {tuple(origins.shape)} and directions {tuple(directions.shape)} must both be [R, 3]")
    return tuple(t.detach().contiguous() for t in (origins, directions, vertices, faces))


def _ray_mesh_workspace(lib, F, dev):
    nbytes = lib.snerf_ray_mesh_workspace_bytes(F)
    if nbytes < 0:
        check(-1, "snerf_ray_mesh_workspace_bytes")
    return torch.empty((nbytes,), device=dev, dtype=torch.uint8), nbytes


def ray_mesh_hits(origins, directions, vertices, faces, max_hits: int = 1, faces_checked: bool = False):
    """All hits of R rays on one triangle mesh (csrc/ray_mesh.hip; include/smplnerf.h states the rule: two-sided Moeller-Trumbore in
    fp32): what the reference asks trimesh's RayMeshIntersector for one ray at a time (:85-89).  origins, directions [R,3] fp32,
    vertices [V,3] fp32, faces [F,3] int32 -> (t_hits [R,K] fp32: the K = max_hits (1 .. 16) smallest hit parameters in ascending
    order, padded with +inf, in units of |direction|; n_hits [R] int32: the number of hits, which may exceed K).  The face table
    is range-checked against V before anything is launched (one device reduction and a host read); faces_checked=True skips
    that for a table that has been through it.  The workspace (36 F bytes) is allocated here.  Nothing of size R F is built."""
    o, d, vt, fc = _ray_mesh_inputs("ray_mesh_hits", origins, directions, vertices, faces, faces_checked)
    R, V, F, dev = o.shape[0], vt.shape[0], fc.shape[0], o.device
    K = int(max_hits)
    if not 1 <= K <= 16:
        raise RuntimeError(f"ray_mesh_hits: max_hits must be 1 .. 16, got {max_hits}")
    t_hits = torch.empty((R, K), device=dev, dtype=torch.float32)
    n_hits = torch.empty((R,), device=dev, dtype=torch.int32)
    lib = _lib.load()
    ws, nbytes = _ray_mesh_workspace(lib, F, dev)
    with torch.cuda.device(dev), _lib.timed(f"ray_mesh_hits[F={F},K={K}]"):
        check(lib.snerf_ray_mesh_hits_f32(ptr(o), ptr(d), ptr(vt), ptr(fc), R, V, F, K, ptr(t_hits), ptr(n_hits), ptr(ws), nbytes,
                                          current_stream()), "snerf_ray_mesh_hits_f32")
    return t_hits, n_hits


def ray_mesh_first_hit(origins, directions, vertices, faces, canon=None, faces_checked: bool = False):
    """The first hit of R rays on one triangle mesh, with its face and where on it (csrc/ray_mesh.hip, the rule and the walk of
    ray_mesh_hits; include/smplnerf.h, snerf_ray_mesh_first_hit_f32): render.py:222-319's get_warp without its two Python loops
    over the rays.  Inputs and checks as ray_mesh_hits -> (t [R] fp32: the smallest hit parameter, +inf on a miss; face [R] int32:
    the face hit, -1 on a miss, the smaller index where two faces are hit at equal t; uv [R,2] fp32: u and v of the hit - the
    point is (1 - u - v) a + u b + v c - zero on a miss).  With canon [V,3], the same mesh in the canonical pose, also
    (warp [R,3]: the same surface point of canon minus the hit point; depth [R]: t |direction|), both zero on a miss.  The outputs
    are data: no grad_fn, whatever the inputs require.  Nothing of size R F is built."""
    if canon is not None and canon.shape != vertices.shape:
        raise RuntimeError(f"ray_mesh_first_hit: canon {tuple(canon.shape)} must have the shape of vertices {tuple(vertices.shape)}")
    o, d, vt, fc = _ray_mesh_inputs("ray_mesh_first_hit", origins, directions, vertices, faces, faces_checked)
    R, V, F, dev = o.shape[0], vt.shape[0], fc.shape[0], o.device
    cn = None
    if canon is not None:
        _need_cuda("canon", canon)
        cn = canon.detach().contiguous()
    t = torch.empty((R,), device=dev, dtype=torch.float32)
    face = torch.empty((R,), device=dev, dtype=torch.int32)
    uv = torch.empty((R, 2), device=dev, dtype=torch.float32)
    warp, depth = (torch.empty((R, 3), device=dev, dtype=torch.float32), torch.empty((R,), device=dev, dtype=torch.float32)) if cn is not None else (None, None)
    lib = _lib.load()
    ws, nbytes = _ray_mesh_workspace(lib, F, dev)
    with torch.cuda.device(dev), _lib.timed(f"ray_mesh_first_hit[F={F}]"):
        check(lib.snerf_ray_mesh_first_hit_f32(ptr(o), ptr(d), ptr(vt), ptr(fc), R, V, F, ptr(cn), ptr(t), ptr(face), ptr(uv), ptr(warp),
                                               ptr(depth), ptr(ws), nbytes, current_stream()), "snerf_ray_mesh_first_hit_f32")
    return (t, face, uv) if cn is None else (t, face, uv, warp, depth)


MeshFrames = collections.namedtuple("MeshFrames", "image t face bary depth warp")
_VERTEX_FACES = {}      # (data_ptr, device, F, V, tensor version, with corners) -> (weak reference to the face tensor, vf_offsets, vf_faces[, vf_corners])


def vertex_face_table(faces, V: int):
    """The CSR table of a face table [F,3] (any integer dtype, host or device): (vf_offsets [V+1], vf_faces [3F]) int32 numpy
    arrays - vertex v owns vf_faces[vf_offsets[v]:vf_offsets[v+1]], its incident faces in ascending face index (a face that names
    a vertex twice is listed twice)."""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).astype(np.int64).reshape(-1, 3)
    flat = f.reshape(-1)
    order = np.argsort(flat, kind="stable")                       # stable: within a vertex the corners stay in face order
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), (order // 3).astype(np.int32)


def vertex_corner_table(faces, V: int):
    """vertex_face_table with, for every entry, which corner of its face it is: (vf_offsets [V+1], vf_faces [3F], vf_corners [3F])
    int32 numpy arrays - vertex v is corner vf_corners[k] of face vf_faces[k] for k in vf_offsets[v]:vf_offsets[v+1], in ascending
    face index and, within a face that names the vertex twice, ascending corner: two distinct corners."""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).astype(np.int64).reshape(-1, 3)
    flat = f.reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), (order // 3).astype(np.int32), (order % 3).astype(np.int32)


def _vertex_faces_cached(faces, V, corners: bool = False):
    key = (faces.data_ptr(), faces.device, faces.shape[0], V, faces._version, corners)
    hit = _VERTEX_FACES.get(key)
    if hit is not None and hit[0]() is faces:
        return hit[1:]
    for k in [k for k, v in _VERTEX_FACES.items() if v[0]() is None]:
        del _VERTEX_FACES[k]
    table = tuple(torch.from_numpy(a).to(faces.device) for a in (vertex_corner_table if corners else vertex_face_table)(faces, V))
    _VERTEX_FACES[key] = (weakref.ref(faces),) + table
    return table


def _mesh_frames_inputs(op, poses, vertices, faces, faces_checked):
    """The checks render_mesh and soft_silhouette share on poses, vertices and faces -> (vertices [Nv,V,3], N, Nv, V, F)."""
    if faces.dtype != torch.int32:
        raise RuntimeError(f"{op}: `faces` must be int32 (got {faces.dtype})")
    if vertices.dim() == 2:
        vertices = vertices[None]
    if vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[1] < 1 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise RuntimeError(f"{op}: vertices {tuple(vertices.shape)} must be [V >= 1, 3] or [N, V, 3] and faces {tuple(faces.shape)} [F >= 1, 3]")
    Nv, V, F = vertices.shape[0], vertices.shape[1], faces.shape[0]
    if not faces_checked:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        if lo < 0 or hi >= V:
            raise RuntimeError(f"{op}: faces index vertices {lo} .. {hi}, outside [0, {V})")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.dtype != torch.float64:
        raise RuntimeError(f"{op}: poses must be float64 [N,4,4], got {poses.dtype} {tuple(poses.shape)}")
    N = poses.shape[0]
    if Nv not in (1, N):
        raise RuntimeError(f"{op}: {Nv} bodies for {N} frames (one for all, or one per frame)")
    return vertices, N, Nv, V, F


def _mesh_frames_device(op, H, W, focal, tensors):
    """... and on the frame size and on where the named tensors live (poses and faces keep their own dtypes)."""
    if int(H) < 1 or int(W) < 1 or not float(focal) > 0:
        raise RuntimeError(f"{op}: H and W must be at least 1 and focal positive")
    for nm, t in tensors:
        if t is not None:
            if not t.is_cuda:
                raise RuntimeError(f"smpl_nerf_amd: `{nm}` must live on the GPU (got {t.device}); there is no CPU path")
            if nm not in ("poses", "faces") and t.dtype != torch.float32:
                raise RuntimeError(f"{op}: `{nm}` must be float32 (got {t.dtype})")


@torch.no_grad()
def render_mesh(poses, focal, H: int, W: int, vertices, faces, uv, texture, ambient: float = 0., intensity: float = 1.,
                background=(1., 1., 1.), canon=None, cull: bool = True, faces_checked: bool = False):
    """N textured, lit frames of a triangle mesh in one call (csrc/mesh_render.hip; include/smplnerf.h, snerf_mesh_render_f32, states
    the rule operation by operation): what create_dataset.py asks pyrender for frame by frame.  poses [N,4,4] float64 camera-to-world
    and focal as RayGenerator holds them; vertices [V,3] (one body for all frames) or [N,V,3] (one per frame) fp32; faces [F,3]
    int32; uv [V,2] fp32, one texture coordinate per vertex; texture [Ht,Wt,3] fp32 in [0,1]; optionally canon [V,3] ->
    MeshFrames(image [N,H,W,3] fp32 - Lambert shade min(1, ambient + intensity max(0, n . l)) times the bilinear texel, `background`
    on a miss -, t [N,H,W] (+inf on a miss; the z-depth: the rays have camera-space z = -1), face [N,H,W] int32 (-1), bary [N,H,W,2]
    (0) and, with canon, depth [N,H,W] and warp [N,H,W,3] (0), else None).  t, face, bary, depth and warp are, bit for bit, what
    ray_mesh_first_hit returns for the rays RayGenerator makes for these poses.  cull=False walks every face for every pixel tile:
    the same bits, slower.  The face table is range-checked once (faces_checked=True skips it) and its vertex-to-face table is
    built on the host once per faces tensor and cached.  The frames are data: no backward, no grad_fn."""
    vertices, N, Nv, V, F = _mesh_frames_inputs("render_mesh", poses, vertices, faces, faces_checked)
    if tuple(uv.shape) != (V, 2) or texture.dim() != 3 or texture.shape[2] != 3 or texture.shape[0] < 1 or texture.shape[1] < 1:
        raise RuntimeError(f"render_mesh: uv {tuple(uv.shape)} must be [V,2] and texture {tuple(texture.shape)} [Ht,Wt,3]")
    if canon is not None and tuple(canon.shape) != (V, 3):
        raise RuntimeError(f"render_mesh: canon {tuple(canon.shape)} must be [V,3] = [{V},3]")
    _mesh_frames_device("render_mesh", H, W, focal, (("poses", poses), ("vertices", vertices), ("faces", faces), ("uv", uv),
                                                     ("texture", texture), ("canon", canon)))
    off, vf = _vertex_faces_cached(faces, V)
    ps, vt, fc, uvc, tex = (x.detach().contiguous() for x in (poses, vertices, faces, uv, texture))
    cn = None if canon is None else canon.detach().contiguous()
    dev, H, W = ps.device, int(H), int(W)
    image = torch.empty((N, H, W, 3), device=dev, dtype=torch.float32)
    t = torch.empty((N, H, W), device=dev, dtype=torch.float32)
    face = torch.empty((N, H, W), device=dev, dtype=torch.int32)
    bary = torch.empty((N, H, W, 2), device=dev, dtype=torch.float32)
    depth, warp = (torch.empty((N, H, W), device=dev, dtype=torch.float32), torch.empty((N, H, W, 3), device=dev, dtype=torch.float32)) if cn is not None else (None, None)
    lib = _lib.load()
    nbytes = lib.snerf_mesh_render_workspace_bytes(N, V, F)
    if nbytes < 0:
        check(-1, "snerf_mesh_render_workspace_bytes")
    ws = torch.empty((max(nbytes, 1),), device=dev, dtype=torch.uint8)
    args = _lib.MeshRenderArgs(float(ambient), float(intensity), (ctypes.c_float * 3)(*(float(b) for b in background)),
                               0 if cull else _lib.RENDER_NO_CULL)
    with torch.cuda.device(dev), _lib.timed(f"mesh_render[N={N},F={F}]"):
        check(lib.snerf_mesh_render_f32(ptr(ps), float(focal), N, H, W, ptr(vt), Nv, V, ptr(fc), F, ptr(off), ptr(vf), ptr(uvc), ptr(tex),
                                        tex.shape[0], tex.shape[1], ctypes.byref(args), ptr(cn), ptr(image), ptr(t), ptr(face), ptr(bary),
                                        ptr(depth), ptr(warp), ptr(ws), nbytes, current_stream()), "snerf_mesh_render_f32")
    return MeshFrames(image, t, face, bary, depth, warp)


def _soft_silhouette_workspace(lib, N, V, F, dev):
    nbytes = lib.snerf_soft_silhouette_workspace_bytes(N, V, F)
    if nbytes < 0:
        check(-1, "snerf_soft_silhouette_workspace_bytes")
    return torch.empty((max(nbytes, 8) // 8,), device=dev, dtype=torch.float64), nbytes


class _SoftSilhouette(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, poses, faces, table, focal, H, W, sigma, cutoff, flags):
        N, (Nv, V, _), F, dev = poses.shape[0], vertices.shape, faces.shape[0], poses.device
        vt = vertices.detach().contiguous()
        sil = torch.empty((N, H, W), device=dev, dtype=torch.float32)
        trans = torch.empty((N, H, W), device=dev, dtype=torch.float64)
        lib = _lib.load()
        ws, nbytes = _soft_silhouette_workspace(lib, N, V, F, dev)
        with torch.cuda.device(dev), _lib.timed(f"soft_silhouette_fwd[N={N},F={F}]"):
            check(lib.snerf_soft_silhouette_fwd_f32(ptr(poses), focal, N, H, W, ptr(vt), Nv, V, ptr(faces), F, sigma, cutoff, flags, ptr(sil),
                                                    ptr(trans), ptr(ws), nbytes, current_stream()), "snerf_soft_silhouette_fwd_f32")
        if ctx.needs_input_grad[0]:      # (under no_grad nothing is kept)
            ctx.save_for_backward(vt, poses, faces, trans)
            ctx.table, ctx.scalars = table, (focal, H, W, sigma, cutoff, flags)
        return sil

    @staticmethod
    def backward(ctx, d_sil):
        vt, poses, faces, trans = ctx.saved_tensors
        focal, H, W, sigma, cutoff, flags = ctx.scalars
        N, (Nv, V, _), F, dev = poses.shape[0], vt.shape, faces.shape[0], poses.device
        ds = d_sil.detach().to(torch.float32).contiguous()
        off, vf, vc = ctx.table
        dv = torch.empty_like(vt)
        lib = _lib.load()
        ws, nbytes = _soft_silhouette_workspace(lib, N, V, F, dev)
        with torch.cuda.device(dev), _lib.timed(f"soft_silhouette_bwd[N={N},F={F}]"):
            check(lib.snerf_soft_silhouette_bwd_f32(ptr(poses), focal, N, H, W, ptr(vt), Nv, V, ptr(faces), F, sigma, cutoff, flags, ptr(ds),
                                                    ptr(trans), ptr(off), ptr(vf), ptr(vc), ptr(dv), ptr(ws), nbytes, current_stream()),
                  "snerf_soft_silhouette_bwd_f32")
        return (dv,) + (None,) * 9


def soft_silhouette(poses, focal, H: int, W: int, vertices, faces, sigma: float = 1.0, cutoff: float = 17.0, cull: bool = True,
                    faces_checked: bool = False):
    """The soft silhouette of a triangle mesh in N frames, differentiable with respect to the vertices (csrc/soft_silhouette.hip;
    include/smplnerf.h, snerf_soft_silhouette_fwd_f32, states the rule operation by operation): per pixel
    1 - prod_f (1 - sigmoid(+-d^2 / sigma)) with d the pixel's distance, in pixels, to the projected face's outline and + inside it.
    poses, focal, H, W, vertices ([V,3]: one body for all frames - several cameras on it are a multi-view fit - or [N,V,3]) and
    faces as render_mesh takes them, with its checks; sigma in pixel^2; a face farther than sqrt(cutoff sigma) pixels from a pixel
    contributes exactly 0 to it -> silhouette [N,H,W] fp32 in [0,1].  The gradient reaches `vertices` only (not the camera), in the
    shape it came in.  cull=False walks every face for every pixel tile: the same bits, slower.  Nothing of size pixels x faces is
    built; under no_grad nothing is kept.  The vertex-to-corner table of `faces` is built on the host once per faces tensor, by the first
    call that needs a gradient, and cached."""
    vt, N, Nv, V, F = _mesh_frames_inputs("soft_silhouette", poses, vertices, faces, faces_checked)
    _mesh_frames_device("soft_silhouette", H, W, focal, (("poses", poses), ("vertices", vt), ("faces", faces)))
    if not (float(sigma) > 0 and math.isfinite(float(sigma)) and 0 <= float(cutoff) < math.inf):
        raise RuntimeError(f"soft_silhouette: sigma must be positive and finite and cutoff finite and not negative, got {sigma} and {cutoff}")
    # (the corner table hangs on the caller's faces tensor, as render_mesh's table does: built on the host once, then cached)
    table = _vertex_faces_cached(faces, V, corners=True) if torch.is_grad_enabled() and vertices.requires_grad else None
    return _SoftSilhouette.apply(vt, poses.detach().contiguous(), faces.detach().contiguous(), table, float(focal), int(H), int(W),
                                 float(sigma), float(cutoff), 0 if cull else _lib.RENDER_NO_CULL)


def vertex_sphere_warp(samples, goal, canon, radius, by_mean: bool = False, want_indices: bool = False):
    """The deterministic warp of the vertex_sphere model (csrc/vertex_sphere.hip; :128-159) in one launch.  samples [..., 3], goal /
    canon [V,3] (one body in the goal and in the canonical pose) -> warp, shaped like samples: canon_i - goal_i of the nearest goal
    vertex i where it is closer than `radius`, else zero (by_mean=False), or the mean of canon_v - goal_v over the goal vertices
    inside the radius (by_mean=True; the reference's 1e-10 in the denominator).  A distance equal to the radius weighs as itself
    (quirk Q12).  want_indices=True: (warp, nearest [...] int32, count [...] int32) with the argmin vertex and the number of
    vertices inside the radius (by_mean=False: whether the nearest is).  The outputs are data: no grad_fn, whatever the inputs
    require.  No [n, V] tensor is built."""
    for nm, t in (("samples", samples), ("goal", goal), ("canon", canon)):
        _need_cuda(nm, t)
    if samples.dim() < 1 or samples.shape[-1] != 3:
        raise RuntimeError(f"vertex_sphere_warp: samples must be [..., 3], got {tuple(samples.shape)}")
    if goal.dim() != 2 or goal.shape[1] != 3 or goal.shape[0] < 1 or canon.shape != goal.shape:
        raise RuntimeError(f"vertex_sphere_warp: goal {tuple(goal.shape)} and canon {tuple(canon.shape)} must both be [V >= 1, 3]")
    x, g, c = (t.detach().contiguous() for t in (samples, goal, canon))
    n, V, dev = x.numel() // 3, g.shape[0], x.device
    warp = torch.empty(samples.shape, device=dev, dtype=torch.float32)
    nearest, count = ((torch.empty(samples.shape[:-1], device=dev, dtype=torch.int32) for _ in range(2)) if want_indices else (None, None))
    lib = _lib.load()
    with torch.cuda.device(dev), _lib.timed(f"vertex_sphere_warp[V={V}]"):
        check(lib.snerf_vertex_sphere_warp_f32(ptr(x), ptr(g), ptr(c), n, V, float(radius), 1 if by_mean else 0, ptr(warp), ptr(nearest),
                                               ptr(count), current_stream()), "snerf_vertex_sphere_warp_f32")
    return (warp, nearest, count) if want_indices else warp


# ------------------------------------------------------------------------------------------------
# Image scores (util/scores.py): SSIM with its backward, MSE and PSNR (csrc/ssim.hip)
# ------------------------------------------------------------------------------------------------
def _ssim_tile_constants():
    """The `constexpr int NAME = value;` lines of csrc/ssim_tiles.h: the kernels' tile extents, for the tests' shapes."""
    import os
    import re
    with open(os.path.join(_lib.HERE, "csrc", "ssim_tiles.h")) as f:
        return {k: int(v) for k, v in re.findall(r"constexpr int (SSIM_[A-Z_]+) = (\d+);", f.read())}


SSIM_TILES = _ssim_tile_constants()
_SSIM_WINDOWS = {}


def ssim_window(kernel_size: int, kernel_sigma: float):
    """The 1-D Gaussian window win[k] (numpy fp32) whose outer product is the reference's gaussian_filter (scores.py:71-86):
    exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) in float64, normalised to sum 1, rounded to fp32 once."""
    import numpy as np
    i = np.arange(int(kernel_size), dtype=np.float64) - (int(kernel_size) - 1) / 2.
    g = np.exp(-(i ** 2) / (2. * float(kernel_sigma) ** 2))
    return (g / g.sum()).astype(np.float32)


def _ssim_window_on(kernel_size, kernel_sigma, dev):
    key = (int(kernel_size), float(kernel_sigma), str(dev))
    if key not in _SSIM_WINDOWS:
        _SSIM_WINDOWS[key] = torch.from_numpy(ssim_window(kernel_size, kernel_sigma)).to(dev)
    return _SSIM_WINDOWS[key]


def _ssim_call(entry, x, y, win, c1, c2, *outputs):
    """One of the two entries on x, y [N,C,H,W] of EQUAL strides (what _ssim_layout hands out), with its workspace."""
    N, C, H, W = x.shape
    k, dev = win.numel(), x.device
    lib = _lib.load()
    nbytes = lib.snerf_ssim_workspace_bytes(N, C, H, W, k)
    if nbytes < 0:
        check(-1, "snerf_ssim_workspace_bytes")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev), _lib.timed(f"{entry}[{H}x{W},k={k}]"):
        check(getattr(lib, f"snerf_{entry}_f32")(ptr(x), ptr(y), N, C, H, W, *x.stride(), ptr(win), k, c1, c2, *(ptr(t) for t in outputs),
                                                 ptr(ws), nbytes, current_stream()), f"snerf_{entry}_f32")


def _ssim_fwd(x, y, win, c1, c2, want_cs, want_sqerr):
    N, C = x.shape[:2]
    ssim, cs, sqerr = (torch.empty((N, C), device=x.device, dtype=torch.float32) if want else None for want in (True, want_cs, want_sqerr))
    _ssim_call("ssim_fwd", x, y, win, c1, c2, ssim, cs, sqerr)
    return ssim, cs, sqerr


def _ssim_bwd(x, y, win, c1, c2, g_ssim, g_cs):
    dx = torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32)
    _ssim_call("ssim_bwd", x, y, win, c1, c2, g_ssim, g_cs, dx)
    return dx


class _SsimFn(torch.autograd.Function):
    """snerf_ssim_fwd_f32 / snerf_ssim_bwd_f32 under autograd: per-channel ssim and cs [N,C].  The inputs are kept, nothing of map
    size is; the backward recomputes the window statistics, one launch per input that wants a gradient (the gradient to y is the
    same entry with the images swapped)."""

    @staticmethod
    def forward(ctx, x, y, win, c1, c2):
        ssim, cs, _ = _ssim_fwd(x, y, win, c1, c2, True, False)
        ctx.save_for_backward(x, y, win)
        ctx.consts = (c1, c2)
        ctx.set_materialize_grads(False)
        return ssim, cs

    @staticmethod
    def backward(ctx, g_ssim, g_cs):
        if g_ssim is None and g_cs is None:
            return None, None, None, None, None
        x, y, win = ctx.saved_tensors
        gs = torch.zeros(x.shape[:2], device=x.device, dtype=torch.float32) if g_ssim is None else g_ssim.contiguous().float()
        gc = None if g_cs is None else g_cs.contiguous().float()
        dx = _ssim_bwd(x, y, win, *ctx.consts, gs, gc) if ctx.needs_input_grad[0] else None
        dy = _ssim_bwd(y, x, win, *ctx.consts, gs, gc) if ctx.needs_input_grad[1] else None
        return dx, dy, None, None, None


def _ssim_layout(x, y):
    """x and y as the entries read them: ONE set of four strides for both, no two elements at one address (dx is written through
    them).  Tensors that already are (channels-first, channels-last, equal slices of both) pass untouched."""
    def plain(t):
        return all(st > 0 or n == 1 for st, n in zip(t.stride(), t.shape))
    if x.stride() == y.stride() and plain(x):
        return x, y
    if plain(x):
        return x, torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=x.dtype).copy_(y)
    return x.contiguous(), y.contiguous()


def _ssim_per_channel(x, y, kernel_size, kernel_sigma, data_range, k1, k2, want_sqerr=False):
    """The checks of ssim() and the launch: (ssim [N,C], cs [N,C], sqerr [N,C] or None)."""
    _need_cuda("x", x)
    _need_cuda("y", y)
    if x.dim() != 4 or x.shape != y.shape:
        raise RuntimeError(f"ssim: x and y must be 4-D [N,C,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise RuntimeError(f"ssim: x on {x.device}, y on {y.device}")
    k = int(kernel_size)
    if x.size(-1) < k or x.size(-2) < k:      # scores.py:148-150
        raise ValueError(f"Kernel size can't be greater than actual input size. Input size: {x.size()}. Kernel size: {k}")
    if not 1 <= k <= SSIM_TILES["SSIM_MAX_K"]:
        raise RuntimeError(f"ssim: kernel_size must be 1 .. {SSIM_TILES['SSIM_MAX_K']}, got {kernel_size}")
    c1, c2 = float((k1 * data_range) ** 2), float((k2 * data_range) ** 2)      # scores.py:152-153
    win = _ssim_window_on(k, kernel_sigma, x.device)
    x, y = _ssim_layout(x, y)
    if not want_sqerr and torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _SsimFn.apply(x, y, win, c1, c2) + (None,)
    return _ssim_fwd(x.detach(), y.detach(), win, c1, c2, True, want_sqerr)


def ssim(x, y, kernel_size: int = 11, kernel_sigma: float = 1.5, data_range=1., reduction: str = 'mean', full: bool = False,
         k1: float = 0.01, k2: float = 0.03):
    """util/scores.py:88-131 on 4-D fp32 GPU tensors [N,C,H,W] of any strides (channels-last views and slices run without a copy):
    per image the channel mean of the per-channel SSIM, then `reduction` ('none' | 'mean' | 'sum') over the batch; full=True returns
    (ssim, cs).  Two launches forward; differentiable with respect to x and y, one backward launch per input that wants a
    gradient.  ValueError where the reference raises it: a window larger than the image.  The window is the separable
    ssim_window(kernel_size, kernel_sigma); any kernel_size up to SSIM_TILES['SSIM_MAX_K'], even ones included."""
    ssim_nc, cs_nc, _ = _ssim_per_channel(x, y, kernel_size, kernel_sigma, data_range, k1, k2)
    ssim_val, cs = ssim_nc.mean(1), cs_nc.mean(1)
    if reduction != 'none':
        reduction_operation = {'mean': torch.mean, 'sum': torch.sum}
        ssim_val, cs = reduction_operation[reduction](ssim_val, dim=0), reduction_operation[reduction](cs, dim=0)
    return (ssim_val, cs) if full else ssim_val


def image_scores(renders, truths, channels_first: bool = False, lpips=None, **ssim_kwargs):
    """The scores of the reference's print_scores (util/scores.py:457-464) of frames [N,H,W,3] (channels_first=True: [N,3,H,W]);
    mse, psnr and ssim come from ONE forward call of the SSIM kernel: dict of 0-d device tensors
        mse   scores.py:28: the mean of (x - y)^2 over every pixel and channel - the kernel's per-channel sums, added in float64
        psnr  scores.py:47-48: -10 ln(mse) / ln(10)
        ssim  ssim(renders, truths, **ssim_kwargs)
        lpips only with lpips=<a lpips.VggLpips on the frames' device>: ops.lpips(renders, truths, lpips), the batch mean (fp32)
    mse and psnr are float64 tensors (an fp32 ulp of a 30 dB PSNR is 2e-6, more than the error of the sums), ssim is fp32.  The
    images are taken to lie in [0, 1] for psnr, as the reference's img2psnr takes them.  Evaluation only: nothing here is
    differentiated through."""
    import math
    reduction = ssim_kwargs.pop("reduction", "mean")
    if ssim_kwargs.pop("full", False):
        raise ValueError("image_scores: `full` is not an option here; ssim(..., full=True) returns cs")
    if renders.dim() != 4:
        raise RuntimeError(f"image_scores: frames must be 4-D, got {tuple(renders.shape)}")
    x, y = (renders.detach(), truths.detach()) if channels_first else (renders.detach().permute(0, 3, 1, 2), truths.detach().permute(0, 3, 1, 2))
    ssim_nc, _, sqerr = _ssim_per_channel(x, y, ssim_kwargs.pop("kernel_size", 11), ssim_kwargs.pop("kernel_sigma", 1.5),
                                          ssim_kwargs.pop("data_range", 1.), ssim_kwargs.pop("k1", 0.01), ssim_kwargs.pop("k2", 0.03),
                                          want_sqerr=True)
    if ssim_kwargs:
        raise TypeError(f"image_scores: unknown arguments {sorted(ssim_kwargs)}")
    val = ssim_nc.mean(1)
    if reduction != 'none':
        val = {'mean': torch.mean, 'sum': torch.sum}[reduction](val, dim=0)
    mse = sqerr.double().sum() / x.numel()
    scores = {"mse": mse, "psnr": -10. * torch.log(mse) / math.log(10.), "ssim": val}
    if lpips is not None:
        scores["lpips"] = _lpips_op(x, y, lpips)      # (ops.lpips: the argument shadows its name here)
    return scores


# ------------------------------------------------------------------------------------------------
# SmplEstimator's convolution block (csrc/conv_block.hip); the network itself: estimator.py
# ------------------------------------------------------------------------------------------------
def conv3x3_block(x, weight, scale, shift, relu: bool = True, pool: bool = False):
    """y = [maxpool2x2](relu(scale[co] * conv3x3_pad1(x, weight)[co] + shift[co])) in one launch: x [N,Ci,H,W], weight [Co,Ci,3,3],
    scale, shift [Co] (an eval-mode BatchNorm2d and the convolution's bias folded: estimator.fold_bn) -> [N,Co,H,W], or
    [N,Co,H//2,W//2] with pool (odd extents floor as nn.MaxPool2d(2, 2)).  fp32 GPU tensors, made contiguous.  Forward only: while
    grad mode is enabled an input that requires grad is refused (no graph could be recorded through this op); under torch.no_grad()
    such a tensor passes, so a module hands its Parameters over as they are."""
    for nm, t in (("x", x), ("weight", weight), ("scale", scale), ("shift", shift)):
        _need_cuda(nm, t)
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"conv3x3_block: `{nm}` requires grad, but this op is inference only: the training kernels of the "
                               "convolution block (batch statistics, weight gradient, pool / ReLU / BatchNorm backward) are "
                               "ops.conv3x3_bn_block")
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        raise RuntimeError(f"conv3x3_block: x must be [N,Ci,H,W] and weight [Co,Ci,3,3], got {tuple(x.shape)} and {tuple(weight.shape)}")
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    if tuple(scale.shape) != (Co,) or tuple(shift.shape) != (Co,):
        raise RuntimeError(f"conv3x3_block: scale and shift must be [{Co}], got {tuple(scale.shape)} and {tuple(shift.shape)}")
    x, weight, scale, shift = (t.detach().contiguous() for t in (x, weight, scale, shift))
    y = torch.empty((N, Co, H // 2, W // 2) if pool else (N, Co, H, W), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _lib.timed(f"conv3x3_block[{Ci}->{Co},{H}x{W}]"):
        check(_lib.load().snerf_conv3x3_block_f32(ptr(x), N, Ci, H, W, ptr(weight), ptr(scale), ptr(shift), Co, int(bool(relu)),
                                                  int(bool(pool)), ptr(y), current_stream()), "snerf_conv3x3_block_f32")
    return y


# ------------------------------------------------------------------------------------------------
# ... and the block in training mode (csrc/conv_train.hip): batch statistics, and every gradient
# ------------------------------------------------------------------------------------------------
def _scratch(query, what, dev):
    """torch.empty of the floats a *_scratch_floats query asks for (a caching-allocator block: aligned far beyond the 8 bytes asked)."""
    n = int(query)
    if n < 0:
        check(-1, what)
    return torch.empty(max(n, 2), device=dev, dtype=torch.float32)


class _ConvBnBlockFn(torch.autograd.Function):
    """forward(x, weight, bias, bn_weight, bn_bias, running_mean, running_var, momentum, eps, relu, pool) -> (y, and the running
    statistics that were given: marked dirty); saves x, z, mean, invstd (and the three parameters the backward reads)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, momentum, eps, relu, pool):
        lib, dev = _lib.load(), x.device
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        xd, wd, bd, gd, btd = (t.detach().contiguous() for t in (x, weight, bias, gamma, beta))
        z = torch.empty((N, Co, H, W), device=dev, dtype=torch.float32)
        mean, invstd = torch.empty(Co, device=dev, dtype=torch.float32), torch.empty(Co, device=dev, dtype=torch.float32)
        y = torch.empty((N, Co, H // 2, W // 2) if pool else (N, Co, H, W), device=dev, dtype=torch.float32)
        ones = torch.ones(Co, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev), _lib.timed(f"conv3x3_bn_block_fwd[{Ci}->{Co},{H}x{W}]"):
            s = current_stream()
            check(lib.snerf_conv3x3_block_f32(ptr(xd), N, Ci, H, W, ptr(wd), ptr(ones), ptr(bd), Co, 0, 0, ptr(z), s), "snerf_conv3x3_block_f32")
            scratch = _scratch(lib.snerf_bn_stats_scratch_floats(N, Co, H, W), "snerf_bn_stats_scratch_floats", dev)
            check(lib.snerf_bn_stats_f32(ptr(z), N, Co, H, W, eps, momentum, ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd),
                                         ptr(scratch), s), "snerf_bn_stats_f32")
            check(lib.snerf_bn_relu_pool_fwd_f32(ptr(z), N, Co, H, W, ptr(mean), ptr(invstd), ptr(gd), ptr(btd), int(relu), int(pool), ptr(y), s),
                  "snerf_bn_relu_pool_fwd_f32")
        dirty = tuple(t for t in (running_mean, running_var) if t is not None)      # moved in place: autograd wants them returned
        ctx.mark_dirty(*dirty)
        ctx.mark_non_differentiable(*dirty)
        ctx.save_for_backward(xd, wd, gd, btd, z, mean, invstd)
        ctx.relu, ctx.pool = int(relu), int(pool)
        return (y,) + dirty

    @staticmethod
    def backward(ctx, dy, *_):
        xd, wd, gd, btd, z, mean, invstd = ctx.saved_tensors
        need_x, need_w, need_b, need_g, need_bt = ctx.needs_input_grad[:5]
        lib, dev = _lib.load(), dy.device
        N, Ci, H, W = xd.shape
        Co = wd.shape[0]
        dy = dy.contiguous()
        need_dz = need_x or need_w or need_b
        dz = torch.empty_like(z) if need_dz else None
        dg = torch.empty(Co, device=dev, dtype=torch.float32) if need_g else None
        dbt = torch.empty(Co, device=dev, dtype=torch.float32) if need_bt else None
        dx = dw = db = None
        with torch.cuda.device(dev), _lib.timed(f"conv3x3_bn_block_bwd[{Ci}->{Co},{H}x{W}]"):
            s = current_stream()
            if need_dz or need_g or need_bt:
                scratch = _scratch(lib.snerf_bn_relu_pool_bwd_scratch_floats(N, Co, H, W, ctx.pool), "snerf_bn_relu_pool_bwd_scratch_floats", dev)
                check(lib.snerf_bn_relu_pool_bwd_f32(ptr(z), ptr(dy), N, Co, H, W, ptr(mean), ptr(invstd), ptr(gd), ptr(btd), ctx.relu, ctx.pool,
                                                     ptr(dz), ptr(dg), ptr(dbt), ptr(scratch), s), "snerf_bn_relu_pool_bwd_f32")
            if need_w or need_b:
                dw = torch.empty_like(wd) if need_w else None
                db = torch.empty(Co, device=dev, dtype=torch.float32) if need_b else None
                scratch = _scratch(lib.snerf_conv3x3_bwd_weight_scratch_floats(N, Ci, H, W, Co), "snerf_conv3x3_bwd_weight_scratch_floats", dev)
                check(lib.snerf_conv3x3_bwd_weight_f32(ptr(dz), ptr(xd), N, Ci, Co, H, W, ptr(dw), ptr(db), ptr(scratch), s),
                      "snerf_conv3x3_bwd_weight_f32")
            if need_x:
                dx = torch.empty_like(xd)
                scratch = _scratch(lib.snerf_conv3x3_bwd_input_scratch_floats(Ci, Co), "snerf_conv3x3_bwd_input_scratch_floats", dev)
                check(lib.snerf_conv3x3_bwd_input_f32(ptr(dz), N, Co, H, W, ptr(wd), Ci, ptr(dx), ptr(scratch), s), "snerf_conv3x3_bwd_input_f32")
        return dx, dw, db, dg, dbt, None, None, None, None, None, None


def conv3x3_bn_block(x, weight, bias, bn_weight, bn_bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, relu: bool = True,
                     pool: bool = False):
    """The block as nn.Conv2d(3, padding=1) - nn.BatchNorm2d in TRAINING mode - ReLU - nn.MaxPool2d(2, 2) compute it:
    y = [maxpool2x2](relu(BN_batch(conv3x3_pad1(x, weight) + bias))), x [N,Ci,H,W], weight [Co,Ci,3,3], the rest [Co]; N H W >= 2.
    Differentiable to x, weight, bias, bn_weight and bn_bias (only what requires grad is computed); running_mean / running_var, when
    given, are moved in place with `momentum` (a float) as F.batch_norm(training=True) moves them.  fp32 GPU tensors, made contiguous."""
    for nm, t in (("x", x), ("weight", weight), ("bias", bias), ("bn_weight", bn_weight), ("bn_bias", bn_bias)):
        _need_cuda(nm, t)
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        raise RuntimeError(f"conv3x3_bn_block: x must be [N,Ci,H,W] and weight [Co,Ci,3,3], got {tuple(x.shape)} and {tuple(weight.shape)}")
    Co = weight.shape[0]
    for nm, t in (("bias", bias), ("bn_weight", bn_weight), ("bn_bias", bn_bias), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None:
            continue
        if tuple(t.shape) != (Co,):
            raise RuntimeError(f"conv3x3_bn_block: `{nm}` must be [{Co}], got {tuple(t.shape)}")
        if nm.startswith("running"):
            _need_cuda(nm, t)
            if not t.is_contiguous() or t.requires_grad:
                raise RuntimeError(f"conv3x3_bn_block: `{nm}` is updated in place: it must be contiguous and must not require grad")
    if momentum is None:
        raise RuntimeError("conv3x3_bn_block: momentum=None (the cumulative average) is not supported")
    return _ConvBnBlockFn.apply(x, weight, bias, bn_weight, bn_bias, running_mean, running_var, float(momentum), float(eps), bool(relu),
                                bool(pool))[0]


# ------------------------------------------------------------------------------------------------
# LPIPS (util/scores.py:286-456): the convolution with a tap, the tap distance, the metric (csrc/conv_block.hip, csrc/lpips.hip)
# ------------------------------------------------------------------------------------------------
def _forward_only(op, tensors):
    for nm, t in tensors:
        _need_cuda(nm, t)
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{op}: `{nm}` requires grad, but this op is forward only (the score: ops.lpips_loss is LPIPS as a training loss); "
                               "call it under torch.no_grad() or detach the tensor")


def conv3x3_block_tap(x, weight, scale, shift, relu: bool = True, full: bool = True, pool: bool = True):
    """ops.conv3x3_block with both of its outputs from one launch: (y_full [N,Co,H,W] or None, y_pool [N,Co,H//2,W//2] or None), the
    un-pooled map (the LPIPS "tap") and its 2 x 2 max from the same accumulators.  Ci, Co up to 512.  Either output has the bits
    ops.conv3x3_block gives it.  Forward only, as ops.conv3x3_block."""
    _forward_only("conv3x3_block_tap", (("x", x), ("weight", weight), ("scale", scale), ("shift", shift)))
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        raise RuntimeError(f"conv3x3_block_tap: x must be [N,Ci,H,W] and weight [Co,Ci,3,3], got {tuple(x.shape)} and {tuple(weight.shape)}")
    if not (full or pool):
        raise RuntimeError("conv3x3_block_tap: one of `full` and `pool` at least")
    N, Ci, H, W = x.shape
    Co = weight.shape[0]
    if tuple(scale.shape) != (Co,) or tuple(shift.shape) != (Co,):
        raise RuntimeError(f"conv3x3_block_tap: scale and shift must be [{Co}], got {tuple(scale.shape)} and {tuple(shift.shape)}")
    x, weight, scale, shift = (t.detach().contiguous() for t in (x, weight, scale, shift))
    y_full = torch.empty((N, Co, H, W), device=x.device, dtype=torch.float32) if full else None
    y_pool = torch.empty((N, Co, H // 2, W // 2), device=x.device, dtype=torch.float32) if pool else None
    with torch.cuda.device(x.device), _lib.timed(f"conv3x3_block_tap[{Ci}->{Co},{H}x{W}]"):
        check(_lib.load().snerf_conv3x3_block_tap_f32(ptr(x), N, Ci, H, W, ptr(weight), ptr(scale), ptr(shift), Co, int(bool(relu)),
                                                      ptr(y_full), ptr(y_pool), current_stream()), "snerf_conv3x3_block_tap_f32")
    return y_full, y_pool


def feature_distance(fx, fy, weights, normalize: bool = True):
    """out[n] = mean_p sum_c weights[c] (x^[c,p] - y^[c,p])^2 of two feature maps [N,C,h,w], x^ = fx / (sqrt(sum_c fx^2) + 1e-10) with
    `normalize` (ContentLoss.normalize, scores.py:403-411) and fx without: one layer's term of the reference's ContentLoss -> [N].
    The rule is written out in include/smplnerf.h; fx == fy gives 0 exactly.  Forward only."""
    _forward_only("feature_distance", (("fx", fx), ("fy", fy), ("weights", weights)))
    if fx.dim() != 4 or fx.shape != fy.shape or weights.numel() != fx.shape[1]:
        raise RuntimeError(f"feature_distance: fx and fy must be [N,C,h,w] of one shape and weights [C], got {tuple(fx.shape)}, "
                           f"{tuple(fy.shape)} and {tuple(weights.shape)}")
    fx, fy, weights = fx.detach().contiguous(), fy.detach().contiguous(), weights.detach().reshape(-1).contiguous()
    N, C, h, w = fx.shape
    lib = _lib.load()
    nbytes = lib.snerf_feature_distance_workspace_bytes(N, h, w)
    if nbytes < 0:
        check(-1, "snerf_feature_distance_workspace_bytes")
    ws = torch.empty((max(nbytes, 8),), device=fx.device, dtype=torch.uint8)
    out = torch.empty((N,), device=fx.device, dtype=torch.float32)
    with torch.cuda.device(fx.device), _lib.timed(f"feature_distance[{C},{h}x{w}]"):
        check(lib.snerf_feature_distance_f32(ptr(fx), ptr(fy), N, C, h, w, ptr(weights), int(bool(normalize)), ptr(out), ptr(ws), nbytes,
                                             current_stream()), "snerf_feature_distance_f32")
    return out


LPIPS_WORKSPACE_BYTES = 1 << 30      # what ops.lpips allocates at the most (one image pair's need, where that is more)


def lpips_layers(x, y, net, workspace=None, max_pairs: Optional[int] = None):
    """snerf_lpips_fwd_f32 on frames x, y [N,3,H,W] of any strides (one set for both; channels-last views run without a copy):
    (layers [N,5], total [N]).  workspace: a uint8 device tensor to run in (a graph capture hands one over: nothing is allocated
    then but the outputs); else one is allocated for min(N, max_pairs) pairs within LPIPS_WORKSPACE_BYTES.  The bits do not depend
    on it."""
    _forward_only("lpips", (("x", x), ("y", y)))
    if x.dim() != 4 or x.shape != y.shape or x.shape[1] != 3:
        raise RuntimeError(f"lpips: x and y must be [N,3,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise RuntimeError(f"lpips: x on {x.device}, y on {y.device}")
    x, y = _ssim_layout(x.detach(), y.detach())
    N, _, H, W = x.shape
    rec = net.record(x.device)
    lib = _lib.load()
    if workspace is None:
        one = lib.snerf_lpips_workspace_bytes(1, H, W, rec.channels)
        if one < 0:
            check(-1, "snerf_lpips_workspace_bytes")
        pairs = max(1, min(N, LPIPS_WORKSPACE_BYTES // one, max_pairs if max_pairs else N))
        workspace = torch.empty((pairs * one,), device=x.device, dtype=torch.uint8)
    layers = torch.empty((N, 5), device=x.device, dtype=torch.float32)
    total = torch.empty((N,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _lib.timed(f"lpips_fwd[{N}x{H}x{W}]"):
        check(lib.snerf_lpips_fwd_f32(ctypes.byref(rec), ptr(x), ptr(y), N, H, W, *x.stride(), ptr(layers), ptr(total), ptr(workspace),
                                      workspace.numel(), current_stream()), "snerf_lpips_fwd_f32")
    return layers, total


def lpips(x, y, net, reduction: str = 'mean', per_layer: bool = False):
    """The reference's LPIPS()(x, y) (util/scores.py:423-456, ContentLoss.forward :356-379) on the device, with the weights of `net`
    (a lpips.VggLpips): frames [N,3,H,W], fp32 - the sum over the five taps of the weighted distance of the unit-normalised features,
    then `reduction` ('mean' | 'sum' | 'none') over the batch.  per_layer=True: (value, the five taps' terms [N,5], reduced alike).
    H, W >= 16 (the reference, which runs the unused pool5, needs 32).  The inputs are not checked for >= 0 (the reference's assert is
    a device synchronisation).  Forward only: an input that requires grad while grad mode is on is refused (ops.lpips_loss is the
    differentiable form)."""
    if reduction not in ('mean', 'sum', 'none'):
        raise KeyError(reduction)
    layers, total = lpips_layers(x, y, net)
    if reduction != 'none':
        op = {'mean': torch.mean, 'sum': torch.sum}[reduction]
        total, layers = op(total, dim=0), op(layers, dim=0)
    return (total, layers) if per_layer else total


_lpips_op = lpips


# ---- LPIPS as a training loss: the backward (csrc/lpips.hip) -------------------------------------------------------------------------
def feature_distance_bwd(fx, fy, weights, g, normalize: bool = True, want_fx: bool = True, want_fy: bool = True):
    """snerf_feature_distance_bwd_f32: (dfx, dfy), the gradient of sum_n g[n] feature_distance(fx, fy, weights)[n] to the two maps
    [N,C,h,w]; g [N].  An output that is not wanted is None; the other has the bits it has beside it.  At a pixel whose features are
    all zero the norm term is taken as 0 (autograd gives NaN there); the rule is written out in include/smplnerf.h.  A plain
    function: nothing is recorded for autograd."""
    for nm, t in (("fx", fx), ("fy", fy), ("weights", weights), ("g", g)):
        _need_cuda(nm, t)
    if fx.dim() != 4 or fx.shape != fy.shape or weights.numel() != fx.shape[1] or g.numel() != fx.shape[0]:
        raise RuntimeError(f"feature_distance_bwd: fx and fy must be [N,C,h,w] of one shape, weights [C] and g [N], got {tuple(fx.shape)}, "
                           f"{tuple(fy.shape)}, {tuple(weights.shape)} and {tuple(g.shape)}")
    if not (want_fx or want_fy):
        raise RuntimeError("feature_distance_bwd: one of `want_fx` and `want_fy` at least")
    fx, fy, weights, g = (t.detach().float().contiguous() for t in (fx, fy, weights.reshape(-1), g.reshape(-1)))
    N, C, h, w = fx.shape
    dfx, dfy = (torch.empty_like(fx) if want else None for want in (want_fx, want_fy))
    with torch.cuda.device(fx.device), _lib.timed(f"feature_distance_bwd[{C},{h}x{w}]"):
        check(_lib.load().snerf_feature_distance_bwd_f32(ptr(fx), ptr(fy), N, C, h, w, ptr(weights), int(bool(normalize)), ptr(g), ptr(dfx),
                                                         ptr(dfy), current_stream()), "snerf_feature_distance_bwd_f32")
    return dfx, dfy


def relu_pool_bwd(y, dy_full=None, dy_pool=None, inplace: bool = False):
    """snerf_relu_pool_bwd_f32: dz = (y > 0) ? dy_full + route(dy_pool) : 0 on the post-ReLU map y [N,C,H,W]; dy_full [N,C,H,W] and
    dy_pool [N,C,H//2,W//2], one of them at least.  route: a window's gradient goes to its first maximum in the order (0,0), (0,1),
    (1,0), (1,1).  inplace=True writes dz over a contiguous fp32 dy_full and returns it.  A plain function."""
    _need_cuda("y", y)
    if y.dim() != 4:
        raise RuntimeError(f"relu_pool_bwd: y must be [N,C,H,W], got {tuple(y.shape)}")
    if dy_full is None and dy_pool is None:
        raise RuntimeError("relu_pool_bwd: one of `dy_full` and `dy_pool` at least")
    N, C, H, W = y.shape
    for nm, t, shape in (("dy_full", dy_full, (N, C, H, W)), ("dy_pool", dy_pool, (N, C, H // 2, W // 2))):
        if t is not None:
            _need_cuda(nm, t)
            if tuple(t.shape) != shape:
                raise RuntimeError(f"relu_pool_bwd: `{nm}` must be {list(shape)}, got {tuple(t.shape)}")
    y = y.detach().float().contiguous()
    if inplace and (dy_full is None or dy_full.dtype != torch.float32 or not dy_full.is_contiguous()):
        raise RuntimeError("relu_pool_bwd: inplace=True needs a contiguous fp32 dy_full")
    dz = dy_full if inplace else torch.empty_like(y)
    dy_full, dy_pool = (None if t is None else t.detach().float().contiguous() for t in (dy_full, dy_pool))
    with torch.cuda.device(y.device), _lib.timed(f"relu_pool_bwd[{C},{H}x{W}]"):
        check(_lib.load().snerf_relu_pool_bwd_f32(ptr(y), ptr(dy_full), ptr(dy_pool), N, C, H, W, ptr(dz), current_stream()),
              "snerf_relu_pool_bwd_f32")
    return dz


def lpips_bwd(x, y, net, g_layers, want_x: bool = True, want_y: bool = True, want_layers: bool = False, workspace=None,
              max_pairs: Optional[int] = None):
    """snerf_lpips_bwd_f32 on frames x, y [N,3,H,W] of one set of strides (what _ssim_layout hands out): (dx, dy, layers), the
    gradient of sum g_layers[n,l] layers[n,l] to the frames, laid out as they are, None where not wanted.  workspace as
    ops.lpips_layers': a uint8 device tensor to run in, else one for min(N, max_pairs) pairs within LPIPS_WORKSPACE_BYTES (one
    pair's need, where that is more).  The bits do not depend on it.  A plain function."""
    if not (want_x or want_y):
        raise RuntimeError("lpips_bwd: one of `want_x` and `want_y` at least")
    for nm, t in (("x", x), ("y", y), ("g_layers", g_layers)):
        _need_cuda(nm, t)
    if x.dim() != 4 or x.shape != y.shape or x.shape[1] != 3 or x.stride() != y.stride():
        raise RuntimeError(f"lpips_bwd: x and y must be [N,3,H,W] of one shape and one set of strides, got {tuple(x.shape)} / {x.stride()} and "
                           f"{tuple(y.shape)} / {y.stride()}")
    N, _, H, W = x.shape
    if tuple(g_layers.shape) != (N, 5):
        raise RuntimeError(f"lpips_bwd: g_layers must be [{N},5], got {tuple(g_layers.shape)}")
    x, y, g_layers = x.detach(), y.detach(), g_layers.detach().float().contiguous()
    rec = net.record(x.device)
    lib = _lib.load()
    if workspace is None:
        fixed, one = (lib.snerf_lpips_bwd_workspace_bytes(k, H, W, rec.channels) for k in (0, 1))
        if one < 0:
            check(-1, "snerf_lpips_bwd_workspace_bytes")
        pairs = max(1, min(N, (LPIPS_WORKSPACE_BYTES - fixed) // (one - fixed), max_pairs if max_pairs else N))
        workspace = torch.empty((fixed + pairs * (one - fixed),), device=x.device, dtype=torch.uint8)
    dx, dy = (torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=torch.float32) if want else None for want in (want_x, want_y))
    layers = torch.empty((N, 5), device=x.device, dtype=torch.float32) if want_layers else None
    with torch.cuda.device(x.device), _lib.timed(f"lpips_bwd[{N}x{H}x{W}]"):
        check(lib.snerf_lpips_bwd_f32(ctypes.byref(rec), ptr(x), ptr(y), N, H, W, *x.stride(), ptr(g_layers), ptr(dx), ptr(dy), ptr(layers),
                                      ptr(workspace), workspace.numel(), current_stream()), "snerf_lpips_bwd_f32")
    return dx, dy, layers


class _LpipsLossFn(torch.autograd.Function):
    """snerf_lpips_fwd_f32 / snerf_lpips_bwd_f32 under autograd: (layers [N,5], total [N]).  The frames are kept, no activation is:
    the backward entry recomputes the forward chunk by chunk.  The net's weights are constants."""

    @staticmethod
    def forward(ctx, x, y, net):
        layers, total = lpips_layers(x.detach(), y.detach(), net)
        ctx.save_for_backward(x, y)
        ctx.net = net
        ctx.set_materialize_grads(False)
        return layers, total

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_layers, g_total):
        if g_layers is None and g_total is None:
            return None, None, None
        x, y = ctx.saved_tensors
        # total = the sum of the five layers: its gradient reaches each of them
        g = g_layers.float() if g_layers is not None else torch.zeros((x.shape[0], 5), device=x.device, dtype=torch.float32)
        if g_total is not None:
            g = g + g_total.float()[:, None]
        dx, dy, _ = lpips_bwd(x, y, ctx.net, g, want_x=ctx.needs_input_grad[0], want_y=ctx.needs_input_grad[1])
        return dx, dy, None


def lpips_loss(x, y, net, reduction: str = 'mean', per_layer: bool = False):
    """ops.lpips as a training loss: the same value, bit for bit (the forward is the same entry), and differentiable once with respect
    to x and y - the reference's ContentLoss is a _Loss with frozen weights (util/scores.py:286-411).  The backward is one call of
    snerf_lpips_bwd_f32: the VGG stack is walked forward and back chunk by chunk within LPIPS_WORKSPACE_BYTES, so no activation
    outlives it.  Frames [N,3,H,W] fp32, channels-first or channels-last views without a copy; H, W >= 16.  The weights of `net` get no
    gradient.  Under torch.no_grad(), or with no input that requires grad, this is ops.lpips."""
    if reduction not in ('mean', 'sum', 'none'):
        raise KeyError(reduction)
    if not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):
        return lpips(x, y, net, reduction=reduction, per_layer=per_layer)
    _need_cuda("x", x)
    _need_cuda("y", y)
    if x.dim() != 4 or x.shape != y.shape or x.shape[1] != 3:
        raise RuntimeError(f"lpips: x and y must be [N,3,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise RuntimeError(f"lpips: x on {x.device}, y on {y.device}")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise RuntimeError(f"lpips_loss: fp32 frames, got {x.dtype} and {y.dtype}")
    x, y = _ssim_layout(x, y)
    layers, total = _LpipsLossFn.apply(x, y, net)
    if reduction != 'none':
        op = {'mean': torch.mean, 'sum': torch.sum}[reduction]
        total, layers = op(total, dim=0), op(layers, dim=0)
    return (total, layers) if per_layer else total
