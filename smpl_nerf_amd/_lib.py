"""ctypes binding of libsmplnerf_hip.so (include/smplnerf.h).

There is exactly one implementation of every op in this package: the HIP library.  If it is
missing, or a call fails, a RuntimeError is raised - there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libsmplnerf_hip.so")
SPLIT_F16X3 = 16   # include/smplnerf.h SNERF_SPLIT_F16X3: nsplit / precision code of the two-part fp16 kernel
FP32_INFER = 32    # include/smplnerf.h SNERF_FP32_INFER: precision code of the render entries - fp32 kernels, composed inference streams
REFERENCE_SUM = 0x100  # include/smplnerf.h SNERF_REFERENCE_SUM: ORed into a precision, the sampler sums in torch's CPU order

SNERF_OK = 0

# `precision` of a net -> nsplit / precision code of its matrix-core arithmetic (include/smplnerf.h); 0 = the exact fp32 kernels
PRECISIONS = {"fp32": 0, "bf16x3": 2, "bf16x6": 3, "f16x3": SPLIT_F16X3}


def precision_code(nets, what="render_rays") -> int:
    """The one precision code of `nets`, which one call or one render runs together.  The split-precision kernels exist for width
    256: with any other width among them the code is 0 (exact fp32), as is that of a name the table does not hold."""
    name, code = nets[0].precision, None      # (plain loops: every launch of the launch-by-launch forward asks, for one net)
    for m in nets:
        if m.precision != name:
            raise RuntimeError(f"{what}: all nets must use the same precision mode (set_precision)")
        if m.width != 256:
            code = 0
    return PRECISIONS.get(name, 0) if code is None else code


class MlpDesc(ctypes.Structure):
    """struct snerf_mlp_desc (include/smplnerf.h) - mirrors RenderRayNet.__init__ (models/render_ray_net.py:8)."""
    _fields_ = [("n_layers", c_int32), ("width", c_int32), ("pos_freqs", c_int32), ("pos_identity", c_int32),
                ("dir_freqs", c_int32), ("dir_identity", c_int32), ("add_dim", c_int32), ("skip_mask", c_uint32),
                ("use_dir", c_int32), ("add_first", c_int32)]


class WarpDesc(ctypes.Structure):
    """struct snerf_warp_desc - mirrors WarpFieldNet.__init__ (models/warp_field_net.py:8)."""
    _fields_ = [("width", c_int32), ("pos_freqs", c_int32), ("pos_identity", c_int32), ("pose_dim", c_int32)]


_P = c_void_p  # device pointers travel as integers (tensor.data_ptr())


class SmplModel(ctypes.Structure):
    """struct snerf_smpl_model - the body model's device arrays and its parent table (a HOST array of J int32)."""
    _fields_ = [("V", c_int32), ("J", c_int32), ("NB", c_int32), ("v_template", _P), ("blend", _P), ("J_template", _P),
                ("J_dirs", _P), ("weights", _P), ("parents", POINTER(c_int32))]


class ConvBn(ctypes.Structure):
    """struct snerf_conv_bn - one Conv2d + BatchNorm2d of SmplEstimator: device pointers to the state_dict's tensors, and bn.eps."""
    _fields_ = [("weight", _P), ("bias", _P), ("bn_weight", _P), ("bn_bias", _P), ("running_mean", _P), ("running_var", _P),
                ("eps", c_double)]


class SmplEstimatorNet(ctypes.Structure):
    """struct snerf_smpl_estimator - models/smpl_estimator.py:14-30."""
    _fields_ = [("block", ConvBn * 5), ("fc1_weight", _P), ("fc1_bias", _P), ("fc2_weight", _P), ("fc2_bias", _P),
                ("human_size", c_int32)]


class ConvWb(ctypes.Structure):
    """struct snerf_conv_wb - one convolution of the VGG stack: device pointers to its weight and bias."""
    _fields_ = [("weight", _P), ("bias", _P)]


class VggLpipsNet(ctypes.Structure):
    """struct snerf_vgg_lpips - the 13 convolutions of vgg16().features, the five lin vectors, the input standardisation."""
    _fields_ = [("conv", ConvWb * 13), ("channels", c_int32 * 5), ("lin", _P * 5), ("mean", c_float * 3), ("std", c_float * 3)]


class MeshRenderArgs(ctypes.Structure):
    """struct snerf_mesh_render_args - the shading constants and flags of snerf_mesh_render_f32."""
    _fields_ = [("ambient", c_float), ("intensity", c_float), ("background", c_float * 3), ("flags", c_int32)]


RENDER_NO_CULL = 1     # include/smplnerf.h SNERF_RENDER_NO_CULL


class AdamState(ctypes.Structure):
    """struct snerf_adam_state - torch.optim.Adam over one flat fp32 buffer (solver/nerf_solver.py:11-14, 31-33)."""
    _fields_ = [("params", _P), ("grads", _P), ("exp_avg", _P), ("exp_avg_sq", _P), ("n_params", c_int64),
                ("scratch", _P), ("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("weight_decay", c_double)]


class AdamRange(ctypes.Structure):
    """struct snerf_adam_range - adjacent parameter tensors taking part in a step, with their device step counters."""
    _fields_ = [("begin", c_int64), ("end", c_int64), ("step", _P), ("n_steps", c_int32)]


class AdamNet(ctypes.Structure):
    """struct snerf_adam_net - a RenderRayNet inside the flat buffer whose weight streams the optimiser step keeps current."""
    _fields_ = [("desc", POINTER(MlpDesc)), ("param_offset", c_int64), ("precision", c_int32), ("packed", _P),
                ("packed_t", _P), ("slot_fwd", _P), ("slot_t", _P)]


class NerfBatch(ctypes.Structure):
    """struct snerf_nerf_batch - the Solver's batch (solver/nerf_solver.py:77-81) plus u and the sigma noise."""
    _fields_ = [("ray_samples", _P), ("rays_o", _P), ("rays_d", _P), ("z_vals", _P), ("rgb_truth", _P), ("u", _P),
                ("noise_coarse", _P), ("noise_fine", _P), ("additional", _P), ("B", c_int64), ("Nc", c_int32), ("Nf", c_int32),
                ("white_background", c_int32)]


class InputGrads(ctypes.Structure):      # snerf_input_grads
    _fields_ = [("d_additional", _P), ("params_coarse", _P), ("params_fine", _P)]


# The parameter groups the training entries share, in the header's order:
_D, _W = POINTER(MlpDesc), POINTER(WarpDesc)
_NETS = [_D, _P, _P, _D, _P, _P]      # desc, packed, packed_t of the coarse and of the fine net
_WARP = [_W, _P, _P]                  # desc_warp, packed_warp, packed_t_warp
# precision, batch, rays_per_chunk, workspace, grad_coarse, grad_fine, loss, rgb, rgb_fine
_NERF = _NETS + [c_int, POINTER(NerfBatch), c_int64, _P, _P, _P, _P, _P, _P]
# precision, batch, pose_enc, rays_per_chunk, workspace, grad_coarse, grad_fine, grad_warp, loss, rgb, rgb_fine
_SMPL = _NETS + _WARP + [c_int, POINTER(NerfBatch), _P, c_int64, _P, _P, _P, _P, _P, _P, _P]
_ADAM = [POINTER(AdamState), POINTER(AdamRange), c_int, POINTER(AdamNet), c_int]      # adam, ranges_host, n_ranges, nets_host, n_nets
_IG = [POINTER(InputGrads)]
_OFF = [c_int64]                      # warp_param_offset
# (what follows them: the optional comm, then stream and, where the entry has one, aux_stream)

# name -> (restype, argtypes); must list every symbol include/smplnerf.h declares
SIGNATURES = {
    "snerf_version": (c_int, []),
    "snerf_last_error_string": (c_char_p, []),
    "snerf_device_count": (c_int, []),
    "snerf_shutdown": (c_int, []),
    "snerf_searchsorted_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int, _P]),
    "snerf_searchsorted": (c_int, [c_int, _P, c_int64, c_int64, _P, c_int64, c_int64, _P, c_int, _P]),
    "snerf_posenc_bwd_f32": (c_int, [_P, _P, c_int64, c_int, c_int, c_int, _P, _P]),
    "snerf_composite_bwd_all_f32": (c_int, [_P, _P, _P, c_int, _P, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "snerf_posenc_f32": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, _P]),
    "snerf_composite_fwd_f32": (c_int, [_P, _P, _P, c_int, _P, c_int64, c_int, c_int, _P, _P, _P, _P]),
    "snerf_composite_bwd_f32": (c_int, [_P, _P, _P, c_int, _P, c_int64, c_int, c_int, _P, _P, _P, _P]),
    # the ray maps: opacity, expected depth and expected point from a compositing's alpha (csrc/ray_maps.hip)
    "snerf_ray_maps_fwd_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P]),
    "snerf_ray_maps_bwd_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P]),
    "snerf_sample_pdf_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int, c_int, _P, _P, _P, _P, _P]),
    "snerf_sample_pdf_strict_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int, c_int, _P, _P, _P, _P, _P]),
    "snerf_sample_pdf_bins_strict_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, _P, _P, _P]),
    "snerf_sample_pdf_bins_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int, c_int, _P, _P, _P]),
    "snerf_sample_pdf_bins_f32": (c_int, [_P, _P, _P, c_int64, c_int, c_int, _P, _P, _P]),
    "snerf_reference_sum_f32": (c_int, [_P, c_int64, c_int64, c_int, c_float, _P, _P]),
    "snerf_reference_sum_host_f32": (c_int, [_P, c_int64, c_int64, c_int, c_float, _P]),
    "snerf_mlp_param_floats": (c_int64, [POINTER(MlpDesc)]),
    "snerf_mlp_packed_floats": (c_int64, [POINTER(MlpDesc)]),
    "snerf_mlp_pack_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P]),
    "snerf_mlp_fwd_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, c_int, _P, c_int64, c_int, _P, _P]),
    "snerf_mlp_packed_bf16_bytes": (c_int64, [POINTER(MlpDesc), c_int]),
    "snerf_mlp_pack_bf16": (c_int, [POINTER(MlpDesc), _P, _P, c_int, _P]),
    "snerf_mlp_fwd_bf16_f32": (c_int, [POINTER(MlpDesc), _P, c_int, _P, _P, c_int, _P, c_int64, c_int, _P, _P]),
    "snerf_mlp_fwd_train_bf16_f32": (c_int, [POINTER(MlpDesc), _P, c_int, _P, _P, c_int, _P, c_int64, c_int, _P, _P, _P]),
    "snerf_mlp_packed_t_bf16_bytes": (c_int64, [POINTER(MlpDesc), c_int, c_int]),
    "snerf_mlp_pack_t_bf16": (c_int, [POINTER(MlpDesc), _P, _P, c_int, c_int, _P]),
    "snerf_mlp_bwd_bf16_f32": (c_int, [POINTER(MlpDesc), _P, c_int, _P, _P, c_int64, _P, _P, _P, _P]),
    "snerf_mlp_bwd_inputs_bf16_f32": (c_int, [POINTER(MlpDesc), _P, c_int, _P, _P, _P, _P, c_int, c_int, c_int64, _P, _P, _P,
                                              _P, _P, _P]),
    "snerf_mlp_train_sizes": (c_int, [POINTER(MlpDesc), c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                      POINTER(c_int64), POINTER(c_int32)]),
    "snerf_mlp_dy_layout": (c_int, [POINTER(MlpDesc), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "snerf_mlp_fwd_train_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, c_int, _P, c_int64, c_int, _P, _P, _P]),
    "snerf_mlp_fwd_encoded_train_f32": (c_int, [POINTER(MlpDesc), _P, _P, c_int64, c_int64, _P, _P, _P]),
    "snerf_mlp_pack_t_f32": (c_int, [POINTER(MlpDesc), _P, _P, c_int, _P]),
    "snerf_mlp_bwd_inputs_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, _P, _P, c_int, c_int, c_int64, _P, _P, _P, _P, _P,
                                         _P]),
    "snerf_mlp_bwd_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, c_int64, _P, _P, _P, _P]),
    "snerf_warp_param_floats": (c_int64, [POINTER(WarpDesc)]),
    "snerf_warp_packed_floats": (c_int64, [POINTER(WarpDesc)]),
    "snerf_warp_pack_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P]),
    "snerf_warp_fwd_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P]),
    "snerf_warp_packed_bf16_bytes": (c_int64, [POINTER(WarpDesc)]),
    "snerf_warp_pack_bf16": (c_int, [POINTER(WarpDesc), _P, _P, _P]),
    "snerf_warp_fwd_bf16_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P]),
    "snerf_warp_train_sizes": (c_int, [POINTER(WarpDesc), c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                       POINTER(c_int64)]),
    "snerf_warp_fwd_train_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P]),
    "snerf_warp_pack_t_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P]),
    "snerf_warp_bwd_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P, c_int64, _P, _P, _P, _P]),
    # DynamicPipeline's vertex-attention warp (csrc/vertex_warp.hip)
    "snerf_vertex_warp_fwd_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P]),
    "snerf_vertex_warp_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int64, c_int, c_int, c_float, c_float, _P, _P, _P, _P]),
    # the image-wise model's linear-attention warp, one body per image (csrc/image_warp.hip)
    "snerf_image_warp_fwd_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_double, c_double, _P, _P, _P, _P, _P]),
    "snerf_image_warp_bwd_workspace_bytes": (c_int64, [c_int64, c_int]),
    "snerf_image_warp_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int64, c_int, c_int, c_double, _P, c_int64, _P, _P, _P, _P]),
    # the canonical-density loss of SmplNerfSolver: Gaussian-mixture pdf and its sample gradient (csrc/gmm_pdf.hip)
    "snerf_gmm_pdf_f32": (c_int, [_P, _P, c_int64, c_int, c_float, _P, _P, _P]),
    # the SMPL body model: linear blend skinning (csrc/smpl_lbs.hip)
    "snerf_smpl_lbs_fwd_f32": (c_int, [POINTER(SmplModel), _P, c_int, _P, _P, c_int64, _P, _P, _P, _P]),
    "snerf_smpl_lbs_bwd_workspace_bytes": (c_int64, [POINTER(SmplModel), c_int64]),
    "snerf_smpl_lbs_bwd_f32": (c_int, [POINTER(SmplModel), _P, c_int, _P, _P, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P]),
    # the vertex_sphere model: ray-mesh hits (csrc/ray_mesh.hip) and the sphere warp (csrc/vertex_sphere.hip)
    "snerf_ray_mesh_workspace_bytes": (c_int64, [c_int]),
    "snerf_ray_mesh_hits_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_int, _P, _P, _P, c_int64, _P]),
    "snerf_ray_mesh_first_hit_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
    # the mesh renderer: textured, lit frames from poses (csrc/mesh_render.hip)
    "snerf_mesh_render_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "snerf_mesh_render_f32": (c_int, [_P, c_double, c_int64, c_int, c_int, _P, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_int, c_int,
                                      POINTER(MeshRenderArgs), _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
    # the soft silhouette with its vertex gradient (csrc/soft_silhouette.hip)
    "snerf_soft_silhouette_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "snerf_soft_silhouette_fwd_f32": (c_int, [_P, c_double, c_int64, c_int, c_int, _P, c_int, c_int, _P, c_int, c_double, c_double, c_int,
                                              _P, _P, _P, c_int64, _P]),
    "snerf_soft_silhouette_bwd_f32": (c_int, [_P, c_double, c_int64, c_int, c_int, _P, c_int, c_int, _P, c_int, c_double, c_double, c_int,
                                              _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
    "snerf_vertex_sphere_warp_f32": (c_int, [_P, _P, _P, c_int64, c_int, c_float, c_int, _P, _P, _P, _P]),
    # image scores: SSIM with its backward and the squared error of MSE / PSNR (csrc/ssim.hip)
    "snerf_ssim_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int64, c_int]),
    "snerf_ssim_fwd_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, _P, c_int, c_float,
                                   c_float, _P, _P, _P, _P, c_int64, _P]),
    "snerf_ssim_bwd_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, _P, c_int, c_float,
                                   c_float, _P, _P, _P, _P, c_int64, _P]),
    # SmplEstimator, inference: the fused conv-BN-ReLU-pool block and the whole network (csrc/conv_block.hip)
    "snerf_conv3x3_block_f32": (c_int, [_P, c_int64, c_int, c_int64, c_int64, _P, _P, _P, c_int, c_int, c_int, _P, _P]),
    "snerf_smpl_estimator_workspace_bytes": (c_int64, [c_int64, c_int]),
    "snerf_smpl_estimator_fwd_f32": (c_int, [POINTER(SmplEstimatorNet), _P, c_int64, _P, _P, c_int64, _P]),
    # LPIPS: the convolution block with a tap, the tap distance, the whole metric (csrc/conv_block.hip, csrc/lpips.hip)
    "snerf_conv3x3_block_tap_f32": (c_int, [_P, c_int64, c_int, c_int64, c_int64, _P, _P, _P, c_int, c_int, _P, _P, _P]),
    "snerf_feature_distance_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "snerf_feature_distance_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, _P, c_int, _P, _P, c_int64, _P]),
    "snerf_lpips_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, POINTER(c_int32)]),
    "snerf_lpips_fwd_f32": (c_int, [POINTER(VggLpipsNet), _P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P,
                                    _P, c_int64, _P]),
    # LPIPS as a loss: the distance gradient, the ReLU / max-pool backward, the whole backward (csrc/lpips.hip)
    "snerf_feature_distance_bwd_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, _P, c_int, _P, _P, _P, _P]),
    "snerf_relu_pool_bwd_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int64, _P, _P]),
    "snerf_lpips_bwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, POINTER(c_int32)]),
    "snerf_lpips_bwd_f32": (c_int, [POINTER(VggLpipsNet), _P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P,
                                    _P, _P, _P, c_int64, _P]),
    # SmplEstimator, training: batch statistics, the block's apply and backward, the convolution's gradients (csrc/conv_train.hip)
    "snerf_bn_stats_scratch_floats": (c_int64, [c_int64, c_int, c_int64, c_int64]),
    "snerf_bn_stats_f32": (c_int, [_P, c_int64, c_int, c_int64, c_int64, c_double, c_double, _P, _P, _P, _P, _P, _P]),
    "snerf_bn_relu_pool_fwd_f32": (c_int, [_P, c_int64, c_int, c_int64, c_int64, _P, _P, _P, _P, c_int, c_int, _P, _P]),
    "snerf_bn_relu_pool_bwd_scratch_floats": (c_int64, [c_int64, c_int, c_int64, c_int64, c_int]),
    "snerf_bn_relu_pool_bwd_f32": (c_int, [_P, _P, c_int64, c_int, c_int64, c_int64, _P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "snerf_conv3x3_bwd_input_scratch_floats": (c_int64, [c_int, c_int]),
    "snerf_conv3x3_bwd_input_f32": (c_int, [_P, c_int64, c_int, c_int64, c_int64, _P, c_int, _P, _P, _P]),
    "snerf_conv3x3_bwd_weight_slices": (c_int64, [c_int64, c_int, c_int64, c_int64, c_int]),
    "snerf_conv3x3_bwd_weight_scratch_floats": (c_int64, [c_int64, c_int, c_int64, c_int64, c_int]),
    "snerf_conv3x3_bwd_weight_f32": (c_int, [_P, _P, c_int64, c_int, c_int, c_int64, c_int64, _P, _P, _P, _P]),
    "snerf_raygen_f64": (c_int, [_P, c_int64, c_int, c_int, c_double, _P, _P, c_int, _P, _P, c_int64, _P, _P, _P, _P, _P]),
    "snerf_mlp_fwd_encoded_f32": (c_int, [POINTER(MlpDesc), _P, _P, c_int64, c_int64, _P, _P]),
    "snerf_render_rays_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "snerf_render_rays_smpl_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "snerf_render_rays_smpl_f32": (c_int, [POINTER(MlpDesc), _P, POINTER(MlpDesc), _P, POINTER(WarpDesc), _P, c_int, _P, _P, _P, _P,
                                           _P, _P, _P, _P, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "snerf_render_rays_add_workspace_bytes": (c_int64, [POINTER(MlpDesc), POINTER(MlpDesc), c_int64, c_int, c_int]),
    "snerf_render_rays_add_f32": (c_int, [POINTER(MlpDesc), _P, POINTER(MlpDesc), _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_int64,
                                          c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "snerf_render_rays_f32": (c_int, [POINTER(MlpDesc), _P, POINTER(MlpDesc), _P, c_int, _P, _P, _P, _P, _P, _P, _P, c_int64,
                                      c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "snerf_mlp_fold_workspace_bytes": (c_int64, [POINTER(MlpDesc), c_int64, c_int]),
    "snerf_mlp_fwd_ws_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, c_int, _P, c_int64, c_int, _P, _P, c_int64, _P]),
    # fp32 inference on the composed stream (csrc/mlp_plan.h: make_plan_infer)
    "snerf_mlp_packed_infer_floats": (c_int64, [POINTER(MlpDesc)]),
    "snerf_mlp_pack_infer_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P]),
    "snerf_mlp_fwd_infer_f32": (c_int, [POINTER(MlpDesc), _P, _P, _P, c_int, _P, c_int64, c_int, _P, _P, c_int64, _P]),
    "snerf_warp_fold_workspace_bytes": (c_int64, [POINTER(WarpDesc), c_int64, c_int]),
    "snerf_warp_fwd_ws_f32": (c_int, [POINTER(WarpDesc), _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, c_int64, _P]),
    "snerf_dy_contract_scratch_floats": (c_int64, [c_int64, c_int, c_int]),
    "snerf_dy_contract_f32": (c_int, [_P, c_int64, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, c_int64, c_int, c_int, _P, _P]),
    "snerf_mlp_stream_slots": (c_int, [POINTER(MlpDesc), _P, _P, c_int, _P]),
    "snerf_smpl_nerf_train_workspace_bytes": (c_int64, [POINTER(MlpDesc), POINTER(MlpDesc), POINTER(WarpDesc), c_int64, c_int, c_int,
                                                        c_int64]),
    "snerf_smpl_nerf_train_grads_f32": (c_int, _SMPL + [_P]),
    "snerf_smpl_nerf_train_step_f32": (c_int, _SMPL + _ADAM + _OFF + [_P]),
    "snerf_warp_repack_f32": (c_int, [POINTER(WarpDesc), _P, c_int64, c_int64, _P, _P, _P]),
    "snerf_adam_step_f32": (c_int, [POINTER(AdamState), POINTER(AdamRange), c_int, POINTER(AdamNet), c_int, _P]),
    "snerf_nerf_train_workspace_bytes": (c_int64, [POINTER(MlpDesc), POINTER(MlpDesc), c_int64, c_int, c_int, c_int64]),
    "snerf_nerf_train_grads_f32": (c_int, _NERF + [_P, _P]),
    "snerf_nerf_train_step_f32": (c_int, _NERF + _ADAM + [_P, _P]),
    "snerf_nerf_train_grads_ig_f32": (c_int, _NERF + _IG + [_P, _P]),
    "snerf_nerf_train_step_ig_f32": (c_int, _NERF + _ADAM + _IG + [_P, _P]),
    # any --netwidth: nn.Linear as stand-alone GEMMs (csrc/linear.hip)
    "snerf_linear_fwd_f32": (c_int, [_P, c_int64, c_int, c_int64, _P, c_int64, c_int, _P, c_int, c_int, _P, c_int64, _P]),
    "snerf_linear_bwd_input_f32": (c_int, [_P, c_int64, c_int, c_int64, _P, c_int64, c_int, c_int, _P, c_int64, _P]),
    "snerf_linear_bwd_weight_scratch_floats": (c_int64, [c_int64, c_int, c_int]),
    "snerf_linear_bwd_weight_f32": (c_int, [_P, c_int64, c_int, c_int64, _P, c_int64, c_int, c_int, _P, c_int64, _P, _P, _P]),
    "snerf_relu_bwd_f32": (c_int, [_P, _P, c_int64, c_int, c_int64, c_int64, _P]),
    # 8(e): RCCL inside the boundary
    "snerf_comm_unique_id": (c_int, [_P]),
    "snerf_comm_init_rank": (c_int, [_P, c_int, c_int, POINTER(_P)]),
    "snerf_comm_destroy": (c_int, [_P]),
    "snerf_comm_info": (c_int, [_P, POINTER(ctypes.c_int32), POINTER(ctypes.c_int32)]),
    "snerf_comm_allreduce_avg_f32": (c_int, [_P, _P, c_int64, _P]),
    "snerf_nerf_train_step_dp_f32": (c_int, _NERF + _ADAM + [_P, _P, _P]),
    "snerf_nerf_train_step_dp_ig_f32": (c_int, _NERF + _ADAM + _IG + [_P, _P, _P]),
    "snerf_smpl_nerf_train_step_dp_f32": (c_int, _SMPL + _ADAM + _OFF + [_P, _P]),
    "snerf_smpl_nerf_train_grads_aux_f32": (c_int, _SMPL + [_P, _P]),
    "snerf_smpl_nerf_train_step_aux_f32": (c_int, _SMPL + _ADAM + _OFF + [_P, _P, _P]),
}

_lib = None


def load():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m smpl_nerf_amd.build` (hipcc, gfx950). "
            "smpl_nerf_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first so both share one HIP runtime)
    except Exception:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != SNERF_OK:
        msg = load().snerf_last_error_string()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-launch timing (HIP events on the launch stream) ---------------------------------
_PROFILE = None


class profile:
    """Context manager: records a pair of events (on the stream the kernels are launched on, i.e.
    PyTorch's current stream) around every C-ABI launch made through `timed()`.

        with _lib.profile() as prof: pipeline(data)
        prof.summary() -> {name: (calls, total_ms)}
    """

    def __enter__(self):
        global _PROFILE
        self.records = []
        self._prev = _PROFILE
        _PROFILE = self
        return self

    def __exit__(self, *exc):
        global _PROFILE
        _PROFILE = self._prev
        return False

    def summary(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.records:
            calls, ms = out.get(name, (0, 0.0))
            out[name] = (calls + 1, ms + e0.elapsed_time(e1))
        return out


CALLS = 0      # C-ABI launches made through timed() since import (bench.py: calls per step of an unprofiled loop)


class timed:
    """with timed("mlp_fwd"): lib.snerf_...(...)  - counts the call; records an event pair when a profile() is active."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global CALLS
        CALLS += 1
        if _PROFILE is not None:
            import torch
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _PROFILE is not None:
            self.e1.record()
            _PROFILE.records.append((self.name, self.e0, self.e1))
        return False
