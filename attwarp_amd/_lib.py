"""ctypes binding of libattwarp_hip.so (C ABI declared in include/attwarp.h).

The HIP library is the product: there is NO CPU fallback.  Importing this module
on a machine without the built library raises ImportError; calling any op on a
non-GPU tensor raises.  Build with ``python __graft_entry__.py`` or
``make -C attwarp_amd/csrc``.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from ctypes import c_double, c_float, c_int, c_int64, c_size_t, c_void_p, c_char_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libattwarp_hip.so")
# the same sources built with -DATTWARP_TUNING: attwarp_debug_set() can force kernel variants.  Loaded only by
# debug_override() (parity tests, A/B tools); the product never touches it.
TUNING_LIB_PATH = os.path.join(_HERE, "csrc", "libattwarp_hip_tuning.so")

# enums of include/attwarp.h
F32, F16, BF16, U8, F64 = 0, 1, 2, 3, 4
HWC, CHW = 0, 1
EXACT, CV2 = 0, 1
TRANSFORM_IDS = {"identity": 0, "square": 1, "sqrt": 2, "exp": 3, "log": 4}
MODE_IDS = {"exact": EXACT, "cv2": CV2}

_DTYPE_IDS = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16, torch.uint8: U8, torch.float64: F64}

# name -> (restype, argtypes); must list every symbol the header declares
SIGNATURES = {
    "attwarp_version": (c_int, []),
    "attwarp_last_error": (c_char_p, []),
    "attwarp_attn_reduce_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64,
                                          c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "attwarp_attn_finalize": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_attn_reduce_stack_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "attwarp_attn_reduce_stack": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                           c_void_p, c_void_p]),
    "attwarp_attn_probe_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "attwarp_attn_probe_last_query": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int64,
                                               c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_float,
                                               c_void_p, c_void_p, c_void_p]),
    "attwarp_attn_probe_head_mean": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int64,
                                              c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_float,
                                              c_void_p, c_void_p, c_void_p]),
    "attwarp_masked_token_mean": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_film_axis_means": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "attwarp_film_axis_means_t": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p]),
    "attwarp_film_axis_means_backward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                                  c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "attwarp_mask_postproc": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "attwarp_mask_upsample_lanczos": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                               c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                               c_void_p]),
    "attwarp_clip_preprocess_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                            c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int, c_void_p]),
    "attwarp_adaptive_avg_pool": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_axis_sums_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "attwarp_gt_marginals": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_safe_softmax": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    "attwarp_safe_softmax_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    "attwarp_upsample_pdf_right_inverse": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "attwarp_cdf_from_density": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_make_strictly_increasing": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p]),
    "attwarp_resample_cdf": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_axis_map_from_cdf": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_axis_maps_from_pdf": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_axis_maps_from_steps": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_axis_maps_from_attention": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                                  c_double, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_warp_step_fused": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_warp_step_fused_slots": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                               c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "attwarp_attn_reduce_and_maps": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                              c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "attwarp_mask_chain_step": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_int, c_int, c_float, c_void_p,
                                         c_int, c_double, c_double, c_int, c_void_p, c_void_p]),
    "attwarp_attention_transform_lut": (c_int, [c_int, c_double, c_double, c_void_p, c_void_p]),
    "attwarp_pil_coeffs_8bpc": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "attwarp_ragged_table_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "attwarp_ragged_plan": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    "attwarp_mask_chain_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_int, c_int, c_float, c_void_p,
                                           c_int, c_double, c_double, c_int, c_void_p, c_void_p]),
    "attwarp_axis_maps_from_steps_t": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_resize_linear": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "attwarp_remap_bilinear": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_int, c_void_p]),
    "attwarp_overlay_workspace_bytes": (c_size_t, [c_int]),
    "attwarp_heatmap_overlay": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int, c_void_p, c_void_p]),
    # the layer-selection study's LANCZOS4 maps and box metrics (grounding.hip)
    "attwarp_lanczos4_coeffs": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "attwarp_resize_lanczos4": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "attwarp_box_metrics_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_box_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    # the Stable-Diffusion warp ablation (sdwarp.hip)
    "attwarp_xattn_chunk": (c_int, [c_int]),
    "attwarp_xattn_reduce_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "attwarp_xattn_reduce": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_cubic_coeffs": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "attwarp_resize_cubic": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "attwarp_gaussian5_taps": (c_int, [c_double, c_void_p]),
    "attwarp_blur5_minmax_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_blur5_minmax": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_minmax_normalize": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    # the MarginalNet training losses (losses.hip, profiles.hip)
    "attwarp_cdf_downsample": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "attwarp_build_axis_cdf_targets": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_l1_cdf_loss": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_l1_cdf_loss_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_sym_kl": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_sym_kl_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_recon_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "attwarp_recon_loss_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    "attwarp_scale_shift": (c_int, [c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p]),
    "attwarp_entropy": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_entropy_backward": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "attwarp_pdf_l1_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_pdf_l1_loss_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_trainer_attention_targets": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                  c_void_p, c_void_p]),
    # the trainer's batches from decoded samples (dataprep.hip)
    "attwarp_prep_images_table_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "attwarp_prep_images_plan": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    "attwarp_prep_images_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "attwarp_pil_nearest_index": (c_int, [c_int, c_int, c_void_p]),
    "attwarp_prep_attention_workspace_bytes": (c_size_t, [c_int]),
    "attwarp_prep_attention_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # the first visit to CLIP: ragged batches, pad-to-square included (clip_ragged.hip)
    "attwarp_clip_images_table_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "attwarp_clip_images_plan": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t]),
    "attwarp_clip_images_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    # the trainer's optimiser step (optim.hip)
    "attwarp_adamw_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "attwarp_adamw_step": (c_int, [c_void_p, c_int, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p]),
    # PNG files of a ragged batch (png.hip)
    "attwarp_png_bound": (c_size_t, [c_int, c_int, c_int]),
    "attwarp_png_table_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_png_plan": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "attwarp_png_table_bytes_ex": (c_size_t, [c_void_p, c_int, c_void_p]),
    "attwarp_png_plan_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_size_t]),
    "attwarp_png_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    # PNG files decoded on the device (pngdec.hip)
    "attwarp_pngdec_table_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "attwarp_pngdec_plan": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t]),
    "attwarp_pngdec_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "attwarp_pngdec_table_bytes_formats": (c_size_t, [c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "attwarp_pngdec_plan_formats": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t]),
    "attwarp_pngdec_table_bytes_wave": (c_size_t, [c_void_p, c_void_p, c_int, c_void_p, c_int]),
    "attwarp_pngdec_plan_wave": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    # baseline JPEG files decoded on the device (jpegdec.hip)
    "attwarp_jpegdec_table_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_jpegdec_plan": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "attwarp_jpegdec_plan_ex": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_int, c_int]),
    "attwarp_jpegdec_info_offset": (ctypes.c_uint64, [c_void_p]),
    "attwarp_jpegdec_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    # progressive files: every scan planned, scans by dependency level
    "attwarp_jpegdec_scans_table_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "attwarp_jpegdec_plan_scans": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_int]),
    "attwarp_jpegdec_decode_scans": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    # the same with marker-less scans cut into segments (segment_bytes, max_rounds, per scan the bytes of its entropy data)
    "attwarp_jpegdec_scans_table_bytes_ex": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "attwarp_jpegdec_plan_scans_ex": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "attwarp_jpegdec_scan_info_offset": (ctypes.c_uint64, [c_void_p]),
    # every layout of a sequential file: four components, any sampling, RGB-coded (jpegdec.hip, jpegfmt_blocks.hpp)
    "attwarp_jpegdec_layouts_table_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_jpegdec_plan_layouts": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_int, c_int]),
    "attwarp_jpegdec_decode_layouts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    # scans of every layout: progressive files of the layout family's frames, sequential files of several scans (jpegscan_blocks.hpp)
    "attwarp_jpegdec_layout_scans_table_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "attwarp_jpegdec_plan_layout_scans": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_int]),
    "attwarp_jpegdec_layout_scans_table_bytes_ex": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "attwarp_jpegdec_plan_layout_scans_ex": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "attwarp_jpegdec_decode_layout_scans": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    # JPEG files of a ragged batch written on the device (jpegenc.hip)
    "attwarp_jpegenc_bound": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "attwarp_jpegenc_table_bytes": (c_size_t, [c_void_p, c_int]),
    "attwarp_jpegenc_plan": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "attwarp_jpegenc_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "attwarp_jpegenc_bound_ex": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "attwarp_jpegenc_table_bytes_ex": (c_size_t, [c_void_p, c_int, c_void_p]),
    "attwarp_jpegenc_plan_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_size_t]),
    "attwarp_jpegenc_bound_prog": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "attwarp_jpegenc_table_bytes_prog": (c_size_t, [c_void_p, c_int, c_void_p, c_void_p]),
    "attwarp_jpegenc_plan_prog": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]),
    # the trainer's debug / validation panels (panel.hip)
    "attwarp_panel_grid": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
}

PIL_LANCZOS, PIL_BICUBIC, PIL_BILINEAR = 0, 1, 2
RECON_MSE, RECON_L1 = 0, 1                          # attwarp_recon_loss kinds
TT_IDENTITY, TT_SQRT, TT_NONE = 0, 1, 2              # attwarp_trainer_attention_targets modes
OVERLAY_BLEND_MASK, OVERLAY_SAVE_WARPED = 0, 1       # attwarp_heatmap_overlay styles
RGB, BGR = 0, 1
# attwarp_png_*: filters and limits (ATTWARP_PNG_* of include/attwarp.h)
PNG_FILTER_IDS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
PNG_SEG_BYTES, PNG_MAX_ROW_BYTES, PNG_SEG_MAX_ROWS, PNG_FILE_OVERHEAD = 24576, 24576, 1024, 68
PNG_MATCH_IDS = {"rle": 0, "lz": 1}
# attwarp_pngdec_*: modes, limits and status codes (ATTWARP_PNGDEC_* of include/attwarp.h)
PNGDEC_MODE_IDS = {"RGB": 0, "L": 1, "keep": 2}
PNGDEC_MAX_UNITS, PNGDEC_MAX_ROW_BYTES = 256, 49152
PNGDEC_STATUS_NAMES = ("OK", "E_CRC", "E_ZLIB_HEADER", "E_TRUNCATED", "E_BLOCK_TYPE", "E_STORED_LEN", "E_CODE_LENGTHS", "E_SYMBOL",
                       "E_DISTANCE", "E_OVERFLOW", "E_UNDERFLOW", "E_ADLER", "E_FILTER")
(PNGDEC_OK, PNGDEC_E_CRC, PNGDEC_E_ZLIB_HEADER, PNGDEC_E_TRUNCATED, PNGDEC_E_BLOCK_TYPE, PNGDEC_E_STORED_LEN, PNGDEC_E_CODE_LENGTHS,
 PNGDEC_E_SYMBOL, PNGDEC_E_DISTANCE, PNGDEC_E_OVERFLOW, PNGDEC_E_UNDERFLOW, PNGDEC_E_ADLER, PNGDEC_E_FILTER) = range(13)
# attwarp_jpegdec_*: modes, limits and status codes (ATTWARP_JPEGDEC_* of include/attwarp.h)
JPEGDEC_MODE_IDS = {"RGB": 0, "L": 1, "keep": 2}
JPEGDEC_MAX_UNITS, JPEGDEC_MAX_BLOCKS = 65536, 1 << 24
JPEGDEC_MAX_SCANS = 64
JPEGDEC_RECORD_BYTES = 2152                              # one image record of a planned table (JdImage of jpegdec_blocks.hpp)
JPEGDEC_LAYOUT_RECORD_BYTES = 3000                       # one image record of the layout families' tables (JfImage of jpegfmt_blocks.hpp)
JPEGDEC_COLOR_IDS = {"grey": 0, "ycc": 1, "rgb": 2, "cmyk": 3, "ycck": 4}   # ATTWARP_JPEGDEC_COLOR_*: the colour rule of a layout image
JPEGDEC_MAX_SLOTS = 10                                   # blocks per MCU (T.81 B.2.3)
JPEGDEC_STATUS_NAMES = ("OK", "E_TRUNCATED", "E_HUFFMAN", "E_COEFF", "E_RESTART", "E_NO_EOI")
(JPEGDEC_OK, JPEGDEC_E_TRUNCATED, JPEGDEC_E_HUFFMAN, JPEGDEC_E_COEFF, JPEGDEC_E_RESTART, JPEGDEC_E_NO_EOI) = range(6)
# attwarp_jpegenc_*: Pillow's subsampling numbers and the limits (ATTWARP_JPEGENC_* of include/attwarp.h)
JPEGENC_SUBSAMPLING_IDS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
JPEGENC_UNIT_MCUS, JPEGENC_MAX_DIM = 16, 65500
# attwarp_panel_grid: limits, flags and source kinds (ATTWARP_PANEL_* of include/attwarp.h)
PANEL_MAX_SRC, PANEL_MAX_HEAT, PANEL_FOR_PNG = 8, 4096, 1
PANEL_F32, PANEL_U8, PANEL_HEAT = 0, 1, 2


class RaggedImage(ctypes.Structure):
    """attwarp_ragged_image (include/attwarp.h): one image of a ragged batch, device pointers in a host array."""
    _fields_ = [("image", c_void_p), ("bounds_x", c_void_p), ("kk_x", c_void_p), ("bounds_y", c_void_p), ("kk_y", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("ksize_x", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RaggedImageDev(ctypes.Structure):
    """The per-image record inside a table written by attwarp_ragged_plan (chain_ragged.hip: RaggedImage): the caller's
    record up to ksize_x, then what the plan adds."""
    _fields_ = RaggedImage._fields_[:-1] + [
        ("plan_w", ctypes.c_int32), ("plan_h", ctypes.c_int32), ("l_nchunks", ctypes.c_int32),
        ("l_rows_per_chunk", ctypes.c_int32), ("ki", ctypes.c_int32), ("mota_off", c_int64), ("sums_off", c_int64)]


class StepSlot(ctypes.Structure):
    """attwarp_step_slot: one batch of an attwarp_warp_step_fused_slots launch, device pointers."""
    _fields_ = [(n, c_void_p) for n in ("src", "dst", "map_x", "map_y", "steps_in", "map_x_next", "map_y_next", "rows",
                                        "starts", "steps_out")]


class OverlayImage(ctypes.Structure):
    """attwarp_overlay_image: one image of an attwarp_heatmap_overlay call, device pointers in a host array."""
    _fields_ = [("image", c_void_p), ("map", c_void_p), ("out", c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


class PngImage(ctypes.Structure):
    """attwarp_png_image: one image of an attwarp_png_plan call, device pointer in a host array."""
    _fields_ = [("src", c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
                ("pitch", ctypes.c_int32), ("order", ctypes.c_int32), ("filter", ctypes.c_int32)]


class PngDecImage(ctypes.Structure):
    """attwarp_pngdec_image: one file of an attwarp_pngdec_plan call, offsets into the packed stream buffer."""
    _fields_ = [("stream_off", ctypes.c_uint64), ("stream_len", ctypes.c_uint64), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("color_type", ctypes.c_int32), ("mode", ctypes.c_int32), ("order", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PngDecChunk(ctypes.Structure):
    """attwarp_pngdec_chunk: one IDAT chunk's payload in the packed stream buffer and the CRC-32 its file states."""
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("image", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class PngDecHeader(ctypes.Structure):
    """attwarp_pngdec_header: the first bytes of a table written by attwarp_pngdec_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("nchunks", ctypes.c_int32), ("check_crc", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("formats", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64), ("off_images", ctypes.c_uint64), ("off_chunks", ctypes.c_uint64),
                ("crc_pow8", ctypes.c_uint32 * 32), ("idat_crc", ctypes.c_uint32), ("reserved2", ctypes.c_uint32)]


class PngDecFormat(ctypes.Structure):
    """attwarp_pngdec_format: what IHDR and PLTE say besides, parallel to the images of attwarp_pngdec_plan_formats."""
    _fields_ = [("depth", ctypes.c_int32), ("interlace", ctypes.c_int32), ("palette_entries", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("palette", ctypes.c_uint8 * 768)]


class JpegDecImage(ctypes.Structure):
    """attwarp_jpegdec_image: one file of an attwarp_jpegdec_plan call; the tables are the scan's, resolved per component."""
    _fields_ = [("stream_off", ctypes.c_uint64), ("stream_len", ctypes.c_uint64), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("ncomp", ctypes.c_int32), ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("order", ctypes.c_int32), ("qt", ctypes.c_uint16 * 64 * 3),
                ("dc_counts", ctypes.c_uint8 * 16 * 3), ("ac_counts", ctypes.c_uint8 * 16 * 3),
                ("dc_symbols", ctypes.c_uint8 * 256 * 3), ("ac_symbols", ctypes.c_uint8 * 256 * 3)]


class JpegDecLayoutImage(ctypes.Structure):
    """attwarp_jpegdec_layout_image: one file of an attwarp_jpegdec_plan_layouts call, up to four components."""
    _fields_ = [("stream_off", ctypes.c_uint64), ("stream_len", ctypes.c_uint64), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("ncomp", ctypes.c_int32), ("h", ctypes.c_int32 * 4), ("v", ctypes.c_int32 * 4), ("color", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("mode", ctypes.c_int32), ("order", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("qt", ctypes.c_uint16 * 64 * 4), ("dc_counts", ctypes.c_uint8 * 16 * 4), ("ac_counts", ctypes.c_uint8 * 16 * 4),
                ("dc_symbols", ctypes.c_uint8 * 256 * 4), ("ac_symbols", ctypes.c_uint8 * 256 * 4)]


class JpegDecScan(ctypes.Structure):
    """attwarp_jpegdec_scan: one scan of a progressive file of an attwarp_jpegdec_plan_scans call."""
    _fields_ = [("image", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("comp", ctypes.c_int32 * 3), ("ss", ctypes.c_int32),
                ("se", ctypes.c_int32), ("ah", ctypes.c_int32), ("al", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("stream_off", ctypes.c_uint64), ("counts", ctypes.c_uint8 * 16 * 3), ("symbols", ctypes.c_uint8 * 256 * 3)]


class JpegDecLayoutScan(ctypes.Structure):
    """attwarp_jpegdec_layout_scan: one scan of a file of an attwarp_jpegdec_plan_layout_scans call."""
    _fields_ = [("image", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("comp", ctypes.c_int32 * 4), ("ss", ctypes.c_int32),
                ("se", ctypes.c_int32), ("ah", ctypes.c_int32), ("al", ctypes.c_int32), ("sequential", ctypes.c_int32),
                ("restart_interval", ctypes.c_int32), ("stream_off", ctypes.c_uint64),
                ("dc_counts", ctypes.c_uint8 * 16 * 4), ("ac_counts", ctypes.c_uint8 * 16 * 4),
                ("dc_symbols", ctypes.c_uint8 * 256 * 4), ("ac_symbols", ctypes.c_uint8 * 256 * 4)]


class JpegDecHeader(ctypes.Structure):
    """attwarp_jpegdec_header: the first bytes of a table written by attwarp_jpegdec_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("total_units", ctypes.c_int32), ("idct_tiles", ctypes.c_int32),
                ("color_tiles", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64),
                ("stream_bytes", ctypes.c_uint64), ("off_images", ctypes.c_uint64)]


class PanelSource(ctypes.Structure):
    """attwarp_panel_source: one row source of an attwarp_panel_grid call, device pointer in a host array."""
    _fields_ = [("data", c_void_p), ("batch_stride", c_int64), ("kind", ctypes.c_int32), ("C", ctypes.c_int32),
                ("N", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("clamp", ctypes.c_int32)]


class JpegEncImage(ctypes.Structure):
    """attwarp_jpegenc_image: one image of an attwarp_jpegenc_plan call, device pointer in a host array."""
    _fields_ = [("src", c_void_p)] + [(n, ctypes.c_int32) for n in ("H", "W", "C", "pitch", "order", "quality", "subsampling",
                                                                   "restart_rows")]


class JpegEncHeader(ctypes.Structure):
    """attwarp_jpegenc_header: the first bytes of a table written by attwarp_jpegenc_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("nunits", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64),
                ("off_images", ctypes.c_uint64), ("off_units", ctypes.c_uint64), ("off_huffman", ctypes.c_uint64),
                ("off_image_out", ctypes.c_uint64), ("off_optimize", ctypes.c_uint64)]


class PngHeader(ctypes.Structure):
    """attwarp_png_header: the first bytes of a table written by attwarp_png_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("nseg", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("scratch_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64),
                ("off_images", ctypes.c_uint64), ("off_segs", ctypes.c_uint64),
                ("crc_pow8", ctypes.c_uint32 * 32), ("idat_head_crc", ctypes.c_uint32), ("reserved2", ctypes.c_uint32)]


class RaggedHeader(ctypes.Structure):
    """attwarp_ragged_header: the first bytes of a table written by attwarp_ragged_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("g", ctypes.c_int32),
                ("H_out", ctypes.c_int32), ("W_out", ctypes.c_int32),
                ("nL", ctypes.c_int32), ("nP", ctypes.c_int32), ("nR", ctypes.c_int32), ("nplans", ctypes.c_int32),
                ("rows_per_block", ctypes.c_int32), ("blocks_per_image", ctypes.c_int32), ("kd", ctypes.c_int32),
                ("max_hw", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("mota_bytes", ctypes.c_uint64), ("sums_bytes", ctypes.c_uint64),
                ("lds_bytes", ctypes.c_uint64), ("off_images", ctypes.c_uint64), ("off_plans", ctypes.c_uint64),
                ("off_lmap", ctypes.c_uint64), ("off_pmap", ctypes.c_uint64), ("off_order", ctypes.c_uint64)]


class PrepHeader(ctypes.Structure):
    """attwarp_prep_header: the first bytes of a table written by attwarp_prep_images_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("S_h", ctypes.c_int32),
                ("S_w", ctypes.c_int32), ("n_fused_images", ctypes.c_int32), ("n_fused_items", ctypes.c_int32),
                ("n_split_images", ctypes.c_int32), ("n_h_items", ctypes.c_int32), ("n_v_items", ctypes.c_int32),
                ("ks", ctypes.c_int32), ("n_wide_items", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("tmp_bytes", ctypes.c_uint64), ("lds_bytes", ctypes.c_uint64),
                ("off_images", ctypes.c_uint64), ("off_items", ctypes.c_uint64)]


class ClipImage(ctypes.Structure):
    """attwarp_clip_image (include/attwarp.h): one image of a ragged CLIP batch, device pointers in a host array."""
    _fields_ = [("image", c_void_p), ("bounds_x", c_void_p), ("kk_x", c_void_p), ("bounds_y", c_void_p), ("kk_y", c_void_p)] + \
               [(n, ctypes.c_int32) for n in ("H", "W", "ksize_x", "ksize_y", "pad_x", "pad_y", "canvas_w", "canvas_h", "nw", "nh",
                                              "left", "top", "vertical_first", "reserved")]


class ClipHeader(ctypes.Structure):
    """attwarp_clip_header: the first bytes of a table written by attwarp_clip_images_plan."""
    _fields_ = [("magic", ctypes.c_uint32), ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("size", ctypes.c_int32),
                ("n_fused_images", ctypes.c_int32), ("n_fused_items", ctypes.c_int32), ("n_wide_items", ctypes.c_int32),
                ("n_split_images", ctypes.c_int32), ("n_h_items", ctypes.c_int32), ("n_v_items", ctypes.c_int32),
                ("ks", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("table_bytes", ctypes.c_uint64), ("tmp_bytes", ctypes.c_uint64), ("lds_bytes", ctypes.c_uint64),
                ("off_images", ctypes.c_uint64), ("off_items", ctypes.c_uint64)]


class AdamWTensor(ctypes.Structure):
    """attwarp_adamw_tensor: one parameter of an optimiser step, device pointers in a host array."""
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("numel", c_int64),
                ("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
                ("step_slot", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_lib = None            # the library every call goes to: the product, or the tuning flavour inside debug_override()
_product = None
_tuning = None


class AttWarpError(RuntimeError):
    """A libattwarp_hip.so entry point returned a negative status."""


def _open(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load (once) and return the ctypes handle.  Fails loudly if the library is missing."""
    global _lib, _product
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"attwarp_amd: HIP library not built ({LIB_PATH} missing). Run `python __graft_entry__.py` or "
            f"`make -C attwarp_amd/csrc`. There is no CPU fallback.")
    _product = _open(LIB_PATH)
    _lib = _product
    return _lib


def load_tuning():
    """The tuning flavour (test / measurement only): same kernels, plus attwarp_debug_set()."""
    global _tuning
    if _tuning is None:
        if not os.path.exists(TUNING_LIB_PATH):
            raise ImportError(f"attwarp_amd: tuning library not built ({TUNING_LIB_PATH} missing); run `make -C attwarp_amd/csrc`")
        _tuning = _open(TUNING_LIB_PATH)
        _tuning.attwarp_debug_set.restype = c_int
        _tuning.attwarp_debug_set.argtypes = [c_char_p, c_int, ctypes.POINTER(c_int)]
        _tuning.attwarp_debug_stream_copy.restype = c_int
        _tuning.attwarp_debug_stream_copy.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]
    return _tuning


def call(name: str, *args):
    """Invoke an int-returning entry point; raise AttWarpError on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.attwarp_last_error().decode("utf-8", "replace")
        raise AttWarpError(f"{name} failed ({rc}): {msg}")


@contextlib.contextmanager
def debug_override(**settings: int):
    """Test / measurement hook: run the calls inside the context on the TUNING flavour of the library with kernel
    variants forced through ``attwarp_debug_set`` -- e.g. ``with debug_override(remap_variant=1): ...`` runs the generic
    gather kernel.  On exit every key gets back the value it had before (nesting works) and calls go to the product
    library again.  Process wide and single threaded: do not use it while other threads launch kernels."""
    global _lib
    load()
    tl = load_tuning()
    outer, _lib = _lib, tl
    prev = {}
    try:
        for k, v in settings.items():
            old = c_int(-1)
            rc = tl.attwarp_debug_set(k.encode(), int(v), ctypes.byref(old))
            if rc != 0:
                raise AttWarpError(f"attwarp_debug_set failed ({rc}): {tl.attwarp_last_error().decode('utf-8', 'replace')}")
            prev[k] = old.value
        yield
    finally:
        for k, v in prev.items():
            tl.attwarp_debug_set(k.encode(), int(v), None)
        _lib = outer


def remap_plan(B: int, C: int, H: int, W: int, H_out: int, W_out: int, mode: str = "cv2", channels_last: bool = True):
    """Test / measurement hook (tuning flavour, no GPU needed): what the float32 staged resample would launch for 16-byte
    aligned images of this shape, under the overrides in force -- ``{"rows", "cpw", "group", "stream"}`` (output rows per
    block, row blocks per workgroup, XCD group, 1 when the launch takes the streaming variant: nontemporal stores),
    or None when the request takes the generic gather kernel."""
    tl = load_tuning()
    key = "remap_plan:%d,%d,%d,%d,%d,%d,%d,%d" % (0 if channels_last else 1, {"exact": 0, "cv2": 1}[mode], B, C, H, W, H_out, W_out)
    packed = c_int(-1)
    rc = tl.attwarp_debug_set(key.encode(), 0, ctypes.byref(packed))
    if rc != 0:
        raise AttWarpError(f"attwarp_debug_set failed ({rc}): {tl.attwarp_last_error().decode('utf-8', 'replace')}")
    v = packed.value
    return None if v < 0 else {"rows": v & 255, "cpw": (v >> 8) & 255, "group": (v >> 16) & 255, "stream": (v >> 24) & 1}


def ptr(t: torch.Tensor | None):
    return None if t is None else c_void_p(t.data_ptr())


def dtype_id(t: torch.Tensor) -> int:
    try:
        return _DTYPE_IDS[t.dtype]
    except KeyError:
        raise TypeError(f"attwarp_amd: unsupported dtype {t.dtype}") from None


def require_gpu(*tensors: torch.Tensor) -> torch.device:
    """All tensors must live on the same GPU; returns it.  No CPU path exists."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "attwarp_amd: tensor is on %s; the HIP kernels need a GPU tensor (there is no CPU fallback)" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"attwarp_amd: tensors on different devices ({dev} vs {t.device})")
    if dev is None:
        raise RuntimeError("attwarp_amd: no tensor given")
    return dev


def needs_grad(*tensors) -> bool:
    """True when autograd has to see through the call (grad mode on and some input requires grad).  The training-time
    call sites of the reference (``net(...)`` and ``upsample_pdf_right_inverse(px_s, ...)`` on the loss path,
    MN/trainer.py:210-260) then take a differentiable route: an autograd.Function whose forward and backward are HIP
    kernels (MarginalNet's FiLM tail and safe_softmax, the losses, the right inverse), or, for inputs those kernels do
    not cover (documented per function), the same formula on stock PyTorch-ROCm ops on the same GPU."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def stream_ptr(dev: torch.device):
    """The caller's current HIP stream on `dev` (kernels are stream ordered, never synchronise)."""
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("attwarp_amd: no GPU visible; the numpy-facing entry points run their kernels on cuda:0 "
                           "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())
