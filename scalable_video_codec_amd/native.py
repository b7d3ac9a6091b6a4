"""ctypes binding of the C ABI (include/svc_hip.h) for the Python harness.

PyTorch is used for device memory and streams only; every computation below runs
in the hand-written HIP kernels of csrc/ through libsvc_hip.so.  There is no
fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libsvc_hip.so")
MOTION_LIB_PATH = os.path.join(PKG, "libsvc_motion.so")

SVC_OK, SVC_ERR_INVALID_ARG, SVC_ERR_UNSUPPORTED, SVC_ERR_HIP, SVC_ERR_NO_DEVICE = range(5)
HBMA_AUTO, HBMA_FORCE_WAVE_PER_BLOCK, HBMA_FORCE_FUSED, HBMA_FORCE_TILED, HBMA_FORCE_LANE = 0, 1, 2, 4, 8


class SvcError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"svc_hip status {status}: {message}")
        self.status = status


class RansacParams(C.Structure):
    _fields_ = [("subset_sz", C.c_uint32), ("inlier_thresh", C.c_float),
                ("success_prob", C.c_float), ("inlier_ratio", C.c_float)]


class SegmentParams(C.Structure):
    _fields_ = [("morph_rect_w", C.c_uint32), ("morph_rect_h", C.c_uint32), ("cluster_count", C.c_uint32),
                ("attempt_count", C.c_uint32), ("max_iter_count", C.c_uint32), ("epsilon", C.c_float),
                ("connectivity", C.c_uint32)]


class StepPair(C.Structure):  # svc_step_pair: one entry of a rate-control ladder
    _fields_ = [("fg_step", C.c_uint32), ("bg_step", C.c_uint32)]


class WireHeader(C.Structure):  # libs/codec.hpp:8-17
    _fields_ = [(n, C.c_uint32) for n in ("frame_count", "frame_w", "frame_h", "frame_excess_w", "frame_excess_h",
                                          "transform_block_w", "transform_block_h", "channel_count")]


# apps/encoder.cpp:47-56
DEFAULT_SEGMENT = dict(morph_rect_w=3, morph_rect_h=3, cluster_count=10, attempt_count=3, max_iter_count=10,
                       epsilon=1.0, connectivity=4)

_vp = C.c_void_p
_u32, _u64 = C.c_uint32, C.c_uint64

# name -> (restype, argtypes); mirrors include/svc_hip.h one to one
SIGNATURES = {
    "svc_hip_last_error": (C.c_char_p, []),
    "svc_hip_abi_version": (C.c_int, []),
    "svc_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "svc_hip_tune_host_allocator": (C.c_int, [_u32]),
    "svc_hip_host_tuning_requested": (C.c_int, []),
    "svc_hip_pyramid_bytes": (_u64, [_u32, _u32, _u32]),
    "svc_hip_hbma_pairs": (C.c_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32, _vp]),
    "svc_hip_hbma_kernel_name": (C.c_char_p, [_u32, _u32, _u32, _u32, _u32, _u32, _u32]),
    "svc_hip_ebma_pairs": (C.c_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "svc_hip_ransac_iter_count": (_u32, [RansacParams]),
    "svc_hip_ransac_frames": (C.c_int, [_vp, _u32, _u32, RansacParams, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "svc_hip_ransac_frames_ex": (C.c_int, [_vp, _u32, _u32, RansacParams, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp]),
    "svc_hip_ransac_rmse_frames": (C.c_int, [_vp, _u32, _u32, RansacParams, _vp, _vp, _vp, _vp, _vp]),
    "svc_hip_segment_frames_ex": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, SegmentParams, _u64, _vp, _u64, _vp, _u32, _vp]),
    "svc_hip_block_types_frames": (C.c_int, [_vp, _u32, _u32, _vp, _vp]),
    "svc_hip_probe_stream": (C.c_int, [_vp, _vp, _u64, _u32, _u32, _vp]),
    "svc_hip_segment_workspace_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "svc_hip_segment_frames": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, SegmentParams, _u64, _vp, _u64, _vp, _vp]),
    "svc_hip_wire_header": (C.c_int, [_u32] * 8 + [C.POINTER(WireHeader)]),
    "svc_hip_serialized_frame_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "svc_hip_serialize_frames": (C.c_int, [_vp, _u64, _u32, _vp] + [_u32] * 8 + [_vp, _u64, _vp]),
    "svc_hip_dct_records_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp]),
    "svc_hip_decode_frames": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp] + [_u32] * 8 + [_vp, _vp]),
    "svc_hip_sse_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 5 + [_vp, _vp]),
    "svc_hip_dct_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "svc_hip_dct_quant_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "svc_hip_quant": (C.c_int, [_vp, _u64, _u32, _vp]),
    "svc_hip_quant_frames": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _vp]),
    "svc_hip_luma_pyramid_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp]),
    "svc_hip_pyramid_levels_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _vp]),
    "svc_hip_dct_records_luma_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _u64, _vp]),
    "svc_hip_wire_patch_types_frames": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, C.c_int, _vp]),
    "svc_hip_dct_quant_luma_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u64, _vp]),
    "svc_hip_dct_redo_workspace_bytes": (_u64, [_u32, _u32, _u32, _u32, _u32]),
    "svc_hip_count_foreground": (C.c_int, [_vp, _u64, _vp, _vp]),
    "svc_hip_dct_quant_redo_frames": (C.c_int, [_vp, _u64, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp]),
    "svc_hip_hbma_host": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _u32]),
    "svc_hip_ebma_host": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "svc_hip_ransac_host": (C.c_int, [_vp, _u32, RansacParams, _vp, _u32, _vp, _vp, _vp, _vp]),
    "svc_hip_dct_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp]),
    "svc_hip_dct_quant_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u32, _vp]),
    "svc_hip_quant_host": (C.c_int, [_vp, _u64, _u32]),
    "svc_hip_global_ebma_workspace_bytes": (_u64, [_u32, _u32]),
    "svc_hip_global_ebma_pairs": (C.c_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_global_avg_frames": (C.c_int, [_vp, _u32, _u32, _vp, _vp]),
    "svc_hip_global_ebma_host": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "svc_hip_global_hbma_host": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    "svc_hip_global_avg_host": (C.c_int, [_vp, _u32, _vp]),
    "svc_hip_comm_available": (C.c_int, []),
    "svc_hip_comm_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int32)]),
    "svc_hip_comm_unique_id": (C.c_int, [_vp]),
    "svc_hip_comm_create": (C.c_int, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "svc_hip_comm_destroy": (C.c_int, [_vp]),
    "svc_hip_halo_shift": (C.c_int, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    # round 4: the per-call image operations behind compat/opencv2/ (host pointers)
    "svc_hip_dct_planes_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, C.POINTER(_vp)]),
    "svc_hip_bgr2yuv_host": (C.c_int, [_vp, _u32, _u32, _vp]),
    "svc_hip_build_pyramid_host": (C.c_int, [_vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "svc_hip_morph_rect_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp]),
    "svc_hip_kmeans_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _u32, C.c_float, _u64, _vp, C.POINTER(C.c_double)]),
    "svc_hip_connected_components_host": (C.c_int, [_vp, _u32, _u32, _u32, _vp, C.POINTER(_u32)]),
    "svc_hip_dct_tiles_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _u32]),
    # the compact quantised-coefficient stream (csrc/levels.hip)
    "svc_hip_levels_max_bytes": (_u64, [_u32] * 7),
    "svc_hip_pack_levels_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_pack_levels_frames": (C.c_int, [_vp, _vp] + [_u32] * 9 + [_vp, _u64, _vp, _u64, _vp, _vp]),
    "svc_hip_unpack_levels_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 7 + [_vp, _u64, _vp, _vp, _vp, _vp]),
    "svc_hip_dct_pack_levels_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_dct_pack_levels_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 4 + [_vp, _u64, _vp, _u64, _vp, _vp]),
    "svc_hip_dct_pack_delta_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_dct_pack_delta_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 4 + [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "svc_hip_dct_pack_delta_auto_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_dct_pack_delta_auto_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 4 +
                                           [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "svc_hip_levels_drain": (C.c_int, [_vp, _vp] + [_u32] * 7 + [_vp, _u64, _vp]),
    # its lossless entropy coding, "SVCE" (csrc/entropy.hip; the drain in csrc/levels.hip)
    "svc_hip_entropy_max_bytes": (_u64, [_u32] * 7),
    "svc_hip_entropy_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_entropy_encode_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 7 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_entropy_decode_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 7 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_entropy_drain": (C.c_int, [_vp, _vp] + [_u32] * 7 + [_vp, _u64, _vp]),
    # the same with rate control, still without planes (csrc/dct_pack.hip)
    "svc_hip_dct_pack_levels_budget_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_levels_budget_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 2 + [C.POINTER(StepPair), _u32, _vp, _vp, _u64,
                                                        _vp, _u64, _vp, _vp, _vp]),
    # its rate control: per-frame steps from a byte budget (csrc/levels.hip)
    "svc_hip_pack_levels_budget_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_pack_levels_budget_frames": (C.c_int, [_vp, _vp] + [_u32] * 7 + [C.POINTER(StepPair), _u32, _vp, _vp, _u64, _vp, _u64, _vp,
                                                                             _vp, _vp]),
    # its decoder (csrc/levels.hip) and the gaze rule
    "svc_hip_decode_levels_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_decode_levels_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 9 + [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    "svc_hip_decode_levels_reduced_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 10 + [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    "svc_hip_decode_entropy_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_decode_entropy_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 9 + [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    "svc_hip_gaze_rect": (C.c_int, [_u32] * 8 + [C.POINTER(_u32)]),
    # two layers: a base and an enhancement stream from one transform, and their decode under a gaze (host statement: layers.py)
    "svc_hip_dct_pack_layers_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_dct_pack_layers_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 5 + [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp,
                                                _vp]),
    "svc_hip_pack_layers_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_pack_layers_frames": (C.c_int, [_vp, _vp] + [_u32] * 10 + [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "svc_hip_decode_layers_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_decode_layers_frames": (C.c_int, [_vp, _u64, _vp, _vp, _u64, _vp] + [_u32] * 9 + [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    "svc_hip_decode_layers_reduced_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_decode_layers_reduced_frames": (C.c_int, [_vp, _u64, _vp, _vp, _u64, _vp] + [_u32] * 10
                                             + [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _vp]),
    # a stored SVCQ stream restricted to a window per output frame (csrc/levels.hip; host statement: layers.window_frames)
    "svc_hip_window_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_window_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp] + [_u32] * 7 + [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    # a stored SVCQ stream restricted to a frequency band (and a window) per output frame, and two such streams joined back (csrc/levels.hip;
    # host statements: layers.band_frames, layers.union_frames)
    "svc_hip_band_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_band_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp] + [_u32] * 7 + [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_union_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_union_levels_frames": (C.c_int, [_vp, _u64, _vp, _vp, _u64, _vp] + [_u32] * 7 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    # an SVCQ stream coded frame against frame in levels, and back (csrc/levels.hip; host statements: layers.delta_frames,
    # layers.undelta_frames)
    "svc_hip_delta_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_delta_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 6 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_undelta_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_undelta_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 6 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    # a delta stream straight to display frames: the undelta and the decode in one call (csrc/levels.hip)
    "svc_hip_decode_delta_levels_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_decode_delta_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 8 + [_vp, _vp, _u64, _vp, _vp, _u32, _u32,
                                                     _vp, _u64, _vp, _vp, _vp]),
    # the three calls above with temporal layers: frame i coded against frame i - min(lowbit(i), period) (csrc/levels.hip; host
    # statements: layers.delta_temporal_frames, layers.undelta_temporal_frames)
    "svc_hip_delta_levels_temporal_workspace_bytes": (_u64, [_u32] * 8),
    "svc_hip_delta_levels_temporal_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 6 +
                                             [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _u32]),
    "svc_hip_undelta_levels_temporal_workspace_bytes": (_u64, [_u32] * 8),
    "svc_hip_undelta_levels_temporal_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 6 +
                                               [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _u32]),
    "svc_hip_decode_delta_levels_temporal_workspace_bytes": (_u64, [_u32] * 8),
    "svc_hip_decode_delta_levels_temporal_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 8 +
                                                    [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _u32]),
    # ... at reduced size: the undelta and the reduced decode in one call, on the first K x K levels of every tile (csrc/levels.hip)
    "svc_hip_decode_delta_levels_reduced_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_decode_delta_levels_reduced_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 9 +
                                                   [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp]),
    # a stored SVCE stream restricted to a window per output frame, on its coded bytes (csrc/entropy.hip; host statement: entropy.window_frames)
    "svc_hip_window_entropy_max_bytes": (_u64, [_u32] * 7),
    "svc_hip_window_entropy_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_window_entropy_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp] + [_u32] * 7 + [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    # a stored fine SVCQ stream split into a base at any steps plus its enhancement (csrc/levels.hip; host statement: layers.split_frames)
    "svc_hip_split_levels_workspace_bytes": (_u64, [_u32] * 8),
    "svc_hip_split_levels_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp] + [_u32] * 10 + [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_split_levels_budget_workspace_bytes": (_u64, [_u32] * 9),
    "svc_hip_split_levels_budget_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp] + [_u32] * 8 + [C.POINTER(StepPair), _u32, _vp, _vp, _vp, _u64,
                                                     _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    # the wire stream's decoder (csrc/records.hip) and its reading of a whole stream
    "svc_hip_decode_records_frames": (C.c_int, [_vp, _u64] + [_u32] * 7 + [_vp, _vp, _vp, _u32, _u32, _vp]),
    "svc_hip_wire_layout": (C.c_int, [C.POINTER(WireHeader), _u64, C.POINTER(_u32), C.POINTER(_u64)]),
    # wire records <-> the compact stream, stream to stream (csrc/levels.hip; numpy statement: wire.py)
    "svc_hip_records_pack_levels_workspace_bytes": (_u64, [_u32] * 6),
    "svc_hip_records_pack_levels_frames": (C.c_int, [_vp, _u64] + [_u32] * 9 + [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "svc_hip_levels_records_workspace_bytes": (_u64, [_u32] * 5),
    "svc_hip_levels_records_frames": (C.c_int, [_vp, _u64, _vp] + [_u32] * 8 + [_vp, _u64, _vp, _u64, _vp, _vp]),
}

# The calls of include/svc_hip_temporal.h: a table of its own because SIGNATURES is tied one to one to the declarations of include/svc_hip.h
# (tests/test_abi.py); load() applies both.
SIGNATURES_TEMPORAL = {
    # the temporal-layer delta stream straight from the transform (csrc/dct_pack.hip; host statement: layers.delta_temporal_frames of the
    # fused pack's frames), and the same with the key frames chosen by size (layers.delta_auto_frames with period)
    "svc_hip_dct_pack_delta_temporal_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_delta_temporal_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 4 + [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp,
                                                        _vp, _u32]),
    "svc_hip_dct_pack_delta_temporal_auto_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_delta_temporal_auto_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 4 + [_vp, _vp, _vp, _vp, _u64, _vp, _u64,
                                                             _vp, _vp, _vp, _vp, _u32]),
}

# The calls of include/svc_hip_temporal_decode.h: a table of its own for the same reason (SIGNATURES_TEMPORAL is tied one to one to
# include/svc_hip_temporal.h by tests/test_dct_pack_delta_temporal_host.py); load() applies all three.
SIGNATURES_TEMPORAL_DECODE = {
    # the temporal-layer delta stream straight to display frames at reduced size (csrc/levels.hip; host statement:
    # layers.undelta_temporal_frames + levels.decode_reduced_frame)
    "svc_hip_decode_delta_levels_temporal_reduced_workspace_bytes": (_u64, [_u32] * 8),
    "svc_hip_decode_delta_levels_temporal_reduced_frames": (C.c_int, [_vp, _u64, _vp, _u32, _vp, _u64, _vp] + [_u32] * 9 +
                                                            [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _u32]),
}

# The calls of include/svc_hip_quality.h: a table of its own for the same reason; load() applies all four.
SIGNATURES_QUALITY = {
    # the fused pack with a distortion target per frame, optionally capped by a byte budget (csrc/dct_pack.hip; host statements:
    # layers.distortion_table, layers.quality_choice)
    "svc_hip_dct_pack_levels_quality_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_levels_quality_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 2 + [C.POINTER(StepPair), _u32, _vp, _vp, _vp,
                                                         _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
}

# The calls of include/svc_hip_delta_budget.h: a table of its own for the same reason; load() applies all five.
SIGNATURES_DELTA_BUDGET = {
    # the delta stream with one ladder entry per group of frames, by a byte budget on the group (csrc/dct_pack.hip; host statements:
    # layers.delta_ladder_counts, layers.delta_budget_choice, layers.delta_budget_frames)
    "svc_hip_dct_pack_delta_budget_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_delta_budget_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 2 + [C.POINTER(StepPair), _u32, _vp, _vp, _vp,
                                                       _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
}

# The calls of include/svc_hip_delta_quality.h: a table of its own for the same reason; load() applies all six.
SIGNATURES_DELTA_QUALITY = {
    # the delta stream with one ladder entry per group of frames, by a distortion target on every frame of the group and an optional byte
    # budget on the group (csrc/dct_pack.hip; host statements: layers.delta_quality_choice, layers.delta_quality_frames)
    "svc_hip_dct_pack_delta_quality_workspace_bytes": (_u64, [_u32] * 7),
    "svc_hip_dct_pack_delta_quality_frames": (C.c_int, [_vp, _u64] + [_u32] * 4 + [_vp] + [_u32] * 2 + [C.POINTER(StepPair), _u32, _vp, _vp, _vp, _vp,
                                                        _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Loads libsvc_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `python -m scalable_video_codec_amd.build` "
                "(or __graft_entry__.build()); the MI355X path has no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(SIGNATURES_TEMPORAL.items()) + list(SIGNATURES_TEMPORAL_DECODE.items()) +
                                  list(SIGNATURES_QUALITY.items()) + list(SIGNATURES_DELTA_BUDGET.items()) +
                                  list(SIGNATURES_DELTA_QUALITY.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _check(rc: int) -> None:
    if rc != SVC_OK:
        raise SvcError(rc, load().svc_hip_last_error().decode())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _bwbh(block) -> Tuple[int, int]:
    """A transform block given as one side (square) or as (block_w, block_h)."""
    return (block, block) if isinstance(block, int) else (int(block[0]), int(block[1]))


def _dev(t: torch.Tensor, dtype) -> int:
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype, (t.device, t.dtype, t.is_contiguous())
    return t.data_ptr()


def ransac_iter_count(subset_sz=1, inlier_thresh=7.5, success_prob=0.99, inlier_ratio=0.5) -> int:
    return int(load().svc_hip_ransac_iter_count(RansacParams(subset_sz, inlier_thresh, success_prob, inlier_ratio)))


def pyramid_bytes(w: int, h: int, levels: int) -> int:
    return int(load().svc_hip_pyramid_bytes(w, h, levels))


def pyramid_stride(w: int, h: int, levels: int) -> int:
    """Packed-pyramid stride used by the harness: rounded up to 256 B."""
    return (pyramid_bytes(w, h, levels) + 255) // 256 * 256


# ---- device-resident, batched ---------------------------------------------------

def hbma_pairs(tracked: torch.Tensor, anchor: torch.Tensor, pair_stride: int, n_pairs: int,
               levels: int, w: int, h: int, search_range: int, block_w: int = 16, block_h: int = 16,
               flags: int = HBMA_AUTO, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """tracked/anchor: u8 CUDA tensors whose data_ptr is pair 0's packed pyramid."""
    blocks = (w // block_w) * (h // block_h)
    if out is None:
        mv = torch.empty((n_pairs, blocks, 2), dtype=torch.float32, device=tracked.device)
        mad = torch.empty((n_pairs, blocks), dtype=torch.float32, device=tracked.device)
    else:
        mv, mad = out
    _check(load().svc_hip_hbma_pairs(_dev(tracked, torch.uint8), _dev(anchor, torch.uint8), pair_stride, n_pairs,
                                     levels, w, h, search_range, block_w, block_h,
                                     _dev(mv, torch.float32), _dev(mad, torch.float32), flags, _stream()))
    return mv, mad


def hbma_kernel_name(levels: int, w: int, h: int, search_range: int, block_w: int = 16, block_h: int = 16,
                     flags: int = HBMA_AUTO) -> str:
    """The kernel hbma_pairs launches for this shape and these flags (aligned pyramids); no GPU work."""
    name = load().svc_hip_hbma_kernel_name(levels, w, h, search_range, block_w, block_h, flags)
    if name is None:  # invalid parameters (the asserts of motion.cpp:417-433) or a forced kernel that does not cover the shape
        msg = load().svc_hip_last_error().decode()
        raise SvcError(SVC_ERR_UNSUPPORTED if "does not cover" in msg else SVC_ERR_INVALID_ARG, msg)
    return name.decode()


def ebma_pairs(tracked: torch.Tensor, anchor: torch.Tensor, pair_stride: int, n_pairs: int, w: int, h: int,
               search_range: int, block_w: int, block_h: int):
    blocks = (w // block_w) * (h // block_h)
    mv = torch.empty((n_pairs, blocks, 2), dtype=torch.float32, device=tracked.device)
    mad = torch.empty((n_pairs, blocks), dtype=torch.float32, device=tracked.device)
    _check(load().svc_hip_ebma_pairs(_dev(tracked, torch.uint8), _dev(anchor, torch.uint8), pair_stride, n_pairs,
                                     w, h, search_range, block_w, block_h,
                                     _dev(mv, torch.float32), _dev(mad, torch.float32), _stream()))
    return mv, mad


LAUNCH_BESIDE = 1
LAUNCH_NO_FORK = 2  # segmentation keeps its heavy attempts on the caller's stream (include/svc_hip.h)


def ransac_frames(mv: torch.Tensor, samples: torch.Tensor, gm_in: Optional[torch.Tensor] = None,
                  subset_sz=1, inlier_thresh=7.5, success_prob=0.99, inlier_ratio=0.5, out=None, flags: int = 0):
    """mv: (frames, blocks, 2) f32; samples: (frames, iters, subset) i32/u32 as int32 storage."""
    frames, blocks, _ = mv.shape
    iters = samples.shape[1] if samples.numel() else 0
    if out is None:
        gm = torch.zeros((frames, 2), dtype=torch.float32, device=mv.device) if gm_in is None else gm_in.clone()
        rmse = torch.empty(frames, dtype=torch.float32, device=mv.device)
        mask = torch.empty((frames, blocks), dtype=torch.uint8, device=mv.device)
        count = torch.empty(frames, dtype=torch.int32, device=mv.device)
    else:
        gm, rmse, mask, count = out
    p = RansacParams(subset_sz, inlier_thresh, success_prob, inlier_ratio)
    _check(load().svc_hip_ransac_frames_ex(_dev(mv, torch.float32), blocks, frames, p, _dev(samples, torch.int32),
                                           iters, _dev(gm, torch.float32), _dev(rmse, torch.float32),
                                           _dev(mask, torch.uint8), _dev(count, torch.int32), flags, _stream()))
    return gm, rmse, mask, count


def ransac_rmse_frames(mv: torch.Tensor, gm: torch.Tensor, mask: torch.Tensor, count: torch.Tensor, rmse: torch.Tensor,
                       subset_sz=1, inlier_thresh=7.5, success_prob=0.99, inlier_ratio=0.5) -> torch.Tensor:
    """Completes a ransac_frames(..., flags=LAUNCH_DEFER_RMSE) call: the in-order RMSE over the inliers, in place."""
    frames, blocks = mv.shape[0], mv.shape[1]
    p = RansacParams(subset_sz, inlier_thresh, success_prob, inlier_ratio)
    _check(load().svc_hip_ransac_rmse_frames(_dev(mv, torch.float32), blocks, frames, p, _dev(gm, torch.float32),
                                             _dev(mask, torch.uint8), _dev(count, torch.int32), _dev(rmse, torch.float32), _stream()))
    return rmse


LAUNCH_BESIDE, LAUNCH_NO_FORK, LAUNCH_WIDE, LAUNCH_NO_WIDE, LAUNCH_DEFER_RMSE = 1, 2, 4, 8, 16


def block_types_frames(mask: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask: (frames, blocks) u8 inlier mask -> (frames, blocks) i32 block types (0 = background)."""
    frames, blocks = mask.shape
    if out is None:
        out = torch.empty((frames, blocks), dtype=torch.int32, device=mask.device)
    _check(load().svc_hip_block_types_frames(_dev(mask, torch.uint8), blocks, frames, _dev(out, torch.int32), _stream()))
    return out


def probe_stream(src: torch.Tensor, dst: torch.Tensor, reads: int, writes: int) -> None:
    """One launch of the plain streaming kernel (measurement aid): reads x 16 B in, writes x 16 B out per lane; one 4 KiB unit per workgroup."""
    _check(load().svc_hip_probe_stream(_dev(src, torch.uint8), _dev(dst, torch.uint8), min(src.numel(), dst.numel()),
                                       reads, writes, _stream()))


def segment_workspace_bytes(mfw: int, mfh: int, frames: int, attempts: int = 3) -> int:
    return int(load().svc_hip_segment_workspace_bytes(mfw, mfh, frames, attempts))


def segment_frames(mask: torch.Tensor, mv: torch.Tensor, mfw: int, mfh: int, mv_block: int = 16, seed: int = 0,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, flags: int = 0,
                   **params) -> torch.Tensor:
    """mask (frames, blocks) u8 inlier mask + mv (frames, blocks, 2) f32 -> (frames, blocks) i32 region ids."""
    frames, blocks = mask.shape
    assert blocks == mfw * mfh
    p = SegmentParams(**{**DEFAULT_SEGMENT, **params})
    need = int(load().svc_hip_segment_workspace_bytes(mfw, mfh, frames, p.attempt_count))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=mask.device)
    if out is None:
        out = torch.empty((frames, blocks), dtype=torch.int32, device=mask.device)
    _check(load().svc_hip_segment_frames_ex(_dev(mask, torch.uint8), _dev(mv, torch.float32), mfw, mfh, frames,
                                            mv_block, mv_block, p, seed, _dev(workspace, torch.uint8),
                                            workspace.numel(), _dev(out, torch.int32), flags, _stream()))
    return out


def wire_header(clip_frames: int, w: int, h: int, mv_block: int, levels: int, tb: int) -> bytes:
    hdr = WireHeader()
    _check(load().svc_hip_wire_header(clip_frames, w, h, mv_block, mv_block, levels, tb, tb, C.byref(hdr)))
    return bytes(hdr)


def serialized_frame_bytes(frame_w: int, frame_h: int, tbw: int, tbh: int) -> int:
    return int(load().svc_hip_serialized_frame_bytes(frame_w, frame_h, tbw, tbh))


def serialize_frames(planes: torch.Tensor, block_types: torch.Tensor, frame_w: int, frame_h: int, tbw: int,
                     tbh: int, mfw: int, mfh: int, mv_block: int = 16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """planes (frames, 3, H, W) f32 + types (frames, blocks) i32 -> (frames, bytes) u8, the records of
    libs/encoder.cpp:222-269 for tile loops over frame_w x frame_h (also the row stride, as in the reference)."""
    n, _, ph, pw = planes.shape
    per = serialized_frame_bytes(frame_w, frame_h, tbw, tbh)
    if out is None:
        out = torch.empty((n, per), dtype=torch.uint8, device=planes.device)
    _check(load().svc_hip_serialize_frames(_dev(planes, torch.float32), ph * pw, n, _dev(block_types, torch.int32),
                                           frame_w, frame_h, tbw, tbh, mfw, mfh, mv_block, mv_block,
                                           _dev(out, torch.uint8), out.stride(0), _stream()))
    return out


def dct_records_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block: int = 16,
                       fg_step: int = 0, bg_step: int = 0, emit_h: Optional[int] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bgr (frames, H, W, 3) u8 -> (frames, bytes) u8 serialised records, DCT (+quant) and
    SerializeEncodedFrame in one kernel."""
    n, h, w, _ = bgr.shape
    emit_h = h if emit_h is None else emit_h
    per = serialized_frame_bytes(w, emit_h, block, block)
    if out is None:
        out = torch.empty((n, per), dtype=torch.uint8, device=bgr.device)
    _check(load().svc_hip_dct_records_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                             _dev(block_types, torch.int32), mv_block, mv_block, fg_step, bg_step,
                                             emit_h, _dev(out, torch.uint8), out.stride(0), _stream()))
    return out


def decode_frames(planes: torch.Tensor, block: int, block_types: torch.Tensor, mv_block: int = 16, fg_step: int = 1,
                  bg_step: int = 640, gaze=(0, 0, 0, 0), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Coefficient planes (frames, 3, H, W) f32 -> reconstructed (frames, H, W, 3) f32 B,G,R
    (libs/decoder.cpp:128-149 over every tile)."""
    n, _, h, w = planes.shape
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.float32, device=planes.device)
    _check(load().svc_hip_decode_frames(_dev(planes, torch.float32), n, w, h, block, _dev(block_types, torch.int32),
                                        mv_block, mv_block, fg_step, bg_step, *gaze, _dev(out, torch.float32), _stream()))
    return out


def sse_frames(src_bgr: torch.Tensor, rec: torch.Tensor, region_w: int, region_h: int) -> torch.Tensor:
    """Exact per-frame SSE (int64) of u8 source frames vs an f32 reconstruction rounded to u8."""
    n, h, w, _ = src_bgr.shape
    out = torch.empty(n, dtype=torch.int64, device=src_bgr.device)
    _check(load().svc_hip_sse_frames(_dev(src_bgr, torch.uint8), h * w * 3, _dev(rec, torch.float32), n, w, h,
                                     region_w, region_h, _dev(out, torch.int64), _stream()))
    return out


def dct_frames(bgr: torch.Tensor, block, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bgr: (frames, H, W, 3) u8 -> (frames, 3, H, W) f32 coefficient planes.  block: side or (block_w, block_h)."""
    n, h, w, _ = bgr.shape
    bw, bh = _bwbh(block)
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=bgr.device)
    _check(load().svc_hip_dct_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, bw, bh,
                                     _dev(out, torch.float32), _stream()))
    return out


def dct_quant_frames(bgr: torch.Tensor, block, block_types: torch.Tensor, mv_block: int, fg_step: int,
                     bg_step: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n, h, w, _ = bgr.shape
    bw, bh = _bwbh(block)
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=bgr.device)
    _check(load().svc_hip_dct_quant_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, bw, bh,
                                           _dev(block_types, torch.int32), mv_block, mv_block, fg_step, bg_step,
                                           _dev(out, torch.float32), _stream()))
    return out


def quant_(coeffs: torch.Tensor, step: int) -> torch.Tensor:
    _check(load().svc_hip_quant(_dev(coeffs, torch.float32), coeffs.numel(), step, _stream()))
    return coeffs


def quant_frames_(planes: torch.Tensor, block_types: torch.Tensor, mv_block: int, fg_step: int, bg_step: int):
    n, _, h, w = planes.shape
    _check(load().svc_hip_quant_frames(_dev(planes, torch.float32), n, w, h, mv_block, mv_block,
                                       _dev(block_types, torch.int32), fg_step, bg_step, _stream()))
    return planes


def luma_pyramid_frames(bgr: torch.Tensor, levels: int, out: Optional[torch.Tensor] = None,
                        stride: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """bgr: (frames, H, W, 3) u8 -> (flat u8 buffer of `frames` packed pyramids, stride)."""
    n, h, w, _ = bgr.shape
    stride = pyramid_stride(w, h, levels) if stride is None else stride
    if out is None:
        out = torch.empty(n * stride, dtype=torch.uint8, device=bgr.device)
    _check(load().svc_hip_luma_pyramid_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, levels,
                                              _dev(out, torch.uint8), stride, _stream()))
    return out, stride


def dct_records_luma_frames(bgr: torch.Tensor, block: int, levels: int, emit_h: Optional[int] = None,
                            records: Optional[torch.Tensor] = None, pyr: Optional[torch.Tensor] = None,
                            stride: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """ONE pass over bgr (frames, H, W, 3) u8: the raw-coefficient records (type words 0) AND level 0 of each frame's packed pyramid,
    then the pyramid's other levels from it.  -> (records (frames, bytes) u8, flat pyramid buffer, pyramid stride)."""
    n, h, w, _ = bgr.shape
    emit_h = h if emit_h is None else emit_h
    per = serialized_frame_bytes(w, emit_h, block, block)
    if records is None:
        records = torch.empty((n, per), dtype=torch.uint8, device=bgr.device)
    stride = pyramid_stride(w, h, levels) if stride is None else stride
    if pyr is None:
        pyr = torch.empty(n * stride, dtype=torch.uint8, device=bgr.device)
    _check(load().svc_hip_dct_records_luma_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block, emit_h, _dev(records, torch.uint8),
                                                  records.stride(0), _dev(pyr, torch.uint8), stride, _stream()))
    _check(load().svc_hip_pyramid_levels_frames(_dev(pyr, torch.uint8), stride, n, w, h, levels, _stream()))
    return records, pyr, stride


def pyramid_levels_frames(pyr: torch.Tensor, stride: int, n: int, w: int, h: int, levels: int) -> torch.Tensor:
    """Levels 1 .. levels - 1 of `n` packed pyramids whose level-0 planes are in place (cv::buildPyramid, libs/encoder.cpp:470)."""
    _check(load().svc_hip_pyramid_levels_frames(_dev(pyr, torch.uint8), stride, n, w, h, levels, _stream()))
    return pyr


def dct_quant_luma_frames(bgr: torch.Tensor, block: int, levels: int, bg_step: int = 640, planes: Optional[torch.Tensor] = None,
                          pyr: Optional[torch.Tensor] = None, stride: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """ONE pass over bgr: coefficient planes with EVERY tile quantised as background AND level 0 of each frame's pyramid (then its other
    levels).  -> (planes (frames, 3, H, W) f32, flat pyramid buffer, stride); dct_quant_redo_frames finishes the foreground tiles."""
    n, h, w, _ = bgr.shape
    if planes is None:
        planes = torch.empty((n, 3, h, w), dtype=torch.float32, device=bgr.device)
    stride = pyramid_stride(w, h, levels) if stride is None else stride
    if pyr is None:
        pyr = torch.empty(n * stride, dtype=torch.uint8, device=bgr.device)
    _check(load().svc_hip_dct_quant_luma_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block, bg_step, _dev(planes, torch.float32),
                                                _dev(pyr, torch.uint8), stride, _stream()))
    _check(load().svc_hip_pyramid_levels_frames(_dev(pyr, torch.uint8), stride, n, w, h, levels, _stream()))
    return planes, pyr, stride


def dct_quant_redo_frames(bgr: torch.Tensor, planes: torch.Tensor, block: int, block_types: torch.Tensor, mv_block: int = 16,
                          fg_step: int = 1) -> torch.Tensor:
    """The tiles of every foreground MV block (region id != 0) transformed again and quantised with fg_step, in place."""
    n, h, w, _ = bgr.shape
    nbytes = load().svc_hip_dct_redo_workspace_bytes(n, w, h, mv_block, mv_block)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=bgr.device)
    _check(load().svc_hip_dct_quant_redo_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block, _dev(block_types, torch.int32), mv_block,
                                                mv_block, fg_step, _dev(planes, torch.float32), _dev(ws, torch.uint8), nbytes, _stream()))
    return planes


def count_foreground(block_types: torch.Tensor) -> int:
    """How many of the region ids are not 0."""
    out = torch.zeros(1, dtype=torch.int32, device=block_types.device)
    _check(load().svc_hip_count_foreground(_dev(block_types, torch.int32) if block_types.numel() else None, block_types.numel(),
                                           _dev(out, torch.int32), _stream()))
    return int(out.item())


def wire_patch_types_frames(records: torch.Tensor, block_types: torch.Tensor, w: int, h: int, block: int, mv_block: int = 16,
                            emit_h: Optional[int] = None, all_tiles: bool = False) -> torch.Tensor:
    """Stores the region id of every foreground MV block into the type words of its tiles' records (in place)."""
    n = records.shape[0]
    emit_h = h if emit_h is None else emit_h
    _check(load().svc_hip_wire_patch_types_frames(_dev(block_types, torch.int32), n, w, h, emit_h, block, mv_block, mv_block,
                                                  _dev(records, torch.uint8), records.stride(0), 1 if all_tiles else 0, _stream()))
    return records


# ---- host-pointer forms (numpy in, numpy out): what include/svc/motion.hpp calls ----

def _np_ptr(a):
    return a.ctypes.data_as(_vp)


def hbma_host(tracked_pyr, anchor_pyr, search_range: int, block_w: int = 16, block_h: int = 16,
              flags: int = HBMA_AUTO):
    import numpy as np
    levels = len(tracked_pyr)
    h, w = tracked_pyr[0].shape
    tp = (_vp * levels)(*[_np_ptr(np.ascontiguousarray(p)) for p in tracked_pyr])
    ap = (_vp * levels)(*[_np_ptr(np.ascontiguousarray(p)) for p in anchor_pyr])
    blocks = (w // block_w) * (h // block_h) if block_w and block_h else 0
    mv = np.empty((max(blocks, 1), 2), np.float32)
    mad = np.empty(max(blocks, 1), np.float32)
    _check(load().svc_hip_hbma_host(C.cast(tp, _vp), C.cast(ap, _vp), levels, w, h, search_range, block_w, block_h,
                                    _np_ptr(mv), _np_ptr(mad), flags))
    return mv[:blocks], mad[:blocks]


def ebma_host(tracked, anchor, search_range: int, block_w: int, block_h: int):
    import numpy as np
    h, w = tracked.shape
    blocks = (w // block_w) * (h // block_h)
    mv = np.empty((blocks, 2), np.float32)
    mad = np.empty(blocks, np.float32)
    _check(load().svc_hip_ebma_host(_np_ptr(np.ascontiguousarray(tracked)), _np_ptr(np.ascontiguousarray(anchor)),
                                    w, h, search_range, block_w, block_h, _np_ptr(mv), _np_ptr(mad)))
    return mv, mad


def ransac_host(mv, samples, gm_in=(0.0, 0.0), subset_sz=1, inlier_thresh=7.5, success_prob=0.99,
                inlier_ratio=0.5):
    import numpy as np
    mv = np.ascontiguousarray(mv, np.float32)
    samples = np.ascontiguousarray(samples, np.uint32)
    n = len(mv)
    gm = np.array(gm_in, np.float32)
    rmse = C.c_float(0)
    inl = np.empty(max(n, 1), np.uint32)
    cnt = C.c_uint32(0)
    p = RansacParams(subset_sz, inlier_thresh, success_prob, inlier_ratio)
    iters = samples.size // subset_sz if subset_sz else 0
    _check(load().svc_hip_ransac_host(_np_ptr(mv), n, p, _np_ptr(samples), iters, _np_ptr(gm),
                                      C.cast(C.byref(rmse), _vp), _np_ptr(inl), C.cast(C.byref(cnt), _vp)))
    return gm, np.float32(rmse.value), inl[:cnt.value].copy()


def dct_host(bgr, block):
    import numpy as np
    bgr = np.ascontiguousarray(bgr, np.uint8)
    h, w, _ = bgr.shape
    bw, bh = _bwbh(block)
    out = np.empty((3, h, w), np.float32)
    _check(load().svc_hip_dct_host(_np_ptr(bgr), w, h, bw, bh, _np_ptr(out)))
    return out


def dct_quant_host(bgr, block, block_types, mv_block, fg_step: int, bg_step: int):
    import numpy as np
    bgr = np.ascontiguousarray(bgr, np.uint8)
    bt = np.ascontiguousarray(block_types, np.uint32)
    h, w, _ = bgr.shape
    bw, bh = _bwbh(block)
    mvw, mvh = _bwbh(mv_block)
    out = np.empty((3, h, w), np.float32)
    _check(load().svc_hip_dct_quant_host(_np_ptr(bgr), w, h, bw, bh, _np_ptr(bt), mvw, mvh,
                                         fg_step, bg_step, _np_ptr(out)))
    return out


def quant_host(coeffs, step: int):
    import numpy as np
    out = np.ascontiguousarray(coeffs, np.float32).copy()
    _check(load().svc_hip_quant_host(_np_ptr(out), out.size, step))
    return out


def global_ebma_host(tracked, anchor, search_range: int):
    """EstimateGlobalMotionExhaustiveSearch (libs/motion.hpp:45-49) -> ((dx, dy), min_mad)."""
    import numpy as np
    h, w = tracked.shape
    gm = np.zeros(2, np.float32)
    mad = C.c_float(0)
    _check(load().svc_hip_global_ebma_host(_np_ptr(np.ascontiguousarray(tracked)), _np_ptr(np.ascontiguousarray(anchor)), w, h,
                                           search_range, _np_ptr(gm), C.cast(C.byref(mad), _vp)))
    return gm, np.float32(mad.value)


def global_hbma_host(tracked_pyr, anchor_pyr, search_range: int):
    """EstimateGlobalMotionHierarchical (libs/motion.hpp:55-59) -> (dx, dy)."""
    import numpy as np
    levels = len(tracked_pyr)
    h, w = tracked_pyr[0].shape
    tp = (_vp * levels)(*[_np_ptr(np.ascontiguousarray(p)) for p in tracked_pyr])
    ap = (_vp * levels)(*[_np_ptr(np.ascontiguousarray(p)) for p in anchor_pyr])
    gm = np.zeros(2, np.float32)
    _check(load().svc_hip_global_hbma_host(C.cast(tp, _vp), C.cast(ap, _vp), levels, w, h, search_range, _np_ptr(gm)))
    return gm


def global_avg_host(mv):
    """EstimateGlobalMotionAvg (libs/motion.hpp:38)."""
    import numpy as np
    mv = np.ascontiguousarray(mv, np.float32)
    out = np.zeros(2, np.float32)
    _check(load().svc_hip_global_avg_host(_np_ptr(mv), len(mv), _np_ptr(out)))
    return out


def global_ebma_pairs(tracked: torch.Tensor, anchor: torch.Tensor, pair_stride: int, n_pairs: int, w: int, h: int,
                      search_range: int):
    ws = torch.empty(int(load().svc_hip_global_ebma_workspace_bytes(search_range, n_pairs)), dtype=torch.uint8, device=tracked.device)
    gm = torch.empty((n_pairs, 2), dtype=torch.float32, device=tracked.device)
    mad = torch.empty(n_pairs, dtype=torch.float32, device=tracked.device)
    _check(load().svc_hip_global_ebma_pairs(_dev(tracked, torch.uint8), _dev(anchor, torch.uint8), pair_stride, n_pairs, w, h,
                                            search_range, _dev(ws, torch.uint8), ws.numel(), _dev(gm, torch.float32),
                                            _dev(mad, torch.float32), _stream()))
    return gm, mad


def global_avg_frames(mv: torch.Tensor) -> torch.Tensor:
    frames, blocks, _ = mv.shape
    out = torch.empty((frames, 2), dtype=torch.float32, device=mv.device)
    _check(load().svc_hip_global_avg_frames(_dev(mv, torch.float32), blocks, frames, _dev(out, torch.float32), _stream()))
    return out


# ---- per-call image operations (host numpy arrays in, numpy arrays out): what compat/opencv2/ forwards to ----------
def _np(a, dtype):
    import numpy as np
    return np.ascontiguousarray(a, dtype)


def bgr2yuv_host(bgr):
    import numpy as np
    src = _np(bgr, np.uint8)
    h, w, _ = src.shape
    out = np.empty_like(src)
    _check(load().svc_hip_bgr2yuv_host(src.ctypes.data, w, h, out.ctypes.data))
    return out


def build_pyramid_host(level0, levels: int):
    import numpy as np
    src = _np(level0, np.uint8)
    h, w = src.shape
    planes = [src] + [np.empty((h >> l, w >> l), np.uint8) for l in range(1, levels)]
    ptrs = (_vp * levels)(*[p.ctypes.data for p in planes])
    _check(load().svc_hip_build_pyramid_host(src.ctypes.data, w, h, levels, ptrs))
    return planes


MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3


def morph_rect_host(img, kw: int, kh: int, op: int):
    import numpy as np
    src = _np(img, np.uint8)
    h, w = src.shape
    out = np.empty_like(src)
    _check(load().svc_hip_morph_rect_host(src.ctypes.data, w, h, kw, kh, op, out.ctypes.data))
    return out


def kmeans_host(features, k: int, attempts: int = 3, max_iter: int = 10, epsilon: float = 1.0, seed: int = 0):
    import numpy as np
    f = _np(features, np.float32)
    n, dims = f.shape
    labels = np.empty(n, np.int32)
    compact = C.c_double(0.0)
    _check(load().svc_hip_kmeans_host(f.ctypes.data, n, dims, k, attempts, max_iter, epsilon, seed, labels.ctypes.data,
                                      C.byref(compact)))
    return labels, compact.value


def connected_components_host(img, connectivity: int = 4):
    import numpy as np
    src = _np(img, np.uint8)
    h, w = src.shape
    labels = np.empty((h, w), np.int32)
    count = _u32(0)
    _check(load().svc_hip_connected_components_host(src.ctypes.data, w, h, connectivity, labels.ctypes.data, C.byref(count)))
    return labels, int(count.value)


def dct_tiles_host(image, bw: int, bh: int, tiles_xy=None):
    """In-place cv::dct over the listed tiles (or the whole regular grid) of an f32 image; returns the image."""
    import numpy as np
    img = np.array(image, np.float32, order="C")
    h, w = img.shape
    if tiles_xy is None:
        _check(load().svc_hip_dct_tiles_host(img.ctypes.data, w, h, bw, bh, None, 0))
    else:
        xy = _np(tiles_xy, np.uint32)
        _check(load().svc_hip_dct_tiles_host(img.ctypes.data, w, h, bw, bh, xy.ctypes.data, len(xy)))
    return img


def dct_planes_host(bgr, bw: int, bh: int):
    import numpy as np
    src = _np(bgr, np.uint8)
    h, w, _ = src.shape
    planes = [np.empty((h, w), np.float32) for _ in range(3)]
    ptrs = (_vp * 3)(*[p.ctypes.data for p in planes])
    _check(load().svc_hip_dct_planes_host(src.ctypes.data, w, h, bw, bh, ptrs))
    return np.stack(planes)


# ---- the compact quantised-coefficient stream (include/svc_hip.h, "SVCQ" v1; host reader: levels.py) ----

def levels_max_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Worst-case bytes of n packed frames (what the output and a drain destination must hold)."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_levels_max_bytes(n, w, h, bw, bh, mbw, mbh))


def pack_levels_workspace_bytes(n: int, w: int, h: int, block) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_pack_levels_workspace_bytes(n, w, h, bw, bh))


def pack_levels_frames(planes: torch.Tensor, block_types: torch.Tensor, block, mv_block, fg_step: int, bg_step: int,
                       out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantised planes (frames, 3, H, W) f32 + region ids (frames, blocks) i32 -> (stream u8 of the worst-case size, offsets
    (frames + 1,) i64 on the device; offsets[-1] = bytes used)."""
    n, _, h, w = planes.shape
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=planes.device)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=planes.device)
    if workspace is None:
        workspace = torch.empty(max(pack_levels_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=planes.device)
    _check(load().svc_hip_pack_levels_frames(_dev(planes, torch.float32), _dev(block_types, torch.int32), n, w, h, bw, bh, mbw, mbh,
                                             fg_step, bg_step, _dev(workspace, torch.uint8), workspace.numel(),
                                             _dev(out, torch.uint8), out.numel(), _dev(offsets, torch.int64), _stream()))
    return out, offsets


def dct_pack_levels_workspace_bytes(n: int, w: int, h: int, block: int, mv_block) -> int:
    """Scratch of dct_pack_levels_frames; 0 for a geometry it refuses (then: dct_quant_frames + pack_levels_frames)."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_levels_workspace_bytes(n, w, h, block, mbw, mbh))


def dct_pack_levels_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int,
                           out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """B,G,R frames (frames, H, W, 3) u8 + region ids (frames, blocks) i32 -> the compact stream of dct_quant_frames +
    pack_levels_frames, byte for byte, without the planes: (stream u8 of the worst-case size, offsets (frames + 1,) i64 on the
    device).  8x8 / 16x16 blocks on widths that are multiples of 16; anything else raises (use the two calls)."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_levels_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    _check(load().svc_hip_dct_pack_levels_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                 _dev(block_types, torch.int32), mbw, mbh, fg_step, bg_step,
                                                 _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                 _dev(offsets, torch.int64), _stream()))
    return out, offsets


def dct_pack_delta_workspace_bytes(n: int, w: int, h: int, block: int, mv_block) -> int:
    """Scratch of dct_pack_delta_frames; 0 for a geometry it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_workspace_bytes(n, w, h, block, mbw, mbh))


def dct_pack_delta_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int,
                          prev_bgr: Optional[torch.Tensor] = None, prev_types: Optional[torch.Tensor] = None, key=None,
                          out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """B,G,R frames (frames, H, W, 3) u8 + region ids (frames, blocks) i32 -> the DELTA stream of those frames, byte for byte
    delta_levels_frames of dct_pack_levels_frames' stream, without that stream (include/svc_hip.h): (stream u8 of the worst-case
    size, offsets (frames + 1,) i64 on the device).  The numpy statement is layers.delta_frames applied to the frames of
    dct_pack_levels_frames: there is no other.  prev_bgr (H, W, 3) u8 with prev_types (blocks,) i32: the frame before frame 0 (the
    last input frame of the call before) -- both or neither; neither: frame 0 is a key frame.  key: None, or per frame != 0 for a
    key frame ((frames,) ints, a tensor or a list).  Geometry as dct_pack_levels_frames."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    k = None if key is None else torch.as_tensor(key, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one key flag per frame"
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    _check(load().svc_hip_dct_pack_delta_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                _dev(block_types, torch.int32), mbw, mbh, fg_step, bg_step,
                                                None if prev_bgr is None else _dev(prev_bgr, torch.uint8),
                                                None if prev_types is None else _dev(prev_types, torch.int32),
                                                None if k is None else _dev(k, torch.int32),
                                                _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                _dev(offsets, torch.int64), _stream()))
    return out, offsets


def dct_pack_delta_auto_workspace_bytes(n: int, w: int, h: int, block: int, mv_block) -> int:
    """Scratch of dct_pack_delta_auto_frames; 0 for a geometry it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_auto_workspace_bytes(n, w, h, block, mbw, mbh))


def dct_pack_delta_auto_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int,
                               prev_bgr: Optional[torch.Tensor] = None, prev_types: Optional[torch.Tensor] = None, forced=None,
                               out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                               keys: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                               workspace: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """dct_pack_delta_frames with the key frames chosen by size (include/svc_hip.h, svc_hip_dct_pack_delta_auto_frames): a frame is a
    key frame iff it has no predecessor, forced[f] != 0, or its difference holds at least as many levels as the frame itself ->
    (stream u8 of the worst-case size, offsets (frames + 1,) i64, keys (frames,) i32 0 / 1, counts (frames, 2) i32: the frame's levels
    and its difference's), all on the device.  Stream and offsets are dct_pack_delta_frames' with key = keys; keys and counts are
    layers.auto_keys and layers.delta_level_counts of dct_pack_levels_frames' stream.  forced: None, or per frame != 0 ((frames,) ints,
    a tensor or a list).  prev_bgr / prev_types and the geometry as dct_pack_delta_frames."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    k = None if forced is None else torch.as_tensor(forced, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one forced flag per frame"
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if keys is None:
        keys = torch.empty(n, dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_auto_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    _check(load().svc_hip_dct_pack_delta_auto_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                     _dev(block_types, torch.int32), mbw, mbh, fg_step, bg_step,
                                                     None if prev_bgr is None else _dev(prev_bgr, torch.uint8),
                                                     None if prev_types is None else _dev(prev_types, torch.int32),
                                                     None if k is None else _dev(k, torch.int32),
                                                     _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                     _dev(offsets, torch.int64), _dev(keys, torch.int32), _dev(counts, torch.int32),
                                                     _stream()))
    return out, offsets, keys, counts


def dct_pack_delta_temporal_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, period: int) -> int:
    """Scratch of dct_pack_delta_temporal_frames; 0 for a geometry or a period it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_temporal_workspace_bytes(n, w, h, block, mbw, mbh, period))


def dct_pack_delta_temporal_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int, period: int,
                                   prev_bgr: Optional[torch.Tensor] = None, prev_types: Optional[torch.Tensor] = None, key=None,
                                   out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dct_pack_delta_frames with temporal layers (include/svc_hip_temporal.h): byte for byte delta_levels_temporal_frames of
    dct_pack_levels_frames' stream, without that stream; the numpy statement is layers.delta_temporal_frames applied to the frames of
    dct_pack_levels_frames.  Frame i is coded against input frame i - min(lowbit(i), period), period 1, 2 or 4; prev_bgr / prev_types:
    the input frame at index -period (both or neither; neither: frame 0 is a key frame).  Everything else as dct_pack_delta_frames."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    k = None if key is None else torch.as_tensor(key, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one key flag per frame"
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_temporal_workspace_bytes(n, w, h, block, mv_block, period), 16), dtype=torch.uint8,
                                device=dev)
    _check(load().svc_hip_dct_pack_delta_temporal_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                         _dev(block_types, torch.int32), mbw, mbh, fg_step, bg_step,
                                                         None if prev_bgr is None else _dev(prev_bgr, torch.uint8),
                                                         None if prev_types is None else _dev(prev_types, torch.int32),
                                                         None if k is None else _dev(k, torch.int32),
                                                         _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                         _dev(offsets, torch.int64), _stream(), period))
    return out, offsets


def dct_pack_delta_temporal_auto_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, period: int) -> int:
    """Scratch of dct_pack_delta_temporal_auto_frames; 0 for a geometry or a period it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_temporal_auto_workspace_bytes(n, w, h, block, mbw, mbh, period))


def dct_pack_delta_temporal_auto_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int,
                                        period: int, prev_bgr: Optional[torch.Tensor] = None, prev_types: Optional[torch.Tensor] = None,
                                        forced=None, out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                                        keys: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                                        workspace: Optional[torch.Tensor] = None
                                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """dct_pack_delta_auto_frames with temporal layers (include/svc_hip_temporal.h): a frame is a key frame iff it has no reference,
    forced[f] != 0, or its difference to input frame f - min(lowbit(f), period) holds at least as many levels as the frame itself ->
    (stream, offsets, keys, counts) as dct_pack_delta_auto_frames.  Stream and offsets are dct_pack_delta_temporal_frames' with
    key = keys; keys and counts are layers.auto_keys and layers.delta_level_counts(.., period=period) of dct_pack_levels_frames' stream."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    k = None if forced is None else torch.as_tensor(forced, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one forced flag per frame"
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if keys is None:
        keys = torch.empty(n, dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_temporal_auto_workspace_bytes(n, w, h, block, mv_block, period), 16), dtype=torch.uint8,
                                device=dev)
    _check(load().svc_hip_dct_pack_delta_temporal_auto_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                              _dev(block_types, torch.int32), mbw, mbh, fg_step, bg_step,
                                                              None if prev_bgr is None else _dev(prev_bgr, torch.uint8),
                                                              None if prev_types is None else _dev(prev_types, torch.int32),
                                                              None if k is None else _dev(k, torch.int32),
                                                              _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                              out.numel(), _dev(offsets, torch.int64), _dev(keys, torch.int32),
                                                              _dev(counts, torch.int32), _stream(), period))
    return out, offsets, keys, counts


def _ladder(ladder) -> Tuple[C.Array, int]:
    """[(fg_step, bg_step), ...] -> a svc_step_pair array for the C ABI (the library checks it)."""
    pairs = [(int(fg), int(bg)) for fg, bg in ladder]
    arr = (StepPair * max(1, len(pairs)))(*[StepPair(fg, bg) for fg, bg in pairs])
    return arr, len(pairs)


def pack_levels_budget_workspace_bytes(n: int, w: int, h: int, block, ladder_len: int) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_pack_levels_budget_workspace_bytes(n, w, h, bw, bh, ladder_len))


def budget_tensor(budget, n: int, device) -> torch.Tensor:
    """A byte budget (one int for every frame, or one per frame) -> (n,) i32 on the device holding the u32 values."""
    import numpy as np
    b = np.broadcast_to(np.asarray(budget, np.int64), (n,))
    if (b < 0).any() or (b > 0xFFFFFFFF).any():
        raise ValueError("a budget is a u32 byte count")
    return torch.from_numpy(b.astype(np.uint32).view(np.int32).copy()).to(device)


def pack_levels_budget_frames(planes: torch.Tensor, block_types: torch.Tensor, block, mv_block, ladder, budget,
                              out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                              workspace: Optional[torch.Tensor] = None, choice: Optional[torch.Tensor] = None
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """RAW coefficient planes (frames, 3, H, W) f32 + region ids -> each frame packed with the finest ladder entry (fg_step, bg_step)
    whose frame fits its byte budget (include/svc_hip.h).  budget: an int, one value per frame, or an (frames,) i32 device tensor
    of u32 bytes.  -> (stream u8, offsets (frames + 1,) i64, choice (frames,) i32 on the device: the entry's index, with bit 31
    set (a negative int32) when even the last entry is over budget)."""
    n, _, h, w = planes.shape
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = planes.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(pack_levels_budget_workspace_bytes(n, w, h, block, k), 16), dtype=torch.uint8, device=dev)
    if choice is None:
        choice = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    if not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n, dev)
    _check(load().svc_hip_pack_levels_budget_frames(_dev(planes, torch.float32), _dev(block_types, torch.int32), n, w, h, bw, bh,
                                                    mbw, mbh, arr, k, _dev(budget, torch.int32), _dev(workspace, torch.uint8),
                                                    workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                    _dev(offsets, torch.int64), _dev(choice, torch.int32), _stream()))
    return out, offsets, choice


def dct_pack_levels_budget_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, ladder_len: int) -> int:
    """Scratch of dct_pack_levels_budget_frames; 0 for a geometry or a ladder length it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_levels_budget_workspace_bytes(n, w, h, block, mbw, mbh, ladder_len))


def dct_pack_levels_budget_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, ladder, budget,
                                  out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """B,G,R frames (frames, H, W, 3) u8 + region ids -> each frame packed with the finest ladder entry whose frame fits its byte
    budget, byte for byte what dct_frames + pack_levels_budget_frames leave, without the planes (include/svc_hip.h).  ladder and
    budget as pack_levels_budget_frames takes them.  -> (stream u8 of the worst-case size, offsets (frames + 1,) i64, choice
    (frames,) i32 on the device)."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = bgr.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_levels_budget_workspace_bytes(n, w, h, block, mv_block, k), 16), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    choice = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    if not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n, dev)
    _check(load().svc_hip_dct_pack_levels_budget_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                        _dev(block_types, torch.int32), mbw, mbh, arr, k, _dev(budget, torch.int32),
                                                        _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                        out.numel(), _dev(offsets, torch.int64), _dev(choice, torch.int32), _stream()))
    return out, offsets, choice


def dct_pack_levels_quality_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, ladder_len: int) -> int:
    """Scratch of dct_pack_levels_quality_frames; 0 for a geometry or a ladder length it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_levels_quality_workspace_bytes(n, w, h, block, mbw, mbh, ladder_len))


def target_tensor(target, n: int, device) -> torch.Tensor:
    """A distortion target (one int for every frame, or one per frame; layers.distortion_target gives it for a PSNR) -> (n,) i64 on the
    device holding the u64 values."""
    import numpy as np
    t = [int(v) for v in np.broadcast_to(np.asarray(target, object), (n,))]
    if any(v < 0 or v > 0xFFFFFFFFFFFFFFFF for v in t):
        raise ValueError("a distortion target is a u64")
    return torch.from_numpy(np.array(t, np.uint64).view(np.int64).copy()).to(device)


def dct_pack_levels_quality_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, ladder, target, budget=None,
                                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, distortion: bool = False):
    """B,G,R frames (frames, H, W, 3) u8 + region ids -> each frame packed with the coarsest ladder entry whose squared error still meets
    its distortion target, not finer than its byte budget allows (include/svc_hip_quality.h; layers.distortion_table and
    layers.quality_choice state it).  target: an int, one per frame, or an (frames,) i64 device tensor of u64 values; budget: None (no
    cap), or as dct_pack_levels_budget_frames takes it.  -> (stream u8 of the worst-case size, offsets (frames + 1,) i64, choice
    (frames,) i32 on the device: the entry's index, bit 31 over budget, bit 30 target not met[, the table (frames, K) i64 holding u64
    values, with distortion=True])."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = bgr.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_levels_quality_workspace_bytes(n, w, h, block, mv_block, k), 16), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    choice = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    table = torch.empty((max(n, 1), max(k, 1)), dtype=torch.int64, device=dev)[:n] if distortion else None
    if not (isinstance(target, torch.Tensor) and target.is_cuda):
        target = target_tensor(target, n, dev)
    if budget is not None and not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n, dev)
    _check(load().svc_hip_dct_pack_levels_quality_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                         _dev(block_types, torch.int32), mbw, mbh, arr, k, _dev(target, torch.int64),
                                                         None if budget is None else _dev(budget, torch.int32),
                                                         _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                         out.numel(), _dev(offsets, torch.int64), _dev(choice, torch.int32),
                                                         None if table is None else _dev(table, torch.int64), _stream()))
    return (out, offsets, choice, table) if distortion else (out, offsets, choice)


def dct_pack_delta_budget_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, ladder_len: int) -> int:
    """Scratch of dct_pack_delta_budget_frames; 0 for a geometry or a ladder length it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_budget_workspace_bytes(n, w, h, block, mbw, mbh, ladder_len))


def dct_pack_delta_budget_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, ladder, budget,
                                 key: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None, counts: bool = False):
    """B,G,R frames (frames, H, W, 3) u8 + region ids -> the delta stream (dct_pack_delta_frames without a frame before frame 0) with
    one ladder entry per GROUP of frames -- from frame 0 or a frame with key[f] != 0 up to the next -- the finest entry at which the
    group's frames together fit the group's byte budget, the sum of its frames' (include/svc_hip_delta_budget.h; layers.delta_ladder_counts,
    layers.delta_budget_choice and layers.delta_budget_frames state it).  ladder and budget as dct_pack_levels_budget_frames takes them;
    key: (frames,) i32 on the device, or None: one group.  -> (stream u8 of the worst-case size, offsets (frames + 1,) i64, choice
    (frames,) i32 on the device: the group's entry, bit 31 over budget[, the counts of differences (frames, K) i32, with counts=True])."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = bgr.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_budget_workspace_bytes(n, w, h, block, mv_block, k), 16), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    choice = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    table = torch.empty((max(n, 1), max(k, 1)), dtype=torch.int32, device=dev)[:n] if counts else None
    if not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n, dev)
    _check(load().svc_hip_dct_pack_delta_budget_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                       _dev(block_types, torch.int32), mbw, mbh, arr, k,
                                                       None if key is None else _dev(key, torch.int32), _dev(budget, torch.int32),
                                                       _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                       out.numel(), _dev(offsets, torch.int64), _dev(choice, torch.int32),
                                                       None if table is None else _dev(table, torch.int32), _stream()))
    return (out, offsets, choice, table) if counts else (out, offsets, choice)


def dct_pack_delta_quality_workspace_bytes(n: int, w: int, h: int, block: int, mv_block, ladder_len: int) -> int:
    """Scratch of dct_pack_delta_quality_frames; 0 for a geometry or a ladder length it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_delta_quality_workspace_bytes(n, w, h, block, mbw, mbh, ladder_len))


def dct_pack_delta_quality_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, ladder, target, budget=None,
                                  key: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                                  workspace: Optional[torch.Tensor] = None, counts: bool = False, distortion: bool = False):
    """B,G,R frames (frames, H, W, 3) u8 + region ids -> the delta stream (dct_pack_delta_frames without a frame before frame 0) with
    one ladder entry per GROUP of frames -- from frame 0 or a frame with key[f] != 0 up to the next -- the coarsest entry at which every
    frame of the group still meets its distortion target and the group's frames together fit the group's byte budget, if there is one
    (include/svc_hip_delta_quality.h; layers.delta_quality_choice and layers.delta_quality_frames state it).  target as
    dct_pack_levels_quality_frames takes it; budget: None (no cap), or as dct_pack_levels_budget_frames takes it; key: (frames,) i32 on
    the device, or None: one group.  -> (stream u8 of the worst-case size, offsets (frames + 1,) i64, choice (frames,) i32 on the device:
    the group's entry, bit 31 over budget, bit 30 target not met[, the counts of differences (frames, K) i32, with counts=True][, the
    distortion table (frames, K) i64 holding u64 values, with distortion=True])."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = bgr.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_delta_quality_workspace_bytes(n, w, h, block, mv_block, k), 16), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    choice = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    ctable = torch.empty((max(n, 1), max(k, 1)), dtype=torch.int32, device=dev)[:n] if counts else None
    dtable = torch.empty((max(n, 1), max(k, 1)), dtype=torch.int64, device=dev)[:n] if distortion else None
    if not (isinstance(target, torch.Tensor) and target.is_cuda):
        target = target_tensor(target, n, dev)
    if budget is not None and not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n, dev)
    _check(load().svc_hip_dct_pack_delta_quality_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block,
                                                        _dev(block_types, torch.int32), mbw, mbh, arr, k,
                                                        None if key is None else _dev(key, torch.int32), _dev(target, torch.int64),
                                                        None if budget is None else _dev(budget, torch.int32),
                                                        _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                        out.numel(), _dev(offsets, torch.int64), _dev(choice, torch.int32),
                                                        None if ctable is None else _dev(ctable, torch.int32),
                                                        None if dtable is None else _dev(dtable, torch.int64), _stream()))
    return (out, offsets, choice) + ((ctable,) if counts else ()) + ((dtable,) if distortion else ())


def unpack_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block,
                         planes: Optional[torch.Tensor] = None, block_types: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A packed stream (u8 on the device) + its offsets -> (planes (frames, 3, H, W) f32, region ids (frames, blocks) i32,
    status (frames,) i32: 0 = the frame's header matched this geometry)."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if planes is None:
        planes = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    if block_types is None:
        block_types = torch.empty((n, (w // mbw) * (h // mbh)), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(pack_levels_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_unpack_levels_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                               mbw, mbh, _dev(workspace, torch.uint8), workspace.numel(),
                                               _dev(planes, torch.float32), _dev(block_types, torch.int32), _dev(status, torch.int32),
                                               _stream()))
    return planes, block_types, status


def levels_drain(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, dst: torch.Tensor) -> None:
    """Copies offsets[-1] bytes of a packed stream into dst, a PINNED host u8 tensor of at least the worst-case size, by a kernel
    on the current stream (the byte count stays on the device)."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    assert not dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous()
    _check(load().svc_hip_levels_drain(_dev(frames, torch.uint8), _dev(offsets, torch.int64), n, w, h, bw, bh, mbw, mbh,
                                       dst.data_ptr(), dst.numel(), _stream()))


# ---- its lossless entropy coding ("SVCE" v1, include/svc_hip.h; host coder: entropy.py) ----

def entropy_max_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Worst-case bytes of n SVCE frames (what the encoder's output and an SVCE drain destination must hold)."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_entropy_max_bytes(n, w, h, bw, bh, mbw, mbh))


def entropy_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_entropy_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def entropy_encode_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block,
                          out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """SVCQ frames (u8 on the device) + their offsets -> (SVCE stream u8 of the worst-case size, offsets (frames + 1,) i64,
    status (frames,) i32: 0, or the unpack's code for a malformed input frame, written as 64 zero bytes)."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if out is None:
        out = torch.empty(max(entropy_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(entropy_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    _check(load().svc_hip_entropy_encode_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                                mbw, mbh, _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                out.numel(), _dev(out_offsets, torch.int64), _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def entropy_decode_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block,
                          out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """SVCE frames (u8 on the device) + their offsets -> (SVCQ stream u8 of SVCQ's worst-case size, offsets (frames + 1,) i64,
    status (frames,) i32 with the codes of include/svc_hip.h; a frame that fails is zeros)."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(entropy_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    _check(load().svc_hip_entropy_decode_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                                mbw, mbh, _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8),
                                                out.numel(), _dev(out_offsets, torch.int64), _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def entropy_drain(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, dst: torch.Tensor) -> None:
    """levels_drain for SVCE frames: dst is a PINNED host u8 tensor of at least entropy_max_bytes."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    assert not dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous()
    _check(load().svc_hip_entropy_drain(_dev(frames, torch.uint8), _dev(offsets, torch.int64), n, w, h, bw, bh, mbw, mbh,
                                        dst.data_ptr(), dst.numel(), _stream()))


def decode_levels_workspace_bytes(n: int, w: int, h: int, block) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_decode_levels_workspace_bytes(n, w, h, bw, bh))


def decode_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fg_step: int = 1,
                         bg_step: int = 640, gaze=None, display: Optional[Tuple[int, int]] = None,
                         rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """A packed stream (u8 on the device) + its offsets -> (rec (frames, H, W, 3) f32 B,G,R at the padded size, display
    (frames, display_h, display_w, 3) u8 or None, status (frames,) i32 with unpack's codes).  fg_step / bg_step are the DECODER's
    steps; gaze: None, or per frame x, y, w, h in padded coordinates ((frames, 4) ints, a tensor or a list); display: (w, h)."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if rec is None:
        rec = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(decode_levels_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    g = None
    if gaze is not None:
        g = torch.as_tensor(gaze, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_decode_levels_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                               mbw, mbh, fg_step, bg_step, None if g is None else _dev(g, torch.int32),
                                               _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
                                               None if out_display is None else _dev(out_display, torch.uint8), dw, dh,
                                               _dev(status, torch.int32), _stream()))
    return rec, out_display, status


def decode_levels_reduced_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fg_step: int = 1,
                                 bg_step: int = 640, reduce: int = 2, gaze=None, display: Optional[Tuple[int, int]] = None,
                                 rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """decode_levels_frames at 1 / reduce of the size (reduce 2, 4 or 8), from the first K x K coefficients of every tile, K = block /
    reduce -> (rec (frames, H / reduce, W / reduce, 3) f32 B,G,R, display (frames, display_h, display_w, 3) u8 or None, status).  w, h
    and the gaze rectangles are the padded full size's; display: (w, h) within (W / reduce, H / reduce).  Host statement:
    levels.reduced_coefficients / levels.decode_reduced_frame."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if rec is None:
        rec = torch.empty((n, h // max(reduce, 1), w // max(reduce, 1), 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(decode_levels_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    g = _rects(gaze, n, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_decode_levels_reduced_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw,
                                                       bh, mbw, mbh, fg_step, bg_step, reduce, None if g is None else _dev(g, torch.int32),
                                                       _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
                                                       None if out_display is None else _dev(out_display, torch.uint8), dw, dh,
                                                       _dev(status, torch.int32), _stream()))
    return rec, out_display, status


def decode_entropy_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_decode_entropy_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def decode_entropy_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fg_step: int = 1,
                          bg_step: int = 640, gaze=None, display: Optional[Tuple[int, int]] = None,
                          rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """decode_levels_frames straight from an SVCE stream (no SVCQ frames in between): the same arguments and outputs, bit for bit
    those of entropy_decode_frames followed by decode_levels_frames; status (frames,) i32 with the entropy decoder's codes."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if rec is None:
        rec = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(decode_entropy_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    g = None
    if gaze is not None:
        g = torch.as_tensor(gaze, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_decode_entropy_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                                mbw, mbh, fg_step, bg_step, None if g is None else _dev(g, torch.int32),
                                                _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
                                                None if out_display is None else _dev(out_display, torch.uint8), dw, dh,
                                                _dev(status, torch.int32), _stream()))
    return rec, out_display, status


# ---- two layers (include/svc_hip.h, "Two layers"; host statement: layers.py) ----

def _rects(rects, n: int, dev) -> Optional[torch.Tensor]:
    """None, or per frame x, y, w, h ((frames, 4) ints, a tensor or a list) -> (frames, 4) i32 on the device."""
    if rects is None:
        return None
    return torch.as_tensor(rects, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()


def dct_pack_layers_workspace_bytes(n: int, w: int, h: int, block: int, mv_block) -> int:
    """Scratch of dct_pack_layers_frames; 0 for a geometry it refuses."""
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_dct_pack_layers_workspace_bytes(n, w, h, block, mbw, mbh))


def dct_pack_layers_frames(bgr: torch.Tensor, block: int, block_types: torch.Tensor, mv_block, fg_step: int, bg_step: int,
                           enh_step: int, window=None, base_out: Optional[torch.Tensor] = None,
                           enh_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """B,G,R frames (frames, H, W, 3) u8 + region ids -> the base stream of dct_pack_levels_frames at (fg_step, bg_step) and the
    enhancement stream that lifts the tiles whose origin is inside the frame's window to enh_step (include/svc_hip.h), from one
    transform.  window: None (every tile), or per frame x, y, w, h in padded coordinates.  -> (base u8, base offsets (frames + 1,)
    i64, enhancement u8, enhancement offsets), each stream of the worst-case size, on the device."""
    n, h, w, _ = bgr.shape
    mbw, mbh = _bwbh(mv_block)
    dev = bgr.device
    cap = max(levels_max_bytes(n, w, h, block, mv_block), 16)
    if base_out is None:
        base_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if enh_out is None:
        enh_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(dct_pack_layers_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    base_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    enh_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    win = _rects(window, n, dev)
    _check(load().svc_hip_dct_pack_layers_frames(_dev(bgr, torch.uint8), h * w * 3, n, w, h, block, _dev(block_types, torch.int32),
                                                 mbw, mbh, fg_step, bg_step, enh_step, None if win is None else _dev(win, torch.int32),
                                                 _dev(workspace, torch.uint8), workspace.numel(), _dev(base_out, torch.uint8),
                                                 base_out.numel(), _dev(base_offsets, torch.int64), _dev(enh_out, torch.uint8),
                                                 enh_out.numel(), _dev(enh_offsets, torch.int64), _stream()))
    return base_out, base_offsets, enh_out, enh_offsets


def pack_layers_workspace_bytes(n: int, w: int, h: int, block) -> int:
    """Scratch of pack_layers_frames; 0 for a geometry it refuses."""
    bw, bh = _bwbh(block)
    return int(load().svc_hip_pack_layers_workspace_bytes(n, w, h, bw, bh))


def pack_layers_frames(planes: torch.Tensor, block_types: torch.Tensor, block, mv_block, fg_step: int, bg_step: int, enh_step: int,
                       window=None, base_out: Optional[torch.Tensor] = None, enh_out: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, base_offsets: Optional[torch.Tensor] = None,
                       enh_offsets: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Raw coefficient planes (frames, 3, H, W) f32 (dct_frames) + region ids -> the base stream pack_levels_frames writes for them at
    (fg_step, bg_step) and the enhancement stream that lifts the tiles whose origin is inside the frame's window to enh_step
    (include/svc_hip.h), for any geometry the pack takes.  window: None (every tile), or per frame x, y, w, h in padded coordinates.
    -> (base u8, base offsets (frames + 1,) i64, enhancement u8, enhancement offsets), each stream of the worst-case size, on the
    device."""
    n, _, h, w = planes.shape
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = planes.device
    cap = max(levels_max_bytes(n, w, h, block, mv_block), 16)
    if base_out is None:
        base_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if enh_out is None:
        enh_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(pack_layers_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    if base_offsets is None:
        base_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if enh_offsets is None:
        enh_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    win = _rects(window, n, dev)
    _check(load().svc_hip_pack_layers_frames(_dev(planes, torch.float32), _dev(block_types, torch.int32), n, w, h, bw, bh, mbw, mbh,
                                             fg_step, bg_step, enh_step, None if win is None else _dev(win, torch.int32),
                                             _dev(workspace, torch.uint8), workspace.numel(), _dev(base_out, torch.uint8),
                                             base_out.numel(), _dev(base_offsets, torch.int64), _dev(enh_out, torch.uint8),
                                             enh_out.numel(), _dev(enh_offsets, torch.int64), _stream()))
    return base_out, base_offsets, enh_out, enh_offsets


def decode_layers_workspace_bytes(n: int, w: int, h: int, block) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_decode_layers_workspace_bytes(n, w, h, bw, bh))


def decode_layers_frames(base: torch.Tensor, base_offsets: torch.Tensor, enh: Optional[torch.Tensor],
                         enh_offsets: Optional[torch.Tensor], w: int, h: int, block, mv_block, fg_step: int = 1, bg_step: int = 640,
                         gaze=None, display: Optional[Tuple[int, int]] = None, rec: Optional[torch.Tensor] = None,
                         out_display: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """decode_levels_frames on a base and an enhancement stream: inside the gaze a tile decodes at the enhancement's step, elsewhere
    as decode_levels_frames decodes the base.  enh / enh_offsets may be None when gaze is None (the enhancement is then not read).
    status (frames,) i32: the base frame's code, else 0x100 | the enhancement frame's, else 0x100 | 11 (not this base's layer)."""
    n = base_offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = base.device
    if rec is None:
        rec = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(decode_layers_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    g = _rects(gaze, n, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_decode_layers_frames(_dev(base, torch.uint8), base.numel(), _dev(base_offsets, torch.int64),
                                               None if enh is None else _dev(enh, torch.uint8), 0 if enh is None else enh.numel(),
                                               None if enh_offsets is None else _dev(enh_offsets, torch.int64), n, w, h, bw, bh,
                                               mbw, mbh, fg_step, bg_step, None if g is None else _dev(g, torch.int32),
                                               _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
                                               None if out_display is None else _dev(out_display, torch.uint8), dw, dh,
                                               _dev(status, torch.int32), _stream()))
    return rec, out_display, status


def decode_layers_reduced_workspace_bytes(n: int, w: int, h: int, block) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_decode_layers_reduced_workspace_bytes(n, w, h, bw, bh))


def decode_layers_reduced_frames(base: torch.Tensor, base_offsets: torch.Tensor, enh: Optional[torch.Tensor],
                                 enh_offsets: Optional[torch.Tensor], w: int, h: int, block, mv_block, fg_step: int = 1,
                                 bg_step: int = 640, reduce: int = 2, gaze=None, display: Optional[Tuple[int, int]] = None,
                                 rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None
                                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """decode_layers_frames at 1 / reduce of the size (reduce 2, 4 or 8), from the first K x K coefficients of every tile of both
    layers, K = block / reduce -> (rec (frames, H / reduce, W / reduce, 3) f32 B,G,R, display (frames, display_h, display_w, 3) u8 or
    None, status as decode_layers_frames).  w, h and the gaze rectangles are the padded full size's; display: (w, h) within (W / reduce,
    H / reduce).  enh / enh_offsets may be None when gaze is None: the call is then decode_levels_reduced_frames on the base.  Host
    statement: layers.reduced_coefficients / layers.decode_layers_reduced_frame."""
    n = base_offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = base.device
    if rec is None:
        rec = torch.empty((n, h // max(reduce, 1), w // max(reduce, 1), 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(decode_layers_reduced_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    g = _rects(gaze, n, dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_decode_layers_reduced_frames(_dev(base, torch.uint8), base.numel(), _dev(base_offsets, torch.int64),
                                                       None if enh is None else _dev(enh, torch.uint8), 0 if enh is None else enh.numel(),
                                                       None if enh_offsets is None else _dev(enh_offsets, torch.int64), n, w, h, bw, bh,
                                                       mbw, mbh, fg_step, bg_step, reduce, None if g is None else _dev(g, torch.int32),
                                                       _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
                                                       None if out_display is None else _dev(out_display, torch.uint8), dw, dh,
                                                       _dev(status, torch.int32), _stream()))
    return rec, out_display, status


def window_levels_workspace_bytes(n_out: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of window_levels_frames for n_out output frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_window_levels_workspace_bytes(n_out, w, h, bw, bh, mbw, mbh))


def window_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, window=None, src=None,
                         out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """An SVCQ stream (u8 on the device) + its offsets, restricted to a window per output frame (include/svc_hip.h; the numpy statement is
    layers.window_frames): output frame i is input frame src[i] (src None: frame i) with only the tiles whose origin window[i] contains.
    window: None (every tile), or per output frame x, y, w, h in padded coordinates; src: None, or the input frame of each output frame
    ((n_out,) ints, a tensor or a list; repeats and any order).  -> (stream u8 of the worst-case size, offsets (n_out + 1,) i64, status
    (n_out,) i32 with unpack's codes for the input frame, 1 for an index past the input; a frame that fails is 64 zero bytes).  `out`
    must not overlap `frames`."""
    n_in = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    s = None if src is None else torch.as_tensor(src, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    n_out = n_in if s is None else s.numel()
    if out is None:
        out = torch.empty(max(levels_max_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(window_levels_workspace_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)[:n_out]
    win = _rects(window, n_out, dev)
    _check(load().svc_hip_window_levels_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n_in,
                                               None if s is None else _dev(s, torch.int32), n_out, w, h, bw, bh, mbw, mbh,
                                               None if win is None else _dev(win, torch.int32), _dev(workspace, torch.uint8),
                                               workspace.numel(), _dev(out, torch.uint8), out.numel(), _dev(out_offsets, torch.int64),
                                               _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def band_levels_workspace_bytes(n_out: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of band_levels_frames for n_out output frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_band_levels_workspace_bytes(n_out, w, h, bw, bh, mbw, mbh))


def band_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, band=None, window=None, src=None,
                       out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """An SVCQ stream (u8 on the device) + its offsets, restricted to a frequency band and a window per output frame (include/svc_hip.h;
    the numpy statement is layers.band_frames): output frame i is input frame src[i] (src None: frame i) with, of the tiles whose origin
    window[i] contains, only the coefficients (row r, column c) with r < hi_h, c < hi_w and not (r < lo_h and c < lo_w).  band: None (every
    coefficient), or per output frame lo_w, lo_h, hi_w, hi_h ((n_out, 4) ints, a tensor or a list); window, src, the buffers and the
    result as window_levels_frames takes and gives them.  `out` must not overlap `frames`."""
    n_in = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    s = None if src is None else torch.as_tensor(src, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    n_out = n_in if s is None else s.numel()
    if out is None:
        out = torch.empty(max(levels_max_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(band_levels_workspace_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)[:n_out]
    win, bnd = _rects(window, n_out, dev), _rects(band, n_out, dev)
    _check(load().svc_hip_band_levels_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n_in,
                                             None if s is None else _dev(s, torch.int32), n_out, w, h, bw, bh, mbw, mbh,
                                             None if win is None else _dev(win, torch.int32), None if bnd is None else _dev(bnd, torch.int32),
                                             _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                             _dev(out_offsets, torch.int64), _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def union_levels_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of union_levels_frames for n frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_union_levels_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def union_levels_frames(a: torch.Tensor, a_offsets: torch.Tensor, b: torch.Tensor, b_offsets: torch.Tensor, w: int, h: int, block, mv_block,
                        out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Two SVCQ streams of the same number of frames whose masks are disjoint, such as two bands of one stream, joined frame by frame
    (include/svc_hip.h; the numpy statement is layers.union_frames): the masks ORed, the levels of both in coefficient order, the header
    and types of `a`.  -> (stream u8 of the worst-case size, offsets (n + 1,) i64, status (n,) i32: a's unpack code, else 0x100 | b's,
    else 0x100 | 11 for other steps or types, else 12 for masks that share a bit; a frame that fails is 64 zero bytes).  `out` must not
    overlap `a` or `b`."""
    n = a_offsets.numel() - 1
    assert b_offsets.numel() == n + 1, "the two streams hold different numbers of frames"
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = a.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(union_levels_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    _check(load().svc_hip_union_levels_frames(_dev(a, torch.uint8), a.numel(), _dev(a_offsets, torch.int64), _dev(b, torch.uint8), b.numel(),
                                              _dev(b_offsets, torch.int64), n, w, h, bw, bh, mbw, mbh, _dev(workspace, torch.uint8),
                                              workspace.numel(), _dev(out, torch.uint8), out.numel(), _dev(out_offsets, torch.int64),
                                              _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def delta_levels_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of delta_levels_frames for n frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_delta_levels_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def undelta_levels_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of undelta_levels_frames for n frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_undelta_levels_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def _delta_call(undo: bool, frames, offsets, w, h, block, mv_block, prev, key, out, out_offsets, workspace, status, period=None):
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    k = None if key is None else torch.as_tensor(key, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one key flag per frame"
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        if period is None:
            query = undelta_levels_workspace_bytes if undo else delta_levels_workspace_bytes
            need = query(n, w, h, block, mv_block)
        else:
            query = undelta_levels_temporal_workspace_bytes if undo else delta_levels_temporal_workspace_bytes
            need = query(n, w, h, block, mv_block, period)
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    if period is None:
        fn = load().svc_hip_undelta_levels_frames if undo else load().svc_hip_delta_levels_frames
    else:
        fn = load().svc_hip_undelta_levels_temporal_frames if undo else load().svc_hip_delta_levels_temporal_frames
    _check(fn(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, None if prev is None else _dev(prev, torch.uint8),
              0 if prev is None else prev.numel(), None if k is None else _dev(k, torch.int32), w, h, bw, bh, mbw, mbh,
              _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(), _dev(out_offsets, torch.int64),
              _dev(status, torch.int32), _stream(), *(() if period is None else (period,))))
    return out, out_offsets, status


def delta_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, prev: Optional[torch.Tensor] = None,
                        key=None, out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """An SVCQ stream (u8 on the device) + its offsets, every frame coded against the frame before it (include/svc_hip.h; the numpy
    statement is layers.delta_frames): in the tiles both frames code at one step the levels' difference modulo 2^16, elsewhere and in a key
    frame the levels.  prev: None (frame 0 is a key frame) or the one input frame before frame 0, exactly its bytes; key: None, or per frame
    != 0 for a key frame ((n,) ints, a tensor or a list).  -> (stream u8 of the worst-case size, offsets (n + 1,) i64, status (n,) i32: the
    frame's unpack code, else 0x100 | its predecessor's; a frame that fails is 64 zero bytes).  `out` must not overlap `frames` or `prev`."""
    return _delta_call(False, frames, offsets, w, h, block, mv_block, prev, key, out, out_offsets, workspace, status)


def undelta_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, prev: Optional[torch.Tensor] = None,
                          key=None, out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """delta_levels_frames undone (include/svc_hip.h; the numpy statement is layers.undelta_frames): frame i is the delta stream's frame i
    plus OUTPUT frame i - 1, with the key flags the delta call took.  prev: None, or the reconstructed frame before frame 0 (the last
    output frame of the call before).  The result as delta_levels_frames gives it; a failure runs down the chain to the next key frame."""
    return _delta_call(True, frames, offsets, w, h, block, mv_block, prev, key, out, out_offsets, workspace, status)


def delta_levels_temporal_workspace_bytes(n: int, w: int, h: int, block, mv_block, period: int) -> int:
    """Scratch of delta_levels_temporal_frames for n frames; 0 for a geometry or a period it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_delta_levels_temporal_workspace_bytes(n, w, h, bw, bh, mbw, mbh, period))


def undelta_levels_temporal_workspace_bytes(n: int, w: int, h: int, block, mv_block, period: int) -> int:
    """Scratch of undelta_levels_temporal_frames for n frames; 0 for a geometry or a period it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_undelta_levels_temporal_workspace_bytes(n, w, h, bw, bh, mbw, mbh, period))


def delta_levels_temporal_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, period: int,
                                 prev: Optional[torch.Tensor] = None, key=None, out: Optional[torch.Tensor] = None,
                                 out_offsets: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                 status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """delta_levels_frames with temporal layers (include/svc_hip.h, "Temporal layers"; the numpy statement is
    layers.delta_temporal_frames): frame i is coded against INPUT frame i - min(lowbit(i), period), period 1, 2 or 4, so the frames with
    i % 2^s == 0 are the stream of period >> s of the thinned clip.  prev: None, or the input frame at index -period.  Frame i of the call
    must have a stream index that is i modulo period.  The rest as delta_levels_frames; a frame's status hangs on its reference's."""
    return _delta_call(False, frames, offsets, w, h, block, mv_block, prev, key, out, out_offsets, workspace, status, period)


def undelta_levels_temporal_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, period: int,
                                   prev: Optional[torch.Tensor] = None, key=None, out: Optional[torch.Tensor] = None,
                                   out_offsets: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                   status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """delta_levels_temporal_frames undone (the numpy statement is layers.undelta_temporal_frames): frame i is the delta stream's frame i
    plus OUTPUT frame i - min(lowbit(i), period).  prev: None, or the reconstructed frame at index -period.  A failure runs down the tree
    of references: a damaged odd frame harms no other."""
    return _delta_call(True, frames, offsets, w, h, block, mv_block, prev, key, out, out_offsets, workspace, status, period)


def decode_delta_levels_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of decode_delta_levels_frames for n frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_decode_delta_levels_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def decode_delta_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fg_step: int = 1,
                               bg_step: int = 640, prev: Optional[torch.Tensor] = None, key=None, gaze=None,
                               display: Optional[Tuple[int, int]] = None, want_last: bool = False, rec: Optional[torch.Tensor] = None,
                               out_display: Optional[torch.Tensor] = None, last: Optional[torch.Tensor] = None,
                               workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """A packed delta stream (u8 on the device) + its offsets -> (rec, display or None, status, last or None, last_bytes or None):
    undelta_levels_frames and decode_levels_frames in one call (include/svc_hip.h).  rec (frames, H, W, 3) f32 B,G,R at the padded size
    and display (frames, display_h, display_w, 3) u8 have the bits of those two calls; status (frames,) i32 is the undelta call's.
    fg_step / bg_step are the DECODER's steps; prev: None (frame 0 is a key frame) or the reconstructed frame before frame 0, exactly its
    bytes; key: None, or per frame != 0 for a key frame; gaze: None, or per frame x, y, w, h in padded coordinates; display: (w, h).
    want_last (or a `last` buffer of at least levels_max_bytes(1, ...)): the reconstructed SVCQ frame of the last frame, the next call's
    prev once cut to last_bytes (a (1,) i64 tensor on the device).  `last` must not overlap `frames` or `prev`."""
    return _decode_delta_call(None, frames, offsets, w, h, block, mv_block, fg_step, bg_step, prev, key, gaze, display, want_last, rec,
                              out_display, last, workspace, status)


def _decode_delta_call(_period, frames, offsets, w, h, block, mv_block, fg_step, bg_step, prev, key, gaze, display, want_last, rec, out_display,
                       last, workspace, status):
    """decode_delta_levels_frames (_period None) or decode_delta_levels_temporal_frames."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    k = None if key is None else torch.as_tensor(key, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one key flag per frame"
    if rec is None:
        rec = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if want_last and last is None:
        last = torch.empty(max(levels_max_bytes(1, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    last_bytes = None if last is None else torch.zeros(1, dtype=torch.int64, device=dev)
    if workspace is None:
        need = (decode_delta_levels_workspace_bytes(n, w, h, block, mv_block) if _period is None else
                decode_delta_levels_temporal_workspace_bytes(n, w, h, block, mv_block, _period))
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    g = None
    if gaze is not None:
        g = torch.as_tensor(gaze, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    fn = load().svc_hip_decode_delta_levels_frames if _period is None else load().svc_hip_decode_delta_levels_temporal_frames
    _check(fn(
        _dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, None if prev is None else _dev(prev, torch.uint8),
        0 if prev is None else prev.numel(), None if k is None else _dev(k, torch.int32), w, h, bw, bh, mbw, mbh, fg_step, bg_step,
        None if g is None else _dev(g, torch.int32), _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
        None if out_display is None else _dev(out_display, torch.uint8), dw, dh, None if last is None else _dev(last, torch.uint8),
        0 if last is None else last.numel(), None if last is None else _dev(last_bytes, torch.int64), _dev(status, torch.int32), _stream(),
        *(() if _period is None else (_period,))))
    return rec, out_display, status, last, last_bytes


def decode_delta_levels_temporal_workspace_bytes(n: int, w: int, h: int, block, mv_block, period: int) -> int:
    """Scratch of decode_delta_levels_temporal_frames for n frames; 0 for a geometry or a period it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_decode_delta_levels_temporal_workspace_bytes(n, w, h, bw, bh, mbw, mbh, period))


def decode_delta_levels_temporal_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, period: int,
                                        fg_step: int = 1, bg_step: int = 640, prev: Optional[torch.Tensor] = None, key=None, gaze=None,
                                        display: Optional[Tuple[int, int]] = None, want_last: bool = False,
                                        rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                                        last: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                        status: Optional[torch.Tensor] = None
                                        ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """decode_delta_levels_frames with temporal layers (include/svc_hip.h, "Temporal layers"): undelta_levels_temporal_frames and
    decode_levels_frames in one call, with that function's arguments and results.  period: 1, 2 or 4; prev: the reconstructed frame at
    index -period; `last` is reconstructed frame period * ((n - 1) // period), the next call's prev."""
    return _decode_delta_call(period, frames, offsets, w, h, block, mv_block, fg_step, bg_step, prev, key, gaze, display, want_last, rec,
                              out_display, last, workspace, status)


def decode_delta_levels_reduced_workspace_bytes(n: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of decode_delta_levels_reduced_frames for n frames, at any reduce; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_decode_delta_levels_reduced_workspace_bytes(n, w, h, bw, bh, mbw, mbh))


def decode_delta_levels_reduced_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fg_step: int = 1,
                                       bg_step: int = 640, reduce: int = 2, prev: Optional[torch.Tensor] = None, key=None, gaze=None,
                                       display: Optional[Tuple[int, int]] = None, want_last: bool = False,
                                       rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                                       last: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                       status: Optional[torch.Tensor] = None
                                       ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """A packed delta stream (u8 on the device), or its band (0, 0, K, K) with K = block / reduce, + its offsets -> (rec, display or None,
    status, last or None, last_bytes or None): undelta_levels_frames and decode_levels_reduced_frames in one call (include/svc_hip.h; the
    numpy statement is layers.undelta_frames + levels.decode_reduced_frame + layers.band_frames).  rec (frames, H / reduce, W / reduce, 3)
    f32 B,G,R and display (frames, display_h, display_w, 3) u8 have the bits of those two calls; status (frames,) i32 is the undelta call's.
    reduce: 2, 4 or 8.  fg_step / bg_step, key, gaze (full-size padded coordinates) and display as decode_delta_levels_frames takes them.
    prev: None (frame 0 is a key frame), or the reconstructed frame before frame 0 or its band (0, 0, K, K), exactly its bytes.
    want_last (or a `last` buffer of at least levels_max_bytes(1, ...)): the band (0, 0, K, K) of the reconstructed last frame, the next
    call's prev once cut to last_bytes (a (1,) i64 tensor on the device).  `last` must not overlap `frames` or `prev`."""
    return _decode_delta_reduced_call(None, frames, offsets, w, h, block, mv_block, fg_step, bg_step, reduce, prev, key, gaze, display,
                                      want_last, rec, out_display, last, workspace, status)


def _decode_delta_reduced_call(_period, frames, offsets, w, h, block, mv_block, fg_step, bg_step, reduce, prev, key, gaze, display, want_last,
                               rec, out_display, last, workspace, status):
    """decode_delta_levels_reduced_frames (_period None) or decode_delta_levels_temporal_reduced_frames."""
    n = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    k = None if key is None else torch.as_tensor(key, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    assert k is None or k.numel() == n, "one key flag per frame"
    if rec is None:
        rec = torch.empty((n, h // max(reduce, 1), w // max(reduce, 1), 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    if want_last and last is None:
        last = torch.empty(max(levels_max_bytes(1, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    last_bytes = None if last is None else torch.zeros(1, dtype=torch.int64, device=dev)
    if workspace is None:
        need = (decode_delta_levels_reduced_workspace_bytes(n, w, h, block, mv_block) if _period is None else
                decode_delta_levels_temporal_reduced_workspace_bytes(n, w, h, block, mv_block, _period))
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    g = None
    if gaze is not None:
        g = torch.as_tensor(gaze, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()
    if status is None:
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    fn = load().svc_hip_decode_delta_levels_reduced_frames if _period is None else load().svc_hip_decode_delta_levels_temporal_reduced_frames
    _check(fn(
        _dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, None if prev is None else _dev(prev, torch.uint8),
        0 if prev is None else prev.numel(), None if k is None else _dev(k, torch.int32), w, h, bw, bh, mbw, mbh, fg_step, bg_step, reduce,
        None if g is None else _dev(g, torch.int32), _dev(workspace, torch.uint8), workspace.numel(), _dev(rec, torch.float32),
        None if out_display is None else _dev(out_display, torch.uint8), dw, dh, None if last is None else _dev(last, torch.uint8),
        0 if last is None else last.numel(), None if last is None else _dev(last_bytes, torch.int64), _dev(status, torch.int32), _stream(),
        *(() if _period is None else (_period,))))
    return rec, out_display, status, last, last_bytes


def decode_delta_levels_temporal_reduced_workspace_bytes(n: int, w: int, h: int, block, mv_block, period: int) -> int:
    """Scratch of decode_delta_levels_temporal_reduced_frames for n frames, at any reduce; 0 for a geometry or a period it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_decode_delta_levels_temporal_reduced_workspace_bytes(n, w, h, bw, bh, mbw, mbh, period))


def decode_delta_levels_temporal_reduced_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, period: int,
                                                fg_step: int = 1, bg_step: int = 640, reduce: int = 2,
                                                prev: Optional[torch.Tensor] = None, key=None, gaze=None,
                                                display: Optional[Tuple[int, int]] = None, want_last: bool = False,
                                                rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None,
                                                last: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                                status: Optional[torch.Tensor] = None
                                                ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """decode_delta_levels_reduced_frames with temporal layers (include/svc_hip_temporal_decode.h): undelta_levels_temporal_frames and
    decode_levels_reduced_frames in one call, with that function's arguments and results plus period (1, 2 or 4).  There is no numpy
    statement of its own: it is layers.undelta_temporal_frames + levels.decode_reduced_frame, and for the streams it takes
    layers.band_frames / layers.thin_frames.  The stream may be the temporal delta stream or its band (0, 0, K, K), K = block / reduce;
    prev: the reconstructed frame at index -period or that band of it; `last` is the band (0, 0, K, K) of reconstructed frame
    period * ((n - 1) // period), the next call's prev."""
    return _decode_delta_reduced_call(period, frames, offsets, w, h, block, mv_block, fg_step, bg_step, reduce, prev, key, gaze, display,
                                      want_last, rec, out_display, last, workspace, status)


def window_entropy_max_bytes(n_out: int, w: int, h: int, block, mv_block) -> int:
    """Worst-case bytes of n_out frames of window_entropy_frames (a canonical frame with a chunk per tile); 0 where it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_window_entropy_max_bytes(n_out, w, h, bw, bh, mbw, mbh))


def window_entropy_workspace_bytes(n_out: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of window_entropy_frames for n_out output frames; 0 for a geometry it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_window_entropy_workspace_bytes(n_out, w, h, bw, bh, mbw, mbh))


def window_entropy_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, window=None, src=None,
                          out: Optional[torch.Tensor] = None, out_offsets: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """window_levels_frames on an SVCE stream, on its coded bytes (include/svc_hip.h; the numpy statement is entropy.window_frames):
    chunks inside the window are copied, chunks outside it become the empty chunk, and only the chunks a window edge cuts are re-coded.
    window, src as window_levels_frames takes them.  -> (SVCE stream u8 of the worst-case size, offsets (n_out + 1,) i64, status (n_out,)
    i32 with the entropy decoder's frame-check codes, 9 for a malformed cut chunk; a frame that fails is 64 zero bytes).  `out` must not
    overlap `frames`."""
    n_in = offsets.numel() - 1
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    s = None if src is None else torch.as_tensor(src, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    n_out = n_in if s is None else s.numel()
    if out is None:
        out = torch.empty(max(window_entropy_max_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if out_offsets is None:
        out_offsets = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(window_entropy_workspace_bytes(n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)[:n_out]
    win = _rects(window, n_out, dev)
    _check(load().svc_hip_window_entropy_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n_in,
                                                None if s is None else _dev(s, torch.int32), n_out, w, h, bw, bh, mbw, mbh,
                                                None if win is None else _dev(win, torch.int32), _dev(workspace, torch.uint8),
                                                workspace.numel(), _dev(out, torch.uint8), out.numel(), _dev(out_offsets, torch.int64),
                                                _dev(status, torch.int32), _stream()))
    return out, out_offsets, status


def split_levels_workspace_bytes(n_in: int, n_out: int, w: int, h: int, block, mv_block) -> int:
    """Scratch of split_levels_frames for n_out output frames; 0 for a geometry or a frame count it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_split_levels_workspace_bytes(n_in, n_out, w, h, bw, bh, mbw, mbh))


def split_levels_budget_workspace_bytes(n_in: int, n_out: int, w: int, h: int, block, mv_block, ladder_len: int) -> int:
    """Scratch of split_levels_budget_frames; 0 for a geometry, a frame count or a ladder length it refuses."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    return int(load().svc_hip_split_levels_budget_workspace_bytes(n_in, n_out, w, h, bw, bh, mbw, mbh, ladder_len))


def _split_buffers(frames, offsets, w, h, block, mv_block, src, window, enhancement, base_out, base_offsets, enh_out, enh_offsets, status):
    """The arguments both split calls share -> (n_in, n_out, src, window, base_out, base_offsets, enh_out, enh_offsets, status)."""
    n_in = offsets.numel() - 1
    dev = frames.device
    s = None if src is None else torch.as_tensor(src, dtype=torch.int32).reshape(-1).to(dev).contiguous()
    n_out = n_in if s is None else s.numel()
    cap = max(levels_max_bytes(n_out, w, h, block, mv_block), 16)
    if base_out is None:
        base_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if base_offsets is None:
        base_offsets = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if enhancement:
        if enh_out is None:
            enh_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        if enh_offsets is None:
            enh_offsets = torch.empty(n_out + 1, dtype=torch.int64, device=dev)
    if status is None:
        status = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)[:n_out]
    return n_in, n_out, s, _rects(window, n_out, dev), base_out, base_offsets, enh_out, enh_offsets, status


def split_levels_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fine_step: int, fg_step: int,
                        bg_step: int, window=None, src=None, enhancement: bool = True, base_out: Optional[torch.Tensor] = None,
                        base_offsets: Optional[torch.Tensor] = None, enh_out: Optional[torch.Tensor] = None,
                        enh_offsets: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                        status: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    """A stored SVCQ stream encoded at (fine_step, fine_step) + its offsets -> a base stream at (fg_step, bg_step), multiples of
    fine_step, and the enhancement stream that lifts the tiles inside window[i] back to fine_step (include/svc_hip.h; the numpy statement
    is layers.split_frames).  window, src as window_levels_frames takes them.  enhancement=False: the base only; enh_out is then neither
    written nor checked and comes back as it was passed.  -> (base u8 of the worst-case size, base offsets (n_out + 1,) i64, enhancement,
    its offsets, status (n_out,) i32: unpack's code for the input frame, 1 for an index past the input, 11 for a frame that is not at
    fine_step; a frame that fails is 64 zero bytes in both outputs).  The outputs must not overlap `frames`."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    n_in, n_out, s, win, base_out, base_offsets, enh_out, enh_offsets, status = _split_buffers(
        frames, offsets, w, h, block, mv_block, src, window, enhancement, base_out, base_offsets, enh_out, enh_offsets, status)
    if workspace is None:
        workspace = torch.empty(max(split_levels_workspace_bytes(n_in, n_out, w, h, block, mv_block), 16), dtype=torch.uint8, device=frames.device)
    _check(load().svc_hip_split_levels_frames(
        _dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n_in, None if s is None else _dev(s, torch.int32), n_out,
        w, h, bw, bh, mbw, mbh, fine_step, fg_step, bg_step, None if win is None else _dev(win, torch.int32),
        _dev(workspace, torch.uint8), workspace.numel(), _dev(base_out, torch.uint8), base_out.numel(), _dev(base_offsets, torch.int64),
        _dev(enh_out, torch.uint8) if enhancement else None, enh_out.numel() if enhancement else 0,
        _dev(enh_offsets, torch.int64) if enhancement else None, _dev(status, torch.int32), _stream()))
    return base_out, base_offsets, enh_out, enh_offsets, status


def split_levels_budget_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, fine_step: int, ladder,
                               budget, window=None, src=None, enhancement: bool = True, base_out: Optional[torch.Tensor] = None,
                               base_offsets: Optional[torch.Tensor] = None, enh_out: Optional[torch.Tensor] = None,
                               enh_offsets: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                               status: Optional[torch.Tensor] = None, choice: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """split_levels_frames with the base steps picked per output frame: the finest ladder entry (fg_step, bg_step) whose BASE frame fits
    its byte budget (ladder and budget as pack_levels_budget_frames takes them; every step a multiple of fine_step).  -> (base, base
    offsets, enhancement, its offsets, status, choice (n_out,) i32: the entry's index, with bit 31 set (a negative int32) when even the
    last entry is over budget; 0 for a frame that fails)."""
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    arr, k = _ladder(ladder)
    dev = frames.device
    n_in, n_out, s, win, base_out, base_offsets, enh_out, enh_offsets, status = _split_buffers(
        frames, offsets, w, h, block, mv_block, src, window, enhancement, base_out, base_offsets, enh_out, enh_offsets, status)
    if workspace is None:
        workspace = torch.empty(max(split_levels_budget_workspace_bytes(n_in, n_out, w, h, block, mv_block, k), 16), dtype=torch.uint8, device=dev)
    if choice is None:
        choice = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)[:n_out]
    if not (isinstance(budget, torch.Tensor) and budget.is_cuda):
        budget = budget_tensor(budget, n_out, dev)
    _check(load().svc_hip_split_levels_budget_frames(
        _dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n_in, None if s is None else _dev(s, torch.int32), n_out,
        w, h, bw, bh, mbw, mbh, fine_step, arr, k, _dev(budget, torch.int32), None if win is None else _dev(win, torch.int32),
        _dev(workspace, torch.uint8), workspace.numel(), _dev(base_out, torch.uint8), base_out.numel(), _dev(base_offsets, torch.int64),
        _dev(enh_out, torch.uint8) if enhancement else None, enh_out.numel() if enhancement else 0,
        _dev(enh_offsets, torch.int64) if enhancement else None, _dev(choice, torch.int32), _dev(status, torch.int32), _stream()))
    return base_out, base_offsets, enh_out, enh_offsets, status, choice


def gaze_rect(cx: int, cy: int, max_w: int, max_h: int, frame_w: int, frame_h: int, padded_w: int, padded_h: int
              ) -> Tuple[int, int, int, int]:
    """The reference decoder's gaze rectangle around a centre in the source frame, scaled to the padded frame: (x, y, w, h)."""
    out = (_u32 * 4)()
    _check(load().svc_hip_gaze_rect(cx, cy, max_w, max_h, frame_w, frame_h, padded_w, padded_h, out))
    return tuple(int(v) for v in out)


def decode_records_frames(records: torch.Tensor, w: int, h: int, block: int, fg_step: int = 1, bg_step: int = 640, gaze=None,
                          display: Optional[Tuple[int, int]] = None, emit_h: Optional[int] = None,
                          rec: Optional[torch.Tensor] = None, out_display: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Wire records (frames, bytes) u8 on the device, frame f's records in row f -> (rec (frames, H, W, 3) f32 B,G,R at the padded
    size w x h, display (frames, display_h, display_w, 3) u8 or None).  fg_step / bg_step are the DECODER's steps; gaze: None, or per
    frame x, y, w, h in padded coordinates; display: (w, h); emit_h: the height the records were emitted for (default h; tile rows
    past it come out as zeros)."""
    n = records.shape[0]
    emit_h = h if emit_h is None else emit_h
    dev = records.device
    if rec is None:
        rec = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    dw, dh = display if display is not None else (0, 0)
    if display is not None and out_display is None:
        out_display = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=dev)
    g = None
    if gaze is not None:
        g = torch.as_tensor(gaze, dtype=torch.int32).reshape(n, 4).to(dev).contiguous()
    _check(load().svc_hip_decode_records_frames(_dev(records, torch.uint8), records.stride(0) if n else 4 * (1 + 3 * block * block),
                                                n, w, h, block, emit_h, fg_step, bg_step, None if g is None else _dev(g, torch.int32),
                                                _dev(rec, torch.float32), None if out_display is None else _dev(out_display, torch.uint8),
                                                dw, dh, _stream()))
    return rec, out_display


def wire_layout(header: bytes, stream_bytes: int) -> Tuple[int, int]:
    """How a whole wire stream of stream_bytes bytes with this 32-byte header is read -> (emit_frame_h, frame_bytes)."""
    hdr = WireHeader.from_buffer_copy(bytes(header[:C.sizeof(WireHeader)]))
    emit, per = _u32(), _u64()
    _check(load().svc_hip_wire_layout(C.byref(hdr), stream_bytes, C.byref(emit), C.byref(per)))
    return int(emit.value), int(per.value)


# ---- wire records <-> the compact stream, stream to stream (include/svc_hip.h; numpy statement: wire.py) ----

def records_pack_levels_workspace_bytes(n: int, w: int, h: int, block: int, mv_block) -> int:
    mbw, mbh = _bwbh(mv_block)
    return int(load().svc_hip_records_pack_levels_workspace_bytes(n, w, h, block, mbw, mbh))


def records_pack_levels_frames(records: torch.Tensor, w: int, h: int, block: int, mv_block, fg_step: int, bg_step: int,
                               emit_h: Optional[int] = None, out: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                               workspace: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Wire records (frames, bytes) u8 on the device, frame f's records in row f, read at the padded size w x h (emit_h: the height
    they were emitted for, default h) -> what pack_levels_frames writes for their planes and per-MV-block types at (fg_step, bg_step),
    without the planes: (stream u8 of the worst-case size, offsets (frames + 1,) i64, status (frames,) i32: 4 = a record's type word
    differs from its MV block's)."""
    n = records.shape[0]
    emit_h = h if emit_h is None else emit_h
    mbw, mbh = _bwbh(mv_block)
    dev = records.device
    if out is None:
        out = torch.empty(max(levels_max_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(records_pack_levels_workspace_bytes(n, w, h, block, mv_block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_records_pack_levels_frames(_dev(records, torch.uint8), records.stride(0) if n else 4 * (1 + 3 * block * block),
                                                     n, w, h, block, emit_h, mbw, mbh, fg_step, bg_step,
                                                     _dev(workspace, torch.uint8), workspace.numel(), _dev(out, torch.uint8), out.numel(),
                                                     _dev(offsets, torch.int64), _dev(status, torch.int32), _stream()))
    return out, offsets, status


def levels_records_workspace_bytes(n: int, w: int, h: int, block) -> int:
    bw, bh = _bwbh(block)
    return int(load().svc_hip_levels_records_workspace_bytes(n, w, h, bw, bh))


def levels_records_frames(frames: torch.Tensor, offsets: torch.Tensor, w: int, h: int, block, mv_block, emit_h: Optional[int] = None,
                          records: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                          status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A packed stream (u8 on the device) + its offsets -> (wire records (frames, bytes) u8, the bytes of unpack_levels_frames +
    serialize_frames(w, emit_h) without the planes; status (frames,) i32 with unpack_levels_frames' codes, a failed frame is zeros).
    records: a (frames, stride) u8 tensor to write into (bytes of a row past its records are left alone)."""
    n = offsets.numel() - 1
    emit_h = h if emit_h is None else emit_h
    (bw, bh), (mbw, mbh) = _bwbh(block), _bwbh(mv_block)
    dev = frames.device
    if records is None:
        records = torch.empty((n, serialized_frame_bytes(w, emit_h, bw, bh)), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(max(levels_records_workspace_bytes(n, w, h, block), 16), dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    _check(load().svc_hip_levels_records_frames(_dev(frames, torch.uint8), frames.numel(), _dev(offsets, torch.int64), n, w, h, bw, bh,
                                                mbw, mbh, emit_h, _dev(workspace, torch.uint8), workspace.numel(),
                                                _dev(records, torch.uint8), records.stride(0) if n else 4 * (1 + 3 * bw * bh),
                                                _dev(status, torch.int32), _stream()))
    return records, status
