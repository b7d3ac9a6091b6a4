/* svc_hip_temporal.h -- the temporal-layer delta stream straight from pixels.
 *
 * These declarations are kept apart from svc_hip.h because that header's declarations are tied one to
 * one to tables that this addition leaves as they are (the ABI and stream-order censuses of the test
 * suite, and svc_hip_abi_version(), which stays 5); they move into svc_hip.h with those tables.
 *
 * Everything svc_hip.h says of its entry points holds here: device pointers, `stream` a hipStream_t
 * (NULL: the null stream), calls only enqueue work and return SVC_OK or an svc_status with
 * svc_hip_last_error() set. */
#ifndef SVC_HIP_TEMPORAL_H
#define SVC_HIP_TEMPORAL_H

#include "svc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * A temporal-layer delta stream straight from pixels: svc_hip_dct_pack_levels_frames and
 * svc_hip_delta_levels_temporal_frames in one call, without the plain stream in between.
 *
 * d_out and d_frame_offsets are byte for byte what svc_hip_dct_pack_levels_frames on the same
 * frames, followed by svc_hip_delta_levels_temporal_frames on its output with the same d_key and
 * period and with d_prev = svc_hip_dct_pack_levels_frames of (d_prev_bgr, d_prev_types) at the same
 * steps, leave.  Frame i > 0 is coded against INPUT frame i - min(lowbit(i), period) (svc_hip.h,
 * "Temporal layers"); frame 0 against the frame at d_prev_bgr with the region ids at d_prev_types,
 * the input frame at index -period (both NULL: none, frame 0 is a key frame).  Frame i of a call
 * has a stream index congruent to i modulo period.  The predicted-tile rule, the difference modulo
 * 2^16 and d_key are those of svc_hip_dct_pack_delta_frames.  A batch cut into two calls at any
 * multiple of period, the second given input frame cut - period and its types, writes the bytes of
 * one call.  svc_hip_undelta_levels_temporal_frames and svc_hip_decode_delta_levels_temporal_frames
 * take the output; every 2^s-th frame of it is this call's output for the thinned clip at
 * period >> s.  Nothing is written past offsets[n_frames].
 *
 * period 1 runs svc_hip_dct_pack_delta_frames and gives its bytes; 2 and 4 run the TEMPORAL form of
 * its transform kernel: a run of 8 frames starts at a frame of layer 0, so every reference but its
 * first frame's lies in the run; a wave keeps the levels of the last layer-0 frame in registers and,
 * at period 4, those of frame 4k + 2 from there to frame 4k + 3.  9 transforms for 8 frames and
 * three launches, whatever n_frames.  Measured in profiles/dct_pack_delta_temporal_c3.txt.
 *
 * Geometry, limits, the order of the checks, alignments and the pairing of d_prev_bgr and
 * d_prev_types are those of svc_hip_dct_pack_delta_frames; a period other than 1, 2 or 4 is
 * SVC_ERR_INVALID_ARG, checked right after the geometry as the temporal calls on streams do.  The
 * workspace query returns 0 where the call refuses.
 * ------------------------------------------------------------------------- */
uint64_t svc_hip_dct_pack_delta_temporal_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                                         uint32_t block, uint32_t mv_block_w, uint32_t mv_block_h,
                                                         uint32_t period);
int svc_hip_dct_pack_delta_temporal_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames,
                                           uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                           const uint32_t* d_block_types /* [n_frames][mv blocks] */,
                                           uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step,
                                           const uint8_t* d_prev_bgr     /* one frame, input frame -period; NULL: frame 0 is a key frame */,
                                           const uint32_t* d_prev_types  /* [mv blocks] of that frame; NULL exactly when d_prev_bgr is */,
                                           const uint32_t* d_key         /* [n_frames] or NULL, as svc_hip_delta_levels_frames takes it */,
                                           uint8_t* d_workspace, uint64_t workspace_bytes,
                                           uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets /* [n_frames + 1] */,
                                           void* stream, uint32_t period /* 1, 2 or 4 */);

/* ------------------------------------------------------------------------- *
 * The same with the key frames chosen by size: svc_hip_dct_pack_delta_auto_frames' rule with "the
 * frame before" read as the frame's temporal reference.  Frame f is a key frame iff it has no
 * reference (f == 0 and d_prev_bgr NULL), or d_forced[f] != 0, or its difference to input frame
 * f - min(lowbit(f), period) (frame 0: the frame at d_prev_bgr) holds at least as many non-zero
 * levels as the frame itself.
 *   d_out, d_frame_offsets   byte for byte svc_hip_dct_pack_delta_temporal_frames with d_key = d_key_out
 *   d_key_out [n]            0 / 1: layers.auto_keys of
 *   d_level_counts [n][2]    layers.delta_level_counts(.., period=period) of
 *                            svc_hip_dct_pack_levels_frames' stream.  May be NULL
 * The choice for a frame depends on that frame and its reference alone, so a batch cut at a
 * multiple of period gives the bytes, flags and counts of one call, and the choices thin as the
 * stream does: for even f the reference of f / 2 at period / 2 is half the reference of f, so
 * every 2^s-th flag, count and frame is this call's on the thinned clip at period >> s.
 *
 * The counting kernel is the TALLY form of the temporal transform, the selection
 * svc_hip_dct_pack_delta_auto_frames' own; five launches whatever n_frames.  period 1 runs that
 * call.  Checks as svc_hip_dct_pack_delta_auto_frames, the period right after the geometry.
 * ------------------------------------------------------------------------- */
uint64_t svc_hip_dct_pack_delta_temporal_auto_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                                              uint32_t block, uint32_t mv_block_w, uint32_t mv_block_h,
                                                              uint32_t period);
int svc_hip_dct_pack_delta_temporal_auto_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames,
                                                uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                const uint32_t* d_block_types /* [n_frames][mv blocks] */,
                                                uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step,
                                                const uint8_t* d_prev_bgr     /* one frame, input frame -period, or NULL */,
                                                const uint32_t* d_prev_types  /* [mv blocks] of that frame; NULL exactly when d_prev_bgr is */,
                                                const uint32_t* d_forced      /* [n_frames] != 0: a key frame whatever its size; or NULL */,
                                                uint8_t* d_workspace, uint64_t workspace_bytes,
                                                uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets /* [n_frames + 1] */,
                                                uint32_t* d_key_out /* [n_frames] */, uint32_t* d_level_counts /* [n_frames][2] or NULL */,
                                                void* stream, uint32_t period /* 1, 2 or 4 */);

#ifdef __cplusplus
}
#endif

#endif /* SVC_HIP_TEMPORAL_H */
