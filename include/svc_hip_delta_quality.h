/* svc_hip_delta_quality.h -- constant quality for the delta stream inside the fused transform: a distortion target per group of frames.
 *
 * These declarations are kept apart from svc_hip.h for the reason svc_hip_temporal.h gives: that header's declarations are tied one
 * to one to tables that this addition leaves as they are (the ABI and stream-order censuses of the test suite, and
 * svc_hip_abi_version(), which stays 5); they move into svc_hip.h with those tables.
 *
 * Everything svc_hip.h says of its entry points holds here: device pointers, `stream` a hipStream_t
 * (NULL: the null stream), calls only enqueue work and return SVC_OK or an svc_status with
 * svc_hip_last_error() set. */
#ifndef SVC_HIP_DELTA_QUALITY_H
#define SVC_HIP_DELTA_QUALITY_H

#include "svc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * svc_hip_dct_pack_delta_budget_frames with a distortion target in place of the byte budget, or
 * beside it: per GROUP of frames the coarsest entry of `ladder` at which every frame of the group
 * still meets its target, within what the group's byte budget (if any) allows.
 * scalable_video_codec_amd/layers.py states it in numpy (delta_groups, delta_ladder_counts,
 * distortion_table, delta_quality_choice, delta_quality_frames); the outputs are bit for bit those
 * statements.
 *
 * Groups, counts and bytes are exactly those of svc_hip_delta_budget.h: a group starts at frame 0 and
 * at every frame f with d_key[f] != 0 (d_key == NULL: one group); a call holds whole groups, there is
 * no d_prev_bgr, and frame 0 is a key frame; count[f][k] is the number of non-zero differences of
 * frame f at entry k and bytes_k(f) = up16(levels offset + 2 * count[f][k]).  d_level_counts, where
 * not NULL, receives the counts, [n_frames][ladder_len] u32.
 *
 * Distortion.  D[f][k] is exactly that of svc_hip_quality.h: the sum over the frame's coefficients of
 * e * e, e = rint(256 * (c - q * s)), as u64.  The delta is lossless in levels, so a frame's
 * distortion at entry k depends neither on its flags nor on its predecessor: d_distortion, where
 * not NULL, receives the table svc_hip_dct_pack_levels_quality_frames gives for the same frames,
 * [n_frames][ladder_len] u64.
 *
 * Choice.  d_target[f]: u64 in the units of D.  d_budget[f]: u32 bytes, or d_budget == NULL: no cap.
 * Per group G, every entry examined (neither table is monotone along a ladder):
 *     Q = the entries k with D[f][k] <= d_target[f] for EVERY frame f of G -- per frame, not a sum: a
 *         viewer sees frames, and a sum would let one bad frame hide behind eleven good ones;
 *     F = the entries k with sum over G of bytes_k(f) <= sum over G of d_budget[f], both sums of 64
 *         bits; every entry where d_budget == NULL;
 *     choice = max(Q and F) where that set is not empty: the coarsest entry that meets the quality and fits;
 *              else, where F is not empty, min(F) with bit 30 set: the finest entry that fits, quality not met;
 *              else ladder_len - 1 with bit 31 set, and bit 30 set iff ladder_len - 1 is not in Q.
 * d_choice[f] is the value of f's group.  With one frame per group and sizes that are monotone along
 * the ladder this is svc_hip_dct_pack_levels_quality_frames' max(kq, kb), flags included.
 * Frame f is then byte for byte frame f of svc_hip_dct_pack_delta_frames with the pair of entry
 * d_choice[f] & 0x3FFFFFFF and the same flags; d_frame_offsets as there (all n_frames + 1), and nothing
 * is written past offsets[n_frames].  svc_hip_undelta_levels_frames and
 * svc_hip_decode_delta_levels_frames take the stream with the same flags.
 *
 * Geometry, stride, ladder rules, limits and the order of the checks are those of
 * svc_hip_dct_pack_delta_budget_frames: geometry, stride, ladder, limits, workspace, capacity
 * (n_frames worst-case frames); n_frames == 0 then returns SVC_OK; then pointers.  d_target and
 * d_distortion are 8-byte aligned, the rest as there.  The query returns 0 where the call refuses.
 * The workspace starts with that call's, so the delta-budget and the fixed delta call run on it as
 * well.  Only enqueues work, on the caller's stream, with no host wait; six launches whatever n_frames:
 * one pass over the pixels for both tables, their sum, the groups' selection, then the delta form's
 * three with each frame's own steps.  A stream past 2^32 bytes is written by the unchanged assemble
 * pass of svc_hip_dct_pack_levels_frames, whose offsets the suite covers there.  Measured in
 * profiles/dct_pack_delta_quality_c3.txt.
 * ------------------------------------------------------------------------- */
uint64_t svc_hip_dct_pack_delta_quality_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                        uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len);
int svc_hip_dct_pack_delta_quality_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames,
                                          uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                          const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h,
                                          const svc_step_pair* ladder /* host, finest first */, uint32_t ladder_len,
                                          const uint32_t* d_key /* [n_frames] or NULL: one group */,
                                          const uint64_t* d_target /* [n_frames] */,
                                          const uint32_t* d_budget /* [n_frames] bytes, or NULL: no cap */,
                                          uint8_t* d_workspace, uint64_t workspace_bytes,
                                          uint8_t* d_out, uint64_t out_capacity,
                                          uint64_t* d_frame_offsets /* [n_frames + 1] */,
                                          uint32_t* d_choice /* [n_frames] */,
                                          uint32_t* d_level_counts /* [n_frames][ladder_len], or NULL: not wanted */,
                                          uint64_t* d_distortion /* [n_frames][ladder_len], or NULL: not wanted */,
                                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SVC_HIP_DELTA_QUALITY_H */
