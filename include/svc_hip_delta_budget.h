/* svc_hip_delta_budget.h -- rate control of the delta stream inside the fused transform: a byte budget per group of frames.
 *
 * These declarations are kept apart from svc_hip.h for the reason svc_hip_temporal.h gives: that header's declarations are tied one
 * to one to tables that this addition leaves as they are (the ABI and stream-order censuses of the test suite, and
 * svc_hip_abi_version(), which stays 5); they move into svc_hip.h with those tables.
 *
 * Everything svc_hip.h says of its entry points holds here: device pointers, `stream` a hipStream_t
 * (NULL: the null stream), calls only enqueue work and return SVC_OK or an svc_status with
 * svc_hip_last_error() set. */
#ifndef SVC_HIP_DELTA_BUDGET_H
#define SVC_HIP_DELTA_BUDGET_H

#include "svc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * svc_hip_dct_pack_delta_frames with the steps chosen from `ladder` by a byte budget, one pair per
 * GROUP of frames.  scalable_video_codec_amd/layers.py states it in numpy (delta_groups,
 * delta_ladder_counts, delta_budget_choice, delta_budget_frames); the outputs are bit for bit those
 * statements.
 *
 * Groups.  A group starts at frame 0 and at every frame f with d_key[f] != 0, and runs up to the next
 * start; d_key == NULL: the call is one group.  A frame that starts a group is a key frame, every
 * other frame is coded against input frame f - 1.  A tile is predicted only where the frame and its
 * predecessor code it at one step, so steps that move from frame to frame would make every frame a
 * key frame: the group is the unit that can carry one pair.
 *
 * No predecessor frame.  A group's choice needs the counts of the whole group, so a call holds whole
 * groups: there is no d_prev_bgr, and frame 0 is a key frame whatever d_key[0] says.  A clip is cut
 * into calls at group starts only.
 *
 * Counts.  For entry k = (fg_step, bg_step) and a frame f, with level_k(c) the pack's level of the
 * raw f32 coefficient c at the step entry k gives c's tile (the type of the MV block that holds the
 * tile, type 0 takes bg_step):
 *     count[f][k] = the coefficients with level_k(c of f) != level_k(c of f - 1)   in a predicted tile,
 *                   the coefficients with level_k(c of f) != 0                     elsewhere,
 * a tile being predicted at entry k where f does not start a group and entry k gives the tile one
 * step in f and in f - 1.  That is header word 10 of frame f of svc_hip_dct_pack_levels_frames at
 * entry k followed by svc_hip_delta_levels_frames with the keys.  It is NOT monotone in k: two
 * levels that agree at a fine step can differ at a coarser one, and an entry with fg_step == bg_step
 * predicts tiles that its neighbours do not.  d_level_counts, where not NULL, receives the table,
 * [n_frames][ladder_len] u32.
 *
 * Choice.  bytes_k(f) = up16(levels offset + 2 * count[f][k]), the SVCQ frame's size.  d_budget[f]:
 * u32 bytes.  Per group G, in 64-bit sums,
 *     choice = the smallest k with sum over G of bytes_k(f) <= sum over G of d_budget[f],
 * found by looking at every entry (an entry may fit behind one that does not); where none fits, the
 * last entry with bit 31 set.  d_choice[f] is the value of f's group.
 * Frame f is then byte for byte frame f of svc_hip_dct_pack_delta_frames with the pair of entry
 * d_choice[f] & 0x7FFFFFFF and the same flags: header steps are the chosen pair, inexact is 0, word
 * 10 the number of non-zero differences.  d_frame_offsets as there (all n_frames + 1), and nothing is
 * written past offsets[n_frames].  svc_hip_undelta_levels_frames and svc_hip_decode_delta_levels_frames
 * take the stream with the same flags: the steps change only at key frames.
 *
 * Geometry, stride and limits are those of svc_hip_dct_pack_delta_frames; the ladder's rules
 * (1 .. 64 entries, positive, non-decreasing in both steps) those of
 * svc_hip_dct_pack_levels_budget_frames.  Checked in this order: geometry, stride, ladder, limits,
 * workspace, capacity (n_frames worst-case frames); n_frames == 0 then returns SVC_OK; then pointers.
 * Frames, output and workspace are 16-byte aligned, offsets 8-byte, d_block_types, d_key, d_budget,
 * d_choice and d_level_counts 4-byte.  The query returns 0 where the call refuses.  The workspace
 * starts with svc_hip_dct_pack_delta_frames', so that call runs on it as well.  Only enqueues work, on
 * the caller's stream, with no host wait; six launches whatever n_frames.  A stream past 2^32 bytes
 * is written by the unchanged assemble pass of svc_hip_dct_pack_levels_frames, whose offsets the
 * suite covers there.  Measured in profiles/dct_pack_delta_budget_c3.txt.
 * ------------------------------------------------------------------------- */
uint64_t svc_hip_dct_pack_delta_budget_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                       uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len);
int svc_hip_dct_pack_delta_budget_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames,
                                         uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                         const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h,
                                         const svc_step_pair* ladder /* host, finest first */, uint32_t ladder_len,
                                         const uint32_t* d_key /* [n_frames] or NULL: one group */,
                                         const uint32_t* d_budget /* [n_frames] bytes */,
                                         uint8_t* d_workspace, uint64_t workspace_bytes,
                                         uint8_t* d_out, uint64_t out_capacity,
                                         uint64_t* d_frame_offsets /* [n_frames + 1] */,
                                         uint32_t* d_choice /* [n_frames] */,
                                         uint32_t* d_level_counts /* [n_frames][ladder_len], or NULL: not wanted */,
                                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SVC_HIP_DELTA_BUDGET_H */
