/* svc_hip_temporal_decode.h -- the temporal-layer delta stream played at reduced size.
 *
 * These declarations are kept apart from svc_hip.h and svc_hip_temporal.h for the reason svc_hip_temporal.h gives: both headers'
 * declarations are tied one to one to tables that this addition leaves as they are (the ABI and stream-order censuses of the test
 * suite, and svc_hip_abi_version(), which stays 5); they move into svc_hip.h with those tables.
 *
 * Everything svc_hip.h says of its entry points holds here: device pointers, `stream` a hipStream_t
 * (NULL: the null stream), calls only enqueue work and return SVC_OK or an svc_status with
 * svc_hip_last_error() set. */
#ifndef SVC_HIP_TEMPORAL_DECODE_H
#define SVC_HIP_TEMPORAL_DECODE_H

#include "svc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- *
 * A temporal-layer delta stream straight to display frames at reduced size:
 * svc_hip_undelta_levels_temporal_frames and svc_hip_decode_levels_reduced_frames in one call, the
 * temporal form of svc_hip_decode_delta_levels_reduced_frames.  K = block / reduce.
 *
 * Pictures and status: d_rec [n_frames][frame_h / reduce][frame_w / reduce][3], d_display and
 * d_status are bit for bit svc_hip_undelta_levels_temporal_frames with the same d_prev, d_key and
 * period, followed by svc_hip_decode_levels_reduced_frames on its output with the same steps, reduce,
 * gaze and display size.  A frame that fails is zeros; the statuses run down the tree of references
 * (svc_hip.h, "Temporal layers"); the gaze rule is the reduced decoder's: full-size padded tile origins.
 *
 * Reads: no level outside the first K x K coefficients of a tile is read, in the frames or in d_prev.
 * So on the band (0, 0, K, K) of the stored temporal stream (svc_hip_band_levels_frames) every output
 * has the bits it has on the full stream.  Band and thinning (svc_hip_window_levels_frames with d_src)
 * commute: a server makes a small, slow viewer's stream from the stored one with those two calls in
 * either order, and the kept frames (i % 2^s == 0) of a period-p stream play through this call at
 * period p >> s -- at p >> s == 1 through svc_hip_decode_delta_levels_reduced_frames -- with the same bits.
 *
 * d_prev is the reconstructed frame at index -period: the full frame or its band (0, 0, K, K).  Frame
 * i of a call has a stream index congruent to i modulo period.
 *
 * d_last receives the band (0, 0, K, K) of reconstructed frame period * ((n_frames - 1) / period), the
 * frame the next call's frame 0 refers to: byte for byte svc_hip_band_levels_frames with that band and
 * no window on that output frame of the temporal undelta call; 64 zero bytes if that frame failed; a
 * set bit of level 0 is cleared.  last_capacity follows svc_hip_decode_delta_levels_reduced_frames.  A
 * stream cut into calls at multiples of period, each given the previous call's d_last, gives the
 * pictures of one call, and a chain moves freely between this call and
 * svc_hip_undelta_levels_temporal_frames on the band stream.
 *
 * period 1 runs svc_hip_decode_delta_levels_reduced_frames and gives its outputs exactly; 2 and 4 run
 * its kernel with one set of 3 K held levels per temporal layer below the odd frames, all in registers.
 * Checked in this order: geometry, period (anything but 1, 2, 4: SVC_ERR_INVALID_ARG), then as
 * svc_hip_decode_delta_levels_reduced_frames.  The query returns 0 where the call refuses; the workspace
 * is that call's.  Only enqueues work; the number of launches does not depend on n_frames.  Measured
 * in profiles/decode_delta_temporal_reduced_c3.txt.
 * ------------------------------------------------------------------------- */
uint64_t svc_hip_decode_delta_levels_temporal_reduced_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                                                      uint32_t block_w, uint32_t block_h,
                                                                      uint32_t mv_block_w, uint32_t mv_block_h, uint32_t period);
int svc_hip_decode_delta_levels_temporal_reduced_frames(const uint8_t* d_frames, uint64_t stream_bytes,
                                                        const uint64_t* d_frame_offsets, uint32_t n_frames,
                                                        const uint8_t* d_prev /* reconstructed frame -period or its band (0, 0, K, K); NULL: frame 0 is a key frame */,
                                                        uint64_t prev_bytes,
                                                        const uint32_t* d_key /* [n_frames], as the delta call took it */,
                                                        uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                        uint32_t mv_block_w, uint32_t mv_block_h,
                                                        uint32_t fg_step, uint32_t bg_step, uint32_t reduce,
                                                        const uint32_t* d_gaze /* [n_frames][4] or NULL */,
                                                        uint8_t* d_workspace, uint64_t workspace_bytes,
                                                        float* d_rec /* [n_frames][frame_h / reduce][frame_w / reduce][3] */,
                                                        uint8_t* d_display /* [n_frames][display_h][display_w][3] or NULL */,
                                                        uint32_t display_w, uint32_t display_h,
                                                        uint8_t* d_last /* the band (0, 0, K, K) of frame period * ((n_frames - 1) / period); NULL: not wanted */,
                                                        uint64_t last_capacity,
                                                        uint64_t* d_last_bytes /* [1] */,
                                                        uint32_t* d_status /* [n_frames] */, void* stream,
                                                        uint32_t period /* 1, 2 or 4 */);

#ifdef __cplusplus
}
#endif

#endif /* SVC_HIP_TEMPORAL_DECODE_H */
