"""The compact stream straight from the transform kernel (csrc/dct_pack.hip) against the two-call route it replaces, at C3 (1080p,
8x8 tiles, steps 1 / 640) or C5 (4K, 16x16 tiles).

  python tools/dct_pack_probe.py kernels [C3|C5]   one batch of 16 encoded frames, region ids from the pipeline; the two-call route
                                                   (svc_hip_dct_quant_frames + svc_hip_pack_levels_frames) 5 times, then the fused
                                                   route (svc_hip_dct_pack_levels_frames) 5 times; the bytes are compared.  Run under
                                                   `rocprofv3 --kernel-trace --stats -- python ...` (a kernel trace only)
  python tools/dct_pack_probe.py fused [C3|C5]     the fused route alone, 5 times (for a counter run of its own: `rocprofv3 --pmc ...`)
  python tools/dct_pack_probe.py step [C3|C5] [frames]
                                                   svc::ClipEncoder over a resident clip (default 300 frames = 299 pairs), serial and
                                                   pipelined: the compact step against the two-pass planes step plus the pack of its
                                                   output; wall time per step over back-to-back steps
  python tools/dct_pack_probe.py budget [C3|C5]    rate control: the same batch, levels.step_ladder(1, 256, 4, 640, 10, 24) (32 entries) and
                                                   1.1 MB per 1080p frame (scaled by the pixels at C5); the planes route (svc_hip_dct_frames +
                                                   svc_hip_pack_levels_budget_frames) 5 times, then svc_hip_dct_pack_levels_budget_frames 5
                                                   times; stream, offsets and choices are compared.  Run under rocprofv3 as `kernels`
  python tools/dct_pack_probe.py quality [C3|C5]   constant quality: the same batch and ladder, svc_hip_dct_pack_levels_quality_frames at a 40 dB
                                                   and a 30 dB target against (a) svc_hip_dct_pack_levels_budget_frames and (b) per entry the
                                                   fixed fused pack + svc_hip_decode_levels_frames + a torch squared error; one process, the
                                                   routes in turn, the median of three rounds; then entries, PSNR and bytes (raw and
                                                   entropy-coded) at both targets on the synthetic clip and on a static background
  python tools/dct_pack_probe.py quality-kernels [C3|C5]
                                                   the quality call and the budgeted call five times each and nothing else: for a kernel trace
  python tools/dct_pack_probe.py quality-variants [C3|C5]
                                                   the quality call against a build of csrc/dct_pack.hip that computes every ladder entry
                                                   (SVC_DCT_PACK_MEASURE_SHARE=0), on the 32-entry ladder and on one whose every entry moves both steps
  python tools/dct_pack_probe.py delta-budget [C3|C5]
                                                   rate control of the delta stream: svc_hip_dct_pack_delta_budget_frames on the same batch and
                                                   ladder with a key frame every 8, against (a) per entry svc_hip_dct_pack_delta_frames for the
                                                   sizes plus one more encode, (b) that call at fixed steps and (c)
                                                   svc_hip_dct_pack_levels_budget_frames; then entries, bytes and PSNR of this call and of the
                                                   per-frame budgeted plain stream at the same budgets, on the synthetic clip and on a static
                                                   background.  delta-budget-kernels: this call and the quality call five times each, for a
                                                   kernel trace
  python tools/dct_pack_probe.py delta-quality [C3|C5]
                                                   constant quality for the delta stream: svc_hip_dct_pack_delta_quality_frames on the same batch
                                                   and ladder with a key frame every 8, against (a) a build of csrc/dct_pack.hip that takes the two
                                                   tables from two passes (SVC_DCT_PACK_DELTA_QUALITY_TWO_PASS=1), (b) the route a caller had before
                                                   it -- the quality call, the delta-budget call and one more delta-budget call standing in for the
                                                   encode at the chosen steps -- and (c) svc_hip_dct_pack_delta_budget_frames alone; then entries,
                                                   bytes raw and entropy-coded and PSNR at 40 dB and 30 dB, of this call and of the per-frame plain
                                                   quality call, on the synthetic clip and on a static background.  delta-quality-kernels: this
                                                   call five times, for a kernel trace
  python tools/dct_pack_probe.py quality_step [C3|C5] [frames]
                                                   svc::ClipEncoder compact steps: fixed, under the budget, at a 40 dB target (SetCompactQuality)
  python tools/dct_pack_probe.py budget_step [C3|C5] [frames]
                                                   svc::ClipEncoder with compact: the step at the fixed steps against the step under that
                                                   budget (SetCompactBudget), serial and pipelined; wall time per step
  python tools/dct_pack_probe.py layers [C3|C5]    two layers, the same batch of 16: (a) svc_hip_dct_pack_layers_frames at (1, 640, 1) and
                                                   (16, 16, 1) against svc_hip_dct_pack_levels_frames twice (base pair, then fine pair);
                                                   (b) svc_hip_decode_layers_frames against svc_hip_decode_levels_frames on the fine stream,
                                                   gaze 64 x 64 and the whole frame; (c) bytes per frame of the base, the enhancement (window
                                                   256 x 256, and none) and the single stream at (1, 1), raw and entropy-coded.  Wall time
                                                   per call over back-to-back calls, as `step`; the outputs are compared
  python tools/dct_pack_probe.py window [C3|C5]    a stored enhancement served under a gaze, the same batch of 16 at (1, 640, 1) with a
                                                   256 x 256 window per frame: svc_hip_window_levels_frames on the every-tile enhancement
                                                   stream against svc_hip_dct_pack_layers_frames with those windows (the other way to these
                                                   bytes), then 4 viewers (n_out = 64 from the 16 stored frames through d_src) against 4 such
                                                   encodes; wall time per call over 20 back-to-back calls; the bytes are compared
  python tools/dct_pack_probe.py split [C3|C5]     a stored fine stream served at other base steps, the same batch of 16 at (fg, bg, e) =
                                                   (1, 640, 1) with a 256 x 256 window per frame: svc_hip_split_levels_frames and
                                                   svc_hip_split_levels_budget_frames (the 32-entry ladder and the budget of `budget`) on the
                                                   stream stored at (1, 1), against svc_hip_dct_pack_layers_frames from the pixels with the same
                                                   steps and windows (the call it replaces) and svc_hip_window_levels_frames on the stored
                                                   enhancement (the call it sits beside); wall time per call over 20 back-to-back calls, the
                                                   bytes each call reads and writes and their fraction of the HBM peak, and the split's base
                                                   against the encoder's base at (1, 640) (an even ratio: they differ)
  python tools/dct_pack_probe.py band [C3|C5] [frames]
                                                   a stored stream served by frequency band, the same batch of 16 stored at (1, 640) and at
                                                   (1, 1): (a) bytes per frame of the bands (0, 0, K, K), K = N / 2, N / 4, N / 8, and of their
                                                   remainders, raw and entropy-coded, beside the stored stream's; (b) svc_hip_band_levels_frames
                                                   against svc_hip_window_levels_frames with no window and svc_hip_split_levels_frames on the
                                                   same stream; (c) svc_hip_union_levels_frames of a band and its remainder against the same
                                                   two, its bytes compared with the stored stream's; (d) 4 viewers at four K (n_out = 64 through
                                                   d_src) against four calls; wall time per call over 20 back-to-back calls; (e) `frames`
                                                   (default 64) frames at (1, 640) as SVCE through tests/dropin/stream_reduced_main at reduce 2,
                                                   4, 8: the band stream against the full stream, alternating, every run printed
  python tools/dct_pack_probe.py delta [C3|C5]     a stream coded frame against frame in levels, the same batch of 16 with frame 0 the key
                                                   frame, stored at (1, 640), at (1, 1) and as the every-tile enhancement at (1, 640, 1):
                                                   (a) bytes per frame of the delta stream beside the intra stream, raw and entropy-coded, and
                                                   undelta(delta) compared with the stored stream; (b) svc_hip_delta_levels_frames and
                                                   svc_hip_undelta_levels_frames against svc_hip_union_levels_frames on two bands of the same
                                                   stream and svc_hip_window_levels_frames with no window, then svc_hip_undelta_levels_frames
                                                   followed by svc_hip_decode_levels_frames against the decode alone; wall time per call over
                                                   20 back-to-back calls
  python tools/dct_pack_probe.py delta-encode      the delta stream straight from the pixels (svc_hip_dct_pack_delta_frames), at C3 and at C5, a batch of 16 at
                                                   (1, 640) and (1, 1), with frame 0 the key frame (a key frame every 16) and with the frame before
                                                   given and no key frame: the call with runs of 1, 2, 4 and 8 frames (csrc/dct_pack.hip built once per
                                                   value into tools/_bin, -DSVC_DCT_PACK_DELTA_RUN), svc_hip_dct_pack_levels_frames alone, that call
                                                   + svc_hip_delta_levels_frames, and the planes route (svc_hip_dct_quant_frames,
                                                   svc_hip_pack_levels_frames) + svc_hip_delta_levels_frames; wall time per call over 20 back-to-back
                                                   calls, the routes alternating in one process, the median of three; the bytes are compared.  Then
                                                   delta bytes against plain bytes, raw and entropy-coded, for the synthetic clip and for a static
                                                   background (the first synthetic frame repeated) under a moving 128 x 128 patch of the clip, region
                                                   ids foreground under the patch.  Then tests/dropin/stream_delta_encode_main on a 33-frame 1080p
                                                   clip, with delta and without, plain and entropy-coded, the list twice
  python tools/dct_pack_probe.py delta-auto        the delta stream with its key frames chosen by size (svc_hip_dct_pack_delta_auto_frames), at C3 and at C5, a
                                                   batch of 16 at (1, 640) and (1, 1): the call against svc_hip_dct_pack_delta_frames with fixed
                                                   flags (a key frame every 16) and against the route a caller has without it --
                                                   svc_hip_dct_pack_levels_frames + svc_hip_dct_pack_delta_frames with no key frame and the choice
                                                   per frame from the two offset arrays (the chosen frames are NOT copied together); wall time
                                                   per call over 20 back-to-back calls, the routes in turn, the median of three; flags and bytes
                                                   are compared.  Then, on the synthetic clip, on the static background under a moving patch and
                                                   on 8 frames of the one followed by 8 of the other turned upside down (a cut), raw and
                                                   entropy-coded bytes per frame of the plain stream, of delta with a key frame every 16 and of
                                                   delta with the chosen flags, and the frames at which the level-count choice is not the
                                                   smaller CODED frame with the bytes that costs.  Then tests/dropin/stream_delta_auto_main on a
                                                   33-frame 1080p clip with auto_key and with delta alone, plain and entropy-coded, the list twice
  python tools/dct_pack_probe.py delta-temporal    temporal layers of the delta stream, at C3 and one line at C5, a batch of 16 at (1, 640) and (1, 1) with
                                                   frame 0 the key frame: svc_hip_delta_levels_temporal_frames at periods 2 and 4 against
                                                   svc_hip_delta_levels_frames on the same plain stream, and the encoder's two-call route
                                                   (svc_hip_dct_pack_levels_frames + the temporal call at period 4) against
                                                   svc_hip_dct_pack_delta_frames; wall time per call over 20 back-to-back calls, the routes in turn,
                                                   the median of three.  Then, at C3, raw and entropy-coded bytes per frame at periods 1, 2 and 4
                                                   for delta-auto's three clips, and what a half-rate and a quarter-rate viewer is sent from the
                                                   period-4 stream.  Then tests/dropin/stream_temporal_main on a 33-frame 1080p clip at periods 4
                                                   and 1 (`delta` alone), encode and play, the list twice
  python tools/dct_pack_probe.py window-entropy [C3|C5]
                                                   a stored entropy-coded enhancement served under a gaze, the same batch of 16 at
                                                   (1, 640, 1) with a 256 x 256 window per frame: svc_hip_window_entropy_frames on the stored
                                                   SVCE stream against the three-call route on the same stream (svc_hip_entropy_decode_frames,
                                                   svc_hip_window_levels_frames, svc_hip_entropy_encode_frames), then 4 viewers (n_out = 64
                                                   through d_src; the three-call route decodes the 16 stored frames once); wall time per call
                                                   over 20 back-to-back calls, the two routes interleaved, bytes in and out and the share of
                                                   chunks in each class; the bytes are compared
  python tools/dct_pack_probe.py pack-layers      both layers from raw planes, at C3 and at C5, a batch of 16 each at (fg, bg, e) =
                                                   (1, 640, 1) with a 256 x 256 window per frame: svc_hip_pack_layers_frames on the planes
                                                   svc_hip_dct_frames wrote, against two svc_hip_pack_levels_frames calls on the same planes
                                                   (at (fg, bg), then at (e, e)) in the same process; wall time per call over 20 back-to-back
                                                   calls, the two routes interleaved, and the bytes each moves; the base is compared
  python tools/dct_pack_probe.py delta-temporal-encode
                                                   the temporal-layer delta stream from pixels: svc_hip_dct_pack_delta_temporal_frames at
                                                   periods 2 and 4, at C3 and C5, steps (1, 640) and (1, 1), against the two calls it replaces
                                                   (bytes compared), svc_hip_dct_pack_delta_frames (period 1) and
                                                   svc_hip_dct_pack_levels_frames alone, and svc_hip_dct_pack_delta_temporal_auto_frames
                                                   against it; one process, the routes in turn, the median of three rounds.  Then
                                                   delta-temporal's host-driver runs (tests/dropin/stream_temporal_main, periods 4 and 1)
  python tools/dct_pack_probe.py stream-layers    the two layers through the host drivers: a 65-frame C3 synthetic clip made on the CPU,
                                                   batches of 16, (1, 640, 1), a 256 x 256 window and a gaze centre per frame;
                                                   tests/dropin/stream_layers_main (plain, entropy-coded, and with every tile enhanced) beside
                                                   stream_levels_main, stream_entropy_main and stream_decode_main on the same clip and gaze,
                                                   the whole list twice in turn; PCIe-inclusive rates as the applications print them
  python tools/dct_pack_probe.py transcode [C3|C5] the wire stream <-> the compact stream without planes, a batch of 8 (the drivers' wire
                                                   batch) of raw-coefficient records with the pipeline's region ids, at (1, 640) and (1, 1):
                                                   svc_hip_records_pack_levels_frames against svc_hip_pack_levels_frames on the same
                                                   coefficients as planes, and svc_hip_levels_records_frames against
                                                   svc_hip_unpack_levels_frames + svc_hip_serialize_frames; wall time per call over 20
                                                   back-to-back calls, the routes alternating, the median of three runs each; the bytes are
                                                   compared.  Then tests/dropin/wire_transcode_main --rate on 24 such frames, to-compact (plain
                                                   and --entropy) and to-wire, beside wire_decode_main on the same stream, the list twice
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from scalable_video_codec_amd import clip as clipmod  # noqa: E402
from scalable_video_codec_amd import configs, levels, native, pipeline, synth  # noqa: E402


def _cfg(argv, k):
    return {"C3": configs.C3, "C5": configs.C5}[argv[k] if len(argv) > k else "C3"]


def _batch(cfg, n):
    """n + 1 padded frames on the device and the pipeline's region ids for the n encoded ones."""
    dev = torch.device("cuda")
    clip = synth.SynthClip(cfg.width, cfg.height, n + 1, cfg.seed, device=dev)
    pw, ph = cfg.padded
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n + 1)]).contiguous()
    enc = pipeline.ClipEncoder(cfg, n + 1, dev)
    enc.load_frames(list(frames))
    enc.step()
    torch.cuda.synchronize()
    return frames[1:].contiguous(), enc.types.clone()


def kernels(cfg, fused_only=False) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, cfg.dct_block, cfg.mv_block)
    offs, offs2 = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    out2 = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws2 = torch.empty(native.dct_pack_levels_workspace_bytes(n, pw, ph, cfg.dct_block, cfg.mv_block), dtype=torch.uint8, device=dev)
    if not fused_only:
        planes = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        ws = torch.empty(native.pack_levels_workspace_bytes(n, pw, ph, cfg.dct_block), dtype=torch.uint8, device=dev)
        for _ in range(5):
            native.dct_quant_frames(bgr, cfg.dct_block, types, cfg.mv_block, cfg.fg_step, cfg.bg_step, out=planes)
            native.pack_levels_frames(planes, types, cfg.dct_block, cfg.mv_block, cfg.fg_step, cfg.bg_step, out=out, offsets=offs, workspace=ws)
    for _ in range(5):
        native.dct_pack_levels_frames(bgr, cfg.dct_block, types, cfg.mv_block, cfg.fg_step, cfg.bg_step, out=out2, offsets=offs2, workspace=ws2)
    torch.cuda.synchronize()
    total = int(offs2[-1].item())
    if not fused_only:
        assert torch.equal(offs, offs2) and torch.equal(out[:total], out2[:total]), "the fused route's bytes differ from the two calls'"
    print(f"{cfg.name} batch of {n}: {total} B compact ({total / n / 1e6:.3f} MB per frame), planes {3 * pw * ph * 4 / 1e6:.2f} MB per frame, "
          f"fused workspace {ws2.numel() / n / 1e6:.2f} MB per frame" + ("" if fused_only else "; fused bytes == two-call bytes"), flush=True)


def _budget(cfg):
    """The ladder and the bytes per frame of profiles/levels_budget_c3.txt (1.1 MB per 1080p frame, by the pixels elsewhere)."""
    pw, ph = cfg.padded
    return levels.step_ladder(1, 256, 4, 640, 10, 24), int(1_100_000 * (pw * ph) / (1920 * 1088)) // 16 * 16


def budget(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    bgr, types = _batch(cfg, n)
    lad, per_frame = _budget(cfg)
    b = native.budget_tensor(per_frame, n, dev)
    cap = native.levels_max_bytes(n, pw, ph, cfg.dct_block, cfg.mv_block)
    out2 = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws2 = torch.empty(native.dct_pack_levels_budget_workspace_bytes(n, pw, ph, cfg.dct_block, cfg.mv_block, len(lad)), dtype=torch.uint8, device=dev)
    planes = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(native.pack_levels_budget_workspace_bytes(n, pw, ph, cfg.dct_block, len(lad)), dtype=torch.uint8, device=dev)
    for _ in range(5):
        native.dct_frames(bgr, cfg.dct_block, out=planes)
        _, _, choice = native.pack_levels_budget_frames(planes, types, cfg.dct_block, cfg.mv_block, lad, b, out=out, offsets=offs, workspace=ws)
    for _ in range(5):
        _, offs2, choice2 = native.dct_pack_levels_budget_frames(bgr, cfg.dct_block, types, cfg.mv_block, lad, b, out=out2, workspace=ws2)
    torch.cuda.synchronize()
    total = int(offs2[-1].item())
    out.view(torch.int32)[offs[:-1] // 4 + 11] = 0  # `inexact`: the planes route counts its raw planes' coefficients, the fused calls write 0
    assert torch.equal(offs, offs2) and torch.equal(choice, choice2) and torch.equal(out[:total], out2[:total]), \
        "the budgeted fused call's bytes differ from the planes route's"
    sizes = (offs2[1:] - offs2[:-1]).cpu().tolist()
    ch = choice2.cpu().numpy().view("uint32")
    print(f"{cfg.name} batch of {n}: {len(lad)} entries, budget {per_frame} B per frame: choices {[int(c) & 0x7FFFFFFF for c in ch]}, over budget "
          f"{int((ch >> 31).sum())}, {min(sizes) / 1e6:.3f} .. {max(sizes) / 1e6:.3f} MB per frame, workspace {ws2.numel() / n / 1e6:.2f} MB per frame; "
          f"bytes, offsets and choices == the planes route's", flush=True)


def budget_step(cfg, frames_n) -> None:
    dev = torch.device("cuda")
    clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=dev)
    pw, ph = cfg.padded
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(frames_n)]).contiguous()
    lad, per_frame = _budget(cfg)
    for schedule, name in ((clipmod.SERIAL, "serial"), (clipmod.PIPELINED, "pipelined")):
        enc = clipmod.Clip(cfg, frames_n, schedule=schedule, compact=True)
        enc.load_frames(frames)
        fixed_ms = _per_step(enc.step, enc.sync)
        enc.set_compact_budget(lad, per_frame)
        budget_ms = _per_step(enc.step, enc.sync)
        ch = enc.read("compact_choice").numpy().view("uint32")
        enc.set_compact_budget([], 0)
        again_ms = _per_step(enc.step, enc.sync)
        i = enc.info
        enc.close()
        del enc
        torch.cuda.empty_cache()
        print(f"{cfg.name} {name}, {i.pairs} pairs, ms per step (best .. worst of 3 runs of 4 back-to-back steps): fixed compact step "
              f"{fixed_ms[0]:.3f} .. {fixed_ms[1]:.3f}; under a budget of {per_frame} B per frame {budget_ms[0]:.3f} .. {budget_ms[1]:.3f} "
              f"({budget_ms[0] / fixed_ms[0]:.2f}x; entries {int((ch & 0x7FFFFFFF).min())} .. {int((ch & 0x7FFFFFFF).max())}, over budget "
              f"{int((ch >> 31).sum())}); fixed again {again_ms[0]:.3f} .. {again_ms[1]:.3f}", flush=True)


def _still(bgr, types, pw, ph, mv):
    """delta_encode_sizes' static background (the first frame, repeated) under a moving 128 x 128 patch of the clip, foreground under it."""
    n = bgr.shape[0]
    mbw, mbh = native._bwbh(mv)
    still = bgr[:1].expand(n, ph, pw, 3).clone()
    still_types = torch.zeros_like(types).view(n, ph // mbh, pw // mbw)
    for f in range(n):
        x, y = 256 + 48 * f, 192 + 16 * f
        still[f, y:y + 128, x:x + 128] = bgr[f, y:y + 128, x:x + 128]
        still_types[f, y // mbh:(y + 128) // mbh, x // mbw:(x + 128) // mbw] = 1
    return still, still_types.reshape(n, -1).contiguous()


def quality(cfg, kernels_only=False) -> None:
    """The quality call at 40 dB and 30 dB against (a) the budgeted call with the same ladder and (b) the route a caller had before it: per
    entry the fixed fused pack, svc_hip_decode_levels_frames and a torch squared error.  One process, the routes in turn, the median of
    three rounds.  Then what the targets give on the synthetic clip and on the static background.  kernels_only: each call five times and
    nothing else, for a kernel trace."""
    from scalable_video_codec_amd import layers as lay
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    lad, per_frame = _budget(cfg)
    t40, t30 = (native.target_tensor(lay.distortion_target(db, pw, ph), n, dev) for db in (40.0, 30.0))
    b = native.budget_tensor(per_frame, n, dev)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, out2 = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    wsq = torch.empty(native.dct_pack_levels_quality_workspace_bytes(n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    wsb = torch.empty(native.dct_pack_levels_budget_workspace_bytes(n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    wsd = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev)
    src = bgr.float()

    def q40():
        return native.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, t40, out=out, workspace=wsq)

    def q30():
        return native.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, t30, out=out, workspace=wsq)

    def q40_cap_table():
        return native.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, t40, b, out=out, workspace=wsq, distortion=True)

    def budgeted():
        return native.dct_pack_levels_budget_frames(bgr, block, types, mv, lad, b, out=out, workspace=wsb)

    def before():  # per entry: encode, decode, compare pixels -> the table a caller had to make by hand (its units: squared pixel error)
        sse = []
        for fg, bg in lad:
            s, so = native.dct_pack_levels_frames(bgr, block, types, mv, int(fg), int(bg), out=out2, workspace=wsb)
            native.decode_levels_frames(s, so, pw, ph, block, mv, int(fg), int(bg), rec=rec, workspace=wsd)
            sse.append(((rec - src) ** 2).sum(dim=(1, 2, 3)))
        return torch.stack(sse, 1)

    if kernels_only:
        for fn in (q40, budgeted):
            for _ in range(5):
                fn()
        sync()
        return
    ms = _median3([q40, q30, q40_cap_table, budgeted], sync, steps=20)
    ms_before = _median3([before], sync, steps=2)[0]
    print(f"{cfg.name} batch of {n}, {len(lad)} entries, ms per call (median of 3 rounds of 20 back-to-back calls, the routes in turn): quality "
          f"call at 40 dB {ms[0]:.3f}, at 30 dB {ms[1]:.3f}, at 40 dB with a cap of {per_frame} B and the table {ms[2]:.3f}; (a) the budgeted call "
          f"{ms[3]:.3f} ({ms[0] / ms[3]:.2f}x: the price of measuring instead of counting); (b) {len(lad)} x (fixed fused pack + decode + torch "
          f"squared error) {ms_before:.3f} ({ms_before / ms[0]:.1f}x the quality call; 2 calls a round); quality workspace "
          f"{wsq.numel() / n / 1e6:.2f} MB per frame against {wsb.numel() / n / 1e6:.2f}", flush=True)
    # the table against route (b)'s, the scale check at full size
    _, _, _, table = q40_cap_table()
    by_hand = before()
    sync()
    d = table.cpu().numpy().view("uint64").astype("float64") / 65536.0
    rel = abs(d - by_hand.double().cpu().numpy()) / by_hand.double().cpu().numpy().clip(min=1.0)
    print(f"  the call's table / 65536 against route (b)'s squared pixel errors (f32 sums of the clipped-free f32 reconstruction): worst relative "
          f"difference {rel.max():.2e}", flush=True)

    def coded_bytes(stream, so):
        _, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
        sync()
        assert not est.any()
        return int(eo[-1])

    still, still_types = _still(bgr, types, pw, ph, mv)
    for clip_name, frames, ty in (("the synthetic clip", bgr, types), ("a static background under a moving 128 x 128 patch", still, still_types)):
        for db, t in ((40.0, t40), (30.0, t30)):
            s, so, ch, tab = native.dct_pack_levels_quality_frames(frames, block, ty, mv, lad, t, distortion=True)
            sync()
            ch, tab = ch.cpu().numpy().view("uint32"), tab.cpu().numpy().view("uint64")
            picks = [int(c) & 0x3FFFFFFF for c in ch]
            psnr = [lay.distortion_psnr(tab[f, k], pw, ph) for f, k in enumerate(picks)]
            raw = int(so[-1])
            print(f"  {clip_name} at {db:g} dB: entries {min(picks)} .. {max(picks)} (steps {tuple(int(v) for v in lad[min(picks)])} .. "
                  f"{tuple(int(v) for v in lad[max(picks)])}), target not met in {int(((ch >> 30) & 1).sum())} frames, PSNR reached "
                  f"{min(psnr):.2f} .. {max(psnr):.2f} dB, {raw / n / 1e6:.4f} MB per frame raw, {coded_bytes(s[:raw], so) / n / 1e6:.4f} "
                  f"entropy-coded", flush=True)


def delta_budget(cfg, kernels_only=False) -> None:
    """svc_hip_dct_pack_delta_budget_frames, a batch of 16 with a key frame every 8 and the 32-entry ladder, against (a) the route a caller
    had before it -- per entry svc_hip_dct_pack_delta_frames to read the sizes (all offsets fetched in one copy), then one more at the
    chosen steps --, (b) svc_hip_dct_pack_delta_frames at fixed steps and (c) svc_hip_dct_pack_levels_budget_frames.  One process, the
    routes in turn, the median of three rounds.  Then what it buys: entries, bytes and PSNR (the quality call's table) of this call and
    of the per-frame budgeted plain stream at the same budgets, on the synthetic clip and on the static background.  kernels_only: this
    call and the quality call five times each and nothing else, for a kernel trace."""
    import numpy as np
    from scalable_video_codec_amd import layers as lay
    dev = torch.device("cuda")
    n, interval = 16, 8
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    lad, per_frame = _budget(cfg)
    key = torch.tensor([int(f % interval == 0) for f in range(n)], dtype=torch.int32, device=dev)
    b = native.budget_tensor(per_frame, n, dev)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, out2 = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    wsg = torch.empty(native.dct_pack_delta_budget_workspace_bytes(n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    wsd = torch.empty(native.dct_pack_delta_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    wsb = torch.empty(native.dct_pack_levels_budget_workspace_bytes(n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    wsq = torch.empty(native.dct_pack_levels_quality_workspace_bytes(n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    all_offs = torch.empty((len(lad), n + 1), dtype=torch.int64, device=dev)
    top = native.target_tensor(2 ** 64 - 1, n, dev)

    def group_call(frames=bgr, ty=types, budget=b, counts=False):
        return native.dct_pack_delta_budget_frames(frames, block, ty, mv, lad, budget, key=key, out=out, workspace=wsg, counts=counts)

    def by_hand():  # (a): every entry's delta stream for its sizes, the choice on the host, one more encode
        for k, (fg, bg) in enumerate(lad):
            native.dct_pack_delta_frames(bgr, block, types, mv, int(fg), int(bg), key=key, out=out2, offsets=all_offs[k], workspace=wsd)
        sizes = np.diff(all_offs.cpu().numpy(), axis=1)  # (entries, frames)
        for g in range(0, n, interval):
            fits = [k for k in range(len(lad)) if sizes[k, g:g + interval].sum() <= per_frame * interval]
            fg, bg = (int(v) for v in lad[fits[0] if fits else len(lad) - 1])
            native.dct_pack_delta_frames(bgr[g:g + interval], block, types[g:g + interval], mv, fg, bg, out=out2, workspace=wsd)

    def fixed():
        return native.dct_pack_delta_frames(bgr, block, types, mv, cfg.fg_step, cfg.bg_step, key=key, out=out2, workspace=wsd)

    def plain_budgeted(frames=bgr, ty=types, budget=b):
        return native.dct_pack_levels_budget_frames(frames, block, ty, mv, lad, budget, out=out2, workspace=wsb)

    def quality_call():
        return native.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, top, out=out2, workspace=wsq)

    if kernels_only:
        for fn in (group_call, quality_call):
            for _ in range(5):
                fn()
        sync()
        return
    ms = _median3([group_call, fixed, plain_budgeted, quality_call], sync, steps=20)
    ms_hand = _median3([by_hand], sync, steps=2)[0]
    print(f"{cfg.name} batch of {n}, a key frame every {interval}, {len(lad)} entries, {per_frame} B per frame; ms per call (median of 3 rounds of "
          f"20 back-to-back calls, the routes in turn): the group-budget call {ms[0]:.3f}; (a) {len(lad)} x svc_hip_dct_pack_delta_frames + one "
          f"copy of the offsets + one more encode per group {ms_hand:.3f} ({ms_hand / ms[0]:.1f}x; 2 calls a round); (b) "
          f"svc_hip_dct_pack_delta_frames at ({cfg.fg_step}, {cfg.bg_step}) {ms[1]:.3f} (the price of choosing: {ms[0] / ms[1]:.2f}x); (c) "
          f"svc_hip_dct_pack_levels_budget_frames {ms[2]:.3f} ({ms[0] / ms[2]:.2f}x); the quality call {ms[3]:.3f}; workspace "
          f"{wsg.numel() / n / 1e6:.2f} MB per frame against {wsd.numel() / n / 1e6:.2f} (delta) and {wsb.numel() / n / 1e6:.2f} (budgeted)", flush=True)

    still, still_types = _still(bgr, types, pw, ph, mv)
    for clip_name, frames, ty in (("the synthetic clip", bgr, types), ("a static background under a moving 128 x 128 patch", still, still_types)):
        _, _, _, dist = native.dct_pack_levels_quality_frames(frames, block, ty, mv, lad, top, workspace=wsq, distortion=True)
        sync()
        dist = dist.cpu().numpy().view("uint64")
        for percent in (100, 92, 85):  # (the masks alone are 74 % of the C3 budget: a frame has a floor no step gets under)
            budget = native.budget_tensor(per_frame * percent // 100 // 16 * 16, n, dev)
            _, so, ch = group_call(frames, ty, budget)
            sync()
            ch, total = ch.cpu().numpy().view("uint32"), int(so[-1])
            picks = [int(c) & 0x7FFFFFFF for c in ch]
            psnr = [lay.distortion_psnr(dist[f, k], pw, ph) for f, k in enumerate(picks)]
            _, po, pch = plain_budgeted(frames, ty, budget)
            sync()
            pch, ptotal = pch.cpu().numpy().view("uint32"), int(po[-1])
            ppicks = [int(c) & 0x7FFFFFFF for c in pch]
            ppsnr = [lay.distortion_psnr(dist[f, k], pw, ph) for f, k in enumerate(ppicks)]
            print(f"  {clip_name}, {per_frame * percent // 100 // 16 * 16} B per frame: this call entries {[picks[g] for g in range(0, n, interval)]} per group "
                  f"(steps {[tuple(int(v) for v in lad[picks[g]]) for g in range(0, n, interval)]}), over budget {int((ch >> 31).sum())} frames, "
                  f"{total / n / 1e6:.4f} MB per frame, PSNR {min(psnr):.2f} .. {max(psnr):.2f} dB (mean {sum(psnr) / n:.2f}); the per-frame budgeted "
                  f"plain stream entries {min(ppicks)} .. {max(ppicks)}, over budget {int((pch >> 31).sum())} frames, {ptotal / n / 1e6:.4f} MB per "
                  f"frame, PSNR {min(ppsnr):.2f} .. {max(ppsnr):.2f} dB (mean {sum(ppsnr) / n:.2f})", flush=True)


def _delta_quality_two_pass_lib():
    """csrc/dct_pack.hip built with both tables from two passes (SVC_DCT_PACK_DELTA_QUALITY_TWO_PASS=1), as _measure_variant_lib builds its
    variant -> (the call, the workspace query)."""
    import ctypes
    import subprocess
    from scalable_video_codec_amd import build
    out = os.path.join(ROOT, "tools", "_bin", "libsvc_dct_pack_delta_quality_two_pass.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build._hipcc(), *build.HIPCC_FLAGS, "-DSVC_DCT_PACK_DELTA_QUALITY_TWO_PASS=1", "-shared", "-o", out,
                               os.path.join(build.CSRC, "dct_pack.hip"), f"-L{build.PKG}", "-lsvc_hip", f"-Wl,-rpath,{build.PKG}"])
    native.load()  # (first: the variant resolves the shared helpers in it)
    lib = ctypes.CDLL(out)
    for name, (res, args) in native.SIGNATURES_DELTA_QUALITY.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib.svc_hip_dct_pack_delta_quality_frames, lib.svc_hip_dct_pack_delta_quality_workspace_bytes


def delta_quality(cfg, kernels_only=False) -> None:
    """svc_hip_dct_pack_delta_quality_frames, a batch of 16 with a key frame every 8 and the 32-entry ladder, at 40 dB with both tables asked
    for, against (a) the two-pass build of the same call, (b) the route a caller had before it and (c) the delta-budget call alone.  One
    process, the routes in turn, the median of three rounds; the two builds' outputs are compared.  Then what the targets give.
    kernels_only: the call five times and nothing else, for a kernel trace."""
    from scalable_video_codec_amd import layers as lay
    dev = torch.device("cuda")
    n, interval = 16, 8
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    lad, per_frame = _budget(cfg)
    arr, k = native._ladder(lad)
    key = torch.tensor([int(f % interval == 0) for f in range(n)], dtype=torch.int32, device=dev)
    b = native.budget_tensor(per_frame, n, dev)
    t40, t30 = (native.target_tensor(lay.distortion_target(db, pw, ph), n, dev) for db in (40.0, 30.0))
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, out2 = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    ws = torch.empty(native.dct_pack_delta_quality_workspace_bytes(n, pw, ph, block, mv, k), dtype=torch.uint8, device=dev)
    wsg = torch.empty(native.dct_pack_delta_budget_workspace_bytes(n, pw, ph, block, mv, k), dtype=torch.uint8, device=dev)
    wsq = torch.empty(native.dct_pack_levels_quality_workspace_bytes(n, pw, ph, block, mv, k), dtype=torch.uint8, device=dev)

    def call(frames=bgr, ty=types, target=t40, budget=None):
        return native.dct_pack_delta_quality_frames(frames, block, ty, mv, lad, target, budget, key=key, out=out, workspace=ws, counts=True,
                                                    distortion=True)

    if kernels_only:
        for _ in range(5):
            call()
        sync()
        return
    two_pass, two_pass_bytes = _delta_quality_two_pass_lib()
    ws2 = torch.empty(two_pass_bytes(n, pw, ph, block, mbw, mbh, k), dtype=torch.uint8, device=dev)
    res2 = (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
            torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev))

    def call_two_pass():
        offs, ch, ct, dt = res2
        native._check(two_pass(bgr.data_ptr(), pw * ph * 3, n, pw, ph, block, types.data_ptr(), mbw, mbh, arr, k, key.data_ptr(), t40.data_ptr(), None,
                               ws2.data_ptr(), ws2.numel(), out2.data_ptr(), out2.numel(), offs.data_ptr(), ch.data_ptr(), ct.data_ptr(),
                               dt.data_ptr(), native._stream()))

    def group_budget():
        return native.dct_pack_delta_budget_frames(bgr, block, types, mv, lad, b, key=key, out=out2, workspace=wsg, counts=True)

    def before():  # (b): both tables from two calls; the host would choose here; the encode at the chosen steps costs a third call
        native.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, t40, out=out2, workspace=wsq, distortion=True)
        group_budget()
        group_budget()

    ms = _median3([call, call_two_pass, before, group_budget], sync, steps=20)
    call_two_pass()  # (last into out2: the routes above share it)
    got = call()
    sync()
    used = int(got[1][-1])
    same = all(torch.equal(a, r) for a, r in zip(got[1:], res2)) and torch.equal(got[0][:used], out2[:used])
    print(f"{cfg.name} batch of {n}, a key frame every {interval}, {k} entries, 40 dB, both tables; ms per call (median of 3 rounds of 20 "
          f"back-to-back calls, the routes in turn): the call (one pass) {ms[0]:.3f}; (a) the two-pass build {ms[1]:.3f} ({ms[1] / ms[0]:.2f}x; "
          f"tables, choices, offsets and bytes {'equal' if same else 'DIFFER'}); (b) quality call + delta-budget call + one more delta-budget "
          f"call {ms[2]:.3f} ({ms[2] / ms[0]:.2f}x); (c) svc_hip_dct_pack_delta_budget_frames alone {ms[3]:.3f} (the price of the second table: "
          f"{ms[0] / ms[3]:.2f}x); workspace {ws.numel() / n / 1e6:.2f} MB per frame against {ws2.numel() / n / 1e6:.2f} (two passes) and "
          f"{wsg.numel() / n / 1e6:.2f} (delta-budget)", flush=True)

    def coded_bytes(stream, so):
        _, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
        sync()
        assert not est.any()
        return int(eo[-1])

    still, still_types = _still(bgr, types, pw, ph, mv)
    for clip_name, frames, ty in (("the synthetic clip", bgr, types), ("a static background under a moving 128 x 128 patch", still, still_types)):
        for db, t in ((40.0, t40), (30.0, t30)):
            s, so, ch, _, tab = call(frames, ty, t)
            sync()
            ch, tab, raw = ch.cpu().numpy().view("uint32"), tab.cpu().numpy().view("uint64"), int(so[-1])
            picks = [int(c) & 0x3FFFFFFF for c in ch]
            psnr = [lay.distortion_psnr(tab[f, kk], pw, ph) for f, kk in enumerate(picks)]
            coded = coded_bytes(s[:raw].clone(), so.clone())
            ps, pso, pch = native.dct_pack_levels_quality_frames(frames, block, ty, mv, lad, t, out=out2, workspace=wsq)
            sync()
            pch, praw = pch.cpu().numpy().view("uint32"), int(pso[-1])
            ppicks = [int(c) & 0x3FFFFFFF for c in pch]
            ppsnr = [lay.distortion_psnr(tab[f, kk], pw, ph) for f, kk in enumerate(ppicks)]
            print(f"  {clip_name} at {db:g} dB: this call entries {[picks[g] for g in range(0, n, interval)]} per group (steps "
                  f"{[tuple(int(v) for v in lad[picks[g]]) for g in range(0, n, interval)]}), target not met in {int(((ch >> 30) & 1).sum())} "
                  f"frames, PSNR {min(psnr):.2f} .. {max(psnr):.2f} dB, {raw / n / 1e6:.4f} MB per frame raw, {coded / n / 1e6:.4f} entropy-coded; "
                  f"the per-frame plain quality call entries {min(ppicks)} .. {max(ppicks)}, not met in {int(((pch >> 30) & 1).sum())}, PSNR "
                  f"{min(ppsnr):.2f} .. {max(ppsnr):.2f} dB, {praw / n / 1e6:.4f} MB per frame raw, {coded_bytes(ps[:praw], pso) / n / 1e6:.4f} "
                  f"entropy-coded ({praw / raw:.2f}x the bytes of this call)", flush=True)


def _measure_variant_lib(share):
    """csrc/dct_pack.hip built with the other form of the measuring loop (SVC_DCT_PACK_MEASURE_SHARE), as _delta_run_lib builds its runs."""
    import ctypes
    import subprocess
    from scalable_video_codec_amd import build
    out = os.path.join(ROOT, "tools", "_bin", f"libsvc_dct_pack_measure_share{share}.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build._hipcc(), *build.HIPCC_FLAGS, f"-DSVC_DCT_PACK_MEASURE_SHARE={share}", "-shared", "-o", out,
                               os.path.join(build.CSRC, "dct_pack.hip"), f"-L{build.PKG}", "-lsvc_hip", f"-Wl,-rpath,{build.PKG}"])
    native.load()  # (first: the variant resolves the shared helpers in it)
    fn = ctypes.CDLL(out).svc_hip_dct_pack_levels_quality_frames
    fn.restype, fn.argtypes = native.SIGNATURES_QUALITY["svc_hip_dct_pack_levels_quality_frames"]
    return fn


def quality_variants(cfg) -> None:
    """The quality call as built against the build that computes every ladder entry, with the 32-entry ladder (11 background steps, then 21
    foreground steps) and with 32 entries that all differ in both classes; same tables and bytes."""
    from scalable_video_codec_amd import layers as lay
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    bgr, types = _batch(cfg, n)
    every = _measure_variant_lib(0)
    t40 = native.target_tensor(lay.distortion_target(40.0, pw, ph), n, dev)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    ladders = (("levels.step_ladder(1, 256, 4, 640, 10, 24)", _budget(cfg)[0]), ("32 entries, both steps rising at each", [(k + 1, 4 + 20 * k) for k in range(32)]))
    for name, lad in ladders:
        arr, k = native._ladder(lad)
        ws = torch.empty(native.dct_pack_levels_quality_workspace_bytes(n, pw, ph, block, mv, k), dtype=torch.uint8, device=dev)
        res = []
        for _ in range(2):
            res.append((torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev),
                        torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev)))

        def call(fn, r):
            out, offs, ch, tab = r
            native._check(fn(bgr.data_ptr(), pw * ph * 3, n, pw, ph, block, types.data_ptr(), mbw, mbh, arr, k, t40.data_ptr(), None, ws.data_ptr(),
                             ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), ch.data_ptr(), tab.data_ptr(), native._stream()))
        ms = _median3([lambda: call(native.load().svc_hip_dct_pack_levels_quality_frames, res[0]), lambda: call(every, res[1])],
                      torch.cuda.synchronize)
        used = int(res[0][1][-1])
        same = all(torch.equal(a, b) for a, b in zip(res[0][1:], res[1][1:])) and torch.equal(res[0][0][:used], res[1][0][:used])
        print(f"{cfg.name} batch of {n}, {name}: the call as built {ms[0]:.3f} ms, every entry computed {ms[1]:.3f} ms ({ms[1] / ms[0]:.2f}x); "
              f"tables, choices, offsets and bytes {'equal' if same else 'DIFFER'}", flush=True)


def quality_step(cfg, frames_n) -> None:
    from scalable_video_codec_amd import layers as lay
    dev = torch.device("cuda")
    clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=dev)
    pw, ph = cfg.padded
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(frames_n)]).contiguous()
    lad, per_frame = _budget(cfg)
    for schedule, name in ((clipmod.SERIAL, "serial"), (clipmod.PIPELINED, "pipelined")):
        enc = clipmod.Clip(cfg, frames_n, schedule=schedule, compact=True)
        enc.load_frames(frames)
        fixed_ms = _per_step(enc.step, enc.sync)
        enc.set_compact_budget(lad, per_frame)
        budget_ms = _per_step(enc.step, enc.sync)
        enc.set_compact_quality(lad, psnr_db=40.0)
        quality_ms = _per_step(enc.step, enc.sync)
        ch = enc.read("compact_choice").numpy().view("uint32")
        dist = enc.read("compact_distortion").numpy().view("uint64")
        enc.set_compact_quality([], target=0)
        again_ms = _per_step(enc.step, enc.sync)
        i = enc.info
        enc.close()
        del enc
        torch.cuda.empty_cache()
        psnr = [lay.distortion_psnr(v, pw, ph) for v in dist]
        print(f"{cfg.name} {name}, {i.pairs} pairs, ms per step (best .. worst of 3 runs of 4 back-to-back steps): fixed compact step "
              f"{fixed_ms[0]:.3f} .. {fixed_ms[1]:.3f}; under a budget of {per_frame} B per frame {budget_ms[0]:.3f} .. {budget_ms[1]:.3f}; at a "
              f"40 dB target {quality_ms[0]:.3f} .. {quality_ms[1]:.3f} ({quality_ms[0] / fixed_ms[0]:.2f}x the fixed step, "
              f"{quality_ms[0] / budget_ms[0]:.2f}x the budgeted; entries {int((ch & 0x3FFFFFFF).min())} .. {int((ch & 0x3FFFFFFF).max())}, "
              f"{min(psnr):.2f} .. {max(psnr):.2f} dB); fixed again {again_ms[0]:.3f} .. {again_ms[1]:.3f}", flush=True)


def _per_step(fn, sync, warm=2, reps=3, steps=4):
    """Wall ms per call of fn over `steps` back-to-back calls and one sync; the best and the worst of `reps` such runs."""
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3 / steps)
    return min(ts), max(ts)


def layers(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    base, fine, lbase, lenh = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4))
    offs_b, offs_f = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    ws1 = torch.empty(native.dct_pack_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(native.dct_pack_layers_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    sync = torch.cuda.synchronize

    def one(fg, bg, out, offs):
        return native.dct_pack_levels_frames(bgr, block, types, mv, fg, bg, out=out, offsets=offs, workspace=ws1)

    def two(fg, bg, enh, window=None):
        return native.dct_pack_layers_frames(bgr, block, types, mv, fg, bg, enh, window=window, base_out=lbase, enh_out=lenh, workspace=ws2)

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    print(f"{cfg.name} batch of {n}, ms per call (best .. worst of 3 runs of 4 back-to-back calls)", flush=True)
    for fg, bg, enh in ((1, 640, 1), (16, 16, 1)):  # (a)
        t_base = _per_step(lambda: one(fg, bg, base, offs_b), sync)
        t_fine = _per_step(lambda: one(enh, enh, fine, offs_f), sync)
        t_two = _per_step(lambda: two(fg, bg, enh), sync)
        _, lo_b, _, _ = two(fg, bg, enh)
        sync()
        used = int(offs_b[-1])
        assert torch.equal(lo_b, offs_b) and torch.equal(lbase[:used], base[:used]), "the base layer differs from the one-layer call's stream"
        print(f"(a) encode ({fg}, {bg}, {enh}): one layer at ({fg}, {bg}) {fmt(t_base)} + at ({enh}, {enh}) {fmt(t_fine)} = "
              f"{t_base[0] + t_fine[0]:.3f} .. {t_base[1] + t_fine[1]:.3f}; two layers {fmt(t_two)} "
              f"({t_two[0] / (t_base[0] + t_fine[0]):.2f} of the sum); same base bytes", flush=True)

    # (b), (c): the streams at (1, 640, 1)
    one(1, 640, base, offs_b)
    one(1, 1, fine, offs_f)
    _, _, _, offs_e = two(1, 640, 1)
    sync()
    ub, uf, ue = int(offs_b[-1]), int(offs_f[-1]), int(offs_e[-1])
    rec_f, rec_l = (torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev) for _ in range(2))
    wsd1 = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    wsd2 = torch.empty(native.decode_layers_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    small = native.gaze_rect(cfg.width // 2, cfg.height // 2, 64, 64, cfg.width, cfg.height, pw, ph)
    for name, rect in (("64 x 64", small), ("the whole frame", (0, 0, pw, ph))):
        gaze = torch.tensor([rect] * n, dtype=torch.int32, device=dev)
        t_f = _per_step(lambda: native.decode_levels_frames(fine[:uf], offs_f, pw, ph, block, mv, 1, 640, gaze=gaze, rec=rec_f, workspace=wsd1), sync)
        t_l = _per_step(lambda: native.decode_layers_frames(lbase[:ub], offs_b, lenh[:ue], offs_e, pw, ph, block, mv, 1, 640, gaze=gaze,
                                                            rec=rec_l, workspace=wsd2), sync)
        same = "" if rect[2] != pw else ("; same d_rec" if torch.equal(rec_f.view(torch.int32), rec_l.view(torch.int32)) else "; d_rec DIFFERS")
        print(f"(b) decode, gaze {name} {tuple(rect)}: fine stream {fmt(t_f)}; two layers {fmt(t_l)} ({t_l[0] / t_f[0]:.2f}x){same}", flush=True)

    def coded(stream, offs, used):
        _, co, st = native.entropy_encode_frames(stream[:used], offs, pw, ph, block, mv)
        sync()
        assert not st.any()
        return int(co[-1])

    rows = [("base (1, 640)", ub, coded(base, offs_b, ub)), ("single stream (1, 1)", uf, coded(fine, offs_f, uf)),
            ("enhancement, no window", ue, coded(lenh, offs_e, ue))]
    wx, wy = (pw - 256) // 2 // 16 * 16, (ph - 256) // 2 // 16 * 16
    _, _, _, offs_w = two(1, 640, 1, window=[(wx, wy, 256, 256)] * n)
    sync()
    uw = int(offs_w[-1])
    rows.append((f"enhancement, window 256 x 256 at ({wx}, {wy})", uw, coded(lenh, offs_w, uw)))
    for name, raw, ent in rows:
        print(f"(c) {name}: {raw / n / 1e6:.3f} MB per frame raw, {ent / n / 1e6:.3f} MB entropy-coded", flush=True)


def window(cfg) -> None:
    dev = torch.device("cuda")
    n, viewers = 16, 4
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    lbase, whole, enc = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
    ws2 = torch.empty(native.dct_pack_layers_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    sync = torch.cuda.synchronize

    def encode(out, win):
        return native.dct_pack_layers_frames(bgr, block, types, mv, 1, 640, 1, window=win, base_out=lbase, enh_out=out, workspace=ws2)

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    def rects(viewer):
        """A 256 x 256 window per frame, on the MV grid, drifting with the frame and different for each viewer."""
        out = []
        for f in range(n):
            x = (pw - 256) // 2 + 32 * ((f + 3 * viewer) % 7 - 3) + 64 * (viewer - 1)
            y = (ph - 256) // 2 + 16 * ((f + viewer) % 5 - 2)
            out.append((x // 16 * 16, y // 16 * 16, 256, 256))
        return out

    _, _, _, offs_e = encode(whole, None)
    sync()
    offs_e = offs_e.clone()
    ue = int(offs_e[-1])
    stored = whole[:ue]
    win = torch.tensor(rects(0), dtype=torch.int32, device=dev)
    out1 = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws1 = torch.empty(native.window_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st1 = torch.empty(n, dtype=torch.int32, device=dev)
    oo1 = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def serve():
        return native.window_levels_frames(stored, offs_e, pw, ph, block, mv, window=win, out=out1, out_offsets=oo1, workspace=ws1, status=st1)

    print(f"{cfg.name} batch of {n}, enhancement at (1, 640, 1), ms per call (best .. worst of 3 runs of 20 back-to-back calls)", flush=True)
    t_enc = _per_step(lambda: encode(enc, win), sync, steps=20)
    t_win = _per_step(serve, sync, steps=20)
    t_enc2 = _per_step(lambda: encode(enc, win), sync, steps=20)  # the encode again, after: the spread of the same call in this run
    _, _, _, offs_w = encode(enc, win)
    serve()
    sync()
    uw = int(offs_w[-1])
    assert not st1.any() and torch.equal(oo1, offs_w) and torch.equal(out1[:uw], enc[:uw]), "the windowed stream differs from the encoder's"
    print(f"(a) one viewer, 256 x 256 per frame: encode with the window {fmt(t_enc)} (again {fmt(t_enc2)}); window the stored stream "
          f"{fmt(t_win)} ({t_win[0] / min(t_enc[0], t_enc2[0]):.3f} of the encode); same bytes; stored {ue / n / 1e6:.3f} MB per frame, "
          f"served {uw / n / 1e6:.3f} MB per frame, workspace {ws1.numel() / n / 1e6:.3f} MB per frame", flush=True)

    # 4 viewers of the same 16 stored frames
    n_out = viewers * n
    src = torch.tensor([f for _ in range(viewers) for f in range(n)], dtype=torch.int32, device=dev)
    win4 = torch.tensor([r for v in range(viewers) for r in rects(v)], dtype=torch.int32, device=dev)
    out4 = torch.empty(native.levels_max_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws4 = torch.empty(native.window_levels_workspace_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st4 = torch.empty(n_out, dtype=torch.int32, device=dev)
    oo4 = torch.empty(n_out + 1, dtype=torch.int64, device=dev)

    def serve4():
        return native.window_levels_frames(stored, offs_e, pw, ph, block, mv, window=win4, src=src, out=out4, out_offsets=oo4, workspace=ws4,
                                           status=st4)

    def encode4():
        for v in range(viewers):
            encode(enc, win4[v * n:(v + 1) * n])

    t_enc4 = _per_step(encode4, sync, steps=20)
    t_win4 = _per_step(serve4, sync, steps=20)
    serve4()
    sync()
    assert not st4.any()
    for v in range(viewers):
        _, _, _, offs_v = encode(enc, win4[v * n:(v + 1) * n])
        sync()
        lo, hi = int(oo4[v * n]), int(oo4[(v + 1) * n])
        assert torch.equal(oo4[v * n:(v + 1) * n + 1] - lo, offs_v) and torch.equal(out4[lo:hi], enc[:hi - lo]), f"viewer {v} differs"
    print(f"(b) {viewers} viewers, n_out = {n_out} through d_src: {viewers} encodes {fmt(t_enc4)}; one window call {fmt(t_win4)} "
          f"({t_win4[0] / t_enc4[0]:.3f} of the encodes); same bytes; served {int(oo4[-1]) / n_out / 1e6:.3f} MB per frame", flush=True)


DELTA_RUNS = (1, 2, 4, 8)


def _delta_run_lib(run):
    """csrc/dct_pack.hip built with runs of `run` frames, as a small library of its own beside libsvc_hip.so (whose other symbols it
    uses); built once, into tools/_bin (git-ignored)."""
    import ctypes
    import subprocess
    from scalable_video_codec_amd import build
    out = os.path.join(ROOT, "tools", "_bin", f"libsvc_dct_pack_delta_run{run}.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build._hipcc(), *build.HIPCC_FLAGS, f"-DSVC_DCT_PACK_DELTA_RUN={run}", "-shared", "-o", out,
                               os.path.join(build.CSRC, "dct_pack.hip"), f"-L{build.PKG}", "-lsvc_hip", f"-Wl,-rpath,{build.PKG}"])
    native.load()  # (first: the variant resolves the shared helpers in it)
    lib = ctypes.CDLL(out)
    fn = lib.svc_hip_dct_pack_delta_frames
    fn.restype, fn.argtypes = native.SIGNATURES["svc_hip_dct_pack_delta_frames"]
    return fn


def _median3(fns, sync, steps=20):
    """Wall ms per call of each fn over `steps` back-to-back calls and one sync: three rounds over the whole list in turn, the median
    of each fn's three."""
    for fn in fns:
        fn()
    sync()
    ts = [[] for _ in fns]
    for _ in range(3):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            sync()
            ts[i].append((time.perf_counter() - t0) * 1e3 / steps)
    return [sorted(t)[1] for t in ts]


def delta_encode_kernels(cfg, runs) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    sync = torch.cuda.synchronize
    all_bgr, all_types = _batch(cfg, n + 1)  # the frame before, and the 16 of the batch
    bgr, types = all_bgr[1:], all_types[1:]
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, plain, ref = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
    offs, plain_offs, ref_offs = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3))
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(native.dct_pack_delta_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(native.delta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(native.pack_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    planes = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
    key16 = torch.zeros(n, dtype=torch.int32, device=dev)
    key16[0] = 1
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, ms per call (20 back-to-back calls, the routes in turn, the median of three rounds)",
          flush=True)
    for fg, bg in ((1, 640), (1, 1)):
        prev_q, prev_qo = native.dct_pack_levels_frames(all_bgr[:1], block, all_types[:1], mv, fg, bg)
        sync()
        prev_q = prev_q[:int(prev_qo[-1])].clone()
        for name, prev_bgr, prev_types, prev_svcq, key in (("a key frame every 16", None, None, None, key16),
                                                          ("the frame before given, no key frame", all_bgr[0], all_types[0], prev_q, None)):
            def new(fn):
                def call():
                    native._check(fn(bgr.data_ptr(), pw * ph * 3, n, pw, ph, block, types.data_ptr(), mbw, mbh, fg, bg,
                                     None if prev_bgr is None else prev_bgr.data_ptr(), None if prev_types is None else prev_types.data_ptr(),
                                     None if key is None else key.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                                     offs.data_ptr(), native._stream()))
                return call

            def fused():
                native.dct_pack_levels_frames(bgr, block, types, mv, fg, bg, out=plain, offsets=plain_offs, workspace=ws)

            def delta_call():
                native.delta_levels_frames(plain, plain_offs, pw, ph, block, mv, prev=prev_svcq, key=key, out=ref, out_offsets=ref_offs,
                                           workspace=ws_d, status=st)

            def fused_delta():
                fused()
                delta_call()

            def planes_delta():
                native.dct_quant_frames(bgr, block, types, mv, fg, bg, out=planes)
                native.pack_levels_frames(planes, types, block, mv, fg, bg, out=plain, offsets=plain_offs, workspace=ws_p)
                delta_call()

            fused_delta()
            sync()
            used = int(ref_offs[-1])
            assert not st.any()
            for r, fn in runs.items():
                out.fill_(0xA5)
                new(fn)()
                sync()
                assert torch.equal(offs, ref_offs) and torch.equal(out[:used], ref[:used]), f"runs of {r}: the bytes differ from the two calls'"
            t = _median3([new(fn) for fn in runs.values()] + [fused, fused_delta, planes_delta], sync)
            t_runs, (t_fused, t_two, t_planes) = dict(zip(runs, t)), t[len(runs):]
            best = min(t_runs, key=t_runs.get)
            print(f"  ({fg}, {bg}), {name}: svc_hip_dct_pack_delta_frames with runs of "
                  + ", ".join(f"{r}: {t_runs[r]:.3f}" for r in runs) + f" (the fastest: {best}); svc_hip_dct_pack_levels_frames alone {t_fused:.3f}; "
                  f"+ svc_hip_delta_levels_frames {t_two:.3f}; the planes route + svc_hip_delta_levels_frames {t_planes:.3f}; "
                  f"delta stream {used / n / 1e6:.4f} MB per frame, plain {int(plain_offs[-1]) / n / 1e6:.4f}; same bytes at every run length",
                  flush=True)


def delta_encode_sizes(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    # a static background (the first frame, repeated) under a moving 128 x 128 patch of the clip; foreground under the patch
    still = bgr[:1].expand(n, ph, pw, 3).clone()
    still_types = torch.zeros_like(types).view(n, ph // mbh, pw // mbw)
    for f in range(n):
        x, y = 256 + 48 * f, 192 + 16 * f  # (on the MV grid at both sizes)
        still[f, y:y + 128, x:x + 128] = bgr[f, y:y + 128, x:x + 128]
        still_types[f, y // mbh:(y + 128) // mbh, x // mbw:(x + 128) // mbw] = 1
    still_types = still_types.reshape(n, -1).contiguous()
    key = [1] + [0] * (n - 1)

    def coded_bytes(stream, so):
        _, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
        sync()
        assert not est.any()
        return int(eo[-1])

    print(f"{cfg.name} batch of {n}, frame 0 the key frame; MB per frame raw / entropy-coded", flush=True)
    for clip_name, frames, ty in (("the synthetic clip (fresh noise every frame)", bgr, types),
                                  ("a static background under a moving 128 x 128 patch", still, still_types)):
        for fg, bg in ((1, 640), (1, 1)):
            p, po = native.dct_pack_levels_frames(frames, block, ty, mv, fg, bg)
            d, do = native.dct_pack_delta_frames(frames, block, ty, mv, fg, bg, key=key)
            sync()
            p, d = p[:int(po[-1])], d[:int(do[-1])]
            raw, craw, draw, dcoded = p.numel(), coded_bytes(p, po), d.numel(), coded_bytes(d, do)
            k0 = int(po[1])
            print(f"  {clip_name} at ({fg}, {bg}): plain {raw / n / 1e6:.4f} / {craw / n / 1e6:.4f}, delta {draw / n / 1e6:.4f} / "
                  f"{dcoded / n / 1e6:.4f} ({draw / raw:.3f}x / {dcoded / craw:.3f}x); the 15 difference frames alone "
                  f"{(draw - k0) / 15 / 1e6:.4f} raw against {(raw - k0) / 15 / 1e6:.4f}", flush=True)


def delta_encode_stream(frames_n=33) -> None:
    import subprocess
    import tempfile
    cfg = configs.C3
    exe = os.path.join(ROOT, "tests", "dropin", "stream_delta_encode_main")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=torch.device("cuda"))
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(frames_n):
                f.write(clip.frame_bgr(t).cpu().numpy().tobytes())
        del clip
        torch.cuda.empty_cache()
        print(f"{cfg.name}, {frames_n} frames from host memory through svc::StreamEncoder (tests/dropin/stream_delta_encode_main), batch 16, depth 3, "
              f"key_interval 16; every run printed", flush=True)
        for turn in range(2):
            for entropy_coded in (0, 1):
                for delta_on in (1, 0):
                    p = subprocess.run([exe, raw, str(cfg.width), str(cfg.height), str(frames_n), str(cfg.levels), str(cfg.dct_block), "16", "3",
                                        str(cfg.seed), str(delta_on), "16", str(entropy_coded), "-"], capture_output=True, text=True, timeout=300)
                    print(f"  run {turn} (exit {p.returncode}): {(p.stdout.strip() or p.stderr.strip())}", flush=True)
                    if p.returncode != 0:
                        sys.exit(1)


def delta_encode() -> None:
    runs = {r: _delta_run_lib(r) for r in DELTA_RUNS}
    for config in (configs.C3, configs.C5):
        delta_encode_kernels(config, runs)
        torch.cuda.empty_cache()
    for config in (configs.C3, configs.C5):
        delta_encode_sizes(config)
        torch.cuda.empty_cache()
    delta_encode_stream()


def delta_auto_kernels(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, plain, never, fixed = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4))
    offs, plain_offs, never_offs, fixed_offs = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(4))
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(native.dct_pack_delta_auto_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    key16 = torch.zeros(n, dtype=torch.int32, device=dev)
    key16[0] = 1
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, ms per call (20 back-to-back calls, the routes in turn, the median of three rounds)",
          flush=True)
    for fg, bg in ((1, 640), (1, 1)):
        def auto():
            native.dct_pack_delta_auto_frames(bgr, block, types, mv, fg, bg, out=out, offsets=offs, keys=keys, counts=counts, workspace=ws)

        def fixed_flags():
            native.dct_pack_delta_frames(bgr, block, types, mv, fg, bg, key=key16, out=fixed, offsets=fixed_offs, workspace=ws)

        def both_and_choose():
            native.dct_pack_levels_frames(bgr, block, types, mv, fg, bg, out=plain, offsets=plain_offs, workspace=ws)
            native.dct_pack_delta_frames(bgr, block, types, mv, fg, bg, out=never, offsets=never_offs, workspace=ws)
            return (never_offs[1:] - never_offs[:-1]) >= (plain_offs[1:] - plain_offs[:-1])

        auto()
        fixed_flags()
        chosen = both_and_choose()
        sync()
        k = keys.bool()
        # a frame's size is its level count rounded up to 16 bytes: where the sizes differ the two choices agree
        differ = (never_offs[1:] - never_offs[:-1]) != (plain_offs[1:] - plain_offs[:-1])
        assert torch.equal(k[differ], chosen[differ]) and bool(k[0])
        want, want_offs = native.dct_pack_delta_frames(bgr, block, types, mv, fg, bg, key=keys)
        sync()
        assert torch.equal(offs, want_offs) and torch.equal(out[:int(offs[-1])], want[:int(offs[-1])]), "the bytes differ from the delta call's"
        t_auto, t_fixed, t_both = _median3([auto, fixed_flags, both_and_choose], sync)
        print(f"  ({fg}, {bg}): svc_hip_dct_pack_delta_auto_frames {t_auto:.3f}; svc_hip_dct_pack_delta_frames with a key frame every 16 "
              f"{t_fixed:.3f} ({t_auto / t_fixed:.2f}x); svc_hip_dct_pack_levels_frames + svc_hip_dct_pack_delta_frames + the choice from "
              f"the offsets {t_both:.3f} ({t_auto / t_both:.2f}x); key frames chosen {int(k.sum())} of {n}; MB per frame auto "
              f"{int(offs[-1]) / n / 1e6:.4f}, key every 16 {int(fixed_offs[-1]) / n / 1e6:.4f}, plain {int(plain_offs[-1]) / n / 1e6:.4f}",
              flush=True)


def delta_auto_sizes(cfg) -> None:
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    # delta_encode_sizes' static background (the first frame, repeated) under a moving 128 x 128 patch of the clip
    still = bgr[:1].expand(n, ph, pw, 3).clone()
    still_types = torch.zeros_like(types).view(n, ph // mbh, pw // mbw)
    for f in range(n):
        x, y = 256 + 48 * f, 192 + 16 * f
        still[f, y:y + 128, x:x + 128] = bgr[f, y:y + 128, x:x + 128]
        still_types[f, y // mbh:(y + 128) // mbh, x // mbw:(x + 128) // mbw] = 1
    # a cut: 8 frames of the static clip, then 8 of the synthetic clip turned upside down -- two unrelated pictures at frame 8
    cut = torch.cat([still[:8], bgr[8:].flip(1)]).contiguous()
    cut_types = torch.cat([still_types[:8], types.view(n, ph // mbh, pw // mbw)[8:].flip(1)]).reshape(n, -1).contiguous()
    still_types = still_types.reshape(n, -1).contiguous()
    key16 = [1] + [0] * (n - 1)

    def coded_sizes(stream, so):
        _, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
        sync()
        assert not est.any()
        return (eo[1:] - eo[:-1]).cpu()

    print(f"{cfg.name} batch of {n}; MB per frame raw / entropy-coded", flush=True)
    for clip_name, frames, ty in (("the synthetic clip (fresh noise every frame)", bgr, types),
                                  ("a static background under a moving 128 x 128 patch", still, still_types),
                                  ("8 static frames, then 8 synthetic ones upside down (a cut)", cut, cut_types)):
        for fg, bg in ((1, 640), (1, 1)):
            p, po = native.dct_pack_levels_frames(frames, block, ty, mv, fg, bg)
            d, do = native.dct_pack_delta_frames(frames, block, ty, mv, fg, bg, key=key16)
            a, ao, keys, counts = native.dct_pack_delta_auto_frames(frames, block, ty, mv, fg, bg)
            sync()
            raw = [int(o[-1]) for o in (po, do, ao)]
            cp, cd, ca = coded_sizes(p[:raw[0]], po), coded_sizes(d[:raw[1]], do), coded_sizes(a[:raw[2]], ao)
            k = keys.bool().cpu()
            assert torch.equal(torch.where(k, cp, cd)[1:], ca[1:])  # (frame 0 is a key frame in all three)
            best = torch.minimum(cp, cd)
            wrong = ca > best
            lost = int((ca - best).sum())
            print(f"  {clip_name} at ({fg}, {bg}): plain {raw[0] / n / 1e6:.4f} / {int(cp.sum()) / n / 1e6:.4f}, delta with a key frame every 16 "
                  f"{raw[1] / n / 1e6:.4f} / {int(cd.sum()) / n / 1e6:.4f}, delta with the chosen key frames {raw[2] / n / 1e6:.4f} / "
                  f"{int(ca.sum()) / n / 1e6:.4f} ({int(k.sum())} key frames: {''.join('K' if v else '.' for v in k.tolist())}); the level-count "
                  f"choice is not the smaller coded frame at {int(wrong.sum())} of {n} frames, {lost} B in all "
                  f"({100.0 * lost / max(int(best.sum()), 1):.3f} % of the best coded stream)", flush=True)


def delta_temporal_kernels(cfg, both_steps=True) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, plain, ref = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
    offs, plain_offs, ref_offs = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3))
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(native.dct_pack_delta_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(native.delta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    key = torch.zeros(n, dtype=torch.int32, device=dev)
    key[0] = 1
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, frame 0 the key frame; ms per call (20 back-to-back calls, the routes in turn, the "
          f"median of three rounds)", flush=True)
    for fg, bg in ((1, 640), (1, 1)) if both_steps else ((1, 640),):
        def pack():
            native.dct_pack_levels_frames(bgr, block, types, mv, fg, bg, out=plain, offsets=plain_offs, workspace=ws)

        def delta_at(period):
            def call():
                if period == 1:
                    native.delta_levels_frames(plain, plain_offs, pw, ph, block, mv, key=key, out=ref, out_offsets=ref_offs, workspace=ws_d,
                                               status=st)
                else:
                    native.delta_levels_temporal_frames(plain, plain_offs, pw, ph, block, mv, period, key=key, out=ref, out_offsets=ref_offs,
                                                        workspace=ws_d, status=st)
            return call

        def fused():
            native.dct_pack_delta_frames(bgr, block, types, mv, fg, bg, key=key, out=out, offsets=offs, workspace=ws)

        def two_calls():
            pack()
            delta_at(4)()

        pack()
        sizes = {}
        for period in (1, 2, 4):
            delta_at(period)()
            sync()
            assert not st.any()
            sizes[period] = int(ref_offs[-1]) / n / 1e6
        t = _median3([delta_at(1), delta_at(2), delta_at(4), fused, two_calls, pack], sync)
        print(f"  ({fg}, {bg}): svc_hip_delta_levels_frames {t[0]:.3f}; svc_hip_delta_levels_temporal_frames at period 2 {t[1]:.3f} "
              f"({t[1] / t[0]:.2f}x), at period 4 {t[2]:.3f} ({t[2] / t[0]:.2f}x); svc_hip_dct_pack_delta_frames (period 1, fused) {t[3]:.3f}; "
              f"svc_hip_dct_pack_levels_frames + the temporal call at period 4 {t[4]:.3f} ({t[4] / t[3]:.2f}x of the fused call; the pack alone "
              f"{t[5]:.3f}); MB per frame at periods 1, 2, 4: " + ", ".join(f"{sizes[p]:.4f}" for p in (1, 2, 4)), flush=True)


def delta_temporal_sizes(cfg) -> None:
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    mbw, mbh = native._bwbh(mv)
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    # delta_auto_sizes' clips: the static background under a moving 128 x 128 patch, and 8 frames of it followed by 8 synthetic ones
    # upside down
    still = bgr[:1].expand(n, ph, pw, 3).clone()
    still_types = torch.zeros_like(types).view(n, ph // mbh, pw // mbw)
    for f in range(n):
        x, y = 256 + 48 * f, 192 + 16 * f
        still[f, y:y + 128, x:x + 128] = bgr[f, y:y + 128, x:x + 128]
        still_types[f, y // mbh:(y + 128) // mbh, x // mbw:(x + 128) // mbw] = 1
    cut = torch.cat([still[:8], bgr[8:].flip(1)]).contiguous()
    cut_types = torch.cat([still_types[:8], types.view(n, ph // mbh, pw // mbw)[8:].flip(1)]).reshape(n, -1).contiguous()
    still_types = still_types.reshape(n, -1).contiguous()
    key16 = [1] + [0] * (n - 1)

    def coded_sizes(stream, so):
        _, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
        sync()
        assert not est.any()
        return (eo[1:] - eo[:-1]).cpu()

    print(f"{cfg.name} batch of {n}, frame 0 the key frame; MB per frame raw / entropy-coded", flush=True)
    for clip_name, frames, ty in (("the synthetic clip (fresh noise every frame)", bgr, types),
                                  ("a static background under a moving 128 x 128 patch", still, still_types),
                                  ("8 static frames, then 8 synthetic ones upside down (a cut)", cut, cut_types)):
        for fg, bg in ((1, 640), (1, 1)):
            p, po = native.dct_pack_levels_frames(frames, block, ty, mv, fg, bg)
            sync()
            p = p[:int(po[-1])].clone()
            row, per_frame = [], {}
            for period in (1, 2, 4):
                if period == 1:
                    d, do, st = native.delta_levels_frames(p, po, pw, ph, block, mv, key=key16)
                else:
                    d, do, st = native.delta_levels_temporal_frames(p, po, pw, ph, block, mv, period, key=key16)
                sync()
                assert not st.any()
                raw = (do[1:] - do[:-1]).cpu()
                coded = coded_sizes(d[:int(do[-1])].clone(), do)
                per_frame[period] = (raw, coded)
                row.append(f"period {period} {int(raw.sum()) / n / 1e6:.4f} / {int(coded.sum()) / n / 1e6:.4f}")
            r1, c1 = (int(v.sum()) for v in per_frame[1])
            grow = ", ".join(f"period {q}: {int(per_frame[q][0].sum()) / r1:.3f}x / {int(per_frame[q][1].sum()) / c1:.3f}x" for q in (2, 4))
            raw4, coded4 = per_frame[4]
            sent = ", ".join(f"{name} {int(raw4[::e].sum()) / int(raw4.sum()):.3f} / {int(coded4[::e].sum()) / int(coded4.sum()):.3f} of the "
                             f"stream's bytes for {len(raw4[::e])} of {n} frames" for name, e in (("half rate", 2), ("quarter rate", 4)))
            print(f"  {clip_name} at ({fg}, {bg}): " + "; ".join(row) + f" (against period 1, {grow}); from the period-4 stream {sent}", flush=True)


def delta_temporal_stream(frames_n=33) -> None:
    import subprocess
    import tempfile
    cfg = configs.C3
    exe = os.path.join(ROOT, "tests", "dropin", "stream_temporal_main")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=torch.device("cuda"))
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(frames_n):
                f.write(clip.frame_bgr(t).cpu().numpy().tobytes())
        del clip
        torch.cuda.empty_cache()
        print(f"{cfg.name}, {frames_n} frames from host memory through svc::StreamEncoder and svc::StreamDecoder (tests/dropin/stream_temporal_main), "
              f"batch 16, depth 3, key_interval 16; every run printed", flush=True)
        for turn in range(2):
            for period in (4, 1):
                p = subprocess.run([exe, raw, str(cfg.width), str(cfg.height), str(frames_n), str(cfg.levels), str(cfg.dct_block), "16", "3",
                                    str(cfg.seed), str(period), "16", "0", "-"], capture_output=True, text=True, timeout=300)
                print(f"  run {turn}, temporal_period {period} (exit {p.returncode}): {(p.stdout.strip() or p.stderr.strip())}", flush=True)
                if p.returncode != 0:
                    sys.exit(1)


def delta_temporal() -> None:
    delta_temporal_kernels(configs.C3)
    torch.cuda.empty_cache()
    delta_temporal_kernels(configs.C5, both_steps=False)
    torch.cuda.empty_cache()
    delta_temporal_sizes(configs.C3)
    torch.cuda.empty_cache()
    delta_temporal_stream()


def _temporal_variant_lib(redo):
    """csrc/dct_pack.hip built with the other form of period 4 (SVC_DCT_PACK_TEMPORAL_REDO), as _delta_run_lib builds its runs."""
    import ctypes
    import subprocess
    from scalable_video_codec_amd import build
    out = os.path.join(ROOT, "tools", "_bin", f"libsvc_dct_pack_temporal_redo{redo}.so")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([build._hipcc(), *build.HIPCC_FLAGS, f"-DSVC_DCT_PACK_TEMPORAL_REDO={redo}", "-shared", "-o", out,
                               os.path.join(build.CSRC, "dct_pack.hip"), f"-L{build.PKG}", "-lsvc_hip", f"-Wl,-rpath,{build.PKG}"])
    fn = ctypes.CDLL(out).svc_hip_dct_pack_delta_temporal_frames
    fn.restype, fn.argtypes = native.SIGNATURES_TEMPORAL["svc_hip_dct_pack_delta_temporal_frames"]
    return fn


def delta_temporal_encode_kernels(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out, plain, ref = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3))
    offs, plain_offs, ref_offs = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3))
    st = torch.empty(n, dtype=torch.int32, device=dev)
    keys, counts = torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(native.dct_pack_delta_temporal_auto_workspace_bytes(n, pw, ph, block, mv, 4), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(native.delta_levels_temporal_workspace_bytes(n, pw, ph, block, mv, 4), dtype=torch.uint8, device=dev)
    key = torch.zeros(n, dtype=torch.int32, device=dev)
    key[0] = 1
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, frame 0 the key frame; ms per call (20 back-to-back calls, the routes in turn, the "
          f"median of three rounds)", flush=True)
    for fg, bg in ((1, 640), (1, 1)):
        def pack():
            native.dct_pack_levels_frames(bgr, block, types, mv, fg, bg, out=plain, offsets=plain_offs, workspace=ws)

        def two_calls(period):
            def call():
                pack()
                native.delta_levels_temporal_frames(plain, plain_offs, pw, ph, block, mv, period, key=key, out=ref, out_offsets=ref_offs,
                                                    workspace=ws_d, status=st)
            return call

        def fused(period):
            def call():
                native.dct_pack_delta_temporal_frames(bgr, block, types, mv, fg, bg, period, key=key, out=out, offsets=offs, workspace=ws)
            return call

        def auto(period):
            def call():
                native.dct_pack_delta_temporal_auto_frames(bgr, block, types, mv, fg, bg, period, forced=key, out=out, offsets=offs, keys=keys,
                                                           counts=counts, workspace=ws)
            return call

        def period1():
            native.dct_pack_delta_frames(bgr, block, types, mv, fg, bg, key=key, out=out, offsets=offs, workspace=ws)

        def variant(redo):  # period 4 in the form built with SVC_DCT_PACK_TEMPORAL_REDO = redo
            fn = _temporal_variant_lib(redo)
            mbw, mbh = native._bwbh(mv)

            def call():
                native._check(fn(bgr.data_ptr(), ph * pw * 3, n, pw, ph, block, types.data_ptr(), mbw, mbh, fg, bg, None, None, key.data_ptr(),
                                 ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), native._stream(), 4))
            return call

        two_calls(4)()
        for redo in (0, 1):
            variant(redo)()
            sync()
            assert torch.equal(offs, ref_offs) and torch.equal(out[:int(offs[-1])], ref[:int(offs[-1])])
        tv = _median3([variant(0), variant(1)], sync)
        print(f"  ({fg}, {bg}): period 4, both sets kept (9 transforms for 8 frames) {tv[0]:.3f}; one set kept, frame 4k transformed again in "
              f"front of frame 4k + 4 (10) {tv[1]:.3f}", flush=True)
        for period in (2, 4):  # the bytes first: the fused call against the two it replaces
            two_calls(period)()
            fused(period)()
            sync()
            assert not st.any() and torch.equal(offs, ref_offs) and torch.equal(out[:int(offs[-1])], ref[:int(offs[-1])])
        t = _median3([fused(2), fused(4), two_calls(2), two_calls(4), period1, pack, auto(2), auto(4)], sync)
        worst = max(t[0] / t[2], t[1] / t[3])
        print(f"  ({fg}, {bg}): svc_hip_dct_pack_delta_temporal_frames at period 2 {t[0]:.3f}, at period 4 {t[1]:.3f}; "
              f"svc_hip_dct_pack_levels_frames + svc_hip_delta_levels_temporal_frames {t[2]:.3f} ({t[2] / t[0]:.2f}x), {t[3]:.3f} "
              f"({t[3] / t[1]:.2f}x); svc_hip_dct_pack_delta_frames (period 1) {t[4]:.3f} (the fused call {t[0] / t[4]:.2f}x, {t[1] / t[4]:.2f}x "
              f"of it); svc_hip_dct_pack_levels_frames alone {t[5]:.3f}; svc_hip_dct_pack_delta_temporal_auto_frames {t[6]:.3f} "
              f"({t[6] / t[0]:.2f}x of the fixed-flag call), {t[7]:.3f} ({t[7] / t[1]:.2f}x); bytes == the two calls'; the fused call is "
              f"{'faster' if worst < 1 else 'NOT faster'} than the two calls at both periods", flush=True)


def delta_temporal_encode() -> None:
    delta_temporal_encode_kernels(configs.C3)
    torch.cuda.empty_cache()
    delta_temporal_encode_kernels(configs.C5)
    torch.cuda.empty_cache()
    delta_temporal_stream()


def delta_auto_stream(frames_n=33) -> None:
    import subprocess
    import tempfile
    cfg = configs.C3
    exe = os.path.join(ROOT, "tests", "dropin", "stream_delta_auto_main")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=torch.device("cuda"))
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(frames_n):
                f.write(clip.frame_bgr(t).cpu().numpy().tobytes())
        del clip
        torch.cuda.empty_cache()
        print(f"{cfg.name}, {frames_n} frames from host memory through svc::StreamEncoder (tests/dropin/stream_delta_auto_main), batch 16, depth 3, "
              f"key_interval 16; every run printed", flush=True)
        for turn in range(2):
            for entropy_coded in (0, 1):
                for auto_on in (1, 0):
                    p = subprocess.run([exe, raw, str(cfg.width), str(cfg.height), str(frames_n), str(cfg.levels), str(cfg.dct_block), "16", "3",
                                        str(cfg.seed), str(auto_on), "16", str(entropy_coded), "-"], capture_output=True, text=True, timeout=300)
                    print(f"  run {turn} (exit {p.returncode}): {(p.stdout.strip() or p.stderr.strip())}", flush=True)
                    if p.returncode != 0:
                        sys.exit(1)


def delta_auto() -> None:
    for config in (configs.C3, configs.C5):
        delta_auto_kernels(config)
        torch.cuda.empty_cache()
    for config in (configs.C3, configs.C5):
        delta_auto_sizes(config)
        torch.cuda.empty_cache()
    delta_auto_stream()


def window_entropy(cfg) -> None:
    import numpy as np
    from scalable_video_codec_amd import entropy
    dev = torch.device("cuda")
    n, viewers = 16, 4
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    lbase, whole = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    ws2 = torch.empty(native.dct_pack_layers_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    sync = torch.cuda.synchronize

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    def rects(viewer):  # the windows of `window`
        out = []
        for f in range(n):
            x = (pw - 256) // 2 + 32 * ((f + 3 * viewer) % 7 - 3) + 64 * (viewer - 1)
            y = (ph - 256) // 2 + 16 * ((f + viewer) % 5 - 2)
            out.append((x // 16 * 16, y // 16 * 16, 256, 256))
        return out

    # what the server holds: the every-tile enhancement, entropy-coded
    _, _, _, offs_q = native.dct_pack_layers_frames(bgr, block, types, mv, 1, 640, 1, window=None, base_out=lbase, enh_out=whole, workspace=ws2)
    sync()
    uq = int(offs_q[-1])
    stored, offs_s, st = native.entropy_encode_frames(whole[:uq], offs_q.clone(), pw, ph, block, mv)
    sync()
    assert not st.any()
    us = int(offs_s[-1])
    stored, offs_s = stored[:us].clone(), offs_s.clone()
    del lbase, whole, ws2, bgr
    torch.cuda.empty_cache()
    wse = torch.empty(native.entropy_workspace_bytes(viewers * n, pw, ph, block, mv), dtype=torch.uint8, device=dev)

    for name, n_out, src, win_rects in (("(a) one viewer", n, None, rects(0)),
                                        (f"(b) {viewers} viewers, n_out = {viewers * n} through d_src", viewers * n,
                                         [f for _ in range(viewers) for f in range(n)], [r for v in range(viewers) for r in rects(v)])):
        win = torch.tensor(win_rects, dtype=torch.int32, device=dev)
        srct = None if src is None else torch.tensor(src, dtype=torch.int32, device=dev)
        out = torch.empty(native.window_entropy_max_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
        ws = torch.empty(native.window_entropy_workspace_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
        oo, stw = torch.empty(n_out + 1, dtype=torch.int64, device=dev), torch.empty(n_out, dtype=torch.int32, device=dev)
        # the three-call route's buffers
        q = torch.empty(cap, dtype=torch.uint8, device=dev)
        qo = torch.empty(n + 1, dtype=torch.int64, device=dev)
        wq = torch.empty(native.levels_max_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
        wo, wst = torch.empty(n_out + 1, dtype=torch.int64, device=dev), torch.empty(n_out, dtype=torch.int32, device=dev)
        wsw = torch.empty(native.window_levels_workspace_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
        e = torch.empty(native.entropy_max_bytes(n_out, pw, ph, block, mv), dtype=torch.uint8, device=dev)
        eo, est = torch.empty(n_out + 1, dtype=torch.int64, device=dev), torch.empty(n_out, dtype=torch.int32, device=dev)

        def serve():
            return native.window_entropy_frames(stored, offs_s, pw, ph, block, mv, window=win, src=srct, out=out, out_offsets=oo,
                                                workspace=ws, status=stw)

        def three():
            native.entropy_decode_frames(stored, offs_s, pw, ph, block, mv, out=q, out_offsets=qo, workspace=wse)
            native.window_levels_frames(q, qo, pw, ph, block, mv, window=win, src=srct, out=wq, out_offsets=wo, workspace=wsw, status=wst)
            # (the encoder reads the stream's bytes through its offsets: the whole worst-case buffer is handed over, as a server would)
            native.entropy_encode_frames(wq, wo, pw, ph, block, mv, out=e, out_offsets=eo, workspace=wse, status=est)

        if src is None:
            print(f"{cfg.name} batch of {n}, stored SVCE enhancement at (1, 640, 1), a 256 x 256 window per frame, ms per call (best .. worst of 3 "
                  f"runs of 20 back-to-back calls; the routes interleaved: three, one, three, one)", flush=True)
        t3a = _per_step(three, sync, steps=20)
        t1a = _per_step(serve, sync, steps=20)
        t3b = _per_step(three, sync, steps=20)
        t1b = _per_step(serve, sync, steps=20)
        serve()
        three()
        sync()
        used = int(oo[-1])
        assert not stw.any() and not est.any() and not wst.any()
        assert torch.equal(oo, eo) and torch.equal(out[:used], e[:used]), "the windowed SVCE stream differs from the three-call route's"
        # the share of chunks in each class, from the statement's classification of the first frames (a frame each of the first viewer's)
        host, ho = stored.cpu().numpy(), offs_s.cpu().tolist()
        cls = np.zeros(3, np.int64)
        for i in range(2):
            f = i if src is None else src[i]
            cls += np.bincount(entropy.chunk_classes(host[ho[f]:ho[f + 1]], win_rects[i]), minlength=3)
        t3, t1 = (min(t3a[0], t3b[0]), max(t3a[1], t3b[1])), (min(t1a[0], t1b[0]), max(t1a[1], t1b[1]))
        uq_out = int(wo[-1])
        print(f"{name}: three calls {fmt(t3a)}, again {fmt(t3b)}; one call {fmt(t1a)}, again {fmt(t1b)} "
              f"({t3[0] / t1[0]:.2f}x by the best of each, {t3[1] / t1[1]:.2f}x by the worst); same bytes and offsets", flush=True)
        print(f"    one call: reads {us / n / 1e6:.3f} MB per stored frame (only kept and cut payloads, the header, types and index of it), writes "
              f"{used / n_out / 1e6:.3f} MB per served frame; workspace {ws.numel() / n_out / 1e6:.3f} MB per served frame", flush=True)
        print(f"    three calls: SVCE in {us / n / 1e6:.3f} MB, SVCQ out {uq / n / 1e6:.3f} MB per stored frame; windowed SVCQ "
              f"{uq_out / n_out / 1e6:.3f} MB per served frame written and read again; SVCE out {used / n_out / 1e6:.3f} MB", flush=True)
        print(f"    chunks per frame (two frames): kept {cls[0] / cls.sum() * 100:.1f} %, dropped {cls[1] / cls.sum() * 100:.1f} %, cut "
              f"{cls[2] / cls.sum() * 100:.1f} % ({cls[2] // 2} cut chunks walked per frame of {cls.sum() // 2})", flush=True)
        del out, ws, q, wq, wsw, e
        torch.cuda.empty_cache()


HBM_PEAK = 8.0e12  # bytes per second, the MI355X's HBM3E


def split(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    fg, bg, e = 1, 640, 1
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    fine, whole, ebase, eenh, sbase, senh, wout = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(7))
    sync = torch.cuda.synchronize
    ws1 = torch.empty(native.dct_pack_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(native.dct_pack_layers_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    win = torch.tensor([((pw - 256) // 2 // 16 * 16 + 32 * (f % 7 - 3), (ph - 256) // 2 // 16 * 16 + 16 * (f % 5 - 2), 256, 256) for f in range(n)],
                       dtype=torch.int32, device=dev)

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    def hbm(nbytes, t):
        return f"{nbytes / 1e6:.2f} MB moved, {nbytes / (t[0] * 1e-3) / HBM_PEAK * 100:.1f} % of the HBM peak"

    # what is stored: the stream at (e, e), and the every-tile enhancement over the base at (fg, bg)
    _, offs_f = native.dct_pack_levels_frames(bgr, block, types, mv, e, e, out=fine, workspace=ws1)
    _, _, _, offs_w = native.dct_pack_layers_frames(bgr, block, types, mv, fg, bg, e, base_out=ebase, enh_out=whole, workspace=ws2)
    sync()
    offs_f, offs_w = offs_f.clone(), offs_w.clone()
    uf, uw = int(offs_f[-1]), int(offs_w[-1])
    stored, stored_enh = fine[:uf], whole[:uw]

    def encode():
        return native.dct_pack_layers_frames(bgr, block, types, mv, fg, bg, e, window=win, base_out=ebase, enh_out=eenh, workspace=ws2)

    wsw = torch.empty(native.window_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    wst, woo = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)

    def serve():
        return native.window_levels_frames(stored_enh, offs_w, pw, ph, block, mv, window=win, out=wout, out_offsets=woo, workspace=wsw, status=wst)

    wss = torch.empty(native.split_levels_workspace_bytes(n, n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    sbo, seo = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    sst = torch.empty(n, dtype=torch.int32, device=dev)

    def fixed():
        return native.split_levels_frames(stored, offs_f, pw, ph, block, mv, e, fg, bg, window=win, base_out=sbase, base_offsets=sbo,
                                          enh_out=senh, enh_offsets=seo, workspace=wss, status=sst)

    lad, per_frame = _budget(cfg)
    budget_t = native.budget_tensor(per_frame, n, dev)
    wsb = torch.empty(native.split_levels_budget_workspace_bytes(n, n, pw, ph, block, mv, len(lad)), dtype=torch.uint8, device=dev)
    choice = torch.empty(n, dtype=torch.int32, device=dev)

    def budgeted():
        return native.split_levels_budget_frames(stored, offs_f, pw, ph, block, mv, e, lad, budget_t, window=win, base_out=sbase,
                                                 base_offsets=sbo, enh_out=senh, enh_offsets=seo, workspace=wsb, status=sst, choice=choice)

    print(f"{cfg.name} batch of {n} at ({fg}, {bg}, {e}), a 256 x 256 window per frame, ms per call (best .. worst of 3 runs of 20 back-to-back "
          f"calls); stored fine stream {uf / n / 1e6:.3f} MB per frame", flush=True)
    t_enc = _per_step(encode, sync, steps=20)
    t_fix = _per_step(fixed, sync, steps=20)
    t_bud = _per_step(budgeted, sync, steps=20)
    t_win = _per_step(serve, sync, steps=20)
    t_enc2 = _per_step(encode, sync, steps=20)  # the encode again, after: the spread of the same call in this run
    _, offs_eb, _, offs_ee = encode()
    fixed()
    sync()
    assert not sst.any()
    ub, ue, sb, se = int(offs_eb[-1]), int(offs_ee[-1]), int(sbo[-1]), int(seo[-1])
    pixels = bgr.numel()
    masks = n * 8 * 3 * (pw // block) * (ph // block) * (block * block // 64)  # the mask section of the n frames
    print(f"(a) encode both layers from the pixels {fmt(t_enc)} (again {fmt(t_enc2)}): {hbm(pixels + ub + ue, t_enc)}", flush=True)
    print(f"(b) split the stored fine stream {fmt(t_fix)} ({t_fix[0] / min(t_enc[0], t_enc2[0]):.3f} of the encode): "
          f"{hbm(2 * uf + masks + sb + se, t_fix)} (the input pass reads the masks, the count and the write pass the frames), workspace "
          f"{wss.numel() / n / 1e6:.3f} MB per frame", flush=True)
    # the ratio 640 is even: the bases differ in the levels the split rounds from a tie; by how much
    same_size = torch.equal(sbo, offs_eb)
    print(f"    base from the split {sb / n / 1e6:.4f} MB per frame, from the encoder {ub / n / 1e6:.4f} MB ({(sb - ub) / ub * 100:+.3f} %); "
          f"offsets {'equal' if same_size else 'differ'}; enhancement {se / n / 1e6:.4f} MB per "
          f"frame against {ue / n / 1e6:.4f} MB", flush=True)
    budgeted()
    sync()
    assert not sst.any()
    ch = choice.cpu().numpy().view("uint32")
    bb, be = int(sbo[-1]), int(seo[-1])
    print(f"(c) split under a budget of {per_frame} B per frame, {len(lad)} entries {fmt(t_bud)} ({t_bud[0] / t_fix[0]:.2f}x the fixed split): "
          f"{hbm(3 * uf + masks + bb + be, t_bud)}; choices {[int(c) & 0x7FFFFFFF for c in ch]}, over budget {int((ch >> 31).sum())}, base "
          f"{bb / n / 1e6:.3f} MB per frame, workspace {wsb.numel() / n / 1e6:.3f} MB per frame", flush=True)
    serve()
    sync()
    print(f"(d) window the stored enhancement {fmt(t_win)}: {hbm(masks + 2 * int(woo[-1]), t_win)} (the masks, the kept levels in and out); stored {uw / n / 1e6:.3f} MB per frame, served "
          f"{int(woo[-1]) / n / 1e6:.3f} MB per frame", flush=True)


def band(cfg, frames_n=64) -> None:
    import subprocess
    import tempfile

    import numpy as np
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    masks = 8 * 3 * (pw // block) * (ph // block) * (block * block // 64)  # the mask section of a frame
    ks = [block // r for r in (2, 4, 8)]

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    def coded_bytes(stream, offs):
        _, eo, st = native.entropy_encode_frames(stream, offs, pw, ph, block, mv)
        sync()
        assert not st.any()
        return int(eo[-1])

    def band_of(stream, offs, rows, src=None):
        out, oo, st = native.band_levels_frames(stream, offs, pw, ph, block, mv, band=rows, src=src)
        sync()
        assert not st.any()
        return out[:int(oo[-1])].clone(), oo.clone()

    stored = {}
    for steps in ((1, 640), (1, 1)):
        out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, *steps)
        sync()
        stored[steps] = (out[:int(offs[-1])].clone(), offs.clone())
    # (a) bytes per frame
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}; the mask section is {masks / 1e6:.3f} MB of every frame, whatever the band", flush=True)
    for steps, (stream, offs) in stored.items():
        print(f"(a) stored at {steps}: {stream.numel() / n / 1e6:.4f} MB per frame, entropy-coded {coded_bytes(stream, offs) / n / 1e6:.4f} MB", flush=True)
        for k in ks:
            for name, row in ((f"band (0, 0, {k}, {k})", (0, 0, k, k)), (f"remainder ({k}, {k}, {block}, {block})", (k, k, block, block))):
                b, bo = band_of(stream, offs, [row] * n)
                print(f"      {name}: {b.numel() / n / 1e6:.4f} MB per frame, entropy-coded {coded_bytes(b, bo) / n / 1e6:.4f} MB", flush=True)
    # (b), (c) the calls' time on the stream stored at (1, 1), which the split takes too; then the band call on the stream at (1, 640)
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(3)]
    oo = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3)]
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ws_w = torch.empty(native.window_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_s = torch.empty(native.split_levels_workspace_bytes(n, n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(native.band_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_u = torch.empty(native.union_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    for steps in ((1, 1), (1, 640)):
        stream, offs = stored[steps]
        print(f"(b) the stream stored at {steps} ({stream.numel() / n / 1e6:.3f} MB per frame), ms per call of {n} frames (best .. worst of 3 "
              f"runs of 20 back-to-back calls)", flush=True)

        def f_window():
            return native.window_levels_frames(stream, offs, pw, ph, block, mv, out=outs[0], out_offsets=oo[0], workspace=ws_w, status=st)

        def f_split():
            return native.split_levels_frames(stream, offs, pw, ph, block, mv, 1, 1, 640, base_out=outs[1], base_offsets=oo[1], enh_out=outs[2],
                                              enh_offsets=oo[2], workspace=ws_s, status=st)
        t_win = _per_step(f_window, sync, steps=20)
        print(f"    svc_hip_window_levels_frames, no window {fmt(t_win)}", flush=True)
        if steps == (1, 1):
            t_split = _per_step(f_split, sync, steps=20)
            assert not st.any()
            print(f"    svc_hip_split_levels_frames to (1, 640), every tile enhanced {fmt(t_split)}", flush=True)
        for k in ks + [block]:
            rows = torch.tensor([(0, 0, k, k)] * n, dtype=torch.int32, device=dev)

            def call():
                return native.band_levels_frames(stream, offs, pw, ph, block, mv, band=rows, out=outs[0], out_offsets=oo[0], workspace=ws_b, status=st)
            t = _per_step(call, sync, steps=20)
            assert not st.any()
            print(f"    svc_hip_band_levels_frames (0, 0, {k}, {k}) {fmt(t)} ({t[0] / t_win[0]:.2f}x the window call"
                  + (f", {t[0] / t_split[0]:.2f}x the split" if steps == (1, 1) else "") + f"), {int(oo[0][-1]) / n / 1e6:.3f} MB per frame out", flush=True)
        t_win2 = _per_step(f_window, sync, steps=20)  # the window call again, after: the spread of the same call in this run
        print(f"    svc_hip_window_levels_frames again {fmt(t_win2)}", flush=True)
        k = ks[0]
        low, lo = band_of(stream, offs, [(0, 0, k, k)] * n)
        high, ho = band_of(stream, offs, [(k, k, block, block)] * n)

        def f_union():
            return native.union_levels_frames(low, lo, high, ho, pw, ph, block, mv, out=outs[0], out_offsets=oo[0], workspace=ws_u, status=st)
        t_u = _per_step(f_union, sync, steps=20)
        assert not st.any() and torch.equal(oo[0], offs) and torch.equal(outs[0][:stream.numel()], stream), "the union is not the stored stream"
        print(f"(c) svc_hip_union_levels_frames of (0, 0, {k}, {k}) and its remainder {fmt(t_u)} ({t_u[0] / t_win[0]:.2f}x the window call"
              + (f", {t_u[0] / t_split[0]:.2f}x the split" if steps == (1, 1) else "") + "); the bytes are the stored stream's", flush=True)
    # (d) one call for 4 viewers at four K against four calls
    stream, offs = stored[(1, 640)]
    four = ks[::-1] + [block]
    src = torch.arange(n, dtype=torch.int32, device=dev).repeat(4)
    rows64 = torch.tensor([(0, 0, k, k) for k in four for _ in range(n)], dtype=torch.int32, device=dev)
    rows16 = [torch.tensor([(0, 0, k, k)] * n, dtype=torch.int32, device=dev) for k in four]
    out64 = torch.empty(4 * cap, dtype=torch.uint8, device=dev)
    oo64, st64 = torch.empty(4 * n + 1, dtype=torch.int64, device=dev), torch.empty(4 * n, dtype=torch.int32, device=dev)
    ws64 = torch.empty(native.band_levels_workspace_bytes(4 * n, pw, ph, block, mv), dtype=torch.uint8, device=dev)

    def one_call():
        return native.band_levels_frames(stream, offs, pw, ph, block, mv, band=rows64, src=src, out=out64, out_offsets=oo64, workspace=ws64, status=st64)

    def four_calls():
        for rows in rows16:
            native.band_levels_frames(stream, offs, pw, ph, block, mv, band=rows, out=outs[0], out_offsets=oo[0], workspace=ws_b, status=st)
    t1, t4 = _per_step(one_call, sync, steps=20), _per_step(four_calls, sync, steps=20)
    t1b = _per_step(one_call, sync, steps=20)
    assert not st64.any()
    print(f"(d) 4 viewers at K = {four} from the stream at (1, 640): one call with n_out = {4 * n} {fmt(t1)} (again {fmt(t1b)}), four calls {fmt(t4)}",
          flush=True)
    # (e) through svc::StreamDecoder on SVCE input: the band stream against the full stream, PCIe included
    here = os.path.join(ROOT, "tests", "dropin")
    bgr, types = _batch(cfg, frames_n)
    out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, 1, 640)
    sync()
    full = (out[:int(offs[-1])].clone(), offs.clone())
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        def store(name, stream, so):
            coded, eo, est = native.entropy_encode_frames(stream, so, pw, ph, block, mv)
            sync()
            assert not est.any()
            coded[:int(eo[-1])].cpu().numpy().tofile(os.path.join(d, name + ".big"))
            eo.cpu().numpy().astype(np.uint64).tofile(os.path.join(d, name + ".offsets"))
            return int(eo[-1])
        print(f"(e) {frames_n} frames at (1, 640) as SVCE through tests/dropin/stream_reduced_main, batch 16, display (W / r, H / r), no gaze; full "
              f"stream {store('full', *full) / frames_n / 1e6:.4f} MB per frame coded", flush=True)
        for r in (2, 4, 8):
            k = block // r
            coded = store(f"band{r}", *band_of(*full, [(0, 0, k, k)] * frames_n))
            print(f"    reduce {r}: band (0, 0, {k}, {k}) {coded / frames_n / 1e6:.4f} MB per frame coded", flush=True)
            for turn in range(3):  # alternating, every run printed: the spread is part of the result
                for name in ("full", f"band{r}"):
                    p = subprocess.run([os.path.join(here, "stream_reduced_main"), os.path.join(d, name), str(frames_n), str(r), "0", "0", "-", "16",
                                        "-"], capture_output=True, text=True, timeout=300)
                    lines = p.stdout.strip().splitlines() or [p.stderr.strip()]
                    print(f"      {name}, run {turn} (exit {p.returncode}): {lines[0]}", flush=True)
                    if turn == 0 and len(lines) > 1:  # where the time went, once per stream
                        print(f"        {lines[1]}", flush=True)
                    if p.returncode != 0:
                        sys.exit(1)


def delta(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    sync = torch.cuda.synchronize
    bgr, types = _batch(cfg, n)
    cap = native.levels_max_bytes(n, pw, ph, block, mv)

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    def coded_bytes(stream, offs):
        _, eo, st = native.entropy_encode_frames(stream, offs, pw, ph, block, mv)
        sync()
        assert not st.any()
        return int(eo[-1])

    def used(out, offs):
        sync()
        return out[:int(offs[-1])].clone(), offs.clone()

    stored = {}
    for steps in ((1, 640), (1, 1)):
        stored[f"{steps}"] = used(*native.dct_pack_levels_frames(bgr, block, types, mv, *steps))
    _, _, enh, enh_offs = native.dct_pack_layers_frames(bgr, block, types, mv, 1, 640, 1)
    stored["(1, 640, 1) enhancement, every tile"] = used(enh, enh_offs)
    # (a) bytes: a key frame every 16, so frame 0 of the batch is the key frame and 15 frames are differences
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, frame 0 a key frame; MB per frame, raw / entropy-coded", flush=True)
    diffs = {}
    for name, (stream, offs) in stored.items():
        out, oo, st = native.delta_levels_frames(stream, offs, pw, ph, block, mv)
        assert not st.any()
        diffs[name] = d, do = used(out, oo)
        back, bo, st = native.undelta_levels_frames(d, do, pw, ph, block, mv)
        sync()
        assert not st.any() and torch.equal(bo, offs) and torch.equal(back[:stream.numel()], stream), "undelta(delta) is not the stored stream"
        raw, craw = stream.numel(), coded_bytes(stream, offs)
        draw, dcoded = d.numel(), coded_bytes(d, do)
        key = int(offs[1])
        print(f"(a) {name}: intra {raw / n / 1e6:.4f} / {craw / n / 1e6:.4f}, delta {draw / n / 1e6:.4f} / {dcoded / n / 1e6:.4f} "
              f"({draw / raw:.3f}x / {dcoded / craw:.3f}x); the 15 difference frames alone {(draw - key) / 15 / 1e6:.4f} raw against "
              f"{(raw - key) / 15 / 1e6:.4f}; undelta(delta) is the stored stream", flush=True)
    # (b) the calls' time beside the two-input merge on streams of the same bytes and the plain copy
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    oo = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ws_w = torch.empty(native.window_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_u = torch.empty(native.union_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(native.delta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_x = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev)
    k = block // 2
    for name in ("(1, 1)", "(1, 640)"):
        stream, offs = stored[name]
        d, do = diffs[name]
        low, lo = used(*native.band_levels_frames(stream, offs, pw, ph, block, mv, band=[(0, 0, k, k)] * n)[:2])
        high, ho = used(*native.band_levels_frames(stream, offs, pw, ph, block, mv, band=[(k, k, block, block)] * n)[:2])
        print(f"(b) the stream stored at {name} ({stream.numel() / n / 1e6:.3f} MB per frame, its delta stream {d.numel() / n / 1e6:.3f}), ms per "
              f"call of {n} frames (best .. worst of 3 runs of 20 back-to-back calls)", flush=True)

        def f_window():
            return native.window_levels_frames(stream, offs, pw, ph, block, mv, out=outs[0], out_offsets=oo[0], workspace=ws_w, status=st)

        def f_union():
            return native.union_levels_frames(low, lo, high, ho, pw, ph, block, mv, out=outs[0], out_offsets=oo[0], workspace=ws_u, status=st)

        def f_delta():
            return native.delta_levels_frames(stream, offs, pw, ph, block, mv, out=outs[0], out_offsets=oo[0], workspace=ws_d, status=st)

        def f_undelta():
            return native.undelta_levels_frames(d, do, pw, ph, block, mv, out=outs[1], out_offsets=oo[1], workspace=ws_d, status=st)

        def f_decode():
            return native.decode_levels_frames(stream, offs, pw, ph, block, mv, 1, 640, rec=rec, workspace=ws_x)

        def f_undelta_decode():
            f_undelta()
            return native.decode_levels_frames(outs[1], oo[1], pw, ph, block, mv, 1, 640, rec=rec, workspace=ws_x)
        t_win = _per_step(f_window, sync, steps=20)
        t_uni = _per_step(f_union, sync, steps=20)
        t_del = _per_step(f_delta, sync, steps=20)
        t_und = _per_step(f_undelta, sync, steps=20)
        assert not st.any() and torch.equal(oo[1], offs) and torch.equal(outs[1][:stream.numel()], stream)
        t_win2 = _per_step(f_window, sync, steps=20)  # the window call again, after: the spread of the same call in this run
        print(f"    svc_hip_window_levels_frames, no window {fmt(t_win)} (again {fmt(t_win2)})", flush=True)
        print(f"    svc_hip_union_levels_frames of (0, 0, {k}, {k}) and its remainder {fmt(t_uni)}", flush=True)
        print(f"    svc_hip_delta_levels_frames {fmt(t_del)} ({t_del[0] / t_uni[0]:.2f}x the union, {t_del[0] / t_win[0]:.2f}x the window call)", flush=True)
        print(f"    svc_hip_undelta_levels_frames {fmt(t_und)} ({t_und[0] / t_uni[0]:.2f}x the union, {t_und[0] / t_win[0]:.2f}x the window call), "
              f"{(d.numel() + stream.numel()) / t_und[0] / 1e6:.1f} GB/s of input plus output", flush=True)
        t_dec = _per_step(f_decode, sync, steps=20)
        t_both = _per_step(f_undelta_decode, sync, steps=20)
        t_dec2 = _per_step(f_decode, sync, steps=20)
        print(f"    svc_hip_decode_levels_frames {fmt(t_dec)} (again {fmt(t_dec2)}); undelta then decode {fmt(t_both)} ({t_both[0] / t_dec[0]:.2f}x)",
              flush=True)


def pack_layers(cfg) -> None:
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    fg, bg, e = 1, 640, 1
    bgr, types = _batch(cfg, n)
    planes = native.dct_frames(bgr, block)
    del bgr
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    base, fine, lbase, lenh = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(4))
    offs_b, offs_f, lo_b, lo_e = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(4))
    ws1 = torch.empty(native.pack_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(native.pack_layers_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    win = torch.tensor([((pw - 256) // 2 // 16 * 16 + 32 * (f % 7 - 3), (ph - 256) // 2 // 16 * 16 + 16 * (f % 5 - 2), 256, 256) for f in range(n)],
                       dtype=torch.int32, device=dev)
    sync = torch.cuda.synchronize

    def two_calls():
        native.pack_levels_frames(planes, types, block, mv, fg, bg, out=base, offsets=offs_b, workspace=ws1)
        native.pack_levels_frames(planes, types, block, mv, e, e, out=fine, offsets=offs_f, workspace=ws1)

    def layered(window):
        return lambda: native.pack_layers_frames(planes, types, block, mv, fg, bg, e, window=window, base_out=lbase, enh_out=lenh,
                                                 workspace=ws2, base_offsets=lo_b, enh_offsets=lo_e)

    def fmt(t):
        return f"{t[0]:.3f} .. {t[1]:.3f}"

    print(f"{cfg.name} batch of {n} at ({fg}, {bg}, {e}), raw planes {planes.numel() * 4 / n / 1e6:.2f} MB per frame, ms per call (best .. worst "
          f"of 3 runs of 20 back-to-back calls; the routes interleaved: two calls, layers, two calls, layers)", flush=True)
    for name, window in (("a 256 x 256 window per frame", win), ("no window: every tile", None)):
        t2a = _per_step(two_calls, sync, steps=20)
        t1a = _per_step(layered(window), sync, steps=20)
        t2b = _per_step(two_calls, sync, steps=20)
        t1b = _per_step(layered(window), sync, steps=20)
        two_calls()
        layered(window)()
        sync()
        ub, uf, lb, le = int(offs_b[-1]), int(offs_f[-1]), int(lo_b[-1]), int(lo_e[-1])
        assert torch.equal(lo_b, offs_b) and torch.equal(lbase[:ub], base[:ub]), "the base layer differs from svc_hip_pack_levels_frames'"
        t2, t1 = (min(t2a[0], t2b[0]), max(t2a[1], t2b[1])), (min(t1a[0], t1b[0]), max(t1a[1], t1b[1]))
        read2, read1 = 2 * 2 * planes.numel() * 4, 2 * planes.numel() * 4  # every pack reads its planes twice: count, then scatter
        print(f"{name}: pack_levels at ({fg}, {bg}) + at ({e}, {e}) {fmt(t2a)}, again {fmt(t2b)}; pack_layers {fmt(t1a)}, again {fmt(t1b)} "
              f"({t1[0] / t2[0]:.2f} of the two calls by the best of each, {t1[1] / t2[1]:.2f} by the worst); same base bytes", flush=True)
        print(f"    two calls: {(read2 + ub + uf) / 1e6:.1f} MB moved ({(read2 + ub + uf) / (t2[0] * 1e-3) / HBM_PEAK * 100:.1f} % of the HBM peak), "
              f"base {ub / n / 1e6:.3f} + fine {uf / n / 1e6:.3f} MB per frame written; pack_layers: {(read1 + lb + le) / 1e6:.1f} MB moved "
              f"({(read1 + lb + le) / (t1[0] * 1e-3) / HBM_PEAK * 100:.1f} %), base {lb / n / 1e6:.3f} + enhancement {le / n / 1e6:.3f} MB per frame; "
              f"workspace {ws2.numel() / n / 1e6:.3f} MB per frame", flush=True)


def _median_ms(fn, sync, runs=3, steps=20):
    """Wall ms per call over `steps` back-to-back calls: every run, and the median."""
    ts = sorted(_per_step(fn, sync, warm=1, reps=1, steps=steps)[0] for _ in range(runs))
    return ts[len(ts) // 2], ts


def transcode(cfg) -> None:
    import subprocess
    dev = torch.device("cuda")
    n = 8
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    bgr, types = _batch(cfg, n)
    planes = native.dct_frames(bgr, block)
    records = native.serialize_frames(planes, types, pw, ph, block, block, pw // mv, ph // mv, mv)
    del bgr
    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    out_r, out_p = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    offs_r, offs_p = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    ws_r = torch.empty(native.records_pack_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(native.pack_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    rec_out = torch.empty_like(records)
    planes_out, types_out, rec_via = torch.empty_like(planes), torch.empty_like(types), torch.empty_like(records)
    sync = torch.cuda.synchronize
    rec_mb = records.numel() / 1e6
    print(f"{cfg.name} batch of {n}: records {rec_mb / n:.2f} MB per frame; ms per call = the median of 3 runs of 20 back-to-back calls, "
          f"the routes alternating (every run in brackets)", flush=True)
    for fg, bg in ((1, 640), (1, 1)):
        def from_records():
            native.records_pack_levels_frames(records, pw, ph, block, mv, fg, bg, out=out_r, offsets=offs_r, workspace=ws_r, status=status)

        def from_planes():
            native.pack_levels_frames(planes, types, block, mv, fg, bg, out=out_p, offsets=offs_p, workspace=ws_p)

        tr, tp = [], []
        for _ in range(3):
            tp += _median_ms(from_planes, sync, runs=1)[1]
            tr += _median_ms(from_records, sync, runs=1)[1]
        used = int(offs_r[-1])
        assert torch.equal(offs_r, offs_p) and torch.equal(out_r[:used], out_p[:used]) and not status.any(), "records_pack differs from the pack"
        mr, mp = sorted(tr)[1], sorted(tp)[1]
        moved = 2 * records.numel() + used  # count and scatter each read the coefficients
        print(f"({fg}, {bg}) forward: pack_levels on planes {mp:.3f} {[round(t, 3) for t in tp]}, records_pack_levels {mr:.3f} "
              f"{[round(t, 3) for t in tr]} ({mr / mp:.2f} of the planes route); {used / n / 1e6:.3f} MB per frame out, {moved / 1e6:.1f} MB moved, "
              f"{moved / (mr * 1e-3) / HBM_PEAK * 100:.1f} % of the HBM peak; same bytes", flush=True)
        stream = out_r[:used].clone()

        def to_records():
            native.levels_records_frames(stream, offs_r, pw, ph, block, mv, records=rec_out, workspace=ws_p, status=status)

        def via_planes():
            native.unpack_levels_frames(stream, offs_r, pw, ph, block, mv, planes=planes_out, block_types=types_out, workspace=ws_p)
            native.serialize_frames(planes_out, types_out, pw, ph, block, block, pw // mv, ph // mv, mv, out=rec_via)

        tr, tp = [], []
        for _ in range(3):
            tp += _median_ms(via_planes, sync, runs=1)[1]
            tr += _median_ms(to_records, sync, runs=1)[1]
        assert torch.equal(rec_out, rec_via), "levels_records differs from unpack + serialize"
        mr, mp = sorted(tr)[1], sorted(tp)[1]
        print(f"({fg}, {bg}) reverse: unpack_levels + serialize {mp:.3f} {[round(t, 3) for t in tp]}, levels_records {mr:.3f} "
              f"{[round(t, 3) for t in tr]} ({mr / mp:.2f} of the planes route); {(used + records.numel()) / 1e6:.1f} MB moved, "
              f"{(used + records.numel()) / (mr * 1e-3) / HBM_PEAK * 100:.1f} % of the HBM peak; same bytes", flush=True)
    # the drivers, PCIe-inclusive: 24 frames (3 batches of 8) = the batch three times over
    import tempfile
    dropin = os.path.join(ROOT, "tests", "dropin")
    hdr = native.wire_header(3 * n + 1, cfg.width, cfg.height, mv, cfg.levels, block)
    body = records.cpu().numpy().tobytes()
    del planes, planes_out, rec_via, rec_out, out_p
    torch.cuda.empty_cache()
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        wire_path, compact_path = os.path.join(d, "clip.wire"), os.path.join(d, "clip.svcq")
        with open(wire_path, "wb") as f:
            f.write(hdr + body * 3)
        with open(wire_path, "rb") as fin, open(compact_path, "wb") as fout:
            subprocess.run([os.path.join(dropin, "wire_transcode_main"), "to-compact", "--mv-block", str(mv)], stdin=fin, stdout=fout, check=True,
                           timeout=300)
        runs = [("wire_decode_main", [], wire_path), ("wire_transcode_main", ["to-compact", "--mv-block", str(mv), "--rate"], wire_path),
                ("wire_transcode_main", ["to-compact", "--mv-block", str(mv), "--entropy", "--rate"], wire_path),
                ("wire_transcode_main", ["to-wire", "--rate"], compact_path)]
        for turn in range(2):
            for name, args, path in runs:
                with open(path, "rb") as fin:
                    r = subprocess.run([os.path.join(dropin, name), *args], stdin=fin, capture_output=True, text=True, timeout=300)
                print(f"== turn {turn}: {name} {' '.join(args)} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
                if r.returncode != 0:
                    sys.exit(1)


def stream_layers() -> None:
    import subprocess
    import tempfile
    cfg = configs.C3
    n = 65
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cpu")
    pw, ph = cfg.padded
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    dropin = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        raw, win, gaze, q = (os.path.join(d, f) for f in ("clip.raw", "windows.txt", "gaze.txt", "q"))
        with open(raw, "wb") as f:
            for t in range(n):
                clip.frame_bgr(t).numpy().tofile(f)
        # a 256 x 256 window on the MV grid that drifts with the frame, and the gaze centre in its middle
        rects = [((pw - 256) // 2 // 16 * 16 + 32 * (i % 7 - 3), (ph - 256) // 2 // 16 * 16 + 16 * (i % 5 - 2), 256, 256) for i in range(n)]
        with open(win, "w") as f:
            f.write("".join("%d %d %d %d\n" % r for r in rects))
        with open(gaze, "w") as f:  # one line per encoded frame: clip frame i + 1
            f.write("".join("%d %d\n" % (min(r[0] + 128, cfg.width - 1), min(r[1] + 128, cfg.height - 1)) for r in rects[1:]))
        common = [raw, str(cfg.width), str(cfg.height), str(n), str(cfg.levels), str(cfg.dct_block)]
        layered = [*common, "16", "3", str(cfg.seed), "1", "640", "1"]
        runs = [("stream_levels_main", [*common, "0", "16", str(cfg.seed), q], "writes the stream stream_decode_main reads"),
                ("stream_levels_main", [*common, "0", "16", str(cfg.seed), "-"], "one layer at (1, 640)"),
                ("stream_decode_main", [q, str(n - 1), "0", "0", gaze, "16", "-"], "one layer, a gaze per frame"),
                ("stream_entropy_main", [*common, "16", str(cfg.seed), gaze, "-"], "one layer, entropy-coded, a gaze per frame"),
                ("stream_layers_main", [*layered, "0", win, gaze, "-"], "two layers, a 256 x 256 window and a gaze per frame"),
                ("stream_layers_main", [*layered, "1", win, gaze, "-"], "two layers, entropy-coded, the same window and gaze"),
                ("stream_layers_main", [*layered, "0", "-", gaze, "-"], "two layers, every tile enhanced, the same gaze")]
        for turn in range(2):
            for name, args, what in runs[1 if turn else 0:]:
                r = subprocess.run([os.path.join(dropin, name), *args], capture_output=True, text=True, timeout=300)
                print(f"== turn {turn}: {name}: {what} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
                if r.returncode != 0:
                    sys.exit(1)


def step(cfg, frames_n) -> None:
    dev = torch.device("cuda")
    clip = synth.SynthClip(cfg.width, cfg.height, frames_n, cfg.seed, device=dev)
    pw, ph = cfg.padded
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(frames_n)]).contiguous()
    for schedule, name in ((clipmod.SERIAL, "serial"), (clipmod.PIPELINED, "pipelined")):
        # the planes step in the two-pass order, and the pack of its output
        enc = clipmod.Clip(cfg, frames_n, schedule=schedule, tuning=clipmod.TUNE_TWO_BGR_PASSES | clipmod.TUNE_WHOLE_SHARD_STEPS)
        enc.load_frames(frames)
        planes_ms = _per_step(enc.step, enc.sync)
        i = enc.info
        coeffs = enc.read("coeffs", device=dev).view(i.pairs, 3, ph, pw)
        types = enc.read("block_types", device=dev).view(i.pairs, i.blocks)
        enc.close()
        del enc
        out = torch.empty(native.levels_max_bytes(i.pairs, pw, ph, cfg.dct_block, cfg.mv_block), dtype=torch.uint8, device=dev)
        offs = torch.empty(i.pairs + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(native.pack_levels_workspace_bytes(i.pairs, pw, ph, cfg.dct_block), dtype=torch.uint8, device=dev)
        pack_ms = _per_step(lambda: native.pack_levels_frames(coeffs, types, cfg.dct_block, cfg.mv_block, cfg.fg_step, cfg.bg_step, out=out,
                                                              offsets=offs, workspace=ws), torch.cuda.synchronize)
        want, want_offs = out[:int(offs[-1].item())].cpu(), offs.cpu()
        del coeffs, out, ws
        torch.cuda.empty_cache()
        enc = clipmod.Clip(cfg, frames_n, schedule=schedule, compact=True)
        enc.load_frames(frames)
        compact_ms = _per_step(enc.step, enc.sync)
        got, got_offs = enc.read_compact()
        assert torch.equal(got_offs, want_offs) and torch.equal(got, want), "the compact step's bytes differ from the pack of the planes"
        enc.close()
        del enc
        torch.cuda.empty_cache()
        print(f"{cfg.name} {name}, {i.pairs} pairs, ms per step (best .. worst of 3 runs of 4 back-to-back steps): planes step "
              f"{planes_ms[0]:.3f} .. {planes_ms[1]:.3f} + pack {pack_ms[0]:.3f} .. {pack_ms[1]:.3f} = {planes_ms[0] + pack_ms[0]:.3f} .. "
              f"{planes_ms[1] + pack_ms[1]:.3f}; compact step {compact_ms[0]:.3f} .. {compact_ms[1]:.3f} "
              f"({(planes_ms[0] + pack_ms[0]) / compact_ms[0]:.2f}x); {got.numel() / i.pairs / 1e6:.3f} MB per frame, same bytes", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "step":
        step(_cfg(sys.argv, 2), int(sys.argv[3]) if len(sys.argv) > 3 else 300)
    elif mode == "budget_step":
        budget_step(_cfg(sys.argv, 2), int(sys.argv[3]) if len(sys.argv) > 3 else 300)
    elif mode == "budget":
        budget(_cfg(sys.argv, 2))
    elif mode in ("quality", "quality-kernels"):
        quality(_cfg(sys.argv, 2), kernels_only=mode == "quality-kernels")
    elif mode == "quality-variants":
        quality_variants(_cfg(sys.argv, 2))
    elif mode in ("delta-budget", "delta-budget-kernels"):
        delta_budget(_cfg(sys.argv, 2), kernels_only=mode == "delta-budget-kernels")
    elif mode in ("delta-quality", "delta-quality-kernels"):
        delta_quality(_cfg(sys.argv, 2), kernels_only=mode == "delta-quality-kernels")
    elif mode == "quality_step":
        quality_step(_cfg(sys.argv, 2), int(sys.argv[3]) if len(sys.argv) > 3 else 300)
    elif mode == "layers":
        layers(_cfg(sys.argv, 2))
    elif mode == "window":
        window(_cfg(sys.argv, 2))
    elif mode == "window-entropy":
        window_entropy(_cfg(sys.argv, 2))
    elif mode == "split":
        split(_cfg(sys.argv, 2))
    elif mode == "band":
        band(_cfg(sys.argv, 2), int(sys.argv[3]) if len(sys.argv) > 3 else 64)
    elif mode == "delta":
        delta(_cfg(sys.argv, 2))
    elif mode == "delta-encode":
        delta_encode()
    elif mode == "delta-auto":
        delta_auto()
    elif mode == "delta-temporal":
        delta_temporal()
    elif mode == "delta-temporal-encode":
        delta_temporal_encode()
    elif mode == "stream-layers":
        stream_layers()
    elif mode == "transcode":
        transcode(_cfg(sys.argv, 2))
    elif mode == "pack-layers":
        for config in (configs.C3, configs.C5):
            pack_layers(config)
            torch.cuda.empty_cache()
    else:
        kernels(_cfg(sys.argv, 2), fused_only=mode == "fused")
