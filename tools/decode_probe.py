"""The decoder of the compact stream (svc_hip_decode_levels_frames) measured at C3 (1920x1088 padded, 8x8 tiles, MV 16, 16 frames).

  python tools/decode_probe.py kernels   one C3 batch through the resident encoder and the pack, then 5 times each: the chain
                                         unpack + svc_hip_decode_frames, the fused reconstruction, the fused reconstruction + the
                                         display pass (1920x1080 u8); run under `rocprofv3 --kernel-trace --stats -- python ...`
  python tools/decode_probe.py rate      tests/dropin/stream_levels_main writes a 65-frame clip's stream, tests/dropin/stream_decode_main
                                         decodes it to 1920x1080 display frames with a moving gaze centre (PCIe included)
  python tools/decode_probe.py reduced   one C3 batch of 16 at (1, 640), in one process: per reduce 2, 4, 8 the reduced call
                                         (svc_hip_decode_levels_reduced_frames) with the display (W / r, H / r) against
                                         svc_hip_decode_levels_frames with the display pass at that size, alternating, device events;
                                         the bytes each route stores; and at steps (1, 1) the PSNR of both against the r x r box mean
  python tools/decode_probe.py reduced-rate   the 65-frame stream of `rate` through tests/dropin/stream_reduced_main and through
                                         stream_decode_main at the same display sizes (PCIe included)
  python tools/decode_probe.py layers-reduced   one C3 batch of 16 as two layers at (1, 640, 1), in one process: per reduce 2, 4, 8 and for a
                                         64 x 64 gaze and the whole frame gazed, svc_hip_decode_layers_reduced_frames with the display
                                         (W / r, H / r) against svc_hip_decode_layers_frames with the display pass at that size and against
                                         svc_hip_decode_levels_reduced_frames on the base alone, alternating, device events
  python tools/decode_probe.py layers-reduced-rate   tests/dropin/stream_layers_main writes the 65-frame clip as two layers, plain and
                                         entropy-coded; tests/dropin/stream_layers_reduced_main decodes them at reduce r and, as the full
                                         route, at reduce 1 with the display (W / r, H / r) (PCIe included)
  python tools/decode_probe.py delta [C3|C5]   one batch of 16 stored at (1, 1) and at (1, 640) and coded frame against frame, with a key
                                         frame every 16 and with none (the frame before the batch given), in one process: the fused
                                         svc_hip_decode_delta_levels_frames against svc_hip_undelta_levels_frames +
                                         svc_hip_decode_levels_frames, against the decode alone on the undelta'd stream, and with and without
                                         d_last, alternating, device events, the median of three windows; the routes' rec compared
  python tools/decode_probe.py temporal [C3|C5]   `delta`'s batch stored at (1, 640) and at (1, 1) with frame 0 the key frame, coded at periods 1, 2
                                         and 4 (include/svc_hip.h, "Temporal layers"), in one process: svc_hip_undelta_levels_temporal_frames
                                         against svc_hip_undelta_levels_frames, svc_hip_decode_delta_levels_temporal_frames against
                                         svc_hip_decode_delta_levels_frames, and the fused temporal decode against the temporal undelta +
                                         svc_hip_decode_levels_frames, alternating, device events, the median of three windows; the
                                         routes' rec compared
  python tools/decode_probe.py delta-rate   `rate`'s stream and its delta stream (a key frame every 16) through
                                         tests/dropin/stream_decode_main (Decode) and tests/dropin/stream_delta_main (DecodeDelta), PCIe
                                         included, alternating
  python tools/decode_probe.py delta-reduced [C3|C5]   `delta`'s streams; per reduce 2, 4, 8, with the display pass (W / r, H / r): the fused
                                         svc_hip_decode_delta_levels_reduced_frames with and without d_last and on the band (0, 0, K, K) of
                                         the delta stream, against svc_hip_undelta_levels_frames + svc_hip_decode_levels_reduced_frames,
                                         against svc_hip_decode_delta_levels_frames with the display pass at that size, and against the
                                         reduced decode of the plain stream, alternating, device events, the median of three windows; the
                                         routes' rec and display compared
  python tools/decode_probe.py delta-reduced-rate   `delta-rate`'s delta stream; per reduce, tests/dropin/stream_delta_reduced_main
                                         (DecodeDeltaReduced) on the entropy-coded band (0, 0, K, K) and on the full SVCQ delta stream against
                                         stream_delta_main (DecodeDelta) at full size with the display (W / r, H / r), PCIe included, alternating
  python tools/decode_probe.py temporal-reduced [C3|C5]   `temporal`'s batch stored at (1, 640) and at (1, 1), frame 0 the key frame, coded at
                                         periods 2 and 4; per reduce 2, 4, 8, with the display pass (W / r, H / r): the fused
                                         svc_hip_decode_delta_levels_temporal_reduced_frames (include/svc_hip_temporal_decode.h) with and without
                                         d_last, on the full stream and on its band (0, 0, K, K), against (a)
                                         svc_hip_undelta_levels_temporal_frames + svc_hip_decode_levels_reduced_frames, (b)
                                         svc_hip_decode_delta_levels_temporal_frames with the display pass at that size and (c)
                                         svc_hip_decode_delta_levels_reduced_frames on the period-1 stream of the same clip (the price of the
                                         layers), alternating, device events, the median of three windows; the routes' rec and display compared
  python tools/decode_probe.py temporal-reduced-rate   `rate`'s stream coded at periods 2 and 4 (a key frame every 16); per reduce 2 and 8,
                                         tests/dropin/stream_temporal_reduced_main (DecodeDeltaTemporalReduced) on the entropy-coded band
                                         (0, 0, K, K) and on the full SVCQ stream against its reduce-0 mode (DecodeDeltaTemporal at full size with
                                         the display (W / r, H / r)), PCIe included, alternating
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scalable_video_codec_amd import configs, synth  # noqa: E402

CFG = configs.C3


def kernels() -> None:
    import torch
    from scalable_video_codec_amd import native, pipeline
    dev = torch.device("cuda")
    n = 17
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device=dev)
    pw, ph = CFG.padded
    enc = pipeline.ClipEncoder(CFG, n, dev)
    enc.load_frames([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)])
    enc.step()
    planes, types = enc.coeffs, enc.types
    out, offs = native.pack_levels_frames(planes, types, CFG.dct_block, CFG.mv_block, CFG.fg_step, CFG.bg_step)
    m = n - 1
    rects = [native.gaze_rect(100 + 100 * i, 500, 64, 64, CFG.width, CFG.height, pw, ph) for i in range(m)]
    back = torch.empty_like(planes)
    back_types = torch.empty_like(types)
    ws = torch.empty(native.decode_levels_workspace_bytes(m, pw, ph, CFG.dct_block), dtype=torch.uint8, device=dev)
    chain_rec = torch.empty((m, ph, pw, 3), dtype=torch.float32, device=dev)
    rec = torch.empty_like(chain_rec)
    disp = torch.empty((m, CFG.height, CFG.width, 3), dtype=torch.uint8, device=dev)
    for _ in range(5):  # the chain, one rectangle for the whole batch (all the existing entry point takes)
        native.unpack_levels_frames(out, offs, pw, ph, CFG.dct_block, CFG.mv_block, planes=back, block_types=back_types, workspace=ws)
        native.decode_frames(back, CFG.dct_block, back_types, CFG.mv_block, CFG.fg_step, CFG.bg_step, gaze=rects[0], out=chain_rec)
    for _ in range(5):
        native.decode_levels_frames(out, offs, pw, ph, CFG.dct_block, CFG.mv_block, CFG.fg_step, CFG.bg_step, gaze=rects, rec=rec,
                                    workspace=ws)
    for _ in range(5):
        _, _, status = native.decode_levels_frames(out, offs, pw, ph, CFG.dct_block, CFG.mv_block, CFG.fg_step, CFG.bg_step, gaze=rects,
                                                   display=(CFG.width, CFG.height), rec=rec, out_display=disp, workspace=ws)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * m
    total = int(offs[-1].item())
    print(f"C3 batch of {m}: {total / m / 1e6:.3f} MB compact per frame, {pw * ph * 12 / 1e6:.2f} MB f32 rec per frame, "
          f"{CFG.width * CFG.height * 3 / 1e6:.2f} MB display per frame", flush=True)


def _stored_stream(d, n):
    """`rate`'s clip and its stream under directory d -> the stream's prefix."""
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device="cpu")
    raw = os.path.join(d, "clip.raw")
    with open(raw, "wb") as f:
        for t in range(n):
            clip.frame_bgr(t).numpy().tofile(f)
    prefix = os.path.join(d, "enc")
    enc = os.path.join(ROOT, "tests", "dropin", "stream_levels_main")
    r = subprocess.run([enc, raw, str(CFG.width), str(CFG.height), str(n), str(CFG.levels), str(CFG.dct_block), "0", "16",
                        str(CFG.seed), prefix], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        print(r.stdout, r.stderr)
        sys.exit(1)
    return prefix


def rate() -> None:
    n = 65
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        prefix = _stored_stream(d, n)
        gaze = os.path.join(d, "gaze.txt")
        with open(gaze, "w") as f:
            for i in range(n - 1):
                f.write(f"{(60 + 29 * i) % CFG.width} {(40 + 17 * i) % CFG.height}\n")
        dec = os.path.join(ROOT, "tests", "dropin", "stream_decode_main")
        for batch in (16,):
            r = subprocess.run([dec, prefix, str(n - 1), str(CFG.width), str(CFG.height), gaze, str(batch), "-"],
                               capture_output=True, text=True, timeout=300)
            print(f"== stream_decode_main batch {batch} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
            if r.returncode != 0:
                sys.exit(1)


def reduced() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    dev = torch.device("cuda")
    n = 17
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device=dev)
    pw, ph = CFG.padded
    frames = [synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)]
    enc = pipeline.ClipEncoder(CFG, n, dev)
    enc.load_frames(frames)
    enc.step()
    planes, types = enc.coeffs, enc.types
    block, mvb = CFG.dct_block, CFG.mv_block
    out, offs = native.pack_levels_frames(planes, types, block, mvb, CFG.fg_step, CFG.bg_step)
    m = n - 1
    total = int(offs[-1].item())
    ws = torch.empty(native.decode_levels_workspace_bytes(m, pw, ph, block), dtype=torch.uint8, device=dev)
    rec_full = torch.empty((m, ph, pw, 3), dtype=torch.float32, device=dev)
    print(f"C3 batch of {m} at steps ({CFG.fg_step}, {CFG.bg_step}): {total / m / 1e6:.3f} MB compact per frame", flush=True)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for r in (2, 4, 8):
        rw, rh = pw // r, ph // r
        rects = [native.gaze_rect((50 + 50 * i) // r, 500 // r, 64, 64, rw, rh, pw, ph) for i in range(m)]
        rec = torch.empty((m, rh, rw, 3), dtype=torch.float32, device=dev)
        disp_r = torch.empty((m, rh, rw, 3), dtype=torch.uint8, device=dev)
        disp_f = torch.empty_like(disp_r)

        def red():
            native.decode_levels_reduced_frames(out, offs, pw, ph, block, mvb, CFG.fg_step, CFG.bg_step, reduce=r, gaze=rects,
                                                display=(rw, rh), rec=rec, out_display=disp_r, workspace=ws)

        def full():
            native.decode_levels_frames(out, offs, pw, ph, block, mvb, CFG.fg_step, CFG.bg_step, gaze=rects, display=(rw, rh),
                                        rec=rec_full, out_display=disp_f, workspace=ws)

        for _ in range(3):
            red(), full()
        torch.cuda.synchronize()
        t_red, t_full = [], []
        for _ in range(7):  # alternating windows of 20 batches each
            t_red.append(timed(red, 20))
            t_full.append(timed(full, 20))
        b_red = rw * rh * 12 + rw * rh * 3
        b_full = pw * ph * 12 + rw * rh * 3
        print(f"reduce {r}: display {rw}x{rh}; reduced call {np.median(t_red):.3f} ms per batch (min {min(t_red):.3f}, max {max(t_red):.3f}), "
              f"stores {b_red / 1e6:.2f} MB per frame; full call + display pass {np.median(t_full):.3f} ms per batch (min {min(t_full):.3f}, "
              f"max {max(t_full):.3f}), stores {b_full / 1e6:.2f} MB per frame; full / reduced = {np.median(t_full) / np.median(t_red):.2f}",
              flush=True)

    # quality at steps (1, 1): both routes' display frames against the r x r box mean of the padded source
    bgr = torch.stack(frames[1:]).contiguous()
    planes1 = native.dct_quant_frames(bgr, block, types, mvb, 1, 1)
    out1, offs1 = native.pack_levels_frames(planes1, types, block, mvb, 1, 1)

    def psnr(a, target):
        mse = float(((a.float() - target) ** 2).mean().item())
        return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))

    for r in (2, 4, 8):
        rw, rh = pw // r, ph // r
        target = bgr.float().reshape(m, rh, r, rw, r, 3).mean(dim=(2, 4))
        _, d_red, _ = native.decode_levels_reduced_frames(out1, offs1, pw, ph, block, mvb, 1, 1, reduce=r, display=(rw, rh))
        _, d_full, _ = native.decode_levels_frames(out1, offs1, pw, ph, block, mvb, 1, 1, display=(rw, rh), rec=rec_full)
        torch.cuda.synchronize()
        print(f"quality at steps (1, 1), reduce {r}, against the {r}x{r} box mean of the source: reduced decode {psnr(d_red, target):.2f} dB, "
              f"full decode + bilinear display {psnr(d_full, target):.2f} dB", flush=True)


def reduced_rate() -> None:
    n = 65
    pw, ph = CFG.padded
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    here = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        prefix = _stored_stream(d, n)
        for r in (2, 4, 8):
            dw, dh = pw // r, ph // r
            gaze = os.path.join(d, f"gaze{r}.txt")
            with open(gaze, "w") as f:
                for i in range(n - 1):
                    f.write(f"{(60 + 29 * i) % dw} {(40 + 17 * i) % dh}\n")
            for turn in range(3):  # alternating, every run printed: the spread is part of the result
                for name, args in (("stream_reduced_main", [str(r), "0", "0"]), ("stream_decode_main", [str(dw), str(dh)])):
                    p = subprocess.run([os.path.join(here, name), prefix, str(n - 1), *args, gaze, "16", "-"], capture_output=True,
                                       text=True, timeout=300)
                    print(f"== {name} display {dw}x{dh} batch 16, run {turn} (exit {p.returncode})\n{p.stdout.strip()}\n{p.stderr.strip()}",
                          flush=True)
                    if p.returncode != 0:
                        sys.exit(1)


def layers_reduced() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    dev = torch.device("cuda")
    m = 16
    clip = synth.SynthClip(CFG.width, CFG.height, m + 1, CFG.seed, device=dev)
    pw, ph = CFG.padded
    frames = [synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(m + 1)]
    enc = pipeline.ClipEncoder(CFG, m + 1, dev)  # `reduced`'s batch: the region ids are the encoder's
    enc.load_frames(frames)
    enc.step()
    types = enc.types
    bgr = torch.stack(frames[1:]).contiguous()
    block, mvb = CFG.dct_block, CFG.mv_block
    fg, bg, e = CFG.fg_step, CFG.bg_step, 1
    base, bo, enh, eo = native.dct_pack_layers_frames(bgr, block, types, mvb, fg, bg, e)
    torch.cuda.synchronize()
    ub, ue = int(bo[-1]), int(eo[-1])
    base, enh = base[:ub].clone(), enh[:ue].clone()
    ws = torch.empty(native.decode_layers_reduced_workspace_bytes(m, pw, ph, block), dtype=torch.uint8, device=dev)
    rec_full = torch.empty((m, ph, pw, 3), dtype=torch.float32, device=dev)
    print(f"C3 batch of {m} as two layers at ({fg}, {bg}, {e}): {ub / m / 1e6:.3f} MB of base and {ue / m / 1e6:.3f} MB of enhancement per frame",
          flush=True)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def fmt(t):
        return f"{np.median(t):.3f} ms per batch (min {min(t):.3f}, max {max(t):.3f})"

    for r in (2, 4, 8):
        rw, rh = pw // r, ph // r
        small = [native.gaze_rect((50 + 50 * i) // r, 500 // r, 64, 64, rw, rh, pw, ph) for i in range(m)]
        rec = torch.empty((m, rh, rw, 3), dtype=torch.float32, device=dev)
        disp_r, disp_f, disp_b = (torch.empty((m, rh, rw, 3), dtype=torch.uint8, device=dev) for _ in range(3))
        for name, rects in (("64 x 64", small), ("the whole frame", [(0, 0, pw, ph)] * m)):
            gaze = torch.tensor(rects, dtype=torch.int32, device=dev)

            def red():
                native.decode_layers_reduced_frames(base, bo, enh, eo, pw, ph, block, mvb, fg, bg, reduce=r, gaze=gaze, display=(rw, rh),
                                                    rec=rec, out_display=disp_r, workspace=ws)

            def full():
                native.decode_layers_frames(base, bo, enh, eo, pw, ph, block, mvb, fg, bg, gaze=gaze, display=(rw, rh), rec=rec_full,
                                            out_display=disp_f, workspace=ws)

            def one():
                native.decode_levels_reduced_frames(base, bo, pw, ph, block, mvb, fg, bg, reduce=r, gaze=gaze, display=(rw, rh), rec=rec,
                                                    out_display=disp_b, workspace=ws)

            for _ in range(3):
                red(), full(), one()
            torch.cuda.synchronize()
            t_red, t_full, t_one = [], [], []
            for _ in range(7):  # alternating windows of 20 batches each
                t_red.append(timed(red, 20))
                t_full.append(timed(full, 20))
                t_one.append(timed(one, 20))
            print(f"reduce {r}, gaze {name}: display {rw}x{rh}; layered reduced call {fmt(t_red)}; full layered call + display pass {fmt(t_full)}, "
                  f"full / reduced = {np.median(t_full) / np.median(t_red):.2f}; one-stream reduced call on the base {fmt(t_one)}, "
                  f"layered / one-stream = {np.median(t_red) / np.median(t_one):.2f}", flush=True)


def layers_reduced_rate() -> None:
    n = 65
    pw, ph = CFG.padded
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    here = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device="cpu")
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(n):
                clip.frame_bgr(t).numpy().tofile(f)
        prefixes = {}
        for coded in (0, 1):
            prefixes[coded] = os.path.join(d, f"layers{coded}")
            p = subprocess.run([os.path.join(here, "stream_layers_main"), raw, str(CFG.width), str(CFG.height), str(n), str(CFG.levels),
                                str(CFG.dct_block), "16", "3", str(CFG.seed), str(CFG.fg_step), str(CFG.bg_step), "1", str(coded), "-", "-",
                                prefixes[coded]], capture_output=True, text=True, timeout=600)
            print(f"== stream_layers_main entropy {coded} (exit {p.returncode})\n{p.stdout.strip()}\n{p.stderr.strip()}", flush=True)
            if p.returncode != 0:
                sys.exit(1)
            os.remove(prefixes[coded] + ".display")
        exe = os.path.join(here, "stream_layers_reduced_main")
        for r in (2, 4, 8):
            dw, dh = pw // r, ph // r
            gaze = os.path.join(d, f"gaze{r}.txt")
            with open(gaze, "w") as f:
                for i in range(n - 1):
                    f.write(f"{(60 + 29 * i) % dw} {(40 + 17 * i) % dh}\n")
            for coded in (0, 1):
                for turn in range(3):  # alternating, every run printed: the spread is part of the result
                    for name, args in (("reduced", [str(r), "0", "0"]), ("full", ["1", str(dw), str(dh)])):
                        p = subprocess.run([exe, prefixes[coded], str(n - 1), *args, gaze, "16", "-"], capture_output=True, text=True, timeout=300)
                        print(f"== stream_layers_reduced_main {name} ({'SVCE' if coded else 'SVCQ'}) display {dw}x{dh} batch 16, run {turn} "
                              f"(exit {p.returncode})\n{p.stdout.strip()}\n{p.stderr.strip()}", flush=True)
                        if p.returncode != 0:
                            sys.exit(1)


def delta() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = {"C3": configs.C3, "C5": configs.C5}[sys.argv[2] if len(sys.argv) > 2 else "C3"]
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    clip = synth.SynthClip(cfg.width, cfg.height, n + 2, cfg.seed, device=dev)
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n + 2)]).contiguous()
    enc = pipeline.ClipEncoder(cfg, n + 2, dev)
    enc.load_frames(list(frames))
    enc.step()
    torch.cuda.synchronize()
    bgr, types = frames[1:].contiguous(), enc.types.clone()  # n + 1 encoded frames: the frame before the batch, then the batch

    def timed(fn, reps=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def fmt(t):
        return f"{np.median(t):.3f} (min {min(t):.3f}, max {max(t):.3f})"

    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    back, bo = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_u = torch.empty(native.undelta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_x = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(native.decode_delta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    rec, rec2 = (torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev) for _ in range(2))
    last = torch.empty(native.levels_max_bytes(1, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st, st2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}; ms per call of {n} frames, device events over 20 back-to-back calls, the median of "
          f"three such windows per route, the routes alternating; workspace of the fused call {ws_f.numel() / 1e6:.1f} MB", flush=True)
    for steps in ((1, 1), (1, 640)):
        out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, *steps)
        torch.cuda.synchronize()
        o = offs.cpu().tolist()
        prev, stream, so = out[:o[1]].clone(), out[o[1]:o[-1]].clone(), (offs[1:] - offs[1]).contiguous()
        for name, keys, before in (("a key frame every 16", [1] + [0] * (n - 1), None), ("no key frame", None, prev)):
            d, do, dst = native.delta_levels_frames(stream, so, pw, ph, block, mv, prev=before, key=keys)
            torch.cuda.synchronize()
            assert not dst.any()
            d = d[:int(do[-1])].clone()

            def two():
                native.undelta_levels_frames(d, do, pw, ph, block, mv, prev=before, key=keys, out=back, out_offsets=bo, workspace=ws_u, status=st2)
                native.decode_levels_frames(back, bo, pw, ph, block, mv, 1, 640, rec=rec2, workspace=ws_x)

            def decode_alone():  # on the stream the undelta left in `back`
                native.decode_levels_frames(back, bo, pw, ph, block, mv, 1, 640, rec=rec2, workspace=ws_x)

            def fused():
                native.decode_delta_levels_frames(d, do, pw, ph, block, mv, 1, 640, prev=before, key=keys, rec=rec, last=last, workspace=ws_f,
                                                  status=st)

            def fused_no_last():
                native.decode_delta_levels_frames(d, do, pw, ph, block, mv, 1, 640, prev=before, key=keys, rec=rec, workspace=ws_f, status=st)

            for _ in range(2):
                two(), fused(), fused_no_last(), decode_alone()
            torch.cuda.synchronize()
            assert not st.any() and not st2.any() and torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "the routes differ"
            assert torch.equal(back[:stream.numel()], stream)
            t = {k: [] for k in ("two", "fused", "no_last", "alone")}
            for _ in range(3):
                t["two"].append(timed(two))
                t["fused"].append(timed(fused))
                t["alone"].append(timed(decode_alone))
                t["no_last"].append(timed(fused_no_last))
            m = {k: float(np.median(v)) for k, v in t.items()}
            print(f"stored at {steps}, {name} ({d.numel() / n / 1e6:.3f} MB per delta frame): undelta + decode {fmt(t['two'])}; "
                  f"svc_hip_decode_delta_levels_frames {fmt(t['fused'])} = {m['fused'] / m['two']:.2f}x of the two calls, "
                  f"{m['fused'] / m['alone']:.2f}x of the decode alone {fmt(t['alone'])}; without d_last {fmt(t['no_last'])}", flush=True)


def temporal() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = {"C3": configs.C3, "C5": configs.C5}[sys.argv[2] if len(sys.argv) > 2 else "C3"]
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    clip = synth.SynthClip(cfg.width, cfg.height, n + 1, cfg.seed, device=dev)
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n + 1)]).contiguous()
    enc = pipeline.ClipEncoder(cfg, n + 1, dev)
    enc.load_frames(list(frames))
    enc.step()
    torch.cuda.synchronize()
    bgr, types = frames[1:].contiguous(), enc.types.clone()

    def timed(fn, reps=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    back, bo = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_u = torch.empty(native.undelta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_x = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(native.decode_delta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    rec, rec2 = (torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev) for _ in range(2))
    last = torch.empty(native.levels_max_bytes(1, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st, st2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    keys = [1] + [0] * (n - 1)
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, frame 0 the key frame; ms per call of {n} frames, device events over 20 back-to-back "
          f"calls, the median of three such windows per route, the routes alternating", flush=True)
    for steps in ((1, 640), (1, 1)):
        out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, *steps)
        torch.cuda.synchronize()
        stream = out[:int(offs[-1])].clone()
        routes, sizes = {}, {}
        for period in (1, 2, 4):
            if period == 1:
                d, do, dst = native.delta_levels_frames(stream, offs, pw, ph, block, mv, key=keys)
            else:
                d, do, dst = native.delta_levels_temporal_frames(stream, offs, pw, ph, block, mv, period, key=keys)
            torch.cuda.synchronize()
            assert not dst.any()
            d = d[:int(do[-1])].clone()
            sizes[period] = d.numel() / n / 1e6

            def undelta(d=d, do=do, period=period):
                if period == 1:
                    native.undelta_levels_frames(d, do, pw, ph, block, mv, key=keys, out=back, out_offsets=bo, workspace=ws_u, status=st2)
                else:
                    native.undelta_levels_temporal_frames(d, do, pw, ph, block, mv, period, key=keys, out=back, out_offsets=bo, workspace=ws_u,
                                                          status=st2)

            def two(undelta=undelta):
                undelta()
                native.decode_levels_frames(back, bo, pw, ph, block, mv, 1, 640, rec=rec2, workspace=ws_x)

            def fused(d=d, do=do, period=period):
                if period == 1:
                    native.decode_delta_levels_frames(d, do, pw, ph, block, mv, 1, 640, key=keys, rec=rec, last=last, workspace=ws_f, status=st)
                else:
                    native.decode_delta_levels_temporal_frames(d, do, pw, ph, block, mv, period, fg_step=1, bg_step=640, key=keys, rec=rec,
                                                               last=last, workspace=ws_f, status=st)

            two(), fused()
            torch.cuda.synchronize()
            assert not st.any() and not st2.any() and torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "the routes differ"
            assert torch.equal(back[:stream.numel()], stream)
            routes[period] = (undelta, two, fused)
        t = {(p, k): [] for p in routes for k in range(3)}
        for _ in range(3):
            for p, fns in routes.items():
                for k, fn in enumerate(fns):
                    t[p, k].append(timed(fn))
        m = {key: float(np.median(v)) for key, v in t.items()}
        for p in (1, 2, 4):
            print(f"stored at {steps}, period {p} ({sizes[p]:.3f} MB per delta frame): undelta {m[p, 0]:.3f} ({m[p, 0] / m[1, 0]:.2f}x of period 1); "
                  f"undelta + decode {m[p, 1]:.3f}; fused decode {m[p, 2]:.3f} = {m[p, 2] / m[p, 1]:.2f}x of the two calls, "
                  f"{m[p, 2] / m[1, 2]:.2f}x of period 1's fused decode (min {min(t[p, 2]):.3f}, max {max(t[p, 2]):.3f})", flush=True)


def delta_rate() -> None:
    """DecodeDelta against Decode on the same clip's plain stream, PCIe included: `rate`'s 64 frames, their delta stream made on the device."""
    import numpy as np
    import torch
    from scalable_video_codec_amd import native
    n = 65
    m = n - 1
    pw, ph = CFG.padded
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    here = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        prefix = _stored_stream(d, n)
        big = torch.from_numpy(np.fromfile(prefix + ".big", np.uint8)).cuda()
        offs = torch.from_numpy(np.fromfile(prefix + ".offsets", np.uint64).astype(np.int64)).cuda()
        keys = [int(i % 16 == 0) for i in range(m)]
        diff, do, st = native.delta_levels_frames(big, offs, pw, ph, CFG.dct_block, CFG.mv_block, key=keys)
        torch.cuda.synchronize()
        assert not st.any()
        dprefix = os.path.join(d, "delta")
        diff[:int(do[-1])].cpu().numpy().tofile(dprefix + ".big")
        do.cpu().numpy().astype(np.uint64).tofile(dprefix + ".offsets")
        print(f"{m} frames: plain stream {big.numel() / m / 1e6:.3f} MB per frame, delta stream (a key frame every 16) {int(do[-1]) / m / 1e6:.3f}",
              flush=True)
        del big, diff
        key_file, gaze = os.path.join(d, "key.txt"), os.path.join(d, "gaze.txt")
        with open(key_file, "w") as f:
            f.write("".join(f"{k}\n" for k in keys))
        with open(gaze, "w") as f:
            for i in range(m):
                f.write(f"{(60 + 29 * i) % CFG.width} {(40 + 17 * i) % CFG.height}\n")
        size = [str(CFG.width), str(CFG.height)]
        for turn in range(3):  # alternating, every run printed: the spread is part of the result
            for name, args in (("stream_decode_main", [prefix, str(m), *size, gaze, "16", "-"]),
                               ("stream_delta_main", [dprefix, str(m), *size, gaze, key_file, "16", "3", "1", "-"])):
                p = subprocess.run([os.path.join(here, name), *args], capture_output=True, text=True, timeout=300)
                print(f"== {name} batch 16, run {turn} (exit {p.returncode})\n{p.stdout.strip()}\n{p.stderr.strip()}", flush=True)
                if p.returncode != 0:
                    sys.exit(1)


def delta_reduced() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = {"C3": configs.C3, "C5": configs.C5}[sys.argv[2] if len(sys.argv) > 2 else "C3"]
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    clip = synth.SynthClip(cfg.width, cfg.height, n + 2, cfg.seed, device=dev)
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n + 2)]).contiguous()
    enc = pipeline.ClipEncoder(cfg, n + 2, dev)
    enc.load_frames(list(frames))
    enc.step()
    torch.cuda.synchronize()
    bgr, types = frames[1:].contiguous(), enc.types.clone()  # n + 1 encoded frames: the frame before the batch, then the batch

    def timed(fn, reps=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def fmt(t):
        return f"{np.median(t):.3f} (min {min(t):.3f}, max {max(t):.3f})"

    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    back, bo = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_u = torch.empty(native.undelta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_x = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(native.decode_delta_levels_reduced_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    rec_full = torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev)
    last = torch.empty(native.levels_max_bytes(1, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st, st2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}; ms per call of {n} frames with the display pass (W / r, H / r), device events over 20 "
          f"back-to-back calls, the median of three such windows per route, the routes alternating; workspace of the fused call "
          f"{ws_f.numel() / 1e6:.1f} MB", flush=True)
    for steps in ((1, 1), (1, 640)):
        out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, *steps)
        torch.cuda.synchronize()
        o = offs.cpu().tolist()
        prev, stream, so = out[:o[1]].clone(), out[o[1]:o[-1]].clone(), (offs[1:] - offs[1]).contiguous()
        for name, keys, before in (("a key frame every 16", [1] + [0] * (n - 1), None), ("no key frame", None, prev)):
            d, do, dst = native.delta_levels_frames(stream, so, pw, ph, block, mv, prev=before, key=keys)
            torch.cuda.synchronize()
            assert not dst.any()
            d = d[:int(do[-1])].clone()
            for r in (2, 4, 8):
                k = block // r
                rw, rh = pw // r, ph // r
                rec, rec2 = (torch.empty((n, rh, rw, 3), dtype=torch.float32, device=dev) for _ in range(2))
                disp, disp2 = (torch.empty((n, rh, rw, 3), dtype=torch.uint8, device=dev) for _ in range(2))
                b, b_offs, bst = native.band_levels_frames(d, do, pw, ph, block, mv, band=[(0, 0, k, k)] * n)  # what a server sends
                torch.cuda.synchronize()
                assert not bst.any()
                b = b[:int(b_offs[-1])].clone()
                b_prev = None
                if before is not None:
                    p, p_offs, _ = native.band_levels_frames(before, torch.tensor([0, before.numel()], dtype=torch.int64, device=dev), pw, ph,
                                                             block, mv, band=[(0, 0, k, k)])
                    b_prev = p[:int(p_offs[1])].clone()
                kw = dict(gaze=None, display=(rw, rh))

                def two():  # the route the fused call replaces
                    native.undelta_levels_frames(d, do, pw, ph, block, mv, prev=before, key=keys, out=back, out_offsets=bo, workspace=ws_u,
                                                 status=st2)
                    native.decode_levels_reduced_frames(back, bo, pw, ph, block, mv, 1, 640, r, rec=rec2, out_display=disp2, workspace=ws_x, **kw)

                def plain():  # the reduced decode on the plain stream the undelta left in `back`: the price of the chain
                    native.decode_levels_reduced_frames(back, bo, pw, ph, block, mv, 1, 640, r, rec=rec2, out_display=disp2, workspace=ws_x, **kw)

                def full():  # what a small viewer pays today: the full-size fused decode with the display pass at the reduced size
                    native.decode_delta_levels_frames(d, do, pw, ph, block, mv, 1, 640, prev=before, key=keys, rec=rec_full, out_display=disp2,
                                                      workspace=ws_f, status=st2, **kw)

                def fused():
                    native.decode_delta_levels_reduced_frames(d, do, pw, ph, block, mv, 1, 640, r, prev=before, key=keys, rec=rec,
                                                              out_display=disp, last=last, workspace=ws_f, status=st, **kw)

                def fused_no_last():
                    native.decode_delta_levels_reduced_frames(d, do, pw, ph, block, mv, 1, 640, r, prev=before, key=keys, rec=rec,
                                                              out_display=disp, workspace=ws_f, status=st, **kw)

                def on_band():
                    native.decode_delta_levels_reduced_frames(b, b_offs, pw, ph, block, mv, 1, 640, r, prev=b_prev, key=keys, rec=rec,
                                                              out_display=disp, workspace=ws_f, status=st, **kw)

                routes = {"two": two, "plain": plain, "full": full, "fused": fused, "no_last": fused_no_last, "band": on_band}
                for _ in range(2):
                    for fn in routes.values():
                        fn()
                torch.cuda.synchronize()
                two(), on_band()
                torch.cuda.synchronize()
                assert not st.any() and not st2.any() and torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "the routes differ"
                assert torch.equal(disp, disp2)
                t = {name_: [] for name_ in routes}
                for _ in range(3):
                    for name_, fn in routes.items():
                        t[name_].append(timed(fn))
                m = {k_: float(np.median(v)) for k_, v in t.items()}
                print(f"stored at {steps}, {name}, reduce {r} ({d.numel() / n / 1e6:.3f} MB per delta frame, {b.numel() / n / 1e6:.3f} in its band): "
                      f"fused without d_last {fmt(t['no_last'])}; with d_last {fmt(t['fused'])}; on the band stream {fmt(t['band'])}; "
                      f"undelta + reduced decode {fmt(t['two'])}, fused / two = {m['no_last'] / m['two']:.2f}; full-size fused decode + display "
                      f"{fmt(t['full'])}, fused / full = {m['no_last'] / m['full']:.2f}; reduced decode of the plain stream {fmt(t['plain'])}, "
                      f"fused / plain = {m['no_last'] / m['plain']:.2f}", flush=True)


def delta_reduced_rate() -> None:
    """DecodeDeltaReduced on the band SVCE stream and on the full SVCQ stream against DecodeDelta at full size on the same clip, PCIe
    included: `rate`'s 64 frames, their delta stream (a key frame every 16), its bands and their entropy coding made on the device."""
    import numpy as np
    import torch
    from scalable_video_codec_amd import native
    n = 65
    m = n - 1
    pw, ph = CFG.padded
    block, mv = CFG.dct_block, CFG.mv_block
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    here = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        prefix = _stored_stream(d, n)
        big = torch.from_numpy(np.fromfile(prefix + ".big", np.uint8)).cuda()
        offs = torch.from_numpy(np.fromfile(prefix + ".offsets", np.uint64).astype(np.int64)).cuda()
        keys = [int(i % 16 == 0) for i in range(m)]
        diff, do, st = native.delta_levels_frames(big, offs, pw, ph, block, mv, key=keys)
        torch.cuda.synchronize()
        assert not st.any()
        diff = diff[:int(do[-1])].clone()

        def store(name, data, data_offs):
            p = os.path.join(d, name)
            data[:int(data_offs[-1])].cpu().numpy().tofile(p + ".big")
            data_offs.cpu().numpy().astype(np.uint64).tofile(p + ".offsets")
            return p, int(data_offs[-1]) / m / 1e6

        dprefix, mb_full = store("delta", diff, do)
        key_file = os.path.join(d, "key.txt")
        with open(key_file, "w") as f:
            f.write("".join(f"{k}\n" for k in keys))
        print(f"{m} frames: plain stream {big.numel() / m / 1e6:.3f} MB per frame, delta stream (a key frame every 16) {mb_full:.3f}", flush=True)
        del big
        for r in (2, 4, 8):
            k = block // r
            dw, dh = pw // r, ph // r
            band, bo, bst = native.band_levels_frames(diff, do, pw, ph, block, mv, band=[(0, 0, k, k)] * m)
            coded, co, est = native.entropy_encode_frames(band[:int(bo[-1])].clone(), bo, pw, ph, block, mv)
            torch.cuda.synchronize()
            assert not bst.any() and not est.any()
            bprefix, mb_band = store(f"band{r}", coded, co)
            print(f"reduce {r}: the band (0, 0, {k}, {k}) of the delta stream {int(bo[-1]) / m / 1e6:.3f} MB per frame, entropy-coded {mb_band:.3f}",
                  flush=True)
            gaze = os.path.join(d, f"gaze{r}.txt")
            with open(gaze, "w") as f:
                for i in range(m):
                    f.write(f"{(60 + 29 * i) % dw} {(40 + 17 * i) % dh}\n")
            tail = [gaze, key_file, "16", "3"]
            for turn in range(3):  # alternating, every run printed: the spread is part of the result
                for what, name, args in (("band SVCE", "stream_delta_reduced_main", [bprefix, str(m), "0", "0", *tail, str(r), "-"]),
                                         ("full SVCQ", "stream_delta_reduced_main", [dprefix, str(m), "0", "0", *tail, str(r), "-"]),
                                         ("full size", "stream_delta_main", [dprefix, str(m), str(dw), str(dh), *tail, "1", "-"])):
                    p = subprocess.run([os.path.join(here, name), *args], capture_output=True, text=True, timeout=300)
                    print(f"== {name} ({what}) display {dw}x{dh} batch 16, run {turn} (exit {p.returncode})\n{p.stdout.strip()}\n{p.stderr.strip()}",
                          flush=True)
                    if p.returncode != 0:
                        sys.exit(1)


def temporal_reduced() -> None:
    import numpy as np
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = {"C3": configs.C3, "C5": configs.C5}[sys.argv[2] if len(sys.argv) > 2 else "C3"]
    dev = torch.device("cuda")
    n = 16
    pw, ph = cfg.padded
    block, mv = cfg.dct_block, cfg.mv_block
    clip = synth.SynthClip(cfg.width, cfg.height, n + 1, cfg.seed, device=dev)
    frames = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n + 1)]).contiguous()
    enc = pipeline.ClipEncoder(cfg, n + 1, dev)
    enc.load_frames(list(frames))
    enc.step()
    torch.cuda.synchronize()
    bgr, types = frames[1:].contiguous(), enc.types.clone()

    def timed(fn, reps=20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def fmt(t):
        return f"{np.median(t):.3f} (min {min(t):.3f}, max {max(t):.3f})"

    cap = native.levels_max_bytes(n, pw, ph, block, mv)
    back, bo = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_u = torch.empty(native.undelta_levels_workspace_bytes(n, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    ws_x = torch.empty(native.decode_levels_workspace_bytes(n, pw, ph, block), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(native.decode_delta_levels_temporal_reduced_workspace_bytes(n, pw, ph, block, mv, 4), dtype=torch.uint8, device=dev)
    rec_full = torch.empty((n, ph, pw, 3), dtype=torch.float32, device=dev)
    last = torch.empty(native.levels_max_bytes(1, pw, ph, block, mv), dtype=torch.uint8, device=dev)
    st, st2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    keys = [1] + [0] * (n - 1)
    print(f"{cfg.name} batch of {n}, tiles {block} x {block}, frame 0 the key frame; ms per call of {n} frames with the display pass (W / r, H / r), "
          f"device events over 20 back-to-back calls, the median of three such windows per route, the routes alternating", flush=True)
    for steps in ((1, 640), (1, 1)):
        out, offs = native.dct_pack_levels_frames(bgr, block, types, mv, *steps)
        torch.cuda.synchronize()
        stream = out[:int(offs[-1])].clone()
        d1, d1o, dst = native.delta_levels_frames(stream, offs, pw, ph, block, mv, key=keys)  # the period-1 stream of the same clip
        torch.cuda.synchronize()
        assert not dst.any()
        d1 = d1[:int(d1o[-1])].clone()
        for period in (2, 4):
            d, do, dst = native.delta_levels_temporal_frames(stream, offs, pw, ph, block, mv, period, key=keys)
            torch.cuda.synchronize()
            assert not dst.any()
            d = d[:int(do[-1])].clone()
            for r in (2, 4, 8):
                k = block // r
                rw, rh = pw // r, ph // r
                rec, rec2 = (torch.empty((n, rh, rw, 3), dtype=torch.float32, device=dev) for _ in range(2))
                disp, disp2 = (torch.empty((n, rh, rw, 3), dtype=torch.uint8, device=dev) for _ in range(2))
                b, b_offs, bst = native.band_levels_frames(d, do, pw, ph, block, mv, band=[(0, 0, k, k)] * n)  # what a server sends
                torch.cuda.synchronize()
                assert not bst.any()
                b = b[:int(b_offs[-1])].clone()
                kw = dict(gaze=None, display=(rw, rh))

                def two():  # (a) the route the fused call replaces
                    native.undelta_levels_temporal_frames(d, do, pw, ph, block, mv, period, key=keys, out=back, out_offsets=bo, workspace=ws_u,
                                                          status=st2)
                    native.decode_levels_reduced_frames(back, bo, pw, ph, block, mv, 1, 640, r, rec=rec2, out_display=disp2, workspace=ws_x, **kw)

                def full():  # (b) the full-size temporal decode with the display pass at the reduced size
                    native.decode_delta_levels_temporal_frames(d, do, pw, ph, block, mv, period, fg_step=1, bg_step=640, key=keys, rec=rec_full,
                                                               out_display=disp2, workspace=ws_f, status=st2, **kw)

                def plain():  # (c) the reduced decode of the period-1 delta stream: the price of the layers
                    native.decode_delta_levels_reduced_frames(d1, d1o, pw, ph, block, mv, 1, 640, r, key=keys, rec=rec2, out_display=disp2,
                                                              workspace=ws_f, status=st2, **kw)

                def fused(data=d, data_offs=do, want_last=None):
                    native.decode_delta_levels_temporal_reduced_frames(data, data_offs, pw, ph, block, mv, period, 1, 640, r, key=keys, rec=rec,
                                                                       out_display=disp, last=want_last, workspace=ws_f, status=st, **kw)

                routes = {"two": two, "full": full, "plain": plain, "no_last": fused, "fused": lambda: fused(want_last=last),
                          "band": lambda: fused(b, b_offs), "band_last": lambda: fused(b, b_offs, last)}
                for _ in range(2):
                    for fn in routes.values():
                        fn()
                torch.cuda.synchronize()
                for fn in (routes["fused"], routes["band_last"]):  # both streams against the two calls, bit for bit
                    rec.zero_(), disp.zero_()
                    two(), fn()
                    torch.cuda.synchronize()
                    assert not st.any() and not st2.any() and torch.equal(rec.view(torch.int32), rec2.view(torch.int32)), "the routes differ"
                    assert torch.equal(disp, disp2)
                t = {name_: [] for name_ in routes}
                for _ in range(3):
                    for name_, fn in routes.items():
                        t[name_].append(timed(fn))
                m = {k_: float(np.median(v)) for k_, v in t.items()}
                print(f"stored at {steps}, period {period}, reduce {r} ({d.numel() / n / 1e6:.3f} MB per delta frame, {b.numel() / n / 1e6:.3f} in its "
                      f"band): fused without d_last {fmt(t['no_last'])}; with d_last {fmt(t['fused'])}; on the band stream {fmt(t['band'])}; on the "
                      f"band with d_last {fmt(t['band_last'])}; (a) temporal undelta + reduced decode {fmt(t['two'])}, fused / a = "
                      f"{m['no_last'] / m['two']:.2f}; (b) full-size temporal decode + display {fmt(t['full'])}, fused / b = "
                      f"{m['no_last'] / m['full']:.2f}; (c) period-1 reduced delta decode {fmt(t['plain'])}, fused / c = "
                      f"{m['no_last'] / m['plain']:.2f}", flush=True)


def temporal_reduced_rate() -> None:
    """DecodeDeltaTemporalReduced on the band SVCE stream and on the full SVCQ stream against DecodeDeltaTemporal at full size with the
    display at the reduced size, PCIe included: `rate`'s 64 frames coded at periods 2 and 4 with a key frame every 16, the bands and their
    entropy coding made on the device."""
    import numpy as np
    import torch
    from scalable_video_codec_amd import native
    n = 65
    m = n - 1
    pw, ph = CFG.padded
    block, mv = CFG.dct_block, CFG.mv_block
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    exe = os.path.join(ROOT, "tests", "dropin", "stream_temporal_reduced_main")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        prefix = _stored_stream(d, n)
        big = torch.from_numpy(np.fromfile(prefix + ".big", np.uint8)).cuda()
        offs = torch.from_numpy(np.fromfile(prefix + ".offsets", np.uint64).astype(np.int64)).cuda()
        keys = [int(i % 16 == 0) for i in range(m)]
        key_file = os.path.join(d, "key.txt")
        with open(key_file, "w") as f:
            f.write("".join(f"{k}\n" for k in keys))

        def store(name, data, data_offs):
            p = os.path.join(d, name)
            data[:int(data_offs[-1])].cpu().numpy().tofile(p + ".big")
            data_offs.cpu().numpy().astype(np.uint64).tofile(p + ".offsets")
            return p, int(data_offs[-1]) / m / 1e6

        for period in (2, 4):
            diff, do, st = native.delta_levels_temporal_frames(big, offs, pw, ph, block, mv, period, key=keys)
            torch.cuda.synchronize()
            assert not st.any()
            diff = diff[:int(do[-1])].clone()
            dprefix, mb_full = store(f"delta{period}", diff, do)
            print(f"{m} frames, period {period}: plain stream {big.numel() / m / 1e6:.3f} MB per frame, temporal delta stream (a key frame every 16) "
                  f"{mb_full:.3f}", flush=True)
            for r in (2, 8):
                k = block // r
                dw, dh = pw // r, ph // r
                band, bo, bst = native.band_levels_frames(diff, do, pw, ph, block, mv, band=[(0, 0, k, k)] * m)
                coded, co, est = native.entropy_encode_frames(band[:int(bo[-1])].clone(), bo, pw, ph, block, mv)
                torch.cuda.synchronize()
                assert not bst.any() and not est.any()
                bprefix, mb_band = store(f"band{period}_{r}", coded, co)
                print(f"period {period}, reduce {r}: the band (0, 0, {k}, {k}) {int(bo[-1]) / m / 1e6:.3f} MB per frame, entropy-coded {mb_band:.3f}",
                      flush=True)
                gaze = os.path.join(d, f"gaze{r}.txt")
                with open(gaze, "w") as f:
                    for i in range(m):
                        f.write(f"{(60 + 29 * i) % dw} {(40 + 17 * i) % dh}\n")
                tail = [gaze, key_file, "16", "3"]
                for turn in range(3):  # alternating, every run printed: the spread is part of the result
                    for what, args in (("band SVCE", [bprefix, str(m), "0", "0", *tail, str(r), str(period), "-"]),
                                       ("full SVCQ", [dprefix, str(m), "0", "0", *tail, str(r), str(period), "-"]),
                                       ("full size, DecodeDeltaTemporal", [dprefix, str(m), str(dw), str(dh), *tail, "0", str(period), "-"])):
                        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
                        print(f"== stream_temporal_reduced_main ({what}) period {period} display {dw}x{dh} batch 16, run {turn} (exit {p.returncode})\n"
                              f"{p.stdout.strip()}\n{p.stderr.strip()}", flush=True)
                        if p.returncode != 0:
                            sys.exit(1)


if __name__ == "__main__":
    {"rate": rate, "kernels": kernels, "reduced": reduced, "reduced-rate": reduced_rate, "layers-reduced": layers_reduced,
     "layers-reduced-rate": layers_reduced_rate, "delta": delta, "delta-rate": delta_rate, "delta-reduced": delta_reduced,
     "delta-reduced-rate": delta_reduced_rate, "temporal": temporal, "temporal-reduced": temporal_reduced,
     "temporal-reduced-rate": temporal_reduced_rate}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
