"""The entropy-coded compact stream (csrc/entropy.hip) measured at C3 (1080p, 8x8 tiles).

  python tools/entropy_probe.py kernels FG BG   one C3 batch of 16 encoded frames through the resident encoder with steps FG / BG and
                                                the pack, then the SVCE encode, decode and drain 5 times each; run under
                                                `rocprofv3 --kernel-trace --stats -- python ...`.  Prints the sizes and checks the
                                                round trip.
  python tools/entropy_probe.py decode-fused FG BG   the same batch's SVCE frames to display frames, 5 times by the two calls
                                                (svc_hip_entropy_decode_frames, then svc_hip_decode_levels_frames) and 5 times by
                                                svc_hip_decode_entropy_frames, in one process; run under `rocprofv3 --kernel-trace
                                                --stats -- python ...`.  Checks that both give the same reconstruction and display.
  python tools/entropy_probe.py rate            HostStreamEncoder(compact=True) beside HostStreamEncoder(compact=True, entropy=True)
                                                on the same 65-frame clip: frames per second and bytes per frame
  python tools/entropy_probe.py cpp             the C++ drivers on a 65-frame C3 clip made on the CPU (this process never opens the
                                                GPU): stream_levels_main and stream_entropy_main encoding ("-": rates), then
                                                stream_decode_main on the SVCQ stream and stream_entropy_main's decode of its SVCE stream
"""
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from scalable_video_codec_amd import configs, synth  # noqa: E402


def kernels(fg: int, bg: int) -> None:
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = dataclasses.replace(configs.C3, fg_step=fg, bg_step=bg)
    dev = torch.device("cuda")
    n = 17
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device=dev)
    pw, ph = cfg.padded
    enc = pipeline.ClipEncoder(cfg, n, dev)
    enc.load_frames([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)])
    enc.step()
    b, mb = cfg.dct_block, cfg.mv_block
    svcq, offs = native.pack_levels_frames(enc.coeffs[:n - 1], enc.types[:n - 1], b, mb, fg, bg)
    ecap = native.entropy_max_bytes(n - 1, pw, ph, b, mb)
    e = torch.empty(ecap, dtype=torch.uint8, device=dev)
    eo = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(native.entropy_workspace_bytes(n - 1, pw, ph, b, mb), dtype=torch.uint8, device=dev)
    back = torch.empty_like(svcq)
    bo = torch.empty_like(offs)
    pinned = torch.empty(ecap, dtype=torch.uint8).pin_memory()
    for _ in range(5):
        _, _, st = native.entropy_encode_frames(svcq, offs, pw, ph, b, mb, out=e, out_offsets=eo, workspace=ws)
    for _ in range(5):
        _, _, ds = native.entropy_decode_frames(e, eo, pw, ph, b, mb, out=back, out_offsets=bo, workspace=ws)
    for _ in range(5):
        native.entropy_drain(e, eo, pw, ph, b, mb, pinned)
    torch.cuda.synchronize()
    q, c = int(offs[-1]), int(eo[-1])
    ok = st.cpu().tolist() == [0] * (n - 1) and ds.cpu().tolist() == [0] * (n - 1) and torch.equal(bo, offs) and \
        torch.equal(back[:q], svcq[:q]) and torch.equal(pinned[:c], e[:c].cpu())
    print(f"C3 batch of {n - 1}, steps ({fg}, {bg}): SVCQ {q / (n - 1) / 1e6:.4f} MB per frame, SVCE {c / (n - 1) / 1e6:.4f} MB per "
          f"frame, ratio {q / c:.2f}x; round trip {'ok' if ok else 'FAILED'}", flush=True)
    if not ok:
        sys.exit(1)


def decode_fused(fg: int, bg: int) -> None:
    import torch
    from scalable_video_codec_amd import native, pipeline
    cfg = dataclasses.replace(configs.C3, fg_step=fg, bg_step=bg)
    dev = torch.device("cuda")
    n = 17
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device=dev)
    pw, ph = cfg.padded
    enc = pipeline.ClipEncoder(cfg, n, dev)
    enc.load_frames([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)])
    enc.step()
    b, mb = cfg.dct_block, cfg.mv_block
    svcq, offs = native.pack_levels_frames(enc.coeffs[:n - 1], enc.types[:n - 1], b, mb, fg, bg)
    e, eo, st = native.entropy_encode_frames(svcq, offs, pw, ph, b, mb)
    display = (cfg.width, cfg.height)
    gaze = [native.gaze_rect(100 + 110 * i, 60 + 60 * i, 64, 64, cfg.width, cfg.height, pw, ph) for i in range(n - 1)]
    gaze = torch.tensor(gaze, dtype=torch.int32, device=dev)
    back, bo = torch.empty_like(svcq), torch.empty_like(offs)
    ews = torch.empty(native.entropy_workspace_bytes(n - 1, pw, ph, b, mb), dtype=torch.uint8, device=dev)
    lws = torch.empty(native.decode_levels_workspace_bytes(n - 1, pw, ph, b), dtype=torch.uint8, device=dev)
    fws = torch.empty(native.decode_entropy_workspace_bytes(n - 1, pw, ph, b, mb), dtype=torch.uint8, device=dev)
    rec = [torch.empty((n - 1, ph, pw, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    disp = [torch.empty((n - 1, display[1], display[0], 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(5):
        _, _, es = native.entropy_decode_frames(e, eo, pw, ph, b, mb, out=back, out_offsets=bo, workspace=ews)
        _, _, ls = native.decode_levels_frames(back, bo, pw, ph, b, mb, 1, 640, gaze=gaze, display=display, rec=rec[0],
                                               out_display=disp[0], workspace=lws)
    torch.cuda.synchronize()
    for _ in range(5):
        _, _, fs = native.decode_entropy_frames(e, eo, pw, ph, b, mb, 1, 640, gaze=gaze, display=display, rec=rec[1],
                                                out_display=disp[1], workspace=fws)
    torch.cuda.synchronize()
    zeros = [0] * (n - 1)
    ok = st.cpu().tolist() == zeros and es.cpu().tolist() == zeros and ls.cpu().tolist() == zeros and fs.cpu().tolist() == zeros and \
        torch.equal(rec[0], rec[1]) and torch.equal(disp[0], disp[1]) and bool(disp[1].any())
    print(f"C3 batch of {n - 1}, steps ({fg}, {bg}): SVCE {int(eo[-1]) / (n - 1) / 1e6:.4f} MB per frame; the two calls and the fused "
          f"call {'agree' if ok else 'DISAGREE'}", flush=True)
    if not ok:
        sys.exit(1)


def rate() -> None:
    import torch
    from scalable_video_codec_amd import stream
    cfg = configs.C3
    n = 65
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cpu")
    host = np.stack([clip.frame_bgr(t).numpy() for t in range(n)])
    dev = torch.device("cuda")
    for entropy in (False, True, False, True):
        enc = stream.HostStreamEncoder(cfg, batch=16, device=dev, compact=True, entropy=entropy)
        for _ in enc.encode(host[:18]):  # warm-up
            pass
        t0 = time.perf_counter()
        total = frames = 0
        for out in enc.encode(host):
            total += out["compact"].size
            frames += out["mv"].shape[0]
        dt = time.perf_counter() - t0
        print(f"HostStreamEncoder compact{' + entropy' if entropy else ''}: {frames / dt:.1f} frames/s, "
              f"{total / frames / 1e6:.4f} MB per frame to the host", flush=True)


def cpp() -> None:
    import subprocess
    import tempfile
    cfg = configs.C3
    n = 65
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cpu")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    dropin = os.path.join(ROOT, "tests", "dropin")
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(n):
                clip.frame_bgr(t).numpy().tofile(f)
        common = [raw, str(cfg.width), str(cfg.height), str(n), str(cfg.levels), str(cfg.dct_block)]
        runs = [("stream_levels_main", [*common, "0", "16", str(cfg.seed), "-"]),
                ("stream_levels_main", [*common, "0", "16", str(cfg.seed), os.path.join(d, "q")]),
                ("stream_decode_main", [os.path.join(d, "q"), str(n - 1), "0", "0", "-", "16", "-"]),
                ("stream_entropy_main", [*common, "16", str(cfg.seed), "-", "-"])]
        for name, args in runs:
            r = subprocess.run([os.path.join(dropin, name), *args], capture_output=True, text=True, timeout=300)
            print(f"== {name} {' '.join(args[-2:])} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
            if r.returncode != 0:
                sys.exit(1)


if __name__ == "__main__":
    {"kernels": lambda: kernels(int(sys.argv[2]), int(sys.argv[3])), "decode-fused": lambda: decode_fused(int(sys.argv[2]), int(sys.argv[3])),
     "rate": rate, "cpp": cpp}[sys.argv[1]]()
