"""The decoder of the reference's wire stream (svc_hip_decode_records_frames, svc::StreamDecoder::DecodeWire) measured at C3
(1920x1088 padded, 8x8 tiles, 16 frames per batch, decoder steps fg 1 / bg 640).

  python tools/decode_wire_probe.py kernels   one C3 batch of raw-coefficient records of a synthetic clip, then 5 times each: the
                                              reconstruction alone and the reconstruction + the display pass (1920x1080 u8); run
                                              under `rocprofv3 --kernel-trace --stats -- python ...`
  python tools/decode_wire_probe.py rate      a 33-frame wire stream (header + records over the padded grid) decoded by
                                              tests/dropin/wire_decode_main to 1920x1080 display frames with a moving gaze
                                              centre (PCIe included)
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scalable_video_codec_amd import configs, synth  # noqa: E402

CFG = configs.C3


def _records(n, dev):
    import torch
    from scalable_video_codec_amd import native
    pw, ph = CFG.padded
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device=dev)
    bgr = torch.stack([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)]).contiguous()
    types = torch.zeros((n, (pw // 8) * (ph // 8)), dtype=torch.int32, device=dev)
    types[:, ::7] = 1  # some foreground tiles
    return native.dct_records_frames(bgr, CFG.dct_block, types, CFG.dct_block)


def kernels() -> None:
    import torch
    from scalable_video_codec_amd import native
    dev = torch.device("cuda")
    m = 16
    pw, ph = CFG.padded
    records = _records(m, dev)
    rects = [native.gaze_rect(100 + 100 * i, 500, 64, 64, CFG.width, CFG.height, pw, ph) for i in range(m)]
    rec = torch.empty((m, ph, pw, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((m, CFG.height, CFG.width, 3), dtype=torch.uint8, device=dev)
    for _ in range(5):
        native.decode_records_frames(records, pw, ph, CFG.dct_block, 1, 640, gaze=rects, rec=rec)
    for _ in range(5):
        native.decode_records_frames(records, pw, ph, CFG.dct_block, 1, 640, gaze=rects, display=(CFG.width, CFG.height), rec=rec,
                                     out_display=disp)
    torch.cuda.synchronize()
    print(f"C3 batch of {m}: {records.shape[1] / 1e6:.2f} MB records per frame, {pw * ph * 12 / 1e6:.2f} MB f32 rec per frame, "
          f"{CFG.width * CFG.height * 3 / 1e6:.2f} MB display per frame", flush=True)


def rate() -> None:
    import torch
    from scalable_video_codec_amd import native
    n = 33
    records = _records(n - 1, torch.device("cuda")).cpu().numpy()
    header = native.wire_header(n, CFG.width, CFG.height, CFG.mv_block, CFG.levels, CFG.dct_block)
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        path = os.path.join(d, "clip.wire")
        with open(path, "wb") as f:
            f.write(header)
            records.tofile(f)
        gaze = os.path.join(d, "gaze.txt")
        with open(gaze, "w") as f:
            for i in range(n - 1):
                f.write(f"{(60 + 29 * i) % CFG.width} {(40 + 17 * i) % CFG.height}\n")
        dec = os.path.join(ROOT, "tests", "dropin", "wire_decode_main")
        for batch in (8, 16):
            r = subprocess.run([dec, "--in", path, "--gaze", gaze, "--batch", str(batch), "--out", "-"], capture_output=True, text=True,
                               timeout=300)
            print(f"== wire_decode_main batch {batch} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
            if r.returncode != 0:
                sys.exit(1)


if __name__ == "__main__":
    {"rate": rate, "kernels": kernels}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
