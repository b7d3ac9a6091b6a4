"""The decoder of the compact stream (svc_hip_decode_levels_frames) measured at C3 (1920x1088 padded, 8x8 tiles, MV 16, 16 frames).

  python tools/decode_probe.py kernels   one C3 batch through the resident encoder and the pack, then 5 times each: the chain
                                         unpack + svc_hip_decode_frames, the fused reconstruction, the fused reconstruction + the
                                         display pass (1920x1080 u8); run under `rocprofv3 --kernel-trace --stats -- python ...`
  python tools/decode_probe.py rate      tests/dropin/stream_levels_main writes a 65-frame clip's stream, tests/dropin/stream_decode_main
                                         decodes it to 1920x1080 display frames with a moving gaze centre (PCIe included)
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


def rate() -> None:
    n = 65
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device="cpu")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
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


if __name__ == "__main__":
    {"rate": rate, "kernels": kernels}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
