"""The compact quantised-coefficient stream (csrc/levels.hip) measured at C3 (1080p, 8x8 tiles, steps 1 / 640).

  python tools/levels_probe.py rate      tests/dropin/stream_main beside tests/dropin/stream_levels_main, both with the output
                                         prefix "-", on the same 65-frame 1080p synthetic clip (made on the CPU: this process never
                                         opens the GPU, so the children's copy engines are not shared with it)
  python tools/levels_probe.py kernels   one C3 batch of 16 encoded frames through the resident encoder, then pack, unpack and
                                         drain 5 times each; run under `rocprofv3 --kernel-trace --stats -- python ...`
  python tools/levels_probe.py budget    one C3 batch of 16 encoded frames as RAW planes, then the fixed pack (steps 1 / 640) and the
                                         budgeted pack (a 32-entry ladder, 1.1 MB per frame) 5 times each; run under rocprofv3 as above
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from scalable_video_codec_amd import configs, synth  # noqa: E402

CFG = configs.C3


def rate() -> None:
    n = 65
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device="cpu")
    tmp = "/dev/shm" if os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        raw = os.path.join(d, "clip.raw")
        with open(raw, "wb") as f:
            for t in range(n):
                clip.frame_bgr(t).numpy().tofile(f)
        for name in ("stream_main", "stream_levels_main"):
            exe = os.path.join(ROOT, "tests", "dropin", name)
            r = subprocess.run([exe, raw, str(CFG.width), str(CFG.height), str(n), str(CFG.levels), str(CFG.dct_block), "0", "16",
                                str(CFG.seed), "-"], capture_output=True, text=True, timeout=300)
            print(f"== {name} (exit {r.returncode})\n{r.stdout.strip()}\n{r.stderr.strip()}", flush=True)
            if r.returncode != 0:
                sys.exit(1)


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
    cap = native.levels_max_bytes(n - 1, pw, ph, CFG.dct_block, CFG.mv_block)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(native.pack_levels_workspace_bytes(n - 1, pw, ph, CFG.dct_block), dtype=torch.uint8, device=dev)
    back = torch.empty_like(planes)
    back_types = torch.empty_like(types)
    pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
    for _ in range(5):
        native.pack_levels_frames(planes, types, CFG.dct_block, CFG.mv_block, CFG.fg_step, CFG.bg_step, out=out, offsets=offs, workspace=ws)
    for _ in range(5):
        _, _, status = native.unpack_levels_frames(out, offs, pw, ph, CFG.dct_block, CFG.mv_block, planes=back, block_types=back_types,
                                                   workspace=ws)
    for _ in range(5):
        native.levels_drain(out, offs, pw, ph, CFG.dct_block, CFG.mv_block, pinned)
    torch.cuda.synchronize()
    total = int(offs[-1].item())
    assert status.cpu().tolist() == [0] * (n - 1) and torch.equal(back, planes)
    plane_bytes = planes.numel() * 4
    print(f"C3 batch of {n - 1}: {total} B compact ({total / (n - 1) / 1e6:.3f} MB per frame) for {plane_bytes / (n - 1) / 1e6:.2f} MB "
          f"of planes per frame ({plane_bytes / total:.1f}x)", flush=True)


def budget() -> None:
    import torch
    from scalable_video_codec_amd import levels, native, pipeline
    dev = torch.device("cuda")
    n = 17
    clip = synth.SynthClip(CFG.width, CFG.height, n, CFG.seed, device=dev)
    pw, ph = CFG.padded
    enc = pipeline.ClipEncoder(CFG, n, dev, quantise=False)
    enc.load_frames([synth.pad_frame(clip.frame_bgr(t), pw, ph) for t in range(n)])
    enc.step()
    planes, types = enc.coeffs, enc.types
    ladder = levels.step_ladder(1, 256, 4, 640, 10, 24)
    assert len(ladder) == 32
    cap = native.levels_max_bytes(n - 1, pw, ph, CFG.dct_block, CFG.mv_block)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    offs = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(native.pack_levels_budget_workspace_bytes(n - 1, pw, ph, CFG.dct_block, len(ladder)), dtype=torch.uint8, device=dev)
    choice = torch.empty(n - 1, dtype=torch.int32, device=dev)
    bud = native.budget_tensor(1_100_000, n - 1, dev)
    for _ in range(5):
        native.pack_levels_frames(planes, types, CFG.dct_block, CFG.mv_block, CFG.fg_step, CFG.bg_step, out=out, offsets=offs, workspace=ws)
    torch.cuda.synchronize()
    fixed_total = int(offs[-1].item())
    for _ in range(5):
        native.pack_levels_budget_frames(planes, types, CFG.dct_block, CFG.mv_block, ladder, bud, out=out, offsets=offs, workspace=ws,
                                         choice=choice)
    torch.cuda.synchronize()
    ch = choice.cpu().numpy().view(np.uint32)
    sizes = np.diff(offs.cpu().numpy())
    print(f"C3 batch of {n - 1} raw frames: fixed pack (1 / 640) {fixed_total / (n - 1) / 1e6:.3f} MB per frame; budgeted pack, "
          f"32 entries, budget 1.1 MB: choices {[int(c & 0x7FFFFFFF) for c in ch]}, over budget {int((ch >> 31).sum())}, "
          f"{sizes.min() / 1e6:.3f} .. {sizes.max() / 1e6:.3f} MB per frame", flush=True)


if __name__ == "__main__":
    {"rate": rate, "kernels": kernels, "budget": budget}[sys.argv[1] if len(sys.argv) > 1 else "rate"]()
