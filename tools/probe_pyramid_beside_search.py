#!/usr/bin/env python3
"""Probe: what can running the pyramid levels (svc_hip_pyramid_levels_frames: vector-memory issue bound, VALU mostly idle) BESIDE the motion
search (svc_hip_hbma_pairs: VALU-paced) be worth, whatever the driver does around them?  On independent buffers of C3's size (299 pairs): each
alone, back to back on one stream, and on two streams -- each both on an idle GPU and right behind a C3-sized front-of-step transform
launch (svc_hip_dct_quant_luma_frames), whose write-back drains into whatever follows it.  Medians of `reps` repetitions, wall time by
HIP events around the whole group; the "behind the transform" rows also give the time beyond the transform alone.
usage: tools/probe_pyramid_beside_search.py [pairs = 299] [reps = 11]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from scalable_video_codec_amd import configs, native, synth  # noqa: E402

cfg = configs.C3
lib = native.load()
dev = torch.device("cuda")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 299
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
pw, ph = cfg.padded
src = synth.SynthClip(cfg.width, cfg.height, n + 1, cfg.seed, device=dev)
bgr = torch.stack([synth.pad_frame(src.frame_bgr(t), pw, ph) for t in range(n + 1)]).contiguous()
planes = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
stride = native.pyramid_stride(pw, ph, cfg.levels)
pyr_search, stride2 = native.luma_pyramid_frames(bgr, cfg.levels)  # n + 1 whole pyramids: what the search reads
assert stride2 == stride
pyr_front = torch.empty(n * stride, dtype=torch.uint8, device=dev)   # what the transform writes its luma planes into
pyr_levels = pyr_search[stride:].clone()                             # n pyramids whose levels >= 1 the pyramid pass rewrites
blocks = (pw // cfg.mv_block) * (ph // cfg.mv_block)
mv = torch.empty((n, blocks, 2), dtype=torch.float32, device=dev)
mad = torch.empty((n, blocks), dtype=torch.float32, device=dev)
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
vp = C.c_void_p


def transform(st):
    native._check(lib.svc_hip_dct_quant_luma_frames(bgr[1:].data_ptr(), ph * pw * 3, n, pw, ph, cfg.dct_block, cfg.bg_step, planes.data_ptr(),
                                                    pyr_front.data_ptr(), stride, vp(st.cuda_stream)))


def levels(st):
    native._check(lib.svc_hip_pyramid_levels_frames(pyr_levels.data_ptr(), stride, n, pw, ph, cfg.levels, vp(st.cuda_stream)))


def search(st):
    native._check(lib.svc_hip_hbma_pairs(pyr_search.data_ptr(), pyr_search.data_ptr() + stride, stride, n, cfg.levels, pw, ph, cfg.search_range,
                                         cfg.mv_block, cfg.mv_block, mv.data_ptr(), mad.data_ptr(), 0, vp(st.cuda_stream)))


def beside(behind):
    """levels on s2, search on s1; behind a transform on s1 both start at its end (an event, as the driver forks)."""
    if behind:
        transform(s1)
        e = torch.cuda.Event()
        e.record(s1)
        s2.wait_event(e)
    levels(s2)
    search(s1)


def timed(fn):
    out = []
    for _ in range(reps + 1):  # (the first repetition warms up)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        s1.wait_event(e0)
        s2.wait_event(e0)
        fn()
        ea, eb = torch.cuda.Event(), torch.cuda.Event()
        ea.record(s1)
        eb.record(s2)
        torch.cuda.current_stream().wait_event(ea)
        torch.cuda.current_stream().wait_event(eb)
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    out = sorted(out[1:])
    return out[len(out) // 2], out[0], out[-1]


print(f"{cfg.name}: {n} pairs, {pw} x {ph}, {cfg.levels} levels, search kernel {native.hbma_kernel_name(cfg.levels, pw, ph, cfg.search_range, cfg.mv_block, cfg.mv_block)}; "
      f"medians of {reps}", flush=True)
t_alone = timed(lambda: transform(s1))[0]
rows = (("transform alone", lambda: transform(s1), False),
        ("levels alone", lambda: levels(s1), False),
        ("search alone", lambda: search(s1), False),
        ("levels | search, one stream", lambda: (levels(s1), search(s1)), False),
        ("search | levels, one stream", lambda: (search(s1), levels(s1)), False),
        ("levels beside search, two streams", lambda: beside(False), False),
        ("transform | levels", lambda: (transform(s1), levels(s1)), True),
        ("transform | search", lambda: (transform(s1), search(s1)), True),
        ("transform | levels | search, one stream", lambda: (transform(s1), levels(s1), search(s1)), True),
        ("transform | search | levels, one stream", lambda: (transform(s1), search(s1), levels(s1)), True),
        ("transform | levels beside search", lambda: beside(True), True))
for name, fn, behind in rows:
    med, lo, hi = timed(fn)
    extra = f"  beyond the transform alone {med - t_alone:.4f} ms" if behind else ""
    print(f"{name:42s} median {med:.4f} ms  min {lo:.4f}  max {hi:.4f}{extra}", flush=True)
