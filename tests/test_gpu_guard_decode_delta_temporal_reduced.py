"""Where svc_hip_decode_delta_levels_temporal_reduced_frames (include/svc_hip_temporal_decode.h) writes and what its results depend on
(tests/helpers/guarded.py), periods 2 and 4: workspace, rec, display, status, the last frame and its length of exactly the sizes the API
asks for inside guarded allocations; zeros, 0xFF, random bytes and the leftovers of three other calls on the same buffers -- this entry
point with another frame count, another reduce and the other period, svc_hip_decode_delta_levels_reduced_frames and
svc_hip_decode_delta_levels_temporal_frames on the same workspace, status and last frame; and other bytes beside each input, the frame
before, the key flags and the gaze included.  The builder has the form of tests/test_gpu_guard_decode_delta_reduced.py's with
tests/test_gpu_guard_delta_temporal.py's clips; tests/test_gpu_placement_decode_delta_temporal_reduced.py and
tests/test_gpu_stream_order_decode_delta_temporal_reduced.py take it from here."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_decode_delta_reduced import e_decode_delta_reduced
from tests.test_gpu_guard_delta import key_flags
from tests.test_gpu_guard_delta_temporal import ENTRIES as FULL_SIZE
from tests.test_gpu_guard_delta_temporal import clip_parts
from tests.test_gpu_guard_streams import DEC, FUSED, NS, Pool, _cuda, _gid, _statuses, _windows

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
REDUCES = (2, 4, 8)
PERIODS = (2, 4)
ENTRY = "decode_delta_levels_temporal_reduced"


def e_decode_delta_temporal_reduced(pool, geom, n, seed, reduce=2, period=2):
    """clip_parts' temporal delta stream with its frame before and key flags, _windows' gaze rectangles, a display smaller than the reduced
    picture."""
    w, h, tile, mv = geom
    rw, rh = w // reduce, h // reduce
    dw, dh = max(1, rw - 5), max(1, rh - 3)
    prev, stream, offs, diff, diff_offs = clip_parts(geom, n, period, seed)
    inputs = {"stream": _cuda(diff), "offsets": _cuda(diff_offs), "prev": _cuda(prev), "key": _cuda(np.asarray(key_flags(n), np.int32)),
              "gaze": _windows(n, w, h)}
    ws = pool.buf("workspace", nat.decode_delta_levels_temporal_reduced_workspace_bytes(n, w, h, tile, mv, period), U8)
    rec = pool.buf("rec", (n, rh, rw, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)
    status = pool.buf("status", n, I32)
    last = pool.buf("last", nat.levels_max_bytes(1, w, h, tile, mv), U8)
    last_bytes = pool.buf("last bytes", 1, I64)

    def call(i):
        before = last.clone()
        nat._check(nat.load().svc_hip_decode_delta_levels_temporal_reduced_frames(
            i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, i["prev"].data_ptr(), i["prev"].numel(), i["key"].data_ptr(),
            w, h, *tile, *mv, *DEC, reduce, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(), disp.data_ptr(), dw, dh,
            last.data_ptr(), last.numel(), last_bytes.data_ptr(), status.data_ptr(), nat._stream(), period))
        _statuses(status, n, None)
        used = int(last_bytes[0])
        assert 64 <= used <= last.numel()
        changed = int((last[used:] != before[used:]).sum())
        assert changed == 0, f"{ENTRY}: {changed} bytes past the last frame's length were written"
        return {"rec": rec, "display": disp, "status": status, "last": last[:used], "last bytes": last_bytes}
    return inputs, call


def _builder(reduce, period):
    def build(pool, geom, n, seed):
        return e_decode_delta_temporal_reduced(pool, geom, n, seed, reduce, period)
    return build


ENTRIES = {f"{ENTRY}_r{r}_p{p}": (_builder(r, p), FUSED) for r in REDUCES for p in PERIODS}
TRIPLES = [(g, r, p) for g in FUSED for r in REDUCES for p in PERIODS]


def reduce_period_of(entry):
    r, p = entry[len(ENTRY) + 1:].split("_")
    return int(r[1:]), int(p[1:])


def test_every_triple_is_sized(native):
    """No case below is a refusal in disguise."""
    for geom, _, period in TRIPLES:
        w, h, tile, mv = geom
        for n in NS:
            assert nat.decode_delta_levels_temporal_reduced_workspace_bytes(n, w, h, tile, mv, period) > 0, (geom, n)
            assert nat.levels_max_bytes(1, w, h, tile, mv) > 0, (geom, n)


def _findings(geom, n, reduce, period):
    pool = Pool()
    inputs, call = e_decode_delta_temporal_reduced(pool, geom, n, 0, reduce, period)
    dirty_n, other_reduce, other_period = max(1, n - 2), REDUCES[(REDUCES.index(reduce) + 1) % 3], 6 - period
    smaller = other_reduce > reduce  # a picture that fits the buffers of this one: the same views; else buffers of its own
    shared, plain = Pool(), Pool()
    for k, g in pool.written.items():
        if smaller or k not in ("rec", "display"):
            for p in (shared, plain):
                p.written[k] = g
                p.borrowed.add(k)
    d_inputs, d_call = e_decode_delta_temporal_reduced(shared, geom, dirty_n, 1, other_reduce, other_period)
    r_inputs, r_call = e_decode_delta_reduced(plain, geom, dirty_n, 3, other_reduce)  # the period-1 call
    full = Pool()
    for k in ("workspace", "status", "last", "last bytes"):  # the full-size call's pictures do not fit: they are its own
        full.written[k] = pool.written[k]
        full.borrowed.add(k)
    f_inputs, f_call = FULL_SIZE[f"decode_delta_levels_temporal{period}"][0](full, geom, dirty_n, 2)

    def dirty():
        d_call(d_inputs)
        r_call(r_inputs)
        f_call(f_inputs)
    name = f"{ENTRY} {_gid(geom)} n={n} reduce={reduce} period={period}"
    unsurrounded = {k: gd.surround(v, 0) for k, v in inputs.items()}
    findings = gd.check_writes(name, pool.written, lambda: call(unsurrounded), dirty=dirty, seed=n)
    findings += gd.check_reads(name, inputs, call, pool.written)
    return findings


@pytest.mark.parametrize("geom,reduce,period", TRIPLES, ids=[f"{_gid(g)}-r{r}-p{p}" for g, r, p in TRIPLES])
def test_poisoned_buffers_and_neighbours(native, geom, reduce, period):
    findings = []
    for n in NS:
        findings += _findings(geom, n, reduce, period)
    assert not findings, "\n".join(findings)
