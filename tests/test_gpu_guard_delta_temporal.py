"""Where the three temporal calls (include/svc_hip.h, "Temporal layers") write and what their results depend on
(tests/helpers/guarded.py): workspace and every output of exactly the sizes the API asks for inside guarded allocations, the four poisons
(the leftovers of a call on another frame count and of another entry point on the same workspace among them), and other bytes beside each
input, the frame before, the key flags and the gaze included.  The builders have the form of tests/test_gpu_guard_delta.py's and
tests/test_gpu_guard_decode_delta.py's, once per period, and run through tests/test_gpu_guard_streams.py's _check;
tests/test_gpu_placement_delta_temporal.py takes them from here."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_gpu_guard_delta import key_flags
from tests.test_gpu_guard_streams import DEC, ENC, FUSED, NS, STREAM, _check, _cuda, _gid, _past, _statuses, _stream_out, _svcq, _windows

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
PERIODS = (2, 4)


@functools.lru_cache(maxsize=None)
def clip_parts(geom, n, period, seed=0):
    """tests/test_gpu_guard_delta.py's clip_parts with the delta stream of this period -> (the frame before, the n frames, their offsets,
    their delta stream by the numpy statement, its offsets), as arrays."""
    q, qo = _svcq(geom, n + 1, ENC, seed)
    f = frames_of(q.tobytes(), qo)
    stream, offs = entropy._join(f[1:])
    diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, key_flags(n), prev=f[0])
    as_array = lambda b, o: (np.frombuffer(b, np.uint8).copy(), np.asarray(o).astype(np.int64))
    return (np.frombuffer(f[0], np.uint8).copy(),) + as_array(stream, offs) + as_array(diff, diff_offs)


def _stream_builder(undo, period):
    def build(pool, geom, n, seed):
        w, h, tile, mv = geom
        prev, stream, offs, diff, diff_offs = clip_parts(geom, n, period, seed)
        inputs = {"stream": _cuda(diff if undo else stream), "offsets": _cuda(diff_offs if undo else offs), "prev": _cuda(prev),
                  "key": _cuda(np.asarray(key_flags(n), np.int32))}
        query = nat.undelta_levels_temporal_workspace_bytes if undo else nat.delta_levels_temporal_workspace_bytes
        fn = nat.undelta_levels_temporal_frames if undo else nat.delta_levels_temporal_frames
        ws = pool.buf("workspace", query(n, w, h, tile, mv, period), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        out_offs = pool.buf("offsets", n + 1, I64)
        status = pool.buf("status", n, I32)

        def call(i):
            before = out.clone()
            fn(i["stream"], i["offsets"], w, h, tile, mv, period, prev=i["prev"], key=i["key"], out=out, out_offsets=out_offs, workspace=ws,
               status=status)
            _past(fn.__name__, (out, out_offs, before))
            _statuses(status, n, None)
            return {"stream": _stream_out(out, out_offs), "offsets": out_offs, "status": status}
        return inputs, call
    return build


def _decode_builder(period):
    def build(pool, geom, n, seed):
        """The delta stream with its frame before and key flags, _windows' gaze rectangles, a display smaller than the frame."""
        w, h, tile, mv = geom
        dw, dh = max(1, w - 5), max(1, h - 3)
        prev, stream, offs, diff, diff_offs = clip_parts(geom, n, period, seed)
        inputs = {"stream": _cuda(diff), "offsets": _cuda(diff_offs), "prev": _cuda(prev), "key": _cuda(np.asarray(key_flags(n), np.int32)),
                  "gaze": _windows(n, w, h)}
        ws = pool.buf("workspace", nat.decode_delta_levels_temporal_workspace_bytes(n, w, h, tile, mv, period), U8)
        rec = pool.buf("rec", (n, h, w, 3), F32)
        disp = pool.buf("display", (n, dh, dw, 3), U8)
        status = pool.buf("status", n, I32)
        last = pool.buf("last", nat.levels_max_bytes(1, w, h, tile, mv), U8)
        last_bytes = pool.buf("last bytes", 1, I64)

        def call(i):
            before = last.clone()
            nat._check(nat.load().svc_hip_decode_delta_levels_temporal_frames(
                i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, i["prev"].data_ptr(), i["prev"].numel(),
                i["key"].data_ptr(), w, h, *tile, *mv, *DEC, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(), disp.data_ptr(),
                dw, dh, last.data_ptr(), last.numel(), last_bytes.data_ptr(), status.data_ptr(), nat._stream(), period))
            _statuses(status, n, None)
            used = int(last_bytes[0])
            assert 64 <= used <= last.numel()
            changed = int((last[used:] != before[used:]).sum())
            assert changed == 0, f"decode_delta_levels_temporal: {changed} bytes past the last frame's length were written"
            return {"rec": rec, "display": disp, "status": status, "last": last[:used], "last bytes": last_bytes}
        return inputs, call
    return build


ENTRIES = {}
for _p in PERIODS:
    ENTRIES[f"delta_levels_temporal{_p}"] = (_stream_builder(False, _p), STREAM)
    ENTRIES[f"undelta_levels_temporal{_p}"] = (_stream_builder(True, _p), STREAM)
    ENTRIES[f"decode_delta_levels_temporal{_p}"] = (_decode_builder(_p), FUSED)
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms]


def period_of(entry):
    return int(entry[-1])


def test_every_pair_is_sized(native):
    """No case below is a refusal in disguise."""
    for entry, geom in PAIRS:
        w, h, tile, mv = geom
        query = getattr(nat, entry[:-1] + "_workspace_bytes")
        for n in NS:
            assert query(n, w, h, tile, mv, period_of(entry)) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0, (entry, geom, n)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    findings = []
    for n in NS:
        findings += _check(entry, ENTRIES[entry][0], geom, n, max(1, n - 2))
    assert not findings, "\n".join(findings)
