"""Where svc_hip_decode_delta_levels_frames writes and what its results depend on (tests/helpers/guarded.py): workspace, rec, display,
status, the last frame and its length of exactly the sizes the API asks for inside guarded allocations, the four poisons (the leftovers of a
call on another frame count and of another entry point on the same workspace among them), and other bytes beside each input, the frame
before, the key flags and the gaze included.  The builder has the form of tests/test_gpu_guard_delta.py's and runs through
tests/test_gpu_guard_streams.py's _check; tests/test_gpu_placement_decode_delta.py takes it from here."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_delta import clip_parts, key_flags
from tests.test_gpu_guard_streams import DEC, FUSED, NS, _check, _cuda, _gid, _statuses, _windows

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32


def e_decode_delta(pool, geom, n, seed):
    """clip_parts' delta stream with its frame before and key flags, _windows' gaze rectangles, a display smaller than the frame."""
    w, h, tile, mv = geom
    dw, dh = max(1, w - 5), max(1, h - 3)
    prev, stream, offs, diff, diff_offs = clip_parts(geom, n, seed)
    inputs = {"stream": _cuda(diff), "offsets": _cuda(diff_offs), "prev": _cuda(prev), "key": _cuda(np.asarray(key_flags(n), np.int32)),
              "gaze": _windows(n, w, h)}
    ws = pool.buf("workspace", nat.decode_delta_levels_workspace_bytes(n, w, h, tile, mv), U8)
    rec = pool.buf("rec", (n, h, w, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)
    status = pool.buf("status", n, I32)
    last = pool.buf("last", nat.levels_max_bytes(1, w, h, tile, mv), U8)
    last_bytes = pool.buf("last bytes", 1, I64)

    def call(i):
        before = last.clone()
        nat._check(nat.load().svc_hip_decode_delta_levels_frames(
            i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, i["prev"].data_ptr(), i["prev"].numel(), i["key"].data_ptr(),
            w, h, *tile, *mv, *DEC, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(), disp.data_ptr(), dw, dh, last.data_ptr(),
            last.numel(), last_bytes.data_ptr(), status.data_ptr(), nat._stream()))
        _statuses(status, n, None)
        used = int(last_bytes[0])
        assert 64 <= used <= last.numel()
        changed = int((last[used:] != before[used:]).sum())
        assert changed == 0, f"decode_delta_levels: {changed} bytes past the last frame's length were written"
        return {"rec": rec, "display": disp, "status": status, "last": last[:used], "last bytes": last_bytes}
    return inputs, call


ENTRIES = {"decode_delta_levels": (e_decode_delta, FUSED)}
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms]


def test_every_pair_is_sized(native):
    """No case below is a refusal in disguise."""
    for _, geom in PAIRS:
        w, h, tile, mv = geom
        for n in NS:
            assert nat.decode_delta_levels_workspace_bytes(n, w, h, tile, mv) > 0 and nat.levels_max_bytes(1, w, h, tile, mv) > 0, (geom, n)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    findings = []
    for n in NS:
        findings += _check(entry, ENTRIES[entry][0], geom, n, max(1, n - 2))
    assert not findings, "\n".join(findings)
