"""Where svc_hip_decode_delta_levels_reduced_frames writes and what its results depend on (tests/helpers/guarded.py): workspace, rec,
display, status, the last frame and its length of exactly the sizes the API asks for inside guarded allocations; zeros, 0xFF, random bytes
and the leftovers of three other calls on the same buffers -- this entry point with another frame count and another reduce, and
svc_hip_decode_delta_levels_frames on the same workspace, status and last frame; and other bytes beside each input, the frame before, the
key flags and the gaze included.  The builder has the form of tests/test_gpu_guard_decode_delta.py's;
tests/test_gpu_placement_decode_delta_reduced.py takes it from here."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_decode_delta import e_decode_delta
from tests.test_gpu_guard_delta import clip_parts, key_flags
from tests.test_gpu_guard_streams import DEC, FUSED, NS, Pool, _cuda, _gid, _statuses, _windows

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
REDUCES = (2, 4, 8)
ENTRY = "decode_delta_levels_reduced"


def e_decode_delta_reduced(pool, geom, n, seed, reduce=2):
    """clip_parts' delta stream with its frame before and key flags, _windows' gaze rectangles, a display smaller than the reduced picture."""
    w, h, tile, mv = geom
    rw, rh = w // reduce, h // reduce
    dw, dh = max(1, rw - 5), max(1, rh - 3)
    prev, stream, offs, diff, diff_offs = clip_parts(geom, n, seed)
    inputs = {"stream": _cuda(diff), "offsets": _cuda(diff_offs), "prev": _cuda(prev), "key": _cuda(np.asarray(key_flags(n), np.int32)),
              "gaze": _windows(n, w, h)}
    ws = pool.buf("workspace", nat.decode_delta_levels_reduced_workspace_bytes(n, w, h, tile, mv), U8)
    rec = pool.buf("rec", (n, rh, rw, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)
    status = pool.buf("status", n, I32)
    last = pool.buf("last", nat.levels_max_bytes(1, w, h, tile, mv), U8)
    last_bytes = pool.buf("last bytes", 1, I64)

    def call(i):
        before = last.clone()
        nat._check(nat.load().svc_hip_decode_delta_levels_reduced_frames(
            i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, i["prev"].data_ptr(), i["prev"].numel(), i["key"].data_ptr(),
            w, h, *tile, *mv, *DEC, reduce, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(), disp.data_ptr(), dw, dh,
            last.data_ptr(), last.numel(), last_bytes.data_ptr(), status.data_ptr(), nat._stream()))
        _statuses(status, n, None)
        used = int(last_bytes[0])
        assert 64 <= used <= last.numel()
        changed = int((last[used:] != before[used:]).sum())
        assert changed == 0, f"{ENTRY}: {changed} bytes past the last frame's length were written"
        return {"rec": rec, "display": disp, "status": status, "last": last[:used], "last bytes": last_bytes}
    return inputs, call


def _builder(reduce):
    def build(pool, geom, n, seed):
        return e_decode_delta_reduced(pool, geom, n, seed, reduce)
    return build


ENTRIES = {f"{ENTRY}_r{r}": (_builder(r), FUSED) for r in REDUCES}
PAIRS = [(g, r) for g in FUSED for r in REDUCES]


def test_every_pair_is_sized(native):
    """No case below is a refusal in disguise."""
    for geom, _ in PAIRS:
        w, h, tile, mv = geom
        for n in NS:
            assert nat.decode_delta_levels_reduced_workspace_bytes(n, w, h, tile, mv) > 0 and nat.levels_max_bytes(1, w, h, tile, mv) > 0, (geom, n)


def _findings(geom, n, reduce):
    pool = Pool()
    inputs, call = e_decode_delta_reduced(pool, geom, n, 0, reduce)
    dirty_n, other_reduce = max(1, n - 2), REDUCES[(REDUCES.index(reduce) + 1) % 3]
    smaller = other_reduce > reduce  # a picture that fits the buffers of this one: the same views; else buffers of its own
    shared = Pool()
    for k, g in pool.written.items():
        if smaller or k not in ("rec", "display"):
            shared.written[k] = g
            shared.borrowed.add(k)
    d_inputs, d_call = e_decode_delta_reduced(shared, geom, dirty_n, 1, other_reduce)  # another frame count, another reduce
    full = Pool()
    for k in ("workspace", "status", "last", "last bytes"):  # the full-size call's pictures do not fit: they are its own
        full.written[k] = pool.written[k]
        full.borrowed.add(k)
    f_inputs, f_call = e_decode_delta(full, geom, dirty_n, 2)

    def dirty():
        d_call(d_inputs)
        f_call(f_inputs)
    name = f"{ENTRY} {_gid(geom)} n={n} reduce={reduce}"
    plain = {k: gd.surround(v, 0) for k, v in inputs.items()}
    findings = gd.check_writes(name, pool.written, lambda: call(plain), dirty=dirty, seed=n)
    findings += gd.check_reads(name, inputs, call, pool.written)
    return findings


@pytest.mark.parametrize("geom,reduce", PAIRS, ids=[f"{_gid(g)}-r{r}" for g, r in PAIRS])
def test_poisoned_buffers_and_neighbours(native, geom, reduce):
    findings = []
    for n in NS:
        findings += _findings(geom, n, reduce)
    assert not findings, "\n".join(findings)
