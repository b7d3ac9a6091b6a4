"""Where svc_hip_delta_levels_frames and svc_hip_undelta_levels_frames write and what their results depend on (tests/helpers/guarded.py):
workspace, output stream, offsets and status of exactly the sizes the API asks for inside guarded allocations, the four poisons, and
other bytes beside each input, the frame before and the key flags included.  The builders have the form of
tests/test_gpu_guard_streams.py's and run through its _check; tests/test_gpu_placement_delta.py takes them from here."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_gpu_guard_streams import ENC, NS, STREAM, _check, _cuda, _gid, _past, _statuses, _stream_out, _svcq

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64


def key_flags(n):
    """A key frame in the middle of a batch of five; none in the shorter ones, whose frames all hang on the frame before."""
    return [int(i == 3) for i in range(n)]


@functools.lru_cache(maxsize=None)
def clip_parts(geom, n, seed=0):
    """_svcq's n + 1 frames: the first is the frame before the call's n -> (the frame before, the n frames, their offsets, their delta
    stream by the numpy statement, its offsets), as arrays."""
    q, qo = _svcq(geom, n + 1, ENC, seed)
    f = frames_of(q.tobytes(), qo)
    stream, offs = entropy._join(f[1:])
    diff, diff_offs = layers.delta_frames(stream, offs, key_flags(n), prev=f[0])
    as_array = lambda b, o: (np.frombuffer(b, np.uint8).copy(), np.asarray(o).astype(np.int64))
    return (np.frombuffer(f[0], np.uint8).copy(),) + as_array(stream, offs) + as_array(diff, diff_offs)


def _builder(undo):
    def build(pool, geom, n, seed):
        w, h, tile, mv = geom
        prev, stream, offs, diff, diff_offs = clip_parts(geom, n, seed)
        inputs = {"stream": _cuda(diff if undo else stream), "offsets": _cuda(diff_offs if undo else offs), "prev": _cuda(prev),
                  "key": _cuda(np.asarray(key_flags(n), np.int32))}
        query = nat.undelta_levels_workspace_bytes if undo else nat.delta_levels_workspace_bytes
        fn = nat.undelta_levels_frames if undo else nat.delta_levels_frames
        ws = pool.buf("workspace", query(n, w, h, tile, mv), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        out_offs = pool.buf("offsets", n + 1, I64)
        status = pool.buf("status", n, I32)

        def call(i):
            before = out.clone()
            fn(i["stream"], i["offsets"], w, h, tile, mv, prev=i["prev"], key=i["key"], out=out, out_offsets=out_offs, workspace=ws,
               status=status)
            _past(fn.__name__, (out, out_offs, before))
            _statuses(status, n, None)
            return {"stream": _stream_out(out, out_offs), "offsets": out_offs, "status": status}
        return inputs, call
    return build


e_delta_levels, e_undelta_levels = _builder(False), _builder(True)
ENTRIES = {"delta_levels": (e_delta_levels, STREAM), "undelta_levels": (e_undelta_levels, STREAM)}
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms]


def test_every_pair_is_sized(native):
    """No case below is a refusal in disguise."""
    for entry, geom in PAIRS:
        w, h, tile, mv = geom
        query = nat.delta_levels_workspace_bytes if entry == "delta_levels" else nat.undelta_levels_workspace_bytes
        for n in NS:
            assert query(n, w, h, tile, mv) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0, (entry, geom, n)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    findings = []
    for n in NS:
        findings += _check(entry, ENTRIES[entry][0], geom, n, max(1, n - 2))
    assert not findings, "\n".join(findings)
