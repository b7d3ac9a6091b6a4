"""Where svc_hip_dct_pack_delta_temporal_frames and svc_hip_dct_pack_delta_temporal_auto_frames write and what their results depend on
(tests/helpers/guarded.py), at periods 2 and 4: workspace, output stream, offsets -- and the auto call's key flags and level counts -- of
exactly the sizes the API asks for inside guarded allocations, the four poisons (the leftovers of a call with another frame count and of
another entry point among them), and other bytes beside each input: the frames, their region ids, the frame at index -period, its region
ids and the key or forced flags.  The builders have the form of tests/test_gpu_guard_streams.py's and run through its _check;
tests/test_gpu_placement_dct_pack_delta_temporal.py and tests/test_gpu_stream_order_dct_pack_delta_temporal.py take them from here.

Nine frames with a flag on the fourth: a run of the kernels' ends inside the call, the flag falls at layer position 3, frame 8 is a run's
first frame whose reference lies in the run before, and frame 0 hangs on the frame handed in.  The call's frame 1 is a copy of its frame
0, its reference at either period: the auto call's rule gives both outcomes."""
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import G8, G16, _bgr, _check, _cuda, _gid, _past, _stream_out

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
N = 9
GEOMS = (G8[0], G16[0])  # 272 x 24 at 8 x 8, 144 x 48 at 16 x 16
PERIODS = (2, 4)
STEPS = (1, 1)           # one step: every tile of a frame that is not a key frame is predicted, whatever the region ids
REPEATED = 1             # the call's frame 1 is its frame 0 again


def flags(n):
    return [int(i == 3) for i in range(n)]


def frames_and_types(geom, n, seed=0):
    """_bgr's n + 1 strided frames and their region ids (the first is the frame in front of the call's n), the call's frame REPEATED a copy
    of the frame before it (where there are that many)."""
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n + 1, seed)
    if n > REPEATED:
        buf[(REPEATED + 1) * stride:(REPEATED + 1) * stride + w * h * 3] = buf[REPEATED * stride:REPEATED * stride + w * h * 3].clone()
    return buf, stride, types


def _inputs(geom, n, seed, flag_name):
    w, h, tile, mv = geom
    buf, stride, types = frames_and_types(geom, n, seed)
    return stride, {"bgr": buf[stride:], "types": types[1:].contiguous(), "prev": buf[:w * h * 3].clone(), "prev types": types[0].clone(),
                    flag_name: _cuda(torch.tensor(flags(n), dtype=torch.int32).numpy())}


def temporal_builder(period):
    def build(pool, geom, n, seed):
        w, h, tile, mv = geom
        stride, inputs = _inputs(geom, n, seed, "key")
        ws = pool.buf("workspace", nat.dct_pack_delta_temporal_workspace_bytes(n, w, h, tile[0], mv, period), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)

        def call(i):
            before = out.clone()
            nat._check(nat.load().svc_hip_dct_pack_delta_temporal_frames(
                i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, *STEPS, i["prev"].data_ptr(),
                i["prev types"].data_ptr(), i["key"].data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                nat._stream(), period))
            _past(f"dct_pack_delta_temporal period {period}", (out, offs, before))
            return {"stream": _stream_out(out, offs), "offsets": offs}
        return inputs, call
    return build


def temporal_auto_builder(period):
    def build(pool, geom, n, seed):
        w, h, tile, mv = geom
        stride, inputs = _inputs(geom, n, seed, "forced")
        ws = pool.buf("workspace", nat.dct_pack_delta_temporal_auto_workspace_bytes(n, w, h, tile[0], mv, period), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)
        keys = pool.buf("key out", n, I32)
        counts = pool.buf("counts", 2 * n, I32)

        def call(i):
            before = out.clone()
            nat._check(nat.load().svc_hip_dct_pack_delta_temporal_auto_frames(
                i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, *STEPS, i["prev"].data_ptr(),
                i["prev types"].data_ptr(), i["forced"].data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                keys.data_ptr(), counts.data_ptr(), nat._stream(), period))
            _past(f"dct_pack_delta_temporal_auto period {period}", (out, offs, before))
            return {"stream": _stream_out(out, offs), "offsets": offs, "key out": keys, "counts": counts}
        return inputs, call
    return build


# key -> (builder, geometries); the key is the C function's name between svc_hip_ and _frames, then the period
ENTRIES = {}
for _p in PERIODS:
    ENTRIES[f"dct_pack_delta_temporal{_p}"] = (temporal_builder(_p), GEOMS)
    ENTRIES[f"dct_pack_delta_temporal_auto{_p}"] = (temporal_auto_builder(_p), GEOMS)


def fn_of(entry):
    return f"svc_hip_{entry.rstrip('0123456789')}_frames"


def period_of(entry):
    return int(entry[-1])


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1):
            for p in PERIODS:
                assert nat.dct_pack_delta_temporal_workspace_bytes(n, w, h, tile[0], mv, p) > 0
                assert nat.dct_pack_delta_temporal_auto_workspace_bytes(n, w, h, tile[0], mv, p) > 0
            assert nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    findings = _check(entry, ENTRIES[entry][0], geom, N, N - 2)
    assert not findings, "\n".join(findings)
