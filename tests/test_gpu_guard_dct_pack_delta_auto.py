"""Where svc_hip_dct_pack_delta_auto_frames writes and what its result depends on (tests/helpers/guarded.py): workspace, output stream,
offsets, key flags and level counts of exactly the sizes the API asks for inside guarded allocations, the four poisons (the leftovers of
a call with another frame count and of another entry point among them -- every count the selection sums was stored by this call's
counting kernel), and other bytes beside each input -- the frames, their region ids, the frame before, its region ids and the forced flags.  The
builder has the form of tests/test_gpu_guard_streams.py's and runs through its _check;
tests/test_gpu_placement_dct_pack_delta_auto.py takes it from here.

Nine frames with the fourth forced: a run of the kernels' ends inside the call, the flag falls inside it, and frame 0 hangs on the frame
before the call.  _bgr's frames (random, synthetic, zero, and again) are all key frames by the rule, so one of them is repeated: the
frame after it is a difference of no level, and both outcomes occur."""
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import G8, G16, _bgr, _check, _cuda, _gid, _past, _stream_out

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
N = 9
GEOMS = (G8[0], G16[0])  # 272 x 24 at 8 x 8, 144 x 48 at 16 x 16
STEPS = (1, 1)           # one step: every tile of a frame that is not a key frame is predicted, whatever the region ids


def forced_flags(n):
    return [int(i == 3) for i in range(n)]


REPEATED = 4  # frame 5 of the n + 1 is frame 4 again


def frames_and_types(geom, n, seed=0):
    """_bgr's n + 1 strided frames and their region ids, frame REPEATED + 1 a copy of frame REPEATED (where there are that many)."""
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n + 1, seed)
    if n + 1 > REPEATED + 1:
        buf[(REPEATED + 1) * stride:(REPEATED + 1) * stride + w * h * 3] = buf[REPEATED * stride:REPEATED * stride + w * h * 3].clone()
    return buf, stride, types


def e_dct_pack_delta_auto(pool, geom, n, seed):
    """frames_and_types' n + 1 strided frames: the first is the frame before the call's n, handed over as a buffer of its own."""
    w, h, tile, mv = geom
    buf, stride, types = frames_and_types(geom, n, seed)
    inputs = {"bgr": buf[stride:], "types": types[1:].contiguous(), "prev": buf[:w * h * 3].clone(), "prev types": types[0].clone(),
              "forced": _cuda(torch.tensor(forced_flags(n), dtype=torch.int32).numpy())}
    ws = pool.buf("workspace", nat.dct_pack_delta_auto_workspace_bytes(n, w, h, tile[0], mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    keys = pool.buf("key out", n, I32)
    counts = pool.buf("counts", 2 * n, I32)

    def call(i):
        before = out.clone()
        nat._check(nat.load().svc_hip_dct_pack_delta_auto_frames(
            i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, *STEPS, i["prev"].data_ptr(), i["prev types"].data_ptr(),
            i["forced"].data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), keys.data_ptr(), counts.data_ptr(),
            nat._stream()))
        _past("dct_pack_delta_auto", (out, offs, before))
        return {"stream": _stream_out(out, offs), "offsets": offs, "key out": keys, "counts": counts}
    return inputs, call


ENTRIES = {"dct_pack_delta_auto": (e_dct_pack_delta_auto, GEOMS)}


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1):
            assert nat.dct_pack_delta_auto_workspace_bytes(n, w, h, tile[0], mv) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_poisoned_buffers_and_neighbours(native, geom):
    findings = _check("dct_pack_delta_auto", e_dct_pack_delta_auto, geom, N, N - 2)
    assert not findings, "\n".join(findings)
