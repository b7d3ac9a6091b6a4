"""Where svc_hip_dct_pack_delta_frames writes and what its result depends on (tests/helpers/guarded.py): workspace, output stream and
offsets of exactly the sizes the API asks for inside guarded allocations, the four poisons (the leftovers of a call with another frame
count and of another entry point among them), and other bytes beside each input -- the frames, their region ids, the frame before, its
region ids and the key flags.  The builder has the form of tests/test_gpu_guard_streams.py's and runs through its _check;
tests/test_gpu_placement_dct_pack_delta.py takes it from here.

Six frames with a key flag on the fourth: the flag falls inside a run of the kernel's, the call's only run is cut short, and frame 0
hangs on the frame before the call."""
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import G8, G16, _bgr, _check, _cuda, _gid, _past, _stream_out

pytestmark = pytest.mark.gpu

U8, I64 = torch.uint8, torch.int64
N = 6
GEOMS = (G8[0], G16[0])  # 272 x 24 at 8 x 8, 144 x 48 at 16 x 16
STEPS = (1, 1)           # one step: every tile of a frame that is not a key frame is predicted, whatever the region ids


def key_flags(n):
    return [int(i == 3) for i in range(n)]


def e_dct_pack_delta(pool, geom, n, seed):
    """_bgr's n + 1 strided frames: the first is the frame before the call's n, handed over as a buffer of its own."""
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n + 1, seed)
    inputs = {"bgr": buf[stride:], "types": types[1:].contiguous(), "prev": buf[:w * h * 3].clone(), "prev types": types[0].clone(),
              "key": _cuda(torch.tensor(key_flags(n), dtype=torch.int32).numpy())}
    ws = pool.buf("workspace", nat.dct_pack_delta_workspace_bytes(n, w, h, tile[0], mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)

    def call(i):
        before = out.clone()
        nat._check(nat.load().svc_hip_dct_pack_delta_frames(
            i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, *STEPS, i["prev"].data_ptr(), i["prev types"].data_ptr(),
            i["key"].data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), nat._stream()))
        _past("dct_pack_delta", (out, offs, before))
        return {"stream": _stream_out(out, offs), "offsets": offs}
    return inputs, call


ENTRIES = {"dct_pack_delta": (e_dct_pack_delta, GEOMS)}


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1):
            assert nat.dct_pack_delta_workspace_bytes(n, w, h, tile[0], mv) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_poisoned_buffers_and_neighbours(native, geom):
    findings = _check("dct_pack_delta", e_dct_pack_delta, geom, N, N - 2)
    assert not findings, "\n".join(findings)
