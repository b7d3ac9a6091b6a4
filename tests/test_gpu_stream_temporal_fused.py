"""svc::StreamEncoder with temporal_period 2 and 4 against ONE svc_hip_dct_pack_delta_temporal_frames call over the whole clip, through
tests/dropin/stream_temporal_main as tests/test_gpu_stream_temporal.py runs it (its clip, its runs): at batches of 4 and 16, depths 3
and 4, key_interval 0 and 5, SVCQ and SVCE, the encoder's stream and key flags are those of the one call on the clip's encoded frames
with the region ids the encoder found -- however the clip falls into batches, and whichever calls the encoder makes per batch."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.test_gpu_stream_temporal import H, MV, N, W, _clip, _dev, _forced, _keys, _stream, _temporal
from tests.test_gpu_stream_temporal import work  # noqa: F401  (the fixture: the clip on disk, shared runs)

pytestmark = pytest.mark.gpu

FG, BG = 1, 640  # StreamEncoderConfig's defaults, which stream_temporal_main leaves


@pytest.mark.parametrize("entropy", [0, 1], ids=["svcq", "svce"])
@pytest.mark.parametrize("key_interval", [0, 5])
@pytest.mark.parametrize("period", [2, 4])
def test_the_encoder_gives_one_call_over_the_clip(native, work, period, key_interval, entropy):  # noqa: F811
    block = 8
    frames = _clip()[1:].contiguous()  # the encoded frame with clip index f is source frame f; the padded size is the clip's
    want_keys = _forced(key_interval)
    want = None
    for batch in (4, 16):
        for depth in (3, 4):
            run = _temporal(work, period, block=block, batch=batch, depth=depth, key_interval=key_interval, entropy=entropy)
            types = torch.from_numpy(np.fromfile(run + ".types", np.uint32).astype(np.int32).reshape(N - 1, -1)).cuda()
            assert types.shape[1] == (W // MV) * (H // MV)
            out, offs = nat.dct_pack_delta_temporal_frames(frames, block, types, MV, FG, BG, period, key=want_keys)
            torch.cuda.synchronize()
            one = (out[:int(offs[-1])].cpu().numpy().tobytes(), offs.cpu().tolist())
            assert want is None or one == want  # the region ids do not depend on batch or depth either
            want = one
            assert _keys(run) == want_keys, (batch, depth)
            got, got_offs = _stream(run)
            if entropy:
                back, back_offs, st = nat.entropy_decode_frames(_dev(got), _dev(got_offs.astype(np.int64)), W, H, block, MV)
                torch.cuda.synchronize()
                assert st.cpu().tolist() == [0] * (N - 1)
                got, got_offs = back[:int(back_offs[-1])].cpu().numpy(), back_offs.cpu().numpy()
            assert got_offs.tolist() == want[1], (batch, depth)
            assert got.tobytes() == want[0], (batch, depth)


@pytest.mark.parametrize("period", [2, 4])
def test_sixteen_by_sixteen_tiles(native, work, period):  # noqa: F811
    block = 16
    frames = _clip()[1:].contiguous()
    for batch, key_interval in ((4, 5), (16, 0)):
        run = _temporal(work, period, block=block, batch=batch, key_interval=key_interval)
        types = torch.from_numpy(np.fromfile(run + ".types", np.uint32).astype(np.int32).reshape(N - 1, -1)).cuda()
        out, offs = nat.dct_pack_delta_temporal_frames(frames, block, types, MV, FG, BG, period, key=_forced(key_interval))
        torch.cuda.synchronize()
        got, got_offs = _stream(run)
        assert got_offs.tolist() == offs.cpu().tolist()
        assert got.tobytes() == out[:int(offs[-1])].cpu().numpy().tobytes()
