"""svc_hip_decode_delta_levels_reduced_frames once on a batch whose frame offsets pass 2^32 and whose frame count is some seventy trips of
256 frames: tests/test_gpu_large_streams.py's case for the full-size call (its sources, its preconditions and its comparison, on
tests/helpers/periodic.py), at reduce 8 so that rec stays near 0.2 GB.  16 x 16 tiles: K = 2, two coefficient rows of a tile in one mask
word.  The workgroups of this kernel walk all frames of the call, so the frame index, the frame's byte offset and the rec row of frame f
are what a 32-bit product would break here.  rec, display and status are bit for bit the same call's output on the 2k-frame prefix, extended
periodically; what that short call computes is pinned by tests/test_gpu_decode_delta_reduced.py."""
import numpy as np
import pytest

from scalable_video_codec_amd import native as nat
from tests.helpers import periodic as pd
from tests.test_gpu_large_streams import DEC, DEV, G16, GAZE, K, _crossed, _decode_case, _figures, _frames_for, _key_frame, _rows, big  # noqa: F401

pytestmark = pytest.mark.gpu

REDUCE = 8
DISPLAY = (24, 20)  # inside the 32 x 32 picture


def test_decode_delta_levels_reduced(big):  # noqa: F811
    """Key flags at frame 0 and at the start of the last whole cycle, above 2^32 in the stream."""
    w, h, tile, mv = G16
    src = big.get("delta", G16)
    ref = nat.decode_delta_levels_reduced_frames(*src.prefix_dev(), w, h, tile, mv, *DEC, REDUCE, gaze=_rows(GAZE).astype(np.int32),
                                                 display=DISPLAY)
    n = _frames_for(src.cycle_bytes)
    restarts = (0, (n // K - 1) * K)
    big.get("svcq", G16).release()
    stream, offs, offs_np = src.take(n, restarts)
    _crossed("in", offs_np)
    _, keys = _key_frame(n, offs_np)
    got = nat.decode_delta_levels_reduced_frames(stream, offs, w, h, tile, mv, *DEC, REDUCE, key=keys, gaze=pd.repeat_rows(GAZE, n, DEV),
                                                 display=DISPLAY)
    assert got[0].shape == (n, h // REDUCE, w // REDUCE, 3) and ref[0][:K].abs().max().item() > 1  # pictures, not zeros
    _decode_case("decode_delta_levels_reduced", n, ref, got, REDUCE, restarts=restarts)
