"""The batch's frame offsets past one 256-frame trip of their kernel (csrc/levels.hip: frame_offsets_kernel, one kernel for the window
call, the split's two layers and the entropy coder's two directions).

300 frames of 16 x 16 (8 x 8 tiles, 16 x 16 MV blocks) from the numpy writer, a few of them without a level, go through
svc_hip_window_levels_frames (a window per frame, some empty), svc_hip_split_levels_frames at (1, 3, 1) and svc_hip_entropy_encode_frames,
and back through svc_hip_entropy_decode_frames.  Every call's n + 1 offsets and its stream are compared byte for byte with the numpy
statements: layers.window_frames, layers.split_frames, entropy.encode_frames.  (A frame's group scan past 256 groups is the 16 x 704 case
of tests/test_gpu_window_levels.py.  Some seventy trips, with the offsets themselves past 2^32, for every stream call: tests/test_gpu_large_streams.py.)"""
import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers
from tests import test_gpu_split_levels as split
from tests import test_gpu_window_levels as window
from tests.test_gpu_entropy import _check_codec
from tests.test_window_levels_host import geom_dict, random_levels

pytestmark = pytest.mark.gpu

N = 300
GEOM = (16, 16, (8, 8), (16, 16))
EMPTY = (0, 7, 255, 256, 299)  # frames without a level, on both sides of the trip's edge


@pytest.fixture(scope="module")
def stream():
    """(bytes, offsets (N + 1,) u64, windows (N, 4)): frames at steps (1, 1), the fine stream the split takes."""
    rng = np.random.default_rng(300)
    w, h, tile, mv = GEOM
    # one MV block per frame: background or foreground, so both of the split's ratios (1 and 3) occur
    frames = [layers.write_frame(geom_dict(*GEOM), np.full((1, 1), 3 * rng.integers(0, 2), np.uint32),
                                 random_levels(rng, w, h, 0.0 if i in EMPTY else 0.3), 1, 1) for i in range(N)]
    # a window per frame: one tile, a row or a column of tiles, the frame, or nothing (w or h of 0)
    rects = [(0, 0, 16, 16), (8, 0, 8, 8), (0, 8, 16, 8), (8, 0, 8, 16), (0, 0, 0, 16), (4, 4, 16, 0), (0, 0, 8, 8)]
    windows = np.array([rects[rng.integers(len(rects))] for _ in range(N)], dtype=np.uint32)
    return entropy._join(frames) + (windows,)


def test_window_offsets_past_one_trip(native, stream):
    data, offs, windows = stream
    got = window._call(data, offs, GEOM, windows)
    window._expect(got, *layers.window_frames(data, offs, windows))
    assert got[2] == [0] * N


def test_split_offsets_of_both_layers_past_one_trip(native, stream):
    data, offs, windows = stream
    got = split._call(data, offs, GEOM, (3, 1, 1), windows)  # (fg, bg, fine) = the entry point's (fine, fg, bg) = (1, 3, 1)
    want = layers.split_frames(data, offs, 1, 3, 1, windows)
    split._expect_layer(got["base"], got["boffs"], want[0], want[1])
    split._expect_layer(got["enh"], got["eoffs"], want[2], want[3])
    assert got["status"] == [0] * N


def test_entropy_offsets_both_ways_past_one_trip(native, stream):
    data, offs, _ = stream
    w, h, tile, mv = GEOM
    _check_codec(split._dev(data), split._offsets(offs), w, h, tile, mv)
