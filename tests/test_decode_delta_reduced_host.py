"""svc_hip_decode_delta_levels_reduced_frames (include/svc_hip.h: a delta stream straight to display frames at 1/2, 1/4, 1/8 size) without a
device: the workspace query, the order of the argument checks -- the reduced decoder's (geometry, steps, reduce, display size, limits,
workspace), then last_capacity, then n_frames == 0, then pointers -- and the identity in numpy that the call rests on: the band (0, 0, K, K)
commutes with the undelta, and the reduced decoder reads nothing else.  What the kernels write is tests/test_gpu_decode_delta_reduced.py."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import layers, levels, native
from tests.test_band_levels_host import frames_of
from tests.test_decode_delta_host import DECODE_GEOMS, REFUSED_GEOMS
from tests.test_delta_levels_host import KEYS, STEPS, _gid, delta_clip

REDUCES = (2, 4, 8)


def test_both_symbols_are_bound():
    assert "svc_hip_decode_delta_levels_reduced_workspace_bytes" in native.SIGNATURES
    assert "svc_hip_decode_delta_levels_reduced_frames" in native.SIGNATURES
    assert native.load().svc_hip_abi_version() == 5


def test_the_workspace_query_is_zero_where_the_call_refuses():
    q = native.decode_delta_levels_reduced_workspace_bytes
    for w, h, tile, mv in DECODE_GEOMS:
        assert q(6, w, h, tile, mv) > 0
        assert q(6, w, h, tile, mv) > q(3, w, h, tile, mv) > q(1, w, h, tile, mv)
    for w, h, tile, mv in REFUSED_GEOMS:
        assert q(6, w, h, tile, mv) == 0
    assert q(2, 72, 64, 8, 8) == 0        # a width that is not whole 16-pixel segments
    assert q(70000, 64, 64, 8, 16) == 0   # more frames than one call takes


def _call(lib, w=64, h=64, bw=8, bh=8, mbw=16, mbh=16, n=2, fg=1, bg=640, reduce=2, dw=0, dh=0, ws=1 << 40, last=None, cap=0):
    return lib.svc_hip_decode_delta_levels_reduced_frames(None, 0, None, n, None, 0, None, w, h, bw, bh, mbw, mbh, fg, bg, reduce, None, None,
                                                          ws, None, None, dw, dh, last, cap, None, None, None)


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL except where a check needs one to be reached: each check comes before the next, and all before the pointers."""
    lib = native.load()
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    a_pointer = 1 << 20  # never dereferenced: the call answers before any device work

    def err():
        return lib.svc_hip_last_error().decode()

    def call(**kw):
        return _call(lib, **kw)

    for n in (2, 0):  # the contract does not depend on the frame count
        # 1. geometry: the format's, then the decoder's
        assert call(w=100, n=n) == bad and "not divisible" in err()
        assert call(mbw=12, n=n) == bad and "multiple of the tile" in err()
        assert call(w=36, h=12, bw=4, bh=4, mbw=12, mbh=12, n=n) == unsup and "8x8, 16x16" in err()
        assert call(w=48, h=32, bw=16, bh=8, mbw=16, mbh=8, n=n) == unsup and "8x8, 16x16" in err()
        assert call(w=72, bw=8, bh=8, mbw=8, mbh=8, n=n) == unsup and "multiple of 16" in err()
        # 2. steps
        assert call(fg=0, n=n) == bad and "steps" in err()
        assert call(bg=0, n=n) == bad and "steps" in err()
        # 3. reduce
        for r in (0, 1, 3, 16):
            assert call(reduce=r, n=n) == bad and "reduce" in err(), r
            assert call(reduce=r, fg=0, n=n) == bad and "steps" in err(), r               # after the steps
            assert call(reduce=r, dw=999, dh=999, n=n) == bad and "reduce" in err(), r    # before the display size
        # 4. display size: 1 .. the padded size / reduce
        for r in REDUCES:
            assert call(reduce=r, dw=64 // r + 1, dh=64 // r, n=n) == bad and "display" in err(), r
            assert call(reduce=r, dw=64 // r, dh=64 // r + 1, n=n) == bad and "display" in err(), r
            assert call(reduce=r, dw=64 // r, dh=0, n=n) == bad and "display" in err(), r
    assert call(w=100, fg=0, reduce=3, dw=999, n=70000, ws=0) == bad and "not divisible" in err()  # geometry before everything
    assert call(fg=0, reduce=3, dw=999, dh=1, n=70000, ws=0) == bad and "steps" in err()
    assert call(reduce=3, dw=999, dh=1, n=70000, ws=0) == bad and "reduce" in err()
    assert call(dw=999, dh=1, n=70000, ws=0) == bad and "display" in err()                          # the display size before limits
    assert call(n=70000, ws=0) == unsup and "65535 frames" in err()                                 # 5. limits before the sizes
    assert call(n=65535, ws=0) == bad and "workspace" in err()                                      # 6. workspace
    need_ws = native.decode_delta_levels_reduced_workspace_bytes(2, 64, 64, 8, 16)
    need_last = native.levels_max_bytes(1, 64, 64, 8, 16)
    assert need_ws > 0 and need_last > 0
    for r in REDUCES:
        assert call(reduce=r, ws=need_ws - 1, last=a_pointer, cap=0) == bad and "workspace" in err()           # workspace before last_capacity
        assert call(reduce=r, ws=need_ws, last=a_pointer, cap=need_last - 16) == bad and "last frame" in err()  # 7. the full-size call's rule
        assert call(reduce=r, ws=need_ws, last=a_pointer, cap=need_last) == bad and "null pointer" in err()     # 9. pointers
        assert call(reduce=r, ws=need_ws, dw=64 // r, dh=64 // r) == bad and "null pointer" in err()
    assert call(ws=need_ws, cap=0) == bad and "null pointer" in err()  # without d_last its capacity is not looked at
    for n_ws in (0, need_ws):
        assert call(n=0, ws=n_ws, last=a_pointer, cap=need_last - 16) == bad and "last frame" in err()  # ... for any n_frames


def test_no_frames_is_ok_with_null_pointers():
    lib = native.load()
    for w, h, (bw, bh), (mbw, mbh) in DECODE_GEOMS:
        for r in REDUCES:
            assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, reduce=r, ws=0) == native.SVC_OK
            assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, fg=4, bg=16, reduce=r, dw=w // r, dh=h // r, ws=0) == native.SVC_OK
    assert _call(lib, n=0, ws=0, last=1 << 20, cap=native.levels_max_bytes(1, 64, 64, 8, 16)) == native.SVC_OK  # (d_last stays untouched)
    for w, h, (bw, bh), (mbw, mbh) in REFUSED_GEOMS:
        assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, ws=0) == native.SVC_ERR_UNSUPPORTED


# ---- the statement: layers.undelta_frames + levels.decode_reduced_frame + layers.band_frames ---------------------------------------------

@pytest.mark.parametrize("geom", DECODE_GEOMS, ids=_gid)
def test_the_band_commutes_with_the_undelta_and_the_reduced_decoder_reads_nothing_else(geom):
    """For every (N, K): the undelta of the band (0, 0, K, K) is the band of the undelta, byte for byte -- the chain is per coefficient -- and
    the reduced decoder gives the same bits on a frame and on its band."""
    w, h, tile, _ = geom
    stream, offs = delta_clip(np.random.default_rng(w + 3 * h), geom)
    gaze = (tile[0], 0, max(tile[0], w // 2), h)
    for keys in (KEYS, None):
        diff, diff_offs = layers.delta_frames(stream, offs, keys)
        back, back_offs = layers.undelta_frames(diff, diff_offs, keys)
        assert back == stream
        for r in REDUCES:
            k = tile[0] // r
            bands = np.tile(np.array([0, 0, k, k]), (6, 1))
            banded = layers.band_frames(back, back_offs, bands)
            served = layers.band_frames(diff, diff_offs, bands)
            assert len(served[0]) < len(diff)
            chained = layers.undelta_frames(*served, keys)
            assert chained[0] == banded[0] and chained[1].tolist() == banded[1].tolist(), (keys, r)
            for full, cut in zip(frames_of(back, back_offs), frames_of(*chained)):
                for steps, gz in ((STEPS, None), ((3, 17), gaze)):
                    a = levels.decode_reduced_frame(full, r, *steps, gz)
                    b = levels.decode_reduced_frame(cut, r, *steps, gz)
                    assert a.shape == (h // r, w // r, 3) and np.array_equal(a.view(np.int32), b.view(np.int32)), (keys, r)
