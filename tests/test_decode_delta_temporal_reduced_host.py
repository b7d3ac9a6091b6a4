"""svc_hip_decode_delta_levels_temporal_reduced_frames (include/svc_hip_temporal_decode.h: a delta stream with temporal layers straight to display
frames at 1/2, 1/4, 1/8 size) without a device: the workspace query, the order of the argument checks -- geometry, then the period, then
the reduced delta decode's own (steps, reduce, display size, limits, workspace, last_capacity, n_frames == 0, pointers) -- and the
identities in numpy that the call rests on: the band (0, 0, K, K) commutes with the temporal undelta and with the thinning, and the reduced
decoder of the undelta's output reads nothing outside K x K.  What the kernels write is tests/test_gpu_decode_delta_temporal_reduced.py."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native
from tests.test_band_levels_host import frames_of
from tests.test_decode_delta_host import DECODE_GEOMS, REFUSED_GEOMS
from tests.test_delta_levels_host import STEPS, _gid, delta_clip
from tests.test_delta_temporal_host import KEYS, N, PERIODS

REDUCES = (2, 4, 8)
BAD_PERIODS = (0, 3, 8)


def test_both_symbols_are_bound():
    assert "svc_hip_decode_delta_levels_temporal_reduced_workspace_bytes" in native.SIGNATURES_TEMPORAL_DECODE
    assert "svc_hip_decode_delta_levels_temporal_reduced_frames" in native.SIGNATURES_TEMPORAL_DECODE
    lib = native.load()
    assert lib.svc_hip_decode_delta_levels_temporal_reduced_frames.argtypes[-1] is native.SIGNATURES_TEMPORAL_DECODE[
        "svc_hip_decode_delta_levels_temporal_reduced_frames"][1][-1]
    # the reduced call's arguments, in its order, and the period behind them
    assert (native.SIGNATURES_TEMPORAL_DECODE["svc_hip_decode_delta_levels_temporal_reduced_frames"][1][:-1]
            == native.SIGNATURES["svc_hip_decode_delta_levels_reduced_frames"][1])
    assert lib.svc_hip_abi_version() == 5


def test_the_workspace_query_is_zero_where_the_call_refuses():
    q, reduced = native.decode_delta_levels_temporal_reduced_workspace_bytes, native.decode_delta_levels_reduced_workspace_bytes
    for period in PERIODS:
        for w, h, tile, mv in DECODE_GEOMS:
            assert q(6, w, h, tile, mv, period) == reduced(6, w, h, tile, mv) > 0  # the reduced call's workspace
            assert q(6, w, h, tile, mv, period) > q(3, w, h, tile, mv, period) > q(1, w, h, tile, mv, period)
        for w, h, tile, mv in REFUSED_GEOMS:
            assert q(6, w, h, tile, mv, period) == 0
        assert q(2, 72, 64, 8, 8, period) == 0        # a width that is not whole 16-pixel segments
        assert q(70000, 64, 64, 8, 16, period) == 0   # more frames than one call takes
    for period in BAD_PERIODS:
        assert q(2, 64, 64, 8, 16, period) == 0


def _call(lib, w=64, h=64, bw=8, bh=8, mbw=16, mbh=16, n=2, fg=1, bg=640, reduce=2, dw=0, dh=0, ws=1 << 40, last=None, cap=0, period=4):
    return lib.svc_hip_decode_delta_levels_temporal_reduced_frames(None, 0, None, n, None, 0, None, w, h, bw, bh, mbw, mbh, fg, bg, reduce, None,
                                                                   None, ws, None, None, dw, dh, last, cap, None, None, None, period)


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
        for period in PERIODS:
            # 1. geometry: the format's, then the decoder's
            assert call(w=100, n=n, period=period) == bad and "not divisible" in err()
            assert call(mbw=12, n=n, period=period) == bad and "multiple of the tile" in err()
            assert call(w=36, h=12, bw=4, bh=4, mbw=12, mbh=12, n=n, period=period) == unsup and "8x8, 16x16" in err()
            assert call(w=48, h=32, bw=16, bh=8, mbw=16, mbh=8, n=n, period=period) == unsup and "8x8, 16x16" in err()
            assert call(w=72, bw=8, bh=8, mbw=8, mbh=8, n=n, period=period) == unsup and "multiple of 16" in err()
            # 3. steps
            assert call(fg=0, n=n, period=period) == bad and "steps" in err()
            assert call(bg=0, n=n, period=period) == bad and "steps" in err()
            # 4. reduce
            for r in (0, 1, 3, 16):
                assert call(reduce=r, n=n, period=period) == bad and "reduce" in err(), r
                assert call(reduce=r, fg=0, n=n, period=period) == bad and "steps" in err(), r               # after the steps
                assert call(reduce=r, dw=999, dh=999, n=n, period=period) == bad and "reduce" in err(), r    # before the display size
            # 5. display size: 1 .. the padded size / reduce
            for r in REDUCES:
                assert call(reduce=r, dw=64 // r + 1, dh=64 // r, n=n, period=period) == bad and "display" in err(), r
                assert call(reduce=r, dw=64 // r, dh=64 // r + 1, n=n, period=period) == bad and "display" in err(), r
                assert call(reduce=r, dw=64 // r, dh=0, n=n, period=period) == bad and "display" in err(), r
        # 2. the period: after the geometry, before the steps and everything behind them
        for period in BAD_PERIODS:
            assert call(w=100, n=n, period=period) == bad and "not divisible" in err() and "period" not in err()
            assert call(w=36, h=12, bw=4, bh=4, mbw=12, mbh=12, n=n, period=period) == unsup and "8x8, 16x16" in err()
            assert call(n=n, period=period) == bad and f"period {period}" in err()
            assert call(n=n, fg=0, period=period) == bad and f"period {period}" in err()
            assert call(n=n, reduce=3, period=period) == bad and f"period {period}" in err()
            assert call(n=n, dw=999, dh=1, period=period) == bad and f"period {period}" in err()
            assert call(n=n, ws=0, last=a_pointer, cap=0, period=period) == bad and f"period {period}" in err()
    assert call(w=100, fg=0, reduce=3, dw=999, n=70000, ws=0, period=3) == bad and "not divisible" in err()  # geometry before everything
    assert call(fg=0, reduce=3, dw=999, dh=1, n=70000, ws=0, period=3) == bad and "period 3" in err()
    assert call(fg=0, reduce=3, dw=999, dh=1, n=70000, ws=0) == bad and "steps" in err()
    assert call(reduce=3, dw=999, dh=1, n=70000, ws=0) == bad and "reduce" in err()
    assert call(dw=999, dh=1, n=70000, ws=0) == bad and "display" in err()                          # the display size before limits
    assert call(n=70000, ws=0) == unsup and "65535 frames" in err()                                 # 6. limits before the sizes
    assert call(n=65535, ws=0) == bad and "workspace" in err()                                      # 7. workspace
    need_last = native.levels_max_bytes(1, 64, 64, 8, 16)
    for period in PERIODS:
        need_ws = native.decode_delta_levels_temporal_reduced_workspace_bytes(2, 64, 64, 8, 16, period)
        assert need_ws > 0 and need_last > 0
        for r in REDUCES:
            kw = dict(reduce=r, period=period)
            assert call(ws=need_ws - 1, last=a_pointer, cap=0, **kw) == bad and "workspace" in err()            # workspace before last_capacity
            assert call(ws=need_ws, last=a_pointer, cap=need_last - 16, **kw) == bad and "last frame" in err()  # 8. the full-size call's rule
            assert call(ws=need_ws, last=a_pointer, cap=need_last, **kw) == bad and "null pointer" in err()     # 10. pointers
            assert call(ws=need_ws, dw=64 // r, dh=64 // r, **kw) == bad and "null pointer" in err()
        assert call(ws=need_ws, cap=0, period=period) == bad and "null pointer" in err()  # without d_last its capacity is not looked at
        for n_ws in (0, need_ws):
            assert call(n=0, ws=n_ws, last=a_pointer, cap=need_last - 16, period=period) == bad and "last frame" in err()  # ... for any n_frames


def test_no_frames_is_ok_with_null_pointers():
    lib = native.load()
    for period in PERIODS:
        for w, h, (bw, bh), (mbw, mbh) in DECODE_GEOMS:
            for r in REDUCES:
                assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, reduce=r, ws=0, period=period) == native.SVC_OK
                assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, fg=4, bg=16, reduce=r, dw=w // r, dh=h // r, ws=0, period=period) == native.SVC_OK
        assert _call(lib, n=0, ws=0, last=1 << 20, cap=native.levels_max_bytes(1, 64, 64, 8, 16), period=period) == native.SVC_OK  # (d_last stays untouched)
        for w, h, (bw, bh), (mbw, mbh) in REFUSED_GEOMS:
            assert _call(lib, w, h, bw, bh, mbw, mbh, n=0, ws=0, period=period) == native.SVC_ERR_UNSUPPORTED
    for period in BAD_PERIODS:
        assert _call(lib, n=0, ws=0, period=period) == native.SVC_ERR_INVALID_ARG


# ---- the statement: layers.undelta_temporal_frames + levels.decode_reduced_frame + layers.band_frames / layers.thin_frames ---------------

@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", DECODE_GEOMS, ids=_gid)
def test_the_band_commutes_with_the_temporal_undelta_and_with_the_thinning(geom, period):
    """For every (N, K): the temporal undelta of the band (0, 0, K, K) is the band of the temporal undelta, byte for byte -- the tree of
    references is per coefficient -- the reduced decoder gives the same bits on a frame and on its band, and the band of the thinned stream
    is the thinned band stream, which undoes at period >> s (at 1: by the plain undelta) to the band of the kept frames."""
    w, h, tile, _ = geom
    stream, offs = delta_clip(np.random.default_rng(w + 3 * h + period), geom, N)
    gaze = (tile[0], 0, max(tile[0], w // 2), h)
    for keys in (KEYS, None):
        diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, keys)
        back, back_offs = layers.undelta_temporal_frames(diff, diff_offs, period, keys)
        assert back == stream
        for r in REDUCES:
            k = tile[0] // r
            bands = np.tile(np.array([0, 0, k, k]), (N, 1))
            banded = layers.band_frames(back, back_offs, bands)
            served = layers.band_frames(diff, diff_offs, bands)
            assert len(served[0]) < len(diff)
            chained = layers.undelta_temporal_frames(*served, period, keys)
            assert chained[0] == banded[0] and chained[1].tolist() == banded[1].tolist(), (keys, r)
            for i, (full, cut) in enumerate(zip(frames_of(back, back_offs), frames_of(*chained))):
                steps, gz = ((STEPS, None), ((3, 17), gaze))[i % 2]
                a = levels.decode_reduced_frame(full, r, *steps, gz)
                b = levels.decode_reduced_frame(cut, r, *steps, gz)
                assert a.shape == (h // r, w // r, 3) and np.array_equal(a.view(np.int32), b.view(np.int32)), (keys, r, i)
            for every in (2, 4):
                if every > period:
                    continue
                kept = list(range(0, N, every))
                thin, thin_offs, thin_keys = layers.thin_frames(diff, diff_offs, keys, every)
                band_then_thin = layers.thin_frames(*served, keys, every)
                thin_then_band = layers.band_frames(thin, thin_offs, bands[:len(kept)])
                assert band_then_thin[0] == thin_then_band[0] and band_then_thin[1].tolist() == thin_then_band[1].tolist(), (keys, r, every)
                # ... which is also the two device calls' statement: the window call with d_src, and the band call with d_src
                assert layers.window_frames(*served, None, src=kept)[0] == thin_then_band[0]
                assert layers.band_frames(diff, diff_offs, bands[:len(kept)], src=kept)[0] == thin_then_band[0]
                undone = layers.undelta_temporal_frames(*thin_then_band, period // every, thin_keys)
                want = entropy._join([frames_of(*banded)[i] for i in kept])
                assert undone[0] == want[0] and undone[1].tolist() == want[1].tolist(), (keys, r, every)
                if period == every:
                    assert layers.undelta_frames(*thin_then_band, thin_keys)[0] == want[0]
