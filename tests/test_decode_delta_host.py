"""svc_hip_decode_delta_levels_frames (include/svc_hip.h: a delta stream straight to display frames) without a device: the workspace
query and the order of the argument checks -- the decoder's (geometry, steps, display size, limits, workspace), then last_capacity, then
n_frames == 0, then pointers.  What the kernels write is tests/test_gpu_decode_delta.py."""
from __future__ import annotations

import pytest

from scalable_video_codec_amd import native

# the geometries of tests/test_delta_levels_host.py::BAND_GEOMS the decoder takes, and three it refuses
DECODE_GEOMS = [(272, 24, (8, 8), (16, 8)), (64, 48, (16, 16), (16, 16)), (16, 704, (8, 8), (16, 16))]
REFUSED_GEOMS = [(36, 12, (4, 4), (12, 12)), (48, 32, (16, 8), (16, 8)), (128, 64, (64, 64), (64, 64))]


def test_both_symbols_are_bound():
    assert "svc_hip_decode_delta_levels_workspace_bytes" in native.SIGNATURES
    assert "svc_hip_decode_delta_levels_frames" in native.SIGNATURES
    assert native.load().svc_hip_abi_version() == 5


def test_the_workspace_query_is_zero_where_the_call_refuses():
    q = native.decode_delta_levels_workspace_bytes
    for w, h, tile, mv in DECODE_GEOMS:
        assert q(6, w, h, tile, mv) > 0
        assert q(6, w, h, tile, mv) > q(3, w, h, tile, mv)
        # the undelta's input arrays, and the last frame's levels at every group's worst-case place
        assert q(1, w, h, tile, mv) >= 2 * 3 * w * h
    for w, h, tile, mv in REFUSED_GEOMS:
        assert q(6, w, h, tile, mv) == 0
        assert native.undelta_levels_workspace_bytes(6, w, h, tile, mv) > 0  # the format's own calls take them
    assert q(2, 72, 64, 8, 8) == 0        # a width that is not whole 16-pixel segments
    assert q(2, 64, 72, 16, 16) == 0      # a frame the tile does not divide
    assert q(70000, 64, 64, 8, 16) == 0   # more frames than one call takes


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL except where a check needs one to be reached: each check comes before the pointer checks."""
    lib = native.load()
    fn = lib.svc_hip_decode_delta_levels_frames
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    a_pointer = 1 << 20  # never dereferenced: the call answers before any device work

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w=64, h=64, bw=8, bh=8, mbw=16, mbh=16, n=2, fg=1, bg=640, dw=0, dh=0, ws=1 << 40, last=None, cap=0):
        return fn(None, 0, None, n, None, 0, None, w, h, bw, bh, mbw, mbh, fg, bg, None, None, ws, None, None, dw, dh, last, cap, None, None,
                  None)

    for n in (2, 0):  # the contract does not depend on the frame count
        # 1. geometry: the format's, then the decoder's
        assert call(w=100, n=n) == bad and "not divisible" in err()
        assert call(mbw=12, n=n) == bad and "multiple of the tile" in err()
        assert call(w=36, h=12, bw=4, bh=4, mbw=12, mbh=12, n=n) == unsup and "8x8, 16x16" in err()
        assert call(w=48, h=32, bw=16, bh=8, mbw=16, mbh=8, n=n) == unsup and "8x8, 16x16" in err()
        assert call(w=128, h=64, bw=64, bh=64, mbw=64, mbh=64, n=n) == unsup and "8x8, 16x16" in err()
        assert call(w=72, bw=8, bh=8, mbw=8, mbh=8, n=n) == unsup and "multiple of 16" in err()
        # 2. steps, 3. display size
        assert call(fg=0, n=n) == bad and "steps" in err()
        assert call(bg=0, n=n) == bad and "steps" in err()
        assert call(dw=65, dh=64, n=n) == bad and "display" in err()
        assert call(dw=64, dh=0, n=n) == bad and "display" in err()
    assert call(w=100, fg=0, dw=999, n=70000, ws=0) == bad and "not divisible" in err()     # geometry before everything
    assert call(fg=0, dw=999, dh=1, n=70000, ws=0) == bad and "steps" in err()              # steps before the display size
    assert call(dw=999, dh=1, n=70000, ws=0) == bad and "display" in err()                  # the display size before limits
    assert call(n=70000, ws=0) == unsup and "65535 frames" in err()                         # 4. limits before the sizes
    assert call(n=65535, ws=0) == bad and "workspace" in err()                              # 5. workspace
    need_ws, need_last = native.decode_delta_levels_workspace_bytes(2, 64, 64, 8, 16), native.levels_max_bytes(1, 64, 64, 8, 16)
    assert need_ws > 0 and need_last > 0
    assert call(ws=need_ws - 1, last=a_pointer, cap=0) == bad and "workspace" in err()      # workspace before last_capacity
    assert call(ws=need_ws, last=a_pointer, cap=need_last - 16) == bad and "last frame" in err()  # 6. last_capacity before pointers
    assert call(ws=need_ws, last=a_pointer, cap=need_last) == bad and "null pointer" in err()
    assert call(ws=need_ws, cap=0) == bad and "null pointer" in err()                       # without d_last its capacity is not looked at
    for n_ws in (0, need_ws):
        assert call(n=0, ws=n_ws, last=a_pointer, cap=need_last - 16) == bad and "last frame" in err()  # ... for any n_frames


def test_no_frames_is_ok_with_null_pointers():
    lib = native.load()
    fn = lib.svc_hip_decode_delta_levels_frames
    for w, h, (bw, bh), (mbw, mbh) in DECODE_GEOMS:
        assert fn(None, 0, None, 0, None, 0, None, w, h, bw, bh, mbw, mbh, 1, 640, None, None, 0, None, None, 0, 0, None, 0, None, None,
                  None) == native.SVC_OK
        assert fn(None, 0, None, 0, None, 0, None, w, h, bw, bh, mbw, mbh, 4, 16, None, None, 0, None, None, w, h, None, 0, None, None,
                  None) == native.SVC_OK
    for w, h, (bw, bh), (mbw, mbh) in REFUSED_GEOMS:
        assert fn(None, 0, None, 0, None, 0, None, w, h, bw, bh, mbw, mbh, 1, 640, None, None, 0, None, None, 0, 0, None, 0, None, None,
                  None) == native.SVC_ERR_UNSUPPORTED
