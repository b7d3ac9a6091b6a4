"""svc_hip_dct_pack_levels_budget_frames (rate control inside the fused transform): what it answers without a device -- the workspace
query and the order of its argument checks.  The bytes it writes are tests/test_gpu_dct_pack_budget.py."""
from __future__ import annotations

import ctypes as C

from scalable_video_codec_amd import clip, native


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_levels_budget_workspace_bytes
    assert q(2, 64, 64, 4, 16, 8) == 0           # a 4x4 block: not the tuned transform
    assert q(2, 72, 64, 8, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16), 8) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8), 8) == 0
    assert q(2, 64, 64, 8, 16, 0) == 0           # a ladder of 1 .. 64 entries
    assert q(2, 64, 64, 8, 16, 65) == 0
    for n, w, h, block, mv in ((2, 64, 64, 8, 16), (1, 3840, 2176, 16, 16), (3, 272, 24, 8, (16, 8))):
        for k in (1, 8, 64):
            assert q(n, w, h, block, mv, k) > 0
            assert q(n, w, h, block, mv, k) >= native.dct_pack_levels_workspace_bytes(n, w, h, block, mv)  # it holds the fused call's


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, and the null-pointer check stands between any of
    them and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, ladder, n=2, ws=1 << 40, cap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        arr, k = native._ladder(ladder)
        return lib.svc_hip_dct_pack_levels_budget_frames(None, stride, n, w, h, block, None, mbw, mbh, arr, k, None, None, ws, None, cap,
                                                         None, None, None)
    good = [(1, 640), (2, 640), (2, 700)]
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, good, n=n) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, good, n=n) == native.SVC_ERR_INVALID_ARG and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, good, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, good, n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in err()
        # geometry before the ladder, the stride before the ladder
        assert call(72, 64, 8, 8, 8, [(0, 640)], n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in err()
        assert call(64, 64, 8, 16, 16, [(0, 640)], n=n, stride=64 * 64 * 3 - 16) == native.SVC_ERR_INVALID_ARG and "stride" in err()
        # the ladder: its length, a zero step, a decreasing fg_step, a decreasing bg_step -- before any size
        assert call(64, 64, 8, 16, 16, [], n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "ladder of 0 entries" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640)] * 65, n=n) == native.SVC_ERR_INVALID_ARG and "ladder of 65 entries" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (0, 640)], n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, [(1, 0)], n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, [(2, 640), (1, 640)], n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "non-decreasing" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (2, 639)], n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "non-decreasing" in err()
    assert call(64, 64, 8, 16, 16, good, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch
    assert call(64, 64, 16, 16, 16, [(3, 17)], n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, good, n=70000, ws=0, cap=0) == native.SVC_ERR_UNSUPPORTED and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_levels_budget_workspace_bytes(2, 64, 64, 8, 16, len(good))
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, good, ws=need_ws - 1, cap=0) == native.SVC_ERR_INVALID_ARG and "workspace" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out - 16) == native.SVC_ERR_INVALID_ARG and "worst case" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out) == native.SVC_ERR_INVALID_ARG and "null pointer" in err()


def test_the_abi_and_the_clip_handle_did_not_move():
    assert native.load().svc_hip_abi_version() == 5
    assert C.sizeof(clip.ClipConfig) == 136 and C.sizeof(clip.ClipInfo) == 80
    assert clip.BUFFERS["compact"][0] == 11 and clip.BUFFERS["compact_offsets"][0] == 12  # the new buffer is appended
    assert clip.BUFFERS["compact_choice"][0] == 13
    assert "svc_clip_set_compact_budget" in clip.SIGNATURES
