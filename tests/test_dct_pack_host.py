"""svc_hip_dct_pack_levels_frames (the compact stream straight from the transform kernel): what it answers without a device --
the workspace query and the order of its argument checks.  The bytes it writes are tests/test_gpu_dct_pack.py."""
from __future__ import annotations

import ctypes as C

from scalable_video_codec_amd import clip, native


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_levels_workspace_bytes
    assert q(2, 64, 64, 4, 16) == 0           # a 4x4 block: not the tuned transform
    lib = native.load()
    # an 8x16 block has no form in this signature (one side); the nearest refusals: a frame the block does not divide ...
    assert lib.svc_hip_dct_pack_levels_workspace_bytes(2, 64, 72, 16, 16, 16) == 0
    assert q(2, 72, 64, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16)) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8)) == 0
    assert q(2, 64, 64, 8, 16) > 0
    assert q(1, 3840, 2176, 16, 16) > 0


def test_workspace_holds_every_piece_at_its_worst_case():
    # 64 x 64 at 8x8: 4 segment columns per tile row = one wave, 8 tile rows, 3 planes = 24 pieces of 1024 int16; 192 mask words
    n, pieces, mask_bytes = 2, 24, 8 * 3 * 64
    assert native.dct_pack_levels_workspace_bytes(n, 64, 64, 8, 16) == n * pieces * 2048 + n * mask_bytes + 4 * n * pieces + 2 * 16
    # 272 wide: 17 segment columns = a full wave and a one-column wave per tile row
    assert native.dct_pack_levels_workspace_bytes(1, 272, 24, 8, 8) >= 3 * 3 * 2 * 2048


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, and the null-pointer check stands between any
    of them and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, fg, bg, n=2, ws=1 << 40, cap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        return lib.svc_hip_dct_pack_levels_frames(None, stride, n, w, h, block, None, mbw, mbh, fg, bg, None, ws, None, cap, None, None)
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, 1, 640, n=n) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, 1, 640, n=n) == native.SVC_ERR_INVALID_ARG and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, 1, 640, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, 1, 640, n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in err()
        assert call(64, 64, 8, 16, 16, 1, 640, n=n, stride=64 * 64 * 3 - 16) == native.SVC_ERR_INVALID_ARG and "stride" in err()
        # geometry before steps
        assert call(72, 64, 8, 8, 8, 0, 640, n=n) == native.SVC_ERR_UNSUPPORTED
        assert call(64, 64, 8, 16, 16, 0, 640, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 1, 0, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        # steps before sizes
        assert call(64, 64, 8, 16, 16, 0, 640, n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch
    assert call(64, 64, 16, 16, 16, 3, 17, n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, 1, 640, n=70000) == native.SVC_ERR_UNSUPPORTED and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_levels_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws - 1, cap=0) == native.SVC_ERR_INVALID_ARG and "workspace" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws, cap=need_out - 16) == native.SVC_ERR_INVALID_ARG and "worst case" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws, cap=need_out) == native.SVC_ERR_INVALID_ARG and "null pointer" in err()


def test_the_abi_version_did_not_move():
    assert native.load().svc_hip_abi_version() == 5


def test_clip_handle_takes_the_switch_in_the_tuning_word():
    assert clip.OUTPUT_COMPACT == 8192
    assert C.sizeof(clip.ClipConfig) == 136 and C.sizeof(clip.ClipInfo) == 80
    assert clip.BUFFERS["compact"][0] == 11 and clip.BUFFERS["compact_offsets"][0] == 12
