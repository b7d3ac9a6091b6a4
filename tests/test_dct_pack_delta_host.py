"""svc_hip_dct_pack_delta_frames (the delta stream straight from the transform kernel): what it answers without a device -- the
workspace query, the order of its argument checks and the pairing of d_prev_bgr with d_prev_types.  The bytes it writes are
tests/test_gpu_dct_pack_delta.py."""
from __future__ import annotations

from scalable_video_codec_amd import native


def test_the_binding_exists():
    assert callable(native.dct_pack_delta_frames) and callable(native.dct_pack_delta_workspace_bytes)


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_delta_workspace_bytes
    assert q(2, 64, 64, 4, 16) == 0           # a 4x4 block: not the tuned transform
    assert native.load().svc_hip_dct_pack_delta_workspace_bytes(2, 64, 72, 16, 16, 16) == 0  # a frame the block does not divide
    assert q(2, 72, 64, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16)) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8)) == 0
    assert q(70000, 64, 64, 8, 16) == 0       # more frames than a call takes
    assert q(2, 64, 64, 8, 16) > 0
    assert q(1, 3840, 2176, 16, 16) > 0
    # the frame before lives in registers: nothing beyond the fused pack's scratch
    assert q(6, 272, 24, 8, 8) == native.dct_pack_levels_workspace_bytes(6, 272, 24, 8, 8)


def _err():
    return native.load().svc_hip_last_error().decode()


def _call(w, h, block, mbw, mbh, fg, bg, n=2, ws=1 << 40, cap=1 << 40, stride=None, ptrs=(None,) * 8):
    """ptrs: d_bgr, d_block_types, d_prev_bgr, d_prev_types, d_key, d_workspace, d_out, d_frame_offsets."""
    stride = w * h * 3 if stride is None else stride
    bgr, types, pbgr, ptypes, key, wsp, out, offs = ptrs
    return native.load().svc_hip_dct_pack_delta_frames(bgr, stride, n, w, h, block, types, mbw, mbh, fg, bg, pbgr, ptypes, key, wsp, ws, out, cap,
                                                       offs, None)


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, and the null-pointer check stands between any
    of them and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    call, err = _call, _err
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, 1, 640, n=n) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, 1, 640, n=n) == native.SVC_ERR_INVALID_ARG and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, 1, 640, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in err()
        assert call(64, 64, 4, 16, 16, 1, 640, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, 1, 640, n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in err()
        assert call(64, 64, 8, 16, 16, 1, 640, n=n, stride=64 * 64 * 3 - 16) == native.SVC_ERR_INVALID_ARG and "stride" in err()
        assert call(64, 64, 8, 16, 16, 1, 640, n=n, stride=64 * 64 * 3 + 8) == native.SVC_ERR_INVALID_ARG and "stride" in err()
        # geometry before steps
        assert call(72, 64, 8, 8, 8, 0, 640, n=n) == native.SVC_ERR_UNSUPPORTED
        assert call(64, 64, 8, 16, 16, 0, 640, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 1, 0, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
        # steps before sizes
        assert call(64, 64, 8, 16, 16, 0, 640, n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch
    assert call(64, 64, 16, 16, 16, 3, 17, n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, 1, 640, n=70000) == native.SVC_ERR_UNSUPPORTED and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_delta_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws - 1, cap=0) == native.SVC_ERR_INVALID_ARG and "workspace" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws, cap=need_out - 16) == native.SVC_ERR_INVALID_ARG and "worst case" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, ws=need_ws, cap=need_out) == native.SVC_ERR_INVALID_ARG and "null pointer" in err()


def test_the_frame_before_is_pixels_and_types_together():
    """The pairing and the alignment rules are answered on the host, in front of any launch: the addresses are never read."""
    a = 0x10000  # 16-byte aligned, never dereferenced
    base = [a, a, None, None, None, a, a, a]

    def call(**over):
        p = list(base)
        for k, v in over.items():
            p[{"bgr": 0, "types": 1, "pbgr": 2, "ptypes": 3, "key": 4, "ws": 5, "out": 6, "offs": 7}[k]] = v
        return _call(64, 64, 8, 16, 16, 1, 640, ptrs=tuple(p))
    assert call(pbgr=a) == native.SVC_ERR_INVALID_ARG and "together" in _err()
    assert call(ptypes=a) == native.SVC_ERR_INVALID_ARG and "together" in _err()
    # each pointer one notch below the alignment the header admits
    assert call(pbgr=a + 8, ptypes=a) == native.SVC_ERR_INVALID_ARG and "aligned" in _err()
    assert call(pbgr=a, ptypes=a + 2) == native.SVC_ERR_INVALID_ARG and "aligned" in _err()
    assert call(key=a + 2) == native.SVC_ERR_INVALID_ARG and "aligned" in _err()
    assert call(bgr=a + 8) == native.SVC_ERR_INVALID_ARG and "aligned" in _err()
    assert call(offs=a + 4) == native.SVC_ERR_INVALID_ARG and "aligned" in _err()
    # a missing required pointer is reported before the pairing
    assert call(bgr=None, pbgr=a) == native.SVC_ERR_INVALID_ARG and "null pointer" in _err()
