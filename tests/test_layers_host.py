"""The two layers of the compact stream (include/svc_hip.h, "Two layers") without a device: the workspace queries and the order of the
argument checks of svc_hip_dct_pack_layers_frames and svc_hip_decode_layers_frames, and the numpy statement
(scalable_video_codec_amd/layers.py) on frames built from random levels.  The bytes the kernels write are tests/test_gpu_layers.py."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native


def test_workspace_queries_are_zero_where_the_calls_refuse():
    q = native.dct_pack_layers_workspace_bytes
    assert q(2, 64, 64, 4, 16) == 0           # a 4x4 block: not the tuned transform
    assert native.load().svc_hip_dct_pack_layers_workspace_bytes(2, 64, 72, 16, 16, 16) == 0  # a frame the block does not divide
    assert q(2, 72, 64, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16)) == 0     # an MV block that is not a multiple of the tile
    assert q(70000, 64, 64, 8, 16) == 0       # more frames than one call takes
    # two layers: twice the one-layer call's
    assert q(2, 64, 64, 8, 16) == 2 * native.dct_pack_levels_workspace_bytes(2, 64, 64, 8, 16) > 0
    assert q(1, 3840, 2176, 16, 16) == 2 * native.dct_pack_levels_workspace_bytes(1, 3840, 2176, 16, 16) > 0
    d = native.decode_layers_workspace_bytes
    assert d(2, 64, 64, 4) == 0 and d(2, 64, 64, (8, 16)) == 0 and d(2, 72, 64, 8) == 0 and d(2, 64, 60, 8) == 0
    assert d(70000, 64, 64, 8) == 0
    assert d(2, 64, 64, 8) == 2 * native.decode_levels_workspace_bytes(2, 64, 64, 8) > 0
    assert d(3, 1920, 1088, 16) == 2 * native.decode_levels_workspace_bytes(3, 1920, 1088, 16) > 0


def test_encode_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, and the null-pointer check stands between any of
    them and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, fg, bg, enh, n=2, ws=1 << 40, cap=1 << 40, ecap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        return lib.svc_hip_dct_pack_layers_frames(None, stride, n, w, h, block, None, mbw, mbh, fg, bg, enh, None, None, ws, None, cap,
                                                  None, None, ecap, None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, 1, 640, 1, n=n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, 1, 640, 1, n=n) == bad and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, 1, 640, 1, n=n) == unsup and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, 1, 640, 1, n=n) == unsup and "multiple of 16" in err()
        assert call(64, 64, 8, 16, 16, 1, 640, 1, n=n, stride=64 * 64 * 3 - 16) == bad and "stride" in err()
        assert call(72, 64, 8, 8, 8, 1, 640, 0, n=n) == unsup  # geometry before steps
        assert call(64, 64, 8, 16, 16, 1, 640, 0, n=n) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 0, 640, 1, n=n) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 1, 0, 1, n=n) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 3, 17, 2, n=n) == bad and "multiple" in err()
        assert call(64, 64, 8, 16, 16, 4, 6, 4, n=n) == bad and "multiple" in err()
        assert call(64, 64, 8, 16, 16, 2, 4, 4, n=n) == bad                       # enh_step above the foreground's step
        assert call(64, 64, 16, 16, 16, 1, 32767, 1, n=n) == unsup and "32766" in err()  # a ratio over 32766
        assert call(64, 64, 16, 16, 16, 2 * 32767, 2, 2, n=n) == unsup and "32766" in err()
        # steps before sizes
        assert call(64, 64, 8, 16, 16, 1, 640, 0, n=n, ws=0, cap=0, ecap=0) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, 3, 17, 2, n=n, ws=0, cap=0, ecap=0) == bad and "multiple" in err()
        assert call(64, 64, 8, 16, 16, 1, 32767, 1, n=n, ws=0, cap=0, ecap=0) == unsup and "32766" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, 1, n=0, ws=0, cap=0, ecap=0) == native.SVC_OK  # a valid empty batch
    assert call(64, 64, 16, 16, 16, 4, 16, 2, n=0) == native.SVC_OK
    assert call(64, 64, 16, 16, 16, 32766, 32766, 1, n=0) == native.SVC_OK             # the largest ratio
    assert call(64, 64, 8, 16, 16, 1, 640, 1, n=70000, ws=0, cap=0, ecap=0) == unsup and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_layers_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, 1, 640, 1, ws=need_ws - 1, cap=0, ecap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, 1, ws=need_ws, cap=need_out - 16, ecap=0) == bad and "base output" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, 1, ws=need_ws, cap=need_out, ecap=need_out - 16) == bad and "enhancement output" in err()
    assert call(64, 64, 8, 16, 16, 1, 640, 1, ws=need_ws, cap=need_out, ecap=need_out) == bad and "null pointer" in err()


def test_decode_argument_checks_answer_without_a_device():
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, fg, bg, n=2, ws=1 << 40, dw=0, dh=0, gaze=None):
        return lib.svc_hip_decode_layers_frames(None, 0, None, None, 0, None, n, w, h, bw, bh, mbw, mbh, fg, bg, gaze, None, ws, None, None,
                                                dw, dh, None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):
        assert call(100, 64, 8, 8, 16, 16, 1, 640, n=n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 16, 16, 16, 1, 640, n=n) == unsup and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, 8, 0, 640, n=n) == unsup                      # geometry before steps
        assert call(64, 64, 8, 8, 16, 16, 0, 640, n=n) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 8, 16, 16, 0, 640, n=n, dw=65, dh=64, ws=0) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 8, 16, 16, 1, 640, n=n, dw=65, dh=64, ws=0) == bad and "steps" not in err()  # the display size, before sizes
    assert call(64, 64, 8, 8, 16, 16, 1, 640, n=70000, ws=0) == unsup and "65535 frames" in err()  # limits before sizes
    need = native.decode_layers_workspace_bytes(2, 64, 64, 8)
    assert call(64, 64, 8, 8, 16, 16, 1, 640, ws=need - 1) == bad and "workspace" in err()
    assert call(64, 64, 8, 8, 16, 16, 1, 640, n=0, ws=0) == native.SVC_OK
    # with and without a gaze the pointers come last
    assert call(64, 64, 8, 8, 16, 16, 1, 640, ws=need) == bad and "null pointer" in err()
    gaze = (native.C.c_uint32 * 8)()
    assert call(64, 64, 8, 8, 16, 16, 1, 640, ws=need, gaze=gaze) == bad and "decode_layers: null pointer" in err()


def test_the_abi_version_did_not_move():
    assert native.load().svc_hip_abi_version() == 5


# ---- layers.py on frames built in numpy -----------------------------------------------------------------------------------------------

W, H, BLOCK, MV = 48, 32, 8, (16, 16)
GEOM = {"frame_w": W, "frame_h": H, "block_w": BLOCK, "block_h": BLOCK, "mv_block_w": MV[0], "mv_block_h": MV[1]}


def _round_half_away(q):
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def _pair(rng, fg, bg, enh):
    """A base and a fine frame of the same random 'coefficients': fine levels are random int16 values, sparse, and the base level of
    a coefficient is what quantising fine * enh at the tile's base step gives -- the relation the two encodes of one frame have."""
    types = (rng.integers(0, 3, (H // MV[1], W // MV[0])) * rng.integers(0, 2, (H // MV[1], W // MV[0]))).astype(np.uint32)
    types[0, 0], types[0, 1] = 0, 5  # both classes, whatever the draw
    bound = 32767  # every int16 fine level: the base level is smaller in magnitude and the residual at most half a ratio
    lf = rng.integers(-bound, bound + 1, (3, H, W)) * (rng.random((3, H, W)) < 0.3)
    lf[0, :2, :4] = [[bound, -bound, 1, -1], [0, 2, -2, 3]]
    step = np.repeat(np.repeat(np.where(types == 0, bg, fg), MV[1], 0), MV[0], 1).astype(np.int64)
    lb = _round_half_away(lf * enh / step[None]).astype(np.int64)
    base = layers.write_frame(GEOM, types, lb, fg, bg)
    fine = layers.write_frame(GEOM, types, lf, enh, enh)
    return types, step, lf, lb, base, fine


def _bits(frame):
    """(header, masks' popcount, the bytes behind the last level) of an SVCQ frame, read from its sections."""
    b = np.frombuffer(frame, np.uint8)
    hdr = b[:64].view("<u4")
    masks_off = 64 + 4 * (W // MV[0]) * (H // MV[1])
    levels_off = masks_off + 8 * 3 * (W // BLOCK) * (H // BLOCK)
    pop = int(np.unpackbits(b[masks_off:levels_off]).sum())
    return hdr, pop, b[levels_off + 2 * int(hdr[10]):]


@pytest.mark.parametrize("fg,bg,enh", [(1, 1, 1), (2, 4, 2), (4, 16, 2), (1, 640, 1), (3, 18, 3), (640, 640, 1)])
def test_enhancement_frames_state_the_definition(fg, bg, enh):
    rng = np.random.default_rng(fg * 1000 + bg + enh)
    n = 3
    pairs = [_pair(rng, fg, bg, enh) for _ in range(n)]
    base, base_offs = entropy._join([p[4] for p in pairs])
    fine, fine_offs = entropy._join([p[5] for p in pairs])
    # edges inside tiles: origins 8 .. 32 in x and 8, 16 in y are inside; an empty window; the whole frame
    windows = [(5, 3, 30, 20), (0, 0, 0, H), (0, 0, W, H)]
    for window in (None, windows):
        enh_bytes, enh_offs = layers.enhancement_frames(base, base_offs, fine, fine_offs, enh, window)
        assert enh_offs[0] == 0 and len(enh_offs) == n + 1 and enh_offs[-1] == len(enh_bytes)
        for f, (types, step, lf, lb, base_f, _) in enumerate(pairs):
            frame = enh_bytes[int(enh_offs[f]):int(enh_offs[f + 1])]
            hdr, types_back, planes = levels.parse_frame(frame)  # raises unless level_count == the masks' popcount
            assert all(hdr[k] == GEOM[k] for k in GEOM) and np.array_equal(types_back, types)
            assert hdr["fg_step"] == hdr["bg_step"] == enh and hdr["inexact"] == 0 and hdr["frame_bytes"] == len(frame) and len(frame) % 16 == 0
            words, pop, pad = _bits(frame)
            assert pop == words[10] and not words[13:16].any() and not pad.any() and len(pad) < 16
            d = np.rint(planes.astype(np.float64) / enh).astype(np.int64)
            oy, ox = np.meshgrid(np.arange(H) // BLOCK * BLOCK, np.arange(W) // BLOCK * BLOCK, indexing="ij")
            inside = np.ones((H, W), bool)
            if window is not None:
                x, y, w, h = window[f]
                inside = (ox >= x) & (ox < x + w) & (oy >= y) & (oy < y + h)
                assert inside.sum() == ((4 * 2 if f == 0 else 0 if f == 1 else 6 * 4) * BLOCK * BLOCK)
            ratio = step // enh
            assert np.array_equal((lb * ratio + d)[:, inside], lf[:, inside])
            assert not d[:, ~inside].any()
            if fg == bg == enh:
                assert hdr["level_count"] == 0  # every frame at its minimum size
            # what the decoder dequantises: the fine levels at enh inside gaze and window, the base's own elsewhere
            gaze = (16, 0, 24, 17)
            merged, steps = layers.merge_levels(base_f, frame, gaze)
            gz = (ox >= 16) & (ox < 40) & (oy < 17)
            assert np.array_equal(merged[:, gz & inside], lf[:, gz & inside])
            assert np.array_equal(merged[:, gz & ~inside], (lb * ratio)[:, gz & ~inside])
            assert np.array_equal(merged[:, ~gz], lb[:, ~gz])
            px = np.repeat(np.repeat(steps, BLOCK, 0), BLOCK, 1)
            assert np.array_equal(px, np.where(gz, enh, step))
            none, none_steps = layers.merge_levels(base_f, None, None)
            assert np.array_equal(none, lb) and np.array_equal(np.repeat(np.repeat(none_steps, BLOCK, 0), BLOCK, 1), step)
        # the entropy coder's host statement takes an enhancement stream like any SVCQ stream
        coded, coded_offs = entropy.encode_frames(enh_bytes, enh_offs)
        back, back_offs = entropy.decode_frames(coded, coded_offs)
        assert back == enh_bytes and np.array_equal(back_offs, enh_offs)


def test_frames_that_are_no_layers_of_each_other_are_refused():
    rng = np.random.default_rng(7)
    types, step, lf, lb, base, fine = _pair(rng, 4, 16, 2)
    with pytest.raises(ValueError, match="steps"):
        layers.enhancement_frames(base, [0, len(base)], fine, [0, len(fine)], 4)  # not the fine stream's step
    two_steps = layers.write_frame(GEOM, types, lf, 2, 4)
    with pytest.raises(ValueError, match="steps"):
        layers.enhancement_frame(base, two_steps, 2)
    with pytest.raises(ValueError, match="not a layer"):
        layers.merge_levels(base, two_steps, (0, 0, W, H))
    with pytest.raises(ValueError, match="not a layer"):
        layers.merge_levels(base, layers.write_frame(GEOM, types, lf, 3, 3), (0, 0, W, H))  # 3 does not divide 4
    other = dict(GEOM, mv_block_w=8, mv_block_h=8)
    with pytest.raises(ValueError, match="geometry"):
        layers.merge_levels(base, layers.write_frame(other, np.zeros((H // 8, W // 8), np.uint32), lf, 2, 2), (0, 0, W, H))
    with pytest.raises(ValueError, match="int16"):
        layers.write_frame(GEOM, types, lf * 0 + 40000, 1, 1)
