"""svc_hip_window_levels_frames (include/svc_hip.h: a stored SVCQ stream restricted to a window per output frame) without a device: the
workspace query, the order of the argument checks, and the numpy statement (scalable_video_codec_amd/layers.py: window_frame,
window_frames) on frames built from seeded random levels -- against layers.enhancement_frame, which states what the encoder writes with a
window.  The bytes the kernels write are tests/test_gpu_window_levels.py, which takes its frames from here."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native
from tests.test_gpu_layers import _window

# frame w, h, tile (w, h), MV block (w, h)
GEOMS = [
    (36, 12, (4, 4), (12, 12)),     # three MV blocks: the masks are only 4-byte aligned; 16 valid bits per mask word
    (36, 24, (12, 12), (12, 12)),   # 3 words per tile, the last partly used
    (272, 24, (8, 8), (16, 8)),     # 34 tiles per row: a group of 32 and one of 2 (16-row MV blocks do not divide 24 rows)
    (272, 32, (8, 8), (16, 16)),    # the same rows with 16 x 16 MV blocks
    (64, 48, (16, 16), (16, 16)),
]
KINDS = ("whole", "empty", "rect", "per-frame")
N = 4


def geom_dict(w, h, tile, mv):
    return {"frame_w": w, "frame_h": h, "block_w": tile[0], "block_h": tile[1], "mv_block_w": mv[0], "mv_block_h": mv[1]}


def random_types(rng, w, h, mv):
    types = (rng.integers(0, 3, (h // mv[1], w // mv[0])) * rng.integers(0, 2, (h // mv[1], w // mv[0]))).astype(np.uint32)
    types.flat[0] = 0
    types.flat[-1] = 5  # both classes where there are two MV blocks
    return types


def random_levels(rng, w, h, density):
    """(3, h, w) i64: int16 values, none of them 0 where the draw keeps the coefficient."""
    lv = rng.integers(1, 32768, (3, h, w)) * rng.choice([-1, 1], (3, h, w))
    return lv * (rng.random((3, h, w)) < density)


def random_stream(rng, geom, n, density, fg=4, bg=16):
    """n frames of seeded random levels -> (bytes, offsets (n + 1,) u64)."""
    w, h, tile, mv = geom
    frames = [layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), random_levels(rng, w, h, density), fg, bg) for _ in range(n)]
    return entropy._join(frames)


def layer_pair(rng, geom, fg, bg, enh, density=0.3):
    """A base and a fine frame of the same random 'coefficients', as two encodes of one frame relate (tests/test_layers_host.py)."""
    w, h, tile, mv = geom
    types = random_types(rng, w, h, mv)
    lf = random_levels(rng, w, h, density)
    step = np.repeat(np.repeat(np.where(types == 0, bg, fg), mv[1], 0), mv[0], 1).astype(np.int64)
    q = lf * enh / step[None]
    lb = (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int64)
    g = geom_dict(*geom)
    return layers.write_frame(g, types, lb, fg, bg), layers.write_frame(g, types, lf, enh, enh)


def _ids(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}-{g[3][0]}x{g[3][1]}"


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.window_levels_workspace_bytes
    assert q(2, 64, 72, 16, 16) == 0            # a frame the tile does not divide
    assert q(2, 64, 64, 8, (12, 16)) == 0       # an MV block that is not a multiple of the tile
    assert q(2, 256, 256, 128, 128) == 0        # a tile of more than 4096 coefficients
    assert q(70000, 64, 64, 8, 16) == 0         # more frames than one call takes
    assert q(2, 64, 64, 8, 16) > 0
    assert q(2, 64, 64, 4, 16) > 0              # not limited to the 8 / 16 transform
    assert q(2, 128, 64, 64, 64) > 0
    assert q(2, 36, 24, 12, 12) > 0
    assert q(4, 64, 64, 8, 16) > q(2, 64, 64, 8, 16)


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: each check below comes before the pointer checks, and the null-pointer check stands between all of them
    and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, n_in=2, n_out=2, src=None, ws=1 << 40, cap=1 << 40):
        return lib.svc_hip_window_levels_frames(None, 0, None, n_in, src, n_out, w, h, bw, bh, mbw, mbh, None, None, ws, None, cap, None,
                                                None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    some_src = (native.C.c_uint32 * 8)()
    for n in (2, 0):  # the contract does not depend on the frame counts
        assert call(100, 64, 8, 8, 16, 16, n, n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 8, 12, 16, n, n) == bad and "multiple of the tile" in err()
        # geometry before limits
        assert call(100, 64, 8, 8, 16, 16, 70000, 70000) == bad and "not divisible" in err()
        assert call(100, 256, 128, 128, 128, 128, n, n) == bad and "not divisible" in err()
        assert call(256, 256, 128, 128, 128, 128, n, n) == unsup and "4096" in err()
        # limits before the d_src rule, for either count
        assert call(64, 64, 8, 8, 16, 16, n, 70000) == unsup and "65535 frames" in err()
        assert call(64, 64, 8, 8, 16, 16, 70000, n, src=some_src) == unsup and "65535 frames" in err()
        assert call(256, 256, 128, 128, 128, 128, n, n + 1) == unsup and "4096" in err()
        # the d_src rule before workspace and capacity
        assert call(64, 64, 8, 8, 16, 16, n, n + 1, ws=0, cap=0) == bad and "d_src" in err()
        assert call(64, 64, 8, 8, 16, 16, n + 3, n, ws=0, cap=0) == bad and "d_src" in err()
    assert call(64, 64, 8, 8, 16, 16, 65535, 65535, ws=0, cap=0) == bad and "workspace" in err()  # the largest counts pass the limits
    need_ws = native.window_levels_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need_out > 0
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0) == bad and "workspace" in err()        # workspace before capacity
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16) == bad and "output" in err()   # capacity before pointers
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
    # the sizes follow n_out, not n_in
    need_ws3 = native.window_levels_workspace_bytes(3, 64, 64, 8, 16)
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3 - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out) == bad and "output" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out // 2 * 3) == bad and "null pointer" in err()
    # an empty batch is valid with sizes of 0, with and without d_src
    assert call(64, 64, 8, 8, 16, 16, 0, 0, ws=0, cap=0) == native.SVC_OK
    assert call(64, 64, 8, 8, 16, 16, 5, 0, src=some_src, ws=0, cap=0) == native.SVC_OK
    assert call(36, 24, 12, 12, 12, 12, 0, 0, ws=0, cap=0) == native.SVC_OK


def test_the_abi_version_did_not_move():
    assert native.load().svc_hip_abi_version() == 5


# ---- layers.window_frame / window_frames on frames built in numpy ------------------------------------------------------------------------

@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
@pytest.mark.parametrize("steps", [(1, 640, 1), (4, 16, 2)], ids=str)
def test_windowing_the_whole_enhancement_is_encoding_with_the_window(geom, steps):
    w, h, tile, mv = geom
    fg, bg, enh = steps
    rng = np.random.default_rng(w * 1000 + h + tile[0] + fg)
    pairs = [layer_pair(rng, geom, fg, bg, enh) for _ in range(N)]
    whole = [layers.enhancement_frame(b, f, enh, None) for b, f in pairs]
    stream, offs = entropy._join(whole)
    for kind in KINDS:
        windows = _window(kind, N, w, h, tile[0])
        want = [layers.enhancement_frame(b, f, enh, windows[i]) for i, (b, f) in enumerate(pairs)]
        for i in range(N):
            assert layers.window_frame(whole[i], windows[i]) == want[i], (kind, i)
        got, got_offs = layers.window_frames(stream, offs, windows)
        want_bytes, want_offs = entropy._join(want)
        assert got == want_bytes and np.array_equal(got_offs, want_offs) and got_offs.dtype == np.uint64
        if kind == "empty":  # every frame at its minimum: header, types, zero masks
            minimum = (64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * ((tile[0] * tile[1] + 63) // 64) + 15) // 16 * 16
            assert [int(o) for o in got_offs] == [i * minimum for i in range(N + 1)]
    # no window: a canonical frame's own bytes, one frame and a batch
    assert all(layers.window_frame(fr, None) == fr for fr in whole)
    got, got_offs = layers.window_frames(stream, offs, None)
    assert got == stream and np.array_equal(got_offs, offs)
    # ... and a base stream is windowed like any other SVCQ stream: a region-of-interest stream the reader takes
    base = pairs[0][0]
    rect = _window("rect", N, w, h, tile[0])[0]
    roi = layers.window_frame(base, rect)
    hdr, types, planes = levels.parse_frame(roi)
    hb, types_b, planes_b = levels.parse_frame(base)
    oy, ox = np.meshgrid(np.arange(h) // tile[1] * tile[1], np.arange(w) // tile[0] * tile[0], indexing="ij")
    inside = (ox >= rect[0]) & (ox < rect[0] + rect[2]) & (oy >= rect[1]) & (oy < rect[1] + rect[3])
    assert np.array_equal(types, types_b) and (hdr["fg_step"], hdr["bg_step"], hdr["inexact"]) == (hb["fg_step"], hb["bg_step"], hb["inexact"])
    assert np.array_equal(planes, np.where(inside[None], planes_b, 0)) and inside.any() and not inside.all()


@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_nested_windows_and_source_indices(geom):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w + h)
    stream, offs = random_stream(rng, geom, N, 0.4)
    frames = [stream[int(offs[i]):int(offs[i + 1])] for i in range(N)]
    outer = (tile[0], 0, w - tile[0] - 1, h)               # drops the first column of tiles; its right edge is inside the last one
    inner = (2 * tile[0] - 1, 0, max(1, w // 2), h - 1)     # its left edge inside a tile: origins from 2 tiles on
    for fr in frames:
        once = layers.window_frame(fr, inner)
        assert layers.window_frame(layers.window_frame(fr, outer), inner) == once
        assert layers.window_frame(once, inner) == once and layers.window_frame(once, outer) == once  # idempotent
        assert len(once) < len(layers.window_frame(fr, outer)) < len(fr)
    # src: repeats, any order, its own window per output frame
    src = [3, 0, 0, 2, 1, 3]
    windows = [outer, inner, outer, (0, 0, w, h), (0, 0, 0, 0), inner]
    got, got_offs = layers.window_frames(stream, offs, windows, src=src)
    want = [layers.window_frame(frames[s], windows[i]) for i, s in enumerate(src)]
    assert got == b"".join(want) and [int(o) for o in got_offs] == [0] + list(np.cumsum([len(x) for x in want]))
    got, got_offs = layers.window_frames(stream, offs, None, src=[2, 2])
    assert got == frames[2] * 2
    got, got_offs = layers.window_frames(stream, offs, None, src=[])
    assert got == b"" and [int(o) for o in got_offs] == [0]
    with pytest.raises(ValueError, match="input frame"):
        layers.window_frames(stream, offs, None, src=[0, N])


def test_the_statement_is_on_masks_and_refuses_what_the_reader_refuses():
    geom = GEOMS[1]
    w, h, tile, mv = geom
    rng = np.random.default_rng(5)
    stream, offs = random_stream(rng, geom, 1, 0.5)
    levels_off = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * 3
    b = np.frombuffer(stream, np.uint8).copy()
    count = int(b[40:44].view("<u4")[0])
    assert count > 8
    b[levels_off:levels_off + 16] = 0  # eight levels of value 0 whose mask bits stay set
    zeroed = b.tobytes()
    assert layers.window_frame(zeroed, None) == zeroed                          # they stay levels, and their bits stay set
    kept = np.frombuffer(layers.window_frame(zeroed, (0, 0, tile[0], tile[1])), np.uint8)
    masks = b[levels_off - 8 * 3 * 6 * 3:levels_off].reshape(3, 2, 3, 24)  # plane, tile row, tile, its three mask words
    first_tiles = int(np.unpackbits(masks[:, 0, 0]).sum())
    assert int(np.unpackbits(masks[0, 0, 0]).sum()) >= 8  # the zeroed levels are the first tile's
    assert int(kept[40:44].view("<u4")[0]) == first_tiles and not kept[levels_off:levels_off + 16].any()
    for word, value in ((0, 0x12345678), (1, 2), (2, w + tile[0]), (12, len(stream) + 16), (10, count + 1), (10, count - 1)):
        bad = np.frombuffer(stream, np.uint8).copy()
        bad[4 * word:4 * word + 4].view("<u4")[0] = value
        with pytest.raises(ValueError):
            layers.window_frame(bad, None)
        with pytest.raises(ValueError):
            layers.window_frames(bad, offs, [(0, 0, w, h)])
    stray = np.frombuffer(stream, np.uint8).copy()
    stray[levels_off - 1] |= 0x80  # bit 191 of the last tile's masks: past its 144 coefficients
    with pytest.raises(ValueError, match="past the tile"):
        layers.window_frame(stray, None)
