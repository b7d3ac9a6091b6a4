"""svc_hip_band_levels_frames and svc_hip_union_levels_frames (include/svc_hip.h: a stored SVCQ stream restricted to a frequency band per
output frame, and bands joined back) without a device: the workspace queries, the order of the argument checks, and the numpy statements
(scalable_video_codec_amd/layers.py: band_frame, band_frames, union_frame, union_frames) on frames built from seeded random levels.  The
bytes the kernels write are tests/test_gpu_band_levels.py, which takes its frames and bands from here."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native
from tests.test_window_levels_host import GEOMS, _ids, geom_dict, random_levels, random_stream, random_types

BAND_GEOMS = GEOMS + [
    (128, 64, (64, 64), (64, 64)),   # 64 mask words per tile
    (48, 32, (16, 8), (16, 8)),      # a tile that is not square
]
DENSITIES = {"zero": 0.0, "sparse": 0.3, "full": 1.0}
N = 3


def partitions(tile):
    """Nested bands that partition a tile: two of them, and four (the cuts at 1/8, 1/4 and 1/2 of the longer side, at least 1 and rising)."""
    bw, bh = tile
    side = max(bw, bh)
    k = sorted({max(1, side // 8), max(2, side // 4), max(3, side // 2)})
    assert len(k) == 3 and k[-1] < side
    two = [(0, 0, k[2], k[2]), (k[2], k[2], bw, bh)]
    four = [(0, 0, k[0], k[0]), (k[0], k[0], k[1], k[1]), (k[1], k[1], k[2], k[2]), (k[2], k[2], bw, bh)]
    return two, four


def join(parts):
    out = parts[0]
    for p in parts[1:]:
        out = layers.union_frame(out, p)
    return out


def frames_of(stream, offs):
    return [stream[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("query", [native.band_levels_workspace_bytes, native.union_levels_workspace_bytes], ids=["band", "union"])
def test_workspace_queries_are_zero_where_the_calls_refuse(query):
    q = query
    assert q(2, 64, 72, 16, 16) == 0            # a frame the tile does not divide
    assert q(2, 64, 64, 8, (12, 16)) == 0       # an MV block that is not a multiple of the tile
    assert q(2, 256, 256, 128, 128) == 0        # a tile of more than 4096 coefficients
    assert q(70000, 64, 64, 8, 16) == 0         # more frames than one call takes
    assert q(2, 64, 64, 8, 16) > 0
    assert q(2, 64, 64, 4, 16) > 0
    assert q(2, 128, 64, 64, 64) > 0
    assert q(2, 36, 24, 12, 12) > 0
    assert q(2, 48, 32, (16, 8), (16, 8)) > 0
    assert q(4, 64, 64, 8, 16) > q(2, 64, 64, 8, 16)
    assert q(2, 64, 64, 8, 16) > native.window_levels_workspace_bytes(2, 64, 64, 8, 16)  # the input pass's arrays, then its own


def test_band_argument_checks_answer_without_a_device():
    """tests/test_window_levels_host.py::test_argument_checks_answer_without_a_device on the band call: every pointer is NULL, each check
    comes before the pointer checks, in the window call's order."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, n_in=2, n_out=2, src=None, ws=1 << 40, cap=1 << 40):
        return lib.svc_hip_band_levels_frames(None, 0, None, n_in, src, n_out, w, h, bw, bh, mbw, mbh, None, None, None, ws, None, cap, None,
                                              None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    some_src = (native.C.c_uint32 * 8)()
    for n in (2, 0):  # the contract does not depend on the frame counts
        assert call(100, 64, 8, 8, 16, 16, n, n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 8, 12, 16, n, n) == bad and "multiple of the tile" in err()
        # geometry before limits
        assert call(100, 64, 8, 8, 16, 16, 70000, 70000) == bad and "not divisible" in err()
        assert call(256, 256, 128, 128, 128, 128, n, n) == unsup and "4096" in err()
        # limits before the d_src rule, for either count
        assert call(64, 64, 8, 8, 16, 16, n, 70000) == unsup and "65535 frames" in err()
        assert call(64, 64, 8, 8, 16, 16, 70000, n, src=some_src) == unsup and "65535 frames" in err()
        assert call(256, 256, 128, 128, 128, 128, n, n + 1) == unsup and "4096" in err()
        # the d_src rule before workspace and capacity
        assert call(64, 64, 8, 8, 16, 16, n, n + 1, ws=0, cap=0) == bad and "d_src" in err()
        assert call(64, 64, 8, 8, 16, 16, n + 3, n, ws=0, cap=0) == bad and "d_src" in err()
    assert call(64, 64, 8, 8, 16, 16, 65535, 65535, ws=0, cap=0) == bad and "workspace" in err()  # the largest counts pass the limits
    need_ws = native.band_levels_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need_out > 0
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0) == bad and "workspace" in err()        # workspace before capacity
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16) == bad and "output" in err()   # capacity before pointers
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
    # the sizes follow n_out, not n_in
    need_ws3 = native.band_levels_workspace_bytes(3, 64, 64, 8, 16)
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3 - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out) == bad and "output" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out // 2 * 3) == bad and "null pointer" in err()
    # an empty batch is valid with sizes of 0, with and without d_src
    assert call(64, 64, 8, 8, 16, 16, 0, 0, ws=0, cap=0) == native.SVC_OK
    assert call(64, 64, 8, 8, 16, 16, 5, 0, src=some_src, ws=0, cap=0) == native.SVC_OK
    assert call(48, 32, 16, 8, 16, 8, 0, 0, ws=0, cap=0) == native.SVC_OK


def test_union_argument_checks_answer_without_a_device():
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, n=2, ws=1 << 40, cap=1 << 40):
        return lib.svc_hip_union_levels_frames(None, 0, None, None, 0, None, n, w, h, bw, bh, mbw, mbh, None, ws, None, cap, None, None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):
        assert call(100, 64, 8, 8, 16, 16, n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 8, 12, 16, n) == bad and "multiple of the tile" in err()
        assert call(100, 64, 8, 8, 16, 16, 70000) == bad and "not divisible" in err()   # geometry before limits
        assert call(256, 256, 128, 128, 128, 128, n) == unsup and "4096" in err()
    assert call(64, 64, 8, 8, 16, 16, 70000, ws=0, cap=0) == unsup and "65535 frames" in err()  # limits before workspace and capacity
    assert call(64, 64, 8, 8, 16, 16, 65535, ws=0, cap=0) == bad and "workspace" in err()
    need_ws = native.union_levels_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need_out > 0
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16) == bad and "output" in err()
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
    assert call(64, 64, 8, 8, 16, 16, 0, ws=0, cap=0) == native.SVC_OK


# ---- the numpy statements -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", sorted(DENSITIES))
@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_ids)
def test_the_statements_identities(geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 31 + h + tile[1] + len(density))
    stream, offs = random_stream(rng, geom, N, DENSITIES[density])
    frames = frames_of(stream, offs)
    two, four = partitions(tile)
    window = (tile[0], 0, max(tile[0], w // 2), h)  # drops the first column of tiles
    for f in frames:
        for bands in (two, four):
            parts = [layers.band_frame(f, b) for b in bands]
            assert join(parts) == f and join(parts[::-1]) == f                                 # the partition joined back, in both orders
            assert sum(levels.parse_frame(p)[0]["level_count"] for p in parts) == levels.parse_frame(f)[0]["level_count"]
            for b in bands:  # band then window equals window then band equals both at once
                both = layers.band_frame(f, b, window)
                assert layers.window_frame(layers.band_frame(f, b), window) == both == layers.band_frame(layers.window_frame(f, window), b)
        # the whole band, however it is said
        for whole in (None, (0, 0, tile[0], tile[1]), (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)):
            assert layers.band_frame(f, whole) == layers.window_frame(f, None) == f
        assert layers.band_frame(f, None, window) == layers.window_frame(f, window)
        # nothing kept: hi == 0, lo == hi, lo > hi
        empty = layers.window_frame(f, (0, 0, 0, 0))
        for none in ((0, 0, 0, 0), (0, 0, tile[0], 0), (3, 3, 3, 3), (5, 5, 2, 2)):
            assert layers.band_frame(f, none) == empty
        lowest = layers.band_frame(f, four[0])
        assert len(lowest) < len(f) if density != "zero" else lowest == f                      # strictly smaller above density 0
        # the reader takes a band as any frame: the kept coefficients, zeros elsewhere
        hdr, types, planes = levels.parse_frame(lowest)
        _, types_f, planes_f = levels.parse_frame(f)
        k = four[0][2]
        inside = ((np.arange(h) % tile[1])[:, None] < k) & ((np.arange(w) % tile[0])[None, :] < k)
        assert np.array_equal(types, types_f) and np.array_equal(planes, np.where(inside[None], planes_f, 0))
    # a batch: a band, a window and a source per output frame
    src = [2, 0, 0, 1]
    bands = [four[0], two[1], None, four[2]]
    bands_arr = [(0, 0, 0xFFFFFFFF, 0xFFFFFFFF) if b is None else b for b in bands]
    windows = [window, (0, 0, w, h), (0, 0, 0, 0), (0, 0, w, tile[1])]
    got, got_offs = layers.band_frames(stream, offs, bands_arr, windows, src)
    want = [layers.band_frame(frames[s], bands[i], windows[i]) for i, s in enumerate(src)]
    assert got == b"".join(want) and [int(o) for o in got_offs] == [0] + list(np.cumsum([len(x) for x in want]))
    assert got_offs.dtype == np.uint64
    got, got_offs = layers.band_frames(stream, offs, None)
    assert got == stream and np.array_equal(got_offs, offs)
    parts = [layers.band_frames(stream, offs, [b] * N) for b in two]
    for first, second in ((0, 1), (1, 0)):
        joined, joined_offs = layers.union_frames(*parts[first], *parts[second])
        assert joined == stream and np.array_equal(joined_offs, offs)
    with pytest.raises(ValueError, match="input frame"):
        layers.band_frames(stream, offs, None, src=[0, N])


def test_a_set_bit_whose_level_is_zero_survives_both_calls():
    geom = GEOMS[1]  # 12 x 12 tiles, 3 mask words each
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(5), geom, 1, 0.5)
    levels_off = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * 3
    b = np.frombuffer(stream, np.uint8).copy()
    count = int(b[40:44].view("<u4")[0])
    assert count > 16
    b[levels_off:levels_off + 32] = 0  # sixteen levels of value 0 whose mask bits stay set
    zeroed = b.tobytes()
    two, four = partitions(tile)
    for bands in (two, four):
        parts = [layers.band_frame(zeroed, band) for band in bands]
        assert sum(int(np.frombuffer(p, np.uint8)[40:44].view("<u4")[0]) for p in parts) == count  # they stay levels in the parts ...
        assert join(parts) == zeroed and join(parts[::-1]) == zeroed                                # ... and in the union
    assert layers.band_frame(zeroed, None) == zeroed


def test_union_refuses_pairs_that_do_not_belong_together():
    geom = GEOMS[4]
    w, h, tile, mv = geom
    rng = np.random.default_rng(9)
    types = random_types(rng, w, h, mv)
    lv = random_levels(rng, w, h, 0.3)
    g = geom_dict(*geom)
    f = layers.write_frame(g, types, lv, 4, 16)
    low, high = layers.band_frame(f, (0, 0, 4, 4)), layers.band_frame(f, (4, 4, 16, 16))
    assert layers.union_frame(low, high) == f
    with pytest.raises(ValueError, match="overlap"):
        layers.union_frame(low, layers.band_frame(f, (3, 4, 16, 16)))  # column 3 of the rows from 4 on is in neither; (r < 4, c = 3) in both
    with pytest.raises(ValueError, match="overlap"):
        layers.union_frame(f, low)
    other_steps = layers.band_frame(layers.write_frame(g, types, lv, 4, 8), (4, 4, 16, 16))
    with pytest.raises(ValueError, match="steps or region ids"):
        layers.union_frame(low, other_steps)
    types2 = types.copy()
    types2.flat[1] ^= 1
    other_types = layers.band_frame(layers.write_frame(g, types2, lv, 4, 16), (4, 4, 16, 16))
    with pytest.raises(ValueError, match="steps or region ids"):
        layers.union_frame(low, other_types)
    other_geom = layers.write_frame(geom_dict(w, h, (8, 8), mv), types, lv, 4, 16)
    with pytest.raises(ValueError, match="geometry"):
        layers.union_frame(low, other_geom)
    bad = np.frombuffer(high, np.uint8).copy()
    bad[0] ^= 1
    with pytest.raises(ValueError):
        layers.union_frame(low, bad)
    with pytest.raises(ValueError):
        layers.band_frame(bad, None)
    with pytest.raises(ValueError, match="numbers of frames"):
        layers.union_frames(*entropy._join([low, low]), *entropy._join([high]))
