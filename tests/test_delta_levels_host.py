"""svc_hip_delta_levels_frames and svc_hip_undelta_levels_frames (include/svc_hip.h: an SVCQ stream coded frame against frame in levels, and
back) without a device: the workspace queries, the order of the argument checks, and the numpy statements
(scalable_video_codec_amd/layers.py: delta_frame, delta_frames, undelta_frame, undelta_frames) on clips built from seeded random levels.
The bytes the kernels write are tests/test_gpu_delta_levels.py, which takes its clips from here."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, native
from tests.test_band_levels_host import frames_of
from tests.test_window_levels_host import geom_dict, random_levels, random_types

# tests/test_gpu_band_levels.py::BAND_GEOMS (that module needs a device to import)
BAND_GEOMS = [
    (36, 12, (4, 4), (12, 12)),      # 16 valid bits per word, the masks only 4-byte aligned
    (36, 24, (12, 12), (12, 12)),    # 3 words per tile, the last partly used
    (272, 24, (8, 8), (16, 8)),      # a group of 32 tiles and one of 2
    (64, 48, (16, 16), (16, 16)),
    (48, 32, (16, 8), (16, 8)),      # a tile that is not square
    (128, 64, (64, 64), (64, 64)),   # 64 words per tile: a group is one tile
    (16, 704, (8, 8), (16, 16)),     # 264 groups: more than one pass of the per-frame scan's workgroup
]
KEYS = [1, 0, 0, 1, 0, 0]
STEPS, OTHER_STEPS, ODD_FRAME = (4, 16), (8, 32), 2  # frame 2's header says other steps: no tile of it, or of frame 3 after it, is predicted


def _gid(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}"


def delta_clip(rng, geom, n=6, density=0.6, steps=STEPS, other=OTHER_STEPS):
    """n frames in which 15 % of the coefficients and 20 % of the MV-block types change from frame to frame (at least one type where there
    are fewer than five blocks), frame ODD_FRAME at other header steps -> (bytes, offsets (n + 1,) u64).  The levels are random_levels':
    the whole int16 range, so differences wrap."""
    w, h, tile, mv = geom
    g = geom_dict(*geom)
    types, lv = random_types(rng, w, h, mv), random_levels(rng, w, h, density)
    frames = []
    for f in range(n):
        if f:
            lv = np.where(rng.random(lv.shape) < 0.15, random_levels(rng, w, h, density), lv)
            flip = rng.random(types.shape) < 0.2
            flip.flat[rng.integers(types.size)] = True
            types = np.where(flip, (types + rng.integers(1, 3, types.shape)) % 3, types).astype(np.uint32)
        frames.append(layers.write_frame(g, types, lv, *(other if f == ODD_FRAME else steps)))
    return entropy._join(frames)


def tile_counts(stream, offs, keys):
    """(predicted, unpredicted) (tile, frame) pairs over the frames that are not key frames, and the coefficients of predicted tiles whose
    difference leaves int16 -- from the frames' sections, not through delta_frame."""
    frames = frames_of(stream, offs)
    predicted = unpredicted = wraps = 0
    for i in range(1, len(frames)):
        if keys is not None and keys[i]:
            continue
        _, _, _, cur, cstep = layers._dense(frames[i])
        _, _, _, prev, pstep = layers._dense(frames[i - 1])
        same = cstep == pstep
        predicted, unpredicted = predicted + int(same.sum()), unpredicted + int((~same).sum())
        d = cur.astype(np.int64) - prev
        wraps += int((((d < -32768) | (d > 32767)) & same[None, :, :, None]).sum())
    return predicted, unpredicted, wraps


@pytest.fixture(scope="module", params=BAND_GEOMS, ids=_gid)
def clip(request):
    geom = request.param
    stream, offs = delta_clip(np.random.default_rng(geom[0] * 3 + geom[1]), geom)
    return geom, stream, offs


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("query", [native.delta_levels_workspace_bytes, native.undelta_levels_workspace_bytes], ids=["delta", "undelta"])
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


@pytest.mark.parametrize("which", ["delta", "undelta"])
def test_argument_checks_answer_without_a_device(which):
    """Every pointer is NULL: each check comes before the pointer checks, in the window call's order -- geometry, limits, workspace,
    output capacity, then n_frames == 0, then pointers."""
    lib = native.load()
    fn = lib.svc_hip_delta_levels_frames if which == "delta" else lib.svc_hip_undelta_levels_frames
    query = native.delta_levels_workspace_bytes if which == "delta" else native.undelta_levels_workspace_bytes

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, n=2, ws=1 << 40, cap=1 << 40):
        return fn(None, 0, None, n, None, 0, None, w, h, bw, bh, mbw, mbh, None, ws, None, cap, None, None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):  # the contract does not depend on the frame count
        assert call(100, 64, 8, 8, 16, 16, n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 8, 12, 16, n) == bad and "multiple of the tile" in err()
        assert call(256, 256, 128, 128, 128, 128, n) == unsup and "4096" in err()
    assert call(100, 64, 8, 8, 16, 16, 70000) == bad and "not divisible" in err()  # geometry before limits
    assert call(64, 64, 8, 8, 16, 16, 70000, ws=0, cap=0) == unsup and "65535 frames" in err()  # limits before the sizes
    assert call(64, 64, 8, 8, 16, 16, 65535, ws=0, cap=0) == bad and "workspace" in err()
    need_ws, need_out = query(2, 64, 64, 8, 16), native.levels_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need_out > 0
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0) == bad and "workspace" in err()       # workspace before capacity
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16) == bad and "output" in err()  # capacity before pointers
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
    assert call(64, 64, 8, 8, 16, 16, 0, ws=0, cap=0) == native.SVC_OK  # an empty batch is valid with sizes of 0
    assert call(48, 32, 16, 8, 16, 8, 0, ws=0, cap=0) == native.SVC_OK


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------------

def test_the_clips_exercise_wrap_around_and_both_kinds_of_tile(clip):
    """Properties 4 and 5, counted from the frames' sections.  A frame of these geometries has 27, 6, 102, 12, 12, 2 and 176 tiles and four
    of a clip's frames have a predecessor, 4 x tiles (tile, frame) pairs: every tile of frame 2 is unpredicted (its header says other
    steps), and the tiles of the three other frames are predicted wherever no region id changed class, which a changed id does about every
    other time -- so at least `tiles` pairs of either kind in every clip, and at least 81 and 27 where half of three frames is 81 tiles
    (a clip of 2 to 27 tiles a frame cannot hold 81 predicted and 27 unpredicted pairs, or only without a change of class)."""
    geom, stream, offs = clip
    w, h, tile, _ = geom
    tiles = (w // tile[0]) * (h // tile[1])
    predicted, unpredicted, wraps = tile_counts(stream, offs, KEYS)
    assert wraps >= 26, wraps
    assert predicted >= tiles and unpredicted >= tiles, (predicted, unpredicted, tiles)
    if 3 * tiles // 2 >= 81:
        assert predicted >= 81 and unpredicted >= 27, (predicted, unpredicted)
    assert unpredicted > tiles or tiles < 3  # region ids that change class, beside the frame at other steps
    # without key flags frame 3 follows the frame at other steps: none of its tiles is predicted either
    assert tile_counts(stream, offs, None)[1] >= 2 * tiles


@pytest.mark.parametrize("keys", [KEYS, None, [0, 0, 1, 1, 0, 1]], ids=["keys", "no-keys", "other-keys"])
def test_undelta_of_delta_is_the_stream(clip, keys):
    """Property 1."""
    geom, stream, offs = clip
    diff, diff_offs = layers.delta_frames(stream, offs, keys)
    assert diff != stream
    back, back_offs = layers.undelta_frames(diff, diff_offs, keys)
    assert back == stream and back_offs.tolist() == [int(o) for o in offs]
    frames, diffs = frames_of(stream, offs), frames_of(diff, diff_offs)
    key = [i == 0 or (keys is not None and keys[i] != 0) for i in range(6)]
    for i in range(6):
        assert diffs[i][:40] == frames[i][:40] and diffs[i][44:48] == frames[i][44:48]  # header words 0 .. 9 and 11
        assert not key[i] or diffs[i] == frames[i]                                       # a key frame is the frame itself
        assert layers._sections(diffs[i])[2].tolist() == layers._sections(frames[i])[2].tolist()
    assert layers.delta_frame(frames[1], frames[0]) == diffs[1] and layers.undelta_frame(diffs[1], frames[0]) == frames[1]


def test_a_call_cut_in_two_gives_the_bytes_of_one(clip):
    """Property 2, at every cut point: prev is the first call's last input frame (delta) or last output frame (undelta)."""
    geom, stream, offs = clip
    frames = frames_of(stream, offs)
    diff, diff_offs = layers.delta_frames(stream, offs, KEYS)
    diffs = frames_of(diff, diff_offs)
    for cut in range(1, 6):
        a, b = entropy._join(frames[:cut]), entropy._join(frames[cut:])
        d0, _ = layers.delta_frames(*a, KEYS[:cut])
        d1, _ = layers.delta_frames(*b, KEYS[cut:], prev=frames[cut - 1])
        assert d0 + d1 == diff, cut
        u0, u0_offs = layers.undelta_frames(*entropy._join(diffs[:cut]), KEYS[:cut])
        u1, _ = layers.undelta_frames(*entropy._join(diffs[cut:]), KEYS[cut:], prev=frames_of(u0, u0_offs)[-1])
        assert u0 + u1 == stream, cut


def test_window_and_band_commute_with_delta(clip):
    """Property 3: a server may store the delta stream and window it."""
    geom, stream, offs = clip
    w, h, tile, _ = geom
    frames = frames_of(stream, offs)
    window = (tile[0], 0, w // 2, h)
    band = (1, 1, max(2, tile[0] // 2), max(2, tile[1] // 2))
    for cur, prev in ((frames[1], frames[0]), (frames[2], frames[1]), (frames[5], frames[4])):
        d = layers.delta_frame(cur, prev)
        assert layers.window_frame(d, window) == layers.delta_frame(layers.window_frame(cur, window), layers.window_frame(prev, window))
        assert layers.band_frame(d, band) == layers.delta_frame(layers.band_frame(cur, band), layers.band_frame(prev, band))
        assert layers.band_frame(d, band, window) == layers.delta_frame(layers.band_frame(cur, band, window), layers.band_frame(prev, band, window))


def with_a_zero_level(frame):
    """The frame with its first level set to 0 under its set bit -> (frame, the same frame as the packers would write it)."""
    b, hdr, types, masks, lv = layers._sections(frame)
    assert lv.size > 2
    bad = np.frombuffer(frame, np.uint8).copy()
    levels_off = 64 + 4 * types.size + masks.size
    bad[levels_off:levels_off + 2] = 0
    _, _, _, vals, _ = layers._dense(bad)
    nz = vals != 0
    clean = layers._assemble(bad[:40].view("<u4"), hdr["inexact"], types, np.packbits(nz, axis=-1, bitorder="little"), vals[nz])
    return bad.tobytes(), clean


@pytest.mark.parametrize("geom", [BAND_GEOMS[0], BAND_GEOMS[3]], ids=_gid)
def test_a_set_bit_of_level_zero_reads_as_zero(geom):
    stream, offs = delta_clip(np.random.default_rng(5), geom, 3)
    f = frames_of(stream, offs)
    bad, clean = with_a_zero_level(f[1])
    assert bad != clean and len(clean) <= len(bad)
    for cur, prev in ((bad, f[0]), (f[2], bad), (bad, None)):
        same = (clean if cur is bad else cur, clean if prev is bad else prev)
        assert layers.delta_frame(cur, prev) == layers.delta_frame(*same)
        assert layers.undelta_frame(cur, prev) == layers.undelta_frame(*same)
    s, o = entropy._join([f[0], bad, f[2]])
    back, _ = layers.undelta_frames(*layers.delta_frames(s, o))
    assert back == f[0] + clean + f[2]  # the stream with that bit cleared


@pytest.mark.parametrize("geom", [BAND_GEOMS[2], BAND_GEOMS[4]], ids=_gid)
def test_with_one_step_every_tile_is_predicted(geom):
    """fg_step == bg_step: the region ids flip, the steps do not -- the difference is the plain difference of the levels."""
    stream, offs = delta_clip(np.random.default_rng(9), geom, 3, steps=(7, 7), other=(7, 7))
    assert tile_counts(stream, offs, None)[1] == 0
    f = frames_of(stream, offs)
    assert layers._sections(f[1])[2].tolist() != layers._sections(f[0])[2].tolist()
    d = layers.delta_frame(f[1], f[0])
    want = (layers._dense(f[1])[3].astype(np.int64) - layers._dense(f[0])[3]).astype(np.uint16).view(np.int16)
    assert np.array_equal(layers._dense(d)[3], want)
    assert layers.undelta_frame(d, f[0]) == f[1]


def test_frames_the_reader_rejects_raise():
    geom = BAND_GEOMS[3]
    stream, offs = delta_clip(np.random.default_rng(2), geom, 2)
    good = frames_of(stream, offs)
    bad = np.frombuffer(good[1], np.uint8).copy()
    bad[0] ^= 1  # the magic
    short = np.frombuffer(good[1], np.uint8).copy()
    short[40:44].view("<u4")[0] -= 1  # the level count
    other, _ = delta_clip(np.random.default_rng(2), BAND_GEOMS[4], 1)
    for fn in (layers.delta_frame, layers.undelta_frame):
        for cur, prev in ((bad, good[0]), (good[0], bad), (short, None), (good[0], short), (good[0], other)):
            with pytest.raises(ValueError):
                fn(cur, prev)
    for fn in (layers.delta_frames, layers.undelta_frames):
        with pytest.raises(ValueError):
            fn(good[0] + bad.tobytes(), offs)
        with pytest.raises(ValueError):
            fn(stream, offs, prev=bad)
        with pytest.raises(ValueError):
            fn(stream, [0, int(offs[1]) - 16, int(offs[2])])
