"""svc_hip_window_entropy_frames (include/svc_hip.h: a stored SVCE stream restricted to a window per output frame, on its coded bytes)
without a device: the numpy statement (scalable_video_codec_amd/entropy.py: window_frame, window_frames) against the three calls it
replaces -- entropy.decode_frame, layers.window_frame, entropy.encode_frame -- the two size queries, and the order of the argument checks.
The bytes the kernels write are tests/test_gpu_window_entropy.py."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native
from tests.test_gpu_window_levels import HOST_GEOMS, _windows_of
from tests.test_window_levels_host import geom_dict, random_levels, random_stream, random_types

N = 4
DENSITY = {"zero": 0.0, "sparse": 0.06, "full": 1.0}


def _ids(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}"


def three_calls(svce, offs, windows, src=None, chunk_tiles=None):
    """The route the call replaces, in numpy: decode every frame, window the SVCQ frames, encode them with the input's chunk_tiles."""
    q, qo = entropy.decode_frames(svce, offs)
    wq, wo = layers.window_frames(q, qo, windows, src)
    if chunk_tiles is None:
        chunk_tiles = int(np.frombuffer(svce, np.uint8)[56:60].view("<u4")[0])
    return entropy.encode_frames(wq, wo, chunk_tiles=chunk_tiles)


def frames_of(stream, offs):
    return [bytes(stream[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]


def chunk_table(frame):
    """-> (geometry, payload start, sizes, counts) of one well-formed SVCE frame."""
    hdr, sizes, counts = entropy.parse_frame(frame)
    g = entropy._Geom(*(hdr[k] for k in ("frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h", "chunk_tiles")))
    start = 64 + hdr["types_bytes"] + 4 * g.chunks + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return g, start, sizes, counts


def empty_chunk(nt):
    """The canonical empty chunk of nt tiles: 7 zero bits (coded, k_dc = k_ac = 0), then two 1 bits per tile."""
    bits = np.zeros((7 + 2 * nt + 7) // 8 * 8, bool)
    bits[7:7 + 2 * nt] = True
    return np.packbits(bits, bitorder="little").tobytes()


# ---- the statement against the three calls it replaces --------------------------------------------------------------------------------

@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("geom", HOST_GEOMS, ids=_ids)
def test_canonical_streams_equal_the_three_call_route(geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    seen = np.zeros(3, np.int64)
    for windows in _windows_of(geom):
        stream, offs = random_stream(rng, geom, N, DENSITY[density])
        svce, so = entropy.encode_frames(stream, offs)
        got, got_offs = entropy.window_frames(svce, so, windows)
        want, want_offs = three_calls(svce, so, windows)
        assert got == want and np.array_equal(got_offs, want_offs) and got_offs.dtype == np.uint64
        src_frames, out_frames = frames_of(svce, so), frames_of(got, got_offs)
        for i in range(N):
            cls = entropy.chunk_classes(src_frames[i], None if windows is None else windows[i])
            seen += np.bincount(cls, minlength=3)
            # a dropped chunk is the constant; a kept chunk its input's bytes and entry; the header as stated
            g, start, sizes, counts = chunk_table(out_frames[i])
            gi, start_i, sizes_i, counts_i = chunk_table(src_frames[i])
            out = np.frombuffer(out_frames[i], np.uint8)
            src = np.frombuffer(src_frames[i], np.uint8)
            for c in range(g.chunks):
                pay = out[start[c]:start[c] + sizes[c]].tobytes()
                if cls[c] == 1:
                    assert pay == empty_chunk(int(g.chunk_nt[c])) and counts[c] == 0
                elif cls[c] == 0:
                    assert pay == src[start_i[c]:start_i[c] + sizes_i[c]].tobytes() and counts[c] == counts_i[c]
            ho, hi_ = out[:64].view("<u4"), src[:64].view("<u4")
            for k in list(range(10)) + [11, 14, 15]:
                assert ho[k] == hi_[k]
            assert ho[10] == counts.sum() and ho[12] == len(out_frames[i]) and ho[13] == (g.levels_off + 2 * int(ho[10]) + 15) // 16 * 16
            assert not out[start[-1] + sizes[-1]:].any() and len(out_frames[i]) % 16 == 0
    # every class of chunk occurred, in every geometry that can have it (a chunk of one tile cannot be cut)
    one_tile_chunks = entropy.chunk_tiles_for(*tile) == 1 or w // tile[0] == 1
    assert seen[0] > 0 and seen[1] > 0 and (seen[2] > 0 or one_tile_chunks), seen


@pytest.mark.parametrize("geom", HOST_GEOMS[:3] + HOST_GEOMS[6:], ids=_ids)
def test_foreign_but_legal_inputs_decode_to_the_windowed_frame(geom):
    """force_k inputs are not canonical, so the output is not the three-call route's bytes: kept chunks stay as they are.  It decodes to
    the windowed SVCQ frame, cut chunks come out canonical, and any chunk_tiles is honoured."""
    w, h, tile, mv = geom
    rng = np.random.default_rng(w + h)
    tx = w // tile[0]
    stream, offs = random_stream(rng, geom, N, 0.06)
    q_frames = frames_of(stream, offs)
    for windows in _windows_of(geom)[4:8]:
        for force_k in ((0, 0), (7, 7), (3, 5)):
            for i in range(N):
                f = entropy.encode_frame(q_frames[i], force_k=force_k)
                out = entropy.window_frame(f, windows[i])
                assert entropy.decode_frame(out) == layers.window_frame(q_frames[i], windows[i])
                canon = entropy.encode_frame(layers.window_frame(q_frames[i], windows[i]))
                cls = entropy.chunk_classes(f, windows[i])
                g, start, sizes, counts = chunk_table(out)
                gc, start_c, sizes_c, _ = chunk_table(canon)
                for c in np.flatnonzero(cls != 0):  # cut and dropped chunks are the canonical encoder's
                    assert out[start[c]:start[c] + sizes[c]] == canon[start_c[c]:start_c[c] + sizes_c[c]]
        for ct in (1, 3, 5, tx, tx + 1):
            svce, so = entropy.encode_frames(stream, offs, chunk_tiles=ct)
            got, got_offs = entropy.window_frames(svce, so, windows)
            want, want_offs = three_calls(svce, so, windows, chunk_tiles=ct)
            assert got == want and np.array_equal(got_offs, want_offs)


def test_a_zero_level_under_a_set_bit_stays_and_forces_raw():
    geom = HOST_GEOMS[2]  # 272 x 24 at 8 x 8: chunks of 32 and of 2 tiles
    w, h, tile, mv = geom
    rng = np.random.default_rng(9)
    lv = random_levels(rng, w, h, 0.06)
    lv[0, 0, 8 * 5 + 3] = 1     # tile 5 of the first row: kept
    lv[0, 0, 8 * 20 + 3] = 1    # tile 20: dropped, in the cut chunk
    lv[0, 8, 8 * 33 + 3] = 1    # second tile row, tile 33 (the short chunk): dropped whole
    frame = np.frombuffer(layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), lv, 4, 16), np.uint8).copy()
    # zero those three levels in place: their mask bits stay set
    hdr, _, _ = levels.parse_frame(frame)
    lo = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // 8) * (h // 8)
    levels16 = frame[lo:lo + 2 * hdr["level_count"]].view("<i2")
    ones = np.flatnonzero(levels16 == 1)
    assert ones.size >= 3
    levels16[ones] = 0
    frame = frame.tobytes()
    svce = entropy.encode_frame(frame)
    window = (0, 0, 8 * 12, h)  # tiles 0 .. 11: the first chunk of every row is cut, the second dropped
    out = entropy.window_frame(svce, window)
    assert out == entropy.encode_frame(layers.window_frame(frame, window))
    assert entropy.decode_frame(out) == layers.window_frame(frame, window)
    g, start, sizes, counts = chunk_table(out)
    assert out[start[0]] & 1  # the cut chunk that keeps a zero level is raw
    whole = entropy.window_frame(svce, None)
    assert whole == svce


def test_refusals_of_the_statement():
    geom = HOST_GEOMS[0]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(2), geom, 2, 0.3)
    svce, so = entropy.encode_frames(stream, offs)
    with pytest.raises(ValueError, match="input frame"):
        entropy.window_frames(svce, so, None, src=[0, 2])
    got, got_offs = entropy.window_frames(svce, so, None, src=[1, 1, 0])
    fr = frames_of(svce, so)
    assert got == fr[1] + fr[1] + fr[0] and [int(o) for o in got_offs] == [0, len(fr[1]), 2 * len(fr[1]), len(got)]
    for word, value in ((0, 0x12345678), (1, 2), (2, w + 4), (14, 0), (12, len(fr[0]) + 16), (13, 16), (15, 2), (10, 0xFFFF)):
        bad = np.frombuffer(fr[0], np.uint8).copy()
        bad[4 * word:4 * word + 4].view("<u4")[0] = value
        with pytest.raises(ValueError):
            entropy.window_frame(bad, None)
    # a chunk_tiles whose raw chunk does not fit the index's u16: refused whatever the window
    big = (512, 64, (64, 64), (64, 64))
    stream, offs = random_stream(np.random.default_rng(3), big, 1, 0.001)
    f8 = entropy.encode_frame(stream, chunk_tiles=8)
    assert entropy.decode_frame(f8) == stream
    with pytest.raises(ValueError, match="u16"):
        entropy.window_frame(f8, None)
    assert entropy.window_frame(entropy.encode_frame(stream, chunk_tiles=7), (64, 0, 128, 64))


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def test_queries_are_zero_where_the_call_refuses():
    for q in (native.window_entropy_max_bytes, native.window_entropy_workspace_bytes):
        assert q(2, 64, 72, 16, 16) == 0            # a frame the tile does not divide
        assert q(2, 64, 64, 8, (12, 16)) == 0       # an MV block that is not a multiple of the tile
        assert q(2, 256, 256, 128, 128) == 0        # a tile of more than 4096 coefficients
        assert q(70000, 64, 64, 8, 16) == 0         # more frames than one call takes
        assert q(2, 64, 64, 8, 16) > 0
        assert q(2, 128, 64, 64, 64) > 0
        assert q(2, 36, 24, 12, 12) > 0
        assert q(4, 64, 64, 8, 16) == 2 * q(2, 64, 64, 8, 16) or q is native.window_entropy_workspace_bytes
        assert q(4, 64, 64, 8, 16) > q(2, 64, 64, 8, 16)
    assert native.window_entropy_workspace_bytes(0, 64, 64, 8, 16) == 0 == native.window_entropy_max_bytes(0, 64, 64, 8, 16)
    # the worst canonical frame with a chunk per tile: SVCQ's worst case, the types' mode word, 5 bytes per tile and plane
    w, h, tile, mv = 272, 24, 8, (16, 8)
    levels_off = 64 + 4 * (w // 16) * (h // 8) + 8 * 3 * (w // 8) * (h // 8)
    assert native.window_entropy_max_bytes(3, w, h, tile, mv) == 3 * ((levels_off + 6 * w * h + 4 + 5 * 3 * (w // 8) * (h // 8) + 15) // 16 * 16)
    assert native.window_entropy_max_bytes(3, w, h, tile, mv) >= native.entropy_max_bytes(3, w, h, tile, mv)


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: each check below comes before the pointer checks, and the null-pointer check stands between all of them
    and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, bw, bh, mbw, mbh, n_in=2, n_out=2, src=None, ws=1 << 40, cap=1 << 40):
        return lib.svc_hip_window_entropy_frames(None, 0, None, n_in, src, n_out, w, h, bw, bh, mbw, mbh, None, None, ws, None, cap, None,
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
    assert call(64, 64, 8, 8, 16, 16, 65535, 65535, ws=0, cap=0) == bad and "workspace" in err()
    need_ws = native.window_entropy_workspace_bytes(2, 64, 64, 8, 16)
    need_out = native.window_entropy_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need_out > 0
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0) == bad and "workspace" in err()        # workspace before capacity
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16) == bad and "output" in err()   # capacity before pointers
    assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
    # the sizes follow n_out, not n_in
    need_ws3 = native.window_entropy_workspace_bytes(3, 64, 64, 8, 16)
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3 - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out) == bad and "output" in err()
    assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out // 2 * 3) == bad and "null pointer" in err()
    # an empty batch is valid with sizes of 0, with and without d_src
    assert call(64, 64, 8, 8, 16, 16, 0, 0, ws=0, cap=0) == native.SVC_OK
    assert call(64, 64, 8, 8, 16, 16, 5, 0, src=some_src, ws=0, cap=0) == native.SVC_OK
    assert call(36, 24, 12, 12, 12, 12, 0, 0, ws=0, cap=0) == native.SVC_OK


def test_the_abi_version_did_not_move():
    assert native.load().svc_hip_abi_version() == 5
