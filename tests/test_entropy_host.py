"""The entropy-coded compact stream ("SVCE" v1, include/svc_hip.h) without a GPU: the numpy coder (scalable_video_codec_amd/entropy.py)
round-trips SVCQ frames of the independent writer of tests/test_levels_host.py byte for byte, takes the raw fallback on white noise
within the C ABI's worst case, refuses every malformed frame the GPU decoder flags, and the C ABI's checks answer before any device
work."""
import numpy as np
import pytest

from scalable_video_codec_amd import entropy, levels, native
from tests.test_levels_host import _case, write_frames

GEOMS = [(64, 48, 8, 8, (16, 16)), (64, 64, 16, 16, (16, 16)), (48, 64, 8, 16, (16, 16)), (32, 24, 4, 4, (8, 8)),
         (66, 48, 6, 6, (6, 6)), (128, 64, 64, 64, (64, 64))]


def _sparse(rng, n, w, h, bw, bh, mb, fg, bg, kind="random"):
    """Quantised planes shaped like the codec's: a few levels near DC per tile, most tiles nearly empty."""
    planes, types = _case(rng, n, w, h, bw, bh, mb, fg, bg, kind)
    tiles = planes.reshape(n, 3, h // bh, bh, w // bw, bw)
    keep = np.zeros((bh, bw), bool)
    keep[:3, :3] = True
    tiles *= keep[None, None, None, :, None, :]
    return planes, types


def _round_trip(buf, offs):
    svce, eoffs = entropy.encode_frames(buf, offs)
    assert all(int(o) % 16 == 0 for o in eoffs) and int(eoffs[-1]) == len(svce)
    back, boffs = entropy.decode_frames(svce, eoffs)
    assert back == buf and np.array_equal(boffs, offs)
    return svce, eoffs


@pytest.mark.parametrize("w,h,bw,bh,mb", GEOMS)
@pytest.mark.parametrize("fg,bg", [(1, 640), (3, 17)])
def test_round_trip_is_byte_identical(w, h, bw, bh, mb, fg, bg):
    rng = np.random.default_rng(w + 5 * bw + 7 * bh + fg)
    for kind in ("random", "background", "foreground"):
        planes, types = _sparse(rng, 2, w, h, bw, bh, mb, fg, bg, kind)
        planes[0, 1, :bh, :bw] = 0  # an all-zero tile
        buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], fg, bg)
        svce, _ = _round_trip(buf, offs)
        assert len(svce) < len(buf), kind


def test_dense_levels_and_types_near_two_to_the_32():
    rng = np.random.default_rng(3)
    w, h, bw, bh, mb = 64, 48, 8, 8, (16, 16)
    planes, types = _case(rng, 3, w, h, bw, bh, mb, 3, 17)
    types[0, :] = 0xFFFFFFFF - rng.integers(0, 3, types.shape[1]).astype(np.uint32)
    types[1, ::2] = 0xFFFFFFFF
    buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], 3, 17)
    _round_trip(buf, offs)


def test_all_zero_frame_and_a_single_frame_batch():
    w, h, bw, bh = 64, 48, 8, 8
    planes = np.zeros((1, 3, h, w), np.float32)
    types = np.zeros((1, 12), np.uint32)
    buf, offs = write_frames(planes, types, bw, bh, 16, 16, 1, 640)
    svce, _ = _round_trip(buf, offs)
    hdr, sizes, counts = entropy.parse_frame(svce)
    assert hdr["level_count"] == 0 and (counts == 0).all() and hdr["chunk_tiles"] == entropy.chunk_tiles_for(bw, bh)
    assert len(svce) == 208  # 64 header + 8 types + 18 x 4 index + 18 x 3 (k bits and two 1-bit codes per tile), to 16


def test_short_last_chunk_in_a_row():
    """tiles_x = 33 at chunk_tiles 32: every row ends with a one-tile chunk."""
    rng = np.random.default_rng(9)
    w, h, bw, bh, mb = 33 * 8, 16, 8, 8, (8, 8)
    assert entropy.chunk_tiles_for(bw, bh) == 32
    planes, types = _sparse(rng, 2, w, h, bw, bh, mb, 1, 640)
    buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], 1, 640)
    svce, _ = _round_trip(buf, offs)
    _, sizes, _ = entropy.parse_frame(svce)
    assert sizes.size == 3 * 2 * 2


def test_white_noise_takes_the_raw_fallback_within_the_worst_case():
    rng = np.random.default_rng(5)
    w, h, bw, bh, mb = 64, 32, 8, 8, (16, 16)
    planes = rng.integers(-30000, 30000, (1, 3, h, w)).astype(np.float32)
    types = np.ones((1, (w // 16) * (h // 16)), np.uint32)
    buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], 1, 640)
    svce, _ = _round_trip(buf, offs)
    hdr, sizes, counts = entropy.parse_frame(svce)
    payload = entropy.HEADER_BYTES + hdr["types_bytes"] + 4 * sizes.size
    starts = payload + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    raw = np.frombuffer(svce, np.uint8)[starts] & 1
    assert raw.all()
    assert len(svce) <= _max_bytes(w, h, bw, bh, mb)


def _max_bytes(w, h, bw, bh, mb):
    """include/svc_hip.h's worst case of one frame: SVCQ's + 4 + 5 per chunk, to 16."""
    nw = (bw * bh + 63) // 64
    chunks = 3 * (h // bh) * -(-(w // bw) // entropy.chunk_tiles_for(bw, bh))
    svcq = 64 + 4 * (w // mb[0]) * (h // mb[1]) + 8 * 3 * (w // bw) * (h // bh) * nw + 2 * 3 * w * h
    return (svcq + 4 + 5 * chunks + 15) // 16 * 16


# ---- malformed frames -----------------------------------------------------------------------------------------------------------

def _frame():
    rng = np.random.default_rng(11)
    planes, types = _sparse(rng, 1, 64, 48, 8, 8, (16, 16), 1, 640, "random")
    buf, _ = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    return bytearray(entropy.encode_frame(buf))


def _set_word(b, i, v):
    b[4 * i:4 * i + 4] = int(v).to_bytes(4, "little")


def _word(b, i):
    return int.from_bytes(b[4 * i:4 * i + 4], "little")


def _index_at(b):
    return entropy.HEADER_BYTES + _word(b, 15)


def test_malformed_frames_raise():
    good = _frame()
    entropy.decode_frame(bytes(good))
    cases = {}
    cases["truncated"] = good[:len(good) - 16]
    b = good.copy(); _set_word(b, 0, levels.MAGIC); cases["magic"] = b
    b = good.copy(); _set_word(b, 1, 2); cases["version"] = b
    b = good.copy(); _set_word(b, 14, 0); cases["no tiles per chunk"] = b
    b = good.copy(); _set_word(b, 13, _word(b, 13) + 16); cases["svcq_frame_bytes"] = b
    b = good.copy(); i = _index_at(b); b[i:i + 2] = (int.from_bytes(b[i:i + 2], "little") + 200).to_bytes(2, "little")
    cases["index overruns the payload"] = b
    b = good.copy(); i = _index_at(b); b[i + 2:i + 4] = (int.from_bytes(b[i + 2:i + 4], "little") + 1).to_bytes(2, "little")
    cases["index level counts"] = b
    b = good.copy(); _set_word(b, 10, _word(b, 10) + 1); cases["level_count"] = b
    for what, bad in cases.items():
        with pytest.raises(ValueError):
            entropy.decode_frame(bytes(bad))
        assert what


def test_a_chunk_that_decodes_past_its_end_raises():
    """Move one byte from chunk 0 to chunk 1 in the index: the sums still hold, chunk 0 runs past its size."""
    b = _frame()
    i = _index_at(b)
    e0, e1 = _word(b, i // 4), _word(b, i // 4 + 1)
    assert (e0 & 0xFFFF) > 1
    _set_word(b, i // 4, e0 - 1)
    _set_word(b, i // 4 + 1, e1 + 1)
    entropy.parse_frame(bytes(b))  # the index is consistent with the frame
    with pytest.raises(ValueError, match="chunk"):
        entropy.decode_frame(bytes(b))


def test_malformed_svcq_input_raises_in_the_encoder():
    rng = np.random.default_rng(2)
    planes, types = _sparse(rng, 1, 64, 48, 8, 8, (16, 16), 1, 640)
    buf, _ = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    for word, value in ((0, entropy.MAGIC), (1, 7), (13, 1), (10, 0)):
        b = bytearray(buf)
        _set_word(b, word, value)
        with pytest.raises(ValueError):
            entropy.encode_frame(bytes(b))


# ---- the C ABI's host-side checks ----------------------------------------------------------------------------------------------

def test_max_bytes_and_workspace_answer_without_a_device():
    lib = native.load()
    for (w, h, bw, bh, mb) in GEOMS:
        assert lib.svc_hip_entropy_max_bytes(3, w, h, bw, bh, *mb) == 3 * _max_bytes(w, h, bw, bh, mb)
        assert lib.svc_hip_entropy_workspace_bytes(3, w, h, bw, bh, *mb) > 0
    assert lib.svc_hip_entropy_max_bytes(1, 64, 48, 7, 8, 16, 16) == 0  # tile does not divide the frame
    assert lib.svc_hip_entropy_max_bytes(1, 128, 128, 128, 128, 128, 128) == 0  # tiles above 4096 coefficients
    assert lib.svc_hip_entropy_workspace_bytes(70000, 64, 48, 8, 8, 16, 16) == 0


def test_entry_points_check_geometry_and_sizes_before_pointers():
    lib = native.load()
    enc, dec = lib.svc_hip_entropy_encode_frames, lib.svc_hip_entropy_decode_frames
    big = 1 << 40
    # geometry first, whatever else is wrong
    assert enc(None, 0, None, 1, 64, 48, 7, 8, 16, 16, None, 0, None, 0, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert dec(None, 0, None, 1, 64, 48, 8, 8, 12, 16, None, 0, None, 0, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert enc(None, 0, None, 1, 128, 128, 128, 128, 128, 128, None, big, None, big, None, None, None) == native.SVC_ERR_UNSUPPORTED
    # sizes before pointers
    assert enc(None, 0, None, 2, 64, 48, 8, 8, 16, 16, None, 0, None, big, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert "workspace" in lib.svc_hip_last_error().decode()
    assert enc(None, 0, None, 2, 64, 48, 8, 8, 16, 16, None, big, None, 16, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert "output" in lib.svc_hip_last_error().decode()
    assert dec(None, 0, None, 2, 64, 48, 8, 8, 16, 16, None, big, None, 16, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert "output" in lib.svc_hip_last_error().decode()
    # n == 0: OK once the pointer-free checks pass; then pointers
    assert enc(None, 0, None, 0, 64, 48, 8, 8, 16, 16, None, 0, None, 0, None, None, None) == native.SVC_OK
    assert dec(None, 0, None, 0, 64, 48, 8, 8, 16, 16, None, 0, None, 0, None, None, None) == native.SVC_OK
    assert enc(None, 0, None, 1, 64, 48, 8, 8, 16, 16, None, big, None, big, None, None, None) == native.SVC_ERR_INVALID_ARG
    assert "null" in lib.svc_hip_last_error().decode()
    assert lib.svc_hip_entropy_drain(None, None, 1, 64, 48, 8, 8, 16, 16, None, 16, None) == native.SVC_ERR_INVALID_ARG
    assert "worst case" in lib.svc_hip_last_error().decode()


# ---- any chunk_tiles the header holds --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ct", [1, 7, 8 + 5, 0xFFFFFFFF])
def test_round_trip_at_any_chunk_tiles(ct):
    rng = np.random.default_rng(ct % 1000)
    w, h, bw, bh, mb = 64, 48, 8, 8, (16, 16)
    planes, types = _sparse(rng, 2, w, h, bw, bh, mb, 1, 640)
    buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], 1, 640)
    svce, eoffs = entropy.encode_frames(buf, offs, chunk_tiles=ct)
    hdr, sizes, _ = entropy.parse_frame(svce)
    assert hdr["chunk_tiles"] == ct and sizes.size == 3 * (h // bh) * -(-(w // bw) // ct)
    back, boffs = entropy.decode_frames(svce, eoffs)
    assert back == buf and np.array_equal(boffs, offs)
    with pytest.raises(ValueError):
        entropy.encode_frame(buf, chunk_tiles=0)


def overflowing_chunk_tiles_frame() -> bytes:
    """An all-zero frame claiming chunk_tiles = 2^32 - 1 with no index and no chunks: one chunk per tile row is what that means,
    and their index is missing, so the frame is malformed (a decoder that wraps tiles_x + chunk_tiles - 1 would see no chunks)."""
    buf, _ = write_frames(np.zeros((1, 3, 48, 64), np.float32), np.zeros((1, 12), np.uint32), 8, 8, 16, 16, 1, 640)
    b = bytearray(entropy.encode_frame(buf))
    tb = _word(b, 15)
    b = b[:(64 + tb + 15) // 16 * 16]
    b[64 + tb:] = bytes(len(b) - 64 - tb)
    _set_word(b, 12, len(b))
    _set_word(b, 14, 0xFFFFFFFF)
    return bytes(b)


def width_32_type_overflow_frame() -> bytes:
    """Region ids up to 2^32 - 1 (width 32), with one stored id - 1 rewritten to 2^32 - 1: it would decode to 2^32."""
    planes = np.zeros((1, 3, 48, 64), np.float32)
    types = np.zeros((1, 12), np.uint32)
    types[0, 3] = 0xFFFFFFFF
    types[0, 5] = 7
    buf, _ = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    b = bytearray(entropy.encode_frame(buf))
    assert _word(b, 16) == 32 << 8  # mode 0, width 32; one bitmap word, then the values
    assert _word(b, 18) == 0xFFFFFFFE
    _set_word(b, 18, 0xFFFFFFFF)
    return bytes(b)


def test_overflowing_chunk_tiles_and_type_raise():
    with pytest.raises(ValueError):
        entropy.decode_frame(overflowing_chunk_tiles_frame())
    with pytest.raises(ValueError, match="2\\^32"):
        entropy.decode_frame(width_32_type_overflow_frame())
