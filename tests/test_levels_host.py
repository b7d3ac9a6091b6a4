"""The compact quantised-coefficient stream ("SVCQ" v1, include/svc_hip.h) without a GPU: an independent numpy writer of the format
against the host reader (scalable_video_codec_amd/levels.py), the worst-case size against its formula, and the argument checks of the
C ABI that answer before any device work."""

import numpy as np
import pytest

from scalable_video_codec_amd import levels, native


def _round_half_away(q):
    q = np.asarray(q, np.float64)
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def write_frame(planes, types, bw, bh, mbw, mbh, fg, bg) -> bytes:
    """One frame of the format, written the plain way: tile by tile, coefficient by coefficient order via reshapes."""
    planes = np.asarray(planes, np.float32)
    _, h, w = planes.shape
    mfw, mfh = w // mbw, h // mbh
    types = np.asarray(types, np.uint32).reshape(mfh, mfw)
    tx, ty, area = w // bw, h // bh, bw * bh
    nw = (area + 63) // 64
    tiles = planes.reshape(3, ty, bh, tx, bw).transpose(0, 1, 3, 2, 4).reshape(3, ty, tx, area)
    tile_type = np.array([[types[(y * bh) // mbh, (x * bw) // mbw] for x in range(tx)] for y in range(ty)])
    step = np.where(tile_type == 0, np.float32(bg), np.float32(fg)).astype(np.float32)[None, :, :, None]
    lv = np.clip(_round_half_away(tiles / step), -32768, 32767).astype(np.int16)  # f32 division, as the quantiser
    inexact = int(np.count_nonzero(tiles != lv.astype(np.float32) * step))
    nz = lv != 0
    bits = np.zeros((3, ty, tx, nw * 64), bool)
    bits[..., :area] = nz
    masks = np.packbits(bits, axis=-1, bitorder="little").reshape(3, ty, tx, nw * 8)
    lev = lv[nz]
    body = types.astype("<u4").tobytes() + masks.tobytes() + lev.astype("<i2").tobytes()
    size = (64 + len(body) + 15) // 16 * 16
    hdr = np.array([0x51435653, 1, w, h, bw, bh, mbw, mbh, fg, bg, lev.size, inexact, size, 0, 0, 0], "<u4").tobytes()
    return hdr + body + bytes(size - 64 - len(body))


def write_frames(planes, types, bw, bh, mbw, mbh, fg, bg):
    """n frames back to back -> (bytes, offsets (n + 1,) u64)."""
    chunks = [write_frame(p, t, bw, bh, mbw, mbh, fg, bg) for p, t in zip(planes, types)]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    return b"".join(chunks), offs


def _case(rng, n, w, h, bw, bh, mb, fg, bg, kind="random"):
    """Quantised planes (level * step in f32) with the region ids they were quantised with."""
    mfw, mfh = w // mb[0], h // mb[1]
    if kind == "background":
        types = np.zeros((n, mfh * mfw), np.uint32)
    elif kind == "foreground":
        types = rng.integers(1, 5, (n, mfh * mfw)).astype(np.uint32)
    else:
        types = (rng.random((n, mfh * mfw)) < 0.3).astype(np.uint32) * rng.integers(1, 4, (n, mfh * mfw)).astype(np.uint32)
    planes = np.zeros((n, 3, h, w), np.float32)
    for f in range(n):
        t = types[f].reshape(mfh, mfw)
        step = np.where(np.repeat(np.repeat(t, mb[1], 0), mb[0], 1) == 0, np.float32(bg), np.float32(fg)).astype(np.float32)
        lv = rng.integers(-40, 41, (3, h, w)) * (rng.random((3, h, w)) < 0.2)
        planes[f] = lv.astype(np.float32) * step[None]
    return planes, types


def _expected_planes(planes):
    return planes + np.float32(0)  # -0.0 decodes as +0.0: equal as numbers


@pytest.mark.parametrize("w,h,bw,bh,mb", [(64, 48, 8, 8, (16, 16)), (64, 64, 16, 16, (16, 16)), (48, 64, 8, 16, (16, 16)),
                                          (32, 24, 4, 4, (8, 8)), (96, 32, 8, 8, (32, 16)), (66, 48, 6, 6, (6, 6))])
@pytest.mark.parametrize("fg,bg", [(1, 640), (3, 17)])
def test_reader_against_independent_writer(w, h, bw, bh, mb, fg, bg):
    rng = np.random.default_rng(w * 7 + bw * 3 + bh + fg)
    planes, types = _case(rng, 3, w, h, bw, bh, mb, fg, bg)
    planes[0, 1, 0, 0] = -0.0
    planes[1, :, :bh, :bw] = 0  # an all-zero tile in every plane
    buf, offs = write_frames(planes, types, bw, bh, mb[0], mb[1], fg, bg)
    assert all(int(o) % 16 == 0 for o in offs) and int(offs[-1]) == len(buf)
    got = list(levels.iter_frames(np.frombuffer(buf, np.uint8), offs))
    assert len(got) == 3
    for f, (hdr, t, p) in enumerate(got):
        nz = int(np.count_nonzero(planes[f]))
        assert hdr == dict(magic=0x51435653, version=1, frame_w=w, frame_h=h, block_w=bw, block_h=bh, mv_block_w=mb[0],
                           mv_block_h=mb[1], fg_step=fg, bg_step=bg, level_count=nz, inexact=0,
                           frame_bytes=int(offs[f + 1] - offs[f]))
        assert np.array_equal(t.reshape(-1), types[f])
        assert p.dtype == np.float32 and np.array_equal(p, _expected_planes(planes[f]))
        assert not np.signbit(p[1, 0, 0]) if f == 0 else True
        used = 64 + 4 * types[f].size + 8 * 3 * (w // bw) * (h // bh) * ((bw * bh + 63) // 64) + 2 * nz
        assert hdr["frame_bytes"] == (used + 15) // 16 * 16
        assert buf[int(offs[f]) + used:int(offs[f + 1])] == bytes(hdr["frame_bytes"] - used)  # zero padding


def test_fully_nonzero_tiles_and_inexact_count():
    rng = np.random.default_rng(5)
    w, h, bw, bh = 32, 16, 8, 8
    types = np.array([0, 1], np.uint32)  # mv blocks 16 x 16: left background, right foreground
    lv = rng.integers(1, 30, (3, h, w)) * rng.choice([-1, 1], (3, h, w))
    step = np.where(np.arange(w)[None, None, :] < 16, 640, 1).astype(np.float32)
    planes = lv.astype(np.float32) * step
    hdr, t, p = levels.parse_frame(write_frame(planes, types, bw, bh, 16, 16, 1, 640))
    assert hdr["level_count"] == 3 * h * w and hdr["inexact"] == 0 and np.array_equal(p, planes)
    raw = planes + np.float32(0.25)  # raw coefficients: not multiples of the step
    hdr, _, p = levels.parse_frame(write_frame(raw, types, bw, bh, 16, 16, 1, 640))
    assert hdr["inexact"] == int(np.count_nonzero(raw != p))


def test_reader_rejects_bad_frames():
    rng = np.random.default_rng(9)
    planes, types = _case(rng, 2, 32, 32, 8, 8, (16, 16), 1, 640)
    buf, offs = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    one = bytearray(buf[:int(offs[1])])
    levels.parse_frame(bytes(one))
    bad = bytearray(one); bad[0] ^= 1
    with pytest.raises(ValueError, match="magic"):
        levels.parse_frame(bytes(bad))
    bad = bytearray(one); bad[4] = 2
    with pytest.raises(ValueError, match="version"):
        levels.parse_frame(bytes(bad))
    with pytest.raises(ValueError, match="truncated"):
        levels.parse_frame(bytes(one[:40]))
    with pytest.raises(ValueError, match="truncated"):
        levels.parse_frame(bytes(one[:-16]))
    with pytest.raises(ValueError, match="truncated"):
        list(levels.iter_frames(buf[:-16], offs))


def test_reader_rejects_mask_bits_past_the_tile():
    """6x6 tiles use bits 0-35 of their one mask word; the format keeps bits 36-63 at 0."""
    rng = np.random.default_rng(12)
    planes, types = _case(rng, 1, 36, 24, 6, 6, (6, 6), 1, 640)
    frame = bytearray(write_frame(planes[0], types[0], 6, 6, 6, 6, 1, 640))
    levels.parse_frame(bytes(frame))
    masks_off = 64 + 4 * types[0].size
    frame[masks_off + 5] |= 0x01  # bit 40 of the first tile's word
    with pytest.raises(ValueError, match="past the tile"):
        levels.parse_frame(bytes(frame))


def _formula(n, w, h, bw, bh, mbw, mbh):
    per = 64 + 4 * (w // mbw) * (h // mbh) + 8 * 3 * (w // bw) * (h // bh) * ((bw * bh + 63) // 64) + 2 * 3 * w * h
    return n * ((per + 15) // 16 * 16)


@pytest.mark.parametrize("geom", [(16, 1920, 1088, 8, 8, 16, 16), (1, 3840, 2160, 16, 16, 16, 16), (5, 160, 96, 8, 16, 16, 16),
                                  (3, 48, 40, 4, 4, 8, 8), (2, 40, 24, 8, 8, 8, 8)])
def test_levels_max_bytes_formula(geom):
    assert native.levels_max_bytes(geom[0], geom[1], geom[2], geom[3:5], geom[5:7]) == _formula(*geom)
    if geom[1:3] == (1920, 1088):
        assert _formula(*geom) / 16 < 1920 * 1088 * 3 * 4  # less than the f32 planes it replaces (about 13.35 MB per C3 frame)


def test_levels_max_bytes_is_zero_where_the_pack_refuses():
    assert native.levels_max_bytes(2, 64, 64, 8, (12, 16)) == 0  # MV block not a multiple of the tile
    assert native.levels_max_bytes(2, 100, 64, 8, 4) == 0  # frame not a multiple of the tile
    assert native.levels_max_bytes(1, 512, 512, 128, 128) == 0  # tiles above 4096 coefficients
    assert native.pack_levels_workspace_bytes(1, 512, 512, 128) == 0


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, and the null-pointer check stands between any
    of them and a launch -- a missing or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def pack(w, h, bw, bh, mbw, mbh, fg, bg, n=2, ws=1 << 30, cap=1 << 40):
        return lib.svc_hip_pack_levels_frames(None, None, n, w, h, bw, bh, mbw, mbh, fg, bg, None, ws, None, cap, None, None)
    assert pack(100, 64, 8, 8, 16, 16, 1, 640) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
    assert pack(64, 64, 8, 8, 12, 16, 1, 640) == native.SVC_ERR_INVALID_ARG and "multiple of the tile" in err()
    assert pack(64, 64, 8, 8, 16, 16, 0, 640) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    assert pack(64, 64, 8, 8, 16, 16, 1, 0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    # the same answers for an empty batch: the contract does not depend on n_frames
    assert pack(100, 64, 8, 8, 16, 16, 1, 640, n=0) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
    assert pack(64, 64, 8, 8, 16, 16, 0, 640, n=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    assert pack(64, 64, 8, 8, 16, 16, 1, 640, n=0) == native.SVC_OK
    # 255 * sqrt(256 * 256) / 1 = 65280 > 32767: a level could leave int16
    assert pack(512, 512, 256, 256, 256, 256, 1, 640) == native.SVC_ERR_UNSUPPORTED and "int16" in err()
    assert pack(512, 512, 128, 128, 128, 128, 1, 640) == native.SVC_ERR_UNSUPPORTED and "4096 coefficients" in err()
    assert pack(64, 64, 8, 8, 16, 16, 1, 640, ws=0) == native.SVC_ERR_INVALID_ARG and "workspace" in err()
    assert pack(64, 64, 8, 8, 16, 16, 1, 640, cap=16) == native.SVC_ERR_INVALID_ARG and "worst case" in err()
    assert pack(64, 64, 8, 8, 16, 16, 1, 640) == native.SVC_ERR_INVALID_ARG and "null pointer" in err()

    def unpack(w, h, mbw, mbh, ws=1 << 30):
        return lib.svc_hip_unpack_levels_frames(None, 1 << 20, None, 2, w, h, 8, 8, mbw, mbh, None, ws, None, None, None, None)
    assert unpack(64, 56, 16, 16) == native.SVC_ERR_INVALID_ARG and "divide the frame" in err()
    assert unpack(64, 64, 16, 16, ws=0) == native.SVC_ERR_INVALID_ARG and "workspace" in err()
    assert unpack(64, 64, 16, 16) == native.SVC_ERR_INVALID_ARG and "null pointer" in err()

    # the drain: a destination below the batch's worst case is refused before any pointer is looked at
    need = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert lib.svc_hip_levels_drain(None, None, 2, 64, 64, 8, 8, 16, 16, None, need - 16, None) == native.SVC_ERR_INVALID_ARG
    assert "worst case" in err()
    assert lib.svc_hip_levels_drain(None, None, 2, 64, 64, 8, 8, 16, 16, None, need, None) == native.SVC_ERR_INVALID_ARG
    assert "null pointer" in err()
