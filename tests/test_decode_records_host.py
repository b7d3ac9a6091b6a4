"""The decoder of the reference's wire stream without a GPU: the argument checks of svc_hip_decode_records_frames, which answer in
their stated order before any device work, and svc_hip_wire_layout's reading of a whole stream (the decoder's padded tile grid or the
reference encoder's unpadded loops), against svc_hip_wire_header + svc_hip_serialized_frame_bytes and the numpy reader."""
import struct

import pytest

from scalable_video_codec_amd import native, wire


def _decode(lib, w, h, block, emit_h=None, fg=1, bg=640, dw=0, dh=0, stride=None, n=2):
    emit_h = h if emit_h is None else emit_h
    if stride is None:
        stride = native.serialized_frame_bytes(w, emit_h, block, block)
    return lib.svc_hip_decode_records_frames(None, stride, n, w, h, block, emit_h, fg, bg, None, None, None, dw, dh, None)


@pytest.mark.parametrize("n", [0, 3])
def test_decode_records_argument_checks_answer_in_order_without_a_device(n):
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    # 1. geometry: tiles other than 8x8 / 16x16 and widths that are not whole 16-pixel segments (as svc_hip_decode_frames)
    for b in (4, 12, 32):
        assert _decode(lib, 96, 96, b, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in err()
    assert _decode(lib, 72, 64, 8, n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in err()
    assert _decode(lib, 64, 60, 8, n=n) == native.SVC_ERR_INVALID_ARG and "not divisible" in err()
    assert _decode(lib, 64, 64, 8, emit_h=0, stride=772, n=n) == native.SVC_ERR_INVALID_ARG and "emit_frame_h" in err()
    assert _decode(lib, 64, 64, 8, emit_h=65, n=n) == native.SVC_ERR_INVALID_ARG and "emit_frame_h" in err()
    # geometry comes before everything else
    assert _decode(lib, 72, 64, 8, fg=0, dw=99, dh=1, stride=1, n=n) == native.SVC_ERR_UNSUPPORTED
    # 2. steps of 0 (the reference's Validate(DecoderConfig&)), before display size and stride
    assert _decode(lib, 64, 64, 8, fg=0, dw=99, dh=1, stride=1, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    assert _decode(lib, 64, 64, 8, bg=0, n=n) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in err()
    # 3. display sizes outside 1 .. padded, before the stride
    assert _decode(lib, 64, 64, 8, dw=65, dh=64, stride=1, n=n) == native.SVC_ERR_INVALID_ARG and "display" in err()
    assert _decode(lib, 64, 64, 8, dw=64, dh=65, n=n) == native.SVC_ERR_INVALID_ARG and "display" in err()
    assert _decode(lib, 64, 64, 8, dw=0, dh=32, n=n) == native.SVC_ERR_INVALID_ARG and "display" in err()
    # 4. stride: at least one frame of the emitted rows, a multiple of 4
    per = native.serialized_frame_bytes(64, 56, 8, 8)
    assert _decode(lib, 64, 64, 8, emit_h=56, stride=per - 4, n=n) == native.SVC_ERR_INVALID_ARG and "stride" in err()
    assert _decode(lib, 64, 64, 8, emit_h=56, stride=per + 2, n=n) == native.SVC_ERR_INVALID_ARG and "stride" in err()
    assert _decode(lib, 64, 64, 16, stride=native.serialized_frame_bytes(64, 64, 16, 16) - 4, n=n) == native.SVC_ERR_INVALID_ARG
    # 5. pointers, only for a batch that is not empty
    want = native.SVC_OK if n == 0 else native.SVC_ERR_INVALID_ARG
    assert _decode(lib, 64, 64, 8, emit_h=56, stride=per, n=n) == want
    assert _decode(lib, 64, 64, 16, emit_h=1, dw=48, dh=40, n=n) == want
    assert _decode(lib, 1920, 1088, 8, emit_h=1080, dw=1920, dh=1080, n=n) == want
    if n:
        assert "null pointer" in err()


def _layout(hdr: bytes, nbytes: int):
    return native.wire_layout(hdr, nbytes)


def _refused(hdr: bytes, nbytes: int, status=native.SVC_ERR_INVALID_ARG) -> str:
    with pytest.raises(native.SvcError) as e:
        native.wire_layout(hdr, nbytes)
    assert e.value.status == status
    return str(e.value)


def _hdr(**kw) -> bytes:
    d = dict(frame_count=4, frame_w=1920, frame_h=1080, frame_excess_w=0, frame_excess_h=8, transform_block_w=8, transform_block_h=8,
             channel_count=3)
    d.update(kw)
    return struct.pack("<8I", *(d[k] for k in wire.FIELDS))


def test_wire_layout_both_readings_at_1080p():
    hdr = native.wire_header(5, 1920, 1080, 16, 3, 8)
    assert hdr == _hdr()
    rec8 = 4 + 12 * 64
    # the decoder's reading: 240 x 136 tiles; the reference encoder's: its unpadded loops emit 135 tile rows
    assert _layout(hdr, 32 + 4 * 240 * 136 * rec8) == (1088, 240 * 136 * rec8)
    assert _layout(hdr, 32 + 4 * 240 * 135 * rec8) == (1080, 240 * 135 * rec8)
    # 16 x 16 tiles: 68 tile rows either way, the decoder's reading (the padded height)
    hdr16 = native.wire_header(5, 1920, 1080, 16, 3, 16)
    rec16 = 4 + 12 * 256
    assert _layout(hdr16, 32 + 4 * 120 * 68 * rec16) == (1088, 120 * 68 * rec16)
    # the numpy reader says the same
    h = wire.parse_header(hdr)
    assert wire.layout(h, 32 + 4 * 240 * 135 * rec8) == (1080, 240 * 135 * rec8)
    assert wire.layout(wire.parse_header(hdr16), 32 + 4 * 120 * 68 * rec16) == (1088, 120 * 68 * rec16)


def test_wire_layout_readings_that_coincide_and_empty_streams():
    hdr = native.wire_header(9, 320, 208, 16, 3, 8)  # no padding: one reading
    per = 40 * 26 * 772
    assert _layout(hdr, 32 + 8 * per) == (208, per)
    # 1080p with 8x8 tiles but no frames: both readings are the header alone, the decoder's wins
    assert _layout(native.wire_header(1, 1920, 1080, 16, 3, 8), 32) == (1088, 240 * 136 * 772)


def test_wire_layout_refusals():
    # the reference encoder's reading of a frame padded in width: its unpadded row stride has scrambled the coefficients
    hdr = native.wire_header(4, 344, 280, 16, 4, 8)
    h = wire.parse_header(hdr)
    assert h["frame_excess_w"] == 8 and h["frame_excess_h"] == 8
    enc = native.serialized_frame_bytes(344, 280, 8, 8)  # 43 x 35 tiles against 44 x 36
    dec = native.serialized_frame_bytes(352, 288, 8, 8)
    assert enc != dec
    assert "scrambled" in _refused(hdr, 32 + 3 * enc)
    assert _layout(hdr, 32 + 3 * dec) == (288, dec)
    # truncated or overlong
    hdr = _hdr()
    per = 240 * 136 * 772
    for nbytes in (0, 31, 32, 33, 32 + 4 * per - 1, 32 + 4 * per + 1, 32 + 4 * per + 772, 32 + 3 * per, 32 + 5 * per):
        msg = _refused(hdr, nbytes)
        assert "truncated or overlong" in msg or nbytes < 32
    # channel count, tiles
    assert "channel_count" in _refused(_hdr(channel_count=1), 32 + 4 * per)
    assert "non-square" in _refused(_hdr(transform_block_h=16), 32, native.SVC_ERR_UNSUPPORTED)
    assert "8x8, 16x16" in _refused(_hdr(transform_block_w=4, transform_block_h=4), 32, native.SVC_ERR_UNSUPPORTED)
    assert "8x8, 16x16" in _refused(_hdr(transform_block_w=0, transform_block_h=0), 32, native.SVC_ERR_UNSUPPORTED)
    # a padded width the decoder does not take
    assert "16-pixel" in _refused(_hdr(frame_w=360, frame_excess_w=0), 32, native.SVC_ERR_UNSUPPORTED)
    with pytest.raises(native.SvcError):
        native.wire_layout(_hdr(frame_w=0), 32)


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
@pytest.mark.parametrize("mv_block", [16, 32])
def test_wire_layout_agrees_with_header_and_frame_bytes(block, levels, mv_block):
    if mv_block < block:
        return
    for w, h in [(1920, 1080), (1280, 720), (720, 576), (344, 280), (320, 200), (320, 208), (176, 144), (100, 70), (16, 8), (1000, 997)]:
        for clip_frames in (1, 2, 7):
            hdr = native.wire_header(clip_frames, w, h, mv_block, levels, block)
            d = wire.parse_header(hdr)
            pw, ph = w + d["frame_excess_w"], h + d["frame_excess_h"]
            n = clip_frames - 1
            dec = native.serialized_frame_bytes(pw, ph, block, block)
            enc = native.serialized_frame_bytes(w, h, block, block)
            assert _layout(hdr, 32 + n * dec) == (ph, dec) == wire.layout(d, 32 + n * dec)
            if n and enc != dec:
                if d["frame_excess_w"]:
                    assert "scrambled" in _refused(hdr, 32 + n * enc)
                else:
                    assert _layout(hdr, 32 + n * enc) == (h, enc) == wire.layout(d, 32 + n * enc)
                    assert -(-h // block) == ph // block - 1 or -(-h // block) < ph // block
            if n:
                _refused(hdr, 32 + n * dec + 4)
                _refused(hdr, 32 + n * dec - 4)
