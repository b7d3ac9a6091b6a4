"""Host reader of the reference's wire stream: Header (libs/codec.hpp:8-17) + per frame one record per transform tile, a u32 type
word and 3 x N x N raw f32 coefficients (libs/encoder.cpp:222-269).  Pure numpy, in the spirit of levels.py: it restates on its own
how a whole stream is read (the rule of svc_hip_wire_layout, include/svc_hip.h) and parses it into per-tile types and planes; and it
states the transcode between this stream and the compact stream (pack_stream, write_stream)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

HEADER_BYTES = 32
FIELDS = ("frame_count", "frame_w", "frame_h", "frame_excess_w", "frame_excess_h", "transform_block_w", "transform_block_h",
          "channel_count")


def parse_header(buf) -> Dict[str, int]:
    b = np.frombuffer(bytes(buf[:HEADER_BYTES]), np.uint8)
    if b.size < HEADER_BYTES:
        raise ValueError(f"a wire stream opens with a {HEADER_BYTES}-byte header; {b.size} bytes given")
    return {k: int(v) for k, v in zip(FIELDS, b.view("<u4"))}


def frame_bytes(w: int, h: int, block: int) -> int:
    """SerializeEncodedFrame's output for tile loops over w x h (libs/encoder.cpp:243-244)."""
    return -(-w // block) * -(-h // block) * (4 + 12 * block * block)


def layout(hdr: Dict[str, int], nbytes: int) -> Tuple[int, int]:
    """(emit_h, frame_bytes) of a stream of nbytes: the decoder's padded grid (libs/decoder.cpp:185-186) if the length fits it, else
    the reference encoder's unpadded loops (libs/encoder.cpp:647-650), which are only decodable without width padding."""
    if hdr["channel_count"] != 3:
        raise ValueError(f"channel_count {hdr['channel_count']}")
    b = hdr["transform_block_w"]
    if b != hdr["transform_block_h"] or b not in (8, 16):
        raise ValueError(f"tiles {b}x{hdr['transform_block_h']}")
    pw, ph = hdr["frame_w"] + hdr["frame_excess_w"], hdr["frame_h"] + hdr["frame_excess_h"]
    n = hdr["frame_count"]
    dec, enc = frame_bytes(pw, ph, b), frame_bytes(hdr["frame_w"], hdr["frame_h"], b)
    if nbytes == HEADER_BYTES + n * dec:
        return ph, dec
    if nbytes == HEADER_BYTES + n * enc:
        if hdr["frame_excess_w"]:
            raise ValueError("the encoder's reading with a padded width: scrambled coefficients")
        return hdr["frame_h"], enc
    raise ValueError(f"{nbytes} bytes: truncated or overlong")


def read_stream(buf) -> Tuple[Dict[str, int], np.ndarray, np.ndarray, np.ndarray]:
    """A whole stream -> (header, records (n, frame_bytes) u8, types (n, ph / N, pw / N) u32, planes (n, 3, ph, pw) f32).  The
    records are views into buf; tile rows the stream does not hold (the encoder's reading) are type 0 and zero coefficients."""
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    hdr = parse_header(b)
    emit_h, per = layout(hdr, b.size)
    n, N = hdr["frame_count"], hdr["transform_block_w"]
    pw, ph = hdr["frame_w"] + hdr["frame_excess_w"], hdr["frame_h"] + hdr["frame_excess_h"]
    tx, ty, rows = pw // N, ph // N, -(-emit_h // N)
    records = b[HEADER_BYTES:HEADER_BYTES + n * per].reshape(n, per)
    words = records.view("<u4").reshape(n, rows, tx, 1 + 3 * N * N)
    types = np.zeros((n, ty, tx), np.uint32)
    types[:, :rows] = words[..., 0]
    coef = words[..., 1:].view("<f4").reshape(n, rows, tx, 3, N, N)  # per channel N rows of N floats (libs/encoder.cpp:257-262)
    planes = np.zeros((n, 3, ph, pw), np.float32)
    planes[:, :, :rows * N] = coef.transpose(0, 3, 1, 4, 2, 5).reshape(n, 3, rows * N, pw)
    return hdr, records, types, planes


# ---- the wire stream <-> the compact stream ("SVCQ"), the statements of svc_hip_records_pack_levels_frames and
# ---- svc_hip_levels_records_frames (include/svc_hip.h) ------------------------------------------------------------------------------

def parse_records(records, pw: int, ph: int, block: int, emit_h: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """read_stream's parse for records without a header and any square tile: records (n, >= frame_bytes) u8, read at the padded size
    pw x ph with ceil(emit_h / block) tile rows held -> (types (n, ph / N, pw / N) u32, planes (n, 3, ph, pw) f32)."""
    N = block
    emit_h = ph if emit_h is None else emit_h
    tx, ty, rows = pw // N, ph // N, -(-emit_h // N)
    per = frame_bytes(pw, emit_h, N)
    records = np.asarray(records, np.uint8)
    n = records.shape[0]
    words = np.ascontiguousarray(records[:, :per]).view("<u4").reshape(n, rows, tx, 1 + 3 * N * N)
    types = np.zeros((n, ty, tx), np.uint32)
    types[:, :rows] = words[..., 0]
    coef = np.ascontiguousarray(words[..., 1:]).view("<f4").reshape(n, rows, tx, 3, N, N)
    planes = np.zeros((n, 3, ph, pw), np.float32)
    planes[:, :, :rows * N] = coef.transpose(0, 3, 1, 4, 2, 5).reshape(n, 3, rows * N, pw)
    return types, planes


def _pack(types: np.ndarray, planes: np.ndarray, rows: int, block: int, mv_block_w: int, mv_block_h: int, fg_step: int, bg_step: int
          ) -> Tuple[bytes, np.ndarray, np.ndarray]:
    """Per-tile types and raw planes, `rows` tile rows of them held -> the SVCQ stream.  An MV block's type is the type of the tile at
    its origin (the rule of svc_hip_dct_quant_frames read backwards); status 4 = a held tile's type differs from its MV block's."""
    from . import layers
    n, _, ph, pw = planes.shape
    if pw % mv_block_w or ph % mv_block_h or mv_block_w % block or mv_block_h % block:
        raise ValueError(f"MV block {mv_block_w}x{mv_block_h} must be a multiple of the tile {block} and divide the frame {pw}x{ph}")
    geometry = {"frame_w": pw, "frame_h": ph, "block_w": block, "block_h": block, "mv_block_w": mv_block_w, "mv_block_h": mv_block_h}
    sy, sx = mv_block_h // block, mv_block_w // block
    mv_types = np.ascontiguousarray(types[:, ::sy, ::sx])
    per_tile = np.repeat(np.repeat(mv_types, sy, 1), sx, 2)
    status = np.where((types[:, :rows] != per_tile[:, :rows]).reshape(n, -1).any(1), 4, 0).astype(np.uint32)
    frames = []
    for f in range(n):
        step = np.repeat(np.repeat(np.where(per_tile[f] == 0, bg_step, fg_step).astype(np.int64), block, 0), block, 1)[None]
        lv = layers.quantise(planes[f], step)
        inexact = int((planes[f] != lv.astype(np.float32) * step.astype(np.float32)).sum())  # as layers.pack_layers_frames counts it
        frames.append(layers.write_frame(geometry, mv_types[f], lv, fg_step, bg_step, inexact))
    offsets = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.uint64)
    return b"".join(frames), offsets, status


def pack_records(records, pw: int, ph: int, block: int, mv_block_w: int, mv_block_h: int, fg_step: int, bg_step: int,
                 emit_h: Optional[int] = None) -> Tuple[bytes, np.ndarray, np.ndarray]:
    """What svc_hip_records_pack_levels_frames writes for these records (finite coefficients) -> (SVCQ bytes, offsets (n + 1,) u64,
    status (n,) u32)."""
    types, planes = parse_records(records, pw, ph, block, emit_h)
    return _pack(types, planes, -(-(ph if emit_h is None else emit_h) // block), block, mv_block_w, mv_block_h, fg_step, bg_step)


def pack_stream(buf, mv_block_w: int, mv_block_h: int, fg_step: int, bg_step: int) -> Tuple[bytes, np.ndarray, np.ndarray]:
    """A whole wire stream (header first, read by read_stream) -> the compact stream at (fg_step, bg_step): (SVCQ bytes, offsets
    (n + 1,) u64, status (n,) u32).  The wire header carries no MV block, so the caller names one."""
    hdr, records, types, planes = read_stream(buf)
    emit_h, _ = layout(hdr, HEADER_BYTES + records.size)
    return _pack(types, planes, -(-emit_h // hdr["transform_block_w"]), hdr["transform_block_w"], mv_block_w, mv_block_h, fg_step, bg_step)


def write_stream(svcq, offsets, emit_h: Optional[int] = None) -> bytes:
    """A compact stream -> a whole wire stream, header included: per frame the records of ceil(emit_h / N) tile rows (default: all),
    each the type of the tile's MV block and the tile's 3 x N x N dequantised coefficients -- what svc_hip_levels_records_frames
    writes behind the header.  The header: frame_count = the number of frames, the padded size and zero excess; with emit_h below the
    padded height, frame_h = emit_h and the rest as frame_excess_h (the reference encoder's reading)."""
    from . import levels
    frames = list(levels.iter_frames(svcq, offsets))
    if not frames:
        raise ValueError("write_stream needs at least one frame: the wire header states the geometry")
    h0 = frames[0][0]
    N, pw, ph = h0["block_w"], h0["frame_w"], h0["frame_h"]
    if N != h0["block_h"]:
        raise ValueError(f"tiles {N}x{h0['block_h']}: a wire record holds a square tile")
    emit_h = ph if emit_h is None else emit_h
    if not 1 <= emit_h <= ph:
        raise ValueError(f"emit_h {emit_h} outside [1, {ph}]")
    tx, rows = pw // N, -(-emit_h // N)
    out = [np.array([len(frames), pw, emit_h, 0, ph - emit_h, N, N, 3], "<u4").tobytes()]
    for hdr, types, planes in frames:
        if any(hdr[k] != h0[k] for k in ("frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h")):
            raise ValueError("frames of different geometries")
        words = np.zeros((rows, tx, 1 + 3 * N * N), "<u4")
        ty_of, tx_of = np.arange(rows) * N // hdr["mv_block_h"], np.arange(tx) * N // hdr["mv_block_w"]
        words[..., 0] = types[ty_of[:, None], tx_of[None, :]]
        coef = planes[:, :rows * N].reshape(3, rows, N, tx, N).transpose(1, 3, 0, 2, 4).reshape(rows, tx, 3 * N * N)
        words[..., 1:] = np.ascontiguousarray(coef, "<f4").view("<u4")
        out.append(words.tobytes())
    return b"".join(out)
