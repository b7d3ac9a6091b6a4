"""Host reader of the reference's wire stream: Header (libs/codec.hpp:8-17) + per frame one record per transform tile, a u32 type
word and 3 x N x N raw f32 coefficients (libs/encoder.cpp:222-269).  Pure numpy, in the spirit of levels.py: it restates on its own
how a whole stream is read (the rule of svc_hip_wire_layout, include/svc_hip.h) and parses it into per-tile types and planes."""
from __future__ import annotations

from typing import Dict, Tuple

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
