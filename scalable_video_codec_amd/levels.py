"""Host reader of the compact quantised-coefficient stream ("SVCQ", format version 1; layout in include/svc_hip.h, written by
svc_hip_pack_levels_frames), and the step ladders its rate control (svc_hip_pack_levels_budget_frames) picks from.  Pure numpy: a
consumer of the stream needs neither a GPU nor the native library."""
from __future__ import annotations

from typing import Dict, Iterator, Tuple

import numpy as np

MAGIC = 0x51435653  # "SVCQ"
VERSION = 1
HEADER_BYTES = 64
FIELDS = ("magic", "version", "frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h", "fg_step", "bg_step",
          "level_count", "inexact", "frame_bytes")


def _need(buf: np.ndarray, end: int, what: str) -> None:
    if end > buf.size:
        raise ValueError(f"truncated SVCQ frame: {what} needs {end} bytes, the buffer has {buf.size}")


def parse_frame(buf) -> Tuple[Dict[str, int], np.ndarray, np.ndarray]:
    """One frame at the start of buf (bytes-like or u8 array) -> (header dict, types (mv_h, mv_w) u32, planes (3, H, W) f32)."""
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    _need(b, HEADER_BYTES, "the header")
    words = b[:HEADER_BYTES].view("<u4")
    hdr = {k: int(v) for k, v in zip(FIELDS, words)}
    if hdr["magic"] != MAGIC:
        raise ValueError(f"not an SVCQ frame (magic 0x{hdr['magic']:08x})")
    if hdr["version"] != VERSION:
        raise ValueError(f"SVCQ version {hdr['version']} (this reader knows {VERSION})")
    w, h, bw, bh = hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"]
    mbw, mbh = hdr["mv_block_w"], hdr["mv_block_h"]
    if min(w, h, bw, bh, mbw, mbh) == 0 or w % bw or h % bh or w % mbw or h % mbh:
        raise ValueError(f"SVCQ header with an inconsistent geometry: {hdr}")
    mfw, mfh = w // mbw, h // mbh
    tx, ty, area = w // bw, h // bh, bw * bh
    nw = (area + 63) // 64
    masks_off = HEADER_BYTES + 4 * mfw * mfh
    levels_off = masks_off + 8 * 3 * ty * tx * nw
    used = levels_off + 2 * hdr["level_count"]
    if hdr["frame_bytes"] != (used + 15) // 16 * 16:
        raise ValueError(f"SVCQ frame_bytes {hdr['frame_bytes']} does not match its sections ({used} B before padding)")
    _need(b, hdr["frame_bytes"], "the frame")
    types = b[HEADER_BYTES:masks_off].view("<u4").reshape(mfh, mfw).copy()
    masks = b[masks_off:levels_off].view("<u8").reshape(3, ty, tx, nw)
    all_bits = np.unpackbits(masks.view(np.uint8).reshape(3, ty, tx, nw * 8), axis=-1, bitorder="little").astype(bool)
    if all_bits[..., area:].any():
        raise ValueError(f"SVCQ masks have bits set past the tile's {area} coefficients")
    bits = all_bits[..., :area]
    if int(bits.sum()) != hdr["level_count"]:
        raise ValueError(f"SVCQ masks hold {int(bits.sum())} levels, the header {hdr['level_count']}")
    levels = b[levels_off:used].view("<i2")
    vals = np.zeros((3, ty, tx, area), np.float32)
    vals[bits] = levels.astype(np.float32)  # boolean assignment fills in C order: plane, tile row, tile, coefficient
    # step of each tile: region id of the MV block holding the tile origin
    tile_types = types[(np.arange(ty) * bh // mbh)[:, None], (np.arange(tx) * bw // mbw)[None, :]]
    step = np.where(tile_types == 0, np.float32(hdr["bg_step"]), np.float32(hdr["fg_step"])).astype(np.float32)
    vals *= step[None, :, :, None]
    planes = vals.reshape(3, ty, tx, bh, bw).transpose(0, 1, 3, 2, 4).reshape(3, h, w)
    return hdr, types, np.ascontiguousarray(planes)


def iter_frames(buf, offsets) -> Iterator[Tuple[Dict[str, int], np.ndarray, np.ndarray]]:
    """Every frame of a batch: offsets has n + 1 entries, frame i in [offsets[i], offsets[i + 1])."""
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    offsets = [int(o) for o in np.asarray(offsets).reshape(-1)]
    _need(b, offsets[-1], "the batch")
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        if lo % 16 or hi < lo:
            raise ValueError(f"SVCQ frame offsets out of order or misaligned: {lo}, {hi}")
        hdr, types, planes = parse_frame(b[lo:hi])
        if hdr["frame_bytes"] != hi - lo:
            raise ValueError(f"SVCQ frame at {lo} has frame_bytes {hdr['frame_bytes']}, its offsets {hi - lo}")
        yield hdr, types, planes


def step_ladder(fg_lo: int, fg_hi: int, bg_lo: int, bg_hi: int, n_bg: int, n_fg: int) -> np.ndarray:
    """A rate-control ladder, finest first: (K, 2) u32 rows (fg_step, bg_step), both columns non-decreasing.

    The background degrades before the foreground (the codec's content scalability): first
      (fg_lo, round(bg_lo * (bg_hi / bg_lo) ** (i / n_bg)))  for i = 0 .. n_bg,
    then
      (round(fg_lo * (fg_hi / fg_lo) ** (j / n_fg)), bg_hi)  for j = 1 .. n_fg,
    with round(x) = floor(x + 0.5) and exact end points; a pair equal to the one before it is dropped.  n_bg = 0 starts at
    (fg_lo, bg_hi); n_fg = 0 ends there.  At most n_bg + n_fg + 1 entries (the C ABI takes up to 64)."""
    for v in (fg_lo, fg_hi, bg_lo, bg_hi):
        if int(v) != v or v < 1:
            raise ValueError("steps are positive integers")
    if fg_lo > fg_hi or bg_lo > bg_hi:
        raise ValueError("a ladder runs from the finest step to the coarsest")
    if n_bg < 0 or n_fg < 0:
        raise ValueError("the numbers of steps are not negative")

    def geometric(lo: int, hi: int, i: int, n: int) -> int:
        if n == 0 or i == n:
            return int(hi)
        return int(min(hi, max(lo, np.floor(lo * (hi / lo) ** (i / n) + 0.5))))

    pairs = [(int(fg_lo), geometric(bg_lo, bg_hi, i, n_bg)) for i in range(n_bg + 1)]
    pairs += [(geometric(fg_lo, fg_hi, j, n_fg), int(bg_hi)) for j in range(1, n_fg + 1)]
    out = [pairs[0]]
    for p in pairs[1:]:
        if p != out[-1]:
            out.append(p)
    return np.array(out, np.uint32).reshape(-1, 2)
