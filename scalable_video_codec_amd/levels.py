"""Host reader of the compact quantised-coefficient stream ("SVCQ", format version 1; layout in include/svc_hip.h, written by
svc_hip_pack_levels_frames), the step ladders its rate control (svc_hip_pack_levels_budget_frames) picks from, and the statement of
the decode at reduced size (svc_hip_decode_levels_reduced_frames).  Pure numpy: a consumer of the stream needs neither a GPU nor the
native library."""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Sequence, Tuple

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


# ---- decode at reduced size from the low frequencies (include/svc_hip.h: svc_hip_decode_levels_reduced_frames) ------------------------

def _reduced_side(hdr: Dict[str, int], reduce: int) -> Tuple[int, int]:
    n = hdr["block_w"]
    if hdr["block_h"] != n or n not in (8, 16):
        raise ValueError(f"transform block {hdr['block_w']}x{hdr['block_h']} (supported: 8x8, 16x16)")
    if reduce not in (1, 2, 4, 8):
        raise ValueError(f"reduce {reduce} (supported: 1, 2, 4, 8)")
    return n, n // reduce


def _reduced(frame, reduce: int, fg_step: int, bg_step: int, gaze) -> Tuple[np.ndarray, int]:
    """reduced_coefficients and its K."""
    if fg_step <= 0 or bg_step <= 0:
        raise ValueError("quant steps must be positive")
    hdr, types, planes = parse_frame(frame)  # planes: (f32)level * (f32)enc_step
    n, k = _reduced_side(hdr, reduce)
    w, h = hdr["frame_w"], hdr["frame_h"]
    tx, ty = w // n, h // n
    ox, oy = (np.arange(tx) * n)[None, :], (np.arange(ty) * n)[:, None]
    background = types[(oy // hdr["mv_block_h"]), (ox // hdr["mv_block_w"])] == 0
    step = np.where(background, np.float32(bg_step), np.float32(fg_step)).astype(np.float32)
    if gaze is not None:
        x, y, gw, gh = (int(v) for v in gaze)
        step = np.where((ox >= x) & (ox - x < gw) & (oy >= y) & (oy - y < gh), np.float32(1), step)
    tiles = planes.reshape(3, ty, n, tx, n)[:, :, :k, :, :k]
    s = step[None, :, None, :, None]
    q = (tiles / s).astype(np.float32).astype(np.float64)
    r = np.copysign(np.floor(np.abs(q) + 0.5), q).astype(np.float32)
    out = (r * s).astype(np.float32) * np.float32(k / n)
    return np.ascontiguousarray(out.reshape(3, ty * k, tx * k), np.float32), k


def reduced_coefficients(frame, reduce: int, fg_step: int, bg_step: int, gaze: Optional[Sequence[int]] = None) -> np.ndarray:
    """What the reduced decoder inverts -> (3, H / reduce, W / reduce) f32, laid out as K x K tiles (K = N / reduce): the first K x K
    coefficients of every N x N tile, c = (f32)level * (f32)enc_step requantised with the decoder's step (1 for a tile whose origin
    the gaze rectangle x, y, w, h holds, else bg_step for a tile whose MV block has type 0, else fg_step), q = roundf(c / step) * step,
    and scaled by K / N.  Every operation is one f32 operation: roundf is taken in f64 on the f32 quotient (exact there; in f32
    floor(|q| + 0.5) is wrong for quotients above 2^23), the scaling is by a power of two.  reduce = 1: the full decoder's q."""
    return _reduced(frame, reduce, fg_step, bg_step, gaze)[0]


def _basis(k: int) -> np.ndarray:
    """The orthonormal DCT-II basis C[u][m] = a_k(u) cos(pi u (2 m + 1) / 2 k), f64."""
    u, m = np.arange(k)[:, None], np.arange(k)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / k), np.sqrt(2.0 / k))
    return a * np.cos(np.pi * u * (2 * m + 1) / (2 * k))


def decode_reduced_frame(frame, reduce: int, fg_step: int, bg_step: int, gaze: Optional[Sequence[int]] = None) -> np.ndarray:
    """The reduced decoder's picture before its rounding to f32 -> (H / reduce, W / reduce, 3) f64 B,G,R: the K-point inverse DCT-II
    along rows and columns of every K x K tile of reduced_coefficients.  reduce = 1 is the full decoder."""
    coef, k = _reduced(frame, reduce, fg_step, bg_step, gaze)
    coef = coef.astype(np.float64)
    c = _basis(k)
    _, rh, rw = coef.shape
    t = coef.reshape(3, rh // k, k, rw // k, k)
    x = np.einsum("vy,pavbu,ux->paybx", c, t, c)  # x[y][x] = sum_v sum_u C[v][y] q[v][u] C[u][x]
    return np.ascontiguousarray(x.reshape(3, rh, rw).transpose(1, 2, 0))
