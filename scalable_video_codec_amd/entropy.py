"""Lossless entropy coding of the compact stream: "SVCE" (format version 1) frames from and back to "SVCQ" frames.

The format is stated in include/svc_hip.h next to the SVCQ table; this module is its executable statement, and the GPU entry points
(svc_hip_entropy_encode_frames / svc_hip_entropy_decode_frames) write and read the same bytes.  decode_frame(encode_frame(f)) == f
byte for byte for every well-formed SVCQ frame.  Pure numpy: a consumer of the stream needs neither a GPU nor the native library.

Encoding is vectorised over the whole frame.  Decoding inside a chunk is serial by design; the decoder here runs every chunk of a
frame in lockstep (one codeword per chunk per step), the way the GPU runs one lane per chunk."""
from __future__ import annotations

from typing import Dict, Iterator, Tuple

import numpy as np

from . import levels

MAGIC = 0x45435653  # "SVCE"
VERSION = 1
HEADER_BYTES = 64
FIELDS = ("magic", "version", "frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h", "fg_step", "bg_step",
          "level_count", "inexact", "frame_bytes", "svcq_frame_bytes", "chunk_tiles", "types_bytes")
CHUNK_COEFFS = 2048  # the encoder's chunk: about this many coefficients, at most MAX_CHUNK_TILES tiles
MAX_CHUNK_TILES = 64
MAX_PREFIX = 24  # an Exp-Golomb prefix longer than this is malformed (no valid value needs more than 17)


def chunk_tiles_for(block_w: int, block_h: int) -> int:
    """The chunk_tiles the encoder writes for a tile shape: clamp(2048 / area, 1, 64)."""
    return int(min(MAX_CHUNK_TILES, max(1, CHUNK_COEFFS // (block_w * block_h))))


def _u8(buf) -> np.ndarray:
    return np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)


def _up(v, m):
    return (v + m - 1) // m * m


def _bitlen(x: np.ndarray) -> np.ndarray:
    """Bit length of non-negative integers below 2^53 (0 -> 0)."""
    return np.frexp(np.asarray(x, np.float64))[1].astype(np.int64)


def _sgn(v: np.ndarray) -> np.ndarray:
    """Signed -> unsigned: v > 0 -> 2v - 1, v <= 0 -> -2v."""
    v = np.asarray(v, np.int64)
    return np.where(v > 0, 2 * v - 1, -2 * v)


def _unsgn(u: np.ndarray) -> np.ndarray:
    u = np.asarray(u, np.int64)
    return np.where(u & 1, (u + 1) >> 1, -(u >> 1))


def _eg_len(u: np.ndarray, k) -> np.ndarray:
    """Length of the Exp-Golomb-k code of u >= 0: 2 * floor(log2((u >> k) + 1)) + 1 + k."""
    u = np.asarray(u, np.int64)
    return 2 * (_bitlen((u >> k) + 1) - 1) + 1 + k


def _eg_field(pos: np.ndarray, u: np.ndarray, k) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The Exp-Golomb-k code of u written at bit pos, as one field (pos', value, bits): w = u + 2^k, n = bit length of w - 1,
    z = n - k zero bits, then a 1, then the low n bits of w, least significant first."""
    u = np.asarray(u, np.int64)
    k = np.asarray(k, np.int64)
    w = u + (np.int64(1) << k)
    n = _bitlen(w) - 1
    z = n - k
    val = (1 | ((w & ((np.int64(1) << n) - 1)) << 1)).astype(np.uint64)
    return np.asarray(pos, np.int64) + z, val, n + 1


class _Geom:
    def __init__(self, w, h, bw, bh, mbw, mbh, ct):
        self.w, self.h, self.bw, self.bh, self.mbw, self.mbh = w, h, bw, bh, mbw, mbh
        self.mfw, self.mfh = w // mbw, h // mbh
        self.mvb = self.mfw * self.mfh
        self.tx, self.ty, self.area = w // bw, h // bh, bw * bh
        self.nw = (self.area + 63) // 64
        self.masks_off = HEADER_BYTES + 4 * self.mvb
        self.levels_off = self.masks_off + 8 * 3 * self.ty * self.tx * self.nw
        self.ct = ct
        self.cx = -(-self.tx // ct)  # chunks per tile row
        self.chunks = 3 * self.ty * self.cx
        # tiles of each chunk (the last chunk of a row may be short)
        self.chunk_nt = np.tile(np.minimum(ct, self.tx - np.arange(self.cx) * ct), 3 * self.ty).astype(np.int64)

    def svcq_bytes(self, level_count: int) -> int:
        return _up(self.levels_off + 2 * level_count, 16)


def _geometry_ok(hdr) -> bool:
    w, h, bw, bh, mbw, mbh = (hdr[k] for k in ("frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h"))
    return (min(w, h, bw, bh, mbw, mbh) > 0 and w % bw == 0 and h % bh == 0 and w % mbw == 0 and h % mbh == 0
            and mbw % bw == 0 and mbh % bh == 0 and hdr["fg_step"] > 0 and hdr["bg_step"] > 0)


def _svcq_sections(b: np.ndarray, chunk_tiles=None):
    """A well-formed SVCQ frame at the start of b -> (header words (16,) u32, geometry, masks (3, ty, tx, nw) u64,
    bits (3, ty, tx, area) bool, levels i16).  ValueError for what svc_hip_entropy_encode_frames flags (statuses 1 .. 7)."""
    if b.size < HEADER_BYTES:
        raise ValueError(f"truncated SVCQ frame: the header needs {HEADER_BYTES} bytes, the buffer has {b.size}")
    words = b[:HEADER_BYTES].view("<u4").astype(np.int64)
    hdr = {k: int(v) for k, v in zip(levels.FIELDS, words)}
    if hdr["magic"] != levels.MAGIC:
        raise ValueError(f"not an SVCQ frame (magic 0x{hdr['magic']:08x})")
    if hdr["version"] != levels.VERSION:
        raise ValueError(f"SVCQ version {hdr['version']} (this coder knows {levels.VERSION})")
    if not _geometry_ok(hdr) or words[13:].any():
        raise ValueError(f"SVCQ header with an inconsistent geometry, a step of 0 or non-zero reserved words: {hdr}")
    g = _Geom(hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"], hdr["mv_block_w"], hdr["mv_block_h"],
              chunk_tiles_for(hdr["block_w"], hdr["block_h"]) if chunk_tiles is None else int(chunk_tiles))
    if hdr["frame_bytes"] != g.svcq_bytes(hdr["level_count"]) or hdr["frame_bytes"] > b.size:
        raise ValueError(f"SVCQ frame_bytes {hdr['frame_bytes']} does not match its sections or runs past the {b.size} B buffer")
    if b[g.levels_off + 2 * hdr["level_count"]:hdr["frame_bytes"]].any():
        raise ValueError("SVCQ frame with non-zero padding")
    masks = b[g.masks_off:g.levels_off].view("<u8").reshape(3, g.ty, g.tx, g.nw)
    all_bits = np.unpackbits(masks.view(np.uint8).reshape(3, g.ty, g.tx, g.nw * 8), axis=-1, bitorder="little").astype(bool)
    if all_bits[..., g.area:].any():
        raise ValueError(f"SVCQ masks have bits set past the tile's {g.area} coefficients")
    bits = all_bits[..., :g.area]
    if int(bits.sum()) != hdr["level_count"]:
        raise ValueError(f"SVCQ masks hold {int(bits.sum())} levels, the header {hdr['level_count']}")
    lev = b[g.levels_off:g.levels_off + 2 * hdr["level_count"]].view("<i2")
    return words, g, masks, bits, lev


# ---- types section --------------------------------------------------------------------------------------------------------------

def _encode_types(types: np.ndarray) -> bytes:
    """u32 word 0: mode | width << 8.  Mode 0: a bitmap of ceil(mvb / 32) u32 (bit i % 32 of word i / 32 = type i != 0), then the
    non-zero types in raster order as (type - 1) in `width` bits each (the bit length of the largest one minus 1), packed least
    significant first into u32 words.  Mode 1 (when strictly smaller): the types as raw u32."""
    t = np.asarray(types, np.uint64).reshape(-1)
    mvb = t.size
    raw_bytes = 4 + 4 * mvb
    nz = t[t != 0]
    width = int(_bitlen(np.array([int(nz.max()) - 1]))[0]) if nz.size else 0
    bm_words = -(-mvb // 32)
    val_words = -(-(nz.size * width) // 32)
    if raw_bytes < 4 * (1 + bm_words + val_words):
        return np.concatenate([[1], t]).astype("<u4").tobytes()
    bitmap = np.packbits(np.concatenate([t != 0, np.zeros(bm_words * 32 - mvb, bool)]), bitorder="little")
    vals = np.zeros(val_words * 32, bool)
    if width:
        v = (nz - np.uint64(1))[:, None] >> np.arange(width, dtype=np.uint64)[None, :]
        vals[:nz.size * width] = (v & np.uint64(1)).astype(bool).reshape(-1)
    return (np.array([width << 8], "<u4").tobytes() + bitmap.tobytes() + np.packbits(vals, bitorder="little").tobytes())


def _decode_types(sec: np.ndarray, mvb: int) -> np.ndarray:
    if sec.size < 4:
        raise ValueError("SVCE types section shorter than its mode word")
    head = int(sec[:4].view("<u4")[0])
    mode, width = head & 0xFF, head >> 8
    if mode == 1 and width == 0:
        if sec.size != 4 + 4 * mvb:
            raise ValueError(f"SVCE raw types section of {sec.size} B, {4 + 4 * mvb} B expected")
        return sec[4:].view("<u4").copy()
    if mode != 0 or width > 32:
        raise ValueError(f"SVCE types section with mode word 0x{head:08x}")
    bm_words = -(-mvb // 32)
    if sec.size < 4 + 4 * bm_words:
        raise ValueError("SVCE types section shorter than its bitmap")
    bits = np.unpackbits(sec[4:4 + 4 * bm_words], bitorder="little").astype(bool)
    if bits[mvb:].any():
        raise ValueError("SVCE types bitmap has bits set past the MV blocks")
    bits = bits[:mvb]
    nnz = int(bits.sum())
    if sec.size != 4 * (1 + bm_words + -(-(nnz * width) // 32)):
        raise ValueError(f"SVCE types section of {sec.size} B does not match its {nnz} non-zero types of {width} bits")
    out = np.zeros(mvb, np.uint64)
    if nnz:
        if width:
            vb = np.unpackbits(sec[4 + 4 * bm_words:], bitorder="little")[:nnz * width].reshape(nnz, width).astype(np.uint64)
            v = (vb << np.arange(width, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        else:
            v = np.zeros(nnz, np.uint64)
        out[bits] = v + np.uint64(1)
    if out.max(initial=0) > 0xFFFFFFFF:
        raise ValueError("SVCE types section holds a type above 2^32 - 1")
    return out.astype(np.uint32)


# ---- encode ---------------------------------------------------------------------------------------------------------------------

def encode_frame(svcq, chunk_tiles=None, force_k=None) -> bytes:
    """One SVCQ frame (at the start of svcq; bytes-like or u8 array) -> its SVCE frame.  chunk_tiles: None = what the GPU encoder
    writes (chunk_tiles_for); any other value from 1 to 2^32 - 1 makes a frame every decoder must read, or a ValueError when a chunk
    of that many tiles does not fit the index's u16 fields.  force_k: None = the encoder's choice (per chunk the k_dc and k_ac of the
    fewest bits, raw when that is smaller); (k_dc, k_ac), each 0 .. 7, codes every chunk with these parameters, and raw only where a
    set mask bit holds level 0 -- a legal stream every decoder must read, with chunks that may be larger than their raw form."""
    if chunk_tiles is not None and not 1 <= int(chunk_tiles) <= 0xFFFFFFFF:
        raise ValueError(f"chunk_tiles {chunk_tiles} is not in 1 .. 2^32 - 1")
    if force_k is not None and not (len(force_k) == 2 and all(0 <= int(k) <= 7 for k in force_k)):
        raise ValueError(f"force_k {force_k} is not a pair of parameters in 0 .. 7")
    b = _u8(svcq)
    words, g, masks, bits, lev = _svcq_sections(b, chunk_tiles)
    C, ct, area = g.chunks, g.ct, g.area
    T = 3 * g.ty * g.tx
    bits_t = bits.reshape(T, area)
    vals = np.zeros((T, area), np.int64)
    vals[bits_t] = lev.astype(np.int64)
    x = np.tile(np.arange(g.tx), 3 * g.ty)
    row = np.repeat(np.arange(3 * g.ty), g.tx)
    chunk = row * g.cx + x // ct
    first = x % ct == 0
    # per tile: DC difference, AC count; per AC level: run, value
    dc = vals[:, 0]
    prev = np.where(first, 0, np.concatenate([[0], dc[:-1]]))
    udc = _sgn(dc - prev)
    ac_t, ac_p = np.nonzero(bits_t[:, 1:])
    ac_p = ac_p + 1
    nac = np.bincount(ac_t, minlength=T).astype(np.int64)
    new_tile = np.concatenate([[True], ac_t[1:] != ac_t[:-1]]) if ac_t.size else np.zeros(0, bool)
    prev_p = np.where(new_tile, 0, np.concatenate([[0], ac_p[:-1]]))
    run = ac_p - prev_p - 1
    uac = _sgn(vals[ac_t, ac_p])
    ac_chunk = chunk[ac_t]
    # per chunk: a zero level under a set mask bit cannot be coded (the DC's bit is implied by its value): raw
    forced = np.bincount(chunk, weights=(bits_t & (vals == 0)).any(axis=1), minlength=C) > 0
    cnt = np.bincount(chunk, weights=bits_t.sum(axis=1), minlength=C).astype(np.int64)
    ks = np.arange(8)
    dc_bits = np.stack([np.bincount(chunk, weights=_eg_len(udc, k), minlength=C) for k in ks], 1)
    ac_bits = np.stack([np.bincount(ac_chunk, weights=_eg_len(uac, k), minlength=C) for k in ks], 1)
    k_dc = np.argmin(dc_bits, axis=1)  # ties: the smallest k
    k_ac = np.argmin(ac_bits, axis=1)
    if force_k is not None:
        k_dc, k_ac = np.full(C, int(force_k[0]), np.int64), np.full(C, int(force_k[1]), np.int64)
    fixed = 7 + np.bincount(chunk, weights=_eg_len(nac, 0), minlength=C) + np.bincount(ac_chunk, weights=_eg_len(run, 0), minlength=C)
    coded_bits = (fixed + dc_bits[np.arange(C), k_dc] + ac_bits[np.arange(C), k_ac]).astype(np.int64)
    coded_bytes = (coded_bits + 7) // 8
    raw_bytes = 1 + 8 * g.nw * g.chunk_nt + 2 * cnt
    raw = forced | ((raw_bytes < coded_bytes) & (force_k is None))
    sizes = np.where(raw, raw_bytes, coded_bytes)
    if sizes.max(initial=0) > 0xFFFF or cnt.max(initial=0) > 0xFFFF:
        raise ValueError(f"a chunk of {ct} tiles holds {int(sizes.max())} bytes or {int(cnt.max())} levels: above the index's u16 fields")

    types_sec = _encode_types(b[HEADER_BYTES:g.masks_off].view("<u4"))
    payload_off = HEADER_BYTES + len(types_sec) + 4 * C
    chunk_off = payload_off + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    used = payload_off + int(sizes.sum())
    frame_bytes = _up(used, 16)
    out = np.zeros(frame_bytes + 8, np.uint8)

    # coded chunks: every codeword as a field (bit position, value, bits); the fields never overlap, so OR == ADD per byte
    coded = ~raw
    kd_t, ka_t = k_dc[chunk], k_ac[chunk]
    l_dc = _eg_len(udc, kd_t)
    l_nac = _eg_len(nac, 0)
    l_pair = _eg_len(run, 0) + _eg_len(uac, ka_t[ac_t])
    tile_len = l_dc + l_nac + np.bincount(ac_t, weights=l_pair, minlength=T).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(tile_len)[:-1]])
    chunk_first_tile = np.flatnonzero(first)
    tile_start = chunk_off[chunk] * 8 + 7 + cs - cs[chunk_first_tile][chunk]
    pcs = np.concatenate([[0], np.cumsum(l_pair)[:-1]]).astype(np.int64)
    tile_first_pair = np.searchsorted(ac_t, np.arange(T))
    pair_start = tile_start[ac_t] + l_dc[ac_t] + l_nac[ac_t] + pcs - pcs[tile_first_pair[ac_t]]
    ct_mask, ac_mask = coded[chunk], coded[ac_chunk]
    fields = [
        (chunk_off[coded] * 8, (k_dc[coded] << 1 | k_ac[coded] << 4).astype(np.uint64), np.full(int(coded.sum()), 7)),
        _eg_field(tile_start[ct_mask], udc[ct_mask], kd_t[ct_mask]),
        _eg_field(tile_start[ct_mask] + l_dc[ct_mask], nac[ct_mask], 0),
        _eg_field(pair_start[ac_mask], run[ac_mask], 0),
        _eg_field(pair_start[ac_mask] + _eg_len(run[ac_mask], 0), uac[ac_mask], ka_t[ac_t][ac_mask]),
    ]
    pos = np.concatenate([f[0] for f in fields]).astype(np.int64)
    val = np.concatenate([f[1] for f in fields]).astype(np.uint64) << (pos & 7).astype(np.uint64)
    byte = pos >> 3
    acc = np.zeros(out.size, np.float64)
    for j in range(5):  # a field is at most 25 bits after its shift: 4 bytes
        part = ((val >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.float64)
        keep = part != 0
        acc += np.bincount(byte[keep] + j, weights=part[keep], minlength=out.size)[:out.size]
    out[:] = acc.astype(np.uint8)

    # raw chunks: a mode byte of 1, then the chunk's mask words and levels verbatim
    lev_off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    mflat = masks.reshape(3 * g.ty, g.tx, g.nw)
    lbytes = lev.view(np.uint8)
    for c in np.flatnonzero(raw):
        r, t0 = divmod(int(c), g.cx)
        t0 *= ct
        nt = int(g.chunk_nt[c])
        o = int(chunk_off[c])
        mb = mflat[r, t0:t0 + nt].view(np.uint8).reshape(-1)
        lb = lbytes[2 * lev_off[c]:2 * (lev_off[c] + cnt[c])]
        out[o] = 1
        out[o + 1:o + 1 + mb.size] = mb
        out[o + 1 + mb.size:o + 1 + mb.size + lb.size] = lb

    hdr = words.copy()
    hdr[0], hdr[12], hdr[13], hdr[14], hdr[15] = MAGIC, frame_bytes, words[12], ct, len(types_sec)
    out[:HEADER_BYTES] = np.frombuffer(hdr.astype("<u4").tobytes(), np.uint8)
    ts = HEADER_BYTES
    out[ts:ts + len(types_sec)] = np.frombuffer(types_sec, np.uint8)
    index = (sizes | (cnt << 16)).astype("<u4")
    out[ts + len(types_sec):payload_off] = np.frombuffer(index.tobytes(), np.uint8)
    return out[:frame_bytes].tobytes()


# ---- parse and decode -----------------------------------------------------------------------------------------------------------

def parse_frame(buf) -> Tuple[Dict[str, int], np.ndarray, np.ndarray]:
    """One SVCE frame at the start of buf -> (header dict, chunk sizes (chunks,) int64, chunk level counts (chunks,) int64).
    Checks the header, the section sizes and the index against each other; ValueError says what is wrong."""
    b = _u8(buf)
    if b.size < HEADER_BYTES:
        raise ValueError(f"truncated SVCE frame: the header needs {HEADER_BYTES} bytes, the buffer has {b.size}")
    hdr = {k: int(v) for k, v in zip(FIELDS, b[:HEADER_BYTES].view("<u4"))}
    if hdr["magic"] != MAGIC:
        raise ValueError(f"not an SVCE frame (magic 0x{hdr['magic']:08x})")
    if hdr["version"] != VERSION:
        raise ValueError(f"SVCE version {hdr['version']} (this reader knows {VERSION})")
    if not _geometry_ok(hdr) or hdr["chunk_tiles"] == 0:
        raise ValueError(f"SVCE header with an inconsistent geometry, a step of 0 or no tiles per chunk: {hdr}")
    if hdr["frame_bytes"] % 16 or hdr["frame_bytes"] < HEADER_BYTES:
        raise ValueError(f"SVCE frame_bytes {hdr['frame_bytes']} is not a multiple of 16")
    if hdr["frame_bytes"] > b.size:
        raise ValueError(f"truncated SVCE frame: frame_bytes {hdr['frame_bytes']}, the buffer has {b.size}")
    g = _Geom(hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"], hdr["mv_block_w"], hdr["mv_block_h"],
              hdr["chunk_tiles"])
    if hdr["level_count"] > 3 * g.w * g.h or hdr["svcq_frame_bytes"] != g.svcq_bytes(hdr["level_count"]):
        raise ValueError(f"SVCE svcq_frame_bytes {hdr['svcq_frame_bytes']}, its level count makes {g.svcq_bytes(hdr['level_count'])}")
    payload_off = HEADER_BYTES + hdr["types_bytes"] + 4 * g.chunks
    if hdr["types_bytes"] % 4 or payload_off > hdr["frame_bytes"]:
        raise ValueError(f"SVCE types section of {hdr['types_bytes']} B and index of {g.chunks} chunks overrun the frame")
    index = b[HEADER_BYTES + hdr["types_bytes"]:payload_off].view("<u4").astype(np.int64)
    sizes, counts = index & 0xFFFF, index >> 16
    if _up(payload_off + int(sizes.sum()), 16) != hdr["frame_bytes"]:
        raise ValueError(f"SVCE index: chunks of {int(sizes.sum())} B after {payload_off} B do not make frame_bytes {hdr['frame_bytes']}")
    if int(counts.sum()) != hdr["level_count"]:
        raise ValueError(f"SVCE index holds {int(counts.sum())} levels, the header {hdr['level_count']}")
    return hdr, sizes, counts


def _peek64(b: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """The 64 bits of b from bit pos (b has 16 zero bytes past every position asked for)."""
    i = pos >> 3
    s = (pos & 7).astype(np.uint64)
    lo = np.zeros(pos.size, np.uint64)
    for j in range(8):
        lo |= b[i + j].astype(np.uint64) << np.uint64(8 * j)
    hi = b[i + 8].astype(np.uint64)
    return (lo >> s) | np.where(s > 0, hi << ((np.uint64(64) - s) & np.uint64(63)), np.uint64(0))


def _ctz64(v: np.ndarray) -> np.ndarray:
    """Trailing zeros of u64 values (64 for 0)."""
    low = v & (~v + np.uint64(1))
    lo32 = (low & np.uint64(0xFFFFFFFF)).astype(np.float64)
    hi32 = (low >> np.uint64(32)).astype(np.float64)
    z = np.where(lo32 > 0, np.frexp(lo32)[1] - 1, np.frexp(hi32)[1] + 31)
    return np.where(v == 0, 64, z).astype(np.int64)


def decode_frame(svce) -> bytes:
    """One SVCE frame (at the start of svce) -> the SVCQ frame it codes.  ValueError for every frame the GPU decoder flags."""
    b = _u8(svce)
    hdr, sizes, counts = parse_frame(b)
    g = _Geom(hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"], hdr["mv_block_w"], hdr["mv_block_h"],
              hdr["chunk_tiles"])
    types = _decode_types(b[HEADER_BYTES:HEADER_BYTES + hdr["types_bytes"]], g.mvb)
    fb = np.zeros(hdr["frame_bytes"] + 16, np.uint8)
    fb[:hdr["frame_bytes"]] = b[:hdr["frame_bytes"]]
    C, ct, area = g.chunks, g.ct, g.area
    payload_off = HEADER_BYTES + hdr["types_bytes"] + 4 * C
    start = payload_off + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    nt = g.chunk_nt
    vals = np.zeros((C, min(ct, g.tx), area), np.int64)
    bits = np.zeros((C, min(ct, g.tx), area), bool)

    def bad(c, why):
        raise ValueError(f"SVCE chunk {int(c)} (of {C}): {why}")

    for c in np.flatnonzero(sizes == 0):
        bad(c, "empty")
    raw = (fb[np.minimum(start, fb.size - 1)] & 1).astype(bool)
    # raw chunks: the mask words and levels verbatim
    for c in np.flatnonzero(raw):
        n_t, o, s = int(nt[c]), int(start[c]), int(sizes[c])
        if s != 1 + 8 * g.nw * n_t + 2 * int(counts[c]):
            bad(c, f"raw chunk of {s} B for {n_t} tiles and {int(counts[c])} levels")
        m = fb[o + 1:o + 1 + 8 * g.nw * n_t]
        mb = np.unpackbits(m, bitorder="little").reshape(n_t, g.nw * 64).astype(bool)
        if mb[:, area:].any():
            bad(c, "raw mask bits set past the tile")
        if int(mb.sum()) != int(counts[c]):
            bad(c, f"raw masks hold {int(mb.sum())} levels, the index {int(counts[c])}")
        bits[c, :n_t] = mb[:, :area]
        lv = fb[o + 1 + m.size:o + s].view("<i2").astype(np.int64)
        vals[c, :n_t][mb[:, :area]] = lv

    # coded chunks in lockstep: one Exp-Golomb codeword per chunk per step
    lane = np.flatnonzero(~raw)
    head = fb[start[lane]].astype(np.int64) | (fb[start[lane] + 1].astype(np.int64) << 8)
    kd, ka = (head >> 1) & 7, (head >> 4) & 7
    pos = start[lane] * 8 + 7
    end = (start[lane] + sizes[lane]) * 8
    phase = np.zeros(lane.size, np.int64)  # 0 DC, 1 AC count, 2 run, 3 level
    tile = np.zeros(lane.size, np.int64)
    dcp = np.zeros(lane.size, np.int64)
    rem = np.zeros(lane.size, np.int64)
    cpos = np.zeros(lane.size, np.int64)
    a = np.arange(lane.size)
    while a.size:
        k = np.select([phase[a] == 0, phase[a] == 3], [kd[a], ka[a]], 0)
        p = pos[a]
        peek = _peek64(fb, p)
        z = _ctz64(peek)
        badz = z > MAX_PREFIX
        if badz.any():
            bad(lane[a[badz][0]], "an Exp-Golomb prefix of more than 24 zeros")
        n = z + k
        length = z + 1 + n
        wlow = (peek >> (z + 1).astype(np.uint64)) & ((np.uint64(1) << n.astype(np.uint64)) - np.uint64(1))
        u = ((np.int64(1) << n) | wlow.astype(np.int64)) - (np.int64(1) << k)
        over = p + length > end[a]
        if over.any():
            bad(lane[a[over][0]], "decodes past its size")
        pos[a] = p + length
        ph = phase[a]
        c = lane[a]
        t = tile[a]
        # DC
        m = ph == 0
        if m.any():
            v = dcp[a[m]] + _unsgn(u[m])
            oob = (v < -32768) | (v > 32767)
            if oob.any():
                bad(c[m][oob][0], "a DC level outside int16")
            vals[c[m], t[m], 0] = v
            bits[c[m], t[m], 0] = v != 0
            dcp[a[m]] = v
            phase[a[m]] = 1
        # AC count
        m = ph == 1
        endt = np.zeros(a.size, bool)
        if m.any():
            oob = u[m] > area - 1
            if oob.any():
                bad(c[m][oob][0], "an AC count outside the tile")
            rem[a[m]] = u[m]
            cpos[a[m]] = 0
            phase[a[m]] = np.where(u[m] == 0, 0, 2)
            endt[m] = u[m] == 0
        # run
        m = ph == 2
        if m.any():
            q = cpos[a[m]] + u[m] + 1
            oob = q > area - 1
            if oob.any():
                bad(c[m][oob][0], "a run past the tile")
            cpos[a[m]] = q
            phase[a[m]] = 3
        # level
        m = ph == 3
        if m.any():
            v = _unsgn(u[m])
            oob = (v < -32768) | (v > 32767)
            if oob.any():
                bad(c[m][oob][0], "an AC level outside int16")
            vals[c[m], t[m], cpos[a[m]]] = v
            bits[c[m], t[m], cpos[a[m]]] = True
            rem[a[m]] -= 1
            done = rem[a[m]] == 0
            phase[a[m]] = np.where(done, 0, 2)
            endt[m] = done
        tile[a[endt]] += 1
        a = a[tile[a] < nt[lane[a]]]
    got = bits[lane].reshape(lane.size, bits.shape[1] * area).sum(axis=1)
    wrong = got != counts[lane]
    if wrong.any():
        bad(lane[wrong][0], f"decodes to {int(got[wrong][0])} levels, the index says {int(counts[lane][wrong][0])}")
    short = (pos + 7) // 8 != start[lane] + sizes[lane]
    if short.any():
        bad(lane[short][0], "ends before its size")

    # the SVCQ frame
    vals = vals.reshape(3, g.ty, g.cx * min(ct, g.tx), area)[:, :, :g.tx]
    bits = bits.reshape(3, g.ty, g.cx * min(ct, g.tx), area)[:, :, :g.tx]
    pad = np.zeros((3, g.ty, g.tx, g.nw * 64), bool)
    pad[..., :area] = bits
    masks = np.packbits(pad, axis=-1, bitorder="little")
    lev = vals[bits].astype("<i2")
    out = np.zeros(hdr["svcq_frame_bytes"], np.uint8)
    words = b[:HEADER_BYTES].view("<u4").copy()
    words[0], words[12], words[13:] = levels.MAGIC, hdr["svcq_frame_bytes"], 0
    out[:HEADER_BYTES] = words.view(np.uint8)
    out[HEADER_BYTES:g.masks_off] = types.astype("<u4").view(np.uint8)
    out[g.masks_off:g.levels_off] = masks.reshape(-1)
    out[g.levels_off:g.levels_off + 2 * lev.size] = lev.view(np.uint8)
    return out.tobytes()


# ---- batches --------------------------------------------------------------------------------------------------------------------

def _frames(buf, offsets, what):
    b = _u8(buf)
    offs = [int(o) for o in np.asarray(offsets).reshape(-1)]
    if offs[-1] > b.size:
        raise ValueError(f"truncated {what} batch: offsets end at {offs[-1]}, the buffer has {b.size}")
    for lo, hi in zip(offs[:-1], offs[1:]):
        if lo % 16 or hi < lo:
            raise ValueError(f"{what} frame offsets out of order or misaligned: {lo}, {hi}")
        yield lo, hi, b[lo:hi]


def _join(frames):
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    return b"".join(frames), offs


def iter_frames(buf, offsets) -> Iterator[bytes]:
    """Every frame of an SVCE batch (offsets has n + 1 entries), decoded to its SVCQ frame."""
    for lo, hi, fr in _frames(buf, offsets, "SVCE"):
        if parse_frame(fr)[0]["frame_bytes"] != hi - lo:
            raise ValueError(f"SVCE frame at {lo} has a frame_bytes other than its offsets' {hi - lo}")
        yield decode_frame(fr)


def encode_frames(buf, offsets, chunk_tiles=None, force_k=None) -> Tuple[bytes, np.ndarray]:
    """An SVCQ batch -> (SVCE bytes, offsets (n + 1,) u64).  chunk_tiles and force_k as encode_frame."""
    return _join([encode_frame(fr, chunk_tiles, force_k) for _, _, fr in _frames(buf, offsets, "SVCQ")])


def decode_frames(buf, offsets) -> Tuple[bytes, np.ndarray]:
    """An SVCE batch -> (SVCQ bytes, offsets (n + 1,) u64)."""
    return _join(list(iter_frames(buf, offsets)))


# ---- a stored SVCE stream restricted to a window, on its coded bytes (include/svc_hip.h: svc_hip_window_entropy_frames) ---------------

def _walk_chunk(payload: np.ndarray, count: int, nt: int, upto: int, g: _Geom, c: int) -> Tuple[np.ndarray, np.ndarray]:
    """Tiles [0, upto) of a chunk of nt tiles, read as the device call reads a cut chunk: from its first tile to its last kept one and
    no further, so the end-of-chunk checks of decode_frame are not made -> (bits (upto, area) bool, values (upto, area) i64)."""
    area, nw = g.area, g.nw
    bits = np.zeros((upto, area), bool)
    vals = np.zeros((upto, area), np.int64)

    def bad(why):
        raise ValueError(f"SVCE chunk {c}: {why}")

    size = payload.size
    if size == 0:
        bad("empty")
    if payload[0] & 1:
        if size != 1 + 8 * nw * nt + 2 * count:
            bad(f"raw chunk of {size} B for {nt} tiles and {count} levels")
        mb = np.unpackbits(payload[1:1 + 8 * nw * upto], bitorder="little").reshape(upto, nw * 64).astype(bool)
        if mb[:, area:].any():
            bad("raw mask bits set past the tile")
        if int(mb.sum()) > count:
            bad("raw masks hold more levels than the index says")
        bits[:] = mb[:, :area]
        lv = payload[1 + 8 * nw * nt:].view("<i2").astype(np.int64)
        vals[bits] = lv[:int(mb.sum())]
        return bits, vals
    v = int.from_bytes(payload.tobytes(), "little")
    end = 8 * size
    kd, ka = (v >> 1) & 7, (v >> 4) & 7
    pos = 7

    def eg(k):
        nonlocal pos
        rest = v >> pos
        z = (rest & -rest).bit_length() - 1 if rest else 64
        if z > MAX_PREFIX:
            bad("an Exp-Golomb prefix of more than 24 zeros")
        n = z + k
        if pos + z + 1 + n > end:
            bad("decodes past its size")
        w = (1 << n) | ((rest >> (z + 1)) & ((1 << n) - 1))
        pos += z + 1 + n
        return w - (1 << k)

    def unsgn(u):
        return (u + 1) >> 1 if u & 1 else -(u >> 1)

    written, dcp = 0, 0
    for t in range(upto):
        dcp += unsgn(eg(kd))
        if not -32768 <= dcp <= 32767:
            bad("a DC level outside int16")
        if dcp:
            written += 1
            vals[t, 0], bits[t, 0] = dcp, True
        nac = eg(0)
        if nac > area - 1:
            bad("an AC count outside the tile")
        p = 0
        for _ in range(nac):
            p += eg(0) + 1
            if p > area - 1:
                bad("a run past the tile")
            lvl = unsgn(eg(ka))
            if not -32768 <= lvl <= 32767:
                bad("an AC level outside int16")
            written += 1
            vals[t, p], bits[t, p] = lvl, True
        if written > count:
            bad(f"decodes to more than the {count} levels of its index entry")
    return bits, vals


def _encode_chunk(bits: np.ndarray, vals: np.ndarray, nw: int) -> Tuple[bytes, int]:
    """One chunk (bits, values (nt, area)) as encode_frame codes it -> (payload, levels): the k_dc and k_ac of the fewest bits (ties: the
    smallest), raw when strictly smaller or when a set mask bit holds level 0."""
    nt, area = bits.shape
    cnt = int(bits.sum())
    dc = vals[:, 0]
    udc = _sgn(dc - np.concatenate([[0], dc[:-1]]))
    ac_t, ac_p = np.nonzero(bits[:, 1:])
    ac_p = ac_p + 1
    nac = np.bincount(ac_t, minlength=nt).astype(np.int64)
    new_tile = np.concatenate([[True], ac_t[1:] != ac_t[:-1]]) if ac_t.size else np.zeros(0, bool)
    run = ac_p - np.where(new_tile, 0, np.concatenate([[0], ac_p[:-1]])) - 1
    uac = _sgn(vals[ac_t, ac_p])
    dc_bits = [int(_eg_len(udc, k).sum()) for k in range(8)]
    ac_bits = [int(_eg_len(uac, k).sum()) for k in range(8)]
    kd, ka = int(np.argmin(dc_bits)), int(np.argmin(ac_bits))
    coded_bytes = (7 + int(_eg_len(nac, 0).sum()) + int(_eg_len(run, 0).sum()) + dc_bits[kd] + ac_bits[ka] + 7) // 8
    raw_bytes = 1 + 8 * nw * nt + 2 * cnt
    if bool((bits & (vals == 0)).any()) or raw_bytes < coded_bytes:
        pad = np.zeros((nt, nw * 64), bool)
        pad[:, :area] = bits
        return b"\x01" + np.packbits(pad, axis=-1, bitorder="little").tobytes() + vals[bits].astype("<i2").tobytes(), cnt
    acc, pos = kd << 1 | ka << 4, 7

    def put(u, k):
        nonlocal acc, pos
        w = int(u) + (1 << k)
        n = w.bit_length() - 1
        pos += n - k
        acc |= (1 | (w & ((1 << n) - 1)) << 1) << pos
        pos += n + 1

    j = 0
    for t in range(nt):
        put(udc[t], kd)
        put(nac[t], 0)
        for _ in range(int(nac[t])):
            put(run[j], 0)
            put(uac[j], ka)
            j += 1
    assert (pos + 7) // 8 == coded_bytes
    return acc.to_bytes(coded_bytes, "little"), cnt


def chunk_classes(svce, window) -> np.ndarray:
    """Per chunk of a well-formed SVCE frame: 0 kept whole, 1 dropped whole, 2 cut by a vertical edge of the window (None: all kept)."""
    return _window_frame(svce, window)[1]


def _window_frame(svce, window) -> Tuple[bytes, np.ndarray]:
    from . import layers
    b = _u8(svce)
    hdr, sizes, counts = parse_frame(b)
    g = _Geom(hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"], hdr["mv_block_w"], hdr["mv_block_h"], hdr["chunk_tiles"])
    types = _decode_types(b[HEADER_BYTES:HEADER_BYTES + hdr["types_bytes"]], g.mvb)
    if 1 + (8 * g.nw + 2 * g.area) * min(g.ct, g.tx) > 0xFFFF:
        raise ValueError(f"SVCE chunk_tiles {g.ct}: a raw chunk of {min(g.ct, g.tx)} tiles is above the index's u16, so a cut chunk could not "
                         "always be written")
    keep = np.ones((g.ty, g.tx), bool)
    if window is not None:
        lh = {k: hdr[k] for k in layers.GEOMETRY}
        _, ox, oy = layers._tile_maps(lh, types.reshape(g.mfh, g.mfw))
        keep = layers._contains(window, ox, oy)
    C = g.chunks
    payload_off = HEADER_BYTES + hdr["types_bytes"] + 4 * C
    start = payload_off + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    cls = np.zeros(C, np.int64)
    out_payload, out_count, empty = [], [], {}
    for c in range(C):
        row, t0 = divmod(c, g.cx)
        t0 *= g.ct
        nt = int(g.chunk_nt[c])
        k = keep[row % g.ty, t0:t0 + nt]
        if k.all():
            out_payload.append(b[start[c]:start[c] + sizes[c]].tobytes())
            out_count.append(int(counts[c]))
        elif not k.any():
            cls[c] = 1
            if nt not in empty:
                empty[nt] = _encode_chunk(np.zeros((nt, g.area), bool), np.zeros((nt, g.area), np.int64), g.nw)[0]
            out_payload.append(empty[nt])
            out_count.append(0)
        else:
            cls[c] = 2
            hi = int(np.flatnonzero(k)[-1]) + 1
            bits = np.zeros((nt, g.area), bool)
            vals = np.zeros((nt, g.area), np.int64)
            bits[:hi], vals[:hi] = _walk_chunk(b[start[c]:start[c] + sizes[c]], int(counts[c]), nt, hi, g, c)
            bits[~k], vals[~k] = False, 0
            pay, cnt = _encode_chunk(bits, vals, g.nw)
            out_payload.append(pay)
            out_count.append(cnt)
    out_sizes = np.array([len(p) for p in out_payload], np.int64)
    level_count = int(sum(out_count))
    frame_bytes = _up(payload_off + int(out_sizes.sum()), 16)
    if frame_bytes > _up(g.levels_off + 6 * g.w * g.h + 4 + 5 * 3 * g.ty * g.tx, 16):
        raise ValueError(f"the windowed frame of {frame_bytes} B is above the worst canonical frame: kept chunks larger than their raw form")
    words = b[:HEADER_BYTES].view("<u4").copy()
    words[10], words[12], words[13] = level_count, frame_bytes, g.svcq_bytes(level_count)
    index = (out_sizes | (np.array(out_count, np.int64) << 16)).astype("<u4")
    body = words.tobytes() + b[HEADER_BYTES:HEADER_BYTES + hdr["types_bytes"]].tobytes() + index.tobytes() + b"".join(out_payload)
    return body + bytes(frame_bytes - len(body)), cls


def window_frame(svce, window) -> bytes:
    """One SVCE frame restricted to the tiles whose origin the window (x, y, w, h in padded coordinates, or None: every tile) contains,
    on its coded bytes and its own chunk grid: what svc_hip_window_entropy_frames writes.  A chunk whose tiles are all kept keeps its
    payload and index entry, canonical or not; a chunk with no kept tile becomes the empty coded chunk (ceil((7 + 2 nt) / 8) bytes, no
    levels); a chunk a vertical window edge cuts is read up to its last kept tile and coded again as encode_frame codes it, with the
    tiles outside the window all zero.  Header words 0 .. 9, 11, 14, 15 and the types section as they are; word 10 the output chunks'
    levels, word 13 the SVCQ frame's bytes for them, word 12 this frame's.  For a frame this module's encoder wrote the result is
    encode_frame(layers.window_frame(decode_frame(svce), window), chunk_tiles=the frame's).  ValueError where the device call flags the
    frame: parse_frame's checks, a types section decode_frame rejects, a chunk_tiles whose raw chunk is above 65535 B, a cut chunk whose
    read part is malformed, an output above the worst canonical frame.  What lies outside the read part of a cut chunk, or inside a
    kept or a dropped chunk, is not read: it passes through or is dropped, as on the device."""
    return _window_frame(svce, window)[0]


def window_frames(stream, offsets, windows, src=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_window_entropy_frames writes for frames that pass their checks -> (bytes, offsets (n_out + 1,) u64); windows and src
    as layers.window_frames takes them."""
    b = _u8(stream)
    offs = [int(o) for o in np.asarray(offsets).reshape(-1)]
    n_in = len(offs) - 1
    idx = list(range(n_in)) if src is None else [int(i) for i in np.asarray(src).reshape(-1)]
    win = None if windows is None else np.asarray(windows).reshape(len(idx), 4)
    frames = []
    for i, f in enumerate(idx):
        if not 0 <= f < n_in:
            raise ValueError(f"output frame {i} names input frame {f} of {n_in}")
        lo, hi = offs[f], offs[f + 1]
        if lo % 16 or hi < lo or hi > b.size:
            raise ValueError(f"SVCE frame offsets out of order, misaligned or past the stream: {lo}, {hi}")
        if parse_frame(b[lo:hi])[0]["frame_bytes"] != hi - lo:
            raise ValueError(f"SVCE frame at {lo} has a frame_bytes other than its offsets' {hi - lo}")
        frames.append(window_frame(b[lo:hi], None if win is None else win[i]))
    return _join(frames)
