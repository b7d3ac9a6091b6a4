"""The two layers of a gaze-scalable compact stream (include/svc_hip.h, "Two layers"), stated in numpy on top of the host reader of
SVCQ frames (levels.parse_frame): what svc_hip_dct_pack_layers_frames writes as its enhancement stream, given the base stream and the
stream encoded at (enh_step, enh_step), and the levels and steps svc_hip_decode_layers_frames dequantises.  A consumer needs neither a
GPU nor the native library.

For a tile of class c (background when the MV block holding its origin has type 0), sb = c's base step and ratio = sb / enh_step (the
steps divide).  Per coefficient, with Lb its level in the base frame and Lf its level at enh_step:
    d = Lf - Lb * ratio     inside the frame's window, 0 outside it
and an enhancement frame is an SVCQ frame whose levels are d, with fg_step = bg_step = enh_step in its header.  Inside the gaze the
decoder dequantises (Lb * ratio + d) * enh_step, elsewhere Lb * sb.

reduced_coefficients / decode_layers_reduced_frame state svc_hip_decode_layers_reduced_frames: the same two layers decoded at 1 / reduce of
the size from the first K x K coefficients of every tile, on top of levels.reduced_coefficients.

window_frame / window_frames state svc_hip_window_levels_frames: a stored frame restricted to the tiles of a window, on its masks.

band_frame / band_frames state svc_hip_band_levels_frames: a stored frame restricted to a frequency band of every tile (and a window), on
its masks; union_frame / union_frames state svc_hip_union_levels_frames, which joins such parts back.

delta_frame / delta_frames state svc_hip_delta_levels_frames: a frame coded against the frame before it, as the difference of their levels
in the tiles both code at one step; undelta_frame / undelta_frames state svc_hip_undelta_levels_frames, which adds the frames back up.
delta_level_counts / auto_keys / delta_auto_frames state the key frames svc_hip_dct_pack_delta_auto_frames chooses by the frame's size.
delta_groups / delta_ladder_counts / delta_budget_choice / delta_budget_frames state svc_hip_dct_pack_delta_budget_frames
(include/svc_hip_delta_budget.h): one pair of steps per group of frames, from a key frame up to the next, by a byte budget on the group.
temporal_ref / delta_temporal_frames / undelta_temporal_frames / thin_frames / temporal_statuses state the temporal layers of the delta
stream (svc_hip_delta_levels_temporal_frames, svc_hip_undelta_levels_temporal_frames): frame i coded against frame i - min(lowbit(i), period),
so that every 2^s-th frame is the stream of period >> s of the thinned clip.

split_frame / split_frames / split_budget_frames state svc_hip_split_levels_frames and its budgeted form: the stream stored at
(fine_step, fine_step) alone determines a base frame at any multiples of fine_step and the enhancement frame that lifts it back, in
integers on the levels' values:
    Lb = sign(Lf) * ((2 |Lf| + r) // (2 r))     Lf / r rounded half away from zero, r = sb / fine_step
    d  = Lf - Lb * r                            inside the window, 0 outside it
Lb * r + d == Lf for any r.  For odd r (both classes) Lb is the level a direct quantisation at sb gives, so the two frames are the
encoder's own; for even r a level that is an odd multiple of r / 2 is a tie the coefficient would have resolved either way, and the base
differs from a direct encode there.

pack_layers_frames states svc_hip_pack_layers_frames: both layers from raw coefficient planes, each level quantised from the coefficient
itself, so the base is the direct encode for any ratio.

distortion_table / quality_choice / distortion_target / distortion_psnr state svc_hip_dct_pack_levels_quality_frames
(include/svc_hip_quality.h): the squared error every ladder entry would leave, in integers, and the per-frame choice by it."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import levels

GEOMETRY = ("frame_w", "frame_h", "block_w", "block_h", "mv_block_w", "mv_block_h")


def _tile_maps(hdr: Dict[str, int], types: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per tile (tiles_y, tiles_x): is it background, and its origin's x and y."""
    tx, ty = hdr["frame_w"] // hdr["block_w"], hdr["frame_h"] // hdr["block_h"]
    ox, oy = np.arange(tx) * hdr["block_w"], np.arange(ty) * hdr["block_h"]
    background = types[(oy // hdr["mv_block_h"])[:, None], (ox // hdr["mv_block_w"])[None, :]] == 0
    return background, np.broadcast_to(ox[None, :], (ty, tx)), np.broadcast_to(oy[:, None], (ty, tx))


def _per_pixel(hdr: Dict[str, int], per_tile: np.ndarray) -> np.ndarray:
    return np.repeat(np.repeat(per_tile, hdr["block_h"], 0), hdr["block_w"], 1)


def _contains(rect, ox: np.ndarray, oy: np.ndarray) -> np.ndarray:
    """The containment rule of the gaze and of the window: the rectangle x, y, w, h holds the tile origin; w or h of 0 holds nothing."""
    x, y, w, h = (int(v) for v in rect)
    return (ox >= x) & (ox - x < w) & (oy >= y) & (oy - y < h)


def _levels_of(hdr: Dict[str, int], types: np.ndarray, planes: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """parse_frame's planes (level * step, rounded to f32) back to the integer levels (3, H, W) i64, and the step of each tile.  The
    f32 rounding moves level * step by at most 2^-24 of itself, that is the quotient by less than 2^-9: rint gives the level back."""
    background, _, _ = _tile_maps(hdr, types)
    step = np.where(background, hdr["bg_step"], hdr["fg_step"]).astype(np.int64)
    lv = np.rint(planes.astype(np.float64) / _per_pixel(hdr, step)[None]).astype(np.int64)
    return lv, step


def _assemble(head, inexact: int, types: np.ndarray, masks: np.ndarray, lv: np.ndarray) -> bytes:
    """An SVCQ frame from its header words 0 .. 9, the region ids, the mask section's bytes and the levels in stream order: word 10 is
    their number, word 12 the frame's bytes, the reserved words and the padding zero."""
    body = np.ascontiguousarray(types, "<u4").tobytes() + np.ascontiguousarray(masks, np.uint8).tobytes() + np.asarray(lv).astype("<i2").tobytes()
    size = (levels.HEADER_BYTES + len(body) + 15) // 16 * 16
    words = np.array([int(v) for v in head[:10]] + [len(lv), inexact, size, 0, 0, 0], "<u4").tobytes()
    return words + body + bytes(size - levels.HEADER_BYTES - len(body))


def write_frame(hdr: Dict[str, int], types: np.ndarray, lv: np.ndarray, fg_step: int, bg_step: int, inexact: int = 0) -> bytes:
    """An SVCQ frame of hdr's geometry with the region ids `types` and the integer levels lv (3, H, W); header word 11 = inexact."""
    w, h, bw, bh = hdr["frame_w"], hdr["frame_h"], hdr["block_w"], hdr["block_h"]
    tx, ty, area = w // bw, h // bh, bw * bh
    nw = (area + 63) // 64
    if lv.min(initial=0) < -32768 or lv.max(initial=0) > 32767:
        raise ValueError("a level outside int16")
    tiles = lv.reshape(3, ty, bh, tx, bw).transpose(0, 1, 3, 2, 4).reshape(3, ty, tx, area)
    nz = tiles != 0
    bits = np.zeros((3, ty, tx, nw * 64), bool)
    bits[..., :area] = nz
    masks = np.packbits(bits, axis=-1, bitorder="little")
    head = [levels.MAGIC, levels.VERSION, w, h, bw, bh, hdr["mv_block_w"], hdr["mv_block_h"], fg_step, bg_step]
    return _assemble(head, inexact, types, masks, tiles[nz])


def _belongs(hb: Dict[str, int], he: Dict[str, int]) -> bool:
    """Is `he` the header of an enhancement (or fine) frame of the base frame `hb`: one step, which divides both base steps?"""
    e = he["fg_step"]
    return e != 0 and he["bg_step"] == e and hb["fg_step"] % e == 0 and hb["bg_step"] % e == 0


def enhancement_frame(base_frame, fine_frame, enh_step: int, window=None) -> bytes:
    """One enhancement frame from the base frame and the frame encoded at (enh_step, enh_step); window: x, y, w, h or None."""
    hb, types, pb = levels.parse_frame(base_frame)
    hf, types_f, pf = levels.parse_frame(fine_frame)
    if any(hb[k] != hf[k] for k in GEOMETRY) or not np.array_equal(types, types_f):
        raise ValueError("the base and the fine frame differ in geometry or region ids")
    if hf["fg_step"] != enh_step or not _belongs(hb, hf):
        raise ValueError(f"the fine frame's steps ({hf['fg_step']}, {hf['bg_step']}) are not ({enh_step}, {enh_step}), or enh_step does "
                         f"not divide the base steps ({hb['fg_step']}, {hb['bg_step']})")
    lb, step = _levels_of(hb, types, pb)
    lf, _ = _levels_of(hf, types, pf)
    d = lf - lb * _per_pixel(hb, step // enh_step)[None]
    if window is not None:
        _, ox, oy = _tile_maps(hb, types)
        d = np.where(_per_pixel(hb, _contains(window, ox, oy))[None], d, 0)
    return write_frame(hb, types, d, enh_step, enh_step)


def enhancement_frames(base, base_offsets, fine, fine_offsets, enh_step: int, window=None) -> Tuple[bytes, np.ndarray]:
    """The enhancement stream of a batch -> (bytes, offsets (n + 1,) u64): frame f from base frame f and fine frame f (the stream
    encoded at (enh_step, enh_step)); window: None (every tile is enhanced) or per frame x, y, w, h in padded coordinates (n, 4)."""
    b = np.frombuffer(base, np.uint8) if not isinstance(base, np.ndarray) else base.reshape(-1).view(np.uint8)
    f = np.frombuffer(fine, np.uint8) if not isinstance(fine, np.ndarray) else fine.reshape(-1).view(np.uint8)
    bo = [int(o) for o in np.asarray(base_offsets).reshape(-1)]
    fo = [int(o) for o in np.asarray(fine_offsets).reshape(-1)]
    if len(bo) != len(fo):
        raise ValueError("the two streams hold different numbers of frames")
    n = len(bo) - 1
    win = None if window is None else np.asarray(window).reshape(n, 4)
    frames = [enhancement_frame(b[bo[i]:bo[i + 1]], f[fo[i]:fo[i + 1]], enh_step, None if win is None else win[i]) for i in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.uint64)
    return b"".join(frames), offs


def merge_levels(base_frame, enh_frame, gaze: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """What the decoder dequantises -> (levels (3, H, W) i64, steps (tiles_y, tiles_x) i64): for a tile whose origin the gaze rectangle
    (x, y, w, h, or None) contains, Lb * ratio + d at the enhancement's step; for every other tile the base frame's levels and step.
    Raises for an enhancement frame that does not belong to the base frame (the decoder's status 0x100 | 11)."""
    hb, types, pb = levels.parse_frame(base_frame)
    lb, step = _levels_of(hb, types, pb)
    if gaze is None:
        return lb, step
    he, _, pe = levels.parse_frame(enh_frame)
    if any(hb[k] != he[k] for k in GEOMETRY):
        raise ValueError("the base and the enhancement frame differ in geometry")
    if not _belongs(hb, he):
        raise ValueError(f"an enhancement frame with steps ({he['fg_step']}, {he['bg_step']}) is not a layer of a base frame with "
                         f"({hb['fg_step']}, {hb['bg_step']})")
    e = he["fg_step"]
    d = np.rint(pe.astype(np.float64) / e).astype(np.int64)  # one step for every tile, whatever the region ids
    _, ox, oy = _tile_maps(hb, types)
    gazed = _contains(gaze, ox, oy)
    merged = np.where(_per_pixel(hb, gazed)[None], lb * _per_pixel(hb, step // e)[None] + d, lb)
    return merged, np.where(gazed, e, step)


# ---- the two layers decoded at reduced size (include/svc_hip.h: svc_hip_decode_layers_reduced_frames) --------------------------------

def _reduced(base_frame, enh_frame, reduce: int, fg_step: int, bg_step: int, gaze) -> Tuple[np.ndarray, int]:
    """reduced_coefficients and its K."""
    out, k = levels._reduced(base_frame, reduce, fg_step, bg_step, None)  # every tile as a tile outside the gaze
    if gaze is None:
        return out, k
    merged, step = merge_levels(base_frame, enh_frame, gaze)  # raises for an enhancement frame that is not this base frame's
    hb, types, _ = levels.parse_frame(base_frame)
    n = hb["block_w"]
    _, ox, oy = _tile_maps(hb, types)
    gazed = _contains(gaze, ox, oy)
    ty, tx = gazed.shape
    c = merged.astype(np.float32) * _per_pixel(hb, step)[None].astype(np.float32)  # a gazed tile: (f32)(Lb * ratio + d) * (f32)enh_step
    tiles = c.reshape(3, ty, n, tx, n)[:, :, :k, :, :k]
    q = (tiles / np.float32(1)).astype(np.float32).astype(np.float64)
    r = np.copysign(np.floor(np.abs(q) + 0.5), q).astype(np.float32)
    lifted = (r * np.float32(1)).astype(np.float32) * np.float32(k / n)
    out = np.where(gazed[None, :, None, :, None], lifted, out.reshape(3, ty, k, tx, k))
    return np.ascontiguousarray(out.reshape(3, ty * k, tx * k), np.float32), k


def reduced_coefficients(base_frame, enh_frame, reduce: int, fg_step: int, bg_step: int, gaze: Optional[Sequence[int]] = None
                         ) -> np.ndarray:
    """What the reduced decoder of two layers inverts -> (3, H / reduce, W / reduce) f32, laid out as levels.reduced_coefficients lays
    it out: the first K x K coefficients of every N x N tile, K = N / reduce.  A tile whose origin (in full-size padded coordinates) the
    gaze rectangle x, y, w, h does not contain, and every tile for gaze None: exactly levels.reduced_coefficients on the base frame.  A
    gazed tile: level = Lb * ratio + d of merge_levels (d = 0 where the enhancement's mask bit is clear, ratio = the tile's base step /
    the enhancement's step), c = (f32)level * (f32)enh_step, requantised at step 1 and scaled by K / N, every operation one f32
    operation as there (roundf in f64 on the f32 quotient).  reduce = 1: the full layered decoder's requantised coefficients.  enh_frame
    is not read for gaze None; otherwise raises ValueError where merge_levels raises."""
    return _reduced(base_frame, enh_frame, reduce, fg_step, bg_step, gaze)[0]


def decode_layers_reduced_frame(base_frame, enh_frame, reduce: int, fg_step: int, bg_step: int,
                                gaze: Optional[Sequence[int]] = None) -> np.ndarray:
    """The reduced decoder's picture of two layers before its rounding to f32 -> (H / reduce, W / reduce, 3) f64 B,G,R: the K-point
    inverse DCT-II along rows and columns of every K x K tile of reduced_coefficients, as levels.decode_reduced_frame takes it."""
    coef, k = _reduced(base_frame, enh_frame, reduce, fg_step, bg_step, gaze)
    coef = coef.astype(np.float64)
    c = levels._basis(k)
    _, rh, rw = coef.shape
    t = coef.reshape(3, rh // k, k, rw // k, k)
    x = np.einsum("vy,pavbu,ux->paybx", c, t, c)
    return np.ascontiguousarray(x.reshape(3, rh, rw).transpose(1, 2, 0))


# ---- a stored stream restricted to a window (include/svc_hip.h: svc_hip_window_levels_frames) -----------------------------------------

def _sections(frame):
    """A frame levels.parse_frame accepts -> (u8 view, header dict, types, mask bytes (3, ty, tx, nw * 8), levels i16 in stream order)."""
    b = np.frombuffer(frame, np.uint8) if not isinstance(frame, np.ndarray) else frame.reshape(-1).view(np.uint8)
    hdr, types, _ = levels.parse_frame(b)  # raises for a frame the reader rejects: the masks and the level count below are sound
    tx, ty = hdr["frame_w"] // hdr["block_w"], hdr["frame_h"] // hdr["block_h"]
    nw = (hdr["block_w"] * hdr["block_h"] + 63) // 64
    masks_off = levels.HEADER_BYTES + 4 * types.size
    levels_off = masks_off + 8 * 3 * ty * tx * nw
    return b, hdr, types, b[masks_off:levels_off].reshape(3, ty, tx, nw * 8), b[levels_off:levels_off + 2 * hdr["level_count"]].view("<i2")


def _window_frame(frame, window) -> Tuple[bytes, Dict[str, int]]:
    b, hdr, types, masks, lv = _sections(frame)
    keep = np.ones(masks.shape[1:3], bool)
    if window is not None:
        _, ox, oy = _tile_maps(hdr, types)
        keep = _contains(window, ox, oy)
    bits = np.unpackbits(masks, axis=-1, bitorder="little").astype(bool)  # the levels follow the set bits in this (C) order
    kept_bits = bits & keep[None, :, :, None]
    out_masks = np.where(keep[None, :, :, None], masks, 0)
    return _assemble(b[:40].view("<u4"), hdr["inexact"], types, out_masks, lv[kept_bits[bits]]), hdr


def window_frame(frame, window) -> bytes:
    """One SVCQ frame restricted to the tiles whose origin the window (x, y, w, h in padded coordinates, or None: every tile) contains:
    header words 0 .. 9 and 11 and the types as they are, a kept tile's mask words as they are and every other tile's zero, the kept
    tiles' levels in the frame's order, word 10 their number, word 12 the new size, zero padding.  Stated on the masks, not on the levels'
    values: a set bit whose level is 0 stays a set bit and keeps its level.  On enhancement_frame(base, fine, e, None) this gives
    enhancement_frame(base, fine, e, window).  Raises ValueError for a frame levels.parse_frame rejects."""
    return _window_frame(frame, window)[0]


def window_frames(stream, offsets, windows, src=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_window_levels_frames writes for frames that pass their checks -> (bytes, offsets (n_out + 1,) u64): output frame i
    is window_frame of input frame src[i] (src None: frame i) and windows[i]; windows: None (every tile of every frame) or per output
    frame x, y, w, h (n_out, 4); src: indices into the input frames, repeats and any order allowed."""
    b = np.frombuffer(stream, np.uint8) if not isinstance(stream, np.ndarray) else stream.reshape(-1).view(np.uint8)
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
            raise ValueError(f"SVCQ frame offsets out of order, misaligned or past the stream: {lo}, {hi}")
        out, hdr = _window_frame(b[lo:hi], None if win is None else win[i])
        if hdr["frame_bytes"] != hi - lo:
            raise ValueError(f"SVCQ frame at {lo} has frame_bytes {hdr['frame_bytes']}, its offsets {hi - lo}")
        frames.append(out)
    out_offs = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.uint64)
    return b"".join(frames), out_offs


# ---- a stored stream restricted to a frequency band, and bands joined back (include/svc_hip.h: svc_hip_band_levels_frames,
# svc_hip_union_levels_frames) ------------------------------------------------------------------------------------------------------------

def _band_bits(hdr: Dict[str, int], band) -> np.ndarray:
    """(nw * 64,) bool: the coefficients of a tile, in mask-bit order, that the band lo_w, lo_h, hi_w, hi_h (or None: all) keeps."""
    bw, bh = hdr["block_w"], hdr["block_h"]
    lo_w, lo_h, hi_w, hi_h = (0, 0, bw, bh) if band is None else (int(v) for v in band)
    r, c = np.arange(bh)[:, None], np.arange(bw)[None, :]
    keep = (r < hi_h) & (c < hi_w) & ~((r < lo_h) & (c < lo_w))
    bits = np.zeros((bw * bh + 63) // 64 * 64, bool)
    bits[:bw * bh] = keep.reshape(-1)
    return bits


def band_frame(frame, band, window=None) -> bytes:
    """One SVCQ frame restricted to a frequency band and a window: coefficient (row r, column c) of a tile is kept iff the window (x, y,
    w, h in padded coordinates, or None: every tile) contains the tile's origin and
        r < hi_h and c < hi_w and not (r < lo_h and c < lo_w)
    for band = (lo_w, lo_h, hi_w, hi_h) (None: every coefficient; a hi above the tile side means the side).  Header words 0 .. 9 and 11
    and the types as they are, every mask word ANDed with the band's bits (zero outside the window), the kept levels in the frame's order,
    word 10 their number, word 12 the new size, zero padding.  Stated on the masks, as window_frame is: a set bit whose level is 0 stays
    set.  band_frame(f, None, window) == window_frame(f, window); the bands (0, 0, K1, K1), (K1, K1, K2, K2), (K2, K2, bw, bh) partition
    a tile.  Raises ValueError for a frame levels.parse_frame rejects."""
    b, hdr, types, masks, lv = _sections(frame)
    keep = np.ones(masks.shape[1:3], bool)
    if window is not None:
        _, ox, oy = _tile_maps(hdr, types)
        keep = _contains(window, ox, oy)
    bits = np.unpackbits(masks, axis=-1, bitorder="little").astype(bool)  # the levels follow the set bits in this (C) order
    kept_bits = bits & keep[None, :, :, None] & _band_bits(hdr, band)[None, None, None, :]
    return _assemble(b[:40].view("<u4"), hdr["inexact"], types, np.packbits(kept_bits, axis=-1, bitorder="little"), lv[kept_bits[bits]])


def band_frames(stream, offsets, bands, windows=None, src=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_band_levels_frames writes for frames that pass their checks -> (bytes, offsets (n_out + 1,) u64): output frame i is
    band_frame of input frame src[i] (src None: frame i), bands[i] and windows[i]; bands: None (every coefficient) or per output frame
    lo_w, lo_h, hi_w, hi_h (n_out, 4); windows, src as window_frames takes them."""
    frames = _source_frames(stream, offsets, src)
    band = None if bands is None else np.asarray(bands).reshape(len(frames), 4)
    win = None if windows is None else np.asarray(windows).reshape(len(frames), 4)
    return _join([band_frame(fr, None if band is None else band[i], None if win is None else win[i]) for i, fr in enumerate(frames)])


def union_frame(a, b) -> bytes:
    """Two frames of one geometry, the same steps and types and disjoint masks -> the frame whose masks are theirs ORed and whose levels
    are both frames' in coefficient order; header words 0 .. 9 and 11 and the types are a's.  The bands of a partition of a frame, joined
    in any order, give the frame back.  Raises ValueError for a frame levels.parse_frame rejects, for a pair that does not belong together
    (the device's status 0x100 | 11) and for masks that share a bit (status 12)."""
    ba, ha, types, ma, la = _sections(a)
    _, hb, types_b, mb, lb = _sections(b)
    if any(ha[k] != hb[k] for k in GEOMETRY):
        raise ValueError("the two frames differ in geometry")
    if (ha["fg_step"], ha["bg_step"]) != (hb["fg_step"], hb["bg_step"]) or not np.array_equal(types, types_b):
        raise ValueError("the two frames differ in steps or region ids: they are not parts of one frame")
    bits_a = np.unpackbits(ma, axis=-1, bitorder="little").astype(bool)
    bits_b = np.unpackbits(mb, axis=-1, bitorder="little").astype(bool)
    if (bits_a & bits_b).any():
        raise ValueError("the two frames' masks overlap")
    vals = np.zeros(bits_a.shape, np.int16)
    vals[bits_a] = la
    vals[bits_b] = lb
    both = bits_a | bits_b
    return _assemble(ba[:40].view("<u4"), ha["inexact"], types, ma | mb, vals[both])


def union_frames(a, a_offsets, b, b_offsets) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_union_levels_frames writes for pairs that pass their checks -> (bytes, offsets (n + 1,) u64): frame i is union_frame
    of frame i of each stream."""
    fa, fb = _source_frames(a, a_offsets, None), _source_frames(b, b_offsets, None)
    if len(fa) != len(fb):
        raise ValueError("the two streams hold different numbers of frames")
    return _join([union_frame(x, y) for x, y in zip(fa, fb)])


# ---- frames coded against their predecessors in levels, and back (include/svc_hip.h: svc_hip_delta_levels_frames,
# svc_hip_undelta_levels_frames) ------------------------------------------------------------------------------------------------------------

def _dense(frame):
    """_sections with the levels at their coefficients -> (u8 view, header dict, types, levels (3, ty, tx, nw * 64) i16, step of each tile
    (ty, tx) i64).  A level is 0 where the mask bit is clear; a set bit whose level is 0 reads as 0."""
    b, hdr, types, masks, lv = _sections(frame)
    bits = np.unpackbits(masks, axis=-1, bitorder="little").astype(bool)  # the levels follow the set bits in this (C) order
    vals = np.zeros(bits.shape, np.int16)
    vals[bits] = lv
    background, _, _ = _tile_maps(hdr, types)
    return b, hdr, types, vals, np.where(background, hdr["bg_step"], hdr["fg_step"]).astype(np.int64)


def _chained(cur, prev, sign: int) -> bytes:
    """cur's levels plus sign * prev's in the tiles both frames code at one step, modulo 2^16, as an SVCQ frame with cur's header words
    0 .. 9 and 11 and types; prev None: cur's levels."""
    b, hdr, types, vals, step = _dense(cur)
    if prev is not None:
        _, hp, _, pvals, pstep = _dense(prev)
        if any(hdr[k] != hp[k] for k in GEOMETRY):
            raise ValueError("the frame and its predecessor differ in geometry")
        predicted = (step == pstep)[None, :, :, None]
        vals = (vals.astype(np.int64) + sign * np.where(predicted, pvals, 0)).astype(np.uint16).view(np.int16)  # two's complement wrap-around
    nz = vals != 0
    return _assemble(b[:40].view("<u4"), hdr["inexact"], types, np.packbits(nz, axis=-1, bitorder="little"), vals[nz])


def delta_frame(cur, prev=None) -> bytes:
    """One SVCQ frame coded against its predecessor, in levels.  With L_F the int16 level of every coefficient of frame F (0 where the
    mask bit is clear; a set bit whose level is 0 reads as 0) and step_F(tile) F's bg_step where the MV block holding the tile's origin
    has type 0, else its fg_step, a tile is predicted iff prev is given and step_cur(tile) == step_prev(tile), and
        D = L_cur - (L_prev in a predicted tile, else 0)     modulo 2^16, as int16
    Nothing overflows and no frame is refused for its values.  The result is again an SVCQ frame: header words 0 .. 9 and 11 and the types
    are cur's, a mask bit is set iff D != 0, the levels are D in coefficient order, word 10 their number, word 12 the size, words 13 .. 15
    and the padding zero.  Nothing in it says that it holds differences: the caller knows, as for an enhancement frame.  prev None: a key
    frame, D = L_cur.  window_frame and band_frame, applied with one window or band to cur and prev, commute with delta_frame.  Raises
    ValueError for a frame levels.parse_frame rejects and for two frames of different geometry."""
    return _chained(cur, prev, -1)


def undelta_frame(diff, prev_rec=None) -> bytes:
    """delta_frame undone: L = D + (L_prev_rec in a predicted tile, else 0), modulo 2^16, written the same way (a mask bit set iff
    L != 0).  Which tiles are predicted follows from diff's header and types and prev_rec's, which are cur's and prev's because both calls
    copy them: undelta_frame(delta_frame(cur, prev), prev) is cur with the set bits of level 0 cleared, byte for byte cur for a frame
    without such bits -- every frame the packers and write_frame write.  prev_rec None: a key frame."""
    return _chained(diff, prev_rec, +1)


def _keys(keys, n: int):
    return np.zeros(n, bool) if keys is None else np.asarray(keys).reshape(n) != 0


def delta_frames(stream, offsets, keys=None, prev=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_delta_levels_frames writes for frames that pass their checks -> (bytes, offsets (n + 1,) u64): frame i is a key
    frame if it has no predecessor or keys[i] != 0 (keys None: no flag is set); otherwise it is delta_frame of input frame i and its
    predecessor, input frame i - 1, for frame 0 the frame `prev` (None: frame 0 is a key frame).  A stream cut into two calls at any
    frame, the second with prev = the first's last input frame, gives the bytes of one call."""
    frames = _source_frames(stream, offsets, None)
    key = _keys(keys, len(frames))
    return _join([delta_frame(fr, None if key[i] else (frames[i - 1] if i else prev)) for i, fr in enumerate(frames)])


def undelta_frames(stream, offsets, keys=None, prev=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_undelta_levels_frames writes for frames that pass their checks -> (bytes, offsets (n + 1,) u64): delta_frames undone
    with the same keys.  The predecessor of frame i is OUTPUT frame i - 1, for frame 0 the reconstructed frame `prev`:
    undelta_frames(*delta_frames(s, o, keys), keys) gives s back for a stream without set bits of level 0.  A stream cut into two calls,
    the second with prev = the first's last output frame, gives the bytes of one call."""
    frames = _source_frames(stream, offsets, None)
    key = _keys(keys, len(frames))
    out = []
    for i, fr in enumerate(frames):
        out.append(undelta_frame(fr, None if key[i] else (out[i - 1] if i else prev)))
    return _join(out)


# ---- temporal layers of the delta stream (include/svc_hip.h: svc_hip_delta_levels_temporal_frames,
# svc_hip_undelta_levels_temporal_frames) ---------------------------------------------------------------------------------------------------

PERIODS = (1, 2, 4)


def temporal_ref(i: int, period: int) -> int:
    """The frame that frame i > 0 of a stream of period 1, 2 or 4 is coded against: i - min(lowbit(i), period), lowbit(i) = i & -i.
    Frame 0 is coded against the frame handed in as `prev` (-period, the last frame of layer 0 before the call).  The frames with
    i % 2^s == 0 (2^s <= period) refer only to each other, and temporal_ref(i, period) // 2^s == temporal_ref(i // 2^s, period >> s)."""
    if period not in PERIODS:
        raise ValueError(f"period {period} (supported: 1, 2, 4)")
    if i <= 0:
        raise ValueError("frame 0 refers to the frame before the call")
    return i - min(i & -i, period)


def delta_temporal_frames(stream, offsets, period: int, keys=None, prev=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_delta_levels_temporal_frames writes for frames that pass their checks -> (bytes, offsets (n + 1,) u64): delta_frames
    with the predecessor of frame i read as INPUT frame temporal_ref(i, period), for frame 0 the frame `prev`, the input frame at index
    -period.  Period 1 is delta_frames.  A stream cut into two calls at a multiple of period, the second with prev = input frame
    cut - period, gives the bytes of one call."""
    frames = _source_frames(stream, offsets, None)
    key = _keys(keys, len(frames))
    return _join([delta_frame(fr, None if key[i] else (frames[temporal_ref(i, period)] if i else prev)) for i, fr in enumerate(frames)])


def undelta_temporal_frames(stream, offsets, period: int, keys=None, prev=None) -> Tuple[bytes, np.ndarray]:
    """What svc_hip_undelta_levels_temporal_frames writes for frames that pass their checks -> (bytes, offsets (n + 1,) u64):
    delta_temporal_frames undone with the same keys; the predecessor of frame i is OUTPUT frame temporal_ref(i, period), for frame 0 the
    reconstructed frame `prev` at index -period.  Period 1 is undelta_frames."""
    frames = _source_frames(stream, offsets, None)
    key = _keys(keys, len(frames))
    out = []
    for i, fr in enumerate(frames):
        out.append(undelta_frame(fr, None if key[i] else (out[temporal_ref(i, period)] if i else prev)))
    return _join(out)


def temporal_statuses(own, period: int, keys=None, prev: Optional[int] = None, chain: bool = True) -> np.ndarray:
    """d_status of the temporal calls from every frame's own unpack code -> (n,) u32: the own code if it is not 0; else 0 for a key frame
    (keys[i] != 0, or frame 0 with prev None); else 0x100 | (s & 0xFF) where the status s of the frame it refers to is not 0.  prev: the
    own code of the frame handed in as d_prev, None where there is none.  chain (the undelta and decode calls): s is the FINAL status of
    output frame temporal_ref(i, period), so a failure runs down the tree of references; not chain (the delta call): s is the input
    frame's own code.  Period 1 is the status of the plain calls."""
    own = [int(c) for c in np.asarray(own).reshape(-1)]
    key = _keys(keys, len(own))
    st = []
    for i, code in enumerate(own):
        if code or key[i] or (i == 0 and prev is None):
            st.append(code)
            continue
        s = int(prev) if i == 0 else (st if chain else own)[temporal_ref(i, period)]
        st.append(0x100 | (s & 0xFF) if s else 0)
    return np.asarray(st, np.uint32)


def thin_frames(stream, offsets, keys, every: int) -> Tuple[bytes, np.ndarray, Optional[np.ndarray]]:
    """Every `every`-th frame of a stream, from frame 0, with its key flag -> (bytes, offsets, keys or None): what a server sends a viewer
    of 1 / every of the frame rate (svc_hip_window_levels_frames with d_src = 0, every, 2 * every, .. and no window writes the same
    bytes).  For every = 2^s <= period, thin_frames of delta_temporal_frames(clip, period, keys) is delta_temporal_frames of the thinned
    clip at period >> s with the thinned keys: at period >> s == 1 the plain delta stream, which every decoder of it takes."""
    if every < 1:
        raise ValueError("every must be at least 1")
    frames = _source_frames(stream, offsets, None)
    kept = range(0, len(frames), every)
    out, offs = _join([bytes(frames[i]) for i in kept])
    return out, offs, None if keys is None else _keys(keys, len(frames))[list(kept)]


# ---- key frames chosen by the SVCQ frame's size (include/svc_hip.h: svc_hip_dct_pack_delta_auto_frames) ------------------------------------

def _level_count(frame: bytes) -> int:
    return int(np.frombuffer(frame, "<u4", 16)[10])


def delta_level_counts(stream, offsets, prev=None, period: int = 1) -> np.ndarray:
    """-> (n, 2) u32: per frame, column 0 the level count of the frame written as a key frame, delta_frame(frame), and column 1 that of
    delta_frame(frame, predecessor) -- header word 10 of the written frame, so a set mask bit over level 0 counts in neither.  The
    predecessor of frame i is input frame i - 1, for frame 0 the frame `prev`; a frame without one (frame 0, prev None) has column 1
    equal to column 0.  No key flag enters the counts: the levels of the frame before are its own, however it is coded, so a row is a
    function of its frame and that frame's predecessor alone, and a stream cut in two at any frame, the second call with prev = the
    first's last input frame, gives the rows of one call.  period 2 or 4 (svc_hip_dct_pack_delta_temporal_auto_frames): the predecessor
    of frame i is input frame temporal_ref(i, period), `prev` the input frame at index -period; a cut then falls on a multiple of period,
    and every 2^s-th row (2^s <= period) is the row of the thinned clip at period >> s."""
    if period not in PERIODS:
        raise ValueError(f"period {period} (supported: 1, 2, 4)")
    frames = _source_frames(stream, offsets, None)
    counts = np.zeros((len(frames), 2), np.uint32)
    for i, fr in enumerate(frames):
        before = frames[temporal_ref(i, period)] if i else prev
        counts[i, 0] = _level_count(delta_frame(fr))
        counts[i, 1] = counts[i, 0] if before is None else _level_count(delta_frame(fr, before))
    return counts


def auto_keys(counts, forced=None, has_prev: bool = True) -> np.ndarray:
    """The key frames chosen by size -> (n,) bool: key[f] = forced[f] != 0 or (f == 0 and not has_prev) or counts[f, 1] >= counts[f, 0],
    counts as delta_level_counts gives them (forced None: no frame is forced).  The mask section of an SVCQ frame has a fixed size, so
    the level count decides the frame's size: a frame is differenced exactly where that makes it smaller.  A tie gives a key frame --
    the same bytes, and a point of random access."""
    counts = np.asarray(counts).reshape(-1, 2)
    key = _keys(forced, len(counts)) | (counts[:, 1] >= counts[:, 0])
    if len(key) and not has_prev:
        key[0] = True
    return key


def delta_auto_frames(stream, offsets, forced=None, prev=None, period: int = 1) -> Tuple[bytes, np.ndarray, np.ndarray, np.ndarray]:
    """What svc_hip_dct_pack_delta_auto_frames writes, given the stream svc_hip_dct_pack_levels_frames writes from the same frames ->
    (bytes, offsets (n + 1,) u64, keys (n,) bool, counts (n, 2) u32): delta_frames with the keys auto_keys chose from
    delta_level_counts.  With forced None every output frame holds min(counts[f]) levels, so frame by frame it is never larger than
    the plain stream's frame nor than the frame delta_frames writes without key flags; a forced frame is the plain stream's.  The
    choice for a frame does not depend on the choice for any other, so a stream cut into two calls at any frame, the second with
    prev = the first's last input frame and its share of `forced`, gives the bytes, keys and counts of one call.
    undelta_frames(bytes, offsets, keys, prev's reconstruction) gives the stream back.  period 2 or 4: what
    svc_hip_dct_pack_delta_temporal_auto_frames writes -- delta_temporal_frames with the keys auto_keys chose from
    delta_level_counts(.., period), `prev` the input frame at index -period; thin_frames of it at 2^s <= period, with the thinned keys
    and counts, is this function on the thinned clip at period >> s."""
    counts = delta_level_counts(stream, offsets, prev, period)
    keys = auto_keys(counts, forced, prev is not None)
    out, offs = delta_temporal_frames(stream, offsets, period, keys, prev)
    return out, offs, keys, counts


# ---- a byte budget per group of frames for the delta stream (include/svc_hip_delta_budget.h: svc_hip_dct_pack_delta_budget_frames) ---------

def delta_groups(keys, n: int):
    """The groups of a delta stream of n frames -> a list of (first, end): a group starts at frame 0 and at every frame f with
    keys[f] != 0, and runs up to the next start (keys None: one group).  Frame 0 starts a group whatever its flag."""
    key = _keys(keys, n)
    starts = [f for f in range(n) if f == 0 or key[f]]
    return [(s, e) for s, e in zip(starts, starts[1:] + [n])]


def delta_ladder_counts(streams, keys=None) -> np.ndarray:
    """-> (n, L) u32: column k is header word 10 of every frame of delta_frames(*streams[k], keys), streams[k] = (bytes, offsets) of
    the plain SVCQ stream of the same frames at ladder entry k (what svc_hip_dct_pack_levels_frames writes with that pair).  Frame 0
    has no predecessor: it is a key frame at every entry.  A frame's tiles are predicted where the frame and its predecessor code
    them at one step, which differs from entry to entry where an entry's fg_step equals its bg_step; and a difference is 0 where two
    levels agree, which a coarser step does not make likelier in every coefficient: a column is NOT monotone in k."""
    cols = []
    for stream, offsets in streams:
        out, offs = delta_frames(stream, offsets, keys)
        cols.append([_level_count(fr) for fr in _source_frames(out, offs, None)])
    return np.asarray(cols, np.uint32).T.reshape(len(cols[0]) if cols else 0, len(cols))


def delta_budget_choice(counts, geometry: Dict[str, int], keys, budgets) -> np.ndarray:
    """choice (n,) u32 of svc_hip_dct_pack_delta_budget_frames.  counts: (n, L) as delta_ladder_counts gives them; geometry: a dict with
    the keys of GEOMETRY; budgets: one u32 byte count for every frame, or one each.  bytes_k(f) = up16(levels offset + 2 counts[f, k]),
    the SVCQ frame's size.  Per group G of delta_groups the choice is the smallest k with sum_G bytes_k <= sum_G budgets (sums of 64
    bits), found by looking at EVERY entry: bytes_k is not monotone in k, so an entry may fit behind one that does not.  If none fits:
    L - 1 with bit 31 set.  Every frame of a group carries its group's value."""
    counts = np.asarray(counts, np.uint32)
    n, L = counts.shape
    tiles = (geometry["frame_w"] // geometry["block_w"]) * (geometry["frame_h"] // geometry["block_h"])
    mvb = (geometry["frame_w"] // geometry["mv_block_w"]) * (geometry["frame_h"] // geometry["mv_block_h"])
    levels_off = levels.HEADER_BYTES + 4 * mvb + 8 * 3 * tiles * ((geometry["block_w"] * geometry["block_h"] + 63) // 64)
    size = (levels_off + 2 * counts.astype(np.int64) + 15) // 16 * 16
    budget = np.broadcast_to(np.asarray(budgets, np.int64), (n,))
    choice = np.zeros(n, np.uint32)
    for first, end in delta_groups(keys, n):
        total, allowed = size[first:end].sum(axis=0), int(budget[first:end].sum())
        fits = [k for k in range(L) if int(total[k]) <= allowed]
        choice[first:end] = fits[0] if fits else (L - 1) | 0x80000000
    return choice


def delta_budget_frames(streams, keys, budgets) -> Tuple[bytes, np.ndarray, np.ndarray, np.ndarray]:
    """What svc_hip_dct_pack_delta_budget_frames writes, given the plain streams of the same frames at every ladder entry ->
    (bytes, offsets (n + 1,) u64, choice (n,) u32, counts (n, L) u32): frame f is frame f of
    delta_frames(*streams[choice[f] & 0x7FFFFFFF], keys).  A group starts at a key frame, so no frame is predicted across a change of
    steps: the result is delta_frames of the plain stream in which every frame is packed at its own chosen pair, and
    undelta_frames(bytes, offsets, keys) gives that stream back."""
    counts = delta_ladder_counts(streams, keys)
    first = _source_frames(*streams[0], None)[0]
    hdr = {k: int(v) for k, v in zip(levels.FIELDS, np.frombuffer(bytes(first[:levels.HEADER_BYTES]), "<u4"))}
    choice = delta_budget_choice(counts, {k: hdr[k] for k in GEOMETRY}, keys, budgets)
    coded = [_source_frames(*delta_frames(s, o, keys), None) for s, o in streams]
    out, offs = _join([bytes(coded[int(c) & 0x7FFFFFFF][f]) for f, c in enumerate(choice)])
    return out, offs, choice, counts


# ---- a distortion target per group of frames for the delta stream (include/svc_hip_delta_quality.h: svc_hip_dct_pack_delta_quality_frames)

def delta_quality_choice(counts, table, geometry: Dict[str, int], keys, targets, budgets=None) -> np.ndarray:
    """choice (n,) u32 of svc_hip_dct_pack_delta_quality_frames.  counts: (n, L) as delta_ladder_counts gives them; table: D (n, L) as
    distortion_table gives it (the delta is lossless in levels: a frame's D does not depend on its flags); geometry: a dict with the keys
    of GEOMETRY; targets: one u64 for every frame, or one each; budgets: None (no cap), or u32 bytes likewise.  Per group G of
    delta_groups, looking at EVERY entry (neither table is monotone along a ladder):
      Q = the entries k with D[f, k] <= targets[f] for every frame f of G (per frame, not a sum);
      F = the entries k with sum_G bytes_k <= sum_G budgets (sums of 64 bits, bytes_k as in delta_budget_choice); every entry without budgets;
      choice = max(Q & F) where that is not empty: the coarsest entry that meets the quality and fits;
               else min(F) with bit 30 set where F is not empty: the finest entry that fits, quality not met;
               else L - 1 with bit 31 set, and bit 30 set where L - 1 is not in Q.
    Every frame of a group carries its group's value."""
    counts = np.asarray(counts, np.uint32)
    n, L = counts.shape
    table = np.asarray(table, np.uint64).reshape(n, L)
    tiles = (geometry["frame_w"] // geometry["block_w"]) * (geometry["frame_h"] // geometry["block_h"])
    mvb = (geometry["frame_w"] // geometry["mv_block_w"]) * (geometry["frame_h"] // geometry["mv_block_h"])
    levels_off = levels.HEADER_BYTES + 4 * mvb + 8 * 3 * tiles * ((geometry["block_w"] * geometry["block_h"] + 63) // 64)
    size = (levels_off + 2 * counts.astype(np.int64) + 15) // 16 * 16
    target = np.broadcast_to(np.asarray(targets, np.uint64), (n,))
    budget = None if budgets is None else np.broadcast_to(np.asarray(budgets, np.int64), (n,))
    choice = np.zeros(n, np.uint32)
    for first, end in delta_groups(keys, n):
        met = [k for k in range(L) if all(int(table[f, k]) <= int(target[f]) for f in range(first, end))]
        fits = list(range(L))
        if budget is not None:
            total, allowed = size[first:end].sum(axis=0), int(budget[first:end].sum())
            fits = [k for k in range(L) if int(total[k]) <= allowed]
        both = [k for k in met if k in fits]
        if both:
            value = both[-1]
        elif fits:
            value = fits[0] | 0x40000000
        else:
            value = (L - 1) | 0x80000000 | (0 if L - 1 in met else 0x40000000)
        choice[first:end] = value
    return choice


def delta_quality_frames(streams, table, keys, targets, budgets=None) -> Tuple[bytes, np.ndarray, np.ndarray, np.ndarray]:
    """What svc_hip_dct_pack_delta_quality_frames writes, given the plain streams of the same frames at every ladder entry and their
    distortion table -> (bytes, offsets (n + 1,) u64, choice (n,) u32, counts (n, L) u32): frame f is frame f of
    delta_frames(*streams[choice[f] & 0x3FFFFFFF], keys).  As in delta_budget_frames a group starts at a key frame, so
    undelta_frames(bytes, offsets, keys) gives back the plain stream in which every frame is packed at its own chosen pair."""
    counts = delta_ladder_counts(streams, keys)
    first = _source_frames(*streams[0], None)[0]
    hdr = {k: int(v) for k, v in zip(levels.FIELDS, np.frombuffer(bytes(first[:levels.HEADER_BYTES]), "<u4"))}
    choice = delta_quality_choice(counts, table, {k: hdr[k] for k in GEOMETRY}, keys, targets, budgets)
    coded = [_source_frames(*delta_frames(s, o, keys), None) for s, o in streams]
    out, offs = _join([bytes(coded[int(c) & 0x3FFFFFFF][f]) for f, c in enumerate(choice)])
    return out, offs, choice, counts


# ---- a stored fine stream split into a base at any steps and its enhancement (include/svc_hip.h: svc_hip_split_levels_frames) ---------

MAX_RATIO = 32766  # of a base step to the fine step: |d| <= ratio / 2 stays an int16


def _check_split_steps(fine_step: int, fg_step: int, bg_step: int) -> None:
    if min(fine_step, fg_step, bg_step) <= 0:
        raise ValueError("quant steps must be positive")
    if fg_step % fine_step or bg_step % fine_step:
        raise ValueError(f"the base steps ({fg_step}, {bg_step}) must be multiples of fine_step {fine_step}")
    if max(fg_step, bg_step) // fine_step > MAX_RATIO:
        raise ValueError(f"residuals of base step {max(fg_step, bg_step)} over fine_step {fine_step} could exceed int16")


def _fine_levels(fine_frame, fine_step: int):
    hdr, types, planes = levels.parse_frame(fine_frame)  # raises for a frame the reader rejects (the device's status 2 .. 7)
    if hdr["fg_step"] != fine_step or hdr["bg_step"] != fine_step:
        raise ValueError(f"the frame's steps ({hdr['fg_step']}, {hdr['bg_step']}) are not ({fine_step}, {fine_step})")  # status 11
    lf, _ = _levels_of(hdr, types, planes)
    return hdr, types, lf


def _base_levels(lf: np.ndarray, ratio: np.ndarray) -> np.ndarray:
    """lf / ratio rounded half away from zero, in integers (ratio per pixel, broadcast over the planes)."""
    return np.sign(lf) * ((2 * np.abs(lf) + ratio) // (2 * ratio))


def split_frame(fine_frame, fine_step: int, fg_step: int, bg_step: int, window=None) -> Tuple[bytes, bytes]:
    """The frame stored at (fine_step, fine_step) -> (base frame at (fg_step, bg_step), enhancement frame): header words 0 .. 7 and 11
    and the types of the input, the base's levels Lb and the enhancement's d (zero outside the window x, y, w, h; None: every tile).
    Stated on the levels' values: a set mask bit whose level is 0 is a zero.  Raises ValueError where the device reports a status."""
    _check_split_steps(fine_step, fg_step, bg_step)
    hdr, types, lf = _fine_levels(fine_frame, fine_step)
    background, ox, oy = _tile_maps(hdr, types)
    ratio = _per_pixel(hdr, np.where(background, bg_step, fg_step).astype(np.int64) // fine_step)[None]
    lb = _base_levels(lf, ratio)
    d = lf - lb * ratio
    if window is not None:
        d = np.where(_per_pixel(hdr, _contains(window, ox, oy))[None], d, 0)
    return (write_frame(hdr, types, lb, fg_step, bg_step, hdr["inexact"]),
            write_frame(hdr, types, d, fine_step, fine_step, hdr["inexact"]))


def _source_frames(stream, offsets, src):
    """The input frame of every output frame, checked as window_frames checks it -> a list of u8 views."""
    b = np.frombuffer(stream, np.uint8) if not isinstance(stream, np.ndarray) else stream.reshape(-1).view(np.uint8)
    offs = [int(o) for o in np.asarray(offsets).reshape(-1)]
    n_in = len(offs) - 1
    idx = list(range(n_in)) if src is None else [int(i) for i in np.asarray(src).reshape(-1)]
    out = []
    for i, f in enumerate(idx):
        if not 0 <= f < n_in:
            raise ValueError(f"output frame {i} names input frame {f} of {n_in}")
        lo, hi = offs[f], offs[f + 1]
        if lo % 16 or hi < lo or hi > b.size:
            raise ValueError(f"SVCQ frame offsets out of order, misaligned or past the stream: {lo}, {hi}")
        if hi - lo >= levels.HEADER_BYTES and int(b[lo + 48:lo + 52].view("<u4")[0]) != hi - lo:
            raise ValueError(f"SVCQ frame at {lo} has frame_bytes {int(b[lo + 48:lo + 52].view('<u4')[0])}, its offsets {hi - lo}")
        out.append(b[lo:hi])
    return out


def _join(frames) -> Tuple[bytes, np.ndarray]:
    return b"".join(frames), np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.uint64)


def split_frames(stream, offsets, fine_step: int, fg_step: int, bg_step: int, windows=None, src=None
                 ) -> Tuple[bytes, np.ndarray, bytes, np.ndarray]:
    """What svc_hip_split_levels_frames writes for frames that pass their checks -> (base bytes, base offsets (n_out + 1,) u64,
    enhancement bytes, its offsets): output frame i is split_frame of input frame src[i] (src None: frame i) and windows[i]."""
    _check_split_steps(fine_step, fg_step, bg_step)
    frames = _source_frames(stream, offsets, src)
    win = None if windows is None else np.asarray(windows).reshape(len(frames), 4)
    pairs = [split_frame(fr, fine_step, fg_step, bg_step, None if win is None else win[i]) for i, fr in enumerate(frames)]
    return _join([p[0] for p in pairs]) + _join([p[1] for p in pairs])


def split_budget_frames(stream, offsets, fine_step: int, ladder, budgets, windows=None, src=None
                        ) -> Tuple[bytes, np.ndarray, bytes, np.ndarray, np.ndarray]:
    """What svc_hip_split_levels_budget_frames writes -> (base bytes, base offsets, enhancement bytes, its offsets, choice (n_out,)
    u32).  ladder: (fg_step, bg_step) pairs, finest first, non-decreasing, multiples of fine_step; budgets: one u32 byte count for
    every output frame, or one each.  For entry k, bytes_k = up16(levels offset + 2 nz_k) with nz_k the coefficients whose
    2 |Lf| >= r_k of their class (exactly Lb != 0): the base frame's size.  choice = the smallest k with bytes_k <= budget, else the
    last entry with bit 31 set; the frame is split_frame at that pair."""
    lad = [(int(fg), int(bg)) for fg, bg in ladder]
    if not 1 <= len(lad) <= 64:
        raise ValueError(f"a ladder of {len(lad)} entries (1 .. 64)")
    for k, (fg, bg) in enumerate(lad):
        if fine_step <= 0 or fg <= 0 or bg <= 0:
            raise ValueError("quant steps must be positive")
        if k and (fg < lad[k - 1][0] or bg < lad[k - 1][1]):
            raise ValueError(f"ladder entry {k} is below entry {k - 1}: the ladder must be non-decreasing")
        if fg % fine_step or bg % fine_step:
            raise ValueError(f"ladder entry {k} ({fg}, {bg}) must be multiples of fine_step {fine_step}")
    _check_split_steps(fine_step, *lad[-1])
    frames = _source_frames(stream, offsets, src)
    n = len(frames)
    win = None if windows is None else np.asarray(windows).reshape(n, 4)
    budget = np.broadcast_to(np.asarray(budgets, np.int64), (n,))
    base, enh, choice = [], [], np.zeros(n, np.uint32)
    for i, fr in enumerate(frames):
        hdr, types, lf = _fine_levels(fr, fine_step)
        background = _per_pixel(hdr, _tile_maps(hdr, types)[0])[None]
        tiles = (hdr["frame_w"] // hdr["block_w"]) * (hdr["frame_h"] // hdr["block_h"])
        levels_off = levels.HEADER_BYTES + 4 * types.size + 8 * 3 * tiles * ((hdr["block_w"] * hdr["block_h"] + 63) // 64)
        pick = None
        for k, (fg, bg) in enumerate(lad):
            nz = int((2 * np.abs(lf) >= np.where(background, bg, fg) // fine_step).sum())
            if (levels_off + 2 * nz + 15) // 16 * 16 <= int(budget[i]):
                pick = k
                break
        choice[i] = pick if pick is not None else (len(lad) - 1) | 0x80000000
        b, e = split_frame(fr, fine_step, *lad[int(choice[i]) & 0x7FFFFFFF], None if win is None else win[i])
        base.append(b)
        enh.append(e)
    return _join(base) + _join(enh) + (choice,)


# ---- both layers from raw coefficient planes (include/svc_hip.h: svc_hip_pack_layers_frames) ----------------------------------------

def quantise(planes: np.ndarray, step) -> np.ndarray:
    """The pack's quantiser on f32 coefficients -> i64 levels: the quotient c / step taken in f32, rounded half away from zero (exactly:
    the f32 quotient plus or minus a half is exact in f64), then clamped to int16.  step: an integer, or an array that broadcasts."""
    q = (np.asarray(planes, np.float32) / np.asarray(step).astype(np.float32)).astype(np.float64)
    return np.clip(np.trunc(q + np.copysign(0.5, q)), -32768, 32767).astype(np.int64)


# ---- a quality target for the fused pack (include/svc_hip_quality.h: svc_hip_dct_pack_levels_quality_frames) -------------------------

def quantisation_error(planes: np.ndarray, step) -> np.ndarray:
    """x = c - quantise(c, step) * step per coefficient, in f64: c is an f32 and the product an integer below 2^24, so the difference is
    exact there.  (It is representable in f32 as well -- q == 0 gives c itself, otherwise x is a multiple of ulp(c) no larger than about
    step / 2 <= |c| -- which is why the kernel's one f32 fma gives the same number; tests/test_quality_host.py checks it.)"""
    c = np.asarray(planes, np.float32).astype(np.float64)
    return c - (quantise(planes, step) * np.asarray(step).astype(np.int64)).astype(np.float64)


def distortion_table(planes, types, geometry: Dict[str, int], ladder) -> np.ndarray:
    """D (n, K) u64 of svc_hip_dct_pack_levels_quality_frames.  planes: raw coefficients (n, 3, H, W) f32, what svc_hip_dct_frames writes;
    types: region ids (n, MV rows, MV columns) or (n, MV blocks); geometry: a dict with the keys of GEOMETRY; ladder: K pairs
    (fg_step, bg_step).  Per coefficient c and entry k, with s the step of c's tile (bg_step where the MV block holding the tile has type
    0): e = rint(256 * (c - quantise(c, s) * s)), half to even, an integer; D[f][k] = the sum of e * e over the frame's three planes.
    D / 65536 is the squared error of the dequantised coefficients and, the transform being orthonormal, of the unclipped picture."""
    w, h = geometry["frame_w"], geometry["frame_h"]
    planes = np.asarray(planes, np.float32).reshape(-1, 3, h, w)
    n = planes.shape[0]
    types = np.asarray(types).astype(np.uint32).reshape(n, h // geometry["mv_block_h"], w // geometry["mv_block_w"])
    lad = [(int(fg), int(bg)) for fg, bg in ladder]
    table = np.zeros((n, len(lad)), np.uint64)
    for f in range(n):
        background = _per_pixel(geometry, _tile_maps(geometry, types[f])[0])[None]
        for k, (fg, bg) in enumerate(lad):
            e = np.rint(256.0 * quantisation_error(planes[f], np.where(background, bg, fg))).astype(np.int64)
            table[f, k] = int((e * e).sum(dtype=np.int64))  # < 2^32 per coefficient on average: below 2^63 for any frame the call takes
    return table


def quality_choice(table, sizes, targets, budgets=None) -> np.ndarray:
    """choice (n,) u32 of svc_hip_dct_pack_levels_quality_frames.  table: D (n, K); sizes: bytes_k (n, K), the SVCQ frame's size at every
    entry; targets: one u64 for every frame, or one each; budgets: None (no cap), or u32 bytes likewise.
      kq = the largest k with D[k] <= target, 0 where no entry meets it (D is not monotone along a ladder);
      kb = the budgeted calls' choice -- the smallest k with bytes_k <= budget, else K - 1 with bit 31 set; 0 without budgets;
      choice = max(kq, kb & 0x7FFFFFFF), bit 31 as kb has it, bit 30 set exactly when D[choice] > target."""
    table = np.asarray(table, np.uint64)
    n, K = table.shape
    sizes = np.asarray(sizes).reshape(n, K)
    target = np.broadcast_to(np.asarray(targets, np.uint64), (n,))
    budget = None if budgets is None else np.broadcast_to(np.asarray(budgets, np.int64), (n,))
    choice = np.zeros(n, np.uint32)
    for f in range(n):
        met = [k for k in range(K) if int(table[f, k]) <= int(target[f])]
        kq = met[-1] if met else 0
        kb, over = 0, 0
        if budget is not None:
            fits = [k for k in range(K) if int(sizes[f, k]) <= int(budget[f])]
            kb, over = (fits[0], 0) if fits else (K - 1, 0x80000000)
        pick = max(kq, kb)
        choice[f] = pick | over | (0x40000000 if int(table[f, pick]) > int(target[f]) else 0)
    return choice


def _psnr_scale(w: int, h: int) -> int:
    return 255 * 255 * 3 * int(w) * int(h) * 65536


def distortion_target(psnr_db, w: int, h: int) -> int:
    """The largest D that still reaches psnr_db on a w x h frame: floor(255^2 * 3 w h * 65536 / 10^(psnr_db / 10)), in decimal
    arithmetic of 60 digits (an f64 quotient is off by thousands of units at these magnitudes), capped at 2^64 - 1."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        d = decimal.Decimal(_psnr_scale(w, h)) / (decimal.Decimal(10) ** (decimal.Decimal(psnr_db) / 10))
        return min(int(d.to_integral_value(rounding=decimal.ROUND_FLOOR)), 2 ** 64 - 1)


def distortion_psnr(d, w: int, h: int) -> float:
    """The PSNR in dB a distortion D stands for on a w x h frame, 10 log10(255^2 * 3 w h * 65536 / D); inf for D = 0."""
    import math
    d = int(d)
    return math.inf if d == 0 else 10.0 * math.log10(_psnr_scale(w, h) / d)


def pack_layers_frames(planes, types, geometry: Dict[str, int], fg_step: int, bg_step: int, enh_step: int, windows=None
                       ) -> Tuple[bytes, np.ndarray, bytes, np.ndarray, np.ndarray]:
    """What svc_hip_pack_layers_frames writes -> (base bytes, base offsets (n + 1,) u64, enhancement bytes, its offsets, inexact (n,)
    u32).  planes: raw coefficients (n, 3, H, W) f32; types: region ids (n, MV rows, MV columns) or (n, MV blocks); geometry: a dict
    with the keys of GEOMETRY; windows: None (every tile is enhanced) or per frame x, y, w, h in padded coordinates (n, 4).  Per frame
    Lb = quantise(c, the tile's base step), Lf = quantise(c, enh_step) and d = Lf - Lb * ratio inside the window, 0 outside it; the
    base's header word 11 counts the coefficients with c != (f32)Lb * (f32)step."""
    _check_split_steps(enh_step, fg_step, bg_step)
    w, h = geometry["frame_w"], geometry["frame_h"]
    planes = np.asarray(planes, np.float32).reshape(-1, 3, h, w)
    n = planes.shape[0]
    types = np.asarray(types).astype(np.uint32).reshape(n, h // geometry["mv_block_h"], w // geometry["mv_block_w"])
    win = None if windows is None else np.asarray(windows).reshape(n, 4)
    base, enh, inexact = [], [], np.zeros(n, np.uint32)
    for f in range(n):
        background, ox, oy = _tile_maps(geometry, types[f])
        step = _per_pixel(geometry, np.where(background, bg_step, fg_step).astype(np.int64))[None]
        lb = quantise(planes[f], step)
        d = quantise(planes[f], enh_step) - lb * (step // enh_step)
        if win is not None:
            d = np.where(_per_pixel(geometry, _contains(win[f], ox, oy))[None], d, 0)
        inexact[f] = int((planes[f] != lb.astype(np.float32) * step.astype(np.float32)).sum())
        base.append(write_frame(geometry, types[f], lb, fg_step, bg_step, int(inexact[f])))
        enh.append(write_frame(geometry, types[f], d, enh_step, enh_step))
    return _join(base) + _join(enh) + (inexact,)
