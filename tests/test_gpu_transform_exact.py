"""Every coefficient producer against the long-double reference of tests/helpers/transform_ref.py, at half an ulp.

csrc/dct.hip and csrc/idct_core.hpp accumulate in float64 and round once to f32; the 1e-4 * max(1, |ref|) bar of the other transform
tests is ~1600 f32 ulps at a DC of 2040 and accepts an f32 table or an f32 pass (tests/test_transform_ref.py shows it).  Here:

  raw         RN32(ref - A) <= got <= RN32(ref + A), A the derived bound of the f64 chains (transform_ref.forward_slack)
  quantised   got == oracle.quant(RN32(ref - A)) or oracle.quant(RN32(ref + A))
  inverse     the same interval around idct_ref(oracle.quant(coefficients)) with A' per tile (transform_ref.inverse_slack)

Where the two ends agree that is equality with the correctly rounded value; the share of positions where they do not is capped from
the reference alone, before the comparison.  Each form is reached directly: planes (svc_hip_dct_frames, svc_hip_dct_host, tuned and
general kernel, svc_hip_dct_tiles_host), fused quantiser (svc_hip_dct_quant_frames tuned and general, svc_hip_dct_quant_luma_frames
then svc_hip_dct_quant_redo_frames), records (svc_hip_dct_records_frames tuned and general, svc_hip_dct_records_luma_frames) and the
inverse (svc_hip_decode_frames).  The fused kernels' quantiser itself (csrc/quant_core.hpp) meets every float next to every rounding
tie in test_quant_fast_at_every_tie.  Inputs and the edges they hit: tests/helpers/transform_inputs.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.helpers import transform_inputs as ti
from tests.helpers import transform_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tr.available(), reason=tr.UNAVAILABLE)]

F32 = np.float32


def _say(msg):
    print(f"[transform-exact] {msg}", flush=True)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(types):
    return _cuda(np.ascontiguousarray(types).view(np.int32))


class _Refs:
    """[lo, hi] per (input, block), computed once per module."""

    def __init__(self):
        self._inputs, self._bounds = {}, {}

    def input(self, key):
        if key not in self._inputs:
            kind, arg = key
            if kind == "placement":
                self._inputs[key] = ti.tuned_placement_frames(arg)
            elif kind == "general":
                self._inputs[key] = ti.general_frames(*arg)
            else:
                frames, types, spec = ti.coverage_case(arg)
                self._inputs[key] = (frames, types, spec)
        return self._inputs[key]

    def bounds(self, key, bw, bh):
        k = (key, bw, bh)
        if k not in self._bounds:
            frames = self.input(key)[0]
            a = tr.forward_slack(bw, bh)
            lo, hi = zip(*(tr.interval(tr.dct_ref(f, bw, bh), a) for f in frames))
            self._bounds[k] = (np.stack(lo), np.stack(hi))  # (n, 3, H, W) f32
        return self._bounds[k]


@pytest.fixture(scope="module")
def refs():
    r = _Refs()
    yield r
    r._inputs.clear()
    r._bounds.clear()


def _where(bad, *arrays):
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} positions, first at {i}: " + ", ".join(repr(float(a[i])) for a in arrays)


def _assert_raw(got, lo, hi, what):
    bad = tr.raw_violations(got, lo, hi)
    assert not bad.any(), f"{what}: outside [RN32(ref - A), RN32(ref + A)] at {_where(bad, got, lo, hi)} (got, lo, hi)"


def _assert_quant(got, qlo, qhi, what):
    bad = tr.quant_violations(got, qlo, qhi)
    assert not bad.any(), f"{what}: neither quant(lo) nor quant(hi) at {_where(bad, got, qlo, qhi)} (got, quant(lo), quant(hi))"


def _cap_raw(lo, hi, count, what):
    """The raw cap, from the reference alone, over the positions of random content."""
    share = float((lo != hi)[count].mean())
    _say(f"{what}: raw ambiguous share {share:.3e} of {int(count.sum())} random-content coefficients")
    assert share <= tr.RAW_AMBIGUOUS_CAP


def _quant_bounds(oracle, lo, hi, types, mv, fg, bg):
    n = lo.shape[0]
    qlo = np.stack([oracle.quant_frame(lo[f], mv[0], mv[1], types[f], fg, bg) for f in range(n)])
    qhi = np.stack([oracle.quant_frame(hi[f], mv[0], mv[1], types[f], fg, bg) for f in range(n)])
    return qlo, qhi


def _random_types(seed, n, w, h, mv):
    rng = np.random.default_rng(seed)
    blocks = (w // mv) * (h // mv)
    return (rng.integers(1, 40, (n, blocks)) * (rng.random((n, blocks)) < 0.5)).astype(np.uint32)


# ---- planes: the tuned kernels ----------------------------------------------------------------------------------------------------------
# input ("placement", N): 3 frames, 176 x 48 (N = 8) or 224 x 160 (N = 16) -- a workgroup's 256 / N segment columns straddle bands and
# frames, the last workgroup is partial, 7 / 27 workgroups are not a multiple of 8 -- holding every impulse position, the saturated, zero and
# checkerboard tiles scattered over all frames, random bytes, and a smooth last frame (transform_inputs.structured_frames)

@pytest.mark.parametrize("block", [8, 16])
def test_dct_frames_tuned(native, refs, block):
    frames, special = refs.input(("placement", block))
    lo, hi = refs.bounds(("placement", block), block, block)
    n, h, w, _ = frames.shape
    seg, wgs, per = ti.tuned_work_split(block, n, h, w)
    _say(f"tuned {block} placement input: {n} frames {w}x{h}, {w // 16} segment columns per band, {seg // n} per frame, {seg} = "
         f"{seg / per:.2f} workgroups of {per} ({wgs} = {wgs % 8} mod 8), {int(special[:, ::block, ::block].sum())} special tiles")
    assert (w // 16) % per != 0 and (seg // n) % per != 0 and seg % per != 0 and wgs % 8 != 0
    _cap_raw(lo[:-1], hi[:-1], ~np.stack([special[:-1]] * 3, axis=1), f"dct_frames tuned {block}")
    got = native.dct_frames(_cuda(frames), block).cpu().numpy()
    _assert_raw(got, lo, hi, f"dct_frames tuned {block}")


@pytest.mark.parametrize("block", [8, 16])
def test_dct_host_tuned(native, refs, block):
    frames, _ = refs.input(("placement", block))
    lo, hi = refs.bounds(("placement", block), block, block)
    for f in range(len(frames)):
        _assert_raw(native.dct_host(frames[f], block), lo[f], hi[f], f"dct_host tuned {block}, frame {f}")


# ---- planes: the general kernel ---------------------------------------------------------------------------------------------------------
# input ("general", (bw, bh)): 2 frames whose width is more than one strip and not a whole number of strips (the last strip of a band is
# narrower than sw), the same special tiles (above 16 x 16: 256 sampled impulse positions with the four corners), random, smooth

@pytest.mark.parametrize("bw,bh", ti.GENERAL_BLOCKS)
def test_dct_general(native, refs, bw, bh):
    key = ("general", (bw, bh))
    frames, special = refs.input(key)
    n, h, w, _ = frames.shape
    sw = ti.general_strip(bw, bh, w)
    _say(f"general {bw}x{bh} input: {n} frames {w}x{h}, strips of {sw} columns, the last of a band {w % sw or sw}, "
         f"{int(special[:, ::bh, ::bw].sum())} special tiles")
    assert (bw, bh) == (64, 64) or w % sw != 0
    assert not (bw == bh and bw in (8, 16) and w % 16 == 0)  # or the tuned kernel would take it
    lo, hi = refs.bounds(key, bw, bh)
    _cap_raw(lo[:1], hi[:1], ~np.stack([special[:1]] * 3, axis=1), f"dct_frames general {bw}x{bh}")
    got = native.dct_frames(_cuda(frames), (bw, bh)).cpu().numpy()
    _assert_raw(got, lo, hi, f"dct_frames general {bw}x{bh}")
    _assert_raw(native.dct_host(frames[1], (bw, bh)), lo[1], hi[1], f"dct_host general {bw}x{bh}")


@pytest.mark.parametrize("bw,bh", [(8, 8), (16, 16), (6, 10), (32, 32)])
def test_dct_tiles_host(native, bw, bh):
    """cv::dct over the tiles of one byte-valued f32 plane, in place: the regular grid, and a list of corners off the grid (every
    other tile of a grid shifted by (3, 5); the rest of the image must come back untouched).  16 x 16 from the definition is
    reachable here only: svc_hip_dct_frames sends it to the tuned kernel at every width it admits."""
    frames, _ = ti.structured_frames(bw, bh, 1, 19 if bw * bh <= 256 else 17, 15 if bw * bh <= 256 else 16, 5000 + bw)
    plane = frames[0, :, :, 1].astype(F32)
    lo, hi = tr.interval(tr.dct_planes_ref(plane[None], bw, bh), tr.forward_slack(bw, bh))
    _assert_raw(native.dct_tiles_host(plane, bw, bh), lo[0], hi[0], f"dct_tiles_host {bw}x{bh} grid")
    h, w = plane.shape
    img = np.zeros((h + 5, w + 3), F32)
    img[5:, 3:] = plane
    corners = [(3 + tx * bw, 5 + ty * bh) for ty in range(h // bh) for tx in range(w // bw) if (tx + ty) % 2 == 0]
    got = native.dct_tiles_host(img, bw, bh, corners)
    listed = np.zeros(plane.shape, bool)
    for x, y in corners:
        listed[y - 5:y - 5 + bh, x - 3:x - 3 + bw] = True
    inner = got[5:, 3:]
    _assert_raw(inner[listed], lo[0][listed], hi[0][listed], f"dct_tiles_host {bw}x{bh} corner list")
    assert np.array_equal(inner[~listed], plane[~listed]) and not got[:5].any() and not got[:, :3].any()


# ---- fused quantiser --------------------------------------------------------------------------------------------------------------------

def _coverage(oracle, refs, form):
    """The coverage input of a fused form, its [lo, hi], and per call of transform_inputs.COVERAGE_STEPS the quantised bounds; the caps
    and the tie counts are asserted here, from the reference alone."""
    key = ("coverage", form)
    frames, types, c = refs.input(key)
    lo, hi = refs.bounds(key, *c["block"])
    _cap_raw(lo, hi, np.ones(lo.shape, bool), f"{form} coverage input")
    census, calls = {}, []
    for fg, bg in ti.COVERAGE_STEPS:
        qlo, qhi = _quant_bounds(oracle, lo, hi, types, c["mv"], fg, bg)
        steps = np.stack([ti.step_plane(types[f], c["w"], c["h"], c["mv"], fg, bg) for f in range(c["n"])])[:, None].repeat(3, 1)
        for s in {fg, bg}:
            ti.add_census(census, ti.tie_census(lo, hi, qlo, qhi, steps, s))
        calls.append((fg, bg, qlo, qhi))
    for s, t in sorted(census.items()):
        _say(f"{form} {c['block'][0]}x{c['block'][1]} step {s}: {t}")
        assert t["ambiguous"] <= tr.QUANT_AMBIGUOUS_CAP * t["positions"]
        if s in (1, 3, 7):
            assert min(t["ties_pos"], t["ties_neg"], t["near_ties"]) >= 32, (form, s, t)
    return frames, types, c, calls


# input ("coverage", form): two 1904 x 1088 frames of random bytes (119 segment columns per band, 1011.5 workgroups) for the tuned
# kernels, two 1900 x 1080 frames at 4 x 4 (strips of 1024 and 876 columns) for the general one, region ids half background
@pytest.mark.parametrize("form", ["tuned8", "tuned16", "general"])
def test_dct_quant_frames(native, oracle, refs, form):
    frames, types, c, calls = _coverage(oracle, refs, form)
    if form != "general":
        seg, wgs, per = ti.tuned_work_split(c["block"][0], c["n"], c["h"], c["w"])
        _say(f"{form} coverage input: {c['n']} frames {c['w']}x{c['h']}, {seg} segment columns = {seg / per:.2f} workgroups of {per} ({wgs} = {wgs % 8} mod 8)")
        assert (c["w"] // 16) % per != 0 and seg % per != 0 and wgs % 8 != 0
    else:
        sw = ti.general_strip(*c["block"], c["w"])
        _say(f"{form} coverage input: {c['n']} frames {c['w']}x{c['h']}, strips of {sw} and {c['w'] % sw} columns")
        assert c["w"] % sw != 0
    bgr, t = _cuda(frames), _i32(types)
    for fg, bg, qlo, qhi in calls:
        got = native.dct_quant_frames(bgr, c["block"], t, c["mv"][0], fg, bg).cpu().numpy()
        _assert_quant(got, qlo, qhi, f"dct_quant_frames {form}, steps ({fg}, {bg})")


@pytest.mark.parametrize("block", [8, 16])
def test_dct_quant_frames_tuned_placement(native, oracle, refs, block):
    """The fused kernels where a workgroup straddles frames, on the special tiles (an exact zero may come out as either zero)."""
    frames, _ = refs.input(("placement", block))
    lo, hi = refs.bounds(("placement", block), block, block)
    n, h, w, _ = frames.shape
    types = _random_types(block, n, w, h, 16)
    for fg, bg in ((1, 640), (3, 17)):
        got = native.dct_quant_frames(_cuda(frames), block, _i32(types), 16, fg, bg).cpu().numpy()
        _assert_quant(got, *_quant_bounds(oracle, lo, hi, types, (16, 16), fg, bg), f"dct_quant_frames tuned {block} placement ({fg}, {bg})")
        for f in (0, n - 1):
            one = native.dct_quant_host(frames[f], block, types[f], 16, fg, bg)
            _assert_quant(one[None], *_quant_bounds(oracle, lo[f:f + 1], hi[f:f + 1], types[f:f + 1], (16, 16), fg, bg),
                          f"dct_quant_host tuned {block}, frame {f}")


@pytest.mark.parametrize("bw,bh,mv", [(6, 10, 30), (32, 32, 32), (8, 8, 8), (2, 2, 2)])
def test_dct_quant_frames_general_placement(native, oracle, refs, bw, bh, mv):
    key = ("general", (bw, bh))
    frames, _ = refs.input(key)
    lo, hi = refs.bounds(key, bw, bh)
    n, h, w, _ = frames.shape
    types = _random_types(bw + bh, n, w, h, mv)
    for fg, bg in ((1, 640), (3, 7)):
        got = native.dct_quant_frames(_cuda(frames), (bw, bh), _i32(types), mv, fg, bg).cpu().numpy()
        _assert_quant(got, *_quant_bounds(oracle, lo, hi, types, (mv, mv), fg, bg), f"dct_quant_frames general {bw}x{bh} ({fg}, {bg})")


@pytest.mark.parametrize("block", [8, 16])
def test_dct_quant_luma_then_redo(native, oracle, refs, block):
    """SPEC 1 (svc_hip_dct_quant_luma_frames: every tile with the background step) and SPEC 2 (svc_hip_dct_quant_redo_frames: the
    tiles of foreground MV blocks again, with the foreground step), each against the reference; on the coverage input, whose
    foreground list is not a whole number of workgroup trips, and on the placement input."""
    for key, mv in ((("coverage", f"tuned{block}"), 16), (("placement", block), 16)):
        got_in = refs.input(key)
        frames = got_in[0]
        n, h, w, _ = frames.shape
        types = got_in[1] if key[0] == "coverage" else _random_types(77 + block, n, w, h, mv)
        lo, hi = refs.bounds(key, block, block)
        listed = int((types != 0).sum()) * (mv // 16) * (mv // block)  # segment columns of the redo list
        _say(f"redo {block} {key[0]} input: {int((types != 0).sum())} foreground MV blocks = {listed} segment columns = "
             f"{listed / (256 // block):.2f} workgroup trips of {256 // block}")
        assert listed % (256 // block) != 0, "the redo list must end in a partial workgroup trip"
        bgr, t = _cuda(frames), _i32(types)
        for fg, bg in ((1, 3), (3, 7)) if key[0] == "coverage" else ((7, 640), (1, 17)):
            planes, _, _ = native.dct_quant_luma_frames(bgr, block, 1, bg_step=bg)
            spec1 = planes.cpu().numpy()
            _assert_quant(spec1, *_quant_bounds(oracle, lo, hi, np.zeros_like(types), (mv, mv), fg, bg),
                          f"dct_quant_luma_frames {block} {key[0]}, step {bg}")
            native.dct_quant_redo_frames(bgr, planes, block, t, mv, fg_step=fg)
            _assert_quant(planes.cpu().numpy(), *_quant_bounds(oracle, lo, hi, types, (mv, mv), fg, bg),
                          f"dct_quant_redo_frames {block} {key[0]}, steps ({fg}, {bg})")


# ---- records ----------------------------------------------------------------------------------------------------------------------------

def _parse_records(rec, w, emit_h, n_side):
    """(frames, bytes) u8 -> (type words (frames, tiles_y, tiles_x) u32, planes (frames, 3, tiles_y * N, W) f32) of libs/encoder.cpp:222-269:
    per tile, row-major, a u32 type then per channel N rows of N floats."""
    tx, ty = w // n_side, -(-emit_h // n_side)
    dw = 1 + 3 * n_side * n_side
    rec = np.ascontiguousarray(rec)
    assert rec.shape[1] == 4 * dw * tx * ty
    words = rec.view(np.uint32).reshape(rec.shape[0], ty, tx, dw)
    coeffs = words[..., 1:].view(F32).reshape(rec.shape[0], ty, tx, 3, n_side, n_side)
    planes = coeffs.transpose(0, 3, 1, 4, 2, 5).reshape(rec.shape[0], 3, ty * n_side, tx * n_side)
    return words[..., 0], planes


def _tile_types(types, w, h, mv, n_side, rows):
    t = np.asarray(types).reshape(-1, h // mv, w // mv)
    return np.repeat(np.repeat(t, mv // n_side, axis=1), mv // n_side, axis=2)[:, :rows]


def _records_case(native, oracle, refs, key, block, mv, what):
    frames, _ = refs.input(key)
    lo, hi = refs.bounds(key, block, block)
    n, h, w, _ = frames.shape
    types = _random_types(block + 5, n, w, h, mv)
    bgr, t = _cuda(frames), _i32(types)
    # raw coefficients, the last tile row not emitted (SerializeEncodedFrame over the unpadded height)
    emit_h = h - block
    tw, planes = _parse_records(native.dct_records_frames(bgr, block, t, mv, 0, 0, emit_h=emit_h).cpu().numpy(), w, emit_h, block)
    assert np.array_equal(tw, _tile_types(types, w, h, mv, block, emit_h // block))
    _assert_raw(planes, lo[:, :, :emit_h], hi[:, :, :emit_h], f"dct_records_frames {what} raw")
    # quantised, every row
    tw, planes = _parse_records(native.dct_records_frames(bgr, block, t, mv, 3, 17).cpu().numpy(), w, h, block)
    assert np.array_equal(tw, _tile_types(types, w, h, mv, block, h // block))
    _assert_quant(planes, *_quant_bounds(oracle, lo, hi, types, (mv, mv), 3, 17), f"dct_records_frames {what} quantised (3, 17)")


@pytest.mark.parametrize("block", [8, 16])
def test_dct_records_frames_tuned(native, oracle, refs, block):
    _records_case(native, oracle, refs, ("placement", block), block, 16, f"tuned {block}")


@pytest.mark.parametrize("block,mv", [(4, 16), (32, 32)])
def test_dct_records_frames_general_square(native, oracle, refs, block, mv):
    _records_case(native, oracle, refs, ("general", (block, block)), block, mv, f"general {block}x{block}")


@pytest.mark.parametrize("block", [8, 16])
def test_dct_records_luma_frames(native, refs, block):
    frames, _ = refs.input(("placement", block))
    lo, hi = refs.bounds(("placement", block), block, block)
    n, h, w, _ = frames.shape
    rec, _, _ = native.dct_records_luma_frames(_cuda(frames), block, 1)
    tw, planes = _parse_records(rec.cpu().numpy(), w, h, block)
    assert not tw.any()  # the region ids do not exist yet: every type word is background
    _assert_raw(planes, lo, hi, f"dct_records_luma_frames {block}")


# ---- inverse ----------------------------------------------------------------------------------------------------------------------------

def _decode_steps(types, w, h, block, mv, fg, bg, gaze):
    """(H, W) u32 step of every coefficient of a frame: gazed tile (origin inside the rectangle) 1, background bg, else fg
    (libs/decoder.cpp:130-135, :202)."""
    s = ti.step_plane(types, w, h, (mv, mv), fg, bg)
    gx, gy, gw, gh = gaze
    if gw and gh:
        ty, tx = np.mgrid[0:h, 0:w]
        ty, tx = ty // block * block, tx // block * block
        s = np.where((tx >= gx) & (tx < gx + gw) & (ty >= gy) & (ty < gy + gh), 1, s).astype(np.uint32)
    return s


def _requant(oracle, coeffs, steps):
    q = np.empty_like(coeffs)
    for s in np.unique(steps):
        m = np.broadcast_to(steps == s, coeffs.shape)
        q[m] = oracle.quant(coeffs[m], int(s))
    return q


@pytest.mark.parametrize("block", [8, 16])
def test_decode_frames(native, oracle, refs, block):
    """svc_hip_decode_frames: coefficient planes that are the correctly rounded transform of the placement input (same uneven work
    split: idct_kernel walks the same segment columns), followed by frames of coefficient impulses -- one coefficient per tile, at each
    of the N^2 positions, so that every basis entry of both inverse passes shows on its own.  Steps {1, 640} and {3, 17}, mixed region
    ids, without and with a gaze rectangle whose edges run through MV blocks (twice the tile) and through tiles."""
    lo, _ = refs.bounds(("placement", block), block, block)
    n0, _, h, w = lo.shape
    tiles = (w // block) * (h // block)
    extra = -(-block * block // tiles)
    imp = np.zeros((extra, 3, h, w), F32)
    for i in range(block * block):
        f, r = divmod(i, tiles)
        ty, tx = divmod(r, w // block)
        for c in range(3):
            p = (i + 17 * c) % (block * block)
            imp[f, c, ty * block + p // block, tx * block + p % block] = 1000.0 if (i + c) % 2 == 0 else -1000.0
    planes = np.concatenate([lo, imp])
    n, mv = len(planes), 2 * block
    types = _random_types(31 + block, n, w, h, mv)
    types[n0:] = 5  # the impulse frames: foreground
    d_planes, t = _cuda(planes), _i32(types)
    for fg, bg in ((1, 640), (3, 17)):
        for gaze in ((0, 0, 0, 0), (40, 8, 72, h - 24)):
            got = native.decode_frames(d_planes, block, t, mv, fg, bg, gaze).cpu().numpy().transpose(0, 3, 1, 2)
            amb = tot = 0
            for f in range(n):
                q = _requant(oracle, planes[f], _decode_steps(types[f], w, h, block, mv, fg, bg, gaze))
                ref, a = tr.idct_ref(q, block, block), tr.inverse_slack(q, block, block)
                # the oracle's f64 statement agrees with the reference within A': pins the step choice above to the oracle's
                f64 = oracle.decode_frame(planes[f], block, types[f], mv, fg, bg, gaze).transpose(2, 0, 1)
                assert (np.abs(f64.astype(np.longdouble) - ref) <= a).all(), (f, fg, bg, gaze)
                rlo, rhi = tr.interval(ref, a)
                if f < n0 - 1:
                    amb, tot = amb + int((rlo != rhi).sum()), tot + rlo.size
                _assert_raw(got[f], rlo, rhi, f"decode_frames {block}, frame {f}, steps ({fg}, {bg}), gaze {gaze}")
            _say(f"decode_frames {block} steps ({fg}, {bg}) gaze {gaze}: ambiguous share {amb / tot:.3e} of {tot} random-content pixels")
            assert amb <= tr.RAW_AMBIGUOUS_CAP * tot


# ---- the fused kernels' quantiser at every tie ------------------------------------------------------------------------------------------

def _probe():
    from scalable_video_codec_amd import build as b
    if not os.path.exists(b.LIB_QUANT_PROBE):
        b.build_quant_probe()
    lib = ctypes.CDLL(b.LIB_QUANT_PROBE)
    lib.svc_quant_probe.restype = ctypes.c_int
    lib.svc_quant_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
    return lib


def _around(x32, ulps=3):
    """Every f32 within `ulps` of each (positive, normal) value of x32, both signs."""
    i = np.asarray(x32, F32).view(np.int32).astype(np.int64)[:, None] + np.arange(-ulps, ulps + 1)[None, :]
    v = i.ravel().astype(np.int32).view(F32)
    return np.concatenate([v, -v])


@pytest.mark.parametrize("step", [1, 3, 7, 640, 65535])
def test_quant_fast_keeps_the_sign_of_zero(oracle, native, step):
    """Regression: c = -0.0.  The division's correction chain returns +0.0 for it (fma(+0, step, -0) = +0) where c / step is -0.0, and
    the rounding offset took its sign from that quotient, so the fast forms gave +0.0 against the reference's -0.0.  It now takes the
    sign of c * inv."""
    c = np.array([-0.0, 0.0, -0.0, -0.0, 0.0, 0.0], F32)
    want = oracle.quant(c, step)
    assert want.view(np.uint32).tolist() == [0x80000000, 0, 0x80000000, 0x80000000, 0, 0]
    lib, steps = _probe(), np.full(len(c), step, np.uint32)
    for form in range(3):
        got = np.empty_like(c)
        assert lib.svc_quant_probe(c.ctypes.data, steps.ctypes.data, got.ctypes.data, len(c), form) == 0
        assert got.tobytes() == want.tobytes(), (form, got)


TIE_STEPS = list(range(1, 2049)) + list(range(2048 + 997, 70001, 997)) + [65535]
TIE_LIMIT = 255 * 64 * 1.01  # the largest coefficient a 64 x 64 tile of bytes has, and a little


def test_quant_fast_at_every_tie(native, oracle):
    """quant1_fast and quant2_fast (even and odd lane) == the oracle's c / step; round; * step, byte for byte, on both signs of every
    f32 within 3 ulps of every tie (k + 1/2) * step up to |c| <= 255 * 64 * 1.01, for steps 1 ... 2048, every 997th up to 70 000 and
    65535; on 0, -0, the smallest normal, step / 2 and its neighbours; and on test_quant_bit_exact's random set.  (Losing the
    correction step of the division changes about 1e-5 of random coefficients at step 3 and none at step 5: only ties show it.)"""
    vals, steps = [], []
    for s in TIE_STEPS:
        k = np.arange(0, int(TIE_LIMIT / s + 0.5) + 1, dtype=np.float64)
        ties = (k + 0.5) * s
        ties = ties[ties <= TIE_LIMIT]
        v = np.concatenate([_around(ties.astype(F32)) if len(ties) else np.empty(0, F32),
                            _around(np.array([0.5 * s], F32), 1),
                            np.array([0.0, -0.0, np.finfo(F32).tiny, -np.finfo(F32).tiny], F32)])
        vals.append(v)
        steps.append(np.full(len(v), s, np.uint32))
    for s in (1, 3, 7, 640, 65535):  # tests/test_gpu_dct_quant.py::test_quant_bit_exact's inputs
        rng = np.random.default_rng(s)
        c = (rng.standard_normal(100003) * 900).astype(F32)
        c[:7] = [0.0, -0.0, 0.5 * s, -0.5 * s, 1.5 * s, 4080.0, -4080.0]
        vals.append(c)
        steps.append(np.full(len(c), s, np.uint32))
    want = np.concatenate([oracle.quant(v, int(s[0])) for v, s in zip(vals, steps)])
    vals, steps = np.ascontiguousarray(np.concatenate(vals)), np.ascontiguousarray(np.concatenate(steps))
    _say(f"quant_fast: {len(vals)} inputs over {len(TIE_STEPS)} steps")
    assert len(vals) > 1_900_000
    lib = _probe()
    for form, name in enumerate(("quant1_fast", "quant2_fast even lane", "quant2_fast odd lane")):
        got = np.empty_like(vals)
        rc = lib.svc_quant_probe(vals.ctypes.data, steps.ctypes.data, got.ctypes.data, len(vals), form)
        assert rc == 0, f"svc_quant_probe: hip error {rc}"
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (f"{name}: {int(bad.sum())} of {len(vals)} differ from the oracle, first: c = {vals[bad][0]!r}, "
                               f"step {steps[bad][0]}, got {got[bad][0]!r}, want {want[bad][0]!r}")
