"""The step's entry points at the weakest placement include/svc_hip.h admits: the transform family, luma and pyramids, the wire records,
the plane decoder, the SSE, the quantiser and the foreground count.  The machinery is tests/test_gpu_placement_streams.py's (Case, the
"one notch below" rule) with tests/test_gpu_guard_step.py's Gapped for every output given with a stride; the inputs are those of
tests/test_gpu_transform_exact.py (the tuned kernels' placement frames, the general kernel's frames) and seeded noise.

Every stride is the smallest admissible value that is not also a multiple of the next power of two: frames and pyramids 16 mod 32,
records 4 mod 8, and where the header asks nothing of a stride, an odd one.  The tuned transform kernels (8 x 8 and 16 x 16 on widths
that are multiples of 16) take frames at 16 and planes at 8 bytes; the general kernel takes frames anywhere and planes at 4.

Per case: guards intact and the bytes between strided frames unchanged; every output bit for bit that of the same call on 256-byte
aligned, tightly strided buffers; and the reference -- the oracle exactly for luma, pyramids, records, quantiser and SSE, the half-ulp
intervals of tests/helpers/transform_ref.py for the float transforms and the inverse, their caps taken from the reference first.
"""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.helpers import transform_inputs as ti
from tests.helpers import transform_ref as tr
from tests.test_gpu_decode_levels import _check_display
from tests.test_gpu_guard_step import Gapped
from tests.test_gpu_guard_streams import NS, _cuda, _windows
from tests.test_gpu_placement_streams import Case
from tests.test_gpu_transform_exact import (_assert_quant, _assert_raw, _decode_steps, _parse_records, _quant_bounds, _random_types, _requant,
                                            _tile_types)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tr.available(), reason=tr.UNAVAILABLE)]

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32

# the documented alignment of every pointer (include/svc_hip.h at each entry point; csrc/capi.hip's preconditions)
A_OUT = {"planes (tuned)": 8, "planes (general)": 4, "planes": 4, "level 0": 16, "pyramids": 16, "pyramids (any)": 1, "records": 4,
         "workspace": 16, "rec (planes)": 8, "rec": 4, "display": 1, "sse": 8, "count": 4}
A_IN = {"bgr": 16, "bgr (any)": 1, "types": 4, "planes": 16, "planes (any)": 4, "records": 4, "gaze": 4, "rec": 4, "level 0": 1}
# the pointers whose alignment the header words and the entry point checks (the rest are typed pointers of which it asks no more than C does)
REFUSES = {"dct": ("bgr", "planes (tuned)", "planes (general)"), "dct_quant": ("bgr", "planes (tuned)", "planes (general)"),
           "dct_quant_luma": ("bgr", "planes (tuned)", "level 0"), "dct_quant_redo": ("bgr", "planes (tuned)", "workspace"),
           "dct_records": ("bgr", "records"), "dct_records_luma": ("bgr", "records", "level 0"), "luma_pyramid": ("bgr", "pyramids"),
           "pyramid_levels": (), "serialize": ("records",), "wire_patch_types": ("records",), "decode": ("planes", "rec (planes)"),
           "decode_records": ("records", "rec", "gaze"), "sse": ("sse",), "quant": (), "count_foreground": ()}
ORDER = (0, 1, 2, 1, 0)  # the frames of a 3-frame input that a batch of 1, 3 or 5 takes


def _stride(pool, least, granule):
    """Tight when everything is aligned; else the smallest multiple of `granule` >= least that is no multiple of 2 * granule."""
    s = -(-least // granule) * granule
    return s + granule if pool.place is not None and s % (2 * granule) == 0 else s


def _strided_in(frames, stride, seed):
    """(n, ...) u8 frames `stride` apart in a flat device buffer that ends with the last frame; noise between them."""
    n, per = frames.shape[0], frames[0].size
    host = np.random.default_rng(seed).integers(0, 256, (n - 1) * stride + per, dtype=np.uint8)
    for f in range(n):
        host[f * stride:f * stride + per] = frames[f].reshape(-1)
    return _cuda(host)


def _gapped(pool, name, n, used, stride):
    g = Gapped(n, used, stride, seed=len(pool.written), at=None if pool.place is None else pool.place[name])
    pool.written[name] = g.g
    return g


@functools.lru_cache(maxsize=None)
def _tuned(block):
    """The tuned kernels' placement input: (frames (3, H, W, 3), lo, hi (3, 3, H, W)), the raw cap asserted on its random content."""
    frames, special = ti.tuned_placement_frames(block)
    a = tr.forward_slack(block, block)
    lo, hi = (np.stack(x) for x in zip(*(tr.interval(tr.dct_ref(f, block, block), a) for f in frames)))
    rnd = ~np.stack([special[:-1]] * 3, axis=1)
    assert float((lo[:-1] != hi[:-1])[rnd].mean()) <= tr.RAW_AMBIGUOUS_CAP
    return frames, lo, hi


@functools.lru_cache(maxsize=None)
def _general(bw, bh):
    frames, special = ti.general_frames(bw, bh)
    a = tr.forward_slack(bw, bh)
    lo, hi = (np.stack(x) for x in zip(*(tr.interval(tr.dct_ref(f, bw, bh), a) for f in frames)))
    assert float((lo[:1] != hi[:1])[~np.stack([special[:1]] * 3, axis=1)].mean()) <= tr.RAW_AMBIGUOUS_CAP
    return frames, lo, hi


def _input(form, n):
    """form: ("tuned", N) or ("general", (bw, bh), MV block) -> (frames (n, H, W, 3), lo, hi (n, 3, H, W), (bw, bh), MV block side)."""
    if form[0] == "tuned":
        frames, lo, hi = _tuned(form[1])
        idx = list(ORDER[:n])
        return frames[idx], lo[idx], hi[idx], (form[1], form[1]), 16
    frames, lo, hi = _general(*form[1])
    idx = [f % 2 for f in range(n)]
    return frames[idx], lo[idx], hi[idx], form[1], form[2]


def _types_of(form, n, w, h, mv):
    return _random_types(77 + sum(form[1]) if form[0] == "general" else 77 + form[1], n, w, h, mv)


FORMS = [("tuned", 8), ("tuned", 16), ("general", (6, 10), 30), ("general", (8, 8), 8)]  # both general paths: not square; square off 16
TUNED = FORMS[:2]


def _fid(form):
    return f"{form[0]}-{form[1]}" if form[0] == "tuned" else f"general-{form[1][0]}x{form[1][1]}"


def _bgr_in(pool, form, frames):
    """The frames as the entry point takes them for this kernel form: name, buffer, stride."""
    per = frames[0].size
    if form[0] == "tuned":
        stride = _stride(pool, per, 16)
        return "bgr", _strided_in(frames, stride, per), stride
    stride = _stride(pool, per, 1)
    return "bgr (any)", _strided_in(frames, stride, per), stride


# ---- the transform family ----------------------------------------------------------------------------------------------------------------------

def e_dct(pool, form, n, seed):
    frames, lo, hi, (bw, bh), _ = _input(form, n)
    _, h, w, _ = frames.shape
    name, buf, stride = _bgr_in(pool, form, frames)
    planes = pool.buf(f"planes ({form[0]})", (n, 3, h, w), F32)

    def call(i):
        nat._check(nat.load().svc_hip_dct_frames(i[name].data_ptr(), stride, n, w, h, bw, bh, planes.data_ptr(), nat._stream()))
        return {"planes": planes}
    return {name: buf}, call


def ref_dct(c, got, oracle):
    _, lo, hi, _, _ = _input(c.geom, c.n)
    _assert_raw(got["planes"].numpy(), lo, hi, f"dct_frames {_fid(c.geom)}")


QUANT = (3, 17)


def e_dct_quant(pool, form, n, seed):
    frames, lo, hi, (bw, bh), mv = _input(form, n)
    _, h, w, _ = frames.shape
    name, buf, stride = _bgr_in(pool, form, frames)
    types = _types_of(form, n, w, h, mv)
    planes = pool.buf(f"planes ({form[0]})", (n, 3, h, w), F32)

    def call(i):
        nat._check(nat.load().svc_hip_dct_quant_frames(i[name].data_ptr(), stride, n, w, h, bw, bh, i["types"].data_ptr(), mv, mv, *QUANT,
                                                      planes.data_ptr(), nat._stream()))
        return {"planes": planes}
    return {name: buf, "types": _cuda(types.view(np.int32))}, call


def ref_dct_quant(c, got, oracle):
    frames, lo, hi, _, mv = _input(c.geom, c.n)
    types = _types_of(c.geom, c.n, frames.shape[2], frames.shape[1], mv)
    _assert_quant(got["planes"].numpy(), *_quant_bounds(oracle, lo, hi, types, (mv, mv), *QUANT), f"dct_quant_frames {_fid(c.geom)}")


def e_dct_quant_luma(pool, form, n, seed):
    frames, lo, hi, (block, _), _ = _input(form, n)
    _, h, w, _ = frames.shape
    name, buf, stride = _bgr_in(pool, form, frames)
    planes = pool.buf("planes (tuned)", (n, 3, h, w), F32)
    luma = _gapped(pool, "level 0", n, w * h, _stride(pool, w * h, 16))

    def call(i):
        luma.arm()
        nat._check(nat.load().svc_hip_dct_quant_luma_frames(i[name].data_ptr(), stride, n, w, h, block, 640, planes.data_ptr(),
                                                           luma.g.addr, luma.stride, nat._stream()))
        return {"planes": planes, **luma.outputs("level 0")}
    return {name: buf}, call


def _luma_is_the_oracles(got, frames, oracle):
    n, h, w, _ = frames.shape
    assert np.array_equal(got["level 0"].numpy().reshape(n, h, w), np.stack([oracle.luma(f) for f in frames]))


def ref_dct_quant_luma(c, got, oracle):
    frames, lo, hi, _, mv = _input(c.geom, c.n)
    none = np.zeros((c.n, (frames.shape[2] // mv) * (frames.shape[1] // mv)), np.uint32)
    _assert_quant(got["planes"].numpy(), *_quant_bounds(oracle, lo, hi, none, (mv, mv), 1, 640), f"dct_quant_luma_frames {_fid(c.geom)}")
    _luma_is_the_oracles(got, frames, oracle)


def e_dct_quant_redo(pool, form, n, seed):
    frames, lo, hi, (block, _), mv = _input(form, n)
    _, h, w, _ = frames.shape
    name, buf, stride = _bgr_in(pool, form, frames)
    types = _types_of(form, n, w, h, mv)
    spec, _, _ = nat.dct_quant_luma_frames(_cuda(frames), block, 1, bg_step=640)  # the speculative planes the redo starts from
    need = int(nat.load().svc_hip_dct_redo_workspace_bytes(n, w, h, mv, mv))
    planes = pool.buf("planes (tuned)", (n, 3, h, w), F32)
    ws = pool.buf("workspace", need, U8)

    pool.before_call = lambda: planes.copy_(spec)  # the planes are input and output

    def call(i):
        pool.before_call()
        nat._check(nat.load().svc_hip_dct_quant_redo_frames(i[name].data_ptr(), stride, n, w, h, block, i["types"].data_ptr(), mv, mv, 7,
                                                           planes.data_ptr(), ws.data_ptr(), need, nat._stream()))
        return {"planes": planes}
    return {name: buf, "types": _cuda(types.view(np.int32))}, call


def ref_dct_quant_redo(c, got, oracle):
    frames, lo, hi, _, mv = _input(c.geom, c.n)
    types = _types_of(c.geom, c.n, frames.shape[2], frames.shape[1], mv)
    _assert_quant(got["planes"].numpy(), *_quant_bounds(oracle, lo, hi, types, (mv, mv), 7, 640), f"dct_quant_redo_frames {_fid(c.geom)}")


def _records_entry(with_luma):
    def build(pool, form, n, seed):
        frames, lo, hi, (block, _), mv = _input(form, n)
        _, h, w, _ = frames.shape
        name, buf, stride = _bgr_in(pool, form, frames)
        types = _types_of(form, n, w, h, mv)
        per = nat.serialized_frame_bytes(w, h, block, block)
        rec = _gapped(pool, "records", n, per, _stride(pool, per, 4))
        luma = _gapped(pool, "level 0", n, w * h, _stride(pool, w * h, 16)) if with_luma else None
        lib = nat.load()

        def call(i):
            rec.arm()
            if with_luma:
                luma.arm()
                nat._check(lib.svc_hip_dct_records_luma_frames(i[name].data_ptr(), stride, n, w, h, block, h, rec.g.addr, rec.stride,
                                                               luma.g.addr, luma.stride, nat._stream()))
                return {**rec.outputs("records"), **luma.outputs("level 0")}
            nat._check(lib.svc_hip_dct_records_frames(i[name].data_ptr(), stride, n, w, h, block, i["types"].data_ptr(), mv, mv, *QUANT, h,
                                                      rec.g.addr, rec.stride, nat._stream()))
            return rec.outputs("records")
        return ({name: buf} if with_luma else {name: buf, "types": _cuda(types.view(np.int32))}), call
    return build


def ref_dct_records(c, got, oracle):
    frames, lo, hi, (block, _), mv = _input(c.geom, c.n)
    _, h, w, _ = frames.shape
    types = _types_of(c.geom, c.n, w, h, mv)
    tw, planes = _parse_records(got["records"].numpy().reshape(c.n, -1), w, h, block)
    assert np.array_equal(tw, _tile_types(types, w, h, mv, block, h // block))
    _assert_quant(planes, *_quant_bounds(oracle, lo, hi, types, (mv, mv), *QUANT), f"dct_records_frames {_fid(c.geom)}")


def ref_dct_records_luma(c, got, oracle):
    frames, lo, hi, (block, _), _ = _input(c.geom, c.n)
    _, h, w, _ = frames.shape
    tw, planes = _parse_records(got["records"].numpy().reshape(c.n, -1), w, h, block)
    assert not tw.any()
    _assert_raw(planes, lo, hi, f"dct_records_luma_frames {_fid(c.geom)}")
    _luma_is_the_oracles(got, frames, oracle)


# ---- luma and pyramids ---------------------------------------------------------------------------------------------------------------------------

PYRAMIDS = [(48, 16, 4), (40, 24, 4)]  # whole 16-pixel segments (level 1 inside the luma kernel); 40: a pixel per lane, then plane to plane


def _noise_frames(w, h, n):
    return np.random.default_rng(w * 31 + h + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def e_luma_pyramid(pool, geom, n, seed):
    w, h, levels = geom
    frames = _noise_frames(w, h, n)
    stride = _stride(pool, w * h * 3, 16)
    exact = nat.pyramid_bytes(w, h, levels)
    out = _gapped(pool, "pyramids", n, exact, _stride(pool, exact, 16))

    def call(i):
        out.arm()
        nat._check(nat.load().svc_hip_luma_pyramid_frames(i["bgr"].data_ptr(), stride, n, w, h, levels, out.g.addr, out.stride, nat._stream()))
        return out.outputs("pyramids")
    return {"bgr": _strided_in(frames, stride, w)}, call


def _packed(pyr):
    return np.concatenate([p.reshape(-1) for p in pyr])


def ref_luma_pyramid(c, got, oracle):
    w, h, levels = c.geom
    want = np.stack([_packed(oracle.luma_pyramid(f, levels)) for f in _noise_frames(w, h, c.n)])
    assert np.array_equal(got["pyramids"].numpy().reshape(c.n, -1), want)


def e_pyramid_levels(pool, geom, n, seed):
    """No alignment is asked of d_pyr or its stride: an odd base and an odd stride (the plane-to-plane kernel; aligned, the strip kernel)."""
    w, h, levels = geom
    planes = _cuda(_noise_frames(w, h, n)[..., 1].reshape(n, h * w).copy())
    exact = nat.pyramid_bytes(w, h, levels)
    out = _gapped(pool, "pyramids (any)", n, exact, _stride(pool, exact, 1))

    def call(i):
        for f in range(n):  # level 0 is input and output: in place before every call
            out.g.interior[f * out.stride:f * out.stride + w * h] = i["level 0"][f]
        out.arm()
        nat._check(nat.load().svc_hip_pyramid_levels_frames(out.g.addr, out.stride, n, w, h, levels, nat._stream()))
        return out.outputs("pyramids (any)")
    return {"level 0": planes}, call


def ref_pyramid_levels(c, got, oracle):
    w, h, levels = c.geom
    for f, level0 in enumerate(_noise_frames(w, h, c.n)[..., 1]):
        pyr = [np.ascontiguousarray(level0)]
        for _ in range(levels - 1):
            pyr.append(oracle.pyr_down(pyr[-1]))
        assert np.array_equal(got["pyramids (any)"].numpy().reshape(c.n, -1)[f], _packed(pyr)), f


# ---- the wire records -----------------------------------------------------------------------------------------------------------------------------

WIRE = [(48, 32, 8, 16), (64, 32, 16, 16)]  # w, h, transform block, MV block


def _wire_case(geom, n):
    w, h, tb, mv = geom
    rng = np.random.default_rng(w + tb + n)
    planes = (rng.standard_normal((n, 3, h, w)) * 300).astype(np.float32)
    return planes, _random_types(w + tb, n, w, h, mv)


def e_serialize(pool, geom, n, seed):
    w, h, tb, mv = geom
    planes, types = _wire_case(geom, n)
    per = nat.serialized_frame_bytes(w, h, tb, tb)
    out = _gapped(pool, "records", n, per, _stride(pool, per, 4))

    def call(i):
        out.arm()
        nat._check(nat.load().svc_hip_serialize_frames(i["planes (any)"].data_ptr(), h * w, n, i["types"].data_ptr(), w, h, tb, tb, w // mv, h // mv,
                                                      mv, mv, out.g.addr, out.stride, nat._stream()))
        return out.outputs("records")
    return {"planes (any)": _cuda(planes), "types": _cuda(types.view(np.int32))}, call


def _wire_records(oracle, geom, n, types=None):
    w, h, tb, mv = geom
    planes, t = _wire_case(geom, n)
    t = t if types is None else types
    return np.stack([oracle.serialize_frame(planes[f], t[f], w, h, tb, tb, w // mv, mv, mv) for f in range(n)])


def ref_serialize(c, got, oracle):
    assert np.array_equal(got["records"].numpy().reshape(c.n, -1), _wire_records(oracle, c.geom, c.n))


def e_wire_patch_types(pool, geom, n, seed):
    """Records serialised with every region id 0 (what the front of the step emits), then the foreground ids patched in: the records of the
    same planes serialised with the ids."""
    from oracle.binding import Oracle
    w, h, tb, mv = geom
    _, types = _wire_case(geom, n)
    blank = torch.from_numpy(_wire_records(Oracle(), geom, n, np.zeros_like(types))).cuda()
    per = blank.shape[1]
    out = _gapped(pool, "records", n, per, _stride(pool, per, 4))

    def before():  # the records are input and output
        for f in range(n):
            out.g.interior[f * out.stride:f * out.stride + per] = blank[f]
    pool.before_call = before

    def call(i):
        before()
        out.arm()
        nat._check(nat.load().svc_hip_wire_patch_types_frames(i["types"].data_ptr(), n, w, h, h, tb, mv, mv, out.g.addr, out.stride, 0,
                                                             nat._stream()))
        return out.outputs("records")
    return {"types": _cuda(types.view(np.int32))}, call


ref_wire_patch_types = ref_serialize


# ---- the decoders of planes and of records, the SSE, the quantiser, the count ------------------------------------------------------------------

GAZE = (40, 8, 72, 16)
DEC = (3, 17)


def _rec_bounds(oracle, coeffs, types, w, h, block, mv, gazes):
    """[lo, hi] of every pixel (tests/test_gpu_transform_exact.py::test_decode_frames), the raw cap from the reference alone."""
    out, amb, tot = [], 0, 0
    for f in range(len(coeffs)):
        q = _requant(oracle, coeffs[f], _decode_steps(types[f], w, h, block, mv, *DEC, gazes[f]))
        rlo, rhi = tr.interval(tr.idct_ref(q, block, block), tr.inverse_slack(q, block, block))
        out.append((rlo, rhi))
        amb, tot = amb + int((rlo != rhi).sum()), tot + rlo.size
    assert amb <= tr.RAW_AMBIGUOUS_CAP * tot, amb / tot
    return out


def e_decode(pool, form, n, seed):
    _, lo, _, (block, _), _ = _input(form, n)
    _, _, h, w = lo.shape
    mv = 2 * block
    types = _random_types(31 + block, n, w, h, mv)
    rec = pool.buf("rec (planes)", (n, h, w, 3), F32)

    def call(i):
        nat._check(nat.load().svc_hip_decode_frames(i["planes"].data_ptr(), n, w, h, block, i["types"].data_ptr(), mv, mv, *DEC, *GAZE,
                                                   rec.data_ptr(), nat._stream()))
        return {"rec": rec}
    return {"planes": _cuda(lo), "types": _cuda(types.view(np.int32))}, call


def ref_decode(c, got, oracle):
    _, lo, _, (block, _), _ = _input(c.geom, c.n)
    _, _, h, w = lo.shape
    types = _random_types(31 + block, c.n, w, h, 2 * block)
    for f, (rlo, rhi) in enumerate(_rec_bounds(oracle, lo, types, w, h, block, 2 * block, [GAZE] * c.n)):
        _assert_raw(got["rec"][f].numpy().transpose(2, 0, 1), rlo, rhi, f"decode_frames {_fid(c.geom)} frame {f}")


@functools.lru_cache(maxsize=None)
def _decode_records_case(form, n):
    from oracle.binding import Oracle
    _, lo, _, (block, _), mv = _input(form, n)
    _, _, h, w = lo.shape
    types = _random_types(41 + block, n, w, h, mv)
    records = np.stack([Oracle().serialize_frame(lo[f], types[f], w, h, block, block, w // mv, mv, mv) for f in range(n)])
    return lo, types, records, block, mv, w, h


def e_decode_records(pool, form, n, seed):
    lo, types, records, block, mv, w, h = _decode_records_case(form, n)
    stride = _stride(pool, records.shape[1], 4)
    dw, dh = w - 5, h - 3
    rec = pool.buf("rec", (n, h, w, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)

    def call(i):
        nat._check(nat.load().svc_hip_decode_records_frames(i["records"].data_ptr(), stride, n, w, h, block, h, *DEC, i["gaze"].data_ptr(),
                                                           rec.data_ptr(), disp.data_ptr(), dw, dh, nat._stream()))
        return {"rec": rec, "display": disp}
    return {"records": _strided_in(records, stride, block), "gaze": _windows(n, w, h)}, call


def ref_decode_records(c, got, oracle):
    lo, types, _, block, mv, w, h = _decode_records_case(c.geom, c.n)
    gazes = [tuple(int(v) for v in g) for g in c.inputs["gaze"].cpu().numpy().view(np.uint32).reshape(c.n, 4)]
    dh, dw = got["display"].shape[1:3]
    for f, (rlo, rhi) in enumerate(_rec_bounds(oracle, lo, types, w, h, block, mv, gazes)):
        rec = got["rec"][f].numpy()
        _assert_raw(rec.transpose(2, 0, 1), rlo, rhi, f"decode_records_frames {_fid(c.geom)} frame {f}")
        _check_display(rec, got["display"][f].numpy(), dw, dh)


SSE = [(96, 40)]


def _sse_case(geom, n):
    w, h = geom
    rng = np.random.default_rng(w + n)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    rec = (frames.astype(np.float32) + rng.standard_normal(frames.shape).astype(np.float32) * 9).astype(np.float32)
    return frames, rec


def e_sse(pool, geom, n, seed):
    """Nothing is asked of the source frames or their stride: an odd base and an odd stride; the sums are 8-byte aligned."""
    w, h = geom
    frames, rec = _sse_case(geom, n)
    stride = _stride(pool, w * h * 3, 1)
    sse = pool.buf("sse", n, I64)

    def call(i):
        nat._check(nat.load().svc_hip_sse_frames(i["bgr (any)"].data_ptr(), stride, i["rec"].data_ptr(), n, w, h, w - 5, h - 3, sse.data_ptr(),
                                                nat._stream()))
        return {"sse": sse}
    return {"bgr (any)": _strided_in(frames, stride, w), "rec": _cuda(rec)}, call


def ref_sse(c, got, oracle):
    w, h = c.geom
    frames, rec = _sse_case(c.geom, c.n)
    assert got["sse"].tolist() == [oracle.sse_frame(frames[f], rec[f], w - 5, h - 3) for f in range(c.n)]


def e_quant(pool, geom, n, seed):
    w, h, _, mv = geom
    coeffs, types = _wire_case(geom, n)
    start = _cuda(coeffs)
    planes = pool.buf("planes", (n, 3, h, w), F32)

    def call(i):
        planes.copy_(start)  # in place
        nat._check(nat.load().svc_hip_quant_frames(planes.data_ptr(), n, w, h, mv, mv, i["types"].data_ptr(), *DEC, nat._stream()))
        return {"planes": planes}
    return {"types": _cuda(types.view(np.int32))}, call


def ref_quant(c, got, oracle):
    w, h, _, mv = c.geom
    coeffs, types = _wire_case(c.geom, c.n)
    want = np.stack([oracle.quant_frame(coeffs[f], mv, mv, types[f], *DEC) for f in range(c.n)])
    assert got["planes"].numpy().tobytes() == want.tobytes()


def e_count_foreground(pool, geom, n, seed):
    w, h, _, mv = geom
    _, types = _wire_case(geom, n)
    count = pool.buf("count", 1, I32)

    def call(i):
        count.zero_()
        nat._check(nat.load().svc_hip_count_foreground(i["types"].data_ptr(), types.size, count.data_ptr(), nat._stream()))
        return {"count": count}
    return {"types": _cuda(types.view(np.int32))}, call


def ref_count_foreground(c, got, oracle):
    assert got["count"].tolist() == [int((_wire_case(c.geom, c.n)[1] != 0).sum())]


ENTRIES = {
    "dct": (e_dct, FORMS), "dct_quant": (e_dct_quant, FORMS), "dct_quant_luma": (e_dct_quant_luma, TUNED), "dct_quant_redo": (e_dct_quant_redo, TUNED),
    "dct_records": (_records_entry(False), TUNED), "dct_records_luma": (_records_entry(True), TUNED),
    "luma_pyramid": (e_luma_pyramid, PYRAMIDS), "pyramid_levels": (e_pyramid_levels, PYRAMIDS),
    "serialize": (e_serialize, WIRE), "wire_patch_types": (e_wire_patch_types, WIRE),
    "decode": (e_decode, TUNED), "decode_records": (e_decode_records, TUNED), "sse": (e_sse, SSE), "quant": (e_quant, WIRE),
    "count_foreground": (e_count_foreground, WIRE[:1]),
}
REFERENCES = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("ref_")}
assert sorted(REFERENCES) == sorted(ENTRIES)
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms]


def _gid(g):
    return _fid(g) if isinstance(g[0], str) else "x".join(str(v) for v in g)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_at_the_weakest_placement(native, oracle, entry, geom):
    for n in NS:
        aligned = Case(entry, geom, n, table=ENTRIES).run()
        c = Case(entry, geom, n, A_OUT, A_IN, table=ENTRIES)
        for k, g in c.pool.written.items():
            assert g.addr % (2 * A_OUT[k]) == A_OUT[k], (entry, k)
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * A_IN[k]) == A_IN[k], (entry, k)
        got = c.run()
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", aligned, got, "differs from the same call on aligned, tightly strided buffers")
        assert not findings, "\n".join(findings)
        REFERENCES[entry](c, got, oracle)


NOTCHES = [(e, g) for e, (_, geoms) in ENTRIES.items() if REFUSES[e] for g in (geoms if geoms is FORMS else geoms[:1])
           if geoms is not FORMS or g in (FORMS[0], FORMS[2])]  # the transform: the tuned and the general kernel's preconditions


@pytest.mark.parametrize("entry,geom", NOTCHES, ids=[f"{e}-{_gid(g)}" for e, g in NOTCHES])
def test_one_notch_below_is_refused(native, entry, geom):
    """Each pointer whose alignment the header words, alone at exactly(A / 2): SVC_ERR_INVALID_ARG, a message that names alignment, no
    byte of any output changed."""
    n = 3
    probe = Case(entry, geom, n, A_OUT, A_IN, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if k in REFUSES[entry]] + [("in", k) for k in probe.inputs if k in REFUSES[entry]]
    assert rows and all((A_OUT if side == "out" else A_IN)[k] > 1 for side, k in rows), rows
    for side, name in rows:
        out_at = {**A_OUT, name: A_OUT[name] // 2} if side == "out" else A_OUT
        in_at = {**A_IN, name: A_IN[name] // 2} if side == "in" else A_IN
        c = Case(entry, geom, n, out_at, in_at, table=ENTRIES)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' one notch below"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
