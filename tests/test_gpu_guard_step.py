"""Where the step's kernels write, and whether their results depend on bytes next to their inputs (tests/helpers/guarded.py).

These entry points take no workspace; their outputs have fixed sizes and some of their buffers are given with a stride.  Every output
is a Guarded of exactly its size (a strided one ends where its last frame's data ends), filled with zeros, 0xFF and random bytes before
the call; every input is surrounded with two seeds of noise, one input at a time.  The claims this pins: the luma and pyramid kernels
reflect at the borders and leave the bytes between two frames' pyramids alone; hbma_fused_kernel reads top-level dwords "where they
lie, only the plane's end guarded" without the result depending on what lies past the plane; the transform kernels read frames given
with a stride and nothing between them.  What each call computes is pinned elsewhere on the same inputs: tests/test_gpu_ransac_pyramid.py,
tests/test_gpu_hbma.py (test_top_level_rows_that_are_not_whole_dwords, test_hbma_tiled_kernel), tests/test_gpu_transform_exact.py (the
placement input), tests/test_gpu_decode.py, tests/test_gpu_decode_records.py.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests import util
from tests.helpers import guarded as gd
from tests.helpers import transform_inputs as ti
from tests.test_gpu_transform_exact import _random_types

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(frames, extra=48):
    """(n, ...) u8 frames -> (flat buffer with `extra` bytes of noise between the frames, ending where the last frame ends; stride)."""
    n = frames.shape[0]
    per = frames[0].numel()
    buf = torch.randint(0, 256, (n * (per + extra) - extra,), dtype=U8, device="cuda")
    for f in range(n):
        buf[f * (per + extra):f * (per + extra) + per] = frames[f].reshape(-1)
    return buf, per + extra


class Gapped:
    """An output of n frames of `used` bytes each, `stride` apart, in a Guarded that ends with the last frame: the frames are the
    defined output, the bytes between them must come back unchanged."""

    def __init__(self, n, used, stride, seed=0, at=None):
        """at: None (256-byte aligned), or A: the first frame lies at gd.exactly(A)."""
        self.n, self.used, self.stride = n, used, stride
        self.g = gd.Guarded((n - 1) * stride + used, U8, "cuda", seed=seed, **({} if at is None else gd.exactly(at)))
        idx = torch.arange(self.g.nbytes, device="cuda") % stride
        self.gap = idx >= used
        self.before = None

    def arm(self):
        self.before = self.g.interior.clone()

    def outputs(self, name):
        buf = self.g.interior
        changed = (buf[self.gap] != self.before[self.gap]).sum().reshape(1)
        assert int(changed) == 0, f"{name}: {int(changed)} bytes between two frames' data were written"
        return {name: buf[~self.gap].clone(), f"bytes written between the frames of {name}": changed}


def _both(name, written, inputs, call):
    plain = {k: gd.surround(v, 0) for k, v in inputs.items()}
    findings = gd.check_writes(name, written, lambda: call(plain), names=("zeros", "ones", "random"))
    return findings + gd.check_reads(name, inputs, call, written)


# ---- luma and pyramids -------------------------------------------------------------------------------------------------------------------

PYRAMIDS = [(48, 16, 4), (176, 144, 4), (40, 24, 4), (128, 2, 2)]  # 40 x 24: not a multiple of 16 wide; 128 x 2: shorter than any tile


@pytest.mark.parametrize("w,h,levels", PYRAMIDS)
def test_luma_pyramid_frames(native, w, h, levels):
    n = 3
    rng = np.random.default_rng(w * 31 + h)
    frames = _cuda(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    bgr, stride = _strided(frames)
    exact = nat.pyramid_bytes(w, h, levels)
    pstride = (exact + 15) // 16 * 16 + 32
    out = Gapped(n, exact, pstride)

    def call(i):
        out.arm()
        nat._check(nat.load().svc_hip_luma_pyramid_frames(i["bgr"].data_ptr(), stride, n, w, h, levels, out.g.interior.data_ptr(), pstride,
                                                         nat._stream()))
        return out.outputs("pyramids")
    findings = _both(f"luma_pyramid_frames {w}x{h} L={levels}", {"pyramids": out.g}, {"bgr": bgr}, call)
    want, ws = nat.luma_pyramid_frames(frames, levels)  # the packed call (tests/test_gpu_ransac_pyramid.py pins it to the oracle)
    got = call({"bgr": bgr})["pyramids"].reshape(n, exact)
    assert torch.equal(got, torch.stack([want[f * ws:f * ws + exact] for f in range(n)]))
    assert not findings, "\n".join(findings)


# svc_hip_pyramid_levels_frames refuses 128 x 2 ("level 0 is too small to reduce"): 128 x 8, the shortest plane its own test gives it
@pytest.mark.parametrize("w,h,levels", PYRAMIDS[:3] + [(128, 8, 2)])
def test_pyramid_levels_frames(native, w, h, levels):
    n = 3
    rng = np.random.default_rng(w * 7 + h + levels)
    planes = _cuda(rng.integers(0, 256, (n, h * w), dtype=np.uint8))
    planes[1] = 255  # saturated: the rounding at the top of the range
    exact = nat.pyramid_bytes(w, h, levels)
    pstride = (exact + 15) // 16 * 16 + 32
    out = Gapped(n, exact, pstride)

    def call(i):
        for f in range(n):  # level 0 is input and output: in place before every call
            out.g.interior[f * pstride:f * pstride + w * h] = i["level 0"][f]
        out.arm()
        nat.pyramid_levels_frames(out.g.interior, pstride, n, w, h, levels)
        got = out.outputs("pyramids")
        assert torch.equal(got["pyramids"].reshape(n, exact)[:, :w * h], i["level 0"])  # level 0 untouched
        return got
    findings = _both(f"pyramid_levels_frames {w}x{h} L={levels}", {"pyramids": out.g}, {"level 0": planes}, call)
    assert not findings, "\n".join(findings)


# ---- the hierarchical search ---------------------------------------------------------------------------------------------------------------

FORCED = {"auto": nat.HBMA_AUTO, "wave": nat.HBMA_FORCE_WAVE_PER_BLOCK, "fused": nat.HBMA_FORCE_FUSED, "tiled": nat.HBMA_FORCE_TILED,
          "lane": nat.HBMA_FORCE_LANE}


@pytest.mark.parametrize("w,h,mb,levels", [(112, 32, 16, 4), (176, 144, 16, 4), (120, 72, 8, 3), (640, 400, 16, 4)])
def test_hbma_pairs(native, w, h, mb, levels):
    """Top planes whose rows are 14 and 22 bytes (112 and 176 wide at 4 levels), 15 bytes (120 at 3 levels of 8 x 8), and the tiled form's
    640 x 400; the pyramids packed at their exact size, so the last pair's top planes end where the input ends."""
    rng = np.random.default_rng(w + levels)
    n, r = 2, 8
    pyrs = [util.random_planes(rng, w, h, levels) for _ in range(n + 1)]
    for p in pyrs:
        p[levels - 1][-3:, -6:] = 77  # ties and clamped windows next to the plane's end
    exact = sum(p.size for p in pyrs[0])
    stride = (exact + 15) & ~15
    buf = util.pack_clip(pyrs, stride, torch.device("cuda"))[:n * stride + exact].clone()
    blocks = (w // mb) * (h // mb)
    findings, ran, results = [], [], {}
    for name, flags in FORCED.items():
        written = {"mv": gd.Guarded(8 * n * blocks, F32, "cuda", shape=(n, blocks, 2)),
                   "mad": gd.Guarded(4 * n * blocks, F32, "cuda", seed=1, shape=(n, blocks))}

        def call(i):
            p = i["pyramids"]
            nat.hbma_pairs(p, p[stride:], stride, n, levels, w, h, r, mb, mb, flags=flags, out=(written["mv"].interior, written["mad"].interior))
            return {"mv": written["mv"].interior, "mad": written["mad"].interior}
        try:
            results[name] = {k: v.clone() for k, v in call({"pyramids": buf}).items()}
        except nat.SvcError as e:  # a forced kernel that does not cover the shape
            assert name not in ("auto", "wave") and e.status == nat.SVC_ERR_UNSUPPORTED, (name, e)
            continue
        ran.append(name)
        findings += _both(f"hbma_pairs {w}x{h} L={levels} {name}", written, {"pyramids": buf}, call)
    # the lane-per-block and the fused form take all four shapes, the tiled form 640 x 400 only: a forced kernel that drops out fails here
    assert ran == ["auto", "wave", "fused"] + (["tiled"] if w == 640 else []) + ["lane"], ran
    for name in ran:  # every form gives the general kernel's vectors (tests/test_gpu_hbma.py pins those to the oracle)
        assert torch.equal(results[name]["mv"], results["wave"]["mv"]) and torch.equal(results[name]["mad"], results["wave"]["mad"]), name
    assert not findings, "\n".join(findings)


# ---- the transform's forms, on the placement input given with a stride -----------------------------------------------------------------------------

@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("form", ["dct", "dct_quant", "dct_quant_luma", "dct_records"])
def test_transform_forms(native, form, block):
    frames, _ = ti.tuned_placement_frames(block)  # 3 frames of 176 x 48 (8) or 224 x 160 (16)
    n, h, w, _ = frames.shape
    mv = 16
    bgr, stride = _strided(_cuda(frames))
    inputs = {"bgr": bgr}
    lib = nat.load()
    if form in ("dct_quant", "dct_records"):
        inputs["types"] = _cuda(_random_types(77 + block, n, w, h, mv).view(np.int32))
    if form == "dct_records":
        per = nat.serialized_frame_bytes(w, h, block, block)
        written = {"records": gd.Guarded(n * per, U8, "cuda", shape=(n, per))}
    else:
        written = {"planes": gd.Guarded(4 * n * 3 * h * w, F32, "cuda", shape=(n, 3, h, w))}
    luma = Gapped(n, w * h, w * h + 32, seed=1) if form == "dct_quant_luma" else None
    if luma is not None:
        written["level 0"] = luma.g
    out = next(iter(written.values())).interior

    def call(i):
        if form == "dct":
            nat._check(lib.svc_hip_dct_frames(i["bgr"].data_ptr(), stride, n, w, h, block, block, out.data_ptr(), nat._stream()))
        elif form == "dct_quant":
            nat._check(lib.svc_hip_dct_quant_frames(i["bgr"].data_ptr(), stride, n, w, h, block, block, i["types"].data_ptr(), mv, mv, 7, 640,
                                                   out.data_ptr(), nat._stream()))
        elif form == "dct_quant_luma":
            luma.arm()
            nat._check(lib.svc_hip_dct_quant_luma_frames(i["bgr"].data_ptr(), stride, n, w, h, block, 640, out.data_ptr(),
                                                        luma.g.interior.data_ptr(), luma.stride, nat._stream()))
            return {"planes": out, **luma.outputs("level 0")}
        else:
            nat._check(lib.svc_hip_dct_records_frames(i["bgr"].data_ptr(), stride, n, w, h, block, i["types"].data_ptr(), mv, mv, 7, 640, h,
                                                     out.data_ptr(), out.stride(0), nat._stream()))
            return {"records": out}
        return {"planes": out}
    findings = _both(f"{form}_frames {block}", written, inputs, call)
    # the pin: the same call on contiguous frames through the binding (tests/test_gpu_transform_exact.py checks that one)
    packed = _cuda(frames)
    want = {"dct": lambda: nat.dct_frames(packed, block), "dct_quant": lambda: nat.dct_quant_frames(packed, block, inputs["types"], mv, 7, 640),
            "dct_quant_luma": lambda: nat.dct_quant_luma_frames(packed, block, 1, bg_step=640)[0],
            "dct_records": lambda: nat.dct_records_frames(packed, block, inputs["types"], mv, 7, 640)}[form]()
    got = call(inputs)
    assert torch.equal(next(iter(got.values())), want)
    if luma is not None:
        pyr, ps = nat.luma_pyramid_frames(packed, 1)
        assert torch.equal(got["level 0"].reshape(n, h * w), torch.stack([pyr[f * ps:f * ps + w * h] for f in range(n)]))
    assert not findings, "\n".join(findings)


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, nat.LAUNCH_BESIDE], ids=["alone", "beside"])
@pytest.mark.parametrize("frames,blocks", [(3, 2049), (5, 8200), (2, 33000)])
def test_ransac_frames(native, frames, blocks, flags):
    """test_ransac_frames_every_launch_shape's fields (integral, fractional and scattered frames), sample indices inside the field."""
    from tests.test_gpu_ransac_pyramid import _field
    subset = 3
    rng = np.random.default_rng(frames * 31 + blocks + subset)
    k = nat.ransac_iter_count(subset_sz=subset)
    mv = np.empty((frames, blocks, 2), np.float32)
    for f in range(frames):
        mv[f] = _field(rng, blocks, 0.05 * (f % 7))
        if f % 3 == 1:
            mv[f] += (rng.random((blocks, 2)) * 0.37).astype(np.float32)
        if f % 5 == 4:
            mv[f] = (rng.random((blocks, 2)) * 1e4).astype(np.float32)
    samples = np.stack([np.stack([rng.choice(blocks, subset, replace=False) for _ in range(k)]) for _ in range(frames)]).astype(np.int32)
    gm_in = _cuda(rng.integers(-3, 4, (frames, 2)).astype(np.float32))
    written = {"gm": gd.Guarded(8 * frames, F32, "cuda", shape=(frames, 2)), "rmse": gd.Guarded(4 * frames, F32, "cuda", seed=1),
               "mask": gd.Guarded(frames * blocks, U8, "cuda", seed=2, shape=(frames, blocks)), "count": gd.Guarded(4 * frames, I32, "cuda", seed=3)}
    out = tuple(written[k_].interior for k_ in ("gm", "rmse", "mask", "count"))

    def call(i):
        out[0].copy_(i["gm_in"])  # the model is input and output
        nat.ransac_frames(i["mv"], i["samples"], subset_sz=subset, out=out, flags=flags)
        return dict(zip(("gm", "rmse", "mask", "count"), out))
    findings = _both(f"ransac_frames {frames}x{blocks} flags {flags}", written, {"mv": _cuda(mv), "samples": _cuda(samples), "gm_in": gm_in}, call)
    assert not findings, "\n".join(findings)


# ---- the decoders of planes and of wire records, and the SSE -----------------------------------------------------------------------------------

@pytest.mark.parametrize("block", [8, 16])
def test_decode_frames_and_sse_frames(native, block):
    w, h, n, mv = 96, 160, 3, 16
    rng = np.random.default_rng(block)
    frames = _cuda(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    types = _cuda(_random_types(block, n, w, h, mv).view(np.int32))
    planes = nat.dct_quant_frames(frames, block, types, mv, 2, 40)
    rec = gd.Guarded(4 * n * h * w * 3, F32, "cuda", shape=(n, h, w, 3))

    def decode(i):
        nat.decode_frames(i["planes"], block, i["types"], mv, 2, 40, gaze=(16, 8, 40, 24), out=rec.interior)
        return {"rec": rec.interior}
    findings = _both(f"decode_frames {block}", {"rec": rec}, {"planes": planes, "types": types}, decode)
    bgr, stride = _strided(frames)
    sse = gd.Guarded(8 * n, I64, "cuda")
    good = rec.interior.clone()

    def measure(i):
        nat._check(nat.load().svc_hip_sse_frames(i["bgr"].data_ptr(), stride, i["rec"].data_ptr(), n, w, h, w - 5, h - 3, sse.interior.data_ptr(),
                                                nat._stream()))
        return {"sse": sse.interior}
    findings += _both(f"sse_frames {block}", {"sse": sse}, {"bgr": bgr, "rec": good}, measure)
    assert torch.equal(measure({"bgr": bgr, "rec": good})["sse"], nat.sse_frames(frames, good, w - 5, h - 3))  # the packed call
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("block", [8, 16])
def test_decode_records_frames(native, block):
    """svc_hip_decode_records_frames takes no workspace; its rec and display are exact."""
    w, h, n, mv = 96, 160, 3, 16
    rng = np.random.default_rng(block + 1)
    frames = _cuda(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    types = _cuda(_random_types(block + 1, n, w, h, mv).view(np.int32))
    records = nat.dct_records_frames(frames, block, types, mv, 2, 40)
    dw, dh = w - 5, h - 3
    written = {"rec": gd.Guarded(4 * n * h * w * 3, F32, "cuda", shape=(n, h, w, 3)),
               "display": gd.Guarded(n * dh * dw * 3, U8, "cuda", seed=1, shape=(n, dh, dw, 3))}
    gaze = _cuda(np.array([(0, 0, 0, 0), (0, 0, w, h), (w - 8, h - 8, 8, 8)], np.int32))

    def call(i):
        nat.decode_records_frames(i["records"], w, h, block, 2, 40, gaze=i["gaze"], display=(dw, dh), rec=written["rec"].interior,
                                  out_display=written["display"].interior)
        return {"rec": written["rec"].interior, "display": written["display"].interior}
    findings = _both(f"decode_records_frames {block}", written, {"records": records, "gaze": gaze}, call)
    assert not findings, "\n".join(findings)
