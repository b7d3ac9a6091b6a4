"""Two layers decoded at reduced size on the GPU (svc_hip_decode_layers_reduced_frames, svc::StreamDecoder::DecodeLayers with
StreamDecoderConfig::reduce): every (N, K) within half an ulp of the long-double inverse of layers.reduced_coefficients, K = 1 bit for
bit; tile by tile the bits of the one-stream reduced decode of the stream encoded at the enhancement's step (inside gaze and window) and
of the base (everywhere else); the residuals outside K x K never read; the display pass on the reduced picture; statuses merged as the
full layered decode merges them, refusals in the stated order; and the C++ driver's display frames equal to the Python path's.

Shapes as tests/test_gpu_decode_reduced.py: 128 x 96 (one partial group at 8 x 8, one exact group at 16 x 16) and 336 x 48 (full groups
plus a partial one at both).  Streams: svc_hip_pack_layers_frames on the raw transform of smooth random frames, a base at (4, 16) and its
enhancement at 1 or 2, for every tile or for a window whose edges fall inside a group; the stream encoded at (e, e) is
svc_hip_pack_levels_frames on the same raw planes, the same quantiser."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers, native, synth
from tests.helpers import transform_ref as tr
from tests.test_gpu_decode_levels import _check_display, _rects
from tests.test_gpu_decode_reduced import _cut

pytestmark = pytest.mark.gpu

SHAPES = [(128, 96, 16), (336, 48, 16), (128, 96, 32)]  # w, h, MV block
NK = [(8, 2), (8, 4), (8, 8), (16, 2), (16, 4), (16, 8)]  # N, reduce
N_FRAMES = 6
# (fg, bg, enh) of the encoder, the decoder's (fg, bg) outside the gaze, the enhancement's window.  The decoder's steps are chosen on the
# numpy statement alone (layers.pack_layers_frames on frames of this distribution): its ambiguous share is 0 and 1.4e-5 at the worst
# (N, K) with these, against the cap of 1e-2; at (1, 640) with enh 2 the few distinct levels cancel to exact zeros in 3 % of the K = 2
# pictures, which the interval counts as ambiguous.
LAYERS = [((4, 16, 1), (3, 17), "cut"), ((4, 16, 2), (2, 24), "every")]


def _window(kind, w, h):
    """None (every tile is enhanced), or per frame a rectangle with its edges inside tiles and inside a group of either tile size."""
    return None if kind == "every" else [(24, 8, w // 2, h - 16)] * N_FRAMES


class Pair:
    """One encode: base and enhancement from svc_hip_pack_layers_frames, and the stream the same planes give at (e, e)."""

    def __init__(self, w, h, block, mv_block, steps, window_kind):
        fg, bg, e = steps
        self.w, self.h, self.block, self.mv_block, self.steps = w, h, block, mv_block, steps
        self.window = _window(window_kind, w, h)
        g = torch.Generator(device="cuda").manual_seed(w + block * 100 + mv_block + e)
        coarse = torch.randint(0, 256, (N_FRAMES, h // 4, w // 4, 3), dtype=torch.uint8, device="cuda", generator=g).float()
        noise = torch.randint(-20, 21, (N_FRAMES, h, w, 3), dtype=torch.int16, device="cuda", generator=g).float()
        bgr = (coarse.repeat_interleave(4, 1).repeat_interleave(4, 2) + noise).clamp(0, 255).to(torch.uint8).contiguous()
        types = torch.randint(0, 3, (N_FRAMES, (w // mv_block) * (h // mv_block)), dtype=torch.int32, device="cuda", generator=g)
        planes = native.dct_frames(bgr, block)
        base, bo, enh, eo = native.pack_layers_frames(planes, types, block, mv_block, fg, bg, e, window=self.window)
        fine, fo = native.pack_levels_frames(planes, types, block, mv_block, e, e)
        torch.cuda.synchronize()
        self.base, self.base_offs = base[:int(bo[-1])].clone(), bo
        self.enh, self.enh_offs = enh[:int(eo[-1])].clone(), eo
        self.fine, self.fine_offs = fine[:int(fo[-1])].clone(), fo
        self.base_frames = self._frames(self.base, bo)
        self.enh_frames = self._frames(self.enh, eo)

    @staticmethod
    def _frames(stream, offs):
        o, host = offs.cpu().tolist(), stream.cpu().numpy()
        return [host[o[i]:o[i + 1]] for i in range(N_FRAMES)]

    def decode(self, reduce, dec, gaze, display=None, base=None, enh=None):
        """svc_hip_decode_layers_reduced_frames into a picture pre-filled with NaN -> (rec, display, status)."""
        base = (self.base, self.base_offs) if base is None else base
        enh = (self.enh, self.enh_offs) if enh is None else enh
        rec = torch.full((N_FRAMES, self.h // reduce, self.w // reduce, 3), float("nan"), dtype=torch.float32, device="cuda")
        return native.decode_layers_reduced_frames(*base, *enh, self.w, self.h, self.block, self.mv_block, *dec, reduce=reduce, gaze=gaze,
                                                   display=display, rec=rec)

    def one_stream(self, which, reduce, dec, gaze, display=None):
        s, o = {"base": (self.base, self.base_offs), "fine": (self.fine, self.fine_offs)}[which]
        return native.decode_levels_reduced_frames(s, o, self.w, self.h, self.block, self.mv_block, *dec, reduce=reduce, gaze=gaze,
                                                   display=display)


_cache = {}


def _pair(w, h, block, mv_block, steps, window_kind) -> Pair:
    key = (w, h, block, mv_block, steps, window_kind)
    if key not in _cache:
        _cache[key] = Pair(*key)
    return _cache[key]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tiles_in(rects, w, h, block, k, default):
    """(n, h k / N, w k / N) bool: is the origin of the reduced pixel's tile, in full-size coordinates, inside its frame's rectangle?"""
    if rects is None:
        return torch.full((N_FRAMES, h // block * k, w // block * k), default, dtype=torch.bool)
    oy = (torch.arange(h // block * k) // k * block)[:, None]
    ox = (torch.arange(w // block * k) // k * block)[None, :]
    return torch.stack([(ox >= x) & (ox < x + ww) & (oy >= y) & (oy < y + hh) for x, y, ww, hh in rects])


def _coefficients(p, reduce, dec, rects):
    return [layers.reduced_coefficients(b, e, reduce, *dec, gaze=r) for b, e, r in zip(p.base_frames, p.enh_frames, rects)]


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("block,reduce", NK)
@pytest.mark.parametrize("steps,dec,window_kind", LAYERS)
def test_rec_is_within_half_an_ulp(native, w, h, mv_block, block, reduce, steps, dec, window_kind):
    if not tr.available():
        pytest.skip(tr.UNAVAILABLE)
    k = block // reduce
    p = _pair(w, h, block, mv_block, steps, window_kind)
    rects = _rects(N_FRAMES, w, h)
    bounds = []
    for coef in _coefficients(p, reduce, dec, rects):
        ref = tr.idct_ref(coef, k, k) if k > 1 else coef.astype(tr.LD)
        bounds.append(tr.interval(ref, tr.inverse_slack(coef, k, k)))
    ambiguous = float(np.mean([np.mean(lo != hi) for lo, hi in bounds]))
    print(f"N={block} K={k} {w}x{h} mv={mv_block} {steps}->{dec} {window_kind}: ambiguous share {ambiguous:.3e}")
    assert ambiguous <= tr.RAW_AMBIGUOUS_CAP  # from the reference alone, before the kernel's output is looked at
    rec, disp, status = p.decode(reduce, dec, rects)
    torch.cuda.synchronize()
    assert disp is None and status.cpu().tolist() == [0] * N_FRAMES
    assert rec.shape == (N_FRAMES, h // reduce, w // reduce, 3) and rec.dtype == torch.float32
    got = rec.cpu().numpy()
    for i, (lo, hi) in enumerate(bounds):
        bad = tr.raw_violations(got[i].transpose(2, 0, 1), lo, hi)
        assert not bad.any(), (i, int(bad.sum()), np.argwhere(bad)[0].tolist())


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("steps,dec,window_kind", LAYERS)
def test_k_one_is_the_mean_bit_for_bit(native, w, h, mv_block, steps, dec, window_kind):
    p = _pair(w, h, 8, mv_block, steps, window_kind)
    rects = _rects(N_FRAMES, w, h)
    rec, _, status = p.decode(8, dec, rects)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * N_FRAMES
    got = rec.cpu().numpy()
    for i, coef in enumerate(_coefficients(p, 8, dec, rects)):
        assert np.array_equal(got[i].transpose(2, 0, 1).view(np.uint32), coef.view(np.uint32)), i


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("block,reduce", NK)
@pytest.mark.parametrize("steps,dec,window_kind", LAYERS)
def test_the_layered_identity_tile_by_tile(native, w, h, mv_block, block, reduce, steps, dec, window_kind):
    """Inside gaze and window the bits of the one-stream reduced decode of the stream encoded at (e, e), everywhere else those of the
    base, both under the same gaze."""
    p = _pair(w, h, block, mv_block, steps, window_kind)
    k = block // reduce
    whole = [(0, 0, w, h)] * N_FRAMES
    seen = 0
    for rects in (_rects(N_FRAMES, w, h), whole):
        rec, _, status = p.decode(reduce, dec, rects)
        a, _, sa = p.one_stream("base", reduce, dec, rects)
        b, _, sb = p.one_stream("fine", reduce, dec, rects)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == sa.cpu().tolist() == sb.cpu().tolist() == [0] * N_FRAMES
        both = _tiles_in(rects, w, h, block, k, False) & _tiles_in(p.window, w, h, block, k, True)
        assert _same_bits(rec, torch.where(both[..., None].cuda(), b, a))
        seen += int(both.sum())
        assert not _same_bits(rec, a)  # the enhancement shows
    assert seen > 0
    # no gaze and no enhancement: the base call, display and status included
    display = (max(1, w // reduce - 7), max(1, h // reduce - 3))
    got = native.decode_layers_reduced_frames(p.base, p.base_offs, None, None, w, h, block, mv_block, *dec, reduce=reduce, display=display)
    want = p.one_stream("base", reduce, dec, None, display)
    # a gaze that holds nothing: the base alone
    empty = [(5, 5, 0, 7)] * N_FRAMES
    rec0, _, st0 = p.decode(reduce, dec, empty)
    want0, _, _ = p.one_stream("base", reduce, dec, empty)
    torch.cuda.synchronize()
    assert _same_bits(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert st0.cpu().tolist() == [0] * N_FRAMES and _same_bits(rec0, want0)


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("block,reduce", NK)
@pytest.mark.parametrize("steps,dec,window_kind", LAYERS)
def test_only_the_low_frequencies_of_both_layers_are_read(native, w, h, mv_block, block, reduce, steps, dec, window_kind):
    """A rank taken from the wrong word, or a residual read outside K x K, shows where high frequencies are present in either layer."""
    p = _pair(w, h, block, mv_block, steps, window_kind)
    k = block // reduce
    low_base, low_enh = _cut(p.base_frames, k), _cut(p.enh_frames, k)
    assert low_base[0].numel() < p.base.numel() and low_enh[0].numel() < p.enh.numel()  # both layers hold levels outside K x K
    rects = _rects(N_FRAMES, w, h)
    display = (max(1, w // reduce - 7), max(1, h // reduce - 3))
    a = p.decode(reduce, dec, rects, display)
    b = p.decode(reduce, dec, rects, display, base=low_base, enh=low_enh)
    band = [(0, 0, k, k)] * N_FRAMES
    bb, bbo, bst = native.band_levels_frames(p.base, p.base_offs, w, h, block, mv_block, band=band)
    be, beo, est = native.band_levels_frames(p.enh, p.enh_offs, w, h, block, mv_block, band=band)
    c = p.decode(reduce, dec, rects, display, base=(bb, bbo), enh=(be, beo))
    torch.cuda.synchronize()
    assert bst.cpu().tolist() == est.cpu().tolist() == [0] * N_FRAMES
    for other in (b, c):
        assert a[2].cpu().tolist() == [0] * N_FRAMES == other[2].cpu().tolist()
        assert _same_bits(a[0], other[0]) and torch.equal(a[1], other[1])


@pytest.mark.parametrize("w,h,mv_block", SHAPES[:2])
@pytest.mark.parametrize("block,reduce", NK)
def test_display_on_the_reduced_picture(native, w, h, mv_block, block, reduce):
    p = _pair(w, h, block, mv_block, (4, 16, 1), "cut")
    rw, rh = w // reduce, h // reduce
    rects = _rects(N_FRAMES, w, h)
    rec, full, st = p.decode(reduce, (1, 3), rects, (rw, rh))
    dw, dh = max(1, rw - 7), max(1, rh - 3)
    rec2, small, _ = p.decode(reduce, (1, 3), rects, (dw, dh))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * N_FRAMES and full.shape == (N_FRAMES, rh, rw, 3) and small.shape == (N_FRAMES, dh, dw, 3)
    assert _same_bits(rec, rec2)
    r = rec.cpu().numpy()
    assert np.array_equal(full.cpu().numpy(), np.clip(np.rint(r), 0, 255).astype(np.uint8))
    for i in range(N_FRAMES):
        _check_display(r[i], small[i].cpu().numpy(), dw, dh)
        _check_display(r[i], full[i].cpu().numpy(), rw, rh)


def _patched(stream, offs, frame, word, value):
    out = stream.clone()
    out[int(offs[frame]):int(offs[frame]) + 64].view(torch.int32)[word] = value
    return out


@pytest.mark.parametrize("block,reduce", [(8, 2), (8, 8), (16, 2), (16, 8)])
def test_statuses(native, block, reduce):
    w, h = 128, 96
    p = _pair(w, h, block, 16, (4, 16, 2), "every")
    n, victim = N_FRAMES, 1
    gaze = [(0, 0, w, h), (8, 0, w, h), (0, 0, 24, h), (0, 0, 0, 0), (16, 8, 40, 24), (0, 0, w, h)]
    disp = (w // reduce, h // reduce)
    good, good_shown, status = p.decode(reduce, (1, 640), gaze, disp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    cases = [
        ("base", 0, 0x12345678, 2),         # a base frame with a bad magic: its own code
        ("enh", 0, 0x12345678, 0x100 | 2),  # an enhancement frame with a bad magic
        ("enh", 9, 4, 0x100 | 11),          # fg_step != bg_step in the enhancement's header
        ("enh", None, 3, 0x100 | 11),       # one step, which does not divide the base's 4 and 16
    ]
    for which, word, value, code in cases:
        base, enh = p.base, p.enh
        if which == "base":
            base = _patched(base, p.base_offs, victim, word, value)
        elif word is None:
            enh = _patched(_patched(enh, p.enh_offs, victim, 8, value), p.enh_offs, victim, 9, value)
        else:
            enh = _patched(enh, p.enh_offs, victim, word, value)
        rec, shown, status = p.decode(reduce, (1, 640), gaze, disp, base=(base, p.base_offs), enh=(enh, p.enh_offs))
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [code if i == victim else 0 for i in range(n)], (which, word)
        assert not rec[victim].view(torch.int32).any() and not shown[victim].any()  # the frame is zeros
        for i in range(n):
            if i != victim:  # its neighbours are unchanged
                assert _same_bits(rec[i], good[i]) and torch.equal(shown[i], good_shown[i]), (which, word, i)


def test_refusals_come_in_the_stated_order(native):
    w, h, block = 128, 96, 8
    p = _pair(w, h, block, 16, (4, 16, 2), "every")
    gaze = [(0, 0, w, h)] * N_FRAMES
    one = torch.empty(native.decode_levels_workspace_bytes(N_FRAMES, w, h, block), dtype=torch.uint8, device="cuda")  # the one-stream size

    def call(reduce, display, workspace):
        return native.decode_layers_reduced_frames(p.base, p.base_offs, p.enh, p.enh_offs, w, h, block, 16, 1, 640, reduce=reduce, gaze=gaze,
                                                   display=display, rec=torch.empty((N_FRAMES, h // 2, w // 2, 3), device="cuda"),
                                                   out_display=torch.empty((N_FRAMES, h, w, 3), dtype=torch.uint8, device="cuda"),
                                                   workspace=workspace)

    for args, word in (((3, (w // 2 + 1, h // 2), one), "reduce"), ((2, (w // 2 + 1, h // 2), one), "display"),
                       ((2, (w // 2, h // 2 + 1), one), "display"), ((2, (w // 2, h // 2), one), "workspace")):
        with pytest.raises(native.SvcError) as e:
            call(*args)
        assert e.value.status == native.SVC_ERR_INVALID_ARG and word in str(e.value), (args[:2], str(e.value))
    assert native.decode_layers_reduced_workspace_bytes(N_FRAMES, w, h, block) == 2 * one.numel()
    _, _, st = call(2, (w // 2, h // 2), torch.empty(2 * one.numel(), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * N_FRAMES


# ---- the driver: svc::StreamDecoder::DecodeLayers with StreamDecoderConfig::reduce, through tests/dropin/stream_layers_reduced_main ----

HERE = os.path.join(os.path.dirname(__file__), "dropin")
CW, CH, CN, CSEED = 96, 64, 11, 7  # the clip of tests/test_gpu_stream_layers.py: its padded size is its size
CSTEPS = (4, 16, 2)
CGAZE = [None if i % 3 == 0 else ((37 * i) % CW, (23 * i) % CH) for i in range(CN - 1)]
CWINDOWS = [None if i % 4 == 0 else (CW - 40, CH - 24, 40, 24) if i % 4 == 3 else (5 * i, 3 * i, 30 + i, 20 + i) for i in range(CN)]


def _exe(name):
    exe = os.path.join(HERE, name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


def _gaze_file(path, centres):
    path.write_text("".join("-\n" if c is None else "%d %d\n" % c for c in centres))
    return path


@pytest.fixture(scope="module")
def stored(native, tmp_path_factory):
    """stream_layers_main's files for 8 x 8 and 16 x 16 tiles, plain and entropy coded -> {(block, entropy): prefix}, the directory."""
    d = tmp_path_factory.mktemp("layers_reduced")
    clip = synth.SynthClip(CW, CH, CN, CSEED, device="cuda")
    torch.stack([clip.frame_bgr(t) for t in range(CN)]).cpu().numpy().tofile(d / "clip.raw")
    (d / "windows.txt").write_text("".join("-\n" if r is None else "%d %d %d %d\n" % r for r in CWINDOWS))
    _gaze_file(d / "gaze.txt", CGAZE)
    out = {}
    for block in (8, 16):
        for coded in (0, 1):
            prefix = str(d / f"run{block}_{coded}")
            r = subprocess.run([_exe("stream_layers_main"), str(d / "clip.raw"), str(CW), str(CH), str(CN), "3", str(block), "3", "4", str(CSEED),
                                *(str(s) for s in CSTEPS), str(coded), str(d / "windows.txt"), str(d / "gaze.txt"), prefix],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            out[(block, coded)] = prefix
    return out, d


def _device_streams(prefix):
    a = (np.fromfile(prefix + ".base", np.uint8), np.fromfile(prefix + ".base.offsets", np.uint64).view(np.int64),
         np.fromfile(prefix + ".enh", np.uint8), np.fromfile(prefix + ".enh.offsets", np.uint64).view(np.int64))
    return [torch.from_numpy(x).cuda() for x in a]


@pytest.mark.parametrize("coded", [0, 1], ids=["svcq", "svce"])
@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("reduce", [2, 4, 8])
def test_cpp_stream_layers_reduced_main_equals_python(native, stored, tmp_path, block, reduce, coded):
    prefixes, _ = stored
    m = CN - 1
    dw, dh = CW // reduce, CH // reduce  # what a display of 0 x 0 means
    centres = [None if i % 5 == 3 else ((37 * i) % dw, (23 * i + 5) % dh) for i in range(m)]
    gaze_file = _gaze_file(tmp_path / "gaze.txt", centres)
    rects = [(0, 0, 0, 0) if c is None else native.gaze_rect(c[0], c[1], 64, 64, dw, dh, CW, CH) for c in centres]
    base, boffs, enh, eoffs = _device_streams(prefixes[(block, 0)])  # the entropy-coded files decode to these
    _, exp, st = native.decode_layers_reduced_frames(base, boffs, enh, eoffs, CW, CH, block, 16, 1, 640, reduce=reduce, gaze=rects,
                                                     display=(dw, dh))
    _, plain, _ = native.decode_levels_reduced_frames(base, boffs, CW, CH, block, 16, 1, 640, reduce=reduce, gaze=rects, display=(dw, dh))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * m and not torch.equal(exp, plain)  # the enhancement shows in what is compared
    exp = exp.cpu().numpy()
    for batch in (3, 4):  # neither divides the 10 frames
        out = str(tmp_path / f"out{batch}")
        r = subprocess.run([_exe("stream_layers_reduced_main"), prefixes[(block, coded)], str(m), str(reduce), "0", "0", str(gaze_file),
                            str(batch), out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.fromfile(out + ".display", np.uint8).reshape(m, dh, dw, 3), exp), batch
        assert np.fromfile(out + ".status", np.uint32).tolist() == [0] * m


@pytest.mark.parametrize("coded", [0, 1], ids=["svcq", "svce"])
def test_cpp_stream_layers_reduced_main_at_reduce_one_smaller_display_and_refusal(native, stored, tmp_path, coded):
    prefixes, d = stored
    m = CN - 1
    prefix = prefixes[(8, coded)]
    out = str(tmp_path / "out")
    # reduce 1: stream_layers_main's own decode of the same files under the same gaze
    r = subprocess.run([_exe("stream_layers_reduced_main"), prefix, str(m), "1", "0", "0", str(d / "gaze.txt"), "3", out], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for ext in (".display", ".status"):
        assert open(out + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    # a display below the reduced picture goes through the display pass
    dw, dh = 41, 29
    centres = [((11 * i) % dw, (7 * i) % dh) for i in range(m)]
    gaze_file = _gaze_file(tmp_path / "gaze.txt", centres)
    rects = [native.gaze_rect(c[0], c[1], 64, 64, dw, dh, CW, CH) for c in centres]
    base, boffs, enh, eoffs = _device_streams(prefixes[(8, 0)])
    _, exp, _ = native.decode_layers_reduced_frames(base, boffs, enh, eoffs, CW, CH, 8, 16, 1, 640, reduce=2, gaze=rects, display=(dw, dh))
    torch.cuda.synchronize()
    r = subprocess.run([_exe("stream_layers_reduced_main"), prefix, str(m), "2", str(dw), str(dh), str(gaze_file), "4", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(out + ".display", np.uint8).reshape(m, dh, dw, 3), exp.cpu().numpy())
    # one above it is refused at the first call
    r = subprocess.run([_exe("stream_layers_reduced_main"), prefix, str(m), "2", str(CW // 2 + 1), str(CH // 2), str(gaze_file), "4", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "display size exceeds the padded frame over reduce" in r.stderr, r.stdout + r.stderr
