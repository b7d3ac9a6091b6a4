"""The decode at reduced size on the GPU (svc_hip_decode_levels_reduced_frames, svc::StreamDecoderConfig::reduce): every (N, K) within
half an ulp of the long-double inverse of levels.reduced_coefficients, K = 1 bit for bit, the coefficients outside K x K never read,
the display pass on the reduced picture, malformed frames reported and zeroed, and the C++ driver's display frames equal to the
Python path's for SVCQ and SVCE input.

Shapes: 128 x 96 and 336 x 48.  A group is 32 tiles at 8 x 8 and 8 tiles at 16 x 16: 128 pixels are one partial group at 8 x 8 and one
exact group at 16 x 16, 336 are full groups plus a partial one at both."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import configs, layers, levels, native, synth
from tests.helpers import transform_ref as tr
from tests.test_gpu_decode_levels import _check_display, _packed, _rects

pytestmark = pytest.mark.gpu

SHAPES = [(128, 96, 16), (336, 48, 16), (128, 96, 32)]  # w, h, MV block
NK = [(8, 2), (8, 4), (8, 8), (16, 2), (16, 4), (16, 8)]  # N, reduce
N_FRAMES = 6

_cache = {}


def _stream(w, h, block, mv_block, enc):
    """_packed once per geometry and encoder steps -> (stream, offsets on the device, the frames' bytes on the host)."""
    key = (w, h, block, mv_block, enc)
    if key not in _cache:
        out, offs, _ = _packed(N_FRAMES, w, h, block, mv_block, *enc, seed=w + block * 100 + mv_block + enc[1])
        o = offs.cpu().tolist()
        host = out.cpu().numpy()
        _cache[key] = (out, offs, [host[o[i]:o[i + 1]] for i in range(N_FRAMES)])
    return _cache[key]


def _coefficients(frames, reduce, dec, rects):
    return [levels.reduced_coefficients(fr, reduce, *dec, gaze=r) for fr, r in zip(frames, rects)]


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("block,reduce", NK)
@pytest.mark.parametrize("enc,dec", [((2, 5), (3, 17)), ((1, 1), (4, 100)), ((1, 1), (1, 1))])
def test_rec_is_within_half_an_ulp(native, w, h, mv_block, block, reduce, enc, dec):
    if not tr.available():
        pytest.skip(tr.UNAVAILABLE)
    k = block // reduce
    out, offs, frames = _stream(w, h, block, mv_block, enc)
    rects = _rects(N_FRAMES, w, h)
    bounds = []
    for coef in _coefficients(frames, reduce, dec, rects):
        ref = tr.idct_ref(coef, k, k) if k > 1 else coef.astype(tr.LD)
        bounds.append(tr.interval(ref, tr.inverse_slack(coef, k, k)))
    ambiguous = float(np.mean([np.mean(lo != hi) for lo, hi in bounds]))
    print(f"N={block} K={k} {w}x{h} mv={mv_block} {enc}->{dec}: ambiguous share {ambiguous:.3e}")
    assert ambiguous <= tr.RAW_AMBIGUOUS_CAP  # from the reference alone, before the kernel's output is looked at
    rec, disp, status = native.decode_levels_reduced_frames(out, offs, w, h, block, mv_block, *dec, reduce=reduce, gaze=rects)
    torch.cuda.synchronize()
    assert disp is None and status.cpu().tolist() == [0] * N_FRAMES
    assert rec.shape == (N_FRAMES, h // reduce, w // reduce, 3) and rec.dtype == torch.float32
    got = rec.cpu().numpy()
    for i, (lo, hi) in enumerate(bounds):
        bad = tr.raw_violations(got[i].transpose(2, 0, 1), lo, hi)
        assert not bad.any(), (i, int(bad.sum()), np.argwhere(bad)[0].tolist())


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("enc,dec", [((1, 640), (1, 640)), ((2, 5), (3, 17))])
def test_k_one_is_the_mean_bit_for_bit(native, w, h, mv_block, enc, dec):
    out, offs, frames = _stream(w, h, 8, mv_block, enc)
    rects = _rects(N_FRAMES, w, h)
    rec, _, status = native.decode_levels_reduced_frames(out, offs, w, h, 8, mv_block, *dec, reduce=8, gaze=rects)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * N_FRAMES
    got = rec.cpu().numpy()
    for i, coef in enumerate(_coefficients(frames, 8, dec, rects)):
        assert np.array_equal(got[i].transpose(2, 0, 1).view(np.uint32), coef.view(np.uint32)), i


def _cut(frames, k):
    """Every frame again with the levels outside the first k x k of every tile set to zero -> (stream, offsets) on the device."""
    cut = []
    for fr in frames:
        hdr, types, planes = levels.parse_frame(fr)
        n, w, h = hdr["block_w"], hdr["frame_w"], hdr["frame_h"]
        oy, ox = (np.arange(h // n) * n)[:, None], (np.arange(w // n) * n)[None, :]
        step = np.where(types[oy // hdr["mv_block_h"], ox // hdr["mv_block_w"]] == 0, hdr["bg_step"], hdr["fg_step"])
        lv = np.rint(planes.astype(np.float64) / np.repeat(np.repeat(step, n, 0), n, 1)[None]).astype(np.int64)
        lv = lv.reshape(3, h // n, n, w // n, n)
        lv[:, :, k:] = 0
        lv[:, :, :, :, k:] = 0
        cut.append(layers.write_frame(hdr, types, lv.reshape(3, h, w), hdr["fg_step"], hdr["bg_step"], hdr["inexact"]))
    offs = np.concatenate([[0], np.cumsum([len(c) for c in cut])]).astype(np.int64)
    return torch.from_numpy(np.frombuffer(b"".join(cut), np.uint8).copy()).cuda(), torch.from_numpy(offs).cuda()


@pytest.mark.parametrize("w,h,mv_block", SHAPES)
@pytest.mark.parametrize("block,reduce", NK)
@pytest.mark.parametrize("steps", [(1, 640), (1, 1)])
def test_the_cut_is_the_cut(native, w, h, mv_block, block, reduce, steps):
    """A rank taken from the wrong word, or a level read outside K x K, shows where high frequencies are present."""
    out, offs, frames = _stream(w, h, block, mv_block, steps)
    low, low_offs = _cut(frames, block // reduce)
    assert low.numel() < out.numel()  # the stream does hold levels outside K x K
    rects = _rects(N_FRAMES, w, h)
    display = (max(1, w // reduce - 7), max(1, h // reduce - 3))
    a = native.decode_levels_reduced_frames(out, offs, w, h, block, mv_block, *steps, reduce=reduce, gaze=rects, display=display)
    b = native.decode_levels_reduced_frames(low, low_offs, w, h, block, mv_block, *steps, reduce=reduce, gaze=rects, display=display)
    torch.cuda.synchronize()
    assert a[2].cpu().tolist() == [0] * N_FRAMES == b[2].cpu().tolist()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("w,h,mv_block", SHAPES[:2])
@pytest.mark.parametrize("block,reduce", NK)
def test_display_on_the_reduced_picture(native, w, h, mv_block, block, reduce):
    out, offs, _ = _stream(w, h, block, mv_block, (1, 1))
    rw, rh = w // reduce, h // reduce
    rects = _rects(N_FRAMES, w, h)
    rec, full, st = native.decode_levels_reduced_frames(out, offs, w, h, block, mv_block, 1, 3, reduce=reduce, gaze=rects, display=(rw, rh))
    dw, dh = max(1, rw - 7), max(1, rh - 3)
    rec2, small, _ = native.decode_levels_reduced_frames(out, offs, w, h, block, mv_block, 1, 3, reduce=reduce, gaze=rects, display=(dw, dh))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * N_FRAMES and full.shape == (N_FRAMES, rh, rw, 3) and small.shape == (N_FRAMES, dh, dw, 3)
    assert torch.equal(rec, rec2)
    r = rec.cpu().numpy()
    assert np.array_equal(full.cpu().numpy(), np.clip(np.rint(r), 0, 255).astype(np.uint8))
    for i in range(N_FRAMES):
        _check_display(r[i], small[i].cpu().numpy(), dw, dh)
        _check_display(r[i], full[i].cpu().numpy(), rw, rh)


@pytest.mark.parametrize("what", ["magic", "level_count", "offsets"])
@pytest.mark.parametrize("block,reduce", [(8, 2), (16, 8)])
def test_malformed_frame_is_reported_and_zeroed(native, what, block, reduce):
    w, h, n = 128, 96, N_FRAMES
    out, offs, _ = _stream(w, h, block, 16, (1, 1))
    rects = _rects(n, w, h)
    display = (w // reduce - 7, h // reduce - 3)

    def run(s, o):
        return native.decode_levels_reduced_frames(s, o, w, h, block, 16, 1, 640, reduce=reduce, gaze=rects, display=display)

    good_rec, good_disp, good_st = run(out, offs)
    torch.cuda.synchronize()
    bad, bad_offs = out.clone(), offs.clone()
    if what == "magic":
        victim = 1
        o = int(offs[victim].item())
        bad[o:o + 4] = 0
    elif what == "level_count":
        victim = 2
        o = int(offs[victim].item())
        cnt = bad[o + 40:o + 44].cpu().numpy().view(np.uint32)[0]
        assert cnt > 0
        bad[o + 40:o + 44] = torch.from_numpy(np.array([cnt - 1], np.uint32).view(np.uint8)).cuda()
    else:  # the last frame's end runs past the stream: only that frame's offsets change
        victim = n - 1
        bad_offs[n] = out.numel() + 16
    rec, disp, status = run(bad, bad_offs)
    _, _, unpack_status = native.unpack_levels_frames(bad, bad_offs, w, h, block, 16)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert good_st.cpu().tolist() == [0] * n
    assert st == unpack_status.cpu().tolist() and st[victim] == {"magic": 2, "level_count": 6, "offsets": 1}[what]
    assert not rec[victim].view(torch.int32).any() and not disp[victim].any()
    for i in range(n):
        if i != victim:
            assert st[i] == 0 and torch.equal(rec[i].view(torch.int32), good_rec[i].view(torch.int32)) and torch.equal(disp[i], good_disp[i]), i


# ---- the driver: svc::StreamDecoder with StreamDecoderConfig::reduce, through tests/dropin/stream_reduced_main ---------------------

HERE = os.path.join(os.path.dirname(__file__), "dropin")
CFG = configs.CodecConfig("decode-main-320x200", 93, 320, 200, 25, levels=3, dct_block=8)


def _exe(name):
    exe = os.path.join(HERE, name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


@pytest.fixture(scope="module")
def stored(native, tmp_path_factory):
    """The stream stream_levels_main writes (the case of test_cpp_stream_decode_main_equals_python) as <prefix>.big / .offsets, and its
    SVCE form beside it -> {"svcq": prefix, "svce": prefix}, the stream and its offsets on the device."""
    d = tmp_path_factory.mktemp("reduced")
    cfg, n = CFG, CFG.frames
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cuda")
    raw = d / "clip.raw"
    torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy().tofile(raw)
    prefix = str(d / "enc")
    r = subprocess.run([_exe("stream_levels_main"), str(raw), str(cfg.width), str(cfg.height), str(n), str(cfg.levels), str(cfg.dct_block),
                        "0", "8", str(cfg.seed), prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    pw, ph = cfg.padded
    assert (pw, ph) == (320, 208)
    big = torch.from_numpy(np.fromfile(prefix + ".big", np.uint8)).cuda()
    offs = torch.from_numpy(np.fromfile(prefix + ".offsets", np.uint64).astype(np.int64)).cuda()
    assert offs.numel() == n
    e, eo, est = native.entropy_encode_frames(big, offs, pw, ph, cfg.dct_block, cfg.mv_block)
    torch.cuda.synchronize()
    assert est.cpu().tolist() == [0] * (n - 1)
    eprefix = str(d / "svce")
    e[:int(eo[-1].item())].cpu().numpy().tofile(eprefix + ".big")
    eo.cpu().numpy().astype(np.uint64).tofile(eprefix + ".offsets")
    return {"svcq": prefix, "svce": eprefix}, big, offs


def _gaze(tmp_path, m, dw, dh):
    centres = [None if i % 5 == 3 else ((37 * i) % dw, (23 * i + 5) % dh) for i in range(m)]
    gaze_file = tmp_path / "gaze.txt"
    gaze_file.write_text("".join("-\n" if c is None else f"{c[0]} {c[1]}\n" for c in centres))
    return centres, gaze_file


@pytest.mark.parametrize("form", ["svcq", "svce"])
@pytest.mark.parametrize("reduce", [2, 4])
def test_cpp_stream_reduced_main_equals_python(native, stored, tmp_path, form, reduce):
    prefixes, big, offs = stored
    cfg, m = CFG, CFG.frames - 1
    pw, ph = cfg.padded
    dw, dh = pw // reduce, ph // reduce  # what a display of 0 x 0 means
    centres, gaze_file = _gaze(tmp_path, m, dw, dh)
    rects = [(0, 0, 0, 0) if c is None else native.gaze_rect(c[0], c[1], 64, 64, dw, dh, pw, ph) for c in centres]
    _, exp, st = native.decode_levels_reduced_frames(big, offs, pw, ph, cfg.dct_block, cfg.mv_block, 1, 640, reduce=reduce, gaze=rects,
                                                     display=(dw, dh))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * m
    exp = exp.cpu().numpy()
    for batch in (1, 7, 16):
        out = tmp_path / f"disp{batch}.raw"
        r = subprocess.run([_exe("stream_reduced_main"), prefixes[form], str(m), str(reduce), "0", "0", str(gaze_file), str(batch), str(out)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, np.uint8).reshape(m, dh, dw, 3)
        assert np.array_equal(got, exp), batch
        assert np.fromfile(str(out) + ".status", np.uint32).tolist() == [0] * m


def test_cpp_stream_reduced_main_smaller_display_and_refusals(native, stored, tmp_path):
    """A display below the reduced picture goes through the display pass; one above it is refused at the first Decode."""
    prefixes, big, offs = stored
    cfg, m = CFG, CFG.frames - 1
    pw, ph = cfg.padded
    dw, dh = 150, 97
    centres, gaze_file = _gaze(tmp_path, m, dw, dh)
    rects = [(0, 0, 0, 0) if c is None else native.gaze_rect(c[0], c[1], 64, 64, dw, dh, pw, ph) for c in centres]
    _, exp, _ = native.decode_levels_reduced_frames(big, offs, pw, ph, cfg.dct_block, cfg.mv_block, 1, 640, reduce=2, gaze=rects,
                                                    display=(dw, dh))
    torch.cuda.synchronize()
    out = tmp_path / "disp.raw"
    r = subprocess.run([_exe("stream_reduced_main"), prefixes["svcq"], str(m), "2", str(dw), str(dh), str(gaze_file), "7", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(m, dh, dw, 3), exp.cpu().numpy())
    r = subprocess.run([_exe("stream_reduced_main"), prefixes["svcq"], str(m), "2", "161", "104", "-", "7", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "display size exceeds" in r.stderr
    r = subprocess.run([_exe("stream_reduced_main"), prefixes["svcq"], str(m), "3", "0", "0", "-", "7", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "invalid configuration" in r.stderr


def test_cpp_stream_reduced_main_at_reduce_one_is_stream_decode_main(native, stored, tmp_path):
    prefixes, _, _ = stored
    cfg, m = CFG, CFG.frames - 1
    dw, dh = cfg.width, cfg.height
    _, gaze_file = _gaze(tmp_path, m, dw, dh)
    a, b = tmp_path / "reduced.raw", tmp_path / "decode.raw"
    r = subprocess.run([_exe("stream_reduced_main"), prefixes["svcq"], str(m), "1", str(dw), str(dh), str(gaze_file), "7", str(a)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([_exe("stream_decode_main"), prefixes["svcq"], str(m), str(dw), str(dh), str(gaze_file), "7", str(b)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(a, np.uint8)
    assert got.size == m * dh * dw * 3 and np.array_equal(got, np.fromfile(b, np.uint8))
    assert np.fromfile(str(a) + ".status", np.uint32).tolist() == [0] * m
