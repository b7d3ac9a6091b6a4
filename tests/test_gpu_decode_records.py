"""The decoder of the reference's wire stream on the GPU (svc_hip_decode_records_frames, svc::StreamDecoder::DecodeWire,
tests/dropin/wire_decode_main): the reconstruction is bit-identical to the numpy parse of the stream followed by svc_hip_decode_frames
with mv_block = block and each frame's own gaze rectangle, agrees with the oracle and with the compact stream's decoder on the same
quantised planes, reads the reference encoder's unpadded emission, really scales with gaze, and the C++ application's display frames
equal the Python path's -- for streams of HostStreamEncoder(wire=True) and of the reference's unchanged encoder."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import configs, native, stream, synth, wire

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")


def _bgr(n, w, h, seed):
    """Smooth-ish random frames on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randint(0, 256, (n, h // 4, w // 4, 3), dtype=torch.uint8, device="cuda", generator=g).float()
    noise = torch.randint(-20, 21, (n, h, w, 3), dtype=torch.int16, device="cuda", generator=g).float()
    return (base.repeat_interleave(4, 1).repeat_interleave(4, 2) + noise).clamp(0, 255).to(torch.uint8).contiguous()


def _header(n, w, h, block, excess_w=0, excess_h=0):
    return struct.pack("<8I", n, w - excess_w, h - excess_h, excess_w, excess_h, block, block, 3)


def _raw_records(n, w, h, block, seed, emit_h=None):
    """Raw-coefficient records of random frames with random per-tile type words (values above 1 included) -> (records on the device,
    the whole stream as bytes)."""
    bgr = _bgr(n, w, h, seed)
    types0 = torch.zeros((n, (w // block) * (h // block)), dtype=torch.int32, device="cuda")
    rec = native.dct_records_frames(bgr, block, types0, block, emit_h=emit_h)
    words = rec.view(torch.int32).view(n, -1, 1 + 3 * block * block)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    tw = torch.randint(0, 4, words[..., 0].shape, dtype=torch.int32, device="cuda", generator=g)
    tw = torch.where(tw == 3, torch.full_like(tw, 0x7FFFFFF3), tw)  # 0 background, 1, 2 and a large id foreground
    words[..., 0] = tw
    torch.cuda.synchronize()
    eh = h if emit_h is None else emit_h
    return rec, _header(n, w, h, block, 0, h - eh) + rec.cpu().numpy().tobytes()


def _rects(n, w, h):
    cycle = [(0, 0, 0, 0), (0, 0, w, h), (16, 8, 40, 24), (w // 2, h // 3, w, h), (8, 16, 0, 32), (w - 8, h - 8, 8, 8)]
    return [cycle[i % len(cycle)] for i in range(n)]


def _chain(stream_bytes, block, fg, bg, rects):
    """The numpy parse, then svc_hip_decode_frames frame by frame with mv_block = block (the MV-block types are the tiles' words)."""
    _, _, types, planes = wire.read_stream(stream_bytes)
    n = planes.shape[0]
    t = torch.from_numpy(types.reshape(n, -1).view(np.int32)).cuda()
    p = torch.from_numpy(planes).cuda()
    out = torch.cat([native.decode_frames(p[i:i + 1], block, t[i:i + 1], block, fg, bg, gaze=r) for i, r in enumerate(rects)])
    torch.cuda.synchronize()
    return out, types, planes


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("dec", [(1, 640), (3, 17), (2, 5)])
def test_rec_is_bit_identical_to_parse_then_decode(native, block, dec):
    n, w, h = 6, 128, 96
    records, big = _raw_records(n, w, h, block, seed=block * 10 + dec[1])
    rects = _rects(n, w, h)
    rec, disp = native.decode_records_frames(records, w, h, block, *dec, gaze=rects)
    exp, types, _ = _chain(big, block, *dec, rects)
    assert disp is None and (types > 2).any() and (types == 0).any()
    for i in range(n):
        assert torch.equal(rec[i], exp[i]), i
    # no gaze at all is the rectangle of size 0 everywhere
    rec0, _ = native.decode_records_frames(records, w, h, block, *dec)
    exp0, _, _ = _chain(big, block, *dec, [(0, 0, 0, 0)] * n)
    assert torch.equal(rec0, exp0)


@pytest.mark.parametrize("block", [8, 16])
def test_rec_matches_the_oracle(native, oracle, block):
    n, w, h = 3, 64, 64
    records, big = _raw_records(n, w, h, block, seed=7 + block)
    rects = [(0, 0, 0, 0), (16, 16, 32, 16), (0, 0, w, h)]
    rec, _ = native.decode_records_frames(records, w, h, block, 3, 17, gaze=rects)
    _, _, types, planes = wire.read_stream(big)
    torch.cuda.synchronize()
    for i in range(n):
        ref = oracle.decode_frame(planes[i], block, types[i].reshape(-1), block, 3, 17, rects[i])
        got = rec[i].cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))), i


@pytest.mark.parametrize("block,mv_block", [(8, 16), (16, 32)])
def test_quantised_records_decode_as_the_compact_stream(native, block, mv_block):
    """Records of quantised planes and the pack of the same planes carry the same numbers: with the same decoder steps and rectangles
    both decoders give the same rec and display, bit for bit."""
    n, w, h = 6, 320, 224  # MV blocks of 32 divide the frame
    bgr = _bgr(n, w, h, seed=block + mv_block)
    g = torch.Generator(device="cuda").manual_seed(5)
    types = torch.randint(0, 3, (n, (w // mv_block) * (h // mv_block)), dtype=torch.int32, device="cuda", generator=g)
    enc = (2, 5)
    records = native.dct_records_frames(bgr, block, types, mv_block, *enc)
    planes = native.dct_quant_frames(bgr, block, types, mv_block, *enc)
    packed, offs = native.pack_levels_frames(planes, types, block, mv_block, *enc)
    rects = _rects(n, w, h)
    for dec in [(1, 640), (3, 17)]:
        rec_r, disp_r = native.decode_records_frames(records, w, h, block, *dec, gaze=rects, display=(300, 200))
        rec_l, disp_l, st = native.decode_levels_frames(packed, offs, w, h, block, mv_block, *dec, gaze=rects, display=(300, 200))
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n
        assert torch.equal(rec_r, rec_l) and torch.equal(disp_r, disp_l), dec


@pytest.mark.parametrize("block,h,emit_h", [(8, 208, 200), (16, 1088, 1080), (8, 96, 8)])
def test_encoders_reading_rows_present_and_absent(native, block, h, emit_h):
    """Records emitted for the unpadded height (what apps/encoder.cpp writes): the rows the stream holds decode as the full stream's,
    the rows it does not hold are zeros."""
    n, w = 3, 320
    bgr = _bgr(n, w, h, seed=h)
    types = torch.zeros((n, (w // block) * (h // block)), dtype=torch.int32, device="cuda")
    full = native.dct_records_frames(bgr, block, types, block)
    part = native.dct_records_frames(bgr, block, types, block, emit_h=emit_h)
    rects = _rects(n, w, h)
    rec_f, _ = native.decode_records_frames(full, w, h, block, 1, 640, gaze=rects)
    rec_p, _ = native.decode_records_frames(part, w, h, block, 1, 640, gaze=rects, emit_h=emit_h)
    rows = -(-emit_h // block) * block
    torch.cuda.synchronize()
    assert torch.equal(rec_p[:, :rows], rec_f[:, :rows])
    assert not rec_p[:, rows:].any()
    # the numpy reader takes the stream the same way
    big = _header(n, w, h, block, 0, h - emit_h) + part.cpu().numpy().tobytes()
    same = native.serialized_frame_bytes(w, emit_h, block, block) == native.serialized_frame_bytes(w, h, block, block)
    assert native.wire_layout(big[:32], len(big)) == (h if same else emit_h, part.shape[1])  # a tie goes to the decoder's reading
    exp, _, _ = _chain(big, block, 1, 640, rects)
    assert torch.equal(rec_p, exp)


def _psnr(sse, count):
    return 10 * np.log10(255.0 ** 2 * count / max(sse, 1e-9))


@pytest.mark.parametrize("block", [8, 16])
def test_gaze_actually_scales(native, block):
    """Raw records of a smooth synthetic clip.  At fg 1 / bg 640 (every tile background) the tiles inside the gaze rectangle are
    decoded at step 1 and the rest at 640: PSNR inside is far above PSNR outside.  At step 1 everywhere the reconstruction is the source
    up to the rounding of every coefficient to an integer: |error| <= 1/2 per coefficient, so by Parseval (the transform is
    orthonormal) the mean squared error of a tile is <= 1/4, and per pixel |error| <= 1/2 * (sum_k |c_k(n)|)^2 <= N / 2 (Cauchy-Schwarz
    on a basis column of unit norm); both with 1e-3 of slack for the f32 coefficients and the f32 result."""
    n, w, h = 4, 320, 208
    clip = synth.SynthClip(w, h, n, seed=0x6A2E, device="cuda")
    src = torch.stack([clip.frame_bgr(t) for t in range(n)]).contiguous()
    types = torch.zeros((n, (w // block) * (h // block)), dtype=torch.int32, device="cuda")
    records = native.dct_records_frames(src, block, types, block)
    x, y, rw, rh = 96, 64, 96, 80  # whole tiles: every tile whose origin lies inside is gazed
    rec, _ = native.decode_records_frames(records, w, h, block, 1, 640, gaze=[(x, y, rw, rh)] * n)
    crop_s = src[:, y:y + rh, x:x + rw].contiguous()
    crop_r = rec[:, y:y + rh, x:x + rw].contiguous()
    sse_in = native.sse_frames(crop_s, crop_r, rw, rh).cpu().numpy()
    sse_all = native.sse_frames(src, rec, w, h).cpu().numpy()
    for i in range(n):
        p_in = _psnr(sse_in[i], rw * rh * 3)
        p_out = _psnr(sse_all[i] - sse_in[i], (w * h - rw * rh) * 3)
        assert p_in > 45 and p_in > p_out + 15, (i, p_in, p_out)
    rec1, _ = native.decode_records_frames(records, w, h, block, 1, 1)
    err = rec1.double() - src.double()
    torch.cuda.synchronize()
    assert err.abs().max().item() <= block / 2 + 1e-3
    tiles = err.reshape(n, h // block, block, w // block, block, 3).pow(2).mean(dim=(2, 4))
    assert tiles.max().item() <= 0.25 + 1e-3


def test_full_c3_batch(native):
    cfg = configs.C3
    pw, ph = cfg.padded
    n = 16
    records, big = _raw_records(n, pw, ph, cfg.dct_block, seed=1080)
    rects = [native.gaze_rect(100 + 110 * i, 60 + 60 * i, 64, 64, cfg.width, cfg.height, pw, ph) if i % 4 else (0, 0, 0, 0)
             for i in range(n)]
    rec, disp = native.decode_records_frames(records, pw, ph, cfg.dct_block, 1, 640, gaze=rects, display=(cfg.width, cfg.height))
    exp, _, _ = _chain(big, cfg.dct_block, 1, 640, rects)
    assert torch.equal(rec, exp)
    assert disp.shape == (n, cfg.height, cfg.width, 3)


def _run_decoder(stream_bytes, gaze_file, out, *args):
    exe = os.path.join(BIN, "wire_decode_main")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    r = subprocess.run([exe, "--gaze", str(gaze_file), "--out", str(out), *args], input=stream_bytes, capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"frames/s" in r.stdout


def _gaze(tmp_path, m, dw, dh, pw, ph, max_w=64, max_h=64):
    centres = [None if i % 5 == 3 else ((37 * i + 11) % dw, (23 * i + 5) % dh) for i in range(m)]
    path = tmp_path / "gaze.txt"
    path.write_text("".join("-\n" if c is None else f"{c[0]} {c[1]}\n" for c in centres))
    rects = [(0, 0, 0, 0) if c is None else native.gaze_rect(c[0], c[1], max_w, max_h, dw, dh, pw, ph) for c in centres]
    return path, rects


def test_cpp_wire_decode_main_equals_python(native, tmp_path):
    cfg = configs.CodecConfig("wire-decode-320x200", 94, 320, 200, 13, levels=3, dct_block=8)
    n = cfg.frames
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cuda")
    host = torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy()
    header, chunks = b"", []
    for o in stream.HostStreamEncoder(cfg, batch=4, device=torch.device("cuda"), wire=True).encode(host):
        header = o.get("header", header)
        chunks.append(o["records"].tobytes())  # a copy: the view is only valid until the next batch is yielded
    big = header + b"".join(chunks)
    pw, ph = cfg.padded
    m = n - 1
    dw, dh = cfg.width, cfg.height  # the header's source size: what the reference shows
    gaze_file, rects = _gaze(tmp_path, m, dw, dh, pw, ph, 48, 80)
    hdr, records, _, _ = wire.read_stream(big)
    assert hdr["frame_count"] == m and native.wire_layout(big[:32], len(big)) == (ph, records.shape[1])
    _, exp = native.decode_records_frames(torch.from_numpy(records.copy()).cuda(), pw, ph, 8, 2, 300, gaze=rects, display=(dw, dh))
    exp = exp.cpu().numpy()
    for batch in (1, 5, 16):
        out = tmp_path / f"disp{batch}.raw"
        _run_decoder(big, gaze_file, out, "--batch", str(batch), "--foreground-quant-step", "2", "--background-quant-step", "300",
                     "--max-gaze-rect-w", "48", "--max-gaze-rect-h", "80")
        got = np.fromfile(out, np.uint8).reshape(m, dh, dw, 3)
        assert np.array_equal(got, exp), batch


def test_reference_encoder_into_wire_decode_main(native, tmp_path):
    """The reference's unchanged encoder application (GPU path) piped into the decoder at 320 x 200: the encoder's unpadded loops
    emit 25 tile rows where the padded 320 x 208 grid has 26, so only the encoder's reading parses the stream."""
    exe = os.path.join(BIN, "ref_encoder_sse2")
    if not os.path.exists(exe):
        pytest.skip("ref_encoder_sse2 not built (needs /root/reference at build time)")
    n, w, h = 5, 320, 200
    clip = synth.SynthClip(w, h, n, seed=0x3E2)
    path = tmp_path / "clip.svcbgr"
    with open(path, "wb") as f:
        f.write(b"SVCBGR1\0" + struct.pack("<4I", w, h, n, 0))
        for t in range(n):
            f.write(np.ascontiguousarray(clip.frame_bgr(t).numpy(), np.uint8).tobytes())
    r = subprocess.run([exe, "--verbose", "0", str(path)], capture_output=True, env=dict(os.environ, SVC_TEST_RANSAC_SEED="777"),
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    big = r.stdout
    hdr, records, _, _ = wire.read_stream(big)
    pw, ph = w + hdr["frame_excess_w"], h + hdr["frame_excess_h"]
    assert (pw, ph) == (320, 208) and records.shape == (n - 1, 40 * 25 * 772)
    assert native.wire_layout(big[:32], len(big)) == (200, records.shape[1])
    gaze_file, rects = _gaze(tmp_path, n - 1, w, h, pw, ph)
    _, exp = native.decode_records_frames(torch.from_numpy(records.copy()).cuda(), pw, ph, 8, 1, 640, gaze=rects, display=(w, h),
                                          emit_h=200)
    out = tmp_path / "disp.raw"
    _run_decoder(big, gaze_file, out)
    got = np.fromfile(out, np.uint8).reshape(n - 1, h, w, 3)
    assert np.array_equal(got, exp.cpu().numpy())
