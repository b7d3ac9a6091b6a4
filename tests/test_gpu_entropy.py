"""The entropy-coded compact stream on the GPU (csrc/entropy.hip): the encoder writes the bytes of the numpy coder
(scalable_video_codec_amd/entropy.py) for GPU-packed SVCQ frames, the decoder gives those SVCQ frames back byte for byte, decoding
through SVCE changes no reconstructed pixel, corrupt frames get their status and zeros without touching their neighbours, the
host-memory encoder's coded output is its compact output, and the coded C3 clip is several times smaller."""
import dataclasses

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import configs, entropy, levels, native, stream, synth
from tests.test_entropy_host import _sparse
from tests.test_levels_host import write_frames

pytestmark = pytest.mark.gpu


def _dct_packed(n, w, h, block, mv, fg, bg, seed):
    """Random-content frames through the GPU transform, quantiser and pack -> (SVCQ u8, offsets i64) on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    # smooth the noise so levels are sparse, as in real content
    bgr = torch.nn.functional.avg_pool2d(bgr.permute(0, 3, 1, 2).float(), 9, 1, 4).round().to(torch.uint8).permute(0, 2, 3, 1)
    blocks = (w // mv) * (h // mv)
    types = torch.randint(0, 3, (n, blocks), dtype=torch.int32, device="cuda", generator=g)
    planes = native.dct_quant_frames(bgr.contiguous(), block, types, mv, fg, bg)
    out, offs = native.pack_levels_frames(planes, types, block, mv, fg, bg)
    return out, offs


def _host_packed(n, w, h, bw, bh, mb, fg, bg, seed, kind="random"):
    planes, types = _sparse(np.random.default_rng(seed), n, w, h, bw, bh, mb, fg, bg, kind)
    out, offs = native.pack_levels_frames(torch.from_numpy(planes).cuda(), torch.from_numpy(types.view(np.int32)).cuda(),
                                          (bw, bh), mb, fg, bg)
    exp, exp_offs = write_frames(planes, types, bw, bh, mb[0], mb[1], fg, bg)
    used = int(offs[-1])
    assert out[:used].cpu().numpy().tobytes() == exp and np.array_equal(offs.cpu().numpy().astype(np.uint64), exp_offs)
    return out, offs


def _check_codec(svcq, offs, w, h, block, mv):
    """GPU encode == numpy encode; GPU decode == the SVCQ frames.  Returns the device SVCE stream and offsets."""
    used = int(offs[-1])
    q_host = svcq[:used].cpu().numpy()
    q_offs = offs.cpu().numpy().astype(np.uint64)
    exp, exp_offs = entropy.encode_frames(q_host, q_offs)
    e, eo, st = native.entropy_encode_frames(svcq, offs, w, h, block, mv)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(eo.cpu().numpy().astype(np.uint64), exp_offs)
    assert e[:int(eo[-1])].cpu().numpy().tobytes() == exp
    d, do, ds = native.entropy_decode_frames(e, eo, w, h, block, mv)
    torch.cuda.synchronize()
    assert (ds.cpu().numpy() == 0).all()
    assert np.array_equal(do.cpu().numpy(), offs.cpu().numpy())
    assert d[:used].cpu().numpy().tobytes() == q_host.tobytes()
    return e, eo


@pytest.mark.parametrize("block", [(8, 8), (16, 16), (8, 16), (4, 4)])
@pytest.mark.parametrize("fg,bg", [(1, 640), (3, 17)])
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_coder_matches_numpy_on_gpu_packed_frames(native, block, fg, bg, n):
    w, h = 256, 160
    _check_codec(*_dct_packed(n, w, h, block, 16, fg, bg, seed=n * 7 + fg), w, h, block, (16, 16))


@pytest.mark.parametrize("w,h,bw,bh,mb", [(66, 48, 6, 6, (6, 6)), (128, 64, 64, 64, (64, 64)), (33 * 8, 16, 8, 8, (8, 8))])
@pytest.mark.parametrize("kind", ["random", "background", "foreground"])
def test_gpu_coder_odd_tiles_and_short_chunks(native, w, h, bw, bh, mb, kind):
    out, offs = _host_packed(3, w, h, bw, bh, mb, 1, 640, seed=w + bw, kind=kind)
    _check_codec(out, offs, w, h, (bw, bh), mb)


def test_gpu_coder_types_near_two_to_the_32_and_dense_levels(native):
    w, h, bw, bh, mb = 64, 48, 8, 8, (16, 16)
    rng = np.random.default_rng(4)
    planes = (rng.integers(-40, 41, (3, 3, h, w)) * (rng.random((3, 3, h, w)) < 0.6)).astype(np.float32) * 3
    types = (0xFFFFFFFF - rng.integers(0, 3, (3, 12))).astype(np.uint32)
    types[1, ::2] = 0
    out, offs = native.pack_levels_frames(torch.from_numpy(planes).cuda(), torch.from_numpy(types.view(np.int32)).cuda(), (bw, bh),
                                          mb, 3, 3)
    _check_codec(out, offs, w, h, (bw, bh), mb)


def test_gpu_coder_white_noise_is_raw_and_within_the_worst_case(native):
    w, h, bw, bh, mb = 64, 32, 8, 8, (16, 16)
    rng = np.random.default_rng(8)
    planes = rng.integers(-30000, 30000, (2, 3, h, w)).astype(np.float32)
    types = np.ones((2, 8), np.int32)
    out, offs = native.pack_levels_frames(torch.from_numpy(planes).cuda(), torch.from_numpy(types).cuda(), (bw, bh), mb, 1, 1)
    e, eo = _check_codec(out, offs, w, h, (bw, bh), mb)
    assert int(eo[-1]) <= native.entropy_max_bytes(2, w, h, (bw, bh), mb)


def test_gpu_coder_padded_1080p(native):
    w, h = 1920, 1088
    _check_codec(*_dct_packed(1, w, h, (8, 8), 16, 1, 640, seed=3), w, h, (8, 8), (16, 16))


@pytest.mark.parametrize("block", [8, 16])
def test_decoding_through_svce_changes_no_pixel(native, block):
    w, h, n = 256, 160, 4
    svcq, offs = _dct_packed(n, w, h, (block, block), 16, 2, 40, seed=block)
    e, eo, _ = native.entropy_encode_frames(svcq, offs, w, h, block, 16)
    d, do, _ = native.entropy_decode_frames(e, eo, w, h, block, 16)
    gaze = [[0, 0, 64, 48], [32, 16, 100, 80], [0, 0, 0, 0], [128, 96, 128, 64]]
    r0, d0, s0 = native.decode_levels_frames(svcq, offs, w, h, block, 16, fg_step=1, bg_step=16, gaze=gaze, display=(200, 120))
    r1, d1, s1 = native.decode_levels_frames(d, do, w, h, block, 16, fg_step=1, bg_step=16, gaze=gaze, display=(200, 120))
    torch.cuda.synchronize()
    assert (s0.cpu() == 0).all() and (s1.cpu() == 0).all()
    assert torch.equal(r0, r1) and torch.equal(d0, d1)


def _corrupt_cases(good: bytes):
    """(name, frame bytes, expected status) for one SVCE frame; every frame keeps its size (offsets stay valid)."""
    def word(b, i):
        return int.from_bytes(b[4 * i:4 * i + 4], "little")

    def put(b, i, v):
        b[4 * i:4 * i + 4] = int(v).to_bytes(4, "little")

    cases = []
    b = bytearray(good); put(b, 0, levels.MAGIC); cases.append(("magic", b, 2))
    b = bytearray(good); put(b, 1, 9); cases.append(("version", b, 3))
    b = bytearray(good); put(b, 2, word(b, 2) + 16); cases.append(("geometry", b, 4))
    b = bytearray(good); put(b, 12, word(b, 12) + 16); cases.append(("frame_bytes", b, 5))
    b = bytearray(good); put(b, 13, word(b, 13) + 16); cases.append(("svcq_frame_bytes", b, 10))
    ix = 64 + word(good, 15)
    b = bytearray(good); put(b, ix // 4, word(b, ix // 4) + 300); cases.append(("index overruns", b, 8))
    b = bytearray(good); put(b, ix // 4, word(b, ix // 4) + (1 << 16)); cases.append(("index levels", b, 8))
    b = bytearray(good); e0, e1 = word(b, ix // 4), word(b, ix // 4 + 1)
    put(b, ix // 4, e0 - 1); put(b, ix // 4 + 1, e1 + 1); cases.append(("chunk past its end", b, 9))
    return cases


def test_corrupt_frame_in_a_batch_gets_its_status_and_zeros(native):
    w, h, block, mv = 128, 64, (8, 8), (16, 16)
    svcq, offs = _dct_packed(5, w, h, block, 16, 1, 40, seed=21)
    used = int(offs[-1])
    q_host, q_offs = svcq[:used].cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
    svce, eoffs = entropy.encode_frames(q_host, q_offs)
    frames = [svce[int(a):int(b)] for a, b in zip(eoffs[:-1], eoffs[1:])]
    for name, bad, code in _corrupt_cases(frames[2]):
        with pytest.raises(ValueError):
            entropy.decode_frame(bytes(bad))
        batch = b"".join(frames[:2] + [bytes(bad)] + frames[3:])
        t = torch.from_numpy(np.frombuffer(batch, np.uint8).copy()).cuda()
        d, do, st = native.entropy_decode_frames(t, torch.from_numpy(eoffs.astype(np.int64)).cuda(), w, h, block, mv)
        torch.cuda.synchronize()
        st, do = st.cpu().numpy(), do.cpu().numpy()
        assert list(st) == [0, 0, code, 0, 0], name
        dh = d.cpu().numpy()
        for f in (0, 1, 3, 4):
            got = dh[do[f]:do[f + 1]].tobytes()
            assert got == q_host[q_offs[f]:q_offs[f + 1]].tobytes(), (name, f)
        assert not dh[do[2]:do[3]].any() and do[3] - do[2] in (64, int(q_offs[3] - q_offs[2])), name


def test_encoder_flags_a_malformed_svcq_frame(native):
    w, h, block, mv = 128, 64, (8, 8), (16, 16)
    svcq, offs = _dct_packed(3, w, h, block, 16, 1, 40, seed=5)
    host = svcq.cpu().numpy().copy()
    o1 = int(offs[1])
    host[o1 + 4 * 10:o1 + 4 * 11] = np.frombuffer((int.from_bytes(host[o1 + 40:o1 + 44].tobytes(), "little") + 1).to_bytes(4, "little"),
                                                   np.uint8)
    e, eo, st = native.entropy_encode_frames(torch.from_numpy(host).cuda(), offs, w, h, block, mv)
    torch.cuda.synchronize()
    st = list(st.cpu().numpy())
    assert st[0] == 0 and st[2] == 0 and st[1] in (5, 6)  # the exact size, or the masks' popcount
    eo = eo.cpu().numpy()
    assert eo[2] - eo[1] == 64 and not e[int(eo[1]):int(eo[2])].cpu().numpy().any()
    d, _ = entropy.decode_frames(e[:int(eo[-1])].cpu().numpy()[np.r_[0:eo[1], eo[2]:eo[3]]],
                                 np.array([0, eo[1], eo[1] + eo[3] - eo[2]], np.uint64))
    q = svcq.cpu().numpy()
    assert d == q[:int(offs[1])].tobytes() + q[int(offs[2]):int(offs[3])].tobytes()


def _small_cfg():
    return configs.CodecConfig("entropy-320x208", 90, 320, 208, 40, levels=3, dct_block=8)


def test_host_stream_encoder_entropy_equals_compact(native):
    cfg = _small_cfg()
    n = 25
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cuda")
    host = torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy()
    dev = torch.device("cuda")
    ref = {}
    for out in stream.HostStreamEncoder(cfg, batch=8, device=dev, compact=True).encode(host):
        ref[out["first"]] = (out["compact"].tobytes(), out["compact_offsets"].copy())
    seen = 0
    for out in stream.HostStreamEncoder(cfg, batch=8, device=dev, compact=True, entropy=True).encode(host):
        q, qo = entropy.decode_frames(out["compact"], out["compact_offsets"])
        assert int(out["compact_offsets"][-1]) == out["compact"].size
        assert (q, list(qo)) == (ref[out["first"]][0], list(ref[out["first"]][1]))
        seen += len(qo) - 1
    assert seen == n - 1
    with pytest.raises(ValueError):
        stream.HostStreamEncoder(cfg, batch=8, device=dev, compact=True, entropy=True, compact_budget=10000,
                                 compact_ladder=[(1, 640)])
    with pytest.raises(ValueError):
        stream.HostStreamEncoder(cfg, batch=8, device=dev, entropy=True)


@pytest.mark.parametrize("fg,bg,limit", [(1, 640, 1 / 8), (16, 16, 1 / 2)])
def test_c3_clip_codes_several_times_smaller(native, fg, bg, limit):
    cfg = dataclasses.replace(configs.C3, fg_step=fg, bg_step=bg)
    n = 17
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cuda")
    host = torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy()
    dev = torch.device("cuda")
    q = [o["compact"].size for o in stream.HostStreamEncoder(cfg, batch=16, device=dev, compact=True).encode(host)]
    e = [o["compact"].size for o in stream.HostStreamEncoder(cfg, batch=16, device=dev, compact=True, entropy=True).encode(host)]
    ratio = sum(e) / sum(q)
    print(f"C3 steps ({fg}, {bg}): SVCQ {sum(q) / (n - 1) / 1e6:.3f} MB/frame, SVCE {sum(e) / (n - 1) / 1e6:.4f} MB/frame, "
          f"1/{1 / ratio:.1f}")
    assert ratio <= limit, ratio


def test_gpu_coder_padded_1080p_batch_of_five(native):
    w, h = 1920, 1088
    _check_codec(*_dct_packed(5, w, h, (8, 8), 16, 1, 640, seed=11), w, h, (8, 8), (16, 16))


@pytest.mark.parametrize("ct", [1, 7, 37, 0xFFFFFFFF])
def test_gpu_decoder_honours_any_chunk_tiles(native, ct):
    """Frames the numpy coder writes with other chunk_tiles than the GPU encoder's (1, odd, above tiles_x, 2^32 - 1)."""
    w, h, block, mv = 256, 160, (8, 8), (16, 16)
    svcq, offs = _dct_packed(3, w, h, block, 16, 1, 40, seed=ct % 97)
    used = int(offs[-1])
    q_host, q_offs = svcq[:used].cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
    svce, eoffs = entropy.encode_frames(q_host, q_offs, chunk_tiles=ct)
    assert entropy.parse_frame(svce)[0]["chunk_tiles"] == ct
    t = torch.from_numpy(np.frombuffer(svce, np.uint8).copy()).cuda()
    d, do, st = native.entropy_decode_frames(t, torch.from_numpy(eoffs.astype(np.int64)).cuda(), w, h, block, mv)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == [0, 0, 0]
    assert np.array_equal(do.cpu().numpy().astype(np.uint64), q_offs)
    assert d[:used].cpu().numpy().tobytes() == q_host.tobytes()


def test_crafted_frames_get_status_8_and_zeros(native):
    """The chunk_tiles that would wrap tiles_x + chunk_tiles - 1 in 32 bits, and a width-32 region id that would decode to 2^32, in
    the middle of a batch of good frames."""
    from tests.test_entropy_host import overflowing_chunk_tiles_frame, width_32_type_overflow_frame
    w, h, block, mv = 64, 48, (8, 8), (16, 16)
    rng = np.random.default_rng(1)
    planes, types = _sparse(rng, 2, w, h, 8, 8, mv, 1, 640)
    q, qo = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    good = [entropy.encode_frame(q[int(a):int(b)]) for a, b in zip(qo[:-1], qo[1:])]
    for bad in (overflowing_chunk_tiles_frame(), width_32_type_overflow_frame()):
        frames = [good[0], bad, good[1]]
        offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
        out = torch.full((native.levels_max_bytes(3, w, h, block, mv),), 0xCD, dtype=torch.uint8, device="cuda")
        t = torch.from_numpy(np.frombuffer(b"".join(frames), np.uint8).copy()).cuda()
        d, do, st = native.entropy_decode_frames(t, torch.from_numpy(offs).cuda(), w, h, block, mv, out=out)
        torch.cuda.synchronize()
        assert list(st.cpu().numpy()) == [0, 8, 0]
        dh, do = d.cpu().numpy(), do.cpu().numpy()
        assert do[2] - do[1] == 64 and not dh[do[1]:do[2]].any()
        assert dh[do[0]:do[1]].tobytes() == q[int(qo[0]):int(qo[1])] and dh[do[2]:do[3]].tobytes() == q[int(qo[1]):int(qo[2])]


# ---- the C++ drivers: svc::StreamEncoderConfig::entropy and svc::StreamDecoder on SVCE -----------------------------------------------

def _exe(name):
    import os
    exe = os.path.join(os.path.dirname(__file__), "dropin", name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


def test_cpp_stream_entropy_main_equals_the_compact_stream_and_its_decode(native, tmp_path):
    import subprocess
    cfg = _small_cfg()
    n = 40
    clip = synth.SynthClip(cfg.width, cfg.height, n, cfg.seed, device="cuda")
    raw = tmp_path / "clip.raw"
    torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy().tofile(raw)
    pw, ph = cfg.padded
    gaze = tmp_path / "gaze.txt"
    gaze.write_text("".join("-\n" if i % 3 == 0 else f"{(37 * i) % cfg.width} {(23 * i) % cfg.height}\n" for i in range(n - 1)))
    pq, pe = str(tmp_path / "levels"), str(tmp_path / "entropy")
    common = [str(raw), str(cfg.width), str(cfg.height), str(n), str(cfg.levels), str(cfg.dct_block)]
    r = subprocess.run([_exe("stream_levels_main"), *common, "0", "8", str(cfg.seed), pq], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([_exe("stream_entropy_main"), *common, "8", str(cfg.seed), str(gaze), pe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for ext in (".mv", ".types", ".gm"):
        assert open(pq + ext, "rb").read() == open(pe + ext, "rb").read(), ext
    # the SVCE stream is the SVCQ stream, coded
    q, qo = np.fromfile(pq + ".big", np.uint8).tobytes(), np.fromfile(pq + ".offsets", np.uint64)
    e, eo = np.fromfile(pe + ".big", np.uint8), np.fromfile(pe + ".offsets", np.uint64)
    back, bo = entropy.decode_frames(e, eo)
    assert back == q and np.array_equal(bo, qo) and e.size < len(q) / 2
    # svc::StreamDecoder on SVCE gives the display frames and statuses it gives on the SVCQ stream
    out_q = str(tmp_path / "disp_q")
    r = subprocess.run([_exe("stream_decode_main"), pq, str(n - 1), "0", "0", str(gaze), "8", out_q], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    disp_q = np.fromfile(out_q, np.uint8)
    assert disp_q.size == (n - 1) * pw * ph * 3
    assert np.array_equal(np.fromfile(pe + ".display", np.uint8), disp_q)
    assert np.array_equal(np.fromfile(pe + ".status", np.uint32), np.fromfile(out_q + ".status", np.uint32))
    assert not np.fromfile(pe + ".status", np.uint32).any()
    # a corrupt SVCE frame in the middle: its status and zeros through svc::StreamDecoder, the others unchanged
    frames = [e[int(a):int(b)].tobytes() for a, b in zip(eo[:-1], eo[1:])]
    bad = bytearray(frames[10])
    ix = 64 + int.from_bytes(bad[60:64], "little")
    bad[ix:ix + 4] = (int.from_bytes(bad[ix:ix + 4], "little") + 300).to_bytes(4, "little")
    frames[10] = bytes(bad)
    pc = str(tmp_path / "corrupt")
    np.frombuffer(b"".join(frames), np.uint8).tofile(pc + ".big")
    eo.tofile(pc + ".offsets")
    out_c = str(tmp_path / "disp_c")
    r = subprocess.run([_exe("stream_decode_main"), pc, str(n - 1), "0", "0", str(gaze), "8", out_c], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = np.fromfile(out_c + ".status", np.uint32)
    assert st[10] == 8 and not np.delete(st, 10).any()
    dc = np.fromfile(out_c, np.uint8).reshape(n - 1, -1)
    dq = disp_q.reshape(n - 1, -1)
    assert not dc[10].any() and np.array_equal(np.delete(dc, 10, 0), np.delete(dq, 10, 0))
    # entropy with a byte budget is refused at construction
    r = subprocess.run([_exe("stream_entropy_main"), *common, "8", str(cfg.seed), "-", "-", "200000"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "budget" in r.stderr, r.stdout + r.stderr


def test_cpp_one_decoder_at_depth_4_across_svcq_wire_and_svce(native, tmp_path):
    """svc::StreamDecoder's slot ring beyond the default depth, its regrow path and the switch between Decode's and DecodeWire's
    buffers: one decoder (depth 4, batch 2, wire_batch 3) decodes the SVCQ, the wire, the SVCE and again the SVCQ stream of a clip
    (stream_entropy_main reuse: 10 encoded frames of 96 x 64 from an encoder at batch 3, depth 4), and gives every time, display
    bytes and frame statuses, what a fresh default decoder gives for that stream -- which test_cpp_stream_decode_main_equals_python
    and tests/test_gpu_decode_records.py pin to the Python statement."""
    import subprocess
    w, h, n = 96, 64, 11
    clip = synth.SynthClip(w, h, n, 7, device="cuda")
    raw = tmp_path / "clip.raw"
    torch.stack([clip.frame_bgr(t) for t in range(n)]).cpu().numpy().tofile(raw)
    prefix = str(tmp_path / "reuse")
    r = subprocess.run([_exe("stream_entropy_main"), "reuse", str(raw), "7", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def out(name, k):
        return (np.fromfile(f"{prefix}.{name}{k}.display", np.uint8), np.fromfile(f"{prefix}.{name}{k}.status", np.uint32))

    for k, kind in enumerate(["SVCQ", "wire", "SVCE", "SVCQ again"]):  # the order the one decoder saw them in
        (disp, status), (fresh_disp, fresh_status) = out("reuse", k), out("fresh", k)
        assert disp.size == (n - 1) * w * h * 3 and status.size == n - 1, kind
        assert np.array_equal(disp, fresh_disp) and np.array_equal(status, fresh_status), kind
        assert not status.any(), kind
    for a, b in ((0, 3), (0, 2)):  # the same stream twice; and the coding is lossless
        assert np.array_equal(out("reuse", a)[0], out("reuse", b)[0]) and np.array_equal(out("reuse", a)[1], out("reuse", b)[1])
    for ext in (".mv", ".types"):  # one clip, one seed: the three encodings tracked and segmented it alike
        q = open(f"{prefix}.q{ext}", "rb").read()
        assert len(q) > 0 and q == open(f"{prefix}.e{ext}", "rb").read() == open(f"{prefix}.w{ext}", "rb").read(), ext
