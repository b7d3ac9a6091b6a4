"""Two layers through the host stream drivers: svc::StreamEncoder with enh_step and svc::StreamDecoder::DecodeLayers, driven through
tests/dropin/stream_layers_main (written against the two public C++ headers only).

An 11-frame 96 x 64 synthetic clip (the padded size is the same), batch 3 and depth 4 -- a short last batch, and more batches than slots.
The encoder's two streams are compared with the device calls on the same frames and region ids, with the numpy statements and with a
second run at another batch size and depth; the decoder's display frames and statuses with svc_hip_decode_layers_frames under the same
rectangles.  A run is made once per command line and shared among the tests that read it.

stream_levels_main takes no quant steps (it encodes at the defaults 1, 640), so where a one-layer stream at other steps is compared, the
two calls its route makes (svc_hip_dct_quant_frames, svc_hip_pack_levels_frames) are made here on the run's region ids."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from scalable_video_codec_amd import synth

pytestmark = pytest.mark.gpu

W, H, N, LEVELS, SEED = 96, 64, 11, 3, 7
MV = 16
STEPS = [(2, 640, 1), (4, 16, 2)]
BLOCKS = [8, 16]
# per clip frame (frame 0 is tracked only): a moving rectangle, none, one that touches the right and bottom edges
WINDOWS = [None if i % 4 == 0 else (W - 40, H - 24, 40, 24) if i % 4 == 3 else (5 * i, 3 * i, 30 + i, 20 + i) for i in range(N)]
GAZE = [None if i % 3 == 0 else ((37 * i) % W, (23 * i) % H) for i in range(N - 1)]  # per encoded frame, as stream_decode_main

_runs = {}


def _exe(name):
    exe = os.path.join(os.path.dirname(__file__), "dropin", name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_layers")
    clip = synth.SynthClip(W, H, N, SEED, device="cuda")
    frames = torch.stack([clip.frame_bgr(t) for t in range(N)]).contiguous()
    frames.cpu().numpy().tofile(d / "clip.raw")
    (d / "windows.txt").write_text("".join("-\n" if r is None else "%d %d %d %d\n" % r for r in WINDOWS))
    (d / "gaze.txt").write_text("".join("-\n" if g is None else "%d %d\n" % g for g in GAZE))
    return d, frames


def _layers_main(work, block, steps, entropy_=0, batch=3, depth=4, windows=True, gaze=True, budget=None, check=True):
    """One run of stream_layers_main per command line -> (its output prefix, the finished process)."""
    d, _ = work
    key = (str(block), steps, entropy_, batch, depth, windows, gaze, budget)
    if key not in _runs:
        prefix = str(d / ("run%d" % len(_runs)))
        cmd = [_exe("stream_layers_main"), str(d / "clip.raw"), str(W), str(H), str(N), str(LEVELS), str(block), str(batch), str(depth),
               str(SEED), *(str(s) for s in steps), str(entropy_), str(d / "windows.txt") if windows else "-",
               str(d / "gaze.txt") if gaze else "-", prefix] + ([str(budget)] if budget else [])
        _runs[key] = (prefix, subprocess.run(cmd, capture_output=True, text=True, timeout=300))
    prefix, r = _runs[key]
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return prefix, r


def _streams(prefix):
    return (np.fromfile(prefix + ".base", np.uint8), np.fromfile(prefix + ".base.offsets", np.uint64),
            np.fromfile(prefix + ".enh", np.uint8), np.fromfile(prefix + ".enh.offsets", np.uint64))


def _types(prefix):
    return torch.from_numpy(np.fromfile(prefix + ".types", np.uint32).view(np.int32).reshape(N - 1, -1)).cuda()


def _host(t, offs):
    torch.cuda.synchronize()
    offs = offs.cpu().numpy().astype(np.uint64)
    return t[:int(offs[-1])].cpu().numpy(), offs


def _rects(windows):
    return [(0, 0, 0, 0) if r is None else r for r in windows]


def _without_inexact(stream, offs):
    out = np.array(stream, copy=True)
    for o in offs[:-1]:
        out[int(o) + 44:int(o) + 48] = 0
    return out.tobytes()


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", STEPS, ids=str)
@pytest.mark.parametrize("block", BLOCKS)
def test_encoder_streams(native, work, block, steps):
    fg, bg, e = steps
    prefix, _ = _layers_main(work, block, steps)
    base, boffs, enh, eoffs = _streams(prefix)
    assert boffs.size == eoffs.size == N and boffs[-1] == base.size and eoffs[-1] == enh.size
    frames, types = work[1][1:], _types(prefix)
    windows = _rects(WINDOWS[1:])
    # both streams are the device call's on the transform of the same frames, with the region ids the run wrote
    planes = nat.dct_frames(frames, block)
    wb, wbo, we, weo = nat.pack_layers_frames(planes, types, block, MV, fg, bg, e, window=windows)
    (wb, wbo), (we, weo) = _host(wb, wbo), _host(we, weo)
    assert np.array_equal(boffs, wbo) and np.array_equal(base, wb)
    assert np.array_equal(eoffs, weo) and np.array_equal(enh, we)
    # the enhancement is the numpy statement's, from the run's base and the one-layer stream at (e, e)
    fine, fine_offs = _host(*nat.pack_levels_frames(nat.dct_quant_frames(frames, block, types, MV, e, e), types, block, MV, e, e))
    want_enh, want_eoffs = layers.enhancement_frames(base, boffs, fine, fine_offs, e, windows)
    assert enh.tobytes() == want_enh and np.array_equal(eoffs, want_eoffs)
    # the base is the one-layer stream at (fg, bg), except the inexact count
    one, one_offs = _host(*nat.pack_levels_frames(nat.dct_quant_frames(frames, block, types, MV, fg, bg), types, block, MV, fg, bg))
    assert np.array_equal(boffs, one_offs) and _without_inexact(base, boffs) == _without_inexact(one, one_offs)
    assert any(base[int(o) + 44:int(o) + 48].any() for o in boffs[:-1]) and not any(one[int(o) + 44:int(o) + 48].any() for o in one_offs[:-1])
    # batch size and depth change no byte, of the streams or of the side outputs
    other, _ = _layers_main(work, block, steps, batch=16, depth=3)
    for ext in (".base", ".base.offsets", ".enh", ".enh.offsets", ".types", ".mv", ".gm", ".display", ".status"):
        assert open(prefix + ext, "rb").read() == open(other + ext, "rb").read(), ext


def test_one_layer_at_the_default_steps_is_stream_levels_mains(native, work):
    """At (1, 640) stream_levels_main's own stream is the base, except the inexact count; and its region ids are the run's."""
    d, _ = work
    prefix, _ = _layers_main(work, 8, (1, 640, 1))
    pq = str(d / "levels")
    r = subprocess.run([_exe("stream_levels_main"), str(d / "clip.raw"), str(W), str(H), str(N), str(LEVELS), "8", "0", "3", str(SEED), pq],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    base, boffs, _, _ = _streams(prefix)
    one, one_offs = np.fromfile(pq + ".big", np.uint8), np.fromfile(pq + ".offsets", np.uint64)
    assert np.array_equal(boffs, one_offs) and _without_inexact(base, boffs) == _without_inexact(one, one_offs)
    for ext in (".types", ".mv", ".gm"):
        assert open(prefix + ext, "rb").read() == open(pq + ext, "rb").read(), ext


@pytest.mark.parametrize("steps", STEPS, ids=str)
@pytest.mark.parametrize("block", BLOCKS)
def test_entropy_coded_streams_decode_to_the_plain_ones(native, work, block, steps):
    plain, _ = _layers_main(work, block, steps)
    coded, _ = _layers_main(work, block, steps, entropy_=1)
    base, boffs, enh, eoffs = _streams(plain)
    cb, cbo, ce, ceo = _streams(coded)
    assert cb[:4].tobytes() == b"SVCE" and ce[:4].tobytes() == b"SVCE"
    back, back_offs = entropy.decode_frames(cb, cbo)
    assert back == base.tobytes() and np.array_equal(back_offs, boffs)
    back, back_offs = entropy.decode_frames(ce, ceo)
    assert back == enh.tobytes() and np.array_equal(back_offs, eoffs)
    for ext in (".types", ".mv", ".gm", ".display", ".status"):  # and DecodeLayers shows the same through either kind
        assert open(plain + ext, "rb").read() == open(coded + ext, "rb").read(), ext


def test_without_a_window_file_every_tile_is_enhanced(native, work):
    steps = (4, 16, 2)
    prefix, _ = _layers_main(work, 8, steps, windows=False)
    base, boffs, enh, eoffs = _streams(prefix)
    wb, wbo, we, weo = nat.pack_layers_frames(nat.dct_frames(work[1][1:], 8), _types(prefix), 8, MV, *steps, window=None)
    (wb, wbo), (we, weo) = _host(wb, wbo), _host(we, weo)
    assert np.array_equal(base, wb) and np.array_equal(boffs, wbo) and np.array_equal(enh, we) and np.array_equal(eoffs, weo)
    windowed, _ = _layers_main(work, 8, steps)
    assert open(prefix + ".base", "rb").read() == open(windowed + ".base", "rb").read()
    assert enh.size > np.fromfile(windowed + ".enh", np.uint8).size


# ---- the decoder ----------------------------------------------------------------------------------------------------------------------------

def _gaze_rects():
    return [(0, 0, 0, 0) if g is None else nat.gaze_rect(g[0], g[1], 64, 64, W, H, W, H) for g in GAZE]


def _decode(prefix, block):
    base, boffs, enh, eoffs = (torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in _streams(prefix))
    _, disp, st = nat.decode_layers_frames(base, boffs, enh, eoffs, W, H, block, MV, 1, 640, gaze=_gaze_rects(), display=(W, H))
    torch.cuda.synchronize()
    return disp.cpu().numpy().reshape(-1), st.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("steps", STEPS, ids=str)
@pytest.mark.parametrize("block", BLOCKS)
def test_decode_layers_is_the_device_calls(native, work, block, steps):
    prefix, _ = _layers_main(work, block, steps)
    disp, st = _decode(prefix, block)
    assert disp.size == (N - 1) * W * H * 3
    assert np.array_equal(np.fromfile(prefix + ".display", np.uint8), disp)
    assert np.array_equal(np.fromfile(prefix + ".status", np.uint32), st) and not st.any()


def test_no_gaze_is_stream_decode_main_on_the_base(native, work, tmp_path):
    prefix, _ = _layers_main(work, 8, (4, 16, 2), gaze=False)
    pq = str(tmp_path / "base")
    np.fromfile(prefix + ".base", np.uint8).tofile(pq + ".big")
    np.fromfile(prefix + ".base.offsets", np.uint64).tofile(pq + ".offsets")
    out = str(tmp_path / "disp")
    r = subprocess.run([_exe("stream_decode_main"), pq, str(N - 1), "0", "0", "-", "3", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(prefix + ".display", np.uint8), np.fromfile(out, np.uint8))
    assert np.array_equal(np.fromfile(prefix + ".status", np.uint32), np.fromfile(out + ".status", np.uint32))
    gazed, _ = _layers_main(work, 8, (4, 16, 2))
    assert not np.array_equal(np.fromfile(prefix + ".display", np.uint8), np.fromfile(gazed + ".display", np.uint8))  # the gaze shows


@pytest.mark.parametrize("entropy_", [0, 1])
def test_a_corrupt_enhancement_frame_is_reported_and_leaves_its_neighbours(native, work, tmp_path, entropy_):
    """Frame 4's magic overwritten in the enhancement file, decoded by stream_layers_main's decode mode: SVCQ -- the device call's
    0x100 | 2; SVCE -- the entropy decoder's code 2 for it, merged by the driver."""
    d, _ = work
    prefix, _ = _layers_main(work, 8, (4, 16, 2), entropy_=entropy_)
    base, boffs, enh, eoffs = _streams(prefix)
    bad = 4
    enh = enh.copy()
    enh[int(eoffs[bad]):int(eoffs[bad]) + 4] = np.frombuffer(b"XXXX", np.uint8)
    pc = str(tmp_path / "corrupt")
    for ext, a in ((".base", base), (".base.offsets", boffs), (".enh", enh), (".enh.offsets", eoffs)):
        a.tofile(pc + ext)
    out = str(tmp_path / "out")
    r = subprocess.run([_exe("stream_layers_main"), "decode", pc, str(N - 1), "3", "4", str(d / "gaze.txt"), out], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = np.fromfile(out + ".status", np.uint32)
    assert st[bad] == (0x100 | 2) and not np.delete(st, bad).any()
    got = np.fromfile(out + ".display", np.uint8).reshape(N - 1, -1)
    want = np.fromfile(prefix + ".display", np.uint8).reshape(N - 1, -1)
    assert not got[bad].any() and np.array_equal(np.delete(got, bad, 0), np.delete(want, bad, 0))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_a_non_square_tile_encodes_and_decode_layers_refuses_it(native, work):
    steps = (4, 16, 2)
    prefix, r = _layers_main(work, "8x4", steps, check=False)
    assert r.returncode == 1 and "transform block 8x4" in r.stderr, r.stdout + r.stderr  # the C ABI's message, from DecodeLayers
    base, boffs, enh, eoffs = _streams(prefix)  # written before the decode
    types = np.fromfile(prefix + ".types", np.uint32).reshape(N - 1, H // MV, W // MV)
    planes = nat.dct_frames(work[1][1:], (8, 4))
    torch.cuda.synchronize()
    geom = {"frame_w": W, "frame_h": H, "block_w": 8, "block_h": 4, "mv_block_w": MV, "mv_block_h": MV}
    want = layers.pack_layers_frames(planes.cpu().numpy(), types, geom, *steps, _rects(WINDOWS[1:]))
    assert base.tobytes() == want[0] and np.array_equal(boffs, want[1]) and enh.tobytes() == want[2] and np.array_equal(eoffs, want[3])


def test_configurations_the_encoder_refuses(native, work):
    _, r = _layers_main(work, 8, (4, 16, 2), budget=200000, check=False)
    assert r.returncode == 1 and "a byte budget counts one stream" in r.stderr, r.stdout + r.stderr
    _, r = _layers_main(work, 8, (4, 6, 4), check=False)
    assert r.returncode == 1 and "must each be a multiple of enh_step" in r.stderr, r.stdout + r.stderr
