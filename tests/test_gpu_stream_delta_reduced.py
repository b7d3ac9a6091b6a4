"""svc::StreamDecoder::DecodeDeltaReduced through tests/dropin/stream_delta_reduced_main (a caller of include/svc/stream_decoder.hpp only):
a delta stream of 11 frames, as SVCQ with a damaged frame and as SVCE, each as the full delta stream and as its band (0, 0, K, K), at reduce
2 and 8, in batches of 1, 4 and 16 and at depths 3 and 4.  Whatever the batch size, the display frames and the statuses are those of ONE
svc_hip_decode_delta_levels_reduced_frames call over the whole stream (tests/test_gpu_decode_delta_reduced.py pins that call): the chain
crosses every batch boundary through the driver's two one-frame buffers, which hold band frames here, and so does a failure on its way to
the next key frame."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_delta_levels_host import delta_clip
from tests.test_gpu_band_levels import _band_call, _damaged, _offsets
from tests.test_gpu_decode_delta import GEOMS
from tests.test_gpu_window_levels import _dev

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(__file__), "dropin")
EXE = os.path.join(HERE, "stream_delta_reduced_main")
GEOM = GEOMS[0]
N = 11
KEYS = [int(i in (0, 7)) for i in range(N)]
STEPS = (1, 640)  # StreamDecoderConfig's defaults
REDUCES = (2, 8)


def _size(reduce):
    return GEOM[0] // reduce - 5, GEOM[1] // reduce - 1


@pytest.fixture(scope="module")
def streams(native, tmp_path_factory):
    """The stored streams, their key and gaze files, and what one device call makes of each ->
    {(kind, form, reduce): (prefix, display, status)}, kind svcq | svce, form full | band."""
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} is not built (python -m scalable_video_codec_amd.build)")
    w, h, tile, mv = GEOM
    d = tmp_path_factory.mktemp("delta_reduced")
    stream, offs = delta_clip(np.random.default_rng(11), GEOM, N, 0.3)
    diff, diff_offs = layers.delta_frames(stream, offs, KEYS)
    (d / "key.txt").write_text("".join(f"{k}\n" for k in KEYS))
    out = {}
    for r in REDUCES:
        dw, dh = _size(r)
        k = tile[0] // r
        centres = [None if i % 5 == 3 else ((37 * i) % dw, (5 * i + 2) % dh) for i in range(N)]
        (d / f"gaze{r}.txt").write_text("".join("-\n" if c is None else f"{c[0]} {c[1]}\n" for c in centres))
        rects = [(0, 0, 0, 0) if c is None else nat.gaze_rect(c[0], c[1], 64, 64, dw, dh, w, h) for c in centres]
        band, band_offs, _ = _band_call(diff, diff_offs, GEOM, bands=[(0, 0, k, k)] * N)
        forms = {"full": (diff, [int(o) for o in diff_offs]), "band": (band[:band_offs[-1]].tobytes(), band_offs)}
        for form, (plain, plain_offs) in forms.items():
            bad, code = _damaged(plain, plain_offs, 4, "magic")
            coded, coded_offs, est = nat.entropy_encode_frames(_dev(plain), _offsets(plain_offs), w, h, tile, mv)
            torch.cuda.synchronize()
            assert est.cpu().tolist() == [0] * N
            coded_offs = coded_offs.cpu().numpy()
            for kind, data, o, svcq in (("svcq", bad, np.asarray(plain_offs), bad),
                                        ("svce", coded[:int(coded_offs[-1])].cpu().numpy(), coded_offs, plain)):
                prefix = str(d / f"{kind}_{form}_{r}")
                np.asarray(data, np.uint8).tofile(prefix + ".big")
                np.asarray(o).astype(np.uint64).tofile(prefix + ".offsets")
                _, disp, st, _, _ = nat.decode_delta_levels_reduced_frames(_dev(svcq), _offsets(plain_offs), w, h, tile, mv, *STEPS, r, key=KEYS,
                                                                           gaze=rects, display=(dw, dh))
                torch.cuda.synchronize()
                out[kind, form, r] = (prefix, disp.cpu().numpy(), st.cpu().tolist())
            assert out["svcq", form, r][2] == [0, 0, 0, 0, code, 0x100 | code, 0x100 | code, 0, 0, 0, 0] and out["svce", form, r][2] == [0] * N
            assert out["svce", form, r][1].any() and not out["svcq", form, r][1][4:7].any()
        for kind in ("svcq", "svce"):  # the served band decodes to the frames of the full stream
            assert np.array_equal(out[kind, "band", r][1], out[kind, "full", r][1])
    return d, out


def _run(d, prefix, size, batch, depth, reduce, out, gaze_reduce=None):
    gaze = d / f"gaze{gaze_reduce or reduce}.txt"
    return subprocess.run([EXE, prefix, str(N), str(size[0]), str(size[1]), str(gaze), str(d / "key.txt"), str(batch), str(depth),
                           str(reduce), str(out)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("form", ["full", "band"])
@pytest.mark.parametrize("kind", ["svcq", "svce"])
def test_any_batch_size_gives_the_device_calls_frames(streams, kind, form, reduce, depth):
    d, out = streams
    prefix, want, want_status = out[kind, form, reduce]
    for batch in (1, 4, 16):
        path = d / f"{kind}_{form}_{reduce}_{batch}_{depth}.raw"
        r = _run(d, prefix, _size(reduce), batch, depth, reduce, path)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(path, np.uint8).reshape(want.shape)
        assert np.fromfile(str(path) + ".status", np.uint32).tolist() == want_status, (batch, depth)
        assert np.array_equal(got, want), (batch, depth)


def test_the_configured_reduce_may_be_the_argument(streams):
    d, out = streams
    prefix, want, want_status = out["svce", "band", 2]
    path = d / "configured.raw"
    r = _run(d, prefix, _size(2), 4, 3, "2:2", path, gaze_reduce=2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(path, np.uint8).reshape(want.shape), want)
    assert np.fromfile(str(path) + ".status", np.uint32).tolist() == want_status


def test_a_display_above_the_reduced_picture_is_refused(streams):
    d, out = streams
    w, h = GEOM[:2]
    for size in ((w // 2 + 1, h // 2), (w // 2, h // 2 + 1), (w, h)):
        r = _run(d, out["svcq", "full", 2][0], size, 4, 3, 2, d / "refused.raw")
        assert r.returncode == 1 and "the display size exceeds the padded frame over reduce" in r.stderr, r.stdout + r.stderr


def test_another_configured_reduce_is_refused(streams):
    d, out = streams
    for arg in ("2:4", "8:2", "4:8"):
        r = _run(d, out["svcq", "full", 2][0], (0, 0), 4, 3, arg, d / "refused.raw", gaze_reduce=2)
        assert r.returncode == 1 and "config.reduce must be 1 or the argument" in r.stderr, r.stdout + r.stderr
    for arg in ("1", "3", "16"):  # the argument itself
        r = _run(d, out["svcq", "full", 2][0], (0, 0), 4, 3, arg, d / "refused.raw", gaze_reduce=2)
        assert r.returncode == 1 and "takes a reduce of 2, 4 or 8" in r.stderr, r.stdout + r.stderr
