"""svc::StreamDecoder::DecodeDeltaTemporalReduced through tests/dropin/stream_temporal_reduced_main (a caller of
include/svc/stream_decoder.hpp only): a temporal-layer delta stream of 21 frames at periods 2 and 4, as SVCQ with a damaged frame of layer 0
and as SVCE, each as the full stream and as its band (0, 0, K, K), at reduce 2 and 8, in batches of 4 and 16 and at depths 3 and 4.
Whatever the batch size, the display frames and the statuses are those of ONE svc_hip_decode_delta_levels_temporal_reduced_frames call over
the whole stream (tests/test_gpu_decode_delta_temporal_reduced.py pins that call): the carried frame -- the band of the batch's last frame of
layer 0 -- crosses every batch boundary through the driver's two one-frame buffers, and so does a failure on its way down the tree."""
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
EXE = os.path.join(HERE, "stream_temporal_reduced_main")
PLAIN_EXE = os.path.join(HERE, "stream_delta_reduced_main")
GEOM = GEOMS[0]
N = 21  # two batches of 16, six of 4
KEYS = [int(i in (0, 12, 17)) for i in range(N)]
STEPS = (1, 640)  # StreamDecoderConfig's defaults
REDUCES = (2, 8)
PERIODS = (2, 4)
DAMAGED = 4  # a frame of layer 0 at both periods: every frame up to the key frame 12 hangs on it, frame 8 across a boundary of batches of 4


def _size(reduce):
    return GEOM[0] // reduce - 5, GEOM[1] // reduce - 1


@pytest.fixture(scope="module")
def streams(native, tmp_path_factory):
    """The stored streams, their key and gaze files, and what one device call makes of each ->
    {(kind, form, reduce, period): (prefix, display, status)}, kind svcq | svce, form full | band; period 1: the plain delta stream."""
    for exe in (EXE, PLAIN_EXE):
        if not os.path.exists(exe):
            pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    w, h, tile, mv = GEOM
    d = tmp_path_factory.mktemp("temporal_reduced")
    stream, offs = delta_clip(np.random.default_rng(11), GEOM, N, 0.3)
    (d / "key.txt").write_text("".join(f"{k}\n" for k in KEYS))
    out = {}
    for r in REDUCES:
        dw, dh = _size(r)
        k = tile[0] // r
        centres = [None if i % 5 == 3 else ((37 * i) % dw, (5 * i + 2) % dh) for i in range(N)]
        (d / f"gaze{r}.txt").write_text("".join("-\n" if c is None else f"{c[0]} {c[1]}\n" for c in centres))
        rects = [(0, 0, 0, 0) if c is None else nat.gaze_rect(c[0], c[1], 64, 64, dw, dh, w, h) for c in centres]
        for period in (1,) + PERIODS:
            diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, KEYS)
            band, band_offs, _ = _band_call(diff, diff_offs, GEOM, bands=[(0, 0, k, k)] * N)
            forms = {"full": (diff, [int(o) for o in diff_offs]), "band": (band[:band_offs[-1]].tobytes(), band_offs)}
            for form, (plain, plain_offs) in forms.items():
                bad, code = _damaged(plain, plain_offs, DAMAGED, "magic")
                coded, coded_offs, est = nat.entropy_encode_frames(_dev(plain), _offsets(plain_offs), w, h, tile, mv)
                torch.cuda.synchronize()
                assert est.cpu().tolist() == [0] * N
                coded_offs = coded_offs.cpu().numpy()
                for kind, data, o, svcq in (("svcq", bad, np.asarray(plain_offs), bad),
                                            ("svce", coded[:int(coded_offs[-1])].cpu().numpy(), coded_offs, plain)):
                    prefix = str(d / f"{kind}_{form}_{r}_{period}")
                    np.asarray(data, np.uint8).tofile(prefix + ".big")
                    np.asarray(o).astype(np.uint64).tofile(prefix + ".offsets")
                    _, disp, st, _, _ = nat.decode_delta_levels_temporal_reduced_frames(_dev(svcq), _offsets(plain_offs), w, h, tile, mv, period,
                                                                                        *STEPS, r, key=KEYS, gaze=rects, display=(dw, dh))
                    torch.cuda.synchronize()
                    out[kind, form, r, period] = (prefix, disp.cpu().numpy(), st.cpu().tolist())
                want = layers.temporal_statuses([code if i == DAMAGED else 0 for i in range(N)], period, KEYS).tolist()
                assert out["svcq", form, r, period][2] == want and out["svce", form, r, period][2] == [0] * N
                failed = [i for i, c in enumerate(want) if c]
                assert len(failed) >= 3 and out["svce", form, r, period][1].any() and not out["svcq", form, r, period][1][failed].any()
            for kind in ("svcq", "svce"):  # the served band decodes to the frames of the full stream
                assert np.array_equal(out[kind, "band", r, period][1], out[kind, "full", r, period][1])
    return d, out


def _run(d, prefix, size, batch, depth, reduce, period, out, gaze_reduce=None, exe=EXE):
    gaze = d / f"gaze{gaze_reduce or reduce}.txt"
    tail = [str(reduce), str(out)] if exe == PLAIN_EXE else [str(reduce), str(period), str(out)]
    return subprocess.run([exe, prefix, str(N), str(size[0]), str(size[1]), str(gaze), str(d / "key.txt"), str(batch), str(depth)] + tail,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("form", ["full", "band"])
@pytest.mark.parametrize("kind", ["svcq", "svce"])
def test_any_batch_size_gives_the_device_calls_frames(streams, kind, form, reduce, period, depth):
    d, out = streams
    prefix, want, want_status = out[kind, form, reduce, period]
    for batch in (4, 16):
        path = d / f"{kind}_{form}_{reduce}_{period}_{batch}_{depth}.raw"
        r = _run(d, prefix, _size(reduce), batch, depth, reduce, period, path)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(path, np.uint8).reshape(want.shape)
        assert np.fromfile(str(path) + ".status", np.uint32).tolist() == want_status, (batch, depth)
        assert np.array_equal(got, want), (batch, depth)


@pytest.mark.parametrize("reduce", REDUCES)
def test_period_one_is_decode_delta_reduced(streams, reduce):
    d, out = streams
    for kind, form in (("svcq", "band"), ("svce", "full")):
        prefix, want, want_status = out[kind, form, reduce, 1]
        a, b = d / f"p1_{kind}_{reduce}.raw", d / f"p1_plain_{kind}_{reduce}.raw"
        for path, exe in ((a, EXE), (b, PLAIN_EXE)):
            r = _run(d, prefix, _size(reduce), 4, 3, reduce, 1, path, exe=exe)
            assert r.returncode == 0, r.stdout + r.stderr
        assert a.read_bytes() == b.read_bytes() and np.array_equal(np.fromfile(a, np.uint8).reshape(want.shape), want)
        assert np.fromfile(str(a) + ".status", np.uint32).tolist() == np.fromfile(str(b) + ".status", np.uint32).tolist() == want_status
    r = _run(d, out["svcq", "full", reduce, 1][0], _size(reduce), 3, 3, reduce, 1, d / "p1_any_batch.raw")  # any batch size at period 1
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_configured_reduce_may_be_the_argument(streams):
    d, out = streams
    prefix, want, want_status = out["svce", "band", 2, 4]
    path = d / "configured.raw"
    r = _run(d, prefix, _size(2), 4, 3, "2:2", 4, path, gaze_reduce=2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(path, np.uint8).reshape(want.shape), want)
    assert np.fromfile(str(path) + ".status", np.uint32).tolist() == want_status


def test_the_four_refusals(streams):
    """Thrown before any device work: the period, the reduce, another configured reduce, a batch that is no multiple of the period."""
    d, out = streams
    prefix = out["svcq", "full", 2, 2][0]

    def refused(message, batch, reduce, period):
        r = _run(d, prefix, (0, 0), batch, 3, reduce, period, d / "refused.raw", gaze_reduce=2)
        assert r.returncode == 1 and message in r.stderr, r.stdout + r.stderr

    for period in (0, 3, 8):
        refused("DecodeDeltaTemporalReduced takes a period of 1, 2 or 4", 4, 2, period)
        refused("DecodeDeltaTemporalReduced takes a period of 1, 2 or 4", 4, 3, period)  # the period first
    for reduce in ("1", "3", "16"):
        refused("DecodeDeltaTemporalReduced takes a reduce of 2, 4 or 8", 4, reduce, 2)
    for reduce in ("2:4", "8:2", "4:8"):
        refused("config.reduce must be 1 or the argument", 4, reduce, 2)
    for batch, period in ((3, 2), (6, 4), (1, 2)):
        refused("config.batch must be a multiple of the period", batch, 2, period)


def test_a_display_above_the_reduced_picture_is_refused(streams):
    d, out = streams
    w, h = GEOM[:2]
    for size in ((w // 2 + 1, h // 2), (w // 2, h // 2 + 1), (w, h)):
        r = _run(d, out["svcq", "full", 2, 2][0], size, 4, 3, 2, 2, d / "refused.raw")
        assert r.returncode == 1 and "the display size exceeds the padded frame over reduce" in r.stderr, r.stdout + r.stderr
