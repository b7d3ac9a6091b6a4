"""svc::StreamDecoder::DecodeDelta through tests/dropin/stream_delta_main (a caller of include/svc/stream_decoder.hpp only): a delta
stream of 11 frames, as SVCQ and as SVCE, in batches of 1, 4 and 16 and at depths 3 and 4.  Whatever the batch size, the display frames and
the statuses are those of ONE svc_hip_decode_delta_levels_frames call over the whole stream (tests/test_gpu_decode_delta.py pins that call):
the chain crosses every batch boundary through the driver's two one-frame buffers.  The SVCQ stream holds a damaged frame, so a failure
runs across batch boundaries to the next key frame as well."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_delta_levels_host import delta_clip
from tests.test_gpu_band_levels import _damaged, _offsets
from tests.test_gpu_decode_delta import GEOMS
from tests.test_gpu_window_levels import _dev

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(__file__), "dropin")
EXE = os.path.join(HERE, "stream_delta_main")
GEOM = GEOMS[0]
N = 11
KEYS = [int(i in (0, 7)) for i in range(N)]
STEPS = (1, 640)  # StreamDecoderConfig's defaults


@pytest.fixture(scope="module")
def streams(native, tmp_path_factory):
    """The two stored streams, their key and gaze files, and what one device call makes of each -> {kind: (prefix, display, status)}."""
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} is not built (python -m scalable_video_codec_amd.build)")
    w, h, tile, mv = GEOM
    d = tmp_path_factory.mktemp("delta")
    dw, dh = w - 5, h - 3
    stream, offs = delta_clip(np.random.default_rng(11), GEOM, N, 0.3)
    diff, diff_offs = layers.delta_frames(stream, offs, KEYS)
    centres = [None if i % 5 == 3 else ((37 * i) % dw, (5 * i + 2) % dh) for i in range(N)]
    (d / "gaze.txt").write_text("".join("-\n" if c is None else f"{c[0]} {c[1]}\n" for c in centres))
    (d / "key.txt").write_text("".join(f"{k}\n" for k in KEYS))
    rects = [(0, 0, 0, 0) if c is None else nat.gaze_rect(c[0], c[1], 64, 64, dw, dh, w, h) for c in centres]
    bad, code = _damaged(diff, diff_offs, 4, "magic")
    coded, coded_offs, est = nat.entropy_encode_frames(_dev(diff), _offsets(diff_offs), w, h, tile, mv)
    torch.cuda.synchronize()
    assert est.cpu().tolist() == [0] * N
    coded_offs = coded_offs.cpu().numpy()
    out = {}
    for kind, data, o, plain in (("svcq", bad, np.asarray(diff_offs), bad), ("svce", coded[:int(coded_offs[-1])].cpu().numpy(), coded_offs, diff)):
        prefix = str(d / kind)
        np.asarray(data, np.uint8).tofile(prefix + ".big")
        np.asarray(o).astype(np.uint64).tofile(prefix + ".offsets")
        _, disp, st, _, _ = nat.decode_delta_levels_frames(_dev(plain), _offsets(diff_offs), w, h, tile, mv, *STEPS, key=KEYS, gaze=rects,
                                                           display=(dw, dh))
        torch.cuda.synchronize()
        out[kind] = (prefix, disp.cpu().numpy(), st.cpu().tolist())
    assert out["svcq"][2] == [0, 0, 0, 0, code, 0x100 | code, 0x100 | code, 0, 0, 0, 0] and out["svce"][2] == [0] * N
    assert out["svce"][1].any() and not out["svcq"][1][4:7].any()
    return d, (dw, dh), out


def _run(d, prefix, size, batch, depth, reduce, out):
    return subprocess.run([EXE, prefix, str(N), str(size[0]), str(size[1]), str(d / "gaze.txt"), str(d / "key.txt"), str(batch), str(depth),
                           str(reduce), str(out)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("kind", ["svcq", "svce"])
def test_any_batch_size_gives_the_device_calls_frames(streams, kind, depth):
    d, size, out = streams
    prefix, want, want_status = out[kind]
    for batch in (1, 4, 16):
        path = d / f"{kind}_{batch}_{depth}.raw"
        r = _run(d, prefix, size, batch, depth, 1, path)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(path, np.uint8).reshape(want.shape)
        assert np.fromfile(str(path) + ".status", np.uint32).tolist() == want_status, (batch, depth)
        assert np.array_equal(got, want), (batch, depth)


def test_a_reduced_size_is_refused(streams):
    d, size, out = streams
    r = _run(d, out["svcq"][0], (0, 0), 4, 3, 2, d / "refused.raw")
    assert r.returncode == 1 and "DecodeDelta does not decode at reduced size" in r.stderr, r.stdout + r.stderr
