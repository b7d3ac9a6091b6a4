"""svc_hip_decode_delta_levels_temporal_frames on the device (include/svc_hip.h, "Temporal layers": a delta stream with temporal layers
straight to display frames).

Its contract is bit equality with two calls pinned by their own tests: svc_hip_undelta_levels_temporal_frames
(tests/test_gpu_delta_temporal.py) with the same frame before, key flags and period, then svc_hip_decode_levels_frames on its output with
the same steps, gaze and display size -- rec, display and the undelta call's status; `last` is the undelta call's output frame
period * ((n - 1) // period).  Every output is pre-filled as tests/test_gpu_decode_delta.py fills it, and the fill behind last_bytes is
asserted."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_delta_levels_host import STEPS, _gid, delta_clip, with_a_zero_level
from tests.test_delta_temporal_host import KEYS, N, PERIODS
from tests.test_gpu_band_levels import _damaged, _offsets
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_decode_delta import DENSITY, GEOMS, OTHER_DEC, REC_FILL, _bits, _displays, _gaze, _same, _zero_frames
from tests.test_gpu_decode_delta import _fused as _plain_fused
from tests.test_gpu_window_levels import _dev

pytestmark = pytest.mark.gpu


def _last_index(n, period):
    return period * ((n - 1) // period)


def _two_calls(diff, offs, geom, period, keys=None, prev=None, steps=(1, 640), gaze=None, display=None):
    """The reference: temporal undelta, then decode -> (rec bits, display, the undelta's status, the undelta's output frame
    period * ((n - 1) // period))."""
    w, h, tile, mv = geom
    back, back_offs, st = nat.undelta_levels_temporal_frames(_dev(diff), _offsets(offs), w, h, tile, mv, period,
                                                             prev=None if prev is None else _dev(prev), key=keys)
    o = back_offs.cpu().tolist()
    stream = back[:o[-1]].clone()
    rec, disp, _ = nat.decode_levels_frames(stream, back_offs, w, h, tile, mv, *steps, gaze=gaze, display=display)
    torch.cuda.synchronize()
    at = _last_index(len(o) - 1, period)
    return _bits(rec), None if disp is None else disp.cpu(), st.cpu().tolist(), stream[o[at]:o[at + 1]].cpu().numpy().tobytes()


def _fused(diff, offs, geom, period, keys=None, prev=None, steps=(1, 640), gaze=None, display=None, want_last=True):
    """The call under test into pre-filled outputs -> (rec bits, display, status, last); the fill behind last_bytes is asserted."""
    w, h, tile, mv = geom
    offsets = _offsets(offs)
    n = offsets.numel() - 1
    rec = torch.full((n, h, w, 3), REC_FILL, dtype=torch.float32, device="cuda")
    disp = None if display is None else torch.full((n, display[1], display[0], 3), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    last = torch.full((nat.levels_max_bytes(1, w, h, tile, mv),), FILL, dtype=torch.uint8, device="cuda") if want_last else None
    got = nat.decode_delta_levels_temporal_frames(_dev(diff), offsets, w, h, tile, mv, period, fg_step=steps[0], bg_step=steps[1],
                                                  prev=None if prev is None else _dev(prev), key=keys, gaze=gaze, display=display, rec=rec,
                                                  out_display=disp, last=last, status=status)
    torch.cuda.synchronize()
    assert got[0] is rec and got[1] is disp and got[2] is status and got[3] is last
    frame = None
    if want_last:
        used = int(got[4].item())
        assert 64 <= used <= last.numel() and used % 16 == 0
        host = last.cpu().numpy()
        assert (host[used:] == FILL).all()  # nothing is written behind the frame
        frame = host[:used].tobytes()
    else:
        assert got[4] is None
    return _bits(rec), None if disp is None else disp.cpu(), status.cpu().tolist(), frame


@functools.lru_cache(maxsize=None)
def _clip(geom, density, n=N):
    w, h = geom[:2]
    return delta_clip(np.random.default_rng(w * 7 + h + len(density)), geom, n, DENSITY[density])


# ---- 1. against the two calls ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_against_undelta_then_decode(native, geom, density, period):
    stream, offs = _clip(geom, density)
    frames = frames_of(stream, offs)
    gaze = _gaze(N, geom)
    for keys in (KEYS, None):
        diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, keys)
        for steps, display in zip((STEPS, OTHER_DEC), _displays(geom)):
            kw = dict(keys=keys, steps=steps, gaze=gaze, display=display)
            want = _two_calls(diff, diff_offs, geom, period, **kw)
            got = _fused(diff, diff_offs, geom, period, **kw)
            _same(got, want, (keys, steps, display))
            assert got[2] == [0] * N and got[3] == frames[_last_index(N, period)]
            assert not (got[0] == int(np.float32(REC_FILL).view(np.int32))).any()  # every pixel is written
            if period == 1:  # exactly the plain call
                _same(got, _plain_fused(diff, diff_offs, geom, **kw))
        _same(_fused(diff, diff_offs, geom, period, keys=keys, want_last=False), _two_calls(diff, diff_offs, geom, period, keys=keys))
    if density != "zero":
        assert _two_calls(*layers.delta_temporal_frames(stream, offs, period), geom, period, steps=STEPS)[0].any()  # pictures, not zeros


@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_frame_counts_around_the_period(native, geom, period):
    """`last` is frame 0 for up to `period` frames and frame `period` for one more."""
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    for n in sorted({1, period - 1, period, period + 1}):
        for prev in (None, f[10]):
            part = entropy._join(f[:n])
            diff = layers.delta_temporal_frames(*part, period, prev=prev)
            kw = dict(prev=prev, steps=OTHER_DEC, gaze=_gaze(n, geom), display=_displays(geom)[1])
            got = _fused(*diff, geom, period, **kw)
            _same(got, _two_calls(*diff, geom, period, **kw), (n, prev is None))
            assert got[2] == [0] * n and got[3] == f[_last_index(n, period)]


@pytest.mark.parametrize("period", [2, 4])
def test_the_thinned_stream_shows_the_kept_frames(native, period):
    """The kept frames through the call at the smaller period, and at remaining period 1 through svc_hip_decode_delta_levels_frames: the
    pictures of those frames in the full decode, bit for bit."""
    geom = GEOMS[0]
    stream, offs = _clip(geom, "sparse")
    diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, KEYS)
    gaze, display = _gaze(N, geom), _displays(geom)[1]
    whole = _fused(diff, diff_offs, geom, period, keys=KEYS, steps=OTHER_DEC, gaze=gaze, display=display)
    for every in (2, 4):
        if every > period:
            continue
        kept = list(range(0, N, every))
        thin, thin_offs, thin_keys = layers.thin_frames(diff, diff_offs, KEYS, every)
        kw = dict(keys=[int(k) for k in thin_keys], steps=OTHER_DEC, gaze=[gaze[i] for i in kept], display=display)
        got = _fused(thin, thin_offs, geom, period // every, **kw)
        assert got[2] == [0] * len(kept)
        assert torch.equal(got[0], whole[0][kept]) and torch.equal(got[1], whole[1][kept])
        if period == every:
            plain = _plain_fused(thin, thin_offs, geom, **kw)
            assert torch.equal(plain[0], whole[0][kept]) and torch.equal(plain[1], whole[1][kept]) and plain[2] == got[2]


@pytest.mark.parametrize("period", [2, 4])
def test_a_chain_cut_into_calls_of_one_period(native, period):
    """33 frames in calls of `period` frames: every call's `last` is its frame 0, reconstructed, and the next call's `prev`."""
    geom = GEOMS[0]
    stream, offs = delta_clip(np.random.default_rng(33), geom, 33, 0.5)
    f = frames_of(stream, offs)
    keys = [int(i in (0, 16, 17, 22)) for i in range(33)]
    diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, keys)
    d = frames_of(diff, diff_offs)
    kw = dict(steps=OTHER_DEC, display=_displays(geom)[1])
    gaze = _gaze(33, geom)
    whole = _fused(diff, diff_offs, geom, period, keys=keys, gaze=gaze, **kw)
    _same(whole, _two_calls(diff, diff_offs, geom, period, keys=keys, gaze=gaze, **kw))
    assert whole[2] == [0] * 33 and whole[3] == f[32]
    prev, recs, disps = None, [], []
    for lo in range(0, 33, period):
        hi = min(lo + period, 33)
        got = _fused(*entropy._join(d[lo:hi]), geom, period, keys=keys[lo:hi], prev=prev, gaze=gaze[lo:hi], **kw)
        assert got[2] == [0] * (hi - lo) and got[3] == f[lo], lo
        prev = got[3]
        recs.append(got[0])
        disps.append(got[1])
    assert torch.equal(torch.cat(recs), whole[0]) and torch.equal(torch.cat(disps), whole[1])


# ---- 2. statuses ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_a_damaged_frame_in_every_layer(native, geom, period):
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    li = _last_index(N, period)
    for keys in (None, KEYS):
        diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, keys)
        kw = dict(keys=keys, steps=STEPS, gaze=_gaze(N, geom), display=_displays(geom)[0])
        good = _fused(diff, diff_offs, geom, period, **kw)
        for at, what in ((4, "magic"), (2, "size"), (5, "levels"), (li, "magic")):
            bad, code = _damaged(diff, diff_offs, at, what)
            got = _fused(bad, diff_offs, geom, period, **kw)
            _same(got, _two_calls(bad, diff_offs, geom, period, **kw), (at, what))
            codes = layers.temporal_statuses([code if i == at else 0 for i in range(N)], period, keys).tolist()
            assert got[2] == codes
            assert _zero_frames(got[0]) == [c != 0 for c in codes]
            for i, c in enumerate(codes):  # the frames that do not hang on it are intact
                assert c != 0 or (torch.equal(got[0][i], good[0][i]) and torch.equal(got[1][i], good[1][i])), (at, i)
            assert got[3] == (bytes(64) if codes[li] else f[li])  # a `last` that failed is 64 zero bytes


@pytest.mark.parametrize("period", [2, 4])
def test_a_damaged_frame_before(native, period):
    geom = GEOMS[0]
    stream, offs = _clip(geom, "sparse", N + 1)
    f = frames_of(stream, offs)
    for keys in (None, KEYS):
        d = layers.delta_temporal_frames(*entropy._join(f[1:]), period, keys, prev=f[0])
        good = _fused(*d, geom, period, keys=keys, prev=f[0], steps=STEPS)
        _same(good, _two_calls(*d, geom, period, keys=keys, prev=f[0], steps=STEPS))
        assert good[2] == [0] * N and good[3] == f[1 + _last_index(N, period)]
        for what in ("magic", "size", "levels"):
            bad, code = _damaged(f[0], [0, len(f[0])], 0, what)
            got = _fused(*d, geom, period, keys=keys, prev=bad, steps=STEPS)
            _same(got, _two_calls(*d, geom, period, keys=keys, prev=bad, steps=STEPS), what)
            codes = layers.temporal_statuses([0] * N, period, keys, prev=code).tolist()
            assert got[2] == codes and _zero_frames(got[0]) == [c != 0 for c in codes]
        got = _fused(*d, geom, period, prev=f[0][:48], steps=STEPS)  # less than a header: out of range
        assert got[2] == [0x101] * N and got[3] == bytes(64)


@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_a_set_bit_of_level_zero(native, geom, period):
    """In the delta stream it gives the pixels of the stream without it, and `last` comes with the bit cleared."""
    stream, offs = delta_clip(np.random.default_rng(5), geom, period + 1)
    d = frames_of(*layers.delta_temporal_frames(stream, offs, period))
    for at in (0, period):  # a key frame that others refer to, and the next frame of layer 0: the call's `last`
        bad, clean = with_a_zero_level(d[at])
        assert bad != clean
        with_bit, without = entropy._join(d[:at] + [bad] + d[at + 1:]), entropy._join(d[:at] + [clean] + d[at + 1:])
        got = _fused(*with_bit, geom, period, steps=STEPS)
        _same(got, _two_calls(*with_bit, geom, period, steps=STEPS))
        want = _fused(*without, geom, period, steps=STEPS)
        assert torch.equal(got[0], want[0]) and got[2] == [0] * (period + 1) and got[3] == want[3]
        assert got[3] == frames_of(*layers.undelta_temporal_frames(*without, period))[period]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[1]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    fn = nat.decode_delta_levels_temporal_frames
    small = torch.empty(16, dtype=torch.uint8, device="cuda")

    def refused(match, status, *args, **kw):
        with pytest.raises(nat.SvcError, match=match) as e:
            fn(*args, **kw)
        assert e.value.status == status

    bad, unsup = nat.SVC_ERR_INVALID_ARG, nat.SVC_ERR_UNSUPPORTED
    for period in (0, 3, 8):
        refused(f"period {period}", bad, frames, offsets, w, h, tile, mv, period, fg_step=0, workspace=small)  # before the steps
    refused("not divisible", bad, frames, offsets, w + 1, h, tile, mv, 3, workspace=small)  # after the geometry
    refused("8x8, 16x16", unsup, frames, offsets, 48, 32, (16, 8), (16, 8), 2, workspace=small)
    refused("steps", bad, frames, offsets, w, h, tile, mv, 2, fg_step=0, bg_step=16)
    refused("display", bad, frames, offsets, w, h, tile, mv, 4, display=(w + 1, h))
    refused("workspace", bad, frames, offsets, w, h, tile, mv, 4, workspace=small)
    refused("last frame", bad, frames, offsets, w, h, tile, mv, 2,
            last=torch.empty(nat.levels_max_bytes(1, w, h, tile, mv) - 16, dtype=torch.uint8, device="cuda"))
    refused("aligned", bad, frames, offsets, w, h, tile, mv, 2, prev=torch.zeros(80, dtype=torch.uint8, device="cuda")[8:])
    # no frames: nothing is written, whatever the sizes
    last = torch.full((nat.levels_max_bytes(1, w, h, tile, mv),), FILL, dtype=torch.uint8, device="cuda")
    none = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    got = fn(frames[:0], none, w, h, tile, mv, 4, last=last, workspace=small)
    torch.cuda.synchronize()
    assert (last == FILL).all() and none.tolist() == [-1] and got[0].numel() == 0
