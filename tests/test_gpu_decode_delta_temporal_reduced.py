"""svc_hip_decode_delta_levels_temporal_reduced_frames on the device (include/svc_hip_temporal_decode.h: a delta stream with temporal layers
straight to display frames at 1/2, 1/4, 1/8 size).

Its contract is bit equality with calls already in the tree and pinned by their own tests: svc_hip_undelta_levels_temporal_frames
(tests/test_gpu_delta_temporal.py) with the same frame before, key flags and period, then svc_hip_decode_levels_reduced_frames on its
output with the same steps, reduce, gaze and display size -- rec, display and the undelta call's status; `last` is
svc_hip_band_levels_frames at (0, 0, K, K) of the undelta call's output frame period * ((n - 1) // period).  Every output is pre-filled as
tests/test_gpu_decode_delta_reduced.py fills it, and the fill behind last_bytes is asserted.  The geometries are that file's: a partial last
group, a single column of groups, both tile sizes -- with all three reduces of each and both periods."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_delta_levels_host import STEPS, delta_clip, with_a_zero_level
from tests.test_delta_temporal_host import KEYS, N
from tests.test_gpu_band_levels import _band_call, _damaged, _offsets
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_decode_delta import _gaze
from tests.test_gpu_decode_delta_reduced import (CASES, DENSITY, GEOMS, OTHER_DEC, REC_FILL, REC_FILL_BITS, REDUCES, _band, _band_of, _bits,
                                                 _cid, _displays, _loud_outside, _same, _served, _with_a_zero_level_at, _zero_frames)
from tests.test_gpu_decode_delta_reduced import _fused as _plain_fused
from tests.test_gpu_window_levels import _call as _window_call
from tests.test_gpu_window_levels import _dev

pytestmark = pytest.mark.gpu

PERIODS = (2, 4)


def _last_index(n, period):
    return period * ((n - 1) // period)


def _undelta(diff, offs, geom, period, keys=None, prev=None):
    """svc_hip_undelta_levels_temporal_frames -> (stream on the device, its offsets on the device, the offsets as a list, the statuses)"""
    w, h, tile, mv = geom
    back, back_offs, st = nat.undelta_levels_temporal_frames(_dev(diff), _offsets(offs), w, h, tile, mv, period,
                                                             prev=None if prev is None else _dev(prev), key=keys)
    o = back_offs.cpu().tolist()
    return back[:o[-1]].clone(), back_offs, o, st.cpu().tolist()


def _two_calls(diff, offs, geom, r, period, keys=None, prev=None, steps=(1, 640), gaze=None, display=None):
    """The reference: temporal undelta, then the reduced decode -> (rec bits, display, the undelta's status, the band (0, 0, K, K) of its
    output frame period * ((n - 1) // period))."""
    w, h, tile, mv = geom
    stream, back_offs, o, st = _undelta(diff, offs, geom, period, keys, prev)
    rec, disp, _ = nat.decode_levels_reduced_frames(stream, back_offs, w, h, tile, mv, *steps, r, gaze=gaze, display=display)
    torch.cuda.synchronize()
    at = _last_index(len(o) - 1, period)
    return _bits(rec), None if disp is None else disp.cpu(), st, _band_of(stream[o[at]:o[at + 1]].cpu().numpy().tobytes(), geom, r)


def _fused(diff, offs, geom, r, period, keys=None, prev=None, steps=(1, 640), gaze=None, display=None, want_last=True):
    """The call under test into pre-filled outputs -> (rec bits, display, status, last); the fill behind last_bytes is asserted."""
    w, h, tile, mv = geom
    offsets = _offsets(offs)
    n = offsets.numel() - 1
    rec = torch.full((n, h // r, w // r, 3), REC_FILL, dtype=torch.float32, device="cuda")
    disp = None if display is None else torch.full((n, display[1], display[0], 3), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    last = torch.full((nat.levels_max_bytes(1, w, h, tile, mv),), FILL, dtype=torch.uint8, device="cuda") if want_last else None
    got = nat.decode_delta_levels_temporal_reduced_frames(_dev(diff), offsets, w, h, tile, mv, period, *steps, r,
                                                          prev=None if prev is None else _dev(prev), key=keys, gaze=gaze, display=display,
                                                          rec=rec, out_display=disp, last=last, status=status)
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


@functools.lru_cache(maxsize=None)
def _delta(geom, density, period, keyed):
    """The clip's temporal delta stream by the numpy statement, computed once -> (bytes, offsets)."""
    return layers.delta_temporal_frames(*_clip(geom, density), period, KEYS if keyed else None)


# ---- 1. against the two calls ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_against_temporal_undelta_then_reduced_decode(native, case, density, period):
    geom, r = case
    frames = frames_of(*_clip(geom, density))
    gaze = _gaze(N, geom)
    want_last = layers.band_frame(frames[_last_index(N, period)], _band(geom, r))  # the band of the stream's own frame
    for keys in (KEYS, None):
        diff, diff_offs = _delta(geom, density, period, keys is not None)
        for steps, display in zip((STEPS, OTHER_DEC), _displays(geom, r)):
            kw = dict(keys=keys, steps=steps, gaze=gaze, display=display)
            want = _two_calls(diff, diff_offs, geom, r, period, **kw)
            got = _fused(diff, diff_offs, geom, r, period, **kw)
            _same(got, want, (keys, steps, display))
            assert got[2] == [0] * N and got[3] == want_last
            assert not (got[0] == REC_FILL_BITS).any()  # every pixel is written
        # no gaze, no display and no d_last
        _same(_fused(diff, diff_offs, geom, r, period, keys=keys, want_last=False), _two_calls(diff, diff_offs, geom, r, period, keys=keys))
    if density != "zero":
        assert _two_calls(*_delta(geom, density, period, True), geom, r, period, keys=KEYS, steps=STEPS)[0].any()  # pictures, not zeros


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_period_one_is_the_reduced_call(native, case):
    """All five outputs: rec, display, status, last and its length (the fill behind it is asserted on both sides)."""
    geom, r = case
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    for keys in (KEYS, None):
        diff, diff_offs = layers.delta_frames(stream, offs, keys)
        kw = dict(keys=keys, steps=OTHER_DEC, gaze=_gaze(N, geom), display=_displays(geom, r)[1])
        got, want = _fused(diff, diff_offs, geom, r, 1, **kw), _plain_fused(diff, diff_offs, geom, r, **kw)
        _same(got, want, keys)
        assert got[3] == want[3] == layers.band_frame(f[N - 1], _band(geom, r)) and len(got[3]) == len(want[3])
    d = layers.delta_frames(*entropy._join(f[1:]), prev=f[0])
    bad, _ = _damaged(*d, 3, "levels")
    for stream_ in (d[0], bad):
        got, want = _fused(stream_, d[1], geom, r, 1, prev=f[0]), _plain_fused(stream_, d[1], geom, r, prev=f[0])
        _same(got, want)
        assert got[3] == want[3]


# ---- 2. the served stream: band and thinning -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_on_the_band_of_the_temporal_stream(native, case, period):
    """A server stores the temporal stream and sends the band (0, 0, K, K) of it: every output has the bits it has on the full stream."""
    geom, r = case
    gaze, display = _gaze(N, geom), _displays(geom, r)[1]
    for density in ("sparse", "full"):
        for keys in (KEYS, None):
            diff, diff_offs = _delta(geom, density, period, keys is not None)
            band, band_offs = _served(diff, diff_offs, geom, r)
            assert len(band) < len(diff)
            kw = dict(keys=keys, steps=OTHER_DEC, gaze=gaze, display=display)
            full = _fused(diff, diff_offs, geom, r, period, **kw)
            got = _fused(band, band_offs, geom, r, period, **kw)
            _same(got, full, (density, keys))
            assert got[3] == full[3] and got[2] == [0] * N
    # a frame damaged on its way fails alike in both
    diff, diff_offs = _delta(geom, "sparse", period, False)
    band, band_offs = _served(diff, diff_offs, geom, r)
    bad, code = _damaged(band, band_offs, 4, "levels")
    got = _fused(bad, band_offs, geom, r, period, steps=STEPS, display=display)
    assert got[2] == layers.temporal_statuses([code if i == 4 else 0 for i in range(N)], period).tolist()
    full = _fused(_damaged(diff, diff_offs, 4, "levels")[0], diff_offs, geom, r, period, steps=STEPS, display=display)
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]) and got[3] == full[3] == bytes(64)


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[4]], ids=_cid)
def test_the_small_slow_viewers_stream(native, case, period):
    """What the window call (d_src, no window) and the band call make of the stored stream for a viewer of 1 / 2^s of the frames at
    1 / reduce of the size is the same bytes in either order; it plays the kept frames' pictures at period >> s, and at a remaining period
    of 1 through svc_hip_decode_delta_levels_reduced_frames."""
    geom, r = case
    diff, diff_offs = _delta(geom, "sparse", period, True)
    gaze, display = _gaze(N, geom), _displays(geom, r)[1]
    whole = _fused(diff, diff_offs, geom, r, period, keys=KEYS, steps=OTHER_DEC, gaze=gaze, display=display)
    for every in (2, 4):
        if every > period:
            continue
        kept = list(range(0, N, every))
        bands = [_band(geom, r)] * len(kept)
        thin, thin_offs, _ = _window_call(diff, diff_offs, geom, src=kept)
        thin_then_band, a_offs, _ = _band_call(thin[:thin_offs[-1]], thin_offs, geom, bands=bands)
        band, band_offs = _served(diff, diff_offs, geom, r)
        band_then_thin, b_offs, _ = _window_call(band, band_offs, geom, src=kept)
        assert list(a_offs) == list(b_offs) and thin_then_band[:a_offs[-1]].tobytes() == band_then_thin[:b_offs[-1]].tobytes()
        served = thin_then_band[:a_offs[-1]].tobytes()
        assert served == layers.band_frames(*layers.thin_frames(diff, diff_offs, KEYS, every)[:2], bands)[0]
        kw = dict(keys=[KEYS[i] for i in kept], steps=OTHER_DEC, gaze=[gaze[i] for i in kept], display=display)
        got = _fused(served, a_offs, geom, r, period // every, **kw)
        assert got[2] == [0] * len(kept)
        assert torch.equal(got[0], whole[0][kept]) and torch.equal(got[1], whole[1][kept])
        if period == every:
            plain = _plain_fused(served, a_offs, geom, r, **kw)
            assert torch.equal(plain[0], whole[0][kept]) and torch.equal(plain[1], whole[1][kept]) and plain[2] == got[2]
            assert plain[3] == got[3]


# ---- 3. d_last and chaining ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_frame_counts_around_the_period(native, case, period):
    """`last` is the band of frame 0 for up to `period` frames and of frame `period` for one more -- with no frame before, with the full
    frame, with its band, and with the full-size temporal call's d_last."""
    geom, r = case
    w, h, tile, mv = geom
    f = frames_of(*_clip(geom, "sparse"))
    head = layers.delta_temporal_frames(*entropy._join(f[:period]), period)  # the call before: frames 0 .. period - 1, `last` is frame 0
    before = nat.decode_delta_levels_temporal_frames(_dev(head[0]), _offsets(head[1]), w, h, tile, mv, period, want_last=True)
    from_full_size = before[3][:int(before[4].item())].cpu().numpy().tobytes()
    assert from_full_size == f[0]
    for n in sorted({1, period - 1, period, period + 1}):
        for prev in (None, f[0], layers.band_frame(f[0], _band(geom, r)), from_full_size):
            part = entropy._join(f[period:period + n])
            diff = layers.delta_temporal_frames(*part, period, prev=None if prev is None else f[0])
            kw = dict(prev=prev, steps=OTHER_DEC, gaze=_gaze(n, geom), display=_displays(geom, r)[1])
            got = _fused(*diff, geom, r, period, **kw)
            _same(got, _two_calls(*diff, geom, r, period, **kw), (n, prev is None))
            assert got[2] == [0] * n and got[3] == layers.band_frame(f[period + _last_index(n, period)], _band(geom, r))


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("r", REDUCES)
def test_a_chain_cut_into_calls_of_one_period(native, r, period):
    """33 frames in calls of `period` frames: every call's `last` is the band of its frame 0, reconstructed, and the next call's `prev`;
    alone, and alternating with svc_hip_undelta_levels_temporal_frames on the band stream with the reduced decode behind it."""
    geom = GEOMS[0]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(33), geom, 33, 0.5)
    f = frames_of(stream, offs)
    keys = [int(i in (0, 16, 17, 22)) for i in range(33)]
    diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, keys)
    band, band_offs = _served(diff, diff_offs, geom, r)
    d = frames_of(band, band_offs)
    kw = dict(steps=OTHER_DEC, display=_displays(geom, r)[1])
    gaze = _gaze(33, geom)
    whole = _fused(diff, diff_offs, geom, r, period, keys=keys, gaze=gaze, **kw)
    _same(whole, _two_calls(diff, diff_offs, geom, r, period, keys=keys, gaze=gaze, **kw))
    assert whole[2] == [0] * 33 and whole[3] == layers.band_frame(f[32], _band(geom, r))
    for alternate in (False, True):
        prev, recs, disps = None, [], []
        for turn, lo in enumerate(range(0, 33, period)):
            hi = min(lo + period, 33)
            part = entropy._join(d[lo:hi])
            if alternate and turn % 2:
                back, back_offs, o, st = _undelta(*part, geom, period, keys[lo:hi], prev)
                rec, disp, _ = nat.decode_levels_reduced_frames(back, back_offs, w, h, tile, mv, *OTHER_DEC, r, gaze=gaze[lo:hi], display=kw["display"])
                assert st == [0] * (hi - lo)
                recs.append(_bits(rec))
                disps.append(disp.cpu())
                prev = back[o[0]:o[1]].cpu().numpy().tobytes()
            else:
                got = _fused(*part, geom, r, period, keys=keys[lo:hi], prev=prev, gaze=gaze[lo:hi], **kw)
                assert got[2] == [0] * (hi - lo)
                recs.append(got[0])
                disps.append(got[1])
                prev = got[3]
            assert prev == layers.band_frame(f[lo], _band(geom, r)), lo
        assert torch.equal(torch.cat(recs), whole[0]) and torch.equal(torch.cat(disps), whole[1]), alternate


# ---- 4. statuses ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", CASES[:6], ids=_cid)
def test_a_damaged_frame_in_every_layer(native, case, period):
    geom, r = case
    f = frames_of(*_clip(geom, "sparse"))
    li = _last_index(N, period)
    for keys in (None, KEYS):
        diff, diff_offs = _delta(geom, "sparse", period, keys is not None)
        kw = dict(keys=keys, steps=STEPS, gaze=_gaze(N, geom), display=_displays(geom, r)[0])
        good = _fused(diff, diff_offs, geom, r, period, **kw)
        for at, what in ((4, "magic"), (2, "size"), (5, "levels"), (li, "magic")):
            bad, code = _damaged(diff, diff_offs, at, what)
            got = _fused(bad, diff_offs, geom, r, period, **kw)
            _same(got, _two_calls(bad, diff_offs, geom, r, period, **kw), (at, what))
            codes = layers.temporal_statuses([code if i == at else 0 for i in range(N)], period, keys).tolist()
            assert got[2] == codes
            assert _zero_frames(got[0]) == [c != 0 for c in codes]
            for i, c in enumerate(codes):  # the frames that do not hang on it are intact
                assert c != 0 or (torch.equal(got[0][i], good[0][i]) and torch.equal(got[1][i], good[1][i])), (at, i)
            assert got[3] == (bytes(64) if codes[li] else layers.band_frame(f[li], _band(geom, r)))  # a `last` that failed is 64 zero bytes


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("r", REDUCES)
def test_a_damaged_frame_before(native, r, period):
    geom = GEOMS[0]
    f = frames_of(*_clip(geom, "sparse", N + 1))
    for keys in (None, KEYS):
        d = layers.delta_temporal_frames(*entropy._join(f[1:]), period, keys, prev=f[0])
        for prev in (f[0], layers.band_frame(f[0], _band(geom, r))):
            good = _fused(*d, geom, r, period, keys=keys, prev=prev, steps=STEPS)
            _same(good, _two_calls(*d, geom, r, period, keys=keys, prev=prev, steps=STEPS))
            assert good[2] == [0] * N and good[3] == layers.band_frame(f[1 + _last_index(N, period)], _band(geom, r))
            for what in ("magic", "size", "levels"):
                bad, code = _damaged(prev, [0, len(prev)], 0, what)
                got = _fused(*d, geom, r, period, keys=keys, prev=bad, steps=STEPS)
                _same(got, _two_calls(*d, geom, r, period, keys=keys, prev=bad, steps=STEPS), what)
                codes = layers.temporal_statuses([0] * N, period, keys, prev=code).tolist()
                assert got[2] == codes and _zero_frames(got[0]) == [c != 0 for c in codes]
        got = _fused(*d, geom, r, period, prev=f[0][:48], steps=STEPS)  # less than a header: out of range
        assert got[2] == [0x101] * N and got[3] == bytes(64)


# ---- 5. levels -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", CASES[:6], ids=_cid)
def test_a_set_bit_of_level_zero(native, case, period):
    """Inside K x K it gives the pixels of the stream without it, and `last` comes with the bit cleared; outside K x K it is never read."""
    geom, r = case
    band = _band(geom, r)
    stream, offs = delta_clip(np.random.default_rng(5), geom, period + 1)
    d = frames_of(*layers.delta_temporal_frames(stream, offs, period))
    for zero in (with_a_zero_level, lambda fr: _with_a_zero_level_at(fr, band[2], True), lambda fr: _with_a_zero_level_at(fr, band[2], False)):
        for at in (0, period):  # a key frame that others refer to, and the next frame of layer 0: the call's `last`
            bad, clean = zero(d[at])
            assert bad != clean
            with_bit, without = entropy._join(d[:at] + [bad] + d[at + 1:]), entropy._join(d[:at] + [clean] + d[at + 1:])
            got = _fused(*with_bit, geom, r, period, steps=STEPS)
            _same(got, _two_calls(*with_bit, geom, r, period, steps=STEPS))
            want = _fused(*without, geom, r, period, steps=STEPS)
            assert torch.equal(got[0], want[0]) and got[2] == [0] * (period + 1) and got[3] == want[3]
            assert got[3] == layers.band_frame(frames_of(*layers.undelta_temporal_frames(*without, period))[period], band)


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_nothing_outside_the_first_k_by_k_is_read(native, case, period):
    """Levels of +-32767 everywhere outside K x K, in every frame and in the frame before, change nothing."""
    geom, r = case
    k = _band(geom, r)[2]
    f = frames_of(*_clip(geom, "sparse", N + 1))
    d = frames_of(*layers.delta_temporal_frames(*entropy._join(f[1:]), period, KEYS, prev=f[0]))
    kw = dict(keys=KEYS, steps=OTHER_DEC, gaze=_gaze(N, geom), display=_displays(geom, r)[1])
    want = _fused(*entropy._join(d), geom, r, period, prev=f[0], **kw)
    loud = entropy._join([_loud_outside(fr, k, i) for i, fr in enumerate(d)])
    assert len(loud[0]) > len(b"".join(d))
    got = _fused(*loud, geom, r, period, prev=_loud_outside(f[0], k, 1), **kw)
    _same(got, want)
    assert got[3] == want[3] == layers.band_frame(f[1 + _last_index(N, period)], _band(geom, r))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[1]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    fn = nat.decode_delta_levels_temporal_reduced_frames
    small = torch.empty(16, dtype=torch.uint8, device="cuda")

    def refused(match, status, *args, **kw):
        with pytest.raises(nat.SvcError, match=match) as e:
            fn(*args, **kw)
        assert e.value.status == status

    bad, unsup = nat.SVC_ERR_INVALID_ARG, nat.SVC_ERR_UNSUPPORTED
    for period in (0, 3, 8):
        refused(f"period {period}", bad, frames, offsets, w, h, tile, mv, period, 0, 16, 3, workspace=small)  # before steps and reduce
    refused("not divisible", bad, frames, offsets, w + 1, h, tile, mv, 3, workspace=small)  # after the geometry
    refused("8x8, 16x16", unsup, frames, offsets, 48, 32, (16, 8), (16, 8), 2, workspace=small)
    refused("steps", bad, frames, offsets, w, h, tile, mv, 2, 0, 16)
    for r in (1, 3, 16):
        refused("reduce", bad, frames, offsets, w, h, tile, mv, 4, 1, 640, r)
    refused("display", bad, frames, offsets, w, h, tile, mv, 4, 1, 640, 4, display=(w // 4 + 1, h // 4))
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
