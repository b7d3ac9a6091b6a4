"""svc_hip_delta_levels_temporal_frames and svc_hip_undelta_levels_temporal_frames on the device (include/svc_hip.h, "Temporal layers").

Their contract is byte equality with the numpy statements layers.delta_temporal_frames / layers.undelta_temporal_frames, whose own
properties (the round trip, the thinning identity, the cuts) are tests/test_delta_temporal_host.py; the statuses are
layers.temporal_statuses, pinned there to trees written by hand.  Every call writes into a stream pre-filled with FILL and offsets and
status pre-filled with -1; all n + 1 offsets, the bytes up to the last one and FILL behind it are asserted."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_delta_levels_host import BAND_GEOMS, _gid, delta_clip, with_a_zero_level
from tests.test_delta_temporal_host import KEYS, N, PERIODS
from tests.test_gpu_band_levels import HOST12, _damaged, _offsets, _used
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_delta_levels import _delta as _plain_delta
from tests.test_gpu_delta_levels import _expect_frames
from tests.test_gpu_delta_levels import _undelta as _plain_undelta
from tests.test_gpu_window_levels import _call as _window_call
from tests.test_gpu_window_levels import _dev, _expect
from tests.test_window_levels_host import geom_dict, random_types

pytestmark = pytest.mark.gpu

DENSITY = {"zero": 0.0, "sparse": 0.06, "full": 1.0}


def _call(undo, stream, offs, geom, period, keys=None, prev=None):
    """One of the two calls on a stream tensor of exactly its bytes (and a frame before it of exactly its) -> (output u8 on the host,
    offsets, status), each whole."""
    w, h, tile, mv = geom
    frames, offsets = _dev(stream), _offsets(offs)
    n = offsets.numel() - 1
    out = torch.full((max(nat.levels_max_bytes(n, w, h, tile, mv), 16),), FILL, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    fn = nat.undelta_levels_temporal_frames if undo else nat.delta_levels_temporal_frames
    fn(frames, offsets, w, h, tile, mv, period, prev=None if prev is None else _dev(prev), key=keys, out=out, out_offsets=out_offs,
       status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _delta(*args, **kw):
    return _call(False, *args, **kw)


def _undelta(*args, **kw):
    return _call(True, *args, **kw)


def _cut(keys, lo, hi):
    return None if keys is None else keys[lo:hi]


# ---- 1. against the numpy statements, and back -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_both_calls_against_the_numpy_statement(native, geom, density):
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(w * 7 + h + len(density)), geom, N, DENSITY[density])
    for period in PERIODS:
        for keys in (KEYS, None):
            want, want_offs = layers.delta_temporal_frames(stream, offs, period, keys)
            got = _delta(stream, offs, geom, period, keys)
            _expect(got, want, want_offs)
            assert got[2] == [0] * N
            back = _undelta(*_used(got), geom, period, keys)  # the round trip on the device
            _expect(back, stream, offs)
            assert back[2] == [0] * N
            if period == 1:  # exactly the plain calls
                plain = _plain_delta(stream, offs, geom, keys)
                assert plain[1] == got[1] and plain[0].tobytes() == got[0].tobytes() and plain[2] == got[2]
                plain = _plain_undelta(want, want_offs, geom, keys)
                assert plain[1] == back[1] and plain[0].tobytes() == back[0].tobytes() and plain[2] == back[2]


@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", [BAND_GEOMS[0], BAND_GEOMS[2], BAND_GEOMS[5]], ids=_gid)
def test_frame_counts_around_the_period(native, geom, period):
    stream, offs = delta_clip(np.random.default_rng(41 + period), geom, N, 0.3)
    f = frames_of(stream, offs)
    for n in sorted({1, period - 1, period, period + 1}):
        for keys in (None, KEYS[3:3 + n]):
            part = entropy._join(f[:n])
            want, want_offs = layers.delta_temporal_frames(*part, period, keys)
            _expect(_delta(*part, geom, period, keys), want, want_offs)
            _expect(_undelta(want, want_offs, geom, period, keys), *part)
            want, want_offs = layers.delta_temporal_frames(*part, period, keys, prev=f[10])  # with a frame before
            _expect(_delta(*part, geom, period, keys, prev=f[10]), want, want_offs)
            _expect(_undelta(want, want_offs, geom, period, keys, prev=f[10]), *part)


@pytest.mark.parametrize("period", [2, 4])
def test_a_chain_longer_than_any_batch(native, period):
    geom = BAND_GEOMS[0]
    stream, offs = delta_clip(np.random.default_rng(33), geom, 33, 0.5)
    keys = [int(i in (0, 16, 17, 22)) for i in range(33)]
    for k in (None, keys):
        want, want_offs = layers.delta_temporal_frames(stream, offs, period, k)
        got = _delta(stream, offs, geom, period, k)
        _expect(got, want, want_offs)
        back = _undelta(want, want_offs, geom, period, k)
        _expect(back, stream, offs)
        assert got[2] == back[2] == [0] * 33


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", [BAND_GEOMS[1], BAND_GEOMS[2]], ids=_gid)
def test_a_call_cut_at_every_multiple_of_the_period(native, geom, period):
    """The second call's d_prev is input frame cut - period (delta) or the first call's output frame cut - period (undelta)."""
    stream, offs = delta_clip(np.random.default_rng(21), geom, N, 0.3)
    f = frames_of(stream, offs)
    diff, diff_offs = layers.delta_temporal_frames(stream, offs, period, KEYS)
    d = frames_of(diff, diff_offs)
    for cut in range(period, N, period):
        first = _delta(*entropy._join(f[:cut]), geom, period, KEYS[:cut])
        second = _delta(*entropy._join(f[cut:]), geom, period, KEYS[cut:], prev=f[cut - period])
        assert first[0][:first[1][-1]].tobytes() + second[0][:second[1][-1]].tobytes() == diff, cut
        _expect(second, *entropy._join(d[cut:]))
        first = _undelta(*entropy._join(d[:cut]), geom, period, KEYS[:cut])
        before = first[0][first[1][cut - period]:first[1][cut - period + 1]].tobytes()
        assert before == f[cut - period]
        second = _undelta(*entropy._join(d[cut:]), geom, period, KEYS[cut:], prev=before)
        _expect(second, *entropy._join(f[cut:]))
        assert first[2] + second[2] == [0] * N


@pytest.mark.parametrize("period", [2, 4])
def test_the_thinned_stream_through_the_window_call(native, period):
    """A server thins the stored stream with svc_hip_window_levels_frames (d_src, no window): what it sends is the stream of the smaller
    period, and at remaining period 1 the plain undelta call takes it."""
    geom = BAND_GEOMS[2]
    stream, offs = delta_clip(np.random.default_rng(12), geom, N, 0.3)
    diff = _used(_delta(stream, offs, geom, period, KEYS))
    for every in (2, 4):
        if every > period:
            continue
        kept = list(range(0, N, every))
        sent = _window_call(*diff, geom, None, src=kept)
        clip_thin, clip_offs, thin_keys = layers.thin_frames(stream, offs, KEYS, every)
        _expect(sent, *layers.delta_temporal_frames(clip_thin, clip_offs, period // every, thin_keys))
        back = _undelta(*_used(sent), geom, period // every, [int(k) for k in thin_keys])
        _expect(back, clip_thin, clip_offs)
        if period == every:
            _expect(_plain_undelta(*_used(sent), geom, [int(k) for k in thin_keys]), clip_thin, clip_offs)


@pytest.mark.parametrize("period", [2, 4])
def test_a_difference_of_minus_32768(native, period):
    geom = BAND_GEOMS[3]
    w, h, tile, mv = geom
    g, types = geom_dict(*geom), random_types(np.random.default_rng(3), w, h, mv)
    a, b = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    a[0, 0, 0], b[0, 0, 0] = 16384, -16384      # -32768, no wrap
    a[1, 5, 17], b[1, 5, 17] = -32768, 0        # +32768 wraps to -32768
    a[2, h - 1, w - 1], b[2, h - 1, w - 1] = 32767, -1  # -32768
    a[0, 3, 3], b[0, 3, 3] = 7, 7               # 0: the bit is cleared
    fa, fb = layers.write_frame(g, types, a, 4, 16), layers.write_frame(g, types, b, 4, 16)
    stream, offs = entropy._join([fa, fa, fb, fb, fb][:period + 1])  # frame `period` refers to frame 0, frame 2 (period 4) to frame 0 too
    want, want_offs = layers.delta_temporal_frames(stream, offs, period)
    d = frames_of(want, want_offs)
    assert layers._sections(d[period])[4].tolist() == [-32768] * 3 and layers._sections(d[2])[4].tolist() == [-32768] * 3
    _expect(_delta(stream, offs, geom, period), want, want_offs)
    _expect(_undelta(want, want_offs, geom, period), stream, offs)


@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", [BAND_GEOMS[0], BAND_GEOMS[3]], ids=_gid)
def test_a_set_bit_of_level_zero(native, geom, period):
    """Read as 0 in the frame itself and in the frame referred to; the undelta writes the stream with that bit cleared."""
    stream, offs = delta_clip(np.random.default_rng(5), geom, 6)
    f = frames_of(stream, offs)
    for at in (0, 2, 3):  # a layer-0 frame others refer to, a frame of layer 1 (period 4) or 0 (period 2), an odd frame
        bad, clean = with_a_zero_level(f[at])
        assert bad != clean
        with_bit = entropy._join(f[:at] + [bad] + f[at + 1:])
        without = entropy._join(f[:at] + [clean] + f[at + 1:])
        want, want_offs = layers.delta_temporal_frames(*without, period)
        _expect(_delta(*with_bit, geom, period), want, want_offs)
        _expect(_undelta(want, want_offs, geom, period), *without)
    d = frames_of(*layers.delta_temporal_frames(stream, offs, period))
    bad, clean = with_a_zero_level(d[2])  # a difference of 0 under a set bit
    _expect(_undelta(*entropy._join(d[:2] + [bad] + d[3:]), geom, period),
            *layers.undelta_temporal_frames(*entropy._join(d[:2] + [clean] + d[3:]), period))


# ---- 2. statuses: a tree, not a chain -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", [2, 4])
@pytest.mark.parametrize("geom", [HOST12, BAND_GEOMS[2]], ids=_gid)
def test_a_damaged_frame_in_every_layer(native, geom, period):
    """Frames 4, 2 and 5 are of layers 0, 1 (0 at period 2) and 2 (1 at period 2).  The frames that do not hang on the damaged one are
    intact: _expect_frames compares every frame that passes with the frame of the undamaged call."""
    stream, offs = delta_clip(np.random.default_rng(6), geom, N, 0.3)
    f = frames_of(stream, offs)
    for keys in (None, KEYS):
        want, want_offs = layers.delta_temporal_frames(stream, offs, period, keys)
        d = frames_of(want, want_offs)
        for at in (4, 2, 5):
            for what in ("magic", "levels"):
                bad, code = _damaged(stream, offs, at, what)
                own = [code if i == at else 0 for i in range(N)]
                _expect_frames(_delta(bad, offs, geom, period, keys), d, layers.temporal_statuses(own, period, keys, chain=False).tolist())
                bad, code = _damaged(want, want_offs, at, what)
                codes = layers.temporal_statuses(own, period, keys).tolist()
                _expect_frames(_undelta(bad, want_offs, geom, period, keys), f, codes)
                assert codes[at] == code and (at != 5 or sum(c != 0 for c in codes) == 1)  # an odd frame harms no other
    # by hand, period 4 without keys: frame 4 takes every later frame with it in the undelta call, frames 5, 6 and 8 in the delta call
    if period == 4:
        want, want_offs = layers.delta_temporal_frames(stream, offs, 4)
        bad, _ = _damaged(want, want_offs, 4, "magic")
        assert _undelta(bad, want_offs, geom, 4)[2] == [0, 0, 0, 0, 2] + [0x102] * 6
        bad, _ = _damaged(stream, offs, 4, "magic")
        assert _delta(bad, offs, geom, 4)[2] == [0, 0, 0, 0, 2, 0x102, 0x102, 0, 0x102, 0, 0]
    # two damaged frames: a frame's own code comes first
    want, want_offs = layers.delta_temporal_frames(stream, offs, period, KEYS)
    bad, _ = _damaged(want, want_offs, 0, "size")
    worse, own8 = _damaged(bad.tobytes(), want_offs, 8, "levels")
    own = [5] + [0] * 7 + [own8, 0, 0]
    _expect_frames(_undelta(worse, want_offs, geom, period, KEYS), f, layers.temporal_statuses(own, period, KEYS).tolist())


@pytest.mark.parametrize("period", [2, 4])
def test_a_damaged_frame_before(native, period):
    geom = HOST12
    stream, offs = delta_clip(np.random.default_rng(8), geom, N + 1, 0.3)
    f = frames_of(stream, offs)
    rest = entropy._join(f[1:])
    for keys in (None, KEYS):
        d = frames_of(*layers.delta_temporal_frames(*rest, period, keys, prev=f[0]))
        _expect_frames(_delta(*rest, geom, period, keys, prev=f[0]), d, [0] * N)
        _expect_frames(_undelta(*entropy._join(d), geom, period, keys, prev=f[0]), f[1:], [0] * N)
        for what in ("magic", "size", "levels", "stray"):
            bad, code = _damaged(f[0], [0, len(f[0])], 0, what)
            _expect_frames(_delta(*rest, geom, period, keys, prev=bad), d, [0x100 | code] + [0] * (N - 1))
            _expect_frames(_undelta(*entropy._join(d), geom, period, keys, prev=bad), f[1:],
                           layers.temporal_statuses([0] * N, period, keys, prev=code).tolist())
        # less than its bytes is a size that does not match (5), less than a header is out of range (1)
        _expect_frames(_undelta(*entropy._join(d), geom, period, keys, prev=f[0][:-16]), f[1:],
                       layers.temporal_statuses([0] * N, period, keys, prev=5).tolist())
        _expect_frames(_delta(*rest, geom, period, keys, prev=f[0][:48]), d, [0x101] + [0] * (N - 1))


def test_the_statuses_of_a_long_call(native):
    """More layer-0 frames than the status wave has lanes, at either period: 300 frames of one small geometry, damaged at a layer-0 frame
    behind the first 64 of them, at a frame of layer 1 and at an odd frame."""
    geom = BAND_GEOMS[0]
    one, _ = delta_clip(np.random.default_rng(4), geom, 1, 0.2)
    n = 300
    stream, offs = entropy._join([one] * n)
    for period in (2, 4):
        keys = [int(i in (100, 292, 295)) for i in range(n)]
        want, want_offs = layers.delta_temporal_frames(stream, offs, period, keys)
        own = [0] * n
        bad = want
        for at, what in ((period * 70, "magic"), (period * 20 + period // 2, "size"), (period * 72 + 1, "size"), (293, "magic")):
            bad, own[at] = _damaged(bad if isinstance(bad, bytes) else bad.tobytes(), want_offs, at, what)
        got = _undelta(bad, want_offs, geom, period, keys)
        codes = layers.temporal_statuses(own, period, keys).tolist()
        assert got[2] == codes
        assert codes[period * 71] == codes[291] == 0x102 and codes[292] == codes[294] == 0 and codes[period * 72 + 1] == 5
        _expect_frames(got, [one] * n, codes)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", [nat.delta_levels_temporal_frames, nat.undelta_levels_temporal_frames], ids=["delta", "undelta"])
def test_refusals_reach_python(native, fn):
    geom = BAND_GEOMS[3]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    for period in (0, 3, 8):
        with pytest.raises(nat.SvcError, match=f"period {period}") as e:
            fn(frames, offsets, w, h, tile, mv, period, workspace=small)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG
    with pytest.raises(nat.SvcError, match="not divisible"):
        fn(frames, offsets, w + 1, h, tile, mv, 3, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"), workspace=small)
    with pytest.raises(nat.SvcError, match="workspace"):
        fn(frames, offsets, w, h, tile, mv, 2, workspace=small)
    with pytest.raises(nat.SvcError, match="worst case"):
        fn(frames, offsets, w, h, tile, mv, 4, out=torch.empty(nat.levels_max_bytes(1, w, h, tile, mv), dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        fn(frames, offsets, w, h, tile, mv, 2, prev=torch.zeros(80, dtype=torch.uint8, device="cuda")[8:])
    # no frames: nothing is written, whatever the sizes
    out = torch.full((16,), FILL, dtype=torch.uint8, device="cuda")
    none = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    fn(frames[:0], none, w, h, tile, mv, 4, out=out, out_offsets=none, workspace=small)
    torch.cuda.synchronize()
    assert (out == FILL).all() and none.tolist() == [-1]
