"""svc_hip_dct_pack_delta_temporal_auto_frames (csrc/dct_pack.hip, include/svc_hip_temporal.h): the temporal-layer delta stream from
pixels with its key frames chosen by size.  The flags and counts are the numpy statement (layers.delta_level_counts with period,
layers.auto_keys) of the stream svc_hip_dct_pack_levels_frames writes from the same frames; stream and offsets are
svc_hip_dct_pack_delta_temporal_frames' with those flags.  The grid of tests/test_gpu_dct_pack_delta_temporal.py, reduced: its three
geometries, periods 2 and 4, counts 1, 5, 9, 11 and 17; d_forced null, given and all ones; with and without the frame in front; then the
thinning identity for flags, counts and bytes, and the cut at every multiple of the period.

Zero-then-white frames (the call's even frames white) give both outcomes at frames nobody forced, whatever the period: a zero frame holds
no level (a key frame), an even frame's reference is an even frame, white like itself, so it differs in nothing (not a key frame); that
is asserted from the numpy result before the device's is looked at."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack_delta import FILL
from tests.test_gpu_dct_pack_delta_temporal import GEOMS, PERIODS, Clip, _gid, _used

pytestmark = pytest.mark.gpu

COUNTS = (1, 5, 9, 11, 17)
FORCED = ("none", "some", "all")


def _forced(kind, n, seed):
    if kind == "none":
        return None
    if kind == "all":
        return [1] * n
    rng = np.random.default_rng(seed)
    return ((rng.random(n) < 0.3).astype(np.int64) * rng.integers(1, 1 << 31, n)).tolist()  # any value but 0 forces


def auto(c, period, first=0, count=None, has_prev=True, forced=None, every=1, prev_at=None, want_counts=True):
    """Clip.call for the call under test -> (output buffer pre-filled with FILL, offsets, flags and counts pre-filled with -1)."""
    count = c.n - first if count is None else count
    at = 1 + first
    sel = [at + i * every for i in range(count)]
    if every == 1:
        buf, stride, types = c.buf[at * c.stride:], c.stride, c.types[at:at + count].contiguous()
    else:
        buf, stride, types = c.bgr[sel].contiguous(), c.w * c.h * 3, c.types[sel].contiguous()
    pb = pt = None
    if has_prev:
        p = at - period * every if prev_at is None else prev_at
        assert p >= 0
        pb, pt = c.bgr[p].clone(), c.types[p].clone()
    w, h, block, mv = c.w, c.h, c.block, c.mv
    out = torch.full((nat.levels_max_bytes(count, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((count + 1,), -1, dtype=torch.int64, device="cuda")
    keys = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((count, 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(nat.dct_pack_delta_temporal_auto_workspace_bytes(count, w, h, block, mv, period), dtype=torch.uint8, device="cuda")
    k = None if forced is None else torch.tensor(forced, dtype=torch.int32, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_temporal_auto_frames(
        buf.data_ptr(), stride, count, w, h, block, types.data_ptr(), mv[0], mv[1], c.fg, c.bg,
        None if pb is None else pb.data_ptr(), None if pt is None else pt.data_ptr(), None if k is None else k.data_ptr(),
        ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), keys.data_ptr(),
        counts.data_ptr() if want_counts else None, nat._stream(), period))
    return out, offs, keys, counts


def _statement(c, period, has_prev, forced):
    counts = layers.delta_level_counts(c.plain.cpu().numpy(), c.plain_offs.cpu().numpy().astype(np.uint64),
                                       prev=c.prev_plain.cpu().numpy() if has_prev else None, period=period)
    keys = layers.auto_keys(counts, forced, has_prev=has_prev)
    return keys.astype(np.int64).tolist(), counts.astype(np.int64).tolist()


def check_case(geom, period, n, content, types_kind, fg, bg, forced_kind, has_prev, seed, want_counts=True):
    c = Clip(geom, n, content, types_kind, fg, bg, seed)
    forced = _forced(forced_kind, n, seed)
    keys, counts = _statement(c, period, has_prev, forced)
    what = (_gid(geom), period, n, content, types_kind, fg, bg, forced_kind, has_prev)
    got, got_offs, got_keys, got_counts = auto(c, period, has_prev=has_prev, forced=forced, prev_at=0, want_counts=want_counts)
    want, want_offs = c.call(period, has_prev=has_prev, key=keys, prev_at=0)
    torch.cuda.synchronize()
    assert got_keys.cpu().tolist() == keys, what
    assert got_counts.cpu().tolist() == (counts if want_counts else [[-1, -1]] * n), what
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist(), what
    used = offs[-1]
    g = got.cpu().numpy()
    assert g[:used].tobytes() == want[:used].cpu().numpy().tobytes(), what
    assert (g[used:] == FILL).all(), what  # nothing is written past the stream
    for f in range(n):  # each frame holds the smaller count, a forced frame its own
        assert int(g[offs[f]:offs[f] + 64].view(np.uint32)[10]) == counts[f][0 if keys[f] else 1], (what, f)
    return keys, counts


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_keys_counts_and_stream(native, geom, period):
    rows = (("random", "random", 1, 640), ("equal", "checker", 1, 640), ("zero-white", "zero", 1, 640), ("zero-white", "checker", 3, 3))
    outcomes = set()
    for ni, n in enumerate(COUNTS):
        for fi, forced_kind in enumerate(FORCED):
            i = ni * len(FORCED) + fi
            content, types_kind, fg, bg = rows[i % 4]
            keys, _ = check_case(geom, period, n, content, types_kind, fg, bg, forced_kind, bool((i // 4 + fi) % 2), seed=n + geom[1])
            if forced_kind == "none":
                outcomes |= set(keys[1:])
    assert outcomes == {0, 1}  # frames the rule made key frames, and frames it did not
    check_case(geom, period, 9, "random", "random", 1, 640, "some", True, seed=2, want_counts=False)  # d_level_counts null


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_zero_then_white_gives_both_outcomes_at_known_frames(native, geom, period):
    """The call's frame i is white for even i.  An odd frame is zero and holds no level: a key frame.  An even frame's reference is an
    even frame: it differs in nothing and is not a key frame -- but frame 0, which has no reference here."""
    n = 9
    c = Clip(geom, n, "zero-white", "zero", 1, 640, seed=1)
    keys, counts = _statement(c, period, False, None)
    assert keys == [1] + [i % 2 for i in range(1, n)]
    assert all(counts[i][0] == 0 for i in range(1, n, 2)) and all(counts[i][1] == 0 < counts[i][0] for i in range(2, n, 2))
    assert check_case(geom, period, n, "zero-white", "zero", 1, 640, "none", False, seed=1)[0] == keys


@pytest.mark.parametrize("has_prev", [False, True], ids=["noprev", "prev"])
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_flags_counts_and_bytes_thin_as_the_stream_does(native, geom, period, has_prev):
    for n, forced_kind, content, types_kind, fg, bg in ((17, "some", "random", "random", 1, 640), (11, "none", "zero-white", "zero", 1, 640)):
        c = Clip(geom, n + period - 1, content, types_kind, fg, bg, seed=5 + n)  # `period` frames in front of the call
        forced = _forced(forced_kind, n, n)
        out, offs, keys, counts = auto(c, period, period - 1, n, has_prev=has_prev, forced=forced)
        got, o = _used(out, offs)
        keys, counts = keys.cpu().tolist(), counts.cpu().tolist()
        for every in (2, 4):
            if every > period:
                continue
            thin, thin_offs, thin_keys = layers.thin_frames(np.frombuffer(got, np.uint8), np.asarray(o, np.uint64), keys, every)
            m = (n + every - 1) // every
            s_out, s_offs, s_keys, s_counts = auto(c, period // every, period - 1, m, has_prev=has_prev,
                                                   forced=None if forced is None else forced[::every], every=every)
            sub, sub_offs = _used(s_out, s_offs)
            assert s_keys.cpu().tolist() == [int(k) for k in thin_keys] == keys[::every], (n, every)
            assert s_counts.cpu().tolist() == counts[::every], (n, every)
            assert sub_offs == [int(v) for v in thin_offs] and sub == bytes(thin), (n, every)


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_a_cut_at_a_multiple_of_the_period_changes_nothing(native, geom, period):
    n = 17
    for forced_kind, content, types_kind, fg, bg in (("some", "random", "random", 1, 640), ("none", "zero-white", "checker", 3, 3)):
        c = Clip(geom, n, content, types_kind, fg, bg, seed=9)
        forced = _forced(forced_kind, n, 9)
        out, offs, keys, counts = auto(c, period, has_prev=False, forced=forced)
        whole, whole_offs = _used(out, offs)
        keys, counts = keys.cpu().tolist(), counts.cpu().tolist()
        for cut in range(period, n, period):
            a = auto(c, period, 0, cut, has_prev=False, forced=forced[:cut] if forced else None)
            b = auto(c, period, cut, n - cut, has_prev=True, forced=forced[cut:] if forced else None)  # given input frame cut - period
            (ab, ao), (bb, bo) = _used(a[0], a[1]), _used(b[0], b[1])
            assert ab + bb == whole and ao + [ao[-1] + v for v in bo[1:]] == whole_offs, cut
            assert a[2].cpu().tolist() + b[2].cpu().tolist() == keys and a[3].cpu().tolist() + b[3].cpu().tolist() == counts, cut


def test_period_1_is_the_auto_call(native):
    geom = GEOMS[0]
    block, w, h, mv = geom
    n = 11
    c = Clip(geom, n, "random", "random", 1, 640, seed=3)
    forced = _forced("some", n, 3)
    out, offs, keys, counts = auto(c, 1, has_prev=True, forced=forced)
    want = nat.dct_pack_delta_auto_frames(c.bgr[1:].contiguous(), block, c.types[1:].contiguous(), mv, 1, 640, c.bgr[0].clone(),
                                          c.types[0].clone(), forced)
    assert _used(out, offs) == _used(want[0], want[1])
    assert torch.equal(keys, want[2]) and torch.equal(counts, want[3])
    with pytest.raises(nat.SvcError, match="period"):
        nat.dct_pack_delta_temporal_auto_frames(c.bgr[1:].contiguous(), block, c.types[1:].contiguous(), mv, 1, 640, 3)
    assert nat.dct_pack_delta_temporal_auto_workspace_bytes(n, w, h, block, mv, 3) == 0
