"""tests/helpers/periodic.py on the host, at a tiny geometry: what tests/test_gpu_large_streams.py expects of a call on a periodic batch,
taken from the numpy statement on the 2k-frame prefix, is what the statement gives for the whole concatenation; and its comparison
catches a stream whose frame offsets were taken modulo a power of two, with a small modulus standing in for 2^32.  No project code is
altered for this: the wrapped "kernel output" is made here, in numpy."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from tests.helpers import periodic as pd
from tests.test_window_levels_host import geom_dict, random_levels, random_types

GEOM = (16, 16, (8, 8), (16, 16))
K = 4
WINDOWS = [(0, 0, 16, 16), (8, 0, 8, 16), (0, 0, 16, 16), (0, 8, 16, 8)]  # whole-frame and partial windows alternating by cycle position


def _cycle(seed=7):
    """Two different frames at density 1.0, one at 0.3, one without a level."""
    rng = np.random.default_rng(seed)
    w, h, tile, mv = GEOM
    frames = [layers.write_frame(geom_dict(*GEOM), random_types(rng, w, h, mv), random_levels(rng, w, h, d), 1, 1) for d in (1.0, 1.0, 0.3, 0.0)]
    return frames, np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)


def _batch(frames, cyc, n):
    """The plain concatenation of n frames of the cycle, as numpy bytes, and the helper's offsets for it."""
    offs = pd.offsets(cyc, n)
    data = b"".join(frames[f % K] for f in range(n))
    assert len(data) == offs[-1] and [len(frames[f % K]) for f in range(n)] == np.diff(offs).tolist()
    return np.frombuffer(data, np.uint8), offs.astype(np.uint64)


def _calls(n, key_at):
    keys = np.zeros(n, np.int32)
    keys[[0, key_at]] = 1
    return {
        "window": lambda d, o: layers.window_frames(d, o, np.array([WINDOWS[f % K] for f in range(len(o) - 1)], np.uint32)),
        "entropy": lambda d, o: entropy.encode_frames(d, o),
        "delta": lambda d, o: layers.delta_frames(d, o, keys[:len(o) - 1]),
    }


@pytest.mark.parametrize("call", ["window", "entropy", "delta"])
@pytest.mark.parametrize("n", [4 * 7, 4 * 7 + 3, 4 * 2 + 1])
def test_period_of_the_prefix_is_the_statement_on_the_whole_batch(call, n):
    frames, cyc = _cycle()
    key_at = 4 * (n // 4 - 1) if n > 12 else 0
    fn = _calls(n, key_at)[call]
    data, offs = _batch(frames, cyc, n)
    want, want_offs = fn(data, offs)
    exp = pd.Periodic(*fn(*_batch(frames, cyc, 2 * K)), K, n, restarts=(0, key_at) if call == "delta" else (0,))
    assert exp.offsets.tolist() == [int(v) for v in want_offs]
    got = torch.from_numpy(np.frombuffer(want, np.uint8).copy())
    assert pd.mismatch(got, torch.from_numpy(np.asarray(want_offs).astype(np.int64)), exp) is None
    assert exp.materialize("cpu").numpy().tobytes() == want
    spoiled = got.clone()
    at = int(exp.offsets[n - 1]) + 3  # one byte of the last frame, in the partial cycle where there is one
    spoiled[at] ^= 1
    assert f"the first frame {n - 1} at byte" in pd.mismatch(spoiled, want_offs, exp)
    assert "offsets[2] = " in pd.mismatch(got, np.asarray(want_offs).astype(np.int64) + (np.arange(n + 1) >= 2), exp)


def test_offsets_and_the_preconditions():
    frames, cyc = _cycle()
    wrap = 1 << 19  # the fewest frames to cross it are more than 256 here
    n = pd.frames_to_cross(cyc[-1], K, wrap)
    offs = pd.offsets(cyc, n)
    assert offs.dtype == np.int64 and offs.tolist() == np.concatenate([[0], np.cumsum([len(frames[f % K]) for f in range(n)])]).tolist()
    s = pd.crossing(offs, K, wrap)
    assert n > 256 and offs[s] < wrap < offs[s + 1]
    with pytest.raises(AssertionError, match="two whole cycles"):
        pd.crossing(offs[:-K], K, wrap)
    with pytest.raises(AssertionError, match="straddles"):
        pd.crossing(offs, K, 1 << 40)
    with pytest.raises(AssertionError, match="straddles"):
        pd.crossing(offs, K, int(offs[s]))  # a frame that starts at the point does not straddle it
    with pytest.raises(AssertionError, match="one trip"):
        pd.crossing(offs[:257], K, 1 << 16)


def _wrapped(exp, wrap, fill=0xA5):
    """What a kernel that keeps its frame offsets in too few bits leaves: every frame's bytes, right in themselves, at its offset modulo
    `wrap`; the n + 1 offsets right, as a 64-bit scan gives them."""
    out = np.full(int(exp.offsets[-1]), fill, np.uint8)
    for f in range(exp.n):
        fr = (exp.head if exp.is_head[f // K] else exp.period)[f % K]
        a = int(exp.offsets[f]) % wrap
        out[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    return torch.from_numpy(out)


@pytest.mark.parametrize("call", ["window", "entropy"])
def test_offsets_taken_modulo_the_wrap_point_are_caught(call):
    frames, cyc = _cycle()
    wrap = 1 << 16
    fn = _calls(8, 0)[call]
    prefix = fn(*_batch(frames, cyc, 2 * K))
    n = pd.frames_to_cross(min(cyc[-1], pd.Periodic(*prefix, K, 2 * K).cycle_bytes()), K, wrap, extra=3)
    n = max(n, 257 + 3)
    exp = pd.Periodic(*prefix, K, n)
    pd.crossing(pd.offsets(cyc, n), K, wrap)
    pd.crossing(exp.offsets, K, wrap)
    data, offs = _batch(frames, cyc, n)
    right, right_offs = fn(data, offs)
    assert pd.mismatch(torch.from_numpy(np.frombuffer(right, np.uint8).copy()), right_offs, exp, wrap) is None
    above = int(np.flatnonzero(exp.offsets[:-1] >= wrap)[0])
    assert exp.offsets[above - 1] < wrap <= exp.offsets[above]
    report = pd.mismatch(_wrapped(exp, wrap), exp.offsets, exp, wrap)
    assert report is not None and f"frame {above}, the first to start at or above {wrap}, differs" in report, report
    assert f"{n - above} of the {n - above} frames from it on differ" in report, report


def _entry_cycle(seed, densities):
    """One cycle at the given level densities: the plain frames of one ladder entry (a coarser entry holds fewer levels)."""
    rng = np.random.default_rng(seed)
    w, h, tile, mv = GEOM
    types = [random_types(rng, w, h, mv) for _ in densities]
    frames = [layers.write_frame(geom_dict(*GEOM), t, random_levels(rng, w, h, d), 1, 1) for t, d in zip(types, densities)]
    return frames, np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)


def test_sums_of_a_periodic_table_and_the_truncation_precondition():
    """pd.range_sums on the prefix's rows is the sum over the whole batch's rows, for a group that runs from frame 0 to a key frame in the
    last whole cycle and for the group behind it; and the precondition of the long-group cases of tests/test_gpu_large_streams_encoders.py
    -- a budget of exactly the group's bytes at entry 1 changes the choice once either sum is taken modulo the wrap point -- holds at a
    modulus of 2^16 and fails where nothing is truncated."""
    n = 4 * 40 + 3
    key_at = 4 * (n // 4 - 1)
    keys = np.zeros(n, np.int32)
    keys[[0, key_at]] = 1
    entries = [_entry_cycle(21, (1.0, 1.0, 0.5, 0.2)), _entry_cycle(22, (0.3, 0.3, 0.1, 0.2))]
    floor = 64 + 4 * 1 + 8 * 3 * 4

    def sizes(count, key):
        counts = layers.delta_ladder_counts([_batch(fr, cyc, count) for fr, cyc in entries], key)
        return (floor + 2 * counts.astype(np.int64) + 15) // 16 * 16
    whole, rows = sizes(n, keys), sizes(2 * K, [1] + [0] * (2 * K - 1))
    restarts = (0, key_at)
    for a, b in ((0, key_at), (key_at, n), (0, n), (5, 4 * 9 + 2), (key_at - 1, key_at + 2), (7, 7)):
        assert pd.range_sums(rows, K, a, b, restarts) == [int(v) for v in whole[a:b].sum(axis=0)], (a, b)
    assert pd.range_sums(rows, K, 0, n) != pd.range_sums(rows, K, 0, n, restarts)  # the head's key frame counts where a cycle restarts
    wrap = 1 << 16
    totals = pd.range_sums(rows, K, 0, key_at, restarts)
    assert totals[0] > totals[1] > wrap
    allowed = totals[1]  # every frame its own bytes at entry 1
    assert pd.truncation_flips(totals, allowed, wrap=wrap) == 1
    budgets = whole[:, 1]
    geometry = dict(zip(layers.GEOMETRY, (GEOM[0], GEOM[1], *GEOM[2], *GEOM[3])))
    assert layers.delta_budget_choice((whole - floor) // 2, geometry, keys, budgets)[:key_at].tolist() == [1] * key_at
    with pytest.raises(AssertionError, match="every comparison stays"):
        pd.truncation_flips(totals, allowed, wrap=1 << 40)
    with pytest.raises(AssertionError, match="the choice stays"):  # a rule that does not look at the comparisons
        pd.truncation_flips(totals, allowed, choose=lambda fits: 0, wrap=wrap)
