"""The seven encoders that make the delta stream, or choose a ladder entry by quality, straight from pixels -- all forms of dct_pack_body
in csrc/dct_pack.hip -- and the reduced temporal decoder, once each on a batch whose stream passes 2^32 bytes and whose frame count is some
forty trips of 256 frames and some fourteen hundred runs of 8: tests/test_gpu_large_streams.py's geometry (256 x 256, 16 x 16 MV blocks,
8 x 8 and 16 x 16 tiles: every kernel here is instantiated per tile size), its preconditions -- a frame straddles 2^32 in the output, two
whole cycles lie above it, n > 256, asserted from the expected offsets before the call -- and its comparison on tests/helpers/periodic.py:
all n + 1 offsets, the stream cycle against cycle, the per-frame outputs (keys, counts, choice, both tables) whole on the device.  n ends
3 frames into a cycle, so the last run of 8 is partial.

The cycle of k = 4 B,G,R frames is this file's own, because that file's four frames are independent and a difference of independent noise
is never smaller than the frame: a random frame A; A with its lower three quarters drawn anew; a synthetic frame S; S with its right three
quarters random.  At steps (1, 1) the rule of svc_hip_dct_pack_delta_auto_frames (layers.auto_keys) differences the second and the fourth
and keys the third; at period 4 it also differences the first, whose reference is the same frame one cycle back.  The region ids of the
second frame are the first's with ids 1 and 7 exchanged in the even MV columns (a tile is predicted across that change at any pair of
steps), the third's are drawn anew (where fg_step != bg_step a tile that changes between id 0 and another is not predicted), the
fourth's are the third's.  All of that is asserted from the numpy statements before any large call.

Expected outputs are the numpy statements' (layers.delta_frames, delta_auto_frames, delta_temporal_frames, delta_budget_frames,
delta_quality_frames, quality_choice, distortion_table) on the plain streams svc_hip_dct_pack_levels_frames writes for the cycle at each
pair of steps.  Each statement runs on THREE cycles: that frames [2k, 3k) equal frames [k, 2k) is asserted (at period 4 a frame refers 1,
2 or 4 frames back; k = 4 is a multiple of it), and the first 2k frames are the prefix -- every statement is causal, a frame's bytes
depend on no later frame.

The long groups (one group of some 11 000 frames, from frame 0 to a key frame above 2^32) have no prefix that gives their choice: the
group's bytes per entry and its budget are summed in Python integers from the periodic rows (pd.range_sums), and the budgets are each
frame's own bytes at entry 1, so that the group fits there exactly.  With either sum taken modulo 2^32 the comparison bytes <= allowed
flips for an entry and the choice changes (pd.truncation_flips, asserted before the call): these cases test the 64-bit sums of
dct_delta_group_select_kernel and dct_delta_quality_select_kernel.

On the input side n * 196 608 bytes of pixels stay below 2^32 (as for svc_hip_dct_pack_levels_frames in that file); the decoder's stream
passes it on the input side.  No case is reduced: the peak is 16.4 GiB (the temporal auto call at period 4, whose cycle is the smallest:
16 955 frames).  The statements of the two group shapes are made once a geometry and shared by the budget and the quality case.

Every case prints that file's line `LARGE <case> seconds=... peak_GiB=... n=... in_max=... out_max=...`."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import periodic as pd
from tests.test_gpu_dct_pack import _content, _types
from tests.test_gpu_large_streams import DEC, DEV, DISPLAY, FIG, GAZE, GEOMS, G8, K, LADDER, _crossed, _decode_case, _figures, _finish  # noqa: F401
from tests.test_gpu_large_streams import _frames_for, _gid, _key_frame, _rows, _rows_case, _tiled, big  # noqa: F401  (big, _figures: fixtures)
from tests.test_gpu_large_streams_temporal import PERIOD, _delta_source
from tests.test_levels_budget_host import frame_floor
from tests.test_window_levels_host import geom_dict

pytestmark = pytest.mark.gpu

OVER, MISSED, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
FINE = (1, 1)
assert LADDER[0] == FINE and LADDER[1][0] != LADDER[1][1] and len(LADDER) == 2
CLIPS = {}


class Clip:
    """The cycle of one geometry, as the 2k-frame prefix on the device, and what the fixed fused pack and the transform make of it."""

    def __init__(self, geom):
        w, h, tile, mv = geom
        seed = 40 + tile[0]
        a, b, c = _content("random", 3, w, h, seed)
        s = _content("synth", 1, w, h, seed + 1)[0]
        a2, s2 = a.clone(), s.clone()
        a2[h // 4:] = b[h // 4:]
        s2[:, w // 4:] = c[:, w // 4:]
        t0, t2 = _types("random", 2, w, h, mv, seed).view(2, h // mv[1], w // mv[0])
        t1 = t0.clone()
        t1[:, 0::2] = torch.where(t0 == 1, 7, torch.where(t0 == 7, 1, t0))[:, 0::2]
        self.geom = geom
        self.bgr = torch.stack([a, a2, s, s2]).repeat(2, 1, 1, 1).contiguous()
        self.types = torch.stack([t0, t1, t2, t2]).reshape(K, -1).repeat(2, 1).contiguous()
        self.made = {}

    def frames(self, pair):
        """The cycle's k plain frames at a pair of steps, as svc_hip_dct_pack_levels_frames writes them."""
        if pair not in self.made:
            w, h, tile, mv = self.geom
            out, offs = nat.dct_pack_levels_frames(self.bgr[:K], tile[0], self.types[:K], mv, *pair)
            torch.cuda.synchronize()
            o = offs.cpu().numpy()
            self.made[pair] = pd.split_frames(out[:int(o[-1])].cpu().numpy(), o)
        return self.made[pair]

    def plain(self, pair, cycles=3):
        return layers._join(self.frames(pair) * cycles)

    def sizes(self, ladder):
        """(k, L): the plain frames' bytes at every entry."""
        return np.array([[len(f) for f in self.frames(tuple(p))] for p in ladder], np.int64).T

    def distortion(self, ladder):
        """(k, L) u64: layers.distortion_table on svc_hip_dct_frames' planes."""
        key = ("D",) + tuple(map(tuple, ladder))
        if key not in self.made:
            w, h, tile, mv = self.geom
            planes = nat.dct_frames(self.bgr[:K], tile[0])
            torch.cuda.synchronize()
            self.made[key] = layers.distortion_table(planes.cpu().numpy(), self.types[:K].cpu().numpy(), geom_dict(*self.geom), ladder)
        return self.made[key]

    def type_changes(self, pair, period=1):
        """Per frame of the period: (MV blocks whose id differs from the reference frame's and that are predicted at `pair`, those that
        are not): delta_frame's rule, a tile is predicted iff both frames code it at one step."""
        t = self.types[:K].cpu().numpy()
        step = np.where(t == 0, pair[1], pair[0])
        out = []
        for f in range(K, 2 * K):
            p = layers.temporal_ref(f, period)
            changed, predicted = t[f % K] != t[p % K], step[f % K] == step[p % K]
            out.append((int((changed & predicted).sum()), int((changed & ~predicted).sum())))
        return out

    def tiled(self, n):
        return _tiled(self.bgr, n), _tiled(self.types, n)


def _clip(geom):
    if geom not in CLIPS:
        CLIPS[geom] = Clip(geom)
    clip = CLIPS[geom]
    # a tile is predicted across a change of id in one frame and not in another (where the pair's steps differ; at (1, 1) every tile is)
    coarse, fine = clip.type_changes(LADDER[1]), clip.type_changes(FINE)
    assert coarse[1][0] > 0 and coarse[1][1] == 0 and coarse[2][1] > 0 and coarse[3] == (0, 0), coarse
    assert fine[2][0] > 0 and all(x[1] == 0 for x in fine), fine
    return clip


def _prefix(data, offs):
    """A statement's stream on three cycles -> its 2k-frame prefix, after the third cycle was found equal to the second."""
    fr = pd.split_frames(data, offs)
    assert len(fr) == 3 * K and fr[2 * K:] == fr[K:2 * K], "the statement's output is not periodic from the second cycle on"
    return layers._join(fr[:2 * K])


def _prefix_rows(rows):
    rows = np.asarray(rows)
    assert rows.shape[0] == 3 * K and (rows[2 * K:] == rows[K:2 * K]).all(), "the statement's rows are not periodic from the second cycle on"
    return np.ascontiguousarray(rows[:2 * K])


def _expect(big, clip, ref, key_cycle):
    """The frame count at which the expected stream crosses, the key frame above 2^32, and the expected stream; the preconditions on the
    output side.  Every large source of the module leaves the device."""
    w, h = clip.geom[:2]
    n = _frames_for(int(ref[1][2 * K]) - int(ref[1][K]))
    r = (n // K - 1) * K
    exp = pd.Periodic(*ref, K, n, (0, r) if key_cycle else (0,))
    FIG["in_max"] = n * h * w * 3
    _crossed("out", exp.offsets)
    assert n % 8 != 0  # the last run is partial
    big.release(keep=())
    return n, r, exp


def _i32(rows):
    """Rows of u32 or u64 values as the signed tensor the call writes."""
    a = np.ascontiguousarray(rows)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).to(DEV)


def _per_frame(values, n, dtype=np.uint32):
    """k values, one per cycle position -> (n,) on the device, repeated with the cycle."""
    return _i32(np.array([int(v) for v in values], dtype)).repeat(-(-n // len(values)))[:n].contiguous()


# ---- 1, 3: the delta stream and its temporal form, key flags given ---------------------------------------------------------------------------

def _delta_case(big, geom, period, flags):
    w, h, tile, mv = geom
    clip = _clip(geom)
    ref = _prefix(*layers.delta_temporal_frames(*clip.plain(FINE), period))
    n, r, exp = _expect(big, clip, ref, flags)
    keys = _key_frame(n, exp.offsets)[1] if flags else None
    bgr, types = clip.tiled(n)
    if period == 1:
        out, got = nat.dct_pack_delta_frames(bgr, tile[0], types, mv, *FINE, key=keys)
    else:
        out, got = nat.dct_pack_delta_temporal_frames(bgr, tile[0], types, mv, *FINE, period, key=keys)
    _finish(f"dct_pack_delta period {period}", out, got, exp)


@pytest.mark.parametrize("flags", [True, False], ids=["keys", "nokeys"])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta(big, geom, flags):
    """Key flags at frame 0 and at the start of the last whole cycle, above 2^32; and no flags at all: one chain through the batch."""
    _delta_case(big, geom, 1, flags)


TEMPORAL = [(GEOMS[0], PERIOD), (GEOMS[1], PERIOD), (G8, 2)]
assert K % PERIOD == 0 and PERIOD == 4  # a restart at a multiple of k is a frame of layer 0


@pytest.mark.parametrize("geom,period", TEMPORAL, ids=lambda v: _gid(v) if isinstance(v, tuple) else f"period{v}")
def test_dct_pack_delta_temporal(big, geom, period):
    """Key flags at frame 0 and at the start of the last whole cycle.  At period 4 the first frame of a cycle is coded against the same
    frame one cycle back, run_first - PERIOD, and holds no level."""
    _delta_case(big, geom, period, True)


# ---- 2, 3: key frames chosen by size ----------------------------------------------------------------------------------------------------------

def _auto_case(big, geom, period, forced):
    w, h, tile, mv = geom
    clip = _clip(geom)
    stream, offs, keys, counts = layers.delta_auto_frames(*clip.plain(FINE), period=period)
    ref, keys, counts = _prefix(stream, offs), _prefix_rows(keys), _prefix_rows(counts)
    free = keys[K:]  # the period: frames nobody forced, each with a reference
    assert free.any() and not free.all(), f"the rule takes one branch only: {keys.tolist()}, {counts.tolist()}"
    assert not free[1] and free[2] and not free[3]
    n, r, exp = _expect(big, clip, ref, forced)
    flags = _key_frame(n, exp.offsets)[1] if forced else None
    bgr, types = clip.tiled(n)
    if period == 1:
        got = nat.dct_pack_delta_auto_frames(bgr, tile[0], types, mv, *FINE, forced=flags)
    else:
        got = nat.dct_pack_delta_temporal_auto_frames(bgr, tile[0], types, mv, *FINE, period, forced=flags)
    _finish(f"dct_pack_delta_auto period {period}", got[0], got[1], exp)
    _rows_case(("key",), n, (_i32(keys.astype(np.uint32)),), (got[2],), (0, r) if forced else (0,))
    _rows_case(("count",), n, (_i32(counts.astype(np.uint32)),), (got[3],))  # no flag enters the counts: frame r has the period's row


@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta_auto(big, geom, forced):
    """No frame forced; and a key frame forced at the start of the last whole cycle, above 2^32."""
    _auto_case(big, geom, 1, forced)


@pytest.mark.parametrize("geom,period", TEMPORAL, ids=lambda v: _gid(v) if isinstance(v, tuple) else f"period{v}")
def test_dct_pack_delta_temporal_auto(big, geom, period):
    _auto_case(big, geom, period, True)


# ---- 4: a distortion target per frame -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [False, True], ids=["nocap", "cap"])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_levels_quality(big, geom, cap):
    """The first frame's target is its D at the second entry, the others' their D at (1, 1): one frame a cycle steps down.  With the cap
    the third frame's budget is its size at the second entry: the cap decides there and the target is missed.  D is about 1e9 at (1, 1)
    and above 2^32 at (4, 16) for every frame of the cycle."""
    w, h, tile, mv = geom
    clip = _clip(geom)
    table, sizes = clip.distortion(LADDER), clip.sizes(LADDER)
    assert (table[:, 1] > table[:, 0]).all() and (table[:, 1] > pd.WRAP).all(), table.tolist()
    targets = [int(table[0, 1])] + [int(table[f, 0]) for f in range(1, K)]
    budgets = None
    if cap:
        assert sizes[2, 1] < sizes[2, 0]
        budgets = [1 << 20, 1 << 20, int(sizes[2, 1]), 1 << 20]
    choice = layers.quality_choice(table, sizes, targets, budgets)
    assert choice.tolist() == ([1, 0, 1 | MISSED, 0] if cap else [1, 0, 0, 0])
    ref = layers._join([clip.frames(LADDER[int(c) & INDEX])[f] for f, c in enumerate(choice)] * 2)
    n, r, exp = _expect(big, clip, ref, False)
    bgr, types = clip.tiled(n)
    out, got, got_choice, got_table = nat.dct_pack_levels_quality_frames(bgr, tile[0], types, mv, LADDER, _per_frame(targets, n, np.uint64),
                                                                        None if budgets is None else _per_frame(budgets, n), distortion=True)
    _finish("dct_pack_levels_quality", out, got, exp)
    _rows_case(("choice", "D"), n, (_i32(np.tile(choice, 2)), _i32(np.tile(table, (2, 1)))), (got_choice, got_table))


# ---- 5, 6: one ladder entry per group of frames -------------------------------------------------------------------------------------------------

def _frame_bytes(counts, geom):
    w, h, tile, mv = geom
    return (frame_floor(w, h, *tile, *mv) + 2 * np.asarray(counts).astype(np.int64) + 15) // 16 * 16


def _cycle_groups(clip):
    """Shape (a): a key flag at every multiple of k, a group a cycle.  -> (the flags of three cycles, the frames' bytes (k, L), budgets by
    cycle position whose sum is the group's bytes at (1, 1) exactly while frame 0's own is its size at the second entry).  Every cycle
    is a group of its own, so the counts come from one cycle; the statements on three cycles must repeat them.  Made once a geometry."""
    if "cycle groups" not in clip.made:
        size = _frame_bytes(layers.delta_ladder_counts([clip.plain(p, 1) for p in LADDER], [1, 0, 0, 0]), clip.geom)
        total = size.sum(axis=0)
        assert total[1] < total[0] and size[0, 1] < size[0, 0]
        budgets = [int(size[0, 1]), int(total[0] - size[0, 1]), 0, 0]
        assert max(budgets) < pd.WRAP and sum(budgets) == total[0]
        assert pd.first_fit([int(size[0, k]) <= budgets[0] for k in range(len(LADDER))]) == 1  # frame 0 weighed alone would step down
        clip.made["cycle groups"] = ([1, 0, 0, 0] * 3, size, budgets)
    return clip.made["cycle groups"]


def _long_group(big, clip):
    """Shape (b): key flags at frame 0 and at the start of the last whole cycle only.  -> (n, r, the expected stream: the delta stream at
    the second entry; the frames' bytes at every entry as periodic rows (2k, L); each frame's own bytes at the second entry, on the
    device: its budget).  The statements' part is made once a geometry."""
    if "long group" not in clip.made:
        keys = [1] + [0] * (3 * K - 1)
        coded = [layers.delta_frames(*clip.plain(p), keys) for p in LADDER]
        # header word 10 of every coded frame: what layers.delta_ladder_counts reads, without differencing the streams again
        counts = np.array([[int(np.frombuffer(f, "<u4", 16)[10]) for f in pd.split_frames(*c)] for c in coded], np.uint32).T
        rows = _prefix_rows(_frame_bytes(counts, clip.geom))
        ref = _prefix(*coded[1])
        assert np.diff(np.asarray(ref[1]).astype(np.int64)).tolist() == rows[:, 1].tolist()
        clip.made["long group"] = (rows, ref)
    rows, ref = clip.made["long group"]
    n, r, exp = _expect(big, clip, ref, True)
    own = _per_frame(rows[K:, 1], n)
    own[:K] = own[r:r + K] = _i32(rows[:K, 1].astype(np.uint32))
    return n, r, exp, rows, own


def _group_sums(rows, n, r):
    """Python integers: the bytes per entry of the group [0, r) and of the group [r, n)."""
    first, second = pd.range_sums(rows, K, 0, r, (0, r)), pd.range_sums(rows, K, r, n, (0, r))
    assert first[1] > pd.WRAP and first[0] > first[1] and second[0] > second[1]
    return first, second


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta_budget_a_group_a_cycle(big, geom):
    """Some 2 900 groups of one cycle each, all with the same budgets by cycle position: every group fits at (1, 1) exactly, though
    frame 0's own budget is its size at the second entry and two frames have none."""
    w, h, tile, mv = geom
    clip = _clip(geom)
    keys, size, budgets = _cycle_groups(clip)
    stream, offs, choice, counts = layers.delta_budget_frames([clip.plain(p) for p in LADDER], keys, budgets * 3)
    assert choice.tolist() == [0] * (3 * K) and (_frame_bytes(counts, geom) == np.tile(size, (3, 1))).all()
    n, r, exp = _expect(big, clip, _prefix(stream, offs), False)
    bgr, types = clip.tiled(n)
    out, got, got_choice, got_counts = nat.dct_pack_delta_budget_frames(bgr, tile[0], types, mv, LADDER, _per_frame(budgets, n),
                                                                        key=_per_frame(keys[:K], n), counts=True)
    _finish("dct_pack_delta_budget", out, got, exp)
    _rows_case(("choice", "count"), n, (_i32(choice[:2 * K]), _i32(_prefix_rows(counts))), (got_choice, got_counts))


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta_budget_one_long_group(big, geom):
    """One group from frame 0 to the key frame above 2^32, one behind it.  Every frame's budget is its own size at the second entry: both
    groups fit there exactly and not at (1, 1).  The first group's bytes and budget are above 2^32: with either sum modulo 2^32 the
    choice would be another."""
    w, h, tile, mv = geom
    clip = _clip(geom)
    n, r, exp, rows, own = _long_group(big, clip)
    first, second = _group_sums(rows, n, r)
    assert first[1] == int(exp.offsets[r]) and second[1] == int(exp.offsets[n] - exp.offsets[r])
    assert pd.truncation_flips(first, first[1]) == 1 and pd.first_fit([t <= second[1] for t in second]) == 1
    keys = _key_frame(n, exp.offsets)[1]
    bgr, types = clip.tiled(n)
    out, got, got_choice = nat.dct_pack_delta_budget_frames(bgr, tile[0], types, mv, LADDER, own, key=keys)
    _finish("dct_pack_delta_budget", out, got, exp)
    assert torch.equal(got_choice, torch.ones(n, dtype=torch.int32, device=DEV)), "choice"


def _quality_rule(met, length):
    """layers.delta_quality_choice on one group, from the entries every frame meets its target at and the comparisons bytes <= allowed."""
    def choose(fits):
        ok = {k for k, v in enumerate(fits) if v}
        if met & ok:
            return max(met & ok)
        return min(ok) | MISSED if ok else (length - 1) | OVER | (0 if length - 1 in met else MISSED)
    return choose


def _branch(met, fits, length):
    """The branch's name, as tests/test_gpu_dct_pack_delta_quality.py counts them (a budget is given)."""
    if met & fits:
        return "capped" if max(met & fits) != max(met) else "met"
    if fits:
        return "fits-missed"
    return "over" if length - 1 in met else "over-missed"


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta_quality_a_group_a_cycle(big, geom):
    """The groups and budgets of the budget case; every frame's target is its own D at (1, 1), which no frame meets at the second entry:
    branch "met" at entry 0.  Both tables are asked for."""
    w, h, tile, mv = geom
    clip = _clip(geom)
    keys, size, budgets = _cycle_groups(clip)
    table = clip.distortion(LADDER)
    assert (table[:, 1] > table[:, 0]).all()
    targets = [int(v) for v in table[:, 0]]
    total = size.sum(axis=0)
    met = {k for k in range(len(LADDER)) if all(int(table[f, k]) <= targets[f] for f in range(K))}
    fits = {k for k in range(len(LADDER)) if int(total[k]) <= sum(budgets)}
    assert met == {0} and fits == {0, 1} and _branch(met, fits, len(LADDER)) == "met"
    stream, offs, choice, counts = layers.delta_quality_frames([clip.plain(p) for p in LADDER], np.tile(table, (3, 1)), keys, targets * 3,
                                                               budgets * 3)
    assert choice.tolist() == [0] * (3 * K) and (_frame_bytes(counts, geom) == np.tile(size, (3, 1))).all()
    n, r, exp = _expect(big, clip, _prefix(stream, offs), False)
    bgr, types = clip.tiled(n)
    out, got, got_choice, got_counts, got_table = nat.dct_pack_delta_quality_frames(
        bgr, tile[0], types, mv, LADDER, _per_frame(targets, n, np.uint64), _per_frame(budgets, n), key=_per_frame(keys[:K], n), counts=True,
        distortion=True)
    _finish("dct_pack_delta_quality", out, got, exp)
    _rows_case(("choice", "count", "D"), n, (_i32(choice[:2 * K]), _i32(_prefix_rows(counts)), _i32(np.tile(table, (2, 1)))),
               (got_choice, got_counts, got_table))


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_dct_pack_delta_quality_one_long_group(big, geom):
    """The groups and budgets of the long budget case.  The first group's targets are each frame's D at (1, 1), met at that entry alone,
    which does not fit: "fits-missed" at the second entry -- and (1, 1) itself with the group's bytes modulo 2^32, the second entry over
    budget with the budget modulo 2^32.  The group behind the key frame has no budget and targets it meets at the second entry: "over".
    Neither table is asked for."""
    w, h, tile, mv = geom
    clip = _clip(geom)
    table = clip.distortion(LADDER)
    assert (table[:, 1] > table[:, 0]).all()
    n, r, exp, rows, own = _long_group(big, clip)
    first, second = _group_sums(rows, n, r)
    rule = _quality_rule({0}, len(LADDER))
    assert pd.truncation_flips(first, first[1], rule) == 1 | MISSED
    assert _branch({0}, {k for k, t in enumerate(first) if t <= first[1]}, len(LADDER)) == "fits-missed"
    assert _branch({0, 1}, {k for k, t in enumerate(second) if t <= 0}, len(LADDER)) == "over"
    targets = _per_frame(table[:, 0], n, np.uint64)
    targets[r:] = _per_frame(table[:, 1], n, np.uint64)[r:]
    own[r:] = 0
    keys = _key_frame(n, exp.offsets)[1]
    bgr, types = clip.tiled(n)
    out, got, got_choice = nat.dct_pack_delta_quality_frames(bgr, tile[0], types, mv, LADDER, targets, own, key=keys)
    _finish("dct_pack_delta_quality", out, got, exp)
    want = torch.full((n,), 1 | MISSED, dtype=torch.int32, device=DEV)
    want[r:] = int(np.array([1 | OVER], np.uint32).view(np.int32)[0])
    assert torch.equal(got_choice, want), "choice"


# ---- 7: the reduced temporal decoder --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_decode_delta_levels_temporal_reduced(big, geom):
    """tests/test_gpu_large_streams_temporal.py's decoder case at reduce 2: period 4, key flags at frame 0 and at the start of the last
    whole cycle, above 2^32 in the stream.  d_last is the band (0, 0, K, K), K = tile / 2, of stored frame 4 * ((n - 1) / 4)."""
    w, h, tile, mv = geom
    reduce = 2
    stored = pd.split_frames(*big.get("svcq", geom).prefix())
    src = _delta_source(big, geom)
    ref = nat.decode_delta_levels_temporal_reduced_frames(*src.prefix_dev(), w, h, tile, mv, PERIOD, *DEC, reduce,
                                                          gaze=_rows(GAZE).astype(np.int32), display=DISPLAY)
    n = _frames_for(src.cycle_bytes)
    restarts = (0, (n // K - 1) * K)
    big.get("svcq", geom).release()
    stream, offs, offs_np = src.take(n, restarts)
    _crossed("in", offs_np)
    _, keys = _key_frame(n, offs_np)
    got = nat.decode_delta_levels_temporal_reduced_frames(stream, offs, w, h, tile, mv, PERIOD, *DEC, reduce, key=keys,
                                                          gaze=pd.repeat_rows(GAZE, n, DEV), display=DISPLAY, want_last=True)
    assert got[0].shape == (n, h // reduce, w // reduce, 3) and ref[0][:K].abs().max().item() > 1  # pictures, not zeros
    _decode_case("decode_delta_levels_temporal_reduced", n, ref, got, reduce, restarts=restarts)
    at = PERIOD * ((n - 1) // PERIOD)
    want = layers.band_frame(stored[at % K], (0, 0, tile[0] // reduce, tile[1] // reduce))
    assert int(got[4].item()) == len(want) and got[3][:len(want)].cpu().numpy().tobytes() == want, "d_last"
    src.release()
