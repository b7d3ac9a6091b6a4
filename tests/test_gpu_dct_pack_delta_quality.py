"""svc_hip_dct_pack_delta_quality_frames (include/svc_hip_delta_quality.h; csrc/dct_pack.hip): the delta stream with one ladder entry per
group of frames, by a distortion target on every frame of the group and an optional byte budget on the group.

The reference is built on the same device from calls this one shares no new kernel with: the table of counts by the Reference of
tests/test_gpu_dct_pack_delta_budget.py (per ladder entry svc_hip_dct_pack_levels_frames, then svc_hip_delta_levels_frames with the key
flags), the table of distortions by svc_hip_dct_pack_levels_quality_frames; layers.delta_quality_choice and layers.delta_quality_frames
give the expected choice and bytes.  Every comparison is exact: both tables, offsets (all n + 1), bytes, choice, the fill past the stream;
svc_hip_undelta_levels_frames of the output against the fused pack at each frame's chosen pair; svc_hip_decode_delta_levels_frames of the
output against svc_hip_decode_levels_frames of that plain stream.  Targets and budgets are made from the reference tables, never from
the call under test.  The shapes are those at which the fused body can break (tests/test_gpu_dct_pack.py)."""
import collections

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _strided, _types
from tests.test_gpu_dct_pack_delta_budget import KEYS11, LADDER5, STEPS8, Reference, _frames, _geometry, _jitter
from tests.test_levels_budget_host import ladder

pytestmark = pytest.mark.gpu

OVER, MISSED, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
U64 = 2 ** 64 - 1
BRANCHES = ("capped", "fits-missed", "over", "over-missed", "nothing-met")


def _call(buf, stride, n, w, h, block, types, mv, lad, keys, target, budget, counts=True, distortion=True, ws=None):
    """The call on buffers with known contents -> (stream pre-filled with FILL, offsets, choice, counts or None, distortion or None)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    choice = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ctab = torch.full((n, len(lad)), -3, dtype=torch.int32, device="cuda") if counts else None
    dtab = torch.full((n, len(lad)), -5, dtype=torch.int64, device="cuda") if distortion else None
    if ws is None:
        ws = torch.empty(nat.dct_pack_delta_quality_workspace_bytes(n, w, h, block, mv, len(lad)), dtype=torch.uint8, device="cuda")
    arr, k = nat._ladder(lad)
    key = None if keys is None else torch.tensor(keys, dtype=torch.int32, device="cuda")
    t = nat.target_tensor(target, n, "cuda")
    b = None if budget is None else nat.budget_tensor(budget, n, "cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_quality_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], arr, k,
                                                               None if key is None else key.data_ptr(), t.data_ptr(),
                                                               None if b is None else b.data_ptr(), ws.data_ptr(), ws.numel(),
                                                               out.data_ptr(), out.numel(), offs.data_ptr(), choice.data_ptr(),
                                                               None if ctab is None else ctab.data_ptr(),
                                                               None if dtab is None else dtab.data_ptr(), nat._stream()))
    return out, offs, choice, ctab, dtab


class QualityReference(Reference):
    """The delta-budget Reference -- the table of counts, every entry's plain and delta stream -- with the distortion table of the same
    frames from svc_hip_dct_pack_levels_quality_frames, and the shared check of this call."""

    def __init__(self, bgr, types, block, mv, lad, keys, extra=0, numpy_bytes=True):
        super().__init__(bgr, types, block, mv, lad, keys, extra, numpy_bytes)
        _, _, _, table = nat.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, 0, distortion=True)
        torch.cuda.synchronize()
        self.dist = table.cpu().numpy().view(np.uint64)
        self.seen = collections.Counter()

    def sets(self, g, target, budget):
        """Q and F of group g, from the reference tables."""
        first, end = self.groups[g]
        L = len(self.lad)
        t = np.broadcast_to(np.asarray(target, np.uint64), (self.n,))
        met = {k for k in range(L) if all(int(self.dist[f, k]) <= int(t[f]) for f in range(first, end))}
        if budget is None:
            return met, set(range(L))
        b = np.broadcast_to(np.asarray(budget, np.int64), (self.n,))
        total = self.group_bytes(g)
        return met, {k for k in range(L) if int(total[k]) <= int(b[first:end].sum())}

    def targets_at(self, entries):
        """Per-frame targets under which group g's entry entries[g] is in Q: every frame its own D there."""
        target = np.zeros(self.n, np.uint64)
        for (first, end), t in zip(self.groups, entries):
            target[first:end] = self.dist[first:end, t]
        return target

    def budgets_at(self, entries):
        """Per-frame budgets under which group g's entry entries[g] is in F, exactly: every frame its own bytes there."""
        budget = np.zeros(self.n, np.int64)
        for (first, end), t in zip(self.groups, entries):
            budget[first:end] = self.sizes[first:end, t]
        return budget

    def check(self, target, budget=None, counts=True, distortion=True, ws=None):
        """THE shared check -> the choices as u32.  The branches the groups took are counted in self.seen."""
        n, w, h, block, mv, L = self.n, self.w, self.h, self.block, self.mv, len(self.lad)
        got, got_offs, got_choice, got_counts, got_dist = _call(self.buf, self.stride, n, w, h, block, self.types, mv, self.lad, self.keys,
                                                                target, budget, counts, distortion, ws)
        torch.cuda.synchronize()
        want_choice = layers.delta_quality_choice(self.table, self.dist, _geometry(w, h, block, mv), self.keys, target, budget)
        want, want_offs = layers._join([self.frame(self.delta, f, int(c) & INDEX) for f, c in enumerate(want_choice)])
        if self.numpy_bytes:  # once per reference (the statement differences every entry's stream again): it gives these very bytes
            self.numpy_bytes = False
            w2, o2, c2, t2 = layers.delta_quality_frames(self.plain, self.dist, self.keys, target, budget)
            assert w2 == want and o2.tolist() == want_offs.tolist() and c2.tolist() == want_choice.tolist() and (t2 == self.table).all()
        choice = got_choice.cpu().numpy().view(np.uint32)
        assert choice.tolist() == want_choice.tolist()
        if counts:
            assert got_counts.cpu().numpy().view(np.uint32).tolist() == self.table.tolist()
        if distortion:
            assert got_dist.cpu().numpy().view(np.uint64).tolist() == self.dist.tolist()
        assert got_offs.cpu().tolist() == [int(o) for o in want_offs]  # all n + 1 of them
        g, used = got.cpu().numpy(), int(want_offs[-1])
        assert g[:used].tobytes() == want
        assert (g[used:] == FILL).all()  # nothing is written past the stream
        picks = [int(c) & INDEX for c in choice]
        for f in range(n):
            hdr = g[int(want_offs[f]):int(want_offs[f]) + 64].view(np.uint32)
            assert (int(hdr[8]), int(hdr[9])) == tuple(int(v) for v in self.lad[picks[f]]) and hdr[11] == 0 and hdr[10] == self.table[f, picks[f]]
        for gi, (first, end) in enumerate(self.groups):  # the branch of the rule, from the sets themselves
            met, fits = self.sets(gi, target, budget)
            value = int(choice[first])
            if met & fits:
                assert value == max(met & fits)
                self.seen["capped" if max(met & fits) != max(met) else "met"] += 1
            elif fits:
                assert value == min(fits) | MISSED
                self.seen["nothing-met" if budget is None and not met else "fits-missed"] += 1
            else:
                assert value == (L - 1) | OVER | (0 if L - 1 in met else MISSED)
                self.seen["over" if L - 1 in met else "over-missed"] += 1
        # undone, frame by frame the fused pack at the chosen pair; decoded in one call, the bits of the plain stream's decode
        own, own_offs = layers._join([self.frame(self.plain, f, k) for f, k in enumerate(picks)])
        back, back_offs, st = nat.undelta_levels_frames(got[:used].clone(), got_offs, w, h, block, mv, key=self.keys)
        rec, _, st2, _, _ = nat.decode_delta_levels_frames(got[:used].clone(), got_offs, w, h, block, mv, key=self.keys)
        ref, _, st3 = nat.decode_levels_frames(torch.from_numpy(np.frombuffer(own, np.uint8).copy()).cuda(),
                                               torch.from_numpy(own_offs.astype(np.int64)).cuda(), w, h, block, mv)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == st2.cpu().tolist() == st3.cpu().tolist() == [0] * n
        assert back_offs.cpu().tolist() == [int(o) for o in own_offs] and back[:len(own)].cpu().numpy().tobytes() == own
        assert torch.equal(rec, ref)
        return choice

    def sweep(self):
        """The runs every case gets: a target entry per group that differs between neighbours, alone and under a cap two entries away;
        targets nobody meets; budgets nobody fits; each table with the other pointer NULL, and both NULL."""
        L, G = len(self.lad), len(self.groups)
        for shift in (0, L // 2 + 1):
            entries = [(shift + g) % L for g in range(G)]
            choice = self.check(self.targets_at(entries), None, counts=shift == 0, distortion=shift != 0)
            assert all((int(choice[first]) & INDEX) >= e and not int(choice[first]) & (OVER | MISSED) for (first, _), e in zip(self.groups, entries))
            self.check(self.targets_at(entries), self.budgets_at([(e + 2) % L for e in entries]), counts=shift != 0, distortion=shift == 0)
        self.check(0, None, counts=False, distortion=False)
        self.check(0, self.budgets_at([(g + 1) % L for g in range(G)]))
        self.check(U64, 0, counts=False, distortion=False)
        self.check(self.targets_at([0] * G) - np.minimum(self.targets_at([0] * G), 1).astype(np.uint64), 0)


SHAPES = [
    # block, w, h, mv, content, region ids, bytes between frames
    (8, 16, 8, (16, 8), "jitter", "random", 0),       # one segment column: 7/8 of the only wave idle
    (8, 48, 16, MV16, "synth", "random", 0),          # 3 MV blocks: the masks are only 4-byte aligned
    (8, 272, 24, (16, 8), "jitter", "random", 48),    # a full wave plus a one-column wave per row; strided frames
    (16, 16, 16, MV16, "jitter", "checker", 0),
    (16, 144, 48, MV16, "synth", "random", 16),       # two full waves plus a one-column wave per row; strided frames
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_call_equals_the_statement(native, case):
    block, w, h, mv, content, kind, extra = case
    n, seed = len(KEYS11), block + w + h
    ref = QualityReference(_frames(content, n, w, h, seed), _types(kind, n, w, h, mv, seed), block, mv, LADDER5, KEYS11, extra)
    ref.sweep()
    assert ref.seen["met"] and ref.seen["fits-missed"] and ref.seen["over"] and ref.seen["over-missed"], ref.seen


@pytest.mark.parametrize("kind", ["random", "zero", "checker"])
@pytest.mark.parametrize("content", ["jitter", "equal", "white-zero", "synth"])
@pytest.mark.parametrize("block", [8, 16])
def test_contents_crossed_with_region_ids(native, block, content, kind):
    w, h, mv, n = (48, 16, MV16, len(KEYS11)) if block == 8 else (16, 16, MV16, len(KEYS11))
    seed = len(content) + len(kind)
    ref = QualityReference(_frames(content, n, w, h, seed), _types(kind, n, w, h, mv, seed), block, mv, LADDER5, KEYS11)
    if content == "equal" and kind == "zero":  # equal frames leave no difference at any entry, and every frame has frame 0's distortion
        assert (ref.table[[f for f in range(n) if not KEYS11[f] and f]] == 0).all() and (ref.dist == ref.dist[0]).all()
    ref.sweep()


def test_every_branch_of_the_rule_occurs(native):
    """Counted over the groups of three cases, from Q and F of the reference tables.  'capped' -- max(Q & F) below max(Q) because a
    coarser entry of Q does not fit -- needs a size that RISES along the ladder: jitter on 16 x 8 at steps 1 .. 16, one group of 9
    frames (the seed of tests/test_gpu_dct_pack_delta_budget.py's test of the rise; the reference table must show it here)."""
    seen = collections.Counter()
    w, h, mv, n = 16, 8, (16, 8), 9
    ref = QualityReference(_jitter(n, w, h, 126), _types("zero", n, w, h, mv, 0), 8, mv, STEPS8, None)
    total = ref.group_bytes(0)
    rises = [j for j in range(len(total) - 1) if total[j + 1] > total[j]]
    assert rises, total.tolist()
    j = rises[0]
    target = np.maximum(ref.dist[:, j], ref.dist[:, j + 1])  # entries j and j + 1 meet it in every frame
    budget = [int(total[j])] + [0] * (n - 1)               # entry j fits, entry j + 1 does not
    met, fits = ref.sets(0, target, budget)
    assert j in met and j + 1 in met and j in fits and j + 1 not in fits
    choice = ref.check(target, budget)
    assert int(choice[0]) == max(met & fits) and max(met & fits) < max(met)
    seen += ref.seen
    w, h, mv, n = 272, 24, (16, 8), len(KEYS11)
    ref = QualityReference(_frames("random", n, w, h, 5), _types("random", n, w, h, mv, 5), 8, mv, ladder(8), KEYS11)
    ref.sweep()
    seen += ref.seen
    for b in BRANCHES:
        assert seen[b] > 0, (b, dict(seen))
    assert seen["met"] > 0


@pytest.mark.parametrize("n,keys", [(17, None), (1, None), (11, KEYS11), (9, [0, 1, 1, 1, 1, 1, 1, 1, 1]), (16, [0] * 8 + [1] + [0] * 7)],
                         ids=["17-no-flags", "1", "11-keys", "9-groups-of-one", "16-two-runs"])
def test_frame_counts_and_flags(native, n, keys):
    """A group that spans three runs (17 frames, no flags), a call of one frame, groups that start inside a run of 8 and end in the next
    and a call that ends mid-run (KEYS11), groups of one frame that follow each other, groups that end with their run."""
    w, h, mv = 48, 16, MV16
    ref = QualityReference(_frames("jitter", n, w, h, n), _types("random", n, w, h, mv, n), 8, mv, ladder(8), keys)
    assert len(ref.groups) == (1 if keys is None else max(1, sum(keys[1:]) + 1))
    ref.sweep()


@pytest.mark.parametrize("block", [8, 16])
def test_every_frame_a_key_frame_is_the_per_frame_quality_call(native, block):
    """Choices, flags included, and bytes are svc_hip_dct_pack_levels_quality_frames' own: a key frame's delta is the frame."""
    w, h, mv, n = (272, 24, (16, 8), 11) if block == 8 else (144, 48, MV16, 11)
    bgr, types = _frames("synth", n, w, h, 7), _types("random", n, w, h, mv, 7)
    ref = QualityReference(bgr, types, block, mv, ladder(8), [1] * n)
    assert (np.diff(ref.sizes, axis=1) <= 0).all()  # key frames: the sizes only fall along the ladder
    flags = set()
    for target, budget in ((ref.targets_at([(3 * g) % 8 for g in range(n)]), None),
                           (ref.targets_at([(3 * g) % 8 for g in range(n)]), ref.budgets_at([(5 * g + 1) % 8 for g in range(n)])),
                           (0, ref.budgets_at([g % 8 for g in range(n)])),
                           (ref.targets_at([7 - g % 8 for g in range(n)]), ref.budgets_at([7] * n) - 16)):
        choice = ref.check(target, budget)
        want, want_offs, want_choice = nat.dct_pack_levels_quality_frames(bgr, block, types, mv, ladder(8), target, budget)
        got, got_offs, _, _, _ = _call(bgr, w * h * 3, n, w, h, block, types, mv, ladder(8), [1] * n, target, budget)
        torch.cuda.synchronize()
        assert choice.tolist() == want_choice.cpu().numpy().view(np.uint32).tolist()
        used = int(want_offs[-1])
        assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])
        flags |= {int(c) >> 30 for c in choice}
    assert flags == {0, 1, 2, 3}


@pytest.mark.parametrize("k", [1, 33, 64])
def test_ladder_lengths(native, k):
    """Lane k keeps entry k: 64 entries is the edge."""
    w, h, mv, n = 16, 8, (16, 8), 5
    lad = ladder(64)[:k] if k == 33 else ladder(k)
    ref = QualityReference(_frames("jitter", n, w, h, k), _types("random", n, w, h, mv, k), 8, mv, lad, [0, 0, 1, 0, 0])
    ref.sweep()
    assert ref.check(ref.targets_at([k - 1, k - 1])).tolist() == [k - 1] * n  # the last entry meets its own D: the coarsest of Q


def test_one_frame_alone_misses_the_target(native):
    """A target every frame of the group meets at the last entry but one: that frame's own D there, less one."""
    w, h, mv, n = 48, 16, MV16, 12
    ref = QualityReference(_frames("jitter", n, w, h, 12), _types("zero", n, w, h, mv, 0), 8, mv, STEPS8, None)
    target = ref.dist[:, 7].copy()
    assert ref.check(target, None, counts=False).tolist() == [7] * n
    assert ref.dist[5, 7] > ref.dist[5, :7].max()  # (the frame meets the lowered target at a finer entry)
    target[5] -= 1
    choice = ref.check(target, None, distortion=False)
    met, _ = ref.sets(0, target, None)
    assert 7 not in met and choice.tolist() == [max(met)] * n


@pytest.mark.parametrize("block", [8, 16])
def test_a_pair_of_1080p_frames(native, block):
    w, h, mv = 1920, 1088, MV16
    lad = np.array([(1, 1), (2, 16), (16, 16), (16, 640)], np.uint32)
    ref = QualityReference(_frames("synth", 2, w, h, 1080 + block), _types("random", 2, w, h, mv, block), block, mv, lad, None, numpy_bytes=False)
    assert (ref.check(ref.targets_at([2])) & INDEX).min() >= 2
    ref.check(ref.targets_at([3]), ref.budgets_at([1]), counts=False, distortion=False)


def test_the_python_entry_and_two_runs(native):
    w, h, mv, n = 272, 24, (16, 8), len(KEYS11)
    bgr, types = _frames("jitter", n, w, h, 9), _types("random", n, w, h, mv, 9)
    key = torch.tensor(KEYS11, dtype=torch.int32, device="cuda")
    target = layers.distortion_target(30.0, w, h)
    a, a_offs, a_ch, a_t, a_d = nat.dct_pack_delta_quality_frames(bgr, 8, types, mv, LADDER5, target, 6000, key=key, counts=True, distortion=True)
    b, b_offs, b_ch = nat.dct_pack_delta_quality_frames(bgr, 8, types, mv, LADDER5, target, 6000, key=key, out=torch.zeros_like(a))
    _, _, c_ch, c_d = nat.dct_pack_delta_quality_frames(bgr, 8, types, mv, LADDER5, target, key=key, distortion=True)
    torch.cuda.synchronize()
    used = int(a_offs[-1])
    assert torch.equal(a_offs, b_offs) and torch.equal(a_ch, b_ch) and torch.equal(a[:used], b[:used]) and torch.equal(a_d, c_d)
    assert a_t.shape == a_d.shape == (n, len(LADDER5)) and (a_t[0] > 0).all() and (a_d[:, -1] > 0).all()
    assert not (c_ch.cpu().numpy().view(np.uint32) & OVER).any()  # no cap: nothing is over it


def test_the_delta_calls_on_the_same_workspace_afterwards(native):
    """The workspace begins with svc_hip_dct_pack_delta_budget_frames', which begins with svc_hip_dct_pack_delta_frames': both run on it
    afterwards and read nothing this call left."""
    w, h, mv, n = 272, 24, (16, 8), 5
    bgr, types = _frames("jitter", n, w, h, 4), _types("checker", n, w, h, mv, 4)
    ws = torch.empty(nat.dct_pack_delta_quality_workspace_bytes(n, w, h, 8, mv, 5), dtype=torch.uint8, device="cuda")
    nat.dct_pack_delta_quality_frames(bgr, 8, types, mv, LADDER5, 1 << 40, 100, workspace=ws)
    got, got_offs = nat.dct_pack_delta_frames(bgr, 8, types, mv, 3, 17, workspace=ws)[:2]
    want, want_offs = nat.dct_pack_delta_frames(bgr, 8, types, mv, 3, 17)[:2]
    got_b, got_b_offs, got_b_ch = nat.dct_pack_delta_budget_frames(bgr, 8, types, mv, LADDER5, 3000, workspace=ws)
    want_b, want_b_offs, want_b_ch = nat.dct_pack_delta_budget_frames(bgr, 8, types, mv, LADDER5, 3000)
    torch.cuda.synchronize()
    used = int(want_offs[-1])
    assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])
    used = int(want_b_offs[-1])
    assert torch.equal(got_b_offs, want_b_offs) and torch.equal(got_b_ch, want_b_ch) and torch.equal(got_b[:used], want_b[:used])


def test_refusals_reach_python(native):
    bgr = _content("zero", 1, 64, 64, 0)
    types = _types("zero", 1, 64, 64, MV16, 0)
    with pytest.raises(Exception, match="non-decreasing"):
        nat.dct_pack_delta_quality_frames(bgr, 8, types, MV16, [(2, 640), (1, 640)], 1 << 20)
    with pytest.raises(Exception, match="8x8, 16x16"):
        nat.dct_pack_delta_quality_frames(bgr, 4, types, MV16, [(1, 640)], 1 << 20, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
