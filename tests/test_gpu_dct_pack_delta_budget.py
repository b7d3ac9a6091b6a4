"""svc_hip_dct_pack_delta_budget_frames (include/svc_hip_delta_budget.h; csrc/dct_pack.hip): the delta stream with one ladder entry per
group of frames, by a byte budget on the group.

The reference is built on the same device from calls this one shares no kernel with: per ladder entry svc_hip_dct_pack_levels_frames, then
svc_hip_delta_levels_frames with the key flags; the frame sizes of those streams give the table of counts, layers.delta_budget_choice and
layers.delta_budget_frames the expected choice and bytes.  Every comparison is exact: offsets (all n + 1), bytes, choice, counts, the fill
past the stream; svc_hip_undelta_levels_frames of the output against the fused pack at each frame's chosen pair; and
svc_hip_decode_delta_levels_frames of the output against svc_hip_decode_levels_frames of that plain stream.  Budgets are made from the
reference table, never from the call under test.  The shapes are those at which the fused body can break (tests/test_gpu_dct_pack.py)."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _strided, _types
from tests.test_levels_budget_host import frame_floor, ladder

pytestmark = pytest.mark.gpu

OVER, INDEX = 0x80000000, 0x7FFFFFFF
LADDER5 = np.array([(1, 1), (1, 3), (3, 3), (3, 640), (640, 640)], np.uint32)  # fg == bg at entries 0, 2 and 4 only
STEPS8 = np.array([(s, s) for s in (1, 2, 3, 4, 6, 8, 12, 16)], np.uint32)
KEYS11 = [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0]  # groups 0-2, 3, 4, 5-8 (starts inside a run, ends in the next), 9-10: a call cut short in a run


def _geometry(w, h, block, mv):
    return dict(frame_w=w, frame_h=h, block_w=block, block_h=block, mv_block_w=mv[0], mv_block_h=mv[1])


def _jitter(n, w, h, seed):
    """Frame 0 random, every later frame frame 0 with -1, 0 or +1 added per pixel and channel (numpy's generator: the same on any host)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3))
    frames = [base] + [np.clip(base + rng.integers(-1, 2, base.shape), 0, 255) for _ in range(n - 1)]
    return torch.from_numpy(np.stack(frames).astype(np.uint8)).cuda()


def _frames(kind, n, w, h, seed):
    if kind == "jitter":
        return _jitter(n, w, h, seed)
    if kind == "equal":
        return _content("random", 1, w, h, seed).expand(n, h, w, 3).contiguous()
    if kind == "white-zero":
        return torch.cat([_content("white", 1, w, h, 0), _content("zero", n - 1, w, h, 0)]).contiguous() if n > 1 else _content("white", 1, w, h, 0)
    if kind == "synth":  # (the synthetic clip needs room for its rectangles: a corner of a larger frame at the smallest shapes)
        return _content("synth", n, max(w, 64), max(h, 32), seed)[:, :h, :w].contiguous()
    return _content("random", n, w, h, seed)


def _call(buf, stride, n, w, h, block, types, mv, lad, keys, budget, table=True, ws=None):
    """The call on buffers with known contents -> (stream pre-filled with FILL, offsets, choice, counts or None)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    choice = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((n, len(lad)), -3, dtype=torch.int32, device="cuda") if table else None
    if ws is None:
        ws = torch.empty(nat.dct_pack_delta_budget_workspace_bytes(n, w, h, block, mv, len(lad)), dtype=torch.uint8, device="cuda")
    arr, k = nat._ladder(lad)
    key = None if keys is None else torch.tensor(keys, dtype=torch.int32, device="cuda")
    b = nat.budget_tensor(budget, n, "cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_budget_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], arr, k,
                                                              None if key is None else key.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.numel(),
                                                              out.data_ptr(), out.numel(), offs.data_ptr(), choice.data_ptr(),
                                                              None if counts is None else counts.data_ptr(), nat._stream()))
    return out, offs, choice, counts


def _host(stream, offs):
    o = offs.cpu().numpy()
    return stream[:int(o[-1])].cpu().numpy().tobytes(), o.astype(np.uint64)


class Reference:
    """What the statement says of a batch, computed once and shared by the runs of a case: per ladder entry the fused pack's plain stream
    and the stored-stream delta call's output with the flags, and from those the table of counts and every entry's frame sizes."""

    def __init__(self, bgr, types, block, mv, lad, keys, extra=0, numpy_bytes=True):
        n, h, w, _ = bgr.shape
        self.bgr, self.types, self.block, self.mv, self.lad, self.keys, self.n, self.w, self.h = bgr, types, block, mv, lad, keys, n, w, h
        self.buf, self.stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
        self.numpy_bytes = numpy_bytes  # small shapes: the bytes from layers.delta_budget_frames; else from the device's delta frames
        self.plain, self.delta = [], []
        for fg, bg in lad:
            p, p_offs = nat.dct_pack_levels_frames(bgr, block, types, mv, int(fg), int(bg))
            d, d_offs, st = nat.delta_levels_frames(p, p_offs, w, h, block, mv, key=keys)
            torch.cuda.synchronize()
            assert st.cpu().tolist() == [0] * n
            self.plain.append(_host(p, p_offs))
            self.delta.append(_host(d, d_offs))
        self.sizes = np.stack([np.diff(o.astype(np.int64)) for _, o in self.delta], axis=1)  # (n, L)
        self.table = np.stack([[int(np.frombuffer(s, "<u4", 16, int(o[f]))[10]) for f in range(n)] for s, o in self.delta], axis=1).astype(np.uint32)
        floor = frame_floor(w, h, block, block, mv[0], mv[1])
        assert (self.sizes == (floor + 2 * self.table.astype(np.int64) + 15) // 16 * 16).all()  # the frame sizes give the table
        self.groups = layers.delta_groups(keys, n)

    def group_bytes(self, g):
        first, end = self.groups[g]
        return self.sizes[first:end].sum(axis=0)

    def frame(self, streams, f, k):
        s, o = streams[k]
        return s[int(o[f]):int(o[f + 1])]

    def budgets_for(self, targets):
        """Per-frame budgets under which group g's smallest fitting entry is targets[g]: entry t fits exactly, every finer entry is over
        (asserted on the reference table); a target of None: a budget of 0 for every frame of the group."""
        budget = np.zeros(self.n, np.int64)
        for (first, end), t in zip(self.groups, targets):
            if t is None:
                continue
            total = self.sizes[first:end].sum(axis=0)
            assert all(total[k] > total[t] for k in range(t)), (first, end, t, total.tolist())
            budget[first:end] = self.sizes[first:end, t]  # each frame its own bytes at t: the group's sum is exact
        return budget

    def check(self, budget, table=True, ws=None):
        """THE shared check -> the choices as u32."""
        n, w, h, block, mv = self.n, self.w, self.h, self.block, self.mv
        got, got_offs, got_choice, got_counts = _call(self.buf, self.stride, n, w, h, block, self.types, mv, self.lad, self.keys, budget, table, ws)
        torch.cuda.synchronize()
        want_choice = layers.delta_budget_choice(self.table, _geometry(w, h, block, mv), self.keys, budget)
        want, want_offs = layers._join([self.frame(self.delta, f, int(c) & INDEX) for f, c in enumerate(want_choice)])
        if self.numpy_bytes:  # once per reference (the statement differences every entry's stream again): it gives these very bytes
            self.numpy_bytes = False
            w2, o2, c2, t2 = layers.delta_budget_frames(self.plain, self.keys, budget)
            assert w2 == want and o2.tolist() == want_offs.tolist() and c2.tolist() == want_choice.tolist() and (t2 == self.table).all()
        choice = got_choice.cpu().numpy().view(np.uint32)
        assert choice.tolist() == want_choice.tolist()
        if table:
            assert got_counts.cpu().numpy().view(np.uint32).tolist() == self.table.tolist()
        assert got_offs.cpu().tolist() == [int(o) for o in want_offs]  # all n + 1 of them
        g, used = got.cpu().numpy(), int(want_offs[-1])
        assert g[:used].tobytes() == want
        assert (g[used:] == FILL).all()  # nothing is written past the stream
        picks = [int(c) & INDEX for c in choice]
        for f in range(n):
            hdr = g[int(want_offs[f]):int(want_offs[f]) + 64].view(np.uint32)
            assert (int(hdr[8]), int(hdr[9])) == tuple(int(v) for v in self.lad[picks[f]]) and hdr[11] == 0 and hdr[10] == self.table[f, picks[f]]
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


def _rotating_targets(ref, shift):
    """A target per group, a different one in neighbouring groups, each the nearest entry at or below (shift + g) % L that the group's own
    sizes allow to be the smallest that fits."""
    out = []
    for g in range(len(ref.groups)):
        total, t = ref.group_bytes(g), (shift + g) % len(ref.lad)
        while any(total[k] <= total[t] for k in range(t)):
            t -= 1
        out.append(t)
    return out


SHAPES = [
    # block, w, h, mv, content, region ids, bytes between frames
    (8, 16, 8, (16, 8), "random", "random", 0),       # one segment column: 7/8 of the only wave idle
    (8, 16, 8, (16, 8), "jitter", "checker", 0),      # the ids flip every frame: no tile is predicted where fg != bg
    (8, 48, 16, MV16, "synth", "random", 0),          # 3 MV blocks: the masks are only 4-byte aligned
    (8, 48, 16, MV16, "equal", "zero", 0),
    (8, 272, 24, (16, 8), "jitter", "random", 48),    # a full wave plus a one-column wave per row; strided frames
    (8, 272, 24, (16, 8), "white-zero", "checker", 0),
    (16, 16, 16, MV16, "jitter", "random", 0),
    (16, 16, 16, MV16, "random", "checker", 0),
    (16, 144, 48, MV16, "synth", "random", 0),        # two full waves plus a one-column wave per row
    (16, 144, 48, MV16, "jitter", "zero", 16),
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_call_equals_the_statement(native, case):
    block, w, h, mv, content, kind, extra = case
    n, seed = len(KEYS11), block + w + h
    ref = Reference(_frames(content, n, w, h, seed), _types(kind, n, w, h, mv, seed), block, mv, LADDER5, KEYS11, extra)
    if content == "equal":  # equal frames leave no difference at any entry (the ids are equal too)
        assert (ref.table[[f for f in range(n) if not KEYS11[f] and f]] == 0).all() and ref.table[0, 0] > 0
    for shift in (0, 2):
        targets = _rotating_targets(ref, shift)
        choice = ref.check(ref.budgets_for(targets), table=shift == 0)
        assert [int(choice[first]) for first, _ in ref.groups] == targets
    # one group over budget, its neighbours not; and a budget nobody feels
    targets = _rotating_targets(ref, 1)
    targets[3] = None
    choice = ref.check(ref.budgets_for(targets))
    first, end = ref.groups[3]
    assert choice[first:end].tolist() == [(len(LADDER5) - 1) | OVER] * (end - first) and not (np.delete(choice, range(first, end)) & OVER).any()
    assert ref.check(0xFFFFFFFF, table=False).tolist() == [0] * n


@pytest.mark.parametrize("lad", [LADDER5, ladder(8)], ids=["fg-equals-bg-changes", "step-ladder-8"])
def test_every_entry_is_chosen_by_some_group_and_neighbours_differ(native, lad):
    # 51 MV blocks a frame, about a third of them background: every entry of either ladder moves a step that thousands of coefficients
    # of every frame feel, so each group's bytes fall strictly along the ladder and every entry can be the smallest that fits
    w, h, mv, n = 272, 24, (16, 8), len(KEYS11)
    ref = Reference(_frames("random", n, w, h, 5), _types("random", n, w, h, mv, 5), 8, mv, lad, KEYS11)
    chosen = set()
    for shift in range(len(lad)):
        want = [(shift + g) % len(lad) for g in range(len(ref.groups))]
        choice = ref.check(ref.budgets_for(want), table=False)  # (budgets_for asserts that the table allows each target)
        picks = [int(choice[first]) for first, _ in ref.groups]
        assert picks == want and len(set(picks)) >= 2  # at least two groups of one call differ in choice
        chosen |= set(picks)
    assert chosen == set(range(len(lad)))


@pytest.mark.parametrize("n,keys", [(17, None), (1, None), (1, [1]), (8, [0] * 8), (9, [0, 1, 1, 1, 1, 1, 1, 1, 1]), (16, [0] * 8 + [1] + [0] * 7)],
                         ids=["17-no-flags", "1", "1-flagged", "8-one-run", "9-groups-of-one", "16-two-runs"])
def test_frame_counts_and_flags(native, n, keys):
    """A group that spans three runs (17 frames, no flags), groups of one frame that follow each other, a call of one frame, groups that
    end with their run."""
    w, h, mv = 48, 16, MV16
    ref = Reference(_frames("jitter", n, w, h, n), _types("random", n, w, h, mv, n), 8, mv, ladder(8), keys)
    assert len(ref.groups) == (1 if keys is None else max(1, sum(keys[1:]) + 1))
    for shift in (1, 6):
        targets = _rotating_targets(ref, shift)
        choice = ref.check(ref.budgets_for(targets))
        assert [int(choice[first]) for first, _ in ref.groups] == targets


@pytest.mark.parametrize("k", [1, 2, 33, 64])
def test_ladder_lengths(native, k):
    w, h, mv, n = 16, 8, (16, 8), 5
    lad = ladder(64)[:k] if k in (2, 33) else ladder(k)
    keys = [0, 0, 1, 0, 0]
    ref = Reference(_frames("jitter", n, w, h, k), _types("random", n, w, h, mv, k), 8, mv, lad, keys)
    for shift in (0, k // 2, k - 1):
        ref.check(ref.budgets_for(_rotating_targets(ref, shift)))
    assert ref.check(0).tolist() == [(k - 1) | OVER] * n  # no frame fits a budget of 0


def test_a_size_that_rises_along_the_ladder(native):
    """Jitter on 16 x 8 at steps 1 .. 16, one group of 9 frames: the group's bytes rise from one entry to the next (the seed was picked on
    the CPU so that the numpy statement shows it; the reference table must show it here).  With the bytes in front of the rise as the
    budget the group fits there and not at the entry after it."""
    w, h, mv, n = 16, 8, (16, 8), 9
    ref = Reference(_jitter(n, w, h, 126), _types("zero", n, w, h, mv, 0), 8, mv, STEPS8, None)
    assert (np.diff(ref.sizes, axis=1) > 0).any(), ref.sizes.tolist()  # some frame's size rises from some entry to the next
    total = ref.group_bytes(0)
    rises = [j for j in range(len(total) - 1) if total[j + 1] > total[j]]
    assert rises, total.tolist()
    j = rises[0]
    budget = [int(total[j])] + [0] * (n - 1)
    want = min(k for k in range(len(total)) if total[k] <= total[j])
    assert want <= j and total[j + 1] > total[j]
    assert ref.check(budget).tolist() == [want] * n
    # one byte less: entry j is over, and so is j + 1; the choice lies behind the rise or nowhere
    later = [k for k in range(len(total)) if total[k] <= total[j] - 16]
    assert ref.check([int(total[j]) - 16] + [0] * (n - 1)).tolist() == [later[0] if later else (len(total) - 1) | OVER] * n


def test_the_group_rule_against_the_per_frame_rule(native):
    """A large key frame followed by small differences, every frame with the same budget: the group fits at the finest entry, while
    svc_hip_dct_pack_levels_budget_frames, which has no differences and weighs every frame alone, has to coarsen."""
    w, h, mv, n = 48, 16, MV16, 6
    bgr, types = _frames("equal", n, w, h, 3), _types("zero", n, w, h, mv, 0)
    lad = ladder(8)
    ref = Reference(bgr, types, 8, mv, lad, None)
    per_frame = int(-(-int(ref.group_bytes(0)[0]) // n))  # the group's bytes at entry 0, shared out
    assert per_frame < ref.sizes[0, 0]  # the key frame alone is over it
    choice = ref.check(per_frame)
    _, _, plain_choice = nat.dct_pack_levels_budget_frames(bgr, 8, types, mv, lad, per_frame)
    torch.cuda.synchronize()
    assert choice.tolist() == [0] * n
    assert plain_choice.cpu().numpy().view(np.uint32).tolist() != choice.tolist() and (plain_choice.cpu().numpy().view(np.uint32) & INDEX).min() > 0


@pytest.mark.parametrize("block", [8, 16])
def test_a_pair_of_1080p_frames(native, block):
    w, h, mv = 1920, 1088, MV16
    lad = np.array([(1, 1), (2, 16), (16, 16), (16, 640)], np.uint32)
    ref = Reference(_frames("synth", 2, w, h, 1080 + block), _types("random", 2, w, h, mv, block), block, mv, lad, None, numpy_bytes=False)
    for shift in (0, 2):
        targets = _rotating_targets(ref, shift)
        assert ref.check(ref.budgets_for(targets), table=shift == 0).tolist() == targets * 2


def test_the_python_entry_and_two_runs(native):
    w, h, mv, n = 272, 24, (16, 8), len(KEYS11)
    bgr, types = _frames("jitter", n, w, h, 9), _types("random", n, w, h, mv, 9)
    key = torch.tensor(KEYS11, dtype=torch.int32, device="cuda")
    a, a_offs, a_ch, a_t = nat.dct_pack_delta_budget_frames(bgr, 8, types, mv, LADDER5, 6000, key=key, counts=True)
    b, b_offs, b_ch = nat.dct_pack_delta_budget_frames(bgr, 8, types, mv, LADDER5, 6000, key=key, out=torch.zeros_like(a))
    torch.cuda.synchronize()
    used = int(a_offs[-1])
    assert torch.equal(a_offs, b_offs) and torch.equal(a_ch, b_ch) and torch.equal(a[:used], b[:used])
    assert a_t.shape == (n, len(LADDER5)) and (a_t[0] > 0).all()


def test_the_delta_call_on_the_same_workspace_afterwards(native):
    """The workspace begins with svc_hip_dct_pack_delta_frames': that call runs on it afterwards and reads nothing the group call left."""
    w, h, mv, n = 272, 24, (16, 8), 5
    bgr, types = _frames("jitter", n, w, h, 4), _types("checker", n, w, h, mv, 4)
    ws = torch.empty(nat.dct_pack_delta_budget_workspace_bytes(n, w, h, 8, mv, 5), dtype=torch.uint8, device="cuda")
    nat.dct_pack_delta_budget_frames(bgr, 8, types, mv, LADDER5, 100, workspace=ws)
    got, got_offs = nat.dct_pack_delta_frames(bgr, 8, types, mv, 3, 17, workspace=ws)[:2]
    want, want_offs = nat.dct_pack_delta_frames(bgr, 8, types, mv, 3, 17)[:2]
    torch.cuda.synchronize()
    used = int(want_offs[-1])
    assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])


def test_refusals_reach_python(native):
    bgr = _content("zero", 1, 64, 64, 0)
    types = _types("zero", 1, 64, 64, MV16, 0)
    with pytest.raises(Exception, match="non-decreasing"):
        nat.dct_pack_delta_budget_frames(bgr, 8, types, MV16, [(2, 640), (1, 640)], 1 << 20)
    with pytest.raises(Exception, match="8x8, 16x16"):
        nat.dct_pack_delta_budget_frames(bgr, 4, types, MV16, [(1, 640)], 1 << 20, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
