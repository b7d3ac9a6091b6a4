"""svc_hip_dct_pack_levels_quality_frames (include/svc_hip_quality.h; csrc/dct_pack.hip): a distortion target inside the fused transform.
The table of squared errors equals layers.distortion_table on svc_hip_dct_frames' planes of the same device, exactly; the choices equal
layers.quality_choice on that table and the two-call route's own frame sizes; each frame is, byte for byte, what
svc_hip_dct_pack_levels_frames writes with its chosen pair.  Every comparison is exact but the scale check, which is a condition against a
wrong unit, not a precision pin.  The shapes are those of tests/test_gpu_dct_pack_budget.py."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers, levels
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _strided, _two_calls, _types
from tests.test_gpu_dct_pack_budget import SHAPES8, SHAPES16, _mixed, _planes, _sizes
from tests.test_levels_budget_host import frame_floor, ladder

pytestmark = pytest.mark.gpu

OVER, UNMET, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
TOP = 2 ** 64 - 1
LADDER32 = levels.step_ladder(1, 256, 4, 640, 10, 24)


def _geometry(w, h, block, mv):
    return dict(frame_w=w, frame_h=h, block_w=block, block_h=block, mv_block_w=mv[0], mv_block_h=mv[1])


def _quality(buf, stride, n, w, h, block, types, mv, lad, target, budget=None, table=True, ws=None):
    """The call on buffers with known contents -> (stream pre-filled with FILL, offsets, choice, table or None)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    choice = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((n, len(lad)), -3, dtype=torch.int64, device="cuda") if table else None
    if ws is None:
        ws = torch.empty(nat.dct_pack_levels_quality_workspace_bytes(n, w, h, block, mv, len(lad)), dtype=torch.uint8, device="cuda")
    arr, k = nat._ladder(lad)
    t = nat.target_tensor(target, n, "cuda")
    b = None if budget is None else nat.budget_tensor(budget, n, "cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_quality_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], arr, k,
                                                                t.data_ptr(), None if b is None else b.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                out.data_ptr(), out.numel(), offs.data_ptr(), choice.data_ptr(),
                                                                None if dist is None else dist.data_ptr(), nat._stream()))
    return out, offs, choice, dist


class Reference:
    """What the numpy statement says of a batch, computed once and shared by the runs of a case: the table from svc_hip_dct_frames'
    planes and every entry's frame size."""

    def __init__(self, bgr, types, block, mv, lad, extra=0):
        n, h, w, _ = bgr.shape
        self.bgr, self.types, self.block, self.mv, self.lad, self.n, self.w, self.h = bgr, types, block, mv, lad, n, w, h
        self.buf, self.stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
        planes = _planes(self.buf, self.stride, n, w, h, block)
        torch.cuda.synchronize()
        self.table = layers.distortion_table(planes.cpu().numpy(), types.cpu().numpy(), _geometry(w, h, block, mv), lad)
        self.sizes = np.array(_sizes(planes, types, block, mv, lad), np.int64)
        self.fixed = {}  # (frame, entry) -> the fixed fused call's bytes

    def frame(self, f, k):
        if (f, k) not in self.fixed:
            fg, bg = (int(v) for v in self.lad[k])
            one, one_offs = nat.dct_pack_levels_frames(self.bgr[f:f + 1].contiguous(), self.block, self.types[f:f + 1].contiguous(), self.mv, fg, bg)
            torch.cuda.synchronize()
            self.fixed[(f, k)] = one[:int(one_offs[-1])].cpu().numpy().tobytes()
        return self.fixed[(f, k)]

    def check(self, target, budget=None, table=True, ws=None):
        """THE shared check: the table, the choices, all offsets, each frame's bytes, the fill past offsets[n].  -> the choices as u32."""
        got, got_offs, got_choice, got_table = _quality(self.buf, self.stride, self.n, self.w, self.h, self.block, self.types, self.mv, self.lad,
                                                        target, budget, table, ws)
        torch.cuda.synchronize()
        if table:
            assert got_table.cpu().numpy().view(np.uint64).tolist() == self.table.tolist()
        want = layers.quality_choice(self.table, self.sizes, target, budget)
        choice = got_choice.cpu().numpy().view(np.uint32)
        assert choice.tolist() == want.tolist()
        offs, g, at = got_offs.cpu().tolist(), got.cpu().numpy(), 0
        for f in range(self.n):
            ref = self.frame(f, int(choice[f]) & INDEX)
            assert offs[f] == at and g[at:at + len(ref)].tobytes() == ref, f
            assert len(ref) == self.sizes[f, int(choice[f]) & INDEX]
            at += len(ref)
        assert offs[self.n] == at  # all n + 1 of them
        assert (g[at:] == FILL).all()  # nothing is written past the stream
        return choice


def _shape_case(block, shape, k):
    w, h, mv, types_kind, extra = shape
    seed = w + h + k + block
    bgr = _mixed(3, w, h, seed)  # a random frame, a synthetic frame, a zero frame
    types = _types(types_kind, 3, w, h, mv, seed)
    lad = ladder(k)
    ref = Reference(bgr, types, block, mv, lad, extra)
    d = ref.table
    assert (d[2] == 0).all() and (k == 1 or d[0, 0] < d[0, k - 1])
    ka, kb = k // 2, (2 * k) // 3
    # targets at D_k exactly (met by k), one below D_k (not met by k), and 0 on the zero frame (met by all: the last entry); no cap
    choice = ref.check([int(d[0, ka]), max(int(d[1, kb]), 1) - 1, 0])
    assert int(choice[0]) & INDEX >= ka and not choice[0] & UNMET and choice[2] == k - 1
    assert d[1, int(choice[1]) & INDEX] < max(int(d[1, kb]), 1) or choice[1] & UNMET
    # 0 on frames that are not zero (no entry meets it unless its error is 0) and 2^64 - 1 (every entry meets it)
    choice = ref.check([0, TOP, TOP])
    assert choice[1] == k - 1 and choice[2] == k - 1 and (d[0, 0] == 0 or choice[0] == UNMET)
    # the cap, three regimes, budgets from the two-call route's own sizes, without the table: the random frame's cap asks for an entry
    # finer than the target does (the target decides), the synthetic frame's for a coarser one (the cap decides and the target is missed),
    # the zero frame's is below the frame's floor (over budget)
    floor = frame_floor(w, h, block, block, mv[0], mv[1])
    shrink = max([j for j in range(1, k) if ref.sizes[0, j] < ref.sizes[0, j - 1]], default=0)
    budget = [int(ref.sizes[0, shrink]), int(ref.sizes[1, k // 2]) - 16, floor - 16]
    choice = ref.check([TOP, 0, 0], budget, table=False)
    assert choice[0] == k - 1 and choice[2] == (k - 1) | OVER
    assert int(choice[1]) & INDEX >= min(k // 2 + 1, k - 1) or ref.sizes[1, k // 2] == ref.sizes[1, -1]
    # a cap that no frame feels, and the table with a cap
    assert ref.check([int(d[0, ka]), TOP, 0], 0xFFFFFFFF).tolist() == ref.check([int(d[0, ka]), TOP, 0]).tolist()


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("shape", SHAPES8, ids=lambda c: "-".join(str(x) for x in c))
def test_quality_8x8_equals_the_statement(native, shape, k):
    _shape_case(8, shape, k)


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("shape", SHAPES16, ids=lambda c: "-".join(str(x) for x in c))
def test_quality_16x16_equals_the_statement(native, shape, k):
    _shape_case(16, shape, k)


@pytest.mark.parametrize("block", [8, 16])
def test_one_1080p_frame(native, block):
    w, h, mv = 1920, 1088, MV16
    bgr = _content("synth", 1, w, h, 1080 + block)
    types = _types("random", 1, w, h, mv, block)
    lad = ladder(8)  # (the numpy statement takes a second or so per entry at this size)
    ref = Reference(bgr, types, block, mv, lad)
    choice = ref.check([layers.distortion_target(40.0, w, h)])
    pick = int(choice[0]) & INDEX
    print(f"1080p {block}x{block}: 40 dB -> entry {pick} {lad[pick].tolist()}, {layers.distortion_psnr(ref.table[0, pick], w, h):.2f} dB, "
          f"{ref.sizes[0, pick]} B")
    assert choice[0] & UNMET or layers.distortion_psnr(ref.table[0, pick], w, h) >= 40.0


def test_a_table_derived_by_hand(native):
    """Flat frames of value 1 at 8x8: every tile's DC is 8.0f and every AC is 0.  Per tile and plane, x = 8 - q s: step 1 leaves 0; step 3,
    q = 3, x = -1, e = 256; step 5, q = 2, x = -2, e = 512; step 16, the tie 8 / 16 rounds away from zero, q = 1, x = -8, e = 2048; step
    17, q = 0, x = 8, e = 2048: a plateau between the last two entries, of which the rule takes the later."""
    w, h, mv = 48, 16, MV16
    per = 3 * (w // 8) * (h // 8)
    row = [0, 65536 * per, 262144 * per, 4194304 * per, 4194304 * per]
    lad = np.array([[1, 1], [3, 3], [5, 5], [16, 16], [17, 17]], np.uint32)
    targets = [0, row[1] - 1, row[1], row[2] - 1, row[2], row[3] - 1, row[3], TOP]
    want = [0, 0, 1, 1, 2, 2, 4, 4]
    n = len(targets)
    bgr = torch.ones((n, h, w, 3), dtype=torch.uint8, device="cuda")
    types = _types("random", n, w, h, mv, 1)
    ref = Reference(bgr, types, 8, mv, lad)
    assert ref.table.tolist() == [row] * n
    assert ref.check(targets).tolist() == want
    out, offs, choice, table = nat.dct_pack_levels_quality_frames(bgr, 8, types, mv, lad, targets, distortion=True)  # the Python entry
    torch.cuda.synchronize()
    assert choice.tolist() == want and table.tolist() == [row] * n
    hdr = out.cpu().numpy()[int(offs[6]):int(offs[6]) + 64].view(np.uint32)
    assert (int(hdr[8]), int(hdr[9]), int(hdr[10])) == (17, 17, 0)  # the coarser entry of the plateau: no level


def test_the_largest_entry_that_meets_not_the_one_before_the_first_failure(native):
    """A flat frame of 255: D is not monotone along the 32-entry ladder (the DC's remainder falls and rises with the step)."""
    w, h, mv = 48, 16, MV16
    bgr = torch.full((1, h, w, 3), 255, dtype=torch.uint8, device="cuda")
    types = _types("random", 1, w, h, mv, 2)
    ref = Reference(bgr, types, 8, mv, LADDER32)
    d = [int(v) for v in ref.table[0]]
    differ = []
    for t in sorted(set(d)):
        largest = max(k for k in range(len(d)) if d[k] <= t)
        first_failure = next((k for k in range(len(d)) if d[k] > t), len(d)) - 1
        if first_failure >= 0 and largest != first_failure:
            differ.append((t, largest, first_failure))
    assert differ, d  # the two rules differ on this frame: the case tests what it says
    for t, largest, first_failure in (differ[0], differ[-1]):
        assert ref.check([t]).tolist() == [largest] != [first_failure]


@pytest.mark.parametrize("block", [8, 16])
def test_the_scale_against_the_decoded_picture(native, block):
    """D[choice] / 65536 within 1 % of the squared error of svc_hip_decode_levels_frames' f32 reconstruction against the source: the
    condition of tests/test_quality_host.py's Parseval test (2.4e-5 at worst there; a missing plane is 33 %).  Pixels from 32 .. 223, so
    the reconstruction is nowhere near a clip."""
    w, h, mv = 64, 48, MV16
    g = torch.Generator().manual_seed(block)
    bgr = torch.randint(32, 224, (2, h, w, 3), dtype=torch.uint8, generator=g).cuda()
    types = _types("random", 2, w, h, mv, block)
    lad = ladder(8)
    targets = [layers.distortion_target(38.0, w, h), layers.distortion_target(24.0, w, h)]
    out, offs, choice, table = nat.dct_pack_levels_quality_frames(bgr, block, types, mv, lad, targets, distortion=True)
    torch.cuda.synchronize()
    picks = [int(c) & INDEX for c in choice.cpu().numpy().view(np.uint32)]
    for f, pick in enumerate(picks):
        fg, bg = (int(v) for v in lad[pick])
        lo, hi = int(offs[f]), int(offs[f + 1])
        rec, _, status = nat.decode_levels_frames(out[lo:hi].clone(), torch.tensor([0, hi - lo], device="cuda"), w, h, block, mv, fg, bg)
        torch.cuda.synchronize()
        assert status.tolist() == [0]
        sse = float(((rec[0].double() - bgr[f].double()) ** 2).sum())
        got = int(table[f, pick]) / 65536.0
        print(f"block {block} frame {f} entry {pick} ({fg}, {bg}): D / 65536 = {got:.1f}, decoded SSE = {sse:.1f}, relative {abs(got - sse) / max(sse, 1):.2e}")
        assert sse > 0 and abs(got - sse) <= 0.01 * sse, (f, pick, got, sse)


@pytest.mark.parametrize("block", [8, 16])
def test_two_runs_give_the_same_bytes(native, block):
    w, h, n = 272, 48, 3
    bgr = _mixed(n, w, h, 9)
    types = _types("random", n, w, h, MV16, 9)
    lad = ladder(8)
    target = [layers.distortion_target(db, w, h) for db in (45.0, 30.0, 50.0)]
    a, a_offs, a_ch, a_t = nat.dct_pack_levels_quality_frames(bgr, block, types, MV16, lad, target, 4000, distortion=True)
    b, b_offs, b_ch, b_t = nat.dct_pack_levels_quality_frames(bgr, block, types, MV16, lad, target, 4000, out=torch.zeros_like(a), distortion=True)
    torch.cuda.synchronize()
    used = int(a_offs[-1])
    assert torch.equal(a_offs, b_offs) and torch.equal(a_ch, b_ch) and torch.equal(a_t, b_t) and torch.equal(a[:used], b[:used])


@pytest.mark.parametrize("block", [8, 16])
def test_the_fixed_and_the_budgeted_call_on_the_same_workspace_afterwards(native, block):
    """The quality call leaves per-frame steps, counts and sums in its workspace, which starts with the budgeted call's and the fixed
    call's: both run on it afterwards and read none of it."""
    w, h, n = 272, 48, 3
    bgr = _mixed(n, w, h, 21)
    types = _types("checker", n, w, h, MV16, 21)
    lad = ladder(8)
    ws = torch.empty(nat.dct_pack_levels_quality_workspace_bytes(n, w, h, block, MV16, len(lad)), dtype=torch.uint8, device="cuda")
    _, _, choice = nat.dct_pack_levels_quality_frames(bgr, block, types, MV16, lad, TOP, workspace=ws)  # every entry meets: the last pair
    got, got_offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17, workspace=ws)
    _, want, want_offs = _two_calls(bgr, w * h * 3, n, w, h, block, types, MV16, 3, 17)
    bud, bud_offs, bud_choice = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, 3000, workspace=ws)
    ref, ref_offs, ref_choice = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, 3000)
    torch.cuda.synchronize()
    assert choice.tolist() == [len(lad) - 1] * n
    used = int(want_offs[-1])
    assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])
    used = int(ref_offs[-1])
    assert torch.equal(bud_offs, ref_offs) and torch.equal(bud_choice, ref_choice) and torch.equal(bud[:used], ref[:used])


def test_refusals_reach_python(native):
    bgr = _content("zero", 1, 64, 64, 0)
    types = _types("zero", 1, 64, 64, MV16, 0)
    with pytest.raises(Exception, match="non-decreasing"):
        nat.dct_pack_levels_quality_frames(bgr, 8, types, MV16, [(2, 640), (1, 640)], 1 << 20)
    with pytest.raises(Exception, match="8x8, 16x16"):
        nat.dct_pack_levels_quality_frames(bgr, 4, types, MV16, [(1, 640)], 1 << 20, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
