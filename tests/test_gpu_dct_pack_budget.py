"""svc_hip_dct_pack_levels_budget_frames (csrc/dct_pack.hip): rate control inside the fused transform leaves, byte for byte, what
svc_hip_dct_frames followed by svc_hip_pack_levels_budget_frames leave on the same device -- the stream, all n + 1 offsets and the
choices -- and each frame is what svc_hip_dct_pack_levels_frames writes with its chosen pair.  Every comparison is exact.  The
shapes are those of tests/test_gpu_dct_pack.py: the smallest at which each mechanism of the fused kernels can break.

One header word cannot equal both references and is compared apart: `inexact` (word 11) counts the coefficients of the planes a
pack was handed that are not level * step.  The planes route packs RAW planes, so its count is in the hundreds per frame; the fused
calls are handed no planes, quantise themselves and write 0, as svc_hip_dct_pack_levels_frames does.  The budgeted fused call writes
0: its frames are the fixed fused call's to the last byte, and the planes route's in every byte but that word."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import levels
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _strided, _two_calls, _types
from tests.test_levels_budget_host import frame_bytes, frame_floor, ladder

pytestmark = pytest.mark.gpu

OVER = 0x80000000


def _mixed(n, w, h, seed):
    """One random frame, one synthetic frame, one zero frame (then again): frames whose sizes along a ladder differ."""
    def one(f):
        if f % 3 == 1:  # (the synthetic clip needs room for its rectangles: a corner of a larger frame at the smallest shapes)
            return _content("synth", 1, max(w, 64), max(h, 32), seed + f)[:, :h, :w]
        return _content(("random", "synth", "zero")[f % 3], 1, w, h, seed + f)
    return torch.cat([one(f) for f in range(n)]).contiguous()


def _planes(buf, stride, n, w, h, block):
    planes = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    nat._check(nat.load().svc_hip_dct_frames(buf.data_ptr(), stride, n, w, h, block, block, planes.data_ptr(), nat._stream()))
    return planes


def _route(planes, types, block, mv, lad, budget):
    """The second half of the two-call route on the first half's planes -> (stream pre-filled with FILL, offsets, choice)."""
    n, _, h, w = planes.shape
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    return nat.pack_levels_budget_frames(planes, types, block, mv, lad, budget, out=out)


def _fused(buf, stride, n, w, h, block, types, mv, lad, budget, ws=None):
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    choice = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if ws is None:
        ws = torch.empty(nat.dct_pack_levels_budget_workspace_bytes(n, w, h, block, mv, len(lad)), dtype=torch.uint8, device="cuda")
    arr, k = nat._ladder(lad)
    b = nat.budget_tensor(budget, n, "cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_budget_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], arr, k,
                                                               b.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                                                               offs.data_ptr(), choice.data_ptr(), nat._stream()))
    return out, offs, choice


def _check(bgr, types, block, mv, lad, budget, extra=0):
    """THE shared check: choice, all offsets, the bytes, the fill past offsets[n]; per frame the fixed fused call with its pair.
    -> (the choices as u32, the stream's bytes on the host, the offsets)."""
    n, h, w, _ = bgr.shape
    buf, stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
    planes = _planes(buf, stride, n, w, h, block)
    budget = budget(planes) if callable(budget) else budget
    want, want_offs, want_choice = _route(planes, types, block, mv, lad, budget)
    got, got_offs, got_choice = _fused(buf, stride, n, w, h, block, types, mv, lad, budget)
    torch.cuda.synchronize()
    choice = got_choice.cpu().numpy().view(np.uint32)
    assert choice.tolist() == want_choice.cpu().numpy().view(np.uint32).tolist()
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist()  # all n + 1 of them
    used = offs[-1]
    g = got.cpu().numpy()
    ref = want[:used].cpu().numpy().copy()
    for f in range(n):  # the planes route's count of raw coefficients that are not level * step: the fused calls write 0 (see above)
        assert g[offs[f]:offs[f] + 64].view(np.uint32)[11] == 0
        ref[offs[f]:offs[f] + 64].view(np.uint32)[11] = 0
    assert g[:used].tobytes() == ref.tobytes()
    assert (g[used:] == FILL).all()  # nothing is written past the stream
    for f in range(n):
        fg, bg = (int(v) for v in lad[int(choice[f]) & 0x7FFFFFFF])
        one, one_offs = nat.dct_pack_levels_frames(bgr[f:f + 1].contiguous(), block, types[f:f + 1].contiguous(), mv, fg, bg)
        torch.cuda.synchronize()
        assert g[offs[f]:offs[f + 1]].tobytes() == one[:int(one_offs[-1])].cpu().numpy().tobytes(), f
    return choice, g[:used], offs


def _sizes(planes, types, block, mv, lad):
    p, t = planes.cpu().numpy(), types.cpu().numpy().view(np.uint32)
    return [frame_bytes(p[f], t[f], block, block, mv[0], mv[1], lad) for f in range(len(p))]


def _mixed_budgets(types, block, mv, lad, below_floor):
    """For the frames of _mixed (n = 3): the random frame lands exactly on the size of an entry it has to step down to, the synthetic
    one is 16 bytes short of one of its sizes, the zero frame is below the masks' floor or has 0xFFFFFFFF.  With a one-entry ladder:
    below the floor, exactly the size, 0xFFFFFFFF."""
    def budgets(planes):
        _, _, h, w = planes.shape
        sizes = _sizes(planes, types, block, mv, lad)
        floor = frame_floor(w, h, block, block, mv[0], mv[1])
        if len(lad) == 1:
            return [floor - 16, int(sizes[1][0]), 0xFFFFFFFF]
        ka = max([k for k in range(1, len(lad)) if sizes[0][k] < sizes[0][k - 1]], default=0)  # the last entry that still shrinks it
        return [int(sizes[0][ka]), int(sizes[1][len(lad) // 2]) - 16, floor - 16 if below_floor else 0xFFFFFFFF]
    return budgets


# w, h, mv, types, bytes between frames: n = 3 mixed frames each
SHAPES8 = [
    (16, 8, (16, 8), "random", 0),        # three waves of one workgroup, each from another frame with another choice
    (48, 16, MV16, "random", 0),          # 3 MV blocks: the masks are only 4-byte aligned
    (272, 24, (16, 8), "checker", 48),    # a full wave + a one-column wave per row, noise between the frames
    (64, 32, (32, 16), "checker", 0),
]
SHAPES16 = [
    (16, 16, MV16, "random", 0),
    (48, 32, MV16, "random", 0),
    (144, 48, MV16, "checker", 16),       # two full waves + a one-column wave per row
]


def _shape_case(block, shape, k):
    w, h, mv, types_kind, extra = shape
    seed = w + h + k + block
    bgr = _mixed(3, w, h, seed)
    types = _types(types_kind, 3, w, h, mv, seed)
    lad = ladder(k)
    choice, _, _ = _check(bgr, types, block, mv, lad, _mixed_budgets(types, block, mv, lad, below_floor=(w // 16) % 2 == 1), extra)
    assert len(set(choice.tolist())) >= 2  # the frames of one batch -- at 16 pixels of width, of one workgroup -- took different entries
    if k > 1:
        assert choice[0] < k  # the random frame is within its budget


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("shape", SHAPES8, ids=lambda c: "-".join(str(x) for x in c))
def test_budgeted_8x8_equals_the_two_calls(native, shape, k):
    _shape_case(8, shape, k)


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("shape", SHAPES16, ids=lambda c: "-".join(str(x) for x in c))
def test_budgeted_16x16_equals_the_two_calls(native, shape, k):
    _shape_case(16, shape, k)


@pytest.mark.parametrize("block", [8, 16])
def test_one_1080p_frame(native, block):
    w, h, mv = 1920, 1088, MV16
    lad = levels.step_ladder(1, 256, 4, 640, 10, 24)
    bgr = _content("synth", 1, w, h, 1080 + block)
    types = _types("random", 1, w, h, mv, block)

    def budget(planes):  # one step below the size of entry 20, from the two-call route's own fixed pack at that pair
        _, offs = nat.pack_levels_frames(planes, types, block, mv, int(lad[20][0]), int(lad[20][1]))
        return [int(offs[1]) - 16]
    choice, _, _ = _check(bgr, types, block, mv, lad, budget)
    assert 21 <= choice[0] < len(lad)


def test_a_rounding_tie_derived_by_hand(native):
    """Flat frames of value 1 at 8x8: every tile's DC is 8.0f (the f64 chain's error is far below half an f32 ulp at 8) and every AC
    is 0.  8 / 16 = 0.5 rounds away from zero: entry (16, 16) keeps every DC, 3 per tile.  8 / 17 rounds to 0: entry (17, 17) keeps
    nothing."""
    w, h, n, mv = 48, 16, 3, MV16
    tiles = (w // 8) * (h // 8)
    floor = frame_floor(w, h, 8, 8, 16, 16)
    assert floor == 64 + 4 * 3 + 8 * 3 * tiles
    size0, size1 = (floor + 2 * 3 * tiles + 15) // 16 * 16, (floor + 15) // 16 * 16
    bgr = torch.ones((n, h, w, 3), dtype=torch.uint8, device="cuda")
    types = _types("random", n, w, h, mv, 1)
    lad = np.array([[16, 16], [17, 17]], np.uint32)
    choice, g, offs = _check(bgr, types, 8, mv, lad, [size0, size0 - 16, floor - 16])
    assert choice.tolist() == [0, 1, 1 | OVER]
    assert offs == [0, size0, size0 + size1, size0 + 2 * size1]
    hdrs = [g[o:o + 64].view(np.uint32) for o in offs[:-1]]
    assert [int(hd[10]) for hd in hdrs] == [3 * tiles, 0, 0]  # level_count
    assert [(int(hd[8]), int(hd[9])) for hd in hdrs] == [(16, 16), (17, 17), (17, 17)]
    lv = g[floor:floor + 2 * 3 * tiles].view(np.int16)
    assert (lv == 1).all()  # 0.5 away from zero


@pytest.mark.parametrize("block", [8, 16])
def test_one_entry_ladder_is_the_fixed_fused_call(native, block):
    w, h, n = 272, 48, 3
    bgr = _mixed(n, w, h, 11)
    types = _types("random", n, w, h, MV16, 11)
    for budget in (1 << 30, [1 << 30, 100, 0]):
        got, got_offs, choice = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, [(3, 17)], budget)
        want, want_offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17)
        torch.cuda.synchronize()
        used = int(want_offs[-1])
        assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])
        exp = [0 if b >= int(want_offs[f + 1] - want_offs[f]) else OVER for f, b in enumerate(np.broadcast_to(budget, (n,)))]
        assert choice.cpu().numpy().view(np.uint32).tolist() == exp


@pytest.mark.parametrize("block", [8, 16])
def test_two_runs_give_the_same_bytes(native, block):
    w, h, n = 272, 48, 3
    bgr = _mixed(n, w, h, 9)
    types = _types("random", n, w, h, MV16, 9)
    lad = ladder(8)
    sizes = _sizes(nat.dct_frames(bgr, block), types, block, MV16, lad)
    budget = [int(sizes[0][3]), int(sizes[1][5]), int(sizes[2][0])]
    a, a_offs, a_ch = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, budget)
    b, b_offs, b_ch = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, budget, out=torch.zeros_like(a))
    torch.cuda.synchronize()
    used = int(a_offs[-1])
    assert torch.equal(a_offs, b_offs) and torch.equal(a_ch, b_ch) and torch.equal(a[:used], b[:used])


@pytest.mark.parametrize("block", [8, 16])
def test_the_budgeted_stream_feeds_the_unpack_and_the_entropy_coder(native, block):
    w, h, n = 144, 48, 3
    bgr = _mixed(n, w, h, 3)
    types = _types("random", n, w, h, MV16, 3)
    lad = ladder(8)
    sizes = _sizes(nat.dct_frames(bgr, block), types, block, MV16, lad)
    out, offs, choice = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, [int(sizes[0][4]), int(sizes[1][2]) - 16, 1 << 20])
    used = int(offs[-1])
    got, got_types, status = nat.unpack_levels_frames(out[:used], offs, w, h, block, MV16)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and torch.equal(got_types, types)
    for f, c in enumerate(choice.cpu().numpy().view(np.uint32)):  # the planes the fixed quantiser leaves with the frame's pair
        fg, bg = (int(v) for v in lad[int(c) & 0x7FFFFFFF])
        assert torch.equal(got[f], nat.dct_quant_frames(bgr[f:f + 1].contiguous(), block, types[f:f + 1].contiguous(), 16, fg, bg)[0]), f
    coded, coded_offs, st = nat.entropy_encode_frames(out[:used], offs, w, h, block, MV16)
    assert st.cpu().tolist() == [0] * n
    back, back_offs, st2 = nat.entropy_decode_frames(coded[:int(coded_offs[-1])], coded_offs, w, h, block, MV16)
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [0] * n
    assert torch.equal(back_offs, offs) and torch.equal(back[:used], out[:used])


@pytest.mark.parametrize("block", [8, 16])
def test_the_fixed_call_on_the_same_workspace_afterwards(native, block):
    """The budgeted call leaves per-frame steps in its workspace; the fixed call that follows on the same workspace must not read them."""
    w, h, n = 272, 48, 3
    bgr = _mixed(n, w, h, 21)
    types = _types("checker", n, w, h, MV16, 21)
    lad = ladder(8)
    ws = torch.empty(nat.dct_pack_levels_budget_workspace_bytes(n, w, h, block, MV16, len(lad)), dtype=torch.uint8, device="cuda")
    _, _, choice = nat.dct_pack_levels_budget_frames(bgr, block, types, MV16, lad, 0, workspace=ws)  # everything over budget: the last pair
    got, got_offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17, workspace=ws)
    _, want, want_offs = _two_calls(bgr, w * h * 3, n, w, h, block, types, MV16, 3, 17)
    torch.cuda.synchronize()
    assert choice.cpu().numpy().view(np.uint32).tolist() == [(len(lad) - 1) | OVER] * n
    used = int(want_offs[-1])
    assert torch.equal(got_offs, want_offs) and torch.equal(got[:used], want[:used])


def test_refusals_reach_python(native):
    bgr = _content("zero", 1, 64, 64, 0)
    types = _types("zero", 1, 64, 64, MV16, 0)
    with pytest.raises(Exception, match="non-decreasing"):
        nat.dct_pack_levels_budget_frames(bgr, 8, types, MV16, [(2, 640), (1, 640)], 1 << 20)
    with pytest.raises(Exception, match="8x8, 16x16"):
        nat.dct_pack_levels_budget_frames(bgr, 4, types, MV16, [(1, 640)], 1 << 20,
                                          workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
