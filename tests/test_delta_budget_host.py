"""svc_hip_dct_pack_delta_budget_frames (include/svc_hip_delta_budget.h: a byte budget per group of frames for the delta stream) without
a device: the numpy statement's identities (layers.delta_groups, delta_ladder_counts, delta_budget_choice, delta_budget_frames) on frames
written with layers.write_frame, every branch of the choice on hand-made tables, and what the C ABI answers before it reaches a kernel.
What the kernels write is tests/test_gpu_dct_pack_delta_budget.py."""
from __future__ import annotations

import os
import re

import numpy as np

from scalable_video_codec_amd import layers, levels, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svc_hip_delta_budget.h")
OVER = 0x80000000
LADDER5 = [(1, 1), (1, 3), (3, 3), (3, 640), (640, 640)]  # fg == bg at entries 0, 2 and 4 only


def geometry(w, h, block, mv=16):
    return dict(frame_w=w, frame_h=h, block_w=block, block_h=block, mv_block_w=mv, mv_block_h=mv)


def levels_off(g):
    tiles = (g["frame_w"] // g["block_w"]) * (g["frame_h"] // g["block_h"])
    mvb = (g["frame_w"] // g["mv_block_w"]) * (g["frame_h"] // g["mv_block_h"])
    return 64 + 4 * mvb + 8 * 3 * tiles * (g["block_w"] * g["block_h"] // 64)


def plain_stream(planes, types, g, fg, bg):
    """The plain SVCQ stream of coefficient planes (n, 3, H, W) at one pair, as the packers write it."""
    frames = []
    for f in range(planes.shape[0]):
        background = layers._per_pixel(g, layers._tile_maps(g, types[f])[0])[None]
        frames.append(layers.write_frame(g, types[f], layers.quantise(planes[f], np.where(background, bg, fg)), fg, bg))
    return layers._join(frames)


def clip(rng, n, w, h, jitter=0.4):
    """Coefficient-like planes of a slowly moving clip: frame 0 random, every later frame its predecessor plus a little noise."""
    base = rng.standard_normal((3, h, w)) * rng.choice([0.4, 3.0, 40.0, 600.0], (3, h, w))
    out = [base]
    for _ in range(n - 1):
        out.append(out[-1] + jitter * rng.standard_normal((3, h, w)))
    return np.clip(np.stack(out), -4080, 4080).astype(np.float32)


def test_groups_start_at_frame_zero_and_at_every_flag():
    assert layers.delta_groups(None, 5) == [(0, 5)]
    assert layers.delta_groups([0, 0, 0], 3) == [(0, 3)]
    assert layers.delta_groups([1, 0, 0], 3) == [(0, 3)]  # frame 0 starts a group whatever its flag
    assert layers.delta_groups([0, 0, 1, 0, 7, 1], 6) == [(0, 2), (2, 4), (4, 5), (5, 6)]
    assert layers.delta_groups([1, 1, 1], 3) == [(0, 1), (1, 2), (2, 3)]
    assert layers.delta_groups(None, 0) == []


def test_the_choice_on_hand_made_tables():
    g = geometry(32, 16, 8)
    off = levels_off(g)
    assert off % 16 == 8  # 64 + 8 + 288: a frame of c levels has up16(off + 2 c) bytes

    def size(c):
        return (off + 2 * c + 15) // 16 * 16
    counts = np.array([[40, 30, 20, 10], [4, 3, 2, 1], [12, 12, 12, 12]], np.uint32)
    choose = layers.delta_budget_choice
    # one group: the sums decide, not any one frame
    total = [size(40) + size(4) + size(12), size(30) + size(3) + size(12), size(20) + size(2) + size(12), size(10) + size(1) + size(12)]
    assert choose(counts, g, None, [total[2], 0, 0]).tolist() == [2, 2, 2]           # fits exactly, and the budgets are summed
    assert choose(counts, g, None, [total[2] - 16, 8, 7]).tolist() == [3, 3, 3]      # one byte short of entry 2
    assert choose(counts, g, None, total[0] // 3 + 16).tolist() == [0, 0, 0]        # one budget for every frame
    assert choose(counts, g, None, 0).tolist() == [3 | OVER] * 3                    # none fits: the last entry, bit 31
    assert choose(counts, g, [0, 0, 0], [total[3] - 1, 0, 0]).tolist() == [3 | OVER] * 3
    # three groups of one frame: each frame on its own
    assert choose(counts, g, [1, 1, 1], [size(30), size(4), size(12) - 16]).tolist() == [1, 0, 3 | OVER]
    # two groups; a tie between entries takes the finest
    flat = np.array([[5, 5, 5], [5, 5, 5], [9, 1, 1]], np.uint32)
    assert choose(flat, g, [0, 0, 1], [size(5), size(5), size(1)]).tolist() == [0, 0, 1]
    # sums of 64 bits: budgets of 2^32 - 1 each do not wrap
    assert choose(counts, g, None, [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]).tolist() == [0, 0, 0]
    assert choose(np.zeros((2, 1), np.uint32), g, None, size(0)).tolist() == [0, 0]  # a one-entry ladder
    assert choose(np.zeros((2, 1), np.uint32), g, None, size(0) - 1).tolist() == [0 | OVER] * 2


def test_every_entry_is_looked_at_in_a_table_that_is_not_monotone():
    g = geometry(32, 16, 8)
    off = levels_off(g)

    def size(c):
        return (off + 2 * c + 15) // 16 * 16
    bumpy = np.array([[50, 20, 60, 10]], np.uint32)  # rises from entry 1 to entry 2
    choose = layers.delta_budget_choice
    assert choose(bumpy, g, None, size(20)).tolist() == [1]       # fits at an entry finer than the rise
    assert size(60) > size(20)                                    # ... and not at the entry after it
    assert choose(bumpy, g, None, size(20) - 16).tolist() == [3]  # behind an entry that does not fit
    assert choose(bumpy, g, None, size(50)).tolist() == [0]
    # the group's sum can be monotone where no frame is, and the other way round
    two = np.array([[10, 30, 20], [30, 10, 25]], np.uint32)
    assert choose(two, g, None, [size(10) + size(30), 0]).tolist() == [0, 0]  # (10 + 30 and 30 + 10: the same bytes, the finest wins)
    assert choose(two, g, None, [size(20) + size(25) - 16, 0]).tolist() == [2 | OVER] * 2
    assert choose(two, g, [1, 1], [size(10), size(10)]).tolist() == [0, 1]


def test_counts_are_word_10_of_the_delta_stream_and_frame_0_is_a_key_frame():
    rng = np.random.default_rng(3)
    g = geometry(32, 16, 8)
    n = 5
    planes = clip(rng, n, 32, 16)
    types = rng.choice([0, 1, 7], (n, 1, 2)).astype(np.uint32)
    keys = [0, 0, 1, 0, 0]
    streams = [plain_stream(planes, types, g, fg, bg) for fg, bg in LADDER5]
    counts = layers.delta_ladder_counts(streams, keys)
    assert counts.shape == (n, 5) and counts.dtype == np.uint32
    for k, (s, o) in enumerate(streams):
        out, offs = layers.delta_frames(s, o, keys)
        for f, (hdr, _, _) in enumerate(levels.iter_frames(out, offs)):
            assert counts[f, k] == hdr["level_count"]
        plain = [h["level_count"] for h, _, _ in levels.iter_frames(s, o)]
        assert counts[0, k] == plain[0] and counts[2, k] == plain[2]  # the key frames: the frames themselves
    assert (layers.delta_ladder_counts(streams, None)[0] == counts[0]).all()
    # equal frames leave no difference at any entry
    still = np.repeat(planes[:1], 3, 0)
    same = rng.choice([0, 1], (1, 1, 2)).astype(np.uint32).repeat(3, 0)
    c = layers.delta_ladder_counts([plain_stream(still, same, g, fg, bg) for fg, bg in LADDER5], None)
    assert (c[1:] == 0).all() and c[0, 0] > 0


def test_the_counts_of_differences_are_not_monotone_along_a_ladder():
    """Single 8x8 tiles under a jitter of +-1 pixel, steps 1 .. 16: in most of them some entry leaves MORE differences than the one
    before it, which no count of levels ever does."""
    rng = np.random.default_rng(11)
    lad = [(s, s) for s in (1, 2, 3, 4, 6, 8, 12, 16)]
    c = np.array([[np.sqrt((1 if u == 0 else 2) / 8) * np.cos(np.pi * u * (2 * m + 1) / 16) for m in range(8)] for u in range(8)])
    rises = 0
    for _ in range(16):
        pix = rng.integers(0, 256, (3, 8, 8)).astype(np.float64)
        moved = np.clip(pix + rng.integers(-1, 2, pix.shape), 0, 255)
        planes = np.stack([np.einsum("ua,cab,vb->cuv", c, p, c) for p in (pix, moved)]).astype(np.float32)
        g = dict(frame_w=8, frame_h=8, block_w=8, block_h=8, mv_block_w=8, mv_block_h=8)
        types = np.zeros((2, 1, 1), np.uint32)
        counts = layers.delta_ladder_counts([plain_stream(planes, types, g, fg, bg) for fg, bg in lad], None)
        assert (np.diff(counts[0].astype(np.int64)) <= 0).all()  # the key frame's levels only fall
        rises += bool((np.diff(counts[1].astype(np.int64)) > 0).any())
    assert rises >= 8, rises


def test_the_stream_is_the_delta_of_the_plain_stream_at_each_frames_own_pair():
    rng = np.random.default_rng(5)
    g = geometry(32, 16, 8)
    n = 9
    planes = clip(rng, n, 32, 16, 2.0)
    types = np.array([[[0, 7]]] * n, np.uint32)  # a background and a foreground block: every entry of the ladder moves a step
    types[4] = [[1, 0]]  # the classes flip inside a group: unpredicted tiles where fg != bg
    keys = np.array([0, 0, 0, 1, 0, 0, 1, 1, 0], np.uint32)
    streams = [plain_stream(planes, types, g, fg, bg) for fg, bg in LADDER5]
    counts = layers.delta_ladder_counts(streams, keys)
    off = levels_off(g)
    size = (off + 2 * counts.astype(np.int64) + 15) // 16 * 16
    # group 0 exactly at entry 1, group 1 over budget, group 2 (one frame) at entry 4, group 3 at entry 0
    budgets = np.zeros(n, np.int64)
    budgets[0] = size[0:3, 1].sum()
    budgets[3] = size[3:6, 4].sum() - 16
    budgets[6] = size[6, 4]
    budgets[7:9] = size[7:9, 0].max()
    assert size[0:3, 0].sum() > budgets[0] and size[6, :4].min() > budgets[6]
    out, offs, choice, got_counts = layers.delta_budget_frames(streams, keys, budgets)
    assert (got_counts == counts).all()
    assert choice.tolist() == [1, 1, 1, 4 | OVER, 4 | OVER, 4 | OVER, 4, 0, 0]
    assert choice.tolist() == layers.delta_budget_choice(counts, g, keys, budgets).tolist()
    # the plain stream in which every frame is packed at its own chosen pair, then delta_frames of it
    picks = [int(c) & 0x7FFFFFFF for c in choice]
    own = layers._join([bytes(layers._source_frames(*streams[k], None)[f]) for f, k in enumerate(picks)])
    want, want_offs = layers.delta_frames(*own, keys)
    assert out == want and offs.tolist() == want_offs.tolist()
    for f, (hdr, _, _) in enumerate(levels.iter_frames(out, offs)):
        assert (hdr["fg_step"], hdr["bg_step"]) == LADDER5[picks[f]] and hdr["inexact"] == 0 and hdr["level_count"] == counts[f, picks[f]]
    back, back_offs = layers.undelta_frames(out, offs, keys)
    assert back == own[0] and back_offs.tolist() == own[1].tolist()
    # without flags the call is one group
    _, _, one, _ = layers.delta_budget_frames(streams, None, 0xFFFFFFFF)
    assert one.tolist() == [0] * n


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

FN = "svc_hip_dct_pack_delta_budget_frames"
QUERY = "svc_hip_dct_pack_delta_budget_workspace_bytes"


def test_every_declaration_is_exported_and_bound_with_its_stream_last():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(svc_hip_\w+)\s*\(", text)
    assert sorted(declared) == sorted(native.SIGNATURES_DELTA_BUDGET) == [FN, QUERY]
    lib = native.load()
    for name, (res, args) in native.SIGNATURES_DELTA_BUDGET.items():
        fn = getattr(lib, name)  # exported
        assert fn.restype is res and list(fn.argtypes) == args
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        assert len(params) == len(args), name
    assert re.search(r"void\s*\*\s*stream\s*\)\s*;", text) and native.SIGNATURES_DELTA_BUDGET[FN][1][-1] is native._vp
    # the budgeted call's arguments with the key flags in front of the budget and the table behind the choice
    b = native.SIGNATURES["svc_hip_dct_pack_levels_budget_frames"][1]
    assert native.SIGNATURES_DELTA_BUDGET[FN][1] == b[:11] + [native._vp] + b[11:-1] + [native._vp] + b[-1:]
    others = [native.SIGNATURES, native.SIGNATURES_TEMPORAL, native.SIGNATURES_TEMPORAL_DECODE, native.SIGNATURES_QUALITY]
    assert all(not set(native.SIGNATURES_DELTA_BUDGET) & set(t) for t in others)
    assert lib.svc_hip_abi_version() == 5


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_delta_budget_workspace_bytes
    assert q(2, 64, 64, 4, 16, 8) == 0           # a 4x4 block: not the tuned transform
    assert q(2, 72, 64, 8, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16), 8) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8), 8) == 0
    assert q(2, 64, 64, 8, 16, 0) == 0           # a ladder of 1 .. 64 entries
    assert q(2, 64, 64, 8, 16, 65) == 0
    assert q(70000, 64, 64, 8, 16, 8) == 0       # more frames than one call takes
    assert q(1, 32768, 32768, 16, 16, 8) == 0    # a frame beyond the u32 frame_bytes field
    for n, w, h, block, mv in ((2, 64, 64, 8, 16), (1, 3840, 2176, 16, 16), (3, 272, 24, 8, (16, 8)), (17, 48, 16, 8, 16)):
        for k in (1, 8, 64):
            assert q(n, w, h, block, mv, k) > native.dct_pack_delta_workspace_bytes(n, w, h, block, mv) > 0  # it begins with that call's


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks -- geometry, stride, ladder, limits, workspace,
    capacity -- and the null-pointer check stands between any of them and a launch."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, ladder, n=2, ws=1 << 40, cap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        arr, k = native._ladder(ladder)
        return getattr(lib, FN)(None, stride, n, w, h, block, None, mbw, mbh, arr, k, None, None, None, ws, None, cap, None, None, None, None)
    good = [(1, 640), (2, 640), (2, 700)]
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, good, n=n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, good, n=n) == bad and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, good, n=n) == unsup and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, good, n=n) == unsup and "multiple of 16" in err()
        assert call(72, 64, 8, 8, 8, [(0, 640)], n=n) == unsup and "multiple of 16" in err()  # geometry before the ladder
        assert call(64, 64, 8, 16, 16, [(0, 640)], n=n, stride=64 * 64 * 3 - 16) == bad and "stride" in err()  # the stride before the ladder
        assert call(64, 64, 8, 16, 16, good, n=n, stride=64 * 64 * 3 + 8) == bad and "stride" in err()
        assert call(64, 64, 8, 16, 16, [], n=n, ws=0, cap=0) == bad and "ladder of 0 entries" in err()  # the ladder before any size
        assert call(64, 64, 8, 16, 16, [(1, 640)] * 65, n=n) == bad and "ladder of 65 entries" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (0, 640)], n=n, ws=0, cap=0) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, [(2, 640), (1, 640)], n=n, ws=0, cap=0) == bad and "non-decreasing" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (2, 639)], n=n, ws=0, cap=0) == bad and "non-decreasing" in err()
        assert "dct_pack_delta_budget" in err()
        assert call(32768, 32768, 16, 16, 16, good, n=n, ws=0, cap=0) == unsup and "frame_bytes" in err()
    assert call(64, 64, 8, 16, 16, good, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch, every pointer NULL
    assert call(64, 64, 16, 16, 16, [(3, 17)], n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, good, n=70000, ws=0, cap=0) == unsup and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_delta_budget_workspace_bytes(2, 64, 64, 8, 16, len(good))
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, good, ws=need_ws - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out - 16) == bad and "worst case" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
