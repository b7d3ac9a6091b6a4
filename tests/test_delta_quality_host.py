"""svc_hip_dct_pack_delta_quality_frames (include/svc_hip_delta_quality.h: a distortion target per group of frames for the delta stream)
without a device: every branch of the choice on hand-made tables (layers.delta_quality_choice), its identities with the per-frame quality
rule and the group budget rule, the stream (layers.delta_quality_frames) on frames written with layers.write_frame, and what the C ABI
answers before it reaches a kernel.  What the kernels write is tests/test_gpu_dct_pack_delta_quality.py."""
from __future__ import annotations

import os
import re

import numpy as np

from scalable_video_codec_amd import layers, levels, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svc_hip_delta_quality.h")
OVER, MISSED, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF
LADDER5 = [(1, 1), (1, 3), (3, 3), (3, 640), (640, 640)]  # fg == bg at entries 0, 2 and 4 only


def geometry(w, h, block, mv=16):
    return dict(frame_w=w, frame_h=h, block_w=block, block_h=block, mv_block_w=mv, mv_block_h=mv)


def levels_off(g):
    tiles = (g["frame_w"] // g["block_w"]) * (g["frame_h"] // g["block_h"])
    mvb = (g["frame_w"] // g["mv_block_w"]) * (g["frame_h"] // g["mv_block_h"])
    return 64 + 4 * mvb + 8 * 3 * tiles * (g["block_w"] * g["block_h"] // 64)


def sizes(g, counts):
    return (levels_off(g) + 2 * np.asarray(counts, np.int64) + 15) // 16 * 16


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


def branch(table, counts, g, keys, targets, budgets, first, end, value):
    """Which of the rule's branches gave a group its value, from the sets themselves: 'both', 'fits', 'none' or 'none-missed'."""
    L = table.shape[1]
    target = np.broadcast_to(np.asarray(targets, np.uint64), (table.shape[0],))
    met = {k for k in range(L) if all(int(table[f, k]) <= int(target[f]) for f in range(first, end))}
    fits = set(range(L))
    if budgets is not None:
        budget = np.broadcast_to(np.asarray(budgets, np.int64), (table.shape[0],))
        total = sizes(g, counts)[first:end].sum(axis=0)
        fits = {k for k in range(L) if int(total[k]) <= int(budget[first:end].sum())}
    if met & fits:
        assert value == max(met & fits)
        return "both-capped" if max(met & fits) != max(met) else "both"
    if fits:
        assert value == min(fits) | MISSED
        return "fits-no-budget" if budgets is None else "fits"
    assert value == (L - 1) | OVER | (0 if L - 1 in met else MISSED)
    return "none" if L - 1 in met else "none-missed"


def test_every_branch_of_the_choice_on_hand_made_tables():
    g = geometry(32, 16, 8)
    size = lambda c: int(sizes(g, c))  # noqa: E731
    counts = np.array([[40, 30, 20, 10], [4, 3, 2, 1], [12, 12, 12, 12]], np.uint32)
    table = np.array([[10, 20, 30, 40], [1, 2, 3, 4], [5, 50, 5, 500]], np.uint64)  # frame 2's D is not monotone
    total = [sum(size(int(c)) for c in counts[:, k]) for k in range(4)]
    choose = layers.delta_quality_choice
    seen = set()
    cases = [
        # (keys, targets, budgets, expected)
        (None, [40, 4, 500], None, [3, 3, 3]),                               # Q = all, no cap: the coarsest
        (None, [30, 3, 49], None, [2, 2, 2]),                                # frame 2 misses at entry 1 but meets at entry 2: Q = {0, 2}
        (None, [30, 3, 49], [total[1], 0, 0], [2, 2, 2]),                    # F = {1, 2, 3}: Q & F = {2}
        (None, [40, 4, 500], [total[1] - 16, 8, 7], [3, 3, 3]),
        (None, [9, 4, 500], None, [0 | MISSED] * 3),                         # Q empty, no budget: entry 0, bit 30
        (None, [10, 1, 5], [total[2], 0, 0], [2 | MISSED] * 3),              # Q = {0}, F = {2, 3}: the finest that fits, bit 30
        (None, [40, 4, 500], 0, [3 | OVER] * 3),                             # F empty, the last entry in Q: bit 31 alone
        (None, [40, 4, 499], 0, [3 | OVER | MISSED] * 3),                    # F empty, the last entry not in Q: both bits
        ([1, 1, 1], [20, 0, 5], [size(10), size(4), size(12) - 16], [3 | MISSED, 0 | MISSED, 3 | OVER | MISSED]),
        ([0, 0, 1], [20, 2, 5], None, [1, 1, 2]),                            # two groups, each its own sets
    ]
    for keys, targets, budgets, want in cases:
        got = choose(counts, table, g, keys, targets, budgets)
        assert got.dtype == np.uint32 and got.tolist() == want, (keys, targets, budgets, got.tolist())
        for first, end in layers.delta_groups(keys, 3):
            assert len(set(got[first:end].tolist())) == 1  # every frame of a group carries its group's value
            seen.add(branch(table, counts, g, keys, targets, budgets, first, end, int(got[first])))
    # a coarser entry of Q that does not fit: sizes that RISE along the ladder, so F = {0, 1} under Q = {0, 1, 2, 3}
    rising = np.array([[1, 2, 30, 40]], np.uint32)
    flat = np.array([[7, 7, 7, 7]], np.uint64)
    got = choose(rising, flat, g, None, 7, size(2))
    assert got.tolist() == [1]
    seen.add(branch(flat, rising, g, None, 7, size(2), 0, 1, 1))
    assert seen == {"both", "both-capped", "fits", "fits-no-budget", "none", "none-missed"}, seen
    # sums of 64 bits: budgets of 2^32 - 1 each do not wrap; targets of 2^64 - 1 compare as u64
    assert choose(counts, table, g, None, 2 ** 64 - 1, [0xFFFFFFFF] * 3).tolist() == [3, 3, 3]
    big = np.array([[2 ** 63 + 5, 2 ** 63 + 7]], np.uint64)
    assert choose(np.zeros((1, 2), np.uint32), big, g, None, 2 ** 63 + 6).tolist() == [0]
    assert choose(np.zeros((2, 1), np.uint32), np.ones((2, 1), np.uint64), g, None, 1, size(0) - 1).tolist() == [0 | OVER] * 2  # one entry


def test_one_frame_alone_can_miss_the_target():
    """Eleven frames meet the target at entry 2 by a wide margin, one misses it by a unit: the group's SUM of D would pass, the group does
    not -- a viewer sees frames."""
    g = geometry(32, 16, 8)
    n = 12
    table = np.tile(np.array([1, 10, 100, 5000], np.uint64), (n, 1))
    table[7, 2] = 1001
    counts = np.tile(np.array([40, 30, 20, 10], np.uint32), (n, 1))
    assert int(table[:, 2].sum()) < 1000 * n and (np.delete(table[:, 2], 7) <= 1000).all()
    assert layers.delta_quality_choice(counts, table, g, None, 1000).tolist() == [1] * n
    table[7, 2] = 1000
    assert layers.delta_quality_choice(counts, table, g, None, 1000).tolist() == [2] * n
    # per-frame targets: the one frame's own target decides
    table[7, 2] = 1001
    targets = np.full(n, 1000, np.uint64)
    targets[7] = 1001
    assert layers.delta_quality_choice(counts, table, g, None, targets).tolist() == [2] * n
    # the frame misses only in its own group
    keys = np.zeros(n, np.uint32)
    keys[[6, 9]] = 1
    assert layers.delta_quality_choice(counts, table, g, keys, 1000).tolist() == [2] * 6 + [1] * 3 + [2] * 3


def test_with_every_frame_a_key_frame_it_is_the_per_frame_quality_rule():
    rng = np.random.default_rng(21)
    g = geometry(48, 16, 8)
    n, L = 40, 7
    counts = np.sort(rng.integers(0, 2000, (n, L)), axis=1)[:, ::-1].astype(np.uint32)  # monotone sizes: levels only fall
    table = rng.integers(1, 10 ** 6, (n, L)).astype(np.uint64)                         # D in any order
    size = sizes(g, counts)
    targets = rng.integers(0, 10 ** 6, n).astype(np.uint64)
    keys = np.ones(n, np.uint32)
    flags = set()
    for budgets in (None, rng.integers(int(size.min()) - 32, int(size.max()) + 32, n)):
        got = layers.delta_quality_choice(counts, table, g, keys, targets, budgets)
        assert got.tolist() == layers.quality_choice(table, size, targets, budgets).tolist()
        flags |= {int(c) >> 30 for c in got}
    assert flags == {0, 1, 2, 3}


def test_at_targets_of_zero_it_is_the_group_budget_rule_with_bit_30():
    rng = np.random.default_rng(22)
    g = geometry(48, 16, 8)
    n, L = 24, 6
    counts = rng.integers(0, 2000, (n, L)).astype(np.uint32)  # not monotone
    table = rng.integers(1, 10 ** 6, (n, L)).astype(np.uint64)
    keys = (rng.random(n) < 0.3).astype(np.uint32)
    size = sizes(g, counts)
    over = 0
    for scale in (0.5, 0.8, 1.0, 1.3):
        budgets = (size.mean(axis=1) * scale).astype(np.int64)
        want = layers.delta_budget_choice(counts, g, keys, budgets) | np.uint32(MISSED)
        assert layers.delta_quality_choice(counts, table, g, keys, 0, budgets).tolist() == want.tolist()
        over += int((want & OVER != 0).sum())
    assert 0 < over < 4 * n


def test_the_stream_is_the_delta_of_the_plain_stream_at_each_frames_own_pair():
    rng = np.random.default_rng(5)
    g = geometry(32, 16, 8)
    n = 9
    planes = clip(rng, n, 32, 16, 2.0)
    types = np.array([[[0, 7]]] * n, np.uint32)
    types[4] = [[1, 0]]  # the classes flip inside a group: unpredicted tiles where fg != bg
    keys = np.array([0, 0, 0, 1, 0, 0, 1, 1, 0], np.uint32)
    streams = [plain_stream(planes, types, g, fg, bg) for fg, bg in LADDER5]
    table = layers.distortion_table(planes, types, g, LADDER5)
    counts = layers.delta_ladder_counts(streams, keys)
    size = sizes(g, counts)
    # group 0 (frames 0-2) at entry 2 by quality, group 1 (3-5) capped below its quality entry, group 2 (6) over budget, group 3 (7-8) at the last
    targets = np.zeros(n, np.uint64)
    targets[0:3] = table[0:3, 2].max()
    targets[3:6] = table[3:6, 3].max()
    targets[6] = table[6, 1]
    targets[7:9] = table[7:9].max()
    budgets = np.full(n, 0xFFFFFFFF, np.int64)
    budgets[3:6] = 0
    budgets[3] = size[3:6, 4].sum()
    budgets[6] = size[6].min() - 16
    out, offs, choice, got_counts = layers.delta_quality_frames(streams, table, keys, targets, budgets)
    assert (got_counts == counts).all()
    assert choice.tolist() == layers.delta_quality_choice(counts, table, g, keys, targets, budgets).tolist()
    picks = [int(c) & INDEX for c in choice]
    assert picks[0:3] == [picks[0]] * 3 and picks[0] >= 2 and picks[7:9] == [4, 4] and int(choice[6]) & OVER
    assert all(int(table[f, picks[f]]) <= int(targets[f]) for f in (0, 1, 2, 7, 8)) and not any(int(c) & MISSED for c in choice[[0, 1, 2, 7, 8]])
    # the plain stream in which every frame is packed at its own chosen pair, then delta_frames of it
    own = layers._join([bytes(layers._source_frames(*streams[k], None)[f]) for f, k in enumerate(picks)])
    want, want_offs = layers.delta_frames(*own, keys)
    assert out == want and offs.tolist() == want_offs.tolist()
    for f, (hdr, _, _) in enumerate(levels.iter_frames(out, offs)):
        assert (hdr["fg_step"], hdr["bg_step"]) == LADDER5[picks[f]] and hdr["inexact"] == 0 and hdr["level_count"] == counts[f, picks[f]]
    back, back_offs = layers.undelta_frames(out, offs, keys)
    assert back == own[0] and back_offs.tolist() == own[1].tolist()
    # without flags and without a cap the call is one group at the coarsest entry every frame meets
    _, _, one, _ = layers.delta_quality_frames(streams, table, None, 2 ** 64 - 1)
    assert one.tolist() == [4] * n


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

FN = "svc_hip_dct_pack_delta_quality_frames"
QUERY = "svc_hip_dct_pack_delta_quality_workspace_bytes"


def test_every_declaration_is_exported_and_bound_with_its_stream_last():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(svc_hip_\w+)\s*\(", text)
    assert sorted(declared) == sorted(native.SIGNATURES_DELTA_QUALITY) == [FN, QUERY]
    lib = native.load()
    for name, (res, args) in native.SIGNATURES_DELTA_QUALITY.items():
        fn = getattr(lib, name)  # exported
        assert fn.restype is res and list(fn.argtypes) == args
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        assert len(params) == len(args), name
    assert re.search(r"void\s*\*\s*stream\s*\)\s*;", text) and native.SIGNATURES_DELTA_QUALITY[FN][1][-1] is native._vp
    # the delta-budget call's arguments with the target in front of the budget and the distortion table behind the counts
    b = native.SIGNATURES_DELTA_BUDGET["svc_hip_dct_pack_delta_budget_frames"][1]
    assert native.SIGNATURES_DELTA_QUALITY[FN][1] == b[:12] + [native._vp] + b[12:-1] + [native._vp] + b[-1:]
    others = [native.SIGNATURES, native.SIGNATURES_TEMPORAL, native.SIGNATURES_TEMPORAL_DECODE, native.SIGNATURES_QUALITY,
              native.SIGNATURES_DELTA_BUDGET]
    assert all(not set(native.SIGNATURES_DELTA_QUALITY) & set(t) for t in others)
    assert lib.svc_hip_abi_version() == 5


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_delta_quality_workspace_bytes
    assert q(2, 64, 64, 4, 16, 8) == 0           # a 4x4 block: not the tuned transform
    assert q(2, 72, 64, 8, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16), 8) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8), 8) == 0
    assert q(2, 64, 64, 8, 16, 0) == 0           # a ladder of 1 .. 64 entries
    assert q(2, 64, 64, 8, 16, 65) == 0
    assert q(70000, 64, 64, 8, 16, 8) == 0       # more frames than one call takes
    assert q(1, 32768, 32768, 16, 16, 8) == 0    # a frame beyond the u32 frame_bytes field
    for n, w, h, block, mv in ((2, 64, 64, 8, 16), (1, 3840, 2176, 16, 16), (3, 272, 24, 8, (16, 8)), (17, 48, 16, 8, 16)):
        for k in (1, 8, 64):  # it begins with the delta-budget call's, which begins with the delta call's
            assert (q(n, w, h, block, mv, k) > native.dct_pack_delta_budget_workspace_bytes(n, w, h, block, mv, k)
                    > native.dct_pack_delta_workspace_bytes(n, w, h, block, mv) > 0)


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks -- geometry, stride, ladder, limits, workspace,
    capacity -- and the null-pointer check stands between any of them and a launch."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, ladder, n=2, ws=1 << 40, cap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        arr, k = native._ladder(ladder)
        return getattr(lib, FN)(None, stride, n, w, h, block, None, mbw, mbh, arr, k, None, None, None, None, ws, None, cap, None, None, None,
                                None, None)
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
        assert "dct_pack_delta_quality" in err()
        assert call(32768, 32768, 16, 16, 16, good, n=n, ws=0, cap=0) == unsup and "frame_bytes" in err()
    assert call(64, 64, 8, 16, 16, good, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch, every pointer NULL
    assert call(64, 64, 16, 16, 16, [(3, 17)], n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, good, n=70000, ws=0, cap=0) == unsup and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_delta_quality_workspace_bytes(2, 64, 64, 8, 16, len(good))
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, good, ws=need_ws - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out - 16) == bad and "worst case" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out) == bad and "null pointer" in err()
