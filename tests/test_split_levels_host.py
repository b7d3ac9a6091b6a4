"""svc_hip_split_levels_frames and its budgeted form (include/svc_hip.h: a stored fine SVCQ stream split into a base stream at any steps
plus its enhancement) without a device: the numpy statement (scalable_video_codec_amd/layers.py: split_frame, split_frames,
split_budget_frames) on frames built from seeded random levels, the workspace queries and the order of the argument checks.  The bytes
the kernels write are tests/test_gpu_split_levels.py."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import entropy, layers, levels, native
from tests.test_gpu_layers import _window
from tests.test_window_levels_host import GEOMS, geom_dict, random_levels, random_types

RATIOS = (1, 2, 3, 16, 639, 640, 32766)
DENSITIES = ((0.0, 1), (0.06, 1), (0.3, 1), (0.3, 2), (1.0, 1))  # with the fine step e


def _ids(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}-{g[3][0]}x{g[3][1]}"


def fine_frame(rng, geom, density, e, extremes=True):
    """-> (the frame at (e, e), its levels (3, h, w) i64, its region ids); the int16 extremes are among the levels."""
    w, h, tile, mv = geom
    lf = random_levels(rng, w, h, density)
    if extremes and density > 0:
        lf[0, 0, :3] = (32767, -32767, -32768)
        lf[2, -1, -3:] = (-32768, 32767, 1)
    types = random_types(rng, w, h, mv)
    return layers.write_frame(geom_dict(*geom), types, lf, e, e), lf, types


# ---- the statement's properties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density,e", DENSITIES)
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_statement_properties(geom, density, e):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 31 + h + int(100 * density) + e)
    rect = _window("rect", 1, w, h, tile[0])[0]
    oy, ox = np.meshgrid(np.arange(h) // tile[1] * tile[1], np.arange(w) // tile[0] * tile[0], indexing="ij")
    inside = (ox >= rect[0]) & (ox - rect[0] < rect[2]) & (oy >= rect[1]) & (oy - rect[1] < rect[3])
    assert inside.any() and not inside.all()
    coded = set()  # frames the lossless coder has given back
    fine, lf, types = fine_frame(rng, geom, density, e)
    for r_fg, r_bg in zip(RATIOS, RATIOS[::-1]):
        fg, bg = r_fg * e, r_bg * e
        base, enh = layers.split_frame(fine, e, fg, bg, None)
        merged, step = layers.merge_levels(base, enh, (0, 0, w, h))
        assert np.array_equal(merged, lf) and (step == e).all()                       # Lb * r + d == Lf, any ratio
        hb, types_b, _ = levels.parse_frame(base)
        he, types_e, pe = levels.parse_frame(enh)
        assert (hb["fg_step"], hb["bg_step"], he["fg_step"], he["bg_step"]) == (fg, bg, e, e)
        assert np.array_equal(types_b, types) and np.array_equal(types_e, types)
        lb, _ = layers._levels_of(hb, types_b, levels.parse_frame(base)[2])
        ratio = layers._per_pixel(hb, np.where(layers._tile_maps(hb, types)[0], r_bg, r_fg))[None]
        assert (np.abs(lb) <= np.abs(lf)).all() and (2 * np.abs(lf - lb * ratio) <= ratio).all()
        assert (np.abs(lf * e - lb * ratio * e) * 2 <= ratio * e).all()             # the base's error: within sb / 2 of Lf * e
        # outside the window d == 0; inside it the every-tile frame's d
        base_w, enh_w = layers.split_frame(fine, e, fg, bg, rect)
        assert base_w == base
        pw = levels.parse_frame(enh_w)[2]
        assert np.array_equal(pw, np.where(inside[None], pe, 0))
        assert enh_w == layers.window_frame(enh, rect)
        for fr in (base, enh, enh_w):  # canonical: the reader takes them, and the lossless coder gives them back
            assert len(fr) % 16 == 0 and np.frombuffer(fr, "<u4")[12] == len(fr)
            if fr not in coded:  # (ratio 1 leaves the same empty enhancement with and without the window)
                assert entropy.decode_frame(entropy.encode_frame(fr)) == fr
                coded.add(fr)


def test_a_set_bit_with_level_zero_is_a_zero():
    geom = GEOMS[1]
    w, h, tile, mv = geom
    rng = np.random.default_rng(7)
    fine, lf, types = fine_frame(rng, geom, 0.5, 2)
    levels_off = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * 3
    b = np.frombuffer(fine, np.uint8).copy()
    assert int(b[40:44].view("<u4")[0]) > 8
    b[levels_off:levels_off + 16] = 0  # eight levels of value 0 whose mask bits stay set
    zeroed = b.tobytes()
    canonical = layers.write_frame(geom_dict(*geom), types, layers._levels_of(*levels.parse_frame(zeroed))[0], 2, 2)
    assert canonical != zeroed and len(canonical) <= len(zeroed)
    for steps in ((2, 2), (4, 16), (6, 1280)):
        for window in (None, (0, 0, tile[0], h)):
            assert layers.split_frame(zeroed, 2, *steps, window) == layers.split_frame(canonical, 2, *steps, window)
    base, enh = layers.split_frame(zeroed, 2, 2, 2)
    assert base == canonical  # ratio 1: the canonical frame itself, and no residual
    assert int(np.frombuffer(enh, "<u4")[10]) == 0


def test_the_statement_refuses_what_the_device_reports():
    geom = GEOMS[1]
    w, h, tile, mv = geom
    rng = np.random.default_rng(5)
    fine, _, _ = fine_frame(rng, geom, 0.5, 2)
    offs = [0, len(fine)]
    count = int(np.frombuffer(fine, "<u4")[10])
    for word, value in ((0, 0x12345678), (1, 2), (2, w + tile[0]), (12, len(fine) + 16), (10, count + 1), (10, count - 1), (8, 4), (9, 4)):
        bad = np.frombuffer(fine, np.uint8).copy()
        bad[4 * word:4 * word + 4].view("<u4")[0] = value
        with pytest.raises(ValueError):
            layers.split_frame(bad, 2, 4, 16)
        with pytest.raises(ValueError):
            layers.split_frames(bad, offs, 2, 4, 16)
        with pytest.raises(ValueError):
            layers.split_budget_frames(bad, offs, 2, [(4, 16)], 1 << 20)
    with pytest.raises(ValueError, match="not \\(4, 4\\)"):
        layers.split_frame(fine, 4, 4, 16)
    with pytest.raises(ValueError, match="input frame"):
        layers.split_frames(fine, offs, 2, 4, 16, src=[0, 1])
    with pytest.raises(ValueError, match="multiples"):
        layers.split_frame(fine, 2, 4, 7)
    with pytest.raises(ValueError, match="int16"):
        layers.split_frame(fine, 2, 2, 2 * 32767)
    with pytest.raises(ValueError, match="positive"):
        layers.split_frame(fine, 2, 0, 4)
    with pytest.raises(ValueError, match="multiples"):
        layers.split_budget_frames(fine, offs, 2, [(2, 2), (4, 5)], 100)
    with pytest.raises(ValueError, match="non-decreasing"):
        layers.split_budget_frames(fine, offs, 2, [(4, 4), (2, 4)], 100)


# ---- odd ratios: the encoder's bytes ---------------------------------------------------------------------------------------------------------

def _quantise(coef, step):
    """The encoder's quantiser on f32 coefficients: f32 division, round half away from zero, clamped to int16."""
    q = coef / np.asarray(step, np.float32)
    assert q.dtype == np.float32
    return np.clip(np.sign(q) * np.floor(np.abs(q).astype(np.float64) + 0.5), -32768, 32767).astype(np.int64)


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2], GEOMS[4]], ids=_ids)
@pytest.mark.parametrize("steps", [(1, 639, 1), (3, 9, 1), (6, 30, 2), (15, 3, 3), (213, 1917, 3)], ids=str)
def test_odd_ratios_give_the_directly_quantised_frames(geom, steps):
    w, h, tile, mv = geom
    fg, bg, e = steps
    rng = np.random.default_rng(fg * 100 + bg + w)
    types = random_types(rng, w, h, mv)
    step = np.repeat(np.repeat(np.where(types == 0, bg, fg), mv[1], 0), mv[0], 1)[None]
    coef = (rng.standard_normal((3, h, w)) * rng.choice([0.7, 30.0, 900.0], (3, h, w))).astype(np.float32)
    # ... and coefficients at and next to the rounding boundaries of both quantisers
    ties = ((rng.integers(-40, 40, (3, h, w)) + 0.5) * np.where(rng.random((3, h, w)) < 0.5, e, step)).astype(np.float32)
    near = rng.random((3, h, w))
    ties = np.where(near < 0.3, np.nextafter(ties, np.float32(np.inf)), np.where(near < 0.6, np.nextafter(ties, np.float32(-np.inf)), ties))
    coef = np.where(rng.random((3, h, w)) < 0.5, coef, ties.astype(np.float32))
    lf, lb = _quantise(coef, e), _quantise(coef, step.astype(np.float32))
    g = geom_dict(*geom)
    fine, direct = layers.write_frame(g, types, lf, e, e), layers.write_frame(g, types, lb, fg, bg)
    for window in (None, _window("rect", 1, w, h, tile[0])[0]):
        base, enh = layers.split_frame(fine, e, fg, bg, window)
        assert base == direct  # no case is excused
        assert enh == layers.enhancement_frame(direct, fine, e, window)


def test_even_ratios_differ_from_a_direct_quantisation_only_at_ties_of_the_level():
    """What the header says of even ratios: the split rounds Lf = r / 2 (mod r) away from zero whatever the coefficient was; everywhere
    else it is the direct level, and its error against the fine reconstruction stays within sb / 2."""
    geom = GEOMS[4]
    w, h, tile, mv = geom
    rng = np.random.default_rng(3)
    types = random_types(rng, w, h, mv)
    for fg, bg, e in ((2, 2, 1), (16, 640, 1), (4, 16, 2)):
        step = np.repeat(np.repeat(np.where(types == 0, bg, fg), mv[1], 0), mv[0], 1)[None]
        coef = (rng.standard_normal((3, h, w)) * 40).astype(np.float32)
        lf, lb = _quantise(coef, e), _quantise(coef, step.astype(np.float32))
        base, _ = layers.split_frame(layers.write_frame(geom_dict(*geom), types, lf, e, e), e, fg, bg)
        got, _ = layers._levels_of(*levels.parse_frame(base))
        r = step // e
        differs = got != lb
        assert (np.abs(lf[differs]) % np.broadcast_to(r, lf.shape)[differs] == np.broadcast_to(r, lf.shape)[differs] // 2).all()
        assert (np.abs(got - lb) <= 1).all()
        if (fg, bg, e) == (2, 2, 1):
            assert differs.any()  # a quarter of the coefficients, on Gaussian data


# ---- the budget -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=_ids)
@pytest.mark.parametrize("e", [1, 2])
def test_budget_statement(geom, e):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w + e)
    frames = []
    for density in (0.3, 0.06, 1.0):  # magnitudes below 900: the ladder's ratios (up to 640) zero a good part of them
        lf = random_levels(rng, w, h, density)
        frames.append(layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), np.sign(lf) * (np.abs(lf) % 900), e, e))
    stream, offs = entropy._join(frames)
    ladder = [(int(fg) * e, int(bg) * e) for fg, bg in levels.step_ladder(1, 4, 1, 640, 6, 2)]
    sizes = [[len(layers.split_frame(fr, e, fg, bg)[0]) for fg, bg in ladder] for fr in frames]
    assert all(s == sorted(s, reverse=True) for s in sizes)
    floor = min(sizes[0])
    budgets = sorted({floor - 16, floor, *sizes[0], sizes[0][0] + 16, 0, 1 << 31})
    previous = None
    for budget in budgets:
        base, base_offs, enh, enh_offs, choice = layers.split_budget_frames(stream, offs, e, ladder, budget)
        picks = [int(c) & 0x7FFFFFFF for c in choice]
        for i, fr in enumerate(frames):
            fits = [k for k, s in enumerate(sizes[i]) if s <= budget]
            assert int(choice[i]) == (fits[0] if fits else (len(ladder) - 1) | 0x80000000)  # bit 31: even the last entry is over
            b, en = layers.split_frame(fr, e, *ladder[picks[i]])
            assert base[int(base_offs[i]):int(base_offs[i + 1])] == b and enh[int(enh_offs[i]):int(enh_offs[i + 1])] == en
        if previous is not None:
            assert all(p <= q for p, q in zip(picks, previous))  # monotone: more bytes, a finer (or the same) entry
        previous = picks
    assert int(layers.split_budget_frames(stream, offs, e, ladder, 0)[4][0]) >> 31 == 1
    # a one-entry ladder is the fixed statement, whatever the budget; windows and src pass through
    windows, src = [(0, 0, w // 2, h), (tile[0], 0, w, h), (0, 0, 0, 0), (0, 0, w, h)], [2, 0, 0, 1]
    want = layers.split_frames(stream, offs, e, 3 * e, 640 * e, windows, src)
    for budget in (0, 1 << 20):
        got = layers.split_budget_frames(stream, offs, e, [(3 * e, 640 * e)], budget, windows, src)
        assert got[0] == want[0] and got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
        assert [int(c) & 0x7FFFFFFF for c in got[4]] == [0] * 4
    # per-frame budgets: a repeated frame under two budgets takes two entries
    got = layers.split_budget_frames(stream, offs, e, ladder, [sizes[0][0], sizes[0][-1]], src=[0, 0])
    assert int(got[4][0]) == 0 and int(got[4][1]) > 0


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def test_workspace_queries_are_zero_where_the_calls_refuse():
    for q in (native.split_levels_workspace_bytes, lambda *a: native.split_levels_budget_workspace_bytes(*a, 8)):
        assert q(2, 2, 64, 72, 16, 16) == 0            # a frame the tile does not divide
        assert q(2, 2, 64, 64, 8, (12, 16)) == 0       # an MV block that is not a multiple of the tile
        assert q(2, 2, 256, 256, 128, 128) == 0        # a tile of more than 4096 coefficients
        assert q(70000, 2, 64, 64, 8, 16) == 0         # more frames than one call takes, in
        assert q(2, 70000, 64, 64, 8, 16) == 0         # ... or out
        assert q(2, 2, 64, 64, 8, 16) > 0
        assert q(2, 2, 64, 64, 4, 16) > 0              # not limited to the 8 / 16 transform
        assert q(2, 2, 128, 64, 64, 64) > 0
        assert q(2, 2, 36, 24, 12, 12) > 0
        assert q(2, 4, 64, 64, 8, 16) > q(2, 2, 64, 64, 8, 16) == q(9, 2, 64, 64, 8, 16)  # sized by n_out
    b = native.split_levels_budget_workspace_bytes
    assert b(2, 2, 64, 64, 8, 16, 0) == 0 and b(2, 2, 64, 64, 8, 16, 65) == 0
    assert b(2, 2, 64, 64, 8, 16, 64) > b(2, 2, 64, 64, 8, 16, 1) > native.split_levels_workspace_bytes(2, 2, 64, 64, 8, 16)


def _ladder(pairs):
    return (native.StepPair * max(1, len(pairs)))(*[native.StepPair(fg, bg) for fg, bg in pairs])


def _host_aligned(nbytes, align, skew=0):
    buf = (native.C.c_uint8 * (nbytes + 2 * align))()
    base = native.C.addressof(buf)
    return buf, (base + align - 1) // align * align + skew


def test_argument_checks_answer_without_a_device():
    """Every device pointer is NULL (but d_enh_out where its capacity is checked: a host address stands in, as in the alignment test):
    each check below comes before the pointer checks, and the null-pointer check stands between all of them and a launch -- a missing
    or reordered check fails this test (its message differs) without reaching a kernel."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def fixed(w, h, bw, bh, mbw, mbh, n_in=2, n_out=2, src=None, steps=(2, 4, 16), ws=1 << 40, cap=1 << 40, ecap=1 << 40, enh=None):
        return lib.svc_hip_split_levels_frames(None, 0, None, n_in, src, n_out, w, h, bw, bh, mbw, mbh, *steps, None, None, ws, None, cap,
                                               None, enh, ecap, None, None, None)

    def budgeted(w, h, bw, bh, mbw, mbh, n_in=2, n_out=2, src=None, steps=(2, 4, 16), ws=1 << 40, cap=1 << 40, ecap=1 << 40, ladder=None,
                 enh=None):
        pairs = [(steps[1], steps[2])] if ladder is None else ladder
        return lib.svc_hip_split_levels_budget_frames(None, 0, None, n_in, src, n_out, w, h, bw, bh, mbw, mbh, steps[0], _ladder(pairs),
                                                      len(pairs), None, None, None, ws, None, cap, None, enh, ecap, None, None, None, None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    some_src = (native.C.c_uint32 * 8)()
    keep, some_enh = _host_aligned(64, 16)
    for call, query in ((fixed, native.split_levels_workspace_bytes),
                        (budgeted, lambda *a: native.split_levels_budget_workspace_bytes(*a, 1))):
        for n in (2, 0):  # the contract does not depend on the frame counts
            assert call(100, 64, 8, 8, 16, 16, n, n) == bad and "not divisible" in err()
            assert call(64, 64, 8, 8, 12, 16, n, n) == bad and "multiple of the tile" in err()
            # geometry before the steps
            assert call(100, 64, 8, 8, 16, 16, n, n, steps=(0, 4, 16)) == bad and "not divisible" in err()
            # the steps: a zero, a non-multiple, a ratio of 32767 -- before the limits
            for steps in ((0, 4, 16), (2, 0, 16), (2, 4, 0)):
                assert call(64, 64, 8, 8, 16, 16, 70000, n, steps=steps) == bad and "positive" in err()
            assert call(64, 64, 8, 8, 16, 16, 70000, n, steps=(2, 4, 7)) == bad and "multiples of fine_step" in err()
            assert call(64, 64, 8, 8, 16, 16, 70000, n, steps=(4, 2, 8)) == bad and "multiples of fine_step" in err()
            assert call(64, 64, 8, 8, 16, 16, 70000, n, steps=(2, 2, 2 * 32767)) == unsup and "int16" in err()
            assert call(256, 256, 128, 128, 128, 128, n, n, steps=(2, 2 * 32767, 2 * 32767)) == unsup and "int16" in err()
            # limits before the d_src rule, for either count
            assert call(256, 256, 128, 128, 128, 128, n, n + 1) == unsup and "4096" in err()
            assert call(64, 64, 8, 8, 16, 16, n, 70000) == unsup and "65535 frames" in err()
            assert call(64, 64, 8, 8, 16, 16, 70000, n, src=some_src) == unsup and "65535 frames" in err()
            # the d_src rule before workspace and capacity
            assert call(64, 64, 8, 8, 16, 16, n, n + 1, ws=0, cap=0) == bad and "d_src" in err()
            assert call(64, 64, 8, 8, 16, 16, n + 3, n, ws=0, cap=0) == bad and "d_src" in err()
        assert call(64, 64, 8, 8, 16, 16, 65535, 65535, steps=(1, 1, 32766), ws=0, cap=0) == bad and "workspace" in err()  # the largest pass
        need_ws, need_out = query(2, 2, 64, 64, 8, 16), native.levels_max_bytes(2, 64, 64, 8, 16)
        assert need_ws > 0 and need_out > 0
        assert call(64, 64, 8, 8, 16, 16, ws=need_ws - 1, cap=0, ecap=0) == bad and "workspace" in err()          # workspace before capacity
        assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out - 16, ecap=8, enh=some_enh) == bad and "base output" in err()  # base first
        assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out, ecap=need_out - 16, enh=some_enh) == bad and "enhancement output" in err()
        assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out, ecap=need_out, enh=some_enh) == bad and "null pointer" in err()
        for ecap in (0, 8, need_out - 16, need_out):  # base only: no second capacity, whatever is passed for it
            assert call(64, 64, 8, 8, 16, 16, ws=need_ws, cap=need_out, ecap=ecap) == bad and "null pointer" in err()
        # the sizes follow n_out, not n_in
        need_ws3 = query(2, 3, 64, 64, 8, 16)
        assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3 - 1, cap=0) == bad and "workspace" in err()
        assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out) == bad and "base output" in err()
        assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out // 2 * 3, ecap=need_out, enh=some_enh) == bad and "enhancement" in err()
        assert call(64, 64, 8, 8, 16, 16, 2, 3, src=some_src, ws=need_ws3, cap=need_out // 2 * 3, ecap=need_out // 2 * 3, enh=some_enh) == bad and "null pointer" in err()
        # an empty batch is valid with sizes of 0, before any pointer, with and without d_src
        assert call(64, 64, 8, 8, 16, 16, 0, 0, ws=0, cap=0, ecap=0) == native.SVC_OK
        assert call(64, 64, 8, 8, 16, 16, 5, 0, src=some_src, ws=0, cap=0, ecap=0) == native.SVC_OK
        assert call(36, 24, 12, 12, 12, 12, 0, 0, ws=0, cap=0, ecap=0) == native.SVC_OK
    # the ladder's own rules, where the fixed call has its steps
    assert lib.svc_hip_split_levels_budget_frames(None, 0, None, 2, None, 2, 64, 64, 8, 8, 16, 16, 2, None, 0, None, None, None, 0, None, 0,
                                                  None, None, 0, None, None, None, None) == bad and "ladder of 0" in err()
    assert budgeted(64, 64, 8, 8, 16, 16, ladder=[(2, 2)] * 65) == bad and "ladder of 65" in err()
    assert budgeted(64, 64, 8, 8, 16, 16, ladder=[(4, 4), (2, 4)]) == bad and "non-decreasing" in err()
    assert budgeted(64, 64, 8, 8, 16, 16, ladder=[(2, 2), (4, 5)]) == bad and "entry 1" in err() and "multiples" in err()
    assert budgeted(64, 64, 8, 8, 16, 16, ladder=[(2, 2), (2, 2 * 32767)]) == unsup and "int16" in err()
    assert budgeted(64, 64, 8, 8, 16, 16, ladder=[(2, 2), (2, 2 * 32766)], ws=0) == bad and "workspace" in err()
    del keep


def test_alignment_is_checked_after_the_null_pointers_and_before_any_launch():
    """Host addresses stand in for device pointers: the alignment check refuses before anything is enqueued."""
    lib = native.load()
    need_ws, need_out = native.split_levels_workspace_bytes(2, 2, 64, 64, 8, 16), native.levels_max_bytes(2, 64, 64, 8, 16)
    keep, p = _host_aligned(64, 16)
    for skew in ({"frames": 4}, {"base": 8}, {"enh": 4}, {"ws": 8}, {"offs": 4}, {"boffs": 4}, {"eoffs": 4}, {"status": 2}, {"window": 2},
                 {"src": 1}):
        at = lambda k: p + skew.get(k, 0)
        rc = lib.svc_hip_split_levels_frames(at("frames"), 0, at("offs"), 2, at("src"), 2, 64, 64, 8, 8, 16, 16, 2, 4, 16, at("window"), at("ws"),
                                             need_ws, at("base"), need_out, at("boffs"), at("enh"), need_out, at("eoffs"), at("status"), None)
        assert rc == native.SVC_ERR_INVALID_ARG and "aligned" in lib.svc_hip_last_error().decode(), skew
    # an enhancement stream without its offsets
    rc = lib.svc_hip_split_levels_frames(p, 0, p, 2, None, 2, 64, 64, 8, 8, 16, 16, 2, 4, 16, None, p, need_ws, p, need_out, p, p, need_out,
                                         None, p, None)
    assert rc == native.SVC_ERR_INVALID_ARG and "null pointer" in lib.svc_hip_last_error().decode()
    del keep


def test_the_abi_version_did_not_move():
    assert native.load().svc_hip_abi_version() == 5
