"""The inputs of tests/test_gpu_transform_exact.py, seeded, so that tests/test_transform_ref.py can check on the CPU what
the GPU tests assume about them (ambiguous shares, ties and near-ties the reference finds in them)."""
import numpy as np

GENERAL_BLOCKS = [(4, 4), (2, 2), (16, 8), (8, 16), (32, 32), (2, 16), (64, 64), (8, 1), (1, 4), (6, 10), (8, 8)]
# width in tiles and height in tiles for each: the width is wider than one strip of dct_general_kernel (sw = min(4096 / area, w / bw)
# tiles) and not a whole number of strips, so the last strip of every band is narrower than sw -- except 64 x 64, whose strip is one tile.
# 8 x 8 at 536 = 16 * 33.5 pixels is the general kernel's only way to a tuned shape (16 x 16 needs a width that is a multiple of 16,
# which is the tuned kernel's condition).
GENERAL_TILES = {(4, 4): (300, 4), (2, 2): (1100, 3), (16, 8): (35, 8), (8, 16): (37, 4), (32, 32): (7, 19), (2, 16): (150, 3),
                 (64, 64): (12, 11), (8, 1): (520, 3), (1, 4): (1100, 3), (6, 10): (75, 3), (8, 8): (67, 3)}


def general_strip(bw: int, bh: int, w: int) -> int:
    """launch_dct_general's strip width."""
    tiles = max(1, 4096 // (bw * bh))
    return min(tiles, w // bw) * bw


def special_tiles(bw: int, bh: int, seed: int):
    """(bh, bw, 3) u8 tiles a transform can be wrong at: one 255 at each position (every basis entry of both passes on its own; a
    seeded sample of 256 positions with the four corners above 16 x 16), saturated, zero, and the two 0 / 255 checkerboards
    (largest DC, largest highest-frequency term).  The channels of an impulse tile carry different positions."""
    rng = np.random.default_rng(seed)
    area = bw * bh
    if area <= 256:
        pos = np.arange(area)
    else:
        corners = np.array([0, bw - 1, area - bw, area - 1])
        rest = np.setdiff1d(np.arange(area), corners)
        pos = np.concatenate([corners, rng.choice(rest, 252, replace=False)])
    tiles = []
    for i, p in enumerate(pos):
        t = np.zeros((bh, bw, 3), np.uint8)
        for c in range(3):
            q = pos[(i + 17 * c) % len(pos)]
            t[q // bw, q % bw, c] = 255
        tiles.append(t)
    tiles.append(np.full((bh, bw, 3), 255, np.uint8))
    tiles.append(np.zeros((bh, bw, 3), np.uint8))
    yy, xx = np.mgrid[0:bh, 0:bw]
    for phase in (0, 1):
        tiles.append(np.repeat((((yy + xx + phase) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    return tiles


def smooth_frames(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """Box-filtered noise (9 x 9 mean, zero padded, rounded): small AC coefficients, where an f32 ulp is far below 1e-4."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, h + 8, w + 8, 3)).astype(np.float64)
    x[:, :4] = 0; x[:, -4:] = 0; x[:, :, :4] = 0; x[:, :, -4:] = 0
    c = np.cumsum(np.cumsum(np.pad(x, ((0, 0), (1, 0), (1, 0), (0, 0))), axis=1), axis=2)
    s = c[:, 9:, 9:] - c[:, :-9, 9:] - c[:, 9:, :-9] + c[:, :-9, :-9]
    return np.rint(s / 81.0).astype(np.uint8)


def structured_frames(bw: int, bh: int, n: int, tiles_x: int, tiles_y: int, seed: int):
    """n frames of tiles_x x tiles_y tiles: random bytes, the last frame smooth, and the special tiles scattered over all frames
    (tile i of the list at tile index i * stride mod total, stride coprime to total) so that they meet different lanes, segment
    columns and workgroups.  -> (frames u8 (n, H, W, 3), special mask (n, H, W) bool)."""
    rng = np.random.default_rng(seed)
    h, w = tiles_y * bh, tiles_x * bw
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames[-1] = smooth_frames(1, h, w, seed + 1)[0]
    special = special_tiles(bw, bh, seed + 2)
    total = n * tiles_x * tiles_y
    assert total >= len(special) + n, (total, len(special))
    stride = next(s for s in range(max(1, int(total * 0.382)), total + 2) if np.gcd(s, total) == 1)  # a permutation of the tile indices
    mask = np.zeros((n, h, w), bool)
    for i, t in enumerate(special):
        g = (i * stride) % total
        f, r = divmod(g, tiles_x * tiles_y)
        ty, tx = divmod(r, tiles_x)
        frames[f, ty * bh:(ty + 1) * bh, tx * bw:(tx + 1) * bw] = t
        mask[f, ty * bh:(ty + 1) * bh, tx * bw:(tx + 1) * bw] = True
    return frames, mask


# ---- the tuned kernels' placement case -------------------------------------------------------------------------------------------
# N = 8: 3 frames of 176 x 48 -- 11 segment columns per band, 66 per frame, 198 in all = 6.19 workgroups of 32.
# N = 16: 3 frames of 224 x 160 -- 14 segment columns per band, 140 per frame, 420 in all = 26.25 workgroups of 16.
# Neither a band nor a frame is a whole number of workgroups, so a workgroup's segment columns straddle bands and frames; the last
# workgroup is partial; 7 and 27 workgroups are not multiples of 8 (xcd_contiguous_block's uneven case).  Both sizes are whole MV
# blocks of twice the tile.
TUNED_PLACEMENT = {8: (3, 22, 6), 16: (3, 14, 10)}  # block -> (frames, tiles_x, tiles_y)


def tuned_placement_frames(block: int):
    n, tx, ty = TUNED_PLACEMENT[block]
    return structured_frames(block, block, n, tx, ty, 9000 + block)


def tuned_work_split(block: int, n: int, h: int, w: int):
    """(segment columns, workgroups, segment columns per workgroup) of dct_kernel<block>."""
    seg = n * (w // 16) * (h // block)
    per = 256 // block
    return seg, -(-seg // per), per


def general_frames(bw: int, bh: int):
    tx, ty = GENERAL_TILES[(bw, bh)]
    return structured_frames(bw, bh, 2, tx, ty, 7000 + 100 * bw + bh)


# ---- the fused forms' coverage case: about two 1080p frames of random bytes per form -------------------------------------------------
# 1904 = 16 * 119 pixels wide (119 segment columns per band: odd), 1088 tall: 2 * 119 * 136 = 32 368 segment columns = 1011.5
# workgroups at N = 8 and 2 * 119 * 68 = 16 184 = 1011.5 at N = 16 (last workgroup partial, 1012 = 4 mod 8).  The general form runs
# 4 x 4 (rational coefficients at {0, 2}^2, so exact ties exist) at 1900 x 1080 with 20 x 20 MV blocks: strips of 1024 and 876 columns.
COVERAGE = {"tuned8": dict(block=(8, 8), n=2, h=1088, w=1904, mv=(16, 16), seed=811),
            "tuned16": dict(block=(16, 16), n=2, h=1088, w=1904, mv=(16, 16), seed=1611),
            "general": dict(block=(4, 4), n=2, h=1080, w=1900, mv=(20, 20), seed=411)}
COVERAGE_STEPS = ((1, 3), (3, 7), (7, 640))  # (fg, bg) of the calls: every coefficient meets 3 and 7, and one of 1 and 640


def coverage_case(form: str):
    """-> (frames u8, types u32 (n, blocks), spec)"""
    c = COVERAGE[form]
    rng = np.random.default_rng(c["seed"])
    frames = rng.integers(0, 256, (c["n"], c["h"], c["w"], 3), dtype=np.uint8)
    blocks = (c["w"] // c["mv"][0]) * (c["h"] // c["mv"][1])
    types = (rng.integers(1, 40, (c["n"], blocks)) * (rng.random((c["n"], blocks)) < 0.5)).astype(np.uint32)
    return frames, types, c


def step_plane(types, w: int, h: int, mv, fg: int, bg: int) -> np.ndarray:
    """(H, W) u32: the quantiser step of every position of one frame (region id 0 = background, libs/decoder.cpp:130-135)."""
    mvw, mvh = mv
    t = np.asarray(types).reshape(h // mvh, w // mvw)
    s = np.where(t == 0, bg, fg).astype(np.uint32)
    return np.repeat(np.repeat(s, mvh, axis=0), mvw, axis=1)


def tie_census(lo, hi, qlo, qhi, steps, s: int) -> dict:
    """What the reference alone says about the positions quantised with step s: how many are ambiguous (quant(lo) != quant(hi)), and
    among the others how many are exact rounding ties of c / s per sign and how many non-exact near-ties (within 4 f32 ulps)."""
    from tests.helpers import transform_ref as tr
    at = steps == s
    amb = at & (qlo != qhi)
    sure = at & (lo == hi)
    c = lo[sure].astype(np.float64)
    exact = np.fmod(2.0 * np.abs(c), 2.0 * s) == float(s)  # |c| = (k + 1/2) s, exactly (fmod is exact)
    near = tr.near_half(c / s) & ~exact
    return dict(step=s, positions=int(at.sum()), ambiguous=int(amb.sum()), ties_pos=int((exact & (c > 0)).sum()),
                ties_neg=int((exact & (c < 0)).sum()), near_ties=int(near.sum()))


def add_census(total: dict, one: dict) -> None:
    """Sums tie_census results per step (the calls of a form quantise disjoint positions with a given step)."""
    t = total.setdefault(one["step"], {k: 0 for k in one if k != "step"})
    for k in t:
        t[k] += one[k]
