"""svc_hip_pack_layers_frames (include/svc_hip.h: both layers of the gaze-scalable stream from raw coefficient planes, for any geometry)
without a device: the numpy statement (scalable_video_codec_amd/layers.py: pack_layers_frames) on seeded random in-range planes against
the statements that exist -- write_frame, enhancement_frames, merge_levels -- and the order of the C ABI's argument checks.  The bytes the
kernels write are tests/test_gpu_pack_layers.py, which takes its planes and its refusals from here."""
from __future__ import annotations

import numpy as np
import pytest

from scalable_video_codec_amd import layers, levels, native
from tests.test_window_levels_host import GEOMS, _ids, geom_dict, random_types

STEPS = [(1, 640, 1), (4, 16, 2), (3, 9, 1), (2, 2, 2)]
N = 4


def random_planes(rng, n, w, h, tile, density=0.3, steps=(4, 16, 2)):
    """(n, 3, h, w) f32 raw 'coefficients' within the transform's bound |c| <= 255 * sqrt(tile area): a `density` share of them drawn
    over the whole range, an eighth of those moved onto exact ties of one of the steps ((k + 1/2) * step, exact in f32), the rest 0 or,
    for one in sixteen, a value below half the finest step (a level of 0 that is inexact)."""
    bound = 255.0 * np.sqrt(tile[0] * tile[1])
    shape = (n, 3, h, w)
    c = rng.uniform(-bound, bound, shape) * (rng.random(shape) < 0.5) + rng.uniform(-40, 40, shape) * (rng.random(shape) < 0.5)
    tie_step = rng.choice(np.array(steps, np.float64), shape)
    ties = (rng.integers(-40, 40, shape) + 0.5) * tie_step
    c = np.where(rng.random(shape) < 0.125, ties, c)
    c = np.where(rng.random(shape) < density, c, np.where(rng.random(shape) < 1 / 16, rng.uniform(-0.49, 0.49, shape) * min(steps), 0.0))
    return np.clip(c, -bound, bound).astype(np.float32)


def windows_of(rng, n, w, h, tile):
    """None, or per frame: the whole frame, nothing, a rectangle whose edges fall inside tiles, one past the frame."""
    return [None, [(0, 0, w, h), (0, 0, 0, 0), (tile[0] // 2, 1, w // 2, h), (w - tile[0], h - tile[1], 4 * w, 1 << 31)][:n]]


def _round_half_away(q):
    """Independent of layers.quantise: by cases on the sign, on the f32 quotient held in f64."""
    q = q.astype(np.float64)
    return np.where(q >= 0, np.floor(q + 0.5), np.ceil(q - 0.5))


def base_levels(planes, types, geom, fg, bg):
    w, h, tile, mv = geom
    step = np.repeat(np.repeat(np.where(types == 0, bg, fg), mv[1], 0), mv[0], 1).astype(np.float32)
    # (a tile's class is its origin's MV block: the MV block is a multiple of the tile, so per pixel is per tile)
    q = planes / step[None]
    assert q.dtype == np.float32
    return np.clip(_round_half_away(q), -32768, 32767).astype(np.int64), step


@pytest.mark.parametrize("steps", STEPS, ids=str)
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_statement_against_the_existing_statements(geom, steps):
    w, h, tile, mv = geom
    fg, bg, e = steps
    g = geom_dict(*geom)
    rng = np.random.default_rng(w * 31 + h + fg)
    planes = random_planes(rng, N, w, h, tile, steps=steps)
    types = np.stack([random_types(rng, w, h, mv) for _ in range(N)])
    fine, fine_offs, fine_enh, fine_eoffs, _ = layers.pack_layers_frames(planes, types, g, e, e, e)
    for windows in windows_of(rng, N, w, h, tile):
        base, boffs, enh, eoffs, inexact = layers.pack_layers_frames(planes, types, g, fg, bg, e, windows)
        assert len(boffs) == len(eoffs) == N + 1 and int(boffs[-1]) == len(base) and int(eoffs[-1]) == len(enh)
        want_base = []
        for f in range(N):
            lb, step = base_levels(planes[f], types[f], geom, fg, bg)
            ix = int((planes[f] != lb.astype(np.float32) * step[None]).sum())
            assert ix == int(inexact[f]) and ix > 0  # raw planes: word 11 is not 0
            want_base.append(layers.write_frame(g, types[f], lb, fg, bg, ix))
        assert base == b"".join(want_base)
        want_enh, want_eoffs = layers.enhancement_frames(base, boffs, fine, fine_offs, e, windows)
        assert enh == want_enh and [int(o) for o in eoffs] == [int(o) for o in want_eoffs]
        # what the decoder dequantises under a whole-frame gaze: Lf inside the window, Lb * ratio outside it
        for f in range(N):
            bf, ef = base[int(boffs[f]):int(boffs[f + 1])], enh[int(eoffs[f]):int(eoffs[f + 1])]
            he = levels.parse_frame(ef)[0]
            assert (he["fg_step"], he["bg_step"], he["inexact"]) == (e, e, 0) and ef[52:64] == bytes(12)
            merged, _ = layers.merge_levels(bf, ef, (0, 0, w, h))
            lb, step = base_levels(planes[f], types[f], geom, fg, bg)
            lf, _ = base_levels(planes[f], types[f], geom, e, e)
            inside = np.ones((h, w), bool)
            if windows is not None:
                _, ox, oy = layers._tile_maps(g, types[f])
                inside = layers._per_pixel(g, layers._contains(windows[f], ox, oy))
            assert np.array_equal(merged, np.where(inside[None], lf, lb * (step.astype(np.int64) // e)[None]))
    # the fine statement's own enhancement, and any ratio of 1, is empty
    assert all(h_["level_count"] == 0 for h_, _, _ in levels.iter_frames(fine_enh, fine_eoffs))
    if fg == bg == e:
        assert len(enh) == len(fine_enh) and enh == fine_enh


def test_ties_round_away_from_zero_and_the_clamp_holds():
    c = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, -0.49999997, 8388609.0, -8388609.0, 1e9, -1e9], np.float32)
    assert layers.quantise(c, 1).tolist() == [1, -1, 2, -2, 3, 0, 0, 32767, -32768, 32767, -32768]
    assert layers.quantise(np.array([3.0, -3.0, 9.0, 2.9999998], np.float32), 6).tolist() == [1, -1, 2, 0]


def test_the_statement_refuses_steps_that_do_not_divide():
    g = geom_dict(*GEOMS[0])
    planes = np.zeros((1, 3, 12, 36), np.float32)
    types = np.zeros((1, 1, 3), np.uint32)
    for steps in ((4, 6, 4), (0, 4, 2), (4, 4, 0), (4, 4, 8)):
        with pytest.raises(ValueError):
            layers.pack_layers_frames(planes, types, g, *steps)


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.pack_layers_workspace_bytes
    assert q(2, 64, 72, 16) == 0                # a frame the tile does not divide
    assert q(2, 256, 256, 128) == 0             # a tile of more than 4096 coefficients
    assert q(70000, 64, 64, 8) == 0             # more frames than one call takes
    assert q(2, 64, 64, 8) > 0
    assert q(2, 64, 64, (8, 4)) > 0             # non-square
    assert q(2, 128, 64, 64) > 0
    assert q(2, 36, 24, 12) > 0
    assert q(4, 64, 64, 8) > q(2, 64, 64, 8)


def check_refusals(planes=None, types=None, workspace=None, base=None, boffs=None, enh=None, eoffs=None):
    """Every refusal of svc_hip_pack_layers_frames in its order.  With every pointer None (this file) each check comes before the pointer
    checks and the null-pointer check stands between all of them and a launch; tests/test_gpu_pack_layers.py passes device pointers of
    a 64 x 64 frame of 8 x 8 tiles, 2 frames, so the same calls also show that a refused call wrote nothing."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w=64, h=64, bw=8, bh=8, mbw=16, mbh=16, n=2, steps=(4, 16, 2), ws=1 << 40, bcap=1 << 40, ecap=1 << 40, window=None, ptrs=True):
        p = (planes, types, workspace, base, boffs, enh, eoffs) if ptrs else (None,) * 7
        return lib.svc_hip_pack_layers_frames(p[0], p[1], n, w, h, bw, bh, mbw, mbh, *steps, window, p[2], ws, p[3], bcap, p[4], p[5], ecap,
                                              p[6], None)
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):  # the contract does not depend on the frame count
        assert call(100, 64, n=n) == bad and "not divisible" in err()
        assert call(mbw=12, n=n) == bad and "multiple of the tile" in err()
        # geometry before steps
        assert call(100, 64, n=n, steps=(0, 16, 2)) == bad and "not divisible" in err()
        # steps: a step of 0, a base step that enh_step does not divide
        for steps in ((0, 16, 2), (4, 0, 2), (4, 16, 0)):
            assert call(n=n, steps=steps) == bad and "must be positive" in err()
        assert call(n=n, steps=(4, 6, 4)) == bad and "multiple of enh_step" in err()
        assert call(n=n, steps=(4, 4, 8)) == bad and "multiple of enh_step" in err()
        # steps before the int16 bounds and the limits
        assert call(256, 256, 256, 128, 256, 128, n=70000, steps=(1, 3, 2)) == bad and "multiple of enh_step" in err()
    for n in (2, 0):
        # 255 * sqrt(64 * 64) / 1 = 16320 fits; 255 * sqrt(128 * 128) = 32640 fits too, 255 * sqrt(128 * 256) does not
        assert call(256, 256, 256, 128, 256, 128, n=n, steps=(1, 1, 1)) == unsup and "exceed int16" in err()
        assert call(n=n, steps=(32767, 32767, 1)) == unsup and "32766 times" in err()
        assert call(n=n, steps=(4, 32767 * 2, 2)) == unsup and "32766 times" in err()
        # the bounds before the limits (a tile above 4096 coefficients whose levels fit is the limits' refusal)
        assert call(256, 256, 128, 128, 128, 128, n=n, steps=(2, 2, 2)) == unsup and "4096" in err()
        assert call(256, 256, 256, 128, 256, 128, n=70000, steps=(1, 1, 1)) == unsup and "exceed int16" in err()
        # limits before the sizes
        assert call(n=70000, ws=0, bcap=0, ecap=0) == unsup and "65535 frames" in err()
    need_ws = native.pack_layers_workspace_bytes(2, 64, 64, 8)
    need = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert need_ws > 0 and need > 0
    # workspace, then the base's capacity, then the enhancement's
    assert call(ws=need_ws - 1, bcap=0, ecap=0) == bad and "workspace" in err()
    assert call(ws=need_ws, bcap=need - 1, ecap=0) == bad and "base output" in err()
    assert call(ws=need_ws, bcap=need, ecap=need - 1) == bad and "enhancement output" in err()
    assert call(n=65535, ws=0) == bad and "workspace" in err()  # the largest count passes the limits
    # an empty batch is no error, with no pointer at all; a batch with frames reaches the pointer check
    assert call(n=0, ws=0, bcap=0, ecap=0, ptrs=False) == native.SVC_OK
    assert call(ws=need_ws, bcap=need, ecap=need, ptrs=False) == bad and "null pointer" in err()


def test_argument_checks_answer_without_a_device():
    check_refusals()
