"""Two layers decoded at reduced size, without a GPU: the identities of the numpy statement (layers.reduced_coefficients,
layers.decode_layers_reduced_frame) against the one-stream statement (levels.reduced_coefficients), against layers.merge_levels at
reduce = 1 and through the band call's statement; and the argument checks of svc_hip_decode_layers_reduced_frames that answer before any
device work.  Frames come from seeded random coefficient planes through layers.pack_layers_frames."""
import numpy as np
import pytest

from scalable_video_codec_amd import layers, levels, native

W, H, N_FRAMES = 128, 64, 3
CASES = [(8, 16, (4, 16, 1)), (8, 32, (4, 16, 2)), (16, 16, (4, 16, 2)), (16, 32, (6, 18, 3))]  # block, MV block, (fg, bg, enh)
REDUCES = [1, 2, 4, 8]
WINDOW = (24, 8, 56, 40)   # its edges inside tiles: it cuts the one group of an 8 x 8 tile row and both groups of a 16 x 16 one
GAZE = (8, 0, 72, 48)      # holds tiles inside the window and tiles outside it, and leaves tiles of both kinds out


def _geometry(block, mv_block):
    return {"frame_w": W, "frame_h": H, "block_w": block, "block_h": block, "mv_block_w": mv_block, "mv_block_h": mv_block}


def _planes(rng, block):
    """Coefficient planes whose amplitude falls with the frequency, as a transform's do: levels in and outside every K x K."""
    r = np.arange(H)[:, None] % block
    c = np.arange(W)[None, :] % block
    amp = 900.0 / (1.0 + r + c) ** 1.5
    return (rng.standard_normal((N_FRAMES, 3, H, W)) * amp).astype(np.float32)


_cache = {}


def _pair(block, mv_block, steps, windowed):
    """-> (geometry, base frames, enhancement frames, the frames written at (e, e)), each a list of N_FRAMES u8 arrays."""
    key = (block, mv_block, steps, windowed)
    if key not in _cache:
        fg, bg, e = steps
        rng = np.random.default_rng(block * 1000 + mv_block * 10 + e)
        geo = _geometry(block, mv_block)
        types = rng.integers(0, 3, (N_FRAMES, H // mv_block, W // mv_block)).astype(np.uint32)
        planes = _planes(rng, block)
        base, bo, enh, eo, _ = layers.pack_layers_frames(planes, types, geo, fg, bg, e, [WINDOW] * N_FRAMES if windowed else None)
        cut = lambda s, o: [np.frombuffer(s, np.uint8)[int(o[i]):int(o[i + 1])] for i in range(N_FRAMES)]
        fine = [np.frombuffer(layers.write_frame(geo, types[f], layers.quantise(planes[f], e), e, e), np.uint8) for f in range(N_FRAMES)]
        _cache[key] = (geo, cut(base, bo), cut(enh, eo), fine)
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tiles_in(rect, block, k):
    """(H k / N, W k / N) bool: is the origin of the coefficient's tile inside the rectangle (full-size padded coordinates)?"""
    oy, ox = (np.arange(H // block) * block)[:, None], (np.arange(W // block) * block)[None, :]
    x, y, w, h = rect
    inside = (ox >= x) & (ox - x < w) & (oy >= y) & (oy - y < h)
    return np.repeat(np.repeat(inside, k, 0), k, 1)


@pytest.mark.parametrize("block,mv_block,steps", CASES)
@pytest.mark.parametrize("reduce", REDUCES)
def test_without_a_gaze_it_is_the_base(block, mv_block, steps, reduce):
    _, base, enh, _ = _pair(block, mv_block, steps, False)
    for b, e in zip(base, enh):
        want = levels.reduced_coefficients(b, reduce, 3, 17)
        assert np.array_equal(_bits(layers.reduced_coefficients(b, e, reduce, 3, 17)), _bits(want))
        assert np.array_equal(_bits(layers.reduced_coefficients(b, None, reduce, 3, 17)), _bits(want))  # the enhancement is not read
        assert np.array_equal(_bits(layers.reduced_coefficients(b, e, reduce, 3, 17, (5, 5, 0, 7))), _bits(want))  # a gaze that holds nothing
        assert np.array_equal(layers.decode_layers_reduced_frame(b, e, reduce, 3, 17), levels.decode_reduced_frame(b, reduce, 3, 17))


@pytest.mark.parametrize("block,mv_block,steps", CASES)
@pytest.mark.parametrize("reduce", REDUCES)
def test_every_tile_gazed_is_the_stream_written_at_the_enhancement_step(block, mv_block, steps, reduce):
    _, base, enh, fine = _pair(block, mv_block, steps, False)
    whole = (0, 0, W, H)
    for b, e, f in zip(base, enh, fine):
        got = layers.reduced_coefficients(b, e, reduce, 3, 17, whole)
        assert got.shape == (3, H // reduce, W // reduce) and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(levels.reduced_coefficients(f, reduce, 3, 17, whole)))
        assert not np.array_equal(_bits(got), _bits(levels.reduced_coefficients(b, reduce, 3, 17, whole)))  # the residuals show
        pic = layers.decode_layers_reduced_frame(b, e, reduce, 3, 17, whole)
        assert pic.shape == (H // reduce, W // reduce, 3) and pic.dtype == np.float64
        assert np.array_equal(pic, levels.decode_reduced_frame(f, reduce, 3, 17, whole))


@pytest.mark.parametrize("block,mv_block,steps", CASES)
@pytest.mark.parametrize("windowed", [False, True])
def test_reduce_one_is_merge_levels_requantised(block, mv_block, steps, windowed):
    geo, base, enh, _ = _pair(block, mv_block, steps, windowed)
    fg, bg = 3, 17
    for b, e in zip(base, enh):
        merged, step = layers.merge_levels(b, e, GAZE)
        _, types, _ = levels.parse_frame(b)
        background, ox, oy = layers._tile_maps(geo, types)
        gazed = layers._contains(GAZE, ox, oy)
        dec = np.where(gazed, 1, np.where(background, bg, fg))
        c = merged.astype(np.float32) * layers._per_pixel(geo, step)[None].astype(np.float32)
        s = layers._per_pixel(geo, dec)[None].astype(np.float32)
        q = (c / s).astype(np.float32).astype(np.float64)
        want = (np.copysign(np.floor(np.abs(q) + 0.5), q).astype(np.float32) * s).astype(np.float32)
        assert np.array_equal(_bits(layers.reduced_coefficients(b, e, 1, fg, bg, GAZE)), _bits(want))


@pytest.mark.parametrize("block,mv_block,steps", CASES)
@pytest.mark.parametrize("reduce", REDUCES)
def test_tile_by_tile_with_a_window_and_a_gaze(block, mv_block, steps, reduce):
    """Inside gaze and window: the stream written at (e, e); everywhere else -- outside the gaze, and inside it but outside the window --
    the base under the same gaze."""
    _, base, enh, fine = _pair(block, mv_block, steps, True)
    k = block // reduce
    both = _tiles_in(GAZE, block, k) & _tiles_in(WINDOW, block, k)
    only_gaze = _tiles_in(GAZE, block, k) & ~_tiles_in(WINDOW, block, k)
    assert both.any() and only_gaze.any() and not _tiles_in(GAZE, block, k).all()
    differs = False
    for b, e, f in zip(base, enh, fine):
        got = layers.reduced_coefficients(b, e, reduce, 3, 17, GAZE)
        a = levels.reduced_coefficients(b, reduce, 3, 17, GAZE)
        lifted = levels.reduced_coefficients(f, reduce, 3, 17, GAZE)
        assert np.array_equal(_bits(got), np.where(both[None], _bits(lifted), _bits(a)))
        differs |= not np.array_equal(_bits(got), _bits(a))
    assert differs


@pytest.mark.parametrize("block,mv_block,steps", CASES[:3])
@pytest.mark.parametrize("reduce", [2, 4, 8])
def test_the_low_band_of_both_layers_gives_the_same_coefficients(block, mv_block, steps, reduce):
    _, base, enh, _ = _pair(block, mv_block, steps, True)
    k = block // reduce
    join = lambda frames: (b"".join(bytes(f) for f in frames), np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64))
    bands = [(0, 0, k, k)] * N_FRAMES
    (lb, lbo), (le, leo) = layers.band_frames(*join(base), bands), layers.band_frames(*join(enh), bands)
    assert len(lb) < sum(len(f) for f in base) and len(le) < sum(len(f) for f in enh)  # both layers hold levels outside K x K
    for i, (b, e) in enumerate(zip(base, enh)):
        low_b = np.frombuffer(lb, np.uint8)[int(lbo[i]):int(lbo[i + 1])]
        low_e = np.frombuffer(le, np.uint8)[int(leo[i]):int(leo[i + 1])]
        assert np.array_equal(_bits(layers.reduced_coefficients(low_b, low_e, reduce, 3, 17, GAZE)),
                              _bits(layers.reduced_coefficients(b, e, reduce, 3, 17, GAZE)))


def test_a_foreign_enhancement_is_refused():
    geo, base, enh, _ = _pair(8, 16, (4, 16, 2), False)
    _, types, planes = levels.parse_frame(enh[0])
    d = np.rint(planes.astype(np.float64) / 2).astype(np.int64)
    two_steps = layers.write_frame(geo, types, d, 2, 4)          # fg_step != bg_step
    no_divisor = layers.write_frame(geo, types, d, 3, 3)         # one step, which does not divide 4 and 16
    other = _geometry(16, 16)
    other_geometry = layers.write_frame(other, types, d, 2, 2)
    for foreign in (two_steps, no_divisor, other_geometry):
        with pytest.raises(ValueError):
            layers.reduced_coefficients(base[0], foreign, 2, 1, 640, GAZE)
        with pytest.raises(ValueError):
            layers.decode_layers_reduced_frame(base[0], foreign, 2, 1, 640, (0, 0, 0, 0))  # checked whatever the gaze holds
        layers.reduced_coefficients(base[0], foreign, 2, 1, 640)  # without a gaze it is not read
    for reduce in (0, 3, 16):
        with pytest.raises(ValueError):
            layers.reduced_coefficients(base[0], enh[0], reduce, 1, 640, GAZE)
    with pytest.raises(ValueError):
        layers.reduced_coefficients(base[0], enh[0], 2, 0, 640, GAZE)


def _decode(lib, w, h, bw, bh, mbw, mbh, fg=1, bg=640, reduce=2, dw=0, dh=0, n=2, ws=1 << 30):
    return lib.svc_hip_decode_layers_reduced_frames(None, 0, None, None, 0, None, n, w, h, bw, bh, mbw, mbh, fg, bg, reduce, None, None, ws,
                                                    None, None, dw, dh, None, None)


def test_argument_checks_answer_without_a_device():
    """The order of svc_hip_decode_levels_reduced_frames with the workspace of svc_hip_decode_layers_frames."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    q = native.decode_layers_reduced_workspace_bytes
    assert q(2, 64, 64, 8) == native.decode_layers_workspace_bytes(2, 64, 64, 8) == 2 * native.decode_levels_workspace_bytes(2, 64, 64, 8) > 0
    assert q(2, 64, 64, 4) == 0 and q(2, 72, 64, 8) == 0 and q(70000, 64, 64, 8) == 0
    one = native.decode_levels_workspace_bytes(2, 64, 64, 8)
    assert _decode(lib, 64, 64, 4, 4, 16, 16, fg=0, reduce=3, dw=99, dh=99, ws=0) == unsup and "8x8, 16x16" in err()
    assert _decode(lib, 100, 64, 8, 8, 16, 16) == bad and "not divisible" in err()
    assert _decode(lib, 64, 64, 8, 8, 16, 16, fg=0, reduce=3, dw=99, dh=99, ws=0) == bad and "steps must be positive" in err()
    for r in (0, 1, 3, 16):
        assert _decode(lib, 64, 64, 8, 8, 16, 16, reduce=r, dw=99, dh=99, ws=0) == bad and "reduce" in err(), r
    for r in (2, 4, 8):
        assert _decode(lib, 64, 64, 16, 16, 16, 16, reduce=r, dw=64 // r + 1, dh=64 // r, ws=0) == bad and "display" in err()
        assert _decode(lib, 64, 64, 16, 16, 16, 16, reduce=r, dw=64 // r, dh=64 // r, ws=one) == bad and "workspace" in err()
        assert _decode(lib, 64, 64, 16, 16, 16, 16, reduce=r, dw=64 // r, dh=64 // r, ws=2 * native.decode_levels_workspace_bytes(2, 64, 64, 16)) == bad \
            and "null pointer" in err()
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=32, dh=32, n=70000, ws=0) == unsup and "65535" in err()
    assert _decode(lib, 64, 64, 8, 8, 16, 16, ws=one) == bad and "workspace" in err()       # the one-stream size where twice that is asked
    assert _decode(lib, 64, 64, 8, 8, 16, 16, ws=2 * one) == bad and "null pointer" in err()
    # an empty batch passes the same checks and is then accepted
    assert _decode(lib, 64, 64, 8, 8, 16, 16, reduce=1, n=0) == bad
    assert _decode(lib, 64, 64, 8, 8, 16, 16, dw=33, dh=1, n=0) == bad
    assert _decode(lib, 64, 64, 8, 8, 16, 16, n=0, ws=0) == native.SVC_OK
