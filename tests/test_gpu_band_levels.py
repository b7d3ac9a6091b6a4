"""svc_hip_band_levels_frames and svc_hip_union_levels_frames on the device (include/svc_hip.h: a stored SVCQ stream restricted to a
frequency band per output frame, and bands joined back).

Their contract is byte equality with code already in the tree: layers.band_frames / layers.union_frames on any SVCQ stream,
svc_hip_window_levels_frames where no band is given, and for the band (0, 0, K, K) the reduced decoder's own output on the full stream.
Every call here writes into a stream pre-filled with FILL and offsets and status pre-filled with -1; all n + 1 offsets, the bytes up to the
last one and FILL behind it are asserted, as tests/test_gpu_window_levels.py does."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import partitions
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_decode_levels import _rects
from tests.test_gpu_window_levels import _dev, _expect, _windows_of
from tests.test_gpu_window_levels import _call as _window_call
from tests.test_window_levels_host import GEOMS, geom_dict, random_levels, random_stream, random_types

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
BAND_GEOMS = [
    (36, 12, (4, 4), (12, 12)),      # 16 valid bits per word, the masks only 4-byte aligned
    (36, 24, (12, 12), (12, 12)),    # 3 words per tile, the last partly used
    (272, 24, (8, 8), (16, 8)),      # a group of 32 tiles and one of 2
    (64, 48, (16, 16), (16, 16)),
    (48, 32, (16, 8), (16, 8)),      # a tile that is not square
    (128, 64, (64, 64), (64, 64)),   # 64 words per tile: a group is one tile
    (16, 704, (8, 8), (16, 16)),     # 264 groups: more than one pass of the per-frame scan's workgroup
]
DENSITY = {"zero": 0.0, "full": 1.0, "sparse": 0.06}


def _gid(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}"


def _u32(rows, n):
    """(n, 4) u32 values, some past 2^31 -> the i32 tensor the binding takes."""
    return torch.from_numpy(np.asarray(rows, dtype=np.uint32).reshape(n, 4).view(np.int32)).cuda()


def _offsets(offs):
    return torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda() if not isinstance(offs, torch.Tensor) else offs


def _band_call(stream, offs, geom, bands=None, windows=None, src=None, fill=FILL):
    """svc_hip_band_levels_frames on a stream tensor of exactly its bytes -> (output u8 on the host, offsets, status), each whole."""
    w, h, tile, mv = geom
    frames, offsets = _dev(stream), _offsets(offs)
    n_out = offsets.numel() - 1 if src is None else len(src)
    out = torch.full((max(nat.levels_max_bytes(n_out, w, h, tile, mv), 16),), fill, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
    nat.band_levels_frames(frames, offsets, w, h, tile, mv, band=None if bands is None else _u32(bands, n_out),
                           window=None if windows is None else _u32(windows, n_out), src=src, out=out, out_offsets=out_offs, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _union_call(a, a_offs, b, b_offs, geom, fill=FILL):
    w, h, tile, mv = geom
    ao = _offsets(a_offs)
    n = ao.numel() - 1
    out = torch.full((max(nat.levels_max_bytes(n, w, h, tile, mv), 16),), fill, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    nat.union_levels_frames(_dev(a), ao, _dev(b), _offsets(b_offs), w, h, tile, mv, out=out, out_offsets=out_offs, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _used(got):
    """The stream a call wrote, as exactly its bytes, and its offsets."""
    out, offs, _ = got
    return out[:offs[-1]].copy(), offs


def _band_sets(tile):
    """Lists of four bands, one per frame of a batch: None (NULL), the whole tile said with 0xFFFFFFFF, nothing (hi = 0, lo = hi, lo >
    hi), DC only and all but DC, K = N / 2, N / 4, N / 8 and their remainders, and an odd K = 3 whose cut falls inside mask words and
    rows."""
    bw, bh = tile
    n = max(bw, bh)
    k2, k4, k8 = max(1, n // 2), max(1, n // 4), max(1, n // 8)
    return [None,
            [(0, 0, ALL, ALL)] * 4,
            [(0, 0, 0, 0), (0, 0, bw, 0), (3, 3, 3, 3), (5, 5, 2, 2)],
            [(0, 0, 1, 1), (1, 1, bw, bh), (0, 0, k2, k2), (0, 0, k4, k4)],
            [(0, 0, k8, k8), (0, 0, 3, 3), (3, 3, bw, bh), (k2, k2, ALL, ALL)],
            [(k4, k4, k2, k2), (k8, k8, k4, k4), (0, 0, bw, 1), (1, 0, 2, bh)]]


def _host_bands(bands):
    return None if bands is None else [tuple(int(v) for v in b) for b in bands]


# ---- 1. against layers.band_frames on host-built frames ----------------------------------------------------------------------------------

@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_host_built_frames(native, geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    stream, offs = random_stream(rng, geom, 4, DENSITY[density])  # (sparse: odd level counts, so the groups' runs share dwords)
    sets = _band_sets(tile)
    cases = [(b, None) for b in sets] + [(sets[(i + 2) % len(sets)], win) for i, win in enumerate(_windows_of(geom))]
    odd_runs = 0
    for bands, windows in cases:
        want, want_offs = layers.band_frames(stream, offs, _host_bands(bands), windows)
        got = _band_call(stream, offs, geom, bands, windows)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 4
        odd_runs += sum(int(np.frombuffer(want, np.uint8)[int(o) + 40:int(o) + 44].view("<u4")[0]) % 2 for o in want_offs[:-1])
    if density == "sparse":
        assert odd_runs >= 8  # frames with an odd number of kept levels: a last level alone in its dword


@pytest.mark.parametrize("geom", [BAND_GEOMS[0], BAND_GEOMS[2], BAND_GEOMS[4]], ids=_gid)
def test_source_indices(native, geom):
    """Repeats, any order, n_out = 4 x n_in: one call for four viewers at four sizes, each with its window."""
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(3), geom, 4, 0.3)
    n = max(tile)
    src = [3, 0, 0, 2, 1, 3, 2, 2, 0, 1, 2, 3, 3, 2, 1, 0]
    bands = [[(0, 0, max(1, n // 8), max(1, n // 8)), (0, 0, max(1, n // 4), max(1, n // 4)), (0, 0, n // 2, n // 2), (0, 0, ALL, ALL)][i // 4]
             for i in range(16)]
    windows = [[(0, 0, w, h), (tile[0], 0, w // 2, h), (0, 0, ALL, ALL), (w - 2 * tile[0], 0, w, tile[1])][i % 4] for i in range(16)]
    got = _band_call(stream, offs, geom, bands, windows, src)
    _expect(got, *layers.band_frames(stream, offs, bands, windows, src))
    assert got[2] == [0] * 16
    got = _band_call(stream, offs, geom, None, None, [1, 1, 0])
    _expect(got, *layers.window_frames(stream, offs, None, [1, 1, 0]))
    # an index past the input: 1, 64 zero bytes, the neighbours as they would be
    out, out_offs, status = _band_call(stream, offs, geom, bands[:3], None, [2, 4, 0])
    want = [layers.band_frame(stream[int(offs[s]):int(offs[s + 1])], bands[i]) for i, s in ((0, 2), (2, 0))]
    assert status == [0, 1, 0] and out[:out_offs[-1]].tobytes() == want[0] + bytes(64) + want[1]
    assert out_offs == [0, len(want[0]), len(want[0]) + 64, len(want[0]) + 64 + len(want[1])] and (out[out_offs[-1]:] == FILL).all()


# ---- 2. no band: the window call's bytes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_without_a_band_it_is_the_window_call(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(w + h), geom, 4, 0.2)
    for windows in (None, _windows_of(geom)[5], _windows_of(geom)[4]):
        want = _window_call(stream, offs, geom, windows)
        got = _band_call(stream, offs, geom, None, windows)
        assert got[1] == want[1] and got[2] == want[2] == [0] * 4 and got[0].tobytes() == want[0].tobytes()
    src = [3, 3, 0, 1, 2, 0]
    want = _window_call(stream, offs, geom, [_windows_of(geom)[5][i % 4] for i in range(6)], src)
    got = _band_call(stream, offs, geom, None, [_windows_of(geom)[5][i % 4] for i in range(6)], src)
    assert got[1] == want[1] and got[2] == want[2] and got[0].tobytes() == want[0].tobytes()


# ---- 3. the union ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_the_bands_of_a_partition_join_back(native, geom, density):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(w * 3 + h + len(density)), geom, 4, DENSITY[density])
    two, four = partitions(tile)
    for bands, orders in ((two, ((0, 1), (1, 0))), (four, ((0, 1, 2, 3), (3, 1, 0, 2)))):
        parts = [_used(_band_call(stream, offs, geom, [b] * 4)) for b in bands]
        for order in orders:
            joined = parts[order[0]]
            for k in order[1:]:
                got = _union_call(*joined, *parts[k], geom)
                assert got[2] == [0] * 4
                joined = _used(got)
            _expect(got, stream, offs)


@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_union_of_disjoint_frames_that_are_not_bands(native, geom):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 5 + h)
    g = geom_dict(*geom)
    fa, fb = [], []
    for f in range(4):
        types = random_types(rng, w, h, mv)
        lv = random_levels(rng, w, h, (0.5, 1.0, 0.07, 0.0)[f])
        mine = rng.random((3, h, w)) < (0.5, 0.5, 0.3, 0.5)[f]
        fa.append(layers.write_frame(g, types, lv * mine, 4, 16, inexact=f))
        fb.append(layers.write_frame(g, types, lv * ~mine, 4, 16, inexact=100 + f))
    a, b = entropy._join(fa), entropy._join(fb)
    want, want_offs = layers.union_frames(*a, *b)
    assert want != layers.union_frames(*b, *a)[0]  # header word 11 is the first stream's
    got = _union_call(*a, *b, geom)
    _expect(got, want, want_offs)
    assert got[2] == [0] * 4
    _expect(_union_call(*b, *a, geom), *layers.union_frames(*b, *a))


# ---- 4. with the reduced decoder and the entropy coder -------------------------------------------------------------------------------------

def _encoded(n, w, h, block, mv, steps, seed):
    """Random content through the fused encoder (svc_hip_dct_pack_levels_frames) -> (stream of exactly its bytes, offsets)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randint(0, 256, (n, h // 4, w // 4, 3), dtype=torch.uint8, device="cuda", generator=g).float()
    noise = torch.randint(-20, 21, (n, h, w, 3), dtype=torch.int16, device="cuda", generator=g).float()
    bgr = (base.repeat_interleave(4, 1).repeat_interleave(4, 2) + noise).clamp(0, 255).to(torch.uint8).contiguous()
    types = torch.randint(0, 3, (n, (w // mv) * (h // mv)), dtype=torch.int32, device="cuda", generator=g)
    out, offs = nat.dct_pack_levels_frames(bgr, block, types, mv, *steps)
    torch.cuda.synchronize()
    return out[:int(offs[-1])].clone(), offs


@pytest.mark.parametrize("block,reduce", [(8, 2), (8, 4), (8, 8), (16, 2), (16, 4), (16, 8)])
@pytest.mark.parametrize("steps", [(1, 1), (1, 640)], ids=str)
def test_the_reduced_decoder_decodes_the_band_as_the_full_stream(native, block, reduce, steps):
    n, w, h, mv = 6, 336, 48, 16  # full groups plus a partial one at both tile sizes
    k = block // reduce
    stream, offs = _encoded(n, w, h, block, mv, steps, seed=block * 10 + reduce + steps[1])
    out, out_offs, status = nat.band_levels_frames(stream, offs, w, h, block, mv, band=[(0, 0, k, k)] * n)
    torch.cuda.synchronize()
    used = int(out_offs[-1])
    assert status.cpu().tolist() == [0] * n and used < stream.numel()  # strictly smaller
    band = out[:used].clone()
    rects = _rects(n, w, h)
    display = (w // reduce - 7, h // reduce - 3)
    a = nat.decode_levels_reduced_frames(stream, offs, w, h, block, mv, *steps, reduce=reduce, gaze=rects, display=display)
    b = nat.decode_levels_reduced_frames(band, out_offs, w, h, block, mv, *steps, reduce=reduce, gaze=rects, display=display)
    torch.cuda.synchronize()
    assert a[2].cpu().tolist() == [0] * n == b[2].cpu().tolist()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert a[0].abs().max().item() > 1
    if steps == (1, 1):  # the band stream through the lossless coder and back: its bytes
        coded, coded_offs, st = nat.entropy_encode_frames(band, out_offs, w, h, block, mv)
        back, back_offs, st2 = nat.entropy_decode_frames(coded[:int(coded_offs[-1])].clone(), coded_offs, w, h, block, mv)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == st2.cpu().tolist() == [0] * n
        assert torch.equal(back_offs, out_offs) and torch.equal(back[:used], band)


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------------------

HOST12 = GEOMS[1]  # 12 x 12 tiles: 144 of a tile's 192 mask bits are coefficients
LEVELS_OFF_12 = 64 + 4 * 6 + 8 * 3 * 6 * 3


def _damaged(stream, offs, f, what):
    """-> (the stream with frame f damaged, the code the unpack gives it)"""
    bad = np.frombuffer(stream, np.uint8).copy()
    o = int(offs[f])
    word = bad[o:o + 64].view("<u4")
    if what == "magic":
        word[0] = 0x12345678
        return bad, 2
    if what == "size":
        word[12] += 16
        return bad, 5
    if what == "levels":
        word[10] -= 1
        return bad, 6
    assert what == "stray"
    bad[o + LEVELS_OFF_12 - 1] |= 0x40  # bit 190 of the frame's last tile: past its 144 coefficients
    return bad, 7


def test_band_statuses(native):
    geom = HOST12
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(4), geom, 3, 0.3)
    bands = [(0, 0, 6, 6), (0, 0, 3, 3), (3, 3, 12, 12)]
    windows = [(0, 0, w, h), (12, 0, 24, 24), (0, 0, w, h)]
    clean, clean_offs, status = _band_call(stream, offs, geom, bands, windows)
    assert status == [0] * 3
    good = clean[clean_offs[1]:clean_offs[2]].tobytes()
    assert good == layers.band_frame(stream[int(offs[1]):int(offs[2])], bands[1], windows[1])
    for first, last in (("magic", "size"), ("levels", "stray"), ("stray", "magic"), ("size", "levels")):
        bad, code0 = _damaged(stream, offs, 0, first)
        bad, code2 = _damaged(bad.tobytes(), offs, 2, last)
        out, out_offs, status = _band_call(bad, offs, geom, bands, windows)  # exactly the stream's bytes: a read past them is outside
        assert status == [code0, 0, code2] and out_offs == [0, 64, 64 + len(good), 128 + len(good)]
        assert out[:out_offs[-1]].tobytes() == bytes(64) + good + bytes(64) and (out[out_offs[-1]:] == FILL).all()
    # a source index past the input between two good frames, and a good frame between two of them
    out, out_offs, status = _band_call(stream, offs, geom, bands, windows, [3, 1, 0xFFFFFFF])
    assert status == [1, 0, 1] and out[:out_offs[-1]].tobytes() == bytes(64) + good + bytes(64) and (out[out_offs[-1]:] == FILL).all()
    # a stream cut short: the last frame runs past stream_bytes
    cut = _dev(stream)[:len(stream) - 16].clone()
    out, out_offs, status = _band_call(cut, _offsets(offs), geom, bands, windows)
    assert status == [0, 0, 1] and out[:out_offs[-1]].tobytes() == clean[:clean_offs[2]].tobytes() + bytes(64)


def test_union_statuses(native):
    geom = HOST12
    w, h, tile, mv = geom
    rng = np.random.default_rng(6)
    g = geom_dict(*geom)
    stream, offs = random_stream(rng, geom, 3, 0.3)
    a, a_offs = _used(_band_call(stream, offs, geom, [(0, 0, 5, 5)] * 3))
    b, b_offs = _used(_band_call(stream, offs, geom, [(5, 5, 12, 12)] * 3))
    good = stream[int(offs[1]):int(offs[2])]

    def expect(got, codes):
        out, out_offs, status = got
        assert status == codes
        want = b"".join(bytes(64) if c else stream[int(offs[i]):int(offs[i + 1])] for i, c in enumerate(codes))
        assert out[:out_offs[-1]].tobytes() == want and (out[out_offs[-1]:] == FILL).all()
        assert out_offs == [0] + list(np.cumsum([64 if c else int(offs[i + 1] - offs[i]) for i, c in enumerate(codes)]))

    expect(_union_call(a, a_offs, b, b_offs, geom), [0, 0, 0])
    assert len(good) > 64
    for what in ("magic", "size", "levels", "stray"):
        bad_b, code = _damaged(b.tobytes(), b_offs, 0, what)
        bad_b, _ = _damaged(bad_b.tobytes(), b_offs, 2, "magic")
        expect(_union_call(a, a_offs, bad_b, b_offs, geom), [0x100 | code, 0, 0x100 | 2])
        bad_a, code_a = _damaged(a.tobytes(), a_offs, 2, what)  # A's own code comes first
        expect(_union_call(bad_a, a_offs, bad_b, b_offs, geom), [0x100 | code, 0, code_a])
    # B's steps, then B's types, differ from A's
    steps = b.copy()
    steps[b_offs[0] + 36:b_offs[0] + 40].view("<u4")[0] += 1  # word 9 of frame 0
    steps[b_offs[2] + 32:b_offs[2] + 36].view("<u4")[0] += 1  # word 8 of frame 2
    expect(_union_call(a, a_offs, steps, b_offs, geom), [0x100 | 11, 0, 0x100 | 11])
    types = b.copy()
    types[b_offs[0] + 64 + 4 * 5] ^= 1  # the last region id of frame 0
    types[b_offs[2] + 64] ^= 2           # the first of frame 2
    expect(_union_call(a, a_offs, types, b_offs, geom), [0x100 | 11, 0, 0x100 | 11])
    # one mask bit set in both: the first coefficient of B's frame 0 that A holds too
    lv = random_levels(rng, w, h, 0.3)
    lv[0, 0, 0], lv[2, h - 1, w - 1] = 7, 9
    types0 = random_types(rng, w, h, mv)
    whole = layers.write_frame(g, types0, lv, 4, 16)
    low, high = layers.band_frame(whole, (0, 0, 5, 5)), layers.band_frame(whole, (5, 5, 12, 12))
    for r, c, plane in ((0, 0, 0), (h - 1, w - 1, 2)):  # the frame's first and its last mask bit
        one = np.zeros((3, h, w), np.int64)
        one[plane, r, c] = 5
        shared = layers.union_frame(high if (r, c) == (0, 0) else low, layers.write_frame(g, types0, one, 4, 16))
        other = low if (r, c) == (0, 0) else high
        x, y = entropy._join([other, other, other]), entropy._join([shared, high if other is low else low, shared])
        out, out_offs, status = _union_call(*x, *y, geom)
        assert status == [12, 0, 12] and out[:out_offs[-1]].tobytes() == bytes(64) + whole + bytes(64)
        assert (out[out_offs[-1]:] == FILL).all()


# ---- 6. two runs ---------------------------------------------------------------------------------------------------------------------------

def test_two_calls_write_the_same_bytes(native):
    geom = BAND_GEOMS[2]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(12), geom, 4, 0.3)
    bands = [(0, 0, 3, 3), (3, 3, 8, 8), (0, 0, 4, 4), (1, 1, 8, 8)]
    windows = _windows_of(geom)[5]
    one = _band_call(stream, offs, geom, bands, windows, fill=FILL)
    two = _band_call(stream, offs, geom, bands, windows, fill=0x00)
    used = one[1][-1]
    assert one[1] == two[1] and one[2] == two[2] == [0] * 4 and one[0][:used].tobytes() == two[0][:used].tobytes()
    assert (one[0][used:] == FILL).all() and (two[0][used:] == 0).all()
    low, high = (_used(_band_call(stream, offs, geom, [b] * 4)) for b in ((0, 0, 3, 3), (3, 3, 8, 8)))
    one = _union_call(*low, *high, geom, fill=FILL)
    two = _union_call(*low, *high, geom, fill=0x5A)
    used = one[1][-1]
    assert one[1] == two[1] and one[2] == two[2] == [0] * 4 and one[0][:used].tobytes() == two[0][:used].tobytes()
    assert (one[0][used:] == FILL).all() and (two[0][used:] == 0x5A).all()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[4]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    with pytest.raises(nat.SvcError, match="not divisible"):
        nat.band_levels_frames(frames, offsets, w + 1, h, tile, mv, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                               workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.band_levels_frames(frames, offsets, w, h, tile, mv, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="worst case"):
        nat.union_levels_frames(frames, offsets, frames, offsets, w, h, tile, mv,
                                out=torch.empty(nat.levels_max_bytes(1, w, h, tile, mv), dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        nat.union_levels_frames(frames, offsets, frames, offsets, w, h, tile, mv,
                                out=torch.empty(nat.levels_max_bytes(2, w, h, tile, mv) + 16, dtype=torch.uint8, device="cuda")[4:])
