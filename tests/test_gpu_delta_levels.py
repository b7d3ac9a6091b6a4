"""svc_hip_delta_levels_frames and svc_hip_undelta_levels_frames on the device (include/svc_hip.h: an SVCQ stream coded frame against
frame in levels, and back).

Their contract is byte equality with code already in the tree: layers.delta_frames / layers.undelta_frames on any SVCQ stream, and the
stream itself after both.  Every call here writes into a stream pre-filled with FILL and offsets and status pre-filled with -1; all n + 1
offsets, the bytes up to the last one and FILL behind it are asserted, as tests/test_gpu_window_levels.py does."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_delta_levels_host import BAND_GEOMS, KEYS, _gid, delta_clip, tile_counts
from tests.test_gpu_band_levels import HOST12, _band_call, _damaged, _offsets, _used
from tests.test_gpu_band_levels import BAND_GEOMS as THE_BAND_GEOMS
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_window_levels import _call as _window_call
from tests.test_gpu_window_levels import _dev, _expect
from tests.test_window_levels_host import geom_dict, random_types

pytestmark = pytest.mark.gpu

DENSITY = {"zero": 0.0, "full": 1.0, "sparse": 0.06}
assert BAND_GEOMS == THE_BAND_GEOMS


def _call(undo, stream, offs, geom, keys=None, prev=None, fill=FILL):
    """One of the two calls on a stream tensor of exactly its bytes (and a frame before it of exactly its) -> (output u8 on the host,
    offsets, status), each whole."""
    w, h, tile, mv = geom
    frames, offsets = _dev(stream), _offsets(offs)
    n = offsets.numel() - 1
    out = torch.full((max(nat.levels_max_bytes(n, w, h, tile, mv), 16),), fill, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    fn = nat.undelta_levels_frames if undo else nat.delta_levels_frames
    fn(frames, offsets, w, h, tile, mv, prev=None if prev is None else _dev(prev), key=keys, out=out, out_offsets=out_offs, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _delta(*args, **kw):
    return _call(False, *args, **kw)


def _undelta(*args, **kw):
    return _call(True, *args, **kw)


def _level_counts(stream, offs):
    return [int(np.frombuffer(stream, np.uint8)[int(o) + 40:int(o) + 44].view("<u4")[0]) for o in offs[:-1]]


# ---- 1. against the numpy statements, and back -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("geom", BAND_GEOMS, ids=_gid)
def test_both_calls_against_the_numpy_statement(native, geom, density):
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(w * 7 + h + len(density)), geom, 6, DENSITY[density])
    odd = [0, 0]
    for keys in (KEYS, None):
        want, want_offs = layers.delta_frames(stream, offs, keys)
        got = _delta(stream, offs, geom, keys)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 6
        back = _undelta(*_used(got), geom, keys)  # the round trip on the device
        _expect(back, stream, offs)
        assert back[2] == [0] * 6
        _expect(back, *layers.undelta_frames(want, want_offs, keys))
        odd[0] += sum(c % 2 for c in _level_counts(want, want_offs))
        odd[1] += sum(c % 2 for c in _level_counts(stream, offs))
    if density == "sparse":
        assert odd[0] and odd[1]  # frames with an odd number of levels, written by either call: a last level alone in its dword
    if density == "full":
        predicted, unpredicted, wraps = tile_counts(stream, offs, KEYS)
        assert predicted and unpredicted and wraps


def test_one_frame(native):
    geom = BAND_GEOMS[2]
    stream, offs = delta_clip(np.random.default_rng(1), geom, 2, 0.3)
    f = frames_of(stream, offs)
    one = entropy._join([f[1]])
    for keys in (None, [0], [1]):
        _expect(_delta(*one, geom, keys), *one)  # a frame without a predecessor is a key frame
        _expect(_undelta(*one, geom, keys), *one)
    d = layers.delta_frame(f[1], f[0])
    _expect(_delta(*one, geom, None, prev=f[0]), d, [0, len(d)])
    _expect(_delta(*one, geom, [1], prev=f[0]), *one)
    _expect(_undelta(d, [0, len(d)], geom, [0], prev=f[0]), *one)


def test_a_chain_longer_than_any_batch(native):
    geom = BAND_GEOMS[0]
    stream, offs = delta_clip(np.random.default_rng(33), geom, 33, 0.5)
    keys = [int(i in (0, 16, 17)) for i in range(33)]
    for k in (None, keys):
        want, want_offs = layers.delta_frames(stream, offs, k)
        got = _delta(stream, offs, geom, k)
        _expect(got, want, want_offs)
        back = _undelta(want, want_offs, geom, k)
        _expect(back, stream, offs)
        assert got[2] == back[2] == [0] * 33


@pytest.mark.parametrize("geom", [BAND_GEOMS[1], BAND_GEOMS[2]], ids=_gid)
def test_a_call_cut_in_two_with_the_frame_before(native, geom):
    """At every cut point: the second call's d_prev is the first's last input frame (delta) or last output frame (undelta)."""
    stream, offs = delta_clip(np.random.default_rng(21), geom, 6, 0.3)
    f = frames_of(stream, offs)
    diff, diff_offs = layers.delta_frames(stream, offs, KEYS)
    d = frames_of(diff, diff_offs)
    for cut in range(1, 6):
        first, second = _delta(*entropy._join(f[:cut]), geom, KEYS[:cut]), _delta(*entropy._join(f[cut:]), geom, KEYS[cut:], prev=f[cut - 1])
        assert first[0][:first[1][-1]].tobytes() + second[0][:second[1][-1]].tobytes() == diff, cut
        _expect(second, *entropy._join(d[cut:]))
        first = _undelta(*entropy._join(d[:cut]), geom, KEYS[:cut])
        last = first[0][first[1][-2]:first[1][-1]].tobytes()
        assert last == f[cut - 1]
        second = _undelta(*entropy._join(d[cut:]), geom, KEYS[cut:], prev=last)
        _expect(second, *entropy._join(f[cut:]))
        assert first[2] + second[2] == [0] * 6


def test_a_difference_of_minus_32768(native):
    geom = BAND_GEOMS[3]
    w, h, tile, mv = geom
    g, types = geom_dict(*geom), random_types(np.random.default_rng(3), w, h, mv)
    a, b = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    a[0, 0, 0], b[0, 0, 0] = 16384, -16384      # -32768, no wrap
    a[1, 5, 17], b[1, 5, 17] = -32768, 0        # +32768 wraps to -32768
    a[2, h - 1, w - 1], b[2, h - 1, w - 1] = 32767, -1  # -32768
    a[0, 3, 3], b[0, 3, 3] = 7, 7               # 0: the bit is cleared
    stream, offs = entropy._join([layers.write_frame(g, types, a, 4, 16), layers.write_frame(g, types, b, 4, 16)])
    want, want_offs = layers.delta_frames(stream, offs)
    d = layers._sections(frames_of(want, want_offs)[1])[4]
    assert d.tolist() == [-32768] * 3
    _expect(_delta(stream, offs, geom), want, want_offs)
    _expect(_undelta(want, want_offs, geom), stream, offs)


# ---- 2. with the encoder, the entropy coder, the window call and the band call --------------------------------------------------------------

def test_an_encoded_clip_through_the_entropy_coder_and_back(native):
    n, w, h, block, mv = 6, 64, 48, 8, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    still = torch.randint(0, 256, (1, h // 4, w // 4, 3), dtype=torch.uint8, device="cuda", generator=g).float()
    noise = torch.randint(-3, 4, (n, h, w, 3), dtype=torch.int16, device="cuda", generator=g).float()
    bgr = (still.repeat_interleave(4, 1).repeat_interleave(4, 2) + noise).clamp(0, 255).to(torch.uint8).contiguous()
    types = torch.randint(0, 3, (n, (w // mv) * (h // mv)), dtype=torch.int32, device="cuda", generator=g)
    out, offs = nat.dct_pack_levels_frames(bgr, block, types, mv, 2, 8)
    torch.cuda.synchronize()
    used = int(offs[-1])
    stream = out[:used].clone()
    keys = [1, 0, 0, 1, 0, 0]
    diff, diff_offs, st = nat.delta_levels_frames(stream, offs, w, h, block, mv, key=keys)
    diff = diff[:int(diff_offs[-1])].clone()
    assert st.cpu().tolist() == [0] * n
    host = stream.cpu().numpy().tobytes()
    assert diff.cpu().numpy().tobytes() == layers.delta_frames(host, offs.cpu().numpy(), keys)[0]
    back, back_offs, st = nat.undelta_levels_frames(diff, diff_offs, w, h, block, mv, key=keys)
    assert st.cpu().tolist() == [0] * n and torch.equal(back_offs, offs) and torch.equal(back[:used], stream)
    coded, coded_offs, st = nat.entropy_encode_frames(diff, diff_offs, w, h, block, mv)
    assert st.cpu().tolist() == [0] * n
    plain, plain_offs, st = nat.entropy_decode_frames(coded[:int(coded_offs[-1])].clone(), coded_offs, w, h, block, mv)
    assert st.cpu().tolist() == [0] * n and torch.equal(plain_offs, diff_offs)
    back, back_offs, st = nat.undelta_levels_frames(plain[:int(plain_offs[-1])].clone(), plain_offs, w, h, block, mv, key=keys)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n and torch.equal(back_offs, offs) and torch.equal(back[:used], stream)


def test_window_and_band_commute_with_delta_on_the_device(native):
    geom = BAND_GEOMS[2]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(17), geom, 4, 0.3)
    keys = [1, 0, 0, 0]
    window, band = [(tile[0] * 3, 0, w // 2, h)] * 4, [(1, 1, 5, 4)] * 4
    diff = _used(_delta(stream, offs, geom, keys))
    a = _window_call(*diff, geom, window)
    b = _delta(*_used(_window_call(stream, offs, geom, window)), geom, keys)
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes() and a[2] == b[2] == [0] * 4
    a = _band_call(*diff, geom, band, window)
    b = _delta(*_used(_band_call(stream, offs, geom, band, window)), geom, keys)
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes() and a[2] == b[2] == [0] * 4
    assert a[1][-1] < diff[1][-1]


# ---- 3. statuses ---------------------------------------------------------------------------------------------------------------------------

def _expect_frames(got, frames, codes):
    """status == codes; a frame with a code is 64 zero bytes, every other one frames[i]."""
    out, out_offs, status = got
    assert status == codes
    want = [bytes(64) if c else frames[i] for i, c in enumerate(codes)]
    assert out[:out_offs[-1]].tobytes() == b"".join(want) and (out[out_offs[-1]:] == FILL).all()
    assert out_offs == [0] + [int(v) for v in np.cumsum([len(x) for x in want])]


def test_statuses(native):
    geom = HOST12
    stream, offs = delta_clip(np.random.default_rng(6), geom, 6, 0.3)
    f = frames_of(stream, offs)
    # delta: the failure reaches one frame -- frame 3's predecessor is the damaged input frame, frame 5's the good frame 4
    keys = [1, 0, 0, 0, 1, 0]
    want, want_offs = layers.delta_frames(stream, offs, keys)
    d = frames_of(want, want_offs)
    bad, code = _damaged(stream, offs, 2, "magic")
    assert code == 2
    _expect_frames(_delta(bad, offs, geom, keys), d, [0, 0, 2, 0x102, 0, 0])
    _expect_frames(_delta(bad, offs, geom, None), frames_of(*layers.delta_frames(stream, offs)), [0, 0, 2, 0x102, 0, 0])
    _expect_frames(_delta(bad, offs, geom, [0, 0, 0, 1, 0, 0]), frames_of(*layers.delta_frames(stream, offs, [0, 0, 0, 1, 0, 0])), [0, 0, 2, 0, 0, 0])
    for what in ("size", "levels", "stray"):  # a frame's own code comes first
        worse, own = _damaged(bad.tobytes(), offs, 3, what)
        _expect_frames(_delta(worse, offs, geom, keys), d, [0, 0, 2, own, 0, 0])
        worse, own = _damaged(stream, offs, 5, what)
        _expect_frames(_delta(worse, offs, geom, keys), d, [0, 0, 0, 0, 0, own])
    # undelta: it runs down the chain to the next key frame
    keys = [1, 0, 0, 0, 0, 1]
    want, want_offs = layers.delta_frames(stream, offs, keys)
    bad, _ = _damaged(want, want_offs, 2, "magic")
    _expect_frames(_undelta(bad, want_offs, geom, keys), f, [0, 0, 2, 0x102, 0x102, 0])
    worse, own = _damaged(bad.tobytes(), want_offs, 4, "levels")
    _expect_frames(_undelta(worse, want_offs, geom, keys), f, [0, 0, 2, 0x102, own, 0])
    want, want_offs = layers.delta_frames(stream, offs)
    bad, _ = _damaged(want, want_offs, 1, "size")
    _expect_frames(_undelta(bad, want_offs, geom), f, [0, 5, 0x105, 0x105, 0x105, 0x105])
    # a stream cut short: the last frame runs past stream_bytes
    cut = _dev(want)[:len(want) - 16].clone()
    _expect_frames(_undelta(cut, _offsets(want_offs), geom), f, [0, 0, 0, 0, 0, 1])


def test_a_damaged_frame_before(native):
    geom = HOST12
    stream, offs = delta_clip(np.random.default_rng(8), geom, 4, 0.3)
    f = frames_of(stream, offs)
    rest = entropy._join(f[1:])
    d = frames_of(*layers.delta_frames(*rest, prev=f[0]))
    _expect_frames(_delta(*rest, geom, prev=f[0]), d, [0, 0, 0])
    for what in ("magic", "size", "levels", "stray"):
        bad, code = _damaged(f[0], [0, len(f[0])], 0, what)
        _expect_frames(_delta(*rest, geom, prev=bad), d, [0x100 | code, 0, 0])
        _expect_frames(_delta(*rest, geom, [1, 0, 0], prev=bad), frames_of(*layers.delta_frames(*rest, [1, 0, 0])), [0, 0, 0])  # not read
        _expect_frames(_undelta(*entropy._join(d), geom, [0, 0, 1], prev=bad), f[1:], [0x100 | code] * 2 + [0])
    # the frame before is checked as a frame occupying [0, prev_bytes): less than its bytes is a size that does not match (5), less than a
    # header is out of range (1)
    _expect_frames(_delta(*rest, geom, prev=f[0][:-16]), d, [0x105, 0, 0])
    _expect_frames(_undelta(*entropy._join(d), geom, prev=f[0][:-16]), f[1:], [0x105] * 3)
    _expect_frames(_delta(*rest, geom, prev=f[0][:48]), d, [0x101, 0, 0])
    _expect_frames(_undelta(*entropy._join(d), geom, prev=f[0][:48]), f[1:], [0x101] * 3)
    _expect_frames(_undelta(*entropy._join(d), geom, prev=f[0]), f[1:], [0, 0, 0])


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", [nat.delta_levels_frames, nat.undelta_levels_frames], ids=["delta", "undelta"])
def test_refusals_reach_python(native, fn):
    geom = BAND_GEOMS[3]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    with pytest.raises(nat.SvcError, match="not divisible"):
        fn(frames, offsets, w + 1, h, tile, mv, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
           workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="workspace"):
        fn(frames, offsets, w, h, tile, mv, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="worst case"):
        fn(frames, offsets, w, h, tile, mv, out=torch.empty(nat.levels_max_bytes(1, w, h, tile, mv), dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        fn(frames, offsets, w, h, tile, mv, prev=torch.zeros(80, dtype=torch.uint8, device="cuda")[8:])
    # no frames: nothing is written, whatever the sizes
    out = torch.full((16,), FILL, dtype=torch.uint8, device="cuda")
    none = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    fn(frames[:0], none, w, h, tile, mv, out=out, out_offsets=none, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert (out == FILL).all() and none.tolist() == [-1]
