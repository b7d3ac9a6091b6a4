"""svc_hip_decode_delta_levels_reduced_frames on the device (include/svc_hip.h: a delta stream straight to display frames at 1/2, 1/4, 1/8
size).

Its contract is bit equality with calls already in the tree and pinned by their own tests: svc_hip_undelta_levels_frames with the same frame
before and key flags, then svc_hip_decode_levels_reduced_frames on its output with the same steps, reduce, gaze and display size -- rec,
display and the undelta call's status; `last` is svc_hip_band_levels_frames at (0, 0, K, K) of the undelta call's last output frame, which is
also layers.band_frame of it.  Every output is pre-filled: rec with REC_FILL, display and last with FILL, status and last_bytes with -1;
behind last_bytes the fill is asserted.  Clips, key flags and gaze rectangles are tests/test_gpu_decode_delta.py's, on its three geometries:
a partial last group, a single column of groups, both tile sizes -- with all three reduces of each tile size."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_band_levels_host import frames_of
from tests.test_decode_delta_host import DECODE_GEOMS
from tests.test_delta_levels_host import KEYS, STEPS, delta_clip, tile_counts, with_a_zero_level
from tests.test_gpu_band_levels import _band_call, _damaged, _offsets
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_decode_delta import _gaze
from tests.test_gpu_window_levels import _dev

pytestmark = pytest.mark.gpu

GEOMS = DECODE_GEOMS
REDUCES = (2, 4, 8)
CASES = [(g, r) for g in GEOMS for r in REDUCES]
DENSITY = {"zero": 0.0, "sparse": 0.06, "full": 1.0}
OTHER_DEC = (3, 17)  # decoder steps that are not the encoder's
REC_FILL = -7.25
REC_FILL_BITS = int(np.float32(REC_FILL).view(np.int32))


def _cid(c):
    g, r = c
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}-r{r}"


def _band(geom, r):
    k = geom[2][0] // r
    return (0, 0, k, k)


def _displays(geom, r):
    w, h = geom[0] // r, geom[1] // r
    return [(w, h), (max(1, w - 5), max(1, h - 3))]


def _bits(rec):
    return rec.contiguous().view(torch.int32).cpu()


def _band_of(frame, geom, r):
    """svc_hip_band_levels_frames at (0, 0, K, K) of one frame, as bytes; 64 zero bytes for a frame that fails."""
    out, offs, _ = _band_call(frame, [0, len(frame)], geom, bands=[_band(geom, r)])
    return out[:offs[1]].tobytes()


def _served(diff, offs, geom, r):
    """What a server sends a 1 / r viewer: the band (0, 0, K, K) of the stored delta stream, one band for all frames, no window."""
    n = len(offs) - 1
    out, o, _ = _band_call(diff, offs, geom, bands=[_band(geom, r)] * n)
    return out[:o[-1]].tobytes(), o


def _undelta(diff, offs, geom, keys=None, prev=None):
    """-> (stream on the device, its offsets on the device, the offsets as a list, the statuses)"""
    w, h, tile, mv = geom
    back, back_offs, st = nat.undelta_levels_frames(_dev(diff), _offsets(offs), w, h, tile, mv, prev=None if prev is None else _dev(prev), key=keys)
    o = back_offs.cpu().tolist()
    return back[:o[-1]].clone(), back_offs, o, st.cpu().tolist()


def _two_calls(diff, offs, geom, r, keys=None, prev=None, steps=(1, 640), gaze=None, display=None):
    """The reference: undelta, then the reduced decode -> (rec bits, display, the undelta's status, the band of its last output frame)."""
    w, h, tile, mv = geom
    stream, back_offs, o, st = _undelta(diff, offs, geom, keys, prev)
    rec, disp, _ = nat.decode_levels_reduced_frames(stream, back_offs, w, h, tile, mv, *steps, r, gaze=gaze, display=display)
    torch.cuda.synchronize()
    return _bits(rec), None if disp is None else disp.cpu(), st, _band_of(stream[o[-2]:o[-1]].cpu().numpy().tobytes(), geom, r)


def _fused(diff, offs, geom, r, keys=None, prev=None, steps=(1, 640), gaze=None, display=None, want_last=True):
    """The call under test into pre-filled outputs -> (rec bits, display, status, last); the fill behind last_bytes is asserted."""
    w, h, tile, mv = geom
    offsets = _offsets(offs)
    n = offsets.numel() - 1
    rec = torch.full((n, h // r, w // r, 3), REC_FILL, dtype=torch.float32, device="cuda")
    disp = None if display is None else torch.full((n, display[1], display[0], 3), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    last = torch.full((nat.levels_max_bytes(1, w, h, tile, mv),), FILL, dtype=torch.uint8, device="cuda") if want_last else None
    got = nat.decode_delta_levels_reduced_frames(_dev(diff), offsets, w, h, tile, mv, *steps, r, prev=None if prev is None else _dev(prev),
                                                 key=keys, gaze=gaze, display=display, rec=rec, out_display=disp, last=last, status=status)
    torch.cuda.synchronize()
    assert got[0] is rec and got[1] is disp and got[2] is status and got[3] is last
    frame = None
    if want_last:
        used = int(got[4].item())
        assert 64 <= used <= last.numel() and used % 16 == 0
        host = last.cpu().numpy()
        assert (host[used:] == FILL).all()  # nothing is written behind the frame
        frame = host[:used].tobytes()
    else:
        assert got[4] is None
    return _bits(rec), None if disp is None else disp.cpu(), status.cpu().tolist(), frame


def _same(got, want, what=""):
    assert got[2] == want[2], what                    # status
    assert torch.equal(got[0], want[0]), what         # rec, bit for bit
    assert (got[1] is None) == (want[1] is None) and (got[1] is None or torch.equal(got[1], want[1])), what
    assert got[3] is None or got[3] == want[3], what  # the chain's frame


@functools.lru_cache(maxsize=None)
def _clip(geom, density, n=6):
    w, h = geom[:2]
    return delta_clip(np.random.default_rng(w * 7 + h + len(density)), geom, n, DENSITY[density])


@functools.lru_cache(maxsize=None)
def _delta(geom, density, keyed):
    """The clip's delta stream by the numpy statement, computed once -> (bytes, offsets)."""
    return layers.delta_frames(*_clip(geom, density), KEYS if keyed else None)


# ---- 1. against the two calls ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_against_undelta_then_reduced_decode(native, case, density):
    geom, r = case
    stream, offs = _clip(geom, density)
    frames = frames_of(stream, offs)
    gaze = _gaze(6, geom)
    for keys in (KEYS, None):
        diff, diff_offs = _delta(geom, density, keys is not None)
        for steps, display in zip((STEPS, OTHER_DEC), _displays(geom, r)):
            kw = dict(keys=keys, steps=steps, gaze=gaze, display=display)
            want = _two_calls(diff, diff_offs, geom, r, **kw)
            got = _fused(diff, diff_offs, geom, r, **kw)
            _same(got, want, (keys, steps, display))
            assert got[2] == [0] * 6
            assert got[3] == layers.band_frame(frames[5], _band(geom, r))  # the band of layers.undelta_frames' last frame: the stream's own
            assert not (got[0] == REC_FILL_BITS).any()  # every pixel is written
        # no gaze, no display and no d_last
        _same(_fused(diff, diff_offs, geom, r, keys=keys, want_last=False), _two_calls(diff, diff_offs, geom, r, keys=keys))
    if density == "full":
        predicted, unpredicted, wraps = tile_counts(stream, offs, KEYS)
        assert predicted and unpredicted and wraps
    if density != "zero":
        assert _two_calls(*_delta(geom, density, True), geom, r, keys=KEYS, steps=STEPS)[0].any()  # pictures, not zeros


# ---- 2. the served stream ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_on_the_band_of_the_delta_stream(native, case):
    """A server stores the delta stream and sends the band (0, 0, K, K) of it: every output has the bits it has on the full stream."""
    geom, r = case
    gaze, display = _gaze(6, geom), _displays(geom, r)[1]
    for density in ("sparse", "full"):
        for keys in (KEYS, None):
            diff, diff_offs = _delta(geom, density, keys is not None)
            band, band_offs = _served(diff, diff_offs, geom, r)
            assert len(band) < len(diff)
            kw = dict(keys=keys, steps=OTHER_DEC, gaze=gaze, display=display)
            full = _fused(diff, diff_offs, geom, r, **kw)
            got = _fused(band, band_offs, geom, r, **kw)
            _same(got, full, (density, keys))
            assert got[3] == full[3] and got[2] == [0] * 6
    # a frame damaged on its way fails alike in both
    diff, diff_offs = _delta(geom, "sparse", False)
    band, band_offs = _served(diff, diff_offs, geom, r)
    bad, code = _damaged(band, band_offs, 3, "levels")
    got = _fused(bad, band_offs, geom, r, steps=STEPS, display=display)
    assert got[2] == [0, 0, 0, code, 0x100 | code, 0x100 | code]
    full = _fused(_damaged(diff, diff_offs, 3, "levels")[0], diff_offs, geom, r, steps=STEPS, display=display)
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]) and got[3] == full[3] == bytes(64)


# ---- 3. chaining ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", REDUCES)
def test_a_chain_longer_than_any_batch(native, r):
    geom = GEOMS[0]
    stream, offs = delta_clip(np.random.default_rng(33), geom, 33, 0.5)
    keys = [int(i in (0, 16, 17)) for i in range(33)]
    for k in (None, keys):
        diff, diff_offs = layers.delta_frames(stream, offs, k)
        kw = dict(keys=k, steps=OTHER_DEC, gaze=_gaze(33, geom), display=_displays(geom, r)[1])
        got = _fused(diff, diff_offs, geom, r, **kw)
        _same(got, _two_calls(diff, diff_offs, geom, r, **kw))
        assert got[2] == [0] * 33 and got[3] == layers.band_frame(frames_of(stream, offs)[32], _band(geom, r))


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_a_call_cut_in_two_at_every_frame(native, case):
    """The second call's `prev` is the first's `last` (the band), or the full-size reconstructed frame from the undelta call, or from the
    full-size fused call's `last`: all three concatenations are the single call."""
    geom, r = case
    w, h, tile, mv = geom
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    diff, diff_offs = _delta(geom, "sparse", True)
    d = frames_of(diff, diff_offs)
    gaze, display = _gaze(6, geom), _displays(geom, r)[1]
    whole = _fused(diff, diff_offs, geom, r, keys=KEYS, steps=OTHER_DEC, gaze=gaze, display=display)
    assert whole[3] == layers.band_frame(f[5], _band(geom, r))
    for cut in range(1, 6):
        head, tail = entropy._join(d[:cut]), entropy._join(d[cut:])
        a = dict(keys=KEYS[:cut], steps=OTHER_DEC, gaze=gaze[:cut], display=display)
        first = _fused(*head, geom, r, **a)
        _same(first, _two_calls(*head, geom, r, **a), cut)
        assert first[3] == layers.band_frame(f[cut - 1], _band(geom, r)), cut
        # the full-size frame before, by both calls that give one
        und, _, o, _ = _undelta(*head, geom, KEYS[:cut])
        from_undelta = und[o[-2]:o[-1]].cpu().numpy().tobytes()
        got = nat.decode_delta_levels_frames(_dev(head[0]), _offsets(head[1]), w, h, tile, mv, *OTHER_DEC, key=KEYS[:cut], want_last=True)
        from_fused = got[3][:int(got[4].item())].cpu().numpy().tobytes()
        assert from_undelta == from_fused == f[cut - 1], cut
        for prev in (first[3], from_undelta, from_fused):
            b = dict(keys=KEYS[cut:], prev=prev, steps=OTHER_DEC, gaze=gaze[cut:], display=display)
            second = _fused(*tail, geom, r, **b)
            _same(second, _two_calls(*tail, geom, r, **b), cut)
            assert torch.equal(torch.cat([first[0], second[0]]), whole[0]) and torch.equal(torch.cat([first[1], second[1]]), whole[1]), cut
            assert first[2] + second[2] == whole[2] == [0] * 6 and second[3] == whole[3], cut


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=_cid)
def test_one_frame(native, case):
    geom, r = case
    stream, offs = delta_clip(np.random.default_rng(1), geom, 2, 0.3)
    f = frames_of(stream, offs)
    one = entropy._join([f[1]])
    d = layers.delta_frame(f[1], f[0])
    alone = _two_calls(*one, geom, r)
    want_last = layers.band_frame(f[1], _band(geom, r))
    for keys in (None, [0], [1]):  # a frame without a predecessor is a key frame
        _same(_fused(*one, geom, r, keys=keys), alone)
    for prev in (f[0], layers.band_frame(f[0], _band(geom, r))):
        for case_kw in (dict(prev=prev), dict(prev=prev, keys=[0])):
            got = _fused(d, [0, len(d)], geom, r, **case_kw)
            _same(got, _two_calls(d, [0, len(d)], geom, r, **case_kw))
            assert torch.equal(got[0], alone[0]) and got[3] == want_last
        got = _fused(*one, geom, r, prev=prev, keys=[1])  # a key frame does not read the frame before
        _same(got, _two_calls(*one, geom, r, prev=prev, keys=[1]))
        assert torch.equal(got[0], alone[0]) and got[3] == want_last


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_a_chain_that_alternates_with_the_undelta_call_on_the_band_stream(native, case):
    """Per call in turn: this call, then svc_hip_undelta_levels_frames on the served stream with the reduced decode behind it.  Either
    hands the next the band of its last reconstructed frame."""
    geom, r = case
    w, h, tile, mv = geom
    diff, diff_offs = _delta(geom, "sparse", True)
    band, band_offs = _served(diff, diff_offs, geom, r)
    d = frames_of(band, band_offs)
    gaze = _gaze(6, geom)
    whole = _fused(diff, diff_offs, geom, r, keys=KEYS, steps=STEPS, gaze=gaze)
    for first_is_fused in (True, False):
        recs, prev, at, fused_turn = [], None, 0, first_is_fused
        for n in (1, 2, 1, 2):
            part = entropy._join(d[at:at + n])
            kw = dict(keys=KEYS[at:at + n], prev=prev)
            if fused_turn:
                got = _fused(*part, geom, r, steps=STEPS, gaze=gaze[at:at + n], **kw)
                assert got[2] == [0] * n
                recs.append(got[0])
                prev = got[3]
            else:
                stream, offs, o, st = _undelta(*part, geom, **kw)
                assert st == [0] * n
                rec, _, _ = nat.decode_levels_reduced_frames(stream, offs, w, h, tile, mv, *STEPS, r, gaze=gaze[at:at + n])
                recs.append(_bits(rec))
                prev = stream[o[-2]:o[-1]].cpu().numpy().tobytes()
            at, fused_turn = at + n, not fused_turn
        assert torch.equal(torch.cat(recs), whole[0]), first_is_fused
        assert prev == whole[3]  # the band of the last frame, by whichever call came last


# ---- 4. failures ---------------------------------------------------------------------------------------------------------------------------

def _zero_frames(rec_bits):
    return [not bool(r.any()) for r in rec_bits]


@pytest.mark.parametrize("case", CASES[:6], ids=_cid)
def test_a_damaged_frame_in_mid_chain(native, case):
    geom, r = case
    stream, offs = _clip(geom, "sparse")
    keys = [1, 0, 0, 0, 0, 1]
    diff, diff_offs = layers.delta_frames(stream, offs, keys)
    kw = dict(keys=keys, steps=STEPS, gaze=_gaze(6, geom), display=_displays(geom, r)[0])
    intact = _fused(diff, diff_offs, geom, r, **kw)
    last = layers.band_frame(frames_of(stream, offs)[5], _band(geom, r))
    for what in ("magic", "size", "levels"):
        bad, code = _damaged(diff, diff_offs, 2, what)
        got = _fused(bad, diff_offs, geom, r, **kw)
        _same(got, _two_calls(bad, diff_offs, geom, r, **kw), what)
        assert got[2] == [0, 0, code, 0x100 | code, 0x100 | code, 0]
        assert _zero_frames(got[0]) == [False, False, True, True, True, False] and not got[1][2:5].any()
        for i in (0, 1, 5):  # the neighbours are intact
            assert torch.equal(got[0][i], intact[0][i]) and torch.equal(got[1][i], intact[1][i])
        assert got[3] == last
    # a frame's own code comes first; a last frame that failed is 64 zero bytes
    worse, own = _damaged(_damaged(diff, diff_offs, 2, "magic")[0].tobytes(), diff_offs, 5, "levels")
    got = _fused(worse, diff_offs, geom, r, **kw)
    _same(got, _two_calls(worse, diff_offs, geom, r, **kw))
    assert got[2] == [0, 0, 2, 0x102, 0x102, own] and got[3] == bytes(64)
    no_keys = _delta(geom, "sparse", False)
    bad, _ = _damaged(*no_keys, 1, "size")
    got = _fused(bad, no_keys[1], geom, r, steps=STEPS)
    _same(got, _two_calls(bad, no_keys[1], geom, r, steps=STEPS))
    assert got[2] == [0, 5] + [0x105] * 4 and got[3] == bytes(64)
    cut = _dev(no_keys[0])[:len(no_keys[0]) - 16].clone()  # a stream cut short: the last frame runs past stream_bytes
    got = _fused(cut, no_keys[1], geom, r, steps=STEPS)
    _same(got, _two_calls(cut, no_keys[1], geom, r, steps=STEPS))
    assert got[2] == [0] * 5 + [1] and got[3] == bytes(64)


@pytest.mark.parametrize("r", REDUCES)
def test_a_damaged_frame_before(native, r):
    geom = GEOMS[0]
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    dd = frames_of(*layers.delta_frames(*entropy._join(f[1:]), prev=f[0]))
    d = entropy._join(dd)
    want_last = layers.band_frame(f[5], _band(geom, r))
    for prev in (f[0], layers.band_frame(f[0], _band(geom, r))):
        good = _fused(*d, geom, r, prev=prev, steps=STEPS)
        _same(good, _two_calls(*d, geom, r, prev=prev, steps=STEPS))
        assert good[2] == [0] * 5 and good[3] == want_last
        for what in ("magic", "size", "levels"):
            bad, code = _damaged(prev, [0, len(prev)], 0, what)
            keys = [0, 0, 0, 1, 0]
            got = _fused(*d, geom, r, prev=bad, keys=keys, steps=STEPS)
            _same(got, _two_calls(*d, geom, r, prev=bad, keys=keys, steps=STEPS), what)
            assert got[2] == [0x100 | code] * 3 + [0, 0] and _zero_frames(got[0]) == [True] * 3 + [False] * 2
            # (the stream was coded without key flags: the frame flagged here is taken as it is, a difference, and the last frame hangs on it)
            assert got[3] == layers.band_frame(layers.undelta_frame(dd[4], dd[3]), _band(geom, r))
    got = _fused(*d, geom, r, prev=f[0][:48], steps=STEPS)  # less than a header: out of range
    _same(got, _two_calls(*d, geom, r, prev=f[0][:48], steps=STEPS))
    assert got[2] == [0x101] * 5 and got[3] == bytes(64)


def _with_a_zero_level_at(frame, k, inside):
    """with_a_zero_level for the first level of the frame that lies inside, or outside, the first k x k coefficients of its tile."""
    b, hdr, types, masks, lv = layers._sections(frame)
    bits = np.unpackbits(masks, axis=-1, bitorder="little").astype(bool)
    coeff = np.broadcast_to(np.arange(bits.shape[-1]), bits.shape)[bits]  # the coefficient of every level, in stream order
    bw = hdr["block_w"]
    there = np.flatnonzero(((coeff // bw < k) & (coeff % bw < k)) == inside)
    assert there.size and lv[there[0]] != 0
    bad = np.frombuffer(frame, np.uint8).copy()
    at = 64 + 4 * types.size + masks.size + 2 * int(there[0])
    bad[at:at + 2] = 0
    _, _, _, vals, _ = layers._dense(bad)
    nz = vals != 0
    clean = layers._assemble(bad[:40].view("<u4"), hdr["inexact"], types, np.packbits(nz, axis=-1, bitorder="little"), vals[nz])
    return bad.tobytes(), clean


@pytest.mark.parametrize("case", CASES[:6], ids=_cid)
def test_a_set_bit_of_level_zero(native, case):
    """Inside K x K it gives the pixels of the stream without it, and `last` comes with the bit cleared; outside K x K it is never read."""
    geom, r = case
    band = _band(geom, r)
    stream, offs = delta_clip(np.random.default_rng(5), geom, 3)
    f = frames_of(stream, offs)
    keys = [1, 0, 1]
    d = frames_of(*layers.delta_frames(stream, offs, keys))
    assert d[2] == f[2]
    for zero in (with_a_zero_level, lambda fr: _with_a_zero_level_at(fr, band[2], True), lambda fr: _with_a_zero_level_at(fr, band[2], False)):
        bad, clean = zero(d[2])
        assert bad != clean
        got = _fused(*entropy._join([d[0], d[1], bad]), geom, r, keys=keys, steps=STEPS)
        _same(got, _two_calls(*entropy._join([d[0], d[1], bad]), geom, r, keys=keys, steps=STEPS))
        want = _fused(*entropy._join([d[0], d[1], clean]), geom, r, keys=keys, steps=STEPS)
        assert torch.equal(got[0], want[0]) and got[2] == [0] * 3 and got[3] == want[3] == layers.band_frame(clean, band)
        # the same in a predicted frame: a difference of 0 under a set bit
        bad, clean = zero(d[1])
        got = _fused(*entropy._join([d[0], bad]), geom, r, steps=STEPS)
        want = _fused(*entropy._join([d[0], clean]), geom, r, steps=STEPS)
        _same(got, _two_calls(*entropy._join([d[0], bad]), geom, r, steps=STEPS))
        assert torch.equal(got[0], want[0]) and got[3] == want[3] == layers.band_frame(layers.undelta_frame(clean, f[0]), band)


# ---- 5. the width of the first K x K -------------------------------------------------------------------------------------------------------

def _loud_outside(frame, k, sign):
    """The frame with every level outside the first k x k coefficients of every tile replaced by +-32767 (all of them set)."""
    b, hdr, types, vals, _ = layers._dense(frame)
    bw, bh = hdr["block_w"], hdr["block_h"]
    coeff = np.arange(vals.shape[-1])
    outside = (coeff < bw * bh) & ((coeff // bw >= k) | (coeff % bw >= k))
    vals = vals.copy()
    vals[..., outside] = np.where((coeff[outside] + sign) % 2 == 0, 32767, -32767).astype(np.int16)
    nz = vals != 0
    return layers._assemble(b[:40].view("<u4"), hdr["inexact"], types, np.packbits(nz, axis=-1, bitorder="little"), vals[nz])


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_nothing_outside_the_first_k_by_k_is_read(native, case):
    geom, r = case
    k = _band(geom, r)[2]
    stream, offs = _clip(geom, "sparse")
    f = frames_of(stream, offs)
    d = frames_of(*layers.delta_frames(*entropy._join(f[1:]), KEYS[1:], prev=f[0]))
    kw = dict(keys=KEYS[1:], steps=OTHER_DEC, gaze=_gaze(5, geom), display=_displays(geom, r)[1])
    want = _fused(*entropy._join(d), geom, r, prev=f[0], **kw)
    loud = entropy._join([_loud_outside(fr, k, i) for i, fr in enumerate(d)])
    assert len(loud[0]) > len(b"".join(d))
    got = _fused(*loud, geom, r, prev=_loud_outside(f[0], k, 1), **kw)
    _same(got, want)
    assert got[3] == want[3] == layers.band_frame(f[5], _band(geom, r))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[1]
    w, h, tile, mv = geom
    stream, offs = delta_clip(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), _offsets(offs)
    fn = nat.decode_delta_levels_reduced_frames
    small = torch.empty(16, dtype=torch.uint8, device="cuda")

    def refused(match, status, *args, **kw):
        with pytest.raises(nat.SvcError, match=match) as e:
            fn(*args, **kw)
        assert e.value.status == status

    bad, unsup = nat.SVC_ERR_INVALID_ARG, nat.SVC_ERR_UNSUPPORTED
    refused("not divisible", bad, frames, offsets, w + 1, h, tile, mv, workspace=small)
    refused("8x8, 16x16", unsup, frames, offsets, 48, 32, (16, 8), (16, 8), workspace=small)
    refused("steps", bad, frames, offsets, w, h, tile, mv, 0, 16)
    for r in (1, 3, 16):
        refused("reduce", bad, frames, offsets, w, h, tile, mv, 1, 640, r)
    refused("display", bad, frames, offsets, w, h, tile, mv, 1, 640, 4, display=(w // 4 + 1, h // 4))
    refused("workspace", bad, frames, offsets, w, h, tile, mv, workspace=small)
    refused("last frame", bad, frames, offsets, w, h, tile, mv, last=torch.empty(nat.levels_max_bytes(1, w, h, tile, mv) - 16, dtype=torch.uint8,
                                                                                 device="cuda"))
    refused("aligned", bad, frames, offsets, w, h, tile, mv, prev=torch.zeros(80, dtype=torch.uint8, device="cuda")[8:])
    # no frames: nothing is written, whatever the sizes
    last = torch.full((nat.levels_max_bytes(1, w, h, tile, mv),), FILL, dtype=torch.uint8, device="cuda")
    none = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    got = fn(frames[:0], none, w, h, tile, mv, last=last, workspace=small)
    torch.cuda.synchronize()
    assert (last == FILL).all() and none.tolist() == [-1] and got[0].numel() == 0
