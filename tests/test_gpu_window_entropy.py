"""svc_hip_window_entropy_frames on the device (include/svc_hip.h: a stored SVCE stream restricted to a window per output frame, on its
coded bytes).

Its contract is byte equality with entropy.window_frames, the numpy statement, and -- on a stream this project's encoder wrote -- with
the three calls it replaces (svc_hip_entropy_decode_frames, svc_hip_window_levels_frames, svc_hip_entropy_encode_frames), whose offsets
and statuses are compared on the same input.  Every call here writes into a stream pre-filled with FILL and offsets pre-filled with -1; all
n_out + 1 offsets, the bytes up to the last one and FILL behind it are asserted."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL
from tests.test_gpu_window_levels import ENCODE, HOST_GEOMS, _dev, _encode, _expect, _windows_of
from tests.test_window_entropy_host import DENSITY, chunk_table, empty_chunk, frames_of
from tests.test_window_levels_host import geom_dict, random_levels, random_stream, random_types

pytestmark = pytest.mark.gpu


def _offs_dev(offs):
    return torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda() if not isinstance(offs, torch.Tensor) else offs


def _call(stream, offs, geom, windows=None, src=None):
    """svc_hip_window_entropy_frames on a stream tensor of exactly its bytes -> (output u8 on the host, offsets, status), each whole."""
    w, h, tile, mv = geom
    frames = _dev(stream)
    offsets = _offs_dev(offs)
    n_out = offsets.numel() - 1 if src is None else len(src)
    out = torch.full((max(nat.window_entropy_max_bytes(n_out, w, h, tile, mv), 16),), FILL, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
    win = None  # u32 rectangles, some past 2^31: as the i32 tensor the binding takes
    if windows is not None:
        win = torch.from_numpy(np.asarray(windows, dtype=np.uint32).reshape(n_out, 4).view(np.int32)).cuda()
    nat.window_entropy_frames(frames, offsets, w, h, tile, mv, window=win, src=src, out=out, out_offsets=out_offs, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _three_calls(stream, offs, geom, windows=None, src=None):
    """The route the call replaces, on the device -> (SVCE bytes, offsets, the first non-zero status of the three per output frame)."""
    w, h, tile, mv = geom
    frames, offsets = _dev(stream), _offs_dev(offs)
    q, qo, st_d = nat.entropy_decode_frames(frames, offsets, w, h, tile, mv)
    win = None if windows is None else torch.from_numpy(np.asarray(windows, dtype=np.uint32).reshape(-1, 4).view(np.int32)).cuda()
    wq, wo, st_w = nat.window_levels_frames(q, qo, w, h, tile, mv, window=win, src=src)
    e, eo, st_e = nat.entropy_encode_frames(wq, wo, w, h, tile, mv)
    torch.cuda.synchronize()
    idx = list(range(offsets.numel() - 1)) if src is None else list(src)
    st_d = st_d.cpu().tolist()
    first = [(st_d[s] if s < len(st_d) else 0) or a or b for s, a, b in zip(idx, st_w.cpu().tolist(), st_e.cpu().tolist())]
    eo = eo.cpu().tolist()
    return e[:eo[-1]].cpu().numpy().tobytes(), eo, first


def _phase_changes(stream, offs, windows, want, want_offs, src=None):
    """Kept chunks of at least 4 bytes whose payload lies at another byte phase mod 4 in the output than in the input."""
    n = 0
    ins, outs = frames_of(stream, offs), frames_of(want, want_offs)
    for i, out in enumerate(outs):
        f = ins[i if src is None else src[i]]
        cls = entropy.chunk_classes(f, None if windows is None else windows[i])
        _, start_i, sizes_i, _ = chunk_table(f)
        _, start_o, _, _ = chunk_table(out)
        n += int(((cls == 0) & (sizes_i >= 4) & ((start_i - start_o) % 4 != 0)).sum())
    return n


# ---- 1. host-built frames ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("geom", HOST_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}")
def test_host_built_frames(native, geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    phase, kept = 0, 0
    # ... and whole tile rows dropped ahead of whole rows kept: the kept payloads move by the bytes their dropped neighbours lose
    rows = [(0, tile[1], w, h), (0, tile[1], w, h), (0, min(2 * tile[1], h - tile[1]), w, h), (0, tile[1], w, tile[1])]
    for windows in _windows_of(geom) + [rows]:
        stream, offs = random_stream(rng, geom, 4, DENSITY[density])
        svce, so = entropy.encode_frames(stream, offs)
        want, want_offs = entropy.window_frames(svce, so, windows)
        got = _call(svce, so, geom, windows)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 4
        ref, ref_offs, ref_st = _three_calls(svce, so, geom, windows)
        assert got[1] == ref_offs and got[2] == ref_st and ref == bytes(want)
        phase += _phase_changes(svce, so, windows, want, want_offs)
        kept += sum(int((entropy.chunk_classes(f, None if windows is None else windows[i]) == 0).sum()) for i, f in enumerate(frames_of(svce, so)))
    assert kept > 0
    if density != "zero":  # (all-zero chunks are of the dropped chunks' size: nothing moves)
        assert phase >= 8, phase  # kept payloads were copied between different byte phases, in every geometry


# ---- 2. foreign but legal inputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [HOST_GEOMS[0], HOST_GEOMS[1], HOST_GEOMS[2], HOST_GEOMS[6]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_any_chunk_tiles_and_forced_parameters(native, geom):
    w, h, tile, mv = geom
    tx = w // tile[0]
    rng = np.random.default_rng(w + h)
    stream, offs = random_stream(rng, geom, 4, 0.06)
    lists = _windows_of(geom)
    variants = [dict(chunk_tiles=c) for c in (1, 3, 5, tx, tx + 1)] + [dict(force_k=k) for k in ((0, 0), (7, 7), (3, 5))]
    for n, kw in enumerate(variants):
        svce, so = entropy.encode_frames(stream, offs, **kw)
        for windows in (lists[5], lists[6 + n % 3]):
            want, want_offs = entropy.window_frames(svce, so, windows)
            got = _call(svce, so, geom, windows)
            _expect(got, want, want_offs)
            assert got[2] == [0] * 4
            # kept chunks verbatim, cut chunks canonical: the output decodes to the windowed SVCQ frames
            q, qo = entropy.decode_frames(got[0][:got[1][-1]].tobytes(), got[1])
            wq, wo = layers.window_frames(stream, offs, windows)
            assert q == wq and np.array_equal(qo, wo)


WIDE = (1056, 8, (8, 8), (16, 8))  # 132 tiles in the one tile row: a chunk of more than a wave's 64 lanes of tiles
WIDE_WINDOWS = [(8 * 3, 0, 8 * 70, 8), (8 * 64, 0, 8 * 10, 8), (8 * 65, 0, 8 * 67, 8), (0, 0, 8 * 131, 8)]


@pytest.mark.parametrize("density", [0.06, 1.0])
def test_chunks_of_more_than_64_tiles(native, density):
    """The wave that sizes and places a cut chunk takes its tiles 64 at a time: cuts in the first, second and third trip."""
    w, h, tile, mv = WIDE
    stream, offs = random_stream(np.random.default_rng(12), WIDE, 4, density)
    for ct in (132, 100, 65):
        svce, so = entropy.encode_frames(stream, offs, chunk_tiles=ct)
        want, want_offs = entropy.window_frames(svce, so, WIDE_WINDOWS)
        got = _call(svce, so, WIDE, WIDE_WINDOWS)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 4
        cut = [int((entropy.chunk_classes(f, WIDE_WINDOWS[i]) == 2).sum()) for i, f in enumerate(frames_of(svce, so))]
        assert sum(c > 0 for c in cut) >= 3, cut  # (a window edge on a chunk's edge cuts nothing)
        wq, wo = layers.window_frames(stream, offs, WIDE_WINDOWS)
        canon, canon_offs = entropy.encode_frames(wq, wo, chunk_tiles=ct)
        assert want == canon and np.array_equal(want_offs, canon_offs)


def _zeroed_levels_frame(geom, rng, spots):
    """An SVCQ frame whose levels at spots (plane, y, x) are 0 under set mask bits."""
    w, h, tile, mv = geom
    lv = random_levels(rng, w, h, 0.06)
    lv[lv == 1] = 2
    for p, y, x in spots:
        lv[p, y, x] = 1
    frame = np.frombuffer(layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), lv, 4, 16), np.uint8).copy()
    lo = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * ((tile[0] * tile[1] + 63) // 64)
    lev = frame[lo:lo + 2 * int(frame[40:44].view("<u4")[0])].view("<i2")
    assert int((lev == 1).sum()) == len(spots)
    lev[lev == 1] = 0
    return frame.tobytes()


def test_zero_levels_under_set_bits(native):
    geom = HOST_GEOMS[2]  # 272 x 24 at 8 x 8: per row a chunk of 32 tiles and one of 2
    w, h, tile, mv = geom
    rng = np.random.default_rng(21)
    # tile 5 (kept in the cut chunk), tile 20 (dropped in the cut chunk), tile 33 of the second row (a chunk dropped whole), and a
    # kept-whole chunk's tile in the third row under the fourth frame's window
    spots = [(0, 0, 8 * 5 + 3), (1, 0, 8 * 20 + 3), (0, 8, 8 * 33 + 3), (2, 16, 8 * 2 + 1)]
    frames = [_zeroed_levels_frame(geom, rng, spots) for _ in range(4)]
    stream, offs = entropy._join(frames)
    svce, so = entropy.encode_frames(stream, offs)
    windows = [(0, 0, 8 * 12, h), (8 * 4, 0, 8 * 4, h), (8 * 20, 0, w, h), (0, 16, w, 8)]
    want, want_offs = entropy.window_frames(svce, so, windows)
    got = _call(svce, so, geom, windows)
    _expect(got, want, want_offs)
    ref, ref_offs, ref_st = _three_calls(svce, so, geom, windows)
    assert got[1] == ref_offs and got[2] == ref_st == [0] * 4 and ref == bytes(want)
    g, start, _, _ = chunk_table(frames_of(want, want_offs)[0])
    assert want[start[0]] & 1  # the cut chunk that keeps the zero level is raw


# ---- 3. the DC chain across the cut ---------------------------------------------------------------------------------------------------------

def test_dc_chain_across_the_cut(native):
    geom = HOST_GEOMS[2]
    w, h, tile, mv = geom
    rng = np.random.default_rng(31)
    frames = []
    for f in range(4):
        lv = random_levels(rng, w, h, 0.03)
        for p in range(3):  # tiles 3 | 4 .. 9 | 10 ..: the tile before the window, its first and last tile, then dropped tiles
            lv[p, 0::8, 8 * 3] = 32767
            lv[p, 0::8, 8 * 4] = -32768
            lv[p, 0::8, 8 * 9] = 32767
            lv[p, 0::8, 8 * 10] = -32768 if f % 2 else 0
        frames.append(layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), lv, 4, 16))
    stream, offs = entropy._join(frames)
    svce, so = entropy.encode_frames(stream, offs)
    windows = [(8 * 4, 0, 8 * 6, h)] * 4
    want, want_offs = entropy.window_frames(svce, so, windows)
    got = _call(svce, so, geom, windows)
    _expect(got, want, want_offs)
    ref, ref_offs, ref_st = _three_calls(svce, so, geom, windows)
    assert got[1] == ref_offs and got[2] == ref_st == [0] * 4 and ref == bytes(want)


# ---- 4. against the encoder -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ENCODE, ids=lambda c: "-".join(str(x) for x in c).replace(" ", ""))
def test_windowing_the_stored_svce_enhancement_gives_the_encoders_bytes(native, case):
    block, w, h, mv, steps, kind = case
    _, _, whole, whole_offs, want, want_offs, windows = _encode(*case)
    stored, stored_offs, st = nat.entropy_encode_frames(whole[:int(whole_offs[-1])].clone(), whole_offs, w, h, block, mv)
    ref, ref_offs, st_ref = nat.entropy_encode_frames(want[:int(want_offs[-1])].clone(), want_offs, w, h, block, mv)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st_ref.cpu().tolist() == [0] * 4
    got = _call(stored[:int(stored_offs[-1])], stored_offs, (w, h, (block, block), mv), windows)
    _expect(got, ref[:int(ref_offs[-1])].cpu().numpy().tobytes(), ref_offs.cpu().tolist())
    assert got[2] == [0] * 4


# ---- 5. d_src ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [HOST_GEOMS[0], HOST_GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_source_indices(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(3), geom, 4, 0.1)
    svce, so = entropy.encode_frames(stream, offs)
    src = [3, 0, 0, 2, 7, 1]
    windows = [(tile[0], 0, w, h), (0, 0, w, h), (0, 0, w // 2, h), (0, 0, 0, 0), (0, 0, w, h), (w - 2 * tile[0], 0, w, tile[1])]
    out, out_offs, status = _call(svce, so, geom, windows, src)
    assert status == [0, 0, 0, 0, 1, 0]
    frames = [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(6)]
    ins = frames_of(svce, so)
    for i, s in enumerate(src):
        assert frames[i] == (bytes(64) if i == 4 else entropy.window_frame(ins[s], windows[i])), i
    assert (out[out_offs[-1]:] == FILL).all()
    # several viewers of one stored frame, and every frame twice without a window
    viewers = [(0, 0, w, h), (tile[0], 0, 3 * tile[0], h), (w // 2, 0, w, tile[1]), (0, 0, 0, 0), (w - tile[0], 0, tile[0], h)]
    got = _call(svce, so, geom, viewers, [2] * 5)
    want, want_offs = entropy.window_frames(svce, so, viewers, [2] * 5)
    _expect(got, want, want_offs)
    assert got[2] == [0] * 5
    got = _call(svce, so, geom, None, [0, 0, 1, 1, 2, 2, 3, 3])
    want, want_offs = entropy.window_frames(svce, so, None, [0, 0, 1, 1, 2, 2, 3, 3])
    _expect(got, want, want_offs)


# ---- 6. malformed frames -----------------------------------------------------------------------------------------------------------------

def _spoiled(svce, so, geom, windows, bad, f, clean, clean_offs, code):
    """The call and the entropy decoder's check on a stream whose frame f is spoiled: status `code` for f alone (the decoder's too,
    where `code` is its check's), frame f 64 zero bytes, its neighbours the clean run's."""
    w, h, tile, mv = geom
    frames = _dev(bad)  # exactly the stream's bytes: a read past them is outside the allocation
    out, out_offs, status = _call(frames, so, geom, windows)
    want = [0] * 4
    want[f] = code
    assert status == want, (f, code, status)
    sizes = [clean_offs[i + 1] - clean_offs[i] if i != f else 64 for i in range(4)]
    assert out_offs == [sum(sizes[:i]) for i in range(5)]
    for i in range(4):
        frame = out[out_offs[i]:out_offs[i + 1]].tobytes()
        assert frame == (bytes(64) if i == f else clean[clean_offs[i]:clean_offs[i + 1]].tobytes()), (f, code, i)
    assert (out[out_offs[-1]:] == FILL).all()
    return frames


def test_malformed_frames(native):
    geom = HOST_GEOMS[2]  # 272 x 24 at 8 x 8
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(4), geom, 4, 0.06)
    svce, so = entropy.encode_frames(stream, offs)
    so = [int(o) for o in so]
    windows = [(8 * 4, 0, 8 * 20, h), (0, 0, w, h), (8 * 30, 8, w, 8), (8 * 33, 0, 8, h)]
    clean, clean_offs, status = _call(svce, so, geom, windows)
    assert status == [0] * 4
    base = np.frombuffer(svce, np.uint8)

    def word(f, k):
        return int(base[so[f] + 4 * k:][:4].view("<u4")[0])

    cases = [(0, 0x12345678, 2), (1, 2, 3), (2, w + 8, 4), (5, 4, 4), (8, 0, 4), (14, 0, 4), (12, "+16", 5), (13, "+16", 10), (10, "+1", 10),
             (15, "+4", 8), ("index", None, 8), ("types", None, 8)]
    seen = set()
    for f in range(4):
        for k, value, code in cases:
            bad = base.copy()
            o = so[f]
            if k == "index":  # one more level in the first entry: the counts no longer sum to word 10
                i0 = o + 64 + word(f, 15)
                bad[i0 + 2:i0 + 4].view("<u2")[0] += 1
            elif k == "types":
                bad[o + 64:o + 68].view("<u4")[0] = 2   # neither bitmap nor raw
            elif isinstance(value, str):
                bad[o + 4 * k:o + 4 * k + 4].view("<u4")[0] = word(f, k) + int(value)
            else:
                bad[o + 4 * k:o + 4 * k + 4].view("<u4")[0] = value
            if k == 10 and (geom_levels_off(geom) + 2 * word(f, 10)) % 16 != 0:
                code = 8  # one more level within the same 16 bytes: the SVCQ size still fits, the index's sum does not
            frames = _spoiled(svce, so, geom, windows, bad, f, clean, clean_offs, code)
            _, _, dec = nat.entropy_decode_frames(frames, _offs_dev(so), w, h, tile, mv)
            assert dec.cpu().tolist()[f] == code and sum(dec.cpu().tolist()) == code
            seen.add(code)
    assert seen >= {2, 3, 4, 5, 8, 10}
    # a stream cut short: the last frame runs past svce_bytes
    cut = _dev(svce)[:len(svce) - 16].clone()
    out, out_offs, status = _call(cut, so, geom, windows)
    assert status == [0, 0, 0, 1] and out[out_offs[3]:out_offs[4]].tobytes() == bytes(64)
    assert out[:out_offs[3]].tobytes() == clean[:clean_offs[3]].tobytes()


def geom_levels_off(geom):
    w, h, tile, mv = geom
    return 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * ((tile[0] * tile[1] + 63) // 64)


def test_garbage_in_a_chunk_is_flagged_only_where_it_is_walked(native):
    """The documented contract: a cut chunk is walked to its last kept tile, kept and dropped chunks not at all."""
    geom = HOST_GEOMS[2]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(6), geom, 4, 0.06)
    svce, so = entropy.encode_frames(stream, offs)
    so = [int(o) for o in so]
    base = np.frombuffer(svce, np.uint8)
    # chunk 0 of every frame: tiles 0 .. 31 of the first row of plane 0
    cut, kept, dropped = [(8 * 4, 0, 8 * 20, h)] * 4, [(0, 0, w, h)] * 4, [(8 * 32, 0, w, h)] * 4
    for f in range(4):
        g, start, sizes, counts = chunk_table(frames_of(svce, so)[f])
        assert sizes[0] >= 8 and not base[so[f] + start[0]] & 1
        bad = base.copy()
        p = so[f] + start[0]
        bad[p] &= 0x7F      # the mode bit and the two parameters stay; then 4 zero bytes: a prefix of more than 24 zeros
        bad[p + 1:p + 5] = 0
        clean, clean_offs, status = _call(svce, so, geom, cut)
        assert status == [0] * 4
        _spoiled(svce, so, geom, cut, bad, f, clean, clean_offs, 9)
        for windows in (kept, dropped):
            want, want_offs = entropy.window_frames(bad, so, windows)
            got = _call(bad, so, geom, windows)
            _expect(got, want, want_offs)
            assert got[2] == [0] * 4
            out = frames_of(want, want_offs)[f]
            _, start_o, sizes_o, _ = chunk_table(out)
            payload = out[start_o[0]:start_o[0] + sizes_o[0]]
            assert payload == (bad[p:p + sizes[0]].tobytes() if windows is kept else empty_chunk(32))
        # ... and the decoder of the copied chunk flags it
        out, out_offs, _ = _call(bad, so, geom, kept)
        _, _, dec = nat.entropy_decode_frames(_dev(out[:out_offs[-1]]), _offs_dev(out_offs), w, h, tile, mv)
        want_dec = [0] * 4
        want_dec[f] = 9
        assert dec.cpu().tolist() == want_dec


def test_a_chunk_tiles_that_cannot_be_recoded_and_an_oversize_frame(native):
    # 512 x 64 at 64 x 64: a raw chunk of 8 tiles is 1 + 8 * (8 * 64 + 2 * 4096) = 69 633 bytes
    big = (512, 64, (64, 64), (64, 64))
    stream, offs = random_stream(np.random.default_rng(3), big, 4, 0.001)
    ok7, ok7_offs = entropy.encode_frames(stream, offs, chunk_tiles=7)
    q = frames_of(stream, offs)
    for f in range(4):
        frames = [entropy.encode_frame(q[i], chunk_tiles=8 if i == f else 7) for i in range(4)]
        svce, so = entropy._join(frames)
        for windows in (None, [(64, 0, 128, 64)] * 4, [(0, 0, 0, 0)] * 4):
            clean, clean_offs, status = _call(ok7, ok7_offs, big, windows)
            assert status == [0] * 4
            _spoiled(svce, [int(o) for o in so], big, windows, np.frombuffer(svce, np.uint8), f, clean, clean_offs, 4)
    # 36 x 12 at 4 x 4: nine chunks (a tile row each); every index entry claims 60 000 bytes of filler, consistently with frame_bytes
    geom = HOST_GEOMS[0]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(5), geom, 4, 0.3)
    svce, so = entropy.encode_frames(stream, offs)
    ins = frames_of(svce, so)
    clean, clean_offs, status = _call(svce, so, geom, None)
    assert status == [0] * 4
    for f in range(4):
        g, start, sizes, counts = chunk_table(ins[f])
        assert g.chunks == 9
        src = np.frombuffer(ins[f], np.uint8)
        head = src[:start[0]].copy()
        head[start[0] - 36:].view("<u4")[:] = 60000 | (counts << 16)
        body = b"".join(src[start[c]:start[c] + sizes[c]].tobytes() + bytes(60000 - int(sizes[c])) for c in range(9))
        size = (len(head) + len(body) + 15) // 16 * 16
        head[48:52].view("<u4")[0] = size
        fat = head.tobytes() + body + bytes(size - len(head) - len(body))
        frames = [fat if i == f else ins[i] for i in range(4)]
        bad, bad_offs = entropy._join(frames)
        dev = _spoiled(bad, [int(o) for o in bad_offs], geom, None, np.frombuffer(bad, np.uint8), f, clean, clean_offs, 5)
        # the frame passes the decoder's check (its index is consistent): only the size of the output refuses it
        _, _, dec = nat.entropy_decode_frames(dev, _offs_dev(bad_offs), w, h, tile, mv)
        assert dec.cpu().tolist()[f] == 9 and sum(dec.cpu().tolist()) == 9
        with pytest.raises(ValueError, match="worst canonical"):
            entropy.window_frame(fat, None)


# ---- 7. two runs, refusals -----------------------------------------------------------------------------------------------------------------

def test_two_runs_write_the_same_bytes(native):
    geom = HOST_GEOMS[3]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(7), geom, 4, 0.1)
    svce, so = entropy.encode_frames(stream, offs)
    windows = _windows_of(geom)[5]
    one = _call(svce, so, geom, windows)
    two = _call(svce, so, geom, windows)
    assert one[1] == two[1] and one[2] == two[2] == [0] * 4 and one[0].tobytes() == two[0].tobytes()


def test_refusals_reach_python(native):
    geom = HOST_GEOMS[4]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(8), geom, 2, 0.1)
    svce, so = entropy.encode_frames(stream, offs)
    frames, offsets = _dev(svce), _offs_dev(so)
    with pytest.raises(nat.SvcError, match="not divisible"):
        nat.window_entropy_frames(frames, offsets, w + 1, h, tile, mv, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                                  workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.window_entropy_frames(frames, offsets, w, h, tile, mv, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="worst case"):
        nat.window_entropy_frames(frames, offsets, w, h, tile, mv, src=[0, 1, 1],
                                  out=torch.empty(nat.window_entropy_max_bytes(2, w, h, tile, mv), dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        nat.window_entropy_frames(frames, offsets, w, h, tile, mv,
                                  out=torch.empty(nat.window_entropy_max_bytes(2, w, h, tile, mv) + 16, dtype=torch.uint8, device="cuda")[4:])
    with pytest.raises(nat.SvcError, match="d_src"):
        # (the binding derives n_out from src: the rule is reached through the C call)
        nat._check(nat.load().svc_hip_window_entropy_frames(frames.data_ptr(), frames.numel(), offsets.data_ptr(), 2, None, 3, w, h,
                                                            tile[0], tile[1], mv[0], mv[1], None, None, 0, None, 0, None, None, None))
