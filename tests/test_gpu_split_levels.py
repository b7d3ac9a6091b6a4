"""svc_hip_split_levels_frames and svc_hip_split_levels_budget_frames on the device (include/svc_hip.h: a stored fine SVCQ stream split
into a base stream at any steps plus its enhancement).

Their contract is byte equality with code already in the tree: for odd ratios with both outputs of svc_hip_dct_pack_layers_frames, for any
ratio with layers.split_frames / split_budget_frames, and under svc_hip_decode_layers_frames bit equality with the fine stream's own
decode.  Every call here writes into streams pre-filled with FILL and offsets pre-filled with -1; all n_out + 1 offsets of both layers,
the bytes up to the last one and FILL behind it are asserted."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers, levels
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _fused, _types
from tests.test_gpu_layers import _gaze, _layers, _same_bits, _window
from tests.test_gpu_window_levels import HOST_GEOMS, _windows_of
from tests.test_window_levels_host import GEOMS, geom_dict, random_levels, random_stream, random_types

pytestmark = pytest.mark.gpu


def _dev(stream):
    """A device tensor of exactly the stream's bytes (bytes, a numpy array or a tensor)."""
    if isinstance(stream, torch.Tensor):
        return stream.clone()
    return torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()


def _offsets(offs):
    return offs if isinstance(offs, torch.Tensor) else torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda()


def _rects(windows, n_out):
    """u32 rectangles, some past 2^31: as the i32 tensor the binding takes."""
    if windows is None:
        return None
    return torch.from_numpy(np.asarray(windows, dtype=np.uint32).reshape(n_out, 4).view(np.int32)).cuda()


def _call(stream, offs, geom, steps, windows=None, src=None, enhancement=True, ladder=None, budget=None):
    """The fixed call (steps = (fg, bg, e)) or, with a ladder, the budgeted one (steps = e) on a stream tensor of exactly its bytes ->
    {base, boffs, enh, eoffs, status[, choice]}: whole host arrays and lists."""
    w, h, tile, mv = geom
    frames, offsets = _dev(stream), _offsets(offs)
    n_out = offsets.numel() - 1 if src is None else len(src)
    cap = max(nat.levels_max_bytes(n_out, w, h, tile, mv), 16)
    base = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    enh = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    boffs = torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda")
    eoffs = torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
    kw = dict(window=_rects(windows, n_out), src=src, enhancement=enhancement, base_out=base, base_offsets=boffs, enh_out=enh,
              enh_offsets=eoffs, status=status)
    out = {}
    if ladder is None:
        fg, bg, e = steps
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, e, fg, bg, **kw)
    else:
        choice = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
        nat.split_levels_budget_frames(frames, offsets, w, h, tile, mv, steps, ladder, budget, choice=choice, **kw)
        out["choice"] = [c & 0xFFFFFFFF for c in choice.cpu().tolist()]
    torch.cuda.synchronize()
    out.update(base=base.cpu().numpy(), boffs=boffs.cpu().tolist(), enh=enh.cpu().numpy(), eoffs=eoffs.cpu().tolist(),
               status=status.cpu().tolist())
    return out


def _expect_layer(out, offs, want_bytes, want_offs):
    assert offs == [int(o) for o in want_offs]  # all n_out + 1 of them
    assert out[:offs[-1]].tobytes() == bytes(want_bytes)
    assert (out[offs[-1]:] == FILL).all()  # nothing is written past the stream


def _expect(got, want):
    """want = (base bytes, base offsets, enhancement bytes, its offsets)."""
    _expect_layer(got["base"], got["boffs"], want[0], want[1])
    _expect_layer(got["enh"], got["eoffs"], want[2], want[3])


def _frames_of(out, offs):
    return [out[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]


def _host(t, offs):
    return t[:int(offs[-1])].cpu().numpy().tobytes(), offs.cpu().tolist()


# ---- 1. against the encoder, odd ratios, byte for byte -------------------------------------------------------------------------------------

ENCODE = [(block, w, h, mv, steps, kind)
          for block, w, h, mv in ((8, 272, 24, (16, 8)), (16, 16, 16, MV16), (16, 48, 32, MV16), (16, 144, 48, MV16))
          for steps in ((1, 639, 1), (3, 9, 1), (6, 30, 2))
          for kind in ("none", "empty", "rect", "per-frame")]


@pytest.mark.parametrize("case", ENCODE, ids=lambda c: "-".join(str(x) for x in c).replace(" ", ""))
def test_odd_ratios_give_the_encoders_bytes(native, case):
    block, w, h, mv, (fg, bg, e), kind = case
    n = 4
    bgr = _content("random", n, w, h, 11)
    types = _types("random", n, w, h, mv, 11)
    windows = _window(kind, n, w, h, block)
    fine, fine_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, e, e)
    want_b, want_boffs, want_e, want_eoffs = _layers(bgr, w * h * 3, n, w, h, block, types, mv, fg, bg, e, windows)
    torch.cuda.synchronize()
    got = _call(fine[:int(fine_offs[-1])], fine_offs, (w, h, (block, block), mv), (fg, bg, e), windows)
    _expect(got, _host(want_b, want_boffs) + _host(want_e, want_eoffs))
    assert got["status"] == [0] * n
    # ... and the base alone is the fused pack at (fg, bg)
    direct, direct_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, fg, bg)
    torch.cuda.synchronize()
    _expect_layer(got["base"], got["boffs"], *_host(direct, direct_offs))


# ---- 2. against layers.split_frames on host-built frames ---------------------------------------------------------------------------------

def _levels_before_first_enh_run(fine, base_enh, geom, window):
    """(levels of the FINE frame ahead of the first tile that holds an enhancement level, enhancement levels): the enhancement's first
    run starts at an even level of its frame; an odd count ahead of it in the input puts source and destination at different phases
    inside a dword."""
    w, h, (tw, th), mv = geom
    tx, ty, nw = w // tw, h // th, (tw * th + 63) // 64
    masks_off = 64 + 4 * (w // mv[0]) * (h // mv[1])

    def per_tile(frame):
        b = np.frombuffer(frame, np.uint8)
        return np.unpackbits(b[masks_off:masks_off + 8 * 3 * ty * tx * nw].reshape(3 * ty * tx, nw * 8), axis=-1).sum(-1)
    fine_t, enh_t = per_tile(fine), per_tile(base_enh[1])
    runs = np.flatnonzero(enh_t > 0)
    return (int(fine_t[:runs[0]].sum()) if runs.size else 0), int(enh_t.sum())


@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("geom", HOST_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}")
def test_host_built_frames(native, geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    odd_phase = 0
    # ... and two more lists whose windows leave out the first column of tiles: a frame's first enhanced tile is then never its first tile
    off_origin = [(tile[0], 0, w, h), (tile[0], 0, tile[0], h), (w - tile[0], 0, tile[0], h), (min(2 * tile[0], w - tile[0]), 0, w, h)]
    for windows in _windows_of(geom) + [off_origin, off_origin[::-1]]:
        for fg, bg, e in ((4, 16, 2), (1, 640, 1), (5, 5, 5)):  # every triple under every window list; ratio 1 leaves no residual at all
            frames = []
            for f in range(4):
                lv = random_levels(rng, w, h, {"zero": 0.0, "full": 1.0, "sparse": 0.06}[density])
                lv = np.where(rng.random(lv.shape) < 0.5, lv, np.sign(lv) * (np.abs(lv) % 700))  # half of them small: the ratios zero those
                types = random_types(rng, w, h, mv)
                frame = layers.write_frame(geom_dict(*geom), types, lv, e, e)
                if density == "sparse" and windows is not None and (fg, bg, e) != (5, 5, 5):
                    win = windows[f]
                    before, kept = _levels_before_first_enh_run(frame, layers.split_frame(frame, e, fg, bg, win), geom, win)
                    if kept and before % 2 == 0 and not layers._contains(win, np.array(0), np.array(0)):
                        lv[0, 0, 0] = 0 if lv[0, 0, 0] else 77  # the first coefficient of the first tile, which the window does not hold
                        frame = layers.write_frame(geom_dict(*geom), types, lv, e, e)
                        before, kept = _levels_before_first_enh_run(frame, layers.split_frame(frame, e, fg, bg, win), geom, win)
                        assert before % 2 == 1
                    odd_phase += bool(kept) and before % 2 == 1
                frames.append(frame)
            stream, offs = entropy._join(frames)
            got = _call(stream, offs, geom, (fg, bg, e), windows)
            _expect(got, layers.split_frames(stream, offs, e, fg, bg, windows))
            assert got["status"] == [0] * 4
    if density == "sparse":
        assert odd_phase >= 8  # enhancement runs whose source and destination differ in phase were written, in every geometry


def test_a_set_bit_with_level_zero_is_a_zero_on_the_device(native):
    """By value, not by mask: the zeroed-levels frame of tests/test_split_levels_host.py (eight levels of value 0 whose mask bits stay
    set) among canonical frames.  Counting or writing by the input's mask bits would give other counts, offsets and bytes."""
    geom = GEOMS[1]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(7), geom, 3, 0.5, 2, 2)
    offs = [int(o) for o in offs]
    levels_off = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * 3
    b = np.frombuffer(stream, np.uint8).copy()
    assert int(b[offs[1] + 40:offs[1] + 44].view("<u4")[0]) > 8 and b[offs[1] + levels_off:offs[1] + levels_off + 16].any()
    b[offs[1] + levels_off:offs[1] + levels_off + 16] = 0  # frame 1
    zeroed = b.tobytes()
    frame = zeroed[offs[1]:offs[2]]
    canonical = layers.write_frame(geom_dict(*geom), levels.parse_frame(frame)[1], layers._levels_of(*levels.parse_frame(frame))[0], 2, 2)
    assert canonical != frame
    windows = [(0, 0, w, h), (0, 0, tile[0], h), (tile[0], 0, w, h)]
    ladder = [(2, 2), (4, 16), (6, 1280)]
    for steps in ladder:
        for win in (None, windows):
            got = _call(zeroed, offs, geom, steps + (2,), win)
            want = layers.split_frames(zeroed, offs, 2, *steps, win)
            _expect(got, want)
            assert got["status"] == [0] * 3
            mine = (_frames_of(got["base"], got["boffs"])[1], _frames_of(got["enh"], got["eoffs"])[1])
            assert mine == layers.split_frame(canonical, 2, *steps, None if win is None else win[1])  # the canonical frame's outputs
    got = _call(zeroed, offs, geom, (2, 2, 2), None)
    assert _frames_of(got["base"], got["boffs"])[1] == canonical  # ratio 1: the canonical frame itself
    # the budgeted count is by value too: budgets at and 16 below the canonical frame's size, per entry
    sizes = [len(layers.split_frame(canonical, 2, fg, bg)[0]) for fg, bg in ladder]
    for k in range(3):
        for budget, pick in ((sizes[k], min(j for j in range(3) if sizes[j] <= sizes[k])), (sizes[k] - 16, None)):
            got = _call(zeroed, offs, geom, 2, windows, src=[1, 1, 1], ladder=ladder, budget=budget)
            want = layers.split_budget_frames(zeroed, offs, 2, ladder, budget, windows, [1, 1, 1])
            assert got["choice"] == [int(c) for c in want[4]]
            if pick is not None:
                assert got["choice"] == [pick] * 3
            _expect(got, want[:4])


# ---- 3. decode, even ratios ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
@pytest.mark.parametrize("steps", [(1, 640, 1), (4, 16, 2)], ids=str)
def test_decode_under_a_gaze(native, block, w, h, mv, steps):
    fg, bg, e = steps
    n = 4
    bgr = _content("random" if fg == 1 else "synth", n, w, h, 13)
    types = _types("random", n, w, h, mv, 13)
    fine, fine_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, e, e)
    torch.cuda.synchronize()
    fine = fine[:int(fine_offs[-1])].clone()

    def split(windows):
        b, bo, en, eo, st = nat.split_levels_frames(fine, fine_offs, w, h, block, mv, e, fg, bg, window=windows)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n
        return b[:int(bo[-1])], bo, en[:int(eo[-1])], eo
    dec = (2, 24)  # the decoder's steps outside the gaze
    whole = [(0, 0, w, h)] * n
    b, bo, en, eo = split(None)
    rec, _, st = nat.decode_layers_frames(b, bo, en, eo, w, h, block, mv, *dec, gaze=whole)
    ref, _, st_ref = nat.decode_levels_frames(fine, fine_offs, w, h, block, mv, *dec, gaze=whole)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st_ref.cpu().tolist() == [0] * n and _same_bits(rec, ref)
    # a gaze per frame and a rect window: inside both, the fine stream's decode; everywhere else the base's own
    windows, gaze = _window("rect", n, w, h, block), _gaze("per-frame", n, w, h)
    b, bo, en, eo = split(windows)
    rec, _, st = nat.decode_layers_frames(b, bo, en, eo, w, h, block, mv, *dec, gaze=gaze)
    fine_rec, _, _ = nat.decode_levels_frames(fine, fine_offs, w, h, block, mv, *dec, gaze=gaze)
    base_rec, _, _ = nat.decode_levels_frames(b, bo, w, h, block, mv, *dec, gaze=gaze)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    oy = (torch.arange(h) // block * block)[:, None]
    ox = (torch.arange(w) // block * block)[None, :]
    both = torch.stack([(ox >= g[0]) & (ox < g[0] + g[2]) & (oy >= g[1]) & (oy < g[1] + g[3]) &
                        (ox >= r[0]) & (ox < r[0] + r[2]) & (oy >= r[1]) & (oy < r[1] + r[3]) for g, r in zip(gaze, windows)])
    assert both.any() and not both.all()
    got, fine_bits, base_bits = (t.cpu().contiguous().view(torch.int32) for t in (rec, fine_rec, base_rec))
    assert torch.equal(got[both], fine_bits[both]) and torch.equal(got[~both], base_bits[~both])


# ---- 4. composition with the window call ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_windows_compose_with_the_window_call(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(6), geom, 4, 0.3, 2, 2)
    src = [1, 3, 3, 0, 2]
    windows = [(tile[0], 0, w, h), (0, 0, w // 2, h), (0, 0, 0, 0), (0, 0, w, h), (w - 2 * tile[0], 0, w, tile[1])]
    got = _call(stream, offs, geom, (4, 16, 2), windows, src)
    whole = _call(stream, offs, geom, (4, 16, 2), None, None)
    assert got["status"] == [0] * 5 and whole["status"] == [0] * 4
    used = whole["eoffs"][-1]
    out, out_offs, st = nat.window_levels_frames(torch.from_numpy(whole["enh"][:used].copy()).cuda(), _offsets(whole["eoffs"]), w, h, tile, mv,
                                                 window=windows, src=src)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 5
    _expect_layer(got["enh"], got["eoffs"], *_host(out, out_offs))
    assert _frames_of(got["base"], got["boffs"]) == [_frames_of(whole["base"], whole["boffs"])[s] for s in src]


# ---- 5. d_src ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_source_indices(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(3), geom, 4, 0.3, 1, 1)
    src = [3, 0, 0, 2, 7, 1]
    windows = [(tile[0], 0, w, h), (0, 0, w, h), (0, 0, w // 2, h), (0, 0, 0, 0), (0, 0, w, h), (w - 2 * tile[0], 0, w, tile[1])]
    got = _call(stream, offs, geom, (1, 640, 1), windows, src)
    assert got["status"] == [0, 0, 0, 0, 1, 0]
    base, enh = _frames_of(got["base"], got["boffs"]), _frames_of(got["enh"], got["eoffs"])
    assert base[4] == enh[4] == bytes(64)
    assert (got["base"][got["boffs"][-1]:] == FILL).all() and (got["enh"][got["eoffs"][-1]:] == FILL).all()
    for i, s in enumerate(src):
        if i == 4:
            continue
        ident = _call(stream, offs, geom, (1, 640, 1), [windows[i]] * 4)  # the identity call with this window for every frame: its frame s
        assert ident["status"] == [0] * 4
        want = layers.split_frame(stream[int(offs[s]):int(offs[s + 1])], 1, 1, 640, windows[i])
        assert (base[i], enh[i]) == (_frames_of(ident["base"], ident["boffs"])[s], _frames_of(ident["enh"], ident["eoffs"])[s]) == want
    # no window, every frame twice
    twice = [0, 0, 1, 1, 2, 2, 3, 3]
    _expect(_call(stream, offs, geom, (1, 640, 1), None, twice), layers.split_frames(stream, offs, 1, 1, 640, None, twice))


# ---- 6. malformed input -----------------------------------------------------------------------------------------------------------------

def test_malformed_frames(native):
    geom = GEOMS[1]  # 12 x 12 tiles: 144 of a tile's 192 mask bits are coefficients
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(4), geom, 4, 0.3, 2, 2)
    windows = [(0, 0, w, h), (12, 0, 12, 24), (0, 12, 36, 12), (24, 0, 12, 12)]
    steps = (4, 16, 2)
    clean = _call(stream, offs, geom, steps, windows)
    assert clean["status"] == [0] * 4
    clean_frames = {k: _frames_of(clean[k], clean[o]) for k, o in (("base", "boffs"), ("enh", "eoffs"))}
    levels_off = 64 + 4 * 6 + 8 * 3 * 6 * 3
    offs_dev = _offsets(offs)

    def word(f, k):
        return int(np.frombuffer(stream, np.uint8)[int(offs[f]) + 4 * k:][:4].view("<u4")[0])

    def check(got, f):
        for k, o in (("base", "boffs"), ("enh", "eoffs")):
            want = [bytes(64) if i == f else fr for i, fr in enumerate(clean_frames[k])]
            assert got[o] == [sum(len(x) for x in want[:i]) for i in range(5)]
            assert _frames_of(got[k], got[o]) == want
            assert (got[k][got[o][-1]:] == FILL).all()

    cases = [(0, 0x12345678, 2), (1, 2, 3), (2, w + 12, 4), (5, 6, 4), (8, 0, 4), (12, None, 5), (10, +1, 6), (10, -1, 6), ("stray", None, 7),
             (8, 4, 11), (9, 4, 11), (8, 1, 11)]  # ... and a frame that is not at fine_step: status 11
    seen = set()
    for f in range(4):
        for k, value, code in cases:
            bad = np.frombuffer(stream, np.uint8).copy()
            o = int(offs[f])
            if k == "stray":
                bad[o + levels_off - 1] |= 0x40  # bit 190 of the frame's last tile: past its 144 coefficients
            elif k == 12:
                bad[o + 48:o + 52].view("<u4")[0] = word(f, 12) + 16
            elif k == 10:
                bad[o + 40:o + 44].view("<u4")[0] = word(f, 10) + value
            else:
                bad[o + 4 * k:o + 4 * k + 4].view("<u4")[0] = value
            if k == 10 and value == 1 and (levels_off + 2 * word(f, 10)) % 16 == 0:
                code = 5  # one more level no longer fits the frame's bytes: the size check comes first
            frames = _dev(bad)  # exactly the stream's bytes: a read past them is outside the allocation
            _, _, unpack = nat.unpack_levels_frames(frames, offs_dev, w, h, tile, mv)
            got = _call(frames, offs_dev, geom, steps, windows)
            want = [0] * 4
            want[f] = code
            assert got["status"] == want, (f, k, value)
            assert unpack.cpu().tolist() == ([0] * 4 if code == 11 else want)  # 11 is a frame the unpack takes
            seen.add(code)
            check(got, f)
    assert seen >= {2, 3, 4, 5, 6, 7, 11}
    # a stream cut short: the last frame runs past stream_bytes
    cut = _dev(stream)[:len(stream) - 16].clone()
    got = _call(cut, offs_dev, geom, steps, windows)
    assert got["status"] == [0, 0, 0, 1]
    check(got, 3)
    # the budgeted call reports the same, and a frame that fails has choice 0
    bad = np.frombuffer(stream, np.uint8).copy()
    bad[int(offs[1]) + 32:int(offs[1]) + 36].view("<u4")[0] = 4
    got = _call(bad, offs, geom, 2, windows, ladder=[(2, 2), (4, 16)], budget=0)
    assert got["status"] == [0, 11, 0, 0] and got["choice"] == [0x80000001, 0, 0x80000001, 0x80000001]
    check(got, 1)


# ---- 7. slack after the input's levels -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_input_with_slack_after_its_levels(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(5), geom, 4, 0.3, 2, 2)
    offs = [int(o) for o in offs]
    b = np.frombuffer(stream, np.uint8)
    slack = np.concatenate([b[:offs[2]], np.zeros(16, np.uint8), b[offs[2]:]])  # behind frame 1
    slack[offs[1] + 48:offs[1] + 52].view("<u4")[0] += 16
    slack_offs = offs[:2] + [o + 16 for o in offs[2:]]
    for windows in (None, [(tile[0], 0, w // 2, h)] * 4):
        got = _call(slack, slack_offs, geom, (4, 16, 2), windows)
        _expect(got, layers.split_frames(stream, offs, 2, 4, 16, windows))
        assert got["status"] == [0] * 4


# ---- 8. base only ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[1], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_base_only(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(9), geom, 4, 0.3, 1, 1)
    both = _call(stream, offs, geom, (3, 640, 1), [(0, 0, w // 2, h)] * 4)
    only = _call(stream, offs, geom, (3, 640, 1), [(0, 0, w // 2, h)] * 4, enhancement=False)
    _expect_layer(only["base"], only["boffs"], both["base"][:both["boffs"][-1]].tobytes(), both["boffs"])
    assert (only["enh"] == FILL).all() and only["eoffs"] == [-1] * 5 and only["status"] == [0] * 4
    budgeted = _call(stream, offs, geom, 1, None, enhancement=False, ladder=[(3, 640)], budget=0)
    _expect_layer(budgeted["base"], budgeted["boffs"], both["base"][:both["boffs"][-1]].tobytes(), both["boffs"])
    assert (budgeted["enh"] == FILL).all() and budgeted["eoffs"] == [-1] * 5


# ---- 9. the budget ---------------------------------------------------------------------------------------------------------------------------

def _small_stream(rng, geom, n, e):
    """n frames at (e, e) of densities 0.3, 0.06, 1, ... with magnitudes below 900: the ladder's ratios (up to 640) zero a good part."""
    w, h, tile, mv = geom
    frames = []
    for f in range(n):
        lf = random_levels(rng, w, h, (0.3, 0.06, 1.0)[f % 3])
        frames.append(layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), np.sign(lf) * (np.abs(lf) % 900), e, e))
    return entropy._join(frames)


@pytest.mark.parametrize("geom", [GEOMS[2], (144, 48, (16, 16), MV16)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("e", [1, 2])
def test_budget(native, geom, e):
    w, h, tile, mv = geom
    n = 4
    stream, offs = _small_stream(np.random.default_rng(w + e), geom, n, e)
    full = [(int(fg) * e, int(bg) * e) for fg, bg in levels.step_ladder(1, 4, 1, 640, 6, 2)]
    windows = _window("per-frame", n, w, h, tile[0])
    for ladder in ([(3 * e, 640 * e)], full):
        sizes = [len(layers.split_frame(stream[int(offs[0]):int(offs[1])], e, fg, bg)[0]) for fg, bg in ladder]
        floor = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * (tile[0] * tile[1] // 64)
        # everything fits; some entries fit (frame 0's middle entry); below the masks' floor; a mix per frame
        for budget in (1 << 30, sizes[len(sizes) // 2], floor - 16, [1 << 30, sizes[-1], 0, sizes[len(sizes) // 2]]):
            got = _call(stream, offs, geom, e, windows, ladder=ladder, budget=budget)
            want = layers.split_budget_frames(stream, offs, e, ladder, budget, windows)
            assert got["choice"] == [int(c) for c in want[4]] and got["status"] == [0] * n
            _expect(got, want[:4])
            base, enh = _frames_of(got["base"], got["boffs"]), _frames_of(got["enh"], got["eoffs"])
            for pick in sorted({c & 0x7FFFFFFF for c in got["choice"]}):  # each frame is the fixed call's frame at its pair
                fixed = _call(stream, offs, geom, ladder[pick] + (e,), windows)
                fb, fe = _frames_of(fixed["base"], fixed["boffs"]), _frames_of(fixed["enh"], fixed["eoffs"])
                for i, c in enumerate(got["choice"]):
                    if c & 0x7FFFFFFF == pick:
                        assert (base[i], enh[i]) == (fb[i], fe[i])
            if budget == 1 << 30:
                assert got["choice"] == [0] * n
            if budget == floor - 16:
                assert got["choice"] == [(len(ladder) - 1) | 0x80000000] * n
    # a repeated frame under two budgets takes two entries
    sizes = [len(layers.split_frame(stream[int(offs[2]):int(offs[3])], e, fg, bg)[0]) for fg, bg in full]
    assert sizes[0] > sizes[-1]
    got = _call(stream, offs, geom, e, None, src=[2, 2, 0], ladder=full, budget=[sizes[0], sizes[-1], 1 << 30])
    want = layers.split_budget_frames(stream, offs, e, full, [sizes[0], sizes[-1], 1 << 30], None, [2, 2, 0])
    assert got["choice"] == [int(c) for c in want[4]] and got["choice"][0] == 0 and 0 < got["choice"][1] < len(full)
    _expect(got, want[:4])


# ---- 10. two runs, and through the entropy coder ---------------------------------------------------------------------------------------------

def test_two_runs_and_the_entropy_coder(native):
    block, w, h, mv, n = 8, 272, 24, (16, 8), 4
    geom = (w, h, (block, block), mv)
    bgr, types = _content("synth", n, w, h, 17), _types("random", n, w, h, mv, 17)
    fine, fine_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, 1, 1)
    torch.cuda.synchronize()
    windows = _window("per-frame", n, w, h, block)
    ladder = [(int(fg), int(bg)) for fg, bg in levels.step_ladder(1, 4, 1, 640, 6, 2)]
    for kw in (dict(steps=(1, 640, 1)), dict(steps=1, ladder=ladder, budget=4000)):
        one = _call(fine[:int(fine_offs[-1])], fine_offs, geom, windows=windows, **kw)
        two = _call(fine[:int(fine_offs[-1])], fine_offs, geom, windows=windows, **kw)
        assert all(np.array_equal(one[k], two[k]) if isinstance(one[k], np.ndarray) else one[k] == two[k] for k in one)
        assert one["status"] == [0] * n
        for k, o in (("base", "boffs"), ("enh", "eoffs")):
            used = one[o][-1]
            mine, mine_offs = torch.from_numpy(one[k][:used].copy()).cuda(), torch.tensor(one[o], dtype=torch.int64, device="cuda")
            coded, coded_offs, st = nat.entropy_encode_frames(mine, mine_offs, w, h, block, mv)
            back, back_offs, st_back = nat.entropy_decode_frames(coded[:int(coded_offs[-1])].clone(), coded_offs, w, h, block, mv)
            torch.cuda.synchronize()
            assert st.cpu().tolist() == st_back.cpu().tolist() == [0] * n
            assert back_offs.cpu().tolist() == one[o] and back[:used].cpu().numpy().tobytes() == one[k][:used].tobytes()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[4]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(8), geom, 2, 0.1, 2, 2)
    frames, offsets = _dev(stream), _offsets(offs)
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    cap2 = nat.levels_max_bytes(2, w, h, tile, mv)
    with pytest.raises(nat.SvcError, match="not divisible"):
        nat.split_levels_frames(frames, offsets, w + 1, h, tile, mv, 2, 4, 16, base_out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                                enh_out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"), workspace=small)
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, 2, 4, 16, workspace=small)
    with pytest.raises(nat.SvcError, match="worst case"):
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, 2, 4, 16, src=[0, 1, 1], base_out=torch.empty(cap2, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="worst case"):
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, 2, 4, 16, src=[0, 1, 1], enh_out=torch.empty(cap2, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, 2, 4, 16, base_out=torch.empty(cap2 + 16, dtype=torch.uint8, device="cuda")[4:])
    with pytest.raises(nat.SvcError, match="multiples of fine_step"):
        nat.split_levels_frames(frames, offsets, w, h, tile, mv, 2, 4, 7)
    with pytest.raises(nat.SvcError, match="multiples of fine_step"):
        nat.split_levels_budget_frames(frames, offsets, w, h, tile, mv, 2, [(2, 2), (4, 7)], 1000)
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.split_levels_budget_frames(frames, offsets, w, h, tile, mv, 2, [(2, 2), (4, 16)], 1000,
                                       workspace=torch.empty(nat.split_levels_workspace_bytes(2, 2, w, h, tile, mv), dtype=torch.uint8, device="cuda"))
