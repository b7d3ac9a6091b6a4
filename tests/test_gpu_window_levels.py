"""svc_hip_window_levels_frames on the device (include/svc_hip.h: a stored SVCQ stream restricted to a window per output frame).

Its contract is byte equality with code already in the tree: on the every-tile enhancement stream of svc_hip_dct_pack_layers_frames the
output is the enhancement stream that call writes with the same windows, and on any SVCQ stream it is layers.window_frames.  Every call
here writes into a stream pre-filled with FILL and offsets pre-filled with -1; all n_out + 1 offsets, the bytes up to the last one and
FILL behind it are asserted."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _types
from tests.test_gpu_layers import _gaze, _layers, _same_bits, _window
from tests.test_window_levels_host import GEOMS, geom_dict, random_levels, random_stream, random_types

pytestmark = pytest.mark.gpu


def _dev(stream):
    """A device tensor of exactly the stream's bytes (bytes, a numpy array or a tensor)."""
    if isinstance(stream, torch.Tensor):
        return stream.clone()
    return torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()


def _call(stream, offs, geom, windows=None, src=None):
    """svc_hip_window_levels_frames on a stream tensor of exactly its bytes -> (output u8 on the host, offsets, status), each whole."""
    w, h, tile, mv = geom
    frames = _dev(stream)
    offsets = torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda() if not isinstance(offs, torch.Tensor) else offs
    n_out = offsets.numel() - 1 if src is None else len(src)
    out = torch.full((max(nat.levels_max_bytes(n_out, w, h, tile, mv), 16),), FILL, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n_out,), -1, dtype=torch.int32, device="cuda")
    win = None  # u32 rectangles, some past 2^31: as the i32 tensor the binding takes
    if windows is not None:
        win = torch.from_numpy(np.asarray(windows, dtype=np.uint32).reshape(n_out, 4).view(np.int32)).cuda()
    nat.window_levels_frames(frames, offsets, w, h, tile, mv, window=win, src=src, out=out, out_offsets=out_offs, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_offs.cpu().tolist(), status.cpu().tolist()


def _expect(got, want_bytes, want_offs):
    out, offs, _ = got
    assert offs == [int(o) for o in want_offs]  # all n_out + 1 of them
    assert out[:offs[-1]].tobytes() == bytes(want_bytes)
    assert (out[offs[-1]:] == FILL).all()  # nothing is written past the stream


# ---- 1. against the encoder, byte for byte --------------------------------------------------------------------------------------------

ENCODE = [(block, w, h, mv, steps, kind)
          for block, w, h, mv in ((8, 272, 24, (16, 8)), (16, 16, 16, MV16), (16, 48, 32, MV16), (16, 144, 48, MV16))
          for steps in ((1, 640, 1), (4, 16, 2))
          for kind in ("none", "empty", "whole", "rect", "per-frame")]


def _encode(block, w, h, mv, steps, kind, n=4, seed=11):
    """-> (base, its offsets, the every-tile enhancement, its offsets, the enhancement encoded with the windows, its offsets, windows)."""
    bgr = _content("random" if steps[0] == 1 else "synth", n, w, h, seed)
    types = _types("random", n, w, h, mv, seed)
    windows = _window(kind, n, w, h, block)
    base, base_offs, whole, whole_offs = _layers(bgr, w * h * 3, n, w, h, block, types, mv, *steps, None)
    _, _, want, want_offs = _layers(bgr, w * h * 3, n, w, h, block, types, mv, *steps, windows)
    torch.cuda.synchronize()
    return base, base_offs, whole, whole_offs, want, want_offs, windows


@pytest.mark.parametrize("case", ENCODE, ids=lambda c: "-".join(str(x) for x in c).replace(" ", ""))
def test_windowing_the_stored_enhancement_gives_the_encoders_bytes(native, case):
    block, w, h, mv, steps, kind = case
    _, _, whole, whole_offs, want, want_offs, windows = _encode(*case)
    got = _call(whole[:int(whole_offs[-1])], whole_offs, (w, h, (block, block), mv), windows)
    used = int(want_offs[-1])
    _expect(got, want[:used].cpu().numpy().tobytes(), want_offs.cpu().tolist())
    assert got[2] == [0] * 4
    assert used <= int(whole_offs[-1]) and (kind not in ("none", "whole") or used == int(whole_offs[-1]))


# ---- 2. against layers.window_frames on host-built frames -------------------------------------------------------------------------------

HOST_GEOMS = GEOMS + [
    (128, 64, (64, 64), (64, 64)),   # 64 mask words per tile: a group is one tile
    (16, 704, (8, 8), (16, 16)),     # 264 groups of the work split: more than one pass of the per-frame scan's workgroup
]


def _windows_of(geom):
    """Lists of four windows (one per frame of a batch): none, empty, whole, past the frame, single tiles, edges inside tiles, and the
    left edge on, one tile before and one after tile 32 of a row (the first tile of a row's second group at 8 x 8) where a row has one,
    else around tile 1."""
    w, h, (tw, th), _ = geom
    out = [None, [(0, 0, 0, h), (0, 0, w, 0), (5, 5, 0, 0), (0, 0, 0, 0)], [(0, 0, w, h)] * 4,
           [(w, 0, 50, h), (0, h, w, 7), (w + 5, h + 5, 1, 1), (0xFFFFFFF0, 0, 0xFFFFFFFF, h)],            # past the frame
           [(tw, 0, tw, th), (w - tw, h - th, tw, th), (0, 0, 1, 1), (w // tw // 2 * tw, h // th // 2 * th, 1, 1)],  # single tiles
           [(max(0, w - 27), 3, 20, max(1, h - 5)), (3, 0, w, h - 1), (0, th, w, th), (tw * 2 - 1, 1, w // 2, h)]]
    t = 32 if w > 33 * tw else 1
    for x in (t * tw, (t - 1) * tw, (t + 1) * tw):
        out.append([(x, 0, w, h), (x, th if h > th else 0, 2 * tw, th), (x, 0, tw, h), (x, 0, 0xFFFFFFFF, 0xFFFFFFFF)])
    return out


def _levels_before_first_run(frame, geom, window):
    """(levels of the frame ahead of the window's first kept level, kept levels), from the masks."""
    w, h, (tw, th), mv = geom
    tx, ty, nw = w // tw, h // th, (tw * th + 63) // 64
    masks_off = 64 + 4 * (w // mv[0]) * (h // mv[1])
    b = np.frombuffer(frame, np.uint8)
    per_tile = np.unpackbits(b[masks_off:masks_off + 8 * 3 * ty * tx * nw].reshape(3, ty, tx, nw * 8), axis=-1).sum(-1)
    ox, oy = np.arange(tx) * tw, np.arange(ty) * th
    x, y, ww, hh = (int(v) for v in window)
    keep = ((ox >= x) & (ox - x < ww))[None, :] & ((oy >= y) & (oy - y < hh))[:, None]
    flat, kept = per_tile.reshape(-1), np.broadcast_to(keep[None], per_tile.shape).reshape(-1)
    runs = np.flatnonzero(kept & (flat > 0))
    return (int(flat[:runs[0]].sum()) if runs.size else 0), int(flat[kept].sum())


@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("geom", HOST_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}")
def test_host_built_frames(native, geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    odd_phase = 0
    for windows in _windows_of(geom):
        frames = []
        for f in range(4):
            lv = random_levels(rng, w, h, {"zero": 0.0, "full": 1.0, "sparse": 0.06}[density])
            types = random_types(rng, w, h, mv)
            frame = layers.write_frame(geom_dict(*geom), types, lv, 4, 16)
            if density == "sparse" and windows is not None:
                # an odd number of levels ahead of the window's first run: the run starts at an even level of the output frame and at
                # an odd one of the input, so its source and destination differ in their phase inside a dword and a 16-byte vector
                before, kept = _levels_before_first_run(frame, geom, windows[f])
                if kept and before % 2 == 0 and not layers._contains(windows[f], np.array(0), np.array(0)):
                    lv[0, 0, 0] = 0 if lv[0, 0, 0] else 77  # the first coefficient of the first tile, which the window does not hold
                    frame = layers.write_frame(geom_dict(*geom), types, lv, 4, 16)
                    before, kept = _levels_before_first_run(frame, geom, windows[f])
                    assert before % 2 == 1
                odd_phase += bool(kept) and before % 2 == 1
            frames.append(frame)
        stream, offs = entropy._join(frames)
        want, want_offs = layers.window_frames(stream, offs, windows)
        got = _call(stream, offs, geom, windows)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 4
    if density == "sparse":
        assert odd_phase >= 8  # runs whose source and destination differ in phase were copied, in every geometry


# ---- 3. d_src ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_source_indices(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(3), geom, 4, 0.3)
    src = [3, 0, 0, 2, 7, 1]
    windows = [(tile[0], 0, w, h), None, (0, 0, w // 2, h), (0, 0, 0, 0), (0, 0, w, h), (w - 2 * tile[0], 0, w, tile[1])]
    windows = [(0, 0, w, h) if r is None else r for r in windows]
    out, out_offs, status = _call(stream, offs, geom, windows, src)
    assert status == [0, 0, 0, 0, 1, 0]
    frames = [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(6)]
    assert frames[4] == bytes(64)
    assert (out[out_offs[-1]:] == FILL).all()
    for i, s in enumerate(src):
        if i == 4:
            continue
        # the identity call on the whole stream with this window for every frame: its frame s
        ident, ident_offs, st = _call(stream, offs, geom, [windows[i]] * 4)
        assert st == [0] * 4
        assert frames[i] == ident[ident_offs[s]:ident_offs[s + 1]].tobytes() == layers.window_frame(
            stream[int(offs[s]):int(offs[s + 1])], windows[i])
    # no window, every frame twice
    got = _call(stream, offs, geom, None, [0, 0, 1, 1, 2, 2, 3, 3])
    want, want_offs = layers.window_frames(stream, offs, None, [0, 0, 1, 1, 2, 2, 3, 3])
    _expect(got, want, want_offs)


# ---- 4. malformed input -----------------------------------------------------------------------------------------------------------------

def test_malformed_frames(native):
    geom = GEOMS[1]  # 12 x 12 tiles: 144 of a tile's 192 mask bits are coefficients
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(4), geom, 4, 0.3)
    windows = [(0, 0, w, h), (12, 0, 12, 24), (0, 12, 36, 12), (24, 0, 12, 12)]
    clean, clean_offs, status = _call(stream, offs, geom, windows)
    assert status == [0] * 4
    levels_off = 64 + 4 * 6 + 8 * 3 * 6 * 3
    offs_dev = torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda()

    def word(f, k):
        return int(np.frombuffer(stream, np.uint8)[int(offs[f]) + 4 * k:][:4].view("<u4")[0])

    cases = [(0, 0x12345678, 2), (1, 2, 3), (2, w + 12, 4), (5, 6, 4), (8, 0, 4), (12, None, 5), (10, +1, 6), (10, -1, 6), ("stray", None, 7)]
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
            out, out_offs, status = _call(frames, offs_dev, geom, windows)
            want = [0] * 4
            want[f] = code
            assert status == unpack.cpu().tolist() == want, (f, k, value)
            seen.add(code)
            sizes = [clean_offs[i + 1] - clean_offs[i] if i != f else 64 for i in range(4)]
            assert out_offs == [sum(sizes[:i]) for i in range(5)]
            for i in range(4):
                frame = out[out_offs[i]:out_offs[i + 1]].tobytes()
                assert frame == (bytes(64) if i == f else clean[clean_offs[i]:clean_offs[i + 1]].tobytes()), (f, k, i)
            assert (out[out_offs[-1]:] == FILL).all()
    assert seen >= {2, 3, 4, 5, 6, 7}
    # a stream cut short: the last frame runs past stream_bytes
    cut = _dev(stream)[:len(stream) - 16].clone()
    out, out_offs, status = _call(cut, offs_dev, geom, windows)
    assert status == [0, 0, 0, 1] and out[out_offs[3]:out_offs[4]].tobytes() == bytes(64)
    assert out[:out_offs[3]].tobytes() == clean[:clean_offs[3]].tobytes()


# ---- 5. slack after the levels ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_input_with_slack_after_its_levels(native, geom):
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(5), geom, 4, 0.3)
    offs = [int(o) for o in offs]
    b = np.frombuffer(stream, np.uint8)
    slack = np.concatenate([b[:offs[2]], np.zeros(16, np.uint8), b[offs[2]:]])  # behind frame 1
    slack[offs[1] + 48:offs[1] + 52].view("<u4")[0] += 16
    slack_offs = offs[:2] + [o + 16 for o in offs[2:]]
    for windows in (None, [(tile[0], 0, w // 2, h)] * 4):
        want, want_offs = layers.window_frames(stream, offs, windows)
        got = _call(slack, slack_offs, geom, windows)
        _expect(got, want, want_offs)
        assert got[2] == [0] * 4


# ---- 6. two runs, and through the entropy coder ------------------------------------------------------------------------------------------

def test_two_runs_and_the_entropy_coder(native):
    block, w, h, mv = 8, 272, 24, (16, 8)
    _, _, whole, whole_offs, want, want_offs, windows = _encode(block, w, h, mv, (1, 640, 1), "per-frame")
    geom = (w, h, (block, block), mv)
    one = _call(whole[:int(whole_offs[-1])], whole_offs, geom, windows)
    two = _call(whole[:int(whole_offs[-1])], whole_offs, geom, windows)
    assert one[1] == two[1] and one[2] == two[2] and one[0].tobytes() == two[0].tobytes()
    used = one[1][-1]
    mine = torch.from_numpy(one[0][:used].copy()).cuda()
    coded, coded_offs, st = nat.entropy_encode_frames(mine, torch.tensor(one[1], dtype=torch.int64, device="cuda"), w, h, block, mv)
    ref, ref_offs, st_ref = nat.entropy_encode_frames(want[:int(want_offs[-1])].clone(), want_offs, w, h, block, mv)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st_ref.cpu().tolist() == [0] * 4
    assert torch.equal(coded_offs, ref_offs) and torch.equal(coded[:int(coded_offs[-1])], ref[:int(ref_offs[-1])])


# ---- 7. decode under a gaze ----------------------------------------------------------------------------------------------------------------

def test_decode_under_a_gaze(native):
    block, w, h, mv, n = 16, 144, 48, MV16, 4
    base, base_offs, whole, whole_offs, want, want_offs, windows = _encode(block, w, h, mv, (4, 16, 2), "rect")
    out, out_offs, status = nat.window_levels_frames(whole[:int(whole_offs[-1])].clone(), whole_offs, w, h, block, mv, window=windows)
    gaze = _gaze("per-frame", n, w, h)
    ub = int(base_offs[-1])
    rec, _, st = nat.decode_layers_frames(base[:ub], base_offs, out[:int(out_offs[-1])], out_offs, w, h, block, mv, 1, 640, gaze=gaze)
    ref, _, st_ref = nat.decode_layers_frames(base[:ub], base_offs, want[:int(want_offs[-1])], want_offs, w, h, block, mv, 1, 640, gaze=gaze)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == st.cpu().tolist() == st_ref.cpu().tolist() == [0] * n
    assert _same_bits(rec, ref)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_reach_python(native):
    geom = GEOMS[4]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(8), geom, 2, 0.1)
    frames, offsets = _dev(stream), torch.as_tensor(np.asarray(offs).astype(np.int64)).cuda()
    with pytest.raises(nat.SvcError, match="not divisible"):
        nat.window_levels_frames(frames, offsets, w + 1, h, tile, mv, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                                 workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.window_levels_frames(frames, offsets, w, h, tile, mv, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="worst case"):
        nat.window_levels_frames(frames, offsets, w, h, tile, mv, src=[0, 1, 1], out=torch.empty(nat.levels_max_bytes(2, w, h, tile, mv),
                                                                                                dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="aligned"):
        nat.window_levels_frames(frames, offsets, w, h, tile, mv,
                                 out=torch.empty(nat.levels_max_bytes(2, w, h, tile, mv) + 16, dtype=torch.uint8, device="cuda")[4:])
