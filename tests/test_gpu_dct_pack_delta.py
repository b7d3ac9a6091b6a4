"""svc_hip_dct_pack_delta_frames (csrc/dct_pack.hip): the delta stream straight from the pixels is, byte for byte, what
svc_hip_dct_pack_levels_frames followed by svc_hip_delta_levels_frames leave on the same device, and what layers.delta_frames (numpy,
independent of the device's delta kernel) makes of the fused pack's frames.  Shapes are those of tests/test_gpu_dct_pack.py at which
the fused body can break; frame counts are chosen so that a key flag falls inside a run, a run is cut short at the end of the call (11
frames, for every run length above 1) and a call holds a single frame."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from scalable_video_codec_amd import synth

pytestmark = pytest.mark.gpu

FILL = 0xA5
MV16 = (16, 16)


def _content(kind, n, w, h, seed):
    if kind == "synth":
        clip = synth.SynthClip(max(w, 64), max(h, 64), n, seed, device="cuda")  # (the generator needs room for its rectangles)
        return torch.stack([clip.frame_bgr(t)[:h, :w] for t in range(n)]).contiguous()
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "equal":  # every frame the same random frame
        return torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, device="cuda", generator=g).expand(n, h, w, 3).contiguous()
    if kind == "white-zero":  # white, zero, white, ..: DC differences of both signs
        out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
        out[0::2] = 255
        return out
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)


def _types(kind, n, w, h, mv, seed):
    mfw, mfh = w // mv[0], h // mv[1]
    if kind == "zero":
        t = torch.zeros((n, mfh, mfw), dtype=torch.int32)
    elif kind == "checker":  # flips every frame: no tile keeps its class
        yy, xx = torch.meshgrid(torch.arange(mfh), torch.arange(mfw), indexing="ij")
        t = ((yy + xx) & 1).to(torch.int32).expand(n, mfh, mfw).clone()
        t[1::2] ^= 1
    else:
        rng = np.random.default_rng(seed)
        t = torch.from_numpy(rng.choice(np.array([0, 1, 7], dtype=np.int32), size=(n, mfh, mfw)))
    return t.reshape(n, mfh * mfw).contiguous().cuda()


def _strided(bgr, extra):
    """The frames in a flat buffer with `extra` bytes (of noise) between them -> (buffer, stride)."""
    n = bgr.shape[0]
    per = bgr[0].numel()
    buf = torch.randint(0, 256, (n * (per + extra),), dtype=torch.uint8, device="cuda")
    buf.view(n, per + extra)[:, :per] = bgr.view(n, per)
    return buf, per + extra


def _fused(buf, stride, n, w, h, block, types, mv, fg, bg):
    """svc_hip_dct_pack_levels_frames -> (stream cut to its bytes, offsets)."""
    out = torch.empty(nat.levels_max_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_levels_workspace_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg,
                                                        ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                                                        nat._stream()))
    return out[:int(offs[-1])], offs


def _delta(buf, stride, n, w, h, block, types, mv, fg, bg, prev_bgr=None, prev_types=None, key=None):
    """The call under test -> (the whole output buffer, pre-filled with FILL, and the offsets, pre-filled with -1)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_delta_workspace_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    k = None if key is None else torch.tensor(key, dtype=torch.int32, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_frames(
        buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg,
        None if prev_bgr is None else prev_bgr.data_ptr(), None if prev_types is None else prev_types.data_ptr(),
        None if k is None else k.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), nat._stream()))
    return out, offs


def _check_case(block, w, h, n, mv, fg, bg, content, types_kind, key=None, extra=0, seed=1):
    """-> (the delta stream's bytes as numpy, its offsets as a list, the fused pack's stream and offsets on the device)."""
    bgr = _content(content, n, w, h, seed)
    types = _types(types_kind, n, w, h, mv, seed)
    buf, stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
    plain, plain_offs = _fused(buf, stride, n, w, h, block, types, mv, fg, bg)
    want, want_offs, st = nat.delta_levels_frames(plain, plain_offs, w, h, block, mv, key=key)
    got, got_offs = _delta(buf, stride, n, w, h, block, types, mv, fg, bg, key=key)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist()  # all n + 1 of them
    used = offs[-1]
    g = got.cpu().numpy()
    assert g[:used].tobytes() == want[:used].cpu().numpy().tobytes()
    assert (g[used:] == FILL).all()  # nothing is written past the stream
    # the numpy statement on the fused pack's frames: independent of the device's delta kernel
    ref, ref_offs = layers.delta_frames(plain.cpu().numpy(), plain_offs.cpu().numpy().astype(np.uint64), keys=key)
    assert offs == [int(o) for o in ref_offs] and g[:used].tobytes() == bytes(ref)
    # and back: the undelta call gives the fused pack's stream
    back, back_offs, st = nat.undelta_levels_frames(got[:used], got_offs, w, h, block, mv, key=key)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    assert torch.equal(back_offs, plain_offs) and torch.equal(back[:plain.numel()], plain)
    return g[:used], offs, plain, plain_offs


def _level_counts(g, offs):
    return [int(g[offs[f]:offs[f] + 64].view(np.uint32)[10]) for f in range(len(offs) - 1)]


def _min_frame(w, h, block, mv):
    levels_off = 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // block) * (h // block) * (block * block // 64)
    return (levels_off + 15) // 16 * 16


SHAPES = [
    # block, w, h, mv
    (8, 16, 8, (16, 8)),      # one segment column: 7/8 of the only wave idle
    (8, 48, 16, MV16),        # 3 MV blocks: the masks are only 4-byte aligned
    (8, 272, 24, (16, 8)),    # 17 segment columns: a full wave + a one-column wave per row
    (8, 64, 32, (32, 16)),
    (16, 16, 16, MV16),
    (16, 48, 32, MV16),
    (16, 144, 48, MV16),      # 9 tiles per row: two full waves + a one-column wave
]
COUNTS = [(6, [1, 0, 0, 1, 0, 0]), (6, None), (11, None), (1, None)]
CONTENTS = ["random", "synth", "equal", "white-zero"]
TYPES = [("random", 1, 640), ("zero", 1, 640), ("checker", 1, 640), ("checker", 3, 3)]


@pytest.mark.parametrize("count", COUNTS, ids=lambda c: f"n{c[0]}-{'keys' if c[1] else 'nokeys'}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}-mv{s[3][0]}x{s[3][1]}")
def test_delta_from_pixels_equals_the_two_calls(native, shape, count):
    block, w, h, mv = shape
    n, key = count
    is_key = [i == 0 or bool(key and key[i]) for i in range(n)]
    for content in CONTENTS:
        for types_kind, fg, bg in TYPES:
            g, offs, plain, _ = _check_case(block, w, h, n, mv, fg, bg, content, types_kind, key=key, seed=w + h + n + block)
            counts = _level_counts(g, offs)
            every_tile_predicted = types_kind == "zero" or fg == bg
            if content == "equal" and every_tile_predicted:  # nothing differs: no level, every frame but the key frames at its minimum size
                for f in range(n):
                    if not is_key[f]:
                        assert counts[f] == 0 and offs[f + 1] - offs[f] == _min_frame(w, h, block, mv)
            if types_kind == "checker" and fg != bg:  # no tile of any frame is predicted: the delta stream is the plain stream
                assert g.tobytes() == plain.cpu().numpy().tobytes()
            if content == "white-zero" and every_tile_predicted and n > 1 and not key:  # each frame but the first: a DC per tile, +- the first's
                assert counts[1:] == [counts[0]] * (n - 1) and counts[0] == 3 * (w // block) * (h // block)


@pytest.mark.parametrize("block,w,h,mv,extra", [(8, 272, 24, (16, 8), 48), (16, 144, 48, MV16, 48)])
def test_frames_strided_by_noise(native, block, w, h, mv, extra):
    _check_case(block, w, h, 6, mv, 1, 640, "random", "random", key=[1, 0, 0, 1, 0, 0], extra=extra, seed=3)
    _check_case(block, w, h, 11, mv, 3, 3, "synth", "checker", extra=extra, seed=4)


@pytest.mark.parametrize("block", [8, 16])
def test_a_1080p_pair(native, block):
    g, offs, _, _ = _check_case(block, 1920, 1088, 2, MV16, 1, 640, "synth", "random", seed=block)
    assert _level_counts(g, offs)[1] > 0


@pytest.mark.parametrize("key", [[1, 0, 0, 1, 0, 0], None], ids=["keys", "nokeys"])
@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_a_call_cut_in_two_at_any_frame_gives_the_bytes_of_one(native, block, w, h, mv, key):
    n = 6
    for content, types_kind, fg, bg in (("synth", "random", 1, 640), ("random", "checker", 3, 3)):
        bgr = _content(content, n, w, h, 7)
        types = _types(types_kind, n, w, h, mv, 7)
        one, one_offs = _delta(bgr, w * h * 3, n, w, h, block, types, mv, fg, bg, key=key)
        torch.cuda.synchronize()
        used = int(one_offs[-1])
        whole = one[:used].cpu().numpy().tobytes()
        for cut in range(1, n):
            a, a_offs = _delta(bgr[:cut], w * h * 3, cut, w, h, block, types[:cut], mv, fg, bg, key=key[:cut] if key else None)
            b, b_offs = _delta(bgr[cut:], w * h * 3, n - cut, w, h, block, types[cut:], mv, fg, bg, prev_bgr=bgr[cut - 1],
                               prev_types=types[cut - 1], key=key[cut:] if key else None)
            torch.cuda.synchronize()
            ua, ub = int(a_offs[-1]), int(b_offs[-1])
            assert a[:ua].cpu().numpy().tobytes() + b[:ub].cpu().numpy().tobytes() == whole, cut
            assert a_offs.cpu().tolist() + [ua + o for o in b_offs.cpu().tolist()[1:]] == one_offs.cpu().tolist(), cut
        # the same through the frame in front given as a buffer of its own, and against the two device calls with d_prev
        cut = 2
        plain, plain_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, fg, bg)
        po = plain_offs.cpu().tolist()
        want, want_offs, st = nat.delta_levels_frames(plain[po[cut]:], plain_offs[cut:] - po[cut], w, h, block, mv,
                                                      prev=plain[po[cut - 1]:po[cut]].clone(), key=key[cut:] if key else None)
        got, got_offs = _delta(bgr[cut:], w * h * 3, n - cut, w, h, block, types[cut:], mv, fg, bg, prev_bgr=bgr[cut - 1].clone(),
                               prev_types=types[cut - 1].clone(), key=key[cut:] if key else None)
        torch.cuda.synchronize()
        assert torch.equal(got_offs, want_offs) and torch.equal(got[:int(got_offs[-1])], want[:int(want_offs[-1])])


@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_the_delta_decoder_reconstructs_what_the_plain_decoder_does(native, block, w, h, mv):
    n, key = 6, [1, 0, 0, 1, 0, 0]
    bgr = _content("synth", n, w, h, 11)
    types = _types("random", n, w, h, mv, 11)
    plain, plain_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, 1, 640)
    out, offs = nat.dct_pack_delta_frames(bgr, block, types, mv, 1, 640, key=key)
    rec, _, st, _, _ = nat.decode_delta_levels_frames(out[:int(offs[-1])], offs, w, h, block, mv, 1, 640, key=key)
    want = nat.decode_levels_frames(plain, plain_offs, w, h, block, mv, 1, 640)
    want_rec = want[0]
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    assert torch.equal(rec.view(torch.int32), want_rec.view(torch.int32))


def test_refusals_reach_python(native):
    def frames(w, h, n=1):
        return torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    big = dict(out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"), workspace=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="8x8, 16x16"):
        nat.dct_pack_delta_frames(frames(64, 64), 4, _types("zero", 1, 64, 64, MV16, 0), 16, 1, 640, **big)
    with pytest.raises(nat.SvcError, match="multiple of 16"):
        nat.dct_pack_delta_frames(frames(72, 64), 8, _types("zero", 1, 72, 64, (8, 8), 0), 8, 1, 640, **big)
    with pytest.raises(nat.SvcError, match="steps must be positive"):
        nat.dct_pack_delta_frames(frames(64, 64), 8, _types("zero", 1, 64, 64, MV16, 0), 16, 0, 640)
    types = _types("zero", 2, 64, 64, MV16, 0)
    with pytest.raises(nat.SvcError, match="together"):
        nat.dct_pack_delta_frames(frames(64, 64), 8, types[:1], 16, 1, 640, prev_bgr=frames(64, 64)[0])
    with pytest.raises(nat.SvcError, match="together"):
        nat.dct_pack_delta_frames(frames(64, 64), 8, types[:1], 16, 1, 640, prev_types=types[1])
    flat = torch.zeros(64 * 64 * 3 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(nat.SvcError, match="aligned"):
        nat.dct_pack_delta_frames(frames(64, 64), 8, types[:1], 16, 1, 640, prev_bgr=flat[8:8 + 64 * 64 * 3].view(64, 64, 3), prev_types=types[1])
