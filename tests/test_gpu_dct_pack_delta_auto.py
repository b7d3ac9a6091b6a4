"""svc_hip_dct_pack_delta_auto_frames (csrc/dct_pack.hip): the delta stream from pixels with its key frames chosen by size.  The flags
and the counts it returns are the numpy statement (layers.delta_level_counts, layers.auto_keys) of the stream
svc_hip_dct_pack_levels_frames writes from the same frames; its stream and offsets are svc_hip_dct_pack_delta_frames' with those flags.

Shapes are those of tests/test_gpu_dct_pack_delta.py with more than one wave, a partly idle wave or 4-byte aligned masks; with the frame
counts a call holds a single frame, less than a run of 8 (6), a run and one frame (9), a run and a part (11) and two runs and one
frame (17).  The "mixed" clip holds, in every six frames, a frame equal to the
one before (a difference of no level), white then zero (a frame of no level: a key frame), zero after zero (a tie: a key frame), and
random and synthetic frames; that both outcomes occur at frames nobody forced is asserted from the numpy result before the device's
is looked at."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack_delta import FILL, MV16, _content, _delta, _fused, _strided, _types

pytestmark = pytest.mark.gpu

EQUAL, ZERO_AFTER_WHITE, ZERO_AFTER_ZERO = 1, 3, 4  # places in a group of six frames of the mixed clip


def _mixed(n, w, h, seed):
    """Frame i by i % 6: 0 a random frame, 1 the same again, 2 white, 3 zero, 4 zero, 5 a synthetic frame."""
    rnd, syn = _content("random", n, w, h, seed), _content("synth", n, w, h, seed)
    out = torch.zeros_like(rnd)
    for i in range(n):
        if i % 6 in (0, 1):
            out[i] = rnd[i - i % 6]
        elif i % 6 == 2:
            out[i] = 255
        elif i % 6 == 5:
            out[i] = syn[i]
    return out


def _frames(content, n, w, h, seed):
    return _mixed(n, w, h, seed) if content == "mixed" else _content(content, n, w, h, seed)


def _forced(kind, n, seed, free=EQUAL):
    """-> d_forced as a list, or None; `free`: a frame that "some" leaves alone."""
    if kind == "none":
        return None
    if kind == "all":
        return [1] * n
    rng = np.random.default_rng(seed)
    f = (rng.random(n) < 0.25).astype(np.int64) * rng.integers(1, 1 << 31, n)  # any value but 0 forces
    if 0 <= free < n:
        f[free] = 0  # (the frame whose difference holds nothing stays free)
    return f.tolist()


def _auto(buf, stride, n, w, h, block, types, mv, fg, bg, prev_bgr=None, prev_types=None, forced=None, want_counts=True):
    """The call under test -> (the whole output buffer, pre-filled with FILL, the offsets, flags and counts, pre-filled with -1)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    keys = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(nat.dct_pack_delta_auto_workspace_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    k = None if forced is None else torch.tensor(forced, dtype=torch.int32, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_auto_frames(
        buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg,
        None if prev_bgr is None else prev_bgr.data_ptr(), None if prev_types is None else prev_types.data_ptr(),
        None if k is None else k.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), keys.data_ptr(),
        counts.data_ptr() if want_counts else None, nat._stream()))
    return out, offs, keys, counts


def _statement(bgr_all, types_all, w, h, block, mv, fg, bg, with_prev, forced):
    """The numpy statement of the fused plain stream of all frames (the first of them the frame in front of the call, with_prev) ->
    (keys as a 0 / 1 list, counts as a list of pairs)."""
    total = bgr_all.shape[0]
    plain, plain_offs = _fused(bgr_all, w * h * 3, total, w, h, block, types_all, mv, fg, bg)
    torch.cuda.synchronize()
    stream, offs = plain.cpu().numpy(), plain_offs.cpu().numpy().astype(np.int64)
    prev = None
    if with_prev:
        prev, stream, offs = stream[:offs[1]], stream[offs[1]:], offs[1:] - offs[1]
    counts = layers.delta_level_counts(stream, offs.astype(np.uint64), prev=prev)
    keys = layers.auto_keys(counts, forced, has_prev=with_prev)
    return keys.astype(np.int64).tolist(), counts.astype(np.int64).tolist()


def _check_case(block, w, h, n, mv, fg, bg, content, types_kind, forced_kind="none", with_prev=False, extra=0, seed=1, want_counts=True):
    """-> (keys, counts) of the numpy statement, after the device's were found equal to them and its stream equal to the delta call's,
    and the flags that were forced."""
    total = n + 1 if with_prev else n
    bgr_all, types_all = _frames(content, total, w, h, seed), _types(types_kind, total, w, h, mv, seed)
    forced = _forced(forced_kind, n, seed, free=EQUAL - (1 if with_prev else 0))
    keys, counts = _statement(bgr_all, types_all, w, h, block, mv, fg, bg, with_prev, forced)
    every_tile_predicted = types_kind == "zero" or fg == bg
    if content == "mixed" and every_tile_predicted:  # both outcomes, and the ties, at frames nobody forced -- before the device is asked
        f0 = 1 if with_prev else 0  # the frame in front of the call is frame 0 of the clip
        place = lambda i: i - f0  # noqa: E731
        if total > EQUAL:
            assert counts[place(EQUAL)][1] == 0 < counts[place(EQUAL)][0]
            assert keys[place(EQUAL)] == (1 if forced_kind == "all" else 0)
        if total > ZERO_AFTER_ZERO:
            assert counts[place(ZERO_AFTER_WHITE)][0] == 0 < counts[place(ZERO_AFTER_WHITE)][1] and keys[place(ZERO_AFTER_WHITE)] == 1
            assert counts[place(ZERO_AFTER_ZERO)] == [0, 0] and keys[place(ZERO_AFTER_ZERO)] == 1
    bgr, types = (bgr_all[1:], types_all[1:]) if with_prev else (bgr_all, types_all)
    prev_bgr, prev_types = (bgr_all[0].clone(), types_all[0].clone()) if with_prev else (None, None)
    buf, stride = _strided(bgr.contiguous(), extra) if extra else (bgr.contiguous(), w * h * 3)
    types = types.contiguous()
    got, got_offs, got_keys, got_counts = _auto(buf, stride, n, w, h, block, types, mv, fg, bg, prev_bgr, prev_types, forced, want_counts)
    want, want_offs = _delta(buf, stride, n, w, h, block, types, mv, fg, bg, prev_bgr, prev_types, key=keys)
    torch.cuda.synchronize()
    assert got_keys.cpu().tolist() == keys
    assert got_counts.cpu().tolist() == (counts if want_counts else [[-1, -1]] * n)
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist()  # all n + 1 of them
    used = offs[-1]
    g = got.cpu().numpy()
    assert g[:used].tobytes() == want[:used].cpu().numpy().tobytes()
    assert (g[used:] == FILL).all()  # nothing is written past the stream
    # each frame holds the smaller count, a forced frame its own
    for f in range(n):
        assert int(g[offs[f]:offs[f] + 64].view(np.uint32)[10]) == counts[f][0 if keys[f] else 1]
    return keys, counts, forced or [0] * n


SHAPES = [
    # block, w, h, mv
    (8, 48, 16, MV16),        # 3 MV blocks: the masks are only 4-byte aligned
    (8, 272, 24, (16, 8)),    # 17 segment columns: a full wave + a one-column wave per row
    (8, 64, 32, (32, 16)),
    (16, 48, 32, MV16),
    (16, 144, 48, MV16),      # 9 tiles per row: two full waves + a one-column wave
]
COUNTS = [1, 6, 9, 11, 17]
CONTENTS = ["mixed", "random", "synth"]
TYPES = [("random", 1, 640), ("zero", 1, 640), ("checker", 1, 640), ("checker", 3, 3)]
FORCED = ["none", "some", "all"]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}-mv{s[3][0]}x{s[3][1]}")
def test_keys_counts_and_stream(native, shape, n):
    """Every content and every (region ids, steps) at this shape and frame count; d_forced null / given / all ones and a frame in front
    of the call or none go round with them, so that every shape and count meets each of them with every content."""
    block, w, h, mv = shape
    turn = SHAPES.index(shape) + COUNTS.index(n)
    free_keys = free_diffs = 0
    for content in CONTENTS:
        for types_kind, fg, bg in TYPES:
            forced_kind, with_prev = FORCED[turn % 3], turn % 2 == 1
            turn += 1
            keys, counts, forced = _check_case(block, w, h, n, mv, fg, bg, content, types_kind, forced_kind, with_prev, seed=w + h + n + block)
            for f in range(0 if with_prev else 1, n):  # the frames the rule alone decided
                if not forced[f]:
                    free_keys += keys[f]
                    free_diffs += 1 - keys[f]
    if n >= 6:
        assert free_keys > 0 and free_diffs > 0


@pytest.mark.parametrize("block,w,h,mv,extra", [(8, 272, 24, (16, 8), 48), (16, 144, 48, MV16, 48)])
def test_frames_strided_by_noise(native, block, w, h, mv, extra):
    _check_case(block, w, h, 9, mv, 1, 640, "mixed", "zero", "some", with_prev=True, extra=extra, seed=3)
    _check_case(block, w, h, 11, mv, 3, 3, "mixed", "checker", "none", extra=extra, seed=4)


@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_the_counts_may_be_left_out(native, block, w, h, mv):
    _check_case(block, w, h, 6, mv, 3, 3, "mixed", "random", "none", want_counts=False, seed=5)


@pytest.mark.parametrize("block", [8, 16])
def test_a_1080p_pair(native, block):
    """The second frame is the first with its upper half redrawn: its difference is smaller, and the counts are those of 24 480 tiles."""
    w, h, n = 1920, 1088, 2
    bgr = _content("synth", 1, w, h, block).expand(n, h, w, 3).contiguous()
    bgr[1, :h // 2] = torch.randint(0, 256, (h // 2, w, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    types = _types("random", 1, w, h, MV16, block).expand(n, -1).contiguous()  # (no tile changes its class)
    keys, counts = _statement(bgr, types, w, h, block, MV16, 1, 640, False, None)
    assert keys == [1, 0] and 0 < counts[1][1] < counts[1][0]
    got, got_offs, got_keys, got_counts = _auto(bgr, w * h * 3, n, w, h, block, types, MV16, 1, 640)
    want, want_offs = _delta(bgr, w * h * 3, n, w, h, block, types, MV16, 1, 640, key=keys)
    torch.cuda.synchronize()
    assert got_keys.cpu().tolist() == keys and got_counts.cpu().tolist() == counts
    assert torch.equal(got_offs, want_offs)
    used = int(got_offs[-1])
    assert torch.equal(got[:used], want[:used]) and bool((got[used:] == FILL).all())


@pytest.mark.parametrize("forced_kind", ["none", "some"])
@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_a_call_cut_in_two_at_any_frame_gives_the_bytes_keys_and_counts_of_one(native, block, w, h, mv, forced_kind):
    n = 11  # cuts in front of, on and behind the end of the first run of 8
    forced = _forced(forced_kind, n, 7)
    for content, types_kind, fg, bg in (("mixed", "random", 1, 640), ("mixed", "checker", 3, 3)):
        bgr, types = _frames(content, n, w, h, 7), _types(types_kind, n, w, h, mv, 7)
        one, one_offs, one_keys, one_counts = _auto(bgr, w * h * 3, n, w, h, block, types, mv, fg, bg, forced=forced)
        torch.cuda.synchronize()
        whole = one[:int(one_offs[-1])].cpu().numpy().tobytes()
        for cut in range(1, n):
            a = _auto(bgr[:cut], w * h * 3, cut, w, h, block, types[:cut], mv, fg, bg, forced=forced[:cut] if forced else None)
            b = _auto(bgr[cut:], w * h * 3, n - cut, w, h, block, types[cut:], mv, fg, bg, prev_bgr=bgr[cut - 1], prev_types=types[cut - 1],
                      forced=forced[cut:] if forced else None)
            torch.cuda.synchronize()
            ua, ub = int(a[1][-1]), int(b[1][-1])
            assert a[0][:ua].cpu().numpy().tobytes() + b[0][:ub].cpu().numpy().tobytes() == whole, cut
            assert a[1].cpu().tolist() + [ua + o for o in b[1].cpu().tolist()[1:]] == one_offs.cpu().tolist(), cut
            assert a[2].cpu().tolist() + b[2].cpu().tolist() == one_keys.cpu().tolist(), cut
            assert a[3].cpu().tolist() + b[3].cpu().tolist() == one_counts.cpu().tolist(), cut


@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_the_delta_decoder_reconstructs_what_the_plain_decoder_does(native, block, w, h, mv):
    n = 9
    bgr, types = _frames("mixed", n, w, h, 11), _types("zero", n, w, h, mv, 11)
    plain, plain_offs = _fused(bgr, w * h * 3, n, w, h, block, types, mv, 1, 640)
    out, offs, keys, _ = nat.dct_pack_delta_auto_frames(bgr, block, types, mv, 1, 640)
    torch.cuda.synchronize()
    flags = keys.cpu().tolist()
    assert flags[0] == 1 and 0 in flags and 1 in flags[1:]
    rec, _, st, _, _ = nat.decode_delta_levels_frames(out[:int(offs[-1])], offs, w, h, block, mv, 1, 640, key=flags)
    want_rec = nat.decode_levels_frames(plain, plain_offs, w, h, block, mv, 1, 640)[0]
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    assert torch.equal(rec.view(torch.int32), want_rec.view(torch.int32))
    # and the undelta call gives the plain stream back, byte for byte
    back, back_offs, st = nat.undelta_levels_frames(out[:int(offs[-1])], offs, w, h, block, mv, key=flags)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n and torch.equal(back_offs, plain_offs) and torch.equal(back[:plain.numel()], plain)


def test_refusals_reach_python(native):
    def frames(w, h, n=1):
        return torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    big = dict(out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"), workspace=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(nat.SvcError, match="8x8, 16x16"):
        nat.dct_pack_delta_auto_frames(frames(64, 64), 4, _types("zero", 1, 64, 64, MV16, 0), 16, 1, 640, **big)
    with pytest.raises(nat.SvcError, match="steps must be positive"):
        nat.dct_pack_delta_auto_frames(frames(64, 64), 8, _types("zero", 1, 64, 64, MV16, 0), 16, 0, 640)
    types = _types("zero", 2, 64, 64, MV16, 0)
    with pytest.raises(nat.SvcError, match="together"):
        nat.dct_pack_delta_auto_frames(frames(64, 64), 8, types[:1], 16, 1, 640, prev_bgr=frames(64, 64)[0])
    with pytest.raises(nat.SvcError, match="workspace"):
        nat.dct_pack_delta_auto_frames(frames(64, 64), 8, types[:1], 16, 1, 640,
                                       workspace=torch.empty(nat.dct_pack_delta_workspace_bytes(1, 64, 64, 8, 16), dtype=torch.uint8, device="cuda"))
