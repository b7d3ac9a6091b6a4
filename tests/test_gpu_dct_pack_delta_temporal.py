"""svc_hip_dct_pack_delta_temporal_frames (csrc/dct_pack.hip, include/svc_hip_temporal.h): the temporal-layer delta stream straight
from the pixels is, byte for byte, what svc_hip_dct_pack_levels_frames followed by svc_hip_delta_levels_temporal_frames leave on the same
device, and what layers.delta_temporal_frames (numpy, independent of the device's delta kernels) makes of the fused pack's frames.

Geometries: the two of tests/test_gpu_guard_dct_pack_delta.py plus 48 x 16 at 8 x 8, whose only wave of a tile row holds three of eight
columns.  Frame counts 1, 3, 4, 5, 8, 9, 11 and 17: the kernel's run of 8 ends inside the call, a second and a third run begin, and the
tail is shorter than a period.  Key flags: none, one frame at each layer position (i % 4 = 0 .. 3; position 0 is frame 8, a run's first
frame, where the call has that many), and all.  Every case is built with one frame more than the call takes: with `prev` that frame is
the input frame at index -period, without it frame 0 is a key frame.

Per case: offsets and bytes against the two device calls and against the numpy statement, nothing written past offsets[n], the call cut
in two at every multiple of the period, the thinning identity at 2 and 4, and the undelta call back to the fused plain stream."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack_delta import FILL, MV16, _fused, _strided, _types

pytestmark = pytest.mark.gpu

GEOMS = [(8, 272, 24, (16, 8)), (16, 144, 48, MV16), (8, 48, 16, MV16)]
PERIODS = (2, 4)
COUNTS = (1, 3, 4, 5, 8, 9, 11, 17)
CONTENTS = ("random", "equal", "white-zero")
TYPES = (("random", 1, 640), ("zero", 1, 640), ("checker", 1, 640), ("checker", 3, 3))
KEYS = ("none", 0, 1, 2, 3, "all")


def _gid(g):
    return f"{g[0]}-{g[1]}x{g[2]}-mv{g[3][0]}x{g[3][1]}"


def _content(kind, n, w, h, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "equal":
        return torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, device="cuda", generator=g).expand(n, h, w, 3).contiguous()
    if kind in ("white-zero", "zero-white"):  # DC differences of both signs; zero-white: the call's even frames (the clip's odd ones) white
        out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
        out[(0 if kind == "white-zero" else 1)::2] = 255
        return out
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)


def key_flags(kind, n):
    """None; every frame; or the one frame at layer position `kind`: the last of 8 + kind, 4 + kind, kind that the call holds."""
    if kind == "none":
        return None
    if kind == "all":
        return [1] * n
    at = next((f for f in (8 + kind, 4 + kind, kind) if f < n), None)
    return [int(i == at) for i in range(n)]


def temporal(buf, stride, n, w, h, block, types, mv, fg, bg, period, prev_bgr=None, prev_types=None, key=None):
    """The call under test -> (the whole output buffer, pre-filled with FILL, and the offsets, pre-filled with -1)."""
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_delta_temporal_workspace_bytes(n, w, h, block, mv, period), dtype=torch.uint8, device="cuda")
    k = None if key is None else torch.tensor(key, dtype=torch.int32, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_delta_temporal_frames(
        buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg,
        None if prev_bgr is None else prev_bgr.data_ptr(), None if prev_types is None else prev_types.data_ptr(),
        None if k is None else k.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), nat._stream(), period))
    return out, offs


def _used(out, offs):
    o = offs.cpu().tolist()
    return out[:o[-1]].cpu().numpy().tobytes(), o


class Clip:
    """n + 1 frames and their region ids; frame 0 is the frame in front of the call's n.  The fused plain stream is made once."""

    def __init__(self, geom, n, content, types_kind, fg, bg, seed, extra=0):
        self.block, self.w, self.h, self.mv = geom
        self.n, self.fg, self.bg = n, fg, bg
        self.bgr = _content(content, n + 1, self.w, self.h, seed)
        self.types = _types(types_kind, n + 1, self.w, self.h, self.mv, seed)
        self.buf, self.stride = _strided(self.bgr, extra) if extra else (self.bgr.view(-1), self.w * self.h * 3)
        plain, offs = _fused(self.buf, self.stride, n + 1, self.w, self.h, self.block, self.types, self.mv, fg, bg)
        o = offs.cpu().tolist()
        self.prev_plain = plain[:o[1]].clone()
        self.plain, self.plain_offs = plain[o[1]:].clone(), (offs[1:] - o[1]).contiguous()

    def call(self, period, first=0, count=None, has_prev=True, key=None, every=1, prev_at=None):
        """Frames first, first + every, .. (count of them) of the call's n through the call under test; with has_prev the frame in front
        is frame first - period * every of the call's (frame -period of the thinned clip), or the clip's frame prev_at."""
        count = self.n - first if count is None else count
        at = 1 + first  # the clip's index of the call's frame 0
        sel = [at + i * every for i in range(count)]
        if every == 1:
            buf, stride, types = self.buf[at * self.stride:], self.stride, self.types[at:at + count].contiguous()
        else:
            buf, stride, types = self.bgr[sel].contiguous(), self.w * self.h * 3, self.types[sel].contiguous()
        pb = pt = None
        if has_prev:
            p = at - period * every if prev_at is None else prev_at
            assert p >= 0
            pb, pt = self.bgr[p].clone(), self.types[p].clone()
        return temporal(buf, stride, count, self.w, self.h, self.block, types, self.mv, self.fg, self.bg, period, pb, pt, key)


def check_case(geom, period, n, content, types_kind, fg, bg, key_kind, has_prev, seed, extra=0):
    c = Clip(geom, n, content, types_kind, fg, bg, seed, extra)
    key = key_flags(key_kind, n)
    w, h, block, mv = c.w, c.h, c.block, c.mv
    what = (_gid(geom), period, n, content, types_kind, fg, bg, key_kind, has_prev)
    got, got_offs = c.call(period, has_prev=has_prev, key=key, prev_at=0)  # the clip's frame 0 stands for input frame -period
    prev = c.prev_plain if has_prev else None
    want, want_offs, st = nat.delta_levels_temporal_frames(c.plain, c.plain_offs, w, h, block, mv, period, prev=prev, key=key)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n, what
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist(), what  # all n + 1 of them
    used = offs[-1]
    g = got.cpu().numpy()
    assert g[:used].tobytes() == want[:used].cpu().numpy().tobytes(), what
    assert (g[used:] == FILL).all(), what  # nothing is written past the stream
    # the numpy statement on the fused pack's frames: independent of the device's delta kernels
    ref, ref_offs = layers.delta_temporal_frames(c.plain.cpu().numpy(), c.plain_offs.cpu().numpy().astype(np.uint64), period, keys=key,
                                                 prev=None if prev is None else prev.cpu().numpy())
    assert offs == [int(o) for o in ref_offs] and g[:used].tobytes() == bytes(ref), what
    # and back: the undelta call gives the fused pack's stream
    back, back_offs, st = nat.undelta_levels_temporal_frames(got[:used], got_offs, w, h, block, mv, period, prev=prev, key=key)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n, what
    assert torch.equal(back_offs, c.plain_offs) and torch.equal(back[:c.plain.numel()], c.plain), what
    return c, key, g[:used].tobytes(), offs


def _cases(gi, pi):
    """(n, content, types, fg, bg, key, has_prev): every count with every key pattern, the other axes dealt round so that every content
    meets every row of TYPES, with and without the frame in front."""
    out = []
    for ni, n in enumerate(COUNTS):
        for ki, key in enumerate(KEYS):
            i = ni * len(KEYS) + ki + gi + 2 * pi
            out.append((n, CONTENTS[i % 3], *TYPES[(i // 3) % 4], key, bool((i // 12 + ki) % 2)))
    return out


def test_the_grid_covers_its_axes():
    for gi in range(len(GEOMS)):
        for pi in range(len(PERIODS)):
            cs = _cases(gi, pi)
            assert {(c[1], c[2], c[3], c[4]) for c in cs} == {(a, *t) for a in CONTENTS for t in TYPES}
            assert {(c[0], c[5]) for c in cs} == {(n, k) for n in COUNTS for k in KEYS}
            assert {(c[5], c[6]) for c in cs} == {(k, p) for k in KEYS for p in (False, True)}
    assert key_flags(0, 9) == [0] * 8 + [1] and key_flags(0, 8) == [0, 0, 0, 0, 1, 0, 0, 0] and key_flags(3, 3) == [0, 0, 0]
    assert key_flags(2, 17)[10] == 1 and key_flags(1, 1) == [0]


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_temporal_delta_from_pixels_equals_the_two_calls_and_the_statement(native, geom, period):
    for n, content, types_kind, fg, bg, key, has_prev in _cases(GEOMS.index(geom), PERIODS.index(period)):
        check_case(geom, period, n, content, types_kind, fg, bg, key, has_prev, seed=n + geom[1])


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_frames_strided_by_noise(native, geom, period):
    check_case(geom, period, 11, "random", "random", 1, 640, 2, True, seed=3, extra=48)
    check_case(geom, period, 17, "random", "checker", 3, 3, "none", False, seed=4, extra=48)


@pytest.mark.parametrize("key_kind", ["none", 0, 2, "all"])
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_a_call_cut_in_two_at_every_multiple_of_the_period_gives_the_bytes_of_one(native, geom, period, key_kind):
    n = 17
    for content, types_kind, fg, bg in (("random", "random", 1, 640), ("white-zero", "checker", 3, 3)):
        c = Clip(geom, n, content, types_kind, fg, bg, seed=7)
        key = key_flags(key_kind, n)
        whole, whole_offs = _used(*c.call(period, has_prev=False, key=key))
        for cut in range(period, n, period):
            a, a_offs = _used(*c.call(period, 0, cut, has_prev=False, key=key[:cut] if key else None))
            b, b_offs = _used(*c.call(period, cut, n - cut, has_prev=True, key=key[cut:] if key else None))  # given input frame cut - period
            assert a + b == whole, cut
            assert a_offs + [a_offs[-1] + o for o in b_offs[1:]] == whole_offs, cut


@pytest.mark.parametrize("has_prev", [False, True], ids=["noprev", "prev"])
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_every_second_and_fourth_frame_is_the_call_on_the_thinned_clip(native, geom, period, has_prev):
    """layers.thin_frames of the output at 2^s <= period is the call on frames 0, 2^s, .. at period >> s, the frame in front the same
    input frame (index -period of the clip, -(period >> s) of the thinned one)."""
    for n, key_kind, content, types_kind, fg, bg in ((17, 2, "random", "random", 1, 640), (11, "none", "white-zero", "checker", 3, 3),
                                                     (9, 0, "equal", "zero", 1, 640)):
        # `period` frames in front of the call, so that input frame -period exists: the clip's first period - 1 frames are not the call's
        c = Clip(geom, n + period - 1, content, types_kind, fg, bg, seed=5 + n)
        key = key_flags(key_kind, n)
        out, offs = c.call(period, period - 1, n, has_prev=has_prev, key=key)
        got, o = _used(out, offs)
        for every in (2, 4):
            if every > period:
                continue
            thin, thin_offs, thin_keys = layers.thin_frames(np.frombuffer(got, np.uint8), np.asarray(o, np.uint64), key, every)
            m = (n + every - 1) // every
            sub, sub_offs = _used(*c.call(period // every, period - 1, m, has_prev=has_prev,
                                          key=None if key is None else [int(k) for k in thin_keys], every=every))
            assert sub_offs == [int(v) for v in thin_offs] and sub == bytes(thin), (n, every)


@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("geom", GEOMS[:2], ids=_gid)
def test_the_temporal_delta_decoder_plays_what_the_plain_decoder_does(native, geom, period):
    block, w, h, mv = geom
    n = 11
    key = key_flags(1, n)
    c = Clip(geom, n, "random", "random", 1, 640, seed=11)
    out, offs = nat.dct_pack_delta_temporal_frames(c.bgr[1:].contiguous(), block, c.types[1:].contiguous(), mv, 1, 640, period, key=key)
    rec, _, st, _, _ = nat.decode_delta_levels_temporal_frames(out[:int(offs[-1])], offs, w, h, block, mv, period, 1, 640, key=key)
    want_rec = nat.decode_levels_frames(c.plain, c.plain_offs, w, h, block, mv, 1, 640)[0]
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    assert torch.equal(rec.view(torch.int32), want_rec.view(torch.int32))


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_period_1_is_the_delta_call(native, geom):
    block, w, h, mv = geom
    for n, key_kind, has_prev in ((11, 1, True), (17, "none", False), (1, "none", True)):
        c = Clip(geom, n, "random", "random", 1, 640, seed=13 + n)
        key = key_flags(key_kind, n)
        got, offs = _used(*c.call(1, has_prev=has_prev, key=key))
        pb, pt = (c.bgr[0].clone(), c.types[0].clone()) if has_prev else (None, None)
        want, want_offs = nat.dct_pack_delta_frames(c.bgr[1:].contiguous(), block, c.types[1:].contiguous(), mv, 1, 640, pb, pt, key)
        assert (got, offs) == _used(want, want_offs)


def test_refusals_reach_python(native):
    bgr = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    types = _types("zero", 2, 64, 64, MV16, 0)
    for period in (0, 3, 8):
        with pytest.raises(nat.SvcError, match="period") as e:
            nat.dct_pack_delta_temporal_frames(bgr, 8, types, 16, 1, 640, period, out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                                               workspace=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
        assert e.value.status == nat.SVC_ERR_INVALID_ARG
        assert nat.dct_pack_delta_temporal_workspace_bytes(2, 64, 64, 8, 16, period) == 0
    with pytest.raises(nat.SvcError, match="together"):
        nat.dct_pack_delta_temporal_frames(bgr, 8, types, 16, 1, 640, 2, prev_bgr=bgr[0].clone())
