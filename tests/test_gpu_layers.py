"""The two layers of the compact stream on the device (include/svc_hip.h, "Two layers").

Encode, svc_hip_dct_pack_layers_frames: the base stream is svc_hip_dct_pack_levels_frames at (fg, bg) byte for byte, and the
enhancement stream is scalable_video_codec_amd/layers.py applied to that base and to svc_hip_dct_pack_levels_frames at (enh, enh) from
the same device.  Decode, svc_hip_decode_layers_frames: with A = svc_hip_decode_levels_frames on the base stream and B = the same call
on the fine stream, under the same gaze, d_rec has B's bits on the tiles whose origin is in gaze and window and A's everywhere else
(Lb * ratio * enh == Lb * sb exactly, and Lb * ratio + d is the fine level).  Shapes are those of tests/test_gpu_dct_pack.py."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_dct_pack import FILL, MV16, _content, _fused, _strided, _types

pytestmark = pytest.mark.gpu


def _layers(buf, stride, n, w, h, block, types, mv, fg, bg, enh, window):
    """svc_hip_dct_pack_layers_frames into buffers pre-filled with FILL -> (base, base offsets, enhancement, its offsets)."""
    cap = nat.levels_max_bytes(n, w, h, block, mv)
    base = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    enh_out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    base_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    enh_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_layers_workspace_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    win = None if window is None else torch.tensor(window, dtype=torch.int32, device="cuda").reshape(n, 4).contiguous()
    nat._check(nat.load().svc_hip_dct_pack_layers_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg, enh,
                                                        None if win is None else win.data_ptr(), ws.data_ptr(), ws.numel(),
                                                        base.data_ptr(), cap, base_offs.data_ptr(), enh_out.data_ptr(), cap,
                                                        enh_offs.data_ptr(), nat._stream()))
    return base, base_offs, enh_out, enh_offs


def _window(kind, n, w, h, block):
    """None, or n rectangles x, y, w, h.  "rect" has its edges inside tiles and, on a 272-wide frame, holds the tile origins 248, 256
    and 264: both sides of x = 256, where the second wave of a row of 8x8 tiles begins."""
    rect = (max(0, w - 27), 3 if h > block else 0, 20, max(1, h - 5))
    table = {"none": None, "empty": [(0, 0, 0, h)] * n, "whole": [(0, 0, w, h)] * n, "rect": [rect] * n,
             "per-frame": [[(0, 0, w, h), rect, (3, 0, w, h - 1), (0, 0, 0, 0)][f % 4] for f in range(n)]}
    return table[kind]


def _tiles_in(rects, n, w, h, block, default):
    """(n, h, w) bool: is the origin of the pixel's tile inside its frame's rectangle (the rule of gaze and window)?"""
    if rects is None:
        return torch.full((n, h, w), default, dtype=torch.bool)
    oy = (torch.arange(h) // block * block)[:, None]
    ox = (torch.arange(w) // block * block)[None, :]
    return torch.stack([(ox >= x) & (ox < x + ww) & (oy >= y) & (oy < y + hh) for x, y, ww, hh in rects])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Streams:
    """One encode of a case: the two layers, and the fine stream the oracle decodes."""

    def __init__(self, block, w, h, n, mv, steps, content, types_kind, window_kind, extra=0, seed=1):
        fg, bg, enh = steps
        self.block, self.w, self.h, self.n, self.mv, self.steps = block, w, h, n, mv, steps
        bgr = _content(content, n, w, h, seed)
        types = _types(types_kind, n, w, h, mv, seed)
        buf, stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
        self.window = _window(window_kind, n, w, h, block)
        self.want_base, self.want_base_offs = _fused(buf, stride, n, w, h, block, types, mv, fg, bg)
        self.fine, self.fine_offs = _fused(buf, stride, n, w, h, block, types, mv, enh, enh)
        self.base, self.base_offs, self.enh, self.enh_offs = _layers(buf, stride, n, w, h, block, types, mv, fg, bg, enh, self.window)
        torch.cuda.synchronize()

    def check_encode(self):
        n = self.n
        offs = self.base_offs.cpu().tolist()
        assert offs == self.want_base_offs.cpu().tolist()  # all n + 1 of them
        got = self.base.cpu().numpy()
        assert got[:offs[-1]].tobytes() == self.want_base[:offs[-1]].cpu().numpy().tobytes()
        assert (got[offs[-1]:] == FILL).all()  # nothing is written past the stream
        fine_offs = self.fine_offs.cpu().numpy()
        want, want_offs = layers.enhancement_frames(got[:offs[-1]], offs, self.fine.cpu().numpy()[:int(fine_offs[-1])], fine_offs,
                                                    self.steps[2], self.window)
        eoffs = self.enh_offs.cpu().tolist()
        assert eoffs == [int(o) for o in want_offs]
        egot = self.enh.cpu().numpy()
        assert egot[:eoffs[-1]].tobytes() == want
        assert (egot[eoffs[-1]:] == FILL).all()
        for f in range(n):
            hdr = egot[eoffs[f]:eoffs[f] + 64].view(np.uint32)
            assert hdr[8] == hdr[9] == self.steps[2] and hdr[11] == 0 and hdr[12] == eoffs[f + 1] - eoffs[f] and not hdr[13:].any()
        return eoffs

    def decode(self, gaze, dec=(1, 640), display=None, base=None, enh=None):
        """svc_hip_decode_layers_frames -> (rec, display, status)."""
        base = self.base if base is None else base
        enh = self.enh if enh is None else enh
        rec = torch.full((self.n, self.h, self.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        return nat.decode_layers_frames(base[:int(self.base_offs[-1])], self.base_offs, enh[:int(self.enh_offs[-1])], self.enh_offs, self.w,
                                        self.h, self.block, self.mv, dec[0], dec[1], gaze=gaze, display=display, rec=rec)

    def oracle(self, gaze, dec=(1, 640), display=None):
        """A and B: svc_hip_decode_levels_frames on the base stream and on the fine stream, with the gaze."""
        a = nat.decode_levels_frames(self.base[:int(self.base_offs[-1])], self.base_offs, self.w, self.h, self.block, self.mv, dec[0], dec[1],
                                     gaze=gaze, display=display)
        b = nat.decode_levels_frames(self.fine[:int(self.fine_offs[-1])], self.fine_offs, self.w, self.h, self.block, self.mv, dec[0], dec[1],
                                     gaze=gaze, display=display)
        return a, b

    def check_decode(self, gaze, dec=(1, 640)):
        """-> the number of tiles-pixels in gaze and window, and in the gaze alone."""
        rec, _, status = self.decode(gaze, dec)
        (a, _, sa), (b, _, sb) = self.oracle(gaze, dec)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == sa.cpu().tolist() == sb.cpu().tolist() == [0] * self.n
        gz = _tiles_in(gaze, self.n, self.w, self.h, self.block, False)
        both = gz & _tiles_in(self.window, self.n, self.w, self.h, self.block, True)
        want = torch.where(both[..., None].cuda(), b, a)
        assert _same_bits(rec, want)
        return int(both.sum()), int(gz.sum())


GAZES = ("empty", "whole", "left", "per-frame")


def _gaze(kind, n, w, h):
    return {"empty": [(5, 5, 0, 7)] * n, "whole": [(0, 0, w, h)] * n, "left": [(0, 0, max(1, w // 2 - 3), h)] * n,
            "per-frame": [[(w // 3, 1, w, h), (0, 0, 1, 1), (0, 0, w, h)][f % 3] for f in range(n)]}[kind]


def _check_case(block, case, seed):
    w, h, n, mv, steps, content, types_kind, window_kind, extra = case
    s = Streams(block, w, h, n, mv, steps, content, types_kind, window_kind, extra, seed)
    s.check_encode()
    for kind in GAZES:
        s.check_decode(_gaze(kind, n, w, h), dec=(1, 640) if kind != "left" else (2, 24))
    # no gaze: the enhancement is not read, and may be absent
    rec, _, status = nat.decode_layers_frames(s.base[:int(s.base_offs[-1])], s.base_offs, None, None, w, h, block, mv, 1, 640)
    want, _, _ = nat.decode_levels_frames(s.base[:int(s.base_offs[-1])], s.base_offs, w, h, block, mv, 1, 640)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and _same_bits(rec, want)
    return s


S1, S2, S3, S4 = (1, 640, 1), (4, 16, 2), (3, 18, 3), (16, 16, 16)
CASES8 = [
    # w, h, n, mv, (fg, bg, enh), content, types, window, bytes between frames
    (16, 8, 1, (16, 8), S1, "random", "random", "none", 0),          # one segment column: 7/8 of the only wave idle
    (16, 8, 1, (16, 8), S2, "white", "zero", "whole", 0),            # one level per tile and layer: the DCs, d = 1020 - 128 * 8
    (16, 8, 1, (16, 8), S4, "random", "ones", "rect", 0),
    (48, 16, 3, MV16, S1, "random", "random", "per-frame", 0),       # 3 MV blocks: the masks are only 4-byte aligned
    (48, 16, 3, MV16, S3, "white", "checker", "none", 0),
    (48, 16, 3, MV16, S2, "synth", "random", "empty", 0),
    (272, 24, 3, (16, 8), S1, "random", "checker", "rect", 48),      # a full wave + a one-column wave per row; the window crosses them
    (272, 24, 3, (16, 8), S2, "synth", "random", "per-frame", 48),
    (272, 24, 3, (16, 24), S3, "zero", "random", "whole", 0),        # no level in either layer
    (272, 24, 3, (8, 8), S4, "random", "random", "none", 16),        # enh_step == both steps: every enhancement frame at its minimum
    (1920, 1088, 1, MV16, S1, "synth", "random", "rect", 0),
]
CASES16 = [
    (16, 16, 1, MV16, S1, "random", "random", "none", 0),
    (16, 16, 1, MV16, S3, "white", "ones", "whole", 0),
    (48, 32, 3, MV16, S2, "random", "random", "per-frame", 0),
    (48, 32, 3, (48, 32), S1, "synth", "zero", "rect", 0),
    (48, 32, 3, MV16, S4, "random", "checker", "empty", 0),
    (144, 48, 3, MV16, S1, "random", "checker", "rect", 16),         # 9 tiles per row: two full waves + a one-column wave
    (144, 48, 3, (48, 16), S2, "synth", "random", "per-frame", 0),
    (144, 48, 3, MV16, S3, "zero", "random", "none", 0),
    (144, 48, 3, MV16, S4, "white", "ones", "whole", 16),
    (1920, 1088, 1, MV16, S1, "synth", "random", "rect", 0),
]


def _id(c):
    return "-".join(str(x) for x in c).replace(" ", "")


@pytest.mark.parametrize("case", CASES8, ids=_id)
def test_layers_8x8(native, case):
    _check_case(8, case, seed=sum(case[:3]))


@pytest.mark.parametrize("case", CASES16, ids=_id)
def test_layers_16x16(native, case):
    _check_case(16, case, seed=sum(case[:3]) + 16)


@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
def test_minimum_size_and_the_window_at_the_wave_boundary(native, block, w, h, mv):
    n = 3
    s = Streams(block, w, h, n, mv, S4, "random", "random", "none", seed=3)
    eoffs = s.check_encode()
    words = block * block // 64
    minimum = (64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // block) * (h // block) * words + 15) // 16 * 16
    assert eoffs == [f * minimum for f in range(n + 1)]  # a tile with sb == enh_step costs its mask bits only
    # gaze inside, straddling and outside the window, each checked to be that
    s = Streams(block, w, h, n, mv, S1, "random", "checker", "rect", seed=4)
    s.check_encode()
    x0, y0, ww, hh = s.window[0]
    inside = [(x0 + 1, y0 + 1, ww - 2, hh - 2)] * n
    straddling = [(x0 - 3 * block, 0, 4 * block + 3, h)] * n
    outside = [(0, 0, x0 - block, h)] * n
    both, gz = s.check_decode(inside)
    assert both == gz > 0
    both, gz = s.check_decode(straddling)
    assert 0 < both < gz
    both, gz = s.check_decode(outside)
    assert both == 0 < gz


@pytest.mark.parametrize("block,w,h", [(8, 272, 24), (16, 144, 48)])
def test_display_and_whole_frame_gaze(native, block, w, h):
    n = 3
    s = Streams(block, w, h, n, MV16 if block == 16 else (16, 8), S1, "synth", "random", "whole", seed=6)
    whole = [(0, 0, w, h)] * n
    disp = (w - 16, h - 8)
    rec, shown, status = s.decode(whole, display=disp)
    (_, _, _), (b, b_shown, _) = s.oracle(whole, display=disp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and _same_bits(rec, b) and torch.equal(shown, b_shown)
    # no gaze and no enhancement: svc_hip_decode_levels_frames on the base, display included
    rec, shown, status = nat.decode_layers_frames(s.base[:int(s.base_offs[-1])], s.base_offs, None, None, w, h, block, s.mv, 2, 24, display=disp)
    a, a_shown, _ = nat.decode_levels_frames(s.base[:int(s.base_offs[-1])], s.base_offs, w, h, block, s.mv, 2, 24, display=disp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and _same_bits(rec, a) and torch.equal(shown, a_shown)


def _patched(stream, offs, frame, word, value):
    out = stream.clone()
    out[int(offs[frame]):int(offs[frame]) + 64].view(torch.int32)[word] = value
    return out


@pytest.mark.parametrize("block,w,h", [(8, 48, 16), (16, 48, 32)])
def test_statuses(native, block, w, h):
    n = 3
    s = Streams(block, w, h, n, MV16, S2, "random", "random", "none", seed=8)
    gaze = [(0, 0, w, h), (8, 0, w, h), (0, 0, 24, h)]
    disp = (w, h)
    good, good_shown, status = s.decode(gaze, display=disp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0]
    cases = [
        ("base", 0, 0x12345678, 2),        # a base frame with a bad magic: its own code
        ("enh", 0, 0x12345678, 0x100 | 2),  # an enhancement frame with a bad magic
        ("enh", 9, 4, 0x100 | 11),         # fg_step != bg_step in the enhancement's header
        ("enh", None, 3, 0x100 | 11),      # one step, which does not divide the base's 4 and 16
    ]
    for which, word, value, code in cases:
        base, enh = s.base, s.enh
        if which == "base":
            base = _patched(base, s.base_offs, 1, word, value)
        elif word is None:
            enh = _patched(_patched(enh, s.enh_offs, 1, 8, value), s.enh_offs, 1, 9, value)
        else:
            enh = _patched(enh, s.enh_offs, 1, word, value)
        rec, shown, status = s.decode(gaze, display=disp, base=base, enh=enh)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, code, 0], (which, word)
        assert not rec[1].any() and not shown[1].any()  # the frame is zeros
        assert _same_bits(rec[0], good[0]) and _same_bits(rec[2], good[2])  # its neighbours are unchanged
        assert torch.equal(shown[0], good_shown[0]) and torch.equal(shown[2], good_shown[2])


@pytest.mark.parametrize("block,w,h", [(8, 48, 16), (16, 48, 32)])
def test_through_the_entropy_coder(native, block, w, h):
    n = 3
    s = Streams(block, w, h, n, MV16, S1, "synth", "random", "per-frame", seed=9)
    gaze = _gaze("per-frame", n, w, h)
    want, _, _ = s.decode(gaze)
    back = []
    for stream, offs in ((s.base, s.base_offs), (s.enh, s.enh_offs)):
        used = int(offs[-1])
        coded, coded_offs, st = nat.entropy_encode_frames(stream[:used], offs, w, h, block, MV16)
        assert st.cpu().tolist() == [0] * n
        out, out_offs, st2 = nat.entropy_decode_frames(coded[:int(coded_offs[-1])], coded_offs, w, h, block, MV16)
        torch.cuda.synchronize()
        assert st2.cpu().tolist() == [0] * n
        assert torch.equal(out_offs, offs) and torch.equal(out[:used], stream[:used])
        back.append(out)
    rec, _, status = s.decode(gaze, base=back[0], enh=back[1])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and _same_bits(rec, want)
