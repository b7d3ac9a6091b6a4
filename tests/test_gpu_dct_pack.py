"""svc_hip_dct_pack_levels_frames (csrc/dct_pack.hip): the compact stream straight from the transform kernel is, byte for byte,
what svc_hip_dct_quant_frames followed by svc_hip_pack_levels_frames leave on the same device -- a route that is itself pinned to
the oracle (tests/test_gpu_transform_exact.py) and to the numpy writer (tests/test_gpu_levels.py).  Shapes are the smallest at which
each mechanism of the fused kernels can break: a wave that is 7/8 idle, a mask section that is only 4-byte aligned, a one-column wave
behind a full one, more than one workgroup per frame, and one full 1080p frame per tile size."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from scalable_video_codec_amd import synth

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _content(kind, n, w, h, seed):
    if kind == "zero":
        return torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    if kind == "white":
        return torch.full((n, h, w, 3), 255, dtype=torch.uint8, device="cuda")
    if kind == "synth":
        clip = synth.SynthClip(w, h, n, seed, device="cuda")
        return torch.stack([clip.frame_bgr(t) for t in range(n)]).contiguous()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)


def _types(kind, n, w, h, mv, seed):
    mfw, mfh = w // mv[0], h // mv[1]
    if kind == "zero":
        t = torch.zeros((n, mfh, mfw), dtype=torch.int32)
    elif kind == "ones":
        t = torch.full((n, mfh, mfw), -1, dtype=torch.int32)  # 0xFFFFFFFF
    elif kind == "checker":
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


def _two_calls(buf, stride, n, w, h, block, types, mv, fg, bg):
    """svc_hip_dct_quant_frames, then svc_hip_pack_levels_frames -> (planes, stream pre-filled with FILL, offsets)."""
    planes = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    nat._check(nat.load().svc_hip_dct_quant_frames(buf.data_ptr(), stride, n, w, h, block, block, types.data_ptr(), mv[0], mv[1], fg, bg,
                                                  planes.data_ptr(), nat._stream()))
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    out, offs = nat.pack_levels_frames(planes, types, block, mv, fg, bg, out=out)
    return planes, out, offs


def _fused(buf, stride, n, w, h, block, types, mv, fg, bg):
    out = torch.full((nat.levels_max_bytes(n, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_levels_workspace_bytes(n, w, h, block, mv), dtype=torch.uint8, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_frames(buf.data_ptr(), stride, n, w, h, block, types.data_ptr(), mv[0], mv[1], fg, bg,
                                                        ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                                                        nat._stream()))
    return out, offs


def _check_case(block, w, h, n, mv, fg, bg, content, types_kind, extra=0, seed=1):
    bgr = _content(content, n, w, h, seed)
    types = _types(types_kind, n, w, h, mv, seed)
    buf, stride = _strided(bgr, extra) if extra else (bgr, w * h * 3)
    _, want, want_offs = _two_calls(buf, stride, n, w, h, block, types, mv, fg, bg)
    got, got_offs = _fused(buf, stride, n, w, h, block, types, mv, fg, bg)
    torch.cuda.synchronize()
    offs = got_offs.cpu().tolist()
    assert offs == want_offs.cpu().tolist()  # all n + 1 of them
    used = offs[-1]
    g = got.cpu().numpy()
    assert g[:used].tobytes() == want[:used].cpu().numpy().tobytes()
    assert (g[used:] == FILL).all()  # nothing is written past the stream
    levels_off = 64 + 4 * types.shape[1] + 8 * 3 * (w // block) * (h // block) * (block * block // 64)
    total_levels = 0
    for f in range(n):
        hdr = g[offs[f]:offs[f] + 64].view(np.uint32)
        assert hdr[11] == 0 and hdr[12] == offs[f + 1] - offs[f]  # inexact, frame_bytes
        assert not g[offs[f] + levels_off + 2 * int(hdr[10]):offs[f + 1]].any()  # the pad is zero
        total_levels += int(hdr[10])
    return used, total_levels


MV16 = (16, 16)
CASES8 = [
    # w, h, n, mv, fg, bg, content, types, bytes between frames
    (16, 8, 1, (16, 8), 1, 1, "random", "random", 0),        # one segment column: 7/8 of the only wave idle
    (16, 8, 3, (16, 8), 3, 17, "random", "ones", 0),
    (48, 16, 3, MV16, 1, 640, "random", "random", 0),        # 3 MV blocks: the masks are only 4-byte aligned
    (48, 16, 1, (48, 16), 3, 17, "white", "zero", 0),        # one MV block covering the frame; only the DCs are set
    (272, 24, 3, (16, 8), 1, 640, "random", "checker", 48),  # 17 segment columns: a full wave + a one-column wave per row, 34 tiles
    (272, 24, 1, (272, 24), 1, 1, "random", "ones", 0),
    (272, 24, 3, (16, 24), 3, 17, "zero", "random", 0),      # level_count 0: every frame at its minimum size
    (64, 32, 3, (32, 16), 3, 17, "synth", "checker", 0),
    (1920, 1088, 1, MV16, 1, 640, "synth", "random", 0),
    (1920, 1088, 1, (32, 16), 1, 1, "random", "random", 0),
]
CASES16 = [
    (16, 16, 1, MV16, 1, 1, "random", "random", 0),
    (16, 16, 3, MV16, 3, 17, "white", "ones", 0),
    (48, 32, 3, MV16, 1, 640, "random", "random", 0),
    (48, 32, 1, (48, 32), 3, 17, "random", "zero", 0),
    (144, 48, 3, MV16, 1, 640, "random", "checker", 16),     # 9 tiles per row: two full waves + a one-column wave; 27 MV blocks
    (144, 48, 3, (48, 16), 1, 1, "zero", "random", 0),
    (64, 32, 3, (32, 16), 3, 17, "synth", "checker", 0),
    (1920, 1088, 1, MV16, 1, 640, "synth", "random", 0),
    (1920, 1088, 1, (32, 16), 3, 17, "random", "ones", 0),
]


@pytest.mark.parametrize("case", CASES8, ids=lambda c: "-".join(str(x) for x in c))
def test_fused_8x8_equals_the_two_calls(native, case):
    w, h, n, mv, fg, bg, content, types, extra = case
    _check_case(8, w, h, n, mv, fg, bg, content, types, extra, seed=w + h + n)


@pytest.mark.parametrize("case", CASES16, ids=lambda c: "-".join(str(x) for x in c))
def test_fused_16x16_equals_the_two_calls(native, case):
    w, h, n, mv, fg, bg, content, types, extra = case
    _check_case(16, w, h, n, mv, fg, bg, content, types, extra, seed=w + h + n + 16)


@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (8, 8)), (16, 144, 48, MV16)])
def test_random_bytes_at_step_one_take_the_dense_path(native, block, w, h, mv):
    """Uniform random bytes at step 1 leave a level almost everywhere (the oracle's planes through the numpy writer: 99.5 % of
    svc_hip_levels_max_bytes at these shapes), so every slot is filled to near its capacity and every mask word is near all ones."""
    n = 3
    used, levels = _check_case(block, w, h, n, mv, 1, 1, "random", "ones", seed=5)
    assert used >= 0.95 * nat.levels_max_bytes(n, w, h, block, mv)
    assert levels >= 0.95 * n * 3 * w * h


@pytest.mark.parametrize("block", [8, 16])
def test_empty_and_constant_frames(native, block):
    w, h, n = 80, 48, 3
    used, levels = _check_case(block, w, h, n, MV16, 1, 640, "zero", "checker")
    levels_off = 64 + 4 * 15 + 8 * 3 * (w // block) * (h // block) * (block * block // 64)  # 15 MV blocks: masks 4-byte aligned
    assert levels == 0 and used == n * ((levels_off + 15) // 16 * 16)  # every frame at its minimum size
    _, levels = _check_case(block, w, h, n, MV16, 1, 1, "white", "zero")
    assert levels == n * 3 * (w // block) * (h // block)  # the DC of every tile, nothing else


@pytest.mark.parametrize("block", [8, 16])
def test_two_runs_give_the_same_bytes(native, block):
    w, h, n = 272, 48, 3
    bgr = _content("random", n, w, h, 9)
    types = _types("random", n, w, h, MV16, 9)
    a, a_offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17)
    b, b_offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17, out=torch.zeros_like(a))
    torch.cuda.synchronize()
    used = int(a_offs[-1])
    assert torch.equal(a_offs, b_offs) and torch.equal(a[:used], b[:used])


@pytest.mark.parametrize("block", [8, 16])
def test_the_fused_stream_feeds_the_unpack_and_the_entropy_coder(native, block):
    w, h, n = 144, 48, 3
    bgr = _content("synth", n, w, h, 3)
    bgr[1] = _content("random", 1, w, h, 4)[0]
    types = _types("random", n, w, h, MV16, 3)
    planes = nat.dct_quant_frames(bgr, block, types, 16, 3, 17)
    out, offs = nat.dct_pack_levels_frames(bgr, block, types, MV16, 3, 17)
    used = int(offs[-1])
    got, got_types, status = nat.unpack_levels_frames(out[:used], offs, w, h, block, MV16)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert torch.equal(got, planes) and torch.equal(got_types, types)  # as numbers: -0.0 comes back as +0.0
    coded, coded_offs, st = nat.entropy_encode_frames(out[:used], offs, w, h, block, MV16)
    assert st.cpu().tolist() == [0] * n
    back, back_offs, st2 = nat.entropy_decode_frames(coded[:int(coded_offs[-1])], coded_offs, w, h, block, MV16)
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [0] * n
    assert torch.equal(back_offs, offs) and torch.equal(back[:used], out[:used])


def test_refusals_reach_python(native):
    bgr = _content("zero", 1, 72, 64, 0)
    with pytest.raises(Exception, match="multiple of 16"):
        nat.dct_pack_levels_frames(bgr, 8, _types("zero", 1, 72, 64, (8, 8), 0), 8, 1, 640,
                                   out=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"),
                                   workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
