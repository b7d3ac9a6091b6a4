"""The transcode between the reference's wire records and the compact stream on the device (svc_hip_records_pack_levels_frames,
svc_hip_levels_records_frames): byte for byte the numpy statements of scalable_video_codec_amd/wire.py and the device routes
through planes (pack_levels_frames on the parsed planes; unpack_levels_frames + serialize_frames), on the smallest shapes at which
the kernels take each of their paths; and the host driver (svc::WireTranscoder, through tests/dropin/wire_transcode_main) against the
device calls."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import configs, levels, native, stream, synth, wire
from tests.helpers import guarded as gd

pytestmark = pytest.mark.gpu

BIG_ID = 0x7FFFFFF3
# (w, h, block, mv_block, emit_h).  48 x 16 with MV block 16: 3 MV blocks, the masks are only 4-byte aligned.  36 x 12 with 6 x 6 tiles: a
# part-filled mask word.  264 x 8: 33 tiles of 8 x 8 in a tile row, a group holds 32 (levels.hip: group_of, kGroupCoeffs / 64), so the row
# spans two groups, the second of one tile.  528 x 16 with 16 x 16 tiles: 8 tiles a group, 33 tiles, five groups.  32 x 32 emitted for
# 20 rows: 3 of 4 tile rows held.
SHAPES = [(32, 16, 8, 8, 16), (32, 16, 8, 16, 16), (48, 16, 8, 8, 16), (48, 16, 8, 16, 16), (64, 32, 16, 16, 32), (64, 32, 16, 32, 32),
          (36, 12, 6, 6, 12), (264, 8, 8, 8, 8), (528, 16, 16, 16, 16), (32, 32, 8, 8, 20), (32, 32, 8, 16, 20)]
DENSITIES = ("zero", "sparse", "dense", "clamp")
FG, BG = 3, 17


def _ids(shape):
    return "x".join(str(v) for v in shape)


def _coefficients(rng, shape, density, bits=False):
    """f32 coefficients.  zero: none; sparse: most of them quantise to 0 at (FG, BG); dense: every one is a non-zero level at both steps;
    clamp: dense plus values past +-32767 levels of both steps.  bits: any bit pattern -- NaN, +-Inf, -0.0, denormals among them."""
    if density == "zero":
        c = np.zeros(shape, np.float32)
    elif density == "sparse":
        c = (rng.standard_normal(shape) * 1.2).astype(np.float32)
        big = rng.random(shape) < 0.02
        c[big] = (rng.standard_normal(int(big.sum())) * 400).astype(np.float32)
    else:
        mag = rng.uniform(BG, 2000.0, shape)
        c = (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
        if density == "clamp":
            edge = np.array([32767.4 * FG, -32768.4 * FG, 32768.0 * BG, -32769.0 * BG, 1e9, -1e9, 3e38, -3e38, 32766.5 * BG], np.float32)
            at = rng.random(shape) < 0.1
            c[at] = rng.choice(edge, int(at.sum()))
    if bits:
        odd = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0x00800000], np.uint32)
        at = rng.random(shape) < 0.15
        c.view(np.uint32)[at] = rng.choice(odd, int(at.sum()))
        at = rng.random(shape) < 0.05
        c.view(np.uint32)[at] = rng.integers(0, 2 ** 32, int(at.sum()), dtype=np.uint64).astype(np.uint32)
    return c


def _records(n, w, h, block, mv, emit_h, density, seed, bits=False):
    """Records (n, frame bytes) u8 with random coefficients and type words uniform over each MV block (0, 1, 2 and a large id)."""
    rng = np.random.default_rng(seed)
    tx, rows = w // block, -(-emit_h // block)
    words = np.zeros((n, rows, tx, 1 + 3 * block * block), np.uint32)
    mv_types = rng.choice(np.array([0, 1, 2, BIG_ID], np.uint32), (n, h // mv, w // mv))
    per_tile = np.repeat(np.repeat(mv_types, mv // block, 1), mv // block, 2)
    words[..., 0] = per_tile[:, :rows]
    words[..., 1:] = _coefficients(rng, (n, rows, tx, 3 * block * block), density, bits).view(np.uint32)
    return words.view(np.uint8).reshape(n, -1)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer views are read-only)


def _used(out, offsets):
    torch.cuda.synchronize()
    o = offsets.cpu().numpy()
    return out[:int(o[-1])].cpu().numpy().tobytes(), o.astype(np.uint64)


def _through_planes(rec_np, w, h, block, mv, emit_h, fg, bg):
    """The device route that exists: the numpy parse, the planes and MV-block types uploaded, svc_hip_pack_levels_frames."""
    types, planes = wire.parse_records(rec_np, w, h, block, emit_h)
    s = mv // block
    mv_types = np.ascontiguousarray(types[:, ::s, ::s]).reshape(rec_np.shape[0], -1)
    out, offsets = native.pack_levels_frames(_cuda(planes), _cuda(mv_types.view(np.int32)), block, mv, fg, bg)
    return _used(out, offsets)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_equals_the_numpy_statement_and_the_route_through_planes(native, shape, density):
    w, h, block, mv, emit_h = shape
    n = 3
    rec_np = _records(n, w, h, block, mv, emit_h, density, seed=7 * sum(shape) + DENSITIES.index(density))
    out, offsets, status = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG, emit_h=emit_h)
    got, got_offsets = _used(out, offsets)
    want, want_offsets, want_status = wire.pack_records(rec_np, w, h, block, mv, mv, FG, BG, emit_h=emit_h)
    assert np.array_equal(got_offsets, want_offsets)
    assert got == want
    assert status.cpu().tolist() == want_status.tolist() == [0] * n
    via, via_offsets = _through_planes(rec_np, w, h, block, mv, emit_h, FG, BG)
    assert np.array_equal(got_offsets, via_offsets) and got == via
    if density == "dense":
        hdr, _, _ = levels.parse_frame(got)
        assert hdr["level_count"] == 3 * w * (-(-emit_h // block) * block)


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_on_any_bits_equals_the_route_through_planes(native, shape, n):
    """NaN, +-Inf, -0.0, denormals and random words: the header's inexact word, masks and levels are those of pack_levels_frames."""
    w, h, block, mv, emit_h = shape
    rec_np = _records(n, w, h, block, mv, emit_h, "sparse" if n == 17 else "clamp", seed=31 * n + w, bits=True)
    for fg, bg in ((1, 640), (FG, BG)):
        out, offsets, status = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, fg, bg, emit_h=emit_h)
        got, got_offsets = _used(out, offsets)
        via, via_offsets = _through_planes(rec_np, w, h, block, mv, emit_h, fg, bg)
        assert np.array_equal(got_offsets, via_offsets) and got == via
        assert status.cpu().tolist() == [0] * n


def test_a_record_that_disagrees_with_its_block_is_status_4(native):
    w, h, block, mv, n = 48, 16, 8, 16, 3
    rec_np = _records(n, w, h, block, mv, h, "sparse", seed=4).copy()
    want, want_offsets, _ = wire.pack_records(rec_np, w, h, block, mv, mv, FG, BG)
    words = rec_np.view(np.uint32).reshape(n, h // block, w // block, -1)
    words[1, 1, 3, 0] += 1  # no MV block's origin
    out, offsets, status = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG)
    got, got_offsets = _used(out, offsets)
    assert status.cpu().tolist() == [0, 4, 0]
    assert got == want and np.array_equal(got_offsets, want_offsets)  # the frame comes out by the origin rule
    words[2, 0, 2, 0] = 9  # the origin of frame 2's MV block (0, 1)
    out, offsets, status = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG)
    got, got_offsets = _used(out, offsets)
    want, want_offsets, want_status = wire.pack_records(rec_np, w, h, block, mv, mv, FG, BG)
    assert status.cpu().tolist() == want_status.tolist() == [0, 4, 4]
    assert got == want and np.array_equal(got_offsets, want_offsets)
    _, t, _ = levels.parse_frame(got[int(got_offsets[2]):])
    assert t[0, 1] == 9


def test_forward_with_a_padded_stride_and_records_at_4_mod_8(native):
    w, h, block, mv, n = 48, 16, 8, 16, 3
    rec_np = _records(n, w, h, block, mv, h, "sparse", seed=8)
    base, base_offsets = _used(*native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG)[:2])
    wide = np.full((n, rec_np.shape[1] + 4), 0xA5, np.uint8)
    wide[:, :-4] = rec_np
    got, got_offsets = _used(*native.records_pack_levels_frames(_cuda(wide), w, h, block, mv, FG, BG)[:2])
    assert got == base and np.array_equal(got_offsets, base_offsets)
    placed = gd.placed(_cuda(rec_np), 3, 4)
    assert placed.data_ptr() % 8 == 4
    got, got_offsets = _used(*native.records_pack_levels_frames(placed, w, h, block, mv, FG, BG)[:2])
    assert got == base and np.array_equal(got_offsets, base_offsets)


# ---- the reverse ----------------------------------------------------------------------------------------------------------------------

def _stream_of(shape, n, density, seed):
    """A compact stream on the device, exactly its bytes long, with its offsets."""
    w, h, block, mv, _ = shape
    rec_np = _records(n, w, h, block, mv, h, density, seed)
    out, offsets, _ = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG)
    torch.cuda.synchronize()
    return out[:int(offsets[-1])].clone(), offsets


def _via_planes(frames, offsets, shape):
    w, h, block, mv, emit_h = shape
    planes, types, status = native.unpack_levels_frames(frames, offsets, w, h, block, mv)
    rec = native.serialize_frames(planes, types, w, emit_h, block, block, w // mv, h // mv, mv)
    torch.cuda.synchronize()
    return rec, status


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reverse_equals_the_numpy_statement_and_the_route_through_planes(native, shape, density):
    w, h, block, mv, emit_h = shape
    frames, offsets = _stream_of(shape, 3, density, seed=11 * sum(shape) + DENSITIES.index(density))
    rec, status = native.levels_records_frames(frames, offsets, w, h, block, mv, emit_h=emit_h)
    via, via_status = _via_planes(frames, offsets, shape)
    assert torch.equal(rec, via) and status.cpu().tolist() == via_status.cpu().tolist() == [0, 0, 0]
    want = wire.write_stream(frames.cpu().numpy().tobytes(), offsets.cpu().numpy(), emit_h=emit_h)
    assert rec.cpu().numpy().tobytes() == want[wire.HEADER_BYTES:]


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[6], SHAPES[10]], ids=_ids)
def test_reverse_of_frames_that_fail_each_check(native, shape):
    """One good frame, then frames corrupted to the statuses 2 .. 7 of svc_hip_unpack_levels_frames, and a last frame whose end lies past
    the stream (1): the statuses and the records are those of the route through planes, a failed frame all zeros."""
    w, h, block, mv, emit_h = shape
    frames, offsets = _stream_of(shape, 8, "dense", seed=12)
    o = offsets.cpu().numpy().copy()
    buf = frames.cpu().numpy().copy()
    head = lambda f: buf[int(o[f]):int(o[f]) + 64].view(np.uint32)
    head(1)[0] ^= 1          # magic
    head(2)[1] = 2           # version
    head(3)[8] = 0           # a step of 0
    head(4)[12] += 16        # the frame's bytes
    head(5)[10] -= 1         # the level count
    want = [0, 2, 3, 4, 5, 6, 0, 1]
    if (block * block) % 64:  # a mask word with bits past the tile
        masks_off = 64 + 4 * (w // mv) * (h // mv)
        buf[int(o[6]) + masks_off + 7] |= 0x80
        want[6] = 7
    o[8] += 16               # past the stream
    frames, offsets = _cuda(buf), _cuda(o)
    fill = torch.full((8, native.serialized_frame_bytes(w, emit_h, block, block)), 0x5A, dtype=torch.uint8, device="cuda")
    rec, status = native.levels_records_frames(frames, offsets, w, h, block, mv, emit_h=emit_h, records=fill)
    via, via_status = _via_planes(frames, offsets, shape)
    assert status.cpu().tolist() == via_status.cpu().tolist() == want
    assert torch.equal(rec, via)
    for f, st in enumerate(want):
        assert bool(rec[f].any()) == (st == 0), f


def test_reverse_leaves_the_stride_past_a_frames_records(native):
    shape = SHAPES[3]
    w, h, block, mv, emit_h = shape
    frames, offsets = _stream_of(shape, 3, "sparse", seed=2)
    base, _ = native.levels_records_frames(frames, offsets, w, h, block, mv)
    wide = torch.full((3, base.shape[1] + 4), 0xC3, dtype=torch.uint8, device="cuda")
    native.levels_records_frames(frames, offsets, w, h, block, mv, records=wide)
    assert torch.equal(wide[:, :-4], base) and bool((wide[:, -4:] == 0xC3).all())


# ---- loops ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5], SHAPES[6], SHAPES[7]], ids=_ids)
def test_pack_of_the_records_of_a_pack_is_that_pack(native, shape):
    w, h, block, mv, _ = shape
    rec_np = _records(3, w, h, block, mv, h, "clamp", seed=6)
    out, offsets, _ = native.records_pack_levels_frames(_cuda(rec_np), w, h, block, mv, FG, BG)
    first, first_offsets = _used(out, offsets)
    rec, status = native.levels_records_frames(out[:len(first)].clone(), offsets, w, h, block, mv)
    assert status.cpu().tolist() == [0, 0, 0]
    again, again_offsets = _used(*native.records_pack_levels_frames(rec, w, h, block, mv, FG, BG)[:2])
    assert np.array_equal(first_offsets, again_offsets)
    # requantised records are exact: only the inexact word (header word 11) may differ
    a, b = np.frombuffer(first, np.uint8).copy(), np.frombuffer(again, np.uint8).copy()
    for f in range(3):
        assert b[int(first_offsets[f]) + 44:int(first_offsets[f]) + 48].view(np.uint32)[0] == 0
        a[int(first_offsets[f]) + 44:int(first_offsets[f]) + 48] = 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("w,h,block,mv", [(48, 16, 8, 16), (64, 32, 16, 16), (272, 16, 8, 8)])
def test_decode_of_the_transcoded_stream_is_the_decode_of_the_records(native, w, h, block, mv):
    """svc_hip_decode_levels_frames of the transcoded stream against svc_hip_decode_records_frames of the records, the same steps on both
    sides and no gaze: both quantise std::round(c / step) in f32 and decode level * step, so d_rec is bit-identical."""
    n = 3
    rec_np = _records(n, w, h, block, mv, h, "dense", seed=w)  # |c| < 2000: within int16 at both steps
    records = _cuda(rec_np)
    out, offsets, status = native.records_pack_levels_frames(records, w, h, block, mv, FG, BG)
    rec_q, _, st = native.decode_levels_frames(out, offsets, w, h, block, mv, FG, BG)
    rec_w, _ = native.decode_records_frames(records, w, h, block, FG, BG)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == st.cpu().tolist() == [0] * n
    assert torch.equal(rec_q.view(torch.int32), rec_w.view(torch.int32))


def test_through_the_entropy_coder_and_back(native):
    shape = SHAPES[3]
    w, h, block, mv, _ = shape
    frames, offsets = _stream_of(shape, 3, "sparse", seed=21)
    coded, coded_offsets, st = native.entropy_encode_frames(frames, offsets, w, h, block, mv)
    back, back_offsets, st2 = native.entropy_decode_frames(coded, coded_offsets, w, h, block, mv)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st2.cpu().tolist() == [0, 0, 0] and torch.equal(back_offsets, offsets)
    assert torch.equal(back[:frames.numel()], frames)
    rec, _ = native.levels_records_frames(back[:frames.numel()].clone(), back_offsets, w, h, block, mv)
    want, _ = native.levels_records_frames(frames, offsets, w, h, block, mv)
    assert torch.equal(rec, want)


# ---- refusals: each item of the check order, with null pointers and no GPU work ------------------------------------------------------------

def _refused(fn, args, status, match):
    rc = fn(*args)
    msg = native.load().svc_hip_last_error().decode()
    assert rc == status, (rc, msg)
    assert match in msg, msg


def test_forward_refusals_in_the_documented_order():
    lib = native.load()
    fn = lib.svc_hip_records_pack_levels_frames
    w, h, block, mv, n = 32, 16, 8, 8, 2
    per = 4 * (1 + 3 * 64) * 8
    ws = lib.svc_hip_records_pack_levels_workspace_bytes(n, w, h, block, mv, mv)
    cap = lib.svc_hip_levels_max_bytes(n, w, h, block, block, mv, mv)
    assert ws > 0 and cap > 0

    def args(**kw):
        a = dict(stride=per, n=n, w=w, h=h, block=block, emit=h, mvw=mv, mvh=mv, fg=1, bg=640, ws=ws, cap=cap)
        a.update(kw)
        return (None, a["stride"], a["n"], a["w"], a["h"], a["block"], a["emit"], a["mvw"], a["mvh"], a["fg"], a["bg"], None, a["ws"], None,
                a["cap"], None, None, None)

    INV, UNS = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    # every later item is wrong too: the earlier one answers
    _refused(fn, args(w=30, fg=0, stride=2, ws=0, cap=0), INV, "not divisible")
    _refused(fn, args(mvw=12, fg=0, stride=2, ws=0, cap=0), INV, "MV block")
    _refused(fn, args(emit=0, fg=0, stride=2, ws=0, cap=0), INV, "emit_frame_h")
    _refused(fn, args(emit=h + 1, fg=0, stride=2, ws=0, cap=0), INV, "emit_frame_h")
    _refused(fn, args(fg=0, stride=2, ws=0, cap=0), INV, "steps")
    _refused(fn, args(bg=0, stride=2, ws=0, cap=0), INV, "steps")
    _refused(fn, args(w=256, h=256, block=256, emit=256, mvw=256, mvh=256, stride=2, ws=0, cap=0), UNS, "int16")
    _refused(fn, args(w=128, h=128, block=128, emit=128, mvw=128, mvh=128, stride=2, ws=0, cap=0), UNS, "tiles above")
    _refused(fn, args(n=65536, stride=2, ws=0, cap=0), UNS, "65535")
    _refused(fn, args(stride=per - 4, ws=0, cap=0), INV, "stride")
    _refused(fn, args(stride=per + 2, ws=0, cap=0), INV, "stride")
    _refused(fn, args(ws=ws - 1, cap=0), INV, "workspace")
    _refused(fn, args(cap=cap - 1), INV, "output")
    _refused(fn, args(), INV, "null pointer")
    assert fn(*args(n=0, ws=0, cap=0)) == native.SVC_OK
    _refused(fn, args(n=0, fg=0), INV, "steps")  # the checks run for an empty batch too
    assert lib.svc_hip_records_pack_levels_workspace_bytes(n, 30, h, block, mv, mv) == 0


def test_reverse_refusals_in_the_documented_order():
    lib = native.load()
    fn = lib.svc_hip_levels_records_frames
    w, h, block, mv, n = 32, 16, 8, 8, 2
    per = 4 * (1 + 3 * 64) * 8
    ws = lib.svc_hip_levels_records_workspace_bytes(n, w, h, block, block)
    assert ws > 0 and ws == lib.svc_hip_pack_levels_workspace_bytes(n, w, h, block, block)

    def args(**kw):
        a = dict(n=n, w=w, h=h, bw=block, bh=block, mvw=mv, mvh=mv, emit=h, ws=ws, stride=per)
        a.update(kw)
        return (None, 0, None, a["n"], a["w"], a["h"], a["bw"], a["bh"], a["mvw"], a["mvh"], a["emit"], None, a["ws"], None, a["stride"],
                None, None)

    INV, UNS = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    _refused(fn, args(w=30, emit=0, stride=2, ws=0), INV, "not divisible")
    _refused(fn, args(bw=16, bh=8, mvw=16, emit=0, stride=2, ws=0), UNS, "non-square")
    _refused(fn, args(emit=0, stride=2, ws=0), INV, "emit_frame_h")
    _refused(fn, args(emit=h + 1, stride=2, ws=0), INV, "emit_frame_h")
    _refused(fn, args(w=128, h=128, bw=128, bh=128, mvw=128, mvh=128, emit=128, stride=2, ws=0), UNS, "tiles above")
    _refused(fn, args(n=65536, stride=2, ws=0), UNS, "65535")
    _refused(fn, args(stride=per - 4, ws=0), INV, "stride")
    _refused(fn, args(stride=per + 2, ws=0), INV, "stride")
    _refused(fn, args(ws=ws - 1), INV, "workspace")
    _refused(fn, args(), INV, "null pointer")
    assert fn(*args(n=0, ws=0)) == native.SVC_OK


# ---- guards and placement -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[6], SHAPES[7], SHAPES[10]], ids=_ids)
def test_forward_writes_inside_buffers_of_exactly_the_size_it_asks_for(native, shape):
    w, h, block, mv, emit_h = shape
    n = 3
    records = _cuda(_records(n, w, h, block, mv, emit_h, "clamp", seed=15))
    written = {"out": gd.Guarded(native.levels_max_bytes(n, w, h, block, mv), device="cuda"),
               "workspace": gd.Guarded(native.records_pack_levels_workspace_bytes(n, w, h, block, mv), device="cuda", seed=1),
               "offsets": gd.Guarded(8 * (n + 1), torch.int64, "cuda", seed=2),
               "status": gd.Guarded(4 * n, torch.int32, "cuda", seed=3)}

    def call():
        out, offsets, status = native.records_pack_levels_frames(
            records, w, h, block, mv, FG, BG, emit_h=emit_h, out=written["out"].interior, offsets=written["offsets"].interior,
            workspace=written["workspace"].interior, status=written["status"].interior)
        torch.cuda.synchronize()
        return {"stream": out[:int(offsets[-1])], "offsets": offsets, "status": status}

    assert gd.check_writes("records_pack_levels_frames", written, call, seed=4, names=("zeros", "ones", "random")) == []


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[6], SHAPES[7], SHAPES[10]], ids=_ids)
def test_reverse_writes_inside_buffers_of_exactly_the_size_it_asks_for(native, shape):
    w, h, block, mv, emit_h = shape
    n = 3
    frames, offsets = _stream_of(shape, n, "clamp", seed=16)
    per = native.serialized_frame_bytes(w, emit_h, block, block)
    written = {"records": gd.Guarded(n * per, device="cuda", shape=(n, per), **gd.exactly(4)),
               "workspace": gd.Guarded(native.levels_records_workspace_bytes(n, w, h, block), device="cuda", seed=1),
               "status": gd.Guarded(4 * n, torch.int32, "cuda", seed=3)}

    def call():
        rec, status = native.levels_records_frames(frames, offsets, w, h, block, mv, emit_h=emit_h, records=written["records"].interior,
                                                   workspace=written["workspace"].interior, status=written["status"].interior)
        torch.cuda.synchronize()
        return {"records": rec, "status": status}

    assert written["records"].addr % 8 == 4
    assert gd.check_writes("levels_records_frames", written, call, seed=5, names=("zeros", "ones", "random")) == []


def test_neither_direction_reads_past_its_inputs(native):
    shape = SHAPES[3]
    w, h, block, mv, emit_h = shape
    records = _cuda(_records(3, w, h, block, mv, emit_h, "sparse", seed=17))

    def forward(given):
        out, offsets, status = native.records_pack_levels_frames(given["records"], w, h, block, mv, FG, BG)
        torch.cuda.synchronize()
        return {"stream": out[:int(offsets[-1])], "offsets": offsets, "status": status}

    assert gd.check_reads("records_pack_levels_frames", {"records": records}, forward) == []
    frames, offsets = _stream_of(shape, 3, "sparse", seed=18)

    def reverse(given):
        rec, status = native.levels_records_frames(given["frames"], given["offsets"], w, h, block, mv)
        torch.cuda.synchronize()
        return {"records": rec, "status": status}

    assert gd.check_reads("levels_records_frames", {"frames": frames, "offsets": offsets}, reverse) == []


# ---- the host driver: tests/dropin/wire_transcode_main (svc::WireTranscoder) ------------------------------------------------------------

BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")


def _run(name, args, data):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    r = subprocess.run([exe, *args], input=data, capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr).decode(errors="replace")[-2000:]
    return r.stdout, r.stderr.decode()


def _compact_file(data):
    n, = struct.unpack_from("<Q", data)
    offsets = np.frombuffer(data, "<u8", n + 1, 8)
    body = data[8 * (n + 2):]
    assert len(body) == int(offsets[-1]) and offsets[0] == 0
    return n, offsets, body


@pytest.fixture(scope="module")
def encoded(native):
    """A small clip through HostStreamEncoder(wire=True): the stream in the decoder's reading (the padded grid) and, cut from it, in the
    reference encoder's reading (its unpadded tile loops: 25 of 26 tile rows)."""
    cfg = configs.CodecConfig("wire-transcode-320x200", 95, 320, 200, 12, levels=3, dct_block=8)
    clip = synth.SynthClip(cfg.width, cfg.height, cfg.frames, cfg.seed, device="cuda")
    host = torch.stack([clip.frame_bgr(t) for t in range(cfg.frames)]).cpu().numpy()
    header, chunks = b"", []
    for o in stream.HostStreamEncoder(cfg, batch=4, device=torch.device("cuda"), wire=True).encode(host):
        header = o.get("header", header)
        chunks.append(o["records"].tobytes())
    padded = header + b"".join(chunks)
    pw, ph = cfg.padded
    assert (pw, ph) == (320, 208)
    _, records, _, _ = wire.read_stream(padded)
    unpadded = header + np.ascontiguousarray(records[:, :wire.frame_bytes(pw, cfg.height, 8)]).tobytes()
    assert native.wire_layout(unpadded[:32], len(unpadded))[0] == cfg.height
    return cfg, {"padded": padded, "unpadded": unpadded}


@pytest.mark.parametrize("reading", ["padded", "unpadded"])
@pytest.mark.parametrize("entropy", [False, True], ids=["svcq", "svce"])
def test_wire_transcode_main_equals_the_device_calls(native, encoded, tmp_path, reading, entropy):
    cfg, streams = encoded
    big = streams[reading]
    pw, ph = cfg.padded
    fg, bg, mv = 2, 40, 16
    hdr, records, _, _ = wire.read_stream(big)
    n = hdr["frame_count"]
    emit_h = ph if reading == "padded" else cfg.height
    out, offsets, status = native.records_pack_levels_frames(_cuda(records), pw, ph, 8, mv, fg, bg, emit_h=emit_h)
    want, want_offsets = _used(out, offsets)
    assert status.cpu().tolist() == [0] * n  # the encoder's types are uniform over its 16 x 16 MV blocks
    if entropy:
        coded, coded_offsets, st = native.entropy_encode_frames(out[:len(want)].clone(), offsets, pw, ph, 8, mv)
        assert st.cpu().tolist() == [0] * n
        want, want_offsets = _used(coded, coded_offsets)
    args = ["--mv-block", str(mv), "--foreground-quant-step", str(fg), "--background-quant-step", str(bg), "--batch", "5"]
    got, err = _run("wire_transcode_main", ["to-compact", *args] + (["--entropy"] if entropy else []), big)
    assert err == ""
    m, got_offsets, body = _compact_file(got)
    assert m == n and np.array_equal(got_offsets, want_offsets) and body == want

    # and back: records the wire decoder plays to the display frames of a stream requantised at the same steps
    back, err = _run("wire_transcode_main", ["to-wire", "--source", f"{cfg.width}x{cfg.height}", "--batch", "3"] +
                     (["--emit-h", str(cfg.height)] if reading == "unpadded" else []), got)
    assert err == "" and back[:32] == big[:32] and len(back) == len(big)
    svcq = _cuda(np.frombuffer(body if not entropy else _used(out, offsets)[0], np.uint8))
    rec, st = native.levels_records_frames(svcq, offsets, pw, ph, 8, mv, emit_h=emit_h)
    assert st.cpu().tolist() == [0] * n and back[32:] == rec.cpu().numpy().tobytes()
    steps = ["--foreground-quant-step", str(fg), "--background-quant-step", str(bg)]
    gaze = tmp_path / "gaze.txt"
    gaze.write_text("-\n" * n)
    shown = []
    for name, data in (("orig", big), ("back", back)):
        path = tmp_path / f"{name}.raw"
        _run("wire_decode_main", ["--gaze", str(gaze), "--out", str(path), *steps], data)
        shown.append(np.fromfile(path, np.uint8))
    assert shown[0].size == n * cfg.width * cfg.height * 3 and np.array_equal(shown[0], shown[1])
