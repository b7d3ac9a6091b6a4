"""svc_hip_dct_pack_delta_temporal_frames and svc_hip_dct_pack_delta_temporal_auto_frames at the weakest placement
include/svc_hip_temporal.h admits, periods 2 and 4, the way tests/test_gpu_placement_streams.py tests the other stream entry points (its
Case, with the builders of tests/test_gpu_guard_dct_pack_delta_temporal.py): every written buffer a Guarded of exactly the asked size at
gd.exactly(A), every input surrounded at exactly(A) -- frames, the frame at index -period, output and workspace 16 bytes, offsets 8,
region ids (that frame's too), key, forced and chosen flags and level counts 4; the frame stride is a multiple of 16 and not of 32.  Per
case the guards are intact and every output is bit for bit that of the same call on 256-byte aligned buffers; the fixed-flag call's
stream is that of the two device calls it replaces, the auto call's flags and counts are the numpy statement's of the fused plain stream
and its stream the fixed-flag call's with those flags.  One notch below, each pointer alone at exactly(A / 2) is refused with
SVC_ERR_INVALID_ARG and a message that names alignment, and no byte of any output changes."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_dct_pack_delta_temporal import ENTRIES, GEOMS, N, REPEATED, STEPS, flags, frames_and_types, period_of
from tests.test_gpu_guard_streams import _bgr, _gid
from tests.test_gpu_placement_streams import A_IN, A_OUT, Case, _same_stream

pytestmark = pytest.mark.gpu

OUT_AT = {**A_OUT, "key out": 4, "counts": 4}
IN_AT = {**A_IN, "prev": 16, "prev types": 4, "key": 4, "forced": 4}


def _plain(geom, n):
    """svc_hip_dct_pack_levels_frames on the n + 1 frames -> (buffer, stride, types, the stream on the device, its offsets there and as a list)."""
    w, h, tile, mv = geom
    buf, stride, types = frames_and_types(geom, n, 0)
    out = torch.empty(nat.levels_max_bytes(n + 1, w, h, tile, mv), dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 2, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_levels_workspace_bytes(n + 1, w, h, tile[0], mv), dtype=torch.uint8, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_frames(buf.data_ptr(), stride, n + 1, w, h, tile[0], types.data_ptr(), *mv, *STEPS,
                                                        ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), nat._stream()))
    torch.cuda.synchronize()
    return buf, stride, types, out, offs, offs.cpu().tolist()


def _two_calls(geom, n, period):
    """... then svc_hip_delta_levels_temporal_frames on the last n with the first as d_prev."""
    w, h, tile, mv = geom
    _, _, _, out, offs, o = _plain(geom, n)
    want, want_offs, st = nat.delta_levels_temporal_frames(out[o[1]:o[-1]], offs[1:] - o[1], w, h, tile, mv, period, prev=out[:o[1]].clone(),
                                                           key=flags(n))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    return want[:int(want_offs[-1])].cpu().numpy().tobytes(), want_offs.cpu().tolist()


def _statement_and_fixed_call(geom, n, period):
    """The numpy statement of the plain stream, and svc_hip_dct_pack_delta_temporal_frames on the last n frames with the statement's flags
    -> (keys, counts, stream bytes, offsets)."""
    w, h, tile, mv = geom
    buf, stride, types, out, _, o = _plain(geom, n)
    o = np.asarray(o, np.int64)
    plain = out[:int(o[-1])].cpu().numpy()
    counts = layers.delta_level_counts(plain[o[1]:], (o[1:] - o[1]).astype(np.uint64), prev=plain[:o[1]], period=period)
    keys = layers.auto_keys(counts, flags(n), has_prev=True).astype(np.int64).tolist()
    d_out = torch.empty(nat.levels_max_bytes(n, w, h, tile, mv), dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_ws = torch.empty(nat.dct_pack_delta_temporal_workspace_bytes(n, w, h, tile[0], mv, period), dtype=torch.uint8, device="cuda")
    k = torch.tensor(keys, dtype=torch.int32, device="cuda")
    prev, prev_types, rest_types = buf[:w * h * 3].clone(), types[0].clone(), types[1:].contiguous()
    nat._check(nat.load().svc_hip_dct_pack_delta_temporal_frames(
        buf[stride:].data_ptr(), stride, n, w, h, tile[0], rest_types.data_ptr(), *mv, *STEPS, prev.data_ptr(), prev_types.data_ptr(),
        k.data_ptr(), d_ws.data_ptr(), d_ws.numel(), d_out.data_ptr(), d_out.numel(), d_offs.data_ptr(), nat._stream(), period))
    torch.cuda.synchronize()
    return keys, counts.astype(np.int64).reshape(-1).tolist(), d_out[:int(d_offs[-1])].cpu().numpy().tobytes(), d_offs.cpu().tolist()


def test_the_tables_name_every_buffer_and_the_stride_is_the_weakest(native):
    for entry in ENTRIES:
        for geom in GEOMS:
            c = Case(entry, geom, N, OUT_AT, IN_AT, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
            for k, g in c.pool.written.items():
                assert g.addr % (2 * OUT_AT[k]) == OUT_AT[k], (entry, k)
            for k, v in c.given.items():
                assert v.data_ptr() % (2 * IN_AT[k]) == IN_AT[k], (entry, k)
            assert _bgr(geom, N + 1)[1] % 32 == 16, geom


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_at_the_weakest_placement(native, entry, geom):
    aligned = Case(entry, geom, N, table=ENTRIES).run()
    c = Case(entry, geom, N, OUT_AT, IN_AT, table=ENTRIES)
    got = c.run()
    findings = gd.output_findings(f"{entry} {_gid(geom)} n={N}", aligned, got, "differs from the same call on 256-byte aligned buffers")
    assert not findings, "\n".join(findings)
    if "auto" in entry:
        keys, counts, stream, offs = _statement_and_fixed_call(geom, N, period_of(entry))
        assert keys[REPEATED] == 0 and counts[2 * REPEATED + 1] == 0 and 1 in keys  # both outcomes at this placement
        assert got["key out"].tolist() == keys and got["counts"].reshape(-1).tolist() == counts
        _same_stream(got["stream"], got["offsets"], stream, offs, entry)
    else:
        _same_stream(got["stream"], got["offsets"], *_two_calls(geom, N, period_of(entry)), entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_one_notch_below_is_refused(native, entry):
    geom = GEOMS[0]
    probe = Case(entry, geom, N, OUT_AT, IN_AT, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if OUT_AT[k] > 1] + [("in", k) for k in probe.inputs if IN_AT[k] > 1]
    assert len(rows) == (10 if "auto" in entry else 8), rows  # three or five written buffers and five inputs
    for side, name in rows:
        out_at = {**OUT_AT, name: OUT_AT[name] // 2} if side == "out" else OUT_AT
        in_at = {**IN_AT, name: IN_AT[name] // 2} if side == "in" else IN_AT
        c = Case(entry, geom, N, out_at, in_at, table=ENTRIES)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(OUT_AT if side == 'out' else IN_AT)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
