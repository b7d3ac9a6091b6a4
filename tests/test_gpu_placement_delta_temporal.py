"""The three temporal calls (include/svc_hip.h, "Temporal layers") at the weakest placement the header admits, the way
tests/test_gpu_placement_delta.py and tests/test_gpu_placement_decode_delta.py test their period-1 siblings
(tests/test_gpu_placement_streams.py's Case with the builders of tests/test_gpu_guard_delta_temporal.py): every written buffer a Guarded of
exactly the asked size at gd.exactly(A), every input surrounded at exactly(A) -- streams, the frame before, the last frame and workspace 16
bytes, offsets and the last frame's length 8, key flags, gaze, rec and status 4.  Per case the guards are intact, every output is bit for
bit that of the same call on 256-byte aligned buffers, the streams are the numpy statement's, and the decode's rec, display, status and last
frame are those of svc_hip_undelta_levels_temporal_frames followed by svc_hip_decode_levels_frames.  One notch below, each pointer alone at
exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that names alignment, and no byte of any output changes."""
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_delta import key_flags
from tests.test_gpu_guard_delta_temporal import ENTRIES, clip_parts, period_of
from tests.test_gpu_guard_streams import DEC, G8, G16, GX, NS, _cuda, _gid
from tests.test_gpu_placement_streams import A_IN, A_OUT, Case, _same_stream

pytestmark = pytest.mark.gpu

OUT_AT = {**A_OUT, "last": 16, "last bytes": 8}
IN_AT = {**A_IN, "prev": 16, "key": 4}
STREAM_GEOMS = (G8[1], G16[1], GX[2])  # 8 x 8 with masks only 4-byte aligned, 16 x 16 in one group, 6 x 6 tiles
DECODE_GEOMS = (G8[0], G8[1], G16[1])  # a group of 32 tiles and one of 2; masks only 4-byte aligned; 16 x 16 in one group
PAIRS = [(e, g) for e in ENTRIES for g in (DECODE_GEOMS if e.startswith("decode") else STREAM_GEOMS)]


def _reference(c, got):
    period = period_of(c.entry)
    w, h, tile, mv = c.geom
    prev, stream, offs, diff, diff_offs = clip_parts(c.geom, c.n, period, 0)
    if c.entry.startswith("delta"):
        _same_stream(got["stream"], got["offsets"], diff.tobytes(), diff_offs, c.entry)
    elif c.entry.startswith("undelta"):
        _same_stream(got["stream"], got["offsets"], *layers.undelta_temporal_frames(diff, diff_offs, period, key_flags(c.n), prev=prev), c.entry)
        _same_stream(got["stream"], got["offsets"], stream.tobytes(), offs, c.entry + ", against the frames the delta stream was made from")
    else:  # undelta, then decode, on fresh allocations
        back, back_offs, st = nat.undelta_levels_temporal_frames(_cuda(diff), _cuda(diff_offs), w, h, tile, mv, period, prev=_cuda(prev),
                                                                 key=key_flags(c.n))
        o = back_offs.cpu().tolist()
        rec, disp, _ = nat.decode_levels_frames(back[:o[-1]].clone(), back_offs, w, h, tile, mv, *DEC, gaze=c.inputs["gaze"],
                                                display=(max(1, w - 5), max(1, h - 3)))
        torch.cuda.synchronize()
        at = period * ((c.n - 1) // period)
        want = {"rec": rec.cpu(), "display": disp.cpu(), "status": st.cpu(), "last": back[o[at]:o[at + 1]].cpu()}
        findings = gd.output_findings(f"{c.entry} {_gid(c.geom)} n={c.n}", want, {k: got[k] for k in want}, "differs from undelta then decode")
        assert not findings, "\n".join(findings)
        assert int(got["last bytes"][0]) == want["last"].numel()


def test_the_tables_name_every_buffer(native):
    for entry, geom in PAIRS:
        c = Case(entry, geom, 3, OUT_AT, IN_AT, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
        for k, g in c.pool.written.items():
            assert g.addr % (2 * OUT_AT[k]) == OUT_AT[k], (entry, k)
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * IN_AT[k]) == IN_AT[k], (entry, k)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_at_the_weakest_placement(native, entry, geom):
    for n in NS:
        aligned = Case(entry, geom, n, table=ENTRIES).run()
        c = Case(entry, geom, n, OUT_AT, IN_AT, table=ENTRIES)
        got = c.run()
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", aligned, got, "differs from the same call on 256-byte aligned buffers")
        assert not findings, "\n".join(findings)
        assert got["status"].tolist() == [0] * n
        _reference(c, got)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_one_notch_below_is_refused(native, entry):
    n, geom = 3, G8[1]
    probe = Case(entry, geom, n, OUT_AT, IN_AT, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if OUT_AT[k] > 1] + [("in", k) for k in probe.inputs if IN_AT[k] > 1]
    assert len(rows) == (10 if entry.startswith("decode") else 8), rows
    for side, name in rows:
        out_at = {**OUT_AT, name: OUT_AT[name] // 2} if side == "out" else OUT_AT
        in_at = {**IN_AT, name: IN_AT[name] // 2} if side == "in" else IN_AT
        c = Case(entry, geom, n, out_at, in_at, table=ENTRIES)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(OUT_AT if side == 'out' else IN_AT)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
