"""svc_hip_decode_delta_levels_temporal_reduced_frames at the weakest placement include/svc_hip_temporal_decode.h admits, periods 2 and 4,
the way tests/test_gpu_placement_decode_delta_reduced.py tests the period-1 call (tests/test_gpu_placement_streams.py's Case with the
builder of tests/test_gpu_guard_decode_delta_temporal_reduced.py): every written buffer a Guarded of exactly the asked size at
gd.exactly(A), every input surrounded at exactly(A) -- streams, the frame before, the last frame and workspace 16 bytes, offsets and the
last frame's length 8, key flags, gaze, rec and status 4.  Per case the guards are intact, every output is bit for bit that of the same
call on 256-byte aligned buffers, and rec, display, status and the last frame are those of svc_hip_undelta_levels_temporal_frames followed
by svc_hip_decode_levels_reduced_frames and, for frame period * ((n - 1) // period), svc_hip_band_levels_frames.  One notch below, each
pointer alone at exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that names alignment, and no byte of any output
changes."""
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_decode_delta_temporal_reduced import ENTRIES, ENTRY, PERIODS, REDUCES
from tests.test_gpu_guard_delta import key_flags
from tests.test_gpu_guard_delta_temporal import clip_parts
from tests.test_gpu_guard_streams import DEC, G8, G16, NS, _cuda, _gid
from tests.test_gpu_placement_streams import A_IN, A_OUT, Case

pytestmark = pytest.mark.gpu

OUT_AT = {**A_OUT, "last": 16, "last bytes": 8}
IN_AT = {**A_IN, "prev": 16, "key": 4}
GEOMS = (G8[0], G8[1], G16[1])  # a group of 32 tiles and one of 2; masks only 4-byte aligned; 16 x 16 in one group
TRIPLES = [(g, r, p) for g in GEOMS for r in REDUCES for p in PERIODS]


def _two_calls(c, reduce, period):
    """The temporal undelta, then the reduced decode, then the band of frame period * ((n - 1) // period), on fresh allocations ->
    (rec, display, status, last)."""
    w, h, tile, mv = c.geom
    k = tile[0] // reduce
    prev, stream, offs, diff, diff_offs = clip_parts(c.geom, c.n, period, 0)
    back, back_offs, st = nat.undelta_levels_temporal_frames(_cuda(diff), _cuda(diff_offs), w, h, tile, mv, period, prev=_cuda(prev),
                                                             key=key_flags(c.n))
    o = back_offs.cpu().tolist()
    rec, disp, _ = nat.decode_levels_reduced_frames(back[:o[-1]].clone(), back_offs, w, h, tile, mv, *DEC, reduce, gaze=c.inputs["gaze"],
                                                    display=(max(1, w // reduce - 5), max(1, h // reduce - 3)))
    at = period * ((c.n - 1) // period)
    band, band_offs, _ = nat.band_levels_frames(back[o[at]:o[at + 1]].clone(), torch.tensor([0, o[at + 1] - o[at]], dtype=torch.int64, device="cuda"),
                                                w, h, tile, mv, band=[(0, 0, k, k)])
    torch.cuda.synchronize()
    assert back[:o[-1]].cpu().numpy().tobytes() == stream.tobytes()  # the frames the delta stream was made from
    return {"rec": rec.cpu(), "display": disp.cpu(), "status": st.cpu(), "last": band[:int(band_offs[1])].cpu()}


def test_the_tables_name_every_buffer(native):
    for geom, r, p in TRIPLES:
        c = Case(f"{ENTRY}_r{r}_p{p}", geom, 3, OUT_AT, IN_AT, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
        assert sorted(c.pool.written) == ["display", "last", "last bytes", "rec", "status", "workspace"]
        assert sorted(c.given) == ["gaze", "key", "offsets", "prev", "stream"]
        for k, g in c.pool.written.items():
            assert g.addr % (2 * OUT_AT[k]) == OUT_AT[k], k
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * IN_AT[k]) == IN_AT[k], k


@pytest.mark.parametrize("geom,reduce,period", TRIPLES, ids=[f"{_gid(g)}-r{r}-p{p}" for g, r, p in TRIPLES])
def test_at_the_weakest_placement(native, geom, reduce, period):
    entry = f"{ENTRY}_r{reduce}_p{period}"
    for n in NS:
        aligned = Case(entry, geom, n, table=ENTRIES).run()
        c = Case(entry, geom, n, OUT_AT, IN_AT, table=ENTRIES)
        got = c.run()
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", aligned, got, "differs from the same call on 256-byte aligned buffers")
        assert not findings, "\n".join(findings)
        assert got["status"].tolist() == [0] * n
        want = _two_calls(c, reduce, period)
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", want, {k: got[k] for k in want},
                                      "differs from the temporal undelta, then the reduced decode and the band of the carried frame")
        assert not findings, "\n".join(findings)
        assert int(got["last bytes"][0]) == want["last"].numel()


@pytest.mark.parametrize("period", PERIODS)
def test_one_notch_below_is_refused(native, period):
    n, geom, entry = 3, GEOMS[1], f"{ENTRY}_r4_p{period}"
    probe = Case(entry, geom, n, OUT_AT, IN_AT, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if OUT_AT[k] > 1] + [("in", k) for k in probe.inputs if IN_AT[k] > 1]
    assert len(rows) == 10, rows  # five written buffers (the display is bytes) and five inputs
    for side, name in rows:
        out_at = {**OUT_AT, name: OUT_AT[name] // 2} if side == "out" else OUT_AT
        in_at = {**IN_AT, name: IN_AT[name] // 2} if side == "in" else IN_AT
        c = Case(entry, geom, n, out_at, in_at, table=ENTRIES)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(OUT_AT if side == 'out' else IN_AT)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
