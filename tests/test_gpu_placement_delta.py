"""svc_hip_delta_levels_frames and svc_hip_undelta_levels_frames at the weakest placement include/svc_hip.h admits, the way
tests/test_gpu_placement_streams.py tests the other stream entry points (its Case, with the builders of tests/test_gpu_guard_delta.py):
every written buffer a Guarded of exactly the asked size at gd.exactly(A), every input surrounded at exactly(A) -- streams, the frame
before and workspace 16 bytes, offsets 8, key flags and status 4.  Per case the guards are intact, every output is bit for bit that of
the same call on 256-byte aligned buffers, and the stream is the numpy statement's.  One notch below, each pointer alone at
exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that names alignment, and no byte of any output changes."""
import pytest

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_delta import ENTRIES, clip_parts, key_flags
from tests.test_gpu_guard_streams import G8, G16, GX, NS, _gid
from tests.test_gpu_placement_streams import A_IN, A_OUT, Case, _same_stream

pytestmark = pytest.mark.gpu

IN_AT = {**A_IN, "prev": 16, "key": 4}
GEOMS = (G8[1], G16[1], GX[2])  # 8 x 8 with masks only 4-byte aligned, 16 x 16 in one group, 6 x 6 tiles
PAIRS = [(e, g) for e in ENTRIES for g in GEOMS]


def ref_delta_levels(c, got):
    prev, stream, offs, diff, diff_offs = clip_parts(c.geom, c.n, 0)
    _same_stream(got["stream"], got["offsets"], diff.tobytes(), diff_offs, "delta_levels")


def ref_undelta_levels(c, got):
    prev, stream, offs, diff, diff_offs = clip_parts(c.geom, c.n, 0)
    _same_stream(got["stream"], got["offsets"], *layers.undelta_frames(diff, diff_offs, key_flags(c.n), prev=prev), "undelta_levels")
    _same_stream(got["stream"], got["offsets"], stream.tobytes(), offs, "undelta_levels, against the frames the delta stream was made from")


REFERENCES = {"delta_levels": ref_delta_levels, "undelta_levels": ref_undelta_levels}


def test_the_tables_name_every_buffer(native):
    for entry, geom in PAIRS:
        c = Case(entry, geom, 3, A_OUT, IN_AT, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
        for k, g in c.pool.written.items():
            assert g.addr % (2 * A_OUT[k]) == A_OUT[k], (entry, k)
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * IN_AT[k]) == IN_AT[k], (entry, k)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_at_the_weakest_placement(native, entry, geom):
    for n in NS:
        aligned = Case(entry, geom, n, table=ENTRIES).run()
        c = Case(entry, geom, n, A_OUT, IN_AT, table=ENTRIES)
        got = c.run()
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", aligned, got, "differs from the same call on 256-byte aligned buffers")
        assert not findings, "\n".join(findings)
        assert got["status"].tolist() == [0] * n
        REFERENCES[entry](c, got)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_one_notch_below_is_refused(native, entry):
    n, geom = 3, GEOMS[0]
    probe = Case(entry, geom, n, A_OUT, IN_AT, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if A_OUT[k] > 1] + [("in", k) for k in probe.inputs if IN_AT[k] > 1]
    assert len(rows) == 8, rows  # four written buffers and four inputs each
    for side, name in rows:
        out_at = {**A_OUT, name: A_OUT[name] // 2} if side == "out" else A_OUT
        in_at = {**IN_AT, name: IN_AT[name] // 2} if side == "in" else IN_AT
        c = Case(entry, geom, n, out_at, in_at, table=ENTRIES)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(A_OUT if side == 'out' else IN_AT)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
