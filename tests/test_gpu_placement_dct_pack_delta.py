"""svc_hip_dct_pack_delta_frames at the weakest placement include/svc_hip.h admits, the way tests/test_gpu_placement_streams.py tests
the other stream entry points (its Case, with the builder of tests/test_gpu_guard_dct_pack_delta.py): every written buffer a Guarded
of exactly the asked size at gd.exactly(A), every input surrounded at exactly(A) -- frames, the frame before, output and workspace
16 bytes, offsets 8, region ids (the frame before's too) and key flags 4; the frame stride is a multiple of 16 and not of 32.  Per case
the guards are intact, every output is bit for bit that of the same call on 256-byte aligned buffers, and the stream is that of the two
device calls it replaces.  One notch below, each pointer alone at exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that
names alignment, and no byte of any output changes."""
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.test_gpu_guard_dct_pack_delta import ENTRIES, GEOMS, N, STEPS, key_flags
from tests.test_gpu_guard_streams import _bgr, _gid
from tests.test_gpu_placement_streams import A_IN, A_OUT, Case, _same_stream

pytestmark = pytest.mark.gpu

IN_AT = {**A_IN, "prev": 16, "prev types": 4, "key": 4}
ENTRY = "dct_pack_delta"


def _two_calls(geom, n):
    """svc_hip_dct_pack_levels_frames on the n + 1 frames, then svc_hip_delta_levels_frames on the last n with the first as d_prev."""
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n + 1, 0)
    out = torch.empty(nat.levels_max_bytes(n + 1, w, h, tile, mv), dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 2, dtype=torch.int64, device="cuda")
    ws = torch.empty(nat.dct_pack_levels_workspace_bytes(n + 1, w, h, tile[0], mv), dtype=torch.uint8, device="cuda")
    nat._check(nat.load().svc_hip_dct_pack_levels_frames(buf.data_ptr(), stride, n + 1, w, h, tile[0], types.data_ptr(), *mv, *STEPS,
                                                        ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), nat._stream()))
    o = offs.cpu().tolist()
    want, want_offs, st = nat.delta_levels_frames(out[o[1]:o[-1]], offs[1:] - o[1], w, h, tile, mv, prev=out[:o[1]].clone(), key=key_flags(n))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    return want[:int(want_offs[-1])].cpu().numpy().tobytes(), want_offs.cpu().tolist()


def test_the_tables_name_every_buffer_and_the_stride_is_the_weakest(native):
    for geom in GEOMS:
        c = Case(ENTRY, geom, N, A_OUT, IN_AT, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
        for k, g in c.pool.written.items():
            assert g.addr % (2 * A_OUT[k]) == A_OUT[k], k
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * IN_AT[k]) == IN_AT[k], k
        assert _bgr(geom, N + 1)[1] % 32 == 16, geom


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_at_the_weakest_placement(native, geom):
    aligned = Case(ENTRY, geom, N, table=ENTRIES).run()
    c = Case(ENTRY, geom, N, A_OUT, IN_AT, table=ENTRIES)
    got = c.run()
    findings = gd.output_findings(f"{ENTRY} {_gid(geom)} n={N}", aligned, got, "differs from the same call on 256-byte aligned buffers")
    assert not findings, "\n".join(findings)
    _same_stream(got["stream"], got["offsets"], *_two_calls(geom, N), ENTRY)


def test_one_notch_below_is_refused(native):
    geom = GEOMS[0]
    probe = Case(ENTRY, geom, N, A_OUT, IN_AT, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if A_OUT[k] > 1] + [("in", k) for k in probe.inputs if IN_AT[k] > 1]
    assert len(rows) == 8, rows  # three written buffers and five inputs
    for side, name in rows:
        out_at = {**A_OUT, name: A_OUT[name] // 2} if side == "out" else A_OUT
        in_at = {**IN_AT, name: IN_AT[name] // 2} if side == "in" else IN_AT
        c = Case(ENTRY, geom, N, out_at, in_at, table=ENTRIES)
        what = f"{ENTRY} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(A_OUT if side == 'out' else IN_AT)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
