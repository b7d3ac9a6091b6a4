"""svc_hip_decode_layers_reduced_frames at the weakest placement include/svc_hip.h admits, the way tests/test_gpu_placement_band.py tests
the band call (the Case of tests/test_gpu_placement_streams.py): every written buffer a Guarded of exactly the asked size at
gd.exactly(A), every input surrounded at exactly(A) -- both streams and the workspace 16 bytes, both offset arrays 8, rec, gaze and
status 4.  Per case the guards are intact, every output is bit for bit that of the same call on 256-byte aligned buffers, and rec lies
within half an ulp of the numpy statement (layers.reduced_coefficients), the display on it.  One notch below, each pointer alone at
exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that names alignment, and no byte of any output changes."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.helpers import transform_ref as tr
from tests.test_gpu_decode_levels import _check_display
from tests.test_gpu_guard_streams import DEC, G8, G16, NS, _cuda, _gid, _windows
from tests.test_gpu_placement_streams import A_IN, A_OUT, LAYER_STEPS, REDUCE, Case, _frames_of, _rects
from tests.test_pack_layers_host import random_planes
from tests.test_window_levels_host import geom_dict, random_types

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tr.available(), reason=tr.UNAVAILABLE)]

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
ENTRY = "decode_layers_reduced"
GEOMS = (G8[0], G8[1], G16[0])  # 8 x 8: a full wave plus a one-column wave, and masks only 4-byte aligned; 16 x 16: nine tiles a row


def e_decode_layers_reduced(pool, geom, n, seed):
    """Both layers from the numpy statement (layers.pack_layers_frames on seeded planes with exact ties of the steps), the enhancement
    for a window whose edges fall inside tiles."""
    w, h, tile, mv = geom
    reduce = REDUCE[tile[0]]
    rng = np.random.default_rng(w * 7 + h + n + seed)
    planes = random_planes(rng, n, w, h, tile, 0.3, LAYER_STEPS)
    types = np.stack([random_types(rng, w, h, mv) for _ in range(n)])
    base, bo, enh, eo, _ = layers.pack_layers_frames(planes, types, geom_dict(*geom), *LAYER_STEPS, [(tile[0] // 2, 1, w // 2, h)] * n)
    rw, rh = w // reduce, h // reduce
    dw, dh = max(1, rw - 5), max(1, rh - 3)
    ws = pool.buf("workspace", nat.decode_layers_reduced_workspace_bytes(n, w, h, tile), U8)
    rec = pool.buf("rec", (n, rh, rw, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)
    status = pool.buf("status", n, I32)

    def call(i):
        nat._check(nat.load().svc_hip_decode_layers_reduced_frames(
            i["base"].data_ptr(), i["base"].numel(), i["base offsets"].data_ptr(), i["enhancement"].data_ptr(), i["enhancement"].numel(),
            i["enhancement offsets"].data_ptr(), n, w, h, *tile, *mv, *DEC, reduce, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(),
            rec.data_ptr(), disp.data_ptr(), dw, dh, status.data_ptr(), nat._stream()))
        return {"rec": rec, "display": disp, "status": status}
    return {"base": _cuda(np.frombuffer(base, np.uint8).copy()), "base offsets": _cuda(bo.astype(np.int64)),
            "enhancement": _cuda(np.frombuffer(enh, np.uint8).copy()), "enhancement offsets": _cuda(eo.astype(np.int64)),
            "gaze": _windows(n, w, h)}, call


ENTRIES = {ENTRY: (e_decode_layers_reduced, GEOMS)}


def _reference(c, got):
    """tests/test_gpu_decode_layers_reduced.py::test_rec_is_within_half_an_ulp on the case's inputs."""
    w, h, tile, mv = c.geom
    reduce = REDUCE[tile[0]]
    k = tile[0] // reduce
    base = _frames_of(c.inputs["base"].cpu(), c.inputs["base offsets"].cpu())
    enh = _frames_of(c.inputs["enhancement"].cpu(), c.inputs["enhancement offsets"].cpu())
    gaze = _rects(c, "gaze")
    bounds, lifted = [], False
    for f in range(c.n):
        rect = tuple(int(v) for v in gaze[f])
        coef = layers.reduced_coefficients(base[f], enh[f], reduce, *DEC, gaze=rect)
        lifted |= not np.array_equal(coef, layers.reduced_coefficients(base[f], None, reduce, *DEC))
        bounds.append(tr.interval(tr.idct_ref(coef, k, k), tr.inverse_slack(coef, k, k)))
    ambiguous = float(np.mean([np.mean(lo != hi) for lo, hi in bounds]))
    assert ambiguous <= tr.RAW_AMBIGUOUS_CAP, ambiguous  # from the reference alone
    assert lifted or c.n < 3  # from three frames on the gaze cycle holds the whole frame: the enhancement is in what is compared
    assert got["status"].tolist() == [0] * c.n
    dh, dw = got["display"].shape[1:3]
    for f, (lo, hi) in enumerate(bounds):
        rec = got["rec"][f].numpy()
        bad = tr.raw_violations(rec.transpose(2, 0, 1), lo, hi)
        assert not bad.any(), (f, int(bad.sum()))
        _check_display(rec, got["display"][f].numpy(), dw, dh)


def test_the_tables_name_every_buffer(native):
    for geom in GEOMS:
        c = Case(ENTRY, geom, 3, A_OUT, A_IN, table=ENTRIES)  # a KeyError here: a buffer the tables do not know
        assert sorted(c.pool.written) == ["display", "rec", "status", "workspace"]
        assert sorted(c.given) == ["base", "base offsets", "enhancement", "enhancement offsets", "gaze"]
        for k, g in c.pool.written.items():
            assert g.addr % (2 * A_OUT[k]) == A_OUT[k], k
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * A_IN[k]) == A_IN[k], k


@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_at_the_weakest_placement(native, geom):
    for n in NS:
        aligned = Case(ENTRY, geom, n, table=ENTRIES).run()
        c = Case(ENTRY, geom, n, A_OUT, A_IN, table=ENTRIES)
        got = c.run()
        findings = gd.output_findings(f"{ENTRY} {_gid(geom)} n={n}", aligned, got, "differs from the same call on 256-byte aligned buffers")
        assert not findings, "\n".join(findings)
        _reference(c, got)


def test_one_notch_below_is_refused(native):
    n, geom = 3, GEOMS[1]
    probe = Case(ENTRY, geom, n, A_OUT, A_IN, table=ENTRIES)
    rows = [("out", k) for k in probe.pool.written if A_OUT[k] > 1] + [("in", k) for k in probe.inputs if A_IN[k] > 1]
    assert len(rows) == 8, rows  # workspace, rec and status; both streams, both offset arrays and the gaze
    for side, name in rows:
        out_at = {**A_OUT, name: A_OUT[name] // 2} if side == "out" else A_OUT
        in_at = {**A_IN, name: A_IN[name] // 2} if side == "in" else A_IN
        c = Case(ENTRY, geom, n, out_at, in_at, table=ENTRIES)
        what = f"{ENTRY} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(A_OUT if side == 'out' else A_IN)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
