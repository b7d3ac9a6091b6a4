"""The stream entry points at the weakest placement include/svc_hip.h admits (tests/helpers/guarded.py: exactly, Misplaced).

Every other GPU test hands these calls fresh allocations: 256-byte aligned.  The header promises less -- streams, frames, planes and
workspaces 16 bytes, offset arrays 8, region ids, windows, gaze, source indices, budgets, choices, status and rec 4 -- and the kernels
lean on exactly that: 64-bit counters carved out of a workspace, 16-byte loads of a stream, interleaved stores to rec.  Here every
buffer a call writes is a Guarded of exactly the size the API asks for at gd.exactly(A), A the pointer's documented alignment, and
every input is surrounded at exactly(A): a multiple of A and not of 2A.  The input builders and the call closures are those of
tests/test_gpu_guard_streams.py.  Per case:

 1. the guards of every written buffer are intact (and, where the closures check it, nothing past offsets[n] is written);
 2. every defined output is bit for bit that of the same call on 256-byte aligned buffers;
 3. the outputs are what the reference says: the numpy statements of levels.py, layers.py and entropy.py, exactly, for every call that
    reads or writes SVCQ / SVCE; tests/helpers/transform_ref.py's half-ulp intervals for what the float transforms and their inverses
    contribute, with the caps of tests/test_gpu_transform_exact.py computed from the reference before the kernel's output is looked at.

One notch below: each pointer argument alone at exactly(A / 2) is refused with SVC_ERR_INVALID_ARG and a message that names alignment,
and no byte of any output changes.
"""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers, levels
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.helpers import transform_ref as tr
from tests.test_gpu_decode_levels import _check_display
from tests.test_gpu_guard_streams import (DEC, ENC, FINE, G8, G16, GX, NS, REFUSED, STREAM, Pool, _bgr, _cuda, _gid, _stream_out, _svce,
                                          _svcq, _windows)
from tests.test_gpu_guard_streams import ENTRIES as GUARDED_ENTRIES
from tests.test_pack_layers_host import random_planes
from tests.test_gpu_transform_exact import _decode_steps, _requant
from tests.test_levels_budget_host import ladder, select
from tests.test_levels_host import write_frame
from tests.test_window_levels_host import geom_dict, random_types

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tr.available(), reason=tr.UNAVAILABLE)]

# the documented alignment of every pointer, by the name it has in tests/test_gpu_guard_streams.py (include/svc_hip.h: "frames, output and
# workspace 16-byte aligned, offsets 8-byte, types, budget, choice, windows, source indices, gaze, status and rec 4-byte")
A_OUT = {"workspace": 16, "stream": 16, "base": 16, "enhancement": 16, "planes": 16, "offsets": 8, "base offsets": 8, "enhancement offsets": 8,
         "status": 4, "choice": 4, "types": 4, "rec": 4, "display": 1}
A_IN = {"stream": 16, "base": 16, "enhancement": 16, "planes": 16, "bgr": 16, "offsets": 8, "base offsets": 8, "enhancement offsets": 8,
        "types": 4, "budget": 4, "window": 4, "gaze": 4, "src": 4}

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
A_OUT["destination"] = 16  # the drains' pinned host memory


# ---- the stream entry points tests/test_gpu_guard_streams.py has no closure for, in its closures' form ---------------------------------------

LAYER_STEPS = (4, 16, 2)
REDUCE = {8: 2, 16: 8}  # K = 4 and K = 2


def e_pack_layers(pool, geom, n, seed):
    """tests/test_gpu_pack_layers.py::test_against_the_numpy_statement's planes (seeded, with exact ties of the steps) and region ids."""
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + n + seed)
    planes = random_planes(rng, n, w, h, tile, 0.3, LAYER_STEPS)
    types = np.stack([random_types(rng, w, h, mv) for _ in range(n)]).astype(np.int32).reshape(n, -1)
    cap = nat.levels_max_bytes(n, w, h, tile, mv)
    ws = pool.buf("workspace", nat.pack_layers_workspace_bytes(n, w, h, tile), U8)
    base, boffs = pool.buf("base", cap, U8), pool.buf("base offsets", n + 1, I64)
    enh, eoffs = pool.buf("enhancement", cap, U8), pool.buf("enhancement offsets", n + 1, I64)

    def call(i):
        nat.pack_layers_frames(i["planes"], i["types"], tile, mv, *LAYER_STEPS, window=i["window"], base_out=base, enh_out=enh, workspace=ws,
                               base_offsets=boffs, enh_offsets=eoffs)
        return {"base": _stream_out(base, boffs), "base offsets": boffs, "enhancement": _stream_out(enh, eoffs), "enhancement offsets": eoffs}
    return {"planes": _cuda(planes), "types": _cuda(types), "window": _windows(n, w, h)}, call


def e_decode_levels_reduced(pool, geom, n, seed):
    w, h, tile, mv = geom
    reduce = REDUCE[tile[0]]
    q, qo = _svcq(geom, n, ENC, seed)
    rw, rh = w // reduce, h // reduce
    dw, dh = max(1, rw - 5), max(1, rh - 3)
    ws = pool.buf("workspace", nat.decode_levels_workspace_bytes(n, w, h, tile), U8)
    rec = pool.buf("rec", (n, rh, rw, 3), F32)
    disp = pool.buf("display", (n, dh, dw, 3), U8)
    status = pool.buf("status", n, I32)

    def call(i):
        nat._check(nat.load().svc_hip_decode_levels_reduced_frames(i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, w, h,
                                                                  *tile, *mv, *DEC, reduce, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(),
                                                                  rec.data_ptr(), disp.data_ptr(), dw, dh, status.data_ptr(), nat._stream()))
        return {"rec": rec, "display": disp, "status": status}
    return {"stream": _cuda(q), "offsets": _cuda(qo), "gaze": _windows(n, w, h)}, call


def _drain(entropy_coded):
    def build(pool, geom, n, seed):
        """The destination is page-locked host memory inside a Guarded of its own, of exactly the worst-case size."""
        w, h, tile, mv = geom
        s, so = _svce(geom, n, seed) if entropy_coded else _svcq(geom, n, ENC, seed)
        cap = (nat.entropy_max_bytes if entropy_coded else nat.levels_max_bytes)(n, w, h, tile, mv)
        kw = {} if pool.place is None else gd.exactly(pool.place["destination"])
        pool.written["destination"] = dst = gd.Guarded(cap, U8, "cpu", seed=9, pin=True, **kw)
        fn = nat.load().svc_hip_entropy_drain if entropy_coded else nat.load().svc_hip_levels_drain

        def call(i):
            nat._check(fn(i["stream"].data_ptr(), i["offsets"].data_ptr(), n, w, h, *tile, *mv, dst.addr, cap, nat._stream()))
            torch.cuda.synchronize()
            return {"destination": dst.bytes[:int(so[-1])]}
        return {"stream": _cuda(s), "offsets": _cuda(so)}, call
    return build


ENTRIES = {**GUARDED_ENTRIES, "pack_layers": (e_pack_layers, STREAM), "decode_levels_reduced": (e_decode_levels_reduced, G8 + G16),
           "levels_drain": (_drain(False), STREAM), "entropy_drain": (_drain(True), STREAM)}

GEOMS = (G8[1], G16[1], GX[2])  # one geometry per kernel form: 8 x 8, 16 x 16 and the general tiles
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in GEOMS if g in geoms and (e, g) not in REFUSED]


class Case:
    """One entry point on one geometry and frame count, its buffers placed by the two tables (None: 256-byte aligned)."""

    def __init__(self, entry, geom, n, out_at=None, in_at=None, table=None):
        self.entry, self.geom, self.n = entry, geom, n
        self.pool = Pool(out_at)
        self.inputs, self.call = (ENTRIES if table is None else table)[entry][0](self.pool, geom, n, 0)
        self.given = {k: gd.surround(v, 7) if in_at is None else gd.placed(v, 7, in_at[k]) for k, v in self.inputs.items()}
        self.fills = {}
        for i, (k, g) in enumerate(self.pool.written.items()):
            self.fills[k] = dict(gd.poisons(g.nbytes, 300 + i))["random"]
            g.fill(self.fills[k])

    def run(self):
        got = {k: v.detach().clone().cpu() for k, v in self.call(self.given).items()}
        torch.cuda.synchronize()
        findings = gd.guard_findings(f"{self.entry} {self.geom} n={self.n}", self.pool.written, "at this placement")
        assert not findings, "\n".join(findings)
        return got

    def untouched(self, what):
        """After a refused call: every written buffer holds its fill -- for a buffer that is input and output, its fill with the input the
        closure put there (pool.before_call, set by such a builder) -- and every guard is intact."""
        torch.cuda.synchronize()
        after = {k: g.bytes.cpu() for k, g in self.pool.written.items()}
        for k, g in self.pool.written.items():
            g.fill(self.fills[k])
        if getattr(self.pool, "before_call", None) is not None:
            self.pool.before_call()
            torch.cuda.synchronize()
        for k, g in self.pool.written.items():
            assert torch.equal(after[k], g.bytes.cpu()), f"{what}: a refused call wrote to '{k}'"
        assert not gd.guard_findings(what, self.pool.written, "in a refused call")


def test_the_tables_name_every_buffer_and_the_strides_are_the_weakest(native):
    for entry, geom in PAIRS:
        c = Case(entry, geom, 3, A_OUT, A_IN)  # a KeyError here: a buffer the tables do not know
        for k, g in c.pool.written.items():
            assert g.addr % (2 * A_OUT[k]) == A_OUT[k], (entry, k)
        for k, v in c.given.items():
            assert v.data_ptr() % (2 * A_IN[k]) == A_IN[k], (entry, k)
    for geom in (G8[1], G16[1]):  # the only stride these calls take: a multiple of 16 and not of 32
        for n in NS:
            assert _bgr(geom, n)[1] % 32 == 16, geom


# ---- the references ------------------------------------------------------------------------------------------------------------------------

def _u8(t):
    return t.numpy().tobytes()


def _frames_of(stream, offs):
    b, o = stream.numpy(), [int(v) for v in offs.numpy().astype(np.int64)]
    assert o[0] == 0 and all(x % 16 == 0 and y >= x for x, y in zip(o[:-1], o[1:])), o
    return [b[x:y] for x, y in zip(o[:-1], o[1:])]


def _same_stream(got, offs, want, want_offs, what):
    assert offs.numpy().astype(np.int64).tolist() == [int(v) for v in want_offs], f"{what}: offsets"
    assert _u8(got) == bytes(want), f"{what}: bytes"


def _rects(c, key):
    return c.inputs[key].cpu().numpy().view(np.uint32).reshape(c.n, 4).astype(np.int64)


def _source_frames(c):
    """(n, h, w, 3) u8: the frames of _bgr's strided buffer."""
    w, h = c.geom[:2]
    buf, stride, types = _bgr(c.geom, c.n, 0)
    b = buf.cpu().numpy()
    return np.stack([b[f * stride:f * stride + w * h * 3].reshape(h, w, 3) for f in range(c.n)]), types.cpu().numpy().view(np.uint32)


def _coefficient_bounds(c):
    """[lo, hi] of every transform coefficient of the case's frames (transform_ref: RN32(ref -+ A)), the raw cap asserted over the frames of
    random bytes -- the synthetic and the zero frames hold exact zeros and exact ties, where either neighbour is right."""
    frames, types = _source_frames(c)
    bw, bh = c.geom[2]
    a = tr.forward_slack(bw, bh)
    lo, hi = zip(*(tr.interval(tr.dct_ref(f, bw, bh), a) for f in frames))
    lo, hi = np.stack(lo), np.stack(hi)
    rnd = lo[0::3] != hi[0::3]
    assert rnd.mean() <= tr.RAW_AMBIGUOUS_CAP, f"raw ambiguous share {rnd.mean():.3e} on the random frames"
    return lo, hi, types


def _step_plane(geom, types, fg, bg):
    """(1, H, W) i64: the step of every coefficient, by the MV block that holds its tile's origin."""
    g = geom_dict(*geom)
    background, _, _ = layers._tile_maps(g, types.reshape(g["frame_h"] // g["mv_block_h"], g["frame_w"] // g["mv_block_w"]))
    return layers._per_pixel(g, np.where(background, bg, fg).astype(np.int64))[None]


def _quantised_bounds(c, lo, hi, types, f, fg, bg):
    """The two level planes the reference admits for frame f at (fg, bg), the quantised cap asserted on a frame of random bytes."""
    step = _step_plane(c.geom, types[f], fg, bg)
    qlo, qhi = layers.quantise(lo[f], step), layers.quantise(hi[f], step)
    if f % 3 == 0:
        assert (qlo != qhi).sum() <= tr.QUANT_AMBIGUOUS_CAP * qlo.size, f"frame {f}: {(qlo != qhi).sum()} ambiguous levels of {qlo.size}"
    return qlo, qhi, step


def _levels_in(frame, geom, types_want, fg, bg, what):
    """A frame the kernel wrote -> its levels (3, H, W) i64 and header; the frame must be the canonical writing of those levels
    (layers.write_frame: header, region ids, masks, levels in order, padding), word 11 (the inexact count) as it came."""
    hdr, types, planes = levels.parse_frame(frame)
    assert (hdr["fg_step"], hdr["bg_step"]) == (fg, bg), (what, hdr)
    assert np.array_equal(types.reshape(-1), types_want.reshape(-1)), f"{what}: region ids"
    lv, _ = layers._levels_of(hdr, types, planes)
    assert frame.tobytes() == layers.write_frame(geom_dict(*geom), types, lv, fg, bg, hdr["inexact"]), f"{what}: not the canonical frame of its levels"
    return lv, hdr


def _either(lv, qlo, qhi, what):
    bad = (lv != qlo) & (lv != qhi)
    assert not bad.any(), f"{what}: {int(bad.sum())} levels are neither quantise(lo) nor quantise(hi), first at {tuple(np.argwhere(bad)[0])}"


def ref_pack_levels(c, got, oracle):
    pass  # the closure compares the stream with layers.write_frame's frames, for this very call


ref_entropy_decode = ref_pack_levels  # the closure compares with the SVCQ frames the SVCE ones were coded from


def ref_unpack_levels(c, got, oracle):
    q, qo = _svcq(c.geom, c.n, ENC, 0)
    assert got["status"].tolist() == [0] * c.n
    for f, (_, types, planes) in enumerate(levels.iter_frames(q, qo)):
        assert np.array_equal(got["types"][f].numpy().view(np.uint32), types.reshape(-1)), f
        assert np.array_equal(got["planes"][f].numpy(), planes), f


def ref_entropy_encode(c, got, oracle):
    q, qo = _svcq(c.geom, c.n, ENC, 0)
    assert got["status"].tolist() == [0] * c.n
    _same_stream(got["stream"], got["offsets"], *entropy.encode_frames(q, qo.astype(np.uint64)), "entropy_encode")


def ref_window_levels(c, got, oracle):
    assert got["status"].tolist() == [0] * c.n
    _same_stream(got["stream"], got["offsets"], *layers.window_frames(*_svcq(c.geom, c.n, ENC, 0), _rects(c, "window")), "window_levels")


def ref_window_entropy(c, got, oracle):
    assert got["status"].tolist() == [0] * c.n
    _same_stream(got["stream"], got["offsets"], *entropy.window_frames(*_svce(c.geom, c.n, 0), _rects(c, "window")), "window_entropy")


def ref_split_levels(c, got, oracle):
    q, qo = _svcq(c.geom, c.n, (FINE, FINE), 0)
    base, bo, enh, eo = layers.split_frames(q, qo, FINE, 4, 16, _rects(c, "window"))
    assert got["status"].tolist() == [0] * c.n
    _same_stream(got["base"], got["base offsets"], base, bo, "split_levels base")
    _same_stream(got["enhancement"], got["enhancement offsets"], enh, eo, "split_levels enhancement")


def ref_split_levels_budget(c, got, oracle):
    q, qo = _svcq(c.geom, c.n, (FINE, FINE), 0)
    lad = [(int(fg) * FINE, int(bg) * FINE) for fg, bg in ladder(8)]
    budget = c.inputs["budget"].cpu().numpy().view(np.uint32).astype(np.int64)
    base, bo, enh, eo, choice = layers.split_budget_frames(q, qo, FINE, lad, budget, _rects(c, "window"))
    assert got["status"].tolist() == [0] * c.n
    assert got["choice"].numpy().view(np.uint32).tolist() == choice.tolist()
    _same_stream(got["base"], got["base offsets"], base, bo, "split_levels_budget base")
    _same_stream(got["enhancement"], got["enhancement offsets"], enh, eo, "split_levels_budget enhancement")


def ref_pack_levels_budget(c, got, oracle):
    """The raw planes are this call's input: the choice is the reference's, every frame the independent writer's at its chosen steps."""
    w, h, tile, mv = c.geom
    p, t = c.inputs["planes"].cpu().numpy(), c.inputs["types"].cpu().numpy().view(np.uint32)
    lad = ladder(8)
    budget = c.inputs["budget"].cpu().numpy().view(np.uint32).astype(np.int64)
    choice = select(p, t, *tile, *mv, lad, budget)
    assert got["choice"].numpy().view(np.uint32).tolist() == choice.tolist()
    frames = [write_frame(p[f], t[f], *tile, *mv, *(int(v) for v in lad[choice[f] & 0x7FFFFFFF])) for f in range(c.n)]
    _same_stream(got["stream"], got["offsets"], b"".join(frames), np.concatenate([[0], np.cumsum([len(x) for x in frames])]), "pack_levels_budget")


def _check_fused_frame(c, frame, lo, hi, types, f, fg, bg, what):
    qlo, qhi, _ = _quantised_bounds(c, lo, hi, types, f, fg, bg)
    lv, hdr = _levels_in(frame, c.geom, types[f], fg, bg, what)
    _either(lv, qlo, qhi, what)
    assert hdr["inexact"] == 0, what  # include/svc_hip.h: the fused forms write header word 11 as 0
    return lv


def ref_dct_pack_levels(c, got, oracle):
    lo, hi, types = _coefficient_bounds(c)
    for f, frame in enumerate(_frames_of(got["stream"], got["offsets"])):
        _check_fused_frame(c, frame, lo, hi, types, f, 1, 1, f"dct_pack_levels frame {f}")


def ref_dct_pack_levels_budget(c, got, oracle):
    """The choice is the reference's on either end of the coefficients' intervals; the frame is the fixed form's at the chosen steps."""
    w, h, tile, mv = c.geom
    lo, hi, types = _coefficient_bounds(c)
    lad = ladder(8)
    budget = c.inputs["budget"].cpu().numpy().view(np.uint32).astype(np.int64)
    admitted = [set(int(v) for v in pair) for pair in zip(select(lo, types, *tile, *mv, lad, budget), select(hi, types, *tile, *mv, lad, budget))]
    assert all(len(a) == 1 for a in admitted[0::3]), "the reference's choice must not be ambiguous on the frames of random bytes"
    choice = got["choice"].numpy().view(np.uint32)
    for f, frame in enumerate(_frames_of(got["stream"], got["offsets"])):
        assert int(choice[f]) in admitted[f], (f, int(choice[f]), admitted[f])
        fg, bg = (int(v) for v in lad[int(choice[f]) & 0x7FFFFFFF])
        _check_fused_frame(c, frame, lo, hi, types, f, fg, bg, f"dct_pack_levels_budget frame {f}")
        assert bool(choice[f] >> 31) == (len(frame) > budget[f]), (f, len(frame), budget[f])


def ref_dct_pack_layers(c, got, oracle):
    """layers.pack_layers_frames on coefficients known to an interval: Lb at the base steps and Lf = Lb * ratio + d at the enhancement's,
    each one of the two levels the interval admits; d is zero outside the window."""
    lo, hi, types = _coefficient_bounds(c)
    g = geom_dict(*c.geom)
    win = _rects(c, "window")
    pairs = zip(_frames_of(got["base"], got["base offsets"]), _frames_of(got["enhancement"], got["enhancement offsets"]))
    for f, (base, enh) in enumerate(pairs):
        lb = _check_fused_frame(c, base, lo, hi, types, f, 4, 16, f"dct_pack_layers base frame {f}")
        d, _ = _levels_in(enh, c.geom, types[f], 1, 1, f"dct_pack_layers enhancement frame {f}")
        _, ox, oy = layers._tile_maps(g, types[f].reshape(g["frame_h"] // g["mv_block_h"], g["frame_w"] // g["mv_block_w"]))
        inside = layers._per_pixel(g, layers._contains(win[f], ox, oy))[None]
        assert not d[np.broadcast_to(~inside, d.shape)].any(), f"frame {f}: residuals outside the window"
        qlo, qhi, _ = _quantised_bounds(c, lo, hi, types, f, 1, 1)
        fine = lb * _step_plane(c.geom, types[f], 4, 16) + d
        m = np.broadcast_to(inside, d.shape)
        _either(fine[m], qlo[m], qhi[m], f"dct_pack_layers frame {f}, base * ratio + d")


def _check_rec(c, got, coeffs_of, oracle):
    """rec against the long double inverse of the requantised coefficients (tests/test_gpu_transform_exact.py::test_decode_frames), the raw cap
    from the reference first; display against the f64 statement of its resize (tests/test_gpu_decode_levels.py)."""
    w, h, tile, mv = c.geom
    assert tile[0] == tile[1] and mv[0] == mv[1]
    gaze = _rects(c, "gaze")
    assert got["status"].tolist() == [0] * c.n
    bounds, amb, tot = [], 0, 0
    for f in range(c.n):
        coeffs, types = coeffs_of(f)
        q = _requant(oracle, coeffs, _decode_steps(types.reshape(-1), w, h, tile[0], mv[0], *DEC, tuple(int(v) for v in gaze[f])))
        rlo, rhi = tr.interval(tr.idct_ref(q, *tile), tr.inverse_slack(q, *tile))
        bounds.append((rlo, rhi))
        amb, tot = amb + int((rlo != rhi).sum()), tot + rlo.size
    assert amb <= tr.RAW_AMBIGUOUS_CAP * tot, f"raw ambiguous share {amb / tot:.3e}"
    dh, dw = got["display"].shape[1:3]
    for f, (rlo, rhi) in enumerate(bounds):
        rec = got["rec"][f].numpy()
        bad = tr.raw_violations(rec.transpose(2, 0, 1), rlo, rhi)
        assert not bad.any(), f"{c.entry} frame {f}: {int(bad.sum())} pixels outside [RN32(ref - A'), RN32(ref + A')]"
        _check_display(rec, got["display"][f].numpy(), dw, dh)


def _svcq_coeffs(c):
    q, qo = _svcq(c.geom, c.n, ENC, 0)
    frames = [(planes, types) for _, types, planes in levels.iter_frames(q, qo)]
    return lambda f: frames[f]


def ref_decode_levels(c, got, oracle):
    _check_rec(c, got, _svcq_coeffs(c), oracle)


ref_decode_entropy = ref_decode_levels  # the same frames, entropy-coded


def ref_decode_layers(c, got, oracle):
    """layers.merge_levels: inside the gaze the enhancement's levels at its step, elsewhere the base's at theirs."""
    g = geom_dict(*c.geom)
    base = _frames_of(c.inputs["base"].cpu(), c.inputs["base offsets"].cpu())
    enh = _frames_of(c.inputs["enhancement"].cpu(), c.inputs["enhancement offsets"].cpu())
    gaze = _rects(c, "gaze")

    def coeffs_of(f):
        lv, step = layers.merge_levels(base[f], enh[f], gaze[f])
        _, types, _ = levels.parse_frame(base[f])
        return (lv * layers._per_pixel(g, step)[None]).astype(np.float32), types
    _check_rec(c, got, coeffs_of, oracle)


def ref_pack_layers(c, got, oracle):
    want = layers.pack_layers_frames(c.inputs["planes"].cpu().numpy(), c.inputs["types"].cpu().numpy().view(np.uint32), geom_dict(*c.geom),
                                     *LAYER_STEPS, _rects(c, "window"))
    _same_stream(got["base"], got["base offsets"], want[0], want[1], "pack_layers base")
    _same_stream(got["enhancement"], got["enhancement offsets"], want[2], want[3], "pack_layers enhancement")


def ref_decode_levels_reduced(c, got, oracle):
    """tests/test_gpu_decode_reduced.py::test_rec_is_within_half_an_ulp: the K x K inverse of levels.reduced_coefficients in long double."""
    w, h, tile, mv = c.geom
    reduce = REDUCE[tile[0]]
    k = tile[0] // reduce
    q, qo = _svcq(c.geom, c.n, ENC, 0)
    gaze = _rects(c, "gaze")
    bounds = []
    for f in range(c.n):
        coef = levels.reduced_coefficients(q[int(qo[f]):int(qo[f + 1])], reduce, *DEC, gaze=tuple(int(v) for v in gaze[f]))
        bounds.append(tr.interval(tr.idct_ref(coef, k, k), tr.inverse_slack(coef, k, k)))
    ambiguous = float(np.mean([np.mean(lo != hi) for lo, hi in bounds]))
    assert ambiguous <= tr.RAW_AMBIGUOUS_CAP, ambiguous
    assert got["status"].tolist() == [0] * c.n
    dh, dw = got["display"].shape[1:3]
    for f, (lo, hi) in enumerate(bounds):
        rec = got["rec"][f].numpy()
        bad = tr.raw_violations(rec.transpose(2, 0, 1), lo, hi)
        assert not bad.any(), (f, int(bad.sum()))
        _check_display(rec, got["display"][f].numpy(), dw, dh)


def ref_levels_drain(c, got, oracle):
    q, qo = _svcq(c.geom, c.n, ENC, 0)
    assert _u8(got["destination"]) == q[:int(qo[-1])].tobytes()
    dst = c.pool.written["destination"]  # past the stream's 16-byte units the destination keeps what it held
    used = (int(qo[-1]) + 15) // 16 * 16
    assert torch.equal(dst.bytes[used:], c.fills["destination"][used:])


def ref_entropy_drain(c, got, oracle):
    e, eo = _svce(c.geom, c.n, 0)
    assert _u8(got["destination"]) == e[:int(eo[-1])].tobytes()
    dst = c.pool.written["destination"]
    used = (int(eo[-1]) + 15) // 16 * 16
    assert torch.equal(dst.bytes[used:], c.fills["destination"][used:])


REFERENCES = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("ref_")}
assert sorted(REFERENCES) == sorted(ENTRIES)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_at_the_weakest_placement(native, oracle, entry, geom):
    for n in NS:
        aligned = Case(entry, geom, n).run()
        c = Case(entry, geom, n, A_OUT, A_IN)
        got = c.run()
        findings = gd.output_findings(f"{entry} {_gid(geom)} n={n}", aligned, got, "differs from the same call on 256-byte aligned buffers")
        assert not findings, "\n".join(findings)
        REFERENCES[entry](c, got, oracle)


# ---- one notch below -----------------------------------------------------------------------------------------------------------------------

def _notches():
    """(entry point, geometry, "out" / "in", the pointer's name): every pointer argument with a documented alignment above 1."""
    rows = []
    for entry, (_, geoms) in ENTRIES.items():
        geom = next(g for g in GEOMS if g in geoms and (entry, g) not in REFUSED)
        rows.append((entry, geom))
    return rows


@pytest.mark.parametrize("entry,geom", _notches(), ids=[e for e, _ in _notches()])
def test_one_notch_below_is_refused(native, entry, geom):
    n = 3
    probe = Case(entry, geom, n, A_OUT, A_IN)
    rows = [("out", k) for k in probe.pool.written if A_OUT[k] > 1] + [("in", k) for k in probe.inputs if A_IN[k] > 1]
    assert len(rows) >= 3, rows
    for side, name in rows:
        out_at = {**A_OUT, name: A_OUT[name] // 2} if side == "out" else A_OUT
        in_at = {**A_IN, name: A_IN[name] // 2} if side == "in" else A_IN
        c = Case(entry, geom, n, out_at, in_at)
        what = f"{entry} {_gid(geom)} with {'output' if side == 'out' else 'input'} '{name}' at exactly({(A_OUT if side == 'out' else A_IN)[name] // 2})"
        with pytest.raises(nat.SvcError) as e:
            c.call(c.given)
        assert e.value.status == nat.SVC_ERR_INVALID_ARG and "align" in str(e.value), (what, e.value)
        c.untouched(what)
