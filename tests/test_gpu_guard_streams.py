"""Where the workspace entry points write, and whether their results depend on memory they were never given (tests/helpers/guarded.py).

For every entry point that takes a caller-sized d_workspace, at the shapes where an index of the stream kernels can go wrong:
every buffer the call writes is a Guarded of EXACTLY the size the API asks for (the workspace exactly *_workspace_bytes, a stream
exactly *_max_bytes, offsets n + 1, status and choice n, planes / rec / display exact), and

 1. the guards of every written buffer are intact after every call;
 2. the defined outputs (the stream up to offsets[n], all n + 1 offsets, status, choice, rec, display, planes, types) are bit for bit
    the same whether the written buffers held zeros, 0xFF, random bytes or what a call on another frame count and a call of
    another entry point on the same workspace left there;
 3. the outputs are the same when other bytes lie next to each input (one input at a time, so that a finding names it).

What each of these calls computes is pinned elsewhere, with the same input builders: the fused forms in tests/test_gpu_dct_pack.py,
test_gpu_dct_pack_budget.py and test_gpu_layers.py (_content / _mixed, _types, frames given with a stride), the pack and the coder in
tests/test_gpu_levels.py and test_gpu_entropy.py, the decoders in tests/test_gpu_decode_levels.py and test_gpu_decode_entropy.py, the
window and split calls in tests/test_gpu_window_levels.py, test_gpu_window_entropy.py and test_gpu_split_levels.py (host-built frames
of layers.write_frame, densities 1 / 0.3 / 0, _rects' window cycle, d_src), segmentation in tests/test_gpu_segment.py, the redo in
tests/test_gpu_transform_exact.py, the exhaustive global search in tests/test_gpu_global_motion.py.  Every comparison here is exact.

svc_hip_decode_records_frames takes no workspace: its outputs are guarded in tests/test_gpu_guard_step.py.
"""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import entropy, layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded as gd
from tests.helpers import transform_inputs as ti
from tests.test_gpu_dct_pack import MV16, _types
from tests.test_gpu_dct_pack_budget import _mixed
from tests.test_gpu_decode_levels import _rects
from tests.test_levels_budget_host import frame_bytes, frame_floor, ladder
from tests.test_window_levels_host import geom_dict, random_levels, random_types

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
NS = (1, 3, 5)  # [n] u32 arrays of 4, 12, 20 bytes and [n + 1] u64 arrays of 16, 32, 48: the 16-byte rounding between arrays; odd [n][2]

# (w, h, tile, MV block)
G8 = [(272, 24, (8, 8), (16, 8)),    # a full wave plus a one-column wave per tile row
      (48, 16, (8, 8), MV16),        # three MV blocks: the masks are only 4-byte aligned
      (16, 8, (8, 8), (16, 8))]      # one workgroup spans three frames
G16 = [(144, 48, (16, 16), MV16), (16, 16, (16, 16), MV16)]
GX = [(264, 16, (8, 8), (8, 8)),     # 33 tiles a row: two chunks, the second of one tile
      (48, 64, (8, 16), MV16),
      (66, 48, (6, 6), (6, 6))]
FUSED = G8 + G16        # the fused transform forms: 8 x 8 and 16 x 16 tiles on widths that are multiples of 16
STREAM = G8 + G16 + GX  # the coders and the entry points that only read or write SVCQ / SVCE

ENC = (4, 16)  # the steps of the host-built frames
FINE = 2       # the step of the fine frames the split calls read
DEC = (3, 17)  # the decoders' steps


def _gid(g):
    return f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}-mv{g[3][0]}x{g[3][1]}"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Pool:
    """The buffers one case writes: first a Guarded of exactly the asked size each; then (reuse) views of the same interiors for the
    call that dirties them.  A borrowed buffer is another pool's Guarded, used through a view from the start."""

    def __init__(self, place=None):
        """place: None (every buffer 256-byte aligned), or name -> A: the buffer lies at gd.exactly(A).  An A that is no multiple of
        the element size (a pointer one notch below its contract) gives a gd.Misplaced: for calls that refuse it."""
        self.written, self.reuse, self.borrowed, self.place = {}, False, set(), place

    def buf(self, name, shape, dtype):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape)) * item
        if not self.reuse and name not in self.borrowed:
            assert name not in self.written
            if self.place is not None and self.place[name] % item:
                m = gd.Misplaced(torch.empty(shape, dtype=dtype, device="cuda"), len(self.written), **gd.exactly(self.place[name]))
                self.written[name] = m.guarded
                return m
            kw = {} if self.place is None else gd.exactly(self.place[name])
            self.written[name] = gd.Guarded(nbytes, dtype, "cuda", seed=len(self.written), shape=shape, **kw)
            return self.written[name].interior
        g = self.written[name]
        assert nbytes <= g.nbytes, (name, nbytes, g.nbytes)
        return g.bytes[:nbytes].view(dtype).view(shape)


# ---- inputs, built once ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _svcq(geom, n, steps=ENC, seed=0):
    """n host-built SVCQ frames (layers.write_frame, as tests/test_window_levels_host.py builds them): white noise (every level set:
    the dense path, raw chunks, the largest frame), an in-between frame, a zero frame (the smallest), and again.
    -> (bytes, offsets (n + 1,) i64 array)"""
    w, h, tile, mv = geom
    rng = np.random.default_rng(1000 * w + 10 * h + n + seed)
    frames = [layers.write_frame(geom_dict(*geom), random_types(rng, w, h, mv), random_levels(rng, w, h, (1.0, 0.3, 0.0)[f % 3]), *steps)
              for f in range(n)]
    stream, offs = entropy._join(frames)
    return np.frombuffer(stream, np.uint8).copy(), np.asarray(offs).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _svce(geom, n, seed=0, chunk_tiles=None):
    """The SVCE coding of _svcq's frames: by the GPU coder (tests/test_gpu_entropy.py pins it to the numpy coder), or by the numpy coder
    where the header is to say another chunk_tiles (test_gpu_decoder_honours_any_chunk_tiles)."""
    w, h, tile, mv = geom
    q, qo = _svcq(geom, n, ENC, seed)
    if chunk_tiles is None:
        e, eo, st = nat.entropy_encode_frames(_cuda(q), _cuda(qo), w, h, tile, mv)
        assert st.cpu().tolist() == [0] * n
        eo = eo.cpu().numpy()
        e = e[:int(eo[-1])].cpu().numpy()
    else:
        e, eo = entropy.encode_frames(q, qo.astype(np.uint64), chunk_tiles=chunk_tiles)
        assert entropy.parse_frame(e)[0]["chunk_tiles"] == chunk_tiles
        e, eo = np.frombuffer(e, np.uint8).copy(), np.asarray(eo).astype(np.int64)
    return e, eo


def _given(damage, build):
    """The stream a case reads: build()'s, or the damaged one of a malformed-input case.  damage = (bytes, offsets, the frames that must
    be refused)."""
    if damage is None:
        return build()
    return np.frombuffer(bytes(damage[0]), np.uint8).copy(), np.asarray(damage[1]).astype(np.int64)


def _statuses(status, n, damage):
    """Exactly the damaged frames are refused (which code each gets is pinned by the tests the damage comes from)."""
    st = status.cpu().tolist()
    assert [f for f in range(n) if st[f]] == sorted(() if damage is None else damage[2]), (st, None if damage is None else damage[2])
    return st


@functools.lru_cache(maxsize=None)
def _bgr(geom, n, seed=0):
    """_mixed of tests/test_gpu_dct_pack_budget.py (a random, a synthetic, a zero frame, and again) in a flat buffer with 48 bytes of noise
    between the frames, as _strided gives them; the last frame ends where the buffer ends.  -> (flat u8 on the device, stride, types)"""
    w, h, tile, mv = geom
    frames = _mixed(n, w, h, 7 * w + h + n + seed)
    per, extra = w * h * 3, 48
    g = torch.Generator(device="cuda").manual_seed(n + seed)
    buf = torch.randint(0, 256, (n * (per + extra) - extra,), dtype=U8, device="cuda", generator=g)
    for f in range(n):
        buf[f * (per + extra):f * (per + extra) + per] = frames[f].reshape(-1)
    return buf, per + extra, _types("random", n, w, h, mv, w + n + seed)


def _raw_planes(buf, stride, n, w, h, block):
    planes = torch.empty((n, 3, h, w), dtype=F32, device="cuda")
    nat._check(nat.load().svc_hip_dct_frames(buf.data_ptr(), stride, n, w, h, block[0], block[1], planes.data_ptr(), nat._stream()))
    return planes


def _budgets(planes, types, tile, mv, lad):
    """Per frame the size of another ladder entry (so the frames of one batch pick different entries, as _mixed_budgets arranges), the
    last frame of a batch below the masks' floor."""
    p, t = planes.cpu().numpy(), types.cpu().numpy().view(np.uint32)
    n, _, h, w = p.shape
    out = [int(frame_bytes(p[f], t[f], tile[0], tile[1], mv[0], mv[1], lad)[(3 * f + len(lad) // 2) % len(lad)]) for f in range(n)]
    if n > 1:
        out[-1] = frame_floor(w, h, tile[0], tile[1], mv[0], mv[1]) - 16
    return nat.budget_tensor(out, n, "cuda")


def _windows(n, w, h, given=None):
    """_rects' cycle of tests/test_gpu_decode_levels.py, entered at its last entry: the last tile, the empty window, the whole frame, then
    its rectangles -- so one frame gets the last tile, two the last tile and the empty window, three and more all three.  given: the
    windows of a malformed-input case instead."""
    rects = [_rects(6, w, h)[(5 + i) % 6] for i in range(n)] if given is None else given
    return _cuda(np.asarray(rects, dtype=np.uint32).view(np.int32).reshape(n, 4))


def _stream_out(out, offs):
    return out[:max(0, min(int(offs[-1]), out.numel()))]


def _past(what, *pairs):
    """For the calls whose own tests promise it (their FILL checks): nothing is written between offsets[n] and the capacity.
    pairs: (stream buffer, its offsets, a copy of the buffer from before the call)."""
    for out, offs, before in pairs:
        used = _stream_out(out, offs).numel()
        changed = int((out[used:] != before[used:]).sum())
        assert changed == 0, f"{what}: {changed} bytes past offsets[n] were written"


# ---- the entry points: each -> (inputs by name, call(inputs) -> defined outputs by name), its written buffers taken from the pool ----------

def e_pack_levels(pool, geom, n, seed):
    # the planes the GPU unpack gives for host-built frames (tests/test_gpu_levels.py); their pack is those frames again
    w, h, tile, mv = geom
    q, qo = _svcq(geom, n, ENC, seed)
    planes, types, st = nat.unpack_levels_frames(_cuda(q), _cuda(qo), w, h, tile, mv)
    assert st.cpu().tolist() == [0] * n
    ws = pool.buf("workspace", nat.pack_levels_workspace_bytes(n, w, h, tile), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)

    def call(i):
        nat.pack_levels_frames(i["planes"], i["types"], tile, mv, *ENC, out=out, offsets=offs, workspace=ws)
        got = _stream_out(out, offs)
        assert got.cpu().numpy().tobytes() == q.tobytes() and offs.cpu().tolist() == qo.tolist()  # the pin, for this very call
        return {"stream": got, "offsets": offs}
    return {"planes": planes, "types": types}, call


def e_unpack_levels(pool, geom, n, seed, damage=None):
    w, h, tile, mv = geom
    q, qo = _given(damage, lambda: _svcq(geom, n, ENC, seed))
    ws = pool.buf("workspace", nat.pack_levels_workspace_bytes(n, w, h, tile), U8)
    planes = pool.buf("planes", (n, 3, h, w), F32)
    types = pool.buf("types", (n, (w // mv[0]) * (h // mv[1])), I32)
    status = pool.buf("status", n, I32)

    def call(i):
        nat._check(nat.load().svc_hip_unpack_levels_frames(i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, w, h, *tile,
                                                          *mv, ws.data_ptr(), ws.numel(), planes.data_ptr(), types.data_ptr(),
                                                          status.data_ptr(), nat._stream()))
        st = _statuses(status, n, damage)
        ok = [f for f in range(n) if st[f] == 0]  # the planes and types of a refused frame are not defined
        return {"planes": planes[ok], "types": types[ok], "status": status}
    return {"stream": _cuda(q), "offsets": _cuda(qo)}, call


def e_pack_levels_budget(pool, geom, n, seed, k=8):
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n, seed)
    planes = _raw_planes(buf, stride, n, w, h, tile)
    lad = ladder(k)
    budget = _budgets(planes, types, tile, mv, lad)
    ws = pool.buf("workspace", nat.pack_levels_budget_workspace_bytes(n, w, h, tile, k), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    choice = pool.buf("choice", n, I32)

    def call(i):
        nat.pack_levels_budget_frames(i["planes"], i["types"], tile, mv, lad, i["budget"], out=out, offsets=offs, workspace=ws, choice=choice)
        return {"stream": _stream_out(out, offs), "offsets": offs, "choice": choice}
    return {"planes": planes, "types": types, "budget": budget}, call


def e_dct_pack_levels(pool, geom, n, seed):
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n, seed)
    ws = pool.buf("workspace", nat.dct_pack_levels_workspace_bytes(n, w, h, tile[0], mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)

    def call(i):
        before = out.clone()
        nat._check(nat.load().svc_hip_dct_pack_levels_frames(i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, 1, 1,
                                                            ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                                                            nat._stream()))
        _past("dct_pack_levels", (out, offs, before))
        return {"stream": _stream_out(out, offs), "offsets": offs}
    return {"bgr": buf, "types": types}, call


def e_dct_pack_levels_budget(pool, geom, n, seed, k=8):
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n, seed)
    lad = ladder(k)
    arr, _ = nat._ladder(lad)
    budget = _budgets(_raw_planes(buf, stride, n, w, h, tile), types, tile, mv, lad)
    ws = pool.buf("workspace", nat.dct_pack_levels_budget_workspace_bytes(n, w, h, tile[0], mv, k), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    choice = pool.buf("choice", n, I32)

    def call(i):
        before = out.clone()
        nat._check(nat.load().svc_hip_dct_pack_levels_budget_frames(i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv,
                                                                   arr, k, i["budget"].data_ptr(), ws.data_ptr(), ws.numel(),
                                                                   out.data_ptr(), out.numel(), offs.data_ptr(), choice.data_ptr(),
                                                                   nat._stream()))
        _past("dct_pack_levels_budget", (out, offs, before))
        return {"stream": _stream_out(out, offs), "offsets": offs, "choice": choice}
    return {"bgr": buf, "types": types, "budget": budget}, call


def e_dct_pack_layers(pool, geom, n, seed):
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n, seed)
    cap = nat.levels_max_bytes(n, w, h, tile, mv)
    ws = pool.buf("workspace", nat.dct_pack_layers_workspace_bytes(n, w, h, tile[0], mv), U8)
    base, boffs = pool.buf("base", cap, U8), pool.buf("base offsets", n + 1, I64)
    enh, eoffs = pool.buf("enhancement", cap, U8), pool.buf("enhancement offsets", n + 1, I64)

    def call(i):
        before = base.clone(), enh.clone()
        nat._check(nat.load().svc_hip_dct_pack_layers_frames(i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, 4, 16, 1,
                                                            i["window"].data_ptr(), ws.data_ptr(), ws.numel(), base.data_ptr(), cap,
                                                            boffs.data_ptr(), enh.data_ptr(), cap, eoffs.data_ptr(), nat._stream()))
        _past("dct_pack_layers", (base, boffs, before[0]), (enh, eoffs, before[1]))
        return {"base": _stream_out(base, boffs), "base offsets": boffs, "enhancement": _stream_out(enh, eoffs),
                "enhancement offsets": eoffs}
    return {"bgr": buf, "types": types, "window": _windows(n, w, h)}, call


def e_entropy_encode(pool, geom, n, seed, damage=None):
    w, h, tile, mv = geom
    q, qo = _given(damage, lambda: _svcq(geom, n, ENC, seed))
    ws = pool.buf("workspace", nat.entropy_workspace_bytes(n, w, h, tile, mv), U8)
    out = pool.buf("stream", nat.entropy_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    status = pool.buf("status", n, I32)

    def call(i):
        nat.entropy_encode_frames(i["stream"], i["offsets"], w, h, tile, mv, out=out, out_offsets=offs, workspace=ws, status=status)
        _statuses(status, n, damage)
        return {"stream": _stream_out(out, offs), "offsets": offs, "status": status}
    return {"stream": _cuda(q), "offsets": _cuda(qo)}, call


def e_entropy_decode(pool, geom, n, seed, chunk_tiles=None, damage=None):
    w, h, tile, mv = geom
    e, eo = _given(damage, lambda: _svce(geom, n, seed, chunk_tiles))
    ws = pool.buf("workspace", nat.entropy_workspace_bytes(n, w, h, tile, mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    status = pool.buf("status", n, I32)

    def call(i):
        nat._check(nat.load().svc_hip_entropy_decode_frames(i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr(), n, w, h, *tile,
                                                           *mv, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                                                           status.data_ptr(), nat._stream()))
        _statuses(status, n, damage)
        if damage is None:
            q, qo = _svcq(geom, n, ENC, seed)
            assert offs.cpu().tolist() == qo.tolist()
            assert _stream_out(out, offs).cpu().numpy().tobytes() == q.tobytes()  # the pin, for this very call
        return {"stream": _stream_out(out, offs), "offsets": offs, "status": status}
    return {"stream": _cuda(e), "offsets": _cuda(eo)}, call


def _decoder(entry, ws_bytes, fn, layered=False):
    def build(pool, geom, n, seed, chunk_tiles=None, damage=None):
        w, h, tile, mv = geom
        dw, dh = max(1, w - 5), max(1, h - 3)
        if layered:  # a base and its enhancement from one transform (tests/test_gpu_layers.py)
            buf, stride, types = _bgr(geom, n, seed)
            cap = nat.levels_max_bytes(n, w, h, tile, mv)
            base, boffs, enh, eoffs = (torch.empty(cap, dtype=U8, device="cuda"), torch.empty(n + 1, dtype=I64, device="cuda"),
                                       torch.empty(cap, dtype=U8, device="cuda"), torch.empty(n + 1, dtype=I64, device="cuda"))
            lws = torch.empty(nat.dct_pack_layers_workspace_bytes(n, w, h, tile[0], mv), dtype=U8, device="cuda")
            nat._check(nat.load().svc_hip_dct_pack_layers_frames(buf.data_ptr(), stride, n, w, h, tile[0], types.data_ptr(), *mv, 4, 16, 1, None,
                                                                lws.data_ptr(), lws.numel(), base.data_ptr(), cap, boffs.data_ptr(),
                                                                enh.data_ptr(), cap, eoffs.data_ptr(), nat._stream()))
            inputs = {"base": base[:int(boffs[-1])].clone(), "base offsets": boffs, "enhancement": enh[:int(eoffs[-1])].clone(),
                      "enhancement offsets": eoffs}
        elif entry == "decode_entropy":
            e, eo = _given(damage, lambda: _svce(geom, n, seed, chunk_tiles))
            inputs = {"stream": _cuda(e), "offsets": _cuda(eo)}
        else:
            q, qo = _given(damage, lambda: _svcq(geom, n, ENC, seed))
            inputs = {"stream": _cuda(q), "offsets": _cuda(qo)}
        inputs["gaze"] = _windows(n, w, h)
        ws = pool.buf("workspace", ws_bytes(n, w, h, tile, mv), U8)
        rec = pool.buf("rec", (n, h, w, 3), F32)
        disp = pool.buf("display", (n, dh, dw, 3), U8)
        status = pool.buf("status", n, I32)

        def call(i):
            if layered:
                head = (i["base"].data_ptr(), i["base"].numel(), i["base offsets"].data_ptr(), i["enhancement"].data_ptr(),
                        i["enhancement"].numel(), i["enhancement offsets"].data_ptr())
            else:
                head = (i["stream"].data_ptr(), i["stream"].numel(), i["offsets"].data_ptr())
            nat._check(fn()(*head, n, w, h, *tile, *mv, *DEC, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(), rec.data_ptr(),
                            disp.data_ptr(), dw, dh, status.data_ptr(), nat._stream()))
            _statuses(status, n, damage)
            return {"rec": rec, "display": disp, "status": status}
        return inputs, call
    return build


e_decode_levels = _decoder("decode_levels", lambda n, w, h, t, mv: nat.decode_levels_workspace_bytes(n, w, h, t),
                           lambda: nat.load().svc_hip_decode_levels_frames)
e_decode_entropy = _decoder("decode_entropy", lambda n, w, h, t, mv: nat.decode_entropy_workspace_bytes(n, w, h, t, mv),
                            lambda: nat.load().svc_hip_decode_entropy_frames)
e_decode_layers = _decoder("decode_layers", lambda n, w, h, t, mv: nat.decode_layers_workspace_bytes(n, w, h, t),
                           lambda: nat.load().svc_hip_decode_layers_frames, layered=True)


def _src_of(n_in, n_out):
    return None if n_in == n_out else _cuda(np.array([(2 * i + 1) % n_in for i in range(n_out)], np.int32))


def _windower(entropy_coded):
    def build(pool, geom, n, seed, n_in=None, chunk_tiles=None, damage=None, windows=None):
        w, h, tile, mv = geom
        n_in = n if n_in is None else n_in
        s, so = _given(damage, lambda: _svce(geom, n_in, seed, chunk_tiles) if entropy_coded else _svcq(geom, n_in, ENC, seed))
        inputs = {"stream": _cuda(s), "offsets": _cuda(so), "window": _windows(n, w, h, windows)}
        if n_in != n:
            inputs["src"] = _src_of(n_in, n)
        sizes = (nat.window_entropy_workspace_bytes, nat.window_entropy_max_bytes) if entropy_coded else (nat.window_levels_workspace_bytes,
                                                                                                           nat.levels_max_bytes)
        fn = nat.window_entropy_frames if entropy_coded else nat.window_levels_frames
        ws = pool.buf("workspace", sizes[0](n, w, h, tile, mv), U8)
        out = pool.buf("stream", sizes[1](n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)
        status = pool.buf("status", n, I32)

        def call(i):
            before = out.clone()
            fn(i["stream"], i["offsets"], w, h, tile, mv, window=i["window"], src=i.get("src"), out=out, out_offsets=offs, workspace=ws,
               status=status)
            _past(fn.__name__, (out, offs, before))
            _statuses(status, n, damage)
            return {"stream": _stream_out(out, offs), "offsets": offs, "status": status}
        return inputs, call
    return build


e_window_levels = _windower(False)
e_window_entropy = _windower(True)


def _splitter(budgeted):
    def build(pool, geom, n, seed, n_in=None, k=8, damage=None, windows=None):
        w, h, tile, mv = geom
        n_in = n if n_in is None else n_in
        q, qo = _given(damage, lambda: _svcq(geom, n_in, (FINE, FINE), seed))
        src = _src_of(n_in, n)
        inputs = {"stream": _cuda(q), "offsets": _cuda(qo), "window": _windows(n, w, h, windows)}
        if src is not None:
            inputs["src"] = src
        cap = nat.levels_max_bytes(n, w, h, tile, mv)
        if budgeted:
            lad = [(int(fg) * FINE, int(bg) * FINE) for fg, bg in ladder(k)]
            picks = range(n) if src is None else src.cpu().tolist()
            budget = []
            for i, f in enumerate(picks):  # the base frame's size at another entry per frame; the last one below the masks' floor
                fg, bg = lad[(3 * i + len(lad) // 2) % len(lad)]
                budget.append(len(layers.split_frame(q[int(qo[f]):int(qo[f + 1])].tobytes(), FINE, fg, bg)[0]) if damage is None else 1 << 20)
            if n > 1 and damage is None:
                budget[-1] = frame_floor(w, h, *tile, *mv) - 16
            inputs["budget"] = nat.budget_tensor(budget, n, "cuda")
            ws = pool.buf("workspace", nat.split_levels_budget_workspace_bytes(n_in, n, w, h, tile, mv, k), U8)
        else:
            ws = pool.buf("workspace", nat.split_levels_workspace_bytes(n_in, n, w, h, tile, mv), U8)
        base, boffs = pool.buf("base", cap, U8), pool.buf("base offsets", n + 1, I64)
        enh, eoffs = pool.buf("enhancement", cap, U8), pool.buf("enhancement offsets", n + 1, I64)
        status = pool.buf("status", n, I32)
        choice = pool.buf("choice", n, I32) if budgeted else None

        def call(i):
            before = base.clone(), enh.clone()
            kw = dict(window=i["window"], src=i.get("src"), base_out=base, base_offsets=boffs, enh_out=enh, enh_offsets=eoffs, workspace=ws,
                      status=status)
            if budgeted:
                nat.split_levels_budget_frames(i["stream"], i["offsets"], w, h, tile, mv, FINE, lad, i["budget"], choice=choice, **kw)
            else:
                nat.split_levels_frames(i["stream"], i["offsets"], w, h, tile, mv, FINE, 4, 16, **kw)
            _statuses(status, n, damage)
            _past("split_levels", (base, boffs, before[0]), (enh, eoffs, before[1]))
            got = {"base": _stream_out(base, boffs), "base offsets": boffs, "enhancement": _stream_out(enh, eoffs),
                   "enhancement offsets": eoffs, "status": status}
            if budgeted:
                got["choice"] = choice
            return got
        return inputs, call
    return build


e_split_levels = _splitter(False)
e_split_levels_budget = _splitter(True)

ENTRIES = {
    "pack_levels": (e_pack_levels, STREAM), "unpack_levels": (e_unpack_levels, STREAM), "pack_levels_budget": (e_pack_levels_budget, STREAM),
    "dct_pack_levels": (e_dct_pack_levels, FUSED), "dct_pack_levels_budget": (e_dct_pack_levels_budget, FUSED),
    "dct_pack_layers": (e_dct_pack_layers, FUSED), "entropy_encode": (e_entropy_encode, STREAM), "entropy_decode": (e_entropy_decode, STREAM),
    "decode_levels": (e_decode_levels, STREAM), "decode_entropy": (e_decode_entropy, STREAM), "decode_layers": (e_decode_layers, FUSED),
    "window_levels": (e_window_levels, STREAM), "window_entropy": (e_window_entropy, STREAM), "split_levels": (e_split_levels, STREAM),
    "split_levels_budget": (e_split_levels_budget, STREAM),
}
SEGMENT_FIELDS = [(22, 18, 0), (33, 31, 0), (240, 135, nat.LAUNCH_NO_WIDE), (240, 135, nat.LAUNCH_WIDE)]  # the last two: above 8 192 blocks
GLOBAL_EBMA = [(97, 61, 5), (30, 20, 19)]
# the ladder of the budgeted forms is a host array the library copies before it returns (svc_step_pair* ladder, "host"): no kernel reads
# it where it lies, so it has no neighbours to vary and is not surrounded
LADDERED = ("pack_levels_budget", "dct_pack_levels_budget", "split_levels_budget")
RESIZING = ("window_levels", "window_entropy", "split_levels", "split_levels_budget")  # n_out != n_in through d_src
SVCE_READERS = ("entropy_decode", "decode_entropy", "window_entropy")
# what an entry point refuses (its *_workspace_bytes is 0 there: check_every_pair_is_sized): the decoders take 8 x 8 and 16 x 16 tiles
# on widths that are multiples of 16 only (validate_decode_geom), so none of GX
REFUSED = {(e, g) for e in ("decode_levels", "decode_entropy") for g in GX}
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms if (e, g) not in REFUSED]


def _workspace_bytes(entry, geom, n=3, k=8):
    w, h, tile, mv = geom
    q = {"pack_levels": lambda: nat.pack_levels_workspace_bytes(n, w, h, tile),
         "unpack_levels": lambda: nat.pack_levels_workspace_bytes(n, w, h, tile),
         "pack_levels_budget": lambda: nat.pack_levels_budget_workspace_bytes(n, w, h, tile, k),
         "dct_pack_levels": lambda: nat.dct_pack_levels_workspace_bytes(n, w, h, tile[0], mv),
         "dct_pack_levels_budget": lambda: nat.dct_pack_levels_budget_workspace_bytes(n, w, h, tile[0], mv, k),
         "dct_pack_layers": lambda: nat.dct_pack_layers_workspace_bytes(n, w, h, tile[0], mv),
         "entropy_encode": lambda: nat.entropy_workspace_bytes(n, w, h, tile, mv),
         "entropy_decode": lambda: nat.entropy_workspace_bytes(n, w, h, tile, mv),
         "decode_levels": lambda: nat.decode_levels_workspace_bytes(n, w, h, tile),
         "decode_entropy": lambda: nat.decode_entropy_workspace_bytes(n, w, h, tile, mv),
         "decode_layers": lambda: nat.decode_layers_workspace_bytes(n, w, h, tile),
         "window_levels": lambda: nat.window_levels_workspace_bytes(n, w, h, tile, mv),
         "window_entropy": lambda: min(nat.window_entropy_workspace_bytes(n, w, h, tile, mv), nat.window_entropy_max_bytes(n, w, h, tile, mv)),
         "split_levels": lambda: nat.split_levels_workspace_bytes(n, n, w, h, tile, mv),
         "split_levels_budget": lambda: nat.split_levels_budget_workspace_bytes(n, n, w, h, tile, mv, k)}[entry]()
    return q


def _sized(entry, geom, n=3, k=8):
    w, h, tile, mv = geom
    return min(_workspace_bytes(entry, geom, n, k), nat.levels_max_bytes(n, w, h, tile, mv), nat.entropy_max_bytes(n, w, h, tile, mv))


def check_every_pair_is_sized():
    """No case below is a refusal in disguise: every size query of every (entry point, geometry) pair is not 0, for every frame count
    and ladder length used; and the pairs left out are refused.  The queries need no device: tests/test_guarded_host.py runs this."""
    for entry, geom in PAIRS:
        for n in NS:
            for k in (1, 8, 64) if entry in LADDERED else (8,):
                assert _sized(entry, geom, n, k) > 0, (entry, geom, n, k)
    for entry, geom in REFUSED:
        assert _sized(entry, geom) == 0, (entry, geom)
    for entry, geoms in SVCQ_READERS.items():  # the malformed-input cases
        for geom in geoms:
            assert _sized(entry, geom, 3) > 0, (entry, geom)
    assert _sized("window_entropy", G8[0], 4) > 0 and _sized("entropy_decode", (64, 48, (8, 8), MV16), 3) > 0
    for mfw, mfh, _ in SEGMENT_FIELDS:
        for n in (3,) if mfw == 240 else NS:
            assert nat.segment_workspace_bytes(mfw, mfh, n) > 0, (mfw, mfh, n)
    for block in (8, 16):
        n, tx, ty = ti.TUNED_PLACEMENT[block]
        assert nat.load().svc_hip_dct_redo_workspace_bytes(n, tx * block, ty * block, 16, 16) > 0, block
    for w, h, r in GLOBAL_EBMA:
        for n in NS:
            assert nat.load().svc_hip_global_ebma_workspace_bytes(r, n) > 0, (r, n)


def _other_entry(entry, pool, geom, n):
    """Another entry point run on this case's workspace interior (its other buffers are its own): the leftovers a caller's shared arena
    holds.  The largest of n frames and one frame whose workspace fits; None where neither does."""
    for other, m in _others(entry, geom, n):
        if _workspace_bytes(other, geom, m) <= pool.written["workspace"].nbytes:
            mine = Pool()
            mine.written["workspace"], mine.borrowed = pool.written["workspace"], {"workspace"}
            return ENTRIES[other][0](mine, geom, m, 2)
    return None


def _others(entry, geom, n):
    """(entry point, frames) to try, the larger workspaces first: the coder, the window call, the pack, the unpack -- never the entry
    point itself or the one that shares its kernels' workspace layout (the coder's two directions)."""
    family = {"entropy_encode": "entropy", "entropy_decode": "entropy"}
    return [(o, m) for o in ("entropy_encode", "window_levels", "pack_levels", "unpack_levels") for m in (n, 1)
            if o != entry and family.get(o, o) != family.get(entry, entry) and _sized(o, geom, m) > 0]


def _check(entry, build, geom, n, dirty_n, **kw):
    pool = Pool()
    inputs, call = build(pool, geom, n, 0, **kw)
    pool.reuse = True
    assert dirty_n <= n  # the calls that dirty the buffers: this entry point with fewer frames (one frame: as many) and other content ...
    d_inputs, d_call = build(pool, geom, dirty_n, 1, **{k: v for k, v in kw.items() if k != "n_in"})
    pool.reuse = False
    other = _other_entry(entry, pool, geom, n)  # ... then another entry point on the same workspace

    def dirty():
        d_call(d_inputs)
        if other is not None:
            other[1](other[0])
    name = f"{entry} {_gid(geom)} n={n} {kw}"
    plain = {k: gd.surround(v, 0) for k, v in inputs.items()}
    findings = gd.check_writes(name, pool.written, lambda: call(plain), dirty=dirty, seed=n)
    findings += gd.check_reads(name, inputs, call, pool.written)
    return findings


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    build = ENTRIES[entry][0]
    findings = []
    for n in NS:
        findings += _check(entry, build, geom, n, max(1, n - 2))
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("entry,geom", [p for p in PAIRS if p[0] in LADDERED], ids=[f"{e}-{_gid(g)}" for e, g in PAIRS if e in LADDERED])
def test_ladders_of_1_and_64_entries(native, entry, geom, k):
    """The budgeted forms above run with 8 entries; the per-entry arrays of their workspaces at the two other lengths."""
    findings = []
    for n in (3, 5):
        findings += _check(entry, ENTRIES[entry][0], geom, n, 2, k=k)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("n_in,n_out", [(2, 5), (5, 2)])
@pytest.mark.parametrize("entry,geom", [p for p in PAIRS if p[0] in RESIZING], ids=[f"{e}-{_gid(g)}" for e, g in PAIRS if e in RESIZING])
def test_other_frame_counts_out_than_in(native, entry, geom, n_in, n_out):
    findings = _check(entry, ENTRIES[entry][0], geom, n_out, n_out // 2, n_in=n_in)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("ct", [1, 0xFFFFFFFF])
@pytest.mark.parametrize("entry", SVCE_READERS)
def test_svce_frames_of_other_chunk_tiles(native, entry, ct):
    """chunk_tiles = 1 in the header: a chunk per tile, the most the decoders' [n][max_chunks] arrays are sized for; 2^32 - 1: a chunk per
    tile row (frames of the numpy coder, as test_gpu_decoder_honours_any_chunk_tiles builds them)."""
    findings = []
    for geom in (G8[0], G8[2], G16[0]):
        findings += _check(entry, ENTRIES[entry][0], geom, 3, 2, chunk_tiles=ct)
    assert not findings, "\n".join(findings)


# ---- malformed input: frames the project already refuses on the GPU today, with other bytes after them --------------------------------------
# The case lists are those of the tests named below, on their geometries.  Each case is applied to the first, the middle and the LAST
# frame of a stream that is exactly its bytes inside a surround: a reader that trusts a damaged count or size of the last frame reads the
# surround's noise, which differs between the two seeds.  Which status each case gets is pinned where the cases come from; here exactly
# the damaged frame must be refused, every output must be the same under both seeds and every guard intact.

HOST12 = (36, 24, (12, 12), (12, 12))  # GEOMS[1] of tests/test_window_levels_host.py: 144 of a tile's 192 mask bits are coefficients


def _levels_off(geom):
    w, h, tile, mv = geom
    return 64 + 4 * (w // mv[0]) * (h // mv[1]) + 8 * 3 * (w // tile[0]) * (h // tile[1]) * ((tile[0] * tile[1] + 63) // 64)


def _svcq_cases(geom, split):
    """test_malformed_frames of tests/test_gpu_window_levels.py and tests/test_gpu_split_levels.py: magic, version, frame_w, block_h, fg_step
    0, frame_bytes + 16, level_count +- 1, a stray mask bit past a 12 x 12 tile's coefficients; for the split calls also the frames that
    are not at fine_step (status 11)."""
    w, h, tile, mv = geom
    cases = [(0, 0x12345678), (1, 2), (2, w + tile[0]), (5, 6), (8, 0), (12, "+16"), (10, "+1"), (10, "-1")]
    if tile == (12, 12):
        cases.append(("stray", None))
    return cases + ([(8, 2 * FINE), (9, 2 * FINE), (8, 1)] if split else [])


def _damaged_svcq(stream, offs, f, case, geom):
    bad, o = stream.copy(), int(offs[f])
    k, value = case
    if k == "stray":
        bad[o + _levels_off(geom) - 1] |= 0x40  # bit 190 of the frame's last tile
    else:
        word = bad[o + 4 * k:o + 4 * k + 4].view("<u4")
        word[0] = (int(word[0]) + int(value)) & 0xFFFFFFFF if isinstance(value, str) else value
    return bad


def _check_damaged(entry, geom, n, damage, what, **kw):
    pool = Pool()
    inputs, call = ENTRIES[entry][0](pool, geom, n, 0, damage=damage, **kw)
    return gd.check_reads(f"{entry} {_gid(geom)} {what}", inputs, call, pool.written)


SVCQ_READERS = {"unpack_levels": (HOST12, G8[0]), "entropy_encode": (HOST12, G8[0]), "window_levels": (HOST12, G8[0]),
                "split_levels": (HOST12, G8[0]), "split_levels_budget": (HOST12, G8[0]),
                "decode_levels": (G8[0], G16[0])}  # the decoder takes 8 x 8 and 16 x 16 tiles only: no stray-bit case for it


@pytest.mark.parametrize("entry", sorted(SVCQ_READERS))
def test_damaged_svcq_frames(native, entry):
    split = entry.startswith("split")
    findings = []
    for geom in SVCQ_READERS[entry]:
        stream, offs = _svcq(geom, 3, (FINE, FINE) if split else ENC, 0)
        for f in range(3):
            for case in _svcq_cases(geom, split):
                bad = _damaged_svcq(stream, offs, f, case, geom)
                assert bad.tobytes() != stream.tobytes(), (f, case)
                findings += _check_damaged(entry, geom, 3, (bad, offs, (f,)), f"frame {f} damaged {case}")
    assert not findings, "\n".join(findings)


def _frames(stream, offs):
    return [bytes(stream[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]


def _joined(frames):
    return np.frombuffer(b"".join(frames), np.uint8).copy(), np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)


def test_damaged_svce_frames_in_the_entropy_decoder(native):
    """tests/test_gpu_entropy.py: every case of _corrupt_cases, and test_crafted_frames_get_status_8_and_zeros' two crafted frames (among
    that test's own good frames), each as the first, the middle and the last frame."""
    from tests.test_entropy_host import _sparse, overflowing_chunk_tiles_frame, width_32_type_overflow_frame
    from tests.test_gpu_entropy import _corrupt_cases
    from tests.test_levels_host import write_frames
    findings = []
    for geom in (G8[0], G16[0]):
        good = _frames(*_svce(geom, 3))
        for f in range(3):
            for name, bad, _ in _corrupt_cases(good[f]):
                e, eo = _joined(good[:f] + [bytes(bad)] + good[f + 1:])
                findings += _check_damaged("entropy_decode", geom, 3, (e, eo, (f,)), f"frame {f}: {name}")
    geom = (64, 48, (8, 8), MV16)
    planes, types = _sparse(np.random.default_rng(1), 2, 64, 48, 8, 8, MV16, 1, 640)
    q, qo = write_frames(planes, types, 8, 8, 16, 16, 1, 640)
    good = [entropy.encode_frame(q[int(a):int(b)]) for a, b in zip(qo[:-1], qo[1:])]
    for bad in (overflowing_chunk_tiles_frame(), width_32_type_overflow_frame()):
        for f in range(3):
            frames = list(good)
            frames.insert(f, bad)
            e, eo = _joined(frames)
            findings += _check_damaged("entropy_decode", geom, 3, (e, eo, (f,)), f"crafted frame at {f}")
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("shape", [0, 1])
def test_damaged_svce_frames_in_the_display_decoder(native, shape):
    """tests/test_gpu_decode_entropy.py::test_damaged_middle_frame_gets_its_status_and_zeros: its stream, every case of its _damage (the
    chunk whose last byte makes the coder walk garbage included), on each of the three frames."""
    from tests import test_gpu_decode_entropy as de
    block, w, h, mv = de.SHAPES[shape]
    geom = (w, h, (block, block), (mv, mv))
    svcq, offs = de._picture_svcq(block, w, h, mv, 6, 40, seed=3)
    e, eo = de._gpu_svce(svcq, offs, block, w, h, mv)
    eo = eo.cpu().numpy().astype(np.int64)
    good = _frames(e.cpu().numpy(), eo)
    findings = []
    for f in range(3):
        for what in ("magic", "index level count", "chunk one byte short", "chunk's last byte", "svcq_frame_bytes"):
            try:
                bad, _ = de._damage(good[f], what)
            except AssertionError:  # no value of a last byte breaks a chunk of this frame: the case exists for the middle frame at least
                assert what == "chunk's last byte" and f != 1
                continue
            assert len(bad) == len(good[f]) and bytes(bad) != good[f]
            stream, _ = _joined(good[:f] + [bytes(bad)] + good[f + 1:])
            findings += _check_damaged("decode_entropy", geom, 3, (stream, eo, (f,)), f"frame {f}: {what}")
    assert not findings, "\n".join(findings)


def test_damaged_svce_frames_in_the_window_call(native):
    """tests/test_gpu_window_entropy.py::test_malformed_frames: its stream, its windows and its cases (header words, svcq_frame_bytes,
    level_count, types_bytes, the index's sum, the types' mode word) on each of the four frames; and
    test_garbage_in_a_chunk_is_flagged_only_where_it_is_walked's garbage in chunk 0 under its window that cuts chunk 0 (a chunk the
    window keeps whole is copied, not walked, and not flagged)."""
    from tests.test_window_entropy_host import chunk_table
    from tests.test_window_levels_host import random_stream
    geom = G8[0]
    w, h, tile, mv = geom
    stream, offs = random_stream(np.random.default_rng(4), geom, 4, 0.06)
    svce, so = entropy.encode_frames(stream, offs)
    base, so = np.frombuffer(svce, np.uint8), np.asarray(so).astype(np.int64)
    windows = [(8 * 4, 0, 8 * 20, h), (0, 0, w, h), (8 * 30, 8, w, 8), (8 * 33, 0, 8, h)]
    cut = [(8 * 4, 0, 8 * 20, h)] * 4
    cases = [(0, 0x12345678), (1, 2), (2, w + 8), (5, 4), (8, 0), (14, 0), (12, "+16"), (13, "+16"), (10, "+1"), (15, "+4"), ("index", None),
             ("types", None), ("garbage", None)]
    findings = []
    for f in range(4):
        o = int(so[f])
        for k, value in cases:
            bad = base.copy()
            if k == "index":  # one more level in the first entry: the counts no longer sum to word 10
                i0 = o + 64 + int(base[o + 60:o + 64].view("<u4")[0])
                bad[i0 + 2:i0 + 4].view("<u2")[0] += 1
            elif k == "types":
                bad[o + 64:o + 68].view("<u4")[0] = 2  # neither bitmap nor raw
            elif k == "garbage":
                _, start, sizes, _ = chunk_table(_frames(base, so)[f])
                assert sizes[0] >= 8 and not base[o + start[0]] & 1
                bad[o + start[0]] &= 0x7F
                bad[o + start[0] + 1:o + start[0] + 5] = 0
            else:
                word = bad[o + 4 * k:o + 4 * k + 4].view("<u4")
                word[0] = int(word[0]) + int(value) if isinstance(value, str) else value
            findings += _check_damaged("window_entropy", geom, 4, (bad, so, (f,)), f"frame {f} damaged {(k, value)}",
                                       windows=cut if k == "garbage" else windows)
    assert not findings, "\n".join(findings)


# ---- the three older workspace entry points --------------------------------------------------------------------------------------------------

def _segment_case(pool, mfw, mfh, n, density, flags, seed):
    """The fields of tests/test_gpu_segment.py::test_segment_heavy_frames: a frame of the given foreground density, a light one, an empty one."""
    rng = np.random.default_rng(int(density * 100) + mfw + seed)
    yy, xx = np.mgrid[0:mfh, 0:mfw]
    masks, mvs = [], []
    for f in range(n):
        blob = rng.random((mfh, mfw)) < (density, 0.02, 0.0)[f % 3]
        masks.append((~blob).astype(np.uint8).reshape(-1))
        mvs.append(np.stack([np.round(6 * np.sin(xx / 17.0 + f) + rng.integers(-2, 3, (mfh, mfw))), rng.integers(-9, 10, (mfh, mfw))],
                            -1).astype(np.float32).reshape(mfw * mfh, 2))
    ws = pool.buf("workspace", nat.segment_workspace_bytes(mfw, mfh, n), U8)
    out = pool.buf("types", (n, mfw * mfh), I32)

    def call(i):
        nat.segment_frames(i["mask"], i["mv"], mfw, mfh, seed=77, out=out, workspace=ws, flags=flags)
        return {"types": out}
    return {"mask": _cuda(np.stack(masks)), "mv": _cuda(np.stack(mvs))}, call


@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("mfw,mfh,flags", SEGMENT_FIELDS,
                         ids=["22x18", "33x31", "240x135-one-workgroup", "240x135-wide"])
def test_segment_frames_ex(native, mfw, mfh, flags, density):
    findings = []
    for n in (3,) if mfw == 240 else NS:
        assert nat.segment_workspace_bytes(mfw, mfh, n) > 0
        pool = Pool()
        inputs, call = _segment_case(pool, mfw, mfh, n, density, flags, 0)
        pool.reuse = True
        d_inputs, d_call = _segment_case(pool, mfw, mfh, max(1, n - 2), 0.7, 0, 1)  # fewer frames of another density, the default form
        name = f"segment_frames_ex {mfw}x{mfh} n={n} density {density} flags {flags}"
        plain = {k: gd.surround(v, 0) for k, v in inputs.items()}
        findings += gd.check_writes(name, pool.written, lambda: call(plain), dirty=lambda: d_call(d_inputs), seed=n)
        findings += gd.check_reads(name, inputs, call, pool.written)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("block", [8, 16])
def test_dct_quant_redo_frames(native, block):
    """The placement input of tests/helpers/transform_inputs.py with test_dct_quant_luma_then_redo's region ids: a foreground list that
    ends in a partial workgroup trip.  The planes are input and output: every call starts from the speculative planes."""
    from tests.test_gpu_transform_exact import _random_types
    frames, _ = ti.tuned_placement_frames(block)
    n, h, w, _ = frames.shape
    mv = 16
    types = _random_types(77 + block, n, w, h, mv)
    assert (int((types != 0).sum()) * (mv // block)) % (256 // block) != 0
    per, extra = w * h * 3, 48
    buf = torch.randint(0, 256, (n * (per + extra) - extra,), dtype=U8, device="cuda")
    for f in range(n):
        buf[f * (per + extra):f * (per + extra) + per] = _cuda(frames[f]).reshape(-1)
    spec, _, _ = nat.dct_quant_luma_frames(_cuda(frames), block, 1, bg_step=640)
    need = int(nat.load().svc_hip_dct_redo_workspace_bytes(n, w, h, mv, mv))
    assert need > 0
    written = {"workspace": gd.Guarded(need, U8, "cuda"), "planes": gd.like(spec, seed=1)}
    ws, planes = written["workspace"].interior, written["planes"].interior

    def call(i):
        planes.copy_(spec)
        nat._check(nat.load().svc_hip_dct_quant_redo_frames(i["bgr"].data_ptr(), per + extra, n, w, h, block, i["types"].data_ptr(), mv, mv, 7,
                                                           planes.data_ptr(), ws.data_ptr(), need, nat._stream()))
        return {"planes": planes}

    def dirty():  # the same scratch after a list of another length: every MV block of the first two frames
        other = torch.ones((n, types.shape[1]), dtype=I32, device="cuda")
        other[2:] = 0
        call({"bgr": buf, "types": other})
    inputs = {"bgr": buf, "types": _cuda(types.view(np.int32))}
    plain = {k: gd.surround(v, 0) for k, v in inputs.items()}
    findings = gd.check_writes(f"dct_quant_redo_frames {block}", written, lambda: call(plain), dirty=dirty)
    findings += gd.check_reads(f"dct_quant_redo_frames {block}", inputs, call, written)
    want = nat.dct_quant_frames(_cuda(frames), block, inputs["types"], mv, 7, 640)
    assert torch.equal(call(plain)["planes"], want)  # the pin, for this very call (tests/test_gpu_dct_quant.py)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("w,h,r", GLOBAL_EBMA)
def test_global_ebma_pairs(native, w, h, r):
    """tests/test_gpu_global_motion.py::test_global_ebma_batched_device's planes at test_global_ebma_vs_oracle's odd shapes."""
    findings = []
    for n in NS:
        rng = np.random.default_rng(w + n)
        planes = rng.integers(0, 256, (n + 1, h, w), dtype=np.uint8)
        planes[1] = np.roll(planes[0], (2, -3), (0, 1))
        need = int(nat.load().svc_hip_global_ebma_workspace_bytes(r, n))
        assert need > 0
        written = {"workspace": gd.Guarded(need, U8, "cuda"), "gm": gd.Guarded(8 * n, F32, "cuda", seed=1, shape=(n, 2)),
                   "mad": gd.Guarded(4 * n, F32, "cuda", seed=2)}
        ws, gm, mad = (written[k].interior for k in ("workspace", "gm", "mad"))

        def call(i, pairs=n):
            p = i["planes"]
            nat._check(nat.load().svc_hip_global_ebma_pairs(p.data_ptr(), p.data_ptr() + w * h, w * h, pairs, w, h, r, ws.data_ptr(), need,
                                                           gm.data_ptr(), mad.data_ptr(), nat._stream()))
            return {"gm": gm[:pairs], "mad": mad[:pairs]}
        inputs = {"planes": _cuda(planes).reshape(-1)}
        plain = {"planes": gd.surround(inputs["planes"], 0)}
        other = {"planes": _cuda(rng.integers(0, 256, (n + 1) * h * w, dtype=np.uint8))}
        findings += gd.check_writes(f"global_ebma_pairs {w}x{h} R={r} n={n}", written, lambda: call(plain),
                                    dirty=lambda: call(other, max(1, n - 2)), seed=n)
        findings += gd.check_reads(f"global_ebma_pairs {w}x{h} R={r} n={n}", inputs, call, written)
    assert not findings, "\n".join(findings)
