"""Where svc_hip_band_levels_frames and svc_hip_union_levels_frames write and what their results depend on (tests/helpers/guarded.py):
workspace, output stream, offsets and status of exactly the sizes the API asks for inside guarded allocations, the four poisons, and
other bytes beside each input.  The builders have the form of tests/test_gpu_guard_streams.py's and run through its _check;
tests/test_gpu_placement_band.py takes them from here."""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import ENC, G8, NS, STREAM, _check, _cuda, _gid, _given, _past, _src_of, _statuses, _stream_out, _svcq, _windows

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
ALL = 0xFFFFFFFF


def band_rows(n, tile):
    """One band per output frame, in a cycle: the lowest quarter, an odd cut's remainder, everything, DC, all but DC."""
    bw, bh = tile
    k = max(1, max(bw, bh) // 4)
    cycle = [(0, 0, k, k), (3, 3, ALL, ALL), (0, 0, ALL, ALL), (0, 0, 1, 1), (1, 1, bw, bh)]
    return [cycle[i % len(cycle)] for i in range(n)]


def _bands(n, tile):
    return _cuda(np.asarray(band_rows(n, tile), dtype=np.uint32).view(np.int32).reshape(n, 4))


def e_band_levels(pool, geom, n, seed, n_in=None, damage=None, windows=None):
    w, h, tile, mv = geom
    n_in = n if n_in is None else n_in
    s, so = _given(damage, lambda: _svcq(geom, n_in, ENC, seed))
    inputs = {"stream": _cuda(s), "offsets": _cuda(so), "window": _windows(n, w, h, windows), "band": _bands(n, tile)}
    if n_in != n:
        inputs["src"] = _src_of(n_in, n)
    ws = pool.buf("workspace", nat.band_levels_workspace_bytes(n, w, h, tile, mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    status = pool.buf("status", n, I32)

    def call(i):
        before = out.clone()
        nat.band_levels_frames(i["stream"], i["offsets"], w, h, tile, mv, band=i["band"], window=i["window"], src=i.get("src"), out=out,
                               out_offsets=offs, workspace=ws, status=status)
        _past("band_levels_frames", (out, offs, before))
        _statuses(status, n, damage)
        return {"stream": _stream_out(out, offs), "offsets": offs, "status": status}
    return inputs, call


@functools.lru_cache(maxsize=None)
def union_parts(geom, n, seed=0):
    """_svcq's frames cut in two at an odd place (row or column 3), by the numpy statement -> (low, its offsets, high, its offsets)."""
    q, qo = _svcq(geom, n, ENC, seed)
    low, lo = layers.band_frames(q, qo, [(0, 0, 3, 3)] * n)
    high, ho = layers.band_frames(q, qo, [(3, 3, ALL, ALL)] * n)
    as_array = lambda b, o: (np.frombuffer(b, np.uint8).copy(), np.asarray(o).astype(np.int64))
    return as_array(low, lo) + as_array(high, ho)


def e_union_levels(pool, geom, n, seed):
    w, h, tile, mv = geom
    low, lo, high, ho = union_parts(geom, n, seed)
    inputs = {"stream": _cuda(high), "offsets": _cuda(ho), "second": _cuda(low), "second offsets": _cuda(lo)}
    ws = pool.buf("workspace", nat.union_levels_workspace_bytes(n, w, h, tile, mv), U8)
    out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
    offs = pool.buf("offsets", n + 1, I64)
    status = pool.buf("status", n, I32)

    def call(i):
        before = out.clone()
        nat.union_levels_frames(i["stream"], i["offsets"], i["second"], i["second offsets"], w, h, tile, mv, out=out, out_offsets=offs,
                                workspace=ws, status=status)
        _past("union_levels_frames", (out, offs, before))
        _statuses(status, n, None)
        return {"stream": _stream_out(out, offs), "offsets": offs, "status": status}
    return inputs, call


ENTRIES = {"band_levels": (e_band_levels, STREAM), "union_levels": (e_union_levels, STREAM)}
PAIRS = [(e, g) for e, (_, geoms) in ENTRIES.items() for g in geoms]


def test_every_pair_is_sized(native):
    """No case below is a refusal in disguise."""
    for entry, geom in PAIRS:
        w, h, tile, mv = geom
        query = nat.band_levels_workspace_bytes if entry == "band_levels" else nat.union_levels_workspace_bytes
        for n in NS:
            assert query(n, w, h, tile, mv) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0, (entry, geom, n)


@pytest.mark.parametrize("entry,geom", PAIRS, ids=[f"{e}-{_gid(g)}" for e, g in PAIRS])
def test_poisoned_buffers_and_neighbours(native, entry, geom):
    findings = []
    for n in NS:
        findings += _check(entry, ENTRIES[entry][0], geom, n, max(1, n - 2))
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("n_in,n_out", [(2, 5), (5, 2)])
@pytest.mark.parametrize("geom", [G8[0], STREAM[-1]], ids=_gid)
def test_other_frame_counts_out_than_in(native, geom, n_in, n_out):
    findings = _check("band_levels", e_band_levels, geom, n_out, n_out // 2, n_in=n_in)
    assert not findings, "\n".join(findings)
