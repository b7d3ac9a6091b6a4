"""Where svc_hip_dct_pack_delta_quality_frames (include/svc_hip_delta_quality.h) writes and what its result depends on
(tests/helpers/guarded.py): workspace, output stream, offsets, choices and both tables of exactly the sizes the API asks for inside
guarded allocations, the four poisons (the leftovers of a call with another frame count and of another entry point among them -- every
row the sum reads and every part and step the later launches read was stored by this call's own kernels), and other bytes beside each
input -- the frames, their region ids, the key flags, the targets and the budgets.  The builder has the form of
tests/test_gpu_guard_streams.py's and runs through its _check; tests/test_gpu_placement_dct_pack_delta_quality.py and
tests/test_gpu_stream_order_dct_pack_delta_quality.py take it from here.

The flags cut a batch into groups of two frames.  Per group the target is every frame's own D at one ladder entry of the reference
(svc_hip_dct_pack_levels_quality_frames' table) and the budget the group's bytes at another (the reference of
tests/test_gpu_guard_dct_pack_delta_budget.py), the last group's 0: the groups of one batch take different entries, by quality and by the
cap, and the last is over budget.  A second builder runs without flags, without a budget and without the tables: all four pointers NULL."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_dct_pack_delta_budget import GEOMS, N, budgets_of, keys_of
from tests.test_gpu_guard_streams import _bgr, _check, _gid, _past, _stream_out
from tests.test_levels_budget_host import ladder

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
ENTRY = "dct_pack_delta_quality"
_tables = {}


def reference_distortion(geom, n, seed, lad):
    """D[f][k] from svc_hip_dct_pack_levels_quality_frames -> (n, K) u64; computed once per case."""
    at = (geom, n, seed, len(lad))
    if at not in _tables:
        w, h, tile, mv = geom
        buf, stride, types = _bgr(geom, n, seed)
        bgr = torch.stack([buf[f * stride:f * stride + w * h * 3] for f in range(n)]).view(n, h, w, 3).contiguous()
        table = nat.dct_pack_levels_quality_frames(bgr, tile[0], types, mv, lad, 0, distortion=True)[3]
        torch.cuda.synchronize()
        _tables[at] = table.cpu().numpy().view(np.uint64)
    return _tables[at]


def targets_of(geom, n, seed, lad, keys):
    """Group g's targets: every frame's own D at entry (4 g + 5) % K of the reference (with budgets_of's entry (3 g + K / 2) % K and 8
    entries: the first group meets its target under its cap, the second is held finer than its target by the cap)."""
    table = reference_distortion(geom, n, seed, lad)
    out = [0] * n
    for g, (first, end) in enumerate(layers.delta_groups(keys, n)):
        for f in range(first, end):
            out[f] = int(table[f, (4 * g + 5) % len(lad)])
    return nat.target_tensor(out, n, "cuda")


def _builder(flags_cap_and_tables):
    def build(pool, geom, n, seed, k=8):
        w, h, tile, mv = geom
        buf, stride, types = _bgr(geom, n, seed)
        lad = ladder(k)
        arr, _ = nat._ladder(lad)
        full = flags_cap_and_tables
        keys = keys_of(n) if full else None
        ws = pool.buf("workspace", nat.dct_pack_delta_quality_workspace_bytes(n, w, h, tile[0], mv, k), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)
        choice = pool.buf("choice", n, I32)
        counts = pool.buf("counts", (n, k), I32) if full else None
        dist = pool.buf("distortion", (n, k), I64) if full else None
        inputs = {"bgr": buf, "types": types, "target": targets_of(geom, n, seed, lad, keys)}
        if full:
            inputs["budget"] = budgets_of(geom, n, seed, lad, keys)
            inputs["key"] = torch.tensor(keys, dtype=I32, device="cuda")

        def call(i):
            before = out.clone()
            nat._check(nat.load().svc_hip_dct_pack_delta_quality_frames(
                i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, arr, k,
                i["key"].data_ptr() if full else None, i["target"].data_ptr(), i["budget"].data_ptr() if full else None,
                ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(), choice.data_ptr(),
                counts.data_ptr() if full else None, dist.data_ptr() if full else None, nat._stream()))
            _past(ENTRY, (out, offs, before))
            got = {"stream": _stream_out(out, offs), "offsets": offs, "choice": choice}
            if full:
                got["counts"] = counts
                got["distortion"] = dist
            return got
        return inputs, call
    return build


e_dct_pack_delta_quality = _builder(True)
e_dct_pack_delta_quality_plain = _builder(False)
ENTRIES = {ENTRY: (e_dct_pack_delta_quality, GEOMS), ENTRY + "_plain": (e_dct_pack_delta_quality_plain, GEOMS)}


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1, 3, 2):
            for k in (1, 8, 64):
                assert nat.dct_pack_delta_quality_workspace_bytes(n, w, h, tile[0], mv, k) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_poisoned_buffers_and_neighbours(native, geom, entry):
    findings = _check(entry, ENTRIES[entry][0], geom, N, N - 2) + _check(entry, ENTRIES[entry][0], geom, 1, 1)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_ladders_of_1_and_64_entries(native, geom, k):
    """The cases above run with 8 entries; the rows and parts of the workspace and both tables' rows at the two other lengths."""
    findings = _check(ENTRY, e_dct_pack_delta_quality, geom, 3, 2, k=k)
    assert not findings, "\n".join(findings)
