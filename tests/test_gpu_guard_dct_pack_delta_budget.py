"""Where svc_hip_dct_pack_delta_budget_frames (include/svc_hip_delta_budget.h) writes and what its result depends on
(tests/helpers/guarded.py): workspace, output stream, offsets, choices and the table of counts of exactly the sizes the API asks for
inside guarded allocations, the four poisons (the leftovers of a call with another frame count and of another entry point among them --
every row the sum reads and every part and step the later launches read was stored by this call's own kernels), and other bytes beside
each input -- the frames, their region ids, the key flags and the budgets.  The builder has the form of
tests/test_gpu_guard_streams.py's and runs through its _check; tests/test_gpu_placement_dct_pack_delta_budget.py and
tests/test_gpu_stream_order_dct_pack_delta_budget.py take it from here.

The flags cut a batch into groups of two frames; per group the budget is the group's bytes at another ladder entry of the reference
(svc_hip_dct_pack_levels_frames, then svc_hip_delta_levels_frames, per entry), the last group's 0: the groups of one batch take different
entries and the last is over budget.  A second builder runs without flags and without the table: both pointers NULL."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import G8, G16, _bgr, _check, _gid, _past, _stream_out
from tests.test_levels_budget_host import frame_floor, ladder

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
N = 5
GEOMS = (G8[0], G16[0])  # 272 x 24 at 8 x 8, 144 x 48 at 16 x 16
ENTRY = "dct_pack_delta_budget"
_tables = {}


def keys_of(n):
    return [1 if f and f % 2 == 0 else 0 for f in range(n)]  # groups of two frames (the last of one where n is odd)


def reference_table(geom, n, seed, lad, keys):
    """count[f][k] from calls the one under test shares no kernel with -> (n, K) u32; computed once per case."""
    at = (geom, n, seed, len(lad), None if keys is None else tuple(keys))
    if at not in _tables:
        w, h, tile, mv = geom
        buf, stride, types = _bgr(geom, n, seed)
        bgr = torch.stack([buf[f * stride:f * stride + w * h * 3] for f in range(n)]).view(n, h, w, 3).contiguous()
        floor = frame_floor(w, h, tile[0], tile[1], mv[0], mv[1])
        cols = []
        for fg, bg in lad:
            d, d_offs, st = nat.delta_levels_frames(*nat.dct_pack_levels_frames(bgr, tile[0], types, mv, int(fg), int(bg)), w, h, tile, mv, key=keys)
            torch.cuda.synchronize()
            assert st.cpu().tolist() == [0] * n
            o = d_offs.cpu().numpy()
            cols.append([int(np.frombuffer(d[int(o[f]):int(o[f]) + 64].cpu().numpy().tobytes(), "<u4")[10]) for f in range(n)])
            assert [(floor + 2 * c + 15) // 16 * 16 for c in cols[-1]] == np.diff(o).tolist()
        _tables[at] = np.array(cols, np.uint32).T.reshape(n, len(lad))
    return _tables[at]


def budgets_of(geom, n, seed, lad, keys):
    """Group g's budget: its bytes at entry (3 g + K / 2) % K of the reference, all of it on the group's first frame; the last group of a
    batch of more than one group: 0."""
    w, h, tile, mv = geom
    table = reference_table(geom, n, seed, lad, keys)
    size = (frame_floor(w, h, tile[0], tile[1], mv[0], mv[1]) + 2 * table.astype(np.int64) + 15) // 16 * 16
    groups = layers.delta_groups(keys, n)
    out = [0] * n
    for g, (first, end) in enumerate(groups):
        if len(groups) > 1 and g == len(groups) - 1:
            continue
        out[first] = int(size[first:end].sum(axis=0)[(3 * g + len(lad) // 2) % len(lad)])
    return nat.budget_tensor(out, n, "cuda")


def _builder(flags_and_table):
    def build(pool, geom, n, seed, k=8):
        w, h, tile, mv = geom
        buf, stride, types = _bgr(geom, n, seed)
        lad = ladder(k)
        arr, _ = nat._ladder(lad)
        keys = keys_of(n) if flags_and_table else None
        ws = pool.buf("workspace", nat.dct_pack_delta_budget_workspace_bytes(n, w, h, tile[0], mv, k), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)
        choice = pool.buf("choice", n, I32)
        table = pool.buf("counts", (n, k), I32) if flags_and_table else None
        inputs = {"bgr": buf, "types": types, "budget": budgets_of(geom, n, seed, lad, keys)}
        if flags_and_table:
            inputs["key"] = torch.tensor(keys, dtype=I32, device="cuda")

        def call(i):
            before = out.clone()
            nat._check(nat.load().svc_hip_dct_pack_delta_budget_frames(
                i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, arr, k,
                i["key"].data_ptr() if flags_and_table else None, i["budget"].data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(),
                offs.data_ptr(), choice.data_ptr(), table.data_ptr() if flags_and_table else None, nat._stream()))
            _past(ENTRY, (out, offs, before))
            got = {"stream": _stream_out(out, offs), "offsets": offs, "choice": choice}
            if flags_and_table:
                got["counts"] = table
            return got
        return inputs, call
    return build


e_dct_pack_delta_budget = _builder(True)
e_dct_pack_delta_budget_plain = _builder(False)
ENTRIES = {ENTRY: (e_dct_pack_delta_budget, GEOMS), ENTRY + "_plain": (e_dct_pack_delta_budget_plain, GEOMS)}


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1, 3, 2):
            for k in (1, 8, 64):
                assert nat.dct_pack_delta_budget_workspace_bytes(n, w, h, tile[0], mv, k) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_poisoned_buffers_and_neighbours(native, geom, entry):
    findings = _check(entry, ENTRIES[entry][0], geom, N, N - 2) + _check(entry, ENTRIES[entry][0], geom, 1, 1)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_ladders_of_1_and_64_entries(native, geom, k):
    """The cases above run with 8 entries; the rows and parts of the workspace and the table's rows at the two other lengths."""
    findings = _check(ENTRY, e_dct_pack_delta_budget, geom, 3, 2, k=k)
    assert not findings, "\n".join(findings)
