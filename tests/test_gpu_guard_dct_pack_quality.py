"""Where svc_hip_dct_pack_levels_quality_frames (include/svc_hip_quality.h) writes and what its result depends on
(tests/helpers/guarded.py): workspace, output stream, offsets, choices and the table of squared errors of exactly the sizes the API asks
for inside guarded allocations, the four poisons (the leftovers of a call with another frame count and of another entry point among them
-- every count and every sum the selection reads was stored by this call's measuring kernel), and other bytes beside each input -- the
frames, their region ids, the targets and the budgets.  The builder has the form of tests/test_gpu_guard_streams.py's and runs through
its _check; tests/test_gpu_placement_dct_pack_quality.py and tests/test_gpu_stream_order_dct_pack_quality.py take it from here.

Per frame the target is the squared error of another ladder entry (the numpy statement's, on svc_hip_dct_frames' planes) and the budget
the size of another, the last frame's below the masks' floor: the frames of one batch take different entries, by the target and by the
cap.  A second builder runs without the cap and without the table: both pointers NULL."""
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_guard_streams import G8, G16, _bgr, _budgets, _check, _gid, _past, _raw_planes, _stream_out
from tests.test_levels_budget_host import ladder

pytestmark = pytest.mark.gpu

U8, I32, I64 = torch.uint8, torch.int32, torch.int64
N = 5
GEOMS = (G8[0], G16[0])  # 272 x 24 at 8 x 8, 144 x 48 at 16 x 16
ENTRY = "dct_pack_levels_quality"


def targets_of(geom, n, seed, lad):
    """Frame f's target: D[f][(3 f + K / 2) % K] of the statement -> (the targets as the call takes them, the budgets likewise)."""
    w, h, tile, mv = geom
    buf, stride, types = _bgr(geom, n, seed)
    planes = _raw_planes(buf, stride, n, w, h, tile)
    g = dict(frame_w=w, frame_h=h, block_w=tile[0], block_h=tile[1], mv_block_w=mv[0], mv_block_h=mv[1])
    d = layers.distortion_table(planes.cpu().numpy(), types.cpu().numpy(), g, lad)
    target = [int(d[f, (3 * f + len(lad) // 2) % len(lad)]) for f in range(n)]
    return nat.target_tensor(target, n, "cuda"), _budgets(planes, types, tile, mv, lad)


def _builder(capped_with_table):
    def build(pool, geom, n, seed, k=8):
        w, h, tile, mv = geom
        buf, stride, types = _bgr(geom, n, seed)
        lad = ladder(k)
        arr, _ = nat._ladder(lad)
        target, budget = targets_of(geom, n, seed, lad)
        ws = pool.buf("workspace", nat.dct_pack_levels_quality_workspace_bytes(n, w, h, tile[0], mv, k), U8)
        out = pool.buf("stream", nat.levels_max_bytes(n, w, h, tile, mv), U8)
        offs = pool.buf("offsets", n + 1, I64)
        choice = pool.buf("choice", n, I32)
        table = pool.buf("distortion", (n, k), I64) if capped_with_table else None
        inputs = {"bgr": buf, "types": types, "target": target}
        if capped_with_table:
            inputs["budget"] = budget

        def call(i):
            before = out.clone()
            nat._check(nat.load().svc_hip_dct_pack_levels_quality_frames(
                i["bgr"].data_ptr(), stride, n, w, h, tile[0], i["types"].data_ptr(), *mv, arr, k, i["target"].data_ptr(),
                i["budget"].data_ptr() if capped_with_table else None, ws.data_ptr(), ws.numel(), out.data_ptr(), out.numel(), offs.data_ptr(),
                choice.data_ptr(), table.data_ptr() if capped_with_table else None, nat._stream()))
            _past(ENTRY, (out, offs, before))
            got = {"stream": _stream_out(out, offs), "offsets": offs, "choice": choice}
            if capped_with_table:
                got["distortion"] = table
            return got
        return inputs, call
    return build


e_dct_pack_levels_quality = _builder(True)
e_dct_pack_levels_quality_plain = _builder(False)
ENTRIES = {ENTRY: (e_dct_pack_levels_quality, GEOMS), ENTRY + "_plain": (e_dct_pack_levels_quality_plain, GEOMS)}


def test_every_case_is_sized(native):
    """No case below is a refusal in disguise."""
    for w, h, tile, mv in GEOMS:
        for n in (N, N - 2, 1, 3, 2):
            for k in (1, 8, 64):
                assert nat.dct_pack_levels_quality_workspace_bytes(n, w, h, tile[0], mv, k) > 0 and nat.levels_max_bytes(n, w, h, tile, mv) > 0


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_poisoned_buffers_and_neighbours(native, geom, entry):
    findings = _check(entry, ENTRIES[entry][0], geom, N, N - 2) + _check(entry, ENTRIES[entry][0], geom, 1, 1)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_ladders_of_1_and_64_entries(native, geom, k):
    """The cases above run with 8 entries; the per-entry arrays of the workspace and the table's rows at the two other lengths."""
    findings = _check(ENTRY, e_dct_pack_levels_quality, geom, 3, 2, k=k)
    assert not findings, "\n".join(findings)
