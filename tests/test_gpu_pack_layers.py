"""svc_hip_pack_layers_frames on the device (include/svc_hip.h: both layers of the gaze-scalable stream from raw coefficient planes, for
any geometry the SVCQ pack takes).

Its contract is byte equality: with layers.pack_layers_frames (numpy) on seeded in-range planes for every geometry, density and window
kind; on transform output with svc_hip_pack_levels_frames (the base, byte for byte) and svc_hip_dct_pack_layers_frames (both streams but
the base's inexact count); and under svc_hip_decode_layers_frames bit equality with the decode of the stream packed at (e, e).  Every
call writes into streams pre-filled with FILL and offsets pre-filled with -1; all n + 1 offsets of both layers, the bytes up to the last
one and FILL behind it are asserted."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.helpers import guarded
from tests.test_gpu_dct_pack import FILL, MV16, _content, _types
from tests.test_gpu_layers import _layers, _same_bits, _window
from tests.test_gpu_split_levels import _expect_layer, _host, _rects
from tests.test_gpu_window_levels import HOST_GEOMS, _windows_of
from tests.test_pack_layers_host import STEPS, check_refusals, random_planes
from tests.test_window_levels_host import geom_dict, random_types

pytestmark = pytest.mark.gpu

N = 4


def _call(planes, types, geom, steps, windows=None):
    """The call on device planes (n, 3, h, w) and types (n, MV blocks) i32 -> {base, boffs, enh, eoffs}: whole host arrays and lists."""
    w, h, tile, mv = geom
    n = planes.shape[0]
    cap = nat.levels_max_bytes(n, w, h, tile, mv)
    base = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    enh = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    boffs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    eoffs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    nat.pack_layers_frames(planes, types, tile, mv, *steps, window=_rects(windows, n), base_out=base, enh_out=enh, base_offsets=boffs,
                           enh_offsets=eoffs)
    torch.cuda.synchronize()
    return dict(base=base.cpu().numpy(), boffs=boffs.cpu().tolist(), enh=enh.cpu().numpy(), eoffs=eoffs.cpu().tolist())


# ---- 1. against the numpy statement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", ["zero", "sparse", "full"])
@pytest.mark.parametrize("geom", HOST_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}-{g[3][0]}x{g[3][1]}")
def test_against_the_numpy_statement(native, geom, density):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w * 7 + h + len(density))
    for k, windows in enumerate(_windows_of(geom)):
        steps = STEPS[k % len(STEPS)]  # every triple under at least two window lists
        planes = random_planes(rng, N, w, h, tile, {"zero": 0.0, "sparse": 0.06, "full": 1.0}[density], steps)
        if density == "zero":
            planes[:] = 0
        types = np.stack([random_types(rng, w, h, mv) for _ in range(N)])
        want = layers.pack_layers_frames(planes, types, geom_dict(*geom), *steps, windows)
        got = _call(torch.from_numpy(planes).cuda(), torch.from_numpy(types.astype(np.int32).reshape(N, -1)).cuda(), geom, steps, windows)
        _expect_layer(got["base"], got["boffs"], want[0], want[1])
        _expect_layer(got["enh"], got["eoffs"], want[2], want[3])


# ---- 2. against what exists, on transform output -----------------------------------------------------------------------------------------

ENCODE = [(block, w, h, mv, steps, kind)
          for block, w, h, mv in ((8, 272, 24, (16, 8)), (16, 16, 16, MV16), (16, 48, 32, MV16), (16, 144, 48, MV16))
          for steps in ((1, 640, 1), (4, 16, 2), (3, 9, 1))
          for kind in ("none", "rect", "per-frame")]


def _without_inexact(stream, offs):
    out = np.array(stream, copy=True)
    for o in offs[:-1]:
        out[o + 44:o + 48] = 0
    return out[:offs[-1]].tobytes()


@pytest.mark.parametrize("case", ENCODE, ids=lambda c: "-".join(str(x) for x in c).replace(" ", ""))
def test_transform_output_gives_the_existing_calls_bytes(native, case):
    block, w, h, mv, (fg, bg, e), kind = case
    bgr = _content("random", N, w, h, 11)
    types = _types("random", N, w, h, mv, 11)
    windows = _window(kind, N, w, h, block)
    planes = nat.dct_frames(bgr, block)
    got = _call(planes, types, (w, h, (block, block), mv), (fg, bg, e), windows)
    # the base is the pack's own, inexact count included
    direct = torch.full((nat.levels_max_bytes(N, w, h, block, mv),), FILL, dtype=torch.uint8, device="cuda")
    direct, direct_offs = nat.pack_levels_frames(planes, types, block, mv, fg, bg, out=direct)
    torch.cuda.synchronize()
    _expect_layer(got["base"], got["boffs"], *_host(direct, direct_offs))
    assert any(got["base"][o + 44:o + 48].any() for o in got["boffs"][:-1])  # raw planes: word 11 is not 0
    # both streams are the fused route's, except that word
    want_b, want_boffs, want_e, want_eoffs = _layers(bgr, w * h * 3, N, w, h, block, types, mv, fg, bg, e, windows)
    torch.cuda.synchronize()
    _expect_layer(got["enh"], got["eoffs"], *_host(want_e, want_eoffs))
    assert got["boffs"] == want_boffs.cpu().tolist()
    assert _without_inexact(got["base"], got["boffs"]) == _without_inexact(want_b.cpu().numpy(), got["boffs"])


# ---- 3. through the decoder --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block,w,h,mv", [(8, 272, 24, (16, 8)), (16, 144, 48, MV16)])
@pytest.mark.parametrize("steps", [(1, 640, 1), (4, 16, 2)], ids=str)
def test_decode(native, block, w, h, mv, steps):
    fg, bg, e = steps
    bgr = _content("random" if fg == 1 else "synth", N, w, h, 13)
    types = _types("random", N, w, h, mv, 13)
    planes = nat.dct_frames(bgr, block)
    b, bo, en, eo = nat.pack_layers_frames(planes, types, block, mv, fg, bg, e)
    fine, fine_offs = nat.pack_levels_frames(planes, types, block, mv, e, e)
    torch.cuda.synchronize()
    b, en, fine = b[:int(bo[-1])].clone(), en[:int(eo[-1])].clone(), fine[:int(fine_offs[-1])].clone()
    dec = (2, 24)  # the decoder's steps outside the gaze
    whole = [(0, 0, w, h)] * N
    rec, _, st = nat.decode_layers_frames(b, bo, en, eo, w, h, block, mv, *dec, gaze=whole)
    ref, _, st_ref = nat.decode_levels_frames(fine, fine_offs, w, h, block, mv, *dec, gaze=whole)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st_ref.cpu().tolist() == [0] * N and _same_bits(rec, ref)
    rec, _, st = nat.decode_layers_frames(b, bo, en, eo, w, h, block, mv, *dec, gaze=None)
    ref, _, st_ref = nat.decode_levels_frames(b, bo, w, h, block, mv, *dec, gaze=None)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == st_ref.cpu().tolist() == [0] * N and _same_bits(rec, ref)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(native):
    """The refusals of tests/test_pack_layers_host.py, in their order, with device pointers of a 64 x 64 frame of 8 x 8 tiles: a refused
    call, and the empty batch, leave every buffer as it was."""
    n, w, h = 2, 64, 64
    planes = torch.zeros((n, 3, h, w), dtype=torch.float32, device="cuda")
    types = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
    ws = torch.full((nat.pack_layers_workspace_bytes(n, w, h, 8),), FILL, dtype=torch.uint8, device="cuda")
    cap = nat.levels_max_bytes(n, w, h, 8, 16)
    bufs = [torch.full((cap,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    offs = [torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    check_refusals(planes.data_ptr(), types.data_ptr(), ws.data_ptr(), bufs[0].data_ptr(), offs[0].data_ptr(), bufs[1].data_ptr(),
                   offs[1].data_ptr())
    torch.cuda.synchronize()
    assert all((b == FILL).all() for b in bufs + [ws]) and all((o == -1).all() for o in offs)
    # misaligned pointers are the last refusal
    with pytest.raises(nat.SvcError, match="16-byte aligned"):
        nat.pack_layers_frames(planes, types, 8, 16, 4, 16, 2, base_out=torch.empty(cap + 16, dtype=torch.uint8, device="cuda")[4:])
    assert nat.pack_layers_workspace_bytes(2, 64, 72, 16) == 0 and nat.pack_layers_workspace_bytes(2, 256, 256, 128) == 0


# ---- 5. guards ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [HOST_GEOMS[0], HOST_GEOMS[2], HOST_GEOMS[5]], ids=lambda g: f"{g[0]}x{g[1]}-{g[2][0]}x{g[2][1]}")
def test_writes_stay_inside_buffers_of_exactly_the_size_asked_for(native, geom):
    w, h, tile, mv = geom
    rng = np.random.default_rng(w + h)
    steps = (4, 16, 2)
    planes = torch.from_numpy(random_planes(rng, N, w, h, tile, 0.3, steps)).cuda()
    types = torch.from_numpy(np.stack([random_types(rng, w, h, mv) for _ in range(N)]).astype(np.int32).reshape(N, -1)).cuda()
    windows = _windows_of(geom)[5]
    cap = nat.levels_max_bytes(N, w, h, tile, mv)
    written = {"workspace": guarded.Guarded(nat.pack_layers_workspace_bytes(N, w, h, tile), device="cuda", seed=1),
               "base": guarded.Guarded(cap, device="cuda", seed=2), "enhancement": guarded.Guarded(cap, device="cuda", seed=3),
               "base offsets": guarded.Guarded(8 * (N + 1), torch.int64, "cuda", seed=4),
               "enhancement offsets": guarded.Guarded(8 * (N + 1), torch.int64, "cuda", seed=5)}

    def call():
        b, bo, e, eo = nat.pack_layers_frames(planes, types, tile, mv, *steps, window=_rects(windows, N), base_out=written["base"].interior,
                                              enh_out=written["enhancement"].interior, workspace=written["workspace"].interior,
                                              base_offsets=written["base offsets"].interior,
                                              enh_offsets=written["enhancement offsets"].interior)
        torch.cuda.synchronize()
        return {"base": b[:int(bo[-1])], "base offsets": bo, "enhancement": e[:int(eo[-1])], "enhancement offsets": eo}
    assert guarded.check_writes("svc_hip_pack_layers_frames", written, call, names=("zeros", "ones", "random")) == []
    want = layers.pack_layers_frames(planes.cpu().numpy(), types.cpu().numpy(), geom_dict(*geom), *steps, windows)
    got = call()
    assert got["base"].cpu().numpy().tobytes() == want[0] and got["enhancement"].cpu().numpy().tobytes() == want[2]
