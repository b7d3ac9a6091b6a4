"""svc_hip_dct_pack_levels_quality_frames (include/svc_hip_quality.h: a distortion target inside the fused transform) without a device:
the numpy statement's identities (layers.quantisation_error, distortion_table, quality_choice, distortion_target, distortion_psnr), every
branch of the choice on hand-made tables, and what the C ABI answers before it reaches a kernel.  What the kernels write is
tests/test_gpu_dct_pack_quality.py."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from scalable_video_codec_amd import layers, levels, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svc_hip_quality.h")
LADDER32 = levels.step_ladder(1, 256, 4, 640, 10, 24)
OVER, UNMET = 0x80000000, 0x40000000


def geometry(w, h, block, mv=16):
    return dict(frame_w=w, frame_h=h, block_w=block, block_h=block, mv_block_w=mv, mv_block_h=mv)


def random_planes(rng, w, h):
    """Coefficient-like f32 values over the range a transform reaches: mostly small, some large, zeros and both signs."""
    c = rng.standard_normal((1, 3, h, w)) * rng.choice([0.3, 4.0, 60.0, 900.0], (1, 3, h, w))
    c[rng.random(c.shape) < 0.05] = 0.0
    return np.clip(c, -4080, 4080).astype(np.float32)


def test_the_error_is_an_f32_for_every_coefficient_and_entry():
    rng = np.random.default_rng(7)
    planes = random_planes(rng, 64, 48)
    assert LADDER32.shape == (32, 2)
    for step in sorted({int(s) for s in LADDER32.ravel()} | {2, 3, 5, 4081, 9000}):
        x = layers.quantisation_error(planes, step)
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x), step                 # representable: one fma gives it
        assert np.array_equal(np.rint(256.0 * x), np.rint((256.0 * x).astype(np.float32))), step  # and 256 x is exact as well
        assert np.abs(x).max() <= step / 2 * (1 + 2.0 ** -10), step  # (the f32 quotient can round a near-tie up: 4080 * 2^-24 of a step)


def test_a_step_above_every_coefficient_leaves_the_coefficients_themselves():
    rng = np.random.default_rng(8)
    planes = random_planes(rng, 32, 32)
    types = rng.integers(0, 3, (1, 2, 2))
    top = int(2 * np.abs(planes).max()) + 2
    d = layers.distortion_table(planes, types, geometry(32, 32, 8), [(top, top), (top, top + 5)])
    e = np.rint(256.0 * planes.astype(np.float64)).astype(np.int64)
    assert d.dtype == np.uint64 and d.shape == (1, 2)
    assert int(d[0, 0]) == int(d[0, 1]) == int((e * e).sum())


def test_a_one_entry_ladder_and_the_class_rule():
    rng = np.random.default_rng(9)
    planes = random_planes(rng, 32, 32)
    types = np.array([[[0, 2], [1, 0]]])
    g = geometry(32, 32, 8)
    one = layers.distortion_table(planes, types, g, [(3, 40)])
    assert one.shape == (1, 1)
    # by hand: type 0 takes bg_step, per 16x16 MV block
    step = np.repeat(np.repeat(np.where(types[0] == 0, 40, 3), 16, 0), 16, 1)[None]
    e = np.rint(256.0 * layers.quantisation_error(planes[0], step)).astype(np.int64)
    assert int(one[0, 0]) == int((e * e).sum())
    both = layers.distortion_table(planes, types, g, [(3, 40), (3, 40)])
    assert both[0].tolist() == [int(one[0, 0])] * 2


@pytest.mark.parametrize("w,h", [(64, 64), (1920, 1088), (3840, 2176)])
def test_target_and_psnr_are_inverse_at_the_boundary(w, h):
    import decimal
    scale = 255 * 255 * 3 * w * h * 65536
    for db in (20, 30.0, 37.5, 40, 46.25, 60):
        t = layers.distortion_target(db, w, h)
        with decimal.localcontext() as ctx:  # the definition, in exact arithmetic: t reaches the PSNR and t + 1 does not
            ctx.prec = 80
            ratio = decimal.Decimal(10) ** (decimal.Decimal(db) / 10)
            assert decimal.Decimal(scale) / t >= ratio > decimal.Decimal(scale) / (t + 1)
        assert layers.distortion_psnr(t, w, h) == pytest.approx(db, abs=1e-6)
        assert layers.distortion_psnr(t, w, h) > layers.distortion_psnr(t + max(1, t >> 30), w, h)
    assert layers.distortion_psnr(0, w, h) == float("inf")
    assert layers.distortion_target(-1000, w, h) == 2 ** 64 - 1  # capped to the field
    assert layers.distortion_target(400, w, h) == 0


def _dct_matrix(n):
    k, i = np.arange(n)[:, None], np.arange(n)[None, :]
    m = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * i + 1) * k / (2 * n))
    m[0] /= np.sqrt(2.0)
    return m


@pytest.mark.parametrize("block", [8, 16])
def test_parseval_the_table_is_the_pictures_squared_error(block):
    """A condition against a wrong scale or a missing plane, not a precision pin: D / 65536 within 1 % of the f64 squared error of the
    dequantised picture in the pixel domain (measured: 2.4e-5 at worst; one plane of three missing is 33 %).  Pixels from 32 .. 223, so no
    reconstruction clips."""
    rng = np.random.default_rng(10 + block)
    w, h = 64, 48
    bgr = rng.integers(32, 224, (h, w, 3), dtype=np.uint8)
    m = _dct_matrix(block)
    src = bgr.transpose(2, 0, 1).astype(np.float64).reshape(3, h // block, block, w // block, block).transpose(0, 1, 3, 2, 4)
    planes = (m @ src @ m.T).transpose(0, 1, 3, 2, 4).reshape(1, 3, h, w).astype(np.float32)  # the orthonormal transform, rounded to f32
    types = rng.integers(0, 2, (1, h // 16, w // 16))
    g = geometry(w, h, block)
    ladder = [(1, 1), (3, 3), (1, 640)]
    table = layers.distortion_table(planes, types, g, ladder)
    background = np.repeat(np.repeat(types[0] == 0, 16, 0), 16, 1)[None]
    for k, (fg, bg) in enumerate(ladder):
        step = np.where(background, bg, fg)
        deq = (layers.quantise(planes[0], step) * step).astype(np.float64)
        tiles = deq.reshape(3, h // block, block, w // block, block).transpose(0, 1, 3, 2, 4)
        rec = (m.T @ tiles @ m).transpose(0, 1, 3, 2, 4).reshape(3, h, w)
        sse = float(((rec - bgr.transpose(2, 0, 1).astype(np.float64)) ** 2).sum())
        got = int(table[0, k]) / 65536.0
        print(f"block {block} entry {ladder[k]}: D / 65536 = {got:.3f}, pixel-domain SSE = {sse:.3f}, relative {abs(got - sse) / sse:.2e}")
        assert abs(got - sse) <= 0.01 * sse, (block, k, got, sse)


def test_every_branch_of_the_choice():
    sizes = np.array([[1000, 800, 600, 400, 200]])
    mono = np.array([[10, 20, 30, 40, 50]], np.uint64)
    choose = layers.quality_choice
    assert choose(mono, sizes, 5).tolist() == [0 | UNMET]                   # no entry meets: entry 0, flagged
    assert choose(mono, sizes, 50).tolist() == [4]                          # all meet: the coarsest
    assert choose(mono, sizes, 2 ** 64 - 1).tolist() == [4]
    assert choose(mono, sizes, 30).tolist() == [2]                          # equality meets
    assert choose(mono, sizes, 29).tolist() == [1]
    assert choose(mono, sizes, 0).tolist() == [0 | UNMET]
    bumpy = np.array([[10, 40, 20, 50, 30]], np.uint64)                     # not monotone: first failure at 1, largest k that meets: 4
    first_failure = next(k for k in range(5) if int(bumpy[0, k]) > 30) - 1
    assert first_failure == 0 and choose(bumpy, sizes, 30).tolist() == [4]
    assert choose(bumpy, sizes, 25).tolist() == [2]
    # the cap: kb below kq changes nothing; kb above kq wins and the target is no longer met; over budget: the last entry, both flags
    assert choose(mono, sizes, 30, 800).tolist() == [2]                     # kb = 1 < kq = 2
    assert choose(mono, sizes, 30, 600).tolist() == [2]                     # kb = kq
    assert choose(mono, sizes, 30, 400).tolist() == [3 | UNMET]             # kb = 3 > kq = 2
    assert choose(mono, sizes, 50, 400).tolist() == [4]                     # kb = 3 < kq = 4: met
    assert choose(mono, sizes, 30, 100).tolist() == [4 | OVER | UNMET]      # over budget, quality not met
    assert choose(mono, sizes, 50, 100).tolist() == [4 | OVER]              # over budget, quality met
    assert choose(bumpy, sizes, 30, 400).tolist() == [4]                    # kb = 3 (D = 50 alone would miss) but kq = 4 is coarser
    assert choose(mono, sizes, 5, 0xFFFFFFFF).tolist() == [0 | UNMET]
    # per frame targets and budgets
    two = np.vstack([mono, bumpy])
    assert choose(two, np.vstack([sizes, sizes]), [30, 25], [400, 1000]).tolist() == [3 | UNMET, 2]
    assert choose(two, np.vstack([sizes, sizes]), [30, 25]).tolist() == [2, 2]
    assert choose(np.array([[7]], np.uint64), [[64]], 7, 64).tolist() == [0]  # a one-entry ladder
    assert choose(np.array([[7]], np.uint64), [[64]], 6, 48).tolist() == [0 | OVER | UNMET]


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def test_every_declaration_is_exported_and_bound_with_its_stream_last():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(svc_hip_\w+)\s*\(", text)
    assert sorted(declared) == sorted(native.SIGNATURES_QUALITY) == ["svc_hip_dct_pack_levels_quality_frames",
                                                                    "svc_hip_dct_pack_levels_quality_workspace_bytes"]
    lib = native.load()
    for name, (res, args) in native.SIGNATURES_QUALITY.items():
        fn = getattr(lib, name)  # exported
        assert fn.restype is res and list(fn.argtypes) == args
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        assert len(params) == len(args), name
    assert re.search(r"void\s*\*\s*stream\s*\)\s*;", text) and native.SIGNATURES_QUALITY["svc_hip_dct_pack_levels_quality_frames"][1][-1] is native._vp
    # the budgeted call's arguments with the target in front of the budget and the table behind the choice
    b = native.SIGNATURES["svc_hip_dct_pack_levels_budget_frames"][1]
    assert native.SIGNATURES_QUALITY["svc_hip_dct_pack_levels_quality_frames"][1] == b[:11] + [native._vp] + b[11:-1] + [native._vp] + b[-1:]
    assert not set(native.SIGNATURES_QUALITY) & set(native.SIGNATURES)
    assert lib.svc_hip_abi_version() == 5


def test_workspace_query_is_zero_where_the_call_refuses():
    q = native.dct_pack_levels_quality_workspace_bytes
    assert q(2, 64, 64, 4, 16, 8) == 0           # a 4x4 block: not the tuned transform
    assert q(2, 72, 64, 8, 8, 8) == 0            # a width of 4.5 segments
    assert q(2, 64, 64, 8, (12, 16), 8) == 0     # an MV block that is not a multiple of the tile
    assert q(2, 64, 64, 16, (16, 8), 8) == 0
    assert q(2, 64, 64, 8, 16, 0) == 0           # a ladder of 1 .. 64 entries
    assert q(2, 64, 64, 8, 16, 65) == 0
    assert q(70000, 64, 64, 8, 16, 8) == 0       # more frames than one call takes
    assert q(1, 32768, 32768, 16, 16, 8) == 0    # a frame beyond the u32 frame_bytes field: the bound that keeps the u64 sums safe
    for n, w, h, block, mv in ((2, 64, 64, 8, 16), (1, 3840, 2176, 16, 16), (3, 272, 24, 8, (16, 8))):
        for k in (1, 8, 64):
            assert q(n, w, h, block, mv, k) > native.dct_pack_levels_budget_workspace_bytes(n, w, h, block, mv, k) > 0  # it holds that call's


def test_argument_checks_answer_without_a_device():
    """Every pointer is NULL: the checks below all come before the pointer checks, in the budgeted call's order, and the null-pointer
    check stands between any of them and a launch."""
    lib = native.load()

    def err():
        return lib.svc_hip_last_error().decode()

    def call(w, h, block, mbw, mbh, ladder, n=2, ws=1 << 40, cap=1 << 40, stride=None):
        stride = w * h * 3 if stride is None else stride
        arr, k = native._ladder(ladder)
        return lib.svc_hip_dct_pack_levels_quality_frames(None, stride, n, w, h, block, None, mbw, mbh, arr, k, None, None, None, ws, None, cap,
                                                          None, None, None, None)
    good = [(1, 640), (2, 640), (2, 700)]
    bad, unsup = native.SVC_ERR_INVALID_ARG, native.SVC_ERR_UNSUPPORTED
    for n in (2, 0):  # the contract does not depend on n_frames
        assert call(100, 64, 8, 16, 16, good, n=n) == bad and "not divisible" in err()
        assert call(64, 64, 8, 12, 16, good, n=n) == bad and "multiple of the tile" in err()
        assert call(48, 48, 12, 12, 12, good, n=n) == unsup and "8x8, 16x16" in err()
        assert call(72, 64, 8, 8, 8, good, n=n) == unsup and "multiple of 16" in err()
        assert call(72, 64, 8, 8, 8, [(0, 640)], n=n) == unsup and "multiple of 16" in err()  # geometry before the ladder
        assert call(64, 64, 8, 16, 16, [(0, 640)], n=n, stride=64 * 64 * 3 - 16) == bad and "stride" in err()  # the stride before the ladder
        assert call(64, 64, 8, 16, 16, [], n=n, ws=0, cap=0) == bad and "ladder of 0 entries" in err()  # the ladder before any size
        assert call(64, 64, 8, 16, 16, [(1, 640)] * 65, n=n) == bad and "ladder of 65 entries" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (0, 640)], n=n, ws=0, cap=0) == bad and "steps must be positive" in err()
        assert call(64, 64, 8, 16, 16, [(2, 640), (1, 640)], n=n, ws=0, cap=0) == bad and "non-decreasing" in err()
        assert call(64, 64, 8, 16, 16, [(1, 640), (2, 639)], n=n, ws=0, cap=0) == bad and "non-decreasing" in err()
        assert "dct_pack_levels_quality" in err()
        assert call(32768, 32768, 16, 16, 16, good, n=n, ws=0, cap=0) == unsup and "frame_bytes" in err()  # 2^31 coefficients and more: refused
    assert call(64, 64, 8, 16, 16, good, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch, every pointer NULL
    assert call(64, 64, 16, 16, 16, [(3, 17)], n=0) == native.SVC_OK
    assert call(64, 64, 8, 16, 16, good, n=70000, ws=0, cap=0) == unsup and "65535 frames" in err()  # limits before sizes
    need_ws = native.dct_pack_levels_quality_workspace_bytes(2, 64, 64, 8, 16, len(good))
    need_out = native.levels_max_bytes(2, 64, 64, 8, 16)
    assert call(64, 64, 8, 16, 16, good, ws=need_ws - 1, cap=0) == bad and "workspace" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out - 16) == bad and "worst case" in err()
    assert call(64, 64, 8, 16, 16, good, ws=need_ws, cap=need_out) == bad and "null pointer" in err()


def test_target_tensor_refuses_what_is_not_a_u64():
    with pytest.raises(ValueError):
        native.target_tensor(-1, 2, "cpu")
    with pytest.raises(ValueError):
        native.target_tensor([0, 2 ** 64], 2, "cpu")
    t = native.target_tensor([0, 2 ** 64 - 1, 2 ** 63], 3, "cpu")
    assert t.dtype.is_floating_point is False and t.numpy().view(np.uint64).tolist() == [0, 2 ** 64 - 1, 2 ** 63]
    assert native.target_tensor(5, 3, "cpu").tolist() == [5, 5, 5]
