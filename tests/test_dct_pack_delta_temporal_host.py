"""The entry points of include/svc_hip_temporal.h (the temporal-layer delta stream straight from the transform kernel): what they answer
without a device -- that they are exported and bound from native.SIGNATURES_TEMPORAL while include/svc_hip.h, native.SIGNATURES and the
ABI version stay as they are, the workspace queries, the order of the argument checks with the period right after the geometry, and the
pairing of d_prev_bgr with d_prev_types.  Then the census tests/test_stream_order_host.py keeps for include/svc_hip.h, restated for
this header: every declaration with a `void* stream` is bound and named by a case of
tests/test_gpu_stream_order_dct_pack_delta_temporal.py.  Last, the numpy statement's `period` keyword (layers.delta_level_counts,
layers.delta_auto_frames): period 1 is the old result, and flags, counts and bytes thin as the stream does.  The bytes the calls
write are tests/test_gpu_dct_pack_delta_temporal.py and tests/test_gpu_dct_pack_delta_temporal_auto.py."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

from scalable_video_codec_amd import layers, native
from tests.helpers import stream_order as so
from tests.test_window_levels_host import random_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "svc_hip_temporal.h")
NAMES = ("svc_hip_dct_pack_delta_temporal_workspace_bytes", "svc_hip_dct_pack_delta_temporal_frames",
         "svc_hip_dct_pack_delta_temporal_auto_workspace_bytes", "svc_hip_dct_pack_delta_temporal_auto_frames")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_symbols_are_exported_and_bound():
    lib = native.load()
    assert set(native.SIGNATURES_TEMPORAL) == set(NAMES)
    assert not set(native.SIGNATURES_TEMPORAL) & set(native.SIGNATURES)
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is native.SIGNATURES_TEMPORAL[name][0] and list(fn.argtypes) == list(native.SIGNATURES_TEMPORAL[name][1]), name
    for name in ("dct_pack_delta_temporal_frames", "dct_pack_delta_temporal_auto_frames", "dct_pack_delta_temporal_workspace_bytes",
                 "dct_pack_delta_temporal_auto_workspace_bytes"):
        assert callable(getattr(native, name)), name


def test_the_abi_version_and_the_main_header_stay():
    assert native.load().svc_hip_abi_version() == 5
    with open(os.path.join(ROOT, "include", "svc_hip.h")) as f:
        assert "dct_pack_delta_temporal" not in f.read()
    text = so.strip_comments(_header())
    assert '#include "svc_hip.h"' in text
    declared = {n for n in NAMES if n + "(" in text.replace(" (", "(")}
    assert declared == set(NAMES)


def test_every_stream_declaration_of_the_header_is_bound_and_has_a_case():
    """The census of tests/test_stream_order_host.py for this header: declared with a `void* stream` == bound with a stream there ==
    reached by a case of the stream-order file; and the signature takes its stream where the header declares it, the period last."""
    from tests import test_gpu_stream_order_dct_pack_delta_temporal as cases
    declared = so.header_stream_params(_header())
    assert set(declared) == {"svc_hip_dct_pack_delta_temporal_frames", "svc_hip_dct_pack_delta_temporal_auto_frames"}
    assert set(declared) <= set(native.SIGNATURES_TEMPORAL)
    assert cases.covered() == set(declared)
    for name, (at, count) in declared.items():
        res, args = native.SIGNATURES_TEMPORAL[name]
        assert res is C.c_int and len(args) == count and args[at] is C.c_void_p and at == count - 2 and args[-1] is C.c_uint32, name
    # the functions without a stream are the queries
    for name in set(native.SIGNATURES_TEMPORAL) - set(declared):
        res, args = native.SIGNATURES_TEMPORAL[name]
        assert res is C.c_uint64 and all(a is C.c_uint32 for a in args) and len(args) == 7, name
    # every case runs both periods on both geometries
    assert len(cases.CASES) == 8 and {c[-len("272x24-8x8-mv16x8"):] for c in cases.CASES if "272" in c} == {"272x24-8x8-mv16x8"}


def _err():
    return native.load().svc_hip_last_error().decode()


def _fixed(w, h, block, mbw, mbh, fg, bg, period, n=2, ws=1 << 40, cap=1 << 40, ptrs=(None,) * 8):
    """ptrs: d_bgr, d_block_types, d_prev_bgr, d_prev_types, d_key, d_workspace, d_out, d_frame_offsets."""
    bgr, types, pbgr, ptypes, key, wsp, out, offs = ptrs
    return native.load().svc_hip_dct_pack_delta_temporal_frames(bgr, w * h * 3, n, w, h, block, types, mbw, mbh, fg, bg, pbgr, ptypes, key, wsp,
                                                                ws, out, cap, offs, None, period)


def _auto(w, h, block, mbw, mbh, fg, bg, period, n=2, ws=1 << 40, cap=1 << 40, ptrs=(None,) * 8, key_out=None):
    """ptrs as _fixed's, d_forced in d_key's place; then d_key_out (d_level_counts stays NULL)."""
    bgr, types, pbgr, ptypes, forced, wsp, out, offs = ptrs
    return native.load().svc_hip_dct_pack_delta_temporal_auto_frames(bgr, w * h * 3, n, w, h, block, types, mbw, mbh, fg, bg, pbgr, ptypes, forced,
                                                                     wsp, ws, out, cap, offs, key_out, None, None, period)


@pytest.mark.parametrize("call", [_fixed, _auto], ids=["fixed", "auto"])
def test_the_period_is_checked_right_after_the_geometry(call):
    """Every pointer is NULL: all of this is answered in front of the pointer checks, so nothing reaches a kernel."""
    for n in (2, 0):
        for period in (0, 3, 8):
            assert call(64, 64, 8, 16, 16, 1, 640, period, n=n) == native.SVC_ERR_INVALID_ARG and "period" in _err()
            # geometry before period
            assert call(100, 64, 8, 16, 16, 1, 640, period, n=n) == native.SVC_ERR_INVALID_ARG and "not divisible" in _err()
            assert call(64, 64, 4, 16, 16, 1, 640, period, n=n) == native.SVC_ERR_UNSUPPORTED and "8x8, 16x16" in _err()
            assert call(72, 64, 8, 8, 8, 1, 640, period, n=n) == native.SVC_ERR_UNSUPPORTED and "multiple of 16" in _err()
            # period before steps, limits and sizes
            assert call(64, 64, 8, 16, 16, 0, 640, period, n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "period" in _err()
        assert call(64, 64, 8, 16, 16, 1, 640, 3, n=70000) == native.SVC_ERR_INVALID_ARG and "period" in _err()
        for period in (1, 2, 4):  # then the delta call's own order
            assert call(64, 64, 8, 16, 16, 0, 640, period, n=n, ws=0, cap=0) == native.SVC_ERR_INVALID_ARG and "steps must be positive" in _err()
    for period in (1, 2, 4):
        assert call(64, 64, 8, 16, 16, 1, 640, period, n=0, ws=0, cap=0) == native.SVC_OK  # a valid empty batch
        assert call(64, 64, 8, 16, 16, 1, 640, period, n=70000) == native.SVC_ERR_UNSUPPORTED and "65535 frames" in _err()
        assert call(64, 64, 8, 16, 16, 1, 640, period, ws=15, cap=0) == native.SVC_ERR_INVALID_ARG and "workspace" in _err()
        assert call(64, 64, 8, 16, 16, 1, 640, period) == native.SVC_ERR_INVALID_ARG and "null pointer" in _err()


def test_workspace_queries():
    q, qa = native.dct_pack_delta_temporal_workspace_bytes, native.dct_pack_delta_temporal_auto_workspace_bytes
    for period in (0, 3, 8):
        assert q(2, 64, 64, 8, 16, period) == 0 and "period" in _err()
        assert qa(2, 64, 64, 8, 16, period) == 0 and "period" in _err()
    for period in (1, 2, 4):
        assert q(2, 64, 64, 4, 16, period) == 0 and qa(2, 72, 64, 8, 8, period) == 0 and q(70000, 64, 64, 8, 16, period) == 0
        # the kept frames live in registers: the delta calls' scratch, whatever the period
        assert q(9, 272, 24, 8, (16, 8), period) == native.dct_pack_delta_workspace_bytes(9, 272, 24, 8, (16, 8)) > 0
        assert qa(9, 272, 24, 8, (16, 8), period) == native.dct_pack_delta_auto_workspace_bytes(9, 272, 24, 8, (16, 8)) > 0
    assert q(2, 100, 64, 8, 16, 3) == 0 and "not divisible" in _err()  # geometry before period


@pytest.mark.parametrize("period", [1, 2, 4])
def test_the_frame_in_front_is_pixels_and_types_together(period):
    a = 0x10000  # 16-byte aligned, never dereferenced
    base = [a, a, None, None, None, a, a, a]

    def both(**over):
        p = list(base)
        for k, v in over.items():
            p[{"bgr": 0, "types": 1, "pbgr": 2, "ptypes": 3, "key": 4}[k]] = v
        return (_fixed(64, 64, 8, 16, 16, 1, 640, period, ptrs=tuple(p)), _err()), (_auto(64, 64, 8, 16, 16, 1, 640, period, ptrs=tuple(p), key_out=a), _err())
    for rc, err in both(pbgr=a) + both(ptypes=a):
        assert rc == native.SVC_ERR_INVALID_ARG and "together" in err
    for rc, err in both(pbgr=a + 8, ptypes=a) + both(pbgr=a, ptypes=a + 2) + both(key=a + 2):
        assert rc == native.SVC_ERR_INVALID_ARG and "aligned" in err
    for rc, err in both(bgr=None, pbgr=a):  # a missing required pointer is reported before the pairing
        assert rc == native.SVC_ERR_INVALID_ARG and "null pointer" in err
    # and a lone d_prev_bgr at a refused period is the period's refusal
    assert _fixed(64, 64, 8, 16, 16, 1, 640, 3, ptrs=(a, a, a, None, None, a, a, a)) == native.SVC_ERR_INVALID_ARG and "period" in _err()


# ---- the numpy statement's period -------------------------------------------------------------------------------------------------------------

GEOM = (48, 16, (8, 8), (16, 16))


def _clip(n, seed):
    """n + 1 SVCQ frames of one geometry with sparse random levels; consecutive and alternate frames share most of them, so that
    differences are smaller than frames at some places and not at others."""
    rng = np.random.default_rng(seed)
    stream, offs = random_stream(rng, GEOM, n + 1, 0.08)
    return np.frombuffer(bytes(stream), np.uint8), np.asarray(offs, np.uint64)


def _frames(stream, offs):
    return [bytes(stream[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]


def _join(frames):
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    return np.frombuffer(b"".join(frames), np.uint8), offs


def _repeating(n, seed):
    """Frames built so that both outcomes occur under every period: frame i is one of three random frames, by a pattern with equal
    frames 1, 2 and 4 apart."""
    stream, offs = _clip(3, seed)
    base = _frames(stream, offs)
    pattern = [0, 0, 1, 0, 0, 2, 0, 1, 1, 1, 2, 0, 2, 2, 0, 1, 0, 0, 0, 1]
    return [base[pattern[i % len(pattern)]] for i in range(n + 1)]


def test_period_1_is_the_old_result():
    frames = _repeating(11, 1)
    stream, offs = _join(frames[1:])
    for prev in (None, frames[0]):
        old = layers.delta_level_counts(stream, offs, prev)
        assert np.array_equal(layers.delta_level_counts(stream, offs, prev, period=1), old)
        assert np.array_equal(layers.delta_level_counts(stream, offs, prev=prev, period=1), old)
        a, b = layers.delta_auto_frames(stream, offs, None, prev), layers.delta_auto_frames(stream, offs, None, prev, period=1)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
        want = layers.delta_frames(stream, offs, a[2], prev)
        assert a[0] == want[0]
    with pytest.raises(ValueError):
        layers.delta_level_counts(stream, offs, period=3)


@pytest.mark.parametrize("period", [2, 4])
def test_counts_and_keys_follow_the_temporal_reference(period):
    n = 19
    frames = _repeating(n, 2)
    stream, offs = _join(frames[1:])
    for prev in (None, frames[0]):
        counts = layers.delta_level_counts(stream, offs, prev, period=period)
        for i in range(n):
            ref = (frames[1 + layers.temporal_ref(i, period)] if i else prev)
            plain = int(np.frombuffer(layers.delta_frame(frames[1 + i]), "<u4", 16)[10])
            diff = plain if ref is None else int(np.frombuffer(layers.delta_frame(frames[1 + i], ref), "<u4", 16)[10])
            assert counts[i].tolist() == [plain, diff], i
        keys = layers.auto_keys(counts, None, prev is not None)
        assert set(keys[1:].tolist()) == {False, True}  # both outcomes
        out, o, k, c = layers.delta_auto_frames(stream, offs, None, prev, period=period)
        assert np.array_equal(k, keys) and np.array_equal(c, counts)
        want, want_offs = layers.delta_temporal_frames(stream, offs, period, keys, prev)
        assert out == want and np.array_equal(o, want_offs)
        # a cut at a multiple of the period, the second part given input frame cut - period
        for cut in range(period, n, period):
            a = layers.delta_auto_frames(*_join(frames[1:1 + cut]), None, prev, period=period)
            b = layers.delta_auto_frames(*_join(frames[1 + cut:]), None, frames[1 + cut - period], period=period)
            assert a[0] + b[0] == out and np.array_equal(np.concatenate([a[2], b[2]]), k) and np.array_equal(np.concatenate([a[3], b[3]]), c)


@pytest.mark.parametrize("period", [2, 4])
def test_keys_counts_and_bytes_thin_as_the_stream_does(period):
    n = 19
    frames = _repeating(n + period - 1, 3)  # `period` frames in front of the call's n
    call = frames[period:]
    stream, offs = _join(call)
    forced = [int(i in (5, 8)) for i in range(n)]
    for prev in (None, frames[0]):  # input frame -period: frame -(period >> s) of the thinned clip
        out, o, keys, counts = layers.delta_auto_frames(stream, offs, forced, prev, period=period)
        for every in (2, 4):
            if every > period:
                continue
            thin, thin_offs, thin_keys = layers.thin_frames(np.frombuffer(out, np.uint8), o, keys, every)
            sub = layers.delta_auto_frames(*_join(call[::every]), forced[::every], prev, period=period // every)
            assert np.array_equal(sub[2], thin_keys) and np.array_equal(sub[2], keys[::every])
            assert np.array_equal(sub[3], counts[::every])
            assert sub[0] == thin and np.array_equal(sub[1], thin_offs)
            assert np.array_equal(layers.auto_keys(counts[::every], forced[::every], prev is not None), keys[::every])
