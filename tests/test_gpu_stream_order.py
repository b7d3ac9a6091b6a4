"""Every device entry point on a side stream: its work is ordered on the caller's stream and the call does not wait on the host
(tests/helpers/stream_order.py has the method and what it cannot see).

include/svc_hip.h promises it for every entry point that takes a `void* stream`; every other GPU test runs on the null stream, where a
launch with stream 0, a memset on the wrong stream, an unjoined fork and a stray hipStreamSynchronize all give the right bytes.  The
host drivers (svc::ClipEncoder, svc::StreamEncoder, svc::StreamDecoder, the transcoder) run on non-blocking streams of their own, where
each of these is a race.  Per case, check_order runs the call on a non-blocking side stream behind a delay while its inputs still hold
the same case built with another seed; test_two_callers_at_once runs two such callers (seeds 0 and 1, buffers and streams of their own)
so that their device work overlaps.  Every comparison is bit for bit against the same call on the null stream.

The cases: the ENTRIES registries of the guard tests with their builders unchanged, on one geometry per tile size and three frames
(what matters here is each distinct sequence of launches, hardly the data); and, in the same form, a builder per launch path of the
entry points those registries do not hold.  tests/test_stream_order_host.py checks on the CPU that the cases plus EXEMPT are exactly the
declarations of include/svc_hip.h that take a stream.

Measured on an MI355X over this whole file (the figures per case are printed; pytest -s shows them): delays of 19.9 to 20.1 ms, the
largest host time from enqueueing a delay to the query after the C call 1.06 ms for a form that is not blocking (23.8 ms for the one
that is: it waits for the delay, as include/svc_hip.h says), no case inconclusive; the delay finally chosen is 20 ms.
"""
import functools

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from tests import util
from tests.helpers import stream_order as so
from tests.test_gpu_guard_streams import DEC, ENC, G8, G16, GX, REFUSED, Pool, _cuda, _gid, _segment_case, _svcq
from tests import (test_gpu_guard_band, test_gpu_guard_dct_pack_delta, test_gpu_guard_dct_pack_delta_auto, test_gpu_guard_decode_delta,
                   test_gpu_guard_decode_delta_reduced, test_gpu_guard_delta, test_gpu_guard_delta_temporal, test_gpu_guard_streams,
                   test_gpu_placement_streams)

pytestmark = pytest.mark.gpu

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32

# Entry-point forms that may wait on the host (finding (d) is not raised for them; (a) to (c) are).  include/svc_hip.h, at
# svc_hip_segment_workspace_bytes: above 64 clusters or 16 attempts the segmentation "waits for `stream` and returns with the ids in place".
BLOCKING = {"segment_frames_ex-22x18-100-clusters": "cluster_count above 64: composed frame by frame through host memory, synchronous"}
# Entry points with no case.
EXEMPT = {"svc_hip_halo_shift": "needs an RCCL communicator of two ranks: more than the one process"}

N = 3
GEOMS = (G8[0], G16[0], GX[0])


# ---- the cases written new: build(pool, geom, n, seed) -> (inputs by name, call(inputs) -> defined outputs by name) ------------------------

def _rng(seed, *salt):
    return np.random.default_rng([seed, *salt])


def _hbma(levels, flags, kernel):
    def build(pool, geom, n, seed):
        w, h, r, mb, pairs = 128, 128, 8, 16, 2
        assert nat.hbma_kernel_name(levels, w, h, r, mb, mb, flags) == kernel
        rng = _rng(seed, 1)  # one generator for all frames: three different pyramids, and other ones per seed
        pyrs = [util.random_planes(rng, w, h, levels) for _ in range(pairs + 1)]
        stride = (sum(p.size for p in pyrs[0]) + 15) & ~15
        buf = util.pack_clip(pyrs, stride, torch.device("cuda"))
        blocks = (w // mb) * (h // mb)
        mv, mad = pool.buf("mv", (pairs, blocks, 2), F32), pool.buf("mad", (pairs, blocks), F32)

        def call(i):
            p = i["pyramids"]
            nat.hbma_pairs(p, p[stride:], stride, pairs, levels, w, h, r, mb, mb, flags=flags, out=(mv, mad))
            return {"mv": mv, "mad": mad}
        return {"pyramids": buf}, call
    return build


def e_ebma(pool, geom, n, seed):
    w, h, r, mb = 64, 48, 4, 16
    planes = _cuda(_rng(seed, 2).integers(0, 256, (n + 1) * w * h, dtype=np.uint8))
    blocks = (w // mb) * (h // mb)
    mv, mad = pool.buf("mv", (n, blocks, 2), F32), pool.buf("mad", (n, blocks), F32)

    def call(i):
        p = i["planes"]
        nat._check(nat.load().svc_hip_ebma_pairs(p.data_ptr(), p.data_ptr() + w * h, w * h, n, w, h, r, mb, mb, mv.data_ptr(), mad.data_ptr(),
                                                 nat._stream()))
        return {"mv": mv, "mad": mad}
    return {"planes": planes}, call


def e_global_ebma(pool, geom, n, seed):
    """tests/test_gpu_guard_streams.py::test_global_ebma_pairs' first shape: a memset of the workspace, then the kernels."""
    w, h, r = 97, 61, 5
    planes = _rng(seed, 3).integers(0, 256, (n + 1, h, w), dtype=np.uint8)
    planes[1] = np.roll(planes[0], (2, -3), (0, 1))
    need = int(nat.load().svc_hip_global_ebma_workspace_bytes(r, n))
    assert need > 0
    ws, gm, mad = pool.buf("workspace", need, U8), pool.buf("gm", (n, 2), F32), pool.buf("mad", n, F32)

    def call(i):
        p = i["planes"]
        nat._check(nat.load().svc_hip_global_ebma_pairs(p.data_ptr(), p.data_ptr() + w * h, w * h, n, w, h, r, ws.data_ptr(), need,
                                                        gm.data_ptr(), mad.data_ptr(), nat._stream()))
        return {"gm": gm, "mad": mad}
    return {"planes": _cuda(planes).reshape(-1)}, call


def e_global_avg(pool, geom, n, seed):
    blocks = 2049
    mv = _cuda((_rng(seed, 4).random((n, blocks, 2)) * 16 - 8).astype(np.float32))
    out = pool.buf("avg", (n, 2), F32)

    def call(i):
        nat._check(nat.load().svc_hip_global_avg_frames(i["mv"].data_ptr(), blocks, n, out.data_ptr(), nat._stream()))
        return {"avg": out}
    return {"mv": mv}, call


SUBSET = 3


@functools.lru_cache(maxsize=None)
def _ransac_fields(n, seed):
    """An integral field with outliers, a fractional one, a scattered one; sample indices inside the field."""
    blocks = 2049
    rng = _rng(seed, 5)
    k = nat.ransac_iter_count(subset_sz=SUBSET)
    mv = np.round(rng.normal(0, 0.6, (n, blocks, 2))).astype(np.float32) + np.float32(2.0)
    mv[:, ::7] += rng.integers(-30, 31, mv[:, ::7].shape).astype(np.float32)
    mv[1 % n] += (rng.random((blocks, 2)) * 0.37).astype(np.float32)
    mv[n - 1] = (rng.random((blocks, 2)) * 1e4).astype(np.float32)
    samples = np.stack([np.stack([rng.choice(blocks, SUBSET, replace=False) for _ in range(k)]) for _ in range(n)]).astype(np.int32)
    return mv, samples, rng.integers(-3, 4, (n, 2)).astype(np.float32)


def _ransac_outputs(pool, n, blocks):
    return pool.buf("gm", (n, 2), F32), pool.buf("rmse", n, F32), pool.buf("mask", (n, blocks), U8), pool.buf("count", n, I32)


def _ransac(form):
    """form: "plain" (svc_hip_ransac_frames), "ex" (flags 0), "deferred": SVC_LAUNCH_DEFER_RMSE on the caller's stream, then
    svc_hip_ransac_rmse_frames on a SECOND stream that waits on an event of the first -- "any stream ordered behind this launch"
    (include/svc_hip.h) -- and the result is the undeferred call's."""
    def build(pool, geom, n, seed):
        mv, samples, gm_in = _ransac_fields(n, seed)
        blocks, iters = mv.shape[1], samples.shape[1]
        out = _ransac_outputs(pool, n, blocks)
        names = ("gm", "rmse", "mask", "count")
        inputs = {"mv": _cuda(mv), "samples": _cuda(samples), "gm_in": _cuda(gm_in)}
        want, second = None, None
        if form == "deferred":
            full = tuple(torch.empty_like(t) for t in out)
            full[0].copy_(inputs["gm_in"])
            nat.ransac_frames(inputs["mv"], inputs["samples"], subset_sz=SUBSET, out=full)
            want = tuple(t.clone() for t in full)
            second = so.side_stream()  # created in front of the caller's side stream, which avoids it (asserted in call)

        def call(i):
            out[0].copy_(i["gm_in"])  # the model is input and output
            if form == "plain":
                p = nat.RansacParams(SUBSET, 7.5, 0.99, 0.5)
                nat._check(nat.load().svc_hip_ransac_frames(i["mv"].data_ptr(), blocks, n, p, i["samples"].data_ptr(), iters, out[0].data_ptr(),
                                                            out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), nat._stream()))
            elif form == "ex":
                nat.ransac_frames(i["mv"], i["samples"], subset_sz=SUBSET, out=out)
            else:
                first = torch.cuda.current_stream()
                assert second.cuda_stream not in (0, first.cuda_stream), "the second stream is the caller's or the null stream"
                nat.ransac_frames(i["mv"], i["samples"], subset_sz=SUBSET, out=out, flags=nat.LAUNCH_DEFER_RMSE)
                launched = torch.cuda.Event()
                launched.record(first)
                second.wait_event(launched)
                with torch.cuda.stream(second):
                    nat.ransac_rmse_frames(i["mv"], out[0], out[2], out[3], out[1], subset_sz=SUBSET)
                first.wait_stream(second)
                for name, got, full in zip(names, out, want):
                    assert not so.gd._differs(got, full), f"deferred RANSAC + rmse: '{name}' is not the undeferred call's"
            return dict(zip(names, out))
        return inputs, call
    return build


def e_ransac_rmse(pool, geom, n, seed):
    """The outputs of a deferred launch, completed: d_rmse is input and output."""
    mv, samples, gm_in = _ransac_fields(n, seed)
    blocks = mv.shape[1]
    mv, gm = _cuda(mv), _cuda(gm_in)
    half = (gm, torch.empty(n, dtype=F32, device="cuda"), torch.empty((n, blocks), dtype=U8, device="cuda"),
            torch.empty(n, dtype=I32, device="cuda"))
    nat.ransac_frames(mv, _cuda(samples), subset_sz=SUBSET, out=half, flags=nat.LAUNCH_DEFER_RMSE)
    rmse = pool.buf("rmse", n, F32)

    def call(i):
        rmse.copy_(i["rmse in"])
        nat.ransac_rmse_frames(i["mv"], i["gm"], i["mask"], i["count"], rmse, subset_sz=SUBSET)
        return {"rmse": rmse}
    return {"mv": mv, "gm": half[0], "mask": half[2], "count": half[3], "rmse in": half[1]}, call


def e_block_types(pool, geom, n, seed):
    blocks = 2049
    mask = _cuda((_rng(seed, 6).random((n, blocks)) < 0.7).astype(np.uint8))
    out = pool.buf("types", (n, blocks), I32)

    def call(i):
        nat.block_types_frames(i["mask"], out=out)
        return {"types": out}
    return {"mask": mask}, call


def _segment(mfw, mfh, flags=0, ex=True, **params):
    """tests/test_gpu_guard_streams.py's _segment_case fields (a heavy frame, a light one, an empty one).  22 x 18: light frames only;
    120 x 68: above 2 048 blocks, the heavy attempts fork to an internal side stream and join back (not with NO_FORK, not in the
    BESIDE shapes); 240 x 135: above 8 192 blocks, the launch sequence over several workgroups (WIDE) or the one-workgroup form."""
    def build(pool, geom, n, seed):
        inputs, _ = _segment_case(Pool(), mfw, mfh, n, 0.5, flags, seed)
        p = nat.SegmentParams(**{**nat.DEFAULT_SEGMENT, **params})
        ws = pool.buf("workspace", nat.segment_workspace_bytes(mfw, mfh, n, p.attempt_count), U8)
        out = pool.buf("types", (n, mfw * mfh), I32)

        def call(i):
            if ex:
                nat.segment_frames(i["mask"], i["mv"], mfw, mfh, seed=77, out=out, workspace=ws, flags=flags, **params)
            else:
                nat._check(nat.load().svc_hip_segment_frames(i["mask"].data_ptr(), i["mv"].data_ptr(), mfw, mfh, n, 16, 16, p, 77, ws.data_ptr(),
                                                             ws.numel(), out.data_ptr(), nat._stream()))
            return {"types": out}
        return inputs, call
    return build


PYR = (176, 144, 4)  # tests/test_gpu_guard_step.py's second pyramid


def e_luma_pyramid(pool, geom, n, seed):
    w, h, levels = PYR
    frames = _cuda(_rng(seed, 7).integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    stride = nat.pyramid_stride(w, h, levels)
    pyr = pool.buf("pyramids", n * stride, U8)

    def call(i):
        pyr.zero_()  # the bytes between two pyramids are not written
        nat.luma_pyramid_frames(i["bgr"], levels, out=pyr, stride=stride)
        return {"pyramids": pyr}
    return {"bgr": frames}, call


def e_pyramid_levels(pool, geom, n, seed):
    w, h, levels = PYR
    planes = _cuda(_rng(seed, 8).integers(0, 256, (n, h * w), dtype=np.uint8))
    stride = nat.pyramid_stride(w, h, levels)
    pyr = pool.buf("pyramids", n * stride, U8)

    def call(i):
        pyr.zero_()
        pyr.view(n, stride)[:, :w * h].copy_(i["level 0"])  # level 0 is input and output
        nat.pyramid_levels_frames(pyr, stride, n, w, h, levels)
        return {"pyramids": pyr}
    return {"level 0": planes}, call


TW, TH, TB, TMV = 176, 48, 8, 16  # the transform's frames: 8 x 8 tiles on a width that is a multiple of 16 (the tuned kernels)


def _frames(n, seed):
    return _cuda(_rng(seed, 9).integers(0, 256, (n, TH, TW, 3), dtype=np.uint8))


def _types(n, seed):
    from tests.test_gpu_transform_exact import _random_types
    return _cuda(_random_types(1000 + seed, n, TW, TH, TMV).view(np.int32))


def _transform(form):
    def build(pool, geom, n, seed):
        inputs = {"bgr": _frames(n, seed)}
        if form in ("dct_quant", "dct_records"):
            inputs["types"] = _types(n, seed)
        if form in ("dct_records", "dct_records_luma"):
            per = nat.serialized_frame_bytes(TW, TH, TB, TB)
            out = pool.buf("records", (n, per), U8)
        else:
            out = pool.buf("planes", (n, 3, TH, TW), F32)
        pstride = (TW * TH + 255) // 256 * 256
        luma = pool.buf("level 0", n * pstride, U8) if form.endswith("_luma") else None

        def call(i):
            if form == "dct":
                nat.dct_frames(i["bgr"], TB, out=out)
            elif form == "dct_quant":
                nat.dct_quant_frames(i["bgr"], TB, i["types"], TMV, 7, 640, out=out)
            elif form == "dct_records":
                nat.dct_records_frames(i["bgr"], TB, i["types"], TMV, 7, 640, out=out)
            else:
                luma.zero_()  # the bytes between two planes are not written
                if form == "dct_quant_luma":
                    nat._check(nat.load().svc_hip_dct_quant_luma_frames(i["bgr"].data_ptr(), TW * TH * 3, n, TW, TH, TB, 640, out.data_ptr(),
                                                                   luma.data_ptr(), pstride, nat._stream()))
                else:
                    nat._check(nat.load().svc_hip_dct_records_luma_frames(i["bgr"].data_ptr(), TW * TH * 3, n, TW, TH, TB, TH, out.data_ptr(),
                                                                     out.stride(0), luma.data_ptr(), pstride, nat._stream()))
                return {"out": out, "level 0": luma}
            return {"out": out}
        return inputs, call
    return build


def e_quant(pool, geom, n, seed):
    coeffs = _cuda((_rng(seed, 10).random(n * 4099) * 2000 - 1000).astype(np.float32))
    out = pool.buf("coeffs", coeffs.numel(), F32)

    def call(i):
        out.copy_(i["coeffs"])  # in place
        nat.quant_(out, 7)
        return {"coeffs": out}
    return {"coeffs": coeffs}, call


def e_quant_frames(pool, geom, n, seed):
    planes = nat.dct_frames(_frames(n, seed), TB)
    out = pool.buf("planes", (n, 3, TH, TW), F32)

    def call(i):
        out.copy_(i["planes"])  # in place
        nat.quant_frames_(out, i["types"], TMV, 7, 640)
        return {"planes": out}
    return {"planes": planes, "types": _types(n, seed)}, call


def e_count_foreground(pool, geom, n, seed):
    count = pool.buf("count", 1, I32)

    def call(i):
        nat._check(nat.load().svc_hip_count_foreground(i["types"].data_ptr(), i["types"].numel(), count.data_ptr(), nat._stream()))
        return {"count": count}
    return {"types": _types(n, seed)}, call


def e_dct_quant_redo(pool, geom, n, seed):
    """The speculative planes (every tile quantised as background) are input and output: every call starts from them."""
    frames = _frames(n, seed)
    spec = nat.dct_quant_luma_frames(frames, TB, 1, bg_step=640)[0]
    need = int(nat.load().svc_hip_dct_redo_workspace_bytes(n, TW, TH, TMV, TMV))
    assert need > 0
    ws, planes = pool.buf("workspace", need, U8), pool.buf("planes", (n, 3, TH, TW), F32)

    def call(i):
        planes.copy_(i["speculative planes"])
        nat._check(nat.load().svc_hip_dct_quant_redo_frames(i["bgr"].data_ptr(), TW * TH * 3, n, TW, TH, TB, i["types"].data_ptr(), TMV, TMV, 7,
                                                            planes.data_ptr(), ws.data_ptr(), need, nat._stream()))
        return {"planes": planes}
    return {"bgr": frames, "types": _types(n, seed), "speculative planes": spec}, call


def e_serialize(pool, geom, n, seed):
    planes = nat.dct_frames(_frames(n, seed), TB)
    out = pool.buf("records", (n, nat.serialized_frame_bytes(TW, TH, TB, TB)), U8)

    def call(i):
        nat.serialize_frames(i["planes"], i["types"], TW, TH, TB, TB, TW // TMV, TH // TMV, TMV, out=out)
        return {"records": out}
    return {"planes": planes, "types": _types(n, seed)}, call


def e_wire_patch_types(pool, geom, n, seed):
    """Records emitted with type words 0 are input and output."""
    records = nat.dct_records_luma_frames(_frames(n, seed), TB, 1)[0]
    out = pool.buf("records", tuple(records.shape), U8)

    def call(i):
        out.copy_(i["records"])
        nat.wire_patch_types_frames(out, i["types"], TW, TH, TB, TMV)
        return {"records": out}
    return {"records": records, "types": _types(n, seed)}, call


def e_decode_frames(pool, geom, n, seed):
    types = _types(n, seed)
    planes = nat.dct_quant_frames(_frames(n, seed), TB, types, TMV, 2, 40)
    rec = pool.buf("rec", (n, TH, TW, 3), F32)

    def call(i):
        nat.decode_frames(i["planes"], TB, i["types"], TMV, 2, 40, gaze=(16, 8, 40, 24), out=rec)
        return {"rec": rec}
    return {"planes": planes, "types": types}, call


def e_sse(pool, geom, n, seed):
    frames, types = _frames(n, seed), _types(n, seed)
    rec = nat.decode_frames(nat.dct_quant_frames(frames, TB, types, TMV, 2, 40), TB, types, TMV, 2, 40)
    sse = pool.buf("sse", n, I64)

    def call(i):
        nat._check(nat.load().svc_hip_sse_frames(i["bgr"].data_ptr(), TW * TH * 3, i["rec"].data_ptr(), n, TW, TH, TW - 5, TH - 3, sse.data_ptr(),
                                                 nat._stream()))
        return {"sse": sse}
    return {"bgr": frames, "rec": rec}, call


def e_decode_records(pool, geom, n, seed):
    records = nat.dct_records_frames(_frames(n, seed), TB, _types(n, seed), TMV, 2, 40)
    dw, dh = TW - 5, TH - 3
    rec, disp = pool.buf("rec", (n, TH, TW, 3), F32), pool.buf("display", (n, dh, dw, 3), U8)
    gaze = _cuda(np.array([(0, 0, 0, 0), (0, 0, TW, TH), (TW - 8, TH - 8, 8, 8)], np.int32)[:n])

    def call(i):
        nat.decode_records_frames(i["records"], TW, TH, TB, 2, 40, gaze=i["gaze"], display=(dw, dh), rec=rec, out_display=disp)
        return {"rec": rec, "display": disp}
    return {"records": records, "gaze": gaze}, call


def e_decode_layers_reduced(pool, geom, n, seed):
    """tests/test_gpu_guard_streams.py's layered streams (a base and its enhancement from one transform) and gaze."""
    w, h, tile, mv = geom
    reduce = test_gpu_placement_streams.REDUCE[tile[0]]
    inputs, _ = test_gpu_guard_streams.e_decode_layers(Pool(), geom, n, seed)
    rw, rh = w // reduce, h // reduce
    dw, dh = max(1, rw - 5), max(1, rh - 3)
    ws = pool.buf("workspace", nat.decode_layers_reduced_workspace_bytes(n, w, h, tile), U8)
    rec, disp, status = pool.buf("rec", (n, rh, rw, 3), F32), pool.buf("display", (n, dh, dw, 3), U8), pool.buf("status", n, I32)

    def call(i):
        nat._check(nat.load().svc_hip_decode_layers_reduced_frames(
            i["base"].data_ptr(), i["base"].numel(), i["base offsets"].data_ptr(), i["enhancement"].data_ptr(), i["enhancement"].numel(),
            i["enhancement offsets"].data_ptr(), n, w, h, *tile, *mv, *DEC, reduce, i["gaze"].data_ptr(), ws.data_ptr(), ws.numel(),
            rec.data_ptr(), disp.data_ptr(), dw, dh, status.data_ptr(), nat._stream()))
        assert status.cpu().tolist() == [0] * n
        return {"rec": rec, "display": disp, "status": status}
    return inputs, call


def e_records_pack_levels(pool, geom, n, seed):
    """tests/test_gpu_wire_transcode.py's sparse records and steps."""
    from tests.test_gpu_wire_transcode import BG, FG, _records
    w, h, block, mv = 48, 16, 8, 16
    records = _cuda(_records(n, w, h, block, mv, h, "sparse", seed=40 + seed))
    ws = pool.buf("workspace", nat.records_pack_levels_workspace_bytes(n, w, h, block, mv), U8)
    out, offs, status = pool.buf("stream", nat.levels_max_bytes(n, w, h, block, mv), U8), pool.buf("offsets", n + 1, I64), pool.buf("status", n, I32)

    def call(i):
        nat.records_pack_levels_frames(i["records"], w, h, block, mv, FG, BG, out=out, offsets=offs, workspace=ws, status=status)
        assert status.cpu().tolist() == [0] * n
        return {"stream": out[:int(offs[-1])], "offsets": offs, "status": status}
    return {"records": records}, call


def e_levels_records(pool, geom, n, seed):
    w, h, tile, mv = geom
    q, qo = _svcq(geom, n, ENC, seed)
    ws = pool.buf("workspace", nat.levels_records_workspace_bytes(n, w, h, tile), U8)
    records, status = pool.buf("records", (n, nat.serialized_frame_bytes(w, h, *tile)), U8), pool.buf("status", n, I32)

    def call(i):
        nat.levels_records_frames(i["stream"], i["offsets"], w, h, tile, mv, records=records, workspace=ws, status=status)
        assert status.cpu().tolist() == [0] * n
        return {"records": records, "status": status}
    return {"stream": _cuda(q), "offsets": _cuda(qo)}, call


def e_probe(pool, geom, n, seed):
    src = _cuda(_rng(seed, 11).integers(0, 256, 1 << 16, dtype=np.uint8))
    dst = pool.buf("out", 1 << 16, U8)

    def call(i):
        nat.probe_stream(i["in"], dst, 1, 1)
        return {"out": dst}
    return {"in": src}, call


# ---- the table of cases: id -> (the C function, its builder, the geometry) -------------------------------------------------------------------

def _fn_of(entry):
    """The C function behind a registry's key: "delta_levels_temporal2" and "decode_delta_levels_reduced_r4" carry a parameter."""
    for tail in ("_r2", "_r4", "_r8"):
        if entry.endswith(tail):
            entry = entry[:-len(tail)]
    entry = entry.rstrip("0123456789")
    return f"svc_hip_{entry}" if entry.endswith("_drain") else f"svc_hip_{entry}_frames"


REGISTRIES = (test_gpu_guard_streams.ENTRIES, test_gpu_guard_delta.ENTRIES, test_gpu_guard_delta_temporal.ENTRIES,
              test_gpu_guard_band.ENTRIES, test_gpu_guard_decode_delta.ENTRIES, test_gpu_guard_decode_delta_reduced.ENTRIES,
              test_gpu_guard_dct_pack_delta.ENTRIES, test_gpu_guard_dct_pack_delta_auto.ENTRIES,
              # the stream entry points of tests/test_gpu_placement_streams.py's registry that the guard registries do not hold
              {k: test_gpu_placement_streams.ENTRIES[k] for k in ("pack_layers", "decode_levels_reduced", "levels_drain", "entropy_drain")})

CASES = {}
for _registry in REGISTRIES:
    for _entry, (_build, _geoms) in _registry.items():
        for _g in GEOMS:
            if _g in _geoms and (_entry, _g) not in REFUSED:
                CASES[f"{_entry}-{_gid(_g)}"] = (_fn_of(_entry), _build, _g)

NEW = {
    "hbma_pairs-tiled": ("svc_hip_hbma_pairs", _hbma(4, nat.HBMA_AUTO, "hbma_tiled16_kernel")),
    "hbma_pairs-fused": ("svc_hip_hbma_pairs", _hbma(3, nat.HBMA_AUTO, "hbma_fused_kernel")),
    "hbma_pairs-wave": ("svc_hip_hbma_pairs", _hbma(4, nat.HBMA_FORCE_WAVE_PER_BLOCK, "hbma_wave_level_kernel")),
    "ebma_pairs": ("svc_hip_ebma_pairs", e_ebma),
    "global_ebma_pairs-97x61-R5": ("svc_hip_global_ebma_pairs", e_global_ebma),
    "global_avg_frames": ("svc_hip_global_avg_frames", e_global_avg),
    "ransac_frames": ("svc_hip_ransac_frames", _ransac("plain")),
    "ransac_frames_ex": ("svc_hip_ransac_frames_ex", _ransac("ex")),
    "ransac_frames_ex-deferred-rmse-on-a-second-stream": ("svc_hip_ransac_frames_ex", _ransac("deferred")),
    "ransac_rmse_frames": ("svc_hip_ransac_rmse_frames", e_ransac_rmse),
    "block_types_frames": ("svc_hip_block_types_frames", e_block_types),
    "segment_frames-22x18": ("svc_hip_segment_frames", _segment(22, 18, ex=False)),
    "segment_frames_ex-22x18": ("svc_hip_segment_frames_ex", _segment(22, 18)),
    "segment_frames_ex-120x68-fork": ("svc_hip_segment_frames_ex", _segment(120, 68)),
    "segment_frames_ex-120x68-no-fork": ("svc_hip_segment_frames_ex", _segment(120, 68, nat.LAUNCH_NO_FORK)),
    "segment_frames_ex-120x68-beside": ("svc_hip_segment_frames_ex", _segment(120, 68, nat.LAUNCH_BESIDE)),
    "segment_frames_ex-240x135-wide": ("svc_hip_segment_frames_ex", _segment(240, 135, nat.LAUNCH_WIDE)),
    "segment_frames_ex-240x135-no-wide": ("svc_hip_segment_frames_ex", _segment(240, 135, nat.LAUNCH_NO_WIDE)),
    "segment_frames_ex-22x18-100-clusters": ("svc_hip_segment_frames_ex", _segment(22, 18, cluster_count=100)),
    "luma_pyramid_frames": ("svc_hip_luma_pyramid_frames", e_luma_pyramid),
    "pyramid_levels_frames": ("svc_hip_pyramid_levels_frames", e_pyramid_levels),
    "dct_frames": ("svc_hip_dct_frames", _transform("dct")),
    "dct_quant_frames": ("svc_hip_dct_quant_frames", _transform("dct_quant")),
    "quant": ("svc_hip_quant", e_quant),
    "quant_frames": ("svc_hip_quant_frames", e_quant_frames),
    "dct_quant_luma_frames": ("svc_hip_dct_quant_luma_frames", _transform("dct_quant_luma")),
    "count_foreground": ("svc_hip_count_foreground", e_count_foreground),
    "dct_quant_redo_frames": ("svc_hip_dct_quant_redo_frames", e_dct_quant_redo),
    "serialize_frames": ("svc_hip_serialize_frames", e_serialize),
    "dct_records_frames": ("svc_hip_dct_records_frames", _transform("dct_records")),
    "dct_records_luma_frames": ("svc_hip_dct_records_luma_frames", _transform("dct_records_luma")),
    "wire_patch_types_frames": ("svc_hip_wire_patch_types_frames", e_wire_patch_types),
    "decode_frames": ("svc_hip_decode_frames", e_decode_frames),
    "sse_frames": ("svc_hip_sse_frames", e_sse),
    "decode_records_frames": ("svc_hip_decode_records_frames", e_decode_records),
    "records_pack_levels_frames": ("svc_hip_records_pack_levels_frames", e_records_pack_levels),
    "probe_stream": ("svc_hip_probe_stream", e_probe),
}
for _id, (_fn, _build) in NEW.items():
    CASES[_id] = (_fn, _build, None)
for _g in (G8[0], G16[0]):
    CASES[f"decode_layers_reduced-{_gid(_g)}"] = ("svc_hip_decode_layers_reduced_frames", e_decode_layers_reduced, _g)
for _g in GEOMS:
    CASES[f"levels_records-{_gid(_g)}"] = ("svc_hip_levels_records_frames", e_levels_records, _g)
assert set(BLOCKING) <= set(CASES)

FORK = "segment_frames_ex-120x68-fork"


def covered():
    """The entry points the cases reach (tests/test_stream_order_host.py compares them with include/svc_hip.h)."""
    return {fn for fn, _, _ in CASES.values()}


def _caller(case, seed):
    """-> (inputs, the same case built with the other seed, call, the buffers it writes)."""
    _, build, geom = CASES[case]
    pool = Pool()
    inputs, call = build(pool, geom, N, seed)
    stale, _ = build(Pool(), geom, N, 1 - seed)
    return inputs, stale, call, pool.written


@pytest.fixture(scope="module")
def delay(native):
    return so.Delay()


@pytest.mark.parametrize("case", sorted(CASES))
def test_order_and_no_host_wait(native, monkeypatch, delay, case):
    proxy = so.install(monkeypatch, native)  # in front of the builders: some bind their C function when they are built
    caller = _caller(case, 0)
    findings = so.check_order(CASES[case][0], *caller, proxy=proxy, delay=delay, blocking=case in BLOCKING)
    assert not findings, "\n".join(findings)


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_callers_at_once(native, monkeypatch, delay, case):
    proxy = so.install(monkeypatch, native)
    callers = [_caller(case, seed) for seed in (0, 1)]
    findings = so.check_concurrent(CASES[case][0], callers, proxy=proxy, delay=delay, blocking=case in BLOCKING)
    assert not findings, "\n".join(findings)


def test_the_segmentation_forks_from_five_caller_streams_at_once(native, monkeypatch, delay):
    """One more caller than the pool of internal side streams holds (4 per device and host thread, the least recently used slot taken
    for a new caller: "stream order makes reuse safe", csrc/segment.hip): all five enqueued from this thread, so they share one pool."""
    callers = []
    for c in range(5):
        _, build, geom = CASES[FORK]
        pool = Pool()
        inputs, call = build(pool, geom, N, c)
        stale, _ = build(Pool(), geom, N, c + 1)
        callers.append((inputs, stale, call, pool.written))
    proxy = so.install(monkeypatch, native)
    findings = so.check_concurrent(CASES[FORK][0], callers, proxy=proxy, delay=delay, threads=False)
    assert not findings, "\n".join(findings)


# ---- the harness sees what it claims: four fake entry points written with torch operations ----------------------------------------------

def _fake_work(x, y):
    y.copy_(x * 3 + 1)
    return 0


def _fake_in_order(x, y, stream):
    assert stream == torch.cuda.current_stream().cuda_stream
    return _fake_work(x, y)


def _fake_on_the_default_stream(x, y, stream):
    with torch.cuda.stream(torch.cuda.default_stream()):
        return _fake_work(x, y)


def _fake_that_waits(x, y, stream):
    torch.cuda.current_stream().synchronize()
    return _fake_work(x, y)


def _fake_that_ignores_its_input(x, y, stream):
    y.fill_(7)
    return 0


FAKES = {"svc_hip_fake_that_ignores_its_input": (_fake_that_ignores_its_input, 2), "svc_hip_fake_in_order": (_fake_in_order, 2), "svc_hip_fake_on_the_default_stream": (_fake_on_the_default_stream, 2),
         "svc_hip_fake_that_waits": (_fake_that_waits, 2)}


def _fake_case(name, seed, peek=False):
    pool = Pool()
    x = _cuda(_rng(seed, 12).integers(0, 1000, 1 << 16).astype(np.int32))
    y = pool.buf("y", 1 << 16, I32)

    def call(i):
        if peek:
            i["x"][0].item()  # reads an input on the host in front of the call
        nat._check(getattr(nat.load(), name)(i["x"], y, nat._stream()))
        return {"y": y}
    return {"x": x}, {"x": _cuda(_rng(1 - seed, 12).integers(0, 1000, 1 << 16).astype(np.int32))}, call, pool.written


def _letters(findings):
    return sorted(f.split(": ", 1)[1][:3] if f.split(": ", 1)[1].startswith("(") else f for f in findings)


@pytest.mark.parametrize("name,peek,want", [("svc_hip_fake_in_order", False, []), ("svc_hip_fake_on_the_default_stream", False, ["(a)"]),
                                            ("svc_hip_fake_that_waits", False, ["(d)"]), ("svc_hip_fake_in_order", True, ["(c)"])],
                         ids=["correct", "default-stream", "host-wait", "void"])
def test_the_harness_sees_what_it_claims(native, monkeypatch, delay, name, peek, want):
    proxy = so.install(monkeypatch, native, FAKES)
    findings = so.check_order(name, *_fake_case(name, 0, peek), proxy=proxy, delay=delay)
    assert _letters(findings) == want, findings


def test_the_harness_refuses_a_case_whose_outputs_are_the_same_for_the_stale_inputs(native, monkeypatch, delay):
    """A builder whose outputs do not depend on the seed (identical frames, say) could not show finding (a): it fails instead."""
    proxy = so.install(monkeypatch, native, FAKES)
    name = "svc_hip_fake_that_ignores_its_input"
    assert so.check_order(name, *_fake_case(name, 0), proxy=proxy, delay=delay) == [so.f_blind(name)]
    inputs, _, call, written = _fake_case("svc_hip_fake_in_order", 0)
    assert so.check_order("svc_hip_fake_in_order", inputs, inputs, call, written, proxy=proxy, delay=delay) == [so.f_same("svc_hip_fake_in_order")]


def test_the_harness_sees_a_stray_launch_among_two_callers(native, monkeypatch, delay):
    proxy = so.install(monkeypatch, native, FAKES)
    name = "svc_hip_fake_on_the_default_stream"
    findings = so.check_concurrent(name, [_fake_case(name, s) for s in (0, 1)], proxy=proxy, delay=delay)
    assert [f.split(": ", 2)[2][:3] for f in findings] == ["(a)", "(a)"], findings
    assert not so.check_concurrent("svc_hip_fake_in_order", [_fake_case("svc_hip_fake_in_order", s) for s in (0, 1)], proxy=proxy, delay=delay)
