"""The co-run order of svc::ClipEncoder (include/svc/clip_encoder.hpp, Schedule): at one rank, in the pipelined schedule, the pyramid
levels of a micro-step that reads its frames once run on the communication stream beside the PREVIOUS micro-step's motion search, and the
micro-step's own search follows one iteration later behind an event.  A search that ran ahead of that event, or a pyramid pass that ran
ahead of the search still reading its slots, would see a stale or half-built pyramid: the two clips here differ, so that gives other
motion vectors.  Every comparison is bit for bit against the SERIAL schedule in the plain two-pass order."""
import ctypes as C

import pytest
import torch

from scalable_video_codec_amd import clip as clipmod
from scalable_video_codec_amd import configs, synth

pytestmark = pytest.mark.gpu

N = 11
CFG = configs.CodecConfig("t-360p-3L-dct8", 41, 640, 360, N, levels=3, dct_block=8)
CFG_B = configs.CodecConfig("t-360p-3L-dct8-b", 77, 640, 360, N, levels=3, dct_block=8)
RANSAC = dict(inlier_thresh=1.5)
FORMS = {"planes": (False, clipmod.TUNE_ALWAYS_SPECULATE, "coeffs"), "wire": (True, 0, "records")}


def _frames(cfg, dev):
    src = synth.SynthClip(cfg.width, cfg.height, N, cfg.seed, device=dev)
    pw, ph = cfg.padded
    return torch.stack([synth.pad_frame(src.frame_bgr(t), pw, ph) for t in range(N)]).contiguous()


@pytest.fixture(scope="module")
def clips(native):
    """The two clips and what the serial two-pass encoder makes of each: computed once, never written."""
    dev = torch.device("cuda")
    frames = {"a": _frames(CFG, dev), "b": _frames(CFG_B, dev)}
    want = {}
    for name, f in frames.items():
        for wire, buf in ((False, "coeffs"), (True, "records")):
            s = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, wire=wire, tuning=clipmod.TUNE_TWO_BGR_PASSES, ransac=RANSAC)
            s.load_frames(f)
            s.step()
            s.sync()
            want[name, buf] = (s.outputs(), s.read(buf), s.read("pyramids"))
            s.close()
    assert not torch.equal(want["a", "coeffs"][0]["mv"], want["b", "coeffs"][0]["mv"])
    assert want["a", "coeffs"][0]["block_types"].count_nonzero() > 0
    return frames, want


def _check(enc, want, name, buf, tag, pyramids=False):
    out = enc.outputs()  # syncs
    w = want[name, buf]
    for key in w[0]:
        assert torch.equal(out[key], w[0][key]), (tag, key)
    assert torch.equal(enc.read(buf), w[1]), (tag, buf)
    if pyramids:  # (slot 0 is the halo's)
        stride = enc.info.pyramid_stride
        assert torch.equal(enc.read("pyramids")[stride:], w[2][stride:]), (tag, "pyramids")


@pytest.mark.parametrize("chunk_pairs", [0, 1, 3])
@pytest.mark.parametrize("lat_depth", [1, 2])
@pytest.mark.parametrize("form", ["planes", "wire"])
def test_back_to_back_steps_over_alternating_clips(clips, form, lat_depth, chunk_pairs):
    """Four back-to-back steps over clips a, b, a, b where they are (step_frames: no drain between them), whole-shard steps and chunked ones.
    Only the newest step's outputs can be read, so the run is repeated at every length 1 .. 4: each step is read once with all its
    predecessors in flight in front of it.  The same with SVC_CLIP_TUNE_PYRAMID_ON_MAIN (the parent's order) gives the same bytes."""
    frames, want = clips
    wire, tuning, buf = FORMS[form]
    for switch in (0, clipmod.TUNE_PYRAMID_ON_MAIN):
        enc = clipmod.Clip(CFG, N, schedule=clipmod.PIPELINED, wire=wire, lat_depth=lat_depth, chunk_pairs=chunk_pairs, tuning=tuning | switch,
                           ransac=RANSAC)
        for length in (1, 2, 3, 4):
            for k in range(length):
                name = "ab"[k & 1]
                enc.step_frames(frames[name], timed=True)
            _check(enc, want, name, buf, (switch, length))
        t = enc.stage_times_ms()
        chunks = enc.info.chunks_per_step
        assert all(t[k][1] == 10 * chunks for k in ("luma_pyramid", "hbma", "dct_quant", "type_patch")), t
        enc.close()


@pytest.mark.parametrize("chunk_pairs", [0, 3])
def test_transitions_between_co_run_and_parent_order(clips, chunk_pairs):
    """SVC_CLIP_TUNE_RANDOM_POLICY | SVC_CLIP_TUNE_IDLE_RULE_ANY_SIZE: micro-steps that read their frames once (co-run) and two-pass ones
    (the parent's order) follow each other in a fixed pseudo-random sequence, over a script of 8 steps with a sync(), a load_frames of the
    other clip and a reset_policy() in the middle.  A search must neither skip the wait for a side-stream pyramid nor wait on an event
    that was never recorded (that would hang or read a stale pyramid).  The script is run to every length 1 .. 8 and read there."""
    frames, want = clips
    enc = clipmod.Clip(CFG, N, schedule=clipmod.PIPELINED, chunk_pairs=chunk_pairs,
                       tuning=clipmod.TUNE_RANDOM_POLICY | clipmod.TUNE_IDLE_RULE_ANY_SIZE, ransac=RANSAC)
    enc.load_frames(frames["a"])
    resident = "a"
    for length in range(1, 9):
        for k in range(length):
            name = "ab"[k & 1]
            if k == 3:
                enc.sync()
            if k == 6:
                enc.reset_policy()
            if k == 5:  # the other clip becomes the resident one (load_frames drains), and this step reads it there
                resident = "b" if resident == "a" else "a"
                enc.load_frames(frames[resident])
                enc.step()
                name = resident
            else:
                enc.step_frames(frames[name])
        _check(enc, want, name, "coeffs", (chunk_pairs, length), pyramids=True)
    p = enc.policy_info()
    assert 0 < p["chunks_speculated"] < p["chunks_decided"]
    enc.close()


@pytest.mark.parametrize("form", ["planes", "wire"])
def test_first_step_after_construction_and_after_a_drain(clips, form):
    """A shard's first chunk also builds the pyramid of the clip's tracked-only frame 0; in the co-run order that launch runs on the side
    stream too.  One step into the new encoder, sync(), one more step: both steps' outputs, and every own pyramid."""
    frames, want = clips
    wire, tuning, buf = FORMS[form]
    enc = clipmod.Clip(CFG, N, schedule=clipmod.PIPELINED, wire=wire, tuning=tuning, ransac=RANSAC)
    enc.load_frames(frames["a"])
    enc.step()
    enc.sync()
    _check(enc, want, "a", buf, "first step", pyramids=True)
    enc.step_frames(frames["b"])
    _check(enc, want, "b", buf, "after the drain", pyramids=True)
    enc.close()


_hip = None


def _hip_memcpy_async(dst, src, nbytes, stream):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")  # the HIP runtime already in the process
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rc = _hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)  # hipMemcpyDeviceToDevice
    assert rc == 0, rc


@pytest.mark.parametrize("form", ["planes", "wire"])
def test_two_shards_on_one_gpu_still_equal_the_unsharded_clip(clips, form):
    """Multi-rank geometry (world = 2, both ranks in this process, the halo copied by the transport hook): the co-run order does not apply
    there -- the communication stream carries the halo -- and the shards, reading their frames once, still encode to the unsharded clip."""
    frames, want = clips
    wire, tuning, buf = FORMS[form]
    w = want["a", buf]
    got = {k: [] for k in w[0]}
    got_buf = []
    prev = None
    for r in range(2):
        enc = clipmod.Clip(CFG, N, rank=r, world=2, schedule=clipmod.PIPELINED, wire=wire, tuning=tuning, ransac=RANSAC)
        i = enc.info
        enc.load_frames(frames["a"][i.first_frame:i.first_frame + i.frames].contiguous())

        def transport(send, recv, nbytes, stream, r=r, prev=prev, stride=i.pyramid_stride):
            if r > 0:  # what rank 0 sends: its last pyramid, finished and synced below
                src, have = C.c_void_p(), C.c_uint64()
                clipmod._check(clipmod.load().svc_clip_output(prev._h, clipmod.BUFFERS["pyramids"][0], C.byref(src), C.byref(have)))
                _hip_memcpy_async(recv, src.value + prev.info.frames * stride, nbytes, stream)
        enc.set_halo_transport(transport)
        for _ in range(4):
            enc.step()
        enc.sync()
        o = enc.outputs()
        for k in got:
            got[k].append(o[k])
        got_buf.append(enc.read(buf))
        prev = enc
    for k in got:
        assert torch.equal(torch.cat(got[k]), w[0][k]), k
    assert torch.equal(torch.cat(got_buf), w[1])
