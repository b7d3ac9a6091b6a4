"""svc::ClipEncoder with ClipEncoderConfig::compact (clip.Clip(compact=True)): the step leaves the compact stream straight from the
transform kernel, and its bytes are the pack (svc_hip_pack_levels_frames) of what a planes encoder with the same configuration and
seed leaves in kCoeffs + kBlockTypes -- in every schedule, for frames stepped where they are, and shard by shard."""
import ctypes as C

import pytest
import torch

from scalable_video_codec_amd import clip as clipmod
from scalable_video_codec_amd import configs
from scalable_video_codec_amd import native as nat
from tests.test_gpu_clip import CFG, _frames, _hip_memcpy_async

pytestmark = pytest.mark.gpu

N = 7  # frames of the test clip: 6 pairs


def _pack_of_planes(enc, block):
    """The newest step of a planes encoder, packed by the two-call route's second half -> (bytes, offsets) on the host."""
    i = enc.info
    coeffs = enc.read("coeffs", device="cuda").view(i.pairs, 3, i.padded_h, i.padded_w)
    types = enc.read("block_types", device="cuda").view(i.pairs, i.blocks)
    out, offs = nat.pack_levels_frames(coeffs, types, block, CFG.mv_block, CFG.fg_step, CFG.bg_step)
    torch.cuda.synchronize()
    return out[:int(offs[-1])].cpu(), offs.cpu()


def _planes_reference(frames, block, **kw):
    enc = clipmod.Clip(CFG, frames.shape[0], schedule=clipmod.SERIAL, dct_block=(block, block), tuning=clipmod.TUNE_TWO_BGR_PASSES, **kw)
    enc.load_frames(frames)
    enc.step()
    enc.sync()
    want = _pack_of_planes(enc, block)
    enc.close()
    return want


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("schedule,steps", [(clipmod.SERIAL, 1), (clipmod.PIPELINED, 3)])
def test_compact_output_is_the_pack_of_the_planes_output(native, block, schedule, steps):
    frames = _frames(CFG, N, torch.device("cuda"))
    want, want_offs = _planes_reference(frames, block)
    enc = clipmod.Clip(CFG, N, schedule=schedule, dct_block=(block, block), compact=True)
    i = enc.info
    assert i.output_sets == 1 and i.chunks_per_step == 1 and i.record_bytes == 0
    enc.load_frames(frames)
    for _ in range(steps):  # back to back, then one sync
        enc.step(timed=True)
    enc.sync()
    got, got_offs = enc.read_compact()
    assert got_offs.tolist() == want_offs.tolist() and got_offs.numel() == i.pairs + 1
    assert torch.equal(got, want)
    assert enc.read("coeffs").numel() == 0 and enc.read("records").numel() == 0  # no plane buffer exists
    t = enc.stage_times_ms()
    assert t["dct_quant"][1] == steps and "type_patch" not in t  # one launch per step, nothing speculated
    enc.close()


def test_compact_frames_stepped_where_they_are(native):
    dev = torch.device("cuda")
    other = configs.CodecConfig("t-360p-3L-dct8-other", 77, CFG.width, CFG.height, N, levels=3, dct_block=8)
    a, b = _frames(CFG, N, dev), _frames(other, N, dev)
    want_a, want_b = _planes_reference(a, 8), _planes_reference(b, 8)
    assert not torch.equal(want_a[0][:4096], want_b[0][:4096])
    enc = clipmod.Clip(CFG, N, schedule=clipmod.PIPELINED, compact=True)
    enc.load_frames(a)
    enc.step()
    s = enc.step_frames(b)
    enc.wait_step(s)
    got, got_offs = enc.read_compact()
    assert got_offs.tolist() == want_b[1].tolist() and torch.equal(got, want_b[0])
    enc.step()  # the resident clip again
    got, got_offs = enc.read_compact()
    assert got_offs.tolist() == want_a[1].tolist() and torch.equal(got, want_a[0])
    enc.close()


@pytest.mark.parametrize("schedule", [clipmod.SERIAL, clipmod.PIPELINED])
def test_two_shards_hold_the_unsharded_clips_frames(native, schedule):
    frames = _frames(CFG, N, torch.device("cuda"))
    whole = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, compact=True)
    whole.load_frames(frames)
    whole.step()
    want, want_offs = whole.read_compact()
    want_offs = want_offs.tolist()
    prev, pair = None, 0
    for r in range(2):
        enc = clipmod.Clip(CFG, N, rank=r, world=2, schedule=schedule, compact=True)
        i = enc.info
        enc.load_frames(frames[i.first_frame:i.first_frame + i.frames].contiguous())

        def transport(send, recv, nbytes, stream, r=r, prev=prev, stride=i.pyramid_stride):
            if r > 0:  # what rank r - 1 sends: its last pyramid, finished and synced below
                src, have = C.c_void_p(), C.c_uint64()
                clipmod._check(clipmod.load().svc_clip_output(prev._h, clipmod.BUFFERS["pyramids"][0], C.byref(src), C.byref(have)))
                _hip_memcpy_async(recv, src.value + prev.info.frames * stride, nbytes, stream)
        enc.set_halo_transport(transport)
        for _ in range(1 if schedule == clipmod.SERIAL else 3):
            enc.step()
        enc.sync()
        got, got_offs = enc.read_compact()
        got_offs = got_offs.tolist()
        assert len(got_offs) == i.pairs + 1 and got_offs[0] == 0 and got.numel() == got_offs[-1]
        for k in range(i.pairs):  # frame by frame: each rank's stream starts at 0
            assert torch.equal(got[got_offs[k]:got_offs[k + 1]], want[want_offs[pair]:want_offs[pair + 1]]), (r, k)
            pair += 1
        prev = enc
    assert pair == N - 1


def test_configurations_compact_refuses(native):
    with pytest.raises(clipmod.ClipError, match="compact and wire"):
        clipmod.Clip(CFG, N, compact=True, wire=True)
    with pytest.raises(clipmod.ClipError, match="whole-shard launches"):
        clipmod.Clip(CFG, N, compact=True, chunk_pairs=2)
    for block in (0, 4):
        with pytest.raises(clipmod.ClipError, match="8x8 or 16x16"):
            clipmod.Clip(CFG, N, compact=True, dct_block=(block, block))
    with pytest.raises(clipmod.ClipError, match="8x8 or 16x16"):
        clipmod.Clip(CFG, N, compact=True, dct_block=(8, 16))
    zero_step = configs.CodecConfig("t-360p-step0", 41, 640, 360, N, levels=3, dct_block=8, fg_step=0)
    with pytest.raises(clipmod.ClipError, match="steps > 0"):
        clipmod.Clip(zero_step, N, compact=True)
    # a planes encoder has no compact stream
    enc = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL)
    assert enc.read("compact").numel() == 0 and enc.read("compact_offsets").numel() == 0
    enc.close()
