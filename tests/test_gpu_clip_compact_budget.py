"""svc::ClipEncoder::SetCompactBudget (clip.Clip.set_compact_budget): a compact step under a byte budget leaves what
svc_hip_dct_pack_levels_budget_frames leaves for the clip's own frames and region ids -- in every schedule, after the budget changes,
shard by shard -- and an empty ladder returns to the configuration's steps."""
import ctypes as C

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import clip as clipmod
from scalable_video_codec_amd import native as nat
from tests.test_gpu_clip import CFG, _frames, _hip_memcpy_async
from tests.test_levels_budget_host import frame_floor, ladder

pytestmark = pytest.mark.gpu

N = 7  # frames of the test clip: 6 pairs
LADDER = ladder(8)  # (1, 16) ... (1, 640) ... (8, 640): the configuration's (1, 640) is entry 4


def _fixed_step(enc):
    """One step at the configuration's steps -> (bytes, offsets as a list)."""
    enc.step()
    got, offs = enc.read_compact()
    return got, offs.tolist()


def _budget_from(offs):
    """Between the fixed step's frame sizes: frames above it cannot even keep (1, 640), and a finer background fits none."""
    sizes = sorted(b - a for a, b in zip(offs, offs[1:]))
    return sizes[len(sizes) // 2]


def _reference(enc, block, budget):
    """svc_hip_dct_pack_levels_budget_frames on the clip's own frames 1 .. and its own region ids, the same budget for every frame."""
    i = enc.info
    bgr = enc.read("bgr", device="cuda").view(i.frames, i.padded_h, i.padded_w, 3)
    types = enc.read("block_types", device="cuda").view(i.pairs, i.blocks)
    out, offs, choice = nat.dct_pack_levels_budget_frames(bgr[i.frames - i.pairs:].contiguous(), block, types, CFG.mv_block, LADDER, budget)
    torch.cuda.synchronize()
    return out[:int(offs[-1])].cpu(), offs.cpu().tolist(), choice.cpu().numpy().view(np.uint32).tolist()


def _read(enc):
    got, offs = enc.read_compact()
    return got, offs.tolist(), enc.read("compact_choice").numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("schedule,steps", [(clipmod.SERIAL, 1), (clipmod.PIPELINED, 3)])
def test_budgeted_step_equals_the_budgeted_call(native, block, schedule, steps):
    frames = _frames(CFG, N, torch.device("cuda"))
    enc = clipmod.Clip(CFG, N, schedule=schedule, dct_block=(block, block), compact=True)
    enc.load_frames(frames)
    fixed, fixed_offs = _fixed_step(enc)
    assert enc.read("compact_choice").numel() == 0  # no budget, no choices
    budget = _budget_from(fixed_offs)
    enc.set_compact_budget(LADDER, budget)
    for _ in range(steps):  # back to back, then one sync
        enc.step(timed=True)
    enc.sync()
    got, offs, choice = _read(enc)
    want, want_offs, want_choice = _reference(enc, block, budget)
    assert choice == want_choice and len(choice) == enc.info.pairs
    assert any(c != 0 for c in choice)  # at least one frame is over the finest entry
    assert offs == want_offs and torch.equal(got, want)
    assert enc.stage_times_ms()["dct_quant"][1] == steps  # one launch of the transform stage per step

    # the next step takes a changed budget
    lower = frame_floor(enc.info.padded_w, enc.info.padded_h, block, block, CFG.mv_block, CFG.mv_block)
    budget2 = lower + (min(b - a for a, b in zip(fixed_offs, fixed_offs[1:])) - lower) // 2
    enc.set_compact_budget(LADDER, budget2)
    enc.step()
    got2, offs2, choice2 = _read(enc)
    want2, want_offs2, want_choice2 = _reference(enc, block, budget2)
    assert choice2 != choice and choice2 == want_choice2
    assert offs2 == want_offs2 and torch.equal(got2, want2)

    # an empty ladder: the configuration's steps again
    enc.set_compact_budget([], 0)
    again, again_offs = _fixed_step(enc)
    assert again_offs == fixed_offs and torch.equal(again, fixed)
    assert enc.read("compact_choice").numel() == 0
    enc.close()


@pytest.mark.parametrize("schedule", [clipmod.SERIAL, clipmod.PIPELINED])
def test_two_shards_hold_the_unsharded_clips_frames(native, schedule):
    frames = _frames(CFG, N, torch.device("cuda"))
    whole = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, compact=True)
    whole.load_frames(frames)
    budget = _budget_from(_fixed_step(whole)[1])
    whole.set_compact_budget(LADDER, budget)
    whole.step()
    want, want_offs, want_choice = _read(whole)
    assert len(set(want_choice)) >= 2
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
        enc.set_compact_budget(LADDER, budget)
        for _ in range(1 if schedule == clipmod.SERIAL else 3):
            enc.step()
        enc.sync()
        got, got_offs, got_choice = _read(enc)
        assert len(got_offs) == i.pairs + 1 and got_offs[0] == 0 and got.numel() == got_offs[-1] and len(got_choice) == i.pairs
        for k in range(i.pairs):  # frame by frame: each rank's stream starts at 0
            assert got_choice[k] == want_choice[pair], (r, k)
            assert torch.equal(got[got_offs[k]:got_offs[k + 1]], want[want_offs[pair]:want_offs[pair + 1]]), (r, k)
            pair += 1
        prev = enc
    assert pair == N - 1


def test_refusals(native):
    planes = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL)
    with pytest.raises(clipmod.ClipError, match="setting of the compact stream"):
        planes.set_compact_budget(LADDER, 1 << 20)
    planes.close()
    enc = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, compact=True)
    with pytest.raises(clipmod.ClipError, match="dct_pack_levels_budget: ladder entry 1: quant steps must be positive"):
        enc.set_compact_budget([(1, 640), (0, 640)], 1 << 20)
    with pytest.raises(clipmod.ClipError, match="dct_pack_levels_budget: ladder entry 1 .* the ladder must be non-decreasing"):
        enc.set_compact_budget([(2, 640), (1, 640)], 1 << 20)
    with pytest.raises(clipmod.ClipError, match="a ladder of 65 entries"):
        enc.set_compact_budget([(1, 640)] * 65, 1 << 20)
    # a refused ladder changes nothing: the step is the fixed one
    enc.load_frames(_frames(CFG, N, torch.device("cuda")))
    enc.step()
    assert enc.read("compact_choice").numel() == 0 and enc.read("compact").numel() > 0
    enc.close()
