"""svc::ClipEncoder::SetCompactQuality (clip.Clip.set_compact_quality): a compact step under a distortion target leaves what
svc_hip_dct_pack_levels_quality_frames leaves for the clip's own frames and region ids -- bytes, offsets, choices and each frame's squared
error at its entry -- in the serial and the pipelined schedule, with and without a byte cap; an empty ladder returns to the
configuration's steps, and a budget set after a target replaces it."""
import numpy as np
import pytest
import torch

from scalable_video_codec_amd import clip as clipmod
from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from tests.test_gpu_clip import CFG, _frames
from tests.test_gpu_clip_compact_budget import LADDER, N, _budget_from, _fixed_step
from tests.test_gpu_clip_compact_budget import _read as _read_budget
from tests.test_gpu_clip_compact_budget import _reference as _budget_reference

pytestmark = pytest.mark.gpu


def _reference(enc, block, target, cap):
    """svc_hip_dct_pack_levels_quality_frames on the clip's own frames 1 .. and its own region ids, one target and one cap for every frame."""
    i = enc.info
    bgr = enc.read("bgr", device="cuda").view(i.frames, i.padded_h, i.padded_w, 3)
    types = enc.read("block_types", device="cuda").view(i.pairs, i.blocks)
    out, offs, choice, table = nat.dct_pack_levels_quality_frames(bgr[i.frames - i.pairs:].contiguous(), block, types, CFG.mv_block, LADDER, target,
                                                                  cap if cap else None, distortion=True)
    torch.cuda.synchronize()
    choice = choice.cpu().numpy().view(np.uint32)
    table = table.cpu().numpy().view(np.uint64)
    chosen = [int(table[f, int(c) & 0x3FFFFFFF]) for f, c in enumerate(choice)]
    return out[:int(offs[-1])].cpu(), offs.cpu().tolist(), choice.tolist(), chosen, table


def _read(enc):
    got, offs = enc.read_compact()
    return (got, offs.tolist(), enc.read("compact_choice").numpy().view(np.uint32).tolist(),
            enc.read("compact_distortion").numpy().view(np.uint64).tolist())


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("schedule,steps", [(clipmod.SERIAL, 1), (clipmod.PIPELINED, 3)])
def test_quality_step_equals_the_quality_call(native, block, schedule, steps):
    frames = _frames(CFG, N, torch.device("cuda"))
    enc = clipmod.Clip(CFG, N, schedule=schedule, dct_block=(block, block), compact=True)
    enc.load_frames(frames)
    fixed, fixed_offs = _fixed_step(enc)
    assert enc.read("compact_choice").numel() == 0 and enc.read("compact_distortion").numel() == 0  # no target: no choices, no distortions
    # a target between the frames' own squared errors at the middle entry: some frames may go coarser than it, some may not
    table = _reference(enc, block, 0, 0)[4]
    target = int(np.sort(table[:, len(LADDER) // 2])[len(table) // 2])
    enc.set_compact_quality(LADDER, target=target)
    for _ in range(steps):  # back to back, then one sync
        enc.step(timed=True)
    enc.sync()
    got, offs, choice, chosen = _read(enc)
    want, want_offs, want_choice, want_chosen, _ = _reference(enc, block, target, 0)
    assert choice == want_choice and len(choice) == enc.info.pairs and chosen == want_chosen
    assert any(c != 0 for c in choice)  # at least one frame is coarser than the finest entry
    assert offs == want_offs and torch.equal(got, want)
    assert enc.stage_times_ms()["dct_quant"][1] == steps  # one launch of the transform stage per step

    # the next step takes a changed target, in dB, and a cap that some frames feel
    cap = _budget_from(fixed_offs)
    enc.set_compact_quality(LADDER, psnr_db=42.0, bytes_cap=cap)
    enc.step()
    got2, offs2, choice2, chosen2 = _read(enc)
    t2 = layers.distortion_target(42.0, enc.info.padded_w, enc.info.padded_h)
    want2, want_offs2, want_choice2, want_chosen2, _ = _reference(enc, block, t2, cap)
    assert choice2 == want_choice2 and chosen2 == want_chosen2
    assert offs2 == want_offs2 and torch.equal(got2, want2)

    # a budget after a target replaces it: the budgeted call's bytes, and no distortions
    enc.set_compact_budget(LADDER, cap)
    enc.step()
    got3, offs3, choice3 = _read_budget(enc)
    want3, want_offs3, want_choice3 = _budget_reference(enc, block, cap)
    assert choice3 == want_choice3 and offs3 == want_offs3 and torch.equal(got3, want3)
    assert enc.read("compact_distortion").numel() == 0

    # ... and a target after a budget replaces that
    enc.set_compact_quality(LADDER, target=target)
    enc.step()
    got4, offs4, choice4, chosen4 = _read(enc)
    want4, want_offs4, want_choice4, want_chosen4, _ = _reference(enc, block, target, 0)
    assert choice4 == want_choice4 == want_choice and chosen4 == want_chosen4 and offs4 == want_offs4 and torch.equal(got4, want4)

    # an empty ladder: the configuration's steps again
    enc.set_compact_quality([], target=0)
    again, again_offs = _fixed_step(enc)
    assert again_offs == fixed_offs and torch.equal(again, fixed)
    assert enc.read("compact_choice").numel() == 0 and enc.read("compact_distortion").numel() == 0
    enc.close()


def test_reading_between_a_setting_and_the_next_step(native):
    """The table and the choices a step left belong to the setting it ran under: after a new setting -- a shorter ladder above all, whose
    table rows are shorter than the old choices reach -- compact_distortion is empty until a step under that setting has finished."""
    enc = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, compact=True)
    enc.load_frames(_frames(CFG, N, torch.device("cuda")))
    enc.set_compact_quality(LADDER, target=2 ** 64 - 1)  # every entry meets it: the last entry for every frame
    assert enc.read("compact_distortion").numel() == 0    # set, not yet stepped
    enc.step()
    _, _, choice, chosen = _read(enc)
    assert choice == [len(LADDER) - 1] * enc.info.pairs and len(chosen) == enc.info.pairs
    assert enc.read("compact_distortion").numpy().view(np.uint64).tolist() == chosen  # a second read of the same step
    short = LADDER[:2]
    enc.set_compact_quality(short, target=2 ** 64 - 1)  # the old choices (7) lie past a two-entry row
    assert enc.read("compact_distortion").numel() == 0
    enc.step()
    _, _, choice2, chosen2 = _read(enc)
    want = _reference(enc, 8, 2 ** 64 - 1, 0)
    assert choice2 == [1] * enc.info.pairs and chosen2 == [int(want[4][f, 1]) for f in range(enc.info.pairs)]
    enc.set_compact_budget(LADDER, 1 << 30)  # a budget in between, then a target again: still nothing before its first step
    enc.step()
    enc.set_compact_quality(short, psnr_db=40.0)
    assert enc.read("compact_distortion").numel() == 0
    enc.close()


def test_refusals(native):
    planes = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL)
    with pytest.raises(clipmod.ClipError, match="setting of the compact stream"):
        planes.set_compact_quality(LADDER, psnr_db=40)
    planes.close()
    enc = clipmod.Clip(CFG, N, schedule=clipmod.SERIAL, compact=True)
    with pytest.raises(clipmod.ClipError, match="dct_pack_levels_quality: ladder entry 1: quant steps must be positive"):
        enc.set_compact_quality([(1, 640), (0, 640)], psnr_db=40)
    with pytest.raises(clipmod.ClipError, match="dct_pack_levels_quality: ladder entry 1 .* the ladder must be non-decreasing"):
        enc.set_compact_quality([(2, 640), (1, 640)], target=5)
    with pytest.raises(clipmod.ClipError, match="a ladder of 65 entries"):
        enc.set_compact_quality([(1, 640)] * 65, target=5)
    with pytest.raises(ValueError):
        enc.set_compact_quality(LADDER)
    with pytest.raises(ValueError):
        enc.set_compact_quality(LADDER, psnr_db=40, target=5)
    # a refused ladder changes nothing: the step is the fixed one
    enc.load_frames(_frames(CFG, N, torch.device("cuda")))
    enc.step()
    assert enc.read("compact_choice").numel() == 0 and enc.read("compact_distortion").numel() == 0 and enc.read("compact").numel() > 0
    enc.close()
