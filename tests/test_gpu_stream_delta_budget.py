"""svc::StreamEncoder with StreamEncoderConfig::delta and compact_budget, through tests/dropin/stream_delta_budget_main (a caller of
include/svc/stream_encoder.hpp only): the delta stream with one ladder entry per group of frames, by a byte budget on the group
(svc_hip_dct_pack_delta_budget_frames).

A 17-frame 96 x 64 synthetic clip (16 encoded frames; the padded size is the same).  The configuration is accepted exactly when every
batch holds whole groups: a key frame every 4 with batches of 4, 8 and 16, every 8 with batches of 8 and 16, at depths 3 and 4.  The
stream must not depend on batch or depth; it equals one device call over the clip with the driver's own region ids, and
svc::StreamDecoder::DecodeDelta plays what Decode plays from the plain stream packed frame by frame at the chosen steps.  A run is made
once per command line and shared among the tests that read it."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import native as nat
from scalable_video_codec_amd import synth
from tests.test_levels_budget_host import ladder

pytestmark = pytest.mark.gpu

W, H, N, LEVELS, SEED = 96, 64, 17, 3, 7
MV = 16
LADDER = ladder(8)
LADDER_ARG = ",".join(f"{fg}:{bg}" for fg, bg in LADDER.tolist())
BATCHES = {4: (4, 8, 16), 8: (8, 16)}  # key_interval -> the batches it divides

_runs = {}


def _exe(name):
    exe = os.path.join(os.path.dirname(__file__), "dropin", name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_delta_budget")
    clip = synth.SynthClip(W, H, N, SEED, device="cuda")
    torch.stack([clip.frame_bgr(t) for t in range(N)]).contiguous().cpu().numpy().tofile(d / "clip.raw")
    return d


def _encode(work, block=8, batch=4, depth=3, key_interval=4, budget=1 << 30, budget2=0, extra=None):
    """One run of stream_delta_budget_main per command line -> (its output prefix, the finished process)."""
    key = (block, batch, depth, key_interval, budget, budget2, extra)
    if key not in _runs:
        prefix = str(work / ("run%d" % len(_runs)))
        cmd = [_exe("stream_delta_budget_main"), str(work / "clip.raw"), str(W), str(H), str(N), str(LEVELS), str(block), str(batch), str(depth),
               str(SEED), str(key_interval), str(budget), LADDER_ARG, str(budget2), prefix] + ([extra] if extra else [])
        _runs[key] = (prefix, subprocess.run(cmd, capture_output=True, text=True, timeout=120))
    return _runs[key]


def _ok(run):
    prefix, r = run
    assert r.returncode == 0, r.stdout + r.stderr
    return prefix


def _keys(prefix):
    return [int(line) for line in open(prefix + ".key").read().split()]


def _device_call(work, prefix, block, budgets):
    """One call over the clip's encoded frames with the driver's own region ids and flags -> (bytes, offsets, choice u32, table)."""
    clip = torch.from_numpy(np.fromfile(work / "clip.raw", np.uint8).reshape(N, H, W, 3)[1:].copy()).cuda()
    types = torch.from_numpy(np.fromfile(prefix + ".types", np.uint32).view(np.int32).reshape(N - 1, -1).copy()).cuda()
    key = torch.tensor(_keys(prefix), dtype=torch.int32, device="cuda")
    out, offs, choice, table = nat.dct_pack_delta_budget_frames(clip, block, types, (MV, MV), LADDER, budgets, key=key, counts=True)
    torch.cuda.synchronize()
    return out[:int(offs[-1])].cpu().numpy().tobytes(), offs.cpu().tolist(), choice.cpu().numpy().view(np.uint32), table.cpu().numpy(), clip, types


def _budget_for(work, key_interval, block, entry):
    """A budget per frame under which every group of the clip lands on `entry` or finer and some group lands on a coarser entry than
    under twice as much: the mean bytes per frame of the clip at that entry, from the device call's table of the free run."""
    free = _ok(_encode(work, block=block, batch=16, key_interval=key_interval))
    table = _device_call(work, free, block, 1 << 30)[3]
    floor = 64 + 4 * (W // MV) * (H // MV) + 8 * 3 * (W // block) * (H // block) * (block * block // 64)
    size = (floor + 2 * table.astype(np.int64) + 15) // 16 * 16
    return int(size[:, entry].mean())


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("key_interval", [4, 8])
def test_one_stream_whatever_the_batch_or_depth_and_it_is_the_device_calls(native, work, key_interval, depth):
    budget = _budget_for(work, key_interval, 8, 3)
    ref = _ok(_encode(work, batch=BATCHES[key_interval][0], depth=3, key_interval=key_interval, budget=budget))
    assert _keys(ref) == [int(i % key_interval == 0) for i in range(N - 1)]
    for batch in BATCHES[key_interval]:
        other = _ok(_encode(work, batch=batch, depth=depth, key_interval=key_interval, budget=budget))
        for ext in (".big", ".offsets", ".key", ".types", ".choice"):
            assert open(ref + ext, "rb").read() == open(other + ext, "rb").read(), (ext, batch, depth)
    want, want_offs, want_choice, _, _, _ = _device_call(work, ref, 8, budget)
    assert open(ref + ".big", "rb").read() == want
    assert np.fromfile(ref + ".offsets", np.uint64).tolist() == want_offs
    choice = np.fromfile(ref + ".choice", np.uint32)
    assert choice.tolist() == want_choice.tolist()
    assert len(set(choice.tolist())) >= 2 or (choice & 0x7FFFFFFF).max() > 0  # the budget binds: not every group at the finest entry
    for g in range(0, N - 1, key_interval):  # one value per group
        assert len(set(choice[g:g + key_interval].tolist())) == 1


@pytest.mark.parametrize("block,key_interval,batch,depth", [(8, 4, 4, 3), (8, 8, 16, 4), (16, 8, 16, 3)])
def test_decode_delta_plays_what_decode_plays_from_the_plain_stream_at_the_chosen_steps(native, work, block, key_interval, batch, depth):
    budget = _budget_for(work, key_interval, block, 3)
    run = _ok(_encode(work, block=block, batch=batch, depth=depth, key_interval=key_interval, budget=budget))
    choice = np.fromfile(run + ".choice", np.uint32) & 0x7FFFFFFF
    _, _, _, _, clip, types = _device_call(work, run, block, budget)
    frames = []
    for f in range(N - 1):  # the plain stream: every frame packed alone at its group's pair
        fg, bg = (int(v) for v in LADDER[int(choice[f])])
        one, one_offs = nat.dct_pack_levels_frames(clip[f:f + 1].contiguous(), block, types[f:f + 1].contiguous(), (MV, MV), fg, bg)
        torch.cuda.synchronize()
        frames.append(one[:int(one_offs[-1])].cpu().numpy().tobytes())
    plain = run + ".plain"
    open(plain + ".big", "wb").write(b"".join(frames))
    np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.uint64).tofile(plain + ".offsets")
    out_d, out_p = run + ".display", plain + ".display"
    r = subprocess.run([_exe("stream_delta_main"), run, str(N - 1), "0", "0", "-", run + ".key", "4", "3", "1", out_d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([_exe("stream_decode_main"), plain, str(N - 1), "0", "0", "-", "4", out_p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got, want = np.fromfile(out_d, np.uint8), np.fromfile(out_p, np.uint8)
    assert got.size == want.size == (N - 1) * W * H * 3 and want.any()
    assert np.array_equal(got, want)
    assert np.fromfile(out_d + ".status", np.uint32).tolist() == [0] * (N - 1)


def test_a_new_budget_takes_effect_at_a_batch_boundary(native, work):
    """Four batches of 4 at depth 3; the sink sets a tighter budget after the first delivery.  Every batch is packed under one of the two
    budgets, the first under the first, the last under the second, and the stream is the device call's with those per-frame budgets."""
    first, second = _budget_for(work, 4, 8, 2), _budget_for(work, 4, 8, 6)
    assert second < first
    run = _ok(_encode(work, batch=4, depth=3, key_interval=4, budget=first, budget2=second))
    batches = [tuple(int(v) for v in line.split()) for line in open(run + ".batches").read().splitlines()]
    assert batches == [(0, 4), (4, 4), (8, 4), (12, 4)]
    choice = np.fromfile(run + ".choice", np.uint32)
    a = _device_call(work, run, 8, first)[2]
    b = _device_call(work, run, 8, second)[2]
    assert all(a[g] != b[g] for g in range(0, N - 1, 4))  # the two budgets tell every group apart
    switched = [g // 4 for g in range(0, N - 1, 4) if choice[g:g + 4].tolist() == b[g:g + 4].tolist()]
    kept = [g // 4 for g in range(0, N - 1, 4) if choice[g:g + 4].tolist() == a[g:g + 4].tolist()]
    assert sorted(kept + switched) == [0, 1, 2, 3] and kept and switched and max(kept) < min(switched), (kept, switched)
    budgets = [first if f // 4 in kept else second for f in range(N - 1)]
    want, want_offs, want_choice, _, _, _ = _device_call(work, run, 8, budgets)
    assert open(run + ".big", "rb").read() == want and choice.tolist() == want_choice.tolist()
    assert np.fromfile(run + ".offsets", np.uint64).tolist() == want_offs


@pytest.mark.parametrize("key_interval,batch,extra,message", [
    (0, 4, None, "not with delta"),
    (3, 4, None, "not with delta"),
    (8, 4, None, "not with delta"),  # a group would be cut across batches
    (4, 4, "auto_key", "not with delta"),
    (4, 4, "temporal", "not with delta"),
    (4, 4, "entropy", "not with delta"),
])
def test_every_other_combination_is_refused(native, work, key_interval, batch, extra, message):
    prefix, r = _encode(work, batch=batch, key_interval=key_interval, budget=100000, extra=extra)
    assert r.returncode == 1 and message in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(prefix + ".big")
