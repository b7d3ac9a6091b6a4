"""svc::StreamEncoder with StreamEncoderConfig::delta and compact_quality, through tests/dropin/stream_delta_quality_main (a caller of
include/svc/stream_encoder.hpp only): the delta stream with one ladder entry per group of frames, by a PSNR every frame of the group holds
(svc_hip_dct_pack_delta_quality_frames), optionally under the group's byte budget.

A 17-frame 96 x 64 synthetic clip (16 encoded frames; the padded size is the same).  A key frame every 4 with batches of 4 and 16, every 8
with batches of 16, at depths 3 and 4, as SVCQ and as SVCE.  Whatever the batching there is one stream, one set of choices and one set of
compact_distortion, all equal to one device call over the clip with the driver's own region ids and the target layers.distortion_target
gives; svc::StreamDecoder::DecodeDelta plays what Decode plays from the plain stream packed frame by frame at the chosen steps.  A run is
made once per command line and shared among the tests that read it."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scalable_video_codec_amd import layers
from scalable_video_codec_amd import native as nat
from scalable_video_codec_amd import synth
from tests.test_levels_budget_host import ladder

pytestmark = pytest.mark.gpu

W, H, N, LEVELS, SEED = 96, 64, 17, 3, 7
MV = 16
LADDER = ladder(8)
LADDER_ARG = ",".join(f"{fg}:{bg}" for fg, bg in LADDER.tolist())
INDEX, MISSED, OVER = 0x3FFFFFFF, 0x40000000, 0x80000000
DB = 30  # (a multiple of 10: the driver's long double target is then exact, see include/svc/stream_encoder.hpp)

_runs = {}


def _exe(name):
    exe = os.path.join(os.path.dirname(__file__), "dropin", name)
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is not built (python -m scalable_video_codec_amd.build)")
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_delta_quality")
    clip = synth.SynthClip(W, H, N, SEED, device="cuda")
    torch.stack([clip.frame_bgr(t) for t in range(N)]).contiguous().cpu().numpy().tofile(d / "clip.raw")
    return d


def _encode(work, block=8, batch=4, depth=3, key_interval=4, quality=DB, budget=0, quality2=0, entropy=0, extra=None):
    """One run of stream_delta_quality_main per command line -> (its output prefix, the finished process)."""
    key = (block, batch, depth, key_interval, quality, budget, quality2, entropy, extra)
    if key not in _runs:
        prefix = str(work / ("run%d" % len(_runs)))
        cmd = [_exe("stream_delta_quality_main"), str(work / "clip.raw"), str(W), str(H), str(N), str(LEVELS), str(block), str(batch), str(depth),
               str(SEED), str(key_interval), str(quality), str(budget), LADDER_ARG, str(quality2), str(entropy), prefix] + ([extra] if extra else [])
        _runs[key] = (prefix, subprocess.run(cmd, capture_output=True, text=True, timeout=120))
    return _runs[key]


def _ok(run):
    prefix, r = run
    assert r.returncode == 0, r.stdout + r.stderr
    return prefix


def _keys(prefix):
    return [int(line) for line in open(prefix + ".key").read().split()]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_call(work, prefix, block, db, budget=None):
    """One call over the clip's encoded frames with the driver's own region ids and flags; db: one PSNR, or one per frame
    -> (bytes, offsets, choice u32, D table u64, the frames, the region ids)."""
    clip = torch.from_numpy(np.fromfile(work / "clip.raw", np.uint8).reshape(N, H, W, 3)[1:].copy()).cuda()
    types = torch.from_numpy(np.fromfile(prefix + ".types", np.uint32).view(np.int32).reshape(N - 1, -1).copy()).cuda()
    key = torch.tensor(_keys(prefix), dtype=torch.int32, device="cuda")
    target = [layers.distortion_target(v, W, H) for v in np.broadcast_to(np.asarray(db), (N - 1,)).tolist()]
    out, offs, choice, table = nat.dct_pack_delta_quality_frames(clip, block, types, (MV, MV), LADDER, target, budget, key=key, distortion=True)
    torch.cuda.synchronize()
    return (out[:int(offs[-1])].cpu().numpy().tobytes(), offs.cpu().tolist(), choice.cpu().numpy().view(np.uint32),
            table.cpu().numpy().view(np.uint64), clip, types)


def _svcq(prefix, block, entropy):
    """The run's stream as SVCQ bytes and offsets: as written, or decoded from its entropy-coded form."""
    big, offs = np.fromfile(prefix + ".big", np.uint8), np.fromfile(prefix + ".offsets", np.uint64)
    if not entropy:
        return big.tobytes(), offs.tolist()
    back, back_offs, st = nat.entropy_decode_frames(_dev(big), _dev(offs.astype(np.int64)), W, H, block, MV)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * (N - 1)
    return back[:int(back_offs[-1])].cpu().numpy().tobytes(), back_offs.cpu().tolist()


def _equals_the_device_call(work, run, block, db, budget=None, entropy=0):
    want, want_offs, want_choice, table, _, _ = _device_call(work, run, block, db, budget)
    got, got_offs = _svcq(run, block, entropy)
    assert got == want and got_offs == want_offs
    choice = np.fromfile(run + ".choice", np.uint32)
    assert choice.tolist() == want_choice.tolist()
    assert np.fromfile(run + ".distortion", np.uint64).tolist() == [int(table[f, int(c) & INDEX]) for f, c in enumerate(choice)]
    return choice, table


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("entropy", [0, 1], ids=["svcq", "svce"])
def test_one_stream_whatever_the_batch_or_depth_and_it_is_the_device_calls(native, work, entropy, depth):
    ref = _ok(_encode(work, batch=4, depth=3, key_interval=4, entropy=entropy))
    assert _keys(ref) == [int(i % 4 == 0) for i in range(N - 1)]
    for batch in (4, 16):
        other = _ok(_encode(work, batch=batch, depth=depth, key_interval=4, entropy=entropy))
        for ext in (".big", ".offsets", ".key", ".types", ".choice", ".distortion"):
            assert open(ref + ext, "rb").read() == open(other + ext, "rb").read(), (ext, batch, depth)
    choice, table = _equals_the_device_call(work, ref, 8, DB, entropy=entropy)
    target = layers.distortion_target(DB, W, H)
    for g in range(0, N - 1, 4):  # one value per group; without a cap nothing is over it, and bit 30 says what the table says
        assert len(set(choice[g:g + 4].tolist())) == 1 and not choice[g] & OVER
        met = all(int(table[f, int(choice[g]) & INDEX]) <= target for f in range(g, g + 4))
        assert bool(choice[g] & MISSED) == (not met)
        if met:  # every frame holds the PSNR
            assert min(layers.distortion_psnr(table[f, int(choice[g]) & INDEX], W, H) for f in range(g, g + 4)) >= DB


@pytest.mark.parametrize("block,key_interval,batch,depth,entropy", [(8, 4, 4, 3, 0), (8, 8, 16, 4, 1), (16, 8, 16, 3, 0)])
def test_decode_delta_plays_what_decode_plays_from_the_plain_stream_at_the_chosen_steps(native, work, block, key_interval, batch, depth, entropy):
    run = _ok(_encode(work, block=block, batch=batch, depth=depth, key_interval=key_interval, entropy=entropy))
    choice, _ = _equals_the_device_call(work, run, block, DB, entropy=entropy)
    _, _, _, _, clip, types = _device_call(work, run, block, DB)
    frames = []
    for f in range(N - 1):  # the plain stream: every frame packed alone at its group's pair
        fg, bg = (int(v) for v in LADDER[int(choice[f]) & INDEX])
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


def test_with_a_budget_the_budget_is_the_cap(native, work):
    """The budget: the mean bytes per frame of the uncapped run, less a quarter -- some group must give way."""
    free = _ok(_encode(work, batch=16, key_interval=4))
    sizes = np.diff(np.fromfile(free + ".offsets", np.uint64).astype(np.int64))
    budget = int(sizes.mean() * 3 // 4)
    run = _ok(_encode(work, batch=16, key_interval=4, budget=budget))
    choice, _ = _equals_the_device_call(work, run, 8, DB, budget)
    assert choice.tolist() != np.fromfile(free + ".choice", np.uint32).tolist()
    capped = np.diff(np.fromfile(run + ".offsets", np.uint64).astype(np.int64))
    for g in range(0, N - 1, 4):
        assert capped[g:g + 4].sum() <= 4 * budget or choice[g] & OVER


def test_a_new_quality_takes_effect_at_a_batch_boundary(native, work):
    """Four batches of 4 at depth 3; the sink sets a lower quality after the first delivery.  Every batch is packed under one of the two
    targets, the first under the first, the last under the second, and the stream is the device call's with those per-frame targets."""
    first, second = 40, 20
    run = _ok(_encode(work, batch=4, depth=3, key_interval=4, quality=first, quality2=second))
    batches = [tuple(int(v) for v in line.split()) for line in open(run + ".batches").read().splitlines()]
    assert batches == [(0, 4), (4, 4), (8, 4), (12, 4)]
    choice = np.fromfile(run + ".choice", np.uint32)
    a = _device_call(work, run, 8, first)[2]
    b = _device_call(work, run, 8, second)[2]
    assert all(a[g] != b[g] for g in range(0, N - 1, 4))  # the two targets tell every group apart
    switched = [g // 4 for g in range(0, N - 1, 4) if choice[g:g + 4].tolist() == b[g:g + 4].tolist()]
    kept = [g // 4 for g in range(0, N - 1, 4) if choice[g:g + 4].tolist() == a[g:g + 4].tolist()]
    assert sorted(kept + switched) == [0, 1, 2, 3] and kept and switched and max(kept) < min(switched), (kept, switched)
    _equals_the_device_call(work, run, 8, [first if f // 4 in kept else second for f in range(N - 1)])


def test_with_the_quality_off_the_bytes_are_the_delta_runs(native, work):
    off = _ok(_encode(work, batch=4, key_interval=4, quality=0))
    prefix = str(work / "parent_delta")
    r = subprocess.run([_exe("stream_delta_encode_main"), str(work / "clip.raw"), str(W), str(H), str(N), str(LEVELS), "8", "4", "3", str(SEED), "1", "4",
                        "0", prefix], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for ext in (".big", ".offsets", ".key", ".types"):
        assert open(off + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    assert os.path.getsize(off + ".choice") == 0 and os.path.getsize(off + ".distortion") == 0


@pytest.mark.parametrize("key_interval,batch,budget,entropy,extra,message", [
    (0, 4, 0, 0, None, "compact_quality picks one pair of steps per group of frames"),
    (3, 4, 0, 0, None, "compact_quality picks one pair of steps per group of frames"),
    (8, 4, 0, 0, None, "compact_quality picks one pair of steps per group of frames"),  # a group would be cut across batches
    (4, 4, 0, 0, "auto_key", "compact_quality needs the groups before it chooses, auto_key"),
    (4, 4, 0, 0, "temporal", "compact_quality picks one pair of steps per group of consecutive frames: not with temporal_period"),
    (4, 4, 0, 0, "enh", "compact_quality measures one layer: not with enh_step"),
    (4, 4, 0, 0, "nodelta", "compact_quality holds every frame of the delta stream at a PSNR: not without delta"),
    (4, 4, 100000, 1, None, "not with delta"),  # the cap counts uncoded bytes: a budget's own rule
])
def test_every_other_combination_is_refused(native, work, key_interval, batch, budget, entropy, extra, message):
    prefix, r = _encode(work, batch=batch, key_interval=key_interval, budget=budget, entropy=entropy, extra=extra)
    assert r.returncode == 1 and message in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(prefix + ".big")
