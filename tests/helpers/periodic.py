"""Periodic batches for tests/test_gpu_large_streams.py: a cycle of k frames repeated until the frame offsets pass 2^32, the outputs a call
must give for it, stated from the call's numpy statement on a 2k-frame prefix, and the comparison on the device the stream lies on.

A batch is `cycle * m` plus a remainder.  A call that treats every frame alike (its per-frame arguments repeating with the cycle) gives
frames [k, 2k) of its output on the prefix again for every later cycle: the period.  Frames [0, k) are the head; they differ from the period
only for the calls that look at the frame before (frame 0 has none), and a later cycle that starts with a key frame (`restarts`) gives the
head again.  Nothing here makes an array of the whole stream on the host: offsets are (n + 1,) int64, the stream is compared as
out[a:a + m * L].view(m, L) against the L bytes of one cycle, a few hundred MiB at a time.

`wrap` is 2^32 everywhere but in tests/test_large_streams_host.py, which stands a small modulus in for it."""
import numpy as np
import torch

WRAP = 1 << 32
CHUNK = 1 << 28  # bytes compared at a time


def offsets(cycle_offsets, n):
    """The n + 1 offsets of the cycle repeated: (f // k) * P + cycle_offsets[f % k], int64."""
    c = np.asarray(cycle_offsets).astype(np.int64)
    assert c[0] == 0 and (np.diff(c) >= 0).all()
    k = c.size - 1
    f = np.arange(n + 1, dtype=np.int64)
    return (f // k) * c[-1] + c[f % k]


def frames_to_cross(cycle_bytes, k, wrap=None, extra=3):
    """The fewest frames with two whole cycles above `wrap` in a stream of cycle_bytes a cycle, and `extra` frames of a partial cycle."""
    wrap = WRAP if wrap is None else wrap
    return (-(-wrap // int(cycle_bytes)) + 2) * k + extra


def crossing(offs, k, wrap=None):
    """Asserts, from the offsets alone, what every case needs before its call: a frame that starts below `wrap` and ends above it, two
    whole cycles above `wrap`, more than one 256-frame trip.  -> the straddling frame."""
    wrap = WRAP if wrap is None else wrap
    offs = np.asarray(offs).astype(np.int64)
    n = offs.size - 1
    assert n > 256, f"{n} frames are one trip of 256"
    s = int(np.searchsorted(offs, wrap, side="right")) - 1  # the last frame that starts at or below wrap
    assert 0 <= s < n and offs[s] < wrap < offs[s + 1], f"no frame straddles {wrap}: frame {s} is [{offs[min(s, n)]}, {offs[min(s + 1, n)]})"
    first = -(-(s + 1) // k)  # the first cycle that starts above wrap
    assert offs[first * k] > wrap and (first + 2) * k <= n, f"fewer than two whole cycles above {wrap}: {n} frames, frame {s} straddles"
    return s


def split_frames(data, offs):
    """bytes + (m + 1,) offsets -> the m frames as bytes."""
    b = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    o = [int(v) for v in np.asarray(offs).reshape(-1)]
    assert o[-1] == len(b), (o[-1], len(b))
    return [b[x:y] for x, y in zip(o[:-1], o[1:])]


class Periodic:
    """What a call writes for n frames of a periodic batch, from its output on the 2k-frame prefix."""

    def __init__(self, data, offs, k, n, restarts=(0,)):
        """data, offs: the numpy statement's bytes and (2k + 1,) offsets for the prefix; restarts: the frames, multiples of k, whose cycle
        comes out as the head does (frame 0; a key frame later on)."""
        frames = split_frames(data, offs)
        assert len(frames) == 2 * k and all(r % k == 0 and r < n for r in restarts) and 0 in restarts
        self.k, self.n = k, n
        self.head, self.period = frames[:k], frames[k:]
        self.heads = sorted(r // k for r in restarts)
        sizes = np.array([[len(f) for f in self.period], [len(f) for f in self.head]], np.int64)
        f = np.arange(n, dtype=np.int64)
        self.is_head = np.isin(np.arange(-(-n // k)), self.heads)  # per cycle, the partial one included
        self.sizes = sizes[self.is_head[f // k].astype(np.int64), f % k]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    def cycle_bytes(self):
        return sum(len(f) for f in self.period)

    def runs(self):
        """(first cycle, whole cycles, head?) for every stretch of like cycles, then (cycle, 0, head?) for the partial one."""
        whole = self.n // self.k
        kinds = self.is_head[:whole]
        edges = [0] + [int(i) + 1 for i in np.flatnonzero(kinds[1:] != kinds[:-1])] + [whole] if whole else [0, 0]
        out = [(a, b - a, bool(kinds[a])) for a, b in zip(edges[:-1], edges[1:]) if b > a]
        if self.n % self.k:
            out.append((whole, 0, bool(self.is_head[whole])))
        return out

    def block(self, head, device, frames=None):
        """One cycle's bytes (its first `frames` frames) as a u8 tensor."""
        fr = (self.head if head else self.period)[:frames]
        return torch.from_numpy(np.frombuffer(b"".join(fr), np.uint8).copy()).to(device)

    def materialize(self, device):
        """The whole expected stream on `device`: the input of the next call of a chain."""
        out = torch.empty(int(self.offsets[-1]), dtype=torch.uint8, device=device)
        for c0, m, head in self.runs():
            b = self.block(head, device, None if m else self.n % self.k)
            a = int(self.offsets[c0 * self.k])
            if b.numel():
                out[a:a + max(m, 1) * b.numel()].view(max(m, 1), b.numel()).copy_(b)
        return out


def differing_frames(out, exp):
    """(n,) bool: the frames of `out` (a u8 tensor, on any device) that are not exp's bytes at exp's offsets."""
    k, n = exp.k, exp.n
    bad = np.zeros(n, bool)
    if out.numel() < int(exp.offsets[-1]):
        raise AssertionError(f"the stream holds {out.numel()} bytes, {int(exp.offsets[-1])} expected")
    for c0, m, head in exp.runs():
        frames = k if m else n % k
        block = exp.block(head, out.device, frames)
        length = block.numel()
        inner = np.concatenate([[0], np.cumsum([len(f) for f in (exp.head if head else exp.period)[:frames]])])
        if length == 0:
            continue
        step = max(1, CHUNK // length)
        for i in range(0, max(m, 1), step):
            rows = min(step, max(m, 1) - i)
            a = int(exp.offsets[(c0 + i) * k])
            neq = out[a:a + rows * length].view(rows, length) != block
            for j in range(frames):
                if inner[j + 1] > inner[j]:
                    bad[(c0 + i) * k + j:(c0 + i + rows) * k:k] = neq[:, inner[j]:inner[j + 1]].any(dim=1).cpu().numpy()
            del neq
    return bad


def mismatch(out, got_offsets, exp, wrap=None):
    """None, or what differs: the first wrong offset; else the first frame whose bytes differ and the first frame that starts at or above `wrap`
    (the frame a 32-bit offset would misplace first), with whether it differs."""
    wrap = WRAP if wrap is None else wrap
    got = np.asarray(got_offsets.cpu() if isinstance(got_offsets, torch.Tensor) else got_offsets).astype(np.int64).reshape(-1)
    if got.shape != exp.offsets.shape:
        return f"{got.size} offsets, {exp.offsets.size} expected"
    wrong = np.flatnonzero(got != exp.offsets)
    if wrong.size:
        i = int(wrong[0])
        return (f"offsets[{i}] = {int(got[i])}, expected {int(exp.offsets[i])} ({wrong.size} offsets differ; the first to pass {wrap} "
                f"is offsets[{int(np.searchsorted(exp.offsets, wrap, side='right'))}])")
    bad = differing_frames(out, exp)
    if not bad.any():
        return None
    above = int(np.searchsorted(exp.offsets[:-1], wrap, side="left"))  # the first frame that starts at or above wrap
    first = int(np.flatnonzero(bad)[0])
    if above >= exp.n:
        return (f"{int(bad.sum())} of {exp.n} frames differ, the first frame {first} at byte {int(exp.offsets[first])}; no frame starts at or "
                f"above {wrap}")
    return (f"{int(bad.sum())} of {exp.n} frames differ, the first frame {first} at byte {int(exp.offsets[first])}; frame {above}, the first "
            f"to start at or above {wrap}, {'differs' if bad[above] else 'matches'}, and {int(bad[above:].sum())} of the {exp.n - above} "
            f"frames from it on differ")


def row_mismatch(out, ref, k, restarts=(0,), what="row"):
    """For outputs of one fixed-size row per frame (rec, display, planes, types, records): None, or which frames of out (n, ...) are not
    bit for bit the row the 2k-frame prefix gives them -- ref (2k, ...), the same dtype: ref[f % k] in the cycles of `restarts`,
    ref[k + f % k] elsewhere."""
    n = out.shape[0]
    assert ref.shape[0] == 2 * k and ref.dtype == out.dtype and ref.shape[1:] == out.shape[1:], (out.shape, ref.shape, out.dtype, ref.dtype)
    o, r = out.reshape(n, -1), ref.reshape(2 * k, -1).to(out.device)
    if o.dtype.is_floating_point:  # bits, not values: -0.0 and NaN payloads count
        bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[o.element_size()]
        o, r = o.view(bits), r.view(bits)
    f = torch.arange(n, device=out.device)
    heads = torch.tensor(sorted(x // k for x in restarts), device=out.device)
    want = f % k + k * (~torch.isin(f // k, heads)).to(torch.int64)
    step = max(1, CHUNK // max(1, o.shape[1] * o.element_size()))
    bad = torch.zeros(n, dtype=torch.bool, device=out.device)
    for a in range(0, n, step):
        bad[a:a + step] = (o[a:a + step] != r.index_select(0, want[a:a + step])).any(dim=1)
    if not bool(bad.any()):
        return None
    first = int(torch.nonzero(bad)[0])
    return f"{int(bad.sum())} of {n} {what}s differ from the prefix's, the first at frame {first}"


def range_sums(rows, k, a, b, restarts=(0,)):
    """The column sums of a per-frame row table over frames [a, b) of a periodic batch, as Python integers.  rows: the (2k, L) table of
    the prefix, integers; the row of frame f is rows[f % k] in the cycles of `restarts` (frames, multiples of k) and rows[k + f % k]
    elsewhere, as in row_mismatch.  Whole cycles x the cycle's sum + the head cycles + the remainder: no table of n rows is made and
    nothing is held in a fixed width.  -> a list of L ints."""
    r = [[int(v) for v in row] for row in np.asarray(rows).reshape(2 * k, -1)]
    assert 0 <= a <= b and all(x % k == 0 for x in restarts)
    heads = sorted(x // k for x in restarts)
    L = len(r[0])
    cum = [[[sum(row[j] for row in r[base:base + m]) for j in range(L)] for m in range(k + 1)] for base in (k, 0)]  # [period, head][m]

    def upto(f):  # frames [0, f)
        c, m = divmod(f, k)
        h = sum(1 for x in heads if x < c)
        part = cum[1 if c in heads else 0][m]
        return [h * cum[1][k][j] + (c - h) * cum[0][k][j] + part[j] for j in range(L)]
    return [y - x for x, y in zip(upto(a), upto(b))]


def first_fit(fits, over=0x80000000):
    """The budgeted calls' rule on one group: the first entry that fits, else the last with bit 31 set."""
    return fits.index(True) if True in fits else (len(fits) - 1) | over


def truncation_flips(totals, allowed, choose=first_fit, wrap=None):
    """The precondition of a case on sums past `wrap`: with the group's bytes per entry (`totals`) or its budget (`allowed`) taken modulo
    `wrap` -- either one alone -- the comparison bytes <= allowed comes out differently for some entry, and choose(fits per entry) gives
    another value than with the whole sums.  Asserts both; -> the choice with the whole sums."""
    wrap = WRAP if wrap is None else wrap
    totals, allowed = [int(t) for t in totals], int(allowed)
    whole = [t <= allowed for t in totals]
    for what, fits in (("bytes", [t % wrap <= allowed for t in totals]), ("allowed", [t <= allowed % wrap for t in totals])):
        assert fits != whole, f"{what} modulo {wrap}: every comparison stays {whole} (bytes {totals}, allowed {allowed})"
        assert choose(fits) != choose(whole), f"{what} modulo {wrap}: the choice stays {choose(whole)} (bytes {totals}, allowed {allowed})"
    return choose(whole)


def repeat_rows(rows, n, device, dtype=torch.int32):
    """k rows of per-frame arguments (u32 values) repeated with the cycle -> (n, len(row)) i32 on `device`."""
    a = np.asarray(rows, dtype=np.uint32)
    a = a.reshape(a.shape[0], -1)
    t = torch.from_numpy(a.view(np.int32).copy()).to(device)
    return t.repeat(-(-n // a.shape[0]), 1)[:n].contiguous().to(dtype)
