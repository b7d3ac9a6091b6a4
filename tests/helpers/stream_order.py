"""Stream order and host waits: does a device entry point do ALL its work on the stream it was given, and does it only enqueue?

include/svc_hip.h promises both for every entry point that takes a `void* stream`.  On the null stream, where every other GPU test
runs, a launch with stream 0, a memset on the wrong stream, a fork that is not joined back and a stray hipStreamSynchronize all give
the right bytes.  Here the call runs on a non-blocking side stream BEHIND A DELAY, while its input buffers still hold another
well-formed case (`stale`): the device copies that put the real inputs back are enqueued behind the delay too.  Work that does not wait
for the side stream reads the stale case, or writes before the poison is overwritten in order, and an output differs from the same
call's null-stream result.  A proxy in front of the library (Proxy: native.load() returns it while a test runs) looks at the delay's
"done" event just before and just after the C call: done before, the case is void; done after, the call waited on the host.

Findings are sentences that name the entry point (the letters are those of check_order's docstring).  The pure parts -- the header's
declarations, the rule that says which signature takes a stream, valid(), judge() and the wording -- need no device:
tests/test_stream_order_host.py.

What makes a run valid is checked in every case: the delay, measured with two events, lasts at least MARGIN times the host time
between enqueueing it and the proxy's query after the C call (a descheduled host thread may take 4 times as long and the stale
inputs are still in place when a stray launch starts).  A case that misses this is reported as inconclusive, which fails the test.
Measured over whole runs of tests/test_gpu_stream_order.py on an MI355X (271 tests, 13 s): the delay lasted 19.9 to 20.1 ms; the largest
host time of a form that is not blocking was 0.96 to 1.06 ms from run to run (segmentation callers), of a single caller 0.83 ms
(svc_hip_split_levels_budget_frames, whose binding builds the ladder first); no case was inconclusive.  4 x 1.06 ms is well below
20 ms, so the delay finally chosen is the 20 ms it started from.

What this cannot see: a stray launch on a stream that shares the side stream's hardware queue (it is held back by the delay like an
ordered one; side_stream() therefore takes only streams beside which the NULL stream is seen to run), a launch that strays but
reads nothing the stale case changes, and a host wait on anything but the caller's stream.
"""
from __future__ import annotations

import re
import threading
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from tests.helpers import guarded as gd

# The delay of every case and the factor between it and the host time of the case (a margin for a descheduled host thread); the
# measurements behind the 20 ms are in the docstring above.
START_DELAY_MS = 20.0
MARGIN = 4.0
POISON = 0xA5


# ---- the header and the signatures: which entry points take a stream, and where ----------------------------------------------------------

def strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def header_stream_params(header_text: str) -> Dict[str, Tuple[int, int]]:
    """Every declaration of include/svc_hip.h with a parameter `void* stream` -> name: (the parameter's index, the parameter count)."""
    out = {}
    text = "\n".join(l for l in strip_comments(header_text).splitlines() if not l.lstrip().startswith("#"))
    for statement in text.split(";"):
        m = re.search(r"\b(svc_hip_\w+)\s*\(([^()]*)\)\s*$", statement, flags=re.S)
        if not m:
            continue
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        at = [i for i, p in enumerate(params) if re.fullmatch(r"void ?\* ?stream", p)]
        if at:
            assert len(at) == 1, (m.group(1), params)
            out[m.group(1)] = (at[0], len(params))
    return out


def signature_stream_index(name: str, restype, argtypes) -> Optional[int]:
    """Where a function of native.SIGNATURES takes its stream, told from the signature alone; None: it takes none.  The stream is the
    last argument of a device entry point (an int-returning function that is neither a host form, `*_host`, nor a communicator call,
    whose last pointer is the communicator or the id); the temporal calls take their period after it."""
    import ctypes as C
    if restype is not C.c_int or name.endswith("_host") or name.startswith("svc_hip_comm_") or not argtypes:
        return None
    if argtypes[-1] is C.c_void_p:
        return len(argtypes) - 1
    if name.endswith("_temporal_frames") and len(argtypes) >= 2 and argtypes[-1] is C.c_uint32 and argtypes[-2] is C.c_void_p:
        return len(argtypes) - 2
    return None


def stream_entry_points(signatures) -> Dict[str, int]:
    out = {}
    for name, (res, args) in signatures.items():
        at = signature_stream_index(name, res, args)
        if at is not None:
            out[name] = at
    return out


# ---- findings: the wording, and the judging of the first call behind a delay ---------------------------------------------------------------

def f_output(entry: str, name: str) -> str:
    return (f"{entry}: (a) output '{name}' on a side stream behind a delay is not bit for bit the null-stream result: "
            "some of its work does not wait for the caller's stream")


def f_stream(entry: str, got: int, want: int) -> str:
    return f"{entry}: (b) the C function was given stream {got:#x}, not the side stream's handle {want:#x}"


def f_void(entry: str) -> str:
    return (f"{entry}: (c) the delay had already ended before the C call: the case is void (something in front of the call waits on "
            "the host); rebuild it on preallocated buffers")


def f_wait(entry: str) -> str:
    return f"{entry}: (d) the delay had ended when the C call returned: the call waited on the host, and it is not listed as blocking"


def f_inconclusive(entry: str, delay_ms: float, host_ms: float) -> str:
    return (f"{entry}: inconclusive: the delay lasted {delay_ms:.2f} ms, less than {MARGIN:g} x the {host_ms:.2f} ms the host took "
            "from enqueueing it to the query after the call")


def f_no_call(entry: str) -> str:
    return f"{entry}: no entry point that takes a stream was called behind the delay"


def f_wrong_call(entry: str, got: str) -> str:
    return f"{entry}: the first call behind the delay was {got}, not the entry point under test"


def f_raised(entry: str, error: BaseException) -> str:
    return f"{entry}: (a) the call on a side stream behind a delay failed: {type(error).__name__}: {error}"


def f_same(entry: str) -> str:
    return f"{entry}: the case is blind: the stale inputs equal the real ones, so a launch out of order could not be seen"


def f_blind(entry: str) -> str:
    return (f"{entry}: the case is blind: on the stale inputs every output is bit for bit the reference, so a launch out of order "
            "would write the right bytes")


def f_apart(entry: str) -> str:
    return f"{entry}: inconclusive: an earlier caller's delay had ended when this caller's call was enqueued: the calls did not overlap"


def valid(delay_ms: float, host_ms: float) -> bool:
    return delay_ms >= MARGIN * host_ms


@dataclass
class Record:
    """What the proxy saw of the first stream-taking call behind a delay."""
    name: str
    stream: int
    done_before: bool
    done_after: bool
    t_before: float
    t_after: float
    peers_done: int = 0


def judge(entry: str, rec: Optional[Record], want_stream: int, blocking: bool, delay_ms: float, t0: float) -> List[str]:
    """Findings (b), (c), (d) and the validity of the run.  A void case says nothing else; a call that waited is not also
    inconclusive (its host time includes the delay).  A blocking form's host time is taken up to the query BEFORE the call."""
    if rec is None:
        return [f_no_call(entry)]
    out = []
    if rec.name != entry:
        out.append(f_wrong_call(entry, rec.name))
    if rec.stream != want_stream:
        out.append(f_stream(entry, rec.stream, want_stream))
    if rec.done_before:
        return out + [f_void(entry)]
    if rec.done_after and not blocking:
        return out + [f_wait(entry)]
    host_ms = ((rec.t_before if blocking else rec.t_after) - t0) * 1e3
    if not valid(delay_ms, host_ms):
        out.append(f_inconclusive(entry, delay_ms, host_ms))
    return out


# ---- the proxy ---------------------------------------------------------------------------------------------------------------------------------

@dataclass
class Watch:
    """One delay a thread has enqueued: query() says whether it has ended.  The first stream-taking call of that thread is recorded."""
    query: Callable[[], bool]
    on_judged: Optional[Callable[[], None]] = None
    record: Optional[Record] = None
    later: List[str] = field(default_factory=list)


class Proxy:
    """Forwards every attribute to the library.  A function that takes a stream (stream_index: name -> position) or a fake registered
    under a made-up svc_hip_ name (fakes: name -> (callable, position)) is wrapped: for the calling thread's armed Watch, the first such
    call is recorded with the stream it was given and the delay's state just before and just after the C call."""

    def __init__(self, lib, stream_index: Dict[str, int], fakes: Optional[Dict[str, Tuple[Callable, int]]] = None):
        self._lib, self._index, self._fakes = lib, dict(stream_index), dict(fakes or {})
        self._watches: Dict[int, Watch] = {}
        self._group: List[Watch] = []

    def arm(self, watch: Watch) -> None:
        self._watches[threading.get_ident()] = watch
        self._group.append(watch)

    def disarm(self) -> None:
        self._watches.pop(threading.get_ident(), None)

    def new_group(self) -> None:
        self._group = []

    def __getattr__(self, name: str):
        if name in self._fakes:
            fn, at = self._fakes[name]
        else:
            fn = getattr(self._lib, name)
            if name not in self._index:
                return fn
            at = self._index[name]

        def wrapped(*args):
            watch = self._watches.get(threading.get_ident())
            if watch is None:
                return fn(*args)
            if watch.record is not None:  # only the first call behind a delay is judged
                watch.later.append(name)
                return fn(*args)
            before, t_before = watch.query(), time.perf_counter()
            rc = fn(*args)
            after, t_after = watch.query(), time.perf_counter()
            peers = sum(1 for w in self._group if w is not watch and w.query())
            watch.record = Record(name, int(args[at] or 0), before, after, t_before, t_after, peers)
            if watch.on_judged is not None:
                watch.on_judged()
            return rc
        return wrapped


def install(monkeypatch, native, fakes=None) -> Proxy:
    """native.load() returns the cached native._lib: swap it for a Proxy until the test ends."""
    proxy = Proxy(native.load(), stream_entry_points(native.SIGNATURES), fakes)
    monkeypatch.setattr(native, "_lib", proxy)
    return proxy


# ---- the delay ------------------------------------------------------------------------------------------------------------------------------------

class Delay:
    """A kernel that keeps a stream busy for about `ms` milliseconds: torch.cuda._sleep where it exists, calibrated once per session with
    two events; otherwise a chain of large element-wise operations, calibrated alike.  enqueue() brackets it with events, so every use
    knows its measured length."""
    _per_ms: Optional[float] = None  # spin cycles (or chain links) per millisecond
    _chain: Optional[torch.Tensor] = None

    def __init__(self, ms: float = START_DELAY_MS):
        self.ms = ms
        if Delay._per_ms is None:
            Delay._per_ms = self._calibrate()

    @classmethod
    def _spin(cls, units: int) -> None:
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(units))
        else:
            if cls._chain is None:
                cls._chain = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
            for _ in range(int(units)):
                cls._chain.mul_(1.0000001)

    @classmethod
    def _calibrate(cls) -> float:
        units = 1_000_000 if hasattr(torch.cuda, "_sleep") else 8
        cls._spin(1)
        torch.cuda.synchronize()
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cls._spin(units)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0:
                return units / ms
            units *= 8
        raise AssertionError("the delay kernel cannot be calibrated: it never lasts 2 ms")

    def enqueue(self) -> Tuple[torch.cuda.Event, torch.cuda.Event]:
        start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self._spin(max(1, round(self.ms * Delay._per_ms)))
        done.record()
        return start, done


_independent: Dict[int, bool] = {}  # a pool stream's handle -> the null stream runs beside it


def _runs_beside_the_null_stream(stream: torch.cuda.Stream) -> bool:
    """HIP multiplexes streams onto a few hardware queues.  A side stream that shares the null stream's queue holds a stray launch on
    stream 0 back for the length of the delay, like an ordered one, and the harness would see nothing: such a stream is not used.
    Probe: a short delay on `stream`, then a small operation on the null stream; it must end while the delay still runs."""
    Delay()
    flag = torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        Delay._spin(max(1, round(3.0 * Delay._per_ms)))
        done = torch.cuda.Event()
        done.record()
    flag.add_(1)
    ran = torch.cuda.Event()
    ran.record()
    ran.synchronize()
    beside = not done.query()
    torch.cuda.synchronize()
    return beside


def side_stream(avoid=()) -> torch.cuda.Stream:
    """A non-blocking stream of torch's pool (they are created non-blocking) beside which the null stream runs, and none of `avoid`."""
    for _ in range(64):
        s = torch.cuda.Stream()
        if s.cuda_stream == 0 or s == torch.cuda.default_stream() or s.cuda_stream in avoid:
            continue
        if s.cuda_stream not in _independent:
            _independent[s.cuda_stream] = _runs_beside_the_null_stream(s)
        if _independent[s.cuda_stream]:
            return s
    raise AssertionError("no stream of the pool runs beside the null stream: the harness cannot see a launch on stream 0")


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------

def put(dst: torch.Tensor, src: torch.Tensor) -> None:
    """src's bytes into dst's buffer: zero-padded where src is shorter, cut where it is longer.  The cut is safe: only a stray launch
    ever reads this state, the calls are given the byte count of the real buffer, and a stale offsets array that points past it
    names a truncated frame, which the stream readers refuse (their contract, pinned in the damaged-frame tests)."""
    d, s = dst.view(-1).view(torch.uint8), src.contiguous().view(-1).view(torch.uint8)
    n = min(d.numel(), s.numel())
    d[:n] = s[:n]
    d[n:] = 0


def _poison(written: Dict[str, gd.Guarded]) -> None:
    for g in written.values():
        g.bytes.fill_(POISON)


def _same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.numel() == b.numel() and not gd._differs(a.contiguous().view(-1), b.contiguous().view(-1).view(a.dtype))


class _Caller:
    """One caller's buffers: private copies of its inputs (the builders share cached inputs: those stay as they are), the null-stream
    reference, a side stream that has run the call once (the allocator keeps a pool per stream)."""

    def __init__(self, entry, inputs, stale, call, written, avoid=()):
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        self.entry, self.call, self.written = entry, call, written
        self.real = {k: v.detach().clone() for k, v in inputs.items()}
        self.mine = {k: v.detach().clone() for k, v in inputs.items()}
        self.stale = stale
        assert stale.keys() == inputs.keys(), (sorted(stale), sorted(inputs))
        self.want = gd._snapshot(call(self.mine))  # 1. the reference; code loading and side-stream creation happen here
        torch.cuda.synchronize()
        self.side = side_stream(avoid)
        assert self.side != torch.cuda.default_stream() and self.side.cuda_stream != 0, "the side stream is the default stream"
        with torch.cuda.stream(self.side):
            self.call(self.mine)
        torch.cuda.synchronize()
        self.watch = self.got = self.error = self.t0 = self.start = self.done = None

    def _blind(self) -> bool:
        """The stale case as a stray launch would find it, run once on the null stream: at least one output must differ from the
        reference, or a launch out of order would write the right bytes and pass.  A call that fails on it (a pin of the closure, a
        frame the library refuses) would fail behind the delay as well: seen."""
        try:
            got = gd._snapshot(self.call(self.mine))
        except Exception:
            return False
        finally:
            torch.cuda.synchronize()
        return not any(gd._differs(self.want[k], got[k]) for k in self.want)

    def prepare(self) -> List[str]:
        for k in self.mine:    # 3. (in front of 2.: the stale case is run once, then everything it wrote is poisoned)
            put(self.mine[k], self.stale[k])
        torch.cuda.synchronize()
        found = []
        if all(_same_bytes(self.mine[k], self.real[k]) for k in self.mine):
            found.append(f_same(self.entry))
        elif self._blind():
            found.append(f_blind(self.entry))
        _poison(self.written)  # 2.
        for k in self.mine:    # the inputs again: a call may not write them, but nothing here relies on that
            put(self.mine[k], self.stale[k])
        torch.cuda.synchronize()  # 4.
        return found

    def enqueue(self, proxy: Proxy, delay: Delay, on_judged=None) -> None:
        """5. on the side stream: the delay, "delay done", the real inputs, the call."""
        try:
            with torch.cuda.stream(self.side):
                assert torch.cuda.current_stream() != torch.cuda.default_stream()
                self.t0 = time.perf_counter()
                self.start, self.done = delay.enqueue()
                self.watch = Watch(self.done.query, on_judged)
                for k in self.mine:
                    self.mine[k].copy_(self.real[k], non_blocking=True)
                proxy.arm(self.watch)
                self.got = gd._snapshot(self.call(self.mine))
        except Exception as e:  # an assertion of the closure on garbage outputs, or a status the library returned
            self.error = e
        finally:
            proxy.disarm()

    def findings(self, blocking: bool, overlap: bool = False) -> List[str]:
        torch.cuda.synchronize()
        delay_ms = self.start.elapsed_time(self.done)
        rec = self.watch.record
        out = judge(self.entry, rec, self.side.cuda_stream, blocking, delay_ms, self.t0)
        if rec is not None:
            print(f"[stream order] {self.entry}: delay {delay_ms:.2f} ms, host {(rec.t_after - self.t0) * 1e3:.3f} ms "
                  f"({(rec.t_before - self.t0) * 1e3:.3f} ms before the call)")
            if overlap and rec.peers_done and not blocking:
                out.append(f_apart(self.entry))
        if self.error is not None:
            out.append(f_raised(self.entry, self.error))
        else:
            assert self.want.keys() == self.got.keys(), (sorted(self.want), sorted(self.got))
            out += [f_output(self.entry, k) for k in self.want if gd._differs(self.want[k], self.got[k])]
        return out


def check_order(entry: str, inputs: Dict[str, torch.Tensor], stale: Dict[str, torch.Tensor], call, written: Dict[str, gd.Guarded],
                proxy: Proxy, delay: Optional[Delay] = None, blocking: bool = False) -> List[str]:
    """entry: the C function's name.  call(inputs) runs it through native (on native._stream()) and returns its defined outputs by name;
    `written`: every buffer it writes, workspace included; `stale`: the same case built with another seed.
     1. on the null stream, call(inputs): the reference;  2. every written buffer is poisoned;  3. `stale` goes into the input buffers;
     4. the device is synchronised;  5. on a non-blocking side stream: a delay, "delay done", device copies that put the real inputs
     back, call(inputs).
    -> the findings: (a) an output is not bit for bit the reference; (b) the C function got another stream than the side stream's;
    (c) the delay was over before the C call (void: a failure); (d) it was over when the C call returned and the form is not
    `blocking`; or the run is inconclusive (valid()); or the case is blind: run once on the null stream in front of 2., the stale case
    gives every output of the reference, so that a launch out of order would pass."""
    c = _Caller(entry, inputs, stale, call, written)
    found = c.prepare()
    proxy.new_group()
    c.enqueue(proxy, delay or Delay())
    return found + c.findings(blocking)


def check_concurrent(entry: str, callers, proxy: Proxy, delay: Optional[Delay] = None, blocking: bool = False,
                     threads: bool = True) -> List[str]:
    """callers: [(inputs_i, stale_i, call_i, written_i)], each with buffers of its own.  Each gets a side stream of its own and is enqueued
    behind a delay of its own, so that the calls overlap on the device; each must equal its own null-stream reference, and (b) to (d)
    hold for each.  threads: a host thread per caller (the closures read their outputs back, which waits for the caller's delay); the
    threads take turns from enqueueing the delay to the return of the C call, so the library is entered by one thread at a time.
    Without threads everything is enqueued from this thread, for closures that do not wait.  A caller whose call was enqueued after
    an earlier caller's delay had ended did not overlap with it: inconclusive."""
    delay = delay or Delay()
    cs = []
    for c in callers:
        cs.append(_Caller(entry, *c, avoid={o.side.cuda_stream for o in cs}))
    found = []
    for c in cs:
        found += c.prepare()
    proxy.new_group()
    if threads:
        turn = threading.Lock()
        # the threads end together: what a thread's end releases (the library keeps staging buffers per host thread, and freeing
        # device memory waits for the whole device) must not fall into another caller's delay and hold its host thread up
        end = threading.Barrier(len(cs))

        def run(c):
            turn.acquire()
            released = []

            def release():
                if not released:
                    released.append(1)
                    turn.release()
            try:
                c.enqueue(proxy, delay, release)
            finally:
                release()
                try:
                    end.wait(timeout=120)
                except threading.BrokenBarrierError:
                    pass
        workers = [threading.Thread(target=run, args=(c,)) for c in cs]
        for t in workers:
            t.start()
        for t in workers:
            t.join()
    else:
        for c in cs:
            c.enqueue(proxy, delay)
    for i, c in enumerate(cs):
        found += [f"caller {i}: {f}" for f in c.findings(blocking, overlap=True)]
    return found
