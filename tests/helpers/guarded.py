"""Guard bands and poisoned buffers: where a kernel writes, and whether its result depends on memory it was never given.

GPU AddressSanitizer is not available to this project, so a kernel's memory behaviour is checked the plain way: every buffer a call
writes is the interior of one larger allocation whose two guards hold a known pattern, and every input is copied into the interior
of such an allocation whose guards hold noise.  An index that is wrong by up to a whole buffer (the guard is at least as large as
the interior, and at least 64 KiB) lands inside the allocation, where check() finds it; nothing here can reach memory that is not
the test's own.  Device-agnostic: tests/test_guarded_host.py runs all of it on CPU tensors.

What this cannot see: a read outside an input that does not change the result, and an overrun larger than the guard.

Exact placement: `skew` puts the interior at an address that is `skew` mod `align`, and exactly(A) is the placement "a multiple of
A and not of 2A", the weakest one a pointer documented as A-byte aligned admits (exactly(1) is an odd address).
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

MIN_GUARD = 65536
POISON_NAMES = ("zeros", "ones", "random", "dirty")


def _round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _pattern(nbytes: int, seed: int) -> torch.Tensor:
    """Seeded bytes in 1 .. 254: non-constant, and never one of the poison values 0x00 and 0xFF."""
    return torch.from_numpy(np.random.default_rng(seed).integers(1, 255, nbytes, dtype=np.uint8))


def exactly(a: int) -> Dict[str, int]:
    """Keyword arguments for Guarded / like / surround: an address that is a multiple of `a` and not of 2 * a."""
    assert a >= 1 and a & (a - 1) == 0, a
    return {"align": 2 * a, "skew": a}


class Guarded:
    """One allocation of guard + nbytes + guard bytes; `interior` is a contiguous view of exactly nbytes bytes as `dtype`, at an
    address that is `skew` mod `align` (0 <= skew < align; a multiple of the element size unless dtype is u8).  guard =
    max(65536, nbytes) rounded up to align, on each side (the front one takes the few bytes that place the interior).  Both guards
    hold a seeded pattern; check() says which of their bytes changed."""

    def __init__(self, nbytes: int, dtype: torch.dtype = torch.uint8, device="cpu", align: int = 256, seed: int = 0,
                 shape: Optional[Tuple[int, ...]] = None, skew: int = 0, pin: bool = False):
        item = torch.empty(0, dtype=dtype).element_size()
        assert nbytes >= 0 and nbytes % item == 0 and align % item == 0, (nbytes, dtype, align)
        assert 0 <= skew < align and skew % item == 0, (skew, align, dtype)
        guard = _round_up(max(MIN_GUARD, nbytes), align)
        self.raw = torch.empty(2 * guard + nbytes + align, dtype=torch.uint8, device=device, pin_memory=pin)  # pin: page-locked host memory
        self.front = guard + (skew - (self.raw.data_ptr() + guard)) % align
        self.nbytes = nbytes
        self.back = self.raw.numel() - self.front - nbytes
        assert self.front >= guard and self.back >= guard
        self.bytes = self.raw[self.front:self.front + nbytes]
        self.interior = self.bytes.view(dtype)
        if shape is not None:
            self.interior = self.interior.view(shape)
        self.addr = self.raw.data_ptr() + self.front  # the interior's address (an empty view's data_ptr() need not say it)
        assert self.addr % align == skew and self.interior.is_contiguous()
        assert nbytes == 0 or self.interior.data_ptr() == self.addr
        assert self.interior.numel() * item == nbytes
        self._want_front = _pattern(self.front, 2 * seed + 1).to(device)
        self._want_back = _pattern(self.back, 2 * seed + 2).to(device)
        self.raw[:self.front] = self._want_front
        self.raw[self.front + nbytes:] = self._want_back

    def fill(self, values: Optional[torch.Tensor]) -> None:
        """Sets the interior's bytes (a u8 tensor of nbytes); None leaves what is there (the "dirty" poison)."""
        if values is not None:
            assert values.dtype == torch.uint8 and values.numel() == self.nbytes
            self.bytes.copy_(values.to(self.raw.device))

    def check(self) -> Tuple[List[int], List[int]]:
        """-> (changed guard bytes before the interior, as negative offsets from its first byte; changed guard bytes after it, as
        offsets from the byte after its last).  Both empty: nothing outside the interior was written."""
        before = torch.nonzero(self.raw[:self.front] != self._want_front).flatten().cpu()
        after = torch.nonzero(self.raw[self.front + self.nbytes:] != self._want_back).flatten().cpu()
        return (before - self.front).tolist(), after.tolist()


def like(t: torch.Tensor, seed: int = 0, align: int = 256, skew: int = 0) -> Guarded:
    """A Guarded whose interior has exactly the shape and type of t (its contents are not copied)."""
    return Guarded(t.numel() * t.element_size(), t.dtype, t.device, align, seed, tuple(t.shape), skew)


class Misplaced(torch.Tensor):
    """A typed tensor whose data_ptr() is an address torch cannot give one (an i32 array at 2 mod 4, an i64 array at 4 mod 8): shape,
    type and contents are those of `like`; data_ptr() is the interior of a u8 Guarded of the same size (`guarded`) that holds like's
    bytes, and stays that through as_tensor / reshape / to / contiguous where they return the same elements.  For calls that must
    refuse the pointer before any launch; should one launch all the same, it reads and writes inside that allocation."""

    @staticmethod
    def __new__(cls, like: torch.Tensor, seed: int = 0, align: int = 256, skew: int = 0, _guarded: Optional[Guarded] = None):
        t = like.detach().contiguous()
        self = torch.Tensor._make_subclass(cls, t)
        if _guarded is None:
            _guarded = Guarded(t.numel() * t.element_size(), torch.uint8, t.device, align, seed, skew=skew)
            _guarded.bytes.copy_(t.view(-1).view(torch.uint8))
        self.guarded = _guarded
        return self

    def data_ptr(self) -> int:
        return self.guarded.addr

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **(kwargs or {}))
            src = next((a for a in args if isinstance(a, Misplaced)), None)
            if (src is not None and isinstance(out, torch.Tensor) and not isinstance(out, Misplaced) and out.dtype == src.dtype
                    and out.numel() == src.numel() and out.is_contiguous() and out.device == src.device
                    and torch.Tensor.data_ptr(out) == torch.Tensor.data_ptr(src)):
                out = Misplaced(out, _guarded=src.guarded)  # the same elements under another shape: still at the placed address
        return out


def placed(tensor: torch.Tensor, seed: int, a: int):
    """surround(tensor) at exactly(a); a Misplaced where a is no multiple of the element size."""
    if a % tensor.element_size() == 0:
        return surround(tensor, seed, **exactly(a))
    return Misplaced(tensor, seed, **exactly(a))


def poisons(nbytes: int, seed: int) -> Iterator[Tuple[str, Optional[torch.Tensor]]]:
    """The fills of a written buffer's interior before a call: (name, u8 bytes).  "dirty" comes with None: the interior keeps what
    a previous call of another geometry or another entry point left there, and the test runs that call first."""
    yield "zeros", torch.zeros(nbytes, dtype=torch.uint8)
    yield "ones", torch.full((nbytes,), 0xFF, dtype=torch.uint8)
    yield "random", torch.from_numpy(np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8))
    yield "dirty", None


def surround(tensor: torch.Tensor, seed: int, align: int = 256, skew: int = 0) -> torch.Tensor:
    """A copy of `tensor` (same shape and type) that is the interior of a Guarded whose guards hold seeded noise: two seeds give the
    same input with different neighbours.  The view keeps the allocation alive."""
    t = tensor.contiguous()
    g = like(t, seed, align, skew)
    g.interior.copy_(t)
    return g.interior


def _sync(device) -> None:
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _first(offsets: List[int]) -> str:
    return f"{len(offsets)} byte(s), first at {offsets[0]:+d}"


def guard_findings(entry: str, written: Dict[str, Guarded], when: str) -> List[str]:
    out = []
    for name, g in written.items():
        before, after = g.check()
        if before:
            out.append(f"{entry}: wrote before buffer '{name}' ({_first(before)}) {when}")
        if after:
            out.append(f"{entry}: wrote after buffer '{name}' ({_first(after)} past its end) {when}")
    return out


def _snapshot(outputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: v.detach().clone() for k, v in outputs.items()}


def _differs(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit (NaNs and signed zeros included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return True
    return not torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def output_findings(entry: str, want: Dict[str, torch.Tensor], got: Dict[str, torch.Tensor], why: str) -> List[str]:
    assert want.keys() == got.keys(), (sorted(want), sorted(got))
    return [f"{entry}: output '{k}' {why}" for k in want if _differs(want[k], got[k])]


def check_writes(entry: str, written: Dict[str, Guarded], call: Callable[[], Dict[str, torch.Tensor]],
                 dirty: Optional[Callable[[], None]] = None, seed: int = 0,
                 names: Iterable[str] = POISON_NAMES) -> List[str]:
    """One baseline call, then one call per poison, every buffer of `written` poisoned alike before it.  call() runs the entry point
    on the interiors of `written` and returns its DEFINED outputs by name (views are fine: they are copied here).  dirty() runs
    another geometry or another entry point on the same interiors (it may write anywhere inside them).  -> the findings, as
    sentences that name the entry point and the buffer: a guard byte that changed, or a defined output that is not bit for bit
    the baseline's under some poison.  Empty: the call writes inside its buffers and does not read what it did not write."""
    device = next(iter(written.values())).raw.device
    findings: List[str] = []
    for i, g in enumerate(written.values()):  # the baseline runs on seeded bytes of its own
        g.fill(torch.from_numpy(np.random.default_rng(1000 * seed + 77 + i).integers(0, 256, g.nbytes, dtype=np.uint8)))
    base = _snapshot(call())
    _sync(device)
    findings += guard_findings(entry, written, "in the baseline call")
    for poison in names:
        if poison == "dirty":
            if dirty is None:
                continue
            dirty()
            _sync(device)
            findings += guard_findings(entry, written, "in the call that dirties the buffers")
        else:
            for i, g in enumerate(written.values()):
                g.fill(dict(poisons(g.nbytes, 1000 * seed + i))[poison])
        got = _snapshot(call())
        _sync(device)
        findings += guard_findings(entry, written, f"with its buffers filled '{poison}'")
        findings += output_findings(entry, base, got, f"depends on what its buffers held before the call (fill '{poison}')")
    return findings


def check_reads(entry: str, inputs: Dict[str, torch.Tensor], call: Callable[[Dict[str, torch.Tensor]], Dict[str, torch.Tensor]],
                written: Optional[Dict[str, Guarded]] = None, seeds: Tuple[int, int] = (1, 2)) -> List[str]:
    """call(inputs) runs the entry point on the given inputs and returns its defined outputs by name.  It runs once with every input
    surrounded with seeds[0], then once per input with that input alone surrounded with seeds[1]: the same bytes, other neighbours.
    The buffers of `written` get the same seeded fill before every call (so that only the neighbours differ between the calls) and
    their guards are checked after it.  -> the findings: an output that differs names the input whose neighbours it depends on."""
    device = next(iter(inputs.values())).device
    written = written or {}
    fills = [dict(poisons(g.nbytes, 500 + i))["random"] for i, g in enumerate(written.values())]

    def run(given, when):
        for g, f in zip(written.values(), fills):
            g.fill(f)
        got = _snapshot(call(given))
        _sync(device)
        return got, guard_findings(entry, written, when)

    first = {k: surround(v, seeds[0]) for k, v in inputs.items()}
    base, findings = run(first, "with its inputs surrounded")
    for name, v in inputs.items():
        got, bad = run({**first, name: surround(v, seeds[1])}, f"with other bytes next to input '{name}'")
        findings += bad + output_findings(entry, base, got, f"depends on the bytes next to input '{name}'")
    return findings
