"""tests/helpers/guarded.py catches what it claims to (no GPU): the stand-in "kernels" are plain torch functions on CPU tensors,
four of them faulty in the four ways the GPU tests look for, one correct.  Each faulty one must be reported with the buffer named."""
import pytest
import torch

from tests.helpers import guarded as gd

N = 40  # elements of the stand-ins' input


def _ptr_view(t: torch.Tensor, first: int, count: int) -> torch.Tensor:
    """`count` elements starting `first` elements from t's first, inside t's allocation: what a kernel's bad index reaches."""
    return torch.as_strided(t, (count,), (1,), t.storage_offset() + first)


def _sum_kernel(src, out, scratch, fault=None):
    """out[0] = sum(src), through per-element partial sums in scratch.  `fault` picks the defect."""
    if fault == "write_before":
        _ptr_view(out, -1, 1)[0] = 7
    if fault == "write_after":
        _ptr_view(scratch, scratch.numel(), 1)[0] = 7
    if fault != "stale_scratch":
        scratch.zero_()
    scratch += src  # a kernel that accumulates into scratch it never cleared
    out[0] = scratch.sum()
    if fault == "read_after":
        out[0] += _ptr_view(src, src.numel(), 1)[0]


def _run(fault):
    src = torch.arange(N, dtype=torch.int32) * 3 + 1
    inside = gd.surround(src, 0)  # a stand-in's bad index must stay inside an allocation here too
    written = {"out": gd.Guarded(4, torch.int32), "scratch": gd.Guarded(4 * N, torch.int32)}

    def call(inputs=None):
        s = inside if inputs is None else inputs["src"]
        _sum_kernel(s, written["out"].interior, written["scratch"].interior, fault)
        return {"out": written["out"].interior}

    def dirty():  # another "geometry" on the same scratch
        written["scratch"].interior[:N // 2] += 5

    return (gd.check_writes("sum_kernel", written, call, dirty=dirty),
            gd.check_reads("sum_kernel", {"src": src}, call, written))


def test_the_correct_stand_in_passes():
    writes, reads = _run(None)
    assert writes == [] and reads == []
    want = int((torch.arange(N) * 3 + 1).sum())
    out = gd.Guarded(4, torch.int32)
    _sum_kernel(torch.arange(N, dtype=torch.int32) * 3 + 1, out.interior, torch.empty(N, dtype=torch.int32))
    assert int(out.interior[0]) == want


def test_a_byte_written_before_the_interior_is_reported():
    writes, _ = _run("write_before")
    assert writes and all("wrote before buffer 'out'" in f and "first at -4" in f for f in writes), writes


def test_a_byte_written_after_the_interior_is_reported():
    writes, _ = _run("write_after")
    assert writes and all("wrote after buffer 'scratch'" in f and "first at +0" in f for f in writes), writes


def test_a_read_after_the_input_is_reported():
    writes, reads = _run("read_after")
    assert writes == []  # poisons of the written buffers cannot see it
    assert reads == ["sum_kernel: output 'out' depends on the bytes next to input 'src'"], reads


def test_scratch_that_is_never_cleared_is_reported():
    writes, reads = _run("stale_scratch")
    assert reads == []
    assert len(writes) == 4 and all("output 'out' depends on what its buffers held" in f for f in writes), writes
    assert [f.split("fill '")[1].rstrip("')") for f in writes] == list(gd.POISON_NAMES)


def test_the_guards_and_the_interior_are_what_the_rule_says():
    for nbytes, dtype in [(0, torch.uint8), (20, torch.int32), (48, torch.int64), (65536 + 8, torch.float32), (200000, torch.uint8)]:
        g = gd.Guarded(nbytes, dtype, seed=3)
        guard = (max(65536, nbytes) + 255) // 256 * 256
        assert guard <= g.front < guard + 256 and g.back >= guard
        assert g.interior.data_ptr() % 256 == 0 and g.interior.numel() * g.interior.element_size() == nbytes
        assert g.check() == ([], [])
        for part in (g.raw[:g.front], g.raw[g.front + nbytes:]):
            assert part.min() > 0 and part.max() < 255 and len(torch.unique(part[:4096])) > 100
        g.raw[g.front - 1] ^= 1
        g.raw[g.front + nbytes + 5] ^= 1
        assert g.check() == ([-1], [5])


def test_exact_placement_arithmetic():
    """exactly(A): a multiple of A and not of 2A, for every type that fits, through Guarded, like and surround; the guards keep
    their size and their pattern."""
    for a in (1, 2, 4, 8, 16, 64):
        assert gd.exactly(a) == {"align": 2 * a, "skew": a}
        for dtype in (torch.uint8, torch.int16, torch.int32, torch.int64):
            item = torch.empty(0, dtype=dtype).element_size()
            if a % item:
                continue
            for nbytes in (0, 8 * 5, 65536 + 8 * 3):
                g = gd.Guarded(nbytes, dtype, seed=a, **gd.exactly(a))
                p = g.addr
                assert p % a == 0 and p % (2 * a) == a, (a, dtype, p)
                assert p == g.raw.data_ptr() + g.front and (nbytes == 0 or g.interior.data_ptr() == p) and g.interior.numel() * item == nbytes
                guard = (max(65536, nbytes) + 2 * a - 1) // (2 * a) * (2 * a)
                assert guard <= g.front < guard + 2 * a and g.back >= guard
                assert g.check() == ([], [])
            t = torch.arange(21, dtype=dtype).reshape(3, 7)
            lk = gd.like(t, 1, **gd.exactly(a))
            sr = gd.surround(t, 2, **gd.exactly(a))
            assert lk.interior.shape == t.shape and lk.interior.dtype == dtype and lk.interior.data_ptr() % (2 * a) == a
            assert torch.equal(sr, t) and sr.is_contiguous() and sr.data_ptr() % (2 * a) == a
    for align, skew in [(256, 16), (256, 255), (32, 24), (2, 0)]:  # any residue, not only the shorthand's
        assert gd.Guarded(24, align=align, skew=skew).interior.data_ptr() % align == skew


def test_exact_placement_refuses_what_the_rule_excludes():
    for kw in ({"align": 16, "skew": 16}, {"align": 16, "skew": -1}):
        with pytest.raises(AssertionError):
            gd.Guarded(16, **kw)
    for dtype, a in [(torch.int32, 2), (torch.int32, 1), (torch.int64, 4), (torch.int16, 1)]:  # skew no multiple of the element
        with pytest.raises(AssertionError):
            gd.Guarded(16, dtype, **gd.exactly(a))
    gd.Guarded(16, torch.uint8, **gd.exactly(1))
    with pytest.raises(AssertionError):
        gd.exactly(3)


def test_guards_catch_one_byte_either_side_of_a_skewed_interior():
    for a in (1, 2, 4, 8, 16, 64):
        for nbytes in (8, 24, 65536 + 8):
            g = gd.Guarded(nbytes, seed=5, **gd.exactly(a))
            before, after = g.raw[g.front - 1].clone(), g.raw[g.front + nbytes].clone()
            g.raw[g.front - 1] ^= 1
            assert g.check() == ([-1], [])
            g.raw[g.front - 1] = before
            g.raw[g.front + nbytes] ^= 0x80
            assert g.check() == ([], [0])
            g.raw[g.front + nbytes] = after
            g.bytes.fill_(0xA5)  # the interior's own first and last byte are not guard
            assert g.check() == ([], [])
    src = torch.arange(N, dtype=torch.int32)
    inside = gd.surround(src, 0, **gd.exactly(4))
    for fault, words in [("write_before", "wrote before buffer 'out'"), ("write_after", "wrote after buffer 'scratch'"), (None, None)]:
        written = {"out": gd.Guarded(4, torch.int32, **gd.exactly(4)), "scratch": gd.Guarded(4 * N, torch.int32, **gd.exactly(8))}

        def call():
            _sum_kernel(inside, written["out"].interior, written["scratch"].interior, fault)
            return {"out": written["out"].interior}
        found = gd.check_writes("sum_kernel", written, call)
        assert (found == []) if fault is None else (found and all(words in f for f in found)), (fault, found)


def test_the_default_placement_is_what_it_was():
    """skew=0, align=256: the same front, back, interior and guard bytes as an allocation placed by the rule as first written."""
    for nbytes, dtype, seed in [(0, torch.uint8, 0), (20, torch.int32, 3), (65536 + 8, torch.float32, 1), (200000, torch.uint8, 9)]:
        g = gd.Guarded(nbytes, dtype, seed=seed)
        h = gd.Guarded(nbytes, dtype, seed=seed, align=256, skew=0)
        guard = (max(65536, nbytes) + 255) // 256 * 256
        for x in (g, h):
            assert x.raw.numel() == 2 * guard + nbytes + 256
            assert x.front == guard + (-(x.raw.data_ptr() + guard)) % 256
            assert x.back == x.raw.numel() - x.front - nbytes
            assert x.interior.data_ptr() % 256 == 0
            assert torch.equal(x.raw[:x.front], gd._pattern(x.front, 2 * seed + 1))
            assert torch.equal(x.raw[x.front + nbytes:], gd._pattern(x.back, 2 * seed + 2))
    t = torch.arange(12, dtype=torch.int16)
    assert gd.like(t).interior.data_ptr() % 256 == 0 and gd.surround(t, 1).data_ptr() % 256 == 0
    assert gd.like(t, 0, 64).interior.data_ptr() % 64 == 0 and gd.surround(t, 1, 64).data_ptr() % 64 == 0  # positional align


def test_a_pointer_torch_cannot_place():
    t = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    m = gd.placed(t, 3, 2)
    assert isinstance(m, gd.Misplaced) and m.data_ptr() % 4 == 2 and m.dtype == torch.int32 and m.shape == (2, 3) and m.numel() == 6
    assert m.is_contiguous() and len(m) == 2 and torch.equal(m[1], t[1]) and torch.equal(m.clone(), t)
    assert torch.equal(m.guarded.bytes, t.view(-1).view(torch.uint8)) and m.guarded.check() == ([], [])
    r = torch.as_tensor(m, dtype=torch.int32).reshape(-1).to("cpu").contiguous()  # what the bindings do to an argument
    assert isinstance(r, gd.Misplaced) and r.data_ptr() == m.data_ptr() and r.shape == (6,)
    assert not isinstance(m.clone(), gd.Misplaced) and m.clone().data_ptr() % 4 == 0  # other elements: an ordinary tensor
    o = gd.placed(torch.arange(4, dtype=torch.int64), 1, 4)
    assert isinstance(o, gd.Misplaced) and o.data_ptr() % 8 == 4
    s = gd.placed(t, 3, 4)
    assert isinstance(s, torch.Tensor) and s.data_ptr() % 8 == 4 and torch.equal(s, t)
    assert isinstance(gd.placed(torch.zeros(5, dtype=torch.uint8), 0, 1), torch.Tensor)


def test_poisons_and_surround():
    got = dict(gd.poisons(33, seed=4))
    assert list(got) == list(gd.POISON_NAMES) and got["dirty"] is None
    assert not got["zeros"].any() and (got["ones"] == 0xFF).all() and len(torch.unique(got["random"])) > 8
    assert torch.equal(got["random"], dict(gd.poisons(33, seed=4))["random"])
    t = torch.arange(35, dtype=torch.int16).reshape(5, 7)
    a, b = gd.surround(t, 1), gd.surround(t, 2)
    assert torch.equal(a, t) and torch.equal(b, t) and a.dtype == t.dtype and a.is_contiguous()
    assert not torch.equal(_ptr_view(a.view(-1), 35, 64), _ptr_view(b.view(-1), 35, 64))  # other neighbours
    assert not torch.equal(_ptr_view(a.view(-1), -64, 64), _ptr_view(b.view(-1), -64, 64))


def test_every_gpu_case_is_sized():
    """tests/test_gpu_guard_streams.py's (entry point, geometry) pairs: every *_workspace_bytes and *_max_bytes query gives a size, and the
    pairs it leaves out are refused (arithmetic only, no device)."""
    from tests import test_gpu_guard_streams as streams
    streams.check_every_pair_is_sized()
    assert len(streams.PAIRS) == 102 and len(streams.REFUSED) == 6
