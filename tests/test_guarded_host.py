"""tests/helpers/guarded.py catches what it claims to (no GPU): the stand-in "kernels" are plain torch functions on CPU tensors,
four of them faulty in the four ways the GPU tests look for, one correct.  Each faulty one must be reported with the buffer named."""
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
