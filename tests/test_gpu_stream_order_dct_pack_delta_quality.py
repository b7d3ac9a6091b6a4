"""Stream order and host waits (tests/helpers/stream_order.py) for svc_hip_dct_pack_delta_quality_frames
(include/svc_hip_delta_quality.h), with the key flags, the cap and both tables and without any of them: on a non-blocking side stream
behind a delay, with another well-formed case in the input buffers until device copies behind the delay put the real one back, every
output is bit for bit the null-stream result, the C function is handed the side stream's handle, and the call returns before the delay
ends.  The builders are those of tests/test_gpu_guard_dct_pack_delta_quality.py.

tests/test_stream_order_host.py ties include/svc_hip.h to tests/test_gpu_stream_order.py's cases; it does not see this header, so the
census is restated for it below (without a device), and the proxy here takes the place of each stream from the header's own
declarations."""
import ctypes as C
import os

import pytest

from scalable_video_codec_amd import native as nat
from tests.helpers import stream_order as so
from tests.test_gpu_guard_dct_pack_delta_quality import ENTRIES, ENTRY, GEOMS, N
from tests.test_gpu_guard_streams import Pool, _gid

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svc_hip_delta_quality.h")
FN = f"svc_hip_{ENTRY}_frames"

# id -> (the C function, its builder, the geometry)
CASES = {f"{entry}-{_gid(g)}": (FN, build, g) for entry, (build, _) in ENTRIES.items() for g in GEOMS}


def test_every_stream_declaration_of_the_header_is_bound_and_has_a_case():
    """The census of tests/test_stream_order_host.py for this header: declared with a `void* stream` == bound with a stream == reached
    by a case here; the signature takes its stream where the header declares it, last."""
    with open(HEADER) as f:
        declared = so.header_stream_params(f.read())
    assert set(declared) == {FN} == {fn for fn, _, _ in CASES.values()}
    at, count = declared[FN]
    res, args = nat.SIGNATURES_DELTA_QUALITY[FN]
    assert res is C.c_int and len(args) == count and args[at] is C.c_void_p and at == count - 1
    assert so.stream_entry_points(nat.SIGNATURES_DELTA_QUALITY) == {FN: at}
    assert set(nat.SIGNATURES_DELTA_QUALITY) - set(declared) == {f"svc_hip_{ENTRY}_workspace_bytes"}  # the query has no stream
    assert len(CASES) == 4  # with and without the flags, the cap and the tables, on both tile sizes


def _install(monkeypatch, native):
    with open(HEADER) as f:
        index = {name: at for name, (at, _) in so.header_stream_params(f.read()).items()}
    proxy = so.Proxy(native.load(), index)
    monkeypatch.setattr(native, "_lib", proxy)
    return proxy


def _caller(case, seed):
    """-> (inputs, the same case built with the other seed, call, the buffers it writes)."""
    _, build, geom = CASES[case]
    pool = Pool()
    inputs, call = build(pool, geom, N, seed)
    stale, _ = build(Pool(), geom, N, 1 - seed)
    return inputs, stale, call, pool.written


@pytest.fixture(scope="module")
def delay(native):
    return so.Delay()


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_order_and_no_host_wait(native, monkeypatch, delay, case):
    proxy = _install(monkeypatch, native)
    findings = so.check_order(CASES[case][0], *_caller(case, 0), proxy=proxy, delay=delay)
    assert not findings, "\n".join(findings)
