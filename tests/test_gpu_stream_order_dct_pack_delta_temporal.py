"""Stream order and host waits (tests/helpers/stream_order.py) for the entry points of include/svc_hip_temporal.h, periods 2 and 4: on a
non-blocking side stream behind a delay, with another well-formed case in the input buffers until device copies behind the delay put
the real one back, every output is bit for bit the null-stream result, the C function is handed the side stream's handle, and the call
returns before the delay ends.  The builders are those of tests/test_gpu_guard_dct_pack_delta_temporal.py.

tests/test_stream_order_host.py ties include/svc_hip.h to tests/test_gpu_stream_order.py's cases; it does not see this header, so the
census is restated for it in tests/test_dct_pack_delta_temporal_host.py against covered() below, and the proxy here takes the place of
each stream from the header's own declarations."""
import os

import pytest

from tests.helpers import stream_order as so
from tests.test_gpu_guard_dct_pack_delta_temporal import ENTRIES, GEOMS, N, fn_of
from tests.test_gpu_guard_streams import Pool, _gid

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svc_hip_temporal.h")

# id -> (the C function, its builder, the geometry)
CASES = {f"{entry}-{_gid(g)}": (fn_of(entry), build, g) for entry, (build, geoms) in ENTRIES.items() for g in GEOMS if g in geoms}


def covered():
    """The entry points the cases reach (tests/test_dct_pack_delta_temporal_host.py compares them with include/svc_hip_temporal.h)."""
    return {fn for fn, _, _ in CASES.values()}


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


@pytest.mark.parametrize("case", sorted(CASES))
def test_order_and_no_host_wait(native, monkeypatch, delay, case):
    proxy = _install(monkeypatch, native)
    findings = so.check_order(CASES[case][0], *_caller(case, 0), proxy=proxy, delay=delay)
    assert not findings, "\n".join(findings)
