"""No device: every declaration of include/svc_hip.h that takes a `void* stream` has a case in tests/test_gpu_stream_order.py or a line
in its EXEMPT table, and the pure logic of tests/helpers/stream_order.py -- the validity condition, the judging of the first call
behind a delay, the wording of the findings -- does what the GPU tests rely on.  A new entry point without a case fails here."""
import ctypes as C
import os

import pytest

from scalable_video_codec_amd import native as nat
from tests import test_gpu_stream_order as cases
from tests.helpers import stream_order as so

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svc_hip.h")


def _declared():
    with open(HEADER) as f:
        return so.header_stream_params(f.read())


def _named(names):
    return ", ".join(sorted(names)) or "none"


def test_every_stream_entry_point_of_the_header_has_a_case_or_an_exemption():
    declared = set(_declared())
    assert len(declared) > 50, "the header's declarations were not found"
    have = cases.covered() | set(cases.EXEMPT)
    assert declared == have, (f"declared with a `void* stream` and neither a case nor exempt: {_named(declared - have)}; "
                              f"a case or an exemption for no such declaration: {_named(have - declared)}")
    assert not cases.covered() & set(cases.EXEMPT), _named(cases.covered() & set(cases.EXEMPT))


def test_the_signatures_take_their_stream_where_the_header_declares_it():
    declared = _declared()
    bound = so.stream_entry_points(nat.SIGNATURES)
    assert set(declared) == set(bound), (f"in the header only: {_named(set(declared) - set(bound))}; "
                                         f"told from native.SIGNATURES only: {_named(set(bound) - set(declared))}")
    for name, (at, count) in declared.items():
        args = nat.SIGNATURES[name][1]
        assert len(args) == count and bound[name] == at and args[at] is C.c_void_p, name
        assert at == count - 1 or (name.endswith("_temporal_frames") and at == count - 2), name  # the temporal calls: the period is last


def test_the_tables_hold_what_the_header_says():
    assert set(cases.EXEMPT) == {"svc_hip_halo_shift"}
    assert set(cases.BLOCKING) == {"segment_frames_ex-22x18-100-clusters"} and set(cases.BLOCKING) <= set(cases.CASES)
    with open(HEADER) as f:
        assert "SYNCHRONOUS: it waits for `stream`" in f.read()  # the sentence the one blocking form rests on


def test_the_header_parser():
    text = """
    /* int svc_hip_in_a_comment(void* stream); */
    #define X 1  // int svc_hip_in_a_line_comment(void* stream);
    typedef struct s { uint32_t a; } s;
    int svc_hip_first(const float* d_x, uint32_t n,
                      void* stream);
    int svc_hip_period(const float* d_x, void *stream, uint32_t period);
    uint64_t svc_hip_bytes(uint32_t n);
    int svc_hip_host(const void* src, void* stream_like);
    """
    assert so.header_stream_params(text) == {"svc_hip_first": (2, 3), "svc_hip_period": (1, 3)}


def test_which_signature_takes_a_stream():
    vp, u32 = C.c_void_p, C.c_uint32
    assert so.signature_stream_index("svc_hip_x_frames", C.c_int, [vp, u32, vp]) == 2
    assert so.signature_stream_index("svc_hip_x_temporal_frames", C.c_int, [vp, vp, u32]) == 1
    assert so.signature_stream_index("svc_hip_x_frames", C.c_int, [vp, vp, u32]) is None
    assert so.signature_stream_index("svc_hip_x_host", C.c_int, [vp, vp]) is None
    assert so.signature_stream_index("svc_hip_comm_destroy", C.c_int, [vp]) is None
    assert so.signature_stream_index("svc_hip_x_bytes", C.c_uint64, [u32]) is None
    assert so.signature_stream_index("svc_hip_abi_version", C.c_int, []) is None


def test_the_validity_condition():
    assert so.MARGIN == 4.0 and so.START_DELAY_MS == 20.0
    assert so.valid(20.0, 5.0) and so.valid(20.0, 0.1)
    assert not so.valid(20.0, 5.01) and not so.valid(0.0, 0.001)


E, SIDE = "svc_hip_x_frames", 0x7F00


def _rec(name=E, stream=SIDE, before=False, after=False, t_before=0.001, t_after=0.002, peers=0):
    return so.Record(name, stream, before, after, t_before, t_after, peers)


def test_the_judging_of_the_first_call():
    judge = lambda rec, blocking=False, delay_ms=20.0: so.judge(E, rec, SIDE, blocking, delay_ms, 0.0)
    assert judge(_rec()) == []
    assert judge(None) == [so.f_no_call(E)]
    assert judge(_rec(name="svc_hip_other")) == [so.f_wrong_call(E, "svc_hip_other")]
    assert judge(_rec(stream=0)) == [so.f_stream(E, 0, SIDE)]
    assert judge(_rec(before=True, after=True)) == [so.f_void(E)]  # void: nothing else is said, and never a pass
    assert judge(_rec(after=True, t_after=0.021)) == [so.f_wait(E)]  # a call that waited is not also inconclusive
    assert judge(_rec(after=True, t_after=0.021), blocking=True) == []  # a blocking form: judged on the time up to the call
    assert judge(_rec(after=True, t_before=0.006, t_after=0.021), blocking=True) == [so.f_inconclusive(E, 20.0, 6.0)]
    assert judge(_rec(t_after=0.006)) == [so.f_inconclusive(E, 20.0, 6.0)]
    assert judge(_rec(t_after=0.005)) == []
    assert judge(_rec(stream=0, after=True)) == [so.f_stream(E, 0, SIDE), so.f_wait(E)]


def test_the_wording_names_the_entry_point_and_the_finding():
    said = {"(a)": so.f_output(E, "planes"), "(b)": so.f_stream(E, 0, SIDE), "(c)": so.f_void(E), "(d)": so.f_wait(E)}
    for letter, sentence in said.items():
        assert sentence.startswith(f"{E}: {letter} "), sentence
    assert "'planes'" in said["(a)"] and "0x7f00" in said["(b)"] and "void" in said["(c)"] and "waited on the host" in said["(d)"]
    for sentence in (so.f_same(E), so.f_blind(E)):
        assert sentence.startswith(f"{E}: the case is blind: "), sentence
    for sentence in (so.f_inconclusive(E, 20.0, 6.0), so.f_apart(E)):
        assert sentence.startswith(f"{E}: inconclusive: "), sentence
    assert "20.00 ms" in so.f_inconclusive(E, 20.0, 6.0) and "6.00 ms" in so.f_inconclusive(E, 20.0, 6.0)
    assert so.f_raised(E, ValueError("boom")).startswith(f"{E}: (a) ") and "ValueError: boom" in so.f_raised(E, ValueError("boom"))


class _Lib:
    def __init__(self):
        self.calls = []

    def svc_hip_x_frames(self, a, stream):
        self.calls.append(("x", a, stream))
        return 0

    def svc_hip_y_frames(self, stream, period):
        self.calls.append(("y", stream, period))
        return 0

    def svc_hip_bytes(self, n):
        return 16 * n


def test_the_proxy_records_only_the_first_call_behind_a_delay():
    lib = _Lib()
    states = iter([False, True])
    fake = lambda a, stream: 7
    proxy = so.Proxy(lib, {"svc_hip_x_frames": 1, "svc_hip_y_frames": 0}, {"svc_hip_fake": (fake, 1)})
    assert proxy.svc_hip_bytes(3) == 48 and proxy.svc_hip_x_frames(1, 5) == 0  # not armed: forwarded, nothing recorded
    judged = []
    watch = so.Watch(lambda: next(states), lambda: judged.append(1))
    proxy.new_group()
    proxy.arm(watch)
    assert proxy.svc_hip_y_frames(None, 2) == 0  # a null stream pointer reads as 0
    assert watch.record.name == "svc_hip_y_frames" and watch.record.stream == 0
    assert (watch.record.done_before, watch.record.done_after) == (False, True) and watch.record.t_before <= watch.record.t_after
    assert judged == [1]
    assert proxy.svc_hip_x_frames(1, SIDE) == 0 and proxy.svc_hip_fake(1, SIDE) == 7  # later calls: forwarded, named, not judged
    assert watch.record.name == "svc_hip_y_frames" and watch.later == ["svc_hip_x_frames", "svc_hip_fake"] and judged == [1]
    proxy.disarm()
    assert proxy.svc_hip_x_frames(2, 6) == 0 and watch.later == ["svc_hip_x_frames", "svc_hip_fake"]
    assert lib.calls == [("x", 1, 5), ("y", None, 2), ("x", 1, SIDE), ("x", 2, 6)]
    with pytest.raises(AttributeError):
        proxy.svc_hip_missing


def test_the_proxy_counts_the_peers_whose_delay_has_ended():
    proxy = so.Proxy(_Lib(), {"svc_hip_x_frames": 1})
    proxy.new_group()
    early, late = so.Watch(lambda: True), so.Watch(lambda: False)
    proxy.arm(early)
    proxy.disarm()
    proxy.arm(late)
    proxy.svc_hip_x_frames(0, SIDE)
    assert late.record.peers_done == 1 and late.record.stream == SIDE
