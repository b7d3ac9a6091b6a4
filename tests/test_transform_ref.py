"""The long-double transform reference (tests/helpers/transform_ref.py) and its acceptance rule, checked without a GPU: the
reference against the oracle's float64 transform, against the coefficients that are rational, and against its own inverse; the
ambiguous shares and the tie / near-tie counts the GPU tests (tests/test_gpu_transform_exact.py) assume of their seeded inputs;
and that the rule tells an f64 transform from two that are not, which the 1e-4 parity bar accepts."""
import numpy as np
import pytest

from tests.helpers import transform_inputs as ti
from tests.helpers import transform_ref as tr

pytestmark = pytest.mark.skipif(not tr.available(), reason=tr.UNAVAILABLE)

LD = np.longdouble
SHAPES = [(8, 8), (16, 16), (6, 10), (2, 2), (64, 64), (8, 1), (1, 4)]


def _ref_slack(bw, bh):
    """The reference's own error bound: forward_slack with the long double's unit roundoff 2^-64 in place of 2^-53."""
    return tr.forward_slack(bw, bh) * LD(2) ** -11


def _frame(bw, bh, seed, tiles=(5, 4)):
    return np.random.default_rng(seed).integers(0, 256, (bh * tiles[1], bw * tiles[0], 3), dtype=np.uint8)


@pytest.mark.parametrize("bw,bh", SHAPES)
def test_reference_agrees_with_the_f64_oracle(oracle, bw, bh):
    bgr = _frame(bw, bh, 1)
    bgr[:bh, :bw] = 255
    ref = tr.dct_ref(bgr, bw, bh)
    d = np.abs(ref - oracle.dct_frame_f64(bgr, bw, bh).astype(LD)).max()
    a = tr.forward_slack(bw, bh)
    print(f"{bw}x{bh}: |ref - f64 oracle| max = {float(d):.3e} = {float(d / a):.3f} A")
    assert d <= a
    assert abs(ref[0, 0, 0] - LD(255) * np.sqrt(LD(bw * bh))) <= _ref_slack(bw, bh)


@pytest.mark.parametrize("n", [8, 16])
def test_rational_positions_are_exact(n):
    """At {0, N/2}^2 the 2-D basis is +-1/N: the coefficient is an integer sum over N, which long double holds exactly."""
    bgr = _frame(n, n, 2, tiles=(9, 7))
    ref = tr.dct_ref(bgr, n, n)
    for (v, u), m in tr.rational_positions(bgr, n).items():
        want = m.astype(LD) / LD(n)
        assert np.abs(ref[:, v::n, u::n] - want).max() <= _ref_slack(n, n), (v, u)
        lo, hi = tr.interval(ref[:, v::n, u::n], tr.forward_slack(n, n))
        nz = m != 0  # m / N is an f32: never ambiguous -- except an exact zero, whose interval is [-A, A]
        assert np.array_equal(lo[nz], hi[nz]) and np.array_equal(lo[nz], want.astype(np.float32)[nz])
        assert (lo[~nz] < 0).all() and (hi[~nz] > 0).all()


@pytest.mark.parametrize("bw,bh", SHAPES)
def test_inverse_of_forward_is_identity(bw, bh):
    """Both are orthonormal: the forward error (<= the reference's slack per coefficient) keeps its 2-norm through the inverse, so a
    pixel moves by at most sqrt(bw bh) of it, plus the inverse's own chains, which the same bound covers."""
    bgr = _frame(bw, bh, 3)
    back = tr.idct_ref(tr.dct_ref(bgr, bw, bh), bw, bh)
    assert np.abs(back - bgr.transpose(2, 0, 1).astype(LD)).max() <= (np.sqrt(LD(bw * bh)) + 1) * _ref_slack(bw, bh)


def test_inverse_slack_is_per_tile():
    q = np.zeros((3, 16, 16), np.float32)
    q[0, 0, 0], q[0, 9, 9], q[1, 3, 12] = 100.0, -7.0, 2.0
    a = tr.inverse_slack(q, 8, 8)
    k = 2 * 20 * 2.0 ** -53 * (2 / 8.0)
    assert np.allclose(a[0, :8, :8].astype(float), 100 * k) and np.allclose(a[0, 8:, 8:].astype(float), 7 * k)
    assert np.allclose(a[1, :8, 8:].astype(float), 2 * k) and a[2].max() == 0 and a[0, :8, 8:].max() == 0


def test_near_half():
    f = np.float32
    q = np.array([2.5, np.nextafter(f(2.5), f(3)), 2.5 + 5 * 2.0 ** -22, -1000.5, 0.5, 0.25], np.float64)
    assert tr.near_half(q).tolist() == [True, True, False, True, True, False]


@pytest.mark.parametrize("form", list(ti.COVERAGE))
def test_coverage_inputs_hold_what_the_gpu_tests_assume(oracle, form):
    """From the reference alone, for the seeds the GPU tests use: the caps on the ambiguous shares, and enough exact ties of each sign
    and non-exact near-ties of c / step among the unambiguous coefficients, for steps 1, 3 and 7."""
    frames, types, c = ti.coverage_case(form)
    bw, bh = c["block"]
    lo, hi = zip(*(tr.interval(tr.dct_ref(f, bw, bh), tr.forward_slack(bw, bh)) for f in frames))
    lo, hi = np.stack(lo), np.stack(hi)
    share = float((lo != hi).mean())
    print(f"{form} {bw}x{bh}: raw ambiguous share {share:.3e}")
    assert share <= tr.RAW_AMBIGUOUS_CAP
    total = {}
    for fg, bg in ti.COVERAGE_STEPS:
        qlo = np.stack([oracle.quant_frame(lo[f], *c["mv"], types[f], fg, bg) for f in range(c["n"])])
        qhi = np.stack([oracle.quant_frame(hi[f], *c["mv"], types[f], fg, bg) for f in range(c["n"])])
        steps = np.stack([ti.step_plane(types[f], c["w"], c["h"], c["mv"], fg, bg) for f in range(c["n"])])[:, None].repeat(3, 1)
        for s in {fg, bg}:
            ti.add_census(total, ti.tie_census(lo, hi, qlo, qhi, steps, s))
    for s, t in sorted(total.items()):
        print(f"  step {s}: {t}")
        assert t["ambiguous"] <= tr.QUANT_AMBIGUOUS_CAP * t["positions"]
        if s in (1, 3, 7):
            assert min(t["ties_pos"], t["ties_neg"], t["near_ties"]) >= 32, (s, t)


@pytest.mark.parametrize("block", [8, 16])
def test_placement_inputs_hit_the_work_split_edges(block):
    frames, special = ti.tuned_placement_frames(block)
    n, h, w, _ = frames.shape
    seg, wgs, per = ti.tuned_work_split(block, n, h, w)
    assert (w // 16) % per != 0 and (seg // n) % per != 0  # a workgroup straddles bands, and frames
    assert seg % per != 0 and wgs % 8 != 0                 # last workgroup partial; xcd_contiguous_block's uneven case
    assert special.any(axis=(1, 2)).all()                  # every frame carries special tiles
    lo, hi = zip(*(tr.interval(tr.dct_ref(f, block, block), tr.forward_slack(block, block)) for f in frames))
    rnd = ~np.stack([special] * 3, axis=1)
    assert float((np.stack(lo) != np.stack(hi))[rnd].mean()) <= tr.RAW_AMBIGUOUS_CAP


@pytest.mark.parametrize("bw,bh", ti.GENERAL_BLOCKS)
def test_general_inputs_end_in_a_narrow_strip(bw, bh):
    tx, _ = ti.GENERAL_TILES[(bw, bh)]
    w, sw = tx * bw, ti.general_strip(bw, bh, tx * bw)
    if (bw, bh) == (64, 64):
        assert sw == 64
    else:
        assert w > sw and w % sw != 0
    assert (bw, bh) != (8, 8) or w % 16 != 0  # or it would be the tuned kernel


# ---- the rule discriminates ----------------------------------------------------------------------------------------------------------

def _stand_in(bgr, bw, bh, tables32=False, column32=False):
    """A plain numpy transform: float64 throughout, or with basis tables rounded to f32, or with the whole column pass in f32."""
    cw, ch = tr.basis(bw).astype(np.float64), tr.basis(bh).astype(np.float64)
    if tables32:
        cw, ch = cw.astype(np.float32).astype(np.float64), ch.astype(np.float32).astype(np.float64)
    out = []
    for c in range(3):
        x = tr._tiles(bgr[..., c].astype(np.float64), bw, bh)
        rows = np.matmul(x, cw.T)
        if column32:
            y = np.einsum("vm,yxmu->yxvu", ch.astype(np.float32), rows.astype(np.float32), optimize=False)
        else:
            y = np.matmul(ch, rows)
        out.append(tr._untile(y.astype(np.float32)))
    return np.stack(out)


def _bar_1e4(got, ref):
    ref = ref.astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / (1e-4 * np.maximum(1.0, np.abs(ref)))).max())


@pytest.mark.parametrize("bw,bh", [(8, 8), (16, 16), (6, 10)])
def test_rule_discriminates(bw, bh):
    bgr = _frame(bw, bh, 4, tiles=(24, 16))
    ref = tr.dct_ref(bgr, bw, bh)
    lo, hi = tr.interval(ref, tr.forward_slack(bw, bh))
    honest = _stand_in(bgr, bw, bh)
    assert not tr.raw_violations(honest, lo, hi).any()  # plain f64 numpy lies inside [lo, hi] everywhere
    for kind in ("tables32", "column32"):
        got = _stand_in(bgr, bw, bh, **{kind: True})
        bad = int(tr.raw_violations(got, lo, hi).sum())
        bar = _bar_1e4(got, ref)
        print(f"{bw}x{bh} {kind}: {bad} of {got.size} outside [lo, hi]; worst error = {bar:.3f} of the 1e-4 bar")
        assert bad > 0  # the rule rejects it
        # ... and today's tolerance accepts it -- except a 16-term f32 column chain over row results of up to 4080, whose error
        # (1.17 of the bar on this input) the 1e-4 bar sees as well
        assert bar <= 1.0 or (bw, bh, kind) == (16, 16, "column32")
