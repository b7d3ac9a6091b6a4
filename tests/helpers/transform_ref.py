"""An independent reference for the transform kernels, in long double (64-bit mantissa), and the acceptance rule built on it.

The kernels accumulate in float64 and round once to f32 (csrc/dct.hip, csrc/idct_core.hpp).  Against a reference that is ~2^11
times more precise than f64, such a kernel may differ from the correctly rounded f32 value only where the exact value lies
within the f64 accumulation error A of an f32 rounding boundary.  So:

  lo = RN32(ref - A), hi = RN32(ref + A)
  raw output        lo <= got <= hi
  quantised output  got == quant(lo, s) or got == quant(hi, s)       (numerically: -0.0 == +0.0)

Where lo == hi that is equality with the correctly rounded value; where they differ the position is AMBIGUOUS, and the share
of ambiguous positions is capped by the tests from the reference alone (RAW_AMBIGUOUS_CAP, QUANT_AMBIGUOUS_CAP).

A is derived, not tuned:
  forward   A(bw, bh) = 2 * (bw + bh + 4) * 2^-53 * 510 * sqrt(bw * bh)
            510 * sqrt(bw * bh) bounds sum |Ch| |X| |Cw| for bytes (|X| <= 255, row sums of |C| <= sqrt(2 N)); (bw + bh + 4) * 2^-53
            is the usual bound for the two FMA chains plus the roundings around them; the factor 2 covers basis entries a few
            f64 ulps off (the generated tables and cospi both are).
  inverse   A'(tile) = 2 * (bw + bh + 4) * 2^-53 * (2 / sqrt(bw * bh)) * sum |q| over the tile's requantised coefficients
            (|Ch[k][n] Cw[l][m]| <= 2 / sqrt(bw * bh)).
The reference's own error is about 2^-11 of that and is ignored.
"""
import numpy as np

LD = np.longdouble
F32 = np.float32
RAW_AMBIGUOUS_CAP = 1e-2
QUANT_AMBIGUOUS_CAP = 1e-5
_PI = "3.14159265358979323846264338327950288419716939937510"


def available() -> bool:
    return np.finfo(LD).nmant >= 63


UNAVAILABLE = "np.longdouble has fewer than 63 mantissa bits here: no reference more precise than float64"


def basis(n: int) -> np.ndarray:
    """C[k][i] = s_k cos(pi (2 i + 1) k / 2 n), s_0 = sqrt(1/n), s_k = sqrt(2/n), in long double.  (2 i + 1) k is reduced mod 4 n
    in integers and folded into [0, n] quarter-turn units, so cosl sees an angle in [0, pi/2]."""
    k = np.arange(n, dtype=np.int64)[:, None]
    i = np.arange(n, dtype=np.int64)[None, :]
    j = ((2 * i + 1) * k) % (4 * n)        # angle = pi j / (2 n), j in [0, 4n)
    j = np.where(j > 2 * n, 4 * n - j, j)  # cos(2 pi - a) = cos a: j in [0, 2n]
    neg = j > n
    j = np.where(neg, 2 * n - j, j)        # cos(pi - a) = -cos a: j in [0, n]
    c = np.cos(LD(_PI) * j.astype(LD) / LD(2 * n))
    c = np.where(j == n, LD(0), c)         # cos(pi/2) exactly
    c = np.where(neg, -c, c)
    s = np.where(k == 0, np.sqrt(LD(1) / LD(n)), np.sqrt(LD(2) / LD(n)))
    return (s * c).astype(LD)


def _tiles(plane: np.ndarray, bw: int, bh: int) -> np.ndarray:
    h, w = plane.shape
    assert h % bh == 0 and w % bw == 0, (h, w, bw, bh)
    return plane.reshape(h // bh, bh, w // bw, bw).transpose(0, 2, 1, 3)  # [ty][tx][bh][bw]


def _untile(t: np.ndarray) -> np.ndarray:
    ty, tx, bh, bw = t.shape
    return t.transpose(0, 2, 1, 3).reshape(ty * bh, tx * bw)


def dct_planes_ref(planes, bw: int, bh: int) -> np.ndarray:
    """Y = Ch X Cw^T per bw x bh tile of each plane of (planes, H, W), long double."""
    cw, ch = basis(bw), basis(bh)
    out = []
    for p in np.asarray(planes):
        x = _tiles(p.astype(LD), bw, bh)
        out.append(_untile(np.matmul(np.matmul(ch, x), cw.T)))
    return np.stack(out)


def dct_ref(bgr, bw: int, bh: int) -> np.ndarray:
    """Orthonormal DCT-II per tile and plane of a (H, W, 3) byte frame -> (3, H, W) long double, planes in B, G, R order."""
    bgr = np.asarray(bgr)
    assert bgr.ndim == 3 and bgr.shape[2] == 3
    return dct_planes_ref(bgr.transpose(2, 0, 1), bw, bh)


def idct_ref(coeffs_f32, bw: int, bh: int) -> np.ndarray:
    """X = Ch^T Y Cw per tile of (3, H, W) coefficient planes -> (3, H, W) long double."""
    cw, ch = basis(bw), basis(bh)
    out = []
    for p in np.asarray(coeffs_f32):
        y = _tiles(p.astype(LD), bw, bh)
        out.append(_untile(np.matmul(np.matmul(ch.T, y), cw)))
    return np.stack(out)


def forward_slack(bw: int, bh: int):
    return LD(2 * (bw + bh + 4)) * LD(2) ** -53 * LD(510) * np.sqrt(LD(bw * bh))


def inverse_slack(q_f32, bw: int, bh: int) -> np.ndarray:
    """A' per position of (3, H, W) requantised coefficient planes (constant over each tile)."""
    k = LD(2 * (bw + bh + 4)) * LD(2) ** -53 * (LD(2) / np.sqrt(LD(bw * bh)))
    out = []
    for p in np.asarray(q_f32):
        t = _tiles(np.abs(p.astype(LD)), bw, bh)
        s = t.sum(axis=(2, 3), keepdims=True) * k
        out.append(_untile(np.broadcast_to(s, t.shape)))
    return np.stack(out)


def interval(ref: np.ndarray, slack):
    """(lo, hi) = (RN32(ref - A), RN32(ref + A)); the long double -> f32 conversion rounds once, to nearest even."""
    return (ref - slack).astype(F32), (ref + slack).astype(F32)


def raw_violations(got, lo, hi) -> np.ndarray:
    """Boolean mask of the positions where lo <= got <= hi does NOT hold (NaN violates)."""
    got = np.asarray(got, F32)
    return ~((lo <= got) & (got <= hi))


def quant_violations(got, qlo, qhi) -> np.ndarray:
    """Boolean mask of the positions where got is neither quant(lo) nor quant(hi) (numeric comparison: -0.0 == +0.0)."""
    got = np.asarray(got, F32)
    return ~((got == qlo) | (got == qhi))


def near_half(q64: np.ndarray, ulps: float = 4.0) -> np.ndarray:
    """Is q (float64 image of an f32 quotient) within `ulps` f32 ulps of some k + 1/2 ?"""
    q = np.abs(np.asarray(q64, np.float64))
    d = np.abs(q - (np.floor(q) + 0.5))
    ulp = np.spacing(np.maximum(q, 0.5).astype(F32)).astype(np.float64)
    return d <= ulps * ulp


def rational_positions(bgr, n: int):
    """N x N tiles, N in {8, 16}: the coefficients at {0, N/2}^2 are sum(+-x) / N exactly.  -> {(v, u): the integer numerators
    as (3, H/N, W/N) int64}."""
    bgr = np.asarray(bgr).astype(np.int64)
    h, w, _ = bgr.shape
    x = bgr.transpose(2, 0, 1).reshape(3, h // n, n, w // n, n)
    # row k = N/2 of the basis: sqrt(2/N) cos(pi (2 i + 1) / 4) = sqrt(1/N) * (+1, -1, -1, +1, ...)
    sgn = np.array([1 if ((2 * i + 1) % 8) in (1, 7) else -1 for i in range(n)], np.int64)
    one = np.ones(n, np.int64)
    m = {}
    for v, sv in ((0, one), (n // 2, sgn)):
        for u, su in ((0, one), (n // 2, sgn)):
            m[(v, u)] = np.einsum("cyvxu,v,u->cyx", x, sv, su)
    return m
