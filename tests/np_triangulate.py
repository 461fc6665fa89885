"""Plain float64 reference of the two-view DLT triangulation (csrc/triangulate.hip: dlt_build + the smallest right singular
vector) and of the cheirality vote of recover_pose_kernel — NumPy only, LAPACK's SVD instead of the one-sided Jacobi sweeps
the kernels and the C oracle share, so a mistake common to those two does not pass here.

The bars the tests hold float32 results to are derived, not measured on the kernels:
  normalised (`v / v[3]` in float32): the kernel casts v[k] and v[3] to float32 (2^-24 relative each) and divides in float32
      (2^-24 relative): |got_k - ref_k| <= 3 * 2^-24 * |ref_k| to first order, asserted per point against max_k |ref_k|;
  raw unit vector: one cast of a number below 1 in magnitude: 2^-25 absolute, asserted at 2^-24 (sign-aligned: a singular
      vector's sign is the algorithm's choice).
test_tri_cases_cpu.py re-asserts on the committed inputs that the C oracle alone stays inside them."""
import numpy as np

U24 = 2.0 ** -24
BAR_NORMALISED = 3.0        # units of 2^-24 * max_k |ref_k|
BAR_RAW = 1.0               # units of 2^-24, absolute
DECIDABLE_EPS = 1e-9


def dlt_system(P1, P2, x1, x2, rows=4):
    """[n, rows, 4] float64: per view x P[2] - P[0], y P[2] - P[1] and, rows = 6, x P[1] - y P[0].  x1, x2: (n, 2)."""
    assert rows in (4, 6)
    per = rows // 2
    A = np.empty((len(x1), rows, 4))
    for v, (P, x) in enumerate(((P1, x1), (P2, x2))):
        P = np.asarray(P, np.float64).reshape(3, 4)
        x = np.asarray(x, np.float64).reshape(-1, 2)
        A[:, v * per + 0] = x[:, :1] * P[2] - P[0]
        A[:, v * per + 1] = x[:, 1:] * P[2] - P[1]
        if per == 3:
            A[:, v * per + 2] = x[:, :1] * P[1] - x[:, 1:] * P[0]
    return A


def triangulate(P1, P2, x1, x2, rows=4):
    """(unit [4, n], normalised [4, n], singular values [n, 4]) in float64; x1, x2: (n, 2) pixel coordinates."""
    if len(x1) == 0:
        return np.zeros((4, 0)), np.zeros((4, 0)), np.zeros((0, 4))
    _, s, vt = np.linalg.svd(dlt_system(P1, P2, x1, x2, rows))
    v = vt[:, 3, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return v.T.copy(), (v / v[:, 3:]).T.copy(), s


def normalised_error(got, ref_normalised):
    """Per point, in units of 2^-24 * max_k |ref_k|: max_k |got_k - ref_k|.  got: float32 [4, n]."""
    ref = np.asarray(ref_normalised, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref).max(0) / (U24 * np.abs(ref).max(0))


def raw_error(got, ref_unit):
    """Per point, in units of 2^-24 (absolute): max_k |s got_k - ref_k| with s the sign that aligns the two vectors."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref_unit, np.float64)
    s = np.where((got * ref).sum(0) < 0, -1.0, 1.0)
    return np.abs(s * got - ref).max(0) / U24


def cheirality(Ps, x1n, x2n, dist=50.0, rows=4, eps=DECIDABLE_EPS):
    """recover_pose_kernel's four tests on the float64 null vector Q of [I|0] / Ps[m]:
        Q2 Q3 > 0,   Q2 / Q3 < dist,   z > 0,   z < dist    with z = Ps[m][2] . (Q / Q3).
    Returns (mask bool [h, n], decidable bool [h, n]).  A point is decidable when none of Q2 Q3, dist - Q2 / Q3, z and
    dist - z is within eps of zero relative to its operands: |Q2 Q3| against |Q| = 1, a difference against the larger of its
    two terms, the sum z against the sum of the magnitudes of its four products.  (All four are invariant under Q -> -Q.)"""
    Ps = np.asarray(Ps, np.float64).reshape(-1, 3, 4)
    x1n, x2n = np.asarray(x1n, np.float64).reshape(-1, 2), np.asarray(x2n, np.float64).reshape(-1, 2)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    mask = np.zeros((len(Ps), len(x1n)), bool)
    dec = np.zeros_like(mask)
    if len(x1n) == 0:
        return mask, dec
    for m, P in enumerate(Ps):
        Q = triangulate(P0, P, x1n, x2n, rows)[0]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = Q / Q[3]
            terms = P[2][:, None] * q
            z = terms.sum(0)
            prod = Q[2] * Q[3]
            mask[m] = (prod > 0) & (q[2] < dist) & (z > 0) & (z < dist)
            d = np.abs(prod) > eps
            d &= np.abs(dist - q[2]) > eps * np.maximum(abs(dist), np.abs(q[2]))
            d &= np.abs(z) > eps * np.abs(terms).sum(0)
            d &= np.abs(dist - z) > eps * np.maximum(abs(dist), np.abs(z))
            d &= np.isfinite(q).all(0)
        dec[m] = d
    return mask, dec
