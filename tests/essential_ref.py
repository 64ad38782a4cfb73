"""CPU restatement of the relative-pose stage of Tracker::initial_pose_estimate: pose::estimate_pose and
pose::estimate_pose_with_known_rotation (reference src/PoseEstimation.cpp:23-88 and :110-227, called at
src/Tracker.cpp:162 and src/Initialization.cpp:153).  numpy, f64 unless stated.  Test infrastructure only; the product
package never imports it.  csrc/pose.hip follows this file operation by operation.

The reference calls cv::findEssentialMat(USAC_ACCURATE, 0.99, 1.0 px).  USAC's samplers, SPRT and GC-RANSAC local
optimisation cannot be restated bit for bit, so this file is the project's own specification.  Where it departs
from OpenCV:

  normalise   x = (u - cx) / fx, y = (v - cy) / fy (f64 of the f32 pixels).  t = threshold_px / ((fx + fy) / 2); a
              point is an inlier iff its squared Sampson distance is < t^2 (strict).  A point with a non-finite
              coordinate is never sampled and never an inlier.
  sampling    a counter-based hash: index k of hypothesis h is draw(seed, h, j) for the j-th draw, j = 0, 1, ...;
              a draw that repeats an earlier index of the sample or hits a non-finite point is discarded; a sample
              with fewer than 5 indices after MAX_DRAWS draws yields no model.
  solver      Nister's five-point method: the 5 x 9 system's null space by Gauss-Jordan with partial pivoting, the
              10 x 20 cubic constraints (det E = 0, 2 E E^T E - tr(E E^T) E = 0) in Nister's monomial order,
              Gauss-Jordan again, the 3 x 3 matrix B(z) and its degree-10 determinant; the real roots
              isolated by the roots of its derivatives and found by bisection of 64-bit keys (real_roots), then
              NEWTON_STEPS guarded Newton steps; x, y from the largest cross product of two rows of B(z).  Up to 10
              models per sample, each of unit Frobenius norm; a model whose max |2 E E^T E - tr(E E^T) E| exceeds
              ESS_EPS is dropped (an ill-conditioned elimination, e.g. a near-pure rotation).
              A rank-deficient sample (a pivot <= PIVOT_EPS * max |entry|) or a polynomial with no real roots yields
              0 models.
  score       the integer inlier count.  The best model has the highest count, ties to the lowest index
              10 h + m (a packed 64-bit maximum of (count, ~index) on the device).
  stopping    hypotheses in rounds of 256 up to max_hypotheses; after a round, stop once the number drawn is
              >= log(1 - confidence) / log(1 - w^5), w = best count / n.
  LO          up to 4 rounds: the linear 8-point fit on the current inliers (the smallest eigenvector of the 9 x 9
              normal matrix, summed in the kernel's fixed order, cyclic Jacobi), projected to singular values (1, 1, 0), re-scored; a refit is kept while
              its count does not drop.  No nonlinear polish.
  recover     recover_pose_from_essential as the reference runs it: decomposeEssentialMat (E = U S V^T by a one-sided
              Jacobi SVD; U, V^T negated when their determinant is negative; R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2])
              and the candidates (R1, t), (R1, -t), (R2, t), (R2, -t) cast to f32; triangulate_points(every finite
              match, I, candidate, K, 0.9999, 2.0) per candidate, the first strict maximum wins.
  edges       fewer than 5 points, or a best count below 5: identity pose, no inliers, status STATUS_FAILED.

estimate_pose_known_rotation is an f32 restatement of the reference loop; the only departures are the rays
((u - cx) / fx, (v - cy) / fy, 1) in f32 (the reference multiplies by Eigen's inverse of K) and the refit, which takes
the smallest eigenvector of the f64 normal matrix of the inlier constraints (3 x 3 cyclic Jacobi) where the reference
runs Eigen's JacobiSVD on the stack.  The 200 (i, j) pairs are an input.
"""
import math

import numpy as np

MAX_DRAWS = 64
PIVOT_EPS = 1e-12
TRIM_EPS = 1e-30            # a leading coefficient below TRIM_EPS * max |coefficient| is dropped
BISECT_ITERS = 64           # halvings of 64-bit keys: any f64 interval closes to two adjacent doubles
NEWTON_STEPS = 3
ESS_EPS = 1e-6              # a unit-norm model is kept only if max |2 E E^T E - tr(E E^T) E| <= ESS_EPS
ROUND = 256
LO_ROUNDS = 4
JACOBI_SWEEPS = 16
JACOBI_TOL = 1e-30          # a Jacobi sweep starts only while sum(off-diagonal^2) > JACOBI_TOL * sum(diagonal^2)
THREADS = 256               # pose_final's workgroup: the reduction order of the LO normal matrix
STATUS_OK, STATUS_FEW_POINTS, STATUS_FAILED = 0, 1, 2

M64 = (1 << 64) - 1
I64_MIN = np.int64(-(1 << 63))

# ------------------------------------------------------------------------------------------------ monomials
B1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                                   # x, y, z, 1
B2 = [(2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
B3 = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
      (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return tuple(i + j for i, j in zip(a, b))


T11 = [[B2.index(_add(a, b)) for b in B1] for a in B1]        # deg1 x deg1 -> deg2 (csrc/pose.hip: POSE_T11)
T21 = [[B3.index(_add(a, b)) for b in B1] for a in B2]        # deg2 x deg1 -> deg3 (POSE_T21)


# ------------------------------------------------------------------------------------------------ sampling
def splitmix64(x):
    x = (int(x) + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, h, j, n):
    """Index of draw j of hypothesis h: splitmix64(splitmix64(seed) + (h << 16 | j)), then the high 32 bits times n,
    shifted right by 32 (a multiply-shift map to [0, n))."""
    u = splitmix64((splitmix64(int(seed) & M64) + ((int(h) << 16) | int(j))) & M64)
    return ((u >> 32) * int(n)) >> 32


def sample(seed, h, n, finite, size=5):
    """The `size` indices of hypothesis h (draw order), or None."""
    out = []
    for j in range(MAX_DRAWS):
        i = draw(seed, h, j, n)
        if finite[i] and i not in out:
            out.append(i)
            if len(out) == size:
                return out
    return None


# ------------------------------------------------------------------------------------------------ geometry helpers
def normalise(pix, K):
    fx, fy, cx, cy = (float(k) for k in K)
    p = np.asarray(pix, np.float32).astype(np.float64)
    return (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy


def sampson(E, x1, y1, x2, y2):
    """Squared Sampson distance, in this order of operations (no fused multiply-add).  E [..., 9] row-major."""
    E = np.asarray(E, np.float64)
    e = [E[..., k][..., None] for k in range(9)]
    ex0 = (e[0] * x1 + e[1] * y1) + e[2]
    ex1 = (e[3] * x1 + e[4] * y1) + e[5]
    ex2 = (e[6] * x1 + e[7] * y1) + e[8]
    et0 = (e[0] * x2 + e[3] * y2) + e[6]
    et1 = (e[1] * x2 + e[4] * y2) + e[7]
    num = (x2 * ex0 + y2 * ex1) + ex2
    den = ((ex0 * ex0 + ex1 * ex1) + et0 * et0) + et1 * et1
    with np.errstate(divide="ignore", invalid="ignore"):
        return num * num / den


def needed_hypotheses(best_count, n, confidence, size=5):
    """log(1 - confidence) / log(1 - w^size), w = best_count / n; inf when w^size underflows to a no-op.  The power is
    formed by repeated left multiplication, (w * w) * w ..."""
    if n <= 0 or best_count <= 0:
        return math.inf
    w = best_count / n
    ws = w
    for _ in range(size - 1):
        ws = ws * w
    if ws >= 1.0:
        return 0.0
    d = math.log(1.0 - ws)
    if not d < 0.0:
        return math.inf
    return math.log(1.0 - confidence) / d


# ------------------------------------------------------------------------------------------------ five-point
def _gauss_jordan(A, ncols_pivot):
    """Vectorised over samples: A [S][r][c]; pivots columns 0 .. ncols_pivot-1.  Returns (A, bad [S])."""
    A = A.copy()
    S, R, _ = A.shape
    mmax = np.abs(A).reshape(S, -1).max(axis=1)
    bad = ~np.isfinite(mmax) | (mmax == 0)
    ar = np.arange(S)
    for c in range(ncols_pivot):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        rc, rp = A[ar, c].copy(), A[ar, p].copy()
        A[ar, c], A[ar, p] = rp, rc
        piv = A[:, c, c].copy()
        bad |= ~(np.abs(piv) > PIVOT_EPS * mmax)
        piv = np.where(bad, 1.0, piv)
        A[:, c, :] = A[:, c, :] / piv[:, None]
        for r in range(R):
            if r != c:
                f = A[:, r, c].copy()
                A[:, r, :] = A[:, r, :] - f[:, None] * A[:, c, :]
    return A, bad


def _mul(a, b, T, nout):
    out = np.zeros(a.shape[:-1] + (nout,))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., T[i][j]] = out[..., T[i][j]] + a[..., i] * b[..., j]
    return out


def _pmul(a, b):
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] = out[..., i + j] + a[..., i] * b[..., j]
    return out


def null_basis(x1, y1, x2, y2):
    """[S][4][9]: the null space of each 5 x 9 system, rows X, Y, Z, W (E = x X + y Y + z Z + W), and bad [S]."""
    Q = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)     # [S][5][9]
    M, bad = _gauss_jordan(Q, 5)
    S = len(M)
    N = np.zeros((S, 4, 9))
    for j in range(4):
        N[:, j, 5 + j] = 1.0
        for i in range(5):
            N[:, j, i] = -M[:, i, 5 + j]
    for j in range(4):                               # modified Gram-Schmidt, in order: an orthonormal basis
        for i in range(j):
            d = np.zeros(S)
            for k in range(9):
                d = d + N[:, i, k] * N[:, j, k]
            N[:, j, :] = N[:, j, :] - d[:, None] * N[:, i, :]
        nn = np.zeros(S)
        for k in range(9):
            nn = nn + N[:, j, k] * N[:, j, k]
        N[:, j, :] = N[:, j, :] / np.sqrt(nn)[:, None]
    return N, bad


def constraint_matrix(N):
    """[S][10][20]: det E and the nine entries of 2 E E^T E - tr(E E^T) E in the monomials B3."""
    E = [np.stack([N[:, 0, e], N[:, 1, e], N[:, 2, e], N[:, 3, e]], -1) for e in range(9)]      # deg-1 polys
    m11 = lambda a, b: _mul(a, b, T11, 10)           # noqa: E731
    m21 = lambda a, b: _mul(a, b, T21, 20)           # noqa: E731
    c0 = m11(E[4], E[8]) - m11(E[5], E[7])
    c1 = m11(E[3], E[8]) - m11(E[5], E[6])
    c2 = m11(E[3], E[7]) - m11(E[4], E[6])
    rows = [(m21(c0, E[0]) - m21(c1, E[1])) + m21(c2, E[2])]
    EE = {}
    for i in range(3):
        for j in range(i, 3):
            EE[i, j] = EE[j, i] = (m11(E[3 * i], E[3 * j]) + m11(E[3 * i + 1], E[3 * j + 1])) + m11(E[3 * i + 2], E[3 * j + 2])
    tr = (EE[0, 0] + EE[1, 1]) + EE[2, 2]
    for i in range(3):
        for j in range(3):
            s = (m21(EE[i, 0], E[j]) + m21(EE[i, 1], E[3 + j])) + m21(EE[i, 2], E[6 + j])
            rows.append(s * 2.0 - m21(tr, E[3 * i + j]))
    return np.stack(rows, 1)


def b_matrix(A):
    """Rows (4, 5), (6, 7), (8, 9) of the reduced system -> B(z) [S][3] as (bx [4], by [4], b1 [5]) ascending in z."""
    R = A[:, :, 10:]
    bx, by, b1 = [], [], []
    for a, b in ((4, 5), (6, 7), (8, 9)):
        ra, rb = R[:, a], R[:, b]
        bx.append(np.stack([ra[:, 2], ra[:, 1] - rb[:, 2], ra[:, 0] - rb[:, 1], -rb[:, 0]], -1))
        by.append(np.stack([ra[:, 5], ra[:, 4] - rb[:, 5], ra[:, 3] - rb[:, 4], -rb[:, 3]], -1))
        b1.append(np.stack([ra[:, 9], ra[:, 8] - rb[:, 9], ra[:, 7] - rb[:, 8], ra[:, 6] - rb[:, 7], -rb[:, 6]], -1))
    return bx, by, b1


def det_poly(bx, by, b1):
    """det B(z), 11 coefficients ascending."""
    c0 = _pmul(by[1], b1[2]) - _pmul(b1[1], by[2])
    c1 = _pmul(bx[1], b1[2]) - _pmul(b1[1], bx[2])
    c2 = _pmul(bx[1], by[2]) - _pmul(by[1], bx[2])
    return (_pmul(bx[0], c0) - _pmul(by[0], c1)) + _pmul(b1[0], c2)


def _key(x):
    """f64 -> int64 keys in the order of the values (+0 and -0 both 0): halving an interval of keys halves the number
    of doubles in it, whatever their magnitude."""
    i = np.asarray(x, np.float64).view(np.int64)
    return np.where(i < 0, I64_MIN - i, i)


def _unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, I64_MIN - k, k).view(np.float64)


def _horner(c, x):
    """c [..., 11] coefficients ascending, x [...]; top-down Horner over all 11 (zero padding is exact)."""
    v = np.zeros(np.shape(x))
    for k in range(10, -1, -1):
        v = v * x + c[..., k]
    return v


def real_roots(polys):
    """polys [S][11] -> roots [S][10] (ascending, NaN-padded), count [S].

    p is scaled by its largest |coefficient|; leading coefficients below TRIM_EPS are dropped (roots beyond ~1 / TRIM_EPS)
    and B = 1 + max |p_k / p_d| bounds every real root of p and of its derivatives (Gauss-Lucas).  The roots of the
    derivatives isolate those of p: level j = 1 .. d takes D = p^(d - j), of degree j; the roots of the level below
    (ascending) and -B, B cut [-B, B] into intervals on which D is monotonic, and an interval whose left end has a
    non-zero sign and whose right end has another sign (or zero) holds exactly one root.  It is found by BISECT_ITERS
    halvings of the interval's ordered-integer keys (the right end: the first double whose sign differs from the left
    end's).  The roots of p then take NEWTON_STEPS guarded Newton steps."""
    polys = np.asarray(polys, np.float64)
    S = len(polys)
    m = np.abs(polys).max(axis=1)
    good = (m > 0.0) & np.isfinite(m)
    p = polys / np.where(good, m, 1.0)[:, None]
    p[~good] = 0.0
    d = np.full(S, 10)
    for _ in range(10):
        trim = (d > 0) & (np.abs(p[np.arange(S), d]) < TRIM_EPS)
        d = np.where(trim, d - 1, d)
    p[np.arange(11)[None, :] > d[:, None]] = 0.0
    d[~good] = 0
    bound = np.zeros(S)
    for s in range(S):
        if d[s] > 0:
            bound[s] = 1.0 + np.abs(p[s, :d[s]] / p[s, d[s]]).max()
    D = np.zeros((S, 11, 11))                        # D[s, r] = the r-th derivative of p, ascending
    D[:, 0] = p
    for r in range(10):
        for k in range(10):
            D[:, r + 1, k] = float(k + 1) * D[:, r, k + 1]
    roots = np.full((S, 10), np.nan)
    nroot = np.zeros(S, np.int64)
    ar = np.arange(S)
    icol = np.arange(10)[None, :]
    for j in range(1, 11):
        act = d >= j
        q = D[ar, np.maximum(d - j, 0)]                                          # [S][11]
        ends = np.full((S, 11), np.nan)
        ends[:, 0] = -bound
        ends[:, 1:] = roots
        ends[ar, nroot + 1] = bound
        a, b = ends[:, :10], ends[:, 1:]
        live = act[:, None] & (icol <= nroot[:, None])
        a, b = np.where(live, a, 0.0), np.where(live, b, 0.0)
        qb = q[:, None, :]
        sa, sb = np.sign(_horner(qb, a)), np.sign(_horner(qb, b))
        has = live & (sa != 0) & (sb != sa)
        lo, hi = _key(a), _key(b)
        for _ in range(BISECT_ITERS):
            mid = ((lo >> 1) + (hi >> 1)) + (lo & hi & 1)
            same = np.sign(_horner(qb, _unkey(mid))) == sa
            lo = np.where(same, mid, lo)
            hi = np.where(same, hi, mid)
        z = np.where(has, _unkey(hi), np.nan)
        order = np.argsort(~has, axis=1, kind="stable")
        nz = np.take_along_axis(z, order, 1)
        nz[icol >= has.sum(1)[:, None]] = np.nan
        roots = np.where(act[:, None], nz, roots)
        nroot = np.where(act, has.sum(1), nroot)
    z = np.where(np.isnan(roots), 0.0, roots)
    pc = p[:, None, :]
    for _ in range(NEWTON_STEPS):
        v = np.zeros(z.shape)
        dv = np.zeros(z.shape)
        for c in range(10, -1, -1):
            dv = dv * z + v
            v = v * z + pc[..., c]
        with np.errstate(divide="ignore", invalid="ignore"):
            zn = z - v / dv
        ok = (dv != 0) & np.isfinite(zn) & (np.abs(zn - z) <= 1e-6 * (1.0 + np.abs(z)))
        z = np.where(ok, zn, z)
    z = np.where(icol < nroot[:, None], z, np.nan)
    return z, nroot


def essential_residual(e):
    """max |2 E E^T E - tr(E E^T) E| of a row-major E [9] (python floats), in pose_hyp's order of operations.  Zero
    exactly when E's singular values are (s, s, 0): the cubic implies det E = 0."""
    EE = [[(e[3 * i] * e[3 * j] + e[3 * i + 1] * e[3 * j + 1]) + e[3 * i + 2] * e[3 * j + 2] for j in range(3)]
          for i in range(3)]
    tr = (EE[0][0] + EE[1][1]) + EE[2][2]
    r = 0.0
    for i in range(3):
        for j in range(3):
            v = ((EE[i][0] * e[j] + EE[i][1] * e[3 + j]) + EE[i][2] * e[6 + j]) * 2.0 - tr * e[3 * i + j]
            r = max(r, abs(v))
    return r


def five_point(x1, y1, x2, y2):
    """Samples [S][5] of normalised coordinates -> models [S][10][9] (unit Frobenius norm; zero-padded), count [S]."""
    x1, y1, x2, y2 = (np.asarray(a, np.float64) for a in (x1, y1, x2, y2))
    S = len(x1)
    N, bad = null_basis(x1, y1, x2, y2)
    C, bad2 = _gauss_jordan(constraint_matrix(N), 10)
    bad |= bad2
    bx, by, b1 = b_matrix(C)
    poly = det_poly(bx, by, b1)
    poly[bad] = 0.0
    z, nroot = real_roots(poly)
    models = np.zeros((S, 10, 9))
    count = np.zeros(S, np.int64)
    for s in range(S):
        for k in range(int(nroot[s])):
            zz = z[s, k]
            rows = []
            for i in range(3):
                rows.append([_h1(bx[i][s], zz), _h1(by[i][s], zz), _h1(b1[i][s], zz)])
            best, bn = None, -1.0
            for a, b in ((0, 1), (0, 2), (1, 2)):
                v = _cross(rows[a], rows[b])
                n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                if n2 > bn:
                    best, bn = v, n2
            if not (abs(best[2]) > PIVOT_EPS * math.sqrt(bn)):
                continue
            x, y = best[0] / best[2], best[1] / best[2]
            e = [((x * N[s, 0, i] + y * N[s, 1, i]) + zz * N[s, 2, i]) + N[s, 3, i] for i in range(9)]
            nn = 0.0
            for v in e:
                nn = nn + v * v
            nn = math.sqrt(nn)
            if not (nn > 0.0 and math.isfinite(nn)):
                continue
            e = [v / nn for v in e]
            if not (essential_residual(e) <= ESS_EPS):
                continue
            models[s, count[s]] = e
            count[s] += 1
    return models, count


def _h1(c, z):
    v = 0.0
    for k in range(len(c) - 1, -1, -1):
        v = v * z + float(c[k])
    return v


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ------------------------------------------------------------------------------------------------ small linear algebra
def jacobi_eigen(A):
    """Cyclic Jacobi on a symmetric n x n (python floats): (eigenvalues, V with eigenvectors as columns)."""
    n = len(A)
    A = [list(map(float, r)) for r in A]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(JACOBI_SWEEPS):
        off, diag = 0.0, 0.0
        for p in range(n):
            diag = diag + A[p][p] * A[p][p]
            for q in range(p + 1, n):
                off = off + A[p][q] * A[p][q]
        if not off > JACOBI_TOL * diag:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def smallest_eigvec(A):
    w, V = jacobi_eigen(A)
    j = 0
    for i in range(1, len(w)):
        if w[i] < w[j]:
            j = i
    return [V[k][j] for k in range(len(w))]


def svd3(E):
    """One-sided Jacobi SVD of a 3 x 3 (python floats): U, s (descending), V with A = U diag(s) V^T.  U's third column
    is U0 x U1, so det U = det V = +1."""
    A = [[float(E[3 * i + j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        changed = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            a = (A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p]
            b = (A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q]
            g = (A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]
            if not (abs(g) > 1e-15 * math.sqrt(a * b)):
                continue
            changed = True
            theta = (b - a) / (2.0 * g)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = A[k][p], A[k][q]
                A[k][p] = c * akp - s * akq
                A[k][q] = s * akp + c * akq
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
        if not changed:
            break
    sv = [math.sqrt((A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j]) for j in range(3)]
    order = [0, 1, 2]
    for i in range(3):                               # stable descending selection
        for j in range(i + 1, 3):
            if sv[order[j]] > sv[order[i]]:
                order[i], order[j] = order[j], order[i]
    s = [sv[o] for o in order]
    Vs = [[V[k][o] for o in order] for k in range(3)]
    U = [[0.0] * 3 for _ in range(3)]
    for j in range(2):
        o = order[j]
        for k in range(3):
            U[k][j] = A[k][o] / sv[o] if sv[o] > 0.0 else 0.0
    u2 = _cross([U[0][0], U[1][0], U[2][0]], [U[0][1], U[1][1], U[2][1]])
    for k in range(3):
        U[k][2] = u2[k]
    if _det3(Vs) < 0.0:                              # the sort may leave an odd permutation: flip V's last column
        for k in range(3):
            Vs[k][2] = -Vs[k][2]
    return U, s, Vs


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) \
        + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])


def _mm3(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _t3(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def project_essential(E):
    """U diag(1, 1, 0) V^T of E's svd3, row-major [9]."""
    U, _, V = svd3(E)
    return [U[i][0] * V[j][0] + U[i][1] * V[j][1] for i in range(3) for j in range(3)]


def decompose(E):
    """cv::decomposeEssentialMat on svd3: (R1, R2, t) as 3 x 3 / 3 lists of python floats."""
    U, _, V = svd3(E)
    Vt = _t3(V)
    if _det3(U) < 0.0:
        U = [[-v for v in r] for r in U]
    if _det3(Vt) < 0.0:
        Vt = [[-v for v in r] for r in Vt]
    W = [[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    R1 = _mm3(_mm3(U, W), Vt)
    R2 = _mm3(_mm3(U, _t3(W)), Vt)
    return R1, R2, [U[0][2], U[1][2], U[2][2]]


def candidates(E):
    """The four f32 poses [4][4][4] in the reference's order (R1, t), (R1, -t), (R2, t), (R2, -t)."""
    R1, R2, t = decompose(E)
    out = np.zeros((4, 4, 4), np.float32)
    for c, (R, sg) in enumerate(((R1, 1.0), (R1, -1.0), (R2, 1.0), (R2, -1.0))):
        out[c] = np.eye(4, dtype=np.float32)
        out[c, :3, :3] = np.array(R, np.float64).astype(np.float32)
        out[c, :3, 3] = (np.array(t, np.float64) * sg).astype(np.float32)
    return out


def cheirality_counts(cands, pix_from, pix_to, K, finite):
    """triangulate_points(every finite match, I, candidate, K, 0.9999, 2.0).size() per candidate (the oracle's DLT)."""
    import pyoracle
    f = np.flatnonzero(finite)
    uv1 = np.asarray(pix_from, np.float32)[f]
    uv2 = np.asarray(pix_to, np.float32)[f]
    counts = []
    for c in range(len(cands)):
        if len(f) == 0:
            counts.append(0)
            continue
        poses = np.stack([np.eye(4, dtype=np.float32), cands[c]])
        r = pyoracle.triangulate(uv1, uv2, poses, np.asarray(K, np.float32))
        counts.append(int(r["keep"].sum()))
    return counts


def first_strict_max(counts):
    best, most = 0, 0
    for i, c in enumerate(counts):
        if c > most:
            best, most = i, c
    return best


# ------------------------------------------------------------------------------------------------ estimate_pose
def normal_matrix(x1, y1, x2, y2, mask):
    """The 9 x 9 normal matrix of the masked points in pose_final's order: thread t (of THREADS) sums the products
    q_a q_b (a <= b) of its points t, t + THREADS, ... in turn; a wave64 butterfly (xor 32, 16, .., 1) leaves lane 0
    of each wave with its sum; the four waves are added as ((w0 + w1) + w2) + w3."""
    q = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)
    iu = [(a, b) for a in range(9) for b in range(a, 9)]
    prod = np.stack([q[:, a] * q[:, b] for a, b in iu], -1)                        # [n][45]
    prod[~np.asarray(mask, bool)] = 0.0
    n = len(prod)
    rows = -(-n // THREADS)
    pad = np.zeros((rows * THREADS, 45))
    pad[:n] = prod
    pad = pad.reshape(rows, THREADS, 45)
    acc = np.zeros((THREADS, 45))
    for r in range(rows):                                                          # each thread's points in turn
        acc = acc + pad[r]
    waves = acc.reshape(THREADS // 64, 64, 45)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ off]
    w = waves[:, 0]
    tot = ((w[0] + w[1]) + w[2]) + w[3]
    A = [[0.0] * 9 for _ in range(9)]
    for k, (a, b) in enumerate(iu):
        A[a][b] = A[b][a] = float(tot[k])
    return A


def estimate_pose(pix_from, pix_to, K, threshold_px=1.0, confidence=0.99, max_hypotheses=1000, seed=0, stages=False):
    """pose::estimate_pose on matched pixels [n][2] f32.  Returns dict(pose [4][4] f32, inlier [n] u8, count, status,
    E [9], best (h, m), drawn, cands, cheir, chosen, lo_kept) and, with stages=True, samples / models / nmodels /
    scores of every drawn hypothesis."""
    pix_from = np.asarray(pix_from, np.float32).reshape(-1, 2)
    pix_to = np.asarray(pix_to, np.float32).reshape(-1, 2)
    n = len(pix_from)
    fx, fy = float(K[0]), float(K[1])
    x1, y1 = normalise(pix_from, K)
    x2, y2 = normalise(pix_to, K)
    finite = np.isfinite(x1) & np.isfinite(y1) & np.isfinite(x2) & np.isfinite(y2)
    t = threshold_px / ((fx + fy) / 2.0)
    thr2 = t * t
    X1, Y1, X2, Y2 = (np.where(finite, a, 0.0) for a in (x1, y1, x2, y2))

    def score(E):
        err = sampson(E, X1, Y1, X2, Y2)
        return (err < thr2) & finite

    out = dict(pose=np.eye(4, dtype=np.float32), inlier=np.zeros(n, np.uint8), count=0, status=STATUS_FEW_POINTS,
               E=np.zeros(9), best=(-1, -1), drawn=0, cands=None, cheir=[0, 0, 0, 0], chosen=-1, lo_kept=0, thr2=thr2,
               samples=np.full((0, 5), -1), models=np.zeros((0, 10, 9)), nmodels=np.zeros(0, np.int64),
               scores=np.zeros((0, 10), np.int64))
    if n < 5:
        return out
    out["status"] = STATUS_FAILED
    samples, models, nmod, scores = [], [], [], []
    best_key = 0
    drawn = 0
    while drawn < max_hypotheses:
        hs = list(range(drawn, min(drawn + ROUND, max_hypotheses)))
        sm = [sample(seed, h, n, finite) for h in hs]
        ok = np.array([s is not None for s in sm])
        idx = np.array([s if s is not None else [0] * 5 for s in sm])
        mdl, cnt = five_point(x1[idx], y1[idx], x2[idx], y2[idx]) if len(idx) else (np.zeros((0, 10, 9)), np.zeros(0, np.int64))
        cnt = np.where(ok, cnt, 0)
        sc = np.zeros((len(hs), 10), np.int64)
        for a, h in enumerate(hs):
            for m in range(int(cnt[a])):
                sc[a, m] = int(score(mdl[a, m]).sum())
                key = (int(sc[a, m]) << 32) | (0xFFFFFFFF - (10 * h + m))
                best_key = max(best_key, key)
        samples.append(np.where(ok[:, None], idx, -1))
        models.append(mdl)
        nmod.append(cnt)
        scores.append(sc)
        drawn = hs[-1] + 1
        if drawn >= needed_hypotheses(best_key >> 32, n, confidence):
            break
    out["drawn"] = drawn
    if stages:
        out.update(samples=np.concatenate(samples), models=np.concatenate(models), nmodels=np.concatenate(nmod),
                   scores=np.concatenate(scores))
    best_count = best_key >> 32
    if best_count < 5:
        return out
    bi = 0xFFFFFFFF - (best_key & 0xFFFFFFFF)
    h, m = bi // 10, bi % 10
    out["best"] = (h, m)
    E = list(np.concatenate(models)[h, m])
    mask = score(np.array(E))
    count = int(mask.sum())
    for _ in range(LO_ROUNDS):
        if count < 8:
            break
        A = normal_matrix(X1, Y1, X2, Y2, mask)
        En = project_essential(smallest_eigvec(A))
        mn = score(np.array(En))
        if int(mn.sum()) < count:
            break
        E, mask, count = En, mn, int(mn.sum())
        out["lo_kept"] += 1
    cands = candidates(E)
    cheir = cheirality_counts(cands, pix_from, pix_to, K, finite)
    ch = first_strict_max(cheir)
    out.update(pose=cands[ch], inlier=mask.astype(np.uint8), count=count, status=STATUS_OK, E=np.array(E), cands=cands,
               cheir=cheir, chosen=ch)
    return out


# ------------------------------------------------------------------------------------------------ known rotation
def _f(v):
    return np.float32(v)


def rays_f32(pix, K):
    fx, fy, cx, cy = (np.float32(k) for k in K)
    p = np.asarray(pix, np.float32)
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, np.ones(len(p), np.float32)], -1).astype(np.float32)


def _matvec_f32(M, v):
    """M [3][3] f32, v [n][3] f32: rows (M0 v0 + M1 v1) + M2 v2."""
    return np.stack([(M[i, 0] * v[:, 0] + M[i, 1] * v[:, 1]) + M[i, 2] * v[:, 2] for i in range(3)], -1).astype(np.float32)


def _cross_f32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(np.float32)


def essential_tr_f32(t, R):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float32)
    return np.array([[(tx[i, 0] * R[0, j] + tx[i, 1] * R[1, j]) + tx[i, 2] * R[2, j] for j in range(3)] for i in range(3)],
                    np.float32)


def epipolar_error_f32(E, fr, to, focal):
    """The reference's epipolar_error (:93-106) in f32, this order of operations; FLT_MAX for a tiny denominator."""
    lt = _matvec_f32(E, fr)
    lf = _matvec_f32(E.T.copy(), to)
    den = (lt[:, 0] * lt[:, 0] + lt[:, 1] * lt[:, 1]) + (lf[:, 0] * lf[:, 0] + lf[:, 1] * lf[:, 1])
    num = (to[:, 0] * lt[:, 0] + to[:, 1] * lt[:, 1]) + to[:, 2] * lt[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        err = (np.float32(focal) * np.abs(num)) / np.sqrt(den)
    return np.where(den < np.float32(1e-12), np.float32(np.finfo(np.float32).max), err).astype(np.float32)


def estimate_pose_known_rotation(pix_from, pix_to, K, R, pairs, max_epipolar_px=2.0):
    """pose::estimate_pose_with_known_rotation with the (i, j) pairs given.  Returns dict(pose [4][4] f32, inlier [n] u8,
    count, status, support [n_iter] (-1: skipped), trans [n_iter][3] f32, best_iter, best_t, t_refit, front (+, -))."""
    pix_from = np.asarray(pix_from, np.float32).reshape(-1, 2)
    pix_to = np.asarray(pix_to, np.float32).reshape(-1, 2)
    R = np.asarray(R, np.float32).reshape(3, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pix_from)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R
    out = dict(pose=pose, inlier=np.zeros(n, np.uint8), count=0, status=STATUS_FEW_POINTS,
               support=np.full(len(pairs), -1, np.int64), trans=np.zeros((len(pairs), 3), np.float32), best_iter=-1,
               best_t=np.array([0, 0, 1], np.float32), t_refit=None, front=(0, 0))
    if n < 8:
        return out
    out["status"] = STATUS_FAILED
    focal = np.float32(K[0])
    fr, to = rays_f32(pix_from, K), rays_f32(pix_to, K)
    cons = _cross_f32(_matvec_f32(R, fr), to)
    best_t, best_s, best_it = np.array([0, 0, 1], np.float32), 0, -1
    for it, (i, j) in enumerate(pairs):
        if i == j or not (0 <= i < n and 0 <= j < n):               # out of range: skipped, as the kernel does
            continue
        tr = _cross_f32(cons[i], cons[j])
        nrm = np.sqrt(np.float32((tr[0] * tr[0] + tr[1] * tr[1]) + tr[2] * tr[2]))
        if nrm < np.float32(1e-9):
            continue
        tr = (tr / nrm).astype(np.float32)
        E = essential_tr_f32(tr, R)
        s = int((epipolar_error_f32(E, fr, to, focal) < np.float32(max_epipolar_px)).sum())
        out["support"][it] = s
        out["trans"][it] = tr
        if s > best_s:
            best_s, best_t, best_it = s, tr, it
    out["best_iter"], out["best_t"] = best_it, best_t
    if best_s < 8:
        return out
    E = essential_tr_f32(best_t, R)
    mask = epipolar_error_f32(E, fr, to, focal) < np.float32(max_epipolar_px)
    inl = np.flatnonzero(mask)
    c = cons[inl].astype(np.float64)
    A = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            s = 0.0
            for k in range(len(c)):
                s = s + c[k, a] * c[k, b]
            A[a][b] = s
    t = np.array(smallest_eigvec(A), np.float64).astype(np.float32)
    if np.float32((t[0] * best_t[0] + t[1] * best_t[1]) + t[2] * best_t[2]) < 0:
        t = -t
    out["t_refit"] = t.copy()

    def in_front(tc):
        P = np.eye(4, dtype=np.float32)
        P[:3, :3] = R
        P[:3, 3] = tc
        import pyoracle
        r = pyoracle.triangulate(pix_from[inl], pix_to[inl], np.stack([np.eye(4, dtype=np.float32), P]),
                                 np.asarray(K, np.float32))
        return int(r["keep"].sum())

    fp, fm = in_front(t), in_front(-t)
    out["front"] = (fp, fm)
    if fm > fp:
        t = -t
    pose[:3, 3] = t
    out.update(pose=pose, inlier=mask.astype(np.uint8), count=len(inl), status=STATUS_OK)
    return out
