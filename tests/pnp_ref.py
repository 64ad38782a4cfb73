"""CPU restatement of the absolute-pose stage: P3P RANSAC with an EPnP refit, the device counterpart of the two
cv::solvePnPRansac(..., 200, threshold, 0.99, inliers, cv::SOLVEPNP_EPNP) calls of the reference (LoopDetector's
verify_pnp, src/LoopDetector.cpp:176-229, and Initialization's third-view check, src/Initialization.cpp:188-228).
numpy, f64 unless stated.  Test infrastructure only; the product package never imports it.  csrc/pnp.hip follows this
file operation by operation.

Agreement with cv::solvePnPRansac is NOT claimed: OpenCV's RNG and its RANSAC internals cannot be restated bit for bit,
so, as with the essential matrix (essential_ref.py), this file is the project's own specification:

  input       n object points (f32 xyz), n pixels (f32), K = fx, fy, cx, cy.  x = (u - cx) / fx, y = (v - cy) / fy in
              f64.  A correspondence with a non-finite coordinate is never sampled, never an inlier, never refitted.
  sampling    essential_ref.draw: hypothesis h takes its first 4 distinct finite indices of MAX_DRAWS draws.
  solver      Grunert's P3P on the first three of the four: with s2 = u s1, s3 = v s1 the law of cosines gives
              u = N(v) / D(v) (N quadratic, D linear) and the quartic N^2 - 2 cos(gamma) N D + (1 - (c^2 / b^2) W) D^2,
              W = 1 - 2 cos(beta) v + v^2, built by polynomial products.  Its real roots come from
              essential_ref.real_roots (zero-padded to degree 10).  Where D(v) nearly vanishes (a near-double root:
              a triangle seen from near a plane of symmetry) u comes from the third cosine law instead, both of its
              roots; every (u, v) then takes two Newton steps in the cosine laws themselves (p3p_ratios, p3p_polish)
              and is dropped if it lands on a pair that the triple already has.
              A pair gives a model iff v > 0, u > 0, the three
              cosine laws hold to P3P_EPS, and the model is finite; R, t from the orthonormal frames of the two
              triangles (no SVD).  Up to 4 models, the first 4 in ascending root order should a near-double root
              yield a fifth; a collinear or coincident triple yields none.  The fourth index
              only keeps OpenCV's sample size.
  score       the integer count of points with positive depth and squared reprojection error (pixels) < threshold^2.
              Every model of every hypothesis is scored; ties go to the lower 4 h + m.
  stopping    rounds of 256; stop once drawn >= log(1 - confidence) / log(1 - w^4), w = best count / n
              (essential_ref.needed_hypotheses with size 4).
  refit       EPnP (Lepetit, Moreno-Noguer, Fua 2009) in normalised coordinates over the best model's inliers, >= 6 of
              them: control points from the centroid and the principal axes; M^T M from 40 sums in the kernel's fixed
              order (ordered_sum); its 12 x 12 eigenvectors by essential_ref.jacobi_eigen; beta approximations N = 1, 2,
              3 (linearisation, normal equations), 5 Gauss-Newton steps each on the N betas; R, t by svd3 of the
              3 x 3 correlation of the control-point offsets (which equals the all-point absolute orientation, the
              barycentric coordinates being whitened); the candidate with the smallest summed squared reprojection
              error wins.  The refit is kept iff its count over all points is >= the minimal model's.
  status      0 ok; 1 fewer than 4 finite points; 2 no model with >= 4 inliers.  1, 2: identity pose, no inliers.
"""
import math

import numpy as np

import essential_ref as E
from essential_ref import MAX_DRAWS, ROUND, THREADS, draw, jacobi_eigen, real_roots, splitmix64, svd3  # noqa: F401

P3P_EPS = 1e-6              # relative residual of each cosine law that a model may have
D_EPS = 1e-3                # |D(v)| <= D_EPS (|D0| + |D1 v|): u = N / D is 0 / 0, take u from the third cosine law
POLISH_STEPS = 2            # Newton steps on (u, v) in the cosine laws after the quartic
POLISH_MAX = 1e-3           # a polishing step longer than POLISH_MAX (1 + |u|) or (1 + |v|) is not taken
DUP_EPS = 1e-6              # a polished (u, v) within DUP_EPS (1 + |.|) of an earlier model's of the same triple is dropped
COLLINEAR_EPS = 1e-6        # |(P2 - P1) x (P3 - P1)| must exceed COLLINEAR_EPS |P2 - P1| |P3 - P1|
SOLVE_EPS = 1e-13           # a pivot of the small normal equations must exceed SOLVE_EPS * max |entry|
GN_STEPS = 5
MIN_REFIT = 6
STATUS_OK, STATUS_FEW_POINTS, STATUS_FAILED = 0, 1, 2
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                 # control-point pairs
MONO = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))                  # beta_k beta_l; the first 1, 3, 6 serve N = 1, 2, 3


def sample(seed, h, n, finite):
    return E.sample(seed, h, n, finite, 4)


def needed_hypotheses(best_count, n, confidence):
    return E.needed_hypotheses(best_count, n, confidence, 4)


# ------------------------------------------------------------------------------------------------ P3P
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _pmul(a, b):
    out = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] + a[i] * b[j]
    return out


def p3p_setup(P, x, y):
    """P [3][3], x, y [3] (python floats).  None for a collinear / coincident triple, else the quartic (5 coefficients
    ascending) and what the models need."""
    jv = []
    for k in range(3):
        nrm = math.sqrt((x[k] * x[k] + y[k] * y[k]) + 1.0)
        jv.append([x[k] / nrm, y[k] / nrm, 1.0 / nrm])
    d21, d31, d32 = _sub(P[1], P[0]), _sub(P[2], P[0]), _sub(P[2], P[1])
    a2, b2, c2 = _dot(d32, d32), _dot(d31, d31), _dot(d21, d21)
    cr = _cross(d21, d31)
    if not (_dot(cr, cr) > (COLLINEAR_EPS * COLLINEAR_EPS) * (b2 * c2)):
        return None
    ca, cb, cg = _dot(jv[1], jv[2]), _dot(jv[0], jv[2]), _dot(jv[0], jv[1])
    q1 = (a2 - c2) / b2
    r = c2 / b2
    N = [1.0 + q1, -2.0 * q1 * cb, q1 - 1.0]
    D = [2.0 * cg, -2.0 * ca]
    W = [1.0, -2.0 * cb, 1.0]
    NN, ND, DD = _pmul(N, N), _pmul(N, D), _pmul(D, D)
    G = [1.0 - r * W[0], -(r * W[1]), -(r * W[2])]
    GD = _pmul(G, DD)
    poly = [(NN[k] - (2.0 * cg) * (ND[k] if k < 4 else 0.0)) + GD[k] for k in range(5)]
    return dict(poly=poly, j=jv, a2=a2, b2=b2, c2=c2, ca=ca, cb=cb, cg=cg, N=N, D=D, P=P)


def _frame(p0, p1, p2):
    """Orthonormal frame of a triangle: e1 along p1 - p0, e3 the normal, e2 = e3 x e1; None when degenerate."""
    d1, d2 = _sub(p1, p0), _sub(p2, p0)
    n1 = math.sqrt(_dot(d1, d1))
    if not n1 > 0.0:
        return None
    e1 = [d1[0] / n1, d1[1] / n1, d1[2] / n1]
    nv = _cross(e1, d2)
    n3 = math.sqrt(_dot(nv, nv))
    if not n3 > 0.0:
        return None
    e3 = [nv[0] / n3, nv[1] / n3, nv[2] / n3]
    return e1, _cross(e3, e1), e3


def p3p_ratios(s, v):
    """(den, the candidates for u = s2 / s1 in ascending order) of root v.  u = N(v) / D(v), except where D(v) nearly
    vanishes: |D(v)| <= D_EPS (|D0| + |D1 v|).  There N(v) vanishes with it (a triangle seen from near a plane of
    symmetry: a near-double root) and the quotient keeps no digits, so u comes from the third cosine law with
    s1^2 = b2 / den instead, u^2 - 2 cos(gamma) u + (1 - (c2 / b2) den) = 0; both roots go through the gates."""
    if not v > 0.0:
        return 0.0, []
    D0, D1 = s["D"][0], s["D"][1] * v
    Dv = D1 + D0
    den = (v * v - (2.0 * s["cb"]) * v) + 1.0
    if not den > 0.0:
        return den, []
    if abs(Dv) <= D_EPS * (abs(D0) + abs(D1)):
        c0 = 1.0 - (s["c2"] / s["b2"]) * den
        disc = s["cg"] * s["cg"] - c0
        if not disc >= 0.0:
            return den, []
        q = s["cg"] + math.copysign(math.sqrt(disc), s["cg"])
        if q == 0.0:
            return den, []
        ua, ub = q, c0 / q
        return den, [min(ua, ub), max(ua, ub)]
    return den, [((s["N"][2] * v + s["N"][1]) * v + s["N"][0]) / Dv]


def p3p_polish(s, u, v):
    """POLISH_STEPS guarded Newton steps on (u, v) in the two cosine laws divided by s1^2 = b2 / den,
    f1 = u^2 + v^2 - 2 u v cos(alpha) - (a2 / b2) den, f2 = 1 + u^2 - 2 u cos(gamma) - (c2 / b2) den.  The quartic's
    coefficients lose digits where its four roots lie close together (a small triangle far away, two bearings nearly
    equal), and u = N / D loses more; the pair of quadrics is as well conditioned as the pose itself.  A step is taken
    only if it is finite and no longer than POLISH_MAX (1 + |.|), so a double root (a singular Jacobian) stays put."""
    qa, qc = s["a2"] / s["b2"], s["c2"] / s["b2"]
    ca, cb, cg = s["ca"], s["cb"], s["cg"]
    for _ in range(POLISH_STEPS):
        den = (v * v - (2.0 * cb) * v) + 1.0
        dd = 2.0 * v - 2.0 * cb
        f1 = ((u * u + v * v) - ((2.0 * u) * v) * ca) - qa * den
        f2 = ((1.0 + u * u) - (2.0 * u) * cg) - qc * den
        j11, j12 = 2.0 * u - (2.0 * v) * ca, (2.0 * v - (2.0 * u) * ca) - qa * dd
        j21, j22 = 2.0 * u - 2.0 * cg, -(qc * dd)
        det = j11 * j22 - j12 * j21
        if det == 0.0:
            break
        du, dv = (f1 * j22 - j12 * f2) / det, (j11 * f2 - f1 * j21) / det
        if not (abs(du) <= POLISH_MAX * (1.0 + abs(u)) and abs(dv) <= POLISH_MAX * (1.0 + abs(v))):
            break
        u, v = u - du, v - dv
    return u, v


def p3p_model(s, v, u):
    """The model [R | t] (12 floats, row-major 3 x 4) of the polished pair (u, v), or None."""
    den = (v * v - (2.0 * s["cb"]) * v) + 1.0
    if not (u > 0.0 and v > 0.0 and den > 0.0):
        return None
    s1 = math.sqrt(s["b2"] / den)
    s2, s3 = u * s1, v * s1
    r1 = ((s2 * s2 + s3 * s3) - ((2.0 * s2) * s3) * s["ca"]) - s["a2"]
    r2 = ((s1 * s1 + s3 * s3) - ((2.0 * s1) * s3) * s["cb"]) - s["b2"]
    r3 = ((s1 * s1 + s2 * s2) - ((2.0 * s1) * s2) * s["cg"]) - s["c2"]
    if not (abs(r1) <= P3P_EPS * s["a2"] and abs(r2) <= P3P_EPS * s["b2"] and abs(r3) <= P3P_EPS * s["c2"]):
        return None
    C = [[sk * jk for jk in j] for sk, j in zip((s1, s2, s3), s["j"])]
    fc, fw = _frame(C[0], C[1], C[2]), _frame(s["P"][0], s["P"][1], s["P"][2])
    if fc is None or fw is None:
        return None
    R = [[(fc[0][i] * fw[0][k] + fc[1][i] * fw[1][k]) + fc[2][i] * fw[2][k] for k in range(3)] for i in range(3)]
    t = [C[0][i] - _dot(R[i], s["P"][0]) for i in range(3)]
    m = [R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2]]
    if not all(math.isfinite(q) for q in m):
        return None
    return m


def p3p(P, x, y):
    """Triples: P [S][3][3], x, y [S][3] -> models [S][4][12] (zero-padded, in ascending root order), count [S]."""
    P, x, y = np.asarray(P, np.float64), np.asarray(x, np.float64), np.asarray(y, np.float64)
    S = len(P)
    setups = [p3p_setup([[float(q) for q in p] for p in P[s]], [float(q) for q in x[s]], [float(q) for q in y[s]])
              for s in range(S)]
    polys = np.zeros((S, 11))
    for s, st in enumerate(setups):
        if st is not None:
            polys[s, :5] = st["poly"]
    models = np.zeros((S, 4, 12))
    count = np.zeros(S, np.int64)
    if S == 0:
        return models, count
    z, nroot = real_roots(polys)
    kept = [[] for _ in range(S)]
    for s, st in enumerate(setups):
        if st is None:
            continue
        for k in range(int(nroot[s])):
            v = float(z[s, k])
            _, us = p3p_ratios(st, v)
            for u in us:
                if count[s] >= 4:
                    break
                up, vp = p3p_polish(st, u, v)
                # the wrong one of the cosine law's two roots may be drawn onto a neighbouring solution: once is enough
                if any(abs(up - ua) <= DUP_EPS * (1.0 + abs(up)) and abs(vp - va) <= DUP_EPS * (1.0 + abs(vp)) for ua, va in kept[s]):
                    continue
                m = p3p_model(st, vp, up)
                if m is not None:
                    models[s, count[s]] = m
                    kept[s].append((up, vp))
                    count[s] += 1
    return models, count


# ------------------------------------------------------------------------------------------------ score
def reproj2(m, X, Y, Z, x, y, fx, fy):
    """(depth [n], squared reprojection error in pixels [n]) of model m [12], in this order of operations."""
    xc = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    yc = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    zc = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = fx * (xc / zc - x)
        ey = fy * (yc / zc - y)
    return zc, ex * ex + ey * ey


# ------------------------------------------------------------------------------------------------ EPnP
def ordered_sum(vals, mask):
    """Column sums of the masked rows of vals [n][k] in pnp_final's order: thread t (of THREADS) adds its rows t,
    t + THREADS, ... in turn; a wave64 butterfly (xor 32, 16, .., 1); the four waves as ((w0 + w1) + w2) + w3."""
    vals = np.array(vals, np.float64)
    vals[~np.asarray(mask, bool)] = 0.0
    n, k = vals.shape
    rows = max(-(-n // THREADS), 1)
    pad = np.zeros((rows * THREADS, k))
    pad[:n] = vals
    pad = pad.reshape(rows, THREADS, k)
    acc = np.zeros((THREADS, k))
    for r in range(rows):
        acc = acc + pad[r]
    waves = acc.reshape(THREADS // 64, 64, k)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ off]
    w = waves[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def solve_small(A, g):
    """Gaussian elimination with partial pivoting of the n x n system A d = g (python floats, n <= 6); None when a
    pivot is <= SOLVE_EPS * max |entry| or anything is non-finite."""
    n = len(g)
    A = [list(map(float, r)) + [float(gi)] for r, gi in zip(A, g)]
    mmax = 0.0
    for r in A:
        for q in r[:n]:
            if not math.isfinite(q):
                return None
            mmax = max(mmax, abs(q))
    if not mmax > 0.0:
        return None
    for c in range(n):
        p = c
        for r in range(c + 1, n):
            if abs(A[r][c]) > abs(A[p][c]):
                p = r
        A[c], A[p] = A[p], A[c]
        piv = A[c][c]
        if not abs(piv) > SOLVE_EPS * mmax:
            return None
        for r in range(c + 1, n):
            f = A[r][c] / piv
            for k in range(c, n + 1):
                A[r][k] = A[r][k] - f * A[c][k]
    d = [0.0] * n
    for c in range(n - 1, -1, -1):
        s = A[c][n]
        for k in range(c + 1, n):
            s = s - A[c][k] * d[k]
        d[c] = s / A[c][c]
    if not all(math.isfinite(q) for q in d):
        return None
    return d


def _normal(L, r, n):
    """(L^T L, L^T r) of the 6-row L [6][n]."""
    A = [[0.0] * n for _ in range(n)]
    g = [0.0] * n
    for a in range(n):
        for b in range(n):
            s = 0.0
            for p in range(6):
                s = s + L[p][a] * L[p][b]
            A[a][b] = s
        s = 0.0
        for p in range(6):
            s = s + L[p][a] * r[p]
        g[a] = s
    return A, g


def epnp(X, Y, Z, x, y, mask, fx, fy, detail=False):
    """EPnP over the masked points.  Returns (model [12] or None, beta case 1 .. 3 or 0)."""
    mask = np.asarray(mask, bool)
    m = int(mask.sum())
    fail = (None, 0, None) if detail else (None, 0)
    if m < 4:
        return fail
    fm = float(m)
    s = ordered_sum(np.stack([X, Y, Z], -1), mask)
    c0 = [float(s[0]) / fm, float(s[1]) / fm, float(s[2]) / fm]
    dx, dy, dz = X - c0[0], Y - c0[1], Z - c0[2]
    cv = ordered_sum(np.stack([dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz], -1), mask)
    cov = [[float(cv[0]), float(cv[1]), float(cv[2])], [float(cv[1]), float(cv[3]), float(cv[4])],
           [float(cv[2]), float(cv[4]), float(cv[5])]]
    lam, V3 = jacobi_eigen(cov)
    sig = []
    for j in range(3):
        q = lam[j] / fm
        if not q > 0.0:
            return fail
        sig.append(math.sqrt(q))
    al = [None] * 4
    for j in range(3):
        al[j + 1] = ((V3[0][j] * dx + V3[1][j] * dy) + V3[2][j] * dz) / sig[j]
    al[0] = ((1.0 - al[1]) - al[2]) - al[3]
    rr = x * x + y * y
    cols = []
    for j in range(4):
        for k in range(j, 4):
            w = al[j] * al[k]
            cols += [w, w * x, w * y, w * rr]
    S = ordered_sum(np.stack(cols, -1), mask)
    M = [[0.0] * 12 for _ in range(12)]
    q = 0
    for j in range(4):
        for k in range(j, 4):
            s1, sx, sy, sr = (float(S[4 * q + i]) for i in range(4))
            q += 1
            for a, b in ((j, k), (k, j)):
                M[3 * a][3 * b] = s1
                M[3 * a + 1][3 * b + 1] = s1
                M[3 * a][3 * b + 2] = -sx
                M[3 * a + 2][3 * b] = -sx
                M[3 * a + 1][3 * b + 2] = -sy
                M[3 * a + 2][3 * b + 1] = -sy
                M[3 * a + 2][3 * b + 2] = sr
    w12, V12 = jacobi_eigen(M)
    order = list(range(12))
    for i in range(3):                               # stable ascending selection of the three smallest
        for j in range(i + 1, 12):
            if w12[order[j]] < w12[order[i]]:
                order[i], order[j] = order[j], order[i]
    v = [[V12[r][order[k]] for r in range(12)] for k in range(3)]
    C = [c0] + [[c0[i] + sig[j] * V3[i][j] for i in range(3)] for j in range(3)]
    rho = []
    dv = [[None] * 6 for _ in range(3)]
    for p, (a, b) in enumerate(PAIRS):
        d = _sub(C[a], C[b])
        rho.append(_dot(d, d))
        for k in range(3):
            dv[k][p] = [v[k][3 * a + i] - v[k][3 * b + i] for i in range(3)]
    cands = []
    for N in (1, 2, 3):
        nm = (1, 3, 6)[N - 1]
        L = [[_dot(dv[MONO[q][0]][p], dv[MONO[q][1]][p]) * (1.0 if MONO[q][0] == MONO[q][1] else 2.0) for q in range(nm)]
             for p in range(6)]
        A, g = _normal(L, rho, nm)
        b = solve_small(A, g)
        if b is None:
            cands.append(None)
            continue
        b = b + [0.0] * (6 - nm)
        if b[0] < 0.0:
            b = [-q for q in b]
        beta = [math.sqrt(b[0]), math.sqrt(max(b[2], 0.0)), math.sqrt(max(b[5], 0.0))]
        if b[1] < 0.0:
            beta[1] = -beta[1]
        if b[3] < 0.0:
            beta[2] = -beta[2]
        beta = beta[:N]
        for _ in range(GN_STEPS):
            J = [[0.0] * N for _ in range(6)]
            res = [0.0] * 6
            for p in range(6):
                cvec = [0.0, 0.0, 0.0]
                for k in range(N):
                    for i in range(3):
                        cvec[i] = cvec[i] + beta[k] * dv[k][p][i]
                res[p] = _dot(cvec, cvec) - rho[p]
                for k in range(N):
                    J[p][k] = 2.0 * _dot(dv[k][p], cvec)
            A, g = _normal(J, res, N)
            d = solve_small(A, g)
            if d is None:
                break
            beta = [beta[k] - d[k] for k in range(N)]
        cc = [[0.0, 0.0, 0.0] for _ in range(4)]
        for j in range(4):
            for k in range(N):
                for i in range(3):
                    cc[j][i] = cc[j][i] + beta[k] * v[k][3 * j + i]
        if cc[0][2] < 0.0:
            cc = [[-q for q in c] for c in cc]
        H = [0.0] * 9
        for j in range(1, 4):
            dc, dw = _sub(cc[j], cc[0]), _sub(C[j], C[0])
            for a in range(3):
                for b_ in range(3):
                    H[3 * a + b_] = H[3 * a + b_] + dc[a] * dw[b_]
        U, _, Vs = svd3(H)
        R = [[(U[i][0] * Vs[k][0] + U[i][1] * Vs[k][1]) + U[i][2] * Vs[k][2] for k in range(3)] for i in range(3)]
        t = [cc[0][i] - _dot(R[i], C[0]) for i in range(3)]
        mdl = [R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2]]
        cands.append(mdl if all(math.isfinite(q) for q in mdl) else None)
    errs = []
    for mdl in cands:
        if mdl is None:
            errs.append(math.inf)
            continue
        zc, e2 = reproj2(mdl, X, Y, Z, x, y, fx, fy)
        e2 = np.where(zc > 0.0, e2, np.inf)
        errs.append(float(ordered_sum(e2[:, None], mask)[0]))
    best, be = 0, math.inf
    for N in (1, 2, 3):
        if errs[N - 1] < be:
            best, be = N, errs[N - 1]
    if best == 0:
        return fail
    return (cands[best - 1], best, dict(errs=errs, cands=cands)) if detail else (cands[best - 1], best)


# ------------------------------------------------------------------------------------------------ the estimator
def prepare(obj, pix, K, object_index=None, pixel_index=None):
    """Gather and normalise: X, Y, Z, x, y f64 [n] (0 where not finite) and finite [n].  A negative index marks a
    non-finite correspondence."""
    obj = np.asarray(obj, np.float32).reshape(-1, 3)
    pix = np.asarray(pix, np.float32).reshape(-1, 2)
    if object_index is not None:
        oi = np.asarray(object_index, np.int64)
        obj = np.where((oi >= 0)[:, None], obj[np.maximum(oi, 0)], np.float32(np.nan)) if len(oi) else obj[:0]
    if pixel_index is not None:
        pi = np.asarray(pixel_index, np.int64)
        pix = np.where((pi >= 0)[:, None], pix[np.maximum(pi, 0)], np.float32(np.nan)) if len(pi) else pix[:0]
    n = min(len(obj), len(pix))
    obj, pix = obj[:n].astype(np.float64), pix[:n].astype(np.float64)
    fx, fy, cx, cy = (float(k) for k in K)
    x, y = (pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy
    fin = np.isfinite(obj).all(1) & np.isfinite(x) & np.isfinite(y)
    z0 = lambda a: np.where(fin, a, 0.0)             # noqa: E731
    return z0(obj[:, 0]), z0(obj[:, 1]), z0(obj[:, 2]), z0(x), z0(y), fin


def estimate_pose_pnp(obj, pix, K, threshold_px=2.0, confidence=0.99, max_hypotheses=200, seed=0, object_index=None,
                      pixel_index=None, stages=False):
    """Returns dict(pose [4][4] f32 world -> camera, Rt [12] f64, mask [n] u8, count, status, best (h, m), best_count,
    drawn, refit_kept, beta_case, thr2) and, with stages=True, samples / nmodels / models / scores of every drawn
    hypothesis."""
    X, Y, Z, x, y, fin = prepare(obj, pix, K, object_index, pixel_index)
    n = len(X)
    fx, fy = float(K[0]), float(K[1])
    thr2 = float(threshold_px) * float(threshold_px)
    ident = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def score(m):
        zc, e2 = reproj2(m, X, Y, Z, x, y, fx, fy)
        return fin & (zc > 0.0) & (e2 < thr2)

    out = dict(pose=np.eye(4, dtype=np.float32), Rt=np.array(ident), mask=np.zeros(n, np.uint8), count=0,
               status=STATUS_FEW_POINTS, best=(-1, -1), best_count=0, drawn=0, refit_kept=0, beta_case=0, thr2=thr2,
               samples=np.full((0, 4), -1), models=np.zeros((0, 4, 12)), nmodels=np.zeros(0, np.int64),
               scores=np.zeros((0, 4), np.int64))
    if int(fin.sum()) < 4:
        return out
    out["status"] = STATUS_FAILED
    samples, models, nmod, scores = [], [], [], []
    best_key, drawn = 0, 0
    while drawn < max_hypotheses:
        hs = list(range(drawn, min(drawn + ROUND, max_hypotheses)))
        sm = [sample(seed, h, n, fin) for h in hs]
        ok = np.array([s is not None for s in sm])
        idx = np.array([s if s is not None else [0] * 4 for s in sm])
        tri = idx[:, :3]
        mdl, cnt = p3p(np.stack([X[tri], Y[tri], Z[tri]], -1), x[tri], y[tri])
        cnt = np.where(ok, cnt, 0)
        sc = np.zeros((len(hs), 4), np.int64)
        for a, h in enumerate(hs):
            for m in range(int(cnt[a])):
                sc[a, m] = int(score(mdl[a, m]).sum())
                best_key = max(best_key, (int(sc[a, m]) << 32) | (0xFFFFFFFF - (4 * h + m)))
        mdl[np.arange(4)[None, :] >= cnt[:, None]] = 0.0
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
    if best_count < 4:
        return out
    bi = 0xFFFFFFFF - (best_key & 0xFFFFFFFF)
    h, m = bi // 4, bi % 4
    Rt = [float(q) for q in np.concatenate(models)[h, m]]
    mask = score(Rt)
    out.update(best=(h, m), best_count=int(best_count), minimal=np.array(Rt))
    if int(mask.sum()) >= MIN_REFIT:
        fit, case = epnp(X, Y, Z, x, y, mask, fx, fy)
        if fit is not None:
            mf = score(fit)
            if int(mf.sum()) >= int(mask.sum()):
                Rt, mask = fit, mf
                out.update(refit_kept=1, beta_case=case)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :] = np.array(Rt, np.float64).reshape(3, 4).astype(np.float32)
    out.update(pose=pose, Rt=np.array(Rt), mask=mask.astype(np.uint8), count=int(mask.sum()), status=STATUS_OK)
    return out
