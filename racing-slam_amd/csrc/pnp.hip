// pnp.hip — the absolute-pose stage: P3P RANSAC with an EPnP refit.
//
// Replaces the two cv::solvePnPRansac(..., 200, threshold, 0.99, inliers, cv::SOLVEPNP_EPNP) calls of the reference
// (LoopDetector's verify_pnp, src/LoopDetector.cpp:176-229; Initialization's third-view check,
// src/Initialization.cpp:188-228).  The specification is tests/pnp_ref.py; this file follows it operation by operation
// (-ffp-contract=off), so sampling, model sets and scores agree with it to rounding.
//
// rs_estimate_pose_pnp: one stream-ordered chain, no host synchronisation, no allocation; the count is read on the device.
// The RANSAC frame (draw, table, key, stop, inlier compaction) is ransac.h's with S = 4, M = 4, D = 12; this file adds:
//   pnp_prep      gather through the two optional index arrays, normalise into f64 SoA scratch, count the finite
//                 correspondences, reset the state and the table
//   pnp_hyp       one lane per hypothesis (4 wave64 workgroups per round of 256): the sample (every lane, in registers),
//                 Grunert's quartic, its real roots by the bisection of ordered 64-bit keys between the roots of the
//                 derivatives (serial per lane), each (u, v) polished by two Newton steps in the cosine laws, up to 4
//                 models [R | t] from the orthonormal frames of the two triangles (the first 4 in ascending root order,
//                 should a near-double root yield a fifth)
//   pnp_score     one workgroup per hypothesis: every point is loaded once and tested against all of its models;
//                 integer counts, the key's atomicMax
//   pnp_stop_k    the adaptive stop after each round of 256 (at once with fewer than 4 finite correspondences); later
//                 rounds exit at entry
//   pnp_final     one workgroup: the best model's mask, the EPnP sums in a fixed order, the 12 x 12 cyclic Jacobi with the
//                 whole workgroup, the three beta cases with Gauss-Newton (lane 0), their summed errors, the keep /
//                 discard decision, the final inlier mask
// No float atomics: two calls with the same inputs write the same bytes.
#include "pose_shared.h"
#include "tri_core.h"

#define PNP_P3P_EPS 1e-6            // relative residual of each cosine law that a model may have
#define PNP_D_EPS 1e-3              // |D(v)| <= this times (|D0| + |D1 v|): u = N / D is 0 / 0, u from the third cosine law
#define PNP_POLISH_STEPS 2          // Newton steps on (u, v) in the cosine laws after the quartic
#define PNP_POLISH_MAX 1e-3         // a polishing step longer than this times (1 + |u|) or (1 + |v|) is not taken
#define PNP_DUP_EPS 1e-6            // a polished (u, v) this close, times (1 + |.|), to an earlier model's is dropped
#define PNP_COLLINEAR_EPS 1e-6      // |(P2 - P1) x (P3 - P1)| must exceed this times |P2 - P1| |P3 - P1|
#define PNP_SOLVE_EPS 1e-13
#define PNP_GN_STEPS 5
#define PNP_MIN_REFIT 6

struct PnpState {
    RansacState r;
    int status, refit_kept, beta_case, inliers;
    int nfin;               // finite correspondences of the last call
    int nfin_acc;           // pnp_prep's atomic counter: zero between calls (pnp_final clears it)
    double Rt[12];
};

struct rs_pnp_estimator : RansacEstimator {          // t: samples [max_hyp][4], models [max_hyp][4][12], scores [max_hyp][4]
    double* x = nullptr;            // [5][max_points] X, Y, Z, x, y
    uint8_t* fin = nullptr;         // [max_points]
    uint8_t* mask = nullptr;        // [2][max_points] the minimal model's mask, the refit's
    PnpState* st = nullptr;
};

struct PnpScratch {
    double *X, *Y, *Z, *x, *y;
    uint8_t* fin;
    RansacTable t;
    PnpState* st;
};

static PnpScratch scratch_of(const rs_pnp_estimator* e)
{
    const size_t m = e->max_points;
    return PnpScratch{e->x, e->x + m, e->x + 2 * m, e->x + 3 * m, e->x + 4 * m, e->fin, e->t, e->st};
}

// ------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void sub3(const double* a, const double* b, double* o)
{
    o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2];
}

// depth and squared reprojection error in pixels of model m [12] (tests/pnp_ref.reproj2)
__device__ __forceinline__ double reproj2(const double* m, double X, double Y, double Z, double x, double y, double fx, double fy,
                                          double* depth)
{
    const double xc = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
    const double yc = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
    const double zc = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    const double ex = fx * (xc / zc - x), ey = fy * (yc / zc - y);
    *depth = zc;
    return ex * ex + ey * ey;
}

// the real roots of a quartic (5 coefficients ascending), ascending: tests/essential_ref.real_roots on one lane
__device__ int quartic_roots(const double* pin, double* z)
{
    double p[5], m = 0.0;
    for (int k = 0; k < 5; k++) m = fmax(m, fabs(pin[k]));
    if (!(m > 0.0 && isfinite(m))) return 0;
    for (int k = 0; k < 5; k++) p[k] = pin[k] / m;
    int d = 4;
    while (d > 0 && fabs(p[d]) < POSE_TRIM_EPS) d--;
    for (int k = d + 1; k < 5; k++) p[k] = 0.0;
    if (d == 0) return 0;
    double bnd = 0.0;
    for (int k = 0; k < d; k++) bnd = fmax(bnd, fabs(p[k] / p[d]));
    const double B = 1.0 + bnd;
    double D[5][5];                                   // D[r] = the r-th derivative, ascending
    for (int k = 0; k < 5; k++) D[0][k] = p[k];
    for (int r = 0; r < 4; r++) {
        for (int k = 0; k < 4; k++) D[r + 1][k] = (double)(k + 1) * D[r][k + 1];
        D[r + 1][4] = 0.0;
    }
    double rt[2][4];
    int nroot = 0;
    for (int j = 1; j <= d; j++) {                    // level j: the roots of D[d - j] (degree j)
        const double* q = D[d - j];
        const double* prev = rt[(j - 1) & 1];
        double* cur = rt[j & 1];
        int nn = 0;
        for (int iv = 0; iv <= nroot; iv++) {
            const double a = iv == 0 ? -B : prev[iv - 1], b = iv == nroot ? B : prev[iv];
            const int sa = poly_sign(q, j, a), sb = poly_sign(q, j, b);
            if (sa != 0 && sb != sa) {
                long long lo = dkey(a), hi = dkey(b);
                for (int it = 0; it < POSE_BISECT_ITERS; it++) {
                    const long long mid = ((lo >> 1) + (hi >> 1)) + (lo & hi & 1ll);
                    if (poly_sign(q, j, dunkey(mid)) == sa) lo = mid; else hi = mid;
                }
                cur[nn++] = dunkey(hi);
            }
        }
        nroot = nn;
    }
    for (int r = 0; r < nroot; r++) {
        double zz = rt[d & 1][r];
        for (int it = 0; it < POSE_NEWTON; it++) {
            double v = 0.0, dv = 0.0;
            for (int c = 4; c >= 0; c--) {
                dv = dv * zz + v;
                v = v * zz + p[c];
            }
            const double zn = zz - v / dv;
            if (dv != 0.0 && isfinite(zn) && fabs(zn - zz) <= 1e-6 * (1.0 + fabs(zz))) zz = zn;
        }
        z[r] = zz;
    }
    return nroot;
}

// orthonormal frame of a triangle (rows e1, e2, e3 of F); false when degenerate
__device__ bool tri_frame(const double* p0, const double* p1, const double* p2, double* F)
{
    double d1[3], d2[3], nv[3];
    sub3(p1, p0, d1);
    sub3(p2, p0, d2);
    const double n1 = sqrt(dot3(d1, d1));
    if (!(n1 > 0.0)) return false;
    for (int i = 0; i < 3; i++) F[i] = d1[i] / n1;
    cross3(F, d2, nv);
    const double n3 = sqrt(dot3(nv, nv));
    if (!(n3 > 0.0)) return false;
    for (int i = 0; i < 3; i++) F[6 + i] = nv[i] / n3;
    cross3(F + 6, F, F + 3);
    return true;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void pnp_prep(const float* __restrict__ object, const int32_t* __restrict__ object_index,
                                                const float2* __restrict__ pixels, const int32_t* __restrict__ pixel_index,
                                                const int32_t* __restrict__ d_count, int max_n, double fx, double fy, double cx,
                                                double cy, int table_hyp, PnpScratch s)
{
    __shared__ int red[4];
    const int n = min(max(*d_count, 0), max_n);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    int c = 0;
    for (int i = tid; i < n; i += stride) {
        const int oi = object_index ? object_index[i] : i, pi = pixel_index ? pixel_index[i] : i;
        float o[3] = {NAN, NAN, NAN};
        if (oi >= 0) { o[0] = object[3 * (size_t)oi]; o[1] = object[3 * (size_t)oi + 1]; o[2] = object[3 * (size_t)oi + 2]; }
        const float2 p = pi >= 0 ? pixels[pi] : make_float2(NAN, NAN);
        const double X = (double)o[0], Y = (double)o[1], Z = (double)o[2];
        const double x = ((double)p.x - cx) / fx, y = ((double)p.y - cy) / fy;
        const bool f = isfinite(X) && isfinite(Y) && isfinite(Z) && isfinite(x) && isfinite(y);
        s.X[i] = f ? X : 0.0; s.Y[i] = f ? Y : 0.0; s.Z[i] = f ? Z : 0.0; s.x[i] = f ? x : 0.0; s.y[i] = f ? y : 0.0;
        s.fin[i] = f ? 1 : 0;
        c += f ? 1 : 0;
    }
    c = block_sum_int(c, red);
    if (threadIdx.x == 0 && c) atomicAdd(&s.st->nfin_acc, c);
    ransac_reset_table<4, 4>(s.t, table_hyp);
    if (tid == 0) {
        PnpState* st = s.st;
        st->r = RansacState{0ull, 0, 0, n, 0, -1, 0};
        st->status = RANSAC_STATUS_FAILED;
        st->refit_kept = 0; st->beta_case = 0; st->inliers = 0;
    }
}

__global__ __launch_bounds__(64) void pnp_hyp(int round, int max_hyp, unsigned long long seed_hash, PnpScratch s)
{
    const int h = round * RANSAC_ROUND + blockIdx.x * 64 + threadIdx.x;
    if (s.st->r.stop || s.st->nfin_acc < 4 || h >= max_hyp) return;
    int idx[4];
    if (!ransac_draw<4>(seed_hash, h, s.st->r.n, s.fin, idx)) { s.t.nmod[h] = 0; return; }
    for (int q = 0; q < 4; q++) s.t.samples[4 * h + q] = idx[q];
    double P[3][3], jv[3][3];
    for (int q = 0; q < 3; q++) {
        const int i = idx[q];
        P[q][0] = s.X[i]; P[q][1] = s.Y[i]; P[q][2] = s.Z[i];
        const double x = s.x[i], y = s.y[i];
        const double nrm = sqrt((x * x + y * y) + 1.0);
        jv[q][0] = x / nrm; jv[q][1] = y / nrm; jv[q][2] = 1.0 / nrm;
    }
    double d21[3], d31[3], d32[3], cr[3];
    sub3(P[1], P[0], d21); sub3(P[2], P[0], d31); sub3(P[2], P[1], d32);
    const double a2 = dot3(d32, d32), b2 = dot3(d31, d31), c2 = dot3(d21, d21);
    cross3(d21, d31, cr);
    if (!(dot3(cr, cr) > (PNP_COLLINEAR_EPS * PNP_COLLINEAR_EPS) * (b2 * c2))) { s.t.nmod[h] = 0; return; }
    const double ca = dot3(jv[1], jv[2]), cb = dot3(jv[0], jv[2]), cg = dot3(jv[0], jv[1]);
    const double q1 = (a2 - c2) / b2, r = c2 / b2;
    const double N[3] = {1.0 + q1, -2.0 * q1 * cb, q1 - 1.0}, D[2] = {2.0 * cg, -2.0 * ca}, W[3] = {1.0, -2.0 * cb, 1.0};
    double NN[5], ND[4], DD[3], GD[5], poly[5], z[4];
    pmul(N, 3, N, 3, NN); pmul(N, 3, D, 2, ND); pmul(D, 2, D, 2, DD);
    const double G[3] = {1.0 - r * W[0], -(r * W[1]), -(r * W[2])};
    pmul(G, 3, DD, 3, GD);
    for (int q = 0; q < 5; q++) poly[q] = (NN[q] - (2.0 * cg) * (q < 4 ? ND[q] : 0.0)) + GD[q];
    const int nroot = quartic_roots(poly, z);
    double Fw[9];
    const bool wok = tri_frame(P[0], P[1], P[2], Fw);
    int nm = 0;
    double ku[4], kv[4];                                     // the (u, v) of the models so far
    for (int q = 0; q < nroot && wok; q++) {
        const double v = z[q];
        if (!(v > 0.0)) continue;
        const double D0 = D[0], D1 = D[1] * v;
        const double Dv = D1 + D0;
        const double den = (v * v - (2.0 * cb) * v) + 1.0;
        if (!(den > 0.0)) continue;
        // u = N(v) / D(v); where D(v) nearly vanishes N(v) does too (a triangle seen from near a plane of symmetry: a
        // near-double root) and the quotient keeps no digits: u then comes from the third cosine law with s1^2 = b2 / den,
        // u^2 - 2 cg u + (1 - r den) = 0, and both of its roots go through the gates below (tests/pnp_ref.p3p_ratios)
        double us[2];
        int nu = 0;
        if (fabs(Dv) <= PNP_D_EPS * (fabs(D0) + fabs(D1))) {
            const double c0 = 1.0 - r * den;
            const double disc = cg * cg - c0;
            if (!(disc >= 0.0)) continue;
            const double qq = cg + copysign(sqrt(disc), cg);
            if (qq == 0.0) continue;
            const double ua = qq, ub = c0 / qq;
            us[0] = fmin(ua, ub); us[1] = fmax(ua, ub);
            nu = 2;
        } else {
            us[0] = ((N[2] * v + N[1]) * v + N[0]) / Dv;
            nu = 1;
        }
        for (int k = 0; k < nu && nm < 4; k++) {             // a fifth model of one triple is dropped: ascending root order
            // two guarded Newton steps on (u, v) in the cosine laws divided by s1^2 (tests/pnp_ref.p3p_polish): the quartic's
            // coefficients lose digits where its roots lie close together, the pair of quadrics does not
            double u = us[k], vv = v;
            const double qa = a2 / b2;
            for (int it = 0; it < PNP_POLISH_STEPS; it++) {
                const double dn = (vv * vv - (2.0 * cb) * vv) + 1.0;
                const double dd = 2.0 * vv - 2.0 * cb;
                const double f1 = ((u * u + vv * vv) - ((2.0 * u) * vv) * ca) - qa * dn;
                const double f2 = ((1.0 + u * u) - (2.0 * u) * cg) - r * dn;
                const double j11 = 2.0 * u - (2.0 * vv) * ca, j12 = (2.0 * vv - (2.0 * u) * ca) - qa * dd;
                const double j21 = 2.0 * u - 2.0 * cg, j22 = -(r * dd);
                const double det = j11 * j22 - j12 * j21;
                if (det == 0.0) break;
                const double du = (f1 * j22 - j12 * f2) / det, dv = (j11 * f2 - f1 * j21) / det;
                if (!(fabs(du) <= PNP_POLISH_MAX * (1.0 + fabs(u)) && fabs(dv) <= PNP_POLISH_MAX * (1.0 + fabs(vv)))) break;
                u = u - du; vv = vv - dv;
            }
            // the wrong one of the cosine law's two roots may be drawn onto a neighbouring solution: once is enough
            bool dup = false;
            for (int j = 0; j < nm; j++)
                dup = dup || (fabs(u - ku[j]) <= PNP_DUP_EPS * (1.0 + fabs(u)) && fabs(vv - kv[j]) <= PNP_DUP_EPS * (1.0 + fabs(vv)));
            if (dup) continue;
            const double dp = (vv * vv - (2.0 * cb) * vv) + 1.0;
            if (!(u > 0.0 && vv > 0.0 && dp > 0.0)) continue;
            const double s1 = sqrt(b2 / dp), s2 = u * s1, s3 = vv * s1;
            const double r1 = ((s2 * s2 + s3 * s3) - ((2.0 * s2) * s3) * ca) - a2;
            const double r2 = ((s1 * s1 + s3 * s3) - ((2.0 * s1) * s3) * cb) - b2;
            const double r3 = ((s1 * s1 + s2 * s2) - ((2.0 * s1) * s2) * cg) - c2;
            if (!(fabs(r1) <= PNP_P3P_EPS * a2 && fabs(r2) <= PNP_P3P_EPS * b2 && fabs(r3) <= PNP_P3P_EPS * c2)) continue;
            double C[3][3], Fc[9], m[12];
            for (int i = 0; i < 3; i++) { C[0][i] = s1 * jv[0][i]; C[1][i] = s2 * jv[1][i]; C[2][i] = s3 * jv[2][i]; }
            if (!tri_frame(C[0], C[1], C[2], Fc)) continue;
            bool fin = true;
            for (int i = 0; i < 3; i++) {
                for (int c = 0; c < 3; c++) m[4 * i + c] = (Fc[i] * Fw[c] + Fc[3 + i] * Fw[3 + c]) + Fc[6 + i] * Fw[6 + c];
                m[4 * i + 3] = C[0][i] - dot3(m + 4 * i, P[0]);
            }
            for (int i = 0; i < 12; i++) fin = fin && isfinite(m[i]);
            if (!fin) continue;
            double* out = s.t.models + 48 * (size_t)h + 12 * nm;
            for (int i = 0; i < 12; i++) out[i] = m[i];
            ku[nm] = u; kv[nm] = vv;
            nm++;
        }
    }
    s.t.nmod[h] = nm;
}

__global__ __launch_bounds__(256) void pnp_score(int round, int max_hyp, double fx, double fy, double thr2, PnpScratch s)
{
    __shared__ int red[4];
    const int h = round * RANSAC_ROUND + blockIdx.x;
    if (s.st->r.stop || s.st->nfin_acc < 4 || h >= max_hyp) return;
    const int nm = s.t.nmod[h], n = s.st->r.n;
    if (nm <= 0) return;                                 // uniform per workgroup
    double m[4][12];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 12; i++) m[q][i] = q < nm ? s.t.models[48 * (size_t)h + 12 * q + i] : 0.0;
    int c[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (!s.fin[i]) continue;
        const double X = s.X[i], Y = s.Y[i], Z = s.Z[i], x = s.x[i], y = s.y[i];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (q < nm) {
                double zc;
                const double e2 = reproj2(m[q], X, Y, Z, x, y, fx, fy, &zc);
                c[q] += (zc > 0.0 && e2 < thr2) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (q >= nm) break;                              // uniform
        const int t = block_sum_int(c[q], red);
        if (threadIdx.x == 0) {
            s.t.scores[4 * h + q] = t;
            atomicMax(&s.st->r.best_key, ransac_key(t, 4 * h + q));
            atomicAdd(&s.st->r.scored, 1);
        }
    }
}

__global__ __launch_bounds__(64) void pnp_stop_k(int round, int max_hyp, double log1mconf, PnpState* st)
{
    if (threadIdx.x != 0 || st->r.stop) return;
    if (st->nfin_acc < 4) { st->r.stop = 1; return; }
    ransac_stop<4>(&st->r, round, max_hyp, log1mconf);
}

struct PnpFinalLds {
    double A[144], V[144];
    double part[4][40], sum[40];
    double Rt[12], cand[3][12];
    double c0[3], sig[3], V3[9];
    int red[4];
    int fail, valid[3], best;
};

// column sums in a fixed order (tests/pnp_ref.ordered_sum): each thread's points in turn, a wave64 butterfly, then the
// four waves as ((w0 + w1) + w2) + w3 into L.sum
template <int K>
__device__ __forceinline__ void ordered_sum(double* acc, PnpFinalLds& L)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = wave_sum_f64(acc[k]);
    __syncthreads();
    if ((tid & 63) == 0)
        for (int k = 0; k < K; k++) L.part[tid >> 6][k] = acc[k];
    __syncthreads();
    if (tid < K) L.sum[tid] = ((L.part[0][tid] + L.part[1][tid]) + L.part[2][tid]) + L.part[3][tid];
    __syncthreads();
}

__device__ __forceinline__ int pnp_score_mask(const double* m, const PnpScratch& s, int n, double fx, double fy, double thr2,
                                              uint8_t* mask, int* red)
{
    int c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double zc;
        const double e2 = reproj2(m, s.X[i], s.Y[i], s.Z[i], s.x[i], s.y[i], fx, fy, &zc);
        const bool in = s.fin[i] && zc > 0.0 && e2 < thr2;
        mask[i] = in ? 1 : 0;
        c += in ? 1 : 0;
    }
    return block_sum_int(c, red);
}

// Gaussian elimination with partial pivoting of the n x n system in A [6][7] (augmented, row stride 7), n <= 6
// (tests/pnp_ref.solve_small)
__device__ bool solve_small(double (*A)[7], int n, double* d)
{
    double mmax = 0.0;
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
            if (!isfinite(A[r][c])) return false;
            mmax = fmax(mmax, fabs(A[r][c]));
        }
    if (!(mmax > 0.0)) return false;
    for (int c = 0; c < n; c++) {
        int p = c;
        for (int r = c + 1; r < n; r++)
            if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
        if (p != c)
            for (int k = 0; k <= n; k++) { const double t = A[c][k]; A[c][k] = A[p][k]; A[p][k] = t; }
        const double piv = A[c][c];
        if (!(fabs(piv) > PNP_SOLVE_EPS * mmax)) return false;
        for (int r = c + 1; r < n; r++) {
            const double f = A[r][c] / piv;
            for (int k = c; k <= n; k++) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
    for (int c = n - 1; c >= 0; c--) {
        double sacc = A[c][n];
        for (int k = c + 1; k < n; k++) sacc = sacc - A[c][k] * d[k];
        d[c] = sacc / A[c][c];
    }
    for (int c = 0; c < n; c++)
        if (!isfinite(d[c])) return false;
    return true;
}

// (L^T L | L^T r) of the 6-row L [6][6] (n columns used) into the augmented A
__device__ void normal6(const double (*Lm)[6], const double* r, int n, double (*A)[7])
{
    for (int a = 0; a < n; a++) {
        for (int b = 0; b < n; b++) {
            double sacc = 0.0;
            for (int p = 0; p < 6; p++) sacc = sacc + Lm[p][a] * Lm[p][b];
            A[a][b] = sacc;
        }
        double sacc = 0.0;
        for (int p = 0; p < 6; p++) sacc = sacc + Lm[p][a] * r[p];
        A[a][n] = sacc;
    }
}

// lane 0 of pnp_final: the three beta cases from the eigenvectors in L.A / L.V (tests/pnp_ref.epnp)
__device__ void epnp_candidates(PnpFinalLds& L)
{
    const int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {1, 2, 3, 2, 3, 3};
    const int MK[6] = {0, 0, 1, 0, 1, 2}, ML[6] = {0, 1, 1, 2, 2, 2};
    int order[12];
    for (int i = 0; i < 12; i++) order[i] = i;
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 12; j++)
            if (L.A[13 * order[j]] < L.A[13 * order[i]]) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    double v[3][12], C[4][3], rho[6], dv[3][6][3];
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 12; r++) v[k][r] = L.V[12 * r + order[k]];
    for (int i = 0; i < 3; i++) {
        C[0][i] = L.c0[i];
        for (int j = 0; j < 3; j++) C[j + 1][i] = L.c0[i] + L.sig[j] * L.V3[3 * i + j];
    }
    for (int p = 0; p < 6; p++) {
        double d[3];
        sub3(C[PA[p]], C[PB[p]], d);
        rho[p] = dot3(d, d);
        for (int k = 0; k < 3; k++)
            for (int i = 0; i < 3; i++) dv[k][p][i] = v[k][3 * PA[p] + i] - v[k][3 * PB[p] + i];
    }
    for (int N = 1; N <= 3; N++) {
        L.valid[N - 1] = 0;
        const int nm = N == 1 ? 1 : (N == 2 ? 3 : 6);
        double Lm[6][6], Aug[6][7], b[6] = {0, 0, 0, 0, 0, 0};
        for (int p = 0; p < 6; p++)
            for (int q = 0; q < nm; q++) Lm[p][q] = dot3(dv[MK[q]][p], dv[ML[q]][p]) * (MK[q] == ML[q] ? 1.0 : 2.0);
        normal6(Lm, rho, nm, Aug);
        if (!solve_small(Aug, nm, b)) continue;
        if (b[0] < 0.0)
            for (int q = 0; q < 6; q++) b[q] = -b[q];
        double beta[3] = {sqrt(b[0]), sqrt(fmax(b[2], 0.0)), sqrt(fmax(b[5], 0.0))};
        if (b[1] < 0.0) beta[1] = -beta[1];
        if (b[3] < 0.0) beta[2] = -beta[2];
        for (int it = 0; it < PNP_GN_STEPS; it++) {
            double res[6], dl[6];
            for (int p = 0; p < 6; p++) {
                double cvec[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < N; k++)
                    for (int i = 0; i < 3; i++) cvec[i] = cvec[i] + beta[k] * dv[k][p][i];
                res[p] = dot3(cvec, cvec) - rho[p];
                for (int k = 0; k < N; k++) Lm[p][k] = 2.0 * dot3(dv[k][p], cvec);
            }
            normal6(Lm, res, N, Aug);
            if (!solve_small(Aug, N, dl)) break;
            for (int k = 0; k < N; k++) beta[k] = beta[k] - dl[k];
        }
        double cc[4][3];
        for (int j = 0; j < 4; j++)
            for (int i = 0; i < 3; i++) {
                double a = 0.0;
                for (int k = 0; k < N; k++) a = a + beta[k] * v[k][3 * j + i];
                cc[j][i] = a;
            }
        if (cc[0][2] < 0.0)
            for (int j = 0; j < 4; j++)
                for (int i = 0; i < 3; i++) cc[j][i] = -cc[j][i];
        double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, U[9], Vs[9];
        for (int j = 1; j < 4; j++) {
            double dc[3], dw[3];
            sub3(cc[j], cc[0], dc);
            sub3(C[j], C[0], dw);
            for (int a = 0; a < 3; a++)
                for (int c = 0; c < 3; c++) H[3 * a + c] = H[3 * a + c] + dc[a] * dw[c];
        }
        svd3(H, U, Vs);
        double* m = L.cand[N - 1];
        bool fin = true;
        for (int i = 0; i < 3; i++) {
            for (int c = 0; c < 3; c++) m[4 * i + c] = (U[3 * i] * Vs[3 * c] + U[3 * i + 1] * Vs[3 * c + 1]) + U[3 * i + 2] * Vs[3 * c + 2];
            m[4 * i + 3] = cc[0][i] - dot3(m + 4 * i, C[0]);
        }
        for (int i = 0; i < 12; i++) fin = fin && isfinite(m[i]);
        L.valid[N - 1] = fin ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void pnp_final(int max_n, double fx, double fy, double thr2, PnpScratch s,
                                                 uint8_t* __restrict__ mask0, uint8_t* __restrict__ mask1,
                                                 float* __restrict__ d_pose, uint8_t* __restrict__ d_inlier,
                                                 int32_t* __restrict__ d_inlier_index, int32_t* __restrict__ d_inlier_count,
                                                 int32_t* __restrict__ d_status)
{
    __shared__ PnpFinalLds L;
    PnpState* st = s.st;
    const int n = st->r.n, nfin = st->nfin_acc, tid = threadIdx.x;
    const unsigned long long key = st->r.best_key;
    const int best_count = ransac_key_count(key);
    const bool ok = nfin >= 4 && best_count >= 4;
    uint8_t* cur = mask0;
    int count = 0, kept = 0, beta_case = 0;
    if (tid < 12) L.Rt[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    __syncthreads();
    if (ok) {
        const int bi = ransac_key_slot(key);
        if (tid < 12) L.Rt[tid] = s.t.models[48 * (size_t)(bi / 4) + 12 * (bi % 4) + tid];
        if (tid == 0) { st->r.best_index = bi; st->r.best_count = best_count; L.fail = 0; }
        __syncthreads();
        count = pnp_score_mask(L.Rt, s, n, fx, fy, thr2, mask0, L.red);
        if (count >= PNP_MIN_REFIT) {                    // uniform
            const double fm = (double)count;
            double acc[40];
            // the centroid
            for (int k = 0; k < 3; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += blockDim.x) {
                if (!mask0[i]) continue;
                acc[0] += s.X[i]; acc[1] += s.Y[i]; acc[2] += s.Z[i];
            }
            ordered_sum<3>(acc, L);
            if (tid < 3) L.c0[tid] = L.sum[tid] / fm;
            __syncthreads();
            const double c0x = L.c0[0], c0y = L.c0[1], c0z = L.c0[2];
            // the covariance, its principal axes (lane 0), the control points' scales
            for (int k = 0; k < 6; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += blockDim.x) {
                if (!mask0[i]) continue;
                const double dx = s.X[i] - c0x, dy = s.Y[i] - c0y, dz = s.Z[i] - c0z;
                acc[0] += dx * dx; acc[1] += dx * dy; acc[2] += dx * dz; acc[3] += dy * dy; acc[4] += dy * dz; acc[5] += dz * dz;
            }
            ordered_sum<6>(acc, L);
            if (tid == 0) {
                double cov[9] = {L.sum[0], L.sum[1], L.sum[2], L.sum[1], L.sum[3], L.sum[4], L.sum[2], L.sum[4], L.sum[5]};
                jacobi_eigen(cov, L.V3, 3);
                for (int j = 0; j < 3; j++) {
                    const double q = cov[4 * j] / fm;
                    if (!(q > 0.0)) L.fail = 1;
                    L.sig[j] = sqrt(q);
                }
            }
            __syncthreads();
            if (!L.fail) {                               // uniform
                // the 40 sums of alpha_j alpha_k {1, x, y, x^2 + y^2}, j <= k
                for (int k = 0; k < 40; k++) acc[k] = 0.0;
                for (int i = tid; i < n; i += blockDim.x) {
                    if (!mask0[i]) continue;
                    const double dx = s.X[i] - c0x, dy = s.Y[i] - c0y, dz = s.Z[i] - c0z, x = s.x[i], y = s.y[i];
                    double al[4];
#pragma unroll
                    for (int j = 0; j < 3; j++) al[j + 1] = ((L.V3[j] * dx + L.V3[3 + j] * dy) + L.V3[6 + j] * dz) / L.sig[j];
                    al[0] = ((1.0 - al[1]) - al[2]) - al[3];
                    const double rr = x * x + y * y;
                    int q = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int k = j; k < 4; k++) {
                            const double w = al[j] * al[k];
                            acc[q] += w; acc[q + 1] += w * x; acc[q + 2] += w * y; acc[q + 3] += w * rr;
                            q += 4;
                        }
                }
                ordered_sum<40>(acc, L);
                for (int i = tid; i < 144; i += blockDim.x) L.A[i] = 0.0;
                __syncthreads();
                if (tid == 0) {
                    int q = 0;
                    for (int j = 0; j < 4; j++)
                        for (int k = j; k < 4; k++, q++) {
                            const double s1 = L.sum[4 * q], sx = L.sum[4 * q + 1], sy = L.sum[4 * q + 2], sr = L.sum[4 * q + 3];
                            for (int w = 0; w < 2; w++) {
                                const int a = w ? k : j, b = w ? j : k;
                                L.A[12 * (3 * a) + 3 * b] = s1;
                                L.A[12 * (3 * a + 1) + 3 * b + 1] = s1;
                                L.A[12 * (3 * a) + 3 * b + 2] = -sx;
                                L.A[12 * (3 * a + 2) + 3 * b] = -sx;
                                L.A[12 * (3 * a + 1) + 3 * b + 2] = -sy;
                                L.A[12 * (3 * a + 2) + 3 * b + 1] = -sy;
                                L.A[12 * (3 * a + 2) + 3 * b + 2] = sr;
                            }
                        }
                }
                __syncthreads();
                jacobi_eigen_block(L.A, L.V, 12);
                __syncthreads();
                if (tid == 0) epnp_candidates(L);
                __syncthreads();
                // the summed squared reprojection error of each candidate over the inliers
                for (int k = 0; k < 3; k++) acc[k] = 0.0;
                for (int i = tid; i < n; i += blockDim.x) {
                    if (!mask0[i]) continue;
                    for (int k = 0; k < 3; k++) {
                        if (!L.valid[k]) continue;
                        double zc;
                        const double e2 = reproj2(L.cand[k], s.X[i], s.Y[i], s.Z[i], s.x[i], s.y[i], fx, fy, &zc);
                        acc[k] += zc > 0.0 ? e2 : INFINITY;
                    }
                }
                ordered_sum<3>(acc, L);
                if (tid == 0) {
                    int best = 0;
                    double be = INFINITY;
                    for (int k = 0; k < 3; k++)
                        if (L.valid[k] && L.sum[k] < be) { best = k + 1; be = L.sum[k]; }
                    L.best = best;
                }
                __syncthreads();
                const int best = L.best;
                if (best) {                              // uniform
                    const int cn = pnp_score_mask(L.cand[best - 1], s, n, fx, fy, thr2, mask1, L.red);
                    if (cn >= count) {
                        count = cn; kept = 1; beta_case = best; cur = mask1;
                        if (tid < 12) L.Rt[tid] = L.cand[best - 1][tid];
                    }
                    __syncthreads();
                }
            }
        }
    }
    const int base = write_inliers(ok, n, max_n, cur, d_inlier, d_inlier_index);
    if (tid < 16) {
        const int r = tid >> 2, c = tid & 3;
        d_pose[tid] = r < 3 ? (float)L.Rt[4 * r + c] : (c == 3 ? 1.f : 0.f);
    }
    if (tid < 12) st->Rt[tid] = L.Rt[tid];
    if (tid == 0) {
        const int status = nfin < 4 ? RANSAC_STATUS_FEW : (ok ? RANSAC_STATUS_OK : RANSAC_STATUS_FAILED);
        *d_inlier_count = base;
        *d_status = status;
        st->status = status; st->refit_kept = kept; st->beta_case = beta_case; st->inliers = base;
        st->nfin = nfin;
        st->nfin_acc = 0;
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
static void pnp_layout(rs_pnp_estimator* e, rs_carve& c)
{
    const size_t m = e->max_points;
    e->x = c.take<double>(5 * m);
    e->fin = c.take<uint8_t>(m);
    e->mask = c.take<uint8_t>(2 * m);
    e->st = c.take<PnpState>(1);
}

extern "C" int rs_pnp_estimator_create(rs_context* ctx, int max_points, int max_hypotheses, rs_pnp_estimator** out)
{
    return ransac_create(ctx, max_points, max_hypotheses, out, 4, 4, 12, "pnp estimator scratch", pnp_layout);
}

extern "C" int rs_pnp_estimator_destroy(rs_pnp_estimator* e) { return rs_drain_and_delete(e); }

extern "C" int rs_estimate_pose_pnp(rs_context* ctx, rs_pnp_estimator* e, const float* d_object, const int32_t* d_object_index,
                                    const float* d_pixels, const int32_t* d_pixel_index, const int32_t* d_count, int max_n,
                                    const float* h_intrinsics, double threshold_px, double confidence, int max_hypotheses,
                                    uint64_t seed, float* d_pose, uint8_t* d_inlier, int32_t* d_inlier_index,
                                    int32_t* d_inlier_count, int32_t* d_status)
{
    int rc = ransac_check_call(ctx, e, d_object, d_pixels, max_n, h_intrinsics, d_pose, d_inlier, d_inlier_index, d_inlier_count,
                               d_status);
    if (!rc) rc = ransac_check_options(ctx, e, d_count, max_hypotheses, threshold_px, confidence);
    if (rc) return rc;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const float* K = h_intrinsics;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], thr2 = threshold_px * threshold_px;
    const PnpScratch s = scratch_of(e);
    hipStream_t st = ctx->stream;
    const int blocks = ransac_blocks(max_n, e->max_hyp);
    {
        rs_prof_scope ps(ctx, "PNP0_prep");
        hipLaunchKernelGGL(pnp_prep, dim3(blocks), dim3(256), 0, st, d_object, d_object_index, (const float2*)d_pixels,
                           d_pixel_index, d_count, max_n, fx, fy, cx, cy, e->max_hyp, s);
    }
    const unsigned long long seed_hash = splitmix64(seed);
    const double log1mconf = std::log(1.0 - confidence);
    const int rounds = (max_hypotheses + RANSAC_ROUND - 1) / RANSAC_ROUND;
    for (int r = 0; r < rounds; r++) {
        const int nh = std::min(RANSAC_ROUND, max_hypotheses - r * RANSAC_ROUND);
        {
            rs_prof_scope ps(ctx, "PNP1_hyp");
            hipLaunchKernelGGL(pnp_hyp, dim3((nh + 63) / 64), dim3(64), 0, st, r, max_hypotheses, seed_hash, s);
        }
        {
            rs_prof_scope ps(ctx, "PNP2_score");
            hipLaunchKernelGGL(pnp_score, dim3(nh), dim3(256), 0, st, r, max_hypotheses, fx, fy, thr2, s);
        }
        hipLaunchKernelGGL(pnp_stop_k, dim3(1), dim3(64), 0, st, r, max_hypotheses, log1mconf, e->st);
    }
    {
        rs_prof_scope ps(ctx, "PNP3_final");
        hipLaunchKernelGGL(pnp_final, dim3(1), dim3(256), 0, st, max_n, fx, fy, thr2, s, e->mask, e->mask + e->max_points, d_pose,
                           d_inlier, d_inlier_index, d_inlier_count, d_status);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_pnp_estimator_stats(rs_context* ctx, const rs_pnp_estimator* e, int32_t* h_stats, double* h_pose)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!e) return rs_fail(ctx, RS_ERR_INVALID, "null estimator");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    PnpState st;
    RS_HIP(ctx, hipMemcpyAsync(&st, e->st, sizeof(PnpState), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_stats) {
        const int v[9] = {st.r.drawn, st.r.scored, st.r.best_index, st.r.best_count, st.refit_kept, st.beta_case, st.status, st.inliers,
                          st.r.n};
        memcpy(h_stats, v, sizeof(v));
    }
    if (h_pose) memcpy(h_pose, st.Rt, sizeof(st.Rt));
    return RS_OK;
}

extern "C" int rs_pnp_hypotheses(rs_context* ctx, const rs_pnp_estimator* e, int32_t* h_samples, int32_t* h_nmodels,
                                 double* h_models, int32_t* h_scores)
{
    return ransac_table_download(ctx, e, 4, 4, 12, h_samples, h_nmodels, h_models, h_scores);
}
