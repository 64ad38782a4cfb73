// pose.hip — the relative-pose stage: five-point essential-matrix RANSAC and the known-rotation translation RANSAC.
//
// Replaces pose::estimate_pose (reference src/PoseEstimation.cpp:59-88 with recover_pose_from_essential, :23-57) and
// pose::estimate_pose_with_known_rotation (:110-227).  The specification is tests/essential_ref.py; this file follows
// it operation by operation (-ffp-contract=off), so sampling, model sets and scores agree with it to rounding.
//
// rs_estimate_pose: one stream-ordered chain, no host synchronisation; the point count is read on the device.  The
// RANSAC frame (draw, table, key, stop, inlier compaction) is ransac.h's with S = 5, M = 10, D = 9; this file adds:
//   pose_prep     gather (through an optional index) + normalise into f64 SoA scratch; reset the state and the table
//   pose_hyp      one wave64 workgroup per hypothesis: the sample (lane 0, into LDS), the 5 x 9 null space (Gauss-Jordan,
//                 lanes per row, Gram-Schmidt), the 10 x 20 cubic constraints (lanes per row), Gauss-Jordan, B(z) and its
//                 degree-10 determinant and derivative table (lane 0), bisection and Newton (one lane per root), models
//   pose_score    one workgroup per hypothesis: integer Sampson inlier counts of its models, the key's atomicMax
//   pose_stop_k   the adaptive stop after each round of 256; later rounds exit at entry
//   pose_final    one workgroup: LO (8-point refits with a fixed reduction order), decomposition, the final inlier mask
//   pose_cheir    4 candidates x point chunks: tri_core.h's DLT and gates, integer counts
//   pose_choose   the first strict maximum; the f32 pose
// rs_estimate_pose_known_rotation: kr_prep, kr_support (one workgroup per pair), kr_final (one workgroup), on the same
// table (slot = the pair's number) with the same key and compaction; its pairs come from the caller, so no draw, no stop.
// No float atomics: two calls with the same inputs write the same bytes.
#include "pose_shared.h"
#include "tri_core.h"

#define POSE_PIVOT_EPS 1e-12
// The real roots of the degree-10 determinant (tests/essential_ref.real_roots): a leading coefficient below
// POSE_TRIM_EPS of the largest is dropped (roots beyond ~1e30); the roots of p's derivatives isolate those of p, level by
// level, and each isolated root takes POSE_BISECT_ITERS halvings of its interval's ordered 64-bit keys (any f64 interval
// closes to two adjacent doubles, whatever the root's magnitude), then POSE_NEWTON guarded Newton steps.  A model is
// kept only if its unit-norm E satisfies max |2 E E^T E - tr(E E^T) E| <= POSE_ESS_EPS.
#define POSE_ESS_EPS 1e-6
#define POSE_LO_ROUNDS 4

struct PoseState {
    RansacState r;
    int status, lo_kept, chosen, inliers;
    int cheir[4];
    int known;                             // 1 after rs_estimate_pose_known_rotation
    double E[9];
    float cand[4][16];
    float pose[16];
};

struct rs_pose_estimator : RansacEstimator {         // t: samples [max_hyp][5], models [max_hyp][10][9], scores [max_hyp][10]
    double* x = nullptr;            // [4][max_points] x1, y1, x2, y2
    float2* pix = nullptr;          // [2][max_points] gathered from / to pixels
    uint8_t* fin = nullptr;         // [max_points]
    uint8_t* mask = nullptr;        // [2][max_points] LO masks
    float* rays = nullptr;          // [9][max_points] known rotation: from, to, constraint
    PoseState* st = nullptr;
};

__constant__ int POSE_T11[4][4] = {{0, 3, 4, 6}, {3, 1, 5, 7}, {4, 5, 2, 8}, {6, 7, 8, 9}};
__constant__ int POSE_T21[10][4] = {{0, 2, 4, 5}, {3, 1, 6, 7}, {10, 13, 16, 17}, {2, 3, 8, 9}, {4, 8, 10, 11},
                                    {8, 6, 13, 14}, {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// ------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ double sampson2(const double* e, double x1, double y1, double x2, double y2)
{
    const double ex0 = (e[0] * x1 + e[1] * y1) + e[2];
    const double ex1 = (e[3] * x1 + e[4] * y1) + e[5];
    const double ex2 = (e[6] * x1 + e[7] * y1) + e[8];
    const double et0 = (e[0] * x2 + e[3] * y2) + e[6];
    const double et1 = (e[1] * x2 + e[4] * y2) + e[7];
    const double num = (x2 * ex0 + y2 * ex1) + ex2;
    const double den = ((ex0 * ex0 + ex1 * ex1) + et0 * et0) + et1 * et1;
    return num * num / den;
}

// one wave (the whole workgroup, 64 lanes): Gauss-Jordan with partial pivoting of A [R][C] in LDS on columns
// 0 .. npiv-1.  false = rank deficient / non-finite.
__device__ bool wave_gauss_jordan(double* A, int R, int C, int npiv, int lane)
{
    double m = 0.0;
    int nonfinite = 0;
    for (int i = lane; i < R * C; i += 64) {
        const double a = fabs(A[i]);
        if (!isfinite(a)) nonfinite = 1;
        m = a > m ? a : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
        nonfinite |= __shfl_xor(nonfinite, off, 64);
    }
    if (nonfinite || m == 0.0) return false;
    for (int c = 0; c < npiv; c++) {
        int p = c;
        double best = fabs(A[c * C + c]);
        for (int r = c + 1; r < R; r++) {
            const double a = fabs(A[r * C + c]);
            if (a > best) { best = a; p = r; }
        }
        __syncthreads();
        if (p != c && lane < C) {
            const double t = A[c * C + lane];
            A[c * C + lane] = A[p * C + lane];
            A[p * C + lane] = t;
        }
        __syncthreads();
        const double piv = A[c * C + c];
        if (!(fabs(piv) > POSE_PIVOT_EPS * m)) return false;      // uniform across the wave
        __syncthreads();
        if (lane < C) A[c * C + lane] = A[c * C + lane] / piv;
        __syncthreads();
        if (lane < R && lane != c) {
            const double f = A[lane * C + c];
            for (int j = 0; j < C; j++) A[lane * C + j] = A[lane * C + j] - f * A[c * C + j];
        }
        __syncthreads();
    }
    return true;
}

__device__ __forceinline__ void mul11(const double* a, const double* b, double* out)
{
    for (int k = 0; k < 10; k++) out[k] = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[POSE_T11[i][j]] = out[POSE_T11[i][j]] + a[i] * b[j];
}

__device__ __forceinline__ void mul21(const double* a, const double* b, double* out)
{
    for (int k = 0; k < 20; k++) out[k] = 0.0;
    for (int i = 0; i < 10; i++)
        for (int j = 0; j < 4; j++) out[POSE_T21[i][j]] = out[POSE_T21[i][j]] + a[i] * b[j];
}

// ------------------------------------------------------------------------------------------------ rs_estimate_pose
struct PoseScratch {
    double *x1, *y1, *x2, *y2;
    float2 *pf, *pt;
    uint8_t* fin;
    RansacTable t;
    PoseState* st;
};

static PoseScratch scratch_of(const rs_pose_estimator* e)
{
    const size_t m = e->max_points;
    return PoseScratch{e->x, e->x + m, e->x + 2 * m, e->x + 3 * m, e->pix, e->pix + m, e->fin, e->t, e->st};
}

__global__ __launch_bounds__(256) void pose_prep(const float2* __restrict__ from, const int32_t* __restrict__ from_index,
                                                 const float2* __restrict__ to, const int32_t* __restrict__ d_count, int max_n,
                                                 double fx, double fy, double cx, double cy, int table_hyp, PoseScratch s)
{
    const int n = min(max(*d_count, 0), max_n);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = tid; i < n; i += stride) {
        const int j = from_index ? from_index[i] : i;
        const float2 a = j >= 0 ? from[j] : make_float2(NAN, NAN), b = to[i];
        const double x1 = ((double)a.x - cx) / fx, y1 = ((double)a.y - cy) / fy;
        const double x2 = ((double)b.x - cx) / fx, y2 = ((double)b.y - cy) / fy;
        const bool f = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
        s.x1[i] = f ? x1 : 0.0; s.y1[i] = f ? y1 : 0.0; s.x2[i] = f ? x2 : 0.0; s.y2[i] = f ? y2 : 0.0;
        s.pf[i] = a; s.pt[i] = b;
        s.fin[i] = f ? 1 : 0;
    }
    ransac_reset_table<5, 10>(s.t, table_hyp);
    if (tid == 0) {
        PoseState* st = s.st;
        st->r = RansacState{0ull, n < 5 ? 1 : 0, 0, n, 0, -1, 0};
        st->status = n < 5 ? RANSAC_STATUS_FEW : RANSAC_STATUS_FAILED;
        st->lo_kept = 0; st->chosen = -1; st->inliers = 0;
        st->cheir[0] = st->cheir[1] = st->cheir[2] = st->cheir[3] = 0;
        st->known = 0;
        for (int k = 0; k < 9; k++) st->E[k] = 0.0;
    }
}

struct HypLds {
    double A[10 * 20];
    double N[4 * 9];
    double Ep[9][4];
    double EE[6][10];
    double minor[3][10];
    double bx[3][4], by[3][4], b1[3][5];
    double D[11 * 11];                  // D[r] = the r-th derivative of the scaled determinant, ascending
    double rt[2][10];                   // the roots of the level below / of this level
    double bound;
    int deg, ok;
    int idx[5];
};

__global__ __launch_bounds__(64) void pose_hyp(int round, int max_hyp, unsigned long long seed_hash, PoseScratch s)
{
    __shared__ HypLds L;
    const int lane = threadIdx.x;
    const int h = round * RANSAC_ROUND + blockIdx.x;
    if (s.st->r.stop || h >= max_hyp) return;
    if (lane == 0) L.ok = ransac_draw<5>(seed_hash, h, s.st->r.n, s.fin, L.idx);
    __syncthreads();
    if (!L.ok) {
        if (lane == 0) s.t.nmod[h] = 0;
        return;
    }
    if (lane < 5) s.t.samples[5 * h + lane] = L.idx[lane];
    if (lane < 45) {                                  // Q [5][9]
        const int r = lane / 9, c = lane - 9 * r, i = L.idx[r];
        const double x1 = s.x1[i], y1 = s.y1[i], x2 = s.x2[i], y2 = s.y2[i];
        const double v[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
        L.A[lane] = v[c];
    }
    __syncthreads();
    bool good = wave_gauss_jordan(L.A, 5, 9, 5, lane);
    if (good) {
        if (lane < 36) {
            const int j = lane / 9, k = lane - 9 * j;
            L.N[lane] = k == 5 + j ? 1.0 : (k < 5 ? -L.A[k * 9 + 5 + j] : 0.0);
        }
        __syncthreads();
        for (int j = 0; j < 4; j++) {                 // modified Gram-Schmidt
            for (int i = 0; i < j; i++) {
                double d = 0.0;
                for (int k = 0; k < 9; k++) d = d + L.N[9 * i + k] * L.N[9 * j + k];
                __syncthreads();
                if (lane < 9) L.N[9 * j + lane] = L.N[9 * j + lane] - d * L.N[9 * i + lane];
                __syncthreads();
            }
            double nn = 0.0;
            for (int k = 0; k < 9; k++) nn = nn + L.N[9 * j + k] * L.N[9 * j + k];
            __syncthreads();
            if (lane < 9) L.N[9 * j + lane] = L.N[9 * j + lane] / sqrt(nn);
            __syncthreads();
        }
        if (lane < 36) L.Ep[lane >> 2][lane & 3] = L.N[9 * (lane & 3) + (lane >> 2)];
        __syncthreads();
        if (lane < 6) {                               // E E^T (i <= j)
            const int i = lane < 3 ? 0 : (lane < 5 ? 1 : 2);
            const int j = lane < 3 ? lane : (lane < 5 ? lane - 2 : 2);
            double t0[10], t1[10], t2[10];
            mul11(L.Ep[3 * i], L.Ep[3 * j], t0);
            mul11(L.Ep[3 * i + 1], L.Ep[3 * j + 1], t1);
            mul11(L.Ep[3 * i + 2], L.Ep[3 * j + 2], t2);
            for (int k = 0; k < 10; k++) L.EE[lane][k] = (t0[k] + t1[k]) + t2[k];
        } else if (lane < 9) {                        // the 2 x 2 minors of the determinant
            const int m = lane - 6;
            const int a0 = m == 0 ? 4 : 3, a1 = m == 2 ? 7 : 8, b0 = m == 0 ? 5 : (m == 1 ? 5 : 4), b1 = m == 0 ? 7 : 6;
            double t0[10], t1[10];
            mul11(L.Ep[a0], L.Ep[a1], t0);
            mul11(L.Ep[b0], L.Ep[b1], t1);
            for (int k = 0; k < 10; k++) L.minor[m][k] = t0[k] - t1[k];
        }
        __syncthreads();
        if (lane < 10) {
            double row[20];
            if (lane == 0) {
                double t0[20], t1[20], t2[20];
                mul21(L.minor[0], L.Ep[0], t0);
                mul21(L.minor[1], L.Ep[1], t1);
                mul21(L.minor[2], L.Ep[2], t2);
                for (int k = 0; k < 20; k++) row[k] = (t0[k] - t1[k]) + t2[k];
            } else {
                const int i = (lane - 1) / 3, j = (lane - 1) % 3;
                auto ee = [&](int a, int b) -> const double* {
                    const int lo = a < b ? a : b, hi = a < b ? b : a;
                    return L.EE[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
                };
                double tr[10], t0[20], t1[20], t2[20], t3[20];
                for (int k = 0; k < 10; k++) tr[k] = (L.EE[0][k] + L.EE[3][k]) + L.EE[5][k];
                mul21(ee(i, 0), L.Ep[j], t0);
                mul21(ee(i, 1), L.Ep[3 + j], t1);
                mul21(ee(i, 2), L.Ep[6 + j], t2);
                mul21(tr, L.Ep[3 * i + j], t3);
                for (int k = 0; k < 20; k++) row[k] = ((t0[k] + t1[k]) + t2[k]) * 2.0 - t3[k];
            }
            for (int k = 0; k < 20; k++) L.A[20 * lane + k] = row[k];
        }
        __syncthreads();
        good = wave_gauss_jordan(L.A, 10, 20, 10, lane);
    }
    if (lane == 0) {
        L.deg = 0;
        if (good) {
            // B(z): rows (4, 5), (6, 7), (8, 9) of the reduced system
            for (int q = 0; q < 3; q++) {
                const double* ra = L.A + 20 * (4 + 2 * q) + 10;
                const double* rb = L.A + 20 * (5 + 2 * q) + 10;
                L.bx[q][0] = ra[2]; L.bx[q][1] = ra[1] - rb[2]; L.bx[q][2] = ra[0] - rb[1]; L.bx[q][3] = -rb[0];
                L.by[q][0] = ra[5]; L.by[q][1] = ra[4] - rb[5]; L.by[q][2] = ra[3] - rb[4]; L.by[q][3] = -rb[3];
                L.b1[q][0] = ra[9]; L.b1[q][1] = ra[8] - rb[9]; L.b1[q][2] = ra[7] - rb[8]; L.b1[q][3] = ra[6] - rb[7];
                L.b1[q][4] = -rb[6];
            }
            double t0[8], t1[8], c0[8], c1[8], c2[7], p[11], u0[11], u1[11], u2[11];
            pmul(L.by[1], 4, L.b1[2], 5, t0); pmul(L.b1[1], 5, L.by[2], 4, t1);
            for (int k = 0; k < 8; k++) c0[k] = t0[k] - t1[k];
            pmul(L.bx[1], 4, L.b1[2], 5, t0); pmul(L.b1[1], 5, L.bx[2], 4, t1);
            for (int k = 0; k < 8; k++) c1[k] = t0[k] - t1[k];
            pmul(L.bx[1], 4, L.by[2], 4, t0); pmul(L.by[1], 4, L.bx[2], 4, t1);
            for (int k = 0; k < 7; k++) c2[k] = t0[k] - t1[k];
            pmul(L.bx[0], 4, c0, 8, u0); pmul(L.by[0], 4, c1, 8, u1); pmul(L.b1[0], 5, c2, 7, u2);
            for (int k = 0; k < 11; k++) p[k] = (u0[k] - u1[k]) + u2[k];
            // scaled, trimmed; the derivative table and the root bound (tests/essential_ref.real_roots)
            double m = 0.0;
            for (int k = 0; k < 11; k++) m = fmax(m, fabs(p[k]));
            if (m > 0.0 && isfinite(m)) {
                for (int k = 0; k < 11; k++) p[k] = p[k] / m;
                int d = 10;
                while (d > 0 && fabs(p[d]) < POSE_TRIM_EPS) d--;
                for (int k = d + 1; k < 11; k++) p[k] = 0.0;
                for (int k = 0; k < 11; k++) L.D[k] = p[k];
                for (int r = 0; r < 10; r++) {
                    for (int k = 0; k < 10; k++) L.D[11 * (r + 1) + k] = (double)(k + 1) * L.D[11 * r + k + 1];
                    L.D[11 * (r + 1) + 10] = 0.0;
                }
                double bnd = 0.0;
                for (int k = 0; k < d; k++) bnd = fmax(bnd, fabs(p[k] / p[d]));
                L.bound = 1.0 + bnd;
                L.deg = d;
            }
        }
    }
    __syncthreads();
    // level j = 1 .. d: the roots of D[d - j] (degree j), one lane per interval between the roots of the level below
    const int deg = L.deg;
    const double B = L.bound;
    int nroot = 0;
    for (int j = 1; j <= deg; j++) {
        const double* q = L.D + 11 * (deg - j);
        const double* rt = L.rt[(j - 1) & 1];
        bool has = false;
        double z = 0.0;
        if (lane <= nroot) {
            const double a = lane == 0 ? -B : rt[lane - 1], b = lane == nroot ? B : rt[lane];
            const int sa = poly_sign(q, j, a), sb = poly_sign(q, j, b);
            if (sa != 0 && sb != sa) {
                has = true;
                long long lo = dkey(a), hi = dkey(b);
                for (int it = 0; it < POSE_BISECT_ITERS; it++) {
                    const long long mid = ((lo >> 1) + (hi >> 1)) + (lo & hi & 1ll);
                    if (poly_sign(q, j, dunkey(mid)) == sa) lo = mid; else hi = mid;
                }
                z = dunkey(hi);
            }
        }
        const unsigned long long hb = __ballot(has);
        if (has) L.rt[j & 1][__popcll(hb & ((1ull << lane) - 1ull))] = z;
        nroot = __popcll(hb);
        __syncthreads();
    }
    bool valid = false;
    double e[9];
    if (lane < nroot) {                               // one lane per root: the (lane + 1)-th smallest
        double z = L.rt[deg & 1][lane];
        for (int it = 0; it < POSE_NEWTON; it++) {
            double v = 0.0, dv = 0.0;
            for (int c = 10; c >= 0; c--) {
                dv = dv * z + v;
                v = v * z + L.D[c];
            }
            const double zn = z - v / dv;
            if (dv != 0.0 && isfinite(zn) && fabs(zn - z) <= 1e-6 * (1.0 + fabs(z))) z = zn;
        }
        double rows[3][3];
        for (int i = 0; i < 3; i++) {
            rows[i][0] = horner_up(L.bx[i], 4, z);
            rows[i][1] = horner_up(L.by[i], 4, z);
            rows[i][2] = horner_up(L.b1[i], 5, z);
        }
        double best[3] = {0, 0, 0}, bn = -1.0;
        for (int pr = 0; pr < 3; pr++) {
            const int a = pr == 2 ? 1 : 0, b = pr == 0 ? 1 : 2;
            double v[3];
            cross3(rows[a], rows[b], v);
            const double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
            if (n2 > bn) { bn = n2; best[0] = v[0]; best[1] = v[1]; best[2] = v[2]; }
        }
        if (fabs(best[2]) > POSE_PIVOT_EPS * sqrt(bn)) {
            const double x = best[0] / best[2], y = best[1] / best[2];
            double nn = 0.0;
            for (int i = 0; i < 9; i++) {
                e[i] = ((x * L.N[i] + y * L.N[9 + i]) + z * L.N[18 + i]) + L.N[27 + i];
                nn = nn + e[i] * e[i];
            }
            nn = sqrt(nn);
            if (nn > 0.0 && isfinite(nn)) {
                for (int i = 0; i < 9; i++) e[i] = e[i] / nn;
                // the essential-matrix identity (tests/essential_ref.essential_residual): a model that fails it is dropped
                double EE[9], res = 0.0;
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++) EE[3 * a + b] = (e[3 * a] * e[3 * b] + e[3 * a + 1] * e[3 * b + 1]) + e[3 * a + 2] * e[3 * b + 2];
                const double tr = (EE[0] + EE[4]) + EE[8];
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++) {
                        const double v = ((EE[3 * a] * e[b] + EE[3 * a + 1] * e[3 + b]) + EE[3 * a + 2] * e[6 + b]) * 2.0 - tr * e[3 * a + b];
                        res = fmax(res, fabs(v));
                    }
                valid = res <= POSE_ESS_EPS;
            }
        }
    }
    const unsigned long long bal = __ballot(valid);
    if (valid) {
        const int slot = __popcll(bal & ((1ull << lane) - 1ull));
        double* out = s.t.models + 90 * (size_t)h + 9 * slot;
        for (int i = 0; i < 9; i++) out[i] = e[i];
    }
    if (lane == 0) s.t.nmod[h] = __popcll(bal);
}

__global__ __launch_bounds__(256) void pose_score(int round, int max_hyp, double thr2, PoseScratch s)
{
    __shared__ int red[4];
    const int h = round * RANSAC_ROUND + blockIdx.x;
    if (s.st->r.stop || h >= max_hyp) return;
    const int nm = s.t.nmod[h], n = s.st->r.n;
    for (int m = 0; m < nm; m++) {
        double e[9];
        const double* src = s.t.models + 90 * (size_t)h + 9 * m;
#pragma unroll
        for (int i = 0; i < 9; i++) e[i] = src[i];
        int c = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            c += (s.fin[i] && sampson2(e, s.x1[i], s.y1[i], s.x2[i], s.y2[i]) < thr2) ? 1 : 0;
        c = block_sum_int(c, red);
        if (threadIdx.x == 0) {
            s.t.scores[10 * h + m] = c;
            atomicMax(&s.st->r.best_key, ransac_key(c, 10 * h + m));
            atomicAdd(&s.st->r.scored, 1);
        }
    }
}

__global__ __launch_bounds__(64) void pose_stop_k(int round, int max_hyp, double log1mconf, PoseState* st)
{
    if (threadIdx.x != 0 || st->r.stop) return;
    ransac_stop<5>(&st->r, round, max_hyp, log1mconf);
}

// score E into mask (for i < n), returns the count (all threads)
__device__ __forceinline__ int score_mask(const double* e, const PoseScratch& s, int n, double thr2, uint8_t* mask, int* red)
{
    int c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const bool in = s.fin[i] && sampson2(e, s.x1[i], s.y1[i], s.x2[i], s.y2[i]) < thr2;
        mask[i] = in ? 1 : 0;
        c += in ? 1 : 0;
    }
    return block_sum_int(c, red);
}

struct FinalLds {
    double E[9], En[9];
    double A[81], V[81];
    double part[4][45];
    int red[4];
    int cnt, stop;
};

__global__ __launch_bounds__(256) void pose_final(int max_n, double thr2, PoseScratch s, uint8_t* __restrict__ mask0,
                                                  uint8_t* __restrict__ mask1, uint8_t* __restrict__ d_inlier,
                                                  int32_t* __restrict__ d_inlier_index, int32_t* __restrict__ d_inlier_count)
{
    __shared__ FinalLds L;
    PoseState* st = s.st;
    const int n = st->r.n, tid = threadIdx.x;
    const unsigned long long key = st->r.best_key;
    const int best_count = ransac_key_count(key);
    const bool ok = n >= 5 && best_count >= 5;
    uint8_t* cur = mask0;
    uint8_t* nxt = mask1;
    int count = 0;
    if (ok) {
        const int bi = ransac_key_slot(key);
        if (tid < 9) L.E[tid] = s.t.models[90 * (size_t)(bi / 10) + 9 * (bi % 10) + tid];
        if (tid == 0) { st->r.best_index = bi; st->r.best_count = best_count; }
        __syncthreads();
        count = score_mask(L.E, s, n, thr2, cur, L.red);
        int kept = 0;
        for (int r = 0; r < POSE_LO_ROUNDS && count >= 8; r++) {
            double acc[45];
#pragma unroll
            for (int k = 0; k < 45; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += blockDim.x) {
                if (!cur[i]) continue;
                const double x1 = s.x1[i], y1 = s.y1[i], x2 = s.x2[i], y2 = s.y2[i];
                const double q[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
                int k = 0;
#pragma unroll
                for (int a = 0; a < 9; a++)
#pragma unroll
                    for (int b = a; b < 9; b++) acc[k++] += q[a] * q[b];
            }
#pragma unroll
            for (int k = 0; k < 45; k++) acc[k] = wave_sum_f64(acc[k]);
            if ((tid & 63) == 0)
                for (int k = 0; k < 45; k++) L.part[tid >> 6][k] = acc[k];
            __syncthreads();
            if (tid == 0) {
                int k = 0;
                for (int a = 0; a < 9; a++)
                    for (int b = a; b < 9; b++, k++) {
                        const double v = ((L.part[0][k] + L.part[1][k]) + L.part[2][k]) + L.part[3][k];
                        L.A[9 * a + b] = v;
                        L.A[9 * b + a] = v;
                    }
            }
            __syncthreads();
            jacobi_eigen_block(L.A, L.V, 9);
            if (tid == 0) {
                const int j = smallest_diag(L.A, 9);
                double f[9], U[9], W[9];
                for (int i = 0; i < 9; i++) f[i] = L.V[9 * i + j];
                svd3(f, U, W);
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++) L.En[3 * a + b] = U[3 * a] * W[3 * b] + U[3 * a + 1] * W[3 * b + 1];
            }
            __syncthreads();
            const int cn = score_mask(L.En, s, n, thr2, nxt, L.red);
            if (cn < count) break;                    // uniform
            count = cn;
            kept++;
            if (tid < 9) L.E[tid] = L.En[tid];
            uint8_t* t = cur; cur = nxt; nxt = t;
            __syncthreads();
        }
        if (tid == 0) {
            st->lo_kept = kept;
            double U[9], W[9], Vt[9], R1[9], R2[9];
            svd3(L.E, U, W);
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) Vt[3 * a + b] = W[3 * b + a];
            if (det3(U) < 0.0)
                for (int i = 0; i < 9; i++) U[i] = -U[i];
            if (det3(Vt) < 0.0)
                for (int i = 0; i < 9; i++) Vt[i] = -Vt[i];
            const double Wm[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
            double UW[9], UWt[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    UW[3 * a + b] = (U[3 * a] * Wm[b] + U[3 * a + 1] * Wm[3 + b]) + U[3 * a + 2] * Wm[6 + b];
                    UWt[3 * a + b] = (U[3 * a] * Wm[3 * b] + U[3 * a + 1] * Wm[3 * b + 1]) + U[3 * a + 2] * Wm[3 * b + 2];
                }
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    R1[3 * a + b] = (UW[3 * a] * Vt[b] + UW[3 * a + 1] * Vt[3 + b]) + UW[3 * a + 2] * Vt[6 + b];
                    R2[3 * a + b] = (UWt[3 * a] * Vt[b] + UWt[3 * a + 1] * Vt[3 + b]) + UWt[3 * a + 2] * Vt[6 + b];
                }
            for (int c = 0; c < 4; c++) {
                const double* R = c < 2 ? R1 : R2;
                const double sg = (c & 1) ? -1.0 : 1.0;
                float* P = st->cand[c];
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) P[4 * a + b] = (float)R[3 * a + b];
                    P[4 * a + 3] = (float)(U[3 * a + 2] * sg);
                }
                P[12] = 0.f; P[13] = 0.f; P[14] = 0.f; P[15] = 1.f;
            }
            for (int i = 0; i < 9; i++) st->E[i] = L.E[i];
            st->status = RANSAC_STATUS_OK;
            st->inliers = count;
        }
    }
    const int base = write_inliers(ok, n, max_n, cur, d_inlier, d_inlier_index);
    if (tid == 0) *d_inlier_count = base;
}

__global__ __launch_bounds__(256) void pose_cheir(TriParams prm, PoseScratch s)
{
    __shared__ int red[4];
    const PoseState* st = s.st;
    if (st->status != RANSAC_STATUS_OK) return;
    const int n = st->r.n, c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x * blockDim.x >= n) return;         // uniform per workgroup
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float T[16];
#pragma unroll
    for (int k = 0; k < 16; k++) T[k] = st->cand[c][k];
    int keep = 0;
    if (i < n && s.fin[i]) {
        float X[3];
        keep = dlt_one(s.pf[i], s.pt[i], I, T, prm, X) ? 1 : 0;
    }
    keep = block_sum_int(keep, red);
    if (threadIdx.x == 0 && keep) atomicAdd(&s.st->cheir[c], keep);
}

__global__ void pose_choose(PoseState* st, float* __restrict__ d_pose, int32_t* __restrict__ d_status)
{
    if (threadIdx.x != 0) return;
    float P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (st->status == RANSAC_STATUS_OK) {
        int best = 0, most = 0;
        for (int c = 0; c < 4; c++)
            if (st->cheir[c] > most) { most = st->cheir[c]; best = c; }
        st->chosen = best;
        for (int k = 0; k < 16; k++) P[k] = st->cand[best][k];
    }
    for (int k = 0; k < 16; k++) { d_pose[k] = P[k]; st->pose[k] = P[k]; }
    *d_status = st->status;
}

// ------------------------------------------------------------------------------------------------ known rotation
struct KrScratch {
    float *fr, *to, *cons;          // [n][3] each
    float2 *pf, *pt;
    RansacTable t;
    PoseState* st;
};

__device__ __forceinline__ void matvec3f(const float* M, const float* v, float* o)
{
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}

__device__ __forceinline__ void cross3f(const float* a, const float* b, float* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

struct Rot9 { float r[9]; };

// [t]x R, (tx_i0 R_0j + tx_i1 R_1j) + tx_i2 R_2j
__device__ __forceinline__ void essential_tr(const float* t, const float* R, float* E)
{
    const float tx[9] = {0.0f, -t[2], t[1], t[2], 0.0f, -t[0], -t[1], t[0], 0.0f};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) E[3 * i + j] = (tx[3 * i] * R[j] + tx[3 * i + 1] * R[3 + j]) + tx[3 * i + 2] * R[6 + j];
}

__device__ __forceinline__ float epipolar_error_f(const float* E, const float* fr, const float* to, float focal)
{
    float lt[3], lf[3];
    matvec3f(E, fr, lt);
    const float Et[9] = {E[0], E[3], E[6], E[1], E[4], E[7], E[2], E[5], E[8]};
    matvec3f(Et, to, lf);
    const float den = (lt[0] * lt[0] + lt[1] * lt[1]) + (lf[0] * lf[0] + lf[1] * lf[1]);
    if (den < 1e-12f) return 3.402823466e38f;
    const float num = (to[0] * lt[0] + to[1] * lt[1]) + to[2] * lt[2];
    return (focal * fabsf(num)) / sqrtf(den);
}

__global__ __launch_bounds__(256) void kr_prep(const float2* __restrict__ from, const int32_t* __restrict__ from_index,
                                               const float2* __restrict__ to, int n, float fx, float fy, float cx, float cy,
                                               Rot9 R, int table_hyp, KrScratch s)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = tid; i < n; i += stride) {
        const int j = from_index ? from_index[i] : i;
        const float2 a = j >= 0 ? from[j] : make_float2(NAN, NAN), b = to[i];
        const float f[3] = {(a.x - cx) / fx, (a.y - cy) / fy, 1.0f}, t[3] = {(b.x - cx) / fx, (b.y - cy) / fy, 1.0f};
        float rf[3], c[3];
        matvec3f(R.r, f, rf);
        cross3f(rf, t, c);
#pragma unroll
        for (int k = 0; k < 3; k++) { s.fr[3 * i + k] = f[k]; s.to[3 * i + k] = t[k]; s.cons[3 * i + k] = c[k]; }
        s.pf[i] = a;
        s.pt[i] = b;
    }
    ransac_reset_table<5, 10>(s.t, table_hyp);
    for (int h = tid; h < table_hyp; h += stride) s.t.scores[10 * h] = -1;      // a pair's one score: -1 until it is counted
    if (tid == 0) {
        PoseState* st = s.st;
        st->r = RansacState{0ull, 1, 0, n, 0, -1, 0};
        st->status = n < 8 ? RANSAC_STATUS_FEW : RANSAC_STATUS_FAILED; st->known = 1;
        st->lo_kept = 0; st->chosen = -1; st->inliers = 0;
        st->cheir[0] = st->cheir[1] = st->cheir[2] = st->cheir[3] = 0;
        for (int k = 0; k < 9; k++) st->E[k] = 0.0;
    }
}

__global__ __launch_bounds__(256) void kr_support(const int32_t* __restrict__ pairs, int n, Rot9 R, float focal, float max_err,
                                                  KrScratch s)
{
    __shared__ int red[4];
    if (n < 8) return;
    const int it = blockIdx.x;
    const int i = pairs[2 * it], j = pairs[2 * it + 1];
    if (threadIdx.x < 2) s.t.samples[5 * it + threadIdx.x] = threadIdx.x ? j : i;
    if (threadIdx.x == 0) {
        s.t.nmod[it] = 0;
        atomicAdd(&s.st->r.drawn, 1);
    }
    if (i == j || i < 0 || j < 0 || i >= n || j >= n) return;
    float ci[3], cj[3], tr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ci[k] = s.cons[3 * i + k]; cj[k] = s.cons[3 * j + k]; }
    cross3f(ci, cj, tr);
    const float nrm = sqrtf((tr[0] * tr[0] + tr[1] * tr[1]) + tr[2] * tr[2]);
    if (nrm < 1e-9f) return;
    tr[0] = tr[0] / nrm; tr[1] = tr[1] / nrm; tr[2] = tr[2] / nrm;
    float E[9];
    essential_tr(tr, R.r, E);
    int c = 0;
    for (int k = threadIdx.x; k < n; k += blockDim.x)
        c += epipolar_error_f(E, s.fr + 3 * k, s.to + 3 * k, focal) < max_err ? 1 : 0;
    c = block_sum_int(c, red);
    if (threadIdx.x == 0) {
        s.t.scores[10 * it] = c;
        s.t.nmod[it] = 1;
        for (int k = 0; k < 3; k++) s.t.models[90 * (size_t)it + k] = (double)tr[k];
        if (c > 0) atomicMax(&s.st->r.best_key, ransac_key(c, it));
    }
}

struct KrLds {
    double part[4][6];
    double A[9], V[9];
    float t[3];
    int red[4];
};

__global__ __launch_bounds__(256) void kr_final(int max_n, Rot9 R, float focal, float max_err, TriParams prm, KrScratch s,
                                                uint8_t* __restrict__ mask, float* __restrict__ d_pose, uint8_t* __restrict__ d_inlier,
                                                int32_t* __restrict__ d_inlier_index, int32_t* __restrict__ d_inlier_count,
                                                int32_t* __restrict__ d_status)
{
    __shared__ KrLds L;
    PoseState* st = s.st;
    const int n = st->r.n, tid = threadIdx.x;
    const unsigned long long key = st->r.best_key;
    const int best_s = ransac_key_count(key);
    const bool ok = n >= 8 && best_s >= 8;
    float P[16] = {R.r[0], R.r[1], R.r[2], 0.f, R.r[3], R.r[4], R.r[5], 0.f, R.r[6], R.r[7], R.r[8], 0.f, 0.f, 0.f, 0.f, 1.f};
    if (ok) {
        const int bi = ransac_key_slot(key);
        float bt[3], E[9];
        for (int k = 0; k < 3; k++) bt[k] = (float)s.t.models[90 * (size_t)bi + k];
        essential_tr(bt, R.r, E);
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int k = tid; k < n; k += blockDim.x) {
            const bool in = epipolar_error_f(E, s.fr + 3 * k, s.to + 3 * k, focal) < max_err;
            mask[k] = in ? 1 : 0;
            if (in) {
                const double c0 = s.cons[3 * k], c1 = s.cons[3 * k + 1], c2 = s.cons[3 * k + 2];
                acc[0] += c0 * c0; acc[1] += c0 * c1; acc[2] += c0 * c2; acc[3] += c1 * c1; acc[4] += c1 * c2; acc[5] += c2 * c2;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) acc[k] = wave_sum_f64(acc[k]);
        if ((tid & 63) == 0)
            for (int k = 0; k < 6; k++) L.part[tid >> 6][k] = acc[k];
        __syncthreads();
        if (tid == 0) {
            double a[6];
            for (int k = 0; k < 6; k++) a[k] = ((L.part[0][k] + L.part[1][k]) + L.part[2][k]) + L.part[3][k];
            L.A[0] = a[0]; L.A[1] = a[1]; L.A[2] = a[2]; L.A[3] = a[1]; L.A[4] = a[3]; L.A[5] = a[4]; L.A[6] = a[2]; L.A[7] = a[4];
            L.A[8] = a[5];
            jacobi_eigen(L.A, L.V, 3);
            const int j = smallest_diag(L.A, 3);
            float t[3] = {(float)L.V[j], (float)L.V[3 + j], (float)L.V[6 + j]};
            if ((t[0] * bt[0] + t[1] * bt[1]) + t[2] * bt[2] < 0.0f) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
            L.t[0] = t[0]; L.t[1] = t[1]; L.t[2] = t[2];
            st->r.best_index = bi;
            st->r.best_count = best_s;
        }
        __syncthreads();
        const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        float Tp[16], Tm[16];
        for (int k = 0; k < 16; k++) { Tp[k] = P[k]; Tm[k] = P[k]; }
        for (int a = 0; a < 3; a++) { Tp[4 * a + 3] = L.t[a]; Tm[4 * a + 3] = -L.t[a]; }
        int fp = 0, fm = 0, cnt = 0;
        for (int k = tid; k < n; k += blockDim.x) {
            if (!mask[k]) continue;
            cnt++;
            float X[3];
            fp += dlt_one(s.pf[k], s.pt[k], I, Tp, prm, X) ? 1 : 0;
            fm += dlt_one(s.pf[k], s.pt[k], I, Tm, prm, X) ? 1 : 0;
        }
        fp = block_sum_int(fp, L.red);
        fm = block_sum_int(fm, L.red);
        cnt = block_sum_int(cnt, L.red);
        const float sg = fm > fp ? -1.0f : 1.0f;
        for (int a = 0; a < 3; a++) P[4 * a + 3] = sg * L.t[a];
        if (tid == 0) {
            st->cheir[0] = fp; st->cheir[1] = fm; st->chosen = fm > fp ? 1 : 0;
            st->status = RANSAC_STATUS_OK; st->inliers = cnt;
        }
    }
    const int base = write_inliers(ok, n, max_n, mask, d_inlier, d_inlier_index);
    if (tid == 0) {
        *d_inlier_count = base;
        for (int k = 0; k < 16; k++) { d_pose[k] = P[k]; st->pose[k] = P[k]; }
        *d_status = ok ? RANSAC_STATUS_OK : (n < 8 ? RANSAC_STATUS_FEW : RANSAC_STATUS_FAILED);
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
static void pose_layout(rs_pose_estimator* e, rs_carve& c)
{
    const size_t m = e->max_points;
    e->x = c.take<double>(4 * m);
    e->pix = c.take<float2>(2 * m);
    e->fin = c.take<uint8_t>(m);
    e->mask = c.take<uint8_t>(2 * m);
    e->rays = c.take<float>(9 * m);
    e->st = c.take<PoseState>(1);
}

extern "C" int rs_pose_estimator_create(rs_context* ctx, int max_points, int max_hypotheses, rs_pose_estimator** out)
{
    return ransac_create(ctx, max_points, max_hypotheses, out, 5, 10, 9, "pose estimator scratch", pose_layout);
}

extern "C" int rs_pose_estimator_destroy(rs_pose_estimator* e) { return rs_drain_and_delete(e); }

extern "C" int rs_estimate_pose(rs_context* ctx, rs_pose_estimator* e, const float* d_pts_from, const int32_t* d_from_index,
                                const float* d_pts_to, const int32_t* d_count, int max_n, const float* h_intrinsics,
                                double threshold_px, double confidence, int max_hypotheses, uint64_t seed, float* d_pose,
                                uint8_t* d_inlier, int32_t* d_inlier_index, int32_t* d_inlier_count, int32_t* d_status)
{
    int rc = ransac_check_call(ctx, e, d_pts_from, d_pts_to, max_n, h_intrinsics, d_pose, d_inlier, d_inlier_index, d_inlier_count,
                               d_status);
    if (!rc) rc = ransac_check_options(ctx, e, d_count, max_hypotheses, threshold_px, confidence);
    if (rc) return rc;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const double fx = h_intrinsics[0], fy = h_intrinsics[1], cx = h_intrinsics[2], cy = h_intrinsics[3];
    const double t = threshold_px / ((fx + fy) / 2.0), thr2 = t * t;
    const PoseScratch s = scratch_of(e);
    hipStream_t st = ctx->stream;
    const int pts_blocks = ransac_blocks(max_n, e->max_hyp);
    {
        rs_prof_scope ps(ctx, "POSE0_prep");
        hipLaunchKernelGGL(pose_prep, dim3(pts_blocks), dim3(256), 0, st, (const float2*)d_pts_from, d_from_index,
                           (const float2*)d_pts_to, d_count, max_n, fx, fy, cx, cy, e->max_hyp, s);
    }
    const unsigned long long seed_hash = splitmix64(seed);
    const double log1mconf = std::log(1.0 - confidence);
    const int rounds = (max_hypotheses + RANSAC_ROUND - 1) / RANSAC_ROUND;
    for (int r = 0; r < rounds; r++) {
        const int nh = std::min(RANSAC_ROUND, max_hypotheses - r * RANSAC_ROUND);
        {
            rs_prof_scope ps(ctx, "POSE1_hyp");
            hipLaunchKernelGGL(pose_hyp, dim3(nh), dim3(64), 0, st, r, max_hypotheses, seed_hash, s);
        }
        {
            rs_prof_scope ps(ctx, "POSE2_score");
            hipLaunchKernelGGL(pose_score, dim3(nh), dim3(256), 0, st, r, max_hypotheses, thr2, s);
        }
        hipLaunchKernelGGL(pose_stop_k, dim3(1), dim3(64), 0, st, r, max_hypotheses, log1mconf, e->st);
    }
    {
        rs_prof_scope ps(ctx, "POSE3_final");
        hipLaunchKernelGGL(pose_final, dim3(1), dim3(256), 0, st, max_n, thr2, s, e->mask, e->mask + e->max_points, d_inlier,
                           d_inlier_index, d_inlier_count);
    }
    {
        const TriParams prm{h_intrinsics[0], h_intrinsics[1], h_intrinsics[2], h_intrinsics[3], 0.9999f, 2.0f};
        rs_prof_scope ps(ctx, "POSE4_cheir");
        if (max_n > 0)
            hipLaunchKernelGGL(pose_cheir, dim3((max_n + 255) / 256, 4), dim3(256), 0, st, prm, s);
    }
    hipLaunchKernelGGL(pose_choose, dim3(1), dim3(64), 0, st, e->st, d_pose, d_status);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_estimate_pose_known_rotation(rs_context* ctx, rs_pose_estimator* e, const float* d_pts_from,
                                               const int32_t* d_from_index, const float* d_pts_to, int n,
                                               const float* h_intrinsics, const float* h_rotation, const int32_t* d_pairs,
                                               int n_iter, float max_epipolar_px, float* d_pose, uint8_t* d_inlier,
                                               int32_t* d_inlier_index, int32_t* d_inlier_count, int32_t* d_status)
{
    int rc = ransac_check_call(ctx, e, d_pts_from, d_pts_to, n, h_intrinsics, d_pose, d_inlier, d_inlier_index, d_inlier_count, d_status);
    if (rc) return rc;
    if (!h_rotation || !d_pairs) return rs_fail(ctx, RS_ERR_INVALID, "null rotation / pairs");
    if (n_iter < 1 || n_iter > e->max_hyp) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "n_iter 1 .. %d (the estimator's max_hypotheses)", e->max_hyp);
    if (!(max_epipolar_px > 0.f)) return rs_fail(ctx, RS_ERR_INVALID, "max_epipolar_px > 0");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    Rot9 R;
    for (int k = 0; k < 9; k++) R.r[k] = h_rotation[k];
    const size_t m = e->max_points;
    const KrScratch s{e->rays, e->rays + 3 * m, e->rays + 6 * m, e->pix, e->pix + m, e->t, e->st};
    hipStream_t st = ctx->stream;
    const float fx = h_intrinsics[0], fy = h_intrinsics[1], cx = h_intrinsics[2], cy = h_intrinsics[3];
    const int blocks = ransac_blocks(n, e->max_hyp);
    {
        rs_prof_scope ps(ctx, "POSEK0_prep");
        hipLaunchKernelGGL(kr_prep, dim3(blocks), dim3(256), 0, st, (const float2*)d_pts_from, d_from_index, (const float2*)d_pts_to,
                           n, fx, fy, cx, cy, R, e->max_hyp, s);
    }
    {
        rs_prof_scope ps(ctx, "POSEK1_support");
        hipLaunchKernelGGL(kr_support, dim3(n_iter), dim3(256), 0, st, d_pairs, n, R, fx, max_epipolar_px, s);
    }
    {
        const TriParams prm{fx, fy, cx, cy, 0.9999f, 2.0f};
        rs_prof_scope ps(ctx, "POSEK2_final");
        hipLaunchKernelGGL(kr_final, dim3(1), dim3(256), 0, st, n, R, fx, max_epipolar_px, prm, s, e->mask, d_pose, d_inlier,
                           d_inlier_index, d_inlier_count, d_status);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_pose_estimator_stats(rs_context* ctx, const rs_pose_estimator* e, int32_t* h_stats, double* h_E, float* h_candidates)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!e) return rs_fail(ctx, RS_ERR_INVALID, "null estimator");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    PoseState st;
    RS_HIP(ctx, hipMemcpyAsync(&st, e->st, sizeof(PoseState), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_stats) {
        const int v[14] = {st.r.drawn, st.r.scored, st.r.best_index, st.r.best_count, st.lo_kept, st.cheir[0], st.cheir[1], st.cheir[2],
                           st.cheir[3], st.chosen, st.status, st.inliers, st.r.n, st.known};
        memcpy(h_stats, v, sizeof(v));
    }
    if (h_E) memcpy(h_E, st.E, sizeof(st.E));
    if (h_candidates) memcpy(h_candidates, st.cand, sizeof(st.cand));
    return RS_OK;
}

extern "C" int rs_pose_hypotheses(rs_context* ctx, const rs_pose_estimator* e, int32_t* h_samples, int32_t* h_nmodels,
                                  double* h_models, int32_t* h_scores)
{
    return ransac_table_download(ctx, e, 5, 10, 9, h_samples, h_nmodels, h_models, h_scores);
}
