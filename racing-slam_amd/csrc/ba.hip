// ba.hip — local-window bundle adjustment (Levenberg-Marquardt with point-block
// Schur elimination), all in f64, with the whole LM schedule resident on the
// device (no host round trip until the summary is read): host orchestration,
// K0 init, K10 finalize, the generic (any size) K5 and K8 and the K7 of a window
// without a free camera.  The fast paths live in ba_schur.hip (K5), ba_solve.hip
// (K7) and ba_update.hip (K8), the K7 of larger systems in ba_solve_big.hip;
// the pose solve of one frame (K11) follows the same schedule in refine_pose.hip.
//
// Replaces optimization::bundle_adjust's ceres::Solve
// (reference src/Optimization.cpp:21-72,127-142,269-374).  The Ceres
// trust-region schedule restated here is documented in oracle/ba.c and
// SURVEY.md §8 a11; this file works in UNSCALED parameters, which is
// algebraically identical to Ceres' Jacobi-scaled solve:
//     (H + Lambda) delta = -g,   Lambda_i = clamp(s_i^2 H_ii, 1e-6, 1e32) / (radius s_i^2),
//     s_i = 1 / (1 + sqrt(H_ii at the first linearisation)),
//     model_cost_change = 1/2 (delta' Lambda delta - delta' g).
//
// Kernel chain per LM iteration (three launches, all unconditional; each kernel
// returns at once when state.done is set):
//   K5 linearise + Schur   applies the accept / reject decision of the PREVIOUS
//                          iteration first (every workgroup redundantly, from the
//                          previous state block and slot sums: no "decide" launch),
//                          then analytic Jacobians (left Jacobian of SO(3), never
//                          stored), Huber weights, V/gp, U/gc, damped V^-1, Schur
//                          products into S and the reduced rhs
//   [RCCL all-reduce of the accumulators when landmark-sharded]
//   K7 reduced solve       one workgroup: (U + Lambda_c - sum Y Y') y = rhs by block
//                          L D L', delta_c, candidate cameras
//   K8 back-substitution   delta_p, candidate points, model-cost terms, robust cost
//                          at the candidate; clears the accumulators for the next K5
//   [RCCL all-reduce of the step scalars]
// K10 applies the last decision and writes the result back.
#include <stdlib.h>
#include <atomic>
#include <thread>

#include "ba_common.h"
#include "ba_backsub_body.h"
#include "ba_init_body.h"
#include "ba_step_body.h"
#include "ba_blocks.h"

// ---------------------------------------------------------------------- K0 (body: ba_init_body.h)
__global__ void ba_init(BaDims d, BaBufs b, BaOpt opt, const double* __restrict__ cams_in,
                        const double* __restrict__ pts_in, unsigned long long free_mask, int from_mask,
                        uint8_t* __restrict__ cam_free, int32_t* __restrict__ zero_i32, int zero_n)
{
    ba_init_body(d, b, opt, cams_in, pts_in, free_mask, from_mask, cam_free, zero_i32, zero_n);
}
// batched (blockIdx.z = window; windows of at most 64 cameras: the free-camera table is the mask)
__global__ void ba_init_batch(const BaWin* w, BaOpt opt)
{
    const BaWin& x = w[blockIdx.z];
    ba_init_body(x.d, x.b, opt, x.cams_in, x.pts_in, x.free_mask, 1, x.cam_free, x.zero_ptr, x.zero_n);
}

// ---------------------------------------------------------------------- K5
__global__ __launch_bounds__(BA_THREADS) void ba_linearize_schur(BaDims d, BaBufs b, BaOpt opt, int it)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [Cf][42]: U(36) gc(6)
    __shared__ BaState st_sh;
    const BaState st = ba_state_for_iteration(b, opt, it, &st_sh);
    if (st.done) return;
    const int nlds = d.Cf * 42;
    for (int i = threadIdx.x; i < nlds; i += blockDim.x) lds[i] = 0.0;
    __syncthreads();

    const double* prep = b.prep + (size_t)st.cur * d.C * BA_PREP;
    const double* Xp = b.Xp + (size_t)st.cur * d.P * 3;
    const size_t rep_off = (size_t)(blockIdx.x & (BA_UREP - 1)) * b.cam_stride;
    double cost = 0.0, gmax = 0.0, fail = 0.0;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < d.P) {
        const double X[3] = {Xp[3 * (size_t)p], Xp[3 * (size_t)p + 1], Xp[3 * (size_t)p + 2]};
        const int o0 = b.obs_ptr[p], o1 = b.obs_ptr[p + 1];
        double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
        ObsLin o;
        for (int oi = o0; oi < o1; oi++) {
            const int c = b.obs_cam[oi];
            obs_eval<true>(prep + (size_t)c * BA_PREP, X, b.obs_uv[oi], d, o);
            cost += 0.5 * o.rho;
            const double w = o.w;
            V[0] += w * (o.jp[0] * o.jp[0] + o.jp[3] * o.jp[3]);
            V[1] += w * (o.jp[0] * o.jp[1] + o.jp[3] * o.jp[4]);
            V[2] += w * (o.jp[0] * o.jp[2] + o.jp[3] * o.jp[5]);
            V[3] += w * (o.jp[1] * o.jp[1] + o.jp[4] * o.jp[4]);
            V[4] += w * (o.jp[1] * o.jp[2] + o.jp[4] * o.jp[5]);
            V[5] += w * (o.jp[2] * o.jp[2] + o.jp[5] * o.jp[5]);
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] += w * (o.jp[k] * o.r0 + o.jp[3 + k] * o.r1);
            const int s = b.slot[c];
            if (s >= 0) {
                double* u = lds + s * 42;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int e = a; e < 6; e++) atomicAdd(&u[a * 6 + e], w * (o.jc[a] * o.jc[e] + o.jc[6 + a] * o.jc[6 + e]));
                    atomicAdd(&u[36 + a], w * (o.jc[a] * o.r0 + o.jc[6 + a] * o.r1));
                }
            }
        }
        gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
        // Jacobi scaling (first linearisation) and LM damping of the point block
        double sp[3], lam[3];
        const double Vd[3] = {V[0], V[3], V[5]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (!st.have_scale) {
                sp[k] = opt.jacobi ? 1.0 / (1.0 + sqrt(Vd[k])) : 1.0;
                b.sp[3 * (size_t)p + k] = sp[k];
            } else {
                sp[k] = b.sp[3 * (size_t)p + k];
            }
            const double s2 = sp[k] * sp[k];
            lam[k] = clampd(s2 * Vd[k], opt.dmin, opt.dmax) / (st.radius * s2);
            b.lamp[3 * (size_t)p + k] = lam[k];
            b.gp[3 * (size_t)p + k] = g[k];
        }
        double Vdm[6] = {V[0] + lam[0], V[1], V[2], V[3] + lam[1], V[4], V[5] + lam[2]}, I[6];
        const bool ok = inv3_psd(Vdm, I);
        if (!ok) { fail = 1.0; I[0] = I[1] = I[2] = I[3] = I[4] = I[5] = 0.0; }
#pragma unroll
        for (int k = 0; k < 6; k++) b.Vinv[6 * (size_t)p + k] = I[k];
        // Schur products: S[si,sj] -= Y_i W_j^T, rhs[si] -= Y_i g,  Y_i = W_i V^-1, W_i = w Jc_i^T Jp_i
        if (ok) {
            for (int oi = o0; oi < o1; oi++) {
                const int ci = b.obs_cam[oi];
                const int si = b.slot[ci];
                if (si < 0) continue;
                obs_eval<true>(prep + (size_t)ci * BA_PREP, X, b.obs_uv[oi], d, o);
                double Y[18];
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    const double w0 = o.w * (o.jc[a] * o.jp[0] + o.jc[6 + a] * o.jp[3]);
                    const double w1 = o.w * (o.jc[a] * o.jp[1] + o.jc[6 + a] * o.jp[4]);
                    const double w2 = o.w * (o.jc[a] * o.jp[2] + o.jc[6 + a] * o.jp[5]);
                    Y[a * 3 + 0] = w0 * I[0] + w1 * I[1] + w2 * I[2];
                    Y[a * 3 + 1] = w0 * I[1] + w1 * I[3] + w2 * I[4];
                    Y[a * 3 + 2] = w0 * I[2] + w1 * I[4] + w2 * I[5];
                    atomicAdd(&b.rhs[rep_off + 6 * si + a], -(Y[a * 3] * g[0] + Y[a * 3 + 1] * g[1] + Y[a * 3 + 2] * g[2]));
                }
                ObsLin oj;
                for (int ojx = o0; ojx < o1; ojx++) {
                    const int cj = b.obs_cam[ojx];
                    const int sj = b.slot[cj];
                    if (sj < 0) continue;
                    obs_eval<true>(prep + (size_t)cj * BA_PREP, X, b.obs_uv[ojx], d, oj);
                    double* Sblk = b.S + (size_t)(6 * si) * d.n + 6 * sj;
#pragma unroll
                    for (int e = 0; e < 6; e++) {
                        const double w0 = oj.w * (oj.jc[e] * oj.jp[0] + oj.jc[6 + e] * oj.jp[3]);
                        const double w1 = oj.w * (oj.jc[e] * oj.jp[1] + oj.jc[6 + e] * oj.jp[4]);
                        const double w2 = oj.w * (oj.jc[e] * oj.jp[2] + oj.jc[6 + e] * oj.jp[5]);
#pragma unroll
                        for (int a = 0; a < 6; a++)
                            atomicAdd(&Sblk[(size_t)a * d.n + e], -(Y[a * 3] * w0 + Y[a * 3 + 1] * w1 + Y[a * 3 + 2] * w2));
                    }
                }
            }
        }
    }
    // block reductions
    cost = wave_sum(cost);
    fail = wave_sum(fail);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gmax = fmax(gmax, __shfl_down(gmax, off, 64));
    if ((threadIdx.x & 63) == 0) {
        const size_t slot = (size_t)(blockIdx.x & (BA_NSLOT - 1)) * BA_SLOT_STRIDE;
        atomicAdd(&b.scal[slot], cost);
        if (fail > 0.0) atomicAdd(&b.scal[slot + 1], fail);
        atomic_max_nonneg(&b.gmax[slot], gmax);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nlds; i += blockDim.x) {
        const int s = i / 42, k = i % 42;
        const double v = lds[i];
        if (v != 0.0) {
            if (k < 36) atomicAdd(&b.U[rep_off + s * 36 + k], v);
            else atomicAdd(&b.gc[rep_off + 6 * s + (k - 36)], v);
        }
    }
}

// ---------------------------------------------------------------------- K7 (bodies: ba_step_body.h)
// A window without a free camera (n == 0) has no reduced system: only the ends of the round are left.  The landmarks
// still move, so the cost, the gradient test and K5's failure flag come from the slot lines; the candidate cameras are
// the cameras.  One workgroup.
__global__ __launch_bounds__(256) void ba_no_free_camera(BaDims d, BaBufs b, BaOpt opt)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    __shared__ BaState st;
    __shared__ int s_fail;
    __shared__ double red[16], red3[16][3];
    if (!ba_step_begin(d, b, &st, &s_fail)) return;
    __syncthreads();
    double cost = 0.0;
    if (st.fresh && tid < 64) cost = slot_sum(b.scal, 0);
    if (!ba_step_gradient_test(b, opt, &st, &s_fail, red, 0.0, cost)) return;
    __syncthreads();
    if (s_fail) {
        if (tid == 0) { st.solver_failed = 1; *b.st = st; }
        return;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    bool bad = false;
    for (int c = tid; c < d.C; c += nt) bad |= ba_step_camera(d, b, st, c, b.dc, b.rhs, b.gc, false, acc);
    ba_step_reduce(&st, &s_fail, red3, acc, bad);
    if (tid == 0) *b.st = st;
}

// ---------------------------------------------------------------------- K8
__global__ __launch_bounds__(BA_THREADS) void ba_backsub_cost(BaDims d, BaBufs b)
{
    const BaState st = *b.st;
    if (st.done) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < b.acc_count; i += (size_t)gridDim.x * blockDim.x) b.acc[i] = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < BA_NSLOT * BA_SLOT_STRIDE; i += gridDim.x * blockDim.x) b.gmax[i] = 0.0;
    if (st.solver_failed) return;
    const double* prep = b.prep + (size_t)st.cur * d.C * BA_PREP;
    const double* prepn = b.prep + (size_t)(st.cur ^ 1) * d.C * BA_PREP;
    const double* Xp = b.Xp + (size_t)st.cur * d.P * 3;
    double* Xn = b.Xp + (size_t)(st.cur ^ 1) * d.P * 3;
    double cost = 0.0, mcc = 0.0, ssq = 0.0, xsq = 0.0;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < d.P) {
        const double X[3] = {Xp[3 * (size_t)p], Xp[3 * (size_t)p + 1], Xp[3 * (size_t)p + 2]};
        const int o0 = b.obs_ptr[p], o1 = b.obs_ptr[p + 1];
        double t[3] = {b.gp[3 * (size_t)p], b.gp[3 * (size_t)p + 1], b.gp[3 * (size_t)p + 2]};
        const double g[3] = {t[0], t[1], t[2]};
        ObsLin o;
        for (int oi = o0; oi < o1; oi++) {
            const int c = b.obs_cam[oi];
            const int s = b.slot[c];
            if (s < 0) continue;
            obs_eval<true>(prep + (size_t)c * BA_PREP, X, b.obs_uv[oi], d, o);
            double m0 = 0.0, m1 = 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) { const double dc = b.dc[6 * s + a]; m0 += o.jc[a] * dc; m1 += o.jc[6 + a] * dc; }
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] += o.w * (o.jp[k] * m0 + o.jp[3 + k] * m1);   // W_i^T delta_c
        }
        const double* I = b.Vinv + 6 * (size_t)p;
        const double dp[3] = {-(I[0] * t[0] + I[1] * t[1] + I[2] * t[2]), -(I[1] * t[0] + I[3] * t[1] + I[4] * t[2]),
                              -(I[2] * t[0] + I[4] * t[1] + I[5] * t[2])};
        double Xc[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Xc[k] = X[k] + dp[k];
            Xn[3 * (size_t)p + k] = Xc[k];
            mcc += 0.5 * (dp[k] * dp[k] * b.lamp[3 * (size_t)p + k] - dp[k] * g[k]);
            ssq += (X[k] - Xc[k]) * (X[k] - Xc[k]);
            xsq += X[k] * X[k];
        }
        for (int oi = o0; oi < o1; oi++) {
            obs_eval<false>(prepn + (size_t)b.obs_cam[oi] * BA_PREP, Xc, b.obs_uv[oi], d, o);
            cost += 0.5 * o.rho;
        }
    }
    cost = wave_sum(cost); mcc = wave_sum(mcc); ssq = wave_sum(ssq); xsq = wave_sum(xsq);
    if ((threadIdx.x & 63) == 0) {
        const size_t slot = (size_t)(blockIdx.x & (BA_NSLOT - 1)) * BA_SLOT_STRIDE;
        atomicAdd(&b.pt_scal[slot + 0], cost);
        atomicAdd(&b.pt_scal[slot + 1], mcc);
        atomicAdd(&b.pt_scal[slot + 2], ssq);
        atomicAdd(&b.pt_scal[slot + 3], xsq);
    }
}

// -------------------------------------------------------------------- finalize
#define BA_FINALIZE_WGS 32
static __device__ __forceinline__ void ba_finalize_body(const BaDims& d, const BaBufs& b, const BaOpt& opt, int it, double* __restrict__ cams_out,
                                                        const uint8_t* __restrict__ cam_free, double* __restrict__ pts_out, BaState* host_st,
                                                        BaTrace* host_trace, double* __restrict__ host_cams, double* __restrict__ host_vb,
                                                        volatile int* host_done = nullptr, int32_t* __restrict__ zero_i32 = nullptr, int zero_n = 0)
{
    __shared__ int usable, cur;
    __shared__ BaState st_fin;
    // the decisions of the last round (every workgroup recomputes them; b.st_prev / b.pt_prev are immutable here)
    if (threadIdx.x < 64) ba_decide(b, opt, it, blockIdx.x == 0 ? b.trace : nullptr, &st_fin, false);
    __syncthreads();
    if (threadIdx.x == 0) {
        BaState st = st_fin;
        // after a successful step the cost at the new point is K5's value if it ran, else the candidate cost
        // a K8 workgroup of the fused launch never saw its K7 publish: the result is unusable — not because the solver failed
        // but because of scheduling (queue preemption, another process on the GPU, counter collection): the host re-runs the
        // solve as separate launches from the untouched inputs (ba_solve_impl)
        if (b.dbg[BA_HAND_ERR] != 0ull) { st.termination = RS_BA_FAILURE; st.hand_lost = 1; }
        const bool ok = st.termination != RS_BA_FAILURE && isfinite(st.x_cost) && st.x_cost <= st.initial_cost;
        usable = ok ? 1 : 0;
        cur = st.cur;
        st.usable = usable;
        if (blockIdx.x == 0) {
            *b.st = st;
            *host_st = st;            // the summary goes straight into pinned host memory: no copy launch after the solve
            if (!host_done) __threadfence_system();      // (with a completion flag, the ONE fence in front of the flag covers it)
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) {            // the per-iteration record follows the summary (entries of earlier iterations were
        const int ne = st_fin.iter * (int)(sizeof(BaTrace) / sizeof(double));   // written by earlier launches, the last one above)
        const double* src = (const double*)b.trace;
        double* dst = (double*)host_trace;
        for (int i = threadIdx.x; i < ne; i += blockDim.x) dst[i] = src[i];
    }
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    const double* Xc = b.Xc + (size_t)cur * d.C * 6;
    const double* Xp = b.Xp + (size_t)cur * d.P * 3;
    // the grouping's histogram / cursors / span word go back to zero for the next solve's count launch (ba_init_count)
    for (int i = tid; i < zero_n; i += nth) zero_i32[i] = 0;
    // Everything the HOST waits for is written by workgroup 0 alone and fenced once: the summary and the trace (above), and
    // the cameras as the caller will see them in d_cameras, mirrored into pinned host memory (poses are host-owned objects in
    // the reference — Frame::set_pose, src/Optimization.cpp:363-368 — so the shim needs them there anyway).  Then it raises
    // the completion flag the host spins on (hipStreamSynchronize is a blocking wait whose wake-up costs tens of
    // microseconds).  The device-side results (d_cameras, d_points) are written by the whole grid and are STREAM-ordered:
    // the call may return while those copies are still running; whatever reads them on the context's stream — the next
    // library call, a staged download, a torch op — is ordered behind them.
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < d.C * 6; i += blockDim.x) host_cams[i] = (usable && cam_free[i / 6]) ? Xc[i] : cams_out[i];
        if (host_vb)        // inertial solve: velocity | bias of the accepted state (the host applies the write-back rule)
            for (int i = threadIdx.x; i < d.C * 9; i += blockDim.x) host_vb[i] = b.imu.Xv[(size_t)cur * d.C * 9 + i];
        if (host_done) {
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) *host_done = it + 1;
        } else {
            __syncthreads();     // (host_cams reads cams_out before the grid rewrites it: this workgroup's share of that is below)
        }
    }
    if (usable) {
        // (workgroup 0 has read cams_out for the mirror above; the other workgroups only touch entries of FREE cameras, whose
        // mirror value comes from Xc, so no ordering between the workgroups is needed)
        for (int i = tid; i < d.C * 6; i += nth)
            if (cam_free[i / 6]) cams_out[i] = Xc[i];
        for (int i = tid; i < d.P * 3; i += nth) pts_out[i] = Xp[i];
    }
}

__global__ void ba_finalize(BaDims d, BaBufs b, BaOpt opt, int it, double* __restrict__ cams_out,
                            const uint8_t* __restrict__ cam_free, double* __restrict__ pts_out, BaState* host_st,
                            BaTrace* host_trace, double* __restrict__ host_cams, double* __restrict__ host_vb, volatile int* host_done,
                            int32_t* __restrict__ zero_i32, int zero_n)
{
    ba_finalize_body(d, b, opt, it, cams_out, cam_free, pts_out, host_st, host_trace, host_cams, host_vb, host_done, zero_i32, zero_n);
}
__global__ void ba_finalize_batch(const BaWin* w, BaOpt opt, int it)
{
    const BaWin& x = w[blockIdx.z];
    const BaBufs b = ba_win_round(x, it, true);
    ba_finalize_body(x.d, b, opt, it, x.cams_out, x.cam_free, x.pts_out, x.h_st, x.h_trace, x.h_cams, nullptr);
}

// Landmark-sharded solves: two facts every rank must agree on travel as MIN all-reduces of one 64-bit key each (the
// collective the sharded matcher already uses): the largest camera span of a landmark (decides between the banded and
// the general reduced solve: every rank must run the same factorisation on the all-reduced system) and "some rank lost a
// hand-off of its fused K7 + K8 launch" (every rank re-runs the solve, or none: their collectives must stay paired).
#define BA_KEY_SPAN 58
#define BA_KEY_LOST 59
__global__ void ba_span_key(const int32_t* __restrict__ maxspan, unsigned long long* __restrict__ key)
{
    *key = ~(unsigned long long)(unsigned)max(*maxspan, 0);            // min of ~span = ~(max span)
}
__global__ void ba_lost_key(const BaState* __restrict__ st, unsigned long long* __restrict__ key)
{
    *key = st->hand_lost ? 0ull : 1ull;                                // min = 0 as soon as one rank lost a hand-off
}

// ------------------------------------------------------------------ host side
extern "C" void rs_ba_default_options(rs_ba_options* o)
{
    if (!o) return;
    o->max_num_iterations = 10;
    o->huber_delta = sqrt(5.991);
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->max_num_consecutive_invalid_steps = 5;
    o->jacobi_scaling = 1;
}

extern "C" int rs_prof_counters(rs_context* ctx, uint64_t* h_out, int n)
{
    if (!ctx || !h_out || n < 0 || n > 64) return RS_ERR_INVALID;
    if (!ctx->ba_cache) { for (int i = 0; i < n; i++) h_out[i] = 0; return RS_OK; }
    RS_HIP(ctx, hipMemcpyAsync(h_out, ctx->ba_cache, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RS_OK;
}

// the inertial residual blocks of one solve (null for a vision-only solve)
struct BaInertialArgs {
    double* h_velocity;            // [C][3] in/out
    double* h_bias;                // [C][6] in/out
    const rs_imu_factor* factors;
    int n_factors;
    const double* gravity;
};

// whitener of src/ImuFactor.cpp:10-17: L^-1 of the covariance's LLT, identity when it is not positive definite
void imu_whitener(const double cov[81], double W[81])
{
    double L[81];
    memcpy(L, cov, sizeof L);
    bool ok = true;
    for (int j = 0; j < 9 && ok; j++) {
        double dd = L[j * 9 + j];
        for (int k = 0; k < j; k++) dd -= L[j * 9 + k] * L[j * 9 + k];
        if (!(dd > 0.0) || !std::isfinite(dd)) { ok = false; break; }
        dd = sqrt(dd);
        L[j * 9 + j] = dd;
        for (int i = j + 1; i < 9; i++) {
            double t = L[i * 9 + j];
            for (int k = 0; k < j; k++) t -= L[i * 9 + k] * L[j * 9 + k];
            L[i * 9 + j] = t / dd;
        }
    }
    memset(W, 0, sizeof(double) * 81);
    if (!ok) { for (int i = 0; i < 9; i++) W[i * 9 + i] = 1.0; return; }
    for (int c = 0; c < 9; c++)
        for (int i = 0; i < 9; i++) {
            double t = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) t -= L[i * 9 + k] * W[k * 9 + c];
            W[i * 9 + c] = t / L[i * 9 + i];
        }
}

// Solves of this process that are between entry and return right now (any context, any thread).  A solve that has the
// device to itself — as far as the library can tell — runs K7 + K8 as one launch: its K8 workgroups hold a CU each while
// they wait for K7.  When other solves are in flight (several sessions on one GPU) those CUs are what the others need,
// and the two-launch form gives the higher aggregate: 8 sessions 3.95 k -> 4.70 k solves/s (tools/multi_session.py).
static std::atomic<int> g_ba_in_flight{0};
struct BaInFlight {
    int others;
    BaInFlight() : others(g_ba_in_flight.fetch_add(1)) {}
    ~BaInFlight() { g_ba_in_flight.fetch_sub(1); }
};

// The argument list of rs_bundle_adjust as one record.  (A missing intrinsics pointer travels as a missing free-camera
// table: ba_solve_once refuses both in the same null-pointer test.)
static rs_ba_problem ba_problem_from(int n_cameras, int n_points, int n_obs, double* d_cameras, const uint8_t* h_cam_free, double* d_points,
                                     const int32_t* d_obs_ptr, const int32_t* d_obs_cam, const float* d_obs_uv, const float* K)
{
    return {n_cameras, n_points, n_obs, d_cameras, K ? h_cam_free : nullptr, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, {K ? K[0] : 0, K ? K[1] : 0, K ? K[2] : 0, K ? K[3] : 0}};
}

// Inertial frames: the cameras an IMU factor touches get a velocity (3) + bias (6) block; inert[c] = index of that block or
// -1, *Ci their number.  *chain: the factors join consecutive inertial cameras (what the reference builds: block-tridiagonal H_zz)
static int ba_inertial_slots(rs_context* ctx, const rs_ba_problem& q, const BaInertialArgs& in, std::vector<int32_t>& inert, int* Ci, bool* chain)
{
    const int C = q.n_cameras;
    for (int f = 0; f < in.n_factors; f++) {
        const int i = in.factors[f].cam_i, j = in.factors[f].cam_j;
        if (i < 0 || j < 0 || i >= C || j >= C || i == j || !q.h_cam_free[i] || !q.h_cam_free[j])
            return rs_fail(ctx, RS_ERR_INVALID, "IMU factor %d must join two distinct optimised cameras", f);
    }
    std::vector<uint8_t> touched(C, 0);
    for (int f = 0; f < in.n_factors; f++) { touched[in.factors[f].cam_i] = 1; touched[in.factors[f].cam_j] = 1; }
    for (int c = 0; c < C; c++) if (touched[c]) inert[c] = (*Ci)++;
    *chain = true;
    for (int f = 0; f < in.n_factors && *chain; f++) *chain = inert[in.factors[f].cam_j] == inert[in.factors[f].cam_i] + 1;
    return RS_OK;
}

// Launch fusion, decided once the grouping is carved.  `others`: solves of this process in flight besides this one.
static void ba_choose_fusion(const rs_context* ctx, const BaDims& d, const BaBufs& b, const BaGroup& grp, BaPath& path, bool allow_fuse, bool inertial, int others)
{
    // K7 + K8 as one launch (ba_solve.hip): the plain local window only — vision-only, one rank, both LDS kernels
    // and only while all of its workgroups are resident at once (one per CU: the launch carries K7's LDS): beyond that
    // K8's workgroups would run in several shifts behind the hand-off, and the launch of its own (many per CU) is faster
    // The whole round as ONE launch (ba_round.hip: K5's item workgroups become K8's after they have counted themselves for
    // K7): the same conditions plus the MFMA K5 with its camera blocks in LDS, and again every workgroup resident at once.
    // (a landmark shard may fuse K7 + K8 too: the launch sits between the two exchange steps of the round, C1 in front of
    // it and C2 behind; whether a rank fuses is its own business — shard sizes differ — but a lost hand-off is agreed on by
    // all ranks after the solve, so that every rank re-runs it or none does)
    path.may_fuse = allow_fuse && path.solve_lds && path.k8_lds && !inertial;
    // Measured (tools/round_stamps.py): 86 us per round against 43 + 45 as two launches — the round is a strict
    // chain (linearise -> solve -> back-substitute), so keeping the workgroups resident buys the boundary and little else.
    // It is therefore opt-in ("ba_fuse_mode" 3); the default stays K5, then K7 + K8 in one launch.
    path.fuse_round = path.may_fuse && !rs_comm_active(ctx) && path.use_mfma && ctx->ba_fuse_mode == 3 && path.ns <= BA_CALIBRATED_SETS &&
                      ba_round_eligible(d) && ba_round_workgroups(d, b, grp) <= ctx->n_cu;
    path.fuse78 = !path.fuse_round && path.may_fuse && d.P > 0 /* an empty landmark shard has no K8 workgroup to clear the accumulators */ &&
                  (ctx->ba_fuse_mode >= 2 || (ctx->ba_fuse_mode == 0 && others == 0)) &&
                  ba_solve_backsub_workgroups(d, b, ctx->n_cu) <= ctx->n_cu;
}

// A 64-bit key every rank holds, MIN-reduced over the ranks and read by the host (the stream is drained when it returns).
static int ba_min_key_to_host(rs_context* ctx, unsigned long long* d_key, volatile unsigned long long* h_key)
{
    const int rc = rs_allreduce_min_u64(ctx, d_key, 1);
    if (rc) return rc;
    RS_HIP(ctx, hipMemcpyAsync((void*)h_key, d_key, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RS_OK;
}

// Blocked reduced solve: is S block-banded?  The grouping has just computed the largest camera span of a landmark; one
// word travels to the host (the solve is milliseconds: the wait costs a few per cent of one round) and decides between
// the one-launch banded factorisation and the general blocked one (*band as in BaPath).
static int ba_choose_band(rs_context* ctx, const BaPath& path, bool inertial, const BaGroup& grp, const BaBufs& b, volatile unsigned long long* h_key, int* band)
{
    *band = 0;
    if (!path.solve_big || !path.use_mfma || inertial || ctx->ba_band_mode == 1) return RS_OK;
    hipStream_t s = ctx->stream;
    const int banded = ctx->ba_band_mode == 2 ? 1 : 2;
    if (rs_comm_active(ctx)) {
        // landmark shards: the span of the WHOLE window is the largest of the ranks' spans (round 4; every rank then runs
        // the same banded factorisation on the same all-reduced system, as it runs the same general one)
        *h_key = 0ull;
        hipLaunchKernelGGL(ba_span_key, dim3(1), dim3(1), 0, s, (const int32_t*)grp.maxspan, b.dbg + BA_KEY_SPAN);
        const int rc = ba_min_key_to_host(ctx, b.dbg + BA_KEY_SPAN, h_key);
        if (rc) return rc;
        if (~*h_key <= (unsigned long long)ba_band_max_span()) *band = banded;      // (the key is ~span)
        return RS_OK;
    }
    volatile int32_t* h_span = (volatile int32_t*)h_key;
    *h_span = -1;
    RS_HIP(ctx, hipMemcpyAsync((void*)h_span, grp.maxspan, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    long spins = 0;
    while (*h_span < 0)
        if ((++spins & 0x3FFFF) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
    if (*h_span < 0) RS_HIP(ctx, hipStreamSynchronize(s));
    if (*h_span >= 0 && *h_span <= ba_band_max_span()) *band = banded;
    return RS_OK;
}

// Inertial blocks onto the device: the carve behind the common workspace, the whitened factors, the inertial slots and the
// velocity | bias state of both parities.  fac_host, xv_host and inert are pageable sources of asynchronous copies: the
// caller keeps them alive until it has synchronised (the copies complete before the call returns — it waits for finalize).
static int ba_inertial_upload(rs_context* ctx, const BaInertialArgs& in, const BaDims& d, BaBufs& b, const BaPath& path, char* ws_big, double* ws_zacc,
                              const std::vector<int32_t>& inert, int Ci, std::vector<ImuFactorDev>& fac_host, std::vector<double>& xv_host)
{
    hipStream_t s = ctx->stream;
    const size_t C = (size_t)d.C;
    const int N_in = d.n + 9 * Ci;
    ImuFactorDev* d_fac = nullptr; int32_t* d_inert = nullptr;
    ba_inertial_carve(ws_big, N_in, in.n_factors, d.C, &b.imu, &d_fac, &d_inert);
    b.imu.n_fac = in.n_factors; b.imu.Ci = Ci; b.imu.N = N_in;
    if (path.imu_lds) {
        b.imu.zacc = ws_zacc;
        b.imu.zacc_n = (int)ba_imu_lds_zacc_doubles(Ci, d.n);
        RS_HIP(ctx, hipMemsetAsync(b.imu.zacc, 0, sizeof(double) * (size_t)b.imu.zacc_n, s));
    }
    for (int k = 0; k < 3; k++) b.imu.gravity[k] = in.gravity[k];
    fac_host.resize((size_t)in.n_factors);
    for (int f = 0; f < in.n_factors; f++) { fac_host[(size_t)f].f = in.factors[f]; imu_whitener(in.factors[f].covariance, fac_host[(size_t)f].W); }
    xv_host.resize(9 * C);
    for (size_t c = 0; c < C; c++) {
        for (int k = 0; k < 3; k++) xv_host[9 * c + k] = in.h_velocity[3 * c + k];
        for (int k = 0; k < 6; k++) xv_host[9 * c + 3 + k] = in.h_bias[6 * c + k];
    }
    RS_HIP(ctx, hipMemcpyAsync(d_fac, fac_host.data(), sizeof(ImuFactorDev) * fac_host.size(), hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(d_inert, inert.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(b.imu.Xv, xv_host.data(), sizeof(double) * 9 * C, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(b.imu.Xv + 9 * C, xv_host.data(), sizeof(double) * 9 * C, hipMemcpyHostToDevice, s));
    return RS_OK;
}
// unpack_inertial for the optimised frames, src/Optimization.cpp:363-368: velocity | bias of the accepted state (h_vb, finalize)
static void ba_inertial_unpack(const BaInertialArgs& in, const rs_ba_problem& q, const double* h_vb)
{
    for (size_t c = 0; c < (size_t)q.n_cameras; c++) {
        if (!q.h_cam_free[c]) continue;
        for (int k = 0; k < 3; k++) in.h_velocity[3 * c + k] = h_vb[9 * c + k];
        for (int k = 0; k < 6; k++) in.h_bias[6 * c + k] = h_vb[9 * c + 3 + k];
    }
}

// LDS attributes of the kernels the path uses (sticky per process: rs_lds_attr)
static int ba_prepare_kernels(rs_context* ctx, const BaDims& d, const BaPath& path)
{
    if (path.solve_lds && ba_prepare_reduced_solve_lds(d.n) != 0) return rs_fail(ctx, RS_ERR_HIP, "LDS attribute (K7)");
    const size_t k5_lds = sizeof(double) * (size_t)d.Cf * 42;
    if (!path.use_mfma && k5_lds > 48 * 1024)
        RS_HIP(ctx, rs_lds_attr((const void*)ba_linearize_schur, k5_lds));
    if (path.use_mfma && ba_prepare_schur(d.C, d.Cf) != 0) return rs_fail(ctx, RS_ERR_HIP, "LDS attribute (K5)");
    return RS_OK;
}

// Set-up launches.  Local windows: K0 and the grouping's count in one launch, its scatter (incl. the item masks) in a
// second — two instead of four (*fused).  The count adds into a histogram that must be zero when the launch starts: the
// finalize kernel of the previous solve leaves it so, and the context remembers that (grp_zero_ptr) unless the workspace was
// reallocated or another caller asked for workspace bytes reaching into it since (ws_dirty_hi); otherwise one memset.
static int ba_enqueue_setup(rs_context* ctx, const BaWin& w, const BaOpt& opt, bool use_mfma, const void* ws, int from_mask, bool* fused)
{
    hipStream_t s = ctx->stream;
    *fused = use_mfma && ba_setup_fusable(w.d, w.g);
    if (*fused) {
        const bool known_zero = ctx->grp_zero_ptr == w.zero_ptr && ctx->grp_zero_n == w.zero_n &&
                                ctx->ws_dirty_hi <= (size_t)((const char*)w.zero_ptr - (const char*)ws);
        ctx->grp_zero_ptr = nullptr;                                  // (until this solve's finalize kernel is enqueued)
        if (!known_zero) RS_HIP(ctx, hipMemsetAsync(w.zero_ptr, 0, sizeof(int32_t) * (size_t)w.zero_n, s));
        ba_launch_setup_fused(ctx, w.d, w.b, opt, w.g, w.cams_in, w.pts_in, w.free_mask, from_mask, w.cam_free);
    } else {
        ctx->grp_zero_ptr = nullptr;
        {
            rs_prof_scope ps(ctx, "K0_ba_init");
            hipLaunchKernelGGL(ba_init, dim3(64), dim3(256), 0, s, w.d, w.b, opt, w.cams_in, w.pts_in, w.free_mask, from_mask, w.cam_free, w.zero_ptr, w.zero_n);
        }
        if (use_mfma) {
            const int rc = ba_launch_grouping(ctx, w.d, w.b, w.g);
            if (rc) return rc;
        }
    }
    ctx->ws_dirty_hi = 0;
    return RS_OK;
}

// Double-buffered state / step-scalar / set blocks: round `it` works on [it & 1] and reads [(it + 1) & 1].  last: the
// finalize launch (round index = rounds enqueued) only reads the blocks of the round before it.
static void ba_point_round(BaWin& w, int it, bool last = false)
{
    BaBufs& b = w.b;
    b.st = w.st_base + (it & 1); b.st_prev = w.st_base + ((it + 1) & 1);
    b.pt_prev = w.pts_base + (size_t)((it + 1) & 1) * w.pts_block;
    b.set_prev = w.set_base + (size_t)((it + 1) & 1) * BA_MAXSETS;
    if (last) return;
    b.pt_scal = w.pts_base + (size_t)(it & 1) * w.pts_block;
    b.set_out = w.set_base + (size_t)(it & 1) * BA_MAXSETS;
}

// One window bound to its part of the workspace and of the pinned block (sized by the same two layouts on a null carver):
// the single solve and every window of the grid batch go through here.  w.d and w.free_mask are the caller's (ba_dims_from);
// the rest of w comes in zeroed and is filled, w.b at round parity 0, and the progress line is reset.  dev / host: carvers
// on the blocks, advanced by this window's pieces.
static BaExtra ba_bind_window(const rs_ba_problem& q, const BaWinAsk& a, rs_carve& dev, rs_carve& host, BaWin& w)
{
    BaBufs& b = w.b;
    BaExtra x;
    b.obs_ptr = q.d_obs_ptr; b.obs_cam = q.d_obs_cam; b.obs_uv = (const float2*)q.d_obs_uv;
    b.hand_timeout = BA_HAND_TIMEOUT_TICKS;
    ba_window_layout(dev, a, w, x);
    ba_pinned_layout(host, a, w, x);
    if (a.use_mfma) {
        ba_group_carve(x.grp, w.d.P, w.d.Cf, w.d.M, &w.g);
        if (a.items >= 0) ba_group_set_items(&w.g, w.d.P, true, a.items);
        ba_group_zero_range(w.g, &w.zero_ptr, &w.zero_n);
    }
    b.obs_cs = w.g.obs_cs;                                  // (null on the generic path)
    w.prog->round = 0; w.prog->done = 0; w.prog->iter = 0;
    b.prog = w.prog;
    w.cams_in = w.cams_out = q.d_cameras; w.pts_in = w.pts_out = q.d_points;
    return x;
}

// K7 of a round, with K8 inside when path.fuse78
static int ba_enqueue_reduced_solve(rs_context* ctx, const BaDims& d, const BaBufs& b, const BaOpt& opt, const BaPath& path, bool inertial, char* ws_big)
{
    hipStream_t s = ctx->stream;
    if (inertial && path.imu_lds) {
        { rs_prof_scope ps(ctx, "K6i_imu_eliminate"); ba_launch_imu_eliminate(s, d, b, opt); }
        { rs_prof_scope ps(ctx, "K7_ba_reduced_solve"); ba_launch_reduced_solve_lds(s, d, b, opt); }
        { rs_prof_scope ps(ctx, "K7i_imu_expand"); ba_launch_imu_expand(s, d, b, opt); }
    }
    else if (inertial) { rs_prof_scope ps(ctx, "K7_ba_reduced_solve_inertial"); return ba_launch_reduced_solve_inertial(ctx, d, b, opt, ws_big); }
    else if (path.solve_lds && path.fuse78) { rs_prof_scope ps(ctx, "K78_ba_solve_backsub"); ba_launch_solve_backsub(s, d, b, opt, ctx->n_cu); }
    else if (path.solve_lds) { rs_prof_scope ps(ctx, "K7_ba_reduced_solve"); ba_launch_reduced_solve_lds(s, d, b, opt); }
    else if (path.solve_big) { rs_prof_scope ps(ctx, "K7_ba_reduced_solve_blocked"); return ba_launch_reduced_solve_big(ctx, d, b, opt, ws_big, path.band); }
    else { rs_prof_scope ps(ctx, "K7_ba_reduced_solve_global"); hipLaunchKernelGGL(ba_no_free_camera, dim3(1), dim3(256), 0, s, d, b, opt); }   // n == 0
    return RS_OK;
}

// One round of the single solve: K5 [C1] K7 K8 [C2], or fewer launches where the path fuses them
static int ba_enqueue_round(rs_context* ctx, BaWin& w, const BaOpt& opt, const BaPath& path, bool inertial, char* ws_big, int it)
{
    hipStream_t s = ctx->stream;
    BaBufs& b = w.b;
    const int pblocks = w.d.P > 0 ? (w.d.P + BA_THREADS - 1) / BA_THREADS : 1;      // (an empty shard still runs the round's decision)
    ba_point_round(w, it);
    if (path.fuse_round) {
        rs_prof_scope ps(ctx, "K578_ba_round");
        ba_launch_round(s, w.d, b, opt, w.g, it);
        return RS_OK;
    }
    if (path.use_mfma) {
        rs_prof_scope ps(ctx, "K5_ba_schur_mfma");
        // more items than compute units: the round's decision once, in front, instead of in every item's prologue
        b.decided = w.g.n_items > ctx->n_cu ? 1 : 0;
        if (b.decided) ba_launch_decide(s, b, opt, it);
        ba_launch_schur(s, w.d, b, opt, w.g, it);
        b.decided = 0;
    } else {
        rs_prof_scope ps(ctx, "K5_ba_linearize_schur");
        hipLaunchKernelGGL(ba_linearize_schur, dim3(pblocks), dim3(BA_THREADS), sizeof(double) * (size_t)w.d.Cf * 42, s, w.d, b, opt, it);
    }
    if (rs_comm_active(ctx)) {
        rs_prof_scope ps(ctx, "C1_allreduce_system");
        // one SUM all-reduce: S | 8 x {rhs, U, gc} | cost / failure slots | every rank's gradient-max block
        const int rc = rs_allreduce_f64(ctx, b.acc, b.acc_count, false);
        if (rc) return rc;
    }
    const int rc = ba_enqueue_reduced_solve(ctx, w.d, b, opt, path, inertial, ws_big);
    if (rc) return rc;
    if (path.fuse78) { /* K8 ran inside the K7 launch */ }
    else if (path.k8_lds) { rs_prof_scope ps(ctx, "K8_ba_backsub_cost"); ba_launch_backsub(s, w.d, b); }
    else { rs_prof_scope ps(ctx, "K8_ba_backsub_cost_global"); hipLaunchKernelGGL(ba_backsub_cost, dim3(pblocks), dim3(BA_THREADS), 0, s, w.d, b); }
    if (rs_comm_active(ctx)) {
        rs_prof_scope ps(ctx, "C2_allreduce_cost");
        return rs_allreduce_f64(ctx, b.pt_scal, w.pts_block, false);
    }
    return RS_OK;
}

static int ba_solve_once(rs_context* ctx, const rs_ba_problem& q, const rs_ba_options* options, rs_ba_summary* h_summary,
                         const BaInertialArgs* in, bool allow_fuse, bool* hand_lost)
{
    *hand_lost = false;
    if (!ctx || !h_summary) return RS_ERR_INVALID;
    const BaInFlight in_flight;
    memset(h_summary, 0, sizeof *h_summary);
    if (q.n_cameras < 0 || q.n_points < 0 || q.n_obs < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    // A landmark shard may be EMPTY (more ranks than landmarks, or a rank whose range holds none): the rank still takes
    // part in every exchange step with zero contributions and solves the reduced system like the others.  Cameras are
    // replicated, so n_cameras == 0 is the same on every rank and ends the call everywhere.
    const bool sharded = rs_comm_active(ctx) && ctx->n_ranks > 1;
    if (q.n_cameras == 0 || ((q.n_points == 0 || q.n_obs == 0) && !sharded)) {   // nothing to optimise
        h_summary->usable = 0;
        h_summary->termination = RS_BA_FAILURE;
        return RS_OK;
    }
    if (!q.d_cameras || !q.h_cam_free || !q.d_obs_ptr || (q.n_points > 0 && !q.d_points) || (q.n_obs > 0 && (!q.d_obs_cam || !q.d_obs_uv)))
        return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    rs_ba_options def;
    if (!options) { rs_ba_default_options(&def); options = &def; }
    RS_HIP(ctx, hipSetDevice(ctx->device));

    // dimensions, inertial slots, kernel path
    BaWin w;
    memset(&w, 0, sizeof w);
    BaDims& d = w.d;
    std::vector<int32_t> slot(q.n_cameras), inert(q.n_cameras, -1);
    const bool supported = ba_dims_from(q, options, d, slot.data(), &w.free_mask);
    const BaOpt opt = ba_opt_from(options);
    if (opt.max_iter < 0 || opt.max_iter > 1000) return rs_fail(ctx, RS_ERR_INVALID, "max_num_iterations out of range");
    if (!supported) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "more than 484 free cameras");
    int Ci = 0, rc = RS_OK; bool imu_chain = false;
    if (in && (rc = ba_inertial_slots(ctx, q, *in, inert, &Ci, &imu_chain)) != RS_OK) return rc;
    // (inertial solves keep three sets: their per-radius elimination kernels were sized and tested for that)
    BaPath path = ba_choose_path(ctx, d, opt.max_iter, in != nullptr, Ci, imu_chain, in ? BA_CALIBRATED_SETS : BA_DEFAULT_SETS,
                                 in ? BA_CALIBRATED_SETS : BA_MAXSETS);

    // the window on its workspace and pinned block; behind the common workspace the blocked / inertial solve's part and the
    // accumulators of the inertial elimination
    const bool comm = rs_comm_active(ctx);
    const BaWinAsk ask = {path.ns, opt.max_iter, comm ? ctx->n_ranks : 1, comm ? ctx->rank : 0, path.srep,
                          path.use_mfma ? ba_group_bytes(d.P, d.Cf, d.M) : 16,
                          in ? ba_inertial_bytes(d.n + 9 * Ci, in->n_factors, d.C) : (path.solve_big ? ba_big_bytes(d.n) : 16),
                          path.imu_lds ? ba_imu_lds_total_doubles(Ci, d.n, path.ns) : 0, true, in != nullptr, path.use_mfma, ctx->ba_item ? ctx->ba_item : -1};
    BaBufs& b = w.b;
    BaExtra x;
    rs_carve ws_size, pin_size;
    ba_window_layout(ws_size, ask, w, x);
    ba_pinned_layout(pin_size, ask, w, x);
    void *ws = nullptr, *pin = nullptr;
    // (this solve keeps its own account of what it leaves behind in the workspace: ba_enqueue_setup)
    if ((rc = rs_workspace_quiet(ctx, ws_size.bytes(), &ws)) || (rc = rs_pinned(ctx, pin_size.bytes(), &pin))) return rc;
    ctx->ba_cams = nullptr; ctx->ba_cams_n = 0; ctx->ba_trace_n = 0;
    rs_carve dev(ws), host(pin);
    x = ba_bind_window(q, ask, dev, host, w);
    if (path.ns == 1) b.prog = nullptr;     // (one set per round: the kernels publish no progress; w.prog only names the line whose pad is the completion flag)
#if RS_STAMPS
    RS_HIP(ctx, hipMemsetAsync(b.dbg, 0, sizeof(unsigned long long) * BA_DBG_WORDS, ctx->stream));
#endif
    ctx->ba_cache = b.dbg;
    const size_t C = (size_t)d.C;
    const int from_mask = C <= 64 ? 1 : 0;
    if (!from_mask) {                                       // beyond the mask: both tables through the pinned block
        memcpy(x.slot, slot.data(), sizeof(int32_t) * C);
        memcpy(x.fre, q.h_cam_free, C);
        RS_HIP(ctx, hipMemcpyAsync(b.slot, x.slot, sizeof(int32_t) * C, hipMemcpyHostToDevice, ctx->stream));
        RS_HIP(ctx, hipMemcpyAsync(w.cam_free, x.fre, C, hipMemcpyHostToDevice, ctx->stream));
    }

    // kernel attributes, inertial blocks, set-up launches
    rc = ba_prepare_kernels(ctx, d, path);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    std::vector<ImuFactorDev> fac_host; std::vector<double> xv_host;      // (sources of ba_inertial_upload's copies: alive until the solve has been waited for)
    if (in && (rc = ba_inertial_upload(ctx, *in, d, b, path, x.big, x.zacc, inert, Ci, fac_host, xv_host)) != RS_OK) return rc;
    bool fused_setup = false;
    rc = ba_enqueue_setup(ctx, w, opt, path.use_mfma, ws, from_mask, &fused_setup);
    if (rc) return rc;

    // what only exists now: the band form (sharded solves agree on it) and the launch fusion
    rc = ba_choose_band(ctx, path, in != nullptr, w.g, b, x.key, &path.band);
    if (rc) return rc;
    b.hand_timeout = 100ull * (unsigned long long)ctx->ba_handoff_timeout_us;
    ba_choose_fusion(ctx, d, b, w.g, path, allow_fuse, in != nullptr, in_flight.others);
    if (path.fuse_round && ba_prepare_round(d) != 0) return rs_fail(ctx, RS_ERR_HIP, "LDS attribute (round)");

    // rounds
    int rounds = 0;
    const BaProgress* const progs[1] = {w.prog};
    rc = ba_follow_rounds(s, opt.max_iter, path.ns, progs, 1,
                          [&](int it) { return ba_enqueue_round(ctx, w, opt, path, in != nullptr, x.big, it); }, rounds);
    if (rc) return rc;
    {
        rs_prof_scope ps(ctx, "K10_ba_finalize");
        // the last decisions: round index `rounds` reads the blocks of round rounds - 1
        const int itf = rounds;
        ba_point_round(w, itf, true);
        b.prog = nullptr;
        w.prog->pad = 0;
        hipLaunchKernelGGL(ba_finalize, dim3(BA_FINALIZE_WGS), dim3(256), 0, s, d, b, opt, itf, q.d_cameras, (const uint8_t*)w.cam_free, q.d_points, w.h_st, w.h_trace,
                           w.h_cams, x.vb, &w.prog->pad, fused_setup ? w.zero_ptr : nullptr, fused_setup ? w.zero_n : 0);
        RS_HIP(ctx, hipGetLastError());
        if (fused_setup) { ctx->grp_zero_ptr = w.zero_ptr; ctx->grp_zero_n = w.zero_n; }      // stream-ordered in front of the next solve
        // wait for the completion flag the last workgroup of ba_finalize raises in pinned memory (summary, trace, camera
        // mirror are then all there); fall back to the stream if it drains without the flag (a failed launch)
        RS_HIP(ctx, ba_wait_flag(s, &w.prog->pad, itf + 1));
    }
    RS_HIP(ctx, hipGetLastError());

    // results
    ba_summary_from(*w.h_st, h_summary);
    ctx->ba_trace = w.h_trace;            // stays valid until the next call that uses the pinned block
    ctx->ba_trace_n = w.h_st->iter;
    ctx->ba_stats[0] = w.h_st->n_rounds; ctx->ba_stats[1] = w.h_st->n_fresh; ctx->ba_stats[2] = w.h_st->n_sets; ctx->ba_stats[3] = rounds;
    *hand_lost = w.h_st->hand_lost != 0;
    if (rs_comm_active(ctx) && path.may_fuse) {
        // every rank gets here (the conditions are the same on all of them: cameras are replicated), fused or not
        hipLaunchKernelGGL(ba_lost_key, dim3(1), dim3(1), 0, s, (const BaState*)b.st, b.dbg + BA_KEY_LOST);
        rc = ba_min_key_to_host(ctx, b.dbg + BA_KEY_LOST, x.key);
        if (rc) return rc;
        *hand_lost = *x.key == 0ull;
    }
    ctx->ba_cams = w.h_cams; ctx->ba_cams_n = q.n_cameras;
    if (in && w.h_st->usable) ba_inertial_unpack(*in, q, x.vb);
    return RS_OK;
}

// A lost hand-off inside the fused K7 + K8 launch (ba_backsub_body.h) says something about scheduling, not about the
// data: the inputs are untouched (nothing is written back from an unusable solve), so the solve runs once more as
// separate launches, which need no hand-off.  Counted in rs_ba_get_stats [4].
static int ba_solve_impl(rs_context* ctx, const rs_ba_problem& q, const rs_ba_options* options, rs_ba_summary* h_summary, const BaInertialArgs* in)
{
    bool lost = false;
    int rc = ba_solve_once(ctx, q, options, h_summary, in, true, &lost);
    if (rc == RS_OK && lost) {
        ctx->ba_stats[4]++;
        rc = ba_solve_once(ctx, q, options, h_summary, in, false, &lost);
    }
    return rc;
}

extern "C" int rs_bundle_adjust(rs_context* ctx, int n_cameras, int n_points, int n_obs, double* d_cameras,
                                const uint8_t* h_cam_free, double* d_points, const int32_t* d_obs_ptr,
                                const int32_t* d_obs_cam, const float* d_obs_uv, const float h_intrinsics[4],
                                const rs_ba_options* options, rs_ba_summary* h_summary)
{
    return ba_solve_impl(ctx, ba_problem_from(n_cameras, n_points, n_obs, d_cameras, h_cam_free, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, h_intrinsics),
                         options, h_summary, nullptr);
}

extern "C" int rs_bundle_adjust_inertial(rs_context* ctx, int n_cameras, int n_points, int n_obs, double* d_cameras,
                                         const uint8_t* h_cam_free, double* d_points, const int32_t* d_obs_ptr,
                                         const int32_t* d_obs_cam, const float* d_obs_uv, const float h_intrinsics[4],
                                         double* h_velocity, double* h_bias, const rs_imu_factor* h_factors, int n_factors,
                                         const double h_gravity[3], const rs_ba_options* options, rs_ba_summary* h_summary)
{
    const rs_ba_problem q = ba_problem_from(n_cameras, n_points, n_obs, d_cameras, h_cam_free, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, h_intrinsics);
    if (n_factors < 0) return ctx ? rs_fail(ctx, RS_ERR_INVALID, "negative n_factors") : RS_ERR_INVALID;
    if (n_factors == 0)                                      // InertialInput::usable() false / no pair with >= 2 samples
        return ba_solve_impl(ctx, q, options, h_summary, nullptr);
    if (!h_velocity || !h_bias || !h_factors || !h_gravity) return ctx ? rs_fail(ctx, RS_ERR_INVALID, "null pointer") : RS_ERR_INVALID;
    const BaInertialArgs in{h_velocity, h_bias, h_factors, n_factors, h_gravity};
    return ba_solve_impl(ctx, q, options, h_summary, &in);
}

// ---------------------------------------------------------------- batch of independent windows
// Several sessions served by one GPU: the windows are independent problems, each a latency chain of small launches
// that fills a fraction of the chip, so they overlap on the device when they sit on different streams.  Lanes = child
// contexts (stream + workspace + pinned block each); one host thread per lane walks its share of the windows with the
// ordinary solve (incl. the round-following logic), which keeps every lane's stream fed.

// Grid mode: the B windows run as ONE launch sequence, blockIdx.z = window (BaWin, ba_common.h).  Every kernel of the
// local-window fast path has a batched entry point that takes its per-window arguments from a device array; a round's
// K5 is then B x items workgroups (instead of 157-250), K7 B x sets workgroups (instead of <= 3), and a launch is paid
// once per round, not once per window and round.  Eligible: windows of <= 64 cameras on the MFMA / LDS path (what a
// local window is).  Returns 1 when the batch is not eligible (the caller falls back to the lanes), 0 when it ran.
static int ba_solve_batch_grid(rs_context* ctx, int B, const rs_ba_problem* Q, const rs_ba_options* options, rs_ba_summary* out, int* rc_out)
{
    *rc_out = RS_OK;
    rs_ba_options def;
    if (!options) { rs_ba_default_options(&def); options = &def; }
    const BaOpt opt = ba_opt_from(options);
    if (opt.max_iter < 1 || opt.max_iter > 1000) return 1;
    std::vector<BaWin> wins((size_t)B);
    int max_P = 0, max_items = 0, max_n = 0, max_C = 0, ns = 1;
    size_t k5_lds = 0, k8_lds = 0;
    // the single solve's window, one per problem: one rank, one copy of S, no tail; pinned without tables (the mask is the table)
    BaWinAsk a = {1, opt.max_iter, 1, 0, 1, 0, 0, 0, false, false, true, ctx->ba_batch_item};
    BaExtra x;
    // workspace: the device's table of windows, then the windows; pinned: the windows' parts, then the table's staging copy
    rs_carve ws_size, pin_size;
    ws_size.take<BaWin>((size_t)B);
    for (int i = 0; i < B; i++) {
        const rs_ba_problem& q = Q[i];
        if (q.n_cameras <= 0 || q.n_points <= 0 || q.n_obs <= 0 || q.n_cameras > 64) return 1;
        if (!q.d_cameras || !q.h_cam_free || !q.d_points || !q.d_obs_ptr || !q.d_obs_cam || !q.d_obs_uv) return 1;
        BaWin& w = wins[(size_t)i];
        memset(&w, 0, sizeof w);
        BaDims& d = w.d;
        if (!ba_dims_from(q, options, d, nullptr, &w.free_mask)) return 1;
        // the plain local-window path only, with at most three sets (throughput mode: extra radii are CU time other windows
        // want) and one copy of S whatever "ba_s_replicas" says
        const BaPath path = ba_choose_path(ctx, d, opt.max_iter, false, 0, false, BA_CALIBRATED_SETS, BA_CALIBRATED_SETS);
        if (!path.local_window()) return 1;
        a.ns = ns = path.ns;                            // (the same for every window: context and options decide it)
        a.grp_bytes = ba_group_bytes(d.P, d.Cf, d.M);
        ba_window_layout(ws_size, a, w, x);
        ba_pinned_layout(pin_size, a, w, x);
        max_P = std::max(max_P, d.P); max_n = std::max(max_n, d.n); max_C = std::max(max_C, d.C);
        k8_lds = std::max(k8_lds, ba_backsub_lds_bytes(d.C, d.n));
    }
    pin_size.take<BaWin>((size_t)B);
    void *ws = nullptr, *pin = nullptr;
    int rc = rs_workspace(ctx, ws_size.bytes(), &ws);
    if (!rc) rc = rs_pinned(ctx, pin_size.bytes(), &pin);
    if (rc) { *rc_out = rc; return 0; }
    // the same takes in the same order, now on the blocks
    rs_carve dev(ws), host(pin);
    const BaWin* d_wins = dev.take<BaWin>((size_t)B);
    std::vector<const BaProgress*> progs((size_t)B);
    for (int i = 0; i < B; i++) {
        BaWin& w = wins[(size_t)i];
        a.grp_bytes = ba_group_bytes(w.d.P, w.d.Cf, w.d.M);
        ba_bind_window(Q[i], a, dev, host, w);
        progs[(size_t)i] = w.prog;
        max_items = std::max(max_items, w.g.n_items);
        k5_lds = std::max(k5_lds, ba_schur_lds_bytes(w.d.C, w.d.Cf, w.g.it_l, ns));
    }
    if (ba_prepare_reduced_solve_lds_batch(max_n) != 0 || ba_prepare_schur_batch(k5_lds) != 0) { *rc_out = rs_fail(ctx, RS_ERR_HIP, "LDS attribute (batch)"); return 0; }
    hipStream_t s = ctx->stream;
    BaWin* h_wins = host.take<BaWin>((size_t)B);
    memcpy(h_wins, wins.data(), sizeof(BaWin) * (size_t)B);
    if (hipMemcpyAsync((void*)d_wins, h_wins, sizeof(BaWin) * (size_t)B, hipMemcpyHostToDevice, s) != hipSuccess) { *rc_out = rs_fail(ctx, RS_ERR_HIP, "window table upload"); return 0; }
    {
        rs_prof_scope ps(ctx, "K0_ba_init");
        hipLaunchKernelGGL(ba_init_batch, dim3(32, 1, B), dim3(256), 0, s, d_wins, opt);
    }
    {
        rs_prof_scope ps(ctx, "K5s_group_landmarks");
        ba_launch_grouping_batch(s, d_wins, B, max_P, max_items);
    }
    auto enqueue_round = [&](int it) {
        { rs_prof_scope ps(ctx, "K5_ba_schur_mfma"); ba_launch_decide_batch(s, d_wins, B, opt, it); ba_launch_schur_batch(s, d_wins, B, opt, it, max_items, wins[0].g.it_l, k5_lds); }
        { rs_prof_scope ps(ctx, "K7_ba_reduced_solve"); ba_launch_reduced_solve_lds_batch(s, d_wins, B, opt, it, ns, max_n); }
        { rs_prof_scope ps(ctx, "K8_ba_backsub_cost"); ba_launch_backsub_batch(s, d_wins, B, it, ns, max_P, k8_lds); }
        return (int)RS_OK;
    };
    int rounds = 0;
    (void)ba_follow_rounds(s, opt.max_iter, ns, progs.data(), B, enqueue_round, rounds);      // (the slowest window decides)
    {
        rs_prof_scope ps(ctx, "K10_ba_finalize");
        hipLaunchKernelGGL(ba_finalize_batch, dim3(16, 1, B), dim3(256), 0, s, d_wins, opt, rounds);
    }
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { *rc_out = rs_fail(ctx, RS_ERR_HIP, "batched bundle adjustment"); return 0; }
    for (int i = 0; i < B; i++) ba_summary_from(*wins[(size_t)i].h_st, &out[i]);
    ctx->ba_trace = nullptr; ctx->ba_trace_n = 0; ctx->ba_cams = nullptr; ctx->ba_cams_n = 0;
    ctx->ba_stats[0] = ctx->ba_stats[1] = ctx->ba_stats[2] = 0; ctx->ba_stats[3] = rounds;
    return 0;
}

extern "C" int rs_bundle_adjust_batch(rs_context* ctx, int n_problems, const rs_ba_problem* h_problems,
                                      const rs_ba_options* options, rs_ba_summary* h_summaries)
{
    if (!ctx || n_problems < 0 || (n_problems > 0 && (!h_problems || !h_summaries))) return RS_ERR_INVALID;
    if (n_problems == 0) return RS_OK;
    if (rs_comm_active(ctx)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "batch of windows on a landmark-sharded context");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n_problems; i++) memset(&h_summaries[i], 0, sizeof(rs_ba_summary));
    if (ctx->ba_batch_mode == 0 && n_problems > 1) {
        int rc = RS_OK;
        if (ba_solve_batch_grid(ctx, n_problems, h_problems, options, h_summaries, &rc) == 0) return rc;
    }
    const int lanes = n_problems < RS_BA_BATCH_LANES ? n_problems : RS_BA_BATCH_LANES;
    while ((int)ctx->batch_lanes.size() < lanes) {
        rs_context* c = nullptr;
        int rc = rs_context_create(ctx->device, &c);
        if (rc) return rs_fail(ctx, rc, "cannot create batch lane");
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { rs_context_destroy(c); return rs_fail(ctx, RS_ERR_HIP, "hipStreamCreate"); }
        c->stream = st;
        c->ba_sets = ctx->ba_sets;
        ctx->batch_lanes.push_back(c);
        ctx->batch_streams.push_back(st);
    }
    // the inputs were produced on the parent's stream: the lanes start after it
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> status((size_t)lanes, RS_OK);
    auto work = [&](int lane) {
        (void)hipSetDevice(ctx->device);
        rs_context* c = ctx->batch_lanes[(size_t)lane];
        c->ba_sets = ctx->ba_sets;
        for (int i = lane; i < n_problems; i += lanes) {
            const int rc = ba_solve_impl(c, h_problems[i], options, &h_summaries[i], nullptr);
            if (rc && !status[(size_t)lane]) status[(size_t)lane] = rc;
        }
    };
    std::vector<std::thread> threads;
    for (int l = 1; l < lanes; l++) threads.emplace_back(work, l);
    work(0);
    for (auto& t : threads) t.join();
    // The lanes' finalize kernels raise their host flags while the device-side copies into d_cameras / d_points may still be
    // running on the LANE streams: the parent's stream (what the caller reads the results on, and what
    // rs_context_synchronize(ctx) covers) waits for every lane stream here, whatever the windows' status.
    const int wrc = rs_context_wait_for(ctx, ctx->batch_lanes.data(), lanes);
    for (int l = 0; l < lanes; l++)
        if (status[(size_t)l]) return rs_fail(ctx, status[(size_t)l], "window on lane %d failed: %s", l, rs_last_error(ctx->batch_lanes[(size_t)l]));
    return wrc;
}

static_assert(sizeof(BaTrace) == sizeof(rs_ba_iteration), "BaTrace mirrors rs_ba_iteration");

extern "C" int rs_ba_get_trace(rs_context* ctx, rs_ba_iteration* h_out, int capacity, int* h_count)
{
    if (!ctx || !h_count || capacity < 0 || (capacity > 0 && !h_out)) return RS_ERR_INVALID;
    const int n = ctx->ba_trace ? ctx->ba_trace_n : 0;
    const int m = n < capacity ? n : capacity;
    if (m > 0) memcpy(h_out, ctx->ba_trace, sizeof(rs_ba_iteration) * (size_t)m);
    *h_count = n;
    return RS_OK;
}

extern "C" int rs_ba_get_cameras(rs_context* ctx, double* h_cameras, int n_cameras)
{
    if (!ctx || !h_cameras || n_cameras < 0) return RS_ERR_INVALID;
    if (!ctx->ba_cams || n_cameras != ctx->ba_cams_n) return rs_fail(ctx, RS_ERR_INVALID, "no bundle adjustment result of %d cameras on this context", n_cameras);
    memcpy(h_cameras, ctx->ba_cams, sizeof(double) * 6 * (size_t)n_cameras);
    return RS_OK;
}

extern "C" int rs_ba_get_stats(rs_context* ctx, int h_out[8])
{
    if (!ctx || !h_out) return RS_ERR_INVALID;
    for (int i = 0; i < 8; i++) h_out[i] = ctx->ba_stats[i];
    return RS_OK;
}
