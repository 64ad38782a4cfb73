// ba_step_body.h — the two ends of a Levenberg-Marquardt round as the single-workgroup reduced solves outside the
// local-window kernel run them: ba_big_prologue / ba_big_finish and ba_imu_prologue / ba_imu_finish (ba_solve_big.hip)
// and ba_no_free_camera (ba.hip).  The local-window K7 (ba_solve_body.h) follows the same schedule, scheduled load by
// load for its own layout.
//   front end   ba_step_begin, ba_step_gradient_test   state, accumulator fold, cost / gradient terminations, failure flag
//   back end    ba_step_camera, ba_step_reduce         delta_c = -x, candidate cameras, camera part of the step scalars
// The Jacobi scale and the damping stay with the kernels (they index different arrays per form).  Every function is
// called by all threads of the workgroup (256, 512 or 1024); `st` and `fail` are words the workgroup shares, the LDS
// scratch `red` / `red3` has one entry per wave (16).
#pragma once
#include "ba_common.h"

// Loads the state block and clears *fail (false: the solve has terminated, nothing was touched); then clears the step
// scalars K8 of this iteration accumulates into and folds the BA_UREP replicas of the camera-side accumulators into
// replica 0.  The caller's next barrier publishes the fold.
__device__ __forceinline__ bool ba_step_begin(const BaDims& d, const BaBufs& b, BaState* st, int* fail)
{
    const int n = d.n, tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) { *st = *b.st; *fail = 0; }
    __syncthreads();
    if (st->done) return false;
    for (int i = tid; i < BA_NSLOT * BA_SLOT_STRIDE; i += nt) b.pt_scal[i] = 0.0;
    for (size_t i = tid; i < b.cam_stride; i += nt) {
        double v = 0.0;
        for (int r = 0; r < BA_UREP; r++) v += b.rhs[(size_t)r * b.cam_stride + i];
        // U | gc are only accumulated on fresh iterations (K5 skips its first pass after a rejected step)
        if ((int)i >= n) { if (st->fresh) b.Ukeep[i - n] = v; else v = b.Ukeep[i - n]; }
        b.rhs[i] = v;
    }
    return true;
}

// Fresh linearisation: `cost` (thread 0's value counts) becomes the cost at x, and the largest gradient entry — `gm` of
// every thread, K5's slot lines for the landmarks — is held against the tolerance.  Always: K5's "bad landmark block"
// count raises *fail, and the state is stored.  False: the solve has terminated.
__device__ __forceinline__ bool ba_step_gradient_test(const BaBufs& b, const BaOpt& opt, BaState* st, int* fail, double* red, double gm, double cost)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    if (st->fresh) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gm = fmax(gm, __shfl_down(gm, off, 64));
        if ((tid & 63) == 0) red[tid >> 6] = gm;
        __syncthreads();
        double gslots = 0.0;
        if (tid < 64) gslots = slot_max_all(b);
        if (tid == 0) {
            st->x_cost = cost;
            if (st->iter == 0) st->initial_cost = st->x_cost;
            double gg = gslots;
            for (int w = 0; w < (nt + 63) / 64; w++) gg = fmax(gg, red[w]);
            if (!isfinite(st->x_cost)) { st->done = 1; st->termination = RS_BA_FAILURE; }
            else if (gg <= opt.gtol) { st->done = 1; st->termination = RS_BA_CONVERGENCE_GRADIENT; }
            else if (st->iter >= opt.max_iter) { st->done = 1; st->termination = RS_BA_NO_CONVERGENCE; }   // max_num_iterations 0: the costs and these two exits, no step
        }
    }
    __syncthreads();
    if (tid < 64) { const double f = slot_sum(b.scal, 1); if (f > 0.0 && tid == 0) *fail = 1; }
    if (tid == 0) *b.st = *st;
    return !st->done;
}

// Camera c of the step: delta_c = -x (x = the solve's result, `lam` / `grad` the damping and the gradient it was solved
// with), the candidate camera and its prepared block; adds the camera's terms of the model cost change, of the step
// norm and of the x norm to acc[0..2].  The norms count a camera that has observations — or that the caller says is
// in the problem anyway (also_active).  True: the step is not finite.
__device__ __forceinline__ bool ba_step_camera(const BaDims& d, const BaBufs& b, const BaState& st, int c, const double* x, const double* lam,
                                               const double* grad, bool also_active, double acc[3])
{
    const double* Xc = b.Xc + (size_t)st.cur * d.C * 6;
    double* Xn = b.Xc + (size_t)(st.cur ^ 1) * d.C * 6;
    const int s = b.slot[c];
    bool active = also_active, bad = false;
    if (s >= 0)
        for (int k = 0; k < 6; k++) active = active || b.U[s * 36 + k * 7] > 0.0;
    for (int k = 0; k < 6; k++) {
        const double xc = Xc[6 * c + k];
        if (s >= 0) {
            const double dlt = -x[6 * s + k];
            if (!isfinite(dlt)) bad = true;
            acc[0] += 0.5 * (dlt * dlt * lam[6 * s + k] - dlt * grad[6 * s + k]);
            const double xn = xc + dlt;
            if (active) { acc[1] += (xc - xn) * (xc - xn); acc[2] += xc * xc; }
            Xn[6 * c + k] = xn;
            b.dc[6 * s + k] = dlt;                          // K8 back-substitutes the points with it
        } else {
            Xn[6 * c + k] = xc;
        }
    }
    cam_prepare(Xn + 6 * c, b.prep + ((size_t)(st.cur ^ 1) * d.C + c) * BA_PREP);
    return bad;
}

// The threads' partial sums, wave by wave and then serially in thread 0, into cam_scal[0..2]; solver_failed when a
// thread saw a non-finite step (or *fail was already raised).  The result is in *st for thread 0, which stores it.
__device__ __forceinline__ void ba_step_reduce(BaState* st, int* fail, double (*red3)[3], const double acc[3], bool bad)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const double mcc = wave_sum(acc[0]), ssq = wave_sum(acc[1]), xsq = wave_sum(acc[2]);
    if (__any(bad) && (tid & 63) == 0) *fail = 1;
    if ((tid & 63) == 0) { red3[tid >> 6][0] = mcc; red3[tid >> 6][1] = ssq; red3[tid >> 6][2] = xsq; }
    __syncthreads();
    if (tid == 0) {
        double a0 = 0, a1 = 0, a2 = 0;
        for (int w = 0; w < (nt + 63) / 64; w++) { a0 += red3[w][0]; a1 += red3[w][1]; a2 += red3[w][2]; }
        st->cam_scal[0] = a0; st->cam_scal[1] = a1; st->cam_scal[2] = a2;
        st->solver_failed = *fail;
    }
}
