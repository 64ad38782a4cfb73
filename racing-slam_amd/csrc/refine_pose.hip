// refine_pose.hip — K11, the pose solve of one frame against constant points, in f64.
//
// Replaces optimization::refine_pose's ceres::Solve (reference src/Optimization.cpp:194-267): vision only (one camera
// block, 6 unknowns), or with a RotationPrior (:252-258: 3 more residuals on the pose block) or an InertialDelta
// (:237-251: the 9-residual preintegration block with the previous frame constant and this frame's velocity as a second
// free block -> 9 unknowns).  The whole LM loop (the schedule of ba.hip's head comment) runs inside ONE launch of a single
// workgroup: per iteration a block reduction of the 6x6 normal equations of the observations, the one extra block
// evaluated with dual numbers (imu_dual.h), a register Cholesky of the nu x nu system (nu = 6 or 9) on lane 0 and a second
// reduction for the candidate cost.  The two kernels are one body, rp_body, compiled with and without the extra block.
#include "ba_blocks.h"

#define RP_THREADS 512         // 2000 observations: four per thread; 256 VGPRs per thread keep the 28 accumulators in registers

__device__ __forceinline__ void block_sum(double* vals, int count, double* scratch /*[RP_THREADS / 64 + 1][32]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < count; k++) {
        const double v = wave_sum_lane63(vals[k]);
        if (lane == 63) scratch[wave * 32 + k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < count) {                 // thread k folds the waves' partial sums of value k (fixed order)
        double t = 0.0;
        for (int w = 0; w < RP_THREADS / 64; w++) t += scratch[w * 32 + threadIdx.x];
        scratch[(RP_THREADS / 64) * 32 + threadIdx.x] = t;
    }
    __syncthreads();
    for (int k = 0; k < count; k++) vals[k] = scratch[(RP_THREADS / 64) * 32 + k];
    __syncthreads();
}

// ---- the pieces of one LM iteration.  Thread 0 runs the serial ones; nx = 6 (pose) or 9 (pose, velocity) state entries.
__device__ __forceinline__ void rp_init(const BaOpt& opt, const double* cam_io, int nx, double* x, double* prep, BaState& st)
{
    for (int k = 0; k < nx; k++) x[k] = cam_io[k];
    cam_prepare(x, prep);
    st.radius = opt.r0; st.decrease_factor = 2.0; st.x_cost = 0.0; st.initial_cost = 0.0;
    st.iter = 0; st.successful = 0; st.invalid_steps = 0; st.done = 0; st.termination = 0; st.cur = 0;
    st.have_scale = 0; st.solver_failed = 0; st.fresh = 1; st.usable = 0; st.consec_accepts = 0; st.nact = 1;
    st.n_rounds = 0; st.n_fresh = 0; st.n_sets = 0; st.hand_lost = 0;
}

// this thread's share of the observations' normal equations: acc = upper triangle of J'WJ (21) | J'Wr (6) | cost
__device__ __forceinline__ void rp_linearize(const BaDims& d, const double* prep, const double* __restrict__ pts,
                                             const float2* __restrict__ uv, int n, double (&acc)[28])
{
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    ObsLin o;
    for (int i = threadIdx.x; i < n; i += RP_THREADS) {
        const double X[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
        obs_eval<true>(prep, X, uv[i], d, o);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int e = a; e < 6; e++) acc[q++] += o.w * (o.jc[a] * o.jc[e] + o.jc[6 + a] * o.jc[6 + e]);
        }
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += o.w * (o.jc[a] * o.r0 + o.jc[6 + a] * o.r1);
        acc[27] += 0.5 * o.rho;
    }
}

// this thread's share of the observations' cost at the candidate
__device__ __forceinline__ double rp_candidate_cost(const BaDims& d, const double* prepn, const double* __restrict__ pts,
                                                    const float2* __restrict__ uv, int n)
{
    double c = 0.0;
    ObsLin o;
    for (int i = threadIdx.x; i < n; i += RP_THREADS) {
        const double X[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
        obs_eval<false>(prepn, X, uv[i], d, o);
        c += 0.5 * o.rho;
    }
    return c;
}

// the reduced sums as H (the pose block; zero beyond it) and g; returns the cost
template <int MAXN>
__device__ __forceinline__ double rp_unpack(const double (&acc)[28], double (&H)[MAXN][MAXN], double (&g)[MAXN])
{
    for (int a = 0; a < MAXN; a++) { g[a] = 0.0; for (int e = 0; e < MAXN; e++) H[a][e] = 0.0; }
    int q = 0;
    for (int a = 0; a < 6; a++)
        for (int e = a; e < 6; e++) { H[a][e] = acc[q]; H[e][a] = acc[q]; q++; }
    for (int a = 0; a < 6; a++) g[a] = acc[21 + a];
    return acc[27];
}

// the extra residual block at x: the first 32 lanes evaluate it with one partial per lane (imu_dual.h) and leave
// residual + Jacobian in LDS for the solving thread
__device__ __forceinline__ void rp_extra_lanes(const RpInertial* __restrict__ ext, const double* x, double* s_extr, double (*s_extJ)[IMU_NP])
{
    const int tid = threadIdx.x;
    if (ext->kind == 1) {
        double r[3], jl[3];
        imu_rotation_prior_lanes(ext->predicted, ext->sigma, x, r, jl);
        for (int a = 0; a < 3; a++) { if (tid < 3) s_extJ[a][tid] = jl[a]; if (tid == 0) s_extr[a] = r[a]; }
    } else {
        double r[9], jl[9];
        imu_preintegration_lanes(ext->fac, ext->gravity, ext->prev_pose, ext->prev_vel, ext->prev_bias, x, x + 6, r, jl);
        for (int a = 0; a < 9; a++) { if (tid < IMU_NP) s_extJ[a][tid] = jl[a]; if (tid == 0) s_extr[a] = r[a]; }
    }
}

// ... folded into H, g and the cost
__device__ __forceinline__ void rp_extra_fold(int kind, const double* s_extr, const double (*s_extJ)[IMU_NP], double (&H)[9][9],
                                              double (&g)[9], double& cost)
{
    if (kind == 1) {
        for (int a = 0; a < 3; a++) {
            cost += 0.5 * s_extr[a] * s_extr[a];
            for (int k = 0; k < 3; k++) { g[k] += s_extJ[a][k] * s_extr[a]; for (int l = 0; l < 3; l++) H[k][l] += s_extJ[a][k] * s_extJ[a][l]; }
        }
    } else {
        for (int a = 0; a < 9; a++) {
            cost += 0.5 * s_extr[a] * s_extr[a];
            for (int k = 0; k < 9; k++) {            // local parameters 15..23 = pose_j (6), velocity_j (3)
                const double jk = s_extJ[a][15 + k];
                g[k] += jk * s_extr[a];
                for (int l = 0; l < 9; l++) H[k][l] += jk * s_extJ[a][15 + l];
            }
        }
    }
}

// ... and its cost at the candidate
__device__ __forceinline__ double rp_extra_cost(const RpInertial* __restrict__ ext, const double* xn)
{
    double ce = 0.0;
    if (ext->kind == 1) {
        double r[3];
        imu_rotation_prior(ext->predicted, ext->sigma, xn, r, nullptr);
        for (int a = 0; a < 3; a++) ce += 0.5 * r[a] * r[a];
    } else {
        double r[9];
        imu_preintegration(ext->fac, ext->gravity, ext->prev_pose, ext->prev_vel, ext->prev_bias, xn, xn + 6, r, nullptr);
        for (int a = 0; a < 9; a++) ce += 0.5 * r[a] * r[a];
    }
    return ce;
}

// what ends the loop in front of a step: a fresh linearisation's cost and gradient, then the iteration limit
template <int MAXN>
__device__ __forceinline__ void rp_check(const BaOpt& opt, BaState& st, int nu, const double (&H)[MAXN][MAXN], const double (&g)[MAXN],
                                         double cost, double* sc)
{
    if (st.fresh) {
        st.x_cost = cost;
        if (st.iter == 0) st.initial_cost = st.x_cost;
        if (!st.have_scale)
            for (int a = 0; a < nu; a++) sc[a] = opt.jacobi ? 1.0 / (1.0 + sqrt(H[a][a])) : 1.0;
        double gm = 0.0;
        for (int a = 0; a < nu; a++) gm = fmax(gm, fabs(g[a]));
        if (!isfinite(st.x_cost)) { st.done = 1; st.termination = RS_BA_FAILURE; }
        else if (gm <= opt.gtol) { st.done = 1; st.termination = RS_BA_CONVERGENCE_GRADIENT; }
    }
    if (!st.done && st.iter >= opt.max_iter) { st.done = 1; st.termination = RS_BA_NO_CONVERGENCE; }
}

// the damped nu x nu system by Cholesky: candidate xn / prepn and the step scalars st.cam_scal[0..2]; true when it failed
template <int MAXN, bool RECIPROCAL>
__device__ __forceinline__ bool rp_solve(const BaOpt& opt, BaState& st, int nu, double (&H)[MAXN][MAXN], const double (&g)[MAXN],
                                         const double* sc, const double* x, double* xn, double* prepn)
{
    double lam[MAXN], dlt[MAXN], rdiag[MAXN];
    for (int a = 0; a < nu; a++) {
        const double s2 = sc[a] * sc[a];
        lam[a] = clampd(s2 * H[a][a], opt.dmin, opt.dmax) / (st.radius * s2);
        H[a][a] += lam[a];
    }
    // s over the diagonal entry j of the factor.  The vision-only kernel runs once per frame and was tuned to one reciprocal
    // per column (this is one lane's serial code); the inertial one divides, and each keeps its arithmetic
    auto over = [&](double s, int j) { return RECIPROCAL ? s * rdiag[j] : s / H[j][j]; };
    for (int j = 0; j < nu; j++) {
        double dj = H[j][j];
        for (int k = 0; k < j; k++) dj -= H[j][k] * H[j][k];
        if (!(dj > 0.0) || !isfinite(dj)) return true;
        dj = sqrt(dj);
        H[j][j] = dj;
        if (RECIPROCAL) rdiag[j] = 1.0 / dj;
        for (int i = j + 1; i < nu; i++) {
            double s = H[i][j];
            for (int k = 0; k < j; k++) s -= H[i][k] * H[j][k];
            H[i][j] = over(s, j);
        }
    }
    for (int i = 0; i < nu; i++) {
        double s = g[i];
        for (int k = 0; k < i; k++) s -= H[i][k] * dlt[k];
        dlt[i] = over(s, i);
    }
    for (int i = nu - 1; i >= 0; i--) {
        double s = dlt[i];
        for (int k = i + 1; k < nu; k++) s -= H[k][i] * dlt[k];
        dlt[i] = over(s, i);
    }
    bool fail = false;
    double mcc = 0.0, ssq = 0.0, xsq = 0.0;
    for (int a = nu; a < MAXN; a++) xn[a] = x[a];       // a rotation prior carries the velocity along
    for (int a = 0; a < nu; a++) {
        dlt[a] = -dlt[a];
        if (!isfinite(dlt[a])) fail = true;
        mcc += 0.5 * (dlt[a] * dlt[a] * lam[a] - dlt[a] * g[a]);
        xn[a] = x[a] + dlt[a];
        ssq += (x[a] - xn[a]) * (x[a] - xn[a]);
        xsq += x[a] * x[a];
    }
    st.cam_scal[0] = mcc; st.cam_scal[1] = ssq; st.cam_scal[2] = xsq;
    cam_prepare(xn, prepn);
    return fail;
}

// The accept / reject decision.  Not ba_apply_decision (ba_common.h): that one tests the iteration limit right behind
// the decision, this loop in front of the next step, after the fresh linearisation's gradient test (rp_check) — a step
// accepted on the last allowed iteration can still end in CONVERGENCE_GRADIENT here.
__device__ __forceinline__ void rp_decide(const BaOpt& opt, BaState& st, double cand, int nx, double* x, const double* xn,
                                          double* prep, const double* prepn)
{
    st.iter++;
    const double mcc = st.cam_scal[0];
    st.fresh = 0;
    if (st.solver_failed || !(mcc > 0.0)) {
        if (++st.invalid_steps >= opt.max_invalid) { st.done = 1; st.termination = RS_BA_FAILURE; }
        else { st.radius /= st.decrease_factor; st.decrease_factor *= 2.0; }
    } else {
        st.invalid_steps = 0;
        const double step_norm = sqrt(st.cam_scal[1]), x_norm = sqrt(st.cam_scal[2]);
        if (step_norm <= opt.ptol * (x_norm + opt.ptol)) { st.done = 1; st.termination = RS_BA_CONVERGENCE_PARAMETER; }
        else if (fabs(st.x_cost - cand) <= opt.ftol * st.x_cost) { st.done = 1; st.termination = RS_BA_CONVERGENCE_FUNCTION; }
        else {
            const double rel = (st.x_cost - cand) / mcc;
            if (rel > opt.min_rel && isfinite(cand)) {
                for (int a = 0; a < nx; a++) x[a] = xn[a];
                for (int a = 0; a < BA_PREP; a++) prep[a] = prepn[a];
                st.successful++;
                const double t = 2.0 * rel - 1.0;
                st.radius = fmin(opt.rmax, st.radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                st.decrease_factor = 2.0;
                st.fresh = 1;
                st.x_cost = cand;
            } else {
                st.radius /= st.decrease_factor;
                st.decrease_factor *= 2.0;
                if (st.radius < opt.rmin) { st.done = 1; st.termination = RS_BA_CONVERGENCE_RADIUS; }
            }
        }
    }
    st.solver_failed = 0;
    st.have_scale = 1;
}

__device__ __forceinline__ void rp_finish(BaState& st, int nx, const double* x, double* cam_io, BaState* st_out, volatile int* host_done)
{
    st.usable = (st.termination != RS_BA_FAILURE && isfinite(st.x_cost) && st.x_cost <= st.initial_cost) ? 1 : 0;
    if (st.usable)
        for (int k = 0; k < nx; k++) cam_io[k] = x[k];
    *st_out = st;
    __threadfence_system();           // cam_io / st_out are pinned host memory
    *host_done = 1;                   // the host spins on this instead of synchronising the stream
    __threadfence_system();
}

// INERTIAL: the state is pose + velocity (cam_io[9]) and *ext holds the extra block; else the pose alone and ext is null.
// d_n non-null: the count is d_n[0], read here and reported in *n_used; <= 0 ends the launch before the solve (the
// completion flag is raised, cam_io and st_out stay as they are).
template <bool INERTIAL>
__device__ __forceinline__ void rp_body(const BaDims& d, const BaOpt& opt, const double* __restrict__ pts, const float2* __restrict__ uv,
                                        int n, const int* __restrict__ d_n, const RpInertial* __restrict__ ext, double* __restrict__ cam_io,
                                        BaState* __restrict__ st_out, volatile int* host_done, int* __restrict__ n_used)
{
    constexpr int NX = INERTIAL ? 9 : 6;
    __shared__ double x[NX], xn[NX], prep[BA_PREP], prepn[BA_PREP], scratch[(RP_THREADS / 64 + 1) * 32];
    __shared__ double s_extr[9], s_extJ[9][IMU_NP];       // (the inertial form's)
    __shared__ BaState st;
    __shared__ double sc[NX];
    const int tid = threadIdx.x;
    int nu = 6;
    if constexpr (INERTIAL) nu = ext->kind == 2 ? 9 : 6;
    if (d_n) {
        n = d_n[0];
        if (tid == 0) *n_used = n;
        if (n <= 0) {
            if (tid == 0) { __threadfence_system(); *host_done = 1; __threadfence_system(); }
            return;
        }
    }
    if (tid == 0) rp_init(opt, cam_io, NX, x, prep, st);
    __syncthreads();
    double acc[28];
    while (true) {
        // linearise at x (recomputed after a rejected step too: same values)
        rp_linearize(d, prep, pts, uv, n, acc);
        if constexpr (INERTIAL) {
            if (tid < 32) rp_extra_lanes(ext, x, s_extr, s_extJ);
        }
        block_sum(acc, 28, scratch);
        if (tid == 0) {
            double H[NX][NX], g[NX];
            double cost = rp_unpack(acc, H, g);
            if constexpr (INERTIAL) rp_extra_fold(ext->kind, s_extr, s_extJ, H, g, cost);
            rp_check(opt, st, nu, H, g, cost, sc);
            if (!st.done) {
                const bool fail = rp_solve<NX, !INERTIAL>(opt, st, nu, H, g, sc, x, xn, prepn);
                if constexpr (INERTIAL) {
                    if (!fail) st.cam_scal[3] = rp_extra_cost(ext, xn);
                }
                st.solver_failed = fail ? 1 : 0;
            }
        }
        __syncthreads();
        if (st.done) break;
        double cc[1] = {0.0};
        if (!st.solver_failed) cc[0] = rp_candidate_cost(d, prepn, pts, uv, n);
        block_sum(cc, 1, scratch);
        if (tid == 0) {
            double cand = cc[0];
            if constexpr (INERTIAL) cand += st.cam_scal[3];
            rp_decide(opt, st, cand, NX, x, xn, prep, prepn);
        }
        __syncthreads();
        if (st.done) break;
    }
    if (tid == 0) rp_finish(st, NX, x, cam_io, st_out, host_done);
}

__global__ __launch_bounds__(RP_THREADS) void ba_refine_pose(BaDims d, BaOpt opt, const double* __restrict__ pts,
                                                            const float2* __restrict__ uv, int n,
                                                            double* __restrict__ cam_io, BaState* __restrict__ st_out, volatile int* host_done)
{
    rp_body<false>(d, opt, pts, uv, n, nullptr, nullptr, cam_io, st_out, host_done, nullptr);
}

__global__ __launch_bounds__(RP_THREADS) void ba_refine_pose_inertial(BaDims d, BaOpt opt, const double* __restrict__ pts,
                                                                     const float2* __restrict__ uv, int n,
                                                                     const RpInertial* __restrict__ ext,
                                                                     double* __restrict__ cam_io /*[9]: pose, velocity*/,
                                                                     BaState* __restrict__ st_out, volatile int* host_done)
{
    rp_body<true>(d, opt, pts, uv, n, nullptr, ext, cam_io, st_out, host_done, nullptr);
}

// the two kernels above on a count that lives on the device (rs_map_refine_pose: the gather kernel has just written it)
__global__ __launch_bounds__(RP_THREADS) void ba_refine_pose_dn(BaDims d, BaOpt opt, const double* __restrict__ pts,
                                                               const float2* __restrict__ uv, const int* __restrict__ d_n,
                                                               double* __restrict__ cam_io, BaState* __restrict__ st_out,
                                                               volatile int* host_done, int* __restrict__ n_used)
{
    rp_body<false>(d, opt, pts, uv, 0, d_n, nullptr, cam_io, st_out, host_done, n_used);
}

__global__ __launch_bounds__(RP_THREADS) void ba_refine_pose_inertial_dn(BaDims d, BaOpt opt, const double* __restrict__ pts,
                                                                        const float2* __restrict__ uv, const int* __restrict__ d_n,
                                                                        const RpInertial* __restrict__ ext, double* __restrict__ cam_io,
                                                                        BaState* __restrict__ st_out, volatile int* host_done,
                                                                        int* __restrict__ n_used)
{
    rp_body<true>(d, opt, pts, uv, 0, d_n, ext, cam_io, st_out, host_done, n_used);
}

// ---------------------------------------------------------------------- host
// the inertial constraint of one solve as the caller passed it (null for a vision-only solve)
struct RpInertialArgs {
    int kind;                 // 1 rotation prior, 2 inertial delta
    const double* predicted; double sigma;
    const double *prev_pose, *prev_velocity, *prev_bias;
    const rs_imu_factor* delta;
    const double* gravity;
    double* velocity;         // [3] in/out (inertial delta)
};

// d_n null: n observations, as the caller counted them.  d_n non-null: at most n, the count is d_n[0] on the device; it
// comes back in *h_n_used, and <= 0 means no solve ran (zeroed summary, h_camera untouched).
static int refine_pose_solve(rs_context* ctx, double h_camera[6], const double* d_points, const float* d_uv, int n,
                             const float h_intrinsics[4], const RpInertialArgs* in, const rs_ba_options* options, rs_ba_summary* h_summary,
                             const int32_t* d_n = nullptr, int* h_n_used = nullptr)
{
    if (!ctx || !h_summary) return RS_ERR_INVALID;
    memset(h_summary, 0, sizeof *h_summary);     // a refused call leaves a zeroed summary too
    if (!h_camera) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (n < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative n");
    if (n == 0 && !d_n) return RS_OK;   // "nothing to constrain", src/Optimization.cpp:227-229 (checked before the inertial block is added)
    if (!d_points || !d_uv || !h_intrinsics) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (in && in->kind == 2 && (!in->prev_pose || !in->prev_velocity || !in->prev_bias || !in->gravity || !in->velocity))
        return rs_fail(ctx, RS_ERR_INVALID, "null pointer (inertial delta)");
    rs_ba_options def;
    if (!options) { rs_ba_default_options(&def); options = &def; }
    RS_HIP(ctx, hipSetDevice(ctx->device));
    BaDims d;
    d.C = 1; d.Cf = 1; d.P = n; d.M = n; d.n = 6;       // with d_n, P and M are only the upper bound: rp_body takes its own n, not these
    d.fx = h_intrinsics[0]; d.fy = h_intrinsics[1]; d.cx = h_intrinsics[2]; d.cy = h_intrinsics[3];
    d.huber_a = options->huber_delta;
    const BaOpt opt = ba_opt_from(options);
    // the call's blocks: the inertial constraint in the workspace, where the inner loops read it; the pinned block (ba_blocks.h)
    RpInertial *d_ext = nullptr, *h_ext = nullptr;
    double* h_cam; BaState* h_st; volatile int* h_done; int* h_nu;
    int rc;
    if (in && (rc = rs_carve_from(ctx, rs_workspace, [&](rs_carve& c) { d_ext = c.take<RpInertial>(1); }))) return rc;
    if ((rc = rs_carve_from(ctx, rs_pinned, [&](rs_carve& c) { rp_pinned_layout(c, in != nullptr, h_cam, h_st, h_done, h_nu, h_ext); }))) return rc;
    ctx->ba_trace_n = 0;                 // the pinned block is reused: the last BA's record is gone
    ctx->ba_cams = nullptr;
    ctx->ba_cams_n = 0;
    *h_nu = 0;
    memcpy(h_cam, h_camera, 6 * sizeof(double));
    hipStream_t s = ctx->stream;
    if (in) {
        memset(h_ext, 0, sizeof *h_ext);
        h_ext->kind = in->kind;
        if (in->kind == 1) {
            memcpy(h_ext->predicted, in->predicted, sizeof h_ext->predicted);
            h_ext->sigma = in->sigma;
        } else {
            memcpy(h_ext->prev_pose, in->prev_pose, sizeof h_ext->prev_pose);
            memcpy(h_ext->prev_vel, in->prev_velocity, sizeof h_ext->prev_vel);
            memcpy(h_ext->prev_bias, in->prev_bias, sizeof h_ext->prev_bias);
            memcpy(h_ext->gravity, in->gravity, sizeof h_ext->gravity);
            h_ext->fac.f = *in->delta;
            imu_whitener(in->delta->covariance, h_ext->fac.W);
        }
        for (int k = 0; k < 3; k++) h_cam[6 + k] = (in->kind == 2) ? in->velocity[k] : 0.0;
        RS_HIP(ctx, hipMemcpyAsync(d_ext, h_ext, sizeof(RpInertial), hipMemcpyHostToDevice, s));   // read in the inner loops: device memory
    }
    {
        // the kernel reads the camera from and writes camera + state to the PINNED block itself: no copy launches around
        // a 40 us kernel (three hipMemcpyAsync cost more than the solve)
        rs_prof_scope ps(ctx, in ? "K11_refine_pose_inertial" : "K11_refine_pose");
        *h_done = 0;
        if (d_n && in)
            hipLaunchKernelGGL(ba_refine_pose_inertial_dn, dim3(1), dim3(RP_THREADS), 0, s, d, opt, d_points, (const float2*)d_uv, (const int*)d_n,
                               (const RpInertial*)d_ext, h_cam, h_st, h_done, h_nu);
        else if (d_n)
            hipLaunchKernelGGL(ba_refine_pose_dn, dim3(1), dim3(RP_THREADS), 0, s, d, opt, d_points, (const float2*)d_uv, (const int*)d_n, h_cam,
                               h_st, h_done, h_nu);
        else if (in)
            hipLaunchKernelGGL(ba_refine_pose_inertial, dim3(1), dim3(RP_THREADS), 0, s, d, opt, d_points, (const float2*)d_uv, n,
                               (const RpInertial*)d_ext, h_cam, h_st, h_done);
        else
            hipLaunchKernelGGL(ba_refine_pose, dim3(1), dim3(RP_THREADS), 0, s, d, opt, d_points, (const float2*)d_uv, n, h_cam, h_st, h_done);
        RS_HIP(ctx, hipGetLastError());
        RS_HIP(ctx, ba_wait_flag(s, h_done, 1));
    }
    RS_HIP(ctx, hipGetLastError());
    if (d_n) {
        if (h_n_used) *h_n_used = *h_nu;
        if (*h_nu <= 0) return RS_OK;
    }
    if (h_st->usable) {
        memcpy(h_camera, h_cam, 6 * sizeof(double));
        if (in && in->kind == 2) memcpy(in->velocity, h_cam + 6, 3 * sizeof(double));    // unpack_inertial, :263-265
    }
    ba_summary_from(*h_st, h_summary);
    return RS_OK;
}

extern "C" int rs_refine_pose(rs_context* ctx, double h_camera[6], const double* d_points, const float* d_uv, int n,
                              const float h_intrinsics[4], const rs_ba_options* options, rs_ba_summary* h_summary)
{
    return refine_pose_solve(ctx, h_camera, d_points, d_uv, n, h_intrinsics, nullptr, options, h_summary);
}

extern "C" int rs_refine_pose_inertial(rs_context* ctx, double h_camera[6], const double* d_points, const float* d_uv, int n,
                                       const float h_intrinsics[4], int kind, const double h_predicted[9], double sigma_radians,
                                       const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                                       const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                                       const rs_ba_options* options, rs_ba_summary* h_summary)
{
    if (!ctx || !h_summary) return RS_ERR_INVALID;
    memset(h_summary, 0, sizeof *h_summary);     // a refused call leaves a zeroed summary too
    if (!h_camera) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (kind < 0 || kind > 2) return rs_fail(ctx, RS_ERR_INVALID, "kind must be 0, 1 or 2");
    // RotationPrior::enabled / InertialDelta::enabled (src/Optimization.h:50-53,60-63): a disabled constraint is no constraint
    if (kind == 1 && (!h_predicted || !(sigma_radians > 0.0))) kind = 0;
    if (kind == 2 && (!h_delta || !(h_delta->duration > 0.0))) kind = 0;
    const RpInertialArgs in = {kind, h_predicted, sigma_radians, h_prev_pose, h_prev_velocity, h_prev_bias, h_delta, h_gravity, h_velocity};
    return refine_pose_solve(ctx, h_camera, d_points, d_uv, n, h_intrinsics, kind ? &in : nullptr, options, h_summary);
}

int rs_refine_pose_device_n(rs_context* ctx, double h_camera[6], const double* d_points, const float* d_uv, const int32_t* d_n, int max_n,
                            const float h_intrinsics[4], int kind, const double h_predicted[9], double sigma_radians,
                            const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                            const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                            const rs_ba_options* options, rs_ba_summary* h_summary, int* h_n_used)
{
    if (!ctx || !h_summary) return RS_ERR_INVALID;
    memset(h_summary, 0, sizeof *h_summary);
    if (!h_camera || !d_n) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (kind < 0 || kind > 2) return rs_fail(ctx, RS_ERR_INVALID, "kind must be 0, 1 or 2");
    if (kind == 1 && (!h_predicted || !(sigma_radians > 0.0))) kind = 0;      // (as rs_refine_pose_inertial)
    if (kind == 2 && (!h_delta || !(h_delta->duration > 0.0))) kind = 0;
    const RpInertialArgs in = {kind, h_predicted, sigma_radians, h_prev_pose, h_prev_velocity, h_prev_bias, h_delta, h_gravity, h_velocity};
    return refine_pose_solve(ctx, h_camera, d_points, d_uv, max_n, h_intrinsics, kind ? &in : nullptr, options, h_summary, d_n, h_n_used);
}
