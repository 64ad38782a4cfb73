// pose_shared.h — what the relative-pose stage (pose.hip) and the absolute-pose stage (pnp.hip) share: the RANSAC frame
// (ransac.h: the hashed draw, the hypothesis table, the best-model key, the adaptive stop, the inlier compaction and the
// host side of an estimator) and the numeric helpers below: the integer workgroup sum, polynomial helpers of the bisection
// root finders (ordered 64-bit keys), cyclic Jacobi (serial and workgroup-wide) and the one-sided Jacobi 3 x 3 SVD.
// Each follows tests/essential_ref.py operation by operation; both stages are compiled with -ffp-contract=off.
#pragma once
#include <climits>
#include <cmath>

#include "common.h"
#include "ransac.h"

#define POSE_TRIM_EPS 1e-30
#define POSE_BISECT_ITERS 64
#define POSE_NEWTON 3
#define POSE_SWEEPS 16
#define POSE_JACOBI_TOL 1e-30       // a sweep starts only while sum(off-diagonal^2) > 1e-30 sum(diagonal^2)

__device__ __forceinline__ int block_sum_int(int v, int* red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    int t = 0;
    for (int i = 0; i < nw; i++) t += red[i];
    __syncthreads();
    return t;
}

__device__ __forceinline__ void pmul(const double* a, int na, const double* b, int nb, double* out)
{
    for (int k = 0; k < na + nb - 1; k++) out[k] = 0.0;
    for (int i = 0; i < na; i++)
        for (int j = 0; j < nb; j++) out[i + j] = out[i + j] + a[i] * b[j];
}

// the sign of the degree-j polynomial c (ascending) at x
__device__ __forceinline__ int poly_sign(const double* c, int j, double x)
{
    double v = c[j];
    for (int k = j - 1; k >= 0; k--) v = v * x + c[k];
    return (v > 0.0) - (v < 0.0);
}

// f64 <-> int64 keys in the order of the values (+0 and -0 both 0)
__device__ __forceinline__ long long dkey(double x)
{
    const long long i = __double_as_longlong(x);
    return i < 0 ? LLONG_MIN - i : i;
}

__device__ __forceinline__ double dunkey(long long k)
{
    return __longlong_as_double(k < 0 ? LLONG_MIN - k : k);
}

__device__ __forceinline__ double horner_up(const double* c, int n, double z)
{
    double v = 0.0;
    for (int k = n - 1; k >= 0; k--) v = v * z + c[k];
    return v;
}

// cyclic Jacobi on a symmetric n x n in A (row-major, stride n), eigenvectors in V; serial (one thread)
__device__ void jacobi_eigen(double* A, double* V, int n)
{
    for (int i = 0; i < n * n; i++) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < n; p++) {
            diag = diag + A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; q++) off = off + A[p * n + q] * A[p * n + q];
        }
        if (!(off > POSE_JACOBI_TOL * diag)) break;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
}

// the same cyclic Jacobi with the whole workgroup: every thread derives (c, s) from LDS, threads k < n rotate column k's
// pair, then row k's pair and V's; each phase touches disjoint entries, so the result is the serial one bit for bit
__device__ void jacobi_eigen_block(double* A, double* V, int n)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < n * n; i += blockDim.x) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < n; p++) {
            diag = diag + A[p * n + p] * A[p * n + p];
            for (int q = p + 1; q < n; q++) off = off + A[p * n + q] * A[p * n + q];
        }
        if (!(off > POSE_JACOBI_TOL * diag)) break;                      // uniform: every thread read the same entries
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                __syncthreads();
                if (tid < n) {
                    const double akp = A[tid * n + p], akq = A[tid * n + q];
                    A[tid * n + p] = c * akp - s * akq;
                    A[tid * n + q] = s * akp + c * akq;
                }
                __syncthreads();
                if (tid < n) {
                    const double apk = A[p * n + tid], aqk = A[q * n + tid];
                    A[p * n + tid] = c * apk - s * aqk;
                    A[q * n + tid] = s * apk + c * aqk;
                } else if (tid < 2 * n) {
                    const int k = tid - n;
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
                __syncthreads();
            }
    }
}

__device__ __forceinline__ int smallest_diag(const double* A, int n)
{
    int j = 0;
    for (int i = 1; i < n; i++)
        if (A[i * n + i] < A[j * n + j]) j = i;
    return j;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double det3(const double* M)
{
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// one-sided Jacobi SVD of a 3 x 3 (tests/essential_ref.svd3): U, V row-major with A = U diag(s) V^T, det U = det V = 1
__device__ void svd3(const double* E, double* U, double* V)
{
    double A[9], W[9];
    for (int i = 0; i < 9; i++) { A[i] = E[i]; W[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < POSE_SWEEPS; sweep++) {
        bool changed = false;
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double a = (A[p] * A[p] + A[3 + p] * A[3 + p]) + A[6 + p] * A[6 + p];
            const double b = (A[q] * A[q] + A[3 + q] * A[3 + q]) + A[6 + q] * A[6 + q];
            const double g = (A[p] * A[q] + A[3 + p] * A[3 + q]) + A[6 + p] * A[6 + q];
            if (!(fabs(g) > 1e-15 * sqrt(a * b))) continue;
            changed = true;
            const double theta = (b - a) / (2.0 * g);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) t = -t;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; k++) {
                const double akp = A[3 * k + p], akq = A[3 * k + q];
                A[3 * k + p] = c * akp - s * akq;
                A[3 * k + q] = s * akp + c * akq;
                const double vkp = W[3 * k + p], vkq = W[3 * k + q];
                W[3 * k + p] = c * vkp - s * vkq;
                W[3 * k + q] = s * vkp + c * vkq;
            }
        }
        if (!changed) break;
    }
    double sv[3];
    for (int j = 0; j < 3; j++) sv[j] = sqrt((A[j] * A[j] + A[3 + j] * A[3 + j]) + A[6 + j] * A[6 + j]);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (sv[ord[j]] > sv[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 3; j++) V[3 * k + j] = W[3 * k + ord[j]];
    for (int j = 0; j < 2; j++) {
        const int o = ord[j];
        for (int k = 0; k < 3; k++) U[3 * k + j] = sv[o] > 0.0 ? A[3 * k + o] / sv[o] : 0.0;
    }
    const double u0[3] = {U[0], U[3], U[6]}, u1[3] = {U[1], U[4], U[7]};
    double u2[3];
    cross3(u0, u1, u2);
    for (int k = 0; k < 3; k++) U[3 * k + 2] = u2[k];
    if (det3(V) < 0.0)
        for (int k = 0; k < 3; k++) V[3 * k + 2] = -V[3 * k + 2];
}
