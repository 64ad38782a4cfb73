// gftt.hip — the replenishment stage: Shi-Tomasi corners (cv::goodFeaturesToTrack) on level 0 of an rs_image.
//
// Replaces Tracker::track_features' replenishment (reference src/Tracker.cpp:127-146): the filled circles at the
// tracked points, OrbFeatureExtractor::extract_features' detector (cv::GFTTDetector::create(3000, 0.005, 5): block 3,
// Sobel 3, min-eigenvalue) with the border filter of cv::ORB::compute (runByImageBorder(31)), and the budget loop.
// The specification is tests/gftt_ref.py, a restatement of OpenCV's algorithm with ONE deliberate difference: the
// structure-tensor sums are exact integers (OpenCV: f32 sums of dx / 3060).  The f32 min-eigenvalue is then the
// restatement's sequence of IEEE operations (-ffp-contract=off, correctly rounded sqrtf), so the eig map and the corner
// list are bit-identical to it.
//
// One launch per stage, no workgroup waits for another inside a launch:
//   gftt_init        replenish mask := static mask (or all-255), counters := 0
//   gftt_stamp       the filled circle (drawing.cpp's midpoint loop, as a half-width table) at every excluded point;
//                    the excluded count is read on the device (rs_track_features' d_count)
//   gftt_response    Sobel from the reflect-101 padded level 0, the tensor in LDS (reflected at the image border),
//                    eig, and the masked max as an atomicMax on an order-preserving u32 image of the f32
//   gftt_candidates  threshold, 3x3 dilate, mask: a per-pixel state image and an (unordered) list of candidates
//   gftt_round x R   one round of the parallel greedy walk (gftt_ref.select_rounds); exits at once when a previous
//                    round left nothing undecided
//   gftt_finish      one workgroup: further rounds until nothing is undecided (correctness never depends on R; R = 0
//                    leaves every decision to it)
//   gftt_output      one workgroup: radix select of the top max_corners accepted keys (eig, offset), LDS bitonic sort,
//                    border filter, budget, the ordered output
// A priority key is (ordered eig bits) << 32 | raster offset: larger = earlier in OpenCV's order, ties by the larger
// offset (4.x greaterThanPtr).  Keys are unique.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "klt.h"

#define GFTT_ROUNDS 12              // round launches before the single-workgroup finisher; at most
                                    // this many, fewer with rs_context_set_int "gftt_round_launches"
#define GFTT_MAX_CORNERS 8192
#define GFTT_MAX_EXCLUDE 8192
#define GFTT_MAX_RADIUS 16
#define GFTT_MAX_MIN_DISTANCE 16.0
#define GFTT_ROUND_BLOCKS 256
#define GFTT_CAND_PPT 8              // pixels per thread of gftt_candidates (one counter atomic per 2048 pixels)

// counters (u32) of a detector
enum {
    C_ACCEPTED = 1,                 // accepted keys appended to d_acc
    C_CANDIDATES = 2,
    C_MAXBITS = 3,                  // order-preserving bits of the masked max of eig (0: empty mask)
    C_FINISH_ROUNDS = 4,            // rounds the finisher ran
    C_CAPPED = 5,                   // min(accepted, max_corners)
    C_ROUND = 8,                    // C_ROUND + r: candidates still undecided after round r
    C_COUNT = C_ROUND + GFTT_ROUNDS
};

struct rs_detector {
    rs_context* ctx = nullptr;
    int width = 0, height = 0, max_corners = 0;
    rs_dev_block block;             // everything below
    uint8_t* d_mask = nullptr;      // replenish mask [h][w]
    uint8_t* d_state = nullptr;     // 0 not a candidate, 1 undecided, 2 accepted, 3 rejected [h][w]
    float* d_eig = nullptr;         // [h][w]
    int32_t* d_cand = nullptr;      // candidate offsets (capacity: every interior pixel)
    unsigned long long* d_acc = nullptr;    // accepted keys (same capacity)
    unsigned long long* d_work = nullptr;   // radix-select working set (same capacity; ping-pong with d_acc)
    uint32_t* d_ctr = nullptr;
    bool filtered = false;          // the last call ran the distance filter
    int round_launches = 0;         // gftt_round launches of the last call (0 .. GFTT_ROUNDS)
};

struct GfttCircle { int r, hw[GFTT_MAX_RADIUS + 1]; };

// order-preserving map f32 -> u32 (every value, either sign) and back
__device__ __forceinline__ uint32_t gftt_ord(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float gftt_unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ unsigned long long gftt_key(float e, int p) { return ((unsigned long long)gftt_ord(e) << 32) | (uint32_t)p; }

// slot of this lane in a wave-aggregated append to *ctr (every lane of the wave must call it)
__device__ __forceinline__ int gftt_append(bool on, uint32_t* ctr)
{
    const unsigned long long b = __ballot(on);
    if (!b) return -1;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)b) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(b));
    base = __shfl(base, leader, 64);
    return on ? (int)(base + __popcll(b & ((1ull << lane) - 1))) : -1;
}

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int gftt_reflect(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// ------------------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(256) void gftt_init(const uint8_t* __restrict__ mask, uint8_t* __restrict__ work, int n,
                                                 uint32_t* __restrict__ ctr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < C_COUNT) ctr[threadIdx.x] = 0;
    if (i < n) work[i] = mask ? mask[i] : (uint8_t)255;
}

// cv::circle(mask, (cvRound(x), cvRound(y)), r, 0, FILLED) per excluded point: one thread per (point, row)
__global__ __launch_bounds__(256) void gftt_stamp(const float2* __restrict__ pts, const int32_t* __restrict__ count,
                                                  GfttCircle c, uint8_t* __restrict__ work, int W, int H)
{
    const int n = min(max(*count, 0), GFTT_MAX_EXCLUDE), rows = 2 * c.r + 1;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n * rows; t += gridDim.x * 256) {
        const int i = t / rows, d = t - i * rows - c.r;
        const float2 p = pts[i];
        if (!(fabsf(p.x) < 65536.f && fabsf(p.y) < 65536.f)) continue;       // NaN / far away: nothing in the image
        const int cx = (int)rintf(p.x), cy = (int)rintf(p.y), y = cy + d, k = c.hw[d < 0 ? -d : d];
        if (k < 0 || y < 0 || y >= H) continue;
        const int x0 = max(cx - k, 0), x1 = min(cx + k, W - 1);
        uint8_t* row = work + (size_t)y * W;
        for (int x = x0; x <= x1; x++) row[x] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ response
#define GT 16                       // output tile GT x GT, one thread per pixel
#define GH (GT + 2)                 // tensor tile with a one-pixel halo

// eig of exact integer tensor sums: calcMinEigenVal in f32, the order of tests/gftt_ref.min_eig
__device__ __forceinline__ float gftt_min_eig(int sxx, int sxy, int syy)
{
    const float a = (float)sxx * 0.5f, b = (float)sxy, c = (float)syy * 0.5f;
    const float u = a - c;
    const float uu = u * u, bb = b * b;
    const float s = uu + bb;
    const float e = (a + c) - sqrtf(s);
    return e * (float)(1.0 / (3060.0 * 3060.0));
}

__global__ __launch_bounds__(GT * GT) void gftt_response(KltLevel L, int pad, const uint8_t* __restrict__ mask,
                                                         float* __restrict__ eig, uint32_t* __restrict__ maxbits)
{
    __shared__ int txx[GH * GH], txy[GH * GH], tyy[GH * GH];
    const int W = L.w, H = L.h, x0 = blockIdx.x * GT, y0 = blockIdx.y * GT, tid = threadIdx.x;
    for (int k = tid; k < GH * GH; k += GT * GT) {
        // the tensor at (tx, ty) is the tensor at its reflect-101 image (the box sum reflects the tensor image)
        const int rx = gftt_reflect(x0 - 1 + k % GH, W), ry = gftt_reflect(y0 - 1 + k / GH, H);
        const uint8_t* r1 = L.img + (size_t)(ry + pad) * L.pitch + rx + pad;    // rows -1 .. +1 lie in the padding
        const uint8_t* r0 = r1 - L.pitch;
        const uint8_t* r2 = r1 + L.pitch;
        const int dx = (r0[1] + 2 * r1[1] + r2[1]) - (r0[-1] + 2 * r1[-1] + r2[-1]);
        const int dy = (r2[-1] + 2 * r2[0] + r2[1]) - (r0[-1] + 2 * r0[0] + r0[1]);
        txx[k] = dx * dx;
        txy[k] = dx * dy;
        tyy[k] = dy * dy;
    }
    __syncthreads();
    const int lx = tid % GT, ly = tid / GT, x = x0 + lx, y = y0 + ly;
    const bool in = x < W && y < H;
    uint32_t m = 0;
    if (in) {
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int k = (ly + j) * GH + lx + i;
                sxx += txx[k];
                sxy += txy[k];
                syy += tyy[k];
            }
        const float e = gftt_min_eig(sxx, sxy, syy);
        const size_t o = (size_t)y * W + x;
        eig[o] = e;
        if (!mask || mask[o]) m = gftt_ord(e);
    }
    if (maxbits) {                    // block max, then one atomic per block, skipped unless it raises the running max
        __shared__ uint32_t wmax[GT * GT / 64];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
        if ((tid & 63) == 0) wmax[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < GT * GT / 64; w++) m = max(m, wmax[w]);
            if (m > *(volatile uint32_t*)maxbits) atomicMax(maxbits, m);
        }
    }
}

// ------------------------------------------------------------------------------------------------ candidates
__device__ __forceinline__ float gftt_thr(const uint32_t* ctr, double quality)
{
    const uint32_t mb = ctr[C_MAXBITS];
    const float maxv = mb ? gftt_unord(mb) : 0.f;                  // minMaxLoc over an empty mask: 0
    return (float)((double)maxv * quality);
}

// candidate test of pixel (x, y): thresholded, a 3x3 maximum of the thresholded map, inside the mask and the interior
__device__ __forceinline__ bool gftt_is_candidate(const float* __restrict__ eig, const uint8_t* __restrict__ work, int x, int y,
                                                  int W, int H, float thr, float& v)
{
    if (x < 1 || x > W - 2 || y < 1 || y > H - 2) return false;
    const size_t o = (size_t)y * W + x;
    if (!work[o]) return false;
    v = eig[o];
    v = v > thr ? v : 0.f;                                           // THRESH_TOZERO
    if (v == 0.f) return false;
    float m = v;                                                     // dilate (3x3; every neighbour lies in the image)
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const float e = eig[o + (ptrdiff_t)j * W + i];
            m = fmaxf(m, e > thr ? e : 0.f);
        }
    return v == m;
}

// one row segment of 256 * GFTT_CAND_PPT pixels per workgroup (pixel x0 + k * 256 + thread); the candidates of the
// segment are appended with one atomic
__global__ __launch_bounds__(256) void gftt_candidates(const float* __restrict__ eig, const uint8_t* __restrict__ work, int W,
                                                       int H, double quality, bool filter, uint8_t* __restrict__ state,
                                                       int32_t* __restrict__ cand, unsigned long long* __restrict__ acc,
                                                       uint32_t* __restrict__ ctr)
{
    __shared__ uint32_t s_base;
    const int y = blockIdx.y, x0 = blockIdx.x * 256 * GFTT_CAND_PPT + threadIdx.x;
    const float thr = gftt_thr(ctr, quality);
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < GFTT_CAND_PPT; k++) {
        const int x = x0 + k * 256;
        if (x >= W) break;
        float v;
        const bool c = gftt_is_candidate(eig, work, x, y, W, H, thr, v);
        state[(size_t)y * W + x] = c ? (filter ? 1 : 2) : 0;
        bits |= (uint32_t)c << k;
    }
    int total;
    int off = rs_block_exclusive_scan(__popc(bits), &total);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(&ctr[C_CANDIDATES], (uint32_t)total) : 0;
    __syncthreads();
    if (!total) return;
    if (!filter && threadIdx.x == 0) atomicAdd(&ctr[C_ACCEPTED], (uint32_t)total);   // the same slots: acc mirrors cand
    off += s_base;
    for (int k = 0; k < GFTT_CAND_PPT; k++) {
        if (!(bits >> k & 1)) continue;
        const int p = y * W + x0 + k * 256;
        cand[off] = p;
        if (!filter) acc[off] = gftt_key(eig[p], p);
        off++;
    }
}

// ------------------------------------------------------------------------------------------------ greedy rounds
struct GfttDist { int R, d2max; };  // scan |dx|, |dy| <= R; conflict where dx^2 + dy^2 <= d2max (< minDistance^2)

// One decision of candidate p: 2 accepted, 3 rejected, 1 still undecided (a higher-priority neighbour is undecided).
// Every neighbour's state and eig are loaded unconditionally (coordinates clamped into the image, the result masked) so
// that the loads of a row are issued together instead of one dependent load after another.
__device__ __forceinline__ int gftt_decide(const float* __restrict__ eig, const uint8_t* state, int p, int W, int H, GfttDist d)
{
    const int y = p / W, x = p - y * W;
    const unsigned long long k = gftt_key(eig[p], p);
    bool rejected = false, blocked = false;
    for (int dy = -d.R; dy <= d.R; dy++) {
        const int yy = y + dy;
        const bool row_in = yy >= 0 && yy < H;
        const int yc = min(max(yy, 0), H - 1);
#pragma unroll 4
        for (int dx = -d.R; dx <= d.R; dx++) {
            const int xx = x + dx;
            const int q = yc * W + min(max(xx, 0), W - 1);
            const int s = state[q];
            const float e = eig[q];
            const bool on = row_in && xx >= 0 && xx < W && dx * dx + dy * dy <= d.d2max && (dx | dy) != 0 && (s == 1 || s == 2) &&
                            gftt_key(e, q) > k;
            rejected |= on && s == 2;
            blocked |= on && s == 1;
        }
    }
    return rejected ? 3 : blocked ? 1 : 2;
}

// one round: grid-stride over the candidates; per iteration of a workgroup one atomic for its accepted keys and one for
// its still-undecided count
__global__ __launch_bounds__(256) void gftt_round(const float* __restrict__ eig, uint8_t* state, const int32_t* __restrict__ cand,
                                                  int W, int H, GfttDist d, int r, unsigned long long* __restrict__ acc,
                                                  uint32_t* __restrict__ ctr)
{
    if (ctr[r == 0 ? C_CANDIDATES : C_ROUND + r - 1] == 0) return;         // every candidate is decided
    __shared__ uint32_t s_base;
    const int n = (int)ctr[C_CANDIDATES];
    const int stride = gridDim.x * 256;
    for (int base = blockIdx.x * 256; base < n; base += stride) {          // workgroup-uniform trip count
        const int i = base + threadIdx.x;
        int res = 0, p = 0;
        if (i < n) {
            p = cand[i];
            if (state[p] == 1) res = gftt_decide(eig, state, p, W, H, d);
        }
        if (res >= 2) state[p] = (uint8_t)res;
        int total;                                                         // accepted in the low half, undecided in the high
        const int off = rs_block_exclusive_scan((res == 2) | (res == 1) << 16, &total);
        if (threadIdx.x == 0) {
            s_base = (total & 0xffff) ? atomicAdd(&ctr[C_ACCEPTED], (uint32_t)(total & 0xffff)) : 0;
            if (total >> 16) atomicAdd(&ctr[C_ROUND + r], (uint32_t)(total >> 16));
        }
        __syncthreads();
        if (res == 2) acc[s_base + (off & 0xffff)] = gftt_key(eig[p], p);
        __syncthreads();
    }
}

// one workgroup: rounds until nothing is undecided; `launched` = the gftt_round launches before it (0: it decides all).
// It keys on the last round launched, as gftt_round keys on the one before it.
__global__ __launch_bounds__(1024) void gftt_finish(const float* __restrict__ eig, uint8_t* state, const int32_t* __restrict__ cand,
                                                    int W, int H, GfttDist d, int launched, unsigned long long* __restrict__ acc,
                                                    uint32_t* __restrict__ ctr)
{
    if (ctr[launched == 0 ? C_CANDIDATES : C_ROUND + launched - 1] == 0) return;     // nothing is undecided
    __shared__ uint32_t s_und;
    const int n = (int)ctr[C_CANDIDATES];
    int rounds = 0;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_und = 0;
        __syncthreads();
        for (int base = 0; base < n; base += 1024) {
            const int i = base + threadIdx.x;
            int res = 0, p = 0;
            if (i < n) {
                p = cand[i];
                if (state[p] == 1) res = gftt_decide(eig, state, p, W, H, d);
            }
            if (res >= 2) state[p] = (uint8_t)res;
            const int s = gftt_append(res == 2, &ctr[C_ACCEPTED]);
            if (res == 2) acc[s] = gftt_key(eig[p], p);
            if (res == 1) atomicAdd(&s_und, 1u);
        }
        __syncthreads();
        rounds++;
        if (s_und == 0) break;
    }
    if (threadIdx.x == 0) ctr[C_FINISH_ROUNDS] = rounds;
}

// ------------------------------------------------------------------------------------------------ output
#define GFTT_OUT_T 1024

// one workgroup: the top max_corners accepted keys in order, the border filter and the budget
__global__ __launch_bounds__(GFTT_OUT_T) void gftt_output(unsigned long long* acc, unsigned long long* work,
                                                          uint32_t* __restrict__ ctr, int max_corners, int W, int H, int border,
                                                          const int32_t* __restrict__ ex_count, int max_total,
                                                          float2* __restrict__ out_pt, float* __restrict__ out_resp,
                                                          int32_t* __restrict__ counts)
{
    __shared__ unsigned long long sel[GFTT_MAX_CORNERS];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_nsel, s_nwork, s_digit, s_above, s_eq;
    const int tid = threadIdx.x;
    const uint32_t A = ctr[C_ACCEPTED];
    const uint32_t K = min(A, (uint32_t)max_corners);
    if (tid == 0) { s_nsel = 0; ctr[C_CAPPED] = K; }
    __syncthreads();
    if (A == K) {
        for (uint32_t i = tid; i < A; i += GFTT_OUT_T) sel[i] = acc[i];
    } else {
        // radix select, 8 bits at a time from the top: keys above the K-th largest go to sel, keys tied on the current
        // prefix form the next working set.  The working set moves between `work` and `acc` (acc is read only by the
        // first pass, and every set fits in either: both hold every interior pixel)
        const unsigned long long* src = acc;
        uint32_t n = A, need = K;
        for (int shift = 56; shift >= 0 && need > 0; shift -= 8) {
            for (int b = tid; b < 256; b += GFTT_OUT_T) hist[b] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < n; i += GFTT_OUT_T) atomicAdd(&hist[(src[i] >> shift) & 255], 1u);
            __syncthreads();
            if (tid == 0) {
                uint32_t above = 0;
                int dgt = 255;
                for (; dgt > 0; dgt--) {
                    if (above + hist[dgt] >= need) break;
                    above += hist[dgt];
                }
                s_digit = dgt;
                s_above = above;
                s_eq = hist[dgt];
                s_nwork = 0;
            }
            __syncthreads();
            const uint32_t dgt = s_digit, above = s_above, eq = s_eq;
            const bool all_eq = above + eq == need;                 // the whole tied bin is selected: done
            unsigned long long* dst = (src == work) ? acc : work;
            for (uint32_t i = tid; i < n; i += GFTT_OUT_T) {
                const unsigned long long k = src[i];
                const uint32_t g = (uint32_t)(k >> shift) & 255;
                if (g > dgt || (g == dgt && all_eq)) sel[atomicAdd(&s_nsel, 1u)] = k;
                else if (g == dgt) dst[atomicAdd(&s_nwork, 1u)] = k;
            }
            __syncthreads();
            need = all_eq ? 0 : need - above;
            n = s_nwork;
            src = dst;
            __syncthreads();
        }
    }
    __syncthreads();
    // bitonic sort of sel[0 .. K) descending, padded with 0 (every real key is larger)
    uint32_t N = 1;
    while (N < K) N <<= 1;
    for (uint32_t i = K + tid; i < N; i += GFTT_OUT_T) sel[i] = 0;
    __syncthreads();
    for (uint32_t size = 2; size <= N; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < N / 2; t += GFTT_OUT_T) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = sel[lo], b = sel[hi];
                if ((a < b) == desc) { sel[lo] = b; sel[hi] = a; }
            }
            __syncthreads();
        }
    // runByImageBorder(border), order kept: an ordered compaction (klt_compact's pattern)
    const int chunk = (int)((K + GFTT_OUT_T - 1) / GFTT_OUT_T);
    const int lo = min(tid * chunk, (int)K), hi = min(lo + chunk, (int)K);
    int cnt = 0;
    for (int i = lo; i < hi; i++) {
        const int p = (int)(uint32_t)sel[i], y = p / W, x = p - y * W;
        cnt += x >= border && x < W - border && y >= border && y < H - border;
    }
    int total;
    int off = rs_block_exclusive_scan(cnt, &total);
    for (int i = lo; i < hi; i++) {
        const unsigned long long k = sel[i];
        const int p = (int)(uint32_t)k, y = p / W, x = p - y * W;
        if (!(x >= border && x < W - border && y >= border && y < H - border)) continue;
        out_pt[off] = make_float2((float)x, (float)y);
        out_resp[off] = gftt_unord((uint32_t)(k >> 32));
        off++;
    }
    if (tid == 0) {
        const int n_ex = ex_count ? min(max(*ex_count, 0), GFTT_MAX_EXCLUDE) : 0;
        const int budget = max_total < 0 ? total : max(0, max_total - n_ex);
        counts[0] = total;
        counts[1] = min(total, budget);
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int rs_detector_create(rs_context* ctx, int width, int height, int max_corners, int block_size, int gradient_size,
                                  rs_detector** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (width < 1 || height < 1 || max_corners < 1) return rs_fail(ctx, RS_ERR_INVALID, "bad detector size / max_corners");
    if (width > KLT_MAX_DIM || height > KLT_MAX_DIM) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "images up to %d x %d", KLT_MAX_DIM, KLT_MAX_DIM);
    if (max_corners > GFTT_MAX_CORNERS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_corners 1 .. %d", GFTT_MAX_CORNERS);
    if (block_size != 3 || gradient_size != 3) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "block and gradient sizes 3 only");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_detector* d = new rs_detector();
    d->ctx = ctx;
    d->width = width;
    d->height = height;
    d->max_corners = max_corners;
    const size_t px = (size_t)width * height;
    const size_t nc = (size_t)std::max(width - 2, 1) * std::max(height - 2, 1);
    const int rc = d->block.carve(ctx, "detector scratch", [&](rs_carve& c) {
        d->d_mask = c.take<uint8_t>(px);
        d->d_state = c.take<uint8_t>(px);
        d->d_eig = c.take<float>(px);
        d->d_cand = c.take<int32_t>(nc);
        d->d_acc = c.take<unsigned long long>(nc);
        d->d_work = c.take<unsigned long long>(nc);
        d->d_ctr = c.take<uint32_t>(C_COUNT);
    });
    if (rc != RS_OK) { delete d; return rc; }
    *out = d;
    return RS_OK;
}

extern "C" int rs_detector_destroy(rs_detector* d) { return rs_drain_and_delete(d); }

static int detector_check(rs_context* ctx, const rs_detector* det, const rs_image* img)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!det || !img) return rs_fail(ctx, RS_ERR_INVALID, "null detector / image");
    if (det->width != img->width || det->height != img->height)
        return rs_fail(ctx, RS_ERR_INVALID, "detector %d x %d, image %d x %d", det->width, det->height, img->width, img->height);
    if (!img->valid) return rs_fail(ctx, RS_ERR_INVALID, "image without an uploaded frame");
    return RS_OK;
}

static void launch_response(rs_context* ctx, const rs_image* img, const uint8_t* mask, float* eig, uint32_t* maxbits)
{
    const KltLevel& L = img->pyr.lv[0];
    rs_prof_scope ps(ctx, "GFTT2_response");
    hipLaunchKernelGGL(gftt_response, dim3((L.w + GT - 1) / GT, (L.h + GT - 1) / GT), dim3(GT * GT), 0, ctx->stream, L, img->pyr.pad,
                       mask, eig, maxbits);
}

extern "C" int rs_corner_response(rs_context* ctx, rs_detector* det, const rs_image* img, float* d_eig)
{
    int rc = detector_check(ctx, det, img);
    if (rc) return rc;
    if (!d_eig) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    launch_response(ctx, img, nullptr, d_eig, nullptr);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

// the half widths of drawing.cpp's filled Circle (LINE_8) per row offset (tests/gftt_ref.circle_half_widths)
static GfttCircle circle_table(int r)
{
    GfttCircle c;
    c.r = r;
    for (int i = 0; i <= GFTT_MAX_RADIUS; i++) c.hw[i] = -1;
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    while (dx >= dy) {
        c.hw[dy] = std::max(c.hw[dy], dx);
        c.hw[dx] = std::max(c.hw[dx], dy);
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
    return c;
}

extern "C" int rs_detect_features(rs_context* ctx, rs_detector* det, const rs_image* img, const uint8_t* d_mask,
                                  const float* d_exclude_pt, const int32_t* d_exclude_count, int exclude_radius, int max_corners,
                                  double quality, double min_distance, int border, int max_total, float* d_pt, float* d_response,
                                  int32_t* d_counts)
{
    int rc = detector_check(ctx, det, img);
    if (rc) return rc;
    if (!d_pt || !d_response || !d_counts) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if ((d_exclude_pt == nullptr) != (d_exclude_count == nullptr)) return rs_fail(ctx, RS_ERR_INVALID, "exclusion points without a count, or a count without points");
    if (max_corners < 1 || max_corners > det->max_corners)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_corners 1 .. %d (the detector's)", det->max_corners);
    if (!(quality > 0.0 && quality <= 1.0)) return rs_fail(ctx, RS_ERR_INVALID, "quality must lie in (0, 1]");
    if (!(min_distance >= 0.0 && min_distance <= GFTT_MAX_MIN_DISTANCE)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "min_distance 0 .. 16");
    if (exclude_radius < 0 || exclude_radius > GFTT_MAX_RADIUS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "exclude_radius 0 .. %d", GFTT_MAX_RADIUS);
    if (border < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative border");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = det->width, H = det->height, n = W * H;
    const bool filter = min_distance >= 1.0;
    const int launches = ctx->gftt_round_launches;
    det->filtered = filter;
    det->round_launches = launches;
    GfttDist dist{0, 0};
    if (filter) {
        dist.d2max = (int)std::ceil(min_distance * min_distance) - 1;            // dx^2 + dy^2 < minDistance^2, integers
        while ((dist.R + 1) * (dist.R + 1) <= dist.d2max) dist.R++;
    }
    {
        rs_prof_scope ps(ctx, "GFTT0_mask");
        hipLaunchKernelGGL(gftt_init, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_mask, det->d_mask, n, det->d_ctr);
        if (d_exclude_pt)
            hipLaunchKernelGGL(gftt_stamp, dim3(64), dim3(256), 0, ctx->stream, (const float2*)d_exclude_pt, d_exclude_count,
                               circle_table(exclude_radius), det->d_mask, W, H);
    }
    launch_response(ctx, img, det->d_mask, det->d_eig, det->d_ctr + C_MAXBITS);
    {
        rs_prof_scope ps(ctx, "GFTT3_candidates");
        hipLaunchKernelGGL(gftt_candidates, dim3((W + 256 * GFTT_CAND_PPT - 1) / (256 * GFTT_CAND_PPT), H), dim3(256), 0, ctx->stream, det->d_eig, det->d_mask, W, H,
                           quality, filter, det->d_state, det->d_cand, det->d_acc, det->d_ctr);
    }
    if (filter) {
        rs_prof_scope ps(ctx, "GFTT4_rounds");
        for (int r = 0; r < launches; r++)
            hipLaunchKernelGGL(gftt_round, dim3(GFTT_ROUND_BLOCKS), dim3(256), 0, ctx->stream, det->d_eig, det->d_state, det->d_cand,
                               W, H, dist, r, det->d_acc, det->d_ctr);
        hipLaunchKernelGGL(gftt_finish, dim3(1), dim3(1024), 0, ctx->stream, det->d_eig, det->d_state, det->d_cand, W, H, dist,
                           launches, det->d_acc, det->d_ctr);
    }
    {
        rs_prof_scope ps(ctx, "GFTT5_output");
        hipLaunchKernelGGL(gftt_output, dim3(1), dim3(GFTT_OUT_T), 0, ctx->stream, det->d_acc, det->d_work, det->d_ctr, max_corners,
                           W, H, border, d_exclude_count, max_total, (float2*)d_pt, d_response, d_counts);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_detector_stats(rs_context* ctx, const rs_detector* det, int32_t* h_stats)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!det || !h_stats) return rs_fail(ctx, RS_ERR_INVALID, "null detector / output");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t c[C_COUNT];
    RS_HIP(ctx, hipMemcpyAsync(c, det->d_ctr, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int rounds = 0;
    if (det->filtered && c[C_CANDIDATES] > 0) {
        rounds = det->round_launches + (int)c[C_FINISH_ROUNDS];
        for (int r = 0; r < det->round_launches; r++)
            if (c[C_ROUND + r] == 0) { rounds = r + 1; break; }
    }
    h_stats[0] = (int32_t)c[C_CANDIDATES];
    h_stats[1] = (int32_t)c[C_ACCEPTED];
    h_stats[2] = rounds;
    h_stats[3] = (int32_t)c[C_FINISH_ROUNDS];
    h_stats[4] = (int32_t)c[C_CAPPED];
    return RS_OK;
}
