// orb.hip — the description stage: ORB (rBRIEF, patch 31) descriptors of supplied keypoints on level 0 of an rs_image.
//
// Replaces OrbFeatureExtractor::refresh_descriptors (reference src/features/OrbFeatureExtractor.cpp:29-61, called at
// src/Tracker.cpp:150): cv::ORB::compute on every keypoint of the frame (octave 0, angle -1: the pattern as it is),
// the rows of keypoints outside ORB's border filter left as the frame carried them.  The same call with no carried
// rows is extract_features' compute (OrbFeatureExtractor.cpp:24).  The specification is tests/orb_ref.py; the blur
// is its f32 sequence of operations (-ffp-contract=off) and the tests are integer compares, so the plane, the rows,
// the fresh flags and the count are bit-identical to it.
//
// Two launches on the context stream, no host synchronisation, no allocation per call:
//   orb_blur      GaussianBlur(7x7, sigma 2, reflect-101) of level 0 into the describer's W x H u8 plane: a 64 x 16
//                 output tile per workgroup, the (64+6) x (16+6) u8 apron and the f32 row pass in LDS; each output
//                 pixel is one thread's fixed 7-tap row sums and symmetric column sum, so no reduction order exists
//   orb_describe  one wave64 per output row: the counts of both lists are read on the device (rs_track_features'
//                 d_count, rs_detect_features' d_counts + 1); list a first, then list b; the border filter; for a
//                 kept point, 4 rounds in which lane l evaluates test 64 r + l and __ballot packs 64 bits (bit k of
//                 byte i is test 8 i + k: the ballot's order is OpenCV's); else the carried row (or zeros)
// Bounds: a kept centre lies in [border, W-border-1] x [border, H-border-1] with border >= ORB_MIN_BORDER > 13, and
// the pattern reaches 13 px, so every gather lies inside the plane.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "klt.h"

#define ORB_PATTERN_STORAGE __constant__
#include "orb_pattern.h"

#define ORB_MAX_POINTS 8192
#define ORB_MIN_BORDER 16           // 13 (the pattern's reach) + 3 (the blur's radius): the border rule never matters
#define ORB_DESC_BYTES 32
#define ORB_TX 64                   // blur output tile
#define ORB_TY 16
#define ORB_R 3                     // blur radius (7 taps)
#define ORB_WAVES 4                 // describe: rows (waves) per workgroup
#define ORB_MAX_BLOCKS 1024         // describe: grid-stride beyond this many workgroups

struct rs_describer {
    rs_context* ctx = nullptr;
    int width = 0, height = 0, max_points = 0;
    rs_dev_block block;
    uint8_t* d_blur = nullptr;      // the blurred level 0 [h][w]
};

struct OrbKernel { float k[2 * ORB_R + 1]; };

struct OrbLists {
    const float2* pa;               // list a (tracked points) and its count; NULL = empty
    const int32_t* ca;
    const int32_t* carry_index;     // row of carry_desc that point a_i carries (NULL: row i)
    const uint8_t* carry_desc;      // NULL: list a carries zeros
    int n_carry;                    // rows of carry_desc; an index outside [0, n_carry) carries zeros
    const float2* pb;               // list b (appended corners) and its count; NULL = empty
    const int32_t* cb;
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int orb_reflect(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// ------------------------------------------------------------------------------------------------ blur
__global__ __launch_bounds__(256) void orb_blur(KltLevel L, int pad, OrbKernel k, uint8_t* __restrict__ out)
{
    constexpr int AX = ORB_TX + 2 * ORB_R, AY = ORB_TY + 2 * ORB_R;
    __shared__ uint8_t tin[AY][AX];
    __shared__ float trow[AY][ORB_TX];
    const int W = L.w, H = L.h, x0 = blockIdx.x * ORB_TX, y0 = blockIdx.y * ORB_TY, tid = threadIdx.x;
    for (int i = tid; i < AY * AX; i += 256) {
        const int ly = i / AX, lx = i - ly * AX;
        // positions past W + 2 / H + 2 feed no output pixel: clamped there to keep the reflection loop short
        const int gx = orb_reflect(min(x0 - ORB_R + lx, W + ORB_R - 1), W);
        const int gy = orb_reflect(min(y0 - ORB_R + ly, H + ORB_R - 1), H);
        tin[ly][lx] = L.img[(size_t)(gy + pad) * L.pitch + gx + pad];
    }
    __syncthreads();
    for (int i = tid; i < AY * ORB_TX; i += 256) {        // row pass: f32, taps in order
        const int ly = i / ORB_TX, lx = i - ly * ORB_TX;
        float s = k.k[0] * (float)tin[ly][lx];
#pragma unroll
        for (int t = 1; t <= 2 * ORB_R; t++) s = s + k.k[t] * (float)tin[ly][lx + t];
        trow[ly][lx] = s;
    }
    __syncthreads();
    for (int i = tid; i < ORB_TY * ORB_TX; i += 256) {    // column pass: the symmetric form
        const int ly = i / ORB_TX, lx = i - ly * ORB_TX, x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        float c = k.k[ORB_R] * trow[ly + ORB_R][lx];
#pragma unroll
        for (int j = 1; j <= ORB_R; j++) c = c + k.k[ORB_R + j] * (trow[ly + ORB_R - j][lx] + trow[ly + ORB_R + j][lx]);
        out[(size_t)y * W + x] = (uint8_t)fminf(fmaxf(rintf(c), 0.f), 255.f);
    }
}

// ------------------------------------------------------------------------------------------------ describe
__global__ __launch_bounds__(64 * ORB_WAVES) void orb_describe(const uint8_t* __restrict__ B, int W, int H, int border, OrbLists l,
                                                             int cap, uint8_t* __restrict__ desc, uint8_t* __restrict__ fresh,
                                                             int32_t* __restrict__ d_n)
{
    const int lane = threadIdx.x & 63;
    int o0[4], o1[4];                                     // this lane's tests 64 r + lane as offsets in the plane
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const signed char* p = orb_bit_pattern_31 + 4 * (64 * r + lane);
        o0[r] = p[1] * W + p[0];
        o1[r] = p[3] * W + p[2];
    }
    const int na = l.pa ? min(max(*l.ca, 0), cap) : 0;
    const int nb = l.pb ? min(max(*l.cb, 0), cap - na) : 0;
    const int n = na + nb;
    if (d_n && blockIdx.x == 0 && threadIdx.x == 0) *d_n = n;
    const bool room = W > 2 * border && H > 2 * border;
    for (int i = blockIdx.x * ORB_WAVES + (threadIdx.x >> 6); i < n; i += gridDim.x * ORB_WAVES) {
        const float2 p = i < na ? l.pa[i] : l.pb[i - na];
        bool keep = room && fabsf(p.x) < 65536.f && fabsf(p.y) < 65536.f;      // NaN / far away: not kept
        int cx = 0, cy = 0;
        if (keep) {
            cx = (int)rintf(p.x);                         // cvRound: half to even
            cy = (int)rintf(p.y);
            keep = cx >= border && cx <= W - border - 1 && cy >= border && cy <= H - border - 1;
        }
        uint8_t* row = desc + (size_t)i * ORB_DESC_BYTES;
        if (keep) {                                       // wave-uniform
            const uint8_t* c = B + (size_t)cy * W + cx;
            const unsigned long long m0 = __ballot(c[o0[0]] < c[o1[0]]), m1 = __ballot(c[o0[1]] < c[o1[1]]),
                                     m2 = __ballot(c[o0[2]] < c[o1[2]]), m3 = __ballot(c[o0[3]] < c[o1[3]]);
            if (lane < ORB_DESC_BYTES) {
                const int q = lane >> 3;
                const unsigned long long m = q == 0 ? m0 : q == 1 ? m1 : q == 2 ? m2 : m3;
                row[lane] = (uint8_t)(m >> (8 * (lane & 7)));
            }
        } else if (lane < ORB_DESC_BYTES) {
            uint8_t v = 0;
            if (i < na && l.carry_desc) {
                const int src = l.carry_index ? l.carry_index[i] : i;
                if (src >= 0 && src < l.n_carry) v = l.carry_desc[(size_t)src * ORB_DESC_BYTES + lane];
            }
            row[lane] = v;
        }
        if (fresh && lane == 0) fresh[i] = keep ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
// getGaussianKernel(7, 2, CV_32F) (tests/orb_ref.gaussian_kernel): f64 weights times 1 / their sum, rounded to f32
static OrbKernel orb_kernel()
{
    OrbKernel k;
    const int n = 2 * ORB_R + 1;
    const double sigma = 2.0, scale2x = -0.125 / (sigma * sigma);
    double t[ORB_R], sum = 0.0;
    for (int i = 0, x = 1 - n; i < ORB_R; i++, x += 2) {
        t[i] = std::exp((double)(x * x) * scale2x);
        sum += t[i];
    }
    sum = sum * 2.0 + 1.0;
    const double mul = 1.0 / sum;
    for (int i = 0; i < ORB_R; i++) k.k[i] = k.k[n - 1 - i] = (float)(t[i] * mul);
    k.k[ORB_R] = (float)mul;
    return k;
}

extern "C" int rs_describer_create(rs_context* ctx, int width, int height, int max_points, rs_describer** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (width < 1 || height < 1 || max_points < 1) return rs_fail(ctx, RS_ERR_INVALID, "bad describer size / max_points");
    if (width > KLT_MAX_DIM || height > KLT_MAX_DIM) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "images up to %d x %d", KLT_MAX_DIM, KLT_MAX_DIM);
    if (max_points > ORB_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_points 1 .. %d", ORB_MAX_POINTS);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_describer* d = new rs_describer();
    d->ctx = ctx;
    d->width = width;
    d->height = height;
    d->max_points = max_points;
    const int rc = d->block.carve(ctx, "describer plane", [&](rs_carve& c) { d->d_blur = c.take<uint8_t>((size_t)width * height); });
    if (rc != RS_OK) { delete d; return rc; }
    *out = d;
    return RS_OK;
}

extern "C" int rs_describer_destroy(rs_describer* d) { return rs_drain_and_delete(d); }

static int describer_check(rs_context* ctx, const rs_describer* d, const rs_image* img)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!d || !img) return rs_fail(ctx, RS_ERR_INVALID, "null describer / image");
    if (d->width != img->width || d->height != img->height)
        return rs_fail(ctx, RS_ERR_INVALID, "describer %d x %d, image %d x %d", d->width, d->height, img->width, img->height);
    if (!img->valid) return rs_fail(ctx, RS_ERR_INVALID, "image without an uploaded frame");
    return RS_OK;
}

static void launch_blur(rs_context* ctx, const rs_image* img, uint8_t* out)
{
    const KltLevel& L = img->pyr.lv[0];
    rs_prof_scope ps(ctx, "ORB0_blur");
    hipLaunchKernelGGL(orb_blur, dim3((L.w + ORB_TX - 1) / ORB_TX, (L.h + ORB_TY - 1) / ORB_TY), dim3(256), 0, ctx->stream, L,
                       img->pyr.pad, orb_kernel(), out);
}

extern "C" int rs_orb_blur(rs_context* ctx, rs_describer* d, const rs_image* img, uint8_t* d_blur)
{
    int rc = describer_check(ctx, d, img);
    if (rc) return rc;
    if (!d_blur) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    launch_blur(ctx, img, d_blur);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_describe_features(rs_context* ctx, rs_describer* d, const rs_image* img, const float* d_pt_a,
                                    const int32_t* d_count_a, const int32_t* d_carry_index, const uint8_t* d_carry_desc,
                                    int n_carry, const float* d_pt_b, const int32_t* d_count_b, int border, uint8_t* d_desc,
                                    uint8_t* d_fresh, int32_t* d_n)
{
    int rc = describer_check(ctx, d, img);
    if (rc) return rc;
    if (!d_desc) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if ((d_pt_a == nullptr) != (d_count_a == nullptr)) return rs_fail(ctx, RS_ERR_INVALID, "list a: points without a count, or a count without points");
    if ((d_pt_b == nullptr) != (d_count_b == nullptr)) return rs_fail(ctx, RS_ERR_INVALID, "list b: points without a count, or a count without points");
    if (n_carry < 0 || (n_carry > 0 && !d_carry_desc)) return rs_fail(ctx, RS_ERR_INVALID, "n_carry must be >= 0, and > 0 only with carried rows");
    if (border < ORB_MIN_BORDER) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "border >= %d", ORB_MIN_BORDER);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if (d_pt_a || d_pt_b) {
        launch_blur(ctx, img, d->d_blur);
        const OrbLists l{(const float2*)d_pt_a, d_count_a, d_carry_index, d_carry_desc, d_carry_desc ? n_carry : 0,
                         (const float2*)d_pt_b, d_count_b};
        const int blocks = std::min((d->max_points + ORB_WAVES - 1) / ORB_WAVES, ORB_MAX_BLOCKS);
        rs_prof_scope ps(ctx, "ORB1_describe");
        hipLaunchKernelGGL(orb_describe, dim3(blocks), dim3(64 * ORB_WAVES), 0, ctx->stream, d->d_blur, d->width, d->height,
                           border, l, d->max_points, d_desc, d_fresh, d_n);
    } else if (d_n) {
        RS_HIP(ctx, hipMemsetAsync(d_n, 0, sizeof(int32_t), ctx->stream));
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}
