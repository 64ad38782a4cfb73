// klt.hip — the KLT stage: device-resident image pyramids and forward-backward pyramidal Lucas-Kanade.
//
// Replaces Tracker::track_features' two cv::calcOpticalFlowPyrLK calls and the filter that follows them (reference
// src/Tracker.cpp:90-131; the same pattern is Initialization.cpp:79-90).  The specification is tests/klt_ref.py, a
// restatement of OpenCV's buildOpticalFlowPyramid / calcSharrDeriv / LKTrackerInvoker with ONE deliberate difference:
// the window sums are accumulated exactly in int64 (OpenCV: f32), so results do not depend on summation order.  Every
// other operation is the f32 / f64 operation of the restatement, in the same order; built with -ffp-contract=off and
// correctly rounded sqrt / division, positions and statuses are bit-identical to it.
//
// Layout of an rs_image: per level l, an image of w_l x h_l u8 padded by `pad` (= the window size) on every side with
// reflect-101, and the Scharr derivatives (dx, dy) as int16 pairs padded by `pad` with zeros; both with the same pitch
// w_l + 2 pad.  A window whose floored origin passes the [-win, cols) x [-win, rows) test reads only inside these padded
// buffers (the bilinear +1 column / row included): the gate that OpenCV applies is also the bounds proof.
//
// LK: one wave64 per point.  Window pixel k = lane + 64 t (t < NP) holds its template value I, Ix, Iy in registers for
// the whole level; an iteration is one bilinear gather of J per pixel, two per-lane int32 partial sums and one int64
// butterfly across the wave.  Every lane then runs the same f32 tail, so control flow stays wave-uniform.  The fused
// launch of rs_track_features runs the backward pass in the same wave right after the forward pass, then the
// forward-backward check, the rounding and the mask test; an ordered compaction (the k4_compact pattern) follows.
#include "common.h"
#include "klt.h"

#define KLT_WAVES 4                 // points (waves) per workgroup

#ifdef RS_KLT_DEBUG
#define KLT_ASSERT(c) assert(c)
#else
#define KLT_ASSERT(c) ((void)0)
#endif

// Highest level buildOpticalFlowPyramid builds: level l + 1 exists only if its size exceeds `win` both ways.
static int klt_num_levels(int w, int h, int win, int max_level)
{
    for (int l = 0; l <= max_level; l++) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (w <= win || h <= win) return l;
    }
    return max_level;
}

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// ------------------------------------------------------------------------------------------------ pyramid
// level 0 interior from a frame: grey passes through, BGR -> BT.601 8-bit fixed point (cv::cvtColor BGR2GRAY)
__global__ __launch_bounds__(256) void klt_grey(const uint8_t* __restrict__ src, int pitch, int channels, KltLevel L, int pad)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= L.w) return;
    const uint8_t* s = src + (size_t)y * pitch + (size_t)x * channels;
    int v = s[0];
    if (channels == 3) v = (1868 * s[0] + 9617 * s[1] + 4899 * s[2] + 8192) >> 14;
    L.img[(size_t)(y + pad) * L.pitch + x + pad] = (uint8_t)v;
}

// pyrDown: 5x5 [1 4 6 4 1] kernel, (s + 128) >> 8, reflect-101 inside the source level
__global__ __launch_bounds__(256) void klt_pyrdown(KltLevel S, KltLevel D, int pad)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= D.w) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int cx[5];
#pragma unroll
    for (int i = 0; i < 5; i++) cx[i] = reflect101(2 * x + i - 2, S.w) + pad;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint8_t* row = S.img + (size_t)(reflect101(2 * y + j - 2, S.h) + pad) * S.pitch;
        int t = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) t += k[i] * row[cx[i]];
        s += k[j] * t;
    }
    D.img[(size_t)(y + pad) * D.pitch + x + pad] = (uint8_t)((s + 128) >> 8);
}

// every padded pixel of a level: the image border (reflect-101 of the interior) and the Scharr derivatives (zero border)
__global__ __launch_bounds__(256) void klt_finish(KltLevel L, int pad)
{
    const int px = blockIdx.x * 256 + threadIdx.x, py = blockIdx.y;
    if (px >= L.pitch) return;
    const int x = px - pad, y = py - pad;
    const bool inside = x >= 0 && x < L.w && y >= 0 && y < L.h;
    const size_t o = (size_t)py * L.pitch + px;
    if (!inside) {
        L.img[o] = L.img[(size_t)(reflect101(y, L.h) + pad) * L.pitch + reflect101(x, L.w) + pad];
        L.der[o] = make_short2(0, 0);
        return;
    }
    const uint8_t* r0 = L.img + (size_t)(reflect101(y - 1, L.h) + pad) * L.pitch + pad;
    const uint8_t* r1 = L.img + (size_t)(y + pad) * L.pitch + pad;
    const uint8_t* r2 = L.img + (size_t)(reflect101(y + 1, L.h) + pad) * L.pitch + pad;
    const int xm = reflect101(x - 1, L.w), xp = reflect101(x + 1, L.w);
    // calcSharrDeriv: vertical smooth / difference first, then horizontal difference / smooth
    const int t0m = (r0[xm] + r2[xm]) * 3 + r1[xm] * 10, t0p = (r0[xp] + r2[xp]) * 3 + r1[xp] * 10;
    const int t1m = r2[xm] - r0[xm], t1c = r2[x] - r0[x], t1p = r2[xp] - r0[xp];
    L.der[o] = make_short2((short)(t0p - t0m), (short)((t1p + t1m) * 3 + t1c * 10));
}

// ------------------------------------------------------------------------------------------------ LK
struct KltParams {
    int win, top, max_iter;
    float half;                      // (win - 1) / 2
    double eps2, min_eig;            // criteria.epsilon squared (calcOpticalFlowPyrLK squares it), minEigThreshold
};

__device__ __forceinline__ long long wave_sum64(long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void klt_weights(float a, float b, int& w00, int& w01, int& w10, int& w11)
{
    const float s = (float)(1 << 14);
    w00 = (int)rintf((1.f - a) * (1.f - b) * s);
    w01 = (int)rintf(a * (1.f - b) * s);
    w10 = (int)rintf((1.f - a) * b * s);
    w11 = (1 << 14) - w00 - w01 - w10;
}

__device__ __forceinline__ bool klt_in_window(float fx, float fy, int cols, int rows, int win)
{
    return fx >= (float)-win && fx < (float)cols && fy >= (float)-win && fy < (float)rows;     // NaN fails
}

// One direction through all levels (LKTrackerInvoker, restated): returns the tracked position and the status.
template <int NP>
__device__ bool klt_point(const KltPyr& P, const KltPyr& Q, float2 pt, bool has_guess, float2 guess, const KltParams& prm,
                          float2& out)
{
    const int lane = threadIdx.x & 63, win = prm.win, pad = P.pad, npix = win * win;
    const float half = prm.half;
    bool status = true;
    float nx = 0.f, ny = 0.f;                 // nextPts[ptidx] of the current level
    int kx[NP], ky[NP];
#pragma unroll
    for (int t = 0; t < NP; t++) {
        const int k = lane + 64 * t;
        kx[t] = k < npix ? k % win : 0;
        ky[t] = k < npix ? k / win : 0;
    }
    for (int l = prm.top; l >= 0; l--) {
        const KltLevel& I = P.lv[l];
        const KltLevel& J = Q.lv[l];
        const float sc = 1.0f / (float)(1 << l);
        float px = pt.x * sc, py = pt.y * sc;
        if (l == prm.top) {
            nx = has_guess ? guess.x * sc : px;
            ny = has_guess ? guess.y * sc : py;
        } else {
            nx = nx * 2.f;
            ny = ny * 2.f;
        }
        px = px - half;
        py = py - half;
        const float fx = floorf(px), fy = floorf(py);
        if (!klt_in_window(fx, fy, I.w, I.h, win)) {
            if (l == 0) status = false;
            continue;
        }
        int w00, w01, w10, w11;
        klt_weights(px - fx, py - fy, w00, w01, w10, w11);
        const int pitch = I.pitch;
        int rel[NP];
        int tI[NP], tX[NP], tY[NP];
        int s11 = 0, s12 = 0, s22 = 0;
        const int base = ((int)fy + pad) * pitch + (int)fx + pad;
#pragma unroll
        for (int t = 0; t < NP; t++) {
            const bool on = lane + 64 * t < npix;
            rel[t] = ky[t] * pitch + kx[t];
            const int o = base + rel[t];
            KLT_ASSERT(o >= 0 && o + pitch + 1 < pitch * I.rows);
            const uint8_t* s = I.img + o;
            const short2* d = I.der + o;
            const short2 d00 = d[0], d01 = d[1], d10 = d[pitch], d11 = d[pitch + 1];
            const int iv = (s[0] * w00 + s[1] * w01 + s[pitch] * w10 + s[pitch + 1] * w11 + (1 << 8)) >> 9;
            const int ix = (d00.x * w00 + d01.x * w01 + d10.x * w10 + d11.x * w11 + (1 << 13)) >> 14;
            const int iy = (d00.y * w00 + d01.y * w01 + d10.y * w10 + d11.y * w11 + (1 << 13)) >> 14;
            tI[t] = on ? iv : 0;
            tX[t] = on ? ix : 0;
            tY[t] = on ? iy : 0;
            s11 += tX[t] * tX[t];
            s12 += tX[t] * tY[t];
            s22 += tY[t] * tY[t];
        }
        const float FS = 1.f / (float)(1 << 20);
        const float A11 = (float)wave_sum64(s11) * FS, A12 = (float)wave_sum64(s12) * FS, A22 = (float)wave_sum64(s22) * FS;
        const float D = A11 * A22 - A12 * A12;
        const float dd = A11 - A22;
        const float mine = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / (float)(2 * win * win);
        if ((double)mine < prm.min_eig || D < __FLT_EPSILON__) {
            if (l == 0) status = false;
            continue;
        }
        const float Di = 1.f / D;
        float qx = nx - half, qy = ny - half;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < prm.max_iter; j++) {
            const float gx = floorf(qx), gy = floorf(qy);
            if (!klt_in_window(gx, gy, J.w, J.h, win)) {
                if (l == 0) status = false;
                break;
            }
            klt_weights(qx - gx, qy - gy, w00, w01, w10, w11);
            const int jb = ((int)gy + pad) * pitch + (int)gx + pad;
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int t = 0; t < NP; t++) {
                const int o = jb + rel[t];
                KLT_ASSERT(o >= 0 && o + pitch + 1 < pitch * J.rows);
                const uint8_t* s = J.img + o;
                const int jv = (s[0] * w00 + s[1] * w01 + s[pitch] * w10 + s[pitch + 1] * w11 + (1 << 8)) >> 9;
                const int diff = jv - tI[t];
                b1 += diff * tX[t];
                b2 += diff * tY[t];
            }
            const float B1 = (float)wave_sum64(b1) * FS, B2 = (float)wave_sum64(b2) * FS;
            const float dx = (A12 * B2 - A22 * B1) * Di;
            const float dy = (A12 * B1 - A11 * B2) * Di;
            qx = qx + dx;
            qy = qy + dy;
            nx = qx + half;
            ny = qy + half;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= prm.eps2) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                nx -= dx * 0.5f;
                ny -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
    }
    out = make_float2(nx, ny);
    return status;
}

// rs_klt_track: one wave per point
template <int NP>
__global__ __launch_bounds__(64 * KLT_WAVES) void klt_track(KltPyr P, KltPyr Q, const float2* __restrict__ pts, int n,
                                                             const float2* __restrict__ guess, KltParams prm,
                                                             float2* __restrict__ next, uint8_t* __restrict__ status)
{
    const int i = blockIdx.x * KLT_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    float2 o;
    const bool ok = klt_point<NP>(P, Q, pts[i], guess != nullptr, guess ? guess[i] : make_float2(0.f, 0.f), prm, o);
    if ((threadIdx.x & 63) == 0) {
        next[i] = o;
        status[i] = ok ? 1 : 0;
    }
}

// rs_track_features: forward, backward, then Tracker.cpp:115-126 for the point; keep[i] = kept
template <int NP>
__global__ __launch_bounds__(64 * KLT_WAVES) void klt_track_fb(KltPyr P, KltPyr Q, const float2* __restrict__ pts, int n,
                                                                KltParams prm, const uint8_t* __restrict__ mask, float fb_max,
                                                                float2* __restrict__ next, uint8_t* __restrict__ keep)
{
    const int i = blockIdx.x * KLT_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const float2 p = pts[i];
    float2 f, b;
    const bool okf = klt_point<NP>(P, Q, p, false, p, prm, f);
    const bool okb = klt_point<NP>(Q, P, f, false, f, prm, b);
    if ((threadIdx.x & 63) != 0) return;
    const float ex = p.x - b.x, ey = p.y - b.y;                             // Point2f difference
    bool k = okf && okb && !(sqrt((double)ex * (double)ex + (double)ey * (double)ey) > (double)fb_max);  // cv::norm, f64
    const float rx = rintf(f.x), ry = rintf(f.y);                           // cvRound: half to even
    const int W = Q.lv[0].w, H = Q.lv[0].h;
    k = k && rx >= 0.f && ry >= 0.f && rx < (float)W && ry < (float)H;
    if (k && mask) k = mask[(size_t)(int)ry * W + (int)rx] != 0;
    next[i] = f;
    keep[i] = k ? 1 : 0;
}

// ordered compaction of the kept points (the k4_compact pattern, triangulate.hip) by ONE workgroup
__global__ __launch_bounds__(1024) void klt_compact(const uint8_t* __restrict__ keep, const float2* __restrict__ pt, int n,
                                                    int32_t* __restrict__ out_index, float2* __restrict__ out_pt,
                                                    int32_t* __restrict__ out_count)
{
    const int T = blockDim.x, chunk = (n + T - 1) / T;
    const int lo = min((int)threadIdx.x * chunk, n), hi = min(lo + chunk, n);
    int cnt = 0;
    for (int i = lo; i < hi; i++) cnt += keep[i] != 0;
    int total;
    int off = rs_block_exclusive_scan(cnt, &total);
    for (int i = lo; i < hi; i++) {
        if (!keep[i]) continue;
        out_index[off] = i;
        out_pt[off] = pt[i];
        off++;
    }
    if (threadIdx.x == 0) *out_count = total;
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int rs_image_create(rs_context* ctx, int width, int height, int max_level, int win, rs_image** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (width < 1 || height < 1 || max_level < 0 || win < 1) return rs_fail(ctx, RS_ERR_INVALID, "bad image size / levels / window");
    if (width > KLT_MAX_DIM || height > KLT_MAX_DIM) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "images up to %d x %d", KLT_MAX_DIM, KLT_MAX_DIM);
    if (max_level > KLT_MAX_LEVELS - 1) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_level 0 .. %d", KLT_MAX_LEVELS - 1);
    if (win < 5 || win > 31 || !(win & 1)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "window odd, 5 .. 31");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_image* im = new rs_image();
    im->ctx = ctx;
    im->width = width;
    im->height = height;
    im->max_level = max_level;
    im->win = win;
    KltPyr& P = im->pyr;
    P.pad = win;
    P.levels = klt_num_levels(width, height, win, max_level) + 1;
    int w = width, h = height;
    for (int l = 0; l < P.levels; l++) {
        KltLevel& L = P.lv[l];
        L.w = w;
        L.h = h;
        L.pitch = w + 2 * win;
        L.rows = h + 2 * win;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
    }
    const int rc = im->block.carve(ctx, "image pyramid", [&](rs_carve& c) {
        for (int l = 0; l < P.levels; l++) {
            const size_t px = (size_t)P.lv[l].pitch * P.lv[l].rows;
            P.lv[l].img = c.take<uint8_t>(px);
            P.lv[l].der = c.take<short2>(px);
        }
        im->d_stage = c.take<uint8_t>((size_t)width * height * 3);
    });
    if (rc != RS_OK) { delete im; return rc; }
    *out = im;
    return RS_OK;
}

extern "C" int rs_image_destroy(rs_image* im) { return rs_drain_and_delete(im); }

extern "C" int rs_image_levels(const rs_image* im, int* h_levels, int* h_sizes)
{
    if (!im || !h_levels) return RS_ERR_INVALID;
    *h_levels = im->pyr.levels;
    if (h_sizes)
        for (int l = 0; l < im->pyr.levels; l++) {
            h_sizes[2 * l] = im->pyr.lv[l].w;
            h_sizes[2 * l + 1] = im->pyr.lv[l].h;
        }
    return RS_OK;
}

static int image_build(rs_context* ctx, rs_image* im, const uint8_t* d_src, int pitch, int channels)
{
    const KltPyr& P = im->pyr;
    const int pad = P.pad;
    {
        rs_prof_scope ps(ctx, "KLT0_grey");
        hipLaunchKernelGGL(klt_grey, dim3((im->width + 255) / 256, im->height), dim3(256), 0, ctx->stream, d_src, pitch, channels,
                           P.lv[0], pad);
    }
    for (int l = 0; l < P.levels; l++) {
        if (l) {
            rs_prof_scope ps(ctx, "KLT1_pyrdown");
            hipLaunchKernelGGL(klt_pyrdown, dim3((P.lv[l].w + 255) / 256, P.lv[l].h), dim3(256), 0, ctx->stream, P.lv[l - 1], P.lv[l], pad);
        }
        rs_prof_scope ps(ctx, "KLT2_border_scharr");
        hipLaunchKernelGGL(klt_finish, dim3((P.lv[l].pitch + 255) / 256, P.lv[l].rows), dim3(256), 0, ctx->stream, P.lv[l], pad);
    }
    RS_HIP(ctx, hipGetLastError());
    im->valid = true;
    return RS_OK;
}

static int upload_check(rs_context* ctx, rs_image* im, const void* px, int pitch, int channels)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!im || !px) return rs_fail(ctx, RS_ERR_INVALID, "null image / pixels");
    if (channels != 1 && channels != 3) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "channels must be 1 (grey) or 3 (BGR)");
    if (pitch < im->width * channels) return rs_fail(ctx, RS_ERR_INVALID, "pitch %d < width * channels", pitch);
    return RS_OK;
}

extern "C" int rs_image_upload(rs_context* ctx, rs_image* im, const uint8_t* h_pixels, int pitch, int channels)
{
    int rc = upload_check(ctx, im, h_pixels, pitch, channels);
    if (rc) return rc;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const int row = im->width * channels;
    RS_HIP(ctx, hipMemcpy2DAsync(im->d_stage, row, h_pixels, pitch, row, im->height, hipMemcpyHostToDevice, ctx->stream));
    return image_build(ctx, im, im->d_stage, row, channels);
}

extern "C" int rs_image_upload_device(rs_context* ctx, rs_image* im, const uint8_t* d_pixels, int pitch, int channels)
{
    int rc = upload_check(ctx, im, d_pixels, pitch, channels);
    if (rc) return rc;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    return image_build(ctx, im, d_pixels, pitch, channels);
}

extern "C" int rs_image_download(rs_context* ctx, const rs_image* im, int level, uint8_t* h_img, int16_t* h_deriv)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!im || level < 0 || level >= im->pyr.levels) return rs_fail(ctx, RS_ERR_INVALID, "no such level");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const KltLevel& L = im->pyr.lv[level];
    const size_t px = (size_t)L.pitch * L.rows;
    if (h_img) RS_HIP(ctx, hipMemcpyAsync(h_img, L.img, px, hipMemcpyDeviceToHost, ctx->stream));
    if (h_deriv) RS_HIP(ctx, hipMemcpyAsync(h_deriv, L.der, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RS_OK;
}

// common argument checks of the two tracking entry points; fills the level count and the launch parameters
static int klt_setup(rs_context* ctx, const rs_image* from, const rs_image* to, int n, int win, int max_level, int max_iter,
                     double eps, double min_eig, KltParams* prm)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!from || !to) return rs_fail(ctx, RS_ERR_INVALID, "null image");
    if (n < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative n");
    if (n > KLT_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "up to %d points per call", KLT_MAX_POINTS);
    if (win < 5 || win > 31 || !(win & 1)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "window odd, 5 .. 31");
    if (max_level < 0 || max_level > KLT_MAX_LEVELS - 1) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_level 0 .. %d", KLT_MAX_LEVELS - 1);
    if (max_iter < 1 || max_iter > 100) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_iter 1 .. 100");
    if (!(eps >= 0.0) || !(min_eig >= 0.0)) return rs_fail(ctx, RS_ERR_INVALID, "eps / min_eig must be >= 0");
    if (from->width != to->width || from->height != to->height || from->win != to->win)
        return rs_fail(ctx, RS_ERR_INVALID, "images differ in size or padding");
    if (win > from->win) return rs_fail(ctx, RS_ERR_INVALID, "window %d exceeds the images' padding %d", win, from->win);
    if (!from->valid || !to->valid) return rs_fail(ctx, RS_ERR_INVALID, "image without an uploaded frame");
    const int top = klt_num_levels(from->width, from->height, win, max_level);
    if (top >= from->pyr.levels || top >= to->pyr.levels)
        return rs_fail(ctx, RS_ERR_INVALID, "pyramid has %d levels, the request needs %d", from->pyr.levels, top + 1);
    prm->win = win;
    prm->top = top;
    prm->max_iter = max_iter;
    prm->half = (float)((win - 1) * 0.5);
    prm->eps2 = eps * eps;
    prm->min_eig = min_eig;
    return RS_OK;
}

#define KLT_DISPATCH(win, KERNEL, ...)                                                                                   \
    do {                                                                                                                 \
        const int np__ = ((win) * (win) + 63) / 64;                                                                      \
        const dim3 g__((n + KLT_WAVES - 1) / KLT_WAVES), b__(64 * KLT_WAVES);                                            \
        if (np__ <= 1) hipLaunchKernelGGL(KERNEL<1>, g__, b__, 0, ctx->stream, __VA_ARGS__);                             \
        else if (np__ <= 2) hipLaunchKernelGGL(KERNEL<2>, g__, b__, 0, ctx->stream, __VA_ARGS__);                        \
        else if (np__ <= 4) hipLaunchKernelGGL(KERNEL<4>, g__, b__, 0, ctx->stream, __VA_ARGS__);                        \
        else if (np__ <= 7) hipLaunchKernelGGL(KERNEL<7>, g__, b__, 0, ctx->stream, __VA_ARGS__);                        \
        else if (np__ <= 10) hipLaunchKernelGGL(KERNEL<10>, g__, b__, 0, ctx->stream, __VA_ARGS__);                      \
        else hipLaunchKernelGGL(KERNEL<16>, g__, b__, 0, ctx->stream, __VA_ARGS__);                                      \
    } while (0)

extern "C" int rs_klt_track(rs_context* ctx, const rs_image* from, const rs_image* to, const float* d_pts, int n,
                            const float* d_guess, int win, int max_level, int max_iter, double eps, double min_eig,
                            float* d_next, uint8_t* d_status)
{
    KltParams prm;
    int rc = klt_setup(ctx, from, to, n, win, max_level, max_iter, eps, min_eig, &prm);
    if (rc) return rc;
    if (n == 0) return RS_OK;
    if (!d_pts || !d_next || !d_status) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    {
        rs_prof_scope ps(ctx, "KLT3_track");
        KLT_DISPATCH(win, klt_track, from->pyr, to->pyr, (const float2*)d_pts, n, (const float2*)d_guess, prm, (float2*)d_next, d_status);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_track_features(rs_context* ctx, const rs_image* prev, const rs_image* next, const float* d_prev_pts, int n,
                                 const uint8_t* d_mask, float fb_max, int32_t* d_kept_index, float* d_kept_pt,
                                 int32_t* d_count)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!prev || !next) return rs_fail(ctx, RS_ERR_INVALID, "null image");
    KltParams prm;
    // cv::calcOpticalFlowPyrLK's defaults: TermCriteria(COUNT + EPS, 30, 0.01), minEigThreshold 1e-4
    int rc = klt_setup(ctx, prev, next, n, prev->win, prev->max_level, 30, 0.01, 1e-4, &prm);
    if (rc) return rc;
    if (!d_count) return rs_fail(ctx, RS_ERR_INVALID, "null count");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        RS_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int32_t), ctx->stream));
        return RS_OK;
    }
    if (!d_prev_pts || !d_kept_index || !d_kept_pt) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    float2* d_next = nullptr;
    uint8_t* d_keep = nullptr;
    if ((rc = rs_carve_from(ctx, rs_workspace, [&](rs_carve& c) { d_next = c.take<float2>((size_t)n); d_keep = c.take<uint8_t>((size_t)n); }))) return rc;
    {
        rs_prof_scope ps(ctx, "KLT4_track_fb");
        KLT_DISPATCH(prm.win, klt_track_fb, prev->pyr, next->pyr, (const float2*)d_prev_pts, n, prm, d_mask, fb_max, d_next, d_keep);
    }
    {
        rs_prof_scope ps(ctx, "KLT5_compact");
        hipLaunchKernelGGL(klt_compact, dim3(1), dim3(1024), 0, ctx->stream, d_keep, d_next, n, d_kept_index, (float2*)d_kept_pt, d_count);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}
