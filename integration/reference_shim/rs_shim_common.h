// rs_shim_common.h — helpers shared by the drop-in translation units of this directory.
//
// These files include the reference's own headers plus Eigen / OpenCV, none of which exists in this repository's build
// image: they are the binding a maintainer of GregVS/Racing-SLAM adds to that tree.  Here they are
// syntax-checked against the reference's real headers with stand-in Eigen / OpenCV declarations
// (integration/check_shim_syntax.py, tests/test_shim_syntax.py).  The pointer graph -> SoA flattening is not theirs: it
// is the templates of rs_marshal.h, the same source that racing-slam_amd/host/slam_host.cpp instantiates on plain types
// and that is compiled, run, tested and timed there; `Access` below is how those templates read the reference's objects.
// The only dependencies besides the reference tree are include/rsgpu.h and rs_marshal.h.
#pragma once
#include <Eigen/Dense>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Frame.h"
#include "MapPoint.h"
#include "rs_marshal.h"
#include "rsgpu.h"

namespace rs_shim {

using rs_marshal::PtrIndex;

inline rs_context* context()
{
    static rs_context* ctx = [] {
        rs_context* c = nullptr;
        if (rs_context_create(0, &c) != RS_OK) { std::printf("rsgpu: no MI355X visible, aborting (no CPU fallback)\n"); std::abort(); }
        return c;
    }();
    return ctx;
}

// no error codes in the reference: log to stdout like it does, caller returns {} / false
inline bool ok(int rc, const char* what)
{
    if (rc == RS_OK) return true;
    std::printf("%s failed: %s\n", what, rs_last_error(context()));
    return false;
}

// One interface call = one staging group (include/rsgpu.h, "staging pool"): grow-only device + pinned arenas,
// asynchronous copies on the context stream, ONE synchronisation per call.  No hipMalloc / hipFree per array.
struct Stage {
    Stage() { ok(rs_stage_begin(context()), "rs_stage_begin"); }
    void sync() { ok(rs_stage_sync(context()), "rs_stage_sync"); }
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    explicit DevBuf(size_t count) : n(count) { ok(rs_stage_alloc(context(), sizeof(T) * (count ? count : 1), (void**)&p), "rs_stage_alloc"); }
    explicit DevBuf(const std::vector<T>& h) : n(h.size()) { ok(rs_stage_upload(context(), h.data(), sizeof(T) * h.size(), (void**)&p), "rs_stage_upload"); }
    DevBuf(const T* h, size_t count) : n(count) { ok(rs_stage_upload(context(), h, sizeof(T) * count, (void**)&p), "rs_stage_upload"); }
    // registers an asynchronous read-back of the first `count` entries; filled when Stage::sync() returns
    std::vector<T> fetch(size_t count) const
    {
        std::vector<T> h(count);
        if (count) ok(rs_stage_download(context(), p, sizeof(T) * count, h.data()), "rs_stage_download");
        return h;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Eigen is column-major, the C-ABI row-major: transpose 16 floats.
inline void pose_to_row_major(const Eigen::Matrix4f& T, float out[16])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = T(i, j);
}
inline Eigen::Matrix4f pose_from_row_major(const float in[16])
{
    Eigen::Matrix4f T;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) T(i, j) = in[4 * i + j];
    return T;
}
inline void append_row_major(const Eigen::Matrix4f& T, std::vector<float>& table)
{
    table.resize(table.size() + 16);
    pose_to_row_major(T, table.data() + table.size() - 16);
}
inline void intrinsics(const Eigen::Matrix3f& M, float K[4])
{
    K[0] = M(0, 0); K[1] = M(1, 1); K[2] = M(0, 2); K[3] = M(1, 2);
}

// 32-byte ORB rows (or no rows at all): the only descriptor layout the Hamming kernels take
inline bool orb_layout(const cv::Mat& d) { return d.empty() || (d.type() == CV_8U && d.cols == RS_DESC_BYTES && d.isContinuous()); }
// float rows the L2 matchers take (rs_match_descriptors_f32, rs_reproj_match_l2): CV_32F, 4 .. 1024 columns in fours, continuous
inline bool f32_layout(const cv::Mat& d)
{
    return d.empty() || (d.type() == CV_32F && d.cols >= 4 && d.cols <= 1024 && d.cols % 4 == 0 && d.isContinuous());
}

// How the flatten templates of rs_marshal.h read the reference's objects (Eigen / OpenCV).
struct Access {
    using Point = slam::MapPoint;
    static void position(const slam::MapPoint& p, float out[3]) { for (int k = 0; k < 3; k++) out[k] = p.position()[k]; }
    static void pose_row_major(const slam::Frame& f, float out[16]) { pose_to_row_major(f.pose(), out); }
    static void center(const slam::Frame& f, float out[3]) { const Eigen::Vector3f c = f.camera_center(); out[0] = c.x(); out[1] = c.y(); out[2] = c.z(); }
    static void keypoint(const slam::Frame& f, size_t i, float out[2]) { out[0] = f.keypoint(i).pt.x; out[1] = f.keypoint(i).pt.y; }
    static bool descriptor_rows(const slam::Frame& f, const uint8_t*& rows, size_t& n_rows)
    {
        const cv::Mat& d = f.features().descriptors;            // N x 32 CV_8U, row-contiguous
        if (!orb_layout(d)) return false;
        rows = d.ptr<uint8_t>(0); n_rows = (size_t)d.rows;
        return true;
    }
    static bool descriptor_rows_f32(const slam::Frame& f, const float*& rows, size_t& n_rows, size_t dim)
    {
        const cv::Mat& d = f.features().descriptors;            // N x dim CV_32F, row-contiguous
        if (!f32_layout(d) || (!d.empty() && (size_t)d.cols != dim)) return false;
        rows = d.ptr<float>(0); n_rows = (size_t)d.rows;
        return true;
    }
    static size_t n_matches(const slam::Frame& f) { return f.num_map_matches(); }
    template <typename Fn>
    static void for_each_match(const slam::Frame& f, Fn fn)
    {
        for (const auto& m : f.map_matches()) fn(m.point, m.keypoint_index);     // ascending keypoint index, src/Frame.cpp:154-174
    }
    template <typename Fn>
    static void for_each_observation(const slam::MapPoint& p, Fn fn)
    {
        for (const auto& [kf, idx] : p.observations()) fn(kf, idx);
    }
    static size_t n_observations(const slam::MapPoint& p) { return p.observations().size(); }
    static const void* observations_address(const slam::MapPoint& p) { return p.observations().empty() ? nullptr : &*p.observations().begin(); }
    static bool is_matched(const slam::Frame& f, const slam::MapPoint& p) { return f.is_matched(p); }
    static bool is_observed_by(const slam::MapPoint& p, slam::KeyFrame* kf) { return p.is_observed_by(kf); }
};

}  // namespace rs_shim
