// Drop-in replacement of the reference's src/MapMatcher.cpp (keeps src/MapMatcher.h byte for byte).
// Compiled only in the reference's tree (OpenCV + Eigen); syntax-checked here, see rs_shim_common.h.
//
// Two descriptor kinds.  NORM_HAMMING on 32-byte CV_8U rows is what the reference runs (OrbFeatureExtractor: max distance
// 64, src/features/OrbFeatureExtractor.h:14-22) and goes to the 256-bit Hamming kernels.  NORM_L2 on continuous CV_32F rows
// (4 .. 1024 columns in fours: what a DeepFeatureExtractor would hand over, src/Tracker.cpp:42) goes to the float matchers
// rs_match_descriptors_f32 / rs_reproj_match_l2 with the float threshold as it is.  Any other norm type or descriptor layout
// is refused loudly — log + empty result — instead of feeding rows to a kernel made for another kind.
#include "MapMatcher.h"

#include "Camera.h"
#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "rs_shim_common.h"

namespace slam {
namespace {

// which matcher takes these rows under this norm: 1 = Hamming on ORB rows, 2 = L2 on float rows, 0 = refused (and said so)
int row_kind(const cv::Mat& d, cv::NormTypes norm, const char* who)
{
    if (norm == cv::NORM_HAMMING && rs_shim::orb_layout(d)) return 1;
    if (norm == cv::NORM_L2 && rs_shim::f32_layout(d)) return 2;
    std::printf("%s: the GPU path matches 32-byte ORB descriptors under NORM_HAMMING or continuous CV_32F rows of 4 .. 1024 columns "
                "(in fours) under NORM_L2 only (norm %d, type %d, cols %d)\n",
                who, (int)norm, d.empty() ? -1 : d.type(), d.empty() ? 0 : d.cols);
    return 0;
}

// Frame keeps its KD-tree private; the shim rebuilds the flattened tree from the keypoints with the library's host
// builder (same median-split rule, ties by keypoint index).  One build per call; a maintainer would cache it on Frame.
struct FrameArrays {
    std::vector<float> kp;
    std::vector<uint8_t> matched;
    std::vector<int32_t> node_kp, left, right;
    int32_t root = -1;
    explicit FrameArrays(const Frame& f)
    {
        const size_t n = f.features().keypoints.size();
        kp.resize(2 * n); matched.resize(n); node_kp.resize(n); left.resize(n); right.resize(n);
        for (size_t i = 0; i < n; i++) { kp[2 * i] = f.keypoint(i).pt.x; kp[2 * i + 1] = f.keypoint(i).pt.y; matched[i] = f.is_matched(i); }
        rs_kdtree_build(kp.data(), (int)n, node_kp.data(), left.data(), right.data(), &root);
    }
};

std::vector<MapPointMatch> reproj(const Camera& camera, float max_distance, cv::NormTypes norm, const Frame& frame,
                                  const std::vector<MapPoint*>& points, KeyFrame* required_observer, bool replace)
{
    using namespace rs_shim;
    const size_t N = frame.features().keypoints.size(), P = points.size();
    const cv::Mat& fd = frame.features().descriptors;
    if (N == 0) return {};
    const int kind = row_kind(fd, norm, "MapMatcher::match");
    if (!kind) return {};
    const bool l2 = kind == 2;
    const size_t dim = l2 ? (size_t)fd.cols : 0;
    FrameArrays fa(frame);
    // map side (rs_marshal.h); a key frame whose descriptors are not rows of the frame's kind and width refuses the whole call
    const rs_marshal::MatchArrays m = l2 ? rs_marshal::flatten_match<true>(frame, points, required_observer, Access{}, dim)
                                         : rs_marshal::flatten_match(frame, points, required_observer, Access{});
    if (m.refused) {
        if (l2) std::printf("MapMatcher::match (key frame): its descriptors are not continuous CV_32F rows of %d columns like the frame's\n", (int)dim);
        else std::printf("MapMatcher::match (key frame): the GPU path matches 32-byte ORB descriptors only (CV_8U, %d columns, continuous)\n", RS_DESC_BYTES);
        return {};
    }
    Stage stage;
    DevBuf<float> d_kp(fa.kp), d_pos(m.pos), d_centers(m.centers);
    DevBuf<uint8_t> d_matched(fa.matched), d_elig(m.eligible);
    DevBuf<int32_t> d_nk(fa.node_kp), d_l(fa.left), d_r(fa.right), d_optr(m.obs_ptr), d_okf(m.obs_kf), d_odesc(m.obs_desc);
    rs_frame_view fv{};
    pose_to_row_major(frame.pose(), fv.pose);
    float K[4];
    intrinsics(camera.get_intrinsic_matrix(), K);
    fv.fx = K[0]; fv.fy = K[1]; fv.cx = K[2]; fv.cy = K[3];
    fv.width = camera.get_width(); fv.height = camera.get_height(); fv.n_keypoints = (int)N;
    fv.d_keypoints = d_kp.p; fv.d_kp_matched = d_matched.p;
    fv.d_kd_node_kp = d_nk.p; fv.d_kd_left = d_l.p; fv.d_kd_right = d_r.p; fv.kd_root = fa.root;
    rs_map_view mv{(int)P, d_pos.p, d_elig.p, d_optr.p, d_okf.p, d_odesc.p, d_centers.p, nullptr};
    DevBuf<int32_t> pk(P), pp(N), mkp(N), mpt(N), cnt(1);
    if (l2) {
        // float distances against the float threshold, strict '<' as the reference writes it (:78, :88)
        DevBuf<float> d_rows(fd.ptr<float>(0), N * dim), d_pool(m.pool_f32), pd(P), pdist(N);
        if (!ok(rs_reproj_match_l2(context(), &fv, &mv, d_rows.p, d_pool.p, (int)dim, replace, max_distance, pk.p, pd.p, pp.p, pdist.p,
                                   mkp.p, mpt.p, cnt.p), "rs_reproj_match_l2"))
            return {};
    } else {
        DevBuf<uint8_t> d_desc(fd.ptr<uint8_t>(0), N * RS_DESC_BYTES), d_pool(m.pool);
        DevBuf<int32_t> pd(P), pdist(N);
        fv.d_descriptors = d_desc.p; mv.d_desc_pool = d_pool.p;
        // the reference keeps a candidate iff distance < max_descriptor_distance (:78, :88) with an integer distance and
        // a FLOAT threshold: d < 50.5 <=> d < 51, d < 64.0 <=> d < 64, i.e. ceil
        const int strict_max = (int)std::ceil(max_distance);
        if (!ok(rs_reproj_match(context(), &fv, &mv, replace, strict_max, pk.p, pd.p, pp.p, pdist.p, mkp.p, mpt.p, cnt.p), "rs_reproj_match"))
            return {};
    }
    const auto hn = cnt.fetch(1);
    const auto hk = mkp.fetch(N), hp = mpt.fetch(N);
    stage.sync();
    std::vector<MapPointMatch> out;
    for (int i = 0; i < hn[0]; i++) out.push_back(MapPointMatch{*points[hp[i]], (size_t)hk[i]});
    return out;
}

std::vector<MapPoint*> all_points(Map& map)
{
    std::vector<MapPoint*> v;
    for (auto& p : map) v.push_back(&p);      // map order, src/Map.h:66
    return v;
}

}  // namespace

MapMatcher::MapMatcher(const Camera& camera, float max_descriptor_distance, cv::NormTypes norm_type)
    : m_camera(camera), m_max_descriptor_distance(max_descriptor_distance), m_norm_type(norm_type) {}

std::vector<MapPointMatch> MapMatcher::match_map(const Frame& frame, Map& map) const { return match(frame, map, nullptr); }

std::vector<MapPointMatch> MapMatcher::match_key_frame(const Frame& frame, Map& map, KeyFrame* key_frame) const { return match(frame, map, key_frame); }

std::vector<MapPointMatch> MapMatcher::match_for_fuse(const Frame& frame, const std::vector<MapPoint*>& points) const
{
    return reproj(m_camera, m_max_descriptor_distance, m_norm_type, frame, points, nullptr, true);
}

std::vector<MapPointMatch> MapMatcher::match(const Frame& frame, Map& map, KeyFrame* required_observer) const
{
    return reproj(m_camera, m_max_descriptor_distance, m_norm_type, frame, all_points(map), required_observer, false);
}

std::vector<MapPointMatch> MapMatcher::match_descriptors(const Frame& frame, const KeyFrame& key_frame) const
{
    using namespace rs_shim;
    const cv::Mat& q = frame.features().descriptors;
    const cv::Mat& kd = key_frame.features().descriptors;
    const int kind = row_kind(q, m_norm_type, "MapMatcher::match_descriptors");
    if (!kind || row_kind(kd, m_norm_type, "MapMatcher::match_descriptors") != kind) return {};
    const bool l2 = kind == 2;
    if (l2 && !q.empty() && !kd.empty() && q.cols != kd.cols) {
        std::printf("MapMatcher::match_descriptors: float rows of %d and %d columns\n", q.cols, kd.cols);
        return {};
    }
    std::vector<MapPoint*> points;
    std::vector<uint8_t> train;
    std::vector<float> train_f32;
    for (const auto& m : key_frame.map_matches()) {                     // ascending keypoint order, :143-144
        points.push_back(&m.point);
        // Frame::descriptor(i) is descriptors.row(i) (src/Frame.cpp:128-131): a row HEADER whose datastart / dataend
        // still span the whole parent matrix — the row's bytes are ptr<uint8_t>(i) .. + 32
        if (l2) {
            const float* row = kd.ptr<float>((int)m.keypoint_index);
            train_f32.insert(train_f32.end(), row, row + kd.cols);
        } else {
            const uint8_t* row = kd.ptr<uint8_t>((int)m.keypoint_index);
            train.insert(train.end(), row, row + RS_DESC_BYTES);
        }
    }
    if (points.empty() || q.empty()) return {};                         // :139-141
    const int nq = q.rows, nt = (int)points.size();
    Stage stage;
    DevBuf<int32_t> mq(nq), mt(nq), cnt(1);
    if (l2) {
        // :152 and :156 on float distances, the float threshold as it is
        DevBuf<float> dq(q.ptr<float>(0), (size_t)nq * (size_t)q.cols), dt(train_f32);
        if (!ok(rs_match_descriptors_f32(context(), dq.p, nq, dt.p, nt, q.cols, 1, m_max_descriptor_distance, mq.p, mt.p, cnt.p, nullptr,
                                         nullptr, nullptr, nullptr), "rs_match_descriptors_f32"))
            return {};
    } else {
        DevBuf<uint8_t> dq(q.ptr<uint8_t>(0), (size_t)nq * RS_DESC_BYTES), dt(train);
        // :152 rejects d0 > max (float) with an integer d0: keep d0 <= floor(max)
        const int keep_max = (int)std::floor(m_max_descriptor_distance);
        if (!ok(rs_match_descriptors(context(), dq.p, nq, dt.p, nt, 1, keep_max, mq.p, mt.p, cnt.p, nullptr, nullptr, nullptr, nullptr),
                "rs_match_descriptors"))
            return {};
    }
    const auto hn = cnt.fetch(1);
    const auto hq = mq.fetch(nq), ht = mt.fetch(nq);
    stage.sync();
    std::vector<MapPointMatch> out;
    for (int i = 0; i < hn[0]; i++) out.push_back({*points[(size_t)ht[i]], (size_t)hq[i]});
    return out;
}

}  // namespace slam
