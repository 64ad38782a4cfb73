// Drop-in replacement of the reference's src/PoseEstimation.cpp (keeps src/PoseEstimation.h).
// Compiled only in the reference's tree; syntax-checked here, see rs_shim_common.h.  Tracker::initial_pose_estimate
// (src/Tracker.cpp:162) and Initialization (src/Initialization.cpp:153) call it unchanged.  The specification of both
// functions is tests/essential_ref.py (include/rsgpu.h, rs_estimate_pose*): agreement with cv::findEssentialMat's USAC
// is not claimed.  The same marshalling is compiled, run and checked in racing-slam_amd/host/slam_host.cpp (slam::pose).
#include "PoseEstimation.h"

#include <random>

#include "rs_shim_common.h"

namespace slam::pose {

namespace {

constexpr int MAX_POINTS = 8192;            // rs_pose_estimator's envelope

rs_pose_estimator* estimator()
{
    static rs_pose_estimator* est = [] {
        rs_pose_estimator* e = nullptr;
        if (!rs_shim::ok(rs_pose_estimator_create(rs_shim::context(), MAX_POINTS, 1000, &e), "rs_pose_estimator_create"))
            return (rs_pose_estimator*)nullptr;
        return e;
    }();
    return est;
}

// the matched pixels, :64-68
void matched_pixels(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                    const std::vector<FeatureMatch>& matches, std::vector<float>& from, std::vector<float>& to)
{
    const size_t n = matches.size();
    from.assign(2 * (n ? n : 1), 0.f);
    to.assign(2 * (n ? n : 1), 0.f);
    for (size_t k = 0; k < n; k++) {
        const auto& a = prev_features.keypoints[matches[k].train_index].pt;
        const auto& b = features.keypoints[matches[k].query_index].pt;
        from[2 * k] = a.x;
        from[2 * k + 1] = a.y;
        to[2 * k] = b.x;
        to[2 * k + 1] = b.y;
    }
}

// pose, inlier list and count read back in ONE synchronisation
PoseEstimate finish(const std::vector<FeatureMatch>& matches, const rs_shim::DevBuf<float>& d_pose,
                    const rs_shim::DevBuf<int32_t>& d_index, const rs_shim::DevBuf<int32_t>& d_count, rs_shim::Stage& stage)
{
    auto pose = d_pose.fetch(16);
    auto index = d_index.fetch(matches.size());
    auto count = d_count.fetch(1);
    stage.sync();
    PoseEstimate estimate;
    estimate.pose = rs_shim::pose_from_row_major(pose.data());
    for (int32_t k = 0; k < count[0]; k++) estimate.inlier_matches.push_back(matches[index[k]]);
    return estimate;
}

PoseEstimate failed(const char* what)
{
    std::printf("%s: no pose estimator, or more than %d matches\n", what, MAX_POINTS);
    PoseEstimate estimate;
    estimate.pose = Eigen::Matrix4f::Identity();
    return estimate;
}

}  // namespace

PoseEstimate estimate_pose(const ExtractedFeatures& prev_features,
                           const ExtractedFeatures& features,
                           const std::vector<FeatureMatch>& matches,
                           const Camera& camera)
{
    using namespace rs_shim;
    const size_t n = matches.size();
    rs_pose_estimator* est = estimator();
    if (!est || n > (size_t)MAX_POINTS) return failed("estimate_pose");
    std::vector<float> from, to;
    matched_pixels(prev_features, features, matches, from, to);
    float K[4];
    intrinsics(camera.get_intrinsic_matrix(), K);
    // findEssentialMat(USAC_ACCURATE, 0.99, 1.0 px) (:70-77): 1000 hypotheses (USAC's maxIters), seed 0
    Stage stage;
    DevBuf<float> d_from(from), d_to(to), d_pose(16);
    DevBuf<int32_t> d_n(std::vector<int32_t>{(int32_t)n}), d_index(n ? n : 1), d_count(1), d_status(1);
    DevBuf<uint8_t> d_inlier(n ? n : 1);
    if (!ok(rs_estimate_pose(context(), est, d_from.p, nullptr, d_to.p, d_n.p, (int)n, K, 1.0, 0.99, 1000, 0, d_pose.p,
                             d_inlier.p, d_index.p, d_count.p, d_status.p),
            "rs_estimate_pose"))
        return failed("estimate_pose");
    // status 1 / 2 (fewer than 5 matches, no model): identity and no inliers, where cv::findEssentialMat would throw
    return finish(matches, d_pose, d_index, d_count, stage);
}

PoseEstimate estimate_pose_with_known_rotation(const ExtractedFeatures& prev_features,
                                               const ExtractedFeatures& features,
                                               const std::vector<FeatureMatch>& matches,
                                               const Camera& camera,
                                               const Eigen::Matrix3f& rotation)
{
    using namespace rs_shim;
    const size_t n = matches.size();
    rs_pose_estimator* est = estimator();
    if (!est || n > (size_t)MAX_POINTS) return failed("estimate_pose_with_known_rotation");
    std::vector<float> from, to;
    matched_pixels(prev_features, features, matches, from, to);
    float K[4], R[9];
    intrinsics(camera.get_intrinsic_matrix(), K);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = rotation(i, j);
    // the reference's 200 draws (:137-143): std::mt19937(0), uniform_int_distribution<size_t>, i then j
    std::vector<int32_t> pairs(400, 0);
    if (n > 0) {
        std::mt19937 generator(0);
        std::uniform_int_distribution<size_t> pick(0, n - 1);
        for (size_t it = 0; it < 200; it++) {
            const size_t i = pick(generator);
            const size_t j = pick(generator);
            pairs[2 * it] = (int32_t)i;
            pairs[2 * it + 1] = (int32_t)j;
        }
    }
    Stage stage;
    DevBuf<float> d_from(from), d_to(to), d_pose(16);
    DevBuf<int32_t> d_pairs(pairs), d_index(n ? n : 1), d_count(1), d_status(1);
    DevBuf<uint8_t> d_inlier(n ? n : 1);
    if (!ok(rs_estimate_pose_known_rotation(context(), est, d_from.p, nullptr, d_to.p, (int)n, K, R, d_pairs.p, 200, 2.0f,
                                            d_pose.p, d_inlier.p, d_index.p, d_count.p, d_status.p),
            "rs_estimate_pose_known_rotation"))
        return failed("estimate_pose_with_known_rotation");
    // fewer than 8 matches or a best support below 8: [rotation | 0] and no inliers, as the reference returns
    return finish(matches, d_pose, d_index, d_count, stage);
}

}  // namespace slam::pose
