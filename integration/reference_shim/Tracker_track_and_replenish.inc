// Tracker_track_and_replenish.inc — OPTIONAL edit of a caller: the whole per-frame front end of Tracker::track_features
// on the GPU, as ONE pair of calls on device-resident pyramids: rs_track_features (the two cv::calcOpticalFlowPyrLK
// passes and the forward-backward filter) then rs_detect_features (the circles at the tracked points, the ORB
// extractor's cv::GFTTDetector(3000, 0.005, 5) with cv::ORB::compute's 31-px border filter, and the budget).  The
// tracked points and their count stay on the device between the two calls; one read-back follows them.
// An alternative to Tracker_track_features.inc (which replaces the KLT half alone); apply one or the other.
//
// How to apply: in the reference's src/Tracker.cpp, function Tracker::track_features,
//   KEEP    lines 90-105   (to_gray, prev_points, the output vectors of the LK calls, window)
//   REPLACE lines 107-146  (both LK calls, the filter loop, extract_features and the budget loop) by
//               #include "Tracker_track_and_replenish.inc"
//   KEEP    lines 148-153  (refresh_descriptors, the log line, return)
// and add `#include "rs_shim_common.h"` and `#include "features/OrbFeatureExtractor.h"` at the top of the file.  Names
// used from the enclosing scope: image, m_last_frame, prev_features, prev_points, next_points, back_points,
// forward_ok, backward_ok, window, prev_gray, next_gray, m_static_mask, m_feature_extractor and the constants of
// src/Tracker.cpp:17-22.  The block leaves behind exactly what the kept tail reads:
//     features        the tracked keypoints (at their tracked positions, with their descriptor rows, in index order),
//                     then the replenished ones, strongest first, up to MAX_TRACKED_FEATURES in all
//     matches         (previous index, new index) per tracked keypoint, as at :128
//     new_features    the detector's keypoints (its size is the "replenished" count of the log line)
// The GPU path is taken only with the ORB extractor (the detector it restates); any other extractor runs the original
// lines 107-146, which are repeated verbatim in the else branch.
//
// Descriptors of the replenished keypoints: the original describes them twice, once in extract_features (:138) and
// again in refresh_descriptors (:150), on the same image, with the same keypoints, one pyramid level, each keypoint
// described on its own; the second pass overwrites every row the first one wrote.  Here they are appended with zero
// rows and refresh_descriptors computes them: the result is the same and the first CPU ORB pass disappears.
// New keypoints are cv::KeyPoint(corner, 31, -1, response): GFTTDetector's KeyPoint(corner, 3, -1, response) with
// the size extract_features sets (:19-21 of OrbFeatureExtractor.cpp).
// Results: the kept list of tests/klt_ref.py and the corners of tests/gftt_ref.py (OpenCV's algorithms with exact
// integer window / tensor sums, DESIGN.md §2).
const bool rs_orb_extractor = dynamic_cast<const features::OrbFeatureExtractor*>(&m_feature_extractor) != nullptr;
ExtractedFeatures features;
std::vector<FeatureMatch> matches;
ExtractedFeatures new_features;
features.keypoints.reserve(prev_points.size());
matches.reserve(prev_points.size());
if (!rs_orb_extractor) {
    // src/Tracker.cpp:107-146 as they are
    cv::calcOpticalFlowPyrLK(
        prev_gray, next_gray, prev_points, next_points, forward_ok, cv::noArray(), window, KLT_PYRAMID_LEVELS);
    cv::calcOpticalFlowPyrLK(
        next_gray, prev_gray, next_points, back_points, backward_ok, cv::noArray(), window, KLT_PYRAMID_LEVELS);
    cv::Mat replenish_mask = m_static_mask.clone();
    for (size_t i = 0; i < prev_points.size(); i++) {
        if (!forward_ok[i] || !backward_ok[i] ||
            cv::norm(prev_points[i] - back_points[i]) > KLT_MAX_FORWARD_BACKWARD_ERROR) {
            continue;
        }
        auto point = cv::Point(cvRound(next_points[i].x), cvRound(next_points[i].y));
        if (point.x < 0 || point.y < 0 || point.x >= next_gray.cols || point.y >= next_gray.rows ||
            m_static_mask.at<uchar>(point) == 0) {
            continue;
        }
        auto keypoint = prev_features.keypoints[i];
        keypoint.pt = next_points[i];
        matches.emplace_back(static_cast<int>(i), static_cast<int>(features.keypoints.size()));
        features.keypoints.push_back(keypoint);
        features.descriptors.push_back(prev_features.descriptors.row(i));
        cv::circle(replenish_mask, point, KLT_REPLENISH_RADIUS, 0, -1);
    }
    new_features = m_feature_extractor.extract_features(image, replenish_mask);
    size_t budget =
        features.keypoints.size() < MAX_TRACKED_FEATURES ? MAX_TRACKED_FEATURES - features.keypoints.size() : 0;
    for (size_t i = 0; i < new_features.keypoints.size() && budget > 0; i++) {
        features.keypoints.push_back(new_features.keypoints[i]);
        features.descriptors.push_back(new_features.descriptors.row(i));
        budget--;
    }
} else {
    using namespace rs_shim;
    constexpr int GFTT_MAX_CORNERS = 3000, ORB_EDGE_THRESHOLD = 31;      // OrbFeatureExtractor.h:25-26
    constexpr double GFTT_QUALITY = 0.005, GFTT_MIN_DISTANCE = 5.0;
    // two pyramids swapped frame after frame (as in Tracker_track_features.inc) and the detector's scratch
    struct Device {
        rs_image* img[2] = {nullptr, nullptr};
        int next = 1;
        const unsigned char* next_data = nullptr;
        int w = 0, h = 0, ch = 0;
        rs_detector* det = nullptr;
    };
    static Device dev;
    const cv::Mat& prev_image = m_last_frame->image();
    const int W = image.cols, H = image.rows;
    auto pitch = [](const cv::Mat& m) { return m.rows > 1 ? (int)(m.ptr<unsigned char>(1) - m.ptr<unsigned char>(0)) : m.cols * m.channels(); };
    bool ready = true;
    if (dev.w != W || dev.h != H) {
        for (auto*& p : dev.img) { rs_image_destroy(p); p = nullptr; }
        rs_detector_destroy(dev.det);
        dev.det = nullptr;
        for (auto*& p : dev.img) ready = ready && ok(rs_image_create(context(), W, H, KLT_PYRAMID_LEVELS, KLT_WINDOW, &p), "rs_image_create");
        ready = ready && ok(rs_detector_create(context(), W, H, GFTT_MAX_CORNERS, 3, 3, &dev.det), "rs_detector_create");
        dev.w = W; dev.h = H; dev.next_data = nullptr;
    }
    if (ready && dev.next_data != nullptr && dev.next_data == prev_image.data && dev.ch == prev_image.channels()) {
        dev.next ^= 1;                                              // last call's `image` is this call's previous frame
    } else if (ready) {
        ready = ok(rs_image_upload(context(), dev.img[dev.next ^ 1], prev_image.ptr<unsigned char>(0), pitch(prev_image),
                                   prev_image.channels()), "rs_image_upload");
    }
    ready = ready && ok(rs_image_upload(context(), dev.img[dev.next], image.ptr<unsigned char>(0), pitch(image), image.channels()),
                        "rs_image_upload");
    dev.next_data = ready ? image.data : nullptr;
    dev.ch = image.channels();
    const size_t n = prev_points.size();
    std::vector<float> pts(2 * n);
    for (size_t i = 0; i < n; i++) { pts[2 * i] = prev_points[i].x; pts[2 * i + 1] = prev_points[i].y; }
    std::vector<uint8_t> mask;                                      // the static mask, rows packed (:123, :131)
    mask.reserve((size_t)W * H);
    for (int r = 0; r < m_static_mask.rows; r++) mask.insert(mask.end(), m_static_mask.ptr<unsigned char>(r), m_static_mask.ptr<unsigned char>(r) + W);
    Stage stage;
    DevBuf<float> d_pts(pts), d_kept_pt(2 * n), d_new_pt(2 * GFTT_MAX_CORNERS), d_new_response(GFTT_MAX_CORNERS);
    DevBuf<uint8_t> d_mask(mask);
    DevBuf<int32_t> d_kept(n), d_count(1), d_new_counts(2);
    // :107-131, then :131-146 with the kept points and their count read on the device
    if (ready && ok(rs_track_features(context(), dev.img[dev.next ^ 1], dev.img[dev.next], d_pts.p, (int)n, d_mask.p,
                                      KLT_MAX_FORWARD_BACKWARD_ERROR, d_kept.p, d_kept_pt.p, d_count.p), "rs_track_features") &&
        ok(rs_detect_features(context(), dev.det, dev.img[dev.next], d_mask.p, d_kept_pt.p, d_count.p, KLT_REPLENISH_RADIUS,
                              GFTT_MAX_CORNERS, GFTT_QUALITY, GFTT_MIN_DISTANCE, ORB_EDGE_THRESHOLD, (int)MAX_TRACKED_FEATURES,
                              d_new_pt.p, d_new_response.p, d_new_counts.p), "rs_detect_features")) {
        const auto count = d_count.fetch(1);
        const auto kept = d_kept.fetch(n);
        const auto kept_pt = d_kept_pt.fetch(2 * n);
        const auto new_counts = d_new_counts.fetch(2);
        const auto new_pt = d_new_pt.fetch(2 * GFTT_MAX_CORNERS);
        const auto new_response = d_new_response.fetch(GFTT_MAX_CORNERS);
        stage.sync();
        for (int k = 0; k < count[0]; k++) {
            const size_t i = (size_t)kept[k];
            auto keypoint = prev_features.keypoints[i];
            keypoint.pt.x = kept_pt[2 * (size_t)k];
            keypoint.pt.y = kept_pt[2 * (size_t)k + 1];
            matches.emplace_back(static_cast<int>(i), static_cast<int>(features.keypoints.size()));
            features.keypoints.push_back(keypoint);
            features.descriptors.push_back(prev_features.descriptors.row((int)i));
        }
        for (int k = 0; k < new_counts[0]; k++) {
            cv::KeyPoint keypoint;
            keypoint.pt.x = new_pt[2 * (size_t)k];
            keypoint.pt.y = new_pt[2 * (size_t)k + 1];
            keypoint.size = 31.f;
            keypoint.angle = -1.f;
            keypoint.response = new_response[(size_t)k];
            keypoint.octave = 0;
            keypoint.class_id = -1;
            new_features.keypoints.push_back(keypoint);
        }
        const cv::Mat zero_row = cv::Mat::zeros(1, 32, CV_8U);      // described by refresh_descriptors (:150)
        for (int k = 0; k < new_counts[1]; k++) {
            features.keypoints.push_back(new_features.keypoints[(size_t)k]);
            features.descriptors.push_back(zero_row);
        }
    }
}
