// Tracker_track_features.inc — OPTIONAL edit of a caller: the two cv::calcOpticalFlowPyrLK passes and the
// forward-backward filter of Tracker::track_features on the GPU, as ONE rs_track_features call on device-resident
// pyramids (each frame is uploaded once; its pyramid is the "previous" image of the next call).
//
// How to apply: in the reference's src/Tracker.cpp, function Tracker::track_features,
//   KEEP    lines 90-105   (to_gray, prev_points, the output vectors of the LK calls; prev_gray / next_gray are no
//                           longer read and lines 92-93 may be dropped too)
//   REPLACE lines 107-134  (both LK calls, the declarations of features / matches / replenish_mask and the filter
//                           loop) by
//               #include "Tracker_track_features.inc"
//   KEEP    lines 136-153  (replenishment, refresh_descriptors, log line, return)
// and add `#include "rs_shim_common.h"` at the top of the file.  Names used from the enclosing scope: image,
// m_last_frame, prev_features, prev_points, m_static_mask and the constants of src/Tracker.cpp:17-20.
// The block leaves behind exactly what the kept tail reads:
//     features        the tracked keypoints (position = their tracked position) and descriptor rows, in index order
//     matches         (previous index, new index) per tracked keypoint, as at :128
//     replenish_mask  m_static_mask with a filled circle of KLT_REPLENISH_RADIUS at every tracked point (:131)
// Results: the kept list of tests/klt_ref.py (OpenCV's LK with exact integer window sums, DESIGN.md §2).  The window,
// levels and thresholds are the reference's (21, 4, 1.0 px; 30 iterations, eps 0.01, minEig 1e-4).
ExtractedFeatures features;
std::vector<FeatureMatch> matches;
features.keypoints.reserve(prev_points.size());
matches.reserve(prev_points.size());
cv::Mat replenish_mask = m_static_mask.clone();
{
    using namespace rs_shim;
    // two pyramids, swapped frame after frame: the pyramid uploaded as `image` by the previous call is the previous
    // frame's (Frame keeps its image's buffer alive, src/Frame.cpp:6-7), so only the new frame travels
    struct Pyramids { rs_image* img[2] = {nullptr, nullptr}; int next = 1; const unsigned char* next_data = nullptr; int w = 0, h = 0, ch = 0; };
    static Pyramids pyr;
    const cv::Mat& prev_image = m_last_frame->image();
    const int W = image.cols, H = image.rows;
    auto pitch = [](const cv::Mat& m) { return m.rows > 1 ? (int)(m.ptr<unsigned char>(1) - m.ptr<unsigned char>(0)) : m.cols * m.channels(); };
    bool ready = true;
    if (pyr.w != W || pyr.h != H) {
        for (auto*& p : pyr.img) { rs_image_destroy(p); p = nullptr; }
        for (auto*& p : pyr.img) ready = ready && ok(rs_image_create(context(), W, H, KLT_PYRAMID_LEVELS, KLT_WINDOW, &p), "rs_image_create");
        pyr.w = W; pyr.h = H; pyr.next_data = nullptr;
    }
    if (ready && pyr.next_data != nullptr && pyr.next_data == prev_image.data && pyr.ch == prev_image.channels()) {
        pyr.next ^= 1;                                              // last call's `image` is this call's previous frame
    } else if (ready) {
        ready = ok(rs_image_upload(context(), pyr.img[pyr.next ^ 1], prev_image.ptr<unsigned char>(0), pitch(prev_image),
                                   prev_image.channels()), "rs_image_upload");
    }
    ready = ready && ok(rs_image_upload(context(), pyr.img[pyr.next], image.ptr<unsigned char>(0), pitch(image), image.channels()),
                        "rs_image_upload");
    pyr.next_data = ready ? image.data : nullptr;
    pyr.ch = image.channels();
    const size_t n = prev_points.size();
    std::vector<float> pts(2 * n);
    for (size_t i = 0; i < n; i++) { pts[2 * i] = prev_points[i].x; pts[2 * i + 1] = prev_points[i].y; }
    std::vector<uint8_t> mask;                                      // the static mask, rows packed (:123)
    mask.reserve((size_t)W * H);
    for (int r = 0; r < m_static_mask.rows; r++) mask.insert(mask.end(), m_static_mask.ptr<unsigned char>(r), m_static_mask.ptr<unsigned char>(r) + W);
    Stage stage;
    DevBuf<float> d_pts(pts), d_kept_pt(2 * n);
    DevBuf<uint8_t> d_mask(mask);
    DevBuf<int32_t> d_kept(n), d_count(1);
    if (ready && ok(rs_track_features(context(), pyr.img[pyr.next ^ 1], pyr.img[pyr.next], d_pts.p, (int)n, d_mask.p,
                                      KLT_MAX_FORWARD_BACKWARD_ERROR, d_kept.p, d_kept_pt.p, d_count.p), "rs_track_features")) {
        const auto count = d_count.fetch(1);
        const auto kept = d_kept.fetch(n);
        const auto kept_pt = d_kept_pt.fetch(2 * n);
        stage.sync();
        for (int k = 0; k < count[0]; k++) {
            const size_t i = (size_t)kept[k];
            auto keypoint = prev_features.keypoints[i];
            keypoint.pt.x = kept_pt[2 * (size_t)k];
            keypoint.pt.y = kept_pt[2 * (size_t)k + 1];
            matches.emplace_back(static_cast<int>(i), static_cast<int>(features.keypoints.size()));
            features.keypoints.push_back(keypoint);
            features.descriptors.push_back(prev_features.descriptors.row((int)i));
            cv::circle(replenish_mask, cv::Point(cvRound(keypoint.pt.x), cvRound(keypoint.pt.y)), KLT_REPLENISH_RADIUS, 0, -1);
        }
    }
}
