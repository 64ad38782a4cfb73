#!/usr/bin/env python3
"""Front-end (-fsyntax-only) check of the drop-in translation units in integration/reference_shim/.

    python integration/check_shim_syntax.py <Racing-SLAM checkout>/src

The shims are OUR marshalling code, but they include the upstream project's own headers and Eigen / OpenCV.  This
type-checks them against the upstream project's REAL headers (the directory given) with the minimal Eigen / OpenCV
stand-ins of tests/shim_stubs/ (declarations only; see its README: this is not a build of the upstream project — none
of its .cpp files is compiled, nothing is linked or run, no parity claim rests on it).  It catches a missing
definition, helpers that do not exist, and signatures that drifted from the headers.  The upstream headers are not
part of this repository, so this is a maintainer's tool and not part of the test suite (tests/test_shim_syntax.py
keeps the checks that need only this repository).  Exit status 0: every unit type-checks.
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "integration", "reference_shim")
UNITS = ("MapMatcher.cpp", "Triangulation.cpp", "Optimization.cpp", "LocalWindow.cpp", "PoseEstimation.cpp")


def flags(upstream_src):
    return ["-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-reorder",
            "-I" + os.path.join(ROOT, "tests", "shim_stubs"), "-I" + upstream_src, "-I" + os.path.join(ROOT, "include"),
            "-I" + SHIM]


def check(path, upstream_src):
    """(ok, compiler diagnostics) of one translation unit."""
    cxx = shutil.which("g++") or shutil.which("c++")
    r = subprocess.run([cxx] + flags(upstream_src) + [path], capture_output=True, text=True)
    return r.returncode == 0, r.stderr


# The two optional caller edits (.inc), spliced into skeletons of the functions they belong to (kept head / tail of
# the upstream function reduced to the declarations the block relies on).
INC_HARNESS = r'''
#include <algorithm>
#include <iostream>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include "Mapper.h"
#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "TrackStore.h"
#include "Trajectory.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
// the constants of src/Mapper.cpp:21-39 that the .inc files use (values as in the reference)
constexpr size_t MIN_NEW_POINTS_PER_KEY_FRAME = 100;
constexpr float ANY_PARALLAX_COSINE = 1.0F;
constexpr float TRACK_MAX_REPROJECTION_ERROR = 4.0F;
constexpr float TRACK_MIN_PARALLAX_COSINE = 0.999848F;
constexpr float ROTATION_PARALLAX_FACTOR = 0.20F;
constexpr float MAX_POINT_REPROJECTION_ERROR = 3.0F;
}
void Mapper::triangulate_tracks(KeyFrame& key_frame, TrackStore& tracks, const Trajectory& trajectory, FrameDiagnostics& diagnostics)
{
    struct Candidate { const Track* track; Eigen::Vector3f position; size_t keypoint_index; float parallax_cosine; float required_cosine; };
    std::vector<Candidate> candidates;
    std::vector<TrackId> inconsistent;
#include "Mapper_triangulate_tracks.inc"
    for (size_t index : accepted) { const auto& candidate = candidates[index]; (void)candidate.track->sightings.size(); }
    (void)topped_up;
}
void Mapper::cull_points(FrameDiagnostics& diagnostics, KeyFrame& key_frame)
{
    std::unordered_set<MapPoint*> local;
#include "Mapper_cull_points.inc"
    for (const auto& point : points_to_remove) m_map.remove_point(point);
}
}  // namespace slam
'''


# Tracker_track_features.inc spliced into a skeleton of Tracker::track_features (kept head :90-105 reduced to what the
# block reads).  The block uses a few OpenCV names the Mapper harness does not need (cv::Point, cv::circle, cvRound,
# Mat::push_back); the check compiles against a copy of tests/shim_stubs/ in a temporary directory whose core.hpp adds
# their declarations (the stubs themselves stay untouched).  The Tracker harnesses share that copy.
TRACKER_HARNESS = r"""
#include "Tracker.h"
#include "Frame.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
constexpr int KLT_WINDOW = 21;
constexpr int KLT_PYRAMID_LEVELS = 4;
constexpr float KLT_MAX_FORWARD_BACKWARD_ERROR = 1.0F;
constexpr int KLT_REPLENISH_RADIUS = 5;
}
std::pair<ExtractedFeatures, std::vector<FeatureMatch>> Tracker::track_features(const cv::Mat& image)
{
    const auto& prev_features = m_last_frame->features();
    std::vector<cv::Point2f> prev_points;
    for (const auto& keypoint : prev_features.keypoints) prev_points.push_back(keypoint.pt);
#include "Tracker_track_features.inc"
    (void)replenish_mask;
    return {std::move(features), std::move(matches)};
}
}  // namespace slam
"""
TRACKER_STUB_EXTRA = """
    void push_back(const Mat& row);
"""
TRACKER_STUB_FREE = """
namespace cv {
struct Point { int x, y; Point(int x, int y); };
void circle(Mat& img, Point center, int radius, double color, int thickness);
}  // namespace cv
int cvRound(float value);
"""

# Tracker_track_and_replenish.inc spliced into a skeleton of Tracker::track_features (kept head :90-105, kept tail
# :148-153 reduced to what it reads).  Besides the Tracker block's names it needs the ones of the original lines it
# repeats (cv::calcOpticalFlowPyrLK, cv::norm, ...), Mat::zeros, and what features/OrbFeatureExtractor.h declares.
REPLENISH_HARNESS = r"""
#include "Tracker.h"
#include "Frame.h"
#include "features/OrbFeatureExtractor.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
constexpr int KLT_WINDOW = 21;
constexpr int KLT_PYRAMID_LEVELS = 4;
constexpr float KLT_MAX_FORWARD_BACKWARD_ERROR = 1.0F;
constexpr int KLT_REPLENISH_RADIUS = 5;
constexpr size_t MAX_TRACKED_FEATURES = 2000;
}
std::pair<ExtractedFeatures, std::vector<FeatureMatch>> Tracker::track_features(const cv::Mat& image)
{
    cv::Mat prev_gray = m_last_frame->image();
    cv::Mat next_gray = image;
    const auto& prev_features = m_last_frame->features();
    std::vector<cv::Point2f> prev_points;
    for (const auto& keypoint : prev_features.keypoints) prev_points.push_back(keypoint.pt);
    std::vector<cv::Point2f> next_points;
    std::vector<cv::Point2f> back_points;
    std::vector<uchar> forward_ok;
    std::vector<uchar> backward_ok;
    auto window = cv::Size(KLT_WINDOW, KLT_WINDOW);
#include "Tracker_track_and_replenish.inc"
    features.descriptors = m_feature_extractor.refresh_descriptors(image, features);
    (void)new_features.keypoints.size();
    return {std::move(features), std::move(matches)};
}
}  // namespace slam
"""
REPLENISH_STUB_EXTRA = """
    static Mat zeros(int rows, int cols, int type);
    template <typename T, typename P> const T& at(const P& point) const;
"""
REPLENISH_STUB_FREE = """
#include <memory>
typedef unsigned char uchar;
namespace cv {
struct Size { int width, height; Size(int width, int height); };
struct NoArray {};
NoArray noArray();
template <typename... Args> void calcOpticalFlowPyrLK(const Args&... args);
Point2f operator-(const Point2f& a, const Point2f& b);
double norm(const Point2f& v);
template <typename T> using Ptr = std::shared_ptr<T>;
class Feature2D { public: virtual ~Feature2D(); };
class GFTTDetector : public Feature2D { public: static Ptr<GFTTDetector> create(int maxCorners, double qualityLevel, double minDistance); };
class ORB : public Feature2D { public: static Ptr<ORB> create(); };
}  // namespace cv
"""


# Tracker_track_tail.inc spliced into a skeleton of Tracker::track (kept head :72-82 reduced to the frame it builds, kept
# tail :87), with the names the caller that owns the resident map supplies declared as locals.
TRACK_TAIL_HARNESS = r"""
#include <iostream>
#include "Tracker.h"
#include "Frame.h"
#include "MapPoint.h"
#include "MotionModel.h"
#include "Slam.h"
#include "features/FeatureExtractor.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
constexpr size_t MIN_TRACKED_MAP_POINTS = 15;
}
std::shared_ptr<Frame> Tracker::track(const cv::Mat& image, size_t frame_index, const Trajectory& trajectory, KeyFrame& last_key_frame,
                                      size_t num_key_frames)
{
    m_last_key_frame = &last_key_frame;
    ExtractedFeatures features;
    auto frame = std::make_shared<Frame>(frame_index, image, features);
    rs_map* resident_map = nullptr;
    std::vector<MapPoint*> resident_points;
    rs_frame* resident_prev = nullptr;
    rs_frame* resident_next = nullptr;
    const int32_t* resident_kept_index = nullptr;
    const int32_t* resident_inlier_index = nullptr;
    const int32_t* resident_inlier_count = nullptr;
    int resident_max_n = 0, resident_last_key_frame = 0;
#include "Tracker_track_tail.inc"
    return frame;
}
}  // namespace slam
"""
# Slam.h (for SlamConfig) pulls in VideoLoader.h, which holds a cv::VideoCapture by value
TRACK_TAIL_STUB_FREE = """
namespace cv {
class VideoCapture {};
}  // namespace cv
"""


# Mapper_insert.inc's three blocks spliced into skeletons of Mapper::insert, Mapper::bundle_adjust and Mapper::cull_points
# (kept lines reduced to the declarations the blocks rely on), with the names the caller that owns the resident map
# supplies declared as locals.
MAPPER_INSERT_HARNESS = r"""
#include <iostream>
#include <unordered_map>
#include "Mapper.h"
#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "Optimization.h"
#include "Slam.h"
#include "TrackStore.h"
#include "Trajectory.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
constexpr size_t BA_WINDOW = 20;
constexpr float MAX_POINT_REPROJECTION_ERROR = 3.0F;
rs_map* resident_map = nullptr;
std::vector<MapPoint*> resident_points;
std::unordered_map<const Frame*, int32_t> resident_key_frames;
rs_frame* resident_frame = nullptr;
}
std::shared_ptr<KeyFrame> Mapper::insert(Frame&& frame, TrackStore& tracks, const Trajectory& trajectory, FrameDiagnostics& diagnostics)
{
    auto key_frame = std::make_shared<KeyFrame>(std::move(frame));
    for (const auto& match : key_frame->map_matches()) m_map.associate(*key_frame, match.point, match.keypoint_index);
#define RS_MAPPER_INSERT_PART 1
#include "Mapper_insert.inc"
    return key_frame;
}
void Mapper::bundle_adjust(KeyFrame& key_frame, bool fix_oldest)
{
    std::vector<std::pair<Frame*, Eigen::Matrix4f>> anchors;
#define RS_MAPPER_INSERT_PART 2
#include "Mapper_insert.inc"
}
void Mapper::cull_points(FrameDiagnostics& diagnostics, KeyFrame& key_frame)
{
#define RS_MAPPER_INSERT_PART 3
#include "Mapper_insert.inc"
}
}  // namespace slam
"""


def tracker_stubs(dst):
    """tests/shim_stubs/ copied to dst with the declarations the Tracker blocks need added to opencv2/core.hpp"""
    src = os.path.join(ROOT, "tests", "shim_stubs")
    shutil.copytree(src, dst)
    core = os.path.join(dst, "opencv2", "core.hpp")
    text = open(core).read()
    head, tail = text.split("    Mat clone() const;\n", 1)
    text = head + "    Mat clone() const;\n" + TRACKER_STUB_EXTRA + REPLENISH_STUB_EXTRA + tail + TRACKER_STUB_FREE + REPLENISH_STUB_FREE + TRACK_TAIL_STUB_FREE
    open(core, "w").write(text)
    return dst


def main(argv):
    if len(argv) != 2 or not os.path.isfile(os.path.join(argv[1], "MapMatcher.h")):
        sys.exit("usage: check_shim_syntax.py <Racing-SLAM checkout>/src  (the directory holding MapMatcher.h)")
    upstream_src = os.path.abspath(argv[1])
    failed = []
    with tempfile.TemporaryDirectory() as d:
        harness = os.path.join(d, "inc_harness.cpp")
        with open(harness, "w") as fh:
            fh.write(INC_HARNESS)
        for name, path in [(u, os.path.join(SHIM, u)) for u in UNITS] + [("Mapper .inc harness", harness)]:
            ok, err = check(path, upstream_src)
            print("%-22s %s" % (name, "ok" if ok else "FAILED"))
            if not ok:
                print(err[-4000:])
                failed.append(name)
        tracker = os.path.join(d, "tracker_harness.cpp")
        with open(tracker, "w") as fh:
            fh.write(TRACKER_HARNESS)
        stubs = tracker_stubs(os.path.join(d, "stubs"))
        cxx = shutil.which("g++") or shutil.which("c++")
        fl = [f.replace(os.path.join(ROOT, "tests", "shim_stubs"), stubs) for f in flags(upstream_src)]
        r = subprocess.run([cxx] + fl + [tracker], capture_output=True, text=True)
        print("%-22s %s" % ("Tracker .inc harness", "ok" if r.returncode == 0 else "FAILED"))
        if r.returncode:
            print(r.stderr[-4000:])
            failed.append("Tracker .inc harness")
        replenish = os.path.join(d, "replenish_harness.cpp")
        with open(replenish, "w") as fh:
            fh.write(REPLENISH_HARNESS)
        r = subprocess.run([cxx] + fl + [replenish], capture_output=True, text=True)
        print("%-22s %s" % ("Replenish .inc harness", "ok" if r.returncode == 0 else "FAILED"))
        if r.returncode:
            print(r.stderr[-4000:])
            failed.append("Replenish .inc harness")
        tail = os.path.join(d, "track_tail_harness.cpp")
        with open(tail, "w") as fh:
            fh.write(TRACK_TAIL_HARNESS)
        r = subprocess.run([cxx] + fl + [tail], capture_output=True, text=True)
        print("%-22s %s" % ("Track tail .inc harness", "ok" if r.returncode == 0 else "FAILED"))
        if r.returncode:
            print(r.stderr[-4000:])
            failed.append("Track tail .inc harness")
        insert = os.path.join(d, "mapper_insert_harness.cpp")
        with open(insert, "w") as fh:
            fh.write(MAPPER_INSERT_HARNESS)
        r = subprocess.run([cxx] + fl + [insert], capture_output=True, text=True)
        print("%-26s %s" % ("Mapper insert .inc harness", "ok" if r.returncode == 0 else "FAILED"))
        if r.returncode:
            print(r.stderr[-4000:])
            failed.append("Mapper insert .inc harness")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main(sys.argv)
