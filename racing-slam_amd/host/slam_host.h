// slam_host.h — host-side C++ mirror of the reference's hot-path interfaces over the C-ABI.
//
// Same names, argument meaning and error behaviour as the reference headers
//   src/MapMatcher.h:16-38, src/Triangulation.h:9-37, src/Optimization.h:21-97, src/LocalWindow.h:13-19
// but on plain array types: OpenCV / Eigen / Ceres are not available in this image, so cv::Mat
// descriptors become a byte vector, Eigen::Matrix4f a row-major std::array<float,16>, etc.
// The data model (Frame / KeyFrame / MapPoint / Map, reference src/Frame.h, src/MapPoint.h,
// src/Map.h) is reduced to what the hot path reads and writes.  Every method marshals the
// pointer graph to the SoA layout of include/rsgpu.h, uploads, calls ONE C-ABI entry point and
// downloads — exactly what the drop-in shims of INTEGRATION.md do with the reference's own types.
// There is no CPU fallback: without a GPU the Session constructor throws.
#pragma once
#include <array>
#include <map>
#include <unordered_map>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <unordered_set>
#include <utility>
#include <string>
#include <vector>

#include "../../include/rsgpu.h"

namespace slam {

struct Vec2f { float x = 0, y = 0; };
struct Vec3f { float x = 0, y = 0, z = 0; };
using Mat4f = std::array<float, 16>;   // row-major world->camera, Frame::pose()

inline Mat4f identity4() { return {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; }

// src/Camera.h:8-25
class Camera {
  public:
    Camera(float fx, float fy, float cx, float cy, int width, int height)
        : m_fx(fx), m_fy(fy), m_cx(cx), m_cy(cy), m_width(width), m_height(height) {}
    float fx() const { return m_fx; }
    float fy() const { return m_fy; }
    float cx() const { return m_cx; }
    float cy() const { return m_cy; }
    int get_width() const { return m_width; }
    int get_height() const { return m_height; }

  private:
    float m_fx, m_fy, m_cx, m_cy;
    int m_width, m_height;
};

// src/features/FeatureExtractor.h:15-38
struct KeyPoint { Vec2f pt; };
struct ExtractedFeatures {
    std::vector<KeyPoint> keypoints;
    std::vector<uint8_t> descriptors;   // N x 32, row-major (cv::Mat N x 32 CV_8U)
    std::vector<float> descriptors_f32; // N x descriptor_dim, row-major (cv::Mat N x dim CV_32F): what a NORM_L2 matcher reads
    int descriptor_dim = 0;             // floats per row of descriptors_f32 (0: none)
};
struct FeatureMatch {
    FeatureMatch(int train, int query) : train_index((size_t)train), query_index((size_t)query) {}
    size_t train_index, query_index;
};

class MapPoint;
class KeyFrame;
struct MapPointMatch { MapPoint& point; size_t keypoint_index; };

// src/Frame.h:18-74 (hot-path subset).  The KD-tree is built at construction like the reference's.
class Frame {
  public:
    Frame(int index, ExtractedFeatures features);
    virtual ~Frame() = default;
    size_t index() const { return m_index; }
    const ExtractedFeatures& features() const { return m_features; }
    const KeyPoint& keypoint(size_t i) const { return m_features.keypoints[i]; }
    const Mat4f& pose() const { return m_pose; }
    void set_pose(const Mat4f& p) { m_pose = p; }
    Vec3f camera_center() const;                               // -R^T t, src/Frame.cpp:39-42
    void add_map_match(const MapPointMatch& m);                // src/Frame.cpp:80-102
    bool is_matched(size_t keypoint_index) const { return m_map_matches[keypoint_index] != nullptr; }
    bool is_matched(const MapPoint& p) const;
    size_t num_map_matches() const { return m_num; }
    std::vector<MapPointMatch> map_matches() const;            // ascending keypoint index, src/Frame.cpp:154-174
    const std::vector<MapPoint*>& match_table() const { return m_map_matches; }   // keypoint -> point or null (what the reference's
                                                               // MapPointIterator walks, src/Frame.h:20-33: no list is built)
    const std::vector<int32_t>& kd_node_kp() const { return m_kd_node_kp; }
    const std::vector<int32_t>& kd_left() const { return m_kd_left; }
    const std::vector<int32_t>& kd_right() const { return m_kd_right; }
    int kd_root() const { return m_kd_root; }

  private:
    size_t m_index;
    ExtractedFeatures m_features;
    Mat4f m_pose = identity4();
    std::vector<MapPoint*> m_map_matches;
    std::unordered_set<const MapPoint*> m_matched_points;      // the points in m_map_matches (src/Frame.h:72): is_matched(point) is a lookup
    size_t m_num = 0;
    std::vector<int32_t> m_kd_node_kp, m_kd_left, m_kd_right;
    int m_kd_root = -1;
};

class KeyFrame : public Frame {
  public:
    explicit KeyFrame(Frame&& f) : Frame(std::move(f)) {}
};

// src/MapPoint.h:12-39.  Observations keep INSERTION order (the reference's unordered_map order is
// unspecified).
class MapPoint {
  public:
    explicit MapPoint(const Vec3f& p) : m_position(p) {}
    const Vec3f& position() const { return m_position; }
    void set_position(const Vec3f& p) { m_position = p; }
    const std::vector<std::pair<KeyFrame*, size_t>>& observations() const { return m_obs; }
    bool is_observed_by(const KeyFrame* kf) const;

  private:
    friend class Map;
    Vec3f m_position;
    std::vector<std::pair<KeyFrame*, size_t>> m_obs;
};

// src/Map.h:12-66 (hot-path subset): owns the points, iteration order = insertion order
class Map {
  public:
    MapPoint& create_point(const Vec3f& position) { m_points.push_back(std::make_unique<MapPoint>(position)); return *m_points.back(); }
    void associate(KeyFrame& kf, MapPoint& point, size_t keypoint_index);   // src/Map.cpp:association
    size_t size() const { return m_points.size(); }
    MapPoint& operator[](size_t i) { return *m_points[i]; }
    const MapPoint& operator[](size_t i) const { return *m_points[i]; }

  private:
    std::vector<std::unique_ptr<MapPoint>> m_points;
};

enum NormTypes { NORM_L2 = 4, NORM_HAMMING = 6 };   // cv::NORM_L2, cv::NORM_HAMMING

// src/MapMatcher.h:16-38.  NORM_HAMMING matches the 32-byte rows (max_descriptor_distance truncated to an int), NORM_L2 the
// float rows (rs_match_descriptors_f32 / rs_reproj_match_l2); any other norm, or frames whose float rows disagree in width,
// match nothing and say so.
class MapMatcher {
  public:
    MapMatcher(const Camera& camera, float max_descriptor_distance, NormTypes norm_type);
    std::vector<MapPointMatch> match_map(const Frame& frame, Map& map) const;
    std::vector<MapPointMatch> match_key_frame(const Frame& frame, Map& map, KeyFrame* key_frame) const;
    std::vector<MapPointMatch> match_for_fuse(const Frame& frame, const std::vector<MapPoint*>& points) const;
    std::vector<MapPointMatch> match_descriptors(const Frame& frame, const KeyFrame& key_frame) const;

  private:
    std::vector<MapPointMatch> match(const Frame& frame, const std::vector<MapPoint*>& points,
                                     const KeyFrame* required_observer, bool replace) const;
    const Camera& m_camera;
    float m_max_descriptor_distance;
    NormTypes m_norm_type;
};

namespace triangulation {
// src/Triangulation.h:9-37
static const float MIN_PARALLAX_COSINE = 0.9999f;
struct TriangulatedPoint { Vec3f position; int match_index; };
std::pair<std::vector<Vec2f>, std::vector<Vec2f>> get_matching_points(const ExtractedFeatures& f1,
                                                                      const ExtractedFeatures& f2,
                                                                      const std::vector<FeatureMatch>& matches);
std::vector<TriangulatedPoint> triangulate_points(const std::vector<Vec2f>& points1, const std::vector<Vec2f>& points2,
                                                  const Mat4f& pose1, const Mat4f& pose2, const Camera& camera,
                                                  float min_parallax_cosine = MIN_PARALLAX_COSINE,
                                                  float max_reprojection_error = 2.0f);
std::vector<TriangulatedPoint> triangulate_points(const Frame& frame1, const Frame& frame2,
                                                  const std::vector<FeatureMatch>& matches, const Camera& camera);
}  // namespace triangulation

namespace tracks {
// The arithmetic body of Mapper::triangulate_tracks (src/Mapper.cpp:246-305) on the types of
// src/TrackStore.h:17-29.  The Mapper keeps the pointer work (window membership, create_point /
// associate, :306-330): it passes the tracks in std::map<TrackId, Track> order together with the
// trajectory poses its sightings refer to and gets back what to create and what to erase.
struct TrackSighting { size_t frame_index = 0; Vec2f pixel; };
struct Track { std::vector<TrackSighting> sightings; size_t keypoint_index = 0; };
struct Candidate {
    size_t track;            // index into the input vector
    Vec3f position;
    size_t keypoint_index;
    float parallax_cosine, required_cosine;
};
struct Selection {
    std::vector<Candidate> accepted;      // creation order: above-threshold in track order, then the quota top-up
    size_t topped_up = 0;
    std::vector<size_t> inconsistent;     // tracks to erase (:332-334)
};
static const float TRACK_MIN_PARALLAX_COSINE = 0.999848f, ROTATION_PARALLAX_FACTOR = 0.20f;
static const float ANY_PARALLAX_COSINE = 1.0f, TRACK_MAX_REPROJECTION_ERROR = 4.0f;
static const size_t MIN_NEW_POINTS_PER_KEY_FRAME = 100;
// `trajectory_poses[i]` = Trajectory::pose_at(i); the key frame contributes its pose and keypoints.
Selection select_track_points(const KeyFrame& key_frame, const std::vector<Track>& tracks,
                              const std::vector<Mat4f>& trajectory_poses, const Camera& camera,
                              size_t min_new_points = MIN_NEW_POINTS_PER_KEY_FRAME);

// The arithmetic of Mapper::cull_points (src/Mapper.cpp:410-419): mean reprojection error of every given point
// over its observations, and which of them exceed the limit.  The Mapper selects the local points (:398-408)
// and removes the returned ones from the map (:426-429).
static const float MAX_POINT_REPROJECTION_ERROR = 3.0f;
struct CullResult {
    std::vector<float> mean_error;            // per input point
    std::vector<size_t> to_remove;            // indices into the input vector, ascending
    double error_sum = 0.0;                   // Slam::reprojection_error() = error_sum / observations (src/Slam.cpp:302-317)
    size_t observations = 0;
};
CullResult point_errors(const std::vector<MapPoint*>& points, const Camera& camera,
                        float max_mean_error = MAX_POINT_REPROJECTION_ERROR);
}  // namespace tracks

namespace optimization {
// src/Optimization.h:23-26, 76-81; src/LocalWindow.h:13-19 (vision-only: InertialInput{} default)
struct FrameConfig { bool optimize; Frame* frame; };
bool refine_pose(Frame& frame, const Camera& camera);
bool bundle_adjust(const std::vector<FrameConfig>& frames, const Camera& camera, Map& map);
std::vector<FrameConfig> build_local_window(const std::vector<std::shared_ptr<KeyFrame>>& key_frames,
                                            Frame& new_frame, size_t window_size, bool fix_oldest = false);
// last solver summary (the reference prints ceres' BriefReport, src/Optimization.cpp:135)
const rs_ba_summary& last_summary();
}  // namespace optimization

// An 8-bit frame (cv::Mat CV_8UC1 / CV_8UC3 BGR), rows packed: pitch = width * channels.
struct Image {
    int width = 0, height = 0, channels = 1;
    std::vector<uint8_t> pixels;
};

// Process-wide device session (one context per process, SURVEY.md §8b "Threading").
class Session {
  public:
    static Session& get();
    rs_context* ctx() const { return m_ctx; }
    ~Session();
    // Tracker::track_features (src/Tracker.cpp:90-131) up to, not including, the replenishment (:133-150): forward and
    // backward pyramidal LK (window 21, 4 levels) and the forward-backward / border / static-mask filter, as ONE
    // rs_track_features call.  Returns {features, matches} of :128-131: the tracked keypoints at their new positions
    // with their descriptor rows, and (previous index, new index) per tracked keypoint.  `mask` with no pixels = none.
    // The session keeps two device pyramids: when `prev` is the Image passed as `next` to the previous call (same
    // object, same buffer, unchanged), its pyramid is reused and only `next` is uploaded.
    std::pair<ExtractedFeatures, std::vector<FeatureMatch>> track_features(const Image& prev, const Image& next,
                                                                           const ExtractedFeatures& prev_features,
                                                                           const Image& mask);
    // Tracker::track_features' replenishment (src/Tracker.cpp:127-146) with the ORB extractor's detector
    // (GFTTDetector(3000, 0.005, 5) + ORB's 31-px border filter, features/OrbFeatureExtractor.cpp:5-27), as ONE
    // rs_detect_features call: the static mask with a filled circle of radius 5 at every keypoint already in `features`,
    // the corners strongest first, and the first max(0, max_total - features.keypoints.size()) of them appended to
    // `features` (max_total < 0: all, the Initialization.cpp:47 / :105 case).  Appended keypoints get zero descriptor
    // rows (when `features` carries rows): the caller's refresh_descriptors (:150) describes every keypoint.  When
    // `next` is the Image passed as `next` to the last track_features call (same object, same buffer, unchanged), its
    // device pyramid is reused and nothing is uploaded.  `static_mask` with no pixels = none; `responses`, if given,
    // receives the appended corners' min-eigenvalues.  Returns the number detected (the reference's "replenished"
    // count), or -1 on failure.
    int replenish_features(const Image& next, const Image& static_mask, ExtractedFeatures& features, int max_total,
                           std::vector<float>* responses = nullptr);
    // OrbFeatureExtractor::refresh_descriptors (features/OrbFeatureExtractor.cpp:29-61, called at src/Tracker.cpp:150)
    // as ONE rs_describe_features call: the ORB descriptor (patch 31, angle -1, one level) of every keypoint of
    // `features` inside ORB's 31-px border on `next`; a keypoint outside it keeps the row the frame carried.  The first
    // matches.size() keypoints are the tracked ones of track_features (matches[k] = (previous index, k)) and carry
    // prev_features' row at their previous index (:130); the rest are appended corners and carry zeros (the rows
    // replenish_features appends).  Returns the N x 32 rows; `features` without keypoints or rows is returned as it
    // is (the reference's early return), and an empty vector on failure.  `next` is reused as replenish_features
    // reuses it: the device pyramid of the last track_features call when it is that call's `next`, else uploaded.
    // Up to 8192 keypoints.
    // With `out_frame`, the same device lists and rows also fill the session's rs_frame (rs_frame_assign_device: KD-tree
    // built on the device, no host pass) in the same chain, and *out_frame is that frame: what rs_map_match and
    // rs_map_add_keyframe take, byte for byte the frame rs_frame_create makes from `features` and the returned rows.  It
    // belongs to the session and is refilled by the next such call; nullptr on failure or on the early return.
    std::vector<uint8_t> refresh_descriptors(const Image& next, const ExtractedFeatures& features,
                                             const ExtractedFeatures& prev_features, const std::vector<FeatureMatch>& matches,
                                             rs_frame** out_frame = nullptr);
    // the relative-pose scratch of pose::estimate_pose* (8192 points, 1000 hypotheses), created on first use
    rs_pose_estimator* pose_estimator();
    // the absolute-pose scratch of pose::estimate_pose_pnp (8192 correspondences, 1000 hypotheses), created on first use
    rs_pnp_estimator* pnp_estimator();

  private:
    Session();
    rs_context* m_ctx = nullptr;
    rs_image* m_pyr[2] = {nullptr, nullptr};    // m_pyr[m_next] holds the last `next` frame
    int m_next = 1, m_pyr_w = 0, m_pyr_h = 0;
    const Image* m_next_image = nullptr;
    const uint8_t* m_next_data = nullptr;
    rs_detector* m_det = nullptr;               // replenish_features: detector scratch and a pyramid of its own
    rs_image* m_det_img = nullptr;              // (used when the frame is not the last tracked one)
    int m_det_w = 0, m_det_h = 0;
    rs_describer* m_orb = nullptr;              // refresh_descriptors: describer plane and a pyramid of its own
    rs_image* m_orb_img = nullptr;
    int m_orb_w = 0, m_orb_h = 0;
    rs_pose_estimator* m_pose = nullptr;
    rs_pnp_estimator* m_pnp = nullptr;
    rs_frame* m_frame = nullptr;                // refresh_descriptors' device-built frame (8192 keypoints), created on first use
};

// src/PoseEstimation.h: the relative pose from prev_features to features (X = R X_prev + t, |t| = 1), Tracker.cpp:162
// and Initialization.cpp:153.  Each is ONE C-ABI call on the device (include/rsgpu.h: rs_estimate_pose /
// rs_estimate_pose_known_rotation) and one read-back.  Up to 8192 matches.
namespace pose {

struct PoseEstimate {
    Mat4f pose = identity4();                    // row-major
    std::vector<FeatureMatch> inlier_matches;    // matches used for the estimate
    int status = -1;                             // rs_estimate_pose's status; -1 = the call failed (logged)
};

// findEssentialMat(USAC_ACCURATE, 0.99, 1.0 px) + recover_pose_from_essential (PoseEstimation.cpp:23-88), as specified
// by tests/essential_ref.py: 1000 hypotheses, seed 0.  Fewer than 5 matches or no model: identity, no inliers.
PoseEstimate estimate_pose(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                           const std::vector<FeatureMatch>& matches, const Camera& camera);
// estimate_pose_with_known_rotation (PoseEstimation.cpp:110-227); rotation row-major.  The 200 (i, j) pairs are the
// reference's draws, known_rotation_pairs(matches.size()).
PoseEstimate estimate_pose_with_known_rotation(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                                               const std::vector<FeatureMatch>& matches, const Camera& camera,
                                               const std::array<float, 9>& rotation);
// std::mt19937(0) and std::uniform_int_distribution<size_t>(0, n - 1), i then j, 200 times (:137-143); [200][2]
std::vector<int32_t> known_rotation_pairs(size_t n);

// cv::solvePnPRansac(object_points, pixels, K, {}, rvec, tvec, false, 200, threshold_px, 0.99, inliers, SOLVEPNP_EPNP) as
// LoopDetector's verify_pnp (src/LoopDetector.cpp:176-229) and Initialization's third-view check
// (src/Initialization.cpp:188-228, 2.0 px) call it, as specified by tests/pnp_ref.py: 200 hypotheses, seed 0.  ONE C-ABI
// call on the device (rs_estimate_pose_pnp) and one read-back.  Up to 8192 correspondences.
struct PnpEstimate {
    Mat4f pose = identity4();                    // row-major, world -> camera
    std::vector<size_t> inliers;                 // indices of the inlier correspondences, ascending
    int status = -1;                             // rs_estimate_pose_pnp's status (0 = solved); -1 = the call failed (logged)
};
PnpEstimate estimate_pose_pnp(const std::vector<Vec3f>& object_points, const std::vector<Vec2f>& pixels, const Camera& camera,
                              double threshold_px);

}  // namespace pose

// The tail of Tracker::track (src/Tracker.cpp:83-86) on the frames' device tables: track_from_last_frame, optimize_pose's
// refit, match_with_last_key_frame and match_with_map as four C-ABI calls (rs_map_carry_matches, rs_map_refine_pose,
// rs_map_match_frame twice) with no host list in between.  prev / next: the rs_frames of the previous and this video
// frame (refresh_descriptors' out_frame); d_prev_index: rs_track_features' d_kept_index; d_inlier_index / d_inlier_count:
// rs_estimate_pose's (null index: every tracked keypoint), each with room for max_n entries.
constexpr int MIN_TRACKED_MAP_POINTS = 15;      // src/Tracker.cpp's
struct TrackTailConstraint {                     // optimization::InertialConstraint, flattened as rs_refine_pose_inertial takes it
    int kind = 0;                                // 0 none, 1 RotationPrior, 2 InertialDelta
    double predicted[9] = {}, sigma_radians = 0.0;
    double prev_pose[6] = {}, prev_velocity[3] = {}, prev_bias[6] = {}, gravity[3] = {}, velocity[3] = {};   // velocity: in / out
    rs_imu_factor delta = {};
};
struct TrackTail {
    int n_used = 0;                              // observations of the refit; -1: fewer than 15 matches, 0: none with 2 observations
    bool refined = false;                        // the solve was usable: `pose` is the refined one (is_rotation_plausible is the caller's)
    rs_ba_summary summary = {};
    int key_frame_matches = 0, map_matches = 0;
};
// `pose` in: the frame's initial pose (Tracker::initial_pose_estimate); out: the refined pose when refined.  `optimize`:
// TrackerConfig::optimize_pose.  last_key_frame: its handle in the map.  False when a call failed (logged).
bool track_tail(rs_context* ctx, rs_map* map, const rs_frame* prev, rs_frame* next, const int32_t* d_prev_index,
                const int32_t* d_inlier_index, const int32_t* d_inlier_count, int max_n, const Camera& camera, bool optimize,
                TrackTailConstraint* constraint, int last_key_frame, Mat4f& pose, TrackTail* out);

// TrackStore (src/TrackStore.h:17-45) on plain types, in the list form the device lists have: the three operations on a
// std::map<id, track> as tests/trackstore_ref.py specifies them.  It is what a host caller would run after downloading the
// lists, the keypoints and the match table, and what DeviceTracks below is held against (tests/test_trackstore_host.py,
// tools/trackstore_time.py).
struct StoredSighting { int32_t frame_index = 0; Vec2f pixel; int32_t key_frame = -1; int32_t keypoint_index = 0; };
struct StoredTrack { std::vector<StoredSighting> sightings; size_t keypoint_index = 0; };
class HostTrackStore {
  public:
    // entry i: current keypoint j = inlier_index[i] (null: i), previous keypoint prev_index[j]; n entries, lists of max_n.
    // The first entry naming a previous keypoint decides for its track; if its current keypoint is taken, the track is dropped.
    void carry_forward(const int32_t* prev_index, const int32_t* inlier_index, int n, int max_n, size_t max_points = 8192);
    void extend(const float* keypoints /*[n][2]*/, size_t n, int frame_index, int key_frame, size_t max_sightings);
    void erase(uint64_t id);
    const std::map<uint64_t, StoredTrack>& tracks() const { return m_tracks; }
    uint64_t next_id() const { return m_next_id; }
    // Mapper::unmapped_tracks (src/Mapper.cpp:103-120) against a match table [n] (point slot or -1)
    size_t unmapped_tracks(const int32_t* table, size_t n, size_t min_sightings = 3, float min_travel = 20.0f) const;

  private:
    std::map<uint64_t, StoredTrack> m_tracks;
    std::unordered_map<size_t, uint64_t> m_by_keypoint;
    uint64_t m_next_id = 0;
};

// The same store on the device (rs_track_store): Slam::step's three call sites and Mapper::triangulate_tracks' loop on the
// front end's device lists.  Per frame: carry_forward, needs_key_frame (the one 24-byte read-back), extend.
struct KeyFrameSighting { int32_t key_frame = -1; int32_t keypoint_index = 0; };
struct DeviceTrackSelection {
    tracks::Selection selection;                 // Candidate::track / inconsistent: positions among the live tracks in id order
    std::vector<size_t> sightings;               // per accepted track (the >= 3 rule of src/Mapper.cpp:326)
    std::vector<std::vector<KeyFrameSighting>> key_frame_sightings;     // per accepted track, sighting order
    size_t out_of_range = 0, tracks = 0;
};
class DeviceTracks {
  public:
    DeviceTracks(rs_context* ctx, int max_points = 8192, int max_sightings = 100);
    ~DeviceTracks();
    DeviceTracks(const DeviceTracks&) = delete;
    DeviceTracks& operator=(const DeviceTracks&) = delete;
    bool valid() const { return m_store != nullptr; }
    rs_track_store* store() const { return m_store; }
    bool carry_forward(const int32_t* d_prev_index, const int32_t* d_inlier_index, const int32_t* d_inlier_count, int max_n);
    // Mapper::needs_key_frame (src/Mapper.cpp:122-140) with the reference's constants; query (null = not wanted) gets the six integers
    bool needs_key_frame(rs_map* map, const rs_frame* frame, int last_key_frame, int frame_gap, int last_key_frame_matches, bool* need,
                         int32_t* query = nullptr);
    bool extend(const rs_frame* frame, int frame_index, int key_frame);
    // d_poses [n_poses][16] = Trajectory::pose_at(pose_base + i), kf_pose the key frame's entry; d_required as rs_triangulate_tracks
    bool triangulate_tracks(const rs_frame* frame, const float* d_poses, int n_poses, int pose_base, int kf_pose, const Camera& camera,
                            const float* d_required, DeviceTrackSelection* out, size_t min_new_points = tracks::MIN_NEW_POINTS_PER_KEY_FRAME);
    bool erase_inconsistent();
    // what the last triangulate_tracks read back, as rs_map_add_track_points takes it (its arrays live in this object)
    const rs_track_results& results() const { return m_results; }

  private:
    rs_context* m_ctx = nullptr;
    rs_track_store* m_store = nullptr;
    int m_max_points = 0;
    rs_track_results m_results{};
    std::vector<int32_t> m_i32;                  // result arrays, made once
    std::vector<float> m_f32;
};

// Mapper::insert (src/Mapper.cpp:152-174) on the resident map, next to track_tail: the tracker's frame with its device match
// table and the track store go in, the key frame comes out inserted, adjusted, re-anchored and culled, with no host pass over
// map objects.  The chain: rs_map_insert_keyframe -> rs_track_store_triangulate -> rs_map_add_track_points ->
// rs_track_store_erase_inconsistent -> rs_map_bundle_adjust -> rs_map_reanchor -> rs_map_cull_points.
struct KeyFrameWindow {
    std::vector<int32_t> key_frames;             // the BA window BEFORE the new key frame (:227-231), in FrameConfig order
    std::vector<uint8_t> optimize;               // FrameConfig::optimize per entry; the new key frame is always optimised
    std::vector<Mat4f> poses;                    // Frame::pose() per entry, as the map holds them: the anchors' poses before (:369-375)
};
struct KeyFrameTrajectory {                      // rs_track_store_triangulate's pose arguments
    const float* d_poses = nullptr; int n_poses = 0, pose_base = 0, kf_pose = 0; const float* d_required = nullptr;
};
struct KeyFrameInsert {
    int key_frame = -1, adopted = 0;
    DeviceTrackSelection selection;              // Mapper::triangulate_tracks' selection (diagnostics)
    std::vector<int32_t> created;                // the point slots of the accepted tracks
    rs_ba_summary summary{};
    std::vector<int32_t> window;                 // the adjusted window: key_frames + the new one
    std::vector<float> poses;                    // [window][16] after the adjustment
    std::vector<int32_t> adjusted; std::vector<float> adjusted_xyz;        // rs_map_bundle_adjust's free points
    std::vector<int32_t> reanchored; std::vector<float> reanchored_xyz;    // the single-observation points carried along
    std::vector<int32_t> culled; std::vector<float> culled_xyz;            // diagnostics.culled (:426-428)
    int local_points = 0;
};
bool insert_key_frame(rs_context* ctx, rs_map* map, DeviceTracks* tracks, const rs_frame* frame, const Mat4f& pose,
                      const KeyFrameWindow& window, const KeyFrameTrajectory& trajectory, const Camera& camera, bool bundle_adjust,
                      bool cull_points, KeyFrameInsert* out);

// LoopDetector::query's "Loop retrieval" stage (src/LoopDetector.cpp:346-373 Impl::score_candidates, :231-265
// rank_candidates) on the device, as specified by tests/bow_ref.py: the DBoW2 vocabulary, one rs_bow and the database of
// the key frames' vectors.  Where the reference computes bow_of lazily per candidate (:351-353, :366-368), every key
// frame is transformed and added once, when it arrives; a query is one rs_bow_database_score call, one read-back of the
// scores and rs_rank_loop_candidates with the reference's constants (:28-32).  LoopVerifier and LoopStreak below take it from there.
struct LoopCandidate {
    size_t entry = 0;                            // index of the key frame in arrival order (Candidate::index)
    float score = 0.0f;
    size_t frame_gap = 0;                        // query frame index - candidate frame index
};
class LoopRetrieval {
  public:
    // vocabulary_path: DBoW2's text format (loadFromTextFile); capacities of the database
    LoopRetrieval(const std::string& vocabulary_path, size_t max_key_frames, size_t max_total_words, float seconds_per_frame);
    ~LoopRetrieval();
    LoopRetrieval(const LoopRetrieval&) = delete;
    LoopRetrieval& operator=(const LoopRetrieval&) = delete;
    bool valid() const { return m_db != nullptr; }
    const rs_vocabulary* vocabulary() const { return m_voc; }
    size_t size() const { return m_frame_index.size(); }
    // the key frame's ORB rows d_desc [max_n][32] and their count d_count [1], both on the device (rs_describe_features'
    // d_desc and d_n): transformed and appended; false on failure (logged), e.g. a full database
    bool add_key_frame(const uint8_t* d_desc, const int32_t* d_count, int max_n, size_t frame_index);
    // the ranked candidates (at most 3) of the key frame added last against all earlier ones
    std::vector<LoopCandidate> query();

  private:
    rs_vocabulary* m_voc = nullptr;
    rs_bow* m_bow = nullptr;
    rs_bow_database* m_db = nullptr;
    double* m_d_score = nullptr;                 // [max_key_frames]
    std::vector<int64_t> m_frame_index;
    std::vector<double> m_score;
    float m_seconds_per_frame = 0.0f;
};

// LoopDetector::query's "Loop verify" stage (src/LoopDetector.cpp:501-506, verify_pnp :176-229) against the resident map,
// as specified by tests/loop_ref.py: ONE C-ABI call (rs_map_verify_loop) and one read-back per query for all candidates.
struct LoopVerification {
    rs_loop_result result{};                     // status, ok, correspondences, inliers, spread, drift, gap, pose
    std::vector<int32_t> query_kp, point, candidate_kp;      // the listed correspondences (inlier_matches when status is 0)
};
class LoopVerifier {
  public:
    // up to max_points keypoints per key frame and max_candidates (<= 8) candidates per query; 200 hypotheses, seed 0
    explicit LoopVerifier(int max_points = 8192, int max_candidates = 3);
    ~LoopVerifier();
    LoopVerifier(const LoopVerifier&) = delete;
    LoopVerifier& operator=(const LoopVerifier&) = delete;
    bool valid() const { return m_verifier != nullptr; }
    // query_kf and candidates are key frames of `map`; empty on failure (logged) or when there is no candidate
    std::vector<LoopVerification> verify(rs_map* map, int query_kf, const std::vector<int32_t>& candidates, const Camera& camera);

  private:
    rs_loop_verifier* m_verifier = nullptr;
    int m_max_points = 0;
    std::vector<rs_loop_result> m_result;
    std::vector<int32_t> m_listed[3];
};

// What LoopDetector::Impl keeps between queries (:324-325, :336) and update_streak (:375-442), over rs_loop_update_streak.
struct LoopConstraint {                          // optimization::PoseGraphConstraint
    size_t from = 0, to = 0;
    std::array<double, 16> relative{};           // row-major pose(query) * inverse(pose(candidate)), f64
    std::vector<std::pair<int32_t, int32_t>> inlier_matches;     // (query keypoint, point slot)
};
class LoopStreak {
  public:
    // one query: `from` = the query's index among the key frames; ranked[i] verified as verifications[i]; candidate_poses[i]
    // the candidate's pose in the map.  Nothing ranked clears the streak.  Returns the chosen candidate or -1.  A constraint
    // whose candidate pose has no inverse is dropped and the streak cleared (-1).
    int update(size_t from, const std::vector<LoopCandidate>& ranked, const std::vector<LoopVerification>& verifications,
               const std::vector<Mat4f>& candidate_poses);
    bool consume_new_loop();
    const std::vector<LoopConstraint>& constraints() const { return m_constraints; }
    size_t streak_length() const { return (size_t)m_state.length; }

  private:
    rs_loop_streak m_state{};
    std::vector<LoopConstraint> m_constraints;
    bool m_new_loop = false;
};

// Slam::step's "LOOP CLOSED" branch (src/Slam.cpp:260-283) on the resident map, next to insert_key_frame: three calls,
// rs_map_pose_graph -> rs_map_fuse_loop (Mapper::fuse_loop with the newest constraint's candidate and inliers) ->
// rs_map_bundle_adjust with the oldest window frame fixed (Mapper::bundle_adjust(query, true)) and its re-anchoring tail,
// rs_map_reanchor.  Nothing walks map objects on the host.
struct LoopClosure {
    bool closed = false;                         // optimization::pose_graph's result; false: nothing after it ran
    rs_ba_summary graph{};
    std::vector<float> graph_poses;              // [key frames][16] after the pose graph
    rs_fuse_report fuse{};
    std::vector<int32_t> sources, removed;       // the old points; the fused-away points in order
    std::vector<int32_t> section_ptr, journal_kp, journal_point, journal_outcome;      // rs_map_fuse_loop's journal
    rs_ba_summary adjust{};
    std::vector<float> poses;                    // [window][16] after the adjustment
    std::vector<int32_t> adjusted; std::vector<float> adjusted_xyz;
    std::vector<int32_t> reanchored; std::vector<float> reanchored_xyz;
};
// loops: every constraint so far, the new one last (LoopStreak::constraints(); from / to are key-frame handles of `map`);
// window: the caller's bundle-adjustment window in order, the query last (`first = size - BA_WINDOW` stays with the caller);
// check: rs_fuse_options::check.  False on failure (logged); a pose graph that is not usable is no failure (closed = false).
bool close_loop(rs_context* ctx, rs_map* map, const std::vector<LoopConstraint>& loops, const std::vector<int32_t>& window,
                const Camera& camera, int max_descriptor_distance, bool four_dof, const double gravity[3], bool bundle_adjust, bool check,
                LoopClosure* out);

}  // namespace slam
