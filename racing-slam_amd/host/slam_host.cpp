// slam_host.cpp — marshalling of the host mirror (slam_host.h) onto the C-ABI of librsgpu.so.
// Pointer graph -> SoA, upload, ONE C-ABI call per interface function, download.
#include "slam_host.h"
#include "../../integration/reference_shim/rs_marshal.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <cstdint>
#include <random>
#include <unordered_map>

namespace slam {

// ------------------------------------------------------------------ device helpers
namespace {

void hip_ok(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// Device arrays of one interface call, carved from the context's staging pool (rs_stage_*, include/rsgpu.h): no
// hipMalloc / hipFree per call, uploads go host -> pinned -> device asynchronously on the context stream, results come
// back with ONE synchronisation per call (fetch ... fetch, stage_sync).
struct StageScope {
    StageScope() { if (rs_stage_begin(Session::get().ctx()) != RS_OK) throw std::runtime_error("rs_stage_begin"); }
};

template <typename T>
class DevBuf {
  public:
    explicit DevBuf(size_t n) : m_n(n)
    {
        if (rs_stage_alloc(Session::get().ctx(), sizeof(T) * (n ? n : 1), (void**)&m_p) != RS_OK) throw std::runtime_error("rs_stage_alloc");
    }
    explicit DevBuf(const std::vector<T>& h) : m_n(h.size())
    {
        if (rs_stage_upload(Session::get().ctx(), h.data(), sizeof(T) * h.size(), (void**)&m_p) != RS_OK) throw std::runtime_error("rs_stage_upload");
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // registers an asynchronous read-back of the first n entries; the vector is filled by stage_sync()
    std::vector<T> fetch(size_t n) const
    {
        std::vector<T> h(n);
        if (n && rs_stage_download(Session::get().ctx(), m_p, sizeof(T) * n, h.data()) != RS_OK) throw std::runtime_error("rs_stage_download");
        return h;           // moved out: the heap block registered above stays where it is
    }
    std::vector<T> download(size_t n) const
    {
        std::vector<T> h = fetch(n);
        stage_sync();
        return h;
    }
    static void stage_sync() { if (rs_stage_sync(Session::get().ctx()) != RS_OK) throw std::runtime_error("rs_stage_sync"); }
    T* get() const { return m_p; }
    size_t size() const { return m_n; }

  private:
    T* m_p = nullptr;
    size_t m_n = 0;
};
inline void stage_sync() { DevBuf<int>::stage_sync(); }

// The reference has no error codes: a failed C-ABI call is logged to stdout like the
// reference logs, and the interface function returns "empty / false".  Nothing throws across it.
bool rs_ok(int rc, const char* what)
{
    if (rc == RS_OK) return true;
    std::printf("%s failed (status %d): %s\n", what, rc, rs_last_error(Session::get().ctx()));
    return false;
}

// the norms MapMatcher has a device path for; anything else is refused loudly, like a failed call
bool norm_supported(int norm_type)
{
    if (norm_type == NORM_HAMMING || norm_type == NORM_L2) return true;
    std::printf("MapMatcher: norm type %d is not supported (NORM_HAMMING on 32-byte rows, NORM_L2 on float rows)\n", norm_type);
    return false;
}

rs_ba_summary g_summary{};

// How the flatten templates of rs_marshal.h read the mirror's objects (the shims' Access reads the reference's:
// integration/reference_shim/rs_shim_common.h).  PtrIndex's tables are thread_local in that header: the flattening is
// re-entrant across threads; the Session (one context, one staging pool) still serves one caller at a time.
struct HostAccess {
    using Point = MapPoint;
    static void position(const MapPoint& p, float out[3]) { out[0] = p.position().x; out[1] = p.position().y; out[2] = p.position().z; }
    static void pose_row_major(const Frame& f, float out[16]) { std::memcpy(out, f.pose().data(), 16 * sizeof(float)); }
    static void center(const Frame& f, float out[3]) { const Vec3f c = f.camera_center(); out[0] = c.x; out[1] = c.y; out[2] = c.z; }
    static void keypoint(const Frame& f, size_t i, float out[2]) { out[0] = f.keypoint(i).pt.x; out[1] = f.keypoint(i).pt.y; }
    static bool descriptor_rows(const Frame& f, const uint8_t*& rows, size_t& n_rows)
    {
        rows = f.features().descriptors.data(); n_rows = f.features().descriptors.size() / RS_DESC_BYTES;
        return true;
    }
    static bool descriptor_rows_f32(const Frame& f, const float*& rows, size_t& n_rows, size_t dim)
    {
        if (dim == 0 || (size_t)f.features().descriptor_dim != dim) return false;
        rows = f.features().descriptors_f32.data(); n_rows = f.features().descriptors_f32.size() / dim;
        return true;
    }
    static size_t n_matches(const Frame& f) { return f.num_map_matches(); }
    template <typename Fn>
    static void for_each_match(const Frame& f, Fn fn)
    {
        const std::vector<MapPoint*>& tab = f.match_table();   // ascending keypoint index, as map_matches(): no list is built
        for (size_t k = 0; k < tab.size(); k++)
            if (tab[k]) fn(*tab[k], k);
    }
    template <typename Fn>
    static void for_each_observation(const MapPoint& p, Fn fn)
    {
        for (const auto& o : p.observations()) fn(o.first, o.second);
    }
    static size_t n_observations(const MapPoint& p) { return p.observations().size(); }
    static const void* observations_address(const MapPoint& p) { return p.observations().data(); }
    static bool is_matched(const Frame& f, const MapPoint& p) { return f.is_matched(p); }
    static bool is_observed_by(const MapPoint& p, const KeyFrame* kf) { return p.is_observed_by(kf); }
};

}  // namespace

Session::Session()
{
    const int rc = rs_context_create(0, &m_ctx);
    if (rc != RS_OK) throw std::runtime_error("rs_context_create failed (no gfx950 GPU? there is no CPU fallback)");
}
Session::~Session()
{
    for (rs_image* p : m_pyr) rs_image_destroy(p);
    rs_image_destroy(m_det_img);
    rs_detector_destroy(m_det);
    rs_image_destroy(m_orb_img);
    rs_describer_destroy(m_orb);
    rs_pose_estimator_destroy(m_pose);
    rs_pnp_estimator_destroy(m_pnp);
    rs_frame_destroy(m_frame);
    rs_context_destroy(m_ctx);
}
Session& Session::get()
{
    static Session s;
    return s;
}

// ------------------------------------------------------------------------ data model
Frame::Frame(int index, ExtractedFeatures features) : m_index((size_t)index), m_features(std::move(features))
{
    const size_t n = m_features.keypoints.size();
    m_map_matches.assign(n, nullptr);
    std::vector<float> kp(2 * n);
    for (size_t i = 0; i < n; i++) { kp[2 * i] = m_features.keypoints[i].pt.x; kp[2 * i + 1] = m_features.keypoints[i].pt.y; }
    m_kd_node_kp.resize(n); m_kd_left.resize(n); m_kd_right.resize(n);
    int32_t root = -1;
    rs_kdtree_build(kp.data(), (int)n, m_kd_node_kp.data(), m_kd_left.data(), m_kd_right.data(), &root);   // src/Frame.cpp:8-15
    m_kd_root = root;
}

Vec3f Frame::camera_center() const
{
    const Mat4f& T = m_pose;
    Vec3f c;
    c.x = (-T[0] * T[3] + -T[4] * T[7]) + -T[8] * T[11];
    c.y = (-T[1] * T[3] + -T[5] * T[7]) + -T[9] * T[11];
    c.z = (-T[2] * T[3] + -T[6] * T[7]) + -T[10] * T[11];
    return c;
}

void Frame::add_map_match(const MapPointMatch& m)
{
    MapPoint* previous = m_map_matches[m.keypoint_index];
    if (previous == &m.point) return;
    if (previous == nullptr) m_num++;
    else m_matched_points.erase(previous);
    for (size_t i = 0; i < m_map_matches.size(); i++) {
        if (m_map_matches[i] != &m.point || i == m.keypoint_index) continue;
        m_map_matches[i] = nullptr;
        if (m_num > 0) m_num--;
    }
    m_map_matches[m.keypoint_index] = &m.point;
    m_matched_points.insert(&m.point);
}

bool Frame::is_matched(const MapPoint& p) const
{
    return m_matched_points.count(&p) != 0;                     // (src/Frame.cpp:148-151)
}

std::vector<MapPointMatch> Frame::map_matches() const
{
    std::vector<MapPointMatch> out;
    for (size_t i = 0; i < m_map_matches.size(); i++)
        if (m_map_matches[i]) out.push_back(MapPointMatch{*m_map_matches[i], i});
    return out;
}

bool MapPoint::is_observed_by(const KeyFrame* kf) const
{
    for (const auto& o : m_obs)
        if (o.first == kf) return true;
    return false;
}

void Map::associate(KeyFrame& kf, MapPoint& point, size_t keypoint_index)
{
    bool found = false;
    for (auto& o : point.m_obs)
        if (o.first == &kf) { o.second = keypoint_index; found = true; }
    if (!found) point.m_obs.emplace_back(&kf, keypoint_index);
    kf.add_map_match(MapPointMatch{point, keypoint_index});
}

// ------------------------------------------------------------------------ MapMatcher
MapMatcher::MapMatcher(const Camera& camera, float max_descriptor_distance, NormTypes norm_type)
    : m_camera(camera), m_max_descriptor_distance(max_descriptor_distance), m_norm_type(norm_type)
{
}

std::vector<MapPointMatch> MapMatcher::match_map(const Frame& frame, Map& map) const
{
    std::vector<MapPoint*> pts(map.size());
    for (size_t i = 0; i < map.size(); i++) pts[i] = &map[i];
    return match(frame, pts, nullptr, false);
}

std::vector<MapPointMatch> MapMatcher::match_key_frame(const Frame& frame, Map& map, KeyFrame* key_frame) const
{
    std::vector<MapPoint*> pts(map.size());
    for (size_t i = 0; i < map.size(); i++) pts[i] = &map[i];
    return match(frame, pts, key_frame, false);
}

std::vector<MapPointMatch> MapMatcher::match_for_fuse(const Frame& frame, const std::vector<MapPoint*>& points) const
{
    return match(frame, points, nullptr, true);
}

// src/MapMatcher.cpp:45-98,117-127,165-175 -> rs_reproj_match
std::vector<MapPointMatch> MapMatcher::match(const Frame& frame, const std::vector<MapPoint*>& points,
                                             const KeyFrame* required_observer, bool replace) const
{
    rs_context* ctx = Session::get().ctx();
    const size_t N = frame.features().keypoints.size(), P = points.size();
    if (N == 0) return {};
    // frame side
    std::vector<float> kp(2 * N);
    std::vector<uint8_t> matched(N);
    for (size_t i = 0; i < N; i++) {
        kp[2 * i] = frame.keypoint(i).pt.x; kp[2 * i + 1] = frame.keypoint(i).pt.y;
        matched[i] = frame.is_matched(i) ? 1 : 0;
    }
    if (!norm_supported(m_norm_type)) return {};
    const bool l2 = m_norm_type == NORM_L2;
    const size_t dim = l2 ? (size_t)frame.features().descriptor_dim : 0;
    if (l2 && (dim == 0 || frame.features().descriptors_f32.size() != N * dim)) {
        std::printf("MapMatcher: NORM_L2 needs N x descriptor_dim float rows on the frame\n");
        return {};
    }
    // map side: positions, eligibility, observation CSR, keyframe table and descriptor pool
    const rs_marshal::MatchArrays m = l2 ? rs_marshal::flatten_match<true>(frame, points, required_observer, HostAccess{}, dim)
                                         : rs_marshal::flatten_match(frame, points, required_observer, HostAccess{});
    if (m.refused) {
        std::printf("MapMatcher: a key frame's descriptor rows are not %zu floats wide\n", dim);
        return {};
    }
    StageScope stage;
    DevBuf<float> d_kp(kp), d_pos(m.pos), d_centers(m.centers);
    DevBuf<uint8_t> d_matched(matched), d_elig(m.eligible);
    DevBuf<int32_t> d_nk(frame.kd_node_kp()), d_l(frame.kd_left()), d_r(frame.kd_right()), d_optr(m.obs_ptr), d_okf(m.obs_kf),
        d_odesc(m.obs_desc);
    rs_frame_view fv{};
    std::memcpy(fv.pose, frame.pose().data(), sizeof fv.pose);
    fv.fx = m_camera.fx(); fv.fy = m_camera.fy(); fv.cx = m_camera.cx(); fv.cy = m_camera.cy();
    fv.width = m_camera.get_width(); fv.height = m_camera.get_height();
    fv.n_keypoints = (int)N; fv.d_keypoints = d_kp.get(); fv.d_kp_matched = d_matched.get();
    fv.d_kd_node_kp = d_nk.get(); fv.d_kd_left = d_l.get(); fv.d_kd_right = d_r.get(); fv.kd_root = frame.kd_root();
    rs_map_view mv{};
    mv.n_points = (int)P; mv.d_positions = d_pos.get(); mv.d_eligible = d_elig.get(); mv.d_obs_ptr = d_optr.get();
    mv.d_obs_kf = d_okf.get(); mv.d_obs_desc = d_odesc.get(); mv.d_kf_centers = d_centers.get();
    DevBuf<int32_t> pk(P), pp(N), mkp(N), mpt(N), cnt(1);
    if (l2) {
        DevBuf<float> d_rows(frame.features().descriptors_f32), d_pool(m.pool_f32), pd(P), pdist(N);
        if (!rs_ok(rs_reproj_match_l2(ctx, &fv, &mv, d_rows.get(), d_pool.get(), (int)dim, replace ? 1 : 0, m_max_descriptor_distance,
                                      pk.get(), pd.get(), pp.get(), pdist.get(), mkp.get(), mpt.get(), cnt.get()), "rs_reproj_match_l2"))
            return {};
    } else {
        DevBuf<uint8_t> d_desc(frame.features().descriptors), d_pool(m.pool);
        DevBuf<int32_t> pd(P), pdist(N);
        fv.d_descriptors = d_desc.get(); mv.d_desc_pool = d_pool.get();
        if (!rs_ok(rs_reproj_match(ctx, &fv, &mv, replace ? 1 : 0, (int)m_max_descriptor_distance, pk.get(), pd.get(), pp.get(),
                                   pdist.get(), mkp.get(), mpt.get(), cnt.get()), "rs_reproj_match"))
            return {};
    }
    const auto hn = cnt.fetch(1);
    const auto hk = mkp.fetch(N), hp = mpt.fetch(N);          // at most N matches: one read-back, one synchronisation
    stage_sync();
    const int n = hn[0];
    std::vector<MapPointMatch> out;
    for (int i = 0; i < n; i++) out.push_back(MapPointMatch{*points[(size_t)hp[i]], (size_t)hk[i]});
    return out;
}

// src/MapMatcher.cpp:129-163 -> rs_match_descriptors
std::vector<MapPointMatch> MapMatcher::match_descriptors(const Frame& frame, const KeyFrame& key_frame) const
{
    rs_context* ctx = Session::get().ctx();
    if (!norm_supported(m_norm_type)) return {};
    const auto km = key_frame.map_matches();                  // ascending keypoint order
    const int nq = (int)frame.features().keypoints.size(), nt = (int)km.size();
    if (nt == 0 || nq == 0) return {};                        // :139-141
    StageScope stage;
    DevBuf<int32_t> mq((size_t)nq), mt((size_t)nq), cnt(1);
    if (m_norm_type == NORM_L2) {
        const size_t dim = (size_t)frame.features().descriptor_dim;
        if (dim == 0 || (size_t)key_frame.features().descriptor_dim != dim || frame.features().descriptors_f32.size() != (size_t)nq * dim) {
            std::printf("MapMatcher: NORM_L2 needs float rows of one width on both frames\n");
            return {};
        }
        std::vector<float> train;
        for (const auto& m : km) {
            const float* row = key_frame.features().descriptors_f32.data() + dim * m.keypoint_index;
            train.insert(train.end(), row, row + dim);
        }
        DevBuf<float> dq(frame.features().descriptors_f32), dt(train);
        if (!rs_ok(rs_match_descriptors_f32(ctx, dq.get(), nq, dt.get(), nt, (int)dim, 1, m_max_descriptor_distance, mq.get(), mt.get(),
                                            cnt.get(), nullptr, nullptr, nullptr, nullptr), "rs_match_descriptors_f32"))
            return {};
    } else {
        std::vector<uint8_t> train;
        for (const auto& m : km) {
            const uint8_t* row = key_frame.features().descriptors.data() + 32 * m.keypoint_index;
            train.insert(train.end(), row, row + 32);
        }
        DevBuf<uint8_t> dq(frame.features().descriptors), dt(train);
        if (!rs_ok(rs_match_descriptors(ctx, dq.get(), nq, dt.get(), nt, 1, (int)m_max_descriptor_distance, mq.get(), mt.get(),
                                        cnt.get(), nullptr, nullptr, nullptr, nullptr), "rs_match_descriptors"))
            return {};
    }
    const auto hn = cnt.fetch(1);
    const auto hq = mq.fetch((size_t)nq), ht = mt.fetch((size_t)nq);
    stage_sync();
    const int n = hn[0];
    std::vector<MapPointMatch> out;
    for (int i = 0; i < n; i++) out.push_back(MapPointMatch{km[(size_t)ht[i]].point, (size_t)hq[i]});   // :159-160
    return out;
}

// --------------------------------------------------------------------- triangulation
namespace triangulation {

std::pair<std::vector<Vec2f>, std::vector<Vec2f>> get_matching_points(const ExtractedFeatures& f1, const ExtractedFeatures& f2,
                                                                      const std::vector<FeatureMatch>& matches)
{
    std::vector<Vec2f> p1, p2;
    for (const auto& m : matches) {                            // src/Triangulation.cpp:11-26
        p1.push_back(f1.keypoints[m.train_index].pt);
        p2.push_back(f2.keypoints[m.query_index].pt);
    }
    return {p1, p2};
}

std::vector<TriangulatedPoint> triangulate_points(const std::vector<Vec2f>& points1, const std::vector<Vec2f>& points2,
                                                  const Mat4f& pose1, const Mat4f& pose2, const Camera& camera,
                                                  float min_parallax_cosine, float max_reprojection_error)
{
    if (points1.empty() || points2.empty()) return {};         // :46-48
    rs_context* ctx = Session::get().ctx();
    const size_t n = points1.size();
    // host in, host out: Vec2f is two packed floats, so the vectors ARE the [n][2] arrays.  Up to 256 correspondences
    // (Mapper::triangulate_tracks calls this with ONE) take a single launch with the result in pinned memory.
    static_assert(sizeof(Vec2f) == 2 * sizeof(float), "Vec2f must be two packed floats");
    std::vector<int32_t> hi(n);
    std::vector<float> hx(3 * n);
    int m = 0;
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    if (!rs_ok(rs_triangulate_host(ctx, &points1[0].x, &points2[0].x, (int)n, pose1.data(), pose2.data(), K, min_parallax_cosine,
                                   max_reprojection_error, hi.data(), hx.data(), &m), "rs_triangulate_host"))
        return {};
    std::vector<TriangulatedPoint> out((size_t)m);
    for (int i = 0; i < m; i++) out[(size_t)i] = TriangulatedPoint{Vec3f{hx[3 * i], hx[3 * i + 1], hx[3 * i + 2]}, hi[(size_t)i]};
    return out;
}

std::vector<TriangulatedPoint> triangulate_points(const Frame& frame1, const Frame& frame2,
                                                  const std::vector<FeatureMatch>& matches, const Camera& camera)
{
    auto pts = get_matching_points(frame1.features(), frame2.features(), matches);   // :28-35
    return triangulate_points(pts.first, pts.second, frame1.pose(), frame2.pose(), camera);
}

}  // namespace triangulation

// ---------------------------------------------------------------------- track triangulation
namespace tracks {

// src/Mapper.cpp:246-305 -> rs_triangulate_tracks
Selection select_track_points(const KeyFrame& key_frame, const std::vector<Track>& tracks,
                              const std::vector<Mat4f>& trajectory_poses, const Camera& camera, size_t min_new_points)
{
    Selection out;
    const size_t T = tracks.size();
    if (T == 0) return out;
    rs_context* ctx = Session::get().ctx();
    std::vector<float> track_uv(2 * T), sight_uv, poses(16 * (trajectory_poses.size() + 1));
    std::vector<uint8_t> skip(T);
    std::vector<int32_t> sight_ptr(T + 1, 0), sight_pose;
    for (size_t t = 0; t < T; t++) {
        const Track& tr = tracks[t];
        skip[t] = (key_frame.is_matched(tr.keypoint_index) || tr.sightings.empty()) ? 1 : 0;     // :248-250
        const Vec2f px = key_frame.keypoint(tr.keypoint_index).pt;
        track_uv[2 * t] = px.x; track_uv[2 * t + 1] = px.y;
        for (const auto& sg : tr.sightings) {
            sight_pose.push_back((int32_t)sg.frame_index);
            sight_uv.push_back(sg.pixel.x); sight_uv.push_back(sg.pixel.y);
        }
        sight_ptr[t + 1] = (int32_t)sight_pose.size();
    }
    for (size_t i = 0; i < trajectory_poses.size(); i++) std::memcpy(&poses[16 * i], trajectory_poses[i].data(), 64);
    const int kf_pose = (int)trajectory_poses.size();                                         // key_frame.pose(), :257
    std::memcpy(&poses[16 * (size_t)kf_pose], key_frame.pose().data(), 64);
    if (sight_pose.empty()) { sight_pose.push_back(0); sight_uv.resize(2); }
    StageScope stage;
    DevBuf<float> d_tuv(track_uv), d_suv(sight_uv), d_poses(poses), d_xyz(3 * T), d_pc(T), d_rc(T);
    DevBuf<uint8_t> d_skip(skip), d_status(T);
    DevBuf<int32_t> d_sptr(sight_ptr), d_spose(sight_pose), d_acc(T), d_inc(T), d_cnt(3);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    // the rotation-dependent requirement per first-sighting pose on the HOST (libm as the reference calls it, :281-288)
    std::vector<float> required((size_t)kf_pose + 1);
    if (!rs_ok(rs_parallax_requirements(poses.data(), kf_pose + 1, kf_pose, TRACK_MIN_PARALLAX_COSINE, ROTATION_PARALLAX_FACTOR,
                                        required.data()), "rs_parallax_requirements"))
        return out;
    DevBuf<float> d_req(required);
    if (!rs_ok(rs_triangulate_tracks(ctx, (int)T, d_tuv.get(), d_skip.get(), d_sptr.get(), d_spose.get(), d_suv.get(),
                                     d_poses.get(), kf_pose + 1, kf_pose, K, ANY_PARALLAX_COSINE,
                                     TRACK_MAX_REPROJECTION_ERROR, TRACK_MIN_PARALLAX_COSINE, ROTATION_PARALLAX_FACTOR,
                                     (int)min_new_points, d_status.get(), d_xyz.get(), d_pc.get(), d_rc.get(), d_acc.get(),
                                     d_inc.get(), d_cnt.get(), d_req.get()), "rs_triangulate_tracks"))
        return out;
    const auto cnt = d_cnt.fetch(3);
    const auto acc = d_acc.fetch(T);
    const auto inc = d_inc.fetch(T);
    const auto xyz = d_xyz.fetch(3 * T);
    const auto pc = d_pc.fetch(T), rc = d_rc.fetch(T);
    stage_sync();
    for (int i = 0; i < cnt[0]; i++) {
        const int32_t t = acc[(size_t)i];
        out.accepted.push_back(Candidate{(size_t)t, Vec3f{xyz[3 * (size_t)t], xyz[3 * (size_t)t + 1], xyz[3 * (size_t)t + 2]},
                                         tracks[(size_t)t].keypoint_index, pc[(size_t)t], rc[(size_t)t]});
    }
    out.topped_up = (size_t)cnt[1];
    for (int i = 0; i < cnt[2]; i++) out.inconsistent.push_back((size_t)inc[(size_t)i]);
    return out;
}

// src/Mapper.cpp:410-419 (+ src/Slam.cpp:302-317) -> rs_point_errors
CullResult point_errors(const std::vector<MapPoint*>& points, const Camera& camera, float max_mean_error)
{
    CullResult out;
    const size_t P = points.size();
    if (P == 0) return out;
    rs_context* ctx = Session::get().ctx();
    const rs_marshal::PointErrorArrays e = rs_marshal::flatten_point_errors(points, HostAccess{});
    if (e.obs_pose.empty()) { out.mean_error.assign(P, 0.0f); return out; }
    StageScope stage;
    DevBuf<float> d_pos(e.pos), d_uv(e.uv), d_poses(e.poses), d_mean(P);
    DevBuf<int32_t> d_ptr(e.obs_ptr), d_op(e.obs_pose), d_idx(P), d_cnt(1);
    DevBuf<uint8_t> d_cull(P);
    DevBuf<double> d_sums(2);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    if (!rs_ok(rs_point_errors(ctx, (int)P, d_pos.get(), d_ptr.get(), d_op.get(), d_uv.get(), d_poses.get(), e.n_poses, K,
                               max_mean_error, d_mean.get(), d_cull.get(), d_idx.get(), d_cnt.get(), d_sums.get()), "rs_point_errors"))
        return out;
    out.mean_error = d_mean.fetch(P);
    const auto hn = d_cnt.fetch(1);
    const auto hidx = d_idx.fetch(P);
    const auto sums = d_sums.fetch(2);
    stage_sync();
    for (int i = 0; i < hn[0]; i++) out.to_remove.push_back((size_t)hidx[(size_t)i]);
    out.error_sum = sums[0];
    out.observations = (size_t)sums[1];
    return out;
}

}  // namespace tracks

// ---------------------------------------------------------------------- optimisation
namespace optimization {

const rs_ba_summary& last_summary() { return g_summary; }

// src/Optimization.cpp:194-267 (vision-only) -> rs_refine_pose
bool refine_pose(Frame& frame, const Camera& camera)
{
    rs_context* ctx = Session::get().ctx();
    const rs_marshal::RefineArrays r = rs_marshal::flatten_refine(frame, HostAccess{});    // MIN_OBSERVATIONS_TO_OPTIMIZE, :98,:206
    const std::vector<float>& uv = r.uv;
    if (uv.empty()) return false;                              // :227-229
    double cam[6];
    rs_pack_pose(frame.pose().data(), cam);
    StageScope stage;
    DevBuf<double> dp(r.pts);
    DevBuf<float> duv(uv);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    if (!rs_ok(rs_refine_pose(ctx, cam, dp.get(), duv.get(), (int)(uv.size() / 2), K, nullptr, &g_summary), "rs_refine_pose")) return false;
    std::printf("refine_pose: iterations %d, cost %.6e -> %.6e, termination %d\n", g_summary.iterations,
                g_summary.initial_cost, g_summary.final_cost, g_summary.termination);
    if (!g_summary.usable) { std::printf("Optimization rejected, unusable or non-improving solution\n"); return false; }
    Mat4f T;
    rs_unpack_pose(cam, T.data());
    frame.set_pose(T);
    return true;
}

// src/Optimization.cpp:269-374 (vision-only) -> rs_bundle_adjust
bool bundle_adjust(const std::vector<FrameConfig>& frames, const Camera& camera, Map&)
{
    rs_context* ctx = Session::get().ctx();
    const size_t C = frames.size();
    const auto b = rs_marshal::flatten_ba(frames, HostAccess{});
    const size_t P = b.free_pts.size();
    if (P == 0 || b.obs_cam.empty()) return false;
    StageScope stage;
    DevBuf<double> dc(b.cams), dp(b.pts);
    DevBuf<int32_t> dptr(b.obs_ptr), dcam(b.obs_cam);
    DevBuf<float> duv(b.obs_uv);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    if (!rs_ok(rs_bundle_adjust(ctx, (int)C, (int)P, (int)b.obs_cam.size(), dc.get(), b.cam_free.data(), dp.get(), dptr.get(), dcam.get(),
                                duv.get(), K, nullptr, &g_summary), "rs_bundle_adjust"))
        return false;
    std::printf("bundle_adjust: iterations %d, cost %.6e -> %.6e, termination %d\n", g_summary.iterations,
                g_summary.initial_cost, g_summary.final_cost, g_summary.termination);
    if (!g_summary.usable) { std::printf("Optimization rejected, unusable or non-improving solution\n"); return false; }
    std::vector<double> hc(6 * C);
    rs_ba_get_cameras(ctx, hc.data(), (int)C);                  // pinned mirror written by the solve's last kernel
    const auto hp = dp.download(3 * P);
    for (size_t c = 0; c < C; c++)
        if (frames[c].optimize) { Mat4f T; rs_unpack_pose(&hc[6 * c], T.data()); frames[c].frame->set_pose(T); }   // :363-368
    for (size_t p = 0; p < P; p++) b.free_pts[p]->set_position(Vec3f{(float)hp[3 * p], (float)hp[3 * p + 1], (float)hp[3 * p + 2]});
    return true;
}

// src/LocalWindow.cpp:10-52 -> rs_build_local_window
std::vector<FrameConfig> build_local_window(const std::vector<std::shared_ptr<KeyFrame>>& key_frames, Frame& new_frame,
                                            size_t window_size, bool fix_oldest)
{
    const int n = (int)key_frames.size();
    const rs_marshal::WindowArrays w = rs_marshal::flatten_local_window(key_frames, new_frame, HostAccess{});
    std::vector<int32_t> of((size_t)n + 1);
    std::vector<uint8_t> oo((size_t)n + 1);
    int32_t cnt = 0;
    if (rs_build_local_window(n, w.new_index, (int)window_size, fix_oldest ? 1 : 0, w.frame_ptr.data(), w.frame_pt.data(), w.pt_ptr.data(),
                              w.pt_obs.data(), of.data(), oo.data(), &cnt) != RS_OK)
        return {};
    std::vector<FrameConfig> out;
    for (int i = 0; i < cnt; i++) {
        Frame* f = of[(size_t)i] == n ? &new_frame : key_frames[(size_t)of[(size_t)i]].get();
        out.push_back(FrameConfig{oo[(size_t)i] != 0, f});
    }
    return out;
}

}  // namespace optimization
// ------------------------------------------------------------------------ Tracker::track_features (src/Tracker.cpp:90-131)
std::pair<ExtractedFeatures, std::vector<FeatureMatch>> Session::track_features(const Image& prev, const Image& next,
                                                                                const ExtractedFeatures& prev_features,
                                                                                const Image& mask)
{
    constexpr int KLT_WINDOW = 21, KLT_PYRAMID_LEVELS = 4;     // src/Tracker.cpp:17-19
    constexpr float KLT_MAX_FORWARD_BACKWARD_ERROR = 1.0F;
    ExtractedFeatures features;
    std::vector<FeatureMatch> matches;
    const int W = next.width, H = next.height;
    if (prev.width != W || prev.height != H || prev.pixels.size() < (size_t)W * H * prev.channels ||
        next.pixels.size() < (size_t)W * H * next.channels || (!mask.pixels.empty() && (mask.width != W || mask.height != H))) {
        std::printf("track_features: frames / mask differ in size\n");
        return {};
    }
    if (m_pyr_w != W || m_pyr_h != H) {
        for (rs_image*& p : m_pyr) { rs_image_destroy(p); p = nullptr; }
        for (rs_image*& p : m_pyr)
            if (!rs_ok(rs_image_create(m_ctx, W, H, KLT_PYRAMID_LEVELS, KLT_WINDOW, &p), "rs_image_create")) { m_pyr_w = 0; return {}; }
        m_pyr_w = W;
        m_pyr_h = H;
        m_next_image = nullptr;
    }
    if (m_next_image == &prev && m_next_data == prev.pixels.data()) {
        m_next ^= 1;                                            // the last call's next frame is this call's previous frame
    } else if (!rs_ok(rs_image_upload(m_ctx, m_pyr[m_next ^ 1], prev.pixels.data(), W * prev.channels, prev.channels), "rs_image_upload")) {
        m_next_image = nullptr;
        return {};
    }
    m_next_image = nullptr;
    if (!rs_ok(rs_image_upload(m_ctx, m_pyr[m_next], next.pixels.data(), W * next.channels, next.channels), "rs_image_upload")) return {};
    m_next_image = &next;
    m_next_data = next.pixels.data();
    const size_t n = prev_features.keypoints.size();
    std::vector<float> pts(2 * n);
    for (size_t i = 0; i < n; i++) {
        pts[2 * i] = prev_features.keypoints[i].pt.x;
        pts[2 * i + 1] = prev_features.keypoints[i].pt.y;
    }
    StageScope scope;
    DevBuf<float> d_pts(pts), d_kept_pt(2 * n);
    DevBuf<int32_t> d_kept(n), d_count(1);
    std::unique_ptr<DevBuf<uint8_t>> d_mask;
    if (!mask.pixels.empty()) d_mask = std::make_unique<DevBuf<uint8_t>>(mask.pixels);
    if (!rs_ok(rs_track_features(m_ctx, m_pyr[m_next ^ 1], m_pyr[m_next], d_pts.get(), (int)n, d_mask ? d_mask->get() : nullptr,
                                 KLT_MAX_FORWARD_BACKWARD_ERROR, d_kept.get(), d_kept_pt.get(), d_count.get()), "rs_track_features"))
        return {};
    const auto count = d_count.fetch(1);
    const auto kept = d_kept.fetch(n);
    const auto kept_pt = d_kept_pt.fetch(2 * n);
    stage_sync();
    const size_t m = (size_t)count[0];
    features.keypoints.reserve(m);
    features.descriptors.reserve(m * RS_DESC_BYTES);
    matches.reserve(m);
    const bool with_desc = prev_features.descriptors.size() >= n * RS_DESC_BYTES;
    for (size_t k = 0; k < m; k++) {                            // :128-130
        const size_t i = (size_t)kept[k];
        KeyPoint kp = prev_features.keypoints[i];
        kp.pt = Vec2f{kept_pt[2 * k], kept_pt[2 * k + 1]};
        matches.emplace_back((int)i, (int)features.keypoints.size());
        features.keypoints.push_back(kp);
        if (with_desc)
            features.descriptors.insert(features.descriptors.end(), prev_features.descriptors.begin() + i * RS_DESC_BYTES,
                                        prev_features.descriptors.begin() + (i + 1) * RS_DESC_BYTES);
    }
    return {std::move(features), std::move(matches)};
}

// ------------------------------------------------------------------------ Tracker::track_features (src/Tracker.cpp:127-146)
int Session::replenish_features(const Image& next, const Image& static_mask, ExtractedFeatures& features, int max_total,
                                std::vector<float>* responses)
{
    constexpr int KLT_REPLENISH_RADIUS = 5;                     // src/Tracker.cpp:20
    constexpr int GFTT_MAX_CORNERS = 3000, ORB_EDGE = 31;       // cv::GFTTDetector::create(3000, 0.005, 5), ORB's border
    constexpr double GFTT_QUALITY = 0.005, GFTT_MIN_DISTANCE = 5.0;
    const int W = next.width, H = next.height;
    if (next.pixels.size() < (size_t)W * H * next.channels ||
        (!static_mask.pixels.empty() && (static_mask.width != W || static_mask.height != H))) {
        std::printf("replenish_features: frame / mask differ in size\n");
        return -1;
    }
    if (m_det_w != W || m_det_h != H) {
        rs_detector_destroy(m_det);
        rs_image_destroy(m_det_img);
        m_det = nullptr;
        m_det_img = nullptr;
        m_det_w = m_det_h = 0;
        if (!rs_ok(rs_detector_create(m_ctx, W, H, GFTT_MAX_CORNERS, 3, 3, &m_det), "rs_detector_create") ||
            !rs_ok(rs_image_create(m_ctx, W, H, 0, 5, &m_det_img), "rs_image_create"))
            return -1;
        m_det_w = W;
        m_det_h = H;
    }
    const rs_image* img = m_det_img;
    if (m_next_image == &next && m_next_data == next.pixels.data() && m_pyr_w == W && m_pyr_h == H) {
        img = m_pyr[m_next];                                    // the frame track_features just uploaded
    } else if (!rs_ok(rs_image_upload(m_ctx, m_det_img, next.pixels.data(), W * next.channels, next.channels), "rs_image_upload")) {
        return -1;
    }
    const size_t n_ex = features.keypoints.size();
    std::vector<float> ex(2 * std::max<size_t>(n_ex, 1));
    for (size_t i = 0; i < n_ex; i++) {
        ex[2 * i] = features.keypoints[i].pt.x;
        ex[2 * i + 1] = features.keypoints[i].pt.y;
    }
    StageScope scope;
    DevBuf<float> d_ex(ex), d_pt(2 * GFTT_MAX_CORNERS), d_resp(GFTT_MAX_CORNERS);
    DevBuf<int32_t> d_ex_count(std::vector<int32_t>{(int32_t)n_ex}), d_counts(2);
    std::unique_ptr<DevBuf<uint8_t>> d_mask;
    if (!static_mask.pixels.empty()) d_mask = std::make_unique<DevBuf<uint8_t>>(static_mask.pixels);
    if (!rs_ok(rs_detect_features(m_ctx, m_det, img, d_mask ? d_mask->get() : nullptr, d_ex.get(), d_ex_count.get(),
                                  KLT_REPLENISH_RADIUS, GFTT_MAX_CORNERS, GFTT_QUALITY, GFTT_MIN_DISTANCE, ORB_EDGE, max_total,
                                  d_pt.get(), d_resp.get(), d_counts.get()), "rs_detect_features"))
        return -1;
    const auto counts = d_counts.fetch(2);
    const auto pt = d_pt.fetch(2 * GFTT_MAX_CORNERS);
    const auto resp = d_resp.fetch(GFTT_MAX_CORNERS);
    stage_sync();
    const bool with_desc = features.descriptors.size() == n_ex * RS_DESC_BYTES;
    for (int k = 0; k < counts[1]; k++) {                       // :140-146
        KeyPoint kp;
        kp.pt = Vec2f{pt[2 * (size_t)k], pt[2 * (size_t)k + 1]};
        features.keypoints.push_back(kp);
        if (with_desc) features.descriptors.insert(features.descriptors.end(), RS_DESC_BYTES, (uint8_t)0);
        if (responses) responses->push_back(resp[(size_t)k]);
    }
    return counts[0];
}

std::vector<uint8_t> Session::refresh_descriptors(const Image& next, const ExtractedFeatures& features,
                                                  const ExtractedFeatures& prev_features, const std::vector<FeatureMatch>& matches,
                                                  rs_frame** out_frame)
{
    if (out_frame) *out_frame = nullptr;
    constexpr int ORB_EDGE = 31, MAX_POINTS = 8192;              // ORB::create()'s edgeThreshold; rs_describer's envelope
    const size_t n = features.keypoints.size(), m = matches.size();
    if (n == 0 || features.descriptors.empty()) return features.descriptors;     // :32-34
    const int W = next.width, H = next.height;
    if (next.pixels.size() < (size_t)W * H * next.channels || n > (size_t)MAX_POINTS || m > n) {
        std::printf("refresh_descriptors: bad frame, more than %d keypoints, or more matches than keypoints\n", MAX_POINTS);
        return {};
    }
    if (m_orb_w != W || m_orb_h != H) {
        rs_describer_destroy(m_orb);
        rs_image_destroy(m_orb_img);
        m_orb = nullptr;
        m_orb_img = nullptr;
        m_orb_w = m_orb_h = 0;
        if (!rs_ok(rs_describer_create(m_ctx, W, H, MAX_POINTS, &m_orb), "rs_describer_create") ||
            !rs_ok(rs_image_create(m_ctx, W, H, 0, 5, &m_orb_img), "rs_image_create"))
            return {};
        m_orb_w = W;
        m_orb_h = H;
    }
    const rs_image* img = m_orb_img;
    if (m_next_image == &next && m_next_data == next.pixels.data() && m_pyr_w == W && m_pyr_h == H) {
        img = m_pyr[m_next];                                    // the frame track_features just uploaded
    } else if (!rs_ok(rs_image_upload(m_ctx, m_orb_img, next.pixels.data(), W * next.channels, next.channels), "rs_image_upload")) {
        return {};
    }
    // list a: the tracked keypoints with (previous index) from matches; list b: the appended ones
    std::vector<float> pa(2 * std::max<size_t>(m, 1)), pb(2 * std::max<size_t>(n - m, 1));
    std::vector<int32_t> carry_index(std::max<size_t>(m, 1));
    for (size_t k = 0; k < n; k++) {
        float* p = k < m ? &pa[2 * k] : &pb[2 * (k - m)];
        p[0] = features.keypoints[k].pt.x;
        p[1] = features.keypoints[k].pt.y;
    }
    for (size_t k = 0; k < m; k++) carry_index[k] = (int32_t)matches[k].train_index;
    const size_t n_prev = prev_features.descriptors.size() / RS_DESC_BYTES;
    StageScope scope;
    DevBuf<float> d_pa(pa), d_pb(pb);
    DevBuf<int32_t> d_carry_index(carry_index), d_counts(std::vector<int32_t>{(int32_t)m, (int32_t)(n - m)}), d_n(1);
    std::unique_ptr<DevBuf<uint8_t>> d_prev;
    if (n_prev) d_prev = std::make_unique<DevBuf<uint8_t>>(prev_features.descriptors);
    DevBuf<uint8_t> d_desc((size_t)MAX_POINTS * RS_DESC_BYTES);
    if (!rs_ok(rs_describe_features(m_ctx, m_orb, img, d_pa.get(), d_counts.get(), d_carry_index.get(),
                                    d_prev ? d_prev->get() : nullptr, (int)n_prev, d_pb.get(), d_counts.get() + 1, ORB_EDGE,
                                    d_desc.get(), nullptr, d_n.get()), "rs_describe_features"))
        return {};
    auto rows = d_desc.fetch(n * RS_DESC_BYTES);                // the one read-back: n x 32 bytes
    if (out_frame) {
        // the frame of rs_map_match / rs_map_add_keyframe from the same device lists and rows: no host pass, KD-tree built
        // on the device (csrc/frame.hip).  One frame per session, allocated once, refilled per video frame.
        int n_frame = -1;
        if ((!m_frame && !rs_ok(rs_frame_create_device(m_ctx, MAX_POINTS, &m_frame), "rs_frame_create_device")) ||
            !rs_ok(rs_frame_assign_device(m_ctx, m_frame, d_pa.get(), d_counts.get(), d_pb.get(), d_counts.get() + 1, d_desc.get(),
                                          &n_frame), "rs_frame_assign_device") || n_frame != (int)n)
            return {};
        *out_frame = m_frame;
    }
    stage_sync();
    return rows;
}

rs_pose_estimator* Session::pose_estimator()
{
    if (!m_pose && !rs_ok(rs_pose_estimator_create(m_ctx, 8192, 1000, &m_pose), "rs_pose_estimator_create")) m_pose = nullptr;
    return m_pose;
}

rs_pnp_estimator* Session::pnp_estimator()
{
    if (!m_pnp && !rs_ok(rs_pnp_estimator_create(m_ctx, 8192, 1000, &m_pnp), "rs_pnp_estimator_create")) m_pnp = nullptr;
    return m_pnp;
}

// ------------------------------------------------------------------------ pose (src/PoseEstimation.cpp)
namespace pose {

namespace {

constexpr int POSE_MAX_POINTS = 8192;

// the matched pixels (prev keypoint of train_index, keypoint of query_index), PoseEstimation.cpp:64-68
void matched_pixels(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                    const std::vector<FeatureMatch>& matches, std::vector<float>& from, std::vector<float>& to)
{
    const size_t n = matches.size();
    from.assign(2 * std::max<size_t>(n, 1), 0.f);
    to.assign(2 * std::max<size_t>(n, 1), 0.f);
    for (size_t k = 0; k < n; k++) {
        const Vec2f a = prev_features.keypoints[matches[k].train_index].pt, b = features.keypoints[matches[k].query_index].pt;
        from[2 * k] = a.x; from[2 * k + 1] = a.y;
        to[2 * k] = b.x; to[2 * k + 1] = b.y;
    }
}

PoseEstimate collect(const std::vector<FeatureMatch>& matches, const std::vector<float>& pose, const std::vector<int32_t>& index,
                     const std::vector<int32_t>& count, const std::vector<int32_t>& status)
{
    PoseEstimate e;
    for (int k = 0; k < 16; k++) e.pose[k] = pose[k];
    for (int32_t k = 0; k < count[0]; k++) e.inlier_matches.push_back(matches[index[k]]);
    e.status = status[0];
    return e;
}

}  // namespace

std::vector<int32_t> known_rotation_pairs(size_t n)
{
    std::vector<int32_t> pairs(400, 0);
    if (n == 0) return pairs;
    std::mt19937 generator(0);
    std::uniform_int_distribution<size_t> pick(0, n - 1);
    for (size_t it = 0; it < 200; it++) {
        const size_t i = pick(generator);
        const size_t j = pick(generator);
        pairs[2 * it] = (int32_t)i;
        pairs[2 * it + 1] = (int32_t)j;
    }
    return pairs;
}

PoseEstimate estimate_pose(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                           const std::vector<FeatureMatch>& matches, const Camera& camera)
{
    const size_t n = matches.size();
    rs_pose_estimator* est = Session::get().pose_estimator();
    if (!est || n > (size_t)POSE_MAX_POINTS) {
        std::printf("estimate_pose: no estimator, or more than %d matches\n", POSE_MAX_POINTS);
        return {};
    }
    std::vector<float> from, to;
    matched_pixels(prev_features, features, matches, from, to);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    StageScope scope;
    DevBuf<float> d_from(from), d_to(to), d_pose(16);
    DevBuf<int32_t> d_count(std::vector<int32_t>{(int32_t)n}), d_index(std::max<size_t>(n, 1)), d_cnt(1), d_status(1);
    DevBuf<uint8_t> d_inlier(std::max<size_t>(n, 1));
    if (!rs_ok(rs_estimate_pose(Session::get().ctx(), est, d_from.get(), nullptr, d_to.get(), d_count.get(), (int)n, K, 1.0, 0.99,
                                1000, 0, d_pose.get(), d_inlier.get(), d_index.get(), d_cnt.get(), d_status.get()),
               "rs_estimate_pose"))
        return {};
    auto pose = d_pose.fetch(16);
    auto index = d_index.fetch(n);
    auto count = d_cnt.fetch(1);
    auto status = d_status.fetch(1);
    stage_sync();
    return collect(matches, pose, index, count, status);
}

PoseEstimate estimate_pose_with_known_rotation(const ExtractedFeatures& prev_features, const ExtractedFeatures& features,
                                               const std::vector<FeatureMatch>& matches, const Camera& camera,
                                               const std::array<float, 9>& rotation)
{
    const size_t n = matches.size();
    rs_pose_estimator* est = Session::get().pose_estimator();
    if (!est || n > (size_t)POSE_MAX_POINTS) {
        std::printf("estimate_pose_with_known_rotation: no estimator, or more than %d matches\n", POSE_MAX_POINTS);
        return {};
    }
    std::vector<float> from, to;
    matched_pixels(prev_features, features, matches, from, to);
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    StageScope scope;
    DevBuf<float> d_from(from), d_to(to), d_pose(16);
    DevBuf<int32_t> d_pairs(known_rotation_pairs(n)), d_index(std::max<size_t>(n, 1)), d_cnt(1), d_status(1);
    DevBuf<uint8_t> d_inlier(std::max<size_t>(n, 1));
    if (!rs_ok(rs_estimate_pose_known_rotation(Session::get().ctx(), est, d_from.get(), nullptr, d_to.get(), (int)n, K,
                                               rotation.data(), d_pairs.get(), 200, 2.0f, d_pose.get(), d_inlier.get(),
                                               d_index.get(), d_cnt.get(), d_status.get()),
               "rs_estimate_pose_known_rotation"))
        return {};
    auto pose = d_pose.fetch(16);
    auto index = d_index.fetch(n);
    auto count = d_cnt.fetch(1);
    auto status = d_status.fetch(1);
    stage_sync();
    return collect(matches, pose, index, count, status);
}

PnpEstimate estimate_pose_pnp(const std::vector<Vec3f>& object_points, const std::vector<Vec2f>& pixels, const Camera& camera,
                              double threshold_px)
{
    const size_t n = std::min(object_points.size(), pixels.size());
    rs_pnp_estimator* est = Session::get().pnp_estimator();
    if (!est || n > (size_t)POSE_MAX_POINTS) {
        std::printf("estimate_pose_pnp: no estimator, or more than %d correspondences\n", POSE_MAX_POINTS);
        return {};
    }
    std::vector<float> obj(3 * std::max<size_t>(n, 1), 0.f), pix(2 * std::max<size_t>(n, 1), 0.f);
    for (size_t k = 0; k < n; k++) {
        obj[3 * k] = object_points[k].x; obj[3 * k + 1] = object_points[k].y; obj[3 * k + 2] = object_points[k].z;
        pix[2 * k] = pixels[k].x; pix[2 * k + 1] = pixels[k].y;
    }
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    StageScope scope;
    DevBuf<float> d_obj(obj), d_pix(pix), d_pose(16);
    DevBuf<int32_t> d_count(std::vector<int32_t>{(int32_t)n}), d_index(std::max<size_t>(n, 1)), d_cnt(1), d_status(1);
    DevBuf<uint8_t> d_inlier(std::max<size_t>(n, 1));
    if (!rs_ok(rs_estimate_pose_pnp(Session::get().ctx(), est, d_obj.get(), nullptr, d_pix.get(), nullptr, d_count.get(), (int)n, K,
                                    threshold_px, 0.99, 200, 0, d_pose.get(), d_inlier.get(), d_index.get(), d_cnt.get(),
                                    d_status.get()),
               "rs_estimate_pose_pnp"))
        return {};
    auto pose = d_pose.fetch(16);
    auto index = d_index.fetch(n);
    auto count = d_cnt.fetch(1);
    auto status = d_status.fetch(1);
    stage_sync();
    PnpEstimate e;
    for (int k = 0; k < 16; k++) e.pose[k] = pose[k];
    for (int32_t k = 0; k < count[0]; k++) e.inliers.push_back((size_t)index[k]);
    e.status = status[0];
    return e;
}

}  // namespace pose

// ------------------------------------------------------------------------ loop retrieval
LoopRetrieval::LoopRetrieval(const std::string& vocabulary_path, size_t max_key_frames, size_t max_total_words, float seconds_per_frame)
    : m_seconds_per_frame(seconds_per_frame)
{
    rs_context* ctx = Session::get().ctx();
    if (!rs_ok(rs_vocabulary_load_text(ctx, vocabulary_path.c_str(), &m_voc), "rs_vocabulary_load_text")) return;
    if (!rs_ok(rs_bow_create(ctx, m_voc, 8192, &m_bow), "rs_bow_create")) return;
    if (hipMalloc(&m_d_score, sizeof(double) * std::max<size_t>(max_key_frames, 1)) != hipSuccess) {
        std::printf("LoopRetrieval: no memory for %zu scores\n", max_key_frames);
        m_d_score = nullptr;
        return;
    }
    rs_ok(rs_bow_database_create(ctx, m_voc, (int)max_key_frames, (int)max_total_words, &m_db), "rs_bow_database_create");
    m_frame_index.reserve(max_key_frames);
}

LoopRetrieval::~LoopRetrieval()
{
    rs_bow_database_destroy(m_db);
    rs_bow_destroy(m_bow);
    rs_vocabulary_destroy(m_voc);
    if (m_d_score) (void)hipFree(m_d_score);
}

bool LoopRetrieval::add_key_frame(const uint8_t* d_desc, const int32_t* d_count, int max_n, size_t frame_index)
{
    if (!valid()) return false;
    rs_context* ctx = Session::get().ctx();
    int32_t entry = -1;
    if (!rs_ok(rs_bow_transform(ctx, m_bow, d_desc, d_count, max_n, nullptr), "rs_bow_transform") ||
        !rs_ok(rs_bow_database_add(ctx, m_db, m_bow, &entry), "rs_bow_database_add"))
        return false;
    m_frame_index.push_back((int64_t)frame_index);
    return true;
}

std::vector<LoopCandidate> LoopRetrieval::query()
{
    std::vector<LoopCandidate> out;
    if (!valid() || m_frame_index.size() < 2) return out;
    rs_context* ctx = Session::get().ctx();
    const int q = (int)m_frame_index.size() - 1;             // the query: the key frame added last, still in m_bow
    if (!rs_ok(rs_bow_database_score(ctx, m_db, m_bow, 0, q, m_d_score), "rs_bow_database_score") ||
        !rs_ok(rs_context_synchronize(ctx), "rs_context_synchronize"))
        return out;
    m_score.resize((size_t)q);
    hip_ok(hipMemcpy(m_score.data(), m_d_score, sizeof(double) * (size_t)q, hipMemcpyDeviceToHost), "scores");
    int32_t entry[3], count = 0, rejected = -1;
    float score[3], rejected_score = 0.0f;
    if (!rs_ok(rs_rank_loop_candidates(m_score.data(), m_frame_index.data(), q, m_frame_index[q], (double)m_seconds_per_frame, 50, 10.0,
                                       0.02f, 1.25f, 3, entry, score, &count, &rejected, &rejected_score),
               "rs_rank_loop_candidates"))
        return out;
    if (count == 0 && rejected >= 0) std::printf("Loop rejected: best kf %d bow %g\n", rejected, (double)rejected_score);   // :262
    for (int32_t r = 0; r < count; r++)
        out.push_back({(size_t)entry[r], score[r], (size_t)(m_frame_index[q] - m_frame_index[entry[r]])});
    return out;
}

// ------------------------------------------------------------------------ loop verification
LoopVerifier::LoopVerifier(int max_points, int max_candidates) : m_max_points(max_points)
{
    if (!rs_ok(rs_loop_verifier_create(Session::get().ctx(), max_points, max_candidates, 200, &m_verifier), "rs_loop_verifier_create")) return;
    m_result.resize((size_t)max_candidates);
    for (auto& l : m_listed) l.resize((size_t)max_candidates * (size_t)max_points);
}

LoopVerifier::~LoopVerifier() { rs_loop_verifier_destroy(m_verifier); }

std::vector<LoopVerification> LoopVerifier::verify(rs_map* map, int query_kf, const std::vector<int32_t>& candidates, const Camera& camera)
{
    std::vector<LoopVerification> out;
    if (!valid() || candidates.empty() || candidates.size() > m_result.size()) return out;
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    // MapMatcher's max_distance 64; PNP_REPROJ_ERROR 4 px, 0.99, 200 iterations (:38, :203-214)
    if (!rs_ok(rs_map_verify_loop(Session::get().ctx(), m_verifier, map, query_kf, candidates.data(), (int)candidates.size(), K,
                                  camera.get_width(), 64, 4.0, 0.99, 200, 0, m_result.data(), m_listed[0].data(), m_listed[1].data(),
                                  m_listed[2].data()),
               "rs_map_verify_loop"))
        return out;
    out.resize(candidates.size());
    for (size_t c = 0; c < candidates.size(); c++) {
        out[c].result = m_result[c];
        const size_t o = c * (size_t)m_max_points, n = (size_t)m_result[c].listed;
        out[c].query_kp.assign(m_listed[0].begin() + (long)o, m_listed[0].begin() + (long)(o + n));
        out[c].point.assign(m_listed[1].begin() + (long)o, m_listed[1].begin() + (long)(o + n));
        out[c].candidate_kp.assign(m_listed[2].begin() + (long)o, m_listed[2].begin() + (long)(o + n));
    }
    return out;
}

// inverse of an affine 4 x 4 (last row 0 0 0 1) in f64 by the cofactors of its 3 x 3 block
static bool affine_inverse(const double* T, double* out)
{
    const double a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], i = T[10];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    if (det == 0.0) return false;
    const double inv[9] = {A / det, -(b * i - c * h) / det, (b * f - c * e) / det,
                           B / det, (a * i - c * g) / det,  -(a * f - c * d) / det,
                           C / det, -(a * h - b * g) / det, (a * e - b * d) / det};
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) out[4 * r + k] = inv[3 * r + k];
        out[4 * r + 3] = -(inv[3 * r] * T[3] + inv[3 * r + 1] * T[7] + inv[3 * r + 2] * T[11]);
    }
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
    return true;
}

int LoopStreak::update(size_t from, const std::vector<LoopCandidate>& ranked, const std::vector<LoopVerification>& verifications,
                       const std::vector<Mat4f>& candidate_poses)
{
    if (ranked.size() != verifications.size() || ranked.size() != candidate_poses.size()) return -1;
    std::vector<int64_t> index, cfrom, cto;
    std::vector<rs_loop_result> results;
    for (size_t i = 0; i < ranked.size(); i++) { index.push_back((int64_t)ranked[i].entry); results.push_back(verifications[i].result); }
    for (const auto& c : m_constraints) { cfrom.push_back((int64_t)c.from); cto.push_back((int64_t)c.to); }
    int32_t chosen = -1, is_new = 0;
    if (rs_loop_update_streak(&m_state, (int64_t)from, index.data(), results.data(), (int)ranked.size(), cfrom.data(), cto.data(),
                              (int)cfrom.size(), &chosen, &is_new) != RS_OK)
        return -1;
    if (!is_new) return chosen;
    const LoopVerification& v = verifications[(size_t)chosen];
    LoopConstraint c;
    c.from = from;
    c.to = ranked[(size_t)chosen].entry;
    double P[16], Q[16], Qi[16];
    for (int k = 0; k < 16; k++) { P[k] = (double)v.result.pose[k]; Q[k] = (double)candidate_poses[(size_t)chosen][(size_t)k]; }
    if (!affine_inverse(Q, Qi)) {                  // a singular candidate pose: no constraint can be formed, the streak starts over
        std::printf("Loop constraint kf %zu -> %zu dropped: the candidate's pose is singular\n", c.from, c.to);
        m_state.length = 0;
        return -1;
    }
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            double s = 0.0;
            for (int j = 0; j < 4; j++) s += P[4 * r + j] * Qi[4 * j + k];
            c.relative[(size_t)(4 * r + k)] = s;                                                   // :437
        }
    for (size_t k = 0; k < v.query_kp.size(); k++) c.inlier_matches.emplace_back(v.query_kp[k], v.point[k]);
    std::printf("Loop constraint kf %zu -> %zu inliers %zu\n", c.from, c.to, c.inlier_matches.size());      // :439-440
    m_constraints.push_back(std::move(c));
    m_new_loop = true;
    return chosen;
}

bool LoopStreak::consume_new_loop()
{
    const bool added = m_new_loop;
    m_new_loop = false;
    return added;
}

// ---------------------------------------------------------------------------------------------- the tail of Tracker::track
bool track_tail(rs_context* ctx, rs_map* map, const rs_frame* prev, rs_frame* next, const int32_t* d_prev_index,
                const int32_t* d_inlier_index, const int32_t* d_inlier_count, int max_n, const Camera& camera, bool optimize,
                TrackTailConstraint* constraint, int last_key_frame, Mat4f& pose, TrackTail* out)
{
    TrackTail t;
    const auto fail = [&](int rc, const char* what) {
        std::printf("%s failed (status %d): %s\n", what, rc, ctx ? rs_last_error(ctx) : "no context");
        if (out) *out = t;
        return false;
    };
    int rc = rs_map_carry_matches(ctx, map, prev, next, d_prev_index, d_inlier_index, d_inlier_count, max_n, MIN_TRACKED_MAP_POINTS, nullptr);   // :83
    if (rc != RS_OK) return fail(rc, "rs_map_carry_matches");
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    if (optimize) {                                                                              // :84, :302-320
        double cam[6];
        rs_pack_pose(pose.data(), cam);
        TrackTailConstraint none;
        TrackTailConstraint& c = constraint ? *constraint : none;
        rc = rs_map_refine_pose(ctx, map, next, cam, K, MIN_TRACKED_MAP_POINTS, c.kind, c.predicted, c.sigma_radians, c.prev_pose,
                                c.prev_velocity, c.prev_bias, &c.delta, c.gravity, c.velocity, nullptr, &t.summary, &t.n_used);
        if (rc != RS_OK) return fail(rc, "rs_map_refine_pose");
        if (t.n_used > 0) {
            std::printf("refine_pose: iterations %d, cost %.6e -> %.6e, termination %d\n", t.summary.iterations, t.summary.initial_cost,
                        t.summary.final_cost, t.summary.termination);
            if (!t.summary.usable) std::printf("Optimization rejected, unusable or non-improving solution\n");
        }
        t.refined = t.n_used > 0 && t.summary.usable != 0;
        if (t.refined) rs_unpack_pose(cam, pose.data());
    }
    rc = rs_map_match_frame(ctx, map, next, pose.data(), K, camera.get_width(), camera.get_height(), last_key_frame, 64, &t.key_frame_matches);   // :85
    if (rc != RS_OK) return fail(rc, "rs_map_match_frame");
    std::printf("Map matches with last frame: %d\n", t.key_frame_matches);
    rc = rs_map_match_frame(ctx, map, next, pose.data(), K, camera.get_width(), camera.get_height(), -1, 64, &t.map_matches);                     // :86
    if (rc != RS_OK) return fail(rc, "rs_map_match_frame");
    std::printf("Number of map matches: %d\n", t.map_matches);
    if (out) *out = t;
    return true;
}

// ---------------------------------------------------------------------------------------------- TrackStore, host and device
void HostTrackStore::carry_forward(const int32_t* prev_index, const int32_t* inlier_index, int n, int max_n, size_t max_points)
{
    std::map<uint64_t, StoredTrack> carried;
    std::unordered_map<size_t, uint64_t> by_keypoint;
    std::unordered_set<size_t> named;
    const size_t lim = std::min((size_t)std::max(max_n, 0), max_points);
    n = std::min(std::max(n, 0), std::max(max_n, 0));
    by_keypoint.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        const int64_t j = inlier_index ? inlier_index[i] : i;
        if (j < 0 || (size_t)j >= lim) continue;
        const int64_t q = prev_index[j];
        if (q < 0) continue;
        const auto existing = m_by_keypoint.find((size_t)q);
        if (existing == m_by_keypoint.end()) continue;
        if (!named.insert((size_t)q).second) continue;           // a later entry naming the same previous keypoint
        if (by_keypoint.count((size_t)j)) continue;              // its current keypoint is taken: the track is dropped
        auto track = m_tracks.find(existing->second);
        track->second.keypoint_index = (size_t)j;
        by_keypoint[(size_t)j] = existing->second;
        carried.emplace(existing->second, std::move(track->second));
    }
    m_tracks = std::move(carried);
    m_by_keypoint = std::move(by_keypoint);
}

void HostTrackStore::extend(const float* keypoints, size_t n, int frame_index, int key_frame, size_t max_sightings)
{
    for (size_t i = 0; i < n; i++) {
        auto existing = m_by_keypoint.find(i);
        if (existing == m_by_keypoint.end()) {
            const uint64_t id = m_next_id++;
            existing = m_by_keypoint.emplace(i, id).first;
            StoredTrack t;
            t.keypoint_index = i;
            m_tracks.emplace(id, std::move(t));
        }
        auto& sightings = m_tracks.at(existing->second).sightings;
        if (sightings.size() < max_sightings) {
            StoredSighting s;
            s.frame_index = frame_index; s.pixel = Vec2f{keypoints[2 * i], keypoints[2 * i + 1]};
            s.key_frame = key_frame < 0 ? -1 : key_frame; s.keypoint_index = (int32_t)i;
            sightings.push_back(s);
        }
    }
}

void HostTrackStore::erase(uint64_t id)
{
    const auto track = m_tracks.find(id);
    if (track == m_tracks.end()) return;
    m_by_keypoint.erase(track->second.keypoint_index);
    m_tracks.erase(track);
}

size_t HostTrackStore::unmapped_tracks(const int32_t* table, size_t n, size_t min_sightings, float min_travel) const
{
    size_t count = 0;
    for (const auto& [id, track] : m_tracks) {
        (void)id;
        if (track.sightings.size() < min_sightings) continue;
        if (track.keypoint_index < n && table[track.keypoint_index] >= 0) continue;
        const float dx = track.sightings.back().pixel.x - track.sightings.front().pixel.x;
        const float dy = track.sightings.back().pixel.y - track.sightings.front().pixel.y;
        const float xx = dx * dx, yy = dy * dy;
        const float travel = std::sqrt(xx + yy);
        if (travel < min_travel) continue;
        count++;
    }
    return count;
}

DeviceTracks::DeviceTracks(rs_context* ctx, int max_points, int max_sightings) : m_ctx(ctx), m_max_points(max_points)
{
    const int rc = rs_track_store_create(ctx, max_points, max_sightings, &m_store);
    if (rc != RS_OK) {
        std::printf("rs_track_store_create failed (status %d): %s\n", rc, ctx ? rs_last_error(ctx) : "no context");
        m_store = nullptr;
        return;
    }
    m_i32.resize(6 * (size_t)max_points + 1 + 8 * (size_t)max_points);      // keypoint, sightings, kf_ptr, track, inconsistent | pairs
    m_f32.resize(5 * (size_t)max_points);                                    // xyz, parallax, required
}

DeviceTracks::~DeviceTracks() { rs_track_store_destroy(m_store); }

static bool tracks_fail(rs_context* ctx, int rc, const char* what)
{
    std::printf("%s failed (status %d): %s\n", what, rc, ctx ? rs_last_error(ctx) : "no context");
    return false;
}

bool DeviceTracks::carry_forward(const int32_t* d_prev_index, const int32_t* d_inlier_index, const int32_t* d_inlier_count, int max_n)
{
    const int rc = rs_track_store_carry(m_ctx, m_store, d_prev_index, d_inlier_index, d_inlier_count, max_n);
    return rc == RS_OK || tracks_fail(m_ctx, rc, "rs_track_store_carry");
}

bool DeviceTracks::needs_key_frame(rs_map* map, const rs_frame* frame, int last_key_frame, int frame_gap, int last_key_frame_matches,
                                   bool* need, int32_t* query)
{
    int32_t q[6];
    int rc = rs_track_store_query(m_ctx, m_store, map, frame, last_key_frame, 3, 20.0f, q);
    if (rc != RS_OK) return tracks_fail(m_ctx, rc, "rs_track_store_query");
    int out = 0;
    if ((rc = rs_needs_key_frame(q, frame_gap, last_key_frame_matches, 20, 200, 50, 0.7f, &out)) != RS_OK) return tracks_fail(m_ctx, rc, "rs_needs_key_frame");
    if (need) *need = out != 0;
    if (query) memcpy(query, q, sizeof q);
    return true;
}

bool DeviceTracks::extend(const rs_frame* frame, int frame_index, int key_frame)
{
    const int rc = rs_track_store_extend(m_ctx, m_store, frame, frame_index, key_frame);
    return rc == RS_OK || tracks_fail(m_ctx, rc, "rs_track_store_extend");
}

bool DeviceTracks::triangulate_tracks(const rs_frame* frame, const float* d_poses, int n_poses, int pose_base, int kf_pose, const Camera& camera,
                                      const float* d_required, DeviceTrackSelection* out, size_t min_new_points)
{
    const size_t T = (size_t)m_max_points;
    rs_track_results& r = m_results;
    r = rs_track_results{};
    r.capacity_tracks = m_max_points; r.capacity_pairs = 4 * m_max_points;
    r.h_keypoint = m_i32.data(); r.h_sightings = r.h_keypoint + T; r.h_kf_ptr = r.h_sightings + T; r.h_track = r.h_kf_ptr + T + 1;
    r.h_inconsistent = r.h_track + T; r.h_kf_pairs = r.h_inconsistent + T;
    r.h_xyz = m_f32.data(); r.h_parallax_cos = r.h_xyz + 3 * T; r.h_required_cos = r.h_parallax_cos + T;
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    const int rc = rs_track_store_triangulate(m_ctx, m_store, nullptr, frame, d_poses, n_poses, pose_base, kf_pose, K, tracks::ANY_PARALLAX_COSINE,
                                              tracks::TRACK_MAX_REPROJECTION_ERROR, tracks::TRACK_MIN_PARALLAX_COSINE,
                                              tracks::ROTATION_PARALLAX_FACTOR, (int)min_new_points, d_required, &r);
    if (rc != RS_OK) return tracks_fail(m_ctx, rc, "rs_track_store_triangulate");
    if (r.n_pairs > r.capacity_pairs) { std::printf("triangulate_tracks: %d key-frame sightings, room for %d\n", r.n_pairs, r.capacity_pairs); return false; }
    if (!out) return true;
    *out = DeviceTrackSelection{};
    out->out_of_range = (size_t)r.out_of_range; out->tracks = (size_t)r.n_tracks;
    out->selection.topped_up = (size_t)r.counts[1];
    for (int a = 0; a < r.counts[0]; a++) {
        tracks::Candidate c;
        c.track = (size_t)r.h_track[a];
        c.position = Vec3f{r.h_xyz[3 * a], r.h_xyz[3 * a + 1], r.h_xyz[3 * a + 2]};
        c.keypoint_index = (size_t)r.h_keypoint[a];
        c.parallax_cosine = r.h_parallax_cos[a]; c.required_cosine = r.h_required_cos[a];
        out->selection.accepted.push_back(c);
        out->sightings.push_back((size_t)r.h_sightings[a]);
        std::vector<KeyFrameSighting> ks;
        for (int i = r.h_kf_ptr[a]; i < r.h_kf_ptr[a + 1]; i++) ks.push_back(KeyFrameSighting{r.h_kf_pairs[2 * i], r.h_kf_pairs[2 * i + 1]});
        out->key_frame_sightings.push_back(std::move(ks));
    }
    for (int i = 0; i < r.counts[2]; i++) out->selection.inconsistent.push_back((size_t)r.h_inconsistent[i]);
    return true;
}

bool DeviceTracks::erase_inconsistent()
{
    const int rc = rs_track_store_erase_inconsistent(m_ctx, m_store);
    return rc == RS_OK || tracks_fail(m_ctx, rc, "rs_track_store_erase_inconsistent");
}

// ---------------------------------------------------------------------------------------------- Mapper::insert
bool insert_key_frame(rs_context* ctx, rs_map* map, DeviceTracks* tracks, const rs_frame* frame, const Mat4f& pose,
                      const KeyFrameWindow& window, const KeyFrameTrajectory& trajectory, const Camera& camera, bool bundle_adjust,
                      bool cull_points, KeyFrameInsert* out)
{
    KeyFrameInsert r;
    const auto done = [&](bool ok) { if (out) *out = std::move(r); return ok; };
    const auto fail = [&](int rc, const char* what) {
        std::printf("%s failed (status %d): %s\n", what, rc, ctx ? rs_last_error(ctx) : "no context");
        return done(false);
    };
    if (window.optimize.size() != window.key_frames.size() || window.poses.size() != window.key_frames.size()) return fail(RS_ERR_INVALID, "insert_key_frame: window");
    int rc = rs_map_insert_keyframe(ctx, map, frame, pose.data(), &r.key_frame, &r.adopted);                  // :155-159
    if (rc != RS_OK) return fail(rc, "rs_map_insert_keyframe");
    if (tracks) {                                                                                             // :161-163
        if (!tracks->triangulate_tracks(frame, trajectory.d_poses, trajectory.n_poses, trajectory.pose_base, trajectory.kf_pose, camera,
                                        trajectory.d_required, &r.selection))
            return done(false);
        r.created.assign((size_t)std::max(tracks->results().counts[0], 0), -1);
        rc = rs_map_add_track_points(map, r.key_frame, &tracks->results(), window.key_frames.data(), (int)window.key_frames.size(),
                                     r.created.data());                                                       // :306-331
        if (rc != RS_OK) return fail(rc, "rs_map_add_track_points");
        if (!tracks->erase_inconsistent()) return done(false);                                                // :333-335
        std::printf("Triangulated from tracks: %zu of %zu tracks, inconsistent %zu, topped up %zu\n", r.created.size(), r.selection.tracks,
                    r.selection.selection.inconsistent.size(), r.selection.selection.topped_up);
    }
    r.window = window.key_frames;
    r.window.push_back(r.key_frame);
    std::vector<uint8_t> free_flags = window.optimize;
    free_flags.push_back(1);
    const int C = (int)r.window.size();
    const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
    int counts[4] = {0, 0, 0, 0};
    if ((rc = rs_map_counts(map, counts)) != RS_OK) return fail(rc, "rs_map_counts");
    const int cap = counts[0];
    if (bundle_adjust) {                                                                                      // :165-167, :364-394
        // the anchors: the optimised frames and their poses before the adjustment (:369-375)
        std::vector<int32_t> anchors;
        std::vector<float> before;
        for (int c = 0; c < C; c++) {
            if (!free_flags[(size_t)c]) continue;
            const Mat4f& T = c + 1 < C ? window.poses[(size_t)c] : pose;
            anchors.push_back(r.window[(size_t)c]);
            before.insert(before.end(), T.begin(), T.end());
        }
        r.poses.assign(16 * (size_t)C, 0.0f);
        r.adjusted.assign((size_t)cap, 0);
        r.adjusted_xyz.assign(3 * (size_t)cap, 0.0f);
        int n = 0;
        rc = rs_map_bundle_adjust(ctx, map, r.window.data(), free_flags.data(), C, K, nullptr, &r.summary, r.poses.data(), r.adjusted.data(),
                                  r.adjusted_xyz.data(), cap, &n);
        if (rc != RS_OK) return fail(rc, "rs_map_bundle_adjust");
        r.adjusted.resize((size_t)std::min(n, cap));
        r.adjusted_xyz.resize(3 * r.adjusted.size());
        r.reanchored.assign((size_t)cap, 0);
        r.reanchored_xyz.assign(3 * (size_t)cap, 0.0f);
        rc = rs_map_reanchor(ctx, map, anchors.data(), before.data(), (int)anchors.size(), r.reanchored.data(), r.reanchored_xyz.data(), cap, &n);
        if (rc != RS_OK) return fail(rc, "rs_map_reanchor");
        r.reanchored.resize((size_t)std::min(n, cap));
        r.reanchored_xyz.resize(3 * r.reanchored.size());
    }
    if (cull_points) {                                                                                        // :168-170, :396-431
        r.culled.assign((size_t)cap, 0);
        r.culled_xyz.assign(3 * (size_t)cap, 0.0f);
        int n = 0;
        rc = rs_map_cull_points(ctx, map, r.window.data(), C, K, tracks::MAX_POINT_REPROJECTION_ERROR, 1, r.culled.data(), r.culled_xyz.data(),
                                cap, &n, &r.local_points);
        if (rc != RS_OK) return fail(rc, "rs_map_cull_points");
        r.culled.resize((size_t)n);
        r.culled_xyz.resize(3 * r.culled.size());
        std::printf("Number of points to remove: %d\n", n);
    }
    return done(true);
}

bool close_loop(rs_context* ctx, rs_map* map, const std::vector<LoopConstraint>& loops, const std::vector<int32_t>& window,
                const Camera& camera, int max_descriptor_distance, bool four_dof, const double gravity[3], bool bundle_adjust, bool check,
                LoopClosure* out)
{
    LoopClosure r;
    const auto done = [&](bool ok) { if (out) *out = std::move(r); return ok; };
    const auto fail = [&](int rc, const char* what) {
        std::printf("%s failed (status %d): %s\n", what, rc, ctx ? rs_last_error(ctx) : "no context");
        return done(false);
    };
    if (loops.empty() || window.empty()) return fail(RS_ERR_INVALID, "close_loop: no constraint or no window");
    int counts[4] = {0, 0, 0, 0};
    int rc = rs_map_counts(map, counts);
    if (rc != RS_OK) return fail(rc, "rs_map_counts");
    const int cap = counts[0], n_kf = counts[3];
    std::vector<rs_pose_graph_edge> edges(loops.size());
    for (size_t i = 0; i < loops.size(); i++) {
        edges[i].from = (int32_t)loops[i].from;
        edges[i].to = (int32_t)loops[i].to;
        for (int k = 0; k < 16; k++) edges[i].relative[k] = loops[i].relative[(size_t)k];
    }
    const double zero[3] = {0.0, 0.0, 0.0};
    r.graph_poses.assign(16 * (size_t)std::max(n_kf, 1), 0.0f);
    rc = rs_map_pose_graph(ctx, map, edges.data(), (int)edges.size(), four_dof ? 1 : 0, gravity ? gravity : zero, nullptr, r.graph_poses.data(),
                           nullptr, &r.graph);                                                                 // src/Slam.cpp:262-268
    if (rc != RS_OK) return fail(rc, "rs_map_pose_graph");
    r.closed = r.graph.usable != 0;
    if (!r.closed) return done(true);
    const LoopConstraint& loop = loops.back();
    const int query = (int)loop.from, C = (int)window.size();
    if ((int)loop.to < n_kf) {                                                                                 // :275-279
        std::vector<int32_t> ikp, ipt;
        for (const auto& m : loop.inlier_matches) { ikp.push_back(m.first); ipt.push_back(m.second); }
        rs_fuse_options opt{};
        opt.intrinsics[0] = camera.fx(); opt.intrinsics[1] = camera.fy(); opt.intrinsics[2] = camera.cx(); opt.intrinsics[3] = camera.cy();
        opt.width = camera.get_width(); opt.height = camera.get_height();
        opt.max_distance = max_descriptor_distance; opt.min_shared = 15; opt.max_covisible = 20; opt.check = check ? 1 : 0;
        r.sources.assign((size_t)std::max(cap, 1), -1);
        r.removed.assign((size_t)std::max(cap, 1), -1);
        opt.h_sources = r.sources.data(); opt.capacity_sources = cap;
        opt.h_removed = r.removed.data(); opt.capacity_removed = cap;
        size_t room = ikp.size();
        for (const int32_t kf : window) {
            int n = 0;
            if (rs_map_get_keyframe_matches(map, kf, nullptr, 0, &n) == RS_OK) room += (size_t)n;
        }
        r.section_ptr.assign((size_t)C + 2, 0);
        r.journal_kp.assign(std::max<size_t>(room, 1), 0);
        r.journal_point = r.journal_kp;
        r.journal_outcome = r.journal_kp;
        int n_entries = 0;
        rc = rs_map_fuse_loop(ctx, map, query, (int)loop.to, ikp.data(), ipt.data(), (int)ikp.size(), window.data(), C, &opt, &r.fuse,
                              r.section_ptr.data(), r.journal_kp.data(), r.journal_point.data(), r.journal_outcome.data(), (int)room, &n_entries);
        if (rc != RS_OK) return fail(rc, "rs_map_fuse_loop");
        r.sources.resize((size_t)std::min(r.fuse.n_sources, cap));
        r.removed.resize((size_t)std::min(r.fuse.n_removed, cap));
        r.journal_kp.resize((size_t)n_entries); r.journal_point.resize((size_t)n_entries); r.journal_outcome.resize((size_t)n_entries);
        std::printf("Fused loop: %d old frames, %d sources, %d fused, %d associated\n", r.fuse.n_old_frames, r.fuse.n_sources,
                    r.fuse.outcomes[RS_FUSE_FUSED], r.fuse.outcomes[RS_FUSE_ASSOCIATED]);
    }
    if (bundle_adjust) {                                                                                       // :280-282, Mapper.cpp:364-394
        const float K[4] = {camera.fx(), camera.fy(), camera.cx(), camera.cy()};
        std::vector<uint8_t> free_flags((size_t)C, 1);
        free_flags[0] = 0;                                                  // fix_oldest
        std::vector<int32_t> anchors;
        std::vector<float> before;
        for (int c = 1; c < C; c++) {
            if (window[(size_t)c] < 0 || window[(size_t)c] >= n_kf) return fail(RS_ERR_INVALID, "close_loop: window");
            anchors.push_back(window[(size_t)c]);
            before.insert(before.end(), r.graph_poses.begin() + 16 * (long)window[(size_t)c], r.graph_poses.begin() + 16 * (long)window[(size_t)c] + 16);
        }
        r.poses.assign(16 * (size_t)C, 0.0f);
        r.adjusted.assign((size_t)std::max(cap, 1), 0);
        r.adjusted_xyz.assign(3 * (size_t)std::max(cap, 1), 0.0f);
        int n = 0;
        rc = rs_map_bundle_adjust(ctx, map, window.data(), free_flags.data(), C, K, nullptr, &r.adjust, r.poses.data(), r.adjusted.data(),
                                  r.adjusted_xyz.data(), cap, &n);
        if (rc != RS_OK) return fail(rc, "rs_map_bundle_adjust");
        r.adjusted.resize((size_t)std::min(n, cap));
        r.adjusted_xyz.resize(3 * r.adjusted.size());
        r.reanchored.assign((size_t)std::max(cap, 1), 0);
        r.reanchored_xyz.assign(3 * (size_t)std::max(cap, 1), 0.0f);
        rc = rs_map_reanchor(ctx, map, anchors.data(), before.data(), (int)anchors.size(), r.reanchored.data(), r.reanchored_xyz.data(), cap, &n);
        if (rc != RS_OK) return fail(rc, "rs_map_reanchor");
        r.reanchored.resize((size_t)std::min(n, cap));
        r.reanchored_xyz.resize(3 * r.reanchored.size());
    }
    return done(true);
}

}  // namespace slam
