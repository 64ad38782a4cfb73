// rs_marshal.h — the pointer graph -> SoA flattening of the drop-in boundary, in ONE place.
//
// The drop-in translation units of this directory (the reference's own types: Eigen, OpenCV) and the host mirror
// (racing-slam_amd/host/slam_host.cpp: plain types; the copy that is compiled, run, tested and timed in this repository)
// instantiate the same templates, each with an `Access` that says how to read its host objects.  A flatten function fills a
// plain struct of std::vectors and does nothing else: no staging, no C-ABI call beyond rs_pack_pose.  Only the standard
// library and rsgpu.h are needed (tests/host_cpp/test_marshal.cpp instantiates the header with a third set of structs).
//
// Access: a struct of small static (or inline) functions, nothing virtual.
//   using Point = ...;                                     the map point type
//   position(point, float[3])                              MapPoint::position()
//   pose_row_major(frame, float[16])                       Frame::pose(), row-major world -> camera
//   center(key_frame, float[3])                            Frame::camera_center()
//   keypoint(frame, i, float[2])                           Frame::keypoint(i).pt
//   descriptor_rows(frame, const uint8_t*&, size_t& n)     the frame's n x RS_DESC_BYTES descriptor rows; false when its
//                                                          descriptors have another layout (flatten_match then refuses)
//   n_matches(frame)                                       Frame::num_map_matches() (sizes the tables, nothing else)
//   for_each_match(frame, fn(point&, keypoint_index))      Frame::map_matches(): ascending keypoint index
//   for_each_observation(point, fn(key_frame*, keypoint_index))   MapPoint::observations(), in iteration order
//   n_observations(point)
//   observations_address(point)                            where that list starts, for a prefetch (may be null)
//   is_matched(frame, point), is_observed_by(point, key_frame*)
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if __has_include("rsgpu.h")
#include "rsgpu.h"
#else
#include "../../include/rsgpu.h"
#endif

namespace rs_marshal {

// Pointer -> dense index, for flattening the reference's pointer graph (MapPoint has no id: src/MapPoint.h:12-39).  Open
// addressing over a power-of-two table of {key, value, generation} entries (one cache line per probe), multiplicative hash
// of the address; the table is kept between calls and "cleared" by bumping the generation — std::unordered_map (a node per
// entry, cleared and rebuilt per call) spent 50 - 100 ns per operation and build_local_window + bundle_adjust make ~10^5 of
// them per key frame; allocating and zeroing a fresh 0.8 MB table per call cost another 0.2 ms.
// The tables' storage is thread_local, one for points and one for frames / key frames: the flatten functions are
// re-entrant across threads, and on one thread at most one PtrIndex per Table is alive at a time.
class PtrIndex {
  public:
    enum Table { POINTS, FRAMES };
    // a table for about `expected` distinct keys (it grows by itself beyond that)
    PtrIndex(Table which, size_t expected) : m_store(storage(which))
    {
        size_t cap = 64;
        while (cap < 2 * expected + 2) cap <<= 1;
        Header* h = header();
        if (!h || h->cap < cap) {
            m_store.assign(sizeof(Header) + cap * sizeof(Entry), 0);
            h = header();
            h->cap = cap; h->gen = 0;
        }
        if (++h->gen == 0) {                                   // generation wrapped: really clear
            std::memset(entries(), 0, h->cap * sizeof(Entry));
            h->gen = 1;
        }
        m_gen = h->gen; m_mask = h->cap - 1; m_e = entries(); m_used = 0;
    }
    PtrIndex(const PtrIndex&) = delete;
    PtrIndex& operator=(const PtrIndex&) = delete;
    // index of p, inserting it with value `fresh` if absent; *inserted says which
    int find_or_insert(const void* p, int fresh, bool* inserted)
    {
        size_t h = slot(p);
        while (m_e[h].gen == m_gen && m_e[h].key != p) h = (h + 1) & m_mask;
        if (m_e[h].gen == m_gen) { *inserted = false; return m_e[h].val; }
        m_e[h].key = p; m_e[h].val = fresh; m_e[h].gen = m_gen; *inserted = true;
        if (2 * ++m_used > m_mask) grow();
        return fresh;
    }
    int find(const void* p) const
    {
        size_t h = slot(p);
        while (m_e[h].gen == m_gen && m_e[h].key != p) h = (h + 1) & m_mask;
        return m_e[h].gen == m_gen ? m_e[h].val : -1;
    }

  private:
    struct Entry { const void* key; int val; unsigned gen; };
    struct Header { size_t cap; unsigned gen; unsigned pad; };
    static std::vector<char>& storage(Table which)
    {
        thread_local std::vector<char> store[2];
        return store[which];
    }
    Header* header() { return m_store.size() >= sizeof(Header) ? reinterpret_cast<Header*>(m_store.data()) : nullptr; }
    Entry* entries() { return reinterpret_cast<Entry*>(m_store.data() + sizeof(Header)); }
    size_t slot(const void* p) const { return (size_t)(((uintptr_t)p >> 4) * 0x9E3779B97F4A7C15ull >> 20) & m_mask; }
    void grow()
    {
        std::vector<Entry> live;
        for (size_t i = 0; i <= m_mask; i++)
            if (m_e[i].gen == m_gen) live.push_back(m_e[i]);
        const size_t cap = 2 * (m_mask + 1);
        m_store.assign(sizeof(Header) + cap * sizeof(Entry), 0);
        Header* h = header();
        h->cap = cap; h->gen = 1;
        m_gen = 1; m_mask = cap - 1; m_e = entries();
        for (const Entry& e : live) {
            size_t q = slot(e.key);
            while (m_e[q].gen == m_gen) q = (q + 1) & m_mask;
            m_e[q] = Entry{e.key, e.val, m_gen};
        }
    }
    std::vector<char>& m_store;
    Entry* m_e = nullptr;
    size_t m_mask = 0, m_used = 0;
    unsigned m_gen = 0;
};

constexpr size_t MIN_OBSERVATIONS_TO_OPTIMIZE = 2;             // src/Optimization.cpp:98

// MapMatcher::match (src/MapMatcher.cpp:45-98, 117-127, 165-175) -> rs_map_view: positions, eligibility (the pointer-set
// tests of :53, :121-123, :169), observation CSR of the eligible points, key-frame table (ids in first-seen order) and
// descriptor pool (each key frame's rows once).  A null point is ineligible and keeps a zero position.
// F32 (NORM_L2, rs_reproj_match_l2): the pool is pool_f32, rows of `dim` floats read through
// Access::descriptor_rows_f32(frame, const float*&, size_t& n, size_t dim) — false when the frame's rows are not n x dim f32.
struct MatchArrays {
    std::vector<float> pos, centers, pool_f32;
    std::vector<uint8_t> eligible, pool;
    std::vector<int32_t> obs_ptr, obs_kf, obs_desc;
    bool refused = false;                                      // a key frame's descriptor_rows said no: the arrays are incomplete
};
template <bool F32 = false, class Frame, class Point, class KeyFrame, class Access>
MatchArrays flatten_match(const Frame& frame, const std::vector<Point*>& points, KeyFrame* required_observer, const Access& A,
                          size_t dim = 0)
{
    const size_t P = points.size();
    MatchArrays m;
    m.pos.assign(3 * P, 0.0f); m.eligible.assign(P, 0); m.obs_ptr.assign(P + 1, 0);
    std::vector<int32_t> pool_off;
    PtrIndex kf_id(PtrIndex::FRAMES, 64);
    for (size_t p = 0; p < P && !m.refused; p++) {
        const Point* mp = points[p];
        bool ok = mp != nullptr && !A.is_matched(frame, *mp);
        if (ok && required_observer && !A.is_observed_by(*mp, required_observer)) ok = false;
        m.eligible[p] = ok ? 1 : 0;
        if (mp) A.position(*mp, &m.pos[3 * p]);
        if (ok)
            A.for_each_observation(*mp, [&](auto* kf, size_t keypoint_index) {
                if (m.refused) return;
                bool fresh = false;
                const int id = kf_id.find_or_insert(kf, (int)pool_off.size(), &fresh);
                if (fresh) {
                    size_t n_rows = 0;
                    if constexpr (F32) {
                        const float* rows = nullptr;
                        if (!A.descriptor_rows_f32(*kf, rows, n_rows, dim)) { m.refused = true; return; }
                        pool_off.push_back((int32_t)(m.pool_f32.size() / dim));
                        m.pool_f32.insert(m.pool_f32.end(), rows, rows + n_rows * dim);
                    } else {
                        const uint8_t* rows = nullptr;
                        if (!A.descriptor_rows(*kf, rows, n_rows)) { m.refused = true; return; }
                        pool_off.push_back((int32_t)(m.pool.size() / RS_DESC_BYTES));
                        m.pool.insert(m.pool.end(), rows, rows + n_rows * RS_DESC_BYTES);
                    }
                    float c[3];
                    A.center(*kf, c);
                    m.centers.insert(m.centers.end(), c, c + 3);
                }
                m.obs_kf.push_back(id);
                m.obs_desc.push_back(pool_off[(size_t)id] + (int32_t)keypoint_index);
            });
        m.obs_ptr[p + 1] = (int32_t)m.obs_kf.size();
    }
    return m;
}

// optimization::refine_pose's gather (src/Optimization.cpp:194-229): the frame's matches with >= 2 observations.
struct RefineArrays {
    std::vector<double> pts;
    std::vector<float> uv;
};
template <class Frame, class Access>
RefineArrays flatten_refine(const Frame& frame, const Access& A)
{
    RefineArrays r;
    A.for_each_match(frame, [&](auto& point, size_t keypoint_index) {
        if (A.n_observations(point) < MIN_OBSERVATIONS_TO_OPTIMIZE) return;
        float x[3], px[2];
        A.position(point, x);
        A.keypoint(frame, keypoint_index, px);
        r.pts.insert(r.pts.end(), {(double)x[0], (double)x[1], (double)x[2]});
        r.uv.insert(r.uv.end(), px, px + 2);
    });
    return r;
}

// optimization::bundle_adjust (src/Optimization.cpp:269-315).  `frames` holds {bool optimize; Frame* frame;}.
// Free points: matched by an optimised frame, >= 2 observations (:287-302), in first-seen order over the optimised frames
// in list order.  Residual blocks: every listed frame (free or fixed) x its matched free points (:304-315), CSR by point,
// frames in list order within a point.
template <class Point>
struct BaArrays {
    std::vector<double> cams, pts;
    std::vector<uint8_t> cam_free;
    std::vector<Point*> free_pts;
    std::vector<int32_t> obs_ptr, obs_cam;
    std::vector<float> obs_uv;
};
template <class Config, class Access>
BaArrays<typename Access::Point> flatten_ba(const std::vector<Config>& frames, const Access& A)
{
    const size_t C = frames.size();
    BaArrays<typename Access::Point> b;
    b.cams.resize(6 * C); b.cam_free.resize(C);
    size_t n_matches = 0;
    for (size_t c = 0; c < C; c++) {
        float T[16];
        A.pose_row_major(*frames[c].frame, T);
        rs_pack_pose(T, &b.cams[6 * c]);
        b.cam_free[c] = frames[c].optimize ? 1 : 0;
        n_matches += A.n_matches(*frames[c].frame);
    }
    PtrIndex pid(PtrIndex::POINTS, n_matches / 2 + 16);
    for (size_t c = 0; c < C; c++) {
        if (!frames[c].optimize) continue;
        A.for_each_match(*frames[c].frame, [&](auto& point, size_t) {
            if (A.n_observations(point) < MIN_OBSERVATIONS_TO_OPTIMIZE) return;
            bool fresh = false;
            pid.find_or_insert(&point, (int)b.free_pts.size(), &fresh);
            if (fresh) b.free_pts.push_back(&point);
        });
    }
    const size_t P = b.free_pts.size();
    // one pass resolves the matches to point ids, a count / prefix / fill builds the CSR
    struct Hit { int point, cam; float uv[2]; };
    std::vector<Hit> hits;
    hits.reserve(n_matches);
    b.obs_ptr.assign(P + 1, 0);
    for (size_t c = 0; c < C; c++)
        A.for_each_match(*frames[c].frame, [&](auto& point, size_t keypoint_index) {
            const int id = pid.find(&point);
            if (id < 0) return;
            Hit h{id, (int)c, {0.0f, 0.0f}};
            A.keypoint(*frames[c].frame, keypoint_index, h.uv);
            hits.push_back(h);
            b.obs_ptr[(size_t)id + 1]++;
        });
    for (size_t p = 0; p < P; p++) b.obs_ptr[p + 1] += b.obs_ptr[p];
    std::vector<int32_t> fill(b.obs_ptr.begin(), b.obs_ptr.end() - 1);
    b.obs_cam.resize(hits.size()); b.obs_uv.resize(2 * hits.size());
    for (const Hit& h : hits) {                                  // (hits are in frame order: so is every point's slice)
        const size_t o = (size_t)fill[(size_t)h.point]++;
        b.obs_cam[o] = h.cam; b.obs_uv[2 * o] = h.uv[0]; b.obs_uv[2 * o + 1] = h.uv[1];
    }
    b.pts.resize(3 * P);
    for (size_t p = 0; p < P; p++) {
        float x[3];
        A.position(*b.free_pts[p], x);
        for (int k = 0; k < 3; k++) b.pts[3 * p + k] = (double)x[k];
    }
    return b;
}

// optimization::build_local_window (src/LocalWindow.cpp:10-52) -> rs_build_local_window: slot i = key_frames[i], slot n =
// new_frame unless it is one of the key frames (new_index >= 0, empty slot n); frame -> its points (ids in first-seen
// order) and point -> its observing slots (observers outside the list are skipped).
struct WindowArrays {
    int new_index = -1;
    std::vector<int32_t> frame_ptr, frame_pt, pt_ptr, pt_obs;
};
template <class KeyFramePtr, class Frame, class Access>
WindowArrays flatten_local_window(const std::vector<KeyFramePtr>& key_frames, const Frame& new_frame, const Access& A)
{
    using Point = typename Access::Point;
    const int n = (int)key_frames.size();
    WindowArrays w;
    PtrIndex fid(PtrIndex::FRAMES, (size_t)n);
    size_t n_matches = A.n_matches(new_frame);
    for (int i = 0; i < n; i++) {
        const Frame* f = static_cast<const Frame*>(&*key_frames[(size_t)i]);
        bool fresh;
        fid.find_or_insert(f, i, &fresh);
        if (f == &new_frame) w.new_index = i;
        n_matches += A.n_matches(*f);
    }
    PtrIndex pid(PtrIndex::POINTS, n_matches / 2 + 16);
    std::vector<const Point*> pts;
    w.frame_ptr.assign((size_t)n + 2, 0);
    w.frame_pt.reserve(n_matches);
    auto add_frame = [&](const Frame& f, int slot) {
        A.for_each_match(f, [&](const Point& point, size_t) {
            bool fresh = false;
            const int id = pid.find_or_insert(&point, (int)pts.size(), &fresh);
            if (fresh) pts.push_back(&point);
            w.frame_pt.push_back(id);
        });
        w.frame_ptr[(size_t)slot + 1] = (int32_t)w.frame_pt.size();
    };
    for (int i = 0; i < n; i++) add_frame(*key_frames[(size_t)i], i);
    if (w.new_index < 0) add_frame(new_frame, n); else w.frame_ptr[(size_t)n + 1] = w.frame_ptr[(size_t)n];
    w.pt_ptr.assign(pts.size() + 1, 0);
    w.pt_obs.reserve(w.frame_pt.size());
    for (size_t p = 0; p < pts.size(); p++) {
        if (p + 8 < pts.size()) __builtin_prefetch(pts[p + 8]);                   // (the points are scattered heap objects)
        if (p + 4 < pts.size()) __builtin_prefetch(A.observations_address(*pts[p + 4]));
        A.for_each_observation(*pts[p], [&](auto* kf, size_t) {
            const int f = fid.find(static_cast<const Frame*>(kf));
            if (f >= 0) w.pt_obs.push_back(f);
        });
        w.pt_ptr[p + 1] = (int32_t)w.pt_obs.size();
    }
    return w;
}

// Mapper::cull_points' projection loop (src/Mapper.cpp:410-419) -> rs_point_errors: every point's observations with the
// observing key frame's pose row; pose rows in first-seen order.
struct PointErrorArrays {
    std::vector<float> pos, uv, poses;
    std::vector<int32_t> obs_ptr, obs_pose;
    int n_poses = 0;
};
template <class Point, class Access>
PointErrorArrays flatten_point_errors(const std::vector<Point*>& points, const Access& A)
{
    const size_t P = points.size();
    PointErrorArrays e;
    e.pos.resize(3 * P); e.obs_ptr.assign(P + 1, 0);
    PtrIndex pose_row(PtrIndex::FRAMES, 64);
    for (size_t p = 0; p < P; p++) {
        A.position(*points[p], &e.pos[3 * p]);
        A.for_each_observation(*points[p], [&](auto* kf, size_t keypoint_index) {
            bool fresh = false;
            const int row = pose_row.find_or_insert(kf, e.n_poses, &fresh);
            if (fresh) {
                float T[16];
                A.pose_row_major(*kf, T);
                e.poses.insert(e.poses.end(), T, T + 16);
                e.n_poses++;
            }
            e.obs_pose.push_back(row);
            float px[2];
            A.keypoint(*kf, keypoint_index, px);
            e.uv.insert(e.uv.end(), px, px + 2);
        });
        e.obs_ptr[p + 1] = (int32_t)e.obs_pose.size();
    }
    return e;
}

}  // namespace rs_marshal
