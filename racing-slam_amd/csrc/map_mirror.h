// map_mirror.h — the host mirror of rs_map and its edits: plain C++ with no HIP in it, so that the index arithmetic of the
// edits can also be built and run on its own (tests/host_cpp/asan_keyframe.cpp, under the address sanitizer).  map.hip's
// rs_map derives from MapMirror and adds the device image; every mirror_* function below is what the public call of the
// same name does after its argument checks.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/rsgpu.h"

struct MapObs { int32_t kf, kp; };

struct MapKeyFrame {
    int n = 0;
    int pool_row = 0;                  // first row of its descriptors in the device pool
    float pose[16];
    std::vector<int32_t> kp_point;     // [n] point slot matched by keypoint i or -1 (Frame::map_matches)
};

struct MapMirror {
    std::vector<float> pos;                         // [P][3]
    std::vector<uint8_t> alive;                     // [P]
    std::vector<std::vector<MapObs>> obs;           // [P]
    std::vector<MapKeyFrame> kfs;
    int n_alive = 0;
    bool dirty_topology = true, dirty_positions = true, dirty_centres = true;
    bool dirty_kp_point = true;
    std::vector<uint8_t> consistent;                // [P] MapPoint::track_consistent
    bool dirty_consistent = true;
};

static inline bool mirror_point_ok(const MapMirror* m, int p) { return p >= 0 && p < (int)m->alive.size() && m->alive[(size_t)p]; }
static inline bool mirror_kf_ok(const MapMirror* m, int kf) { return kf >= 0 && kf < (int)m->kfs.size(); }

static inline int mirror_add_point(MapMirror* m, const float xyz[3])
{
    m->pos.insert(m->pos.end(), xyz, xyz + 3);
    m->alive.push_back(1);
    m->consistent.push_back(0);
    m->obs.emplace_back();
    m->n_alive++;
    m->dirty_topology = m->dirty_positions = m->dirty_consistent = true;      // (the device flag of the new slot is not yet written)
    return (int)m->alive.size() - 1;
}

static inline int mirror_remove_observation(MapMirror* m, int point, int kf)
{
    if (!mirror_point_ok(m, point) || !mirror_kf_ok(m, kf)) return RS_ERR_INVALID;
    auto& v = m->obs[(size_t)point];
    for (size_t i = 0; i < v.size(); i++)
        if (v[i].kf == kf) {
            auto& tab = m->kfs[(size_t)kf].kp_point;
            if (tab[(size_t)v[i].kp] == point) tab[(size_t)v[i].kp] = -1;
            v.erase(v.begin() + (long)i);
            m->dirty_topology = m->dirty_kp_point = true;
            return RS_OK;
        }
    return RS_OK;       // MapPoint::remove_observation of an absent key frame is a no-op (src/Map.cpp:117-124)
}

static inline bool mirror_observed_by(const MapMirror* m, int point, int kf)
{
    for (const auto& o : m->obs[(size_t)point])
        if (o.kf == kf) return true;
    return false;
}

// Map::associate (src/Map.cpp:95-113): the key frame's keypoint and the point end up matched to each other; whatever
// either was matched to before (in that key frame) is disassociated first.
static inline int mirror_add_observation(MapMirror* m, int point, int kf, int keypoint)
{
    if (!mirror_point_ok(m, point) || !mirror_kf_ok(m, kf)) return RS_ERR_INVALID;
    MapKeyFrame& k = m->kfs[(size_t)kf];
    if (keypoint < 0 || keypoint >= k.n) return RS_ERR_INVALID;
    const int existing = k.kp_point[(size_t)keypoint];
    auto& v = m->obs[(size_t)point];
    const bool seen = mirror_observed_by(m, point, kf);
    if (existing == point && seen) return RS_OK;                          // :97-100
    if (existing >= 0 && existing != point) mirror_remove_observation(m, existing, kf);     // :101-106
    if (seen) mirror_remove_observation(m, point, kf);                    // :107-109
    v.push_back({kf, keypoint});
    k.kp_point[(size_t)keypoint] = point;
    m->dirty_topology = m->dirty_kp_point = true;
    return RS_OK;
}

static inline int mirror_remove_point(MapMirror* m, int point)
{
    if (!mirror_point_ok(m, point)) return RS_ERR_INVALID;
    for (const auto& o : m->obs[(size_t)point]) {                         // Frame::remove_map_match for every observer
        auto& tab = m->kfs[(size_t)o.kf].kp_point;
        if (tab[(size_t)o.kp] == point) tab[(size_t)o.kp] = -1;
    }
    m->obs[(size_t)point].clear();
    m->obs[(size_t)point].shrink_to_fit();
    m->alive[(size_t)point] = 0;
    m->n_alive--;
    m->dirty_topology = m->dirty_kp_point = true;
    return RS_OK;
}

// MapPoint::set_track_consistent: the flag only ever goes up
static inline int mirror_set_track_consistent(MapMirror* m, int point)
{
    if (!mirror_point_ok(m, point)) return RS_ERR_INVALID;
    if (!m->consistent[(size_t)point]) { m->consistent[(size_t)point] = 1; m->dirty_consistent = true; }
    return RS_OK;
}

// Mapper::insert's adoption loop (src/Mapper.cpp:157-159) on a frame's match table [n] (point slot or -1), ascending
// keypoint: every entry whose point is alive is associated with key frame kf at that keypoint; an entry that names a
// removed slot or a slot the map never had (a dangling pointer in the reference) is skipped.  Returns the associations made.
static inline int mirror_adopt_table(MapMirror* m, int kf, const int32_t* table, int n)
{
    int adopted = 0;
    const int rows = n < m->kfs[(size_t)kf].n ? n : m->kfs[(size_t)kf].n;
    for (int i = 0; i < rows; i++) {
        const int32_t p = table[i];
        if (p < 0 || !mirror_point_ok(m, p)) continue;
        if (mirror_add_observation(m, p, kf, i) == RS_OK) adopted++;
    }
    return adopted;
}

// Mapper::triangulate_tracks' creation loop (src/Mapper.cpp:310-331) for the accepted tracks of an rs_track_results, in their
// order.  Everything is checked before the first edit: a refused call leaves the mirror as it was.
static inline int mirror_add_track_points(MapMirror* m, int kf, const rs_track_results* r, const int32_t* h_window_kfs, int n_window,
                                          int32_t* h_new_points)
{
    if (!r || !mirror_kf_ok(m, kf) || n_window < 0 || (n_window > 0 && !h_window_kfs)) return RS_ERR_INVALID;
    const int na = r->counts[0];
    if (na < 0 || na > r->capacity_tracks || r->n_pairs < 0) return RS_ERR_INVALID;
    if (r->n_pairs > r->capacity_pairs) return RS_ERR_INVALID;            // only the first capacity_pairs pairs were copied
    if (na == 0) return RS_OK;
    if (!r->h_keypoint || !r->h_xyz || !r->h_sightings || !r->h_kf_ptr || (r->n_pairs > 0 && !r->h_kf_pairs)) return RS_ERR_INVALID;
    const size_t KF = m->kfs.size();
    std::vector<uint8_t> in_window(KF, 0);
    for (int w = 0; w < n_window; w++) {
        if (!mirror_kf_ok(m, h_window_kfs[w])) return RS_ERR_INVALID;
        in_window[(size_t)h_window_kfs[w]] = 1;
    }
    const int kf_n = m->kfs[(size_t)kf].n;
    if (r->h_kf_ptr[0] < 0) return RS_ERR_INVALID;
    for (int a = 0; a < na; a++) {
        if (r->h_keypoint[a] < 0 || r->h_keypoint[a] >= kf_n) return RS_ERR_INVALID;
        const int32_t s0 = r->h_kf_ptr[a], s1 = r->h_kf_ptr[a + 1];
        if (s1 < s0 || s1 > r->n_pairs) return RS_ERR_INVALID;
        for (int32_t s = s0; s < s1; s++) {
            const int32_t h = r->h_kf_pairs[2 * (size_t)s], kp = r->h_kf_pairs[2 * (size_t)s + 1];
            if (h < 0 || h == kf || h >= (int32_t)KF || !in_window[(size_t)h]) continue;        // skipped below as well
            if (kp < 0 || kp >= m->kfs[(size_t)h].n) return RS_ERR_INVALID;
        }
    }
    for (int a = 0; a < na; a++) {
        const int p = mirror_add_point(m, r->h_xyz + 3 * (size_t)a);                             // Map::create_point, :312
        mirror_add_observation(m, p, kf, r->h_keypoint[a]);
        for (int32_t s = r->h_kf_ptr[a]; s < r->h_kf_ptr[a + 1]; s++) {
            const int32_t h = r->h_kf_pairs[2 * (size_t)s], kp = r->h_kf_pairs[2 * (size_t)s + 1];
            if (h < 0 || h == kf || h >= (int32_t)KF || !in_window[(size_t)h]) continue;        // :316-318
            if (m->kfs[(size_t)h].kp_point[(size_t)kp] >= 0 || mirror_observed_by(m, p, h)) continue;   // :319-321
            mirror_add_observation(m, p, h, kp);                                                 // :322
        }
        if (r->h_sightings[a] >= 3) mirror_set_track_consistent(m, p);                           // :326-329
        if (h_new_points) h_new_points[a] = p;
    }
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ loop fusion
// The invariant every edit above keeps: table[kf][kp] == p exactly when (kf, kp) is an observation of the alive point p, and a
// point has at most one observation per key frame.
static inline bool mirror_consistent(const MapMirror* m)
{
    size_t in_tables = 0, in_rows = 0;
    for (size_t k = 0; k < m->kfs.size(); k++)
        for (int i = 0; i < m->kfs[k].n; i++) {
            const int p = m->kfs[k].kp_point[(size_t)i];
            if (p < 0) continue;
            in_tables++;
            if (!mirror_point_ok(m, p)) return false;
            int found = 0;
            for (const MapObs& o : m->obs[(size_t)p]) found += (o.kf == (int)k && o.kp == i) ? 1 : 0;
            if (found != 1) return false;
        }
    for (size_t p = 0; p < m->obs.size(); p++) {
        if (!m->alive[p] && !m->obs[p].empty()) return false;
        for (size_t a = 0; a < m->obs[p].size(); a++) {
            const MapObs& o = m->obs[p][a];
            if (!mirror_kf_ok(m, o.kf) || o.kp < 0 || o.kp >= m->kfs[(size_t)o.kf].n) return false;
            for (size_t b = a + 1; b < m->obs[p].size(); b++)
                if (m->obs[p][b].kf == o.kf) return false;
        }
        in_rows += m->obs[p].size();
    }
    return in_tables == in_rows;
}

// Frame::is_matched(point): the key frame's table names the point somewhere
static inline bool mirror_kf_matches(const MapMirror* m, int kf, int point)
{
    for (const int32_t p : m->kfs[(size_t)kf].kp_point)
        if (p == point) return true;
    return false;
}

// Map::fuse (src/Map.cpp:78-95): the observations of `discarded` move to `kept`, in discarded's observation order, unless
// the observer already sees `kept`; `discarded` hands over its track_consistent flag (:91-93) and is removed.  The loop
// walks a COPY of the list, as the reference does: every turn erases from the original.
static inline int mirror_fuse(MapMirror* m, int kept, int discarded)
{
    if (!mirror_point_ok(m, kept) || !mirror_point_ok(m, discarded)) return RS_ERR_INVALID;
    if (kept == discarded) return RS_OK;                                  // :80-82
    const std::vector<MapObs> observations = m->obs[(size_t)discarded];
    for (const MapObs& o : observations) {
        mirror_remove_observation(m, discarded, o.kf);                    // :85
        if (mirror_observed_by(m, kept, o.kf) || m->kfs[(size_t)o.kf].kp_point[(size_t)o.kp] >= 0 || mirror_kf_matches(m, o.kf, kept))
            continue;                                                     // :86-88
        mirror_add_observation(m, kept, o.kf, o.kp);                      // :89
    }
    if (m->consistent[(size_t)discarded]) mirror_set_track_consistent(m, kept);
    return mirror_remove_point(m, discarded);                             // :94
}

// Mapper::fuse_match (src/Mapper.cpp:176-196) for keypoint kp of key frame kf and the point `kept`; is_old [n_flags] marks
// the loop's old points.  Returns the outcome (RS_FUSE_*); *removed = the discarded slot of a fuse, else -1.  An entry
// whose keypoint is outside the key frame or whose point is dead or unknown is a no-op (the reference would follow a
// dangling pointer).
static inline int mirror_fuse_match(MapMirror* m, int kf, int kp, int kept, const uint8_t* is_old, size_t n_flags, int* removed)
{
    if (removed) *removed = -1;
    if (!mirror_kf_ok(m, kf) || kp < 0 || kp >= m->kfs[(size_t)kf].n || !mirror_point_ok(m, kept)) return RS_FUSE_SKIPPED;
    const int existing = m->kfs[(size_t)kf].kp_point[(size_t)kp];
    if (existing < 0) {                                                   // :184-190
        if (mirror_kf_matches(m, kf, kept)) return RS_FUSE_POINT_MATCHED;
        mirror_add_observation(m, kept, kf, kp);
        return RS_FUSE_ASSOCIATED;
    }
    if (existing == kept) return RS_FUSE_SAME;                            // :192
    if ((size_t)existing < n_flags && is_old[(size_t)existing]) return RS_FUSE_OLD;
    if (mirror_fuse(m, kept, existing) != RS_OK) return RS_FUSE_SKIPPED;
    if (removed) *removed = existing;
    return RS_FUSE_FUSED;
}

// loop_covisibles (src/Mapper.cpp:41-66): the candidate, then at most max_covisible key frames that share at least
// min_shared of the candidate's points, ranked by shared count descending, key-frame handle ascending (the reference
// sorts an unordered_map by count alone: ties are unspecified upstream).  The candidate's own observations do not count.
static inline void mirror_loop_old_frames(const MapMirror* m, int candidate, int min_shared, int max_covisible, std::vector<int32_t>* out)
{
    out->assign(1, candidate);
    const size_t KF = m->kfs.size();
    std::vector<int32_t> shared(KF, 0);
    for (const int32_t p : m->kfs[(size_t)candidate].kp_point) {
        if (p < 0) continue;
        for (const MapObs& o : m->obs[(size_t)p])
            if (o.kf != candidate) shared[(size_t)o.kf]++;
    }
    for (int r = 0; r < max_covisible; r++) {
        int best = -1;
        for (size_t k = 0; k < KF; k++)
            if (shared[k] > 0 && shared[k] >= min_shared && (best < 0 || shared[k] > shared[(size_t)best])) best = (int)k;
        if (best < 0) break;
        out->push_back(best);
        shared[(size_t)best] = 0;
    }
}

// loop_points (src/Mapper.cpp:68-77) as a flag per point slot
static inline void mirror_loop_points(const MapMirror* m, const std::vector<int32_t>& old_frames, std::vector<uint8_t>* is_old)
{
    is_old->assign(m->alive.size(), 0);
    for (const int32_t kf : old_frames)
        for (const int32_t p : m->kfs[(size_t)kf].kp_point)
            if (p >= 0) (*is_old)[(size_t)p] = 1;
}

// One journal section — the (keypoint, point) pairs of key frame kf, in order — applied to the mirror.  Every outcome is
// recomputed here: the section supplies matches, not decisions.  outcomes [n] (NULL = not wanted); the discarded slots of
// the fuses are appended to *removed (NULL = not wanted); counts [6] are incremented per outcome.
static inline void mirror_replay_fuse(MapMirror* m, int kf, const int32_t* kp, const int32_t* point, int n, const uint8_t* is_old,
                                      size_t n_flags, int32_t* outcomes, std::vector<int32_t>* removed, int counts[6])
{
    for (int i = 0; i < n; i++) {
        int gone = -1;
        const int oc = mirror_fuse_match(m, kf, kp[i], point[i], is_old, n_flags, &gone);
        if (outcomes) outcomes[i] = oc;
        if (counts) counts[oc]++;
        if (gone >= 0 && removed) removed->push_back(gone);
    }
}
