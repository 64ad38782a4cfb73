// asan_keyframe.cpp — the mirror edits of rs_map_insert_keyframe and rs_map_add_track_points (csrc/map_mirror.h: plain C++, no
// GPU, no HIP) in a program of its own, built with -fsanitize=address,undefined by tests/test_keyframe_host.py.  Every input
// lives in an exactly-sized heap block, so an index one past a table, a pair list or a window list aborts here; the results
// are checked against what Map::associate's rules give.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../racing-slam_amd/csrc/map_mirror.h"

static int g_bad = 0;
static void expect_true(bool ok, const char* what)
{
    if (!ok) { g_bad++; std::printf("FAILED: %s\n", what); }
}

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
}

static int add_keyframe(MapMirror* m, int n)
{
    MapKeyFrame k;
    k.n = n;
    k.kp_point.assign((size_t)n, -1);
    for (int i = 0; i < 16; i++) k.pose[i] = i % 5 == 0 ? 1.f : 0.f;
    m->kfs.push_back(k);
    return (int)m->kfs.size() - 1;
}

static size_t n_obs(const MapMirror& m)
{
    size_t c = 0;
    for (const auto& v : m.obs) c += v.size();
    return c;
}

// both directions agree (tests/map_model.MapModel.consistent)
static bool consistent(const MapMirror& m)
{
    size_t in_tables = 0;
    for (size_t k = 0; k < m.kfs.size(); k++)
        for (int i = 0; i < m.kfs[k].n; i++) {
            const int p = m.kfs[k].kp_point[(size_t)i];
            if (p < 0) continue;
            in_tables++;
            if (!mirror_point_ok(&m, p)) return false;
            bool found = false;
            for (const auto& o : m.obs[(size_t)p]) found = found || (o.kf == (int)k && o.kp == i);
            if (!found) return false;
        }
    return in_tables == n_obs(m);
}

int main()
{
    MapMirror m;
    const float x[3] = {1.f, 2.f, 3.f};
    for (int k = 0; k < 4; k++) add_keyframe(&m, 8 + k);                    // 8, 9, 10, 11 keypoints
    for (int p = 0; p < 6; p++) mirror_add_point(&m, x);
    mirror_add_observation(&m, 0, 0, 0);
    mirror_add_observation(&m, 1, 0, 7);                                     // the last keypoint of key frame 0
    mirror_add_observation(&m, 1, 1, 8);                                     // the last keypoint of key frame 1
    mirror_add_observation(&m, 2, 2, 3);
    mirror_remove_point(&m, 3);                                              // a removed slot

    // ---- adoption: a table of exactly n entries; alive points, a removed slot, slots the map never had, one point twice
    const int kf = add_keyframe(&m, 5);
    {
        auto table = exact<int32_t>({1, 3, 6, 1, 2});
        expect_true(mirror_adopt_table(&m, kf, table.get(), 5) == 3, "adopted 3 entries (1, 1 again, 2)");
        expect_true(m.kfs[(size_t)kf].kp_point == std::vector<int32_t>({-1, -1, -1, 1, 2}), "the later keypoint holds point 1");
        expect_true(m.obs[1].size() == 3 && m.obs[1].back().kf == kf && m.obs[1].back().kp == 3, "point 1: three observers");
        auto huge = exact<int32_t>({2147483647, -2147483647 - 1, -1, 0, 5});
        const int kf2 = add_keyframe(&m, 5);
        expect_true(mirror_adopt_table(&m, kf2, huge.get(), 5) == 2, "extreme slots are skipped");
        expect_true(mirror_adopt_table(&m, kf2, huge.get(), 0) == 0, "an empty table");
        auto shorter = exact<int32_t>({4, 4});
        expect_true(mirror_adopt_table(&m, kf2, shorter.get(), 2) == 2 && m.kfs[(size_t)kf2].kp_point[1] == 4, "a table shorter than the key frame");
        expect_true(consistent(m), "consistent after the adoptions");
    }

    // ---- the creation loop: exactly-sized results; every skip rule; the last keypoint of every key frame
    const int nk = add_keyframe(&m, 6);                                      // the new key frame: handle 6
    {
        //   track 0: kp 5 (the last); pairs (0, 1) taken below? no: free -> associated; (-1, 0) null; (6, 2) itself; (1, 8) taken by point 1
        //   track 1: kp 0; pairs (3, 10) the last keypoint of key frame 3 -> associated; (3, 9) same observer again -> skipped
        //   track 2: kp 2; pairs (2, 9) outside the window; (7, 0) a key frame that does not exist -> skipped like one outside the window
        //   track 3: kp 1; no pairs; 3 sightings -> consistent
        auto kp = exact<int32_t>({5, 0, 2, 1});
        auto xyz = exact<float>({0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0, 4});
        auto sight = exact<int32_t>({2, 3, 1, 3});
        auto ptr = exact<int32_t>({0, 4, 6, 8, 8});
        auto pairs = exact<int32_t>({0, 1, -1, 0, 6, 2, 1, 8, 3, 10, 3, 9, 2, 9, 7, 0});
        auto window = exact<int32_t>({0, 1, 3, 6});
        auto created = exact<int32_t>({-1, -1, -1, -1});
        rs_track_results r{};
        r.capacity_tracks = 4; r.capacity_pairs = 8; r.counts[0] = 4; r.n_tracks = 4; r.n_pairs = 8;
        r.h_keypoint = kp.get(); r.h_xyz = xyz.get(); r.h_sightings = sight.get(); r.h_kf_ptr = ptr.get(); r.h_kf_pairs = pairs.get();
        const size_t slots0 = m.alive.size(), obs0 = n_obs(m);
        // refusals first: each leaves the mirror as it was
        r.n_pairs = 9;
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "n_pairs > capacity_pairs is refused");
        r.n_pairs = 8;
        auto bad_window = exact<int32_t>({0, 1, 3, 9});
        expect_true(mirror_add_track_points(&m, nk, &r, bad_window.get(), 4, created.get()) == RS_ERR_INVALID, "an unknown window key frame is refused");
        expect_true(mirror_add_track_points(&m, 9, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "an unknown key frame is refused");
        kp[0] = 6;
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "a keypoint outside the key frame is refused");
        kp[0] = 5;
        pairs[9] = 11;
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "a sighting keypoint outside its key frame is refused");
        pairs[9] = 10;
        ptr[4] = 9;
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "a pair offset past n_pairs is refused");
        ptr[4] = 8;
        r.counts[0] = 5;
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_ERR_INVALID, "more accepted tracks than capacity is refused");
        r.counts[0] = 4;
        expect_true(m.alive.size() == slots0 && n_obs(m) == obs0, "refusals changed nothing");
        expect_true(mirror_add_track_points(&m, nk, &r, window.get(), 4, created.get()) == RS_OK, "the creation loop");
        const int p0 = (int)slots0;
        expect_true(created[0] == p0 && created[1] == p0 + 1 && created[2] == p0 + 2 && created[3] == p0 + 3, "new slots in track order");
        expect_true(m.obs[(size_t)p0].size() == 2 && m.obs[(size_t)p0][1].kf == 0 && m.obs[(size_t)p0][1].kp == 1, "track 0: the new key frame and key frame 0");
        expect_true(m.kfs[1].kp_point[8] == 1, "a taken keypoint keeps its point");
        expect_true(m.obs[(size_t)p0 + 1].size() == 2 && m.kfs[3].kp_point[10] == p0 + 1 && m.kfs[3].kp_point[9] == -1, "track 1: one observation per observer");
        expect_true(m.obs[(size_t)p0 + 2].size() == 1 && m.kfs[2].kp_point[9] == -1, "track 2: outside the window");
        expect_true(m.consistent[(size_t)p0] == 0 && m.consistent[(size_t)p0 + 1] == 1 && m.consistent[(size_t)p0 + 2] == 0 && m.consistent[(size_t)p0 + 3] == 1,
                    "track-consistent from three sightings");
        expect_true(m.kfs[(size_t)nk].kp_point == std::vector<int32_t>({p0 + 1, p0 + 3, p0 + 2, -1, -1, p0}), "the new key frame's table");
        expect_true(consistent(m), "consistent after the creation loop");
        // no accepted tracks, null arrays: nothing to read
        rs_track_results none{};
        expect_true(mirror_add_track_points(&m, nk, &none, nullptr, 0, nullptr) == RS_OK && m.alive.size() == slots0 + 4, "no accepted tracks");
        // a window of zero key frames: only the key frame itself observes the new points
        auto kp1 = exact<int32_t>({3});
        auto ptr1 = exact<int32_t>({0, 1});
        auto pairs1 = exact<int32_t>({0, 2});
        auto one = exact<int32_t>({-1});
        rs_track_results r1{};
        r1.capacity_tracks = 1; r1.capacity_pairs = 1; r1.counts[0] = 1; r1.n_tracks = 1; r1.n_pairs = 1;
        r1.h_keypoint = kp1.get(); r1.h_xyz = xyz.get(); r1.h_sightings = sight.get(); r1.h_kf_ptr = ptr1.get(); r1.h_kf_pairs = pairs1.get();
        expect_true(mirror_add_track_points(&m, nk, &r1, nullptr, 0, one.get()) == RS_OK && m.obs[(size_t)one[0]].size() == 1, "an empty window");
    }
    // ---- removal after all of it: the tables forget the points
    for (int p = 0; p < (int)m.alive.size(); p++)
        if (mirror_point_ok(&m, p)) mirror_remove_point(&m, p);
    expect_true(n_obs(m) == 0 && m.n_alive == 0 && consistent(m), "everything removed");
    if (g_bad) return 1;
    std::printf("asan keyframe checks passed\n");
    return 0;
}
