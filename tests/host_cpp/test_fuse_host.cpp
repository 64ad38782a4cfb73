// test_fuse_host.cpp — drives slam::close_loop (racing-slam_amd/host: pose graph -> fuse_loop -> bundle adjustment with the
// oldest window frame fixed, all on the resident map) on a scene written by tests/test_fuse_host.py.
//
//     test_fuse_host <scene> <out>
// <scene>: integers only (floats as their 32-bit words):  fx fy cx cy width height | query candidate | n_kf, per key frame
// "n pose[16]" and n lines "x y d0 .. d31" | n_slots, per slot "alive x y z n_obs (kf kp)*" | n_inliers (kp point)* |
// n_window kf*.  The loop constraint's relative pose is the two key frames' own (rs_pose_relative), so the pose graph has
// nothing to correct beyond rounding.
// <out>: two runs on two maps built alike.  Run 1 (no adjustment, self-check on): "graph usable", the poses after the pose
// graph and the positions as words, then rs_map_fuse_loop's old frames, sources, removed points, sections and entries, the
// mismatch count and rs_map_counts — tests/test_fuse_host.py replays the fuse in tests/fuse_ref.py from those poses and
// positions.  Run 2 (with the adjustment): the summary, whether the oldest window frame kept its pose, and rs_map_counts.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

struct Scene {
    float K[4]; int width = 0, height = 0, query = 0, candidate = 0;
    struct Kf { int n = 0; float pose[16]; std::vector<float> kp; std::vector<uint8_t> desc; };
    struct Pt { int alive = 1; float xyz[3]; std::vector<int> obs; };
    std::vector<Kf> kfs;
    std::vector<Pt> pts;
    std::vector<int32_t> inlier_kp, inlier_pt, window;
};

static bool word(FILE* f, float* v)
{
    unsigned u = 0;
    if (std::fscanf(f, "%u", &u) != 1) return false;
    std::memcpy(v, &u, 4);
    return true;
}

static bool read_scene(const char* path, Scene* s)
{
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    bool ok = true;
    for (float& v : s->K) ok = ok && word(f, &v);
    ok = ok && std::fscanf(f, "%d %d %d %d", &s->width, &s->height, &s->query, &s->candidate) == 4;
    int n = 0;
    ok = ok && std::fscanf(f, "%d", &n) == 1;
    for (int k = 0; ok && k < n; k++) {
        Scene::Kf kf;
        ok = std::fscanf(f, "%d", &kf.n) == 1;
        for (float& v : kf.pose) ok = ok && word(f, &v);
        kf.kp.resize(2 * (size_t)kf.n);
        kf.desc.resize(32 * (size_t)kf.n);
        for (int i = 0; ok && i < kf.n; i++) {
            ok = word(f, &kf.kp[2 * (size_t)i]) && word(f, &kf.kp[2 * (size_t)i + 1]);
            for (int b = 0; ok && b < 32; b++) { unsigned u = 0; ok = std::fscanf(f, "%u", &u) == 1; kf.desc[32 * (size_t)i + (size_t)b] = (uint8_t)u; }
        }
        s->kfs.push_back(kf);
    }
    ok = ok && std::fscanf(f, "%d", &n) == 1;
    for (int p = 0; ok && p < n; p++) {
        Scene::Pt pt;
        int no = 0;
        ok = std::fscanf(f, "%d", &pt.alive) == 1 && word(f, &pt.xyz[0]) && word(f, &pt.xyz[1]) && word(f, &pt.xyz[2]) && std::fscanf(f, "%d", &no) == 1;
        pt.obs.resize(2 * (size_t)no);
        for (int& v : pt.obs) ok = ok && std::fscanf(f, "%d", &v) == 1;
        s->pts.push_back(pt);
    }
    ok = ok && std::fscanf(f, "%d", &n) == 1;
    for (int i = 0; ok && i < n; i++) { int a = 0, b = 0; ok = std::fscanf(f, "%d %d", &a, &b) == 2; s->inlier_kp.push_back(a); s->inlier_pt.push_back(b); }
    ok = ok && std::fscanf(f, "%d", &n) == 1;
    for (int i = 0; ok && i < n; i++) { int a = 0; ok = std::fscanf(f, "%d", &a) == 1; s->window.push_back(a); }
    std::fclose(f);
    return ok;
}

static rs_map* build_map(rs_context* ctx, const Scene& s)
{
    rs_map* map = nullptr;
    if (rs_map_create(ctx, &map) != RS_OK) return nullptr;
    for (const auto& k : s.kfs) {
        rs_frame* f = nullptr;
        int kf = -1;
        if (rs_frame_create(ctx, k.kp.data(), k.desc.data(), k.n, &f) != RS_OK || rs_map_add_keyframe(map, f, k.pose, &kf) != RS_OK) return nullptr;
        rs_frame_destroy(f);
    }
    for (const auto& p : s.pts) {
        int slot = -1;
        if (rs_map_add_point(map, p.xyz, &slot) != RS_OK) return nullptr;
        for (size_t o = 0; o + 1 < p.obs.size(); o += 2)
            if (rs_map_add_observation(map, slot, p.obs[o], p.obs[o + 1]) != RS_OK) return nullptr;
        if (!p.alive && rs_map_remove_point(map, slot) != RS_OK) return nullptr;
    }
    return map;
}

static void words(FILE* out, const char* name, const float* v, size_t n)
{
    std::fprintf(out, "%s", name);
    for (size_t i = 0; i < n; i++) { unsigned u; std::memcpy(&u, v + i, 4); std::fprintf(out, " %u", u); }
    std::fprintf(out, "\n");
}

static void ints(FILE* out, const char* name, const int32_t* v, size_t n)
{
    std::fprintf(out, "%s", name);
    for (size_t i = 0; i < n; i++) std::fprintf(out, " %d", v[i]);
    std::fprintf(out, "\n");
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::printf("usage: test_fuse_host <scene> <out>\n"); return 2; }
    Scene s;
    if (!read_scene(argv[1], &s)) { std::printf("cannot read the scene\n"); return 2; }
    FILE* out = std::fopen(argv[2], "w");
    rs_context* ctx = nullptr;
    if (!out || rs_context_create(0, &ctx) != RS_OK) { std::printf("no context\n"); return 2; }
    const slam::Camera camera(s.K[0], s.K[1], s.K[2], s.K[3], s.width, s.height);
    slam::LoopConstraint loop;
    loop.from = (size_t)s.query;
    loop.to = (size_t)s.candidate;
    rs_pose_relative(s.kfs[(size_t)s.query].pose, s.kfs[(size_t)s.candidate].pose, loop.relative.data());
    for (size_t i = 0; i < s.inlier_kp.size(); i++) loop.inlier_matches.push_back({s.inlier_kp[i], s.inlier_pt[i]});
    const double gravity[3] = {0.0, 0.0, 0.0};
    for (int run = 1; run <= 2; run++) {
        rs_map* map = build_map(ctx, s);
        if (!map) { std::printf("cannot build the map: %s\n", rs_last_error(ctx)); return 1; }
        slam::LoopClosure r;
        if (!slam::close_loop(ctx, map, {loop}, s.window, camera, 64, false, gravity, run == 2, true, &r)) return 1;
        int counts[4] = {0, 0, 0, 0};
        rs_map_counts(map, counts);
        if (run == 1) {
            std::vector<float> pos(3 * (size_t)counts[0] + 3);
            rs_map_get_positions(map, 0, counts[0], pos.data());
            std::fprintf(out, "graph %d\n", r.closed ? 1 : 0);
            words(out, "poses", r.graph_poses.data(), 16 * s.kfs.size());
            words(out, "positions", pos.data(), 3 * (size_t)counts[0]);
            ints(out, "old", r.fuse.old_frames, (size_t)r.fuse.n_old_frames);
            ints(out, "sources", r.sources.data(), r.sources.size());
            ints(out, "removed", r.removed.data(), r.removed.size());
            ints(out, "sections", r.section_ptr.data(), r.section_ptr.size());
            ints(out, "kp", r.journal_kp.data(), r.journal_kp.size());
            ints(out, "point", r.journal_point.data(), r.journal_point.size());
            ints(out, "outcome", r.journal_outcome.data(), r.journal_outcome.size());
            std::fprintf(out, "mismatches %d\n", r.fuse.device_state_mismatches);
            ints(out, "counts", counts, 4);
        } else {
            const bool fixed = std::memcmp(r.poses.data(), r.graph_poses.data() + 16 * (size_t)s.window[0], 64) == 0;
            std::fprintf(out, "adjust %d %d %d %.17g %.17g\n", r.adjust.usable, fixed ? 1 : 0, (int)r.adjusted.size(), r.adjust.initial_cost, r.adjust.final_cost);
            ints(out, "counts2", counts, 4);
            std::fprintf(out, "mismatches2 %d\n", r.fuse.device_state_mismatches);
        }
        rs_map_destroy(map);
    }
    std::fclose(out);
    rs_context_destroy(ctx);
    std::printf("fuse host ok\n");
    return 0;
}
