// test_track_host.cpp — argument validation of the frame-table calls (racing-slam_amd/csrc/frame_matches.hip) and of the
// host mirror's slam::track_tail, from C++:
//     test_track_host
// null pointers, a foreign context, a frame of another context, `kind` out of range and the RS_ERR_UNSUPPORTED envelope
// must be refused with the documented status and must leave the frame's table and the outputs as they were; then one
// tiny valid sequence (add, carry below min_points, gated refit, match on an empty map) must run.  Prints
// "track host ok: <checks>"; any surprise is reported and the exit status is 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

static int g_checks = 0, g_bad = 0;
static void expect(int got, int want, const char* what)
{
    g_checks++;
    if (got != want) { g_bad++; std::printf("%s: status %d, expected %d\n", what, got, want); }
}
static void expect_true(bool ok, const char* what)
{
    g_checks++;
    if (!ok) { g_bad++; std::printf("%s\n", what); }
}

int main()
{
    rs_context *ctx = nullptr, *other = nullptr;
    if (rs_context_create(0, &ctx) != RS_OK || rs_context_create(0, &other) != RS_OK) { std::printf("no context\n"); return 2; }
    const int n = 40;
    std::vector<float> kp(2 * n);
    std::vector<uint8_t> desc(32 * n);
    for (int i = 0; i < n; i++) { kp[2 * i] = 10.f + 13.f * i; kp[2 * i + 1] = 20.f + 7.f * (i % 9); desc[32 * i] = (uint8_t)i; }
    rs_frame *f = nullptr, *g = nullptr, *foreign = nullptr;
    rs_map *map = nullptr, *foreign_map = nullptr;
    if (rs_frame_create(ctx, kp.data(), desc.data(), n, &f) != RS_OK || rs_frame_create(ctx, kp.data(), desc.data(), n, &g) != RS_OK ||
        rs_frame_create(other, kp.data(), desc.data(), n, &foreign) != RS_OK || rs_map_create(ctx, &map) != RS_OK ||
        rs_map_create(other, &foreign_map) != RS_OK) { std::printf("setup failed\n"); return 2; }
    void *d_kp = nullptr, *d_pt = nullptr;
    std::vector<int32_t> lk(n), lp(n);
    for (int i = 0; i < n; i++) { lk[i] = i; lp[i] = 100 + i; }
    expect(rs_stage_begin(ctx), RS_OK, "rs_stage_begin");
    expect(rs_stage_upload(ctx, lk.data(), 4 * n, &d_kp), RS_OK, "upload");
    expect(rs_stage_upload(ctx, lp.data(), 4 * n, &d_pt), RS_OK, "upload");
    const int32_t *dk = (const int32_t*)d_kp, *dp = (const int32_t*)d_pt;
    std::vector<int32_t> tab(n, 7);
    int cnt = -5;

    // ---- the table
    expect(rs_frame_matches_clear(nullptr, f), RS_ERR_INVALID, "clear: null context");
    expect(rs_frame_matches_clear(ctx, nullptr), RS_ERR_INVALID, "clear: null frame");
    expect(rs_frame_matches_clear(ctx, foreign), RS_ERR_INVALID, "clear: a frame of another context");
    expect(rs_frame_matches_add(nullptr, f, dk, dp, nullptr, n), RS_ERR_INVALID, "add: null context");
    expect(rs_frame_matches_add(other, f, dk, dp, nullptr, n), RS_ERR_INVALID, "add: foreign context");
    expect(rs_frame_matches_add(ctx, f, nullptr, dp, nullptr, n), RS_ERR_INVALID, "add: null keypoint list");
    expect(rs_frame_matches_add(ctx, f, dk, nullptr, nullptr, n), RS_ERR_INVALID, "add: null point list");
    expect(rs_frame_matches_add(ctx, f, dk, dp, nullptr, -1), RS_ERR_INVALID, "add: negative max_n");
    expect(rs_frame_matches_add(ctx, f, dk, dp, nullptr, 8193), RS_ERR_UNSUPPORTED, "add: more than 8192 entries");
    expect(rs_frame_matches_download(ctx, nullptr, tab.data(), &cnt), RS_ERR_INVALID, "download: null frame");
    expect(rs_frame_matches_download(other, f, tab.data(), &cnt), RS_ERR_INVALID, "download: foreign context");
    expect(rs_frame_matches_download(ctx, f, tab.data(), &cnt), RS_OK, "download");
    bool empty = cnt == 0;
    for (int i = 0; i < n; i++) empty = empty && tab[i] == -1;
    expect_true(empty, "a refused call changed the table, or a new frame's table is not empty");
    expect(rs_frame_matches_add(ctx, f, dk, dp, nullptr, 0), RS_OK, "add: an empty list");
    expect(rs_frame_matches_add(ctx, f, dk, dp, nullptr, 10), RS_OK, "add");
    expect(rs_frame_matches_download(ctx, f, tab.data(), &cnt), RS_OK, "download");
    expect_true(cnt == 10 && tab[0] == 100 && tab[9] == 109 && tab[10] == -1, "add: wrong table");
    expect(rs_frame_matches_download(ctx, f, nullptr, nullptr), RS_OK, "download: nothing wanted");

    // ---- carry-over
    expect(rs_map_set_track_consistent(nullptr, 0), RS_ERR_INVALID, "set_track_consistent: null map");
    expect(rs_map_set_track_consistent(map, 0), RS_ERR_INVALID, "set_track_consistent: no such point");
    expect(rs_map_carry_matches(ctx, nullptr, f, g, dk, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: null map");
    expect(rs_map_carry_matches(ctx, foreign_map, f, g, dk, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: a map of another context");
    expect(rs_map_carry_matches(ctx, map, nullptr, g, dk, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: null prev");
    expect(rs_map_carry_matches(ctx, map, f, foreign, dk, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: a frame of another context");
    expect(rs_map_carry_matches(ctx, map, f, f, dk, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: one frame twice");
    expect(rs_map_carry_matches(ctx, map, f, g, nullptr, nullptr, nullptr, n, 15, nullptr), RS_ERR_INVALID, "carry: null index list");
    expect(rs_map_carry_matches(ctx, map, f, g, dk, nullptr, nullptr, -2, 15, nullptr), RS_ERR_INVALID, "carry: negative max_n");
    expect(rs_map_carry_matches(ctx, map, f, g, dk, nullptr, nullptr, 9000, 15, nullptr), RS_ERR_UNSUPPORTED, "carry: more than 8192 entries");
    expect(rs_map_carry_matches(ctx, map, f, g, dk, nullptr, nullptr, n, 15, nullptr), RS_OK, "carry: an empty map");

    // ---- refit
    double cam[6] = {0.1, 0.2, 0.3, 1, 2, 3}, cam0[6], vel[3] = {0, 0, 0};
    std::memcpy(cam0, cam, sizeof cam);
    const float K[4] = {500, 500, 320, 240};
    rs_ba_summary s;
    int used = 99;
    std::memset(&s, 0x55, sizeof s);
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, nullptr, &used),
           RS_ERR_INVALID, "refine: null summary");
    expect(rs_map_refine_pose(ctx, nullptr, f, cam, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: null map");
    expect_true(s.usable == 0 && s.iterations == 0, "refine: a refused call must zero the summary");
    expect(rs_map_refine_pose(ctx, map, foreign, cam, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: a frame of another context");
    expect(rs_map_refine_pose(ctx, map, f, nullptr, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: null camera");
    expect(rs_map_refine_pose(ctx, map, f, cam, nullptr, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: null intrinsics");
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, nullptr),
           RS_ERR_INVALID, "refine: null n_used");
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 15, 3, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: kind 3");
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 15, -1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_ERR_INVALID, "refine: kind -1");
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 15, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_OK, "refine: 10 matches");
    expect_true(used == -1 && s.usable == 0 && !std::memcmp(cam, cam0, sizeof cam), "refine: the match gate must refuse and leave the camera");
    expect(rs_map_refine_pose(ctx, map, f, cam, K, 5, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, vel, nullptr, &s, &used),
           RS_OK, "refine: no point of the table is in the map");
    expect_true(used == 0 && s.usable == 0 && !std::memcmp(cam, cam0, sizeof cam), "refine: no observation, no solve");

    // ---- match
    const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    cnt = -5;
    expect(rs_map_match_frame(ctx, map, f, T, K, 640, 480, -1, 64, nullptr), RS_ERR_INVALID, "match: null count");
    expect(rs_map_match_frame(ctx, map, f, nullptr, K, 640, 480, -1, 64, &cnt), RS_ERR_INVALID, "match: null pose");
    expect(rs_map_match_frame(ctx, map, f, T, nullptr, 640, 480, -1, 64, &cnt), RS_ERR_INVALID, "match: null intrinsics");
    expect(rs_map_match_frame(ctx, foreign_map, f, T, K, 640, 480, -1, 64, &cnt), RS_ERR_INVALID, "match: a map of another context");
    expect(rs_map_match_frame(ctx, map, foreign, T, K, 640, 480, -1, 64, &cnt), RS_ERR_INVALID, "match: a frame of another context");
    expect(rs_map_match_frame(ctx, map, f, T, K, 640, 480, 0, 64, &cnt), RS_ERR_INVALID, "match: unknown key frame");
    expect(rs_map_match_frame(ctx, map, f, T, K, 640, 480, -1, 64, &cnt), RS_OK, "match: an empty map");
    expect_true(cnt == 0, "match: an empty map matches nothing");

    // ---- the host mirror: one point seen twice, straight ahead of keypoint 3
    int kf0 = -1, kf1 = -1, pt = -1;
    const float xyz[3] = {(kp[6] - K[2]) / K[0] * 5.f, (kp[7] - K[3]) / K[1] * 5.f, 5.f};
    expect(rs_map_add_keyframe(map, g, T, &kf0), RS_OK, "add_keyframe");
    expect(rs_map_add_keyframe(map, g, T, &kf1), RS_OK, "add_keyframe");
    expect(rs_map_add_point(map, xyz, &pt), RS_OK, "add_point");
    expect(rs_map_add_observation(map, pt, kf0, 3), RS_OK, "add_observation");
    expect(rs_map_add_observation(map, pt, kf1, 3), RS_OK, "add_observation");
    expect(rs_map_set_track_consistent(map, pt), RS_OK, "set_track_consistent");
    expect(rs_frame_matches_clear(ctx, f), RS_OK, "clear");
    expect(rs_stage_begin(ctx), RS_OK, "rs_stage_begin");            // (the matches above recycled the pool the list lived in)
    expect(rs_stage_upload(ctx, lk.data(), 4 * n, &d_kp), RS_OK, "upload");
    dk = (const int32_t*)d_kp;
    slam::Camera camera(K[0], K[1], K[2], K[3], 640, 480);
    slam::Mat4f pose = slam::identity4();
    slam::TrackTail tail;
    expect_true(slam::track_tail(ctx, map, g, f, dk, nullptr, nullptr, n, camera, true, nullptr, kf1, pose, &tail), "track_tail failed");
    expect_true(tail.n_used == -1 && !tail.refined && tail.key_frame_matches == 1 && tail.map_matches == 0, "track_tail: wrong outcome");
    expect(rs_frame_matches_download(ctx, f, tab.data(), &cnt), RS_OK, "download");
    expect_true(cnt == 1 && tab[3] == pt, "track_tail: the match is not in the table");
    expect_true(!slam::track_tail(ctx, nullptr, g, f, dk, nullptr, nullptr, n, camera, true, nullptr, kf1, pose, &tail), "track_tail: a null map must fail");

    rs_frame_destroy(f); rs_frame_destroy(g); rs_frame_destroy(foreign);
    rs_map_destroy(map); rs_map_destroy(foreign_map);
    rs_context_destroy(other); rs_context_destroy(ctx);
    if (g_bad) { std::printf("track host: %d of %d checks failed\n", g_bad, g_checks); return 1; }
    std::printf("track host ok: %d\n", g_checks);
    return 0;
}
