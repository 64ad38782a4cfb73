// test_pose_host.cpp — drives slam::pose::estimate_pose and estimate_pose_with_known_rotation (racing-slam_amd/host),
// the mirror of the reference's src/PoseEstimation.h, the way Tracker::initial_pose_estimate (src/Tracker.cpp:162) and
// Initialization.cpp:153 call them.
//
//     test_pose_host <dir>
// reads <dir>/meta.txt ("n fx fy cx cy"), from.f32 and to.f32 ([n][2]: match k pairs previous keypoint k with keypoint
// k) and rot.f32 ([9] row-major).  Writes <dir>/out.txt: for estimate_pose then the known-rotation form, a line
// "status count" followed by the 16 pose entries (hexadecimal f32 bits) and a line of the inlier match indices; then a
// line of the 400 pair indices of known_rotation_pairs(n).  tests/test_pose_host.py compares them with
// tests/essential_ref.py.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

static bool read_floats(const std::string& path, std::vector<float>& out, size_t count)
{
    std::ifstream f(path, std::ios::binary);
    out.resize(count);
    return f && f.read((char*)out.data(), (std::streamsize)(4 * count)) && (size_t)f.gcount() == 4 * count;
}

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

static void write(FILE* o, const slam::pose::PoseEstimate& e)
{
    std::fprintf(o, "%d %zu\n", e.status, e.inlier_matches.size());
    for (int k = 0; k < 16; k++) std::fprintf(o, "%08x%c", bits(e.pose[k]), k == 15 ? '\n' : ' ');
    for (const auto& m : e.inlier_matches) std::fprintf(o, "%zu ", m.query_index);
    std::fprintf(o, "\n");
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_pose_host <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int n = 0;
    float fx, fy, cx, cy;
    FILE* m = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %f %f %f %f", &n, &fx, &fy, &cx, &cy) != 5) { std::printf("bad meta.txt\n"); return 2; }
    std::fclose(m);
    std::vector<float> from, to, rot;
    if (!read_floats(dir + "/from.f32", from, 2 * (size_t)n) || !read_floats(dir + "/to.f32", to, 2 * (size_t)n) ||
        !read_floats(dir + "/rot.f32", rot, 9)) {
        std::printf("bad input files\n");
        return 2;
    }
    slam::ExtractedFeatures prev, cur;
    std::vector<slam::FeatureMatch> matches;
    for (int k = 0; k < n; k++) {
        slam::KeyPoint a, b;
        a.pt = {from[2 * k], from[2 * k + 1]};
        b.pt = {to[2 * k], to[2 * k + 1]};
        prev.keypoints.push_back(a);
        cur.keypoints.push_back(b);
        matches.emplace_back(k, k);
    }
    const slam::Camera camera(fx, fy, cx, cy, 1280, 720);
    std::array<float, 9> R;
    for (int k = 0; k < 9; k++) R[k] = rot[k];
    const auto e = slam::pose::estimate_pose(prev, cur, matches, camera);
    const auto k = slam::pose::estimate_pose_with_known_rotation(prev, cur, matches, camera, R);
    if (e.status < 0 || k.status < 0) { std::printf("a pose call failed\n"); return 1; }
    FILE* o = std::fopen((dir + "/out.txt").c_str(), "w");
    if (!o) return 2;
    write(o, e);
    write(o, k);
    for (int32_t v : slam::pose::known_rotation_pairs((size_t)n)) std::fprintf(o, "%d ", v);
    std::fprintf(o, "\n");
    std::fclose(o);
    std::printf("estimate_pose: status %d, %zu inliers; known rotation: status %d, %zu inliers\n", e.status,
                e.inlier_matches.size(), k.status, k.inlier_matches.size());
    return 0;
}
