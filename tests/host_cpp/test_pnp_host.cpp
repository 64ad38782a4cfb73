// test_pnp_host.cpp — drives slam::pose::estimate_pose_pnp (racing-slam_amd/host), the host-side form of the reference's
// cv::solvePnPRansac calls (LoopDetector's verify_pnp, Initialization's third-view check).
//
//     test_pnp_host <dir>
// reads <dir>/meta.txt ("n fx fy cx cy threshold"), object.f32 ([n][3]) and pixels.f32 ([n][2]).  Writes <dir>/out.txt: a
// line "status count", the 16 pose entries (hexadecimal f32 bits) and a line of the inlier indices.
// tests/test_pnp_host.py compares them with tests/pnp_ref.py.
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

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_pnp_host <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int n = 0;
    float fx, fy, cx, cy, thr;
    FILE* m = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %f %f %f %f %f", &n, &fx, &fy, &cx, &cy, &thr) != 6) { std::printf("bad meta.txt\n"); return 2; }
    std::fclose(m);
    std::vector<float> obj, pix;
    if (!read_floats(dir + "/object.f32", obj, 3 * (size_t)n) || !read_floats(dir + "/pixels.f32", pix, 2 * (size_t)n)) {
        std::printf("bad input files\n");
        return 2;
    }
    std::vector<slam::Vec3f> points(n);
    std::vector<slam::Vec2f> pixels(n);
    for (int k = 0; k < n; k++) {
        points[k] = {obj[3 * k], obj[3 * k + 1], obj[3 * k + 2]};
        pixels[k] = {pix[2 * k], pix[2 * k + 1]};
    }
    const slam::Camera camera(fx, fy, cx, cy, 1280, 720);
    const auto e = slam::pose::estimate_pose_pnp(points, pixels, camera, (double)thr);
    if (e.status < 0) { std::printf("the pnp call failed\n"); return 1; }
    FILE* o = std::fopen((dir + "/out.txt").c_str(), "w");
    if (!o) return 2;
    std::fprintf(o, "%d %zu\n", e.status, e.inliers.size());
    for (int k = 0; k < 16; k++) std::fprintf(o, "%08x%c", bits(e.pose[k]), k == 15 ? '\n' : ' ');
    for (size_t i : e.inliers) std::fprintf(o, "%zu ", i);
    std::fprintf(o, "\n");
    std::fclose(o);
    std::printf("estimate_pose_pnp: status %d, %zu inliers\n", e.status, e.inliers.size());
    return 0;
}
