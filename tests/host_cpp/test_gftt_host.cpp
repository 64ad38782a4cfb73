// test_gftt_host.cpp — drives slam::Session::replenish_features (racing-slam_amd/host) the way Tracker::track_features
// does after its KLT half (src/Tracker.cpp:127-146), and the way Initialization does (no budget, no tracked points).
//
//     test_gftt_host <dir>
// reads <dir>/meta.txt ("width height n"), img1.u8, img2.u8 (grey frames), pts.f32 ([n][2]) and mask.u8, and writes
// <dir>/out_<call>.txt: "detected appended n_keypoints" then "x y r" per appended keypoint (the hexadecimal bit patterns
// of the f32 position and response), for
//   call 0: track_features(img1 -> img2, mask), then replenish_features(img2, mask, tracked, 2000)  (pyramid reused)
//   call 1: replenish_features(img1, mask, {}, -1)                                                   (frame uploaded)
// tests/test_gftt_host.py compares the outputs with tests/klt_ref.py and tests/gftt_ref.py.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

static bool read_file(const std::string& path, std::vector<uint8_t>& out, size_t bytes)
{
    std::ifstream f(path, std::ios::binary);
    out.resize(bytes);
    return f && f.read((char*)out.data(), (std::streamsize)bytes) && (size_t)f.gcount() == bytes;
}

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

static void write_out(const std::string& path, int detected, size_t first, const slam::ExtractedFeatures& f,
                      const std::vector<float>& resp)
{
    FILE* o = std::fopen(path.c_str(), "w");
    std::fprintf(o, "%d %zu %zu\n", detected, f.keypoints.size() - first, f.keypoints.size());
    for (size_t k = first; k < f.keypoints.size(); k++)
        std::fprintf(o, "%08x %08x %08x\n", bits(f.keypoints[k].pt.x), bits(f.keypoints[k].pt.y), bits(resp[k - first]));
    std::fclose(o);
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_gftt_host <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int W = 0, H = 0, n = 0;
    FILE* m = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %d %d", &W, &H, &n) != 3) { std::printf("bad meta.txt\n"); return 2; }
    std::fclose(m);
    slam::Image img[2], mask;
    const char* names[2] = {"/img1.u8", "/img2.u8"};
    for (int i = 0; i < 2; i++) {
        img[i].width = W; img[i].height = H; img[i].channels = 1;
        if (!read_file(dir + names[i], img[i].pixels, (size_t)W * H)) { std::printf("cannot read %s\n", names[i]); return 2; }
    }
    mask.width = W; mask.height = H;
    std::vector<uint8_t> raw;
    if (!read_file(dir + "/mask.u8", mask.pixels, (size_t)W * H) || !read_file(dir + "/pts.f32", raw, sizeof(float) * 2 * (size_t)n)) {
        std::printf("cannot read inputs\n");
        return 2;
    }
    slam::ExtractedFeatures prev;
    for (int i = 0; i < n; i++) {
        slam::KeyPoint kp;
        std::memcpy(&kp.pt.x, &raw[8 * (size_t)i], 4);
        std::memcpy(&kp.pt.y, &raw[8 * (size_t)i + 4], 4);
        prev.keypoints.push_back(kp);
        for (int b = 0; b < RS_DESC_BYTES; b++) prev.descriptors.push_back((uint8_t)(i + b + 1));
    }
    auto& s = slam::Session::get();
    auto tracked = s.track_features(img[0], img[1], prev, mask).first;
    const size_t m0 = tracked.keypoints.size();
    std::vector<float> resp;
    const int d0 = s.replenish_features(img[1], mask, tracked, 2000, &resp);
    if (d0 < 0) { std::printf("replenish_features failed\n"); return 1; }
    // descriptor rows stay aligned: the tracked rows unchanged, zero rows for the appended keypoints
    if (tracked.descriptors.size() != tracked.keypoints.size() * RS_DESC_BYTES) { std::printf("descriptor rows misaligned\n"); return 1; }
    for (size_t k = m0; k < tracked.keypoints.size(); k++)
        for (int b = 0; b < RS_DESC_BYTES; b++)
            if (tracked.descriptors[k * RS_DESC_BYTES + b] != 0) { std::printf("appended row not zero\n"); return 1; }
    write_out(dir + "/out_0.txt", d0, m0, tracked, resp);
    slam::ExtractedFeatures fresh;
    std::vector<float> resp1;
    const int d1 = s.replenish_features(img[0], mask, fresh, -1, &resp1);
    if (d1 < 0) { std::printf("replenish_features failed\n"); return 1; }
    write_out(dir + "/out_1.txt", d1, 0, fresh, resp1);
    std::printf("gftt host run done\n");
    return 0;
}
