// test_klt_host.cpp — drives slam::Session::track_features (racing-slam_amd/host) the way Tracker::track frames do.
//
//     test_klt_host <dir>
// reads <dir>/meta.txt ("width height n"), img1.u8, img2.u8, img3.u8 (grey frames; the test passes frame 1 again as frame 3), bgr2.u8 (frame 2 as BGR),
// pts.f32 ([n][2]) and mask.u8, and writes <dir>/out_<call>.txt: "count" then "index x y" per kept point
// (x, y as the hexadecimal bit patterns of the f32 values), for
//   call 0: img1 -> img2 with the mask          (both frames uploaded)
//   call 1: img2 -> img3 with the mask          (frame 2's pyramid reused: the previous call's `next` object)
//   call 2: img1 -> bgr2 without a mask         (BGR upload)
// tests/test_klt_host.py compares the outputs with tests/klt_ref.py.
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

static void write_out(const std::string& path, const std::pair<slam::ExtractedFeatures, std::vector<slam::FeatureMatch>>& r)
{
    FILE* f = std::fopen(path.c_str(), "w");
    std::fprintf(f, "%zu\n", r.second.size());
    for (size_t k = 0; k < r.second.size(); k++) {
        uint32_t x, y;
        const auto& pt = r.first.keypoints[r.second[k].query_index].pt;
        std::memcpy(&x, &pt.x, 4);
        std::memcpy(&y, &pt.y, 4);
        std::fprintf(f, "%zu %08x %08x\n", r.second[k].train_index, x, y);
    }
    std::fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_klt_host <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int W = 0, H = 0, n = 0;
    FILE* m = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %d %d", &W, &H, &n) != 3) { std::printf("bad meta.txt\n"); return 2; }
    std::fclose(m);
    slam::Image img[3], bgr2, mask, none;
    const char* names[3] = {"/img1.u8", "/img2.u8", "/img3.u8"};
    for (int i = 0; i < 3; i++) {
        img[i].width = W; img[i].height = H; img[i].channels = 1;
        if (!read_file(dir + names[i], img[i].pixels, (size_t)W * H)) { std::printf("cannot read %s\n", names[i]); return 2; }
    }
    bgr2.width = W; bgr2.height = H; bgr2.channels = 3;
    mask.width = W; mask.height = H;
    std::vector<uint8_t> raw;
    if (!read_file(dir + "/bgr2.u8", bgr2.pixels, (size_t)W * H * 3) || !read_file(dir + "/mask.u8", mask.pixels, (size_t)W * H) ||
        !read_file(dir + "/pts.f32", raw, sizeof(float) * 2 * (size_t)n)) { std::printf("cannot read inputs\n"); return 2; }
    slam::ExtractedFeatures prev;
    for (int i = 0; i < n; i++) {
        slam::KeyPoint kp;
        std::memcpy(&kp.pt.x, &raw[8 * (size_t)i], 4);
        std::memcpy(&kp.pt.y, &raw[8 * (size_t)i + 4], 4);
        prev.keypoints.push_back(kp);
        for (int b = 0; b < RS_DESC_BYTES; b++) prev.descriptors.push_back((uint8_t)(i + b));
    }
    auto& s = slam::Session::get();
    const auto r0 = s.track_features(img[0], img[1], prev, mask);
    // descriptor rows follow their keypoints (:130)
    for (size_t k = 0; k < r0.second.size(); k++)
        if (r0.first.descriptors[RS_DESC_BYTES * k] != (uint8_t)r0.second[k].train_index) { std::printf("descriptor row mismatch\n"); return 1; }
    write_out(dir + "/out_0.txt", r0);
    write_out(dir + "/out_1.txt", s.track_features(img[1], img[2], prev, mask));
    write_out(dir + "/out_2.txt", s.track_features(img[0], bgr2, prev, none));
    std::printf("klt host run done\n");
    return 0;
}
