// test_frame_host.cpp — drives slam::Session::refresh_descriptors' device-built frame (racing-slam_amd/host): the
// rs_frame that rs_frame_assign_device fills from the device lists of the front end, against the rs_frame that
// rs_frame_create builds on the host from the keypoints and rows the same call returned.
//
//     test_frame_host <dir>
// reads <dir>/meta.txt ("width height n"), img1.u8, img2.u8 (grey frames), pts.f32 ([n][2]) and mask.u8; runs
// track_features -> replenish_features -> refresh_descriptors(..., &frame) for img1 -> img2 and then, on the features that
// came out, for img2 -> img1 (the session's frame is refilled).  After each: rs_frame_download of both frames must hold
// the same bytes (n, keypoints, rows, node_kp | left | right, root, packed tree), and rs_map_match against a small
// resident map (every third keypoint a point 5 m down its ray, seen by a key frame made of the host frame) must return
// the same (keypoint, point) lists for both.  Prints "frame host ok: n1 matches1 n2 matches2"; any difference is
// reported and the exit status is 1.
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

struct Downloaded {
    int n = -1, root = -2;
    std::vector<float> kp;
    std::vector<uint8_t> desc, packed;
    std::vector<int32_t> kd;
};

static bool download(rs_context* ctx, const rs_frame* f, Downloaded& d)
{
    if (rs_frame_download(ctx, f, &d.n, nullptr, nullptr, nullptr, nullptr, nullptr) != RS_OK || d.n < 0) return false;
    const size_t m = d.n > 0 ? (size_t)d.n : 1;
    d.kp.assign(2 * m, 0.f); d.desc.assign(32 * m, 0); d.kd.assign(3 * m, 0); d.packed.assign(20 * m, 0);
    return rs_frame_download(ctx, f, &d.n, d.kp.data(), d.desc.data(), d.kd.data(), &d.root, d.packed.data()) == RS_OK;
}

static bool same(const Downloaded& a, const Downloaded& b)
{
    const size_t n = (size_t)a.n;
    const char* what = nullptr;
    if (a.n != b.n) what = "n";
    else if (a.root != b.root) what = "root";
    else if (n && std::memcmp(a.kp.data(), b.kp.data(), 8 * n)) what = "keypoints";
    else if (n && std::memcmp(a.desc.data(), b.desc.data(), 32 * n)) what = "descriptor rows";
    else if (n && std::memcmp(a.kd.data(), b.kd.data(), 12 * n)) what = "node_kp | left | right";
    else if (n && std::memcmp(a.packed.data(), b.packed.data(), 20 * n)) what = "packed tree";
    if (what) std::printf("device-built and host-built frame differ in: %s (n %d / %d)\n", what, a.n, b.n);
    return what == nullptr;
}

// one video frame: the session's device-built frame against rs_frame_create on what the session returned; the number of
// matches of both against a map made from the frame itself, or -1
static int one_frame(slam::Session& s, const slam::Image& from, const slam::Image& to, const slam::Image& mask,
                     const slam::ExtractedFeatures& prev, slam::ExtractedFeatures& out, int* n_out)
{
    rs_context* ctx = s.ctx();
    auto tracked = s.track_features(from, to, prev, mask);
    out = tracked.first;
    if (s.replenish_features(to, mask, out, 2000) < 0) { std::printf("replenish_features failed\n"); return -1; }
    rs_frame* dev = nullptr;
    const auto rows = s.refresh_descriptors(to, out, prev, tracked.second, &dev);
    const size_t n = out.keypoints.size();
    if (rows.size() != n * RS_DESC_BYTES || !dev) { std::printf("refresh_descriptors failed\n"); return -1; }
    out.descriptors = rows;
    std::vector<float> kp(2 * n);
    for (size_t k = 0; k < n; k++) { kp[2 * k] = out.keypoints[k].pt.x; kp[2 * k + 1] = out.keypoints[k].pt.y; }
    rs_frame* host = nullptr;
    if (rs_frame_create(ctx, kp.data(), rows.data(), (int)n, &host) != RS_OK) { std::printf("rs_frame_create failed\n"); return -1; }
    Downloaded a, b;
    int result = -1;
    rs_map* map = nullptr;
    if (download(ctx, dev, a) && download(ctx, host, b) && same(a, b) && rs_map_create(ctx, &map) == RS_OK) {
        const float K[4] = {1000.f, 1000.f, to.width / 2.f, to.height / 2.f};
        float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        int kf = -1;
        bool ok = rs_map_add_keyframe(map, host, T, &kf) == RS_OK;
        for (size_t k = 0; ok && k < n; k += 3) {
            const float xyz[3] = {(kp[2 * k] - K[2]) / K[0] * 5.f, (kp[2 * k + 1] - K[3]) / K[1] * 5.f, 5.f};
            int pt = -1;
            ok = rs_map_add_point(map, xyz, &pt) == RS_OK && rs_map_add_observation(map, pt, kf, (int)k) == RS_OK;
        }
        T[3] = 0.01f;                                            // a small step sideways: ~2 px
        std::vector<int32_t> mk[2], mp[2];
        int cnt[2] = {-1, -1};
        rs_frame* both[2] = {host, dev};
        for (int i = 0; ok && i < 2; i++) {
            mk[i].assign(n, -1); mp[i].assign(n, -1);
            ok = rs_map_match(ctx, map, both[i], T, K, to.width, to.height, nullptr, nullptr, 0, -1, nullptr, -1, 0, 64, mk[i].data(),
                              mp[i].data(), &cnt[i]) == RS_OK;
        }
        if (!ok) std::printf("map calls failed: %s\n", rs_last_error(ctx));
        else if (cnt[0] != cnt[1] || mk[0] != mk[1] || mp[0] != mp[1]) std::printf("matches differ (%d / %d)\n", cnt[0], cnt[1]);
        else result = cnt[0];
    }
    rs_map_destroy(map);
    rs_frame_destroy(host);
    *n_out = (int)n;
    return result;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_frame_host <dir>\n"); return 2; }
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
    slam::ExtractedFeatures f1, f2;
    int n1 = 0, n2 = 0;
    const int m1 = one_frame(s, img[0], img[1], mask, prev, f1, &n1);
    if (m1 < 0) return 1;
    const int m2 = one_frame(s, img[1], img[0], mask, f1, f2, &n2);      // the session's frame is refilled
    if (m2 < 0) return 1;
    std::printf("frame host ok: %d %d %d %d\n", n1, m1, n2, m2);
    return 0;
}
