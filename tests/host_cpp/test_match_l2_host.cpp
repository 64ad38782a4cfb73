// test_match_l2_host.cpp — the host mirror's MapMatcher under NORM_L2 (racing-slam_amd/host/slam_host.h) through all four
// methods on one scene written by tests/test_match_l2_host.py, and under NORM_HAMMING on the same frames.  Usage:
//   test_match_l2_host.bin <dir>     reads <dir>/meta.txt and the arrays named below, writes <dir>/out.txt:
//   one line per call, "<label> <n> <keypoint> <point> ..." in the order the call returned them.
// Exit code 0 = ran to the end (the comparison with the restatement is the Python test's).  Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

using namespace slam;

template <typename T>
static std::vector<T> read_all(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    const size_t bytes = (size_t)f.tellg();
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read((char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = std::string(argv[1]) + "/";
    int N, P, NKF, dim, W, H, kf_required;
    float fx, fy, cx, cy, md_l2, md_u8;
    {
        std::ifstream meta(dir + "meta.txt");
        meta >> N >> P >> NKF >> dim >> W >> H >> fx >> fy >> cx >> cy >> md_l2 >> md_u8 >> kf_required;
        if (!meta) { std::printf("bad meta.txt\n"); return 2; }
    }
    const auto pose = read_all<float>(dir + "pose.f32"), kp = read_all<float>(dir + "kp.f32"), rows = read_all<float>(dir + "rows.f32");
    const auto desc = read_all<uint8_t>(dir + "desc.u8"), pool_u8 = read_all<uint8_t>(dir + "pool.u8");
    const auto pos = read_all<float>(dir + "pos.f32"), centers = read_all<float>(dir + "centers.f32"), pool_f32 = read_all<float>(dir + "pool.f32");
    const auto obs_ptr = read_all<int32_t>(dir + "obs_ptr.i32"), obs_kf = read_all<int32_t>(dir + "obs_kf.i32"),
               obs_desc = read_all<int32_t>(dir + "obs_desc.i32");
    const Camera camera(fx, fy, cx, cy, W, H);

    // the frame: both kinds of rows on one object
    ExtractedFeatures ff;
    for (int i = 0; i < N; i++) ff.keypoints.push_back(KeyPoint{Vec2f{kp[2 * i], kp[2 * i + 1]}});
    ff.descriptors = desc; ff.descriptors_f32 = rows; ff.descriptor_dim = dim;
    Frame frame(NKF, std::move(ff));
    Mat4f T;
    for (int i = 0; i < 16; i++) T[i] = pose[i];
    frame.set_pose(T);

    // key frame k holds one keypoint per observation made from it, in the order the points list them; its pose is the identity
    // rotation at the given centre, so that camera_center() returns the centre's floats exactly
    std::vector<ExtractedFeatures> kff((size_t)NKF);
    std::vector<std::vector<std::pair<int, size_t>>> assoc((size_t)NKF);        // (point, keypoint index) per key frame
    for (int p = 0; p < P; p++)
        for (int o = obs_ptr[p]; o < obs_ptr[p + 1]; o++) {
            ExtractedFeatures& f = kff[(size_t)obs_kf[o]];
            const size_t row = (size_t)obs_desc[o];
            assoc[(size_t)obs_kf[o]].emplace_back(p, f.keypoints.size());
            f.keypoints.push_back(KeyPoint{Vec2f{(float)(o % 640), (float)(o / 640)}});
            f.descriptors.insert(f.descriptors.end(), pool_u8.begin() + 32 * row, pool_u8.begin() + 32 * (row + 1));
            f.descriptors_f32.insert(f.descriptors_f32.end(), pool_f32.begin() + dim * row, pool_f32.begin() + dim * (row + 1));
        }
    std::vector<std::shared_ptr<KeyFrame>> kfs;
    for (int k = 0; k < NKF; k++) {
        kff[(size_t)k].descriptor_dim = dim;
        kfs.push_back(std::make_shared<KeyFrame>(Frame(k, std::move(kff[(size_t)k]))));
        Mat4f Tk = identity4();
        Tk[3] = -centers[3 * k]; Tk[7] = -centers[3 * k + 1]; Tk[11] = -centers[3 * k + 2];
        kfs.back()->set_pose(Tk);
    }
    Map map;
    std::unordered_map<const MapPoint*, int> index_of;
    for (int p = 0; p < P; p++) index_of[&map.create_point(Vec3f{pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]})] = p;
    // observation lists keep insertion order: associate point by point, in list order
    {
        std::vector<size_t> next((size_t)NKF, 0);
        for (int p = 0; p < P; p++)
            for (int o = obs_ptr[p]; o < obs_ptr[p + 1]; o++) {
                const size_t k = (size_t)obs_kf[o];
                map.associate(*kfs[k], map[(size_t)p], assoc[k][next[k]++].second);
            }
    }

    std::FILE* out = std::fopen((dir + "out.txt").c_str(), "w");
    if (!out) return 2;
    auto emit = [&](const char* label, const std::vector<MapPointMatch>& m) {
        std::fprintf(out, "%s %zu", label, m.size());
        for (const auto& x : m) std::fprintf(out, " %zu %d", x.keypoint_index, index_of.at(&x.point));
        std::fprintf(out, "\n");
        std::printf("%s: %zu matches\n", label, m.size());
    };
    std::vector<MapPoint*> some;
    for (int p = 0; p < P; p += 2) some.push_back(&map[(size_t)p]);
    some.push_back(nullptr);                                                    // nulls are skipped (:121-123)

    const MapMatcher l2(camera, md_l2, NORM_L2), ham(camera, md_u8, NORM_HAMMING);
    const auto first = l2.match_map(frame, map);
    emit("l2_map", first);
    emit("l2_kf", l2.match_key_frame(frame, map, kfs[(size_t)kf_required].get()));
    emit("l2_fuse", l2.match_for_fuse(frame, some));
    emit("l2_desc", l2.match_descriptors(frame, *kfs[(size_t)kf_required]));
    emit("u8_map", ham.match_map(frame, map));
    emit("u8_desc", ham.match_descriptors(frame, *kfs[(size_t)kf_required]));
    for (const auto& m : first) frame.add_map_match(m);                         // matched keypoints and ineligible points
    emit("l2_map2", l2.match_map(frame, map));
    emit("l2_fuse2", l2.match_for_fuse(frame, some));
    emit("bad_norm", MapMatcher(camera, md_l2, (NormTypes)2).match_map(frame, map));
    std::fclose(out);
    return 0;
}
