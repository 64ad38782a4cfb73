// test_bow_host.cpp — drives slam::LoopRetrieval (racing-slam_amd/host), the host-side form of LoopDetector::query's "Loop
// retrieval" stage (score_candidates + rank_candidates), and the vocabulary's text loader.
//
//     test_bow_host <dir>
// reads <dir>/voc.txt (DBoW2's text format, written by tests/bow_ref.py), meta.txt ("key_frames rows seconds_per_frame"),
// frames.i64 ([key_frames] frame indices), counts.i32 ([key_frames]) and desc.u8 ([key_frames][rows][32]).  Every key
// frame is added and queried in turn.  Writes <dir>/out.txt: one line per key frame, "q count" and count pairs "entry
// score" (hexadecimal f32 bits); and the vocabulary as loaded: info.txt (k L weighting scoring nodes words),
// parent.i32, nodes.u8, weight.f64.  tests/test_bow_host.py compares them with tests/bow_ref.py.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

template <typename T>
static bool read_file(const std::string& path, std::vector<T>& out, size_t count)
{
    std::ifstream f(path, std::ios::binary);
    out.resize(count);
    const std::streamsize bytes = (std::streamsize)(sizeof(T) * count);
    return f && (count == 0 || (f.read((char*)out.data(), bytes) && f.gcount() == bytes));
}

template <typename T>
static bool write_file(const std::string& path, const std::vector<T>& v)
{
    std::ofstream f(path, std::ios::binary);
    return (bool)f.write((const char*)v.data(), (std::streamsize)(sizeof(T) * v.size()));
}

static uint32_t bits(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: test_bow_host <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int n_kf = 0, rows = 0;
    float spf = 0.f;
    FILE* m = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!m || std::fscanf(m, "%d %d %f", &n_kf, &rows, &spf) != 3 || n_kf < 1 || rows < 1) { std::printf("bad meta.txt\n"); return 2; }
    std::fclose(m);
    std::vector<int64_t> frames;
    std::vector<int32_t> counts;
    std::vector<uint8_t> desc;
    if (!read_file(dir + "/frames.i64", frames, (size_t)n_kf) || !read_file(dir + "/counts.i32", counts, (size_t)n_kf) ||
        !read_file(dir + "/desc.u8", desc, (size_t)n_kf * rows * 32)) {
        std::printf("bad input files\n");
        return 2;
    }
    slam::LoopRetrieval loops(dir + "/voc.txt", (size_t)n_kf, (size_t)n_kf * rows, spf);
    if (!loops.valid()) { std::printf("no LoopRetrieval\n"); return 1; }
    // the vocabulary as loaded
    int32_t info[6];
    if (rs_vocabulary_info(loops.vocabulary(), info) != RS_OK) return 1;
    std::vector<int32_t> parent((size_t)info[4]);
    std::vector<uint8_t> nodes(32 * (size_t)info[4]);
    std::vector<double> weight((size_t)info[4]);
    if (rs_vocabulary_arrays(loops.vocabulary(), parent.data(), nodes.data(), weight.data()) != RS_OK) return 1;
    FILE* fi = std::fopen((dir + "/info.txt").c_str(), "w");
    if (!fi) return 2;
    std::fprintf(fi, "%d %d %d %d %d %d\n", info[0], info[1], info[2], info[3], info[4], info[5]);
    std::fclose(fi);
    if (!write_file(dir + "/parent.i32", parent) || !write_file(dir + "/nodes.u8", nodes) || !write_file(dir + "/weight.f64", weight)) return 2;
    // the key frames' rows and counts, on the device as rs_describe_features leaves them
    uint8_t* d_desc = nullptr;
    int32_t* d_counts = nullptr;
    if (hipMalloc(&d_desc, desc.size()) != hipSuccess || hipMalloc(&d_counts, 4 * counts.size()) != hipSuccess ||
        hipMemcpy(d_desc, desc.data(), desc.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_counts, counts.data(), 4 * counts.size(), hipMemcpyHostToDevice) != hipSuccess) {
        std::printf("device buffers failed\n");
        return 1;
    }
    FILE* o = std::fopen((dir + "/out.txt").c_str(), "w");
    if (!o) return 2;
    size_t found = 0;
    for (int q = 0; q < n_kf; q++) {
        if (!loops.add_key_frame(d_desc + (size_t)q * rows * 32, d_counts + q, rows, (size_t)frames[q])) { std::printf("add_key_frame %d failed\n", q); return 1; }
        const auto ranked = loops.query();
        std::fprintf(o, "%d %zu", q, ranked.size());
        for (const auto& c : ranked) std::fprintf(o, " %zu %08x", c.entry, bits(c.score));
        std::fprintf(o, "\n");
        found += ranked.size();
    }
    std::fclose(o);
    (void)hipFree(d_desc);
    (void)hipFree(d_counts);
    std::printf("LoopRetrieval: %d key frames, %zu ranked candidates\n", n_kf, found);
    return 0;
}
