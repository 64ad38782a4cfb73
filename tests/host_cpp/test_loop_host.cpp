// test_loop_host.cpp — drives slam::LoopStreak (racing-slam_amd/host), the host-side form of LoopDetector::Impl's streak
// and constraints (update_streak, consume_new_loop, constraints), over scripted queries.  No GPU is touched.
//
//     test_loop_host <script> <out>
// <script>: one query per line, "from n" followed by n triples "candidate_index ok inliers"; every verified candidate
// carries the pose and the candidate pose written below and `inliers` listed pairs (k, 100 + k).  <out>: per query
// "chosen new_loop streak_length", then per constraint "from to pairs" and its 16 relative entries (%.17g).
// tests/test_loop_host.py compares them with tests/loop_ref.py.
#include <cstdio>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::printf("usage: test_loop_host <script> <out>\n"); return 2; }
    FILE* in = std::fopen(argv[1], "r");
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) { std::printf("cannot open files\n"); return 2; }
    float pose[16], cand[16];
    for (float& v : pose) if (std::fscanf(in, "%f", &v) != 1) return 2;
    for (float& v : cand) if (std::fscanf(in, "%f", &v) != 1) return 2;
    slam::LoopStreak streak;
    long from = 0;
    int n = 0;
    while (std::fscanf(in, "%ld %d", &from, &n) == 2) {
        std::vector<slam::LoopCandidate> ranked((size_t)n);
        std::vector<slam::LoopVerification> ver((size_t)n);
        std::vector<slam::Mat4f> poses((size_t)n);
        for (int i = 0; i < n; i++) {
            long index = 0;
            int ok = 0, inliers = 0;
            if (std::fscanf(in, "%ld %d %d", &index, &ok, &inliers) != 3) return 2;
            ranked[(size_t)i].entry = (size_t)index;
            ver[(size_t)i].result.ok = ok;
            ver[(size_t)i].result.inliers = inliers;
            ver[(size_t)i].result.listed = inliers;
            for (int k = 0; k < 16; k++) { ver[(size_t)i].result.pose[k] = pose[k]; poses[(size_t)i][(size_t)k] = cand[k]; }
            for (int k = 0; k < inliers; k++) { ver[(size_t)i].query_kp.push_back(k); ver[(size_t)i].point.push_back(100 + k); }
        }
        const int chosen = streak.update((size_t)from, ranked, ver, poses);
        std::fprintf(out, "%d %d %zu\n", chosen, streak.consume_new_loop() ? 1 : 0, streak.streak_length());
    }
    for (const auto& c : streak.constraints()) {
        std::fprintf(out, "%zu %zu %zu", c.from, c.to, c.inlier_matches.size());
        for (double v : c.relative) std::fprintf(out, " %.17g", v);
        std::fprintf(out, "\n");
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
