// test_trackstore_host.cpp — slam::DeviceTracks (rs_track_store behind the host mirror) against slam::HostTrackStore, the
// std::map restatement of TrackStore, from C++:
//     test_trackstore_host            a 30-frame synthetic sequence with two key frames: after every frame the device
//                                     store, downloaded, equals the std::map (ids, keypoints, counts, sightings bit for
//                                     bit), the query's waiting / live counts equal the host's, and on the key frames
//                                     DeviceTracks::triangulate_tracks equals rs_triangulate_tracks on the CSR built
//                                     from the std::map, key-frame sightings included.  Prints "trackstore host ok: <checks>".
//     test_trackstore_host --time R   the timing of tools/trackstore_time.py: both forms in this one process, one JSON line.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../racing-slam_amd/host/slam_host.h"

static int g_checks = 0, g_bad = 0;
static void expect_true(bool ok, const char* what, int frame)
{
    g_checks++;
    if (!ok) { g_bad++; std::printf("frame %d: %s\n", frame, what); }
}

template <class T> static T* dev_copy(const std::vector<T>& v, size_t room = 0)
{
    T* d = nullptr;
    if (hipMalloc((void**)&d, sizeof(T) * std::max<size_t>(std::max(room, v.size()), 1)) != hipSuccess) { std::printf("hipMalloc failed\n"); std::exit(2); }
    if (!v.empty() && hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) { std::printf("upload failed\n"); std::exit(2); }
    return d;
}

// static points in front of a camera moving along x: keypoint i of frame f is point i
struct Scene {
    int n = 0, frames = 0;
    std::vector<std::vector<float>> pix;         // [frames][n][2]
    std::vector<float> poses;                    // [frames][16]
    std::vector<std::vector<int32_t>> inliers;   // [frames] ascending, about `keep` of the keypoints
    slam::Camera camera{1000.f, 1000.f, 960.f, 540.f, 1920, 1080};
    Scene(int n_, int frames_, double keep, unsigned seed) : n(n_), frames(frames_)
    {
        std::mt19937 rng(seed);
        std::uniform_real_distribution<float> ux(-4.f, 4.f), uy(-2.f, 2.f), uz(4.f, 9.f), u01(0.f, 1.f);
        std::vector<float> X(3 * (size_t)n);
        for (int i = 0; i < n; i++) { X[3 * i] = ux(rng); X[3 * i + 1] = uy(rng); X[3 * i + 2] = uz(rng); }
        pix.resize(frames); inliers.resize(frames); poses.assign(16 * (size_t)frames, 0.f);
        for (int f = 0; f < frames; f++) {
            const float c = 0.1f * f;
            float* P = &poses[16 * (size_t)f];
            P[0] = P[5] = P[10] = P[15] = 1.f; P[3] = -c;
            pix[f].resize(2 * (size_t)n);
            for (int i = 0; i < n; i++) {
                pix[f][2 * i] = 1000.f * (X[3 * i] - c) / X[3 * i + 2] + 960.f;
                pix[f][2 * i + 1] = 1000.f * X[3 * i + 1] / X[3 * i + 2] + 540.f;
                if (u01(rng) < keep) inliers[f].push_back(i);
            }
        }
    }
};

// rs_triangulate_tracks' inputs from the std::map, in id order (what Mapper_triangulate_tracks.inc builds on the host)
struct HostCsr {
    std::vector<float> track_uv, sight_uv;
    std::vector<uint8_t> skip;
    std::vector<int32_t> sight_ptr, sight_pose;
    std::vector<uint64_t> ids;
    void build(const slam::HostTrackStore& st, const float* kp, const int32_t* table, int n, int pose_base, int n_poses)
    {
        track_uv.clear(); sight_uv.clear(); skip.clear(); sight_ptr.assign(1, 0); sight_pose.clear(); ids.clear();
        for (const auto& [id, t] : st.tracks()) {
            const bool has = t.keypoint_index < (size_t)n;
            bool sk = !has || table[t.keypoint_index] >= 0;
            track_uv.push_back(has ? kp[2 * t.keypoint_index] : 0.f);
            track_uv.push_back(has ? kp[2 * t.keypoint_index + 1] : 0.f);
            for (const auto& s : t.sightings) {
                const int p = s.frame_index - pose_base;
                sk = sk || p < 0 || p >= n_poses;
                sight_pose.push_back(p);
                sight_uv.push_back(s.pixel.x); sight_uv.push_back(s.pixel.y);
            }
            sight_ptr.push_back((int32_t)sight_pose.size());
            skip.push_back(sk ? 1 : 0);
            ids.push_back(id);
        }
    }
};

// device buffers of the host form's rs_triangulate_tracks call, made once
struct HostTriangulation {
    int cap = 0;
    float *d_uv = nullptr, *d_suv = nullptr, *d_xyz = nullptr, *d_pc = nullptr, *d_rc = nullptr;
    uint8_t *d_skip = nullptr, *d_status = nullptr;
    int32_t *d_ptr = nullptr, *d_pose = nullptr, *d_acc = nullptr, *d_inc = nullptr, *d_counts = nullptr;
    std::vector<int32_t> accepted, inconsistent;
    std::vector<float> xyz;
    int32_t counts[3] = {0, 0, 0};
    HostTriangulation(const HostTriangulation&) = delete;
    ~HostTriangulation()
    {
        for (void* d : {(void*)d_uv, (void*)d_suv, (void*)d_xyz, (void*)d_pc, (void*)d_rc, (void*)d_skip, (void*)d_status, (void*)d_ptr,
                        (void*)d_pose, (void*)d_acc, (void*)d_inc, (void*)d_counts})
            (void)hipFree(d);
    }
    HostTriangulation(int max_tracks, int max_sightings) : cap(max_tracks)
    {
        const size_t T = (size_t)max_tracks, S = T * (size_t)max_sightings;
        d_uv = dev_copy(std::vector<float>(), 2 * T); d_suv = dev_copy(std::vector<float>(), 2 * S); d_xyz = dev_copy(std::vector<float>(), 3 * T);
        d_pc = dev_copy(std::vector<float>(), T); d_rc = dev_copy(std::vector<float>(), T);
        d_skip = dev_copy(std::vector<uint8_t>(), T); d_status = dev_copy(std::vector<uint8_t>(), T);
        d_ptr = dev_copy(std::vector<int32_t>(), T + 1); d_pose = dev_copy(std::vector<int32_t>(), S);
        d_acc = dev_copy(std::vector<int32_t>(), T); d_inc = dev_copy(std::vector<int32_t>(), T); d_counts = dev_copy(std::vector<int32_t>(), 4);
        accepted.resize(T); inconsistent.resize(T); xyz.resize(3 * T);
    }
    bool run(rs_context* ctx, const HostCsr& c, const float* d_poses, int n_poses, int kf_pose, const slam::Camera& cam)
    {
        const size_t T = c.skip.size(), S = c.sight_pose.size();
        if (T == 0) { counts[0] = counts[1] = counts[2] = 0; return true; }
        bool ok = hipMemcpyAsync(d_uv, c.track_uv.data(), 8 * T, hipMemcpyHostToDevice, 0) == hipSuccess &&
                  hipMemcpyAsync(d_skip, c.skip.data(), T, hipMemcpyHostToDevice, 0) == hipSuccess &&
                  hipMemcpyAsync(d_ptr, c.sight_ptr.data(), 4 * (T + 1), hipMemcpyHostToDevice, 0) == hipSuccess &&
                  hipMemcpyAsync(d_pose, c.sight_pose.data(), 4 * S, hipMemcpyHostToDevice, 0) == hipSuccess &&
                  hipMemcpyAsync(d_suv, c.sight_uv.data(), 8 * S, hipMemcpyHostToDevice, 0) == hipSuccess;
        const float K[4] = {cam.fx(), cam.fy(), cam.cx(), cam.cy()};
        ok = ok && rs_triangulate_tracks(ctx, (int)T, d_uv, d_skip, d_ptr, d_pose, d_suv, d_poses, n_poses, kf_pose, K, 1.0f, 4.0f, 0.999848f, 0.20f, 100,
                                         d_status, d_xyz, d_pc, d_rc, d_acc, d_inc, d_counts, nullptr) == RS_OK;
        ok = ok && hipMemcpy(counts, d_counts, 12, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(accepted.data(), d_acc, 4 * T, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(inconsistent.data(), d_inc, 4 * T, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(xyz.data(), d_xyz, 12 * T, hipMemcpyDeviceToHost) == hipSuccess;
        return ok;
    }
};

static bool same_store(rs_context* ctx, const slam::DeviceTracks& dev, const slam::HostTrackStore& host, int cap, int max_s)
{
    std::vector<uint64_t> id((size_t)cap);
    std::vector<int32_t> kp((size_t)cap), cnt((size_t)cap), sg(5 * (size_t)cap * max_s);
    int n = -1;
    uint64_t next = 0;
    if (rs_track_store_download(ctx, dev.store(), &n, &next, id.data(), kp.data(), cnt.data(), sg.data()) != RS_OK) return false;
    if ((size_t)n != host.tracks().size() || next != host.next_id()) return false;
    size_t t = 0;
    for (const auto& [hid, tr] : host.tracks()) {
        if (id[t] != hid || (size_t)kp[t] != tr.keypoint_index || (size_t)cnt[t] != tr.sightings.size()) return false;
        for (size_t s = 0; s < tr.sightings.size(); s++) {
            const int32_t* w = &sg[5 * (t * (size_t)max_s + s)];
            const slam::StoredSighting& h = tr.sightings[s];
            if (w[0] != h.frame_index || memcmp(&w[1], &h.pixel.x, 4) || memcmp(&w[2], &h.pixel.y, 4) || w[3] != h.key_frame || w[4] != h.keypoint_index)
                return false;
        }
        t++;
    }
    return true;
}

static int run_sequence(rs_context* ctx)
{
    const int n = 400, F = 30, cap = 512, max_s = 12;
    Scene sc(n, F, 0.8, 7);
    for (int i = 150; i < 170; i++) { sc.pix[7][2 * i] += 30.f; sc.pix[17][2 * i + 1] += 30.f; }      // bad sightings: inconsistent tracks
    slam::DeviceTracks dev(ctx, cap, max_s);
    slam::HostTrackStore host;
    if (!dev.valid()) return 2;
    std::vector<int32_t> ident((size_t)n);
    for (int i = 0; i < n; i++) ident[i] = i;
    int32_t* d_prev = dev_copy(ident);
    float* d_poses = dev_copy(sc.poses);
    HostTriangulation ht(cap, max_s);
    HostCsr csr;
    std::vector<uint8_t> desc(32 * (size_t)n, 0);
    std::mt19937 rng(3);
    int key_frames = 0, last_kf_frame = 0;
    for (int f = 0; f < F; f++) {
        rs_frame* fr = nullptr;
        if (rs_frame_create(ctx, sc.pix[f].data(), desc.data(), n, &fr) != RS_OK) return 2;
        std::vector<int32_t> table((size_t)n, -1), mk, mp;
        for (int i = 0; i < n; i++)
            if (rng() % 4 == 0 && !(i >= 150 && i < 170)) { table[i] = (int32_t)mk.size(); mk.push_back(i); mp.push_back(table[i]); }
        int32_t *d_mk = dev_copy(mk), *d_mp = dev_copy(mp);
        expect_true(rs_frame_matches_add(ctx, fr, d_mk, d_mp, nullptr, (int)mk.size()) == RS_OK, "matches_add", f);
        if (f > 0) {
            std::vector<int32_t> inl = sc.inliers[f];
            for (int i = 150; i < 170; i++) if (!std::binary_search(inl.begin(), inl.end(), i)) inl.push_back(i);
            std::sort(inl.begin(), inl.end());
            const int32_t cnt = (int32_t)inl.size();
            inl.resize((size_t)n, 0);
            int32_t* d_inl = dev_copy(inl);
            int32_t* d_cnt = dev_copy(std::vector<int32_t>(1, cnt));
            expect_true(dev.carry_forward(d_prev, d_inl, d_cnt, n), "carry_forward", f);
            host.carry_forward(ident.data(), inl.data(), cnt, n, (size_t)cap);
            expect_true(same_store(ctx, dev, host, cap, max_s), "the store differs after carry_forward", f);
            (void)hipFree(d_inl); (void)hipFree(d_cnt);
        }
        bool need = false;
        int32_t q[6];
        expect_true(dev.needs_key_frame(nullptr, fr, -1, f - last_kf_frame, 300, &need, q), "needs_key_frame", f);
        expect_true((size_t)q[2] == host.unmapped_tracks(table.data(), (size_t)n) && (size_t)q[3] == host.tracks().size() && q[1] == (int)mk.size(),
                    "the query's counts differ from the host's", f);
        expect_true(need, "no map: nothing is covisible, a key frame is needed", f);
        const bool key_frame = f == 0 || f == 10 || f == 20;
        if (key_frame && f > 0) {
            const int base = 0, n_poses = f + 1;         // every frame so far: Trajectory::pose_at
            slam::DeviceTrackSelection sel;
            expect_true(dev.triangulate_tracks(fr, d_poses + 16 * (size_t)base, n_poses, base, n_poses - 1, sc.camera, nullptr, &sel), "triangulate_tracks", f);
            csr.build(host, sc.pix[f].data(), table.data(), n, base, n_poses);
            expect_true(ht.run(ctx, csr, d_poses + 16 * (size_t)base, n_poses, n_poses - 1, sc.camera), "host rs_triangulate_tracks", f);
            bool same = (int)sel.selection.accepted.size() == ht.counts[0] && (int)sel.selection.topped_up == ht.counts[1] &&
                        (int)sel.selection.inconsistent.size() == ht.counts[2] && sel.tracks == csr.ids.size();
            auto it = host.tracks().begin();
            std::vector<const slam::StoredTrack*> by_pos;
            for (; it != host.tracks().end(); ++it) by_pos.push_back(&it->second);
            for (int a = 0; same && a < ht.counts[0]; a++) {
                const size_t t = (size_t)ht.accepted[a];
                const slam::tracks::Candidate& c = sel.selection.accepted[a];
                same = c.track == t && c.keypoint_index == by_pos[t]->keypoint_index && !memcmp(&c.position, &ht.xyz[3 * t], 12) &&
                       sel.sightings[a] == by_pos[t]->sightings.size();
                std::vector<slam::KeyFrameSighting> want;
                for (const auto& s : by_pos[t]->sightings) if (s.key_frame >= 0) want.push_back({s.key_frame, s.keypoint_index});
                same = same && want.size() == sel.key_frame_sightings[a].size();
                for (size_t i = 0; same && i < want.size(); i++)
                    same = want[i].key_frame == sel.key_frame_sightings[a][i].key_frame && want[i].keypoint_index == sel.key_frame_sightings[a][i].keypoint_index;
            }
            for (int i = 0; same && i < ht.counts[2]; i++) same = sel.selection.inconsistent[i] == (size_t)ht.inconsistent[i];
            expect_true(same, "triangulate_tracks differs from rs_triangulate_tracks on the host-built CSR", f);
            expect_true(ht.counts[0] >= 100 && ht.counts[2] >= 10, "the key frame accepted or erased too little to test anything", f);
            expect_true(dev.erase_inconsistent(), "erase_inconsistent", f);
            for (int i = 0; i < ht.counts[2]; i++) host.erase(csr.ids[(size_t)ht.inconsistent[i]]);
            expect_true(same_store(ctx, dev, host, cap, max_s), "the store differs after erase", f);
        }
        if (key_frame) { key_frames++; last_kf_frame = f; }
        expect_true(dev.extend(fr, f, key_frame ? key_frames - 1 : -1), "extend", f);
        host.extend(sc.pix[f].data(), (size_t)n, f, key_frame ? key_frames - 1 : -1, (size_t)max_s);
        expect_true(same_store(ctx, dev, host, cap, max_s), "the store differs after extend", f);
        (void)hipFree(d_mk); (void)hipFree(d_mp);
        rs_frame_destroy(fr);
    }
    expect_true(host.next_id() > (uint64_t)2 * n, "no churn", F);
    (void)hipFree(d_prev); (void)hipFree(d_poses);
    std::printf("trackstore host ok: %d\n", g_checks);
    return g_bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- timing
static double median_us(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
template <class F> static double timed(rs_context* ctx, int reps, F&& fn)
{
    for (int i = 0; i < 10; i++) fn();
    std::vector<double> us;
    for (int i = 0; i < reps; i++) {
        rs_context_synchronize(ctx);
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        rs_context_synchronize(ctx);
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    return median_us(us);
}

static int run_timing(rs_context* ctx, int reps)
{
    std::string json = "{\"reps\": " + std::to_string(reps) + ", \"max_sightings\": 100, \"sizes\": {";
    const int sizes[2] = {2000, 8192};
    for (int si = 0; si < 2; si++) {
        const int n = sizes[si], F = 14, max_s = 100;
        Scene sc(n, F, 0.7, 100 + si);
        slam::DeviceTracks dev(ctx, 8192, max_s);
        slam::HostTrackStore host;
        std::vector<int32_t> ident((size_t)n);
        for (int i = 0; i < n; i++) ident[i] = i;
        int32_t* d_prev = dev_copy(ident);
        float* d_poses = dev_copy(sc.poses);
        std::vector<uint8_t> desc(32 * (size_t)n, 0);
        std::vector<rs_frame*> fr((size_t)F);
        std::vector<int32_t*> d_inl((size_t)F), d_cnt((size_t)F);
        std::vector<float*> d_kp((size_t)F);
        std::vector<int32_t> table((size_t)n, -1), mk, mp;
        for (int i = 0; i < n; i += 3) { table[i] = i / 3; mk.push_back(i); mp.push_back(i / 3); }
        int32_t *d_mk = dev_copy(mk), *d_mp = dev_copy(mp), *d_table = dev_copy(table);
        for (int f = 0; f < F; f++) {
            if (rs_frame_create(ctx, sc.pix[f].data(), desc.data(), n, &fr[f]) != RS_OK) return 2;
            rs_frame_matches_add(ctx, fr[f], d_mk, d_mp, nullptr, (int)mk.size());
            std::vector<int32_t> inl = sc.inliers[f];
            d_cnt[f] = dev_copy(std::vector<int32_t>(1, (int32_t)inl.size()));
            inl.resize((size_t)n, 0);
            d_inl[f] = dev_copy(inl);
            d_kp[f] = dev_copy(sc.pix[f]);
        }
        dev.extend(fr[0], 0, 0);
        host.extend(sc.pix[0].data(), (size_t)n, 0, 0, max_s);
        for (int f = 1; f < F - 1; f++) {
            dev.carry_forward(d_prev, d_inl[f], d_cnt[f], n);
            dev.extend(fr[f], f, f % 5 == 0 ? f / 5 : -1);
            host.carry_forward(ident.data(), sc.inliers[f].data(), (int)sc.inliers[f].size(), n);
            host.extend(sc.pix[f].data(), (size_t)n, f, f % 5 == 0 ? f / 5 : -1, max_s);
        }
        // the key-frame chains first, on the store as built: frame F - 1 is the key frame
        bool need;
        int32_t q[6];
        dev.needs_key_frame(nullptr, fr[F - 1], -1, 1, 100, &need, q);
        slam::DeviceTrackSelection sel;
        // (timed without the Selection's vectors: the host form below returns raw arrays too; one call fills `sel` for the check)
        dev.triangulate_tracks(fr[F - 1], d_poses, F, 0, F - 1, sc.camera, nullptr, &sel);
        const double kf_dev = timed(ctx, reps, [&] { dev.triangulate_tracks(fr[F - 1], d_poses, F, 0, F - 1, sc.camera, nullptr, nullptr); dev.erase_inconsistent(); });
        HostTriangulation ht(8192, max_s);
        HostCsr csr;
        double build_us = 0;
        const double kf_host = timed(ctx, reps, [&] {
            const auto t0 = std::chrono::steady_clock::now();
            csr.build(host, sc.pix[F - 1].data(), table.data(), n, 0, F);
            build_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            ht.run(ctx, csr, d_poses, F, F - 1, sc.camera);
            for (int i = 0; i < ht.counts[2]; i++) host.erase(csr.ids[(size_t)ht.inconsistent[i]]);
        });
        const bool same_kf = (int)sel.selection.accepted.size() == ht.counts[0] && q[3] == (int)host.tracks().size();
        // the per-frame chains, both cycling through the same frames
        int fd = F - 2, fh = F - 2;
        const double fr_dev = timed(ctx, reps, [&] {
            fd = fd % (F - 1) + 1;
            dev.carry_forward(d_prev, d_inl[fd], d_cnt[fd], n);
            dev.needs_key_frame(nullptr, fr[fd], -1, 1, 100, &need, q);
            dev.extend(fr[fd], 100 + fd, -1);
        });
        std::vector<int32_t> h_prev((size_t)n), h_inl((size_t)n), h_table((size_t)n);
        std::vector<float> h_kp(2 * (size_t)n);
        size_t waiting = 0;
        const double fr_host = timed(ctx, reps, [&] {
            fh = fh % (F - 1) + 1;
            int32_t c = 0;
            (void)hipMemcpy(&c, d_cnt[fh], 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(h_prev.data(), d_prev, 4 * (size_t)n, hipMemcpyDeviceToHost);
            (void)hipMemcpy(h_inl.data(), d_inl[fh], 4 * (size_t)c, hipMemcpyDeviceToHost);
            (void)hipMemcpy(h_kp.data(), d_kp[fh], 8 * (size_t)n, hipMemcpyDeviceToHost);
            (void)hipMemcpy(h_table.data(), d_table, 4 * (size_t)n, hipMemcpyDeviceToHost);
            host.carry_forward(h_prev.data(), h_inl.data(), c, n);
            waiting = host.unmapped_tracks(h_table.data(), (size_t)n);
            host.extend(h_kp.data(), (size_t)n, 100 + fh, -1, max_s);
        });
        char buf[1024];
        std::snprintf(buf, sizeof buf,
                      "%s\"%d\": {\"live_after_carry\": %d, \"accepted\": %d, \"accepted_device\": %zu, \"same_result\": %s, "
                      "\"frame_chain_device_us\": %.1f, \"frame_chain_host_us\": %.1f, \"key_frame_chain_device_us\": %.1f, "
                      "\"key_frame_chain_host_us\": %.1f, \"host_csr_build_us\": %.1f, \"waiting\": %zu}",
                      si ? ", " : "", n, q[3], ht.counts[0], sel.key_frame_sightings.size(), same_kf ? "true" : "false", fr_dev, fr_host, kf_dev,
                      kf_host, build_us, waiting);
        json += buf;
        for (int f = 0; f < F; f++) { rs_frame_destroy(fr[f]); (void)hipFree(d_inl[f]); (void)hipFree(d_cnt[f]); (void)hipFree(d_kp[f]); }
        for (void* d : {(void*)d_prev, (void*)d_poses, (void*)d_mk, (void*)d_mp, (void*)d_table}) (void)hipFree(d);
    }
    std::printf("%s}}\n", json.c_str());
    return 0;
}

int main(int argc, char** argv)
{
    rs_context* ctx = nullptr;
    if (rs_context_create(0, &ctx) != RS_OK) { std::printf("no context\n"); return 2; }
    const int rc = (argc > 2 && !strcmp(argv[1], "--time")) ? run_timing(ctx, std::max(atoi(argv[2]), 1)) : run_sequence(ctx);
    rs_context_destroy(ctx);
    return rc;
}
