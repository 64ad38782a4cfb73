// test_marshal.cpp — integration/reference_shim/rs_marshal.h on its own: no GPU, no librsgpu (rs_pack_pose comes from
// racing-slam_amd/csrc/host.cpp, host code), built with -fsanitize=address,undefined (tests/test_marshal_cpu.py).
// A third set of plain structs and an Access for them (neither the mirror's nor the reference's) instantiates the five
// flatten templates; every output array is compared, element for element, with a restatement written the obvious way:
// std::unordered_map for the ids and a vector of vectors per point.
#include <array>
#include <cstdio>
#include <functional>
#include <memory>
#include <random>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../integration/reference_shim/rs_marshal.h"

namespace {

struct KeyFr;
struct Pt {
    float xyz[3] = {0, 0, 0};
    std::vector<std::pair<KeyFr*, size_t>> obs;
};
struct Fr {
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<std::array<float, 2>> kp;
    std::vector<uint8_t> desc;                                 // kp.size() x 32
    std::vector<Pt*> table;                                    // keypoint -> point or null
    explicit Fr(size_t n, int tag) : kp(n), desc(32 * n), table(n, nullptr)
    {
        for (size_t i = 0; i < n; i++) kp[i] = {(float)(100 * tag) + (float)i, (float)(7 * tag) - 0.5f * (float)i};
        for (size_t i = 0; i < desc.size(); i++) desc[i] = (uint8_t)(31 * tag + 3 * i);
        pose[3] = 0.25f * (float)tag; pose[7] = -1.0f * (float)tag; pose[11] = 2.0f + (float)tag; pose[1] = 0.01f * (float)tag; pose[4] = -0.01f * (float)tag;
    }
    virtual ~Fr() = default;
};
struct KeyFr : Fr { using Fr::Fr; };
struct Cfg { bool optimize; Fr* frame; };

void centre_of(const Fr& f, float out[3]) { out[0] = -f.pose[3]; out[1] = -f.pose[7]; out[2] = -f.pose[11]; }
bool matched(const Fr& f, const Pt& p)
{
    for (const Pt* q : f.table) if (q == &p) return true;
    return false;
}
void match(Fr& f, Pt& p, size_t k) { f.table[k] = &p; }
void observe(KeyFr& kf, Pt& p, size_t k) { p.obs.emplace_back(&kf, k); kf.table[k] = &p; }

struct TestAccess {
    using Point = Pt;
    static void position(const Pt& p, float out[3]) { for (int k = 0; k < 3; k++) out[k] = p.xyz[k]; }
    static void pose_row_major(const Fr& f, float out[16]) { for (int k = 0; k < 16; k++) out[k] = f.pose[k]; }
    static void center(const Fr& f, float out[3]) { centre_of(f, out); }
    static void keypoint(const Fr& f, size_t i, float out[2]) { out[0] = f.kp[i][0]; out[1] = f.kp[i][1]; }
    static bool descriptor_rows(const Fr& f, const uint8_t*& rows, size_t& n) { rows = f.desc.data(); n = f.kp.size(); return true; }
    static size_t n_matches(const Fr& f)
    {
        size_t n = 0;
        for (const Pt* p : f.table) n += p != nullptr;
        return n;
    }
    template <typename Fn> static void for_each_match(const Fr& f, Fn fn)
    {
        for (size_t k = 0; k < f.table.size(); k++) if (f.table[k]) fn(*f.table[k], k);
    }
    template <typename Fn> static void for_each_observation(const Pt& p, Fn fn) { for (const auto& o : p.obs) fn(o.first, o.second); }
    static size_t n_observations(const Pt& p) { return p.obs.size(); }
    static const void* observations_address(const Pt& p) { return p.obs.data(); }
    static bool is_matched(const Fr& f, const Pt& p) { return matched(f, p); }
    static bool is_observed_by(const Pt& p, const KeyFr* kf)
    {
        for (const auto& o : p.obs) if (o.first == kf) return true;
        return false;
    }
};

// ------------------------------------------------------------------ the restatements
rs_marshal::MatchArrays ref_match(const Fr& frame, const std::vector<Pt*>& points, const KeyFr* required)
{
    const size_t P = points.size();
    rs_marshal::MatchArrays m;
    m.pos.assign(3 * P, 0.0f); m.eligible.assign(P, 0); m.obs_ptr.assign(P + 1, 0);
    std::unordered_map<const KeyFr*, int> kf_id;
    std::vector<int> pool_off;
    for (size_t p = 0; p < P; p++) {
        const Pt* mp = points[p];
        bool run = mp != nullptr && !matched(frame, *mp);
        if (run && required != nullptr && !TestAccess::is_observed_by(*mp, required)) run = false;
        m.eligible[p] = run;
        if (mp) for (int k = 0; k < 3; k++) m.pos[3 * p + k] = mp->xyz[k];
        if (run)
            for (const auto& [kf, idx] : mp->obs) {
                auto it = kf_id.find(kf);
                if (it == kf_id.end()) {
                    it = kf_id.emplace(kf, (int)kf_id.size()).first;
                    float c[3];
                    centre_of(*kf, c);
                    m.centers.insert(m.centers.end(), {c[0], c[1], c[2]});
                    pool_off.push_back((int)(m.pool.size() / 32));
                    m.pool.insert(m.pool.end(), kf->desc.begin(), kf->desc.end());
                }
                m.obs_kf.push_back(it->second);
                m.obs_desc.push_back(pool_off[(size_t)it->second] + (int32_t)idx);
            }
        m.obs_ptr[p + 1] = (int32_t)m.obs_kf.size();
    }
    return m;
}

rs_marshal::RefineArrays ref_refine(const Fr& frame)
{
    rs_marshal::RefineArrays r;
    for (size_t k = 0; k < frame.table.size(); k++) {
        const Pt* p = frame.table[k];
        if (!p || p->obs.size() < 2) continue;
        for (int j = 0; j < 3; j++) r.pts.push_back((double)p->xyz[j]);
        r.uv.push_back(frame.kp[k][0]);
        r.uv.push_back(frame.kp[k][1]);
    }
    return r;
}

rs_marshal::BaArrays<Pt> ref_ba(const std::vector<Cfg>& frames)
{
    const size_t C = frames.size();
    rs_marshal::BaArrays<Pt> b;
    b.cams.resize(6 * C); b.cam_free.resize(C);
    for (size_t c = 0; c < C; c++) { rs_pack_pose(frames[c].frame->pose, &b.cams[6 * c]); b.cam_free[c] = frames[c].optimize; }
    std::unordered_map<const Pt*, int> pid;
    for (const auto& fc : frames) {
        if (!fc.optimize) continue;
        for (Pt* p : fc.frame->table) {
            if (!p || p->obs.size() < 2) continue;
            if (pid.emplace(p, (int)b.free_pts.size()).second) b.free_pts.push_back(p);
        }
    }
    const size_t P = b.free_pts.size();
    std::vector<std::vector<std::pair<int, std::array<float, 2>>>> per_point(P);
    for (size_t c = 0; c < C; c++)
        for (size_t k = 0; k < frames[c].frame->table.size(); k++) {
            auto it = pid.find(frames[c].frame->table[k]);
            if (it != pid.end()) per_point[(size_t)it->second].emplace_back((int)c, frames[c].frame->kp[k]);
        }
    b.obs_ptr.assign(P + 1, 0);
    b.pts.resize(3 * P);
    for (size_t p = 0; p < P; p++) {
        for (int k = 0; k < 3; k++) b.pts[3 * p + k] = (double)b.free_pts[p]->xyz[k];
        for (const auto& [c, px] : per_point[p]) { b.obs_cam.push_back(c); b.obs_uv.push_back(px[0]); b.obs_uv.push_back(px[1]); }
        b.obs_ptr[p + 1] = (int32_t)b.obs_cam.size();
    }
    return b;
}

rs_marshal::WindowArrays ref_window(const std::vector<std::shared_ptr<KeyFr>>& key_frames, const Fr& new_frame)
{
    const int n = (int)key_frames.size();
    rs_marshal::WindowArrays w;
    std::unordered_map<const Fr*, int> fid;
    for (int i = 0; i < n; i++) { fid[key_frames[(size_t)i].get()] = i; if (key_frames[(size_t)i].get() == &new_frame) w.new_index = i; }
    std::unordered_map<const Pt*, int> pid;
    std::vector<const Pt*> pts;
    w.frame_ptr.assign((size_t)n + 2, 0);
    auto add = [&](const Fr& f, int slot) {
        for (const Pt* p : f.table) {
            if (!p) continue;
            auto it = pid.find(p);
            if (it == pid.end()) { it = pid.emplace(p, (int)pts.size()).first; pts.push_back(p); }
            w.frame_pt.push_back(it->second);
        }
        w.frame_ptr[(size_t)slot + 1] = (int32_t)w.frame_pt.size();
    };
    for (int i = 0; i < n; i++) add(*key_frames[(size_t)i], i);
    if (w.new_index < 0) add(new_frame, n); else w.frame_ptr[(size_t)n + 1] = w.frame_ptr[(size_t)n];
    w.pt_ptr.assign(pts.size() + 1, 0);
    for (size_t p = 0; p < pts.size(); p++) {
        for (const auto& [kf, idx] : pts[p]->obs) {
            auto it = fid.find(kf);
            if (it != fid.end()) w.pt_obs.push_back(it->second);
        }
        w.pt_ptr[p + 1] = (int32_t)w.pt_obs.size();
    }
    return w;
}

rs_marshal::PointErrorArrays ref_point_errors(const std::vector<Pt*>& points)
{
    rs_marshal::PointErrorArrays e;
    e.obs_ptr = {0};
    std::unordered_map<const KeyFr*, int32_t> pose_row;
    for (const Pt* p : points) {
        for (int k = 0; k < 3; k++) e.pos.push_back(p->xyz[k]);
        for (const auto& [kf, idx] : p->obs) {
            auto it = pose_row.find(kf);
            if (it == pose_row.end()) {
                it = pose_row.emplace(kf, (int32_t)pose_row.size()).first;
                e.poses.insert(e.poses.end(), kf->pose, kf->pose + 16);
            }
            e.obs_pose.push_back(it->second);
            e.uv.push_back(kf->kp[idx][0]);
            e.uv.push_back(kf->kp[idx][1]);
        }
        e.obs_ptr.push_back((int32_t)e.obs_pose.size());
    }
    e.n_poses = (int)pose_row.size();
    return e;
}

// ------------------------------------------------------------------ comparison
int g_failed = 0;
void check(bool ok, const char* what)
{
    if (!ok) { std::printf("FAILED: %s\n", what); g_failed++; }
}
template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b, const char* what, const char* field)
{
    if (a == b) return true;
    std::printf("FAILED: %s: %s differs (%zu vs %zu entries)\n", what, field, a.size(), b.size());
    g_failed++;
    return false;
}
#define SAME(field) ok &= same(a.field, b.field, what, #field)
bool eq(const rs_marshal::MatchArrays& a, const rs_marshal::MatchArrays& b, const char* what)
{
    bool ok = true;
    SAME(pos); SAME(eligible); SAME(obs_ptr); SAME(obs_kf); SAME(obs_desc); SAME(centers); SAME(pool);
    check(!a.refused, what);
    return ok;
}
bool eq(const rs_marshal::RefineArrays& a, const rs_marshal::RefineArrays& b, const char* what)
{
    bool ok = true;
    SAME(pts); SAME(uv);
    return ok;
}
bool eq(const rs_marshal::BaArrays<Pt>& a, const rs_marshal::BaArrays<Pt>& b, const char* what)
{
    bool ok = true;
    SAME(cams); SAME(cam_free); SAME(free_pts); SAME(pts); SAME(obs_ptr); SAME(obs_cam); SAME(obs_uv);
    return ok;
}
bool eq(const rs_marshal::WindowArrays& a, const rs_marshal::WindowArrays& b, const char* what)
{
    bool ok = true;
    SAME(frame_ptr); SAME(frame_pt); SAME(pt_ptr); SAME(pt_obs);
    if (a.new_index != b.new_index) { std::printf("FAILED: %s: new_index %d vs %d\n", what, a.new_index, b.new_index); g_failed++; ok = false; }
    return ok;
}
bool eq(const rs_marshal::PointErrorArrays& a, const rs_marshal::PointErrorArrays& b, const char* what)
{
    bool ok = true;
    SAME(pos); SAME(uv); SAME(poses); SAME(obs_ptr); SAME(obs_pose);
    if (a.n_poses != b.n_poses) { std::printf("FAILED: %s: n_poses %d vs %d\n", what, a.n_poses, b.n_poses); g_failed++; ok = false; }
    return ok;
}
#undef SAME

// A map of n_kf key frames with n_kp keypoints each and n_pt points, every point observed by 0 - 4 key frames.
struct Scene {
    std::vector<std::shared_ptr<KeyFr>> kfs;
    std::vector<std::unique_ptr<Pt>> pts;
    std::vector<Cfg> window;
    Scene(unsigned seed, int n_kf, size_t n_kp, int n_pt)
    {
        std::mt19937 rng(seed);
        for (int k = 0; k < n_kf; k++) kfs.push_back(std::make_shared<KeyFr>(n_kp, k + 1));
        for (int p = 0; p < n_pt; p++) {
            pts.push_back(std::make_unique<Pt>());
            for (int k = 0; k < 3; k++) pts.back()->xyz[k] = (float)(rng() % 1000) * 0.01f;
            const int n_obs = (int)(rng() % 5);
            for (int o = 0; o < n_obs; o++) {
                KeyFr& kf = *kfs[rng() % kfs.size()];
                const size_t k = rng() % n_kp;
                if (kf.table[k] == nullptr && !matched(kf, *pts.back())) observe(kf, *pts.back(), k);
            }
        }
        for (int k = 0; k < n_kf; k++) window.push_back(Cfg{k % 3 != 0, kfs[(size_t)k].get()});
    }
    std::vector<Pt*> points() const
    {
        std::vector<Pt*> v;
        for (const auto& p : pts) v.push_back(p.get());
        return v;
    }
};

void test_bundle_adjust_and_refine()
{
    // frames: fixed, free, free.  a: matched by the fixed and a free frame; b: one observation in total; c: matched only by
    // the fixed frame (two observations, one outside the list); d: first seen in the LAST frame but matched earlier by the
    // fixed one too; e: matched by both free frames
    KeyFr fixed(6, 1), free1(6, 2), free2(6, 3), outside(6, 4);
    Pt a, b, c, d, e;
    Pt* all[] = {&a, &b, &c, &d, &e};
    for (int i = 0; i < 5; i++) for (int k = 0; k < 3; k++) all[i]->xyz[k] = (float)(i + 1) + 0.1f * (float)k;
    observe(free1, e, 0); observe(free1, a, 4); observe(fixed, a, 2);
    observe(free1, b, 1);
    observe(fixed, c, 0); observe(outside, c, 0);
    observe(free2, d, 1); observe(fixed, d, 5);
    observe(free2, e, 3);
    const std::vector<Cfg> frames = {{false, &fixed}, {true, &free1}, {true, &free2}};
    const auto got = rs_marshal::flatten_ba(frames, TestAccess{});
    eq(got, ref_ba(frames), "flatten_ba, fixed + free frames");
    check(got.free_pts == std::vector<Pt*>{&e, &a, &d}, "free points: first-seen order over the optimised frames; b (1 observation) and c (fixed only) left out");
    check(got.obs_ptr == std::vector<int32_t>{0, 2, 4, 6} && got.obs_cam == std::vector<int32_t>{1, 2, 0, 1, 0, 2},
          "every point's slice in frame-list order, the fixed frame included");
    check(got.cam_free == std::vector<uint8_t>{0, 1, 1}, "cam_free");
    const auto r = rs_marshal::flatten_refine(free1, TestAccess{});
    eq(r, ref_refine(free1), "flatten_refine");
    check(r.uv.size() == 4 && r.pts.size() == 6 && r.pts[0] == (double)e.xyz[0] && r.pts[3] == (double)a.xyz[0], "refine: e and a, not b");
}

void test_local_window()
{
    auto k0 = std::make_shared<KeyFr>(5, 1), k1 = std::make_shared<KeyFr>(5, 2), k2 = std::make_shared<KeyFr>(5, 3);
    KeyFr outside(5, 4);
    Fr fresh(5, 5);
    Pt a, b, c;
    observe(*k0, a, 1); observe(outside, a, 0); observe(*k2, a, 4);
    observe(*k1, b, 0); observe(*k2, b, 2);
    observe(outside, c, 3); observe(*k1, c, 3);
    match(fresh, c, 2); match(fresh, a, 0);
    const std::vector<std::shared_ptr<KeyFr>> kfs = {k0, k1, k2};
    const auto among = rs_marshal::flatten_local_window(kfs, static_cast<const Fr&>(*k2), TestAccess{});
    eq(among, ref_window(kfs, *k2), "flatten_local_window, new frame among the key frames");
    check(among.new_index == 2 && among.frame_ptr[4] == among.frame_ptr[3], "new frame among the key frames: its index, empty slot n");
    check(among.pt_obs == std::vector<int32_t>{0, 2, 1, 2, 1}, "an observer outside the list is skipped");
    const auto apart = rs_marshal::flatten_local_window(kfs, fresh, TestAccess{});
    eq(apart, ref_window(kfs, fresh), "flatten_local_window, new frame of its own");
    check(apart.new_index == -1 && apart.frame_ptr[4] == apart.frame_ptr[3] + 2, "new frame of its own: slot n holds its two matches");
}

void test_match()
{
    KeyFr k0(4, 1), k1(4, 2), k2(4, 3);
    Fr frame(4, 9);
    Pt a, b, taken, dead, c;
    a.xyz[0] = 1; b.xyz[1] = 2; taken.xyz[2] = 3; dead.xyz[0] = 4; c.xyz[1] = 5;
    observe(k1, a, 0); observe(k0, a, 3);
    observe(k1, b, 1);
    observe(k0, taken, 0); match(frame, taken, 2);
    observe(k2, c, 2); observe(k0, c, 1);
    const std::vector<Pt*> fuse = {&a, nullptr, &taken, &dead, &b, &a};
    const KeyFr* none = nullptr;
    const auto got = rs_marshal::flatten_match(frame, fuse, none, TestAccess{});
    eq(got, ref_match(frame, fuse, nullptr), "flatten_match, fuse list");
    check(got.eligible == std::vector<uint8_t>{1, 0, 0, 1, 1, 1}, "null and already-matched entries are ineligible, the list order is kept");
    check(got.obs_ptr == std::vector<int32_t>{0, 2, 2, 2, 2, 3, 5} && got.obs_kf == std::vector<int32_t>{0, 1, 0, 0, 1},
          "key-frame ids in first-seen order; a dead point has an empty slice; a point listed twice is flattened twice");
    check(got.pos[3] == 0.0f && got.pos[6 + 2] == 3.0f, "a null entry keeps a zero position, an ineligible one its own");
    const std::vector<Pt*> map = {&a, &b, &taken, &c};
    const KeyFr* required = &k0;
    const auto obs = rs_marshal::flatten_match(frame, map, required, TestAccess{});
    eq(obs, ref_match(frame, map, &k0), "flatten_match, required observer");
    check(obs.eligible == std::vector<uint8_t>{1, 0, 0, 1}, "only the required observer's unmatched points are eligible");
    check(obs.pool.size() == 3 * 4 * 32 && obs.centers.size() == 9, "the pool holds each key frame once (k1, k0, k2)");
}

void test_point_errors()
{
    KeyFr k0(3, 1), k1(3, 2), k2(3, 3);
    Pt a, b, c;
    observe(k2, a, 0); observe(k0, a, 1);
    observe(k0, b, 0);
    observe(k1, c, 2); observe(k2, c, 1); observe(k0, c, 2);
    const std::vector<Pt*> pts = {&a, &b, &c};
    const auto got = rs_marshal::flatten_point_errors(pts, TestAccess{});
    eq(got, ref_point_errors(pts), "flatten_point_errors");
    check(got.n_poses == 3 && got.obs_pose == std::vector<int32_t>{0, 1, 1, 2, 0, 1}, "pose rows in first-seen order: k2, k0, k1");
    check(got.poses[3] == k2.pose[3] && got.poses[16 + 3] == k0.pose[3] && got.poses[32 + 3] == k1.pose[3], "pose table rows");
}

void test_empty_inputs()
{
    Fr bare(0, 1), unmatched(3, 2);
    const KeyFr* none = nullptr;
    const std::vector<Pt*> no_points, nulls = {nullptr, nullptr, nullptr};
    const auto m0 = rs_marshal::flatten_match(bare, no_points, none, TestAccess{});
    check(m0.obs_ptr == std::vector<int32_t>{0} && m0.pos.empty() && m0.pool.empty() && m0.obs_kf.empty(), "flatten_match without points");
    const auto m1 = rs_marshal::flatten_match(unmatched, nulls, none, TestAccess{});
    eq(m1, ref_match(unmatched, nulls, nullptr), "flatten_match, null points only");
    check(m1.obs_ptr == std::vector<int32_t>(4, 0) && m1.eligible == std::vector<uint8_t>(3, 0), "null points only: P + 1 zeros");
    const auto r = rs_marshal::flatten_refine(unmatched, TestAccess{});
    check(r.pts.empty() && r.uv.empty() && rs_marshal::flatten_refine(bare, TestAccess{}).uv.empty(), "flatten_refine without matches");
    const std::vector<Cfg> no_frames, idle = {{true, &unmatched}, {false, &bare}};
    const auto b0 = rs_marshal::flatten_ba(no_frames, TestAccess{});
    check(b0.obs_ptr == std::vector<int32_t>{0} && b0.cams.empty() && b0.free_pts.empty() && b0.obs_cam.empty(), "flatten_ba without frames");
    const auto b1 = rs_marshal::flatten_ba(idle, TestAccess{});
    eq(b1, ref_ba(idle), "flatten_ba, frames without matches");
    check(b1.obs_ptr == std::vector<int32_t>{0} && b1.cams.size() == 12, "frames without matches: no points, two cameras");
    const std::vector<std::shared_ptr<KeyFr>> no_kfs;
    const auto w = rs_marshal::flatten_local_window(no_kfs, unmatched, TestAccess{});
    eq(w, ref_window(no_kfs, unmatched), "flatten_local_window without key frames");
    check(w.new_index == -1 && w.frame_ptr == std::vector<int32_t>{0, 0} && w.pt_ptr == std::vector<int32_t>{0} && w.pt_obs.empty(), "no key frames, no matches");
    const auto e0 = rs_marshal::flatten_point_errors(no_points, TestAccess{});
    check(e0.obs_ptr == std::vector<int32_t>{0} && e0.n_poses == 0 && e0.pos.empty(), "flatten_point_errors without points");
    Pt lonely;
    const std::vector<Pt*> one = {&lonely};
    const auto e1 = rs_marshal::flatten_point_errors(one, TestAccess{});
    eq(e1, ref_point_errors(one), "flatten_point_errors, a point without observations");
    check(e1.obs_ptr == std::vector<int32_t>{0, 0} && e1.poses.empty(), "a point without observations");
}

void test_ptr_index()
{
    using rs_marshal::PtrIndex;
    std::vector<std::array<char, 16>> keys(400);
    {
        PtrIndex first(PtrIndex::POINTS, 1);                    // 64 slots: grows at 32, 64 and 128 keys
        bool grown_ok = true;
        for (int i = 0; i < 200; i++) {
            bool fresh = false;
            grown_ok &= first.find_or_insert(&keys[(size_t)i], i, &fresh) == i && fresh;
        }
        for (int i = 0; i < 200; i++) {
            bool fresh = true;
            grown_ok &= first.find(&keys[(size_t)i]) == i && first.find_or_insert(&keys[(size_t)i], -7, &fresh) == i && !fresh;
            grown_ok &= first.find(&keys[(size_t)(200 + i)]) == -1;
        }
        check(grown_ok, "PtrIndex: 200 keys through three growths, every key found, 200 absent ones not");
    }
    {
        PtrIndex second(PtrIndex::POINTS, 1);                   // same thread, same storage: the generation bump empties it
        bool empty = true;
        for (int i = 0; i < 200; i++) empty &= second.find(&keys[(size_t)i]) == -1;
        check(empty, "PtrIndex: a second table on the same thread sees none of the first one's keys");
        PtrIndex frames(PtrIndex::FRAMES, 1);                   // the other table is alive at the same time (build_local_window)
        bool fresh = false;
        frames.find_or_insert(&keys[0], 5, &fresh);
        second.find_or_insert(&keys[1], 6, &fresh);
        check(frames.find(&keys[0]) == 5 && frames.find(&keys[1]) == -1 && second.find(&keys[1]) == 6 && second.find(&keys[0]) == -1,
              "PtrIndex: the point and the frame table do not share storage");
    }
}

void test_scenes_and_threads()
{
    // larger random maps against the restatements, every function
    const Scene s1(1, 7, 40, 150), s2(2, 11, 64, 400);
    for (const Scene* s : {&s1, &s2}) {
        const auto pts = s->points();
        const KeyFr* required = s->kfs[1].get();
        const KeyFr* none = nullptr;
        Fr probe(8, 20);
        match(probe, *pts[3], 1); match(probe, *pts[10], 6);
        eq(rs_marshal::flatten_match(probe, pts, none, TestAccess{}), ref_match(probe, pts, nullptr), "scene: flatten_match");
        eq(rs_marshal::flatten_match(probe, pts, required, TestAccess{}), ref_match(probe, pts, required), "scene: flatten_match, observer");
        eq(rs_marshal::flatten_refine(*s->kfs[0], TestAccess{}), ref_refine(*s->kfs[0]), "scene: flatten_refine");
        eq(rs_marshal::flatten_ba(s->window, TestAccess{}), ref_ba(s->window), "scene: flatten_ba");
        const std::vector<std::shared_ptr<KeyFr>> some(s->kfs.begin() + 1, s->kfs.end() - 1);
        eq(rs_marshal::flatten_local_window(some, static_cast<const Fr&>(*s->kfs.back()), TestAccess{}), ref_window(some, *s->kfs.back()), "scene: flatten_local_window");
        eq(rs_marshal::flatten_local_window(s->kfs, static_cast<const Fr&>(*s->kfs[2]), TestAccess{}), ref_window(s->kfs, *s->kfs[2]), "scene: flatten_local_window, among");
        eq(rs_marshal::flatten_point_errors(pts, TestAccess{}), ref_point_errors(pts), "scene: flatten_point_errors");
    }
    // two threads, each flattening its own map at the same time: the same arrays as alone (thread_local table storage)
    const auto alone1 = rs_marshal::flatten_ba(s1.window, TestAccess{}), alone2 = rs_marshal::flatten_ba(s2.window, TestAccess{});
    int differ[2] = {0, 0};
    auto run = [](const Scene& s, const rs_marshal::BaArrays<Pt>& want, int* n) {
        for (int i = 0; i < 50; i++) {
            const auto b = rs_marshal::flatten_ba(s.window, TestAccess{});
            if (b.free_pts != want.free_pts || b.obs_ptr != want.obs_ptr || b.obs_cam != want.obs_cam || b.obs_uv != want.obs_uv ||
                b.pts != want.pts || b.cams != want.cams || b.cam_free != want.cam_free)
                ++*n;
        }
    };
    std::thread t1(run, std::cref(s1), std::cref(alone1), &differ[0]), t2(run, std::cref(s2), std::cref(alone2), &differ[1]);
    t1.join(); t2.join();
    check(differ[0] == 0 && differ[1] == 0, "flatten_ba on two threads at once gives each the arrays it gets alone");
}

}  // namespace

int main()
{
    test_bundle_adjust_and_refine();
    test_local_window();
    test_match();
    test_point_errors();
    test_empty_inputs();
    test_ptr_index();
    test_scenes_and_threads();
    if (g_failed) { std::printf("%d marshal checks FAILED\n", g_failed); return 1; }
    std::printf("marshal checks passed\n");
    return 0;
}
