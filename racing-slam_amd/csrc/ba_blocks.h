// ba_blocks.h — the per-call blocks of the bundle-adjustment driver and of refine_pose as layouts on rs_carve (carve.h): each
// function is the ONE statement of a block's pieces, run on a null carver to size and on the block to place.  Host code, no
// HIP call: tests/host_cpp/test_ba_blocks.cpp runs every layout on malloc'ed memory without a GPU.
#pragma once
#include "ba_common.h"
#include "imu_dual.h"

// What the caller decides about one window (w.d says how large it is): for the layouts and the window binder (ba.hip)
struct BaWinAsk {
    int ns, max_iter;                 // speculative sets per round; iteration cap (sizes the trace)
    int n_ranks, rank, srep;          // landmark shards, this rank's gradient-max block; replicas of S
    size_t grp_bytes;                 // the landmark grouping's sub-block (ba_group_bytes), 16 off the MFMA path
    size_t big_bytes, zacc_doubles;   // single solve only: the blocked / inertial reduced solve's part, the inertial elimination's accumulators
    bool tables, inertial;            // pinned block: with the slot / free-camera tables (single solve), with velocity | bias
    bool use_mfma; int items;         // carve the grouping; landmarks per item in throughput mode (ba_group_set_items), < 0: as carved
};
// the pieces of a window that BaWin has no field for
struct BaExtra {
    char* grp; char* big; double* zacc;                     // workspace: [grp_bytes] [big_bytes] [zacc_doubles]
    int32_t* slot; uint8_t* fre;                            // pinned [C] each: windows of more than 64 cameras upload their tables from here
    volatile unsigned long long* key; double* vb;           // pinned: span / lost-key word; [C][9] velocity | bias of the accepted state
};

// Workspace of one window, for the single solve and every window of a batched solve: w.b (round parity 0), the round bases,
// the free-camera table.
static inline void ba_window_layout(rs_carve& c, const BaWinAsk& a, BaWin& w, BaExtra& x)
{
    const BaDims& d = w.d;
    BaBufs& b = w.b;
    const size_t n = (size_t)d.n, C = (size_t)d.C, P = (size_t)d.P, Cf = (size_t)d.Cf, ns = (size_t)a.ns, nb = ns + 1;
    const size_t slots = (size_t)BA_NSLOT * BA_SLOT_STRIDE;
    b.ns = a.ns; b.srep = a.srep; b.s_rep_stride = ns * n * n; b.gmax_blocks = a.n_ranks; b.decided = 0;
    b.cam_stride = ns * n + Cf * 36 + n;
    b.acc_count = (size_t)a.srep * ns * n * n + (size_t)BA_UREP * b.cam_stride + (1 + (size_t)a.n_ranks) * slots;
    w.pts_block = ns * slots;
    b.Xc = c.take<double>(nb * C * 6);
    b.Xp = c.take<double>(nb * P * 3);
    b.prep = c.take<double>(nb * C * BA_PREP);
    b.slot = c.take<int32_t>(C);
    b.sc = c.take<double>(n + 1);
    b.sp = c.take<double>(P * 3);
    b.Vinv = c.take<double>(ns * P * 6);
    b.gp = c.take<double>(P * 3);
    b.lamp = c.take<double>(ns * P * 3);
    b.Vc = c.take<double>(P * 6);
    b.Ukeep = c.take<double>(Cf * 36 + n + 1);
    b.acc = c.take<double>(b.acc_count);
    b.pt_prev = b.pt_scal = w.pts_base = c.take<double>(2 * w.pts_block);
    b.dc = c.take<double>(ns * BA_DC_STRIDE(n));
    b.st_prev = b.st = w.st_base = c.take<BaState>(2);
    b.set_prev = b.set_out = w.set_base = c.take<BaSetOut>(2 * BA_MAXSETS);
    b.trace = c.take<BaTrace>((size_t)a.max_iter + 1);
    b.dbg = c.take<unsigned long long>(BA_DBG_WORDS);
    w.cam_free = c.take<uint8_t>(C);
    x.grp = c.take<char>(a.grp_bytes);
    x.big = c.take<char>(a.big_bytes);
    x.zacc = c.take<double>(a.zacc_doubles);
    // inside the accumulators (one all-reduce): S | BA_UREP x { rhs U gc } | scal | every rank's gmax
    b.S = b.rhs = b.U = b.gc = b.scal = b.gmax_all = b.gmax = nullptr;
    if (!b.acc) return;
    b.S = b.acc; b.rhs = b.S + (size_t)a.srep * ns * n * n; b.U = b.rhs + ns * n; b.gc = b.U + Cf * 36;
    b.scal = b.rhs + (size_t)BA_UREP * b.cam_stride;
    b.gmax_all = b.scal + slots;
    b.gmax = b.gmax_all + (size_t)a.rank * slots;
}

// Pinned block of one window: what the host reads while and after the device works.  The progress line is a 64-byte line of
// its own — nothing else the device writes during the rounds shares it — with the key word in its unused half; the
// completion flag is BaProgress::pad.
static inline void ba_pinned_layout(rs_carve& c, const BaWinAsk& a, BaWin& w, BaExtra& x)
{
    const size_t C = (size_t)w.d.C;
    w.h_st = c.take<BaState>(1);
    x.slot = a.tables ? c.take<int32_t>(C) : nullptr;
    x.fre = a.tables ? c.take<uint8_t>(C) : nullptr;
    char* line = c.take<char>(64);
    w.prog = (BaProgress*)line;
    x.key = line ? (volatile unsigned long long*)(line + 32) : nullptr;
    w.h_trace = c.take<BaTrace>((size_t)a.max_iter + 1);
    w.h_cams = c.take<double>(C * 6);
    x.vb = a.inertial ? c.take<double>(C * 9) : nullptr;
}
static_assert(sizeof(BaProgress) <= 32, "the key word sits in the progress line's second half");

// ---- refine_pose (refine_pose.hip): the inertial constraint as the kernel reads it (one piece of the workspace), and the
// pinned block, whose pieces the kernel reads and writes itself
struct RpInertial {
    int kind;                 // 1 rotation prior, 2 inertial delta
    double predicted[9], sigma;
    double prev_pose[6], prev_vel[3], prev_bias[6], gravity[3];
    ImuFactorDev fac;
};
static inline void rp_pinned_layout(rs_carve& c, bool inertial, double*& cam, BaState*& st, volatile int*& done, int*& n_used, RpInertial*& ext)
{
    cam = c.take<double>(9);            // camera (6), velocity (3)
    st = c.take<BaState>(1);
    done = c.take<int>(1);              // completion flag the host spins on
    n_used = c.take<int>(1);            // the device-side count
    ext = inertial ? c.take<RpInertial>(1) : nullptr;      // staging copy of the inertial constraint
}
