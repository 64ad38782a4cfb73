// racing-slam_amd/csrc/ba_blocks.h on its own: the workspace and pinned layouts of a bundle-adjustment window and the two
// blocks of refine_pose, each run on a null carver and on a malloc'ed block, as a stand-alone program under the address and
// undefined-behaviour sanitizers (tests/test_ba_blocks_cpu.py).  It makes no HIP call and needs no GPU.  Blocks of up to
// 8 MiB are written and read back byte by byte through the typed pointers; of the larger ones (the 64-camera windows with
// replicas, the 131- and 486-camera windows, up to 2.7 GB) the first and the last element of every piece, besides the checks of
// alignment, order, disjointness and extent that every block gets.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../racing-slam_amd/csrc/ba_blocks.h"

static long g_fail = 0;
#define CHECK(c)                                                                             \
    do {                                                                                     \
        if (!(c)) { if (g_fail < 40) printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #c, g_case); g_fail++; } \
    } while (0)
static char g_case[256] = "";

// a piece as the test expects it: where the layout put it, and the bytes the test itself computes for it
struct Piece {
    const char* name; char* p; size_t bytes;
    void (*fill)(char* p, size_t bytes, int tag, bool all);
};
// writes through the typed pointer: every element, or (blocks too large to fill in a quick test) the first and the last
template <class T>
static void fill(char* p, size_t bytes, int tag, bool all)
{
    T* t = (T*)p;
    const size_t n = bytes / sizeof(T);
    for (size_t i = 0; i < n; i = (all || i + 1 >= n) ? i + 1 : n - 1) memset((void*)&t[i], tag, sizeof(T));
}
template <class T>
static void add(std::vector<Piece>& v, const char* name, T* p, size_t count) { v.push_back({name, (char*)p, sizeof(T) * count, fill<T>}); }

// 256-aligned block of `bytes` inside a malloc'ed one (malloc gives 16-byte alignment)
struct Block {
    char* raw; char* base;
    explicit Block(size_t bytes) : raw((char*)malloc(bytes + 255)), base(nullptr)
    {
        if (raw) base = raw + (rs_align256((size_t)(uintptr_t)raw) - (size_t)(uintptr_t)raw);
    }
    ~Block() { free(raw); }
};

#define FILL_ALL_LIMIT ((size_t)8 << 20)      // blocks up to 8 MiB are written and read back byte by byte
static void check_pieces(const std::vector<Piece>& pieces, char* base, size_t total)
{
    const char* at = base;
    for (const Piece& q : pieces) {
        CHECK(q.p != nullptr);
        CHECK(((uintptr_t)q.p & 255) == 0);
        CHECK(q.p >= at);                                   // in order, disjoint from the one before
        at = q.p + q.bytes;
    }
    CHECK(at <= base + total);                              // the last piece ends inside the block
    const bool all = total <= FILL_ALL_LIMIT;
    for (size_t i = 0; i < pieces.size(); i++) pieces[i].fill(pieces[i].p, pieces[i].bytes, (int)(i + 1), all);
    for (size_t i = 0; i < pieces.size(); i++) {
        const Piece& q = pieces[i];
        if (all) { for (size_t k = 0; k < q.bytes; k++) if ((unsigned char)q.p[k] != i + 1) { CHECK(!"byte read back"); break; } }
        else if (q.bytes) CHECK((unsigned char)q.p[0] == i + 1 && (unsigned char)q.p[q.bytes - 1] == i + 1);
    }
}

static BaDims dims(int C, int Cf, int P, int M)
{
    BaDims d;
    memset(&d, 0, sizeof d);
    d.C = C; d.Cf = Cf; d.P = P; d.M = M; d.n = 6 * Cf;
    return d;
}
// a stand-in for ba_group_bytes (ba_schur.hip): the layout takes the grouping's size as a number
static size_t grp_standin(const BaDims& d) { return 4 * (size_t)d.M + 40 * (size_t)d.P + 8 * (size_t)d.Cf * d.Cf + 24; }

// the pieces of ba_window_layout in the order taken, counts restated from BaBufs' comments (ba_common.h)
static void window_pieces(const BaWinAsk& a, const BaWin& w, const BaExtra& k, std::vector<Piece>& v)
{
    const BaDims& d = w.d;
    const BaBufs& b = w.b;
    const size_t n = (size_t)d.n, C = (size_t)d.C, P = (size_t)d.P, Cf = (size_t)d.Cf, ns = (size_t)a.ns, slots = (size_t)BA_NSLOT * BA_SLOT_STRIDE;
    v.clear();
    add(v, "Xc", b.Xc, (ns + 1) * C * 6); add(v, "Xp", b.Xp, (ns + 1) * P * 3); add(v, "prep", b.prep, (ns + 1) * C * BA_PREP);
    add(v, "slot", b.slot, C); add(v, "sc", b.sc, n + 1); add(v, "sp", b.sp, P * 3); add(v, "Vinv", b.Vinv, ns * P * 6);
    add(v, "gp", b.gp, P * 3); add(v, "lamp", b.lamp, ns * P * 3); add(v, "Vc", b.Vc, P * 6); add(v, "Ukeep", b.Ukeep, Cf * 36 + n + 1);
    add(v, "acc", b.acc, (size_t)a.srep * ns * n * n + BA_UREP * (ns * n + Cf * 36 + n) + (1 + (size_t)a.n_ranks) * slots);
    add(v, "pts", b.pt_scal, 2 * ns * slots); add(v, "dc", b.dc, ns * BA_DC_STRIDE(n)); add(v, "st", b.st, 2);
    add(v, "set", b.set_out, 2 * BA_MAXSETS); add(v, "trace", b.trace, (size_t)a.max_iter + 1); add(v, "dbg", b.dbg, BA_DBG_WORDS);
    add(v, "fre", w.cam_free, C); add(v, "grp", k.grp, a.grp_bytes); add(v, "big", k.big, a.big_bytes); add(v, "zacc", k.zacc, a.zacc_doubles);
}

// one window: null run, placed run, the pieces, what is derived from them; returns the total
static size_t check_window(const BaDims& d, const BaWinAsk& a)
{
    BaWin w;
    BaExtra k;
    std::vector<Piece> v;
    memset(&w, 0, sizeof w);
    w.d = d;
    BaBufs& b = w.b;
    rs_carve size;
    ba_window_layout(size, a, w, k);
    window_pieces(a, w, k, v);
    for (const Piece& q : v) CHECK(q.p == nullptr);
    CHECK(!b.S && !b.rhs && !b.U && !b.gc && !b.scal && !b.gmax_all && !b.gmax);       // nothing derived from a null base
    const size_t total = size.bytes();
    CHECK(total % 256 == 0);
    Block blk(total);
    CHECK(blk.base != nullptr);
    if (!blk.base) return total;
    rs_carve place(blk.base);
    ba_window_layout(place, a, w, k);
    CHECK(place.bytes() == total);                                                     // the two runs agree
    window_pieces(a, w, k, v);
    CHECK(b.Xc == (double*)blk.base);
    check_pieces(v, blk.base, total);
    // inside the accumulators: S | BA_UREP x { rhs U gc } | scal | every rank's gmax, ending where acc ends
    const size_t n = (size_t)d.n, ns = (size_t)a.ns, slots = (size_t)BA_NSLOT * BA_SLOT_STRIDE;
    CHECK(b.ns == a.ns && b.srep == a.srep && b.s_rep_stride == ns * n * n && b.gmax_blocks == a.n_ranks && b.decided == 0);
    CHECK(b.cam_stride == ns * n + (size_t)d.Cf * 36 + n);
    CHECK(b.S == b.acc && b.rhs == b.S + (size_t)a.srep * b.s_rep_stride && b.U == b.rhs + ns * n && b.gc == b.U + (size_t)d.Cf * 36);
    CHECK(b.scal == b.rhs + BA_UREP * b.cam_stride && b.gmax_all == b.scal + slots && b.gmax == b.gmax_all + (size_t)a.rank * slots);
    CHECK(b.gmax_all + (size_t)a.n_ranks * slots == b.acc + b.acc_count);
    CHECK(w.pts_block == ns * slots && b.pt_prev == b.pt_scal && b.st_prev == b.st && b.set_prev == b.set_out);
    CHECK(w.pts_base == b.pt_scal && w.st_base == b.st && w.set_base == b.set_out);
    return total;
}

static void check_pinned(const BaDims& d, const BaWinAsk& a)
{
    BaWin w;
    BaExtra h;
    memset(&w, 0, sizeof w);
    w.d = d;
    rs_carve size;
    ba_pinned_layout(size, a, w, h);
    CHECK(!w.h_st && !h.slot && !h.fre && !w.prog && !h.key && !w.h_trace && !w.h_cams && !h.vb);
    const size_t total = size.bytes(), C = (size_t)d.C;
    Block blk(total);
    CHECK(blk.base != nullptr);
    if (!blk.base) return;
    rs_carve place(blk.base);
    ba_pinned_layout(place, a, w, h);
    CHECK(place.bytes() == total);
    CHECK((h.slot != nullptr) == a.tables && (h.fre != nullptr) == a.tables && (h.vb != nullptr) == a.inertial);
    std::vector<Piece> v;
    add(v, "st", w.h_st, 1);
    if (a.tables) { add(v, "slot", h.slot, C); add(v, "fre", h.fre, C); }
    add(v, "line", (char*)w.prog, 64);
    add(v, "trace", w.h_trace, (size_t)a.max_iter + 1); add(v, "cams", w.h_cams, C * 6);
    if (a.inertial) add(v, "vb", h.vb, C * 9);
    check_pieces(v, blk.base, total);
    // the progress line: a 64-byte line of its own (the pieces around it start on other 256-byte boundaries, checked above),
    // the progress words in its first half, the key word at + 32 and nothing else
    BaProgress* prog = w.prog;
    CHECK((char*)h.key == (char*)prog + 32 && sizeof(BaProgress) <= 32);
    for (const Piece& q : v)
        if (q.p != (char*)prog) CHECK(q.p + q.bytes <= (char*)prog || q.p >= (char*)prog + 64);
    prog->round = 1; prog->done = 2; prog->iter = 3; prog->pad = 4; *h.key = ~0ull;
    CHECK(prog->round == 1 && prog->done == 2 && prog->iter == 3 && prog->pad == 4 && *h.key == ~0ull);
}

static void check_refine_pose(bool inertial)
{
    double* cam; BaState* st; volatile int* done; int* n_used; RpInertial* ext;
    rs_carve size;
    rp_pinned_layout(size, inertial, cam, st, done, n_used, ext);
    CHECK(!cam && !st && !done && !n_used && !ext);
    const size_t total = size.bytes();
    Block blk(total);
    CHECK(blk.base != nullptr);
    if (!blk.base) return;
    rs_carve place(blk.base);
    rp_pinned_layout(place, inertial, cam, st, done, n_used, ext);
    CHECK(place.bytes() == total && (ext != nullptr) == inertial);
    std::vector<Piece> v;
    add(v, "cam", cam, 9); add(v, "st", st, 1); add(v, "done", (int*)done, 1); add(v, "n_used", n_used, 1);
    if (inertial) add(v, "ext", ext, 1);
    check_pieces(v, blk.base, total);
    // flag and count share no 64-byte line with the summary
    CHECK((char*)done >= (char*)st + rs_align256(sizeof(BaState)) && (char*)n_used >= (char*)st + rs_align256(sizeof(BaState)));
}

int main()
{
    const int grid[8][4] = {{1, 1, 0, 0}, {1, 1, 1, 1}, {3, 0, 60, 180}, {8, 6, 300, 900}, {64, 62, 500, 2000}, {65, 63, 500, 2000},
                            {131, 129, 400, 1600}, {486, 484, 1000, 4000}};
    const int nss[3] = {1, 3, 5}, its[3] = {0, 1, 1000}, rks[2] = {1, 8}, srs[2] = {1, 8};
    long windows = 0;
    for (const int* g : grid) for (int ns : nss) for (int mi : its) for (int nr : rks) for (int sr : srs) {
        const BaDims d = dims(g[0], g[1], g[2], g[3]);
        BaWinAsk a = {};
        a.ns = ns; a.max_iter = mi; a.n_ranks = nr; a.rank = nr - 1; a.srep = sr;
        // the grid batch's window (no tail) where one rank and one copy of S; else the single solve's, with and without the inertial tail
        a.grp_bytes = sr == 1 ? grp_standin(d) : 16;
        a.big_bytes = (nr == 1 && sr == 1) ? 0 : (mi == 1 ? 8 * (size_t)d.n * d.n + 100 : 16);
        a.zacc_doubles = (nr == 8 && mi == 1) ? 1000 + 7 * (size_t)d.n : 0;
        snprintf(g_case, sizeof g_case, "window C %d Cf %d P %d M %d ns %d max_iter %d ranks %d srep %d", d.C, d.Cf, d.P, d.M, ns, mi, nr, sr);
        check_window(d, a);
        windows++;
    }
    // the totals of the hand layout this function replaced, recorded from its formula at four of the grid points (the
    // grouping's size is an input of both: 16, or grp_standin() in place of ba_group_bytes)
    {
        struct { int g, ns, mi, nr, sr; bool standin; size_t total; } lit[4] = {
            {0, 5, 1, 8, 8, false, 100352}, {3, 5, 1, 8, 8, false, 720384}, {2, 3, 1000, 1, 1, true, 132096}, {4, 3, 1000, 1, 1, true, 4017152}};
        for (const auto& l : lit) {
            const BaDims d = dims(grid[l.g][0], grid[l.g][1], grid[l.g][2], grid[l.g][3]);
            BaWinAsk a = {};
            a.ns = l.ns; a.max_iter = l.mi; a.n_ranks = l.nr; a.rank = 0; a.srep = l.sr; a.grp_bytes = l.standin ? grp_standin(d) : 16;
            snprintf(g_case, sizeof g_case, "literal total of grid point %d", l.g);
            CHECK(check_window(d, a) == l.total);
            a.big_bytes = 16;                                   // the single solve's smallest tail: one more 256-byte piece
            CHECK(check_window(d, a) == l.total + 256);
        }
    }
    // the batch form: the table of windows, then one window after the other on the same carver
    {
        snprintf(g_case, sizeof g_case, "batch");
        const int B = 3, idx[3] = {2, 3, 4};
        rs_carve size;
        size.take<BaWin>(B);
        size_t sum = rs_align256(sizeof(BaWin) * (size_t)B);
        for (int i : idx) {
            const BaDims d = dims(grid[i][0], grid[i][1], grid[i][2], grid[i][3]);
            BaWinAsk a = {};
            a.ns = 3; a.max_iter = 10; a.n_ranks = 1; a.srep = 1; a.grp_bytes = grp_standin(d);
            BaWin w; BaExtra k;
            w.d = d;
            const size_t before = size.bytes();
            ba_window_layout(size, a, w, k);
            CHECK(before == sum && size.bytes() - before == check_window(d, a));
            sum = size.bytes();
        }
    }
    // pinned block: every flag combination
    long pinned = 0;
    for (const int* g : grid) for (int mi : its) for (int tables = 0; tables < 2; tables++) for (int inertial = 0; inertial < 2; inertial++) {
        const BaDims d = dims(g[0], g[1], g[2], g[3]);
        BaWinAsk a = {};
        a.max_iter = mi; a.tables = tables != 0; a.inertial = inertial != 0;
        snprintf(g_case, sizeof g_case, "pinned C %d max_iter %d tables %d inertial %d", d.C, mi, tables, inertial);
        check_pinned(d, a);
        pinned++;
    }
    snprintf(g_case, sizeof g_case, "refine_pose");
    check_refine_pose(false);
    check_refine_pose(true);

    if (g_fail) { printf("%ld BA block checks FAILED\n", g_fail); return 1; }
    printf("BA block checks passed (%ld windows, %ld pinned blocks)\n", windows, pinned);
    return 0;
}
