// bow.hip — key-frame recognition: the vocabulary tree, the bag-of-words transform of a frame's ORB rows, and L1
// scoring of that vector against a database of earlier key frames' vectors.
//
// Replaces the "Loop retrieval" stage of LoopDetector::query (reference src/LoopDetector.cpp:346-373, bow_of and
// vocabulary->score; DBoW2's TemplatedVocabulary::transform :1066-1122 / :1218-1259, BowVector.cpp:34-84 and
// L1Scoring::score, ScoringObject.cpp:23-68).  The specification is tests/bow_ref.py.  Word ids, occurrence counts and
// the word list are integer results and equal it exactly; values, the norm and scores are f64 sums of at most 8192
// positive terms in a fixed order (count x weight, fixed trees), so two runs give identical bytes.
//
// The tree is stored in breadth-first order with every node's children contiguous and in ascending node id (the
// reference's child order), so one level of the descent is one contiguous read of at most 20 x 32 bytes and the first
// BOW_LDS_NODES nodes (the top levels) are a prefix that bow_descend stages in LDS.
//   bow_descend   16 lanes per feature, one child per lane (a second trip for children 16 .. 19); each lane holds the
//                 feature's eight dwords, counts the bits of its child's row and the sub-group takes the minimum of
//                 (distance << 5 | child position): the lowest position wins ties, the reference's strict '<'
//   bow_reduce    one workgroup: bitonic sort of the word ids in LDS, run lengths, stopped words dropped, values,
//                 the norm by a fixed tree, the division; it also keeps the object's dense word -> position + 1 table
//                 in step with the vector (the old words cleared, the new ones set)
//   bow_score     one wave per database entry; lanes stride over the entry's words and look the query's value up in
//                 that table (or, "bow_score_mode" 1, by binary search in the query's sorted words); a fixed shuffle tree
// Bounds: every child index is below n_nodes by construction of the tree (rs_vocabulary_create checks the parents);
// a feature index is below n <= min(max_n, max_points); a word id is below n_words, the size of the table; database
// offsets are checked on the host against the capacities before anything is copied.
#include <algorithm>
#include <fstream>
#include <sstream>

#include "common.h"

#define BOW_MAX_K 20
#define BOW_MAX_L 10
#define BOW_MAX_NODES 4194304
#define BOW_MAX_POINTS 8192
#define BOW_MAX_ENTRIES 1048576
#define BOW_MAX_TOTAL_WORDS 1073741824
#define BOW_LDS_NODES 1280          // nodes of the tree's breadth-first prefix kept in LDS (40 B each)
#define BOW_SUB 16                  // lanes per feature
#define BOW_THREADS 1024
#define BOW_GROUPS (BOW_THREADS / BOW_SUB)
#define BOW_ITEMS (BOW_MAX_POINTS / BOW_THREADS)
#define BOW_MAX_BLOCKS 256
#define BOW_SCORE_WAVES 4

struct rs_vocabulary {
    rs_context* ctx = nullptr;
    int k = 0, L = 0, weighting = 0, scoring = 0, n_nodes = 0, n_words = 0;
    rs_dev_block block;
    uint4* d_desc = nullptr;            // [n_nodes][2], breadth-first order
    int2* d_info = nullptr;             // [n_nodes] {first child, children}; a leaf: {word id, 0}
    double* d_word_weight = nullptr;    // [n_words]
    std::vector<int32_t> parent;        // the arrays as given, in node order (rs_vocabulary_arrays)
    std::vector<uint8_t> desc;
    std::vector<double> weight;
};

struct rs_bow {
    rs_context* ctx = nullptr;
    rs_vocabulary* voc = nullptr;
    int max_points = 0;
    rs_dev_block block;
    int32_t* d_feat_word = nullptr;     // [max_points] word of every feature of the last transform
    int32_t* d_words = nullptr;         // [max_points] the vector: sorted unique words,
    int32_t* d_counts = nullptr;        //              their occurrences
    double* d_values = nullptr;         //              and values
    int32_t* d_hdr = nullptr;           // [2] words in the vector, features of the last transform
    double* d_norm = nullptr;           // [1]
    int32_t* d_lookup = nullptr;        // [n_words] position + 1 of a word in the vector, 0 = absent
};

struct rs_bow_database {
    rs_context* ctx = nullptr;
    rs_vocabulary* voc = nullptr;
    int max_entries = 0, max_total_words = 0;
    rs_dev_block block;
    int32_t* d_ptr = nullptr;           // [max_entries + 1] CSR offsets
    int32_t* d_words = nullptr;         // [max_total_words]
    double* d_values = nullptr;
    std::vector<int32_t> ptr;           // host mirror of d_ptr[0 .. entries]
};

struct BowTree { const uint4* desc; const int2* info; int n_lds; };
struct BowVec { int32_t* words; int32_t* counts; double* values; int32_t* hdr; double* norm; int32_t* lookup; };

__device__ __forceinline__ int bow_distance(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    return __popcll(((unsigned long long)(a0.x ^ b0.x) << 32) | (a0.y ^ b0.y)) + __popcll(((unsigned long long)(a0.z ^ b0.z) << 32) | (a0.w ^ b0.w)) +
           __popcll(((unsigned long long)(a1.x ^ b1.x) << 32) | (a1.y ^ b1.y)) + __popcll(((unsigned long long)(a1.z ^ b1.z) << 32) | (a1.w ^ b1.w));
}

// ------------------------------------------------------------------------------------------------ descent
__global__ __launch_bounds__(BOW_THREADS) void bow_descend(BowTree t, const uint4* __restrict__ feat, const int32_t* __restrict__ d_count,
                                                         int max_n, int cap, int32_t* __restrict__ feat_word,
                                                         int32_t* __restrict__ d_word, int32_t* __restrict__ hdr)
{
    __shared__ uint4 s_desc[2 * BOW_LDS_NODES];
    __shared__ int2 s_info[BOW_LDS_NODES];
    const int tid = threadIdx.x, sub = tid & (BOW_SUB - 1), grp = tid / BOW_SUB;
    const int n = min(max(d_count[0], 0), min(max_n, cap));
    if (blockIdx.x == 0 && tid == 0) hdr[1] = n;
    if (d_word)
        for (int i = n + blockIdx.x * BOW_THREADS + tid; i < max_n; i += gridDim.x * BOW_THREADS) d_word[i] = -1;
    if ((int)blockIdx.x * BOW_GROUPS >= n) return;            // the whole workgroup
    for (int i = tid; i < 2 * t.n_lds; i += BOW_THREADS) s_desc[i] = t.desc[i];
    for (int i = tid; i < t.n_lds; i += BOW_THREADS) s_info[i] = t.info[i];
    __syncthreads();
    for (int base = blockIdx.x * BOW_GROUPS; base < n; base += gridDim.x * BOW_GROUPS) {
        const int f = base + grp;
        const bool live = f < n;
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        if (live) { q0 = feat[2 * (size_t)f]; q1 = feat[2 * (size_t)f + 1]; }
        int node = 0, word = -1;
        bool walking = live;
        while (__any(walking)) {                              // the wave stays together: the shuffles below need every lane
            int2 info = make_int2(0, 0);
            if (walking) info = node < t.n_lds ? s_info[node] : t.info[node];
            if (walking && info.y == 0) { word = info.x; walking = false; }
            unsigned best = 0xFFFFFFFFu;
#pragma unroll
            for (int trip = 0; trip < (BOW_MAX_K + BOW_SUB - 1) / BOW_SUB; trip++) {
                const int j = trip * BOW_SUB + sub;
                if (walking && j < info.y) {
                    const int c = info.x + j;
                    uint4 c0, c1;
                    if (c < t.n_lds) { c0 = s_desc[2 * c]; c1 = s_desc[2 * c + 1]; }
                    else { c0 = t.desc[2 * (size_t)c]; c1 = t.desc[2 * (size_t)c + 1]; }
                    best = min(best, ((unsigned)bow_distance(q0, q1, c0, c1) << 5) | (unsigned)j);
                }
            }
#pragma unroll
            for (int off = BOW_SUB / 2; off > 0; off >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, off, BOW_SUB));
            if (walking) node = info.x + (int)(best & 31u);
        }
        if (live && sub == 0) {
            feat_word[f] = word;
            if (d_word) d_word[f] = word;
        }
    }
}

// ------------------------------------------------------------------------------------------------ reduce
__global__ __launch_bounds__(BOW_THREADS) void bow_reduce(const int32_t* __restrict__ feat_word, const double* __restrict__ word_weight,
                                                        int weighting, BowVec v)
{
    __shared__ int32_t key[BOW_MAX_POINTS];
    __shared__ uint16_t pos[BOW_MAX_POINTS + 2];              // start of every run of equal words, then n
    __shared__ double part[BOW_THREADS];
    const int tid = threadIdx.x, n = v.hdr[1], old = v.hdr[0];
    for (int i = tid; i < old; i += BOW_THREADS) v.lookup[v.words[i]] = 0;       // the previous vector leaves the table
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += BOW_THREADS) key[i] = i < n ? feat_word[i] : 0x7FFFFFFF;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += BOW_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int a = key[i], b = key[i + j];
                if ((a > b) == ((i & k2) == 0)) { key[i] = b; key[i + j] = a; }
            }
            __syncthreads();
        }
    // runs of equal words: thread tid owns positions 8 tid .. 8 tid + 7
    const int i0 = tid * BOW_ITEMS;
    int heads = 0;
#pragma unroll
    for (int e = 0; e < BOW_ITEMS; e++) {
        const int i = i0 + e;
        heads += (i < n && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
    }
    int U = 0;
    int off = rs_block_exclusive_scan(heads, &U);
#pragma unroll
    for (int e = 0; e < BOW_ITEMS; e++) {
        const int i = i0 + e;
        if (i < n && (i == 0 || key[i] != key[i - 1])) pos[off++] = (uint16_t)i;
    }
    if (tid == 0) pos[U] = (uint16_t)n;
    __syncthreads();
    // unique words: thread tid owns runs 8 tid .. 8 tid + 7; stopped words (weight <= 0) are dropped
    int w[BOW_ITEMS], c[BOW_ITEMS], kept = 0;
    double val[BOW_ITEMS], sum = 0.0;
#pragma unroll
    for (int e = 0; e < BOW_ITEMS; e++) {
        const int u = i0 + e;
        w[e] = -1; c[e] = 0; val[e] = 0.0;
        if (u < U) {
            const int p = pos[u], word = key[p];
            const double wt = word_weight[word];
            if (wt > 0.0) {
                w[e] = word;
                c[e] = (int)pos[u + 1] - p;
                val[e] = weighting <= 1 ? (double)c[e] * wt : wt;                // TF_IDF, TF: once per occurrence
                sum += val[e];
                kept++;
            }
        }
    }
    int M = 0;
    int at = rs_block_exclusive_scan(kept, &M);
    part[tid] = sum;
    __syncthreads();
    for (int st = BOW_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) part[tid] += part[tid + st];
        __syncthreads();
    }
    const double norm = part[0];
#pragma unroll
    for (int e = 0; e < BOW_ITEMS; e++)
        if (w[e] >= 0) {
            v.words[at] = w[e];
            v.counts[at] = c[e];
            v.values[at] = norm > 0.0 ? val[e] / norm : val[e];
            v.lookup[w[e]] = at + 1;
            at++;
        }
    if (tid == 0) { v.hdr[0] = M; *v.norm = norm; }
}

// ------------------------------------------------------------------------------------------------ score
template <bool DENSE>
__global__ __launch_bounds__(64 * BOW_SCORE_WAVES) void bow_score(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ewords,
                                                                const double* __restrict__ evalues, int first, int count,
                                                                const int32_t* __restrict__ lookup, const int32_t* __restrict__ qwords,
                                                                const double* __restrict__ qvalues, const int32_t* __restrict__ qhdr,
                                                                double* __restrict__ out)
{
    const int e = blockIdx.x * BOW_SCORE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= count) return;                                   // the whole wave
    const int b = ptr[first + e], en = ptr[first + e + 1], nq = qhdr[0];
    double s = 0.0;
    for (int i = b + lane; i < en; i += 64) {
        const int word = ewords[i];
        int p = 0;
        if (DENSE) {
            p = lookup[word];
        } else {
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qwords[mid] < word) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qwords[lo] == word) p = lo + 1;
        }
        if (p) {
            const double a = qvalues[p - 1], x = evalues[i];
            s += fabs(a - x) - fabs(a) - fabs(x);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[e] = -s / 2.0;
}

__global__ void bow_set_int(int32_t* p, int32_t v) { *p = v; }

// ------------------------------------------------------------------------------------------------ vocabulary
// h_is_leaf (NULL = not checked): the text file's leaf flags
static int vocabulary_build(rs_context* ctx, int k, int L, int weighting, int scoring, int n_nodes, const int32_t* h_parent,
                            const uint8_t* h_desc, const double* h_weight, const uint8_t* h_is_leaf, rs_vocabulary** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (!h_parent || !h_desc || !h_weight) return rs_fail(ctx, RS_ERR_INVALID, "null vocabulary arrays");
    if (k < 1 || k > BOW_MAX_K || L < 1 || L > BOW_MAX_L || n_nodes < 2 || n_nodes > BOW_MAX_NODES)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "vocabulary: k 1 .. %d, L 1 .. %d, 2 .. %d nodes", BOW_MAX_K, BOW_MAX_L, BOW_MAX_NODES);
    if (weighting < 0 || weighting > 3) return rs_fail(ctx, RS_ERR_INVALID, "weighting must be 0 (TF_IDF), 1 (TF), 2 (IDF) or 3 (BINARY)");
    if (scoring != 0) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "scoring type %d: only L1_NORM (0) is implemented", scoring);
    const size_t n = (size_t)n_nodes;
    std::vector<int32_t> cnt(n, 0), first(n + 1, 0);
    for (size_t i = 1; i < n; i++) {
        const int32_t p = h_parent[i];
        if (p < 0 || (size_t)p >= i) return rs_fail(ctx, RS_ERR_INVALID, "node %zu: parent %d is not below it", i, p);
        if (++cnt[p] > k) return rs_fail(ctx, RS_ERR_INVALID, "node %d has more than k = %d children", p, k);
    }
    if (h_is_leaf)
        for (size_t i = 1; i < n; i++)
            if ((h_is_leaf[i] != 0) != (cnt[i] == 0))
                return rs_fail(ctx, RS_ERR_INVALID, "node %zu: leaf flag %d with %d children", i, (int)h_is_leaf[i], cnt[i]);
    // children in ascending node id (the loader's push_back order), then the breadth-first order
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + cnt[i];
    std::vector<int32_t> child(n > 1 ? n - 1 : 1), fill(first.begin(), first.end() - 1), order(n), word_of(n, -1);
    for (size_t i = 1; i < n; i++) child[fill[h_parent[i]]++] = (int32_t)i;
    int n_words = 0;
    for (size_t i = 0; i < n; i++)
        if (cnt[i] == 0) word_of[i] = n_words++;
    std::vector<int2> info(n);
    size_t tail = 1;
    order[0] = 0;
    for (size_t p = 0; p < n; p++) {
        const int32_t node = order[p];
        if (cnt[node] == 0) { info[p] = make_int2(word_of[node], 0); continue; }
        info[p] = make_int2((int)tail, cnt[node]);
        for (int32_t j = 0; j < cnt[node]; j++) order[tail++] = child[first[node] + j];
    }
    std::vector<uint8_t> desc(32 * n);
    std::vector<double> ww((size_t)n_words);
    for (size_t p = 0; p < n; p++) {
        memcpy(&desc[32 * p], h_desc + 32 * (size_t)order[p], 32);
        if (cnt[order[p]] == 0) ww[word_of[order[p]]] = h_weight[order[p]];
    }
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_vocabulary* v = new rs_vocabulary();
    v->ctx = ctx;
    v->k = k; v->L = L; v->weighting = weighting; v->scoring = scoring; v->n_nodes = n_nodes; v->n_words = n_words;
    const int rc = v->block.carve(ctx, "vocabulary", [&](rs_carve& c) {
        v->d_desc = c.take<uint4>(2 * n);
        v->d_info = c.take<int2>(n);
        v->d_word_weight = c.take<double>((size_t)n_words);
    });
    if (rc != RS_OK) { delete v; return rc; }
    if (hipMemcpy(v->d_desc, desc.data(), 32 * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->d_info, info.data(), sizeof(int2) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->d_word_weight, ww.data(), sizeof(double) * (size_t)n_words, hipMemcpyHostToDevice) != hipSuccess) {
        delete v;
        return rs_fail(ctx, RS_ERR_HIP, "vocabulary upload failed");
    }
    v->parent.assign(h_parent, h_parent + n);
    v->parent[0] = -1;
    v->desc.assign(h_desc, h_desc + 32 * n);
    v->weight.assign(h_weight, h_weight + n);
    *out = v;
    return RS_OK;
}

extern "C" int rs_vocabulary_create(rs_context* ctx, int k, int L, int weighting, int scoring, int n_nodes, const int32_t* h_parent,
                                    const uint8_t* h_descriptors, const double* h_weight, rs_vocabulary** out_voc)
{
    return vocabulary_build(ctx, k, L, weighting, scoring, n_nodes, h_parent, h_descriptors, h_weight, nullptr, out_voc);
}

extern "C" int rs_vocabulary_load_text(rs_context* ctx, const char* path, rs_vocabulary** out_voc)
{
    if (!ctx || !out_voc) return RS_ERR_INVALID;
    *out_voc = nullptr;
    if (!path) return rs_fail(ctx, RS_ERR_INVALID, "null path");
    std::ifstream f(path, std::ios::binary);
    if (!f) return rs_fail(ctx, RS_ERR_INVALID, "cannot open %s", path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    std::vector<std::pair<size_t, size_t>> lines;             // [begin, end) of every line, trailing blank lines dropped
    for (size_t b = 0; b < text.size();) {
        size_t e = text.find('\n', b);
        if (e == std::string::npos) e = text.size();
        lines.push_back({b, e});
        b = e + 1;
    }
    auto blank = [&](const std::pair<size_t, size_t>& l) { return text.find_first_not_of(" \t\r", l.first) >= l.second; };
    while (!lines.empty() && blank(lines.back())) lines.pop_back();
    if (lines.size() < 2) return rs_fail(ctx, RS_ERR_INVALID, "%s: no nodes", path);
    if (lines.size() > BOW_MAX_NODES) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "%s: more than %d nodes", path, BOW_MAX_NODES);
    // a line that ends early fails its own count: nothing is read across a '\n'.  A field ends at a blank or at the end of
    // its line, so "7x" is no number and the integer part of a weight is no byte of a line that lacks one
    auto ends = [](const char* p) { return *p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == '\0'; };
    auto ints = [&](const char*& p, long* v, int count) {
        for (int i = 0; i < count; i++) {
            while (*p == ' ' || *p == '\t') p++;
            if (*p == '\n' || *p == '\r' || *p == '\0') return false;
            char* e = nullptr;
            v[i] = strtol(p, &e, 10);
            if (e == p || !ends(e)) return false;
            p = e;
        }
        return true;
    };
    long hd[4];
    const char* p = text.c_str() + lines[0].first;
    if (!ints(p, hd, 4)) return rs_fail(ctx, RS_ERR_INVALID, "%s: line 1 is not 'k L scoring weighting'", path);
    const size_t n = lines.size();
    std::vector<int32_t> parent(n, -1);
    std::vector<uint8_t> desc(32 * n, 0), leaf(n, 0);
    std::vector<double> weight(n, 0.0);
    for (size_t i = 1; i < n; i++) {
        long v[34];
        p = text.c_str() + lines[i].first;
        if (blank(lines[i]) || !ints(p, v, 34)) return rs_fail(ctx, RS_ERR_INVALID, "%s: line %zu is not 'parent is_leaf b0 .. b31 weight'", path, i + 1);
        while (*p == ' ' || *p == '\t') p++;
        char* e = nullptr;
        if (*p != '\n' && *p != '\r' && *p != '\0') weight[i] = strtod(p, &e);
        if (!e || e == p || !ends(e)) return rs_fail(ctx, RS_ERR_INVALID, "%s: line %zu has no weight", path, i + 1);
        if (v[0] < 0 || v[0] > 0x7FFFFFFF) return rs_fail(ctx, RS_ERR_INVALID, "%s: line %zu: parent %ld", path, i + 1, v[0]);
        parent[i] = (int32_t)v[0];
        leaf[i] = v[1] > 0;
        for (int b = 0; b < 32; b++) {
            if (v[2 + b] < 0 || v[2 + b] > 255) return rs_fail(ctx, RS_ERR_INVALID, "%s: line %zu: byte %ld", path, i + 1, v[2 + b]);
            desc[32 * i + b] = (uint8_t)v[2 + b];
        }
    }
    auto narrow = [](long v) { return (int)std::max<long>(-1, std::min<long>(v, 1 << 20)); };
    return vocabulary_build(ctx, narrow(hd[0]), narrow(hd[1]), narrow(hd[3]), narrow(hd[2]), (int)n, parent.data(), desc.data(),
                            weight.data(), leaf.data(), out_voc);
}

extern "C" int rs_vocabulary_info(const rs_vocabulary* voc, int32_t* h_info)
{
    if (!voc || !h_info) return RS_ERR_INVALID;
    const int32_t v[6] = {voc->k, voc->L, voc->weighting, voc->scoring, voc->n_nodes, voc->n_words};
    memcpy(h_info, v, sizeof(v));
    return RS_OK;
}

extern "C" int rs_vocabulary_arrays(const rs_vocabulary* voc, int32_t* h_parent, uint8_t* h_descriptors, double* h_weight)
{
    if (!voc) return RS_ERR_INVALID;
    if (h_parent) memcpy(h_parent, voc->parent.data(), sizeof(int32_t) * voc->parent.size());
    if (h_descriptors) memcpy(h_descriptors, voc->desc.data(), voc->desc.size());
    if (h_weight) memcpy(h_weight, voc->weight.data(), sizeof(double) * voc->weight.size());
    return RS_OK;
}

extern "C" int rs_vocabulary_destroy(rs_vocabulary* voc) { return rs_drain_and_delete(voc); }

// ------------------------------------------------------------------------------------------------ rs_bow
extern "C" int rs_bow_create(rs_context* ctx, rs_vocabulary* voc, int max_points, rs_bow** out_bow)
{
    if (!ctx || !out_bow) return RS_ERR_INVALID;
    *out_bow = nullptr;
    if (!voc || voc->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null vocabulary, or one of another context");
    if (max_points < 1) return rs_fail(ctx, RS_ERR_INVALID, "bad max_points");
    if (max_points > BOW_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_points 1 .. %d", BOW_MAX_POINTS);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_bow* b = new rs_bow();
    b->ctx = ctx;
    b->voc = voc;
    b->max_points = max_points;
    const size_t m = (size_t)max_points, W = (size_t)voc->n_words;
    const int rc = b->block.carve(ctx, "bag-of-words scratch", [&](rs_carve& c) {
        b->d_feat_word = c.take<int32_t>(m);
        b->d_words = c.take<int32_t>(m);
        b->d_counts = c.take<int32_t>(m);
        b->d_values = c.take<double>(m);
        b->d_hdr = c.take<int32_t>(2);
        b->d_norm = c.take<double>(1);
        b->d_lookup = c.take<int32_t>(W);
    });
    if (rc != RS_OK) { delete b; return rc; }
    // an empty vector: on the context stream, ahead of the first transform
    if (hipMemsetAsync(b->d_hdr, 0, 8, ctx->stream) != hipSuccess || hipMemsetAsync(b->d_norm, 0, 8, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_lookup, 0, 4 * W, ctx->stream) != hipSuccess) {
        delete b;
        return rs_fail(ctx, RS_ERR_HIP, "bag-of-words scratch could not be cleared");
    }
    *out_bow = b;
    return RS_OK;
}

extern "C" int rs_bow_destroy(rs_bow* bow) { return rs_drain_and_delete(bow); }

extern "C" int rs_bow_transform(rs_context* ctx, rs_bow* bow, const uint8_t* d_desc, const int32_t* d_count, int max_n, int32_t* d_word)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!bow || bow->ctx != ctx || !d_desc || !d_count) return rs_fail(ctx, RS_ERR_INVALID, "null bag-of-words object, descriptors or count");
    if (max_n < 0) return rs_fail(ctx, RS_ERR_INVALID, "max_n must be >= 0");
    if (((uintptr_t)d_desc & 15) != 0) return rs_fail(ctx, RS_ERR_INVALID, "descriptor rows must be 16-byte aligned");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const rs_vocabulary* voc = bow->voc;
    const BowTree t{voc->d_desc, voc->d_info, std::min(voc->n_nodes, BOW_LDS_NODES)};
    const int most = std::min(max_n, bow->max_points);
    const int blocks = std::max(1, std::min((most + BOW_GROUPS - 1) / BOW_GROUPS, BOW_MAX_BLOCKS));
    {
        rs_prof_scope ps(ctx, "BOW0_descend");
        hipLaunchKernelGGL(bow_descend, dim3(blocks), dim3(BOW_THREADS), 0, ctx->stream, t, (const uint4*)d_desc, d_count, max_n,
                           bow->max_points, bow->d_feat_word, d_word, bow->d_hdr);
    }
    {
        const BowVec v{bow->d_words, bow->d_counts, bow->d_values, bow->d_hdr, bow->d_norm, bow->d_lookup};
        rs_prof_scope ps(ctx, "BOW1_reduce");
        hipLaunchKernelGGL(bow_reduce, dim3(1), dim3(BOW_THREADS), 0, ctx->stream, bow->d_feat_word, voc->d_word_weight, voc->weighting, v);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_bow_download(rs_context* ctx, const rs_bow* bow, int32_t* h_words, int32_t* h_counts, double* h_values,
                               int32_t* h_n_words, double* h_norm)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!bow || bow->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null bag-of-words object");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int32_t hdr[2] = {0, 0};
    RS_HIP(ctx, hipMemcpy(hdr, bow->d_hdr, 8, hipMemcpyDeviceToHost));
    const size_t m = (size_t)std::min(std::max(hdr[0], 0), bow->max_points);
    if (h_n_words) *h_n_words = (int32_t)m;
    if (h_norm) RS_HIP(ctx, hipMemcpy(h_norm, bow->d_norm, 8, hipMemcpyDeviceToHost));
    if (m && h_words) RS_HIP(ctx, hipMemcpy(h_words, bow->d_words, 4 * m, hipMemcpyDeviceToHost));
    if (m && h_counts) RS_HIP(ctx, hipMemcpy(h_counts, bow->d_counts, 4 * m, hipMemcpyDeviceToHost));
    if (m && h_values) RS_HIP(ctx, hipMemcpy(h_values, bow->d_values, 8 * m, hipMemcpyDeviceToHost));
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ database
extern "C" int rs_bow_database_create(rs_context* ctx, rs_vocabulary* voc, int max_entries, int max_total_words, rs_bow_database** out_db)
{
    if (!ctx || !out_db) return RS_ERR_INVALID;
    *out_db = nullptr;
    if (!voc || voc->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null vocabulary, or one of another context");
    if (max_entries < 1 || max_total_words < 1) return rs_fail(ctx, RS_ERR_INVALID, "bad database capacities");
    if (max_entries > BOW_MAX_ENTRIES || max_total_words > BOW_MAX_TOTAL_WORDS)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_entries 1 .. %d, max_total_words 1 .. %d", BOW_MAX_ENTRIES, BOW_MAX_TOTAL_WORDS);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_bow_database* db = new rs_bow_database();
    db->ctx = ctx;
    db->voc = voc;
    db->max_entries = max_entries;
    db->max_total_words = max_total_words;
    db->ptr.reserve((size_t)max_entries + 1);
    db->ptr.push_back(0);
    const int rc = db->block.carve(ctx, "bag-of-words database", [&](rs_carve& c) {
        db->d_ptr = c.take<int32_t>((size_t)max_entries + 1);
        db->d_words = c.take<int32_t>((size_t)max_total_words);
        db->d_values = c.take<double>((size_t)max_total_words);
    });
    if (rc != RS_OK) { delete db; return rc; }
    if (hipMemsetAsync(db->d_ptr, 0, 4, ctx->stream) != hipSuccess) {
        delete db;
        return rs_fail(ctx, RS_ERR_HIP, "database could not be cleared");
    }
    *out_db = db;
    return RS_OK;
}

extern "C" int rs_bow_database_destroy(rs_bow_database* db) { return rs_drain_and_delete(db); }

extern "C" int rs_bow_database_add(rs_context* ctx, rs_bow_database* db, const rs_bow* bow, int32_t* h_entry)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!db || !bow || db->ctx != ctx || bow->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null database or bag-of-words object");
    if (db->voc != bow->voc) return rs_fail(ctx, RS_ERR_INVALID, "the database and the vector belong to different vocabularies");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    void* pin = nullptr;
    int rc = rs_pinned(ctx, sizeof(int32_t), &pin);
    if (rc) return rc;
    RS_HIP(ctx, hipMemcpyAsync(pin, bow->d_hdr, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));            // the one read-back: the vector's word count
    const int m = *(const int32_t*)pin, entries = (int)db->ptr.size() - 1, used = db->ptr.back();
    if (m < 0 || m > bow->max_points) return rs_fail(ctx, RS_ERR_HIP, "corrupt word count %d", m);
    if (entries >= db->max_entries) return rs_fail(ctx, RS_ERR_NOMEM, "the database is full: %d entries", entries);
    if (m > db->max_total_words - used)
        return rs_fail(ctx, RS_ERR_NOMEM, "the database holds %d of %d words: no room for %d more", used, db->max_total_words, m);
    if (m) {
        RS_HIP(ctx, hipMemcpyAsync(db->d_words + used, bow->d_words, 4 * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
        RS_HIP(ctx, hipMemcpyAsync(db->d_values + used, bow->d_values, 8 * (size_t)m, hipMemcpyDeviceToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(bow_set_int, dim3(1), dim3(1), 0, ctx->stream, db->d_ptr + entries + 1, used + m);
    RS_HIP(ctx, hipGetLastError());
    db->ptr.push_back(used + m);
    if (h_entry) *h_entry = entries;
    return RS_OK;
}

extern "C" int rs_bow_database_score(rs_context* ctx, const rs_bow_database* db, const rs_bow* bow, int first, int count, double* d_score)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!db || !bow || db->ctx != ctx || bow->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null database or bag-of-words object");
    if (db->voc != bow->voc) return rs_fail(ctx, RS_ERR_INVALID, "the database and the vector belong to different vocabularies");
    const int entries = (int)db->ptr.size() - 1;
    if (first < 0 || count < 0 || first > entries || count > entries - first)
        return rs_fail(ctx, RS_ERR_INVALID, "entries %d .. %d of %d", first, first + count - 1, entries);
    if (count == 0) return RS_OK;
    if (!d_score) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((count + BOW_SCORE_WAVES - 1) / BOW_SCORE_WAVES), block(64 * BOW_SCORE_WAVES);
    rs_prof_scope ps(ctx, "BOW2_score");
    if (ctx->bow_score_mode == 0)
        hipLaunchKernelGGL(bow_score<true>, grid, block, 0, ctx->stream, db->d_ptr, db->d_words, db->d_values, first, count, bow->d_lookup,
                           bow->d_words, bow->d_values, bow->d_hdr, d_score);
    else
        hipLaunchKernelGGL(bow_score<false>, grid, block, 0, ctx->stream, db->d_ptr, db->d_words, db->d_values, first, count, bow->d_lookup,
                           bow->d_words, bow->d_values, bow->d_hdr, d_score);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_bow_database_counts(const rs_bow_database* db, int32_t* h_entries, int32_t* h_total_words)
{
    if (!db) return RS_ERR_INVALID;
    if (h_entries) *h_entries = (int32_t)db->ptr.size() - 1;
    if (h_total_words) *h_total_words = db->ptr.back();
    return RS_OK;
}
