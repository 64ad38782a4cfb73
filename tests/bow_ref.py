"""CPU restatement (numpy, no DBoW2) of key-frame recognition: the vocabulary tree, the bag-of-words transform, L1
scoring and LoopDetector's candidate ranking.  It is the specification of csrc/bow.hip and rs_rank_loop_candidates.

What it restates (reference lines):
  thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424  loadFromTextFile: line 1 "k L scoring weighting", then one
        line per node after the root, "parent is_leaf b0 .. b31 weight"; node ids are line numbers, a node's children
        are in file order (= ascending id), leaves become words 0 .. W-1 in file order.  The reference's
        while(!f.eof()) loop makes one extra node from the empty last line; that is NOT restated: a trailing blank
        line is ignored.  A line is read with operator>>: any run of blanks separates fields and whatever follows
        the weight is ignored; a line with fewer fields, a field that is no number or a byte outside 0 .. 255 (which
        the reference would take without a word) raises ValueError here.
  TemplatedVocabulary.h:1218-1259  descent of one feature: from the root to the child of smallest Hamming distance,
        strict '<' (the first child among equals), until a leaf; the word is the leaf's word id, with its weight.
  TemplatedVocabulary.h:1066-1122  transform: stopped words (weight <= 0) dropped; TF_IDF / TF add the weight once per
        occurrence, IDF / BINARY once per word; L1 scoring normalises.
  BowVector.cpp:34-84              addWeight / addIfNotExist / normalize (divide by the sum of |v| if it is > 0).
  ScoringObject.cpp:23-68          L1Scoring::score: over shared words s = sum(|v-w| - |v| - |w|), score = -s / 2.
  FORB.cpp:81-101                  the 256-bit population count (here: numpy's bit counts of the xor).
  src/LoopDetector.cpp:64-73, :231-265, :346-373   percentile, rank_candidates, score_candidates.
Where the reference would index out of range (a node with more than k children, a parent not below the node, a leaf
flag that contradicts the children, a scoring type other than L1) the restatement raises ValueError.
std::sort leaves ties among equal scores unspecified; here equal scores keep their considered order.
"""
import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM = 0
MAX_K, MAX_L, MAX_NODES = 20, 10, 4194304

# LoopDetector.cpp:28-32
MIN_LOOP_SECONDS = 10.0
MIN_KEYFRAME_GAP = 50
TOP_CANDIDATES = 3
PEAK_OVER_MEDIAN = 1.25
MIN_BOW_SCORE = 0.02

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """Bit count of a ^ b over the last axis (32 bytes)."""
    return _POP8[np.bitwise_xor(a, b)].sum(-1)


class Vocabulary:
    """Arrays in node order: parent [n] i32 (parent[0] = -1), desc [n][32] u8, weight [n] f64."""

    def __init__(self, k, L, weighting, scoring, parent, desc, weight, is_leaf=None):
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        n = len(parent)
        if not (1 <= k <= MAX_K and 1 <= L <= MAX_L and 2 <= n <= MAX_NODES):
            raise ValueError("outside the envelope")
        if weighting not in (TF_IDF, TF, IDF, BINARY):
            raise ValueError("unknown weighting")
        if scoring != L1_NORM:
            raise ValueError("only L1 scoring")
        if len(desc) != n or len(weight) != n:
            raise ValueError("array lengths differ")
        ids = np.arange(n)
        if np.any(parent[1:] < 0) or np.any(parent[1:] >= ids[1:]):
            raise ValueError("a parent is not below its node")
        n_children = np.bincount(parent[1:], minlength=n)
        if n_children.max() > k:
            raise ValueError("a node has more than k children")
        if is_leaf is not None:
            is_leaf = np.asarray(is_leaf).astype(bool)
            if np.any(is_leaf[1:] != (n_children[1:] == 0)):
                raise ValueError("a leaf flag contradicts the node's children")
        self.k, self.L, self.weighting, self.scoring = int(k), int(L), int(weighting), int(scoring)
        self.parent, self.desc, self.weight = parent, desc, weight
        self.n_nodes = n
        # children in ascending node id (the loader's push_back order)
        order = np.argsort(parent[1:], kind="stable") + 1
        self.child_ptr = np.concatenate([[0], np.cumsum(n_children)]).astype(np.int64)
        self.child = order.astype(np.int32)
        self.leaf = n_children == 0
        self.word_of = np.full(n, -1, np.int32)
        self.word_of[self.leaf] = np.arange(int(self.leaf.sum()), dtype=np.int32)
        self.node_of_word = np.flatnonzero(self.leaf).astype(np.int32)
        self.n_words = len(self.node_of_word)
        self.word_weight = weight[self.node_of_word]

    def children(self, node):
        return self.child[self.child_ptr[node]:self.child_ptr[node + 1]]


# ------------------------------------------------------------------------------------------------ text format
def write_text(voc, path):
    """saveToTextFile's layout; weights as repr() so that they read back exactly."""
    with open(path, "w") as f:
        f.write(f"{voc.k} {voc.L} {voc.scoring} {voc.weighting}\n")
        for i in range(1, voc.n_nodes):
            f.write(f"{int(voc.parent[i])} {int(voc.leaf[i])} " + " ".join(str(int(b)) for b in voc.desc[i]) +
                    f" {float(voc.weight[i])!r}\n")


def parse_text(path):
    with open(path) as f:
        lines = f.read().split("\n")
    while lines and not lines[-1].strip():
        lines.pop()
    k, L, scoring, weighting = (int(v) for v in lines[0].split())
    n = len(lines)
    parent = np.full(n, -1, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    weight = np.zeros(n, np.float64)
    is_leaf = np.zeros(n, bool)
    for i in range(1, n):
        t = lines[i].split()
        if len(t) < 35:                                         # (fields past the weight are not read, as in the reference)
            raise ValueError(f"line {i + 1}: {len(t)} fields")
        parent[i], is_leaf[i] = int(t[0]), int(t[1]) > 0
        row = [int(v) for v in t[2:34]]
        if min(row) < 0 or max(row) > 255:
            raise ValueError(f"line {i + 1}: a descriptor byte outside 0 .. 255")
        desc[i] = row
        weight[i] = float(t[34])
    return Vocabulary(k, L, weighting, scoring, parent, desc, weight, is_leaf)


# ------------------------------------------------------------------------------------------------ descent, transform
def descend(voc, desc):
    """Word id per feature row ([n] i32).  All features step one level at a time; a feature at a leaf stays there."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    node = np.zeros(len(desc), np.int64)
    while True:
        live = np.flatnonzero(~voc.leaf[node])
        if not len(live):
            break
        cur = node[live]
        best_d = np.full(len(live), 1 << 30, np.int64)
        best_c = np.zeros(len(live), np.int64)
        first, cnt = voc.child_ptr[cur], voc.child_ptr[cur + 1] - voc.child_ptr[cur]
        for j in range(int(cnt.max())):
            has = j < cnt
            c = voc.child[np.where(has, first + j, 0)]
            d = hamming(desc[live], voc.desc[c])
            better = has & (d < best_d)                         # strict: the first child among equals
            best_d = np.where(better, d, best_d)
            best_c = np.where(better, c, best_c)
        node[live] = best_c
    return voc.word_of[node].astype(np.int32)


def transform(voc, desc):
    """dict(word_of_feature [n] i32, words [m] i32 ascending, counts [m] i32, values [m] f64, norm f64)."""
    wid = descend(voc, desc)
    acc, cnt = {}, {}
    add_each = voc.weighting in (TF_IDF, TF)
    for w in wid.tolist():
        wt = float(voc.word_weight[w])
        if not wt > 0:
            continue                                            # stopped
        cnt[w] = cnt.get(w, 0) + 1
        if w not in acc:
            acc[w] = wt
        elif add_each:
            acc[w] = acc[w] + wt
    words = np.array(sorted(acc), np.int32)
    values = np.array([acc[w] for w in words.tolist()], np.float64)
    counts = np.array([cnt[w] for w in words.tolist()], np.int32)
    norm = 0.0
    for v in values.tolist():
        norm += abs(v)
    if norm > 0.0:
        values = values / norm
    return dict(word_of_feature=wid, words=words, counts=counts, values=values, norm=norm)


def score(a, b):
    """L1Scoring::score of two transform() results: a merge over the two sorted word lists."""
    wa, va, wb, vb = a["words"], a["values"], b["words"], b["values"]
    i = j = 0
    s = 0.0
    while i < len(wa) and j < len(wb):
        if wa[i] == wb[j]:
            v, w = float(va[i]), float(vb[j])
            s += abs(v - w) - abs(v) - abs(w)
            i += 1
            j += 1
        elif wa[i] < wb[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0


# ------------------------------------------------------------------------------------------------ ranking
def percentile(values, fraction):
    """LoopDetector.cpp:64-73 in f32."""
    if not len(values):
        return np.float32(0.0)
    v = np.sort(np.asarray(values, np.float32))
    idx = min(len(v) - 1, int(np.float32(fraction) * np.float32(len(v) - 1)))
    return v[idx]


def score_candidates(scores, frame_index, query_frame_index, seconds_per_frame, min_keyframe_gap=MIN_KEYFRAME_GAP,
                     min_loop_seconds=MIN_LOOP_SECONDS):
    """:346-373 over entries i < query = len(scores): (entries [c] i32, scores [c] f32) of the considered ones."""
    q = len(scores)
    ent, sc = [], []
    for i in range(q):
        if q - i < min_keyframe_gap:
            continue
        dt = float(int(query_frame_index) - int(frame_index[i])) * float(seconds_per_frame)
        if dt < min_loop_seconds:
            continue
        ent.append(i)
        sc.append(np.float32(scores[i]))
    return np.array(ent, np.int32), np.array(sc, np.float32)


def rank_candidates(entries, scores, min_score=MIN_BOW_SCORE, peak_over_median=PEAK_OVER_MEDIAN, top=TOP_CANDIDATES):
    """:231-265.  dict(entries, scores: the ranked ones; rejected: (entry, score) of the best considered entry when
    none passes and some were considered, else None)."""
    scores = np.asarray(scores, np.float32)
    median = percentile(scores, 0.5)
    thresh = max(np.float32(min_score), np.float32(median * np.float32(peak_over_median)))
    keep = []
    n = len(scores)
    for i in range(n):
        if scores[i] < thresh:
            continue
        left = np.float32(0.0) if i == 0 else scores[i - 1]
        right = np.float32(0.0) if i + 1 == n else scores[i + 1]
        if scores[i] < left or scores[i] < right:
            continue
        keep.append(i)
    keep.sort(key=lambda i: -float(scores[i]))                  # stable: equal scores keep their considered order
    keep = keep[:top]
    rejected = None
    if not keep and n:
        b = int(np.argmax(scores))                              # max_element: the first maximum
        rejected = (int(entries[b]), np.float32(scores[b]))
    return dict(entries=np.array([entries[i] for i in keep], np.int32), scores=np.array([scores[i] for i in keep], np.float32),
                rejected=rejected)


def retrieve(scores, frame_index, query_frame_index, seconds_per_frame, **kw):
    """score_candidates + rank_candidates: what rs_rank_loop_candidates computes."""
    gate = {k: kw.pop(k) for k in ("min_keyframe_gap", "min_loop_seconds") if k in kw}
    e, s = score_candidates(scores, frame_index, query_frame_index, seconds_per_frame, **gate)
    return rank_candidates(e, s, **kw)
