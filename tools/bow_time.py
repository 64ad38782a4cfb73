#!/usr/bin/env python3
"""GPU time of key-frame recognition (csrc/bow.hip) by HIP events on the context stream, with a synthetic 10-way
6-level vocabulary (synth.make_vocabulary: 1 111 111 nodes, 10^6 words) and 2000 descriptors: rs_bow_transform alone,
rs_bow_database_score against 1000 and 4000 entries (each the vector of 2000 rows drawn from a pool of 20000; both forms
of the query lookup, "bow_score_mode" 0 and 1), and rs_describe_features -> rs_bow_transform -> rs_bow_database_score
(4000 entries) at 1920x1080 with no host synchronisation in between.  Median / min of --reps after --warmup.

    python tools/bow_time.py [--reps 200] [--warmup 20] [--json out.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bow_time.py --reps 50`.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--entries", type=int, default=4000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    t = synth.make_vocabulary(a.k, a.levels)
    voc = ctx.vocabulary(t["k"], t["L"], 0, 0, t["parent"], t["desc"], t["weight"])
    n = a.points
    bow, db = ctx.bow(voc, 8192), ctx.bow_database(voc, a.entries, a.entries * n)
    pool = ctx.dev(synth.make_bow_descriptors(t, 10 * n, equidistant_fraction=0.0))
    d_n = ctx.dev(np.array([n], np.int32))
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(a.entries):
        rows = pool[torch.randint(0, len(pool), (n,), generator=g).to(pool.device)].contiguous()
        bow.transform(rows, d_n, n, words=False)
        db.add(bow)
    query = pool[torch.randint(0, len(pool), (n,), generator=g).to(pool.device)].contiguous()
    d_word = ctx.empty((n,), torch.int32)
    scores = ctx.empty((a.entries,), torch.float64)
    stream = torch.cuda.current_stream()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        ts.sort()
        return dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1))

    def transform():
        ctx._check(ctx.lib.rs_bow_transform(ctx.h, bow.h, rs._dp(query), rs._dp(d_n), n, rs._dp(d_word)), "rs_bow_transform")

    def score(count):
        return lambda: db.score(bow, 0, count, out=scores)

    transform()
    small = min(1000, a.entries)
    res = dict(k=voc.k, levels=voc.L, nodes=voc.n_nodes, words=voc.n_words, points=n, entries=a.entries, reps=a.reps,
               transform=timed(transform))
    res[f"score_{small}"] = timed(score(small))
    res[f"score_{a.entries}"] = timed(score(a.entries))
    ctx.set_int("bow_score_mode", 1)
    res[f"score_{small}_binary_search"] = timed(score(small))
    res[f"score_{a.entries}_binary_search"] = timed(score(a.entries))
    ctx.set_int("bow_score_mode", 0)
    # the chain from pixels' descriptors: describe -> transform -> score on the device count
    d = synth.make_klt_pair(2)
    W, H = d["width"], d["height"]
    im, ds = ctx.image(W, H, frame=d["img2"]), ctx.describer(W, H, 8192)
    d_pts, d_cnt = ctx.dev(d["pts"][:n]), ctx.dev(np.array([min(n, len(d["pts"]))], np.int32))
    out_o = ctx.describe_features(ds, im, None, None, None, None, 0, d_pts, d_cnt)

    def chain():
        ctx.describe_features(ds, im, None, None, None, None, 0, d_pts, d_cnt, out=out_o)
        ctx._check(ctx.lib.rs_bow_transform(ctx.h, bow.h, rs._dp(out_o["desc"]), rs._dp(out_o["n"]), n, None), "rs_bow_transform")
        db.score(bow, 0, a.entries, out=scores)

    res["describe_transform_score"] = timed(chain)
    res.update(width=W, height=H, query_words=len(bow.download()["words"]), database_words=db.counts()[1])
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for x in (im, ds, bow, db, voc):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
