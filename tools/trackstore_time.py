#!/usr/bin/env python3
"""Time of the device track store (csrc/track_store.hip) at 2000 and 8192 keypoints, max_sightings = 100, about 70 % of
the tracks carried from frame to frame, in one run on one GPU.  Median / min of --reps after --warmup.

  (a) frame_chain       rs_track_store_carry -> rs_track_store_query -> rs_track_store_extend: what a frame that does not
                        become a key frame costs.  The query ends in the chain's one host synchronisation (24 bytes), so
                        wall clock and HIP events bracket the same work; both are given.
  (b) key_frame_chain   rs_track_store_triangulate (pack, rs_triangulate_tracks, result filter, one read-back) and
                        rs_track_store_erase_inconsistent, on tracks of a static scene seen from a moving camera.
  (c) forms             the device form against the host form it replaces, both from C++ in ONE process
                        (tests/host_cpp/test_trackstore_host.bin --time): per frame slam::DeviceTracks' carry_forward,
                        needs_key_frame, extend against five read-backs (inlier count and list, kept-index list, keypoints,
                        match table) and slam::HostTrackStore's std::map pass; per key frame DeviceTracks::triangulate_tracks
                        + erase against the CSR built from the std::map, its upload, rs_triangulate_tracks, the read-back
                        of its outputs and the erase.  Wall clock around a synchronised chain.
  (d) kernels           mean device time per kernel from the library's own event brackets (rs_prof_begin / rs_prof_end);
                        the key-frame kernels are profiled on the store the key-frame wall time was measured on, before
                        the frame chain turns its tracks over.
For the kernel trace (profiles/trackstore_kernel_stats.csv) run it under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/trackstore_time.py --reps 50`.

    python tools/trackstore_time.py [--reps 200] [--warmup 20] [--json profiles/trackstore_time.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs = pkg.rsgpu
    ctx = rs.Context(0)
    stream = torch.cuda.current_stream()

    def stat(ts):
        ts = sorted(ts)
        return dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1))

    def wall(fn, reps=None):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(reps or a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(1e6 * (time.perf_counter() - t0))
        return stat(ts)

    def events(fn):
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
        return stat(ts)

    res = dict(reps=a.reps, warmup=a.warmup, max_sightings=100, sizes={})
    K = (1000.0, 1000.0, 960.0, 540.0)
    for n in (2000, 8192):
        rng = np.random.default_rng(n)
        frames = 14
        X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], axis=1)
        poses = np.tile(np.eye(4, dtype=np.float32), (frames, 1, 1))
        pix = np.zeros((frames, n, 2), np.float32)
        for f in range(frames):
            poses[f, 0, 3] = -0.1 * f
            pix[f, :, 0] = K[0] * (X[:, 0] - 0.1 * f) / X[:, 2] + K[2]
            pix[f, :, 1] = K[1] * X[:, 1] / X[:, 2] + K[3]
        st = rs.TrackStore(ctx, 8192, 100)
        fr = [rs.ResidentFrame(ctx, pix[f], np.zeros((n, 32), np.uint8)) for f in range(frames)]
        d_prev = ctx.dev(np.arange(n, dtype=np.int32))
        inl = [np.flatnonzero(rng.random(n) < 0.7).astype(np.int32) for _ in range(frames)]
        d_inl = [ctx.dev(np.concatenate([i, np.zeros(n - len(i), np.int32)])) for i in inl]
        d_cnt = [ctx.dev(np.array([len(i)], np.int32)) for i in inl]
        table = np.full(n, -1, np.int32)
        table[rng.choice(n, n // 3, replace=False)] = np.arange(n // 3)
        last = fr[frames - 1]
        last.matches_add(ctx.dev(np.flatnonzero(table >= 0).astype(np.int32)), ctx.dev(table[table >= 0]))
        st.extend(fr[0], 0, 0)
        for f in range(1, frames - 1):
            st.carry(d_prev, d_inl[f], d_cnt[f], n)
            st.extend(fr[f], f, f // 5 if f % 5 == 0 else -1)
        d_poses = ctx.dev(poses.reshape(frames, 16))
        q = st.query(last)
        r = dict(live_tracks=q["live"], waiting=q["waiting"])

        def key_frame():
            got = st.triangulate(last, d_poses, 0, frames - 1, K)
            st.erase_inconsistent()
            return got

        got = key_frame()
        r["key_frame"] = dict(accepted=int(got["counts"][0]), inconsistent=int(got["counts"][2]), key_frame_pairs=got["n_pairs"])
        r["key_frame_chain_wall"] = wall(lambda: (key_frame(), ctx.synchronize()))
        ctx.prof_begin()
        for _ in range(20):
            key_frame()
        prof = ctx.prof_end()
        r["key_frame_kernels_mean_us"] = {k: round(1e3 * ms / max(cnt, 1), 1) for k, (cnt, ms) in prof.items() if k.startswith(("KT_", "K6"))}
        state = dict(f=frames - 1)

        def frame_chain():
            f = state["f"] = state["f"] % (frames - 1) + 1
            st.carry(d_prev, d_inl[f], d_cnt[f], n)
            st.query(fr[f])
            st.extend(fr[f], 100 + f, -1)

        r["frame_chain_wall"] = wall(lambda: (frame_chain(), ctx.synchronize()))
        r["frame_chain_events"] = events(frame_chain)
        ctx.prof_begin()
        for _ in range(a.reps):
            frame_chain()
        prof = ctx.prof_end()
        r["frame_kernels_mean_us"] = {k: round(1e3 * ms / max(cnt, 1), 1) for k, (cnt, ms) in prof.items() if k.startswith("KT_")}
        res["sizes"][str(n)] = r
        for f in fr:
            f.close()
        st.close()
    ctx.close()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_trackstore_host
    out = subprocess.run([test_trackstore_host.build_trackstore_host(rs), "--time", str(a.reps)], capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.split("\n") if ln.startswith("{")]
    assert out.returncode == 0 and line, (out.stdout[-2000:], out.stderr[-2000:])
    res["forms"] = json.loads(line[-1])
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
