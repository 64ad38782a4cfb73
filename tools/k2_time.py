#!/usr/bin/env python3
"""Times K2 (rs_reproj_match) alone on the benchmark scene (20 KF / 10 k landmarks / 2000 keypoints).

    python tools/k2_time.py [n_keypoints]

More than 6144 keypoints do not fit in LDS: both k2_mode values then run the one-lane kernel's walk over global memory,
unless the frame's cell grid is used (k2_mode 0 with k2_grid 1, the default), which does not depend on the tree's size."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("racing-slam_amd")
rs, synth = pkg.rsgpu, pkg.synth
import torch  # noqa: E402

n_keypoints = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ctx = rs.Context(0)
w = synth.make_ba_window()
frame, mp = synth.make_match_scene(w, n_keypoints=n_keypoints, kdtree_build=rs.kdtree_build)
fv, keep_f = ctx.make_frame_view(frame, pack=True)
mv, keep_m = ctx.make_map_view(mp)
has_grid = bool(fv.d_kd_grid)                        # (a parent library under RS_LIB has none)
for mode, grid in ((0, 1), (0, 0), (1, 0)) if has_grid else ((0, 0), (1, 0)):      # cell grid / eight lanes per map point / one lane per point
    ctx.set_int("k2_mode", mode)
    if has_grid:
        ctx.set_int("k2_grid", grid)
    out = ctx.reproj_match(fv, mv)
    for _ in range(20):
        ctx.reproj_match(fv, mv, out=out)
    ctx.synchronize()
    ctx.prof_begin()
    for _ in range(200):
        ctx.reproj_match(fv, mv, out=out)
    ctx.synchronize()
    p = ctx.prof_end()
    n = int(out["count"].item())
    sums = [int(out[k][:m].to(torch.int64).sum().item()) for k, m in (("point_kp", mv.n_points), ("point_dist", mv.n_points),
                                                                       ("match_kp", n), ("match_point", n))]
    print("n_keypoints", n_keypoints, "k2_mode", mode, "k2_grid", grid, {k: round(1e3 * v[1] / v[0], 2) for k, v in p.items()},
          "matches", n, "sums", sums, flush=True)
ctx.close()
