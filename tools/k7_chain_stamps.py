#!/usr/bin/env python3
"""Chain-wave times of K7 (RS_STAMPS=1 build, workgroup of set 0), us per launch, averaged over the launches of one cfg-3 solve:
wait for the tile waves' set-up | set-up wait + factor loop | end of the loop -> end of the backward substitution; then the K7 body stamps."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("racing-slam_amd")
rs, synth = pkg.rsgpu, pkg.synth

ctx = rs.Context(0)
for k, v in (a.split("=") for a in sys.argv[1:] if "=" in a):
    ctx.set_int(k, int(v))
w = synth.make_ba_window()
dev = [ctx.dev(w[k]) for k in ("obs_ptr", "obs_cam", "obs_uv")]
for rep in range(2):
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    ctx.bundle_adjust(dc, w["cam_free"], dp, *dev, w["K"])
    ctx.synchronize()
    c = ctx.prof_counters(48)
    st = ctx.ba_stats()
    st["rounds"] = max(int(c[31]), 1)        # launches the stamping workgroup (set 0) went through the loop
    print(sys.argv[1:], "us per launch: set-up wait", round(c[22] / st["rounds"] / 100, 2), "set-up + loop", round(c[30] / st["rounds"] / 100, 2), "loop end -> backsub done", round(c[25] / st["rounds"] / 100, 2),
          "| K7 body stamps", [round(v / st["rounds"]) for v in c[:8]])
ctx.close()
