"""The scenes of tests/test_loop_cpu.py and tests/test_gpu_loop.py (synth.loop_scene) and their restatement results,
computed once per process."""
import functools
import importlib

import numpy as np

import loop_ref as L
import pnp_ref as P

# name -> (seed, nq, candidates (n, matched, shared, outlier_frac, strip)); what each candidate is there for
SCENES = {
    "paths": (1, 300, ((400, 200, 70, 0.3, None),           # 0 verified
                       (60, 0, 0, 0.0, None),               # 1 nt = 0                      -> status 1
                       (60, 1, 1, 0.0, None),               # 2 nt = 1 (K1's no-ratio path) -> status 1
                       (100, 11, 11, 0.0, None),            # 3 11 matched                  -> status 1
                       (200, 100, 40, 1.0, None),           # 4 every match wrong           -> status 2
                       (300, 100, 16, 0.0, None),           # 5 fewer than 20 inliers
                       (300, 150, 90, 0.7, None),           # 6 inlier ratio below 0.35
                       (300, 120, 50, 0.0, (0.40, 0.55)))), # 7 all inliers in a narrow strip
    "big": (2, 300, ((2500, 1100, 120, 0.3, None),          # the compaction crosses chunk boundaries, nt > one block
                     (400, 200, 60, 0.2, None))),
}
EXPECT = {"paths": [(0, True), (1, False), (1, False), (1, False), (2, False), (0, False), (0, False), (0, False)],
          "big": [(0, True), (0, True)]}


def synth():
    return importlib.import_module("racing-slam_amd").synth


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, nq, cands = SCENES[name]
    return synth().loop_scene(seed, nq, cands)


@functools.lru_cache(maxsize=None)
def reference(name):
    """loop_ref.verify_pnp of every candidate of the scene against its query (the reference's constants, seed 0)."""
    s = scene(name)
    q = s["key_frames"][s["query"]]
    return [L.verify_pnp(q, s["key_frames"][c], s["points"], s["K"], s["width"]) for c in range(s["query"])]


def near_threshold(s, r):
    """The correspondences of a verification within test_gpu_pnp.py's band of the final model: |e^2 - thr^2| <= 1e-9 thr^2."""
    if r["pnp"] is None:
        return np.zeros(len(r["mq"]), bool)
    q = s["key_frames"][s["query"]]
    X, Y, Z, x, y, fin = P.prepare(r["obj"], q["kp"], s["K"], r["mt"], r["mq"])
    zc, e2 = P.reproj2(r["pnp"]["Rt"], X, Y, Z, x, y, float(s["K"][0]), float(s["K"][1]))
    thr2 = r["pnp"]["thr2"]
    return fin & (np.abs(e2 - thr2) <= 1e-9 * thr2)
