"""What tests/test_gpu_loop.py and tests/test_gpu_loop_envelope.py share: a scene in an rs_map with the mirror the tests keep
of it, and the two comparison layers (the rules are in tests/test_gpu_loop.py's docstring)."""
import numpy as np

import loop_cases as S
import loop_ref as L
import match_ref


class Built:
    """A scene in an rs_map, with the mirror the tests keep of it (kp_point per key frame, positions)."""

    def __init__(self, ctx, rs, s):
        self.s, self.map = s, rs.ResidentMap(ctx)
        self.frames = [rs.ResidentFrame(ctx, k["kp"], k["desc"]) for k in s["key_frames"]]
        for k, f in zip(s["key_frames"], self.frames):
            self.map.add_keyframe(f, k["pose"])
        for xyz in s["points"]:
            self.map.add_point(xyz)
        for p, k, i in s["observations"]:
            self.map.add_observation(p, k, i)
        self.kp_point = [k["kp_point"].copy() for k in s["key_frames"]]
        self.pos = s["points"].copy()

    def close(self):
        self.map.close()
        for f in self.frames:
            f.close()


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _check(ver, b, cands, got, refs=None, max_distance=64):
    """Every candidate of one call: the exact layer, and end to end where the restatement's results are given (refs: per key
    frame, a list or a dict; a key frame a dict leaves out gets the exact layer only).  max_distance: the call's."""
    s = b.s
    q = s["key_frames"][s["query"]]
    qc = L.centre_of(q["pose"])
    for c, (kf, g) in enumerate(zip(cands, got)):
        k = s["key_frames"][kf]
        d = ver.download(c)
        rows = L.candidate_rows(b.kp_point[kf])
        assert d["nt"] == len(rows) and np.array_equal(d["keypoints"], rows)
        assert np.array_equal(d["slots"], b.kp_point[kf][rows]) and np.array_equal(d["rows"], k["desc"][rows])
        assert np.array_equal(d["positions"], b.pos[b.kp_point[kf][rows]])
        mq, mt = match_ref.match_descriptors(q["desc"], k["desc"][rows], max_distance)
        assert np.array_equal(d["match_query"], mq) and np.array_equal(d["match_train"], mt)
        # PnP reports inliers only with its status 0 (include/rsgpu.h), so "PnP status != 0 or no inliers" is "no inliers"
        # here; that PnP's status itself is read right is covered end to end below, against loop_ref's status
        status = 1 if len(mq) < 12 else (0 if len(d["inlier_index"]) else 2)
        f = L.finish(status, g["pose"], d["inlier_index"], mq, mt, rows, b.kp_point[kf], q["kp"], s["width"], qc, L.centre_of(k["pose"]))
        print(kf, {n: g[n] for n in ("status", "ok", "correspondences", "inliers", "listed", "spread", "drift", "gap")})
        for n in ("status", "ok", "correspondences", "inliers", "listed"):
            assert g[n] == f[n], (kf, n, g[n], f[n])
        for n in ("spread", "drift", "gap"):
            assert _bits(g[n]) == _bits(f[n]), (kf, n, g[n], f[n])
        for n in ("query_kp", "point", "candidate_kp"):
            assert np.array_equal(g[n], f[n]), (kf, n)
        if status != 0:
            assert np.array_equal(g["pose"], np.eye(4, dtype=np.float32)) and len(d["inlier_index"]) == 0
        if refs is None or (isinstance(refs, dict) and kf not in refs):
            continue
        r = refs[kf]
        assert (g["status"], g["correspondences"], g["ok"]) == (r["status"], r["correspondences"], r["ok"]), kf
        assert np.allclose(g["pose"], r["pose"], atol=1e-5), kf
        if r["status"] == 0:
            near = S.near_threshold(s, r)
            mask = np.zeros(len(mq), bool)
            mask[d["inlier_index"]] = True
            assert np.array_equal(mask[~near], r["pnp"]["mask"].astype(bool)[~near]), kf


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for n in x:
            assert np.asarray(x[n]).tobytes() == np.asarray(y[n]).tobytes(), n
