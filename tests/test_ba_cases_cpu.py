"""The case tables of tests/ba_cases.py, pinned on the CPU before tests/test_gpu_ba_envelope.py holds the GPU to them:
  the oracle's vision-only solve (orc_bundle_adjust) under every option case against the independent dense restatement
  (tests/dense_lm.py), on the PLAIN-size windows, with the comparison of test_inertial_ba_cpu.py;
  every case reaches what it exists for (termination, a moved state, a failed first factorisation, a rejected step in
  every hard window, unequal iteration counts inside the mixed batch);
  every (window, option) pair the GPU file compares exactly is well posed: with the input points scaled by 1 +- 1e-13 the
  oracle repeats its schedule and moves its results by at most a tenth of the GPU file's tolerances.  A pair that fails
  this is replaced in ba_cases.py, never tolerated: the GPU file has no skip list."""
import numpy as np
import pytest

import ba_cases as B
import ba_compare as CMP
import dense_lm as D

BASE = [w for w in B.WINDOWS if not w.endswith("_hard")]
HARDS = [w for w in B.WINDOWS if w.endswith("_hard")]
DENSE = B.pairs(["plain", "plain_hard"])
# what the GPU file compares: every option on the window of every path class, HARD_OPTIONS on the hard twins
GPU_PAIRS = B.pairs(BASE) + B.pairs(HARDS, B.HARD_OPTIONS)
STRUCTURE = [(w, e) for w in B.STRUCTURE_WINDOWS for e in B.STRUCTURE]
BATCH_WINDOWS = [(b, i) for b, c in B.BATCHES.items() for i in range(len(c["windows"])) if not c["windows"][i].get("empty")]

_SOLVED = {}


def _solved(oracle, synth, wn, on):
    """window, options, oracle result of a pair (solved once per session)."""
    if (wn, on) not in _SOLVED:
        w, opt = B.window(synth, wn, on), B.opt_of(wn, on)
        _SOLVED[wn, on] = (w, opt, B.solve_oracle(oracle, w, opt))
    return _SOLVED[wn, on]


def _ids(pairs):
    return ["-".join(map(str, p)) for p in pairs]


def test_tables_are_complete():
    """Every vision-only path of test_gpu_ba_paths.CASES is there, every class has a hard twin, every option applies to the
    window of every class except where TUNED says that no value reaches the case, and those gaps are covered by the twin."""
    assert set(B.PATHS) == {k for k, (kind, _, _) in B.P.CASES.items() if kind != "inertial"} and len(B.PATHS) == 12
    assert {c for _, c, _ in B.PATHS.values()} == set(BASE)
    for w in BASE:
        missing = [o for o in B.OPTIONS if not B.applies(w, o)]
        assert all(B.OPTIONS[o].get("moved") or o == "radius_huge" for o in missing), (w, missing)
    assert {o for w, o in B.EXCLUDED if w in BASE} == {"radius_huge"} and B.applies("plain", "radius_huge") and B.applies("wide", "radius_huge")
    assert set(B.SETS) <= set(B.HARD_OPTIONS) <= set(B.OPTIONS)


@pytest.mark.parametrize("wn,on", DENSE, ids=_ids(DENSE))
def test_oracle_matches_dense_lm(oracle, synth, wn, on):
    w, opt, (c, p, s, tr) = _solved(oracle, synth, wn, on)
    dc, dp, ds, dtr = B.solve_dense(D, oracle, w, opt)
    assert [s[k] for k in CMP.SCHEDULE] == [ds[k] for k in CMP.SCHEDULE]
    assert B.outcomes(tr) == B.outcomes(dtr)
    for k, tol in (("radius", 1e-8), ("cost", 1e-10), ("candidate_cost", 1e-9), ("model_cost_change", 1e-7)):
        assert np.allclose([t[k] for t in tr], [t[k] for t in dtr], rtol=tol, equal_nan=True), k
    if not s["usable"]:            # nothing moves: the inputs come back bit for bit
        assert c.tobytes() == w["cams"].tobytes() and p.tobytes() == w["points"].tobytes()
        return
    assert np.isclose(s["final_cost"], ds["final_cost"], rtol=1e-10)
    assert np.allclose(c, dc, rtol=1e-8, atol=1e-10)
    assert np.allclose(p, dp, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("wn,on", GPU_PAIRS, ids=_ids(GPU_PAIRS))
def test_cases_reach_what_they_are_for(oracle, synth, wn, on):
    case = B.OPTIONS[on]
    w, opt, (c, p, s, tr) = _solved(oracle, synth, wn, on)
    if "expect" in case:
        assert s["termination"] == case["expect"]
    if case.get("poke"):
        assert s["iterations"] == 0 and not s["usable"] and not np.isfinite(s["initial_cost"])
    if case.get("moved"):
        assert s["successful_steps"] >= 1 and not s["usable"]
        assert c.tobytes() == w["cams"].tobytes() and p.tobytes() == w["points"].tobytes()
    if case.get("not_pd"):          # the very first factorisation fails (a failed factorisation reports no model change)
        assert tr[0]["outcome"] == B.INVALID and tr[0]["model_cost_change"] == 0.0 and s["successful_steps"] == 0
    invalid = [t for t in tr if t["outcome"] == B.INVALID]
    if case.get("tuned") in ("not_pd", "unusable"):
        n = opt["max_num_consecutive_invalid_steps"]
        assert len(invalid) == n and B.outcomes(tr).endswith("I" * n) and all(t["model_cost_change"] == 0.0 for t in invalid)
    else:                           # nowhere else does an invalid step appear (radius_huge: see ba_cases.EXCLUDED)
        assert not invalid
    if on == "max_iter_0":
        assert s["iterations"] == 0 and s["usable"] and tr == []
    if on == "gradient":
        assert s["iterations"] == 0 and s["usable"]
    if on == "default" and wn.endswith("_hard"):
        assert "R" in B.outcomes(tr)
    fixed = np.asarray(w["cam_free"]) == 0
    assert c[fixed].tobytes() == w["cams"][fixed].tobytes()


def _perturbed(w, seed):
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], w["points"].shape)
    return dict(w, points=w["points"] * (1.0 + 1e-13 * sign))


def _assert_stable(oracle, w, opt, ref):
    """Everything the GPU file compares, at a tenth of its tolerances, except the initial cost: that is a function of the
    input alone (the GPU gets the oracle's input bit for bit and is held to 1e-12 on it), and 1e-13 on the points moves it
    by up to 4e-12 by itself — |d cost| / cost ~ |r . J dp| / cost with J ~ f / z = 100 px per unit."""
    c, p, s, tr = ref
    for seed in (0, 1):
        pc, pp, ps, ptr = B.solve_oracle(oracle, _perturbed(w, seed), opt)
        CMP.assert_same_solve(dict(s=ps, tr=ptr, c=pc, p=pp), (c, p, None, None, s, tr), scale=0.1, initial=False)


@pytest.mark.parametrize("wn,on", GPU_PAIRS, ids=_ids(GPU_PAIRS))
def test_schedule_is_stable(oracle, synth, wn, on):
    w, opt, ref = _solved(oracle, synth, wn, on)
    _assert_stable(oracle, w, opt, ref)


@pytest.mark.parametrize("wn,edit", STRUCTURE, ids=_ids(STRUCTURE))
def test_structure_cases(oracle, synth, wn, edit):
    """The edit is what its name says, the oracle solves the edited window to a usable result, stably."""
    w0, w = B.window(synth, wn), B.structure_window(synth, wn, edit)
    n_obs, n_obs0 = np.diff(w["obs_ptr"]), np.diff(w0["obs_ptr"])
    changed = np.flatnonzero(n_obs != n_obs0)
    if edit == "single_observation":
        assert len(changed) == 1 and n_obs[changed[0]] == 1
    elif edit == "fixed_cameras_only":
        assert len(changed) == 1 and n_obs[changed[0]] == 2
        o = slice(w["obs_ptr"][changed[0]], w["obs_ptr"][changed[0] + 1])
        assert not np.any(w["cam_free"][w["obs_cam"][o]])
    elif edit == "far_behind":
        assert len(changed) == 0 and np.count_nonzero(np.any(w["points"] != w0["points"], axis=1)) == 1
    else:
        c = int(np.flatnonzero(w["cam_free"])[-1])
        assert not np.any(w["obs_cam"] == c) and np.any(w0["obs_cam"] == c) and n_obs.min() >= 1
    ref = B.solve_oracle(oracle, w, {})
    assert ref[2]["usable"] and ref[2]["iterations"] >= 2 and not [t for t in ref[3] if t["outcome"] == B.INVALID]
    _assert_stable(oracle, w, {}, ref)


def test_mixed_batch_ends_at_different_iterations(oracle, synth):
    for name in ("mixed_exits", "mixed_exits_not_pd"):
        case = B.BATCHES[name]
        out = [B.solve_oracle(oracle, B.batch_window(synth, oracle, spec), case["opt"]) for spec in case["windows"]]
        its = [s["iterations"] for _, _, s, _ in out]
        terms = [s["termination"] for _, _, s, _ in out]
        assert len(set(its)) >= 4 and 0 in its, its
        assert B.FAILURE in terms and any(s["usable"] for _, _, s, _ in out) and any(not s["usable"] for _, _, s, _ in out)
        # the window that starts at its optimum ends first among those that iterate at all
        assert its[-1] == min(i for i in its if i > 0)
    out_hard = B.solve_oracle(oracle, B.batch_window(synth, oracle, B.BATCHES["mixed_exits"]["windows"][5]), B.BATCHES["mixed_exits"]["opt"])
    assert "R" in B.outcomes(out_hard[3])


@pytest.mark.parametrize("bn,i", BATCH_WINDOWS, ids=_ids(BATCH_WINDOWS))
def test_batch_windows_are_stable(oracle, synth, bn, i):
    case = B.BATCHES[bn]
    w = B.batch_window(synth, oracle, case["windows"][i])
    _assert_stable(oracle, w, case["opt"], B.solve_oracle(oracle, w, case["opt"]))
