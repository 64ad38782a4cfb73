"""rs_bundle_adjust and rs_bundle_adjust_batch on the GPU against the oracle: every vision-only kernel path of the host
driver (the vision-only entries of test_gpu_ba_paths.CASES) under every option case of tests/ba_cases.py, which
tests/test_ba_cases_cpu.py pins on the CPU (the oracle against dense_lm, every case reaching its exit, every compared pair
stable under 1e-13 on its input).  The Levenberg-Marquardt policy behind rs_ba_options (damping clamp, Jacobi scale,
gradient exit, failed factorisation) is written out once per path in csrc: a case that fails on some paths and passes on
the others names the copy that is wrong.  Per solve:
  the path   the profile's scope names are those test_gpu_ba_paths.EXPECT records for the path
  the solve  the oracle's, by the contract of tests/ba_compare.py (schedule and outcomes exact, values to its tolerances)
  the inputs untouched when the solve is unusable; fixed cameras always
Also: 1, 2, 3 and 5 speculative radii on the local-window paths through the exits and failures that can fall inside a
speculated set; windows with degenerate structure; batches whose windows end at different iterations, fail, or make the
grid decline, in both batch modes; and what the library refuses."""
import ctypes as C

import numpy as np
import pytest

import ba_cases as B
import ba_compare as CMP
import test_gpu_ba_paths as P
from conftest import to_np

pytestmark = pytest.mark.gpu

RS_OK, RS_ERR_INVALID = 0, 1
MAX_SETS = 5                                # the largest "ba_speculative_sets" the library takes
ROUND_KERNEL_SETS = 3                       # "ba_fuse_mode" 3 holds at most three sets in its one launch; beyond: the default launches
LOCAL = [p for p in B.SINGLE_PATHS if B.PATHS[p][1] == "plain"]           # the paths of the local window (p.local_window())

OPTION_CASES = [(p, o) for p in B.SINGLE_PATHS for o in B.OPTIONS if B.applies(B.PATHS[p][1], o)]
HARD_CASES = [(p, o) for p in B.SINGLE_PATHS for o in B.HARD_OPTIONS if B.applies(B.PATHS[p][1] + "_hard", o)]
SETS_CASES = [(p, o, ns) for p in LOCAL for o in B.SETS for ns in (1, 2, 3, MAX_SETS)]
BATCH_OPTION_CASES = [(p, o) for p in B.BATCH_PATHS for o in B.OPTIONS if B.applies(B.PATHS[p][1], o)]
STRUCTURE_CASES = [(p, e) for p in ("plain", "blocked_banded") for e in B.STRUCTURE]

_ORACLE = {}


def _ids(cases):
    return ["-".join(map(str, c)) for c in cases]


def _problem(synth, oracle, wn, on):
    """window, options, oracle result (cams, points, summary, trace) of a pair: solved once per session, shared by the paths."""
    if (wn, on) not in _ORACLE:
        w, opt = B.window(synth, wn, on), B.opt_of(wn, on)
        _ORACLE[wn, on] = (w, opt, B.solve_oracle(oracle, w, opt))
    return _ORACLE[wn, on]


def _device(c, w):
    dc, dp = c.dev(w["cams"]), c.dev(w["points"])
    return dc, dp, (dc, w["cam_free"], dp, c.dev(w["obs_ptr"]), c.dev(w["obs_cam"]), c.dev(w["obs_uv"]), w["K"])


def _raw(c, rs, w, dc, dp, rest, options=None, n_cameras=None, n_points=None, n_obs=None, null_points=False):
    """rs_bundle_adjust through the raw library: (status, summary)."""
    cam_free = np.ascontiguousarray(w["cam_free"], np.uint8)
    Kc = (C.c_float * 4)(*[float(v) for v in w["K"]])
    s = rs.BaSummary()
    rc = c.lib.rs_bundle_adjust(
        c.h, len(w["cams"]) if n_cameras is None else n_cameras, len(w["points"]) if n_points is None else n_points,
        len(w["obs_cam"]) if n_obs is None else n_obs, C.c_void_p(dc.data_ptr()), cam_free.ctypes.data_as(C.c_void_p),
        None if null_points else C.c_void_p(dp.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in rest], Kc,
        None if options is None else C.byref(options), C.byref(s))
    return rc, s.as_dict()


def _gpu(c, rs, w, opt, knobs):
    """One profiled solve under `knobs` (reset afterwards): status, summary, trace, state, profile, stats."""
    try:
        for k, v in knobs.items():
            c.set_int(k, v)
        dc, dp, args = _device(c, w)
        c.prof_begin()
        try:
            rc, s = _raw(c, rs, w, dc, dp, args[3:6], B.options(rs, opt))
        finally:
            prof = c.prof_end()
        c.synchronize()
        return dict(rc=rc, s=s, tr=c.ba_trace() if rc == RS_OK else [], c=to_np(dc), p=to_np(dp), prof=prof, stats=c.ba_stats())
    finally:
        for k in P.KNOBS:
            c.set_int(k, 0)


def _context(ctx, rs, kind):
    """The context a path runs on: "comm" takes a communicator of one rank on a context of its own."""
    if kind != "comm":
        return ctx
    c = rs.Context(0)
    rs.Context.comm_init_local([c])
    return c


def _release(ctx, c):
    if c is not ctx:
        c.comm_destroy()
        c.close()


def _expected_scopes(path, sets=0):
    """The scope names test_gpu_ba_paths.EXPECT records for the path.  The first round is always enqueued (a solve of
    max_num_iterations 0 needs its front end for the cost and the gradient at the input), so even a solve that ends
    before its first iteration shows the path it took."""
    if B.PATHS[path][2].get("ba_fuse_mode") == 3 and sets > ROUND_KERNEL_SETS:
        path = "plain"
    return set(P.EXPECT[path][0])


def _assert_untouched_where_due(g, w):
    fixed = np.asarray(w["cam_free"]) == 0
    assert g["c"][fixed].tobytes() == w["cams"][fixed].tobytes()
    if not g["s"]["usable"]:
        assert g["c"].tobytes() == w["cams"].tobytes() and g["p"].tobytes() == w["points"].tobytes()


def _run(ctx, rs, path, w, opt, ref, sets=None):
    kind, _, knobs = B.PATHS[path]
    if sets is not None:
        knobs = dict(knobs, ba_speculative_sets=sets)
    c = _context(ctx, rs, kind)
    try:
        g = _gpu(c, rs, w, opt, knobs)
    finally:
        _release(ctx, c)
    rc_, rp, s, tr = ref
    print(path, opt, B.outcomes(tr), {k: s[k] for k in CMP.SCHEDULE}, "gpu", B.outcomes(g["tr"]), {k: g["s"][k] for k in CMP.SCHEDULE},
          s["final_cost"], g["s"]["final_cost"], sorted(g["prof"]), g["stats"])
    assert g["rc"] == RS_OK
    # (a solve never speculates on more radii than it may run iterations)
    assert set(g["prof"]) == _expected_scopes(path, min(knobs.get("ba_speculative_sets", 0), opt.get("max_num_iterations", 10))), sorted(g["prof"])
    CMP.assert_same_solve(g, (rc_, rp, None, None, s, tr))
    _assert_untouched_where_due(g, w)
    return g


@pytest.mark.parametrize("path,on", OPTION_CASES, ids=_ids(OPTION_CASES))
def test_path_under_option(ctx, rs, oracle, synth, path, on):
    w, opt, ref = _problem(synth, oracle, B.PATHS[path][1], on)
    _run(ctx, rs, path, w, opt, ref)


@pytest.mark.parametrize("path,on", HARD_CASES, ids=_ids(HARD_CASES))
def test_path_on_the_hard_window(ctx, rs, oracle, synth, path, on):
    """The twin with 10 % outliers and 2 degrees of rotation noise: rejected steps on every path."""
    w, opt, ref = _problem(synth, oracle, B.PATHS[path][1] + "_hard", on)
    _run(ctx, rs, path, w, opt, ref)


@pytest.mark.parametrize("path,on,ns", SETS_CASES, ids=_ids(SETS_CASES))
def test_speculative_sets(ctx, rs, oracle, synth, path, on, ns):
    """1 .. 5 trust-region radii per round on the local-window paths: the per-iteration record is the oracle's whatever the
    number, through exits and failures that fall inside a speculated set.  The accounting: a round that did work evaluates
    between one set and min(sets, iterations left) and commits at least one iteration; the first round evaluates one set,
    the second min(sets, iterations left) of them (s.nact, ba_common.h) if the solve gets that far."""
    w, opt, ref = _problem(synth, oracle, "plain_hard", on)
    g = _run(ctx, rs, path, w, opt, ref, sets=ns)
    st, its = g["stats"], g["s"]["iterations"]
    max_iter = opt.get("max_num_iterations", 10)
    assert st["rounds"] <= its <= st["set_evaluations"] <= min(ns, max_iter) * st["rounds"]
    if min(ns, max_iter - 1) <= 1 or its < 2:
        assert st["rounds"] == st["set_evaluations"] == its, st
    else:
        assert st["set_evaluations"] > st["rounds"], st


@pytest.mark.parametrize("path,edit", STRUCTURE_CASES, ids=_ids(STRUCTURE_CASES))
def test_degenerate_structure(ctx, rs, oracle, synth, path, edit):
    """A landmark with one observation, one seen by fixed cameras only, one far behind its cameras, a free camera without
    observations.  rs_bundle_adjust takes the FREE points (two observations or more, seen by a free frame): for the first
    two the library may refuse with RS_ERR_INVALID and leave everything untouched, or solve like the oracle; nothing else."""
    wn = B.PATHS[path][1]
    key = (wn, "structure:" + edit)
    if key not in _ORACLE:
        w = B.structure_window(synth, wn, edit)
        _ORACLE[key] = (w, {}, B.solve_oracle(oracle, w, {}))
    w, opt, ref = _ORACLE[key]
    g = _gpu(ctx, rs, w, opt, B.PATHS[path][2])
    print(path, edit, g["rc"], g["s"], ref[2], sorted(g["prof"]))
    if g["rc"] != RS_OK:
        assert edit in B.MAY_REFUSE and g["rc"] == RS_ERR_INVALID
        assert g["c"].tobytes() == w["cams"].tobytes() and g["p"].tobytes() == w["points"].tobytes()
        return
    assert set(g["prof"]) == _expected_scopes(path)
    CMP.assert_same_solve(g, (ref[0], ref[1], None, None, ref[2], ref[3]))
    _assert_untouched_where_due(g, w)


# ------------------------------------------------------------------------------------------------------------------ batch
def _batch(ctx, rs, windows, opt, mode):
    """One profiled rs_bundle_adjust_batch in ba_batch_mode `mode`: summaries, states, profile."""
    dev = [_device(ctx, w) for w in windows]
    ctx.set_int("ba_batch_mode", mode)
    try:
        ctx.prof_begin()
        try:
            out = ctx.bundle_adjust_batch([d[2] for d in dev], options=B.options(rs, opt))
        finally:
            prof = ctx.prof_end()
    finally:
        ctx.set_int("ba_batch_mode", 0)
    ctx.synchronize()
    return out, [(to_np(dc), to_np(dp)) for dc, dp, _ in dev], prof


def _grid_ran(prof):
    """The grid form runs its launches on the calling context, once for all windows; the lanes are contexts of their own
    whose launches this profile does not see."""
    if "K7_ba_reduced_solve" in prof:
        assert int(prof["K0_ba_init"][0]) == 1
        return True
    assert not prof, sorted(prof)
    return False


def _assert_batch(out, states, windows, refs):
    """Every window against the oracle's solve of it: a batch has no trace, so summary, cameras and points."""
    for i, (s, (gc, gp), w, ref) in enumerate(zip(out, states, windows, refs)):
        g = dict(s=s, c=gc, p=gp)
        if ref is None:                 # no landmark: nothing to optimise
            assert (s["termination"], s["usable"], s["iterations"]) == (B.FAILURE, 0, 0), i
        else:
            CMP.assert_same_summary(s, gc, gp, (ref[0], ref[1], ref[2]))
        _assert_untouched_where_due(g, w)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(B.BATCHES))
def test_batch(ctx, rs, oracle, synth, name, mode):
    """Windows of one batch that end at different iterations (ba_follow_rounds follows the slowest), fail at iteration 0 or
    after steps, start at their optimum; batches the grid declines (a window too large for it, no iteration, a window
    without landmarks) and the lanes run.  A failed window comes back untouched and the windows around it are the oracle's."""
    case = B.BATCHES[name]
    key = ("batch", name)
    if key not in _ORACLE:
        ws = [B.batch_window(synth, oracle, spec) for spec in case["windows"]]
        _ORACLE[key] = (ws, [None if len(w["points"]) == 0 else B.solve_oracle(oracle, w, case["opt"]) for w in ws])
    ws, refs = _ORACLE[key]
    out, states, prof = _batch(ctx, rs, ws, case["opt"], mode)
    print(name, mode, [tuple(s[k] for k in CMP.SCHEDULE) for s in out], [r and tuple(r[2][k] for k in CMP.SCHEDULE) for r in refs], sorted(prof))
    assert _grid_ran(prof) == (case["grid"] and mode == 0)
    _assert_batch(out, states, ws, refs)


@pytest.mark.parametrize("path,on", BATCH_OPTION_CASES, ids=_ids(BATCH_OPTION_CASES))
def test_batch_path_under_option(ctx, rs, oracle, synth, path, on):
    """The batched entry points of the local-window kernels (grid) and the lanes under every option case: the window of the
    case twice, as two problems with buffers of their own."""
    _, wn, knobs = B.PATHS[path]
    w, opt, ref = _problem(synth, oracle, wn, on)
    mode = knobs.get("ba_batch_mode", 0)
    out, states, prof = _batch(ctx, rs, [w, w], opt, mode)
    print(path, on, [tuple(s[k] for k in CMP.SCHEDULE) for s in out], tuple(ref[2][k] for k in CMP.SCHEDULE), sorted(prof))
    assert _grid_ran(prof) == (mode == 0 and opt.get("max_num_iterations", 10) > 0)
    if prof:
        assert set(prof) == set(P.EXPECT[path][0])
    _assert_batch(out, states, [w, w], [ref, ref])


# --------------------------------------------------------------------------------------------------------------- refusals
REFUSALS = {
    "max_iter_-1": (dict(max_num_iterations=-1), {}, RS_ERR_INVALID),
    "max_iter_1001": (dict(max_num_iterations=1001), {}, RS_ERR_INVALID),
    "negative_cameras": ({}, dict(n_cameras=-1), RS_ERR_INVALID),
    "negative_points": ({}, dict(n_points=-1), RS_ERR_INVALID),
    "negative_observations": ({}, dict(n_obs=-1), RS_ERR_INVALID),
    "null_points": ({}, dict(null_points=True), RS_ERR_INVALID),
    "no_camera": ({}, dict(n_cameras=0), RS_OK),
    "no_point": ({}, dict(n_points=0), RS_OK),
    "no_observation": ({}, dict(n_obs=0), RS_OK),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_everything_untouched(ctx, rs, oracle, synth, name):
    """What rs_bundle_adjust refuses (RS_ERR_INVALID) and what it has nothing to optimise in (RS_OK, FAILURE, unusable):
    the device arrays come back bit for bit, and the same context solves the window normally afterwards."""
    fields, sizes, status = REFUSALS[name]
    w, opt, ref = _problem(synth, oracle, "plain", "default")
    dc, dp, args = _device(ctx, w)
    rc, s = _raw(ctx, rs, w, dc, dp, args[3:6], B.options(rs, fields), **sizes)
    ctx.synchronize()
    print(name, rc, s)
    assert rc == status
    if status == RS_OK:
        assert (s["termination"], s["usable"], s["iterations"]) == (B.FAILURE, 0, 0)
    assert to_np(dc).tobytes() == w["cams"].tobytes() and to_np(dp).tobytes() == w["points"].tobytes()
    _run(ctx, rs, "plain", w, opt, ref)
