"""The absolute-pose restatement tests/pnp_ref.py against the independent high-precision reference tests/pnp_hp.py, on
the cases of tests/pnp_cases.py.  No GPU.  It also holds the conditions on the inputs that tests/test_gpu_pnp_envelope.py
relies on: at most 3 points within 1e-9 of the bound per model, at most 2 % of the high-precision models set aside as
not isolated, no stop decision within 1e-9 of a multiple of 256, a clean set whose refit is computed and discarded, the
symmetric family's selected hypotheses, and the unchanged default scene.

The symmetric family (an isosceles triangle seen from eps g off its plane of symmetry; 20 scenes per eps, the
hypotheses that sample the triangle as (0, 1, 2) or (2, 1, 0); `found` = a model within 1e-5 of the high-precision model
nearest the true pose):

    eps      selected   isolated (gap >= 1e-3)   found, u = N / D only   found, with the cosine-law fallback
    0        95         0                        0                       68
    1e-8     95         0                        0                       75
    1e-4     95         0                        26                      95
    1e-2     95         30                       95                      95
    1e-1     95         68                       95                      95

Below eps = 1e-4 the pose is a genuine double root of f32 data: the root is located to about 1e-8 and the model to about
1e-4, which is the recorded limit."""
import hashlib

import numpy as np
import pytest

import pnp_cases as PC
import pnp_hp as HP
import pnp_ref as P

DEFAULT_SCENE_SHA256 = "846e0edbf4b7fd7275865b18048f3bedae012b2846cc8269f28a2ee50c2144d3"


def test_default_scene_is_unchanged():
    """The knobs added to synth.make_pnp_scene leave its default output byte for byte (recorded before they existed)."""
    d = PC.synth().make_pnp_scene()
    h = hashlib.sha256(b"".join(np.ascontiguousarray(d[k]).tobytes() for k in ("points", "pixels", "K", "pose", "inlier")))
    assert h.hexdigest() == DEFAULT_SCENE_SHA256


def test_hp_reference_on_a_constructed_triple():
    """pnp_hp by itself: exact projections of a known pose; the true pose is among its models to 1e-12, every model puts
    the three points back onto their bearings, and swapping two points swaps nothing in the set of poses."""
    rng = np.random.default_rng(2)
    R = PC.synth().rodrigues(rng.normal(0, 0.5, 3))
    t = np.array([0.3, -0.2, 1.0])
    Xc = np.array([[-1.0, 0.4, 5.0], [0.7, 0.9, 7.0], [0.2, -1.1, 4.0]])
    W = (Xc - t) @ R
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    hp = HP.p3p_hp(W, x, y)
    truth = np.concatenate([R, t[:, None]], 1).ravel()
    assert 1 <= len(hp) <= 4 and min(HP.model_dist(m, truth) for m, _, _ in hp) < 1e-12
    for m, gap, v in hp:
        M = m.reshape(3, 4)
        Y = W @ M[:, :3].T + M[:, 3]
        assert np.abs(Y[:, 0] / Y[:, 2] - x).max() < 1e-12 and np.abs(Y[:, 1] / Y[:, 2] - y).max() < 1e-12 and (Y[:, 2] > 0).all()
        assert max(np.abs(HP.rotation_checks(m))) < 1e-14 and gap > 0
    sw = HP.p3p_hp(W[[2, 1, 0]], x[[2, 1, 0]], y[[2, 1, 0]])
    assert len(sw) == len(hp) and all(min(HP.model_dist(m, q) for q, _, _ in sw) < 1e-12 for m, _, _ in hp)


def _decisions(name, r):
    """(drawn, needed) at every stop decision of a restatement run."""
    _, _, _, count, kw = PC.call_args(name)
    n = min(max(count, 0), len(PC.scene(name)["points"]))
    out = []
    for drawn in list(range(P.ROUND, r["drawn"], P.ROUND)) + [r["drawn"]]:
        best = int(r["scores"][:drawn].max()) if drawn else 0
        out.append((drawn, P.needed_hypotheses(best, n, kw["confidence"])))
    return out


@pytest.mark.parametrize("name", PC.PLAIN)
def test_case_against_the_high_precision_reference(name):
    case, d, r = PC.CASES[name], PC.scene(name), PC.ref(name)
    pts, pix, K, count, kw = PC.call_args(name)
    ex = case["expect"]
    if ex["status"] is not None:
        assert r["status"] == ex["status"]
    if "refit_kept" in ex:
        assert r["refit_kept"] == ex["refit_kept"]
    if "drawn" in ex:
        assert r["drawn"] == ex["drawn"]
    if ex.get("nmodels_zero"):
        assert (r["nmodels"] == 0).all() and r["drawn"] == kw["max_hypotheses"]
    if r["status"] == P.STATUS_FEW_POINTS:
        assert r["drawn"] == 0 and len(r["samples"]) == 0
        return
    # the stop: where the case says, and never decided by the last digits of a logarithm
    if case["stop"] is None:
        assert r["drawn"] == kw["max_hypotheses"]
    elif case["stop"] == ">=3":
        assert r["drawn"] >= 3 * P.ROUND
    else:
        assert r["drawn"] == min(P.ROUND * case["stop"], kw["max_hypotheses"])
    for drawn, needed in _decisions(name, r):
        if np.isfinite(needed) and needed > 0:
            k = max(round(needed / P.ROUND), 1)
            assert abs(needed - P.ROUND * k) > 1e-9 * needed and abs(needed - drawn) > 1e-9 * needed, (drawn, needed)
    if ex.get("nmodels_zero"):
        return
    total, excluded = PC.check_table(name, r, r["drawn"])
    print(name, "high-precision models", total, "not isolated", excluded)
    if total >= 100:
        assert excluded <= 0.02 * total, (excluded, total)
    # beyond the first 256 hypotheses: the near-threshold slack that the GPU comparison grants stays <= 3
    for h in range(PC.HP_LIMIT, r["drawn"]):
        for m in range(r["nmodels"][h]):
            assert HP.reproj_count(r["models"][h, m], pts[:len(r["mask"])], pix[:len(r["mask"])], K, kw["threshold_px"])[1] <= 3
    PC.check_final(name, r["Rt"], r["mask"], r["refit_kept"], r["status"])
    if case["kind"] == "sparse" and r["status"] != P.STATUS_FEW_POINTS:
        assert (r["nmodels"] == 0).mean() > 0.5                       # most draws fail


def test_a_clean_set_discards_its_computed_refit():
    """At least one of the clean sets has >= 6 inliers under its minimal model, a refit that EPnP does compute, and a
    refit that is then discarded (it keeps fewer inliers): the path of pnp_final that overwrites nothing."""
    hit = []
    for n in PC.CLEAN:
        name = f"clean{n}"
        d, r = PC.scene(name), PC.ref(name)
        assert r["status"] == 0
        if r["refit_kept"] or r["best_count"] < P.MIN_REFIT:
            continue
        prep = P.prepare(d["points"], d["pixels"], d["K"])
        zc, e2 = P.reproj2(r["minimal"], *prep[:5], float(d["K"][0]), float(d["K"][1]))
        mask = prep[5] & (zc > 0) & (e2 < r["thr2"])
        fit, _ = P.epnp(*prep[:5], mask, float(d["K"][0]), float(d["K"][1]))
        if fit is not None:
            hit.append(name)
    print("discarded refits:", hit)
    assert hit


@pytest.mark.parametrize("eps", PC.SYM_EPS)
def test_symmetric_family(eps):
    """Every scene has a selected hypothesis; every emitted model passes the table checks; at eps = 1e-2 and 1e-1 every
    selected hypothesis whose true-pose root is isolated holds a model within 1e-5 of the high-precision model nearest
    the true pose.  At eps = 1e-4 the same is asked of the roots isolated by 1e-5 (1 + |v|): a root with that gap is
    located to about 1e-16 / 1e-5 = 1e-11, and u from the cosine law loses no more, so 1e-5 holds with a wide margin;
    u = N / D alone lost 69 of the 95 there.  Below that only the recovered share is printed (see the table above)."""
    selected = isolated = found = 0
    for k in range(PC.SYM_SCENES):
        name = PC.sym_name(eps, k)
        r = PC.ref(name)
        assert r["drawn"] == PC.SYM_HYP
        sel = PC.sym_selected(r["samples"], r["drawn"])
        assert sel, name
        PC.check_table(name, r, r["drawn"], completeness=eps >= 1e-2)
        for h in sel:
            m, gap, dist = PC.sym_true_model(name, r["samples"][h])
            assert dist < 1e-4, (name, h, dist)                   # the high-precision set does hold the true pose
            ok = any(np.abs(r["models"][h, q] - m).max() <= 1e-5 for q in range(r["nmodels"][h]))
            selected, found = selected + 1, found + ok
            if eps >= 1e-2 and gap >= HP.ISOLATED:
                isolated += 1
                assert ok, (name, h, gap)
            if eps == 1e-4 and gap >= 1e-5:
                assert ok, (name, h, gap)
    print("eps %g: selected %d, isolated %d, true pose found %d" % (eps, selected, isolated, found))




def test_symmetric_family_isolation_share():
    """At least half of the selected hypotheses at eps = 1e-2 and 1e-1 pass the isolation gate, so the acceptance above
    is asked of a real share of them."""
    sel = iso = 0
    for eps in (1e-2, 1e-1):
        for k in range(PC.SYM_SCENES):
            name = PC.sym_name(eps, k)
            r = PC.ref(name)
            for h in PC.sym_selected(r["samples"], r["drawn"]):
                sel += 1
                iso += PC.sym_true_model(name, r["samples"][h])[1] >= HP.ISOLATED
    assert 2 * iso >= sel, (iso, sel)
