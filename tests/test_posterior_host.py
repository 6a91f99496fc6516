"""The restatement of cmps_bank_posterior (tests/_posterior_ref.py) without a GPU: against a plain np.longdouble soft-max of the running
totals, the sums of its rows, a cut, absent members, all-absent steps, exact ties, a -inf prior and the decision rule -- and, for every
draw tests/test_gpu_posterior.py feeds the kernel, the two conditions under which the device's `best` and decision records can be
compared exactly (no reference step within 1e-9 of a threshold; no runner-up within 1e-9 max(1, |a|) of the best unless it ties it
exactly).  NO step of any draw is excused: the seeds of `_posterior_ref.cases` are chosen so."""
import numpy as np
import pytest

import _posterior_ref as PR

CASES = PR.cases()


def _long_softmax(c, lp, kappa):
    """p [M] in extended precision from float32 totals c [M] (non-finite: absent); None when nobody can win."""
    L = np.longdouble
    ok = np.isfinite(c) & (lp > -np.inf)
    if not ok.any():
        return None
    a = L(kappa) * c[ok].astype(L) - lp[ok].astype(L)
    e = np.exp(-(a - a.min()))
    p = np.zeros(c.shape[0], L)
    p[ok] = e / e.sum()
    return p


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_the_restatement_against_extended_precision(name, kw):
    ref = PR.posterior(**kw)
    M, n, steps = kw["nll"].shape
    lp = np.zeros(M) if kw["log_prior"] is None else kw["log_prior"]
    # an independent fold: the two float32 terms added in float64 -- exact at these magnitudes -- and rounded to float32 once
    tot = np.zeros((M, n), np.float32) if kw["total_in"] is None else kw["total_in"].copy()
    worst = 0.0
    for k in range(steps if M <= 130 else 8):
        with np.errstate(invalid="ignore", over="ignore"):
            tot = np.float32(tot.astype(np.float64) + kw["nll"][:, :, k].astype(np.float64))     # (a float32 sum rounded once: the same)
        assert np.array_equal(tot, ref["c"][:, :, k], equal_nan=True)
        for g in range(n):
            p = _long_softmax(tot[:, g], lp, kw["inv_temp"])
            if p is None:
                assert ref["best"][g, k] == -1 and ref["conf"][g, k] == 0 and not ref["post"][:, g, k].any()
                assert not np.signbit(ref["post"][:, g, k]).any() and not np.signbit(ref["conf"][g, k])
                continue
            bar = PR.bound(p.astype(np.float64), M, ref["scale"][g, k])
            err = np.abs(ref["post"][:, g, k].astype(np.longdouble) - p).astype(np.float64)
            assert np.all(err <= bar), (name, g, k, err.max(), bar.min())
            assert abs(float(ref["conf"][g, k] - p.max())) <= PR.bound(float(p.max()), M, ref["scale"][g, k])
            assert abs(float(ref["post64"][:, g, k].sum()) - 1.0) <= float(bar.sum())            # a row sums to 1 within the bound
            assert p[ref["best"][g, k]] == p.max()
            worst = max(worst, float((err / bar).max()))
    print(f"{name}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_every_gpu_draw_is_well_posed_and_moves(name, kw):
    ref = PR.posterior(**kw)
    near, close = PR.ill_posed(ref, PR.THRESHOLDS)
    assert len(near) == 0, (name, "steps within 1e-9 of a threshold", near[:5])
    assert len(close) == 0, (name, "runner-up within 1e-9 of the best", close[:5])


def test_the_draws_cross_both_thresholds_somewhere():
    moved = {t: 0 for t in PR.THRESHOLDS}
    for name, kw in CASES:
        if kw["nll"].shape[0] < 2:
            continue
        conf = PR.posterior(**kw)["conf64"]
        for t in PR.THRESHOLDS:
            up = (conf[:, 1:] >= t) & (conf[:, :-1] < t) & (conf[:, :-1] > 0)
            moved[t] += int(up.sum())
    assert all(v >= 5 for v in moved.values()), moved


@pytest.mark.parametrize("name,kw", [c for c in CASES if c[1]["nll"].shape[2] >= 5], ids=[c[0] for c in CASES if c[1]["nll"].shape[2] >= 5])
def test_a_cut_changes_nothing(name, kw):
    whole = PR.posterior(**kw)
    steps = kw["nll"].shape[2]
    edges = [0] + PR.cuts(steps) + [steps]
    total, rec, parts = kw["total_in"], None, []
    for a, b in zip(edges[:-1], edges[1:]):
        part = PR.posterior(kw["nll"][:, :, a:b], total_in=total, log_prior=kw["log_prior"], inv_temp=kw["inv_temp"],
                            threshold=kw["threshold"], first_step=kw["first_step"] + a, decision=rec, reset=rec is None)
        total, rec = part["total_out"], part["decision"]
        parts.append(part)
    for key in ("post", "best", "conf", "c"):
        got = np.concatenate([p[key] for p in parts], axis=-1)
        assert np.array_equal(got.view(np.uint8), whole[key].view(np.uint8)), key
    assert np.array_equal(total.view(np.uint32), whole["total_out"].view(np.uint32))
    assert np.array_equal(rec, whole["decision"])


def test_absent_members_and_all_absent_steps():
    kw = dict(CASES)["planted"]
    ref = PR.posterior(**kw)
    base = dict(kw, nll=np.nan_to_num(kw["nll"], nan=0.0, posinf=0.0, neginf=0.0))
    clean = PR.posterior(**base)
    gone = {(1, 0): 7, (3, 1): 64, (4, 2): 129, (0, 2): 3}
    M, n, steps = kw["nll"].shape
    for m in range(M):
        for g in range(n):
            k = gone.get((m, g), steps)
            assert np.all(np.isfinite(ref["c"][m, g, :k])) and not np.isfinite(ref["c"][m, g, k:]).any()
            assert not ref["post"][m, g, k:].any() and np.all(ref["best"][g, k:] != m)
    assert np.isnan(ref["c"][0, 2, 70]) and np.isposinf(ref["c"][0, 2, 69])                  # +Inf then -Inf in one row: NaN
    assert np.array_equal(ref["post"][:, 0, :7], clean["post"][:, 0, :7]) and np.array_equal(ref["best"][1, :64], clean["best"][1, :64])
    kw = dict(CASES)["all-absent"]
    ref = PR.posterior(**kw)
    assert np.all(ref["best"][0] == -1) and not ref["conf"][0].any() and not ref["post"][:, 0].any()
    assert np.all(ref["best"][1, :2] >= 0) and np.all(ref["best"][1, 2:] == -1) and not ref["conf"][1, 2:].any()
    assert ref["decision"]["step"][0] == -1 and ref["decision"]["member"][0] == -1
    assert not np.signbit(ref["conf"]).any() and not np.signbit(ref["post"]).any()


def test_exact_ties_go_to_the_lower_member():
    for name, lo in (("tie-3", 1), ("tie-65", 7), ("tie-130", 7)):
        ref = PR.posterior(**dict(CASES)[name])
        assert np.all(ref["best"] == lo) and np.all(ref["conf"] <= 0.5) and np.all(ref["decision"]["step"] == -1), name


def test_a_member_with_log_prior_minus_infinity_never_wins():
    for name, kw in CASES:
        if not name.endswith("-never"):
            continue
        M = kw["nll"].shape[0]
        ref = PR.posterior(**kw)
        assert not ref["post"][M // 2].any() and np.all(ref["best"] != M // 2), name
        if M == 1:                                                     # nobody else: a step with no member present
            assert np.all(ref["best"] == -1) and not ref["conf"].any() and ref["decision"]["step"][0] == -1
        else:
            others = PR.posterior(**dict(kw, nll=np.delete(kw["nll"], M // 2, 0), total_in=np.delete(kw["total_in"], M // 2, 0),
                                         log_prior=np.delete(kw["log_prior"], M // 2)))
            assert np.array_equal(np.delete(ref["post"], M // 2, 0), others["post"]) and np.array_equal(ref["conf"], others["conf"])


def test_the_decision_is_the_first_crossing_and_survives_later_dips():
    nll = np.zeros((2, 3, 6), np.float32)
    nll[1, 0] = [1, 2, -9, -9, 2, 2]         # path 0: member 0 is sure at step 1, member 1 takes over at step 3
    nll[1, 1] = [0, 1, 1, -2, -1, 0]         # path 1: sure at step 2 only (a dip behind it)
    ref = PR.posterior(nll, threshold=0.8, first_step=100)
    assert ref["decision"]["step"].tolist() == [101, 102, -1] and ref["decision"]["member"].tolist() == [0, 0, -1]
    assert ref["conf64"][0, 1] >= 0.8 and ref["best"][0, 5] == 1 and ref["conf64"][1, 3] < 0.8 and np.all(ref["conf64"][2] == 0.5)
    again = PR.posterior(nll[:, :, ::-1].copy(), threshold=0.8, first_step=106, decision=ref["decision"], reset=False)
    assert again["decision"]["step"].tolist()[:2] == [101, 102] and again["decision"]["reserved"].tolist() == [0, 0, 0]
    fresh = PR.posterior(nll, threshold=0.8, first_step=0, decision=ref["decision"], reset=True)
    assert fresh["decision"]["step"].tolist() == [1, 2, -1]
    assert PR.posterior(nll, threshold=1.0)["decision"]["step"].tolist() == [-1, -1, -1]
    one = PR.posterior(nll[:1], threshold=1.0, first_step=7)            # one member: sure at once, 1 / S = 1 >= 1
    assert one["decision"]["step"].tolist() == [7, 7, 7] and np.all(one["conf"] == 1)
