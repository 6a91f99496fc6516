"""The stream sweep can fail: tests/test_gpu_sweep_stream.py's seeds and counts on the CPU, no kernel involved.  (a) the draws are a pure
function of the seed; (b) at most 5 % of either family's draws are skipped for a non-finite reference (a condition: a sweep that skips its
draws proves nothing); (c) the float32 reference, handed to check_* as the result, is under every bar; (d) a float32 reference with one
wrong step, handed to check_* the same way, is over a bar in at least one draw of the seed set, for each of the eight ways of being wrong
below.  A mutant is installed with monkeypatch on the oracle primitive the references compose (O.update_ancilla_psi, O._rho_step,
O.expectation, the rho reference's _expect, O.inc_loss_psi, the plan's expand); the running sum is a local of the references' loop, so
that mutant is the reference's `out` with the sum carried over the forced steps (the sum feeds nothing but `out`).

What caught each mutant first on these seeds (the quantity furthest over its bar in that draw; printed by the test):
  mutant              psi_stream                rho_stream
  sigma2_x0           total  seed 41 draw 1     pred  seed 41 draw 6
  sigma2_x2           pred   seed 41 draw 1     pred  seed 41 draw 6
  late_expectation    pred   seed 41 draw 0     pred  seed 41 draw 0
  fixed_delta_t       pred   seed 41 draw 1     pred  seed 41 draw 6
  fixed_A             pred   seed 41 draw 0     pred  seed 41 draw 0
  sum_not_reset       out    seed 41 draw 0     out   seed 41 draw 2
  score_normalised    total  seed 41 draw 1     nll   seed 41 draw 2
  anchor_not_skipped  nll    seed 41 draw 0     pred  seed 41 draw 3
"""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import cmps_oracle as O
import _score_ref as SC
import _rho_score_ref as RS
import _sweep as SW
from test_gpu_sweep_stream import SEEDS, COUNTS              # (the GPU module imports no torch until a test of it runs)

FAMILY = {"psi_stream": (SW.draw_psi_stream, SW.reference_psi_stream, SW.check_psi_stream),
          "rho_stream": (SW.draw_rho_stream, SW.reference_rho_stream, SW.check_rho_stream)}
NOMINAL_DT = 1.0 / 16000


def draws(seed):
    """{family: cases} as run_sweep(seed, COUNTS, families=tuple(COUNTS)) draws them: one generator, psi_stream first."""
    rng = np.random.default_rng(seed)
    return {fam: [FAMILY[fam][0](rng, it) for it in range(COUNTS[fam])] for fam in COUNTS}


@functools.lru_cache(maxsize=None)
def cases(fam):
    """[(seed, case, ref32, ref64)] of the whole seed set, references computed once and left unchanged."""
    out = []
    for seed in SEEDS:
        for case in draws(seed)[fam]:
            out.append((seed, case, FAMILY[fam][1](case, "f32"), FAMILY[fam][1](case, "f64")))
    return out


def usable(fam):
    return [c for c in cases(fam) if SW.all_finite(c[2]) and SW.all_finite(c[3])]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    if dataclasses.is_dataclass(a):
        return _same(dataclasses.asdict(a), dataclasses.asdict(b))
    return a == b


def test_draws_are_a_pure_function_of_the_seed():
    """(a) and the ranges the issue sets: both D ranges, both variants, a shared clip, another delta_t, every kind of segment, anchors."""
    for seed in SEEDS[:2]:
        assert _same(draws(seed), draws(seed))
    assert not _same(draws(SEEDS[0])["psi_stream"][0], draws(SEEDS[1])["psi_stream"][0])
    for fam in COUNTS:
        cs = [c[1] for c in cases(fam)]
        assert len(cs) == len(SEEDS) * COUNTS[fam]
        assert {c["variant"] for c in cs} == {SW.AUTO, SW.BLOCK}
        assert any(c["hparams"].bond_dim > 32 for c in cs) and any(c["hparams"].bond_dim <= 32 for c in cs)
        assert any(c["n_audio"] == 1 < c["n"] for c in cs) and any(c["hparams"].delta_t != NOMINAL_DT for c in cs)
        assert {seg[0] for c in cs for seg in c["plan"]} == {SC.SCORE, SC.FOLLOW, SC.SAMPLE}
        assert any(seg[2] for c in cs for seg in c["plan"]) and all(not c["plan"][0][2] for c in cs)
        for c in cs:
            S, F, L, _ = SC.plan_counts(c["plan"])
            assert (c["clip"] is None) == (S + F == 0) and (c["noise"] is None) == (L == 0)
            assert c["clip"] is None or c["clip"].shape == (c["n_audio"], SC.clip_columns(c["plan"]))
            assert c["noise"] is None or c["noise"].shape == (L, c["n"])
    assert any(c[1]["options"]["rank1"] == SW.BF16X3 for c in cases("rho_stream"))


@pytest.mark.parametrize("fam", list(COUNTS))
def test_few_draws_are_skipped(fam):
    """(b) measured on these seeds: psi_stream 0 of 96, rho_stream 1 of 64 (seed 47 draw 6: a clip of amplitude 4.4 at A = 1.07 takes 1 + z
    below zero, so the reference's own log is not finite)."""
    total, kept = len(cases(fam)), len(usable(fam))
    print(f"{fam}: {total - kept} of {total} draws skipped for a non-finite reference")
    assert total - kept <= 0.05 * total


@pytest.mark.parametrize("fam", list(COUNTS))
def test_float32_reference_passes_every_bar(fam):
    """(c) and every draw yields checks of what its plan produces."""
    check = FAMILY[fam][2]
    for seed, case, r32, r64 in usable(fam):
        records = check(case, r32, r32, r64)
        bad = [r for r in records if not r[2] <= r[3]]
        assert not bad, (seed, bad)
        S, F, L, _ = SC.plan_counts(case["plan"])
        want = ({"finite"} | ({"nll", "total"} if S else set()) | ({"pred"} if S + F else set()) | ({"out"} if L else set())
                | ({"rho", "purity"} if fam == "rho_stream" else set()))
        assert {r[1] for r in records} == want, (seed, case["cfg"])


# ---------------------------------------------------------------------------------------------------
# (d) the mutants: each is install(monkeypatch, case) -> None, or a function of the finished float32 reference
# ---------------------------------------------------------------------------------------------------
def _with_sigma2(factor):
    def install(mp, case):
        psi, rho = O.update_ancilla_psi, O._rho_step
        scaled = lambda hp: dataclasses.replace(hp, sigma=hp.sigma * factor ** 0.5)      # noqa: E731
        mp.setattr(O, "update_ancilla_psi", lambda p, s, t, R, f, A, hp, dtype="f32": psi(p, s, t, R, f, A, scaled(hp), dtype))
        mp.setattr(O, "_rho_step", lambda r, x, t, R, f, A, hp, dtype: rho(r, x, t, R, f, A, scaled(hp), dtype))
    return install


def _expectation_only(mp, wrap):
    """Replace the expectation that becomes pred and the sampled increment, and leave the score's own (O.inc_loss_psi looks
    O.expectation up when it is called; _rho_step computes its own)."""
    psi, rho = O.expectation, RS._expect

    def inc_loss(p, signal, t, R, freqs, A, dtype="f32"):              # O.inc_loss_psi on the unmutated expectation
        real, _ = O._dt(dtype)
        z = (psi(p, t, R, freqs, dtype) * signal.astype(real)) / real(A)
        return (-np.log(real(1) + z)).astype(real)

    mp.setattr(O, "inc_loss_psi", inc_loss)
    mp.setattr(O, "expectation", lambda p, t, R, f, dtype="f32": wrap(psi, p, t, R, f, dtype))
    mp.setattr(RS, "_expect", lambda r, t, R, f, dtype: wrap(rho, r, t, R, f, dtype))


def late_expectation(mp, case):
    dt = np.float32(case["hparams"].delta_t)
    _expectation_only(mp, lambda fn, x, t, R, f, dtype: fn(x, np.float32(t + dt), R, f, dtype))


def fixed_delta_t(mp, case):
    k = np.float32(NOMINAL_DT / case["hparams"].delta_t)
    _expectation_only(mp, lambda fn, x, t, R, f, dtype: (fn(x, t, R, f, dtype) * k).astype(np.float32))


def fixed_A(mp, case):
    psi, rho = O.update_ancilla_psi, O._rho_step
    mp.setattr(O, "update_ancilla_psi", lambda p, s, t, R, f, A, hp, dtype="f32": psi(p, s, t, R, f, np.float32(10.0), hp, dtype))
    mp.setattr(O, "_rho_step", lambda r, x, t, R, f, A, hp, dtype: rho(r, x, t, R, f, np.float32(5.0), hp, dtype))


def score_normalised(mp, case):
    psi, rho = O.inc_loss_psi, O._rho_step
    mp.setattr(O, "inc_loss_psi", lambda p, s, t, R, f, A, dtype="f32": psi(O.normalize_psi(p, axis=1, dtype=dtype), s, t, R, f, A, dtype))

    def step(*args):
        st = rho(*args)
        return dict(st, z=(st["z"] / st["m"]).astype(st["z"].dtype))    # e is linear in rho: z on rho' / tr rho'
    mp.setattr(O, "_rho_step", step)


def anchor_not_skipped(mp, case):
    expand = SC.expand
    plain = lambda plan: [(kind, False) for kind, _ in expand(plan)]   # noqa: E731
    mp.setattr(SC, "expand", plain)
    mp.setattr(RS, "expand", plain)


def sum_not_reset(case, r32):
    """`out` with the running sum carried over the forced steps."""
    out, carry, j = r32["out"].copy(), np.zeros(case["n"], np.float32), 0
    for kind, steps, _ in case["plan"]:
        if kind == SC.SAMPLE:
            out[:, j:j + steps] += carry[:, None]
            j += steps
        elif j:
            carry = out[:, j - 1]
    return dict(r32, out=out)


MUTANTS = {"sigma2_x0": _with_sigma2(0.0), "sigma2_x2": _with_sigma2(2.0), "late_expectation": late_expectation, "fixed_delta_t": fixed_delta_t,
           "fixed_A": fixed_A, "sum_not_reset": sum_not_reset, "score_normalised": score_normalised, "anchor_not_skipped": anchor_not_skipped}


@pytest.mark.parametrize("fam", list(COUNTS))
@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(name, fam, monkeypatch):
    """(d) the first draw of the seed set whose mutated float32 reference is over a bar, and the quantity that is."""
    _, reference, check = FAMILY[fam]
    for seed, case, r32, r64 in usable(fam):
        if name == "sum_not_reset":
            mutated = sum_not_reset(case, r32)
        else:
            with monkeypatch.context() as mp:
                MUTANTS[name](mp, case)
                mutated = reference(case, "f32")
        over = [(what, err, bar) for _, what, err, bar, _ in check(case, mutated, r32, r64) if not err <= bar]
        if over:
            what, err, bar = max(over, key=lambda r: r[1] / r[2] if r[2] > 0 else np.inf)
            print(f"{name} / {fam}: caught by {what} ({err:.2e} over {bar:.2e}) at seed {seed}, draw {case['cfg'][0]}: {case['cfg']}")
            return
    pytest.fail(f"{name} passes every bar of {fam} on seeds {SEEDS}: the draws are too mild")
