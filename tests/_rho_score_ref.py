"""What a scored RhoCMPS stream must give for a *plan*: tests/_rho_stream_ref.py::rho_stream_reference with a third kind of step, composed
from the same oracle primitives (O._rho_step, _expect, O.rho_0, O.time_table).  A plan is tests/_score_ref.py's: a list of segments
(kind, steps) or (kind, steps, anchored), kind in ("score", "follow", "sample"):

  follow  _rho_update (model.py:144-150) on the clip's increment (:138): records Re tr((Rt + Rt^dagger) rho) * delta_t before the step,
          resets the running sum;
  score   the same step, and of the O._rho_step it makes anyway the fold's increment (_rho_and_loss_update, model.py:152-158;
          _inc_loss_rho, :169-170): lv = -log(1 + st["z"]), z = e' x / A on the updated, un-normalised rho'; total += lv in step order --
          per step to `nll`, summed to `total`;
  sample  _rho_and_sample_update (:160-167).

One time grid runs through all segments, the forced steps read ONE clip through the column cursor of tests/_score_ref.py (an anchored
segment first skips one column).  The function is a plain loop over the steps of the expanded plan, so it cannot depend on the
segmentation; tests/test_rho_score_host.py asserts that once."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O
from _score_ref import SCORE, FOLLOW, SAMPLE, plan_counts, clip_columns, expand, refine      # noqa: F401  (the plan helpers are the pure-state ones)
from _rho_primed_ref import _expect, case_model, oracle_side, R_fro      # noqa: F401


def rho_score_reference(hp: O.HParams, var: O.Variables, Wx, Wy, plan, clip, noise=None, dtype="f32", start=None, n=None):
    """clip [n_audio, clip_columns(plan)] (n_audio = n, or 1: shared; None without forced steps), noise [sampled, n] or None ->
    (nll [n, scored], total [n], pred [n, scored + followed], out [n, sampled], rhos [n, steps, D, D] after every step, purity [n, steps],
    carry).  carry = (rho [n, D, D], running sum [n], step index, total [n], clip cursor); `start` = a carry to resume from (the cursor then
    indexes the clip handed to THIS call, i.e. restart it at 0 with the overlap column first), None: rho_0 at t_0 with total 0."""
    real, cplx = O._dt(dtype)
    v = var if dtype == "f32" else var.astype(np.float64)
    R, freqs, _, _ = O.effective_params(hp, v, dtype)
    A = real(v.A)
    S, F, L, _ = plan_counts(plan)
    if clip is not None:
        clip = np.asarray(clip, dtype=real)
        clip = clip[None, :] if clip.ndim == 1 else clip
    if n is None:
        n = np.shape(noise)[1] if noise is not None else clip.shape[0]
    noise = np.zeros((0, n), dtype=real) if noise is None else np.asarray(noise, dtype=real)
    assert noise.shape == (L, n)
    if S + F:
        clip = np.tile(clip, (n, 1)) if clip.shape[0] == 1 else clip
        assert clip.shape == (n, clip_columns(plan))
    if start is None:
        rho = np.tile(O.rho_0(np.asarray(Wx, dtype=real), np.asarray(Wy, dtype=real), dtype)[None], (n, 1, 1))
        run, k0, total = np.zeros(n, dtype=real), 0, np.zeros(n, dtype=real)
    else:
        rho, run, k0, total = start[0].astype(cplx), start[1].astype(real), int(start[2]), start[3].astype(real)
    t = O.time_table(hp.delta_t, k0 + S + F + L, dtype)                       # t_0 = 0, t += dt per step, forced or sampled
    D = rho.shape[-1]
    nll, pred, out = np.empty((n, S), dtype=real), np.empty((n, S + F), dtype=real), np.empty((n, L), dtype=real)
    rhos = np.empty((n, S + F + L, D, D), dtype=cplx)
    c = jn = jf = js = 0
    for j, (kind, skip) in enumerate(expand(plan)):
        tk = t[k0 + j]
        edt = (_expect(rho, tk, R, freqs, dtype) * real(hp.delta_t)).astype(real)
        if kind == SAMPLE:                                                    # _rho_and_sample_update
            inc = (edt + noise[js]).astype(real)                              # :162
            run = (run + inc).astype(real)                                    # :163
            out[:, js] = run
            js += 1
        else:                                                                 # _rho_update
            c += skip
            inc = (clip[:, c + 1] - clip[:, c]).astype(real)                  # :138
            c += 1
            pred[:, jf] = edt
            run = np.zeros(n, dtype=real)
            jf += 1
        st = O._rho_step(rho, inc, tk, R, freqs, A, hp, dtype)                # :164 / :147 / :154
        if kind == SCORE:
            lv = (-np.log(real(1) + st["z"])).astype(real)                    # :155, :166 on the updated, un-normalised rho'
            nll[:, jn] = lv
            total = (total + lv).astype(real)
            jn += 1
        rho = (st["new_rho"] * (real(1) / st["m"]).astype(cplx)[:, None, None]).astype(cplx)      # :165 / :201-203
        rhos[:, j] = rho
    purity = np.einsum('abcd,abdc->ab', rhos, rhos).real.astype(real)         # :101
    return nll, total, pred, (A * out).astype(real), rhos, purity, (rho, run, k0 + S + F + L, total, c)


# ---------------------------------------------------------------------------------------------------
# shared cases: the model of tests/_rho_primed_ref.py, damped-sine clips seeded with D
# ---------------------------------------------------------------------------------------------------
# (D, rank, variant, rank1 option, n, scored segments) of tests/test_gpu_rho_stream_score.py, the families of _rho_stream_ref.GPU_CASES;
# variant 0 = AUTO, 1 = BLOCK; rank1 2 = BF16X3
GPU_CASES = [(7, 7, 0, None, 1, (1, 3)),
             (20, 9, 0, None, 3, (63, 1, 1, 65)),
             (32, 32, 0, None, 5, (64, 64, 65)),
             (32, 4, 0, 2, 2, (65, 1, 40)),
             (32, 32, 1, None, 3, (40, 30)),
             (40, 3, 0, None, 2, (33, 1, 40)),
             (96, 96, 0, None, 2, (3, 2, 5))]


@functools.lru_cache(maxsize=None)
def case_clip(D, rank, n, columns):
    """O.damped_sine(n, columns, dt, seed=D) on case_model(D, rank): computed once, shared, never written to."""
    clip = O.damped_sine(n, columns, oracle_side(case_model(D, rank))[0].delta_t, seed=D)
    clip.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def case_reference(D, rank, n, segments, dtype="f32"):
    """rho_score_reference of a case whose plan scores `segments` (a tuple of step counts) from k0 = 0: (nll, total, pred, rhos, purity),
    computed once per (case, dtype) and shared by the tests that need it."""
    plan = [(SCORE, m) for m in segments]
    clip = case_clip(D, rank, n, clip_columns(plan))
    ohp, ov, Wx, Wy = oracle_side(case_model(D, rank))
    nll, total, pred, _, rhos, pur, _ = rho_score_reference(ohp, ov, Wx, Wy, plan, clip, None, dtype)
    for a in (nll, total, pred, rhos, pur):
        a.setflags(write=False)
    return nll, total, pred, rhos, pur
