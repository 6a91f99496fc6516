"""What a resumable RhoCMPS sampler run must give for a *plan*, a list of (forced, sampled) segments: tests/_rho_primed_ref.py::
rho_primed_reference generalised the way tests/_stream_ref.py generalises the pure-state one, composed from the same oracle primitives
(O._rho_step, _expect, O.rho_0, O.time_table).  One time grid runs through all segments; a forced step takes its increment from the clip
(model.py:138), resets the running sum to 0 and records Re tr((Rt + Rt^dagger) rho) * delta_t before the step; a sampled step adds its
noise to that expectation (model.py:162) and continues the running sum.  The forced steps of all segments read ONE clip
[n_audio, 1 + total forced] in order, the sampled steps one noise array [total sampled, n] in order (tests/_stream_ref.py).  The function is
a plain loop over the steps of the expanded plan, so it cannot depend on the segmentation; tests/test_rho_stream_host.py asserts that once."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O
from _stream_ref import plan_steps, expand, refine            # noqa: F401  (re-exported: the plan helpers are the pure-state ones)
from _rho_primed_ref import _expect, case_model, oracle_side, R_fro      # noqa: F401


def rho_stream_reference(hp: O.HParams, var: O.Variables, Wx, Wy, plan, clip, noise, dtype="f32", start=None, n=None):
    """clip [n_audio, 1 + F] (n_audio = n, or 1: shared; may be None when F = 0), noise [L, n] (may be None when L = 0; then the path count
    is `n`, or the clip's rows) -> (out [n, L], pred [n, F], rhos [n, F + L, D, D] after every step, purity [n, F + L], carry).
    `start` = a carry (rho [n, D, D], running sum [n], step index) to resume from; None: rho_0 at t_0."""
    real, cplx = O._dt(dtype)
    v = var if dtype == "f32" else var.astype(np.float64)
    R, freqs, _, _ = O.effective_params(hp, v, dtype)
    A = real(v.A)
    F, L = plan_steps(plan)
    if clip is not None:
        clip = np.asarray(clip, dtype=real)
        clip = clip[None, :] if clip.ndim == 1 else clip
    if n is None:
        n = np.shape(noise)[1] if noise is not None else clip.shape[0]
    noise = np.zeros((0, n), dtype=real) if noise is None else np.asarray(noise, dtype=real)
    assert noise.shape == (L, n)
    if F:
        clip = np.tile(clip, (n, 1)) if clip.shape[0] == 1 else clip
        assert clip.shape == (n, F + 1)
        incs = (clip[:, 1:] - clip[:, :-1]).astype(real)                      # model.py:138
    if start is None:
        rho = np.tile(O.rho_0(np.asarray(Wx, dtype=real), np.asarray(Wy, dtype=real), dtype)[None], (n, 1, 1))
        total, k0 = np.zeros(n, dtype=real), 0
    else:
        rho, total, k0 = start[0].astype(cplx), start[1].astype(real), int(start[2])
    t = O.time_table(hp.delta_t, k0 + F + L, dtype)                           # t_0 = 0, t += dt per step, forced or sampled
    D = rho.shape[-1]
    out, pred = np.empty((n, L), dtype=real), np.empty((n, F), dtype=real)
    rhos = np.empty((n, F + L, D, D), dtype=cplx)

    def step(rho, inc, tk):                                                   # _update_ancilla_rho + _normalize_rho
        st = O._rho_step(rho, inc, tk, R, freqs, A, hp, dtype)
        return (st["new_rho"] * (real(1) / st["m"]).astype(cplx)[:, None, None]).astype(cplx)

    jf = js = 0
    for j, forced in enumerate(expand(plan)):
        tk = t[k0 + j]
        edt = _expect(rho, tk, R, freqs, dtype) * real(hp.delta_t)
        if forced:                                                            # _rho_update
            pred[:, jf] = edt
            inc = incs[:, jf]
            total = np.zeros(n, dtype=real)
            jf += 1
        else:                                                                 # _rho_and_sample_update
            inc = (edt + noise[js]).astype(real)                              # :162
            total = (total + inc).astype(real)                                # :163
            out[:, js] = total
            js += 1
        rho = step(rho, inc, tk)                                              # :164-165
        rhos[:, j] = rho
    purity = np.einsum('abcd,abdc->ab', rhos, rhos).real.astype(real)         # :101
    return (A * out).astype(real), pred, rhos, purity, (rho, total, k0 + F + L)   # :116


# ---------------------------------------------------------------------------------------------------
# shared cases: the model of tests/_rho_primed_ref.py, inputs of the kind tests/_stream_ref.py uses (damped-sine clips, noise at temp 0.5)
# ---------------------------------------------------------------------------------------------------
# (D, rank, variant, rank1 option, n, plan) of tests/test_gpu_rho_stream.py; variant 0 = AUTO, 1 = BLOCK; rank1 2 = BF16X3
GPU_CASES = [(7, 7, 0, None, 1, ((1, 0), (0, 3))),
             (20, 9, 0, None, 3, ((63, 0), (1, 0), (0, 1), (0, 63), (37, 70))),
             (32, 32, 0, None, 5, ((64, 0), (0, 64), (65, 65))),
             (32, 4, 0, 2, 2, ((65, 0), (0, 1), (0, 40), (30, 34))),
             (32, 32, 1, None, 3, ((40, 30), (0, 40))),
             (40, 3, 0, None, 2, ((33, 40), (1, 1))),
             (96, 96, 0, None, 2, ((3, 0), (0, 2), (2, 5)))]


@functools.lru_cache(maxsize=None)
def case_inputs(D, rank, plan, n):
    """(clip [n, 1 + F], noise [L, n]) of a case; computed once, shared, never written to."""
    ohp = oracle_side(case_model(D, rank))[0]
    F, L = plan_steps(plan)
    clip = O.damped_sine(n, F + 1, ohp.delta_t, seed=D)
    noise = O.sample_noise(ohp, n, max(L, 1), temp=0.5, seed=D)[:L]
    clip.setflags(write=False)
    noise.setflags(write=False)
    return clip, noise


@functools.lru_cache(maxsize=None)
def case_reference(D, rank, plan, n, dtype="f32"):
    """rho_stream_reference of a case: (out, pred, rhos, purity), computed once per (case, dtype) and shared by the tests that need it."""
    clip, noise = case_inputs(D, rank, plan, n)
    ohp, ov, Wx, Wy = oracle_side(case_model(D, rank))
    res = rho_stream_reference(ohp, ov, Wx, Wy, plan, clip, noise, dtype)[:4]
    for x in res:
        x.setflags(write=False)
    return res
