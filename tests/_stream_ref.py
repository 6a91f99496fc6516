"""What a resumable sampler run must give for a *plan*, a list of (forced, sampled) segments: tests/_primed_ref.py::primed_reference
generalised, composed from the same oracle primitives.  One time grid runs through all segments; a forced step takes its increment from
the clip (model.py:263), resets the running sum to 0 and records expectation * delta_t; a sampled step adds its noise to that expectation
(model.py:286) and continues the running sum.  The forced steps of all segments read ONE clip [n_audio, 1 + total forced] in order (segment s
uses the columns f0 .. f0 + forced, f0 = forced steps before it: consecutive blocks overlap by one sample), the sampled steps one noise
array [total sampled, n] in order.  The function is a plain loop over the steps of the expanded plan, so it cannot depend on the
segmentation; tests/test_stream_host.py asserts that once."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O
import _primed_ref as PR


def plan_steps(plan):
    """(total forced, total sampled) of a plan."""
    return sum(f for f, _ in plan), sum(s for _, s in plan)


def expand(plan):
    """One bool per step: True = forced."""
    kinds = []
    for f, s in plan:
        assert f >= 0 and s >= 0 and f + s >= 1
        kinds += [True] * f + [False] * s
    return kinds


def refine(plan):
    """Every call of a plan cut again: in the middle of its forced part, at its forced / sampled hand-over and one step into its sampled part."""
    out = []
    for f, s in plan:
        cuts = sorted({c for c in (f // 2, f if s else 0, f + 1 if s > 1 else 0) if 0 < c < f + s})
        lo = 0
        for hi in cuts + [f + s]:
            out.append((max(min(hi, f) - min(lo, f), 0), max(hi - max(lo, f), 0)))
            lo = hi
    assert expand(out) == expand(plan) and all(a + b >= 1 for a, b in out)
    return out


def stream_reference(hp: O.HParams, var: O.Variables, plan, clip, noise, dtype="f32", start=None, n=None):
    """clip [n_audio, 1 + F] (n_audio = n, or 1: shared; may be None when F = 0), noise [L, n] (may be None when L = 0; then the path count is `n`, or
    the clip's rows) -> (out [n, L], pred [n, F], carry).  `start` = a carry (psi [n, D], running sum [n], step index) to resume from; None: psi_0 at t_0."""
    real = np.float32 if dtype == "f32" else np.float64
    cplx = np.complex64 if dtype == "f32" else np.complex128
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
        incs = (clip[:, 1:] - clip[:, :-1]).astype(real)                      # model.py:263
    if start is None:
        psi = np.tile(O.psi_0(v, dtype)[None, :], (n, 1)).astype(cplx)        # model.py:245
        total, k0 = np.zeros(n, dtype=real), 0                                # model.py:244
    else:
        psi, total, k0 = start[0].astype(cplx), start[1].astype(real), int(start[2])
    t = O.time_table(hp.delta_t, k0 + F + L, dtype)                           # t_0 = 0, t += dt per step, forced or sampled
    out, pred = np.empty((n, L), dtype=real), np.empty((n, F), dtype=real)
    jf = js = 0
    for j, forced in enumerate(expand(plan)):
        tk = t[k0 + j]
        edt = (O.expectation(psi, tk, R, freqs, dtype) * real(hp.delta_t)).astype(real)
        if forced:                                                            # _psi_update
            pred[:, jf] = edt
            inc = incs[:, jf]
            total = np.zeros(n, dtype=real)
            jf += 1
        else:                                                                 # _psi_and_sample_update
            inc = (edt + noise[js]).astype(real)                              # :286
            total = (total + inc).astype(real)                                # :287
            out[:, js] = A * total                                            # :251
            js += 1
        psi = O.update_ancilla_psi(psi, inc, tk, R, freqs, A, hp, dtype)      # :288
        psi = O.normalize_psi(psi, axis=1, dtype=dtype)                       # :289
    return out.astype(real), pred, (psi, total, k0 + F + L)


# ---------------------------------------------------------------------------------------------------
# shared cases: the model and the kind of inputs of tests/_primed_ref.py (damped-sine clips, O.sample_noise at temp 0.5)
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(D, plan, n):
    """(clip [n, 1 + F], noise [L, n]) of a case; computed once, shared, never written to."""
    hp = PR.case_hparams(D, n)
    F, L = plan_steps(plan)
    clip = O.damped_sine(n, F + 1, hp.delta_t, seed=D)
    noise = O.sample_noise(hp, n, max(L, 1), temp=0.5, seed=D)[:L]
    clip.setflags(write=False)
    noise.setflags(write=False)
    return clip, noise


@functools.lru_cache(maxsize=None)
def case_reference(D, plan, n, dtype="f32"):
    """stream_reference of a case: (out, pred), computed once per (case, dtype) and shared by the tests that need it."""
    clip, noise = case_inputs(D, plan, n)
    out, pred, _ = stream_reference(PR.case_hparams(D, n), PR.case_variables(D, n), plan, clip, noise, dtype)
    out.setflags(write=False)
    pred.setflags(write=False)
    return out, pred
