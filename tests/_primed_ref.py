"""What a primed sampler run must give, composed from the oracle's public step primitives: P = prime_T - 1 teacher-forced steps of
_psi_update (model.py:269-274) on the clip's increments (model.py:263), then `length` steps of _psi_and_sample_update (:284-291),
one time grid through both.  `dtype` is handed to every primitive, so the same composition exists in float32 and in float64."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O


def primed_reference(hp: O.HParams, var: O.Variables, prime, noise, dtype="f32"):
    """prime [n_prime, prime_T] (n_prime = n, or 1: shared), noise [length, n] (the reference's layout) ->
    (out [n, length] = A * running sum of the sampled increments, pred [n, prime_T - 1] = expectation * delta_t before each forced step)."""
    real = np.float32 if dtype == "f32" else np.float64
    cplx = np.complex64 if dtype == "f32" else np.complex128
    v = var if dtype == "f32" else var.astype(np.float64)
    R, freqs, _, _ = O.effective_params(hp, v, dtype)
    A = real(v.A)
    noise = np.asarray(noise, dtype=real)
    length, n = noise.shape
    prime = np.asarray(prime, dtype=real)
    if prime.ndim == 1:
        prime = prime[None, :]
    if prime.shape[0] == 1:
        prime = np.tile(prime, (n, 1))
    assert prime.shape[0] == n and prime.shape[1] >= 2
    incs = (prime[:, 1:] - prime[:, :-1]).astype(real)                       # model.py:263
    P = incs.shape[1]
    t = O.time_table(hp.delta_t, P + length, dtype)                          # t_0 = 0, t += dt per step, forced or sampled
    psi = np.tile(O.psi_0(v, dtype)[None, :], (n, 1)).astype(cplx)           # model.py:245
    pred = np.empty((n, P), dtype=real)
    for k in range(P):                                                       # _psi_update
        pred[:, k] = O.expectation(psi, t[k], R, freqs, dtype) * real(hp.delta_t)
        psi = O.update_ancilla_psi(psi, incs[:, k], t[k], R, freqs, A, hp, dtype)
        psi = O.normalize_psi(psi, axis=1, dtype=dtype)
    sample = np.zeros(n, dtype=real)                                         # model.py:244, restarted at the hand-over
    out = np.empty((length, n), dtype=real)
    for k in range(length):                                                  # _psi_and_sample_update
        tk = t[P + k]
        inc = (O.expectation(psi, tk, R, freqs, dtype) * real(hp.delta_t) + noise[k]).astype(real)    # :286
        sample = (sample + inc).astype(real)                                                          # :287
        psi = O.update_ancilla_psi(psi, inc, tk, R, freqs, A, hp, dtype)                              # :288
        psi = O.normalize_psi(psi, axis=1, dtype=dtype)                                               # :289
        out[k] = sample
    return (A * out.T).astype(real), pred                                                             # :251


# ---------------------------------------------------------------------------------------------------
# the test model of tests/test_gpu_parity.py::test_sampling_matches_oracle, as the oracle sees it
# ---------------------------------------------------------------------------------------------------
def case_hparams(D, n):
    return O.HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0)


def case_variables(D, n):
    """The raw variables PsiCMPS(HParams(...), seed=D) draws (audio_mps_amd.model.CMPS.__init__ / PsiCMPS.__init__ and
    O.init_variables share the order of the draws), with Rx, Ry scaled by 0.05."""
    var = O.init_variables(case_hparams(D, n), seed=D)
    var.Rx = var.Rx * np.float32(0.05)
    var.Ry = var.Ry * np.float32(0.05)
    return var


@functools.lru_cache(maxsize=None)
def case_inputs(D, P, length, n):
    """(prime [n, P + 1] damped sine, noise [length, n] at temp 0.5) of a case; computed once, shared, never written to."""
    hp = case_hparams(D, n)
    prime = O.damped_sine(n, P + 1, hp.delta_t, seed=D)
    noise = O.sample_noise(hp, n, length, temp=0.5, seed=D)
    prime.setflags(write=False)
    noise.setflags(write=False)
    return prime, noise


@functools.lru_cache(maxsize=None)
def case_reference(D, P, length, n, dtype="f32"):
    """primed_reference of a case: (out, pred), computed once per (case, dtype) and shared by the tests that need it."""
    prime, noise = case_inputs(D, P, length, n)
    out, pred = primed_reference(case_hparams(D, n), case_variables(D, n), prime, noise, dtype)
    out.setflags(write=False)
    pred.setflags(write=False)
    return out, pred
