"""What a primed RhoCMPS sampler run must give, composed from the oracle's own step functions the way O.rho_sample is: P = prime_T - 1
teacher-forced steps of _rho_update (model.py:144-150: _rho_step plus trace normalisation) on the clip's increments (model.py:138), with
pred = Re tr(X rho) * delta_t (the expression of model.py:162) taken BEFORE each step, then `length` steps of _rho_and_sample_update
(:160-167), one time grid through both.  `dtype` is handed to every primitive, so the same composition exists in float32 and float64."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O


def _expect(rho, t, R, freqs, dtype):
    """Re tr((Rt + Rt^dagger) rho) per path on the current rho (model.py:189-196), as O.rho_sample forms it."""
    real, cplx = O._dt(dtype)
    ph = O._phases(freqs, real(t), dtype)
    Rt = (ph[:, None] * R * np.conj(ph)[None, :]).astype(cplx)
    X = (Rt + np.conj(Rt.T)).astype(cplx)
    return np.einsum('ab,cba->c', X, rho).real.astype(real)


def rho_primed_reference(hp: O.HParams, var: O.Variables, Wx, Wy, prime, noise, dtype="f32"):
    """prime [n_prime, prime_T] (n_prime = n, or 1: shared), noise [length, n] (the reference's layout) ->
    (out [n, length] = A * running sum of the sampled increments, pred [n, P], rhos [n, P + length, D, D] after every step, forced steps
    first, purity [n, P + length])."""
    real, cplx = O._dt(dtype)
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
    incs = (prime[:, 1:] - prime[:, :-1]).astype(real)                       # model.py:138
    P = incs.shape[1]
    t = O.time_table(hp.delta_t, P + length, dtype)                          # t_0 = 0, t += dt per step, forced or sampled
    rho = np.tile(O.rho_0(np.asarray(Wx, dtype=real), np.asarray(Wy, dtype=real), dtype)[None], (n, 1, 1))
    pred = np.empty((n, P), dtype=real)
    rhos = []

    def step(rho, inc, tk):                                                  # _update_ancilla_rho + _normalize_rho
        st = O._rho_step(rho, inc, tk, R, freqs, A, hp, dtype)
        return (st["new_rho"] * (real(1) / st["m"]).astype(cplx)[:, None, None]).astype(cplx)

    for k in range(P):                                                       # _rho_update
        pred[:, k] = _expect(rho, t[k], R, freqs, dtype) * real(hp.delta_t)
        rho = step(rho, incs[:, k], t[k])
        rhos.append(rho)
    sample = np.zeros(n, dtype=real)                                         # restarted at the hand-over
    out = np.empty((length, n), dtype=real)
    for k in range(length):                                                  # _rho_and_sample_update
        tk = t[P + k]
        inc = (_expect(rho, tk, R, freqs, dtype) * real(hp.delta_t) + noise[k]).astype(real)      # :162
        sample = (sample + inc).astype(real)                                                      # :163
        rho = step(rho, inc, tk)                                                                  # :164-165
        rhos.append(rho)
        out[k] = sample
    rhos = np.stack(rhos, axis=1)
    purity = np.einsum('abcd,abdc->ab', rhos, rhos).real.astype(real)                             # :101
    return (A * out.T).astype(real), pred, rhos, purity                                           # :116


# ---------------------------------------------------------------------------------------------------
# the test model of tests/test_gpu_rho.py::test_rho_gemm_sampler_matches_block_sampler (sigma = 0.1, Rx, Ry *= 0.3, A = 5, seed 17)
# ---------------------------------------------------------------------------------------------------
# (D, rank, P, length, n) of tests/test_gpu_rho_primed.py: P and P + length on both sides of the 64-step chunk, a partly filled workgroup
# (n = 5), rank 9 at padded D = 20, both column homes of the block kernel (D = 40: LDS; D = 96, rank 96: the workspace)
GPU_CASES = [(7, 7, 1, 3, 1), (20, 9, 63, 70, 3), (32, 32, 64, 130, 5), (32, 4, 65, 64, 2), (32, 32, 100, 40, 3), (40, 3, 33, 40, 2),
             (96, 96, 5, 7, 2)]


def case_model(D, rank, backend=None):
    """The product's RhoCMPS of a case (its constructor draws the variables; no backend is touched until a scan runs)."""
    from audio_mps_amd import HParams, RhoCMPS
    hp = HParams(minibatch_size=2, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    m = RhoCMPS(hp, seed=17, backend=backend)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m


def oracle_side(m):
    """(oracle HParams, oracle Variables, Wx, Wy) of a RhoCMPS (tests/test_gpu_rho.py::_oracle_side)."""
    D = m.bond_d
    ov = O.Variables(np.asarray(m.variables["A"], dtype=np.float32), m.variables["Rx"].copy(), m.variables["Ry"].copy(),
                     m.variables["freqs"].copy(), np.zeros(D, np.float32), np.zeros(D, np.float32),
                     scaled_R=float(m._c_r) != 1.0, scaled_freqs=float(m._c_h) != 1.0)
    return O.HParams(**m.hparams.values()), ov, m.variables["Wx"].copy(), m.variables["Wy"].copy()


def R_fro(D, rank):
    """|R|_F of a case's effective R."""
    ohp, ov, _, _ = oracle_side(case_model(D, rank))
    return float(np.linalg.norm(O.effective_params(ohp, ov.astype(np.float64), "f64")[0]))


@functools.lru_cache(maxsize=None)
def case_inputs(D, rank, P, length, n, loud=False):
    """(prime [n, P + 1] damped sine, noise [length, n] at temp 0.5) of a case; computed once, shared, never written to.
    loud: the clip scaled so that max |s_k| |R|_F = 1 (s_k = increment / A)."""
    ohp = oracle_side(case_model(D, rank))[0]
    prime = O.damped_sine(n, P + 1, ohp.delta_t, seed=D)
    if loud:
        s_max = float(np.max(np.abs(np.diff(prime.astype(np.float64), axis=1)))) / ohp.A
        prime = (prime / (s_max * R_fro(D, rank))).astype(np.float32)
    noise = O.sample_noise(ohp, n, length, temp=0.5, seed=D)
    prime.setflags(write=False)
    noise.setflags(write=False)
    return prime, noise


@functools.lru_cache(maxsize=None)
def case_reference(D, rank, P, length, n, dtype="f32"):
    """rho_primed_reference of a case: (out, pred, rhos, purity), computed once per (case, dtype) and shared by the tests that need it."""
    prime, noise = case_inputs(D, rank, P, length, n)
    ohp, ov, Wx, Wy = oracle_side(case_model(D, rank))
    res = rho_primed_reference(ohp, ov, Wx, Wy, prime, noise, dtype)
    for x in res:
        x.setflags(write=False)
    return res
