"""The hand-derived adjoints of oracle/ against automatic differentiation of a restated forward (tests/_autograd_ref.py), on the CPU.

(a) Every gradient path of oracle/ -- C.psi_scan and O.psi_loss_and_grads ("f64" and "f64t32"), O.rho_loss_and_grads (both),
    O.legacy_loss_and_grads -- agrees with the twin to 1e-10 (rel_inf per tensor, per-clip losses relative to max(|loss_b|, 1)): two
    float64 evaluations of one function.  The effective-parameter cotangents are compared as the scans emit them, and the raw-variable
    gradients through the automatically differentiated raw -> effective map of tests/_step_ref.py.
(b) The check functions the GPU module asserts with reject a wrong kernel: the float32 oracle, handed over as the "kernel result",
    passes; three deliberately wrong results each fail.

The clips lie on a 16-bit grid (multiples of 2^-15): the twin takes the increments as float32 differences, as the reference and the
kernels do, the float64 modes of oracle/ take them as float64 differences of the float32 clip, and on that grid both are exact --
the same function.  (On an arbitrary float32 clip the two differ by the rounding of one float32 subtraction, 6e-8 of an increment.)

Measured worst case of (a) over the cases below, on one machine (the condition is 1e-10):
    PsiCMPS  C.psi_scan              5.1e-15   (psi0bar of "floor", f64t32)
    PsiCMPS  O.psi_loss_and_grads    1.2e-14   (Abar of "d7_sigma1", f64t32)
    RhoCMPS  O.rho_loss_and_grads    2.1e-15   (fbar of "d5_r2", f64t32)
    legacy   O.legacy_loss_and_grads 5.3e-16   (gR of "d5", f64t32)
"near_floor" (a case of this module's own: a step with 0 < |y|^2 < 1e-12, so that the floored branch CHANGES the gradient, which it
does not where the state is annihilated exactly) meets the condition on its loss, Rbar and fbar; psi0bar and Abar, which flow back
through the 1e6 of the floored step, are held to a 60-digit derivative instead (test_near_floor_gradient_against_60_digit_differences:
2.4e-8 at worst, for the twin and both oracle paths alike).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
from oracle import c_oracle as C
import _autograd_ref as AR
from _util import make_audio

torch.set_num_threads(min(8, torch.get_num_threads()))

TWIN_RTOL = 1e-10
GRIDS = ("f64", "f64t32")


def pcm(audio):
    """The clip on the 16-bit grid: float32 values whose float32 differences are exact."""
    return (np.round(np.asarray(audio, dtype=np.float64) * 2.0 ** 15) / 2.0 ** 15).astype(np.float32)


def _agree(label, got, want, worst):
    e = AR.loss_err(got, want) if label.endswith("per_clip") else AR.rel_inf(got, want)
    worst.append((e, label))
    return e


def _assert_all(worst, rtol=None):
    """Every (error, label) within TWIN_RTOL, or within ``rtol[label]`` where the case prices a quantity itself."""
    e, label = max(worst)
    print(f"worst {e:.2e} ({label})")
    bad = [(l, x) for x, l in worst if not x <= (rtol or {}).get(l, TWIN_RTOL)]
    assert not bad, bad


def _pairs(g, names):
    """Raw gradients as the complex tensors they are parts of: Rx + i Ry, psi_x + i psi_y, Wx + i Wy (a part that vanishes by symmetry
    is rounding noise on both sides and has no scale of its own)."""
    g = g if isinstance(g, dict) else {k: getattr(g, k) for k in names}
    out = {"A": np.asarray(g["A"]), "freqs": np.asarray(g["freqs"]), "R": np.asarray(g["Rx"]) + 1j * np.asarray(g["Ry"])}
    if "psi_x" in names:
        out["psi"] = np.asarray(g["psi_x"]) + 1j * np.asarray(g["psi_y"])
    if "Wx" in names:
        out["W"] = np.asarray(g["Wx"]) + 1j * np.asarray(g["Wy"])
    return out


# ---------------------------------------------------------------------------------------------------
# PsiCMPS
# ---------------------------------------------------------------------------------------------------
FLOOR_a, FLOOR_A = 2.0, 4.0                            # tests/test_gpu_parity.py::test_normalisation_floor_branch
PSI_CASES = {
    "d1": dict(D=1, T=30, B=2),                                                     # R = 0 after model.py:42
    "floor": dict(D=2, T=40, B=3, floor="exact"),                                   # |y|^2 = 0 at step 0 of clip 1
    "near_floor": dict(D=2, T=40, B=3, floor="near"),                               # 0 < |y|^2 < 1e-12 there: the branch changes the gradient
    "d7_sigma1": dict(D=7, T=130, B=3, sigma=1.0, rscale=0.1),
    "d17_silent": dict(D=17, T=300, B=2, silent=True),                              # a silent first third
    "d32_sigma": dict(D=32, T=60, B=5, sigma=0.36, A=66.0, rscale=0.69, amp=0.09),  # test_qbar_sums_visible_at_large_sigma's configuration
    "d32_long": dict(D=32, T=300, B=4),
    "d32_t600": dict(D=32, T=600, B=2),                                             # (for the time-table mutant; beyond the T <= 300 of the rest)
}


@functools.lru_cache(maxsize=None)
def psi_case(name):
    c = dict(PSI_CASES[name])
    D, T, B = c["D"], c["T"], c["B"]
    if c.get("floor"):
        hp = O.HParams(minibatch_size=B, bond_dim=D, sigma=0.0, A=FLOOR_A)
        p = np.float32(np.sqrt(0.5))
        if c["floor"] == "near":                       # psi_0 = (p + 4 ulp, p - 4 ulp): (I + s R) psi_0 = (8 ulp, -8 ulp) exactly, |y|^2 = 4.5e-13
            psi_in = np.array([p + 4 * np.spacing(p), p - 4 * np.spacing(p)], dtype=np.complex64)
        else:
            psi_in = np.array([1, 1], dtype=np.complex64)
        var = O.init_variables(hp, R_in=np.array([[0, FLOOR_a], [FLOOR_a, 0]], dtype=np.complex64),
                               freqs_in=np.array([3.0, -5.0], dtype=np.float32), psi_in=psi_in)
        audio = make_audio(B, T, hp.delta_t, 77, noise=0.05)
        audio[1, 0] = 0.0
        audio[1, 1] = -FLOOR_A / FLOOR_a              # s R u = -u at step 0 of clip 1
    else:
        hp = O.HParams(minibatch_size=B, bond_dim=D, sigma=c.get("sigma", 1e-4), A=c.get("A", 100.0))
        var = O.init_variables(hp, seed=D + T)
        var.Rx, var.Ry = var.Rx * np.float32(c.get("rscale", 1.0)), var.Ry * np.float32(c.get("rscale", 1.0))
        audio = (make_audio(B, T, hp.delta_t, D) * np.float32(c.get("amp", 1.0))).astype(np.float32)
        if c.get("silent"):
            audio[:, : T // 3] = 0.0
    return hp, var, pcm(audio)


def psi_effective(name, grid):
    """(R, freqs, psi_0, A, c_r, c_h) in float64 as the oracle's own a1 / a2 give them: the input of both sides."""
    hp, var, _ = psi_case(name)
    v64 = var.astype(np.float64)
    R, f, c_r, c_h = O.effective_params(hp, v64, grid)
    return R, f, O.psi_0(v64, grid), float(var.A), float(c_r), float(c_h)


@functools.lru_cache(maxsize=None)
def psi_twin(name, grid):
    hp, _, audio = psi_case(name)
    R, f, p0, A, _, _ = psi_effective(name, grid)
    aux = {}
    out = AR.psi_twin(audio, R, f, p0, A, hp.delta_t, hp.sigma, grid, aux=aux)
    out["norm"] = aux["norm"]
    return out


def test_the_floor_cases_take_the_floored_branch():
    """Clip 1 is floored from step 0 on in "floor" (annihilated exactly, the state stays zero), at step 0 alone in "near_floor"
    (0 < |y|^2 < 1e-12, the state recovers), and no other step of any case is."""
    for name in PSI_CASES:
        n = psi_twin(name, "f64t32")["norm"]
        floored = np.argwhere(n <= AR.FLOOR).tolist()
        want = {"exact": [[1, k] for k in range(n.shape[1])], "near": [[1, 0]], None: []}[PSI_CASES[name].get("floor")]
        assert floored == want, (name, floored)
    assert np.all(psi_twin("floor", "f64t32")["norm"][1] == 0.0)
    assert 1e-13 < psi_twin("near_floor", "f64t32")["norm"][1, 0] < AR.FLOOR
    assert all(np.all(np.isfinite(psi_twin(name, g)["per_clip"])) for name in PSI_CASES for g in GRIDS)


THROUGH_THE_FLOOR = ("psi0bar", "Abar", "raw psi", "raw A")


def _near_floor_rtol(name, grid):
    """"near_floor" leaves what flows back through its floored step to test_near_floor_gradient_against_60_digit_differences: no float64
    evaluation has ten digits of it.  Its loss, Rbar and fbar stay under the common condition."""
    return {k: np.inf for k in THROUGH_THE_FLOOR} if name == "near_floor" else None


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(PSI_CASES))
def test_psi_c_oracle_adjoint_is_the_twins_gradient(name, grid):
    hp, _, audio = psi_case(name)
    R, f, p0, A, _, _ = psi_effective(name, grid)
    tw = psi_twin(name, grid)
    ref = C.psi_scan(audio, R, f, p0, A, hp.delta_t, hp.sigma, grid, want_grad=True)
    g = C.unpack_grad(ref["grad"], hp.bond_dim)
    worst = []
    _agree("per_clip", ref["loss_per_clip"], tw["per_clip"], worst)
    for k in AR.PSI_KEYS:
        _agree(k, g[k], tw[k], worst)
    _assert_all(worst, _near_floor_rtol(name, grid))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(PSI_CASES))
def test_psi_numpy_oracle_adjoint_is_the_twins_gradient(name, grid):
    hp, var, audio = psi_case(name)
    B = audio.shape[0]
    _, _, _, _, c_r, c_h = psi_effective(name, grid)
    tw = psi_twin(name, grid)
    ref = O.psi_loss_and_grads(hp, var.astype(np.float64), audio, grid)
    worst = []
    _agree("per_clip", ref.per_clip, tw["per_clip"], worst)
    for k in AR.PSI_KEYS:                              # the oracle's effective cotangents are those of the MEAN loss
        _agree(k, np.asarray(ref.eff[k]) * B, tw[k], worst)
    raw = AR.raw_gradients({k: getattr(var, k) for k in O.Variables.NAMES}, {k: tw[k] / B for k in AR.PSI_KEYS}, c_r, c_h)
    got, want = _pairs(ref, O.Variables.NAMES), _pairs(raw, O.Variables.NAMES)
    for k in want:
        _agree("raw " + k, got[k], want[k], worst)
    _assert_all(worst, _near_floor_rtol(name, grid))


NEAR_FLOOR_RTOL = 1e-6


def _mp_clip_gradient(x, t, R, f, p0, A):
    """(psi0bar [2] complex, Abar) of one D = 2, sigma = 0 clip by central differences of the fold written in 60-digit arithmetic
    (model.py:276-282, 293-334 once more, in mpmath): no adjoint and no automatic differentiation."""
    import mpmath as mp
    with mp.workdps(60):
        Rm = [[mp.mpc(float(R[i, j].real), float(R[i, j].imag)) for j in range(2)] for i in range(2)]
        floor, h = mp.mpf("1e-12"), mp.mpf("1e-25")

        def loss(psi, a):
            total = mp.mpf(0)
            for k in range(len(x)):
                s = mp.mpf(float(x[k])) / a
                ph = [mp.expj(mp.mpf(float(f[d])) * mp.mpf(float(t[k]))) for d in range(2)]
                U = [psi[d] * mp.conj(ph[d]) for d in range(2)]
                psi = [psi[d] + ph[d] * s * (Rm[d][0] * U[0] + Rm[d][1] * U[1]) for d in range(2)]
                Up = [psi[d] * mp.conj(ph[d]) for d in range(2)]
                e = 2 * mp.re(sum(mp.conj(Up[d]) * (Rm[d][0] * Up[0] + Rm[d][1] * Up[1]) for d in range(2)))
                total -= mp.log(1 + e * mp.mpf(float(x[k])) / a)
                ss = sum(mp.re(z) ** 2 + mp.im(z) ** 2 for z in psi)
                psi = [z / mp.sqrt(max(ss, floor)) for z in psi]
            return total

        P, a0 = [mp.mpc(float(z.real), float(z.imag)) for z in p0], mp.mpf(float(A))

        def d(fn):
            return float((fn(h) - fn(-h)) / (2 * h))
        bar = [complex(d(lambda e, i=i: loss([P[j] + (e if j == i else 0) for j in range(2)], a0)),
                       d(lambda e, i=i: loss([P[j] + (1j * e if j == i else 0) for j in range(2)], a0))) for i in range(2)]
        return np.array(bar), d(lambda e: loss(P, a0 + e))


@pytest.mark.parametrize("grid", GRIDS)
def test_near_floor_gradient_against_60_digit_differences(grid):
    """The floored clip of "near_floor" alone (B = 1).  The floored step multiplies the cotangent by rsqrt(1e-12) = 1e6, and what comes
    back is a difference of such terms: psi0bar = (I + s R)^dagger (1e6 g) keeps 1e-5 of them, Abar's 1e6 Re<g, R u> x / A^2 1e-4.  A
    relative rounding of 1e-16 therefore arrives as 1e-10 ... 1e-8 in ANY float64 evaluation (measured against the 60-digit derivative:
    twin 1.1e-9 / 1.0e-8, C oracle 8.6e-11 / 2.4e-8, numpy oracle 1.7e-10 / 2.0e-8 for psi0bar / Abar at worst over the two grids), so the condition here is 1e-6 -- 1e10 roundings, five orders
    below what differentiating through the floor changes (4.5e-1 of psi0bar, the third mutant) -- for the twin as for both oracle paths."""
    hp, var, audio = psi_case("near_floor")
    one = audio[1:2]
    R, f, p0, A, _, _ = psi_effective("near_floor", grid)
    x = (one[0, 1:] - one[0, :-1]).astype(np.float64)
    truth = dict(zip(("psi0bar", "Abar"), _mp_clip_gradient(x, AR.time_grid(hp.delta_t, len(x), grid), R, f, p0, A)))
    c = C.unpack_grad(C.psi_scan(one, R, f, p0, A, hp.delta_t, hp.sigma, grid, want_grad=True)["grad"], 2)
    o = O.psi_loss_and_grads(hp, var.astype(np.float64), one, grid).eff
    worst = []
    for who, g in (("twin", AR.psi_twin(one, R, f, p0, A, hp.delta_t, hp.sigma, grid)), ("C", c), ("numpy", o)):
        for k in truth:
            e = AR.rel_inf(g[k], truth[k])
            print(f"{who:5s} {k:8s} {e:.2e}")
            worst.append((e, who + " " + k))
    assert max(worst)[0] <= NEAR_FLOOR_RTOL, worst


# ---------------------------------------------------------------------------------------------------
# RhoCMPS
# ---------------------------------------------------------------------------------------------------
RHO_CASES = {
    "d5_r2": dict(D=5, rank=2, T=40, B=2),
    "d8_r3": dict(D=8, rank=3, T=66, B=3, sigma=0.5, rscale=0.3),
    "d20_r9": dict(D=20, rank=9, T=129, B=2, sigma=0.2, rscale=0.5),
    "d32_r32": dict(D=32, rank=32, T=96, B=3),
    "d40_r6": dict(D=40, rank=6, T=40, B=2),
    "d5_trace": dict(D=5, rank=2, T=40, B=2, A=3.0, rscale=0.25, amp=3.0, sigma=0.5),      # s Rt of order 1: the trace leaves 1 by far
}


@functools.lru_cache(maxsize=None)
def rho_case(name):
    c = RHO_CASES[name]
    D, T, B = c["D"], c["T"], c["B"]
    hp = O.HParams(minibatch_size=B, bond_dim=D, initial_rank=c["rank"], sigma=c.get("sigma", 1e-4), A=c.get("A", 100.0))
    var = O.init_variables(hp, seed=D + T)
    var.Rx, var.Ry = var.Rx * np.float32(c.get("rscale", 1.0)), var.Ry * np.float32(c.get("rscale", 1.0))
    var.psi_x, var.psi_y = np.zeros(D, np.float32), np.zeros(D, np.float32)
    Wx, Wy = O.rho_init_W(hp, seed=D)
    audio = (make_audio(B, T, hp.delta_t, D) * np.float32(c.get("amp", 1.0))).astype(np.float32)
    return hp, var, Wx, Wy, pcm(audio)


@functools.lru_cache(maxsize=None)
def rho_twin(name, grid):
    hp, var, Wx, Wy, audio = rho_case(name)
    R, f, _, _ = O.effective_params(hp, var.astype(np.float64), grid)
    aux = {}
    out = AR.rho_twin(audio, R, f, Wx, Wy, float(var.A), hp.delta_t, hp.sigma, grid, aux=aux)
    out["norm"] = aux["norm"]
    return out


def test_the_trace_case_is_far_from_one_and_above_the_floor():
    tr = rho_twin("d5_trace", "f64t32")["norm"]
    print(f"trace of the un-normalised rho: {tr.min():.3g} ... {tr.max():.3g}")
    assert tr.min() > 1e3 * AR.FLOOR and np.max(np.abs(tr - 1.0)) > 0.5          # (the ordinary cases stay within 1e-2 of 1)
    assert np.all(np.isfinite(rho_twin("d5_trace", "f64t32")["per_clip"]))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(RHO_CASES))
def test_rho_oracle_adjoint_is_the_twins_gradient(name, grid):
    hp, var, Wx, Wy, audio = rho_case(name)
    v64 = var.astype(np.float64)
    _, _, c_r, c_h = O.effective_params(hp, v64, grid)
    tw = rho_twin(name, grid)
    ref = O.rho_loss_and_grads(hp, v64, Wx.astype(np.float64), Wy.astype(np.float64), audio, grid)
    assert np.all(np.isfinite(ref["per_clip"]))
    worst = []
    _agree("per_clip", ref["per_clip"], tw["per_clip"], worst)
    for k in ("Rbar", "fbar", "Abar"):
        _agree(k, ref["eff"][k], tw[k], worst)
    raw = AR.raw_gradients({k: getattr(var, k) for k in ("Rx", "Ry", "freqs", "A")}, tw, float(c_r), float(c_h))
    raw.update(Wx=tw["Wx"], Wy=tw["Wy"])
    got, want = _pairs(ref, AR.RHO_KEYS), _pairs(raw, AR.RHO_KEYS)
    for k in want:
        _agree("raw " + k, got[k], want[k], worst)
    _assert_all(worst)


# ---------------------------------------------------------------------------------------------------
# legacy AudioMPS
# ---------------------------------------------------------------------------------------------------
LEGACY_CASES = {"d5": (5, 60, 3, 0.01), "d32": (32, 66, 3, 0.004), "d40": (40, 34, 2, 0.004)}


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(LEGACY_CASES))
def test_legacy_oracle_adjoint_is_the_twins_gradient(name, grid):
    """The oracle's legacy arithmetic has no float32 constants of its own in float64: "f64t32" hands it dt as the float32 value."""
    D, T, B, dt = LEGACY_CASES[name]
    H, R = O.legacy_init(D, seed=D)
    audio = pcm(make_audio(B, T, dt, D, noise=0.05))
    tw = AR.legacy_twin(audio, H, R, dt, grid)
    ref = O.legacy_loss_and_grads(H.astype(np.float64), R.astype(np.float64), AR.const32(dt, grid), audio, "f64")
    worst = []
    _agree("per_clip", ref["per_clip"], tw["per_clip"], worst)
    for k in AR.LEGACY_KEYS:
        _agree(k, ref[k], tw[k], worst)
    assert np.all(np.triu(tw["gH"], 1) == 0)           # only the lower triangle of H is read
    _assert_all(worst)


# ---------------------------------------------------------------------------------------------------
# (b) the checks catch a wrong kernel
# ---------------------------------------------------------------------------------------------------
def _c_result(name, dtype, sigma=None):
    """C.psi_scan as a "kernel result" in the keys of check_psi."""
    hp, var, audio = psi_case(name)
    v = var if dtype == "f32" else var.astype(np.float64)
    R, f, _, _ = O.effective_params(hp, v, dtype)
    out = C.psi_scan(audio, R, f, O.psi_0(v, dtype), float(var.A), hp.delta_t, hp.sigma if sigma is None else sigma, dtype, want_grad=True)
    g = C.unpack_grad(out["grad"], hp.bond_dim)
    return dict({k: g[k] for k in AR.PSI_KEYS}, per_clip=out["loss_per_clip"])


def _show(label, records):
    for what, err, bar in records:
        print(f"{label:28s} {what:8s} err {err:.2e}  bar {bar:.2e}{'   FAILS' if not err <= bar else ''}")


@pytest.mark.parametrize("name", list(PSI_CASES))
def test_the_float32_oracle_passes_its_check(name):
    ref32 = _c_result(name, "f32")
    rec = AR.check_psi(ref32, psi_twin(name, "f64t32"), ref32)
    _show(name, rec)
    assert not AR.failures(rec)


def test_mutant_sigma_squared_scaled_is_rejected():
    """sigma^2 x 1.01 at the sigma-visible shape: Q = -(dt sigma^2 / 2) R^dagger R is 1 % off in every step."""
    ref32 = _c_result("d32_sigma", "f32")
    wrong = _c_result("d32_sigma", "f32", sigma=0.36 * np.sqrt(1.01))
    rec = AR.check_psi(wrong, psi_twin("d32_sigma", "f64t32"), ref32)
    _show("sigma^2 x 1.01", rec)
    assert AR.failures(rec)


def test_mutant_time_table_as_a_product_is_rejected():
    """t_k = float32(k dt) instead of the float32 running sum.  Every addition inside one binade of t rounds the same way, so the two
    tables part by up to k / 2 units in the last place of t_k: the phase f t_k is off by a multiple of k^2.  At T = 300 that leaves the
    frequency gradient at about half its bar (5.5e-5 of 1e-4; the loss at 9.2e-6 of 1e-5), so the mutant runs at T = 600, four times
    the phase error."""
    name = "d32_t600"
    hp, _, audio = psi_case(name)
    N = audio.shape[1] - 1
    R, f, p0, A, _, _ = psi_effective(name, "f64t32")
    product = (np.arange(N, dtype=np.float64) * hp.delta_t).astype(np.float32)
    drift = np.max(np.abs(product - AR.time_grid(hp.delta_t, N, "f64t32"))[1:] / product[1:])
    print(f"largest relative distance of the two tables {drift:.2e}")
    wrong = AR.psi_twin(audio, R, f, p0, A, hp.delta_t, hp.sigma, "f64t32", times=product)
    rec = AR.check_psi(wrong, psi_twin(name, "f64t32"), _c_result(name, "f32"))
    _show("t_k = float32(k dt)", rec)
    assert AR.failures(rec)


def test_mutant_floor_differentiated_through_is_rejected():
    """The floored step's gradient as if max(ss, 1e-12) were ss (a straight-through floor: same forward, the norm's derivative kept)."""
    def through(ss, floor):
        return ss + (torch.maximum(ss, floor) - ss).detach()
    hp, _, audio = psi_case("near_floor")
    R, f, p0, A, _, _ = psi_effective("near_floor", "f64t32")
    tw = psi_twin("near_floor", "f64t32")
    wrong = AR.psi_twin(audio, R, f, p0, A, hp.delta_t, hp.sigma, "f64t32", maximum=through)
    np.testing.assert_array_equal(wrong["per_clip"], tw["per_clip"])          # the forward is untouched
    rec = AR.check_psi(wrong, tw, _c_result("near_floor", "f32"))
    _show("floor differentiated", rec)
    assert AR.failures(rec)
