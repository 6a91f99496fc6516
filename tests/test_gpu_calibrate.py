"""cmps_bank_calibrate on the GPU against tests/_calib_ref.py: the closed forms, stationarity of the returned theta evaluated in long
double within the header's rounding bounds, the box, and the memory and determinism contract.  Every buffer is a tests/_guard.py Guarded:
loss_dev, theta and the record sit between red zones, the rows of loss_dev are padded to ld = N + 3 with the guard's NaN fill, and the
inputs are compared with their snapshots after the call."""
import ctypes

import numpy as np
import pytest

import _calib_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


def run(loss, labels, N, fit, kappa, c, tol=TOL, max_iter=1000, kmin=1e-6, kmax=1e6, events=False, fill=None):
    """One call on a fresh handle: (kappa, c, record dict, raw bytes of theta | record, kernel names or None)."""
    import torch
    import _guard
    from audio_mps_amd import _capi
    drv = _guard.Driver(8, fill=_guard.NAN_FILL if fill is None else fill,
                        options=((_capi.CMPS_OPT_KERNEL_EVENTS, 1),) if events else ())
    try:
        M, ld = loss.shape
        theta0 = np.concatenate([[kappa], np.asarray(c, dtype=np.float64)])
        lo, la = drv.load("loss", loss), drv.load("label", np.asarray(labels, dtype=np.int32))
        th = drv.load("theta", theta0, const=False)
        rec = drv.new("record", 80, out=torch.int32)
        nbytes = int(drv.lib.cmps_bank_calibrate_scratch_bytes(M, N))
        assert nbytes > 0
        scr = drv.new("scratch", nbytes)
        drv.call("cmps_bank_calibrate", lo, M, N, ld, la, fit, max_iter, tol, kmin, kmax, th, rec, scr, nbytes)
        drv.finish()
        theta = th.numpy(np.float64)
        record = {k: rec.numpy(np.uint8).view(_capi.CALIB_REC)[0][k].item() for k in _capi.CALIB_REC.names}
        names = None
        if events:
            buf = ctypes.create_string_buffer(4096)
            ms, counts = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
            k = drv.lib.cmps_kernel_times(drv.h, buf, 4096, ms, counts, 64)
            names = dict(zip(buf.value.decode().split("\n"), list(counts)[:k]))
        return float(theta[0]), theta[1:].copy(), record, np.concatenate([th.numpy(np.uint8), rec.numpy(np.uint8)]), names
    finally:
        drv.close()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_closed_form_temperature():
    """M = 2, three clips whose own member is lower by exactly 1 and one whose own member is higher by 1: g = 0 where
    1 / (1 + exp(kappa)) = 1 / 4, kappa* = log 3, h = 3 / 16, so |kappa - log 3| <= tol / (kappa* h) < 5 tol."""
    loss = np.array([[2000.0, 2001.0, 1999.0, 2004.0], [2001.0, 2000.0, 2000.0, 2003.0]], dtype=np.float32)
    labels = np.array([0, 1, 0, 0], dtype=np.int32)
    kappa, c, rec, _, _ = run(loss, labels, 4, R.FIT_TEMPERATURE, 1.0, [0.0, 0.0])
    print("kappa", kappa, "log 3", np.log(3.0), rec)
    assert rec["flags"] == R.CONVERGED and rec["n_used"] == 4 and rec["n_unfitted"] == 0
    assert abs(kappa - np.log(3.0)) <= 10 * TOL + 1e-14
    assert abs(rec["curvature"] - 3.0 / 16.0) <= 1e-8
    assert np.array_equal(bits(c), bits([0.0, 0.0]))


def test_closed_form_prior():
    """M = 2, all losses equal, labels 5 against 3, the prior fitted from a uniform start: 5/8 and 3/8; kappa keeps its bits."""
    loss = np.full((2, 8), 1234.5, dtype=np.float32)
    labels = np.array([0, 1, 0, 0, 1, 0, 1, 0], dtype=np.int32)
    for fit in (R.FIT_PRIOR, R.FIT_PRIOR | R.FIT_TEMPERATURE):
        kappa, c, rec, _, _ = run(loss, labels, 8, fit, 0.37, [0.0, 0.0])
        prior = R.normalised_prior(c)
        print(fit, prior, rec)
        assert rec["flags"] == R.CONVERGED
        assert np.max(np.abs(prior - [5 / 8, 3 / 8])) <= TOL
        assert bits(kappa) == bits(0.37)                                 # g == 0 and h == 0: kappa keeps its start value
        assert rec["xent_end"] < rec["xent_start"] == pytest.approx(np.log(2.0), abs=1e-12)


@pytest.mark.parametrize("fit", [1, 2, 3])
@pytest.mark.parametrize("M,N", R.SHAPES)
def test_stationarity_against_the_reference(M, N, fit):
    loss, labels, N = R.draw(M, N, seed=100 + M)
    l = loss[:, :N]
    k0, c0 = R.start(l, labels, fit)
    kappa, c, rec, _, _ = run(loss, labels, N, fit, k0, c0)
    start, end = R.evaluate(l, labels, k0, c0, np.longdouble), R.evaluate(l, labels, kappa, c, np.longdouble)
    eJ0, _, _ = start.bounds()
    eJ, eg, eq = end.bounds()
    kr, cr, _ = R.optimise(l, labels, fit, k0, c0)
    best = R.evaluate(l, labels, kr, cr, np.longdouble)
    print(f"M {M} N {N} fit {fit}: kappa {kappa} (reference {float(kr)}) |kappa g| {abs(kappa * float(end.g)):.3e} resid {end.resid():.3e} "
          f"J {float(end.J)} (reference {float(best.J)}) bounds {eJ:.2e} {kappa * eg:.2e} {eq / end.n:.2e} record {rec}")
    assert rec["flags"] == R.CONVERGED
    assert (rec["n_used"], rec["n_unlabelled"], rec["n_own_absent"]) == (end.n, end.n_unlabelled, end.n_own_absent)
    assert rec["n_unfitted"] == int(np.sum(end.n_m == 0))
    if fit & R.FIT_TEMPERATURE:
        assert abs(kappa * float(end.g)) <= TOL + kappa * eg
    else:
        assert bits(kappa) == bits(k0)
    if fit & R.FIT_PRIOR:
        assert end.resid() <= TOL + eq / end.n
    else:
        assert np.array_equal(bits(c), bits(c0))
    assert np.array_equal(bits(c[end.n_m == 0]), bits(c0[end.n_m == 0]))
    assert abs(rec["xent_start"] - float(start.J)) <= eJ0 and abs(rec["xent_end"] - float(end.J)) <= eJ
    assert abs(rec["g_logk"] - kappa * float(end.g)) <= kappa * eg
    assert rec["xent_end"] <= rec["xent_start"]
    assert rec["xent_end"] - float(best.J) >= -eJ


def test_bounds_of_the_box():
    loss, labels, N = R.draw(5, 100, seed=7, specials=False)
    l = loss[:, :N].copy()
    right = l.copy()
    right[labels, np.arange(N)] = np.min(l, axis=0) - 2.0                       # every clip right by a margin
    kappa, _, rec, _, _ = run(right, labels, N, R.FIT_TEMPERATURE, 1.0, np.zeros(5), kmax=4.0)
    print(kappa, rec)
    assert rec["flags"] == R.CONVERGED | R.AT_KAPPA_MAX and kappa == 4.0
    wrong = l.copy()
    wrong[labels, np.arange(N)] = np.max(l, axis=0) + 2.0                       # every clip wrong
    kappa, _, rec, _, _ = run(wrong, labels, N, R.FIT_TEMPERATURE, 1.0, np.zeros(5), kmin=1e-3)
    print(kappa, rec)
    assert rec["flags"] & R.AT_KAPPA_MIN and rec["flags"] & R.CONVERGED and kappa == 1e-3
    # a start outside the box is put on it
    kappa, _, rec, _, _ = run(loss, labels, N, R.FIT_TEMPERATURE, 1e9, np.zeros(5))
    assert rec["flags"] == R.CONVERGED and 1e-6 < kappa < 1e6
    # ... and xent_start is J there: an always-right bank started above kappa_max, where J is lower than anywhere inside the box
    kappa, _, rec, _, _ = run(right, labels, N, R.FIT_TEMPERATURE, 40.0, np.zeros(5), kmax=4.0)
    at_max = R.evaluate(right, labels, 4.0, np.zeros(5), np.longdouble)
    assert rec["flags"] == R.CONVERGED | R.AT_KAPPA_MAX and kappa == 4.0 and rec["passes"] == 2
    assert rec["xent_end"] <= rec["xent_start"] and abs(rec["xent_start"] - float(at_max.J)) <= at_max.bounds()[0]
    assert float(R.evaluate(right, labels, 40.0, np.zeros(5), np.longdouble).J) < float(at_max.J)


def test_max_iter_returns_the_best_theta():
    loss, labels, N = R.draw(5, 300, seed=105)
    l = loss[:, :N]
    k0, c0 = R.start(l, labels, 3, kappa=7.0)
    kappa, c, rec, _, _ = run(loss, labels, N, 3, k0, c0, max_iter=1)
    print(kappa, rec)
    assert rec["flags"] == R.MAX_ITER and rec["passes"] == 2
    assert rec["xent_end"] <= rec["xent_start"]
    end = R.evaluate(l, labels, kappa, c, np.longdouble)
    assert abs(rec["xent_end"] - float(end.J)) <= end.bounds()[0]               # the figures belong to the returned theta


@pytest.mark.parametrize("M,N", [(3, 37), (65, 70)])
def test_evaluate_only_keeps_theta(M, N):
    """fit == 0 or max_iter == 0: theta keeps its bits, xent_end == xent_start, passes == 1."""
    loss, labels, N = R.draw(M, N, seed=100 + M)
    rng = np.random.default_rng(M)
    k0, c0 = 0.731, rng.standard_normal(M)
    ref = R.evaluate(loss[:, :N], labels, k0, c0, np.longdouble)
    for fit, max_iter in ((0, 0), (0, 5), (3, 0)):
        kappa, c, rec, _, _ = run(loss, labels, N, fit, k0, c0, max_iter=max_iter)
        assert bits(kappa) == bits(k0) and np.array_equal(bits(c), bits(c0))
        assert rec["xent_end"] == rec["xent_start"] and rec["passes"] == 1
        assert abs(rec["xent_start"] - float(ref.J)) <= ref.bounds()[0]
        assert rec["flags"] == (R.CONVERGED if fit == 0 else R.MAX_ITER)


def test_no_data():
    loss, labels, N = R.draw(3, 37, seed=103)
    none = np.where(np.arange(N) % 2 == 0, -1, 3).astype(np.int32)
    k0, c0 = 2.0, np.array([0.1, -0.2, 0.3])
    kappa, c, rec, _, _ = run(loss, none, N, 3, k0, c0)
    assert rec["flags"] == R.NO_DATA and rec["n_used"] == 0 and rec["n_unlabelled"] == N and rec["passes"] == 1
    assert rec["xent_start"] == 0.0 and rec["xent_end"] == 0.0
    assert bits(kappa) == bits(k0) and np.array_equal(bits(c), bits(c0))


def test_skipped_clips_and_absent_members_reach_nothing():
    """A changed loss in a skipped clip changes no bit; neither does the kind of non-finite value an absent member holds."""
    loss, labels, N = R.draw(5, 300, seed=105)
    l = loss[:, :N]
    k0, c0 = R.start(l, labels, 3)
    _, _, _, raw, _ = run(loss, labels, N, 3, k0, c0)
    ev = R.evaluate(l, labels, k0, c0)
    assert ev.n_unlabelled >= 2 and ev.n_own_absent >= 2
    other = loss.copy()
    skipped = np.flatnonzero(~ev.used)
    other[:, skipped] = np.float32(-1e30)
    for b in skipped:                                                           # (an own member that was absent stays absent)
        if 0 <= labels[b] < 5:
            other[labels[b], b] = np.float32(np.inf)
    absent = ~np.isfinite(other[:, :N]) & ev.used[None, :]
    assert absent.any()
    other[:, :N][absent] = np.float32(np.nan)
    _, _, _, raw2, _ = run(other, labels, N, 3, k0, c0)
    assert np.array_equal(raw, raw2)
    # ... and the same call gives the same bits, whatever the scratch and the outputs held before
    import _guard
    _, _, _, raw3, _ = run(loss, labels, N, 3, k0, c0, fill=_guard.ZERO_FILL)
    assert np.array_equal(raw, raw3)


def test_unfitted_members_keep_their_bits():
    """(1024, 3): 1021 members without a clip.  With a prior of zero they stay at -inf; with a finite c (J then has no minimum: the fit
    may end with MAX_ITER) they keep their bits all the same, and J does not rise."""
    loss, labels, N = R.draw(1024, 3, seed=1124)
    l = loss[:, :N]
    c0 = np.random.default_rng(5).standard_normal(1024)
    kappa, c, rec, _, _ = run(loss, labels, N, R.FIT_PRIOR, 1.0, c0, max_iter=50)
    unfitted = R.evaluate(l, labels, 1.0, c0).n_m == 0
    assert rec["n_unfitted"] == int(unfitted.sum()) == 1022
    assert np.array_equal(bits(c[unfitted]), bits(c0[unfitted])) and not np.array_equal(bits(c[~unfitted]), bits(c0[~unfitted]))
    assert rec["xent_end"] <= rec["xent_start"] and rec["flags"] in (R.CONVERGED, R.MAX_ITER)
    assert bits(kappa) == bits(1.0)


def test_kernel_events_name_the_two_kernels():
    loss, labels, N = R.draw(3, 37, seed=103)
    _, _, rec, _, names = run(loss, labels, N, 1, 1.0, np.zeros(3), max_iter=20, events=True)
    print(names, rec)
    assert names.get("k_calib_pass") == 21 and names.get("k_calib_update") == 21     # max_iter + 1 pairs, enqueued without looking
