"""k_loss_stats on a real MI355X against tests/_eval_ref.Stats, in guarded buffers (tests/_guard.py): one call and three calls continuing
one record, reset over a dirty record, ties, an all-non-finite input, run-to-run identity.

Every integer field and min / max must be exact.  The bar of the two sums is the textbook bound of a summation in double in ANY order,
|s - exact| <= (n - 1) u sum|x| + O(u^2) with u = 2^-53, taken with a factor 2 to spare:
  |sum - fsum(x)| <= n_finite * 2^-52 * sum|x|,     likewise sumsq against fsum of the exact double squares (x^2 >= 0: sum|x^2| = sumsq).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _eval_ref as ER
import _guard as G

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 70001]


class _Lib:
    """One libcmps handle on the current device and stream, every pointer a Guarded's."""

    def __init__(self, D=8):
        from audio_mps_amd import _capi
        self.capi, self.lib = _capi, _capi.load()
        self.dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.h = ctypes.c_void_p()
        assert self.lib.cmps_create(D, ctypes.byref(self.h)) == _capi.CMPS_OK
        self.inputs = []

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def losses(self, x, name="loss"):
        g = G.Guarded(x.nbytes, self.dev, align=256, fill=G.NAN_FILL, name=name)
        g.load(x)
        g.snapshot(x)
        self.inputs.append(g)
        return g

    def record(self, dirty=None):
        g = G.Guarded(64, self.dev, align=256, fill=G.NAN_FILL, name="stats")
        if dirty is not None:
            g.load(dirty)
        return g

    def stats(self, loss, first_id, reset, rec):
        code = self.lib.cmps_loss_stats(self.h, loss.ptr, loss.nbytes // 4, first_id, reset, rec.ptr, self.stream())
        assert code == self.capi.CMPS_OK, self.lib.cmps_last_error(self.h)
        torch.cuda.synchronize(self.dev)
        assert rec.zones_intact() is None, rec.zones_intact()
        for g in self.inputs:
            assert g.zones_intact() is None and g.equals_snapshot() is None, g.name
        return rec.numpy(np.uint8)

    def close(self):
        self.lib.cmps_destroy(self.h)


def _values(B, seed, plant=True):
    """float32 of mixed sign and magnitude; NaN, +Inf and -Inf planted, at element 0 and at element B - 1 among others."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(B) * 10.0 ** rng.integers(-6, 7, B)).astype(np.float32)
    if plant and B >= 3:
        x[0], x[B - 1], x[B // 2] = np.nan, -np.inf, np.inf
        if B > 300:
            x[rng.integers(1, B - 1, 5)] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    return x


def _check(raw, ref: ER.Stats, what=""):
    from audio_mps_amd import _capi
    got, want = raw.view(_capi.LOSS_STATS)[0], ref.record()
    for k in ("n_finite", "n_nonfinite", "argmin", "argmax", "first_nonfinite"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    for k in ("min", "max"):
        assert np.float32(got[k]).view(np.uint32) == np.float32(want[k]).view(np.uint32), (what, k, got[k], want[k])
    n = want["n_finite"]
    e_sum, bar_sum = abs(float(got["sum"]) - want["sum"]), n * 2.0 ** -52 * want["abs_sum"]
    e_sq, bar_sq = abs(float(got["sumsq"]) - want["sumsq"]), n * 2.0 ** -52 * want["sumsq"]
    print(f"{what}: n_finite {n}  |sum - fsum| {e_sum:.3e} (bar {bar_sum:.3e})  |sumsq - fsum| {e_sq:.3e} (bar {bar_sq:.3e})")
    assert e_sum <= bar_sum and e_sq <= bar_sq, (what, e_sum, bar_sum, e_sq, bar_sq)


@pytest.mark.parametrize("B", SIZES)
def test_one_call_and_three_calls_continuing_one_record(B):
    lib = _Lib()
    try:
        x = _values(B, 100 + B)
        g = lib.losses(x)
        first = 2 ** 40 + 7                                                            # ids beyond 32 bits
        one = lib.stats(g, first, 1, lib.record())                                     # reset over the guard's pattern: no memset needed
        _check(one, ER.Stats().add(x, first), f"B={B} one call")
        again = lib.stats(g, first, 1, lib.record())
        assert np.array_equal(one, again)                                              # the same call, the same bytes
        # three calls, first_id moving on; the second batch plain, the third with its own plants
        y, z = _values(B, 200 + B, plant=False), _values(B, 300 + B)
        gy, gz = lib.losses(y, "loss2"), lib.losses(z, "loss3")
        runs = []
        for _ in range(2):
            rec = lib.record()
            lib.stats(g, 5, 1, rec)
            lib.stats(gy, 5 + B, 0, rec)
            runs.append(lib.stats(gz, 5 + 2 * B, 0, rec))
        ref = ER.Stats().add(x, 5).add(y, 5 + B).add(z, 5 + 2 * B)
        _check(runs[0], ref, f"B={B} three calls")
        assert np.array_equal(runs[0], runs[1])                                        # the same sequence, the same bytes
    finally:
        lib.close()


def test_reset_over_a_dirty_record_and_continuing_out_of_order():
    from audio_mps_amd import _capi
    lib = _Lib(D=48)
    try:
        x = _values(300, 1)
        g = lib.losses(x)
        for fill in (np.full(64, 0xFF, np.uint8), np.zeros(64, np.uint8)):
            _check(lib.stats(g, 0, 1, lib.record(fill)), ER.Stats().add(x, 0), "reset over a dirty record")
        dirty = np.zeros(1, _capi.LOSS_STATS)                                          # a record that claims a better minimum and a sum
        dirty["sum"], dirty["n_finite"], dirty["min"], dirty["argmin"], dirty["n_nonfinite"] = 1e30, 9, -3e38, 4, 77
        _check(lib.stats(g, 0, 7, lib.record(dirty.view(np.uint8))), ER.Stats().add(x, 0), "reset != 0 is any non-zero value")
        # reset == 0 does continue: the batches fed in descending id order -- ties and first_nonfinite still go to the lowest id
        y = x.copy()
        rec = lib.record()
        lib.stats(g, 1000, 1, rec)
        gy = lib.losses(y, "again")
        _check(lib.stats(gy, 10, 0, rec), ER.Stats().add(x, 1000).add(y, 10), "continued with lower ids")
    finally:
        lib.close()


@pytest.mark.parametrize("B", [2, 257, 1000])
def test_ties_take_the_lowest_id(B):
    lib = _Lib()
    try:
        rng = np.random.default_rng(B)
        x = rng.integers(-3, 4, B).astype(np.float32)                                  # seven values: ties everywhere
        x[rng.integers(0, B, 2)] = 5.0
        x[rng.integers(0, B, 2)] = -5.0
        raw = lib.stats(lib.losses(x), 11, 1, lib.record())
        _check(raw, ER.Stats().add(x, 11), f"ties B={B}")
        z = np.zeros(B, np.float32)                                                    # all equal: both at the first id; +0.0 and -0.0 tie
        z[1::2] = -0.0
        rec = lib.stats(lib.losses(z, "zeros"), 3, 1, lib.record())
        from audio_mps_amd import _capi
        got = rec.view(_capi.LOSS_STATS)[0]
        assert (int(got["argmin"]), int(got["argmax"]), int(got["n_finite"])) == (3, 3, B) and float(got["sum"]) == 0.0
    finally:
        lib.close()


@pytest.mark.parametrize("B", [1, 64, 300])
def test_all_non_finite_leaves_the_record_empty(B):
    from audio_mps_amd import _capi
    lib = _Lib(D=1)
    try:
        x = np.resize(np.array([np.inf, np.nan, -np.inf], np.float32), B)
        got = lib.stats(lib.losses(x), 40, 1, lib.record()).view(_capi.LOSS_STATS)[0]
        assert (float(got["sum"]), float(got["sumsq"]), int(got["n_finite"]), int(got["n_nonfinite"])) == (0.0, 0.0, 0, B)
        assert (int(got["argmin"]), int(got["argmax"]), int(got["first_nonfinite"])) == (-1, -1, 40)
        assert float(got["min"]) == math.inf and float(got["max"]) == -math.inf
    finally:
        lib.close()


def test_through_hipscan_and_the_kernel_events():
    from audio_mps_amd.scan import HipScan
    be = HipScan(20)
    x = _values(1000, 9)
    loss = torch.from_numpy(x).to(be.device)
    be.kernel_events(True)
    st = be.loss_stats(loss[:600].contiguous(), 0)
    assert st.dtype == torch.uint8 and st.numel() == 64 and st.is_cuda
    assert be.loss_stats(loss[600:].contiguous(), 600, st) is st
    got = be.read_stats(st)
    times = be.kernel_times()
    be.kernel_events(False)
    assert list(times) == ["k_loss_stats"] and times["k_loss_stats"][1] == 2
    want = ER.Stats().add(x, 0).record()
    assert all(got[k] == want[k] for k in ("n_finite", "n_nonfinite", "argmin", "argmax", "first_nonfinite", "min", "max"))
    assert abs(got["sum"] - want["sum"]) <= want["n_finite"] * 2.0 ** -52 * want["abs_sum"]
    for bad in (loss.double(), loss.reshape(10, 100), loss.cpu(), loss[::2]):
        with pytest.raises(ValueError, match="loss_stats"):
            be.loss_stats(bad, 0)
    with pytest.raises(ValueError, match="stats"):
        be.loss_stats(loss, 0, torch.empty(32, dtype=torch.uint8, device=be.device))
