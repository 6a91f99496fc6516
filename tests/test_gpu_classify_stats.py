"""k_classify_stats on a real MI355X against tests/_classify_ref.py, in guarded buffers (tests/_guard.py): the record, `best_dev` and the
losses each between two red zones, the labels and losses compared with their snapshots after every call.

Every count, `best`, the confusion matrix, `unlabelled_best` and `first_undecided` must be exact.  The bars of the two sums are the ones
include/cmps.h states for cmps_bank_classify_stats (ROUNDING), computed by _classify_ref.Record.bounds for exactly the clips fed:
  |sum_xent - exact| <= 2^-52 n_xent (M + 40 + 2 L + sum xent),     |sum_margin - exact| <= 2^-52 n_margin (sum margin).
"""
import ctypes

import numpy as np
import pytest
import torch

import _classify_ref as CR
import _guard as G

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 63), (3, 64), (3, 65), (88, 257), (1024, 5)]


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

    def const(self, x, name):
        g = G.Guarded(x.nbytes, self.dev, align=256, fill=G.NAN_FILL, name=name)
        g.load(x)
        g.snapshot(x)
        self.inputs.append(g)
        return g

    def record(self, M, dirty=None):
        n = int(self.lib.cmps_bank_classify_stats_bytes(M))
        assert n == 72 + 8 * M * M + 8 * M
        g = G.Guarded(n, self.dev, align=256, fill=G.NAN_FILL, name="stats")
        if dirty is not None:
            g.load(np.resize(dirty, n).astype(np.uint8))
        return g

    def call(self, loss, labels, first_id, reset, rec, ld=None, want_best=True):
        """``loss`` float32 [M, B] (uploaded with rows ``ld`` apart, the gaps holding the guard's NaN pattern) -> (record bytes, best)."""
        M, B = loss.shape
        ld = B if ld is None else ld
        padded = np.full((M, ld), np.uint32(G.NAN_FILL).view(np.float32), np.float32)
        padded[:, :B] = loss
        flat = padded.reshape(-1)[:(M - 1) * ld + B].copy()                             # exactly the documented extent
        g_loss = self.const(flat, "loss")
        g_lab = self.const(np.ascontiguousarray(labels, dtype=np.int32), "labels") if labels is not None else None
        g_best = G.Guarded(4 * B, self.dev, align=256, fill=G.NAN_FILL, name="best") if want_best else None
        code = self.lib.cmps_bank_classify_stats(self.h, g_loss.ptr, M, B, ld, g_lab.ptr if g_lab else None, first_id, reset, rec.ptr,
                                                 g_best.ptr if g_best else None, self.stream())
        assert code == self.capi.CMPS_OK, self.lib.cmps_last_error(self.h)
        torch.cuda.synchronize(self.dev)
        for g in [rec] + ([g_best] if g_best else []):
            assert g.zones_intact() is None, (g.name, g.zones_intact())
        for g in self.inputs:
            assert g.zones_intact() is None and g.equals_snapshot() is None, g.name
        return rec.numpy(np.uint8), (g_best.numpy(np.int32) if g_best else None)

    def close(self):
        self.lib.cmps_destroy(self.h)


def _case(M, B, seed, scale_max=5):
    """Losses of mixed magnitude (up to 1e5) with planted ties, NaN / +-Inf members and all-absent clips; labels in and outside [0, M)."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal((M, B))) * 10.0 ** rng.integers(-2, scale_max + 1, (1, B))).astype(np.float32)
    x[rng.random((M, B)) < 0.1] *= -1.0
    lab = rng.integers(0, M, B)
    for b in range(B):
        r = rng.random()
        if r < 0.15 and M >= 2:                                        # a tie for the minimum between two members
            i, j = rng.choice(M, 2, replace=False)
            x[i, b] = x[j, b] = x[:, b].min() - np.float32(1.0)
        elif r < 0.30:                                                 # absent members, the label's own among them now and then
            k = rng.integers(1, M + 1)
            x[rng.choice(M, k, replace=False), b] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), k)
        elif r < 0.38:
            x[:, b] = np.nan                                           # nobody present: undecided
        elif r < 0.45:
            x[:, b] = x[0, b]                                          # every member the same loss
    lab = lab.astype(np.int64)
    out = rng.random(B) < 0.2
    lab[out] = rng.choice(np.array([-1, M, M + 7, -2 ** 31, 2 ** 31 - 1], np.int64), int(out.sum()))
    return x, lab


def _check(raw, best, ref: CR.Record, n_new, what=""):
    from audio_mps_amd import _capi
    M = ref.M
    got, want = raw.view(_capi.classify_stats_dtype(M))[0], ref.record()
    for k in CR.HEAD[2:]:
        assert int(got["head"][k]) == want[k], (what, k, int(got["head"][k]), want[k])
    assert np.array_equal(got["confusion"], want["confusion"]), what
    assert np.array_equal(got["unlabelled_best"], want["unlabelled_best"]), what
    if best is not None:
        assert np.array_equal(best, want["best"][-n_new:]), what
    bar_x, bar_m = ref.bounds()
    e_x, e_m = abs(float(got["head"]["sum_xent"]) - want["sum_xent"]), abs(float(got["head"]["sum_margin"]) - want["sum_margin"])
    print(f"{what}: n_xent {want['n_xent']} |sum_xent - exact| {e_x:.3e} (bar {bar_x:.3e})  n_margin {want['n_margin']} "
          f"|sum_margin - exact| {e_m:.3e} (bar {bar_m:.3e})")
    assert e_x <= bar_x and e_m <= bar_m, (what, e_x, bar_x, e_m, bar_m)


@pytest.mark.parametrize("M,B", SHAPES)
def test_one_call_against_the_reference(M, B):
    lib = _Lib()
    try:
        x, lab = _case(M, B, 1000 * M + B)
        first = 2 ** 40 + 3                                                            # ids beyond 32 bits
        ld = B + 5 if (M, B) == (3, 65) else None                                      # rows further apart than they are long, once
        raw, best = lib.call(x, lab, first, 1, lib.record(M), ld=ld)                   # reset over the guard's pattern: no memset needed
        _check(raw, best, CR.Record(M).add(x, lab, first), B, f"M={M} B={B}")
        again, best2 = lib.call(x, lab, first, 1, lib.record(M, dirty=np.array([0xFF], np.uint8)), ld=ld)
        assert np.array_equal(raw, again) and np.array_equal(best, best2)              # the same call, the same bytes, whatever was there
    finally:
        lib.close()


@pytest.mark.parametrize("M,B", [(3, 65), (88, 257)])
def test_three_calls_continue_one_record(M, B):
    lib = _Lib(D=48)
    try:
        parts = [_case(M, B, 7 + M)[:2], _case(M, B // 2 + 1, 8 + M), _case(M, B, 9 + M)]
        whole, labels = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts])
        runs = []
        for _ in range(2):
            rec, first = lib.record(M), 11
            for i, (x, lab) in enumerate(parts):
                raw, best = lib.call(x, lab, first, 1 if i == 0 else 0, rec)
                first += x.shape[1]
            runs.append(raw)
        ref = CR.Record(M)
        first = 11
        for x, lab in parts:
            ref.add(x, lab, first)
            first += x.shape[1]
        _check(runs[0], best, ref, parts[-1][0].shape[1], f"M={M} three calls")
        assert np.array_equal(runs[0], runs[1])                                        # the same sequence, the same bytes
        one, _ = lib.call(whole, labels, 11, 1, lib.record(M))                         # ... and one call on the concatenation
        from audio_mps_amd import _capi
        a, b = (r.view(_capi.classify_stats_dtype(M))[0] for r in (runs[0], one))
        for k in CR.HEAD[2:]:
            assert a["head"][k] == b["head"][k], k
        assert np.array_equal(a["confusion"], b["confusion"]) and np.array_equal(a["unlabelled_best"], b["unlabelled_best"])
        _check(one, None, CR.Record(M).add(whole, labels, 11), 0, f"M={M} concatenated")
    finally:
        lib.close()


def test_no_labels_no_best_and_an_all_undecided_batch():
    lib = _Lib(D=1)
    try:
        x, _ = _case(5, 70, 3)
        raw, best = lib.call(x, None, 0, 1, lib.record(5), want_best=False)            # label_dev == NULL, best_dev == NULL
        assert best is None
        ref = CR.Record(5).add(x, None, 0)
        _check(raw, None, ref, 0, "no labels")
        want = ref.record()
        assert want["n_xent"] == 0 and want["n_correct"] == 0 and want["n_unlabelled"] == want["n_decided"] and not want["confusion"].any()
        nobody = np.full((4, 130), np.inf, np.float32)
        raw, best = lib.call(nobody, np.zeros(130, np.int64), 40, 1, lib.record(4))
        from audio_mps_amd import _capi
        got = raw.view(_capi.classify_stats_dtype(4))[0]
        assert (int(got["head"]["n_undecided"]), int(got["head"]["n_decided"]), int(got["head"]["first_undecided"])) == (130, 0, 40)
        assert float(got["head"]["sum_xent"]) == 0.0 and float(got["head"]["sum_margin"]) == 0.0 and not got["confusion"].any()
        assert np.array_equal(best, np.full(130, -1, np.int32))
    finally:
        lib.close()


def test_through_hipscan_and_the_kernel_events():
    from audio_mps_amd.scan import HipScan
    be = HipScan(20)
    x, lab = _case(6, 300, 21)
    loss = torch.from_numpy(x).to(be.device)
    labels = torch.from_numpy(lab.astype(np.int32)).to(be.device)
    best = torch.full((300,), 77, dtype=torch.int32, device=be.device)
    be.kernel_events(True)
    st = be.classify_stats(loss[:, :200], labels[:200].contiguous(), 0, best=best[:200])          # a view: ld = 300 > B = 200
    assert st.dtype == torch.uint8 and st.numel() == 72 + 8 * 36 + 8 * 6 and st.is_cuda
    assert be.classify_stats(loss[:, 200:], labels[200:].contiguous(), 200, st, best=best[200:]) is st
    got = be.read_classify_stats(st, 6)
    times = be.kernel_times()
    be.kernel_events(False)
    assert list(times) == ["k_classify_stats"] and times["k_classify_stats"][1] == 2
    ref = CR.Record(6).add(x, lab, 0)
    want = ref.record()
    assert all(got[k] == want[k] for k in CR.HEAD[2:])
    assert np.array_equal(got["confusion"], want["confusion"]) and np.array_equal(got["unlabelled_best"], want["unlabelled_best"])
    assert np.array_equal(best.cpu().numpy(), want["best"])
    bar_x, bar_m = ref.bounds()
    assert abs(got["sum_xent"] - want["sum_xent"]) <= bar_x and abs(got["sum_margin"] - want["sum_margin"]) <= bar_m
    for bad in (loss.double(), loss.reshape(-1), loss.cpu(), loss.t()):
        with pytest.raises(ValueError, match="classify_stats"):
            be.classify_stats(bad, None, 0)
    with pytest.raises(ValueError, match="stats"):
        be.classify_stats(loss, None, 0, torch.empty(64, dtype=torch.uint8, device=be.device))
    with pytest.raises(ValueError, match="labels"):
        be.classify_stats(loss, labels[:10].contiguous(), 0)
