"""k_classify_weights on a real MI355X against tests/_disc_ref.py, in guarded buffers (tests/_guard.py): the weights and the record each
between two red zones, the gaps of a padded weight matrix compared with the guard's pattern, losses and labels with their snapshots.

The counts, the skipped clips' and absent members' +0 are exact.  The bars are the ones include/cmps.h derives for
cmps_bank_classify_weights (ROUNDING); the device and the float64 reference each meet them, so the two differ by at most twice:
  |w - exact| <= 2^-24 |exact| + 2^-52 (alpha + beta kappa) (M + 16) + 2^-149
  |sum_xent - exact| <= 2^-52 n_used (M + 32 + 2 kappa L + sum xent),     |sum_own_loss - exact| <= 2^-53 n_used sum |l_y|.
"""
import numpy as np
import pytest
import torch

import _classify_ref as CR
import _disc_ref as DR
import _guard as G
from test_gpu_classify_stats import _Lib, _case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 5), (5, 255), (5, 257), (1024, 3)]
PARAMS = [(1.0, 0.0, 1.0), (0.01, 0.5, 2.0)]                     # (inv_temp, gen_weight, disc_weight)
NAN_F32 = np.uint32(G.NAN_FILL).view(np.float32)


class Lib(_Lib):
    def rec40(self, dirty=None):
        g = G.Guarded(40, self.dev, align=256, fill=G.NAN_FILL, name="record")
        if dirty is not None:
            g.load(np.resize(dirty, 40).astype(np.uint8))
        return g

    def weights(self, loss, labels, params, reset, rec, ld=None, ldw=None):
        """``loss`` float32 [M, B] uploaded with rows ``ld`` apart -> (weights [M, B], record as a dict); the weight matrix has rows ``ldw``
        apart and exactly the documented extent, its gaps must keep the guard's pattern."""
        M, B = loss.shape
        ld, ldw = B if ld is None else ld, B if ldw is None else ldw
        padded = np.full((M, ld), NAN_F32, np.float32)
        padded[:, :B] = loss
        g_loss = self.const(padded.reshape(-1)[:(M - 1) * ld + B].copy(), "loss")
        g_lab = self.const(np.ascontiguousarray(labels, dtype=np.int32), "labels")
        n_w = (M - 1) * ldw + B
        g_w = G.Guarded(4 * n_w, self.dev, align=256, fill=G.NAN_FILL, name="weights")
        code = self.lib.cmps_bank_classify_weights(self.h, g_loss.ptr, M, B, ld, g_lab.ptr, *params, reset, g_w.ptr, ldw, rec.ptr, self.stream())
        assert code == self.capi.CMPS_OK, self.lib.cmps_last_error(self.h)
        torch.cuda.synchronize(self.dev)
        for g in (rec, g_w):
            assert g.zones_intact() is None, (g.name, g.zones_intact())
        for g in self.inputs:
            assert g.zones_intact() is None and g.equals_snapshot() is None, g.name
        flat = np.concatenate([g_w.numpy(np.float32), np.full(M * ldw - n_w, NAN_F32, np.float32)]).reshape(M, ldw)
        assert np.all(flat[:, B:].view(np.uint32) == np.uint32(G.NAN_FILL)), "the gaps between the weight rows were written"
        raw = rec.numpy(np.uint8).view(self.capi.CLASSIFY_WEIGHTS_REC)[0]
        return flat[:, :B].copy(), {k: (float(raw[k]) if k.startswith("sum") else int(raw[k])) for k in DR.FIELDS}


def labels32(lab):
    """What the device reads of a label: its low 32 bits as an int."""
    return np.asarray(lab, dtype=np.int64).astype(np.int32).astype(np.int64)


def _case_w(M, B, seed, scale_max):
    x, lab = _case(M, B, seed, scale_max=scale_max)
    return x, labels32(lab)


def check(w, rec, x, lab, params, parts, what):
    """Device weights of ONE call against the reference; the record against ``parts``, every call since the reset."""
    M, B = x.shape
    kappa, alpha, beta = params
    ref = parts[-1]
    skipped = ref["state"] != 0
    absent = ~np.isfinite(x)
    assert np.all(w.view(np.uint32)[:, skipped] == 0), what                            # bit-exact +0
    assert np.all(w.view(np.uint32)[absent] == 0), what
    err = np.abs(w.astype(np.float64) - ref["w64"])
    bar = 2.0 * DR.weight_bound(ref["w64"], M, kappa, alpha, beta)
    want = DR.record(parts)
    assert all(rec[k] == want[k] for k in DR.FIELDS[2:]), (what, rec, want)
    xs = [p["x"] for p in parts]
    L = max([float(np.abs(a[np.isfinite(a)]).max()) if np.isfinite(a).any() else 0.0 for a in xs])
    own = np.concatenate([p["own"] for p in parts])
    bar_x, bar_o = DR.record_bounds(want, M, kappa, L, float(np.nansum(np.abs(own))))
    e_x, e_o = abs(rec["sum_xent"] - want["sum_xent"]), abs(rec["sum_own_loss"] - want["sum_own_loss"])
    print(f"{what}: used {want['n_used']} max |w - ref| / bar {float(np.max(err / bar)):.3f}  |sum_xent - ref| {e_x:.3e} (bar {2 * bar_x:.3e})  "
          f"|sum_own - ref| {e_o:.3e} (bar {2 * bar_o:.3e})")
    assert np.all(err <= bar), (what, float(np.max(err / bar)))
    assert e_x <= 2 * bar_x and e_o <= 2 * bar_o, (what, e_x, bar_x, e_o, bar_o)


def ref_of(x, lab, params):
    r = DR.weights(x, lab, *params)
    r["x"] = x
    return r


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("M,B", SHAPES)
def test_one_call_against_the_reference(M, B, params):
    lib = Lib()
    try:
        # unit temperature: losses up to 1e5 apart, far members whose p underflows to 0; the soft one: losses within a few hundred
        x, lab = _case_w(M, B, 1000 * M + B, scale_max=5 if params[0] == 1.0 else 2)
        pad = (M, B) == (5, 257)
        ld, ldw = (B + 5, B + 3) if pad else (None, None)                               # rows further apart than they are long, once
        w, rec = lib.weights(x, lab, params, 1, lib.rec40(), ld=ld, ldw=ldw)            # reset over the guard's pattern: no memset needed
        check(w, rec, x, lab, params, [ref_of(x, lab, params)], f"M={M} B={B} params={params}")
        w2, rec2 = lib.weights(x, lab, params, 1, lib.rec40(dirty=np.array([0xFF], np.uint8)), ld=ld, ldw=ldw)
        assert np.array_equal(w.view(np.uint32), w2.view(np.uint32)) and rec == rec2   # the same call, the same bits, whatever was there
    finally:
        lib.close()


def test_hand_made_clips_ties_far_members_and_one_member():
    lib = Lib(D=1)
    try:
        nan, inf = np.nan, np.inf
        #              tie     far (p = 0)  own absent  other absent  all absent  unlabelled  label -1
        x = np.array([[2.0,    1.0,         nan,        nan,          nan,        1.0,        1.0],
                      [2.0,    2000.0,      4.0,        4.0,          inf,        2.0,        2.0],
                      [7.0,    3000.0,      6.0,        6.0,          -inf,       3.0,        3.0]], np.float32)
        lab = np.array([1, 0, 0, 2, 1, 3, -1])
        params = (1.0, 0.25, 1.0)
        w, rec = lib.weights(x, lab, params, 1, lib.rec40())
        check(w, rec, x, lab, params, [ref_of(x, lab, params)], "by hand")
        assert (rec["n_used"], rec["n_unlabelled"], rec["n_own_absent"]) == (3, 2, 2)
        assert np.all(w.view(np.uint32)[1:, 1] == 0) and w[0, 1] == np.float32(0.25)   # the far members: exactly +0; the own: alpha alone
        # gen_weight alone: the own member's weight is exactly 1, every other exactly +0
        w, rec = lib.weights(x, lab, (3.0, 1.0, 0.0), 1, lib.rec40())
        want = np.zeros_like(x)
        want[1, 0] = want[0, 1] = want[2, 3] = 1.0
        assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
        # M = 1
        one = np.array([[2.5, nan, -1.0]], np.float32)
        w, rec = lib.weights(one, np.array([0, 0, 1]), (0.5, 0.25, 3.0), 1, lib.rec40())
        assert np.array_equal(w.view(np.uint32), np.array([[0.25, 0.0, 0.0]], np.float32).view(np.uint32))
        assert rec == {"sum_xent": 0.0, "sum_own_loss": 2.5, "n_used": 1, "n_unlabelled": 1, "n_own_absent": 1}
    finally:
        lib.close()


def test_reset_0_continues_the_record_and_unit_temperature_agrees_with_classify_stats():
    lib = Lib(D=48)
    try:
        M, params = 5, (1.0, 0.0, 1.0)
        cases = [_case_w(M, 257, 41, 3), _case_w(M, 100, 42, 3), _case_w(M, 255, 43, 3)]
        runs = []
        for _ in range(2):
            rec = lib.rec40()
            parts = []
            for i, (x, lab) in enumerate(cases):
                w, got = lib.weights(x, lab, params, 1 if i == 0 else 0, rec)
                parts.append(ref_of(x, lab, params))
                check(w, got, x, lab, params, parts, f"call {i}")
            runs.append(got)
        assert runs[0] == runs[1]                                                      # the same sequence, the same bits
        # kappa = 1: the xent is cmps_bank_classify_stats's, clip for clip -- the two records agree within the two headers' bounds
        stats = lib.record(M)
        ref = CR.Record(M)
        first = 0
        for i, (x, lab) in enumerate(cases):
            raw, _ = lib.call(x, lab, first, 1 if i == 0 else 0, stats, want_best=False)
            ref.add(x, lab, first)
            first += x.shape[1]
        head = raw.view(lib.capi.classify_stats_dtype(M))[0]["head"]
        assert int(head["n_xent"]) == runs[0]["n_used"] > 100
        L = max(float(np.abs(x[np.isfinite(x)]).max()) for x, _ in cases)
        bar = DR.record_bounds(DR.record(parts), M, 1.0, L, 0.0)[0] + ref.bounds()[0]
        diff = abs(float(head["sum_xent"]) - runs[0]["sum_xent"])
        print(f"sum_xent: classify_weights {runs[0]['sum_xent']!r} classify_stats {float(head['sum_xent'])!r} diff {diff:.3e} bar {bar:.3e}")
        assert diff <= bar
    finally:
        lib.close()


def test_through_hipscan_and_the_kernel_events():
    from audio_mps_amd.scan import HipScan
    be = HipScan(20)
    x, lab = _case_w(6, 300, 21, 2)
    params = (0.05, 0.5, 1.5)
    loss = torch.from_numpy(x).to(be.device)
    labels = torch.from_numpy(lab.astype(np.int32)).to(be.device)
    be.kernel_events(True)
    whole = torch.full((6, 300), 7.0, dtype=torch.float32, device=be.device)
    w, rec = be.classify_weights(loss[:, :200], labels[:200].contiguous(), *params, weights=whole[:, :200])      # views: ld = ldw = 300 > B
    assert w.data_ptr() == whole.data_ptr() and rec.dtype == torch.uint8 and rec.numel() == 40
    w2, rec2 = be.classify_weights(loss[:, 200:], labels[200:].contiguous(), *params, weights=whole[:, 200:], record=rec, reset=False)
    assert rec2 is rec
    got = be.read_classify_weights_record(rec)
    times = be.kernel_times()
    be.kernel_events(False)
    assert list(times) == ["k_classify_weights"] and times["k_classify_weights"][1] == 2
    ref = ref_of(x, lab, params)
    check(whole.cpu().numpy(), got, x, lab, params, [ref], "HipScan, two halves")
    fresh, _ = be.classify_weights(loss, labels, *params)                               # allocated by the method: the same bits
    assert torch.equal(fresh.view(torch.int32), whole.view(torch.int32))
    for bad in (loss.double(), loss.reshape(-1), loss.cpu(), loss.t()):
        with pytest.raises(ValueError, match="classify_weights"):
            be.classify_weights(bad, labels, *params)
    with pytest.raises(ValueError, match="labels"):
        be.classify_weights(loss, labels[:10].contiguous(), *params)
    with pytest.raises(ValueError, match="record"):
        be.classify_weights(loss, labels, *params, record=torch.empty(64, dtype=torch.uint8, device=be.device))
    with pytest.raises(ValueError, match="weights"):
        be.classify_weights(loss, labels, *params, weights=torch.empty((6, 10), dtype=torch.float32, device=be.device))
