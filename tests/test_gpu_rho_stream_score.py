"""The scored RhoCMPS stream on a real MI355X: cmps_rho_stream_score in the row-array GEMM kernel (k_sample_rho_mfma, both arithmetics) and
the block kernel (k_sample_rho, both column homes).  (a) cutting a scored run into more segments changes no bit of nll, loss, pred, the
state record or the saved rho / purity; (b) scoring perturbs nothing: pred, the record and the saved rho / purity are cmps_rho_stream's on
the same segments; (c) nll and the totals against the oracle composition (tests/_rho_score_ref.py) and against cmps_rho_loss_fwd;
(d) score / generate / score anchored; (e) error returns; (f) kernel names; (g) the memory contract; (h) the host layer.

Bars:
  * nll per step:  max |hip - nll64| <= 4 * max |nll32 - nll64| + 8 * 2^-22 * |R|_F * max|x| / A + 2^-22
                   (the first two terms are the rho pred bar of tests/test_gpu_rho_stream.py, its product-error floor carried through
                   z = e' x / A instead of e delta_t; the last is two roundings of 1 + z at 1, as in tests/test_gpu_stream_score.py)
  * totals:        |loss - total32| <= 1e-5 * max(|l|, 1)                 (the project's loss bar)
  * forward:       |loss - cmps_rho_loss_fwd| <= 2e-5 * max(|l|, 1)       (both within 1e-5 of the same oracle)
"""
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
import _guard as G
import _rho_primed_ref as RR
import _rho_score_ref as RC
from test_gpu_rho_primed import AUTO, BLOCK, OUT_RTOL, _model
from test_gpu_rho_stream import run_plan as run_followed

pytestmark = pytest.mark.gpu

CASES = RC.GPU_CASES
NLL_FLOOR = 2.0 ** -22
LOSS_RTOL = 1e-5


def refine(segments):
    """Every segment cut again at its middle and one step in."""
    return tuple(m for _, m, _ in RC.refine([(RC.SCORE, s) for s in segments]))


def run_scored(m, segments, clip, n, same_state=False, null_final=False, repeat_params=False, save=True):
    """The segments call by call through HipScan.rho_stream_score (with save_states), segment s on clip[:, f0 : f0 + steps + 1]:
    (nll [n, F], loss [n] behind the last segment, pred [n, F], the final state record as bytes, or None with null_final, rho
    [n, F, D, D] and purity [n, F] gathered call by call, or None without save).  The tables have F + 1 rows, the rho workspace rows for the
    longest call only.  The state alternates between two tensors, or (same_state) is read and written in place; repeat_params calls
    set_params and rho_set_state again, with the same arguments, behind the first segment."""
    be = m._get_backend()
    F, longest = sum(segments), max(segments)

    def prepare():
        be.set_params(m.effective_params(), n, F + 1, train=False)
        be.rho_set_state(m.columns(), n, longest + 1, train=save)

    prepare()
    states = [be.rho_stream_state(n), be.rho_stream_state(n)]
    nlls, preds, rhos, purs, cur, f0 = [], [], [], [], None, 0
    loss = np.full(n, np.nan, np.float32)                          # (not read at k0 = 0)
    for idx, f in enumerate(segments):
        if idx == len(segments) - 1 and null_final:
            nxt = None
        elif same_state:
            nxt = states[0]
        else:
            nxt = states[1] if cur is states[0] else states[0]
        nll, loss, pred = be.rho_stream_score(cur, nxt, f0, clip[:, f0:f0 + f + 1], want_nll=True, want_pred=True, n=n, loss=loss,
                                              save_states=save)
        assert nll.shape == (n, f) and pred.shape == (n, f) and loss.shape == (n,)
        if save:
            r, p = be.rho_states(n, f, want_rho=True, want_purity=True)
            rhos.append(r)
            purs.append(p)
        nlls.append(nll)
        preds.append(pred)
        cur, f0 = nxt, f0 + f
        if repeat_params and idx == 0:
            prepare()
    return (np.concatenate(nlls, axis=1), loss, np.concatenate(preds, axis=1), (None if cur is None else cur.cpu().numpy()),
            np.concatenate(rhos, axis=1) if save else None, np.concatenate(purs, axis=1) if save else None)


def _clip(D, rank, n, segments):
    return RC.case_clip(D, rank, n, sum(segments) + 1)


def _nll_bar(D, rank, clip, nll32, nll64, A):
    """(bar, d_o32) of the per-step increments of a case."""
    d_o32 = float(np.max(np.abs(nll32.astype(np.float64) - nll64)))
    x_max = float(np.max(np.abs(np.diff(np.asarray(clip, dtype=np.float64), axis=1))))
    return 4.0 * d_o32 + 8.0 * 2.0 ** -22 * RR.R_fro(D, rank) * x_max / float(A) + NLL_FLOOR, d_o32


@pytest.mark.parametrize("D,rank,variant,rank1,n,segments", CASES)
def test_cuts_are_bit_exact(D, rank, variant, rank1, n, segments):
    """(a) the plan as written against the plan with every segment cut again: nll, loss, pred, the final record and the saved rho and
    purity; the same with the state updated in place, a NULL final state_out, set_params + rho_set_state repeated between two segments, and
    one shared signal against its tiled copy."""
    m = _model(D, rank, variant, rank1)
    clip = _clip(D, rank, n, segments)
    fine = refine(segments)
    assert len(fine) > len(segments) and sum(fine) == sum(segments)
    nll, loss, pred, rec, rho, pur = run_scored(m, segments, clip, n)
    assert all(np.all(np.isfinite(x)) for x in (nll, loss, pred, rho, pur)) and rec.any() and nll.any()
    for kw in ({}, {"same_state": True}, {"repeat_params": True}, {"null_final": True}):
        n2, l2, p2, r2, rho2, pur2 = run_scored(m, fine, clip, n, **kw)
        assert np.array_equal(n2, nll) and np.array_equal(l2, loss) and np.array_equal(p2, pred), kw
        assert (r2 is None) if kw.get("null_final") else np.array_equal(r2, rec), kw
        assert np.array_equal(rho2, rho) and np.array_equal(pur2, pur), kw
    n3, l3, p3, r3, _, _ = run_scored(m, fine, clip, n, save=False)                      # (the other SAVE instance: the same bits)
    assert np.array_equal(n3, nll) and np.array_equal(l3, loss) and np.array_equal(p3, pred) and np.array_equal(r3, rec)
    one = np.ascontiguousarray(clip[n - 1:n])
    a = run_scored(m, fine, one, n)                                                      # n_audio = 1
    b = run_scored(m, segments, np.tile(one, (n, 1)), n)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(a[0][0], a[0][j]) for j in range(n))                       # one signal: every path scores it alike


@pytest.mark.parametrize("D,rank,variant,rank1,n,segments", CASES)
def test_scoring_perturbs_nothing(D, rank, variant, rank1, n, segments):
    """(b) pred, the final record and the saved rho / purity of the scored run are cmps_rho_stream's on the same followed segments, bit for
    bit, in every case (measured on an MI355X: identical in all seven cases)."""
    m = _model(D, rank, variant, rank1)
    clip = _clip(D, rank, n, segments)
    _, _, pred, rec, rho, pur = run_scored(m, segments, clip, n)
    _, pred_f, rec_f, rho_f, pur_f = run_followed(m, tuple((f, 0) for f in segments), clip, None, n)
    assert np.array_equal(pred, pred_f) and np.array_equal(rec, rec_f)
    assert np.array_equal(rho, rho_f) and np.array_equal(pur, pur_f)


@pytest.mark.parametrize("D,rank,variant,rank1,n,segments", CASES)
def test_scores_match_oracle_composition(D, rank, variant, rank1, n, segments):
    """(c) nll against the float64 composition in units of the float32 composition's own distance from it plus the split arithmetics'
    product-error floor, loss against the float32 total, and loss against cmps_rho_loss_fwd on the same clips.

    Measured on an MI355X (cases in the order of CASES; rank1 2 = BF16X3, variant 1 = BLOCK; total err and vs fwd relative to max(|l|, 1),
    bars 1e-05 and 2e-05):
      D   rank variant rank1 n  steps  max|nll|   |hip - f64|  |o32 - f64|  ratio  nll bar    total err  vs fwd
      7   7    0       -     1  4      7.121e-02  4.929e-08    4.556e-08    1.08   9.710e-07  1.490e-08  0.000e+00
      20  9    0       -     3  130    3.643e-01  6.299e-07    6.952e-07    0.91   4.436e-06  3.283e-07  1.114e-07
      32  32   0       -     5  193    3.449e-01  1.472e-06    1.427e-06    1.03   8.329e-06  3.841e-07  7.722e-08
      32  4    0       2     2  106    2.918e-01  4.255e-07    5.410e-07    0.79   4.784e-06  6.435e-08  6.509e-08
      32  32   1       -     3  70     3.410e-01  5.455e-07    6.250e-07    0.87   5.113e-06  9.320e-08  1.864e-07
      40  3    0       -     2  74     4.501e-01  2.638e-06    2.460e-06    1.07   1.316e-05  1.974e-07  0.000e+00
      96  96   0       -     2  10     5.749e-01  1.049e-07    1.269e-07    0.83   7.706e-06  2.242e-07  1.121e-07"""
    m = _model(D, rank, variant, rank1)
    clip = _clip(D, rank, n, segments)
    nll32, total32 = RC.case_reference(D, rank, n, segments, "f32")[:2]
    nll64, total64 = RC.case_reference(D, rank, n, segments, "f64")[:2]
    nll, loss, _, _, _, _ = run_scored(m, segments, clip, n, save=False)
    d_hip = float(np.max(np.abs(nll.astype(np.float64) - nll64)))
    bar, d_o32 = _nll_bar(D, rank, clip, nll32, nll64, m.A)
    d_tot = float(np.max(np.abs(loss - total32) / np.maximum(np.abs(total32), 1.0)))
    fwd = m.loss_per_clip(clip)
    d_fwd = float(np.max(np.abs(loss - fwd) / np.maximum(np.abs(fwd), 1.0)))
    print(f"rho score D={D} rank={rank} variant={variant} rank1={rank1} n={n} steps={sum(segments)}: max|nll| {float(np.max(np.abs(nll))):.3e}  "
          f"|hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  ratio {d_hip / max(d_o32, 1e-300):.2f}  nll bar {bar:.3e}  total err {d_tot:.3e} "
          f"(bar {LOSS_RTOL:.0e})  |hip - f64| total {float(np.max(np.abs(loss - total64))):.3e}  vs fwd {d_fwd:.3e} (bar {2 * LOSS_RTOL:.0e})")
    assert d_o32 > 0 and float(np.max(np.abs(nll32))) > 1e-3                             # the bars are not vacuous
    assert d_hip <= bar
    assert d_tot <= LOSS_RTOL
    assert d_fwd <= 2 * LOSS_RTOL


@pytest.mark.parametrize("D,rank,variant", [(32, 32, AUTO), (40, 3, AUTO)])
def test_score_generate_score(D, rank, variant):
    """(d) score 40 steps, generate 30, score 50 anchored, against the composition, for the row-array kernel and the block kernel: out at
    the rho stream tests' bar, nll and the total as in (c); the generated run leaves the total alone.
    Measured on an MI355X: D = rank = 32 (row-array kernel) out err 1.490e-08, nll |hip - f64| 2.392e-06 (|o32 - f64| 2.590e-06, bar
    1.298e-05), total err 3.815e-06 absolute; D = 40, rank 3 (block kernel) out err 7.451e-09, nll 1.763e-06 (1.899e-06, bar 1.092e-05),
    total err 5.722e-06 absolute."""
    n = 3
    m = _model(D, rank, variant)
    be = m._get_backend()
    ohp, ov, Wx, Wy = RR.oracle_side(RR.case_model(D, rank))
    plan = [(RC.SCORE, 40), (RC.SAMPLE, 30), (RC.SCORE, 50, True)]
    clip = RC.case_clip(D, rank, n, RC.clip_columns(plan))
    assert clip.shape == (n, 92)
    noise = O.sample_noise(ohp, n, 30, temp=0.5, seed=D)
    nll32, total32, pred32, out32 = RC.rho_score_reference(ohp, ov, Wx, Wy, plan, clip, noise, "f32")[:4]
    nll64, _, pred64 = RC.rho_score_reference(ohp, ov, Wx, Wy, plan, clip, noise, "f64")[:3]
    be.set_params(m.effective_params(), n, 121, train=False)
    be.rho_set_state(m.columns(), n, 121, train=False)
    st = be.rho_stream_state(n)
    a, loss_a, pa = be.rho_stream_score(None, st, 0, clip[:, :41], want_pred=True, n=n)
    out, none = be.rho_stream(st, st, 40, None, noise, False, n=n)
    b, loss_b, pb = be.rho_stream_score(st, st, 70, clip[:, 41:], want_pred=True, n=n, loss=loss_a)
    nll, pred = np.concatenate([a, b], axis=1), np.concatenate([pa, pb], axis=1)
    seq = loss_a.copy()
    for j in range(50):
        seq = (seq + b[:, j]).astype(np.float32)
    assert none is None and np.array_equal(seq, loss_b)                                  # continued from loss_a: nothing added in between
    d_hip = float(np.max(np.abs(nll - nll64)))
    bar, d_o32 = _nll_bar(D, rank, clip, nll32, nll64, m.A)
    err = float(np.max(np.abs(out - out32)))
    print(f"rho mixed D={D} rank={rank}: out err {err:.3e}  nll |hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  nll bar {bar:.3e}  total err "
          f"{float(np.max(np.abs(loss_b - total32))):.3e}")
    assert err <= OUT_RTOL * float(np.max(np.abs(out32)))
    assert d_hip <= bar
    assert float(np.max(np.abs(loss_b - total32) / np.maximum(np.abs(total32), 1.0))) <= LOSS_RTOL
    assert float(np.max(np.abs(pred - pred64))) <= (4.0 * float(np.max(np.abs(pred32 - pred64)))
                                                    + 8.0 * 2.0 ** -22 * RR.R_fro(D, rank) * float(m.hparams.delta_t))
    # the same run with the scored segments followed: the waveform keeps its bits
    st2 = be.rho_stream_state(n)
    be.rho_stream(None, st2, 0, clip[:, :41], None, True, n=n)
    out2, _ = be.rho_stream(st2, st2, 40, None, noise, False, n=n)
    assert np.array_equal(out2, out)


def test_rho_score_error_returns():
    """(e) every error return of the contract; none of them launches anything (the kernel-event record stays empty)."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, rank, n, forced, k0 = 8, 3, 3, 4, 6
    T = k0 + forced + 1
    m = _model(D, rank)
    be = m._get_backend()
    lib, h, dev = be._lib, be._h, be.device
    audio = torch.zeros((n, forced + 1), dtype=torch.float32, device=dev)
    nll = torch.empty((n, forced), dtype=torch.float32, device=dev)
    pred = torch.empty((n, forced), dtype=torch.float32, device=dev)
    loss = torch.zeros(n, dtype=torch.float32, device=dev)
    OK, BAD, STATE, WS = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE, _capi.CMPS_ERR_WORKSPACE
    be.set_params(m.effective_params(), n, T - 1, train=False)                          # one row short
    be.rho_set_state(m.columns(), n, T - 1, train=False)
    st = be.rho_stream_state(n)

    def call(sin=st.data_ptr(), sout=st.data_ptr(), k0_=k0, audio_p=audio.data_ptr(), n_audio=n, forced_=forced, n_=n, nll_p=nll.data_ptr(),
             loss_p=loss.data_ptr(), pred_p=pred.data_ptr(), save=0, b=be):
        return b._lib.cmps_rho_stream_score(b._h, sin, sout, k0_, audio_p, n_audio, forced_, n_, nll_p, loss_p, pred_p, save, b._stream())

    fresh = HipScan(D)
    assert call(b=fresh) == STATE                                                       # before cmps_set_params
    fresh.set_params(m.effective_params(), n, T, train=False)
    assert call(b=fresh) == STATE and "cmps_rho_set_state" in fresh._lib.cmps_last_error(fresh._h).decode()
    assert call() == BAD
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {T}" in msg and "cmps_rho_stream_score" in msg, msg
    be.set_params(m.effective_params(), n, T, train=False)                              # exactly enough rows
    be.rho_set_state(m.columns(), n, T, train=False)
    assert call(sin=None, k0_=0) == OK                                                  # (a start, so that the record read below is a state)
    assert call() == OK
    assert call(sout=None) == OK and call(n_audio=1) == OK and call(nll_p=None) == OK and call(pred_p=None) == OK
    torch.cuda.synchronize()
    be.kernel_events(True)
    be.kernel_times()
    assert call(sin=None) == BAD and call(k0_=0) == BAD                                 # state_in == NULL <=> k0 == 0
    assert call(n_=0, n_audio=0) == BAD
    assert call(forced_=0) == BAD and call(forced_=-1) == BAD and call(k0_=-1) == BAD   # a scored segment makes one step at least
    assert call(audio_p=None) == BAD
    assert call(loss_p=None) == BAD and "loss_dev" in lib.cmps_last_error(h).decode()
    assert call(n_audio=2) == BAD
    assert call(k0_=k0 + 1) == BAD and "T >=" in lib.cmps_last_error(h).decode()
    assert lib.cmps_rho_stream_score(None, None, None, 0, audio.data_ptr(), n, forced, n, None, loss.data_ptr(), None, 0, None) == BAD
    # save_states: a forward-only rho workspace has no rows; a TRAIN one with one row too few
    assert call(save=1) == WS
    be.rho_set_state(m.columns(), n, forced, train=True)
    assert call(save=1) == WS
    assert be.kernel_times() == {}                                                      # no refused call launched anything
    be.kernel_events(False)
    be.rho_set_state(m.columns(), n, forced + 1, train=True)
    assert call(save=1) == OK
    pur = be.rho_states(n, forced, want_rho=False, want_purity=True)
    assert pur.shape == (n, forced) and np.all(np.isfinite(pur))
    torch.cuda.synchronize()
    # columns in the workspace (rank * D above the LDS limit): n must not exceed B_max
    m96 = _model(96, 96)
    b96 = m96._get_backend()
    b96.set_params(m96.effective_params(), 2, T, train=False)
    b96.rho_set_state(m96.columns(), 2, T, train=False)
    assert call(b=b96, sin=None, sout=None, k0_=0) == WS                                # n = 3 > B_max = 2
    assert call(b=b96, sin=None, sout=None, k0_=0, n_=2, n_audio=2) == OK
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
    Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    be.legacy_set_params(R, Q, 1e-3, n, T, train=False)
    assert call() == STATE
    assert "legacy" in lib.cmps_last_error(h).decode()


@pytest.mark.parametrize("D,rank,variant,name", [(8, 3, AUTO, "k_sample_rho_mfma_score"), (32, 32, AUTO, "k_sample_rho_mfma_score"),
                                                 (32, 5, BLOCK, "k_sample_rho_score"), (40, 3, AUTO, "k_sample_rho_score")])
def test_rho_score_kernel_names(D, rank, variant, name):
    """(f) the launch is recorded under the kernel the variant resolves to."""
    n = 2
    m = _model(D, rank, variant)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, 8, train=False)
    be.rho_set_state(m.columns(), n, 8, train=False)
    be.kernel_events(True)
    st = be.rho_stream_state(n)
    _, loss, _ = be.rho_stream_score(None, st, 0, np.zeros((1, 3), np.float32), n=n)
    be.rho_stream_score(st, st, 2, np.zeros((n, 4), np.float32), want_nll=False, n=n, loss=loss)
    times = be.kernel_times()
    assert list(times) == [name] and times[name][1] == 2


@pytest.mark.parametrize("D,rank,variant", [(32, 4, AUTO), (40, 3, AUTO)])
def test_rho_score_memory_contract(D, rank, variant):
    """(g) red zones round nll, loss, pred, the audio, both records and the (pattern-filled) workspaces under both fill patterns (loss_dev
    holds the NaN pattern at k0 = 0: it is not read there); nll_dev == NULL and pred_dev == NULL segments; every documented output fully
    written; the carried floats of a record and nothing behind them; the same bits as HipScan."""
    from test_gpu_memory_contract import both_fills, as_f32, rho_carried
    from audio_mps_amd.scan import HipScan
    n, segments = 2, (65, 1, 40)
    F = sum(segments)
    clip = RC.case_clip(D, rank, n, F + 1)
    m = RR.case_model(D, rank, backend=False)
    carried = rho_carried(D, rank, variant)
    recs = {}

    def run(fill):
        drv = G.Driver(D, fill, variant)
        G.set_params(drv, m, n, F + 1, train=False)
        G.rho_set_state(drv, m, n, max(segments) + 1, train=True)
        nbytes = int(drv.lib.cmps_rho_stream_state_bytes(drv.h, n))
        assert nbytes > 0 and nbytes % 16 == 0
        states = [drv.new("state_a", nbytes), drv.new("state_b", nbytes)]
        loss = drv.new("loss", 4 * n, out=torch.float32)
        names, f0 = ["loss"], 0
        for idx, f in enumerate(segments):
            a = drv.load(f"audio_{idx}", np.ascontiguousarray(clip[:, f0:f0 + f + 1], dtype=np.float32))
            nll = drv.new(f"nll_{idx}", 4 * n * f, out=torch.float32) if idx != 1 else None
            pred = drv.new(f"pred_{idx}", 4 * n * f, out=torch.float32) if idx != 2 else None
            names += [f"nll_{idx}"] * (nll is not None) + [f"pred_{idx}"] * (pred is not None)
            drv.call("cmps_rho_stream_score", states[(idx + 1) % 2] if idx else None, states[idx % 2], f0, a, n, f, n, nll, loss, pred,
                     idx % 2)                                                            # (save_states in the middle segment)
            if idx % 2:
                names += G.rho_states(drv, n, f, f"_{idx}")
            f0 += f
        drv.finish()
        recs[fill] = [(s.numpy(np.float32).reshape(n, -1), s.untouched_mask(torch.float32).cpu().numpy().reshape(n, -1)) for s in states]
        return drv.result(names)
    res = both_fills(run, f"cmps_rho_stream_score ({D}, {rank})")
    for (ra, left), (rb, _) in zip(recs[G.NAN_FILL], recs[G.ZERO_FILL]):
        assert not left[:, :carried].any() and left[:, carried:].all()                   # the carried floats, and nothing behind them
        assert np.array_equal(ra[:, :carried].view(np.uint32), rb[:, :carried].view(np.uint32))
    nll_h, loss_h, pred_h, rec_h, _, _ = run_scored(RR.case_model(D, rank, backend=HipScan(D, variant=variant)), segments, clip, n, save=False)
    assert np.array_equal(as_f32(res, "loss"), loss_h)
    assert np.array_equal(as_f32(res, "nll_0", (n, 65)), nll_h[:, :65]) and np.array_equal(as_f32(res, "nll_2", (n, 40)), nll_h[:, 66:])
    assert np.array_equal(as_f32(res, "pred_0", (n, 65)), pred_h[:, :65]) and np.array_equal(as_f32(res, "pred_1", (n, 1)), pred_h[:, 65:66])
    final = recs[G.NAN_FILL][0][0]                                                       # segment 2 wrote state_a
    assert np.array_equal(final[:, :carried].view(np.uint32), rec_h.view(np.float32).reshape(n, -1)[:, :carried].view(np.uint32))


def test_sample_stream_score_matches_loss_per_clip():
    """(h) SampleStream.score / total_nll, states() / purity() behind a score call, and nll_per_step(segment=...) against loss_per_clip
    (another kernel: the bar of (c))."""
    D, rank, n, T = 8, 3, 3, 200
    m = _model(D, rank)
    clip = RC.case_clip(D, rank, n, T)
    want = m.loss_per_clip(clip)
    st = m.open_stream(n, T - 1)
    parts = [st.score(clip[:, :10]), st.score(clip[:, 10:11]), st.score(clip[:, 11:])]
    nll = np.concatenate(parts, axis=1)
    assert nll.shape == (n, T - 1) and nll.dtype == np.float32 and st.position == T - 1 and st.last_pred.shape == (n, T - 11)
    assert float(np.max(np.abs(st.total_nll - want) / np.maximum(np.abs(want), 1.0))) <= 2 * LOSS_RTOL
    with pytest.raises(ValueError):
        st.score(clip[:, :1])                                                            # one step past max_steps
    whole, cut = m.nll_per_step(clip), m.nll_per_step(clip, segment=64)
    assert np.array_equal(whole, nll) and np.array_equal(cut, nll)                       # (tables of the same T: the same bits)
    rows = whole.astype(np.float64).sum(axis=1)
    assert float(np.max(np.abs(rows - want) / np.maximum(np.abs(want), 1.0))) <= 2 * LOSS_RTOL
    # keep_states: rho and the purity behind a score call are those behind a follow call
    ks, kf = m.open_stream(n, T - 1, keep_states=64), None
    ks.score(clip[:, :41])
    rho_s, pur_s = ks.states(), ks.purity()
    kf = m.open_stream(n, T - 1, keep_states=64)
    kf.follow(clip[:, :41])
    assert rho_s.shape == (n, 40, D, D) and np.array_equal(rho_s, kf.states()) and np.array_equal(pur_s, kf.purity())
    # unscored steps leave the total alone, scored ones behind them continue it
    st = m.open_stream(n, 300, seed=1)
    st.score(clip[:, :120])
    t = st.total_nll.copy()
    st.generate(5)
    st.follow(clip[:, :4], anchor=True)
    assert np.array_equal(st.total_nll, t) and st.position == 119 + 5 + 3
    more = st.score(clip[:, 4:40])
    seq = t.copy()
    for j in range(36):
        seq = (seq + more[:, j]).astype(np.float32)
    assert more.shape == (n, 36) and np.array_equal(st.total_nll, seq) and not np.array_equal(seq, t)


def test_sample_main_score_on_a_rho_checkpoint(tmp_path, capsys):
    """(h) python -m audio_mps_amd.sample --score on the rho_mps checkpoint recipe of tests/test_gpu_rho_stream.py, whole and in segments."""
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd import sample as S
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    from _util import make_audio
    D, rank = 8, 3
    hp = HParams(minibatch_size=4, bond_dim=D, initial_rank=rank)
    m = RhoCMPS(hp, data_iterator=make_audio(4, 128, hp.delta_t, 5), seed=0, backend=HipScan(D))
    tr = Trainer(m, hp, device_step=True)
    tr.step()
    tr.step()
    ckdir = os.path.join(tmp_path, "model")
    tr.save(os.path.join(ckdir, S.CKPT_NAME))
    clip = 0.5 * O.damped_sine(1, 300, hp.delta_t, seed=2)[0]
    wav = os.path.join(tmp_path, "clip.wav")
    S.write_wav(wav, clip, 16000)
    one = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", os.path.join(tmp_path, "one")])
    assert "total nll" in capsys.readouterr().out
    out_dir = os.path.join(tmp_path, "seg")
    seg = S.main(["--modeldir", ckdir, "--score", wav, "--out_dir", out_dir, "--segment", "64"])
    assert one.shape == (1, 299) and np.all(np.isfinite(one)) and np.array_equal(seg, one)
    assert sorted(os.listdir(out_dir)) == ["nll.npy", "pred.npy"]
    assert np.array_equal(np.load(os.path.join(out_dir, "nll.npy")), one) and np.load(os.path.join(out_dir, "pred.npy")).shape == (1, 299)
