"""The resumable RhoCMPS sampler on a real MI355X: cmps_rho_stream in the row-array GEMM kernel (k_sample_rho_mfma, both arithmetics) and
the block kernel (k_sample_rho, both column homes).  (a) cutting a run into more segments changes no bit of out, pred, the state record or
the saved rho / purity; (b) the run against the oracle composition for a plan (tests/_rho_stream_ref.py); (c) one call against
cmps_rho_sample_primed and cmps_rho_sample; (d) the error returns; (e) the kernel names; (f) the host layer (open_stream with and without
keep_states, fill_gaps, python -m audio_mps_amd.sample --segment on a rho_mps checkpoint).

Bars (those of tests/test_gpu_rho_primed.py, stated there):
  * out:  |hip - composition_f32| <= 2e-4 * max |composition_f32|
  * pred: max |hip - composition_f64| <= 4 * max |composition_f32 - composition_f64| + 8 * 2^-22 * |R|_F * delta_t
  * states: rel_inf(rho) <= 2e-4, purity rtol 2e-4 / atol 1e-6, purity in [1/D - 1e-4, 1 + 1e-4]
"""
import os

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O
from _util import rel_inf
import _rho_primed_ref as RR
import _rho_stream_ref as RS
from test_gpu_rho_primed import AUTO, BLOCK, OUT_RTOL, _model

pytestmark = pytest.mark.gpu

CASES = RS.GPU_CASES


def _pred_bar(D, rank, p32, p64, delta_t):
    return 4.0 * float(np.max(np.abs(p32.astype(np.float64) - p64))) + 8.0 * 2.0 ** -22 * RR.R_fro(D, rank) * float(delta_t)


def run_plan(m, plan, clip, noise, n, same_state=False, null_final=False, repeat_params=False):
    """The plan call by call through HipScan.rho_stream with save_states, segment s on clip[:, f0 : f0 + forced + 1] and
    noise[l0 : l0 + sampled]: (out [n, L], pred [n, F], the final state record as bytes, or None with null_final, rho [n, F + L, D, D] and
    purity [n, F + L] gathered call by call).  The tables have F + L + 1 rows, the rho workspace rows for the plan's longest call only.  The
    state alternates between two tensors, or (same_state) is read and written in place; repeat_params calls set_params and rho_set_state
    again, with the same arguments, behind the first segment."""
    be = m._get_backend()
    F, L = RS.plan_steps(plan)
    longest = max(f + s for f, s in plan)

    def prepare():
        be.set_params(m.effective_params(), n, F + L + 1, train=False)
        be.rho_set_state(m.columns(), n, longest + 1, train=True)

    prepare()
    states = [be.rho_stream_state(n), be.rho_stream_state(n)]
    outs, preds, rhos, purs, cur, k0, f0, l0 = [], [], [], [], None, 0, 0, 0
    for idx, (f, s) in enumerate(plan):
        if idx == len(plan) - 1 and null_final:
            nxt = None
        elif same_state:
            nxt = states[0]
        else:
            nxt = states[1] if cur is states[0] else states[0]
        out, pred = be.rho_stream(cur, nxt, k0, clip[:, f0:f0 + f + 1] if f else None, noise[l0:l0 + s] if s else None, True, n=n,
                                  save_states=True)
        assert out.shape == (n, s) and pred.shape == (n, f)
        r, p = be.rho_states(n, f + s, want_rho=True, want_purity=True)
        outs.append(out)
        preds.append(pred)
        rhos.append(r)
        purs.append(p)
        cur, k0, f0, l0 = nxt, k0 + f + s, f0 + f, l0 + s
        if repeat_params and idx == 0:
            prepare()
    return (np.concatenate(outs, axis=1), np.concatenate(preds, axis=1), (None if cur is None else cur.cpu().numpy()),
            np.concatenate(rhos, axis=1), np.concatenate(purs, axis=1))


@pytest.mark.parametrize("D,rank,variant,rank1,n,plan", CASES)
def test_refinement_is_bit_exact(D, rank, variant, rank1, n, plan):
    """(a) the plan as written against the plan with every call cut again (middle of the forced part, the hand-over, one step into the
    sampled part): out, pred, the final record and the saved rho and purity (of every call, the plan's last one among them, against the
    same steps gathered from the refined run); the same with the state updated in place, a NULL final state_out, set_params +
    rho_set_state repeated between two segments, and one shared signal against its tiled copy."""
    m = _model(D, rank, variant, rank1)
    clip, noise = RS.case_inputs(D, rank, plan, n)
    fine = tuple(RS.refine(plan))
    assert len(fine) > len(plan)
    out, pred, rec, rho, pur = run_plan(m, plan, clip, noise, n)
    assert all(np.all(np.isfinite(x)) for x in (out, pred, rho, pur)) and rec.any()
    last = sum(plan[-1])
    for kw in ({}, {"same_state": True}, {"repeat_params": True}, {"null_final": True}):
        o2, p2, r2, rho2, pur2 = run_plan(m, fine, clip, noise, n, **kw)
        assert np.array_equal(o2, out) and np.array_equal(p2, pred), kw
        assert (r2 is None) if kw.get("null_final") else np.array_equal(r2, rec), kw
        assert np.array_equal(rho2[:, -last:], rho[:, -last:]) and np.array_equal(pur2[:, -last:], pur[:, -last:]), kw
        assert np.array_equal(rho2, rho) and np.array_equal(pur2, pur), kw
    one = np.ascontiguousarray(clip[n - 1:n])
    s_ = run_plan(m, fine, one, noise, n)                                              # n_audio = 1
    t_ = run_plan(m, plan, np.tile(one, (n, 1)), noise, n)
    assert all(np.array_equal(a, b) for a, b in zip(s_, t_))
    if n > 1 and out.shape[1]:
        assert not np.array_equal(s_[0][0], s_[0][1])                                   # one signal, a noise row per path


@pytest.mark.parametrize("D,rank,variant,rank1,n,plan", CASES)
def test_plan_matches_oracle_composition(D, rank, variant, rank1, n, plan):
    """(b) out against the float32 composition, pred against the float64 one in units of the float32 composition's own distance from it
    plus the split arithmetics' product-error floor, rho and purity of every call against the float32 composition.

    Measured on an MI355X (cases in the order of CASES; rank1 2 = BF16X3, variant 1 = BLOCK):
      D   rank variant rank1 n  steps  out err    out bar    |hip - f64|  |o32 - f64|  ratio  pred bar   rho        purity
      7   7    0       -     1  4      8.731e-11  3.031e-07  3.768e-13    8.562e-12    0.04   1.731e-09  5.823e-07  2.300e-07
      20  9    0       -     3  235    9.267e-08  8.856e-06  8.882e-09    9.410e-09    0.94   4.197e-08  3.187e-06  1.276e-06
      32  32   0       -     5  258    1.378e-07  1.008e-05  1.576e-08    1.576e-08    1.00   7.032e-08  5.872e-06  1.905e-06
      32  4    0       2     2  170    2.980e-08  7.121e-06  6.737e-09    6.941e-09    0.97   3.503e-08  4.458e-06  2.295e-06
      32  32   1       -     3  110    3.912e-08  8.844e-06  5.610e-10    7.049e-10    0.80   1.009e-08  5.939e-06  1.111e-06
      40  3    0       -     2  75     2.794e-08  7.016e-06  9.452e-10    9.108e-10    1.04   1.312e-08  3.267e-06  1.019e-06
      96  96   0       -     2  12     2.794e-09  4.382e-06  1.055e-10    3.746e-10    0.28   2.296e-08  2.159e-06  3.936e-07"""
    m = _model(D, rank, variant, rank1)
    clip, noise = RS.case_inputs(D, rank, plan, n)
    o32, p32, r32, u32 = RS.case_reference(D, rank, plan, n, "f32")
    p64 = RS.case_reference(D, rank, plan, n, "f64")[1]
    out, pred, _, rho, pur = run_plan(m, plan, clip, noise, n)
    err, bar = float(np.max(np.abs(out - o32))), OUT_RTOL * float(np.max(np.abs(o32)))
    d_hip = float(np.max(np.abs(pred.astype(np.float64) - p64)))
    d_o32 = float(np.max(np.abs(p32.astype(np.float64) - p64)))
    pbar = _pred_bar(D, rank, p32, p64, m.hparams.delta_t)
    print(f"rho stream D={D} rank={rank} variant={variant} rank1={rank1} n={n} steps={sum(RS.plan_steps(plan))}: out err {err:.3e} bar {bar:.3e}  "
          f"|hip - f64| {d_hip:.3e}  |o32 - f64| {d_o32:.3e}  ratio {d_hip / max(d_o32, 1e-300):.2f}  pred bar {pbar:.3e}  "
          f"rho {rel_inf(rho, r32):.3e}  purity {np.max(np.abs(pur - u32) / u32):.3e}")
    assert err <= bar
    assert d_hip <= pbar
    assert rel_inf(rho, r32) <= 2e-4
    np.testing.assert_allclose(pur, u32, rtol=2e-4, atol=1e-6)
    assert np.all(pur <= 1 + 1e-4) and np.all(pur >= 1.0 / D - 1e-4)


@pytest.mark.parametrize("D,rank,P,length,n,variant", [(32, 32, 64, 130, 5, AUTO), (40, 3, 33, 40, 2, AUTO)])
def test_one_call_against_the_existing_entries(D, rank, P, length, n, variant):
    """(c) one stream call with k0 = 0 and a primed run's arguments against cmps_rho_sample_primed, and a sampled-only call against
    cmps_rho_sample, for the row-array kernel (D = 32) and the block kernel (D = 40): asserted are the bars of (b), printed is whether
    the bits agree.
    Measured on an MI355X: both kernels bit-identical to cmps_rho_sample_primed in out and pred, and to cmps_rho_sample in out."""
    m = _model(D, rank, variant)
    be = m._get_backend()
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    o32, p32, _, _ = RR.case_reference(D, rank, P, length, n, "f32")
    p64 = RR.case_reference(D, rank, P, length, n, "f64")[1]
    be.set_params(m.effective_params(), n, P + length + 1, train=False)
    be.rho_set_state(m.columns(), n, P + length + 1, train=False)
    out_p, pred_p = be.rho_sample_primed(prime, noise, want_pred=True)
    out_s, pred_s = be.rho_stream(None, None, 0, prime, noise, True, n=n)
    bar = OUT_RTOL * float(np.max(np.abs(o32)))
    pbar = _pred_bar(D, rank, p32, p64, m.hparams.delta_t)
    d_out, d_pred = float(np.max(np.abs(out_s - out_p))), float(np.max(np.abs(pred_s - pred_p)))
    print(f"rho stream vs primed D={D} rank={rank}: out {'bit-identical' if np.array_equal(out_s, out_p) else f'max diff {d_out:.3e}'}, "
          f"pred {'bit-identical' if np.array_equal(pred_s, pred_p) else f'max diff {d_pred:.3e}'}")
    assert float(np.max(np.abs(out_s - o32))) <= bar and d_out <= bar
    assert float(np.max(np.abs(pred_s - p64))) <= pbar and d_pred <= pbar
    w = be.rho_sample(noise)
    w_s, none = be.rho_stream(None, None, 0, None, noise, False, n=n)
    d_w = float(np.max(np.abs(w_s - w)))
    print(f"rho stream vs sample D={D} rank={rank}: out {'bit-identical' if np.array_equal(w_s, w) else f'max diff {d_w:.3e}'}")
    assert none is None and d_w <= OUT_RTOL * float(np.max(np.abs(w)))


def test_rho_stream_error_returns():
    """(d) every error return of the contract."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import HipScan
    D, rank, n, forced, length, k0 = 8, 3, 3, 4, 5, 6
    T = k0 + forced + length + 1
    m = _model(D, rank)
    be = m._get_backend()
    lib, h, dev = be._lib, be._h, be.device
    audio = torch.zeros((n, forced + 1), dtype=torch.float32, device=dev)
    noise = torch.zeros((n, length), dtype=torch.float32, device=dev)
    out = torch.empty((n, length), dtype=torch.float32, device=dev)
    pred = torch.empty((n, forced), dtype=torch.float32, device=dev)
    OK, BAD, STATE, WS = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE, _capi.CMPS_ERR_WORKSPACE
    be.set_params(m.effective_params(), n, T - 1, train=False)                          # one row short
    be.rho_set_state(m.columns(), n, T - 1, train=False)
    st = be.rho_stream_state(n)
    one = lib.cmps_rho_stream_state_bytes(h, 1)
    assert one > 0 and one % 16 == 0 and one >= 64 * rank * 4 and st.numel() == n * one     # the row-array kernel's rows
    assert lib.cmps_rho_stream_state_bytes(h, 0) == 0 and lib.cmps_rho_stream_state_bytes(h, -1) == 0

    def call(sin=st.data_ptr(), sout=st.data_ptr(), k0_=k0, audio_p=audio.data_ptr(), n_audio=n, forced_=forced, noise_p=noise.data_ptr(),
             length_=length, n_=n, out_p=out.data_ptr(), save=0, b=be):
        return b._lib.cmps_rho_stream(b._h, sin, sout, k0_, audio_p, n_audio, forced_, noise_p, length_, n_, out_p, pred.data_ptr(), save,
                                      b._stream())

    fresh = HipScan(D)
    assert call(b=fresh) == STATE                                                       # before cmps_set_params
    fresh.set_params(m.effective_params(), n, T, train=False)
    assert call(b=fresh) == STATE and fresh._lib.cmps_rho_stream_state_bytes(fresh._h, n) == 0   # before cmps_rho_set_state
    assert call() == BAD
    msg = lib.cmps_last_error(h).decode()
    assert f"T >= {T}" in msg, msg
    be.set_params(m.effective_params(), n, T, train=False)                              # exactly enough rows
    be.rho_set_state(m.columns(), n, T, train=False)
    assert call(sin=None, sout=st.data_ptr(), k0_=0, forced_=forced, length_=2) == OK   # (a start, so that the record read below is a state)
    assert call() == OK
    assert call(sout=None) == OK and call(n_audio=1) == OK
    assert call(forced_=0, audio_p=None) == OK and call(length_=0, noise_p=None, out_p=None) == OK
    torch.cuda.synchronize()
    assert call(sin=None) == BAD and call(k0_=0) == BAD                                 # state_in == NULL <=> k0 == 0
    assert call(sin=None, k0_=0) == OK
    assert call(n_=0, n_audio=0) == BAD
    assert call(forced_=-1) == BAD and call(length_=-1) == BAD and call(k0_=-1) == BAD
    assert call(forced_=0, length_=0) == BAD
    assert call(audio_p=None) == BAD                                                    # forced > 0
    assert call(noise_p=None) == BAD and call(out_p=None) == BAD                        # length > 0
    assert call(n_audio=2) == BAD
    assert call(k0_=k0 + 1) == BAD and "T >=" in lib.cmps_last_error(h).decode()
    assert lib.cmps_rho_stream(None, None, None, 0, audio.data_ptr(), n, forced, noise.data_ptr(), length, n, out.data_ptr(), None, 0,
                               None) == BAD
    # save_states: a forward-only rho workspace has no rows; a TRAIN one with one row too few; the rho workspace's T is a capacity only
    assert call(save=1) == WS
    be.rho_set_state(m.columns(), n, forced + length, train=True)
    assert call(save=1) == WS
    be.rho_set_state(m.columns(), n, forced + length + 1, train=True)
    assert call(save=1) == OK
    pur = be.rho_states(n, forced + length, want_rho=False, want_purity=True)
    assert pur.shape == (n, forced + length) and np.all(np.isfinite(pur))
    with pytest.raises(_capi.CmpsError):
        be.rho_states(n, length, want_rho=False, want_purity=True)
    torch.cuda.synchronize()
    # the record belongs to the kernel: the block kernel's holds the columns
    blk = _model(D, rank, BLOCK)._get_backend()
    blk.set_params(m.effective_params(), n, T, train=False)
    blk.rho_set_state(m.columns(), n, T, train=False)
    b1 = blk._lib.cmps_rho_stream_state_bytes(blk._h, 1)
    assert b1 % 16 == 0 and b1 >= (2 * rank * D + 1) * 4 and b1 != one
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


@pytest.mark.parametrize("D,rank,variant,name", [(8, 3, AUTO, "k_sample_rho_mfma_stream"), (32, 32, AUTO, "k_sample_rho_mfma_stream"),
                                                 (32, 5, BLOCK, "k_sample_rho_stream"), (40, 3, AUTO, "k_sample_rho_stream")])
def test_rho_stream_kernel_names(D, rank, variant, name):
    """(e) the launch is recorded under the kernel the variant resolves to."""
    n = 2
    m = _model(D, rank, variant)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, 8, train=False)
    be.rho_set_state(m.columns(), n, 8, train=False)
    be.kernel_events(True)
    st = be.rho_stream_state(n)
    be.rho_stream(None, st, 0, np.zeros((1, 3), np.float32), np.zeros((2, n), np.float32), True, n=n)
    be.rho_stream(st, st, 4, None, np.zeros((3, n), np.float32), False, n=n)
    times = be.kernel_times()
    assert list(times) == [name] and times[name][1] == 2


def test_open_stream_follow_generate_matches_continue_clip():
    """(f) open_stream -> follow -> generate against continue_clip (another T of the tables: the bar, not the bits)."""
    D, rank, P, length, n = 20, 9, 63, 70, 3
    m = _model(D, rank)
    prime, noise = RR.case_inputs(D, rank, P, length, n)
    ref = RR.case_reference(D, rank, P, length, n, "f32")[0]
    want = m.continue_clip(prime, n, length, noise=noise)
    pred_want = m.predict_increments(prime)
    st = m.open_stream(n, 300)
    pred = np.concatenate([st.follow(prime[:, :10]), st.follow(prime[:, 10:])], axis=1)
    got = np.concatenate([st.generate(1, noise=noise[:1]), st.generate(length - 1, noise=noise[1:])], axis=1)
    assert st.position == P + length and got.dtype == np.float32 and got.shape == (n, length)
    assert float(np.max(np.abs(got - want))) <= OUT_RTOL * float(np.max(np.abs(ref))) / float(m.A)
    p64 = RR.case_reference(D, rank, P, length, n, "f64")[1]
    assert float(np.max(np.abs(pred - pred_want))) <= 2.0 * _pred_bar(D, rank, RR.case_reference(D, rank, P, length, n, "f32")[1], p64,
                                                                      m.hparams.delta_t)      # (each within the bar of the composition)
    with pytest.raises(ValueError):
        st.generate(300 - P - length + 1)
    for f in (st.states, st.purity):
        with pytest.raises(ValueError):
            f()


def test_keep_states_purity_of_a_long_run_in_segments():
    """(f) open_stream(keep_states=64): the purity (and rho) of a 200-step run collected in segments against one purity(prime=...) call,
    whose stash holds all 200 steps.  Measured on an MI355X: purity and rho agree in every bit (the tables have the same T here)."""
    D, rank, P, length, n = 8, 3, 90, 110, 2
    m = _model(D, rank)
    ohp = RR.oracle_side(m)[0]
    prime = O.damped_sine(n, P + 1, ohp.delta_t, seed=5)
    noise = O.sample_noise(ohp, n, length, temp=0.5, seed=5)
    want = m.purity(n, length, noise=noise, prime=prime)
    rho_want = m.rho_evolve_with_sampling(n, length, noise=noise, prime=prime)
    st = m.open_stream(n, P + length, keep_states=64)
    purs, rhos = [], []
    for a, b in ((0, 65), (65, P + 1)):                                                 # 64 and 26 forced steps
        st.follow(prime[:, a:b])
        purs.append(st.purity())
        rhos.append(st.states())
    for a, b in ((0, 64), (64, length)):                                                # 64 and 46 sampled steps
        st.generate(b - a, noise=noise[a:b])
        purs.append(st.purity())
        rhos.append(st.states())
    pur, rho = np.concatenate(purs, axis=1), np.concatenate(rhos, axis=1)
    assert pur.shape == (n, P + length) and rho.shape == (n, P + length, D, D)
    print(f"keep_states purity: max rel diff {np.max(np.abs(pur - want) / want):.3e}, rho rel_inf {rel_inf(rho, rho_want):.3e}")
    np.testing.assert_allclose(pur, want, rtol=2e-4, atol=1e-6)
    assert np.all(pur <= 1 + 1e-4) and np.all(pur >= 1.0 / D - 1e-4)
    assert rel_inf(rho, rho_want) <= 2e-4
    with pytest.raises(ValueError):
        m.open_stream(n, 200, keep_states=64).generate(65)


def test_fill_gaps_on_the_gpu():
    """(f) D = 8, rank 3, T = 200, one gap of 40 samples: the known samples come back unchanged, the gap is finite and differs between
    two paths."""
    D, rank, T, n = 8, 3, 200, 2
    m = _model(D, rank)
    clip = O.damped_sine(1, T, m.hparams.delta_t, seed=3)[0]
    known = np.ones(T, bool)
    known[90:130] = False
    wave = m.open_stream(n, T, temp=0.5, seed=1).fill_gaps(clip, known)
    assert wave.shape == (n, T) and np.array_equal(wave[:, known], np.tile(clip[known], (n, 1)))
    gap = wave[:, 90:130]
    assert np.all(np.isfinite(gap)) and not np.array_equal(gap[0], gap[1])


def test_sample_main_segment_on_a_rho_checkpoint(tmp_path):
    """(f) python -m audio_mps_amd.sample --segment 64 on a checkpoint written by two Trainer steps of a rho_mps model: the clip, then the
    stream's continuation, which is the one-shot command's within the out bar (the same noise; tables of the same T)."""
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
    args = ["--modeldir", ckdir, "--prime", wav, "--sample_duration", "200", "--num_samples", "2", "--seed", "4"]
    one = S.main(args + ["--out_dir", os.path.join(tmp_path, "one")])
    out_dir = os.path.join(tmp_path, "seg")
    seg = S.main(args + ["--out_dir", out_dir, "--segment", "64"])
    assert seg.shape == (2, 500) and np.all(np.isfinite(seg))
    assert sorted(os.listdir(out_dir)) == ["sample_0.wav", "sample_1.wav", "samples.npy"]
    assert np.array_equal(np.load(os.path.join(out_dir, "samples.npy")), seg)
    assert np.array_equal(seg[:, :300], one[:, :300]) and not np.array_equal(seg[0, 300:], seg[1, 300:])
    d = float(np.max(np.abs(seg - one)))
    print(f"sample --segment 64 against one shot: {'bit-identical' if np.array_equal(seg, one) else f'max diff {d:.3e}'}")
    assert d <= OUT_RTOL * float(np.max(np.abs(one[:, 300:] - one[:, 299:300])))
