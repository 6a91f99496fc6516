"""A bank's streams on the GPU (cmps_bank_stream, cmps_bank_stream_score, audio_mps_amd/stream.py::BankStream): member m's slices of out,
pred, nll, the running loss and the state records hold, BIT FOR BIT, what cmps_psi_stream / cmps_psi_stream_score give on a fresh plain
handle set to model m with the same T, fed member m's audio and noise rows -- the sampler kernels are the plain STREAM / SCORE instances
with a member grid dimension.

Every comparison is np.array_equal on raw bytes, and every caller array of every call lies between two red zones (tests/_guard.py), checked
after each call.  That bar rests on the plain path being reproducible, which test_plain_stream_is_reproducible checks first.

One plan per shape: follow 70, generate 50, score 30, generate 65 (215 steps, off the 64-step chunk; tables of T = 216), and the same plan
with every call cut in two at an odd point.  Shapes: D below and at the wave family's width and padded, the block kernel below and above
D = 32, n such that the wave kernel's last workgroup is partial (n = 3, 5 with four waves a workgroup), M > 2.

Against the float64 oracle (tests/_score_ref.py) the bars are the samplers' own: waveform <= 2e-4 max|w|, scored totals <= 1e-5 max(|l|, 1).
"""
import ctypes

import numpy as np
import pytest
import torch

from audio_mps_amd import HParams, PsiCMPS, _capi, layout

import _guard as G
import _score_ref as SC
from _util import make_audio, oracle_hparams, oracle_variables

pytestmark = pytest.mark.gpu

AUTO, BLOCK = _capi.CMPS_VARIANT_AUTO, _capi.CMPS_VARIANT_BLOCK
#         family   D   M  n  variant
SHAPES = [("wave", 3, 3, 3, AUTO),
          ("wave", 16, 2, 5, AUTO),
          ("wave", 17, 4, 3, AUTO),
          ("wave", 32, 3, 2, AUTO),
          ("block", 5, 3, 3, BLOCK),
          ("block", 40, 2, 2, BLOCK)]
IDS = [f"{s[0]}-D{s[1]}" for s in SHAPES]
PLAN = (("F", 70), ("G", 50), ("S", 30), ("G", 65))
CUT = (("F", 33), ("F", 37), ("G", 23), ("G", 27), ("S", 13), ("S", 17), ("G", 31), ("G", 34))
STEPS = sum(s for _, s in PLAN)
T = STEPS + 1
FORCED = sum(s for k, s in PLAN if k != "G")
SAMPLED = STEPS - FORCED
# (rows of the audio, rows of the noise) as multiples: "1" one row, "n", "Mn"
MODES = (("1", "n"), ("n", "Mn"), ("Mn", "n"))
OUT_RTOL, LOSS_RTOL = 2e-4, 1e-5


def member_model(D, n, m):
    """Member m: the model of the stream tests (sigma = 1, A = 10, Rx, Ry x 0.05) with its own seed and its own A."""
    mo = PsiCMPS(HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0 + m), seed=100 + m, backend=False)
    mo.variables["Rx"] *= np.float32(0.05)
    mo.variables["Ry"] *= np.float32(0.05)
    return mo


def param_row(mo):
    p = mo.effective_params()
    return layout.pack(layout.param_fields(mo.bond_d, with_A=True),
                       {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})


_INPUTS = {}


def inputs(shape):
    """(models, params [M, NP], clip [M, n, FORCED + 1], noise [M, n, SAMPLED]) of a shape: computed once, never written to."""
    if shape not in _INPUTS:
        _, D, M, n, _ = shape
        models = [member_model(D, n, m) for m in range(M)]
        hp = models[0].hparams
        clip = np.stack([make_audio(n, FORCED + 1, hp.delta_t, seed=11 + m) for m in range(M)]).astype(np.float32)
        std = float(hp.sigma) * np.sqrt(0.5 * float(hp.delta_t))
        noise = (std * np.random.default_rng(D).standard_normal((M, n, SAMPLED))).astype(np.float32)
        _INPUTS[shape] = (models, np.stack([param_row(mo) for mo in models]), clip, noise)
    return _INPUTS[shape]


def rows_of(full, mode, member=None):
    """The rows a run is handed out of `full` [M, n, cols]: a bank's (member None) in the sharing `mode`, or member m's on a plain handle."""
    M, n, cols = full.shape
    if mode == "1":
        return full[0, :1]
    if mode == "n":
        return full[0]
    return full.reshape(M * n, cols) if member is None else full[member]


def run(shape, calls, mode=("Mn", "Mn"), member=None, nulls=False, drv=None, tag=""):
    """The calls through cmps_bank_stream* (member None) or, for one member, through cmps_psi_stream* on a plain handle set to its row of
    the parameters; ONE state buffer (state_out == state_in), pre-filled with the guard pattern so that what a record leaves unwritten
    compares too.  nulls: pred_dev / nll_dev NULL in every call and state_out_dev NULL in the last one.
    Returns {"out", "pred", "nll": [paths, steps] float32 bits over the whole plan, "loss": [calls, paths] after every call, "state"}."""
    _, D, M, n, variant = shape
    models, params, clip, noise = inputs(shape)
    hp = models[0].hparams
    bank = member is None
    P = M * n if bank else n
    own = drv is None
    if own:
        drv = G.Driver(D, variant=variant)
        flags = _capi.CMPS_WS_FWD_ONLY
        if bank:
            nbytes = int(drv.lib.cmps_bank_workspace_bytes(D, M, n, T, flags))
            drv.call("cmps_bank_set_params_dev", M, drv.load("params", params), float(hp.sigma), float(hp.delta_t), T, n, flags,
                     drv.new("ws", nbytes), nbytes)
        else:
            nbytes = int(drv.lib.cmps_workspace_bytes(D, n, T, flags))
            drv.call("cmps_set_params_dev", drv.load("params", params[member]), float(hp.sigma), float(hp.delta_t), T, n, flags,
                     drv.new("ws", nbytes), nbytes)
    stream_fn, score_fn = ("cmps_bank_stream", "cmps_bank_stream_score") if bank else ("cmps_psi_stream", "cmps_psi_stream_score")
    sbytes = int(getattr(drv.lib, "cmps_bank_stream_state_bytes" if bank else "cmps_psi_stream_state_bytes")(drv.h, n))
    assert sbytes > 0 and sbytes == P * int(drv.lib.cmps_psi_stream_state_bytes(drv.h, 1))
    state = drv.new("state" + tag, sbytes)
    loss = drv.load("loss" + tag, np.zeros(P, np.float32), const=False)   # (the first scored call resumes a stream: it continues this total)
    audio, nz = rows_of(clip, mode[0], member), rows_of(noise, mode[1], member)
    res = {"out": [], "pred": [], "nll": [], "loss": []}
    k0 = f0 = l0 = 0
    for idx, (kind, s) in enumerate(calls):
        t = f"{tag}_{idx}"
        sin = state if idx else None
        sout = None if (nulls and idx == len(calls) - 1) else state
        if kind == "G":
            z = drv.load("noise" + t, np.ascontiguousarray(nz[:, l0:l0 + s]))
            out = drv.new("out" + t, 4 * P * s, out=torch.float32)
            extra = (nz.shape[0],) if bank else ()
            drv.call(stream_fn, sin, sout, k0, None, 1, 0, z, *extra, s, n, out, None)
            res["out"].append(out.numpy(np.uint32, (P, s)))
            l0 += s
        else:
            a = drv.load("audio" + t, np.ascontiguousarray(audio[:, f0:f0 + s + 1]))
            pred = None if nulls else drv.new("pred" + t, 4 * P * s, out=torch.float32)
            if kind == "F":
                extra = (n,) if bank else ()
                drv.call(stream_fn, sin, sout, k0, a, audio.shape[0], s, None, *extra, 0, n, None, pred)
            else:
                nll = None if nulls else drv.new("nll" + t, 4 * P * s, out=torch.float32)
                drv.call(score_fn, sin, sout, k0, a, audio.shape[0], s, n, nll, loss, pred)
                if nll is not None:
                    res["nll"].append(nll.numpy(np.uint32, (P, s)))
            if pred is not None:
                res["pred"].append(pred.numpy(np.uint32, (P, s)))
            f0 += s
        res["loss"].append(loss.numpy(np.uint32))
        k0 += s
    drv.finish()
    out = {k: np.concatenate(v, axis=1) for k, v in res.items() if v and k != "loss"}
    out["loss"] = np.stack(res["loss"])
    out["state"] = state.numpy(np.uint8, (P, -1))
    if own:
        drv.close()
    return out


_RUNS = {}


def bank_run(shape, calls, mode):
    key = (shape, calls, mode)
    if key not in _RUNS:
        _RUNS[key] = run(shape, calls, mode)
    return _RUNS[key]


def f32(bits):
    return np.ascontiguousarray(bits).view(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plain_stream_is_reproducible(shape):
    """The footing of every bit comparison below: the plain plan run twice on ONE handle gives the same bits."""
    _, D, M, n, variant = shape
    models, params, _, _ = inputs(shape)
    hp = models[0].hparams
    drv = G.Driver(D, variant=variant)
    nbytes = int(drv.lib.cmps_workspace_bytes(D, n, T, 0))
    drv.call("cmps_set_params_dev", drv.load("params", params[1]), float(hp.sigma), float(hp.delta_t), T, n, 0, drv.new("ws", nbytes), nbytes)
    a = run(shape, PLAN, member=1, drv=drv, tag="a")
    b = run(shape, PLAN, member=1, drv=drv, tag="b")
    drv.close()
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.all(np.isfinite(f32(a["out"]))) and f32(a["out"]).any() and f32(a["nll"]).any() and f32(a["pred"]).any()
    assert np.all(np.isfinite(f32(a["loss"]))) and np.all(f32(a["loss"])[-1] != 0) and not f32(a["loss"])[:2].any()


@pytest.mark.parametrize("mode", MODES, ids=["audio1-noisen", "audion-noiseMn", "audioMn-noisen"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_member_m_is_the_plain_stream_bit_for_bit(shape, mode):
    _, D, M, n, variant = shape
    got = bank_run(shape, PLAN, mode)
    assert got["out"].shape == (M * n, SAMPLED) and got["pred"].shape == (M * n, FORCED) and got["nll"].shape == (M * n, 30)
    for m in range(M):
        want = run(shape, PLAN, mode, member=m)
        for k in ("out", "pred", "nll", "state"):
            assert np.array_equal(got[k][m * n:(m + 1) * n], want[k]), (m, k)
        assert np.array_equal(got["loss"][:, m * n:(m + 1) * n], want["loss"]), m          # the running loss after every call
    # the members are models of their own, and shared noise is shared: with one signal and one noise, what differs is the model
    assert not np.array_equal(got["out"][:n], got["out"][n:2 * n])
    # a record ends in padding that is never written (the wave family's 3 floats, the block family's 1 or 3): it kept the pattern
    assert np.all(got["state"].reshape(M * n, -1, 4)[:, -1] == np.frombuffer(np.uint32(G.NAN_FILL).tobytes(), dtype=np.uint8))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_cut_changes_no_bit(shape):
    whole, cut = bank_run(shape, PLAN, ("Mn", "Mn")), bank_run(shape, CUT, ("Mn", "Mn"))
    for k in ("out", "pred", "nll", "state"):
        assert np.array_equal(whole[k], cut[k]), k
    assert np.array_equal(whole["loss"], cut["loss"][1::2])                                # behind the second half of every call


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_stated_extents_only_and_null_outputs(shape):
    """Red zones round every caller array (state_out == state_in) are checked after every call inside run(), and every element of a
    documented output is written (Driver.finish).  With pred_dev, nll_dev and the last state_out_dev NULL, what is left keeps its bits."""
    _, D, M, n, variant = shape
    full, bare = bank_run(shape, PLAN, ("n", "Mn")), run(shape, PLAN, ("n", "Mn"), nulls=True)
    assert "pred" not in bare and "nll" not in bare
    assert np.array_equal(bare["out"], full["out"]) and np.array_equal(bare["loss"], full["loss"])
    # the last call wrote no record: the buffer still holds the one behind the third call
    assert not np.array_equal(bare["state"], full["state"])
    assert np.array_equal(bare["state"], bank_run(shape, PLAN[:3], ("n", "Mn"))["state"])


def test_errors_behind_a_successful_set_params_launch_nothing():
    shape = SHAPES[1]
    _, D, M, n, variant = shape
    assert (M, n) == (2, 5)                                                                # (the row counts below are wrong for THIS M and n)
    models, params, clip, noise = inputs(shape)
    hp = models[0].hparams
    lib = _capi.load()
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == OK
    try:
        Ts = 20
        nbytes = lib.cmps_bank_workspace_bytes(D, M, n, Ts, 0)
        ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        p = torch.from_numpy(params).cuda()
        x = torch.zeros(1 << 16, dtype=torch.float32, device="cuda").data_ptr()           # stands in for every pointer of a refused call
        assert lib.cmps_bank_set_params_dev(h, M, p.data_ptr(), hp.sigma, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
        assert lib.cmps_bank_stream_state_bytes(h, n) == M * lib.cmps_psi_stream_state_bytes(h, n) > 0
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 1) == OK
        torch.cuda.synchronize()

        def stream(sin=None, sout=x, k0=0, audio=x, n_audio=1, forced=4, nz=x, n_noise=n, length=4, n_=n, out=x, pred=None):
            return lib.cmps_bank_stream(h, sin, sout, k0, audio, n_audio, forced, nz, n_noise, length, n_, out, pred, None)

        def score(sin=None, sout=x, k0=0, audio=x, n_audio=1, forced=4, n_=n, nll=x, loss=x, pred=None):
            return lib.cmps_bank_stream_score(h, sin, sout, k0, audio, n_audio, forced, n_, nll, loss, pred, None)

        def refused(code, want, who, *words):
            msg = lib.cmps_last_error(h).decode()
            assert code == want and msg.startswith(who + ":") and all(w in msg for w in words), (who, code, msg)

        for bad in (0, 2, 6, 11, -1):
            refused(stream(n_audio=bad), BAD, "cmps_bank_stream", "n_audio")
            refused(score(n_audio=bad), BAD, "cmps_bank_stream_score", "n_audio")
        for bad in (0, 1, 2, 9, 20):
            refused(stream(n_noise=bad), BAD, "cmps_bank_stream", "n_noise")
        refused(stream(k0=Ts - 8, sin=x), BAD, "cmps_bank_stream", f"T >= {Ts + 1}")      # rows beyond T, naming the needed T
        refused(score(k0=Ts - 4, sin=x), BAD, "cmps_bank_stream_score", f"T >= {Ts + 1}")
        refused(stream(sin=x), BAD, "cmps_bank_stream", "state_in_dev")                    # state NULL <=> k0 == 0
        refused(stream(k0=3), BAD, "cmps_bank_stream", "state_in_dev")
        refused(score(sin=x), BAD, "cmps_bank_stream_score", "state_in_dev")
        refused(score(k0=3), BAD, "cmps_bank_stream_score", "state_in_dev")
        refused(stream(n_=0), BAD, "cmps_bank_stream")
        refused(stream(forced=0, length=0), BAD, "cmps_bank_stream")
        refused(stream(audio=None), BAD, "cmps_bank_stream", "audio_dev")
        refused(stream(nz=None), BAD, "cmps_bank_stream", "noise_dev")
        refused(stream(out=None), BAD, "cmps_bank_stream", "out_dev")
        refused(score(forced=0), BAD, "cmps_bank_stream_score")
        refused(score(audio=None), BAD, "cmps_bank_stream_score", "audio_dev")
        refused(score(loss=None), BAD, "cmps_bank_stream_score", "loss_dev")
        refused(stream(n_=2 ** 28, n_audio=1, n_noise=2 ** 28), BAD, "cmps_bank_stream", "2^31")
        refused(score(n_=2 ** 29, n_audio=1), BAD, "cmps_bank_stream_score", "2^31")
        # the plain entries stay refused in bank mode
        refused(lib.cmps_psi_stream(h, None, x, 0, None, 1, 0, x, 4, 1, x, None, None), STATE, "cmps_psi_stream")
        refused(lib.cmps_psi_stream_score(h, None, x, 0, x, 1, 4, 1, x, x, None, None), STATE, "cmps_psi_stream_score")
        # a changed option, plain mode, legacy mode
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_F16_SCALE_SHIFT, 1) == OK
        refused(stream(), STATE, "cmps_bank_stream")
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_F16_SCALE_SHIFT, 0) == OK
        names = ctypes.create_string_buffer(512)
        ms, calls = (ctypes.c_float * 8)(), (ctypes.c_int * 8)()
        assert lib.cmps_kernel_times(h, names, 512, ms, calls, 8) == 0                     # none of these launched anything
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 0) == OK
        assert lib.cmps_set_params_dev(h, p.data_ptr(), hp.sigma, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
        refused(stream(), STATE, "cmps_bank_stream", "cmps_bank_set_params_dev")
        refused(score(), STATE, "cmps_bank_stream_score", "cmps_bank_set_params_dev")
        assert lib.cmps_bank_stream_state_bytes(h, n) == 0
        assert lib.cmps_legacy_set_params(h, x, x, x, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
        refused(stream(), STATE, "cmps_bank_stream")
        refused(score(), STATE, "cmps_bank_stream_score")
        assert lib.cmps_bank_stream_state_bytes(h, n) == 0
        torch.cuda.synchronize()
    finally:
        lib.cmps_destroy(h)


def test_a_rho_bank_is_refused_and_the_kernel_names():
    from audio_mps_amd.scan import HipScan
    from test_gpu_rho_bank import hparams as rho_hparams, member_arrays
    D, rank, n, M = 8, 3, 2, 2
    be = HipScan(D)
    arrays = [member_arrays(D, rank, n, 50 + m) for m in range(M)]
    p = torch.from_numpy(np.stack([a[0] for a in arrays])).cuda()
    f = torch.from_numpy(np.stack([a[1] for a in arrays])).cuda()
    hp = rho_hparams(D, rank, n)
    be.rho_bank_set_state_dev(p, f, rank, hp.sigma, hp.delta_t, n, 20, train=False)
    x = torch.zeros(4096, dtype=torch.float32, device="cuda").data_ptr()
    lib, h = be._lib, be._h
    assert lib.cmps_bank_stream_state_bytes(h, n) == 0
    assert lib.cmps_bank_stream(h, None, x, 0, x, 1, 4, x, n, 4, n, x, None, None) == _capi.CMPS_ERR_STATE
    assert lib.cmps_last_error(h).decode().startswith("cmps_bank_stream:")
    assert lib.cmps_bank_stream_score(h, None, x, 0, x, 1, 4, n, x, x, None, None) == _capi.CMPS_ERR_STATE
    assert lib.cmps_last_error(h).decode().startswith("cmps_bank_stream_score:")
    # the launches of a PsiCMPS bank are recorded under the plain entries' names
    for variant, family in ((AUTO, "wave"), (BLOCK, "block")):
        be = HipScan(D, variant=variant)
        be.bank_set_params([member_model(D, n, m).effective_params() for m in range(M)], n, 20)
        be.kernel_events(True)
        st = be.bank_stream_state(n)
        be.bank_stream(None, st, 0, np.zeros((1, 5), np.float32), np.zeros((3, n), np.float32), n=n)
        be.bank_stream_score(st, st, 7, np.zeros((M * n, 4), np.float32), n=n)
        times = be.kernel_times()
        assert list(times) == [f"k_sample_{family}_stream", f"k_sample_{family}_score"] and all(c == 1 for _, c in times.values())


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5]], ids=[IDS[2], IDS[5]])
def test_against_the_float64_oracle(shape):
    """Bank and plain could be wrong together: every member against the float64 composition, at the samplers' own bars.

    Measured on an MI355X (waveform err / max|w|, bar 2e-4; total err relative to max(|l|, 1), bar 1e-5):
      D   member  max|w|     waveform   total
      17  0       1.002e+00  1.908e-07  9.532e-07
      17  1       1.305e+00  9.423e-08  5.181e-07
      17  2       1.229e+00  1.315e-07  4.443e-07
      17  3       1.030e+00  3.846e-07  4.284e-07
      40  0       6.806e-01  3.552e-07  7.160e-07
      40  1       9.178e-01  2.675e-07  1.390e-06"""
    _, D, M, n, variant = shape
    models, _, clip, noise = inputs(shape)
    got = bank_run(shape, PLAN, ("Mn", "Mn"))
    plan = [(SC.FOLLOW, 70), (SC.SAMPLE, 50), (SC.SCORE, 30), (SC.SAMPLE, 65)]
    for m, mo in enumerate(models):
        _, total, _, out, _ = SC.score_reference(oracle_hparams(mo.hparams), oracle_variables(mo), plan, clip[m], noise[m].T, "f64")
        w = f32(got["out"])[m * n:(m + 1) * n]
        loss = f32(got["loss"])[-1, m * n:(m + 1) * n]
        e_out = float(np.max(np.abs(w - out))) / float(np.max(np.abs(out)))
        e_tot = float(np.max(np.abs(loss - total) / np.maximum(np.abs(total), 1.0)))
        print(f"bank stream D={D} member {m}: max|w| {float(np.max(np.abs(out))):.3e}  waveform err / max|w| {e_out:.3e} (bar {OUT_RTOL:.0e})  "
              f"total err {e_tot:.3e} (bar {LOSS_RTOL:.0e})  max|total| {float(np.max(np.abs(total))):.3e}")
        assert float(np.max(np.abs(out))) > 1e-3 and np.all(total != 0)                    # the bars are not vacuous
        assert e_out <= OUT_RTOL and e_tot <= LOSS_RTOL


MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1}, {"seed": 4, "learning_rate": 3e-3}, {"seed": 5, "r_reg": 1.0}]


def test_open_stream_end_to_end_next_to_a_trainer():
    """PsiBank.open_stream on a bank whose BankTrainer has taken two device steps: the stream sees the stepped parameters, and a further
    training step behind it gives the bits of a run that never opened a stream."""
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.scan import HipScan
    D, B, Tt, n = 8, 2, 40, 3
    hp = HParams(minibatch_size=B, bond_dim=D)
    audio = make_audio(B, Tt, hp.delta_t, seed=2)
    clip = make_audio(n, 50, hp.delta_t, seed=3)

    def trained():
        bt = BankTrainer(PsiBank(hp, MEMBERS, backend=HipScan(D)))
        assert bt.native
        bt.step(audio, sync=False)
        bt.step(audio, sync=False)
        return bt

    bt, ref = trained(), trained()
    st = bt.bank.open_stream(n, 120, temp=0.5, seed=9, device_noise=True)
    assert st.native and st._be is not bt.bank.backend
    got = [st.follow(clip[:, :20]), st.generate(30), st.score(clip[:, 20:]), st.generate(40)]
    own = bt.open_stream(n, 120, temp=0.5, seed=9, device_noise=True, independent_noise=True)
    own.follow(clip[:, :20])
    wave_own = own.generate(30)
    after, after_ref = bt.step(audio), ref.step(audio)                                     # the trainer's workspace was never disturbed
    assert np.array_equal(after["model_loss"], after_ref["model_loss"]) and np.array_equal(after["total_loss"], after_ref["total_loss"])
    for m in range(len(MEMBERS)):
        for k, v in ref.member(m).variables.items():
            assert np.array_equal(bt.member(m).variables[k], v), (m, k)
    two = trained()                                                                        # the members as they were when the stream was opened
    for m in range(len(MEMBERS)):
        ms = two.member(m).open_stream(n, 120, temp=0.5, seed=9, device_noise=True)
        want = [ms.follow(clip[:, :20]), ms.generate(30), ms.score(clip[:, 20:]), ms.generate(40)]
        for a, b in zip(got, want):
            assert np.array_equal(a[m], b), m
        assert np.array_equal(st.total_nll[m], ms.total_nll)
        # independent noise: global path g = m n + b
        be = two.member(m)._get_backend()
        ms = two.member(m).open_stream(n, 120, temp=0.5)
        ms.follow(clip[:, :20])
        z = be.draw_noise(9, 19, n, 30, ms._std, first_path=m * n).cpu().numpy().T
        assert np.array_equal(wave_own[m], ms.generate(30, noise=z)), m
    assert not np.array_equal(wave_own[1], got[1][1]) and np.array_equal(wave_own[0], got[1][0])
    assert st.best().shape == (n,) and np.array_equal(st.best(), np.argmin(st.total_nll, axis=0))
