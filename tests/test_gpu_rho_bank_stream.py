"""A RhoCMPS bank's streams on the GPU (cmps_rho_bank_stream, cmps_rho_bank_stream_score, audio_mps_amd/stream.py::BankStream over a
RhoBank): member m's slices of out, pred, nll, the running loss and the state records hold, BIT FOR BIT, what cmps_rho_stream /
cmps_rho_stream_score give on a fresh plain handle set to model m (cmps_set_params_dev on row m of the parameters, cmps_rho_set_state on
member m's columns) with the same T, fed member m's audio and noise rows -- k_sample_rho_mfma's STREAM / SCORE instances with a member
grid dimension.

Every comparison is np.array_equal on raw bytes, and every caller array of every call lies between two red zones (tests/_guard.py), checked
after each call.  That bar rests on the plain path being reproducible, which test_plain_stream_is_reproducible checks first.

One plan per shape: follow 70, generate 50, score 30, generate 65 (215 steps, off the 64-step chunk; tables of T = 216), and the same plan
with every call cut in two at an odd point.  Shapes (D, rank, M, n): the smallest D and rank, an odd rank with n such that the last
workgroup is partial (n = 5 with four waves a workgroup), D above 16 with M > 2, the full width D = rank = 32.

Against the float64 oracle (tests/_rho_score_ref.py) the bars are the RhoCMPS samplers' own: waveform <= 2e-4 max|w|, scored totals <=
1e-5 max(|l|, 1).
"""
import ctypes

import numpy as np
import pytest
import torch

from audio_mps_amd import HParams, RhoCMPS, _capi, layout

import _guard as G
import _rho_score_ref as RC
from _rho_primed_ref import oracle_side
from _util import make_audio

pytestmark = pytest.mark.gpu

#          D  rank M  n
SHAPES = [(3, 3, 3, 3),
          (16, 5, 2, 5),
          (17, 8, 4, 3),
          (32, 32, 3, 2)]
IDS = [f"D{s[0]}-r{s[1]}" for s in SHAPES]
PLAN = (("F", 70), ("G", 50), ("S", 30), ("G", 65))
CUT = (("F", 33), ("F", 37), ("G", 23), ("G", 27), ("S", 13), ("S", 17), ("G", 31), ("G", 34))
STEPS = sum(s for _, s in PLAN)
T = STEPS + 1
FORCED = sum(s for k, s in PLAN if k != "G")
SAMPLED = STEPS - FORCED
# (rows of the audio, rows of the noise) as multiples: "1" one row, "n", "Mn"
MODES = (("1", "n"), ("n", "Mn"), ("Mn", "n"))
OUT_RTOL, LOSS_RTOL = 2e-4, 1e-5
FLAGS = _capi.CMPS_WS_FWD_ONLY


def member_model(D, rank, n, m):
    """Member m: the model of the RhoCMPS sampler tests (sigma = 0.1, A = 5, Rx, Ry x 0.3) with its own seed and its own A."""
    mo = RhoCMPS(HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0 + m), seed=100 + m, backend=object())
    mo.variables["Rx"] *= np.float32(0.3)
    mo.variables["Ry"] *= np.float32(0.3)
    return mo


def member_rows(mo):
    """(params row R_re | R_im | freqs | psi0_re | psi0_im | A, phi row phi_re | phi_im) of a member"""
    p, D = mo.effective_params(), mo.bond_d
    params = layout.pack(layout.param_fields(D, with_A=True), {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})
    return params, layout.pack(layout.phi_fields(D, mo.rank_rho_0), layout.split("phi", mo.columns()))


_INPUTS = {}


def inputs(shape):
    """(models, params [M, NP], phi [M, 2 rank D], clip [M, n, FORCED + 1], noise [M, n, SAMPLED]) of a shape: computed once, never written to."""
    if shape not in _INPUTS:
        D, rank, M, n = shape
        models = [member_model(D, rank, n, m) for m in range(M)]
        hp = models[0].hparams
        rows = [member_rows(mo) for mo in models]
        clip = np.stack([make_audio(n, FORCED + 1, hp.delta_t, seed=11 + m) for m in range(M)]).astype(np.float32)
        std = float(hp.sigma) * np.sqrt(0.5 * float(hp.delta_t))
        noise = (std * np.random.default_rng(D).standard_normal((M, n, SAMPLED))).astype(np.float32)
        _INPUTS[shape] = (models, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), clip, noise)
    return _INPUTS[shape]


def rows_of(full, mode, member=None):
    """The rows a run is handed out of `full` [M, n, cols]: a bank's (member None) in the sharing `mode`, or member m's on a plain handle."""
    M, n, cols = full.shape
    if mode == "1":
        return full[0, :1]
    if mode == "n":
        return full[0]
    return full.reshape(M * n, cols) if member is None else full[member]


def configure(drv, shape, member=None):
    """cmps_rho_bank_set_state_dev for the whole bank, or the plain pair of calls for one member, on tables of T rows."""
    D, rank, M, n = shape
    models, params, phi, _, _ = inputs(shape)
    hp = models[0].hparams
    if member is None:
        nbytes = int(drv.lib.cmps_rho_bank_workspace_bytes(D, rank, M, n, T, FLAGS))
        assert nbytes > 0
        drv.call("cmps_rho_bank_set_state_dev", M, drv.load("params", params), drv.load("phi", phi), rank, float(hp.sigma), float(hp.delta_t),
                 T, n, FLAGS, drv.new("ws", nbytes), nbytes)
    else:
        nbytes = int(drv.lib.cmps_workspace_bytes(D, n, T, FLAGS))
        drv.call("cmps_set_params_dev", drv.load("params", params[member]), float(hp.sigma), float(hp.delta_t), T, n, FLAGS,
                 drv.new("ws", nbytes), nbytes)
        rbytes = int(drv.lib.cmps_rho_workspace_bytes(D, rank, n, T, FLAGS))
        f = drv.load("phi", phi[member])
        drv.call("cmps_rho_set_state", f, f.ptr + 4 * rank * D, rank, T, n, FLAGS, drv.new("rho_ws", rbytes), rbytes)


def run(shape, calls, mode=("Mn", "Mn"), member=None, nulls=False, drv=None, tag=""):
    """The calls through cmps_rho_bank_stream* (member None) or, for one member, through cmps_rho_stream* on a plain handle set to its
    rows; ONE state buffer (state_out == state_in), pre-filled with the guard pattern so that what a record leaves unwritten compares too.
    nulls: pred_dev / nll_dev NULL in every call and state_out_dev NULL in the last one.
    Returns {"out", "pred", "nll": [paths, steps] float32 bits over the whole plan, "loss": [calls, paths] after every call, "state"}."""
    D, rank, M, n = shape
    _, _, _, clip, noise = inputs(shape)
    bank = member is None
    P = M * n if bank else n
    own = drv is None
    if own:
        drv = G.Driver(D)
        configure(drv, shape, member)
    stream_fn, score_fn = ("cmps_rho_bank_stream", "cmps_rho_bank_stream_score") if bank else ("cmps_rho_stream", "cmps_rho_stream_score")
    sbytes = int(getattr(drv.lib, "cmps_rho_bank_stream_state_bytes" if bank else "cmps_rho_stream_state_bytes")(drv.h, n))
    assert sbytes == P * (64 * rank + 4) * 4
    plain_tail = () if bank else (0,)                                          # save_states of the plain entries
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
            drv.call(stream_fn, sin, sout, k0, None, 1, 0, z, *extra, s, n, out, None, *plain_tail)
            res["out"].append(out.numpy(np.uint32, (P, s)))
            l0 += s
        else:
            a = drv.load("audio" + t, np.ascontiguousarray(audio[:, f0:f0 + s + 1]))
            pred = None if nulls else drv.new("pred" + t, 4 * P * s, out=torch.float32)
            if kind == "F":
                extra = (n,) if bank else ()
                drv.call(stream_fn, sin, sout, k0, a, audio.shape[0], s, None, *extra, 0, n, None, pred, *plain_tail)
            else:
                nll = None if nulls else drv.new("nll" + t, 4 * P * s, out=torch.float32)
                drv.call(score_fn, sin, sout, k0, a, audio.shape[0], s, n, nll, loss, pred, *plain_tail)
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
    drv = G.Driver(shape[0])
    configure(drv, shape, member=1)
    a = run(shape, PLAN, member=1, drv=drv, tag="a")
    b = run(shape, PLAN, member=1, drv=drv, tag="b")
    names = set(drv.calls)
    drv.close()
    assert {"cmps_rho_stream", "cmps_rho_stream_score"} <= names
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.all(np.isfinite(f32(a["out"]))) and f32(a["out"]).any() and f32(a["nll"]).any() and f32(a["pred"]).any()
    assert np.all(np.isfinite(f32(a["loss"]))) and np.all(f32(a["loss"])[-1] != 0) and not f32(a["loss"])[:2].any()


@pytest.mark.parametrize("mode", MODES, ids=["audio1-noisen", "audion-noiseMn", "audioMn-noisen"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_member_m_is_the_plain_stream_bit_for_bit(shape, mode):
    D, rank, M, n = shape
    got = bank_run(shape, PLAN, mode)
    assert got["out"].shape == (M * n, SAMPLED) and got["pred"].shape == (M * n, FORCED) and got["nll"].shape == (M * n, 30)
    for m in range(M):
        want = run(shape, PLAN, mode, member=m)
        for k in ("out", "pred", "nll", "state"):
            assert np.array_equal(got[k][m * n:(m + 1) * n], want[k]), (m, k)
        assert np.array_equal(got["loss"][:, m * n:(m + 1) * n], want["loss"]), m          # the running loss after every call
    # the members are models of their own, and shared noise is shared: with one signal and one noise, what differs is the model
    assert not np.array_equal(got["out"][:n], got["out"][n:2 * n])
    # a record ends in three floats of padding that are never written: they kept the pattern
    assert np.all(got["state"].reshape(M * n, -1, 4)[:, -3:] == np.frombuffer(np.uint32(G.NAN_FILL).tobytes(), dtype=np.uint8))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_cut_changes_no_bit(shape):
    whole, cut = bank_run(shape, PLAN, ("Mn", "Mn")), bank_run(shape, CUT, ("Mn", "Mn"))
    for k in ("out", "pred", "nll", "state"):
        assert np.array_equal(whole[k], cut[k]), k
    assert np.array_equal(whole["loss"], cut["loss"][1::2])                                # behind the second half of every call


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_stated_extents_only_and_null_outputs(shape):
    """Red zones round every caller array (state_out == state_in) are checked after every call inside run(), and every element of a
    documented output is written (Driver.finish).  With pred_dev, nll_dev and the last state_out_dev NULL, what is left keeps its bits."""
    full, bare = bank_run(shape, PLAN, ("n", "Mn")), run(shape, PLAN, ("n", "Mn"), nulls=True)
    assert "pred" not in bare and "nll" not in bare
    assert np.array_equal(bare["out"], full["out"]) and np.array_equal(bare["loss"], full["loss"])
    # the last call wrote no record: the buffer still holds the one behind the third call
    assert not np.array_equal(bare["state"], full["state"])
    assert np.array_equal(bare["state"], bank_run(shape, PLAN[:3], ("n", "Mn"))["state"])


def _kernel_names(lib, h):
    names = ctypes.create_string_buffer(512)
    ms, calls = (ctypes.c_float * 8)(), (ctypes.c_int * 8)()
    k = lib.cmps_kernel_times(h, names, 512, ms, calls, 8)
    assert k >= 0
    return [x for x in names.value.decode().split("\n") if x], list(calls)[:k]


def test_errors_behind_a_successful_set_state_launch_nothing_and_the_kernel_names():
    shape = SHAPES[1]
    D, rank, M, n = shape
    assert (M, n) == (2, 5)                                                                # (the row counts below are wrong for THIS M and n)
    models, params, phi, clip, noise = inputs(shape)
    hp = models[0].hparams
    lib = _capi.load()
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == OK
    try:
        Ts = 20
        nbytes = lib.cmps_rho_bank_workspace_bytes(D, rank, M, n, Ts, 0)
        ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        p, f = torch.from_numpy(params).cuda(), torch.from_numpy(phi).cuda()
        x = torch.zeros(1 << 16, dtype=torch.float32, device="cuda").data_ptr()           # stands in for every pointer of a refused call

        def set_state():
            return lib.cmps_rho_bank_set_state_dev(h, M, p.data_ptr(), f.data_ptr(), rank, hp.sigma, hp.delta_t, Ts, n, 0, ptr, nbytes, None)

        assert set_state() == OK
        rec = 4 * (64 * rank + 4)
        assert lib.cmps_rho_bank_stream_state_bytes(h, n) == M * n * rec and lib.cmps_rho_bank_stream_state_bytes(h, 0) == 0
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 1) == OK
        torch.cuda.synchronize()

        def stream(sin=None, sout=x, k0=0, audio=x, n_audio=1, forced=4, nz=x, n_noise=n, length=4, n_=n, out=x, pred=None):
            return lib.cmps_rho_bank_stream(h, sin, sout, k0, audio, n_audio, forced, nz, n_noise, length, n_, out, pred, None)

        def score(sin=None, sout=x, k0=0, audio=x, n_audio=1, forced=4, n_=n, nll=x, loss=x, pred=None):
            return lib.cmps_rho_bank_stream_score(h, sin, sout, k0, audio, n_audio, forced, n_, nll, loss, pred, None)

        def refused(code, want, who, *words):
            msg = lib.cmps_last_error(h).decode()
            assert code == want and msg.startswith(who + ":") and all(w in msg for w in words), (who, code, msg)

        S, C = "cmps_rho_bank_stream", "cmps_rho_bank_stream_score"
        for bad in (0, 2, 6, 11, -1):
            refused(stream(n_audio=bad), BAD, S, "n_audio")
            refused(score(n_audio=bad), BAD, C, "n_audio")
        for bad in (0, 1, 2, 9, 20):
            refused(stream(n_noise=bad), BAD, S, "n_noise")
        refused(stream(k0=Ts - 8, sin=x), BAD, S, f"T >= {Ts + 1}")                        # rows beyond T, naming the needed T
        refused(score(k0=Ts - 4, sin=x), BAD, C, f"T >= {Ts + 1}")
        refused(stream(sin=x), BAD, S, "state_in_dev")                                     # state NULL <=> k0 == 0
        refused(stream(k0=3), BAD, S, "state_in_dev")
        refused(score(sin=x), BAD, C, "state_in_dev")
        refused(score(k0=3), BAD, C, "state_in_dev")
        refused(stream(n_=0), BAD, S)
        refused(stream(forced=0, length=0), BAD, S)
        refused(stream(audio=None), BAD, S, "audio_dev")
        refused(stream(nz=None), BAD, S, "noise_dev")
        refused(stream(out=None), BAD, S, "out_dev")
        refused(score(forced=0), BAD, C)
        refused(score(audio=None), BAD, C, "audio_dev")
        refused(score(loss=None), BAD, C, "loss_dev")
        refused(stream(n_=2 ** 28, n_audio=1, n_noise=2 ** 28), BAD, S, "2^31")
        refused(score(n_=2 ** 29, n_audio=1), BAD, C, "2^31")
        # the plain entries and the PsiCMPS bank's stay refused in RhoCMPS bank mode
        refused(lib.cmps_rho_stream(h, None, x, 0, None, 1, 0, x, 4, 1, x, None, 0, None), STATE, "cmps_rho_stream")
        refused(lib.cmps_rho_stream_score(h, None, x, 0, x, 1, 4, 1, x, x, None, 0, None), STATE, "cmps_rho_stream_score")
        refused(lib.cmps_bank_stream(h, None, x, 0, x, 1, 4, x, n, 4, n, x, None, None), STATE, "cmps_bank_stream")
        assert lib.cmps_rho_stream_state_bytes(h, n) == 0 and lib.cmps_bank_stream_state_bytes(h, n) == 0
        # a non-default option or another variant set behind cmps_rho_bank_set_state_dev
        for opt, val, back in ((_capi.CMPS_OPT_F16_SCALE_SHIFT, 1, 0), (_capi.CMPS_OPT_RANK1, _capi.CMPS_RANK1_BF16X3, _capi.CMPS_RANK1_DEFAULT),
                               (_capi.CMPS_OPT_RHO_BWD, 1, 0)):
            assert lib.cmps_get_option(h, opt) == back
            assert lib.cmps_set_option(h, opt, val) == OK
            refused(stream(), STATE, S, "default")
            refused(score(), STATE, C, "default")
            assert lib.cmps_set_option(h, opt, back) == OK
        assert lib.cmps_set_variant(h, _capi.CMPS_VARIANT_BLOCK) == OK
        refused(stream(), STATE, S, "CMPS_VARIANT")
        refused(score(), STATE, C, "CMPS_VARIANT")
        assert lib.cmps_set_variant(h, _capi.CMPS_VARIANT_AUTO) == OK
        assert _kernel_names(lib, h)[0] == []                                              # none of these launched anything
        # ... and the two that are not refused are recorded under the plain entries' names
        st = torch.zeros(M * n * rec, dtype=torch.uint8, device="cuda")
        a = torch.from_numpy(np.ascontiguousarray(clip[0, :, :5])).cuda()
        z = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        o = torch.empty((M, n, 4), dtype=torch.float32, device="cuda")
        lo = torch.zeros((M, n), dtype=torch.float32, device="cuda")
        assert stream(sout=st.data_ptr(), audio=a.data_ptr(), n_audio=n, nz=z.data_ptr(), out=o.data_ptr()) == OK
        assert score(sin=st.data_ptr(), sout=st.data_ptr(), k0=8, audio=a.data_ptr(), n_audio=n, nll=None, loss=lo.data_ptr()) == OK
        torch.cuda.synchronize()
        assert _kernel_names(lib, h) == (["k_sample_rho_mfma_stream", "k_sample_rho_mfma_score"], [1, 1])
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 0) == OK
        # plain mode, a PsiCMPS bank, legacy mode
        pbytes = lib.cmps_workspace_bytes(D, n, Ts, 0)
        assert pbytes <= nbytes
        assert lib.cmps_set_params_dev(h, p.data_ptr(), hp.sigma, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
        for mode_set in (None, "bank", "legacy"):
            if mode_set == "bank":
                assert lib.cmps_bank_workspace_bytes(D, M, n, Ts, 0) <= nbytes
                assert lib.cmps_bank_set_params_dev(h, M, p.data_ptr(), hp.sigma, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
            if mode_set == "legacy":
                assert lib.cmps_legacy_set_params(h, x, x, x, hp.delta_t, Ts, n, 0, ptr, nbytes, None) == OK
            refused(stream(), STATE, S, "cmps_rho_bank_set_state_dev")
            refused(score(), STATE, C, "cmps_rho_bank_set_state_dev")
            assert lib.cmps_rho_bank_stream_state_bytes(h, n) == 0
        torch.cuda.synchronize()
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=[IDS[2], IDS[3]])
def test_against_the_float64_oracle(shape):
    """Bank and plain could be wrong together: every member against the float64 composition, at the RhoCMPS samplers' own bars.

    Measured on an MI355X (waveform err / max|w|, bar 2e-4; total err relative to max(|l|, 1), bar 1e-5):
      D   rank  member  max|w|     waveform   total
      17  8     0       6.678e-02  4.501e-06  3.897e-06
      17  8     1       7.458e-02  4.134e-06  5.850e-06
      17  8     2       9.045e-02  4.197e-06  2.045e-06
      17  8     3       5.277e-02  6.563e-06  4.904e-06
      32  32    0       4.775e-02  5.277e-06  3.484e-06
      32  32    1       5.528e-02  5.718e-06  1.643e-06
      32  32    2       5.443e-02  1.375e-05  4.199e-06"""
    D, rank, M, n = shape
    models, _, _, clip, noise = inputs(shape)
    got = bank_run(shape, PLAN, ("Mn", "Mn"))
    plan = [(RC.FOLLOW, 70), (RC.SAMPLE, 50), (RC.SCORE, 30), (RC.SAMPLE, 65)]
    for m, mo in enumerate(models):
        ohp, ov, Wx, Wy = oracle_side(mo)
        _, total, _, out, _, _, _ = RC.rho_score_reference(ohp, ov, Wx, Wy, plan, clip[m], noise[m].T, "f64")
        w = f32(got["out"])[m * n:(m + 1) * n]
        loss = f32(got["loss"])[-1, m * n:(m + 1) * n]
        e_out = float(np.max(np.abs(w - out))) / float(np.max(np.abs(out)))
        e_tot = float(np.max(np.abs(loss - total) / np.maximum(np.abs(total), 1.0)))
        print(f"rho bank stream D={D} rank={rank} member {m}: max|w| {float(np.max(np.abs(out))):.3e}  waveform err / max|w| {e_out:.3e} "
              f"(bar {OUT_RTOL:.0e})  total err {e_tot:.3e} (bar {LOSS_RTOL:.0e})  max|total| {float(np.max(np.abs(total))):.3e}")
        assert float(np.max(np.abs(out))) > 1e-3 and np.all(total != 0)                    # the bars are not vacuous
        assert e_out <= OUT_RTOL and e_tot <= LOSS_RTOL


MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1}, {"seed": 4, "learning_rate": 3e-3}, {"seed": 5, "r_reg": 1.0}]


def test_open_stream_end_to_end_next_to_a_trainer():
    """RhoBank.open_stream on a bank whose BankTrainer has taken two device steps: the stream sees the stepped parameters, and a further
    training step behind it gives the bits of a run that never opened a stream."""
    from audio_mps_amd.bank import BankTrainer, RhoBank
    from audio_mps_amd.scan import HipScan
    D, rank, B, Tt, n = 8, 4, 2, 40, 3
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=rank)
    audio = make_audio(B, Tt, hp.delta_t, seed=2)
    clip = make_audio(n, 50, hp.delta_t, seed=3)

    def trained():
        bt = BankTrainer(RhoBank(hp, MEMBERS, backend=HipScan(D)))
        assert bt.native
        bt.step(audio, sync=False)
        bt.step(audio, sync=False)
        return bt

    bt, ref = trained(), trained()
    fresh = RhoBank(hp, MEMBERS, backend=HipScan(D)).open_stream(n, 120, temp=0.5, seed=9, device_noise=True)
    st = bt.open_stream(n, 120, temp=0.5, seed=9, device_noise=True)
    assert st.native and st._be is not bt.bank.backend
    got = [st.follow(clip[:, :20]), st.generate(30), st.score(clip[:, 20:]), st.generate(40)]
    assert not np.array_equal(got[0], fresh.follow(clip[:, :20]))                          # the stepped parameters, not the initial ones
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
