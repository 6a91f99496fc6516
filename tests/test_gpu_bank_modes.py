"""The host rules of the bank layer, pinned where nothing else pins them.

  1. ONE HipScan walked through its modes (plain, PsiCMPS bank, RhoCMPS bank, legacy, a bank of another M, plain RhoCMPS, RhoCMPS bank
     again) with one (B, T) throughout, so that the main workspace is reallocated at every change of kind and the allocator may hand
     back an address whose tables are stale: every stage gives, BIT FOR BIT, what a fresh HipScan gives for that stage alone, and
     every bank call made after its mode was left raises RuntimeError and launches nothing.
  2. Every refusal of the stream and score entries that needs a configured handle (cmps_{psi,rho,bank}_stream, cmps_{psi,rho,bank}_
     stream_score), with its code and its whole message as literals, in the order the checks fire.  The apply-step entries' refusals
     need no device: tests/test_bank_capi.py.

Shapes: D = 4 (the 16-row family) and D = 20 (the 32-row family), rank 3, M = 2 (and 3), B = 2, T = 9 -- the smallest that still has
two members, two clips and an odd step count; the refusals at D = 4, M = 2, n = 2, T = 8."""
import numpy as np
import pytest
import torch

from audio_mps_amd import HParams, RhoCMPS, _capi, layout

from _util import make_audio

pytestmark = pytest.mark.gpu

RANK, B, T = 3, 2, 9


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Models:
    """Three RhoCMPS models of one D: their effective parameters (host and packed), their columns, a legacy (R, Q) pair, the audio."""

    def __init__(self, D):
        self.D = D
        self.hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=RANK)
        models = [RhoCMPS(self.hp, seed=100 + m, backend=object()) for m in range(3)]
        self.eff = [mo.effective_params() for mo in models]
        self.cols = [mo.columns() for mo in models]
        fields = layout.param_fields(D, with_A=True)
        self.params = np.stack([layout.pack(fields, {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})
                                for p in self.eff])
        self.phi = np.stack([layout.pack(layout.phi_fields(D, RANK), layout.split("phi", c)) for c in self.cols])
        rng = np.random.default_rng(D)
        self.R = (0.1 * rng.standard_normal((D, D))).astype(np.float32)
        self.Q = (0.01 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
        self.audio = np.stack([make_audio(B, T, self.hp.delta_t, seed=7 + m) for m in range(3)])


def done(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in tensors]


# the stages: each configures `be` and runs one forward and one backward; (losses, gradient sums) as host arrays
def stage_plain(be, mo, shared):
    be.set_params(mo.eff[0], B, T)
    loss = be.forward(torch.from_numpy(mo.audio[0]).cuda(), save_for_bwd=True)
    return done(loss, be.backward())


def bank_audio(mo, M, shared):
    return torch.from_numpy(np.ascontiguousarray(mo.audio[1] if shared else mo.audio[:M])).cuda()


def stage_psi_bank(M):
    def run(be, mo, shared):
        p = torch.from_numpy(mo.params[:M].copy()).cuda()           # (held until the scans have run: they read A from it)
        be.bank_set_params_dev(p, mo.hp.sigma, mo.hp.delta_t, B, T, train=True)
        loss = be.bank_forward(bank_audio(mo, M, shared), save_for_bwd=True)
        assert tuple(loss.shape) == (M, B)
        return done(loss, be.bank_backward())
    return run


def stage_rho_bank(be, mo, shared):
    p, f = torch.from_numpy(mo.params[:2].copy()).cuda(), torch.from_numpy(mo.phi[:2].copy()).cuda()
    be.rho_bank_set_state_dev(p, f, RANK, mo.hp.sigma, mo.hp.delta_t, B, T, train=True)
    loss = be.rho_bank_forward(bank_audio(mo, 2, shared), save_for_bwd=True)
    return done(loss, be.rho_bank_backward())


def stage_legacy(be, mo, shared):
    be.legacy_set_params(mo.R, mo.Q, mo.hp.delta_t, B, T)
    loss = be.legacy_forward(torch.from_numpy(mo.audio[2]).cuda(), save_for_bwd=True)
    return done(loss, be.legacy_backward())


def stage_plain_rho(be, mo, shared):
    be.set_params(mo.eff[1], B, T)
    be.rho_set_state(mo.cols[1], B, T)
    loss = be.rho_forward(torch.from_numpy(mo.audio[1]).cuda(), save_for_bwd=True)
    return done(loss, be.rho_backward())


#        name            stage                 the bank mode the handle is in behind it
WALK = [("plain", stage_plain, None),
        ("psi bank", stage_psi_bank(2), "bank"),
        ("rho bank", stage_rho_bank, "rho_bank"),
        ("legacy", stage_legacy, None),
        ("psi bank M=3", stage_psi_bank(3), "bank"),
        ("plain rho", stage_plain_rho, None),
        ("rho bank again", stage_rho_bank, "rho_bank")]


def stale_calls(be, mo, mode):
    """Every bank call whose mode the handle is not in: RuntimeError, nothing launched."""
    x = torch.zeros((2, B, T), dtype=torch.float32, device="cuda")
    block, st = np.zeros((1, 3), np.float32), torch.zeros(64, dtype=torch.uint8, device="cuda")
    psi = [("bank_forward", lambda: be.bank_forward(x, save_for_bwd=True)), ("bank_backward", be.bank_backward),
           ("bank_grad_status", be.bank_grad_status), ("bank_stream_state", lambda: be.bank_stream_state(2)),
           ("bank_stream", lambda: be.bank_stream(None, st, 0, block, None, n=2)),
           ("bank_stream_score", lambda: be.bank_stream_score(None, st, 0, block, n=2))]
    rho = [("rho_bank_forward", lambda: be.rho_bank_forward(x, save_for_bwd=True)), ("rho_bank_backward", be.rho_bank_backward)]
    be.kernel_times()                                                # (what the stage itself launched)
    for name, call in (psi if mode != "bank" else []) + (rho if mode != "rho_bank" else []):
        with pytest.raises(RuntimeError) as e:
            call()
        assert not isinstance(e.value, _capi.CmpsError), (name, str(e.value))       # refused on the host: the C ABI was not asked
        assert name + "() needs " in str(e.value), (name, str(e.value))
        assert be.kernel_times() == {}, name


_FRESH = {}


def fresh(D, shared):
    """Every stage of WALK on a fresh HipScan of its own, computed once per (D, shared)."""
    from audio_mps_amd.scan import HipScan
    if (D, shared) not in _FRESH:
        mo = Models(D)
        _FRESH[(D, shared)] = (mo, [stage(HipScan(D), mo, shared) for _, stage, _ in WALK])
    return _FRESH[(D, shared)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared-audio", "own-audio"])
@pytest.mark.parametrize("D", [4, 20])
def test_one_handle_walked_through_its_modes(D, shared):
    from audio_mps_amd.scan import HipScan
    mo, want = fresh(D, shared)
    be = HipScan(D)
    be.kernel_events(True)
    stale_calls(be, mo, None)                                        # a handle that never held a bank
    for (name, stage, mode), ref in zip(WALK, want):
        loss, grad = stage(be, mo, shared)
        assert np.isfinite(loss).all() and np.isfinite(grad).all(), name
        assert loss.shape == ref[0].shape and grad.shape == ref[1].shape, name
        assert same(loss, ref[0]), (name, loss, ref[0])
        assert same(grad, ref[1]), name
        stale_calls(be, mo, mode)
    # (the members and the stages do differ: equal bits are no accident of equal inputs)
    assert not same(want[1][0][0], want[1][0][1]) and not same(want[1][0], want[2][0]) and not same(want[1][1][0], want[1][1][1])


# ---- refusals of the stream and score entries: (arguments that differ from a good call, code, message behind "<entry>: ") ----
OK, BAD, STATE, WS = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE, _capi.CMPS_ERR_WORKSPACE
NEED = "need n >= 1, forced >= 0, length >= 0, forced + length >= 1 and k0 >= 0"
NEED_SCORE = "need n >= 1, forced >= 1 and k0 >= 0"
START = "state_in_dev is NULL exactly at the start of a stream (k0 == 0)"
CLIPS = "n_audio must be n, or 1 for one clip shared by every path"
ROWS_AUDIO = "n_audio must be 1 (one signal for every path of every member), n (shared by the members) or M * n"
ROWS_NOISE = "n_noise must be n (every member hears the same noise) or M * n"
EXTENT = "M * n * (forced + length) exceeds 2^31 - 1"
TABLE = "k0 + forced + length + 1 = 9 exceeds T = 8 of cmps_set_params (the per-step tables): needs T >= 9"
TABLE_10 = "k0 + forced + length + 1 = 10 exceeds T = 8 of cmps_set_params (the per-step tables): needs T >= 10"
TABLE_SCORE = "k0 + forced + 1 = 9 exceeds T = 8 of cmps_set_params (the per-step tables): needs T >= 9"
NO_PSI = "call cmps_set_params first (not available in legacy mode)"
NO_RHO = "call cmps_set_params and cmps_rho_set_state first (not available in legacy mode)"
NO_BANK = "needs a PsiCMPS bank (call cmps_bank_set_params_dev first)"
IS_BANK = "the handle holds a bank (cmps_bank_set_params_dev / cmps_rho_bank_set_state_dev); call cmps_set_params for one model first"
BANK_OPTIONS = "a bank runs with the default CMPS_OPT_RANK1, CMPS_OPT_BWD_WAVES and CMPS_OPT_F16_SCALE_SHIFT only"
X = "x"                                                              # stands for the one device buffer behind every pointer


def stream_refusals(clips, bank):
    rows = [(dict(n=0), NEED), (dict(forced=-1), NEED), (dict(length=-1), NEED), (dict(forced=0, length=0), NEED), (dict(k0=-1, state_in=X), NEED),
            (dict(state_in=X), START), (dict(k0=1), START), (dict(audio=None), "forced > 0 needs audio_dev"),
            (dict(noise=None), "length > 0 needs noise_dev and out_dev"), (dict(out=None), "length > 0 needs noise_dev and out_dev"),
            (dict(n_audio=3), clips), (dict(n_audio=0), clips)]
    if bank:
        rows += [(dict(n_noise=1), ROWS_NOISE), (dict(n_noise=3), ROWS_NOISE), (dict(n=2 ** 30, forced=1, length=0), EXTENT)]
    rows += [(dict(forced=4, length=4), TABLE), (dict(state_in=X, k0=5), TABLE_10),
             # the first failing check speaks
             (dict(n=0, state_in=X, audio=None), NEED), (dict(state_in=X, audio=None, n_audio=3), START),
             (dict(audio=None, noise=None, n_audio=3), "forced > 0 needs audio_dev"), (dict(out=None, n_audio=3, forced=4, length=4), "length > 0 needs noise_dev and out_dev"),
             (dict(n_audio=3, forced=4, length=4), clips)]
    if bank:
        rows += [(dict(n_audio=3, n_noise=3), ROWS_AUDIO), (dict(n_noise=3, forced=4, length=4), ROWS_NOISE),
                 (dict(n=2 ** 30, forced=4, length=4, n_audio=1, n_noise=2 ** 30), EXTENT)]
    return [(kw, BAD, text) for kw, text in rows]


def score_refusals(clips, loss_text, bank):
    rows = [(dict(n=0), NEED_SCORE), (dict(forced=0), NEED_SCORE), (dict(k0=-1, state_in=X), NEED_SCORE), (dict(state_in=X), START), (dict(k0=1), START),
            (dict(audio=None), "needs audio_dev"), (dict(loss=None), loss_text), (dict(n_audio=3), clips), (dict(n_audio=0), clips)]
    if bank:
        rows += [(dict(n=2 ** 30, forced=1), EXTENT)]
    rows += [(dict(forced=8), TABLE_SCORE),
             (dict(forced=0, state_in=X, audio=None), NEED_SCORE), (dict(state_in=X, audio=None, loss=None), START),
             (dict(audio=None, loss=None, n_audio=3), "needs audio_dev"), (dict(loss=None, n_audio=3, forced=8), loss_text), (dict(n_audio=3, forced=8), clips)]
    if bank:
        rows += [(dict(n=2 ** 30, forced=8), EXTENT)]
    return [(kw, BAD, text) for kw, text in rows]


PER_PATH, PER_MEMBER = "needs loss_dev (the running loss per path)", "needs loss_dev (the running loss per member and path)"
ARGUMENTS = {"cmps_psi_stream": stream_refusals(CLIPS, False), "cmps_rho_stream": stream_refusals(CLIPS, False),
             "cmps_bank_stream": stream_refusals(ROWS_AUDIO, True),
             "cmps_psi_stream_score": score_refusals(CLIPS, PER_PATH, False), "cmps_rho_stream_score": score_refusals(CLIPS, PER_PATH, False),
             "cmps_bank_stream_score": score_refusals(ROWS_AUDIO, PER_MEMBER, True)}
PSI, RHO, BANKED = ("cmps_psi_stream", "cmps_psi_stream_score"), ("cmps_rho_stream", "cmps_rho_stream_score"), ("cmps_bank_stream", "cmps_bank_stream_score")


def test_every_refusal_of_the_stream_and_score_entries():
    from audio_mps_amd.scan import HipScan
    D, M, n, T_ = 4, 2, 2, 8
    mo = Models(D)
    be = HipScan(D)
    lib, h = be._lib, be._h
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")     # behind every pointer: no refused call looks at it
    x = buf.data_ptr()
    be.kernel_events(True)

    def call(entry, save=0, **kw):
        a = dict(state_in=None, state_out=X, k0=0, audio=X, n_audio=1, forced=2, noise=X, n_noise=n, length=2, n=n, out=X, pred=None, nll=X, loss=X)
        a.update(kw)
        a = {k: (x if v is X else v) for k, v in a.items()}
        head = (h, a["state_in"], a["state_out"], a["k0"], a["audio"], a["n_audio"], a["forced"])
        if entry.endswith("_score"):
            tail = (a["n"], a["nll"], a["loss"], a["pred"])
        else:
            tail = (a["noise"],) + ((a["n_noise"],) if entry == "cmps_bank_stream" else ()) + (a["length"], a["n"], a["out"], a["pred"])
        return getattr(lib, entry)(*head, *tail, *((save,) if "_rho_" in entry else ()), None)

    def refused(entry, want, text, **kw):
        code = call(entry, **kw)
        assert (code, lib.cmps_last_error(h).decode()) == (want, f"{entry}: {text}"), kw
        assert be.kernel_times() == {}, (entry, kw)                  # no kernel ran

    def arguments(entries):
        be.kernel_times()                                            # (what the set-up launched)
        for entry in entries:
            for kw, want, text in ARGUMENTS[entry]:
                refused(entry, want, text, **kw)

    # a fresh handle: the call order speaks before any argument
    for entry, text in zip(PSI + RHO + BANKED, (NO_PSI,) * 2 + (NO_RHO,) * 2 + (NO_BANK,) * 2):
        refused(entry, STATE, text)
        refused(entry, STATE, text, n=0, audio=None, n_audio=3)
    # one plain model
    be.set_params(mo.eff[0], n, T_, train=False)
    arguments(PSI)
    for entry, text in zip(RHO + BANKED, (NO_RHO,) * 2 + (NO_BANK,) * 2):
        refused(entry, STATE, text, n=0)
    # ... with the columns of rho_0, in a workspace without the training sections
    be.rho_set_state(mo.cols[0], n, T_, train=False)
    arguments(RHO)
    refused("cmps_rho_stream", WS, "save_states needs a CMPS_WS_TRAIN rho workspace with B_max*(T-1) >= n*(forced+length)", save=1)
    refused("cmps_rho_stream_score", WS, "save_states needs a CMPS_WS_TRAIN rho workspace with B_max*(T-1) >= n*forced", save=1)
    refused("cmps_rho_stream", BAD, CLIPS, save=1, n_audio=3)       # (the arguments first)
    # a PsiCMPS bank
    be.bank_set_params(mo.eff[:M], n, T_)
    arguments(BANKED)
    for entry, text in zip(PSI + RHO, (IS_BANK,) * 2 + (NO_RHO,) * 2):
        refused(entry, STATE, text, n=0)
    be.set_rank1(_capi.CMPS_RANK1_BF16X2)
    for entry in BANKED:
        refused(entry, STATE, BANK_OPTIONS, n=0)
    be.set_rank1(_capi.CMPS_RANK1_DEFAULT)
    # the handle is as usable as before: one good call of each bank entry, then legacy mode
    st = be.bank_stream_state(n)
    out, nll, loss = x + 4096, x + 8192, x + 12288                  # (what a good call writes, apart from what it reads)
    assert call("cmps_bank_stream", state_out=st.data_ptr(), out=out) == OK, lib.cmps_last_error(h).decode()
    assert call("cmps_bank_stream_score", state_in=st.data_ptr(), state_out=st.data_ptr(), k0=4, nll=nll, loss=loss) == OK, lib.cmps_last_error(h).decode()
    assert list(be.kernel_times()) == ["k_sample_wave_stream", "k_sample_wave_score"]
    be.legacy_set_params(mo.R, mo.Q, mo.hp.delta_t, n, T_, train=False)
    be.kernel_times()
    for entry, text in zip(PSI + RHO + BANKED, (NO_PSI,) * 2 + (NO_RHO,) * 2 + (NO_BANK,) * 2):
        refused(entry, STATE, text, n=0)
