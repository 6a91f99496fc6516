"""The memory contract of the C ABI (include/cmps.h) on a real MI355X: all device memory is the caller's, a workspace of exactly
cmps_workspace_bytes() / cmps_rho_workspace_bytes() bytes is enough, without CMPS_WS_REUSE_TABLES every call rebuilds every table.
(The fourth promise, "asynchronously on the caller's stream", is tests/test_gpu_caller_stream.py.)

Every buffer an entry takes is a tests/_guard.py::Guarded: exactly as long as include/cmps.h says, between two pattern-filled zones of
max(64 KiB, its own size), the payload itself pattern-filled too.  Every case runs twice, the pattern being the quiet NaN 0x7FC5A5A5 and
0x00000000.  After every entry: CMPS_OK, every zone of every buffer intact, every const input unchanged; at the end no element of a
documented output keeps the NaN pattern, and the outputs of the NaN-filled and the zero-filled run are bit-identical (the library has no
floating-point atomics), so nothing the result depends on was read from memory this call sequence did not write.

Anchors, so that two equally wrong runs cannot pass: the driver's result is bit-identical to the same calls through HipScan, and meets
the project's own bars against the existing oracles -- LOSS_BAR / GRAD_BAR / _dA_bar of tests/_sweep.py against the float32 C restatement
(the bf16 pair kernels: sweep_pair's bars against the bf16-emulating oracle, the only oracle that family has; legacy: sweep_legacy's),
rho against O.rho_loss_and_grads(f64t32) with the elastic bar of sweep_rho, samplers against the compositions of tests/_primed_ref.py,
_stream_ref.py, _rho_primed_ref.py, _rho_stream_ref.py at the bars of their tests (psi: tests/test_gpu_primed.py, test_gpu_stream.py; rho:
tests/test_gpu_rho_primed.py, test_gpu_rho_stream.py; at D = 72 the composition anchors a short case, see there).  No tolerance is new.

Inputs: sigma = 0.36, A = 66, audio x 0.09, Rx, Ry x 0.69 (x 0.5 above D = 32), where Q = -(dt sigma^2 / 2) R^dagger R is visible in
float32 (tests/_guard.py); every case's oracle losses are asserted finite before the case counts.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cmps_oracle as O, c_oracle as C
import _guard as G
import _primed_ref as PR
import _rho_primed_ref as RPR
import _rho_stream_ref as RSR
import _stream_ref as SR
from _sweep import GRAD_BAR, LOSS_BAR, PAIR_GRAD_BAR, PAIR_LOSS_BAR, _dA_bar, _loss_err
from _util import c_oracle_run, oracle_hparams, oracle_variables, rel_inf

pytestmark = pytest.mark.gpu

AUTO, BLOCK, WAVE, PAIR, WAVE32, WIDE = 0, 1, 2, 3, 4, 5
OPT_RANK1, OPT_WIDE_CHAIN, OPT_RHO_BWD, OPT_BWD_WAVES = 1, 3, 5, 6
OUT_RTOL = 2e-5                                      # tests/test_gpu_primed.py, test_gpu_stream.py: out against the float32 composition


def opts(**kw):
    names = {"rank1": OPT_RANK1, "chain": OPT_WIDE_CHAIN, "rho_bwd": OPT_RHO_BWD, "waves": OPT_BWD_WAVES}
    return tuple((names[k], v) for k, v in kw.items())


def both_fills(run, what=""):
    """run(fill) -> {name: bytes}; the NaN-filled and the zero-filled run must agree bit for bit.  Returns the NaN-filled one."""
    a, b = run(G.NAN_FILL), run(G.ZERO_FILL)
    G.same_bits(a, b, f"{what}: NaN-filled against zero-filled buffers")
    return a


def as_f32(res, name, shape=(-1,)):
    return res[name].view(np.float32).reshape(shape)


# ---------------------------------------------------------------------------------------------------
# oracles, once per shape
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def psi_oracle(D, B, T, seed=3):
    m, audio = G.psi_model(D, B), G.contract_audio(B, T, seed)
    ref = c_oracle_run(m, audio, "f32")
    assert np.all(np.isfinite(ref["loss_per_clip"])), ("the oracle's losses are not finite: not a case", D, B, T)
    return ref, C.unpack_grad(ref["grad"], D), C.unpack_grad(c_oracle_run(m, audio, "f64t32")["grad"], D)


def check_psi_against_oracle(res, D, B, T, bf16x2=False, tag="", seed=3):
    from audio_mps_amd.scan import unpack_grad
    ref, gr, gt = psi_oracle(D, B, T, seed)
    per, g = as_f32(res, "loss" + tag), unpack_grad(as_f32(res, "grad" + tag), D)
    assert _loss_err(per, ref["loss_per_clip"]) <= LOSS_BAR, (D, B, T, _loss_err(per, ref["loss_per_clip"]))
    for k in ("Rbar", "fbar", "psi0bar"):
        assert rel_inf(g[k], gr[k]) <= GRAD_BAR * (2 if bf16x2 else 1), (D, B, T, k, rel_inf(g[k], gr[k]))
    assert rel_inf(g["Abar"], gr["Abar"]) <= _dA_bar(gr["Abar"], gt["Abar"], GRAD_BAR), (D, B, T, "dA")
    assert abs(float(g["loss_sum"]) - float(np.sum(per, dtype=np.float64))) <= 1e-5 * abs(float(g["loss_sum"]))    # (tests/test_gpu_parity.py)


def set_options(be, options):
    """cmps_set_option on a HipScan's handle, checked."""
    from audio_mps_amd import _capi
    for o, v in options:
        _capi.check(be._h, be._lib.cmps_set_option(be._h, o, v))


def hipscan_psi(D, variant, options, B, T):
    """The same calls through HipScan (torch.empty buffers): loss, grad, states as raw bytes."""
    from audio_mps_amd.scan import HipScan
    be = HipScan(D, variant=variant)
    set_options(be, options)
    m = G.psi_model(D, B)
    be.set_params(m.effective_params(), B, T, train=True)
    audio = torch.from_numpy(G.contract_audio(B, T)).to(be.device)
    loss = be.forward(audio, save_for_bwd=True)
    grad = be.backward()
    out = {"loss": loss.cpu().numpy().view(np.uint8), "grad": grad.cpu().numpy().view(np.uint8)}
    st = be.states()
    out["states"] = np.stack([st.real, st.imag], axis=-1).astype(np.float32).reshape(-1).view(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------
# 1. the pure-state families: set_params -> fwd(save) -> bwd -> grad_status -> states
# ---------------------------------------------------------------------------------------------------
WAVE_OPTS = [opts(waves=w, rank1=r) for w in (1, 2) for r in (0, 1, 2, 3)]
WIDE_OPTS = [opts(chain=c, rank1=r) for c in (0, 1, 2) for r in (1, 2, 3, 4)]
# (family, variant, the variant it must resolve to, D, B values, T values, option sets)
PSI_ROWS = [("wave16", AUTO, WAVE, D, (1, 5), (2, 9, 66), [()]) for D in (3, 16)] + \
           [("wave", WAVE, WAVE, D, (1, 5), (2, 33, 66, 130), WAVE_OPTS) for D in (17, 32)] + \
           [("wave32", WAVE32, WAVE32, 9, (3,), (47,), [()])] + \
           [("wide", AUTO, WIDE, D, (1, 3), (2, 5, 66, 130), WIDE_OPTS) for D in (33, 96, 128)] + \
           [("pair", PAIR, PAIR, D, (3,), (65,), [()]) for D in (40, 128)] + \
           [("block", BLOCK, BLOCK, D, (3,), (66,), [()]) for D in (5, 48)]
PSI_CASES = [pytest.param(fam, v, rv, D, B, Ts, os, id=f"{fam}-D{D}-B{B}") for fam, v, rv, D, Bs, Ts, os in PSI_ROWS for B in Bs]


def run_psi(fill, D, variant, options, B_max, T, audio, resolved=None, train=True, bwd=True, states=True):
    drv = G.Driver(D, fill, variant, options)
    if resolved is not None:
        assert drv.variant == resolved
    G.set_params(drv, G.psi_model(D, B_max), B_max, T, train=train)
    names = G.psi_scan(drv, audio, save=train, bwd=bwd, states=states)
    if bwd:
        code, sticky = drv.grad_status()
        assert (code, sticky) == (0, 0), ("cmps_psi_grad_status", code, sticky)
    drv.finish()
    res = drv.result(names)
    drv.close()
    return res


@functools.lru_cache(maxsize=None)
def pair_oracle(D, B, T, seed=3):
    m, audio = G.psi_model(D, B), G.contract_audio(B, T, seed)
    em = O.psi_bf16_scan(oracle_hparams(m.hparams), oracle_variables(m), audio)
    assert np.all(np.isfinite(em["loss_per_clip"])), ("the oracle's losses are not finite: not a case", D, B, T)
    return em


def check_pair_against_oracle(res, D, B, T, seed=3):
    from audio_mps_amd.scan import unpack_grad
    em = pair_oracle(D, B, T, seed)
    per, g = as_f32(res, "loss"), unpack_grad(as_f32(res, "grad"), D)
    assert _loss_err(per, em["loss_per_clip"]) <= PAIR_LOSS_BAR
    for k in ("Rbar", "fbar", "psi0bar"):
        assert rel_inf(g[k], em[k]) <= PAIR_GRAD_BAR, (D, k, rel_inf(g[k], em[k]))
    assert rel_inf(g["Abar"], em["Abar"]) <= 10 * PAIR_GRAD_BAR


@pytest.mark.parametrize("family,variant,resolved,D,B,Ts,option_sets", PSI_CASES)
def test_psi_train_sequence(family, variant, resolved, D, B, Ts, option_sets):
    for T in Ts:
        audio = G.contract_audio(B, T)
        for options in option_sets:
            res = both_fills(lambda fill: run_psi(fill, D, variant, options, B, T, audio, resolved), f"{family} D={D} B={B} T={T} {options}")
            if family == "pair":
                check_pair_against_oracle(res, D, B, T)
            else:
                check_psi_against_oracle(res, D, B, T, bf16x2=(family == "wide" and dict(options).get(OPT_RANK1) == 1))
            if T == Ts[-1]:
                G.same_bits(res, hipscan_psi(D, variant, options, B, T), f"{family} D={D}: guarded driver against HipScan")


# ---------------------------------------------------------------------------------------------------
# legacy arithmetic (wave, wide, block): legacy tables, no time table, no cmps_psi_states / cmps_psi_grad_status in this mode
# ---------------------------------------------------------------------------------------------------
def check_legacy_against_oracle(res, m, audio):
    """The checks of tests/_sweep.py::sweep_legacy."""
    ref = O.legacy_loss_and_grads(m.variables["H"], m.variables["R"], m.delta_t, audio, "f32")
    assert np.all(np.isfinite(ref["per_clip"])), "the oracle's losses are not finite: not a case"
    assert _loss_err(as_f32(res, "loss"), ref["per_clip"]) <= LOSS_BAR
    _, grads = m.chain_rule(as_f32(res, "grad"), audio.shape[0])
    assert max(rel_inf(grads["R"], ref["gR"]), rel_inf(grads["H"], ref["gH"])) <= GRAD_BAR


def run_legacy(fill, D, variant, B, T, audio):
    drv = G.Driver(D, fill, variant)
    G.legacy_set_params(drv, G.legacy_model(D, B), B, T)
    names = G.legacy_scan(drv, audio)
    drv.finish()
    res = drv.result(names)
    drv.close()
    return res


@pytest.mark.parametrize("D,variant", [(12, AUTO), (40, AUTO), (40, BLOCK)])
def test_legacy_train_sequence(D, variant):
    from audio_mps_amd import layout
    from audio_mps_amd.scan import HipScan
    from _util import make_audio
    B, T = 3, 65
    m = G.legacy_model(D, B)
    audio = make_audio(B, T, m.delta_t, 303, noise=0.05)
    res = both_fills(lambda fill: run_legacy(fill, D, variant, B, T, audio), f"legacy D={D}")
    check_legacy_against_oracle(res, m, audio)
    be = HipScan(D, variant=variant)
    be.legacy_set_params(m.variables["R"], m.Q, m.delta_t, B, T)
    loss = be.legacy_forward(torch.from_numpy(audio).to(be.device), save_for_bwd=True)
    grad = be.legacy_backward()
    assert grad.numel() == layout.size(layout.legacy_grad_fields(D))
    G.same_bits(res, {"loss": loss.cpu().numpy().view(np.uint8), "grad": grad.cpu().numpy().view(np.uint8)}, "legacy: driver against HipScan")


# ---------------------------------------------------------------------------------------------------
# RhoCMPS: set_params -> rho_set_state -> fwd(save) -> bwd -> rho_states
# ---------------------------------------------------------------------------------------------------
RHO_SHAPES = [(8, 3), (24, 12), (32, 32), (32, 11), (40, 5), (72, 72)]


def rho_T(D, rank):
    return (2, 12) if (D, rank) == (72, 72) else (2, 40)


def run_rho(fill, D, rank, options, B_max, T, audio, variant=AUTO, train=True, bwd=True, states=True):
    drv = G.Driver(D, fill, variant, options)
    m = G.rho_model(D, rank, B_max)
    G.set_params(drv, m, B_max, T, train=False)                   # (as RhoCMPS._prepare: the main workspace holds the tables only)
    G.rho_set_state(drv, m, B_max, T, train=train)
    names = G.rho_scan(drv, audio, save=train, bwd=bwd, states=states)
    drv.finish()
    res = drv.result(names)
    drv.close()
    return res


@functools.lru_cache(maxsize=None)
def rho_oracle(D, rank, B, T, seed=3):
    m, audio = G.rho_model(D, rank, B), G.contract_audio(B, T, seed)
    ohp, ov, Wx, Wy = RPR.oracle_side(m)
    f64 = np.float64
    ref, ref64 = (O.rho_loss_and_grads(ohp, ov.astype(f64), Wx.astype(f64), Wy.astype(f64), audio, d) for d in ("f64t32", "f64"))
    assert np.all(np.isfinite(ref["per_clip"])), ("the oracle's losses are not finite: not a case", D, rank, B, T)
    return ref, ref64, O.rho_loss_and_grads(ohp, ov, Wx, Wy, audio, "f32")


def check_rho_against_oracle(res, D, rank, B, T, seed=3):
    """The checks of tests/_sweep.py::sweep_rho: loss, every gradient tensor and dA at their elastic bars (and the f64-anchored check
    wherever the re-anchored bar is the wider)."""
    ref, ref64, ref32 = rho_oracle(D, rank, B, T, seed)
    m = G.rho_model(D, rank, B)
    per = as_f32(res, "loss")
    assert _loss_err(per, ref["per_clip"]) <= LOSS_BAR, (D, rank, B, T, _loss_err(per, ref["per_clip"]))
    _, grads = m.chain_rule(as_f32(res, "grad"), B)
    for k in ("Rx", "Ry", "freqs", "Wx", "Wy"):
        e, bar = rel_inf(grads[k], ref[k]), max(GRAD_BAR, 2.0 * rel_inf(ref32[k], ref[k]))
        e64, bar64 = rel_inf(grads[k], ref64[k]), max(GRAD_BAR, 2.0 * rel_inf(ref32[k], ref64[k]))
        assert e <= bar, (D, rank, B, T, k, e, bar)
        if bar > bar64:
            assert e64 <= bar64, (D, rank, B, T, k, "f64-anchored", e64, bar64)
    bar, bar64 = _dA_bar(ref32["A"], ref["A"], GRAD_BAR), _dA_bar(ref32["A"], ref64["A"], GRAD_BAR)
    assert rel_inf(grads["A"], ref["A"]) <= bar, (D, rank, B, T, "dA")
    if bar > bar64:
        assert rel_inf(grads["A"], ref64["A"]) <= bar64, (D, rank, B, T, "dA f64-anchored")


def hipscan_rho(D, rank, options, B, T):
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    set_options(be, options)
    m = G.rho_model(D, rank, B)
    be.set_params(m.effective_params(), B, T, train=False)
    be.rho_set_state(m.columns(), B, T, train=True)
    loss, grad = be.rho_loss_and_grad_sums(torch.from_numpy(G.contract_audio(B, T)).to(be.device))
    out = {"loss": loss.cpu().numpy().view(np.uint8), "grad": grad.cpu().numpy().view(np.uint8)}
    rho, pur = be.rho_states(B, T - 1, want_rho=True, want_purity=True)
    out["rho_states"] = np.stack([rho.real, rho.imag], axis=-1).astype(np.float32).reshape(-1).view(np.uint8)
    out["purity"] = pur.reshape(-1).view(np.uint8)
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D,rank", RHO_SHAPES)
def test_rho_train_sequence(D, rank, B):
    from audio_mps_amd import layout
    for T in rho_T(D, rank):
        audio = G.contract_audio(B, T)
        for options in ([opts(rho_bwd=0), opts(rho_bwd=1)] if D <= 32 else [()]):
            res = both_fills(lambda fill: run_rho(fill, D, rank, options, B, T, audio), f"rho ({D}, {rank}) B={B} T={T} {options}")
            g = layout.unpack(layout.grad_fields(D, rank), as_f32(res, "grad"))
            for k in ("psi0_re", "psi0_im"):                      # include/cmps.h: "2*D unused zeros"
                assert np.array_equal(g[k].view(np.uint32), np.zeros(D, np.uint32)), (k, g[k])
            check_rho_against_oracle(res, D, rank, B, T)
            if T == rho_T(D, rank)[-1]:
                G.same_bits(res, hipscan_rho(D, rank, options, B, T), f"rho ({D}, {rank}): guarded driver against HipScan")


# ---------------------------------------------------------------------------------------------------
# forward only: a CMPS_WS_FWD_ONLY workspace of its own, exact size
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,variant,D", [("wave16", AUTO, 16), ("wave", WAVE, 32), ("wave32", WAVE32, 9), ("wide", AUTO, 96),
                                              ("pair", PAIR, 40), ("block", BLOCK, 48)])
def test_forward_only_workspace(family, variant, D):
    B, T = 3, 66
    audio = G.contract_audio(B, T)
    res = both_fills(lambda fill: run_psi(fill, D, variant, (), B, T, audio, train=False, bwd=False, states=False), f"{family} forward only")
    per = as_f32(res, "loss")
    if family == "pair":
        assert _loss_err(per, pair_oracle(D, B, T)["loss_per_clip"]) <= PAIR_LOSS_BAR
    else:
        assert _loss_err(per, psi_oracle(D, B, T)[0]["loss_per_clip"]) <= LOSS_BAR


@pytest.mark.parametrize("D,variant", [(12, AUTO), (40, AUTO), (40, BLOCK)])
def test_forward_only_workspace_legacy(D, variant):
    from _util import make_audio
    B, T = 3, 65
    m = G.legacy_model(D, B)
    audio = make_audio(B, T, m.delta_t, 303, noise=0.05)

    def run(fill):
        drv = G.Driver(D, fill, variant)
        G.legacy_set_params(drv, m, B, T, train=False)
        names = G.legacy_scan(drv, audio, save=False, bwd=False)
        drv.finish()
        return drv.result(names)
    res = both_fills(run, "legacy forward only")
    ref = O.legacy_loss_and_grads(m.variables["H"], m.variables["R"], m.delta_t, audio, "f32")
    assert _loss_err(as_f32(res, "loss"), ref["per_clip"]) <= LOSS_BAR


@pytest.mark.parametrize("D,rank", [(24, 12), (40, 5)])
def test_forward_only_workspace_rho(D, rank):
    B, T = 3, 40
    audio = G.contract_audio(B, T)
    res = both_fills(lambda fill: run_rho(fill, D, rank, (), B, T, audio, train=False, bwd=False, states=False), "rho forward only")
    assert _loss_err(as_f32(res, "loss"), rho_oracle(D, rank, B, T)[0]["per_clip"]) <= LOSS_BAR


# ---------------------------------------------------------------------------------------------------
# B < B_max: a workspace that saw B_max loud clips, then B different clips -- against a workspace that never saw the first batch
# ---------------------------------------------------------------------------------------------------
def loud_audio(B, T):
    return (G.contract_audio(B, T, seed=29) * np.float32(3.0)).astype(np.float32)


@pytest.mark.parametrize("family,variant,D,T", [("wave16", AUTO, 16, 66), ("wave", WAVE, 32, 66), ("wave32", WAVE32, 9, 47), ("wide", AUTO, 33, 66),
                                                ("pair", PAIR, 40, 65), ("block", BLOCK, 48, 66)])
def test_smaller_batch_in_a_used_workspace(family, variant, D, T):
    B_max, B = 5, 2
    small = G.contract_audio(B, T, seed=5)

    def run(fill, dirty):
        drv = G.Driver(D, fill, variant)
        G.set_params(drv, G.psi_model(D, B_max), B_max, T)
        if dirty:
            G.psi_scan(drv, loud_audio(B_max, T), tag="_first")
        names = G.psi_scan(drv, small)
        assert drv.grad_status()[0] == 0
        drv.finish()
        return drv.result(names)
    clean = both_fills(lambda fill: run(fill, False), f"{family}: B = 2 of B_max = 5, unused workspace")
    if family == "pair":
        check_pair_against_oracle(clean, D, B, T, seed=5)
    else:
        check_psi_against_oracle(clean, D, B, T, seed=5)
    dirty = both_fills(lambda fill: run(fill, True), f"{family}: B = 2 of B_max = 5, used workspace")
    G.same_bits(dirty, clean, f"{family}: B = 2 behind a B_max = 5 batch against an unused workspace")


@pytest.mark.parametrize("D,variant", [(12, AUTO), (40, AUTO), (40, BLOCK)])
def test_smaller_batch_in_a_used_workspace_legacy(D, variant):
    from _util import make_audio
    B_max, B, T = 5, 2, 65
    m = G.legacy_model(D, B_max)
    first, small = make_audio(B_max, T, m.delta_t, 311, noise=0.05) * np.float32(3), make_audio(B, T, m.delta_t, 313, noise=0.05)

    def run(fill, dirty):
        drv = G.Driver(D, fill, variant)
        G.legacy_set_params(drv, m, B_max, T)
        if dirty:
            G.legacy_scan(drv, first, tag="_first")
        names = G.legacy_scan(drv, small)
        drv.finish()
        return drv.result(names)
    clean = both_fills(lambda fill: run(fill, False))
    check_legacy_against_oracle(clean, m, small)
    G.same_bits(both_fills(lambda fill: run(fill, True)), clean, "legacy: B = 2 behind B_max = 5")


@pytest.mark.parametrize("D,rank,T", [(8, 3, 40), (32, 32, 40), (32, 11, 40), (40, 5, 40), (72, 72, 12)])
def test_smaller_batch_in_a_used_workspace_rho(D, rank, T):
    B_max, B = 3, 1
    small = G.contract_audio(B, T, seed=5)
    for options in ([opts(rho_bwd=0), opts(rho_bwd=1)] if D <= 32 else [()]):
        def run(fill, dirty):
            drv = G.Driver(D, fill, AUTO, options)
            m = G.rho_model(D, rank, B_max)
            G.set_params(drv, m, B_max, T, train=False)
            G.rho_set_state(drv, m, B_max, T)
            if dirty:
                G.rho_scan(drv, loud_audio(B_max, T), tag="_first")
            names = G.rho_scan(drv, small)
            drv.finish()
            return drv.result(names)
        clean = both_fills(lambda fill: run(fill, False))
        check_rho_against_oracle(clean, D, rank, B, T, seed=5)
        G.same_bits(both_fills(lambda fill: run(fill, True)), clean, f"rho ({D}, {rank}) {options}: B = 1 behind B_max = 3")


# ---------------------------------------------------------------------------------------------------
# table reuse
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 32, 48])
def test_tables_are_rebuilt_without_the_reuse_flag(D):
    """set_params, the whole workspace overwritten with the pattern, set_params again WITHOUT CMPS_WS_REUSE_TABLES: the documented safe
    default must give the bits of a first-time run."""
    B, T = 3, 66
    audio = G.contract_audio(B, T)

    def run(fill, poison):
        drv = G.Driver(D, fill)
        m = G.psi_model(D, B)
        G.set_params(drv, m, B, T)
        if poison:
            drv.bufs["ws"].refill_payload()
            G.set_params(drv, m, B, T)
        names = G.psi_scan(drv, audio)
        assert drv.grad_status() == (0, 0)
        drv.finish()
        return drv.result(names)
    first = both_fills(lambda fill: run(fill, False))
    again = both_fills(lambda fill: run(fill, True))
    G.same_bits(again, first, f"D={D}: set_params behind a poisoned workspace against a first-time run")
    check_psi_against_oracle(first, D, B, T)


@pytest.mark.parametrize("D", [8, 32, 48])
def test_legitimate_table_reuse(D):
    """The same workspace untouched, CMPS_WS_REUSE_TABLES set, T changed 66 -> 130 -> 66: each result against a fresh run at that T, and
    cmps_psi_grad_status (0, sticky 0) after every step -- the two flag words sit behind the stash and the slabs, so they move with T and
    cmps_set_params has to clear them where they now are."""
    B = 3

    def fresh(fill, T):
        drv = G.Driver(D, fill)
        G.set_params(drv, G.psi_model(D, B), B, T)
        names = G.psi_scan(drv, G.contract_audio(B, T))
        assert drv.grad_status() == (0, 0)
        drv.finish()
        return drv.result(names)

    def reused(fill):
        drv = G.Driver(D, fill)
        m = G.psi_model(D, B)
        drv.new("ws", G.ws_bytes(drv, B, 130, True))              # sized for the longer clips; the T = 66 layout is its prefix
        out = []
        for i, T in enumerate((66, 130, 66)):
            G.set_params(drv, m, B, T, reuse=i > 0)
            names = G.psi_scan(drv, G.contract_audio(B, T), tag=f"_{i}")
            assert drv.grad_status() == (0, 0), (i, T)              # the flag words move with T: they must start at zero there
            out.append({k[:-2]: v for k, v in drv.result(names).items()})
        drv.finish()
        return {f"{k}_{i}": v for i, o in enumerate(out) for k, v in o.items()}
    got = both_fills(reused)
    f66, f130 = both_fills(lambda fill: fresh(fill, 66)), both_fills(lambda fill: fresh(fill, 130))
    for i, ref in enumerate((f66, f130, f66)):
        G.same_bits({k: got[f"{k}_{i}"] for k in ref}, ref, f"D={D}: reuse step {i}")


# ---------------------------------------------------------------------------------------------------
# cmps_set_params_dev behind cmps_psi_apply_step(grad_sums = NULL)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 33])
def test_set_params_dev_equals_host_parameters(D):
    B, T = 3, 66
    audio = G.contract_audio(B, T)

    def run(fill):
        drv = G.Driver(D, fill)
        m = G.psi_model(D, B)
        G.apply_step(drv, m, None)
        n = G.ws_bytes(drv, B, T, True)
        drv.new("ws", n)
        p = m.effective_params()
        drv.call("cmps_set_params_dev", drv.bufs["params_out"], float(p.sigma), float(p.delta_t), T, B, 1, drv.bufs["ws"], n)
        drv.const.add("params_out")
        drv.bufs["params_out"].snapshot()
        names = G.psi_scan(drv, audio)
        drv.finish()
        return drv.result(names + ["params_out"])
    dev = both_fills(run, f"set_params_dev D={D}")
    host = both_fills(lambda fill: run_psi(fill, D, AUTO, (), B, T, audio))
    G.same_bits({k: dev[k] for k in host}, host, f"D={D}: cmps_set_params_dev against cmps_set_params")
    m = G.psi_model(D, B)
    assert np.array_equal(as_f32(dev, "params_out"), np.append(G.psi_param_array(m), np.float32(m.A)))


# ---------------------------------------------------------------------------------------------------
# one update step
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 40])
def test_update_ancilla(D):
    from audio_mps_amd.scan import HipScan
    B, t = 3, 0.37
    rng = np.random.default_rng(D)
    psi = (rng.standard_normal((B, D)) + 1j * rng.standard_normal((B, D))).astype(np.complex64)
    a = (rng.standard_normal((B, D, D)) + 1j * rng.standard_normal((B, D, D))).astype(np.complex64)
    rho = (a @ np.conj(np.swapaxes(a, 1, 2))).astype(np.complex64)
    rho /= np.trace(rho, axis1=1, axis2=2)[:, None, None]
    signal = (0.01 * rng.standard_normal(B)).astype(np.float32)
    m = G.psi_model(D, B)
    for fn, x, name in (("cmps_psi_update_ancilla", psi, "update_ancilla"), ("cmps_rho_update_ancilla", rho, "rho_update_ancilla")):
        def run(fill):
            drv = G.Driver(D, fill)
            G.set_params(drv, m, B, 2, train=False)
            names = G.ancilla(drv, fn, x, signal, t)
            drv.finish()
            return drv.result(names)
        res = both_fills(run, fn)
        be = HipScan(D)
        be.set_params(m.effective_params(), B, 2, train=False)
        ref = getattr(be, name)(x, signal, t)
        got = as_f32(res, "anc_out", x.shape + (2,))
        assert np.array_equal(got[..., 0], ref.real) and np.array_equal(got[..., 1], ref.imag), fn
        ohp, ov = oracle_hparams(m.hparams), oracle_variables(m)
        z = got[..., 0] + 1j * got[..., 1]
        if fn == "cmps_psi_update_ancilla":                     # the bars of test_update_ancilla_matches_oracle / test_rho_update_ancilla_matches_oracle
            R, freqs, _, _ = O.effective_params(ohp, ov)
            assert rel_inf(z, O.update_ancilla_psi(psi, signal, t, R, freqs, ov.A, ohp)) <= 1e-5
        else:
            assert rel_inf(z, O.rho_update_ancilla(ohp, ov, rho, signal, t)) <= 1e-5


# ---------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------
def sampler_model(D, n, backend=False):
    """The model of tests/_primed_ref.py / _stream_ref.py (sigma = 1, A = 10, R x 0.05), so that their compositions are the reference."""
    from audio_mps_amd import HParams, PsiCMPS
    m = PsiCMPS(HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0), seed=D, backend=backend)
    m.variables["Rx"] *= np.float32(0.05)
    m.variables["Ry"] *= np.float32(0.05)
    return m


PSI_SAMPLERS = [(8, WAVE), (32, WAVE), (48, AUTO), (128, WIDE), (48, BLOCK)]


SAMPLER_SHAPES = [(length, prime_T) for length in (65, 70) for prime_T in (2, 66)]
RHO_OUT_RTOL = 2e-4                                  # tests/test_gpu_rho_primed.py, test_gpu_rho_stream.py: out against max |float32 composition|


def pred_bar(p32, p64):
    """tests/test_gpu_primed.py, test_gpu_stream.py."""
    return 4.0 * float(np.max(np.abs(p32 - p64))) + 2e-6 * float(np.max(np.abs(p64)))


def rho_pred_bar(D, rank, p32, p64, delta_t):
    """tests/test_gpu_rho_primed.py, test_gpu_rho_stream.py."""
    return 4.0 * float(np.max(np.abs(p32.astype(np.float64) - p64))) + 8.0 * 2.0 ** -22 * RPR.R_fro(D, rank) * float(delta_t)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("D,variant", PSI_SAMPLERS)
def test_psi_samplers(D, variant, n):
    from audio_mps_amd.scan import HipScan
    m = sampler_model(D, n)
    for length, prime_T in SAMPLER_SHAPES:
        P = prime_T - 1
        prime, noise = PR.case_inputs(D, P, length, n)
        T = prime_T + length

        def run(fill, primed, n_prime):
            drv = G.Driver(D, fill, variant)
            G.set_params(drv, m, n, T, train=False)
            names = G.sample(drv, "cmps_psi_sample_primed" if primed else "cmps_psi_sample", noise,
                             prime=np.ascontiguousarray(prime[:n_prime]) if primed else None)
            drv.finish()
            return drv.result(names)
        plain = both_fills(lambda fill: run(fill, False, 0), f"cmps_psi_sample D={D}")
        primed = both_fills(lambda fill: run(fill, True, n), f"cmps_psi_sample_primed D={D}")
        shared = both_fills(lambda fill: run(fill, True, 1), f"cmps_psi_sample_primed n_prime=1 D={D}")
        # anchors: HipScan bit for bit, the oracle composition at the bars of tests/test_gpu_primed.py
        be = HipScan(D, variant=variant)
        be.set_params(m.effective_params(), n, T, train=False)
        o_h, p_h = be.sample_primed(prime, noise, want_pred=True)
        assert np.array_equal(as_f32(primed, "out", (n, length)), o_h) and np.array_equal(as_f32(primed, "pred", (n, P)), p_h)
        assert np.array_equal(as_f32(plain, "out", (n, length)), be.sample(noise))
        o1_h, p1_h = be.sample_primed(prime[:1], noise, want_pred=True)
        assert np.array_equal(as_f32(shared, "out", (n, length)), o1_h) and np.array_equal(as_f32(shared, "pred", (n, P)), p1_h)
        o32, p32 = PR.case_reference(D, P, length, n, "f32")
        _, p64 = PR.case_reference(D, P, length, n, "f64")
        assert float(np.max(np.abs(as_f32(primed, "out", (n, length)) - o32))) <= OUT_RTOL * max(1.0, float(np.max(np.abs(o32))))
        assert float(np.max(np.abs(as_f32(primed, "pred", (n, P)) - p64))) <= pred_bar(p32, p64)


RHO_SAMPLERS = [(8, 3, AUTO), (32, 32, AUTO), (40, 3, AUTO), (72, 72, AUTO)]


@pytest.mark.parametrize("D,rank,variant", RHO_SAMPLERS)
def test_rho_samplers(D, rank, variant):
    from audio_mps_amd.scan import HipScan
    n = 2
    m = RPR.case_model(D, rank, backend=False)
    # D = 72: the float32 and float64 compositions of the four shapes take 25 s in numpy; there the composition anchors a short case
    # (length 7, prime_T 6, the size of tests/_rho_primed_ref.py's (96, 96) case) and the four shapes keep guards and HipScan identity
    for length, prime_T in SAMPLER_SHAPES + ([(7, 6)] if D > 40 else []):
        P = prime_T - 1
        prime, noise = RPR.case_inputs(D, rank, P, length, n)
        T = prime_T + length

        def run(fill, primed, save):
            drv = G.Driver(D, fill, variant)
            G.set_params(drv, m, n, T, train=False)
            G.rho_set_state(drv, m, n, T, train=bool(save))
            names = G.sample(drv, "cmps_rho_sample_primed" if primed else "cmps_rho_sample", noise, prime=prime if primed else None,
                             flags=(save,))
            if save:
                names += G.rho_states(drv, n, (P if primed else 0) + length)
            drv.finish()
            return drv.result(names)
        be = HipScan(D, variant=variant)
        for save in (0, 1):
            plain = both_fills(lambda fill: run(fill, False, save), f"cmps_rho_sample ({D}, {rank}) save_states={save}")
            primed = both_fills(lambda fill: run(fill, True, save), f"cmps_rho_sample_primed ({D}, {rank}) save_states={save}")
            be.set_params(m.effective_params(), n, T, train=False)
            be.rho_set_state(m.columns(), n, T, train=bool(save))
            assert np.array_equal(as_f32(plain, "out", (n, length)), be.rho_sample(noise, save_states=bool(save)))
            o_h, p_h = be.rho_sample_primed(prime, noise, want_pred=True, save_states=bool(save))
            assert np.array_equal(as_f32(primed, "out", (n, length)), o_h) and np.array_equal(as_f32(primed, "pred", (n, P)), p_h)
            if save:
                pur = be.rho_states(n, P + length, want_rho=False, want_purity=True)
                assert np.array_equal(as_f32(primed, "purity", (n, P + length)), pur)
        if D > 40 and (length, prime_T) != (7, 6):
            continue
        o32, p32 = RPR.case_reference(D, rank, P, length, n, "f32")[:2]
        p64 = RPR.case_reference(D, rank, P, length, n, "f64")[1]
        assert float(np.max(np.abs(as_f32(primed, "out", (n, length)) - o32))) <= RHO_OUT_RTOL * float(np.max(np.abs(o32)))
        assert float(np.max(np.abs(as_f32(primed, "pred", (n, P)) - p64))) <= rho_pred_bar(D, rank, p32, p64, m.hparams.delta_t)


# ---------------------------------------------------------------------------------------------------
# resumable samplers: three segments (forced, sampled, mixed) on one exact-size record buffer; state_out == state_in in the second,
# state_out == NULL in the third; pred_dev a valid address at forced == 0 (second) and NULL with forced > 0 (third)
# ---------------------------------------------------------------------------------------------------
PLAN = ((65, 0), (0, 70), (2, 3))


def psi_carried(D, variant):
    """Floats a path's record carries (audio_mps_amd/csrc/cmps_internal.h): wave u [64], |y|^2 partial per lane [64], running sum | wide
    ut [2 DP], |y|^2 partial per wave [DP / 16], running sum | block u [2 D], running sum."""
    DP = (D + 31) // 32 * 32
    if variant == BLOCK:
        return 2 * D + 1
    return 129 if D <= 32 else 2 * DP + DP // 16 + 1


def rho_carried(D, rank, variant):
    """... of the RhoCMPS samplers: row-array kernel U [rank][64], running sum | block kernel S [rank][D] float2, running sum."""
    return 64 * rank + 1 if (variant != BLOCK and D <= 32 and rank <= 32) else 2 * rank * D + 1


def check_records(recs_nan, recs_zero, n, carried):
    """Every carried float of every record is written and agrees between the NaN-filled and the zero-filled run; what keeps the caller's
    bytes is exactly the rounding to a multiple of 16 bytes behind the carried floats (include/cmps.h says so)."""
    assert len(recs_nan) == len(recs_zero) == 2                 # the first two of the three segments write the record
    for (bytes_a, left), (bytes_b, _) in zip(recs_nan, recs_zero):
        per_path = left.reshape(n, -1)
        rec = per_path.shape[1]
        assert rec == (carried + 3) // 4 * 4, (rec, carried)
        assert not per_path[:, :carried].any(), ("carried floats of a record never written", np.nonzero(per_path[:, :carried]))
        assert per_path[:, carried:].all(), "the rounding behind the carried floats was written"
        a, b = bytes_a.reshape(n, rec, 4)[:, :carried], bytes_b.reshape(n, rec, 4)[:, :carried]
        assert np.array_equal(a, b), "state records of the NaN-filled and the zero-filled run differ"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("D,variant", PSI_SAMPLERS)
def test_psi_stream(D, variant, n):
    from test_gpu_stream import run_plan
    from audio_mps_amd.scan import HipScan
    m = sampler_model(D, n)
    clip, noise = SR.case_inputs(D, PLAN, n)
    F, L = SR.plan_steps(PLAN)
    recs = {}

    def run(fill):
        drv = G.Driver(D, fill, variant)
        G.set_params(drv, m, n, F + L + 1, train=False)
        names, recs[fill] = G.stream_plan(drv, "cmps_psi_stream", "cmps_psi_stream_state_bytes", PLAN, clip, noise, n)
        drv.finish()
        return drv.result(names)
    res = both_fills(run, f"cmps_psi_stream D={D}")
    check_records(recs[G.NAN_FILL], recs[G.ZERO_FILL], n, psi_carried(D, variant))
    out = np.concatenate([as_f32(res, f"seg_out_{i}", (n, s)) for i, (f, s) in enumerate(PLAN)], axis=1)
    m = sampler_model(D, n, backend=HipScan(D, variant=variant))
    o_h, p_h, _ = run_plan(m, PLAN, clip, noise, n)
    assert np.array_equal(out, o_h)
    assert np.array_equal(as_f32(res, "seg_pred_0", (n, 65)), p_h[:, :65]) and res["seg_pred_1"].size == 0      # (segment 2: pred_dev == NULL)
    o32, p32 = SR.case_reference(D, PLAN, n, "f32")
    _, p64 = SR.case_reference(D, PLAN, n, "f64")
    assert float(np.max(np.abs(out - o32))) <= OUT_RTOL * max(1.0, float(np.max(np.abs(o32))))
    assert float(np.max(np.abs(p_h - p64))) <= pred_bar(p32, p64)


SHORT_PLAN = ((3, 0), (0, 2), (2, 5))               # the same three kinds of segment at the size of tests/_rho_stream_ref.py's (96, 96) case


@pytest.mark.parametrize("D,rank,variant", RHO_SAMPLERS + [(32, 32, BLOCK)])
def test_rho_stream(D, rank, variant):
    """D = 72: the compositions of PLAN take 8 s in numpy; there PLAN keeps guards, records and HipScan identity and the composition
    anchors SHORT_PLAN, run the same way."""
    for plan, compose in ((PLAN, D <= 40), (SHORT_PLAN, True)) if D > 40 else ((PLAN, True),):
        rho_stream_case(D, rank, variant, plan, compose)


def rho_stream_case(D, rank, variant, plan, compose):
    from test_gpu_rho_stream import run_plan
    from audio_mps_amd.scan import HipScan
    n = 2
    m = RPR.case_model(D, rank, backend=False)
    clip, noise = RSR.case_inputs(D, rank, plan, n)
    F, L = SR.plan_steps(plan)
    longest = max(f + s for f, s in plan)
    recs = {}
    for save in (0, 1):
        def run(fill):
            drv = G.Driver(D, fill, variant)
            G.set_params(drv, m, n, F + L + 1, train=False)
            G.rho_set_state(drv, m, n, longest + 1, train=bool(save))   # its T is the stash's capacity: the longest segment
            names, recs[fill] = G.stream_plan(drv, "cmps_rho_stream", "cmps_rho_stream_state_bytes", plan, clip, noise, n, flags=(save,),
                                              states_steps=True if save else None)
            drv.finish()
            return drv.result(names)
        res = both_fills(run, f"cmps_rho_stream ({D}, {rank}) save_states={save}")
        check_records(recs[G.NAN_FILL], recs[G.ZERO_FILL], n, rho_carried(D, rank, variant))
    out = np.concatenate([as_f32(res, f"seg_out_{i}", (n, s)) for i, (f, s) in enumerate(plan)], axis=1)
    o_h, p_h = run_plan(RPR.case_model(D, rank, backend=HipScan(D, variant=variant)), plan, clip, noise, n)[:2]
    assert np.array_equal(out, o_h)
    f0 = plan[0][0]
    assert np.array_equal(as_f32(res, "seg_pred_0", (n, f0)), p_h[:, :f0]) and res["seg_pred_1"].size == 0      # (segment 2: pred_dev == NULL)
    if compose:
        o32, p32 = RSR.case_reference(D, rank, plan, n, "f32")[:2]
        p64 = RSR.case_reference(D, rank, plan, n, "f64")[1]
        assert float(np.max(np.abs(out - o32))) <= RHO_OUT_RTOL * float(np.max(np.abs(o32)))
        assert float(np.max(np.abs(p_h - p64))) <= rho_pred_bar(D, rank, p32, p64, m.hparams.delta_t)


# ---------------------------------------------------------------------------------------------------
# optimiser steps
# ---------------------------------------------------------------------------------------------------
def synthetic_grad_sums(D, rank=0, bad=False):
    """Gradient sums of the layout of cmps_psi_loss_bwd / cmps_rho_loss_bwd: finite values of ordinary size; bad: one Inf in the gradient
    part next to the finite loss sum (the skipped step)."""
    from audio_mps_amd import layout
    n = layout.grad_size(D, rank)
    g = (0.1 * np.random.default_rng(D + rank).standard_normal(n)).astype(np.float32)
    g[2 * D * D + 3 * D + 1] = np.float32(12.5)
    if bad:
        g[(n - 1) if rank else (D * D // 2)] = np.float32(np.inf)
    return g


@pytest.mark.parametrize("D,rank", [(1, 0), (5, 0), (33, 0), (128, 0), (1, 1), (5, 3), (33, 40), (128, 128)])
def test_apply_step(D, rank):
    from audio_mps_amd.scan import HipScan
    m = G.rho_model(D, rank) if rank else G.psi_model(D)
    state = ("vars", "adam_m", "adam_v")
    for mode in ("grads", "null", "skipped"):
        gs = None if mode == "null" else synthetic_grad_sums(D, rank, bad=(mode == "skipped"))

        def run(fill):
            drv = G.Driver(D, fill)
            names = G.apply_step(drv, m, gs, rank)
            if mode != "grads":                                      # include/cmps.h: variables and Adam slots "stay as they are"
                for k in state:
                    assert drv.bufs[k].equals_snapshot() is None, (mode, k, drv.bufs[k].equals_snapshot())
            drv.finish()
            return drv.result(names)
        res = both_fills(run, f"apply_step ({D}, {rank}) {mode}")
        # anchor: the same call through HipScan
        be = HipScan(D)
        dev = be.device
        v0 = G.var_array(m, rank)
        t = {k: torch.from_numpy(as_input).to(dev) for k, as_input in zip(state, apply_inputs(v0))}
        params = torch.empty(2 * D * D + 3 * D + 1, dtype=torch.float32, device=dev)
        losses = torch.zeros(2, dtype=torch.float32, device=dev)
        hp = m.hparams
        args = (None if gs is None else torch.from_numpy(gs).to(dev),) + ((rank,) if rank else ()) + \
               (4, 1e-3, 0.9, 0.999, 1e-8, float(hp.h_reg), float(hp.r_reg), float(m._c_r), float(m._c_h), True, params)
        if rank:
            phi = torch.empty(2 * rank * D, dtype=torch.float32, device=dev)
            be.rho_apply_step(t["vars"], t["adam_m"], t["adam_v"], *args, phi, losses)
        else:
            be.apply_step(t["vars"], t["adam_m"], t["adam_v"], *args, losses)
        ref = {k: t[k].cpu().numpy().view(np.uint8) for k in state}
        ref["params_out"] = params.cpu().numpy().view(np.uint8)
        if rank:
            ref["phi_out"] = phi.cpu().numpy().view(np.uint8)
        if gs is not None:
            ref["losses"] = losses.cpu().numpy().view(np.uint8)
        G.same_bits(res, ref, f"apply_step ({D}, {rank}) {mode}: driver against HipScan")
        if mode == "skipped":
            assert np.isnan(as_f32(res, "losses")[1]) and as_f32(res, "losses")[0] == np.float32(12.5 / 4)
        if mode == "grads":
            assert not np.array_equal(res["vars"], v0.view(np.uint8)) and np.all(np.isfinite(as_f32(res, "vars")))


def apply_inputs(v0):
    """The variables and Adam slots tests/_guard.py::apply_step loads."""
    rng = np.random.default_rng(11)
    return v0, (1e-3 * rng.standard_normal(v0.size)).astype(np.float32), (1e-6 * rng.random(v0.size)).astype(np.float32)
