"""The mode x entry matrix of the C ABI: ONE handle walked through its six states, and in every state every entry whose answer depends on
the state (those that tests/test_gpu_bank_modes.py part 2 does not pin: the loss forward and reverse entries of all five kinds, the grad
status entries, the state read-outs, the ancilla updates, the samplers, cmps_rho_set_state, the *_stream_state_bytes, CMPS_OPT_SAVED_ROWS).

A refused call is pinned by its code and its whole message; an accepted call returns CMPS_OK on real device buffers and is waited for;
a byte count is zero or not.  The fresh handle needs no device (every call is refused before a pointer is looked at); the five
configured states run on the GPU.  Shapes as in tests/test_gpu_bank_modes.py: D = 4, rank 3, M = 2, B = 2, T = 9, n = 2.

NOT CALLED (accepted by the library, but no test and no caller in this repository runs the pair, so it is not tried out here either):
  - legacy x cmps_psi_update_ancilla, cmps_psi_sample: accepted after any setter of the main workspace; nobody samples the legacy tables;
  - PsiCMPS model with cmps_rho_set_state x cmps_psi_loss_fwd, cmps_psi_loss_bwd, cmps_psi_grad_status, cmps_psi_states, cmps_psi_sample,
    cmps_psi_sample_primed: cmps_rho_set_state leaves the main workspace alone, so the answers are those of the column before; no
    caller runs the pure-state scans on a handle that holds the columns of rho_0."""
import ctypes

import pytest

from audio_mps_amd import _capi

D, RANK, M, B, T, N = 4, 3, 2, 2, 9, 2
OK, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_STATE
NC = "not called"
STATES = ("fresh", "psi", "psi + rho", "legacy", "psi bank", "rho bank")

SET = "call cmps_set_params first"
NO_PSI = "call cmps_set_params first (not available in legacy mode)"
NO_RHO = "call cmps_set_params and cmps_rho_set_state first (not available in legacy mode)"
NO_RHO_PLAIN = "call cmps_set_params and cmps_rho_set_state first"
IS_BANK = "the handle holds a bank (cmps_bank_set_params_dev / cmps_rho_bank_set_state_dev); call cmps_set_params for one model first"
LEGACY = "not available in legacy mode"
PSI_FWD = "needs cmps_psi_loss_fwd(save_for_bwd=1) first"
LEGACY_SET, LEGACY_FWD = "call cmps_legacy_set_params first", "needs cmps_legacy_loss_fwd(save_for_bwd=1) first"
RHO_SET, RHO_FWD = "call cmps_rho_set_state (after cmps_set_params) first", "needs cmps_rho_loss_fwd(save_for_bwd=1) first"
BANK_SET, BANK_FWD = "call cmps_bank_set_params_dev first", "needs cmps_bank_loss_fwd(save_for_bwd=1) first"
RHO_BANK_SET, RHO_BANK_FWD = "call cmps_rho_bank_set_state_dev first", "needs cmps_rho_bank_loss_fwd(save_for_bwd=1) first"
WEIGHTED_RHO = "the handle holds a RhoCMPS bank; the weighted reverse pass is for PsiCMPS banks (cmps_bank_set_params_dev)"
PSI_STATUS = "needs cmps_set_params with a CMPS_WS_TRAIN workspace"
BANK_STATUS = "needs cmps_bank_set_params_dev with a CMPS_WS_TRAIN workspace"
RHO_STATES = "needs cmps_rho_loss_fwd(save_for_bwd=1) or cmps_rho_sample(save_states=1) first"

# entry: its answer in the six STATES -- OK, NC, or the message of its CMPS_ERR_STATE behind "<entry>: ".  The order of the rows is the
# order of the calls in a state: a read-out and then a reverse pass follow their forward, the samplers (which overwrite the rho record)
# come behind cmps_rho_states, and cmps_rho_set_state (which discards it) comes last.
MATRIX = [
    ("cmps_psi_loss_fwd",           (SET, OK, NC, SET, SET, SET)),
    ("cmps_psi_states",             (PSI_FWD, OK, NC, LEGACY + " (no time table for the lab-frame phases)", IS_BANK, IS_BANK)),
    ("cmps_psi_loss_bwd",           (PSI_FWD, OK, NC, PSI_FWD, PSI_FWD, PSI_FWD)),
    ("cmps_psi_grad_status",        (PSI_STATUS, OK, NC, PSI_STATUS, IS_BANK, IS_BANK)),
    ("cmps_legacy_loss_fwd",        (LEGACY_SET, LEGACY_SET, LEGACY_SET, OK, LEGACY_SET, LEGACY_SET)),
    ("cmps_legacy_loss_bwd",        (LEGACY_FWD, LEGACY_FWD, LEGACY_FWD, OK, LEGACY_FWD, LEGACY_FWD)),
    ("cmps_rho_loss_fwd",           (RHO_SET, RHO_SET, OK, RHO_SET, RHO_SET, RHO_SET)),
    ("cmps_rho_states",             (RHO_STATES, RHO_STATES, OK, RHO_STATES, RHO_STATES, RHO_STATES)),
    ("cmps_rho_loss_bwd",           (RHO_FWD, RHO_FWD, OK, RHO_FWD, RHO_FWD, RHO_FWD)),
    ("cmps_bank_loss_fwd",          (BANK_SET, BANK_SET, BANK_SET, LEGACY, OK, BANK_SET)),
    ("cmps_bank_loss_bwd",          (BANK_FWD, BANK_FWD, BANK_FWD, LEGACY, OK, BANK_FWD)),
    ("cmps_bank_loss_fwd",          (BANK_SET, BANK_SET, BANK_SET, LEGACY, OK, BANK_SET)),      # (a forward of its own for the weighted pass)
    ("cmps_bank_loss_bwd_weighted", (BANK_FWD, BANK_FWD, BANK_FWD, LEGACY, OK, WEIGHTED_RHO)),
    ("cmps_bank_grad_status",       (BANK_STATUS, BANK_STATUS, BANK_STATUS, BANK_STATUS, OK, BANK_STATUS)),
    ("cmps_rho_bank_loss_fwd",      (RHO_BANK_SET, RHO_BANK_SET, RHO_BANK_SET, RHO_BANK_SET, RHO_BANK_SET, OK)),
    ("cmps_rho_bank_loss_bwd",      (RHO_BANK_FWD, RHO_BANK_FWD, RHO_BANK_FWD, RHO_BANK_FWD, RHO_BANK_FWD, OK)),
    ("cmps_psi_update_ancilla",     (SET, OK, OK, NC, IS_BANK, IS_BANK)),
    ("cmps_rho_update_ancilla",     (SET, OK, OK, SET, IS_BANK, IS_BANK)),
    ("cmps_psi_sample",             (SET, OK, NC, NC, IS_BANK, IS_BANK)),
    ("cmps_psi_sample_primed",      (NO_PSI, OK, NC, NO_PSI, IS_BANK, IS_BANK)),
    ("cmps_rho_sample",             (NO_RHO_PLAIN, NO_RHO_PLAIN, OK, NO_RHO_PLAIN, NO_RHO_PLAIN, NO_RHO_PLAIN)),
    ("cmps_rho_sample_primed",      (NO_RHO, NO_RHO, OK, NO_RHO, NO_RHO, NO_RHO)),
    ("cmps_rho_set_state",          (SET, OK, OK, SET, IS_BANK, IS_BANK)),
]
# the byte counts of n = 2 paths, non-zero (True) or zero; the pure-state count asks nothing of the mode
BYTES = [("cmps_psi_stream_state_bytes",      (True, True, True, True, True, True)),
         ("cmps_rho_stream_state_bytes",      (False, False, True, False, False, False)),
         ("cmps_bank_stream_state_bytes",     (False, False, False, False, True, False)),
         ("cmps_rho_bank_stream_state_bytes", (False, False, False, False, False, True))]


def calls(lib, h, x, out, rho_ws, rho_bytes):
    """entry -> a call with good arguments for (D, RANK, M, B, T, N): every input pointer is x, the outputs are `out` (apart; the losses 8192 bytes into it), the bank
    entries share one batch (n_audio = 1); the status words come back in host arrays"""
    sticky, codes, stickies = ctypes.c_int(), (ctypes.c_int * M)(), (ctypes.c_int * M)()
    loss = out + 8192                                                # (a forward's losses stay while its reverse pass writes to `out`)
    keep = (sticky, codes, stickies)
    return {
        "cmps_psi_loss_fwd": lambda: lib.cmps_psi_loss_fwd(h, x, B, T, loss, 1, None),
        "cmps_psi_loss_bwd": lambda: lib.cmps_psi_loss_bwd(h, x, B, T, out, None),
        "cmps_psi_grad_status": lambda: lib.cmps_psi_grad_status(h, ctypes.byref(sticky), None),
        "cmps_psi_states": lambda: lib.cmps_psi_states(h, B, T, out, None),
        "cmps_legacy_loss_fwd": lambda: lib.cmps_legacy_loss_fwd(h, x, B, T, loss, 1, None),
        "cmps_legacy_loss_bwd": lambda: lib.cmps_legacy_loss_bwd(h, x, B, T, out, None),
        "cmps_rho_loss_fwd": lambda: lib.cmps_rho_loss_fwd(h, x, B, T, loss, 1, None),
        "cmps_rho_loss_bwd": lambda: lib.cmps_rho_loss_bwd(h, x, B, T, out, None),
        "cmps_rho_states": lambda: lib.cmps_rho_states(h, B, T - 1, out, None, None),
        "cmps_bank_loss_fwd": lambda: lib.cmps_bank_loss_fwd(h, x, 1, B, T, loss, 1, None),
        "cmps_bank_loss_bwd": lambda: lib.cmps_bank_loss_bwd(h, x, 1, B, T, out, None),
        "cmps_bank_loss_bwd_weighted": lambda: lib.cmps_bank_loss_bwd_weighted(h, x, 1, B, T, x, B, out, None),
        "cmps_bank_grad_status": lambda: lib.cmps_bank_grad_status(h, codes, stickies, None),
        "cmps_rho_bank_loss_fwd": lambda: lib.cmps_rho_bank_loss_fwd(h, x, 1, B, T, loss, 1, None),
        "cmps_rho_bank_loss_bwd": lambda: lib.cmps_rho_bank_loss_bwd(h, x, 1, B, T, out, None),
        "cmps_psi_update_ancilla": lambda: lib.cmps_psi_update_ancilla(h, x, x, 0.0, B, out, None),
        "cmps_rho_update_ancilla": lambda: lib.cmps_rho_update_ancilla(h, x, x, 0.0, B, out, None),
        "cmps_psi_sample": lambda: lib.cmps_psi_sample(h, x, N, 4, out, None),
        "cmps_psi_sample_primed": lambda: lib.cmps_psi_sample_primed(h, x, 1, 3, x, N, 4, out, None, None),
        "cmps_rho_sample": lambda: lib.cmps_rho_sample(h, x, N, 4, out, 0, None),
        "cmps_rho_sample_primed": lambda: lib.cmps_rho_sample_primed(h, x, 1, 3, x, N, 4, out, None, 0, None),
        "cmps_rho_set_state": lambda: lib.cmps_rho_set_state(h, x, x, RANK, T, B, _capi.CMPS_WS_TRAIN, rho_ws, rho_bytes, None),
    }, keep


def walk_state(lib, h, state, call, sync=lambda: None):
    """Every row of BYTES and of MATRIX in STATES[state] (the byte counts first: the last call of MATRIX may enter the next state)"""
    for entry, answers in BYTES:
        assert (getattr(lib, entry)(h, N) != 0) == answers[state], (STATES[state], entry)
    for entry, answers in MATRIX:
        want = answers[state]
        if want is NC:
            continue
        code = call[entry]()
        message = lib.cmps_last_error(h).decode()
        if want is OK:
            assert code == OK, (STATES[state], entry, code, message)
            sync()
        else:
            assert (code, message) == (STATE, f"{entry}: {want}"), (STATES[state], entry)
    # (D = 4 is the 16-row family: no forward of this walk writes normalised rows)
    assert lib.cmps_get_option(h, _capi.CMPS_OPT_SAVED_ROWS) == 0, STATES[state]


def test_the_matrix_names_every_state_once():
    assert all(len(answers) == len(STATES) for _, answers in MATRIX + BYTES)
    assert len({entry for entry, _ in MATRIX}) == len(MATRIX) - 1 and len(dict(MATRIX)) == len(calls(None, None, 0, 0, 0, 0)[0])
    # every entry is accepted in some state, and refused in some other
    assert all(OK in answers and any(a not in (OK, NC) for a in answers) for _, answers in MATRIX)


def test_fresh_handle_refuses_before_it_looks_at_a_pointer(hip_lib):
    lib = hip_lib
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == OK
    try:
        call, keep = calls(lib, h, 4096, 8192, 12288, 1 << 20)       # non-null "device pointers"
        assert all(answers[0] not in (OK, NC) for _, answers in MATRIX)
        walk_state(lib, h, 0, call)
        del keep
    finally:
        lib.cmps_destroy(h)


@pytest.mark.gpu
def test_one_handle_walked_through_its_five_configured_states():
    import torch
    from audio_mps_amd.scan import HipScan
    from test_gpu_bank_modes import Models
    mo = Models(D)
    be = HipScan(D)
    lib, h = be._lib, be._h
    # inputs: one buffer of 0.1 behind every input pointer; outputs: one buffer apart, larger than the largest output of the walk
    # (cmps_rho_states: B (T - 1) D^2 complex = 512 floats; a bank's gradient sums: M (2 D^2 + 3 D + 2 + 2 RANK D) = 140)
    x = torch.full((4096,), 0.1, dtype=torch.float32, device="cuda")
    out = torch.zeros(4096, dtype=torch.float32, device="cuda")
    rho_bytes = lib.cmps_rho_workspace_bytes(D, RANK, B, T, _capi.CMPS_WS_TRAIN)
    rho_ws = torch.zeros(rho_bytes, dtype=torch.uint8, device="cuda")
    assert rho_bytes > 0 and rho_ws.data_ptr() % 256 == 0
    call, keep = calls(lib, h, x.data_ptr(), out.data_ptr(), rho_ws.data_ptr(), rho_bytes)

    be.set_params(mo.eff[0], B, T)
    walk_state(lib, h, 1, call, torch.cuda.synchronize)             # (its last call, cmps_rho_set_state, enters the next state)
    walk_state(lib, h, 2, call, torch.cuda.synchronize)
    be.legacy_set_params(mo.R, mo.Q, mo.hp.delta_t, B, T)
    walk_state(lib, h, 3, call, torch.cuda.synchronize)
    be.bank_set_params(mo.eff[:M], B, T, train=True)
    walk_state(lib, h, 4, call, torch.cuda.synchronize)
    be.rho_bank_set_state(mo.eff[:M], mo.cols[:M], B, T, train=True)
    walk_state(lib, h, 5, call, torch.cuda.synchronize)
    del keep
