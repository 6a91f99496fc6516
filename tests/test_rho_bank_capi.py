"""The RhoCMPS model bank at the C ABI without a GPU (cmps_rho_bank_*, include/cmps.h): the symbols, the two size functions, and every
refusal of cmps_rho_bank_set_state_dev and cmps_rho_bank_apply_step that comes before the device is touched -- each with its code and a
message that starts with the entry's name.  The kernels are tested in tests/test_gpu_rho_bank.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384     # non-null, 256-byte aligned "device pointers": every call returns before anything looks at them
RHO_BANK = ("cmps_rho_bank_workspace_bytes", "cmps_rho_bank_set_state_dev", "cmps_rho_bank_loss_fwd", "cmps_rho_bank_loss_bwd",
            "cmps_rho_bank_apply_step_scratch_bytes", "cmps_rho_bank_apply_step")
BIG = 1 << 40


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in RHO_BANK:
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
    block = header[header.index("M RhoCMPS models of one shape"):]
    for cite in ("train.py:18-20, 50-53", "train.py:41", "model.py:55-203", "rank <= 2", "k_bwd_rho_mfma", "multi-rank", "samplers",
                 "CMPS_VARIANT_BLOCK", "CMPS_WS_FWD_ONLY"):
        assert cite in block, cite
    assert hip_lib.cmps_rho_bank_apply_step.argtypes[7:13] == [ctypes.c_double] * 6
    assert hip_lib.cmps_version() == 500                                             # no new error codes, no new version


@pytest.mark.parametrize("D,rank,M,B,T", [(3, 3, 3, 3, 70), (16, 5, 4, 3, 100), (32, 32, 1024, 1, 2)])
@pytest.mark.parametrize("flags", [0, 1, 5])
def test_workspace_is_M_times_main_tables_plus_rho_layout(hip_lib, D, rank, M, B, T, flags):
    lib = hip_lib
    main, rho = lib.cmps_workspace_bytes(D, B, T, 0), lib.cmps_rho_workspace_bytes(D, rank, B, T, flags & 1)
    assert main > 0 and rho > 0 and main % 256 == 0 and rho % 256 == 0
    assert lib.cmps_rho_bank_workspace_bytes(D, rank, M, B, T, flags) == M * (main + rho)
    assert lib.cmps_rho_bank_apply_step_scratch_bytes(D, rank, M) == M * lib.cmps_rho_apply_step_scratch_bytes(D, rank)


def test_size_functions_return_zero_on_bad_arguments(hip_lib):
    lib = hip_lib
    good = dict(D=8, rank=8, M=4, B=2, T=40)
    assert lib.cmps_rho_bank_workspace_bytes(*good.values(), 1) > 0
    for key, bad in (("M", 0), ("M", -1), ("M", 1025), ("D", 0), ("D", 33), ("rank", 2), ("rank", 33), ("rank", 0), ("B", 0), ("T", 1)):
        args = {**good, key: bad}
        assert lib.cmps_rho_bank_workspace_bytes(*args.values(), 1) == 0, (key, bad)
        if key in ("M", "D", "rank"):
            assert lib.cmps_rho_bank_apply_step_scratch_bytes(args["D"], args["rank"], args["M"]) == 0, (key, bad)


def _handle(lib, D, variant=0):
    from audio_mps_amd import _capi
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
    return h


def _said(lib, h, code, want, entry, *words):
    msg = lib.cmps_last_error(h).decode()
    assert code == want and msg.startswith(entry + ":") and all(w in msg for w in words), (code, msg)


def _set_state(lib, h, M=2, params=PTR, phi=PTR3, rank=4, T=8, B=2, ws=PTR2, nbytes=BIG):
    return lib.cmps_rho_bank_set_state_dev(h, M, params, phi, rank, 1e-4, 1e-4, T, B, 1, ws, nbytes, None)


def _apply(lib, h, M=2, vars_=PTR, params=PTR3, phi=PTR3, hyper=PTR2, grad=PTR, m=PTR, v=PTR, losses=PTR3, scratch=PTR4, batch=2.0, rank=4):
    return lib.cmps_rho_bank_apply_step(h, M, vars_, m, v, grad, rank, batch, 1.0, 1.0, 0.9, 0.999, 1e-8, hyper, 1, params, phi, losses, scratch, None)


@pytest.mark.parametrize("D,variant", [(3, 0), (20, 2), (32, 0)])
def test_refusals_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    lib, BAD, WS, STATE, UNS = hip_lib, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_WORKSPACE, _capi.CMPS_ERR_STATE, _capi.CMPS_ERR_UNSUPPORTED_D
    assert _set_state(lib, None) == BAD and _apply(lib, None) == BAD
    assert lib.cmps_rho_bank_loss_fwd(None, PTR, 1, 2, 8, PTR2, 0, None) == BAD
    assert lib.cmps_rho_bank_loss_bwd(None, PTR, 1, 2, 8, PTR2, None) == BAD
    h = _handle(lib, D, variant)
    try:
        who = "cmps_rho_bank_set_state_dev"
        _said(lib, h, _set_state(lib, h, params=None), BAD, who, "null")
        _said(lib, h, _set_state(lib, h, phi=None), BAD, who, "null")
        for M in (0, -1, 1025):
            _said(lib, h, _set_state(lib, h, M=M), BAD, who, "M")
        for rank in (2, 33):
            _said(lib, h, _set_state(lib, h, rank=rank), UNS, who, "rank")
        _said(lib, h, _set_state(lib, h, B=0), BAD, who, "B_max", "T")
        _said(lib, h, _set_state(lib, h, T=1), BAD, who, "B_max", "T")
        _said(lib, h, _set_state(lib, h, M=1024, rank=32, B=2 ** 12, T=2 ** 20), BAD, who, "overflows")
        _said(lib, h, _set_state(lib, h, ws=None), WS, who, "null workspace")
        _said(lib, h, _set_state(lib, h, ws=PTR2 + 128), WS, who, "256-byte aligned")
        need = lib.cmps_rho_bank_workspace_bytes(D, 4, 2, 2, 8, 1)
        assert need > 0
        _said(lib, h, _set_state(lib, h, nbytes=need - 1), WS, who, "workspace has", str(need))
        # the scans need cmps_rho_bank_set_state_dev first
        _said(lib, h, lib.cmps_rho_bank_loss_fwd(h, PTR, 1, 2, 8, PTR2, 0, None), STATE, "cmps_rho_bank_loss_fwd", "cmps_rho_bank_set_state_dev")
        _said(lib, h, lib.cmps_rho_bank_loss_bwd(h, PTR, 1, 2, 8, PTR2, None), STATE, "cmps_rho_bank_loss_bwd", "cmps_rho_bank_loss_fwd")

        who = "cmps_rho_bank_apply_step"
        for kw in (dict(vars_=None), dict(params=None), dict(phi=None), dict(hyper=None)):
            _said(lib, h, _apply(lib, h, **kw), BAD, who, "null")
        for M in (0, -1, 1025):
            _said(lib, h, _apply(lib, h, M=M), BAD, who, "M")
        for rank in (2, 33):
            _said(lib, h, _apply(lib, h, rank=rank), UNS, who, "rank")
        for kw in (dict(m=None), dict(v=None), dict(losses=None), dict(scratch=None)):
            _said(lib, h, _apply(lib, h, **kw), BAD, who, "Adam")
        _said(lib, h, _apply(lib, h, batch=0.0), BAD, who, "positive batch")
        _said(lib, h, _apply(lib, h, scratch=PTR4 + 4), BAD, who, "scratch_dev", "8-byte")
        _said(lib, h, _apply(lib, h, hyper=PTR2 + 4), BAD, who, "hyper_dev", "8-byte")
    finally:
        lib.cmps_destroy(h)


def test_D_above_32_is_unsupported(hip_lib):
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, 33)
    try:
        _said(lib, h, _set_state(lib, h), _capi.CMPS_ERR_UNSUPPORTED_D, "cmps_rho_bank_set_state_dev", "D <= 32")
        _said(lib, h, _apply(lib, h), _capi.CMPS_ERR_UNSUPPORTED_D, "cmps_rho_bank_apply_step", "D <= 32")
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("variant", [1, 4])          # CMPS_VARIANT_BLOCK, CMPS_VARIANT_WAVE32
def test_other_variants_are_refused(hip_lib, variant):
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, 8, variant)
    try:
        _said(lib, h, _set_state(lib, h), _capi.CMPS_ERR_STATE, "cmps_rho_bank_set_state_dev", "CMPS_VARIANT_AUTO")
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("option,value", [("CMPS_OPT_RHO_BWD", 1), ("CMPS_OPT_RANK1", 2), ("CMPS_OPT_BWD_WAVES", 1), ("CMPS_OPT_F16_SCALE_SHIFT", -2)])
def test_non_default_options_are_refused(hip_lib, option, value):
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, 8)
    try:
        assert _capi.CMPS_RHO_BWD_GEMM == 1
        assert lib.cmps_set_option(h, getattr(_capi, option), value) == _capi.CMPS_OK
        _said(lib, h, _set_state(lib, h), _capi.CMPS_ERR_STATE, "cmps_rho_bank_set_state_dev", "CMPS_OPT_RHO_BWD", "CMPS_OPT_RANK1",
              "CMPS_OPT_BWD_WAVES", "CMPS_OPT_F16_SCALE_SHIFT")
    finally:
        lib.cmps_destroy(h)
