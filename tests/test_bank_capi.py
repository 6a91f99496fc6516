"""The model bank at the C ABI without a GPU (cmps_bank_*, include/cmps.h): the symbols, cmps_bank_workspace_bytes, and every
CMPS_ERR_BAD_ARG / UNSUPPORTED_D / STATE / WORKSPACE of the contracts that can be provoked before the device is touched -- each with a
message that starts with the entry's name, the first failing check speaking.  The kernels are tested in tests/test_gpu_bank.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384     # non-null, 256-byte aligned "device pointers": every call returns before anything looks at them
BANK = ("cmps_bank_workspace_bytes", "cmps_bank_set_params_dev", "cmps_bank_loss_fwd", "cmps_bank_loss_bwd",
        "cmps_bank_apply_step_scratch_bytes", "cmps_bank_apply_step", "cmps_bank_grad_status")


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in BANK:
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
    assert re.search(r"^int cmps_bank_loss_fwd\(cmps_handle_t h, const float\* audio_dev, int n_audio, int B, int T, float\* loss_dev, "
                     r"int save_for_bwd, void\* stream\);", header, flags=re.M)
    for cite in ("train.py:31", "train.py:41", "reader.py:9-66", "cmps_set_params_dev", "cmps_psi_apply_step", "cmps_psi_grad_status"):
        assert cite in header[header.index("Model bank"):], cite
    assert hip_lib.cmps_bank_apply_step.argtypes[6:12] == [ctypes.c_double] * 6
    assert hip_lib.cmps_version() == 500                                             # no new error codes, no new version


@pytest.mark.parametrize("D,M,B,T,flags", [(3, 3, 3, 70, 1), (16, 5, 2, 130, 1), (17, 4, 3, 100, 0), (32, 1, 8, 16000, 1), (40, 2, 2, 50, 1),
                                           (128, 1024, 1, 2, 5)])
def test_bank_workspace_is_M_plain_workspaces(hip_lib, D, M, B, T, flags):
    plain = hip_lib.cmps_workspace_bytes(D, B, T, flags)
    assert plain > 0 and plain % 256 == 0
    assert hip_lib.cmps_bank_workspace_bytes(D, M, B, T, flags) == M * plain
    for bad_M in (0, -1, 1025):
        assert hip_lib.cmps_bank_workspace_bytes(D, bad_M, B, T, flags) == 0
    assert hip_lib.cmps_bank_workspace_bytes(D, M, 0, T, flags) == 0 and hip_lib.cmps_bank_workspace_bytes(D, M, B, 1, flags) == 0
    assert hip_lib.cmps_bank_apply_step_scratch_bytes(D, M) == M * hip_lib.cmps_apply_step_scratch_bytes(D)
    assert hip_lib.cmps_bank_apply_step_scratch_bytes(D, 0) == 0


def _handle(lib, D, variant=0):
    from audio_mps_amd import _capi
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
    return h


@pytest.mark.parametrize("D,variant", [(3, 0), (20, 0), (32, 4), (48, 1), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    lib, BAD, WS, STATE = hip_lib, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_WORKSPACE, _capi.CMPS_ERR_STATE
    big = 1 << 40
    assert lib.cmps_bank_set_params_dev(None, 2, PTR, 1e-4, 1e-4, 8, 2, 1, PTR2, big, None) == BAD
    assert lib.cmps_bank_loss_fwd(None, PTR, 1, 2, 8, PTR2, 0, None) == BAD
    assert lib.cmps_bank_loss_bwd(None, PTR, 1, 2, 8, PTR2, None) == BAD
    assert lib.cmps_bank_apply_step(None, 2, PTR, PTR, PTR, None, 1.0, 1.0, 1.0, 0.9, 0.999, 1e-8, PTR2, 1, PTR3, PTR3, PTR4, None) == BAD
    assert lib.cmps_bank_grad_status(None, (ctypes.c_int * 2)(), None, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = _handle(lib, D, variant)
    try:
        def said(code, want, entry, *words):
            msg = lib.cmps_last_error(h).decode()
            assert code == want and msg.startswith(entry + ":") and all(w in msg for w in words), (code, msg)

        def setp(want, words, M=2, params=PTR, T=8, B=2, ws=PTR2, nbytes=big):
            said(lib.cmps_bank_set_params_dev(h, M, params, 1e-4, 1e-4, T, B, 1, ws, nbytes, None), want, "cmps_bank_set_params_dev", *words)

        setp(BAD, ["null"], params=None)
        for M in (0, -1, 1025):
            setp(BAD, ["M"], M=M)
        setp(BAD, ["B", "T"], B=0)
        setp(BAD, ["B", "T"], T=1)
        setp(BAD, ["overflows"], M=1024, B=2 ** 20, T=2 ** 20)
        setp(WS, ["null workspace"], ws=None)
        need = lib.cmps_bank_workspace_bytes(D, 2, 2, 8, 1)
        setp(WS, ["workspace has", str(need)], nbytes=need - 1)
        # the first failing check speaks: the pointer, then M, then the shape, then the workspace
        setp(BAD, ["null"], params=None, M=0, B=0, ws=None)
        setp(BAD, ["M"], M=0, B=0, ws=None)
        setp(BAD, ["B", "T"], B=0, ws=None)

        # the scans and the status need cmps_bank_set_params_dev first
        said(lib.cmps_bank_loss_fwd(h, PTR, 1, 2, 8, PTR2, 0, None), STATE, "cmps_bank_loss_fwd", "cmps_bank_set_params_dev")
        said(lib.cmps_bank_loss_bwd(h, PTR, 1, 2, 8, PTR2, None), STATE, "cmps_bank_loss_bwd", "cmps_bank_loss_fwd")
        said(lib.cmps_bank_grad_status(h, (ctypes.c_int * 2)(), None, None), STATE, "cmps_bank_grad_status", "cmps_bank_set_params_dev")
        said(lib.cmps_bank_grad_status(h, None, None, None), BAD, "cmps_bank_grad_status", "codes_out")

        def apply(words, M=2, vars_=PTR, params=PTR3, hyper=PTR2, grad=PTR, m=PTR, v=PTR, losses=PTR3, scratch=PTR4, batch=2.0):
            said(lib.cmps_bank_apply_step(h, M, vars_, m, v, grad, batch, 1.0, 1.0, 0.9, 0.999, 1e-8, hyper, 1, params, losses, scratch, None), BAD,
                 "cmps_bank_apply_step", *words)

        apply(["null"], vars_=None)
        apply(["null"], params=None)
        apply(["null"], hyper=None)
        for M in (0, 1025):
            apply(["M"], M=M)
        apply(["Adam"], m=None)
        apply(["Adam"], losses=None)
        apply(["Adam"], scratch=None)
        apply(["positive batch"], batch=0.0)
        apply(["scratch_dev", "8-byte"], scratch=PTR4 + 4)
        apply(["hyper_dev", "8-byte"], hyper=PTR2 + 4)
        apply(["null"], vars_=None, M=0, hyper=PTR2 + 4)
        apply(["M"], M=0, hyper=PTR2 + 4)
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("D,variant", [(33, 0), (48, 0), (64, 5), (128, 3)])
def test_a_bank_above_32_needs_the_block_variant(hip_lib, D, variant):
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        for code in (lib.cmps_bank_set_params_dev(h, 2, PTR, 1e-4, 1e-4, 8, 2, 1, PTR2, 1 << 40, None),
                     lib.cmps_bank_loss_fwd(h, PTR, 1, 2, 8, PTR2, 0, None), lib.cmps_bank_loss_bwd(h, PTR, 1, 2, 8, PTR2, None)):
            msg = lib.cmps_last_error(h).decode()
            assert code == _capi.CMPS_ERR_UNSUPPORTED_D and msg.startswith("cmps_bank_") and "needs CMPS_VARIANT_BLOCK" in msg, (code, msg)
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("option,value", [("CMPS_OPT_RANK1", 2), ("CMPS_OPT_RANK1", 3), ("CMPS_OPT_BWD_WAVES", 1), ("CMPS_OPT_F16_SCALE_SHIFT", -2)])
@pytest.mark.parametrize("D,variant", [(8, 0), (24, 0), (40, 1)])
def test_non_default_options_are_refused(hip_lib, D, variant, option, value):
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        assert lib.cmps_set_option(h, getattr(_capi, option), value) == _capi.CMPS_OK
        for entry, code in (("cmps_bank_set_params_dev", lib.cmps_bank_set_params_dev(h, 2, PTR, 1e-4, 1e-4, 8, 2, 1, PTR2, 1 << 40, None)),
                            ("cmps_bank_loss_fwd", lib.cmps_bank_loss_fwd(h, PTR, 1, 2, 8, PTR2, 0, None)),
                            ("cmps_bank_loss_bwd", lib.cmps_bank_loss_bwd(h, PTR, 1, 2, 8, PTR2, None))):
            assert code == _capi.CMPS_ERR_STATE, (entry, code)
        msg = lib.cmps_last_error(h).decode()
        assert msg.startswith("cmps_bank_loss_bwd:") and "CMPS_OPT_RANK1" in msg and "CMPS_OPT_BWD_WAVES" in msg
    finally:
        lib.cmps_destroy(h)


# Every refusal of the four *_apply_step entries, in the order their checks fire: (arguments that differ from a good call, code, message
# behind "<entry>: ").  None needs a configured handle, and none touches the device: a launch on these fake pointers would come back as
# CMPS_ERR_HIP, so the code also says that no kernel ran.
_ADAM = "an update needs the Adam slots, losses_dev, scratch_dev and a positive batch"
_SCRATCH, _HYPER, _M = "scratch_dev must be 8-byte aligned", "hyper_dev must be 8-byte aligned", "M outside [1, 1024]"
_UPDATE = [(dict(m=None), _ADAM), (dict(v=None), _ADAM), (dict(losses=None), _ADAM), (dict(scratch=None), _ADAM), (dict(batch=0.0), _ADAM),
           (dict(batch=float("nan")), _ADAM), (dict(scratch=PTR4 + 4), _SCRATCH), (dict(grad=None, scratch=PTR4 + 4), _SCRATCH)]
_BANK_UPDATE = _UPDATE + [(dict(hyper=PTR2 + 4), _HYPER), (dict(grad=None, hyper=PTR2 + 4), _HYPER)]
APPLY_REFUSALS = {
    "cmps_psi_apply_step": [(dict(vars_=None), "null variable / parameter buffer"), (dict(params=None), "null variable / parameter buffer")] + _UPDATE + [
        # the first failing check speaks
        (dict(vars_=None, m=None, scratch=PTR4 + 4), "null variable / parameter buffer"), (dict(m=None, scratch=PTR4 + 4), _ADAM)],
    "cmps_rho_apply_step": [(dict(vars_=None), "null variable / parameter / column buffer"), (dict(params=None), "null variable / parameter / column buffer"),
                            (dict(phi=None), "null variable / parameter / column buffer"), (dict(rank=0), "rank outside [1, 128]"),
                            (dict(rank=129), "rank outside [1, 128]")] + _UPDATE + [
        (dict(phi=None, rank=0, m=None), "null variable / parameter / column buffer"), (dict(rank=0, m=None, scratch=PTR4 + 4), "rank outside [1, 128]"),
        (dict(m=None, scratch=PTR4 + 4), _ADAM)],
    "cmps_bank_apply_step": [(dict(vars_=None), "null variable / parameter / hyper-parameter buffer"),
                             (dict(params=None), "null variable / parameter / hyper-parameter buffer"),
                             (dict(hyper=None), "null variable / parameter / hyper-parameter buffer"), (dict(M=0), _M), (dict(M=1025), _M)] + _BANK_UPDATE + [
        (dict(hyper=None, M=0, m=None), "null variable / parameter / hyper-parameter buffer"), (dict(M=0, m=None, scratch=PTR4 + 4), _M),
        (dict(m=None, scratch=PTR4 + 4, hyper=PTR2 + 4), _ADAM), (dict(scratch=PTR4 + 4, hyper=PTR2 + 4), _SCRATCH)],
    "cmps_rho_bank_apply_step": [(dict(rank=2), "a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32"), (dict(rank=33), "a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32"),
                                 (dict(vars_=None), "null variable / parameter / column / hyper-parameter buffer"),
                                 (dict(params=None), "null variable / parameter / column / hyper-parameter buffer"),
                                 (dict(phi=None), "null variable / parameter / column / hyper-parameter buffer"),
                                 (dict(hyper=None), "null variable / parameter / column / hyper-parameter buffer"), (dict(M=0), _M),
                                 (dict(M=1025), _M)] + _BANK_UPDATE + [
        (dict(rank=2, vars_=None, M=0), "a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32"),
        (dict(phi=None, M=0, m=None), "null variable / parameter / column / hyper-parameter buffer"), (dict(M=0, m=None, scratch=PTR4 + 4), _M),
        (dict(m=None, scratch=PTR4 + 4, hyper=PTR2 + 4), _ADAM), (dict(scratch=PTR4 + 4, hyper=PTR2 + 4), _SCRATCH)],
}


def _apply_step(lib, h, entry, M=2, rank=3, vars_=PTR, m=PTR, v=PTR, grad=PTR, batch=2.0, hyper=PTR2, params=PTR3, phi=PTR3, losses=PTR3, scratch=PTR4):
    adam = (0.9, 0.999, 1e-8)
    if entry == "cmps_psi_apply_step":
        return lib.cmps_psi_apply_step(h, vars_, m, v, grad, batch, 1e-3, *adam, 0.0, 0.0, 1.0, 1.0, 1, params, losses, scratch, None)
    if entry == "cmps_rho_apply_step":
        return lib.cmps_rho_apply_step(h, vars_, m, v, grad, rank, batch, 1e-3, *adam, 0.0, 0.0, 1.0, 1.0, 1, params, phi, losses, scratch, None)
    if entry == "cmps_bank_apply_step":
        return lib.cmps_bank_apply_step(h, M, vars_, m, v, grad, batch, 1.0, 1.0, *adam, hyper, 1, params, losses, scratch, None)
    return lib.cmps_rho_bank_apply_step(h, M, vars_, m, v, grad, rank, batch, 1.0, 1.0, *adam, hyper, 1, params, phi, losses, scratch, None)


@pytest.mark.parametrize("entry", sorted(APPLY_REFUSALS))
def test_every_refusal_of_the_apply_step_entries(hip_lib, entry):
    from audio_mps_amd import _capi
    lib = hip_lib
    assert _apply_step(lib, None, entry) == _capi.CMPS_ERR_BAD_ARG
    h = _handle(lib, 4)
    try:
        for kw, text in APPLY_REFUSALS[entry]:
            want = _capi.CMPS_ERR_UNSUPPORTED_D if text.startswith("a RhoCMPS bank") else _capi.CMPS_ERR_BAD_ARG
            code = _apply_step(lib, h, entry, **kw)
            assert (code, lib.cmps_last_error(h).decode()) == (want, f"{entry}: {text}"), kw
    finally:
        lib.cmps_destroy(h)
    if entry == "cmps_rho_bank_apply_step":                      # the shape rule reads the handle's D as well
        h = _handle(lib, 33, 1)
        try:
            assert _apply_step(lib, h, entry) == _capi.CMPS_ERR_UNSUPPORTED_D
            assert lib.cmps_last_error(h).decode() == "cmps_rho_bank_apply_step: a RhoCMPS bank needs D <= 32 and 3 <= rank <= 32"
        finally:
            lib.cmps_destroy(h)
