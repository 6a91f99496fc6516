"""A RhoCMPS bank's streams at the C ABI without a GPU (cmps_rho_bank_stream_state_bytes, cmps_rho_bank_stream,
cmps_rho_bank_stream_score; include/cmps.h): the symbols, the prototypes, and what the contract answers before
cmps_rho_bank_set_state_dev has succeeded -- a null handle, a fresh handle of every kernel family, a handle whose set-up was refused --
each with a message that starts with the entry's name.  Nothing here touches a device: the pointers are fake.  What needs a bank on the
device (the argument errors, the other modes, the bits) is in tests/test_gpu_rho_bank_stream.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384     # non-null "device pointers": every call returns before anything looks at them
NEW = ("cmps_rho_bank_stream_state_bytes", "cmps_rho_bank_stream", "cmps_rho_bank_stream_score")


def _handle(lib, D, variant=0):
    from audio_mps_amd import _capi
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
    return h


def _stream(lib, h, state_in=None, state_out=PTR, k0=0, audio=PTR2, n_audio=1, forced=4, noise=PTR3, n_noise=2, length=4, n=2, out=PTR4,
            pred=None):
    return lib.cmps_rho_bank_stream(h, state_in, state_out, k0, audio, n_audio, forced, noise, n_noise, length, n, out, pred, None)


def _score(lib, h, state_in=None, state_out=PTR, k0=0, audio=PTR2, n_audio=1, forced=4, n=2, nll=PTR3, loss=PTR4, pred=None):
    return lib.cmps_rho_bank_stream_score(h, state_in, state_out, k0, audio, n_audio, forced, n, nll, loss, pred, None)


ENTRIES = ((_stream, "cmps_rho_bank_stream"), (_score, "cmps_rho_bank_stream_score"))


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
    flat = re.sub(r"\s+", " ", header)
    assert ("int cmps_rho_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, "
            "int n_audio, int forced, const float* noise_dev, int n_noise, int length, int n, float* out_dev, float* pred_dev, "
            "void* stream);") in flat
    assert ("int cmps_rho_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, "
            "int n_audio, int forced, int n, float* nll_dev, float* loss_dev, float* pred_dev, void* stream);") in flat
    assert "size_t cmps_rho_bank_stream_state_bytes(cmps_handle_t h, int n);" in flat
    # the argument lists are those of cmps_bank_stream*
    assert hip_lib.cmps_rho_bank_stream.argtypes == hip_lib.cmps_bank_stream.argtypes and len(hip_lib.cmps_rho_bank_stream.argtypes) == 14
    assert hip_lib.cmps_rho_bank_stream_score.argtypes == hip_lib.cmps_bank_stream_score.argtypes
    assert len(hip_lib.cmps_rho_bank_stream_score.argtypes) == 12
    assert hip_lib.cmps_rho_bank_stream_state_bytes.restype is ctypes.c_size_t
    assert hip_lib.cmps_rho_bank_stream.restype is ctypes.c_int and hip_lib.cmps_rho_bank_stream_score.restype is ctypes.c_int
    section = header[header.index("stream, sample and score with M RhoCMPS models"):]
    for cite in ("bit for bit", "cmps_rho_stream_score", "cmps_rho_set_state", "k_sample_rho_mfma_stream", "k_sample_rho_mfma_score", "n_noise",
                 "save_states", "CMPS_ERR_STATE"):
        assert cite in section, cite
    # the RhoCMPS bank's own section no longer says there are none, and points at them
    bank = header[header.index("M RhoCMPS models of one shape per kernel launch"):header.index("size_t cmps_rho_bank_workspace_bytes")]
    assert "no bank samplers" not in bank and "cmps_rho_bank_stream" in bank
    assert hip_lib.cmps_version() == 500                                             # no new error codes, no new version


def test_a_null_handle(hip_lib):
    from audio_mps_amd import _capi
    lib = hip_lib
    assert lib.cmps_rho_bank_stream_state_bytes(None, 3) == 0
    assert _stream(lib, None) == _capi.CMPS_ERR_BAD_ARG
    assert _score(lib, None) == _capi.CMPS_ERR_BAD_ARG


@pytest.mark.parametrize("D,variant", [(3, 0), (16, 0), (20, 2), (32, 4), (5, 1), (48, 1), (64, 0), (128, 3)])
def test_a_fresh_handle_holds_no_bank(hip_lib, D, variant):
    """Outside RhoCMPS bank mode the state size is 0 and both entries answer CMPS_ERR_STATE before they look at an argument: with good
    arguments and with every argument wrong at once, the message is the call order's."""
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        for n in (-3, 0, 1, 2, 1000):
            assert lib.cmps_rho_bank_stream_state_bytes(h, n) == 0
        for call, entry in ENTRIES:
            for kw in ({}, dict(n=0, forced=-1, k0=-1, audio=None, n_audio=7, state_in=PTR)):
                code = call(lib, h, **kw)
                msg = lib.cmps_last_error(h).decode()
                assert code == _capi.CMPS_ERR_STATE and msg.startswith(entry + ":") and "cmps_rho_bank_set_state_dev" in msg, (code, msg)
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("D,rank,variant,M,code", [(8, 2, 0, 2, "CMPS_ERR_UNSUPPORTED_D"), (33, 4, 0, 2, "CMPS_ERR_UNSUPPORTED_D"),
                                                   (8, 4, 1, 2, "CMPS_ERR_STATE"), (8, 4, 0, 0, "CMPS_ERR_BAD_ARG"),
                                                   (8, 4, 0, 2, "CMPS_ERR_WORKSPACE")])
def test_a_refused_set_up_leaves_the_handle_outside_bank_mode(hip_lib, D, rank, variant, M, code):
    """cmps_rho_bank_set_state_dev refused by its own checks (rank, D, variant, M, a null workspace -- all before the device is touched):
    the streams still say the call order, and the sizes stay 0."""
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        ws = None if code == "CMPS_ERR_WORKSPACE" else PTR3
        assert lib.cmps_rho_bank_set_state_dev(h, M, PTR, PTR2, rank, 1e-4, 1e-4, 8, 2, 0, ws, 1 << 40, None) == getattr(_capi, code)
        assert lib.cmps_rho_bank_stream_state_bytes(h, 2) == 0
        for call, entry in ENTRIES:
            assert call(lib, h) == _capi.CMPS_ERR_STATE
            assert lib.cmps_last_error(h).decode().startswith(entry + ":")
        # the PsiCMPS bank's entries and the plain RhoCMPS ones answer as before
        assert lib.cmps_bank_stream_state_bytes(h, 2) == 0 and lib.cmps_rho_stream_state_bytes(h, 2) == 0
    finally:
        lib.cmps_destroy(h)
