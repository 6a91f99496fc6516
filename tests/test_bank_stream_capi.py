"""A bank's streams at the C ABI without a GPU (cmps_bank_stream_state_bytes, cmps_bank_stream, cmps_bank_stream_score; include/cmps.h):
the symbols, and what the contract answers before cmps_bank_set_params_dev has succeeded -- a null handle, a fresh handle in every
kernel family, a handle whose options a bank refuses -- each with a message that starts with the entry's name, the first failing check
speaking.  Nothing here touches a device: the pointers are fake.  What needs a bank on the device (the argument errors behind a
successful cmps_bank_set_params_dev, legacy mode, a RhoCMPS bank) is in tests/test_gpu_bank_stream.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384     # non-null "device pointers": every call returns before anything looks at them
NEW = ("cmps_bank_stream_state_bytes", "cmps_bank_stream", "cmps_bank_stream_score")


def _handle(lib, D, variant=0):
    from audio_mps_amd import _capi
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
    return h


def _stream(lib, h, state_in=None, state_out=PTR, k0=0, audio=PTR2, n_audio=1, forced=4, noise=PTR3, n_noise=2, length=4, n=2, out=PTR4,
            pred=None):
    return lib.cmps_bank_stream(h, state_in, state_out, k0, audio, n_audio, forced, noise, n_noise, length, n, out, pred, None)


def _score(lib, h, state_in=None, state_out=PTR, k0=0, audio=PTR2, n_audio=1, forced=4, n=2, nll=PTR3, loss=PTR4, pred=None):
    return lib.cmps_bank_stream_score(h, state_in, state_out, k0, audio, n_audio, forced, n, nll, loss, pred, None)


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
    flat = re.sub(r"\s+", " ", header)
    assert ("int cmps_bank_stream(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, int n_audio, "
            "int forced, const float* noise_dev, int n_noise, int length, int n, float* out_dev, float* pred_dev, void* stream);") in flat
    assert ("int cmps_bank_stream_score(cmps_handle_t h, const void* state_in_dev, void* state_out_dev, int k0, const float* audio_dev, "
            "int n_audio, int forced, int n, float* nll_dev, float* loss_dev, float* pred_dev, void* stream);") in flat
    assert "size_t cmps_bank_stream_state_bytes(cmps_handle_t h, int n);" in flat
    section = header[header.index("stream, sample and score with M PsiCMPS models"):]
    for cite in ("train.py:82-85", "reader.py:9-66", "bit for bit", "cmps_psi_stream", "k_sample_wave_stream", "k_sample_block_score", "n_noise"):
        assert cite in section, cite
    # the list of plain entries a bank refuses points at the new ones
    refused = header[header.index("In bank mode"):header.index("int cmps_bank_set_params_dev")]
    assert "cmps_psi_stream*" in refused and "cmps_bank_stream" in refused
    assert len(hip_lib.cmps_bank_stream.argtypes) == 14 and len(hip_lib.cmps_bank_stream_score.argtypes) == 12
    assert hip_lib.cmps_bank_stream_state_bytes.restype is ctypes.c_size_t
    assert hip_lib.cmps_version() == 500                                             # no new error codes, no new version


def test_a_null_handle(hip_lib):
    from audio_mps_amd import _capi
    lib = hip_lib
    assert lib.cmps_bank_stream_state_bytes(None, 3) == 0
    assert _stream(lib, None) == _capi.CMPS_ERR_BAD_ARG
    assert _score(lib, None) == _capi.CMPS_ERR_BAD_ARG
    assert b"handle" in lib.cmps_last_error(None)


@pytest.mark.parametrize("D,variant", [(3, 0), (16, 0), (20, 2), (32, 4), (5, 1), (48, 1), (128, 1)])
def test_a_fresh_handle_holds_no_bank(hip_lib, D, variant):
    """Outside bank mode the state size is 0 and both entries answer CMPS_ERR_STATE before they look at an argument: with good arguments
    and with every argument wrong at once, the message is the call order's."""
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        for n in (-3, 0, 1, 2, 1000):
            assert lib.cmps_bank_stream_state_bytes(h, n) == 0
        assert lib.cmps_psi_stream_state_bytes(h, 2) > 0                              # (the plain entry's answer does not depend on the mode)
        for call, entry in ((_stream, "cmps_bank_stream"), (_score, "cmps_bank_stream_score")):
            for kw in ({}, dict(n=0, forced=-1, k0=-1, audio=None, n_audio=7, state_in=PTR)):
                code = call(lib, h, **kw)
                msg = lib.cmps_last_error(h).decode()
                assert code == _capi.CMPS_ERR_STATE and msg.startswith(entry + ":") and "cmps_bank_set_params_dev" in msg, (code, msg)
        # a cmps_bank_set_params_dev that fails its own checks leaves the handle outside bank mode
        assert lib.cmps_bank_set_params_dev(h, 0, PTR, 1e-4, 1e-4, 8, 2, 0, PTR2, 1 << 40, None) == _capi.CMPS_ERR_BAD_ARG
        assert lib.cmps_bank_stream_state_bytes(h, 2) == 0 and _stream(lib, h) == _capi.CMPS_ERR_STATE
        assert lib.cmps_last_error(h).decode().startswith("cmps_bank_stream:")
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("D,variant", [(33, 0), (64, 5), (128, 3)])
def test_the_wide_family_has_no_bank(hip_lib, D, variant):
    """Above D = 32 without CMPS_VARIANT_BLOCK there is no bank to stream: the set-up is refused, and the streams say the call order."""
    from audio_mps_amd import _capi
    lib = hip_lib
    h = _handle(lib, D, variant)
    try:
        assert lib.cmps_bank_set_params_dev(h, 2, PTR, 1e-4, 1e-4, 8, 2, 0, PTR2, 1 << 40, None) == _capi.CMPS_ERR_UNSUPPORTED_D
        for call, entry in ((_stream, "cmps_bank_stream"), (_score, "cmps_bank_stream_score")):
            assert call(lib, h) == _capi.CMPS_ERR_STATE
            assert lib.cmps_last_error(h).decode().startswith(entry + ":")
        assert lib.cmps_bank_stream_state_bytes(h, 2) == 0
    finally:
        lib.cmps_destroy(h)
