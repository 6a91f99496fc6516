"""cmps_batch_gather and cmps_damped_sine_fill at the C ABI without a GPU: the symbols, and every CMPS_ERR_BAD_ARG of their contracts,
returned before the device is touched with a message that starts with the entry's name and names the argument -- the first failing check
speaking.  The kernels themselves are tested in tests/test_gpu_device_data.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3 = 4096, 8192, 12288      # non-null "device pointers": every call below must return before anything looks at them


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in ("cmps_batch_gather", "cmps_damped_sine_fill"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
    assert re.search(r"^int cmps_batch_gather\(cmps_handle_t h, const float\* data_dev, long long n_clips, long long clip_len,\s*"
                     r"const int\* index_dev, const int\* offset_dev, int B, int T,\s*float\* audio_dev, void\* stream\);", header, flags=re.M)
    assert re.search(r"^int cmps_damped_sine_fill\(cmps_handle_t h, unsigned long long seed, unsigned long long first_clip,\s*"
                     r"int B, int T, double delta_t, float\* audio_dev, void\* stream\);", header, flags=re.M)
    assert "k_batch_gather" in header and "k_damped_sine" in header                     # CMPS_OPT_KERNEL_EVENTS names them
    assert hip_lib.cmps_batch_gather.argtypes[2:4] == [ctypes.c_longlong, ctypes.c_longlong]
    assert hip_lib.cmps_damped_sine_fill.argtypes[1:3] == [ctypes.c_ulonglong, ctypes.c_ulonglong]
    assert hip_lib.cmps_damped_sine_fill.argtypes[5] == ctypes.c_double
    assert hip_lib.cmps_version() == 500


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_batch_gather(None, PTR, 4, 8, PTR2, None, 2, 8, PTR3, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    assert lib.cmps_damped_sine_fill(None, 1, 0, 2, 8, 1e-3, PTR, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def said(entry, names):
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith(entry + ":") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        def gather(names, data=PTR, n_clips=4, clip_len=8, index=PTR2, offset=None, B=2, T=8, audio=PTR3):
            assert lib.cmps_batch_gather(h, data, n_clips, clip_len, index, offset, B, T, audio, None) == BAD
            said("cmps_batch_gather", names)

        gather(["data_dev"], data=None)
        gather(["index_dev"], index=None)
        gather(["audio_dev"], audio=None)
        for B in (0, -3):
            gather(["B", "T"], B=B)
        for T in (0, -1):
            gather(["B", "T"], T=T)
        for n in (0, -1, 2 ** 31, 2 ** 40):
            gather(["n_clips"], n_clips=n)
        gather(["clip_len", "T"], clip_len=7)
        gather(["clip_len", "T"], clip_len=0)
        gather(["clip_len", "T"], clip_len=-2 ** 40)
        # the first failing check speaks: the pointers in the order of the signature, then B and T, then n_clips, then clip_len
        gather(["data_dev"], data=None, index=None, audio=None, B=0)
        gather(["index_dev"], index=None, audio=None, n_clips=0)
        gather(["audio_dev"], audio=None, B=0, clip_len=1)
        gather(["B", "T"], B=0, n_clips=0, clip_len=1)
        gather(["n_clips"], n_clips=0, clip_len=1)

        def sine(names, seed=1, first_clip=0, B=2, T=8, delta_t=1e-3, audio=PTR):
            assert lib.cmps_damped_sine_fill(h, seed, first_clip, B, T, delta_t, audio, None) == BAD
            said("cmps_damped_sine_fill", names)

        sine(["audio_dev"], audio=None)
        for B in (0, -4):
            sine(["B", "T"], B=B)
        for T in (0, -1, 2 ** 24 + 1, 2 ** 31 - 1):
            sine(["B", "T"], T=T)
        for dt in (0.0, -1e-3, -0.0, float("inf"), float("-inf"), float("nan")):
            sine(["delta_t"], delta_t=dt)
        sine(["first_clip", "B"], first_clip=2 ** 64 - 1, B=1)                          # first_clip + B = 2^64
        sine(["first_clip", "B"], first_clip=2 ** 64 - 3, B=2 ** 31 - 1)
        # the first failing check speaks: the pointer, then the sizes, then delta_t, then the clip range
        sine(["audio_dev"], audio=None, B=0, delta_t=0.0)
        sine(["B", "T"], T=2 ** 24 + 1, delta_t=float("nan"), first_clip=2 ** 64 - 1)
        sine(["delta_t"], delta_t=0.0, first_clip=2 ** 64 - 1)
    finally:
        lib.cmps_destroy(h)
