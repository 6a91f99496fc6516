"""cmps_noise_fill at the C ABI without a GPU: the symbol, and every CMPS_ERR_BAD_ARG of its contract, returned before the device is
touched with a message that names the argument.  The kernel itself is tested in tests/test_gpu_noise.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 4096                 # a non-null "device pointer": every call below must return before anything looks at it


def test_symbol_is_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    assert "cmps_noise_fill" in _capi.SYMBOLS and hasattr(hip_lib, "cmps_noise_fill")
    assert re.search(r"^int cmps_noise_fill\(cmps_handle_t h, unsigned long long seed, unsigned long long first_step,\s*"
                     r"unsigned first_path, int n, int length, float stddev,\s*float\* noise_dev, void\* stream\);", header, flags=re.M)
    assert "k_noise_philox" in header                                                   # CMPS_OPT_KERNEL_EVENTS names it
    assert hip_lib.cmps_noise_fill.argtypes[1:4] == [ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_uint]


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_noise_fill(None, 1, 0, 0, 1, 1, 1.0, PTR, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def bad(names, seed=1, first_step=0, first_path=0, n=2, length=3, stddev=1.0, ptr=PTR):
            assert lib.cmps_noise_fill(h, seed, first_step, first_path, n, length, stddev, ptr, None) == BAD
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_noise_fill:") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        bad(["noise_dev"], ptr=None)
        bad(["n", "length"], n=0)
        bad(["n", "length"], n=-4)
        bad(["n", "length"], length=0)
        bad(["n", "length"], length=-1)
        for s in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
            bad(["stddev"], stddev=s)
        bad(["first_path", "n"], first_path=2 ** 32 - 1, n=2)                            # first_path + n = 2^32 + 1
        bad(["first_path", "n"], first_path=2 ** 32 - 5, n=6)
        bad(["first_step", "length"], first_step=2 ** 64 - 1, length=1)                  # first_step + length = 2^64
        bad(["first_step", "length"], first_step=2 ** 64 - 3, length=2 ** 31 - 1)
        # the first failing check speaks: a null pointer before the sizes, the sizes before stddev
        bad(["noise_dev"], ptr=None, n=0, stddev=-1.0)
        bad(["n", "length"], n=0, stddev=-1.0, first_path=2 ** 32 - 1)
    finally:
        lib.cmps_destroy(h)
