"""cmps_bank_classify_weights and cmps_bank_loss_bwd_weighted at the C ABI without a GPU: the symbols, the 40-byte record's layout against
the header's table, and every CMPS_ERR_BAD_ARG of both contracts, returned before the device is touched with a message that starts with the
entry's name and names the argument -- the first failing check speaking (the convention of tests/test_classify_capi.py).  The kernels are
tested in tests/test_gpu_classify_weights.py and tests/test_gpu_bank_weighted.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384      # non-null "device pointers": every call below must return before anything looks at them
NAN, INF = float("nan"), float("inf")


def _header():
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        return f.read()


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    header = _header()
    for name in ("cmps_bank_classify_weights", "cmps_bank_loss_bwd_weighted"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
    assert re.search(r"^int cmps_bank_classify_weights\(cmps_handle_t h, const float\* loss_dev, int M, int B, long long ld, "
                     r"const int\* label_dev, double inv_temp,\s*double gen_weight, double disc_weight, int reset, float\* weight_dev, "
                     r"long long ldw, void\* record_dev,\s*void\* stream\);", header, flags=re.M)
    assert re.search(r"^int cmps_bank_loss_bwd_weighted\(cmps_handle_t h, const float\* audio_dev, int n_audio, int B, int T, "
                     r"const float\* weight_dev, long long ldw,\s*float\* grad_dev, void\* stream\);", header, flags=re.M)
    events = header[header.index("CMPS_OPT_KERNEL_EVENTS = 2"):]
    events = events[:events.index("*/")]
    assert "k_classify_weights" in events
    c = ctypes
    assert hip_lib.cmps_bank_classify_weights.argtypes[2:5] == [c.c_int, c.c_int, c.c_longlong]
    assert hip_lib.cmps_bank_classify_weights.argtypes[6:10] == [c.c_double, c.c_double, c.c_double, c.c_int]
    assert hip_lib.cmps_bank_classify_weights.argtypes[11] == c.c_longlong
    assert hip_lib.cmps_bank_loss_bwd_weighted.argtypes[2:5] == [c.c_int] * 3 and hip_lib.cmps_bank_loss_bwd_weighted.argtypes[6] == c.c_longlong
    assert hip_lib.cmps_version() == 500


def test_the_record_dtype_is_the_headers_layout():
    from audio_mps_amd import _capi
    want = [("sum_xent", 0, "<f8"), ("sum_own_loss", 8, "<f8"), ("n_used", 16, "<i8"), ("n_unlabelled", 24, "<i8"), ("n_own_absent", 32, "<i8")]
    dt = _capi.CLASSIFY_WEIGHTS_REC
    assert dt.itemsize == 40 and list(dt.names) == [w[0] for w in want]
    for name, off, kind in want:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind), name
    header = _header()
    block = header[header.index("cmps_bank_classify_weights_rec below"):header.index("} cmps_bank_classify_weights_rec;")]
    for name, off, _ in want:                                                           # the table of the header: offset, type, field
        assert re.search(r"^\s*\*\s+%d\s+(double|long long)\s+%s\b" % (off, name), block, flags=re.M), name
    assert re.search(r"double sum_xent, sum_own_loss;\s*long long n_used, n_unlabelled, n_own_absent;", block)
    import _disc_ref
    assert _disc_ref.FIELDS == dt.names


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_classify_weights_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_bank_classify_weights(None, PTR, 3, 4, 4, PTR3, 1.0, 0.0, 1.0, 1, PTR4, 4, PTR2, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def bad(names, loss=PTR, M=3, B=4, ld=4, label=PTR3, kappa=1.0, alpha=0.0, beta=1.0, reset=1, weight=PTR4, ldw=4, rec=PTR2):
            assert lib.cmps_bank_classify_weights(h, loss, M, B, ld, label, kappa, alpha, beta, reset, weight, ldw, rec, None) == BAD
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_bank_classify_weights:") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        bad(["loss_dev"], loss=None)
        bad(["label_dev"], label=None)
        bad(["weight_dev"], weight=None)
        bad(["record_dev"], rec=None)
        for off in (1, 2, 4, 7):
            bad(["record_dev", "aligned"], rec=PTR2 + off)
        for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
            bad(["M"], M=M)
        for B in (0, -1, -2 ** 31):
            bad(["B"], B=B)
        for ld in (3, 0, -1, -2 ** 63):
            bad(["ld", "B"], ld=ld)
        for ldw in (3, 0, -1, -2 ** 63):
            bad(["ldw", "B"], ldw=ldw)
        for k in (0.0, -0.0, -1.0, NAN, INF, -INF):
            bad(["inv_temp"], kappa=k)
        for x in (-1e-300, -1.0, NAN, INF, -INF):
            bad(["gen_weight"], alpha=x)
            bad(["disc_weight"], beta=x)
        # the first failing check speaks: the pointers in the order loss, label, weight, record (null, then alignment), M, B, ld, ldw,
        # inv_temp, gen_weight, disc_weight -- whatever reset
        for reset in (0, 1):
            rest = dict(M=0, B=0, ld=-1, ldw=-1, kappa=NAN, alpha=-1.0, beta=-1.0, reset=reset)
            bad(["loss_dev"], loss=None, label=None, weight=None, rec=None, **rest)
            bad(["label_dev"], label=None, weight=None, rec=None, **rest)
            bad(["weight_dev"], weight=None, rec=None, **rest)
            bad(["record_dev"], rec=None, **rest)
            bad(["record_dev", "aligned"], rec=PTR2 + 4, **rest)
            bad(["M"], **rest)
            bad(["B"], **{**rest, "M": 3})
            bad(["ld"], **{**rest, "M": 3, "B": 4, "ld": 3})
            bad(["ldw"], **{**rest, "M": 3, "B": 4, "ld": 4, "ldw": 3})
            bad(["inv_temp"], kappa=NAN, alpha=-1.0, beta=-1.0, reset=reset)
            bad(["gen_weight"], alpha=-1.0, beta=-1.0, reset=reset)
            bad(["disc_weight"], beta=-1.0, reset=reset)
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("D,variant", [(3, 0), (17, 0), (7, 1)])
def test_weighted_backward_bad_arguments_and_state_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    lib = hip_lib
    assert lib.cmps_bank_loss_bwd_weighted(None, PTR, 1, 4, 16, PTR2, 4, PTR3, None) == _capi.CMPS_ERR_BAD_ARG
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def call(weight=PTR2, ldw=4, B=4):
            rc = lib.cmps_bank_loss_bwd_weighted(h, PTR, 1, B, 16, weight, ldw, PTR3, None)
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_bank_loss_bwd_weighted:"), msg
            return rc, msg
        rc, msg = call(weight=None)
        assert rc == _capi.CMPS_ERR_BAD_ARG and "weight_dev" in msg
        rc, msg = call(weight=None, ldw=3)                                              # (the first failing check speaks)
        assert rc == _capi.CMPS_ERR_BAD_ARG and "weight_dev" in msg
        for ldw in (3, 0, -1, -2 ** 63):
            rc, msg = call(ldw=ldw)
            assert rc == _capi.CMPS_ERR_BAD_ARG and "ldw" in msg and "B" in msg
        # with its own two arguments in order it is cmps_bank_loss_bwd: no saved bank forward on this handle
        rc, msg = call()
        assert rc == _capi.CMPS_ERR_STATE and "cmps_bank_loss_fwd" in msg
    finally:
        lib.cmps_destroy(h)
