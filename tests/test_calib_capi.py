"""cmps_bank_calibrate at the C ABI without a GPU: the symbols, the prototype in the header, the argtypes, the record's layout, the scratch
size, and every CMPS_ERR_BAD_ARG of its contract, returned before the device is touched with a message that starts with the entry's name
and names the argument -- the first failing check speaking, in the order include/cmps.h states them (the convention of
tests/test_posterior_capi.py).  Nothing is launched on an error: with CMPS_OPT_KERNEL_EVENTS on, no kernel is recorded.  The kernels are
tested in tests/test_gpu_calibrate.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4, PTR5 = 4096, 8192, 12288, 16384, 20480      # non-null "device pointers": every call below returns before they are looked at


def header():
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        return f.read()


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    text = header()
    for name in ("cmps_bank_calibrate", "cmps_bank_calibrate_scratch_bytes"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
    assert re.search(r"^size_t cmps_bank_calibrate_scratch_bytes\(int M, long long N\);", text, flags=re.M)
    assert re.search(r"^int cmps_bank_calibrate\(cmps_handle_t h, const float\* loss_dev, int M, long long N, long long ld, const int\* label_dev,\s*"
                     r"int fit, int max_iter, double tol, double kappa_min, double kappa_max,\s*"
                     r"double\* theta_dev, void\* record_dev, void\* scratch_dev, size_t scratch_bytes, void\* stream\);", text, flags=re.M)
    assert re.search(r"enum \{ CMPS_CALIB_TEMPERATURE = 1, CMPS_CALIB_PRIOR = 2 \};", text)
    assert (_capi.CMPS_CALIB_TEMPERATURE, _capi.CMPS_CALIB_PRIOR) == (1, 2)
    assert (_capi.CALIB_CONVERGED, _capi.CALIB_AT_KAPPA_MIN, _capi.CALIB_AT_KAPPA_MAX, _capi.CALIB_NO_DATA, _capi.CALIB_MAX_ITER) == (1, 2, 4, 8, 16)
    events = text[text.index("CMPS_OPT_KERNEL_EVENTS = 2"):]
    events = events[:events.index("*/")]
    assert "k_calib_pass" in events and "k_calib_update" in events
    c = ctypes
    at = hip_lib.cmps_bank_calibrate.argtypes
    assert len(at) == 16 and at[2:5] == [c.c_int, c.c_longlong, c.c_longlong] and at[6:11] == [c.c_int, c.c_int, c.c_double, c.c_double, c.c_double]
    assert at[14] == c.c_size_t and hip_lib.cmps_bank_calibrate_scratch_bytes.argtypes == [c.c_int, c.c_longlong]
    assert hip_lib.cmps_bank_calibrate_scratch_bytes.restype == c.c_size_t
    assert hip_lib.cmps_version() == 500


def test_the_record_is_the_headers_struct():
    from audio_mps_amd import _capi
    dt = _capi.CALIB_REC
    want = [("xent_start", 0, "<f8"), ("xent_end", 8, "<f8"), ("g_logk", 16, "<f8"), ("resid_prior", 24, "<f8"), ("curvature", 32, "<f8"),
            ("n_used", 40, "<i8"), ("n_unlabelled", 48, "<i8"), ("n_own_absent", 56, "<i8"), ("passes", 64, "<i4"), ("flags", 68, "<i4"),
            ("n_unfitted", 72, "<i4"), ("reserved", 76, "<i4")]
    assert dt.itemsize == 80 and list(dt.names) == [w[0] for w in want]
    for name, off, kind in want:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind), name
    struct = re.search(r"typedef struct cmps_bank_calibrate_rec \{(.*?)\} cmps_bank_calibrate_rec;", header(), flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"^\s*(double|long long|int)\s+([\w, ]+);", struct, flags=re.M):
        fields += [(kind, n.strip()) for n in names.split(",")]
    kinds = {"<f8": "double", "<i8": "long long", "<i4": "int"}
    assert fields == [(kinds[k], n) for n, _, k in want]


def test_scratch_bytes(hip_lib):
    size = hip_lib.cmps_bank_calibrate_scratch_bytes
    for M, N in ((0, 5), (-1, 5), (1025, 5), (3, 0), (3, -1), (3, -2 ** 63), (1024, 2 ** 62), (2, 2 ** 61 + 1)):
        assert size(M, N) == 0, (M, N)
    assert size(1, 1) > 0 and size(1024, 2 ** 52) > 0
    assert size(5, 300) % 8 == 0 and size(5, 300) >= 8 * (1 + 5) + 5 * 8 * (3 + 2 * 5)       # theta's copy and five tiles' sums at the least
    assert size(5, 64) < size(5, 65) <= size(5, 128)                                          # a row of sums per tile of 64 clips
    assert size(1024, 10 ** 9) == size(1024, 10 ** 12) < 64 * 2 ** 20                         # ... up to a fixed number of workgroups


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_bank_calibrate(None, PTR, 3, 7, 7, PTR2, 3, 10, 1e-9, 1e-6, 1e6, PTR3, PTR4, PTR5, 1 << 20, None) == BAD
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 1) == _capi.CMPS_OK

        def bad(names, loss=PTR, M=3, N=7, ld=9, label=PTR2, fit=3, max_iter=10, tol=1e-9, kmin=1e-6, kmax=1e6, theta=PTR3, record=PTR4,
                scratch=PTR5, nbytes=1 << 20):
            assert lib.cmps_bank_calibrate(h, loss, M, N, ld, label, fit, max_iter, tol, kmin, kmax, theta, record, scratch, nbytes, None) == BAD
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_bank_calibrate:") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        nan, inf = float("nan"), float("inf")
        bad(["loss_dev"], loss=None)
        bad(["label_dev"], label=None)
        for name, key, ptr in (("theta_dev", "theta", PTR3), ("record_dev", "record", PTR4), ("scratch_dev", "scratch", PTR5)):
            bad([name, "null"], **{key: None})
            for off in (1, 2, 4, 7):
                bad([name, "aligned"], **{key: ptr + off})
        for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
            bad(["M"], M=M)
        for N in (0, -1, -2 ** 63):
            bad(["N"], N=N)
        bad(["M", "ld"], M=1024, N=7, ld=2 ** 52 + 1)
        bad(["M", "ld"], M=3, N=7, ld=2 ** 62)
        for ld in (6, 0, -1):
            bad(["ld", "N"], ld=ld)
        for fit in (-1, 4, 2 ** 31 - 1):
            bad(["fit"], fit=fit)
        for max_iter in (-1, 10001, -2 ** 31):
            bad(["max_iter"], max_iter=max_iter)
        for v in (0.0, -1.0, nan, inf, -inf):
            bad(["tol"], tol=v)
            bad(["kappa_min"], kmin=v)
        for v in (nan, inf, -inf, 0.0, 0.5e-6):
            bad(["kappa_max"], kmax=v)
        need = lib.cmps_bank_calibrate_scratch_bytes(3, 7)
        for nbytes in (0, 8, need - 1):
            bad(["scratch_bytes"], nbytes=nbytes)
        # the first failing check speaks, in the header's order
        worse = dict(label=None, theta=PTR3 + 4, record=None, scratch=PTR5 + 2, M=0, N=0, ld=-1, fit=9, max_iter=-1, tol=nan, kmin=nan, kmax=nan,
                     nbytes=0)
        order = [("loss_dev", dict(loss=None)), ("label_dev", dict(label=PTR2)), ("theta_dev", dict(theta=PTR3)), ("record_dev", dict(record=PTR4)),
                 ("scratch_dev", dict(scratch=PTR5)), ("M", dict(M=3)), ("N", dict(N=7)), ("ld", dict(ld=7)), ("fit", dict(fit=0)),
                 ("max_iter", dict(max_iter=0)), ("tol", dict(tol=1.0)), ("kappa_min", dict(kmin=1.0)), ("kappa_max", dict(kmax=1.0)),
                 ("scratch_bytes", dict())]
        fixed = dict(worse)
        for name, fix in order:
            if name == "loss_dev":
                bad([name], **dict(fixed, **fix))
                continue
            bad([name], **fixed)
            fixed.update(fix)
        # nothing was launched: no kernel has been recorded on this handle
        names = ctypes.create_string_buffer(4096)
        ms, counts = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
        assert lib.cmps_kernel_times(h, names, 4096, ms, counts, 64) == 0
    finally:
        lib.cmps_destroy(h)
