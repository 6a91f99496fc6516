"""cmps_bank_posterior at the C ABI without a GPU: the symbol, the decision record's layout, and every CMPS_ERR_BAD_ARG of its contract,
returned before the device is touched with a message that starts with the entry's name and names the argument -- the first failing check
speaking, in the order include/cmps.h states them (the convention of tests/test_classify_capi.py).  Nothing is launched on an error: with
CMPS_OPT_KERNEL_EVENTS on, no kernel is recorded.  The kernel is tested in tests/test_gpu_posterior.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4, PTR5 = 4096, 8192, 12288, 16384, 20480      # non-null "device pointers": every call below returns before they are looked at


def test_symbol_is_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    assert "cmps_bank_posterior" in _capi.SYMBOLS and hasattr(hip_lib, "cmps_bank_posterior")
    assert re.search(r"^int cmps_bank_posterior\(cmps_handle_t h, const float\* nll_dev, int M, int n, int steps,\s*"
                     r"const float\* total_in_dev, const double\* log_prior_dev, double inv_temp,\s*"
                     r"float\* total_out_dev, float\* post_dev, int\* best_dev, float\* conf_dev,\s*"
                     r"double threshold, long long first_step, int reset, void\* decision_dev, void\* stream\);", header, flags=re.M)
    events = header[header.index("CMPS_OPT_KERNEL_EVENTS = 2"):]
    events = events[:events.index("*/")]
    assert "k_bank_posterior" in events
    c = ctypes
    assert hip_lib.cmps_bank_posterior.argtypes[2:5] == [c.c_int, c.c_int, c.c_int]
    assert hip_lib.cmps_bank_posterior.argtypes[7] == c.c_double
    assert hip_lib.cmps_bank_posterior.argtypes[12:15] == [c.c_double, c.c_longlong, c.c_int]
    assert len(hip_lib.cmps_bank_posterior.argtypes) == 17
    assert hip_lib.cmps_version() == 500


def test_the_decision_record_is_the_headers_struct():
    from audio_mps_amd import _capi
    dt = _capi.DECISION_REC
    want = [("step", 0, "<i8"), ("member", 8, "<i4"), ("reserved", 12, "<i4")]
    assert dt.itemsize == 16 and list(dt.names) == [w[0] for w in want]
    for name, off, kind in want:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind), name
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    struct = re.search(r"typedef struct cmps_bank_decision \{(.*?)\} cmps_bank_decision;", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(long long|int)\s+(\w+);", struct, flags=re.M)
    assert fields == [("long long", "step"), ("int", "member"), ("int", "reserved")]


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_bank_posterior(None, PTR, 3, 2, 5, None, None, 1.0, PTR2, None, PTR3, PTR4, 0.9, 0, 1, PTR5, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
        assert lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 1) == _capi.CMPS_OK

        def bad(names, nll=PTR, M=3, n=2, steps=5, total_in=None, log_prior=None, inv_temp=1.0, total_out=PTR2, post=None, best=PTR3,
                conf=PTR4, threshold=0.9, first_step=0, reset=1, decision=PTR5):
            assert lib.cmps_bank_posterior(h, nll, M, n, steps, total_in, log_prior, inv_temp, total_out, post, best, conf, threshold,
                                           first_step, reset, decision, None) == BAD
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_bank_posterior:") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        nan, inf = float("nan"), float("inf")
        bad(["nll_dev"], nll=None)
        for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
            bad(["M"], M=M)
        for n in (0, -1, -2 ** 31):
            bad(["n"], n=n)
        for steps in (0, -1, -2 ** 31):
            bad(["steps"], steps=steps)
        bad(["M", "n", "steps"], M=1024, n=2 ** 11, steps=2 ** 10)                    # 2^31
        bad(["M", "n", "steps"], M=1, n=2 ** 31 - 1, steps=2)
        bad(["M", "n", "steps"], M=3, n=2 ** 31 - 1, steps=2 ** 31 - 1)
        for kappa in (0.0, -1.0, nan, inf, -inf):
            bad(["inv_temp"], inv_temp=kappa)
        for off in (1, 2, 4, 7):
            bad(["log_prior_dev", "aligned"], log_prior=PTR2 + off)
            bad(["decision_dev", "aligned"], decision=PTR5 + off)
        for thr in (0.0, -0.5, 1.0000001, 2.0, nan, inf, -inf):
            bad(["threshold"], threshold=thr)
        for first in (-1, -2 ** 63):
            bad(["first_step"], first_step=first)
        bad(["first_step", "steps"], first_step=2 ** 63 - 1, steps=1)                  # first_step + steps = 2^63
        bad(["first_step", "steps"], first_step=2 ** 63 - 5)
        # the first failing check speaks: nll_dev, M, n, steps, the product, inv_temp, the two alignments, threshold, the step range --
        # whatever reset and the optional pointers
        for reset, total_in, post in ((0, PTR3, PTR4), (1, None, None)):
            kw = dict(reset=reset, total_in=total_in, post=post)
            worse = dict(inv_temp=nan, log_prior=PTR2 + 4, decision=PTR5 + 4, threshold=nan, first_step=-1)
            bad(["nll_dev"], nll=None, M=0, n=0, steps=0, **worse, **kw)
            bad(["M"], M=0, n=0, steps=0, **worse, **kw)
            bad(["n"], n=0, steps=0, **worse, **kw)
            bad(["steps"], steps=0, **worse, **kw)
            bad(["M", "n", "steps"], M=1024, n=2 ** 11, steps=2 ** 10, **worse, **kw)
            bad(["inv_temp"], **worse, **kw)
            bad(["log_prior_dev"], **dict(worse, inv_temp=1.0), **kw)
            bad(["decision_dev"], **dict(worse, inv_temp=1.0, log_prior=PTR2), **kw)
            bad(["threshold"], **dict(worse, inv_temp=1.0, log_prior=PTR2, decision=PTR5), **kw)
            bad(["first_step"], **dict(worse, inv_temp=1.0, log_prior=PTR2, decision=PTR5, threshold=1.0), **kw)
        # nothing was launched: no kernel has been recorded on this handle
        names = ctypes.create_string_buffer(4096)
        ms, counts = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
        assert lib.cmps_kernel_times(h, names, 4096, ms, counts, 64) == 0
    finally:
        lib.cmps_destroy(h)
