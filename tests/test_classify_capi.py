"""cmps_bank_classify_stats at the C ABI without a GPU: the symbols, the record's layout, the record's size, and every CMPS_ERR_BAD_ARG of
its contract, returned before the device is touched with a message that starts with the entry's name and names the argument -- the first
failing check speaking (the convention of tests/test_eval_capi.py).  The kernel is tested in tests/test_gpu_classify_stats.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3, PTR4 = 4096, 8192, 12288, 16384      # non-null "device pointers": every call below must return before anything looks at them


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in ("cmps_bank_classify_stats", "cmps_bank_classify_stats_bytes"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
    assert re.search(r"^size_t cmps_bank_classify_stats_bytes\(int M\);", header, flags=re.M)
    assert re.search(r"^int cmps_bank_classify_stats\(cmps_handle_t h, const float\* loss_dev, int M, int B, long long ld,\s*"
                     r"const int\* label_dev, long long first_id, int reset,\s*void\* stats_dev, int\* best_dev, void\* stream\);",
                     header, flags=re.M)
    events = header[header.index("CMPS_OPT_KERNEL_EVENTS = 2"):]
    events = events[:events.index("*/")]
    assert "k_classify_stats" in events
    assert hip_lib.cmps_bank_classify_stats.argtypes[2:5] == [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    assert hip_lib.cmps_bank_classify_stats.argtypes[6:8] == [ctypes.c_longlong, ctypes.c_int]
    assert hip_lib.cmps_version() == 500


def test_the_record_dtype_is_the_headers_layout():
    from audio_mps_amd import _capi
    want = [("sum_xent", 0, "<f8"), ("sum_margin", 8, "<f8"), ("n_decided", 16, "<i8"), ("n_undecided", 24, "<i8"),
            ("n_unlabelled", 32, "<i8"), ("n_correct", 40, "<i8"), ("n_xent", 48, "<i8"), ("n_margin", 56, "<i8"), ("first_undecided", 64, "<i8")]
    dt = _capi.CLASSIFY_HEAD
    assert dt.itemsize == 72 and list(dt.names) == [w[0] for w in want]
    for name, off, kind in want:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind), name
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name, off, _ in want:                                                           # the table of the header: offset, type, field
        assert re.search(r"^\s*\*\s+%d\s+(double|long long)\s+%s\b" % (off, name), header, flags=re.M), name
    assert re.search(r"^\s*\*\s+72\s+long long\s+confusion\[M\]\[M\]", header, flags=re.M)
    for M in (1, 3, 1024):
        whole = _capi.classify_stats_dtype(M)
        assert whole.itemsize == 72 + 8 * M * M + 8 * M
        assert whole.fields["confusion"][1] == 72 and whole.fields["unlabelled_best"][1] == 72 + 8 * M * M
    for M in (0, 1025):
        with pytest.raises(ValueError):
            _capi.classify_stats_dtype(M)


def test_the_records_size(hip_lib):
    want = {0: 0, 1: 72 + 8 + 8, 2: 72 + 32 + 16, 1024: 72 + 8 * 1024 * 1024 + 8 * 1024, 1025: 0, -1: 0}
    for M, n in want.items():
        assert hip_lib.cmps_bank_classify_stats_bytes(M) == n, M


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_bank_classify_stats(None, PTR, 3, 4, 4, PTR3, 0, 1, PTR2, PTR4, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def bad(names, loss=PTR, M=3, B=4, ld=4, label=PTR3, first_id=0, reset=1, rec=PTR2, best=PTR4):
            assert lib.cmps_bank_classify_stats(h, loss, M, B, ld, label, first_id, reset, rec, best, None) == BAD
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith("cmps_bank_classify_stats:") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        bad(["loss_dev"], loss=None)
        bad(["stats_dev"], rec=None)
        for off in (1, 2, 4, 7):
            bad(["stats_dev", "aligned"], rec=PTR2 + off)
        for M in (0, -1, 1025, 2 ** 31 - 1, -2 ** 31):
            bad(["M"], M=M)
        for B in (0, -1, -2 ** 31):
            bad(["B"], B=B)
        for ld in (3, 0, -1, -2 ** 63):
            bad(["ld", "B"], ld=ld)
        for first in (-1, -2 ** 63):
            bad(["first_id"], first_id=first)
        bad(["first_id", "B"], first_id=2 ** 63 - 1, B=1, ld=1)                        # first_id + B = 2^63
        bad(["first_id", "B"], first_id=2 ** 63 - 4)
        # the first failing check speaks: loss_dev, stats_dev (null, then alignment), M, B, ld, the id range -- whatever reset, labels and best
        for reset, label, best in ((0, PTR3, PTR4), (1, None, None)):
            kw = dict(reset=reset, label=label, best=best)
            bad(["loss_dev"], loss=None, rec=None, M=0, B=0, ld=-1, first_id=-1, **kw)
            bad(["stats_dev"], rec=None, M=0, B=0, ld=-1, first_id=-1, **kw)
            bad(["stats_dev", "aligned"], rec=PTR2 + 4, M=0, B=0, ld=-1, first_id=-1, **kw)
            bad(["M"], M=0, B=0, ld=-1, first_id=-1, **kw)
            bad(["B"], B=0, ld=-1, first_id=-1, **kw)
            bad(["ld"], ld=3, first_id=-1, **kw)
            bad(["first_id"], first_id=-1, **kw)
    finally:
        lib.cmps_destroy(h)
