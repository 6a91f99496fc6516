"""cmps_loss_stats and cmps_batch_gather_i16 at the C ABI without a GPU: the symbols, the record's layout, and every CMPS_ERR_BAD_ARG of
their contracts, returned before the device is touched with a message that starts with the entry's name and names the argument -- the first
failing check speaking (the convention of tests/test_data_capi.py).  The kernels themselves are tested in tests/test_gpu_loss_stats.py and
tests/test_gpu_gather_i16.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2, PTR3 = 4096, 8192, 12288      # non-null "device pointers": every call below must return before anything looks at them


def test_symbols_are_declared_exported_and_in_the_header(hip_lib):
    from audio_mps_amd import _capi
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name in ("cmps_loss_stats", "cmps_batch_gather_i16"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name)
    assert re.search(r"^int cmps_loss_stats\(cmps_handle_t h, const float\* loss_dev, int B, long long first_id,\s*"
                     r"int reset, void\* stats_dev, void\* stream\);", header, flags=re.M)
    assert re.search(r"^int cmps_batch_gather_i16\(cmps_handle_t h, const short\* data_dev, long long n_clips, long long clip_len,\s*"
                     r"const int\* index_dev, const int\* offset_dev, int B, int T, float scale,\s*float\* audio_dev, void\* stream\);",
                     header, flags=re.M)
    assert "k_loss_stats" in header and "k_batch_gather_i16" in header                  # CMPS_OPT_KERNEL_EVENTS names them
    events = header[header.index("CMPS_OPT_KERNEL_EVENTS = 2"):]
    events = events[:events.index("*/")]
    assert "k_loss_stats" in events and "k_batch_gather_i16" in events
    assert hip_lib.cmps_loss_stats.argtypes[2:5] == [ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    assert hip_lib.cmps_batch_gather_i16.argtypes[2:4] == [ctypes.c_longlong, ctypes.c_longlong]
    assert hip_lib.cmps_batch_gather_i16.argtypes[8] == ctypes.c_float
    assert hip_lib.cmps_version() == 500


def test_the_record_dtype_is_the_headers_layout():
    from audio_mps_amd import _capi
    want = [("sum", 0, "<f8"), ("sumsq", 8, "<f8"), ("n_finite", 16, "<i8"), ("n_nonfinite", 24, "<i8"), ("argmin", 32, "<i8"),
            ("argmax", 40, "<i8"), ("first_nonfinite", 48, "<i8"), ("min", 56, "<f4"), ("max", 60, "<f4")]
    dt = _capi.LOSS_STATS
    assert dt.itemsize == 64 and list(dt.names) == [w[0] for w in want]
    for name, off, kind in want:
        assert dt.fields[name][1] == off and dt.fields[name][0] == np.dtype(kind), name
    with open(os.path.join(ROOT, "include", "cmps.h")) as f:
        header = f.read()
    for name, off, _ in want:                                                           # the table of the header: offset, type, field
        assert re.search(r"^\s*\*\s+%d\s+(double|long long|float)\s+%s\b" % (off, name), header, flags=re.M), name


@pytest.mark.parametrize("D,variant", [(1, 0), (20, 0), (48, 0), (128, 1)])
def test_bad_arguments_on_a_fresh_handle(hip_lib, D, variant):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    lib = hip_lib
    assert lib.cmps_loss_stats(None, PTR, 4, 0, 1, PTR2, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    assert lib.cmps_batch_gather_i16(None, PTR, 4, 8, PTR2, None, 2, 8, 2.0 ** -15, PTR3, None) == BAD
    assert b"handle" in lib.cmps_last_error(None)
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK

        def said(entry, names):
            msg = lib.cmps_last_error(h).decode()
            assert msg.startswith(entry + ":") and all(re.search(r"\b%s\b" % k, msg) for k in names), msg

        def stats(names, loss=PTR, B=4, first_id=0, reset=1, rec=PTR2):
            assert lib.cmps_loss_stats(h, loss, B, first_id, reset, rec, None) == BAD
            said("cmps_loss_stats", names)

        stats(["loss_dev"], loss=None)
        stats(["stats_dev"], rec=None)
        for off in (1, 2, 4, 7):
            stats(["stats_dev", "aligned"], rec=PTR2 + off)
        for B in (0, -1, -2 ** 31):
            stats(["B"], B=B)
        for first in (-1, -2 ** 63):
            stats(["first_id"], first_id=first)
        stats(["first_id", "B"], first_id=2 ** 63 - 1, B=1)                             # first_id + B = 2^63
        stats(["first_id", "B"], first_id=2 ** 63 - 2 ** 31 + 1, B=2 ** 31 - 1)
        stats(["first_id", "B"], first_id=2 ** 63 - 4, B=4)
        # the first failing check speaks: loss_dev, stats_dev (null, then alignment), B, the id range -- for either value of reset
        for reset in (0, 1):
            stats(["loss_dev"], loss=None, rec=None, B=0, first_id=-1, reset=reset)
            stats(["stats_dev"], rec=None, B=0, first_id=-1, reset=reset)
            stats(["stats_dev", "aligned"], rec=PTR2 + 4, B=0, first_id=-1, reset=reset)
            stats(["B"], B=0, first_id=-1, reset=reset)
            stats(["first_id"], first_id=-1, reset=reset)

        def gather(names, data=PTR, n_clips=4, clip_len=8, index=PTR2, offset=None, B=2, T=8, scale=2.0 ** -15, audio=PTR3):
            assert lib.cmps_batch_gather_i16(h, data, n_clips, clip_len, index, offset, B, T, scale, audio, None) == BAD
            said("cmps_batch_gather_i16", names)

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
        for scale in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            gather(["scale"], scale=scale)
        # the first failing check speaks: the order of cmps_batch_gather, and scale last
        gather(["data_dev"], data=None, index=None, audio=None, B=0, scale=0.0)
        gather(["index_dev"], index=None, audio=None, n_clips=0, scale=0.0)
        gather(["audio_dev"], audio=None, B=0, clip_len=1, scale=0.0)
        gather(["B", "T"], B=0, n_clips=0, clip_len=1, scale=0.0)
        gather(["n_clips"], n_clips=0, clip_len=1, scale=0.0)
        gather(["clip_len", "T"], clip_len=1, scale=float("nan"))
        # the messages are cmps_batch_gather's behind the entry's name
        for kw in ({"data": None}, {"B": 0}, {"n_clips": 0}, {"clip_len": 1}):
            gather([], **kw)
            mine = lib.cmps_last_error(h).decode()
            a = dict(data=PTR, n_clips=4, clip_len=8, index=PTR2, offset=None, B=2, T=8, audio=PTR3)
            a.update(kw)
            assert lib.cmps_batch_gather(h, a["data"], a["n_clips"], a["clip_len"], a["index"], a["offset"], a["B"], a["T"], a["audio"],
                                         None) == BAD
            theirs = lib.cmps_last_error(h).decode()
            assert mine.split(":", 1)[1] == theirs.split(":", 1)[1], (mine, theirs)
    finally:
        lib.cmps_destroy(h)
