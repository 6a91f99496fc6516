"""k_bank_posterior on a real MI355X against tests/_posterior_ref.py at the C ABI, in guarded buffers (tests/_guard.py): every output
between two red zones, every input compared with its snapshot after the call.  Synthetic nll, no model: the draws are
`_posterior_ref.cases()`, which tests/test_posterior_host.py has shown to be well-posed (no step within 1e-9 of a threshold, no runner-up
within 1e-9 of the best), so `best` and the decision records must EQUAL the restatement's; `total_out` must equal the float32 loop bit
for bit; `post` and `conf` must lie within twice the bound include/cmps.h states for cmps_bank_posterior (ROUNDING):
  |post - exact| <= 2^-24 |exact| + 2^-52 (M + 16 + 4 A') + 2^-149.
"""
import ctypes

import numpy as np
import pytest
import torch

import _guard as G
import _posterior_ref as PR

pytestmark = pytest.mark.gpu

CASES = PR.cases()
IDS = [c[0] for c in CASES]
OUTPUTS = ("total_out", "post", "best", "conf", "decision")
DTYPE = {"total_out": np.float32, "post": np.float32, "best": np.int32, "conf": np.float32, "decision": PR.DECISION}


class _Lib:
    """One libcmps handle on the current device and stream, every pointer a Guarded's."""

    def __init__(self, D=8, events=False):
        from audio_mps_amd import _capi
        self.capi, self.lib = _capi, _capi.load()
        self.dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.h = ctypes.c_void_p()
        assert self.lib.cmps_create(D, ctypes.byref(self.h)) == _capi.CMPS_OK
        if events:
            assert self.lib.cmps_set_option(self.h, _capi.CMPS_OPT_KERNEL_EVENTS, 1) == _capi.CMPS_OK

    def close(self):
        self.lib.cmps_destroy(self.h)

    def guarded(self, nbytes, name, fill=G.NAN_FILL):
        return G.Guarded(nbytes, self.dev, align=256, fill=fill, name=name)

    def const(self, x, name):
        g = self.guarded(x.nbytes, name)
        g.load(x)
        g.snapshot(x)
        return g

    def call(self, kw, lo=0, hi=None, total_in="kw", decision=None, reset=1, want=OUTPUTS, fill=G.NAN_FILL, in_place=False):
        """cmps_bank_posterior over steps lo .. hi of the case ``kw`` -> {output: array}.  ``total_in``: the case's own ("kw"), None, or
        an array [M, n]; ``decision``: records to continue (uploaded into the output buffer); ``in_place``: total_out_dev == total_in_dev."""
        nll = np.ascontiguousarray(kw["nll"][:, :, lo:hi])
        M, n, steps = nll.shape
        total = kw["total_in"] if isinstance(total_in, str) else total_in
        ins = {"nll": self.const(nll, "nll")}
        if total is not None and not in_place:
            ins["total_in"] = self.const(np.ascontiguousarray(total, dtype=np.float32), "total_in")
        if kw["log_prior"] is not None:
            ins["log_prior"] = self.const(np.ascontiguousarray(kw["log_prior"], dtype=np.float64), "log_prior")
        size = {"total_out": 4 * M * n, "post": 4 * M * n * steps, "best": 4 * n * steps, "conf": 4 * n * steps, "decision": 16 * n}
        outs = {k: self.guarded(size[k], k, fill) for k in want}
        if in_place:
            assert total is not None and "total_out" in outs
            outs["total_out"].load(np.ascontiguousarray(total, dtype=np.float32))
        if decision is not None:
            outs["decision"].load(np.ascontiguousarray(decision, dtype=PR.DECISION))
        ptr = lambda d, k: d[k].ptr if k in d else None                                # noqa: E731
        t_in = outs["total_out"].ptr if in_place else ptr(ins, "total_in")
        thr = kw["threshold"] if "decision" in outs else float("nan")                  # (not read without a record)
        code = self.lib.cmps_bank_posterior(self.h, ins["nll"].ptr, M, n, steps, t_in, ptr(ins, "log_prior"), float(kw["inv_temp"]),
                                            ptr(outs, "total_out"), ptr(outs, "post"), ptr(outs, "best"), ptr(outs, "conf"), thr,
                                            kw["first_step"] + lo, reset, ptr(outs, "decision"),
                                            ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        assert code == self.capi.CMPS_OK, self.lib.cmps_last_error(self.h)
        torch.cuda.synchronize(self.dev)
        for g in ins.values():
            assert g.zones_intact() is None and g.equals_snapshot() is None, g.name
        res = {}
        for k, g in outs.items():
            assert g.zones_intact() is None, (k, g.zones_intact())
            if fill == G.NAN_FILL and k != "decision":
                assert not bool(g.untouched_mask(torch.float32).any()), f"{k}: an element was never written"
            res[k] = g.numpy(DTYPE[k])
        shape = {"total_out": (M, n), "post": (M, n, steps), "best": (n, steps), "conf": (n, steps), "decision": (n,)}
        return {k: v.reshape(shape[k]) for k, v in res.items()}


@pytest.fixture(scope="module")
def lib():
    x = _Lib()
    yield x
    x.close()


@pytest.fixture(scope="module")
def refs():
    """The restatement of every case, computed once and left unchanged."""
    return {name: PR.posterior(**kw) for name, kw in CASES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, int(np.sum(_bits(a[k]) != _bits(b[k]))))


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_against_the_restatement(lib, refs, name, kw):
    ref, got = refs[name], lib.call(kw)
    M = kw["nll"].shape[0]
    assert np.array_equal(_bits(got["total_out"]), _bits(ref["total_out"])), "total_out is the float32 loop, bit for bit"
    for key, exact, scale in (("post", ref["post64"], ref["scale"][None]), ("conf", ref["conf64"], ref["scale"])):
        bar = 2.0 * PR.bound(exact, M, scale)
        err = np.abs(got[key].astype(np.float64) - ref[key].astype(np.float64))
        print(f"{name}: {key} worst error {err.max():.3e}, worst error / (2 x bound) {float((err / bar).max()):.3f}")
        assert np.all(err <= bar), (key, float(err.max()), float((err / bar).max()))
        assert not np.signbit(got[key]).any(), key                                     # an absent member, an empty step: +0
    assert np.array_equal(got["best"], ref["best"])
    assert np.array_equal(got["decision"], ref["decision"]), (got["decision"], ref["decision"])
    absent = ~np.isfinite(ref["c"])
    assert not got["post"][absent].any()


@pytest.mark.parametrize("name,kw", [c for c in CASES if c[1]["nll"].shape[2] >= 5], ids=[i for i, c in zip(IDS, CASES) if c[1]["nll"].shape[2] >= 5])
def test_a_cut_changes_no_bit(lib, name, kw):
    whole = lib.call(kw)
    steps = kw["nll"].shape[2]
    edges = [0] + PR.cuts(steps) + [steps]
    total, rec, parts = kw["total_in"], None, []
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        part = lib.call(kw, a, b, total_in=total, decision=rec, reset=int(rec is None), in_place=i % 2 == 1)
        total, rec = part["total_out"], part["decision"]
        parts.append(part)
    for key in ("post", "best", "conf"):
        assert np.array_equal(_bits(np.concatenate([p[key] for p in parts], axis=-1)), _bits(whole[key])), key
    assert np.array_equal(_bits(total), _bits(whole["total_out"])) and np.array_equal(rec, whole["decision"])


def test_resumed_totals_are_total_in_plus_the_fold(lib, refs):
    name, kw = CASES[IDS.index("5x3x130-prior")]
    got = lib.call(kw, want=("total_out",))
    assert np.array_equal(_bits(got["total_out"]), _bits(PR.fold(kw["nll"], kw["total_in"])[:, :, -1]))
    zero = lib.call(kw, total_in=None, want=("total_out",))
    assert np.array_equal(_bits(zero["total_out"]), _bits(PR.fold(kw["nll"])[:, :, -1]))
    assert not np.array_equal(got["total_out"], zero["total_out"])


def test_null_outputs_are_not_written_and_null_inputs_mean_zeros(lib):
    name, kw = CASES[IDS.index("5x3x130-prior")]
    full = lib.call(kw)
    for leave in OUTPUTS:
        want = tuple(k for k in OUTPUTS if k != leave)
        _same(lib.call(kw, want=want), {k: full[k] for k in want}, f"without {leave}")
    for only in OUTPUTS:
        _same(lib.call(kw, want=(only,)), {only: full[only]}, f"only {only}")
    M, n, _ = kw["nll"].shape
    plain = dict(kw, total_in=None, log_prior=None)
    zeros = dict(kw, total_in=np.zeros((M, n), np.float32), log_prior=np.zeros(M))
    _same(lib.call(plain), lib.call(zeros), "NULL total_in / log_prior against explicit zeros")
    shifted = dict(kw, log_prior=kw["log_prior"] + 3.25)                                # a common shift of the log prior: the same best
    assert np.array_equal(lib.call(shifted)["best"], full["best"])


def test_two_runs_give_the_same_bits_whatever_the_buffers_held(lib):
    for name in ("5x3x130-prior", "1024x1x40-uniform", "planted"):
        kw = CASES[IDS.index(name)][1]
        _same(lib.call(kw), lib.call(kw), name)
        _same(lib.call(kw), lib.call(kw, fill=G.ZERO_FILL), name + " (zero-filled buffers)")


def test_the_decision_record_resets_continues_and_is_left_alone(lib, refs):
    name, kw = CASES[IDS.index("5x3x130-uniform")]
    ref = refs[name]["decision"]
    assert np.all(ref["step"] >= 0)
    held = PR.fresh_decision(3)
    held["step"], held["member"], held["reserved"] = [7, -1, 10 ** 12], [4, -1, 0], [0, 0, 0]
    got = lib.call(kw, decision=held, reset=0)["decision"]                             # decided paths are left alone, path 1 is decided now
    assert got["step"].tolist() == [7, int(ref["step"][1]), 10 ** 12] and got["member"].tolist() == [4, int(ref["member"][1]), 0]
    dirty = np.frombuffer(np.random.default_rng(5).bytes(48), PR.DECISION)
    assert np.array_equal(lib.call(kw, decision=dirty, reset=1)["decision"], ref)      # reset: whatever the record held
    tie = CASES[IDS.index("tie-3")][1]                                                 # two members tie all along: nobody is ever sure
    never = lib.call(tie, decision=dirty[:2], reset=1)["decision"]
    assert never["step"].tolist() == [-1] * 2 and never["member"].tolist() == [-1] * 2 and never["reserved"].tolist() == [0] * 2


@pytest.mark.parametrize("D,variant", [(20, 0), (128, 1)])
def test_any_handle_will_do_and_the_launch_is_recorded(D, variant):
    from audio_mps_amd import _capi
    x = _Lib(D, events=True)
    try:
        assert x.lib.cmps_set_variant(x.h, variant) == _capi.CMPS_OK
        name, kw = CASES[IDS.index("65x2x40-prior")]
        got = x.call(kw)
        names = ctypes.create_string_buffer(2048)
        ms, counts = (ctypes.c_float * 8)(), (ctypes.c_int * 8)()
        assert x.lib.cmps_kernel_times(x.h, names, 2048, ms, counts, 8) == 1
        assert names.value.decode() == "k_bank_posterior" and counts[0] == 1 and ms[0] > 0
    finally:
        x.close()
    y = _Lib()
    try:
        _same(got, y.call(kw), "a handle of another D")
    finally:
        y.close()
