"""An independent restatement of cmps_bank_posterior (include/cmps.h) in numpy: the running totals by an explicit float32 loop over the
steps, the soft-max over the present members in float64 with its sums in member order, the decision rule and the header's rounding bound.
`cases()` are the draws tests/test_gpu_posterior.py feeds the kernel; tests/test_posterior_host.py asserts on every one of them the two
conditions that let the device's `best` and decision records be compared exactly (`ill_posed`).  `PosteriorEntries` is mixed into a
stand-in backend: HipScan's bank_stream_posterior answered from this file."""
import numpy as np

DECISION = np.dtype([("step", "<i8"), ("member", "<i4"), ("reserved", "<i4")])
MARGIN = 1e-9                 # how far a reference step stays from a threshold, and a runner-up from the best, to be compared exactly


def fold(nll, total_in=None):
    """``nll`` float32 [M, n, steps] -> the running totals c [M, n, steps]: ONE float32 addition per step, in step order."""
    x = np.asarray(nll, dtype=np.float32)
    assert x.ndim == 3 and x.dtype == np.float32
    c = np.empty_like(x)
    run = np.zeros(x.shape[:2], np.float32) if total_in is None else np.array(total_in, dtype=np.float32)
    assert run.shape == x.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[2]):
            run = (run + x[:, :, k]).astype(np.float32)
            c[:, :, k] = run
    return c


def fresh_decision(n):
    d = np.zeros(n, DECISION)
    d["step"], d["member"] = -1, -1
    return d


def posterior(nll, total_in=None, log_prior=None, inv_temp=1.0, threshold=None, first_step=0, decision=None, reset=True):
    """The definition: a dict of ``total_out`` float32 [M, n], ``c`` (the running totals), ``a`` float64 [M, n, steps] (+inf where a member
    cannot win), ``post64`` / ``post`` [M, n, steps], ``best`` int32 [n, steps], ``conf64`` / ``conf`` [n, steps], ``scale`` [n, steps] (A'
    of the rounding bound) and, with a threshold, ``decision`` [n] records continued from ``decision`` (reset False) or started afresh."""
    c = fold(nll, total_in)
    M, n, steps = c.shape
    kappa = float(inv_temp)
    lp = np.zeros(M, np.float64) if log_prior is None else np.asarray(log_prior, dtype=np.float64)
    assert lp.shape == (M,)
    present = np.isfinite(c)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(present, kappa * c.astype(np.float64) - lp[:, None, None], np.inf)
    amin = a.min(axis=0)                                              # [n, steps]
    some = amin < np.inf
    best = np.where(some, np.argmin(a, axis=0), -1).astype(np.int32)  # (argmin: the first, so the lowest m on ties)
    shift = np.where(some, amin, 0.0)
    e = np.zeros((M, n, steps), np.float64)
    S = np.zeros((n, steps), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(M):                                            # the sum in member order
            e[m] = np.where(a[m] < np.inf, np.exp(-(a[m] - shift)), 0.0)
            S = S + e[m]
        post64 = np.where(some[None], e / np.where(some, S, 1.0)[None], 0.0)
        conf64 = np.where(some, 1.0 / np.where(some, S, 1.0), 0.0)
        size = np.where(a < np.inf, kappa * np.abs(c.astype(np.float64)) + np.abs(lp)[:, None, None], 0.0)
    out = {"total_out": c[:, :, -1].copy(), "c": c, "a": a, "post64": post64, "post": (post64 + 0.0).astype(np.float32), "best": best,
           "conf64": conf64, "conf": (conf64 + 0.0).astype(np.float32), "scale": np.nan_to_num(size, nan=0.0, posinf=0.0).max(axis=0)}
    if threshold is not None:
        rec = fresh_decision(n) if (reset or decision is None) else np.array(decision, dtype=DECISION)
        for g in range(n):
            if rec["step"][g] >= 0:
                continue
            sure = np.flatnonzero(some[g] & (conf64[g] >= float(threshold)))
            if sure.size:
                rec["step"][g], rec["member"][g] = int(first_step) + int(sure[0]), best[g, sure[0]]
        out["decision"] = rec
    return out


def bound(exact, M, scale):
    """The ROUNDING paragraph of cmps_bank_posterior: |post - exact| <= 2^-24 |exact| + 2^-52 (M + 16 + 4 A') + 2^-149, A' = ``scale``."""
    return 2.0 ** -24 * np.abs(exact) + 2.0 ** -52 * (M + 16 + 4.0 * np.asarray(scale)) + 2.0 ** -149


def ill_posed(ref, thresholds):
    """(steps within MARGIN of a threshold, steps whose runner-up is neither MARGIN max(1, |a|) above the best nor tied with it exactly):
    two index arrays [count, 2] of (path, step).  Where both are empty the device must give the reference's best and decisions."""
    a = ref["a"]
    near = np.zeros(ref["conf64"].shape, bool)
    for t in thresholds:
        near |= (np.abs(ref["conf64"] - t) < MARGIN) & (ref["best"] >= 0)
    close = np.zeros_like(near)
    if a.shape[0] >= 2:
        two = np.sort(a, axis=0)[:2]
        with np.errstate(invalid="ignore"):
            gap = two[1] - two[0]
            close = (ref["best"] >= 0) & (two[1] < np.inf) & (gap != 0.0) & (gap < MARGIN * np.maximum(1.0, np.abs(two[0])))
    return np.argwhere(near), np.argwhere(close)


# ---------------------------------------------------------------------------------------------------
# the draws of the GPU tests
# ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (3, 2, 5), (2, 1, 63), (2, 1, 64), (2, 1, 65), (5, 3, 130), (65, 2, 40), (130, 1, 33), (1024, 1, 40)]
THRESHOLDS = (0.6, 0.99)


def draw(M, n, steps, seed):
    """nll uniform in +-[0, 3] plus a small offset per member: the totals drift apart slowly, so the posterior moves and crosses both
    thresholds somewhere.  Also running totals to resume from and a non-uniform prior."""
    rng = np.random.default_rng(seed)
    nll = (rng.uniform(-3.0, 3.0, (M, n, steps)) + rng.uniform(-0.5, 0.5, (M, 1, 1))).astype(np.float32)
    total = rng.uniform(-20.0, 20.0, (M, n)).astype(np.float32)
    prior = rng.uniform(0.2, 1.0, M)
    return nll, total, np.log(prior / prior.sum())


def cases():
    """[(id, kwargs of `posterior` without the decision's state)]: every shape under three settings, then the planted ones."""
    out = []
    for i, (M, n, steps) in enumerate(SHAPES):
        nll, total, lp = draw(M, n, steps, 100 + i)
        tag = f"{M}x{n}x{steps}"
        out.append((tag + "-uniform", dict(nll=nll, total_in=None, log_prior=None, inv_temp=1.0, threshold=0.6, first_step=0)))
        out.append((tag + "-prior", dict(nll=nll, total_in=total, log_prior=lp, inv_temp=0.5, threshold=0.99, first_step=1000)))
        never = lp.copy()
        never[M // 2] = -np.inf                                      # (M == 1: nobody can win)
        out.append((tag + "-never", dict(nll=nll, total_in=total, log_prior=never, inv_temp=4.0, threshold=0.6, first_step=2 ** 40)))
    # a NaN, a +Inf and a -Inf make exactly that member absent from there on, for that path only; +Inf then -Inf in one row: a NaN
    nll, total, lp = draw(5, 3, 130, 200)
    nll[1, 0, 7], nll[3, 1, 64], nll[4, 2, 129], nll[0, 2, 3], nll[0, 2, 70] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    out.append(("planted", dict(nll=nll, total_in=None, log_prior=lp, inv_temp=1.0, threshold=0.6, first_step=0)))
    # nobody present: path 0 from its first step (its total comes in as NaN), path 1 from step 2 on
    nll, total, lp = draw(3, 2, 5, 201)
    total[:, 0] = np.nan
    nll[:, 1, 2] = [np.nan, np.inf, -np.inf]
    out.append(("all-absent", dict(nll=nll, total_in=total, log_prior=None, inv_temp=1.0, threshold=0.6, first_step=0)))
    # two bit-identical rows, far below the others: the tie goes to the lower m, and nobody is ever sure
    for j, (M, n, steps) in enumerate([(3, 2, 5), (65, 2, 40), (130, 1, 33)]):
        nll, total, lp = draw(M, n, steps, 210 + j)
        lo, hi = (1, 2) if M == 3 else (7, M - 1)                    # (M - 1: another thread, another wavefront than row 7)
        nll[lo] -= np.float32(8.0)
        nll[hi] = nll[lo]
        out.append((f"tie-{M}", dict(nll=nll, total_in=None, log_prior=None, inv_temp=1.0, threshold=0.6, first_step=0)))
    return out


def cuts(steps):
    """Where the cut test cuts a run: after step 1, mid-chunk, and at the chunk edges that the run reaches."""
    return sorted({c for c in (1, 21, 32, 64, 75, 128) if c < steps})


# ---------------------------------------------------------------------------------------------------
# a stand-in for HipScan's bank_stream_posterior / rho_bank_stream_posterior
# ---------------------------------------------------------------------------------------------------
class PosteriorEntries:
    """Mixed into a stand-in backend that has `bank_stream_score`: the scored segment with nll kept, then this file's `posterior`."""

    def _posterior(self, score, state_in, state_out, k0, audio, n=None, loss=None, log_prior=None, inv_temp=1.0, threshold=None,
                   decision=None, want_post=False, want_nll=False, want_pred=False):
        nll, total, pred = score(state_in, state_out, k0, audio, want_nll=True, want_pred=True, n=n, loss=loss)
        ref = posterior(nll, total_in=loss, log_prior=log_prior, inv_temp=inv_temp, threshold=threshold, first_step=k0, decision=decision,
                        reset=decision is None)
        assert np.array_equal(ref["total_out"], total, equal_nan=True)
        self.posterior_calls = getattr(self, "posterior_calls", []) + [(k0, np.shape(nll), threshold, want_post, want_nll, want_pred)]
        return {"best": ref["best"], "conf": ref["conf"], "loss": ref["total_out"], "decision": ref.get("decision"), "carry": ref.get("decision"),
                "post": ref["post"] if want_post else None, "nll": nll if want_nll else None, "pred": (lambda: pred) if want_pred == "lazy" else pred if want_pred else None}

    def bank_stream_posterior(self, *args, **kw):
        return self._posterior(self.bank_stream_score, *args, **kw)
