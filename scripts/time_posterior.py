"""Time BankStream.score_posterior (cmps_bank_stream_score / cmps_rho_bank_stream_score, then cmps_bank_posterior on the device) against
what it replaces: `score` as it is -- which downloads nll and pred [M, n, steps] -- followed by the numpy restatement of the posterior on
the host (tests/_posterior_ref.py).

  python scripts/time_posterior.py [--out profiles/posterior_times.json]

Settings, n = 3 paths per model: PsiCMPS banks (D, M) = (8, 64) and (32, 16), a RhoCMPS bank D = 8, rank 8, M = 64; one shared
16000-sample clip in ten calls of 1600 steps.  And one evaluation shape: D = 8, M = 64, a batch of 64 clips of T = 2048 through
`classify` (+ the restatement on `nll_per_step`'s download) against `posterior_trace`.
A run opens its stream -- outside the clock for the stream settings, inside it for the evaluation shape, where opening is part of both
methods -- and makes the calls: the wall clock between two device synchronisations, so a figure holds everything a caller waits for.  Per
setting: 2 warm-up runs, then 5 timed ones, the three sides (bare score; score + host posterior; score_posterior) alternating inside one
process.  Reported: the median of the five, [min, max], and the two ratios.  THE GATE, judged against the bare `score` measured in the same
run and never against an expectation: score_posterior costs at most 1.05 x the bare score calls (the project's margin for a stage added
beside a scan).  The two methods' results are compared as the tests compare them: `best` and the decisions equal wherever the reference is
well-posed, `conf` within twice the header's bound.  k_bank_posterior's own time comes from kernel events, in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _posterior_ref as PR  # noqa: E402
from audio_mps_amd import HParams  # noqa: E402
from audio_mps_amd.bank import PsiBank, RhoBank  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402

#           kind     D  rank  M   n   steps  calls
SETTINGS = [("psi", 8, 0, 64, 3, 16000, 10), ("psi", 32, 0, 16, 3, 16000, 10), ("rho", 8, 8, 64, 3, 16000, 10), ("eval", 8, 0, 64, 64, 2047, 1)]
WARMUP, REPS = 2, 5
THRESHOLD, GATE = 0.99, 1.05


def make_bank(kind, D, rank, M, n):
    """M models of the stream tests' kind (sigma = 1, A = 10, Rx, Ry x 0.05)."""
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=1.0, A=10.0, initial_rank=rank or None)
    bank = (RhoBank if kind == "rho" else PsiBank)(hp, [{"seed": m} for m in range(M)], backend=HipScan(D))
    for model in bank.models:
        model.variables["Rx"] *= np.float32(0.05)
        model.variables["Ry"] *= np.float32(0.05)
    return bank, hp


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def agree(ref, best, conf, decided_at, decided_as, M):
    """The comparison of the tests: (best equal where well-posed, conf within twice the bound, decisions equal, ill-posed steps)."""
    near, close = PR.ill_posed(ref, (THRESHOLD,))
    ok = np.ones(ref["best"].shape, bool)
    ok[tuple(close.T)] = False
    within = bool(np.all(np.abs(conf.astype(np.float64) - ref["conf"].astype(np.float64)) <= 2.0 * PR.bound(ref["conf64"], M, ref["scale"])))
    same = bool(np.array_equal(decided_at, ref["decision"]["step"]) and np.array_equal(decided_as, ref["decision"]["member"]))
    return {"best_equal": bool(np.array_equal(best[ok], ref["best"][ok])), "conf_within_twice_the_bound": within,
            "decisions_equal": same, "ill_posed_steps": int(len(near) + len(close))}


def measure(kind, D, rank, M, n, steps, calls):
    bank, hp = make_bank(kind, D, rank, M, n)
    per = steps // calls
    clip = HipScan(D).damped_sine(1, 0, n if kind == "eval" else 1, steps + 1, hp.delta_t).cpu().numpy()
    blocks = [clip[:, c * per + (1 if c else 0):(c + 1) * per + 1] for c in range(calls)]

    def bare():
        if kind == "eval":
            return bank.classify(clip)
        st = bank.open_stream(n, steps)
        return timed(lambda: [st.score(b) for b in blocks])

    def host():
        if kind == "eval":
            return PR.posterior(bank.nll_per_step(clip), threshold=THRESHOLD)
        st = bank.open_stream(n, steps)
        return timed(lambda: PR.posterior(np.concatenate([st.score(b) for b in blocks], axis=-1), threshold=THRESHOLD))

    def device():
        if kind == "eval":
            return bank.posterior_trace(clip, threshold=THRESHOLD)
        st = bank.open_stream(n, steps, threshold=THRESHOLD)
        ms, traces = timed(lambda: [st.score_posterior(b) for b in blocks])
        return ms, (traces, st)

    sides = {"score": bare, "score_host_posterior": host, "score_posterior": device}
    ms = {k: [] for k in sides}
    last = {}
    for rep in range(WARMUP + REPS):
        for name, fn in sides.items():
            t, last[name] = timed(fn) if kind == "eval" else fn()
            if rep >= WARMUP:
                ms[name].append(t)
    ref = last["score_host_posterior"]
    if kind == "eval":
        tr = last["score_posterior"]
        check = agree(ref, tr.best, tr.conf, tr.decided_at, tr.decided_as, M)
    else:
        traces, st = last["score_posterior"]
        check = agree(ref, np.concatenate([t.best for t in traces], axis=1), np.concatenate([t.conf for t in traces], axis=1), st.decided_at,
                      st.decided_as, M)
        check["total_nll_bit_equal"] = bool(np.array_equal(st.total_nll.view(np.uint32), ref["total_out"].view(np.uint32)))
    # the kernel's own time, from kernel events, in a run of its own
    st = bank.open_stream(n, steps, threshold=THRESHOLD)
    st._be.kernel_events(True)
    for b in blocks:
        st.score_posterior(b)
    kt = st._be.kernel_times()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"kind": kind, "D": D, "rank": rank, "M": M, "n": n, "steps": steps, "calls": calls, "ms": ms,
           "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}, "max_ms": {k: max(v) for k, v in ms.items()},
           "ratio_posterior_over_score": med["score_posterior"] / med["score"],
           "ratio_host_over_posterior": med["score_host_posterior"] / med["score_posterior"],
           "kernel_ms": {k: {"sum_ms": v[0], "launches": v[1]} for k, v in kt.items()}, "results": check}
    row["gate_posterior_within_1.05_of_score"] = bool(row["ratio_posterior_over_score"] <= GATE)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "posterior_times.json"))
    args = ap.parse_args()
    rows = []
    for s in SETTINGS:
        rows.append(measure(*s))
        r = rows[-1]
        m, lo, hi = r["median_ms"], r["min_ms"], r["max_ms"]
        kp = r["kernel_ms"].get("k_bank_posterior", {"sum_ms": float("nan"), "launches": 0})
        print(f"{r['kind']} D={r['D']} M={r['M']} n={r['n']} {r['steps']} steps in {r['calls']} call(s): "
              + "  ".join(f"{k} {m[k]:.2f} ms [{lo[k]:.2f}, {hi[k]:.2f}]" for k in m)
              + f"  posterior/score {r['ratio_posterior_over_score']:.3f}  host/posterior {r['ratio_host_over_posterior']:.2f}"
              + f"  k_bank_posterior {kp['sum_ms']:.3f} ms in {kp['launches']} launch(es)  {r['results']}", flush=True)
        torch.cuda.empty_cache()
    cond = {"gate_every_setting": all(r["gate_posterior_within_1.05_of_score"] for r in rows),
            "results_agree": all(r["results"]["best_equal"] and r["results"]["conf_within_twice_the_bound"] and r["results"]["decisions_equal"]
                                 for r in rows)}
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "threshold": THRESHOLD, "gate": GATE, "settings": rows,
           "conditions": cond}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(cond))


if __name__ == "__main__":
    main()
