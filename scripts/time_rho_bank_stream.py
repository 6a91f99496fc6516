"""Time a RhoCMPS bank's stream (cmps_rho_bank_stream, cmps_rho_bank_stream_score) against a Python loop over M plain RhoCMPS streams of
its members (cmps_rho_stream, cmps_rho_stream_score).

  python scripts/time_rho_bank_stream.py [--out profiles/rho_bank_stream_times.json]

Settings, n = 3 paths per model (the reference's num_samples, train.py:82-85), rank = D:
  generate   D = 8, M in {1, 8, 64}, and D = 32, M = 16: 16000 steps in ten `generate` calls of 1600 with device-drawn noise;
  score      D = 8, M = 64: one shared 16000-sample clip followed and scored by every model, in ten `score` calls.
A run opens the stream(s) -- outside the clock -- and makes the ten calls: the wall clock between two device synchronisations, so a figure
holds everything a caller waits for (the noise fill, the sampler kernel, the download of the results).  Per setting and method: 2 warm-up
runs, then 5 timed ones; the bank and the loop alternate inside one process, on one stream.  Reported: the median of the five, their min
and max, the ratio loop / bank, and -- judged against the loop measured here and never against an expectation -- whether the bank at M = 1
lies inside [min, max] of the five loop measurements (and by how much it misses them if not), and whether the bank at M = 64 is faster
than the loop.  The two methods' results are compared bit for bit once per setting.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_mps_amd import HParams  # noqa: E402
from audio_mps_amd.bank import RhoBank  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402

#           kind        D   M
SETTINGS = [("generate", 8, 1), ("generate", 8, 8), ("generate", 8, 64), ("generate", 32, 16), ("score", 8, 64)]
N, STEPS, CALLS = 3, 16000, 10
WARMUP, REPS = 2, 5


def make_bank(D, M):
    """M models of the RhoCMPS sampler tests' kind (sigma = 0.1, A = 5, Rx, Ry x 0.3, rank = D), every one with a backend of its own for
    the loop; the bank's stream opens its own too."""
    hp = HParams(minibatch_size=N, bond_dim=D, sigma=0.1, initial_rank=D, A=5.0)
    bank = RhoBank(hp, [{"seed": m} for m in range(M)], backend=HipScan(D))
    for model in bank.models:
        model.variables["Rx"] *= np.float32(0.3)
        model.variables["Ry"] *= np.float32(0.3)
        model._backend = HipScan(D)
    return bank, hp


def measure(kind, D, M):
    bank, hp = make_bank(D, M)
    per = STEPS // CALLS
    clip = HipScan(D).damped_sine(1, 0, 1, STEPS + 1, hp.delta_t).cpu().numpy() if kind == "score" else None

    def calls(streams):
        """The ten calls on every stream of `streams`; the last call's results."""
        res = None
        for c in range(CALLS):
            if kind == "generate":
                res = [st.generate(per) for st in streams]
            else:
                res = [st.score(clip[:, c * per + (1 if c else 0):(c + 1) * per + 1]) for st in streams]
        return res

    def run(banked, seed):
        kw = dict(temp=0.5, seed=seed, device_noise=True) if kind == "generate" else {}
        streams = [bank.open_stream(N, STEPS, **kw)] if banked else [m.open_stream(N, STEPS, **kw) for m in bank.models]
        assert not banked or streams[0].native
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = calls(streams)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, (res[0] if banked else np.stack(res)), streams

    t_loop, t_bank, same = [], [], True
    for rep in range(WARMUP + REPS):
        a, ra, sa = run(False, rep)
        b, rb, sb = run(True, rep)
        if rep >= WARMUP:
            t_loop.append(a)
            t_bank.append(b)
        same = same and ra.tobytes() == rb.tobytes() and bool(np.all(np.isfinite(rb)))    # the two methods ran the same steps
        if kind == "score":
            same = same and np.stack([s.total_nll for s in sa]).tobytes() == sb[0].total_nll.tobytes()
    med_l, med_b = statistics.median(t_loop), statistics.median(t_bank)
    return {"kind": kind, "D": D, "rank": D, "M": M, "n": N, "steps": STEPS, "calls": CALLS, "loop_ms": t_loop, "bank_ms": t_bank,
            "loop_median_ms": med_l, "bank_median_ms": med_b, "loop_min_ms": min(t_loop), "loop_max_ms": max(t_loop),
            "bank_min_ms": min(t_bank), "bank_max_ms": max(t_bank), "ratio_loop_over_bank": med_l / med_b, "results_bit_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rho_bank_stream_times.json"))
    args = ap.parse_args()
    rows = []
    for kind, D, M in SETTINGS:
        rows.append(measure(kind, D, M))
        r = rows[-1]
        print(f"{kind} D=rank={D} M={M} n={N} {STEPS} steps in {CALLS} calls: loop {r['loop_median_ms']:.2f} ms [{r['loop_min_ms']:.2f}, "
              f"{r['loop_max_ms']:.2f}]  bank {r['bank_median_ms']:.2f} ms [{r['bank_min_ms']:.2f}, {r['bank_max_ms']:.2f}]  loop/bank "
              f"{r['ratio_loop_over_bank']:.2f}  bit-equal {r['results_bit_equal']}", flush=True)
        torch.cuda.empty_cache()
    one = rows[0]
    inside = one["loop_min_ms"] <= one["bank_median_ms"] <= one["loop_max_ms"]
    miss = 0.0 if inside else (one["bank_median_ms"] - one["loop_max_ms"] if one["bank_median_ms"] > one["loop_max_ms"]
                               else one["bank_median_ms"] - one["loop_min_ms"])
    cond = {"bank_M1_within_loop_spread": inside, "bank_M1_outside_by_ms": miss,
            "bank_M64_faster_than_loop": all(r["bank_median_ms"] < r["loop_median_ms"] for r in rows if r["M"] == 64),
            "all_results_bit_equal": all(r["results_bit_equal"] for r in rows)}
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "settings": rows, "conditions": cond}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(cond))


if __name__ == "__main__":
    main()
