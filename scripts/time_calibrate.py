#!/usr/bin/env python3
"""Time the calibration of a class bank: cmps_bank_calibrate against a host fit of the downloaded losses, and BankTrainer.calibrate's pass
against evaluate_classifier's.

  python scripts/time_calibrate.py [--out profiles/calibrate_times.json] [--parts fit,pass] [--shapes 64x4096,1024x4096]
                                   [--warmup 2] [--reps 5] [--device_only 1024x4096]

Per timed figure: --warmup warm-ups, then --reps measurements, each the wall clock between two device synchronisations; the two sides of
a comparison alternate inside one run, on one stream.  Reported: the median with [min, max].  The defaults are the protocol; a run with
others says so in its output ("warmup", "reps").
  fit   (a) cmps_bank_calibrate (HipScan.bank_calibrate and the one download of theta and the record), fit = both, on the draw of
        tests/_calib_ref.py at each (M, N) of --shapes, against what a user had before it: download the [M][N] losses and fit them with
        the numpy reference (tests/_calib_ref.py::optimise in float64: bisection on g for kappa, scaling sweeps for c, until |kappa g| and
        the prior residual are below the same tolerance).  Both sides must reach the same theta: each side's theta is evaluated by the
        reference in long double and ASSERTED stationary within the tests' tolerances (tol + the header's rounding bounds), and the two
        cross-entropies asserted equal within 2 eps_J + tol.  Reported too: the passes the device used and the time per pass.
        A shape named in --device_only is timed on the device alone (its row says "host": null): at (1024, 4096) ONE host fit of this
        draw takes more than ten minutes, seven of them more than a session.
  pass  (b) D = 8, M = 64, batches of 8 clips of T = 16000: BankTrainer.calibrate per batch against evaluate_classifier per batch over the
        same held-out set.  The one-off fit (bank_calibrate on the kept losses, with its download) is timed on its own and taken out of
        calibrate's total before the division by the number of batches.  The gate is the project's own for such additions: per batch,
        calibrate <= 1.05 x evaluate_classifier; a miss is reported as a miss.
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

import _calib_ref as R  # noqa: E402
from audio_mps_amd import HParams  # noqa: E402
from audio_mps_amd.bank import BankTrainer, PsiBank  # noqa: E402
from audio_mps_amd.device_data import ResidentDataset  # noqa: E402
from audio_mps_amd.scan import HipScan  # noqa: E402

TOL, MAX_ITER = 1e-9, 2000
D, B, T, M = 8, 8, 16000, 64
N_BATCHES = 16


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(a, b, warmup, reps):
    ta, tb = [], []
    for rep in range(warmup + reps):
        x, y = timed(a), timed(b)
        if rep >= warmup:
            ta.append(x)
            tb.append(y)
    return ta, tb


def summary(ts):
    return {"ms": ts, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def stationary(l, labels, kappa, c, who):
    """The tests' tolerances at a theta, in long double: |kappa g| <= tol + kappa eps_g and the prior residual <= tol + eps_q / n."""
    ev = R.evaluate(l, labels, kappa, c, np.longdouble)
    eJ, eg, eq = ev.bounds()
    kg, resid = abs(float(kappa * ev.g)), ev.resid()
    assert 1e-6 < kappa < 1e6 and kg <= TOL + kappa * eg and resid <= TOL + eq / ev.n, (who, kappa, kg, resid)
    return {"kappa": float(kappa), "abs_kappa_g": kg, "resid_prior": resid, "xent": float(ev.J), "eps_J": eJ}


def fit_against_the_host(be, M_, N_, warmup, reps, with_host=True):
    padded, labels, N_ = R.draw(M_, N_, seed=100 + M_)
    l = np.ascontiguousarray(padded[:, :N_])
    k0, c0 = R.start(l, labels, 3)
    loss, lab = torch.from_numpy(l).to(be.device), torch.from_numpy(labels).to(be.device)
    got = {}

    def device():
        got["device"] = be.read_calibrate_record(be.bank_calibrate(loss, lab, 3, k0, c0, TOL, MAX_ITER))

    def host():
        down = loss.cpu().numpy()
        got["host"] = R.optimise(down, labels, 3, k0, c0, dtype=np.float64, resid_tol=TOL, kappa_tol=TOL / 10, rounds=MAX_ITER)

    if not with_host:                                  # --device_only: the device side alone, where a host fit takes too long to repeat
        t_dev = [timed(device) for _ in range(warmup + reps)][warmup:]
        theta, rec = got["device"]
        row = {"M": M_, "N": N_, "fit": "both", "tol": TOL, "max_iter": MAX_ITER, "launch_pairs_enqueued": MAX_ITER + 1,
               "device": summary(t_dev), "host": None, "passes": rec["passes"], "flags": rec["flags"],
               "device_ms_per_pass": statistics.median(t_dev) / rec["passes"], "xent_start": rec["xent_start"], "xent_end": rec["xent_end"]}
        if rec["flags"] == R.CONVERGED:
            row["device_theta"] = stationary(l, labels, float(theta[0]), theta[1:], "device")
        print(f"fit M={M_} N={N_}: device {row['device']['median_ms']:.3f} ms [{min(t_dev):.3f}, {max(t_dev):.3f}] in {rec['passes']} passes "
              f"({row['device_ms_per_pass']:.4f} ms per pass), flags {rec['flags']}; host not run", flush=True)
        return row
    t_dev, t_host = alternate(device, host, warmup, reps)
    theta, rec = got["device"]
    kr, cr, rounds = got["host"]
    assert rec["flags"] == R.CONVERGED, rec
    dev = stationary(l, labels, float(theta[0]), theta[1:], "device")
    hst = stationary(l, labels, float(kr), np.asarray(cr, dtype=np.float64), "host")
    assert abs(dev["xent"] - hst["xent"]) <= 2 * dev["eps_J"] + TOL, (dev, hst)
    row = {"M": M_, "N": N_, "fit": "both", "tol": TOL, "max_iter": MAX_ITER, "launch_pairs_enqueued": MAX_ITER + 1,
           "device": summary(t_dev), "host": summary(t_host), "host_over_device": statistics.median(t_host) / statistics.median(t_dev),
           "passes": rec["passes"], "device_ms_per_pass": statistics.median(t_dev) / rec["passes"], "host_rounds": rounds,
           "xent_start": rec["xent_start"], "xent_end": rec["xent_end"], "device_theta": dev, "host_theta": hst,
           "kappa_difference": abs(dev["kappa"] - hst["kappa"]), "same_theta_within_the_tests_tolerances": True}
    print(f"fit M={M_} N={N_}: device {row['device']['median_ms']:.3f} ms [{min(t_dev):.3f}, {max(t_dev):.3f}] in {rec['passes']} passes "
          f"({row['device_ms_per_pass']:.4f} ms per pass); host {row['host']['median_ms']:.1f} ms [{min(t_host):.1f}, {max(t_host):.1f}] in "
          f"{rounds} rounds; kappa {dev['kappa']:.9g} / {hst['kappa']:.9g}", flush=True)
    return row


def pass_against_evaluate_classifier(warmup, reps):
    hp = HParams(minibatch_size=B, bond_dim=D)
    be = HipScan(D)
    classes = list(range(M))
    bank = BankTrainer(PsiBank(hp, [{"seed": m} for m in range(M)], backend=be, classes=classes, label_key="pitch"))
    n = B * N_BATCHES
    held = ResidentDataset(be.damped_sine(2, 0, n, T, hp.delta_t), be, labels=np.arange(n) % M)
    t_cal, t_cls = alternate(lambda: bank.calibrate(held, B, fit="both"), lambda: bank.evaluate_classifier(held, B), warmup, reps)
    loss, labels, _, _ = bank._heldout_losses(held, B, None, "time_calibrate")
    t_fit = [timed(lambda: be.read_calibrate_record(be.bank_calibrate(loss, labels, 3, 1.0, None))) for _ in range(warmup + reps)][warmup:]
    fit = statistics.median(t_fit)
    per_cal, per_cls = [(t - fit) / N_BATCHES for t in t_cal], [t / N_BATCHES for t in t_cls]
    ratio = statistics.median(per_cal) / statistics.median(per_cls)
    res = bank.calibrate(held, B, fit="both")
    out = {"D": D, "M": M, "batch": B, "batches": N_BATCHES, "T": T, "calibrate_total": summary(t_cal), "evaluate_classifier_total": summary(t_cls),
           "one_off_fit": summary(t_fit), "calibrate_per_batch_without_the_fit": summary(per_cal), "evaluate_classifier_per_batch": summary(per_cls),
           "ratio_per_batch": ratio, "within_1.05": ratio <= 1.05, "fit_passes": res.passes, "fit_converged": res.converged}
    print(f"pass per batch: calibrate {statistics.median(per_cal):.3f} ms [{min(per_cal):.3f}, {max(per_cal):.3f}]  evaluate_classifier "
          f"{statistics.median(per_cls):.3f} ms [{min(per_cls):.3f}, {max(per_cls):.3f}]  ratio {ratio:.4f} "
          f"({'within' if ratio <= 1.05 else 'MISSES'} 1.05); the one-off fit {fit:.3f} ms ({res.passes} passes)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_times.json"))
    ap.add_argument("--parts", default="fit,pass")
    ap.add_argument("--shapes", default="64x4096,1024x4096")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device_only", default="", help="shapes of --shapes whose host fit is not run (MxN,...): the device side alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps}
    if os.path.exists(args.out):                       # a run of some parts or shapes keeps what an earlier one of the same protocol wrote
        with open(args.out) as f:
            old = json.load(f)
        if (old.get("warmup"), old.get("reps")) == (args.warmup, args.reps):
            out = {**old, **out}
    parts = args.parts.split(",")
    if "fit" in parts:
        be = HipScan(8)
        rows = {f"{r['M']}x{r['N']}": r for r in out.get("fit", [])}
        for shape in args.shapes.split(","):
            m, n = (int(v) for v in shape.split("x"))
            rows[shape] = fit_against_the_host(be, m, n, args.warmup, args.reps, shape not in args.device_only.split(","))
        out["fit"] = list(rows.values())
    if "pass" in parts:
        out["pass"] = pass_against_evaluate_classifier(args.warmup, args.reps)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
