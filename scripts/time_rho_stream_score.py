#!/usr/bin/env python3
"""What scoring a followed signal costs for RhoCMPS: cmps_rho_stream_score against a plain follow (cmps_rho_stream, forced steps only) of
the same steps, and against cmps_rho_loss_fwd on the same clips, in one process.

usage: python scripts/time_rho_stream_score.py [--out profiles/rho_stream_score_times.json] [--reps 5] [--warmup 2]

Shapes: D = rank = 32, 256 paths, 1000 steps (the row-array GEMM kernel k_sample_rho_mfma, the default fp16 x 2 arithmetic); D = 64,
rank 16, 64 paths, 200 steps (the block kernel k_sample_rho).  One sine clip per path; the audio block, nll, loss and the state records
are resident in device memory, pred is not asked for and no columns are saved.  A job is one call over all steps; its time is the wall
clock between two device synchronisations (the launch and the host's wait are part of it, so it is an upper bound of the kernel time --
at these sizes by a few tens of microseconds).  Every job is run --warmup times untimed and then --reps times; the median, every value
and the spread (max - min) / median go to the JSON file, with the ratios scored / followed and scored / forward.  The scored total is
compared with cmps_rho_loss_fwd's loss (max relative difference, recorded).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 32, 256, 1000), (64, 16, 64, 200)]       # (D, rank, paths, steps)


def _model(D, rank, n, backend):
    import numpy as np
    from audio_mps_amd import HParams, RhoCMPS
    hp = HParams(minibatch_size=n, bond_dim=D, sigma=0.1, initial_rank=rank, A=5.0)
    m = RhoCMPS(hp, seed=17, backend=backend)
    m.variables["Rx"] *= np.float32(0.3)
    m.variables["Ry"] *= np.float32(0.3)
    return m


def time_shape(D, rank, n, steps, reps, warmup):
    import numpy as np
    import torch
    from audio_mps_amd.scan import HipScan
    be = HipScan(D)
    m = _model(D, rank, n, be)
    be.set_params(m.effective_params(), n, steps + 1, train=False)
    be.rho_set_state(m.columns(), n, steps + 1, train=False)
    lib, h, dev = be._lib, be._h, be.device
    t = np.arange(steps + 1, dtype=np.float64) / 16000.0
    clip = (0.5 * np.sin(2 * np.pi * 261.6 * t[None, :] + np.arange(n)[:, None])).astype(np.float32)
    audio = torch.from_numpy(clip).to(dev)
    stream = be._stream()
    state = be.rho_stream_state(n)
    nll = torch.empty((n, steps), dtype=torch.float32, device=dev)
    loss = torch.zeros(n, dtype=torch.float32, device=dev)
    fwd_loss = torch.zeros(n, dtype=torch.float32, device=dev)

    def job_score():
        code = lib.cmps_rho_stream_score(h, None, state.data_ptr(), 0, audio.data_ptr(), n, steps, n, nll.data_ptr(), loss.data_ptr(), None, 0, stream)
        assert code == 0, lib.cmps_last_error(h)

    def job_follow():
        code = lib.cmps_rho_stream(h, None, state.data_ptr(), 0, audio.data_ptr(), n, steps, None, 0, n, None, None, 0, stream)
        assert code == 0, lib.cmps_last_error(h)

    def job_fwd():
        code = lib.cmps_rho_loss_fwd(h, audio.data_ptr(), n, steps + 1, fwd_loss.data_ptr(), 0, stream)
        assert code == 0, lib.cmps_last_error(h)

    def timed(job):
        for _ in range(warmup):
            job()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            job()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        med = statistics.median(ms)
        return {"median_ms": med, "all_ms": ms, "spread": (max(ms) - min(ms)) / med, "us_per_step": 1e3 * med / steps}

    be.kernel_events(True)
    job_score()
    job_follow()
    job_fwd()
    kernels = list(be.kernel_times())
    be.kernel_events(False)
    res = {"kernels": kernels, "cmps_rho_loss_fwd": timed(job_fwd), "follow": timed(job_follow), "score": timed(job_score)}
    res["score_over_follow"] = res["score"]["median_ms"] / res["follow"]["median_ms"]
    res["score_over_loss_fwd"] = res["score"]["median_ms"] / res["cmps_rho_loss_fwd"]["median_ms"]
    lo, fw = loss.cpu().numpy().astype(np.float64), fwd_loss.cpu().numpy().astype(np.float64)
    res["score_total_vs_fwd_max_rel"] = float(np.max(np.abs(lo - fw) / np.maximum(np.abs(fw), 1.0)))
    res["finite"] = bool(np.all(np.isfinite(lo)))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rho_stream_score_times.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    shapes = {}
    for D, rank, n, steps in SHAPES:
        shapes[f"D{D}_rank{rank}_n{n}_steps{steps}"] = dict(D=D, rank=rank, n=n, steps=steps, **time_shape(D, rank, n, steps, a.reps, a.warmup))
    doc = {"what": "wall clock between two device synchronisations of one followed / scored / forward job of forced steps (one call, inputs "
                   "resident in device memory), milliseconds; median of --reps runs after --warmup untimed ones",
           "device": "MI355X (gfx950); torch.cuda.get_device_name: " + torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for key, row in shapes.items():
        print(key, {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in row.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
