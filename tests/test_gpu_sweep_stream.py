"""The random sweep of the sampler, stream and score kernels under `-m gpu`: fixed seeds, the psi_stream and rho_stream families of
tests/_sweep.py, asserted bars.  The fixed tests of these kernels (test_gpu_primed, test_gpu_stream, test_gpu_stream_score and their
RhoCMPS counterparts) compare them with the oracle at one operating point per model -- sigma = 1, A = 10, R x 0.05 and sigma = 0.1, A = 5,
R x 0.3, both at delta_t = 1/16000 and unit amplitude -- where a delta_t taken from the wrong place, an A applied twice and cancelled or a
normalisation that only works near |psi| = 1 passes.  The draws move sigma over four decades, R over 1.5 (2.7 for RhoCMPS), A over two,
the clip's amplitude over three, the sampling rate over 3-100 kHz, through random plans of scored, followed and sampled segments with
anchors, in k_sample_wave / _wide / _block, k_sample_rho_mfma (both arithmetics) / k_sample_rho and k_states_rho.
tests/test_sweep_stream_host.py shows on the CPU, for these seeds and counts, that the bars catch eight kinds of wrong step.

Measured on an MI355X, seeds 41-48 (96 + 64 draws, RhoCMPS seed 47 draw 6 skipped: amplitude 4.4 at A = 1.07 takes 1 + z
below zero in the reference; 0.2 ... 1.9 s per seed): the worst
error / bar per family and quantity -- records, not bars:
  quantity   psi_stream   rho_stream
  out        0.15         0.16
  pred       0.31         0.28
  nll        0.26         0.19
  total      0.26         0.06
  rho        -            0.04
  purity     -            0.03
  finite     every value  every value
By hand, scripts/random_sweep.py seeds 1-6 with the full counts (360 + 240 draws, 2854 records): one record over its bar, psi_stream pred
5.80e-12 against 5.09e-12 at seed 6 draw 8 (D = 48, the wide kernel, plan "score 1, sample 2").  That pred is one number, the expectation
on psi_0 at t = 0 times delta_t (no clip or noise enters it), 1.87e-06 out of terms of size |R|_F delta_t = 9.3e-04; the float32
reference landed 3.4e-13 from float64, and of 200 float32 evaluations of the reference's own formula with the basis permuted (another
summation order, nothing else) 9 % are further from float64 than the bar, 8.5e-12 at the most.  The kernel's error is 0.1 ulp of the terms
it sums: rounding, not a wrong step; bar and draws stay as they are.  Seeds 7-40 the same way (16010 records): none over its bar, the
worst at 0.61 of it (psi_stream pred, again a plan with a single forced step).
The [follow, sample] plans among the draws (psi_stream 2, rho_stream 1) gave the bits of cmps_{psi,rho}_sample_primed in out and pred.
"""
import time

import pytest

from _sweep import run_sweep, worst_by_kind

pytestmark = pytest.mark.gpu

SEEDS = (41, 42, 43, 44, 45, 46, 47, 48)
COUNTS = {"psi_stream": 12, "rho_stream": 8}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sweep_stream(seed):
    t0 = time.perf_counter()
    records = run_sweep(seed, COUNTS, families=tuple(COUNTS))
    worst = worst_by_kind(records)
    print(f"seed {seed}: {len(records)} checks in {time.perf_counter() - t0:.1f} s")
    for key, (err, bar, cfg) in worst.items():
        print(f"  {key:24s} worst {err:.2e} (bar {bar:.1e}, ratio {err / bar if bar > 0 else float(err > 0):.2f}) at {cfg}")
    bad = [(fam, what, err, bar, cfg) for fam, what, err, bar, cfg in records if not err <= bar]
    assert not bad, bad
    assert {r[0] for r in records} == set(COUNTS)          # both families produced checks
