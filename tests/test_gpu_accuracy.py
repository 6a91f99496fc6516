"""Accuracy of the HIP path at the benchmark's full sizes, against f64t32: the float64 evaluation of the problem the kernels solve
(float64 arithmetic on the reference's float32 time grid, t += dt in float32, model.py:16, :281; oracle/cmps_oracle.c).

Per case, for every per-clip loss and every effective gradient tensor (R, freqs, psi_0, A):
    |hip - f64t32| <= max(fixed bar, 1.5 |oracle_f32 - f64t32|)
where the fixed bars are the parity bars of tests/test_gpu_parity.py (loss 1e-5 of max(|loss_b|, 1), gradients 1e-4 of the tensor's
max) and |oracle_f32 - f64t32| is the float32 C restatement's own rounding on the same draw.  Against plain float64 the float32
oracle's distance is mostly the time-grid mismatch, which grows with T (fbar at T = 2^16 in the case below: 0.8 of its max from f64,
8.7e-4 from f64t32) and would excuse anything; against f64t32 it is rounding alone, so the kernels may do at most 1.5 x as badly as
the float32 restatement does.  Both distances are printed.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import c_oracle as C
from _util import c_oracle_run, make_audio, rel_inf, strict_grad_sums

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-4


def _loss_err(per, ref):
    return float(np.max(np.abs(per - ref) / np.maximum(np.abs(ref), 1.0)))


@pytest.mark.parametrize("D,T,B,amp,silent,rscale", [
    (16, 4096, 256, None, False, None),       # BASELINE configs[1] in full
    (32, 16000, 32, None, False, None),       # configs[2] at full T
    (32, 65536, 6, None, False, None),        # the reference's default --sample_duration = 2^16 (train.py:27)
    (128, 16000, 4, None, False, 0.35),       # configs[4] at full T, in float32 (the wide kernels, AUTO above D = 32)
    (32, 16000, 8, 1e-3, True, None),         # quiet clips with a silent first third: the fp16 scales at their smallest
], ids=["c2", "c3", "t65536", "c5_f32", "quiet"])
def test_full_length_accuracy_against_f64t32(D, T, B, amp, silent, rscale):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan, unpack_grad
    hp = HParams(minibatch_size=B, bond_dim=D)
    audio = make_audio(B, T, hp.delta_t, seed=D + B)
    if amp is not None:
        audio = (audio * np.float32(amp)).astype(np.float32)
    if silent:
        audio[:, : T // 3] = 0.0
    m = PsiCMPS(hp, data_iterator=audio, seed=D + B, backend=HipScan(D))
    if rscale is not None:                   # as the benchmark and tests/test_gpu_wide.py do at D > 64 (1 + e x / A stays positive)
        m.variables["Rx"] *= np.float32(rscale)
        m.variables["Ry"] *= np.float32(rscale)
    per = m.loss_per_clip()
    flat = strict_grad_sums(m)[0].cpu().numpy()
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat))
    with ThreadPoolExecutor(2) as pool:       # the two oracle runs side by side (ctypes releases the GIL), 8 threads each
        r32, rt = pool.map(lambda d: c_oracle_run(m, audio, d, nthreads=8), ("f32", "f64t32"))
    assert np.all(np.isfinite(r32["loss_per_clip"])) and np.all(np.isfinite(rt["loss_per_clip"]))
    print(f"D {D} T {T} B {B} variant {m._get_backend().variant}")
    e, own = _loss_err(per, rt["loss_per_clip"]), _loss_err(r32["loss_per_clip"], rt["loss_per_clip"])
    bar = max(LOSS_RTOL, 1.5 * own)
    print(f"  loss     |hip - f64t32| {e:.2e}   |f32 - f64t32| {own:.2e}   bar {bar:.2e}")
    bad = [] if e <= bar else [("loss", e, bar)]
    g, g32, gt = unpack_grad(flat, D), C.unpack_grad(r32["grad"], D), C.unpack_grad(rt["grad"], D)
    for k in ("Rbar", "fbar", "psi0bar", "Abar"):
        e, own = rel_inf(g[k], gt[k]), rel_inf(g32[k], gt[k])
        bar = max(GRAD_RTOL, 1.5 * own)
        print(f"  {k:8s} |hip - f64t32| {e:.2e}   |f32 - f64t32| {own:.2e}   bar {bar:.2e}")
        if not e <= bar:
            bad.append((k, e, bar))
    assert not bad, bad
