"""Random robustness sweep: random shapes, parameter scales, amplitudes and sampling rates through every kernel family against
the oracles.  Shared by `tests/test_gpu_sweep.py` (the loss and gradient families) and `tests/test_gpu_sweep_stream.py` (the sampler, stream
and score families) -- fixed seeds, asserted bars: what the driver runs -- and `scripts/random_sweep.py` (any seed, prints the worst case
per family).

Why it is a test: rounds 2-3 were green with a wrong `Qbar` in `k_bwd_wave` (a VALU write one wait state in front of
the MFMA that read it) because no fixed test made Q = -(dt sigma^2 / 2) R^dagger R (/root/reference/model.py:312)
visible in float32; this sweep drew sigma = 0.36 with a large R and found it -- but only ran by hand.

Every record is (family, quantity, error, bar, configuration).  Bars: the float32 families' parity bars of tests/test_gpu_parity.py
(loss 1e-5 of max(|loss_b|, 1), gradients 1e-4 of each tensor's max) against the float32 C restatement; the bf16 pair kernels' bars of
tests/test_gpu_pair.py against the bf16-emulating oracle; dA apart everywhere: it is ONE scalar made of two large cancelling sums, so
its bar is the float32 oracle's own distance to f64t32, float64 on the float32 time grid the kernels follow (never below the tensor
bar); where that bar is above the one anchored on the plain float64 twin, the old check is recorded next to it ("... f64-anchored").
A batch for which grad_sums took the fp16-range fallback (BF16X3 / VALU re-run) is a failed "fallback" check (bar 0): the sweep is
there to stress the fp16 scales, and the re-run would otherwise stand in for the kernel under test."""
from __future__ import annotations

import dataclasses

import numpy as np

from oracle import cmps_oracle as O, c_oracle as C
from _util import make_audio, c_oracle_run, grad_sums_and_fallbacks, rel_inf, oracle_hparams, oracle_variables
import _score_ref as SC
import _rho_score_ref as RS
from _score_ref import SCORE, FOLLOW, SAMPLE

LOSS_BAR, GRAD_BAR = 1e-5, 1e-4
PAIR_LOSS_BAR, PAIR_GRAD_BAR = 3e-4, 2e-3          # tests/test_gpu_pair.py, vs oracle.psi_bf16_scan
DEFAULT_COUNTS = {"psi": 60, "wide": 16, "step": 8, "pair": 14, "rho": 34, "legacy": 10, "psi_stream": 60, "rho_stream": 40}

# The stream families (psi_stream, rho_stream: the samplers, the resumable stream, its score mode, the saved RhoCMPS states) keep three
# things apart: draw_*(rng, it) -> case and check_*(case, result, ref32, ref64) -> records need numpy and the oracle only, so
# tests/test_sweep_stream_host.py can show on the CPU that the checks catch a wrong step; run_*_hip(case) -> result is the kernels.  Every
# check is against the float64 reference; its bar is the floor of the fixed tests plus their factor 4 on the float32 reference's own distance
# from float64.  Factor and floors are those of the headers of the fixed tests, quoted here once:
STREAM_FACTOR = 4.0                       # test_gpu_primed.py: "the kernels sum in another order than numpy (factor 4)"
PSI_OUT_FLOOR = 2e-5                      # test_gpu_primed.py OUT_RTOL, x max(1, max |out|)
PSI_PRED_FLOOR = 2e-6                     # test_gpu_primed.py, x max |pred|: "the accuracy tests' own"
NLL_FLOOR = 2.0 ** -22                    # test_gpu_stream_score.py: "two roundings of 1 + z at 1"
RHO_OUT_FLOOR = 2e-4                      # test_gpu_rho_primed.py OUT_RTOL, x max |out|
RHO_PRODUCT_FLOOR = 8.0 * 2.0 ** -22      # test_gpu_rho_primed.py: x |R|_F delta_t for pred; test_gpu_rho_stream_score.py: x |R|_F max|x| / A for nll
RHO_STATE_FLOOR = 2e-4                    # test_gpu_rho_stream.py: rel_inf(rho), x max |rho|
PURITY_RTOL, PURITY_ATOL = 2e-4, 1e-6     # test_gpu_rho_stream.py
AUTO, BLOCK, BF16X3 = 0, 1, 2             # CMPS_VARIANT_AUTO, CMPS_VARIANT_BLOCK; CMPS_OPT_RANK1 = BF16X3


def _loss_err(per, ref):
    return float(np.max(np.abs(per - ref) / np.maximum(np.abs(ref), 1)))


def _dA_bar(g32, gt, floor):
    """dA's bar: the float32 restatement's own distance from f64t32 on this draw (x 2), never below `floor`."""
    return max(floor, 2.0 * rel_inf(g32, gt))


def _elastic(out, fam, what, e_new, bar_new, e_old, bar_old, cfg):
    """The re-anchored check, and the f64-anchored one next to it where the new bar is the wider."""
    out.append((fam, what, e_new, bar_new, cfg))
    if bar_new > bar_old:
        out.append((fam, what + " f64-anchored", e_old, bar_old, cfg))


def sweep_psi(rng, n, out):
    """Pure-state wave (16- and 32-row) / block kernels vs the C restatement (model.py:257-334)."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan, unpack_grad
    for it in range(n):
        D = int(rng.integers(1, 33)); T = int(rng.integers(2, 700)); B = int(rng.integers(1, 14))
        sigma = float(10 ** rng.uniform(-4, 0)); rs = float(10 ** rng.uniform(-1.5, 0)); variant = int(rng.choice([1, 2]))
        hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma, A=float(10 ** rng.uniform(0, 2)))
        if it % 4 == 1:                                    # other sampling rates: 3 kHz ... 100 kHz (rotation table, dt_k, the scale of Q)
            hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma, A=hp.A, delta_t=float(10 ** rng.uniform(-5, -3.5)))
        amp = float(10 ** rng.uniform(-3, 0.3))           # amplitudes over three decades, silent stretches: the fp16 scales
        audio = (make_audio(B, T, hp.delta_t, it) * np.float32(amp)).astype(np.float32)
        if T > 40 and it % 3 == 0:
            audio[:, : T // 3] = 0.0
        m = PsiCMPS(hp, data_iterator=audio, seed=it, backend=HipScan(D, variant=variant, rank1=int(rng.choice([2, 3, 4]))))
        m.variables["Rx"] *= np.float32(rs); m.variables["Ry"] *= np.float32(rs)
        per = m.loss_per_clip(); (flat, _), nfb = grad_sums_and_fallbacks(m); g = unpack_grad(flat.cpu().numpy(), D)
        ref = c_oracle_run(m, audio, "f32"); gr = C.unpack_grad(ref["grad"], D)
        if not np.all(np.isfinite(ref["loss_per_clip"])):
            continue
        gt = C.unpack_grad(c_oracle_run(m, audio, "f64t32")["grad"], D)
        g64 = C.unpack_grad(c_oracle_run(m, audio, "f64")["grad"], D)
        cfg = (D, T, B, round(sigma, 5), round(rs, 3), variant, round(amp, 4), m._get_backend().effective_rank1, float(f"{hp.delta_t:.3g}"))
        assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat.cpu().numpy())), ("psi non-finite", cfg)
        out.append(("psi", "loss", _loss_err(per, ref["loss_per_clip"]), LOSS_BAR, cfg))
        out.append(("psi", "grad", max(rel_inf(g[k], gr[k]) for k in ("Rbar", "fbar", "psi0bar")), GRAD_BAR, cfg))
        out.append(("psi", "fallback", float(nfb), 0.0, cfg))
        eA = rel_inf(g["Abar"], gr["Abar"])
        _elastic(out, "psi", "dA", eA, _dA_bar(gr["Abar"], gt["Abar"], GRAD_BAR), eA, _dA_bar(gr["Abar"], g64["Abar"], GRAD_BAR), cfg)


def sweep_wide(rng, n, out):
    """Wide kernels (float32, 32 < D <= 128; AUTO), all three CMPS_OPT_WIDE_CHAIN values and every GEMM arithmetic."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan, unpack_grad
    from audio_mps_amd.data import synthetic_audio
    for it in range(n):
        D = int(rng.integers(33, 129)); T = int(rng.integers(2, 500)); B = int(rng.integers(1, 8))
        sigma = float(10 ** rng.uniform(-4, 0)); rs = float(10 ** rng.uniform(-1.5, -0.3))
        inp = str(rng.choice(["damped_sine", "damped_sine_noise", "bandlimited"]))
        hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma, A=float(10 ** rng.uniform(0.5, 2)))
        audio = synthetic_audio(inp, B, T, hp.delta_t, 400 + it)
        m = PsiCMPS(hp, data_iterator=audio, seed=it, backend=HipScan(D, rank1=int(rng.choice([1, 2, 3, 4]))))
        assert m._get_backend().variant == 5
        m._get_backend().set_wide_chain(int(rng.choice([0, 1, 1, 2])))
        m.variables["Rx"] *= np.float32(rs); m.variables["Ry"] *= np.float32(rs)
        per = m.loss_per_clip(); (flat, _), nfb = grad_sums_and_fallbacks(m); g = unpack_grad(flat.cpu().numpy(), D)
        ref = c_oracle_run(m, audio, "f32"); gr = C.unpack_grad(ref["grad"], D)
        gt = C.unpack_grad(c_oracle_run(m, audio, "f64t32")["grad"], D)
        g64 = C.unpack_grad(c_oracle_run(m, audio, "f64")["grad"], D)
        cfg = (D, T, B, round(sigma, 5), round(rs, 3), inp, m._get_backend().effective_rank1, m._get_backend().wide_chain)
        assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat.cpu().numpy())), ("wide non-finite", cfg)
        bf16x2 = m._get_backend().effective_rank1 == 1       # two bf16 pieces carry 16 operand bits (test_gpu_wide.py's bar for that mode)
        out.append(("wide", "loss", _loss_err(per, ref["loss_per_clip"]), LOSS_BAR, cfg))
        out.append(("wide", "grad", max(rel_inf(g[k], gr[k]) for k in ("Rbar", "fbar", "psi0bar")), GRAD_BAR * (2 if bf16x2 else 1), cfg))
        out.append(("wide", "fallback", float(nfb), 0.0, cfg))
        eA = rel_inf(g["Abar"], gr["Abar"])
        _elastic(out, "wide", "dA", eA, _dA_bar(gr["Abar"], gt["Abar"], GRAD_BAR), eA, _dA_bar(gr["Abar"], g64["Abar"], GRAD_BAR), cfg)


def sweep_step(rng, n, out):
    """Device-resident optimiser step (cmps_psi_apply_step) vs the host one, 10 steps (train.py:55-60, 88-89)."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    for it in range(n):
        D = int(rng.choice([3, 8, 16, 24, 32, 48])); T = int(rng.integers(20, 300)); B = int(rng.integers(1, 9))
        hp = HParams(minibatch_size=B, bond_dim=D, learning_rate=float(10 ** rng.uniform(-3, -1.7)))
        audio = make_audio(B, T, hp.delta_t, 500 + it)
        ms = [PsiCMPS(hp, data_iterator=audio, seed=it, backend=HipScan(D)) for _ in range(2)]
        if D > 32:
            for mm in ms:
                mm.variables["Rx"] *= np.float32(0.5); mm.variables["Ry"] *= np.float32(0.5)
        td, th = Trainer(ms[0], hp, device_step=True), Trainer(ms[1], hp)
        dev = np.array([td.step()["total_loss"] for _ in range(10)]); host = np.array([th.step()["total_loss"] for _ in range(10)])
        out.append(("step", "trajectory", float(np.max(np.abs(dev - host) / np.maximum(np.abs(host), 1))), 1e-6, (D, T, B, round(hp.learning_rate, 4))))


def sweep_pair(rng, n, out):
    """bf16 pair kernels vs the bf16-emulating oracle; odd draws make Q visible in float32 (sigma up to 0.5, large R)."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan, unpack_grad
    for it in range(n):
        D = int(rng.integers(33, 129)); T = int(rng.integers(2, 400)); B = int(rng.integers(1, 7))
        sigma = float(10 ** rng.uniform(-4, -0.3)) if it % 2 else 1e-4
        hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma)
        audio = make_audio(B, T, hp.delta_t, 100 + it)
        m = PsiCMPS(hp, data_iterator=audio, seed=it, backend=HipScan(D, variant=3))
        if it % 2:
            rs = float(10 ** rng.uniform(-1.0, -0.2))
            m.variables["Rx"] *= np.float32(rs); m.variables["Ry"] *= np.float32(rs)
        per = m.loss_per_clip(); (flat, _), nfb = grad_sums_and_fallbacks(m); g = unpack_grad(flat.cpu().numpy(), D)
        em = O.psi_bf16_scan(oracle_hparams(hp), oracle_variables(m), audio)
        cfg = (D, T, B, round(sigma, 5))
        out.append(("pair", "fallback", float(nfb), 0.0, cfg))
        if not np.all(np.isfinite(em["loss_per_clip"])):
            continue
        assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat.cpu().numpy())), ("pair non-finite", cfg)
        out.append(("pair", "loss", _loss_err(per, em["loss_per_clip"]), PAIR_LOSS_BAR, cfg))
        out.append(("pair", "grad", max(rel_inf(g[k], em[k]) for k in ("Rbar", "fbar", "psi0bar")), PAIR_GRAD_BAR, cfg))
        out.append(("pair", "dA", rel_inf(g["Abar"], em["Abar"]), 10 * PAIR_GRAD_BAR, cfg))


def sweep_rho(rng, n, out):
    """RhoCMPS (model.py:55-203): column kernels for rank <= 8, GEMM kernels above, general kernels for D > 32; vs the float64 matrix-form oracle."""
    from audio_mps_amd import HParams, RhoCMPS
    for it in range(n):
        D = int(rng.integers(2, 41)); r = int(rng.integers(1, min(D, 32) + 1)); T = int(rng.integers(2, 150)); B = int(rng.integers(1, 6))
        rs, amp = 0.4, 1.0
        kind = it % 12 if n < 34 else (3 if it in (3, 7, 11) else 11 if it >= 31 else 5 if it >= 14 else 0)
        if kind == 3:                                      # the general kernels' column groups: 32 < D <= 128, ragged ranks
            D = int(rng.integers(33, 129)); r = int(rng.integers(1, min(D, 40) + 1)); T = int(rng.integers(2, 40)); B = int(rng.integers(1, 4))
        if kind == 11:                                     # the reference's default rank = D above the old LDS limit (workspace columns)
            D = int(rng.integers(72, 129)); r = D; T = int(rng.integers(2, 12)); B = int(rng.integers(1, 3))
        elif kind >= 5:                                    # the GEMM kernels: rank > 8 at D <= 32, the fp16 x 2 forward's scales --
            D = int(rng.integers(9, 33)); r = int(rng.integers(9, D + 1)); T = int(rng.integers(2, 400))      # loud / quiet clips, large / tiny R
            rs = float(10 ** rng.uniform(-2.5, 0.2)); amp = float(10 ** rng.uniform(-3, 0.7))
        hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=r, sigma=float(10 ** rng.uniform(-4, -0.3)))
        audio = (make_audio(B, T, hp.delta_t, 200 + it) * np.float32(amp)).astype(np.float32)
        if kind >= 5 and it % 4 == 0 and T > 30:
            audio[:, T // 2:] = audio[:, T // 2: T // 2 + 1]                # a silent tail (increments exactly zero)
        m = RhoCMPS(hp, data_iterator=audio, seed=it)
        m.variables["Rx"] *= np.float32(rs); m.variables["Ry"] *= np.float32(rs)
        ov = O.Variables(np.asarray(m.variables["A"], np.float32), m.variables["Rx"], m.variables["Ry"], m.variables["freqs"],
                         np.zeros(D, np.float32), np.zeros(D, np.float32), scaled_R=True, scaled_freqs=True)
        ref, ref64 = (O.rho_loss_and_grads(O.HParams(**hp.values()), ov.astype(np.float64), m.variables["Wx"].astype(np.float64),
                                           m.variables["Wy"].astype(np.float64), audio, d) for d in ("f64t32", "f64"))
        if not np.all(np.isfinite(ref["per_clip"])):
            continue                                       # (1 + z <= 0 somewhere: the model itself diverges on this draw)
        per = m.loss_per_clip(); loss, grads = m.loss_and_grads()
        cfg = (D, r, T, B, round(rs, 4), round(amp, 4), round(hp.sigma, 5))
        assert np.all(np.isfinite(per)) and all(np.all(np.isfinite(grads[k])) for k in grads), ("rho non-finite", cfg)
        out.append(("rho", "loss", _loss_err(per, ref["per_clip"]), LOSS_BAR, cfg))
        ref32 = O.rho_loss_and_grads(O.HParams(**hp.values()), ov, m.variables["Wx"], m.variables["Wy"], audio, "f32")
        # per tensor against max(bar, 2 x the float32 oracle's own distance from f64t32): at tiny R / long clips the frequency gradient of
        # ANY float32 evaluation sat 1 - 2e-4 from float64 (seeds 31, 32: 1.1e-4 ... 2.0e-4 for the oracle and for every kernel setting
        # alike, scripts/dev_rho_sweep_cases.py) -- the float32 time grid against float64's; the record is the tensor closest to (or
        # furthest above) its bar, and the f64-anchored check of that tensor where its bar was the tighter
        checks = [(rel_inf(grads[k], ref[k]), max(GRAD_BAR, 2.0 * rel_inf(ref32[k], ref[k])),
                   rel_inf(grads[k], ref64[k]), max(GRAD_BAR, 2.0 * rel_inf(ref32[k], ref64[k]))) for k in ("Rx", "Ry", "freqs", "Wx", "Wy")]
        worst = max(checks, key=lambda c: c[0] / c[1])
        out.append(("rho", "grad", worst[0], worst[1], cfg))
        old = [c for c in checks if c[1] > c[3]]
        if old:
            worst = max(old, key=lambda c: c[2] / c[3])
            out.append(("rho", "grad f64-anchored", worst[2], worst[3], cfg))
        eA = rel_inf(grads["A"], ref["A"])
        _elastic(out, "rho", "dA", eA, _dA_bar(ref32["A"], ref["A"], GRAD_BAR),
                 rel_inf(grads["A"], ref64["A"]), _dA_bar(ref32["A"], ref64["A"], GRAD_BAR), cfg)


def sweep_legacy(rng, n, out):
    """Legacy AudioMPS arithmetic (training_estimators.py:43-45): wave kernels in legacy mode / general kernels above D = 32."""
    from audio_mps_amd import LegacyAudioMPS
    for it in range(n):
        D = int(rng.integers(2, 41)); T = int(rng.integers(2, 300)); B = int(rng.integers(1, 7)); dt = float(10 ** rng.uniform(-3, -2))
        audio = make_audio(B, T, dt, 300 + it, noise=0.05)
        m = LegacyAudioMPS(D, dt, B, data_iterator=audio, seed=it)
        ref = O.legacy_loss_and_grads(m.variables["H"], m.variables["R"], dt, audio, "f32")
        per = m.loss_per_clip(); loss, grads = m.loss_and_grads()
        out.append(("legacy", "loss", _loss_err(per, ref["per_clip"]), LOSS_BAR, (D, T, B)))
        out.append(("legacy", "grad", max(rel_inf(grads["R"], ref["gR"]), rel_inf(grads["H"], ref["gH"])), GRAD_BAR, (D, T, B)))


# ---------------------------------------------------------------------------------------------------
# the sampler, stream and score kernels: random plans of scored, followed and sampled segments
# ---------------------------------------------------------------------------------------------------
def _draw_plan(rng, cap=None):
    """1-5 segments of kind score, follow or sample; each step count from {1, 2, U[1, 40), U[60, 70), U[1, 140)} (single steps, both sides
    of the kernels' 64-step chunk), at most `cap`; a forced segment behind the first is anchored at random."""
    plan = []
    for s in range(int(rng.integers(1, 6))):
        kind = (SCORE, FOLLOW, SAMPLE)[int(rng.integers(3))]
        steps = (1, 2, int(rng.integers(1, 40)), int(rng.integers(60, 70)), int(rng.integers(1, 140)))[int(rng.integers(5))]
        anchored = bool(rng.integers(2)) and kind != SAMPLE and s > 0
        plan.append((kind, steps if cap is None else min(steps, cap), anchored))
    return plan


def _draw_inputs(rng, hp, plan, n, n_audio, amp, temp, silent):
    """(clip [n_audio, columns] = O.damped_sine x amp, its first third silent with `silent`, or None without forced steps;
    noise [sampled, n] = O.sample_noise at `temp`, or None without sampled steps)."""
    S, F, L, _ = SC.plan_counts(plan)
    clip = noise = None
    seed = int(rng.integers(2 ** 31))
    if S + F:
        cols = SC.clip_columns(plan)
        clip = (O.damped_sine(n_audio, cols, hp.delta_t, seed=seed) * np.float32(amp)).astype(np.float32)
        if silent and S + F > 40:
            clip[:, : cols // 3] = 0.0                       # increments exactly zero
    if L:
        noise = O.sample_noise(hp, n, L, temp=temp, seed=seed + 1)
    return clip, noise


def _plan_text(plan):
    return " ".join(f"{kind[:2]}{steps}{'a' if anchored else ''}" for kind, steps, anchored in plan)


def draw_psi_stream(rng, it):
    """Draw `it` of the psi_stream family (numpy only): the ranges of sweep_psi / sweep_wide, a plan, its clip and its noise."""
    D = int(rng.integers(33, 129)) if it % 3 == 2 else int(rng.integers(1, 33))
    variant = BLOCK if int(rng.integers(4)) == 0 else AUTO
    n = int(rng.integers(1, 7))
    n_audio = 1 if int(rng.integers(4)) == 0 else n         # one clip shared by every path
    sigma = float(10 ** rng.uniform(-4, 0))
    rs = float(10 ** (rng.uniform(-1.5, 0) if D <= 32 else rng.uniform(-1.5, -0.3)))
    A = float(10 ** rng.uniform(0, 2))
    amp = float(10 ** rng.uniform(-3, 0.3))
    delta_t = float(10 ** rng.uniform(-5, -3.5)) if it % 4 == 1 else 1.0 / 16000      # 3 kHz ... 100 kHz, as sweep_psi
    temp = float(rng.uniform(0.1, 1.5))
    plan = _draw_plan(rng)
    hp = O.HParams(minibatch_size=n, bond_dim=D, delta_t=delta_t, sigma=sigma, A=A)
    var = O.init_variables(hp, seed=int(rng.integers(2 ** 31)))
    var.Rx, var.Ry = var.Rx * np.float32(rs), var.Ry * np.float32(rs)
    clip, noise = _draw_inputs(rng, hp, plan, n, n_audio, amp, temp, silent=it % 3 == 0)
    cfg = (it, D, n, n_audio, variant, round(sigma, 5), round(rs, 3), round(A, 2), round(amp, 4), float(f"{delta_t:.3g}"), round(temp, 2),
           _plan_text(plan))
    return dict(family="psi_stream", hparams=hp, variables=var, plan=plan, clip=clip, noise=noise, n=n, n_audio=n_audio, variant=variant,
                options={}, cfg=cfg)


def draw_rho_stream(rng, it):
    """Draw `it` of the rho_stream family (numpy only): three draws of four in the row-array kernel's range with sweep_rho's scales of R and
    of the clip, the fourth in the general kernel's (32 < D <= 128, segments of at most 30 steps: the reference keeps n x steps x D^2
    states)."""
    big = it % 4 == 3
    if big:
        D = int(rng.integers(33, 129)); rank = int(rng.integers(1, min(D, 40) + 1)); rs = 0.4
    else:
        D = int(rng.integers(2, 33)); rank = int(rng.integers(1, D + 1)); rs = float(10 ** rng.uniform(-2.5, 0.2))
    rank1 = BF16X3 if not big and int(rng.integers(4)) == 0 else None
    variant = BLOCK if int(rng.integers(4)) == 0 else AUTO
    n = int(rng.integers(1, 5))
    n_audio = 1 if int(rng.integers(4)) == 0 else n
    sigma = float(10 ** rng.uniform(-4, -0.3))
    A = float(10 ** rng.uniform(0, 2))
    amp = float(10 ** rng.uniform(-3, 0.7))
    delta_t = float(10 ** rng.uniform(-5, -3.5)) if int(rng.integers(4)) == 0 else 1.0 / 16000      # (drawn: `it % 4` picks the kernel here)
    temp = float(rng.uniform(0.1, 1.5))
    plan = _draw_plan(rng, cap=30 if big else None)
    hp = O.HParams(minibatch_size=n, bond_dim=D, delta_t=delta_t, sigma=sigma, A=A, initial_rank=rank)
    seed = int(rng.integers(2 ** 31))
    var = O.init_variables(hp, seed=seed)
    var.Rx, var.Ry = var.Rx * np.float32(rs), var.Ry * np.float32(rs)
    var.psi_x, var.psi_y = np.zeros(D, np.float32), np.zeros(D, np.float32)          # (RhoCMPS has none)
    Wx, Wy = O.rho_init_W(hp, seed=seed)
    clip, noise = _draw_inputs(rng, hp, plan, n, n_audio, amp, temp, silent=False)
    cfg = (it, D, rank, n, n_audio, variant, rank1, round(sigma, 5), round(rs, 4), round(A, 2), round(amp, 4), float(f"{delta_t:.3g}"),
           round(temp, 2), _plan_text(plan))
    return dict(family="rho_stream", hparams=hp, variables=var, Wx=Wx, Wy=Wy, plan=plan, clip=clip, noise=noise, n=n, n_audio=n_audio,
                variant=variant, options={"rank1": rank1}, cfg=cfg)


def reference_psi_stream(case, dtype):
    """SC.score_reference on the draw's own hparams and variables: dict(nll, total, pred, out)."""
    with np.errstate(all="ignore"):
        nll, total, pred, out, _ = SC.score_reference(case["hparams"], case["variables"], case["plan"], case["clip"], case["noise"], dtype,
                                                      n=case["n"])
    return dict(nll=nll, total=total, pred=pred, out=out)


def reference_rho_stream(case, dtype):
    """RS.rho_score_reference on the draw's own hparams and variables: dict(nll, total, pred, out, rho, purity)."""
    with np.errstate(all="ignore"):
        nll, total, pred, out, rho, purity, _ = RS.rho_score_reference(case["hparams"], case["variables"], case["Wx"], case["Wy"],
                                                                       case["plan"], case["clip"], case["noise"], dtype, n=case["n"])
    return dict(nll=nll, total=total, pred=pred, out=out, rho=rho, purity=purity)


def all_finite(res):
    return all(np.all(np.isfinite(v)) for v in res.values() if isinstance(v, np.ndarray))


def _amax(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def _dist(a, b):
    """max |a - b| in double precision (NaN if either holds one)."""
    wide = np.complex128 if np.iscomplexobj(b) else np.float64
    return _amax(np.asarray(a, dtype=wide) - np.asarray(b, dtype=wide))


def _is_primed_plan(plan):
    """One followed segment, then one sampled one: what cmps_{psi,rho}_sample_primed runs in one call."""
    return [seg[0] for seg in plan] == [FOLLOW, SAMPLE]


def _forced_increments(case):
    """The clip increments the plan's forced steps read [n_audio, scored + followed]."""
    cols, c = [], 0
    for kind, skip in SC.expand(case["plan"]):
        if kind != SAMPLE:
            c += skip
            cols.append(c)
            c += 1
    clip = np.asarray(case["clip"], dtype=np.float64)
    return clip[:, [c + 1 for c in cols]] - clip[:, cols]


def _stream_records(case, res, r32, r64, floors):
    """The records every stream family shares: each quantity's distance from the float64 reference against STREAM_FACTOR x the float32
    reference's own distance plus the family's floor `floors[quantity]`; the totals relative to max(|l|, 1); finiteness."""
    fam, cfg = case["family"], case["cfg"]
    S = SC.plan_counts(case["plan"])[0]
    rec = [(fam, "finite", float(sum(int(np.sum(~np.isfinite(v))) for v in res.values() if isinstance(v, np.ndarray))), 0.0, cfg)]
    for what in ("out", "pred", "nll"):
        if r64[what].size:
            assert res[what].shape == r64[what].shape, (fam, what, res[what].shape, r64[what].shape, cfg)
            rec.append((fam, what, _dist(res[what], r64[what]), STREAM_FACTOR * _dist(r32[what], r64[what]) + floors[what], cfg))
    if S:
        scale = np.maximum(np.abs(r64["total"]), 1.0)
        own = _amax((r32["total"].astype(np.float64) - r64["total"]) / scale)
        rec.append((fam, "total", _amax((res["total"].astype(np.float64) - r64["total"]) / scale), max(LOSS_BAR, STREAM_FACTOR * own), cfg))
    return rec


def check_psi_stream(case, res, r32, r64):
    """Records of one psi_stream draw: `res` (dict(nll, total, pred, out) and, from the kernels, "primed") against the references."""
    floors = {"out": PSI_OUT_FLOOR * max(1.0, _amax(r64["out"])), "pred": PSI_PRED_FLOOR * _amax(r64["pred"]), "nll": NLL_FLOOR}
    rec = _stream_records(case, res, r32, r64, floors)
    if res.get("primed") is not None:                    # tests/test_gpu_stream.py::test_one_call_equals_the_existing_entries, of the pair
        out_p, pred_p = res["primed"]
        rec.append(("psi_stream", "primed out", _dist(out_p, res["out"]), PSI_OUT_FLOOR * max(1.0, _amax(r32["out"])), case["cfg"]))
        rec.append(("psi_stream", "primed pred", _dist(pred_p, res["pred"]),
                    STREAM_FACTOR * _dist(r32["pred"], r64["pred"]) + PSI_PRED_FLOOR * _amax(r64["pred"]), case["cfg"]))
    return rec


def check_rho_stream(case, res, r32, r64):
    """Records of one rho_stream draw: `res` (dict(nll, total, pred, out, rho, purity) and, from the kernels, "primed")."""
    hp, cfg = case["hparams"], case["cfg"]
    R_fro = float(np.linalg.norm(O.effective_params(hp, case["variables"].astype(np.float64), "f64")[0]))
    product = RHO_PRODUCT_FLOOR * R_fro                  # the split arithmetics' product error on e at unit trace
    x_max = _amax(_forced_increments(case)) if r64["pred"].size else 0.0
    floors = {"out": RHO_OUT_FLOOR * _amax(r64["out"]), "pred": product * hp.delta_t,
              "nll": NLL_FLOOR + product * x_max / float(case["variables"].A)}
    rec = _stream_records(case, res, r32, r64, floors)
    rec.append(("rho_stream", "rho", _dist(res["rho"], r64["rho"]),
                STREAM_FACTOR * _dist(r32["rho"], r64["rho"]) + RHO_STATE_FLOOR * _amax(r64["rho"]), cfg))
    allowed = STREAM_FACTOR * _dist(r32["purity"], r64["purity"]) + PURITY_ATOL + PURITY_RTOL * np.abs(r64["purity"])
    rec.append(("rho_stream", "purity", _amax((res["purity"].astype(np.float64) - r64["purity"]) / allowed), 1.0, cfg))      # (in units of its bar)
    if res.get("primed") is not None:                    # tests/test_gpu_rho_stream.py::test_one_call_against_the_existing_entries
        out_p, pred_p = res["primed"]
        rec.append(("rho_stream", "primed out", _dist(out_p, res["out"]), RHO_OUT_FLOOR * _amax(r32["out"]), cfg))
        rec.append(("rho_stream", "primed pred", _dist(pred_p, res["pred"]),
                    STREAM_FACTOR * _dist(r32["pred"], r64["pred"]) + product * hp.delta_t, cfg))
    return rec


def _segments(plan):
    """(kind, steps, first clip column or None, first noise row or None, k0) of every segment: the clip cursor of tests/_score_ref.py -- an
    anchored segment starts one column further on, without a step."""
    c = l0 = k0 = 0
    for seg in plan:
        kind, steps, anchored = SC._seg(seg)
        if kind == SAMPLE:
            yield kind, steps, None, l0, k0
            l0 += steps
        else:
            c += anchored
            yield kind, steps, c, None, k0
            c += steps
        k0 += steps


def _gather(parts, n):
    return np.concatenate([np.empty((n, 0), np.float32)] + parts, axis=1)


def _running_loss(plan, n):
    """The running loss handed to the first scored segment: not read at k0 = 0 (the NaN pattern proves it), zero behind unscored steps."""
    return np.full(n, np.nan if plan[0][0] == SCORE else 0.0, np.float32)


def run_psi_stream_hip(case):
    """The plan call by call through HipScan: stream_score for a scored segment, stream with audio for a followed one, stream with noise
    for a sampled one; the state alternates between two records.  A [follow, sample] plan also goes through sample_primed ("primed")."""
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    hp, var, plan, clip, noise, n = (case[k] for k in ("hparams", "variables", "plan", "clip", "noise", "n"))
    m = PsiCMPS(HParams(**dataclasses.asdict(hp)), seed=0, backend=HipScan(hp.bond_dim, variant=case["variant"]))
    for k in O.Variables.NAMES:
        m.variables[k] = np.array(getattr(var, k), dtype=np.float32)
    be = m._get_backend()
    be.set_params(m.effective_params(), n, sum(SC.plan_counts(plan)[:3]) + 1, train=False)
    states = [be.stream_state(n), be.stream_state(n)]
    cur, loss = None, _running_loss(plan, n)
    nll, pred, out = [], [], []
    for idx, (kind, steps, c, l0, k0) in enumerate(_segments(plan)):
        nxt = states[idx % 2]
        if kind == SCORE:
            a, loss, p = be.stream_score(cur, nxt, k0, clip[:, c:c + steps + 1], want_nll=True, want_pred=True, n=n, loss=loss)
            nll.append(a)
            pred.append(p)
        elif kind == FOLLOW:
            pred.append(be.stream(cur, nxt, k0, clip[:, c:c + steps + 1], None, True, n=n)[1])
        else:
            out.append(be.stream(cur, nxt, k0, None, noise[l0:l0 + steps], False, n=n)[0])
        cur = nxt
    res = dict(nll=_gather(nll, n), total=loss, pred=_gather(pred, n), out=_gather(out, n))
    if _is_primed_plan(plan):
        res["primed"] = be.sample_primed(clip, noise, want_pred=True)
    return res


def run_rho_stream_hip(case):
    """run_psi_stream_hip for RhoCMPS: rho_stream_score / rho_stream with save_states, and rho_states behind every call."""
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.scan import HipScan
    hp, var, plan, clip, noise, n = (case[k] for k in ("hparams", "variables", "plan", "clip", "noise", "n"))
    D = hp.bond_dim
    m = RhoCMPS(HParams(**dataclasses.asdict(hp)), seed=0, backend=HipScan(D, variant=case["variant"], rank1=case["options"]["rank1"]))
    for k, v in (("A", var.A), ("Rx", var.Rx), ("Ry", var.Ry), ("freqs", var.freqs), ("Wx", case["Wx"]), ("Wy", case["Wy"])):
        m.variables[k] = np.array(v, dtype=np.float32)
    be = m._get_backend()
    total = sum(SC.plan_counts(plan)[:3])
    be.set_params(m.effective_params(), n, total + 1, train=False)
    be.rho_set_state(m.columns(), n, max(seg[1] for seg in plan) + 1, train=True)       # (stash rows for the longest call only)
    states = [be.rho_stream_state(n), be.rho_stream_state(n)]
    cur, loss = None, _running_loss(plan, n)
    nll, pred, out, rho, pur = [], [], [], [], []
    for idx, (kind, steps, c, l0, k0) in enumerate(_segments(plan)):
        nxt = states[idx % 2]
        if kind == SCORE:
            a, loss, p = be.rho_stream_score(cur, nxt, k0, clip[:, c:c + steps + 1], want_nll=True, want_pred=True, n=n, loss=loss,
                                             save_states=True)
            nll.append(a)
            pred.append(p)
        elif kind == FOLLOW:
            pred.append(be.rho_stream(cur, nxt, k0, clip[:, c:c + steps + 1], None, True, n=n, save_states=True)[1])
        else:
            out.append(be.rho_stream(cur, nxt, k0, None, noise[l0:l0 + steps], False, n=n, save_states=True)[0])
        r, p = be.rho_states(n, steps, want_rho=True, want_purity=True)
        rho.append(r)
        pur.append(p)
        cur = nxt
    res = dict(nll=_gather(nll, n), total=loss, pred=_gather(pred, n), out=_gather(out, n), rho=np.concatenate(rho, axis=1),
               purity=np.concatenate(pur, axis=1))
    if _is_primed_plan(plan):
        be.rho_set_state(m.columns(), n, total + 1, train=False)
        res["primed"] = be.rho_sample_primed(clip, noise, want_pred=True)
    return res


def _sweep_stream(draw, reference, run, check, rng, n, out):
    for it in range(n):
        case = draw(rng, it)
        r32, r64 = reference(case, "f32"), reference(case, "f64")
        if not (all_finite(r32) and all_finite(r64)):
            continue                                       # (1 + z <= 0 somewhere: the model itself diverges on this draw, as in sweep_psi)
        out += check(case, run(case), r32, r64)


def sweep_psi_stream(rng, n, out):
    """k_sample_wave / k_sample_wide / k_sample_block in their stream, score and primed modes vs the plan composition (tests/_score_ref.py)."""
    _sweep_stream(draw_psi_stream, reference_psi_stream, run_psi_stream_hip, check_psi_stream, rng, n, out)


def sweep_rho_stream(rng, n, out):
    """k_sample_rho_mfma / k_sample_rho in the same modes, k_states_rho behind them, vs tests/_rho_score_ref.py."""
    _sweep_stream(draw_rho_stream, reference_rho_stream, run_rho_stream_hip, check_rho_stream, rng, n, out)


FAMILIES = {"psi": sweep_psi, "wide": sweep_wide, "step": sweep_step, "pair": sweep_pair, "rho": sweep_rho, "legacy": sweep_legacy,
            "psi_stream": sweep_psi_stream, "rho_stream": sweep_rho_stream}


def run_sweep(seed, counts=None, families=None):
    """All families with one generator (the order is fixed, so a seed names its draws).  Returns the list of records."""
    rng = np.random.default_rng(seed)
    counts = dict(DEFAULT_COUNTS, **(counts or {}))
    out = []
    for fam, fn in FAMILIES.items():
        if families is None or fam in families:
            fn(rng, counts[fam], out)
    return out


def _ratio(err, bar):
    return err / bar if bar > 0 else (np.inf if err > 0 else 0.0)


def worst_by_kind(records):
    worst = {}
    for fam, what, err, bar, cfg in records:
        key = f"{fam} {what}"
        if key not in worst or _ratio(err, bar) > _ratio(*worst[key][:2]):
            worst[key] = (err, bar, cfg)
    return worst
