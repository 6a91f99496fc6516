"""Every gradient kernel family against float64 AUTOGRAD of the restated forward (tests/_autograd_ref.py, "f64t32": float64 arithmetic
on the float32 time grid the kernels follow), through that module's check functions.  The other gradient tests compare with oracle/,
whose reverse sweeps were derived by hand from the derivation the kernels implement; the twin shares no derivation with either
(tests/test_autograd_host.py holds oracle/ itself to it at 1e-10, and shows that these checks reject a wrong kernel).

Per case: the per-clip loss of the forward-only scan, the loss sum and every gradient tensor of the training forward + reverse scan
(PsiCMPS: the effective-parameter sums of cmps_psi_loss_bwd; RhoCMPS: A, Rx, Ry, freqs, Wx, Wy, the twin's effective cotangents mapped to the
raw variables by automatic differentiation of tests/_step_ref.py::effective; legacy: H, R) at the bars of tests/test_gpu_accuracy.py:
    loss max(1e-5, 1.5 |oracle_f32 - twin|) of max(|loss_b|, 1);  tensors max(1e-4, 1.5 |oracle_f32 - twin|) of the tensor's max;
    A as tests/_sweep.py prices it; the two-piece bf16 rank-1 sums (CMPS_RANK1_BF16X2) with the project's existing extra 3e-5.
An fp16-range fallback fails the case (tests/_util.py's strict accessors), the named kernels must have run (kernel events), and both
distances, |hip - twin| and |oracle_f32 - twin|, are printed for every quantity.  Shapes are the smallest that cross each kernel's
boundaries: one step past a 32- / 64-step chunk, a lone top octet, padded D, ragged batches.

The bf16 pair kernels (CMPS_VARIANT_PAIR) are left out: their arithmetic is bf16 by design and tests/test_gpu_pair.py holds them to a
bf16-emulating oracle; a float64 reference adds nothing there.

Largest |hip - twin| / |oracle_f32 - twin| per family, one MI355X box's figures (loss; the worst gradient tensor and which):
    family        loss                  worst gradient tensor
    wave16        2.4e-07 / 4.2e-07     fbar    8.7e-07 / 3.3e-07   (D 16, T 66, B 5)
    two-wave      5.5e-07 / 3.1e-07     Abar    1.9e-06 / 5.1e-07   (D 17, T 66, B 5)
    one-wave      3.4e-07 / 3.4e-07     Rbar    7.6e-06 / 3.0e-07   (BF16X2; the other three arithmetics 1.1e-06 at most)
    block         3.5e-07 / 3.5e-07     Rbar    7.5e-07 / 2.9e-07   (D 7, T 40, B 3)
    wide          4.4e-07 / 8.7e-08     Rbar    1.1e-06 / 3.4e-07   (D 128, VALU chain, fp16 x 2 GEMM)
    floor         2.0e-07 / 2.0e-08     psi0bar 7.1e-05 / 5.4e-07   (WAVE; BLOCK 6.4e-05)
    rho columns   2.1e-07 / 2.1e-07     A       8.6e-06 / 2.3e-06   (D 5, rank 2)
    rho virtual   8.4e-07 / 7.7e-07     Ry      1.4e-06 / 2.4e-06   (D 20, rank 9)
    rho gemm      8.4e-07 / 7.7e-07     Ry      1.3e-06 / 2.4e-06   (D 20, rank 9)
    rho wide      2.7e-07 / 2.0e-07     freqs   6.4e-07 / 7.2e-07   (D 40, rank 6)
    rho block     1.5e-07 / 3.3e-08     Rx      3.2e-07 / 3.8e-07   (D 12, rank 40)
    legacy        1.9e-07 / 4.9e-08     gH      6.7e-07 / 2.0e-07   (D 64, T 66, B 2)
"""
import functools

import numpy as np
import pytest

import _autograd_ref as AR

pytestmark = pytest.mark.gpu

AUTO, BLOCK, WAVE = 0, 1, 2                            # CMPS_VARIANT_*
BF16X2, BF16X3, DEFAULT = 1, 2, 4                      # CMPS_RANK1_*
BF16X2_EXTRA = 3e-5                                    # tests/test_gpu_parity.py: "BF16X2 carries 16 operand bits"


def _events(be, fn):
    """(fn(), names of the kernels it launched)."""
    be.kernel_events(True)
    try:
        out = fn()
        names = set(be.kernel_times())
    finally:
        be.kernel_events(False)
    return out, names


def _assert(family, label, records, own):
    AR.report(f"[{family}] {label}", records, own)
    bad = AR.failures(records)
    assert not bad, (label, bad)


# ---------------------------------------------------------------------------------------------------
# PsiCMPS
# ---------------------------------------------------------------------------------------------------
SIGMA_VISIBLE = dict(sigma=0.36, A=66.0, rscale=0.69, amp=0.09, seed=7, audio_seed=3)       # test_qbar_sums_visible_at_large_sigma


def _psi_model(D, T, B, backend=None, sigma=1e-4, A=100.0, rscale=None, amp=None, seed=None, audio_seed=None):
    from audio_mps_amd import HParams, PsiCMPS
    from _util import make_audio
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma, A=A)
    audio = make_audio(B, T, hp.delta_t, D + T if audio_seed is None else audio_seed)
    if amp is not None:
        audio = (audio * np.float32(amp)).astype(np.float32)
    m = PsiCMPS(hp, data_iterator=audio, seed=D + T if seed is None else seed, backend=backend)
    if rscale is not None:
        m.variables["Rx"] *= np.float32(rscale)
        m.variables["Ry"] *= np.float32(rscale)
    return m, audio


def _floor_model(backend=None):
    """tests/test_gpu_parity.py::test_normalisation_floor_branch: (I + s R) u = 0 at step 0 of clip 1."""
    from audio_mps_amd import HParams, PsiCMPS
    from _util import make_audio
    a, A, T = 2.0, 4.0, 40
    hp = HParams(minibatch_size=3, bond_dim=2, sigma=0.0, A=A)
    audio = make_audio(3, T, hp.delta_t, 77, noise=0.05)
    audio[1, 0] = 0.0
    audio[1, 1] = -A / a
    m = PsiCMPS(hp, R_in=np.array([[0, a], [a, 0]], dtype=np.complex64), freqs_in=np.array([3.0, -5.0], dtype=np.float32),
                psi_in=np.array([1, 1], dtype=np.complex64), data_iterator=audio, backend=backend)
    return m, audio


def _psi_refs_of(m, audio):
    """(twin, float32 oracle) of a model on the parameters the kernels receive: the float32 effective R, freqs, psi_0, A."""
    from oracle import c_oracle as C
    from _util import c_oracle_run
    p = m.effective_params()
    aux = {}
    twin = AR.psi_twin(audio, p.R, p.freqs, p.psi0, p.A, p.delta_t, p.sigma, "f64t32", aux=aux)
    twin["norm"] = aux["norm"]
    r = c_oracle_run(m, audio, "f32")
    ref32 = dict(C.unpack_grad(r["grad"], m.bond_d), per_clip=r["loss_per_clip"])
    assert np.all(np.isfinite(twin["per_clip"])) and np.all(np.isfinite(ref32["per_clip"]))
    return twin, ref32


@functools.lru_cache(maxsize=None)
def _psi_refs(D, T, B, cfg):
    """The references of a shape, computed once and shared by the kernel settings that run it."""
    return _psi_refs_of(*_psi_model(D, T, B, **dict(cfg)))


@functools.lru_cache(maxsize=None)
def _floor_refs():
    return _psi_refs_of(*_floor_model())


def _psi_result(m, audio):
    """dict(per_clip, loss_sum, Rbar, fbar, psi0bar, Abar) of the HIP path and the names of the kernels of the training pass."""
    from audio_mps_amd.scan import unpack_grad
    from _util import strict_grad_sums
    be = m._get_backend()
    per = m.loss_per_clip()
    (flat, _), names = _events(be, lambda: strict_grad_sums(m))
    flat = flat.cpu().numpy()
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(flat))
    return dict(unpack_grad(flat, m.bond_d), per_clip=per), names


def _check_psi(family, label, m, audio, refs, kernels, extra=0.0):
    twin, ref32 = refs
    res, names = _psi_result(m, audio)
    assert set(kernels) <= names, (label, kernels, names)
    own = AR.own_distances(twin, ref32, AR.PSI_KEYS)
    records = AR.check_psi(res, twin, ref32, extra)
    B = len(twin["per_clip"])                          # the training forward's own loss, as tests/test_gpu_parity.py asks it of the sum
    records.append(("loss_sum", abs(float(res["loss_sum"]) - twin["loss_sum"]) / max(abs(twin["loss_sum"]), B), records[0][2]))
    own["loss_sum"] = abs(float(ref32["loss_sum"]) - twin["loss_sum"]) / max(abs(twin["loss_sum"]), B)
    _assert(family, label, records, own)
    return records


def _hipscan(D, **kw):
    from audio_mps_amd.scan import HipScan
    return HipScan(D, **kw)


@pytest.mark.parametrize("D,T,B", [(3, 34, 3), (16, 66, 5)])
def test_psi_wave16(D, T, B):
    """The 16-row layout (cmps_wave16.hip): a partly and a fully used row set; one step past its 32-step forward chunk / the 64-step
    scalar chunk, a lone top octet."""
    m, audio = _psi_model(D, T, B, backend=_hipscan(D, variant=WAVE))
    _check_psi("wave16", f"D {D} T {T} B {B}", m, audio, _psi_refs(D, T, B, ()), {"k_fwd_wave16", "k_bwd_wave16"})


@pytest.mark.parametrize("D,T,B,cfg", [(17, 66, 5, ()), (32, 131, 3, ()), (32, 60, 5, tuple(SIGMA_VISIBLE.items()))],
                         ids=["17-66-5", "32-131-3", "32-60-5-sigma"])
def test_psi_two_wave_default(D, T, B, cfg):
    """What a new handle runs at 16 < D <= 32: k_fwd_wave2 (normalised stash rows) + the chain / gradient wave pair k_bwd_wave2w; ragged
    batches, (N - 1) & 7 = 0 and 2, and Q = -(dt sigma^2 / 2) R^dagger R visible in float32."""
    from audio_mps_amd import _capi
    m, audio = _psi_model(D, T, B, backend=_hipscan(D), **dict(cfg))
    be = m._get_backend()
    assert be._lib.cmps_get_option(be._h, _capi.CMPS_OPT_BWD_WAVES) == 2 and be.rank1 == DEFAULT
    _check_psi("two-wave", f"D {D} T {T} B {B}", m, audio, _psi_refs(D, T, B, cfg), {"k_fwd_wave2", "k_bwd_wave2w"})


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_psi_one_wave_every_rank1_arithmetic(mode):
    """CMPS_OPT_BWD_WAVES = 1: k_bwd_wave with exact fp32 MFMAs, two / three bf16 pieces, two fp16 pieces."""
    from audio_mps_amd import _capi
    D, T, B = 24, 66, 3
    m, audio = _psi_model(D, T, B, backend=_hipscan(D, rank1=mode))
    be = m._get_backend()
    _capi.check(be._h, be._lib.cmps_set_option(be._h, _capi.CMPS_OPT_BWD_WAVES, 1))
    assert be.rank1 == mode
    _check_psi("one-wave", f"rank1 {mode}", m, audio, _psi_refs(D, T, B, ()), {"k_fwd_wave2", "k_bwd_wave"},
               extra=BF16X2_EXTRA if mode == BF16X2 else 0.0)


@pytest.mark.parametrize("D,T,B", [(7, 40, 3), (33, 20, 2)])
def test_psi_block(D, T, B):
    """CMPS_VARIANT_BLOCK: the general one-workgroup-per-clip kernels, below and above the wave kernels' D."""
    m, audio = _psi_model(D, T, B, backend=_hipscan(D, variant=BLOCK))
    _check_psi("block", f"D {D} T {T} B {B}", m, audio, _psi_refs(D, T, B, ()), {"k_fwd_block", "k_bwd_block"})


@pytest.mark.parametrize("rank1", [DEFAULT, BF16X3])
@pytest.mark.parametrize("chain", [0, 1, 2])
@pytest.mark.parametrize("D,T,B,rscale", [(40, 67, 3, None), (128, 34, 2, 0.35)])
def test_psi_wide(D, T, B, rscale, chain, rank1):
    """AUTO above D = 32 (cmps_wide.hip): every CMPS_OPT_WIDE_CHAIN value (fp32 VALU chain; fp16 x 2 on the matrix cores both ways; forward
    only) x the gradient GEMM with two fp16 / three bf16 pieces; padded D (40 -> 64) and the largest D, an odd batch (a half-filled pair),
    one step past the 64-step chunk and the 4-step GEMM units."""
    from audio_mps_amd import _capi
    m, audio = _psi_model(D, T, B, backend=_hipscan(D, rank1=rank1), rscale=rscale)
    be = m._get_backend()
    assert be.variant == _capi.CMPS_VARIANT_WIDE
    be.set_wide_chain(chain)
    fwd = "k_fwd_wide" if chain == _capi.CMPS_WIDE_CHAIN_VALU else "k_fwd_chain16"
    bwd = "k_bwd_chain16" if chain == _capi.CMPS_WIDE_CHAIN_MFMA else "k_bwd_wide"
    gemm = "k_grad_gemm<f16x2>" if rank1 == DEFAULT else "k_grad_gemm<3>"
    _check_psi("wide", f"D {D} chain {chain} rank1 {rank1}", m, audio, _psi_refs(D, T, B, (("rscale", rscale),)),
               {fwd, bwd, gemm})


@pytest.mark.parametrize("variant", [WAVE, BLOCK])
def test_psi_floor(variant):
    """The annihilated-state clip: |y|^2 = 0 <= 1e-12 at step 0 of clip 1, the floored branch of the normalisation and of its adjoint
    (the twin: torch.maximum, whose gradient goes to the constant there).  tests/test_gpu_parity.py holds this clip's gradients to 1e-3
    of the float32 oracle; the kernels meet this module's elastic bars here (psi0bar 7.1e-5 and Rbar 1.5e-5 of a 1e-4 bar, the rest below
    4e-7), so those are asserted.  That the kernels sit 100 x further out than the float32 oracle here (5e-7) is the two ORDINARY clips, not the
    annihilated one, whose gradient is exactly zero on every side: freqs = (3, -5) rad/s turn 2e-4 rad per step, where the modulus rounding
    of the float32 rotation table (up to 3e-8 per step, put right at the end of each 64-step chunk, cmps_prep.hip) is largest next to the
    rotation itself; it mixes the two components by 1.5e-8 per step against the true 2.5e-4, the ratio seen in psi0bar."""
    m, audio = _floor_model(backend=_hipscan(2, variant=variant))
    twin, ref32 = _floor_refs()
    assert np.all(twin["norm"][1] == 0.0) and np.all(np.delete(twin["norm"], 1, axis=0) > AR.FLOOR)
    kernels = {"k_fwd_wave16", "k_bwd_wave16"} if variant == WAVE else {"k_fwd_block", "k_bwd_block"}
    _check_psi("floor", f"variant {variant}", m, audio, (twin, ref32), kernels)


# ---------------------------------------------------------------------------------------------------
# RhoCMPS
# ---------------------------------------------------------------------------------------------------
def _rho_model(D, rank, T, B, backend=None, sigma=1e-4, rscale=None):
    from audio_mps_amd import HParams, RhoCMPS
    from _util import make_audio
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=sigma, initial_rank=rank)
    audio = make_audio(B, T, hp.delta_t, D + T)
    m = RhoCMPS(hp, data_iterator=audio, seed=D + T, backend=backend)
    if rscale is not None:
        m.variables["Rx"] *= np.float32(rscale)
        m.variables["Ry"] *= np.float32(rscale)
    return m, audio


@functools.lru_cache(maxsize=None)
def _rho_refs(D, rank, T, B, sigma, rscale):
    from oracle import cmps_oracle as O
    m, audio = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    v = m.variables
    twin = AR.rho_twin(audio, m.R, m.freqs, v["Wx"], v["Wy"], float(m.A), float(m.delta_t), float(m.sigma), "f64t32")
    raw = AR.raw_gradients({k: v[k] for k in ("Rx", "Ry", "freqs", "A")}, twin, float(m._c_r), float(m._c_h))
    twin.update(raw)                                   # A, Rx, Ry, freqs next to the twin's own Wx, Wy
    ov = O.Variables(np.asarray(v["A"], dtype=np.float32), v["Rx"].copy(), v["Ry"].copy(), v["freqs"].copy(), np.zeros(D, np.float32),
                     np.zeros(D, np.float32), scaled_R=True, scaled_freqs=True)
    ref32 = O.rho_loss_and_grads(O.HParams(**m.hparams.values()), ov, v["Wx"], v["Wy"], audio, "f32")
    assert np.all(np.isfinite(twin["per_clip"])) and np.all(np.isfinite(ref32["per_clip"]))
    return twin, ref32


def _check_rho(family, label, m, refs, kernels, absent=()):
    from _util import strict_loss_and_grads
    twin, ref32 = refs
    be = m._get_backend()
    per = m.loss_per_clip()
    (loss, grads), names = _events(be, lambda: strict_loss_and_grads(m))
    assert set(kernels) <= names and not set(absent) & names, (label, kernels, absent, names)
    assert np.all(np.isfinite(per)) and all(np.all(np.isfinite(grads[k])) for k in grads)
    own = AR.own_distances(twin, ref32, AR.RHO_KEYS)
    records = AR.check_rho(dict(grads, per_clip=per), twin, ref32)
    records.append(("mean", abs(float(loss) - twin["loss"]) / max(abs(twin["loss"]), 1.0), records[0][2]))
    own["mean"] = abs(float(ref32["loss"]) - twin["loss"]) / max(abs(twin["loss"]), 1.0)
    _assert(family, label, records, own)


RHO_SHAPES = {
    "columns": [(5, 2, 40, 2, 0.5, 0.3)],                                          # rank <= 2: the column-by-column wave kernels
    "virtual": [(8, 3, 66, 3, 0.5, 0.3)],                                          # rank 3-8: row-array forward + virtual-clip reverse
    "gemm": [(20, 9, 129, 2, 0.2, 0.5), (32, 32, 66, 3, 1e-4, None)],              # padded D, smallest rank k_bwd_rho_mfma takes; full rank
    "wide": [(40, 6, 40, 2, 1e-4, None), (72, 3, 24, 2, 1e-4, None)],              # 40 -> 64 rows; two-wave workgroups, an odd rank
    "block": [(12, 40, 20, 2, 1e-4, None)],                                        # rank > 32: the general kernels at a small D
}


@pytest.mark.parametrize("D,rank,T,B,sigma,rscale", RHO_SHAPES["columns"])
def test_rho_column_kernels(D, rank, T, B, sigma, rscale):
    m, _ = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    _check_rho("rho columns", f"D {D} rank {rank}", m, _rho_refs(D, rank, T, B, sigma, rscale), {"k_fwd_rho_wave"}, {"k_bwd_wave2w", "k_bwd_wave"})


@pytest.mark.parametrize("D,rank,T,B,sigma,rscale", RHO_SHAPES["virtual"] + RHO_SHAPES["gemm"])
def test_rho_gemm_forward_and_virtual_clip_reverse(D, rank, T, B, sigma, rscale):
    """k_fwd_rho_mfma, then the pure-state two-wave reverse scan on one virtual clip per column (the default from rank 3)."""
    m, _ = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    _check_rho("rho virtual", f"D {D} rank {rank}", m, _rho_refs(D, rank, T, B, sigma, rscale), {"k_fwd_rho_mfma", "k_bwd_wave2w"})


@pytest.mark.parametrize("D,rank,T,B,sigma,rscale", RHO_SHAPES["gemm"])
def test_rho_gemm_forward_and_gemm_reverse(D, rank, T, B, sigma, rscale):
    """CMPS_OPT_RHO_BWD = CMPS_RHO_BWD_GEMM: k_bwd_rho_mfma (no event scope of its own: the virtual-clip scans must NOT have run)."""
    from audio_mps_amd import _capi
    m, _ = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    be = m._get_backend()
    _capi.check(be._h, be._lib.cmps_set_option(be._h, _capi.CMPS_OPT_RHO_BWD, _capi.CMPS_RHO_BWD_GEMM))
    _check_rho("rho gemm", f"D {D} rank {rank}", m, _rho_refs(D, rank, T, B, sigma, rscale), {"k_fwd_rho_mfma"}, {"k_bwd_wave2w", "k_bwd_wave"})


@pytest.mark.parametrize("D,rank,T,B,sigma,rscale", RHO_SHAPES["wide"])
def test_rho_wide(D, rank, T, B, sigma, rscale):
    m, _ = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    _check_rho("rho wide", f"D {D} rank {rank}", m, _rho_refs(D, rank, T, B, sigma, rscale),
               {"k_fwd_wide_rho", "k_bwd_wide", "k_grad_gemm", "k_rho_merge_e"})


@pytest.mark.parametrize("D,rank,T,B,sigma,rscale", RHO_SHAPES["block"])
def test_rho_block_above_rank_32(D, rank, T, B, sigma, rscale):
    m, _ = _rho_model(D, rank, T, B, sigma=sigma, rscale=rscale)
    _check_rho("rho block", f"D {D} rank {rank}", m, _rho_refs(D, rank, T, B, sigma, rscale), {"k_fwd_rho"},
               {"k_fwd_rho_mfma", "k_fwd_rho_wave", "k_fwd_wide_rho"})


# ---------------------------------------------------------------------------------------------------
# legacy AudioMPS
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,B", [(5, 34, 3), (32, 66, 3), (40, 34, 2), (64, 66, 2)])
def test_legacy(D, T, B):
    """D <= 32: the wave kernels in legacy mode (no event scope of their own: the wide kernels must not have run); above: the wide kernels
    in legacy mode.  gH and gR through LegacyAudioMPS.chain_rule."""
    from audio_mps_amd import LegacyAudioMPS
    from oracle import cmps_oracle as O
    from _util import make_audio, strict_loss_and_grads
    dt = 0.004
    audio = make_audio(B, T, dt, D, noise=0.05)
    m = LegacyAudioMPS(D, dt, B, data_iterator=audio, seed=D)
    H, R = m.variables["H"], m.variables["R"]
    twin = AR.legacy_twin(audio, H, R, dt, "f64t32")
    ref32 = O.legacy_loss_and_grads(H, R, dt, audio, "f32")
    be = m._get_backend()
    per = m.loss_per_clip()
    (loss, grads), names = _events(be, lambda: strict_loss_and_grads(m))
    wide = {"k_bwd_wide<legacy>", "k_grad_gemm<legacy>"}
    assert (wide <= names) if D > 32 else not (wide & names), names
    own = AR.own_distances(twin, ref32, AR.LEGACY_KEYS)
    records = AR.check_legacy(dict(per_clip=per, gH=grads["H"], gR=grads["R"]), twin, ref32)
    records.append(("mean", abs(float(loss) - twin["loss"]) / max(abs(twin["loss"]), 1.0), records[0][2]))
    own["mean"] = abs(float(ref32["loss"]) - twin["loss"]) / max(abs(twin["loss"]), 1.0)
    assert np.all(np.triu(grads["H"], 1) == 0)
    _assert("legacy", f"D {D} T {T} B {B}", records, own)
