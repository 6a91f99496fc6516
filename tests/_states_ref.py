"""State read-outs (cmps_psi_states: k_states; cmps_rho_states: k_states_rho) against the float64 oracle: the case tables, the inputs of
a case and one reference routine per model.  The CPU conditions (tests/test_states_host.py), the GPU tests (tests/test_gpu_states.py) and
scripts/states_parity.py all read this module; importing it needs numpy and the oracle only (the product is imported by the runners at
the bottom, when they are called).

Reference: O.psi_loss_per_clip / O.rho_loss_per_clip(..., return_states=True) in "f64t32" -- float64 arithmetic on the float32 time grid
the kernels follow, the variables cast to float64 -- so the distance of a float32 evaluation from it is rounding alone.  The same
routines with dtype "f32" give the float32 oracle's own distance d32, which the bars are built from.

Every stash layout the two kernels decode is one family of cases: STASH_WAVE16 / WAVE32 / WIDE / PAIR / BLOCK (cmps_block.hip) and
RHO_STASH_WAVE / MFMA / WIDE / BLOCK (cmps_rho.hip)."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from oracle import cmps_oracle as O
from _util import make_audio

# include/cmps.h
AUTO, BLOCK, WAVE, PAIR, WAVE32, WIDE = 0, 1, 2, 3, 4, 5
RANK1_BF16X3, RANK1_F16X2, RANK1_DEFAULT = 2, 3, 4
CHAIN_VALU, CHAIN_MFMA, CHAIN_MFMA_FWD = 0, 1, 2

# ---------------------------------------------------------------------------------------------------
# bars and caps (conditions of the issue, not measurements)
# ---------------------------------------------------------------------------------------------------
PSI_BAR = 1e-5           # max |hip - f64t32| on unit vectors: the figure of the kernel-against-kernel state checks (test_gpu_parity / _wide)
PAIR_BAR = 5e-3          # bf16 mat-vec operands: the figure of tests/test_gpu_pair.py
PSI_D32_CAP = 2e-6       # the float32 oracle's own distance from f64t32 stays below this, so PSI_BAR >= 5 d32 is a constant
RHO_FLOOR = 1e-5         # rel_inf(hip, f64t32) <= max(RHO_FLOOR, 3 d32): tests/test_gpu_rho.py::_check_elastic's construction
RHO_D32_CAP = 1e-5       # relative to max |rho|: no elastic bar exceeds 3e-5
QFLAG_LIMIT = 2.0 ** -19  # k_qflag (cmps_prep.hip): |Q|_F at or below it selects the Q-free instance of the chain16 kernels (D > 32)

INIT = (1e-4, None)      # the reference's initialisation: |Q|_F is tiny (sigma^2 delta_t / 2 = 3e-13)
VISIBLE = (0.3, 0.3)     # (sigma, R scale): Q = -(delta_t sigma^2 / 2) R^dagger R is visible


class PsiCase(NamedTuple):
    layout: str                          # the stash layout k_states must decode
    D: int
    variant: int                         # what HipScan is asked for (AUTO resolves by D)
    options: Tuple[Tuple[str, int], ...]  # (("rank1", mode),) or (("wide_chain", mode),)
    T: int
    B: int
    sigma: float
    rscale: Optional[float]
    amp: float = 1.0                     # the audio is scaled by it (the pair cases: see PAIR_AMP)

    @property
    def bar(self):
        return PAIR_BAR if self.layout == "pair" else PSI_BAR

    @property
    def id(self):
        opt = "".join(f"-{k}{v}" for k, v in self.options)
        return f"{self.layout}-D{self.D}-T{self.T}-B{self.B}-s{self.sigma:g}{opt}"


class RhoCase(NamedTuple):
    layout: str
    D: int
    rank: int
    variant: int
    T: int
    B: int
    sigma: float
    rscale: Optional[float]

    @property
    def id(self):
        return f"{self.layout}-D{self.D}-r{self.rank}-T{self.T}-s{self.sigma:g}-v{self.variant}"


# What each layout's forward is called in cmps_kernel_times, and the variant the backend must report.
PSI_VARIANT = {"wave16": WAVE, "wave32": WAVE32, "wide": WIDE, "pair": PAIR, "block": BLOCK}
RHO_FWD_KERNEL = {"wave": "k_fwd_rho_wave", "mfma": "k_fwd_rho_mfma", "wide": "k_fwd_wide_rho", "block": "k_fwd_rho"}


def psi_fwd_kernel(case) -> str:
    if case.layout == "wide":       # the chain kernel of the training forward: fp32 VALU, or fp16 x 2 operands on the matrix cores
        return "k_fwd_wide" if dict(case.options)["wide_chain"] == CHAIN_VALU else "k_fwd_chain16"
    return {"wave16": "k_fwd_wave16", "wave32": "k_fwd_wave2", "pair": "k_fwd_pair", "block": "k_fwd_block"}[case.layout]


# The pair bar is 5e-3 absolute, so its cases must move by 5e-2 per step and differ by 5e-2 between clips (tests/test_states_host.py):
# louder audio.  The error of bf16 mat-vec operands is relative to what a step adds (2^-9 of s R u, summed over the steps), so an
# absolute bar asks for no more motion than the discrimination needs: per case the smallest even factor at which every clip's largest
# step and every two clips' largest difference reach PAIR_MOTION = 6e-2 (1.2 x 10 x the bar) in the reference.
PAIR_MOTION = 6e-2
PAIR_AMP = {(40, INIT): 6.0, (40, VISIBLE): 18.0, (128, INIT): 6.0, (128, VISIBLE): 16.0}


def _psi_cases():
    cases = []
    # STASH_WAVE16: D <= 16 under AUTO and under WAVE; 65 steps run over the 32-step forward chunks and the 64-step scalar chunks; B = 5
    # leaves a workgroup of four clips and one of one
    for D, variant in ((3, AUTO), (16, WAVE)):
        for sigma, rs in (INIT, VISIBLE):
            cases.append(PsiCase("wave16", D, variant, (), 66, 5, sigma, rs))
    # STASH_WAVE32: rows 16 ... 31 of a stash row are read at D = 17, 24, 32; both loss-wave arithmetics at D = 17 and D = 32
    for D in (9, 17, 24, 32):
        modes = (RANK1_DEFAULT, RANK1_BF16X3) if D in (17, 32) else (RANK1_DEFAULT,)
        for mode in modes:
            for T in (34, 66, 131):
                cases.append(PsiCase("wave32", D, WAVE32, (("rank1", mode),), T, 5 if T != 66 else 7, *VISIBLE))
            cases.append(PsiCase("wave32", D, WAVE32, (("rank1", mode),), 131, 5, *INIT))
    # STASH_WIDE: the padded sizes 64 (D = 33: one row beyond a wave's 32; D = 64), 96 (D = 72) and 128; B = 3: the last pair holds one clip
    for D in (33, 64, 72, 128):
        for chain in (CHAIN_VALU, CHAIN_MFMA, CHAIN_MFMA_FWD):
            for T in (10, 67):
                cases.append(PsiCase("wide", D, AUTO, (("wide_chain", chain),), T, 3, *VISIBLE))
            cases.append(PsiCase("wide", D, AUTO, (("wide_chain", chain),), 67, 3, *INIT))
    for D in (40, 128):
        for sigma, rs in (INIT, VISIBLE):
            cases.append(PsiCase("pair", D, PAIR, (), 67, 3, sigma, rs, PAIR_AMP[D, (sigma, rs)]))
    # STASH_BLOCK: D = 65 and 128 run two-wave workgroups (the red[] path of k_states)
    for D in (1, 2, 65, 128):
        for sigma, rs in (INIT, VISIBLE):
            cases.append(PsiCase("block", D, BLOCK, (), 67, 3, sigma, rs))
    return cases


def _rho_cases():
    cases = []
    vis = VISIBLE
    # D <= 32, rank <= 8: the column-by-column wave kernels.  A forward that saves for the default reverse sweep (CMPS_RHO_BWD_VIRTUAL)
    # takes the row-array GEMM kernel from rank 3 already (cmps_rho_loss_fwd), so AUTO reaches RHO_STASH_WAVE at rank <= 2 only; above,
    # CMPS_VARIANT_WAVE32 asks for the column kernels
    for (D, r), variant in (((7, 3), WAVE32), ((12, 1), AUTO), ((32, 8), WAVE32)):
        for T in (66, 131):
            cases.append(RhoCase("wave", D, r, variant, T, 3, *vis))
    cases.append(RhoCase("wave", 7, 3, WAVE32, 66, 3, *INIT))
    for D, r in ((20, 9), (24, 17), (32, 32)):                                          # rank > 8: row-array GEMM forward
        for T in (66, 131):
            cases.append(RhoCase("mfma", D, r, AUTO, T, 3, *vis))
    cases.append(RhoCase("mfma", 20, 9, AUTO, 66, 3, *INIT))
    for D, r in ((7, 3), (32, 8)):                                                      # what AUTO runs at 3 <= rank <= 8 when it saves
        cases.append(RhoCase("mfma", D, r, AUTO, 66, 3, *vis))
    # D > 32: the columns as virtual clips of the wide kernels; (40, 7): odd rank, a zero column pads the last pair
    for D, r, T in ((40, 7, 40), (64, 1, 40), (64, 16, 33), (96, 9, 40), (48, 48, 24), (128, 24, 20)):
        cases.append(RhoCase("wide", D, r, AUTO, T, 3, *vis))
    cases.append(RhoCase("wide", 40, 7, AUTO, 40, 3, *INIT))
    # CMPS_VARIANT_BLOCK: the general kernels; (128, 128) is the largest LDS request of k_states_rho
    for D, r, T in ((7, 7, 40), (40, 3, 40), (72, 5, 30), (128, 128, 6)):
        cases.append(RhoCase("block", D, r, BLOCK, T, 3, *vis))
    cases.append(RhoCase("block", 7, 7, BLOCK, 40, 3, *INIT))
    return cases


PSI_CASES = _psi_cases()
RHO_CASES = _rho_cases()
FLOOR_VARIANTS = (BLOCK, WAVE)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _seed(*key):
    return int(sum(key))


# d32 of a RhoCMPS case is led by the rounding of fl(freqs t) in the phases, |f| t 2^-24 per phase with |f| up to ~1e4 and t up to
# 130 delta_t: the T = 131 cases draw 6e-6 ... 1.1e-5 depending on freqs.  The cap is 1e-5 and stays; the draw is what may change.  Bases
# 0, 100, 200, 300, 400 give a largest d32 of 1.06e-5, 8.8e-6, 8.7e-6, 8.5e-6, 8.4e-6 over the table: the first that meets the cap.
RHO_SEED_BASE = 100


# ---------------------------------------------------------------------------------------------------
# inputs: the oracle's own initialisation (numpy only); the runners below hand the same variables to the product
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def psi_inputs(D, T, B, sigma, rscale, amp):
    """(oracle HParams, oracle Variables, audio [B, T]) of a pure-state case; computed once, shared, never written to."""
    hp = O.HParams(minibatch_size=B, bond_dim=D, sigma=sigma)
    seed = _seed(D, T)
    var = O.init_variables(hp, seed=seed)
    if rscale is not None:
        var.Rx = (var.Rx * np.float32(rscale)).astype(np.float32)
        var.Ry = (var.Ry * np.float32(rscale)).astype(np.float32)
    audio = (make_audio(B, T, hp.delta_t, seed) * np.float32(amp)).astype(np.float32)
    _freeze(var.Rx, var.Ry, var.freqs, var.psi_x, var.psi_y, audio)
    return hp, var, audio


def case_inputs(case):
    if isinstance(case, RhoCase):
        return rho_inputs(case.D, case.rank, case.T, case.B, case.sigma, case.rscale)
    return psi_inputs(case.D, case.T, case.B, case.sigma, case.rscale, case.amp)


@functools.lru_cache(maxsize=None)
def rho_inputs(D, rank, T, B, sigma, rscale):
    """(oracle HParams, oracle Variables, Wx, Wy, audio [B, T]) of a RhoCMPS case."""
    hp = O.HParams(minibatch_size=B, bond_dim=D, sigma=sigma, initial_rank=rank)
    seed = _seed(RHO_SEED_BASE, D, rank, T)
    var = O.init_variables(hp, seed=seed)
    if rscale is not None:
        var.Rx = (var.Rx * np.float32(rscale)).astype(np.float32)
        var.Ry = (var.Ry * np.float32(rscale)).astype(np.float32)
    var.psi_x, var.psi_y = np.zeros(D, np.float32), np.zeros(D, np.float32)       # unused on this path
    Wx, Wy = O.rho_init_W(hp, seed=seed)
    audio = make_audio(B, T, hp.delta_t, seed)
    _freeze(var.Rx, var.Ry, var.freqs, Wx, Wy, audio)
    return hp, var, Wx, Wy, audio


FLOOR_T, FLOOR_A, FLOOR_R = 40, 4.0, 2.0


@functools.lru_cache(maxsize=None)
def floor_inputs():
    """tests/test_gpu_parity.py::test_normalisation_floor_branch: two levels, R = [[0, a], [a, 0]], psi_0 = the +a eigenvector, sigma = 0,
    and clip 1's first increment x = -A / a, so that (1 + s R) u = 0 at step 0: |y|^2 = 0 <= 1e-12 (model.py:332)."""
    a, A = FLOOR_R, FLOOR_A
    hp = O.HParams(minibatch_size=3, bond_dim=2, sigma=0.0, A=A)
    var = O.init_variables(hp, R_in=np.array([[0, a], [a, 0]], dtype=np.complex64), freqs_in=np.array([3.0, -5.0], dtype=np.float32),
                           psi_in=np.array([1, 1], dtype=np.complex64))
    audio = make_audio(3, FLOOR_T, hp.delta_t, 77, noise=0.05)
    audio[1, 0] = 0.0
    audio[1, 1] = -A / a
    _freeze(var.Rx, var.Ry, var.freqs, var.psi_x, var.psi_y, audio)
    return hp, var, audio


# ---------------------------------------------------------------------------------------------------
# the reference routines
# ---------------------------------------------------------------------------------------------------
def _cast(var, dtype):
    return var if dtype == "f32" else var.astype(np.float64)


def psi_states_reference(hp, var, audio, dtype="f64t32"):
    """What psi_evolve_with_data returns (model.py:231-240): the normalised lab-frame psi after every step, [B, T - 1, D].  Also the
    per-clip loss [B] of the same run (a case whose loss is not finite has left the model's domain: 1 + z <= 0)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        loss, states = O.psi_loss_per_clip(hp, _cast(var, dtype), audio, dtype, return_states=True)
    return states, loss


def rho_states_reference(hp, var, Wx, Wy, audio, dtype="f64t32"):
    """What rho_evolve_with_data returns (model.py:76-84): the trace-normalised rho after every step, [B, T - 1, D, D]; its purity
    Re tr(rho_k^2) [B, T - 1] (model.py:101); the per-clip loss [B]."""
    wt = np.float32 if dtype == "f32" else np.float64
    with np.errstate(invalid="ignore", divide="ignore"):
        loss, rhos = O.rho_loss_per_clip(hp, _cast(var, dtype), np.asarray(Wx, dtype=wt), np.asarray(Wy, dtype=wt), audio, dtype,
                                         return_states=True)
    purity = np.einsum('abcd,abdc->ab', rhos, rhos).real.astype(wt)
    return rhos, purity, loss


@functools.lru_cache(maxsize=None)
def case_reference(case, dtype="f64t32"):
    """The reference of a case in `dtype`, computed once and shared: (states, loss) or (rhos, purity, loss).  Cases that differ only in
    the kernel they select (variant, options) share their inputs and therefore this result."""
    if isinstance(case, RhoCase):
        return _rho_reference(case.D, case.rank, case.T, case.B, case.sigma, case.rscale, dtype)
    return _psi_reference(case.D, case.T, case.B, case.sigma, case.rscale, case.amp, dtype)


@functools.lru_cache(maxsize=None)
def _psi_reference(D, T, B, sigma, rscale, amp, dtype):
    res = psi_states_reference(*psi_inputs(D, T, B, sigma, rscale, amp), dtype)
    _freeze(*res)
    return res


@functools.lru_cache(maxsize=None)
def _rho_reference(D, rank, T, B, sigma, rscale, dtype):
    res = rho_states_reference(*rho_inputs(D, rank, T, B, sigma, rscale), dtype)
    _freeze(*res)
    return res


@functools.lru_cache(maxsize=None)
def floor_reference(dtype="f64t32"):
    res = psi_states_reference(*floor_inputs(), dtype)
    _freeze(*res)
    return res


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.complex128) - np.asarray(b, dtype=np.complex128))))


def rel_inf(a, b):
    return max_abs(a, b) / max(float(np.max(np.abs(b))), 1e-300)


def psi_d32(case):
    """max |oracle_f32 - f64t32| of a pure-state case."""
    return max_abs(case_reference(case, "f32")[0], case_reference(case, "f64t32")[0])


def rho_d32(case):
    """(rel_inf of rho, rel_inf of the purity) of the float32 oracle against f64t32."""
    r32, p32, _ = case_reference(case, "f32")
    rt, pt, _ = case_reference(case, "f64t32")
    return rel_inf(r32, rt), rel_inf(p32, pt)


def rho_bars(case):
    """(bar on rel_inf(rho), bar on rel_inf(purity)): max(1e-5, 3 d32) each."""
    d_rho, d_pur = rho_d32(case)
    return max(RHO_FLOOR, 3 * d_rho), max(RHO_FLOOR, 3 * d_pur)


def q_frobenius(hp, var):
    """|Q|_F of Q = -(delta_t sigma^2 / 2) R^dagger R (model.py:312), what k_qflag compares with 2^-19."""
    R = O.effective_params(hp, var.astype(np.float64), "f64")[0]
    return float(np.linalg.norm(0.5 * hp.delta_t * hp.sigma ** 2 * (np.conj(R.T) @ R)))


# ---------------------------------------------------------------------------------------------------
# runners (GPU): the product's model holding exactly the case's variables, one saved forward, the read-out
# ---------------------------------------------------------------------------------------------------
def _with_events(be, fn):
    """fn() with CMPS_OPT_KERNEL_EVENTS on -> (its result, the names cmps_kernel_times reports)."""
    be.kernel_events(True)
    try:
        out = fn()
        names = set(be.kernel_times())
    finally:
        be.kernel_events(False)
    return out, names


def psi_model(hp, var, audio, variant=AUTO, options=()):
    from audio_mps_amd import HParams, PsiCMPS
    from audio_mps_amd.scan import HipScan
    be = HipScan(hp.bond_dim, variant=variant)
    for name, value in options:
        getattr(be, "set_" + name)(value)
    kw = {}
    if not var.scaled_R:
        kw["R_in"] = (var.Rx + 1j * var.Ry).astype(np.complex64)
    if not var.scaled_freqs:
        kw["freqs_in"] = var.freqs
    m = PsiCMPS(HParams(**vars(hp)), data_iterator=np.array(audio), backend=be, **kw)       # (a writable copy: the shared inputs stay frozen)
    for k in O.Variables.NAMES:
        m.variables[k] = np.array(getattr(var, k), dtype=np.float32)
    return m


def run_psi(hp, var, audio, variant=AUTO, options=()):
    """psi_evolve_with_data on the GPU -> dict(states, again (a second read of the same saved forward), variant, rank1, wide_chain,
    kernels (names of the forward's kernels))."""
    m = psi_model(hp, var, audio, variant, options)
    be = m._get_backend()
    states, names = _with_events(be, m.psi_evolve_with_data)
    return dict(states=states, again=be.states(), variant=be.variant, rank1=be.rank1, wide_chain=be.wide_chain, kernels=names)


def run_psi_case(case):
    return run_psi(*case_inputs(case), variant=case.variant, options=case.options)


def run_rho_case(case):
    """rho_evolve_with_data on the GPU, then the read-outs of cmps_rho_states on the same saved forward -> dict(rho (the model's return),
    rho2, purity (want_rho and want_purity together), purity_only, kernels)."""
    from audio_mps_amd import HParams, RhoCMPS
    from audio_mps_amd.scan import HipScan
    hp, var, Wx, Wy, audio = case_inputs(case)
    be = HipScan(case.D, variant=case.variant)
    m = RhoCMPS(HParams(**vars(hp)), data_iterator=np.array(audio), backend=be)
    for k in ("A", "Rx", "Ry", "freqs"):
        m.variables[k] = np.array(getattr(var, k), dtype=np.float32)
    m.variables["Wx"], m.variables["Wy"] = Wx.copy(), Wy.copy()
    assert m.rank_rho_0 == case.rank
    rho, names = _with_events(be, m.rho_evolve_with_data)
    rho2, purity = be.rho_states(case.B, case.T - 1, want_rho=True, want_purity=True)
    purity_only = be.rho_states(case.B, case.T - 1, want_rho=False, want_purity=True)
    return dict(rho=rho, rho2=rho2, purity=purity, purity_only=purity_only, kernels=names)
