"""A diverged clip must not change its batch-mates' losses: the inputs, the wild clips, the per-clip references and the check shared by
tests/test_wild_host.py (CPU: the references keep the clips of a batch apart, the check catches a coupled kernel) and
tests/test_gpu_wild_clip.py (every forward family on the GPU).  numpy and the oracles only.

Inputs (`base_model`, `base_audio`): sigma = 0.36, A = 1, make_audio(B, T, delta_t, 3) x 0.09, Rx, Ry x 0.69 (x 0.5 above D = 32), model
seed 1 -- tests/_guard.py's settings with A = 1 instead of 66: at A = 66 the losses are about 0.004 and a bar of 1e-5 max(|l|, 1) is an
absolute one that a mate computed as zero would pass; at A = 1 every clip's |loss| is above 0.5 (tests/test_wild_host.py asserts it) and
all of them are finite in the float32 restatement.

The reference of a batch with a wild clip is the reference of the CLEAN batch: the references treat every clip on its own
(tests/test_wild_host.py asserts bit-identity of the mates with and without the wild clip), so the mates' expected losses do not depend
on what the wild clip does.  The wild clip's own loss is judged only where the model itself diverges (`NONFINITE`); for the other kinds a
kernel may say either, it is that clip's own business.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O
from _util import c_oracle_run, make_audio, oracle_hparams, oracle_variables
from _sweep import LOSS_BAR, PAIR_LOSS_BAR, STREAM_FACTOR, NLL_FLOOR, RHO_PRODUCT_FLOOR      # noqa: F401  (the existing bars, re-exported)
import _score_ref as SC
import _rho_score_ref as RS
import _rho_primed_ref as RP

SIGMA, AMP_A, AUDIO_SCALE, R_SCALE, MODEL_SEED, AUDIO_SEED = 0.36, 1.0, 0.09, 0.69, 1, 3
LEGACY_DT, LEGACY_NOISE = 0.004, 0.05                # tests/test_gpu_parity.py::test_legacy_audiomps_matches_oracle
KINDS = ("nan", "inf", "click40", "loud30", "tail", "head")
NONFINITE = ("nan", "inf", "loud30")                 # the float32 restatement gives NaN for these (f32 and f64t32, D = 8 and D = 33)


def wild(kind, clip):
    """A copy of `clip` [T] made wild."""
    c = np.array(clip, dtype=np.float32)
    T = c.shape[0]
    if kind == "nan":
        c[T // 2] = np.nan
    elif kind == "inf":
        c[T // 2] = np.inf
    elif kind == "click40":
        c[T // 2] = np.float32(2.0 ** 40)
    elif kind == "loud30":
        c *= np.float32(2.0 ** 30)
    elif kind == "tail":
        c[T - 1] = np.float32(1e30)                  # only the final increment is wild
    elif kind == "head":
        c[1] = np.float32(2.0 ** 40)                 # the first increment is wild
    else:
        raise ValueError(kind)
    return c


def dirty(audio, kind, j):
    """A copy of the batch `audio` [B, T] whose clip j is wild."""
    out = np.array(audio, dtype=np.float32)
    out[j] = wild(kind, audio[j])
    return out


def _rs(D):
    return np.float32(R_SCALE * (0.5 if D > 32 else 1.0))


@functools.lru_cache(maxsize=None)
def base_audio(B=5, T=66):
    from audio_mps_amd import HParams
    a = (make_audio(B, T, HParams().delta_t, AUDIO_SEED) * np.float32(AUDIO_SCALE)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def legacy_audio(B=5, T=66):
    a = make_audio(B, T, LEGACY_DT, AUDIO_SEED, noise=LEGACY_NOISE)
    a.setflags(write=False)
    return a


def base_model(D, B=5, backend=False, rank=None):
    """The product's PsiCMPS (rank None) or RhoCMPS of the base case; backend=False: host only, no scan is ever run."""
    from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
    hp = HParams(minibatch_size=B, bond_dim=D, sigma=SIGMA, A=AMP_A, initial_rank=rank)
    m = (PsiCMPS if rank is None else RhoCMPS)(hp, seed=MODEL_SEED, backend=backend)
    m.variables["Rx"] *= _rs(D)
    m.variables["Ry"] *= _rs(D)
    return m


def legacy_model(D, B=5, backend=False):
    from audio_mps_amd import LegacyAudioMPS
    return LegacyAudioMPS(D, LEGACY_DT, B, seed=MODEL_SEED, backend=backend)


def base_case(D, B=5, T=66):
    """(host model, audio [B, T]) of the pure-state base case."""
    return base_model(D, B), base_audio(B, T)


# ---------------------------------------------------------------------------------------------------
# per-clip references (float32, each clip on its own)
# ---------------------------------------------------------------------------------------------------
def psi_ref(m, audio, dtype="f32"):
    """The float32 C restatement's per-clip losses."""
    with np.errstate(all="ignore"):
        return np.array(c_oracle_run(m, np.ascontiguousarray(audio, dtype=np.float32), dtype, want_grad=False)["loss_per_clip"])


def pair_ref(m, audio):
    """The bf16-emulating oracle's per-clip losses (the bf16 pair kernels' reference, tests/test_gpu_pair.py)."""
    with np.errstate(all="ignore"):
        return np.array(O.psi_bf16_scan(oracle_hparams(m.hparams), oracle_variables(m), audio, want_grad=False)["loss_per_clip"])


def rho_ref(m, audio):
    ohp, ov, Wx, Wy = RP.oracle_side(m)
    with np.errstate(all="ignore"):
        return np.array(O.rho_loss_and_grads(ohp, ov, Wx, Wy, audio, "f32")["per_clip"])


def legacy_ref(m, audio):
    with np.errstate(all="ignore"):
        return np.array(O.legacy_loss_and_grads(m.variables["H"], m.variables["R"], m.delta_t, audio, "f32")["per_clip"])


def psi_score_ref(m, audio, dtype="f32"):
    """Per-step NLL [B, T - 1] of a batch scored from k0 = 0 (tests/_score_ref.py)."""
    with np.errstate(all="ignore"):
        return SC.score_reference(oracle_hparams(m.hparams), oracle_variables(m), [(SC.SCORE, audio.shape[1] - 1)], audio, None, dtype)[0]


def rho_score_ref(m, audio, dtype="f32"):
    ohp, ov, Wx, Wy = RP.oracle_side(m)
    with np.errstate(all="ignore"):
        return RS.rho_score_reference(ohp, ov, Wx, Wy, [(SC.SCORE, audio.shape[1] - 1)], audio, None, dtype)[0]


def rho_nll_floor(m, audio, mates):
    """tests/test_gpu_rho_stream_score.py's floor of a RhoCMPS step's NLL: NLL_FLOOR + RHO_PRODUCT_FLOOR |R|_F max |x| / A over the mates."""
    ohp, ov, _, _ = RP.oracle_side(m)
    R_fro = float(np.linalg.norm(O.effective_params(ohp, ov.astype(np.float64), "f64")[0]))
    a = np.asarray(audio, dtype=np.float64)[mates]
    return NLL_FLOOR + RHO_PRODUCT_FLOOR * R_fro * float(np.max(np.abs(a[:, 1:] - a[:, :-1]))) / float(ov.A)


# ---------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------
def check_mates(per_dirty, per_clean_ref, j, kind, per_clean_kernel=None, bar=LOSS_BAR, expect_nonfinite=None):
    """Records (what, error, bar) of one batch whose clip j is wild of `kind`: a record fails when error > bar.

      "mate loss"     max over i != j of |per_dirty[i] - ref[i]| / max(|ref[i]|, 1) against `bar` (Inf when a mate is not finite);
      "mates finite"  how many mates are not finite, against 0;
      "wild clip"     1 when the wild clip's own loss came out finite although the model diverges on it, against 0.  That is expected for
                      kind in NONFINITE; a caller whose reference does not diverge on one of those kinds (the legacy arithmetic squares
                      the sample and stays finite at 2^30) passes expect_nonfinite = what its own reference says;
      "dirty - clean" information, bar Inf: max over the mates of |per_dirty[i] - per_clean_kernel[i]| when the caller supplies the same
                      kernel's run of the clean batch.
    """
    per = np.asarray(per_dirty, dtype=np.float64)
    ref = np.asarray(per_clean_ref, dtype=np.float64)
    assert per.shape == ref.shape and np.all(np.isfinite(ref)), "the clean batch's reference must be finite"
    mates = np.array([i for i in range(per.shape[0]) if i != j], dtype=np.int64)
    if expect_nonfinite is None:
        expect_nonfinite = kind in NONFINITE
    with np.errstate(all="ignore"):
        err = np.abs(per[mates] - ref[mates]) / np.maximum(np.abs(ref[mates]), 1.0)
    err = np.where(np.isfinite(per[mates]), err, np.inf)
    rec = [("mate loss", float(np.max(err)), float(bar)),
           ("mates finite", float(np.sum(~np.isfinite(per[mates]))), 0.0),
           ("wild clip", float(bool(expect_nonfinite) and bool(np.isfinite(per[j]))), 0.0)]
    if per_clean_kernel is not None:
        clean = np.asarray(per_clean_kernel, dtype=np.float64)
        with np.errstate(all="ignore"):
            d = np.abs(per[mates] - clean[mates])
        rec.append(("dirty - clean", float(np.max(np.where(np.isfinite(d), d, np.inf))), float("inf")))
    return rec


def failures(records):
    return [r for r in records if not r[1] <= r[2]]


def check_score_mates(nll_dirty, nll32, nll64, j, floor):
    """Records of the mates' per-step NLL rows [T - 1]: distance from the float64 reference of the clean batch against STREAM_FACTOR x
    the float32 reference's own distance + `floor` (the bar of tests/_sweep.py::_stream_records), and their finiteness."""
    got = np.asarray(nll_dirty, dtype=np.float64)
    mates = [i for i in range(got.shape[0]) if i != j]
    r32, r64 = np.asarray(nll32, dtype=np.float64)[mates], np.asarray(nll64, dtype=np.float64)[mates]
    assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
    g = got[mates]
    with np.errstate(all="ignore"):
        d = np.abs(g - r64)
    d = float(np.max(np.where(np.isfinite(g), d, np.inf)))
    return [("mate nll", d, STREAM_FACTOR * float(np.max(np.abs(r32 - r64))) + float(floor)),
            ("mate nll finite", float(np.sum(~np.isfinite(g))), 0.0)]


def worst(records):
    """{what: (error, bar)} with the largest error per kind of record."""
    out = {}
    for what, err, bar in records:
        if what not in out or not err <= out[what][0]:
            out[what] = (err, bar)
    return out
