"""What a scored stream must give for a *plan*: tests/_stream_ref.py::stream_reference with a third kind of step, composed from the same
oracle primitives.  A plan is a list of segments (kind, steps) or (kind, steps, anchored), kind in ("score", "follow", "sample"):

  follow  _psi_update (model.py:269-274) on the clip's increment (:263): records expectation * delta_t, resets the running sum;
  score   the same step, and behind the update, before the normalisation, the fold's increment (model.py:276-282):
          lv = O.inc_loss_psi(updated psi, increment, t_k) = -log(1 + e' x / A), total += lv -- per step to `nll`, summed to `total`;
  sample  _psi_and_sample_update (:284-291).

One time grid runs through all segments.  The forced steps (scored or followed) read ONE clip [n_audio, 1 + F + anchors] through a
column cursor: a step takes clip[c + 1] - clip[c] and moves on; an anchored segment first skips one column (the stream is re-anchored on
its block's first sample without a step, SampleStream.follow(anchor=True)), so the clip holds one column more per anchored segment.  The
function is a plain loop over the steps of the expanded plan, so it cannot depend on the segmentation; tests/test_score_host.py asserts
that once."""
from __future__ import annotations

import functools

import numpy as np

from oracle import cmps_oracle as O
import _primed_ref as PR

SCORE, FOLLOW, SAMPLE = "score", "follow", "sample"


def _seg(seg):
    kind, steps = seg[0], int(seg[1])
    anchored = bool(seg[2]) if len(seg) > 2 else False
    assert kind in (SCORE, FOLLOW, SAMPLE) and steps >= 1 and not (anchored and kind == SAMPLE)
    return kind, steps, anchored


def plan_counts(plan):
    """(scored, followed, sampled, anchors) of a plan."""
    c = {SCORE: 0, FOLLOW: 0, SAMPLE: 0}
    anchors = 0
    for seg in plan:
        kind, steps, anchored = _seg(seg)
        c[kind] += steps
        anchors += anchored
    return c[SCORE], c[FOLLOW], c[SAMPLE], anchors


def clip_columns(plan):
    """Columns of the clip a plan reads."""
    s, f, _, a = plan_counts(plan)
    return 1 + s + f + a


def expand(plan):
    """One (kind, skip) per step: skip = the step is the first of an anchored segment."""
    steps = []
    for seg in plan:
        kind, m, anchored = _seg(seg)
        steps += [(kind, anchored and j == 0) for j in range(m)]
    return steps


def refine(plan):
    """Every segment cut again at its middle and one step in (the anchor stays with the first piece)."""
    out = []
    for seg in plan:
        kind, m, anchored = _seg(seg)
        cuts = sorted({c for c in (1, m // 2) if 0 < c < m})
        lo = 0
        for hi in cuts + [m]:
            out.append((kind, hi - lo, anchored and lo == 0))
            lo = hi
    assert expand(out) == expand(plan)
    return out


def score_reference(hp: O.HParams, var: O.Variables, plan, clip, noise=None, dtype="f32", start=None, n=None):
    """clip [n_audio, clip_columns(plan)] (n_audio = n, or 1: shared; None without forced steps), noise [sampled, n] or None ->
    (nll [n, scored], total [n], pred [n, scored + followed], out [n, sampled], carry).  carry = (psi [n, D], running sum [n], step index,
    total [n], clip cursor); `start` = a carry to resume from (the cursor then indexes the clip handed to THIS call, i.e. restart it at 0
    with the overlap column first), None: psi_0 at t_0 with total 0."""
    real = np.float32 if dtype == "f32" else np.float64
    cplx = np.complex64 if dtype == "f32" else np.complex128
    v = var if dtype == "f32" else var.astype(np.float64)
    R, freqs, _, _ = O.effective_params(hp, v, dtype)
    A = real(v.A)
    S, F, L, _ = plan_counts(plan)
    if clip is not None:
        clip = np.asarray(clip, dtype=real)
        clip = clip[None, :] if clip.ndim == 1 else clip
    if n is None:
        n = np.shape(noise)[1] if noise is not None else clip.shape[0]
    noise = np.zeros((0, n), dtype=real) if noise is None else np.asarray(noise, dtype=real)
    assert noise.shape == (L, n)
    if S + F:
        clip = np.tile(clip, (n, 1)) if clip.shape[0] == 1 else clip
        assert clip.shape == (n, clip_columns(plan))
    if start is None:
        psi = np.tile(O.psi_0(v, dtype)[None, :], (n, 1)).astype(cplx)        # model.py:245, :260
        run, k0, total = np.zeros(n, dtype=real), 0, np.zeros(n, dtype=real)  # model.py:244, :266
    else:
        psi, run, k0, total = start[0].astype(cplx), start[1].astype(real), int(start[2]), start[3].astype(real)
    t = O.time_table(hp.delta_t, k0 + S + F + L, dtype)
    nll, pred, out = np.empty((n, S), dtype=real), np.empty((n, S + F), dtype=real), np.empty((n, L), dtype=real)
    c = jn = jf = js = 0
    for j, (kind, skip) in enumerate(expand(plan)):
        tk = t[k0 + j]
        edt = (O.expectation(psi, tk, R, freqs, dtype) * real(hp.delta_t)).astype(real)
        if kind == SAMPLE:                                                    # _psi_and_sample_update
            inc = (edt + noise[js]).astype(real)                              # :286
            run = (run + inc).astype(real)                                    # :287
            out[:, js] = A * run                                              # :251
            js += 1
        else:                                                                 # _psi_update
            c += skip
            inc = (clip[:, c + 1] - clip[:, c]).astype(real)                  # :263
            c += 1
            pred[:, jf] = edt
            run = np.zeros(n, dtype=real)
            jf += 1
        psi = O.update_ancilla_psi(psi, inc, tk, R, freqs, A, hp, dtype)      # :288 / :278
        if kind == SCORE:
            lv = O.inc_loss_psi(psi, inc, tk, R, freqs, A, dtype)             # :279, :293-294 on the updated, un-normalised state
            nll[:, jn] = lv
            total = (total + lv).astype(real)
            jn += 1
        psi = O.normalize_psi(psi, axis=1, dtype=dtype)                       # :289 / :280
    return nll, total, pred, out.astype(real), (psi, run, k0 + S + F + L, total, c)


# ---------------------------------------------------------------------------------------------------
# shared cases: the model of tests/_primed_ref.py, damped-sine clips seeded with D
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_clip(D, n, columns):
    """O.damped_sine(n, columns, dt, seed=D): computed once, shared, never written to."""
    clip = O.damped_sine(n, columns, PR.case_hparams(D, n).delta_t, seed=D)
    clip.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def case_reference(D, n, segments, dtype="f32"):
    """score_reference of a case whose plan scores `segments` (a tuple of step counts) from k0 = 0: (nll, total, pred), computed once per
    (case, dtype) and shared by the tests that need it."""
    plan = [(SCORE, m) for m in segments]
    clip = case_clip(D, n, clip_columns(plan))
    nll, total, pred, _, _ = score_reference(PR.case_hparams(D, n), PR.case_variables(D, n), plan, clip, None, dtype)
    for a in (nll, total, pred):
        a.setflags(write=False)
    return nll, total, pred
