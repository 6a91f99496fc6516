"""A diverged clip must not change its batch-mates' losses, on a real MI355X: every forward family that packs several clips into one
workgroup, with one clip of the batch made wild (tests/_wild_ref.py: NaN, +Inf, a 2^40 click, the whole clip x 2^30, a wild last or first
increment), at both members of a pair and at the lone last clip of the odd batch.  `evaluate` (README, "Evaluating") promises that a
non-finite clip "enters nothing else", and include/cmps.h that a NaN or Inf propagates into THAT clip's loss.

Every mate is judged against the per-clip reference of the CLEAN batch at the project's existing bars (tests/_sweep.py): the float32 C
restatement at LOSS_BAR for the float32 families, oracle.psi_bf16_scan at PAIR_LOSS_BAR for the bf16 pair kernels, the numpy oracles for
RhoCMPS and the legacy arithmetic; the per-step scores against tests/_score_ref.py / _rho_score_ref.py at the stream tests' floors.  The
wild clip's own loss must be non-finite where the model itself diverges on it (NaN, Inf, x 2^30) and is not judged otherwise.  Each case
prints the worst mate error against its bar and the worst difference between the mates' losses in the dirty and in the clean batch of the
same kernel (information: bit-identity is not asked for).

Both forward entries run: save_for_bwd = 0 on a forward-only workspace (what loss_per_clip and evaluate run) and save_for_bwd = 1 on a
TRAIN workspace (the training forward: other kernels above D = 32).

What these cases found when they were written, all in the training forward above D = 32 and all at both members of a pair (j = 0, 1):
k_fwd_chain16 (every wide case with the MFMA chain) took one vector scale sV from the largest increment of BOTH clips, and an Inf, 2^40
or x 2^30 clip flushed its mate's fp16 pieces to zero (mate error 0.98 ... 1.08 of |l|: the correction (Q + s R) u computed as zero);
k_hy_wide<f16x2> (CMPS_RANK1_DEFAULT, also under the VALU chain and in the legacy arithmetic at D = 40, 64) took one scale sB from the
largest |y|^2 of both clips, with the same effect for click40, head, tail and loud30 (error 1.0: e = 0 at every step).  Both scales are
per clip now.  The forward-only entry, the wave, block and bf16 pair kernels, RhoCMPS (its column pairs never span two clips: the
rank is padded to even) and the scored streams kept every mate bit-identical to the clean batch."""
import functools

import numpy as np
import pytest
import torch

import _wild_ref as W
import _eval_ref as ER

pytestmark = pytest.mark.gpu

AUTO, BLOCK, WAVE, PAIR, WAVE32, WIDE = 0, 1, 2, 3, 4, 5
VALU, MFMA, MFMA_FWD = 0, 1, 2                          # CMPS_OPT_WIDE_CHAIN
BF16X3, DEFAULT = 2, 4                                  # CMPS_OPT_RANK1
B, T = 5, 66


@functools.lru_cache(maxsize=None)
def _psi_ref(D):
    """The float32 restatement's losses of the clean base case: computed once per D, shared, never written to."""
    ref = W.psi_ref(*W.base_case(D, B, T))
    ref.setflags(write=False)
    return ref


def _run_family(name, m, audio, ref, positions, bar=W.LOSS_BAR, ref_dirty=None):
    """Both forward entries over every kind and position; prints the family's worst figures and asserts every record.
    ref_dirty(audio) -> the reference's own losses of a dirty batch, for a family whose reference need not diverge on W.NONFINITE."""
    dev = m._get_backend().device
    records, failed = [], []
    for save in (False, True):
        be = m._prepare(audio.shape[0], audio.shape[1], train=save)
        fwd = m._forward_entry(be)

        def run(a):
            return fwd(torch.from_numpy(np.ascontiguousarray(a)).to(dev), save_for_bwd=save).cpu().numpy().copy()
        clean = run(audio)
        err = float(np.max(np.abs(clean - ref) / np.maximum(np.abs(ref), 1.0)))
        print(f"{name} save_for_bwd={int(save)}: clean batch {err:.3e} (bar {bar:.1e})")
        assert np.all(np.isfinite(clean)) and err <= bar, (name, "clean batch", save, err, bar)
        for kind in W.KINDS:
            for j in positions:
                bad = W.dirty(audio, kind, j)
                expect = None
                if ref_dirty is not None and kind in W.NONFINITE:
                    expect = not np.isfinite(ref_dirty(bad)[j])
                rec = W.check_mates(run(bad), ref, j, kind, clean, bar=bar, expect_nonfinite=expect)
                records += rec
                failed += [(kind, j, "save" if save else "fwd") + f for f in W.failures(rec)]
    w = W.worst(records)
    print(f"{name}: worst mate error {w['mate loss'][0]:.3e} (bar {w['mate loss'][1]:.1e}), worst |dirty - clean| {w['dirty - clean'][0]:.3e}, "
          f"{len(failed)} of {len(records)} records failed")
    assert not failed, (name, sorted({f[:4] for f in failed}), max(failed, key=lambda f: f[4]))


def _psi(D, variant=AUTO, rank1=None, chain=None):
    from audio_mps_amd.scan import HipScan
    be = HipScan(D, variant=variant, rank1=rank1)
    if chain is not None:
        be.set_wide_chain(chain)
    return W.base_model(D, B, backend=be)


@pytest.mark.parametrize("family,D,variant,expected", [("wave16", 3, AUTO, WAVE), ("wave16", 16, AUTO, WAVE), ("wave", 17, AUTO, WAVE),
                                                       ("wave", 32, AUTO, WAVE), ("wave32", 9, WAVE32, WAVE32), ("block", 5, BLOCK, BLOCK),
                                                       ("block", 48, BLOCK, BLOCK)])
def test_wave_and_block_mates(family, D, variant, expected):
    m = _psi(D, variant)
    assert m._get_backend().variant == expected
    _run_family(f"{family} D={D}", m, W.base_audio(B, T), _psi_ref(D), (0, 1, 4))


@pytest.mark.parametrize("rank1", [DEFAULT, BF16X3])
@pytest.mark.parametrize("chain", [VALU, MFMA, MFMA_FWD])
@pytest.mark.parametrize("D", [33, 96, 128])
def test_wide_mates(D, chain, rank1):
    m = _psi(D, AUTO, rank1=rank1, chain=chain)
    assert m._get_backend().variant == WIDE and m._get_backend().wide_chain == chain
    _run_family(f"wide D={D} chain={chain} rank1={rank1}", m, W.base_audio(B, T), _psi_ref(D), (0, 1, 4))


@pytest.mark.parametrize("D", [40, 128])
def test_pair_mates(D):
    m = _psi(D, PAIR)
    assert m._get_backend().variant == PAIR
    audio = W.base_audio(B, T)
    _run_family(f"pair D={D}", m, audio, W.pair_ref(m, audio), (0, 1, 4), bar=W.PAIR_LOSS_BAR)


@pytest.mark.parametrize("D", [12, 40, 64])
def test_legacy_mates(D):
    from audio_mps_amd.scan import HipScan
    m = W.legacy_model(D, B, backend=HipScan(D))
    audio = W.legacy_audio(B, T)
    # the legacy loss squares the sample: x 2^30 stays finite in its oracle (1e18), so the oracle says where the clip must diverge
    _run_family(f"legacy D={D}", m, audio, W.legacy_ref(m, audio), (0, 1, 4), ref_dirty=lambda a: W.legacy_ref(m, a))


@pytest.mark.parametrize("D,rank", [(8, 3), (20, 9), (32, 32), (40, 3), (72, 3), (64, 4)])
def test_rho_mates(D, rank):
    from audio_mps_amd.scan import HipScan
    m = W.base_model(D, 3, backend=HipScan(D), rank=rank)
    audio = W.base_audio(3, 24 if D > 32 else T)
    _run_family(f"rho D={D} rank={rank}", m, audio, W.rho_ref(m, audio), (0, 1, 2))


# ---------------------------------------------------------------------------------------------------
# per-step scores: the samplers' score mode (two paths per workgroup above D = 32, four per workgroup below)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rank", [(8, None), (32, None), (96, None), (32, 32), (40, 3)])
def test_score_mates(D, rank):
    from audio_mps_amd.scan import HipScan
    rho = rank is not None
    n = 3 if rho else B
    audio = W.base_audio(n, 24 if rho and D > 32 else T)
    m = W.base_model(D, n, backend=HipScan(D), rank=rank)
    score_ref = W.rho_score_ref if rho else W.psi_score_ref
    n32, n64 = score_ref(m, audio, "f32"), score_ref(m, audio, "f64")
    assert np.all(np.isfinite(n32)) and np.all(np.isfinite(n64)) and float(np.max(np.abs(n32))) > 1e-3
    records, failed = [], []
    for kind in W.KINDS:
        for j in ((0, 1, 2) if rho else (0, 1, 4)):
            bad = W.dirty(audio, kind, j)
            mates = [i for i in range(n) if i != j]
            floor = W.rho_nll_floor(m, audio, mates) if rho else W.NLL_FLOOR
            nll = m.nll_per_step(bad)
            assert nll.shape == (n, audio.shape[1] - 1)
            rec = W.check_score_mates(nll, n32, n64, j, floor)
            # the mates' totals against their loss_per_clip of the same batch (another kernel: the bar of
            # tests/test_gpu_stream_score.py::test_sample_stream_score_matches_loss_per_clip)
            per = m.loss_per_clip(bad).astype(np.float64)[mates]
            tot = np.sum(nll.astype(np.float64), axis=1)[mates]
            with np.errstate(all="ignore"):
                d = np.abs(tot - per) / np.maximum(np.abs(per), 1.0)
            rec.append(("mate total", float(np.max(np.where(np.isfinite(tot) & np.isfinite(per), d, np.inf))), 2 * W.LOSS_BAR))
            records += rec
            failed += [(kind, j) + f for f in W.failures(rec)]
    w = W.worst(records)
    print(f"score D={D} rank={rank}: worst mate nll distance {w['mate nll'][0]:.3e} (bar {w['mate nll'][1]:.3e}), worst total "
          f"{w['mate total'][0]:.3e} (bar {w['mate total'][1]:.1e}), {len(failed)} of {len(records)} records failed")
    assert not failed, failed[:12]


# ---------------------------------------------------------------------------------------------------
# evaluate end to end
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 33])
def test_evaluate_keeps_wild_clips_out_of_everything_else(D):
    """7 clips, minibatch 4 (a ragged last batch of 3), clip 2 with an Inf sample and clip 5 with a 2^40 click.

    n_nonfinite and first_nonfinite are those of the per-clip losses that come back with keep_losses (a click may leave its clip finite:
    its own business).  The statistics are checked twice: against tests/_eval_ref.py on the returned losses at the bars of
    tests/test_gpu_evaluate.py (sums to 1e-12, std to 1e-6, extremes and their ids exactly) -- the wild clips enter nothing but the two
    counters -- and against tests/_eval_ref.py on the restatement's losses of the ordinary clips.  For the second, every ordinary loss
    lies within eps = LOSS_BAR max(|l|, 1) of the restatement's (asserted first), so the mean and the extremes lie within eps and the
    unbiased std within sqrt(n / (n - 1)) eps (the std is 1-Lipschitz in |.|_2 / sqrt(n - 1)); a wild clip that came out finite is a
    legitimate member of the statistics and enters the expectation with the value the kernel gave it."""
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.evaluate import evaluate
    from audio_mps_amd.scan import HipScan
    N, MB = 7, 4
    clips = np.array(W.base_audio(N, T))
    wild = {2: "inf", 5: "click40"}
    ordinary = [i for i in range(N) if i not in wild]
    m = W.base_model(D, MB, backend=HipScan(D))
    ref = W.psi_ref(m, clips)
    assert np.all(np.isfinite(ref))
    for j, kind in wild.items():
        clips[j] = W.wild(kind, clips[j])
    res = evaluate(m, ResidentDataset(clips, m._get_backend(), storage="float32"), MB, keep_losses=True)
    l = res.losses.astype(np.float64)
    fin = np.isfinite(l)
    print(f"evaluate D={D}: losses {res.losses}, n_nonfinite {res.n_nonfinite}, first {res.first_nonfinite}, mean {res.mean:.6f}")
    assert not fin[2]                                                                    # the model diverges on an Inf sample
    assert res.n_clips == N and res.n_nonfinite == int(np.sum(~fin)) and res.first_nonfinite == int(np.flatnonzero(~fin)[0])
    rec = []
    for j, kind in wild.items():                                                         # batches [0..3] and [4..6]: j within its batch
        lo = j // MB * MB
        rec += W.check_mates(res.losses[lo:lo + MB], ref[lo:lo + MB], j - lo, kind)
    assert not W.failures(rec), rec
    # (1) the record against the returned losses, at the bars of tests/test_gpu_evaluate.py
    own = ER.Stats().add(res.losses, 0).record()
    f = l[fin]
    assert res.mean == pytest.approx(f.mean(), rel=1e-12, abs=1e-12) and res.std == pytest.approx(f.std(ddof=1), rel=1e-6)
    assert (res.min, res.max, res.argmin, res.argmax) == (own["min"], own["max"], own["argmin"], own["argmax"])
    # (2) ... and against the restatement's losses of the ordinary clips
    want = ref.astype(np.float64)
    for j in wild:
        want[j] = l[j]
    exp = ER.Stats().add(want.astype(np.float32), 0).record()
    n = exp["n_finite"]
    assert n == int(np.sum(fin)) >= len(ordinary)
    eps = W.LOSS_BAR * max(float(np.max(np.abs(ref[ordinary]))), 1.0)
    ws = want[np.isfinite(want)]
    assert abs(res.mean - exp["sum"] / n) <= eps and abs(res.min - exp["min"]) <= eps and abs(res.max - exp["max"]) <= eps
    assert abs(res.std - ws.std(ddof=1)) <= np.sqrt(n / (n - 1.0)) * eps
    order = np.sort(ws)
    if order[1] - order[0] > 2 * eps:                                                    # the best and worst clips, where eps cannot swap them
        assert res.argmin == exp["argmin"]
    if order[-1] - order[-2] > 2 * eps:
        assert res.argmax == exp["argmax"]
