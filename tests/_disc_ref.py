"""An independent restatement of cmps_bank_classify_weights (include/cmps.h) in numpy: every clip of a [M, B] loss matrix on its own, in
float64 and in member order as the header states it -- the weights, the per-clip objective, the record and the header's rounding bounds."""
import numpy as np

FIELDS = ("sum_xent", "sum_own_loss", "n_used", "n_unlabelled", "n_own_absent")


def clip_terms(col, y, kappa):
    """One used clip: ``col`` float32 [M] with member y present -> (present mask, p [M] float64 with 0 where absent, xent)."""
    present = np.isfinite(col)
    lmin = np.float64(col[present].min())
    e = np.zeros(col.shape[0], np.float64)
    S = 0.0
    for m in np.flatnonzero(present):                                 # the sum in member order
        e[m] = np.exp(-(kappa * (np.float64(col[m]) - lmin)))
        S += e[m]
    return present, e / S, kappa * (np.float64(col[y]) - lmin) + np.log(S)


def weights(loss, labels, inv_temp=1.0, gen_weight=0.0, disc_weight=1.0):
    """``loss`` float32 [M, B], ``labels`` int [B] -> {"w": float32 [M, B], "w64": the same before the rounding to float32, "xent" and
    "own" float64 [B] (NaN for a skipped clip), "state" int [B]: 0 used, 1 unlabelled, 2 own member absent}."""
    x = np.asarray(loss, dtype=np.float32)
    assert x.ndim == 2
    M, B = x.shape
    lab = np.asarray(labels, dtype=np.int64)
    assert lab.shape == (B,)
    kappa, alpha, beta = float(inv_temp), float(gen_weight), float(disc_weight)
    w64 = np.zeros((M, B), np.float64)
    xent, own, state = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, np.int64)
    for b in range(B):
        y = lab[b]
        if y < 0 or y >= M:
            state[b] = 1
            continue
        if not np.isfinite(x[y, b]):
            state[b] = 2
            continue
        present, p, xent[b] = clip_terms(x[:, b], y, kappa)
        own[b] = np.float64(x[y, b])
        delta = (np.arange(M) == y).astype(np.float64)
        w64[present, b] = (alpha * delta + (beta * kappa) * (delta - p))[present]
    return {"w": (w64 + 0.0).astype(np.float32), "w64": w64, "xent": xent, "own": own, "state": state}


def objective(loss64, labels, inv_temp=1.0, gen_weight=0.0, disc_weight=1.0):
    """sum_b J_b = sum over the used clips of gen_weight * l_y + disc_weight * xent_b for float64 losses [M, B] (NaN / Inf: absent): what the
    weights are the partial derivatives of."""
    x = np.asarray(loss64, dtype=np.float64)
    M, B = x.shape
    total = 0.0
    for b in range(B):
        y = int(labels[b])
        if y < 0 or y >= M or not np.isfinite(x[y, b]):
            continue
        col = x[:, b]
        present = np.isfinite(col)
        lmin = col[present].min()
        S = np.sum(np.exp(-(inv_temp * (col[present] - lmin))))
        total += gen_weight * col[y] + disc_weight * (inv_temp * (col[y] - lmin) + np.log(S))
    return total


def record(parts):
    """The record after the calls ``parts`` (the dicts ``weights`` returned, in order, since the last reset)."""
    xent = np.concatenate([p["xent"] for p in parts])
    own = np.concatenate([p["own"] for p in parts])
    state = np.concatenate([p["state"] for p in parts])
    used = state == 0
    return {"sum_xent": float(np.sum(xent[used])), "sum_own_loss": float(np.sum(own[used])), "n_used": int(used.sum()),
            "n_unlabelled": int((state == 1).sum()), "n_own_absent": int((state == 2).sum())}


def weight_bound(w_exact, M, inv_temp, gen_weight, disc_weight):
    """The ROUNDING paragraph of cmps_bank_classify_weights: |w - exact| <= 2^-24 |exact| + 2^-52 (alpha + beta kappa) (M + 16) + 2^-149."""
    return 2.0 ** -24 * np.abs(w_exact) + 2.0 ** -52 * (gen_weight + disc_weight * inv_temp) * (M + 16) + 2.0 ** -149


def record_bounds(rec, M, inv_temp, L, sum_abs_own):
    """(bar of sum_xent, bar of sum_own_loss) of the same paragraph; L the largest |present loss| fed."""
    return (2.0 ** -52 * rec["n_used"] * (M + 32 + 2 * inv_temp * L + rec["sum_xent"]), 2.0 ** -53 * rec["n_used"] * sum_abs_own)
