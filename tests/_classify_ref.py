"""An independent restatement of cmps_bank_classify_stats (include/cmps.h): every clip of a [M, B] loss matrix judged on its own in numpy
-- the sums in extended precision (np.longdouble: a 64-bit significand on x86, 2^-11 of a double's rounding) -- the record those clips
add up to, the rounding bound the header states, and stand-in backend methods for the host tests that ARE this reference."""
import numpy as np

HEAD = ("sum_xent", "sum_margin", "n_decided", "n_undecided", "n_unlabelled", "n_correct", "n_xent", "n_margin", "first_undecided")
LD = np.longdouble


def judge(loss, labels=None):
    """``loss`` float32 [M, B], ``labels`` int [B] or None -> per clip: best (int, -1 undecided), margin and xent (longdouble, NaN where the
    clip has none), label (int, -1 unlabelled)."""
    x = np.asarray(loss, dtype=np.float32)
    assert x.ndim == 2
    M, B = x.shape
    lab = np.full(B, -1, np.int64) if labels is None else np.asarray(labels, dtype=np.int64).copy()
    lab[(lab < 0) | (lab >= M)] = -1
    best = np.full(B, -1, np.int64)
    margin, xent = np.full(B, np.nan, LD), np.full(B, np.nan, LD)
    for b in range(B):
        col = x[:, b]
        present = np.flatnonzero(np.isfinite(col))
        if present.size == 0:
            continue
        vals = col[present]
        lo = vals.min()                                               # float32 compare
        best[b] = present[np.flatnonzero(vals == lo)[0]]              # the lowest m on ties
        if present.size >= 2:
            second = np.sort(vals, kind="stable")[1]
            margin[b] = LD(second) - LD(lo)
        y = lab[b]
        if y >= 0 and np.isfinite(col[y]):
            d = vals.astype(LD) - LD(lo)
            xent[b] = (LD(col[y]) - LD(lo)) + np.log(np.sum(np.exp(-d)))
    return {"best": best, "margin": margin, "xent": xent, "label": lab}


class Record:
    """Every call a record has been fed since its last reset; `record()` is what it must hold (sums exact to 2^-64), `bounds()` the bars
    of the header for exactly those clips."""

    def __init__(self, M):
        self.M, self.parts = int(M), []

    def add(self, loss, labels, first_id, reset=False):
        x = np.asarray(loss, dtype=np.float32)
        assert x.shape[0] == self.M
        if reset:
            self.parts = []
        j = judge(x, labels)
        j["ids"] = np.arange(first_id, first_id + x.shape[1], dtype=np.int64)
        fin = x[np.isfinite(x)]
        j["L"] = float(np.abs(fin).max()) if fin.size else 0.0
        self.parts.append(j)
        return self

    def _all(self, key):
        return np.concatenate([p[key] for p in self.parts])

    def record(self):
        M = self.M
        best, lab, margin, xent, ids = (self._all(k) for k in ("best", "label", "margin", "xent", "ids"))
        decided, labelled = best >= 0, lab >= 0
        conf, unl = np.zeros((M, M), np.int64), np.zeros(M, np.int64)
        np.add.at(conf, (lab[decided & labelled], best[decided & labelled]), 1)
        np.add.at(unl, best[decided & ~labelled], 1)
        has_x, has_m = ~np.isnan(xent), ~np.isnan(margin)
        return {"sum_xent": float(np.sum(np.sort(xent[has_x]))), "sum_margin": float(np.sum(np.sort(margin[has_m]))),
                "n_decided": int(decided.sum()), "n_undecided": int((~decided).sum()), "n_unlabelled": int((decided & ~labelled).sum()),
                "n_correct": int((decided & labelled & (best == lab)).sum()), "n_xent": int(has_x.sum()), "n_margin": int(has_m.sum()),
                "first_undecided": int(ids[~decided].min()) if (~decided).any() else -1,
                "confusion": conf, "unlabelled_best": unl, "best": best.astype(np.int32)}

    def bounds(self):
        """(bar of sum_xent, bar of sum_margin), the ROUNDING paragraph of cmps_bank_classify_stats:
        2^-52 n_xent (M + 40 + 2 L + sum xent)  and  2^-52 n_margin (sum margin), L the largest |finite loss| fed."""
        rec = self.record()
        L = max(p["L"] for p in self.parts)
        return (2.0 ** -52 * rec["n_xent"] * (self.M + 40 + 2 * L + rec["sum_xent"]), 2.0 ** -52 * rec["n_margin"] * rec["sum_margin"])


class ClassifyMethods:
    """Mixed into a stand-in backend: `classify_stats` / `read_classify_stats` from this reference on host tensors, counting what an
    evaluation may do only once."""

    def _classify_init(self):
        self.classify_calls, self.classify_downloads = [], 0

    def classify_stats(self, loss, labels, first_id, stats=None, reset=False, best=None):
        x = loss.detach().cpu().numpy()
        self.classify_calls.append((int(first_id), tuple(x.shape), stats is None or bool(reset)))
        stats = Record(x.shape[0]) if stats is None else stats
        stats.add(x, None if labels is None else labels.numpy(), int(first_id), reset=reset)
        if best is not None:
            import torch
            best.copy_(torch.from_numpy(stats.parts[-1]["best"].astype(np.int32)))
        return stats

    def read_classify_stats(self, stats, M):
        self.classify_downloads += 1
        assert stats.M == M
        rec = stats.record()
        rec.pop("best")
        return rec
