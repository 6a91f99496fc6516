"""An independent restatement of the evaluation side of include/cmps.h: the record of cmps_loss_stats accumulated exactly (math.fsum over
everything seen so far, ids kept), the int16 gather of cmps_batch_gather_i16 built on tests/_data_ref.gather, and stand-in backend methods
for the host tests (tests/test_eval_host.py) that ARE this reference and count their calls."""
import math

import numpy as np

import _data_ref as DR

FIELDS = ("sum", "sumsq", "n_finite", "n_nonfinite", "argmin", "argmax", "first_nonfinite", "min", "max")


class Stats:
    """Every (id, loss) a record has been fed since its last reset; `record()` is what the 64 bytes must hold."""

    def __init__(self):
        self.ids, self.values = [], []

    def add(self, loss, first_id, reset=False):
        x = np.asarray(loss, dtype=np.float32).reshape(-1)
        if reset:
            self.ids, self.values = [], []
        self.ids.append(np.arange(first_id, first_id + x.size, dtype=np.int64))
        self.values.append(x.copy())
        return self

    def record(self):
        ids, x = np.concatenate(self.ids), np.concatenate(self.values)
        fin = np.isfinite(x)
        xf, idf = x[fin], ids[fin]
        rec = {"sum": math.fsum(float(v) for v in xf), "sumsq": math.fsum(float(v) * float(v) for v in xf),        # (a float32 squared in
               "n_finite": int(fin.sum()), "n_nonfinite": int((~fin).sum()),                                       # double is exact)
               "argmin": -1, "argmax": -1, "first_nonfinite": int(ids[~fin].min()) if (~fin).any() else -1,
               "min": float("inf"), "max": float("-inf"), "abs_sum": math.fsum(abs(float(v)) for v in xf)}
        if xf.size:
            lo, hi = xf.min(), xf.max()
            rec["argmin"], rec["argmax"] = int(idf[xf == lo].min()), int(idf[xf == hi].min())       # the lowest id on ties
            rec["min"], rec["max"] = float(lo), float(hi)
        return rec


def gather_i16(data_i16, index, offset, T, scale):
    """What cmps_batch_gather_i16 defines: the float32 gather of (float32)data * scale -- an exact conversion and one float32 multiply."""
    data = np.asarray(data_i16)
    assert data.dtype == np.int16
    return DR.gather(data.astype(np.float32) * np.float32(scale), index, offset, T)


class EvalMethods:
    """Mixed into a stand-in backend: `loss_stats` / `read_stats` / an int16-aware `gather_batch` from this reference, on host tensors,
    counting what an evaluation may do only once."""

    def _eval_init(self):
        self.stats_calls, self.downloads, self.gathers = [], 0, []

    def loss_stats(self, loss, first_id, stats=None, reset=False):
        x = loss.detach().cpu().numpy()
        self.stats_calls.append((int(first_id), x.size, stats is None or bool(reset)))
        stats = Stats() if stats is None else stats
        return stats.add(x, int(first_id), reset=reset)

    def read_stats(self, stats):
        self.downloads += 1
        rec = stats.record()
        return {k: rec[k] for k in FIELDS}

    def gather_batch(self, data, index, offset=None, T=None, scale=2.0 ** -15):
        import torch
        T = data.shape[1] if T is None else T
        idx, off = index.numpy().copy(), None if offset is None else offset.numpy().copy()
        self.gathers.append((idx, off, T, str(data.dtype)))
        if data.dtype == torch.int16:
            return torch.from_numpy(gather_i16(data.numpy(), idx, off, T, scale))
        assert data.dtype == torch.float32
        return torch.from_numpy(DR.gather(data.numpy(), idx, off, T))
