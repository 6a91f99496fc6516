"""The input of a training step produced on the device (``--device_data``): the batch no longer comes from the host every step.

  ResidentDataset    a TFRecord dataset uploaded ONCE, [N, L] float32 (or, for 16-bit PCM data, int16: storage=) in device memory; every
                     batch is then a row gather
                     (HipScan.gather_batch, cmps_batch_gather) driven by an index plan.  The plan is the reference's pipeline
                     (data.py:37-40 batch -> shuffle(24) -> repeat; training_estimators.py:92 shuffle(24) -> repeat -> batch) run on
                     clip INDICES: tfrecord._shuffle draws from its Generator by the buffer's length alone, so fed indices and the
                     same seed it emits the positions of exactly the clips tfrecord.audio_batches emits -- the k-th batch holds the
                     same bits.  A plan is uploaded an epoch at a time as one int32 tensor and sliced per step.
  ClassBatches       a labelled ResidentDataset (labels=, from_tfrecord(label_key=)) read as one stream per class, the reference's
                     per-pitch input (reader.py:22-40), for a bank of one model per class: [M, B, T] per step from ONE gather of M B rows.
  LabelledBatches    the batches of a plain BatchStream over a labelled ResidentDataset together with the labels of exactly their rows
                     (BatchStream.last_index): the ONE shared batch of a class bank trained as a classifier.
  DampedSineSource   the reference's synthetic batch (data.py:8-22) generated where it is used (HipScan.damped_sine,
                     cmps_damped_sine_fill): clip c of the run is a pure function of (seed, c, T, delta_t).

Both need a backend that has the two methods; one without them (the stand-ins of the host tests) is a ValueError, as with draw_noise.
"""
from __future__ import annotations

import threading
import time
from typing import Optional, Tuple

import numpy as np
import torch

from . import tfrecord

UPLOAD_CLIPS_BYTES = 64 << 20          # from_tfrecord: host clips are uploaded in chunks of about this many bytes


def _need(backend, method: str, what: str):
    if not hasattr(backend, method):
        raise ValueError(f"--device_data ({what}) needs a backend that produces the batch on the device ({method}): "
                         f"{type(backend).__name__} has none")


def _device(backend):
    dev = getattr(backend, "device", None)
    return dev if dev is not None else torch.device("cpu")


PCM_SCALE = 2.0 ** -15                 # int16 storage: sample = i * 2^-15, the float32 value of 16-bit PCM (x = i / 32768)
STORAGES = ("float32", "int16", "auto")


def _as_pcm16(t: torch.Tensor):
    """``t`` float32 [n, L] -> (int16 tensor i with float32(i) * 2^-15 equal to ``t`` BIT FOR BIT, None), or (None, flat position of the
    first sample no i in [-32768, 32767] reproduces): a sample off the grid, one outside [-1, 1 - 2^-15], a NaN -- or a -0.0, which would
    come back as +0.0."""
    i = torch.nan_to_num(t * 32768.0, nan=0.0, posinf=32767.0, neginf=-32768.0).clamp_(-32768.0, 32767.0).to(torch.int16)
    bad = (i.to(torch.float32) * PCM_SCALE).view(torch.int32) != t.view(torch.int32)
    if bool(bad.any()):
        return None, int(torch.nonzero(bad.reshape(-1))[0])
    return i, None


def _not_pcm16(first_clip: int, flat: int, L: int, value) -> ValueError:
    return ValueError(f"storage='int16' needs every sample to equal i * 2^-15 bit for bit with i in [-32768, 32767]: clip "
                      f"{first_clip + flat // L}, sample {flat % L} holds {float(value)!r}")


class ResidentDataset:
    """``clips`` [N, L] float32 (host array or tensor) held on the backend's device.  ``storage``: "float32" (the default) holds them as
    they are; "int16" holds 16-bit PCM data as int16, half the memory, widened by the gather (cmps_batch_gather_i16) without changing a bit
    of any batch -- allowed only where i * 2^-15 reproduces every sample bit for bit, else a ValueError naming the first offending clip and
    sample; "auto" takes int16 where that holds and float32 otherwise.  (An int16 tensor is taken as PCM as it is.)"""

    def __init__(self, clips, backend, storage: str = "float32", labels=None):
        _need(backend, "gather_batch", "ResidentDataset")
        if storage not in STORAGES:
            raise ValueError(f"storage must be one of {STORAGES}, not {storage!r}")
        self.backend = backend
        t = clips if isinstance(clips, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(clips, dtype=None if np.asarray(clips).dtype == np.int16 else np.float32))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("ResidentDataset needs clips [N, L] with N >= 1 and L >= 1")
        if t.dtype == torch.int16:
            if storage == "float32":
                t = t.to(torch.float32) * PCM_SCALE
        else:
            t = t.to(dtype=torch.float32)
            if storage != "float32":
                i, bad = _as_pcm16(t.contiguous())
                if i is None and storage == "int16":
                    raise _not_pcm16(0, bad, int(t.shape[1]), t.reshape(-1)[bad])
                t = t if i is None else i
        self.clips = t.to(device=_device(backend)).contiguous()
        self.labels = None             # with labels: a host array [n_clips], int64 or object (str), one label per clip
        if labels is not None:
            lab = np.asarray(labels)
            lab = lab.astype(np.int64) if lab.dtype.kind in "iu" else np.array([str(x) for x in lab.reshape(-1)], dtype=object).reshape(lab.shape)
            if lab.shape != (int(t.shape[0]),):
                raise ValueError(f"labels must hold one label per clip ([{int(t.shape[0])}]), not {lab.shape}")
            self.labels = lab

    @property
    def n_clips(self) -> int:
        return int(self.clips.shape[0])

    @property
    def clip_len(self) -> int:
        return int(self.clips.shape[1])

    @property
    def storage(self) -> str:
        """"int16" or "float32": how the clips are held."""
        return "int16" if self.clips.dtype == torch.int16 else "float32"

    @property
    def nbytes(self) -> int:
        """Device memory the clips occupy."""
        return int(self.clips.numel() * self.clips.element_size())

    def gather(self, index: torch.Tensor, offset: Optional[torch.Tensor] = None, T: Optional[int] = None) -> torch.Tensor:
        """Rows ``index`` (cut at ``offset``, to ``T`` samples) as a float32 batch on the device, from either storage."""
        if self.clips.dtype == torch.int16:
            return self.backend.gather_batch(self.clips, index, offset, T=T, scale=PCM_SCALE)
        return self.backend.gather_batch(self.clips, index, offset, T=T)

    @classmethod
    def from_tfrecord(cls, path: str, sample_duration: int, backend, verify: bool = False, storage: str = "float32",
                      label_key: Optional[str] = None) -> "ResidentDataset":
        """Reads the file once (tfrecord._audio_records: every record's "audio" must hold ``sample_duration`` values) and uploads it in
        chunks; the chunks are joined on the device, so twice the dataset is allocated for a moment at the end.  ``storage`` is decided
        and converted per chunk, on the host, so an int16 dataset is uploaded as int16; the first chunk that fails under "auto" converts
        the chunks already stored back to float32, once.  ``label_key``: also keep every record's label (tfrecord.labelled_records) as
        ``dataset.labels``."""
        _need(backend, "gather_batch", "ResidentDataset")
        if storage not in STORAGES:
            raise ValueError(f"storage must be one of {STORAGES}, not {storage!r}")
        dev = _device(backend)
        L = int(sample_duration)
        per_chunk = max(1, UPLOAD_CLIPS_BYTES // (4 * L))
        chunks, cur = [], []
        state = {"pcm": storage != "float32", "seen": 0}

        def flush():
            if not cur:
                return
            t = torch.from_numpy(np.stack(cur))
            if state["pcm"]:
                i, bad = _as_pcm16(t)
                if i is None and storage == "int16":
                    raise _not_pcm16(state["seen"], bad, L, t.reshape(-1)[bad])
                if i is None:                                   # "auto": float32 from here on, and for what is already there
                    state["pcm"] = False
                    chunks[:] = [c.to(torch.float32) * PCM_SCALE for c in chunks]
                else:
                    t = i
            chunks.append(t.to(dev))
            state["seen"] += len(cur)
            cur.clear()
        labels = None if label_key is None else []
        records = tfrecord._audio_records(path, L, verify) if label_key is None else tfrecord.labelled_records(path, L, label_key, verify)
        for a in records:
            if labels is not None:
                a, label = a
                labels.append(label)
            cur.append(a)
            if len(cur) == per_chunk:
                flush()
        flush()
        if not chunks:
            raise ValueError(f"{path}: no records")
        return cls(chunks[0] if len(chunks) == 1 else torch.cat(chunks), backend, storage="int16" if state["pcm"] else "float32",
                   labels=labels)

    def ordered(self, minibatch_size: int, T: Optional[int] = None):
        """Every clip once, in file order: yields (first_id, batch [B, T] on the device) with B = ``minibatch_size`` but for the short last
        batch, which is kept.  ``T < L`` takes the first T samples of every clip.  The plan (the clip numbers) is uploaded once."""
        mb, N, L = int(minibatch_size), self.n_clips, self.clip_len
        if mb < 1:
            raise ValueError("ordered needs minibatch_size >= 1")
        T = L if T is None else int(T)
        if not 1 <= T <= L:
            raise ValueError(f"T must lie in [1, {L}] (the clips' length), not {T}")
        plan = torch.arange(N, dtype=torch.int32).to(self.clips.device)
        for first in range(0, N, mb):
            yield first, self.gather(plan[first:first + mb], None, T)

    def class_positions(self, classes) -> np.ndarray:
        """Host int32 [n_clips]: each clip's position in ``classes``, -1 where its label is not among them."""
        if self.labels is None:
            raise ValueError("the dataset holds no labels (ResidentDataset(..., labels=) or from_tfrecord(..., label_key=))")
        classes = list(classes)
        if len(set(classes)) != len(classes):
            raise ValueError(f"classes must be distinct: {classes}")
        where = {(int(c) if self.labels.dtype != object else str(c)): m for m, c in enumerate(classes)}
        return np.array([where.get(int(x) if self.labels.dtype != object else x, -1) for x in self.labels], dtype=np.int32)

    def class_index(self, classes) -> torch.Tensor:
        """``class_positions`` on the device: what cmps_bank_classify_stats reads as a clip's label."""
        return torch.from_numpy(self.class_positions(classes)).to(self.clips.device)

    def class_batches(self, classes, minibatch_size: int, seed: int = 0, shuffle_buffer: int = 24, crop: Optional[int] = None) -> "ClassBatches":
        """A callable returning the next [M, B, T] batch, one [B, T] batch per class of ``classes``, forever (see ClassBatches)."""
        return ClassBatches(self, classes, minibatch_size, seed, shuffle_buffer, crop)

    def batches(self, minibatch_size: int, seed: int = 0, order: str = "data", shuffle_buffer: int = 24, crop: Optional[int] = None,
                crop_seed: int = 0) -> "BatchStream":
        """A callable returning the next batch as a device tensor, forever (see BatchStream).
        order="data":       batch -> shuffle(shuffle_buffer) -> repeat   (over BATCHES; the short last batch of an epoch is kept)
        order="estimator":  shuffle(shuffle_buffer) -> repeat -> batch
        ``crop=T < L``: every clip of every batch is cut to T samples from a random start in [0, L - T], drawn from a Generator of its own
        (``crop_seed``), so the order is the one without crops.  The reference has no crops."""
        return BatchStream(self, minibatch_size, seed, order, shuffle_buffer, crop, crop_seed)

    def labelled_batches(self, classes, minibatch_size: int, seed: int = 0, order: str = "data", shuffle_buffer: int = 24,
                         crop: Optional[int] = None, crop_seed: int = 0) -> "LabelledBatches":
        """A callable returning the next (batch [B, T], labels [B] int32 on the device), forever: the batches of ``batches(...)`` with the
        same arguments, bit for bit, and of exactly those rows ``class_index(classes)`` -- the shared batch of a class bank trained as a
        classifier (BankTrainer.step_classifier)."""
        return LabelledBatches(self, classes, self.batches(minibatch_size, seed, order, shuffle_buffer, crop, crop_seed))


class BatchStream:
    """``stream()`` -> the next batch [B, T] on the device; ``stream(shard=(start, count))`` -> rows start .. start + count - 1 of that
    batch (cut to its size) and nothing else gathered; ``stream.next_size`` is the size of the batch the next call returns (a rank needs
    it to pick its shard of a short batch)."""

    takes_shard = True             # (training_estimators.Estimator.train: hand this callable the rank's shard instead of slicing its result)

    def __init__(self, dataset: ResidentDataset, minibatch_size: int, seed: int, order: str, shuffle_buffer: int, crop: Optional[int],
                 crop_seed: int):
        if order not in ("data", "estimator"):
            raise ValueError(f"order must be 'data' or 'estimator', not {order!r}")
        if int(minibatch_size) < 1 or int(shuffle_buffer) < 1:
            raise ValueError("batches needs minibatch_size >= 1 and shuffle_buffer >= 1")
        self.ds, self.mb, self.order, self.buffer = dataset, int(minibatch_size), order, int(shuffle_buffer)
        L = dataset.clip_len
        if crop is not None and not 1 <= int(crop) <= L:
            raise ValueError(f"crop must lie in [1, {L}] (the clips' length), not {crop}")
        self.T = L if crop is None else int(crop)
        self._crop = crop is not None and self.T < L
        self._rng = np.random.default_rng(seed)
        self._crop_rng = np.random.default_rng(crop_seed)
        self._plan = None              # int32 device tensor [2 if crops else 1, n]: the indices (and offsets) of the clips still to come
        self._pos = 0                  # clips of _plan already handed out
        self._sizes = []               # order="data": sizes of the planned batches still to come
        self.last_index = None         # int32 device tensor: the dataset rows of the batch (or shard) the last call returned

    # -- planning (host; one upload per epoch) ----------------------------------------------------
    def _plan_epoch(self, N: int) -> np.ndarray:
        """One more epoch over clips 0 .. N - 1, on the host: int32 [2 if crops else 1, n] -- the clip of every row to come, in order, and
        its crop offset.  Draws from the stream's two Generators, so successive calls continue the sequence."""
        if self.order == "data":
            rows = [list(range(i, min(i + self.mb, N))) for i in range(0, N, self.mb)]
            rows = list(tfrecord._shuffle(iter(rows), self.buffer, self._rng))
            self._sizes += [len(r) for r in rows]
            idx = np.array([i for r in rows for i in r], dtype=np.int32)
        else:
            idx = np.array(list(tfrecord._shuffle(iter(range(N)), self.buffer, self._rng)), dtype=np.int32)
        plan = idx[None, :]
        if self._crop:
            off = self._crop_rng.integers(0, self.ds.clip_len - self.T + 1, size=idx.size).astype(np.int32)
            plan = np.stack([idx, off])
        return plan

    def _epoch(self):
        """Plan one more epoch and append it to what is left of the current plan."""
        plan = self._plan_epoch(self.ds.n_clips)
        new = torch.from_numpy(np.ascontiguousarray(plan)).to(self.ds.clips.device)
        left = None if self._plan is None else self._plan[:, self._pos:]
        self._plan = new if left is None or left.shape[1] == 0 else torch.cat([left, new], dim=1)     # (joined on the device)
        self._pos = 0

    def _planned(self) -> int:
        return 0 if self._plan is None else int(self._plan.shape[1]) - self._pos

    @property
    def next_size(self) -> int:
        if self.order == "estimator":
            return self.mb
        if not self._sizes:
            self._epoch()
        return self._sizes[0]

    def __call__(self, shard: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        n = self.next_size
        while self._planned() < n:
            self._epoch()
        if self.order == "data":
            self._sizes.pop(0)
        lo, hi = (0, n) if shard is None else (min(max(int(shard[0]), 0), n), min(max(int(shard[0]), 0) + max(int(shard[1]), 0), n))
        at = self._pos
        self._pos += n
        self.last_index = self._plan[0, at + lo:at + hi]       # (a view of the plan: nothing is drawn or copied for it)
        if hi <= lo:
            return torch.empty((0, self.T), dtype=torch.float32, device=self.ds.clips.device)
        index = self.last_index
        offset = self._plan[1, at + lo:at + hi] if self._crop else None
        return self.ds.gather(index, offset, self.T)


class LabelledBatches:
    """``stream()`` -> (the next batch of ``stream``, a BatchStream, and its rows' positions in ``classes``: int32 [B] on the device, -1
    for a label that is not among them).  The labels are uploaded once; a step is the stream's gather and one index_select."""

    def __init__(self, dataset: ResidentDataset, classes, stream: BatchStream):
        self.ds, self.classes, self.stream = dataset, list(classes), stream
        self.labels = dataset.class_index(self.classes)
        self.T = stream.T

    @property
    def next_size(self) -> int:
        return self.stream.next_size

    def __call__(self):
        batch = self.stream()
        return batch, self.labels.index_select(0, self.stream.last_index.to(torch.int64))


class _ClassPlanner(BatchStream):
    """The plan of ONE class of a ClassBatches, kept on the host: BatchStream's own epochs (order="estimator") over the class's clips
    0 .. n - 1, translated to their positions ``ids`` in the whole dataset.  Never gathers."""

    def __init__(self, dataset: ResidentDataset, ids: np.ndarray, minibatch_size: int, seed: int, shuffle_buffer: int, crop: Optional[int]):
        super().__init__(dataset, minibatch_size, seed, "estimator", shuffle_buffer, crop, seed)
        self.ids = np.asarray(ids, dtype=np.int32)
        self._host = np.zeros((2 if self._crop else 1, 0), dtype=np.int32)

    def take(self, n: int) -> np.ndarray:
        """The next ``n`` rows of the class's stream: int32 [2 if crops else 1, n] (dataset clip, crop offset)."""
        while self._host.shape[1] < n:
            plan = self._plan_epoch(int(self.ids.size)).copy()
            plan[0] = self.ids[plan[0]]
            self._host = np.concatenate([self._host, plan], axis=1)
        out, self._host = self._host[:, :n], self._host[:, n:]
        return out


class ClassBatches:
    """``stream()`` -> the next [M, B, T] batch on the device, one [B, T] batch per class of ``classes``: the reference's per-pitch input
    (reader.py:22-40: filter -> shuffle -> repeat -> batch) for every class at once.  Member m's k-th batch is bit for bit the k-th batch of
    ``ResidentDataset(clips[ids_m]).batches(B, seed=seed + m, order="estimator", shuffle_buffer=..., crop=..., crop_seed=seed + m)`` with
    ids_m the clips of class m in file order -- the order in which a class smaller than B still gives full batches.  One step is ONE
    gather of M B rows out of the whole dataset; the rows (and crop offsets) of ``PLAN_STEPS`` steps are planned on the host, one planner
    per class because the classes run out of epoch at different steps, and uploaded as one block, so most steps copy nothing to the device."""

    PLAN_STEPS = 256

    def __init__(self, dataset: ResidentDataset, classes, minibatch_size: int, seed: int = 0, shuffle_buffer: int = 24,
                 crop: Optional[int] = None):
        if dataset.labels is None:
            raise ValueError("class_batches needs a dataset with labels (ResidentDataset(..., labels=) or from_tfrecord(..., label_key=))")
        self.ds, self.classes, self.mb = dataset, list(classes), int(minibatch_size)
        if not self.classes:
            raise ValueError("class_batches needs at least one class")
        index = dataset.class_positions(self.classes)
        self.planners = []
        for m, c in enumerate(self.classes):
            ids = np.flatnonzero(index == m)
            if ids.size == 0:
                raise ValueError(f"class_batches: class {c!r} has no clip in the dataset")
            self.planners.append(_ClassPlanner(dataset, ids, self.mb, int(seed) + m, shuffle_buffer, crop))
        self.T, self._crop = self.planners[0].T, self.planners[0]._crop
        self._block = None             # int32 device tensor [2 if crops else 1, steps, M * B]: the rows of the steps still to come
        self._at = 0                   # steps of _block already handed out
        self.uploads = 0               # blocks uploaded so far
        self._ahead = None             # (worker thread, [its block or its exception]): the block behind the current one

    def __len__(self) -> int:
        return len(self.classes)

    def _plan_block(self, steps: int, pause=lambda: None) -> np.ndarray:
        """int32 [2 if crops else 1, steps, M * B]: step k's rows, class after class.  ``pause()`` is called after every class (the
        worker yields the interpreter to the training loop there)."""
        per_class = []                                                                         # each [rows, steps * B]
        for p in self.planners:
            per_class.append(p.take(steps * self.mb))
            pause()
        rows = per_class[0].shape[0]
        return np.ascontiguousarray(np.stack([c.reshape(rows, steps, self.mb) for c in per_class], axis=2).reshape(rows, steps, -1))

    def _plan_ahead(self):
        """Start planning the next block on a worker thread: M B shuffle draws per step are host work of the order of a tenth of a
        training step, done while the device works through the current block.  One worker at a time, joined before its block is used, so
        the planners' Generators are drawn from in the same order as without it."""
        box = []

        def work():
            try:
                box.append(self._plan_block(self.PLAN_STEPS, pause=lambda: time.sleep(0)))
            except BaseException as e:                                                  # re-raised by the caller's thread
                box.append(e)
        worker = threading.Thread(target=work, name="ClassBatches-plan", daemon=True)
        worker.start()
        self._ahead = (worker, box)

    def _next_block(self) -> np.ndarray:
        if self._ahead is None:
            self._plan_ahead()
        worker, box = self._ahead
        worker.join()
        self._ahead = None
        if isinstance(box[0], BaseException):
            raise box[0]
        return box[0]

    def __call__(self) -> torch.Tensor:
        if self._block is None or self._at == self._block.shape[1]:
            self._block = torch.from_numpy(self._next_block()).to(self.ds.clips.device)
            self._at, self.uploads = 0, self.uploads + 1
            self._plan_ahead()
        k, self._at = self._at, self._at + 1
        out = self.ds.gather(self._block[0, k], self._block[1, k] if self._crop else None, self.T)
        return out.view(len(self.classes), self.mb, self.T)


class DampedSineSource:
    """The synthetic damped-sine batch of every step, generated on the device: step k of the run (k = the trainer's global_step, so a
    restored run continues the sequence) holds clips k * minibatch_size .. (k + 1) * minibatch_size - 1 of the seed's sequence."""

    def __init__(self, backend, minibatch_size: int, T: int, delta_t: float, seed: int = 0):
        _need(backend, "damped_sine", "DampedSineSource")
        if int(minibatch_size) < 1 or int(T) < 1:
            raise ValueError("DampedSineSource needs minibatch_size >= 1 and T >= 1")
        self.backend, self.mb, self.T, self.delta_t, self.seed = backend, int(minibatch_size), int(T), float(delta_t), int(seed)

    def next(self, step: int, shard: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """The batch of ``step``, or with ``shard=(start, count)`` rows start .. start + count - 1 of it, without generating the rest."""
        start, count = (0, self.mb) if shard is None else (int(shard[0]), int(shard[1]))
        if count < 1:
            return torch.empty((0, self.T), dtype=torch.float32, device=_device(self.backend))
        return self.backend.damped_sine(self.seed, int(step) * self.mb + start, count, self.T, self.delta_t)
