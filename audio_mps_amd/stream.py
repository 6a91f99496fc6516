"""A resumable sampler for PsiCMPS and RhoCMPS: follow and score an incoming signal and generate audio in segments (cmps_psi_stream,
cmps_psi_stream_score, cmps_rho_stream, cmps_rho_stream_score).

The reference samples a whole waveform in one tf.scan (model.py:242-251) and has nothing that carries on.  A ``SampleStream`` keeps what
the sampler kernel carries between two steps on the device, so a scan can be continued, can alternate between teacher-forced blocks
(``follow``) and sampled ones (``generate``), and can follow only.  Cutting a run into segments changes no bit of it.  A stream opened
with ``device_noise=True`` draws the noise of a generated step on the device, as a function of (seed, path, position) alone
(cmps_noise_fill), instead of on the host.

    st = model.open_stream(num_paths=4, max_steps=3 * 16000, seed=0)
    pred = st.follow(block)             # [4, steps]: the model's expected increment before every followed sample
    nll = st.score(block2)              # [4, steps]: follow, and how likely every sample was; st.total_nll sums them
    wave = st.generate(16000)           # [4, 16000] in the clip's own units, continuing the followed signal
    wave2 = st.generate(16000)          # ... and on from there

A RhoCMPS stream opened with ``keep_states=S`` also returns rho and the purity after every step of the last call (``st.states()``,
``st.purity()``), from a stash that holds S steps however long the run is -- behind a ``score`` call as behind a ``follow``.

A ``BankStream`` (``PsiBank.open_stream`` / ``RhoBank.open_stream``; cmps_bank_stream, cmps_bank_stream_score, cmps_rho_bank_stream,
cmps_rho_bank_stream_score) is the same stream for every member of a bank at once: results [M, num_paths, steps], ``total_nll``
[M, num_paths], ``ranking()`` and ``best()`` -- M models along one signal.  ``score_posterior`` (cmps_bank_posterior) is ``score`` judged as a
classifier after every sample: the most probable member and its probability per step, and the step at which the bank was first sure.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .prior import log_prior_of


def segments(N: int, S: Optional[int] = None) -> list:
    """The column slices (lo, hi) of a clip of ``N`` steps ([n, N + 1]) followed in segments of ``S`` steps (None: whole): the anchor and S
    steps, (0, S + 1), then S steps at a time, (a, a + S) for a = S + 1, 2 S + 1, ... <= N.  The last slice may reach past the clip.
    A list, built at once, so that a caller who cuts before it opens its stream has a bad ``S`` refused before anything is opened."""
    S = int(N) if S is None else int(S)
    if S < 1:
        raise ValueError("segment must be positive")
    return [(0, S + 1)] + [(a, a + S) for a in range(S + 1, int(N) + 1, S)]


def as_clips(clips, who: str) -> np.ndarray:
    """``clips`` ([T'] or [n, T']; a torch tensor or an array) as a stream follows them: contiguous float32 [n, T'] with T' >= 2."""
    if hasattr(clips, "detach"):
        clips = clips.detach().cpu().numpy()
    clips = np.asarray(clips, dtype=np.float32)
    if clips.ndim == 1:
        clips = clips[None, :]
    if clips.ndim != 2 or clips.shape[1] < 2:
        raise ValueError(f"{who}: need [T'] or [n, T'] with two samples at least (one increment), not {clips.shape}")
    return np.ascontiguousarray(clips)


class SampleStream:
    """Returned by ``PsiCMPS.open_stream`` / ``RhoCMPS.open_stream``.  ``position`` is the number of steps taken (the next table row), ``max_steps`` the number the
    stream was sized for, ``last`` the last sample per path [num_paths] (None while the stream has seen no audio and generated nothing)."""

    def __init__(self, model, num_paths: int, max_steps: int, temp=1, seed=None, keep_states: int = 0, device_noise: bool = False):
        if num_paths < 1 or max_steps < 1:
            raise ValueError("open_stream needs num_paths >= 1 and max_steps >= 1")
        self.num_paths, self.max_steps, self.keep_states = int(num_paths), int(max_steps), int(keep_states)
        self._saved = None             # steps of the last call whose columns the backend kept (keep_states)
        self.position = 0
        self.last = None
        self._shape = self._path_shape(model)   # of everything the stream keeps per path: (num_paths,); a BankStream: (M, num_paths)
        self._A = self._scale(model)
        self._std = float(model.sigma) * math.sqrt(temp * float(model.delta_t))      # CMPS._noise
        self.device_noise = bool(device_noise)
        self.noise_seed = None         # device noise: the seed every generated step's noise is a function of, with its path and position
        if self.device_noise:
            model._device_noise_backend()                                            # (ValueError before anything runs)
            self.noise_seed = model._noise_seed(seed)
        self._rng = np.random.default_rng(seed)
        self._be = model._prepare_stream(self.num_paths, self.max_steps, self.keep_states)   # T = max_steps + 1: one table row per step
        new_state, self._segment = model._stream_entries(self._be)
        self._state = new_state(self.num_paths)
        self._level = None             # inside a sampled run: the level it began at
        self._raw = None               # the last generate call as the entry returned it (PsiBank.sample)
        self._model = model
        self.total_nll = np.zeros(self._shape, dtype=np.float32)      # the fold carry of the scored steps so far (model.py:279)
        self.last_pred = None          # the predictions of the last score call

    def _path_shape(self, model):
        return (self.num_paths,)

    def _scale(self, model):
        """model.A as the waveforms are divided by it"""
        return np.float32(model.A)

    # ------------------------------------------------------------------
    def _launch(self, steps, entry, *args, **kw):
        """One call of ``steps`` steps through ``entry`` (the stream's segment entry, or `score`'s): the bounds first -- a refused call
        changes nothing -- then the entry on the stream's state and position, then the bookkeeping."""
        if self.position + steps > self.max_steps:
            raise ValueError(f"the stream was opened for max_steps={self.max_steps}: {self.position} taken, {steps} more asked for")
        if self.keep_states and steps > self.keep_states:
            raise ValueError(f"the stream was opened with keep_states={self.keep_states}: a call of {steps} steps does not fit")
        if self.keep_states:
            kw["save_states"] = True
        res = entry(self._state if self.position else None, self._state, self.position, *args, n=self.num_paths, **kw)
        self.position += steps
        self._saved = steps if self.keep_states else None
        return res

    def _kept(self, want_rho):
        if not self.keep_states:
            raise ValueError("states() / purity() need a RhoCMPS stream opened with keep_states")
        if not self._saved:
            raise ValueError("states() / purity() return the steps of the last follow / generate call: none has made a step yet")
        return self._be.rho_states(self.num_paths, self._saved, want_rho=want_rho, want_purity=not want_rho)

    def states(self) -> np.ndarray:
        """Lab-frame rho after every step of the last follow / score / generate call, [num_paths, steps, D, D] (keep_states streams)."""
        return self._kept(True)

    def purity(self) -> np.ndarray:
        """tr rho^2 after every step of the last follow / score / generate call, [num_paths, steps] (keep_states streams)."""
        return self._kept(False)

    def _block(self, block) -> np.ndarray:
        if hasattr(block, "detach"):
            block = block.detach().cpu().numpy()
        block = np.asarray(block, dtype=np.float32)
        if block.ndim == 1:
            block = block[None, :]
        if block.ndim != 2 or block.shape[0] not in (1, self.num_paths) or block.shape[1] < 1:
            raise ValueError(f"a block must be [m], [1, m] or [{self.num_paths}, m] with m >= 1, not {block.shape}")
        return block

    def _anchored(self, block, anchor):
        """(block, the audio of a forced call [n_audio, steps + 1]): the block behind the sample it continues from, follow's rule."""
        block = self._block(block)
        if anchor or self.last is None:
            audio = block
        else:
            audio = self._behind_last(block)
        return block, audio

    def _behind_last(self, block):
        """The block behind the stream's last samples: shared by every path while they are all equal, else one row per path."""
        if block.shape[0] == 1 and np.all(self.last == self.last[0]):
            return np.concatenate([self.last[:1, None], block], axis=1)
        return np.concatenate([self.last[:, None], np.broadcast_to(block, (self.num_paths, block.shape[1]))], axis=1)

    def _rows(self, audio):
        """A forced call's audio as the entry takes it: [n_audio, steps + 1]."""
        return np.ascontiguousarray(audio)

    def score(self, block, anchor: bool = False) -> np.ndarray:
        """``follow`` that also says how likely the block was (cmps_psi_stream_score / cmps_rho_stream_score): same arguments, anchoring
        rule and bookkeeping, returns the negative log-likelihood of every step, [num_paths, steps] = -log(1 + e' x / A) of
        model.py:293-294 (RhoCMPS: :166, 169-170),
        and adds them to ``total_nll`` [num_paths] in step order (the fold carry of model.py:279; over a whole clip from a fresh
        stream: ``loss_per_clip``).  The predictions ``follow`` would have returned are in ``last_pred``.  Scoring changes nothing the
        stream carries: ``follow``, ``score`` and ``generate`` alternate freely, and unscored steps leave ``total_nll`` as it is."""
        entry = self._model._stream_score_entry(self._be)
        block, audio = self._anchored(block, anchor)
        steps = audio.shape[-1] - 1
        nll = np.empty(self._shape + (0,), dtype=np.float32)
        pred = np.empty(self._shape + (0,), dtype=np.float32)
        if steps:
            nll, total, pred = self._launch(steps, entry, self._rows(audio), want_nll=True, want_pred=True, loss=self.total_nll)
            self.total_nll = np.asarray(total, dtype=np.float32)
        self.last_pred = pred
        self.last = np.array(np.broadcast_to(block[..., -1], self._shape), dtype=np.float32)
        self._level = None
        return nll

    def follow(self, block, anchor: bool = False) -> np.ndarray:
        """Teacher-force the stream on ``block`` ([num_paths, m], or [m] / [1, m] for one signal shared by every path; the clip's own
        units).  On a stream that has seen no audio the block's first sample is the anchor X_0 and makes no step; later blocks make one
        step per sample, the first one from the stream's last sample.  ``anchor=True`` re-anchors on ``block[..., 0]`` without a step
        (to resume behind a generated gap without showing the model the jump).  Returns the model's expected increment before every
        step, [num_paths, steps]."""
        block, audio = self._anchored(block, anchor)
        steps = audio.shape[-1] - 1
        pred = np.empty(self._shape + (0,), dtype=np.float32)
        if steps:
            _, pred = self._launch(steps, self._segment, self._rows(audio), None, True)
        self.last = np.array(np.broadcast_to(block[..., -1], self._shape), dtype=np.float32)
        self._level = None
        return pred

    def generate(self, length: int, noise=None) -> np.ndarray:
        """Sample ``length`` steps: [num_paths, length] in the clip's own units = the level when the sampled run began (0 on a fresh
        stream, model.py:244; else the last followed sample) + the running sum of the sampled increments, which the kernel state
        carries, so consecutive calls continue one waveform.  The noise [length, num_paths] comes from the stream's own Generator
        (stddev sigma sqrt(temp delta_t), as CMPS._noise), or is passed in.  A stream opened with ``device_noise=True`` draws it on the
        device instead (cmps_noise_fill): step k of path b gets stddev * z(noise_seed, b, k), a function of the stream's position alone, so
        how a run is cut into calls -- or into processes -- changes no bit of it."""
        length, n = int(length), self._noise_paths()
        if length < 1:
            raise ValueError("generate needs length >= 1")
        if self.position + length > self.max_steps:                  # (before the draw: a refused call leaves the Generator alone)
            raise ValueError(f"the stream was opened for max_steps={self.max_steps}: {self.position} taken, {length} more asked for")
        kw = {}
        if noise is None and self.device_noise:
            from .scan import NoisePlan
            noise, kw = NoisePlan(self.noise_seed, self.position, self._std), {"length": length, **self._plan_kw()}
        else:
            if noise is None:
                noise = (self._std * self._rng.standard_normal((length, n))).astype(np.float32)
            noise = np.asarray(noise, dtype=np.float32)
            if noise.shape != (length, n):
                raise ValueError(f"noise must be [{length}, {n}]")
        if self._level is None:
            self._level = np.zeros(self._shape, dtype=np.float32) if self.last is None else self.last.copy()
        out, _ = self._launch(length, self._segment, None, noise, False, **kw)
        self._raw = out                # A * running sum of the sampled increments: the reference's convention (model.py:251)
        wave = (self._level[..., None] + out / self._A).astype(np.float32)
        self.last = wave[..., -1].copy()
        return wave

    def _noise_paths(self) -> int:
        """Columns of a generate call's noise"""
        return self.num_paths

    def _plan_kw(self) -> dict:
        """What the segment entry needs next to a NoisePlan besides ``length``"""
        return {}

    def fill_gaps(self, clip, known) -> np.ndarray:
        """``clip`` [T] or [num_paths, T] with a boolean mask ``known`` [T]: runs of True are followed, runs of False generated, and each
        known run behind a gap is re-anchored on its first sample.  Returns [num_paths, T]: the clip where it is known, the model's
        waveform in the gaps."""
        clip = self._block(clip)
        known = np.asarray(known, dtype=bool)
        if known.shape != (clip.shape[-1],):
            raise ValueError(f"known must be a boolean mask [{clip.shape[-1]}]")
        T = clip.shape[-1]
        wave = np.array(np.broadcast_to(clip, self._shape + (T,)), dtype=np.float32)
        edges = [0] + [k for k in range(1, T) if known[k] != known[k - 1]] + [T]
        for a, b in zip(edges[:-1], edges[1:]):
            if known[a]:
                self.follow(clip[..., a:b], anchor=a > 0)
            else:
                wave[..., a:b] = self.generate(b - a)
        return wave


class _MemberLoop:
    """The bank entries of HipScan (bank_stream_state, bank_stream, bank_stream_score and their rho_bank_* counterparts) for a backend that
    lacks them: a loop over one plain backend per member, as BankTrainer loops over plain steps.  A state is the list of the members'
    states."""

    def __init__(self, backends):
        self.backends = list(backends)

    def bank_set_params(self, members, B, T, train=False):
        for be, p in zip(self.backends, members):
            be.set_params(p, B, T, train=train)

    def rho_bank_set_state(self, members, columns, B, T, train=False):
        for be, p, phi in zip(self.backends, members, columns):
            be.set_params(p, B, T, train=False)
            be.rho_set_state(phi, B, T, train=train)

    def _member(self, rows, m, n, axis):
        """Member m's rows of an array shared by the members (1 or n rows) or holding M n"""
        if rows is None or rows.shape[axis] in (1, n) and len(self.backends) * n != rows.shape[axis]:
            return rows
        return np.take(rows, range(m * n, (m + 1) * n), axis=axis)

    # one loop per operation; `pre` is "" (PsiCMPS members: stream_state, stream, stream_score) or "rho_"
    def _state(self, pre, n):
        return [getattr(be, pre + "stream_state")(n) for be in self.backends]

    def _stream(self, pre, state_in, state_out, k0, audio, noise, want_pred=False, n=None):
        audio = None if audio is None else np.asarray(audio, dtype=np.float32)
        noise = None if noise is None else np.asarray(noise, dtype=np.float32)
        res = [getattr(be, pre + "stream")(None if state_in is None else state_in[m], None if state_out is None else state_out[m], k0,
                                           self._member(audio, m, n, 0), self._member(noise, m, n, 1), want_pred, n=n)
               for m, be in enumerate(self.backends)]
        return np.stack([r[0] for r in res]), (np.stack([r[1] for r in res]) if want_pred else None)

    def _score(self, pre, state_in, state_out, k0, audio, want_nll=True, want_pred=False, n=None, loss=None):
        audio = np.asarray(audio, dtype=np.float32)
        res = [getattr(be, pre + "stream_score")(None if state_in is None else state_in[m], None if state_out is None else state_out[m], k0,
                                                 self._member(audio, m, n, 0), want_nll, want_pred, n=n, loss=None if loss is None else loss[m])
               for m, be in enumerate(self.backends)]
        pick = lambda i, want: np.stack([r[i] for r in res]) if want else None   # noqa: E731
        return pick(0, want_nll), np.stack([r[1] for r in res]), pick(2, want_pred)

    def bank_stream_state(self, n):
        return self._state("", n)

    def bank_stream(self, *args, **kw):
        return self._stream("", *args, **kw)

    def bank_stream_score(self, *args, **kw):
        return self._score("", *args, **kw)

    def rho_bank_stream_state(self, n):
        return self._state("rho_", n)

    def rho_bank_stream(self, *args, **kw):
        return self._stream("rho_", *args, **kw)

    def rho_bank_stream_score(self, *args, **kw):
        return self._score("rho_", *args, **kw)


class _BankScan:
    """What SampleStream asks of its model, answered by a PsiBank or a RhoBank: the members' effective parameters (RhoBank: and their
    columns of rho_0) as they are when the stream is opened, on a backend of the stream's own."""

    def __init__(self, bank):
        self.members = [m.effective_params() for m in bank.models]
        self.columns = [m.columns() for m in bank.models] if bank.rank else None
        self._pre = "rho_bank_" if bank.rank else "bank_"            # the backend's entries of this kind of bank
        m0 = bank.models[0]
        self.sigma, self.delta_t = m0.sigma, m0.delta_t
        self._noise_seed = m0._noise_seed
        self.backend = bank.stream_backend()
        if not hasattr(self.backend, self._pre + "stream"):
            if bank.rank and not hasattr(self.backend, "rho_stream"):
                raise ValueError(f"open_stream: this backend streams PsiCMPS banks only: {type(self.backend).__name__} has neither "
                                 "rho_bank_stream nor rho_stream (cmps_rho_bank_stream, cmps_rho_stream)")
            self.backend = _MemberLoop([self.backend] + [bank.stream_backend() for _ in self.members[1:]])

    def __len__(self):
        return len(self.members)

    def _device_noise_backend(self):
        if not hasattr(self.backend, "draw_noise"):
            raise ValueError("device_noise=True needs a backend that draws noise on the device (draw_noise): the bank's has none")
        return self.backend

    def _prepare_stream(self, num_paths, max_steps, keep_states=0):
        if self.columns is None:
            self.backend.bank_set_params(self.members, num_paths, max_steps + 1, train=False)
        else:
            self.backend.rho_bank_set_state(self.members, self.columns, num_paths, max_steps + 1, train=False)
        return self.backend

    def _stream_entries(self, be):
        return getattr(be, self._pre + "stream_state"), getattr(be, self._pre + "stream")

    def _stream_score_entry(self, be):
        if self.columns is not None and isinstance(be, _MemberLoop) and not hasattr(be.backends[0], "rho_stream_score"):
            raise ValueError(f"this backend scores PsiCMPS-only streams: {type(be.backends[0]).__name__} has no rho_stream_score "
                             "(cmps_rho_stream_score)")       # (as RhoCMPS._stream_score_entry: said before anything runs)
        return getattr(be, self._pre + "stream_score")

    def _stream_posterior_entry(self, be):
        name = self._pre + "stream_posterior"
        if not hasattr(be, name):
            inner = be.backends[0] if isinstance(be, _MemberLoop) else be
            raise ValueError(f"score_posterior needs a backend that folds the members' losses on the device: {type(inner).__name__} has no "
                             f"{name} (cmps_bank_posterior)")
        return getattr(be, name)


@dataclass
class PosteriorTrace:
    """What ``BankStream.score_posterior`` and ``PsiBank.posterior_trace`` return: per path and scored step the most probable member
    ``best`` [n, steps] (int32, -1 where no member has a finite total) and its posterior probability ``conf`` [n, steps]; on request the
    whole posterior ``post`` [M, n, steps] and the members' ``nll`` [M, n, steps]; ``decided_at`` / ``decided_as`` [n]: the stream position
    of the first step at which ``conf`` reached the threshold and the member it was then, -1 while undecided (or without a threshold)."""
    best: np.ndarray
    conf: np.ndarray
    post: Optional[np.ndarray] = None
    nll: Optional[np.ndarray] = None
    decided_at: Optional[np.ndarray] = None
    decided_as: Optional[np.ndarray] = None


class BankStream(SampleStream):
    """Returned by ``PsiBank.open_stream`` / ``RhoBank.open_stream`` / ``BankTrainer.open_stream``: a SampleStream of every member at once
    (cmps_bank_stream, cmps_bank_stream_score; a RhoBank: cmps_rho_bank_stream, cmps_rho_bank_stream_score).  Everything carries a leading member axis -- results [M, num_paths, steps], ``last`` and ``total_nll``
    [M, num_paths] -- and a block may be [m] / [1, m] (one signal for everybody), [num_paths, m] (shared by the members) or
    [M, num_paths, m].  Member m, path b gets the noise ``member(m).open_stream(num_paths, ..., seed=seed)`` would give path b, so what
    differs between two members' samples is the model and not the draw; ``independent_noise=True`` numbers the paths globally instead
    (g = m num_paths + b).  On a backend without the bank entries the stream loops over plain streams of its members."""

    def __init__(self, bank, num_paths: int, max_steps: int, temp=1, seed=None, device_noise: bool = False, independent_noise: bool = False,
                 prior=None, temperature: float = 1.0, threshold: Optional[float] = None):
        self.independent_noise = bool(independent_noise)
        log_prior = log_prior_of(prior, len(bank), bank.class_counts, "open_stream")
        if not (math.isfinite(temperature) and temperature > 0):
            raise ValueError("open_stream: temperature must be finite and positive")
        if threshold is not None and not 0.0 < float(threshold) <= 1.0:
            raise ValueError("open_stream: threshold must lie in (0, 1]")
        self._pred = None              # last_pred: the host array, or what downloads it when somebody asks
        super().__init__(_BankScan(bank), num_paths, max_steps, temp=temp, seed=seed, device_noise=device_noise)
        self.native = not isinstance(self._be, _MemberLoop)
        self.temperature, self.threshold = float(temperature), None if threshold is None else float(threshold)
        self.log_prior = log_prior     # [M] float64 or None (uniform): what score_posterior weighs the members with
        up = getattr(self._be, "log_prior_tensor", None)
        self._log_prior_be = up(log_prior) if up is not None else log_prior          # (goes up once)
        self._decision = None          # the backend's decision records, carried from one score_posterior call to the next
        self.decided_at = np.full(self.num_paths, -1, dtype=np.int64)                 # the position of the first sure step per path
        self.decided_as = np.full(self.num_paths, -1, dtype=np.int32)                 # ... and the member it was sure of

    def __len__(self) -> int:
        return self._shape[0]

    def _path_shape(self, model):
        return (len(model), self.num_paths)

    def _scale(self, model):
        return np.array([p.A for p in model.members], dtype=np.float32)[:, None, None]

    def _block(self, block) -> np.ndarray:
        if hasattr(block, "detach"):
            block = block.detach().cpu().numpy()
        block = np.asarray(block, dtype=np.float32)
        if block.ndim == 1:
            block = block[None, :]
        M, n = self._shape
        if not (block.ndim == 2 and block.shape[0] in (1, n) or block.shape[:-1] == (M, n)) or block.shape[-1] < 1:
            raise ValueError(f"a block must be [m], [1, m], [{n}, m] or [{M}, {n}, m] with m >= 1, not {block.shape}")
        return block

    def _behind_last(self, block):
        M, n = self._shape
        m = block.shape[-1]
        if block.ndim == 2 and np.all(self.last == self.last[0]):       # the members agree: the audio stays shared between them
            if block.shape[0] == 1 and np.all(self.last[0] == self.last[0, 0]):
                return np.concatenate([self.last[0, :1, None], block], axis=1)
            return np.concatenate([self.last[0][:, None], np.broadcast_to(block, (n, m))], axis=1)
        return np.concatenate([self.last[..., None], np.broadcast_to(block, (M, n, m))], axis=-1)

    def _rows(self, audio):
        return np.ascontiguousarray(audio.reshape(-1, audio.shape[-1]))

    def _noise_paths(self) -> int:
        return self._shape[0] * self.num_paths if self.independent_noise else self.num_paths

    def _plan_kw(self) -> dict:
        return {"n_noise": self._noise_paths()}

    @property
    def last_pred(self):
        """The predictions of the last score / score_posterior call (score_posterior: downloaded when first read)."""
        if callable(self._pred):
            self._pred = self._pred()
        return self._pred

    @last_pred.setter
    def last_pred(self, value):
        self._pred = value

    def score_posterior(self, block, anchor: bool = False, want_post: bool = False, want_nll: bool = False) -> PosteriorTrace:
        """``score`` judged as a classifier after every sample (cmps_bank_stream_score / cmps_rho_bank_stream_score, then
        cmps_bank_posterior on the losses where they lie): same arguments, anchoring rule and bookkeeping -- state, ``position``,
        ``last``, ``last_pred`` and ``total_nll`` end up as ``score`` leaves them, bit for bit -- but what comes back is a PosteriorTrace:
        per path and step the member that is the most probable given everything scored so far, and its probability, under the stream's
        ``prior`` and ``temperature`` (p_m proportional to prior_m exp(-total_nll_m / temperature)).  A stream opened with a ``threshold``
        also keeps, across calls, the position of the first step at which that probability reached it (``decided_at`` [num_paths], -1
        while undecided) and the member it was (``decided_as``).  The members' per-step losses stay on the device unless ``want_nll``."""
        entry = self._model._stream_posterior_entry(self._be)
        block, audio = self._anchored(block, anchor)
        steps = audio.shape[-1] - 1
        M, n = self._shape
        trace = PosteriorTrace(np.empty((n, 0), np.int32), np.empty((n, 0), np.float32),
                               np.empty((M, n, 0), np.float32) if want_post else None, np.empty((M, n, 0), np.float32) if want_nll else None)
        pred = np.empty(self._shape + (0,), dtype=np.float32)
        if steps:
            res = self._launch(steps, entry, self._rows(audio), loss=self.total_nll, log_prior=self._log_prior_be,
                               inv_temp=1.0 / self.temperature, threshold=self.threshold, decision=self._decision, want_post=want_post,
                               want_nll=want_nll, want_pred="lazy")
            self.total_nll = np.asarray(res["loss"], dtype=np.float32)
            pred = res["pred"]
            if self.threshold is not None:
                self._decision = res["carry"]
                self.decided_at = np.array(res["decision"]["step"], dtype=np.int64)
                self.decided_as = np.array(res["decision"]["member"], dtype=np.int32)
            trace = PosteriorTrace(res["best"], res["conf"], res["post"], res["nll"])
        self.last_pred = pred
        self.last = np.array(np.broadcast_to(block[..., -1], self._shape), dtype=np.float32)
        self._level = None
        trace.decided_at, trace.decided_as = self.decided_at.copy(), self.decided_as.copy()
        return trace

    def ranking(self) -> np.ndarray:
        """Per path, the members ordered by ``total_nll``, the most likely first: [M, num_paths] (a stable sort; NaN last)."""
        return np.argsort(self.total_nll, axis=0, kind="stable")

    def best(self) -> np.ndarray:
        """Per path, the member under which the scored samples so far were the most likely: [num_paths], the classifier's answer."""
        return self.ranking()[0]
