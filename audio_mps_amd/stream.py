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
"""
from __future__ import annotations

import math

import numpy as np


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
        self._A = np.float32(model.A)
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
        self._model = model
        self.total_nll = np.zeros(self.num_paths, dtype=np.float32)   # the fold carry of the scored steps so far (model.py:279)
        self.last_pred = None          # the predictions of the last score call

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
        n = self.num_paths
        if anchor or self.last is None:
            audio = block
        elif block.shape[0] == 1 and np.all(self.last == self.last[0]):
            audio = np.concatenate([self.last[:1, None], block], axis=1)
        else:
            audio = np.concatenate([self.last[:, None], np.broadcast_to(block, (n, block.shape[1]))], axis=1)
        return block, audio

    def score(self, block, anchor: bool = False) -> np.ndarray:
        """``follow`` that also says how likely the block was (cmps_psi_stream_score / cmps_rho_stream_score): same arguments, anchoring
        rule and bookkeeping, returns the negative log-likelihood of every step, [num_paths, steps] = -log(1 + e' x / A) of
        model.py:293-294 (RhoCMPS: :166, 169-170),
        and adds them to ``total_nll`` [num_paths] in step order (the fold carry of model.py:279; over a whole clip from a fresh
        stream: ``loss_per_clip``).  The predictions ``follow`` would have returned are in ``last_pred``.  Scoring changes nothing the
        stream carries: ``follow``, ``score`` and ``generate`` alternate freely, and unscored steps leave ``total_nll`` as it is."""
        entry = self._model._stream_score_entry(self._be)
        block, audio = self._anchored(block, anchor)
        n, steps = self.num_paths, audio.shape[1] - 1
        nll = np.empty((n, 0), dtype=np.float32)
        pred = np.empty((n, 0), dtype=np.float32)
        if steps:
            nll, total, pred = self._launch(steps, entry, np.ascontiguousarray(audio), want_nll=True, want_pred=True, loss=self.total_nll)
            self.total_nll = np.asarray(total, dtype=np.float32)
        self.last_pred = pred
        self.last = np.array(np.broadcast_to(block[:, -1], (n,)), dtype=np.float32)
        self._level = None
        return nll

    def follow(self, block, anchor: bool = False) -> np.ndarray:
        """Teacher-force the stream on ``block`` ([num_paths, m], or [m] / [1, m] for one signal shared by every path; the clip's own
        units).  On a stream that has seen no audio the block's first sample is the anchor X_0 and makes no step; later blocks make one
        step per sample, the first one from the stream's last sample.  ``anchor=True`` re-anchors on ``block[..., 0]`` without a step
        (to resume behind a generated gap without showing the model the jump).  Returns the model's expected increment before every
        step, [num_paths, steps]."""
        block, audio = self._anchored(block, anchor)
        n = self.num_paths
        steps = audio.shape[1] - 1
        pred = np.empty((n, 0), dtype=np.float32)
        if steps:
            _, pred = self._launch(steps, self._segment, np.ascontiguousarray(audio), None, True)
        self.last = np.array(np.broadcast_to(block[:, -1], (n,)), dtype=np.float32)
        self._level = None
        return pred

    def generate(self, length: int, noise=None) -> np.ndarray:
        """Sample ``length`` steps: [num_paths, length] in the clip's own units = the level when the sampled run began (0 on a fresh
        stream, model.py:244; else the last followed sample) + the running sum of the sampled increments, which the kernel state
        carries, so consecutive calls continue one waveform.  The noise [length, num_paths] comes from the stream's own Generator
        (stddev sigma sqrt(temp delta_t), as CMPS._noise), or is passed in.  A stream opened with ``device_noise=True`` draws it on the
        device instead (cmps_noise_fill): step k of path b gets stddev * z(noise_seed, b, k), a function of the stream's position alone, so
        how a run is cut into calls -- or into processes -- changes no bit of it."""
        length, n = int(length), self.num_paths
        if length < 1:
            raise ValueError("generate needs length >= 1")
        if self.position + length > self.max_steps:                  # (before the draw: a refused call leaves the Generator alone)
            raise ValueError(f"the stream was opened for max_steps={self.max_steps}: {self.position} taken, {length} more asked for")
        kw = {}
        if noise is None and self.device_noise:
            from .scan import NoisePlan
            noise, kw = NoisePlan(self.noise_seed, self.position, self._std), {"length": length}
        else:
            if noise is None:
                noise = (self._std * self._rng.standard_normal((length, n))).astype(np.float32)
            noise = np.asarray(noise, dtype=np.float32)
            if noise.shape != (length, n):
                raise ValueError(f"noise must be [{length}, {n}]")
        if self._level is None:
            self._level = np.zeros(n, dtype=np.float32) if self.last is None else self.last.copy()
        out, _ = self._launch(length, self._segment, None, noise, False, **kw)
        wave = (self._level[:, None] + out / self._A).astype(np.float32)
        self.last = wave[:, -1].copy()
        return wave

    def fill_gaps(self, clip, known) -> np.ndarray:
        """``clip`` [T] or [num_paths, T] with a boolean mask ``known`` [T]: runs of True are followed, runs of False generated, and each
        known run behind a gap is re-anchored on its first sample.  Returns [num_paths, T]: the clip where it is known, the model's
        waveform in the gaps."""
        clip = self._block(clip)
        known = np.asarray(known, dtype=bool)
        if known.shape != (clip.shape[1],):
            raise ValueError(f"known must be a boolean mask [{clip.shape[1]}]")
        T, n = clip.shape[1], self.num_paths
        wave = np.array(np.broadcast_to(clip, (n, T)), dtype=np.float32)
        edges = [0] + [k for k in range(1, T) if known[k] != known[k - 1]] + [T]
        for a, b in zip(edges[:-1], edges[1:]):
            if known[a]:
                self.follow(clip[:, a:b], anchor=a > 0)
            else:
                wave[:, a:b] = self.generate(b - a)
        return wave
