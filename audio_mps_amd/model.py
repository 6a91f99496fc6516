"""Host-side mirror of the reference's model surface for the pure-state path.

Same class names, constructor arguments, hyper-parameter field names and attributes as
/root/reference/model.py (CMPS :5-52, PsiCMPS :206-334) and the legacy ``AudioMPS`` surface that
training_estimators.py:43-45 / follow_vae.py:45-51 call.  The reference builds a TensorFlow graph whose
``.loss`` tensor is evaluated in a session and differentiated by ``AdamOptimizer.minimize``
(train.py:89); here ``.loss`` launches the HIP scan (audio_mps_amd/csrc) and ``loss_and_grads()`` runs
the forward + reverse kernels and applies the tiny host-side chain rule from the kernels' outputs
(gradients w.r.t. the effective R, freqs, psi_0, A) to the raw variables (Rx, Ry, freqs, psi_x, psi_y, A).

RhoCMPS (model.py:55-203, ``mixed=True``) is mirrored the same way on top of the cmps_rho_* entry points.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Callable, Dict, Optional

import numpy as np

from . import layout
from .layout import EffectiveParams, unpack_grad

VARIABLE_NAMES = ("A", "Rx", "Ry", "freqs", "psi_x", "psi_y")


# --------------------------------------------------------------------------------------------------
# hyper-parameters: field names of tf.contrib.training.HParams at train.py:41-43
# --------------------------------------------------------------------------------------------------
@dataclass
class HParams:
    minibatch_size: int = 8
    bond_dim: int = 8
    delta_t: float = 1.0 / 16000
    sigma: float = 0.0001
    h_reg: float = 200.0 / (math.pi * 16000) ** 2
    r_reg: float = 0.1
    initial_rank: Optional[int] = None
    A: float = 100.0
    learning_rate: float = 0.001

    def parse(self, spec: str) -> "HParams":
        """``--hparams=name=value,...`` override (train.py:31,44)."""
        if not spec:
            return self
        known = {f.name: f for f in fields(self)}
        for item in spec.split(","):
            if not item.strip():
                continue
            name, _, value = item.partition("=")
            name = name.strip()
            if name not in known:
                raise ValueError(f"Unknown hyperparameter: {name}")
            cur = getattr(self, name)
            if name == "initial_rank":
                setattr(self, name, None if value.strip() in ("None", "") else int(value))
            elif isinstance(cur, int) and not isinstance(cur, bool):
                setattr(self, name, int(value))
            else:
                setattr(self, name, float(value))
        return self

    def values(self) -> dict:
        return {f.name: getattr(self, f.name) for f in fields(self)}


def _f32(x):
    return np.float32(x)


def _rsqrt32(x) -> np.float32:
    """tf.rsqrt(python_float): evaluated in float32 (model.py:36,38,49)."""
    return np.float32(1) / np.sqrt(np.float32(x))


def _normalize_psi_host(p: np.ndarray) -> np.ndarray:
    """_normalize_psi with axis=None (model.py:327-334) for the D-vector psi_0 (tiny; host)."""
    a = np.abs(p).astype(np.float32)
    ss = np.sum(np.square(a), dtype=np.float32)
    inv = np.float32(1) / np.sqrt(np.maximum(ss, np.float32(1e-12)))
    return (p * np.complex64(inv)).astype(np.complex64)


# --------------------------------------------------------------------------------------------------
class _ScanModel:
    """What every model class needs to run a scan on its backend.  Expects ``bond_d``, ``data_iterator``, ``_backend``, ``_last`` and
    the subclass's ``_prepare(B, T, train)`` (upload the parameters, return the backend), ``_forward_entry(be)`` (the backend's forward
    scan for this model), ``grad_sums`` and ``chain_rule``."""

    def _get_backend(self):
        if self._backend is None:
            from .scan import HipScan   # raises if libcmps.so or the GPU is missing: no fallback
            self._backend = HipScan(self.bond_d)
        return self._backend

    def _batch(self, data=None):
        data = self.data_iterator if data is None else data
        if callable(data):
            data = data()
        return data

    def _to_device(self, data):
        import torch
        be = self._get_backend()
        dev = getattr(be, "device", None)
        if isinstance(data, torch.Tensor):
            t = data.to(dtype=torch.float32)
            if dev is not None:
                t = t.to(dev)
            return t.contiguous()
        t = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))
        return t.to(dev) if dev is not None else t

    def _scan(self, data, train: bool):
        """(backend holding the current parameters, the batch on its device, B, T): the start of every scan method."""
        audio = self._to_device(self._batch(data))
        B, T = audio.shape
        return self._prepare(B, T, train), audio, B, T

    def loss_per_clip_dev(self, data=None):
        """``loss_per_clip`` left where the scan wrote it: the backend's per-clip loss tensor [B] (forward only; the next forward
        overwrites it).  What an evaluation pass reduces on the device (audio_mps_amd/evaluate.py)."""
        be, audio, _, _ = self._scan(data, train=False)
        return self._forward_entry(be)(audio, save_for_bwd=False)

    def loss_and_grads(self, data=None, with_reg: bool = False):
        """(loss, {variable: gradient}) of mean_b loss_b (+ train.py's regularisers if with_reg): what
        ``AdamOptimizer.minimize`` obtains from TF (train.py:89)."""
        flat, B = self.grad_sums(data)
        host = flat.detach().cpu().numpy() if hasattr(flat, "detach") else np.asarray(flat)
        self._last = host
        return self.chain_rule(host, B, with_reg=with_reg)


class _VarDict(dict):
    """model.variables: a plain dict whose item assignment invalidates a live device-resident copy of the variables (see CMPS.variables)."""

    def __init__(self, model):
        super().__init__()
        self._model = model

    def __setitem__(self, key, value):
        owner = self._model._owner()
        if owner is not None:
            owner.drop_device_state()              # device -> host for everything else, then forget the device copy (if one is live)
        super().__setitem__(key, value)


class CMPS(_ScanModel):
    """Continuous Matrix Product State: the trainable variables and the effective parameters
    (model.py:5-52).  ``self.R`` (complex64 [D,D], diagonal removed as at model.py:42), ``self.freqs``,
    ``self.A``, ``self.sigma`` are the attributes train.py:55-75 reads."""

    def __init__(self, hparams, data_iterator=None, freqs_in=None, R_in=None, seed: int = 0):
        self._device_owner = None      # weak reference to the ResidentState (Trainer, BankTrainer) that holds a device copy of self._variables
        self._dirty_owner = None       # that owner again, held STRONGLY while its device state has steps the host copies lack
        self._backend = None           # the scan implementation (the subclasses' `backend` argument); None: a HipScan on first use
        self._last = None              # the flat gradient sums of the last loss_and_grads (host copy)
        self.hparams = hparams
        self.bond_d = int(hparams.bond_dim)
        self.batch_size = hparams.minibatch_size
        self.h_reg = hparams.h_reg
        self.r_reg = hparams.r_reg
        self.delta_t = hparams.delta_t
        self.dt = np.float32(hparams.delta_t)                     # model.py:16
        self.sigma = hparams.sigma                                # model.py:21 (not trainable)
        self.data_iterator = data_iterator
        D = self.bond_d
        rng = np.random.default_rng(seed)
        self._variables: Dict[str, np.ndarray] = _VarDict(self)
        self.variables["A"] = np.asarray(np.float32(hparams.A))   # model.py:19
        # --- R (model.py:31-42)
        if R_in is not None:
            R_in = np.asarray(R_in)
            if R_in.shape != (D, D):
                raise ValueError(f"R_in must be [{D},{D}]")
            self.variables["Rx"] = R_in.real.astype(np.float32)
            self.variables["Ry"] = R_in.imag.astype(np.float32)
            self._c_r = np.float32(1)
        else:
            self.variables["Rx"] = rng.standard_normal((D, D)).astype(np.float32)   # random_normal_initializer
            self.variables["Ry"] = rng.standard_normal((D, D)).astype(np.float32)
            self._c_r = _rsqrt32(self.r_reg)
        # --- freqs (model.py:44-49)
        if freqs_in is not None:
            freqs_in = np.asarray(freqs_in, dtype=np.float32)
            if freqs_in.shape != (D,):
                raise ValueError(f"freqs_in must be [{D}]")
            self.variables["freqs"] = freqs_in.copy()
            self._c_h = np.float32(1)
        else:
            self.variables["freqs"] = rng.standard_normal(D).astype(np.float32)
            self._c_h = _rsqrt32(self.h_reg)
        self._rng = rng

    def _owner(self):
        ref = self._device_owner
        return ref() if ref is not None else None

    @property
    def variables(self) -> Dict[str, np.ndarray]:
        """The raw trainable variables (host copies).  While a Trainer or a BankTrainer runs the device-resident optimiser step the
        current values live on the GPU; reading this attribute then brings them back first (ResidentState._lazy_sync,
        audio_mps_amd/resident.py: one device -> host copy, only after steps that changed them), so loss / sample / effective_params /
        summaries never see stale parameters.  ASSIGNING an entry (``m.variables["Rx"] = ...``, ``m.variables["Rx"] *= c``)
        while a device-resident state is live brings that state back and drops it (drop_device_state), so the owner's next step starts
        from the host values (such writes used to be ignored).  The owner is held by a weak reference and, only while it has
        device steps that have not come back, by a strong one as well (``_dirty_owner``): an owner that goes out of scope in that state,
        e.g. inside a helper that returns the model alone, stays alive until this attribute has brought its steps back instead of taking
        them with it (ADVICE: they used to be lost without notice).  The model <-> owner cycle of that interval is the garbage
        collector's to break; an owner that is not dirty is still released at once."""
        owner = self._owner()
        if owner is not None:
            owner._lazy_sync()
        return self._variables

    # effective parameters, recomputed from the current variables ---------------------------------
    @property
    def A(self) -> np.float32:
        return np.float32(self.variables["A"])

    @property
    def R(self) -> np.ndarray:
        Rx = (self._c_r * self.variables["Rx"]).astype(np.float32) if self._c_r != 1 else self.variables["Rx"]
        Ry = (self._c_r * self.variables["Ry"]).astype(np.float32) if self._c_r != 1 else self.variables["Ry"]
        Z = (Rx + 1j * Ry).astype(np.complex64)                   # model.py:41
        return (Z - np.diagonal(Z)[None, :]).astype(np.complex64)  # model.py:42 (row-vector broadcast)

    @property
    def freqs(self) -> np.ndarray:
        f = self.variables["freqs"]
        return (self._c_h * f).astype(np.float32) if self._c_h != 1 else f.astype(np.float32)

    @property
    def freqsc(self) -> np.ndarray:
        return self.freqs.astype(np.complex64)                    # model.py:52

    _LOSS_LINE = None              # where the reference's subclass defines `loss` (cited by its AttributeError)

    @property
    def loss(self) -> np.float32:
        """``.loss`` of the reference (PsiCMPS model.py:224-225, 267; RhoCMPS :69-70, 144): mean over the batch of the per-clip loss."""
        if self.data_iterator is None:
            raise AttributeError(f"loss: the model was built without a data_iterator (model.py:{self._LOSS_LINE})")
        return np.float32(np.mean(self.loss_per_clip(), dtype=np.float32))

    def _effective(self, psi0) -> EffectiveParams:
        return EffectiveParams(R=self.R, freqs=self.freqs, psi0=psi0, A=float(self.A),
                               sigma=float(self.sigma), delta_t=float(self.delta_t))

    @staticmethod
    def _noise_seed(seed) -> int:
        """The 64-bit seed of device-drawn noise: ``seed``, or (None) a fresh 63-bit one from the system's entropy."""
        if seed is None:
            return int(np.random.SeedSequence().entropy) & (2 ** 63 - 1)
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("the seed of device-drawn noise must lie in [0, 2^64)")
        return seed

    def _device_noise_backend(self):
        """The backend, if it can draw noise itself (HipScan.draw_noise, cmps_noise_fill); else device_noise=True is a ValueError."""
        be = self._get_backend()
        if not hasattr(be, "draw_noise"):
            raise ValueError(f"device_noise=True needs a backend that draws noise on the device (draw_noise): {type(be).__name__} has none")
        return be

    @staticmethod
    def _plan_shape(noise, length, n) -> dict:
        """The ``length`` / ``n`` keywords a backend's sampler entry needs next to a NoisePlan; none next to an array, which brings its shape."""
        if isinstance(noise, np.ndarray):
            return {}
        from .scan import NoisePlan
        return {"length": int(length), "n": int(n)} if isinstance(noise, NoisePlan) else {}

    def _noise(self, num_samples, length, temp, seed, noise, device_noise=False, first_step=0):
        """The sampler's Gaussian noise [length, num_samples] (stddev sigma * sqrt(temp * delta_t), model.py:246 / :88, 96, 106):
        drawn on the host with a numpy Generator (``seed``), or ``noise`` as passed in, like the reference's tensor.  With ``device_noise``
        (and no ``noise``) nothing is drawn here: the return value is a NoisePlan(seed, first_step, stddev) the backend draws from on the
        device, where it samples (cmps_noise_fill); ``first_step`` is the table row of the first sampled step."""
        std = float(self.sigma) * math.sqrt(temp * float(self.delta_t))
        if noise is None and device_noise:
            from .scan import NoisePlan
            self._device_noise_backend()
            return NoisePlan(self._noise_seed(seed), int(first_step), std)
        if noise is None:
            rng = np.random.default_rng(seed)
            noise = (std * rng.standard_normal((length, num_samples))).astype(np.float32)
        noise = np.asarray(noise, dtype=np.float32)
        if noise.shape != (length, num_samples):
            raise ValueError(f"noise must be [{length}, {num_samples}]")
        return noise

    # ---- primed sampling: units and shapes around the subclass's sample(prime=...) and its backend entry ----
    def _sample_primed(self, be, prime, noise, want_pred, length=None, n=None):
        """The backend's primed sampler for this model, (out, pred) with want_pred: HipScan.sample_primed / rho_sample_primed.  ``length``
        and ``n`` are needed where ``noise`` is a NoisePlan."""
        raise NotImplementedError

    # ---- resumable sampling (audio_mps_amd/stream.py) ----
    def _stream_entries(self, be):
        """The backend's resumable sampler for this model, (state allocator, segment entry): HipScan.stream_state / stream, or
        rho_stream_state / rho_stream."""
        raise NotImplementedError

    def _stream_score_entry(self, be):
        """The backend's scored segment entry for this model: HipScan.stream_score, or rho_stream_score."""
        raise NotImplementedError

    def nll_per_step(self, data=None, segment=None) -> np.ndarray:
        """The fold's increment of every step, [B, T - 1]: -log(1 + e' x / A) of model.py:276-282, 293-294 (RhoCMPS: :152-158,
        169-170; the reference only returns their sum).  One scored stream over the batch (cmps_psi_stream_score / cmps_rho_stream_score), cut into segments of ``segment`` steps when given -- the
        cut changes no bit.  Row sums are ``loss_per_clip`` to float32 rounding."""
        from .stream import as_clips, segments
        data = as_clips(self._batch(data), "nll_per_step")
        B, N = data.shape[0], data.shape[1] - 1
        cuts = segments(N, segment)
        st = self.open_stream(B, N)
        return np.concatenate([st.score(data[:, lo:hi]) for lo, hi in cuts], axis=1)

    def _prepare_stream(self, num_paths, max_steps, keep_states=0):
        """The backend as a stream needs it: T = max_steps + 1, one table row per step."""
        return self._prepare(num_paths, max_steps + 1, train=False)

    def open_stream(self, num_paths, max_steps, temp=1, seed=None, device_noise=False):
        """A resumable sampler of ``num_paths`` paths (no reference counterpart; audio_mps_amd/stream.py, cmps_psi_stream /
        cmps_rho_stream): follow (and score) an incoming signal block by block, generate in segments, or alternate.  Prepares the backend once with
        T = max_steps + 1 -- the only sizing decision, 8 DP bytes of phase table per step; running past ``max_steps`` raises ValueError.
        The model's variables are read here: a stream keeps the parameters it was opened with.  ``device_noise=True``: ``generate`` draws
        its noise on the device from (``seed``, path, step) instead of a host Generator (SampleStream.generate)."""
        from .stream import SampleStream
        return SampleStream(self, num_paths, max_steps, temp=temp, seed=seed, device_noise=device_noise)

    @staticmethod
    def _prime(prime, num_samples) -> np.ndarray:
        """A prime as the backend takes it: float32 [1, T'] (shared by every path) or [num_samples, T'], T' >= 2."""
        from .stream import as_clips
        prime = as_clips(prime, "prime")
        if prime.shape[0] not in (1, num_samples):
            raise ValueError(f"prime must be [T'], [1, T'] or [{num_samples}, T'], not {prime.shape}")
        return prime

    def continue_clip(self, prime, num_samples, length, temp=1, seed=None, noise=None, device_noise=False) -> np.ndarray:
        """The continuation of ``prime`` in the clip's own units, [num_samples, length]: the array to plot or write behind the clip.
        The model's waveform is A * (running sum of increments) and the data enter as increments / A (model.py:303, :175), so the
        sampled sum is divided by A and starts from the clip's last sample."""
        prime = self._prime(prime, num_samples)
        out = self.sample(num_samples, length, temp=temp, seed=seed, noise=noise, prime=prime, device_noise=device_noise)
        return (prime[..., -1:] + out / self.A).astype(np.float32)

    def predict_increments(self, data=None) -> np.ndarray:
        """Teacher-forced one-step predictions [B, T - 1] for a batch [B, T] (default: the model's data_iterator): entry k is the
        model's expected increment (2 Re<psi|R|psi> delta_t, or Re tr((Rt + Rt^dagger) rho) delta_t) at t_k, given the clip up to sample
        k -- to compare with data[:, k + 1] - data[:, k].  Runs the primed sampler with one sampled step and discards it."""
        data = self._batch(data)
        if data is None:
            raise ValueError("predict_increments needs a batch (data, or the model's data_iterator)")
        B = int(np.shape(data)[0])
        prime = self._prime(data, B)
        be = self._prepare(B, prime.shape[1] + 1, train=False)
        return self._sample_primed(be, prime, np.zeros((1, B), dtype=np.float32), True)[1]

    def _chain_common(self, Rbar, fbar, Abar, loss, with_reg: bool):
        """Adjoint of model.py:36-42 (scaling + the row-broadcast diagonal removal) and :49 for batch-mean cotangents of
        the effective R, freqs, A; optionally the regularisers of train.py:55-60."""
        if with_reg:
            R = self.R.astype(np.complex128)
            f = self.freqs.astype(np.float64)
            loss = loss + self.h_reg * np.sum(f * f) + self.r_reg * np.sum((np.conj(R) * R).real)
            fbar = fbar + 2.0 * self.h_reg * f
            Rbar = Rbar + 2.0 * self.r_reg * R
        Zbar = Rbar - np.diag(np.sum(Rbar, axis=0))               # adjoint of model.py:42
        c_r, c_h = float(self._c_r), float(self._c_h)
        return loss, {
            "A": np.asarray(np.float32(Abar)),
            "Rx": (c_r * Zbar.real).astype(np.float32),
            "Ry": (c_r * Zbar.imag).astype(np.float32),
            "freqs": (c_h * fbar).astype(np.float32),
        }


# --------------------------------------------------------------------------------------------------
class PsiCMPS(CMPS):
    """Evolves the state (model.py:206-334).

    ``data_iterator`` is the batch the loss is evaluated on: a float32 [B, T] numpy array or CUDA tensor,
    or a zero-argument callable returning one (the eager stand-in for the TF input tensor that yields a
    new batch per session.run).  ``backend`` is the scan implementation; the product has exactly one
    (``HipScan``, the HIP kernels) and constructs it on first use -- tests may inject another object with
    the same two methods to exercise the host logic without a GPU.
    """

    _LOSS_LINE = 224

    def __init__(self, hparams, psi_in=None, *args, backend=None, **kwargs):
        super().__init__(hparams, *args, **kwargs)
        D = self.bond_d
        if psi_in is not None:
            # the reference's branch is broken (undefined psi_x_in, model.py:214-216); a complex D-vector
            psi_in = np.asarray(psi_in)
            if psi_in.shape != (D,):
                raise ValueError(f"psi_in must be [{D}]")
            self.variables["psi_x"] = psi_in.real.astype(np.float32)
            self.variables["psi_y"] = psi_in.imag.astype(np.float32)
        else:
            # initializer=None -> TF default glorot_uniform; 1-D [D]: limit sqrt(6 / (D + D))  (model.py:218-219)
            lim = math.sqrt(6.0 / (2 * D))
            self.variables["psi_x"] = self._rng.uniform(-lim, lim, D).astype(np.float32)
            self.variables["psi_y"] = self._rng.uniform(-lim, lim, D).astype(np.float32)
        self._backend = backend

    # ---- attributes of the reference object ----
    @property
    def psi_0(self) -> np.ndarray:
        p = (self.variables["psi_x"] + 1j * self.variables["psi_y"]).astype(np.complex64)   # model.py:221
        return _normalize_psi_host(p)                                                        # model.py:222

    # ---- backend plumbing ----
    def effective_params(self):
        return self._effective(self.psi_0)

    def _prepare(self, B, T, train):
        be = self._get_backend()
        be.set_params(self.effective_params(), B, T, train=train)
        return be

    # ---- the hot path ----
    def loss_per_clip(self, data=None) -> np.ndarray:
        """The fold carry ``loss`` [B] of model.py:265-266 (forward only)."""
        return self.loss_per_clip_dev(data).detach().cpu().numpy()

    def _forward_entry(self, be):
        return be.forward

    def flat_size(self) -> int:
        """Length of the buffer grad_sums() returns (cmps_psi_loss_bwd's layout): what an empty shard adds to the all-reduce as zeros."""
        return layout.grad_size(self.bond_d)

    def grad_sums(self, data=None):
        """Forward + reverse scan on this process's clips.  Returns (flat device/host buffer of SUMS over
        clips as laid out by cmps_psi_loss_bwd, number of clips).  Used by loss_and_grads and by the
        data-parallel trainer, which all-reduces the buffer before the chain rule."""
        be, audio, B, _ = self._scan(data, train=True)
        _, grad = be.loss_and_grad_sums(audio, check=True)       # fp16-range check + documented fallback (include/cmps.h)
        return grad, B

    def chain_rule(self, flat_sums: np.ndarray, global_batch: int, with_reg: bool = False):
        """Effective-parameter gradient sums -> (mean loss, gradients w.r.t. the raw variables).
        Adjoint of model.py:36-42 (scaling + the row-broadcast diagonal removal), :49, :221-222, and
        optionally the regularisers of train.py:55-60."""
        g = unpack_grad(np.asarray(flat_sums, dtype=np.float64), self.bond_d)
        invB = 1.0 / float(global_batch)
        p0bar = g["psi0bar"] * invB
        loss, grads = self._chain_common(g["Rbar"] * invB, g["fbar"] * invB, g["Abar"] * invB, g["loss_sum"] * invB, with_reg)
        p = (self.variables["psi_x"].astype(np.float64) + 1j * self.variables["psi_y"].astype(np.float64))
        ss = float(np.sum(np.abs(p) ** 2))
        m = max(ss, 1e-12)
        inv = 1.0 / math.sqrt(m)
        pbar = p0bar * inv
        if ss > 1e-12:
            inv_bar = float(np.sum((np.conj(p0bar) * p).real))
            pbar = pbar + 2.0 * (inv_bar * (-0.5 * inv / m)) * p
        grads["psi_x"] = pbar.real.astype(np.float32)
        grads["psi_y"] = pbar.imag.astype(np.float32)
        return np.float32(loss), grads

    # ---- other reference methods on this class ----
    def _update_ancilla_psi(self, psi, signal, t):
        """model.py:300-317 for a batch of states (used by the reference's testTrivialUpdateOfAncilla)."""
        psi = np.asarray(psi, dtype=np.complex64)
        return self._prepare(psi.shape[0], 2, train=False).update_ancilla(psi, np.asarray(signal, dtype=np.float32), float(t))

    def psi_evolve_with_data(self, data=None) -> np.ndarray:
        """model.py:231-240: the normalised state after every step, [B, T-1, D]."""
        be, audio, _, _ = self._scan(data, train=True)
        be.forward(audio, save_for_bwd=True)
        return be.states()

    def sample(self, num_samples, length, temp=1, seed=None, noise=None, prime=None, return_pred=False, device_noise=False):
        """model.py:242-251: waveforms [num_samples, length] = A * running sum of the sampled increments.
        The Gaussian noise (stddev sigma * sqrt(temp * delta_t), model.py:246) is drawn on the host with a numpy
        Generator (``seed``), or passed in as ``noise`` [length, num_samples] like the reference's tensor.  ``device_noise=True``
        draws it on the device instead, where the reference draws it: counter-based normals of (``seed``, path, table row of the step)
        (cmps_noise_fill; ``seed=None``: a fresh seed), so a primed sample and a stream that followed the same clip draw the same noise.
        An explicit ``noise`` wins.

        ``prime`` (no reference counterpart): a clip [T'], [1, T'] (shared by all paths) or [num_samples, T'] the state is first
        teacher-forced on -- T' - 1 steps of _psi_update (model.py:269-274) on its increments -- before the ``length`` sampled
        steps follow in the same scan (cmps_psi_sample_primed).  The return value keeps the reference's convention: A * running
        sum of the SAMPLED increments, zero at the hand-over (``continue_clip`` returns the clip's own units).  ``return_pred``
        adds the model's expected increment of every forced step, [num_samples, T' - 1]."""
        if prime is None:
            if return_pred:
                raise ValueError("return_pred needs a prime: the predictions belong to the teacher-forced steps")
            noise = self._noise(num_samples, length, temp, seed, noise, device_noise)
            return self._prepare(num_samples, length + 1, train=False).sample(noise, **self._plan_shape(noise, length, num_samples))
        prime = self._prime(prime, num_samples)
        noise = self._noise(num_samples, length, temp, seed, noise, device_noise, first_step=prime.shape[1] - 1)
        be = self._prepare(num_samples, prime.shape[1] + length, train=False)    # one table row per step, forced or sampled
        return self._sample_primed(be, prime, noise, bool(return_pred), length, num_samples)

    def _sample_primed(self, be, prime, noise, want_pred, length=None, n=None):
        return be.sample_primed(prime, noise, want_pred=want_pred, **self._plan_shape(noise, length, n))

    def _stream_entries(self, be):
        return be.stream_state, be.stream

    def _stream_score_entry(self, be):
        return be.stream_score


# --------------------------------------------------------------------------------------------------
class RhoCMPS(CMPS):
    """Evolves the density matrix (model.py:55-203).

    Variables Wx, Wy [rank, D] (rank = hparams.initial_rank or bond_dim, :62-65), rho_0 = W^dagger W / trace (:127-132).
    The HIP scan carries rho as its ``rank`` columns phi_a = conj(W[a, :]) / sqrt(trace) (cmps_rho_* in include/cmps.h);
    everything the reference exposes on this class is mirrored: ``loss``, ``rho_0``, ``rho_evolve_with_data``,
    ``rho_evolve_with_sampling``, ``purity``, ``sample``, ``_update_ancilla_rho``."""

    VARIABLE_NAMES = ("A", "Rx", "Ry", "freqs", "Wx", "Wy")
    _LOSS_LINE = 69

    def __init__(self, hparams, W_in=None, *args, backend=None, **kwargs):
        super().__init__(hparams, *args, **kwargs)
        D = self.bond_d
        self.rank_rho_0 = int(hparams.initial_rank) if hparams.initial_rank is not None else D     # :62-65
        if W_in is not None:
            W_in = np.asarray(W_in)
            if W_in.ndim != 2 or W_in.shape[1] != D:
                raise ValueError(f"W_in must be [rank, {D}]")
            self.rank_rho_0 = W_in.shape[0]
            self.variables["Wx"] = W_in.real.astype(np.float32)                                    # :121-124
            self.variables["Wy"] = W_in.imag.astype(np.float32)
        else:
            # initializer=None -> glorot_uniform on [rank, D]: limit sqrt(6 / (rank + D))           (:126-127)
            lim = math.sqrt(6.0 / (self.rank_rho_0 + D))
            self.variables["Wx"] = self._rng.uniform(-lim, lim, (self.rank_rho_0, D)).astype(np.float32)
            self.variables["Wy"] = self._rng.uniform(-lim, lim, (self.rank_rho_0, D)).astype(np.float32)
        self._backend = backend

    # ---- attributes of the reference object ----
    @property
    def W(self) -> np.ndarray:
        return (self.variables["Wx"] + 1j * self.variables["Wy"]).astype(np.complex64)            # :128

    @property
    def rho_0(self) -> np.ndarray:
        W = self.W
        r0 = (np.conj(W.T) @ W).astype(np.complex64)                                               # :129
        return (r0 / np.trace(r0)).astype(np.complex64)                                            # :130

    def columns(self) -> np.ndarray:
        """phi [rank, D] with rho_0 = sum_a phi_a phi_a^dagger: phi_a = conj(W[a, :]) / sqrt(tr W^dagger W)."""
        W = self.W.astype(np.complex128)
        t0 = float(np.sum(np.abs(W) ** 2))
        return (np.conj(W) / math.sqrt(t0)).astype(np.complex64)

    def effective_params(self):
        e0 = np.zeros(self.bond_d, dtype=np.complex64)
        e0[0] = 1                                                  # the pure-state psi_0 slot is unused on this path
        return self._effective(e0)

    def _prepare(self, B, T, train):
        be = self._get_backend()
        be.set_params(self.effective_params(), B, T, train=False)
        be.rho_set_state(self.columns(), B, T, train=train)
        return be

    # ---- the scan ----
    def loss_per_clip(self, data=None) -> np.ndarray:
        return self.loss_per_clip_dev(data).detach().cpu().numpy()

    def _forward_entry(self, be):
        return be.rho_forward

    def flat_size(self) -> int:
        """Length of the buffer grad_sums() returns: the pure-state layout followed by the 2 rank D column cotangents
        (include/cmps.h: cmps_rho_loss_bwd)."""
        return layout.grad_size(self.bond_d, self.rank_rho_0)

    def grad_sums(self, data=None):
        """(flat buffer of SUMS over this process's clips as laid out by cmps_rho_loss_bwd, number of clips)."""
        be, audio, B, _ = self._scan(data, train=True)
        _, grad = be.rho_loss_and_grad_sums(audio)
        return grad, B

    def chain_rule(self, flat_sums: np.ndarray, global_batch: int, with_reg: bool = False):
        """Effective-parameter gradient sums -> (mean loss, gradients w.r.t. A, Rx, Ry, freqs, Wx, Wy)."""
        g = unpack_grad(np.asarray(flat_sums, dtype=np.float64), self.bond_d, self.rank_rho_0)
        invB = 1.0 / float(global_batch)
        loss, grads = self._chain_common(g["Rbar"] * invB, g["fbar"] * invB, g["Abar"] * invB, g["loss_sum"] * invB, with_reg)
        phibar = g["phibar"] * invB
        # phi = p / |p|, p = conj(W) (all rank * D entries as one vector), then W = conj(p)        adjoint of :128-130
        W = self.W.astype(np.complex128)
        nrm = math.sqrt(float(np.sum(np.abs(W) ** 2)))
        phi = np.conj(W) / nrm
        pbar = (phibar - phi * float(np.sum((np.conj(phi) * phibar).real))) / nrm
        grads["Wx"] = pbar.real.astype(np.float32)
        grads["Wy"] = (-pbar.imag).astype(np.float32)
        return np.float32(loss), grads

    # ---- other reference methods on this class ----
    def _update_ancilla_rho(self, rho, signal, t):
        """model.py:172-187 for a batch of density matrices [B, D, D]."""
        be = self._get_backend()
        rho = np.asarray(rho, dtype=np.complex64)
        be.set_params(self.effective_params(), rho.shape[0], 2, train=False)      # (needs no cmps_rho_set_state)
        return be.rho_update_ancilla(rho, np.asarray(signal, dtype=np.float32), float(t))

    def rho_evolve_with_data(self, data=None) -> np.ndarray:
        """model.py:76-84: the normalised rho after every step, [B, T-1, D, D]."""
        be, audio, B, T = self._scan(data, train=True)
        be.rho_forward(audio, save_for_bwd=True)
        return be.rho_states(B, T - 1, want_rho=True)

    def _sample_primed(self, be, prime, noise, want_pred, save_states=False, length=None, n=None):
        return be.rho_sample_primed(prime, noise, want_pred=want_pred, save_states=save_states, **self._plan_shape(noise, length, n))

    def _stream_entries(self, be):
        return be.rho_stream_state, be.rho_stream

    def _stream_score_entry(self, be):
        entry = getattr(be, "rho_stream_score", None)
        if entry is None:                                             # (as device_noise on a backend that cannot draw: said before anything runs)
            raise ValueError(f"this backend scores PsiCMPS-only streams: {type(be).__name__} has no rho_stream_score (cmps_rho_stream_score)")
        return entry

    def _prepare_stream(self, num_paths, max_steps, keep_states=0):
        if not keep_states:
            return super()._prepare_stream(num_paths, max_steps)
        be = self._get_backend()
        be.set_params(self.effective_params(), num_paths, max_steps + 1, train=False)
        be.rho_set_state(self.columns(), num_paths, keep_states + 1, train=True)     # (its T is the stash's capacity, not the tables')
        return be

    def open_stream(self, num_paths, max_steps, temp=1, seed=None, keep_states=0, device_noise=False):
        """CMPS.open_stream, from rho_0.  ``keep_states = S > 0`` also keeps the columns of every follow / generate call of at most S
        steps (a longer one raises ValueError), so that ``st.states()`` [num_paths, steps, D, D] and ``st.purity()`` [num_paths, steps]
        return the lab-frame rho and tr rho^2 after every step of the last call: rho along a run of any length from a stash that holds
        S steps (num_paths * S * rank * D' * 8 bytes) instead of the whole run."""
        from .stream import SampleStream
        keep_states = int(keep_states)
        if keep_states < 0:
            raise ValueError("keep_states must not be negative")
        return SampleStream(self, num_paths, max_steps, temp=temp, seed=seed, keep_states=min(keep_states, int(max_steps)),
                            device_noise=device_noise)

    def _sample_scan(self, num_samples, length, temp, seed, noise, save_states, prime=None, want_pred=False, device_noise=False):
        """(backend, what its sampler returned, steps of the scan): unprimed, or (``prime``) P = T' - 1 forced steps in front."""
        if prime is None:
            noise = self._noise(num_samples, length, temp, seed, noise, device_noise)
            be = self._prepare(num_samples, length + 1, train=save_states)
            return be, be.rho_sample(noise, save_states=save_states, **self._plan_shape(noise, length, num_samples)), length
        prime = self._prime(prime, num_samples)
        noise = self._noise(num_samples, length, temp, seed, noise, device_noise, first_step=prime.shape[1] - 1)
        be = self._prepare(num_samples, prime.shape[1] + length, train=save_states)      # one table row per step, forced or sampled
        return be, self._sample_primed(be, prime, noise, want_pred, save_states, length, num_samples), prime.shape[1] - 1 + length

    def sample(self, num_samples, length, temp=1, seed=None, noise=None, prime=None, return_pred=False, device_noise=False):
        """model.py:103-116: waveforms [num_samples, length] = A * running sum of the sampled increments.  ``device_noise`` as in
        PsiCMPS.sample: the noise is drawn on the device (cmps_noise_fill) unless ``noise`` is given.

        ``prime`` / ``return_pred`` as in PsiCMPS.sample: the state is first teacher-forced on the clip -- T' - 1 steps of _rho_update
        (model.py:144-150) on its increments -- and the ``length`` sampled steps follow in the same scan (cmps_rho_sample_primed);
        ``return_pred`` adds Re tr((Rt + Rt^dagger) rho) delta_t before every forced step, [num_samples, T' - 1]."""
        if prime is None and return_pred:
            raise ValueError("return_pred needs a prime: the predictions belong to the teacher-forced steps")
        return self._sample_scan(num_samples, length, temp, seed, noise, False, prime, bool(return_pred), device_noise)[1]

    def rho_evolve_with_sampling(self, num_samples, length, temp=1, seed=None, noise=None, prime=None, device_noise=False) -> np.ndarray:
        """model.py:86-92: rho after every sampled step, [num_samples, length, D, D]; with ``prime`` [num_samples, P + length, D, D], the
        P = T' - 1 teacher-forced steps first."""
        be, _, steps = self._sample_scan(num_samples, length, temp, seed, noise, True, prime, device_noise=device_noise)
        return be.rho_states(num_samples, steps, want_rho=True)

    def purity(self, num_samples, length, temp=1, seed=None, noise=None, prime=None, device_noise=False) -> np.ndarray:
        """model.py:94-101: tr rho^2 along sampled paths, [num_samples, length]; with ``prime`` [num_samples, P + length], forced steps first."""
        be, _, steps = self._sample_scan(num_samples, length, temp, seed, noise, True, prime, device_noise=device_noise)
        return be.rho_states(num_samples, steps, want_rho=False, want_purity=True)


class LegacyAudioMPS(_ScanModel):
    """The legacy ``AudioMPS`` arithmetic (reconstructed from logging/graph.pbtxt): real
    variables H, R [D,D] (glorot-uniform), H_s = tril(H) + tril(H)^T, psi_0 = e_0,
    loss = mean_b sum_k (x_k - 2 Re<psi|R|psi>)^2 / 2 evaluated BEFORE the update,
    psi' = psi + dt (-i H_s - R^T R / 2) psi + dt x R psi, normalised.  Trained with Adam(1e-3) on the bare loss
    (training_estimators.py:64-68)."""

    VARIABLE_NAMES = ("H", "R")

    def __init__(self, bond_d, dt, batch_size=8, data_iterator=None, seed: int = 0, backend=None):
        self.bond_d = int(bond_d)
        self.delta_t = float(dt)
        self.batch_size = batch_size
        self.data_iterator = data_iterator
        rng = np.random.default_rng(seed)
        lim = math.sqrt(6.0 / (2 * self.bond_d))            # glorot_uniform, graph.pbtxt:9076-9114
        self.variables: Dict[str, np.ndarray] = {
            "H": rng.uniform(-lim, lim, (self.bond_d, self.bond_d)).astype(np.float32),
            "R": rng.uniform(-lim, lim, (self.bond_d, self.bond_d)).astype(np.float32)}
        self._backend = backend
        self._last = None

    @property
    def H_s(self) -> np.ndarray:
        L = np.tril(self.variables["H"])
        return (L + L.T).astype(np.float32)                  # graph.pbtxt:9442-9605

    @property
    def Q(self) -> np.ndarray:
        R = self.variables["R"]
        RtR = (R.T @ R).astype(np.float32)                   # MatMul transpose_a, :13041
        return ((np.complex64(-1j) * self.H_s.astype(np.complex64) - (RtR / np.float32(2)).astype(np.complex64))
                * np.complex64(np.float32(self.delta_t))).astype(np.complex64)

    def _prepare(self, B, T, train):
        be = self._get_backend()
        be.legacy_set_params(self.variables["R"], self.Q, self.delta_t, B, T, train=train)
        return be

    def loss_per_clip(self, data=None) -> np.ndarray:
        return self.loss_per_clip_dev(data).detach().cpu().numpy()

    def _forward_entry(self, be):
        return be.legacy_forward

    @property
    def loss(self) -> np.float32:
        return np.float32(np.mean(self.loss_per_clip(), dtype=np.float32))

    def flat_size(self) -> int:
        """Length of the buffer grad_sums() returns (cmps_legacy_loss_bwd's layout)."""
        return layout.size(layout.legacy_grad_fields(self.bond_d))

    def grad_sums(self, data=None):
        be, audio, B, _ = self._scan(data, train=True)
        be.legacy_forward(audio, save_for_bwd=True)
        return be.legacy_backward(), B

    def chain_rule(self, flat_sums, global_batch: int, with_reg: bool = False):
        """(dQ, dR_direct) sums -> gradients w.r.t. H and R  (adjoint of Q = dt (-i H_s - R^T R / 2), H_s = L + L^T)."""
        g = layout.unpack(layout.legacy_grad_fields(self.bond_d), np.asarray(flat_sums, dtype=np.float64) / float(global_batch))
        Qbar, Rdir, loss = layout.join(g, "Q"), g["R"], g["loss_sum"]
        dt = float(np.float32(self.delta_t))
        R = self.variables["R"].astype(np.float64)
        Hs_bar = -dt * Qbar.imag
        M_bar = -(dt / 2.0) * Qbar.real
        gR = Rdir + R @ (M_bar + M_bar.T)
        gH = np.tril(Hs_bar + Hs_bar.T)
        return np.float32(loss), {"H": gH.astype(np.float32), "R": gR.astype(np.float32)}


class AudioMPS(PsiCMPS):
    """Legacy surface: ``AudioMPS(bond_d, dt, batch_size, data_iterator=..., mixed=...)``
    (training_estimators.py:43-45; ``AudioMPS(bond_d, delta_t=..., data_iterator=...)`` in
    notebooks/testing-AudioMPS.ipynb:268).  The class body no longer exists in the reference's model.py;
    PsiCMPS is its successor, so this wraps PsiCMPS with train.py's remaining hyper-parameters."""

    def __new__(cls, *args, arithmetic: str = "psi", **kwargs):
        # arithmetic="legacy": the model this surface originally named (LegacyAudioMPS)
        if arithmetic == "legacy":
            kwargs.pop("mixed", None)
            dt = kwargs.pop("delta_t", None)
            if dt is not None and len(args) < 2:
                kwargs["dt"] = dt
            kwargs.pop("hparams", None)
            return LegacyAudioMPS(*args, **kwargs)
        # mixed=True: the density-matrix model (RhoCMPS); a non-instance return skips AudioMPS.__init__
        names = ("bond_d", "dt", "batch_size", "data_iterator", "mixed")
        bound = dict(zip(names, args))
        bound.update(kwargs)
        if bound.get("mixed", False):
            hp = cls._hparams(bound["bond_d"], bound.get("dt"), bound.get("batch_size", 8), bound.get("delta_t"),
                              bound.get("hparams"))
            extra = {k: v for k, v in bound.items() if k not in names + ("delta_t", "hparams")}
            return RhoCMPS(hp, data_iterator=bound.get("data_iterator"), **extra)
        return super().__new__(cls)

    @staticmethod
    def _hparams(bond_d, dt, batch_size, delta_t, hparams):
        if dt is None:
            dt = delta_t
        if dt is None:
            raise TypeError("AudioMPS needs dt (or delta_t)")
        hp = hparams if hparams is not None else HParams()
        return HParams(**{**hp.values(), "bond_dim": int(bond_d), "delta_t": float(dt),
                          "minibatch_size": int(batch_size)})

    def __init__(self, bond_d, dt=None, batch_size=8, data_iterator=None, mixed=False, delta_t=None,
                 hparams: Optional[HParams] = None, arithmetic: str = "psi", **kwargs):
        hp = self._hparams(bond_d, dt, batch_size, delta_t, hparams)
        super().__init__(hp, data_iterator=data_iterator, **kwargs)
