"""Many models at once: a bank of M same-shape PsiCMPS (or RhoCMPS) models that train in one kernel launch per stage.

  reference          a sweep is a Python loop over models: a grid over --hparams (train.py:31) at minibatch_size = 8, bond_dim = 8
                     (train.py:41), several seeds of the random initialisation (model.py:36-50), one model per pitch (reader.py:9-66)
  PsiBank            M PsiCMPS models of one D, each initialised exactly as PsiCMPS(hparams_m, seed=seed_m)
  RhoBank            the same for the reference's other model (train.py:18-20, 50-53): M RhoCMPS models of one D and one initial_rank;
                     the device path uses cmps_rho_bank_* (D <= 32, 3 <= rank <= 32)
  BankTrainer        one optimiser step of every member: cmps_bank_set_params_dev, cmps_bank_loss_fwd / _bwd, cmps_bank_apply_step --
                     the plain kernels with a member grid dimension, so member m gets bit for bit what Trainer(device_step=True) gives
                     model m alone.  On a backend without the bank entries the trainer loops over plain steps of its members.

  class bank         ``classes=[...]``: member m models the clips labelled classes[m] (a model per pitch).  It trains on
                     ResidentDataset.class_batches ([M, B, T], one batch per member) and is judged as a classifier by
                     ``BankTrainer.evaluate_classifier`` (cmps_bank_classify_stats: accuracy, cross-entropy, confusion matrix).
                     ``BankTrainer.step_classifier`` trains its members against each other on ONE shared labelled batch
                     (ResidentDataset.labelled_batches; cmps_bank_classify_weights, cmps_bank_loss_bwd_weighted; PsiCMPS members).

Common to a bank: bond_dim, minibatch_size, sigma, delta_t, A, Adam's betas and epsilon.  Free per member: seed, learning_rate, h_reg, r_reg
and the data.  Every member is sampled, followed and scored at once through ``open_stream`` (a BankStream: cmps_bank_stream*; a RhoBank:
cmps_rho_bank_stream*), ``sample``, ``nll_per_step`` and ``classify``; for everything else a member is taken out as an ordinary model:
``BankTrainer.member(m)``.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, fields, replace
from typing import List, Optional, Sequence

import numpy as np

from .model import HParams, PsiCMPS, RhoCMPS
from .parallel import DataParallel
from .prior import log_prior_array, log_prior_json, log_prior_of, normalised_prior     # noqa: F401  (normalised_prior: imported from here)
from .resident import ResidentState
from .train import Trainer

MEMBER_KEYS = ("seed", "learning_rate", "h_reg", "r_reg")
CALIBRATION_FITS = {"temperature": 1, "prior": 2, "both": 3}        # cmps_bank_calibrate's `fit` bits
CALIBRATION_KEYS = ("temperature", "log_prior", "fit", "dataset", "clips", "T", "xent_before", "xent_after")     # bank.json's "calibration"


@dataclass
class CalibrationResult:
    """A temperature and a prior fitted on held-out clips (BankTrainer.calibrate), from theta and the record of cmps_bank_calibrate."""
    temperature: float             # 1 / kappa
    prior: np.ndarray              # float64 [M]: exp(log_prior - logsumexp(log_prior))
    log_prior: np.ndarray          # float64 [M]: c as the device left it (never shifted there)
    xent_before: float             # the held-out cross-entropy at the start values
    xent_after: float              # ... and at the returned ones: never above xent_before
    converged: bool
    at_bound: bool                 # the temperature sits on kappa_min or kappa_max, with the gradient pushing outwards
    unfitted: list                 # the classes without a used held-out clip: their prior kept its start value
    passes: int
    n_used: int
    n_unlabelled: int
    n_own_absent: int
    T: int                         # a temperature fitted on whole clips of T samples belongs to that T
    fit: str = "temperature"

    def line(self) -> str:
        return (f"temperature={self.temperature:.6g} xent_before={self.xent_before:.6g} xent_after={self.xent_after:.6g} "
                f"converged={self.converged} passes={self.passes} unfitted={len(self.unfitted)}")

    def scalars(self) -> dict:
        out = {f.name: getattr(self, f.name) for f in fields(self) if f.name not in ("prior", "log_prior")}
        out["prior"], out["log_prior"] = [float(p) for p in self.prior], log_prior_json(self.log_prior)
        return out

    def meta(self, dataset: Optional[str] = None) -> dict:
        """What bank.json keeps under "calibration"."""
        return {"temperature": float(self.temperature), "log_prior": log_prior_json(self.log_prior), "fit": self.fit, "dataset": dataset,
                "clips": int(self.n_used), "T": int(self.T), "xent_before": float(self.xent_before), "xent_after": float(self.xent_after)}


class PsiBank:
    """``members``: a list of dicts overriding ``seed``, ``learning_rate``, ``h_reg``, ``r_reg`` of ``hparams`` (any other key is a
    ValueError naming it).  ``models[m]`` is PsiCMPS(hparams_m, seed=seed_m); all of them share one backend."""

    MODEL = PsiCMPS
    MODEL_NAME = "psi_mps"        # --mps_model (train.py:18-20); written into a Rho bank's bank.json
    rank = 0                      # columns of rho_0 (RhoBank); 0: pure states

    def __init__(self, hparams: HParams, members: Sequence[dict], backend=None, classes: Optional[Sequence] = None,
                 label_key: Optional[str] = None):
        if len(members) < 1:
            raise ValueError("a bank needs at least one member")
        self.classes = None if classes is None else [c if isinstance(c, str) else int(c) for c in classes]     # member m models classes[m]
        self.class_counts = None            # clips per class of the training set, where somebody counted them (bank.json keeps them)
        self.label_key = label_key          # the TFRecord feature the classes are values of (bank.json keeps it for evaluate / sample)
        if self.classes is not None and (len(self.classes) != len(members) or len(set(self.classes)) != len(self.classes)):
            raise ValueError(f"a class bank needs one distinct class per member: {len(members)} members, classes {self.classes}")
        self.hparams = hparams
        self.overrides: List[dict] = []
        for m, ov in enumerate(members):
            ov = dict(ov)
            for key in ov:
                if key not in MEMBER_KEYS:
                    raise ValueError(f"member {m}: '{key}' cannot differ inside a bank (free per member: {', '.join(MEMBER_KEYS)})")
            self.overrides.append(ov)
        self.member_hparams = [replace(hparams, **{k: float(v) for k, v in ov.items() if k != "seed"}) for ov in self.overrides]
        self.seeds = [int(ov.get("seed", 0)) for ov in self.overrides]
        if backend is None:
            from .scan import HipScan       # raises if libcmps.so or the GPU is missing: no fallback
            backend = HipScan(int(hparams.bond_dim))
        self.backend = backend
        self.models = [self.MODEL(hp, seed=seed, backend=backend) for hp, seed in zip(self.member_hparams, self.seeds)]

    def __len__(self) -> int:
        return len(self.models)

    @property
    def bond_d(self) -> int:
        return int(self.hparams.bond_dim)

    def member_of(self, label) -> int:
        """The member that models class ``label`` of a class bank."""
        if self.classes is None:
            raise ValueError("member_of: this bank has no classes")
        label = label if isinstance(label, str) else int(label)
        if label not in self.classes:
            raise ValueError(f"member_of: no member models class {label!r} (classes: {self.classes})")
        return self.classes.index(label)

    # -- every member at once: stream, sample, score (cmps_bank_stream*, cmps_rho_bank_stream*) ---------------------------------
    def stream_backend(self):
        """A new backend of the bank's kind, D and variant: what a stream of the bank runs on."""
        be = self.backend
        if type(be).__name__ == "HipScan":
            return type(be)(self.bond_d, device=be.device, variant=be.variant)
        return type(be)(self.bond_d)

    def open_stream(self, num_paths, max_steps, temp=1, seed=None, device_noise=False, independent_noise=False, prior=None,
                    temperature=1.0, threshold=None):
        """``PsiCMPS.open_stream`` (RhoBank: ``RhoCMPS.open_stream`` without keep_states) for every member at once: a BankStream
        (audio_mps_amd/stream.py) of ``num_paths`` paths per member.  It runs on a backend of its own, so it never disturbs a trainer's workspace on the bank's shared one, and keeps the parameters
        the members have now.  By default member m, path b hears the noise ``models[m].open_stream(num_paths, ..., seed=seed)`` would
        give path b; ``independent_noise=True`` numbers the paths globally (g = m num_paths + b).  ``prior`` ([M] probabilities, normalised
        here; None: uniform), ``temperature`` and ``threshold`` are what the stream's ``score_posterior`` judges the members with."""
        from .stream import BankStream
        return BankStream(self, num_paths, max_steps, temp=temp, seed=seed, device_noise=device_noise, independent_noise=independent_noise,
                          prior=prior, temperature=temperature, threshold=threshold)

    def sample(self, n, length, temp=1, seed=None, prime=None, device_noise=False) -> np.ndarray:
        """``PsiCMPS.sample`` (RhoBank: ``RhoCMPS.sample``) of every member, [M, n, length] in the reference's convention (A * running sum
        of the sampled increments, zero at the hand-over behind a ``prime`` [T'], [1, T'] or [n, T']).  Every member hears the same noise."""
        steps = 0 if prime is None else self.MODEL._prime(prime, n).shape[1] - 1
        st = self.open_stream(n, steps + int(length), temp=temp, seed=seed, device_noise=device_noise)
        if prime is not None:
            st.follow(self.MODEL._prime(prime, n))
        st.generate(length)
        return st._raw

    def nll_per_step(self, clips, segment=None) -> np.ndarray:
        """``PsiCMPS.nll_per_step`` under every member, [M, B, T - 1]: one scored bank stream over ``clips`` [B, T], in segments of
        ``segment`` steps when given (the cut changes no bit)."""
        return self._scored(clips, segment, "nll_per_step")[0]

    def classify(self, clips):
        """M per-class generative models are a classifier: (best [B], total_nll [M, B]) -- the member under which each clip of ``clips``
        [B, T] is the most likely, and every member's loss of every clip."""
        _, st = self._scored(clips, None, "classify")
        return st.best(), st.total_nll

    def posterior_trace(self, clips, prior=None, temperature=1.0, threshold=None, segment=None, want_post=False):
        """``classify`` after every sample: one scored bank stream with one path per clip of ``clips`` [B, T], judged by
        ``BankStream.score_posterior`` in segments of ``segment`` steps when given (the cut changes no bit).  Returns a PosteriorTrace:
        ``best``, ``conf`` [B, T - 1] (``post`` [M, B, T - 1] with want_post) and ``decided_at``, ``decided_as`` [B] -- the step, counted
        from 0, at which the best member's probability first reached ``threshold``, and that member; -1 for a clip that never got there."""
        from .stream import PosteriorTrace, as_clips, segments
        clips = as_clips(clips, "posterior_trace")
        B, N = clips.shape[0], clips.shape[1] - 1
        cuts = segments(N, segment)
        st = self.open_stream(B, N, prior=prior, temperature=temperature, threshold=threshold)
        parts = [st.score_posterior(clips[:, lo:hi], want_post=want_post) for lo, hi in cuts]
        cat = lambda key: np.concatenate([getattr(p, key) for p in parts], axis=-1)                 # noqa: E731
        return PosteriorTrace(cat("best"), cat("conf"), cat("post") if want_post else None, None, parts[-1].decided_at, parts[-1].decided_as)

    def _scored(self, clips, segment, who):
        from .stream import as_clips, segments
        clips = as_clips(clips, who)
        B, N = clips.shape[0], clips.shape[1] - 1
        cuts = segments(N, segment)
        st = self.open_stream(B, N)
        return np.concatenate([st.score(clips[:, lo:hi]) for lo, hi in cuts], axis=-1), st


class RhoBank(PsiBank):
    """``models[m]`` is RhoCMPS(hparams_m, seed=seed_m); ``hparams.initial_rank`` (None: bond_dim) is common to the bank."""
    MODEL = RhoCMPS
    MODEL_NAME = "rho_mps"

    def __init__(self, hparams: HParams, members: Sequence[dict], backend=None, classes: Optional[Sequence] = None,
                 label_key: Optional[str] = None):
        super().__init__(hparams, members, backend, classes, label_key)
        self.rank = int(self.models[0].rank_rho_0)


RHO_BANK_ENTRIES = ("rho_bank_set_state_dev", "rho_bank_forward", "rho_bank_backward", "rho_bank_apply_step")


class BankTrainer(ResidentState):
    """One optimiser step of every member of a PsiBank or RhoBank per ``step``.  Every member keeps an ordinary Trainer (its model, its Adam slots,
    its checkpoint format); on a backend with the bank entries (HipScan) variables, Adam slots and effective parameters of all members
    live on the device as [M, ...] arrays between steps and come back with ``sync_to_host`` (``member`` and ``save`` do so).  While that
    state is live the bank is every member model's device owner by the protocol a Trainer(device_step=True) follows (ResidentState,
    audio_mps_amd/resident.py): reading ``bank.models[m].variables`` brings the state back first, and assigning an entry brings it back
    and drops it, so the next step starts from the host values of every member."""

    STACKED = True                # (SYNC_CLEAN stays off: sync_to_host() without a step since the last one touches no member)

    def __init__(self, bank: PsiBank, dp: Optional[DataParallel] = None):
        if dp is not None and dp.world_size > 1:
            raise ValueError("BankTrainer: multi-rank training of a bank is not supported (world size must be 1)")
        self.bank = bank
        be = bank.backend
        self.rank = int(bank.rank)    # 0: PsiCMPS members; else the columns of every RhoCMPS member (selects the layouts and the rho_bank_* entries)
        entries = RHO_BANK_ENTRIES if self.rank else ("bank_set_params_dev", "bank_forward", "bank_backward", "bank_apply_step")
        self.native = all(hasattr(be, name) for name in entries)
        if self.native:               # the backend's operations of this kind of bank, bound once: every call below goes through them
            setter, self._forward, self._backward, apply_step = (getattr(be, name) for name in entries)
            m0, r = bank.models[0], self.rank
            if r:
                self._configure = lambda st, B, T, train: setter(st["params"], st["phi"], r, m0.sigma, m0.delta_t, B, T, train=train)
                self._apply_step = lambda st, grad, *a: apply_step(st["vars"], st["m"], st["v"], grad, r, *a, st["params"], st["phi"], st["losses"])
            else:
                self._configure = lambda st, B, T, train: setter(st["params"], m0.sigma, m0.delta_t, B, T, train=train)
                self._apply_step = lambda st, grad, *a: apply_step(st["vars"], st["m"], st["v"], grad, *a, st["params"], st["losses"])
        plain_device = type(be).__name__ == "HipScan"
        self.trainers = [Trainer(model, hp, device_step=plain_device and not self.native)
                         for model, hp in zip(bank.models, bank.member_hparams)]
        self.global_step = 0
        self.objective = None         # a dict the caller sets for a run that is not generative (train --bank_objective): kept in bank.json
        self.calibration = None       # a dict (CALIBRATION_KEYS) once `calibrate` ran or `restore` found one: kept in bank.json
        self.last = None            # the last synchronised step's per-member losses: {"model_loss": [M], "total_loss": [M]}
        self._resident([(tr.model, tr.opt) for tr in self.trainers], bank.bond_d, self.rank)

    def __len__(self) -> int:
        return len(self.trainers)

    # -- device-resident state of the native path ([M, ...] rows of ResidentState's tensors, and "hyper") ---------------
    def _device_state(self):
        if self._dev is None:
            import torch
            be = self.bank.backend
            hyper = np.array([[tr.opt.lr, tr.model.h_reg, tr.model.r_reg, float(tr.model._c_r), float(tr.model._c_h)] for tr in self.trainers],
                             dtype=np.float64)
            self._upload(be.device)["hyper"] = torch.from_numpy(hyper).to(be.device)       # uploaded once: the device forms lr_t itself
            self._apply(None, 1)                                      # effective parameters of the current variables
        return self._dev

    def _apply(self, grad_sums, global_batch):
        st, o = self._dev, self.trainers[0].opt
        t = max(o.t, 1)
        self._apply_step(st, grad_sums, global_batch, math.sqrt(1.0 - o.b2 ** t), 1.0 - o.b1 ** t, o.b1, o.b2, o.eps, st["hyper"], True)

    # -- one step -------------------------------------------------------------------------------------
    def step(self, data, sync: bool = True) -> dict:
        """``data`` [B, T] (one batch shared by every member) or [M, B, T] (one per member).  Returns per-member ``model_loss`` and
        ``total_loss`` ([M] arrays), or -- ``sync=False`` -- ``losses_dev`` [M, 2] where the step left it."""
        M = len(self.trainers)
        nd = data.dim() if hasattr(data, "dim") else np.ndim(data)
        if nd not in (2, 3) or (nd == 3 and len(data) != M):
            raise ValueError(f"data must be [B, T] or [M, B, T] with M = {M}")
        if self.native:
            out = self._step_native(data)
        else:
            recs = [tr.step(data if nd == 2 else data[m], sync=True) for m, tr in enumerate(self.trainers)]
            out = {"losses_dev": np.array([[r["model_loss"], r["total_loss"]] for r in recs], dtype=np.float32)}
        self.global_step += 1
        out["global_step"] = self.global_step
        if sync:
            lo = out.pop("losses_dev")
            lo = lo.cpu().numpy() if hasattr(lo, "cpu") else lo
            out.update(model_loss=lo[:, 0].copy(), total_loss=lo[:, 1].copy())
            self.last = out
        return out

    def _step_native(self, data):
        st = self._device_state()
        audio = self.bank.models[0]._to_device(data)
        B, T = audio.shape[-2:]
        self._configure(st, int(B), int(T), True)
        self._forward(audio, save_for_bwd=True)
        flat = self._backward()
        self._finish_step(flat, int(B))
        return {"losses_dev": st["losses"]}

    def _finish_step(self, grad_sums, B):
        """The optimiser tail of a native step: every member's Adam step and step count advance, the device applies the step, and the
        resident state is newer than the host's."""
        for tr in self.trainers:
            tr.opt.t += 1
            tr.global_step += 1
        self._apply(grad_sums, B)
        self._mark_dirty()

    def step_classifier(self, data, labels, gen_weight: float = 0.0, disc_weight: float = 1.0, temperature: float = 1.0,
                        sync: bool = True) -> dict:
        """One step of a class bank trained as a classifier: ``data`` [B, T], ONE batch shared by every member, and ``labels`` [B], the
        member each clip belongs to (``dataset.class_index(bank.classes)``; outside [0, M): the clip is skipped).  Every member descends
        sum_b (gen_weight * loss[label_b, b] + disc_weight * xent_b) / B with p(m | clip) = softmax(-loss / temperature), the objective
        of cmps_bank_classify_weights: a shared-batch forward, the weights, cmps_bank_loss_bwd_weighted and the optimiser step of
        ``step``.  Returns what ``step`` returns -- ``model_loss`` [M] is each member's weighted loss sum / B -- and ``xent`` (the mean over
        the used clips), ``used``, ``unlabelled`` and ``own_absent``; with ``sync=False`` ``losses_dev`` and ``record_dev`` instead."""
        import torch
        be = self.bank.backend
        if self.bank.classes is None:
            raise ValueError("step_classifier needs a class bank (PsiBank(..., classes=))")
        if self.rank:
            raise ValueError("step_classifier: a RhoBank has no weighted reverse pass (cmps_bank_loss_bwd_weighted is for PsiCMPS members)")
        if not (self.native and hasattr(be, "classify_weights")):
            raise ValueError("step_classifier needs the backend's bank entries and classify_weights (the native path): "
                             f"{type(be).__name__} has none")
        if not (temperature > 0.0 and math.isfinite(temperature)):
            raise ValueError("step_classifier: temperature must be finite and positive")
        nd = data.dim() if hasattr(data, "dim") else np.ndim(data)
        if nd != 2:
            raise ValueError("step_classifier: data must be [B, T], one batch shared by every member")
        st = self._device_state()
        audio = self.bank.models[0]._to_device(data)
        B, T = audio.shape[-2:]
        if not isinstance(labels, torch.Tensor):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32))
        labels = labels.to(device=audio.device, dtype=torch.int32).contiguous()
        if labels.dim() != 1 or int(labels.numel()) != int(B):
            raise ValueError(f"step_classifier: labels must be [B] with B = {int(B)}")
        self._configure(st, int(B), int(T), True)
        loss = self._forward(audio, save_for_bwd=True)
        weights, record = be.classify_weights(loss, labels, 1.0 / float(temperature), float(gen_weight), float(disc_weight))
        flat = self._backward(weights=weights)
        self._finish_step(flat, int(B))
        self.global_step += 1
        out = {"global_step": self.global_step}
        if not sync:
            out.update(losses_dev=st["losses"], record_dev=record)
            return out
        lo = st["losses"].cpu().numpy()
        rec = be.read_classify_weights_record(record)
        out.update(model_loss=lo[:, 0].copy(), total_loss=lo[:, 1].copy(),
                   xent=rec["sum_xent"] / rec["n_used"] if rec["n_used"] else float("nan"),
                   used=rec["n_used"], unlabelled=rec["n_unlabelled"], own_absent=rec["n_own_absent"])
        self.last = out
        return out

    def best(self) -> int:
        """The member with the lowest last ``model_loss`` among the finite ones."""
        if self.last is None:
            raise RuntimeError("best() needs a synchronised step first")
        loss = np.asarray(self.last["model_loss"], dtype=np.float64)
        if not np.isfinite(loss).any():
            raise RuntimeError("best(): no member has a finite loss")
        return int(np.argmin(np.where(np.isfinite(loss), loss, np.inf)))

    def member(self, m: int):
        """Member ``m`` as an ordinary PsiCMPS (RhoBank: RhoCMPS) holding its current variables: sample, open_stream, evaluate and save work on it as on any
        model (its scans reconfigure the shared backend; the next bank step configures it again)."""
        self.sync_to_host()
        return self.trainers[m].model

    def open_stream(self, num_paths, max_steps, temp=1, seed=None, device_noise=False, independent_noise=False, prior=None,
                    temperature=1.0, threshold=None):
        """``PsiBank.open_stream`` on the members' current variables: the device-resident state comes back first."""
        self.sync_to_host()
        return self.bank.open_stream(num_paths, max_steps, temp=temp, seed=seed, device_noise=device_noise, independent_noise=independent_noise,
                                     prior=prior, temperature=temperature, threshold=threshold)

    # -- held-out evaluation ------------------------------------------------------------------------------
    def _heldout_pass(self, dataset, minibatch_size, T, who):
        """One ordered pass over ``dataset`` (a ResidentDataset) with one bank forward per shared batch: (T, an iterator of (first_id,
        loss [M, B]) on the device).  The backend is configured here, once, for the largest batch; a backend without the bank entries
        runs its members one after the other.  Forward scans only: no optimiser state, no Adam step and no random stream is touched."""
        import torch
        from .evaluate import pass_shape
        mb, T, B_max = pass_shape(self.bank.backend, dataset, minibatch_size, self.bank.hparams.minibatch_size, T)
        if self.native:
            self._configure(self._device_state(), B_max, T, False)
            forward = lambda batch: self._forward(batch, save_for_bwd=False)                        # noqa: E731
        else:
            def forward(batch):
                rows = [tr.model._forward_entry(tr.model._prepare(B_max, T, train=False))(batch, save_for_bwd=False).clone() for tr in self.trainers]
                return torch.stack(rows)

        def batches():
            first_id = None
            for first_id, batch in dataset.ordered(mb, T):
                yield first_id, forward(batch)
            if first_id is None:
                raise ValueError(f"{who}: the dataset yielded no batch")
        return T, batches()

    def evaluate(self, dataset, minibatch_size: Optional[int] = None, T: Optional[int] = None, keep_losses: bool = False):
        """Every member's loss over every clip of ``dataset`` (a ResidentDataset): a list of EvalResult.  The batches are shared; the bank
        forward scores them for all members at once and cmps_loss_stats folds every member's row into its own record."""
        if not self.native:
            return [tr.evaluate(dataset, minibatch_size, T, keep_losses) for tr in self.trainers]
        import torch
        from .evaluate import EvalResult
        be, M = self.bank.backend, len(self.trainers)
        T, batches = self._heldout_pass(dataset, minibatch_size, T, "evaluate")
        stats, kept = [None] * M, [[] for _ in range(M)]
        for first_id, loss in batches:
            for m in range(M):
                stats[m] = be.loss_stats(loss[m], first_id, stats[m], reset=stats[m] is None)
                if keep_losses:
                    kept[m].append(loss[m])
        return [EvalResult.from_stats(be.read_stats(stats[m]), T, torch.cat(kept[m]).cpu().numpy() if keep_losses else None) for m in range(M)]

    def evaluate_classifier(self, dataset, minibatch_size: Optional[int] = None, T: Optional[int] = None, keep_best: bool = False):
        """The class bank judged as a classifier over every clip of ``dataset`` (a ResidentDataset; its labels, where it has some, are
        looked up in ``bank.classes``): a ClassifierResult.  One pass of ``dataset.ordered``: the batches are shared, every batch costs ONE
        bank forward and ONE cmps_bank_classify_stats launch, and the record comes back ONCE at the end (``keep_best``: and with it
        every clip's decision, ``result.best`` [n_clips], -1 where no member gave a finite loss)."""
        import torch
        from .evaluate import ClassifierResult
        be = self.bank.backend
        if self.bank.classes is None:
            raise ValueError("evaluate_classifier needs a class bank (PsiBank / RhoBank(..., classes=))")
        if not (hasattr(be, "classify_stats") and hasattr(be, "read_classify_stats")):
            raise ValueError("evaluate_classifier needs a backend that judges the members' losses on the device (classify_stats): "
                             f"{type(be).__name__} has none")
        T, batches = self._heldout_pass(dataset, minibatch_size, T, "evaluate_classifier")
        labels = dataset.class_index(self.bank.classes) if dataset.labels is not None else None
        best = torch.empty(dataset.n_clips, dtype=torch.int32, device=dataset.clips.device) if keep_best else None
        stats = None
        for first_id, loss in batches:
            B = int(loss.shape[1])
            stats = be.classify_stats(loss, None if labels is None else labels[first_id:first_id + B], first_id, stats, reset=stats is None,
                                      best=None if best is None else best[first_id:first_id + B])
        return ClassifierResult.from_stats(be.read_classify_stats(stats, len(self.trainers)), self.bank.classes, T,
                                           best.cpu().numpy() if keep_best else None)

    def _heldout_losses(self, dataset, minibatch_size, T, who):
        """`evaluate_classifier`'s ordered pass with every batch's [M][B] losses kept side by side on the device: (loss [M, N], labels
        [N] int32, the labels on the host, T)."""
        import torch
        be = self.bank.backend
        if self.bank.classes is None:
            raise ValueError(f"{who} needs a class bank (PsiBank / RhoBank(..., classes=))")
        if not (hasattr(be, "bank_calibrate") and hasattr(be, "read_calibrate_record")):
            raise ValueError(f"{who} needs a backend that fits on the device (bank_calibrate): {type(be).__name__} has none")
        if dataset.labels is None:
            raise ValueError(f"{who}: the dataset has no labels")
        T, batches = self._heldout_pass(dataset, minibatch_size, T, who)
        host_labels = dataset.class_positions(self.bank.classes)
        labels = torch.from_numpy(host_labels).to(dataset.clips.device)
        kept = None
        for first_id, loss in batches:
            if kept is None:
                kept = torch.empty((len(self.trainers), int(dataset.n_clips)), dtype=torch.float32, device=loss.device)
            kept[:, first_id:first_id + int(loss.shape[1])].copy_(loss)                             # device to device
        return kept, labels, host_labels, T

    def calibrate(self, dataset, minibatch_size: Optional[int] = None, T: Optional[int] = None, fit: str = "temperature",
                  temperature: float = 1.0, prior=None, tol: float = 1e-9, max_iter: int = 200, kappa_min: float = 1e-6,
                  kappa_max: float = 1e6) -> CalibrationResult:
        """Fit the temperature and (or) the prior of p_m ~ prior_m exp(-loss_m / temperature) on every labelled clip of ``dataset`` (a
        ResidentDataset of HELD-OUT clips): `evaluate_classifier`'s ordered pass with the [M][B] losses of every batch copied into one
        resident [M][N] tensor, then ONE cmps_bank_calibrate call and ONE download (a second one, of the own members' losses, only where a class
        lost its last clip to a non-finite loss and ``unfitted`` has to name it).  ``fit``: "temperature", "prior" or "both";
        ``temperature`` and ``prior`` (None: uniform, "empirical": the class counts, or [M] probabilities) are the start.  The result is
        kept in ``self.calibration`` (and by ``save`` in bank.json).  Like `evaluate_classifier` it runs forward scans only: the training
        steps after it are bit for bit those of a run without it."""
        if fit not in CALIBRATION_FITS:
            raise ValueError(f"calibrate: fit is one of {', '.join(CALIBRATION_FITS)}, not {fit!r}")
        res = self._calibrate(dataset, minibatch_size, T, CALIBRATION_FITS[fit], fit, temperature, prior, tol, max_iter, kappa_min, kappa_max,
                              "calibrate")
        self.calibration = res.meta()
        return res

    def cross_entropy(self, dataset, temperature: float = 1.0, prior=None, minibatch_size: Optional[int] = None, T: Optional[int] = None,
                      log_prior=None) -> float:
        """The held-out cross-entropy of the bank under a GIVEN temperature and prior: `calibrate`'s pass and cmps_bank_calibrate with
        zero iterations (cmps_bank_classify_stats knows temperature 1 and the uniform prior only).  ``log_prior`` ([M], finite or -inf)
        instead of ``prior`` is taken as it is: a saved calibration's."""
        if log_prior is not None:
            if prior is not None:
                raise ValueError("cross_entropy: give prior or log_prior, not both")
            log_prior = log_prior_array(log_prior).reshape(-1)
            if log_prior.shape != (len(self.trainers),) or np.any(np.isnan(log_prior)) or np.any(log_prior == np.inf):
                raise ValueError(f"cross_entropy: log_prior must be {len(self.trainers)} values, each finite or -inf")
        return self._calibrate(dataset, minibatch_size, T, 0, "none", temperature, prior, 1e-9, 0, 1e-6, 1e6, "cross_entropy",
                               log_prior).xent_before

    def _calibrate(self, dataset, minibatch_size, T, fit_bits, fit, temperature, prior, tol, max_iter, kappa_min, kappa_max, who,
                   log_prior=None):
        import torch
        if not (math.isfinite(temperature) and temperature > 0.0):
            raise ValueError(f"{who}: temperature must be finite and positive")
        if log_prior is None:
            log_prior = log_prior_of(prior, len(self.trainers), self.bank.class_counts, who)
        c0 = np.zeros(len(self.trainers), dtype=np.float64) if log_prior is None else log_prior             # (None: uniform)
        loss, labels, host_labels, T = self._heldout_losses(dataset, minibatch_size, T, who)
        known = host_labels >= 0
        counts = np.bincount(host_labels[known], minlength=len(self.trainers))
        if np.any((counts > 0) & (np.asarray(c0) == -math.inf)):     # its clips would have probability zero: the cross-entropy is +inf
            zero = [self.bank.classes[m] for m in range(len(counts)) if counts[m] > 0 and c0[m] == -math.inf]
            raise ValueError(f"{who}: the prior is zero for {zero}, of which the dataset holds clips")
        be, M = self.bank.backend, len(self.trainers)
        theta, rec = be.read_calibrate_record(be.bank_calibrate(loss, labels, fit_bits, 1.0 / float(temperature), c0, tol, max_iter, kappa_min,
                                                                kappa_max))
        if rec["flags"] & 8:
            raise ValueError(f"{who}: no clip of the dataset carries a label of the bank's classes with a finite loss under its own member "
                             f"({rec['n_unlabelled']} unlabelled, {rec['n_own_absent']} with the own member absent)")
        # the classes without a used clip, from the labels the host holds; where a class lost its last clip to a non-finite loss of its
        # own member (the device counted more unfitted members than the labels show) the own losses come down too, a second download
        if rec["n_own_absent"] and int(np.sum(counts == 0)) != rec["n_unfitted"]:     # a class lost its last clip to a non-finite loss: look
            own = loss[labels.clamp(min=0).to(torch.int64), torch.arange(loss.shape[1], device=loss.device)].cpu().numpy()
            counts = np.bincount(host_labels[known & np.isfinite(own)], minlength=M)
        unfitted = [self.bank.classes[m] for m in range(M) if counts[m] == 0]
        return CalibrationResult(temperature=1.0 / float(theta[0]), prior=normalised_prior(theta[1:]), log_prior=theta[1:].copy(),
                                 xent_before=rec["xent_start"], xent_after=rec["xent_end"], converged=bool(rec["flags"] & 1),
                                 at_bound=bool(rec["flags"] & 6), unfitted=unfitted, passes=rec["passes"], n_used=rec["n_used"],
                                 n_unlabelled=rec["n_unlabelled"], n_own_absent=rec["n_own_absent"], T=int(T), fit=fit)

    # -- checkpoints: model.<m>.ckpt.npz in the format of Trainer.save, bank.json with the members' overrides -----------
    @staticmethod
    def member_path(directory: str, m: int) -> str:
        return os.path.join(directory, f"model.{m}.ckpt.npz")

    def save(self, directory: str):
        self.sync_to_host()
        os.makedirs(directory, exist_ok=True)
        for m, tr in enumerate(self.trainers):
            tr.save(self.member_path(directory, m))
        meta = {"members": self.bank.overrides, "adam_step": int(self.trainers[0].opt.t), "global_step": int(self.global_step)}
        if self.rank:                 # (a PsiCMPS bank's file stays as it was)
            meta["model"] = self.bank.MODEL_NAME
        if self.bank.classes is not None:     # (and so does the file of a bank without classes)
            meta["label_key"], meta["classes"] = self.bank.label_key, self.bank.classes
        if getattr(self.bank, "class_counts", None) is not None:      # clips per class of the training set: an empirical prior
            meta["class_counts"] = [int(c) for c in self.bank.class_counts]
        if self.objective is not None:        # (and of a generatively trained one)
            meta["objective"] = self.objective
        if self.calibration is not None:      # (and of a bank nobody calibrated)
            meta["calibration"] = self.calibration
        tmp = os.path.join(directory, "bank.json.tmp")
        with open(tmp, "w") as f:
            json.dump(meta, f)
        os.replace(tmp, os.path.join(directory, "bank.json"))

    def restore(self, directory: str) -> bool:
        path = os.path.join(directory, "bank.json")
        if not os.path.exists(path):
            return False
        with open(path) as f:
            meta = json.load(f)
        if meta.get("model", PsiBank.MODEL_NAME) != self.bank.MODEL_NAME:
            raise ValueError(f"{path} was written by a bank of {meta.get('model', PsiBank.MODEL_NAME)} models, this bank holds {self.bank.MODEL_NAME}")
        if meta["members"] != json.loads(json.dumps(self.bank.overrides)):
            raise ValueError(f"{path} was written by a bank of other members: {meta['members']}")
        if meta.get("classes") != self.bank.classes:
            raise ValueError(f"{path} was written by a bank of classes {meta.get('classes')}, this bank's are {self.bank.classes}")
        self.drop_device_state()      # the device-resident copy is rebuilt from the restored state
        for m, tr in enumerate(self.trainers):
            if not tr.restore(self.member_path(directory, m)):
                raise FileNotFoundError(self.member_path(directory, m))
        self.global_step = int(meta["global_step"])
        self.calibration = meta.get("calibration")
        return True


def parse_bank_hparams(spec: str) -> List[dict]:
    """``--bank_hparams "learning_rate=1e-3,3e-3;r_reg=0.1,1"`` -> the Cartesian grid as member overrides, the first name varying slowest:
    [{lr 1e-3, r_reg 0.1}, {lr 1e-3, r_reg 1}, {lr 3e-3, r_reg 0.1}, {lr 3e-3, r_reg 1}]."""
    grid: List[dict] = [{}]
    for item in spec.split(";"):
        if not item.strip():
            continue
        name, _, values = item.partition("=")
        name = name.strip()
        if name not in MEMBER_KEYS or name == "seed":
            raise ValueError(f"--bank_hparams: '{name}' cannot differ inside a bank (learning_rate, h_reg, r_reg)")
        vals = [float(v) for v in values.split(",") if v.strip()]
        if not vals:
            raise ValueError(f"--bank_hparams: no values for '{name}'")
        grid = [{**g, name: v} for g in grid for v in vals]
    return grid


def bank_members(seed: int, n_seeds: int, spec: str) -> List[dict]:
    """The members of ``--bank N --bank_hparams SPEC``: every seed of seed .. seed + N - 1 once per grid point (grid point varying slowest)."""
    grid = parse_bank_hparams(spec) if spec else [{}]
    return [{**g, "seed": seed + s} for g in grid for s in range(max(int(n_seeds), 1))]
