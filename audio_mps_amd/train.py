"""Trainer mirroring /root/reference/train.py for the pure-state model.

  hparams            train.py:41-44      (same names, same defaults, ``--hparams=a=b,...`` override)
  data               train.py:46-47      get_audio(...)
  model              train.py:49-53      PsiCMPS(hparams, data_iterator=data)
  total loss         train.py:55-60      loss + h_reg * sum(freqs^2) + r_reg * sum(|R|^2)   (effective R, freqs)
  optimiser          train.py:88-89      tf.train.AdamOptimizer(learning_rate).minimize(total_loss, global_step)
  loop / checkpoints train.py:93-94      tf.contrib.training.train(..., save_checkpoint_secs=60, logdir=...)

The TensorBoard summaries (train.py:62-85: scalars, audio, histogram, tfplot images, model.sample) are
not part of the hot path; the scalar ones are returned by ``Trainer.step`` as a dict.
Run:  python -m audio_mps_amd.train --dataset=damped_sine --hparams=bond_dim=32,minibatch_size=64
(under torchrun for several GPUs: the batch is sharded over ranks, one RCCL all-reduce per step).
``--device_data`` produces every batch on the device instead of on the host (audio_mps_amd/device_data.py): a TFRecord dataset is uploaded
once and gathered from in the host pipeline's order, damped_sine is generated there.
``--eval_dataset NAME --eval_every N`` evaluates a held-out set every N steps and after the last one (Trainer.evaluate,
audio_mps_amd/evaluate.py): a line on the console, a JSON line in {logdir}/eval.jsonl, and model.best.ckpt.npz when the mean improves.
``--bank N`` and ``--bank_hparams "learning_rate=1e-3,3e-3;r_reg=0.1,1"`` train many models of --mps_model at once (audio_mps_amd/bank.py): N seeds,
the Cartesian grid, or every seed once per grid point; one kernel launch per stage serves all of them, every member sees the same batch,
and the checkpoints are {logdir}/model.<m>.ckpt.npz (each loads in audio_mps_amd.sample / .evaluate) next to bank.json.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from collections import deque
from typing import Dict, Optional

import numpy as np

from . import layout
from .layout import VAR_ORDER  # noqa: F401  (bench.py imports it from here)
from .model import HParams, PsiCMPS, RhoCMPS
from .parallel import DataParallel
from .resident import ResidentState


class AdamOptimizer:
    """tf.train.AdamOptimizer (train.py:89; legacy graph: beta1 0.9, beta2 0.999, eps 1e-8,
    logging/graph.pbtxt:32102-32192): lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t);
    m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  var -= lr_t * m / (sqrt(v) + eps)."""

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon
        self.t = 0
        self.m: Dict[str, np.ndarray] = {}
        self.v: Dict[str, np.ndarray] = {}

    def apply_gradients(self, variables: Dict[str, np.ndarray], grads: Dict[str, np.ndarray]):
        self.t += 1
        lr_t = self.lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for name in sorted(grads):
            g = np.asarray(grads[name], dtype=np.float32)
            if name not in self.m:
                self.m[name] = np.zeros_like(g)
                self.v[name] = np.zeros_like(g)
            m = self.m[name] = (self.b1 * self.m[name] + (1.0 - self.b1) * g).astype(np.float32)
            v = self.v[name] = (self.b2 * self.v[name] + (1.0 - self.b2) * g * g).astype(np.float32)
            variables[name] = (variables[name] - np.float32(lr_t) * m / (np.sqrt(v) + np.float32(self.eps))).astype(np.float32)

    def state_dict(self):
        return {"t": self.t, **{f"m/{k}": v for k, v in self.m.items()}, **{f"v/{k}": v for k, v in self.v.items()}}

    def load_state_dict(self, sd):
        self.t = int(sd["t"])
        self.m = {k[2:]: np.asarray(v) for k, v in sd.items() if k.startswith("m/")}
        self.v = {k[2:]: np.asarray(v) for k, v in sd.items() if k.startswith("v/")}


class Trainer(ResidentState):
    """One optimiser step = parameter tables, forward scan, reverse scan, (all-reduce), chain rule, Adam.

    ``device_step=False``: the gradient sums come to the host, chain rule (model.chain_rule) and Adam (AdamOptimizer) run in
    numpy, the parameters are uploaded again -- the tested reference implementation of the optimiser half.
    ``device_step=True`` (PsiCMPS or RhoCMPS on the HIP backend): variables, Adam slots and effective parameters (for RhoCMPS the
    columns of rho_0 as well) live on the GPU and cmps_psi_apply_step / cmps_rho_apply_step does the optimiser half there; a step
    issues no device -> host copy.  ``step`` then returns the
    losses as a 2-element device tensor under "losses_dev" unless ``sync=True``; ``sync_to_host()`` brings variables and
    Adam state back (checkpoints, sampling, inspection).  That state, its upload and download and the model's way to it (reading
    model.variables syncs, assigning an entry drops it) are ResidentState's (audio_mps_amd/resident.py)."""

    HISTORY = 4096                # step records kept (a long run must not grow without bound)
    SYNC_CLEAN = True             # sync_to_host() after a synced step, or before any, still copies (save: explicit zero Adam slots)

    def __init__(self, model: PsiCMPS, hparams: HParams, dp: Optional[DataParallel] = None, device_step: bool = False):
        self.model = model
        self.hparams = hparams
        self.dp = dp if dp is not None else DataParallel()
        self.opt = AdamOptimizer(hparams.learning_rate)
        self.global_step = 0
        self.history = deque(maxlen=self.HISTORY)   # the dict of every step (the scalar summaries of train.py:62-66)
        self.device_step = bool(device_step)
        self._resident([(model, self.opt)], model.bond_d, self._rank())    # _dev: flat "vars", "m", "v", "params", "losses" (RhoCMPS: + "phi")
        if self.device_step and not isinstance(model, (PsiCMPS, RhoCMPS)):
            raise ValueError("device_step: the device-resident optimiser step exists for PsiCMPS or RhoCMPS")

    # -- host reference path ----------------------------------------------------------------------
    def step(self, data=None, sync: bool = True, global_batch: Optional[int] = None) -> dict:
        """``data``: this rank's shard [B_local, T] (or None to use model.data_iterator).  An empty shard (a short final batch
        with fewer clips than ranks) skips the scan and contributes zeros to the all-reduce."""
        if self.device_step:
            return self._step_device(data, sync, global_batch)
        if data is not None and not callable(data) and len(data) == 0:
            import torch
            # sized from the MODEL (RhoCMPS appends its column cotangents: a shorter buffer here would be a size mismatch in the
            # all-reduce -- ADVICE r3), not from what an earlier call happened to leave behind
            dev = getattr(self.model._get_backend(), "device", None)
            flat = torch.zeros(self.model.flat_size(), dtype=torch.float32, device=dev if dev is not None else "cpu")
            b_local = 0
        else:
            flat, b_local = self.model.grad_sums(data)
        host, b_global = self.dp.allreduce_sums(flat, b_local)
        if global_batch is not None:
            b_global = int(global_batch)
        total, grads = self.model.chain_rule(host, max(b_global, 1), with_reg=True)       # train.py:55-60
        model_loss = layout.unpack_grad(host, self.model.bond_d)["loss_sum"] / max(b_global, 1)    # (RhoCMPS's tail sits behind it)
        self.opt.apply_gradients(self.model.variables, grads)                     # train.py:89
        self.global_step += 1
        out = {"model_loss": float(model_loss), "total_loss": float(total), "global_step": self.global_step,
               "global_batch": b_global}
        self.history.append(out)
        return out

    # -- device-resident path ---------------------------------------------------------------------
    def _rank(self) -> int:
        """0 for PsiCMPS; RhoCMPS: the number of columns of rho_0 (selects the variable layout and the rho entry points)."""
        return int(self.model.rank_rho_0) if isinstance(self.model, RhoCMPS) else 0

    def _device_state(self):
        if self._dev is None:
            self._upload(self.model._get_backend().device)
            self._apply(None, 1)                                   # effective parameters of the current variables
        return self._dev

    def _apply(self, grad_sums, global_batch):
        st, m, o = self._dev, self.model, self.opt
        lr_t = o.lr * math.sqrt(1.0 - o.b2 ** max(o.t, 1)) / (1.0 - o.b1 ** max(o.t, 1))
        be, rank = m._get_backend(), self._rank()
        if rank:
            be.rho_apply_step(st["vars"], st["m"], st["v"], grad_sums, rank, global_batch, lr_t, o.b1, o.b2, o.eps,
                              m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), True, st["params"], st["phi"], st["losses"])
        else:
            be.apply_step(st["vars"], st["m"], st["v"], grad_sums, global_batch, lr_t, o.b1, o.b2, o.eps,
                          m.h_reg, m.r_reg, float(m._c_r), float(m._c_h), True, st["params"], st["losses"])

    def _step_device(self, data, sync, global_batch):
        import torch
        m = self.model
        st = self._device_state()
        be = m._get_backend()
        audio = m._to_device(m._batch(data))
        b_local, T = audio.shape
        rank = self._rank()
        if b_local > 0 and rank:                                   # (RhoCMPS._prepare: the main workspace holds the tables only)
            be.set_params_dev(st["params"], m.sigma, m.delta_t, b_local, T, train=False)
            be.rho_set_state_dev(st["phi"], rank, b_local, T, train=True)
            be.rho_forward(audio, save_for_bwd=True)
            flat = be.rho_backward()
        elif b_local > 0:
            be.set_params_dev(st["params"], m.sigma, m.delta_t, b_local, T, train=True)
            be.forward(audio, save_for_bwd=True)
            flat = be.backward()
        else:
            flat = torch.zeros(m.flat_size(), dtype=torch.float32, device=be.device)
        if global_batch is None:                                   # known without communication: the reference's batch is the global one
            global_batch = b_local if self.dp.world_size == 1 else int(self.hparams.minibatch_size)
        self.dp.allreduce_device(flat)
        self.opt.t += 1
        self._apply(flat, global_batch)
        self._mark_dirty()                                          # the host copies (model.variables, Adam slots) are stale now
        self.global_step += 1
        out = {"global_step": self.global_step, "global_batch": int(global_batch), "losses_dev": st["losses"]}
        if sync:
            lo = st["losses"].cpu().numpy()
            out.update(model_loss=float(lo[0]), total_loss=float(lo[1]))
            del out["losses_dev"]
            self.history.append(out)
        return out

    # -- held-out evaluation ------------------------------------------------------------------------
    def evaluate(self, dataset, minibatch_size: Optional[int] = None, T: Optional[int] = None, keep_losses: bool = False):
        """The current parameters' loss over every clip of ``dataset`` (a ResidentDataset; audio_mps_amd/evaluate.py): an EvalResult.
        Under ``device_step`` the parameters are the device-resident ones (the buffers cmps_*_apply_step wrote), read where they are.
        Training is left untouched: the pass runs forward scans only, writes no variable and no Adam slot, and every training step
        configures the backend for itself (set_params* with its own shape), so the steps after an evaluation are bit for bit those of a
        run without it.  With several ranks every rank evaluates the whole dataset: nothing is communicated."""
        from .evaluate import pass_shape, run_pass
        m = self.model
        be = m._get_backend()
        mb, T, B_max = pass_shape(be, dataset, minibatch_size, self.hparams.minibatch_size, T)
        if self.device_step:
            st, rank = self._device_state(), self._rank()
            be.set_params_dev(st["params"], m.sigma, m.delta_t, B_max, T, train=False)
            if rank:
                be.rho_set_state_dev(st["phi"], rank, B_max, T, train=False)
        else:
            be = m._prepare(B_max, T, train=False)
        fwd = m._forward_entry(be)
        return run_pass(dataset.ordered(mb, T), lambda batch: fwd(batch, save_for_bwd=False), be, T, keep_losses)

    # -- checkpoint / resume (train.py:93: save_checkpoint_secs=60, automatic restore from logdir) --
    def save(self, path: str):
        self.sync_to_host()
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        payload = {f"model/{k}": v for k, v in self.model.variables.items()}
        payload.update({f"adam/{k}": v for k, v in self.opt.state_dict().items()})
        payload["global_step"] = np.int64(self.global_step)
        tmp = path + ".tmp.npz"
        np.savez(tmp, **payload)
        os.replace(tmp, path)

    def restore(self, path: str) -> bool:
        if not os.path.exists(path):
            return False
        with np.load(path) as z:
            for k in list(self.model.variables):
                self.model.variables[k] = np.asarray(z[f"model/{k}"], dtype=np.float32)
            self.opt.load_state_dict({k[5:]: z[k] for k in z.files if k.startswith("adam/")})
            self.global_step = int(z["global_step"])
        self._forget()                                              # the device-resident copy is rebuilt from the restored state
        return True


def build_parser():
    p = argparse.ArgumentParser(description="Train PsiCMPS on MI355X (mirror of audio-mps train.py)")
    p.add_argument("--log_every", type=int, default=1, help="print the losses every n-th step (the device-resident step copies them "
                   "to the host only then)")
    p.add_argument("--mps_model", default="psi_mps", choices=["rho_mps", "psi_mps"])           # train.py:18-20
    p.add_argument("--dataset", default="damped_sine",
                   choices=["damped_sine", "guitar", "organ", "nsynth"])                       # train.py:23-25
    p.add_argument("--sample_duration", type=int, default=2 ** 16)                              # train.py:27
    p.add_argument("--sample_rate", type=int, default=16000)                                    # train.py:28
    p.add_argument("--hparams", default="")                                                     # train.py:31
    p.add_argument("--datadir", default="./data")                                               # train.py:32
    p.add_argument("--logdir", default="../logging/audio_mps")                                  # train.py:33
    p.add_argument("--max_steps", type=int, default=100)
    p.add_argument("--save_checkpoint_secs", type=float, default=60.0)                          # train.py:93
    p.add_argument("--seed", type=int, default=0)                                               # train.py:13
    p.add_argument("--kernel_variant", type=int, default=0,
                   help="0 auto (float32: wave-per-clip kernels for D <= 32, wide kernels above), 1 block, 2 wave, "
                        "3 MFMA pair kernels (32 < D <= 128, bf16 mat-vec operands), 5 float32 wide kernels (32 < D <= 128)")
    p.add_argument("--host_optimizer", action="store_true",
                   help="chain rule and Adam in numpy on the host (the reference implementation of the optimiser half) instead of "
                        "the device-resident step (cmps_psi_apply_step / cmps_rho_apply_step)")
    p.add_argument("--device_data", action="store_true",
                   help="produce every batch on the device instead of on the host: damped_sine is generated there from (--seed, clip "
                        "number) (cmps_damped_sine_fill: other clips than the host generator draws for the same seed), a TFRecord dataset "
                        "is uploaded once and every batch gathered from it in the order of the host pipeline (cmps_batch_gather).  With "
                        "more than one rank every rank holds the whole dataset and gathers its shard of the batch")
    p.add_argument("--crop_duration", type=int, default=None,
                   help="with --device_data and a TFRecord dataset: train on this many samples of every clip, cut from a random start "
                        "(--sample_duration stays the length of the records)")
    p.add_argument("--eval_dataset", default=None, metavar="NAME",
                   help="held-out evaluation (audio_mps_amd/evaluate.py): NAME.tfrecords in --datadir, uploaded once and held on the "
                        "device; 'damped_sine' instead evaluates clips [0, --eval_clips) of seed --seed + 1 of the device's synthetic "
                        "sequence (cmps_damped_sine_fill).  With several ranks every rank evaluates the whole set; rank 0 writes")
    p.add_argument("--eval_every", type=int, default=0, help="evaluate every N steps (0: off); also after the last step")
    p.add_argument("--eval_clips", type=int, default=256, help="clips of the synthetic held-out set (--eval_dataset damped_sine)")
    p.add_argument("--eval_minibatch", type=int, default=None, help="clips per evaluation batch (default: minibatch_size)")
    p.add_argument("--bank", type=int, default=0, metavar="N",
                   help="train N models of --mps_model at once, seeds --seed .. --seed + N - 1 (audio_mps_amd/bank.py); every member trains on the "
                        "same batch")
    p.add_argument("--bank_hparams", default="", metavar="SPEC",
                   help="train the Cartesian grid of 'learning_rate=1e-3,3e-3;r_reg=0.1,1' (learning_rate, h_reg, r_reg) at once; with --bank "
                        "every seed runs once per grid point")
    p.add_argument("--bank_by", default=None, metavar="KEY",
                   help="train one model per class at once (reader.py:9-66: a model per pitch): KEY is the TFRecord feature that labels "
                        "every record (an Int64List such as pitch, a BytesList such as instrument_family_str); member m, seed --seed + m, "
                        "trains on the clips of class m only.  Needs --device_data and a TFRecord dataset; with --eval_dataset the bank is "
                        "judged as a classifier on the held-out file (BankTrainer.evaluate_classifier)")
    p.add_argument("--bank_classes", default=None, metavar="A,B,C",
                   help="with --bank_by: the classes, in member order (default: the sorted distinct labels of the dataset)")
    p.add_argument("--bank_objective", default="generative", choices=["generative", "discriminative"],
                   help="with --bank_by: generative (default) trains member m on the clips of class m alone; discriminative trains the "
                        "members against each other on ONE shared labelled batch per step (BankTrainer.step_classifier: every member "
                        "descends gen_weight * loss[own] + disc_weight * cross-entropy of softmax(-loss / temperature)).  No --mps_model rho_mps")
    p.add_argument("--disc_weight", type=float, default=1.0, help="--bank_objective discriminative: weight of the cross-entropy")
    p.add_argument("--gen_weight", type=float, default=0.0, help="--bank_objective discriminative: weight of the own member's loss")
    p.add_argument("--disc_temperature", type=float, default=1.0,
                   help="--bank_objective discriminative: temperature of the softmax over the members' losses.  A per-clip loss is a sum "
                        "over sample_duration - 1 samples, so differences between members are of that order: a temperature of that order "
                        "(e.g. sample_duration) keeps the softmax from saturating where the members' losses differ by that much; where "
                        "they differ by a few nats (README, \"Class banks\") such a temperature flattens it instead")
    p.add_argument("--eval_storage", default="float32", choices=["float32", "int16", "auto"],
                   help="how a TFRecord held-out set is held on the device (int16: half the memory for 16-bit PCM data, the same bits)")
    return p


def eval_dataset(args, hp, backend):
    """--eval_dataset: the held-out set as a ResidentDataset on the backend's device."""
    from .device_data import ResidentDataset, _need
    if args.eval_dataset == "damped_sine":
        _need(backend, "damped_sine", "--eval_dataset damped_sine")
        if args.eval_clips < 1:
            raise ValueError("--eval_clips must be positive")
        return ResidentDataset(backend.damped_sine(args.seed + 1, 0, args.eval_clips, args.sample_duration, hp.delta_t), backend)
    path = os.path.join(str(args.datadir), f"{args.eval_dataset}.tfrecords")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return ResidentDataset.from_tfrecord(path, args.sample_duration, backend, storage=args.eval_storage)


class EvalLog:
    """What train.main does with an evaluation: a line on the console, a JSON line appended to {logdir}/eval.jsonl, and
    {logdir}/model.best.ckpt.npz whenever the mean improves with no non-finite clip (rank 0 only; the best so far survives a restart
    through eval.jsonl)."""

    def __init__(self, logdir: str, write: bool):
        self.path, self.best_path, self.write = os.path.join(logdir, "eval.jsonl"), os.path.join(logdir, "model.best.ckpt.npz"), write
        self.best = math.inf
        if write and os.path.exists(self.path):
            with open(self.path) as f:
                for line in f:
                    rec = json.loads(line)
                    if rec.get("n_nonfinite") == 0 and rec.get("mean") is not None and rec["mean"] < self.best:
                        self.best = float(rec["mean"])

    def __call__(self, trainer, res):
        if not self.write:
            return
        print(f"eval step={trainer.global_step} loss={res.mean:.6f} per_sample={res.per_sample:.6g} clips={res.n_clips} "
              f"nonfinite={res.n_nonfinite}")
        os.makedirs(os.path.dirname(self.path) or ".", exist_ok=True)
        with open(self.path, "a") as f:
            f.write(json.dumps({"global_step": trainer.global_step, **res.scalars()}) + "\n")
        if res.n_nonfinite == 0 and res.mean < self.best:
            self.best = res.mean
            trainer.save(self.best_path)


def device_source(args, hp, backend):
    """--device_data: (next_size, next_shard) of the run's input.  next_size(step) is the size of the global batch of ``step``,
    next_shard(step, (start, count)) that rank's rows of it as a device tensor; the two are called in turn, once per step."""
    from .device_data import DampedSineSource, ResidentDataset
    if args.dataset == "damped_sine":
        src = DampedSineSource(backend, hp.minibatch_size, args.sample_duration, hp.delta_t, seed=args.seed)
        return (lambda step: hp.minibatch_size), src.next
    path = os.path.join(str(args.datadir), f"{args.dataset}.tfrecords")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} (the reference's data blobs are not distributed: .MISSING_LARGE_BLOBS)")
    stream = ResidentDataset.from_tfrecord(path, args.sample_duration, backend).batches(
        hp.minibatch_size, seed=args.seed, order="data", crop=args.crop_duration, crop_seed=args.seed)
    return (lambda step: stream.next_size), (lambda step, shard: stream(shard=shard))


def step_input(args, hp, backend):
    """The run's input, built ONCE (train.py:46-47): ``batch(step, shard)`` -> (size n of the global batch of ``step``, its rows
    ``shard(n) = (start, count)``; default: all of them).  For TFRecord datasets get_audio returns the one-shot iterator's get_next
    (batch -> shuffle(24) -> repeat, data.py:37-40), for damped_sine every step draws fresh delays (data.py:15); --device_data: the same
    batches (TFRecords) / the device's own clips (damped_sine), produced on the device, the asked rows only."""
    from .data import get_audio
    on_device = device_source(args, hp, backend) if args.device_data else None
    source = get_audio(args.datadir, args.dataset, hp, args.sample_duration, seed=args.seed) \
        if args.dataset != "damped_sine" and on_device is None else None

    def batch(step, shard=lambda n: (0, n)):
        if on_device is not None:
            n = int(on_device[0](step))
            return n, on_device[1](step, shard(n))
        full = source() if source is not None else get_audio(args.datadir, args.dataset, hp, args.sample_duration, seed=args.seed + step)
        n = int(full.shape[0])
        s0, c0 = shard(n)
        return n, full[s0:s0 + c0]
    return batch


def main(argv=None, backend=None):
    """``backend``: a scan backend to use instead of HipScan (CPU tests of the host logic inject one; the product
    always builds a HipScan and fails loudly without a GPU)."""
    args = build_parser().parse_args(argv)
    hp = HParams(delta_t=1.0 / args.sample_rate, h_reg=200.0 / (math.pi * args.sample_rate) ** 2)  # train.py:41-43
    hp.parse(args.hparams)
    if args.crop_duration is not None and (not args.device_data or args.dataset == "damped_sine"):
        raise ValueError("--crop_duration needs --device_data and a TFRecord dataset (crops are cut by the device-side gather)")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if backend is None:
        import torch
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        dp = DataParallel(device=dev)
        from .scan import HipScan
        backend = HipScan(hp.bond_dim, device=dev, variant=args.kernel_variant)
    else:
        dp = DataParallel(backend="gloo")
    start, count = dp.shard(hp.minibatch_size)
    if args.bank_classes is not None and args.bank_by is None:
        raise ValueError("--bank_classes names the classes of --bank_by KEY: it needs that flag")
    disc_flags = (args.disc_weight, args.gen_weight, args.disc_temperature) != (1.0, 0.0, 1.0)
    if args.bank_objective == "discriminative" and args.bank_by is None:
        raise ValueError("--bank_objective discriminative trains the members of a class bank against each other: it needs --bank_by KEY")
    if args.bank_objective != "discriminative" and disc_flags:
        raise ValueError("--disc_weight, --gen_weight and --disc_temperature belong to --bank_objective discriminative")
    if args.bank_by is not None:
        return class_bank_main(args, hp, backend, dp)
    if args.bank or args.bank_hparams:
        return bank_main(args, hp, backend, dp)
    cls = RhoCMPS if args.mps_model == "rho_mps" else PsiCMPS                                   # train.py:50-53
    model = cls(hp, seed=args.seed, backend=backend)
    device_step = (not args.host_optimizer and type(backend).__name__ == "HipScan")
    trainer = Trainer(model, hp, dp, device_step=device_step)
    logdir = f"{args.logdir}/{args.dataset}/{hp.bond_dim}_{hp.delta_t}_{hp.minibatch_size}"    # train.py:94
    ckpt = os.path.join(logdir, "model.ckpt.npz")
    if trainer.restore(ckpt) and dp.rank == 0:
        print(f"Restoring parameters from {ckpt} (global_step {trainer.global_step})")
    last_save = time.time()
    held_out = eval_dataset(args, hp, backend) if args.eval_dataset else None
    eval_log = EvalLog(logdir, dp.rank == 0)
    batch = step_input(args, hp, backend)
    for it in range(args.max_steps):
        # every rank reads the same global batch and keeps its shard (a short final batch of an epoch is sharded as it is)
        n_full, shard = batch(trainer.global_step, lambda n: dp.shard(n) if n != hp.minibatch_size else (start, count))
        # the losses come to the host only on logging steps (the device-resident step needs no device -> host copy otherwise)
        log_now = (it % max(args.log_every, 1) == 0) or it == args.max_steps - 1
        out = trainer.step(shard, sync=log_now, global_batch=n_full)
        if dp.rank == 0:
            if log_now:
                print(f"step {out['global_step']}: model_loss {out['model_loss']:.6f} total_loss {out['total_loss']:.6f}")
            if time.time() - last_save > args.save_checkpoint_secs or it == args.max_steps - 1:
                trainer.save(ckpt)
                last_save = time.time()
        if held_out is not None and ((args.eval_every > 0 and trainer.global_step % args.eval_every == 0) or it == args.max_steps - 1):
            eval_log(trainer, trainer.evaluate(held_out, args.eval_minibatch))
    dp.close()
    return trainer


def bank_main(args, hp, backend, dp):
    """``--bank`` / ``--bank_hparams``: the loop of ``main`` for a BankTrainer.  One batch per step, shared by every member."""
    from .bank import RHO_BANK_ENTRIES, BankTrainer, PsiBank, RhoBank, bank_members
    rho = args.mps_model == "rho_mps"                                                        # train.py:18-20, 50-53
    if rho and backend is not None and not all(hasattr(backend, name) for name in RHO_BANK_ENTRIES):
        raise ValueError("--bank --mps_model rho_mps needs a backend with the cmps_rho_bank_* entries (HipScan): this one "
                         f"({type(backend).__name__}) has none, and a loop of plain RhoCMPS trainers is what --bank is there to replace")
    if args.bank < 0:
        raise ValueError("--bank must not be negative (0: one seed per point of --bank_hparams)")
    # what the loop below does not do is refused, not ignored
    if args.eval_dataset or args.eval_every or args.eval_minibatch is not None:
        raise ValueError("--bank does not evaluate while it trains (--eval_dataset, --eval_every, --eval_minibatch): run "
                         "python -m audio_mps_amd.evaluate on a member's model.<m>.ckpt.npz, or BankTrainer.evaluate")
    if args.host_optimizer:
        raise ValueError("--bank runs the device-resident optimiser step of every member (cmps_bank_apply_step): no --host_optimizer")
    members = bank_members(args.seed, args.bank, args.bank_hparams)
    trainer = BankTrainer((RhoBank if rho else PsiBank)(hp, members, backend=backend), dp)
    logdir = f"{args.logdir}/{args.dataset}/{hp.bond_dim}_{hp.delta_t}_{hp.minibatch_size}"    # train.py:94
    if trainer.restore(logdir):
        print(f"Restoring {len(trainer)} members from {logdir} (global_step {trainer.global_step})")
    last_save = time.time()
    batch = step_input(args, hp, backend)
    for it in range(args.max_steps):
        log_now = (it % max(args.log_every, 1) == 0) or it == args.max_steps - 1
        out = trainer.step(batch(trainer.global_step)[1], sync=log_now)
        if log_now:
            print(bank_log_line(out))
        if time.time() - last_save > args.save_checkpoint_secs or it == args.max_steps - 1:
            trainer.save(logdir)
            last_save = time.time()
    dp.close()
    return trainer


def parse_classes(spec: str, labels: np.ndarray) -> list:
    """``--bank_classes a,b,c`` as values of the dataset's labels: ints where those are ints."""
    items = [s.strip() for s in spec.split(",") if s.strip()]
    if not items:
        raise ValueError("--bank_classes names no class")
    return items if labels.dtype == object else [int(s) for s in items]


def class_bank_main(args, hp, backend, dp):
    """``--bank_by KEY``: a labelled TFRecord dataset trained as one model per class, every member on the clips of its own class
    (ResidentDataset.class_batches: one gather of M B rows per step), and -- with --eval_dataset -- judged as a classifier on a held-out
    file while it trains (BankTrainer.evaluate_classifier: one forward and one reduction per batch, one download per pass)."""
    from .bank import RHO_BANK_ENTRIES, BankTrainer, PsiBank, RhoBank
    from .device_data import ResidentDataset
    rho = args.mps_model == "rho_mps"
    if args.bank or args.bank_hparams:
        raise ValueError("--bank_by makes one member per class, seeds --seed + m: it does not go with --bank N or --bank_hparams")
    if not args.device_data or args.dataset == "damped_sine":
        raise ValueError("--bank_by needs --device_data and a TFRecord dataset: the classes are the values of a feature of its records, "
                         "and every member's batch is gathered from the resident dataset (damped_sine has no labels)")
    if args.host_optimizer:
        raise ValueError("--bank_by runs the device-resident optimiser step of every member (cmps_bank_apply_step): no --host_optimizer")
    disc = args.bank_objective == "discriminative"
    if disc and rho:
        raise ValueError("--bank_objective discriminative trains PsiCMPS members (cmps_bank_loss_bwd_weighted): no --mps_model rho_mps")
    if disc and not (args.disc_weight >= 0.0 and args.gen_weight >= 0.0 and args.disc_temperature > 0.0
                     and all(math.isfinite(x) for x in (args.disc_weight, args.gen_weight, args.disc_temperature))):
        raise ValueError("--bank_objective discriminative needs finite --disc_weight >= 0, --gen_weight >= 0 and --disc_temperature > 0")
    if disc and not hasattr(backend, "classify_weights"):
        raise ValueError("--bank_objective discriminative needs a backend with cmps_bank_classify_weights and the weighted reverse pass "
                         f"(HipScan): this one ({type(backend).__name__}) has none")
    if rho and not all(hasattr(backend, name) for name in RHO_BANK_ENTRIES):
        raise ValueError("--bank_by --mps_model rho_mps needs a backend with the cmps_rho_bank_* entries (HipScan): this one "
                         f"({type(backend).__name__}) has none")
    if args.eval_dataset == "damped_sine":
        raise ValueError("--bank_by judges the bank on a labelled TFRecord file: --eval_dataset damped_sine has no labels")
    if (args.eval_every or args.eval_minibatch is not None) and not args.eval_dataset:
        raise ValueError("--eval_every and --eval_minibatch need --eval_dataset")

    def resident(name, storage):
        path = os.path.join(str(args.datadir), f"{name}.tfrecords")
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        return ResidentDataset.from_tfrecord(path, args.sample_duration, backend, storage=storage, label_key=args.bank_by)
    data = resident(args.dataset, "float32")
    classes = parse_classes(args.bank_classes, data.labels) if args.bank_classes is not None else sorted(set(data.labels.tolist()))
    bank = (RhoBank if rho else PsiBank)(hp, [{"seed": args.seed + m} for m in range(len(classes))], backend=backend, classes=classes,
                                         label_key=args.bank_by)
    at = data.class_positions(classes)
    bank.class_counts = np.bincount(at[at >= 0], minlength=len(classes)).tolist()   # bank.json keeps them: sample / evaluate --prior empirical
    trainer = BankTrainer(bank, dp)
    logdir = f"{args.logdir}/{args.dataset}/{hp.bond_dim}_{hp.delta_t}_{hp.minibatch_size}"    # train.py:94
    if trainer.restore(logdir):
        print(f"Restoring {len(trainer)} members from {logdir} (global_step {trainer.global_step})")
    if disc:        # one shared labelled batch per step, the members trained against each other (bank.json records the objective)
        trainer.objective = {"name": "discriminative", "disc_weight": args.disc_weight, "gen_weight": args.gen_weight,
                             "temperature": args.disc_temperature}
        stream = data.labelled_batches(classes, hp.minibatch_size, seed=args.seed, order="estimator", crop=args.crop_duration,
                                       crop_seed=args.seed)           # (shuffle -> repeat -> batch: every batch is full, as class_batches')
    else:
        stream = data.class_batches(classes, hp.minibatch_size, seed=args.seed, crop=args.crop_duration)
    held_out = resident(args.eval_dataset, args.eval_storage) if args.eval_dataset else None
    last_save = time.time()
    for it in range(args.max_steps):
        log_now = (it % max(args.log_every, 1) == 0) or it == args.max_steps - 1
        if disc:
            batch, labels = stream()
            out = trainer.step_classifier(batch, labels, gen_weight=args.gen_weight, disc_weight=args.disc_weight,
                                          temperature=args.disc_temperature, sync=log_now)
        else:
            out = trainer.step(stream(), sync=log_now)
        if log_now:
            print(bank_log_line(out) + (f" xent={out['xent']:.6f} used={out['used']}" if disc else ""))
        if time.time() - last_save > args.save_checkpoint_secs or it == args.max_steps - 1:
            trainer.save(logdir)
            last_save = time.time()
        if held_out is not None and ((args.eval_every > 0 and trainer.global_step % args.eval_every == 0) or it == args.max_steps - 1):
            res = trainer.evaluate_classifier(held_out, args.eval_minibatch)
            print(f"eval step={trainer.global_step} {res.line()}")
            os.makedirs(logdir, exist_ok=True)
            with open(os.path.join(logdir, "eval.jsonl"), "a") as f:
                f.write(json.dumps({"global_step": trainer.global_step, **res.scalars()}) + "\n")
    dp.close()
    return trainer


def bank_log_line(out) -> str:
    """The log line of a bank step: best, median and worst member loss among the finite ones, and how many are not."""
    loss = np.asarray(out["model_loss"], dtype=np.float64)
    fin = np.sort(loss[np.isfinite(loss)])
    if fin.size == 0:
        return f"step {out['global_step']}: members {loss.size} nonfinite {loss.size}"
    return (f"step {out['global_step']}: members {loss.size} best {fin[0]:.6f} (member {int(np.nanargmin(np.where(np.isfinite(loss), loss, np.nan)))}) "
            f"median {float(np.median(fin)):.6f} worst {fin[-1]:.6f} nonfinite {loss.size - fin.size}")


if __name__ == "__main__":
    main()
