"""Sampler for a trained model: the reference's sample.py, which declares its flags (sample.py:10-14) and leaves ``main`` empty.

  flags              sample.py:10-14     --sample_duration, --sample_rate, --modeldir (same names, same defaults)
  model              train.py:49-53      PsiCMPS(hparams) or, for a checkpoint holding Wx / Wy (--mps_model rho_mps), RhoCMPS(hparams); its
                                         variables read from the checkpoint Trainer.save writes
  waveform           model.py:242-251    model.sample(num_samples, sample_duration, temp) / A, in the data's units (RhoCMPS: :103-116)

``--prime FILE`` (a 16-bit mono .wav, or a .npy array [T'], [1, T'] or [num_samples, T']) continues a clip instead: the state is
teacher-forced on the clip and the sampler carries on from there (continue_clip; cmps_psi_sample_primed / cmps_rho_sample_primed); the written
waveform is the clip followed by its continuation.  Writes ``sample_<i>.wav`` (16-bit PCM mono at --sample_rate, clipped to
[-1, 1)) and ``samples.npy`` (float32 [num_samples, samples], unclipped) into --out_dir.
``--segment S`` runs the same job through a resumable stream (model.open_stream; cmps_psi_stream / cmps_rho_stream) in segments of S steps: the
prime, if given, is followed, then the waveform is generated; the files and the return value are the same.
``--device_noise`` (plain, --prime and --segment runs) draws the noise on the device instead of on the host (cmps_noise_fill): counter-based
normals of (--seed, path, step), so --segment then changes no bit of the waveform however it cuts the run.
``--score FILE`` (a clip as --prime reads it; either model) samples nothing: the clip is followed and scored through a stream
(SampleStream.score; cmps_psi_stream_score / cmps_rho_stream_score), in segments of --segment steps when given.  Writes ``nll.npy`` (float32
[clips, T' - 1]: the negative log-likelihood of every sample, model.py:293-294 / :166, 169-170) and ``pred.npy`` (the model's expected increments) into --out_dir and prints
the total and the mean per sample; returns the nll array.
``--bankdir DIR`` (a directory BankTrainer.save wrote: bank.json + model.<m>.ckpt.npz; PsiCMPS members, or RhoCMPS members where bank.json says
rho_mps) does the same with every member of the bank at once (PsiBank.open_stream / RhoBank.open_stream; cmps_bank_stream* /
cmps_rho_bank_stream*), every member hearing the same noise: sampling writes
``sample_m<m>_<i>.wav`` and ``samples.npy`` [M, num_samples, samples]; --prime continues one clip with every member; --score --posterior
judges the members as a classifier after every sample of the clip (``posterior.npy`` [M, steps], ``best.npy``, ``conf.npy``; --prior,
--temperature, --threshold); --score writes
``nll.npy`` ([M, T' - 1] for one clip, else [M, clips, T' - 1]) and ``pred.npy`` and prints one line per member and the best member.
Run:  python -m audio_mps_amd.sample --modeldir=LOGDIR --sample_duration=16000 --prime=clip.wav
"""
from __future__ import annotations

import argparse
import math
import os
import wave

import numpy as np

from .model import CMPS, HParams, PsiCMPS, RhoCMPS
from .prior import log_prior_of, normalised_prior
from .stream import as_clips, segments

CKPT_NAME = "model.ckpt.npz"          # what train.main saves into its logdir


def read_wav(path: str):
    """(float32 samples in [-1, 1), sample rate) of a 16-bit mono PCM file: int16 / 32768.  Anything else is an error."""
    with wave.open(path, "rb") as w:
        ch, width, rate, frames, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()
        if ch != 1 or width != 2 or comp != "NONE":
            raise ValueError(f"{path}: need 16-bit mono PCM, found {ch} channel(s), {8 * width}-bit samples, compression {comp}")
        raw = w.readframes(frames)
    return (np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768)), rate


def write_wav(path: str, x, rate: int):
    """16-bit mono PCM at ``rate``: round(x * 32768) clipped to the int16 range, i.e. x clipped to [-1, 1)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.tobytes())


def load_prime(path: str, sample_rate: int) -> np.ndarray:
    """The clip to continue: .npy (float array [T'], [1, T'] or [n, T'], the data's units) or .wav (16-bit mono at --sample_rate)."""
    if path.lower().endswith(".npy"):
        return np.asarray(np.load(path), dtype=np.float32)
    if path.lower().endswith(".wav"):
        x, rate = read_wav(path)
        if rate != sample_rate:
            raise ValueError(f"{path}: sampled at {rate} Hz, the model runs at --sample_rate {sample_rate} Hz")
        return x
    raise ValueError(f"--prime {path}: need a .wav or .npy file")


def load_variables(modeldir: str) -> dict:
    """The ``model/*`` entries of a checkpoint written by Trainer.save; ``modeldir`` is the directory holding it, or the file."""
    path = os.path.join(modeldir, CKPT_NAME) if os.path.isdir(modeldir) else modeldir
    if not os.path.exists(path):
        raise FileNotFoundError(f"no checkpoint at {path} (--modeldir: a directory holding {CKPT_NAME}, or the file itself)")
    with np.load(path) as z:
        out = {k[len("model/"):]: np.asarray(z[k], dtype=np.float32) for k in z.files if k.startswith("model/")}
    if not out:
        raise ValueError(f"{path} holds no model/* variables")
    return out


def build_parser():
    p = argparse.ArgumentParser(description="Sample from a trained PsiCMPS or RhoCMPS on MI355X, or continue a clip (audio-mps sample.py, filled in)")
    p.add_argument("--sample_duration", type=int, default=2 ** 16, help="samples to generate (as integer)")      # sample.py:10
    p.add_argument("--sample_rate", type=int, default=16000)                                                      # sample.py:11
    p.add_argument("--modeldir", default="./data", help=f"directory holding {CKPT_NAME}, or the checkpoint file")  # sample.py:14
    p.add_argument("--hparams", default="", help="as for training (r_reg, h_reg, sigma, delta_t must be the training run's; "
                   "bond_dim and initial_rank are read from the checkpoint)")
    p.add_argument("--num_samples", type=int, default=1)
    p.add_argument("--temp", type=float, default=1.0, help="noise temperature (model.py:246)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--prime", default=None, metavar="FILE", help=".wav (16-bit mono) or .npy clip to continue")
    p.add_argument("--score", default=None, metavar="FILE", help=".wav (16-bit mono) or .npy clip to follow and score instead of sampling (PsiCMPS or RhoCMPS)")
    p.add_argument("--device_noise", action="store_true", help="draw the noise on the device, from (--seed, path, step) (cmps_noise_fill), "
                   "instead of a host Generator")
    p.add_argument("--segment", type=int, default=None, metavar="S", help="run through a resumable stream in segments of S steps")
    p.add_argument("--bankdir", default=None, metavar="DIR", help="a directory BankTrainer.save wrote (bank.json + model.<m>.ckpt.npz): sample, "
                   "continue or score with every member of a PsiCMPS or RhoCMPS bank at once, instead of --modeldir")
    p.add_argument("--posterior", action="store_true", help="with --bankdir --score: judge the members as a classifier after every sample "
                   "(cmps_bank_posterior); writes posterior.npy, best.npy and conf.npy instead of nll.npy and pred.npy")
    p.add_argument("--prior", default=None, metavar="P0,P1,...|empirical", help="with --posterior: the members' prior probabilities, or "
                   "'empirical': the class counts bank.json holds (default: uniform)")
    p.add_argument("--temperature", type=float, default=1.0, help="with --posterior: the members' total losses are divided by it")
    p.add_argument("--threshold", type=float, default=None, metavar="P", help="with --posterior: report the first sample at which the best "
                   "member's probability reached P")
    p.add_argument("--calibrated", action="store_true", help="with --posterior: take temperature and prior from the calibration "
                   "bank.json holds (evaluate --calibrate ... --save_calibration), instead of --temperature and --prior")
    p.add_argument("--out_dir", default="./samples")
    p.add_argument("--kernel_variant", type=int, default=0, help="as in audio_mps_amd.train")
    return p


def _segmented(model, args, n, length):
    """The job of `main` through a SampleStream in segments of --segment steps: the prime's increments followed, then `length` generated."""
    S = args.segment
    prime = None if args.prime is None else CMPS._prime(load_prime(args.prime, args.sample_rate), n)
    P = 0 if prime is None else prime.shape[1] - 1
    st = model.open_stream(n, P + length, temp=args.temp, seed=args.seed, device_noise=args.device_noise)
    parts = []
    if prime is not None:
        parts.append(np.broadcast_to(prime, (n, prime.shape[1])))
        for lo, hi in segments(P, S):
            st.follow(prime[:, lo:hi])
    for a in range(0, length, S):
        parts.append(st.generate(min(S, length - a)))
    return np.concatenate(parts, axis=1)


def _scored(model, args):
    """--score: the clip followed and scored through a SampleStream, whole or in segments of --segment steps; writes nll.npy / pred.npy."""
    clip = as_clips(load_prime(args.score, args.sample_rate), f"--score {args.score}")
    n, N = clip.shape[0], clip.shape[1] - 1
    st = model.open_stream(n, N)
    nll = _save_scored(st, clip, args)
    total = float(np.sum(st.total_nll, dtype=np.float64))
    print(f"scored {n} clip(s) of {N} steps: total nll {total:.6g}, mean per sample {total / (n * N):.6g}; wrote nll.npy and pred.npy to {args.out_dir}")
    return nll


def _save_scored(st, clip, args, one=lambda x: x):
    """The job of --score for one model and for a bank: ``clip`` [n, T'] followed and scored through the fresh stream ``st``, whole or
    in segments of --segment steps, then nll.npy and pred.npy written (a bank with a single clip drops the clip axis through ``one``).
    Returns the nll array; the totals are in ``st.total_nll``."""
    nll, pred = [], []
    for lo, hi in segments(clip.shape[1] - 1, args.segment):
        nll.append(st.score(clip[:, lo:hi]))
        pred.append(st.last_pred)
    nll, pred = (np.ascontiguousarray(one(np.concatenate(x, axis=-1)), dtype=np.float32) for x in (nll, pred))
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(os.path.join(args.out_dir, "nll.npy"), nll)
    np.save(os.path.join(args.out_dir, "pred.npy"), pred)
    return nll


def build_model(variables: dict, sample_rate: int, hparams: str = "", kernel_variant: int = 0, seed: int = 0, backend=None):
    """The model a checkpoint's ``variables`` (load_variables) belong to, holding them: RhoCMPS where they include Wx / Wy, else PsiCMPS;
    bond_dim and initial_rank are read from their shapes, the other hyper-parameters are train.main's defaults overridden by ``hparams``."""
    rho = "Wx" in variables and "Wy" in variables             # a RhoCMPS checkpoint (train.py --mps_model rho_mps)
    if not rho and "psi_x" not in variables:
        raise ValueError("the checkpoint holds neither psi_x (PsiCMPS) nor Wx / Wy (RhoCMPS)")
    hp = HParams(delta_t=1.0 / sample_rate, h_reg=200.0 / (math.pi * sample_rate) ** 2)       # train.py:41-43
    if rho:
        hp.initial_rank, hp.bond_dim = (int(x) for x in variables["Wx"].shape)
    else:
        hp.bond_dim = int(variables["psi_x"].shape[0])
    hp.parse(hparams)
    if backend is None:
        from .scan import HipScan
        backend = HipScan(hp.bond_dim, variant=kernel_variant)
    model = (RhoCMPS if rho else PsiCMPS)(hp, seed=seed, backend=backend)
    for k in model.variables:
        if variables[k].shape != model.variables[k].shape:
            raise ValueError(f"checkpoint variable {k} has shape {variables[k].shape}, bond_dim={hp.bond_dim} needs {model.variables[k].shape}")
        model.variables[k] = variables[k]
    return model


def load_bank(bankdir: str, sample_rate: int, hparams: str = "", kernel_variant: int = 0, backend=None):
    """The PsiBank (a bank.json of rho_mps: the RhoBank) a directory written by BankTrainer.save holds, every member with its checkpoint's
    variables; bond_dim (and initial_rank) are read from their shapes, as `build_model` does."""
    import json
    from .bank import BankTrainer, PsiBank, RhoBank
    path = os.path.join(bankdir, "bank.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"no bank at {path} (--bankdir: a directory BankTrainer.save wrote)")
    with open(path) as f:
        meta = json.load(f)
    name = meta.get("model", PsiBank.MODEL_NAME)
    if name not in (PsiBank.MODEL_NAME, RhoBank.MODEL_NAME):
        raise ValueError(f"{path} was written by a bank of {name} models: --bankdir knows {PsiBank.MODEL_NAME} and {RhoBank.MODEL_NAME}")
    rho = name == RhoBank.MODEL_NAME
    variables = [load_variables(BankTrainer.member_path(bankdir, m)) for m in range(len(meta["members"]))]
    hp = HParams(delta_t=1.0 / sample_rate, h_reg=200.0 / (math.pi * sample_rate) ** 2)       # train.py:41-43
    if rho:
        if any("Wx" not in v or "Wy" not in v for v in variables):
            raise ValueError(f"{bankdir}: bank.json says {name}, but a member's checkpoint holds no Wx / Wy (RhoCMPS)")
        hp.initial_rank, hp.bond_dim = (int(x) for x in variables[0]["Wx"].shape)
    else:
        if any("psi_x" not in v for v in variables):
            raise ValueError(f"{bankdir}: a member's checkpoint holds no psi_x (PsiCMPS)")
        hp.bond_dim = int(variables[0]["psi_x"].shape[0])
    hp.parse(hparams)
    if backend is None:
        from .scan import HipScan
        backend = HipScan(hp.bond_dim, variant=kernel_variant)
    if rho and not (hasattr(backend, "rho_bank_stream") or hasattr(backend, "rho_stream")):
        raise ValueError(f"{path} holds a bank of {name} models: {type(backend).__name__} has neither rho_bank_stream nor rho_stream")
    bank = (RhoBank if rho else PsiBank)(hp, meta["members"], backend=backend, classes=meta.get("classes"), label_key=meta.get("label_key"))
    bank.class_counts = meta.get("class_counts")                  # clips per class of the training set, where the trainer recorded them
    bank.calibration = meta.get("calibration")                    # a fitted temperature and log prior, where somebody calibrated the bank
    for m, (model, var) in enumerate(zip(bank.models, variables)):
        for k in model.variables:
            if var[k].shape != model.variables[k].shape:
                raise ValueError(f"member {m}: checkpoint variable {k} has shape {var[k].shape}, bond_dim={hp.bond_dim} needs {model.variables[k].shape}")
            model.variables[k] = var[k]
    return bank


def parse_prior(spec, bank, where: str = ""):
    """--prior: None (uniform) and "empirical" as they are (prior.log_prior_of knows both), "p0,p1,..." -> [M] floats.  What comes back
    is a prior the bank takes: a wrong one is refused here, before anything is loaded or scored."""
    prior = spec if spec is None or spec == "empirical" else [float(x) for x in spec.split(",")]
    if isinstance(prior, list) and len(prior) != len(bank):
        raise ValueError(f"--prior names {len(prior)} probabilities, {where or 'the bank'} has {len(bank)} members")
    log_prior_of(prior, len(bank), bank.class_counts, f"--prior {spec}")
    return prior


def saved_calibration(bank, where: str, temperature: float = 1.0, prior=None):
    """--calibrated: (temperature, prior [M]) of the calibration bank.json holds (evaluate --calibrate ... --save_calibration), the prior
    normalised as exp(c - logsumexp c).  It stands in for --temperature and --prior, so neither may be given beside it."""
    if temperature != 1.0 or prior is not None:
        raise ValueError("--calibrated takes temperature and prior from bank.json: it goes with neither --temperature nor --prior")
    cal = getattr(bank, "calibration", None)
    if cal is None:
        raise ValueError(f"--calibrated: {where} holds no calibration (evaluate --bankdir ... --calibrate ... --save_calibration writes one)")
    if len(cal["log_prior"]) != len(bank):
        raise ValueError(f"--calibrated: the calibration of {where} names {len(cal['log_prior'])} members, the bank has {len(bank)}")
    return float(cal["temperature"]), [float(p) for p in normalised_prior(cal["log_prior"])]


def posterior_settings(bank, args):
    """(temperature, prior) a posterior over the members is judged with: the calibration bank.json holds (--calibrated), else --temperature
    and --prior."""
    if args.calibrated:
        return saved_calibration(bank, args.bankdir, args.temperature, args.prior)
    return args.temperature, parse_prior(args.prior, bank, args.bankdir)


def _bank_posterior(bank, args, clip):
    """--bankdir --score --posterior: the clip followed by every member and judged after every sample (BankStream.score_posterior)."""
    M, n, N = len(bank), clip.shape[0], clip.shape[1] - 1
    temperature, prior = posterior_settings(bank, args)
    tr = bank.posterior_trace(clip, prior=prior, temperature=temperature, threshold=args.threshold, segment=args.segment, want_post=True)
    one = (lambda x, lead: x[:, 0] if lead else x[0]) if n == 1 else (lambda x, lead: x)
    post = np.ascontiguousarray(one(tr.post, True), dtype=np.float32)
    np.save(os.path.join(args.out_dir, "posterior.npy"), post)
    np.save(os.path.join(args.out_dir, "best.npy"), np.ascontiguousarray(one(tr.best, False)))
    np.save(os.path.join(args.out_dir, "conf.npy"), np.ascontiguousarray(one(tr.conf, False)))
    named = (lambda m: f" (class {bank.classes[m]!r})") if bank.classes is not None else (lambda m: "")
    for m in range(M):
        print(f"member {m}{named(m)}: final posterior " + " ".join(f"{tr.post[m, i, -1]:.6g}" for i in range(n)))
    for i in range(n):
        b = int(tr.best[i, -1])
        head = f"clip {i}: final best " + (f"member {b}{named(b)}, probability {tr.conf[i, -1]:.6g}" if b >= 0 else "nobody (no finite loss)")
        if args.threshold is None:
            print(head)
        elif tr.decided_at[i] < 0:
            print(f"{head}; undecided (never reached {args.threshold:g})")
        else:
            a = int(tr.decided_as[i])
            print(f"{head}; decided at sample {int(tr.decided_at[i])} as member {a}{named(a)}")
    print(f"judged {n} clip(s) of {N} steps under {M} members; wrote posterior.npy, best.npy and conf.npy to {args.out_dir}")
    return post


def _bank_main(args, backend):
    """--bankdir: `main`'s three jobs with every member of a bank at once, through one BankStream."""
    bank = load_bank(args.bankdir, args.sample_rate, args.hparams, args.kernel_variant, backend)
    M, n, length = len(bank), args.num_samples, args.sample_duration
    os.makedirs(args.out_dir, exist_ok=True)
    if args.score is not None:
        clip = as_clips(load_prime(args.score, args.sample_rate), f"--score {args.score}")
        if args.posterior:
            return _bank_posterior(bank, args, clip)
        n, N = clip.shape[0], clip.shape[1] - 1
        st = bank.open_stream(n, N)
        nll = _save_scored(st, clip, args, (lambda x: x[:, 0]) if n == 1 else (lambda x: x))
        totals = np.sum(st.total_nll, axis=1, dtype=np.float64)
        named = (lambda m: f" (class {bank.classes[m]!r})") if bank.classes is not None else (lambda m: "")     # a class bank names its classes
        for m in range(M):
            print(f"member {m}{named(m)}: total nll {totals[m]:.6g}, mean per sample {totals[m] / (n * N):.6g}, {bank.overrides[m]}")
        best = int(np.argmin(np.where(np.isfinite(totals), totals, np.inf)))
        print(f"best member {best}{named(best)} of {M} over {n} clip(s) of {N} steps; wrote nll.npy and pred.npy to {args.out_dir}")
        return nll
    prime = None if args.prime is None else CMPS._prime(load_prime(args.prime, args.sample_rate), n)
    P = 0 if prime is None else prime.shape[1] - 1
    S = max(P, length) if args.segment is None else args.segment
    st = bank.open_stream(n, P + length, temp=args.temp, seed=args.seed, device_noise=args.device_noise)
    parts = []
    if prime is not None:
        parts.append(np.broadcast_to(prime, (M, n, prime.shape[1])))
        for lo, hi in segments(P, S):
            st.follow(prime[:, lo:hi])
    for a in range(0, length, S):
        parts.append(st.generate(min(S, length - a)))
    waves = np.ascontiguousarray(np.concatenate(parts, axis=-1), dtype=np.float32)
    np.save(os.path.join(args.out_dir, "samples.npy"), waves)
    for m in range(M):
        for i in range(n):
            write_wav(os.path.join(args.out_dir, f"sample_m{m}_{i}.wav"), waves[m, i], args.sample_rate)
    print(f"wrote {M} x {n} waveform(s) of {waves.shape[-1]} samples to {args.out_dir}")
    return waves


def main(argv=None, backend=None):
    """Returns the waveforms [num_samples, samples] it wrote.  ``backend``: a scan backend to use instead of HipScan (CPU tests of the
    host logic inject one; the product always builds a HipScan and fails loudly without a GPU)."""
    import sys
    args = build_parser().parse_args(argv)
    if args.sample_duration < 1 or args.num_samples < 1:
        raise ValueError("--sample_duration and --num_samples must be positive")
    if args.posterior and (args.bankdir is None or args.score is None):
        raise ValueError("--posterior judges the members of a bank along a clip: it needs --bankdir and --score")
    if not args.posterior and (args.prior is not None or args.threshold is not None or args.temperature != 1.0):
        raise ValueError("--prior, --temperature and --threshold belong to --posterior")
    if args.calibrated and not args.posterior:
        raise ValueError("--calibrated belongs to --posterior: it stands in for --temperature and --prior")
    if args.calibrated and (args.temperature != 1.0 or args.prior is not None):
        raise ValueError("--calibrated takes temperature and prior from bank.json: it goes with neither --temperature nor --prior")
    if args.bankdir is not None:
        if any(a == "--modeldir" or a.startswith("--modeldir=") for a in (sys.argv[1:] if argv is None else argv)):
            raise ValueError("--bankdir and --modeldir do not go together: a bank's members are read from --bankdir")
        if args.segment is not None and args.segment < 1:
            raise ValueError("--segment must be positive")
        if args.score is not None and (args.device_noise or args.prime is not None):
            raise ValueError("--score follows and scores its clip and samples nothing: it goes with neither --device_noise nor --prime")
        return _bank_main(args, backend)
    model = build_model(load_variables(args.modeldir), args.sample_rate, args.hparams, args.kernel_variant, args.seed, backend)
    n, length = args.num_samples, args.sample_duration
    if args.segment is not None and args.segment < 1:
        raise ValueError("--segment must be positive")
    if args.score is not None:
        if args.device_noise:
            raise ValueError("--score follows and scores its clip and samples nothing: there is no noise for --device_noise to draw")
        if args.prime is not None:
            raise ValueError("--score follows and scores its clip and samples nothing: it does not go with --prime")
        model._stream_score_entry(model._get_backend())           # (a backend that cannot score this model says so before anything is written)
        return _scored(model, args)
    if args.segment is not None:
        waves = _segmented(model, args, n, length)
    elif args.prime is None:
        waves = model.sample(n, length, temp=args.temp, seed=args.seed, device_noise=args.device_noise) / model.A
    else:
        prime = CMPS._prime(load_prime(args.prime, args.sample_rate), n)
        cont = model.continue_clip(prime, n, length, temp=args.temp, seed=args.seed, device_noise=args.device_noise)
        waves = np.concatenate([np.broadcast_to(prime, (n, prime.shape[1])), cont], axis=1)
    waves = np.ascontiguousarray(waves, dtype=np.float32)
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(os.path.join(args.out_dir, "samples.npy"), waves)
    for i in range(n):
        write_wav(os.path.join(args.out_dir, f"sample_{i}.wav"), waves[i], args.sample_rate)
    print(f"wrote {n} waveform(s) of {waves.shape[1]} samples to {args.out_dir}")
    return waves


if __name__ == "__main__":
    main()
