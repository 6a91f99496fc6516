"""A class bank's prior over its members: the three ways a caller spells one, and the log prior as bank.json, a JSON line and the device
hold it.  ``stream.BankStream`` (score_posterior), ``bank.BankTrainer`` (calibrate) and the --prior flags of sample and evaluate all come
here."""
from __future__ import annotations

import math

import numpy as np


def log_prior_of(prior, M: int, class_counts=None, who: str = ""):
    """``prior``: None (uniform: stays None), "empirical" (``class_counts``, the clips per class of the training set) or [M] probabilities
    (any positive scale; a zero: that member never wins; any shape of M entries, flattened) -> the normalised log, float64 [M] with
    -inf for a zero."""
    if prior is None:
        return None
    who = who and who + ": "
    if isinstance(prior, str):
        if prior != "empirical":
            raise ValueError(f"{who}prior is None, 'empirical' or {M} probabilities, not {prior!r}")
        if class_counts is None:
            raise ValueError(f"{who}prior='empirical' needs the bank's class counts (bank.json of a bank trained with --bank_by)")
        prior = class_counts
    p = np.asarray(prior, dtype=np.float64).reshape(-1)
    if p.shape != (M,) or not np.all(np.isfinite(p)) or np.any(p < 0.0) or not np.sum(p) > 0.0:
        raise ValueError(f"{who}prior must be {M} finite probabilities, none negative and not all zero")
    with np.errstate(divide="ignore"):
        return np.log(p / np.sum(p))


def log_prior_json(log_prior) -> list:
    """A log prior as bank.json and a JSON line hold it: floats, and null for -inf (a prior of zero), which JSON has no number for."""
    return [None if c == -math.inf else float(c) for c in np.asarray(log_prior, dtype=np.float64)]


def log_prior_array(values) -> np.ndarray:
    """`log_prior_json` read back (an array passes through): float64 [M] with -inf for null."""
    return np.array([-math.inf if c is None else float(c) for c in values], dtype=np.float64)


def normalised_prior(log_prior) -> np.ndarray:
    """exp(c - logsumexp c) of a log prior whose entries are finite or -inf (null: -inf)."""
    c = log_prior_array(log_prior)
    top = np.max(c)
    w = np.exp(c - top)
    return w / np.sum(w)
