"""The flat float32 buffers of include/cmps.h, named once (numpy only: importable without torch or the library).

A layout is a tuple of (field, shape) pairs in buffer order; complex tensors are planar (``x_re`` then ``x_im``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

FLOAT_BYTES = 4
VAR_ORDER = ("A", "Rx", "Ry", "freqs", "psi_x", "psi_y")      # the device-resident variable / Adam-slot buffers (cmps_psi_apply_step)
RHO_VAR_ORDER = ("A", "Rx", "Ry", "freqs", "Wx", "Wy")        # ... of cmps_rho_apply_step


@dataclass
class EffectiveParams:
    """What CMPS.__init__ / PsiCMPS.__init__ hand to the scan (model.py:41-52, 221-222)."""
    R: np.ndarray        # [D, D] complex64, after the diagonal removal of model.py:42
    freqs: np.ndarray    # [D] float32
    psi0: np.ndarray     # [D] complex64, normalised
    A: float
    sigma: float
    delta_t: float


def param_fields(D: int, with_A: bool = False):
    """cmps_set_params' five tensors as one buffer; cmps_set_params_dev / cmps_psi_apply_step append A."""
    f = (("R_re", (D, D)), ("R_im", (D, D)), ("freqs", (D,)), ("psi0_re", (D,)), ("psi0_im", (D,)))
    return f + (("A", ()),) if with_A else f


def phi_fields(D: int, rank: int):
    """cmps_rho_set_state: the `rank` columns of rho_0."""
    return (("phi_re", (rank, D)), ("phi_im", (rank, D)))


def grad_fields(D: int, rank: int = 0):
    """cmps_psi_loss_bwd: cotangents of the effective parameters, then sum_b loss_b; cmps_rho_loss_bwd appends the columns'."""
    f = param_fields(D, with_A=True) + (("loss_sum", ()),)
    return f + phi_fields(D, rank) if rank else f


def legacy_param_fields(D: int):
    return (("R", (D, D)), ("Q_re", (D, D)), ("Q_im", (D, D)))


def legacy_grad_fields(D: int):
    return (("Q_re", (D, D)), ("Q_im", (D, D)), ("R", (D, D)), ("loss_sum", ()))


def var_order(rank: int = 0):
    return RHO_VAR_ORDER if rank else VAR_ORDER


def var_fields(D: int, rank: int = 0):
    """The variable / Adam-slot buffer of cmps_psi_apply_step; rank > 0: of cmps_rho_apply_step (Wx, Wy [rank, D] in place of psi_x, psi_y)."""
    shapes = {"A": (), "Rx": (D, D), "Ry": (D, D), "freqs": (D,), "psi_x": (D,), "psi_y": (D,), "Wx": (rank, D), "Wy": (rank, D)}
    return tuple((k, shapes[k]) for k in var_order(rank))


def size(fields) -> int:
    return sum(math.prod(shape) for _, shape in fields)


def offsets(fields):
    """Element offset of every field."""
    out, o = [], 0
    for _, shape in fields:
        out.append(o)
        o += math.prod(shape)
    return out


def pointers(base: int, fields):
    """Address of every field of a float32 buffer that starts at `base`."""
    return [base + FLOAT_BYTES * o for o in offsets(fields)]


def pack(fields, values, out=None) -> np.ndarray:
    """{field: array} -> flat float32 buffer (into `out` if given)."""
    if out is None:
        return np.concatenate([np.asarray(values[k], dtype=np.float32).ravel() for k, _ in fields])
    for (k, shape), o in zip(fields, offsets(fields)):
        out[o:o + math.prod(shape)] = np.asarray(values[k], dtype=np.float32).ravel()
    return out


def unpack(fields, flat) -> dict:
    """Flat buffer -> {field: view of its shape} (a scalar field gives the element)."""
    flat = np.asarray(flat)
    return {k: flat[o:o + math.prod(shape)].reshape(shape) if shape else flat[o]
            for (k, shape), o in zip(fields, offsets(fields))}


def split(name: str, z) -> dict:
    """Complex array -> its two planar fields."""
    z = np.asarray(z)
    return {name + "_re": z.real, name + "_im": z.imag}


def join(g: dict, name: str) -> np.ndarray:
    return g[name + "_re"] + 1j * g[name + "_im"]


def grad_size(D: int, rank: int = 0) -> int:
    return size(grad_fields(D, rank))


def unpack_grad(flat, D: int, rank: int = 0) -> dict:
    """Flat buffer of cmps_psi_loss_bwd (rank > 0: cmps_rho_loss_bwd, adds "phibar" [rank, D]) -> dict (sums over clips)."""
    g = unpack(grad_fields(D, rank), flat)
    out = {"Rbar": join(g, "R"), "fbar": g["freqs"], "psi0bar": join(g, "psi0"), "Abar": g["A"], "loss_sum": g["loss_sum"]}
    if rank:
        out["phibar"] = join(g, "phi")
    return out
