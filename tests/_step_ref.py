"""Float64 reference of the optimiser half of a training step (CPU only: numpy + torch float64 autograd; nothing from oracle/).

The raw -> effective map is restated from the reference model (model.py:36-42, 49, 221-222, 128-130, 327-334) and differentiated
AUTOMATICALLY: the hand-derived adjoint that audio_mps_amd/model.py (chain_rule), cmps_opt.hip (k_apply_step, k_rho_apply_step) and
oracle/ each write out -- the row-broadcast diagonal removal, the psi_0 normalisation with its 1e-12 floor, phi = conj(W) / |W| -- is
not written here a fourth time.  Complex tensors are planar (``x_re``, ``x_im``) under the field names of audio_mps_amd.layout, and the
cotangent convention is layout.unpack_grad's: bar = d/d re + i d/d im, so <bar, field> = bar_re field_re + bar_im field_im."""
from __future__ import annotations

import math

import numpy as np
import torch

from audio_mps_amd import layout

PSI_FLOOR = 1e-12                                      # epsilon of _normalize_psi (model.py:327)


def _t64(x, requires_grad=False):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, requires_grad=requires_grad)


def effective(variables, c_r, c_h, rank):
    """{raw variable: float64 tensor} -> {effective field: float64 tensor}: R_re, R_im, freqs, A and (rank = 0) psi0_re, psi0_im or
    (rank > 0) phi_re, phi_im [rank, D]."""
    zx, zy = c_r * variables["Rx"], c_r * variables["Ry"]                     # model.py:36-41 (c_r = 1: R_in was given)
    out = {"R_re": zx - torch.diagonal(zx)[None, :],                          # model.py:42: the diagonal broadcasts as a ROW
           "R_im": zy - torch.diagonal(zy)[None, :],
           "freqs": c_h * variables["freqs"],                                 # model.py:49
           "A": variables["A"]}
    if rank == 0:
        x, y = variables["psi_x"], variables["psi_y"]                         # model.py:221-222, 327-334
        inv = 1.0 / torch.sqrt(torch.maximum(torch.sum(x * x + y * y), _t64(PSI_FLOOR)))
        out["psi0_re"], out["psi0_im"] = x * inv, y * inv
    else:
        x, y = variables["Wx"], variables["Wy"]                               # model.py:127-130: rho_0 = W^dagger W / tr, as columns
        nrm = torch.sqrt(torch.sum(x * x + y * y))
        out["phi_re"], out["phi_im"] = x / nrm, -y / nrm
    return out


def objective(variables, grad_sums, batch, h_reg, r_reg, c_r, c_h, rank, with_reg):
    """(L, reported total) as float64 tensors.  L = loss_sum / B + sum_fields <bar / B, effective field> (+ regularisers) is the
    function whose gradient w.r.t. the raw variables a training step needs; the total is L without the linear terms."""
    D = variables["Rx"].shape[0]
    g = layout.unpack(layout.grad_fields(D, rank), np.asarray(grad_sums, dtype=np.float64))
    eff = effective(variables, c_r, c_h, rank)
    total = _t64(g["loss_sum"] / batch)
    if with_reg:                                                              # train.py:55-60, on the effective R and freqs
        total = total + h_reg * torch.sum(eff["freqs"] ** 2) + r_reg * torch.sum(eff["R_re"] ** 2 + eff["R_im"] ** 2)
    L = total
    for k in eff:                                                             # (rank > 0: the two psi_0 blocks are not read)
        L = L + torch.sum(_t64(g[k] / batch) * eff[k])
    return L, total


def total_and_grads(variables, grad_sums, batch, h_reg, r_reg, c_r, c_h, rank, with_reg=True):
    """-> (reported total, {raw variable: dL / d variable}) in float64, the gradient from backward()."""
    v = {k: _t64(variables[k], requires_grad=True) for k in layout.var_order(rank)}
    L, total = objective(v, grad_sums, batch, float(h_reg), float(r_reg), float(c_r), float(c_h), rank, with_reg)
    L.backward()
    return float(total.detach()), {k: (v[k].grad.numpy().copy() if v[k].grad is not None else np.zeros(v[k].shape)) for k in v}


def adam64(var, m, v, g, lr, b1, b2, eps, t):
    """Textbook Adam (train.py:89) in float64 -> (var, m, v) after step t; ``g`` is the float32 gradient cast up."""
    var, m, v, g = (np.asarray(x, dtype=np.float64) for x in (var, m, v, g))
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return var - lr_t * m / (np.sqrt(v) + eps), m, v


def _ordered(a):
    """float32 -> int64 that grows with the value: the bit pattern, sign-magnitude folded, so that +0 and -0 both map to 0."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    """Elementwise distance of two float32 arrays in units in the last place (the count of floats between them); +0 == -0.  A NaN
    is 0 away from a NaN and 2^32 away from anything else."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    d = np.abs(_ordered(a) - _ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, np.where(na & nb, 0, 2 ** 32), d)
