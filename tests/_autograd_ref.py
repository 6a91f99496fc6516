"""Float64 twins of the three loss folds, differentiated AUTOMATICALLY (CPU only: numpy + torch float64 / complex128; nothing from oracle/).

The reference defines its gradients as TensorFlow's automatic differentiation of the forward fold (train.py:89).  oracle/ and the HIP
kernels each derive that reverse sweep by hand, from the same derivation; here only the forwards are written -- from the reference's
text, statement by statement, the lines cited on the right -- and every gradient comes from ``backward()``.  What has to be trusted
is the forward of each model, which can be read against model.py (legacy: SURVEY.md Appendix A) line by line.  (tests/_step_ref.py
does the same for the optimiser half of a step.)

Grid modes, stated here and not imported:
  "f64"     float64 throughout: dt, the running time and every constant are Python doubles.
  "f64t32"  float64 arithmetic on the reference's float32 time grid, the float64 evaluation of the problem the kernels solve:
              * t is the float32 running sum t += dt with dt = float32(delta_t)        (model.py:16, :266, :281),
              * a Python-float constant the reference casts to float32 / complex64 enters as that float32 value
                (-delta_t * sigma^2 formed in double, model.py:312; delta_t and sigma^2 one by one, model.py:184; legacy: dt),
            everything else is float64.
In both modes the increments are the FLOAT32 differences of the float32 clip (model.py:263, :138: the data tensor is float32), cast up.

Cotangent convention (audio_mps_amd.layout.unpack_grad): for a complex z = x + i y the leaves are x and y, and zbar = dL/dx + i dL/dy.
The floors are ``torch.maximum(value, constant)``: on the floored branch the gradient goes to the constant, as tf.maximum's does.

The check functions at the end take (kernel result, twin result, float32-oracle result) and return records (quantity, error, bar);
they need numpy only, so tests/test_autograd_host.py can show on the CPU that they reject a wrong kernel (tests/_sweep.py has the same
draw / check / run split).  The bars are those of tests/test_gpu_accuracy.py, unchanged:
    loss                 max(1e-5, 1.5 |oracle_f32 - twin|)   of max(|loss_b|, 1)
    each gradient tensor max(1e-4, 1.5 |oracle_f32 - twin|)   of the tensor's max
    A (one scalar)       max(1e-4, 2 |oracle_f32 - twin|)     as tests/_sweep.py prices it (_dA_bar)
"""
from __future__ import annotations

import numpy as np
import torch

FLOOR = 1e-12                                          # epsilon of _normalize_psi / _normalize_rho (model.py:327, :198)
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4                        # tests/test_gpu_accuracy.py: LOSS_RTOL, GRAD_RTOL
OWN_FACTOR, A_FACTOR = 1.5, 2.0                        # ... its factor on the float32 oracle's own distance; tests/_sweep.py::_dA_bar's


# ---------------------------------------------------------------------------------------------------
# the grid rules
# ---------------------------------------------------------------------------------------------------
def const32(x, grid):
    """A Python-float constant that the reference turns into a float32 value: that value in "f64t32", itself in "f64"."""
    if grid not in ("f64", "f64t32"):
        raise ValueError(grid)
    return float(np.float32(x)) if grid == "f64t32" else float(x)


def time_grid(delta_t, steps, grid):
    """t_0 = 0, t_{k+1} = t_k + dt [steps] as float64 values: summed in float32 from dt = float32(delta_t) in "f64t32"
    (model.py:16 ``tf.constant(delta_t, tf.float32)``, :266 the initial 0., :281 ``t += self.dt``), in float64 in "f64"."""
    if grid not in ("f64", "f64t32"):
        raise ValueError(grid)
    real = np.float32 if grid == "f64t32" else np.float64
    t, acc, dt = np.empty(steps, dtype=np.float64), real(0), real(delta_t)
    for k in range(steps):
        t[k] = acc
        acc = real(acc + dt)
    return t


def _leaf(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, requires_grad=True)


def _increments(audio):
    """model.py:263 / :138: data[:, 1:] - data[:, :-1] on the float32 clip, as a float64 tensor [B, T - 1]."""
    a = np.asarray(audio, dtype=np.float32)
    return torch.from_numpy((a[:, 1:] - a[:, :-1]).astype(np.float64))


def _phases(freqs, t):
    """exp(1j * freqs * t) (model.py:305, :178): the argument is the product freqs * t, the exponential of a purely imaginary number."""
    th = freqs * t
    return torch.complex(torch.cos(th), torch.sin(th))


def _floor():
    return torch.tensor(FLOOR, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------
# PsiCMPS: model.py:257-334
# ---------------------------------------------------------------------------------------------------
def psi_losses(audio, R_re, R_im, freqs, psi0_re, psi0_im, A, delta_t, sigma, grid="f64t32", times=None, maximum=torch.maximum,
               aux=None):
    """Per-clip loss [B] of PsiCMPS on the effective parameters (float64 tensors; R after model.py:42, psi_0 as the scan starts from it).
    ``times`` replaces the grid's time table and ``maximum`` the floor operation: the seams tests/test_autograd_host.py builds its wrong
    "kernels" with.  ``aux`` (a dict) receives "norm" [B, T - 1], sum |psi'|^2 of every step before the floor."""
    x = _increments(audio)                                                     # :263
    B, N = x.shape
    R = torch.complex(R_re, R_im)                                              # :41-42, as given
    psi = torch.complex(psi0_re, psi0_im)[None, :].expand(B, -1)               # :260  stack(batch_size * [psi_0])
    loss = torch.zeros(B, dtype=torch.float64)                                 # :261
    t = time_grid(delta_t, N, grid) if times is None else np.asarray(times, dtype=np.float64)       # :266, :281
    cc = const32(-delta_t * sigma ** 2, grid)                                  # :312  the Python product, then the cast
    norms = []
    for k in range(N):                                                         # :265  foldl over the increments
        s = x[:, k] / A                                                        # :303
        ph = _phases(freqs, float(t[k]))                                       # :304-305
        U = psi * torch.conj(ph)                                               # :306
        V = U @ R.T                                                            # :309  einsum('bc,ac->ab', R, Upsi)
        W = V @ torch.conj(R)                                                  # :308, :310  einsum('bc,ac->ab', adjoint(R), RUpsi)
        delta = cc * W / 2.0 + s[:, None] * V                                  # :312-313
        psi = psi + ph * delta                                                 # :315-317  (:278: not normalised yet)
        Up = psi * torch.conj(ph)                                              # :322-323, on the updated psi at the same t
        e = 2.0 * torch.sum(torch.conj(Up) * (Up @ R.T), dim=1).real           # :324-325
        loss = loss + -torch.log(1.0 + e * x[:, k] / A)                        # :279, :294
        ss = torch.sum(psi.real ** 2 + psi.imag ** 2, dim=1, keepdim=True)     # :331  square(abs(x)) summed over axis 1
        psi = psi * torch.rsqrt(maximum(ss, _floor()))                         # :280, :332-334
        norms.append(ss.detach()[:, 0])
    if aux is not None:
        aux["norm"] = torch.stack(norms, dim=1).numpy() if norms else np.zeros((B, 0))
    return loss


def psi_twin(audio, R, freqs, psi0, A, delta_t, sigma, grid="f64t32", **seams):
    """The twin of cmps_psi_loss_bwd: dict(per_clip [B], Rbar [D, D] complex, fbar [D], psi0bar [D] complex, Abar, loss_sum), the
    gradients of sum_b loss_b w.r.t. the effective parameters (the keys of layout.unpack_grad), from backward()."""
    R, psi0 = np.asarray(R, dtype=np.complex128), np.asarray(psi0, dtype=np.complex128)
    lv = {"R_re": _leaf(R.real), "R_im": _leaf(R.imag), "freqs": _leaf(freqs), "psi0_re": _leaf(psi0.real), "psi0_im": _leaf(psi0.imag),
          "A": _leaf(A)}
    per = psi_losses(audio, lv["R_re"], lv["R_im"], lv["freqs"], lv["psi0_re"], lv["psi0_im"], lv["A"], delta_t, sigma, grid, **seams)
    torch.sum(per).backward()
    g = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape)) for k, v in lv.items()}
    return {"per_clip": per.detach().numpy().copy(), "Rbar": g["R_re"] + 1j * g["R_im"], "fbar": g["freqs"],
            "psi0bar": g["psi0_re"] + 1j * g["psi0_im"], "Abar": float(g["A"]), "loss_sum": float(per.detach().sum())}


# ---------------------------------------------------------------------------------------------------
# RhoCMPS: model.py:127-130, 132-203, the reference's lab-frame matrix form
# ---------------------------------------------------------------------------------------------------
def rho_losses(audio, R_re, R_im, freqs, Wx, Wy, A, delta_t, sigma, grid="f64t32", aux=None):
    """Per-clip loss [B] of RhoCMPS on the effective R, freqs and the raw Wx, Wy [rank, D].  ``aux`` receives "norm" [B, T - 1], the
    trace of every step's rho before it is normalised."""
    x = _increments(audio)                                                     # :138
    B, N = x.shape
    R = torch.complex(R_re, R_im)
    D = R.shape[0]
    W = torch.complex(Wx, Wy)                                                  # :127
    r0 = torch.conj(W).T @ W                                                   # :128  matmul(W, W, adjoint_a=True)
    rho = (r0 / torch.trace(r0))[None].expand(B, -1, -1)                       # :129, :135
    loss = torch.zeros(B, dtype=torch.float64)                                 # :136
    t = time_grid(delta_t, N, grid)                                            # :141 initial 0., :157
    c = -0.5 * const32(delta_t, grid) * const32(sigma ** 2, grid)              # :184  - 0.5 * . * self.delta_t * self.sigma**2
    eye = torch.eye(D, dtype=torch.complex128)
    traces = []
    for k in range(N):                                                         # :140  foldl
        s = x[:, k] / A                                                        # :175
        ph = _phases(freqs, float(t[k]))                                       # :176, :178
        Rt = ph[:, None] * R * torch.conj(ph)[None, :]                         # :179  einsum('a,ab,b->ab')
        RRd = torch.conj(Rt).T @ Rt                                            # :180  matmul(Rt, Rt, adjoint_a=True)
        U = eye[None] + (c * RRd)[None] + s[:, None, None] * Rt[None]          # :181-184
        rho = U @ rho @ torch.conj(U).transpose(1, 2)                          # :185-186
        X = Rt + torch.conj(Rt).T                                              # :193-194, at the same t (:155)
        e = torch.einsum("ab,cba->c", X, rho).real                             # :195-196  trace(einsum('ab,cbd->cad'))
        loss = loss + -torch.log(1.0 + e * x[:, k] / A)                        # :155, :170
        tr = torch.einsum("caa->c", rho).real                                  # :200-201
        rho = rho / torch.maximum(tr, _floor())[:, None, None]                 # :201-203
        traces.append(tr.detach())
    if aux is not None:
        aux["norm"] = torch.stack(traces, dim=1).numpy() if traces else np.zeros((B, 0))
    return loss


def rho_twin(audio, R, freqs, Wx, Wy, A, delta_t, sigma, grid="f64t32", aux=None):
    """The twin of RhoCMPS.loss_and_grads before the raw -> effective map: dict(per_clip, loss, Rbar, fbar, Abar, Wx, Wy), the gradients
    of mean_b loss_b w.r.t. the effective R, freqs, A and the raw Wx, Wy."""
    R = np.asarray(R, dtype=np.complex128)
    lv = {"R_re": _leaf(R.real), "R_im": _leaf(R.imag), "freqs": _leaf(freqs), "Wx": _leaf(Wx), "Wy": _leaf(Wy), "A": _leaf(A)}
    per = rho_losses(audio, lv["R_re"], lv["R_im"], lv["freqs"], lv["Wx"], lv["Wy"], lv["A"], delta_t, sigma, grid, aux=aux)
    torch.mean(per).backward()                                                 # :142
    g = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(v.shape)) for k, v in lv.items()}
    return {"per_clip": per.detach().numpy().copy(), "loss": float(per.detach().mean()), "Rbar": g["R_re"] + 1j * g["R_im"],
            "fbar": g["freqs"], "Abar": float(g["A"]), "Wx": g["Wx"], "Wy": g["Wy"]}


# ---------------------------------------------------------------------------------------------------
# legacy AudioMPS: SURVEY.md Appendix A (rows "H symmetrisation" ... "Result")
# ---------------------------------------------------------------------------------------------------
def legacy_losses(audio, H, R, dt, grid="f64t32", aux=None):
    """Per-clip loss [B] of the legacy arithmetic on the raw real H, R [D, D]."""
    x = _increments(audio)                                                     # "Increments"
    B, N = x.shape
    D = R.shape[0]
    dt = const32(dt, grid)                                                     # the graph's float32 constants 0.01 ("Step: update")
    L = torch.tril(H)
    Hs = L + L.T                                                               # "H symmetrisation": band_part(H, -1, 0) + its transpose
    Q = torch.complex(-(R.T @ R) / 2.0, -Hs) * dt                              # "Step: update": Q = dt (-i H_s - R^T R / 2)
    Rc = torch.complex(R, torch.zeros_like(R))
    psi = torch.zeros((B, D), dtype=torch.complex128)
    psi[:, 0] = 1.0                                                            # "psi_0": one_hot(0, D), per clip
    loss = torch.zeros(B, dtype=torch.float64)
    norms = []
    for k in range(N):
        v = psi @ Rc.T
        e = 2.0 * torch.sum(torch.conj(psi) * v, dim=1).real                   # "Step: expectation", on the pre-update normalised psi
        loss = loss + (x[:, k] - e) ** 2 / 2.0                                 # "Step: loss"
        y = psi + psi @ Q.T + (dt * x[:, k])[:, None] * v                      # "Step: update": psi + Q psi + dt x (R psi)
        ss = torch.sum(y.real ** 2 + y.imag ** 2, dim=1, keepdim=True)
        psi = y * torch.rsqrt(torch.maximum(ss, _floor()))                     # "Step: normalise"
        norms.append(ss.detach()[:, 0])
    if aux is not None:
        aux["norm"] = torch.stack(norms, dim=1).numpy() if norms else np.zeros((B, 0))
    return loss


def legacy_twin(audio, H, R, dt, grid="f64t32"):
    """The twin of LegacyAudioMPS.loss_and_grads: dict(per_clip, loss, gH, gR), the gradients of mean_b loss_b ("Result")."""
    h, r = _leaf(H), _leaf(R)
    per = legacy_losses(audio, h, r, dt, grid)
    torch.mean(per).backward()
    return {"per_clip": per.detach().numpy().copy(), "loss": float(per.detach().mean()),
            "gH": h.grad.numpy().copy() if h.grad is not None else np.zeros(h.shape), "gR": r.grad.numpy().copy()}


# ---------------------------------------------------------------------------------------------------
# the checks: (kernel result, twin result, float32-oracle result) -> records (quantity, error, bar)
# ---------------------------------------------------------------------------------------------------
PSI_KEYS = ("Rbar", "fbar", "psi0bar", "Abar")         # effective-parameter sums of cmps_psi_loss_bwd (layout.unpack_grad)
RHO_KEYS = ("A", "Rx", "Ry", "freqs", "Wx", "Wy")      # RhoCMPS.loss_and_grads
LEGACY_KEYS = ("gH", "gR")                             # LegacyAudioMPS.loss_and_grads, under the oracle's names
SCALAR_KEYS = ("A", "Abar")                            # one scalar made of two large cancelling sums: its own price


def rel_inf(a, b):
    """max |a - b| / max |b| in double precision (0 where both vanish)."""
    wide = np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64
    a, b = np.asarray(a, dtype=wide), np.asarray(b, dtype=wide)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def loss_err(per, ref):
    """max_b |per_b - ref_b| / max(|ref_b|, 1)."""
    per, ref = np.asarray(per, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(per - ref) / np.maximum(np.abs(ref), 1.0)))


def own_distances(twin, ref32, keys):
    """{quantity: |oracle_f32 - twin|}: the float32 restatement's own rounding on this draw, in the units of the records."""
    own = {"loss": loss_err(ref32["per_clip"], twin["per_clip"])}
    own.update({k: rel_inf(ref32[k], twin[k]) for k in keys})
    return own


def check(result, twin, ref32, keys, extra=0.0):
    """Records (quantity, |result - twin|, bar) for the per-clip loss and every tensor of ``keys``; ``extra`` widens the bars of the
    tensors that are not scalars (the project's existing 3e-5 of the two-piece bf16 rank-1 sums).  A non-finite error fails its bar."""
    own = own_distances(twin, ref32, keys)
    rec = [("loss", loss_err(result["per_clip"], twin["per_clip"]), max(LOSS_BAR, OWN_FACTOR * own["loss"]))]
    for k in keys:
        if k in SCALAR_KEYS:
            bar = max(GRAD_BAR, A_FACTOR * own[k])                             # tests/_sweep.py::_dA_bar
        else:
            bar = max(GRAD_BAR, OWN_FACTOR * own[k]) + extra
        rec.append((k, rel_inf(result[k], twin[k]), bar))
    return rec


def check_psi(result, twin, ref32, extra=0.0):
    return check(result, twin, ref32, PSI_KEYS, extra)


def check_rho(result, twin, ref32, extra=0.0):
    return check(result, twin, ref32, RHO_KEYS, extra)


def check_legacy(result, twin, ref32, extra=0.0):
    return check(result, twin, ref32, LEGACY_KEYS, extra)


def failures(records):
    """The records whose error is above its bar (or not a number)."""
    return [r for r in records if not r[1] <= r[2]]


def report(label, records, own):
    """One printed line per record: both distances, |result - twin| and |oracle_f32 - twin|, and the bar."""
    for what, err, bar in records:
        print(f"{label} {what:8s} |hip - twin| {err:.2e}   |f32 - twin| {own[what]:.2e}   bar {bar:.2e}")


# ---------------------------------------------------------------------------------------------------
# raw <- effective, by automatic differentiation of tests/_step_ref.py::effective
# ---------------------------------------------------------------------------------------------------
def raw_gradients(variables, bars, c_r, c_h):
    """{raw variable: gradient} from the cotangents ``bars`` = dict(Rbar complex [D, D], fbar [D], Abar and, for PsiCMPS, psi0bar complex
    [D]) of the effective R, freqs, A, psi_0: the vector-Jacobian product of _step_ref.effective (model.py:36-42, 49, 221-222), from
    backward() -- not the oracle's chain rule.  ``variables`` needs Rx, Ry, freqs, A (and psi_x, psi_y next to a psi0bar)."""
    import _step_ref as SR
    names = ("Rx", "Ry", "freqs", "A") + (("psi_x", "psi_y") if "psi0bar" in bars else ())
    v = {k: _leaf(variables[k]) for k in names}
    probe = v if "psi0bar" in bars else dict(v, psi_x=torch.ones(1, dtype=torch.float64), psi_y=torch.zeros(1, dtype=torch.float64))
    eff = SR.effective(probe, float(c_r), float(c_h), 0)
    cot = {"R_re": np.real(bars["Rbar"]), "R_im": np.imag(bars["Rbar"]), "freqs": bars["fbar"], "A": bars["Abar"]}
    if "psi0bar" in bars:
        cot.update({"psi0_re": np.real(bars["psi0bar"]), "psi0_im": np.imag(bars["psi0bar"])})
    L = sum(torch.sum(torch.from_numpy(np.array(c, dtype=np.float64)) * eff[k]) for k, c in cot.items())
    L.backward()
    return {k: v[k].grad.numpy().copy() for k in v}
