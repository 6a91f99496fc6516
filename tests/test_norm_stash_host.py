"""CPU side of the normalised stash rows (tests/test_gpu_norm_stash.py has the GPU side).

  * the C API's record of which rows a saved forward holds, as far as it can be reached without a device: CMPS_OPT_SAVED_ROWS is 0 on a
    handle that has saved nothing, read-only, and the reverse pass refuses to run without a saved forward;
  * the diagnostic switch that keeps (y, H y) rows (-DCMPS_DIAG -DCMPS_DIAG_YHY_ROWS, scripts/ablate.py) still compiles;
  * a numpy restatement of the chain wave's two forms of ybar_k.  k_bwd_wave2w on (y, H y) rows evaluates
        ybar = (yhb - dot yhp) inv + pre,   yhp = invok y,  pre = te (H y),  dot = rad_{k+1}
    and on normalised rows
        ybar = fma(yhb, inv, t),            t = fma(-q, yhat, p),  yhat = inv y,  p = te (H y),  q = rad_{k+1} [n > 1e-12] inv
    (inv = 1 / sqrt(max(n, 1e-12)), invok = [n > 1e-12] inv, te = 2 ebar, rad = 2 ebar e).  Both are the same real number; in float32 they
    differ by the roundings of at most ten operations, each relative 2^-24 to a term no larger than
    M = |yhb| inv + |rad yhat| inv + |p|, so |a - b| <= 10 * 2^-24 * M.
    The unit vectors yhat_k are the float32 oracle's states on the shapes of the GPU test; n_k, e_k follow from them with the model's
    H = R + R^dagger and step x_k R; the cotangent yhb (which the oracle does not expose) is drawn per step with |yhb| ~ 1.  One step per
    clip is put below the 1e-12 floor: q must be exactly 0 there."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import cmps_oracle as O
from _util import make_audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_saved_rows_option_without_a_device(hip_lib):
    from audio_mps_amd import _capi
    h = ctypes.c_void_p()
    assert hip_lib.cmps_create(32, ctypes.byref(h)) == _capi.CMPS_OK
    assert _capi.CMPS_OPT_SAVED_ROWS == 7
    assert hip_lib.cmps_get_option(h, _capi.CMPS_OPT_SAVED_ROWS) == 0                 # nothing saved yet
    assert hip_lib.cmps_set_option(h, _capi.CMPS_OPT_SAVED_ROWS, 1) == _capi.CMPS_ERR_BAD_ARG
    assert b"read-only" in hip_lib.cmps_last_error(h)
    # the settings that select the rows are plain options: changing them saves nothing and needs no device
    assert hip_lib.cmps_set_option(h, _capi.CMPS_OPT_BWD_WAVES, 1) == _capi.CMPS_OK
    assert hip_lib.cmps_set_option(h, _capi.CMPS_OPT_BWD_WAVES, 2) == _capi.CMPS_OK
    assert hip_lib.cmps_get_option(h, _capi.CMPS_OPT_SAVED_ROWS) == 0
    # no saved forward: the reverse pass is a call-order error whatever the options say
    assert hip_lib.cmps_psi_loss_bwd(h, None, 1, 2, None, None) == _capi.CMPS_ERR_STATE
    assert hip_lib.cmps_psi_states(h, 1, 2, None, None) == _capi.CMPS_ERR_STATE
    hip_lib.cmps_destroy(h)


def test_yhy_rows_diagnostic_switch_compiles(tmp_path):
    from audio_mps_amd import build
    out = os.path.join(tmp_path, "capi_diag.o")
    cmd = [build._hipcc()] + build._flags() + ["--cuda-host-only", "-c", "-DCMPS_DIAG", "-DCMPS_DIAG_YHY_ROWS",
                                               os.path.join(build.CSRC, "cmps_capi.hip"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]


f32 = np.float32


def _fma(a, b, c):
    """float32 fma: the float64 product of two float32 values is exact, one rounding of the sum is left (then to float32)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _rsq(n):
    return (1.0 / np.sqrt(n.astype(np.float64))).astype(f32)      # (rsq_newton is float32-faithful)


@pytest.mark.parametrize("N", [1, 2, 8, 9, 33, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [17, 32])
def test_two_forms_of_ybar_agree_to_float32_rounding(D, B, N):
    T = N + 1
    hp = O.HParams(minibatch_size=B, bond_dim=D, sigma=1e-4)
    var = O.init_variables(hp, seed=D + N)
    audio = make_audio(B, T, hp.delta_t, D + N)
    if B >= 3:
        audio[2] = audio[2, 0]                                   # a constant clip: te = 0, p = 0
    _, states = O.psi_loss_per_clip(hp, var, audio, "f32", return_states=True)       # [B, N, D] unit vectors
    R = np.asarray(O.effective_params(hp, var, "f32")[0]).astype(np.complex64)
    H = (R + np.conj(R.T)).astype(np.complex64)
    A = f32(var.A)
    rng = np.random.default_rng(1000 * D + 10 * N + B)
    x = (audio[:, 1:] - audio[:, :-1]).astype(f32)                # x_k, [B, N]
    prev = np.concatenate([states[:, :1], states[:, :-1]], axis=1).astype(np.complex64)
    ynorm = prev + (x / A)[..., None] * np.einsum("ij,bkj->bki", R, prev)           # (1 + s_k R) psi_{k-1}: the size of y_k
    n = np.sum(np.abs(ynorm) ** 2, axis=-1).astype(f32)           # [B, N]
    n[:, N // 2] = f32(3e-13)                                     # one step per clip below the floor
    yhat_c = states.astype(np.complex64)
    y_c = (yhat_c * np.sqrt(np.maximum(n, f32(1e-12)))[..., None]).astype(np.complex64)
    hy_c = np.einsum("ij,bkj->bki", H, y_c).astype(np.complex64)
    e = np.sum((np.conj(y_c) * hy_c).real, axis=-1).astype(f32)
    # the scalar stage in the kernels' operation order (cmps_wave_bwd2.hip::scal_commit)
    inv = _rsq(np.maximum(n, f32(1e-12)))
    ok = n > f32(1e-12)
    invok = np.where(ok, inv, f32(0))
    z = (e * x) / A
    zbar = f32(-1.0) / (f32(1.0) + z)
    te = f32(2.0) * (zbar * x / A)
    rad = te * e
    rad_next = np.concatenate([rad[:, 1:], np.zeros((B, 1), f32)], axis=1)             # rad_{k+1}; no step N
    q = np.where(ok, rad_next * inv, f32(0))
    assert np.all(q[:, N // 2] == 0)
    if B >= 3:
        assert np.all(te[2] == 0)
    worst = 0.0
    for comp in ("real", "imag"):
        y, hy = getattr(y_c, comp).astype(f32), getattr(hy_c, comp).astype(f32)
        yhb = rng.standard_normal(y.shape).astype(f32) / f32(np.sqrt(D))
        i_, io_, t_, rn_, q_ = (v[..., None] for v in (inv, invok, te, rad_next, q))
        # (y, H y) rows
        pre, yhp = t_ * hy, io_ * y
        a = (yhb - rn_ * yhp) * i_ + pre
        # normalised rows: yhat and p rounded by the forward, t and ybar one FMA each
        yhat, p = i_ * y, t_ * hy
        t = _fma(-np.broadcast_to(q_, yhat.shape), yhat, p)
        b = _fma(yhb, np.broadcast_to(i_, yhb.shape), t)
        M = np.abs(yhb) * i_ + np.abs(rn_ * yhat) * i_ + np.abs(p)
        bound = 10.0 * 2.0 ** -24 * M.astype(np.float64)
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
        assert np.all(diff <= bound), (comp, float(np.max(diff / np.maximum(bound, 1e-300))))
    print(f"D={D} B={B} N={N}: largest |a - b| / bound = {worst:.3f}")
