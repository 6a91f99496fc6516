"""cmps_noise_fill on a real MI355X: k_noise_philox (a) element by element against the numpy restatement of the definition
(tests/_noise_ref.py), (b) its memory contract in guarded buffers (tests/_guard.py), (c) NoisePlan / device-tensor noise through every
sampler entry of HipScan against the same calls handed the downloaded array, (d) streams opened with device_noise=True, whose waveform
no cut changes, (e) the kernel's name in cmps_kernel_times.

Bar of (a), the project's form for a float32 result judged against float64 (tests/test_gpu_stream.py):
  max |hip - f64| <= 4 * max |ref32 - f64| + 2e-6 * stddev,   ref32 the reference evaluated in float32.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _guard as G
import _noise_ref as NR
import _primed_ref as PR
from test_gpu_primed import AUTO, BLOCK, WAVE, WIDE, _model
from test_gpu_rho_primed import _model as _rho_model

pytestmark = pytest.mark.gpu

SEED = 20261019
STD_SMALL = float(np.float32(0.0123))          # (what the C ABI's float argument holds)
# (n, length, first_step, first_path, seed)
CASES = [(1, 1, 0, 0, SEED),
         (3, 5, 3, 0, SEED),                   # odd rows: no row base aligned
         (2, 64, 0, 0, SEED),                  # the all-aligned path
         (3, 67, 2 ** 34 - 3, 0, SEED),        # across the 32-bit counter word
         (5, 1000, 1, 2 ** 32 - 5, SEED),      # the last paths a 32-bit word reaches
         (1, 2 ** 20, 0, 0, SEED),
         (2, 4, 0, 0, 2 ** 64 - 1)]


@functools.lru_cache(maxsize=None)
def _unit(n, length, first_step, first_path, seed, dtype):
    """The reference's unit normals [n, length] of a case: computed once, shared, never written to."""
    z = np.stack([NR.normals(seed, first_path + b, first_step, length, dtype) for b in range(n)])
    z.setflags(write=False)
    return z


def _backend(D=8, variant=AUTO):
    from audio_mps_amd.scan import HipScan
    return HipScan(D, variant=variant)


@pytest.mark.parametrize("std", [1.0, STD_SMALL])
@pytest.mark.parametrize("n,length,first_step,first_path,seed", CASES)
def test_noise_matches_the_reference(n, length, first_step, first_path, seed, std):
    """(a) on a fresh handle, before any cmps_set_params.

    Measured on an MI355X (cases in the order of CASES; stddev 1 | stddev 0.0123):
      n  length  first_step  first_path  seed      |hip - f64|  |ref32 - f64|  bar        |  |hip - f64|  |ref32 - f64|  bar
      1  1       0           0           20261019  1.380e-07    1.004e-07      2.402e-06  |  2.094e-09    1.631e-09      3.112e-08
      3  5       3           0           20261019  5.949e-08    4.438e-07      3.775e-06  |  8.776e-10    5.586e-09      4.694e-08
      2  64      0           0           20261019  2.319e-07    5.293e-07      4.117e-06  |  2.738e-09    6.579e-09      5.092e-08
      3  67      2^34-3      0           20261019  3.219e-07    1.110e-06      6.438e-06  |  5.045e-09    1.352e-08      7.868e-08
      5  1000    1           2^32-5      20261019  3.602e-07    8.390e-07      5.356e-06  |  5.296e-09    1.051e-08      6.665e-08
      1  2^20    0           0           20261019  6.202e-07    1.562e-06      8.246e-06  |  9.475e-09    1.929e-08      1.018e-07
      2  4       0           0           2^64-1    6.317e-08    8.960e-08      2.358e-06  |  1.643e-09    1.643e-09      3.117e-08"""
    be = _backend()
    got = be.draw_noise(seed, first_step, n, length, std, first_path=first_path)
    assert got.shape == (n, length) and got.dtype == torch.float32 and got.is_cuda
    hip = got.cpu().numpy().astype(np.float64)
    f64 = std * _unit(n, length, first_step, first_path, seed, np.float64)
    ref32 = (np.float32(std) * _unit(n, length, first_step, first_path, seed, np.float32)).astype(np.float64)
    d_hip, d_ref = float(np.max(np.abs(hip - f64))), float(np.max(np.abs(ref32 - f64)))
    bar = 4.0 * d_ref + 2e-6 * std
    print(f"noise n={n} length={length} first_step={first_step} first_path={first_path} seed={seed} std={std:.4g}: "
          f"|hip - f64| {d_hip:.3e}  |ref32 - f64| {d_ref:.3e}  bar {bar:.3e}")
    assert np.all(np.isfinite(hip)) and float(np.max(np.abs(hip))) <= 5.7682 * std * (1 + 1e-6)
    assert d_hip <= bar


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("n,length,first_step", [(3, 5, 3), (2, 64, 0), (7, 33, 2)])
def test_noise_memory_contract(n, length, first_step, offset):
    """(b) the payload is fully written, both zones stay intact, and where the payload sits changes no value.  offset 0: a 256-byte aligned
    payload; offset 4: the address handed over is 4 bytes behind a 256-byte boundary (the payload's first element then belongs to the
    caller and must keep its pattern), so no row base is 16-byte aligned unless its row's own offset makes it so."""
    from audio_mps_amd import _capi
    lib = _capi.load()
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    h = ctypes.c_void_p()
    assert lib.cmps_create(8, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        g = G.Guarded(4 * n * length + offset, dev, align=256, fill=G.NAN_FILL, name="noise")
        assert g.ptr % 256 == 0
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        code = lib.cmps_noise_fill(h, SEED, first_step, 0, n, length, 1.0, g.ptr + offset, stream)
        assert code == _capi.CMPS_OK, lib.cmps_last_error(h)
        torch.cuda.synchronize(dev)
        assert g.zones_intact() is None, g.zones_intact()
        left = g.untouched_mask(torch.float32).cpu().numpy()
        assert left.shape == (n * length + offset // 4,) and left[:offset // 4].all() and not left[offset // 4:].any(), np.nonzero(left)[0]
        got = g.numpy(np.float32)[offset // 4:].reshape(n, length)
    finally:
        lib.cmps_destroy(h)
    want = _backend().draw_noise(SEED, first_step, n, length, 1.0).cpu().numpy()
    assert np.array_equal(got, want)
    f64 = _unit(n, length, first_step, 0, SEED, np.float64)
    assert float(np.max(np.abs(got - f64))) <= 4.0 * float(np.max(np.abs(_unit(n, length, first_step, 0, SEED, np.float32) - f64))) + 2e-6


# ---------------------------------------------------------------------------------------------------
# (c) plumbing
# ---------------------------------------------------------------------------------------------------
def _psi_entries(D, variant, n):
    m = _model(D, n, variant)
    be = m._get_backend()
    return m, be, be.sample, be.sample_primed, be.stream, be.stream_state


def _rho_entries(D, rank, variant, n):
    m = _rho_model(D, rank, variant)
    be = m._get_backend()
    return m, be, be.rho_sample, be.rho_sample_primed, be.rho_stream, be.rho_stream_state


@pytest.mark.parametrize("kind,D,variant", [("psi", 20, WAVE), ("psi", 48, WIDE), ("psi", 32, BLOCK), ("rho", 8, AUTO), ("rho", 8, BLOCK)])
def test_plan_and_device_tensor_equal_the_downloaded_array(kind, D, variant):
    """(c) sample, sample_primed and a two-segment stream handed a NoisePlan, the device tensor [n, length] and the downloaded array in the
    host layout [length, n]: the same bits."""
    from audio_mps_amd.scan import NoisePlan
    n, L, P, seed = 3, 70, 21, 5
    m, be, sample, primed, stream, new_state = _psi_entries(D, variant, n) if kind == "psi" else _rho_entries(D, 3, variant, n)
    std = float(m.sigma) * float(np.sqrt(0.5 * m.delta_t))
    prime, _ = PR.case_inputs(D, P, L, n)
    m._prepare(n, P + L + 1, train=False)
    dev0, devP = be.draw_noise(seed, 0, n, L, std), be.draw_noise(seed, P, n, L, std)
    host0, hostP = np.ascontiguousarray(dev0.cpu().numpy().T), np.ascontiguousarray(devP.cpu().numpy().T)
    assert host0.shape == (L, n) and not np.array_equal(host0, hostP) and np.array_equal(host0[P:], hostP[:L - P])
    # plain
    want = sample(host0)
    assert want.shape == (n, L) and np.all(np.isfinite(want)) and not np.array_equal(want[0], want[1])
    assert np.array_equal(sample(NoisePlan(seed, 0, std), length=L, n=n), want)
    assert np.array_equal(sample(dev0), want)
    # primed: the first sampled step is table row P
    want, wpred = primed(prime, hostP, want_pred=True)
    out, pred = primed(prime, NoisePlan(seed, P, std), want_pred=True, length=L, n=n)
    assert np.array_equal(out, want) and np.array_equal(pred, wpred)
    out, pred = primed(prime, devP, want_pred=True)
    assert np.array_equal(out, want) and np.array_equal(pred, wpred)
    # a stream of two segments: (P forced, 30 sampled), (0, L - 30)
    def run(first, second, l1=None, l2=None):
        st = new_state(n)
        o1, p1 = stream(None, st, 0, prime, first, True, n=n, length=l1)
        o2, _ = stream(st, st, P + 30, None, second, False, n=n, length=l2)
        return np.concatenate([o1, o2], axis=1), p1, st.cpu().numpy()
    w_out, w_pred, w_rec = run(hostP[:30], hostP[30:])
    for args in ((NoisePlan(seed, P, std), NoisePlan(seed, P + 30, std), 30, L - 30),
                 (devP[:, :30].contiguous(), devP[:, 30:].contiguous())):
        out, pred, rec = run(*args)
        assert np.array_equal(out, w_out) and np.array_equal(pred, w_pred) and np.array_equal(rec, w_rec)
    with pytest.raises(ValueError):
        sample(NoisePlan(seed, 0, std))                                                 # a plan brings no shape
    with pytest.raises(ValueError):
        sample(dev0, length=L + 1)


# ---------------------------------------------------------------------------------------------------
# (d) streams
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 48])
def test_device_noise_stream_is_cut_independent(D):
    """(d) follow(33 steps), generate(65), generate(1), generate(64) against one generate(130) behind the same follow: waveform and state
    record bit-equal; two paths differ; two seeds differ."""
    n = 3
    m = _model(D, n, AUTO)
    clip, _ = PR.case_inputs(D, 33, 130, n)
    clip = clip[0]                                                                      # one signal under every path

    def run(seed, cuts):
        st = m.open_stream(n, 33 + 130, temp=0.5, seed=seed, device_noise=True)
        assert st.noise_seed == seed
        st.follow(clip)
        wave = np.concatenate([st.generate(k) for k in cuts], axis=1)
        assert st.position == 163
        return wave, st._state.cpu().numpy()

    w1, r1 = run(11, (65, 1, 64))
    w2, r2 = run(11, (130,))
    assert w1.shape == (n, 130) and np.all(np.isfinite(w1))
    assert np.array_equal(w1, w2) and np.array_equal(r1, r2) and r1.any()
    assert not np.array_equal(w1[0], w1[1]) and not np.array_equal(w1[1], w1[2])
    w3, _ = run(12, (130,))
    assert not np.array_equal(w3, w1)
    # ... and the primed sampler with the same seed draws the same noise (tables of another T: the bar of tests/test_gpu_stream.py (f))
    cont = m.continue_clip(clip, n, 130, temp=0.5, seed=11, device_noise=True)
    assert float(np.max(np.abs(cont - w1))) <= 2e-5 * max(1.0, float(np.max(np.abs(cont - clip[-1]))) * float(m.A)) / float(m.A)


def test_kernel_events_name_the_noise_kernel():
    """(e) k_noise_philox in cmps_kernel_times, once per draw."""
    from audio_mps_amd.scan import NoisePlan
    n, L = 2, 9
    m = _model(20, n, WAVE)
    be = m._prepare(n, L + 1, train=False)
    be.kernel_events(True)
    for k in range(3):
        be.draw_noise(1, k, n, L, 1.0)
    be.sample(NoisePlan(1, 0, 1e-3), length=L, n=n)
    times = be.kernel_times()
    assert list(times) == ["k_noise_philox", "k_sample_wave"]
    assert times["k_noise_philox"][1] == 4 and times["k_sample_wave"][1] == 1 and times["k_noise_philox"][0] > 0.0
