"""The device-resident training input on a real MI355X: k_batch_gather bit for bit against tests/_data_ref.gather in guarded buffers
(tests/_guard.py), k_damped_sine element by element against the numpy restatement of the definition, and the input end to end -- a
Trainer fed by ResidentDataset.batches against one fed the same batches as numpy arrays, and train.main with and without --device_data.

Bar of the damped sine, the one cmps_noise_fill is held to (tests/test_gpu_noise.py), the waveform's scale being 1:
  max |hip - f64| <= 4 * max |ref32 - f64| + 2e-6,   ref32 the float32 evaluation of tests/_data_ref.damped_sine.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _data_ref as DR
import _guard as G
from _util import make_audio

pytestmark = pytest.mark.gpu

SEED = 20261019
POISON = np.float32(-7.0e37)                   # what the source holds wherever no valid row may read


def _backend(D=8):
    from audio_mps_amd.scan import HipScan
    return HipScan(D)


class _Lib:
    """One libcmps handle on the current device and stream, every pointer a Guarded's."""

    def __init__(self, D=8):
        from audio_mps_amd import _capi
        self.capi, self.lib = _capi, _capi.load()
        self.dev = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.h = ctypes.c_void_p()
        assert self.lib.cmps_create(D, ctypes.byref(self.h)) == _capi.CMPS_OK

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def guarded(self, array, name):
        a = np.ascontiguousarray(array)
        g = G.Guarded(a.nbytes, self.dev, align=256, fill=G.NAN_FILL, name=name)
        g.load(a)
        g.snapshot(a)
        return g

    def ok(self, code):
        assert code == self.capi.CMPS_OK, self.lib.cmps_last_error(self.h)
        torch.cuda.synchronize(self.dev)

    def close(self):
        self.lib.cmps_destroy(self.h)


# ---------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------
def _source(N, L):
    rng = np.random.default_rng(N * 1000003 + L)
    data = rng.standard_normal((N, L)).astype(np.float32)
    data.view(np.uint32)[0, 0] = 0x7FC12345               # bits travel as they are: a NaN with a payload, a denormal, a negative zero
    data.view(np.uint32)[-1, -1] = 0x00000001
    data.view(np.uint32)[N // 2, L // 2] = 0x80000000
    return data


def _run_gather(data, index, offset, T, audio_offset=0, poison=True):
    """cmps_batch_gather in guarded buffers -> the uint32 bits of audio [B, T].  poison: the source the kernel sees holds POISON wherever
    no valid row reads, so a stray read would show in the output.  Every zone, every input and the caller's bytes in front of a shifted
    audio_dev are checked."""
    N, L = data.shape
    index = np.asarray(index, dtype=np.int32)
    offs = None if offset is None else np.asarray(offset, dtype=np.int32)
    B = index.size
    seen = np.array(data)
    if poison:
        mask = np.zeros(data.shape, dtype=bool)
        for i, o in zip(index, np.zeros(B, np.int64) if offs is None else offs):
            if 0 <= i < N and 0 <= o <= L - T:
                mask[i, o:o + T] = True
        seen[~mask] = POISON
    lib = _Lib()
    try:
        d, ix = lib.guarded(seen, "data"), lib.guarded(index, "index")
        of = None if offs is None else lib.guarded(offs, "offset")
        out = G.Guarded(4 * B * T + audio_offset, lib.dev, align=256, fill=G.NAN_FILL, name="audio")
        lib.ok(lib.lib.cmps_batch_gather(lib.h, d.ptr, N, L, ix.ptr, of.ptr if of is not None else None, B, T, out.ptr + audio_offset,
                                         lib.stream()))
        for g in (d, ix, out) + ((of,) if of is not None else ()):
            assert g.zones_intact() is None, (g.name, g.zones_intact())
        for g in (d, ix) + ((of,) if of is not None else ()):
            assert g.equals_snapshot() is None, g.name
        left = out.untouched_mask(torch.float32).cpu().numpy()
        assert left[:audio_offset // 4].all(), "the bytes in front of audio_dev were written"
        return out.numpy(np.uint32)[audio_offset // 4:].reshape(B, T)
    finally:
        lib.close()


# (N, L, B, T, offsets, index or None for 0 .. B - 1)
GATHER_CASES = [
    (1, 2, 1, 2, None, None),                                  # smallest shape
    (5, 67, 3, 67, None, [4, 0, 2]),                           # odd rows, no row base aligned
    (4, 64, 4, 64, None, [3, 1, 0, 2]),                        # the all-aligned path
    (6, 64, 5, 61, [0, 1, 2, 3, 3], [5, 4, 0, 2, 1]),          # every source misalignment against an unaligned destination
    (3, 4099, 2, 4096, [0, 3], [2, 0]),                        # a row longer than one workgroup pass, with head and tail
    (3, 32, 7, 32, None, [2, 0, 0, 1, 2, 2, 1]),               # B > N: repeated indices
    (2, 8205, 3, 8201, [0, 4, 1], [1, 0, 1]),                  # three chunks per row; rows 1, 2 start off a 16-byte boundary
    (3, 5, 2100, 3, "mod3", "mod3"),                           # more rows than blocks in flight: the kernel's stride over the rows
]


@pytest.mark.parametrize("N,L,B,T,offset,index", GATHER_CASES)
def test_gather_matches_the_reference_bit_for_bit(N, L, B, T, offset, index):
    data = _source(N, L)
    index = np.arange(B) % N if index in (None, "mod3") else index
    offset = np.arange(B) % (L - T + 1) if isinstance(offset, str) else offset
    got = _run_gather(data, index, offset, T)
    want = DR.gather(data, index, offset, T).view(np.uint32)
    assert got.shape == want.shape == (B, T) and np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_gather_into_an_audio_dev_shifted_by_4_bytes():
    """The all-aligned shape with audio_dev 4 bytes behind a 256-byte boundary: no row is 16-byte aligned any more, the first element
    of the buffer stays the caller's."""
    data = _source(4, 64)
    got = _run_gather(data, [3, 1, 0, 2], None, 64, audio_offset=4)
    assert np.array_equal(got, DR.gather(data, [3, 1, 0, 2], None, 64).view(np.uint32))
    got = _run_gather(data, [3, 1, 0, 2], [3, 0, 2, 1], 61, audio_offset=4)
    assert np.array_equal(got, DR.gather(data, [3, 1, 0, 2], [3, 0, 2, 1], 61).view(np.uint32))


@pytest.mark.parametrize("L,T", [(40, 33), (4200, 4100)])
def test_gather_bad_rows_are_nan_and_read_nothing(L, T):
    """index = [-1, 0, N, 2] and offset = [0, L - T + 1, 0, -1]: each alone (with a valid partner: rows 1, 3 / rows 0, 2 stay good) and
    both together (every row bad).  NaN rows exactly where the rule says (0x7fc00000 in every element), the neighbours correct, the zones
    intact, and the source poisoned outside the valid rows' windows."""
    N = 4
    data = _source(N, L)
    bad_index, bad_offset = [-1, 0, N, 2], [0, L - T + 1, 0, -1]
    for index, offset, nan_rows in ((bad_index, None, [0, 2]), (bad_index, [0, 1, 2, 3], [0, 2]), ([3, 1, 0, 2], bad_offset, [1, 3]),
                                    (bad_index, bad_offset, [0, 1, 2, 3]), ([2 ** 31 - 1, -2 ** 31, 1, 1], [0, 0, 2 ** 31 - 1, -2 ** 31], [0, 1, 2, 3])):
        got = _run_gather(data, index, offset, T)
        want = DR.gather(data, index, offset, T).view(np.uint32)
        assert np.array_equal(got, want)
        for b in range(4):
            assert bool(np.all(got[b] == 0x7FC00000)) == (b in nan_rows), (index, offset, b)


# ---------------------------------------------------------------------------------------------------
# damped sine
# ---------------------------------------------------------------------------------------------------
# (B, T, first_clip, seed)
SINE_CASES = [(1, 1, 0, SEED),
              (3, 5, 0, SEED),
              (2, 64, 0, SEED),
              (3, 67, 2 ** 32 - 1, SEED),                      # across the counter word
              (4, 4000, 5, 2 ** 64 - 1)]
# the kernel's two strides, which none of the shapes above reaches
STRIDE_CASES = [(66000, 1, 0, SEED),                           # more clips than blocks in flight: the stride over the clips
                (1, 70001, 0, SEED)]                           # a row longer than the grid: the stride along the row


@functools.lru_cache(maxsize=None)
def _sine(B, T, first_clip, seed, delta_t, dtype):
    """The reference's clips of a case: computed once, shared, never written to."""
    z = DR.damped_sine(seed, first_clip, B, T, delta_t, dtype)
    z.setflags(write=False)
    return z


def _check_sine(B, T, first_clip, seed, delta_t, delay_term=False):
    """cmps_damped_sine_fill on a fresh handle, into a guarded buffer: every element written and finite, the zones intact, the values
    within the bar (delay_term: see test_damped_sine_strides)."""
    lib = _Lib()
    try:
        out = G.Guarded(4 * B * T, lib.dev, align=256, fill=G.NAN_FILL, name="audio")
        lib.ok(lib.lib.cmps_damped_sine_fill(lib.h, seed, first_clip, B, T, delta_t, out.ptr, lib.stream()))
        assert out.zones_intact() is None, out.zones_intact()
        assert not out.untouched_mask(torch.float32).any()
        hip32 = out.numpy(np.float32).reshape(B, T)
    finally:
        lib.close()
    hip = hip32.astype(np.float64)
    f64, ref32 = _sine(B, T, first_clip, seed, delta_t, np.float64), _sine(B, T, first_clip, seed, delta_t, np.float32).astype(np.float64)
    d_hip, d_ref = float(np.max(np.abs(hip - f64))), float(np.max(np.abs(ref32 - f64)))
    bar = 4.0 * d_ref + 2e-6
    if delay_term:
        bar += (2 * np.pi * 261.6 + 10.0) * delta_t * 6.0 * 2.0 ** -24 * float(np.max(DR.delays(seed, first_clip, B, T)))
    print(f"damped sine B={B} T={T} first_clip={first_clip} seed={seed} delta_t={delta_t:.3e}: "
          f"|hip - f64| {d_hip:.3e}  |ref32 - f64| {d_ref:.3e}  bar {bar:.3e}")
    assert np.all(np.isfinite(hip)) and float(np.max(np.abs(hip))) <= 1.0
    assert d_hip <= bar
    # the same through HipScan, wherever torch puts the buffer
    got = _backend().damped_sine(seed, first_clip, B, T, delta_t)
    assert got.shape == (B, T) and got.dtype == torch.float32 and got.is_cuda and np.array_equal(got.cpu().numpy(), hip32)


@pytest.mark.parametrize("delta_t", [1.0 / 16000, 1.0 / 8000])
@pytest.mark.parametrize("B,T,first_clip,seed", SINE_CASES)
def test_damped_sine_matches_the_reference(B, T, first_clip, seed, delta_t):
    """The bar of the module docstring, as it stands.

    Measured on an MI355X (delta_t 1/16000 | 1/8000):
      B  T     first_clip  seed      |hip - f64|  |ref32 - f64|  bar        |  |hip - f64|  |ref32 - f64|  bar
      1  1     0           20261019  0.000e+00    0.000e+00      2.000e-06  |  0.000e+00    0.000e+00      2.000e-06
      3  5     0           20261019  3.973e-08    6.953e-08      2.278e-06  |  4.922e-08    6.633e-08      2.265e-06
      2  64    0           20261019  5.283e-07    5.134e-07      4.054e-06  |  9.473e-07    9.771e-07      5.908e-06
      3  67    2^32-1      20261019  6.244e-07    6.254e-07      4.502e-06  |  1.201e-06    1.199e-06      6.795e-06
      4  4000  5           2^64-1    1.008e-05    1.008e-05      4.233e-05  |  9.690e-06    9.688e-06      4.075e-05"""
    _check_sine(B, T, first_clip, seed, delta_t)


@pytest.mark.parametrize("delta_t", [1.0 / 16000, 1.0 / 8000])
@pytest.mark.parametrize("B,T,first_clip,seed", STRIDE_CASES)
def test_damped_sine_strides(B, T, first_clip, seed, delta_t):
    """Shapes large enough for the kernel's two grid strides.  At T = 70001 a delay is hundreds to thousands of samples, and there the
    bar above stops being a bound: it scales the error ref32 HAPPENED to make, while two correct float32 evaluations of
    delay = fl32(T / 200) * (-(logf(u0) + logf(u1))) may differ by the roundings of that line -- two logarithms good to 1 ulp each, a sum
    and a product to half an ulp: 3 * 2^-24 relative per evaluation, 6 * 2^-24 between two.  A delay error d shifts the waveform by
    |d/dt (sin(w t) exp(-t / 0.1))| * delta_t * d <= (w + 10) * delta_t * d, w = 2 pi 261.6.  So for these shapes the bar is
      4 * max |ref32 - f64| + 2e-6 + (w + 10) * delta_t * 6 * 2^-24 * max delay
    (for the shapes of test_damped_sine_matches_the_reference the added term stays below 5e-6: delays of at most 66 samples).
    Measured on an MI355X at (1, 70001), delta_t 1/16000 | 1/8000: |hip - f64| 1.480e-05 | 2.959e-05, |ref32 - f64| 7.252e-06 | 6.081e-06."""
    _check_sine(B, T, first_clip, seed, delta_t, delay_term=True)


def test_damped_sine_shard_is_a_slice_of_the_whole_fill():
    """Clips [2, 5) of a fill equal rows 2 .. 4 of the fill of [0, 8) bit for bit (row bases of another alignment: T = 67)."""
    be = _backend()
    for T in (67, 64):
        whole = be.damped_sine(SEED, 0, 8, T, 1.0 / 16000).cpu().numpy()
        part = be.damped_sine(SEED, 2, 3, T, 1.0 / 16000).cpu().numpy()
        assert np.array_equal(part.view(np.uint32), whole[2:5].view(np.uint32))
        assert not np.array_equal(whole[0], whole[1]) and np.any(whole != 0)
        assert not np.array_equal(be.damped_sine(SEED + 1, 0, 8, T, 1.0 / 16000).cpu().numpy(), whole)


def test_kernel_events_name_both_kernels():
    be = _backend()
    be.kernel_events(True)
    data = torch.from_numpy(_source(4, 64)).to(be.device)
    index = torch.tensor([3, 1], dtype=torch.int32, device=be.device)
    for _ in range(2):
        be.gather_batch(data, index)
    be.damped_sine(1, 0, 2, 64, 1e-3)
    times = be.kernel_times()
    assert list(times) == ["k_batch_gather", "k_damped_sine"]
    assert times["k_batch_gather"][1] == 2 and times["k_damped_sine"][1] == 1
    assert times["k_batch_gather"][0] > 0.0 and times["k_damped_sine"][0] > 0.0


def test_gather_batch_checks_its_tensors():
    be = _backend()
    data = torch.zeros((4, 8), dtype=torch.float32, device=be.device)
    index = torch.zeros(2, dtype=torch.int32, device=be.device)
    assert be.gather_batch(data, index[:0]).shape == (0, 8)
    for bad in (lambda: be.gather_batch(data.cpu(), index), lambda: be.gather_batch(data, index.long()),
                lambda: be.gather_batch(data.double(), index), lambda: be.gather_batch(data, index, index[:1]),
                lambda: be.gather_batch(data[:, ::2], index)):
        with pytest.raises(ValueError, match="gather_batch"):
            bad()


# ---------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------
def _trainer(kind, D, B):
    from audio_mps_amd import HParams, PsiCMPS, RhoCMPS
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=2)
    m = (RhoCMPS if kind == "rho" else PsiCMPS)(hp, seed=0, backend=HipScan(D))
    return Trainer(m, hp, device_step=True)


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_trainer_fed_from_the_device_equals_the_trainer_fed_from_the_host(kind):
    """D = 4, T = 64, B = 8, device-resident optimiser: three steps fed by ResidentDataset.batches (20 clips: batches of 8, 8 and 4) leave
    variables and Adam slots bit-identical to three steps fed the same batches as numpy arrays."""
    from audio_mps_amd.device_data import ResidentDataset
    D, T, B = 4, 64, 8
    clips = make_audio(20, T, 1.0 / 16000, 5)
    t_dev, t_host = _trainer(kind, D, B), _trainer(kind, D, B)
    feed = ResidentDataset(clips, t_dev.model._get_backend()).batches(B, seed=3, order="data")
    twin = ResidentDataset(clips, t_host.model._get_backend()).batches(B, seed=3, order="data")
    sizes = []
    for _ in range(3):
        batch = feed()
        assert batch.is_cuda
        host = twin().cpu().numpy()
        assert isinstance(host, np.ndarray) and host.shape == tuple(batch.shape)
        sizes.append(host.shape[0])
        t_dev.step(batch, sync=False, global_batch=host.shape[0])
        t_host.step(host, sync=False, global_batch=host.shape[0])
    assert sorted(sizes) == [4, 8, 8]
    t_dev.sync_to_host()
    t_host.sync_to_host()
    assert t_dev.opt.t == t_host.opt.t == 3
    assert "Wx" in t_host.model.variables if kind == "rho" else "psi_x" in t_host.model.variables
    for k in list(t_host.model.variables):
        for a, b, what in ((t_dev.model.variables, t_host.model.variables, "variable"), (t_dev.opt.m, t_host.opt.m, "adam m"),
                           (t_dev.opt.v, t_host.opt.v, "adam v")):
            assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), (what, k)
            assert np.all(np.isfinite(a[k]))
    assert any(np.any(t_dev.opt.m[k] != 0) for k in t_dev.opt.m)


def _ckpt(logdir, dataset, hp):
    return os.path.join(logdir, dataset, f"{hp.bond_dim}_{hp.delta_t}_{hp.minibatch_size}", "model.ckpt.npz")


def test_train_main_writes_the_same_checkpoint_with_and_without_device_data(tmp_path):
    """train.main on a 10-clip TFRecord file, sample_duration 64, minibatch_size 4, 7 steps (two epoch boundaries, two short batches):
    the same model.ckpt.npz variables (and Adam slots) bit for bit."""
    from audio_mps_amd import tfrecord as tfr
    from audio_mps_amd import train
    tfr.write_audio_tfrecord(os.path.join(tmp_path, "organ.tfrecords"), make_audio(10, 64, 1.0 / 16000, 3))
    argv = ["--dataset", "organ", "--datadir", str(tmp_path), "--sample_duration", "64", "--max_steps", "7",
            "--hparams", "bond_dim=4,minibatch_size=4", "--seed", "1"]
    t_host = train.main(argv + ["--logdir", os.path.join(tmp_path, "host")])
    t_dev = train.main(argv + ["--logdir", os.path.join(tmp_path, "dev"), "--device_data"])
    assert t_host.device_step and t_dev.device_step and t_dev.global_step == t_host.global_step == 7
    with np.load(_ckpt(os.path.join(tmp_path, "host"), "organ", t_host.hparams)) as a, \
            np.load(_ckpt(os.path.join(tmp_path, "dev"), "organ", t_dev.hparams)) as b:
        assert sorted(a.files) == sorted(b.files) and any(k.startswith("model/") for k in a.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
        assert all(np.all(np.isfinite(a[k])) for k in a.files)
    assert [h["global_batch"] for h in t_dev.history] == [h["global_batch"] for h in t_host.history]
    assert sorted(h["global_batch"] for h in t_host.history)[:2] == [2, 2]


def test_train_main_on_device_generated_damped_sines(tmp_path):
    """train.main --dataset damped_sine --device_data, T = 256, 3 steps: finite losses that differ from step to step (fresh clips every
    step), a checkpoint written."""
    from audio_mps_amd import train
    t = train.main(["--dataset", "damped_sine", "--device_data", "--sample_duration", "256", "--max_steps", "3",
                    "--hparams", "bond_dim=4,minibatch_size=4", "--logdir", str(tmp_path)])
    assert t.global_step == 3 and len(t.history) == 3
    losses = [h["model_loss"] for h in t.history]
    assert np.all(np.isfinite(losses)) and np.all(np.isfinite([h["total_loss"] for h in t.history])) and len(set(losses)) == 3
    assert os.path.exists(_ckpt(str(tmp_path), "damped_sine", t.hparams))
