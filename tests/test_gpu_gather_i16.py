"""k_batch_gather_i16 on a real MI355X, bit for bit against tests/_eval_ref.gather_i16 (= tests/_data_ref.gather of the widened dataset) in
guarded buffers (tests/_guard.py): every destination cut and both source phases (a row's first sample at 0 or 2 mod 4 bytes), data_dev itself
at 0 or 2 mod 4, the row-stride loop, the row guard, and the first and last row of the buffer against poisoned neighbours.

The source the kernel sees is POISONED wherever no valid row reads: an int16 of its own (-21846 = 0xAAAA) that no clip holds, so a stray
sample that reached the output would show.  The bytes around the buffer hold the guard's pattern and are checked after every call."""
import ctypes

import numpy as np
import pytest
import torch

import _eval_ref as ER
import _guard as G

pytestmark = pytest.mark.gpu

POISON = np.int16(-21846)
SCALES = [2.0 ** -15, 1.0, 3.0]


def _source(N, L):
    """int16 clips without the poison value, the ends of the range included."""
    rng = np.random.default_rng(N * 1000003 + L)
    data = rng.integers(-32768, 32768, size=(N, L)).astype(np.int16)
    data[data == POISON] = 12345
    data.reshape(-1)[[0, -1]] = [-32768, 32767]
    data[N // 2, L // 2] = 32767
    data[N // 2, (L // 2 + 1) % L] = -32768
    return data


def _run(data, index, offset, T, scale, audio_shift=0, data_shift=0, poison=True):
    """cmps_batch_gather_i16 in guarded buffers -> the uint32 bits of audio [B, T].  ``data_shift`` (bytes, 0 or 2) puts data_dev that far
    behind a 256-byte boundary, the buffer ending against the guard zone with no slack; ``audio_shift`` (floats) likewise for audio_dev."""
    from audio_mps_amd import _capi
    lib = _capi.load()
    dev = torch.device(f"cuda:{torch.cuda.current_device()}")
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
    h = ctypes.c_void_p()
    assert lib.cmps_create(8, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        # the data buffer: `data_shift` bytes of the guard's pattern, then the clips, then the back zone at once
        d = G.Guarded(data_shift + seen.nbytes, dev, align=256, fill=G.NAN_FILL, name="data")
        front = d.numpy(np.uint8)[:data_shift]
        image = np.concatenate([front, seen.reshape(-1).view(np.uint8)])
        d.load(image)
        d.snapshot(image)
        inputs = [d]
        for name, a in (("index", index), ("offset", offs)):
            if a is not None:
                g = G.Guarded(a.nbytes, dev, align=256, fill=G.NAN_FILL, name=name)
                g.load(a)
                g.snapshot(a)
                inputs.append(g)
        out = G.Guarded(4 * (B * T + audio_shift), dev, align=256, fill=G.NAN_FILL, name="audio")
        code = lib.cmps_batch_gather_i16(h, d.ptr + data_shift, N, L, inputs[1].ptr, inputs[2].ptr if offs is not None else None, B, T,
                                         scale, out.ptr + 4 * audio_shift, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert code == _capi.CMPS_OK, lib.cmps_last_error(h)
        torch.cuda.synchronize(dev)
        for g in inputs + [out]:
            assert g.zones_intact() is None, (g.name, g.zones_intact())
        for g in inputs:
            assert g.equals_snapshot() is None, g.name
        assert out.untouched_mask(torch.float32).cpu().numpy()[:audio_shift].all(), "the floats in front of audio_dev were written"
        return out.numpy(np.uint32)[audio_shift:].reshape(B, T)
    finally:
        lib.cmps_destroy(h)


def _want(data, index, offset, T, scale):
    return ER.gather_i16(data, index, offset, T, scale).view(np.uint32)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1021, 8197])
def test_every_cut_and_both_source_phases(T):
    """Per T: clip_len odd and even, offsets odd and even (sources at 0 and 2 mod 4 bytes), audio_dev shifted by 0 .. 3 floats, data_dev at 0
    and 2 mod 4, the three scales.  The first and the last clip of the buffer are always among the rows, at offset 0 and at L - T."""
    k = 0
    for L in (T + 4, T + 5):
        N = 3
        data = _source(N, L)
        index = [0, 2, 1, 2, 0]
        offset = [0, L - T, 1, 2, 3]                             # clip 0 from its first sample, clip N - 1 up to the buffer's last
        for audio_shift in (0, 1, 2, 3):
            scale, data_shift = SCALES[k % 3], 2 * (k % 2)
            k += 1
            got = _run(data, index, offset, T, scale, audio_shift, data_shift)
            want = _want(data, index, offset, T, scale)
            assert got.shape == want.shape and np.array_equal(got, want), (L, audio_shift, scale, data_shift, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("scale", SCALES)
def test_whole_buffer_and_the_row_stride(scale):
    """T = L: the gather reads every sample of the buffer, first and last included, at both placements of data_dev (odd clip_len: the rows
    alternate between the two phases); B = 2050 at T = 8 goes through the kernel's stride over the rows."""
    for N, L in ((4, 7), (3, 64), (2, 8197)):
        data = _source(N, L)
        index = np.arange(N)[::-1]
        for data_shift in (0, 2):
            got = _run(data, index, None, L, scale, data_shift=data_shift, poison=False)
            assert np.array_equal(got, _want(data, index, None, L, scale)), (N, L, data_shift)
    data = _source(5, 11)
    index, offset = np.arange(2050) % 5, np.arange(2050) % 4
    got = _run(data, index, offset, 8, scale, data_shift=2)
    assert np.array_equal(got, _want(data, index, offset, 8, scale))
    # the values are what the definition says: an exact conversion and one multiply
    assert np.array_equal(got.view(np.float32)[0], data[0, :8].astype(np.float32) * np.float32(scale))


@pytest.mark.parametrize("L,T", [(40, 33), (4201, 4100)])
def test_bad_rows_are_nan_and_read_nothing(L, T):
    """index -1, N and 2^31 - 1, offset -1 and L - T + 1: NaN rows exactly where the rule says (0x7fc00000 in every element), the other
    rows correct, the source poisoned outside the valid rows' windows."""
    N = 4
    data = _source(N, L)
    bad_index, bad_offset = [-1, 0, N, 2], [0, L - T + 1, 0, -1]
    for index, offset, nan_rows in ((bad_index, None, [0, 2]), (bad_index, [0, 1, 2, 3], [0, 2]), ([3, 1, 0, 2], bad_offset, [1, 3]),
                                    (bad_index, bad_offset, [0, 1, 2, 3]), ([2 ** 31 - 1, 0, 3, 1], [0, 0, L - T, 1], [0])):
        got = _run(data, index, offset, T, 2.0 ** -15, data_shift=2)
        assert np.array_equal(got, _want(data, index, offset, T, 2.0 ** -15))
        for b in range(4):
            assert bool(np.all(got[b] == 0x7FC00000)) == (b in nan_rows), (index, offset, b)


def test_through_hipscan_dispatch_and_kernel_events():
    from audio_mps_amd.scan import HipScan
    be = HipScan(8)
    data = _source(6, 101)
    index, offset = np.array([5, 0, 3], np.int32), np.array([1, 0, 30], np.int32)
    d16 = torch.from_numpy(data).to(be.device)
    d32 = torch.from_numpy(data.astype(np.float32) * np.float32(2.0 ** -15)).to(be.device)
    ix, of = torch.from_numpy(index).to(be.device), torch.from_numpy(offset).to(be.device)
    be.kernel_events(True)
    a = be.gather_batch(d16, ix, of, T=70)
    b = be.gather_batch(d32, ix, of, T=70)
    c = be.gather_batch(d16, ix, None, scale=3.0)
    times = be.kernel_times()
    be.kernel_events(False)
    assert {k: v[1] for k, v in times.items()} == {"k_batch_gather_i16": 2, "k_batch_gather": 1}
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(c.cpu().numpy().view(np.uint32), _want(data, index, None, 101, 3.0))
    with pytest.raises(ValueError, match="gather_batch"):
        be.gather_batch(d16.to(torch.int32), ix)
