"""An independent numpy restatement of the device-side training input of include/cmps.h: the synthetic clips of cmps_damped_sine_fill
(Philox4x32-10 from tests/_noise_ref.py, then the float part in the normative operation order, evaluated in a chosen dtype) and the row
gather of cmps_batch_gather with its NaN rows.  `damped_sine(..., np.float64)` is the definition the device is judged against,
`damped_sine(..., np.float32)` the float32 evaluation whose own distance from it sets the bar."""
import numpy as np

import _noise_ref as NR

QNAN = np.uint32(0x7FC00000)


def delays(seed, first_clip, B, T, dtype=np.float64):
    """The delay of clips first_clip .. first_clip + B - 1, [B] of `dtype`: dt(T / 200) * (-(log u0 + log u1)), a Gamma(2, T / 200) draw."""
    seed, first_clip, B, T = int(seed), int(first_clip), int(B), int(T)
    assert 0 <= seed < 2 ** 64 and first_clip >= 0 and B >= 1 and first_clip + B < 2 ** 64 and 1 <= T <= 2 ** 24
    c = np.array([first_clip + b for b in range(B)], dtype=np.uint64)
    x = NR.philox4x32_10((c & NR.MASK, c >> NR.S32, np.uint64(0), np.uint64(1)), (seed & 0xFFFFFFFF, seed >> 32))
    dt = np.dtype(dtype).type
    u0, u1 = (((x[i] >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dt(2.0 ** -24) for i in (0, 1))
    return dt(T / 200.0) * (-(np.log(u0) + np.log(u1)))


def damped_sine(seed, first_clip, B, T, delta_t, dtype=np.float64):
    """What cmps_damped_sine_fill defines, [B, T] of `dtype`: every constant rounded to `dtype`, every operation in it, in the header's order."""
    dt = np.dtype(dtype).type
    d = delays(seed, first_clip, B, T, dtype)
    t = (np.arange(T).astype(dtype)[None, :] - d[:, None]) * dt(delta_t)
    return ((dt(0.5) * (np.sign(t) + dt(1))) * np.sin(dt(2 * np.pi * 261.6) * t)) * np.exp(-t / dt(0.1))


def gather(data, index, offset, T):
    """What cmps_batch_gather defines, float32 [B, T]: row b = data[index[b], offset[b] : offset[b] + T], or T quiet NaNs (0x7fc00000) where
    index[b] lies outside [0, N) or offset[b] outside [0, L - T].  offset None: all zero."""
    data = np.asarray(data, dtype=np.float32)
    N, L = data.shape
    index = np.asarray(index, dtype=np.int64)
    offset = np.zeros_like(index) if offset is None else np.asarray(offset, dtype=np.int64)
    out = np.empty((index.size, T), dtype=np.float32)
    for b, (i, o) in enumerate(zip(index, offset)):
        if 0 <= i < N and 0 <= o <= L - T:
            out[b] = data[i, o:o + T]
        else:
            out[b].view(np.uint32)[:] = QNAN
    return out
