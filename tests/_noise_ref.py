"""An independent numpy restatement of the counter-based normals of include/cmps.h (cmps_noise_fill): Philox4x32-10 in uint64 arithmetic,
then the Box-Muller map evaluated in a chosen dtype with cos(pi v) / sin(pi v) as the trig functions.  `normals(..., np.float64)` is the
definition the device is judged against, `normals(..., np.float32)` the float32 evaluation whose own distance from it sets the bar."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words (broadcastable), key: two 32-bit ints -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # 32 x 32 -> 64 bits: no wrap in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normals(seed, path, first, length, dtype=np.float64):
    """z(seed, path, s) for s = first .. first + length - 1 as an array [length] of `dtype` (python ints of any size in)."""
    seed, path, first, length = int(seed), int(path), int(first), int(length)
    assert 0 <= seed < 2 ** 64 and 0 <= path < 2 ** 32 and first >= 0 and length >= 1 and first + length <= 2 ** 64
    q_lo, q_hi = first >> 2, (first + length - 1) >> 2
    q = np.array([q_lo + i for i in range(q_hi - q_lo + 1)], dtype=np.uint64) if q_hi >= 2 ** 63 else \
        np.arange(q_lo, q_hi + 1, dtype=np.uint64)
    x = philox4x32_10((q & MASK, q >> S32, np.uint64(path), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
    dt = np.dtype(dtype).type
    z = np.empty((q.size, 4), dtype=dtype)
    for j in (0, 1):
        u = ((x[2 * j] >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dt(2.0 ** -24)
        v = (x[2 * j + 1] >> np.uint64(8)).astype(dtype) * dt(2.0 ** -23)
        rad = np.sqrt(dt(-2) * np.log(u))
        z[:, 2 * j] = rad * np.cos(dt(np.pi) * v)
        z[:, 2 * j + 1] = rad * np.sin(dt(np.pi) * v)
    off = first - 4 * q_lo
    return np.ascontiguousarray(z.reshape(-1)[off:off + length])


def noise(seed, first_step, n, length, std, first_path=0, dtype=np.float64):
    """What cmps_noise_fill defines, [n, length]: std * z(seed, first_path + b, first_step + j), the product in `dtype`."""
    dt = np.dtype(dtype).type
    return np.stack([dt(std) * normals(seed, first_path + b, first_step, length, dtype) for b in range(n)])
