"""The parameter-derived tables of a workspace (cmps_set_params*, cmps_bank_set_params_dev, cmps_legacy_set_params, cmps_rho_set_state,
cmps_rho_bank_set_state_dev): where they lie, what they must hold, and a numpy restatement that builds them.  numpy only; the exact sums
of `Q` are taken in Python integers (exact rational arithmetic), so nothing else is needed.

Where they lie -- the table sections of make_layout (audio_mps_amd/csrc/cmps_internal.h), restated by `layout`:

    R | RT | Q | QT | psi0 | freqs | qflag | ttab | dtk | rho | rfix      each section 256-byte aligned, DP = D rounded up to 32, N = T - 1

The end of `rfix` is cmps_workspace_bytes(D, B, T, CMPS_WS_FWD_ONLY) for every B; the callers assert that, and that R, psi0 and freqs read
back at these offsets echo what was uploaded, so that a drifted copy of the layout fails loudly.  Member m of a PsiCMPS bank lies at
m * cmps_workspace_bytes(D, B, T, flags), member m of a RhoCMPS bank at m * (the FWD_ONLY bytes + cmps_rho_workspace_bytes(...)), its
`phi0` behind its FWD_ONLY bytes; a rho workspace starts with `phi0` (make_rho_layout).

What they must hold -- written from the comments of cmps_prep.hip and the layout block, not from the kernel bodies; every check_* below
asserts one item and returns report rows (label, worst observed, bound).  The bounds are derived, none is fitted:

    time grid     ttab[0] = 0, ttab[k+1] = fl32(ttab[k] + fl32(dt)) in bits; dtk[k] = ttab[k] - ttab[k+1] exactly (the float64 difference
                  of the two float32 values is a float32 and equals the entry); dtk[N .. N+63] = 0
    packed        R, RT = R^T, psi0, freqs exact copies, every padding entry +0
    Q             c_half = fl32(-(double)dt sigma sigma) / 2; Q[i][j] within half a float32 ulp (at the exact value) x (1 + 2^-20)
                  + D 2^-52 |c_half| sum_k |terms| of c_half (R^dagger R)[i][j]: one rounding to float32 of a sum accumulated in double
    rho, entries  every entry that is not the last of its 64-step chunk: (fl32(cos d), fl32(sin d)), d = (double)fl32(f t_k) -
                  (double)fl32(f t_{k+1}), each component within half a float32 ulp x (1 + 2^-20) of the float64 value; lanes >= D and
                  row N hold (1, 0) in bits
    rho, product  C_k = the complex128 running product of the float32 entries, target_k = exp(-i fl32(f t_{k+1})), u = sqrt(2) 2^-25:
                  |C_k - target_k| <= 2 u at the last step of every chunk (one float32 rounding of the corrected entry, whose components
                  may lie in [1, 2)), independent of the chunk index, and <= (2 + k % 64) u everywhere
    qflag         D > 32: the word is |Q|_F <= 2^-19, |Q|_F in float64 from the table's own Q (inputs keep it 1e-3 away from the threshold)
    legacy        R (real), RT, Q, QT exact copies / transposes, zero padded; rho = (1, 0) over (N + 1) DP; dtk = 0 over N + 64; psi0 = e_0
    phi0          row a, lane d an exact copy, +0 for d >= D

Hermiticity of Q.  |Q[i][j] - conj(Q[j][i])| is at most 1 float32 ulp of the exact value, per component, and where the exact value is
zero (the imaginary part of the diagonal) the two agree exactly: a product of two float32 values is exact in double, so the bracket
conj(R[k][i]) R[k][i] cancels without a residue, fused or not, and the table holds +-0 there.  The largest difference is reported.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

F32 = np.float32
U = math.sqrt(2.0) * 2.0 ** -25          # one float32 rounding of a complex number of modulus < 2
SLACK = 1.0 + 2.0 ** -20                 # on every half-ulp bar: the float64 reference's own error, far below it
QFLAG_THRESHOLD = 2.0 ** -19
QFLAG_MARGIN = 1e-3
NAN_WORD = 0x7FC5A5A5                    # what a workspace of tests/_guard.py holds where nothing was written

# the frequencies of every case, tiled to D (rad/s): zero, tiny, moderate, a note of the scale, the Nyquist edge and beyond
FREQS = np.array([0.0, 1e-3, -1e-3, 3e-2, 0.37, 1.0, 50.0, -2 * math.pi * 261.6, 2 * math.pi * 7999, 1e5], dtype=F32)

SECTIONS = ("R", "RT", "Q", "QT", "psi0", "freqs", "qflag", "ttab", "dtk", "rho", "rfix")
PSI_TABLES = ("R", "RT", "Q", "psi0", "freqs", "ttab", "dtk", "rho")          # what cmps_set_params* defines (+ qflag at D > 32)
LEGACY_TABLES = ("R", "RT", "Q", "QT", "psi0", "dtk", "rho")


def padded(D: int) -> int:
    return (D + 31) // 32 * 32


def align256(x: int) -> int:
    return (x + 255) & ~255


def layout(D: int, T: int) -> dict:
    """{section: (byte offset, bytes)} of the table sections, and "end": the first byte behind rfix."""
    DP, N = padded(D), T - 1
    sizes = {"R": DP * DP * 8, "RT": DP * DP * 8, "Q": DP * DP * 8, "QT": DP * DP * 8, "psi0": DP * 8, "freqs": DP * 4, "qflag": 4,
             "ttab": (N + 1) * 4, "dtk": (N + 64) * 4, "rho": (N + 1) * DP * 8, "rfix": (N + 63) // 64 * DP * 2 * 16}
    out, o = {}, 0
    for name in SECTIONS:
        out[name] = (o, sizes[name])
        o = align256(o + sizes[name])
    out["end"] = o
    return out


class Tables:
    """Typed views of the table sections of ONE model's workspace inside `raw` (uint8), which starts `base` bytes into it."""

    def __init__(self, raw: np.ndarray, D: int, T: int, base: int = 0):
        assert raw.dtype == np.uint8 and raw.ndim == 1
        self.D, self.T, self.N, self.DP = D, T, T - 1, padded(D)
        self.L = layout(D, T)
        assert base % 256 == 0 and base + self.L["end"] <= raw.size, (base, self.L["end"], raw.size)
        DP, N = self.DP, self.N

        def sec(name, dtype, shape):
            off, n = self.L[name]
            return raw[base + off:base + off + n].view(dtype).reshape(shape)

        for name in ("R", "RT", "Q", "QT"):
            setattr(self, name, sec(name, np.complex64, (DP, DP)))
        self.psi0 = sec("psi0", np.complex64, (DP,))
        self.freqs = sec("freqs", F32, (DP,))
        self.qflag = sec("qflag", np.uint32, (1,))
        self.ttab = sec("ttab", F32, (N + 1,))
        self.dtk = sec("dtk", F32, (N + 64,))
        self.rho = sec("rho", np.complex64, (N + 1, DP))

    def bits(self, names=None) -> dict:
        """{section: its 32-bit words}: what bit-identity of two workspaces is asserted on."""
        names = names if names is not None else PSI_TABLES + (("qflag",) if self.D > 32 else ())
        return {k: words(getattr(self, k)) for k in names}


def words(a: np.ndarray) -> np.ndarray:
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def same_bits(a: dict, b: dict, what=""):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        bad = np.flatnonzero(a[k] != b[k])
        assert bad.size == 0, f"{what}: table '{k}' differs in {bad.size} of {a[k].size} words, the first at {int(bad[0])}"


def _exact(got: np.ndarray, want: np.ndarray, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    got, want = words(got), words(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, the first at {int(bad[0])}: {got[bad[0]]:#010x} != {want[bad[0]]:#010x}"
    return (what, 0, 0)


def ulp32(x) -> np.ndarray:
    """The spacing of float32 at the float64 value(s) x: 2^(floor(log2 |x|) - 23), never below the subnormal spacing 2^-149."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))                  # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 1 - 23, -149))


def c_half_of(sigma: float, dt: float) -> np.float32:
    """(float)(-delta_t * sigma * sigma) / 2.0f as cmps_capi.hip forms it: a double product, one rounding, an exact halving."""
    return F32(F32(-float(dt) * float(sigma) * float(sigma)) / F32(2.0))


# ---------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------
def time_grid(dt: float, N: int):
    """(ttab [N + 1], dtk [N + 64]) of the contract: the strictly sequential float32 sum."""
    dt32 = F32(dt)
    ttab = np.zeros(N + 1, dtype=F32)
    t = F32(0.0)
    for k in range(N):
        t = F32(t + dt32)
        ttab[k + 1] = t
    dtk = np.zeros(N + 64, dtype=F32)
    dtk[:N] = (ttab[:-1].astype(np.float64) - ttab[1:].astype(np.float64)).astype(F32)
    return ttab, dtk


def check_time_grid(t: Tables, dt: float):
    N = t.N
    ttab, _ = time_grid(dt, N)
    rows = [_exact(t.ttab, ttab, "ttab = running float32 sum")]
    d = t.ttab[:-1].astype(np.float64) - t.ttab[1:].astype(np.float64)
    assert np.array_equal(d.astype(F32).astype(np.float64), d), "ttab[k] - ttab[k+1] is not a float32 somewhere"
    bad = np.flatnonzero(t.dtk[:N].astype(np.float64) != d)
    assert bad.size == 0, f"dtk[k] != ttab[k] - ttab[k+1] at {bad.size} steps, the first k = {int(bad[0])}"
    rows.append(("dtk = ttab[k] - ttab[k+1], exact", 0, 0))
    rows.append(_exact(t.dtk[N:], np.zeros(64, dtype=F32), "dtk padding [N, N + 64) = 0"))
    return rows


def _padded_square(M: np.ndarray, DP: int) -> np.ndarray:
    out = np.zeros((DP, DP), dtype=np.complex64)
    out[:M.shape[0], :M.shape[1]] = M
    return out


def _padded_vec(v: np.ndarray, DP: int, dtype) -> np.ndarray:
    out = np.zeros(DP, dtype=dtype)
    out[:v.shape[0]] = v
    return out


def check_echo(t: Tables, R: np.ndarray, psi0: np.ndarray, freqs: np.ndarray):
    """The layout's self-check: what was uploaded is read back, bit for bit, at the restated offsets."""
    D = t.D
    return [_exact(t.R[:D, :D], R.astype(np.complex64), "echo R"), _exact(t.psi0[:D], psi0.astype(np.complex64), "echo psi0"),
            _exact(t.freqs[:D], freqs.astype(F32), "echo freqs")]


def check_packed(t: Tables, R: np.ndarray, psi0: np.ndarray, freqs: np.ndarray):
    DP = t.DP
    R = R.astype(np.complex64)
    return [_exact(t.R, _padded_square(R, DP), "R copy, zero padded"), _exact(t.RT, _padded_square(R.T, DP), "RT = R^T, zero padded"),
            _exact(t.psi0, _padded_vec(psi0.astype(np.complex64), DP, np.complex64), "psi0 copy, zero padded"),
            _exact(t.freqs, _padded_vec(freqs.astype(F32), DP, F32), "freqs copy, zero padded")]


def _to_int(x: np.ndarray, shift: int) -> np.ndarray:
    """The float32 array x as an object array of Python integers x 2^shift (exact: the caller's shift makes every entry an integer)."""
    scaled = np.ldexp(x.astype(np.float64), shift)
    assert np.array_equal(scaled, np.rint(scaled))
    return np.array([int(v) for v in scaled.reshape(-1)], dtype=object).reshape(x.shape)


@lru_cache(maxsize=16)
def _gram_exact(key):
    """(Re, Im, shift): (R^dagger R) 2^(2 shift) as exact Python integers, for the float32 matrix whose bytes are `key`."""
    D, re_bytes, im_bytes = key
    re = np.frombuffer(re_bytes, dtype=F32).reshape(D, D)
    im = np.frombuffer(im_bytes, dtype=F32).reshape(D, D)
    nz = np.concatenate([re[re != 0], im[im != 0]])
    shift = 0
    if nz.size:
        _, e = np.frexp(np.abs(nz).astype(np.float64))
        shift = int(24 - e.min())                                              # the smallest entry is m 2^e with a 24-bit m: an integer after 2^(24 - e)
    a, b = _to_int(re, shift), _to_int(im, shift)
    # (R^dagger R)[i][j] = sum_k conj(R[k][i]) R[k][j] = (a^T a + b^T b) + i (a^T b - b^T a)
    return a.T.dot(a) + b.T.dot(b), a.T.dot(b) - b.T.dot(a), shift


def q_reference(R: np.ndarray, c_half: np.float32):
    """(ref, absterm): c_half R^dagger R exactly, rounded once to float64 (complex128 [D][D]), and sum_k |terms| per component
    (real, imaginary) as a pair of float64 [D][D] for the double-accumulation term of the bar."""
    R = R.astype(np.complex64)
    D = R.shape[0]
    re, im = np.ascontiguousarray(R.real), np.ascontiguousarray(R.imag)
    gr, gi, shift = _gram_exact((D, re.tobytes(), im.tobytes()))
    c = float(c_half)
    cm, ce = math.frexp(c)
    ci = int(math.ldexp(cm, 53))                                               # c_half = ci 2^(ce - 53) exactly
    den_shift = 2 * shift + 53 - ce

    def ratio(n: int) -> float:                                                # n ci 2^-den_shift, correctly rounded (int / int is)
        n = n * ci
        return n / (1 << den_shift) if den_shift >= 0 else float(n << -den_shift)

    ref = np.array([[complex(ratio(gr[i, j]), ratio(gi[i, j])) for j in range(D)] for i in range(D)], dtype=np.complex128).reshape(D, D)
    ar, ai = np.abs(re).astype(np.float64), np.abs(im).astype(np.float64)
    return ref, (ar.T @ ar + ai.T @ ai, ar.T @ ai + ai.T @ ar)


def check_q(t: Tables, R: np.ndarray, sigma: float, dt: float):
    D, DP = t.D, t.DP
    c_half = c_half_of(sigma, dt)
    ref, (abs_re, abs_im) = q_reference(R, c_half)
    acc_re, acc_im = (D * 2.0 ** -52 * abs(float(c_half)) * a for a in (abs_re, abs_im))
    got = t.Q[:D, :D].astype(np.complex128)
    rows = []
    worst = 0.0
    for name, g, r, acc in (("re", got.real, ref.real, acc_re), ("im", got.imag, ref.imag, acc_im)):
        bar = 0.5 * ulp32(r) * SLACK + acc
        err = np.abs(g - r)
        i = int(np.argmax(err / bar))
        worst = max(worst, float((err / bar).reshape(-1)[i]))
        assert np.all(err <= bar), f"Q.{name}[{i // D}][{i % D}] = {g.reshape(-1)[i]!r}, exact {r.reshape(-1)[i]!r}: off by {err.reshape(-1)[i]:.3e}, bar {bar.reshape(-1)[i]:.3e}"
    rows.append(("Q = fl32(c_half R^dagger R): error / (half ulp (1 + 2^-20) + D 2^-52 |c_half| sum|terms|)", worst, 1.0))
    pad = t.Q.copy()
    pad[:D, :D] = 0
    rows.append(_exact(pad, np.zeros((DP, DP), dtype=np.complex64), "Q padding = 0"))
    # Hermiticity: at most 1 float32 ulp of the exact value per component; exactly equal where the exact value is zero
    herm = 0.0
    mirror = np.conj(got.T)
    for name, g, m, r in (("re", got.real, mirror.real, ref.real), ("im", got.imag, mirror.imag, ref.imag)):
        diff = np.abs(g - m)
        assert np.all(diff[r == 0] == 0), f"Q.{name}: Q[i][j] and conj(Q[j][i]) differ by {diff[r == 0].max():.3e} where the exact value is zero"
        herm = max(herm, float((diff / ulp32(r)).max()))
    assert herm <= 1.0, f"Q[i][j] and conj(Q[j][i]) differ by {herm} float32 ulps"
    rows.append(("Q Hermiticity: |Q[i][j] - conj(Q[j][i])| in float32 ulps of the exact value (exactly 0 where that is zero)", herm, 1.0))
    return rows


def angles(t: Tables):
    """fl32(f_d t_k) [N + 1][D], from the table's own freqs and ttab (asserted in bits elsewhere)."""
    return (t.ttab[:, None] * t.freqs[None, :t.D]).astype(F32)


def chunk_last(N: int) -> np.ndarray:
    """bool [N]: step k is the last of its 64-step chunk."""
    k = np.arange(N)
    return (k % 64 == 63) | (k == N - 1)


def check_rho_entries(t: Tables):
    D, DP, N = t.D, t.DP, t.N
    th = angles(t).astype(np.float64)
    delta = th[:-1] - th[1:]                                                   # exact: a float64 difference of two float32
    keep = ~chunk_last(N)
    worst = 0.0
    for name, g, r in (("cos", t.rho[:N, :D].real.astype(np.float64), np.cos(delta)), ("sin", t.rho[:N, :D].imag.astype(np.float64), np.sin(delta))):
        ratio = (np.abs(g - r) / (0.5 * ulp32(r)))[keep]
        if ratio.size:
            worst = max(worst, float(ratio.max()))
            i = int(np.argmax(ratio))
            assert ratio.max() <= SLACK, (f"rho.{name}: step {int(np.flatnonzero(keep)[i // D])}, lane {i % D}: {ratio.max():.4f} half-ulps "
                                          f"from fl32({name}(fl32(f t_k) - fl32(f t_k+1)))")
    rows = [("rho entries (not last of chunk): error in half float32 ulps", worst, SLACK)]
    one = np.zeros((N + 1, DP), dtype=np.complex64) + np.complex64(1.0)
    rows.append(_exact(t.rho[:, D:], one[:, D:], "rho lanes >= D = (1, 0)"))
    rows.append(_exact(t.rho[N], one[N], "rho row N = (1, 0)"))
    return rows


def rho_errors(t: Tables) -> np.ndarray:
    """|C_k - target_k| / u [N][D]."""
    D, N = t.D, t.N
    C = np.cumprod(t.rho[:N, :D].astype(np.complex128), axis=0)
    target = np.exp(-1j * angles(t)[1:].astype(np.float64))
    return np.abs(C - target) / U


def check_rho_accumulated(t: Tables):
    N = t.N
    err = rho_errors(t)
    last = chunk_last(N)
    k = np.arange(N)
    at_boundary = err[last].max(axis=1)
    b = int(np.argmax(at_boundary))
    assert at_boundary[b] <= 2.0, f"|C_k - target_k| = {at_boundary[b]:.2f} u at the chunk boundary k = {int(np.flatnonzero(last)[b])} (bar 2 u)"
    inside = (err / (2.0 + k % 64)[:, None]).max(axis=1)
    w = int(np.argmax(inside))
    assert inside[w] <= 1.0, f"|C_k - target_k| = {err[w].max():.2f} u at k = {w} (bar {2 + w % 64} u)"
    rows = [("rho product at chunk boundaries: |C_k - target_k| / u", float(at_boundary[b]), 2.0),
            ("rho product everywhere: |C_k - target_k| / ((2 + k % 64) u)", float(inside[w]), 1.0)]
    if at_boundary.size >= 8:                                                  # does the boundary error grow with the chunk index?
        q = at_boundary.size // 4
        rows.append((f"rho product at the boundaries of the first {q} chunks: |C_k - target_k| / u", float(at_boundary[:q].max()), 2.0))
        rows.append((f"rho product at the boundaries of the last {q} chunks: |C_k - target_k| / u", float(at_boundary[-q:].max()), 2.0))
    return rows


def q_norm(t: Tables) -> float:
    q = t.Q.astype(np.complex128)
    return math.sqrt(float(np.sum(q.real ** 2 + q.imag ** 2)))


def check_qflag(t: Tables):
    if t.D <= 32:
        return []
    nrm = q_norm(t)
    assert abs(nrm / QFLAG_THRESHOLD - 1.0) >= QFLAG_MARGIN, f"test input: |Q|_F = {nrm!r} is too close to 2^-19"
    want = 1 if nrm <= QFLAG_THRESHOLD else 0
    assert int(t.qflag[0]) == want, f"qflag = {int(t.qflag[0])} at |Q|_F = {nrm:.4e} (2^-19 = {QFLAG_THRESHOLD:.4e})"
    # (a threshold ratio, not an error against a bound: the row carries no bound)
    return [(f"qflag = {want} as |Q|_F <= 2^-19 says; the ratio |Q|_F / 2^-19 (a threshold ratio, kept 1e-3 away from 1)", nrm / QFLAG_THRESHOLD, None)]


def check_psi(t: Tables, R, psi0, freqs, sigma, dt):
    """Every item of the PsiCMPS contract on one model's tables; the report rows."""
    rows = check_echo(t, R, psi0, freqs) + check_time_grid(t, dt) + check_packed(t, R, psi0, freqs) + check_q(t, R, sigma, dt)
    return rows + check_rho_entries(t) + check_rho_accumulated(t) + check_qflag(t)


def check_legacy(t: Tables, R: np.ndarray, Q: np.ndarray):
    D, DP, N = t.D, t.DP, t.N
    Rc, Q = R.astype(F32).astype(np.complex64), Q.astype(np.complex64)
    e0 = np.zeros(DP, dtype=np.complex64)
    e0[0] = 1.0
    return [_exact(t.R, _padded_square(Rc, DP), "legacy R (real) copy, zero padded"), _exact(t.RT, _padded_square(Rc.T, DP), "legacy RT = R^T"),
            _exact(t.Q, _padded_square(Q, DP), "legacy Q copy, zero padded"), _exact(t.QT, _padded_square(Q.T, DP), "legacy QT = Q^T"),
            _exact(t.rho, np.zeros((N + 1, DP), dtype=np.complex64) + np.complex64(1.0), "legacy rho = (1, 0)"),
            _exact(t.dtk, np.zeros(N + 64, dtype=F32), "legacy dtk = 0"), _exact(t.psi0, e0, "legacy psi0 = e_0")]


def phi0_view(raw: np.ndarray, D: int, rank: int, base: int = 0) -> np.ndarray:
    """The phi0 section [rank][DP] complex64 of a rho workspace (its first section, make_rho_layout) that starts at byte `base`."""
    DP = padded(D)
    assert base % 256 == 0 and base + rank * DP * 8 <= raw.size
    return raw[base:base + rank * DP * 8].view(np.complex64).reshape(rank, DP)


def check_phi0(got: np.ndarray, phi: np.ndarray):
    rank, DP = got.shape
    want = np.zeros((rank, DP), dtype=np.complex64)
    want[:, :phi.shape[1]] = phi.astype(np.complex64)
    return [_exact(got, want, "phi0 copy, zero padded")]


# ---------------------------------------------------------------------------------------------------
# inputs of a case
# ---------------------------------------------------------------------------------------------------
def case_inputs(D: int, seed: int = 0, r_scale: float = 0.3, roll: int = 0):
    """(R complex64 [D][D], psi0 complex64 [D], freqs float32 [D]): FREQS tiled to D (started `roll` entries in, so that a small D need
    not sit on the zero frequency), normal R x r_scale, a normalised normal psi0."""
    rng = np.random.default_rng(1000 * D + seed)
    R = (r_scale * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64)
    psi0 = rng.standard_normal(D) + 1j * rng.standard_normal(D)
    psi0 = (psi0 / np.linalg.norm(psi0)).astype(np.complex64)
    freqs = np.resize(np.roll(FREQS, -roll), D).astype(F32)
    return R, psi0, freqs


def pack_params(R, psi0, freqs, A=1.0) -> np.ndarray:
    """R_re | R_im | freqs | psi0_re | psi0_im | A, float32 [2 D^2 + 3 D + 1]: the buffer of cmps_set_params_dev and one row of a bank's."""
    R, psi0 = R.astype(np.complex64), psi0.astype(np.complex64)
    return np.concatenate([R.real.reshape(-1), R.imag.reshape(-1), freqs.astype(F32), psi0.real, psi0.imag, [F32(A)]]).astype(F32)


# ---------------------------------------------------------------------------------------------------
# the restatement: the tables built in numpy, and the wrong tables the checks must reject
# ---------------------------------------------------------------------------------------------------
MUTANTS = ("no_drift_correction", "partial_chunk_uncorrected", "t_is_k_dt", "delta_from_dt", "dtk_padding", "rt_not_transposed",
           "padding_lane", "q_float32")


def blank(nbytes: int) -> np.ndarray:
    """A workspace nobody wrote: the quiet-NaN pattern of tests/_guard.py in every word."""
    assert nbytes % 4 == 0
    return np.full(nbytes // 4, NAN_WORD, dtype=np.uint32).view(np.uint8)


def build_psi(raw: np.ndarray, D: int, T: int, R, psi0, freqs, sigma: float, dt: float, base: int = 0, mutant: str | None = None):
    """Write the PsiCMPS tables of the contract into `raw` at byte `base`; `mutant` names one deliberate error (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    t = Tables(raw, D, T, base)
    DP, N = t.DP, t.N
    R = R.astype(np.complex64)
    dt32 = F32(dt)
    ttab, dtk = time_grid(dt, N)
    if mutant == "t_is_k_dt":
        ttab = (np.arange(N + 1, dtype=np.float64).astype(F32) * dt32).astype(F32)
        dtk[:N] = (ttab[:-1].astype(np.float64) - ttab[1:].astype(np.float64)).astype(F32)
    if mutant == "dtk_padding":
        dtk[N + 5] = dt32
    t.ttab[:], t.dtk[:] = ttab, dtk
    t.R[:] = _padded_square(R, DP)
    t.RT[:] = _padded_square(R if mutant == "rt_not_transposed" else R.T, DP)
    t.psi0[:] = _padded_vec(psi0.astype(np.complex64), DP, np.complex64)
    t.freqs[:] = _padded_vec(freqs.astype(F32), DP, F32)
    # Q: accumulated in double, scaled in double, rounded once
    c_half = c_half_of(sigma, dt)
    if mutant == "q_float32":
        acc = np.zeros((D, D), dtype=np.complex64)
        for k in range(D):
            acc = (acc + np.conj(R[k])[:, None] * R[k][None, :]).astype(np.complex64)
        q = (np.complex64(c_half) * acc).astype(np.complex64)
    else:
        Rd = R.astype(np.complex128)
        q = (float(c_half) * (Rd.conj().T @ Rd)).astype(np.complex64)
    t.Q[:] = _padded_square(q, DP)
    t.qflag[0] = 1 if q_norm(t) <= QFLAG_THRESHOLD else 0
    # rho: raw entries, then the last entry of every chunk replaced by fl32(target / actual)
    f = t.freqs[:D]
    th = (ttab[:, None] * f[None, :]).astype(F32).astype(np.float64)
    delta = th[:-1] - th[1:]
    if mutant == "delta_from_dt":
        delta = (f[None, :] * (ttab[:-1] - ttab[1:]).astype(F32)[:, None]).astype(F32).astype(np.float64)
    rho = np.ones((N + 1, DP), dtype=np.complex64)
    rho[:N, :D] = (np.cos(delta) + 1j * np.sin(delta)).astype(np.complex64)
    if mutant != "no_drift_correction":
        acc = np.ones(D, dtype=np.complex128)                                  # the exact product of the float32 table so far
        for k0 in range(0, N, 64):
            k1 = min(k0 + 64, N)
            before = acc * np.prod(rho[k0:k1 - 1, :D].astype(np.complex128), axis=0)
            if mutant == "partial_chunk_uncorrected" and k1 - k0 < 64:
                break
            last = (np.exp(-1j * th[k1]) / before).astype(np.complex64)
            rho[k1 - 1, :D] = last
            acc = before * last.astype(np.complex128)
    if mutant == "padding_lane":
        if D < DP:
            rho[N // 2, DP - 1] = np.complex64(1.0 + 1e-7)
        else:
            rho[N, 0] = np.complex64(1.0 + 1e-7)
    t.rho[:] = rho
    return t


def build_legacy(raw: np.ndarray, D: int, T: int, R: np.ndarray, Q: np.ndarray, base: int = 0):
    t = Tables(raw, D, T, base)
    DP = t.DP
    Rc, Q = R.astype(F32).astype(np.complex64), Q.astype(np.complex64)
    t.R[:], t.RT[:], t.Q[:], t.QT[:] = (_padded_square(M, DP) for M in (Rc, Rc.T, Q, Q.T))
    t.rho[:] = 1.0
    t.dtk[:] = 0.0
    t.psi0[:] = 0.0
    t.psi0[0] = 1.0
    return t


def build_phi0(raw: np.ndarray, D: int, phi: np.ndarray, base: int = 0):
    got = phi0_view(raw, D, phi.shape[0], base)
    got[:] = 0.0
    got[:, :D] = phi.astype(np.complex64)
    return got


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_tables.py (tests/test_tables_host.py runs the restatement through the same)
# ---------------------------------------------------------------------------------------------------
DT = (1.0 / 16000, 1.0 / 3000, 1e-5)
# (D, N = T - 1, dt, sigma, r_scale, roll): D over {1, 16, 31, 32, 33, 64, 128} (DP = 32, 64, 128 and the qflag launch), N over
# {1, 33, 63, 64, 65, 97, 191, 256, 289, 543} (NC = 1, 2, 3, 4, 5, 9; last chunks of 1, 33, 63, 64 and 31 steps), every dt, both sigma;
# at D = 64 R is scaled so that both qflag values occur at sigma = 0.36
CASES = (
    (1, 1, DT[0], 0.36, 0.3, 8), (1, 191, DT[1], 0.36, 0.3, 7), (16, 33, DT[1], 1e-4, 0.3, 0), (16, 543, DT[2], 0.36, 0.3, 3),
    (31, 63, DT[2], 0.36, 0.3, 0), (31, 289, DT[0], 1e-4, 0.3, 5), (32, 64, DT[0], 0.36, 0.3, 0), (32, 97, DT[1], 0.36, 0.3, 2),
    (33, 65, DT[1], 0.36, 0.3, 0), (33, 256, DT[2], 1e-4, 0.3, 4), (64, 97, DT[0], 0.36, 0.3, 0), (64, 256, DT[0], 0.36, 0.01, 1),
    (64, 191, DT[2], 1e-4, 0.3, 6), (128, 289, DT[1], 0.36, 0.2, 0), (128, 543, DT[0], 1e-4, 0.2, 9), (128, 1, DT[2], 0.36, 0.2, 0),
)
# the long grids (D <= 32 only): the boundary error must not grow with the chunk index
LONG_CASES = ((32, 16000, DT[0], 0.36, 0.3, 0), (31, 65535, DT[0], 1e-4, 0.3, 0))


def case_id(case) -> str:
    D, N, dt, sigma, r_scale, roll = case
    return f"D{D}-N{N}-dt{dt:.3g}-s{sigma:g}-r{r_scale:g}"


def report(title: str, rows) -> list:
    """The printed worst-versus-bound lines of one case (a row without a bound is a plain value)."""
    lines = [f"TABLES {title}: {label}: " + (f"value {worst:.6g}" if bound is None else f"worst {worst:.6g}, bound {bound:.6g}")
             for label, worst, bound in rows]
    print("\n".join(lines))
    return lines
