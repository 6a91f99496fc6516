"""cmps_bank_calibrate restated in numpy (include/cmps.h states the model, the objective and the rounding bounds): J, g, h and q at a
theta in float64 and in np.longdouble, a reference optimiser that shares no line with the device's solver (bisection on the monotone g
for kappa, the scaling sweep for c, alternated until both residuals are below 1e-13), and the draws the tests run on.

    l[m][b]  float32 losses, M members, N clips; y_b the labels; theta = (kappa, c_0 .. c_{M-1})
    ABSENT   a NaN or +-Inf loss;  SKIPPED  y_b outside [0, M) (n_unlabelled), else the own member absent (n_own_absent)
    a_m = kappa (l_m - lmin_b) - c_m, shifted by its minimum;  p_m = exp(-a_m) / sum exp(-a_m');  xent_b = a_y + log sum exp(-a_m)
    J = mean xent_b;  g = mean ((l_y - lmin_b) - E_b);  h = mean V_b;  q_m = sum_b p_m(b);  dJ / dc_m = (q_m - n_m) / n
"""
import numpy as np

FIT_TEMPERATURE, FIT_PRIOR = 1, 2
CONVERGED, AT_KAPPA_MIN, AT_KAPPA_MAX, NO_DATA, MAX_ITER = 1, 2, 4, 8, 16
NAN_FILL = np.array([0x7FC5A5A5], dtype=np.uint32).view(np.float32)[0]          # tests/_guard.py's fill
SHAPES = [(2, 4), (3, 37), (5, 300), (65, 70), (1024, 3)]                        # (5, 300): five tiles of 64 clips, the last one partial


class Evaluation:
    """J, g, h, q [M], n_m [M] and the counts at a theta, with D and A of the header's ROUNDING paragraph."""

    def bounds(self):
        """(eps_J, eps_g, eps_q) of include/cmps.h at this theta."""
        M, n, u2 = self.M, float(self.n), 2.0 ** -52
        eps_J = u2 * (M + 32 + 6 * self.A + (n / 2 + 2) * float(self.J))
        eps_g = u2 * self.D * (1.5 * M + 14 + 6 * self.A + n / 2)
        eps_q = u2 * n * (0.7 * M + 9 + 6 * self.A + n / 2)
        return eps_J, eps_g, eps_q

    def resid(self):
        fitted = self.n_m > 0
        return float(np.max(np.abs(self.q[fitted] - self.n_m[fitted]))) / float(self.n) if self.n and fitted.any() else 0.0


def evaluate(loss, labels, kappa, c, dtype=np.float64):
    """The definition at theta = (kappa, c), every operation in ``dtype`` on the float32 losses."""
    loss = np.asarray(loss, dtype=np.float32)
    labels = np.asarray(labels)
    M, N = loss.shape
    ev = Evaluation()
    ev.M = M
    present = np.isfinite(loss)
    labelled = (labels >= 0) & (labels < M)
    own = np.where(labelled, labels, 0)
    own_present = present[own, np.arange(N)]
    used = labelled & own_present
    ev.n_unlabelled, ev.n_own_absent, ev.n = int(np.sum(~labelled)), int(np.sum(labelled & ~own_present)), int(np.sum(used))
    ev.used = used
    ev.n_m = np.bincount(labels[used], minlength=M).astype(np.int64)
    ev.q = np.zeros(M, dtype=dtype)
    ev.J = ev.g = ev.h = dtype(0)
    ev.D = ev.A = 0.0
    if ev.n == 0:
        return ev
    l = loss[:, used].astype(dtype)
    pr = present[:, used]
    y = labels[used]
    cols = np.arange(ev.n)
    kappa, c = dtype(kappa), np.asarray(c, dtype=dtype)
    big = dtype(np.inf)
    lmin = np.min(np.where(pr, l, big), axis=0)
    d = np.where(pr, l - lmin[None, :], dtype(0))
    a = np.where(pr, kappa * d - c[:, None], big)
    amin = np.min(a, axis=0)
    e = np.exp(-(a - amin[None, :]))                      # (an absent member, or one with a prior of zero: a = +inf, e = 0)
    S = np.sum(e, axis=0)
    p = e / S[None, :]
    xent = (a[y, cols] - amin) + np.log(S)
    E = np.sum(p * d, axis=0)
    V = np.sum(p * d * d, axis=0) - E * E
    ev.J, ev.g, ev.h = np.mean(xent), np.mean(d[y, cols] - E), np.mean(V)
    ev.q = np.sum(p, axis=1)
    ev.D = float(np.max(d))
    ev.A = float(abs(kappa)) * ev.D + float(np.max(np.abs(c[np.isfinite(c)]))) if np.isfinite(c).any() else float(abs(kappa)) * ev.D
    return ev


def optimise(loss, labels, fit, kappa, c, kappa_min=1e-6, kappa_max=1e6, dtype=np.longdouble, resid_tol=1e-13, rounds=20000, strict=True,
             kappa_tol=None):
    """The reference optimiser: (kappa, c, rounds used).  kappa: bisection in log kappa on the monotone g inside the box, to the last bit;
    c: one scaling sweep of the members that have a clip; alternated until |kappa g| (or a bound with g pushing outwards) and the prior
    residual are both below ``resid_tol`` (``strict=False``: or ``rounds`` are used up).
    ``kappa_tol``: the search for kappa stops once |kappa g| is below it, instead of at the last bit, and goes by false position
    (Illinois) once the bracket is narrower than a factor 4: a timing run's host side, which should not be slower than it has to be."""
    kappa, c = dtype(kappa), np.array(c, dtype=dtype)

    def g_at(k):
        return evaluate(loss, labels, k, c, dtype).g

    def solve_kappa():
        lo, hi, side = dtype(kappa_min), dtype(kappa_max), 0
        if g_at(lo) >= 0:
            return lo
        if g_at(hi) <= 0:
            return hi
        g_lo, g_hi = g_at(lo), g_at(hi)
        for _ in range(400):
            mid = np.sqrt(lo * hi)
            if kappa_tol is not None and hi / lo < 4:      # false position with Illinois' halving, once the bracket is narrow: fewer looks
                mid = (lo * g_hi - hi * g_lo) / (g_hi - g_lo)
            if mid <= lo or mid >= hi:
                break
            g_mid = g_at(mid)
            if kappa_tol is not None and abs(mid * g_mid) <= kappa_tol:
                return mid
            if g_mid < 0:
                lo, g_lo, g_hi = mid, g_mid, (g_hi / 2 if side == -1 else g_hi)
                side = -1
            else:
                hi, g_hi, g_lo = mid, g_mid, (g_lo / 2 if side == 1 else g_lo)
                side = 1
        return lo if abs(g_at(lo)) <= abs(g_at(hi)) else hi

    for r in range(rounds):
        if fit & FIT_TEMPERATURE:
            kappa = solve_kappa()
        ev = evaluate(loss, labels, kappa, c, dtype)
        if ev.n == 0 or not fit & FIT_PRIOR or ev.resid() <= resid_tol:
            return kappa, c, r + 1
        fitted = ev.n_m > 0
        c[fitted] += np.log(ev.n_m[fitted].astype(dtype) / ev.q[fitted])
    if strict:
        raise AssertionError("the reference optimiser did not converge")
    return kappa, c, rounds


def draw(M, N, seed, scale=1.5, margin=None, specials=True):
    """One test problem: (loss [M][N + 3] float32 with rows padded by the guard's NaN fill, labels [N] int32, N).  l[m][b] = base_b + s z
    with base_b near 2000 (the totals of a clip of a few thousand samples: the shifts matter), the own member lowered by a margin that
    leaves the accuracy near 70 %; a few NaN, +Inf and -Inf entries, a few labels of -1 and of M, a few clips whose own member is absent.
    A fit needs more clips than it has parameters, and wrong ones among them, to have its optimum at a finite theta: the labels come from
    K = min(M, max(2, N / 8)) of the M classes (all of them where N >= 8 M), each of which keeps a used clip (the first K clips carry one
    label each and stay as they are); the other members are UNFITTED (`start` gives them a prior of zero where the prior is fitted).
    (1024, 3) is built by hand: two classes a, b; one clip of a that is right, one clip of a that prefers b by 3, one clip of b that
    prefers b by 1 -- no prior between a and b serves both of the last two, so temperature and prior have a joint optimum inside."""
    rng = np.random.default_rng(seed)
    ld = N + 3
    K = M if N >= 8 * M else min(M, max(2, N // 8))
    if margin is None:                                      # the smallest of k normals sits near -sqrt(2 log k): about 70 % right among
        margin = scale * (0.75 + 0.55 * np.log(np.sqrt(M * K)))          # sqrt(M K) members, between the K fitted ones and all M
    base = 2000.0 + 50.0 * rng.standard_normal(N)
    loss = base[None, :] + scale * rng.standard_normal((M, N))
    if N < 8 and M > N:
        assert N == 3
        a, b = (int(v) for v in rng.choice(M, size=2, replace=False))
        labels = np.array([a, a, b], dtype=np.int32)
        loss += margin + 4.0 * scale                        # every other member well above the two
        loss[[a, b], :] = base[None, :] + np.array([[0.0, 3.0, 1.0], [2.0, 0.0, 0.0]])
        loss = loss.astype(np.float32)
    else:
        classes = rng.permutation(M)[:K]
        labels = classes[np.concatenate([rng.permutation(K), rng.integers(0, K, size=N - K)])].astype(np.int32)
        loss[labels, np.arange(N)] -= margin
        loss = loss.astype(np.float32)
        if specials and N >= 30 and N - K >= 4:
            k = max(3, N // 12)
            for value in (np.nan, np.inf, -np.inf):
                mm, bb = rng.integers(0, M, size=k), rng.integers(0, N, size=k)
                keep = labels[bb] != mm                     # (own members go absent below, among the spare clips only)
                loss[mm[keep], bb[keep]] = value
            spare = K + rng.choice(N - K, size=4, replace=False)
            loss[labels[spare[2:]], spare[2:]] = (np.nan, np.inf)
            labels[spare[:2]] = (-1, M)
    padded = np.full((M, ld), NAN_FILL, dtype=np.float32)
    padded[:, :N] = loss
    return padded, labels, N


def start(loss, labels, fit, kappa=1.0):
    """The start of a fit on a draw: kappa and c = 0, with c = -inf (a prior of zero) for the members without a used clip where the prior
    is fitted -- at a finite c such a member keeps a share of every clip that no finite prior of the others takes away, and J has no
    minimum."""
    M = loss.shape[0]
    c = np.zeros(M)
    if fit & FIT_PRIOR:
        c[evaluate(loss, labels, kappa, c).n_m == 0] = -np.inf
    return float(kappa), c


def normalised_prior(c):
    c = np.asarray(c, dtype=np.float64)
    fin = np.isfinite(c)
    top = np.max(c[fin])
    w = np.where(fin, np.exp(np.where(fin, c, top) - top), 0.0)
    return w / np.sum(w)


class CalibMethods:
    """Mixed into a stand-in backend: `bank_calibrate` / `read_calibrate_record` from this reference on host tensors, recording the
    arguments and counting the downloads."""

    def _calib_init(self):
        self.calib_calls, self.calib_downloads = [], 0

    def bank_calibrate(self, loss, labels, fit, kappa, log_prior=None, tol=1e-9, max_iter=200, kappa_min=1e-6, kappa_max=1e6):
        l, y = loss.detach().cpu().numpy(), labels.detach().cpu().numpy()
        M = l.shape[0]
        c0 = np.zeros(M) if log_prior is None else np.array(log_prior, dtype=np.float64)
        self.calib_calls.append(dict(shape=tuple(l.shape), fit=int(fit), kappa=float(kappa), log_prior=c0.copy(), tol=tol, max_iter=max_iter,
                                     kappa_min=kappa_min, kappa_max=kappa_max, loss=l.copy(), labels=y.copy()))
        before = evaluate(l, y, kappa, c0)
        if before.n == 0:
            return np.concatenate([[kappa], c0]), dict(xent_start=0.0, xent_end=0.0, g_logk=0.0, resid_prior=0.0, curvature=0.0, n_used=0,
                                                       n_unlabelled=before.n_unlabelled, n_own_absent=before.n_own_absent, passes=1,
                                                       flags=NO_DATA, n_unfitted=M, reserved=0)
        k, c, rounds = (kappa, c0, 1) if fit == 0 or max_iter == 0 else \
            optimise(l, y, fit, kappa, c0, kappa_min, kappa_max, np.float64, tol, rounds=min(max_iter, 60), strict=False)
        after = evaluate(l, y, k, c)
        at_min, at_max = bool(fit & 1 and k == kappa_min), bool(fit & 1 and k == kappa_max)
        done = (not fit & 1 or at_min or at_max or abs(float(k * after.g)) <= tol) and (not fit & 2 or after.resid() <= tol)
        flags = (CONVERGED if done else MAX_ITER) | (AT_KAPPA_MIN if at_min else 0) | (AT_KAPPA_MAX if at_max else 0)
        rec = dict(xent_start=float(before.J), xent_end=float(after.J), g_logk=float(k * after.g), resid_prior=after.resid() if fit & 2 else 0.0,
                   curvature=float(after.h), n_used=after.n, n_unlabelled=after.n_unlabelled, n_own_absent=after.n_own_absent, passes=rounds,
                   flags=flags, n_unfitted=int(np.sum(after.n_m == 0)), reserved=0)
        return np.concatenate([[float(k)], np.asarray(c, dtype=np.float64)]), rec

    def read_calibrate_record(self, out):
        self.calib_downloads += 1
        return out[0].copy(), dict(out[1])
