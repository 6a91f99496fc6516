"""The parameter-derived tables the kernels of cmps_prep.hip (k_ttable, k_pack, k_rho_raw, k_rho_fix, k_qflag), cmps_legacy.hip
(k_pack_legacy, k_legacy_tables) and cmps_rho.hip (k_pack_phi) leave in the caller's workspace, downloaded and held to the contract of
tests/_tables_ref.py: in bits where the contract is exact, at bounds derived from float32 rounding elsewhere.  Each case is one
set_params-class call on a guarded, pattern-filled workspace (tests/_guard.py), one download and no scan; every case prints its worst
observed value next to its bound (profiles/prep_tables_bounds.log holds the `TABLES MI355X` lines of one `pytest -s` run of this file, as
printed but for pytest's progress dots in front of some of them)."""
import numpy as np
import pytest

import _tables_ref as TR
from _guard import NAN_FILL, Driver

pytestmark = pytest.mark.gpu

B_MAX = 1
REUSE = 4            # CMPS_WS_REUSE_TABLES
SIGMA, DT0 = 0.36, TR.DT[0]


@pytest.fixture
def drivers():
    made = []

    def make(D):
        made.append(Driver(D))
        return made[-1]
    yield make
    for d in made:
        d.close()


def _ws(drv, name, nbytes):
    if name not in drv.bufs:
        drv.new(name, nbytes)
    assert drv.bufs[name].nbytes >= nbytes
    return drv.bufs[name]


def _main_bytes(drv, T, flags=0):
    n = int(drv.lib.cmps_workspace_bytes(drv.D, B_MAX, T, flags & 1))
    assert n > 0
    return n


def psi_call(drv, T, params, sigma, dt, entry="cmps_set_params", flags=0, ws="ws", ws_bytes=None):
    """One cmps_set_params / cmps_set_params_dev of the packed buffer `params` (a buffer name) at B_max = 1; the workspace's bytes."""
    D = drv.D
    g, w = drv.bufs[params], _ws(drv, ws, ws_bytes or _main_bytes(drv, T, flags))
    if entry == "cmps_set_params":
        DD = 4 * D * D
        ptrs = [g.ptr + o for o in (0, DD, 2 * DD, 2 * DD + 4 * D, 2 * DD + 8 * D)]
        A = float(g.numpy()[-1])
        drv.call(entry, *ptrs, A, float(sigma), float(dt), int(T), B_MAX, int(flags), w, w.nbytes)
    else:
        drv.call(entry, g, float(sigma), float(dt), int(T), B_MAX, int(flags), w, w.nbytes)
    return w.numpy(np.uint8)


def fresh_bits(make, D, T, row, sigma=SIGMA, dt=DT0, entry="cmps_set_params_dev"):
    """The tables of a fresh handle on a fresh workspace for the packed parameters `row`."""
    drv = make(D)
    drv.load("params", row)
    return TR.Tables(psi_call(drv, T, "params", sigma, dt, entry=entry), D, T).bits()


def _case(make, case, entry="cmps_set_params"):
    D, N, dt, sigma, r_scale, roll = case
    R, psi0, freqs = TR.case_inputs(D, r_scale=r_scale, roll=roll)
    drv = make(D)
    drv.load("params", TR.pack_params(R, psi0, freqs, A=1.5))
    raw = psi_call(drv, N + 1, "params", sigma, dt, entry=entry)
    assert TR.layout(D, N + 1)["end"] == raw.size                              # the restated layout ends where the library's does
    return TR.Tables(raw, D, N + 1), (R, psi0, freqs, sigma, dt)


@pytest.mark.parametrize("case", TR.CASES + TR.LONG_CASES, ids=TR.case_id)
def test_psi_tables_hold_the_contract(drivers, case):
    t, inputs = _case(drivers, case)
    rows = TR.check_psi(t, *inputs)
    TR.report("MI355X " + TR.case_id(case), rows)
    assert np.all(TR.words(t.QT) == NAN_FILL)                                  # not a table of this mode: nothing may have written it


@pytest.mark.parametrize("case", [TR.CASES[3], TR.CASES[8], TR.CASES[13]], ids=TR.case_id)
def test_set_params_dev_builds_the_same_bits(drivers, case):
    a, _ = _case(drivers, case, "cmps_set_params")
    b, _ = _case(drivers, case, "cmps_set_params_dev")
    TR.same_bits(a.bits(), b.bits(), "cmps_set_params_dev against cmps_set_params")


@pytest.mark.parametrize("D", [20, 40])
def test_reused_workspace_holds_what_a_fresh_one_does(drivers, D):
    """One handle, one workspace, CMPS_WS_REUSE_TABLES: T 66 -> 130 -> 66, then another dt at the same T, then other parameters at the
    same T and dt (the one call whose time table is really reused)."""
    rows = [TR.pack_params(*TR.case_inputs(D, seed=s, roll=s), A=2.0) for s in (0, 1)]
    drv = drivers(D)
    drv.load("p0", rows[0])
    drv.load("p1", rows[1])
    nbytes = _main_bytes(drv, 130)
    for step, (T, dt, p) in enumerate([(66, DT0, 0), (130, DT0, 0), (66, DT0, 0), (66, TR.DT[1], 0), (66, TR.DT[1], 1)]):
        raw = psi_call(drv, T, f"p{p}", SIGMA, dt, flags=REUSE, ws_bytes=nbytes)
        TR.same_bits(TR.Tables(raw, D, T).bits(), fresh_bits(drivers, D, T, rows[p], dt=dt, entry="cmps_set_params"),
                     f"reuse step {step} (T = {T}, dt = {dt:.3g})")


@pytest.mark.parametrize("D", [20, 40])
def test_two_T_share_the_table_below_the_last_full_chunk(drivers, D):
    """include/cmps.h, the stream contract: "A different T moves the drift-corrected last row of the final 64-step chunk" -- and nothing
    below the last 64-step boundary of the shorter table (T = 66: steps [0, 64), its last chunk is the single step 64)."""
    row = TR.pack_params(*TR.case_inputs(D, roll=2))
    tabs = {}
    for T in (66, 130):
        drv = drivers(D)
        drv.load("params", row)
        tabs[T] = TR.Tables(psi_call(drv, T, "params", SIGMA, DT0), D, T)
    a, b = tabs[66], tabs[130]
    edge = (a.N // 64) * 64
    assert edge == 64 and a.N % 64 != 0
    TR.same_bits({"ttab": TR.words(a.ttab[:edge + 1]), "dtk": TR.words(a.dtk[:edge]), "rho": TR.words(a.rho[:edge])},
                 {"ttab": TR.words(b.ttab[:edge + 1]), "dtk": TR.words(b.dtk[:edge]), "rho": TR.words(b.rho[:edge])}, "T = 66 against T = 130")
    # and the row the contract says moves does move: the longer table's step 64 is an ordinary entry, the shorter one's is corrected
    assert np.any(TR.words(a.rho[edge, :D]) != TR.words(b.rho[edge, :D]))


# ---- banks ----
def _bank_rows(D, M, first=0):
    members = [TR.case_inputs(D, seed=20 + first + m, roll=first + m) for m in range(M)]
    return members, np.stack([TR.pack_params(*mem, A=1.0 + first + m) for m, mem in enumerate(members)])


def _bank_call(drv, T, params, M, flags, ws_bytes):
    w = _ws(drv, "ws", ws_bytes)
    drv.call("cmps_bank_set_params_dev", int(M), drv.bufs[params], SIGMA, DT0, int(T), B_MAX, int(flags), w, w.nbytes)
    return w.numpy(np.uint8)


@pytest.mark.parametrize("D", [8, 20])
@pytest.mark.parametrize("train", [0, 1])
def test_bank_members_hold_the_plain_tables(drivers, D, train):
    T, M = 66, 3
    members, rows = _bank_rows(D, M)
    drv = drivers(D)
    drv.load("params", rows)
    stride = _main_bytes(drv, T, train)
    assert int(drv.lib.cmps_bank_workspace_bytes(D, M, B_MAX, T, train)) == M * stride
    raw = _bank_call(drv, T, "params", M, train, M * stride)
    for m in range(M):
        t = TR.Tables(raw, D, T, m * stride)
        TR.report(f"MI355X bank D{D} train{train} member {m}", TR.check_psi(t, *members[m], SIGMA, DT0))
        TR.same_bits(t.bits(), fresh_bits(drivers, D, T, rows[m]), f"bank member {m} against a plain handle")


@pytest.mark.parametrize("D", [8, 20])
def test_bank_plain_bank_walk_leaves_fresh_bits(drivers, D):
    T = 66
    _, rows3 = _bank_rows(D, 3)
    _, rows2 = _bank_rows(D, 2, first=3)
    drv = drivers(D)
    drv.load("p3", rows3)
    drv.load("p2", rows2)
    drv.load("p1", rows3[1])
    stride = _main_bytes(drv, T)
    raw = _bank_call(drv, T, "p3", 3, REUSE, 3 * stride)
    for m in range(3):
        TR.same_bits(TR.Tables(raw, D, T, m * stride).bits(), fresh_bits(drivers, D, T, rows3[m]), f"bank of 3, member {m}")
    raw = psi_call(drv, T, "p1", SIGMA, DT0, entry="cmps_set_params_dev", flags=REUSE)
    TR.same_bits(TR.Tables(raw, D, T).bits(), fresh_bits(drivers, D, T, rows3[1]), "plain after the bank")
    raw = _bank_call(drv, T, "p2", 2, REUSE, 2 * stride)
    for m in range(2):
        TR.same_bits(TR.Tables(raw, D, T, m * stride).bits(), fresh_bits(drivers, D, T, rows2[m]), f"bank of 2 after plain, member {m}")


# ---- RhoCMPS: phi0, and the bank of RhoCMPS members ----
def _phi(D, rank, seed):
    rng = np.random.default_rng(7000 + 100 * D + rank + seed)
    return (rng.standard_normal((rank, D)) + 1j * rng.standard_normal((rank, D))).astype(np.complex64)


def _phi_row(phi):
    return np.concatenate([phi.real.reshape(-1), phi.imag.reshape(-1)]).astype(np.float32)


def _rho_plain(drv, T, params, phi_name, rank, flags=0):
    """cmps_set_params_dev + cmps_rho_set_state on a plain handle: (main workspace bytes, rho workspace bytes)."""
    raw = psi_call(drv, T, params, SIGMA, DT0, entry="cmps_set_params_dev", flags=flags)
    n = int(drv.lib.cmps_rho_workspace_bytes(drv.D, rank, B_MAX, T, 0))
    assert n > 0
    w, g = _ws(drv, "rho_ws", n), drv.bufs[phi_name]
    drv.call("cmps_rho_set_state", g.ptr, g.ptr + 4 * rank * drv.D, int(rank), int(T), B_MAX, 0, w, w.nbytes)
    return raw, w.numpy(np.uint8)


@pytest.mark.parametrize("D", [5, 40])
@pytest.mark.parametrize("rank", [1, 5, 40])
def test_phi0_is_an_exact_zero_padded_copy(drivers, D, rank):
    T = 66
    phi = _phi(D, rank, 0)
    drv = drivers(D)
    drv.load("params", TR.pack_params(*TR.case_inputs(D)))
    drv.load("phi", _phi_row(phi))
    _, rho_raw = _rho_plain(drv, T, "params", "phi", rank)
    TR.report(f"MI355X phi0 D{D} rank{rank}", TR.check_phi0(TR.phi0_view(rho_raw, D, rank), phi))


def _rho_bank_call(drv, T, params, phi, M, rank, flags, ws_bytes):
    w = _ws(drv, "ws", ws_bytes)
    drv.call("cmps_rho_bank_set_state_dev", int(M), drv.bufs[params], drv.bufs[phi], int(rank), SIGMA, DT0, int(T), B_MAX, int(flags), w, w.nbytes)
    return w.numpy(np.uint8)


def _fresh_rho(make, D, T, row, phi, rank):
    drv = make(D)
    drv.load("params", row)
    drv.load("phi", _phi_row(phi))
    raw, rho_raw = _rho_plain(drv, T, "params", "phi", rank)
    return TR.Tables(raw, D, T).bits(), TR.words(TR.phi0_view(rho_raw, D, rank))


def _assert_rho_member(make, raw, D, T, rank, m, stride, main, row, phi, what):
    bits, phi_bits = _fresh_rho(make, D, T, row, phi, rank)
    TR.same_bits(TR.Tables(raw, D, T, m * stride).bits(), bits, what)
    got = TR.phi0_view(raw, D, rank, m * stride + main)
    TR.check_phi0(got, phi)
    TR.same_bits({"phi0": TR.words(got)}, {"phi0": phi_bits}, what)


def test_rho_bank_members_and_walk(drivers):
    D, rank, T = 12, 5, 66
    members, rows3 = _bank_rows(D, 3)
    _, rows2 = _bank_rows(D, 2, first=3)
    phis3, phis2 = [_phi(D, rank, m) for m in range(3)], [_phi(D, rank, 3 + m) for m in range(2)]
    drv = drivers(D)
    drv.load("p3", rows3)
    drv.load("p2", rows2)
    drv.load("p1", rows3[1])
    drv.load("f3", np.stack([_phi_row(p) for p in phis3]))
    drv.load("f2", np.stack([_phi_row(p) for p in phis2]))
    drv.load("f1", _phi_row(phis3[1]))
    main = _main_bytes(drv, T)
    stride = main + int(drv.lib.cmps_rho_workspace_bytes(D, rank, B_MAX, T, 0))
    assert int(drv.lib.cmps_rho_bank_workspace_bytes(D, rank, 3, B_MAX, T, 0)) == 3 * stride
    raw = _rho_bank_call(drv, T, "p3", "f3", 3, rank, REUSE, 3 * stride)
    for m in range(3):
        TR.report(f"MI355X rho bank D{D} rank{rank} member {m}", TR.check_psi(TR.Tables(raw, D, T, m * stride), *members[m], SIGMA, DT0))
        _assert_rho_member(drivers, raw, D, T, rank, m, stride, main, rows3[m], phis3[m], f"rho bank of 3, member {m}")
    raw, rho_raw = _rho_plain(drv, T, "p1", "f1", rank, flags=REUSE)
    bits, phi_bits = _fresh_rho(drivers, D, T, rows3[1], phis3[1], rank)
    TR.same_bits(TR.Tables(raw, D, T).bits(), bits, "plain after the rho bank")
    TR.same_bits({"phi0": TR.words(TR.phi0_view(rho_raw, D, rank))}, {"phi0": phi_bits}, "plain after the rho bank")
    raw = _rho_bank_call(drv, T, "p2", "f2", 2, rank, REUSE, 2 * stride)
    for m in range(2):
        _assert_rho_member(drivers, raw, D, T, rank, m, stride, main, rows2[m], phis2[m], f"rho bank of 2 after plain, member {m}")


# ---- legacy mode ----
@pytest.mark.parametrize("D", [5, 40])
def test_legacy_tables(drivers, D):
    T = 66
    rng = np.random.default_rng(300 + D)
    R = rng.standard_normal((D, D)).astype(np.float32)
    Q = (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))).astype(np.complex64)
    drv = drivers(D)
    g = drv.load("params", np.concatenate([R.reshape(-1), Q.real.reshape(-1), Q.imag.reshape(-1)]).astype(np.float32))
    w = _ws(drv, "ws", _main_bytes(drv, T))
    drv.call("cmps_legacy_set_params", g.ptr, g.ptr + 4 * D * D, g.ptr + 8 * D * D, DT0, T, B_MAX, 0, w, w.nbytes)
    TR.report(f"MI355X legacy D{D}", TR.check_legacy(TR.Tables(w.numpy(np.uint8), D, T), R, Q))
