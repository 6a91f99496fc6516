"""tests/_tables_ref.py without a GPU: the restated layout ends where the library says a tables-only workspace ends, the numpy restatement
of the tables passes every check of the contract on every case of tests/test_gpu_tables.py, and each deliberately wrong table is
rejected by the check that owns it -- the mutant changes only the table, never a bound."""
import numpy as np
import pytest

import _tables_ref as TR

ALL_CASES = TR.CASES + TR.LONG_CASES


def _built(case, mutant=None):
    D, N, dt, sigma, r_scale, roll = case
    R, psi0, freqs = TR.case_inputs(D, r_scale=r_scale, roll=roll)
    raw = TR.blank(TR.layout(D, N + 1)["end"])
    return TR.build_psi(raw, D, N + 1, R, psi0, freqs, sigma, dt, mutant=mutant), (R, psi0, freqs, sigma, dt)


@pytest.mark.parametrize("B", [1, 3])
def test_layout_ends_where_the_library_says(hip_lib, B):
    for D, N, *_ in ALL_CASES:
        L = TR.layout(D, N + 1)
        assert all(off % 256 == 0 for off, _ in (L[s] for s in TR.SECTIONS))
        assert L["end"] == hip_lib.cmps_workspace_bytes(D, B, N + 1, 0), (D, N)
    # a tables-only rho workspace whose columns fit the LDS is its phi0 section alone
    for D, rank in ((5, 1), (5, 5), (12, 5), (40, 5), (40, 40)):
        assert hip_lib.cmps_rho_workspace_bytes(D, rank, B, 66, 0) == TR.align256(rank * TR.padded(D) * 8)
    assert hip_lib.cmps_rho_bank_workspace_bytes(12, 5, 3, B, 66, 0) == 3 * (TR.layout(12, 66)["end"] + TR.align256(5 * 32 * 8))


@pytest.mark.parametrize("case", ALL_CASES, ids=TR.case_id)
def test_restatement_passes_its_own_checks(case):
    t, inputs = _built(case)
    rows = TR.check_psi(t, *inputs)
    TR.report("numpy " + TR.case_id(case), rows)
    assert len(rows) >= 13
    # nothing outside the sections was written, and QT / rfix are not part of the PsiCMPS contract: still the blank pattern
    assert np.all(TR.words(t.QT) == TR.NAN_WORD)


def test_blank_pattern_is_the_guards():
    from _guard import NAN_FILL
    assert TR.NAN_WORD == NAN_FILL


def test_both_qflag_values_occur_at_64():
    flags = {int(_built(c)[0].qflag[0]) for c in TR.CASES if c[0] == 64 and c[3] == 0.36}
    assert flags == {0, 1}


def test_last_chunks_cover_the_edges():
    N = sorted({c[1] for c in TR.CASES})
    assert N == [1, 33, 63, 64, 65, 97, 191, 256, 289, 543]
    assert sorted({(n + 63) // 64 for n in N}) == [1, 2, 3, 4, 5, 9]
    assert {1, 33, 63, 64} <= {n - (n - 1) // 64 * 64 for n in N}
    assert sorted({c[0] for c in TR.CASES}) == [1, 16, 31, 32, 33, 64, 128]
    assert {c[2] for c in TR.CASES} == set(TR.DT) and {c[3] for c in TR.CASES} == {1e-4, 0.36}


# ---- the wrong tables: (mutant, the check that owns it, the cases it is shown on) ----
def _time(t, i): return TR.check_time_grid(t, i[4])
def _packed(t, i): return TR.check_packed(t, *i[:3])
def _q(t, i): return TR.check_q(t, i[0], i[3], i[4])
def _entries(t, i): return TR.check_rho_entries(t)
def _product(t, i): return TR.check_rho_accumulated(t)


CHUNKS_33_63 = tuple(c for c in ALL_CASES if c[1] % 64 in (33, 63))
MUTANT_CASES = [
    ("no_drift_correction", _product, tuple(c for c in ALL_CASES if c[1] > 1)),         # (N = 1: one rounding, a corrected entry is no closer)
    ("partial_chunk_uncorrected", _product, CHUNKS_33_63),
    ("t_is_k_dt", _time, tuple(c for c in ALL_CASES if c[1] >= 63)),
    ("delta_from_dt", _entries, tuple(c for c in ALL_CASES if c[1] >= 33)),
    ("dtk_padding", _time, TR.CASES),
    ("rt_not_transposed", _packed, tuple(c for c in TR.CASES if c[0] > 1)),             # (a 1 x 1 matrix is its own transpose)
    ("padding_lane", _entries, TR.CASES),
    ("q_float32", _q, tuple(c for c in TR.CASES if c[0] == 128)),
]


def test_every_mutant_of_the_issue_is_listed():
    assert {m for m, _, _ in MUTANT_CASES} == set(TR.MUTANTS)
    assert {c[1] % 64 for c in CHUNKS_33_63} == {33, 63}


@pytest.mark.parametrize("mutant,owner,cases", MUTANT_CASES, ids=[m for m, _, _ in MUTANT_CASES])
def test_mutant_is_rejected_by_its_owner(mutant, owner, cases):
    assert cases
    for case in cases:
        t, inputs = _built(case, mutant)
        with pytest.raises(AssertionError):
            owner(t, inputs)
        good, _ = _built(case)
        owner(good, inputs)                                                    # the same check accepts the right table
        print(f"TABLES mutant {mutant} on {TR.case_id(case)}: rejected")


# ---- banks, legacy, phi0 ----
def _bank_image(D, T, M, stride):
    raw = TR.blank(M * stride)
    members = [TR.case_inputs(D, seed=10 + m, roll=m) for m in range(M)]
    for m, (R, psi0, freqs) in enumerate(members):
        TR.build_psi(raw, D, T, R, psi0, freqs, 0.36, TR.DT[0], base=m * stride)
    return raw, members


@pytest.mark.parametrize("D", [8, 20])
def test_bank_members_lie_one_workspace_apart(hip_lib, D):
    T, M, B = 66, 3, 2
    for flags in (0, 1):
        stride = hip_lib.cmps_workspace_bytes(D, B, T, flags)
        assert hip_lib.cmps_bank_workspace_bytes(D, M, B, T, flags) == M * stride
        raw, members = _bank_image(D, T, M, stride)
        for m, inputs in enumerate(members):
            TR.check_psi(TR.Tables(raw, D, T, m * stride), *inputs, 0.36, TR.DT[0])
        # a member read at the wrong stride: the echo check owns it
        for wrong in (stride - 256, stride + 256, TR.layout(D, T)["end"] if flags else stride + 512):
            for m in (1, 2):
                if m * wrong + TR.layout(D, T)["end"] > raw.size:
                    continue
                with pytest.raises(AssertionError):
                    TR.check_echo(TR.Tables(raw, D, T, m * wrong), *members[m])
        print(f"TABLES mutant wrong bank stride at D = {D}, flags = {flags}: rejected")


@pytest.mark.parametrize("D", [5, 40])
def test_legacy_and_phi0_restatement(D):
    T = 66
    rng = np.random.default_rng(D)
    R = rng.standard_normal((D, D)).astype(np.float32)
    Q = (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))).astype(np.complex64)
    raw = TR.blank(TR.layout(D, T)["end"])
    t = TR.build_legacy(raw, D, T, R, Q)
    assert len(TR.check_legacy(t, R, Q)) == 7
    t.QT[:] = t.Q
    with pytest.raises(AssertionError):
        TR.check_legacy(t, R, Q)
    for rank in (1, 5, 40):
        phi = (rng.standard_normal((rank, D)) + 1j * rng.standard_normal((rank, D))).astype(np.complex64)
        raw = TR.blank(TR.align256(rank * TR.padded(D) * 8))
        got = TR.build_phi0(raw, D, phi)
        TR.check_phi0(got, phi)
        got[rank - 1, D] = 1e-30
        with pytest.raises(AssertionError):
            TR.check_phi0(got, phi)
