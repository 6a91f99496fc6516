"""cmps_rho_apply_step / cmps_rho_apply_step_scratch_bytes without a GPU: the symbols are exported, every argument check answers
CMPS_ERR_BAD_ARG with its message before anything touches the device, and the variable layout of the rho step packs and unpacks."""
import ctypes

import numpy as np
import pytest


def test_rho_apply_step_symbols_are_exported(hip_lib):
    from audio_mps_amd import _capi
    for name in ("cmps_rho_apply_step_scratch_bytes", "cmps_rho_apply_step"):
        assert name in _capi.SYMBOLS and hasattr(hip_lib, name), name
    assert hip_lib.cmps_version() == 500


def test_rho_apply_step_scratch_bytes(hip_lib):
    for D in (0, 129):
        assert hip_lib.cmps_rho_apply_step_scratch_bytes(D, 4) == 0
    for rank in (0, 129):
        assert hip_lib.cmps_rho_apply_step_scratch_bytes(8, rank) == 0
    # the column sums in double and the R gradients in float32 (W is updated in place): no smaller than that at any valid shape
    for D, rank in ((1, 1), (8, 3), (33, 40), (128, 128)):
        n = hip_lib.cmps_rho_apply_step_scratch_bytes(D, rank)
        assert n >= 2 * D * 8 + 2 * D * D * 4 and n % 8 == 0, (D, rank, n)


def test_rho_apply_step_argument_checks(hip_lib):
    from audio_mps_amd import _capi
    BAD = _capi.CMPS_ERR_BAD_ARG
    f = hip_lib.cmps_rho_apply_step
    h = ctypes.c_void_p()
    assert hip_lib.cmps_create(8, ctypes.byref(h)) == _capi.CMPS_OK
    z = [0.0] * 8                            # lr_t, beta1, beta2, epsilon, h_reg, r_reg, c_r, c_h
    p = 256                                  # a non-null, 8-byte aligned address: every call below is rejected before it is used

    def err():
        return hip_lib.cmps_last_error(h)

    assert f(None, p, p, p, p, 3, 4.0, *z, 1, p, p, p, p, None) == BAD                      # null handle
    # null vars / params / phi
    for vars_, params, phi in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(h, vars_, p, p, p, 3, 4.0, *z, 1, params, phi, p, p, None) == BAD
        assert b"cmps_rho_apply_step: null variable / parameter / column buffer" in err()
    # also without an update (grad_sums NULL) those three are needed
    assert f(h, None, None, None, None, 3, 0.0, *z, 1, None, None, None, None, None) == BAD and b"null variable" in err()
    # rank outside [1, 128]
    for rank in (0, -1, 129):
        assert f(h, p, p, p, p, rank, 4.0, *z, 1, p, p, p, p, None) == BAD
        assert b"rank outside [1, 128]" in err()
    assert f(h, p, None, None, None, 129, 0.0, *z, 1, p, p, None, None, None) == BAD and b"rank outside" in err()
    # an update (grad_sums given) needs the Adam slots, the loss outputs, the scratch buffer and a positive batch
    for m_, v_, losses, scratch, batch in ((None, p, p, p, 4.0), (p, None, p, p, 4.0), (p, p, None, p, 4.0), (p, p, p, None, 4.0),
                                           (p, p, p, p, 0.0), (p, p, p, p, -2.0), (p, p, p, p, float("nan"))):
        assert f(h, p, m_, v_, p, 3, batch, *z, 1, p, p, losses, scratch, None) == BAD
        assert b"an update needs the Adam slots, losses_dev, scratch_dev and a positive batch" in err()
    # misaligned scratch, with and without an update
    assert f(h, p, p, p, p, 3, 4.0, *z, 1, p, p, p, 260, None) == BAD and b"scratch_dev must be 8-byte aligned" in err()
    assert f(h, p, None, None, None, 3, 0.0, *z, 1, p, p, None, 260, None) == BAD and b"8-byte aligned" in err()
    hip_lib.cmps_destroy(h)


@pytest.mark.parametrize("D,rank", [(1, 1), (5, 3), (12, 12), (33, 40), (128, 128)])
def test_rho_variable_layout_round_trip(D, rank):
    from audio_mps_amd import layout
    fields = layout.var_fields(D, rank)
    assert tuple(k for k, _ in fields) == layout.RHO_VAR_ORDER == ("A", "Rx", "Ry", "freqs", "Wx", "Wy")
    assert layout.size(fields) == 2 * D * D + D + 1 + 2 * rank * D
    rng = np.random.default_rng(D * 1000 + rank)
    values = {k: rng.standard_normal(shape).astype(np.float32) for k, shape in fields}
    flat = layout.pack(fields, values)
    assert flat.dtype == np.float32 and flat.shape == (layout.size(fields),)
    back = layout.unpack(fields, flat)
    for k, shape in fields:
        assert np.shape(back[k]) == shape and np.array_equal(back[k], values[k]), k
    # buffer order: A first, Wx then Wy at the end, row-major [a][d]
    assert flat[0] == values["A"] and np.array_equal(flat[-rank * D:], values["Wy"].ravel())
    assert np.array_equal(flat[-2 * rank * D:-rank * D], values["Wx"].ravel())
    # the pure-state layout is untouched
    assert tuple(k for k, _ in layout.var_fields(D)) == layout.VAR_ORDER == ("A", "Rx", "Ry", "freqs", "psi_x", "psi_y")
    assert layout.size(layout.var_fields(D)) == 2 * D * D + 3 * D + 1


def test_rho_model_variables_pack_into_the_layout():
    """RhoCMPS.variables (A a 0-d array, Wx / Wy [rank, D]) fill the layout the Trainer uploads; flat_size is the gradient buffer's."""
    from audio_mps_amd import HParams, RhoCMPS, layout
    m = RhoCMPS(HParams(bond_dim=6, initial_rank=4), seed=2, backend=object())
    fields = layout.var_fields(6, m.rank_rho_0)
    flat = layout.pack(fields, m.variables)
    assert flat.size == 2 * 36 + 6 + 1 + 2 * 4 * 6 and m.flat_size() == 2 * 36 + 3 * 6 + 2 + 2 * 4 * 6
    back = layout.unpack(fields, flat)
    assert all(np.array_equal(back[k], m.variables[k]) for k in RhoCMPS.VARIABLE_NAMES)
