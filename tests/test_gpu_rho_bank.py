"""The RhoCMPS model bank on the GPU (cmps_rho_bank_*, audio_mps_amd/bank.py::RhoBank): member m of a bank gives, BIT FOR BIT, what a
plain handle gives for model m alone -- the kernels are the plain ones with a member grid dimension, every member working in its own
region (main tables + rho layout) of the bank's one workspace.

Every comparison is np.array_equal on the raw float32 bits against a fresh plain handle, or a plain Trainer(device_step=True), per
member.  That bar rests on the plain path being reproducible, which test_plain_path_is_reproducible checks first.

Shapes (D, rank, T, B, M): B * rank is no multiple of the 4 clips per workgroup, T is off the 64- and 32-step chunks and off the 8-step
octets, rank lies below and above the forward-only switch at 8 (k_fwd_rho_wave / k_fwd_rho_mfma<false>), D below, at and above 16.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from audio_mps_amd import HParams, RhoCMPS, _capi, layout

from _guard import Guarded
from _util import make_audio

pytestmark = pytest.mark.gpu

#         D  rank  T   B  M
SHAPES = [(3, 3, 70, 3, 3),
          (8, 8, 130, 2, 5),
          (16, 5, 100, 3, 4),
          (17, 9, 100, 3, 3),
          (32, 32, 70, 2, 3)]
IDS = [f"D{s[0]}-r{s[1]}" for s in SHAPES]
SOME = [SHAPES[0], SHAPES[3]]
SOME_IDS = [IDS[0], IDS[3]]
TRAIN = _capi.CMPS_WS_TRAIN


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def hparams(D, rank, B, **kw):
    return HParams(minibatch_size=B, bond_dim=D, initial_rank=rank, **kw)


def member_arrays(D, rank, B, seed):
    """RhoCMPS(seed) as the two buffers the device entries read: params R_re | R_im | freqs | psi0_re | psi0_im | A, phi phi_re | phi_im."""
    mo = RhoCMPS(hparams(D, rank, B), seed=seed, backend=object())
    p = mo.effective_params()
    params = layout.pack(layout.param_fields(D, with_A=True), {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})
    return params, layout.pack(layout.phi_fields(D, rank), layout.split("phi", mo.columns()))


def plain_run(D, rank, params, phi, audio, hp, be=None, save=True, events=False):
    """One model on the plain entries: (losses, gradient sums or None, kernel names or None)."""
    from audio_mps_amd.scan import HipScan
    be = HipScan(D) if be is None else be
    B, T = audio.shape
    p, f = torch.from_numpy(params).cuda(), torch.from_numpy(phi).cuda()      # (held until the scans have run)
    be.set_params_dev(p, hp.sigma, hp.delta_t, B, T, train=False)
    be.rho_set_state_dev(f, rank, B, T, train=save)
    if events:
        be.kernel_events(True)
    loss = be.rho_forward(torch.from_numpy(audio).cuda(), save_for_bwd=save).clone()
    grad = be.rho_backward().clone() if save else None
    torch.cuda.synchronize()
    names = list(be.kernel_times()) if events else None
    return loss.cpu().numpy(), None if grad is None else grad.cpu().numpy(), names


def bank_run(D, rank, params, phi, audio, hp, be=None, calls=1, save=True, events=False):
    """Bank forward (+ backward); audio [B, T] (shared) or [M, B, T].  calls = 2: set_state twice (the second with CMPS_WS_REUSE_TABLES)."""
    from audio_mps_amd.scan import HipScan
    be = HipScan(D) if be is None else be
    B, T = audio.shape[-2:]
    p, f = torch.from_numpy(np.ascontiguousarray(params)).cuda(), torch.from_numpy(np.ascontiguousarray(phi)).cuda()
    for _ in range(calls):
        be.rho_bank_set_state_dev(p, f, rank, hp.sigma, hp.delta_t, B, T, train=save)
    if events:
        be.kernel_events(True)
    loss = be.rho_bank_forward(torch.from_numpy(np.ascontiguousarray(audio)).cuda(), save_for_bwd=save)
    grad = be.rho_bank_backward() if save else None
    torch.cuda.synchronize()
    names = list(be.kernel_times()) if events else None
    return loss.cpu().numpy(), None if grad is None else grad.cpu().numpy(), names


_CASES = {}


def case(shape):
    """(params [M, NP], phi [M, 2 rank D], audio [M, B, T], plain (loss, grad) per member, hp) of a shape, computed once: every member
    on a FRESH plain handle."""
    if shape not in _CASES:
        D, rank, T, B, M = shape
        hp = hparams(D, rank, B)
        arrays = [member_arrays(D, rank, B, 100 + m) for m in range(M)]
        params, phi = np.stack([a[0] for a in arrays]), np.stack([a[1] for a in arrays])
        audio = np.stack([make_audio(B, T, hp.delta_t, seed=7 + m) for m in range(M)])
        plain = [plain_run(D, rank, params[m], phi[m], audio[m], hp)[:2] for m in range(M)]
        _CASES[shape] = (params, phi, audio, plain, hp)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plain_path_is_reproducible(shape):
    """What the bit-for-bit bar rests on: the plain forward + backward twice on ONE handle, and on a second one, give the same bits."""
    from audio_mps_amd.scan import HipScan
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    be = HipScan(D)
    a = plain_run(D, rank, params[0], phi[0], audio[0], hp, be)
    b = plain_run(D, rank, params[0], phi[0], audio[0], hp, be)
    assert same(a[0], b[0]) and same(a[1], b[1]), "the plain path is not reproducible"
    assert same(a[0], plain[0][0]) and same(a[1], plain[0][1]), "a second handle gives other bits"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_own_and_shared_audio(shape):
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    loss, grad, _ = bank_run(D, rank, params, phi, audio, hp)
    assert loss.shape == (M, B) and grad.shape == (M, layout.grad_size(D, rank))
    for m in range(M):
        assert same(loss[m], plain[m][0]), (m, loss[m], plain[m][0])
        assert same(grad[m], plain[m][1]), m
    assert not same(loss[0], loss[1]) and not same(grad[0], grad[1])          # (the members do differ)
    # one batch shared by every member (n_audio = 1) = M copies of it
    shared = audio[1]
    l1, g1, _ = bank_run(D, rank, params, phi, shared, hp)
    lM, gM, _ = bank_run(D, rank, params, phi, np.stack([shared] * M), hp)
    assert same(l1, lM) and same(g1, gM)
    ref = plain_run(D, rank, params[1], phi[1], shared, hp)
    assert same(l1[1], ref[0]) and same(g1[1], ref[1])
    assert not same(l1[0], l1[1])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_only_losses_and_kernel_names(shape):
    """save_for_bwd = 0 on a FWD_ONLY workspace: k_fwd_rho_wave up to rank 8, k_fwd_rho_mfma<false> above; the recorded names are the
    plain handle's."""
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    loss, _, names = bank_run(D, rank, params, phi, audio, hp, save=False, events=True)
    refs = [plain_run(D, rank, params[m], phi[m], audio[m], hp, save=False, events=(m == 0)) for m in range(M)]
    for m in range(M):
        assert same(loss[m], refs[m][0]), m
    assert names == refs[0][2] == ["k_fwd_rho_wave" if rank <= 8 else "k_fwd_rho_mfma"]
    # ... and of a training step
    _, _, names = bank_run(D, rank, params, phi, audio, hp, events=True)
    assert names == plain_run(D, rank, params[0], phi[0], audio[0], hp, events=True)[2] == ["k_fwd_rho_mfma", "k_bwd_wave2w", "reduce + finalize"]


@pytest.mark.parametrize("shape", SOME, ids=SOME_IDS)
def test_one_member_equals_the_plain_entries_and_a_permuted_bank(shape):
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    loss, grad, _ = bank_run(D, rank, params[:1], phi[:1], audio[:1], hp)
    assert same(loss[0], plain[0][0]) and same(grad[0], plain[0][1])
    perm = [2, 0, 1]
    la, ga, _ = bank_run(D, rank, params[:3], phi[:3], audio[:3], hp)
    lb, gb, _ = bank_run(D, rank, params[perm], phi[perm], audio[perm], hp)
    assert same(lb, la[perm]) and same(gb, ga[perm])


MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1},
           {"seed": 4, "learning_rate": 3e-3, "h_reg": 4e-7, "r_reg": 1.0},
           {"seed": 5, "learning_rate": 2e-4, "h_reg": 9e-8, "r_reg": 0.03}]


@pytest.mark.parametrize("shape", SOME, ids=SOME_IDS)
def test_three_optimiser_steps_equal_plain_device_trainers(shape):
    """vars, adam_m, adam_v, params, phi and losses after every step against M plain Trainer(device_step=True) runs on fresh handles;
    the members' learning_rate, h_reg and r_reg all differ."""
    from audio_mps_amd.bank import BankTrainer, RhoBank
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    D, rank, T, B, _ = shape
    hp = hparams(D, rank, B)
    bank = RhoBank(hp, MEMBERS, backend=HipScan(D))
    bt = BankTrainer(bank)
    assert bt.native and bt.rank == rank
    plain = [Trainer(RhoCMPS(h, seed=s, backend=HipScan(D)), h, device_step=True) for h, s in zip(bank.member_hparams, bank.seeds)]
    M = len(MEMBERS)
    for step in range(3):
        audio = np.stack([make_audio(B, T, hp.delta_t, seed=50 + 10 * step + m) for m in range(M)])
        out = bt.step(audio, sync=True)
        for m, tr in enumerate(plain):
            ref = tr.step(audio[m], sync=True)
            for name in ("vars", "m", "v", "params", "phi", "losses"):
                assert same(bt._dev[name][m], tr._dev[name]), (step, m, name)
            assert np.float32(ref["model_loss"]) == out["model_loss"][m] and np.float32(ref["total_loss"]) == out["total_loss"][m]
    for m, tr in enumerate(plain):
        mine = bt.member(m)
        for k, v in tr.model.variables.items():
            assert same(mine.variables[k], v), (m, k)
        assert bt.trainers[m].opt.t == tr.opt.t == 3


def apply_args(D, rank, B, M):
    models = [RhoCMPS(hparams(D, rank, B), seed=100 + m, backend=object()) for m in range(M)]
    fields = layout.var_fields(D, rank)
    v0 = np.stack([layout.pack(fields, mo.variables) for mo in models])
    hyper = np.array([[1e-3 * (m + 1), mo.h_reg, mo.r_reg, float(mo._c_r), float(mo._c_h)] for m, mo in enumerate(models)], dtype=np.float64)
    return v0, hyper


def test_a_nan_member_does_not_disturb_its_neighbours():
    """Member 1's W holds a NaN (so every column of its rho_0 does): members 0 and 2 keep the bits of the clean bank in the losses, the
    gradients and the next variables; member 1 comes out exactly as the plain path leaves that model."""
    from audio_mps_amd.scan import HipScan
    shape = SHAPES[0]
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    dirty = phi.copy()
    dirty[1] = np.nan
    lc, gc, _ = bank_run(D, rank, params, phi, audio, hp)
    ld, gd, _ = bank_run(D, rank, params, dirty, audio, hp)
    for m in (0, 2):
        assert same(ld[m], lc[m]) and same(gd[m], gc[m])
    assert not np.isfinite(ld[1]).any()
    ref_l, ref_g, _ = plain_run(D, rank, params[1], dirty[1], audio[1], hp)
    assert same(ld[1], ref_l) and same(gd[1], ref_g)

    v0, hyper = apply_args(D, rank, B, M)
    vd = v0.copy()
    vd[1, -1] = np.nan                                    # the last entry of member 1's Wy
    nv, nphi = v0.shape[1], 2 * rank * D
    npar = layout.size(layout.param_fields(D, with_A=True))
    hy = torch.from_numpy(hyper).cuda()

    def step(vars0, grad):
        be = HipScan(D)
        st = {k: torch.from_numpy(a.copy()).cuda() for k, a in (("vars", vars0), ("m", np.zeros_like(vars0)), ("v", np.zeros_like(vars0)))}
        st["params"] = torch.zeros((M, npar), dtype=torch.float32).cuda()
        st["phi"] = torch.zeros((M, nphi), dtype=torch.float32).cuda()
        st["losses"] = torch.zeros((M, 2), dtype=torch.float32).cuda()
        be.rho_bank_apply_step(st["vars"], st["m"], st["v"], torch.from_numpy(grad).cuda(), rank, B, np.sqrt(1 - 0.999), 1 - 0.9, 0.9, 0.999, 1e-8, hy,
                               True, st["params"], st["phi"], st["losses"])
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in st.items()}

    sc, sd = step(v0, gc), step(vd, gd)
    for m in (0, 2):
        for k in sc:
            assert same(sc[k][m], sd[k][m]), (m, k)
        assert not same(sc["vars"][m], v0[m])
    # member 1: what the plain step makes of those variables and that gradient
    be = HipScan(D)
    st = {k: torch.from_numpy(a.copy()).cuda() for k, a in (("vars", vd[1]), ("m", np.zeros_like(vd[1])), ("v", np.zeros_like(vd[1])))}
    par, ph, los = (torch.zeros(n, dtype=torch.float32).cuda() for n in (npar, nphi, 2))
    h = hyper[1]
    be.rho_apply_step(st["vars"], st["m"], st["v"], torch.from_numpy(ref_g).cuda(), rank, B, h[0] * np.sqrt(1 - 0.999) / (1 - 0.9), 0.9, 0.999, 1e-8,
                      h[1], h[2], h[3], h[4], True, par, ph, los)
    torch.cuda.synchronize()
    for k in ("vars", "m", "v"):
        assert same(sd[k][1], st[k]), k
    assert same(sd["params"][1], par) and same(sd["phi"][1], ph) and same(sd["losses"][1], los)


def raw_bank(D, rank, params, phi, audio, hp, ws_fill):
    """The whole step at the C ABI on caller-made buffers: set_state, forward, backward, apply_step, forward only.  Every buffer the
    library is handed sits between red zones; the workspace is exactly cmps_rho_bank_workspace_bytes."""
    lib = _capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    M, B, T = audio.shape
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        nv, ng, npar, nphi = layout.size(layout.var_fields(D, rank)), layout.grad_size(D, rank), params.shape[1], phi.shape[1]
        sizes = {"ws": lib.cmps_rho_bank_workspace_bytes(D, rank, M, B, T, TRAIN), "loss": 4 * M * B, "loss0": 4 * M * B, "grad": 4 * M * ng,
                 "params": 4 * M * npar, "phi": 4 * M * nphi, "losses": 8 * M, "scratch": lib.cmps_rho_bank_apply_step_scratch_bytes(D, rank, M),
                 "vars": 4 * M * nv, "m": 4 * M * nv, "v": 4 * M * nv, "params_in": 4 * M * npar, "phi_in": 4 * M * nphi, "audio": 4 * M * B * T,
                 "hyper": 8 * M * 5}
        assert sizes["ws"] == M * (lib.cmps_workspace_bytes(D, B, T, 0) + lib.cmps_rho_workspace_bytes(D, rank, B, T, TRAIN))
        bufs = {k: Guarded(n, dev, name=k) for k, n in sizes.items()}
        bufs["ws"].payload.fill_(ws_fill)
        v0, hyper = apply_args(D, rank, B, M)
        for k, a in (("vars", v0), ("params_in", params), ("phi_in", phi), ("audio", audio), ("hyper", hyper)):
            bufs[k].load(a)
        bufs["m"].payload.zero_()
        bufs["v"].payload.zero_()
        torch.cuda.synchronize()

        def ok(code):
            assert code == _capi.CMPS_OK, lib.cmps_last_error(h).decode()

        ok(lib.cmps_rho_bank_set_state_dev(h, M, bufs["params_in"].ptr, bufs["phi_in"].ptr, rank, hp.sigma, hp.delta_t, T, B, TRAIN, bufs["ws"].ptr,
                                           sizes["ws"], None))
        ok(lib.cmps_rho_bank_loss_fwd(h, bufs["audio"].ptr, M, B, T, bufs["loss"].ptr, 1, None))
        ok(lib.cmps_rho_bank_loss_bwd(h, bufs["audio"].ptr, M, B, T, bufs["grad"].ptr, None))
        ok(lib.cmps_rho_bank_apply_step(h, M, bufs["vars"].ptr, bufs["m"].ptr, bufs["v"].ptr, bufs["grad"].ptr, rank, float(B), np.sqrt(1 - 0.999),
                                        1 - 0.9, 0.9, 0.999, 1e-8, bufs["hyper"].ptr, 1, bufs["params"].ptr, bufs["phi"].ptr, bufs["losses"].ptr,
                                        bufs["scratch"].ptr, None))
        ok(lib.cmps_rho_bank_loss_fwd(h, bufs["audio"].ptr, M, B, T, bufs["loss0"].ptr, 0, None))
        torch.cuda.synchronize()
        for k, g in bufs.items():
            assert g.zones_intact() is None, (k, g.zones_intact())
        for k in ("loss", "loss0", "grad", "params", "phi", "losses"):
            assert not bool(bufs[k].untouched_mask().any()), f"{k}: an element was never written"
        for k, a in (("params_in", params), ("phi_in", phi), ("audio", audio)):
            assert same(bufs[k].numpy(), a.ravel()), f"{k}: an input was written"
        return {k: bufs[k].numpy() for k in ("loss", "loss0", "grad", "params", "phi", "losses", "vars", "m", "v")}
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_memory_contract_red_zones_and_dirty_workspace(shape):
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    dirty = raw_bank(D, rank, params, phi, audio, hp, ws_fill=0xFF)
    clean = raw_bank(D, rank, params, phi, audio, hp, ws_fill=0x00)
    for k in dirty:
        assert same(dirty[k], clean[k]), k
    for m in range(M):
        assert same(dirty["loss"].reshape(M, B)[m], plain[m][0]) and same(dirty["grad"].reshape(M, -1)[m], plain[m][1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=[IDS[0], IDS[4]])
def test_caller_stream_and_reused_tables(shape):
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        loss, grad, _ = bank_run(D, rank, params, phi, audio, hp)
    l2, g2, _ = bank_run(D, rank, params, phi, audio, hp, calls=2)            # the second set_state keeps the time tables
    for m in range(M):
        assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1])
        assert same(l2[m], plain[m][0]) and same(g2[m], plain[m][1])


def test_reused_tables_follow_a_changed_stride_and_member_count():
    """CMPS_WS_REUSE_TABLES on one handle and one workspace while B_max shrinks (every member's region moves: the stride is the size of
    one region) and while M changes (regions appear): the tables are rebuilt where they now lie -- the bits are the plain path's."""
    shape = SHAPES[0]
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    lib = _capi.load()
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        nbytes = lib.cmps_rho_bank_workspace_bytes(D, rank, M, B + 2, T, TRAIN)
        ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        p, f, a = torch.from_numpy(params).cuda(), torch.from_numpy(phi).cuda(), torch.from_numpy(audio).cuda()
        loss = torch.empty((M, B), dtype=torch.float32, device="cuda")
        grad = torch.empty((M, layout.grad_size(D, rank)), dtype=torch.float32, device="cuda")
        REUSE = TRAIN | _capi.CMPS_WS_REUSE_TABLES
        for Mk, B_max, flags in ((M - 1, B + 2, TRAIN), (M - 1, B, REUSE), (M, B, REUSE), (M, B, REUSE)):
            assert lib.cmps_rho_bank_set_state_dev(h, Mk, p.data_ptr(), f.data_ptr(), rank, hp.sigma, hp.delta_t, T, B_max, flags, ptr, nbytes,
                                                   None) == _capi.CMPS_OK, lib.cmps_last_error(h).decode()
            assert lib.cmps_rho_bank_loss_fwd(h, a.data_ptr(), Mk, B, T, loss.data_ptr(), 1, None) == _capi.CMPS_OK
            assert lib.cmps_rho_bank_loss_bwd(h, a.data_ptr(), Mk, B, T, grad.data_ptr(), None) == _capi.CMPS_OK
            torch.cuda.synchronize()
            for m in range(Mk):
                assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1]), (Mk, B_max, m)
    finally:
        lib.cmps_destroy(h)


def test_call_order_and_mode_errors_at_the_c_abi():
    """The call-order half of the contract, which needs a successful set_state and so a device: every refusal below comes back with its
    code and a message that starts with the entry's name, launches nothing, and leaves the handle usable -- every cross-refusal between
    the plain, the PsiCMPS-bank and the RhoCMPS-bank mode, then the bank's and the plain bits."""
    shape = SHAPES[0]
    D, rank, T, B, M = shape
    params, phi, audio, plain, hp = case(shape)
    lib = _capi.load()
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == OK
    try:
        nbytes = max(lib.cmps_rho_bank_workspace_bytes(D, rank, M, B, T, TRAIN), lib.cmps_bank_workspace_bytes(D, M, B, T, TRAIN))
        ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        rbytes = lib.cmps_rho_workspace_bytes(D, rank, B, T, TRAIN)
        rws = torch.full((rbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        rptr = (rws.data_ptr() + 255) // 256 * 256
        p, f, a = torch.from_numpy(params).cuda(), torch.from_numpy(phi).cuda(), torch.from_numpy(audio).cuda()
        a2 = a.clone()
        loss = torch.zeros((M, B), dtype=torch.float32, device="cuda")
        grad = torch.zeros((M, layout.grad_size(D, rank)), dtype=torch.float32, device="cuda")
        buf = torch.zeros(4096, dtype=torch.float32, device="cuda")          # stands in for every pointer of the refused calls
        x = buf.data_ptr()
        torch.cuda.synchronize()

        def refused(code, want, who):
            msg = lib.cmps_last_error(h).decode()
            assert code == want and msg.startswith(who + ":"), (who, code, msg)

        def ok(code):
            assert code == OK, lib.cmps_last_error(h).decode()

        def rho_bank_state():
            ok(lib.cmps_rho_bank_set_state_dev(h, M, p.data_ptr(), f.data_ptr(), rank, hp.sigma, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))

        def psi_bank_params():
            ok(lib.cmps_bank_set_params_dev(h, M, p.data_ptr(), hp.sigma, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))

        def plain_state():
            ok(lib.cmps_set_params_dev(h, p.data_ptr(), hp.sigma, hp.delta_t, T, B, 0, ptr, nbytes, None))
            ok(lib.cmps_rho_set_state(h, f.data_ptr(), f.data_ptr() + 4 * rank * D, rank, T, B, TRAIN, rptr, rbytes, None))

        def fwd(n_audio=M, B_=B, T_=T, save=1, aud=a):
            return lib.cmps_rho_bank_loss_fwd(h, aud.data_ptr(), n_audio, B_, T_, loss.data_ptr(), save, None)

        def bwd(n_audio=M, B_=B, T_=T, aud=a):
            return lib.cmps_rho_bank_loss_bwd(h, aud.data_ptr(), n_audio, B_, T_, grad.data_ptr(), None)

        # before any set_state, in plain mode and in the PsiCMPS bank's mode: the scans need cmps_rho_bank_set_state_dev
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        plain_state()
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        ok(lib.cmps_rho_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 1, None))
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")                     # a bank reverse pass after a plain forward
        psi_bank_params()
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        ok(lib.cmps_bank_loss_fwd(h, a.data_ptr(), M, B, T, loss.data_ptr(), 1, None))
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")                     # ... and after a PsiCMPS bank's forward

        # rho-bank mode: the arguments of the forward
        rho_bank_state()
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")                     # no forward yet (set_state dropped every record)
        for n_audio in (0, 2, M + 1, -1):
            refused(fwd(n_audio=n_audio), BAD, "cmps_rho_bank_loss_fwd")
        refused(fwd(T_=T - 1), BAD, "cmps_rho_bank_loss_fwd")
        refused(fwd(B_=B + 1), BAD, "cmps_rho_bank_loss_fwd")
        refused(fwd(B_=0), BAD, "cmps_rho_bank_loss_fwd")
        ok(fwd(save=0))
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")                     # the forward saved nothing
        ok(fwd())
        # ... the PsiCMPS bank's scan entries
        refused(lib.cmps_bank_loss_fwd(h, a.data_ptr(), M, B, T, loss.data_ptr(), 1, None), STATE, "cmps_bank_loss_fwd")
        refused(lib.cmps_bank_loss_bwd(h, a.data_ptr(), M, B, T, grad.data_ptr(), None), STATE, "cmps_bank_loss_bwd")
        codes, sticky = (ctypes.c_int * M)(), (ctypes.c_int * M)()
        refused(lib.cmps_bank_grad_status(h, codes, sticky, None), STATE, "cmps_bank_grad_status")
        # ... the plain entries of one model
        refused(lib.cmps_psi_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 0, None), STATE, "cmps_psi_loss_fwd")
        refused(lib.cmps_psi_loss_bwd(h, a.data_ptr(), B, T, grad.data_ptr(), None), STATE, "cmps_psi_loss_bwd")
        one = ctypes.c_int()
        refused(lib.cmps_psi_grad_status(h, ctypes.byref(one), None), STATE, "cmps_psi_grad_status")
        refused(lib.cmps_psi_states(h, B, T, x, None), STATE, "cmps_psi_states")
        refused(lib.cmps_psi_update_ancilla(h, x, x, 0.0, B, x, None), STATE, "cmps_psi_update_ancilla")
        refused(lib.cmps_psi_sample(h, x, 1, 8, x, None), STATE, "cmps_psi_sample")
        refused(lib.cmps_psi_sample_primed(h, x, 1, 4, x, 1, 8, x, None, None), STATE, "cmps_psi_sample_primed")
        refused(lib.cmps_psi_stream(h, None, x, 0, None, 1, 0, x, 8, 1, x, None, None), STATE, "cmps_psi_stream")
        refused(lib.cmps_psi_stream_score(h, None, x, 0, x, 1, 4, 1, x, x, None, None), STATE, "cmps_psi_stream_score")
        refused(lib.cmps_rho_set_state(h, x, x, rank, T, B, 0, rptr, rbytes, None), STATE, "cmps_rho_set_state")
        refused(lib.cmps_rho_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 0, None), STATE, "cmps_rho_loss_fwd")
        refused(lib.cmps_rho_loss_bwd(h, a.data_ptr(), B, T, grad.data_ptr(), None), STATE, "cmps_rho_loss_bwd")
        refused(lib.cmps_rho_update_ancilla(h, x, x, 0.0, B, x, None), STATE, "cmps_rho_update_ancilla")
        refused(lib.cmps_rho_sample(h, x, 1, 8, x, 0, None), STATE, "cmps_rho_sample")
        refused(lib.cmps_rho_sample_primed(h, x, 1, 4, x, 1, 8, x, None, 0, None), STATE, "cmps_rho_sample_primed")
        refused(lib.cmps_rho_stream(h, None, x, 0, None, 1, 0, x, 8, 1, x, None, 0, None), STATE, "cmps_rho_stream")
        refused(lib.cmps_rho_stream_score(h, None, x, 0, x, 1, 4, 1, x, x, None, 0, None), STATE, "cmps_rho_stream_score")
        refused(lib.cmps_rho_states(h, B, T - 1, x, None, None), STATE, "cmps_rho_states")
        refused(lib.cmps_legacy_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 0, None), STATE, "cmps_legacy_loss_fwd")
        # ... the reverse pass follows ITS forward: another n_audio, B, T or audio buffer is a call-order error
        refused(bwd(n_audio=1), STATE, "cmps_rho_bank_loss_bwd")
        refused(bwd(B_=B - 1), STATE, "cmps_rho_bank_loss_bwd")
        refused(bwd(T_=T - 1), STATE, "cmps_rho_bank_loss_bwd")
        refused(bwd(aud=a2), STATE, "cmps_rho_bank_loss_bwd")
        ok(fwd(n_audio=1))
        refused(bwd(n_audio=M), STATE, "cmps_rho_bank_loss_bwd")
        # ... and a changed option or variant, at both calls
        for option, value, back in ((_capi.CMPS_OPT_F16_SCALE_SHIFT, 1, 0), (_capi.CMPS_OPT_RHO_BWD, _capi.CMPS_RHO_BWD_GEMM, _capi.CMPS_RHO_BWD_VIRTUAL)):
            ok(lib.cmps_set_option(h, option, value))
            refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
            refused(bwd(n_audio=1), STATE, "cmps_rho_bank_loss_bwd")
            ok(lib.cmps_set_option(h, option, back))
        ok(lib.cmps_set_variant(h, _capi.CMPS_VARIANT_BLOCK))
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        refused(bwd(n_audio=1), STATE, "cmps_rho_bank_loss_bwd")
        ok(lib.cmps_set_variant(h, _capi.CMPS_VARIANT_AUTO))

        # legacy mode
        ok(lib.cmps_legacy_set_params(h, x, x, x, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")

        # none of this has left a trace: the bank's scans give the plain bits
        torch.cuda.synchronize()
        ws.fill_(0xFF)
        loss.zero_()
        grad.zero_()
        rho_bank_state()
        ok(fwd())
        ok(bwd())
        torch.cuda.synchronize()
        for m in range(M):
            assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1]), m
        # a plain set_params puts the handle back: the plain entries work again, the bank's do not
        plain_state()
        ok(lib.cmps_rho_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 1, None))
        ok(lib.cmps_rho_loss_bwd(h, a.data_ptr(), B, T, grad.data_ptr(), None))
        refused(bwd(), STATE, "cmps_rho_bank_loss_bwd")
        refused(fwd(), STATE, "cmps_rho_bank_loss_fwd")
        torch.cuda.synchronize()
        assert same(loss[0], plain[0][0]) and same(grad[0], plain[0][1])
    finally:
        lib.cmps_destroy(h)


def test_python_surface_step_member_sample_evaluate_save_restore(tmp_path):
    from audio_mps_amd.bank import BankTrainer, RhoBank
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    D, rank, B, T = 8, 4, 2, 40
    hp = hparams(D, rank, B)

    def fresh():
        return BankTrainer(RhoBank(hp, MEMBERS, backend=HipScan(D)))

    bt = fresh()
    be = bt.bank.backend
    M = len(bt)
    shared = make_audio(B, T, hp.delta_t, seed=1)
    out = bt.step(shared)
    assert out["model_loss"].shape == (M,) and out["total_loss"].shape == (M,) and np.isfinite(out["model_loss"]).all()
    dev = bt.step(np.stack([shared] * M), sync=False)
    assert tuple(dev["losses_dev"].shape) == (M, 2) and "model_loss" not in dev
    with pytest.raises(ValueError):
        bt.step(np.zeros((M + 1, B, T), np.float32))
    assert 0 <= bt.best() < M
    # models[m].variables read directly is current, and the two ways of feeding the same batch gave the same steps
    ref = fresh()
    ref.step(shared)
    ref.step(shared)
    for m in range(M):
        for k, v in ref.member(m).variables.items():
            assert same(bt.bank.models[m].variables[k], v), (m, k)
    # evaluation of every member on a resident 6-clip dataset = Trainer.evaluate of that member; a member samples
    ds = ResidentDataset(be.damped_sine(9, 0, 6, T, hp.delta_t), be)
    res = bt.evaluate(ds, minibatch_size=4, keep_losses=True)
    assert len(res) == M
    for m in range(M):
        model = bt.member(m)
        assert isinstance(model, RhoCMPS)
        x = model.sample(2, 16, seed=1)
        assert x.shape == (2, 16) and np.isfinite(x).all()
        one = Trainer(model, bt.bank.member_hparams[m], device_step=True).evaluate(ds, minibatch_size=4, keep_losses=True)
        assert res[m].scalars() == one.scalars() and same(res[m].losses, one.losses), m
    # save / restore continue bit for bit (the bank goes on after its members were used on the shared backend)
    d = str(tmp_path / "bank")
    bt.save(d)
    again = fresh()
    assert again.restore(d) and again.global_step == 2
    a, b = bt.step(shared), again.step(shared)
    assert same(a["model_loss"], b["model_loss"]) and same(a["total_loss"], b["total_loss"])
    for m in range(M):
        for k, v in bt.member(m).variables.items():
            assert same(again.member(m).variables[k], v), (m, k)
    # an assignment to a member's variables is not overwritten by the next step
    new_rx = (0.5 * bt.bank.models[1].variables["Rx"]).astype(np.float32)
    bt.bank.models[1].variables["Rx"] = new_rx
    bt.step(shared)
    assert not same(bt.bank.models[1].variables["Rx"], new_rx) and not same(bt.bank.models[1].variables["Rx"], again.member(1).variables["Rx"])


def test_train_main_with_a_rho_bank(tmp_path, capsys):
    from audio_mps_amd.bank import BankTrainer, RhoBank
    from audio_mps_amd.train import main
    argv = ["--dataset", "damped_sine", "--hparams", "bond_dim=4,minibatch_size=2,initial_rank=3", "--sample_duration", "32", "--max_steps", "2",
            "--logdir", str(tmp_path), "--bank", "2", "--mps_model", "rho_mps", "--seed", "1"]
    trainer = main(argv)
    assert isinstance(trainer, BankTrainer) and isinstance(trainer.bank, RhoBank) and trainer.native
    assert len(trainer) == 2 and trainer.global_step == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 2 and all("members 2 best" in ln and ln.endswith("nonfinite 0") for ln in lines)
    logdir = next(p for p, _, files in os.walk(tmp_path) if "bank.json" in files)
    assert sorted(f for f in os.listdir(logdir) if f.startswith("model.")) == ["model.0.ckpt.npz", "model.1.ckpt.npz"]
    again = main(argv)                                           # restores and continues
    assert again.global_step == 4
