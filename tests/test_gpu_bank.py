"""The model bank on the GPU (cmps_bank_*, audio_mps_amd/bank.py): member m of a bank gives, BIT FOR BIT, what a plain handle gives for
model m alone -- the kernels are the plain ones with a member grid dimension, every member working in its own workspace.

Every comparison is np.array_equal on the raw float32 bits against a fresh plain handle per member.  That bar rests on the plain path
being reproducible, which test_plain_path_is_reproducible checks first for every family used (forward + backward twice on one handle).

Shapes: the smallest at which member indexing, chunk edges and padding can go wrong -- D below and at the family's width, T off the 64-
and 32-step chunk sizes, B odd and even, M > 2, the block kernels below and above D = 32.
"""
import ctypes

import numpy as np
import pytest
import torch

from audio_mps_amd import HParams, PsiCMPS, _capi, layout

from _guard import Guarded
from _util import make_audio

pytestmark = pytest.mark.gpu

AUTO, BLOCK = _capi.CMPS_VARIANT_AUTO, _capi.CMPS_VARIANT_BLOCK
#         family    D   T    B  M  variant
SHAPES = [("wave16", 3, 70, 3, 3, AUTO),
          ("wave16", 16, 130, 2, 5, AUTO),
          ("wave2", 17, 100, 3, 4, AUTO),
          ("wave2", 32, 130, 2, 3, AUTO),
          ("block", 5, 70, 3, 3, BLOCK),
          ("block", 40, 50, 2, 2, BLOCK)]
IDS = [f"{s[0]}-D{s[1]}" for s in SHAPES]


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def hparams(D, B, **kw):
    return HParams(minibatch_size=B, bond_dim=D, **kw)


def member_params(D, B, seed):
    """The effective parameters of PsiCMPS(seed) as the buffer cmps_set_params_dev reads: R_re | R_im | freqs | psi0_re | psi0_im | A."""
    p = PsiCMPS(hparams(D, B), seed=seed, backend=object()).effective_params()
    return layout.pack(layout.param_fields(D, with_A=True), {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})


_CASES = {}


def case(shape):
    """(params [M, NP], audio [M, B, T], plain results per member) of a shape, computed once: every member on a FRESH plain handle."""
    if shape not in _CASES:
        _, D, T, B, M, variant = shape
        hp = hparams(D, B)
        params = np.stack([member_params(D, B, 100 + m) for m in range(M)])
        audio = np.stack([make_audio(B, T, hp.delta_t, seed=7 + m) for m in range(M)])
        plain = [plain_run(D, variant, params[m], audio[m], hp) for m in range(M)]
        _CASES[shape] = (params, audio, plain, hp)
    return _CASES[shape]


def plain_run(D, variant, params, audio, hp, be=None):
    from audio_mps_amd.scan import HipScan
    be = HipScan(D, variant=variant) if be is None else be
    B, T = audio.shape
    p = torch.from_numpy(params).cuda()                   # (held until the scans have run: they read A from it)
    be.set_params_dev(p, hp.sigma, hp.delta_t, B, T, train=True)
    loss = be.forward(torch.from_numpy(audio).cuda(), save_for_bwd=True).clone()
    grad = be.backward().clone()
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy()


def bank_run(D, variant, params, audio, hp, be=None, calls=1):
    """Bank forward + backward; audio [B, T] (shared) or [M, B, T].  calls = 2: set_params twice (the second with CMPS_WS_REUSE_TABLES)."""
    from audio_mps_amd.scan import HipScan
    be = HipScan(D, variant=variant) if be is None else be
    B, T = audio.shape[-2:]
    p = torch.from_numpy(np.ascontiguousarray(params)).cuda()
    for _ in range(calls):
        be.bank_set_params_dev(p, hp.sigma, hp.delta_t, B, T, train=True)
    loss = be.bank_forward(torch.from_numpy(np.ascontiguousarray(audio)).cuda(), save_for_bwd=True)
    grad = be.bank_backward()
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.cpu().numpy(), be


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plain_path_is_reproducible(shape):
    """What the bit-for-bit bar rests on: the plain forward + backward twice on ONE handle give the same bits."""
    from audio_mps_amd.scan import HipScan
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    be = HipScan(D, variant=variant)
    a = plain_run(D, variant, params[0], audio[0], hp, be)
    b = plain_run(D, variant, params[0], audio[0], hp, be)
    assert same(a[0], b[0]) and same(a[1], b[1]), f"{shape[0]}: the plain path is not reproducible"
    assert same(a[0], plain[0][0]) and same(a[1], plain[0][1]), f"{shape[0]}: a second handle gives other bits"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_own_and_shared_audio(shape):
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    loss, grad, _ = bank_run(D, variant, params, audio, hp)
    assert loss.shape == (M, B) and grad.shape == (M, layout.grad_size(D))
    for m in range(M):
        assert same(loss[m], plain[m][0]), (m, loss[m], plain[m][0])
        assert same(grad[m], plain[m][1]), m
    # one batch shared by every member (n_audio = 1) = M copies of it
    shared = audio[1]
    l1, g1, _ = bank_run(D, variant, params, shared, hp)
    lM, gM, _ = bank_run(D, variant, params, np.stack([shared] * M), hp)
    assert same(l1, lM) and same(g1, gM)
    ref = plain_run(D, variant, params[1], shared, hp)
    assert same(l1[1], ref[0]) and same(g1[1], ref[1])
    assert not same(l1[0], l1[1])                       # (the members do differ)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_one_member_equals_the_plain_entries(shape):
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    loss, grad, _ = bank_run(D, variant, params[:1], audio[:1], hp)
    assert same(loss[0], plain[0][0]) and same(grad[0], plain[0][1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_permuted_bank_gives_permuted_members(shape):
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    perm = [2, 0, 1]
    la, ga, _ = bank_run(D, variant, params[:3], audio[:3], hp)
    lb, gb, _ = bank_run(D, variant, params[perm], audio[perm], hp)
    assert same(lb, la[perm]) and same(gb, ga[perm])


MEMBERS = [{"seed": 3, "learning_rate": 1e-3, "h_reg": 2e-7, "r_reg": 0.1},
           {"seed": 4, "learning_rate": 3e-3, "h_reg": 4e-7, "r_reg": 1.0},
           {"seed": 5, "learning_rate": 2e-4, "h_reg": 9e-8, "r_reg": 0.03}]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_three_optimiser_steps_equal_plain_device_trainers(shape):
    """vars, adam_m, adam_v, params and losses after every step against M plain Trainer(device_step=True) runs on fresh handles; the
    members' learning_rate, h_reg and r_reg all differ."""
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    _, D, T, B, _, variant = shape
    hp = hparams(D, B)
    bank = PsiBank(hp, MEMBERS, backend=HipScan(D, variant=variant))
    bt = BankTrainer(bank)
    assert bt.native
    plain = [Trainer(PsiCMPS(h, seed=s, backend=HipScan(D, variant=variant)), h, device_step=True)
             for h, s in zip(bank.member_hparams, bank.seeds)]
    M = len(MEMBERS)
    for step in range(3):
        audio = np.stack([make_audio(B, T, hp.delta_t, seed=50 + 10 * step + m) for m in range(M)])
        out = bt.step(audio, sync=True)
        for m, tr in enumerate(plain):
            ref = tr.step(audio[m], sync=True)
            for name in ("vars", "m", "v", "params", "losses"):
                assert same(bt._dev[name][m], tr._dev[name]), (step, m, name)
            assert np.float32(ref["model_loss"]) == out["model_loss"][m] and np.float32(ref["total_loss"]) == out["total_loss"][m]
    # the host copies after the sync are the plain trainers'
    for m, tr in enumerate(plain):
        mine = bt.member(m)
        for k, v in tr.model.variables.items():
            assert same(mine.variables[k], v), (m, k)
        assert bt.trainers[m].opt.t == tr.opt.t == 3


def test_a_nan_member_does_not_disturb_its_neighbours():
    """Member 1's R holds a NaN: members 0 and 2 keep the bits of the clean bank (losses, gradients, the next variables),
    cmps_bank_grad_status reports per member, and member 1 itself comes out exactly as the plain path leaves that model."""
    from audio_mps_amd.scan import HipScan
    shape = SHAPES[0]
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    dirty = params.copy()
    dirty[1, 1] = np.nan                                  # R_re[0][1]
    lc, gc, bec = bank_run(D, variant, params, audio, hp)
    ld, gd, bed = bank_run(D, variant, dirty, audio, hp)
    for m in (0, 2):
        assert same(ld[m], lc[m]) and same(gd[m], gc[m])
    assert not np.isfinite(ld[1]).any()
    codes, sticky = bed.bank_grad_status()
    assert codes == [_capi.CMPS_OK] * M                   # (loss and gradient both non-finite propagates, as in the plain entry)
    assert sticky[0] == 0 and sticky[2] == 0 and sticky[1] == 3
    assert bec.bank_grad_status() == ([_capi.CMPS_OK] * M, [0] * M)
    assert bed.bank_grad_status()[1] == [0] * M           # the sticky words restart
    ref_l, ref_g = plain_run(D, variant, dirty[1], audio[1], hp)
    assert same(ld[1], ref_l) and same(gd[1], ref_g)

    # the optimiser step on both banks' gradients
    nv = layout.size(layout.var_fields(D))
    models = [PsiCMPS(hparams(D, B), seed=100 + m, backend=object()) for m in range(M)]
    v0 = np.stack([layout.pack(layout.var_fields(D), mo.variables) for mo in models])
    hyper = torch.tensor([[1e-3 * (m + 1), mo.h_reg, mo.r_reg, float(mo._c_r), float(mo._c_h)] for m, mo in enumerate(models)], dtype=torch.float64).cuda()

    def step(be, grad):
        st = {k: torch.from_numpy(a.copy()).cuda() for k, a in (("vars", v0), ("m", np.zeros_like(v0)), ("v", np.zeros_like(v0)))}
        st["params"] = torch.zeros((M, nv), dtype=torch.float32).cuda()
        st["losses"] = torch.zeros((M, 2), dtype=torch.float32).cuda()
        be.bank_apply_step(st["vars"], st["m"], st["v"], torch.from_numpy(grad).cuda(), B, np.sqrt(1 - 0.999), 1 - 0.9, 0.9, 0.999, 1e-8, hyper, True,
                           st["params"], st["losses"])
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in st.items()}

    sc, sd = step(bec, gc), step(bed, gd)
    for m in (0, 2):
        for k in sc:
            assert same(sc[k][m], sd[k][m]), (m, k)
        assert not same(sc["vars"][m], v0[m])
    # member 1: what the plain step makes of that gradient
    be = HipScan(D, variant=variant)
    st = {k: torch.from_numpy(a.copy()).cuda() for k, a in (("vars", v0[1]), ("m", np.zeros_like(v0[1])), ("v", np.zeros_like(v0[1])))}
    par, los = torch.zeros(nv, dtype=torch.float32).cuda(), torch.zeros(2, dtype=torch.float32).cuda()
    h = hyper.cpu().numpy()[1]
    be.apply_step(st["vars"], st["m"], st["v"], torch.from_numpy(ref_g).cuda(), B, h[0] * np.sqrt(1 - 0.999) / (1 - 0.9), 0.9, 0.999, 1e-8,
                  h[1], h[2], h[3], h[4], True, par, los)
    torch.cuda.synchronize()
    for k in ("vars", "m", "v"):
        assert same(sd[k][1], st[k]), k
    assert same(sd["params"][1], par) and same(sd["losses"][1], los)


def raw_bank(D, variant, params, audio, hp, ws_fill, guarded):
    """The whole step at the C ABI on caller-made buffers: set_params, forward, backward, apply_step.  guarded: every buffer the library
    writes sits between red zones.  Returns the outputs and the Guarded buffers."""
    lib = _capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    M, B, T = audio.shape
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        assert lib.cmps_set_variant(h, variant) == _capi.CMPS_OK
        nv, ng = layout.size(layout.var_fields(D)), layout.grad_size(D)
        sizes = {"ws": lib.cmps_bank_workspace_bytes(D, M, B, T, _capi.CMPS_WS_TRAIN), "loss": 4 * M * B, "grad": 4 * M * ng, "params": 4 * M * nv,
                 "losses": 8 * M, "scratch": lib.cmps_bank_apply_step_scratch_bytes(D, M), "vars": 4 * M * nv, "m": 4 * M * nv, "v": 4 * M * nv}
        assert sizes["ws"] == M * lib.cmps_workspace_bytes(D, B, T, _capi.CMPS_WS_TRAIN)
        bufs = {k: Guarded(n, dev, name=k) for k, n in sizes.items()}
        bufs["ws"].payload.fill_(ws_fill)
        models = [PsiCMPS(hparams(D, B), seed=100 + m, backend=object()) for m in range(M)]
        bufs["vars"].load(np.stack([layout.pack(layout.var_fields(D), mo.variables) for mo in models]))
        bufs["m"].payload.zero_()
        bufs["v"].payload.zero_()
        pin = torch.from_numpy(params).to(dev)
        aud = torch.from_numpy(audio).to(dev)
        hyper = torch.tensor([[1e-3, mo.h_reg, mo.r_reg, float(mo._c_r), float(mo._c_h)] for mo in models], dtype=torch.float64).to(dev)
        torch.cuda.synchronize()

        def ok(code):
            assert code == _capi.CMPS_OK, lib.cmps_last_error(h).decode()

        ok(lib.cmps_bank_set_params_dev(h, M, pin.data_ptr(), hp.sigma, hp.delta_t, T, B, _capi.CMPS_WS_TRAIN, bufs["ws"].ptr, sizes["ws"], None))
        ok(lib.cmps_bank_loss_fwd(h, aud.data_ptr(), M, B, T, bufs["loss"].ptr, 1, None))
        ok(lib.cmps_bank_loss_bwd(h, aud.data_ptr(), M, B, T, bufs["grad"].ptr, None))
        ok(lib.cmps_bank_apply_step(h, M, bufs["vars"].ptr, bufs["m"].ptr, bufs["v"].ptr, bufs["grad"].ptr, float(B), np.sqrt(1 - 0.999), 1 - 0.9,
                                    0.9, 0.999, 1e-8, hyper.data_ptr(), 1, bufs["params"].ptr, bufs["losses"].ptr, bufs["scratch"].ptr, None))
        torch.cuda.synchronize()
        out = {k: bufs[k].numpy() for k in ("loss", "grad", "params", "losses", "vars", "m", "v")}
        if guarded:
            for k, g in bufs.items():
                assert g.zones_intact() is None, (k, g.zones_intact())
            for k in ("loss", "grad", "params", "losses"):
                assert not bool(bufs[k].untouched_mask().any()), f"{k}: an element was never written"
        return out
    finally:
        lib.cmps_destroy(h)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_memory_contract_red_zones_and_dirty_workspace(shape):
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    dirty = raw_bank(D, variant, params, audio, hp, ws_fill=0xFF, guarded=True)
    clean = raw_bank(D, variant, params, audio, hp, ws_fill=0x00, guarded=True)
    for k in dirty:
        assert same(dirty[k], clean[k]), k
    for m in range(M):
        assert same(dirty["loss"].reshape(M, B)[m], plain[m][0]) and same(dirty["grad"].reshape(M, -1)[m], plain[m][1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_caller_stream_and_reused_tables(shape):
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        loss, grad, _ = bank_run(D, variant, params, audio, hp)
    l2, g2, _ = bank_run(D, variant, params, audio, hp, calls=2)            # the second set_params keeps the time tables
    for m in range(M):
        assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1])
        assert same(l2[m], plain[m][0]) and same(g2[m], plain[m][1])


def test_reused_tables_follow_a_changed_member_stride():
    """CMPS_WS_REUSE_TABLES on one handle and one workspace while B_max shrinks: every member's workspace moves (the stride is the plain
    workspace's size), so its tables are rebuilt where they now lie -- the bits are those of the plain path."""
    shape = SHAPES[0]
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    lib = _capi.load()
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        nbytes = lib.cmps_bank_workspace_bytes(D, M, B + 2, T, _capi.CMPS_WS_TRAIN)
        ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        p, a = torch.from_numpy(params).cuda(), torch.from_numpy(audio).cuda()
        loss = torch.empty((M, B), dtype=torch.float32, device="cuda")
        grad = torch.empty((M, layout.grad_size(D)), dtype=torch.float32, device="cuda")
        for B_max, flags in ((B + 2, _capi.CMPS_WS_TRAIN), (B, _capi.CMPS_WS_TRAIN | _capi.CMPS_WS_REUSE_TABLES)):
            assert lib.cmps_bank_set_params_dev(h, M, p.data_ptr(), hp.sigma, hp.delta_t, T, B_max, flags, ptr, nbytes, None) == _capi.CMPS_OK
            assert lib.cmps_bank_loss_fwd(h, a.data_ptr(), M, B, T, loss.data_ptr(), 1, None) == _capi.CMPS_OK
            assert lib.cmps_bank_loss_bwd(h, a.data_ptr(), M, B, T, grad.data_ptr(), None) == _capi.CMPS_OK
            torch.cuda.synchronize()
            for m in range(M):
                assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1]), (B_max, m)
    finally:
        lib.cmps_destroy(h)


def test_python_surface_step_member_sample_evaluate():
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.device_data import ResidentDataset
    from audio_mps_amd.scan import HipScan
    from audio_mps_amd.train import Trainer
    D, B, T = 8, 2, 40
    hp = hparams(D, B)
    be = HipScan(D)
    bt = BankTrainer(PsiBank(hp, MEMBERS, backend=be))
    M = len(bt)
    shared = make_audio(B, T, hp.delta_t, seed=1)
    out = bt.step(shared)
    assert out["model_loss"].shape == (M,) and out["total_loss"].shape == (M,) and np.isfinite(out["model_loss"]).all()
    dev = bt.step(np.stack([shared] * M), sync=False)
    assert tuple(dev["losses_dev"].shape) == (M, 2) and "model_loss" not in dev
    with pytest.raises(ValueError):
        bt.step(np.zeros((M + 1, B, T), np.float32))
    assert 0 <= bt.best() < M
    # evaluation of every member on a resident 6-clip dataset = Trainer.evaluate of that member
    ds = ResidentDataset(be.damped_sine(9, 0, 6, T, hp.delta_t), be)
    res = bt.evaluate(ds, minibatch_size=4, keep_losses=True)
    assert len(res) == M
    for m in range(M):
        model = bt.member(m)
        x = model.sample(2, 16, seed=1)
        assert x.shape == (2, 16) and np.isfinite(x).all()
        ref = Trainer(model, bt.bank.member_hparams[m], device_step=True).evaluate(ds, minibatch_size=4, keep_losses=True)
        assert res[m].scalars() == ref.scalars() and same(res[m].losses, ref.losses), m
    # the bank goes on after its members were used on the shared backend
    assert np.isfinite(bt.step(shared)["model_loss"]).all()


def test_call_order_and_mode_errors_at_the_c_abi():
    """The call-order half of the contract, which needs a successful set_params and so a device: every refusal below comes back with its
    code and a message that starts with the entry's name, launches nothing, and leaves the handle usable -- the bank forward + backward
    at the end of the sequence gives the plain bits.  The workspace starts as 0xFF bytes, so the members' status words read zero only
    if cmps_bank_set_params_dev cleared every one of them."""
    shape = SHAPES[0]
    _, D, T, B, M, variant = shape
    params, audio, plain, hp = case(shape)
    lib = _capi.load()
    OK, BAD, STATE = _capi.CMPS_OK, _capi.CMPS_ERR_BAD_ARG, _capi.CMPS_ERR_STATE
    TRAIN = _capi.CMPS_WS_TRAIN
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == OK
    try:
        nbytes = lib.cmps_bank_workspace_bytes(D, M, B, T, TRAIN)
        ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        ptr = (ws.data_ptr() + 255) // 256 * 256
        p, a = torch.from_numpy(params).cuda(), torch.from_numpy(audio).cuda()
        a2 = a.clone()
        loss = torch.zeros((M, B), dtype=torch.float32, device="cuda")
        grad = torch.zeros((M, layout.grad_size(D)), dtype=torch.float32, device="cuda")
        buf = torch.zeros(4096, dtype=torch.float32, device="cuda")          # stands in for every pointer of the refused plain calls
        x = buf.data_ptr()
        torch.cuda.synchronize()

        def refused(code, want, who):
            msg = lib.cmps_last_error(h).decode()
            assert code == want and msg.startswith(who + ":"), (who, code, msg)

        def ok(code):
            assert code == OK, lib.cmps_last_error(h).decode()

        def bank_params():
            ok(lib.cmps_bank_set_params_dev(h, M, p.data_ptr(), hp.sigma, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))

        def plain_params():
            ok(lib.cmps_set_params_dev(h, p.data_ptr(), hp.sigma, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))

        def bank_fwd(n_audio=M, B_=B, T_=T, save=1, aud=a):
            return lib.cmps_bank_loss_fwd(h, aud.data_ptr(), n_audio, B_, T_, loss.data_ptr(), save, None)

        def bank_bwd(n_audio=M, B_=B, T_=T, aud=a):
            return lib.cmps_bank_loss_bwd(h, aud.data_ptr(), n_audio, B_, T_, grad.data_ptr(), None)

        # before any set_params, and in plain mode: the bank scans need cmps_bank_set_params_dev
        refused(bank_fwd(), STATE, "cmps_bank_loss_fwd")
        plain_params()
        refused(bank_fwd(), STATE, "cmps_bank_loss_fwd")
        ok(lib.cmps_psi_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 1, None))
        refused(bank_bwd(), STATE, "cmps_bank_loss_bwd")                    # a bank reverse pass after a plain forward
        codes, sticky = (ctypes.c_int * M)(), (ctypes.c_int * M)()
        refused(lib.cmps_bank_grad_status(h, codes, sticky, None), STATE, "cmps_bank_grad_status")

        # bank mode: the arguments of the forward
        bank_params()
        refused(bank_bwd(), STATE, "cmps_bank_loss_bwd")                    # no forward yet (set_params dropped the plain one's record)
        for n_audio in (0, 2, M + 1, -1):
            refused(bank_fwd(n_audio=n_audio), BAD, "cmps_bank_loss_fwd")
        refused(bank_fwd(T_=T - 1), BAD, "cmps_bank_loss_fwd")
        refused(bank_fwd(B_=B + 1), BAD, "cmps_bank_loss_fwd")
        refused(bank_fwd(B_=0), BAD, "cmps_bank_loss_fwd")
        # ... the plain entries of one model in bank mode
        refused(lib.cmps_psi_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 1, None), STATE, "cmps_psi_loss_fwd")
        ok(bank_fwd(save=0))
        refused(bank_bwd(), STATE, "cmps_bank_loss_bwd")                    # the forward saved nothing
        ok(bank_fwd())
        refused(lib.cmps_psi_loss_bwd(h, a.data_ptr(), B, T, grad.data_ptr(), None), STATE, "cmps_psi_loss_bwd")   # plain after a bank forward
        one = ctypes.c_int()
        refused(lib.cmps_psi_grad_status(h, ctypes.byref(one), None), STATE, "cmps_psi_grad_status")
        refused(lib.cmps_psi_states(h, B, T, x, None), STATE, "cmps_psi_states")
        refused(lib.cmps_psi_update_ancilla(h, x, x, 0.0, B, x, None), STATE, "cmps_psi_update_ancilla")
        refused(lib.cmps_psi_sample(h, x, 1, 8, x, None), STATE, "cmps_psi_sample")
        refused(lib.cmps_psi_sample_primed(h, x, 1, 4, x, 1, 8, x, None, None), STATE, "cmps_psi_sample_primed")
        refused(lib.cmps_psi_stream(h, None, x, 0, None, 1, 0, x, 8, 1, x, None, None), STATE, "cmps_psi_stream")
        refused(lib.cmps_psi_stream_score(h, None, x, 0, x, 1, 4, 1, x, x, None, None), STATE, "cmps_psi_stream_score")
        refused(lib.cmps_rho_set_state(h, x, x, 1, T, B, 0, ptr, nbytes, None), STATE, "cmps_rho_set_state")
        refused(lib.cmps_rho_update_ancilla(h, x, x, 0.0, B, x, None), STATE, "cmps_rho_update_ancilla")
        # ... the reverse pass follows ITS forward: another n_audio, B, T or audio buffer is a call-order error
        refused(bank_bwd(n_audio=1), STATE, "cmps_bank_loss_bwd")
        refused(bank_bwd(B_=B - 1), STATE, "cmps_bank_loss_bwd")
        refused(bank_bwd(T_=T - 1), STATE, "cmps_bank_loss_bwd")
        refused(bank_bwd(aud=a2), STATE, "cmps_bank_loss_bwd")
        ok(bank_fwd(n_audio=1))
        refused(bank_bwd(n_audio=M), STATE, "cmps_bank_loss_bwd")
        # ... and a changed option
        ok(lib.cmps_set_option(h, _capi.CMPS_OPT_F16_SCALE_SHIFT, 1))
        refused(bank_fwd(), STATE, "cmps_bank_loss_fwd")
        refused(bank_bwd(n_audio=1), STATE, "cmps_bank_loss_bwd")
        ok(lib.cmps_set_option(h, _capi.CMPS_OPT_F16_SCALE_SHIFT, 0))

        # legacy mode
        ok(lib.cmps_legacy_set_params(h, x, x, x, hp.delta_t, T, B, TRAIN, ptr, nbytes, None))
        refused(bank_fwd(), STATE, "cmps_bank_loss_fwd")
        refused(bank_bwd(), STATE, "cmps_bank_loss_bwd")
        refused(lib.cmps_bank_grad_status(h, codes, sticky, None), STATE, "cmps_bank_grad_status")

        # none of this has left a trace: the bank's scans give the plain bits, and every member's status words were cleared
        torch.cuda.synchronize()
        ws.fill_(0xFF)
        loss.zero_()
        grad.zero_()
        bank_params()
        ok(bank_fwd())
        ok(bank_bwd())
        ok(lib.cmps_bank_grad_status(h, codes, sticky, None))
        assert list(codes) == [OK] * M and list(sticky) == [0] * M
        for m in range(M):
            assert same(loss[m], plain[m][0]) and same(grad[m], plain[m][1]), m
        # a plain set_params puts the handle back: the plain entries work again, the bank's do not
        plain_params()
        ok(lib.cmps_psi_loss_fwd(h, a.data_ptr(), B, T, loss.data_ptr(), 1, None))
        ok(lib.cmps_psi_loss_bwd(h, a.data_ptr(), B, T, grad.data_ptr(), None))
        refused(bank_bwd(), STATE, "cmps_bank_loss_bwd")
        torch.cuda.synchronize()
        assert same(loss[0], plain[0][0]) and same(grad[0], plain[0][1])
    finally:
        lib.cmps_destroy(h)


def test_the_bank_owns_its_members_device_state():
    """bank.models[m].variables read directly is current after a step, and an assignment to it is not overwritten by the next step: the
    bank is its members' device owner, as a Trainer(device_step=True) is its model's."""
    from audio_mps_amd.bank import BankTrainer, PsiBank
    from audio_mps_amd.scan import HipScan
    D, B, T = 3, 2, 40
    hp = hparams(D, B)
    audio = make_audio(B, T, hp.delta_t, seed=2)

    def fresh():
        bt = BankTrainer(PsiBank(hp, MEMBERS, backend=HipScan(D)))
        assert bt.native
        return bt

    bt, ref = fresh(), fresh()
    before = [{k: v.copy() for k, v in mo.variables.items()} for mo in bt.bank.models]
    bt.step(audio, sync=False)
    ref.step(audio, sync=False)
    for m, mo in enumerate(bt.bank.models):
        assert not same(mo.variables["Rx"], before[m]["Rx"]), m                  # (read directly, not through member(m))
        assert same(mo.variables["Rx"], ref.member(m).variables["Rx"]), m
    # an assignment drops the device copy of every member (after bringing it back): the next step starts from the host values
    new_rx = (0.5 * bt.bank.models[1].variables["Rx"]).astype(np.float32)
    bt.bank.models[1].variables["Rx"] = new_rx
    ref.member(1)
    ref.trainers[1].model._variables["Rx"] = new_rx.copy()                       # the same change made the long way round:
    ref._dev = None                                                               # host values in, device copy rebuilt
    a, b = bt.step(audio), ref.step(audio)
    assert same(a["model_loss"], b["model_loss"]) and same(a["total_loss"], b["total_loss"])
    for m in range(len(bt)):
        for k, v in ref.member(m).variables.items():
            assert same(bt.bank.models[m].variables[k], v), (m, k)
    assert not same(bt.bank.models[1].variables["Rx"], new_rx)                   # (member 1 did train on from the assigned value)
