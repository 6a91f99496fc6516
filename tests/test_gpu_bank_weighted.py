"""cmps_bank_loss_bwd_weighted on a real MI355X: the reverse pass of a PsiCMPS bank with a cotangent per clip and member.

Every family a bank may use, at the C ABI on a fresh handle per run, every reverse pass behind a forward of its own; `grad_dev` and the
padded `weight_dev` (rows ldw = B + 3 apart) sit between red zones (tests/_guard.py), and both n_audio values are run:
  1. weights of all 1.0 give cmps_bank_loss_bwd's grad_dev, bit for bit;
  2. weights of all 2.0 give exactly twice that, bit for bit (no sum of these draws is subnormal, which the test asserts);
  3. a clip of weight 0 may hold NaN audio, or be swapped for another clip, without changing one bit of grad_dev -- its last element
     included -- or a word of cmps_bank_grad_status;
  4. random signed weights against float64 AUTOGRAD of the restated forward (tests/_autograd_ref.py::psi_losses on the "f64t32" grid,
     ``torch.sum(w * per).backward()``).  The error of each tensor is normalised by max over its elements of sum_b |w_b| |g_b|, g_b the
     twin's per-clip gradients -- signed weights cancel in the result and must not shrink the yardstick -- and the bars are that file's:
     max(GRAD_BAR, OWN_FACTOR |oracle_f32 - twin|), the float32 oracle's per-clip gradients weighted by the same w (LOSS_BAR for the
     weighted loss sum, normalised by sum_b |w_b| max(|loss_b|, 1)).  That the float32 oracle itself stays inside GRAD_BAR on these draws
     is asserted on the CPU (test_the_float32_oracle_weighted_by_the_draws_stays_inside_the_bar), so the fixed bar decides.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _autograd_ref as AR

gpu = pytest.mark.gpu

AUTO, BLOCK = 0, 1                                     # CMPS_VARIANT_*
#        family     D   T   B   M  variant  reverse scan
CASES = [("wave16", 3, 34, 5, 3, AUTO, "k_bwd_wave16"),
         ("wave2w", 17, 66, 5, 2, AUTO, "k_bwd_wave2w"),
         ("block", 7, 40, 5, 3, BLOCK, "k_bwd_block"),
         ("groups", 3, 12, 37, 2, AUTO, "k_bwd_wave16")]         # B = 37: an RPART group holds two clips, the 19th group one, 13 none
IDS = [c[0] for c in CASES]
PAD = 3                                                # ldw = B + PAD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def models_of(case):
    from audio_mps_amd import HParams, PsiCMPS
    _, D, T, B, M, _, _ = case
    return [PsiCMPS(HParams(minibatch_size=B, bond_dim=D), seed=100 + m, backend=object()) for m in range(M)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params [M, NP], audio [M, B, T], hparams) of a case; audio[0] is also the shared batch of n_audio = 1."""
    from audio_mps_amd import layout
    from _util import make_audio
    _, D, T, B, M, _, _ = case
    rows = []
    for mo in models_of(case):
        p = mo.effective_params()
        rows.append(layout.pack(layout.param_fields(D, with_A=True),
                                {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A}))
    hp = models_of(case)[0].hparams
    audio = np.stack([make_audio(B, T, hp.delta_t, seed=7 + m) for m in range(M)])
    return np.stack(rows), audio, hp


def draw_weights(case, seed=5):
    """Signed weights [M, B] in +-[0.25, 2]: no clip is nearly switched off, so every clip's error counts."""
    _, D, T, B, M, _, _ = case
    rng = np.random.default_rng(seed + D + B)
    return (rng.uniform(0.25, 2.0, (M, B)) * rng.choice([-1.0, 1.0], (M, B))).astype(np.float32)


def run(case, audio, weights, events=False):
    """A fresh handle: cmps_bank_set_params_dev, cmps_bank_loss_fwd(save_for_bwd = 1) of ``audio`` ([B, T]: shared; [M, B, T]), then
    cmps_bank_loss_bwd (``weights`` None) or cmps_bank_loss_bwd_weighted.  Returns dict(grad [M, NG], loss [M, B], codes, sticky, kernels)."""
    from audio_mps_amd import _capi, layout
    from _guard import NAN_FILL, Guarded
    _, D, T, B, M, variant, _ = case
    params, _, hp = inputs(case)
    lib = _capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    n_audio = 1 if audio.ndim == 2 else M
    h = ctypes.c_void_p()
    assert lib.cmps_create(D, ctypes.byref(h)) == _capi.CMPS_OK
    try:
        def ok(code):
            assert code == _capi.CMPS_OK, lib.cmps_last_error(h).decode()
        ok(lib.cmps_set_variant(h, variant))
        if events:
            ok(lib.cmps_set_option(h, _capi.CMPS_OPT_KERNEL_EVENTS, 1))
        ng = layout.grad_size(D)
        n_ws = lib.cmps_bank_workspace_bytes(D, M, B, T, _capi.CMPS_WS_TRAIN)
        ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
        pin = torch.from_numpy(params).to(dev)
        aud = torch.from_numpy(np.ascontiguousarray(audio)).to(dev)
        loss = torch.empty((M, B), dtype=torch.float32, device=dev)
        g_grad = Guarded(4 * M * ng, dev, name="grad")
        ok(lib.cmps_bank_set_params_dev(h, M, pin.data_ptr(), hp.sigma, hp.delta_t, T, B, _capi.CMPS_WS_TRAIN, ws.data_ptr(), n_ws, None))
        ok(lib.cmps_bank_loss_fwd(h, aud.data_ptr(), n_audio, B, T, loss.data_ptr(), 1, None))
        if weights is None:
            ok(lib.cmps_bank_loss_bwd(h, aud.data_ptr(), n_audio, B, T, g_grad.ptr, None))
        else:
            ldw = B + PAD
            padded = np.full((M, ldw), np.uint32(NAN_FILL).view(np.float32), np.float32)
            padded[:, :B] = weights
            flat = padded.reshape(-1)[:(M - 1) * ldw + B].copy()                        # exactly the documented extent
            g_w = Guarded(flat.nbytes, dev, name="weights")
            g_w.load(flat)
            g_w.snapshot(flat)
            ok(lib.cmps_bank_loss_bwd_weighted(h, aud.data_ptr(), n_audio, B, T, g_w.ptr, ldw, g_grad.ptr, None))
        codes, sticky = (ctypes.c_int * M)(), (ctypes.c_int * M)()
        ok(lib.cmps_bank_grad_status(h, codes, sticky, None))                           # (waits for the stream)
        torch.cuda.synchronize()
        assert g_grad.zones_intact() is None, g_grad.zones_intact()
        assert not bool(g_grad.untouched_mask().any()), "grad_dev: an element was never written"
        if weights is not None:
            assert g_w.zones_intact() is None and g_w.equals_snapshot() is None
        kernels = set()
        if events:
            names, ms, cnt = ctypes.create_string_buffer(2048), (ctypes.c_float * 32)(), (ctypes.c_int * 32)()
            n = lib.cmps_kernel_times(h, names, 2048, ms, cnt, 32)
            assert n > 0, n
            kernels = set(names.value.decode().split("\n"))
        return {"grad": g_grad.numpy().reshape(M, ng), "loss": loss.cpu().numpy(), "codes": list(codes), "sticky": list(sticky),
                "kernels": kernels}
    finally:
        lib.cmps_destroy(h)


def audio_of(case, n_audio):
    _, audio, _ = inputs(case)
    return audio[0] if n_audio == 1 else audio


def _n_audio(case, which):
    return 1 if which == "shared" else case[4]


@gpu
@pytest.mark.parametrize("which", ["shared", "own"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unit_weights_are_the_plain_reverse_pass_and_doubled_weights_double_it(case, which):
    _, D, T, B, M, _, scan = case
    audio = audio_of(case, _n_audio(case, which))
    plain = run(case, audio, None)
    one = run(case, audio, np.ones((M, B), np.float32), events=True)
    assert np.array_equal(bits(one["grad"]), bits(plain["grad"])), "weights of 1.0 differ from cmps_bank_loss_bwd"
    assert np.array_equal(bits(one["loss"]), bits(plain["loss"])) and one["codes"] == plain["codes"] and one["sticky"] == plain["sticky"] == [0] * M
    assert {scan, "reduce + finalize (weighted)"} <= one["kernels"] and "reduce + finalize" not in one["kernels"], one["kernels"]
    g = plain["grad"].astype(np.float64)
    assert np.all(np.isfinite(g)) and np.all((g == 0) | (np.abs(g) > 2.0 ** -120)), "a subnormal sum: doubling would not be exact"
    two = run(case, audio, np.full((M, B), 2.0, np.float32))
    assert np.array_equal(bits(two["grad"]), bits(plain["grad"] * np.float32(2.0))), "weights of 2.0 are not twice the plain result"


@gpu
@pytest.mark.parametrize("which", ["shared", "own"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_clip_of_weight_zero_is_not_read(case, which):
    _, D, T, B, M, _, _ = case
    n_audio = _n_audio(case, which)
    audio = audio_of(case, n_audio).copy()
    w = draw_weights(case, seed=9)
    off = [(m, b) for m in range(M) for b in ((1, B - 1) if n_audio == 1 else (m % B, B - 1 - m))]       # shared: the same clips of every member
    for m, b in off:
        w[m, b] = 0.0 if (m + b) % 2 else -0.0                                          # either sign of zero
    clean = run(case, audio, w)
    assert clean["sticky"] == [0] * M and np.all(np.isfinite(clean["grad"]))
    nan_audio, swapped = audio.copy(), audio.copy()
    for m, b in off:
        if n_audio == 1:
            nan_audio[b, T // 2:] = np.nan
            swapped[b] = audio[(b + 2) % B] * np.float32(1.5)
        else:
            nan_audio[m, b, T // 2:] = np.nan
            swapped[m, b] = audio[m, (b + 2) % B] * np.float32(1.5)
    for what, other in (("NaN audio", nan_audio), ("another clip", swapped)):
        got = run(case, other, w)
        assert np.array_equal(bits(got["grad"]), bits(clean["grad"])), what
        assert got["codes"] == clean["codes"] and got["sticky"] == clean["sticky"], (what, got["codes"], got["sticky"])
    got = run(case, nan_audio, w)                                                       # ... and those clips' losses did go bad: nothing was masked
    assert all(not np.isfinite(got["loss"][m, b]) for m, b in off)
    # the same NaN clips with a weight: the sums and the status words see them
    w_on = np.where(w == 0, np.float32(1.0), w).astype(np.float32)
    bad = run(case, nan_audio, w_on)
    assert not np.all(np.isfinite(bad["grad"])) and any(bad["sticky"])


# ---------------------------------------------------------------------------------------------------
# random signed weights against float64 autograd
# ---------------------------------------------------------------------------------------------------
KEYS = AR.PSI_KEYS


def _twin_weighted(audio, p, w):
    """The twin's gradient of sum_b w_b loss_b, from backward(): dict of KEYS, per_clip [B], loss_sum."""
    R, psi0 = np.asarray(p.R, dtype=np.complex128), np.asarray(p.psi0, dtype=np.complex128)
    lv = {"R_re": AR._leaf(R.real), "R_im": AR._leaf(R.imag), "freqs": AR._leaf(p.freqs), "psi0_re": AR._leaf(psi0.real),
          "psi0_im": AR._leaf(psi0.imag), "A": AR._leaf(p.A)}
    per = AR.psi_losses(audio, lv["R_re"], lv["R_im"], lv["freqs"], lv["psi0_re"], lv["psi0_im"], lv["A"], p.delta_t, p.sigma, "f64t32")
    wt = torch.from_numpy(np.asarray(w, dtype=np.float64))
    torch.sum(wt * per).backward()
    g = {k: v.grad.numpy().copy() for k, v in lv.items()}
    return {"per_clip": per.detach().numpy().copy(), "Rbar": g["R_re"] + 1j * g["R_im"], "fbar": g["freqs"],
            "psi0bar": g["psi0_re"] + 1j * g["psi0_im"], "Abar": float(g["A"]), "loss_sum": float((wt * per.detach()).sum())}


@functools.lru_cache(maxsize=None)
def weighted_refs(case):
    """Per member (own audio, n_audio = M): the weighted twin, the yardsticks max sum_b |w_b| |g_b| per tensor, and the float32 oracle
    weighted by the same w.  Computed once, on the CPU."""
    from oracle import c_oracle as C
    from _util import c_oracle_run
    _, D, T, B, M, _, _ = case
    _, audio, _ = inputs(case)
    w = draw_weights(case)
    out = []
    for m, mo in enumerate(models_of(case)):
        p = mo.effective_params()
        twin = _twin_weighted(audio[m], p, w[m])
        yard = {k: 0.0 for k in KEYS}
        f32 = {k: 0.0 for k in KEYS}
        f32_loss = 0.0
        for b in range(B):
            one = AR.psi_twin(audio[m, b:b + 1], p.R, p.freqs, p.psi0, p.A, p.delta_t, p.sigma, "f64t32")
            r = c_oracle_run(mo, audio[m, b:b + 1], "f32")
            g32 = C.unpack_grad(r["grad"], D)
            for k in KEYS:
                yard[k] = yard[k] + abs(float(w[m, b])) * np.abs(np.asarray(one[k]))
                f32[k] = f32[k] + float(w[m, b]) * np.asarray(g32[k]).astype(np.complex128 if np.iscomplexobj(g32[k]) else np.float64)
            f32_loss += float(w[m, b]) * float(r["loss_per_clip"][0])
        yard = {k: float(np.max(v)) for k, v in yard.items()}
        yard["loss_sum"] = float(np.sum(np.abs(w[m]) * np.maximum(np.abs(twin["per_clip"]), 1.0)))
        own = {k: float(np.max(np.abs(f32[k] - twin[k]))) / yard[k] for k in KEYS}
        own["loss_sum"] = abs(f32_loss - twin["loss_sum"]) / yard["loss_sum"]
        out.append({"twin": twin, "yard": yard, "own": own})
    return w, out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_float32_oracle_weighted_by_the_draws_stays_inside_the_bar(case):
    """No GPU: the float32 restatement of the same weighted sums is well inside the fixed bars on these draws, so that GRAD_BAR / LOSS_BAR
    and not the elastic OWN_FACTOR term decide what the kernels are held to."""
    _, refs = weighted_refs(case)
    for m, r in enumerate(refs):
        for k in KEYS:
            assert r["own"][k] * AR.OWN_FACTOR <= AR.GRAD_BAR, (m, k, r["own"][k])
        assert r["own"]["loss_sum"] * AR.OWN_FACTOR <= AR.LOSS_BAR, (m, r["own"]["loss_sum"])
        assert all(v > 0 for v in r["yard"].values())


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_signed_weights_against_float64_autograd(case):
    from audio_mps_amd.scan import unpack_grad
    _, D, T, B, M, _, _ = case
    w, refs = weighted_refs(case)
    got = run(case, audio_of(case, M), w)
    assert got["codes"] == [0] * M and got["sticky"] == [0] * M
    bad = []
    for m, r in enumerate(refs):
        res = unpack_grad(got["grad"][m], D)
        for k in KEYS + ("loss_sum",):
            wide = np.complex128 if np.iscomplexobj(res[k]) else np.float64             # (a float32 scalar would round the twin to itself)
            err = float(np.max(np.abs(np.asarray(res[k], dtype=wide) - r["twin"][k]))) / r["yard"][k]
            bar = max(AR.LOSS_BAR if k == "loss_sum" else AR.GRAD_BAR, AR.OWN_FACTOR * r["own"][k])
            print(f"[{case[0]}] member {m} {k:8s} |hip - twin| {err:.2e}   |f32 - twin| {r['own'][k]:.2e}   bar {bar:.2e}")
            if not err <= bar:
                bad.append((m, k, err, bar))
    assert not bad, bad
