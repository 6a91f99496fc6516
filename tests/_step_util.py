"""One optimiser step on a synthetic gradient buffer, three ways: the device kernel (cmps_psi_apply_step / cmps_rho_apply_step), the host
implementation (model.chain_rule + AdamOptimizer) and the float64 autograd reference (tests/_step_ref.py) -- with the inputs, the
comparisons and the bars that tests/test_step_host.py (CPU), tests/test_gpu_psi_step.py and tests/test_gpu_rho_step.py share.  Only
``device_step`` needs torch on a GPU.

Every step returns {"vars", "m", "v": {variable: array}, "losses": [mean loss, total]} (+ "grads" from host and reference, "params" and
"phi" from the device).  ``rank`` is the model's: 0 for PsiCMPS (HipScan.apply_step, layout.var_fields(D)), RhoCMPS's rank_rho_0 else."""
from __future__ import annotations

import math

import numpy as np

import _step_ref as R

B1, B2, EPS = 0.9, 0.999, 1e-8                       # AdamOptimizer's defaults
LR = 0.01
BATCH = 4

# ---- bars against the float64 reference (fractions of the reference tensor's max |.|), from the number formats:
GRAD_REF_BAR = 2.5e-7     # one float32 rounding of a double result (6e-8), the float32 roundings of the effective R / freqs inside the
#                           regulariser term, and the two roundings of m = fl(0.1f g) and m / 0.1f through which the device's g is read
SLOT_REF_BAR = 5e-7       # the gradient's rounding (twice in v), the float32 constants 0.9f / 0.1f / 0.999f / 0.001f, two roundings each
VAR_REF_BAR = 2.0 ** -23  # one float32 rounding of the variable and a step a hundred times smaller
LOSS_REF_BAR = 2e-7       # a double value rounded once to float32 (6e-8), the regulariser sums on float32-rounded R / freqs
# ---- bars against the host implementation, in ulp (the kernel's header promises the host's rounding points; a float32 gradient one
# ulp apart -- the double sums colsum / block_sum_d ordered or contracted differently from numpy's -- is the one admitted difference)
M_ULP, V_ULP, VAR_ULP, PSI0_ULP = 1, 2, 2, 4


def rank_of(m) -> int:
    return int(getattr(m, "rank_rho_0", 0))


def given_kw(D, given):
    """Constructor arguments for `given`: False (both scaled by rsqrt(reg)), True (R_in and freqs_in: c_r = c_h = 1), "R" (R_in only:
    c_r = 1, c_h != 1), "freqs" (freqs_in only)."""
    rng = np.random.default_rng(1)
    kw = {"R_in": (0.3 * (rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))).astype(np.complex64),
          "freqs_in": (100.0 * rng.standard_normal(D)).astype(np.float32)}
    keep = {False: (), True: ("R_in", "freqs_in"), "R": ("R_in",), "freqs": ("freqs_in",)}[given]
    return {k: kw[k] for k in keep}


def psi_model(D, given=False, seed=3, backend=None, psi=None):
    """PsiCMPS with LR; ``psi``: "zero" (psi_x = psi_y = 0 exactly) or a float (sum |p|^2 scaled to it, e.g. 1e-13: inside the floor of
    _normalize_psi on the float32 and on the double comparison alike)."""
    from audio_mps_amd import HParams, PsiCMPS
    hp = HParams(minibatch_size=BATCH, bond_dim=D, learning_rate=LR)
    m = PsiCMPS(hp, seed=seed, backend=backend, **given_kw(D, given))
    if psi == "zero":
        m.variables["psi_x"] = np.zeros(D, np.float32)
        m.variables["psi_y"] = np.zeros(D, np.float32)
    elif psi is not None:
        x, y = m.variables["psi_x"].astype(np.float64), m.variables["psi_y"].astype(np.float64)
        s = math.sqrt(float(psi) / float(np.sum(x * x + y * y)))
        m.variables["psi_x"], m.variables["psi_y"] = (s * x).astype(np.float32), (s * y).astype(np.float32)
    return m


def rho_model(D, rank, given=False, seed=3, backend=None, data=None, B=BATCH):
    """RhoCMPS with LR; above D = 32 Rx, Ry are halved, as the trainer tests do."""
    from audio_mps_amd import HParams, RhoCMPS
    hp = HParams(minibatch_size=B, bond_dim=D, initial_rank=rank, learning_rate=LR)
    m = RhoCMPS(hp, data_iterator=data, seed=seed, backend=backend, **given_kw(D, given))
    if D > 32:
        m.variables["Rx"] *= np.float32(0.5)
        m.variables["Ry"] *= np.float32(0.5)
    return m


def grad_buffer(m, batch, seed, loss_sum=None):
    """A synthetic cmps_psi_loss_bwd / cmps_rho_loss_bwd buffer: random cotangents x batch and a finite loss sum; for RhoCMPS NaN in the
    two psi_0 blocks nobody may read."""
    from audio_mps_amd import layout
    D, rank = m.bond_d, rank_of(m)
    rng = np.random.default_rng(seed)
    gs = (batch * rng.standard_normal(m.flat_size())).astype(np.float32)
    if rank:
        g = layout.unpack(layout.grad_fields(D, rank), gs)           # (views)
        g["psi0_re"][...] = np.nan
        g["psi0_im"][...] = np.nan
    gs[loss_index(D)] = np.float32(37.5 * batch if loss_sum is None else loss_sum)
    return gs


def loss_index(D):
    return 2 * D * D + 3 * D + 1


def field_slice(m, field):
    """Where `field` of layout.grad_fields sits in the gradient buffer."""
    from audio_mps_amd import layout
    fields = layout.grad_fields(m.bond_d, rank_of(m))
    i = [k for k, _ in fields].index(field)
    o = layout.offsets(fields)[i]
    return slice(o, o + math.prod(fields[i][1]))


def copy_vars(d):
    return {k: np.array(a, dtype=np.float32) for k, a in d.items()}


def zero_slots(m):
    z = {k: np.zeros_like(np.asarray(v, dtype=np.float32)) for k, v in m.variables.items()}
    return z, copy_vars(z)


def random_slots(m, seed):
    """Adam slots in the middle of a run: m ~ 0.1 N(0, 1), v ~ 0.01 U(0, 1)."""
    rng = np.random.default_rng(seed)
    m0 = {k: (0.1 * rng.standard_normal(np.shape(v))).astype(np.float32) for k, v in m.variables.items()}
    v0 = {k: (0.01 * rng.uniform(0.0, 1.0, np.shape(v))).astype(np.float32) for k, v in m.variables.items()}
    return m0, v0


def slots_for(m, mode, seed=77):
    """mode "zero" -> (zero slots, t = 1); "random" -> (random_slots, t = 7)."""
    return (*zero_slots(m), 1) if mode == "zero" else (*random_slots(m, seed), 7)


def lr_t(t, lr=LR):
    return lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


# ---- the three implementations ----------------------------------------------------------------------------------------------
def device_step(m, gs, batch, t=1, m0=None, v0=None, with_reg=True, c_r=None, c_h=None, losses_init=float("nan")):
    """One cmps_psi_apply_step (rank 0) / cmps_rho_apply_step on copies of the model's variables and of the slots (None: zeros); every
    output buffer starts as NaN (losses: losses_init).  gs None: no gradients (only the outputs are written).  The model is not touched."""
    import torch
    from audio_mps_amd import layout
    be, D, rank = m._get_backend(), m.bond_d, rank_of(m)
    fields = layout.var_fields(D, rank)
    dev = be.device
    zeros = zero_slots(m)[0]
    vars_, am, av = (torch.from_numpy(layout.pack(fields, x if x is not None else zeros)).to(dev) for x in (m.variables, m0, v0))
    pf = layout.param_fields(D, with_A=True)
    params = torch.full((layout.size(pf),), float("nan"), dtype=torch.float32, device=dev)
    losses = torch.full((2,), losses_init, dtype=torch.float32, device=dev)
    g = torch.from_numpy(gs).to(dev) if gs is not None else None
    c_r = float(m._c_r) if c_r is None else float(c_r)
    c_h = float(m._c_h) if c_h is None else float(c_h)
    phi = None
    if rank:
        phi = torch.full((2 * rank * D,), float("nan"), dtype=torch.float32, device=dev)
        be.rho_apply_step(vars_, am, av, g, rank, batch, lr_t(t), B1, B2, EPS, m.h_reg, m.r_reg, c_r, c_h, with_reg, params, phi, losses)
    else:
        be.apply_step(vars_, am, av, g, batch, lr_t(t), B1, B2, EPS, m.h_reg, m.r_reg, c_r, c_h, with_reg, params, losses)
    torch.cuda.synchronize()
    un = lambda x: {k: np.array(a) for k, a in layout.unpack(fields, x.cpu().numpy()).items()}
    out = {"vars": un(vars_), "m": un(am), "v": un(av), "losses": losses.cpu().numpy(),
           "params": layout.unpack(pf, params.cpu().numpy())}
    if rank:
        out["phi"] = layout.join(layout.unpack(layout.phi_fields(D, rank), phi.cpu().numpy()), "phi")
    return out


def host_step(m, gs, batch, t=1, m0=None, v0=None, with_reg=True):
    """model.chain_rule + AdamOptimizer.apply_gradients on copies; losses = [float32(loss_sum / batch), chain_rule's total]."""
    from audio_mps_amd.train import AdamOptimizer
    z = zero_slots(m)[0]
    total, grads = m.chain_rule(gs, batch, with_reg=with_reg)
    opt = AdamOptimizer(LR, B1, B2, EPS)
    opt.t, opt.m, opt.v = t - 1, copy_vars(m0 if m0 is not None else z), copy_vars(v0 if v0 is not None else z)
    variables = copy_vars(m.variables)
    opt.apply_gradients(variables, grads)
    mean = np.float32(np.float64(gs[loss_index(m.bond_d)]) / batch)
    return {"vars": variables, "m": opt.m, "v": opt.v, "grads": grads, "losses": np.array([mean, total], dtype=np.float32)}


def reference_step(m, gs, batch, t=1, m0=None, v0=None, with_reg=True, c_r=None, c_h=None):
    """_step_ref.total_and_grads + adam64 (on the reference gradient rounded to float32 and cast up), all float64."""
    z = zero_slots(m)[0]
    m0, v0 = (m0 if m0 is not None else z), (v0 if v0 is not None else z)
    c_r = float(m._c_r) if c_r is None else float(c_r)
    c_h = float(m._c_h) if c_h is None else float(c_h)
    total, grads = R.total_and_grads(m.variables, gs, batch, m.h_reg, m.r_reg, c_r, c_h, rank_of(m), with_reg)
    out = {"vars": {}, "m": {}, "v": {}, "grads": grads,
           "losses": np.array([np.float64(gs[loss_index(m.bond_d)]) / batch, total], dtype=np.float64)}
    for k in grads:
        g32 = grads[k].astype(np.float32).astype(np.float64)
        out["vars"][k], out["m"][k], out["v"][k] = R.adam64(m.variables[k], m0[k], v0[k], g32, LR, B1, B2, EPS, t)
    return out


# ---- the comparisons ---------------------------------------------------------------------------------------------------------
def _frac(got, want):
    """max |got - want| as a fraction of max |want| (0 / 0 = 0: a tensor that is exactly zero must be met exactly)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, top = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    return 0.0 if err == 0.0 else (err / top if top > 0.0 else np.inf)


def check_against_reference(label, got, ref, from_zero_slots, names=None):
    """The bars of the float64 reference on one step's result; prints the worst distance per tensor (fraction of the tensor's max)
    before it asserts.  ``from_zero_slots``: also read the float32 gradient back as m / float32(0.1) and compare it."""
    fails = []
    for k in (names if names is not None else sorted(ref["grads"])):
        rows = [("var", _frac(got["vars"][k], ref["vars"][k]), VAR_REF_BAR), ("m", _frac(got["m"][k], ref["m"][k]), SLOT_REF_BAR),
                ("v", _frac(got["v"][k], ref["v"][k]), SLOT_REF_BAR)]
        if from_zero_slots:
            g32 = np.asarray(got["m"][k], dtype=np.float32) / np.float32(0.1)
            rows.insert(0, ("grad", _frac(g32, ref["grads"][k]), GRAD_REF_BAR))
        print(f"{label} vs float64 reference, {k}: " + ", ".join(f"{w} {e:.2e} (bar {b:.1e})" for w, e, b in rows))
        fails += [(k, w, e, b) for w, e, b in rows if not e <= b]
    for i, what in ((0, "mean loss"), (1, "total")):
        e = abs(float(got["losses"][i]) - float(ref["losses"][i])) / abs(float(ref["losses"][i]))
        print(f"{label} vs float64 reference, {what}: {e:.2e} (bar {LOSS_REF_BAR:.1e})")
        if not e <= LOSS_REF_BAR:
            fails.append((what, "loss", e, LOSS_REF_BAR))
    assert not fails, (label, fails)


def check_against_host(label, dev, host, names=None):
    """The ulp bars of the device step against the host step; prints the worst ulp distance per tensor before it asserts."""
    fails = []
    for k in (names if names is not None else sorted(host["vars"])):
        rows = [(w, int(np.max(R.ulp_distance(dev[key][k], host[key][k]))), bar)
                for w, key, bar in (("var", "vars", VAR_ULP), ("m", "m", M_ULP), ("v", "v", V_ULP))]
        print(f"{label} vs host, {k}: " + ", ".join(f"{w} {e} ulp (bar {b})" for w, e, b in rows))
        fails += [(k, w, e, b) for w, e, b in rows if e > b]
    assert not fails, (label, fails)


def check_params(label, model_with_vars, params):
    """params_out against the accessors of a model that holds the same (updated) variables: R, freqs, A bit-identical (both sides
    compute fl(c x) - fl(c d) in float32), psi_0 (PsiCMPS) within PSI0_ULP (hypotf and the order of the sum may differ); RhoCMPS: e_0."""
    from audio_mps_amd import layout
    mv = model_with_vars
    want = mv.R
    assert np.asarray(params["R_re"], np.float32).tobytes() == np.ascontiguousarray(want.real, np.float32).tobytes(), (label, "R_re")
    assert np.asarray(params["R_im"], np.float32).tobytes() == np.ascontiguousarray(want.imag, np.float32).tobytes(), (label, "R_im")
    assert np.asarray(params["freqs"], np.float32).tobytes() == np.ascontiguousarray(mv.freqs, np.float32).tobytes(), (label, "freqs")
    assert np.float32(params["A"]).tobytes() == np.float32(mv.A).tobytes(), (label, "A")
    if rank_of(mv):
        e0 = np.zeros(mv.bond_d, np.float32)
        e0[0] = 1
        assert np.array_equal(params["psi0_re"], e0) and np.array_equal(params["psi0_im"], np.zeros(mv.bond_d, np.float32))
        return
    p0 = mv.psi_0
    worst = max(int(np.max(R.ulp_distance(params["psi0_re"], p0.real))), int(np.max(R.ulp_distance(params["psi0_im"], p0.imag))))
    print(f"{label} params_out psi_0 vs model.psi_0: {worst} ulp (bar {PSI0_ULP})")
    assert worst <= PSI0_ULP, (label, "psi_0", worst)


def with_variables(m, variables):
    """A model like `m` (same class, hyper-parameters, scalings) holding `variables`; `m` itself is not touched."""
    import copy
    m2 = copy.copy(m)
    m2._device_owner = None
    m2._variables = dict(copy_vars(variables))
    return m2


# ---- the cases the CPU and the GPU tests share (the CPU run shows that every GPU case's inputs leave the HOST inside the bars) --------
MODES = ("zero", "random")                           # slots_for
PSI_SHAPES = (1, 5, 32, 33, 128)                     # D^2 = 1 | 25 | 1024: exactly one pass of the 1024 threads | 1089: ragged | sixteen passes
# (D, given, with_reg, psi): the branches of k_apply_step, at D = 5, and at D = 33 where the branch touches the D^2 loops
PSI_BRANCHES = tuple((D, g, True, None) for g in ("R", "freqs", True) for D in (5, 33)) + \
    ((5, False, False, None), (33, False, False, None), (5, True, False, None), (5, False, True, "zero"), (5, False, True, 1e-13))
RHO_SHAPES = ((1, 1, False), (5, 3, False), (12, 12, True), (33, 40, False), (128, 128, False))


def psi_case(D, given=False, with_reg=True, psi=None, mode="zero", backend=None):
    """(model, gradient buffer, keyword arguments of the three *_step functions) of one PsiCMPS case."""
    m = psi_model(D, given, backend=backend, psi=psi)
    m0, v0, t = slots_for(m, mode)
    return m, grad_buffer(m, BATCH, seed=10 * D), dict(t=t, m0=m0, v0=v0, with_reg=with_reg)


def rho_case(D, rank, given=False, mode="zero", backend=None):
    m = rho_model(D, rank, given, backend=backend)
    m0, v0, t = slots_for(m, mode)
    return m, grad_buffer(m, BATCH, seed=10 * D + rank), dict(t=t, m0=m0, v0=v0, with_reg=True)
