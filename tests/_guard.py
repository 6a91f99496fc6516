"""Guarded device buffers and a thin driver of the C ABI (include/cmps.h) for the memory-contract tests.

`Guarded` is ONE torch.uint8 allocation `front zone | payload | back zone`: the payload starts at a multiple of `align` and is exactly
`nbytes` long, each zone is max(64 KiB, nbytes) long, and the whole allocation -- payload included -- holds a 4-byte pattern before use.
A write past either end of the payload lands in a zone and is found by `zones_intact`; a read of something nobody wrote sees the pattern
(a quiet NaN with a payload no arithmetic produces, or zero) and shows in the outputs.  Everything stays inside the one allocation: no
guard pages, nothing at an allocation's edge -- a wrong write is a failed assertion, never a fault.

`Driver` owns one libcmps handle and calls the ABI through `_capi.load()` with every device pointer taken from a `Guarded`; after each
entry (following torch.cuda.synchronize()) it asserts the return code, every zone of every buffer and every `const` input's snapshot, and
`finish()` asserts that no element of a registered output keeps the NaN pattern.  The sequences below (psi / legacy / rho loss, samplers,
resumable samplers, optimiser steps) are shared by tests/test_gpu_memory_contract.py and tests/test_gpu_caller_stream.py; a driver built
with `queue=True` creates every buffer at once and makes the library calls later, on the stream it is given.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import torch

NAN_FILL = 0x7FC5A5A5        # a quiet NaN whose payload no arithmetic produces (an ordinary NaN is 0x7FC00000)
ZERO_FILL = 0x00000000
FILLS = (NAN_FILL, ZERO_FILL)
ZONE_MIN = 64 * 1024


def _pattern(fill: int, start: int, count: int, device="cpu") -> torch.Tensor:
    """`count` bytes of the little-endian 4-byte pattern, the first one being byte `start % 4` of it (uint8 tensor on `device`)."""
    four = torch.tensor(list(struct.pack("<I", fill)), dtype=torch.uint8, device=device)
    return four.repeat(count // 4 + 2)[start % 4: start % 4 + count]


class Guarded:
    def __init__(self, nbytes: int, device, align: int = 256, fill: int = NAN_FILL, name: str = ""):
        nbytes = int(nbytes)
        assert nbytes >= 0 and align >= 4 and align % 4 == 0
        self.nbytes, self.align, self.fill, self.name = nbytes, align, fill, name
        self.zone = max(ZONE_MIN, nbytes)
        self.raw = torch.empty(align + 2 * self.zone + nbytes, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        self.off = (base + self.zone + align - 1) // align * align - base        # payload offset in `raw`: a front zone fits below it
        assert self.off >= self.zone and self.off + nbytes + self.zone <= self.raw.numel()
        self._snap = None
        self._staged = None       # the host copy stage() prepared for commit()
        self._pat = _pattern(fill, -self.off % 4, self.raw.numel(), self.raw.device).clone()      # what an untouched allocation holds
        self.refill()

    # the pattern is phased on the payload's first byte, so that every aligned 4-byte element of the payload holds `fill`
    def _expected(self, lo: int, hi: int) -> torch.Tensor:
        return self._pat[lo:hi]

    def refill(self):
        """Pattern over the whole allocation, payload included (on the current stream)."""
        self.raw.copy_(self._pat)

    def refill_payload(self):
        self.payload.copy_(self._expected(self.off, self.off + self.nbytes))

    @property
    def payload(self) -> torch.Tensor:
        return self.raw[self.off:self.off + self.nbytes]

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + self.off

    def view(self, dtype, shape=(-1,)) -> torch.Tensor:
        """A typed view of the payload (torch dtype)."""
        return self.payload.view(dtype).reshape(shape)

    def numpy(self, dtype=np.float32, shape=(-1,)) -> np.ndarray:
        return self.payload.cpu().numpy().view(dtype).reshape(shape).copy()

    def stage(self, array):
        """The first half of load(): the host copy (pinned for a device buffer) of exactly nbytes."""
        a = np.ascontiguousarray(array)
        src = torch.from_numpy(a.view(np.uint8).reshape(-1).copy())
        assert src.numel() == self.nbytes, (self.name, src.numel(), self.nbytes)
        self._staged = src.pin_memory() if self.raw.is_cuda else src

    def commit(self):
        """The second half: the staged bytes into the payload, asynchronously on the current stream."""
        self.payload.copy_(self._staged, non_blocking=True)

    def load(self, array):
        """Copy a host array into the payload: exactly nbytes."""
        self.stage(array)
        self.commit()

    def zones_intact(self):
        """None when both zones (and the slack below the front one) still hold the pattern; else (front, back): the first altered byte of
        each side as an offset from the payload's first byte (front: negative) / from the first byte behind the payload, or None."""
        out = []
        for lo, hi, origin in ((0, self.off, self.off), (self.off + self.nbytes, self.raw.numel(), self.off + self.nbytes)):
            diff = self.raw[lo:hi] != self._expected(lo, hi)
            out.append(int(torch.nonzero(diff)[0]) + lo - origin if bool(diff.any()) else None)
        return None if out == [None, None] else tuple(out)

    def untouched_mask(self, dtype=torch.float32) -> torch.Tensor:
        """bool per payload element of `dtype`: it still holds the fill pattern bit for bit."""
        size = torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % size == 0
        same = self.payload == self._expected(self.off, self.off + self.nbytes)
        return same.reshape(-1, size).all(dim=1)

    def snapshot(self, data=None):
        """Remember the payload (or `data`, the host array a queued load will put there) for equals_snapshot."""
        if data is None:
            self._snap = self.payload.clone()
        else:
            self._snap = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()).to(self.raw.device)
        assert self._snap.numel() == self.nbytes

    def equals_snapshot(self):
        """None when the payload equals its snapshot, else the offset of the first differing byte."""
        assert self._snap is not None, "no snapshot"
        bad = torch.nonzero(self.payload != self._snap)
        return int(bad[0]) if bad.numel() else None


# ---------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------
class Driver:
    """One libcmps handle; every device pointer it hands to the library is a `Guarded`'s."""

    def __init__(self, D, fill=NAN_FILL, variant=0, options=(), device=None, queue=False):
        from audio_mps_amd import _capi
        self.capi, self.lib = _capi, _capi.load()
        self.D, self.fill = int(D), fill
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.h = ctypes.c_void_p()
        assert self.lib.cmps_create(self.D, ctypes.byref(self.h)) == _capi.CMPS_OK
        self.check(self.lib.cmps_set_variant(self.h, int(variant)), "cmps_set_variant")
        for opt, val in options:
            self.check(self.lib.cmps_set_option(self.h, int(opt), int(val)), "cmps_set_option")
        self.bufs = {}            # name -> Guarded
        self.const = set()        # names of snapshotted read-only inputs
        self.outputs = {}         # name -> torch dtype: documented outputs that must be fully written
        self.queue = [] if queue else None      # queue mode: (fn name, args) to be made later by run_queue()
        self.pending = []         # queue mode: buffers whose staged input flush_inputs() copies in
        self.stream = None        # hipStream_t as an int (None: the default stream)
        self.hints = {}           # queue mode: sizes the library only tells after a call that has not been made yet
        self.calls = []           # names of the entries made, in order

    def close(self):
        if self.h:
            self.lib.cmps_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, code, where):
        msg = self.lib.cmps_last_error(self.h)
        assert code == self.capi.CMPS_OK, f"{where}: code {code}: {msg.decode() if msg else '?'}"

    @property
    def variant(self):
        return int(self.lib.cmps_get_variant(self.h))

    # ---- buffers ----
    def new(self, name, nbytes, out=None) -> Guarded:
        """A pattern-filled buffer of exactly nbytes; out = a torch dtype registers it as a documented output."""
        assert name not in self.bufs, name
        g = Guarded(nbytes, self.device, fill=self.fill, name=name)
        self.bufs[name] = g
        if out is not None:
            self.outputs[name] = out
        return g

    def load(self, name, array, const=True) -> Guarded:
        """A buffer holding `array` (queue mode: the pattern, until flush_inputs() copies the array in); const: snapshotted and compared
        after every call."""
        a = np.ascontiguousarray(array)
        g = self.new(name, a.nbytes)
        g.stage(a)
        if self.queue is None:
            g.commit()
        else:
            self.pending.append(g)
        g.snapshot(a)
        if const:
            self.const.add(name)
        return g

    def flush_inputs(self):
        for g in self.pending:
            g.commit()
        self.pending = []

    # ---- calls ----
    def call(self, fn, *args):
        """lib.<fn>(handle, *args, stream) with every Guarded replaced by its payload address; then synchronise and verify."""
        if self.queue is not None:
            self.queue.append((fn, args))
            return
        self._call(fn, args)
        torch.cuda.synchronize(self.device)
        self.verify(fn)

    def _call(self, fn, args):
        raw = [a.ptr if isinstance(a, Guarded) else a for a in args]
        code = getattr(self.lib, fn)(self.h, *raw, ctypes.c_void_p(self.stream))
        self.calls.append(fn)
        self.check(code, fn)

    def run_queue(self):
        """Queue mode: make the queued calls on self.stream, without synchronising or reading anything back."""
        for fn, args in self.queue:
            self._call(fn, args)
        self.queue = []

    def verify(self, where=""):
        for name, g in self.bufs.items():
            assert g.zones_intact() is None, f"{where}: guard zone of '{name}' altered at (front, back) = {g.zones_intact()}"
        for name in self.const:
            assert self.bufs[name].equals_snapshot() is None, \
                f"{where}: read-only input '{name}' altered at byte {self.bufs[name].equals_snapshot()}"

    def finish(self):
        """After the last call: zones, inputs, and no element of a documented output keeps the NaN pattern."""
        torch.cuda.synchronize(self.device)
        self.verify("finish")
        if self.fill == NAN_FILL:
            for name, dtype in self.outputs.items():
                left = torch.nonzero(self.bufs[name].untouched_mask(dtype))
                assert left.numel() == 0, f"output '{name}': {left.numel()} element(s) never written, the first at index {int(left[0])}"

    def grad_status(self):
        """cmps_psi_grad_status (it waits for the stream itself): (code, sticky)."""
        sticky = ctypes.c_int(-1)
        code = int(self.lib.cmps_psi_grad_status(self.h, ctypes.byref(sticky), ctypes.c_void_p(self.stream)))
        self.calls.append("cmps_psi_grad_status")
        self.verify("cmps_psi_grad_status")
        return code, int(sticky.value)

    def result(self, names):
        """{name: raw bytes of the payload} of the named buffers: what bit-identity is asserted on."""
        return {k: self.bufs[k].numpy(np.uint8) for k in names}


def f32(drv, name, shape=(-1,)):
    return drv.bufs[name].numpy(np.float32, shape)


def same_bits(a: dict, b: dict, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
            f"{what}: '{k}' differs in {int(np.sum(a[k] != b[k]))} of {a[k].size} bytes, the first at {int(np.argmax(a[k] != b[k]))}"


# ---------------------------------------------------------------------------------------------------
# inputs that make the tables visible: sigma = 0.36, A = 66, audio x 0.09, Rx, Ry x 0.69 (x 0.5 above D = 32) -- the settings of
# test_qbar_sums_visible_at_large_sigma (tests/test_gpu_parity.py, tests/test_gpu_wide.py): Q = -(dt sigma^2 / 2) R^dagger R is far above
# float32 resolution, so a stale Q / Q^T table cannot hide
# ---------------------------------------------------------------------------------------------------
SIGMA, AMP_A, AUDIO_SCALE, R_SCALE = 0.36, 66.0, 0.09, 0.69


def _rs(D):
    return np.float32(R_SCALE * (0.5 if D > 32 else 1.0))


def contract_audio(B, T, seed=3):
    from _util import make_audio
    from audio_mps_amd import HParams
    return (make_audio(B, T, HParams().delta_t, seed) * np.float32(AUDIO_SCALE)).astype(np.float32)


def psi_model(D, B=3):
    from audio_mps_amd import HParams, PsiCMPS
    m = PsiCMPS(HParams(minibatch_size=B, bond_dim=D, sigma=SIGMA, A=AMP_A), seed=7, backend=False)
    m.variables["Rx"] *= _rs(D)
    m.variables["Ry"] *= _rs(D)
    return m


def rho_model(D, rank, B=3):
    from audio_mps_amd import HParams, RhoCMPS
    m = RhoCMPS(HParams(minibatch_size=B, bond_dim=D, sigma=SIGMA, A=AMP_A, initial_rank=rank), seed=7, backend=False)
    m.variables["Rx"] *= _rs(D)
    m.variables["Ry"] *= _rs(D)
    return m


def legacy_model(D, B=3):
    from audio_mps_amd import LegacyAudioMPS
    return LegacyAudioMPS(D, 1e-3, B, seed=7, backend=False)


def psi_param_array(m):
    from audio_mps_amd import layout
    p = m.effective_params()
    return layout.pack(layout.param_fields(m.bond_d), {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0)})


# ---------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------
def ws_bytes(drv, B_max, T, train):
    n = int(drv.lib.cmps_workspace_bytes(drv.D, B_max, T, 1 if train else 0))
    assert n > 0
    return n


def set_params(drv, m, B_max, T, train=True, reuse=False, ws="ws"):
    """cmps_set_params into the exact-size workspace `ws` (created on first use)."""
    from audio_mps_amd import layout
    p = m.effective_params()
    if "params" not in drv.bufs:
        drv.load("params", psi_param_array(m))
    n = ws_bytes(drv, B_max, T, train)
    if ws not in drv.bufs:
        drv.new(ws, n)
    assert drv.bufs[ws].nbytes >= n
    flags = (1 if train else 0) | (drv.capi.CMPS_WS_REUSE_TABLES if reuse else 0)
    drv.call("cmps_set_params", *layout.pointers(drv.bufs["params"].ptr, layout.param_fields(drv.D)), float(p.A), float(p.sigma),
             float(p.delta_t), int(T), int(B_max), flags, drv.bufs[ws], n)
    drv.T = T


def psi_scan(drv, audio, tag="", save=True, bwd=True, states=True):
    """cmps_psi_loss_fwd (+ _bwd, cmps_psi_states) of the clips `audio` [B, T]; returns the names of the result buffers."""
    B, T = audio.shape
    D = drv.D
    a = drv.load("audio" + tag, audio)
    loss = drv.new("loss" + tag, 4 * B, out=torch.float32)
    drv.call("cmps_psi_loss_fwd", a, B, T, loss, 1 if save else 0)
    names = ["loss" + tag]
    if bwd:
        grad = drv.new("grad" + tag, 4 * (2 * D * D + 3 * D + 2), out=torch.float32)
        drv.call("cmps_psi_loss_bwd", a, B, T, grad)
        names.append("grad" + tag)
    if states:
        st = drv.new("states" + tag, 4 * B * (T - 1) * D * 2, out=torch.float32)
        drv.call("cmps_psi_states", B, T, st)
        names.append("states" + tag)
    return names


def legacy_set_params(drv, m, B_max, T, train=True):
    from audio_mps_amd import layout
    D = drv.D
    fields = layout.legacy_param_fields(D)
    drv.load("params", layout.pack(fields, {"R": m.variables["R"], **layout.split("Q", m.Q)}))
    n = ws_bytes(drv, B_max, T, train)
    drv.new("ws", n)
    drv.call("cmps_legacy_set_params", *layout.pointers(drv.bufs["params"].ptr, fields), float(m.delta_t), int(T), int(B_max),
             1 if train else 0, drv.bufs["ws"], n)


def legacy_scan(drv, audio, tag="", save=True, bwd=True):
    B, T = audio.shape
    D = drv.D
    a = drv.load("audio" + tag, audio)
    loss = drv.new("loss" + tag, 4 * B, out=torch.float32)
    drv.call("cmps_legacy_loss_fwd", a, B, T, loss, 1 if save else 0)
    names = ["loss" + tag]
    if bwd:
        grad = drv.new("grad" + tag, 4 * (3 * D * D + 1), out=torch.float32)
        drv.call("cmps_legacy_loss_bwd", a, B, T, grad)
        names.append("grad" + tag)
    return names


def rho_ws_bytes(drv, rank, B_max, T, train):
    n = int(drv.lib.cmps_rho_workspace_bytes(drv.D, rank, B_max, T, 1 if train else 0))
    assert n > 0
    return n


def rho_set_state(drv, m, B_max, T, train=True, ws="rho_ws"):
    """cmps_rho_set_state of the model's columns into the exact-size rho workspace (created on first use)."""
    from audio_mps_amd import layout
    phi = m.columns()
    r = phi.shape[0]
    if "phi" not in drv.bufs:
        drv.load("phi", layout.pack(layout.phi_fields(drv.D, r), layout.split("phi", phi)))
    n = rho_ws_bytes(drv, r, B_max, T, train)
    if ws not in drv.bufs:
        drv.new(ws, n)
    assert drv.bufs[ws].nbytes >= n
    drv.call("cmps_rho_set_state", *layout.pointers(drv.bufs["phi"].ptr, layout.phi_fields(drv.D, r)), r, int(T), int(B_max),
             1 if train else 0, drv.bufs[ws], n)
    drv.rank = r


def rho_scan(drv, audio, tag="", save=True, bwd=True, states=True):
    B, T = audio.shape
    D, r = drv.D, drv.rank
    a = drv.load("audio" + tag, audio)
    loss = drv.new("loss" + tag, 4 * B, out=torch.float32)
    drv.call("cmps_rho_loss_fwd", a, B, T, loss, 1 if save else 0)
    names = ["loss" + tag]
    if bwd:
        grad = drv.new("grad" + tag, 4 * (2 * D * D + 3 * D + 2 + 2 * r * D), out=torch.float32)
        drv.call("cmps_rho_loss_bwd", a, B, T, grad)
        names.append("grad" + tag)
    if states:
        names += rho_states(drv, B, T - 1, tag)
    return names


def rho_states(drv, B, steps, tag=""):
    D = drv.D
    st = drv.new("rho_states" + tag, 4 * B * steps * D * D * 2, out=torch.float32)
    pu = drv.new("purity" + tag, 4 * B * steps, out=torch.float32)
    drv.call("cmps_rho_states", B, steps, st, pu)
    return ["rho_states" + tag, "purity" + tag]


def ancilla(drv, fn, x, signal, t, tag=""):
    """cmps_{psi,rho}_update_ancilla of complex states x [B, ...]."""
    inter = np.stack([x.real, x.imag], axis=-1).astype(np.float32)
    i = drv.load("anc_in" + tag, inter)
    s = drv.load("anc_signal" + tag, np.asarray(signal, dtype=np.float32))
    o = drv.new("anc_out" + tag, inter.nbytes, out=torch.float32)
    drv.call(fn, i, s, float(t), x.shape[0], o)
    return ["anc_out" + tag]


def sample(drv, fn, noise, prime=None, want_pred=True, flags=(), tag=""):
    """cmps_{psi,rho}_sample, or with `prime` [n_prime, prime_T] cmps_{psi,rho}_sample_primed; noise [length, n] (the reference's layout)."""
    length, n = noise.shape
    nz = drv.load("noise" + tag, np.ascontiguousarray(noise.T, dtype=np.float32))
    out = drv.new("out" + tag, 4 * n * length, out=torch.float32)
    names = ["out" + tag]
    if prime is None:
        drv.call(fn, nz, n, length, out, *flags)
        return names
    n_prime, prime_T = prime.shape
    pr = drv.load("prime" + tag, np.ascontiguousarray(prime, dtype=np.float32))
    pred = None
    if want_pred:
        pred = drv.new("pred" + tag, 4 * n * (prime_T - 1), out=torch.float32)
        names.append("pred" + tag)
    drv.call(fn, pr, n_prime, prime_T, nz, n, length, out, pred, *flags)
    return names


def stream_plan(drv, fn, bytes_fn, plan, clip, noise, n, flags=(), null_pred_at=2, states_steps=None):
    """The plan [(forced, sampled), ...] through cmps_{psi,rho}_stream with ONE state buffer of exactly *_stream_state_bytes(h, n) bytes
    (state_out == state_in from the second segment on, state_out == NULL on the last one) and pred_dev == NULL in segment `null_pred_at`.
    After every segment the record zones are checked with all the others; returns (result names, [(record bytes, untouched float mask)]
    per segment that wrote a record)."""
    nbytes = drv.hints.get("state_bytes") or int(getattr(drv.lib, bytes_fn)(drv.h, n))
    assert nbytes > 0 and nbytes % 16 == 0
    drv.hints["state_bytes"] = nbytes
    state = drv.new("state", nbytes)
    names, recs = [], []
    k0 = f0 = l0 = 0
    for idx, (f, s) in enumerate(plan):
        tag = f"_{idx}"
        last = idx == len(plan) - 1
        a = drv.load("seg_audio" + tag, np.ascontiguousarray(clip[:, f0:f0 + f + 1], dtype=np.float32)) if f else None
        nz = drv.load("seg_noise" + tag, np.ascontiguousarray(noise[l0:l0 + s].T, dtype=np.float32)) if s else None
        out = drv.new("seg_out" + tag, 4 * n * s, out=torch.float32)
        pred = None
        if idx != null_pred_at:
            pred = drv.new("seg_pred" + tag, 4 * n * f, out=torch.float32)      # (forced == 0: an empty payload between two zones)
            names.append("seg_pred" + tag)
        names.append("seg_out" + tag)
        drv.call(fn, state if idx else None, None if last else state, k0, a, clip.shape[0] if f else 1, f, nz, s, n,
                 out if s else None, pred, *flags)          # (pred at forced == 0: a valid address nothing may be written to)
        if drv.queue is None and not last:
            recs.append((state.numpy(np.uint8), state.untouched_mask(torch.float32).cpu().numpy()))
        if states_steps is not None and drv.queue is None:
            names += rho_states(drv, n, f + s, tag)
        k0, f0, l0 = k0 + f + s, f0 + f, l0 + s
    return names, recs


def var_array(m, rank=0):
    from audio_mps_amd import layout
    return layout.pack(layout.var_fields(m.bond_d, rank), {k: m.variables[k] for k in layout.var_order(rank)})


def apply_step(drv, m, grad_sums, rank=0, tag=""):
    """cmps_psi_apply_step / cmps_rho_apply_step (rank > 0) on the model's variables with Adam slots of a previous step; grad_sums None:
    the first step.  Every buffer guarded, the scratch of exactly *_scratch_bytes."""
    D = drv.D
    v0 = var_array(m, rank)
    rng = np.random.default_rng(11)
    vars_ = drv.load("vars" + tag, v0, const=False)
    am = drv.load("adam_m" + tag, (1e-3 * rng.standard_normal(v0.size)).astype(np.float32), const=False)
    av = drv.load("adam_v" + tag, (1e-6 * rng.random(v0.size)).astype(np.float32), const=False)
    gs = drv.load("grad_sums" + tag, grad_sums) if grad_sums is not None else None
    params = drv.new("params_out" + tag, 4 * (2 * D * D + 3 * D + 1), out=torch.float32)
    losses = drv.new("losses" + tag, 8, out=torch.float32 if grad_sums is not None else None)
    nscr = int(drv.lib.cmps_rho_apply_step_scratch_bytes(D, rank) if rank else drv.lib.cmps_apply_step_scratch_bytes(D))
    assert nscr > 0
    scratch = drv.new("scratch" + tag, nscr)
    hp = m.hparams
    common = (4.0, 1e-3, 0.9, 0.999, 1e-8, float(hp.h_reg), float(hp.r_reg), float(m._c_r), float(m._c_h), 1)
    names = ["vars" + tag, "adam_m" + tag, "adam_v" + tag, "params_out" + tag]
    if rank:
        phi = drv.new("phi_out" + tag, 4 * 2 * rank * D, out=torch.float32)
        drv.call("cmps_rho_apply_step", vars_, am, av, gs, rank, *common, params, phi, losses, scratch)
        names.append("phi_out" + tag)
    else:
        drv.call("cmps_psi_apply_step", vars_, am, av, gs, *common, params, losses, scratch)
    if grad_sums is not None:
        names.append("losses" + tag)
    return names
