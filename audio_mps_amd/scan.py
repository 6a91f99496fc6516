"""Host driver of the HIP scan: owns a libcmps handle and a device workspace (a torch uint8 tensor used
purely as an allocation), and exposes the two operations the model needs.

PyTorch appears here only as plumbing: device memory, the current HIP stream, host<->device copies.
All arithmetic of the hot path happens in libcmps.so (audio_mps_amd/csrc/*.hip).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _capi, layout
from .layout import EffectiveParams, grad_size, unpack_grad  # noqa: F401  (their historical home: tests and scripts import them from here)


def _to_interleaved(z: np.ndarray, device) -> torch.Tensor:
    """Complex host array [...] -> float32 device tensor [..., 2] (re, im): the ABI's layout of states and matrices."""
    inter = np.stack([z.real, z.imag], axis=-1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(inter)).to(device)


def _from_interleaved(t: torch.Tensor) -> np.ndarray:
    o = t.cpu().numpy()
    return (o[..., 0] + 1j * o[..., 1]).astype(np.complex64)


class NoisePlan(NamedTuple):
    """Noise to be drawn on the device instead of an array of it: what a sampler entry takes as ``noise`` next to ``length`` and ``n``.
    Path b, sampled step j gets std * z(seed, b, first_step + j) of include/cmps.h (cmps_noise_fill); ``first_step`` is the table row of
    the first sampled step: 0 for a plain sample, prime_T - 1 behind a prime, the stream's position in a segment."""
    seed: int
    first_step: int
    std: float


def _is_tensor(t, device, dtype, shape, rows: bool = False) -> bool:
    """The one argument check of the backend: ``t`` is a tensor of ``dtype`` on ``device`` (None: on any CUDA device) of the rank
    ``shape`` (an int) or the shape ``shape`` (a tuple, None for any extent), and contiguous -- or, with ``rows``, a matrix whose rows
    are contiguous (a row stride of its own is allowed)."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and (t.is_cuda if device is None else t.device == device)):
        return False
    if isinstance(shape, int):
        shape = (None,) * shape
    if t.dim() != len(shape) or any(want is not None and want != have for want, have in zip(shape, t.shape)):
        return False
    if rows:
        return t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])
    return t.is_contiguous()


def _read_record(record: torch.Tensor, dtype: np.dtype, head: Optional[str] = None):
    """The one device -> host copy of a record: (its scalar fields -- those of the field ``head``, if given -- as Python numbers, the
    numpy record)."""
    rec = record.cpu().numpy().view(dtype)[0]
    scalars = rec if head is None else rec[head]
    return {k: (float(scalars[k]) if scalars.dtype[k].kind == "f" else int(scalars[k])) for k in scalars.dtype.names}, rec


def _ptr(t: Optional[torch.Tensor]):
    """The address of a device tensor as an entry takes it: NULL for None and for a tensor without elements."""
    return t.data_ptr() if t is not None and t.numel() else None


BANK_SETTER = {"bank": "bank_set_params_dev", "rho_bank": "rho_bank_set_state_dev"}      # kind of a bank -> the method that configures it


@dataclass
class _Bank:
    """The bank a HipScan holds (``kind`` None: none).  Every set_params* replaces it, so what a mode kept alive goes with the mode."""
    kind: Optional[str] = None                # a key of BANK_SETTER
    M: int = 0
    rank: int = 0                             # columns of every member's rho_0 ("rho_bank"; else 0)
    saved: Optional[tuple] = None             # the last forward's (audio, loss, n_audio): the reverse pass reads both tensors
    params: Optional[object] = None           # the rows bank_set_params / rho_bank_set_state uploaded: the scans read A from them
    scratch: Optional[torch.Tensor] = None    # of the apply-step entries; sized by (D, rank, M) alone, so it is handed on from mode to mode


class HipScan:
    """The MI355X backend: per-clip loss and parameter-gradient sums for a batch resident on the GPU."""

    name = "hip"

    def __init__(self, D: int, device: Optional[torch.device] = None, variant: int = _capi.CMPS_VARIANT_AUTO,
                 rank1: Optional[int] = None):
        self._h = None                # (first: __del__ runs even when a line below raises)
        self._lib = _capi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("HipScan needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.D = int(D)
        h = ctypes.c_void_p()
        code = self._lib.cmps_create(self.D, ctypes.byref(h))
        if code != _capi.CMPS_OK:
            raise _capi.CmpsError(code, f"cmps_create(D={D}) failed")
        self._h = h
        _capi.check(self._h, self._lib.cmps_set_variant(self._h, int(variant)))
        if rank1 is not None:
            self.set_rank1(rank1)
        if os.environ.get("CMPS_BWD_WAVES"):            # diagnostic (like CMPS_LIB): A/B of the one- and two-wave reverse scans without code changes
            _capi.check(self._h, self._lib.cmps_set_option(self._h, _capi.CMPS_OPT_BWD_WAVES, int(os.environ["CMPS_BWD_WAVES"])))
        self._mode = "psi"            # which arithmetic the handle was last configured for: set_params* -> "psi", legacy_set_params -> "legacy",
        self._bank = _Bank()          # the bank setters -> their kind, with the bank's record (`_configured`)
        self._ws = {"main": None, "rho": None}        # caller-owned workspaces of the C ABI, keyed by the shape they were sized for
        self._ws_key = {"main": None, "rho": None}
        self._ws_fresh = False        # the main workspace was (re)allocated since the last set_params*: its cached tables are gone
        self._n_params = layout.size(layout.param_fields(self.D))
        self._param_buf = torch.empty(self._n_params, dtype=torch.float32, device=self.device)
        self._param_host = torch.empty(self._n_params, dtype=torch.float32).pin_memory()
        self._param_evt = None
        self._legacy_buf = self._phi_buf = None       # the last legacy_set_params / rho_set_state upload (kept alive for the stream)
        self._opt_scratch = self._rho_opt_scratch = None
        self._B = self._T = self._rho_rank = 0
        self._audio = None
        self._loss = self._rho_loss = None            # per-clip losses of the main workspace's forwards (psi, legacy) and of rho_forward: each
        #                                               reverse pass reads the loss buffer of its own forward (the handle's two records)
        self._grad = torch.empty(grad_size(D), dtype=torch.float32, device=self.device)
        self._legacy_grad = self._rho_grad = None
        self.f16_fallbacks = 0        # loss_and_grad_sums(check=True) re-runs that cmps_psi_grad_status asked for
        self.timing = None            # a list: forward() / backward() then append HIP-event pairs around their launches (bench.py)

    # ------------------------------------------------------------------
    def __del__(self):
        try:
            if self._h:
                self._lib.cmps_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def variant(self) -> int:
        return int(self._lib.cmps_get_variant(self._h))

    def set_rank1(self, mode: int):
        """cmps_set_option(CMPS_OPT_RANK1): arithmetic of the rank-1 gradient updates (wave kernels, D <= 32)."""
        _capi.check(self._h, self._lib.cmps_set_option(self._h, _capi.CMPS_OPT_RANK1, int(mode)))

    @property
    def rank1(self) -> int:
        return int(self._lib.cmps_get_option(self._h, _capi.CMPS_OPT_RANK1))

    def set_wide_chain(self, mode: int):
        """cmps_set_option(CMPS_OPT_WIDE_CHAIN): 0 = fp32 VALU chain, 1 = fp16 x 2 split operands on the matrix cores (wide kernels' training forward)."""
        _capi.check(self._h, self._lib.cmps_set_option(self._h, _capi.CMPS_OPT_WIDE_CHAIN, int(mode)))

    @property
    def wide_chain(self) -> int:
        return int(self._lib.cmps_get_option(self._h, _capi.CMPS_OPT_WIDE_CHAIN))

    @property
    def effective_rank1(self) -> int:
        """The arithmetic the selected kernels run for the current option value (include/cmps.h): the wide kernels' gradient GEMM
        knows two bf16 pieces, three bf16 pieces (also for EXACT_F32) and two fp16 pieces (also for DEFAULT); the wave reverse scan
        exact fp32, two bf16 pieces, two fp16 pieces (also for DEFAULT) and three bf16 pieces.  (The 16-row kernels of D <= 16 always
        use exact fp32 MFMAs and the legacy mode maps the fp16 form to three bf16 pieces: this property describes the 32-row kernel.)"""
        mode, wide = self.rank1, self.variant == _capi.CMPS_VARIANT_WIDE
        if self._mode == "legacy" and not wide:        # a handle in legacy mode (legacy_set_params): the wave
            # reverse scan's legacy instance has no fp16 form -- F16X2 / DEFAULT run three bf16 pieces (include/cmps.h's table)
            return mode if mode in (_capi.CMPS_RANK1_EXACT_F32, _capi.CMPS_RANK1_BF16X2) else _capi.CMPS_RANK1_BF16X3
        if wide:
            return {0: _capi.CMPS_RANK1_BF16X3, 4: _capi.CMPS_RANK1_F16X2}.get(mode, mode)
        if mode == _capi.CMPS_RANK1_DEFAULT:
            return _capi.CMPS_RANK1_F16X2
        return mode if mode in (_capi.CMPS_RANK1_EXACT_F32, _capi.CMPS_RANK1_BF16X2, _capi.CMPS_RANK1_F16X2) else _capi.CMPS_RANK1_BF16X3

    def kernel_events(self, on: bool):
        """cmps_set_option(CMPS_OPT_KERNEL_EVENTS): bracket every kernel of forward() / backward() and of sample() / sample_primed() / stream() / stream_score() / rho_sample_primed() / rho_stream() / rho_stream_score() / draw_noise() / gather_batch() / loss_stats() / classify_stats() / classify_weights() / bank_posterior() / bank_calibrate() / damped_sine() with HIP
        events (a measurement aid, used by bench.py outside its timed region)."""
        _capi.check(self._h, self._lib.cmps_set_option(self._h, _capi.CMPS_OPT_KERNEL_EVENTS, 1 if on else 0))

    def kernel_times(self) -> dict:
        """cmps_kernel_times: {kernel name: (summed ms, launches)} since the last call, in first-launch order (synchronises)."""
        cap = 32
        names = ctypes.create_string_buffer(2048)
        ms = (ctypes.c_float * cap)()
        calls = (ctypes.c_int * cap)()
        n = self._lib.cmps_kernel_times(self._h, names, 2048, ms, calls, cap)
        if n < 0:
            raise _capi.CmpsError(n, self._lib.cmps_last_error(self._h).decode())
        keys = names.value.decode().split("\n") if n else []
        return {k: (float(ms[i]), int(calls[i])) for i, k in enumerate(keys)}

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ws_flags(train: bool, fresh: bool = True) -> int:
        """The `flags` word of cmps_*workspace_bytes / cmps_*set_*.  fresh=False: this object owns the workspace and has not touched it
        since its previous set_params* -- keep the time table (CMPS_WS_REUSE_TABLES; without it every table is rebuilt)."""
        flags = _capi.CMPS_WS_TRAIN if train else _capi.CMPS_WS_FWD_ONLY
        return flags if fresh else flags | _capi.CMPS_WS_REUSE_TABLES

    def workspace_bytes(self, B: int, T: int, train: bool) -> int:
        return int(self._lib.cmps_workspace_bytes(self.D, B, T, self._ws_flags(train)))

    def _alloc(self, which: str, key: tuple, sized):
        """(256-byte aligned address, usable bytes) of workspace `which` ("main" / "rho"), (re)allocated when `key`, the kind and shape it
        was sized for, changes.  Only then is `sized()` asked for (the bytes the C ABI wants, what they are for): 0 bytes is the ABI's
        answer to an invalid shape."""
        if self._ws_key[which] != key:
            nbytes, what = sized()
            if nbytes == 0:
                raise ValueError(f"invalid shape for {what}")
            self._ws[which] = None        # (free before allocating)
            self._ws[which] = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            self._ws_key[which] = key
            if which == "main":
                self._ws_fresh = True     # the allocator may hand back the old address: the cached tables are gone
        ws = self._ws[which]
        return (ws.data_ptr() + 255) // 256 * 256, ws.numel() - 256

    def _main_workspace(self, key: tuple, sized, reuse: bool = True):
        """set_params* and the bank setters: (flags, address, bytes) of the main workspace, as the C ABI takes them.  `key` ends with the
        train flag.  A reallocated workspace is fresh; one this object has not touched since its last set_params* reuses its tables.
        reuse=False (legacy_set_params, which rebuilds every table): fresh flags, and a reallocation stays noted for the next set_params*."""
        ws_ptr, ws_bytes = self._alloc("main", key, sized)
        if not reuse:
            return self._ws_flags(key[-1]), ws_ptr, ws_bytes
        flags = self._ws_flags(key[-1], self._ws_fresh)
        self._ws_fresh = False
        return flags, ws_ptr, ws_bytes

    def _psi_workspace(self, B: int, T: int, train: bool, reuse: bool = True):
        """set_params* of one model: (flags, address, bytes) of the main workspace, as the C ABI takes them."""
        return self._main_workspace((None, B, T, train), lambda: (self.workspace_bytes(B, T, train), f"the scan: D={self.D}, B={B}, T={T}"), reuse)

    def _rho_workspace(self, B: int, T: int, train: bool, rank: int):
        """rho_set_state*: (address, bytes) of the rho workspace of `rank` columns."""
        return self._alloc("rho", (rank, B, T, train), lambda: (int(self._lib.cmps_rho_workspace_bytes(self.D, rank, B, T, self._ws_flags(train))),
                                                                f"the rho scan (rank={rank}): D={self.D}, B={B}, T={T}"))

    def _configured(self, B: int, T: int, mode: str, M: int = 0, rank: int = 0):
        """What every set_params* ends with: the shape and the arithmetic the handle now holds, and the record of the bank it holds (M
        members; none outside the bank modes).  The batch and the parameter rows a mode kept alive are released when it is left."""
        self._B, self._T, self._mode = B, T, mode
        self._bank = _Bank(mode if M else None, M, rank, scratch=self._bank.scratch)

    def _upload(self, fields, values):
        """Pack `values` as the layout `fields` -> (device tensor, address of every field)."""
        buf = torch.from_numpy(layout.pack(fields, values)).to(self.device)
        return buf, layout.pointers(buf.data_ptr(), fields)

    # ------------------------------------------------------------------
    def set_params(self, p: EffectiveParams, B: int, T: int, train: bool = True):
        """cmps_set_params: upload the effective parameters and rebuild the derived tables."""
        D = self.D
        if np.shape(p.R) != (D, D):
            raise ValueError(f"R must be [{D},{D}]")
        if self._param_evt is not None:
            self._param_evt.synchronize()  # the previous upload must have left the pinned buffer
        fields = layout.param_fields(D)
        layout.pack(fields, {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0)}, out=self._param_host.numpy())
        self._param_buf.copy_(self._param_host, non_blocking=True)
        self._param_evt = torch.cuda.Event()
        self._param_evt.record(torch.cuda.current_stream(self.device))
        _capi.check(self._h, self._lib.cmps_set_params(
            self._h, *layout.pointers(self._param_buf.data_ptr(), fields), float(p.A), float(p.sigma), float(p.delta_t), int(T), int(B),
            *self._psi_workspace(B, T, train), self._stream()))
        self._configured(B, T, "psi")

    def set_params_dev(self, params: torch.Tensor, sigma: float, delta_t: float, B: int, T: int, train: bool = True):
        """cmps_set_params_dev: the effective parameters (A included) are read from the device buffer `params`
        [2 D^2 + 3 D + 1] that cmps_psi_apply_step wrote -- no host copy, no synchronisation."""
        if not (params.is_cuda and params.dtype == torch.float32 and params.numel() == self._n_params + 1):
            raise ValueError("params must be a float32 CUDA tensor of 2 D^2 + 3 D + 1 elements")
        _capi.check(self._h, self._lib.cmps_set_params_dev(self._h, params.data_ptr(), float(sigma), float(delta_t), int(T), int(B),
                                                           *self._psi_workspace(B, T, train), self._stream()))
        self._configured(B, T, "psi")

    def apply_step(self, vars_: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad_sums: Optional[torch.Tensor], global_batch: int,
                   lr_t: float, beta1: float, beta2: float, eps: float, h_reg: float, r_reg: float, c_r: float, c_h: float,
                   with_reg: bool, params: torch.Tensor, losses: torch.Tensor):
        """cmps_psi_apply_step: chain rule + regularisers + Adam + next effective parameters, on the device (grad_sums None: only
        the effective parameters of `vars_`)."""
        if self._opt_scratch is None:
            n = int(self._lib.cmps_apply_step_scratch_bytes(self.D))
            self._opt_scratch = torch.empty((n + 7) // 8, dtype=torch.float64, device=self.device)
        _capi.check(self._h, self._lib.cmps_psi_apply_step(
            self._h, vars_.data_ptr(), m.data_ptr(), v.data_ptr(), grad_sums.data_ptr() if grad_sums is not None else None,
            float(max(global_batch, 1)), float(lr_t), float(beta1), float(beta2), float(eps), float(h_reg), float(r_reg), float(c_r),
            float(c_h), 1 if with_reg else 0, params.data_ptr(), losses.data_ptr(), self._opt_scratch.data_ptr(), self._stream()))

    def rho_apply_step(self, vars_: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad_sums: Optional[torch.Tensor], rank: int,
                       global_batch: int, lr_t: float, beta1: float, beta2: float, eps: float, h_reg: float, r_reg: float, c_r: float,
                       c_h: float, with_reg: bool, params: torch.Tensor, phi: torch.Tensor, losses: torch.Tensor):
        """cmps_rho_apply_step: apply_step for RhoCMPS's variables (Wx, Wy [rank, D]); `phi` [2 rank D] receives the next columns
        (the input of rho_set_state_dev)."""
        key = (self.D, int(rank))
        if self._rho_opt_scratch is None or self._rho_opt_scratch[0] != key:
            n = int(self._lib.cmps_rho_apply_step_scratch_bytes(self.D, int(rank)))
            if n == 0:
                raise ValueError(f"invalid shape for the rho optimiser step: D={self.D}, rank={rank}")
            self._rho_opt_scratch = (key, torch.empty((n + 7) // 8, dtype=torch.float64, device=self.device))
        if phi.numel() != 2 * int(rank) * self.D:
            raise ValueError("phi must have 2 rank D elements")
        _capi.check(self._h, self._lib.cmps_rho_apply_step(
            self._h, vars_.data_ptr(), m.data_ptr(), v.data_ptr(), grad_sums.data_ptr() if grad_sums is not None else None, int(rank),
            float(max(global_batch, 1)), float(lr_t), float(beta1), float(beta2), float(eps), float(h_reg), float(r_reg), float(c_r),
            float(c_h), 1 if with_reg else 0, params.data_ptr(), phi.data_ptr(), losses.data_ptr(),
            self._rho_opt_scratch[1].data_ptr(), self._stream()))

    # ------------------------------------------------------------------
    # Model bank (cmps_bank_*): M PsiCMPS models of this handle's D per launch.  The bank's workspace is M plain ones behind each other.
    def bank_workspace_bytes(self, M: int, B: int, T: int, train: bool) -> int:
        return int(self._lib.cmps_bank_workspace_bytes(self.D, int(M), B, T, self._ws_flags(train)))

    def bank_set_params_dev(self, params: torch.Tensor, sigma: float, delta_t: float, B: int, T: int, train: bool = True):
        """cmps_bank_set_params_dev: ``params`` [M, 2 D^2 + 3 D + 1], the buffer bank_apply_step wrote; every member's tables are rebuilt."""
        if not _is_tensor(params, None, torch.float32, (None, self._n_params + 1)):
            raise ValueError("params must be a contiguous float32 CUDA tensor [M, 2 D^2 + 3 D + 1]")
        M = int(params.shape[0])
        ws = self._main_workspace(("bank", M, B, T, train),
                                  lambda: (self.bank_workspace_bytes(M, B, T, train), f"a bank: D={self.D}, M={M}, B={B}, T={T}"))
        _capi.check(self._h, self._lib.cmps_bank_set_params_dev(self._h, M, params.data_ptr(), float(sigma), float(delta_t), int(T), int(B), *ws,
                                                                self._stream()))
        self._configured(B, T, "bank", M)

    # The drivers of both kinds of bank (`kind`: a key of BANK_SETTER, also the prefix of the public methods' names)
    def _bank_of(self, kind: str, what: str) -> _Bank:
        """The record of the bank of `kind` this handle holds; without one, the RuntimeError of the method `what`."""
        if self._bank.kind != kind:
            raise RuntimeError(f"{what}() needs {BANK_SETTER[kind]}() first")
        return self._bank

    def _bank_audio(self, M: int, audio: torch.Tensor):
        """A bank's batch [B, T] (shared) or [M, B, T] -> (n_audio, B, T) as the scan entries take them."""
        if not (_is_tensor(audio, None, torch.float32, 2) or _is_tensor(audio, None, torch.float32, 3)):
            raise ValueError("audio must be a contiguous float32 CUDA tensor [B, T] (shared) or [M, B, T]")
        n_audio = 1 if audio.dim() == 2 else int(audio.shape[0])
        B, T = audio.shape[-2:]
        if n_audio not in (1, M) or T != self._T or B > self._B:
            raise ValueError(f"audio shape {tuple(audio.shape)} does not fit the bank (M={M}, B={self._B}, T={self._T})")
        return n_audio, int(B), int(T)

    def _bank_forward(self, kind: str, fn, audio: torch.Tensor, save_for_bwd: bool) -> torch.Tensor:
        """The one forward driver of a bank: `fn` is cmps_{bank,rho_bank}_loss_fwd.  Returns the per-clip losses [M, B]."""
        bank = self._bank_of(kind, kind + "_forward")
        n_audio, B, T = self._bank_audio(bank.M, audio)
        loss = torch.empty((bank.M, B), dtype=torch.float32, device=self.device)
        _capi.check(self._h, fn(self._h, audio.data_ptr(), n_audio, B, T, loss.data_ptr(), 1 if save_for_bwd else 0, self._stream()))
        bank.saved = (audio, loss, n_audio)
        return loss

    def _bank_backward(self, kind: str, fn) -> torch.Tensor:
        """The one backward driver of a bank: `fn` is cmps_{bank,rho_bank}_loss_bwd.  Returns the gradient sums, one row per member."""
        bank = self._bank
        if bank.kind != kind or bank.saved is None:
            raise RuntimeError(f"{kind}_backward() needs {kind}_forward(save_for_bwd=True) first")
        audio, _, n_audio = bank.saved
        B, T = audio.shape[-2:]
        grad = torch.empty((bank.M, grad_size(self.D, bank.rank)), dtype=torch.float32, device=self.device)
        _capi.check(self._h, fn(self._h, audio.data_ptr(), n_audio, int(B), int(T), grad.data_ptr(), self._stream()))
        return grad

    def _bank_apply_step(self, fn, n_scratch: int, vars_, m, v, grad_sums, rank: tuple, global_batch, bias_num, bias_den, beta1, beta2, eps,
                         hyper, with_reg, outs: tuple):
        """The one apply-step driver of a bank: `fn` is cmps_{bank,rho_bank}_apply_step, `n_scratch` its scratch bytes, `rank` what it
        takes behind grad_sums_dev (nothing, or the rank), `outs` the buffers it writes, in its order."""
        bank = self._bank
        if bank.scratch is None or bank.scratch.numel() * 8 < n_scratch:
            bank.scratch = torch.empty((n_scratch + 7) // 8, dtype=torch.float64, device=self.device)
        _capi.check(self._h, fn(
            self._h, int(vars_.shape[0]), vars_.data_ptr(), m.data_ptr(), v.data_ptr(), grad_sums.data_ptr() if grad_sums is not None else None,
            *rank, float(max(global_batch, 1)), float(bias_num), float(bias_den), float(beta1), float(beta2), float(eps), hyper.data_ptr(),
            1 if with_reg else 0, *(t.data_ptr() for t in outs), bank.scratch.data_ptr(), self._stream()))

    @staticmethod
    def _check_hyper(hyper: torch.Tensor, M: int):
        if not _is_tensor(hyper, None, torch.float64, (M, 5)):
            raise ValueError("hyper must be a contiguous float64 CUDA tensor [M, 5]")

    def bank_forward(self, audio: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        """cmps_bank_loss_fwd: per-clip losses [M, B] for ``audio`` [B, T] (one batch shared by every member) or [M, B, T]."""
        return self._bank_forward("bank", self._lib.cmps_bank_loss_fwd, audio, save_for_bwd)

    def bank_backward(self, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cmps_bank_loss_bwd after bank_forward(save_for_bwd=True): gradient sums [M, 2 D^2 + 3 D + 2].  With ``weights`` (float32
        [M, B] on this device, rows contiguous; classify_weights' output) cmps_bank_loss_bwd_weighted: member m's row is the gradient of
        sum_b weights[m, b] * loss[m, b], its last element that sum."""
        if weights is None:
            return self._bank_backward("bank", self._lib.cmps_bank_loss_bwd)
        saved = self._bank.saved if self._bank.kind == "bank" else None
        M, B = (self._bank.M, int(saved[0].shape[-2])) if saved is not None else (-1, -1)
        if not _is_tensor(weights, self.device, torch.float32, 2, rows=True):
            raise ValueError("bank_backward: weights must be a float32 tensor [M, B] with contiguous rows on the backend's device")
        if saved is not None and tuple(weights.shape) != (M, B):
            raise ValueError(f"bank_backward: weights of shape {tuple(weights.shape)} do not fit the forward's losses [{M}, {B}]")
        ldw = int(weights.stride(0)) if weights.shape[0] > 1 else int(weights.shape[1])
        w_ptr = weights.data_ptr()

        def weighted(h, audio, n_audio, B_, T_, grad, stream):
            return self._lib.cmps_bank_loss_bwd_weighted(h, audio, n_audio, B_, T_, w_ptr, ldw, grad, stream)
        return self._bank_backward("bank", weighted)

    def bank_apply_step(self, vars_: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad_sums: Optional[torch.Tensor], global_batch: int,
                        bias_num: float, bias_den: float, beta1: float, beta2: float, eps: float, hyper: torch.Tensor, with_reg: bool,
                        params: torch.Tensor, losses: torch.Tensor):
        """cmps_bank_apply_step: every member's optimiser step; ``hyper`` [M, 5] float64 on the device (learning_rate, h_reg, r_reg, c_r, c_h)."""
        M = int(vars_.shape[0])
        self._check_hyper(hyper, M)
        self._bank_apply_step(self._lib.cmps_bank_apply_step, int(self._lib.cmps_bank_apply_step_scratch_bytes(self.D, M)), vars_, m, v,
                              grad_sums, (), global_batch, bias_num, bias_den, beta1, beta2, eps, hyper, with_reg, (params, losses))

    def bank_grad_status(self):
        """cmps_bank_grad_status: (codes [M], sticky flags [M]).  Waits for the stream."""
        M = self._bank_of("bank", "bank_grad_status").M
        codes, sticky = (ctypes.c_int * M)(), (ctypes.c_int * M)()
        _capi.check(self._h, self._lib.cmps_bank_grad_status(self._h, codes, sticky, self._stream()))
        return [int(c) for c in codes], [int(x) for x in sticky]

    # ------------------------------------------------------------------
    # Model bank of RhoCMPS members (cmps_rho_bank_*): ONE workspace, every member's main layout (tables only) followed by its rho layout.
    def rho_bank_workspace_bytes(self, rank: int, M: int, B: int, T: int, train: bool) -> int:
        return int(self._lib.cmps_rho_bank_workspace_bytes(self.D, int(rank), int(M), B, T, self._ws_flags(train)))

    def rho_bank_set_state_dev(self, params: torch.Tensor, phi: torch.Tensor, rank: int, sigma: float, delta_t: float, B: int, T: int,
                               train: bool = True):
        """cmps_rho_bank_set_state_dev: ``params`` [M, 2 D^2 + 3 D + 1] and ``phi`` [M, 2 rank D], the buffers rho_bank_apply_step wrote."""
        rank = int(rank)
        if not _is_tensor(params, None, torch.float32, (None, self._n_params + 1)):
            raise ValueError("params must be a contiguous float32 CUDA tensor [M, 2 D^2 + 3 D + 1]")
        M = int(params.shape[0])
        if not _is_tensor(phi, None, torch.float32, (M, 2 * rank * self.D)):
            raise ValueError("phi must be a contiguous float32 CUDA tensor [M, 2 rank D]")
        ws = self._main_workspace(("rho_bank", M, rank, B, T, train), lambda: (self.rho_bank_workspace_bytes(rank, M, B, T, train),
                                                                                f"a RhoCMPS bank: D={self.D}, rank={rank}, M={M}, B={B}, T={T}"))
        _capi.check(self._h, self._lib.cmps_rho_bank_set_state_dev(self._h, M, params.data_ptr(), phi.data_ptr(), rank, float(sigma), float(delta_t),
                                                                   int(T), int(B), *ws, self._stream()))
        self._configured(B, T, "rho_bank", M, rank)
        self._rho_rank = 0            # (the plain rho state is gone: rho_forward() asks for rho_set_state again)

    def rho_bank_forward(self, audio: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        """cmps_rho_bank_loss_fwd: per-clip losses [M, B] for ``audio`` [B, T] (one batch shared by every member) or [M, B, T]."""
        return self._bank_forward("rho_bank", self._lib.cmps_rho_bank_loss_fwd, audio, save_for_bwd)

    def rho_bank_backward(self) -> torch.Tensor:
        """cmps_rho_bank_loss_bwd after rho_bank_forward(save_for_bwd=True): gradient sums [M, 2 D^2 + 3 D + 2 + 2 rank D]."""
        return self._bank_backward("rho_bank", self._lib.cmps_rho_bank_loss_bwd)

    def rho_bank_apply_step(self, vars_: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad_sums: Optional[torch.Tensor], rank: int,
                            global_batch: int, bias_num: float, bias_den: float, beta1: float, beta2: float, eps: float,
                            hyper: torch.Tensor, with_reg: bool, params: torch.Tensor, phi: torch.Tensor, losses: torch.Tensor):
        """cmps_rho_bank_apply_step: every member's optimiser step; ``hyper`` [M, 5] float64 on the device as for bank_apply_step."""
        M, rank = int(vars_.shape[0]), int(rank)
        self._check_hyper(hyper, M)
        if tuple(phi.shape) != (M, 2 * rank * self.D) or tuple(params.shape) != (M, self._n_params + 1):
            raise ValueError("phi must be [M, 2 rank D] and params [M, 2 D^2 + 3 D + 1]")
        n = int(self._lib.cmps_rho_bank_apply_step_scratch_bytes(self.D, rank, M))
        if n == 0:
            raise ValueError(f"invalid shape for a RhoCMPS bank's optimiser step: D={self.D}, rank={rank}, M={M}")
        self._bank_apply_step(self._lib.cmps_rho_bank_apply_step, n, vars_, m, v, grad_sums, (rank,), global_batch, bias_num, bias_den, beta1,
                              beta2, eps, hyper, with_reg, (params, phi, losses))

    def _check_audio(self, audio: torch.Tensor):
        if not _is_tensor(audio, None, torch.float32, 2):
            raise ValueError("audio must be a contiguous float32 CUDA tensor [B, T]")
        B, T = audio.shape
        if T != self._T or B > self._B:
            raise ValueError(f"audio shape {tuple(audio.shape)} does not fit set_params(B={self._B}, T={self._T})")
        return B, T

    def _forward(self, fn, audio: torch.Tensor, save_for_bwd: bool, timed: bool = False, slot: str = "_loss") -> torch.Tensor:
        """The one forward driver: `fn` is cmps_{psi,legacy,rho}_loss_fwd.  Returns this object's per-clip loss tensor [B] (`slot`)."""
        B, T = self._check_audio(audio)
        loss = getattr(self, slot)
        if loss is None or loss.numel() != B:
            loss = torch.empty(B, dtype=torch.float32, device=self.device)
            setattr(self, slot, loss)
        ev = self._event_pair() if timed else None
        _capi.check(self._h, fn(self._h, audio.data_ptr(), B, T, loss.data_ptr(), 1 if save_for_bwd else 0, self._stream()))
        self._event_close("fwd", ev)
        self._audio = audio
        return loss

    def _backward(self, fn, grad: Optional[torch.Tensor], n: int, who: str = "", timed: bool = False) -> torch.Tensor:
        """The one backward driver: `fn` is cmps_{psi,legacy,rho}_loss_bwd, `grad` the caller's buffer for its `n` gradient sums
        (replaced when it does not fit), which is returned."""
        audio = self._audio
        if audio is None:
            raise RuntimeError(f"{who}backward() needs {who}forward(save_for_bwd=True) first")
        B, T = audio.shape
        if grad is None or grad.numel() != n:
            grad = torch.empty(n, dtype=torch.float32, device=self.device)
        ev = self._event_pair() if timed else None
        _capi.check(self._h, fn(self._h, audio.data_ptr(), B, T, grad.data_ptr(), self._stream()))
        self._event_close("bwd", ev)
        return grad

    def forward(self, audio: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        """Per-clip loss [B] (device tensor): cmps_psi_loss_fwd."""
        return self._forward(self._lib.cmps_psi_loss_fwd, audio, save_for_bwd, timed=True)

    def backward(self) -> torch.Tensor:
        """Flat gradient sums [2D^2+3D+2] (device tensor): cmps_psi_loss_bwd after forward(save_for_bwd=True)."""
        return self._backward(self._lib.cmps_psi_loss_bwd, self._grad, self._grad.numel(), timed=True)

    # HIP events on the stream the kernels are launched on (torch's current stream is the one handed to the C ABI); they are read
    # only after the caller has synchronised (timing_ms), so recording them never stalls the host
    def _event_pair(self):
        if self.timing is None:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(self.device))
        return e0, e1

    def _event_close(self, what, ev):
        if ev is not None:
            ev[1].record(torch.cuda.current_stream(self.device))
            self.timing.append((what, ev[0], ev[1]))

    def timing_ms(self):
        """{'fwd': [ms ...], 'bwd': [ms ...]} of the launches recorded since `timing` was set to a list (synchronises)."""
        torch.cuda.synchronize(self.device)
        out = {"fwd": [], "bwd": []}
        for what, e0, e1 in self.timing or []:
            out[what].append(e0.elapsed_time(e1))
        return out

    def grad_status(self):
        """cmps_psi_grad_status: (code, sticky flags).  Waits for the stream.  code = CMPS_ERR_F16_RANGE when the last backward()
        left Inf / NaN in the gradient next to finite per-clip losses (an fp16-split operand out of its scaled range)."""
        sticky = ctypes.c_int(0)
        code = int(self._lib.cmps_psi_grad_status(self._h, ctypes.byref(sticky), self._stream()))
        if code not in (_capi.CMPS_OK, _capi.CMPS_ERR_F16_RANGE):
            _capi.check(self._h, code)
        return code, int(sticky.value)

    def loss_and_grad_sums(self, audio: torch.Tensor, check: bool = False):
        """forward(save) + backward().  check=True (the host trainer and the model's gradient accessors: they read the result
        on the host anyway) asks cmps_psi_grad_status afterwards and, on CMPS_ERR_F16_RANGE, takes the documented fallback once:
        CMPS_OPT_RANK1 = BF16X3, CMPS_OPT_WIDE_CHAIN = VALU (no fp16 piece anywhere), the same two calls again; the handle's
        options are restored.  A gradient that is non-finite in that arithmetic as well is returned as it is (it propagates, as in
        the reference)."""
        loss = self.forward(audio, save_for_bwd=True)
        grad = self.backward()
        if check:
            code, _ = self.grad_status()
            if code == _capi.CMPS_ERR_F16_RANGE and (self.effective_rank1 == _capi.CMPS_RANK1_F16X2 or
                                                     (self.variant == _capi.CMPS_VARIANT_WIDE and self.wide_chain != _capi.CMPS_WIDE_CHAIN_VALU)):
                import warnings
                warnings.warn("libcmps: " + self._lib.cmps_last_error(self._h).decode() + " -- re-running this batch with bf16x3 pieces")
                keep = (self.rank1, self.wide_chain)
                self.f16_fallbacks += 1
                try:
                    self.set_rank1(_capi.CMPS_RANK1_BF16X3)
                    self.set_wide_chain(_capi.CMPS_WIDE_CHAIN_VALU)
                    loss = self.forward(audio, save_for_bwd=True)
                    grad = self.backward()
                finally:
                    self.set_rank1(keep[0])
                    self.set_wide_chain(keep[1])
        return loss, grad

    # ------------------------------------------------------------------
    def _ancilla(self, fn, what: str, x: np.ndarray, signal: np.ndarray, t: float) -> np.ndarray:
        """One update step of a batch of states [B, D] / matrices [B, D, D] (host in, host out): `fn` is cmps_{psi,rho}_update_ancilla."""
        x = np.asarray(x, dtype=np.complex64)
        if x.shape[1:] != (self.D,) * (1 if what == "psi" else 2):
            raise ValueError(f"{what} has the wrong bond dimension")
        d_in = _to_interleaved(x, self.device)
        d_sig = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32)).to(self.device)
        d_out = torch.empty_like(d_in)
        _capi.check(self._h, fn(self._h, d_in.data_ptr(), d_sig.data_ptr(), float(t), x.shape[0], d_out.data_ptr(), self._stream()))
        return _from_interleaved(d_out)

    def draw_noise(self, seed: int, first_step: int, n: int, length: int, std: float, first_path: int = 0) -> torch.Tensor:
        """cmps_noise_fill: the samplers' noise drawn on the device, float32 [n, length] (the layout the sampler entries read), element
        [b, j] = std * z(seed, first_path + b, first_step + j) of include/cmps.h.  No host copy, no synchronisation."""
        n, length = int(n), int(length)
        if n < 1 or length < 1:
            raise ValueError("draw_noise needs n >= 1 and length >= 1")
        out = torch.empty((n, length), dtype=torch.float32, device=self.device)
        _capi.check(self._h, self._lib.cmps_noise_fill(self._h, int(seed), int(first_step), int(first_path), n, length, float(std),
                                                       out.data_ptr(), self._stream()))
        return out

    def gather_batch(self, data: torch.Tensor, index: torch.Tensor, offset: Optional[torch.Tensor] = None, T: Optional[int] = None,
                     scale: float = 2.0 ** -15) -> torch.Tensor:
        """cmps_batch_gather: a batch cut out of a dataset that lives on the device.  ``data`` float32 [N, L], ``index`` (and ``offset``,
        default all zero) int32 [B], all contiguous on this device; returns float32 [B, T] (T defaults to L) with row b =
        data[index[b], offset[b] : offset[b] + T] -- or T quiet NaNs where index[b] or offset[b] is out of range.  No host copy, no
        synchronisation.  ``data`` int16 [N, L] goes to cmps_batch_gather_i16 instead: row b = float32(data[...]) * ``scale``."""
        i16 = isinstance(data, torch.Tensor) and data.dtype == torch.int16
        if not _is_tensor(data, self.device, torch.int16 if i16 else torch.float32, 2):
            raise ValueError("gather_batch: data must be a contiguous float32 or int16 tensor [N, L] on the backend's device")
        if not _is_tensor(index, self.device, torch.int32, 1) or (offset is not None and not _is_tensor(offset, self.device, torch.int32, tuple(index.shape))):
            raise ValueError("gather_batch: index (and offset) must be contiguous int32 tensors [B] on the backend's device")
        N, L = int(data.shape[0]), int(data.shape[1])
        B, T = int(index.shape[0]), L if T is None else int(T)
        out = torch.empty((B, T), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        off_ptr = offset.data_ptr() if offset is not None else None
        if i16:
            _capi.check(self._h, self._lib.cmps_batch_gather_i16(self._h, data.data_ptr(), N, L, index.data_ptr(), off_ptr, B, T,
                                                                 float(scale), out.data_ptr(), self._stream()))
        else:
            _capi.check(self._h, self._lib.cmps_batch_gather(self._h, data.data_ptr(), N, L, index.data_ptr(), off_ptr, B, T,
                                                             out.data_ptr(), self._stream()))
        return out

    def loss_stats(self, loss: torch.Tensor, first_id: int, stats: Optional[torch.Tensor] = None, reset: bool = False) -> torch.Tensor:
        """cmps_loss_stats: fold the per-clip losses ``loss`` [B] (float32, on this device; clip ids first_id .. first_id + B - 1) into the
        64-byte record ``stats`` (a uint8 device tensor this method allocates -- and resets -- when None) and return it.  No host copy, no
        synchronisation: read_stats is the download."""
        if not (_is_tensor(loss, self.device, torch.float32, 1) and loss.numel() >= 1):
            raise ValueError("loss_stats: loss must be a contiguous float32 tensor [B], B >= 1, on the backend's device")
        stats, reset = self._record(stats, 64, reset, "loss_stats: stats")
        _capi.check(self._h, self._lib.cmps_loss_stats(self._h, loss.data_ptr(), int(loss.numel()), int(first_id), 1 if reset else 0,
                                                       stats.data_ptr(), self._stream()))
        return stats

    def _record(self, record: Optional[torch.Tensor], nbytes: int, reset: bool, what: str):
        """A device record of ``nbytes`` bytes and whether the entry resets it: a new one (reset), or the caller's, checked."""
        if record is None:
            return torch.empty(nbytes, dtype=torch.uint8, device=self.device), True
        if not _is_tensor(record, self.device, torch.uint8, (nbytes,)):
            raise ValueError(f"{what} must be a contiguous uint8 tensor of {nbytes} bytes on the backend's device")
        return record, reset

    def _member_losses(self, loss, who: str, what: str = "loss"):
        """(M, B, ld) of ``loss`` [M, B], every member's value of every clip as the classifier entries take it: float32 on this device,
        rows contiguous ``ld`` floats apart, 1 <= M <= CLASSIFY_MAX_M and B >= 1."""
        if not (_is_tensor(loss, self.device, torch.float32, 2, rows=True) and loss.numel() >= 1):
            raise ValueError(f"{who}: {what} must be a float32 tensor [M, B] with contiguous rows, M >= 1 and B >= 1, on the backend's device")
        M, B = int(loss.shape[0]), int(loss.shape[1])
        if M > _capi.CLASSIFY_MAX_M:
            raise ValueError(f"{who}: a bank holds 1 .. {_capi.CLASSIFY_MAX_M} members, not {M}")
        return M, B, int(loss.stride(0)) if M > 1 else B

    def _clip_labels(self, labels, B: int, who: str, what: str = "labels"):
        if not _is_tensor(labels, self.device, torch.int32, (B,)):
            raise ValueError(f"{who}: {what} must be a contiguous int32 tensor [B] on the backend's device")

    @staticmethod
    def read_stats(stats: torch.Tensor) -> dict:
        """The record of loss_stats as a dict of Python numbers (_capi.LOSS_STATS's fields): the one device -> host copy of an evaluation."""
        return _read_record(stats, _capi.LOSS_STATS)[0]

    def classify_stats(self, loss: torch.Tensor, labels: Optional[torch.Tensor], first_id: int, stats: Optional[torch.Tensor] = None,
                       reset: bool = False, best: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cmps_bank_classify_stats: judge the losses ``loss`` [M, B] of a bank forward over one shared batch (float32 on this device, rows
        contiguous; clip ids first_id .. first_id + B - 1) as a classifier and fold the result into the record ``stats`` (a uint8 device
        tensor of cmps_bank_classify_stats_bytes(M) bytes this method allocates -- and resets -- when None), which it returns.
        ``labels``: int32 [B] on this device, the member each clip belongs to (outside [0, M): unlabelled), or None for no labels;
        ``best``: int32 [B] to receive each clip's decision.  No host copy, no synchronisation: read_classify_stats is the download."""
        M, B, ld = self._member_losses(loss, "classify_stats")
        for name, t in (("labels", labels), ("best", best)):
            if t is not None:
                self._clip_labels(t, B, "classify_stats", name)
        stats, reset = self._record(stats, int(self._lib.cmps_bank_classify_stats_bytes(M)), reset, "classify_stats: stats")
        _capi.check(self._h, self._lib.cmps_bank_classify_stats(
            self._h, loss.data_ptr(), M, B, ld, labels.data_ptr() if labels is not None else None, int(first_id), 1 if reset else 0,
            stats.data_ptr(), best.data_ptr() if best is not None else None, self._stream()))
        return stats

    @staticmethod
    def read_classify_stats(stats: torch.Tensor, M: int) -> dict:
        """The record of classify_stats: the header's fields as Python numbers (_capi.CLASSIFY_HEAD), ``confusion`` [M, M] and
        ``unlabelled_best`` [M] as int64 arrays.  The one device -> host copy of a classifier evaluation."""
        out, rec = _read_record(stats, _capi.classify_stats_dtype(M), "head")
        out["confusion"], out["unlabelled_best"] = rec["confusion"].copy(), rec["unlabelled_best"].copy()
        return out

    def classify_weights(self, loss: torch.Tensor, labels: torch.Tensor, inv_temp: float, gen_weight: float, disc_weight: float,
                         weights: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None, reset: bool = True):
        """cmps_bank_classify_weights: turn the losses ``loss`` [M, B] of a bank forward over one shared batch and the ``labels`` (int32
        [B] on this device) into the cotangents of the cross-entropy objective of include/cmps.h, ``weights`` [M, B] (float32, rows
        contiguous; allocated when None), and fold the batch into the 40-byte ``record`` (uint8 on this device; allocated -- and reset --
        when None).  Returns (weights, record).  No host copy, no synchronisation: read_classify_weights_record is the download."""
        M, B, ld = self._member_losses(loss, "classify_weights")
        self._clip_labels(labels, B, "classify_weights")
        if weights is None:
            weights, ldw = torch.empty((M, B), dtype=torch.float32, device=self.device), B
        else:
            Mw, Bw, ldw = self._member_losses(weights, "classify_weights", "weights")
            if (Mw, Bw) != (M, B):
                raise ValueError(f"classify_weights: weights must be [{M}, {B}] as loss is, not {list(weights.shape)}")
        record, reset = self._record(record, _capi.CLASSIFY_WEIGHTS_REC.itemsize, reset, "classify_weights: record")
        _capi.check(self._h, self._lib.cmps_bank_classify_weights(
            self._h, loss.data_ptr(), M, B, ld, labels.data_ptr(), float(inv_temp), float(gen_weight), float(disc_weight),
            1 if reset else 0, weights.data_ptr(), ldw, record.data_ptr(), self._stream()))
        return weights, record

    @staticmethod
    def read_classify_weights_record(record: torch.Tensor) -> dict:
        """The record of classify_weights as a dict of Python numbers (_capi.CLASSIFY_WEIGHTS_REC's fields): one 40-byte download."""
        return _read_record(record, _capi.CLASSIFY_WEIGHTS_REC)[0]

    def bank_calibrate(self, loss: torch.Tensor, labels: torch.Tensor, fit: int, kappa: float, log_prior=None, tol: float = 1e-9,
                       max_iter: int = 200, kappa_min: float = 1e-6, kappa_max: float = 1e6) -> torch.Tensor:
        """cmps_bank_calibrate: fit the inverse temperature and (or) the log prior of a class bank on the held-out losses ``loss`` [M, N]
        (float32 on this device, rows contiguous) and ``labels`` (int32 [N] on this device), from the start ``kappa`` and ``log_prior``
        ([M] floats, finite or -inf; None: zeros).  ``fit``: a set of _capi.CMPS_CALIB_TEMPERATURE | _capi.CMPS_CALIB_PRIOR; 0 (or
        max_iter = 0) evaluates the cross-entropy under the given values.  Returns ONE uint8 device tensor, theta [1 + M] doubles with
        the 80-byte record behind it: read_calibrate_record is the one download.  No host copy of the losses, no synchronisation."""
        M, N, ld = self._member_losses(loss, "bank_calibrate")
        self._clip_labels(labels, N, "bank_calibrate")
        theta = np.zeros(1 + M, dtype=np.float64)
        theta[0] = float(kappa)
        if log_prior is not None:
            theta[1:] = np.asarray(log_prior, dtype=np.float64).reshape(M)
        out = torch.empty(8 * (1 + M) + _capi.CALIB_REC.itemsize, dtype=torch.uint8, device=self.device)
        out[:8 * (1 + M)].copy_(torch.from_numpy(theta.view(np.uint8)))
        nbytes = int(self._lib.cmps_bank_calibrate_scratch_bytes(M, N))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        _capi.check(self._h, self._lib.cmps_bank_calibrate(
            self._h, loss.data_ptr(), M, N, ld, labels.data_ptr(), int(fit), int(max_iter), float(tol),
            float(kappa_min), float(kappa_max), out.data_ptr(), out.data_ptr() + 8 * (1 + M), scratch.data_ptr(), nbytes, self._stream()))
        return out

    @staticmethod
    def read_calibrate_record(out: torch.Tensor) -> tuple:
        """What bank_calibrate returned, downloaded once: (theta [1 + M] float64, the record as a dict of Python numbers)."""
        raw = out.cpu().numpy()
        split = raw.size - _capi.CALIB_REC.itemsize
        rec = raw[split:].view(_capi.CALIB_REC)[0]
        return raw[:split].view(np.float64).copy(), {k: (float(rec[k]) if rec.dtype[k].kind == "f" else int(rec[k])) for k in rec.dtype.names}

    def log_prior_tensor(self, log_prior) -> Optional[torch.Tensor]:
        """A log prior [M] (finite or -inf) as `bank_posterior` takes it: float64 on this device.  None stays None (a uniform prior)."""
        if log_prior is None or isinstance(log_prior, torch.Tensor):
            return log_prior
        return torch.from_numpy(np.array(log_prior, dtype=np.float64, order="C")).to(self.device)

    def bank_posterior(self, nll: torch.Tensor, total_in: Optional[torch.Tensor] = None, log_prior: Optional[torch.Tensor] = None,
                       inv_temp: float = 1.0, threshold: Optional[float] = None, first_step: int = 0,
                       decision: Optional[torch.Tensor] = None, want_post: bool = False) -> dict:
        """cmps_bank_posterior: the per-step losses ``nll`` [M, n, steps] of a scored bank stream (float32, contiguous, on this device)
        folded into the running totals and, after every step, the posterior over the members.  ``total_in`` [M, n] float32 or None (zeros),
        ``log_prior`` [M] float64 or None (uniform).  With a ``threshold`` the first step at which the best member's probability reached
        it is kept per path in ``decision`` (a uint8 tensor of 16 n bytes, _capi.DECISION_REC; None: a fresh one), numbered from
        ``first_step``.  Returns {"total": [M, n], "best": int32 [n, steps], "conf": [n, steps], "post": [M, n, steps] with want_post else
        None, "decision": the records (new memory, continued from ``decision``) or None}, all on the device; "pack" is the one uint8
        tensor the small results are views of, in the order and sizes of "pack_sizes" (records, total, best, conf).  No host copy, no
        synchronisation."""
        if not (_is_tensor(nll, self.device, torch.float32, 3) and nll.numel() >= 1):
            raise ValueError("bank_posterior: nll must be a contiguous float32 tensor [M, n, steps] with M, n, steps >= 1 on the backend's device")
        M, n, steps = (int(x) for x in nll.shape)
        if M > _capi.CLASSIFY_MAX_M:
            raise ValueError(f"bank_posterior: a bank holds 1 .. {_capi.CLASSIFY_MAX_M} members, not {M}")
        if total_in is not None and not _is_tensor(total_in, self.device, torch.float32, (M, n)):
            raise ValueError(f"bank_posterior: total_in must be a contiguous float32 tensor [{M}, {n}] on the backend's device")
        if log_prior is not None and not _is_tensor(log_prior, self.device, torch.float64, (M,)):
            raise ValueError(f"bank_posterior: log_prior must be a contiguous float64 tensor [{M}] on the backend's device")
        if threshold is None and decision is not None:
            raise ValueError("bank_posterior: decision records need a threshold")
        if decision is not None and not _is_tensor(decision, self.device, torch.uint8, (16 * n,)):
            raise ValueError(f"bank_posterior: decision must be a contiguous uint8 tensor of {16 * n} bytes on the backend's device")
        # one allocation for everything small, so that a caller who wants it on the host downloads once: records | total | best | conf
        sizes = (16 * n if threshold is not None else 0, 4 * M * n, 4 * n * steps, 4 * n * steps)
        pack = torch.empty(sum(sizes), dtype=torch.uint8, device=self.device)
        rec, b_total, b_best, b_conf = torch.split(pack, sizes)
        total, best, conf = b_total.view(torch.float32).view(M, n), b_best.view(torch.int32).view(n, steps), b_conf.view(torch.float32).view(n, steps)
        if threshold is None:
            rec = None
        elif decision is not None:
            rec.copy_(decision)                                        # continued where the caller's records are, in the new allocation
        post = torch.empty((M, n, steps), dtype=torch.float32, device=self.device) if want_post else None
        _capi.check(self._h, self._lib.cmps_bank_posterior(
            self._h, _ptr(nll), M, n, steps, _ptr(total_in), _ptr(log_prior), float(inv_temp), _ptr(total), _ptr(post), _ptr(best), _ptr(conf),
            0.0 if threshold is None else float(threshold), int(first_step), int(decision is None), _ptr(rec), self._stream()))
        return {"total": total, "best": best, "conf": conf, "post": post, "decision": rec, "pack": pack, "pack_sizes": sizes}

    def damped_sine(self, seed: int, first_clip: int, B: int, T: int, delta_t: float) -> torch.Tensor:
        """cmps_damped_sine_fill: clips first_clip .. first_clip + B - 1 of the seed's synthetic damped-sine sequence (include/cmps.h),
        float32 [B, T], generated on the device.  No host copy, no synchronisation."""
        B, T = int(B), int(T)
        if B < 1 or T < 1:
            raise ValueError("damped_sine needs B >= 1 and T >= 1")
        out = torch.empty((B, T), dtype=torch.float32, device=self.device)
        _capi.check(self._h, self._lib.cmps_damped_sine_fill(self._h, int(seed), int(first_clip), B, T, float(delta_t), out.data_ptr(),
                                                             self._stream()))
        return out

    def _device_noise(self, noise, length=None, n=None):
        """What a sampler entry is handed as ``noise`` -> (device tensor [n, length], length, n).  A host array [length, n] (the reference's
        layout) is transposed and uploaded; a device tensor [n, length] is used as it is; a NoisePlan is drawn by `draw_noise` for the
        ``length`` and ``n`` given.  With an array, ``length`` and ``n`` default to its shape and must agree with it."""
        if isinstance(noise, NoisePlan):
            if length is None or n is None:
                raise ValueError("a NoisePlan needs length and n: there is no array to take them from")
            d_noise = self.draw_noise(noise.seed, noise.first_step, n, length, noise.std)
        elif isinstance(noise, torch.Tensor):
            if not _is_tensor(noise, None, torch.float32, 2):
                raise ValueError("device noise must be a contiguous float32 CUDA tensor [n, length]")
            d_noise = noise
        else:
            noise = np.asarray(noise, dtype=np.float32)
            if noise.ndim != 2:
                raise ValueError("noise must be [length, n]")
            d_noise = torch.from_numpy(np.array(noise.T, order="C")).to(self.device)    # (a copy: torch wants a writable array)
        if (length is not None and int(length) != d_noise.shape[1]) or (n is not None and int(n) != d_noise.shape[0]):
            raise ValueError(f"noise for {tuple(d_noise.shape)} (paths, steps) does not fit length={length}, n={n}")
        return d_noise, int(d_noise.shape[1]), int(d_noise.shape[0])

    def _sample(self, fn, noise, length, n, *flags) -> np.ndarray:
        """Noise (`_device_noise`: pre-drawn [length, n] in the reference's layout, a device tensor, or a NoisePlan) in, waveforms
        [n, length] down: `fn` is cmps_{psi,rho}_sample."""
        d_noise, length, n = self._device_noise(noise, length, n)
        d_out = torch.empty((n, length), dtype=torch.float32, device=self.device)
        _capi.check(self._h, fn(self._h, d_noise.data_ptr(), n, length, d_out.data_ptr(), *flags, self._stream()))
        return d_out.cpu().numpy()

    def update_ancilla(self, psi: np.ndarray, signal: np.ndarray, t: float) -> np.ndarray:
        """PsiCMPS._update_ancilla_psi for a batch of states (host arrays in, host array out)."""
        return self._ancilla(self._lib.cmps_psi_update_ancilla, "psi", psi, signal, t)

    def states(self) -> np.ndarray:
        """Normalised lab-frame psi after every step, [B, T-1, D] complex64 (psi_evolve_with_data)."""
        audio = self._audio
        if audio is None:
            raise RuntimeError("states() needs forward(save_for_bwd=True) first")
        B, T = audio.shape
        out = torch.empty((B, T - 1, self.D, 2), dtype=torch.float32, device=self.device)
        _capi.check(self._h, self._lib.cmps_psi_states(self._h, B, T, out.data_ptr(), self._stream()))
        return _from_interleaved(out)

    def sample(self, noise, length: Optional[int] = None, n: Optional[int] = None) -> np.ndarray:
        """PsiCMPS.sample for pre-drawn noise [length, n] (the reference's layout) -> waveforms [n, length].  ``noise`` may also be a device
        tensor [n, length] or a NoisePlan with ``length`` and ``n`` (`_device_noise`); so for every sampler entry below."""
        return self._sample(self._lib.cmps_psi_sample, noise, length, n)

    def _sample_primed(self, fn, prime: np.ndarray, noise, length, n, want_pred: bool, *flags):
        """Clips [n_prime, prime_T] up and the noise in (`_device_noise`), waveforms [n, length] and, with want_pred, the forced steps'
        predictions [n, prime_T - 1] down: `fn` is cmps_{psi,rho}_sample_primed."""
        prime = np.array(prime, dtype=np.float32, order="C")          # (a copy: torch wants a writable array)
        if prime.ndim != 2:
            raise ValueError("prime must be [n_prime, prime_T]")
        n_prime, prime_T = prime.shape
        d_noise, length, n = self._device_noise(noise, length, n)
        d_prime = torch.from_numpy(prime).to(self.device)
        d_out = torch.empty((n, length), dtype=torch.float32, device=self.device)
        d_pred = torch.empty((n, max(prime_T - 1, 0)), dtype=torch.float32, device=self.device) if want_pred else None
        _capi.check(self._h, fn(self._h, d_prime.data_ptr(), n_prime, prime_T, d_noise.data_ptr(), n, length, d_out.data_ptr(),
                                d_pred.data_ptr() if want_pred else None, *flags, self._stream()))
        out = d_out.cpu().numpy()
        return (out, d_pred.cpu().numpy()) if want_pred else out

    def sample_primed(self, prime: np.ndarray, noise, want_pred: bool = False, length: Optional[int] = None, n: Optional[int] = None):
        """cmps_psi_sample_primed: teacher-force the clips ``prime`` [n_prime, prime_T] (n_prime = n, or 1 for one clip shared by every
        path), then sample ``length`` steps with the pre-drawn ``noise`` [length, n] (the reference's layout, as `sample` takes it).
        Returns out [n, length] = A * running sum of the sampled increments (zero at the hand-over), or (out, pred [n, prime_T - 1])
        with want_pred: the model's expected increment of every forced step.  After set_params with T >= prime_T + length."""
        return self._sample_primed(self._lib.cmps_psi_sample_primed, prime, noise, length, n, want_pred)

    def _stream_state(self, bytes_fn, n: int, hint: str = "") -> torch.Tensor:
        """Device memory for the stream-state records of ``n`` paths: `bytes_fn` is cmps_{psi,rho}_stream_state_bytes."""
        nbytes = int(bytes_fn(self._h, int(n)))
        if nbytes == 0:
            raise ValueError(f"invalid path count for a stream: n={n}" + hint)
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _stream_paths(self, bytes_fn, state_in, state_out, n, n_audio) -> int:
        """The path count of a segment (``n``, else a state tensor's, else the audio's rows), with the state tensors checked against it."""
        if n is None:
            st = state_out if state_out is not None else state_in
            n = st.numel() // int(bytes_fn(self._h, 1)) if st is not None else n_audio
        n = int(n)
        for st in (state_in, state_out):
            if st is not None and not (st.is_cuda and st.dtype == torch.uint8 and st.is_contiguous()
                                       and st.numel() == int(bytes_fn(self._h, n))):
                raise ValueError(f"a stream state must be the tensor stream_state({n}) returned")
        return n

    def _audio_block(self, audio, least: int, rows: Optional[tuple] = None, need: str = ""):
        """A signal block [n_audio, forced + 1] of at least `least` columns (and, given `rows`, of one of these row counts) -> (device
        tensor, or None where no step is forced; n_audio; forced).  `need` is how the caller's error message names these conditions."""
        audio = np.array(audio, dtype=np.float32, order="C")           # (a copy: torch wants a writable array)
        if audio.ndim != 2 or audio.shape[1] < least or (rows is not None and audio.shape[0] not in rows):
            raise ValueError("audio must be [n_audio, forced + 1]" + need)
        forced = audio.shape[1] - 1
        return (torch.from_numpy(audio).to(self.device) if forced > 0 else None), audio.shape[0], forced

    def _running_loss(self, loss, shape: tuple) -> torch.Tensor:
        """The running loss of a scored stream on the device: zeros for None, else the host array of `shape`."""
        if loss is None:
            return torch.zeros(shape, dtype=torch.float32, device=self.device)
        if isinstance(loss, torch.Tensor):                             # (already there: the entry updates it in place)
            if not _is_tensor(loss, self.device, torch.float32, shape):
                raise ValueError(f"loss must be {list(shape)}")
            return loss
        loss = np.array(loss, dtype=np.float32, order="C")
        if loss.shape != shape:
            raise ValueError(f"loss must be {list(shape)}")
        return torch.from_numpy(loss).to(self.device)

    def _stream_launch(self, fn, state_in, state_out, k0, block, noise_args, n, length, want_pred, lead, *flags):
        """One segment behind its checks, for the paths of one model (`lead` = ()) or of every member of a bank ((M,)): (out lead + [n,
        length], pred lead + [n, forced] or None) down.  `fn` is cmps_{psi,rho,bank}_stream, `block` what `_audio_block` returned,
        `noise_args` what `fn` takes between forced and n, `flags` what it takes behind pred_dev."""
        d_audio, n_audio, forced = block
        d_out = torch.empty(lead + (n, length), dtype=torch.float32, device=self.device)
        d_pred = torch.empty(lead + (n, forced), dtype=torch.float32, device=self.device) if want_pred else None
        _capi.check(self._h, fn(self._h, _ptr(state_in), _ptr(state_out), int(k0), _ptr(d_audio), n_audio, forced, *noise_args, n, _ptr(d_out),
                                _ptr(d_pred), *flags, self._stream()))
        return d_out.cpu().numpy(), (d_pred.cpu().numpy() if want_pred else None)

    def _stream_call(self, fn, bytes_fn, state_in, state_out, k0, audio, noise, want_pred, n, length, *flags):
        """One segment of one model: the signal block [n_audio, forced + 1] up and the noise in (`_device_noise`; None: no sampled step),
        (out [n, length], pred [n, forced] or None) down.  `fn` / `bytes_fn` are cmps_{psi,rho}_stream / _stream_state_bytes, `flags` what
        `fn` takes behind pred_dev."""
        d_noise, block = None, (None, 1, 0)
        if noise is not None:
            d_noise, length, n = self._device_noise(noise, length, n)
        else:
            length = 0
        if audio is not None:
            block = self._audio_block(audio, 1)
        n = self._stream_paths(bytes_fn, state_in, state_out, n, block[1])
        return self._stream_launch(fn, state_in, state_out, k0, block, (_ptr(d_noise), length), n, length, want_pred, (), *flags)

    def stream_state(self, n: int) -> torch.Tensor:
        """Device memory for the stream-state records of ``n`` paths (cmps_psi_stream_state_bytes): opaque bytes, valid for this
        object's D and variant."""
        return self._stream_state(self._lib.cmps_psi_stream_state_bytes, n)

    def stream(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, noise, want_pred: bool = False,
               n: Optional[int] = None, length: Optional[int] = None):
        """cmps_psi_stream, one segment of a resumable scan on table rows k0 ..: ``audio`` [n_audio, forced + 1] (n_audio = n, or 1: one
        signal shared by every path; its first column is the sample before the segment's first forced step) or None, then ``noise``
        [length, n] (the reference's layout) or None.  ``state_in`` is None exactly at k0 = 0, ``state_out`` may be None or ``state_in``
        (tensors of `stream_state`).  Returns (out [n, length], pred [n, forced] with want_pred, else None).  The path count is taken from
        the noise, else from a state tensor, else from ``n`` or the audio's rows."""
        return self._stream_call(self._lib.cmps_psi_stream, self._lib.cmps_psi_stream_state_bytes, state_in, state_out, k0, audio, noise,
                                 want_pred, n, length)

    def _score_launch(self, fn, state_in, state_out, k0, block, want_nll, want_pred, n, loss, lead, *flags):
        """One scored segment behind its checks, for the paths of one model (`lead` = ()) or of every member of a bank ((M,)): the running
        loss up, (nll lead + [n, forced] or None, loss lead + [n], pred lead + [n, forced] or None) down.  `fn` is
        cmps_{psi,rho,bank}_stream_score, `block` what `_audio_block` returned, `flags` what `fn` takes behind pred_dev."""
        d_nll, d_loss, d_pred = self._score_device(fn, state_in, state_out, k0, block, want_nll, want_pred, n, loss, lead, *flags)
        return (d_nll.cpu().numpy() if want_nll else None), d_loss.cpu().numpy(), (d_pred.cpu().numpy() if want_pred else None)

    def _score_device(self, fn, state_in, state_out, k0, block, want_nll, want_pred, n, loss, lead, *flags):
        """`_score_launch` up to the downloads: (nll or None, the running loss behind the segment, pred or None) on the device."""
        d_audio, n_audio, forced = block
        d_loss = self._running_loss(loss, lead + (n,))
        d_nll = torch.empty(lead + (n, forced), dtype=torch.float32, device=self.device) if want_nll else None
        d_pred = torch.empty(lead + (n, forced), dtype=torch.float32, device=self.device) if want_pred else None
        _capi.check(self._h, fn(self._h, _ptr(state_in), _ptr(state_out), int(k0), _ptr(d_audio), n_audio, forced, n, _ptr(d_nll), _ptr(d_loss),
                                _ptr(d_pred), *flags, self._stream()))
        return d_nll, d_loss, d_pred

    def _stream_score_call(self, fn, bytes_fn, state_in, state_out, k0, audio, want_nll, want_pred, n, loss, *flags):
        """One scored segment of one model: the signal block [n_audio, forced + 1] and the running loss up, (nll [n, forced] or None, loss
        [n], pred [n, forced] or None) down.  `fn` / `bytes_fn` are cmps_{psi,rho}_stream_score / _stream_state_bytes, `flags` what `fn`
        takes behind pred_dev."""
        block = self._audio_block(audio, 2, need=" with forced >= 1")
        n = self._stream_paths(bytes_fn, state_in, state_out, n, block[1])
        return self._score_launch(fn, state_in, state_out, k0, block, want_nll, want_pred, n, loss, (), *flags)

    def stream_score(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, want_nll: bool = True,
                     want_pred: bool = False, n: Optional[int] = None, loss=None):
        """cmps_psi_stream_score, one scored segment of a resumable scan on table rows k0 ..: `stream`'s forced steps on ``audio``
        [n_audio, forced + 1] (forced >= 1) that also give the loss increment of every step.  ``loss`` [n] is the running loss to
        continue (not read at k0 = 0).  ``loss=None`` on a resumed segment (k0 > 0) starts the total again from zero: the caller keeps
        the total, the state record does not.  Returns (nll [n, forced] with want_nll else None, the running loss [n] behind the
        segment, pred [n, forced] with want_pred else None).  The states are `stream`'s: a scan may alternate between the two."""
        return self._stream_score_call(self._lib.cmps_psi_stream_score, self._lib.cmps_psi_stream_state_bytes, state_in, state_out, k0, audio,
                                       want_nll, want_pred, n, loss)

    # ------------------------------------------------------------------
    # A bank's streams (cmps_bank_stream*, cmps_rho_bank_stream*): `stream` / `stream_score` with a leading member axis on everything a
    # path writes or carries.  One driver per operation; `kind` is a key of BANK_SETTER and the prefix of the public methods' names.
    @staticmethod
    def _param_rows(D: int, members) -> np.ndarray:
        fields = layout.param_fields(D, with_A=True)
        return np.stack([layout.pack(fields, {**layout.split("R", p.R), "freqs": p.freqs, **layout.split("psi0", p.psi0), "A": p.A})
                         for p in members])

    def bank_set_params(self, members, B: int, T: int, train: bool = False):
        """cmps_bank_set_params_dev from host values: ``members`` is a list of EffectiveParams of one sigma and delta_t (A per member)."""
        params = torch.from_numpy(self._param_rows(self.D, members)).to(self.device)
        self.bank_set_params_dev(params, members[0].sigma, members[0].delta_t, B, T, train=train)
        self._bank.params = params

    def rho_bank_set_state(self, members, columns, B: int, T: int, train: bool = False):
        """cmps_rho_bank_set_state_dev from host values: ``members`` as for `bank_set_params` (psi0 is not read by a RhoCMPS scan),
        ``columns`` every member's phi [rank, D] complex (rho_0 = sum_a phi_a phi_a^dagger), one rank for all."""
        columns = [np.asarray(c) for c in columns]
        rank = columns[0].shape[0]
        if len(columns) != len(members) or any(c.shape != (rank, self.D) for c in columns):
            raise ValueError("columns must be one [rank, D] array per member, of one rank")
        fields = layout.phi_fields(self.D, rank)
        params = torch.from_numpy(self._param_rows(self.D, members)).to(self.device)
        phi = torch.from_numpy(np.stack([layout.pack(fields, layout.split("phi", c)) for c in columns])).to(self.device)
        self.rho_bank_set_state_dev(params, phi, rank, members[0].sigma, members[0].delta_t, B, T, train=train)
        self._bank.params = (params, phi)

    def _bank_stream_entries(self, kind: str):
        """(cmps_*_stream_state_bytes, cmps_*_stream, cmps_*_stream_score) of a bank of `kind`"""
        pre = "cmps_bank_stream" if kind == "bank" else "cmps_rho_bank_stream"
        return getattr(self._lib, pre + "_state_bytes"), getattr(self._lib, pre), getattr(self._lib, pre + "_score")

    def _bank_stream_state(self, kind: str, n: int) -> torch.Tensor:
        self._bank_of(kind, kind + "_stream_state")
        return self._stream_state(self._bank_stream_entries(kind)[0], n, f" (or the handle holds no {'PsiCMPS' if kind == 'bank' else 'RhoCMPS'} bank)")

    def _bank_stream(self, kind: str, state_in, state_out, k0, audio, noise, want_pred, n, length, n_noise):
        bytes_fn, fn, _ = self._bank_stream_entries(kind)
        M, n = self._bank_of(kind, kind + "_stream").M, int(n)
        self._stream_paths(bytes_fn, state_in, state_out, n, n)
        d_noise, rows, block = None, n, (None, 1, 0)
        if noise is not None:
            if n_noise is None and isinstance(noise, NoisePlan):
                n_noise = n                                                   # (an array brings its own path count)
            d_noise, length, rows = self._device_noise(noise, length, n_noise)
            if rows not in (n, M * n):
                raise ValueError(f"noise for {rows} paths fits neither n = {n} nor M n = {M * n}")
        else:
            length = 0
        if audio is not None:
            block = self._audio_block(audio, 1, (1, n, M * n), f" with n_audio in (1, {n}, {M * n}) and forced >= 0")
        return self._stream_launch(fn, state_in, state_out, k0, block, (_ptr(d_noise), rows, length), n, length, want_pred, (M,))

    def _bank_stream_score(self, kind: str, state_in, state_out, k0, audio, want_nll, want_pred, n, loss):
        bytes_fn, _, fn = self._bank_stream_entries(kind)
        M, n = self._bank_of(kind, kind + "_stream_score").M, int(n)
        self._stream_paths(bytes_fn, state_in, state_out, n, n)
        block = self._audio_block(audio, 2, (1, n, M * n), f" with n_audio in (1, {n}, {M * n}) and forced >= 1")
        return self._score_launch(fn, state_in, state_out, k0, block, want_nll, want_pred, n, loss, (M,))

    def _bank_stream_posterior(self, kind: str, state_in, state_out, k0, audio, n, loss, log_prior, inv_temp, threshold, decision, want_post,
                               want_nll, want_pred):
        """The scored segment of `_bank_stream_score` with nll kept on the device, then `bank_posterior` on it."""
        bytes_fn, _, fn = self._bank_stream_entries(kind)
        M, n = self._bank_of(kind, kind + "_stream_posterior").M, int(n)
        self._stream_paths(bytes_fn, state_in, state_out, n, n)
        block = self._audio_block(audio, 2, (1, n, M * n), f" with n_audio in (1, {n}, {M * n}) and forced >= 1")
        d_before = self._running_loss(loss, (M, n))
        d_nll, d_loss, d_pred = self._score_device(fn, state_in, state_out, k0, block, True, bool(want_pred), n, d_before.clone(), (M,))
        res = self.bank_posterior(d_nll, d_before, self.log_prior_tensor(log_prior), inv_temp, threshold, int(k0), decision, want_post)
        pred = None
        if want_pred == "lazy":
            pred = lambda: d_pred.cpu().numpy()                                        # noqa: E731
        elif want_pred:
            pred = d_pred.cpu().numpy()
        forced = block[2]
        h_rec, h_total, h_best, h_conf = np.split(res["pack"].cpu().numpy(), np.cumsum(res["pack_sizes"])[:-1])       # ONE download
        return {"best": h_best.view(np.int32).reshape(n, forced), "conf": h_conf.view(np.float32).reshape(n, forced),
                "loss": h_total.view(np.float32).reshape(M, n), "decision": h_rec.view(_capi.DECISION_REC) if h_rec.size else None,
                "carry": res["decision"], "post": res["post"].cpu().numpy() if want_post else None,
                "nll": d_nll.cpu().numpy() if want_nll else None, "pred": pred}

    def bank_stream_posterior(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio,
                              n: Optional[int] = None, loss=None, log_prior=None, inv_temp: float = 1.0, threshold: Optional[float] = None,
                              decision: Optional[torch.Tensor] = None, want_post: bool = False, want_nll: bool = False, want_pred=False) -> dict:
        """cmps_bank_stream_score, then cmps_bank_posterior on its nll where it lies: `bank_stream_score`'s segment judged as a classifier
        after every step.  ``loss`` [M, n] is the running loss to continue, ``log_prior`` [M] (host values or `log_prior_tensor`'s) or None,
        ``decision`` the "carry" of the previous segment's result or None (fresh records).  Only what is asked for comes down: {"best"
        int32 [n, forced], "conf" [n, forced], "loss" [M, n] behind the segment, "decision" (_capi.DECISION_REC [n], steps numbered
        from k0) or None without a threshold, "carry" (the records on the device), "post" / "nll" [M, n, forced] and "pred" on request,
        else None; want_pred="lazy": a function that downloads it}."""
        return self._bank_stream_posterior("bank", state_in, state_out, k0, audio, n, loss, log_prior, inv_temp, threshold, decision, want_post,
                                           want_nll, want_pred)

    def rho_bank_stream_posterior(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio,
                                  n: Optional[int] = None, loss=None, log_prior=None, inv_temp: float = 1.0,
                                  threshold: Optional[float] = None, decision: Optional[torch.Tensor] = None, want_post: bool = False,
                                  want_nll: bool = False, want_pred=False) -> dict:
        """`bank_stream_posterior` for a RhoCMPS bank (cmps_rho_bank_stream_score, then cmps_bank_posterior)."""
        return self._bank_stream_posterior("rho_bank", state_in, state_out, k0, audio, n, loss, log_prior, inv_temp, threshold, decision,
                                           want_post, want_nll, want_pred)

    def bank_stream_state(self, n: int) -> torch.Tensor:
        """Device memory for the stream-state records of ``n`` paths of every member (cmps_bank_stream_state_bytes)."""
        return self._bank_stream_state("bank", n)

    def bank_stream(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, noise, want_pred: bool = False,
                    n: Optional[int] = None, length: Optional[int] = None, n_noise: Optional[int] = None):
        """cmps_bank_stream: `stream` for every member of the bank at once.  ``audio`` [n_audio, forced + 1] with n_audio = 1 (one signal for
        everybody), n (one per path, shared by the members) or M n, or None; ``noise`` [length, n_noise] (the reference's layout), a device
        tensor [n_noise, length] or a NoisePlan -- drawn by ONE cmps_noise_fill over ``n_noise`` paths from path 0 -- with n_noise = n
        (every member hears the same noise) or M n, or None.  ``n`` is required.  Returns (out [M, n, length], pred [M, n, forced] with
        want_pred, else None)."""
        return self._bank_stream("bank", state_in, state_out, k0, audio, noise, want_pred, n, length, n_noise)

    def bank_stream_score(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, want_nll: bool = True,
                          want_pred: bool = False, n: Optional[int] = None, loss=None):
        """cmps_bank_stream_score: `stream_score` for every member of the bank at once; ``audio`` as in `bank_stream` (forced >= 1), ``loss``
        [M, n] the running loss to continue.  Returns (nll [M, n, forced] with want_nll else None, the running loss [M, n], pred
        [M, n, forced] with want_pred else None)."""
        return self._bank_stream_score("bank", state_in, state_out, k0, audio, want_nll, want_pred, n, loss)

    def rho_bank_stream_state(self, n: int) -> torch.Tensor:
        """`bank_stream_state` for a RhoCMPS bank (cmps_rho_bank_stream_state_bytes)."""
        return self._bank_stream_state("rho_bank", n)

    def rho_bank_stream(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, noise,
                        want_pred: bool = False, n: Optional[int] = None, length: Optional[int] = None, n_noise: Optional[int] = None):
        """cmps_rho_bank_stream: `bank_stream` for a RhoCMPS bank (after rho_bank_set_state*), every argument and result as there."""
        return self._bank_stream("rho_bank", state_in, state_out, k0, audio, noise, want_pred, n, length, n_noise)

    def rho_bank_stream_score(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, want_nll: bool = True,
                              want_pred: bool = False, n: Optional[int] = None, loss=None):
        """cmps_rho_bank_stream_score: `bank_stream_score` for a RhoCMPS bank, every argument and result as there."""
        return self._bank_stream_score("rho_bank", state_in, state_out, k0, audio, want_nll, want_pred, n, loss)

    # ------------------------------------------------------------------
    # legacy AudioMPS arithmetic
    # ------------------------------------------------------------------
    def legacy_set_params(self, R: np.ndarray, Q: np.ndarray, delta_t: float, B: int, T: int, train: bool = True):
        self._legacy_buf, ptrs = self._upload(layout.legacy_param_fields(self.D), {"R": R, **layout.split("Q", Q)})
        _capi.check(self._h, self._lib.cmps_legacy_set_params(
            self._h, *ptrs, float(delta_t), int(T), int(B), *self._psi_workspace(B, T, train, reuse=False), self._stream()))
        self._configured(B, T, "legacy")

    def legacy_forward(self, audio: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        return self._forward(self._lib.cmps_legacy_loss_fwd, audio, save_for_bwd)

    def legacy_backward(self) -> torch.Tensor:
        self._legacy_grad = self._backward(self._lib.cmps_legacy_loss_bwd, self._legacy_grad,
                                           layout.size(layout.legacy_grad_fields(self.D)), "legacy_")
        return self._legacy_grad

    # ------------------------------------------------------------------
    # RhoCMPS: the density matrix carried as its `rank` columns
    # ------------------------------------------------------------------
    def rho_grad_size(self, rank: int) -> int:
        return grad_size(self.D, rank)

    def rho_set_state(self, phi: np.ndarray, B: int, T: int, train: bool = True):
        """cmps_rho_set_state: phi [rank, D] complex, rho_0 = sum_a phi_a phi_a^dagger.  After set_params."""
        phi = np.asarray(phi)
        r, D = phi.shape
        if D != self.D:
            raise ValueError("phi has the wrong bond dimension")
        ws_ptr, ws_bytes = self._rho_workspace(B, T, train, r)
        self._phi_buf, ptrs = self._upload(layout.phi_fields(D, r), layout.split("phi", phi))
        _capi.check(self._h, self._lib.cmps_rho_set_state(
            self._h, *ptrs, r, int(T), int(B), self._ws_flags(train), ws_ptr, ws_bytes, self._stream()))
        self._rho_rank = r

    def rho_set_state_dev(self, phi: torch.Tensor, rank: int, B: int, T: int, train: bool = True):
        """cmps_rho_set_state with the columns read from the device buffer `phi` = phi_re [rank D] | phi_im [rank D] that
        cmps_rho_apply_step wrote -- no upload, no synchronisation.  After set_params*."""
        r, D = int(rank), self.D
        if not (phi.is_cuda and phi.dtype == torch.float32 and phi.is_contiguous() and phi.numel() == 2 * r * D):
            raise ValueError("phi must be a contiguous float32 CUDA tensor of 2 rank D elements")
        ws_ptr, ws_bytes = self._rho_workspace(B, T, train, r)
        self._phi_buf = phi
        _capi.check(self._h, self._lib.cmps_rho_set_state(
            self._h, *layout.pointers(phi.data_ptr(), layout.phi_fields(D, r)), r, int(T), int(B), self._ws_flags(train), ws_ptr, ws_bytes,
            self._stream()))
        self._rho_rank = r

    def rho_forward(self, audio: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        return self._forward(self._lib.cmps_rho_loss_fwd, audio, save_for_bwd, slot="_rho_loss")

    def rho_backward(self) -> torch.Tensor:
        self._rho_grad = self._backward(self._lib.cmps_rho_loss_bwd, self._rho_grad, self.rho_grad_size(self._rho_rank), "rho_")
        return self._rho_grad

    def rho_loss_and_grad_sums(self, audio: torch.Tensor):
        loss = self.rho_forward(audio, save_for_bwd=True)
        return loss, self.rho_backward()

    def rho_update_ancilla(self, rho: np.ndarray, signal: np.ndarray, t: float) -> np.ndarray:
        """RhoCMPS._update_ancilla_rho for a batch of matrices [B, D, D] (host in, host out)."""
        return self._ancilla(self._lib.cmps_rho_update_ancilla, "rho", rho, signal, t)

    def rho_sample(self, noise, save_states: bool = False, length: Optional[int] = None, n: Optional[int] = None) -> np.ndarray:
        """RhoCMPS.sample for pre-drawn noise [length, n] -> waveforms [n, length]."""
        return self._sample(self._lib.cmps_rho_sample, noise, length, n, 1 if save_states else 0)

    def rho_sample_primed(self, prime: np.ndarray, noise, want_pred: bool = False, save_states: bool = False,
                          length: Optional[int] = None, n: Optional[int] = None):
        """cmps_rho_sample_primed: `sample_primed` for RhoCMPS, from the columns of rho_set_state.  save_states keeps the columns of all
        prime_T - 1 + length steps for rho_states (a train=True rho workspace with T >= prime_T + length)."""
        return self._sample_primed(self._lib.cmps_rho_sample_primed, prime, noise, length, n, want_pred, 1 if save_states else 0)

    def rho_stream_state(self, n: int) -> torch.Tensor:
        """`stream_state` for RhoCMPS (cmps_rho_stream_state_bytes): valid for this object's D and variant and the rank of rho_set_state,
        which must have been called."""
        return self._stream_state(self._lib.cmps_rho_stream_state_bytes, n, " (or rho_set_state has not been called)")

    def rho_stream(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, noise, want_pred: bool = False,
                   n: Optional[int] = None, save_states: bool = False, length: Optional[int] = None):
        """cmps_rho_stream: `stream` for RhoCMPS, from the columns of rho_set_state (states of `rho_stream_state`).  save_states keeps the
        columns of this segment's steps for rho_states(n, forced + length): a train=True rho workspace whose T - 1 is at least that many
        steps; the rho workspace's T is a stash capacity only and may be smaller than set_params's."""
        return self._stream_call(self._lib.cmps_rho_stream, self._lib.cmps_rho_stream_state_bytes, state_in, state_out, k0, audio, noise,
                                 want_pred, n, length, 1 if save_states else 0)

    def rho_stream_score(self, state_in: Optional[torch.Tensor], state_out: Optional[torch.Tensor], k0: int, audio, want_nll: bool = True,
                         want_pred: bool = False, n: Optional[int] = None, loss=None, save_states: bool = False):
        """cmps_rho_stream_score: `stream_score` for RhoCMPS, from the columns of rho_set_state (states of `rho_stream_state`, shared with
        `rho_stream`: a scan may alternate between the two).  Returns (nll, loss, pred) as `stream_score` does.  save_states keeps the
        columns of this segment's steps for rho_states(n, forced), as in `rho_stream`."""
        return self._stream_score_call(self._lib.cmps_rho_stream_score, self._lib.cmps_rho_stream_state_bytes, state_in, state_out, k0, audio,
                                       want_nll, want_pred, n, loss, 1 if save_states else 0)

    def rho_states(self, B: int, steps: int, want_rho: bool = True, want_purity: bool = False):
        """Lab-frame rho [B, steps, D, D] and/or purity [B, steps] of the last saved scan."""
        D = self.D
        d_rho = torch.empty((B, steps, D, D, 2), dtype=torch.float32, device=self.device) if want_rho else None
        d_pur = torch.empty((B, steps), dtype=torch.float32, device=self.device) if want_purity else None
        _capi.check(self._h, self._lib.cmps_rho_states(
            self._h, B, steps, d_rho.data_ptr() if want_rho else None, d_pur.data_ptr() if want_purity else None,
            self._stream()))
        out = ([_from_interleaved(d_rho)] if want_rho else []) + ([d_pur.cpu().numpy()] if want_purity else [])
        return out[0] if len(out) == 1 else tuple(out)
