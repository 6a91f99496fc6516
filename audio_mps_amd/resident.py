"""Device-resident optimiser state and its ownership protocol with the models: what Trainer(device_step=True) and BankTrainer share.

While variables and Adam slots live in torch tensors on a device, the host copies (model.variables, opt.m, opt.v) are stale.  The owner
of those tensors is known to every model it trains, so that the model can ask for them (CMPS.variables, _VarDict.__setitem__):

  model._device_owner   weak reference to the owner, from the upload on: an owner nobody holds any more is collected at once
  model._dirty_owner    the owner itself, from a device step until the steps are back on the host: an owner that goes out of scope in
                        between stays alive until the first read of model.variables has brought them back
  reading  model.variables       -> owner._lazy_sync(): one device -> host copy, only if steps are outstanding
  assigning model.variables[k]   -> owner.drop_device_state(): everything else comes back, the device copy is forgotten, and the next
                                    device step uploads the host values again

Nothing here knows a kernel or a backend: the subclass runs the steps on ``_dev`` and calls ``_mark_dirty()`` after each.
"""
from __future__ import annotations

import weakref

import numpy as np

from . import layout


class ResidentState:
    """``_resident(members, D, rank)`` in the subclass's __init__: ``members`` is the list of (model, optimizer) whose variables and Adam
    slots the state holds.  ``_dev`` is None or a plain dict of tensors: "vars", "m", "v" (layout.var_fields), "params", "losses" [2] and,
    with ``rank``, "phi" -- flat, or (STACKED) with a leading axis over the members.  ``_dirty``: a step has run since the last download."""

    STACKED = False               # one row per member ([M, n]) instead of one flat member ([n])
    SYNC_CLEAN = False            # sync_to_host() copies a live state that no step has changed as well (see sync_to_host)

    def _resident(self, members, D: int, rank: int):
        self._members, self._shape = list(members), (int(D), int(rank))
        self._dev = None
        self._dirty = False

    # -- host -> device ---------------------------------------------------------------------------------
    def _upload(self, device) -> dict:
        """Pack every member's variables and Adam slots (a missing slot starts at zero), allocate the rest, take the models."""
        import torch
        D, rank = self._shape
        fields = layout.var_fields(D, rank)
        rows = {"vars": [], "m": [], "v": []}
        for model, opt in self._members:
            variables = model.variables                            # (the property: another owner's outstanding steps come back first)
            zeros = {k: np.zeros_like(variables[k]) for k in layout.var_order(rank)}
            for slot, src in (("vars", variables), ("m", opt.m), ("v", opt.v)):
                rows[slot].append(layout.pack(fields, {**zeros, **src}))
        lead = (len(self._members),) if self.STACKED else ()
        st = {slot: torch.from_numpy(np.stack(r) if self.STACKED else r[0]).to(device) for slot, r in rows.items()}
        st["params"] = torch.empty(lead + (layout.size(layout.param_fields(D, with_A=True)),), dtype=torch.float32, device=device)
        st["losses"] = torch.zeros(lead + (2,), dtype=torch.float32, device=device)
        if rank:
            st["phi"] = torch.empty(lead + (layout.size(layout.phi_fields(D, rank)),), dtype=torch.float32, device=device)
        self._dev, self._dirty = st, False
        self._own(dirty=False)                                     # model.variables now asks this owner first
        return st

    # -- the protocol -------------------------------------------------------------------------------------
    def _own(self, dirty: bool):
        for model, _ in self._members:
            model._device_owner = weakref.ref(self)
            if dirty:
                model._dirty_owner = self

    def _mark_dirty(self):
        """After every device step: the host copies are stale, and until they are synced the models keep this owner alive.  (Ownership
        is asserted again as well: another owner, such as a plain Trainer of a bank's member, may have taken a model in between.)"""
        self._dirty = True
        self._own(dirty=True)

    def _release(self):
        """Not dirty any more: the models drop their strong reference to this owner (the weak one stays)."""
        for model, _ in self._members:
            if model._dirty_owner is self:
                model._dirty_owner = None

    def _lazy_sync(self):
        """Called by model.variables: device state -> host copies if a device step has run since the last sync."""
        if self._dirty:
            self.sync_to_host()

    def sync_to_host(self):
        """Device-resident state -> every member's model.variables and Adam slots (checkpoints, sampling, inspection)."""
        # SYNC_CLEAN: a Trainer copies a never-stepped state too, which turns missing Adam slots into explicit zeros (a checkpoint's adam/m/*
        # keys); a bank leaves its members' host state alone until a step has changed it
        if self._dev is None or not (self._dirty or self.SYNC_CLEAN):
            return
        fields = layout.var_fields(*self._shape)
        host = {slot: self._dev[slot].cpu().numpy() for slot in ("vars", "m", "v")}
        for i, (model, opt) in enumerate(self._members):
            for slot, dst in (("vars", model._variables), ("m", opt.m), ("v", opt.v)):
                for k, a in layout.unpack(fields, host[slot][i] if self.STACKED else host[slot]).items():
                    dict.__setitem__(dst, k, np.asarray(a, dtype=np.float32).copy())     # (past _VarDict: nothing is being assigned)
        self._dirty = False
        self._release()

    def drop_device_state(self):
        """Bring the device-resident state back and forget it: the next device step uploads variables and Adam slots from the host
        again (called when an entry of model.variables is assigned; nothing to do when no state is live)."""
        if self._dev is not None:
            self.sync_to_host()
            self._forget()

    def _forget(self):
        """Forget the device copy WITHOUT reading it back (restore: the host state has just been replaced)."""
        self._dev = None
        self._dirty = False
        self._release()
