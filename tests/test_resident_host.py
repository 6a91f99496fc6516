"""The owner of device-resident optimiser state (audio_mps_amd/resident.py) without a GPU and without a kernel: upload, download and the
ownership protocol with the models, driven through a minimal subclass whose "device step" adds a constant to ``_dev["vars"]`` on torch
CPU tensors.  Every case runs for one flat member (the form and clean-state rule of Trainer) and three stacked ones (those of
BankTrainer), for PsiCMPS and RhoCMPS."""
import gc
import weakref

import numpy as np
import pytest

from audio_mps_amd import HParams, PsiCMPS, RhoCMPS, layout
from audio_mps_amd.bank import BankTrainer
from audio_mps_amd.resident import ResidentState
from audio_mps_amd.train import AdamOptimizer, Trainer

from _util import OracleBackend

D, RANK = 4, 2
CASES = [(form, kind) for form in ("flat", "stacked") for kind in ("psi", "rho")]


@pytest.fixture(scope="module", autouse=True)
def _only_this_modules_objects_are_collected():
    """The gc.collect() calls below are full collections; with everything that exists before this module's tests parked in the permanent
    generation they scan what the tests made instead of every object of the imported libraries (a third of a second each)."""
    gc.collect()
    gc.freeze()
    yield
    gc.unfreeze()


class Owner(ResidentState):
    def __init__(self, models, stacked, sync_clean=None):
        self.STACKED = stacked
        self.SYNC_CLEAN = (not stacked) if sync_clean is None else sync_clean      # (default: the rule of the class of that form)
        self.opts = [AdamOptimizer() for _ in models]
        self._resident(list(zip(models, self.opts)), D, RANK if isinstance(models[0], RhoCMPS) else 0)

    def state(self):
        if self._dev is None:
            self._upload("cpu")
        return self._dev

    def step(self, c=1.0):
        self.state()["vars"] += c
        self._mark_dirty()


def make_model(kind, seed):
    hp = HParams(minibatch_size=2, bond_dim=D, initial_rank=RANK)
    return (RhoCMPS if kind == "rho" else PsiCMPS)(hp, seed=seed, backend=OracleBackend(D))


def make(form, kind, sync_clean=None):
    models = [make_model(kind, 11 + s) for s in range(3 if form == "stacked" else 1)]
    return models, Owner(models, form == "stacked", sync_clean)


def snapshot(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rows(owner, slot):
    """The members' rows of a state tensor as numpy arrays."""
    t = owner._dev[slot].numpy()
    return list(t) if owner.STACKED else [t]


def test_the_two_classes_keep_their_forms_and_clean_state_rules():
    assert not Trainer.STACKED and Trainer.SYNC_CLEAN and BankTrainer.STACKED and not BankTrainer.SYNC_CLEAN


@pytest.mark.parametrize("form,kind", CASES)
def test_pack_then_unpack_round_trips_every_variable_and_slot_bit_for_bit(form, kind):
    models, own = make(form, kind)
    rng = np.random.default_rng(5)
    want = []
    for mo, opt in own._members:
        for slot in (opt.m, opt.v):
            for k, v in mo.variables.items():
                slot[k] = rng.standard_normal(v.shape).astype(np.float32)
        want.append((snapshot(mo.variables), snapshot(opt.m), snapshot(opt.v)))
    st = own.state()
    n = layout.size(layout.var_fields(*own._shape))
    lead = (len(models),) if own.STACKED else ()
    assert all(tuple(st[s].shape) == lead + (n,) for s in ("vars", "m", "v")) and tuple(st["losses"].shape) == lead + (2,)
    assert ("phi" in st) == (kind == "rho") and st["params"].dim() == len(lead) + 1 and not own._dirty
    for mo, opt in own._members:                                  # the host copies are rewritten, not just left alone
        for d in (mo._variables, opt.m, opt.v):
            for k in list(d):
                dict.__setitem__(d, k, np.full_like(d[k], np.nan))
    own._mark_dirty()
    own.sync_to_host()
    for (mo, opt), (vars0, m0, v0) in zip(own._members, want):
        for got, ref in ((mo.variables, vars0), (opt.m, m0), (opt.v, v0)):
            assert set(got) == set(ref)
            for k in ref:
                assert same(got[k], ref[k]), k


@pytest.mark.parametrize("form,kind", CASES)
def test_a_missing_slot_uploads_as_zeros(form, kind):
    models, own = make(form, kind)
    rx = np.full((D, D), 3.0, np.float32)
    own.opts[0].m["Rx"] = rx                                      # one slot of one member present, everything else missing
    own.state()
    fields = layout.var_fields(*own._shape)
    for i, row in enumerate(rows(own, "m")):
        for k, a in layout.unpack(fields, row).items():
            assert np.array_equal(a, rx if (i == 0 and k == "Rx") else np.zeros_like(a)), (i, k)
    assert all(not row.any() for row in rows(own, "v"))


@pytest.mark.parametrize("read", ["variables", "R"])
@pytest.mark.parametrize("form,kind", CASES)
def test_the_first_read_after_a_step_syncs_and_the_second_copies_nothing(form, kind, read):
    models, own = make(form, kind)
    before = [snapshot(mo.variables) for mo in models]
    own.step(0.5)
    assert own._dirty and all(mo._dirty_owner is own and mo._owner() is own for mo in models)
    if read == "R":
        twin = make_model(kind, 0)
        for k, v in before[0].items():
            twin.variables[k] = v + np.float32(0.5)
        assert same(models[0].R, twin.R)
    else:
        models[0].variables
    assert not own._dirty and all(mo._dirty_owner is None and mo._owner() is own for mo in models)
    own._dev["vars"].fill_(float("nan"))                          # a second read that copied would show this
    for mo, b in zip(models, before):
        for k, v in b.items():
            assert same(mo.variables[k], v + np.float32(0.5)), k
    assert own._dev is not None and not own._dirty


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("form,kind", CASES)
def test_an_assignment_brings_the_rest_back_and_drops_the_state(form, kind, inplace):
    models, own = make(form, kind)
    before = [snapshot(mo.variables) for mo in models]
    own.step(2.0)
    if inplace:
        models[-1].variables["Rx"] *= np.float32(0.5)              # (reads the stepped value, assigns the product)
        new_rx = (before[-1]["Rx"] + np.float32(2.0)) * np.float32(0.5)
    else:
        new_rx = np.full((D, D), 7.0, np.float32)
        models[-1].variables["Rx"] = new_rx
    assert own._dev is None and not own._dirty and all(mo._dirty_owner is None for mo in models)
    for i, (mo, b) in enumerate(zip(models, before)):
        for k, v in b.items():
            want = new_rx if (mo is models[-1] and k == "Rx") else v + np.float32(2.0)
            assert same(mo.variables[k], want), (i, k)
    fields = layout.var_fields(*own._shape)                       # the next upload starts from the host values
    own.state()
    for mo, row in zip(models, rows(own, "vars")):
        for k, a in layout.unpack(fields, row).items():
            assert np.array_equal(a, mo._variables[k]), k


@pytest.mark.parametrize("form,kind", CASES)
def test_a_clean_owner_is_collectable_at_once(form, kind):
    models, own = make(form, kind)
    own.state()
    ref = weakref.ref(own)
    assert all(mo._owner() is own and mo._dirty_owner is None for mo in models)
    del own
    gc.collect()
    assert ref() is None and all(mo._owner() is None for mo in models)
    models[0].variables["Rx"] = models[0].variables["Rx"]        # (reads and writes with a dead owner are plain dict accesses)


@pytest.mark.parametrize("form,kind", CASES)
def test_a_dirty_owner_lives_until_its_steps_have_been_read(form, kind):
    models, own = make(form, kind)
    before = [snapshot(mo.variables) for mo in models]
    own.step(1.5)
    ref = weakref.ref(own)
    del own
    gc.collect()
    assert ref() is not None and all(mo._dirty_owner is ref() for mo in models)
    for mo, b in zip(models, before):
        for k, v in b.items():
            assert same(mo.variables[k], v + np.float32(1.5)), k
    assert all(mo._dirty_owner is None for mo in models)
    gc.collect()
    assert ref() is None and all(mo._owner() is None for mo in models)


@pytest.mark.parametrize("sync_clean", [True, False])
@pytest.mark.parametrize("form,kind", CASES)
def test_sync_to_host_on_a_live_clean_state(form, kind, sync_clean):
    """Trainer's rule (SYNC_CLEAN): the copy is made, and never-stepped Adam slots become explicit zeros; BankTrainer's: nothing is touched."""
    models, own = make(form, kind, sync_clean)
    own.state()
    held = [mo._variables["Rx"] for mo in models]
    own.sync_to_host()
    for mo, opt, rx in zip(models, own.opts, held):
        if sync_clean:
            assert set(opt.m) == set(opt.v) == set(mo._variables) and all(not a.any() for a in list(opt.m.values()) + list(opt.v.values()))
            assert mo._variables["Rx"] is not rx and same(mo._variables["Rx"], rx)
        else:
            assert opt.m == {} and opt.v == {} and mo._variables["Rx"] is rx
    assert own._dev is not None and not own._dirty
    own.step(1.0)                                                  # after a step both rules copy
    own.sync_to_host()
    assert all(same(mo._variables["Rx"], rx + np.float32(1.0)) and set(opt.m) == set(mo._variables) for mo, opt, rx in zip(models, own.opts, held))


def test_sync_and_drop_without_a_state_do_nothing():
    models, own = make("flat", "psi")
    own.sync_to_host()
    own.drop_device_state()
    own._lazy_sync()
    assert own._dev is None and own.opts[0].m == {} and models[0]._owner() is None


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_forget_drops_the_state_without_reading_it_back(kind):
    models, own = make("stacked", kind)
    before = [snapshot(mo.variables) for mo in models]
    own.step(1.0)
    own._forget()
    assert own._dev is None and not own._dirty and all(mo._dirty_owner is None for mo in models)
    assert all(same(mo.variables[k], v) for mo, b in zip(models, before) for k, v in b.items())


@pytest.mark.parametrize("kind", ["psi", "rho"])
def test_a_stacked_owner_takes_a_member_back_from_a_plain_one(kind):
    models, bank = make("stacked", kind)
    before = snapshot(models[1].variables)
    bank.step(1.0)
    plain = Owner([models[1]], stacked=False)
    plain.step(2.0)                                                # its upload reads models[1].variables: the bank's step comes back first
    assert not bank._dirty and models[1]._owner() is plain and models[1]._dirty_owner is plain and models[0]._owner() is bank
    assert same(rows(plain, "vars")[0], rows(bank, "vars")[1] + np.float32(2.0))
    plain.sync_to_host()
    assert models[1]._dirty_owner is None and models[1]._owner() is plain
    assert same(models[1]._variables["Rx"], before["Rx"] + np.float32(3.0))
    bank.step(1.0)
    assert all(mo._owner() is bank and mo._dirty_owner is bank for mo in models)
    models[1].variables
    assert not bank._dirty and all(mo._dirty_owner is None for mo in models)
