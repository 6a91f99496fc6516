"""include/cmps.h: everything runs "asynchronously on the caller's stream".  Every other test runs on the default stream, where a helper
kernel or a hipMemsetAsync launched on stream 0 instead of `stream` is silently correct; for a caller on its own non-blocking stream it
is a race.  Here, per family:

  1. every buffer is created while synchronised (tests/_guard.py, a queued Driver); the inputs hold the NaN pattern;
  2. a fresh torch.cuda.Stream() is kept busy by a chain of large matmuls (the producer); behind it, on that stream, the workspaces
     are overwritten with the pattern once more and the real inputs are copied in; an event is recorded behind the copies;
  3. all library calls of the case are made with `stream` = that side stream;
  4. immediately after the last call returns the event must NOT be complete: the inputs were still poison while every call was
     enqueued, so anything the library put on another stream read NaN, or wrote before the producer finished (and was overwritten).
     An event that is already complete proves nothing: the case FAILS;
  5. after synchronising, the results are bit-identical to the same case on the default stream and every guard zone is intact.

cmps_psi_grad_status waits for `stream` by contract, so it is called behind step 4.  One side stream, no graph capture.
"""
import time

import numpy as np
import pytest
import torch

import _guard as G
import _primed_ref as PR
import _rho_primed_ref as RPR
import _stream_ref as SR
from test_gpu_memory_contract import AUTO, BLOCK, WAVE, sampler_model, synthetic_grad_sums

pytestmark = pytest.mark.gpu

PRODUCER_MS = 250.0          # how long the side stream is kept busy: see INTEGRATION.md ("Memory contract") for the measured enqueue times
MATMUL_N = 8192


@pytest.fixture(scope="module")
def producer():
    """A chain of MATMUL_N^3 float32 matmuls, timed once with HIP events and sized to PRODUCER_MS."""
    dev = torch.device("cuda", torch.cuda.current_device())
    a = torch.full((MATMUL_N, MATMUL_N), 1.0 / MATMUL_N, dtype=torch.float32, device=dev)
    b, c = a.clone(), torch.empty_like(a)
    torch.matmul(a, b, out=c)                                     # (the first call loads the kernel)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        torch.matmul(a, b, out=c)
    e1.record()
    torch.cuda.synchronize()
    one = e0.elapsed_time(e1) / 4
    count = max(4, int(np.ceil(PRODUCER_MS / one)))
    print(f"producer: one {MATMUL_N}^3 float32 matmul takes {one:.2f} ms; {count} of them keep the side stream busy for {count * one:.0f} ms")

    def run():
        for _ in range(count):
            torch.matmul(a, b, out=c)
    yield run
    del a, b, c


def on_side_stream(producer, D, variant, build, status=False, extra=()):
    """build(drv) -> result names.  The case on the default stream (eager, checked after every call), then on a busy side stream."""
    ref_drv = G.Driver(D, G.NAN_FILL, variant)
    names = list(build(ref_drv)) + list(extra)
    if status:
        assert ref_drv.grad_status() == (0, 0)
    ref_drv.finish()
    ref = ref_drv.result(names)

    drv = G.Driver(D, G.NAN_FILL, variant, queue=True)
    drv.hints = dict(ref_drv.hints)
    assert list(build(drv)) + list(extra) == names
    for g in drv.pending:                                          # the inputs are poison until the side stream's copies run
        assert bool(g.untouched_mask(torch.uint8).all())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        t_all = time.perf_counter()
        producer()
        for name, g in drv.bufs.items():
            if name.endswith("ws"):
                g.refill_payload()                                 # whatever an early (wrong-stream) launch wrote there is gone again
        drv.flush_inputs()
        done.record(side)
        drv.stream = side.cuda_stream
        t0 = time.perf_counter()
        drv.run_queue()
        enqueue_ms, host_ms = 1e3 * (time.perf_counter() - t0), 1e3 * (time.perf_counter() - t_all)
        still_busy = not done.query()
    print(f"D={D} variant={variant}: {len(drv.calls)} calls enqueued in {enqueue_ms:.2f} ms; {host_ms:.2f} ms on the host since the producer's first launch")
    assert still_busy, "the inputs' copies had completed before the last call returned: the case proved nothing"
    torch.cuda.synchronize()
    if status:
        assert drv.grad_status() == (0, 0)
    drv.finish()
    G.same_bits(drv.result(names), ref, "side stream against the default stream")
    assert ref_drv.calls == drv.calls
    drv.close()
    ref_drv.close()


@pytest.mark.parametrize("family,variant,D", [("wave16", AUTO, 8), ("wave", WAVE, 32), ("wide", AUTO, 48), ("block", BLOCK, 48)])
def test_psi_on_the_callers_stream(producer, family, variant, D):
    B, T = 3, 66
    audio = G.contract_audio(B, T)

    def build(drv):
        G.set_params(drv, G.psi_model(D, B), B, T)
        return G.psi_scan(drv, audio)
    on_side_stream(producer, D, variant, build, status=True)


def test_legacy_on_the_callers_stream(producer):
    from _util import make_audio
    D, B, T = 12, 3, 65
    m = G.legacy_model(D, B)
    audio = make_audio(B, T, m.delta_t, 303, noise=0.05)

    def build(drv):
        G.legacy_set_params(drv, m, B, T)
        return G.legacy_scan(drv, audio)
    on_side_stream(producer, D, AUTO, build)


@pytest.mark.parametrize("D,rank", [(32, 32), (40, 5)])
def test_rho_on_the_callers_stream(producer, D, rank):
    B, T = 3, 40
    audio = G.contract_audio(B, T)

    def build(drv):
        m = G.rho_model(D, rank, B)
        G.set_params(drv, m, B, T, train=False)
        G.rho_set_state(drv, m, B, T)
        return G.rho_scan(drv, audio)
    on_side_stream(producer, D, AUTO, build)


def test_psi_sampler_on_the_callers_stream(producer):
    D, n, P, length = 32, 3, 65, 70
    prime, noise = PR.case_inputs(D, P, length, n)

    def build(drv):
        G.set_params(drv, sampler_model(D, n), n, P + 1 + length, train=False)
        return G.sample(drv, "cmps_psi_sample_primed", noise, prime=prime) + G.sample(drv, "cmps_psi_sample", noise, tag="_plain")
    on_side_stream(producer, D, WAVE, build)


def test_rho_sampler_on_the_callers_stream(producer):
    D, rank, n, P, length = 32, 32, 2, 65, 70
    prime, noise = RPR.case_inputs(D, rank, P, length, n)

    def build(drv):
        m = RPR.case_model(D, rank, backend=False)
        G.set_params(drv, m, n, P + 1 + length, train=False)
        G.rho_set_state(drv, m, n, P + 1 + length, train=True)
        names = G.sample(drv, "cmps_rho_sample_primed", noise, prime=prime, flags=(1,)) + G.rho_states(drv, n, P + length)
        return names + G.sample(drv, "cmps_rho_sample", noise, flags=(0,), tag="_plain")
    on_side_stream(producer, D, AUTO, build)


@pytest.mark.parametrize("model", ["psi", "rho"])
def test_stream_segments_on_the_callers_stream(producer, model):
    plan, n = ((65, 3), (2, 70)), 2
    D, rank = (48, 0) if model == "psi" else (40, 5)
    clip, noise = SR.case_inputs(D, plan, n)
    F, L = SR.plan_steps(plan)

    def build(drv):
        if model == "psi":
            G.set_params(drv, sampler_model(D, n), n, F + L + 1, train=False)
            return G.stream_plan(drv, "cmps_psi_stream", "cmps_psi_stream_state_bytes", plan, clip, noise, n, null_pred_at=-1)[0]
        m = RPR.case_model(D, rank, backend=False)
        G.set_params(drv, m, n, F + L + 1, train=False)
        G.rho_set_state(drv, m, n, F + L + 1, train=False)
        return G.stream_plan(drv, "cmps_rho_stream", "cmps_rho_stream_state_bytes", plan, clip, noise, n, flags=(0,), null_pred_at=-1)[0]
    on_side_stream(producer, D, AUTO, build, extra=("state",))


@pytest.mark.parametrize("D,rank", [(33, 0), (33, 40)])
def test_apply_step_on_the_callers_stream(producer, D, rank):
    m = G.rho_model(D, rank) if rank else G.psi_model(D)
    gs = synthetic_grad_sums(D, rank)
    on_side_stream(producer, D, AUTO, lambda drv: G.apply_step(drv, m, gs, rank))


def test_params_dev_and_ancilla_on_the_callers_stream(producer):
    """cmps_psi_apply_step(grad_sums = NULL) -> cmps_set_params_dev -> forward, and the two one-step entries."""
    D, B, T = 33, 3, 66
    m = G.psi_model(D, B)
    audio = G.contract_audio(B, T)
    rng = np.random.default_rng(D)
    psi = (rng.standard_normal((B, D)) + 1j * rng.standard_normal((B, D))).astype(np.complex64)
    rho = (rng.standard_normal((B, D, D)) + 1j * rng.standard_normal((B, D, D))).astype(np.complex64)
    signal = (0.01 * rng.standard_normal(B)).astype(np.float32)

    def build(drv):
        names = G.apply_step(drv, m, None)
        n = G.ws_bytes(drv, B, T, True)
        drv.new("ws", n)
        p = m.effective_params()
        drv.call("cmps_set_params_dev", drv.bufs["params_out"], float(p.sigma), float(p.delta_t), T, B, 1, drv.bufs["ws"], n)
        names += G.psi_scan(drv, audio)
        names += G.ancilla(drv, "cmps_psi_update_ancilla", psi, signal, 0.37, tag="_psi")
        return names + G.ancilla(drv, "cmps_rho_update_ancilla", rho, signal, 0.37, tag="_rho")
    on_side_stream(producer, D, AUTO, build, status=True)
