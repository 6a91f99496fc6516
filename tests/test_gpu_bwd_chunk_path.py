"""The unrolled full-chunk path of the two-wave reverse scan's chain wave (cmps_wave_bwd2.hip).

A 32-step chunk that is full, starts octet-aligned and has a chunk below it runs with compile-time step numbers on a PsiCMPS stash of
normalised rows; the top chunk, the steps above the first aligned octet, chunk 0, step 0, RhoCMPS virtual clips and (y, H y) rows keep
the octet loop.  What a chunk does not know at compile time -- the ring half of its first octet, the half of the 64 scalar rows it
reads, whether its first step projects -- is settled once in front of it, and these shapes are where that can go wrong: one, two,
three and more full chunks under an aligned and under an unaligned top (the ring-half parity both ways, both scalar-chunk parities
inside the path), a scalar-chunk boundary under a non-zero (N - 1) & 7, ragged workgroups, padded rows, Q visible, a bank launch.

The checks and their bars are tests/test_gpu_parity.py::test_two_wave_reverse_scan_matches_oracle_and_one_wave's: that test is
called on the new shapes (against the float32 oracle, and against CMPS_OPT_BWD_WAVES = 1), and the cases it cannot express take its
bars through tests/test_gpu_norm_stash.py's helpers, which build them the same way."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from _util import c_oracle_run, make_audio
import test_gpu_bank as TB
import test_gpu_norm_stash as NS
import test_gpu_parity as TP

pytestmark = pytest.mark.gpu


# N = T - 1.  One full chunk below a top chunk: 64 stops one step short of it (the boundary from below), 65 has an empty, 69 an unaligned
# top; two full chunks (both scalar-chunk parities): 96 ... 100; three: 128 ... 135; four and more: 160 ... 199; 259: a scalar-chunk
# boundary inside the path under (N - 1) & 7 = 2
@pytest.mark.parametrize("N", [64, 65, 69, 96, 97, 100, 128, 129, 135, 160, 193, 199, 259])
def test_full_chunks_match_oracle_and_one_wave(N):
    TP.test_two_wave_reverse_scan_matches_oracle_and_one_wave(32, N + 1, 3, 1e-4, None)


@pytest.mark.parametrize("D,B,sigma,rscale", [(32, 5, 1e-4, None), (32, 1, 1e-4, None),      # ragged against four clips per workgroup
                                              (17, 3, 1e-4, None),                            # padded rows
                                              (32, 3, 0.36, 0.69)])                           # Q visible
def test_full_chunks_ragged_padded_visible(D, B, sigma, rscale):
    TP.test_two_wave_reverse_scan_matches_oracle_and_one_wave(D, 101, B, sigma, rscale)


def test_full_chunks_in_a_bank_launch():
    """Two members in one launch (blockIdx.y): every member's gradient has the bits of its own plain handle (the bank's bar,
    tests/test_gpu_bank.py) and meets the oracle at the usual bars."""
    from audio_mps_amd import PsiCMPS
    from audio_mps_amd.scan import unpack_grad
    D, T, B, M = 32, 101, 2, 2
    hp = TB.hparams(D, B)
    params = np.stack([TB.member_params(D, B, 100 + m) for m in range(M)])
    audio = np.stack([make_audio(B, T, hp.delta_t, seed=7 + m) for m in range(M)])
    loss, grad, be = TB.bank_run(D, TB.AUTO, params, audio, hp)
    assert np.all(np.isfinite(grad))
    for m in range(M):
        pl, pg = TB.plain_run(D, TB.AUTO, params[m], audio[m], hp)
        assert TB.same(loss[m], pl) and TB.same(grad[m], pg), m
        model = PsiCMPS(hp, seed=100 + m, backend=object())
        gr, gt, g64 = (C.unpack_grad(c_oracle_run(model, audio[m], d)["grad"], D) for d in ("f32", "f64t32", "f64"))
        NS._check(f"member {m} vs oracle", unpack_grad(grad[m], D), gr, gr, gt, g64)


def test_rho_virtual_clips_keep_the_octet_loop():
    """RhoCMPS D = 32, rank 4, 100 steps: the columns are virtual clips on (y, H y) rows with a row stride, which the full-chunk path does
    not serve.  tests/test_gpu_norm_stash.py::test_rho_virtual_clips_keep_their_rows at a length with full chunks."""
    from audio_mps_amd import _capi
    from oracle import cmps_oracle as O
    import test_gpu_rho as TR
    m, audio = TR._rho_model(32, 101, 2, rank=4, sigma=0.2, seed=98, rscale=0.5)
    be = m._get_backend()
    ohp, ov, Wx, Wy = TR._oracle_side(m)
    ref = O.rho_loss_and_grads(ohp, ov, Wx, Wy, audio, "f32")
    reft, ref64 = (TR._rho_ref64(ohp, ov, Wx, Wy, audio, d) for d in ("f64t32", "f64"))
    NS._set(be, _capi.CMPS_OPT_BWD_WAVES, 2)
    be.kernel_events(True)
    _, g = m.loss_and_grads()
    names = set(be.kernel_times())
    be.kernel_events(False)
    assert "k_bwd_wave2w" in names, names
    assert NS._saved_rows(be) == 0
    TR._check_elastic(g, ref, reft, ref64, ("A", "Rx", "Ry", "freqs", "Wx", "Wy"), "virtual, rank 4 ")


def test_forward_saved_with_plain_rows():
    """A forward saved for the one-wave scan holds (y, H y) rows; with the option back at two waves the reverse pass is k_bwd_wave2w's
    other instance, which keeps the octet loop: 100 steps, against the oracle."""
    from audio_mps_amd import _capi
    from audio_mps_amd.scan import unpack_grad
    D, T, B = 32, 101, 5
    m, audio = NS._model(D, T, B, seed=5)
    be = m._get_backend()
    be.set_params(m.effective_params(), B, T, train=True)
    NS._set(be, _capi.CMPS_OPT_BWD_WAVES, 1)
    be.forward(torch.from_numpy(audio).to(be.device), save_for_bwd=True)
    assert NS._saved_rows(be) == 0
    NS._set(be, _capi.CMPS_OPT_BWD_WAVES, 2)
    be.kernel_events(True)
    flat = be.backward().cpu().numpy()
    names = set(be.kernel_times())
    be.kernel_events(False)
    assert "k_bwd_wave2w" in names, names
    assert np.all(np.isfinite(flat))
    gr, gt, g64 = NS._oracle_grads(m, audio)
    NS._check("(y, H y) rows vs oracle", unpack_grad(flat, D), gr, gr, gt, g64)
