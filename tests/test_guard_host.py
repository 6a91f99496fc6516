"""tests/_guard.py::Guarded on CPU tensors: the helper the memory-contract tests (tests/test_gpu_memory_contract.py,
tests/test_gpu_caller_stream.py) rest on must itself find what it claims to find."""
import numpy as np
import pytest
import torch

from _guard import FILLS, NAN_FILL, ZONE_MIN, Guarded

CPU = torch.device("cpu")
SIZES = [0, 4, 12, 1000, ZONE_MIN + 8]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("align", [256, 64])
def test_payload_is_aligned_exact_and_patterned(nbytes, fill, align):
    g = Guarded(nbytes, CPU, align=align, fill=fill)
    assert g.ptr % align == 0
    assert g.payload.numel() == nbytes and (nbytes == 0 or g.payload.data_ptr() == g.ptr)     # (torch gives an empty slice no address)
    assert g.zone == max(ZONE_MIN, nbytes)
    # a whole zone on either side of the payload, inside the one allocation
    assert g.ptr - g.raw.data_ptr() >= g.zone
    assert g.raw.data_ptr() + g.raw.numel() - (g.ptr + nbytes) >= g.zone
    assert g.zones_intact() is None
    # the whole allocation, payload included, holds the pattern, phased on the payload
    words = g.view(torch.int32).numpy().view(np.uint32)
    assert np.all(words == fill)
    assert bool(g.untouched_mask(torch.float32).all())
    everything = g.raw[(g.off % 4):][: (g.raw.numel() - g.off % 4) // 4 * 4].view(torch.int32).numpy().view(np.uint32)
    assert np.all(everything == fill)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes", [0, 12, 1000])
def test_one_altered_zone_byte_is_found_and_located(nbytes, fill):
    g = Guarded(nbytes, CPU, fill=fill)
    end = g.off + nbytes
    # (position in the allocation, expected (front, back)): first and last byte of each zone
    spots = [(g.off - g.zone, (-g.zone, None)), (g.off - 1, (-1, None)), (end, (None, 0)), (end + g.zone - 1, (None, g.zone - 1))]
    for pos, want in spots:
        old = int(g.raw[pos])
        g.raw[pos] = old ^ 0x01
        assert g.zones_intact() == want, (pos, want)
        g.raw[pos] = old
        assert g.zones_intact() is None
    g.raw[g.off - 1] ^= 0x80
    g.raw[end + 5] ^= 0x80
    g.raw[end + 9] ^= 0x80
    assert g.zones_intact() == (-1, 5)                     # both sides at once: the first altered byte of each


def test_payload_writes_do_not_touch_the_zones():
    g = Guarded(40, CPU)
    g.load(np.arange(10, dtype=np.float32))
    assert g.zones_intact() is None
    assert np.array_equal(g.numpy(np.float32), np.arange(10, dtype=np.float32))
    assert np.array_equal(g.view(torch.float32, (2, 5)).numpy(), np.arange(10, dtype=np.float32).reshape(2, 5))
    with pytest.raises(AssertionError):
        g.load(np.arange(11, dtype=np.float32))              # not exactly nbytes


def test_altered_input_byte_is_found():
    g = Guarded(64, CPU)
    data = np.linspace(-1, 1, 16).astype(np.float32)
    g.load(data)
    g.snapshot()
    assert g.equals_snapshot() is None
    g.payload[37] ^= 0x01
    assert g.equals_snapshot() == 37
    g.payload[37] ^= 0x01
    assert g.equals_snapshot() is None
    h = Guarded(64, CPU)
    h.snapshot(data)                                         # the snapshot of a load that has not happened yet
    assert h.equals_snapshot() == 0
    h.load(data)
    assert h.equals_snapshot() is None


def test_leftover_pattern_element_is_found_and_an_ordinary_nan_is_not():
    g = Guarded(4 * 9, CPU, fill=NAN_FILL)
    out = np.arange(9, dtype=np.float32)
    out[2] = np.float32(np.nan)                              # 0x7FC00000: a NaN a kernel may legitimately produce
    out[4] = np.inf
    assert out.view(np.uint32)[2] == 0x7FC00000
    g.load(out)
    assert not bool(g.untouched_mask(torch.float32).any())
    g.view(torch.int32)[7] = np.array(NAN_FILL, dtype=np.uint32).view(np.int32).item()
    mask = g.untouched_mask(torch.float32).numpy()
    assert mask.tolist() == [False] * 7 + [True, False]
    # three of the pattern's four bytes are not the pattern
    g.payload[4 * 7] ^= 0x01
    assert not bool(g.untouched_mask(torch.float32).any())
    # wider elements: all of their bytes must be the pattern
    d = Guarded(32, CPU, fill=NAN_FILL)
    d.view(torch.int32)[1] = 0
    assert d.untouched_mask(torch.float64).tolist() == [False, True, True, True]


def test_refill_restores_the_pattern():
    g = Guarded(100, CPU)
    g.raw[:] = 7
    assert g.zones_intact() == (-g.off, 0)
    g.refill()
    assert g.zones_intact() is None and bool(g.untouched_mask(torch.int32).all())
    g.payload[:] = 1
    g.refill_payload()
    assert bool(g.untouched_mask(torch.int32).all())
