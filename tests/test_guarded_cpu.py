"""
tests/guarded.py proved on CPU tensors with a fake writer: every kind of stray store the GPU tests rely on it to see is
reported, with the guard and the offset named, and a clean run passes.  (No GPU test stores out of bounds on purpose;
this file stands in for that.)
"""
import numpy as np
import pytest
import torch

import guarded as G

W = 13


def _arrays(dtype=np.float64):
    rng = np.random.default_rng(7)
    return [(100 * rng.standard_normal((6, W))).astype(dtype), (100 * rng.standard_normal((4, W))).astype(dtype),
            (100 * rng.standard_normal((2, W))).astype(dtype)]                # even sizes: an odd guard alternates the bases


FILLS = {"nan": G.NAN_BITS, "1e300": G.BIG_BITS}


@pytest.mark.parametrize("fill", sorted(FILLS))
def test_a_clean_run_passes_and_the_layout_is_as_described(fill):
    arrs = _arrays()
    g = G.min_guard(W) + 1                                            # odd
    views, h = G.embed(arrs, g, FILLS[fill])
    assert g % 2 == 1 and g >= 2 * W + 64
    for v, a in zip(views, arrs):
        assert v.is_contiguous() and np.array_equal(v.numpy(), a)
    base = [v.data_ptr() % 16 for v in views]
    assert base == [8, 0, 8], base                                    # alternating alignment classes
    assert h.spans[0][0] == g and h.spans[1][0] - h.spans[0][1] == g and h.buf.numel() - h.spans[2][1] == g
    views[1].mul_(1.0)                                                # a write that changes no bit
    G.check(h, "clean")
    # the fills are what they claim to be
    guard = h.buf[:g].numpy()
    assert (np.isnan(guard).all() if fill == "nan" else (guard == 1e300).all())
    assert (guard.view(np.int64) == np.int64(G._signed(FILLS[fill], 8))).all()


def test_tight_layout_is_back_to_back():
    arrs = _arrays()
    views, h = G.embed(arrs, 0, tail=G.min_guard(W))
    assert views[1].data_ptr() == views[0].data_ptr() + 8 * arrs[0].size
    assert views[2].data_ptr() == views[1].data_ptr() + 8 * arrs[1].size
    G.check(h, "tight")
    h.buf[h.spans[2][1]] = 0.0
    with pytest.raises(AssertionError, match=r"guard 3 of 4 .* at offset 0 "):
        G.check(h, "tight")


def test_a_store_one_element_before_the_first_array_is_reported():
    views, h = G.embed(_arrays(), 91, inputs=False)
    h.buf[h.spans[0][0] - 1] = 1.0
    with pytest.raises(AssertionError, match=r"guard 0 of 4 .* at offset 90 \(1 from its end\)"):
        G.check(h, "before")


def test_a_store_one_element_after_the_last_array_is_reported():
    views, h = G.embed(_arrays(), 91, inputs=False)
    h.buf[h.spans[2][1]] = 1.0
    with pytest.raises(AssertionError, match=r"guard 3 of 4 .* after array 2\) was written at offset 0 "):
        G.check(h, "after")


def test_a_store_into_a_middle_guard_is_reported():
    views, h = G.embed(_arrays(), 91, inputs=False)
    h.buf[h.spans[1][1] + 17] = -2.5
    with pytest.raises(AssertionError, match=r"guard 2 of 4 .* at offset 17 "):
        G.check(h, "middle")
    # outputs may change freely
    views, h = G.embed(_arrays(), 91, inputs=False)
    views[0].zero_()
    G.check(h, "outputs are free")


def test_a_store_into_an_input_is_reported():
    views, h = G.embed(_arrays(), 91)
    views[1][2, 5] += 1.0
    with pytest.raises(AssertionError, match=r"input array 1 was written at flat offset %d " % (2 * W + 5)):
        G.check(h, "input")
    # ... and so is a sign flip of a zero, which compares equal as a float
    views, h = G.embed([np.zeros((3, W))], 91)
    views[0][1, 1] = -0.0
    with pytest.raises(AssertionError, match="input array 0"):
        G.check(h, "negative zero")


def test_a_nan_for_nan_rewrite_with_another_payload_is_reported():
    views, h = G.embed(_arrays(), 91, G.NAN_BITS, inputs=False)
    h.buf[3] = float("nan")                                           # the default quiet NaN: not the payload of the fill
    assert torch.isnan(h.buf[:91]).all()
    with pytest.raises(AssertionError, match=r"guard 0 of 4 .* at offset 3 "):
        G.check(h, "payload")


@pytest.mark.parametrize("dtype", [np.int32, np.uint16, np.float32])
def test_other_element_types(dtype):
    if dtype == np.uint16:
        arrs = [torch.from_numpy(a.astype(np.int32)).to(torch.uint16) for a in _arrays(np.int32)]
    else:
        arrs = _arrays(dtype)
    views, h = G.embed(arrs, 91)
    G.check(h, "clean")
    if dtype == np.int32:
        assert int(h.buf[0]) == G.INT32_FILL
    h.bits()[h.spans[0][1]] += 1
    with pytest.raises(AssertionError, match=r"guard 1 of 4 .* at offset 0 "):
        G.check(h, "typed")
