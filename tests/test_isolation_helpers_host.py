"""CPU self-tests of the row-isolation helpers in tests/helpers.py: banded() / untouched() (an output placed between two bands of a NaN bit
pattern, so that a store in front of it or behind it shows) and group_index() / poison_groups() (every odd attention group or row made
NaN / +Inf, so that every clean group has poisoned neighbours on both sides in any tile packing).  The GPU tests that use them are not
part of this file."""
import pytest
import torch

from helpers import banded, untouched, group_index, poison_groups, BAND_BYTES, BAND_PATTERN


def test_banded_detects_a_write_on_either_side_and_counts_untouched_words():
    v, check = banded((5, 3), device="cpu")
    assert v.shape == (5, 3) and v.dtype == torch.float32 and v.is_contiguous()
    base = v.untyped_storage()
    assert base.nbytes() == BAND_BYTES + BAND_BYTES + BAND_BYTES and v.storage_offset() * 4 == BAND_BYTES
    assert torch.isnan(v).all() and (v.view(torch.int32) == BAND_PATTERN).all()
    check()
    assert untouched(v) == 15
    v[1, 2] = 1.0
    v[4, 2] = float("nan")          # another NaN than the pattern counts as written
    assert untouched(v) == 13
    check()
    flat = torch.empty(0, dtype=torch.float32).set_(base, 0, (base.nbytes() // 4,))
    first = BAND_BYTES // 4
    for word in (first - 1, first + 15, 0, flat.numel() - 1):       # one element before the view, one past it, the far ends
        keep = flat[word].clone()
        flat[word] = 0.0
        with pytest.raises(AssertionError):
            check()
        flat[word] = keep
        check()
    # a byte-sized view whose length is no multiple of four: the band starts at the first byte behind it
    w, wcheck = banded((4099,), dtype=torch.uint8, device="cpu")
    wcheck()
    assert untouched(w) == 1024
    wb = torch.empty(0, dtype=torch.uint8).set_(w.untyped_storage(), 0, (w.untyped_storage().nbytes(),))
    assert wb.numel() == BAND_BYTES + 2 * BAND_BYTES + BAND_BYTES
    wb[BAND_BYTES + 4098] ^= 0xFF       # the view's last byte: inside
    wcheck()
    wb[BAND_BYTES + 4099] ^= 0xFF       # one past it
    with pytest.raises(AssertionError):
        wcheck()


def test_poison_groups_and_group_arithmetic():
    B, T, J = 2, 3, 5
    x = torch.arange(B * T * J * 4, dtype=torch.float32).reshape(B * T * J, 4)
    for temporal in (True, False):
        g = group_index(B, T, J, temporal)
        want = torch.tensor([(b * J + j) if temporal else (b * T + t) for b in range(B) for t in range(T) for j in range(J)])
        assert torch.equal(g, want)
        bad, keep = poison_groups(x, g)
        assert torch.equal(keep, want % 2 == 0)
        assert torch.equal(bad[keep], x[keep])
        assert torch.isnan(bad[want % 4 == 1]).all() and (bad[want % 4 == 3] == float("inf")).all()
        assert (want % 4 == 1).any() and (want % 4 == 3).any() and torch.isfinite(x).all()      # x itself is not modified
        part, keep2 = poison_groups(x, g, cols=slice(2, 4))
        assert torch.equal(keep2, keep) and torch.equal(part[:, :2], x[:, :2]) and not torch.isfinite(part[~keep][:, 2:]).any()
