"""The guarded buffers of guarded.py, on CPU tensors: the checker is shown to fail before the GPU tests trust it."""
import pytest
import torch

import guarded

DTYPES = [torch.float32, torch.float64, torch.int32]


def _value(dtype):
    return torch.tensor(3, dtype=dtype)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_layout_and_canary(dtype, lead):
    v = guarded.arena((5, 7), dtype, "cpu", lead)
    flat, start, n = guarded.bits(v)
    size = v.element_size()
    assert v.shape == (5, 7) and v.is_contiguous() and n == 35
    assert start * size >= guarded.BAND_BYTES and (flat.numel() - start - n) * size >= guarded.BAND_BYTES
    assert (v.data_ptr() - flat.data_ptr()) == start * size and start == guarded.BAND_BYTES // size + lead
    assert v.data_ptr() % size == 0 and (lead == 0) == ((v.data_ptr() - flat.data_ptr()) % guarded.BAND_BYTES == 0)
    assert v.contiguous() is v  # (the library sees the interior pointer)
    assert (flat == guarded.CANARY[dtype]).all()
    if dtype.is_floating_point:
        assert torch.isnan(v).all()  # a quiet NaN: an over-read that reaches a live result shows
    else:
        assert guarded.CANARY[dtype] % 2 == 1
    assert guarded.check(v) == 35


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_check_passes_in_bounds_and_counts_unwritten_elements(dtype, lead):
    v = guarded.arena((4, 6), dtype, "cpu", lead)
    v[:3] = _value(dtype)
    assert guarded.check(v) == 6  # the last row was never written
    v[3, :5] = _value(dtype)
    assert guarded.check(v) == 1
    v.view(-1)[0] = _value(dtype)  # the first and the last element, again: in bounds
    v.view(-1)[-1] = _value(dtype)
    assert guarded.check(v) == 0


@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_check_fails_one_element_outside(dtype, lead, where):
    v = guarded.arena((4, 6), dtype, "cpu", lead)
    v[:] = _value(dtype)
    assert guarded.check(v) == 0
    flat, start, n = guarded.bits(v)
    flat.view(dtype)[start - 1 if where == "before" else start + n] = _value(dtype)
    with pytest.raises(AssertionError) as err:
        guarded.check(v)
    assert ("front" if where == "before" else "back") in str(err.value)
    assert f"offsets {-1 if where == 'before' else n} .. " in str(err.value)


def test_check_fails_at_the_far_ends_of_the_bands():
    for at in (0, -1):
        v = guarded.arena((3,), torch.float64, "cpu", 1)
        flat = guarded.bits(v)[0]
        flat[at] = 0
        with pytest.raises(AssertionError):
            guarded.check(v)


def test_a_nan_with_another_payload_is_not_the_canary():
    v = guarded.arena((3,), torch.float32, "cpu")
    v[:] = float("nan")
    assert guarded.check(v) == 0


def test_snapshot_sees_any_changed_bit():
    v = guarded.place([[1.0, 2.0], [3.0, 4.0]], torch.float64, "cpu", 1)
    before = guarded.snapshot(v)
    assert guarded.same_bits(v, before)
    v[1, 0] = -3.0
    assert not guarded.same_bits(v, before) and guarded.same_bits(v, before, 2, 3) and not guarded.same_bits(v, before, 0, 2)
    v[1, 0] = 3.0
    guarded.bits(v)[0][-1] = 0
    assert not guarded.same_bits(v, before) and not guarded.same_bits(v, before, 0, 4)


@pytest.mark.parametrize("lead", [0, 1])
def test_guarded_outputs_patches_torch_empty_and_restores_it(lead):
    real = torch.empty
    with guarded.guarded_outputs(lead) as made:
        a = torch.empty((3, 2), dtype=torch.float64, device="cpu")
        b = torch.empty(4, dtype=torch.int32, device="cpu")
        c = torch.empty((2,), dtype=torch.uint8)  # not a guarded type: the real one
    assert torch.empty is real
    assert len(made) == 2 and made[0] is a and made[1] is b and c.dtype == torch.uint8
    assert guarded.check(a) == 6 and guarded.check(b) == 4 and guarded.bits(a)[1] == 512 + lead
    with pytest.raises(RuntimeError):
        with guarded.guarded_outputs():
            raise RuntimeError("restored after an exception too")
    assert torch.empty is real
