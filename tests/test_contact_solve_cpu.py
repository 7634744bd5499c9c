"""What grbda_contact_dynamics_* launches its solve kernel with, pinned without a device (grbda_contact_solve_launch, device < 0): the
states per workgroup and the dynamic LDS of a workgroup for 1 .. 8 contacts in both precisions, as contact_solve_lanes() of
contact_kernels.hip decides them -- of 64, 32 and 16 lanes the width with the most states resident on a CU (160 KiB of LDS in granules of
1 280 bytes, at most 32 workgroups), the wider one on a tie.  The table below is worked out by hand from that rule, not read back from the
library; launch_contact_solve reads the same record, so a change of the rule shows here.  tests/test_contact_solve_gpu.py takes the
widths of its lane-boundary cases from the same query."""
import ctypes

import pytest

import generalized_rbda_amd as G

# (precision, contacts): (lanes, LDS bytes per workgroup = (m (m + 1) / 2 + m) lanes sizeof(T), m = 3 n)
TABLE = {
    ("f32", 1): (64, 2304), ("f64", 1): (64, 4608),
    ("f32", 2): (64, 6912), ("f64", 2): (64, 13824),
    ("f32", 3): (64, 13824), ("f64", 3): (32, 13824),
    ("f32", 4): (64, 23040), ("f64", 4): (32, 23040),
    ("f32", 5): (32, 17280), ("f64", 5): (16, 17280),
    ("f32", 6): (64, 48384), ("f64", 6): (32, 48384),
    ("f32", 7): (16, 16128), ("f64", 7): (64, 129024),
    ("f32", 8): (16, 20736), ("f64", 8): (16, 41472),
}
LDS_PER_CU, GRANULE = 160 * 1024, 1280


def per_cu(lds):
    """workgroups of `lds` bytes a CU holds, at most 32"""
    return min(32, LDS_PER_CU // (-(-lds // GRANULE) * GRANULE))


@pytest.mark.parametrize("key", sorted(TABLE), ids=lambda k: f"{k[0]}-n{k[1]}")
def test_width_and_lds_of_every_row(key):
    dtype, n = key
    lanes, lds, cap = G.contact_solve_launch(n, dtype)
    m, elem = 3 * n, 4 if dtype == "f32" else 8
    assert (lanes, lds) == TABLE[key]
    assert lds == (m * (m + 1) // 2 + m) * lanes * elem
    assert lds <= LDS_PER_CU
    assert cap == per_cu(lds) >= 1  # device < 0: one CU


def test_fp64_with_seven_contacts_is_the_one_row_above_64_kib():
    above = [k for k in TABLE if G.contact_solve_launch(k[1], k[0])[1] > 64 * 1024]
    assert above == [("f64", 7)]


def test_the_width_keeps_the_most_states_resident():
    """the rule itself, so that the table cannot be edited into agreement with a wrong width"""
    for (dtype, n), (lanes, _) in TABLE.items():
        m, elem = 3 * n, 4 if dtype == "f32" else 8
        states = {w: (per_cu(b) * w if b <= LDS_PER_CU else 0) for w in (64, 32, 16) for b in [(m * (m + 1) // 2 + m) * w * elem]}
        best = max(states.values())
        assert lanes == max(w for w, s in states.items() if s == best), (dtype, n, states)


def test_refusals():
    L = G.lib()
    lanes, lds, cap = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    out = (ctypes.byref(lanes), ctypes.byref(lds), ctypes.byref(cap))
    assert L.grbda_contact_solve_launch(0, 64, -1, *out) == -1
    assert L.grbda_contact_solve_launch(9, 64, -1, *out) == -1
    assert L.grbda_contact_solve_launch(4, 16, -1, *out) == -1
    assert L.grbda_contact_solve_launch(4, 64, -1, None, out[1], out[2]) == -1
    assert L.grbda_contact_solve_launch(4, 64, -1, *out) == 0 and lanes.value == 32
