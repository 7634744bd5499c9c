"""What grbda_energy_*, grbda_centroidal_* and grbda_centroidal_matrix_* (f64, f32 and the host-array variants) refuse, and that they
refuse it before looking for a device; and grbda_plan_total_mass, which needs none.

No device is needed: the argument checks run on the host before any device call, and a machine without a device answers
GRBDA_ENODEVICE to a call that passes them (test_contact_args_cpu.py: the same method).  On a machine WITH a device the rows expected to
pass the checks are not called (the arrays of this file are host memory).

The expectations are the rules of include/grbda_hip.h ("energy and centroidal quantities"): GRBDA_EINVAL for a NULL plan, a missing
required pointer, no output asked for, outputs that overlap inputs or each other; GRBDA_EUNSUPPORTED with text for com, com_vel, h, hdot
or A when the total mass is not positive (energy is still served); B == 0 is GRBDA_OK."""
import ctypes
import itertools
import os
import subprocess
from ctypes import c_double, c_int, c_size_t, c_void_p

import numpy as np
import pytest

import centroidal_ref as C
import generalized_rbda_amd as G
from entry_points import _model
from models import zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED, ENODEVICE = 0, -1, -2, -3
# entry point -> (inputs, outputs); every entry point ends (B, device[, stream])
ENTRIES = {
    "energy": (("q", "qd"), ("kinetic", "potential")),
    "centroidal": (("q", "qd", "ydd"), ("com", "com_vel", "h", "hdot")),
    "centroidal_matrix": (("q",), ("A",)),
}
# output -> the inputs it needs besides q
NEEDS = {"kinetic": ("qd",), "potential": (), "com": (), "com_vel": ("qd",), "h": ("qd",), "hdot": ("qd", "ydd"), "A": ()}
VARIANTS = [f"{e}_{v}" for e in ENTRIES for v in ("f64", "f32", "host_f64") if (e, v) != ("centroidal_matrix", "host_f64")]


@pytest.fixture(scope="module")
def plan():
    return G.Plan(_model("urdf_mini_cheetah"))


@pytest.fixture(scope="module")
def massless_plan():
    """the four-bar with every body's inertia zero: total mass 0"""
    from generalized_rbda_amd.states import parse_clusters  # noqa: F401  (the description parses)

    import deriv_recursion_numpy as D
    import struct

    blob = bytearray(_model("urdf_four_bar"))
    m = D.parse(bytes(blob))
    # every body record holds its 6 x 6 inertia as 36 doubles: find each by value and zero it
    for bd in m["bodies"]:
        raw = struct.pack("<36d", *np.asarray(bd["I"]).reshape(-1))
        at = bytes(blob).find(raw)
        assert at >= 0
        blob[at:at + len(raw)] = bytes(len(raw))
    return G.Plan(bytes(blob))


def entry_of(variant):
    return variant.rsplit("_host", 1)[0].rsplit("_f", 1)[0]


def _library():
    G.lib()
    L = ctypes.CDLL(G.LIB_PATH)
    L.grbda_last_error.restype = ctypes.c_char_p
    return L


def call(L, plan_handle, variant, values, B=1):
    """(return code, error text) of one call; values: name -> address or None, in the entry point's argument order"""
    entry = entry_of(variant)
    host = variant.endswith("host_f64")
    ins, outs = ENTRIES[entry]
    fn = getattr(L, "grbda_" + variant)
    fn.argtypes = [c_void_p] * (1 + len(ins) + len(outs)) + [c_size_t, c_int] + ([] if host else [c_void_p])
    rc = fn(plan_handle, *[values[n] for n in ins + outs], B, 0, *([] if host else [None]))
    return rc, (L.grbda_last_error().decode() if rc else "")


def valid(entry, keep):
    """one 8 KiB host array per pointer argument (B = 1: the largest, 6 x nv, is under 1 KB)"""
    values = {}
    for n in ENTRIES[entry][0] + ENTRIES[entry][1]:
        keep.append((c_double * 1024)())
        values[n] = ctypes.addressof(keep[-1])
    return values


def passes(L, plan, variant, values):
    """a call that passes every check: GRBDA_ENODEVICE here; not made on a machine with a device (host arrays)"""
    if G.device_count() > 0:
        return
    rc, text = call(L, plan._h, variant, values)
    assert (rc, text) == (ENODEVICE, "no HIP device available (there is no CPU fallback)"), (variant, rc, text)


@pytest.mark.parametrize("variant", VARIANTS)
def test_refusals_come_before_the_device(variant, plan):
    L, keep = _library(), []
    entry = entry_of(variant)
    ins, outs = ENTRIES[entry]
    passes(L, plan, variant, valid(entry, keep))
    # a null plan, before anything else
    for change in ({}, {"q": None}, {outs[0]: None}):
        rc, text = call(L, None, variant, {**valid(entry, keep), **change})
        assert (rc, text) == (EINVAL, "null plan"), (change, rc, text)
    rc, text = call(L, plan._h, variant, {**valid(entry, keep), "q": None})
    assert (rc, text) == (EINVAL, "null argument")
    # no output asked for
    rc, text = call(L, plan._h, variant, {**valid(entry, keep), **{o: None for o in outs}})
    assert rc == EINVAL and text == ("null argument" if entry == "centroidal_matrix" else "no output asked for"), (rc, text)
    # every subset of the outputs, with exactly the inputs it needs and with each needed input missing
    for k in range(1, len(outs) + 1):
        for asked in itertools.combinations(outs, k):
            need = {i for o in asked for i in NEEDS[o]}
            v = {**valid(entry, keep), **{o: None for o in outs if o not in asked}, **{i: None for i in ins[1:] if i not in need}}
            passes(L, plan, variant, v)
            for missing in need:
                rc, text = call(L, plan._h, variant, {**v, missing: None})
                assert rc == EINVAL and "need" in text and missing in text, (asked, missing, rc, text)
    # outputs that overlap inputs or each other
    for o in outs:
        for i in ins:
            v = valid(entry, keep)
            rc, text = call(L, plan._h, variant, {**v, o: v[i]})
            assert (rc, text) == (EINVAL, "an output array overlaps an input array"), (o, i, rc, text)
    for a, b in itertools.combinations(outs, 2):
        v = valid(entry, keep)
        rc, text = call(L, plan._h, variant, {**v, b: v[a]})
        assert (rc, text) == (EINVAL, "two output arrays overlap"), (a, b, rc, text)
    # B == 0: nothing to do, no device asked for
    assert call(L, plan._h, variant, valid(entry, keep), B=0) == (OK, "")


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_model_without_mass_is_refused_where_the_centre_of_mass_enters(variant, massless_plan):
    L, keep = _library(), []
    assert massless_plan.total_mass() == 0.0
    entry = entry_of(variant)
    if entry == "energy":
        passes(L, massless_plan, variant, valid(entry, keep))
        return
    for o in ENTRIES[entry][1]:
        v = {**valid(entry, keep), **{x: None for x in ENTRIES[entry][1] if x != o}}
        rc, text = call(L, massless_plan._h, variant, v)
        assert rc == EUNSUPPORTED and "total mass" in text, (o, rc, text)
    # the argument rules come first
    rc, text = call(L, massless_plan._h, variant, {**valid(entry, keep), "q": None})
    assert (rc, text) == (EINVAL, "null argument")


@pytest.mark.parametrize("name", list(zoo()) + ["parallel_chain_exp_d10_l16", "two_parent"])
def test_total_mass_is_the_sum_of_the_body_masses(name):
    blob = _model(name)
    plan = G.Plan(blob)
    assert plan.total_mass() == pytest.approx(C.total_mass(blob), rel=1e-14) and plan.total_mass() > 0


def test_total_mass_refuses_null_arguments(plan):
    L = _library()
    L.grbda_plan_total_mass.argtypes = [c_void_p, c_void_p]
    m = c_double(-1.0)
    assert L.grbda_plan_total_mass(None, ctypes.byref(m)) == EINVAL
    assert L.grbda_plan_total_mass(plan._h, None) == EINVAL
    assert L.grbda_plan_total_mass(plan._h, ctypes.byref(m)) == OK and m.value == plan.total_mass()


def test_facade_total_mass_and_batch_refusals(tmp_path):
    """tests/cpp/centroidal_facade_test.cpp: ClusterTreeModel::totalMass, energyBatch and centroidalBatch, built the way
    tests/cpp/integrate_facade_test.cpp is"""
    out = tmp_path / "centroidal_facade_test"
    lib_dir = os.path.join(ROOT, "generalized_rbda_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I/opt/rocm/include", "-I" + os.path.join(lib_dir, "include"),
                    os.path.join(ROOT, "tests", "cpp", "centroidal_facade_test.cpp"), "-o", str(out), "-L" + lib_dir, "-lgrbda_hip",
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(out), os.path.join(ROOT, "tests", "golden", "robot-models", "mini_cheetah.urdf")], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
