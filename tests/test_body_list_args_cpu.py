"""Poses and twists of a listed few bodies (include/grbda_hip_bodies.h) without a GPU: the symbols, the signature table against that header
parameter by parameter, the argument rules -- every refusal is decided before a device is looked at, so a machine without one answers
GRBDA_EINVAL to a bad call and GRBDA_ENODEVICE only to a good one -- and the walk grbda_body_list_walk reports, held to walks derived here
from the models' parent tables.  The arrays are host buffers standing in for device arrays: the rules never read them, and no call that
passes the rules is made where a device is present."""
import ctypes
import os

import numpy as np
import pytest

import entry_points as EP
import generalized_rbda_amd as G
import test_abi_table_cpu as abi
import wrench_ref as W
from deriv_recursion_numpy import parse
from generalized_rbda_amd._abi import BODIES_SIGNATURES, JVP_SIGNATURES, SIGNATURES, STEP_VJP_SIGNATURES, VJP_SIGNATURES, WRENCH_SIGNATURES
from id_derivative_refs import blob_of

EINVAL, ENODEVICE, OK = -1, -3, 0
POSES = ("grbda_body_poses_list_f64", "grbda_body_poses_list_f32", "grbda_body_poses_list_host_f64")
TWISTS = ("grbda_body_twists_list_f64", "grbda_body_twists_list_f32", "grbda_body_twists_list_host_f64")
ENTRY_POINTS = POSES + TWISTS
BODIES_HEADER = os.path.join(os.path.dirname(abi.HEADER), "grbda_hip_bodies.h")
# the caps of devplan.h, as include/grbda_hip_bodies.h states them
MAX_WALK, MAX_SAVED = 19, 4


def test_the_symbols_are_exported_and_bound():
    L = ctypes.CDLL(G.LIB_PATH)
    assert len(BODIES_SIGNATURES) == 7
    for name in ENTRY_POINTS + ("grbda_body_list_walk",):
        assert hasattr(L, name), name
        assert name in BODIES_SIGNATURES
    others = (SIGNATURES, VJP_SIGNATURES, STEP_VJP_SIGNATURES, WRENCH_SIGNATURES, JVP_SIGNATURES)
    assert not any(set(BODIES_SIGNATURES) & set(t) for t in others)
    assert len(SIGNATURES) == 96 and len(WRENCH_SIGNATURES) == 7
    for method in ("body_poses_list", "body_twists_list", "body_poses_list_host", "body_twists_list_host", "body_list_walk"):
        assert callable(getattr(G.Plan, method))


def test_the_table_declares_what_the_header_does(monkeypatch):
    monkeypatch.setattr(abi, "HEADER", BODIES_HEADER)
    protos = abi.header_prototypes()
    assert set(protos) == set(BODIES_SIGNATURES)
    assert protos["grbda_body_poses_list_f32"][1][2] == ("int", "n") and protos["grbda_body_twists_list_f64"][1][4] == ("int", "n")
    assert [p for _, p in protos["grbda_body_twists_list_host_f64"][1]][-1] == "device"
    abi.compare(BODIES_SIGNATURES, protos)
    broken = dict(BODIES_SIGNATURES)  # (the comparison does fail on a defect: n declared as a pointer)
    args = list(broken["grbda_body_poses_list_f64"][1])
    args[2] = ctypes.c_void_p
    broken["grbda_body_poses_list_f64"] = (ctypes.c_int, tuple(args))
    with pytest.raises(AssertionError):
        abi.compare(broken, protos)
    text = open(BODIES_HEADER).read()
    assert f"longer than {MAX_WALK} steps" in text and f"more than {MAX_SAVED} branch" in text


def test_the_loaded_library_carries_the_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load)
    L = G.lib()
    for name, (restype, argtypes) in BODIES_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_body_poses_list_f64.argtypes) == 8 and len(L.grbda_body_twists_list_host_f64.argtypes) == 9


class _Call:
    """one plan, host buffers of B states standing in for the arrays"""

    def __init__(self, B=3, n=2):
        self.plan = G.Plan(blob_of("tree16_fixed"))
        nq, nv = self.plan.nq, self.plan.nv
        self.B, self.n = B, n
        self.q, self.qd, self.ydd = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, nv))
        self.out = np.zeros((B, 16, 12))

    def __call__(self, fn, q="q", qd="qd", ydd="ydd", n=None, bodies=(0, 1), out="out", B=None, plan=True):
        ptr = lambda a: None if a is None else getattr(self, a).ctypes.data if isinstance(a, str) else a
        n = self.n if n is None else n
        arr = None if bodies is None else (ctypes.c_int * max(len(bodies), 1))(*bodies)
        state = [ptr(q)] + ([ptr(qd), ptr(ydd)] if fn in TWISTS else [])
        args = [self.plan._h if plan else None, *state, n, arr, ptr(out), self.B if B is None else B, 0]
        if "host" not in fn:
            args.append(None)
        return getattr(G.lib(), fn)(*args)


def _item(fn):
    return 4 if fn.endswith("f32") else 8


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_null_arguments_are_refused(fn):
    c = _Call()
    assert c(fn, plan=False) == EINVAL
    for name in ("q", "out", "bodies") + (("qd", "ydd") if fn in TWISTS else ()):
        assert c(fn, **{name: None}) == EINVAL, name
        assert c(fn, B=0, **{name: None}) == EINVAL, name


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_the_list_is_checked(fn):
    c = _Call()
    n_bodies = c.plan.n_bodies
    assert c(fn, n=-1) == EINVAL and c(fn, n=17, bodies=tuple(range(16)) + (0,)) == EINVAL
    assert "0..16" in G.lib().grbda_last_error().decode()
    assert c(fn, bodies=(0, n_bodies)) == EINVAL and c(fn, bodies=(-1, 0)) == EINVAL
    assert "body index" in G.lib().grbda_last_error().decode()
    assert c(fn, n=1, bodies=(0, n_bodies), B=0) == OK  # (only the first n entries are the list)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_overlapping_arguments_are_refused(fn):
    c = _Call()
    item = _item(fn)
    for name in ("q",) + (("qd", "ydd") if fn in TWISTS else ()):
        a = getattr(c, name)
        assert c(fn, out=a.ctypes.data) == EINVAL, name
        assert c(fn, out=a.ctypes.data + (a.size - 1) * item) == EINVAL, name  # the input's last element is the output's first
    assert "overlaps" in G.lib().grbda_last_error().decode()
    assert c(fn, out=c.q.ctypes.data - c.B * c.n * 12 * item + item) == EINVAL      # the output's last element is the input's first
    assert c(fn, out=c.q.ctypes.data - c.B * c.n * 12 * item, B=0) == OK            # (right in front of q)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_an_empty_batch_or_list_is_ok_without_a_device(fn):
    c = _Call()
    assert c(fn, B=0) == OK and c(fn, B=0, n=16, bodies=(1,) * 16) == OK
    assert c(fn, n=0) == OK and c(fn, n=0, bodies=None, out=None) == OK and c(fn, n=0, B=0, bodies=None, out=None) == OK
    assert not c.out.any()
    if G.device_count() == 0:  # a good call needs a device, and says so
        assert c(fn) == ENODEVICE


def test_the_walk_call_checks_its_arguments():
    c = _Call()
    a, b, r = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    walk = lambda plan, n, bodies: G.lib().grbda_body_list_walk(plan, n, None if bodies is None else (ctypes.c_int * max(len(bodies), 1))(*bodies),
                                                                ctypes.byref(a), ctypes.byref(b), ctypes.byref(r))
    h = c.plan._h
    assert walk(None, 1, (0,)) == EINVAL and walk(h, -1, (0,)) == EINVAL and walk(h, 17, (0,) * 17) == EINVAL and walk(h, 1, None) == EINVAL
    assert walk(h, 1, (c.plan.n_bodies,)) == EINVAL and walk(h, 1, (-1,)) == EINVAL
    assert walk(h, 0, None) == OK and (a.value, b.value, r.value) == (0, 0, 0)
    assert G.lib().grbda_body_list_walk(h, 1, (ctypes.c_int * 1)(0), None, None, None) == OK  # (any output may be left out)


# ---- the walk, against the parent table ------------------------------------------------------------------------------------------------
def _tree(name):
    blob = EP._model(name)
    return G.Plan(blob), [b["parent"] for b in parse(blob)["bodies"]], W.tree_places(blob)


def _path(parent, b):
    """b and its ancestors"""
    out = []
    while b >= 0:
        out.append(b)
        b = parent[b]
    return out


def _expected(parent, bodies):
    """(walk length, peak number of saved values) of a list, from the parent table alone: the walk is the union of the root paths; a body
    with two or more children in it holds a saved value from its own step up to the step of its last child, depth first with the
    children in index order"""
    walk = sorted(set().union(*[_path(parent, b) for b in bodies]))
    kids = {b: [c for c in walk if parent[c] == b] for b in walk}
    peak, held = 0, set()

    def visit(b):
        nonlocal peak
        if len(kids[b]) >= 2:
            held.add(b)
            peak = max(peak, len(held))
        for c in kids[b]:
            if c == kids[b][-1] and len(kids[b]) >= 2:
                held.discard(b)  # (read by its last child's step, before that step saves anything of its own)
                # the child's own save, if any, is counted inside visit(c)
            visit(c)

    for root in [b for b in walk if parent[b] < 0]:
        visit(root)
    return len(walk), peak


def test_walks_of_the_mini_cheetah():
    plan, parent, places = _tree("urdf_mini_cheetah")
    base, tips, rotors = places["base"], places["tips"], places["rotors"]
    assert parent[base] == -1 and len(tips) == 4
    # one leaf link: its root path, nothing saved -- foot, knee... hip, base
    foot = tips[0]
    assert not any(p == foot for p in parent)
    assert plan.body_list_walk([foot]) == (len(_path(parent, foot)), 0, 0) == (4, 0, 0)
    # two feet on different legs: they share the base alone, which is walked once and saved for the second leg
    other = tips[1]
    assert set(_path(parent, foot)) & set(_path(parent, other)) == {base}
    both = len(_path(parent, foot)) + len(_path(parent, other)) - 1
    assert plan.body_list_walk([other, foot]) == (both, 1, 0) == (7, 1, 0)
    assert plan.body_list_walk([foot, other]) == (both, 1, 0)
    # a body with its own ancestor: the body's walk
    knee = parent[foot]
    assert plan.body_list_walk([foot, knee]) == plan.body_list_walk([foot]) and plan.body_list_walk([base, foot, knee])[0] == 4
    # a rotor: its own path, no other rotor on it
    rotor = rotors[-1]
    path = _path(parent, rotor)
    assert [b for b in path if b in rotors] == [rotor]
    assert plan.body_list_walk([rotor]) == (len(path), 0, 0)
    # the same body twice: the same walk (and two output slots, which the device tests read)
    assert plan.body_list_walk([foot, foot]) == plan.body_list_walk([foot])
    # all four feet: the base is saved once, for three legs
    assert plan.body_list_walk(tips) == (1 + 4 * 3, 1, 0)


@pytest.mark.parametrize("name", ["rev_rotor_chain_3", "urdf_mini_cheetah", "tello_with_arms", "tree_generic_float", "urdf_mit_humanoid"])
def test_walks_follow_the_parent_table(name):
    plan, parent, _ = _tree(name)
    nb = plan.n_bodies
    rng = np.random.default_rng(5)
    lists = [[b] for b in range(nb)] + [list(range(min(nb, 16)))] + [list(range(max(nb - 16, 0), nb))]
    lists += [list(rng.integers(0, nb, size=int(rng.integers(1, 17)))) for _ in range(40)]
    for bodies in lists:
        n_walk, peak = _expected(parent, bodies)
        assert plan.body_list_walk(bodies) == (n_walk, peak, int(n_walk > MAX_WALK or peak > MAX_SAVED)), bodies


def test_a_list_past_the_cap_takes_the_full_kernel_and_a_gather():
    plan, parent, _ = _tree("parallel_chain_exp_d10_l16")
    nb = plan.n_bodies
    bodies = list(range(nb - 16, nb))  # sixteen bodies whose ancestors are all the others
    assert len(set().union(*[_path(parent, b) for b in bodies])) == nb == 20 > MAX_WALK
    assert plan.body_list_walk(bodies) == (20, 0, 1)
    shorter = bodies[:-1]  # without the last leaf: every body but that one
    assert not any(p == nb - 1 for p in parent) and len(set().union(*[_path(parent, b) for b in shorter])) == MAX_WALK
    assert plan.body_list_walk(shorter) == (MAX_WALK, 0, 0)  # (the cap itself is still a walk)


def test_python_argument_rules_without_a_device():
    import torch

    plan = _Call().plan
    q, z = torch.zeros((2, plan.nq), dtype=torch.float64), torch.zeros((2, plan.nv), dtype=torch.float64)
    with pytest.raises(G.GrbdaError):  # (host tensors: no CPU fallback)
        plan.body_poses_list(q, [0])
    with pytest.raises(G.GrbdaError):
        plan.body_twists_list(q, z, z, [0, 1])
    with pytest.raises(G.GrbdaError):
        plan.body_list_walk([plan.n_bodies])
