"""What the contact and kinematics entry points of the C ABI refuse, and in which order: (return code, grbda_last_error() text) of a
table of bad calls per entry point -- grbda_inv_osim_*, grbda_apply_test_force_*, grbda_contact_points_*, grbda_contact_dynamics_*,
grbda_body_poses_*, grbda_body_twists_*, grbda_rnea_derivatives_* (f64, f32 and the host-array variant of each) and
grbda_contact_solve_launch.

No device is needed: the argument checks run before any device call, and a machine without a device answers GRBDA_ENODEVICE to a call
that passes them.  That answer is part of the table -- it shows WHERE a check sits: grbda_inv_osim_host_f64 looks at the body indices
only after it has found its device, so a bad index there is GRBDA_ENODEVICE here.  On a machine WITH a device the rows recorded as
GRBDA_ENODEVICE are not called (the arrays of this file are host memory).

The rows of one entry point (rows(), from its argument list): the valid call; a null plan; each pointer argument null in turn; 0 and 9
contacts; body index -1 and n_bodies; negative and NaN damping; no output asked for; each output aliasing each input; each pair of
outputs aliasing; and every pair of a short list of faults at once (the first of the two messages pins the order of the checks).

EXPECTED was recorded on the PARENT of the commit that gave the contact side one contact-set check and one overlap rule (its library
built apart and selected with GRBDA_HIP_LIB; `PYTHONPATH=.:oracle:tests python tests/test_contact_args_cpu.py` prints the table), never
on the code under test."""
import ctypes
import itertools
from ctypes import POINTER, c_double, c_int, c_size_t, c_void_p

import pytest

import generalized_rbda_amd as G
from entry_points import _model

ENODEVICE = -3
NO_DEVICE = (ENODEVICE, "no HIP device available (there is no CPU fallback)")
# argument kinds: "in" / "out" arrays, with "?" where NULL is allowed; "n": contact count; "bodies" / "offsets": the host arrays of the
# contact description; "body": one body index; "damping", "step": scalars.  Every entry point ends (B, device[, stream]).
ENTRIES = {
    "inv_osim": [("q", "in"), ("n", "n"), ("bodies", "bodies"), ("offsets", "offsets"), ("Linv", "out"), ("J", "out?")],
    "apply_test_force": [("q", "in"), ("body", "body"), ("offset", "offsets"), ("force", "in"), ("lambda_inv", "out"), ("dstate", "out")],
    "contact_points": [("q", "in"), ("qd", "in?"), ("ydd", "in?"), ("n", "n"), ("bodies", "bodies"), ("offsets", "offsets"), ("pos", "out?"),
                       ("vel", "out?"), ("acc", "out?")],
    "contact_dynamics": [("q", "in"), ("qd", "in"), ("tau", "in"), ("f_ext", "in?"), ("n", "n"), ("bodies", "bodies"), ("offsets", "offsets"),
                         ("a_des", "in?"), ("damping", "damping"), ("ydd", "out"), ("lambda", "out"), ("ydd_free", "out?")],
    "body_poses": [("q", "in"), ("Xa", "out")],
    "body_twists": [("q", "in"), ("qd", "in"), ("ydd", "in"), ("V", "out")],
    "rnea_derivatives": [("q", "in"), ("qd", "in"), ("ydd", "in"), ("step", "step"), ("dq", "out?"), ("dqd", "out?"), ("dydd", "out?")],
}
VARIANTS = [f"{e}_{v}" for e in ENTRIES for v in ("f64", "f32", "host_f64")]
CTYPE = {"n": c_int, "body": c_int, "bodies": POINTER(c_int), "offsets": POINTER(c_double), "damping": c_double, "step": c_double}
N_CONTACTS = 2


@pytest.fixture(scope="module")
def plan():
    return G.Plan(_model("urdf_mini_cheetah"))


def _library():
    """a handle of its own on the library G.lib() loaded: the argument types set here stay here"""
    G.lib()
    L = ctypes.CDLL(G.LIB_PATH)
    L.grbda_last_error.restype = ctypes.c_char_p
    return L


def _valid(args, n_bodies):
    """name -> value of a call that passes every check: one 8 KiB array per pointer argument (B = 1: the largest, nv x nv, is 2.6 KB)"""
    call = {"keep": []}
    for name, kind in args:
        if kind.rstrip("?") in ("in", "out"):
            call["keep"].append((c_double * 1024)())
            call[name] = ctypes.addressof(call["keep"][-1])
        elif kind == "bodies":
            call[name] = [1, 2] + [1] * 7
        elif kind == "offsets":
            call["keep"].append((c_double * 27)())
            call[name] = call["keep"][-1]
        else:
            call[name] = {"n": N_CONTACTS, "body": 1, "damping": 0.0, "step": 1e-6}[kind]
    return call


def _set(name, value):
    return lambda c, nb: c.__setitem__(name, value)


def _body(name, at, value):
    return lambda c, nb: c[name].__setitem__(at, nb if value == "top" else value)


def _alias(dst, src):
    return lambda c, nb: c.__setitem__(dst, c[src])


def _both(*fs):
    def apply(c, nb):
        for f in fs:
            f(c, nb)
    return apply


def rows(args):
    """[(row id, change of the valid call)]"""
    of = lambda *kinds: [n for n, k in args if k in kinds]
    ins, outs, ptrs = of("in", "in?"), of("out", "out?"), of("in", "in?", "out", "out?", "bodies", "offsets")
    single = {"valid": lambda c, nb: None, "null-plan": _set("plan", None)}
    for name in ptrs:
        single[f"null-{name}"] = _set(name, None)
    if of("n"):
        single["n=0"], single["n=9"] = _set("n", 0), _set("n", 9)
        single["body=-1"], single["body=n_bodies"] = _body("bodies", 0, -1), _body("bodies", N_CONTACTS - 1, "top")
    if of("body"):
        single["body=-1"], single["body=n_bodies"] = _set("body", -1), lambda c, nb: c.__setitem__("body", nb)
    if of("damping"):
        single["damping<0"], single["damping=nan"] = _set("damping", -1.0), _set("damping", float("nan"))
    if not of("out"):
        single["no-output"] = _both(*[_set(o, None) for o in outs])
    for o in outs:
        for i in ins:
            single[f"{o}=={i}"] = _alias(o, i)
    for a, b in itertools.combinations(outs, 2):
        single[f"{b}=={a}"] = _alias(b, a)
    # two faults at once: every pair of these, the first applied first
    order = ["null-plan", f"null-{ins[0]}", "n=0", "body=-1", "damping<0", "no-output", f"{outs[0]}=={ins[0]}"]
    order += [f"{outs[1]}=={outs[0]}"] if len(outs) > 1 else []
    order = [k for k in order if k in single]
    out = list(single.items())
    out += [(f"{a} + {b}", _both(single[a], single[b])) for a, b in itertools.combinations(order, 2)]
    return out


def observe_variant(L, plan, variant, skip=()):
    """row id -> (return code, error text) of every row of one entry point; rows in `skip` are not called"""
    entry, host = next((e, variant.endswith("host_f64")) for e in ENTRIES if variant.startswith(e + "_"))
    args = ENTRIES[entry]
    fn = getattr(L, "grbda_" + variant)
    fn.argtypes = [c_void_p] + [CTYPE.get(k, c_void_p) for _, k in args] + [c_size_t, c_int] + ([] if host else [c_void_p])
    got = {}
    for rid, change in rows(args):
        if rid in skip:
            continue
        call = _valid(args, plan.n_bodies)
        call["plan"] = plan._h
        change(call, plan.n_bodies)
        values = []
        for name, kind in args:
            v = call[name]
            values.append((c_int * 9)(*v) if kind == "bodies" and v is not None else v)
        rc = fn(call["plan"], *values, 1, 0, *([] if host else [None]))
        got[rid] = (rc, L.grbda_last_error().decode() if rc else "")
    return got


def observe_solve_launch(L):
    """grbda_contact_solve_launch(n_contacts, precision, device = -1: no device asked for)"""
    fn = L.grbda_contact_solve_launch
    fn.argtypes = [c_int, c_int, c_int, POINTER(c_int), POINTER(c_size_t), POINTER(c_size_t)]
    lanes, lds, cap = c_int(), c_size_t(), c_size_t()
    got = {}
    for rid, n, prec, nulls in [("valid", 4, 64, ()), ("n=0", 0, 64, ()), ("n=9", 9, 32, ()), ("precision=16", 4, 16, ()), ("null-lanes", 4, 64, (0,)),
                                ("null-lds_bytes", 4, 64, (1,)), ("null-grid_cap", 4, 64, (2,)), ("n=0 + precision=16", 0, 16, ()),
                                ("n=9 + null-lanes", 9, 64, (0,))]:
        outs = [None if i in nulls else ctypes.byref(v) for i, v in enumerate((lanes, lds, cap))]
        rc = fn(n, prec, -1, *outs)
        got[rid] = (rc, L.grbda_last_error().decode() if rc else "")
    return got


# entry point (its f64, f32 and host variants alike, or the host variant apart) -> {(return code, text): [row ids]}, recorded on the parent
EINVAL = -1
_NULL, _PLAN, _BODY = (EINVAL, "null argument"), (EINVAL, "null plan"), (EINVAL, "body index out of range")
_IN, _OUT, _NONE = (EINVAL, "an output array overlaps an input array"), (EINVAL, "two output arrays overlap"), (EINVAL, "no output asked for")
_POINTS, _FRAMES = (EINVAL, "1..8 contact points per call"), (EINVAL, "1..8 contact frames per call")
EXPECTED = {
    "apply_test_force": {
        NO_DEVICE: ["valid", "lambda_inv==q", "lambda_inv==force", "dstate==q", "dstate==force", "dstate==lambda_inv",
                    "lambda_inv==q + dstate==lambda_inv"],
        _BODY: ["body=-1", "body=n_bodies", "body=-1 + lambda_inv==q", "body=-1 + dstate==lambda_inv"],
        _NULL: ["null-q", "null-offset", "null-force", "null-lambda_inv", "null-dstate", "null-q + body=-1", "null-q + lambda_inv==q",
                "null-q + dstate==lambda_inv"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + body=-1", "null-plan + lambda_inv==q", "null-plan + dstate==lambda_inv"]},
    "apply_test_force_host_f64": {
        NO_DEVICE: ["valid", "null-offset", "body=-1", "body=n_bodies", "lambda_inv==q", "lambda_inv==force", "dstate==q", "dstate==force",
                    "dstate==lambda_inv", "body=-1 + lambda_inv==q", "body=-1 + dstate==lambda_inv", "lambda_inv==q + dstate==lambda_inv"],
        _NULL: ["null-q", "null-force", "null-lambda_inv", "null-dstate", "null-q + body=-1", "null-q + lambda_inv==q",
                "null-q + dstate==lambda_inv"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + body=-1", "null-plan + lambda_inv==q", "null-plan + dstate==lambda_inv"]},
    "body_poses": {
        NO_DEVICE: ["valid", "Xa==q"],
        _NULL: ["null-q", "null-Xa", "null-q + Xa==q"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + Xa==q"]},
    "body_twists": {
        NO_DEVICE: ["valid", "V==q", "V==qd", "V==ydd"],
        _NULL: ["null-q", "null-qd", "null-ydd", "null-V", "null-q + V==q"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + V==q"]},
    "contact_dynamics": {
        NO_DEVICE: ["valid", "null-f_ext", "null-a_des", "null-ydd_free"],
        _POINTS: ["n=0", "n=9", "n=0 + body=-1", "n=0 + damping<0", "n=0 + ydd==q", "n=0 + lambda==ydd"],
        _IN: ["ydd==q", "ydd==qd", "ydd==tau", "ydd==f_ext", "ydd==a_des", "lambda==q", "lambda==qd", "lambda==tau", "lambda==f_ext",
              "lambda==a_des", "ydd_free==q", "ydd_free==qd", "ydd_free==tau", "ydd_free==f_ext", "ydd_free==a_des", "ydd==q + lambda==ydd"],
        _BODY: ["body=-1", "body=n_bodies", "body=-1 + damping<0", "body=-1 + ydd==q", "body=-1 + lambda==ydd"],
        (EINVAL, "damping must be finite and not negative"): ["damping<0", "damping=nan", "damping<0 + ydd==q", "damping<0 + lambda==ydd"],
        _NULL: ["null-q", "null-qd", "null-tau", "null-bodies", "null-offsets", "null-ydd", "null-lambda", "null-q + n=0", "null-q + body=-1",
                "null-q + damping<0", "null-q + ydd==q", "null-q + lambda==ydd"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + n=0", "null-plan + body=-1", "null-plan + damping<0", "null-plan + ydd==q",
                "null-plan + lambda==ydd"],
        _OUT: ["lambda==ydd", "ydd_free==ydd", "ydd_free==lambda"]},
    "contact_points": {
        NO_DEVICE: ["valid", "null-pos", "null-vel", "null-acc"],
        _POINTS: ["n=0", "n=9", "n=0 + body=-1", "n=0 + no-output", "n=0 + pos==q", "n=0 + vel==pos"],
        (EINVAL, "acc needs ydd"): ["null-ydd"],
        _IN: ["pos==q", "pos==qd", "pos==ydd", "vel==q", "vel==qd", "vel==ydd", "acc==q", "acc==qd", "acc==ydd", "no-output + pos==q",
              "pos==q + vel==pos"],
        _BODY: ["body=-1", "body=n_bodies", "body=-1 + no-output", "body=-1 + pos==q", "body=-1 + vel==pos"],
        _NONE: ["no-output", "no-output + vel==pos"],
        _NULL: ["null-q", "null-bodies", "null-offsets", "null-q + n=0", "null-q + body=-1", "null-q + no-output", "null-q + pos==q",
                "null-q + vel==pos"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + n=0", "null-plan + body=-1", "null-plan + no-output", "null-plan + pos==q",
                "null-plan + vel==pos"],
        _OUT: ["vel==pos", "acc==pos", "acc==vel"],
        (EINVAL, "vel and acc need qd"): ["null-qd"]},
    "contact_solve_launch": {
        _POINTS: ["n=0", "n=9"],
        (EINVAL, "bad argument"): ["precision=16", "null-lanes", "null-lds_bytes", "null-grid_cap", "n=0 + precision=16", "n=9 + null-lanes"],
        (0, ""): ["valid"]},
    "inv_osim": {
        NO_DEVICE: ["valid", "null-J", "Linv==q", "J==q", "J==Linv", "Linv==q + J==Linv"],
        _FRAMES: ["n=0", "n=9", "n=0 + body=-1", "n=0 + Linv==q", "n=0 + J==Linv"],
        _BODY: ["body=-1", "body=n_bodies", "body=-1 + Linv==q", "body=-1 + J==Linv"],
        _NULL: ["null-q", "null-bodies", "null-offsets", "null-Linv", "null-q + n=0", "null-q + body=-1", "null-q + Linv==q", "null-q + J==Linv"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + n=0", "null-plan + body=-1", "null-plan + Linv==q", "null-plan + J==Linv"]},
    "inv_osim_host_f64": {
        NO_DEVICE: ["valid", "null-bodies", "null-offsets", "null-J", "body=-1", "body=n_bodies", "Linv==q", "J==q", "J==Linv",
                    "body=-1 + Linv==q", "body=-1 + J==Linv", "Linv==q + J==Linv"],
        _FRAMES: ["n=0", "n=9", "n=0 + body=-1", "n=0 + Linv==q", "n=0 + J==Linv"],
        _NULL: ["null-q", "null-Linv", "null-q + n=0", "null-q + body=-1", "null-q + Linv==q", "null-q + J==Linv"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + n=0", "null-plan + body=-1", "null-plan + Linv==q", "null-plan + J==Linv"]},
    "rnea_derivatives": {
        NO_DEVICE: ["valid", "null-dq", "null-dqd", "null-dydd"],
        _IN: ["dq==q", "dq==qd", "dq==ydd", "dqd==q", "dqd==qd", "dqd==ydd", "dydd==q", "dydd==qd", "dydd==ydd", "no-output + dq==q",
              "dq==q + dqd==dq"],
        _NONE: ["no-output", "no-output + dqd==dq"],
        _NULL: ["null-q", "null-qd", "null-ydd", "null-q + no-output", "null-q + dq==q", "null-q + dqd==dq"],
        _PLAN: ["null-plan", "null-plan + null-q", "null-plan + no-output", "null-plan + dq==q", "null-plan + dqd==dq"],
        _OUT: ["dqd==dq", "dydd==dq", "dydd==dqd"]},
}


def _expected(variant):
    """row id -> (return code, text) of `variant` on the parent"""
    table = EXPECTED.get(variant) or EXPECTED[next(e for e in ENTRIES if variant.startswith(e + "_"))]
    return {rid: outcome for outcome, ids in table.items() for rid in ids}


@pytest.mark.parametrize("variant", VARIANTS)
def test_refusals_and_their_order(variant, plan):
    want = _expected(variant)
    assert sorted(want) == sorted(rid for rid, _ in rows(ENTRIES[next(e for e in ENTRIES if variant.startswith(e + "_"))]))
    past_the_checks = [rid for rid, (rc, _) in want.items() if rc == ENODEVICE] if G.device_count() > 0 else []
    got = observe_variant(_library(), plan, variant, skip=past_the_checks)
    wrong = {rid: (got[rid], want[rid]) for rid in got if got[rid] != want[rid]}
    assert not wrong, f"{variant}: (got, parent) {wrong}"
    assert len(got) + len(past_the_checks) == len(want)


def test_contact_solve_launch_refusals():
    got = observe_solve_launch(_library())
    assert got == _expected("contact_solve_launch")


if __name__ == "__main__":
    import pprint

    L, p = _library(), G.Plan(_model("urdf_mini_cheetah"))
    table = {v: observe_variant(L, p, v) for v in VARIANTS}
    for e in ENTRIES:  # one table per entry point where its three variants answer alike, else the host variant's apart
        assert table.pop(e + "_f32") == table[e + "_f64"]
        table[e] = table.pop(e + "_f64")
        if table[e + "_host_f64"] == table[e]:
            del table[e + "_host_f64"]
    table["contact_solve_launch"] = observe_solve_launch(L)
    grouped = {}
    for v, got in table.items():
        for rid, outcome in got.items():
            grouped.setdefault(v, {}).setdefault(outcome, []).append(rid)
    print("EXPECTED = " + pprint.pformat(grouped, width=150, compact=True).replace(repr(NO_DEVICE), "NO_DEVICE"))
