"""The numpy reference of centroidal_ref.py is pinned to the oracle (no GPU), each check per state on the quantity's own scale
(centroidal_ref.scale_error) at entry_points.TOL64:

  * kinetic = 1/2 yd^T H yd with the oracle's mass matrix, A yd = h, the total mass = the sum of the description's body masses;
  * momentum balance, the floating-base models: with ydd the ORACLE's forward dynamics and no external force, hdot = [0; M g]; with a
    random f_ext, hdot = [0; M g] + the wrenches taken about the centre of mass.  The identity restates nothing of ours: it ties the
    oracle's forward dynamics to the kinematics and the sums of the reference;
  * the float32 run of the reference leaves out at most term_states.MAX_LEFT_OUT of the batch under term_states.FLOOR for every
    (model, output) the fp32 GPU test runs, and is a yardstick: its own error is not zero.

BALANCE_WORST is the worst value the balance identity has shown in this reference, on the 65 states of the device test and relative
to 1 + max_j |A[:, j]| |ydd|_inf, the measure of the device test, over FLOATING and both cases.  It is rounding noise of a sum that
cancels (about 20 eps), and it depends on the host: the same code measured 1.0e-15 on one machine (tree_mixed_float with f_ext; 6.8e-16
without) and 4.9e-15 on another (tree_mixed_float without f_ext); the other three models stay under 4e-17 on both.  The constant is the
larger of the two, and test_centroidal_gpu.py bounds the device by ten times it.  The test below prints the value it measures and does not
hold it to the constant -- a third host may round differently again; what it asserts is the identity on its own scale at TOL64.  In the
balance cases tau acts on the joints only: a generalized force on the floating base IS an external wrench."""
import functools

import numpy as np
import pytest

import centroidal_ref as C
import entry_points as EP
import kinematics_ref as K
import oracle_py as O
import term_states as TS
from models import zoo

PIN_MODELS = list(zoo())
FLOATING = ("urdf_mini_cheetah", "urdf_mit_humanoid", "tello_with_arms", "tree_mixed_float")
N_PIN = 16
SEED = 83
BALANCE_WORST = 4.9e-15  # the largest measured on any host so far (tree_mixed_float, no f_ext); see the module docstring


@functools.lru_cache(maxsize=None)
def pin_states(name, B=N_PIN):
    blob = EP._model(name)
    return blob, tuple(TS._frozen(a) for a in EP._states(blob, B, SEED))


def balance_scale(A, ydd):
    """1 + max_j |A[:, j]|_inf |ydd|_inf per state: the size of the terms that cancel in hdot"""
    return 1.0 + np.abs(A).max(axis=(1, 2)) * np.abs(ydd).max(axis=1)


def internal_forces(blob, tau):
    """tau with the floating base's six entries zero: a generalized force on the base is an external wrench, the joints' are internal"""
    tau = np.array(tau)
    for cl in K._parse(blob)["clusters"]:
        if cl[9] == 1:
            tau[:, cl[5]:cl[5] + 6] = 0.0
    return tau


def balance_cases(blob, q, qd, tau, forward_dynamics):
    """[(case, hdot reference [B, 6], ydd, f_ext)] of the momentum balance with the given forward dynamics; tau acts on the joints only"""
    B, nb = q.shape[0], K._parse(blob)["nb"]
    tau = internal_forces(blob, tau)
    g = K._parse(blob)["grav"][3:]
    ref0 = C.centroidal(blob, q)
    gravity = np.concatenate([np.zeros((B, 3)), np.broadcast_to(ref0["mass"] * g, (B, 3))], axis=1)
    f_ext = np.random.default_rng(SEED).uniform(-1, 1, (B, nb, 6))
    return [("free", gravity, forward_dynamics(q, qd, tau, None), None),
            ("f_ext", gravity + C.wrench_about(ref0["com"], f_ext), forward_dynamics(q, qd, tau, f_ext), f_ext)]


@pytest.mark.parametrize("name", PIN_MODELS)
def test_energy_momentum_and_mass_are_the_oracle_s(name):
    blob, (q, qd, _) = pin_states(name)
    ref = C.centroidal(blob, q, qd)
    H = EP._mass_oracle(blob, q)
    ke = 0.5 * np.einsum("bi,bij,bj->b", qd, H, qd)
    e_ke = C.scale_error(ref["kinetic"], ke).max()
    A = C.momentum_matrix(blob, q)
    e_A = C.scale_error(np.einsum("bij,bj->bi", A, qd), ref["h"]).max()
    masses = [bd["I"][3, 3] for bd in K._parse(blob)["bodies"]]
    print(f"{name}: kinetic against yd^T H yd / 2 {e_ke:.1e}; A yd against h {e_A:.1e}; mass {ref['mass']:.6g}")
    assert e_ke < EP.TOL64 and e_A < EP.TOL64
    assert ref["mass"] == C.total_mass(blob) == pytest.approx(sum(masses), rel=1e-15) and ref["mass"] > 0
    # the linear momentum is M c_dot, and the potential energy -M g . c
    assert C.scale_error(ref["h"][:, 3:], ref["mass"] * ref["com_vel"]).max() < EP.TOL64
    assert C.scale_error(ref["potential"], -ref["mass"] * ref["com"] @ K._parse(blob)["grav"][3:]).max() < EP.TOL64


@pytest.mark.parametrize("name", FLOATING)
def test_momentum_balance_with_the_oracle_s_forward_dynamics(name):
    """on the states of the device test (test_centroidal_gpu.test_momentum_balance_and_identities_on_the_device)"""
    import test_centroidal_gpu as TC

    blob = EP._model(name)
    q, qd, tau = (a[:TC.B_BALANCE] for a in TC.draw(name, False))
    A = C.momentum_matrix(blob, q)
    for case, want, ydd, _ in balance_cases(blob, q, qd, tau, lambda q, qd, tau, fe: O.forward_dynamics(blob, q, qd, tau, fe)):
        hdot = C.centroidal(blob, q, qd, ydd)["hdot"]
        own = C.scale_error(hdot, want).max()
        rel = (np.abs(hdot - want).max(axis=1) / balance_scale(A, ydd)).max()
        print(f"{name} {case}: hdot against gravity + wrenches {own:.1e} on its own scale, {rel:.1e} of 1 + max_j |A_j| |ydd|")
        assert own < EP.TOL64


def test_the_float32_run_leaves_out_no_more_than_the_cap():
    import test_centroidal_gpu as TC

    for name, out in TC.CASES32:
        ref64, ref32 = TC.references32(name)
        ref, fl = TC.rows(ref64[out]), TC.rows(ref32[out])
        assert TS.left_out(ref) <= TS.MAX_LEFT_OUT, (name, out, TS.left_out(ref))
        assert 0 < TS.term_error(fl, ref).max() < 1e-4, (name, out, TS.term_error(fl, ref).max())
    assert set(TC.MARGINS) <= set(TC.CASES32) and not set(TC.NOT_RUN) & set(TC.CASES32)
    assert all(margin > TS.MARGIN and abs(margin - 2 * worst) < 0.1 for margin, (worst, _), _ in TC.MARGINS.values())
