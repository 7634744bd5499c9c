"""The fp32 chain forward dynamics that keeps a tile's inputs in registers (aba_chain_kernel<float, 2, 3>) against the fp64 oracle, over the
edges of its tile prologue and either side of its dispatch rule (run with -m gpu).

The prologue copies the tile's q, qd and tau into LDS and every lane reads its own row into three register arrays of 32 entries
(devmath.h, stage_inputs_reg): 16-byte reads when the column count is a multiple of four, 4-byte reads otherwise; all three blocks at once
when the wavefront's LDS holds them, one after the other when it does not.  What can go wrong is a column in the wrong register, a row of
the wrong lane, or a ragged tile reading past its rows, so:

* batches of 1, 63, 64, 65 and 129 states (a lone lane, a tile short of one lane, a full tile, a second tile of one lane, two tiles and one
  lane) -- plans compiled with latency mode off, so that these small batches run the one-wavefront kernel the large ones run;
* MIT Humanoid (25 columns of q: 4-byte reads; 24 of qd and tau: 16-byte reads), Mini Cheetah (19 and 18: neither a multiple of four) and
  the fixed-base chain of links with rotors (a run that starts on the ground);
* the dispatch rule (devplan.h, chain_inputs_in_registers): eight limbs of four links on the ground, nq = nv = 32, run the in-register
  kernel -- its 96 staged rows exceed the wavefront's LDS, so this is also the one-array-at-a-time prologue -- the same with one limb of
  five, nq = nv = 33, runs the slab kernel, and so does ONE chain of 32 links, whose [sin, cos, v] blocks overflow LDS into the slab.

Every case holds TOL32 of tests/test_gpu_parity.py in its measure (rel_err) against the oracle on the same fp32-representable inputs."""
import functools
import os

import numpy as np
import pytest

import generalized_rbda_amd as G
import oracle_py as O
import term_states as TS
from generalized_rbda_amd import modeldesc as md
from models import ROBOT_MODELS, valid_states

pytestmark = pytest.mark.gpu
TOL32 = 1e-3
BATCHES = (1, 63, 64, 65, 129)
URDFS = ("mit_humanoid", "mini_cheetah", "revolute_rotor_chain")
INREG, SLAB = "aba_chain_kernel<float, 2, 3>", "aba_chain_kernel<float, 2, 0>"
# limbs (links each) on the ground -> the kernel its fp32 forward dynamics runs
BOUNDARY = {"limbs_8x4_nv32": ((4,) * 8, INREG), "limbs_7x4_5_nv33": ((4,) * 7 + (5,), SLAB), "chain_32_nv32": ((32,), SLAB)}


def rel_err(a, b):
    """max over states of ||a - b||_inf / (1 + ||b||_inf)   (tests/test_gpu_parity.py)"""
    return float((np.abs(a - b).max(axis=1) / (1.0 + np.abs(b).max(axis=1))).max())


def limbs_on_the_ground(limbs):
    """serial limbs of revolute links with rotors, all rooted on the ground; every limb and link with a tree transform of its own"""
    m = md.ClusterTreeModel(gravity=(0.0, 0.0, -9.81))
    link_I = md.spatial_inertia(1.0, [0.5, 0.0, 0.0], np.diag([0.02, 0.03, 1.0]))
    rotor_I = md.spatial_inertia(0.0, [0.0, 0.0, 0.0], np.diag([0.0, 0.0, 1e-4]))
    for a, n in enumerate(limbs):
        prev = "ground"
        for i in range(n):
            E = md.coordinate_rotation("x", 0.3 * a + 0.2 * i)
            r = [0.1 * a, 0.0, 0.0] if i == 0 else [1.0, 0.0, 0.0]
            m.registerBody(f"link-{a}-{i}", link_I, prev, E, r)
            m.registerBody(f"rotor-{a}-{i}", rotor_I, prev, E, r)
            m.appendRegisteredBodiesAsCluster(f"cluster-{a}-{i}", "RevoluteWithRotor", joint_axis="z", rotor_axis="z", gear_ratio=6.0)
            prev = f"link-{a}-{i}"
    return m.serialize()


@functools.lru_cache(maxsize=None)
def case(model):
    """(plan with latency mode off, q, qd, tau rounded to fp32, fp64 oracle) for the largest batch; the smaller ones are its first rows"""
    blob = limbs_on_the_ground(BOUNDARY[model][0]) if model in BOUNDARY else G.urdf_to_blob(os.path.join(ROBOT_MODELS, model + ".urdf"))
    q, qd, tau = (TS._frozen(TS.fp32_rounded(a)) for a in valid_states(blob, max(BATCHES), config_index=23))
    return TS.compile_under(blob, TS.ROUTES["chain"][0]), q, qd, tau, TS._frozen(O.forward_dynamics(blob, q, qd, tau))


def run(plan, q, qd, tau, B, gpu):
    import torch

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[:B]), dtype=torch.float32, device=gpu)
    out = plan.forward_dynamics(t(q), t(qd), t(tau))
    torch.cuda.synchronize()
    return out.double().cpu().numpy()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("model", URDFS)
def test_prologue_edges_match_oracle(model, B, gpu):
    plan, q, qd, tau, ref = case(model)
    name = plan.kernel_name("aba", "f32", B)
    assert INREG in name, name
    got = run(plan, q, qd, tau, B, gpu)
    err = rel_err(got, ref[:B])
    print(f"INREG {model} B={B} nq={plan.nq} nv={plan.nv} {name}: rel err {err:.2e}")
    assert got.shape == (B, plan.nv) and np.isfinite(got).all()
    assert err < TOL32


@pytest.mark.parametrize("B", (64, 65))
@pytest.mark.parametrize("model", list(BOUNDARY))
def test_dispatch_boundary(model, B, gpu):
    plan, q, qd, tau, ref = case(model)
    limbs, kernel = BOUNDARY[model]
    assert plan.nq == plan.nv == sum(limbs)
    name = plan.kernel_name("aba", "f32", B)
    assert kernel in name, name
    got = run(plan, q, qd, tau, B, gpu)
    err = rel_err(got, ref[:B])
    print(f"INREG {model} B={B} nq={plan.nq} nv={plan.nv} {name}: rel err {err:.2e}")
    assert np.isfinite(got).all()
    assert err < TOL32
