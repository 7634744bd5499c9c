"""Latency mode against the ORACLE (aba_chain_lm_kernel / rnea_chain_lm_kernel<T, 2 | 4>), not against another kernel.

Batches of at most one tile per SIMD run a tile on a workgroup of two wavefronts, batches of at most two tiles per CU on four when
the base carries four limbs or more; the limbs below the floating base are dealt out to the wavefronts.  Models: every zoo model
whose latency-mode programs are built, eight models of the generated family of tests/test_lds_schedule_cpu.py that have the shape
the round-6 review found racy (a wavefront owns two direct limbs, the last direct limb in program order has kid chains and runs on
another wavefront), and TelloWithArms with the arms before the legs.  Forward and inverse dynamics, fp32 and -- where the program
exists -- fp64, at 1 state, 64 * 2 * n_cu states (four wavefronts where the program exists), 64 * 2 * n_cu + 1 (two) and 1 000
states of a GRBDA_LM_WAVES=2 plan.  The kernel name of every launch is asserted, from a table of the programs each model has, so
that the test fails when the selection thresholds or the plan compiler move instead of quietly testing another kernel.

A GPU run cannot prove that a schedule has no race between wavefronts: a race decided by timing passes most of the time.  The
deterministic guard is the host-side schedule checker (tests/cpp/lds_schedule_check.cpp); this test is the end-to-end parity."""
import numpy as np
import pytest

import oracle_py as O
import generalized_rbda_amd as G
from models import lds_family, tello_with_arms_arms_first, valid_states, zoo

pytestmark = pytest.mark.gpu

TOL64 = 1e-9
TOL32 = 1e-3

# the latency-mode programs each model has (plan.h: chain32p / chain64p two wavefronts, ...q four; r...: inverse dynamics), as the
# plan compiler builds them with capi.cpp's budgets (build/lds_check/lds_schedule_check prints them)
_ALL = "chain32p chain32q rchain32p rchain32q"
PROGRAMS = {
    "chain_tree_a": _ALL,
    "chain_tree_b": _ALL,
    "chain_tree_norotor": _ALL + " chain64q",
    "chain_tree_rpy": "chain32p rchain32p",
    "tello": "chain32p rchain32p",
    "tello_with_arms": _ALL,
    "tree_chain_rev_float": "chain32p rchain32p",
    "tree_rotor_float": "chain32p chain64p rchain32p",
    "urdf_mini_cheetah": _ALL + " chain64p chain64q rchain64p rchain64q",
    "urdf_mini_cheetah_rpy": _ALL + " chain64p chain64q rchain64p rchain64q",
    "urdf_mit_humanoid": _ALL + " chain64p chain64q",
    "tello_with_arms_arms_first": _ALL,
}
FAMILY = ["chain_tree_l6_flat_s0", "chain_tree_l6_flat_s8", "chain_tree_l5_flat_s2", "chain_tree_l5_flat_s6", "chain_tree_l5_flat_s4",
          "chain_tree_l6_deep_s5", "chain_tree_l6_deep_s3", "chain_tree_l5_deep_s4"]
PROGRAMS.update({name: _ALL for name in FAMILY})


def _blob(name):
    if name == "tello_with_arms_arms_first":
        return tello_with_arms_arms_first().serialize()
    if name in FAMILY:
        return lds_family()[name].serialize()
    return zoo()[name]


def rel_err(a, b):
    """max over states of ||a - b||_inf / (1 + ||b||_inf)"""
    return float((np.abs(a - b).max(axis=1) / (1.0 + np.abs(b).max(axis=1))).max())


def test_the_table_covers_every_zoo_model_with_latency_mode():
    """A zoo model that gains or loses the forward dynamics' latency mode must be added to / removed from PROGRAMS."""
    for name, blob in zoo().items():
        info = G.Plan(blob).info()
        has = set(PROGRAMS.get(name, "").split())
        assert bool(info.latency_mode_f32) == ("chain32p" in has), name
        assert bool(info.latency_mode_f64) == ("chain64p" in has), name


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_latency_mode_matches_the_oracle(name, gpu, monkeypatch):
    import torch

    blob = _blob(name)
    has = set(PROGRAMS[name].split())
    plan = G.Plan(blob)
    monkeypatch.setenv("GRBDA_LM_WAVES", "2")
    two = G.Plan(blob)
    monkeypatch.delenv("GRBDA_LM_WAVES")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    big = 64 * 2 * n_cu
    oracle = {"aba": O.forward_dynamics, "rnea": O.inverse_dynamics}
    # one draw of states for every batch (the implicit-loop models project theirs onto the constraint manifold: seconds per draw)
    states = valid_states(blob, big + 1, config_index=90)
    checked = 0
    for algo, pre in (("aba", "chain"), ("rnea", "rchain")):
        for dt, bits in ((torch.float32, "32"), (torch.float64, "64")):
            p2, p4 = pre + bits + "p" in has, pre + bits + "q" in has
            if not (p2 or p4):
                continue
            T = "float" if bits == "32" else "double"
            tag = "f" + bits
            runs = []
            for B in (1, big):  # at most two tiles per CU: four wavefronts where that program exists
                assert f"lm_kernel<{T}, {4 if p4 else 2}" in plan.kernel_name(algo, tag, B), (algo, tag, B, plan.kernel_name(algo, tag, B))
                runs.append((plan, B))
            name_2 = plan.kernel_name(algo, tag, big + 1)
            if p2:
                assert f"lm_kernel<{T}, 2" in name_2, (algo, tag, name_2)
                assert f"lm_kernel<{T}, 2" in two.kernel_name(algo, tag, 1000), (algo, tag, two.kernel_name(algo, tag, 1000))
                runs += [(plan, big + 1), (two, 1000)]
            else:
                assert "lm_kernel" not in name_2, (algo, tag, name_2)
            for pl, B in runs:
                q, qd, x = (a[:B] for a in states)
                if dt == torch.float32:  # (inputs the fp32 kernel holds exactly: the oracle sees the same state)
                    q, qd, x = (a.astype(np.float32).astype(np.float64) for a in (q, qd, x))
                t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=gpu)
                fn = pl.forward_dynamics if algo == "aba" else pl.inverse_dynamics
                got = fn(t(q), t(qd), t(x))
                torch.cuda.synchronize()
                got = got.double().cpu().numpy()
                ref = oracle[algo](blob, q, qd, x)
                err = rel_err(got, ref)
                assert err < (TOL32 if bits == "32" else TOL64), f"{algo} {tag} B={B} ({pl.kernel_name(algo, tag, B)}): {err:.2e}"
                checked += 1
    assert checked >= 4
