"""Model zoo for the tests: the reference's uniform chains plus seeded random cluster trees that
exercise every explicit cluster-joint type the reference has (testRigidBodyDynamicsAlgos.cpp:94-109
uses the same families with random parameters)."""
import os

import numpy as np

from generalized_rbda_amd import modeldesc as md


def random_inertia(rng, massless=False):
    """A physically valid random spatial inertia (randomBody, include/grbda/Dynamics/Body.h:45-60)."""
    m = 0.0 if massless else rng.uniform(0.2, 2.0)
    com = rng.uniform(-0.3, 0.3, 3)
    A = rng.uniform(-1, 1, (3, 3))
    I3 = A @ A.T * 0.05 + np.eye(3) * rng.uniform(1e-3, 0.05)
    return md.spatial_inertia(m, com, I3)


def axisym_rotor_inertia(rng, axis, massless=False):
    """A rotor whose inertia is invariant under rotation about its joint axis (COM on the axis, equal transverse
    inertias) -- what the reference's geared rotors are (MIT_Humanoid.hpp:46-66) and what the plan compiler's q = 0
    shortcut and the chain kernels rely on."""
    a, b = rng.uniform(1e-4, 5e-3), rng.uniform(1e-4, 5e-3)
    I3 = np.eye(3) * a
    k = "xyz".index(axis)
    I3[k, k] = b
    com = np.zeros(3)
    com[k] = rng.uniform(-0.05, 0.05)
    return md.spatial_inertia(0.0 if massless else rng.uniform(0.02, 0.2), com, I3)


def random_xtree(rng):
    return md.rpy_to_rotmat(rng.uniform(-1, 1, 3)), rng.uniform(-0.5, 0.5, 3)


def random_cluster_tree(seed, n_clusters=8, floating=True, kinds=("rev", "rotor", "pair", "triple", "generic"),
                        ori_repr="quaternion"):
    """Random tree of clusters.  Every cluster hangs off ONE body of an earlier cluster."""
    rng = np.random.default_rng(seed)
    m = md.ClusterTreeModel(gravity=(0.0, 0.0, -9.81), ori_repr=ori_repr)
    link_names = []
    if floating:
        m.appendBody("base", random_inertia(rng), "ground", joint="free")
        link_names.append("base")
    ax = lambda: "xyz"[rng.integers(3)]
    for c in range(n_clusters):
        parent = "ground" if not link_names else link_names[rng.integers(len(link_names))]
        if not link_names and floating is False and c > 0:
            parent = link_names[rng.integers(len(link_names))]
        kind = kinds[rng.integers(len(kinds))]
        if kind == "rev":
            E, r = random_xtree(rng)
            m.appendBody(f"l{c}", random_inertia(rng), parent, E, r, joint="revolute", axis=ax())
            link_names.append(f"l{c}")
        elif kind == "rotor":
            E, r = random_xtree(rng)
            m.registerBody(f"l{c}", random_inertia(rng), parent, E, r)
            E2, r2 = random_xtree(rng)
            m.registerBody(f"r{c}", random_inertia(rng, massless=rng.random() < 0.5), parent, E2, r2)
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevoluteWithRotor", joint_axis=ax(), rotor_axis=ax(),
                                              gear_ratio=rng.uniform(2, 12))
            link_names.append(f"l{c}")
        elif kind == "axirotor":  # RevoluteWithRotor with an axisymmetric rotor (the shape of every geared joint of the reference's robots)
            E, r = random_xtree(rng)
            m.registerBody(f"l{c}", random_inertia(rng), parent, E, r)
            E2, r2 = random_xtree(rng)
            ra = ax()
            m.registerBody(f"r{c}", axisym_rotor_inertia(rng, ra, massless=rng.random() < 0.3), parent, E2, r2)
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevoluteWithRotor", joint_axis=ax(), rotor_axis=ra,
                                              gear_ratio=rng.uniform(2, 12))
            link_names.append(f"l{c}")
        elif kind == "axipair":  # leaf RevolutePairWithRotor with axisymmetric rotors (MIT humanoid knee / ankle)
            X = [random_xtree(rng) for _ in range(4)]
            ra = ax() + ax()
            order = rng.permutation(3)  # registration order of [rotor2, link1, rotor1] varies; link2 comes after link1
            regs = {}
            for o in order:
                if o == 0:
                    regs["r2"] = m.registerBody(f"r2_{c}", axisym_rotor_inertia(rng, ra[1]), parent, *X[0])
                elif o == 1:
                    regs["l1"] = m.registerBody(f"l1_{c}", random_inertia(rng), parent, *X[1])
                else:
                    regs["r1"] = m.registerBody(f"r1_{c}", axisym_rotor_inertia(rng, ra[0]), parent, *X[2])
            regs["l2"] = m.registerBody(f"l2_{c}", random_inertia(rng), f"l1_{c}", *X[3])
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevolutePairWithRotor", link1=regs["l1"], rotor1=regs["r1"],
                                              rotor2=regs["r2"], link2=regs["l2"], joint_axes=ax() + ax(), rotor_axes=ra,
                                              gear_ratios=rng.uniform(2, 10, 2), belt_ratios_1=rng.uniform(1, 3, 1),
                                              belt_ratios_2=rng.uniform(1, 3, 2))
            # a leaf cluster: nothing hangs off it
        elif kind == "pair":
            # MIT-humanoid knee/ankle registration order: [rotor2, link1, rotor1, link2]
            X = [random_xtree(rng) for _ in range(4)]
            r2 = m.registerBody(f"r2_{c}", random_inertia(rng), parent, *X[0])
            l1 = m.registerBody(f"l1_{c}", random_inertia(rng), parent, *X[1])
            r1 = m.registerBody(f"r1_{c}", random_inertia(rng), parent, *X[2])
            l2 = m.registerBody(f"l2_{c}", random_inertia(rng), f"l1_{c}", *X[3])
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevolutePairWithRotor", link1=l1, rotor1=r1, rotor2=r2,
                                              link2=l2, joint_axes=ax() + ax(), rotor_axes=ax() + ax(),
                                              gear_ratios=rng.uniform(2, 10, 2), belt_ratios_1=rng.uniform(1, 3, 1),
                                              belt_ratios_2=rng.uniform(1, 3, 2))
            link_names += [f"l1_{c}", f"l2_{c}"]
        elif kind == "triple":
            names = [f"t{c}_l{i}" for i in range(3)]
            par = parent
            for nm in names:
                m.registerBody(nm, random_inertia(rng), par, *random_xtree(rng))
                par = nm
            for i in range(3):
                m.registerBody(f"t{c}_r{i}", random_inertia(rng), parent, *random_xtree(rng))
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevoluteTripleWithRotor", joint_axes=ax() + ax() + ax(),
                                              rotor_axes=ax() + ax() + ax(), gear_ratios=rng.uniform(2, 8, 3),
                                              belt_ratios_1=rng.uniform(1, 2, 1), belt_ratios_2=rng.uniform(1, 2, 2),
                                              belt_ratios_3=rng.uniform(1, 2, 3))
            link_names += names
        else:  # generic static: k bodies in a random in-cluster tree, random coupling G
            # ("generic_big": beyond the structured kernels' 8 bodies / 4 coordinates -- the spanning-tree route)
            k = int(rng.integers(9, 21)) if kind == "generic_big" else int(rng.integers(2, 6))
            n = int(rng.integers(5, min(k, 12) + 1)) if kind == "generic_big" else int(rng.integers(1, min(k, 4) + 1))
            names = [f"g{c}_{i}" for i in range(k)]
            for i, nm in enumerate(names):
                par = parent if i == 0 or rng.random() < 0.4 else names[rng.integers(i)]
                m.registerBody(nm, random_inertia(rng), par, *random_xtree(rng))
            ind = sorted(rng.choice(k, size=n, replace=False).tolist())
            dep = [i for i in range(k) if i not in ind]
            G = np.zeros((k, n))
            K = np.zeros((k - n, k))
            for j, i in enumerate(ind):
                G[i, j] = 1.0
            for r_, i in enumerate(dep):
                w = rng.uniform(-3, 3, n) if kind != "generic_big" else rng.uniform(-1, 1, n) * (rng.random(n) < 0.4)
                G[i] = w
                K[r_, i] = -1.0
                for j, ii in enumerate(ind):
                    K[r_, ii] = w[j]
            m.appendRegisteredBodiesAsCluster(f"c{c}", "Generic", axes=[ax() for _ in range(k)], G=G, K=K)
            link_names += names
    return m


def chain_test_tree(seed, n_limbs=4, ori_repr="quaternion", rotors=True, deep_pairs=False):
    """A floating-base robot of the kind the chain-structured kernels cover (plan.h, ChainProgram): limbs that are
    chains of revolute links (with axisymmetric rotors when `rotors`), some ending in a leaf RevolutePairWithRotor
    cluster, some branching into two sub-chains half way down.  deep_pairs: pair clusters also sit in the middle of a limb
    (child clusters on their second link) and directly on the base -- the explicit pairs that run through the
    differential's segments (plan.cpp, class 6)."""
    rng = np.random.default_rng(seed)
    m = md.ClusterTreeModel(gravity=(0.0, 0.0, -9.81), ori_repr=ori_repr)
    m.appendBody("base", random_inertia(rng), "ground", joint="free")
    ax = lambda: "xyz"[rng.integers(3)]
    count = [0]

    def link(parent):
        c = count[0]
        count[0] += 1
        E, r = random_xtree(rng)
        if rotors and rng.random() < 0.8:
            m.registerBody(f"l{c}", random_inertia(rng), parent, E, r)
            ra = ax()
            m.registerBody(f"r{c}", axisym_rotor_inertia(rng, ra, massless=rng.random() < 0.3), parent, *random_xtree(rng))
            m.appendRegisteredBodiesAsCluster(f"c{c}", "RevoluteWithRotor", joint_axis=ax(), rotor_axis=ra, gear_ratio=rng.uniform(2, 12))
        else:
            m.appendBody(f"l{c}", random_inertia(rng), parent, E, r, joint="revolute", axis=ax())
        return f"l{c}"

    def pair(parent):
        c = count[0]
        count[0] += 1
        X = [random_xtree(rng) for _ in range(4)]
        ra = ax() + ax()
        regs = {}
        for o in rng.permutation(3):
            if o == 0:
                regs["r2"] = m.registerBody(f"r2_{c}", axisym_rotor_inertia(rng, ra[1]), parent, *X[0])
            elif o == 1:
                regs["l1"] = m.registerBody(f"l1_{c}", random_inertia(rng), parent, *X[1])
            else:
                regs["r1"] = m.registerBody(f"r1_{c}", axisym_rotor_inertia(rng, ra[0]), parent, *X[2])
        regs["l2"] = m.registerBody(f"l2_{c}", random_inertia(rng), f"l1_{c}", *X[3])
        m.appendRegisteredBodiesAsCluster(f"c{c}", "RevolutePairWithRotor", link1=regs["l1"], rotor1=regs["r1"], rotor2=regs["r2"],
                                          link2=regs["l2"], joint_axes=ax() + ax(), rotor_axes=ra, gear_ratios=rng.uniform(2, 10, 2),
                                          belt_ratios_1=rng.uniform(1, 3, 1), belt_ratios_2=rng.uniform(1, 3, 2))
        return f"l2_{c}"

    def chain(parent, length, depth):
        p = parent
        for i in range(length):
            if deep_pairs and rng.random() < 0.3:
                p = pair(p)  # a pair in the middle of the limb (or on the base): the limb goes on below its second link
                continue
            p = link(p)
            if depth < 1 and i == length // 2 and rng.random() < 0.5:  # a branching link: two sub-chains below it
                chain(p, int(rng.integers(1, 3)), depth + 1)
                chain(p, int(rng.integers(1, 3)), depth + 1)
                return
        if rng.random() < 0.5:
            pair(p)

    for _ in range(n_limbs):
        chain("base", int(rng.integers(1, 5)), 0)
    return m


def tello_with_arms_arms_first():
    """TelloWithArms with the two arms appended BEFORE the two legs (the package builder appends the legs first).  Cluster order
    decides the order of the limbs below the torso in the chain programs and how latency mode deals them to wavefronts: with the
    arms first, the last limb in program order is a leg whose hip differential and knee-ankle differential are kid chains, and
    each wavefront of a two-wavefront tile owns an arm and a leg.  The builder's calls are recorded and replayed in that order,
    so the model's parameters are the package's."""
    import generalized_rbda_amd.robots as R

    calls = []

    class Recorder:
        def __init__(self, *a, **k):
            calls.append(("__init__", a, k))

        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))

    real = R.ClusterTreeModel
    R.ClusterTreeModel = Recorder
    try:
        R.tello_with_arms()
    finally:
        R.ClusterTreeModel = real
    groups, cur = [], []
    for c in calls[1:]:
        cur.append(c)
        if c[0].startswith("append"):  # appendBody / appendRegisteredBodiesAsCluster / appendTrigPolyCluster close a cluster
            groups.append(cur)
            cur = []
    assert not cur
    is_arm = lambda g: any(s in g[-1][1][0] for s in ("shoulder", "elbow"))
    base, rest = groups[0], groups[1:]
    m = real(*calls[0][1], **calls[0][2])
    for g in [base] + [g for g in rest if is_arm(g)] + [g for g in rest if not is_arm(g)]:
        for name, a, k in g:
            getattr(m, name)(*a, **k)
    return m


# The generated family of tests/test_lds_schedule_cpu.py: chain_test_tree over these seeds, 2 - 6 limbs, deep pairs on and off
def lds_family():
    """name -> ClusterTreeModel"""
    fam = {}
    for n_limbs in range(2, 7):
        for deep in (False, True):
            for seed in range(12):
                fam[f"chain_tree_l{n_limbs}_{'deep' if deep else 'flat'}_s{seed}"] = chain_test_tree(
                    1000 + 100 * n_limbs + seed, n_limbs, deep_pairs=deep)
    return fam


ROBOT_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robot-models")


def valid_states(blob, B, config_index=0, max_cond=None, big=False, scale=1.0):
    """random_states + (for implicit-loop clusters) Newton projection of the dependent positions onto
    phi(q) = 0 with the oracle, rejecting states that do not converge (GenericJoint.cpp:289-385) or that fail the
    conditioning gate of generalized_rbda_amd/states.py (evaluated on the ORACLE's constraint Jacobian here).
    max_cond: a tighter bound on the condition number of K_d, for the tests that compare DERIVATIVES with differences taken along
    re-projected states: a state that satisfies phi to 1e-12 sits 1e-12 / sigma_min(K_d) off the manifold, and d G / d y changes by
    ~1 / sigma_min^3 per unit of that distance -- at cond 1400 the analytic derivative AT the state and the difference quotient ALONG
    the manifold differ by per cents although both are exact (measured on four_bar.urdf next to its flat pose).
    big: the oracle build with room for clusters of 48 bodies; scale: shrinks the drawn positions (long closed chains close only near
    their reference configuration)."""
    import oracle_py as O
    from generalized_rbda_amd.states import accept, parse_clusters, random_states

    if not any(c[9] >= 2 for c in parse_clusters(blob)["clusters"]):
        return random_states(blob, B, config_index)
    qs, qds, taus = [], [], []
    loop_clusters = [c for c in parse_clusters(blob)["clusters"] if c[9] == 2]
    have, attempt = 0, 0
    while have < B:
        q, qd, tau = random_states(blob, max(2 * B, 16), config_index + 7919 * attempt)
        q *= scale
        q, ok = O.project_positions(blob, q, big=big)
        for c in loop_clusters:  # revolute loops: Newton from a far guess may land whole turns away -- the same pose, wrapped
            q[:, c[3]:c[3] + c[4]] = np.remainder(q[:, c[3]:c[3] + c[4]] + np.pi, 2 * np.pi) - np.pi
        gmax, kcond = O.spanning_state(blob, q, qd, big=big)[2:]
        ok &= accept(blob, q, gmax, kcond)
        if max_cond is not None:
            ok &= kcond < max_cond
        qs.append(q[ok]); qds.append(qd[ok]); taus.append(tau[ok])
        have += int(ok.sum())
        attempt += 1
        if attempt > 50:
            raise RuntimeError("could not sample valid loop states")
    return np.concatenate(qs)[:B], np.concatenate(qds)[:B], np.concatenate(taus)[:B]


def zoo():
    """name -> model description bytes"""
    import generalized_rbda_amd as G

    z = {}
    for name in ("four_bar", "six_bar", "planar_leg_linkage", "mini_cheetah", "mit_humanoid", "jvrc1_humanoid",
                 "revolute_rotor_chain", "mit_humanoid_leg"):
        z["urdf_" + name] = G.urdf_to_blob(os.path.join(ROBOT_MODELS, name + ".urdf"))
    # ori_representation::RollPitchYaw floating bases (OrientationRepresentation.h:30-49, OrientationTools.h:121-130)
    z["urdf_mini_cheetah_rpy"] = G.urdf_to_blob(os.path.join(ROBOT_MODELS, "mini_cheetah.urdf"), ori_repr="rpy")
    z["tree_mixed_float_rpy"] = random_cluster_tree(8, 9, floating=True, ori_repr="rpy").serialize()
    from generalized_rbda_amd.robots import tello_with_arms

    z["tello_with_arms"] = tello_with_arms().serialize()
    # the other hand-built robots of the reference's unit tests (testClusterTreeModel.cpp:26-37)
    from generalized_rbda_amd.robots import mit_humanoid_no_rotors, teleop_arm, tello
    z["tello"] = tello().serialize()
    z["teleop_arm"] = teleop_arm().serialize()
    z["mit_humanoid_no_rotors"] = mit_humanoid_no_rotors().serialize()
    from generalized_rbda_amd.robots import jvrc1_humanoid

    z["jvrc1_hand_built"] = jvrc1_humanoid().serialize()  # the reference's JVRC1_Humanoid: 32 rotor clusters, 65 bodies
    for n in (2, 3, 4):
        z[f"rev_rotor_chain_{n}"] = md.revolute_chain_with_rotor(n).serialize()
    for n in (2, 4):
        z[f"rev_pair_rotor_chain_{n}"] = md.revolute_pair_chain_with_rotor(n).serialize()
    # the random serial chains of the reference's unit tests (testRigidBodyDynamicsAlgos.cpp:94-109)
    for n in (3, 6):
        z[f"rev_triple_rotor_chain_{n}"] = md.revolute_triple_chain_with_rotor(n, seed=n).serialize()
    for a, b in ((0, 8), (4, 4), (8, 0)):
        z[f"rev_chain_{a}_with_{b}_without_rotor"] = md.revolute_chain_with_and_without_rotor(a, b, seed=10 * a + b).serialize()
    z["rev_pair_chain_4"] = md.revolute_pair_chain(4, seed=4).serialize()
    z["tree_rev_fixed"] = random_cluster_tree(1, 6, floating=False, kinds=("rev",)).serialize()
    z["tree_rotor_float"] = random_cluster_tree(2, 8, floating=True, kinds=("rotor", "rev")).serialize()
    z["tree_pair_float"] = random_cluster_tree(3, 6, floating=True, kinds=("pair", "rotor")).serialize()
    z["tree_triple_fixed"] = random_cluster_tree(4, 4, floating=False, kinds=("triple", "rev")).serialize()
    z["tree_generic_float"] = random_cluster_tree(5, 7, floating=True, kinds=("generic",)).serialize()
    # models the chain-structured kernels cover (plan.h, ChainProgram): floating base, revolute links, links with
    # axisymmetric rotors, leaf pair clusters -- random topologies with long chains, branching links and mixed runs
    z["tree_chain_rotor_float"] = random_cluster_tree(11, 14, floating=True, kinds=("axirotor",)).serialize()
    z["tree_chain_rev_float"] = random_cluster_tree(14, 10, floating=True, kinds=("rev",)).serialize()
    z["chain_tree_a"] = chain_test_tree(21, 4).serialize()
    z["chain_tree_b"] = chain_test_tree(22, 5).serialize()
    z["chain_tree_rpy"] = chain_test_tree(23, 3, ori_repr="rpy").serialize()
    z["chain_tree_norotor"] = chain_test_tree(24, 4, rotors=False).serialize()
    z["tree_mixed_float"] = random_cluster_tree(6, 12, floating=True).serialize()
    z["tree_mixed_fixed"] = random_cluster_tree(7, 10, floating=False).serialize()
    return z
