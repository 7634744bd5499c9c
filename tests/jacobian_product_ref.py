"""Test infrastructure: the products J v and J^T f at a listed few body frames in numpy -- the reference the device entry points of
include/grbda_hip_jacobian_products.h are held to.  A helper module, not a test file; nothing here calls the library under test.  Both are
numpy.einsum over frame_jacobian_ref.jacobians (or over a J assembled by frame_jacobian_ref.assemble); tests/
test_jacobian_product_ref_cpu.py pins them to the listed twists and to the oracle's inverse dynamics, independently of that einsum.

    jv   [B, n, 6]   J_i v, [angular 3; linear 3]: the velocity of frame i for the joint velocity v
    jtf  [B, nv]     sum over i of J_i^T f_i, f_i = [moment 3; force 3] in the frame of J_i -- at the point offsets[i], in the body's axes
                     (frame="body") or in world axes (frame="world"): the joint torques that BALANCE the wrenches, so that inverse dynamics
                     with the wrenches applied needs jtf less"""
import numpy as np

import frame_jacobian_ref as FJ


def jv_of(J, v):
    return np.einsum("bcik,bk->bci", J, np.asarray(v, dtype=np.float64))


def jtf_of(J, f):
    return np.einsum("bcik,bci->bk", J, np.asarray(f, dtype=np.float64))


def jv(blob, q, v, bodies, offsets=None, frame="body", big=False):
    return jv_of(FJ.jacobians(blob, q, bodies, offsets, frame, big=big), v)


def jtf(blob, q, f, bodies, offsets=None, frame="body", big=False):
    return jtf_of(FJ.jacobians(blob, q, bodies, offsets, frame, big=big), f)
