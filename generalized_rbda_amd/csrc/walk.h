// walk.h -- the ancestor walk of a listed few bodies: the step records the walk kernels read (body_list_kernels.hip,
// frame_jacobian_kernels.hip, frame_product_kernels.hip, through walk_dev.h) and the host builders of walk.cpp.  Plain C++: built with g++ like plan.cpp, so that the
// sanitizer driver (tools/asan_driver.cpp) reaches the builders; devplan.h includes this header for the kernels and capi.cpp.
//
// A WALK is the union of the listed bodies' ancestors, each body once, depth first from the roots.  capi.cpp builds it per call from the
// caller's host list and it travels by value in the kernel arguments, like WrenchList and ContactSet.  A step computes its body from the
// running value of the root path, which the kernels hold in registers: the step before it is its tree parent, unless `restore` names the
// saved value of a branch point to start from.  `save` names the slot that keeps the body's value for its later children (a body with two
// or more children in the walk); a slot is free again once the last child has read it.  Saved values live in LDS, [slot][value 12][lane].
#pragma once
#include <cstdint>
#include <vector>

#include "plan.h"

namespace grbda_hip {

constexpr int kMaxBodyList = 16;
// steps of a walk: the MIT humanoid's two feet take 11, the sixteen last bodies of the humanoid, Tello and the Mini Cheetah 17 to 18.  The cap
// is kept where a list can pass it on a model of the test set (all sixteen of the 20 bodies of parallel_chain_exp_d10_l16 walk 20), so that
// the fallback is a route that runs; a step is 20 bytes of kernel arguments, and nothing but this constant stands against a longer walk
constexpr int kMaxWalk = 19;
constexpr int kMaxSaved = 4;   // values saved at once: 4 x 12 x 64 lanes x 8 bytes = 24 KiB of LDS in fp64
constexpr int kWalkNone = 0xFF;
// Poses and twists of a listed few bodies (include/grbda_hip_bodies.h): the children of a body in index order.  The n_out output slots a
// step stores are the next n_out entries of BodyWalk::slot.
struct BodyWalkStep {
    int32_t cofs;      // BodyRec::cofs
    int16_t body;      // plan body index
    int16_t q_col;     // first position column the joint angle reads (an implicit cluster: the body's own spanning position)
    int16_t span_col;  // the body's first spanning rate
    uint8_t free;      // 1: the floating base (its own pose and twist, no parent)
    uint8_t n;         // explicit clusters: the angle is the body's G row times the cluster's n positions; 0: q[q_col] itself
    uint8_t axis;      // BodyRec::axis
    uint8_t canon;     // BodyRec::canon_axis
    uint8_t root;      // 1: no tree parent
    uint8_t save;      // slot to keep the body's value in, or kWalkNone
    uint8_t restore;   // slot to start from, or kWalkNone: the running value
    uint8_t n_out;     // output slots stored after the step
};
// the walk's fallback: out[nb][n][12] = full[nb][n_bodies][12] at the listed bodies
struct BodyList {
    int n;
    int body[kMaxBodyList];
};

// Frame Jacobians (include/grbda_hip_jacobians.h), route 0: the steps of a body walk -- a body's in-cluster child first among its children,
// so that the cluster's axes go on accumulating in registers from the one step to the next -- with, per step, the frames at or below the
// body (`below`), the frames that ARE the body (`own`: the first pass leaves their [E | point] in LDS slot n_saved + i) and the frames whose
// columns of the body's cluster are complete at this step (`emit`: the body is the deepest one of its cluster on their root paths).  cont:
// the step before is the body's in-cluster parent and the cluster's world-frame axes A[n][6] go on accumulating; otherwise they start from
// zero.  Only the floating base and explicit clusters of 1..kJacMaxDof coordinates walk; G rows at kBodyConstFixed.
constexpr int kJacMaskWords = 2;  // per frame the bit mask of the velocity columns on its root path (all ones when nv > 128)
constexpr int kJacMaxDof = 4;
constexpr int kJacMaxSlots = 10;  // saved values + frames: 10 x 12 x 64 lanes x 8 bytes = 60 KiB of LDS in fp64, what a launch gets unasked
struct JacWalkStep {
    int32_t cofs;
    int16_t q_col, v_col;
    uint16_t below, own, emit;
    uint8_t free, n, axis, root, save, restore, cont, pad[3];
};

// The precision-independent part of a walk, built on the host per call (n and every index checked by the caller).  walk_len and max_saved
// are counted in full even when they pass the caps (or an index does not fit a step's fields): `route` is then 1 and the steps are not
// used.  Body list, route 1: the full kernel and a gather.
struct BodyWalkHost {
    int walk_len = 0, max_saved = 0, route = 0, n = 0;
    uint8_t slot[kMaxBodyList] = {};
    BodyWalkStep step[kMaxWalk] = {};
    BodyList list{};
};
BodyWalkHost build_body_walk(const HostPlan &h, const Layout &L, int n, const int *bodies);
// Frame Jacobians: `route` is 1 -- the expanded batch through the listed twists -- when a root path holds anything but the floating base
// and explicit clusters of 1..kJacMaxDof coordinates, on the spanning-tree route, when a body of the walk has two in-cluster children, and
// past the caps: kMaxWalk steps, kJacMaxSlots frames and saved values together, 128 velocities.  cols: per frame, the velocity columns on
// its root path (on either route).
struct JacWalkHost {
    int walk_len = 0, max_saved = 0, route = 0, n = 0;
    JacWalkStep step[kMaxWalk] = {};
    uint64_t cols[kMaxBodyList][kJacMaskWords] = {};
    uint8_t canon[kMaxBodyList] = {};
};
JacWalkHost build_jac_walk(const HostPlan &h, const Layout &L, int n, const int *bodies);

}  // namespace grbda_hip
