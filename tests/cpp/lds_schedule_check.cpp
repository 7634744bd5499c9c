// Host-side checker of the LDS / slab schedules of the chain programs (plan.h, ChainProgram / RneaChainProgram).
//
// The plan compiler places every LDS object by its live range in program order; the latency-mode programs (n_waves = 2 / 4) run
// the limbs below the floating base on different wavefronts of one workgroup, ordered only by SEG_BARRIER / RSEG_BARRIER.  This
// driver compiles a model with the LDS budgets capi.cpp uses and checks the FINISHED programs against what the kernels of
// chain_kernels.hip touch -- not against the allocator's own objects and live ranges:
//   * access table: per segment op, the rows the kernel reads, writes or read-modify-writes, from the record fields it reaches
//     (sizes from the kernel's loads and stores: [sin, cos, v] 8, [v | a] 12, an accumulator [IA | psi] 27, [K | y0] 7, ...),
//     LDS rows and global-slab rows (kSlotGlobal) as two row spaces;
//   * races: segments of different owners between two barriers run concurrently; neither may write a row the other touches;
//   * def-use: the program run abstractly over rows in program order; every write labels its rows with (kind, whose quantity,
//     block); every read must find one whole block of the kind it expects, of the body it expects (from the cluster tree, not
//     from the program's slot fields), not overwritten since; a read-modify-write with acc_first == 0 must find the accumulator
//     already begun; the result rows of an LDS-resident output must still hold the results at the end;
//   * bounds: every row below n_lds / n_glb, and no slab slot where the kernel addresses LDS only.
// --self-test applies mutations to copies of the programs and requires each to be flagged.
// Usage: lds_schedule_check [--self-test] [--quiet] model.urdf | model.grbd ...   (exit status 0: no finding)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../generalized_rbda_amd/csrc/plan.h"
#include "../../include/grbda_hip.h"
#include "../../include/grbda_model_desc.h"

namespace grbda_hip {
int urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, std::vector<unsigned char> &blob, std::string &err);
}
using namespace grbda_hip;

namespace {

// ---- what a segment touches ------------------------------------------------------------------------------------------------
enum Kind { RD, WR, RMW, SCR };  // SCR: work space the segment writes and reads itself (a write for the race check)
// block kinds (what the rows hold)
enum Type { T_V6, T_SV, T_VA, T_ACC, T_KB, T_PAIRK, T_DGX, T_DK, T_Y0, T_OUT, T_RBLK, T_RDBLK, T_F, T_SCR, T_N };
const char *type_name[T_N] = {"[v]", "[sin,cos,v]", "[v|a]", "[IA|psi]", "[K|y0]", "pair [K|y0]", "diff [X|g|sc]", "diff [K|y0]",
                              "base [y0]", "result", "[f|sc|tau_r]", "diff [f2|sc|X]", "[f]", "work space"};
struct Accept { int type, off; };  // a read is satisfied by rows [off, off + n) of a block of this kind
struct Access {
    Kind kind;
    int type;                // block kind written (WR / SCR) or expected (RD / RMW: also accept[])
    std::vector<Accept> accept;
    int slot, n;
    int ident;               // whose quantity: v_index of its cluster (-1: none / ground); -2: do not check
    bool lds_only;           // the kernel addresses LDS whatever the slot number says
    bool slab_flag_required; // the kernel addresses the slab through glb_*, without LDS blocks (GRBDA_KLDS off)
    const char *field;
    int32_t *ptr;            // the record field the slot came from (self-test mutations), or null
    int ptr_add;             // slot = *ptr + ptr_add
};
struct Seg { int op; int owner; bool barrier; bool gen; std::vector<Access> acc; };
struct Prog {
    std::string name;
    bool rnea = false;
    int n_waves = 1, n_lds = 0, n_glb = 0, out_lds = -1, nv = 0;
    std::vector<Seg> segs;
};

const char *aba_op[] = {"FREE_FWD", "RUN_FWD", "RUN_BWD", "FREE_BWD", "FREE_ACC", "RUN_ACC", "PAIR_ACC", "DIFF_FWD", "DIFF_BWD",
                        "DIFF_ACC", "BARRIER", "GEN_FWD", "GEN_BWD", "GEN_ACC"};
const char *rnea_op[] = {"FREE_FWD", "RUN_FWD", "PAIR", "RUN_BWD", "FREE_BWD", "DIFF_FWD", "DIFF_BWD", "GEN_FWD", "GEN_BWD", "BARRIER"};
const char *op_name(const Prog &P, int op)
{
    if (P.rnea) return op >= 0 && op < 10 ? rnea_op[op] : "?";
    return op >= 0 && op < 14 ? aba_op[op] : "?";
}

// the cluster tree, from the plan's cluster records (independent of the chain programs' slot fields)
struct Tree {
    std::map<int, int> parent_of_v;  // v_index of a cluster -> v_index of the cluster its parent body belongs to (-1: ground)
    int parent(int v) const
    {
        auto it = parent_of_v.find(v);
        return it == parent_of_v.end() ? -3 : it->second;
    }
};
Tree make_tree(const HostPlan &hp)
{
    Tree t;
    const std::vector<ClusterRec> &cl = hp.lay32.clusters;
    for (const ClusterRec &c : cl) {
        int pv = -1;
        if (c.parent_body >= 0)
            for (const ClusterRec &p : cl)
                if (c.parent_body >= p.first_body && c.parent_body < p.first_body + p.k) pv = p.v_index;
        t.parent_of_v[c.v_index] = pv;
    }
    return t;
}

Access rd(int type, int32_t *ptr, int add, int n, int ident, bool lds_only, const char *field)
{
    return Access{RD, type, {{type, 0}}, ptr ? *ptr + add : -1, n, ident, lds_only, false, field, ptr, add};
}
Access wr(int type, int32_t *ptr, int add, int n, int ident, bool lds_only, const char *field)
{
    return Access{WR, type, {}, ptr ? *ptr + add : -1, n, ident, lds_only, false, field, ptr, add};
}
// a velocity: the v part of a [sin, cos, v] block (links, differentials) or the floating base's [v]
Access rd_v(int32_t *ptr, int ident, bool lds_only, const char *field)
{
    Access a = rd(T_V6, ptr, 0, 6, ident, lds_only, field);
    a.accept = {{T_SV, 2}, {T_V6, 0}};
    return a;
}
// a parent body's force: the first six rows of a link's / differential's block or one of the base's force blocks
Access rmw_f(int32_t *ptr, int ident, bool lds_only, const char *field)
{
    Access a = rd(T_F, ptr, 0, 6, ident, lds_only, field);
    a.kind = RMW;
    a.accept = {{T_F, 0}, {T_RBLK, 0}, {T_RDBLK, 0}};
    return a;
}

int diff_atoms(const HostPlan &hp, int tofs_i) { return tofs_i >= 0 ? hp.cints[tofs_i + 1] : 0; }

// ---- access table: forward dynamics (aba_chain_kernel / aba_chain_lm_kernel) ------------------------------------------------
// klds: the kernel is built with GRBDA_KLDS (glb_* of an unflagged slot addresses LDS); else glb_* slots must carry kSlotGlobal
Prog build_aba(ChainProgram &CP, const HostPlan &hp, const Tree &T, const std::string &name, bool klds)
{
    Prog P;
    P.name = name;
    P.n_waves = CP.n_waves;
    P.n_lds = CP.n_lds;
    P.n_glb = CP.n_glb;
    P.out_lds = CP.out_lds;
    P.nv = hp.nv;
    const bool svg = CP.sv_global;
    auto glb = [&](Access a) { a.slab_flag_required = !klds; return a; };
    auto out = [&](std::vector<Access> &v, int vi) {
        if (CP.out_lds < 0) return;  // (slab rows behind the inputs: outside both row spaces)
        Access a = wr(T_OUT, nullptr, 0, 1, vi, true, "out_lds");
        a.slot = CP.out_lds + vi;
        v.push_back(a);
    };
    for (ChainSeg &sg : CP.segs) {
        Seg s{sg.op, sg.owner, sg.op == SEG_BARRIER, sg.op >= SEG_GEN_FWD, {}};
        std::vector<Access> &A = s.acc;
        switch (sg.op) {
            case SEG_RUN_FWD: {
                ChainLink &l0 = CP.links[sg.first];
                if (l0.lds_pv != -1) A.push_back(rd_v(&l0.lds_pv, T.parent(l0.v_index), !svg, "ChainLink::lds_pv"));
                for (int i = 0; i < sg.count; i++) {
                    ChainLink &l = CP.links[sg.first + i];
                    A.push_back(wr(T_SV, &l.lds_sv, 0, 8, l.v_index, !svg, "ChainLink::lds_sv"));
                }
                break;
            }
            case SEG_RUN_BWD: {
                if (sg.head == HEAD_PAIR) {
                    ChainPair &pr = CP.pairs[sg.head_arg];
                    A.push_back(rd_v(&pr.lds_pv, T.parent(pr.v_index), false, "ChainPair::lds_pv"));
                    A.push_back(glb(wr(T_PAIRK, &pr.glb_k, 0, 14, pr.v_index, false, "ChainPair::glb_k")));
                } else if (sg.head == HEAD_SLOT) {
                    A.push_back(rd(T_ACC, &sg.head_arg, 0, 27, CP.links[sg.first].v_index, false, "ChainSeg::head_arg"));
                }
                for (int i = 0; i < sg.count; i++) {
                    ChainLink &l = CP.links[sg.first + i];
                    A.push_back(rd(T_SV, &l.lds_sv, 0, 8, l.v_index, !svg, "ChainLink::lds_sv"));
                    if (l.rofs >= 0) {
                        if (l.lds_pv != -1) A.push_back(rd_v(&l.lds_pv, T.parent(l.v_index), !svg, "ChainLink::lds_pv (rotor)"));
                        else if (T.parent(l.v_index) != -1) {  // the rotor would be evaluated on the ground
                            Access a = rd_v(&l.lds_pv, T.parent(l.v_index), !svg, "ChainLink::lds_pv (rotor)");
                            A.push_back(a);
                        }
                    }
                    A.push_back(glb(wr(T_KB, &l.glb_k, 0, 7, l.v_index, false, "ChainLink::glb_k")));
                }
                if (sg.lds_acc_out != -1) {
                    const int top = CP.links[sg.first + sg.count - 1].v_index;
                    if (sg.acc_first) A.push_back(wr(T_ACC, &sg.lds_acc_out, 0, 27, T.parent(top), false, "ChainSeg::lds_acc_out"));
                    else {
                        Access a = rd(T_ACC, &sg.lds_acc_out, 0, 27, T.parent(top), false, "ChainSeg::lds_acc_out");
                        a.kind = RMW;
                        A.push_back(a);
                    }
                }
                break;
            }
            case SEG_RUN_ACC: {
                const ChainLink &l0 = CP.links[sg.first];
                if (sg.lds_pva >= 0) A.push_back(rd(T_VA, &sg.lds_pva, 0, 12, T.parent(l0.v_index), true, "ChainSeg::lds_pva"));
                else if (T.parent(l0.v_index) != -1) A.push_back(rd(T_VA, &sg.lds_pva, 0, 12, T.parent(l0.v_index), true, "ChainSeg::lds_pva"));
                for (int i = 0; i < sg.count; i++) {
                    ChainLink &l = CP.links[sg.first + i];
                    A.push_back(glb(rd(T_KB, &l.glb_k, 0, 7, l.v_index, false, "ChainLink::glb_k")));
                    out(A, l.v_index);
                    if (l.has_child && l.lds_va >= 0) A.push_back(wr(T_VA, &l.lds_va, 0, 12, l.v_index, true, "ChainLink::lds_va"));
                }
                break;
            }
            case SEG_PAIR_ACC: {
                ChainPair &pr = CP.pairs[sg.first];
                A.push_back(glb(rd(T_PAIRK, &pr.glb_k, 0, 14, pr.v_index, false, "ChainPair::glb_k")));
                A.push_back(rd(T_VA, &pr.lds_pva, 0, 12, T.parent(pr.v_index), true, "ChainPair::lds_pva"));
                out(A, pr.v_index);
                out(A, pr.v_index + 1);
                break;
            }
            case SEG_FREE_FWD: {
                ChainFree &f = CP.frees[sg.first];
                if (f.lds_v >= 0) A.push_back(wr(T_V6, &f.lds_v, 0, 6, f.v_index, true, "ChainFree::lds_v"));
                break;
            }
            case SEG_FREE_BWD: {
                ChainFree &f = CP.frees[sg.first];
                if (f.lds_acc != -1) {
                    A.push_back(rd(T_ACC, &f.lds_acc, 0, 27, f.v_index, false, "ChainFree::lds_acc"));
                    if (f.lds_acc2 != -1) {
                        A.push_back(rd(T_ACC, &f.lds_acc2, 0, 27, f.v_index, false, "ChainFree::lds_acc2"));
                        if (f.lds_acc3 != -1) {
                            A.push_back(rd(T_ACC, &f.lds_acc3, 0, 27, f.v_index, false, "ChainFree::lds_acc3"));
                            if (f.lds_acc4 != -1) A.push_back(rd(T_ACC, &f.lds_acc4, 0, 27, f.v_index, false, "ChainFree::lds_acc4"));
                        }
                    }
                }
                A.push_back(glb(wr(T_Y0, &f.glb_y0, 0, 6, f.v_index, false, "ChainFree::glb_y0")));
                break;
            }
            case SEG_FREE_ACC: {
                ChainFree &f = CP.frees[sg.first];
                A.push_back(glb(rd(T_Y0, &f.glb_y0, 0, 6, f.v_index, false, "ChainFree::glb_y0")));
                for (int j = 0; j < 6; j++) out(A, f.v_index + j);
                if (f.lds_va >= 0) A.push_back(wr(T_VA, &f.lds_va, 0, 12, f.v_index, true, "ChainFree::lds_va"));
                break;
            }
            case SEG_DIFF_FWD: {
                ChainDiff &d = CP.diffs[sg.first];
                if (d.tofs_i >= 0) {
                    Access w = wr(T_SCR, &d.lds_w, 0, 3 * diff_atoms(hp, d.tofs_i), -1, true, "ChainDiff::lds_w");
                    w.kind = SCR;
                    A.push_back(w);
                }
                A.push_back(glb(wr(T_DGX, &d.glb_k, 14, 10, d.v_index, false, "ChainDiff::glb_k + 14")));
                if (d.lds_sv != -1) {
                    if (d.lds_pv != -1 || T.parent(d.v_index) != -1) A.push_back(rd_v(&d.lds_pv, T.parent(d.v_index), false, "ChainDiff::lds_pv"));
                    A.push_back(wr(T_SV, &d.lds_sv, 0, 8, d.v_index, false, "ChainDiff::lds_sv"));
                }
                break;
            }
            case SEG_DIFF_BWD: {
                ChainDiff &d = CP.diffs[sg.first];
                if (d.lds_pv != -1 || T.parent(d.v_index) != -1) A.push_back(rd_v(&d.lds_pv, T.parent(d.v_index), false, "ChainDiff::lds_pv"));
                A.push_back(glb(rd(T_DGX, &d.glb_k, 14, 10, d.v_index, false, "ChainDiff::glb_k + 14")));
                if (d.lds_acc != -1) A.push_back(rd(T_ACC, &d.lds_acc, 0, 27, d.v_index, false, "ChainDiff::lds_acc"));
                A.push_back(glb(wr(T_DK, &d.glb_k, 0, 14, d.v_index, false, "ChainDiff::glb_k")));
                if (d.lds_acc_out != -1) {
                    if (d.acc_first) A.push_back(wr(T_ACC, &d.lds_acc_out, 0, 27, T.parent(d.v_index), false, "ChainDiff::lds_acc_out"));
                    else {
                        Access a = rd(T_ACC, &d.lds_acc_out, 0, 27, T.parent(d.v_index), false, "ChainDiff::lds_acc_out");
                        a.kind = RMW;
                        A.push_back(a);
                    }
                }
                break;
            }
            case SEG_DIFF_ACC: {
                ChainDiff &d = CP.diffs[sg.first];
                A.push_back(glb(rd(T_DK, &d.glb_k, 0, 14, d.v_index, false, "ChainDiff::glb_k")));
                A.push_back(glb(rd(T_DGX, &d.glb_k, 14, 10, d.v_index, false, "ChainDiff::glb_k + 14")));
                if (d.lds_pva >= 0 || T.parent(d.v_index) != -1) A.push_back(rd(T_VA, &d.lds_pva, 0, 12, T.parent(d.v_index), true, "ChainDiff::lds_pva"));
                out(A, d.v_index);
                out(A, d.v_index + 1);
                if (d.lds_va >= 0) A.push_back(wr(T_VA, &d.lds_va, 0, 12, d.v_index, true, "ChainDiff::lds_va"));
                break;
            }
            default: break;  // barriers; generic clusters (not modelled: the program is skipped)
        }
        P.segs.push_back(s);
    }
    return P;
}

// ---- access table: inverse dynamics (rnea_chain_kernel / rnea_chain_lm_kernel) ----------------------------------------------
Prog build_rnea(RneaChainProgram &R, const HostPlan &hp, const Tree &T, const std::string &name)
{
    Prog P;
    P.name = name;
    P.rnea = true;
    P.n_waves = R.n_waves;
    P.n_lds = R.n_lds;
    P.n_glb = R.n_glb;
    P.nv = hp.nv;
    // GLB (the kernel's template flag): the link blocks and the force rows they receive may live in the slab; the latency-mode kernel
    // is built without it
    const bool lo = !(R.n_waves == 1 && R.n_glb > 0);
    for (RneaSeg &sg : R.segs) {
        Seg s{sg.op, sg.owner, sg.op == RSEG_BARRIER, sg.op == RSEG_GEN_FWD || sg.op == RSEG_GEN_BWD, {}};
        std::vector<Access> &A = s.acc;
        switch (sg.op) {
            case RSEG_RUN_FWD: {
                const RneaLink &l0 = R.links[sg.first];
                if (sg.lds_pva >= 0 || T.parent(l0.v_index) != -1) A.push_back(rd(T_VA, &sg.lds_pva, 0, 12, T.parent(l0.v_index), true, "RneaSeg::lds_pva"));
                for (int i = 0; i < sg.count; i++) {
                    RneaLink &l = R.links[sg.first + i];
                    if (l.rofs >= 0 && l.lds_pf >= 0) A.push_back(rmw_f(&l.lds_pf, T.parent(l.v_index), lo, "RneaLink::lds_pf (rotor)"));
                    A.push_back(wr(T_RBLK, &l.lds_blk, 0, 9, l.v_index, lo, "RneaLink::lds_blk"));
                    if (l.lds_va >= 0) A.push_back(wr(T_VA, &l.lds_va, 0, 12, l.v_index, true, "RneaLink::lds_va"));
                }
                break;
            }
            case RSEG_RUN_BWD: {
                for (int i = 0; i < sg.count; i++) {
                    RneaLink &l = R.links[sg.first + i];
                    A.push_back(rd(T_RBLK, &l.lds_blk, 0, 9, l.v_index, lo, "RneaLink::lds_blk"));
                }
                const int top = R.links[sg.first + sg.count - 1].v_index;
                if (sg.lds_pf >= 0 || T.parent(top) != -1) A.push_back(rmw_f(&sg.lds_pf, T.parent(top), lo, "RneaSeg::lds_pf"));
                break;
            }
            case RSEG_PAIR: {
                RneaPair &pr = R.pairs[sg.first];
                A.push_back(rd(T_VA, &pr.lds_pva, 0, 12, T.parent(pr.v_index), true, "RneaPair::lds_pva"));
                A.push_back(rmw_f(&pr.lds_pf, T.parent(pr.v_index), lo, "RneaPair::lds_pf"));
                break;
            }
            case RSEG_FREE_FWD: {
                RneaFree &f = R.frees[sg.first];
                A.push_back(wr(T_F, &f.lds_f, 0, 6, f.v_index, true, "RneaFree::lds_f"));
                if (f.lds_va >= 0) A.push_back(wr(T_VA, &f.lds_va, 0, 12, f.v_index, true, "RneaFree::lds_va"));
                if (R.n_waves > 1) {  // (rnea_chain_lm_kernel: the force blocks of the other wavefronts start at zero)
                    if (f.lds_f2 != -1) A.push_back(wr(T_F, &f.lds_f2, 0, 6, f.v_index, true, "RneaFree::lds_f2"));
                    if (f.lds_f3 != -1) A.push_back(wr(T_F, &f.lds_f3, 0, 6, f.v_index, true, "RneaFree::lds_f3"));
                    if (f.lds_f4 != -1) A.push_back(wr(T_F, &f.lds_f4, 0, 6, f.v_index, true, "RneaFree::lds_f4"));
                }
                break;
            }
            case RSEG_FREE_BWD: {
                RneaFree &f = R.frees[sg.first];
                if (R.n_waves > 1 && f.lds_f2 != -1) {
                    int32_t *const extra[3] = {&f.lds_f2, &f.lds_f3, &f.lds_f4};
                    const char *names[3] = {"RneaFree::lds_f2", "RneaFree::lds_f3", "RneaFree::lds_f4"};
                    for (int e = 0; e < 3 && *extra[e] != -1; e++) {
                        A.push_back(rd(T_F, extra[e], 0, 6, f.v_index, true, names[e]));
                        A.push_back(rmw_f(&f.lds_f, f.v_index, true, "RneaFree::lds_f"));
                    }
                }
                A.push_back(rd(T_F, &f.lds_f, 0, 6, f.v_index, true, "RneaFree::lds_f"));
                break;
            }
            case RSEG_DIFF_FWD: {
                RneaDiff &d = R.diffs[sg.first];
                if (d.tofs_i >= 0) {
                    Access w = wr(T_SCR, &d.lds_w, 0, 3 * diff_atoms(hp, d.tofs_i), -1, true, "RneaDiff::lds_w");
                    w.kind = SCR;
                    A.push_back(w);
                }
                if (d.lds_pva >= 0 || T.parent(d.v_index) != -1) A.push_back(rd(T_VA, &d.lds_pva, 0, 12, T.parent(d.v_index), true, "RneaDiff::lds_pva"));
                if (d.lds_pf >= 0 || T.parent(d.v_index) != -1) A.push_back(rmw_f(&d.lds_pf, T.parent(d.v_index), lo, "RneaDiff::lds_pf"));
                A.push_back(wr(T_RDBLK, &d.lds_blk, 0, 14, d.v_index, true, "RneaDiff::lds_blk"));
                if (d.lds_va >= 0) A.push_back(wr(T_VA, &d.lds_va, 0, 12, d.v_index, true, "RneaDiff::lds_va"));
                break;
            }
            case RSEG_DIFF_BWD: {
                RneaDiff &d = R.diffs[sg.first];
                A.push_back(rd(T_RDBLK, &d.lds_blk, 0, 14, d.v_index, true, "RneaDiff::lds_blk"));
                if (d.lds_pf >= 0 || T.parent(d.v_index) != -1) A.push_back(rmw_f(&d.lds_pf, T.parent(d.v_index), lo, "RneaDiff::lds_pf"));
                break;
            }
            default: break;
        }
        P.segs.push_back(s);
    }
    return P;
}

// ---- checks -----------------------------------------------------------------------------------------------------------------
struct Findings {
    int race = 0, defuse = 0, bounds = 0, structure = 0;
    std::vector<std::string> lines;
    int total() const { return race + defuse + bounds + structure; }
    void add(int &counter, const std::string &s)
    {
        counter++;
        if (lines.size() < 40) lines.push_back(s);
    }
};
bool is_glb(int slot) { return (slot & kSlotGlobal) != 0 && slot >= 0; }
int row_of(int slot) { return slot & ~kSlotGlobal; }
std::string where(const Prog &P, int si, const Access &a)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, "seg %d (owner %d, %s) %s %s %s rows %s[%d, %d)", si, P.segs[si].owner, op_name(P, P.segs[si].op),
                  a.kind == RD ? "reads" : (a.kind == RMW ? "read-modify-writes" : "writes"), a.field, type_name[a.type],
                  is_glb(a.slot) ? "slab " : "LDS ", row_of(a.slot), row_of(a.slot) + a.n);
    return buf;
}

void check_bounds(const Prog &P, Findings &F)
{
    for (size_t si = 0; si < P.segs.size(); si++)
        for (const Access &a : P.segs[si].acc) {
            if (a.n <= 0) continue;
            if (a.slot < 0) {
                F.add(F.structure, where(P, static_cast<int>(si), a) + ": no slot, but the body it belongs to is not the ground");
                continue;
            }
            if (is_glb(a.slot) && a.lds_only) {
                F.add(F.bounds, where(P, static_cast<int>(si), a) + ": a slab slot where the kernel addresses LDS");
                continue;
            }
            if (!is_glb(a.slot) && a.slab_flag_required) {
                F.add(F.bounds, where(P, static_cast<int>(si), a) + ": an LDS slot where the kernel addresses the slab");
                continue;
            }
            const int lim = is_glb(a.slot) ? P.n_glb : P.n_lds;
            if (row_of(a.slot) + a.n > lim) {
                char buf[64];
                std::snprintf(buf, sizeof buf, ": beyond %s %d", is_glb(a.slot) ? "n_glb" : "n_lds", lim);
                F.add(F.bounds, where(P, static_cast<int>(si), a) + buf);
            }
        }
}

void check_structure(const Prog &P, Findings &F)
{
    for (size_t si = 0; si < P.segs.size(); si++) {
        const Seg &s = P.segs[si];
        if (P.n_waves > 1 && s.gen) F.add(F.structure, "seg " + std::to_string(si) + ": a generic-cluster segment in a latency-mode program");
        if (!s.barrier && (s.owner < 0 || s.owner >= P.n_waves))
            F.add(F.structure, "seg " + std::to_string(si) + ": owner " + std::to_string(s.owner) + " outside the workgroup");
    }
}

// segments of different owners between two barriers run concurrently
void check_races(const Prog &P, Findings &F)
{
    if (P.n_waves < 2) return;
    size_t begin = 0;
    while (begin < P.segs.size()) {
        size_t end = begin;
        while (end < P.segs.size() && !P.segs[end].barrier) end++;
        for (size_t i = begin; i < end; i++)
            for (size_t j = i + 1; j < end; j++) {
                if (P.segs[i].owner == P.segs[j].owner) continue;
                int reported = 0;
                for (const Access &a : P.segs[i].acc)
                    for (const Access &b : P.segs[j].acc) {
                        if (a.slot < 0 || b.slot < 0 || is_glb(a.slot) != is_glb(b.slot)) continue;
                        if (a.kind == RD && b.kind == RD) continue;
                        const int a0 = row_of(a.slot), b0 = row_of(b.slot);
                        if (a0 >= b0 + b.n || b0 >= a0 + a.n) continue;
                        if (reported++ < 2)
                            F.add(F.race, "race: " + where(P, static_cast<int>(i), a) + "  <->  " + where(P, static_cast<int>(j), b));
                        else
                            F.race++;
                    }
            }
        begin = end + 1;
    }
}

struct Label { int wid = -1, type = -1, base = 0, ident = -1, seg = -1; const char *field = ""; };
struct Machine {
    std::vector<Label> lds, glb;
    int next = 0;
    std::vector<Label> &space(int slot) { return is_glb(slot) ? glb : lds; }
};

// abstract run in program order; hook(seg, access, machine) is called before every access
void run_defuse(const Prog &P, Findings &F, const std::function<void(int, const Access &, Machine &)> &hook = nullptr)
{
    Machine M;
    M.lds.assign(static_cast<size_t>(std::max(P.n_lds, 0)), Label());
    M.glb.assign(static_cast<size_t>(std::max(P.n_glb, 0)), Label());
    auto in_range = [&](const Access &a) {
        if (a.slot < 0 || a.n <= 0) return false;
        const std::vector<Label> &v = M.space(a.slot);
        return row_of(a.slot) + a.n <= static_cast<int>(v.size());
    };
    for (size_t si = 0; si < P.segs.size(); si++)
        for (const Access &a : P.segs[si].acc) {
            if (hook) hook(static_cast<int>(si), a, M);
            if (!in_range(a)) continue;  // (reported by the bounds check)
            std::vector<Label> &v = M.space(a.slot);
            const int r0 = row_of(a.slot);
            if (a.kind == RD || a.kind == RMW) {
                const Label &L = v[r0];
                bool ok = L.wid >= 0;
                int off = r0 - L.base;
                bool type_ok = false;
                for (const Accept &ac : a.accept) type_ok = type_ok || (ac.type == L.type && ac.off == off);
                ok = ok && type_ok;
                for (int i = 1; i < a.n && ok; i++) ok = v[r0 + i].wid == L.wid;
                if (ok && a.ident != -2 && L.ident != a.ident) ok = false;
                if (!ok) {
                    char buf[256];
                    if (L.wid < 0) std::snprintf(buf, sizeof buf, ": finds rows nobody wrote");
                    else
                        std::snprintf(buf, sizeof buf, ": finds %s of cluster v%d (seg %d, %s, block at row %d%s), expected cluster v%d",
                                      type_name[L.type], L.ident, L.seg, L.field, L.base, type_ok ? "" : ", wrong kind or offset", a.ident);
                    std::string msg = where(P, static_cast<int>(si), a) + buf;
                    for (int i = 1; i < a.n; i++)
                        if (v[r0 + i].wid != L.wid) {
                            const Label &o = v[r0 + i];
                            std::snprintf(buf, sizeof buf, "; row %d was overwritten by seg %d (%s, %s)", r0 + i, o.seg, o.field,
                                          o.type >= 0 ? type_name[o.type] : "-");
                            msg += buf;
                            break;
                        }
                    F.add(F.defuse, "def-use: " + msg);
                }
            } else {
                Label L;
                L.wid = M.next++;
                L.type = a.type;
                L.base = r0;
                L.ident = a.ident;
                L.seg = static_cast<int>(si);
                L.field = a.field;
                for (int i = 0; i < a.n; i++) v[r0 + i] = L;
            }
        }
    // the result rows must still hold the results when the epilogue reads them
    if (P.out_lds >= 0 && P.out_lds + P.nv <= static_cast<int>(M.lds.size()))
        for (int j = 0; j < P.nv; j++) {
            const Label &L = M.lds[P.out_lds + j];
            if (L.type != T_OUT || L.ident != j) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "def-use: result row %d (LDS row %d) holds %s of seg %d (%s) at the end", j, P.out_lds + j,
                              L.type >= 0 ? type_name[L.type] : "nothing", L.seg, L.field);
                F.add(F.defuse, buf);
            }
        }
    else if (P.out_lds >= 0)
        F.add(F.bounds, "result rows [" + std::to_string(P.out_lds) + ", +" + std::to_string(P.nv) + ") beyond n_lds " + std::to_string(P.n_lds));
}

Findings check(const Prog &P)
{
    Findings F;
    check_structure(P, F);
    check_bounds(P, F);
    check_races(P, F);
    run_defuse(P, F);
    return F;
}

// ---- the shape of the ADVICE race, read from a latency-mode program -----------------------------------------------------------
// one wavefront owns two or more direct limbs (limbs on the base); the last direct limb in program order has kid chains and runs on
// a different wavefront from an earlier limb.  Direct limbs: the forward-type segments of the phase that read the base's block.
bool advice_shape(const Prog &P)
{
    if (P.n_waves < 2) return false;
    // the base's block the limbs read: RNEA [v | a] written by FREE_FWD, ABA [v | a] written by FREE_ACC
    const int src_op = P.rnea ? static_cast<int>(RSEG_FREE_FWD) : static_cast<int>(SEG_FREE_ACC);
    int base_v = -1, src = -1;
    for (size_t si = 0; si < P.segs.size() && src < 0; si++)
        if (P.segs[si].op == src_op) {
            src = static_cast<int>(si);
            for (const Access &a : P.segs[si].acc)
                if (a.type == T_VA && a.kind == WR) base_v = a.ident;
        }
    if (src < 0 || base_v < 0) return false;
    const bool rnea = P.rnea;
    auto is_fwd = [&](int op) { return rnea ? (op == RSEG_RUN_FWD || op == RSEG_DIFF_FWD) : (op == SEG_RUN_ACC || op == SEG_DIFF_ACC); };
    std::vector<int> direct, other;
    for (size_t si = src + 1; si < P.segs.size(); si++) {
        if (P.segs[si].barrier) {
            if (rnea && !direct.empty()) break;  // (the RNEA's limbs end at the second barrier)
            continue;
        }
        if (!is_fwd(P.segs[si].op)) continue;
        bool on_base = false;
        for (const Access &a : P.segs[si].acc)
            if (a.type == T_VA && a.kind == RD && a.ident == base_v) on_base = true;
        (on_base ? direct : other).push_back(static_cast<int>(si));
    }
    if (direct.size() < 2) return false;
    std::map<int, int> per_wave;
    for (int si : direct) per_wave[P.segs[si].owner]++;
    bool two = false;
    for (auto &kv : per_wave) two = two || kv.second >= 2;
    const int last = direct.back();
    bool kids = false;
    for (int si : other) kids = kids || si > last;
    bool other_wave_earlier = false;
    for (int si : direct)
        if (si != last && P.segs[si].owner != P.segs[last].owner) other_wave_earlier = true;
    return two && kids && other_wave_earlier;
}

// ---- self-test: mutations that the checks must flag ---------------------------------------------------------------------------
template <class CPT> constexpr bool P_is_rnea() { return std::is_same<CPT, RneaChainProgram>::value; }
struct SelfTest { bool moved = false, barrier = false, shifted = false, stale = false; };

// (the programs are rebuilt from a copy of the plan program for every mutation; the mutation goes through the record fields)
template <class CPT, class Build>
void self_test(const CPT &orig, Build build, SelfTest &st, const std::string &name)
{
    // 1. move one wavefront's object onto rows another wavefront uses in the same interval
    if (!st.moved && orig.n_waves > 1) {
        CPT cp = orig;
        Prog P = build(cp);
        bool done = false;
        size_t begin = 0;
        while (begin < P.segs.size() && !done) {
            size_t end = begin;
            while (end < P.segs.size() && !P.segs[end].barrier) end++;
            for (size_t i = begin; i < end && !done; i++)
                for (size_t j = begin; j < end && !done; j++) {
                    if (P.segs[i].owner == P.segs[j].owner) continue;
                    for (const Access &a : P.segs[i].acc) {
                        if (done || a.kind != WR || !a.ptr || a.slot < 0 || is_glb(a.slot)) continue;
                        for (const Access &b : P.segs[j].acc)
                            if (!done && b.slot >= 0 && !is_glb(b.slot) && b.n >= a.n) {
                                *a.ptr = b.slot - a.ptr_add;
                                done = true;
                            }
                    }
                }
            begin = end + 1;
        }
        if (done) {
            Findings F = check(build(cp));
            if (F.race > 0) {
                st.moved = true;
                std::printf("self-test %s: object moved onto another wavefront's rows: flagged (%d races)\n", name.c_str(), F.race);
            }
        }
    }
    // 2. delete a barrier
    if (!st.barrier && orig.n_waves > 1) {
        CPT cp = orig;
        Prog P = build(cp);
        for (size_t si = 0; si < P.segs.size(); si++)
            if (P.segs[si].barrier) {
                cp.segs.erase(cp.segs.begin() + static_cast<long>(si));
                break;
            }
        Findings F = check(build(cp));
        if (F.race > 0) {
            st.barrier = true;
            std::printf("self-test %s: barrier deleted: flagged (%d races)\n", name.c_str(), F.race);
        }
    }
    // 3. shift an lds_pva by one row
    if (!st.shifted) {
        CPT cp = orig;
        bool done = false;
        for (auto &sg : cp.segs)
            if (!done && sg.op == (P_is_rnea<CPT>() ? (int)RSEG_RUN_FWD : (int)SEG_RUN_ACC) && sg.lds_pva >= 0) {
                sg.lds_pva += 1;
                done = true;
            }
        if (done) {
            Findings F = check(build(cp));
            if (F.defuse > 0) {
                st.shifted = true;
                std::printf("self-test %s: lds_pva shifted by one row: flagged (%d def-use)\n", name.c_str(), F.defuse);
            }
        }
    }
    // 4. point a consumer at a block of the same kind that something else has overwritten since it was written
    if (!st.stale) {
        CPT cp = orig;
        Prog P = build(cp);
        struct W { int type, base, n, wid; bool glb; };
        std::vector<W> log;
        int32_t *target = nullptr;
        int value = 0;
        Findings dummy;
        run_defuse(P, dummy, [&](int, const Access &a, Machine &M) {
            if (target) return;
            if (a.kind == RD && a.ptr && a.ptr_add == 0 && a.slot >= 0 && a.accept.size() == 1 && a.accept[0].off == 0) {
                for (const W &w : log) {
                    if (w.type != a.type || w.n != a.n || w.glb != is_glb(a.slot)) continue;
                    std::vector<Label> &v = w.glb ? M.glb : M.lds;
                    if (w.base + w.n > static_cast<int>(v.size())) continue;
                    bool overwritten = false;
                    for (int i = 0; i < w.n; i++) overwritten = overwritten || v[w.base + i].wid != w.wid;
                    if (overwritten) {
                        target = a.ptr;
                        value = w.glb ? (w.base | kSlotGlobal) : w.base;
                        break;
                    }
                }
            }
            if ((a.kind == WR) && a.slot >= 0) log.push_back({a.type, row_of(a.slot), a.n, M.next, is_glb(a.slot)});
        });
        if (target) {
            *target = value;
            Findings F = check(build(cp));
            if (F.defuse > 0) {
                st.stale = true;
                std::printf("self-test %s: consumer pointed at an overwritten block: flagged (%d def-use)\n", name.c_str(), F.defuse);
            }
        }
    }
}
}  // namespace

int main(int argc, char **argv)
{
    bool self = false, quiet = false;
    std::vector<std::string> files;
    for (int a = 1; a < argc; a++) {
        if (!std::strcmp(argv[a], "--self-test")) self = true;
        else if (!std::strcmp(argv[a], "--quiet")) quiet = true;
        else files.push_back(argv[a]);
    }
    int n_checked = 0, n_skipped = 0, n_absent = 0, n_find = 0;
    SelfTest st;
    for (const std::string &file : files) {
        std::vector<unsigned char> blob;
        if (file.size() > 5 && file.substr(file.size() - 5) == ".urdf") {
            std::string err;
            const char *paths[1] = {file.c_str()};
            if (urdf_to_blob(paths, 1, 0, blob, err)) {
                std::printf("%s: reader error %s\n", file.c_str(), err.c_str());
                n_find++;
                continue;
            }
        } else {
            FILE *f = std::fopen(file.c_str(), "rb");
            if (!f) { std::printf("%s: cannot open\n", file.c_str()); n_find++; continue; }
            unsigned char buf[4096];
            size_t n;
            while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
            std::fclose(f);
        }
        // the library's default budgets (PlanOptions); the latency-mode programs carry their own (plan.cpp)
        HostPlan hp;
        char msg[512] = {0};
        if (int rc = compile_plan(blob.data(), blob.size(), PlanOptions{}, hp, msg, sizeof msg)) {
            std::printf("%s: plan error %d %s\n", file.c_str(), rc, msg);
            n_find++;
            continue;
        }
        const Tree T = make_tree(hp);
        std::string model = file.substr(file.find_last_of('/') + 1);
        // (the programs whose [K | y0] blocks are LDS objects: plan.cpp builds them with k_lds)
        const auto klds_of = [](int s) { return s == SLOT_LM2_F32 || s == SLOT_LM4_F32 || s == SLOT_LM4_F64; };
        auto report = [&](const char *prog, bool ok, const Prog *P) {
            if (!ok) {
                n_absent++;
                if (!quiet) std::printf("%s %s: not built\n", model.c_str(), prog);
                return;
            }
            bool gen = false;
            for (const Seg &s : P->segs) gen = gen || s.gen;
            if (gen && P->n_waves == 1) {
                n_skipped++;
                if (!quiet) std::printf("%s %s: skipped (generic-cluster segments)\n", model.c_str(), prog);
                return;
            }
            n_checked++;
            Findings F = check(*P);
            const bool shape = advice_shape(*P);
            std::printf("%s %s: checked, %zu segments, %d waves, n_lds %d, n_glb %d, shape %d, findings %d\n", model.c_str(), prog,
                        P->segs.size(), P->n_waves, P->n_lds, P->n_glb, shape ? 1 : 0, F.total());
            for (const std::string &l : F.lines) std::printf("    %s\n", l.c_str());
            if (F.total() > static_cast<int>(F.lines.size())) std::printf("    ... %zu more\n", F.total() - F.lines.size());
            n_find += F.total();
        };
        for (int s = 0; s < kChainSlots; s++) {
            const char *name = kChainSlotName[s];
            const ChainProgram &cp = hp.chain[s];
            if (!cp.ok) { report(name, false, nullptr); continue; }
            ChainProgram copy = cp;
            const bool klds = klds_of(s);
            Prog P = build_aba(copy, hp, T, name, klds);
            report(name, true, &P);
            if (self && cp.n_waves > 1) {
                const std::string nm = model + " " + name;
                self_test(cp, [&](ChainProgram &c) { return build_aba(c, hp, T, nm, klds); }, st, nm);
            }
        }
        for (int s = 0; s < kChainSlots; s++) {
            const std::string name = std::string("r") + kChainSlotName[s];
            const RneaChainProgram &rp = hp.rchain[s];
            if (!rp.ok) { report(name.c_str(), false, nullptr); continue; }
            RneaChainProgram copy = rp;
            Prog P = build_rnea(copy, hp, T, name);
            report(name.c_str(), true, &P);
            if (self && rp.n_waves > 1) {
                const std::string nm = model + " " + name;
                self_test(rp, [&](RneaChainProgram &c) { return build_rnea(c, hp, T, nm); }, st, nm);
            }
        }
    }
    std::printf("programs checked %d, skipped %d, not built %d; findings %d\n", n_checked, n_skipped, n_absent, n_find);
    int rc = n_find ? 1 : 0;
    if (self) {
        const int flagged = st.moved + st.barrier + st.shifted + st.stale;
        std::printf("self-test: %d of 4 mutations flagged (moved %d, barrier %d, shifted %d, stale %d)\n", flagged, st.moved, st.barrier,
                    st.shifted, st.stale);
        if (flagged != 4) rc = 1;
    }
    return rc;
}
