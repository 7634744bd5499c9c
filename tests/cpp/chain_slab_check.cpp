// chain_slab_check -- the slab rule of the chain forward dynamics (devplan.h, chain_slab_rows) over the chain programs of real plans, on the
// host: `make slab-check && build/slab_check/chain_slab_check tests/golden/robot-models/*.urdf` (tests/test_chain_slab_rule_cpu.py; built with
// AddressSanitizer and UBSan, host code only, no device needed).
//
// The kernel takes its slab pointers from the rule and run_chain (capi.cpp) sizes the allocation by the rule's `total`, so what can still go
// wrong is the rule itself: a region outside `total`, the global slots and the result rows overlapping, or a launch with its inputs in
// registers paying for input rows.  For every program of every plan, in both layouts:
//   * the global slots [glb, glb + n_glb) and -- when the plan keeps no result rows in LDS -- the result rows [out, out + nv) lie in
//     [0, total) and do not overlap;
//   * inputs in registers: total = n_glb (+ nv without LDS result rows), nothing else;
//   * staged inputs: total = nq + 2 nv + n_glb, the input rows [0, nq + 2 nv) in front of the global slots and the result rows on tau's;
//   * the bytes a grid of wavefronts is given (rows x 64 scalars each) cover the last wavefront's last row.
// It also prints, per model, which layout the fp32 program gets (chain_inputs_in_registers) and the rows saved.
#include <cstdio>
#include <string>
#include <vector>

#include "../../generalized_rbda_amd/csrc/devplan.h"
#include "../../include/grbda_hip.h"
#include "../../include/grbda_model_desc.h"

namespace grbda_hip {
int urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, std::vector<unsigned char> &blob, std::string &err);
}
using namespace grbda_hip;

static int n_bad = 0;
static void expect(bool ok, const std::string &where, const char *what)
{
    if (ok) return;
    n_bad++;
    std::printf("%s: %s\n", where.c_str(), what);
}

static void check_rule(const std::string &where, bool inreg, int nq, int nv, int n_glb, int out_lds)
{
    const ChainSlabRows r = chain_slab_rows(inreg, nq, nv, n_glb, out_lds);
    const bool out_rows = out_lds < 0;
    expect(r.glb >= 0 && r.glb + n_glb <= r.total, where, "global slots outside the slab");
    if (out_rows) {
        expect(r.out >= 0 && r.out + nv <= r.total, where, "result rows outside the slab");
        expect(r.out + nv <= r.glb || r.glb + n_glb <= r.out, where, "result rows overlap the global slots");
    }
    if (inreg) {
        expect(r.total == n_glb + (out_rows ? nv : 0), where, "a slab without input rows holds the global slots and the result rows only");
    } else {
        expect(r.total == nq + 2 * nv + n_glb, where, "staged layout: nq + 2 nv input rows and the global slots");
        expect(r.glb == nq + 2 * nv && r.out == nq + nv, where, "staged layout: inputs first, results on tau's rows");
    }
    // the allocation of a grid: every wavefront's rows, touched through a real buffer so that the sanitizer sees an index past it
    const size_t grid = 3;
    std::vector<float> slab(grid * static_cast<size_t>(r.total) * kWave, 0.f);
    for (size_t w = 0; w < grid; w++) {
        float *mine = slab.data() + w * static_cast<size_t>(r.total) * kWave;
        for (int s = 0; s < n_glb; s++) mine[static_cast<size_t>(r.glb + s) * kWave + (kWave - 1)] += 1.f;
        if (out_rows)
            for (int j = 0; j < nv; j++) mine[static_cast<size_t>(r.out + j) * kWave + (kWave - 1)] += 1.f;
    }
    float most = 0.f;
    for (const float v : slab) most = v > most ? v : most;
    expect(most <= 1.f, where, "two rows of a wavefront, or of neighbouring wavefronts, share an address");
}

int main(int argc, char **argv)
{
    int n_models = 0;
    for (int a = 1; a < argc; a++) {
        const std::string file = argv[a];
        std::vector<unsigned char> blob;
        std::string err;
        const char *paths[1] = {file.c_str()};
        if (urdf_to_blob(paths, 1, 0, blob, err)) {
            std::printf("%s: reader error %s\n", file.c_str(), err.c_str());
            n_bad++;
            continue;
        }
        HostPlan hp;
        char msg[512] = {0};
        if (const int rc = compile_plan(blob.data(), blob.size(), PlanOptions{}, hp, msg, sizeof msg)) {
            std::printf("%s: plan error %d %s\n", file.c_str(), rc, msg);
            n_bad++;
            continue;
        }
        n_models++;
        const std::string model = file.substr(file.find_last_of('/') + 1);
        for (const ChainSlot slot : {SLOT_F32, SLOT_F64}) {
            const ChainProgram &cp = hp.chain[slot];
            if (!cp.ok) continue;
            const size_t elem = slot == SLOT_F32 ? 4 : 8;
            const bool inreg = chain_inputs_in_registers(elem, static_cast<int>(cp.gens.size()), static_cast<int>(cp.diffs.size()), cp.sv_global ? 1 : 0, hp.nq, hp.nv);
            const std::string where = model + (elem == 4 ? " fp32" : " fp64");
            for (const bool layout : {false, true})
                for (const int out_lds : {cp.out_lds, -1, 0})
                    check_rule(where + (layout ? " registers" : " staged"), layout, hp.nq, hp.nv, cp.n_glb, out_lds);
            const int staged = chain_slab_rows(false, hp.nq, hp.nv, cp.n_glb, cp.out_lds).total, now = chain_slab_rows(inreg, hp.nq, hp.nv, cp.n_glb, cp.out_lds).total;
            expect(inreg || now == staged, where, "a launch with staged inputs keeps its rows");
            expect(!inreg || now == staged - (hp.nq + 2 * hp.nv) + (cp.out_lds < 0 ? hp.nv : 0), where, "inputs in registers: the input rows are gone");
            std::printf("%s: nq %d nv %d n_glb %d out_lds %d -> %s, %d rows per wavefront (staged layout: %d)\n", where.c_str(), hp.nq, hp.nv, cp.n_glb, cp.out_lds,
                        inreg ? "inputs in registers" : "staged inputs", now, staged);
        }
    }
    std::printf("%d models, %d findings\n", n_models, n_bad);
    return n_bad == 0 && n_models > 0 ? 0 : 1;
}
