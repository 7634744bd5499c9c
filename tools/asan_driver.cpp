// AddressSanitizer / UBSan driver of the host-side code (make asan): the URDF+ reader (csrc/urdf.cpp), the plan compiler
// (csrc/plan.cpp) at the launch shapes capi.cpp uses, the builders of the ancestor walks (csrc/walk.cpp) on lists of every shape, and the
// oracle (oracle/grbda_oracle.c) on a few states -- for every URDF given on the command line, both base orientations.  Also a truncated
// and a corrupted blob: the plan compiler and the oracle must reject them without reading out of bounds.  Exit code 0 = no finding (the
// sanitizers abort otherwise).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../generalized_rbda_amd/csrc/plan.h"
#include "../generalized_rbda_amd/csrc/walk.h"
#include "../include/grbda_hip.h"
#include "../include/grbda_model_desc.h"
extern "C" {
#include "../oracle/grbda_oracle.h"
}

namespace grbda_hip {
int urdf_to_blob(const char *const *paths, int n_paths, int ori_repr, std::vector<unsigned char> &blob, std::string &err);
}

static int compile(const std::vector<unsigned char> &blob, grbda_hip::HostPlan &hp, char *msg, size_t cap)
{
    return grbda_hip::compile_plan(blob.data(), blob.size(), grbda_hip::PlanOptions{}, hp, msg, cap);  // the library's defaults
}

// ---- the ancestor walks (csrc/walk.cpp) ------------------------------------------------------------------------------------------
// Both builders on one list, checked against a plain recursive walk of the driver's own: the order of the bodies, where a value is saved,
// where one is restored and how many are live at once.  The step records are looked at only on route 0, where the kernels read them.
namespace walkcheck {
using namespace grbda_hip;

struct Tree {
    const Layout &L;
    std::vector<int> cluster_of;
    explicit Tree(const Layout &lay) : L(lay), cluster_of(lay.bodies.size(), -1)
    {
        for (size_t ci = 0; ci < L.clusters.size(); ci++)
            for (int i = 0; i < L.clusters[ci].k; i++) cluster_of[L.clusters[ci].first_body + i] = static_cast<int>(ci);
    }
    int parent(int b) const { return L.clusters[cluster_of[b]].kind == CK_FREE ? -1 : L.bodies[b].parent; }
    bool in_cluster(int b, int par) const { return L.bodies[b].lam == par && cluster_of[b] == cluster_of[par]; }
};
// the walk a list asks for: per body of the ancestor union its children (cluster_first: the in-cluster child in front), the bodies in
// depth-first order, and the peak number of values held for later children
struct Expect {
    std::vector<std::vector<int>> kids;
    std::vector<int> roots, order;
    int peak = 0;
    void visit(int b, int live)
    {
        order.push_back(b);
        const size_t nk = kids[b].size();
        if (nk >= 2) live++;  // the body's own value, until its last child has read it
        peak = std::max(peak, live);
        for (size_t k = 0; k < nk; k++) visit(kids[b][k], nk >= 2 && k + 1 == nk ? live - 1 : live);
    }
    Expect(const Tree &t, int n, const int *bodies, bool cluster_first) : kids(t.L.bodies.size())
    {
        std::vector<char> in(t.L.bodies.size(), 0);
        for (int i = 0; i < n; i++)
            for (int b = bodies[i]; b >= 0 && !in[b]; b = t.parent(b)) in[b] = 1;
        for (int b = 0; b < static_cast<int>(in.size()); b++) {
            if (!in[b]) continue;
            const int par = t.parent(b);
            if (par < 0) roots.push_back(b);
            else if (cluster_first && t.in_cluster(b, par)) kids[par].insert(kids[par].begin(), b);
            else kids[par].push_back(b);
        }
        for (int r : roots) visit(r, 0);
    }
};
// the save and restore fields of a walk's steps against the expected walk: a restore names the slot its parent saved, while children of
// that parent are still to come; a save takes a slot that holds nothing
template <class Step>
int check_slots(const Tree &t, const Expect &e, const Step *step, int cap)
{
    int bad = 0;
    std::vector<int> slot_of(t.L.bodies.size(), -1), owner(static_cast<size_t>(cap), -1), to_come(t.L.bodies.size(), 0);
    for (size_t s = 0; s < e.order.size(); s++) {
        const int b = e.order[s], par = t.parent(b);
        const bool later_child = par >= 0 && e.kids[par][0] != b;
        if (later_child) {
            const int sl = step[s].restore;
            if (sl >= cap || sl != slot_of[par] || owner[sl] != par || to_come[par] <= 0) { bad++; continue; }
            if (--to_come[par] == 0) owner[sl] = -1;
        } else if (step[s].restore != kWalkNone) bad++;
        if (e.kids[b].size() >= 2) {
            const int sl = step[s].save;
            if (sl >= cap || owner[sl] != -1) { bad++; continue; }
            owner[sl] = b;
            slot_of[b] = sl;
            to_come[b] = static_cast<int>(e.kids[b].size()) - 1;
        } else if (step[s].save != kWalkNone) bad++;
    }
    for (int o : owner) bad += o != -1;  // every saved value was read by the last child
    return bad;
}
int check_list(const HostPlan &hp, const Layout &L, int n, const int *bodies)
{
    int bad = 0;
    const Tree t(L);
    {
        const BodyWalkHost W = build_body_walk(hp, L, n, bodies);
        const Expect e(t, n, bodies, false);
        bad += W.walk_len != static_cast<int>(e.order.size()) || W.max_saved != e.peak || W.n != n;
        if (W.route == 0) {
            bad += W.walk_len > kMaxWalk || W.max_saved > kMaxSaved;
            if (!bad) bad += check_slots(t, e, W.step, kMaxSaved);
            int outs = 0;  // the n_out sum to n, and `slot` lists every output once, at its body's step
            unsigned seen = 0;
            for (int s = 0; s < W.walk_len && !bad; s++) {
                bad += W.step[s].body != e.order[s];
                for (int k = 0; k < W.step[s].n_out; k++, outs++) {
                    if (outs >= n) { bad++; break; }
                    const int i = W.slot[outs];
                    if (i >= n || ((seen >> i) & 1) || bodies[i] != W.step[s].body) bad++;
                    else seen |= 1u << i;
                }
            }
            bad += outs != n || seen != (n ? ~0u >> (32 - n) : 0u);
        }
    }
    {
        const JacWalkHost W = build_jac_walk(hp, L, n, bodies);
        const Expect e(t, n, bodies, true);
        bad += W.walk_len != static_cast<int>(e.order.size()) || W.max_saved != e.peak || W.n != n;
        if (W.route == 0) {
            bad += W.walk_len > kMaxWalk || n + W.max_saved > kJacMaxSlots;
            if (!bad) bad += check_slots(t, e, W.step, kJacMaxSlots - n);
            unsigned seen = 0;
            for (int s = 0; s < W.walk_len && !bad; s++) {
                bad += (W.step[s].own & seen) != 0;
                for (int i = 0; i < n; i++)
                    if ((W.step[s].own >> i) & 1) bad += bodies[i] != e.order[s];
                seen |= W.step[s].own;
            }
            bad += seen != (n ? ~0u >> (32 - n) : 0u);
        }
    }
    return bad;
}
// the lists: none, every single body, one body sixteen times, the first and the last sixteen bodies, up to sixteen leaves
int check_model(const HostPlan &hp, const Layout &L)
{
    int bad = 0;
    const int nbod = hp.n_bodies, m = std::min(nbod, kMaxBodyList);
    bad += check_list(hp, L, 0, nullptr);
    std::vector<int> list;
    for (int b = 0; b < nbod; b++) bad += check_list(hp, L, 1, &b);
    if (nbod == 0) return bad;
    list.assign(kMaxBodyList, nbod - 1);
    bad += check_list(hp, L, kMaxBodyList, list.data());
    list.clear();
    for (int b = 0; b < m; b++) list.push_back(b);
    bad += check_list(hp, L, m, list.data());
    list.clear();
    for (int b = nbod - m; b < nbod; b++) list.push_back(b);
    bad += check_list(hp, L, m, list.data());
    list.clear();
    for (int b = 0; b < nbod && static_cast<int>(list.size()) < kMaxBodyList; b++)
        if (!L.bodies[b].has_child) list.push_back(b);
    bad += check_list(hp, L, static_cast<int>(list.size()), list.data());
    return bad;
}
}  // namespace walkcheck

int main(int argc, char **argv)
{
    int bad = 0;
    char msg[512];
    for (int a = 1; a < argc; a++) {
        for (int ori = 0; ori < 2; ori++) {
            std::vector<unsigned char> blob;
            std::string err;
            const char *paths[1] = {argv[a]};
            int rc = 0;
            const std::string name = argv[a];
            if (name.size() > 5 && name.substr(name.size() - 5) == ".grbd") {  // a serialised model description (e.g. TelloWithArms)
                if (ori == 1) continue;
                FILE *f = std::fopen(argv[a], "rb");
                if (!f) { std::printf("%s: cannot open\n", argv[a]); bad++; continue; }
                unsigned char buf[4096];
                size_t n;
                while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
                std::fclose(f);
            } else {
                rc = grbda_hip::urdf_to_blob(paths, 1, ori, blob, err);
            }
            if (rc) { std::printf("%s: reader %d (%s)\n", argv[a], rc, err.c_str()); bad++; continue; }
            grbda_hip::HostPlan hp;
            msg[0] = 0;
            rc = compile(blob, hp, msg, sizeof msg);
            std::printf("%s ori %d: %zu bytes, plan rc %d %s nq %d nv %d chain %d\n", argv[a], ori, blob.size(), rc, msg, hp.nq, hp.nv,
                        hp.chain[grbda_hip::SLOT_F32].ok ? 1 : 0);
            if (rc) { bad++; continue; }
            const int walks = walkcheck::check_model(hp, hp.lay32) + walkcheck::check_model(hp, hp.lay64);
            std::printf("   walks of %d bodies: %d findings\n", hp.n_bodies, walks);
            if (walks) bad++;
            // the oracle on a few states (zero positions are on every explicit model's manifold; implicit models: the
            // oracle's own Newton projection first)
            const int B = 3;
            std::vector<double> q(static_cast<size_t>(B) * hp.nq, 0.0), qd(static_cast<size_t>(B) * hp.nv), tau(qd.size()), ydd(qd.size()), back(qd.size());
            std::mt19937 gen(7);
            std::uniform_real_distribution<double> U(-1, 1);
            for (auto &x : q) x = 0.3 * U(gen);
            for (auto &x : qd) x = U(gen);
            for (auto &x : tau) x = U(gen);
            const grbda_desc_header *h = reinterpret_cast<const grbda_desc_header *>(blob.data());
            if (hp.nq == hp.nv + 1 && ori == 0 && h->n_clusters > 0)
                for (int b = 0; b < B; b++) { double *o = &q[static_cast<size_t>(b) * hp.nq + 3]; o[0] = 1; o[1] = o[2] = o[3] = 0; }
            std::vector<int> ok(B, 0);
            grbda_oracle_project_positions(blob.data(), blob.size(), q.data(), B, 50, ok.data());
            rc = grbda_oracle_forward_dynamics(blob.data(), blob.size(), q.data(), qd.data(), tau.data(), nullptr, ydd.data(), B);
            if (!rc) rc = grbda_oracle_inverse_dynamics(blob.data(), blob.size(), q.data(), qd.data(), ydd.data(), nullptr, back.data(), B);
            double err_rt = 0;
            for (size_t i = 0; i < back.size(); i++)
                if (ok[i / hp.nv]) err_rt = std::max(err_rt, std::fabs(back[i] - tau[i]));
            std::printf("   oracle rc %d, ID(FD(tau)) - tau = %.2e\n", rc, err_rt);
            if (ori == 0) {  // malformed inputs: every prefix length class and a few flipped bytes must be rejected or survive cleanly
                for (size_t cut : {size_t(0), size_t(40), size_t(96), blob.size() / 2, blob.size() - 8}) {
                    std::vector<unsigned char> t(blob.begin(), blob.begin() + static_cast<long>(cut));
                    grbda_hip::HostPlan h2;
                    (void)compile(t, h2, msg, sizeof msg);
                    (void)grbda_oracle_forward_dynamics(t.data(), t.size(), q.data(), qd.data(), tau.data(), nullptr, ydd.data(), 1);
                }
                for (int trial = 0; trial < 200; trial++) {
                    std::vector<unsigned char> t(blob);
                    const size_t at = 96 + (gen() % (t.size() - 96));  // past the header: counts and offsets of bodies / clusters
                    t[at] = static_cast<unsigned char>(gen());
                    grbda_hip::HostPlan h2;
                    (void)compile(t, h2, msg, sizeof msg);
                }
            }
        }
    }
    std::printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
