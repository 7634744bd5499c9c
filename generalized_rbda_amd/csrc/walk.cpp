// walk.cpp -- the host builders of the ancestor walks (walk.h): ONE depth-first traversal with the save / restore slot allocator, and per
// walk kernel what is its own: the order of a body's children, the step record, the conditions under which the record fits, the route.
#include "walk.h"

#include <algorithm>

namespace grbda_hip {

namespace {

// per body: its cluster
std::vector<int> clusters_of_bodies(const Layout &L, int n_bodies)
{
    std::vector<int> cluster_of(static_cast<size_t>(n_bodies), -1);
    for (size_t ci = 0; ci < L.clusters.size(); ci++)
        for (int i = 0; i < L.clusters[ci].k; i++) cluster_of[L.clusters[ci].first_body + i] = static_cast<int>(ci);
    return cluster_of;
}
// the tree parent; a floating base hangs off nothing
int parent_of(const Layout &L, const std::vector<int> &cluster_of, int b)
{
    return L.clusters[cluster_of[b]].kind == CK_FREE ? -1 : L.bodies[b].parent;
}
bool in_cluster_child(const Layout &L, const std::vector<int> &cluster_of, int b, int par)
{
    return L.bodies[b].lam == par && cluster_of[b] == cluster_of[par];
}

// The traversal both builders share: depth first from `roots`, the children of body b in the order of kids[b].  A body with two or more
// children keeps its value in a save slot, the lowest free one; its first child continues from the running value, the others start from
// the saved one and the last of them frees the slot.  visit(step, body, save slot or -1, restore slot or -1) per step, in walk order; the
// slot numbers are not capped here.
struct WalkShape {
    int walk_len = 0, max_saved = 0;
};
template <class Visit>
WalkShape traverse(const std::vector<int> &roots, const std::vector<std::vector<int>> &kids, Visit &&visit)
{
    WalkShape shape;
    std::vector<char> slot_used;
    int in_use = 0;
    // iteratively: (body, restore slot or -1, whether this is the last child to read that slot)
    struct Item {
        int body, restore;
        bool last;
    };
    std::vector<Item> stack;
    for (auto it = roots.rbegin(); it != roots.rend(); ++it) stack.push_back({*it, -1, false});
    while (!stack.empty()) {
        const Item item = stack.back();
        stack.pop_back();
        const std::vector<int> &ch = kids[item.body];
        if (item.restore >= 0 && item.last) {  // (the step reads the slot before it writes one of its own)
            slot_used[item.restore] = 0;
            in_use--;
        }
        int save = -1;
        if (ch.size() >= 2) {
            size_t sl = 0;
            while (sl < slot_used.size() && slot_used[sl]) sl++;
            if (sl == slot_used.size()) slot_used.push_back(0);
            slot_used[sl] = 1;
            save = static_cast<int>(sl);
            in_use++;
            shape.max_saved = std::max(shape.max_saved, in_use);
        }
        visit(shape.walk_len++, item.body, save, item.restore);
        for (size_t k = ch.size(); k-- > 0;) stack.push_back({ch[k], k == 0 ? -1 : save, k + 1 == ch.size()});
    }
    return shape;
}
uint8_t slot_field(int slot, int cap) { return static_cast<uint8_t>(slot >= 0 && slot < cap ? slot : kWalkNone); }

}  // namespace

BodyWalkHost build_body_walk(const HostPlan &h, const Layout &L, int n, const int *bodies)
{
    BodyWalkHost W;
    W.n = W.list.n = n;
    for (int i = 0; i < kMaxBodyList; i++) W.list.body[i] = i < n ? bodies[i] : -1;
    const int nbod = h.n_bodies;
    std::vector<char> in_walk(static_cast<size_t>(nbod), 0);
    for (int i = 0; i < n; i++)
        for (int b = bodies[i]; b >= 0 && !in_walk[b]; b = L.bodies[b].parent) in_walk[b] = 1;
    const std::vector<int> cluster_of = clusters_of_bodies(L, nbod);
    // per cluster: its first spanning rate
    std::vector<int> span_at(L.clusters.size(), 0);
    int at = 0;
    for (size_t ci = 0; ci < L.clusters.size(); ci++) {
        span_at[ci] = at;
        at += L.clusters[ci].kind == CK_FREE ? 6 : L.clusters[ci].k;
    }
    // children in the walk, in index order (a parent precedes its children in the plan's body order)
    std::vector<std::vector<int>> kids(static_cast<size_t>(nbod));
    std::vector<int> roots;
    for (int b = 0; b < nbod; b++) {
        if (!in_walk[b]) continue;
        const int par = parent_of(L, cluster_of, b);
        (par < 0 ? roots : kids[par]).push_back(b);
    }
    bool fits = nbod <= 32767 && h.nq <= 32767 && at <= 32767;
    int n_slots_out = 0;
    const WalkShape shape = traverse(roots, kids, [&](int s, int b, int save, int restore) {
        int n_out = 0;
        for (int i = 0; i < n; i++)
            if (bodies[i] == b) {
                W.slot[n_slots_out++] = static_cast<uint8_t>(i);
                n_out++;
            }
        if (s >= kMaxWalk || !fits) return;
        const int ci = cluster_of[b];
        const ClusterRec &c = L.clusters[ci];
        const BodyRec &br = L.bodies[b];
        const int i = b - c.first_body;
        BodyWalkStep &st = W.step[s];
        st.cofs = br.cofs;
        st.body = static_cast<int16_t>(b);
        st.free = c.kind == CK_FREE;
        st.q_col = static_cast<int16_t>(c.kind == CK_LOOP ? c.q_index + i : c.q_index);
        st.span_col = static_cast<int16_t>(span_at[ci] + (c.kind == CK_FREE ? 0 : i));
        st.n = static_cast<uint8_t>(c.kind == CK_LOOP || c.kind == CK_FREE ? 0 : c.n);
        fits = fits && (c.kind == CK_LOOP || c.kind == CK_FREE || (c.n >= 1 && c.n <= 255));
        st.axis = static_cast<uint8_t>(br.axis);
        st.canon = static_cast<uint8_t>(br.canon_axis);
        st.root = parent_of(L, cluster_of, b) < 0;
        st.save = slot_field(save, kMaxSaved);
        st.restore = slot_field(restore, kMaxSaved);
        st.n_out = static_cast<uint8_t>(n_out);
    });
    W.walk_len = shape.walk_len;
    W.max_saved = shape.max_saved;
    W.route = (W.walk_len > kMaxWalk || W.max_saved > kMaxSaved || !fits) ? 1 : 0;
    return W;
}

JacWalkHost build_jac_walk(const HostPlan &h, const Layout &L, int n, const int *bodies)
{
    JacWalkHost W;
    W.n = n;
    const int nbod = h.n_bodies;
    const std::vector<int> cluster_of = clusters_of_bodies(L, nbod);
    bool ok = !h.big_clusters && h.nv <= 64 * kJacMaskWords && nbod <= 32767 && h.nq <= 32767;
    const bool masks = h.nv <= 64 * kJacMaskWords;
    std::vector<unsigned> below(static_cast<size_t>(nbod), 0);
    for (int i = 0; i < n; i++) {
        W.canon[i] = static_cast<uint8_t>(L.bodies[bodies[i]].canon_axis);
        if (!masks) W.cols[i][0] = W.cols[i][1] = ~0ull;
        for (int b = bodies[i]; b >= 0; b = parent_of(L, cluster_of, b)) {
            below[b] |= 1u << i;
            const ClusterRec &c = L.clusters[cluster_of[b]];
            const int nc = c.kind == CK_FREE ? 6 : c.n;
            if (masks)
                for (int k = c.v_index; k < c.v_index + nc; k++) W.cols[i][k >> 6] |= 1ull << (k & 63);
            if (c.kind == CK_FREE) ok = ok && L.bodies[b].canon_axis == 2;
            else ok = ok && c.kind == CK_STATIC && c.n >= 1 && c.n <= kJacMaxDof && L.bodies[b].jtype == 0;
        }
    }
    // children in the walk: the in-cluster child first, the others in index order
    std::vector<std::vector<int>> kids(static_cast<size_t>(nbod));
    std::vector<int> roots;
    for (int b = 0; b < nbod; b++) {
        if (!below[b]) continue;
        const int par = parent_of(L, cluster_of, b);
        if (par < 0) roots.push_back(b);
        else if (in_cluster_child(L, cluster_of, b, par)) {
            if (!kids[par].empty() && in_cluster_child(L, cluster_of, kids[par][0], par)) ok = false;
            kids[par].insert(kids[par].begin(), b);
        } else kids[par].push_back(b);
    }
    const WalkShape shape = traverse(roots, kids, [&](int s, int b, int save, int restore) {
        if (s >= kMaxWalk || !ok) return;
        const ClusterRec &c = L.clusters[cluster_of[b]];
        const BodyRec &br = L.bodies[b];
        JacWalkStep &st = W.step[s];
        st.cofs = br.cofs;
        st.free = c.kind == CK_FREE;
        st.q_col = static_cast<int16_t>(c.q_index);
        st.v_col = static_cast<int16_t>(c.v_index);
        st.n = static_cast<uint8_t>(st.free ? 0 : c.n);
        st.axis = static_cast<uint8_t>(br.axis);
        st.root = parent_of(L, cluster_of, b) < 0;
        st.save = slot_field(save, kJacMaxSlots);
        st.restore = slot_field(restore, kJacMaxSlots);
        st.cont = !st.root && in_cluster_child(L, cluster_of, b, br.parent);
        st.below = static_cast<uint16_t>(below[b]);
        unsigned deeper = 0;  // frames that meet the cluster again further down
        if (!kids[b].empty() && in_cluster_child(L, cluster_of, kids[b][0], b)) deeper = below[kids[b][0]];
        st.emit = static_cast<uint16_t>(below[b] & ~deeper);
        for (int i = 0; i < n; i++)
            if (bodies[i] == b) st.own |= static_cast<uint16_t>(1u << i);
    });
    W.walk_len = shape.walk_len;
    W.max_saved = shape.max_saved;
    W.route = (!ok || W.walk_len > kMaxWalk || n + W.max_saved > kJacMaxSlots) ? 1 : 0;
    return W;
}

}  // namespace grbda_hip
