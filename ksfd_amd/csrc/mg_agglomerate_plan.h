// libksfd_hip.so -- the level list of the multigrid hierarchy on slab ranks with coarse-level agglomeration (ksfd_set_mg_agglomerate),
// in plain C++: no device code, no handle, no library.  A small driver compiled with the host compiler exercises exactly what the
// library runs (tests/test_mg_agglomerate_cpu.py).
#pragma once

namespace ksfd_ctl {

struct MGPlanLevel {
    long long n[3];      // GLOBAL extents per axis (1 on the axes the grid does not have)
    long long sloc;      // slow units this rank computes: its slab on a distributed level, the whole slow extent on a replicated one
    int rep;             // 0: distributed over the slab ranks (ghost units, halo exchange); 1: replicated, every rank holds the whole level
};

// Level list for a grid of `dim` axes with global extents n[] (the slow axis, dim - 1, is cut into `ranks` equal slabs).
// ring: the handle has a halo transport (also a ring of one rank).  A pure function of its arguments: every rank gets the same list.
//
// Distributed levels coarsen while every extent is even and keeps >= 8 points after halving (the slow axis: the LOCAL count is even, so
// that every slab starts on a coarse unit, and the GLOBAL count keeps >= 8) -- and, on a ring, while every rank keeps >= 4 slow units
// (ghost width 2 + the 4th-order star).  max_points = 0 ends the hierarchy there: the rule of a handle without agglomeration.
// max_points > 0, on a ring: the level the 4-units rule refuses is replicated instead, and so is, earlier, every level below level 0
// whose GLOBAL point count is <= max_points.  Below the first replicated level everything is replicated and coarsens by the single-rank
// rule on the global extents.  Returns the number of levels written (at most cap; level 0 is always there), or -1 for arguments that
// describe no grid.
static inline int mg_agglomerate_plan(int dim, const long long *n, int ranks, int ring, long long max_points, MGPlanLevel *out, int cap)
{
    if (dim < 1 || dim > 3 || ranks < 1 || max_points < 0 || cap < 1) return -1;
    const int slow = dim - 1;
    long long g[3] = { 1, 1, 1 };
    for (int a = 0; a < dim; a++) { if (n[a] < 1) return -1; g[a] = n[a]; }
    if (g[slow] % ranks) return -1;
    const bool agg = ring && max_points > 0 && dim > 1;
    bool rep = false;
    int nl = 0;
    for (;;) {
        MGPlanLevel &L = out[nl++];
        for (int a = 0; a < 3; a++) L.n[a] = g[a];
        L.sloc = rep ? g[slow] : g[slow] / ranks;
        L.rep = rep ? 1 : 0;
        if (nl == cap) break;
        // the next level exists by the rule of the global grid ...
        bool ok = true;
        for (int a = 0; a < dim; a++) ok = ok && g[a] % 2 == 0 && g[a] / 2 >= 8;
        if (!rep) ok = ok && L.sloc % 2 == 0;
        if (!ok) break;
        // ... and stays distributed, becomes replicated, or (no agglomeration) ends the hierarchy at the 4-units rule
        if (!rep) {
            const bool refused = ring && L.sloc / 2 < 4;
            const long long pts = (g[0] / 2) * (dim > 1 ? g[1] / 2 : 1) * (dim > 2 ? g[2] / 2 : 1);
            if (agg && (refused || pts <= max_points)) rep = true;
            else if (refused) break;
        }
        for (int a = 0; a < dim; a++) g[a] /= 2;
    }
    return nl;
}

}  // namespace ksfd_ctl
