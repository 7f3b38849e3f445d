// libksfd_hip.so -- which levels of the multigrid V cycle run as ONE workgroup launch with every level vector in the LDS
// (ksfd_set_mg_tail; kernel: k_mg_tail in mg.hip.h), in plain C++: no device code, no handle, no library.  A small driver compiled
// with the host compiler exercises exactly what the library runs (tests/test_mg_tail_cpu.py).
#pragma once

namespace ksfd_ctl {

// what a workgroup may have of the LDS on gfx950 (160 KB per CU); k_mg_tail declares no static LDS, so this is the tail's budget
constexpr long long MG_TAIL_LDS_BUDGET = 163840;
// levels one launch takes at the most: its by-value level descriptors are an array of this length
constexpr int MG_TAIL_MAX_LEVELS = 8;
// threads of the one workgroup
constexpr int MG_TAIL_THREADS = 1024;

// LDS bytes of one tail level with `points` points and F fields: the level vectors x, b, r, d (F planes each) and one dG plane, fp64.
// THE formula: the plan sums it, the kernel's carve-up advances by it, the host books the launch with it.  The coefficient planes and
// the fp32 inverse point blocks are not in it: they stay in global memory (read-only, L2-resident).
constexpr long long mg_tail_level_bytes(long long points, int F) { return 8 * points * (4 * (long long)F + 1); }

// points a tail level can have at the most with F fields: the budget bounds them, whatever max_points says
constexpr long long mg_tail_max_points(int F, long long budget = MG_TAIL_LDS_BUDGET) { return budget / mg_tail_level_bytes(1, F); }
// ... and so the points ONE thread of the workgroup owns at the most (the trip count of the kernel's point loops, a compile-time number)
constexpr int mg_tail_points_per_thread(int F) { return (int)((mg_tail_max_points(F) + MG_TAIL_THREADS - 1) / MG_TAIL_THREADS); }

// points[l], local[l] of levels 0 .. end (end = the level the cycle ends on); local: the level is whole on this rank with wrapped indices
// (a single-rank handle without a halo transport, or a replicated level of slab ranks) -- a distributed level (ghost units, halo
// exchange) never qualifies.  Returns the first tail level t: the SMALLEST t >= 1 for which every level t .. end is local, has at most
// max_points points, and the levels together fit the budget (sum of mg_tail_level_bytes) -- in at most MG_TAIL_MAX_LEVELS levels.
// -1: no such level, max_points <= 0 (off), no hierarchy (end < 1), F < 1.  Level 0 is never part of the tail.
// lds_bytes (may be NULL): the sum over the tail's levels, 0 with -1.
static inline int mg_tail_first_level(const long long *points, const int *local, int end, int F, long long max_points, long long budget,
                                      long long *lds_bytes)
{
    if (lds_bytes) *lds_bytes = 0;
    if (end < 1 || F < 1 || max_points <= 0) return -1;
    int t = -1;
    long long sum = 0;
    for (int l = end; l >= 1 && end - l < MG_TAIL_MAX_LEVELS; l--) {
        if (!local[l] || points[l] < 1 || points[l] > max_points) break;
        const long long s = sum + mg_tail_level_bytes(points[l], F);
        if (s > budget) break;
        sum = s;
        t = l;
    }
    if (t < 0) return -1;
    if (lds_bytes) *lds_bytes = sum;
    return t;
}

}  // namespace ksfd_ctl
