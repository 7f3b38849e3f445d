// libksfd_hip.so -- which level the multigrid V cycle ends on (ksfd_set_mg_coarse), in plain C++: no device code, no handle, no
// library.  A small driver compiled with the host compiler exercises exactly what the library runs (tests/test_mg_coarse_cpu.py).
#pragma once

namespace ksfd_ctl {

// unknowns[l] = F * points of level l (level 0 = the solver's own grid, sizes fall with l), nlevels of them; cap = KSFD_MG_DIRECT_MAX.
// kind 0 (Chebyshev): the hierarchy's own coarsest level, whatever max_unknowns says.
// kind 1 (exact solve): max_unknowns <= 0: the coarsest level; > 0: the FINEST level below level 0 with at most max_unknowns unknowns.
// Returns the level, or -1 = refuse: no hierarchy (fewer than two levels), a kind other than 0 or 1, max_unknowns above the cap,
// no level that qualifies, or a chosen level with more unknowns than the cap.
static inline int mg_coarse_level(const long long *unknowns, int nlevels, int kind, long long max_unknowns, long long cap)
{
    if (nlevels < 2 || kind < 0 || kind > 1) return -1;
    if (kind == 0) return nlevels - 1;
    if (max_unknowns > cap) return -1;
    if (max_unknowns <= 0) return unknowns[nlevels - 1] <= cap ? nlevels - 1 : -1;
    for (int l = 1; l < nlevels; l++)
        if (unknowns[l] <= max_unknowns) return l;
    return -1;
}

}  // namespace ksfd_ctl
