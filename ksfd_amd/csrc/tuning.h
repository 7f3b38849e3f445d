// libksfd_hip.so -- the switches that choose between code paths: what the caller wished for through ksfd_set_tuning (the tuning word
// KSFD_TUNE_* of include/ksfd_hip.h, the segment lengths) and through the -7 rule of ksfd_set_mg_params.  Plain C++ without device code
// and without the handle (tests/test_tuning_cpu.py compiles it with the host compiler alone).  One record, embedded in the handle once
// (ksfd_handle::tune); the two functions below are its only writers.  A field is a wish: what also takes a fact about the handle (a
// mapped result buffer, no collectives inside the cycle) is asked through zero_copy_on / mg_graph_on in handle.hip.h.
// DESIGN.md ("Switches") has the table of every switch: where it is read, which test sets it, what was measured.
#pragma once
#include <stdint.h>
#include "../../include/ksfd_hip.h"

namespace ksfd_ctl {

struct Tuning {
    // ---- operators ----
    bool use_fused = true;          // strip kernels of the RHS and of the Jacobian action where the grid allows them (ops.hip.h: jvp_path)
    bool use_frozen = true;         // Jacobian action from the frozen coefficient planes
    bool overlap = true;            // halo exchange overlapped with the interior rows
    bool fuse_stage = true;         // stage-vector algebra inside the RHS kernel (2-D strip path; 3-D: inside the G pass + strip kernel)
    bool rhs3d_strip = true;        // 3-D RHS: G pass + z-marching strip kernel (false: generic one-thread-per-point stencil pass)
    bool rhs_carry = true;          // stage vectors that enter both sides of a stage RHS are read once (k_rhs2d_fused<NL, true>)
    bool rhs_dots = true;           // inner products for the stage guesses from the RHS kernel's store epilogue
    bool rhs_gplane = true;         // stage-0 RHS of the 2-D strip path takes G from plane 1 of coef
    bool zero_copy = true;          // reduction results through the mapped flag
    // ---- Krylov solvers ----
    int async_mode = 0;             // pipelined GMRES: 0 off (measured no gain on one GPU, tools/async_bench.py), 1 whenever legal, 2 when the
                                    // local problem is small (no bit sets 2)
    int rec_mode = 1;               // recycling across the stage systems of a step: 0 off, 1 selected earlier stages, 2 every earlier stage
    int rec_keep = 3;               // leading vectors kept per stage (<= 4)
    bool rec_mg = false;            // multigrid-preconditioned solves keep the WHOLE first cycle of every stage (measured: no gain, see gmres)
    bool restart_grow = true;       // a GMRES cycle that ends without convergence is followed by one of twice the length
    bool poly_fp32 = true;          // Horner temporaries and coefficients of p(A) in fp32 storage (the outer A z_j stays fp64)
    // ---- spectral solver ----
    bool spec_guess = true;         // stage solves start from the span of the earlier stage solutions of the step
    bool spec_predict = true;       // predicted last sweep of the defect correction (spec_solve)
    // ---- multigrid ----
    bool mg_fuse = true;            // smoother algebra inside the Jacobian-action epilogues (modes 5/6)
    bool mg_warm_power = true;      // power iteration of a level starts from the vector of the previous set-up
    bool mg_fp32 = true;            // V cycle with fp32 level vectors when the solve tolerance allows; see mg_vcycle
    bool mg_use_graph = true;       // coarse part of the V cycle replayed from a captured graph
    // ---- the step ----
    bool old_boundary = false;      // groom every step, error vector stored by the completion, fp32 coefficient copy made by k_jcoef
    // ---- launch geometry ----
    int yseg = 48;        // rows per wave segment, RHS kernel (tools/kbench.py at 4096^2 with the hand-rolled log/exp: 8: 0.253, 16: 0.222, 32: 0.198, 64: 0.190 ms)
    int yseg_jvp = 16;    // same for the Jacobian-action kernels
    int zseg = 32;        // planes per wave segment, 3-D z-marching kernel (no entry sets it)
};

// ksfd_set_tuning.  A negative word changes no switch; any other word replaces every one of them, except that 0 in the rec_keep field
// keeps the count in force.  yseg / yseg_jvp <= 0 keep theirs
static inline void tuning_apply(Tuning &t, int32_t word, int32_t yseg, int32_t yseg_jvp)
{
    if (word >= 0) {
        t.use_fused = (word & KSFD_TUNE_FUSED) != 0;
        t.use_frozen = !(word & KSFD_TUNE_RECOMPUTE_JVP);
        t.overlap = !(word & KSFD_TUNE_NO_OVERLAP);
        t.async_mode = (word & KSFD_TUNE_ASYNC_GMRES) ? 1 : 0;
        t.rec_mode = (word & KSFD_TUNE_NO_RECYCLE) ? 0 : ((word & KSFD_TUNE_RECYCLE_ALL) ? 2 : 1);
        const int keep = (word & KSFD_TUNE_REC_KEEP_MASK) / KSFD_TUNE_REC_KEEP(1);
        if (keep) t.rec_keep = keep < 4 ? keep : 4;
        t.poly_fp32 = !(word & KSFD_TUNE_POLY_FP64);
        t.fuse_stage = !(word & KSFD_TUNE_UNFUSED_STAGE);
        t.zero_copy = !(word & KSFD_TUNE_NO_ZERO_COPY);
        t.mg_fuse = !(word & KSFD_TUNE_UNFUSED_SMOOTHER);
        t.rhs3d_strip = !(word & KSFD_TUNE_GENERIC_RHS3D);
        t.spec_guess = !(word & KSFD_TUNE_NO_SPEC_GUESS);
        t.rhs_carry = !(word & KSFD_TUNE_NO_RHS_CARRY);
        t.spec_predict = !(word & KSFD_TUNE_NO_SPEC_PREDICT);
        t.restart_grow = !(word & KSFD_TUNE_NO_RESTART_GROWTH);
        t.mg_warm_power = !(word & KSFD_TUNE_COLD_POWER);
        t.mg_fp32 = !(word & KSFD_TUNE_MG_FP64);
        t.rec_mg = (word & KSFD_TUNE_REC_MG) != 0;
        t.rhs_dots = !(word & KSFD_TUNE_OWN_DOTS);
        t.old_boundary = (word & KSFD_TUNE_OLD_BOUNDARY) != 0;
        t.rhs_gplane = !(word & KSFD_TUNE_NO_GPLANE);
    }
    if (yseg > 0) t.yseg = yseg;
    if (yseg_jvp > 0) t.yseg_jvp = yseg_jvp;
}

// ksfd_set_mg_params: power_its = KSFD_MG_EAGER asks for eager launches of the coarse cycle; every other call of that entry asks for
// the captured graph again
static inline void tuning_mg_graph(Tuning &t, int32_t power_its) { t.mg_use_graph = power_its != KSFD_MG_EAGER; }

}  // namespace ksfd_ctl
