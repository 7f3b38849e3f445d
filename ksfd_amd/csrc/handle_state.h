// libksfd_hip.so -- what the handle knows to be current: which derived data still belongs to the resident state and to the solver
// configuration.  Plain C++ without device code and without the handle (tests/test_handle_state_cpu.py compiles it with the host
// compiler alone).  One record, embedded in the handle once (ksfd_handle::cur); the functions below are its only writers, one per thing
// that can happen to the handle, named for what happened.  DESIGN.md ("What is current") has the table of events against products.
//
// A product's validity is a bool, the shift it was built for, or the key the coarse cycle was captured under.  The products hang on
// each other in the order the code makes them:
//     state u, parameters -> coefficient planes -> fp32 copy of the planes
//                                               -> grid means of the spectral preconditioner
//                                               -> coarse planes -> shift set-up (+ exact coarse factors) -> captured coarse cycle
// Only the link a product hangs on is ended by an event; everything behind it falls when that link is made again: ensure_coef is the
// one door to the planes and planes_recomputed ends what was made from the old ones, mg_precond asks for the coarse planes and the
// shift set-up in that order, and shift_setup_done ends the captured cycle through its key.
#pragma once

namespace ksfd_ctl {

struct Current {
    // ---- the resident state u ----
    bool coef_fresh = false;        // the coefficient planes [rho, G, G_rho, G_U..] are those of u and the parameters as they are now
    bool coef32_fresh = false;      // the fp32 copy of the planes is the rounded copy of the planes as they are now
    bool floor_ok = false;          // every owned value of u is at or above its floor (rhomin / Umin): k_groom would store what it loads
    bool ckpt_floor_ok = false;     // ... of the state in the checkpoint slot
    bool means_valid = false;       // the grid means of the spectral preconditioner are those of the planes as they are now
    // ---- multigrid ----
    bool mg_coef_valid = false;     // the coarse coefficient planes are the restriction of the planes as they are now
    double mg_shift = -1.0;         // shift the block diagonals / eigen-bounds (and the exact coarse factors) are built for; -1: no set-up in force
    bool mgc_ready = false;         // the inverse of the exact coarse solve belongs to the set-up in force (false: that set-up fell back to Chebyshev)
    double mg_graph_shift = -1.0;   // key of the captured coarse cycle: shift, the level-0 vector it reads, precision of the level vectors
    const void *mg_graph_x = nullptr;
    bool mg_graph_f32 = false;
    // ---- Krylov solvers ----
    double poly_shift = -1.0;       // shift the polynomial's coefficients are made for
    bool dr_valid = false;          // the relation A M^-1 V_kk = V_kk+1 H of the deflated solver stands in the leading slots of V (and Zb)
    bool rec_valid[4] = { false, false, false, false };   // the leading Arnoldi vectors of stage q stand in V / Zb
    int rec_vtop = 0, rec_ztop = 0; // first free slot of V / Zb behind the kept vectors
    // ---- embedded error vector ----
    bool have_err = false;          // the last completion's error vector can be handed out
    bool err_pending = false;       // ... but is not formed yet: it is sum (b2t_j - bt_j) Y_j of the stage vectors still in Y (err_materialize)
};

// the shift set-up is over.  The exact coarse factors are part of it; the captured cycle goes with the set-up that follows
// (shift_setup_done), which every cycle asks for before it looks at the graph
static inline void end_shift_setup(Current &c) { c.mg_shift = -1.0; c.mgc_ready = false; }
static inline void drop_recycled(Current &c) { for (bool &v : c.rec_valid) v = false; c.rec_vtop = c.rec_ztop = 0; }

// ---- the state and the parameters -------------------------------------------------------------------------------------------------
// u has new values (set_state, set_state_random, scale_rho, mul_rho, an accepted step, a checkpoint restore).  The planes are made of u,
// so they end; everything made of the planes ends when ensure_coef makes them again.  floor_proof: the writer knows that no value lies
// under its floor (the accepted completion counted none; the restore brings the proof the checkpoint holds)
static inline void state_written(Current &c, bool floor_proof = false) { c.coef_fresh = false; c.floor_ok = floor_proof; }
// ksfd_device_state handed out a writable pointer to u: the caller may lower values, so the floor proof ends.  The planes are
// deliberately NOT ended: callers that write through the pointer follow it with an entry that does (open question)
static inline void state_handed_out(Current &c) { c.floor_ok = false; }
// k_groom ran over u (ksfd_groom, head of a step): nothing is under its floor now.  The planes clamp rho and U the same way, so they stay
static inline void state_groomed(Current &c) { c.floor_ok = true; }
// update_params: G, G_rho, G_U depend on the parameters, so the planes end; rhomin / Umin may have moved, under the state and under
// the one in the checkpoint slot, so both floor proofs end
static inline void params_changed(Current &c) { c.coef_fresh = false; c.floor_ok = c.ckpt_floor_ok = false; }

// ---- the planes and what is made of them --------------------------------------------------------------------------------------------
// ensure_coef ran k_jcoef on the resident state.  The fp32 copy is current exactly when that launch stored it, the means exactly when
// it delivered them; the coarse planes were restricted from the old planes and the shift set-up was built on those, so both end
static inline void planes_recomputed(Current &c, bool coef32_stored, bool means_delivered)
{
    c.coef_fresh = true;
    c.coef32_fresh = coef32_stored;
    c.means_valid = means_delivered;
    c.mg_coef_valid = false;
    end_shift_setup(c);
}
static inline void coef32_made(Current &c) { c.coef32_fresh = true; }                 // ensure_coef32
static inline void means_computed(Current &c) { c.means_valid = true; }               // spec_means
static inline void coarse_planes_restricted(Current &c) { c.mg_coef_valid = true; }   // mg_restrict_coefs
// mg_setup_shift: block diagonals and Chebyshev bounds are those of `shift`; a cycle captured before replays the old bounds, so its key ends
static inline void shift_setup_done(Current &c, double shift) { c.mg_shift = shift; c.mg_graph_shift = -1.0; }
// mgc_setup: the factorization of shift*I - J_c went through / hit a zero or non-finite pivot (the set-up falls back to Chebyshev)
static inline void coarse_factors_ready(Current &c) { c.mgc_ready = true; }
static inline void coarse_factors_ended(Current &c) { c.mgc_ready = false; }
static inline bool graph_current(const Current &c, double shift, const void *x, bool f32) { return c.mg_graph_shift == shift && c.mg_graph_x == x && c.mg_graph_f32 == f32; }
static inline void graph_captured(Current &c, double shift, const void *x, bool f32) { c.mg_graph_shift = shift; c.mg_graph_x = x; c.mg_graph_f32 = f32; }

// ---- the V cycle ------------------------------------------------------------------------------------------------------------------
// the cycle is another one (set_mg_params, the mg_fuse bit of set_tuning, set_mg_coarse, set_mg_tail): bounds, sweep counts, the level it
// ends on or the launches it is made of differ, so the shift set-up ends -- and with it the exact coarse factors and, through the key,
// the captured cycle.  The coarse planes do not depend on the cycle and stay
static inline void vcycle_config_changed(Current &c) { end_shift_setup(c); }
// mg_free: the levels' buffers are gone (ksfd_set_mg_agglomerate rebuilds them, ksfd_destroy does not): coarse planes, set-up, factors
// and the captured cycle, which recorded those buffers, all end
static inline void hierarchy_freed(Current &c) { c.mg_coef_valid = false; end_shift_setup(c); c.mg_graph_shift = -1.0; }
// a test or benchmark entry set the hierarchy or the coarse factors up for a shift of its own, or is done with them (mg_coarse_apply
// op 1, the coarse-solve benchmarks, mgp_begin / mgp_end): what the levels hold is no step's set-up
static inline void hierarchy_borrowed(Current &c) { end_shift_setup(c); }

// ---- Krylov solvers ---------------------------------------------------------------------------------------------------------------
static inline void poly_set_up(Current &c, double shift) { c.poly_shift = shift; }    // poly_setup
static inline void poly_config_changed(Current &c) { c.poly_shift = -1.0; }           // set_poly_params: degree cap or target moved
// something writes the Krylov basis V from slot 0 on (basis_rotate, krylov_op, the rotation benchmarks, gmres_dr): the deflated
// solver's relation and the recycled spaces stood there.  behind_recycled: gmres() builds behind the spaces it keeps, they stay
static inline void krylov_basis_overwritten(Current &c, bool behind_recycled = false) { c.dr_valid = false; if (!behind_recycled) drop_recycled(c); }
// a solve that neither projects on the recycled spaces nor keeps its own starts (spectral sweeps, pipelined GMRES)
static inline void recycled_spaces_dropped(Current &c) { drop_recycled(c); }
static inline void recycled_space_kept(Current &c, int stage, int vtop, int ztop) { c.rec_valid[stage] = true; c.rec_vtop = vtop; c.rec_ztop = ztop; }
static inline void dr_relation_kept(Current &c) { c.dr_valid = true; }

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// ksfd_step begins: the polynomial is set up again for this step's shift and eigenvalue estimate, even at the shift of the last step
static inline void step_begins(Current &c) { c.poly_shift = -1.0; }
// an attempt with its own step size begins: it has its own matrix, so no Krylov relation is carried into it (stage 0 of every solver
// drops the recycled spaces itself).  Its stage solves overwrite Y: an error vector that is still only a promise on Y goes with it, and
// the query has nothing to return until the next completion (it fails instead of returning the vector of an older attempt)
static inline void attempt_begins(Current &c)
{
    c.dr_valid = false;
    if (c.err_pending) { c.err_pending = false; c.have_err = false; }
}
// k_rosw_finish ran.  stored: it wrote the error vector itself (old step boundary); else the vector is formed on demand from Y
static inline void completion_done(Current &c, bool stored) { c.have_err = true; c.err_pending = !stored; }
static inline void error_vector_formed(Current &c) { c.err_pending = false; }         // err_materialize
// the test entry ksfd_stage_rhs runs the stages of an attempt of its own on the caller's vectors: Y and the stored right-hand sides are
// overwritten, which is what an attempt that begins does to them.  completed: it also ran the completion and formed the error vector,
// of vectors that belong to no step -- nothing is left to hand out, as after a step that completed no attempt
static inline void stage_vectors_borrowed(Current &c, bool completed)
{
    attempt_begins(c);
    if (completed) { c.have_err = false; c.err_pending = false; }
}

// a test entry (ksfd_stage_rhs, ksfd_stage_jvp) made the planes, their fp32 copy or the means for itself: what was not current when it
// began (`before`: the record as the entry found it) is not current when it returns, so the step that follows makes it again, launch for
// launch as on a handle the entry never touched.  Only ends; what was current before and still is stays
static inline void derived_given_back(Current &c, const Current &before)
{
    c.coef_fresh = c.coef_fresh && before.coef_fresh;
    c.coef32_fresh = c.coef32_fresh && before.coef32_fresh;
    c.means_valid = c.means_valid && before.means_valid;
}

// ---- checkpoint -------------------------------------------------------------------------------------------------------------------
// save: the floor proof is a property of the state being copied
static inline void checkpoint_saved(Current &c) { c.ckpt_floor_ok = c.floor_ok; }
// restore: the state is written, with the proof the checkpoint holds; the error vector belongs to a step of the abandoned state
static inline void checkpoint_restored(Current &c) { state_written(c, c.ckpt_floor_ok); c.have_err = false; c.err_pending = false; }

}  // namespace ksfd_ctl
