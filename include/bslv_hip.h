/*
 * bslv_hip.h -- C ABI of libbslv_hip.so, the MI355X-native engine behind the two inner loops of
 * BENSOLVE's Benson outer-approximation algorithm.
 *
 * Every entry point is plain C: pointers, sizes, ints.  No torch / HIP types cross the boundary.
 * All pointers are HOST pointers unless the name ends in _dev.  Return value 0 = success,
 * non-zero = BSLV_E_* error (bslv_last_error() has the text).  The library never falls back
 * to a CPU path: if no gfx950 device is usable every constructor fails with BSLV_E_NODEVICE.
 *
 * Reference interfaces replaced (file:line relative to the reference tree):
 *   - bslv_lp.h:27-105   the 17 lp_* functions bslv_algs.o / bslv_main.o import
 *                        (one global glp_prob, bslv_lp.c:31)            -> section 1 + section 3
 *   - bslv_poly.h:90-118 the poly__* functions and the polytope / poly_args structs
 *                        (bslv_poly.h:55-82)                            -> section 2 + section 3
 *   - bslv_algs.c:958-1161 phase2_primal's inner loop (one vertex -> one LP -> one cut)
 *                        re-shaped into batch -> kernels -> gather      -> section 4
 */
#ifndef BSLV_HIP_H
#define BSLV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    BSLV_OK = 0,
    BSLV_E_NODEVICE = 1,   /* no usable HIP device / HIP call failed */
    BSLV_E_ARG = 2,        /* bad argument */
    BSLV_E_NOMEM = 3,      /* device or host allocation failed / pool exhausted */
    BSLV_E_CAPACITY = 4,   /* a fixed-capacity device array overflowed */
    BSLV_E_STATE = 5       /* call out of order */
};

/* LP status codes: same numbering as lp_status_type (bslv_lp.h:47). */
enum { BSLV_LP_INFEASIBLE = 0, BSLV_LP_UNBOUNDED = 1, BSLV_LP_UNEXPECTED = 2, BSLV_LP_UNDEFINED = 3, BSLV_LP_OPTIMAL = 4 };

const char *bslv_last_error(void);
int bslv_device_count(void);
/* the GPU the calling thread's engines live on from now (one process per GPU: LOCAL_RANK); engines are created on the
 * current HIP device of the thread that creates them */
int bslv_set_device(int device);
/* name / CU count / total global memory of the device the calling thread uses */
int bslv_device_info(char *name, int name_len, int *cus, size_t *mem_bytes);

/* ------------------------------------------------------------------------------------------
 * 1. Batched scalar-LP engine  (replaces lp_solve + getters, bslv_lp.c:219-308, for batches)
 *
 * Model (GLPK's, as bslv_lp.c uses it): auxiliary variables r = A x; every variable -- aux
 * 0..M-1, structural M..M+N-1 -- has bounds [lb,ub] (+-INFINITY allowed); minimise cost.x + c0.
 * A contiguous range of variables [var_first, var_first+var_cnt) gets PER-LP bounds: these are
 * the r rows  R_j.y - z <= R_j.v  of P2(v) (bslv_algs.c:637-649,1041-1048).
 *
 * State lives in a pool of TABLEAU SLOTS resident in HBM.  A slot holds one LP's dense compact
 * simplex tableau x_B = T x_N (with reduced-cost row and basic values), so a solved slot is a
 * warm start for any other right-hand side: every slot that reached optimality is dual feasible
 * for every v.  solve_batch copies src -> dst, installs the new bounds, and runs the bounded dual
 * simplex in lock step over the batch.
 * ------------------------------------------------------------------------------------------ */
typedef struct bslv_lpq bslv_lpq;

int  bslv_lpq_create(bslv_lpq **out, int M, int N,
                     const double *A /* M*N row-major */,
                     const double *lb, const double *ub /* M+N each */,
                     const double *cost /* N+1: cost[0] = constant shift (bslv_lp.h:33) */,
                     int var_first, int var_cnt, int pool_slots);
void bslv_lpq_destroy(bslv_lpq *h);
/* PRESOLVE at this boundary: a row of A with a single non-zero outside the per-LP range is a bound on its column (the rows `d 0 1`
 * over free columns of ex/example10.m:21-24); it is folded into the column's bounds and leaves the tableau.  Every index of this
 * interface stays an index of the model AS GIVEN (GLPK's, bslv_lp.c:60-70): get_primal of a folded row returns a_ij x_j, get_dual
 * the column's reduced cost over a_ij when the column sits on the bound that row gave it.  BSLV_NO_PRESOLVE=1 switches it off. */
int  bslv_lpq_rows_folded(const bslv_lpq *h);
/* REVISED FORM (the reference hands A to its solver as COO, bslv_lp.c:60-70 -> glp_load_matrix): for wide sparse
 * problems the engine can keep the BASIS INVERSE of every LP (M x M) instead of its tableau ((M+1) x N) and A once, as CSC and CSR,
 * for the whole pool; tableau rows and columns are sparse products, the delayed update and its pass kernel run on B^-1 (ex09 of the
 * reference's suite: 171 MB per LP instead of 1.36 GB).  Same interface, same slots and warm starts, bslv_lpq_solve_batch_obj included
 * (the new reduced-cost row is one tableau row built from y = sum of c_t times the rows of the parent's B^-1 that hold the basic
 * cost-carrying variables).  Within a solve B^-1 is only ever updated, and children inherit it from their parents: an LP whose inverse
 * has drifted (the pivot element from its row and from its column disagree) comes back BSLV_LP_UNDEFINED for the caller's retry from the
 * standard basis (bslv_lp.c:222-227) -- unless the refactorisation below is switched on, which is off by default.  Chosen by itself
 * for N >= 2 M, < 2 % non-zeros and tableaux of 4 GiB and more; BSLV_LP_REV=0 / 1 forces the form.  Returns 1 in the revised form. */
int  bslv_lpq_is_revised(const bslv_lpq *h);
/* REFACTORISATION (revised form only; the tableau form answers BSLV_E_ARG, its message names the tableau form).
 * bslv_lpq_refactor rebuilds B^-1 of the n named slots (distinct) in place from their basis heads alone -- nothing numeric in the
 * slot's matrix is read: the slot is set to the identity and the structural basic variables enter one after the other in ascending
 * variable id, each on the row partial pivoting chooses among the rows whose auxiliary variable is nonbasic, as ordinary pending
 * pivots of the engine (KP steps per pass, at most ceil(M / KP) + 2 rounds for all slots in lock step).  The result is a function of
 * the heads and the model.  Afterwards the heads of the basic variables name the rows they ended in (the basis as a set, the nonbasic
 * heads, statuses and values stay), the reduced costs are rebuilt for the ENGINE'S OWN cost vector -- a slot that an objective batch
 * produced gets the own-cost (zero) row, bslv_lpq_solve_batch_obj rebuilds its row from y anyway -- and the basic values are
 * recomputed.  status_out[b] (may be NULL): 0, or BSLV_LP_UNDEFINED for a singular basis (a pivot with |v_r| <= 1e-9 (1 + max |v|))
 * or inconsistent heads; such a slot is reset to the standard basis as by bslv_lpq_reset_slot.  Errors: tableau form, bad slot (out of
 * range or named twice), n < 0.
 * bslv_lpq_set_refactor(h, 1) (BSLV_LP_REFACTOR=1 when an engine comes up in the revised form; the tableau form ignores the variable
 * and answers BSLV_E_ARG to on = 1): an LP that the pivot cross-check gives up is, after the rounds of the batch and inside the same
 * solve_batch / solve_batch_obj call, refactorised in its dst slot and solved again in place with its own bounds (and costs), at
 * most 3 times per LP and call; iters[] add up and bslv_lpq_last_stats covers the whole call.  It stays BSLV_LP_UNDEFINED, as without
 * the switch, when the restart is refused or it fails again at the cap.  With the switch off nothing changes.
 * bslv_lpq_last_refactor_stats, of the last solve call or explicit refactor: [0] slots refactorised, [1] replay pivots, [2] LPs
 * rescued (they ended with a status other than UNDEFINED), [3] refactorisations that failed or rescues that stayed UNDEFINED. */
int  bslv_lpq_refactor(bslv_lpq *h, int n, const int *slots, int *status_out);
int  bslv_lpq_set_refactor(bslv_lpq *h, int on);
int  bslv_lpq_get_refactor(const bslv_lpq *h);
int  bslv_lpq_last_refactor_stats(const bslv_lpq *h, long out[4]);
/* PERIODIC REFACTORISATION inside a solve (revised form only; off by default, and with the period at 0 every launch and every result
 * is what it is without it).  Every slot has an AGE: the rank-1 steps applied to its matrix since it was last built from the identity.
 * bslv_lpq_reset_slot, a successful bslv_lpq_refactor, a refactorisation of the rescue above and one made by the period set it to 0; a
 * solve leaves age[dst] = age[src] + the LP's own steps since its last refactorisation inside the solve (in place too).  The ages live
 * beside the pool (bslv_lpq_slot_bytes is what it was) and are kept whether a period is set or not; bslv_lpq_slot_age reads one (the
 * tableau form reports 0).  The steps of a solve are counted as its iterations: a primal step in which the entering variable only switches
 * bound counts too, so the age never underestimates.
 * bslv_lpq_set_refactor_period(h, K): 0 = off; K < 0 is BSLV_E_ARG; the tableau form answers BSLV_E_ARG to K > 0 (its message names the
 * tableau form) and accepts 0.  BSLV_LP_REFACTOR_EVERY=K sets the period when an engine comes up in the revised form; the tableau form
 * ignores the variable.  Independent of bslv_lpq_set_refactor: both may be on, the pivot cross-check and the rescue stay as they are.
 * With K > 0, in bslv_lpq_solve_batch and bslv_lpq_solve_batch_obj alike:
 *  - at the START of a call an LP that was accepted and whose parent's age is >= K is refactorised in its dst slot, from the heads it
 *    inherited, before its first selection; it then has its own matrix, and no number of the parent's matrix enters what it computes;
 *  - during the ROUNDS the ages are checked where the host reads the status vector back, which with a period happens at least every
 *    max(1, K / KP) rounds (KP = 6 pivots per round): a running LP whose age is >= K there is refactorised and GOES ON.  It keeps its
 *    bounds, nonbasic statuses and values, iteration count, perturbation, stall and Bland state and its place in the batch; the matrix,
 *    the heads of the basic variables (they follow the rows the replay put them in), the basic values and the TRUE reduced costs
 *    d_j = c_j - y K_j, y = sum_i c[bh_i] X[i, :] -- c being the LP's own cost in an objective batch -- are rebuilt before its next
 *    selection; a perturbed cost row keeps its offsets to the true one.  No selection is made on an inverse older than 2 K + KP: a
 *    bound that follows from the readback rule (derived, not measured); the statistics report the largest age met;
 *  - a replay that finds the basis singular ends that LP BSLV_LP_UNDEFINED and its slot is reset as by bslv_lpq_reset_slot; the rescue,
 *    if on, and the callers' retries see it like any other UNDEFINED.
 * bslv_lpq_last_period_stats, summed over the last solve call: [0] refactorisations made at the start, [1] during the rounds, [2] replay
 * pivots, [3] the largest age at which any selection was made.  bslv_lpq_last_refactor_stats does not count these; bslv_lpq_last_stats
 * (total_ms, and update_ms with the profile on) and bslv_lpq_last_passes cover the replay's passes. */
int  bslv_lpq_set_refactor_period(bslv_lpq *h, int pivots);
int  bslv_lpq_get_refactor_period(const bslv_lpq *h);
int  bslv_lpq_slot_age(const bslv_lpq *h, int slot, long *age);
int  bslv_lpq_last_period_stats(const bslv_lpq *h, long out[4]);
/* Test and diagnostic support of the revised form, plain C ABI like everything here.  bslv_lpq_get_inverse: the basis heads (M
 * variable ids: 0..M-1 auxiliary, M.. structural) and, unless X is NULL, the stored matrix of a slot, M x M row-major, in the indices
 * of the engine's own model (M = rows given minus bslv_lpq_rows_folded).  bslv_lpq_debug_perturb_inverse multiplies entry (i, c) of
 * the stored matrix by 1 + rel (1 + hash01(i M + c)): a deterministic stand-in for drift, for tests only.  BSLV_LP_REV_DRIFT=b:p
 * (test hook, read per solve call, off by default): the pivot cross-check of LP b of the batch is taken as failed at the LP's p-th
 * pivot (p >= 1), once per call and not again in the in-call rescue; nothing else changes.  bslv_lpq_debug_swap_heads, for tests only:
 * the basic variable of row r and the nonbasic variable at position q (0 .. N-1 of the slot's nonbasic list; position j of a reset slot
 * holds structural j) change places in the heads of the slot; the variable that leaves gets the nonbasic status and value of its
 * bounds in the model.  The stored matrix is not touched and belongs to the old basis until bslv_lpq_refactor rebuilds it. */
int  bslv_lpq_get_inverse(bslv_lpq *h, int slot, int *heads /* M */, double *X /* M x M row-major, may be NULL */);
int  bslv_lpq_debug_perturb_inverse(bslv_lpq *h, int slot, double rel);
int  bslv_lpq_debug_swap_heads(bslv_lpq *h, int slot, int r, int q);
/* A BASIS TAKEN OUT OF A SLOT AND PUT INTO ONE, in both forms (GLPK has glp_get_row_stat / glp_set_row_stat beside glp_std_basis; the
 * reference itself only ever calls glp_std_basis, bslv_lp.c:101,225).  Every index is one of the engine's OWN model, as in
 * bslv_lpq_get_inverse: M = rows given minus bslv_lpq_rows_folded, variables 0..M-1 auxiliary, M..M+N-1 structural.
 * bslv_lpq_var_map is the one translation a caller needs: own_of_given[v] for every variable v of the model as given (M_given + N), -1
 * for a folded row.  The status codes are GLPK's GLP_BS .. GLP_NS.
 * bslv_lpq_get_basis: vstat[k] of every variable of a slot that may be passed as `src` and, unless row_of is NULL, the row of a basic
 * variable (-1 otherwise).  Heads and statuses follow every committed pivot, so a parked or lazily open slot answers what it answers after
 * bslv_lpq_materialise.  A nonbasic variable is reported by the side the engine holds it on -- LOWER / UPPER also where that bound is one
 * of the engine's artificial ones (+-1e7 in place of an infinite bound on the side a cost needs), which load_basis accepts back -- FIXED
 * where its bounds were equal in the solve that left it, FREE where it rests at 0 without a bound.  A slot that bslv_lpq_reset_slot left
 * reports every structural LOWER: the standard basis' placeholder, which the next solve replaces by the side the bounds allow.
 * bslv_lpq_load_basis installs the basis vstat[b * (M + N) ..] in slot slots[b] (distinct, as for bslv_lpq_refactor).  Nothing numeric
 * in the slot is read.  Nonbasic values come from the bound the status names: vlo / vup[b * var_cnt ..] inside the per-LP range (both
 * NULL: the model's bounds there too), the model's bounds (with the artificial ones) elsewhere, FREE is 0; a LOWER / UPPER variable whose
 * two bounds are equal is held as FIXED.  The tableau form rebuilds the slot's tableau on the device: the slot starts as the standard
 * image [A ; cost], the structural basic variables enter in ascending variable id, each on the row partial pivoting chooses among the
 * rows whose auxiliary variable is nonbasic in the target and not yet pivoted (ties: the smallest row), as ordinary pending pivots, KP
 * per pass of the tableau-update kernel, the cost row carried by the same pivots, and a refresh pass recomputes the basic values and the
 * objective; nonbasic position j ends holding structural j or the auxiliary variable that left when structural j entered.  The revised
 * form writes heads, statuses and values and runs the replay of bslv_lpq_refactor; the slot's age is 0.  Either way the reduced costs
 * are those of the ENGINE'S OWN cost vector, no atomics enter the arithmetic and every reduction has a fixed order: the result is a
 * function of (vstat, model, bounds).  The slot is then a valid `src`.
 * FEASIBILITY IS NOT CHECKED: that is the caller's business.  A later solve_batch from such a slot first re-seats every nonbasic variable
 * against the bounds of ITS call, as from any parent.  Then under BSLV_LP_METHOD_DUAL a basis that is not dual feasible comes back
 * BSLV_LP_UNDEFINED (primal infeasibility is what the dual simplex removes); under PRIMAL a phase 1 removes primal infeasibility and
 * primal steps the dual one; under REPAIR the dual simplex runs where it can start and the primal start takes the rest.  A basis that is
 * optimal for the call's bounds comes back OPTIMAL with 0 iterations.
 * BSLV_E_ARG, with nothing changed: a status code outside 1..5; a count of BASIC other than M; LOWER / UPPER naming an infinite bound (a
 * free variable has none to name); FREE on a variable with a finite bound of the model's own; FIXED on a variable whose bounds differ; a
 * slot out of range or named twice; n < 0; only one of vlo / vup.  A SINGULAR basis is not an error of the call: by the test of
 * bslv_lpq_refactor -- a pivot with |v_r| <= 1e-9 (1 + max |v|) -- status_out[b] (may be NULL) = BSLV_LP_UNDEFINED, that slot is reset as by
 * bslv_lpq_reset_slot and the other slots of the call are unaffected; 0 otherwise.  A call while slots of the last batch still wait for
 * their tableau (bslv_lpq_set_lazy) gives all of them their tableau first, as a solve does; a parked record of a named slot is dropped,
 * one that reads a named slot as its parent makes its pass first.
 * bslv_lpq_rebuild is load_basis with the slot's own basis: every variable keeps its nonbasic status and value, the tableau, the reduced
 * costs (the engine's own cost vector: see bslv_lpq_refactor for slots of an objective batch) and the basic values are rebuilt from the
 * model.  A slot whose pass is parked or pending is materialised first, by bslv_lpq_materialise.  In the revised form it IS
 * bslv_lpq_refactor: same code path, same result bit for bit.  bslv_lpq_refactor, _set_refactor and _set_refactor_period keep refusing
 * the tableau form: no rebuild happens inside a solve there.
 * bslv_lpq_last_rebuild_stats, of the last load_basis / rebuild: [0] slots rebuilt, [1] replay pivots, [2] passes over a slot ((LP, pass)
 * pairs of the tableau-update kernel, the refresh pass included), [3] slots that failed (singular).
 * BSLV_LP_BASIS_TIMING=1 (tableau form): one line per call on stderr with the HIP-event time of the replay, of its passes and of the
 * refresh pass alone -- a plain pass of the tableau-update kernel over the same slots, for comparison. */
enum { BSLV_LP_VS_BASIC = 1, BSLV_LP_VS_LOWER = 2, BSLV_LP_VS_UPPER = 3, BSLV_LP_VS_FREE = 4, BSLV_LP_VS_FIXED = 5 };
int  bslv_lpq_var_map(const bslv_lpq *h, int *own_of_given /* M_given + N */);
int  bslv_lpq_get_basis(bslv_lpq *h, int slot, int *vstat /* M + N, engine's own model */, int *row_of /* M + N or NULL */);
int  bslv_lpq_load_basis(bslv_lpq *h, int n, const int *slots, const int *vstat /* n * (M + N) */,
                         const double *vlo, const double *vup /* n * var_cnt, or both NULL: the model's bounds */, int *status_out /* n or NULL */);
int  bslv_lpq_rebuild(bslv_lpq *h, int n, const int *slots, int *status_out);
int  bslv_lpq_last_rebuild_stats(const bslv_lpq *h, long out[4]);
int  bslv_lpq_pool_slots(const bslv_lpq *h);
size_t bslv_lpq_slot_bytes(const bslv_lpq *h);
/* LAZY TABLEAUX.  The first pass of a solve writes the LP's tableau into its own slot -- the largest memory item of a batch, and
 * wasted where nobody uses the slot as a parent again (the reference keeps ONE basis and warm-starts from it, bslv_lp.c:170-173; here
 * only the LP of a vertex that yields a new cut becomes a parent).  After bslv_lpq_set_lazy(h, 1) an LP that is finished when its
 * pass would be due keeps its pending pivots; values, duals and objective are served from its vectors as always.  The caller then
 * names the slots it will start later LPs from: bslv_lpq_materialise gives those their tableau (the same pass), and
 * bslv_lpq_discard_pending drops the rest.  A slot that was not materialised must not be passed as `src`.  A solve_batch that finds
 * slots still open materialises all of them first.  bslv_lpq_lazy_stats: [0] LP passes skipped, [1] passes made on request
 * (those of parked slots included, when they are made), [2] host microseconds spent in bslv_lpq_materialise and bslv_lpq_park (totals).
 * PARKED PASSES.  Most slots a caller keeps never become a parent after all.  bslv_lpq_park(h, n, slots) takes the place of
 * bslv_lpq_materialise for slots that MAY be used as `src` later: what the pass of such a slot needs (its pending pivots and its
 * reduced-cost row, ~2 % of a slot) is copied to a store beside the pool, without a pass and without a host wait, and the slot may
 * be used like a materialised one.  The engine makes the pass by itself -- same arithmetic, same result bit for bit -- at the start
 * of the solve_batch / solve_batch_obj that names the slot as `src`, in bslv_lpq_materialise, and, where the pass still reads the
 * slot's own parent, before that parent is overwritten (as `dst` of a batch, by bslv_lpq_reset_slot).  A parked slot that is itself
 * overwritten loses its record; bslv_lpq_drop_parked tells the engine which slots the caller will never read again.  The getters
 * answer for a parked slot what they answer after bslv_lpq_materialise.  The pass of a parked slot counts in lazy_stats[1] and in
 * the statistics of the batch it precedes (bslv_lpq_last_passes / _last_launches, update_ms).  bslv_lpq_set_park(h, 0) (or
 * BSLV_LP_PARK=0 at create) makes bslv_lpq_park materialise at once, as it does in the revised form and where the store does not
 * fit; switching off gives every parked slot its tableau.  bslv_lpq_park_stats: [0] slots parked, [1] passes made for a child (or
 * on request), [2] passes made because the parent was about to be overwritten, [3] records dropped unused, [4] records live now. */
int  bslv_lpq_set_lazy(bslv_lpq *h, int on);
int  bslv_lpq_materialise(bslv_lpq *h, int n, const int *slots);
int  bslv_lpq_discard_pending(bslv_lpq *h);
int  bslv_lpq_lazy_stats(const bslv_lpq *h, long out[3]);
int  bslv_lpq_park(bslv_lpq *h, int n, const int *slots);
int  bslv_lpq_drop_parked(bslv_lpq *h, int n, const int *slots);
int  bslv_lpq_park_stats(const bslv_lpq *h, long out[5]);
int  bslv_lpq_set_park(bslv_lpq *h, int on);
int  bslv_lpq_get_park(const bslv_lpq *h);
/* replace the shared bounds (lp_set_rows / lp_set_cols, bslv_lp.c:112-134) */
int  bslv_lpq_set_bounds(bslv_lpq *h, const double *lb, const double *ub);
/* put the standard basis (all aux basic; glp_std_basis, bslv_lp.c:101,225) into a slot */
int  bslv_lpq_reset_slot(bslv_lpq *h, int slot);
/* Solve B LPs.  LP b starts from slot src[b], works in slot dst[b] (src==dst allowed: in place),
 * with bounds vlo/vup[b*var_cnt + j] on variable var_first+j.  status[b] gets BSLV_LP_*,
 * iters[b] the number of dual-simplex pivots.  Any of status/iters may be NULL. */
int  bslv_lpq_solve_batch(bslv_lpq *h, int B, const int *src, const int *dst,
                          const double *vlo, const double *vup, int *status, int *iters);
/* solve_batch under `method` (BSLV_LP_METHOD_DUAL / _PRIMAL / _REPAIR, see bslv_lpq_set_method) for THIS call only; the engine's own
 * method (bslv_lpq_set_method) is neither read nor changed.  Both forms.  What a retry or a re-solve for a ray wants: another method
 * for one call, not for the engine.
 *   Tableau form  the call IS set_method(method); solve_batch(..); set_method(old), bit for bit: statuses, iters, slots, getters and
 *                 every last_* statistic.
 *   Revised form  DUAL is solve_batch bit for bit.  PRIMAL and REPAIR mean what bslv_lpq_set_method says of them: the start of
 *                 primal_start_status, phase 1 by the sum of infeasibilities with the Harris test of oracle/lp_dense.c primal_simplex,
 *                 then primal steps on the true reduced costs; they imply the extended selection.  This call is the only way to them
 *                 there: set_method and BSLV_LP_METHOD stay what they were.  The phase-1 pricing vector of a slot that holds B^-1 is the
 *                 tableau row of a synthesised rho, y1 = sum of +-(row i of B^-1) over the infeasible rows, rebuilt when the tableau
 *                 form rebuilds its own (last_phase1_stats[2]) and after a periodic refactorisation of an LP in phase 1.  Such a batch
 *                 runs the kernel instance of the DEFAULT pricing rule (k_select_p1_rev) whatever the two pricing switches say; Devex
 *                 pricing reaches it per call, bslv_lpq_solve_batch_method_priced below.
 * method outside 0..2, or h == NULL: BSLV_E_ARG, nothing changed.  bslv_lpq_last_phase1_stats, last_stats, last_ext_stats, last_passes,
 * last_period_stats and the ages cover the call as they cover a solve_batch; the in-call rescue (bslv_lpq_set_refactor) re-solves under
 * the call's method. */
int  bslv_lpq_solve_batch_method(bslv_lpq *h, int method, int B, const int *src, const int *dst,
                                 const double *vlo, const double *vup, int *status, int *iters);
/* ... under `method` AND under the two pricing rules of THIS call: dual_rule for the dual simplex steps, primal_rule for the primal ones
 * (BSLV_LP_PRICING_DANTZIG / _DEVEX, with the meaning documented at bslv_lpq_set_pricing and bslv_lpq_set_primal_pricing).  The engine's
 * method and its two pricing switches are neither read nor changed: the getters answer what they did and a later solve runs as if the call
 * had not been made.
 *   Tableau form  the call IS set_pricing(dual_rule); set_primal_pricing(primal_rule); solve_batch_method(method, ..); <both old switches
 *                 back>, bit for bit: statuses, iters, slots, getters, every last_* statistic and both norm read-outs.
 *   Revised form  DUAL is set_pricing(dual_rule); solve_batch(..); <the old switch back>, bit for bit (the primal rule does not reach a
 *                 DUAL batch, in either form).  PRIMAL and REPAIR: this call is the only way to Devex pricing for such a batch there
 *                 (k_select_priced_p1_rev<RULE>).  Which rule runs is decided as in the tableau form: dual_rule DEVEX runs the dual-Devex
 *                 instance and the primal counters read 0 (no instance carries both rules); otherwise primal_rule DEVEX runs the
 *                 primal-Devex instance; both DANTZIG is bslv_lpq_solve_batch_method, bit for bit.  New reference frameworks start where
 *                 the two rules say: under the primal rule with a dual pivot of the LP, under the dual rule with a primal or phase-1
 *                 pivot, under both with a refactorisation replay (the in-call rescue's re-solve, the resume after a periodic
 *                 refactorisation).  Phase 1 weights its own pricing vector by the same norms; nothing is reset when it ends.
 * A method or a rule out of range, or h == NULL: BSLV_E_ARG, nothing changed.  bslv_lpq_last_pricing_stats, _last_primal_pricing_stats and
 * both _norms read-outs answer for this call as for a batch under the switches; last_phase1_stats, last_stats, last_period_stats and the
 * ages cover it; the in-call rescue (bslv_lpq_set_refactor) re-solves under the call's method AND the call's rules. */
int  bslv_lpq_solve_batch_method_priced(bslv_lpq *h, int method, int dual_rule, int primal_rule, int B, const int *src, const int *dst,
                                        const double *vlo, const double *vup, int *status, int *iters);
/* The LPs of the batch differ in their OBJECTIVE (lp_set_obj_coeffs + lp_solve, bslv_lp.c:141-151, 219-259, as phase2_dual
 * drives them, bslv_algs.c:1469-1477): cost costs[b*cost_cnt + t] on variable cost_first + t, zero elsewhere (the engine must
 * have been created with a zero cost vector).  LP b starts from the basis of slot src[b], which has to be primal feasible
 * (any solved slot is: the bounds do not change) and runs primal simplex steps.  vlo/vup as in solve_batch.  Works in both forms
 * (tableau and revised); src[b] == dst[b] solves in place.  In the revised form an LP can come back BSLV_LP_UNDEFINED (see above):
 * retry it from a slot known to be accurate.  BSLV_LP_OBJ_UNDEFINED=K:b (test hook, off by default) reports LP b of the K-th call
 * on an engine as UNDEFINED and changes nothing else. */
int  bslv_lpq_solve_batch_obj(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                              int cost_first, int cost_cnt, const double *costs, int *status, int *iters);
/* getters for solved slots: out[b*cnt + j] = value for variable first+j of slot[b]
 * (lp_primal_solution_rows/cols, lp_dual_solution_rows/cols, lp_obj_val: bslv_lp.c:261-308) */
int  bslv_lpq_get_primal(bslv_lpq *h, int B, const int *slot, int first, int cnt, double *out);
int  bslv_lpq_get_dual(bslv_lpq *h, int B, const int *slot, int first, int cnt, double *out);
int  bslv_lpq_get_obj(bslv_lpq *h, int B, const int *slot, double *out);
/* CERTIFICATE of solved slots.  Read-only: no slot, vector, age, parked record, counter or statistic changes, and the next
 * solve behaves bit for bit as without the call.  It computes on the device, from the model and the vectors the getters above would
 * return -- nothing else of a slot is read -- the worst residual of each of five kinds, for LPs that came back BSLV_LP_OPTIMAL:
 * with p / y the primal / dual vector over all M + N variables of the model AS GIVEN (folded rows, parked and lazily open slots
 * included), r = p[:M], x = p[M:], lambda = y[:M], d = y[M:], lo / up the bounds given to create / set_bounds with the per-LP range
 * replaced by vlo[b] / vup[b] (the engine's artificial bounds play no part), and c the engine's own cost or, with cost_cnt > 0, zero
 * everywhere except costs[b] on cost_first .. (rows may carry a cost there, as in bslv_lpq_solve_batch_obj: a cost c_i on row i is the
 * column cost a_ij c_i, so c_j stands for c_j + sum_i a_ij c_i below; a range over folded rows is BSLV_E_ARG as it is there):
 *   res[b*5 + 0]  rows   max_i |r_i - sum_j a_ij x_j|
 *   res[b*5 + 1]  feas   max_k of (lo_k - p_k) / (1 + |lo_k|) and (p_k - up_k) / (1 + |up_k|) over the finite bounds, not below 0
 *   res[b*5 + 2]  dj     max_j |d_j - (c_j - sum_i a_ij lambda_i)|
 *   res[b*5 + 3]  side   over the k with |y_k| > tol[5]: |p_k - the bound of y_k's sign| (y > 0: lower, y < 0: upper); +inf if that
 *                        bound is infinite
 *   res[b*5 + 4]  gap    max(|D - P|, |P - z|), P = c0 + c . x, D = c0 + sum_k y_k (the bound of y_k's sign) over the k whose bound is
 *                        finite, z = what bslv_lpq_get_obj returns for the slot and c0 = the engine's constant shift cost[0] -- for a
 *                        slot of an objective batch too: there get_obj is the batch's objective plus the same shift
 * Every sum is accumulated compensated (as accurate as in twice the working precision, rounded once) in a fixed order: the same call on
 * the same state returns the same bits.  at[b*5 + k] is the variable, in the model as given, where the worst residual of kind k was met
 * (ties: the smaller index; feas: the variable nearest to or furthest beyond a finite bound); -1 for gap and where nothing was examined.
 * verdict[b] is a bit mask: bit k is set when residual k of LP b is over its tolerance (or is not a number); 0 = certified.
 * tol: rows, feas, dj, side = 1e-9, 1e-8, 1e-8, 1e-7; tol[4] = 1e-9 is applied as tol[4] (1 + |z|); tol[5] = 1e-9 is the dual-zero
 * threshold of side.  tol == NULL or an entry <= 0: that default.
 * BSLV_E_ARG: h == NULL, B < 0, a slot out of range, vlo / vup missing with var_cnt > 0, res == NULL with B > 0, a cost range outside
 * the model.  B == 0 returns 0.  A slot may be named more than once, with different bounds.  Works in both forms and under every
 * method and switch.  The call waits for its stream.  Its scratch grows with the largest call and is released by bslv_lpq_destroy
 * (bslv_lpq_slot_bytes and the pool do not change); a call whose scratch would exceed 256 MiB runs its LPs in chunks.
 * BSLV_LP_CERTIFY_TIMING=1: one line per call on stderr with the time of each kernel (HIP events).
 * bslv_lpq_last_certify_stats, of the last call: [0] LPs examined, [1] LPs with a verdict other than 0, [2] kernel launches. */
int bslv_lpq_certify(bslv_lpq *h, int B, const int *slot,
                     const double *vlo, const double *vup,      /* B * var_cnt, as given to the solve; may be NULL when var_cnt == 0 */
                     int cost_first, int cost_cnt, const double *costs, /* an objective batch's (B * cost_cnt); cost_cnt == 0: the engine's own cost */
                     const double *tol,                         /* 6 doubles or NULL = the defaults above */
                     double *res,                               /* B * 5: rows, feas, dj, side, gap */
                     int *at,                                   /* B * 5, may be NULL */
                     int *verdict);                             /* B, may be NULL */
int bslv_lpq_last_certify_stats(const bslv_lpq *h, long out[3]);
/* for tests only: damage a slot by plain copies (no kernel).  what 0 adds delta to the stored value of variable var (basic or nonbasic,
 * wherever it lives), what 1 to the stored reduced cost of a NONBASIC variable (a basic one is BSLV_E_ARG).  var is an index of the
 * engine's own model: an engine with folded rows answers BSLV_E_ARG. */
int bslv_lpq_debug_poke(bslv_lpq *h, int slot, int what, int var, double delta);
/* RAYS: why an LP came back BSLV_LP_INFEASIBLE or BSLV_LP_UNBOUNDED.  Off unless asked for (bslv_lpq_set_rays(h, 1), or BSLV_LP_RAYS=1
 * in the environment when an engine is created; both forms); off, nothing is allocated, no kernel is launched and no result bit differs.
 * On, every slot has a kind and a vector of M + N doubles beside the pool (like the ages: bslv_lpq_slot_bytes is what it was),
 * allocated by set_rays(1), released by set_rays(0) and bslv_lpq_destroy.  A solve call (solve_batch, solve_batch_obj, the in-call
 * rescue's re-solve) sets the kind of every dst slot it was accepted for; bslv_lpq_reset_slot and a successful bslv_lpq_refactor set
 * NONE.  The kind is NONE unless the LP's final conclusion is one of three, in which the kernel holds the proof when it concludes
 * (x_B = T x_N, alpha = T; the concluding thread records row / column, side and where the vectors lie, the kernel k_ray builds the
 * vector once after the rounds of the call -- no selection kernel is kept out of the plan, each holds its vector at the conclusion):
 *   FARKAS, dual row    INFEASIBLE from the dual selection: row r, basic variable k = bh[r], has no entering candidate.  Below its
 *                       lower bound: z_k = 1, z_nh[j] = -alpha_rj for every nonbasic position j, 0 on the other basic variables; above
 *                       its upper bound: the negative of that.
 *   FARKAS, phase 1     INFEASIBLE from the primal phase 1 (methods PRIMAL / REPAIR): no column lowers the sum of infeasibilities.
 *                       z = sum_i sigma_i (e_bh[i] - sum_j alpha_ij e_nh[j]), sigma_i = +1 below the lower bound, -1 above the upper one.
 *   DIRECTION           UNBOUNDED from a primal step (objective batches, methods PRIMAL / REPAIR): entering position q moves by dir
 *                       = +-1 and no row blocks.  delta_nh[q] = dir, delta_bh[i] = alpha_iq dir, 0 elsewhere.
 * The stored vector is divided by its largest absolute entry (one division per entry; the divisor is a value, so ties need no rule).
 * A FARKAS vector z has z . (A x, x) = 0 for every x; with every entry's NEEDED bound (the lower one for z_k > 0, the upper one for
 * z_k < 0) finite and S = sum_k z_k (needed bound) > 0 no point of the box exists.  A conclusion that leaned on one of the engine's
 * ARTIFICIAL bounds shows as an entry whose needed bound, in the model as given, is infinite: no proof for that model.
 * TWO CONCLUSIONS STORE NOTHING (kind NONE, counted in last_ray_stats[2]):
 *   - UNBOUNDED on an active artificial bound (the dual method found no violated row while a nonbasic variable with a non-zero reduced
 *     cost sits on an artificial bound).  The engine never looked for a ray there, and a single column is in general not a ray.  A
 *     caller who needs the ray re-solves the LP under BSLV_LP_METHOD_PRIMAL (bslv_lpq_set_method; in the revised form, and for one
 *     call in either form, bslv_lpq_solve_batch_method).
 *   - the empty box a folded row left (solve_batch answers INFEASIBLE without touching a slot).
 * bslv_lpq_get_ray answers in the indices of the model AS GIVEN: kind[b] and, unless ray == NULL, ray[b * (M + N) ..] of slot[b] (zeros
 * for NONE).  With folded rows a column entry z_j whose needed bound came from folded row i (coefficient a_ij) moves to that row:
 * z_i = z_j / a_ij, z_j = 0 -- the rule of the duals; a DIRECTION has delta r_i = a_ij delta x_j there.
 * BSLV_E_STATE with the switch off, BSLV_E_ARG for a slot out of range or h == NULL; B == 0 returns 0; a slot may be named twice.
 * bslv_lpq_last_ray_stats, of the last solve call: [0] FARKAS rays stored, [1] DIRECTION rays stored, [2] INFEASIBLE / UNBOUNDED
 * conclusions without a ray.  BSLV_LP_RAY_TIMING=1: one line per solve call on stderr with the HIP-event time of k_ray. */
enum { BSLV_LP_RAY_NONE = 0, BSLV_LP_RAY_FARKAS = 1, BSLV_LP_RAY_DIRECTION = 2 };
int bslv_lpq_set_rays(bslv_lpq *h, int on);
int bslv_lpq_get_rays(const bslv_lpq *h);
int bslv_lpq_get_ray(bslv_lpq *h, int B, const int *slot, int *kind /* B */, double *ray /* B * (M + N), may be NULL */);
int bslv_lpq_last_ray_stats(const bslv_lpq *h, long out[3]);
/* CERTIFICATE of the stored rays.  Read-only like bslv_lpq_certify, same meaning of vlo / vup / costs: the bounds of the model as given
 * with the per-LP range replaced, the engine's artificial bounds play no part.  Per LP four residuals, with z / delta = what
 * bslv_lpq_get_ray returns for the slot:
 *   FARKAS     res[0] ident   max_j |z_{M+j} + sum_i a_ij z_i|
 *              res[1] open    the largest |z_k| whose needed bound is infinite (at[1] = k); entries with |z_k| <= tol[2] count as zero:
 *                             they are left out here and in the two sums
 *              res[2] margin  S = sum_k z_k (needed bound) over the other entries
 *              res[3]         sum_k |z_k (needed bound)|
 *   DIRECTION  res[0] rows    max_i |delta r_i - sum_j a_ij delta x_j|
 *              res[1] cross   max over k of -delta_k where lo_k is finite and of delta_k where up_k is finite, not below 0
 *              res[2] margin  -c . delta, c as in bslv_lpq_certify (a cost on a row counts as c_i delta r_i)
 *              res[3]         sum_k |c_k delta_k|
 * verdict: bit 0 = res[0] > tol[0] (FARKAS) or > tol[1] (DIRECTION); bit 1 = res[1] > tol[2]; bit 2 = not (res[2] > tol[3] (1 + res[3]));
 * bit 3 = the slot's kind is NONE (its res are NaN, its at -1); a residual that is not a number sets its bit (so NONE reads 15).
 * 0 = the LP is infeasible / unbounded in the model as given.  at[b*4 + 0] / [1]: where res[0] / res[1] was met (ties: the smaller
 * index; -1 where res[1] is 0), [2] = [3] = -1.  tol (4 doubles, or NULL; an entry <= 0: the default) = 1e-8, 1e-9, 1e-9, 1e-9: the dj,
 * rows, dual-zero and gap numbers of bslv_lpq_certify.  Every sum is compensated, in a fixed order: same state, same bits.
 * BSLV_E_STATE with the ray store off; BSLV_E_ARG as bslv_lpq_certify.  bslv_lpq_last_ray_certify_stats: [0] LPs examined, [1] LPs with a
 * verdict other than 0, [2] kernel launches. */
int bslv_lpq_certify_rays(bslv_lpq *h, int B, const int *slot, const double *vlo, const double *vup,
                          int cost_first, int cost_cnt, const double *costs, const double *tol /* 4 or NULL */,
                          double *res /* B * 4 */, int *at /* B * 4, may be NULL */, int *verdict /* B, may be NULL */);
int bslv_lpq_last_ray_certify_stats(const bslv_lpq *h, long out[3]);
/* statistics of the last solve_batch: lock-step iterations, tableau-update kernel launches,
 * and the HIP-event time (ms) spent in the tableau-update kernel */
/* when on, every tableau-update launch is bracketed by HIP events on the engine's stream */
int  bslv_lpq_set_profile(bslv_lpq *h, int on);
int  bslv_lpq_last_stats(const bslv_lpq *h, int *lockstep_iters, long *pivots, double *update_ms, double *total_ms);
/* lockstep_iters = rounds (each: up to KP selections on vectors + one pass of k_flush over the tableaux with pending pivots);
 * update_ms = time in k_flush (HIP events, with set_profile).  Tableau passes of the last batch, i.e. how many (LP, round)
 * pairs k_flush read and wrote: */
long bslv_lpq_last_passes(const bslv_lpq *h);
/* k_flush launches behind those passes: one per lock-step round, plus one per bslv_lpq_materialise that had something to do and
 * one per pass over parked slots made since the batch before
 * (what a kernel trace counts; update_ms / this = the average launch) */
long bslv_lpq_last_launches(const bslv_lpq *h);
/* extended selection of the last solve_batch (LPs with boxed variables): out[0] iterations in which boxed columns switched
 * bound (long-step ratio test), [1] cost perturbations switched on, [2] primal simplex steps, [3] perturbation removals
 * that left reduced costs of the wrong sign (what the bound switches / primal steps then repaired) */
int  bslv_lpq_last_ext_stats(const bslv_lpq *h, long out[4]);
/* of the iterations with bound switches (out[0] above): those whose switches were carried into beta by a vector update, i.e.
 * without a pass over the tableau (at most 48 switches in the iteration) */
long bslv_lpq_last_flip_updates(const bslv_lpq *h);
/* how the last solve_batch started its LPs: the number of (parent, range of children) chunks k_init_grouped ran on, 0 when k_init
 * ran (a new objective, rows of more than 2048 columns, BSLV_INIT_GROUP=0) */
long bslv_lpq_last_init_chunks(const bslv_lpq *h);
/* The extended selection (bound flipping where variables are boxed, cost perturbation against dual-degenerate stalling, primal
 * clean-up) is compiled in for LPs with a boxed variable and, by itself, for tableaux of 1 GiB and more (ex09 of the reference's
 * suite: the plain dual simplex stalls there until the iteration limit).  on != 0 switches it on for every later solve of this
 * engine; the callers' retry does that when an LP is still undefined after the restart from the standard basis
 * (bslv_lp.c:222-227 is the reference's two-stage retry).  Same optimal values, other pivots. */
int  bslv_lpq_set_extended(bslv_lpq *h, int on);
int  bslv_lpq_get_extended(const bslv_lpq *h);
/* THE SIMPLEX METHOD of every later solve_batch of this engine (the reference hands its choice to GLPK: lp_set_options,
 * bslv_lp.c:153-217 -- PRIMAL_SIMPLEX / DUAL_SIMPLEX / DUAL_PRIMAL_SIMPLEX become GLP_PRIMAL / GLP_DUAL / GLP_DUALP, and GLPK's
 * primal simplex has a phase 1 of its own).
 *   DUAL    the default, and the engine as it was: LP b needs a dual feasible start in slot src[b], else BSLV_LP_UNDEFINED.
 *   PRIMAL  LP b starts from the basis of src[b] as it stands: the nonbasic variables keep their side where the new bounds allow it,
 *           a dual infeasible start is not an error.  While a basic variable is outside its bounds the LP runs a primal PHASE 1
 *           (sum of infeasibilities, Dantzig pricing, Harris ratio test in which an infeasible basic variable blocks at the bound
 *           it violates: oracle/lp_dense.c primal_simplex), then primal simplex steps on the true reduced costs.  The only dual
 *           simplex steps are the ones that conclude a primal clean-up today (rounding left a bound violated).
 *   REPAIR  the dual simplex, except that an LP whose start is dual infeasible is started as under PRIMAL instead of coming back
 *           UNDEFINED (GLP_DUALP: "dual, and primal if it fails").
 * Both imply the extended selection (the primal steps live there).  Objective batches (solve_batch_obj) keep their own start -- primal
 * steps from the parent's basis -- whatever this method is; they take a method per call: bslv_lpq_solve_batch_obj_method, below.
 * Not for the revised form: there a method other than DUAL is BSLV_E_ARG here, and the engine-wide method stays DUAL.  The revised
 * form does have PRIMAL and REPAIR, per call: bslv_lpq_solve_batch_method, in both forms, solves one batch under a method of its own
 * and leaves this one alone.  (Still open: an engine-wide PRIMAL / REPAIR default for the revised form, here and through BSLV_LP_METHOD.
 * The callers above the engine carry a method of their own: bslv_benson_set_lp_method.)
 * BSLV_LP_METHOD=dual|primal|repair sets the method an engine is created with (ignored by an engine that comes up in the revised form).
 * bslv_lpq_last_phase1_stats, of the last solve_batch: [0] LPs that entered phase 1, [1] phase-1 iterations (pivots + bound
 * switches), [2] rebuilds of the phase-1 pricing vector from the tableau rows (it is otherwise updated with every pivot). */
enum { BSLV_LP_METHOD_DUAL = 0, BSLV_LP_METHOD_PRIMAL = 1, BSLV_LP_METHOD_REPAIR = 2 };
int  bslv_lpq_set_method(bslv_lpq *h, int method);
int  bslv_lpq_get_method(const bslv_lpq *h);
int  bslv_lpq_last_phase1_stats(const bslv_lpq *h, long out[3]);
/* THE PRICING RULE of the dual simplex steps of every later solve_batch of this engine: which violated basis row leaves.  (The
 * reference leaves it to GLPK's defaults, glp_init_smcp with only meth set, bslv_lp.c:153-217: projected steepest edge.)
 *   DANTZIG  the default, and the engine as it was: the row with the largest bound violation (oracle/lp_dense.c dual_simplex).
 *   DEVEX    dual Devex pricing (Forrest and Goldfarb): every basis row i of an LP has a reference norm s_i >= 1, all 1 in the
 *            reference framework -- the basis the solve starts from (solve_batch, the in-call rescue's re-solve, the re-start after a
 *            periodic refactorisation); the row with the largest violation / s_i leaves, ties as under DANTZIG.  A dual pivot on row r
 *            with the entering column's multipliers f_i = alpha_iq / alpha_rq leaves s_i = max(s_i, |f_i| s_r) (i != r) and
 *            s_r = max(s_r / |alpha_rq|, 1); the multipliers are the ones the delayed update forms anyway, no tableau entry is read for
 *            the norms.  Bound switches of the long-step ratio test change nothing; any other basis change (a primal clean-up step, a
 *            phase-1 step, a refactorisation replay) starts a new framework.  Bland's rule, once it holds, ignores the norms.
 * With all s_i = 1 the rule IS the default one, bit for bit: the first pivot of every solve, and every LP the default rule solves in at
 * most one pivot, are the same.  Otherwise: same statuses and optimal values, other pivots, possibly another optimal basis.
 * Both forms, every method, extended selection on or off, canonical duals on or off.  Objective batches (solve_batch_obj: primal steps
 * only), the tie phases of the canonical switches and the replay's own selection never read the norms.  With the switch on a batch
 * runs kernel instances of its own (k_select_priced<RULE_DVX, ..>) and the plan does NOT take k_select_cached, the register-resident
 * selection of narrow tableau-form batches; with it off nothing is allocated, nothing launched and no bit differs.  Any other rule is
 * BSLV_E_ARG.  BSLV_LP_PRICING=dantzig|devex sets the rule an engine is created with.
 * bslv_lpq_last_pricing_stats, of the last solve call: [0] dual selections made under the weighted rule, [1] of those, selections whose
 * row is not the row of the largest violation, [2] new reference frameworks after the start (one per primal or phase-1 pivot, one per
 * LP and refactorisation replay during the rounds).  All 0 with the switch off.
 * REVISED FORM, PRIMAL / REPAIR (bslv_lpq_solve_batch_method): the rule reaches such a batch only through
 * bslv_lpq_solve_batch_method_priced.  Under this switch it runs the instance of the default rule -- the bits of the switch off -- and
 * the counters read 0.
 * bslv_lpq_last_pricing_norms (for tests): s_0 .. s_(M-1) of LP b of the last batch, M rows of the engine's OWN model (the given rows
 * less bslv_lpq_rows_folded); BSLV_E_STATE if the last solve call did not run under DEVEX, BSLV_E_ARG for b outside the batch. */
enum { BSLV_LP_PRICING_DANTZIG = 0, BSLV_LP_PRICING_DEVEX = 1 };
int  bslv_lpq_set_pricing(bslv_lpq *h, int rule);
int  bslv_lpq_get_pricing(const bslv_lpq *h);
int  bslv_lpq_last_pricing_stats(const bslv_lpq *h, long out[3]);
int  bslv_lpq_last_pricing_norms(bslv_lpq *h, int b, double *s);
/* THE PRICING RULE of the PRIMAL simplex steps, the counterpart of the above: which eligible nonbasic column enters.  Primal steps are
 * the whole solve of an objective batch (solve_batch_obj: the P1(w) LPs of the dual Benson variant) and phase 1 with the primal phase 2
 * behind it of a batch under BSLV_LP_METHOD_PRIMAL / _REPAIR.  (The reference: GLPK's projected steepest edge, as above.)
 *   DANTZIG  the default, and the engine as it was: the column with the largest reduced-cost violation |d_j| beyond TOL_DJ.
 *   DEVEX    primal Devex pricing: every nonbasic column POSITION j of an LP has a reference norm t_j >= 1, all 1 in the reference
 *            framework -- the basis the solve starts from (solve_batch_obj, solve_batch under PRIMAL / REPAIR, the in-call rescue's
 *            re-solve, the re-start after a periodic refactorisation); among the columns eligible under DANTZIG the one with the largest
 *            |d_j| / t_j enters, ties as under DANTZIG.  Phase 1 weights its own pricing vector by the same norms, and nothing is reset
 *            when it ends: the norms do not depend on the cost.  A primal pivot (r, q) with the pivot row alpha_r leaves
 *            t_j = max(t_j, |alpha_rj / alpha_rq| t_q) (j != q) and, for position q, which now holds the leaving variable,
 *            t_q = max(t_q / |alpha_rq|, 1): one more pass over the pivot row the selection has fetched anyway, no further tableau entry
 *            is read.  A bound switch of the entering variable changes nothing; a dual simplex pivot of the LP and a refactorisation
 *            replay start a new framework (all t_j = 1).  Bland's rule, whenever it holds, ignores the norms.  The norms belong to the
 *            LP of the batch, not to its slot: children do not inherit them.
 * With all t_j = 1 the rule IS the default one, bit for bit: the first primal selection of every solve, and every LP of at most one
 * primal selection, are the same.  Otherwise: same statuses and optimal values, other pivots, possibly another optimal basis.
 * WHICH BATCHES run under the rule (kernel instances of their own: k_select_priced<RULE_PDV, ..>, in both forms):
 *   - objective batches whenever the primal rule is DEVEX, whatever the dual rule is;
 *   - PRIMAL / REPAIR batches when the primal rule is DEVEX and the dual rule (bslv_lpq_set_pricing) is DANTZIG.  With BOTH rules on
 *     such a batch keeps the dual-Devex instance: its primal steps are priced as before and the counters below read 0 -- no instance
 *     carries both rules;
 *   - DUAL-method batches never: their primal clean-up steps stay as they are;
 *   - PRIMAL / REPAIR batches of the REVISED form (bslv_lpq_solve_batch_method) never, under either switch: the rules reach them only
 *     through bslv_lpq_solve_batch_method_priced; under the switches the batch runs the instance of the default rule and both counter
 *     triples read 0.
 * The tie phases of the canonical switches and the replay's own selection never read or write the norms.  With the switch off nothing
 * is allocated, nothing launched and no bit differs.  Any other rule is BSLV_E_ARG; both forms accept the call.
 * BSLV_LP_PRIMAL_PRICING=dantzig|devex sets the rule an engine is created with (so the Benson and VLP drivers and bensolve_hip get it
 * without an option of their own).
 * In the REVISED form use it with bslv_lpq_set_refactor_period (or bslv_lpq_set_refactor): on long solves (ex09's P1(w): thousands of
 * pivots) the basis inverse drifts further along Devex's columns than along the default rule's, and without a refactorisation LPs came
 * back UNDEFINED, one UNBOUNDED, that are OPTIMAL under both rules with a period of 200 (profiles/lp_primal_pricing_pivots.txt).
 * bslv_lpq_last_primal_pricing_stats, of the last solve call: [0] primal selections priced under the weighted rule (phase 1 and 2,
 * pivots and bound switches; not those under Bland's rule), [1] of those, selections whose column is not the column of the largest
 * unweighted score, [2] new reference frameworks after the start (one per dual pivot of an LP, one per LP and refactorisation replay
 * during the rounds).  All 0 with the switch off.
 * bslv_lpq_last_primal_pricing_norms (for tests): the norms of LP b of the last batch BY VARIABLE of the engine's own model, M + N values,
 * rows first (the given rows less bslv_lpq_rows_folded), then columns: t for a nonbasic variable, 0 for a basic one.  BSLV_E_STATE if
 * the last solve call ran no weighted instance, BSLV_E_ARG for b outside the batch. */
int  bslv_lpq_set_primal_pricing(bslv_lpq *h, int rule);
int  bslv_lpq_get_primal_pricing(const bslv_lpq *h);
int  bslv_lpq_last_primal_pricing_stats(const bslv_lpq *h, long out[3]);
int  bslv_lpq_last_primal_pricing_norms(bslv_lpq *h, int b, double *t /* M + N */);
/* CANONICAL OPTIMAL DUALS.  Benson's cut is built from the dual solution of P2(v) (w = lp_dual_solution_rows, bslv_algs.c:1050).  Where
 * the optimum is primal degenerate -- y = v + z c on an edge or a vertex of the image -- every w of the normal cone at y is optimal and
 * the basis the pivoting ended in names one of them, which need not be a facet normal.  With on != 0 every later solve_batch ends in the
 * CANONICAL optimal basis instead: the one that stays optimal for the per-LP bounds vlo + t dir, vup + t dir (dir: var_cnt values, one
 * per variable of the per-LP range; infinite bounds stay infinite) for all small enough t > 0.  Status, objective and primal values are
 * those of t = 0, bit for bit; only the basis may differ, and with it bslv_lpq_get_dual (:1050).  No t is ever formed: an LP that ends
 * OPTIMAL goes on into a TIE PHASE -- dual simplex pivots of length zero among the rows that sit on a bound, chosen by the derivative
 * of the basic values with respect to t (lp_engine.hip, k_select_tie) -- when the rounds of its batch are over.  The phase keeps the
 * status OPTIMAL however it ends; its pivots are counted in iters[].  Works with every method and with the extended selection on or
 * off (it does not need it); objective batches (solve_batch_obj) ignore this switch -- theirs is bslv_lpq_set_canonical_obj, below, and
 * the two are independent; the revised form answers BSLV_E_ARG.  With on = 0
 * (dir may be NULL) the engine computes what it always did.
 * bslv_lpq_last_canonical_stats, of the last solve_batch: [0] LPs that entered the tie phase (all that ended OPTIMAL), [1] tie pivots,
 * [2] LPs whose phase ended without an entering candidate (the shifted LP is infeasible for t > 0), [3] LPs that gave up at the cap. */
int  bslv_lpq_set_canonical(bslv_lpq *h, int on, const double *dir /* var_cnt, NULL with on = 0 */);
int  bslv_lpq_get_canonical(const bslv_lpq *h);
int  bslv_lpq_last_canonical_stats(const bslv_lpq *h, long out[4]);
/* ... PER CALL, in both forms: one solve_batch under the engine's own method, followed by the tie phase towards the canonical basis for
 * dir, with the meaning documented at bslv_lpq_set_canonical, for THIS batch only.  The engine's own switch and its stored direction are
 * neither read nor changed (bslv_lpq_get_canonical answers what it did; a later solve_batch runs as if the call had not been made).  In
 * the tableau form the call is set_canonical(1, dir); solve_batch(..); <the old switch and direction back>, bit for bit.  In the
 * REVISED form, where bslv_lpq_set_canonical answers BSLV_E_ARG, this call is the way to the tie phase (lp_engine.hip,
 * k_select_tie_rev): g comes from one product with B^-1, the pivot row and the entering column from the sparse products of a
 * selection (helper workgroups included), and the pivot element is cross-checked between the two as in every selection of that form.
 * A tie pivot is a rank-1 step on B^-1 and counts in iters[] and in the slot's age (bslv_lpq_slot_age); no periodic refactorisation
 * runs inside the phase.  With bslv_lpq_set_refactor the rescue re-solves before the tie phase of the LPs it takes, as in any
 * solve_batch; only LPs that end OPTIMAL enter the phase.
 * h == NULL, dir == NULL with var_cnt > 0 or a non-finite dir[j]: BSLV_E_ARG, nothing changed.  var_cnt == 0: the call is solve_batch.
 * bslv_lpq_last_canonical_stats covers the call (the rescue's solves included); for this call [3] reads "gave up: at the cap, or
 * (revised form) on a drifted inverse" -- an LP whose cross-check fails commits nothing, keeps the optimal basis it had reached with
 * the status OPTIMAL and is not marked for the rescue: the optimum is already known. */
int  bslv_lpq_solve_batch_canonical(bslv_lpq *h, const double *dir /* var_cnt */, int B, const int *src, const int *dst,
                                    const double *vlo, const double *vup, int *status, int *iters);
/* CANONICAL OPTIMAL POINTS of objective batches.  The dual variant builds the cut of the lower image from the optimal point y = P x of
 * P1(w) (phase2_dual takes it from lp_primal_solution_cols, bslv_algs.c:1479-1486).  Where w is the normal of a face of the upper
 * image of dimension >= 1 the LP is dual degenerate: every y of that face is optimal and the pivoting ends in P x of whichever vertex x
 * of the feasible set it reached, which need not be a vertex of the image.  With on != 0 every later solve_batch_obj over the cost
 * range (cost_first, cost_cnt) ends in the CANONICAL optimal solution instead: the one that stays optimal for the costs c + t ddir
 * (ddir: cost_cnt values, one per variable of the cost range) for all small enough t > 0, i.e. the lexicographic minimum of
 * (c . x, ddir . x).  No t is ever formed: an LP that ends OPTIMAL goes on into a tie phase when the rounds of its batch are over --
 * primal simplex steps among the nonbasic columns whose reduced cost is zero (|d_j| <= 1e-9), chosen by g, the reduced-cost row of
 * ddir, which the engine keeps per LP and updates with every pivot (lp_engine.hip, k_select_tie_obj).  Unlike the steps of
 * bslv_lpq_set_canonical these have a length: x moves along the optimal face, the objective by at most 1e-9 x step.  The phase keeps
 * the status OPTIMAL however it ends -- no wrong tied column (canonical), an entering column without a blocking row (ddir . x is
 * unbounded on the optimal face: the basis reached stays), or the cap of 1000 + 2 (M + N) iterations; its iterations are counted in
 * iters[].  A solve_batch_obj with another cost range answers BSLV_E_ARG while the switch is on; solve_batch ignores the switch; it
 * is independent of bslv_lpq_set_canonical.  A non-finite ddir, a bad range or on with ddir == NULL is BSLV_E_ARG, and so is on for an
 * engine in the revised form (there the phase is reached per call: bslv_lpq_solve_batch_obj_canonical, below).  With on = 0 the engine computes what it always did, bit
 * for bit.
 * bslv_lpq_last_canonical_obj_stats, of the last solve_batch_obj: [0] LPs that entered the phase (all that ended OPTIMAL), [1] tie
 * iterations (pivots + bound switches), [2] LPs that ended on a column without a blocking row, [3] LPs that gave up at the cap; all
 * zero after a batch with the switch off. */
int  bslv_lpq_set_canonical_obj(bslv_lpq *h, int on, int cost_first, int cost_cnt, const double *ddir /* cost_cnt; NULL with on = 0 */);
int  bslv_lpq_get_canonical_obj(const bslv_lpq *h);
int  bslv_lpq_last_canonical_obj_stats(const bslv_lpq *h, long out[4]);
/* ... PER CALL, in both forms: one solve_batch_obj, followed by the tie phase towards the canonical optimal point for ddir on the cost
 * range of the call, with the meaning documented at bslv_lpq_set_canonical_obj, for THIS batch only.  The engine's own switch, its cost
 * range and its stored direction are neither read nor changed (bslv_lpq_get_canonical_obj answers what it did; a later solve_batch_obj
 * runs as if the call had not been made), and the call takes its own range: solve_batch_obj's refusal of a range other than the
 * switch's does not apply to it.  In the tableau form the call is set_canonical_obj(1, cost_first, cost_cnt, ddir);
 * solve_batch_obj(..); <the old switch, range and direction back>, bit for bit.  In the REVISED form, where
 * bslv_lpq_set_canonical_obj answers BSLV_E_ARG, this call is the way to the phase (lp_engine.hip, k_select_tie_obj_rev): a slot holds
 * B^-1 and T[r][j] = -rho_r . K[nh_j], so g on entry is one tableau row, the one of the synthesised y = sum_t ddir_t rho_pos(cost_first + t)
 * over the basic variables of the range, g_j = ddir_{nh[j]} - y . K[nh_j], through the sparse products of a selection (helper workgroups
 * included); the entering column and the pivot row come from those products too, and the pivot element is cross-checked between the
 * two as in every selection of that form (a bound switch fetches no row and has no check).  A tie pivot is a rank-1 step on B^-1 and
 * counts in iters[] and in the slot's age (bslv_lpq_slot_age); no periodic refactorisation runs inside the phase, and neither Devex
 * switch reaches it.  With bslv_lpq_set_refactor the rescue re-solves before the tie phase of the LPs it takes, as in any
 * solve_batch_obj; only LPs that end OPTIMAL enter the phase.
 * h == NULL, ddir == NULL, a non-finite ddir[t] or a bad range: BSLV_E_ARG, nothing changed; whatever solve_batch_obj refuses stays
 * refused with its own code.  bslv_lpq_last_canonical_obj_stats covers the call (the rescue's solves included); for this call [3]
 * reads "gave up: at the cap, or (revised form) on a drifted inverse" -- an LP whose cross-check fails commits nothing, keeps the
 * optimal basis it had reached (every step of the phase keeps optimality) with the status OPTIMAL and is not marked for the rescue. */
int  bslv_lpq_solve_batch_obj_canonical(bslv_lpq *h, const double *ddir /* cost_cnt */, int B, const int *src, const int *dst,
                                        const double *vlo, const double *vup, int cost_first, int cost_cnt, const double *costs,
                                        int *status, int *iters);
/* AN OBJECTIVE BATCH UNDER A METHOD, per call and in both forms (the reference runs the P1(w) LPs of -a dual / -A dual under whatever
 * -l / -L asks for: lp_set_options, bslv_lp.c:153-217).  The engine's own method (bslv_lpq_set_method) is neither read nor changed.
 *   PRIMAL  bslv_lpq_solve_batch_obj, bit for bit: statuses, iters, slots, getters and every last_* record.
 *   DUAL    the basis of src[b] is made dual feasible for the NEW objective and the LP runs dual simplex steps.  The new reduced-cost
 *           row d is built as for solve_batch_obj (tableau form: k_prep's sum over the parent's tableau rows; revised form: k_rev_price,
 *           one tableau row of y = sum c_t rho_t -- the dense row stays on the device).  Every nonbasic variable then takes the side d_j
 *           wants where it has a bound there: the lower one for d_j > 1e-9, the upper one for d_j < -1e-9; otherwise it keeps the side
 *           solve_batch_obj gives it (the parent's, sanitised against the bounds).  This is the rule of a DUAL solve_batch fed the new
 *           d_j.  beta is formed from the nonbasic values so chosen, by the kernels that form it in every solve (k_init; revised form:
 *           k_rev_u, k_init); the order of the start is k_prep, (revised form: k_rev_price,) k_obj_art, k_obj_start, (k_rev_u,) k_init
 *           in both forms: in the revised form the row exists only after k_prep.
 *           The LP then runs the selection of a DUAL solve_batch with the extended selection on (an objective batch always has it) --
 *           bound flipping, cost perturbation, primal clean-up, Bland fallback as there -- under the dual Devex instance where
 *           bslv_lpq_set_pricing is DEVEX; the primal Devex switch does not reach a DUAL call.
 *           ARTIFICIAL BOUNDS.  An engine that solves objective batches has a zero cost vector and so no artificial bounds of its own.
 *           The call makes its own by the engine's rule, applied to the reduced costs it starts from (oracle/lp_dense.c olp_solve, the
 *           "artificial-bounds start of the dual simplex"): a nonbasic variable outside the per-LP range whose d_j in SOME LP of the
 *           batch points where it has no bound (d_j > 1e-9 without a lower, d_j < -1e-9 without an upper bound) has -+1e7 there for
 *           every LP of the batch, for this call only.  They count as bounds exactly as the engine's own do in solve_batch: a variable
 *           starts on one where its d_j wants it, and an LP that ends with a non-zero reduced cost on one comes back BSLV_LP_UNBOUNDED
 *           -- it is unbounded in the direction the PRIMAL path reports as a ray; with bslv_lpq_set_rays this conclusion stores NO ray
 *           (kind NONE, counted in last_ray_stats[2]), as for solve_batch: re-solve under PRIMAL for the DIRECTION.  THE POLISH: a variable put on an
 *           artificial bound that never enters the basis -- a free column ends with d_j = 0 wherever it stands -- would stay 1e7 away
 *           on the optimal face, and values of that size leave 1e-8 .. 1e-5 in the rows.  So every LP that started on an artificial
 *           bound and ended OPTIMAL is solved once more in its own slot as the PRIMAL objective batch it would have been, under the
 *           engine's own bounds, inside the same call (0 .. 7 iterations measured): what comes back is a basis and a point of the LP as
 *           given.  These iterations count in iters[] and in every last_* record of the call.  Nothing guarantees that the
 *           basis the dual steps reached is primal feasible once the variables are back on their natural sides; the primal steps mend
 *           what rounding left, and a polish that does not end OPTIMAL makes the LP BSLV_LP_UNDEFINED (never OPTIMAL, never the
 *           polish's own verdict).  The artificial bounds are the BATCH's, not the LP's: a variable one
 *           LP needs bounded is bounded at -+1e7 for every LP of the call.  An LP that does not need it never STARTS on it (no natural
 *           side is an artificial bound), but it sees the variable as bounded -- in the ratio tests, and a basic variable could in
 *           principle leave towards it -- so what an LP computes may depend on the other LPs of its batch; only a PRIMAL call keeps
 *           "an LP of a batch is that LP alone" bit for bit.
 *           An LP with a nonbasic variable that no side makes dual feasible -- a variable of the per-LP range (its bounds come per LP,
 *           it gets no artificial one) that is free with |d_j| > 1e-7 or bounded on the wrong side only -- comes back BSLV_LP_UNDEFINED
 *           with 0 iterations and leaves slot dst[b] unusable, as a solve_batch with a dual infeasible start does.
 *   REPAIR  DUAL, except that an LP whose start cannot be made dual feasible takes the start of PRIMAL instead of coming back UNDEFINED
 *           (primal steps from the parent's basis, which must be primal feasible as for solve_batch_obj).  Decided per LP, inside one
 *           call.  Pricing: the dual Devex instance where that switch is on, else the primal Devex instance where that one is.
 * method outside 0..2 or h == NULL: BSLV_E_ARG, nothing changed; whatever solve_batch_obj refuses stays refused with its own code.  The
 * in-call rescue (bslv_lpq_set_refactor) re-solves under the call's method.  The tie phase of objective batches follows a PRIMAL solve
 * only: with bslv_lpq_set_canonical_obj on, DUAL and REPAIR are BSLV_E_ARG; bslv_lpq_solve_batch_obj_canonical keeps its signature and
 * its PRIMAL solve.
 * bslv_lpq_last_obj_method_stats, of the last solve call: [0] LPs that started dual, [1] nonbasic variables moved off the side
 * solve_batch_obj would have given them at the start, [2] LPs REPAIR handed to the primal start, [3] dual pivots (all iterations less
 * the primal ones).  All zero after any other call and after a PRIMAL one. */
int  bslv_lpq_solve_batch_obj_method(bslv_lpq *h, int method, int B, const int *src, const int *dst,
                                     const double *vlo, const double *vup,
                                     int cost_first, int cost_cnt, const double *costs, int *status, int *iters);
int  bslv_lpq_last_obj_method_stats(const bslv_lpq *h, long out[4]);

/* ------------------------------------------------------------------------------------------
 * 2. Polyhedron engine  (replaces bslv_poly.h:90-118)
 *
 * Same object as the reference's poly_args: a primal polyhedron (points + directions) and its
 * dual (one dual vertex per halfspace); `val`/`ideal` arguments are what the reference passes in
 * poly_args.val / poly_args.ideal.  v2h selects the dualV2primalH callback (a function pointer
 * without context in the reference, bslv_poly.h:79-80):
 *   0 cone_polar (bslv_poly.c:30-39)  1 lowerV2upperH (bslv_algs.c:287-305, parameter c)
 *   2 upperV2lowerH (bslv_algs.c:307-313, parameter c)
 * rc_out follows the reference's EXIT_SUCCESS(0) / EXIT_FAILURE(1) convention.
 * ------------------------------------------------------------------------------------------ */
typedef struct bslv_poly bslv_poly;

int  bslv_poly_create(bslv_poly **out, int dim, int v2h, const double *c /* dim, may be NULL */);
                                                              /* poly__set_default_args + poly__initialise :41-102 */
void bslv_poly_destroy(bslv_poly *h);                         /* poly__kill :258 */
int  bslv_poly_dual0_apex(bslv_poly *h);                      /* cone_vertenum's tweak, bslv_algs.c:338-339 */
int  bslv_poly_add(bslv_poly *h, const double *val, int ideal, int *rc_out);       /* poly__add_vrtx :104 */
int  bslv_poly_add_cuts(bslv_poly *h, int B, const double *val /* B*dim */, const int *ideal /* may be NULL */,
                        int *rc_out /* B */);                 /* batched poly__add_vrtx */
/* add_cuts strategy: 0 = one cut at a time (slot numbering identical to the sequential definition),
 * 1 = rounds of independent cuts applied in one pass each (default; same sets, different slot numbers) */
int  bslv_poly_set_batch_mode(bslv_poly *h, int mode);
long bslv_poly_rounds_run(const bslv_poly *h);
/* which paths of the single-cut pipeline ran (tests, tuning): out[0] chunks in hot mode, [1] cuts whose round B was
 * queued speculatively, [2] of those declined by the device and rerun, [3] prunes redone by the multi-kernel path,
 * [4] cuts applied one at a time, [5] multi-kernel prunes that confirmed their edges through facet-major member lists */
int  bslv_poly_path_stats(const bslv_poly *h, long out[6]);
/* multi-GPU (4a): adjacency prunes whose pair space was dealt to the ranks (facets of at least 32768 elements; bslv_poly_debug_set
 * key 10 changes the threshold): every rank tests a contiguous share of the rows, the adjacent pairs found are all-gathered and
 * appended in rank order, which is the order a single GPU writes them in */
long bslv_poly_sharded_prunes(const bslv_poly *h);
/* the projection sub-band of poly__cut (bslv_poly.c:666-674): with on = 1 an element that lies between 1e-2 POLY_EPS and POLY_EPS above a cut
 * that removes something is moved onto the hyperplane before it is treated as lying on it, exactly as the reference does, and cuts are applied
 * one at a time in the order handed in (the rounds of independent cuts classify ahead and stay off).  Default 0: such an element keeps its
 * coordinates (same index sets, coordinates within 1e-9: tests/test_oracle_poly.py::test_snap_band_*).  Also BSLV_POLY_SNAP=1. */
int  bslv_poly_set_snap(bslv_poly *h, int on);
int  bslv_poly_snapped(bslv_poly *h, long *moved);        /* elements moved so far */
int  bslv_poly_largest_facet(const bslv_poly *h);     /* members of the largest new facet that went through the multi-kernel prune */
long bslv_poly_noflag_prunes(const bslv_poly *h);      /* large-facet prunes that kept no flag byte per pair (k_pair_retest_emit) */
/* The multi-kernel prune of a large new facet (row-tiled pair kernel) walks the pair space in WINDOWS: contiguous ranges of row groups
 * (8 rows each), each tested, scanned and emitted before the next one starts.  A pair block is one row i with 256 columns j > i; block
 * ids are 64-bit on the host and 32-bit relative to the window on the device, and the scratch arrays (16 B per block) are sized by the
 * largest window, so a facet of any number of pair blocks is pruned.  The edge list is the one a single pass writes, bit for bit.
 * bslv_poly_set_prune_window: blocks > 0 = the most pair blocks a window may hold (values above the default are taken as the default;
 * a single row group larger than `blocks` still forms a window), 0 = the default, 0x7FFFFFF0: every facet below 2^31 blocks (about
 * 1.05 M members) runs in one window, exactly as without windows.  blocks < 0 is BSLV_E_ARG and changes nothing.  Also
 * BSLV_K2_WINDOW=blocks, read when a polyhedron engine is created (also those bslv_benson_create* and bslv_vlp_solve_* create): the
 * knob for a card with less free memory than 16 B x 2^31.  The one-dimensional pair launches, the sorted-list path and a prune whose
 * pair space is dealt to the ranks ignore the window and keep their 32-bit caps (BSLV_E_CAPACITY).
 * bslv_poly_prune_window_stats: out[0] prunes that ran in more than one window, [1] the windows of those prunes in total, [2] the
 * largest number of pair blocks any window held (one-window prunes of the tiled path included). */
int  bslv_poly_set_prune_window(bslv_poly *h, long blocks);
long bslv_poly_get_prune_window(const bslv_poly *h);
int  bslv_poly_prune_window_stats(const bslv_poly *h, long out[3]);
/* cuts that were still untouched when a chunk's rounds ended on "no cut alive" and were handed to the one-cut pipeline instead
 * (0 in every run but one of round 2's test runs; kept as a counter so that it cannot hide) */
long bslv_poly_rounds2_late_left(const bslv_poly *h);
/* reads of a round's mailbox (mapped pinned memory, four cache lines) whose sequence number had arrived before the rest of the
 * state: detected by the checksum the state carries and repeated */
long bslv_poly_rounds2_torn_reads(const bslv_poly *h);
/* test hook, same switches as the BSLV_* environment variables but at run time: key 0 dynamic LDS bytes of the one-workgroup
 * prune (64 forces the multi-kernel prune), 1 speculative launch on/off, 2 hot mode on/off, 3 CROSS_UB, 4 size of a new facet
 * from which the multi-kernel prune builds facet-major member lists (default 4096), 5 member lists on/off, 6 device-selected
 * rounds of independent cuts inside a hot chunk on/off, 7 cuts per chunk (32..4096, default 512); keys 8, 10-12, 14, 16 and 18-26:
 * bslv_poly_debug_set in poly_engine.hip; any other key is BSLV_E_ARG */
/* bslv_poly_add_cuts may hand cuts BACK (rc 2: not applied, dual slot left unused) when the rounds of a chunk get thinner than
 * min_cuts cuts -- the tail of a chunk is its cliques, one cut each per pass over the polyhedron; the caller hands the same
 * halfspaces in again with its next batch (phase2_primal has no counterpart: bslv_algs.c:1041-1080 applies one cut per LP).
 * 0 (default): every cut handed in is applied or found redundant, as poly__add_vrtx does (bslv_poly.c:104-151). */
int  bslv_poly_set_defer(bslv_poly *h, int min_cuts);
int  bslv_poly_debug_set(bslv_poly *h, int key, long value);
/* rounds of independent cuts chosen and applied on the device inside a hot chunk (debug_set key 6 switches them off, key 7 sets
 * the number of cuts classified and applied together): out[0] rounds, [1] cuts applied in them, [2] chunks, [3] prunes that took
 * the multi-kernel path, [4] rounds taken back for want of capacity */
int  bslv_poly_rounds2_stats(const bslv_poly *h, long out[5]);
/* rounds: prunes of a round that were worked in parts by several workgroups of the launch (debug_set keys 23-26; BSLV_R2_SPLIT,
 * _MIN, _PARTS, _H): out[0] prunes that were split, [1] helper workgroups that took a part of one */
int  bslv_poly_split_stats(bslv_poly *h, long out[2]);
int  bslv_poly_init(bslv_poly *h, int *rc_out);               /* poly__intl_apprx :153 */
int  bslv_poly_next(bslv_poly *h, double *val, int *ideal, int *idx, int *rc_out); /* poly__get_vrtx :210 */
int  bslv_poly_unprocessed(bslv_poly *h, int max_out, int *idx, double *val, int *ideal, int *count);
int  bslv_poly_unprocessed2(bslv_poly *h, int max_out, int from_end, int *idx, double *val, int *ideal, int *parent, int *count);
/* families: counts[k] = unprocessed elements whose parent (the newest facet through them) is dual slot first_facet + k; the
 * unprocessed children of a list of facets (at most max_out, the newest slots, ascending; parent[] = dual slots) */
int  bslv_poly_children_hist(bslv_poly *h, int first_facet, int n, int *counts, int *total, int *older);
int  bslv_poly_children_of(bslv_poly *h, int nfacets, const int *facets, int max_out, int *idx, double *val, int *ideal, int *parent, int *n_out);
int  bslv_poly_mark(bslv_poly *h, int n, const int *idx);     /* ST_BT(primal.sltn, idx) */
int  bslv_poly_dual_adjacency(bslv_poly *h);                  /* poly__update_adjacence(&dual) :992 */
/* batched incidence kernel on the current elements: hps = B x (dim+1) halfspaces (normal, alpha);
 * words_out: ceil(B/32) x nprimal 64-bit words, 2 bits per class (0 dead 1 MINUS 2 ZERO 3 PLUS) */
int  bslv_poly_classify_batch(bslv_poly *h, int B, const double *hps, unsigned long long *words_out,
                              int *anyminus_out, int repeats, float *ms_out);
/* TEST: the incidence kernel as the chunked cut application launches it: tc_out[i] = halfspaces element i is not strictly
 * inside, t1_out[i] = the first of them or -1 (nv ints each); words_out as bslv_poly_classify_batch (may be NULL) */
int  bslv_poly_classify_batch_touch(bslv_poly *h, int B, const double *hps, unsigned long long *words_out, int *tc_out, int *t1_out);
/* MEASUREMENT ONLY: replace the polyhedron by nv synthetic live points (for timing the incidence kernel) */
int  bslv_poly_bench_fill(bslv_poly *h, int nv, unsigned long long seed);
/* counts and slot-indexed dumps (poly__vrtx2file / adj2file / inc2file write these, :341-414) */
int  bslv_poly_dim(const bslv_poly *h);
int  bslv_poly_nprimal(const bslv_poly *h);
int  bslv_poly_ndual(const bslv_poly *h);
long bslv_poly_nedges(const bslv_poly *h);
long bslv_poly_ninc(bslv_poly *h);
long bslv_poly_ndual_edges(const bslv_poly *h);
long bslv_poly_pair_tests(const bslv_poly *h);
long bslv_poly_new_vertices(const bslv_poly *h);
int  bslv_poly_get_primal(bslv_poly *h, unsigned char *used, unsigned char *ideal, unsigned char *sltn, double *coords);
int  bslv_poly_get_dual(bslv_poly *h, unsigned char *used, unsigned char *ideal, double *coords);
/* coordinates of the primal slots first .. first+count-1 only (count x dim, row-major): the coordinates of a slot never change, so
 * a caller that mirrors `polytope` (poly_compat.hip, bslv_poly.h:55-69) fetches only what a cut added */
int  bslv_poly_get_primal_range(bslv_poly *h, int first, int count, double *coords);
int  bslv_poly_get_edges(bslv_poly *h, int *ab);
int  bslv_poly_get_inc(bslv_poly *h, int *pairs);
int  bslv_poly_get_dual_edges(bslv_poly *h, int *ab);
/* CONSISTENCY CHECK of the resident polyhedron (poly__polyck, bslv_poly.c:940-990, and its converse). Read-only: no element, list,
 * edge, counter or statistic of the engine changes, and the next cut behaves bit for bit as without the call.
 *   out[0]  live elements                       out[1]  live facets (as bslv_poly_get_dual defines live)
 *   out[2]  incidences examined
 *   out[3]  BAD INCIDENCES: listed (element, facet) with |hp.x - alpha| > tol, alpha = 0 for an ideal element and hp the engine's own
 *           hyperplane of the dual slot; also a list entry that is no valid rank or an unapplied facet, an entry that does not ascend
 *           strictly, and (once) a list that does not lie inside the pool
 *   out[4]  UNLISTED INCIDENCES: a live element within POLY_EPS (1e-9) of a live facet's hyperplane that its list does not hold
 *   out[5]  INFEASIBLE: live element with hp.x - alpha < -tol for a live facet
 *   out[6]  edges in the list                   out[7]  BAD EDGES: an endpoint out of range, dead, or a == b
 *   out[8]  DUPLICATE EDGES: the same unordered pair again
 *   out[9]  pairs of the examined rows that pass the edge test (edge_test, bslv_poly.c:467-512)
 *   out[10] MISSING: passes the test, not listed (the reference's third check)
 *   out[11] EXTRA: listed, fails the test (the converse, which the reference omits)
 * Dual slot 0 while it is ideal is the facet at infinity (bslv_poly.c:83-92): its incidences are combinatorial, so it is counted in
 * [1] and [2], its entries are checked for rank and order, and it takes no part in the residuals of [3] nor in [4] and [5].
 * worst[0] = the largest |residual| of a listed incidence, worst[1] = the most negative slack met in [5]'s scan (0: none).
 * Rows: the live elements in ascending slot order are rows 0 .. L-1; the pair scan covers the pairs (i, j), i < j, with i in
 * [row_first, row_first + row_count), and [9]-[11] count those pairs only -- [11] counts a listed edge under the row of its smaller
 * endpoint, so the counts of a partition of the rows add up to those of the whole.  [2]-[8] are always over the whole polyhedron.
 * Offenders: (kind, a, b) with kind = the index into out (3, 4, 5, 7, 8, 10, 11) and (a, b) = (element, dual slot; -1 where the entry
 * names none) or (element, element), sorted by (kind, a, b); if there are more than max_off, *n_off is the total and which are kept
 * is unspecified.  BSLV_E_ARG: bad range, max_off < 0; BSLV_E_STATE: before bslv_poly_init.  The call waits for its stream.
 * What the check finds out of range it counts ([3], [7]) and never dereferences.  BSLV_POLY_CHECK_TIMING=1: one line per call on
 * stderr with the time of each kernel (HIP events). */
int  bslv_poly_check(bslv_poly *h, double tol /* <= 0: 1e-6, the reference's */, int row_first, int row_count /* < 0: all */,
                     long out[12], double worst[2] /* may be NULL */,
                     int *offenders /* 3 * max_off ints (kind, a, b), may be NULL */, int max_off, int *n_off);
/* for tests only: damage the resident state by plain copies (no kernel).  what 0: delete edge number a from the list (the last edge
 * takes its place), 1: append edge (a, b), 2: drop the last entry of element a's incidence list, 3: add x to coordinate b of element
 * a.  Anything else, or an index out of range, is BSLV_E_ARG. */
int  bslv_poly_debug_corrupt(bslv_poly *h, int what, int a, int b, double x);
/* COMPACTION of the resident polyhedron.  The slot of a cut-off element is never reused and a rebuilt incidence list is copied to the
 * end of the pool, so slots and pool words grow with the run, not with the live polyhedron; the 32-bit limits (2^30 elements, 2^30
 * edges, 0xF0000000 pool words) and everything proportional to nprimal count the dead as well.
 * bslv_poly_garbage (read-only, one small launch): out[0] primal slots in use (nprimal), [1] live elements, [2] pool words used, [3]
 * pool words the lists of live elements hold (sum of their lengths, slack not counted), [4] edges, [5] device bytes of the element,
 * pool and edge arrays at their current capacities.
 * bslv_poly_compact renumbers the live elements 0 .. live-1 in ascending order of their old slots (MONOTONE: live element i becomes its
 * rank among the live ones, dead slots vanish) and packs their lists; nprimal afterwards equals the live count.  new_of_old (nprimal-
 * before ints, may be NULL) receives the map, -1 for a dead slot; out (may be NULL) the six figures AFTER the call.  A second call
 * straight after is a no-op: the identity map, 0 removed, no allocation.
 *   Kept bit for bit: the coordinates, the used / ideal / sltn marks, every incidence list in its order (the lists hold facet RANKS,
 *   which do not change), the edge list in its order with both ends mapped, and the whole dual side (dual points, hyperplanes, the
 *   order of application, dual edges).  So bslv_poly_unprocessed2 / children_of / children_hist answer the same elements under their new
 *   names with the same parent facets, and the .sol writers produce the same bytes (they number live elements in slot order anyway).
 *   The pool is rebuilt densely (offsets = a 64-bit scan of the list lengths over the live elements), lists are packed WITHOUT slack --
 *   a long list gets its slack back at its next rebuild -- and no keep mark is set over the new pool.
 *   Legal only between bslv_poly_add / bslv_poly_add_cuts calls (never from inside a chunk of cuts: BSLV_E_STATE); a prune still in
 *   flight is waited for first.  A halfspace that was classified ahead of its turn is DROPPED: it is classified once more by its cut.
 *   An edge with an end that is no live element, or a list that does not lie inside the pool, is BSLV_E_STATE with a message and
 *   nothing is moved -- bslv_poly_check calls both defects, so none is expected, and none is silently dropped.
 *   OUT OF PLACE: every new array is allocated before anything moves, so a failed allocation is BSLV_E_NODEVICE and leaves the
 *   polyhedron untouched; the peak is old + new.  New capacities are max(the engine's minimum for that array, twice what is needed) and
 *   never above the old capacity: this is how memory is handed back.
 *   STALE IDS: element ids handed out before the call (bslv_poly_unprocessed*, bslv_poly_next, bslv_poly_children_of) are stale
 *   afterwards; the caller maps them through new_of_old.  bslv_poly_mark and every later call take NEW ids.
 *   h == NULL: BSLV_E_ARG.  Before bslv_poly_init, or with no element: 0, nothing done, the figures zero.
 * The reference's struct interface (bslv_poly_compat.h) does not offer compaction, and the drivers of the dual variant never ask.
 * bslv_poly_last_compact_stats: out[0] calls so far, [1] slots removed by the last call, [2] pool words removed, [3] bytes handed back
 * (capacities before - after), [4] slots removed by all calls, [5] pool words removed by all calls, [6] microseconds of the last call
 * (host clock around it), [7] of all calls.
 * The Benson driver can make the call by itself between applies: bslv_benson_set_compact / BSLV_POLY_COMPACT (section 4). */
int  bslv_poly_garbage(bslv_poly *h, long out[6]);
int  bslv_poly_compact(bslv_poly *h, int *new_of_old /* nprimal-before ints, may be NULL */, long out[6] /* may be NULL */);
int  bslv_poly_last_compact_stats(const bslv_poly *h, long out[8]);
/* host-only self-test of the two mailbox readers of the polyhedron engine (no GPU needed): a writer thread publishes `rounds`
 * messages with the sequence number FIRST and the content afterwards; 0 = every message was taken with its own content
 * (*torn_out: reads that had to be repeated), negative = a reader accepted foreign content.  which: 0 Mail, 1 round state */
int  bslv_selftest_mailbox(int which, int rounds, long *torn_out);
/* self-test of the index arithmetic of a windowed prune (needs a GPU, no polyhedron): the host builds the window table of a facet of
 * nm >= 2 members for window_blocks (0 = default, as bslv_poly_set_prune_window) and checks that the windows are contiguous, cover all
 * G(nm-1) pair blocks, hold at most max(window_blocks, their single row group) blocks each and keep every relative id below 2^31
 * (BSLV_E_STATE otherwise); a kernel takes `samples` hashed pairs i < j < nm, forms the virtual block as the pair kernel does, maps it
 * to (window, relative id) and back as the emission kernels do.  out[0] windows, [1] pair blocks in total, [2] pairs that did not come
 * back as (i, i + 1 + 256 c), [3] the largest relative id.  The only place where block ids beyond 2^32 run in milliseconds. */
int  bslv_selftest_pair_blocks(int nm, long window_blocks, int samples, long out[4]);

/* ------------------------------------------------------------------------------------------
 * 4. Batched Benson phase-2 driver  (replaces phase2_primal's loop, bslv_algs.c:958-1082,
 *    and init_P2, :574-664).  Problem in the reference's normal form "min, c_q > 0"
 *    (sol_init, bslv_vlp.c:845-861); A is m x n, P is q x n, dense row-major; bound types
 *    'f','l','u','d','s' as in the .vlp format; R is q x r with generators as columns
 *    (bslv_algs.c:599) -- R = Z = I for the default cone in the bounded case (-b, :943-956).
 *    One outer iteration = collect -> solve_local -> (all-gather records) -> apply.
 * ------------------------------------------------------------------------------------------ */
typedef struct bslv_benson bslv_benson;

int  bslv_benson_create(bslv_benson **out, int m, int n, int q, const double *A, const double *P,
                        const char *rtype, const double *rlb, const double *rub,
                        const char *ctype, const double *clb, const double *cub,
                        const double *R, int r, const double *c, double eps, int pool_slots);
/* the same with the homogeneous problem of phases 0 and 1 (init_P2(..., HOMOGENEOUS), bslv_algs.c:574-664): hom != 0 zeroes
 * every bound of the VLP ('d' becomes fixed; lp_set_rows_hom / lp_set_cols_hom, bslv_lp.c:118-134), R holds the generators Z
 * of the dual ordering cone and the last row reads eta.y <= 1 (eta NULL = 0).  The cut of a vertex is then
 * y* = (w + alpha eta, alpha), alpha = dual of that row (phase1_primal, bslv_algs.c:876-883). */
int  bslv_benson_create_ex(bslv_benson **out, int m, int n, int q, const double *A, const double *P,
                           const char *rtype, const double *rlb, const double *rub,
                           const char *ctype, const double *clb, const double *cub,
                           const double *R, int r, const double *c, const double *eta, int hom, int flags, double eps, int pool_slots);
/* flags of bslv_benson_create_ex.  PREIMAGES = option -s (opt->solution == PRE_IMG_ON): the engine keeps x of every confirmed
 * vertex and (u, w) of every cut (bslv_algs.c:1064-1079); every row of A stays in the LP (no presolve) */
enum { BSLV_BENSON_PREIMAGES = 2 };
/* 0 + data, or 1 when nothing is stored for that element */
int  bslv_benson_preimage_p(const bslv_benson *h, int element, double *x /* n */);
int  bslv_benson_preimage_d(const bslv_benson *h, int facet, double *uw /* m + q */);
int  bslv_benson_set_preimage_p(bslv_benson *h, int element, const double *x /* n */);
void bslv_benson_destroy(bslv_benson *h);
int  bslv_benson_start(bslv_benson *h, int *vlp_status /* 0 ok, 1 infeasible, 2 unbounded */);
int  bslv_benson_collect(bslv_benson *h, int max_batch, int rank, int world, int *n_local, int *n_total);
int  bslv_benson_record_len(const bslv_benson *h);             /* q + 5 doubles */
int  bslv_benson_solve_local(bslv_benson *h, double *records, int *pivots_out, int *lockstep_out);
int  bslv_benson_apply(bslv_benson *h, int nrec, const double *records, long *stats /* 5, may be NULL */);
int  bslv_benson_step(bslv_benson *h, int max_batch, long *stats /* 8 */, double *ms /* 3 */);
/* two batch contexts (ctx 0/1): the LPs of batch k (solve_local_ctx, may run on a second host thread) overlap with
 * the cut application of batch k-1 (apply_ctx).  set_pipelined(1): batch members are marked when collected. */
int  bslv_benson_set_pipelined(bslv_benson *h, int on);
int  bslv_benson_collect_ctx(bslv_benson *h, int ctx, int max_batch, int rank, int world, int *n_local, int *n_total);
int  bslv_benson_solve_local_ctx(bslv_benson *h, int ctx, double *records, int *pivots_out, int *lockstep_out);
int  bslv_benson_apply_ctx(bslv_benson *h, int ctx, int nrec, const double *records, long *stats);
int  bslv_benson_unprocessed_left(const bslv_benson *h);
/* CANONICAL DUALS: with on != 0 the cut of every vertex v is built from the dual that P2(v + t d) would have for small t > 0 instead
 * of the dual the pivoting happened to reach (w of bslv_algs.c:1050), d_k = 1 + hash01(k) a fixed generic direction -- a facet normal
 * of the image at y = v + z c also where y lies on an edge or a vertex.  The driver hands dir_j = R_j . d to bslv_lpq_set_canonical on
 * its LP engine (the bound of row j is R_j . v, :1041-1046); the LPs of the retry ladder are solved with it too, the weighted-sum LPs
 * of PART 1 are not.  Off by default; BSLV_CANONICAL_DUAL=1 switches it on when an engine is created.  A homogeneous engine (hom != 0)
 * answers BSLV_E_ARG: its cut (w + alpha eta, alpha) has another normal cone (the environment switch leaves such engines alone).  The
 * dual-variant entry points do not know this switch; theirs is BSLV_VLP_CANONICAL (bslv_vlp_solve_dual2).  bslv_benson_canonical_stats: the four counts of bslv_lpq_last_canonical_stats
 * summed over the LPs of the last solve_local, retries included (last), and over all of them (total); either may be NULL. */
int  bslv_benson_set_canonical(bslv_benson *h, int on);
int  bslv_benson_get_canonical(const bslv_benson *h);
int  bslv_benson_canonical_stats(const bslv_benson *h, long last[4], long total[4]);
/* THE SIMPLEX METHOD of the driver's LPs (the reference: lp_set_options per phase, -k / -L / -l).  method = BSLV_LP_METHOD_DUAL /
 * _PRIMAL / _REPAIR, or -1 = unset, the default: the calls as they always were, bit for bit (the LP engine's own method).  Set, the
 * weighted-sum LPs of the start, every P2(v) batch of bslv_benson_solve_local (and its _ctx twin) and every stage of its retry -- from
 * the root tableau, from the standard basis, with the extended selection -- go through bslv_lpq_solve_batch_method, in both forms of
 * the LP engine.  With bslv_benson_set_canonical on, the tableau form keeps its tie phase (the engine's switch holds under every method
 * of a call); a revised engine, whose tie phase is bslv_lpq_solve_batch_canonical under the engine's own method, accepts DUAL and answers
 * BSLV_E_ARG to PRIMAL and REPAIR from solve_local, with a message that names both.  BSLV_BENSON_LP_METHOD=dual|primal|repair sets it
 * when an engine is created.  Anything else: BSLV_E_ARG.  bslv_benson_lp_method_stats: LPs handed to such calls so far under DUAL,
 * PRIMAL, REPAIR (retries count again; all 0 while unset). */
int  bslv_benson_set_lp_method(bslv_benson *h, int method);
int  bslv_benson_get_lp_method(const bslv_benson *h);
int  bslv_benson_lp_method_stats(const bslv_benson *h, long out[3]);
/* THE PRICING RULES of the driver's LPs, per call (bslv_lpq_solve_batch_method_priced): dual_rule and primal_rule are
 * BSLV_LP_PRICING_DANTZIG / _DEVEX, or -1 / -1 = unset, the default.  Set, and only while the driver carries a method
 * (bslv_benson_set_lp_method), the batches that went through bslv_lpq_solve_batch_method -- the start LPs, the P2(v) batches and both
 * stages of the retry -- go through bslv_lpq_solve_batch_method_priced with these rules; without a method, or unset, the calls are what
 * they were, bit for bit.  The LP engine's own switches are not touched.  This is how Devex pricing reaches the PRIMAL / REPAIR batches
 * of a revised LP engine.  One rule -1 and the other not, or any other value: BSLV_E_ARG, nothing changed.
 * BSLV_BENSON_LP_PRICING=<dantzig|devex>[:<dantzig|devex>] (dual[:primal], primal defaulting to dantzig) sets them when an engine is
 * created, next to BSLV_BENSON_LP_METHOD (so bensolve_hip -l primal_simplex gets the rule without an option of its own); a malformed
 * value leaves them unset.  bslv_benson_get_lp_pricing: the two rules as set (either pointer may be NULL); BSLV_E_ARG for h == NULL. */
int  bslv_benson_set_lp_pricing(bslv_benson *h, int dual_rule, int primal_rule);
int  bslv_benson_get_lp_pricing(const bslv_benson *h, int *dual_rule, int *primal_rule);
/* LP CERTIFICATE: with on != 0 bslv_benson_solve_local and its _ctx twin certify the LPs of the batch that ended BSLV_LP_OPTIMAL with
 * bslv_lpq_certify, after the retries and before the getters, with the slots and bounds of the solve.  The first LP that is not certified
 * is printed on stderr (batch number, slot, the five residuals and where they were met), a summary line when the engine is destroyed;
 * the run goes on, no record, cut or status changes.  Off by default (nothing is allocated, no launch is added); BSLV_LP_CERTIFY=1
 * switches it on when an engine is created.  bslv_benson_certify_stats: counts = LPs certified, LPs with a verdict other than 0, calls;
 * worst = the largest residual of each kind so far (rows, feas, dj, side, gap); either may be NULL.  The P1(w) batches of the dual
 * variant do not pass through solve_local: bslv_lpq_certify serves them directly. */
int  bslv_benson_set_certify(bslv_benson *h, int on);
int  bslv_benson_get_certify(const bslv_benson *h);
int  bslv_benson_certify_stats(const bslv_benson *h, long counts[3], double worst[5]);
/* COMPACTION TRIGGER: with dead_fraction f in (0, 1] bslv_benson_apply and its _ctx twin END -- after the cuts and the parking -- with
 * bslv_poly_compact on their polyhedron when it holds at least min_slots primal slots (< 0: the default, 65536) and
 * (slots - live) / slots >= f; the driver then re-keys what it holds by primal element (the pre-images of option -s) through
 * new_of_old.  0 = off, the default: no launch, no synchronisation, no allocation and no bit of any result changes; switched on, an
 * apply that reaches min_slots pays one small counting launch.  f negative, above 1 or NaN: BSLV_E_ARG, the switch stays as it was.
 * BSLV_POLY_COMPACT=f[:min] sets it when an engine is created, homogeneous engines included (nothing about compaction depends on the
 * cut formula).
 * PIPELINED MODE: while the OTHER batch context holds a collected batch that is not applied yet, the trigger is skipped -- that batch's
 * element ids are in flight in solve_local_ctx, possibly on another thread, and come back in its records; it fires at the next apply
 * that finds the other context empty.
 * SEVERAL RANKS: the decision reads replicated state only (slots, live count), so every rank compacts after the same apply and the
 * element ids in the records that travel between ranks keep one meaning.
 * STALE IDS: an element id a caller took from the engine's polyhedron before an apply (bslv_poly_unprocessed*, bslv_benson_preimage_p
 * keys) may be stale after it once the switch is on; bslv_benson_collect_given must be given ids read after the last apply.
 * bslv_benson_compact_stats: out[0] compactions, [1] slots removed, [2] pool words removed, [3] microseconds, all of them summed. */
int  bslv_benson_set_compact(bslv_benson *h, double dead_fraction /* 0 = off (default); (0, 1] */, long min_slots /* < 0: the default, 65536 */);
int  bslv_benson_compact_stats(const bslv_benson *h, long out[4]);
/* batch selection: 1 = newest vertices first (default), 2 = spread evenly over the unprocessed queue, 3 = newest first but at
 * most `cap` children of one cut per batch, chosen from a window of `window` batches (set_sibling_rule; default 1, 8): the
 * children of one cut mostly see the same facet of the upper image, so their LPs return the same cut -- the reference's
 * sequential loop never solves them, because the first copy of the cut removes the siblings (bslv_algs.c:1030-1080) */
int  bslv_benson_set_policy(bslv_benson *h, int policy);
int  bslv_benson_set_sibling_rule(bslv_benson *h, int cap, int window);
/* policy 4: K depth-first fronts (a vertex belongs to the front of the cut that created it, a cut to the front of the vertex
 * whose LP returned it; newest first inside a front, at most sib_cap children of one cut per front and batch) */
int  bslv_benson_set_fronts(bslv_benson *h, int nfronts, int sib_cap);
/* policy 5: the children of the newest cuts first (by the dual slot of the cut, not by the element's own slot);
 * policy 6: whole families -- all unprocessed children of a cut -- of parents chosen among the cuts of the last `batches` outer
 * iterations: mode 0 newest cuts first, 1 pseudo-random, 2 far apart (farthest-point sampling on the cuts' normals) */
int  bslv_benson_set_families(bslv_benson *h, int mode, int batches);
/* Thin rounds at the end of a chunk of cuts (its cliques, one cut each per pass over the polyhedron) may hand their cuts back
 * (bslv_poly_set_defer(min_cuts)); bslv_benson_apply keeps them and hands them in again in front of the next batch's cuts,
 * bslv_benson_collect applies whatever is waiting before it reports "nothing left".  0 = off (every cut of a batch is applied
 * in its own outer iteration, as bslv_algs.c:1041-1080 does).  stats: [0] handed back so far, [1] waiting, [2] flushes by
 * collect, [3] batches that one family would have filled (taken newest first). */
int  bslv_benson_set_defer(bslv_benson *h, int min_cuts);
int  bslv_benson_defer_stats(const bslv_benson *h, long out[4]);
/* tuning hooks (no counterpart in the reference): the caller chooses the batch itself -- elements with their coordinates and
 * parent facets as bslv_poly_unprocessed2 returns them -- and reads, per LP of this rank's last solve_local, the warm-start slot
 * (0 = root tableau), the pivots and the generation of the new slot; returns the number of entries written */
int  bslv_benson_collect_given(bslv_benson *h, int n, const int *idx, const double *val, const int *parent, int rank, int world, int *n_local, int *n_total);
int  bslv_benson_last_local(bslv_benson *h, int max_out, int *src, int *pivots, int *gen);
/* tableau pool: out[0] free slots, [1] resident warm-start sources, [2] held by a batch in flight, [3] pool size */
int  bslv_benson_pool_stats(bslv_benson *h, long out[4]);
/* the resident warm-start sources themselves (read-only, for probes: scripts/probe/tableau_drift.py): their slots and, per slot, its
 * generation -- the warm starts between the root tableau and the slot; either may be NULL.  Returns the number of entries written, at
 * most max_out */
int  bslv_benson_resident_slots(bslv_benson *h, int max_out, int *slots, int *gen);
/* apply() parks the tableau passes of the slots it keeps (bslv_lpq_park) and tells the LP engine which parked slots the pool has
 * evicted (bslv_lpq_drop_parked); set_park(h, 0), or BSLV_LP_PARK=0 at create, makes the passes at the end of apply() instead
 * (bslv_lpq_materialise).  Same LPs, same cuts, same slots either way.  park_stats: as bslv_lpq_park_stats. */
int  bslv_benson_set_park(bslv_benson *h, int on);
int  bslv_benson_park_stats(const bslv_benson *h, long out[5]);
int  bslv_benson_totals(const bslv_benson *h, long *lps, long *cuts, long *pivots);
/* warm starts: LPs whose parent's tableau was not resident on this rank (evicted, or solved on another rank) and that started
 * from the root tableau / from the resident tableau whose own vertex is nearest */
int  bslv_benson_start_stats(const bslv_benson *h, long *root_starts, long *nearest_starts);
/* size of the P2 model: M x N of init_P2 (bslv_algs.c:574-664), the model every index at the LP boundary refers to;
 * rows_folded of its rows (rows of A with a single non-zero: the hypercube rows of S-degenerate, ex/example10.m:21-24) were
 * turned into column bounds by the LP layer's presolve (bslv_lpq_create), so the tableau has M - rows_folded rows */
int  bslv_benson_lp_dims(const bslv_benson *h, int *M, int *N, int *rows_folded);
bslv_poly *bslv_benson_poly(bslv_benson *h);
bslv_lpq  *bslv_benson_lp(bslv_benson *h);

/* ------------------------------------------------------------------------------------------
 * 4a. Multi-GPU: one process per GPU, one exchange step per outer iteration, in the library.
 *     bslv_set_device(LOCAL_RANK), then either bslv_dist_init with the 128-byte ncclUniqueId of rank 0 (RCCL over xGMI; the
 *     host side distributes the id: bensolve_hip over TCP to MASTER_ADDR:MASTER_PORT, bench.py with one broadcast), or
 *     bslv_dist_init_callback with an all-gather of the caller (tests on a one-GPU box, where RCCL refuses two ranks on one
 *     device).  From then on bslv_benson_step -- and with it bslv_vlp_solve_primal and the command-line driver -- runs
 *     bslv_benson_step_dist: the vertex batch is dealt to the ranks (bslv_benson_collect), every rank solves its shard, ONE
 *     all-gather of fixed-size record blocks, every rank applies all records in ascending source slot, so the replicas of
 *     the polyhedron stay bit-identical.  The reference has no counterpart (single process, bslv_algs.c:1030-1080).
 * ------------------------------------------------------------------------------------------ */
typedef int (*bslv_allgather_fn)(const double *send, double *recv, int count_per_rank, void *ctx);   /* 0 = ok */
int  bslv_dist_unique_id(unsigned char *out, int len /* >= 128 */);          /* rank 0: ncclGetUniqueId */
int  bslv_dist_init(int rank, int world, const unsigned char *id, int len);  /* ncclCommInitRank on the current device */
int  bslv_dist_init_callback(int rank, int world, bslv_allgather_fn fn, void *ctx);
void bslv_dist_finalize(void);
int  bslv_dist_rank(void);
int  bslv_dist_world(void);
int  bslv_dist_allgather(const double *send, double *recv, int count_per_rank);   /* host buffers; recv holds world * count */
int  bslv_dist_stats(long *gathers, double *ms);
int  bslv_benson_step_dist(bslv_benson *h, int max_batch_global, long *stats /* 8 */, double *ms /* 3 */);
/* host wall clock (ms) of the phases of the last bslv_benson_step_dist on this rank: collect, this rank's LPs, all-gather of the
 * records (includes the wait for the slowest rank), application of all ranks' cuts (replicated on every rank) */
int  bslv_dist_last_phases(double out[4]);

/* ------------------------------------------------------------------------------------------
 * 4b. The callers around phase 2: ordering cone data (sol_init, bslv_vlp.c:599-864), cone_vertenum
 *     (bslv_algs.c:331-407), phase 0 (bslv_algs.c:673-800), phase 1 of the primal algorithm (bslv_algs.c:811-933) and the
 *     sequence of bslv_main.c:236-345.  Matrices of generators are q x k row-major with the generators as columns
 *     (M[j*k + i] = component j of generator i), as sol->Z / sol->R / vlp->gen are.
 * ------------------------------------------------------------------------------------------ */
typedef struct bslv_vlp_info {
    int q, o, p, r, h;            /* soltype: generators of C (o), of C* (p), of the dual recession cone (r), of the recession cone (h) */
    int c_dir;                    /* +1 c_q > 0, -1 c_q < 0 (bslv_vlp.c:690-776) */
    int negate_primal;            /* poly_trans_primal (bslv_algs.c:221-229): the result writers negate y ... */
    int negate_dual_last;         /* ... and y*_q */
    long lps, steps;              /* LPs solved in all phases, outer iterations */
    double *c, *eta, *R, *H, *Y, *Z;   /* malloc'ed: c as written to _c.sol (before the sign change of :844-853); free with bslv_vlp_info_free */
    char message[160];            /* the reference's message when the status is not "optimal" */
} bslv_vlp_info;
/* flags: PHASE1_DUAL = "-A dual" (opt->alg_phase1, bslv_main.c:283-296: phase1_dual, bslv_algs.c:1248-1371, instead of
 * phase1_primal); PREIMAGES = "-s" (opt->solution == PRE_IMG_ON; bslv_vlp_solve_primal only): the phase-2 engine keeps the
 * pre-images (BSLV_BENSON_PREIMAGES) and the directions of the upper image get theirs (bslv_algs.c:1083-1112);
 * CANONICAL (bslv_vlp_solve_dual2 only; BSLV_CANONICAL_OBJ=1 in the environment sets it there): phase 2 switches
 * bslv_lpq_set_canonical_obj on for its P1(w) LPs -- PART 1, the batches and their retries -- with ddir = sum_j (1 + hash01(j)) R_j
 * over the generators R_j of the cone the weights live in (a generic interior point of it, so ddir . y is bounded below on every
 * optimal face; the default cone: ddir_k = 1 + hash01(k), the direction of bslv_benson_set_canonical): every cut of the lower image is
 * then built from a VERTEX of the upper image (bslv_algs.c:1479-1486) and is a facet.  The homogeneous engine of phase1_dual is left
 * alone.  An LP engine that comes up in the revised form makes the call fail with that engine's message;
 * CANONICAL_CALL (bslv_vlp_solve_dual2 only; BSLV_CANONICAL_OBJ_CALL=1 in the environment sets it there): the same ddir, handed to
 * every P1(w) solve -- PART 1, the batches and their retries -- per call, through bslv_lpq_solve_batch_obj_canonical, in both forms
 * of the LP engine: the way to the canonical points on an engine in the revised form.  The engine's switch stays off.  Neither flag
 * is a default. */
enum { BSLV_VLP_PHASE1_DUAL = 1, BSLV_VLP_PREIMAGES = 2, BSLV_VLP_CANONICAL = 4, BSLV_VLP_CANONICAL_CALL = 8 };
/* THE LP METHOD PER PHASE (the reference: -k / -L / -l, lp_set_options per phase_type).  Two bits per phase above the four flags:
 * BSLV_VLP_LP_METHOD(phase, m) with phase 0, 1, 2 and m = BSLV_LP_METHOD_DUAL / _PRIMAL / _REPAIR; nothing given for a phase = "auto"
 * = the calls as they always were, NOT the reference's default of that phase (making phase 0 primal because the reference does would
 * change every existing run).  A given method reaches: phase 0's LPs (bslv_lpq_solve_batch_method, their retry from the standard basis
 * included); the homogeneous Benson engine of phase 1 (bslv_benson_set_lp_method) or, with PHASE1_DUAL, the feasibility LP and the
 * objective batches of the homogeneous dual variant (bslv_lpq_solve_batch_obj_method); in phase 2 the Benson engine of
 * bslv_vlp_solve_primal or the feasibility LP and the P1(w) batches of bslv_vlp_solve_dual2, PART 1 and retries included.  The LPs of the
 * pre-images of directions (PREIMAGES) take none.  bslv_vlp_solve_dual2 with CANONICAL or CANONICAL_CALL and a phase-2 method other
 * than primal: BSLV_E_ARG (the tie phase of objective batches follows a PRIMAL solve only).
 * bslv_vlp_last_lp_method_stats, of the calling thread's last solve: out[phase_type][method] = LPs handed to a call under that
 * method, phase_type as the reference's enum (PHASE0, PHASE1_PRIMAL, PHASE1_DUAL, PHASE2_PRIMAL, PHASE2_DUAL); retries count again;
 * all 0 where no method was given. */
#define BSLV_VLP_LP_METHOD(phase, m) (((m) + 1) << (4 + 2 * (phase)))
#define BSLV_VLP_LP_METHOD_OF(flags, phase) ((((flags) >> (4 + 2 * (phase))) & 3) - 1)      /* -1: not given */
int  bslv_vlp_last_lp_method_stats(long out[5][3]);
/* cone_kind 0 default (R^q_+), 1 `gen` generates C, 2 `gen` generates C* (vlp->cone_gen); c_in: q or NULL (vlp->c).
 * vlp_status (sol->status, bslv_main.h:103): 1 infeasible, 2 unbounded, 3 no vertex, 4 optimal, 5 input error.
 * With status 4 *engine_out is the finished phase-2 engine (bslv_benson_poly(engine) is the result; destroy it). */
int  bslv_vlp_solve_primal(int m, int n, int q, const double *A, const double *P,
                           const char *rtype, const double *rlb, const double *rub,
                           const char *ctype, const double *clb, const double *cub,
                           int optdir, int cone_kind, const double *gen, int n_gen, const double *c_in,
                           int bounded, int flags, double eps_phase0, double eps_phase1, double eps_benson_phase1, double eps_benson_phase2,
                           int batch, bslv_benson **engine_out, int *vlp_status, bslv_vlp_info *info /* may be NULL */);
/* the same with the DUAL algorithm in phase 2 ("-a dual": phase2_dual, bslv_algs.c:1381-1592, P1(w) LPs that differ in the
 * objective; phases 0 and 1 stay primal).  With status 4 *lower_image_out is a polyhedron whose primal side is the LOWER image
 * and whose dual side is the upper image: write it with bslv_sol_write3(..., swap = 1, ...), destroy with bslv_poly_destroy. */
int  bslv_vlp_solve_dual2(int m, int n, int q, const double *A, const double *P,
                          const char *rtype, const double *rlb, const double *rub,
                          const char *ctype, const double *clb, const double *cub,
                          int optdir, int cone_kind, const double *gen, int n_gen, const double *c_in,
                          int bounded, int flags, double eps_phase0, double eps_phase1, double eps_benson_phase1, double eps_benson_phase2,
                          int batch, bslv_poly **lower_image_out, int *vlp_status, bslv_vlp_info *info /* may be NULL */);
/* the four counters of bslv_lpq_last_canonical_obj_stats summed over the objective solves of phase 2 of the calling thread's last
 * bslv_vlp_solve_dual2 (all zero without BSLV_VLP_CANONICAL or BSLV_VLP_CANONICAL_CALL) */
int  bslv_vlp_last_canonical_obj_stats(long out[4]);
/* option -s with the dual algorithm (flags & BSLV_VLP_PREIMAGES in bslv_vlp_solve_dual2; phase2_dual with PRE_IMG_ON,
 * bslv_algs.c:1388-1389, 1431-1432, 1484-1497, 1508-1546): x (n values) of an element of the UPPER image = dual slot `facet` of the
 * returned polyhedron, (u, w) (m + q values) of a vertex of the LOWER image = its primal element.  0 + data, 1: nothing stored.
 * bslv_dual_preimages_free before bslv_poly_destroy. */
int  bslv_dual_preimage_x(const bslv_poly *lower_image, int facet, double *x);
int  bslv_dual_preimage_uw(const bslv_poly *lower_image, int element, double *uw);
void bslv_dual_preimages_free(const bslv_poly *lower_image);
void bslv_vlp_info_free(bslv_vlp_info *info);
/* cone_vertenum: prim = the non-redundant generators among gen (dim x n_prim), dual = generators of the dual cone
 * (dim x n_dual); malloc'ed, free with bslv_free.  rc_out 1: the cone has no interior (poly__intl_apprx failed). */
int  bslv_cone_vertenum(const double *gen, int n_in, int dim, double **prim, int *n_prim, double **dual, int *n_dual, int *rc_out);
void bslv_free(void *p);

/* ------------------------------------------------------------------------------------------
 * 5. Host side that stays C: the .vlp reader (vlp_init, bslv_vlp.c:275-588; kept file-format
 *    contract) and the result-file writers (poly_output, bslv_algs.c:50-144; formats of
 *    bslv_poly.c:341-414).  Struct bslv_vlp: bensolve_amd/csrc/host/bslv_host.h.
 * ------------------------------------------------------------------------------------------ */
struct bslv_vlp;
int  bslv_vlp_read(const char *path, struct bslv_vlp **out, int *err_line);
void bslv_vlp_free(struct bslv_vlp *v);
const char *bslv_vlp_message(const struct bslv_vlp *v);
int  bslv_sol_write(bslv_poly *poly, const char *base, const char *suffix, int optdir, long *counts /* 4, may be NULL */);
/* the same with the two sign changes of poly_trans_primal (bslv_algs.c:221-229) spelled out (bslv_vlp_info) */
int  bslv_sol_write2(bslv_poly *poly, const char *base, const char *suffix, int negate_primal, int negate_dual_last, long *counts);
/* swap != 0: the engine's primal side is the LOWER image (dual algorithm; poly_output(..., SWAP, ...), bslv_algs.c:1566-1573) */
/* <base>_pre_img_p<suffix> / _pre_img_d<suffix> (poly__primg2file, bslv_poly.c:362-380; poly_output :120-139): one row per
 * element in the order of the _img_ files: x (n values) of the upper image's elements, (u, w) (m + q values) of the lower
 * image's vertices, zeros where nothing is stored (directions of the lower image, :1114-1121).  u is multiplied by optdir
 * and w by c_dir as the reference stores them (:1068-1070). */
int  bslv_sol_write_preimages(bslv_benson *eng, const char *base, const char *suffix, int m, int n, int optdir, int c_dir);
int  bslv_sol_write3(bslv_poly *poly, const char *base, const char *suffix, int swap, int negate_upper, int negate_lower_last, long *counts);
/* the pre-image files of the dual algorithm: rows in the order of the _img_ files written by bslv_sol_write3(..., swap = 1, ...) */
int  bslv_sol_write_preimages_dual(bslv_poly *lower_image, const char *base, const char *suffix, int m, int n, int optdir, int c_dir);

#ifdef __cplusplus
}
#endif
#endif
