// lp_engine.hip -- batched bounded dual simplex on HBM-resident dense tableaux (gfx950).
//
// Replaces, for whole batches of right-hand sides, what the reference does one LP at a time
// through GLPK: lp_set_rows + lp_solve + getters (bslv_lp.c:112-116, 219-259, 261-308) as driven
// by phase2_primal's loop (bslv_algs.c:1041-1062).
//
// Data layout in HBM (one "slot" per LP):
//   T     (M+1) x ld doubles, row-major, ld = N rounded up to 16 doubles (128-B rows);
//         rows 0..M-1: x_B = T x_N ; row M: reduced costs d (objective = d . x_N)
//   beta  M+1 doubles: values of the basic variables, beta[M] = objective value (without shift)
//   xN    ld doubles: values of the nonbasic variables (padding = 0)
//   bh[M], nh[N] basis heads (variable ids: 0..M-1 aux, M..M+N-1 structural)
//   nstat[N] nonbasic status, pos[M+N] (row if basic, -1-col if nonbasic)
// One ROUND of the lock-step loop = KP x k_select (one workgroup per LP: leaving row, Harris ratio test on the tableau as it
// would be after the pivots still pending -- rebuilt from the stored tableau and the pending (pivot row, multipliers) pairs)
// + k_flush (persistent grid over (LP, row tile): pure HBM streaming, every tableau element read once, all pending pivots
// applied to it in order, written once -> 16 B per element per ROUND instead of per pivot).
// bslv_lpq_certify, the read-only optimality certificate of solved slots (tests/lp_cases.py: certify, on the device): lp_certify.inc.
#include "common.h"
#include <vector>
#include <algorithm>
#include <chrono>
#include <type_traits>

namespace bslv {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// debugging aids of common.h (malloc0 / grow): fill byte of fresh device memory, allocation log
int debug_fill()
{
    static const int v = [] { const char *e = getenv("BSLV_FILL"); return e ? (int)(strtol(e, nullptr, 0) & 0xFF) : 0; }();
    return v;
}
void debug_note_alloc(const char *name, const void *p, size_t bytes, const char *file, int line)
{
    static const char *path = getenv("BSLV_ALLOC_LOG");
    if (!path) return;
    FILE *f = fopen(path, "a");
    if (!f) return;
    const char *base = strrchr(file, '/');
    fprintf(f, "%s %p %zu %s:%d\n", name, p, bytes, base ? base + 1 : file, line);
    fclose(f);
}

constexpr int NS_L = 0, NS_U = 1, NS_F = 2, NS_S = 3;
constexpr int ST_RUNNING = -1;
constexpr int MODE_NONE = 0, MODE_PIVOT = 1, MODE_REFRESH = 2;
constexpr int PRIMAL_STALL = 500;           // consecutive degenerate steps of a primal clean-up before Bland's rule takes over (until a step has a length again)
constexpr int PF_PERT = 1, PF_PRIMAL = 2, PF_PERT_PENDING = 4, PF_USES_SHIFT = 8;   // BatchView::pflags
// primal phase 1 (bits 4..7 of pflags; the perturbations of the solve are counted from bit PF_USES_SHIFT up): the LP is in phase 1 and dper
// holds its pricing vector d1; it has been there in this solve; d1 has to be rebuilt from the rows; d1 is current although nothing is pending
constexpr int PF_PHASE1 = 16, PF_P1_SEEN = 32, PF_P1_STALE = 64, PF_P1_KEEP = 128;
// RAY RECORD (bslv_lpq_set_rays): the thread that concludes INFEASIBLE or UNBOUNDED while it holds the proof leaves one word in
// BatchView::stall -- a finished LP has no use for its stall count, and no member is added to BatchView (see NormView) -- from which k_ray
// builds the vector after the rounds: RAY_REC | index << 7 | pending pivots << 3 | side << 2 | what.  what: RAY_ROW = the dual selection's
// row `index` without an entering candidate (side: below its lower bound), RAY_P1 = phase 1 without an improving column, RAY_DIR = the
// primal step's column `index` without a blocking row (side: dir = +1).  The pending count says where the selection's row[] / pc[] lie.
// A stall count never reaches RAY_REC (it is at most the iteration limit).
constexpr int RAY_REC = 1 << 30, RAY_ROW = 1, RAY_P1 = 2, RAY_DIR = 3, RAY_IDX_MAX = 1 << 23;
__device__ __forceinline__ int ray_record(int what, int idx, int np, bool side) { return RAY_REC | (idx << 7) | (np << 3) | (side ? 4 : 0) | what; }
constexpr int STALL_LIMIT = 3;         // consecutive degenerate pivots (dual step <= 1e-11) after which the costs are perturbed
constexpr int PERT_MAX_USES = 3;       // perturbations per solve
#ifndef BSLV_KP
#define BSLV_KP 6
#endif
constexpr int KP = BSLV_KP;                  // pivots selected between two passes over the tableau (delayed update; 4: 3.4 ms, 6: 3.0, 8: 3.1 ms per S-mid batch)
constexpr int REFRESH_AFTER = 32;      // pivots of one solve after which optimality is only declared on a recomputed beta
constexpr double TOL_BND = 1e-9, TOL_DJ = 1e-9, TOL_PIV = 1e-9;
constexpr double BIG = 1e7;   // artificial bound for dual-infeasible free columns
constexpr int TR = 32;        // tableau rows per workgroup in k_flush / k_init
constexpr int NT = 256;       // threads per workgroup
constexpr int FLIP_INCR_MAX = 48;   // bound switches of one iteration that beta follows by a vector update (more: recomputed in the pass)
constexpr int NT_BIG = 1024;  // k_flush where its LDS footprint leaves room for one or two workgroups per CU

struct PivDesc { int r, q; double p, pbeta, enter_val; };

struct LpView {
    int M, N, ld, Mp1, Mp1p, vfirst, vcnt, maxit, bland_after, trace, stall_limit;
    int objmode, cfirst, ccnt;  // solve_batch_obj: the LPs of the batch differ in the cost of variables cfirst .. cfirst+ccnt-1 (BatchView::cvals)
    size_t slotT;
    double pert_scale;          // multiplies the cost perturbation (1; tests raise it to force the clean-up paths)
    double *T, *beta, *xN;
    int *bh, *nh, *nstat, *pos;
    const double *lb, *ub;
    const unsigned char *art;   // bit0: lb is artificial, bit1: ub is artificial
    // REVISED FORM (round 4; bslv_lpq_create chooses it for wide sparse problems -- ex07 / ex09 of the reference's suite, which hands A
    // to GLPK as COO, bslv_lp.c:60-70): the matrix of a slot is the BASIS INVERSE B^-1 (M x ldt) instead of the tableau
    // T = -B^-1 N ((M+1) x ld), A is kept once, as CSC and CSR, for the whole pool.  With K = [I | -A] (column k of K belongs to
    // variable k: e_k for the auxiliary variable of row k, -A_j for structural j) a basis is B = K[:, bh] and
    //   row r of the tableau     T[r][j] = -rho . K_nh[j],  rho = row r of B^-1     (one sparse dot product per nonbasic column)
    //   column q of the tableau  T[:, q] = -B^-1 K_nh[q]                            (a few columns of B^-1)
    // and a pivot updates B^-1 by the SAME row operations it applies to the tableau -- row r := -rho p, row i -= f_i rho -- so the
    // delayed update, k_flush and its roofline carry over; only the tableau's column swap (entry q of every row) has no counterpart.
    // ex09: 171 MB per slot instead of 1.36 GB.  rev == 0: ldt = ld, mrows = M + 1 and everything is as before.
    int rho_off;                // rev: byte offset of the LDS copy of rho (row of B^-1 the tableau row is built from) in k_select's dynamic LDS, or -1 (does not fit: gathers from global memory)
    int helpers, launch_id;      // revised form: workgroups per LP in k_select (1 = none besides the LP's own) that share the sparse products of a tableau row; a number per launch for their mailbox
    int rev, ldt, mrows, probe;  // probe: BSLV_REV_PROBE, timing experiments only (8: phase clocks of the selection, see phase_mark; 16: rev_take_slices without its release fence)
    double *dsl;                // rev: [slots][ld] reduced costs of each slot (the tableau form keeps them as row M of T)
    const int *cptr, *cidx; const double *cval;   // rev: CSC of A
    const int *rptr, *ridx; const double *rval;   // rev: CSR of A
    // rev, refactorisation (bslv_lpq_set_refactor): rfx != 0 = an LP the pivot cross-check gives up is marked in BatchView::rmark (the call
    // rebuilds its inverse and solves it again); drift_b / drift_p: test hook BSLV_LP_REV_DRIFT, the cross-check of LP drift_b is taken as
    // failed at its drift_p-th pivot (-1: off)
    int rfx, drift_b, drift_p;
};
struct BatchView {
    const int *src, *dst;
    const double *vlo, *vup;
    int *status, *iters, *mode, *verified;    // verified: bit 0 = beta is fresh, bit 1 = the solve started with a variable on an artificial bound
    // Delayed update: up to KP pivots of an LP are SELECTED on vectors only (the pivot row and the entering column of the
    // tableau as it would be after the pending pivots, the reduced-cost row dcur, beta) and then applied to the tableau in
    // ONE pass (k_flush): a solve of <= KP pivots reads and writes its tableau once instead of once per pivot.
    int *npend, *flushed;       // pending pivots of the LP; has the tableau of this solve been written to its own slot yet
    PivDesc *desc;              // [B][KP]
    double *prow;               // [B][KP][ld]   pivot rows as they were when chosen
    double *pcol;               // [B][KP][Mp1p] multipliers f_i = (entering column)_i * p of every row i (0 for the pivot row)
    double *dcur;               // [B][ld]       reduced-cost row of the LP, up to date
    // Extended selection (k_select<true>): cost perturbation against dual degenerate stalling, primal clean-up afterwards
    double *dper;               // [B][ld]       perturbed reduced costs (the ratio tests use them while PF_PERT is set); while PF_PHASE1 is set: the phase-1 pricing vector d1
    int *pflags, *stall;        // PF_* bits; consecutive degenerate pivots
    const double *cvals;        // [B][ccnt] objective coefficients (objmode)
    int *xstat;                 // [8] of the batch: iterations with bound switches, perturbations, primal steps, removals that left wrong signs, switch iterations carried into beta without a pass; phase 1: LPs that entered it, its iterations, rebuilds of d1
    int *work, *nwork;      // LPs whose tableau k_flush passes over in a round (k_list_pending), their number per round
    // revised form
    double *trow;           // [B][ld]   the tableau row of the selection at hand (prow then holds rows of B^-1: [B][KP][ldt])
    double *uvec;           // [B][ldt]  -K_N x_N: beta = B^-1 uvec (k_rev_u; k_init and the refresh pass of k_flush multiply by it)
    double *xfull;          // [B][N]    scratch of k_rev_u: values of the nonbasic structurals by column
    int *rmark;             // [B]       revised form with LpView::rfx: 1 = given up by the pivot cross-check (zeroed per solve only while the switch is on)
    int *hmail;             // [B][8]    revised form, helper workgroups of k_select: request word, slices done, pending count, slice ticket
    int lazy;               // bslv_lpq_set_lazy: an LP that is finished when its pass would be due keeps its pending pivots; its slot gets the tableau only when asked for (bslv_lpq_materialise)
    unsigned long long *dbg; // BSLV_REV_PROBE & 8: 100 MHz clock ticks per phase of the dual selection of LP 0 (timing experiments)
};
// Devex pricing, dual (bslv_lpq_set_pricing) or primal (bslv_lpq_set_primal_pricing): what a batch keeps for its rule.  A view of its
// own, an argument of the priced kernels alone: two more pointers in BatchView move the argument segment of EVERY kernel that takes one
// (measured: other scratch sizes and scalar spills in k_select, k_select_p1 and k_select_cached), and the kernels of the default rule
// are to stay what they were.
enum { RULE_DVX = 1, RULE_PDV = 2 };      // the rule of a priced instance (k_select_priced); no instance carries both
struct NormView {
    // reference norms >= 1 (the square roots of the Devex weights), 1 in the reference framework.  DVX: [B][Mp1p], s_i of every basis row;
    // PDV: [B][ld], t_j of every nonbasic column POSITION j
    double *norm;
    // [3] of the batch: selections under the weighted rule; those whose row (DVX) / column (PDV) is not the one of the largest violation /
    // score; frameworks started anew after the start
    int *stat;
};

__device__ __forceinline__ double LO(const LpView &L, const BatchView &Bv, int b, int k)
{
    int j = k - L.vfirst;
    return (j >= 0 && j < L.vcnt) ? Bv.vlo[(size_t)b * L.vcnt + j] : L.lb[k];
}
__device__ __forceinline__ double UP(const LpView &L, const BatchView &Bv, int b, int k)
{
    int j = k - L.vfirst;
    return (j >= 0 && j < L.vcnt) ? Bv.vup[(size_t)b * L.vcnt + j] : L.ub[k];
}
__device__ __forceinline__ double btol(double bnd) { return TOL_BND * (1.0 + fabs(bnd)); }

// ---- k_prep: copy the small per-slot arrays src -> dst, sanitise nonbasic statuses against the
//      new bounds and set the nonbasic values (oracle/lp_dense.c sanitize()) ----
// The nonbasic status a DUAL start gives a variable (lo .. up) that the parent held at st with the reduced cost dj, and whether
// the dual simplex can start from it
__device__ __forceinline__ int dual_start_status(int st, double lo, double up, const double *drow, int j, int objmode)
{
    if (lo == up) st = NS_S;
    else if (isinf(lo) && isinf(up)) st = NS_F;
    else if (isinf(lo)) st = NS_U;
    else if (isinf(up)) st = NS_L;
    else {
        // boxed: sit at the bound that keeps the reduced cost dual feasible
        double dj = objmode ? 0.0 : drow[j];       // (new objective: stay where the parent was, that is primal feasible)
        if (dj < -TOL_DJ) st = NS_U;
        else if (dj > TOL_DJ) st = NS_L;
        else if (st != NS_L && st != NS_U) st = NS_L;
    }
    return st;
}
__device__ __forceinline__ bool dual_start_infeasible(int st, double dj) { return (st == NS_F && fabs(dj) > 1e-7) || (st == NS_L && dj < -1e-7) || (st == NS_U && dj > 1e-7); }
// ... and a PRIMAL start (bslv_lpq_set_method): the parent's side where the bounds still have it; an artificial bound is no place to
// start from (1e7 in x_N leaves 1e-9 of debris in beta), the variable starts on its own bound or, without one, free at zero
__device__ __forceinline__ int primal_start_status(int st, double lo, double up, unsigned char art)
{
    const bool nlo = isinf(lo) || (art & 1), nup = isinf(up) || (art & 2);
    if (lo == up) return NS_S;
    if (nlo && nup) return NS_F;
    if (nlo) return NS_U;
    if (nup) return NS_L;
    return (st == NS_L || st == NS_U) ? st : NS_L;
}
// METHOD: bslv_lpq_set_method's (objective batches: DUAL).  DUAL is the kernel as it always was; PRIMAL starts every LP as it stands,
// REPAIR the ones a DUAL start reports UNDEFINED -- both with PF_PRIMAL, the selection's phase 1 takes it from there.
template <int METHOD>
__global__ __launch_bounds__(NT) void k_prep(LpView L, BatchView Bv, int B)
{
    int b = blockIdx.x;
    if (b >= B) return;
    int src = Bv.src[b], dst = Bv.dst[b];
    const int *bh_s = L.bh + (size_t)src * L.M, *nh_s = L.nh + (size_t)src * L.N;
    const int *ns_s = L.nstat + (size_t)src * L.N, *pos_s = L.pos + (size_t)src * (L.M + L.N);
    int *bh_d = L.bh + (size_t)dst * L.M, *nh_d = L.nh + (size_t)dst * L.N;
    int *ns_d = L.nstat + (size_t)dst * L.N, *pos_d = L.pos + (size_t)dst * (L.M + L.N);
    double *xN_d = L.xN + (size_t)dst * L.ld;
    const double *drow_s = L.rev ? L.dsl + (size_t)src * L.ld : L.T + (size_t)src * L.slotT + (size_t)L.M * L.ld;
    if (src != dst) {
        for (int i = threadIdx.x; i < L.M; i += NT) bh_d[i] = bh_s[i];
        for (int i = threadIdx.x; i < L.M + L.N; i += NT) pos_d[i] = pos_s[i];
    }
    int dual_infeasible = 0, bigm = 0;     // bigm: a nonbasic variable sits on an artificial (+-1e7) bound
    bool primal_start = METHOD == BSLV_LP_METHOD_PRIMAL;
    if constexpr (METHOD == BSLV_LP_METHOD_REPAIR) {      // would the dual start below fail?  (asked first: in place, the loop below overwrites the parent's statuses)
        int bad = 0;
        for (int j = threadIdx.x; j < L.N; j += NT) {
            const int k = nh_s[j];
            if (dual_start_infeasible(dual_start_status(ns_s[j], LO(L, Bv, b, k), UP(L, Bv, b, k), drow_s, j, 0), drow_s[j])) bad = 1;
        }
        primal_start = __syncthreads_or(bad);
    }
    for (int j = threadIdx.x; j < L.ld; j += NT) {
        if (j >= L.N) { xN_d[j] = 0.0; continue; }
        int k = nh_s[j];
        double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k);
        int st = ns_s[j];
        if (METHOD != BSLV_LP_METHOD_DUAL && primal_start) st = primal_start_status(st, lo, up, L.art[k]);
        else {      // (dual_start_status and dual_start_infeasible, in the words the DUAL kernel was compiled from: its code stays what it was)
        if (lo == up) st = NS_S;
        else if (isinf(lo) && isinf(up)) st = NS_F;
        else if (isinf(lo)) st = NS_U;
        else if (isinf(up)) st = NS_L;
        else {
            // boxed: sit at the bound that keeps the reduced cost dual feasible
            double dj = L.objmode ? 0.0 : drow_s[j];       // (new objective: stay where the parent was, that is primal feasible)
            if (dj < -TOL_DJ) st = NS_U;
            else if (dj > TOL_DJ) st = NS_L;
            else if (st != NS_L && st != NS_U) st = NS_L;
        }
        // the dual simplex needs a dual feasible start: a bound that vanished under a non-zero
        // reduced cost cannot be repaired by a flip (the reference's GLPK would run its primal phase)
        {
            double dj = drow_s[j];
            if (!L.objmode && ((st == NS_F && fabs(dj) > 1e-7) || (st == NS_L && dj < -1e-7) || (st == NS_U && dj > 1e-7))) dual_infeasible = 1;
        }
        }
        { const unsigned char a = L.art[k]; if ((st == NS_L && (a & 1)) || (st == NS_U && (a & 2))) bigm = 1; }
        nh_d[j] = k;
        ns_d[j] = st;
        xN_d[j] = (st == NS_F) ? 0.0 : (st == NS_U ? up : lo);
    }
    {   // working copy of the reduced-cost row (k_select keeps it up to date between passes over the tableau)
        double *dc = Bv.dcur + (size_t)b * L.ld;
        if (!L.objmode) for (int j = threadIdx.x; j < L.ld; j += NT) dc[j] = j < L.N ? drow_s[j] : 0.0;
        else if (!L.rev) {
            // new objective: d_j = c_{nh[j]} + sum over the basic cost-carrying variables c_k T[row of k][j], from the parent's
            // tableau; it also becomes row M of the new slot (k_init takes beta_M = d . x_N from there)
            const double *Ts = L.T + (size_t)src * L.slotT;
            double *rowM = L.T + (size_t)dst * L.slotT + (size_t)L.M * L.ld;
            const double *cv = Bv.cvals + (size_t)b * L.ccnt;
            for (int j = threadIdx.x; j < L.ld; j += NT) {
                double v = 0.0;
                if (j < L.N) {
                    const int kj = nh_s[j] - L.cfirst;
                    if (kj >= 0 && kj < L.ccnt) v = cv[kj];
                    for (int t = 0; t < L.ccnt; t++) { const int pr = pos_s[L.cfirst + t]; if (pr >= 0) v = fma(cv[t], Ts[(size_t)pr * L.ld + j], v); }
                }
                dc[j] = v;
                rowM[j] = v;
            }
        }
        // (revised form with a new objective: a slot holds B^-1, M rows and no row M; the reduced costs are k_rev_price's, which runs next)
    }
    dual_infeasible = __syncthreads_or(dual_infeasible);
    bigm = __syncthreads_or(bigm);
    if (threadIdx.x == 0) {
        Bv.status[b] = dual_infeasible ? BSLV_LP_UNDEFINED : ST_RUNNING;
        Bv.iters[b] = 0;
        Bv.mode[b] = MODE_NONE;
        Bv.verified[b] = 1 | (bigm ? 2 : 0);   // k_init recomputes beta from scratch
        Bv.npend[b] = 0;
        Bv.pflags[b] = (L.objmode || (METHOD != BSLV_LP_METHOD_DUAL && primal_start)) ? PF_PRIMAL : 0;       // a new objective on a primal feasible basis: primal simplex steps (a primal start: phase 1 first where it is not feasible)
        Bv.stall[b] = 0;
        Bv.flushed[b] = (src == dst) || (L.objmode && !L.rev);      // (in place: the slot already holds the tableau; tableau form with a new objective: it is copied up front, see solve_batch; revised form: the first pass streams B^-1 from the parent, as for solve_batch)
    }
}

// ---- k_init: beta_dst = T_src . xN_dst, one wave per row, and the reduced-cost row T_dst[M] = T_src[M].  It starts the batches
//      k_init_grouped (below) has no instance for -- new objectives, rows of more than 2048 columns -- and every batch under
//      BSLV_INIT_GROUP=0; plan_init decides.  The rest of the
//      parent's tableau is NOT copied here: the first pivot of the solve reads the parent and writes the new slot
//      (k_flush), which saves one write and one read of the tableau per LP; solves without a pivot are copied by
//      k_copy_unpivoted at the end. ----
__global__ __launch_bounds__(NT) void k_init(LpView L, BatchView Bv, int B)
{
    int b = blockIdx.y;
    if (b >= B) return;
    int src = Bv.src[b], dst = Bv.dst[b];
    const double *Ts = L.T + (size_t)src * L.slotT;
    double *Td = L.T + (size_t)dst * L.slotT;
    const double *xN = L.rev ? Bv.uvec + (size_t)b * L.ldt : L.xN + (size_t)dst * L.ld;      // (rev: beta = B^-1 uvec, k_rev_u; beta[M] comes from there too)
    double *beta = L.beta + (size_t)dst * L.Mp1p;
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int ld2 = L.ldt >> 1;
    bool copy = (src != dst) && !L.rev;
    for (int rr = wave; rr < TR; rr += NT / WAVE) {
        int i = blockIdx.x * TR + rr;
        if (i >= L.mrows) break;
        const double2 *s = reinterpret_cast<const double2 *>(((L.objmode && i == L.M) ? Td : Ts) + (size_t)i * L.ldt);   // (objmode: k_prep wrote the new row M)
        double2 *d = reinterpret_cast<double2 *>(Td + (size_t)i * L.ldt);
        const double2 *x2 = reinterpret_cast<const double2 *>(xN);
        double acc = 0.0;
        for (int j2 = lane; j2 < ld2; j2 += WAVE) {
            double2 v = s[j2];
            double2 x = x2[j2];
            if (copy && i == L.M && !L.objmode) d[j2] = v;      // only the reduced-cost row: the first pass streams the rest from the parent (k_flush)
            acc = fma(v.x, x.x, acc);
            acc = fma(v.y, x.y, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) beta[i] = acc;
    }
}

// wave_sum of R values at once: on return a[0] of lane l holds the sum of value init_row_of_lane<R>(l), added up in wave_sum's own
// order.  The lanes l and l ^ o hold the same sum after wave_sum's step o, so each of the first log2(R) steps halves the number
// of values instead: a lane keeps the even value of a pair if its bit o is clear and the odd one if it is set, and gets the
// partner's half of the value it keeps.  8 values: 4 + 2 + 1 + 3 shuffles instead of 8 x 6.
template <int R>
__device__ __forceinline__ void wave_sum_rows(double (&a)[R], int lane)
{
    static_assert(R == 2 || R == 4 || R == 8, "two, four or eight values");
    auto halve = [&](auto n, int o) {
        const bool odd = (lane & o) != 0;
#pragma unroll
        for (int k = 0; k < decltype(n)::value / 2; k++) {
            const double keep = odd ? a[2 * k + 1] : a[2 * k], give = odd ? a[2 * k] : a[2 * k + 1];
            a[k] = keep + __shfl_xor(give, o, WAVE);
        }
    };
    if constexpr (R == 8) { halve(std::integral_constant<int, 8>{}, 32); halve(std::integral_constant<int, 4>{}, 16); halve(std::integral_constant<int, 2>{}, 8); }
    if constexpr (R == 4) { halve(std::integral_constant<int, 4>{}, 32); halve(std::integral_constant<int, 2>{}, 16); }
    if constexpr (R == 2) halve(std::integral_constant<int, 2>{}, 32);
#pragma unroll
    for (int o = 32 / R; o > 0; o >>= 1) a[0] += __shfl_xor(a[0], o, WAVE);
}
template <int R>
__device__ __forceinline__ int init_row_of_lane(int lane)      // (step o = 32 chose bit 0 of the value's index, o = 16 bit 1, o = 8 bit 2)
{
    int r = (lane >> 5) & 1;
    if (R >= 4) r |= ((lane >> 4) & 1) << 1;
    if (R >= 8) r |= ((lane >> 3) & 1) << 2;
    return r;
}

// ---- k_init_grouped: k_init for a batch whose LPs share a few parents (plan_init says which of the two runs).  The host has
//      sorted the batch by parent and cut every family into chunks of children (InitChunk); a workgroup takes one chunk and
//      4 x R rows of the parent, a wave R of them.  The wave reads its rows ONCE into registers -- lane l holds the entries
//      j2 = l, l + 64, ... of each row, the ones it touches in k_init -- and then walks the children of the chunk: x_N of the
//      child, the same fma chain per row as k_init, the same wave reduction (wave_sum_rows), beta of the child; row M goes
//      to the child's slot from the registers.  Per LP it reads and writes what k_init reads and writes, bit for bit; the
//      parent's tableau is read once per chunk instead of once per child.  EPL: double2 entries of a row per lane. ----
struct InitChunk { int first, cnt; };      // children order[first .. first + cnt) of the batch, all of one parent
template <int EPL, int R>
__global__ __launch_bounds__(NT) void k_init_grouped(LpView L, BatchView Bv, const int *__restrict__ order, const InitChunk *__restrict__ chunks)
{
    const InitChunk ch = chunks[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = (blockIdx.x * (NT / WAVE) + wave) * R;      // first row of this wave
    if (i0 >= L.mrows) return;
    const int ld2 = L.ldt >> 1;
    const int src = Bv.src[order[ch.first]];
    const double *Ts = L.T + (size_t)src * L.slotT;
    double2 v[R][EPL];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const double2 *s = reinterpret_cast<const double2 *>(Ts + (size_t)min(i0 + r, L.mrows - 1) * L.ldt);      // (rows past the last: loaded again, never written)
#pragma unroll
        for (int e = 0; e < EPL; e++) { const int j2 = lane + e * WAVE; v[r][e] = j2 < ld2 ? s[j2] : make_double2(0.0, 0.0); }
    }
    const int rowM = (!L.rev && L.M >= i0 && L.M < i0 + R) ? L.M - i0 : -1;      // the reduced-cost row is one of this wave's
    const int myrow = init_row_of_lane<R>(lane);
    const bool writer = (lane & (WAVE / R - 1)) == 0 && i0 + myrow < L.mrows;
    auto x_of = [&](int c) -> const double2 * {
        const int b = order[ch.first + c];
        return reinterpret_cast<const double2 *>(L.rev ? Bv.uvec + (size_t)b * L.ldt : L.xN + (size_t)Bv.dst[b] * L.ld);
    };
    double2 x[EPL], xn[EPL];
    {
        const double2 *x2 = x_of(0);
#pragma unroll
        for (int e = 0; e < EPL; e++) { const int j2 = lane + e * WAVE; xn[e] = j2 < ld2 ? x2[j2] : make_double2(0.0, 0.0); }
    }
    for (int c = 0; c < ch.cnt; c++) {
        const int dst = Bv.dst[order[ch.first + c]];
#pragma unroll
        for (int e = 0; e < EPL; e++) x[e] = xn[e];
        if (c + 1 < ch.cnt) {      // the next child's x_N is on its way while this one is multiplied
            const double2 *x2 = x_of(c + 1);
#pragma unroll
            for (int e = 0; e < EPL; e++) { const int j2 = lane + e * WAVE; xn[e] = j2 < ld2 ? x2[j2] : make_double2(0.0, 0.0); }
        }
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.0;
#pragma unroll
        for (int e = 0; e < EPL; e++)
            if (lane + e * WAVE < ld2) {      // (k_init's loop bound: a lane past the row's end adds nothing)
#pragma unroll
                for (int r = 0; r < R; r++) { acc[r] = fma(v[r][e].x, x[e].x, acc[r]); acc[r] = fma(v[r][e].y, x[e].y, acc[r]); }
            }
        wave_sum_rows<R>(acc, lane);
        if (writer) L.beta[(size_t)dst * L.Mp1p + i0 + myrow] = acc[0];
        if (rowM >= 0 && src != dst) {      // only the reduced-cost row: the first pass streams the rest from the parent (k_flush)
            double2 *d = reinterpret_cast<double2 *>(L.T + (size_t)dst * L.slotT + (size_t)L.M * L.ldt);
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r == rowM) {
#pragma unroll
                    for (int e = 0; e < EPL; e++) { const int j2 = lane + e * WAVE; if (j2 < ld2) d[j2] = v[r][e]; }
                }
        }
    }
}

// block-wide helpers (for the block they are called from: 4 waves with NT threads, 16 with NT_BIG)
__device__ __forceinline__ ValIdx block_argmax(ValIdx x, double *sv, int *si)
{
    x = wave_argmax(x);
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) { sv[wave] = x.v; si[wave] = x.i; }
    __syncthreads();
    ValIdx r{sv[0], si[0]};
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = better_max(r, ValIdx{sv[w], si[w]});
    return r;
}
__device__ __forceinline__ double block_max(double v, double *sv)
{
    v = wave_max(v);
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sv[wave] = v;
    __syncthreads();
    double r = sv[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = fmax(r, sv[w]);
    return r;
}
__device__ __forceinline__ double block_min(double v, double *sv)
{
    v = wave_min(v);
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sv[wave] = v;
    __syncthreads();
    double r = sv[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = fmin(r, sv[w]);
    return r;
}

// ---- k_select: dual simplex choice of (leaving row r, entering column q) for each running LP.
//      Same rules as oracle/lp_dense.c dual_simplex(): largest bound violation, Harris two-pass
//      ratio test with the largest |pivot| among the ties. ----
// THE RULES, each stated once for select_once and select_once_cached (below): the two differ in where a pivot's row and column state
// lives and in how loads are issued, never in a rule -- same pivots, same bits (tests/test_lp_select_cache_gpu.py).
// One pending pivot (1 / pivot element p, multiplier f of the entry's row, entry of the pivot row in its column) applied to one entry, as k_flush does
__device__ __forceinline__ double apply_pending(double v, bool is_pivot_row, bool is_pivot_col, double p, double f, double rowentry)
{
    if (is_pivot_row) return is_pivot_col ? p : -rowentry * p;
    return is_pivot_col ? f : fma(-f, rowentry, v);
}
// leaving row: largest bound violation (smallest variable id under Bland's rule); id = 2*i + (below ? 1 : 0)
__device__ __forceinline__ ValIdx leave_candidate(ValIdx best, double lo, double up, double bt, int k, int i, bool bland, int nvar)
{
    if (!isinf(lo)) { double v = lo - bt; if (v > btol(lo)) best = better_max(best, ValIdx{bland ? (double)(nvar - k) : v, 2 * i + 1}); }
    if (!isinf(up)) { double v = bt - up; if (v > btol(up)) best = better_max(best, ValIdx{bland ? (double)(nvar - k) : v, 2 * i}); }
    return best;
}
// ... under dual Devex pricing (bslv_lpq_set_pricing): largest violation over the row's reference norm s >= 1 -- with s == 1 the key is
// the violation itself, bit for bit (x / 1.0 is exact); Bland's rule does not look at s
__device__ __forceinline__ ValIdx leave_candidate_dvx(ValIdx best, double lo, double up, double bt, double s, int k, int i, bool bland, int nvar)
{
    if (!isinf(lo)) { double v = lo - bt; if (v > btol(lo)) best = better_max(best, ValIdx{bland ? (double)(nvar - k) : v / s, 2 * i + 1}); }
    if (!isinf(up)) { double v = bt - up; if (v > btol(up)) best = better_max(best, ValIdx{bland ? (double)(nvar - k) : v / s, 2 * i}); }
    return best;
}
// may a column of status st with the (signed) row entry a enter?
__device__ __forceinline__ bool is_candidate(int st, double a, double ptol) { return st != NS_S && !(fabs(a) < ptol) && ((a > 0 && (st == NS_L || st == NS_F)) || (a < 0 && (st == NS_U || st == NS_F))); }
__device__ __forceinline__ double harris_key(double d, double a, bool bland) { return (fabs(d) + (bland ? 0.0 : TOL_DJ)) / fabs(a); }
__device__ __forceinline__ bool within_bound(double d, double a, double th) { return fabs(d) / fabs(a) <= th; }

// entry (i, j) of the tableau as it is after the pending pivots 0..np-1, given its value v0 in the stored tableau
__device__ __forceinline__ double virt_entry(double v, int i, int j, int np, const PivDesc *pd, const double *prow, const double *pcol, int ld, int Mp1p)
{
    for (int s = 0; s < np; s++) {
        const PivDesc d = pd[s];
        const bool pr = i == d.r, pq = j == d.q;
        v = apply_pending(v, pr, pq, d.p, pr ? 0.0 : pcol[(size_t)s * Mp1p + i], pq ? 0.0 : prow[(size_t)s * ld + j]);
    }
    return v;
}

// revised form: entry (i, c) of B^-1 as it is after the pending pivots, given its stored value (no column swap: see LpView)
__device__ __forceinline__ double virt_entry_b(double v, int i, int c, int np, const PivDesc *pd, const double *prow, const double *pcol, int ldt, int Mp1p)
{
    for (int s = 0; s < np; s++) {
        const PivDesc d = pd[s];
        const bool pr = i == d.r;
        v = apply_pending(v, pr, false, d.p, pr ? 0.0 : pcol[(size_t)s * Mp1p + i], prow[(size_t)s * ldt + c]);
    }
    return v;
}
// revised form: uvec = -K_N x_N of LP b (one workgroup per LP), and beta[M] = d . x_N.  which: nullptr = every LP of the batch,
// else the work list of round `it` (only the LPs waiting for a refresh of beta are done).
__global__ __launch_bounds__(NT) void k_rev_u(LpView L, BatchView Bv, int B, const int *which, int it)
{
    __shared__ double sv[NT / WAVE];
    int b = blockIdx.x;
    if (which) { if (b >= Bv.nwork[it]) return; b = Bv.work[b]; if (Bv.mode[b] != MODE_REFRESH) return; }
    else if (b >= B) return;
    const int slot = Bv.dst[b], M = L.M, N = L.N;
    const int *nh = L.nh + (size_t)slot * N, *pos = L.pos + (size_t)slot * (M + N);
    const double *xN = L.xN + (size_t)slot * L.ld;
    double *xf = Bv.xfull + (size_t)b * N, *u = Bv.uvec + (size_t)b * L.ldt;
    for (int j = threadIdx.x; j < N; j += NT) xf[j] = 0.0;
    __syncthreads();
    double acc = 0.0;
    const double *dc = Bv.dcur + (size_t)b * L.ld;
    for (int j = threadIdx.x; j < N; j += NT) {
        const int k = nh[j];
        const double v = xN[j];
        if (k >= M) xf[k - M] = v;
        acc = fma(dc[j], v, acc);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L.ldt; i += NT) {
        double ui = 0.0;
        if (i < M) {
            const int p = pos[i];
            if (p < 0) ui = xN[-1 - p];                        // the auxiliary variable of row i is nonbasic: + e_i x_i
            for (int t = L.rptr[i]; t < L.rptr[i + 1]; t++) ui = fma(-L.rval[t], xf[L.ridx[t]], ui);
        }
        u[i] = -ui;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int w = 0; w < NT / WAVE; w++) t += sv[w]; L.beta[(size_t)slot * L.Mp1p + M] = t; }
}
// revised form: the reduced costs of every LP of the batch go to its slot (the tableau form has them in row M, which k_flush updates)
__global__ void k_rev_store_d(LpView L, BatchView Bv, int B)
{
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && j < L.ld) L.dsl[(size_t)Bv.dst[b] * L.ld + j] = Bv.dcur[(size_t)b * L.ld + j];
}
__global__ void k_rev_identity(LpView L, int slot, const double *cost)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < (size_t)L.M * L.ldt) { const int i = (int)(k / L.ldt), c = (int)(k % L.ldt); L.T[(size_t)slot * L.slotT + k] = i == c ? 1.0 : 0.0; }
    if (k < (size_t)L.ld) L.dsl[(size_t)slot * L.ld + k] = k < (size_t)L.N ? cost[k + 1] : 0.0;
}

// EXT = the extended selection, compiled in when the LP has boxed variables (two finite, non-artificial bounds):
//  * bound flipping ("long step") ratio test: the dual step passes the breakpoints of boxed candidates -- they switch to
//    their other bound instead of entering the basis -- for as long as the leaving row stays infeasible.  Without it every
//    boxed column with a zero reduced cost costs one degenerate pivot (hypercube rows of S-degenerate: hundreds of thousands);
//  * cost perturbation after STALL_LIMIT consecutive degenerate pivots (the ratio tests then use dper, every nonbasic reduced
//    cost moved 5e-7..1e-6 away from zero on its feasible side; the true reduced costs dcur are carried along);
//  * when the perturbed problem is solved the perturbation is taken away: boxed columns whose true reduced cost has the wrong
//    sign switch bound (dual simplex goes on), any other wrong sign is repaired by PRIMAL simplex pivots from the primal
//    feasible basis at hand (Dantzig pricing, Harris ratio test on the entering column) -- oracle/lp_dense.c does the same
//    with its primal_simplex().
// cap2 = capacity of the candidate arrays in dynamic LDS.
// (hash01: common.h)
// ---- revised form: the tableau row as sparse products, by slices that several workgroups take ----
// One sparse dot product per nonbasic column j in [j0, j1): row[j] = -rho[k] for a slack k = nh[j] < M, else -(rho . A_k) ... as the
// caller's sign convention has it (K = [I | -A]: the column of structural k is -A_k; cval holds -A).  The non-zeros of a column are fetched
// EIGHT at a time with independent loads (index, value, then the gathers from rho) and two columns are in flight per thread: entry after
// entry, each a chain of three dependent loads, cost 0.7 ms per selection on ex09 (37 000 columns, one workgroup).
// Slice t of ns takes the columns t, t + ns, t + 2 ns, ...: the few dense columns sit next to each other in the list and would all fall to one slice of a contiguous split.
constexpr int REV_HQ = 512;                        // places in rev_row_slice's queue of heavy columns
// (XS: the DVX instances of the selection hand in the LDS of the queue, xq[REV_HQ + 1] -- see SelSharedDvx -- and leave the others' alone)
template <bool XS = false>
__device__ __forceinline__ void rev_row_slice(const LpView &L, const double *brow, const int *nh, double *row, int t_sl, int ns_sl, int *xq = nullptr)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, M = L.M, N = L.N;
    constexpr int RU = 8;
    auto dot8 = [&](int beg, int end) -> double {
        double v = 0.0;
        for (int t0 = beg; t0 < end; t0 += RU) {
            int ix[RU]; double va[RU], rh[RU];
#pragma unroll
            for (int u = 0; u < RU; u++) { const bool in = t0 + u < end; ix[u] = in ? L.cidx[t0 + u] : 0; va[u] = in ? L.cval[t0 + u] : 0.0; }
#pragma unroll
            for (int u = 0; u < RU; u++) rh[u] = brow[ix[u]];
#pragma unroll
            for (int u = 0; u < RU; u++) v = fma(rh[u], va[u], v);
        }
        return v;
    };
    // A column with many non-zeros (ex09: 75 of its 36 939 columns hold 512 or 1024, the others 2 or 4) is not one thread's to sum -- 128
    // rounds of dependent loads, 150 us, while the other 1023 threads of the workgroup wait: it goes to a queue in LDS and a whole wave
    // takes it, 64 non-zeros per round.
    constexpr int HEAVY = 32, HQ = REV_HQ;
    int *p_hq, *p_hq_n;
    if constexpr (XS) { p_hq = xq; p_hq_n = xq + HQ; }
    else { __shared__ int hq[HQ]; __shared__ int hq_n; p_hq = hq; p_hq_n = &hq_n; }
    int *const hq = p_hq; int &hq_n = *p_hq_n;
    if (tid == 0) hq_n = 0;
    __syncthreads();
    const int j1 = L.ld;
    for (int i = tid; t_sl + ns_sl * i < j1; i += 2 * NT) {
        const int j = t_sl + ns_sl * i, j2 = t_sl + ns_sl * (i + NT);
        const int k1 = j < N ? nh[j] : -1, k2 = (j2 < j1 && j2 < N) ? nh[j2] : -1;
        int b1 = k1 >= M ? L.cptr[k1 - M] : 0, e1 = k1 >= M ? L.cptr[k1 - M + 1] : 0;
        int b2 = k2 >= M ? L.cptr[k2 - M] : 0, e2 = k2 >= M ? L.cptr[k2 - M + 1] : 0;
        bool q1 = false, q2 = false;
        if (e1 - b1 > HEAVY) { const int s = atomicAdd(&hq_n, 1); if (s < HQ) { hq[s] = j; q1 = true; e1 = b1; } }
        if (e2 - b2 > HEAVY) { const int s = atomicAdd(&hq_n, 1); if (s < HQ) { hq[s] = j2; q2 = true; e2 = b2; } }
        double v1 = (k1 >= 0 && k1 < M) ? -brow[k1] : 0.0, v2 = (k2 >= 0 && k2 < M) ? -brow[k2] : 0.0;
        if (e1 - b1 <= RU && e2 - b2 <= RU) {             // (the usual case: both columns in one round of loads)
            int ix[2 * RU]; double va[2 * RU], rh[2 * RU];
#pragma unroll
            for (int u = 0; u < RU; u++) {
                const bool i1 = b1 + u < e1, i2 = b2 + u < e2;
                ix[u] = i1 ? L.cidx[b1 + u] : 0; va[u] = i1 ? L.cval[b1 + u] : 0.0;
                ix[RU + u] = i2 ? L.cidx[b2 + u] : 0; va[RU + u] = i2 ? L.cval[b2 + u] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 2 * RU; u++) rh[u] = brow[ix[u]];
#pragma unroll
            for (int u = 0; u < RU; u++) { v1 = fma(rh[u], va[u], v1); v2 = fma(rh[RU + u], va[RU + u], v2); }
        } else { v1 += dot8(b1, e1); v2 += dot8(b2, e2); }
        if (!q1) row[j] = v1;
        if (j2 < j1 && !q2) row[j2] = v2;
    }
    __syncthreads();
    {
        const int nq = min(hq_n, HQ), lane = tid & (WAVE - 1), wv = tid / WAVE, nwv = NT / WAVE;
        for (int s = wv; s < nq; s += nwv) {
            const int j = hq[s], k = nh[j];
            const int beg = L.cptr[k - M], end = L.cptr[k - M + 1];
            double v = 0.0;
            for (int t0 = beg + lane; t0 < end; t0 += 4 * WAVE) {       // (four rounds in flight)
                int ix[4]; double va[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int t = t0 + u * WAVE; const bool in = t < end; ix[u] = in ? L.cidx[t] : 0; va[u] = in ? L.cval[t] : 0.0; }
#pragma unroll
                for (int u = 0; u < 4; u++) v = fma(brow[ix[u]], va[u], v);
            }
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
            if (lane == 0) row[j] = v;
        }
    }
    __syncthreads();
}
// ---- revised form, new objective (solve_batch_obj): the reduced-cost row of LP b.  In the tableau form k_prep sums the parent's
//      tableau rows, d_j = c[nh_j] + sum_t c_t T[pos(cfirst + t)][j]; here T[r][j] = -rho_r . K[nh_j], so the same row is ONE tableau
//      row built from a synthesised rho:  d_j = c[nh_j] - y . K[nh_j],  y = sum over the basic cost-carrying t of c_t rho_pos(cfirst + t)
//      (rows of the PARENT's B^-1: the slot the first pass streams from).  Grid (column slices, B); slice t takes the columns t, t + ns,
//      ... as rev_row_slice's other callers do, so the dense columns spread over the slices. ----
__device__ __forceinline__ void rev_price_y(const LpView &L, const BatchView &Bv, const int b, double *y)
{
    const int *pos = L.pos + (size_t)Bv.dst[b] * (L.M + L.N);         // (k_prep copied the parent's heads)
    const double *Binv = L.T + (size_t)Bv.src[b] * L.slotT;
    const double *cv = Bv.cvals + (size_t)b * L.ccnt;
    for (int c = threadIdx.x; c < L.ldt; c += blockDim.x) {
        double v = 0.0;
        if (c < L.M) for (int t = 0; t < L.ccnt; t++) { const int pr = pos[L.cfirst + t]; if (pr >= 0) v = fma(cv[t], Binv[(size_t)pr * L.ldt + c], v); }
        y[c] = v;
    }
}
// y of every LP into its scratch vector uvec (free until k_rev_u): where y does not fit in k_rev_price's LDS
__global__ __launch_bounds__(NT) void k_rev_y(LpView L, BatchView Bv, int B)
{
    const int b = blockIdx.x;
    if (b < B) rev_price_y(L, Bv, b, Bv.uvec + (size_t)b * L.ldt);
}
// y_lds: every workgroup forms y of its LP in LDS (ldt doubles of dynamic LDS), else it reads the one k_rev_y left in uvec
__global__ __launch_bounds__(NT) void k_rev_price(LpView L, BatchView Bv, int B, int y_lds)
{
    extern __shared__ double s_y[];
    const int b = blockIdx.y;
    if (b >= B) return;
    const double *y = Bv.uvec + (size_t)b * L.ldt;
    if (y_lds) { rev_price_y(L, Bv, b, s_y); __syncthreads(); y = s_y; }
    const int *nh = L.nh + (size_t)Bv.dst[b] * L.N;
    double *dc = Bv.dcur + (size_t)b * L.ld;
    rev_row_slice(L, y, nh, dc, blockIdx.x, gridDim.x);        // dc[j] = -(y . K[nh_j]), 0 on the padding (barrier at its end)
    const double *cv = Bv.cvals + (size_t)b * L.ccnt;
    for (int j = blockIdx.x + gridDim.x * threadIdx.x; j < L.N; j += gridDim.x * blockDim.x) {
        const int kj = nh[j] - L.cfirst;
        if (kj >= 0 && kj < L.ccnt) dc[j] += cv[kj];
    }
}
constexpr int REV_PRICE_SLICE = 2 * NT;             // columns per slice of k_rev_price (two per thread, one round of rev_row_slice)
// ---- an OBJECTIVE batch under a method (bslv_lpq_solve_batch_obj_method, DUAL and REPAIR), both forms: the dual start.  When these
//      kernels run the LP has the start of solve_batch_obj -- k_prep's objective mode: every nonbasic variable on its NATURAL side (the
//      parent's, sanitised against the bounds), PF_PRIMAL -- and its new reduced-cost row d in dcur (tableau form: k_prep; revised form:
//      k_rev_price, which is why the sides can only be chosen now).  The basis is made dual feasible for d: every nonbasic variable goes to
//      the side d_j wants, and the LP runs dual simplex steps (pflags 0); k_init (revised form: k_rev_u first) forms beta from the values
//      left here.
//      ARTIFICIAL BOUNDS of the call (oracle/lp_dense.c olp_solve does the same per LP): the engine of an objective batch has a zero cost
//      and none of its own.  k_obj_art gives a variable outside the per-LP range -+BIG on the side some LP of the batch needs and the
//      variable lacks (d_j > TOL_DJ without a lower, d_j < -TOL_DJ without an upper bound), in the call's own copy of lb / ub / art, which
//      every later kernel of the call sees in place of the engine's (solve_batch_impl).  They count as bounds as the engine's own do in
//      solve_batch: a start on one sets bit 1 of `verified`, a conclusion on one is UNBOUNDED (conclude_optimal).  An LP that needs none
//      never meets one: no natural side is artificial, and only a variable that needed the bound is put there.
//      An LP with a variable no side makes dual feasible (a variable of the per-LP range without the bound its d_j wants): UNDEFINED
//      under DUAL; under REPAIR its primal start stands, per LP.
//      xstat[8..10]: LPs started dual, nonbasic variables moved off their natural side, LPs REPAIR left to the primal start. ----
__device__ __forceinline__ int obj_dual_side(int natural, double lo, double up, double dj)
{
    if (natural == NS_S) return NS_S;
    if (dj > TOL_DJ && !isinf(lo)) return NS_L;
    if (dj < -TOL_DJ && !isinf(up)) return NS_U;
    return natural;
}
// art: the call's copy as 32-bit words (M + N bytes, rounded up), lb / ub: the call's copies
__global__ __launch_bounds__(NT) void k_obj_art(LpView L, BatchView Bv, int B, unsigned *art, double *lb, double *ub)
{
    const int b = blockIdx.x;
    if (b >= B) return;
    const int *nh = L.nh + (size_t)Bv.dst[b] * L.N;
    const double *dc = Bv.dcur + (size_t)b * L.ld;
    for (int j = threadIdx.x; j < L.N; j += NT) {
        const int k = nh[j];
        if (k >= L.vfirst && k < L.vfirst + L.vcnt) continue;
        const double lo = L.lb[k], up = L.ub[k], v = dc[j];
        if (lo == up) continue;
        if (v > TOL_DJ && isinf(lo)) { atomicOr(art + (k >> 2), 1u << (8 * (k & 3))); lb[k] = -BIG; }
        if (v < -TOL_DJ && isinf(up)) { atomicOr(art + (k >> 2), 2u << (8 * (k & 3))); ub[k] = BIG; }
    }
}
template <int METHOD>
__global__ __launch_bounds__(NT) void k_obj_start(LpView L, BatchView Bv, int B)
{
    const int b = blockIdx.x;
    if (b >= B) return;
    const int dst = Bv.dst[b];
    const int *nh = L.nh + (size_t)dst * L.N;
    int *ns = L.nstat + (size_t)dst * L.N;
    double *xN = L.xN + (size_t)dst * L.ld;
    const double *dc = Bv.dcur + (size_t)b * L.ld;
    int bad = 0;
    for (int j = threadIdx.x; j < L.N; j += NT) {
        const int k = nh[j];
        const double v = dc[j];
        if (dual_start_infeasible(obj_dual_side(ns[j], LO(L, Bv, b, k), UP(L, Bv, b, k), v), v)) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (bad) {      // (REPAIR: the primal start stands)
        if (threadIdx.x == 0) { if (METHOD == BSLV_LP_METHOD_DUAL) Bv.status[b] = BSLV_LP_UNDEFINED; else atomicAdd(&Bv.xstat[10], 1); }
        return;
    }
    int bigm = 0, moved = 0;
    for (int j = threadIdx.x; j < L.N; j += NT) {
        const int k = nh[j], natural = ns[j];
        const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k);
        const unsigned char a = L.art[k];
        const int st = obj_dual_side(natural, lo, up, dc[j]);
        if (st == natural) continue;
        moved++;
        if ((st == NS_L && (a & 1)) || (st == NS_U && (a & 2))) bigm = 1;
        ns[j] = st;
        xN[j] = st == NS_U ? up : lo;
    }
    if (moved) atomicAdd(&Bv.xstat[9], moved);
    bigm = __syncthreads_or(bigm);
    if (threadIdx.x == 0) { Bv.pflags[b] = 0; Bv.verified[b] = 1 | (bigm ? 2 : 0); atomicAdd(&Bv.xstat[8], 1); }
}

// The slices of a row are dealt by a ticket (hmail[3]) to whoever asks: the LP's own workgroup and its helpers -- workgroups of the same
// k_select launch (blockIdx.y > 0) that do nothing but wait for a request.  ONE workgroup per LP is what a selection is, and on ex09 the
// products over 36 865 columns were 300 of its 450 us.  Nothing waits for a workgroup that is not running: a slice nobody else took is
// taken by the LP's own workgroup, so helpers that the chip has no room for (or that gave up waiting) only cost their share.
// hmail[0]: request word = launch_id << 8 | n (n-th request of this launch; 0xFF: the launch is over), [1]: slices done, [2]: pending
// pivots of the request (which row of prow holds rho), [3]: slice ticket.  Device-scope release / acquire around every hand-over: the
// workgroups of one LP sit on different XCDs, each with its own L2.
constexpr int REV_SLICE = 2048;                    // columns per slice (two per thread of a 1024-thread workgroup)
__device__ __forceinline__ int rev_nslices(const LpView &L) { return (L.ld + REV_SLICE - 1) / REV_SLICE; }
// (XS: the DVX instances of the selection hand in the LDS word for the ticket, with the late flag and rev_row_slice's queue behind it -- see SelSharedDvx -- and leave the others' alone)
template <bool XS>
__device__ __forceinline__ void rev_take_slices_in(const LpView &L, int *mb, const int n, const double *brow, const int *nh, double *row, unsigned long long *cnt, int *xt)
{
    int *p_t;
    if constexpr (XS) p_t = xt;
    else { __shared__ int l_t; p_t = &l_t; }
    int &s_t = *p_t;
    const int ns = rev_nslices(L);
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) {
            // a ticket of request n and of no other: a helper that comes back late from request n - 1 must not take (or use up) one of n's
            int v = __hip_atomic_load(&mb[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), t = -1;
            while ((v >> 16) == n && (v & 0xFFFF) < ns) {
                if (__hip_atomic_compare_exchange_strong(&mb[3], &v, v + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { t = v & 0xFFFF; break; }
            }
            s_t = t;
        }
        __syncthreads();
        const int t = s_t;
        if (t < 0) break;
        if (cnt && threadIdx.x == 0) *cnt += 1;
        rev_row_slice<XS>(L, brow, nh, row, t, ns, XS ? xt + 2 : nullptr);
        if (!(L.probe & 16)) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // (the slice is out before it is counted)
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(&mb[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ void rev_take_slices(const LpView &L, int *mb, const int n, const double *brow, const int *nh, double *row, unsigned long long *cnt = nullptr)
{
    rev_take_slices_in<false>(L, mb, n, brow, nh, row, cnt, nullptr);
}
// (XS: as rev_take_slices_in; xr: the request word and the ticket, xdyn: the kernel's dynamic LDS)
template <bool XS = false>
__device__ __forceinline__ void rev_helper(const LpView &L, const BatchView &Bv, const int b, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    int *p_req; unsigned char *dyn;
    if constexpr (XS) { p_req = xr; dyn = xdyn; }
    else { extern __shared__ unsigned char dyn_sel[]; __shared__ int l_req; p_req = &l_req; dyn = dyn_sel; }
    int &s_req = *p_req;
    int *mb = Bv.hmail + (size_t)b * 8;
    const int tid = threadIdx.x, NT = (int)blockDim.x;
    const int slot = Bv.dst[b];
    const int *nh = L.nh + (size_t)slot * L.N;
    double *srho = L.rho_off >= 0 ? reinterpret_cast<double *>(dyn + L.rho_off) : nullptr;
    int last = L.launch_id << 8;
    for (long spins = 0; spins < 20000000L; spins++) {          // (bounded: ~10 s; a helper that leaves is not missed, see above)
        if (tid == 0) s_req = __hip_atomic_load(&mb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (relaxed: an acquire here invalidates the L2 of the XCD on every poll, for everyone on it)
        __syncthreads();
        const int req = s_req;
        __syncthreads();
        if ((req >> 8) != L.launch_id || req == last) { __builtin_amdgcn_s_sleep(8); continue; }
        if ((req & 0xFF) == 0xFF) return;
        last = req;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (once per request: rho, the pending count and the heads as the LP's workgroup left them)
        const int np = __hip_atomic_load(&mb[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double *brow_g = Bv.prow + (size_t)b * KP * L.ldt + (size_t)np * L.ldt;
        if (srho) { for (int c = tid; c < L.ldt; c += NT) srho[c] = brow_g[c]; __syncthreads(); }
        if constexpr (XS) rev_take_slices_in<true>(L, mb, req & 0xFF, srho ? srho : brow_g, nh, Bv.trow + (size_t)b * L.ld, nullptr, xr + 1);
        else rev_take_slices(L, mb, req & 0xFF, srho ? srho : brow_g, nh, Bv.trow + (size_t)b * L.ld);
    }
}
// BSLV_REV_PROBE & 8: 100 MHz clock ticks per phase of the selections of LP 0, summed in Bv.dbg[k] (solve_batch_impl prints them)
__device__ __forceinline__ void phase_mark(const LpView &L, const BatchView &Bv, int b, int k, unsigned long long &t)
{
    if ((L.probe & 8) && b == 0) { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long tn = wall_clock64(); Bv.dbg[k] += tn - t; t = tn; } }
}
// The vectors of LP b as one selection sees them
struct SelCtx {
    const double *T0;            // the stored tableau of this solve: the parent's slot until the first pass has written its own (see k_init)
    double *beta, *xN; int *bh, *nh, *nstat, *pos;
    double *prow0, *pcol0;       // the pending pivots' rows and multipliers
    double *drow;                // the reduced costs (the true ones: a perturbation has a row of its own, dper)
    double *row;                 // the pivot row as it is after the pending pivots, where k_flush will read it (revised form: k_flush reads the row of B^-1 from there, and the tableau row lives in a scratch vector of the LP)
    double *pc;                  // the multipliers of the rows (primal selection: first the entering column itself)
    const PivDesc *pd; int np, b;
};
__device__ __forceinline__ SelCtx sel_ctx(const LpView &L, const BatchView &Bv, int b, int np, int slot, int stored_slot)
{
    SelCtx c;
    c.T0 = L.T + (size_t)stored_slot * L.slotT;
    c.beta = L.beta + (size_t)slot * L.Mp1p; c.xN = L.xN + (size_t)slot * L.ld;
    c.bh = L.bh + (size_t)slot * L.M; c.nh = L.nh + (size_t)slot * L.N;
    c.nstat = L.nstat + (size_t)slot * L.N; c.pos = L.pos + (size_t)slot * (L.M + L.N);
    c.prow0 = Bv.prow + (size_t)b * KP * L.ldt; c.pcol0 = Bv.pcol + (size_t)b * KP * L.Mp1p;
    c.drow = Bv.dcur + (size_t)b * L.ld; c.row = L.rev ? Bv.trow + (size_t)b * L.ld : c.prow0 + (size_t)np * L.ld;
    c.pc = c.pcol0 + (size_t)np * L.Mp1p; c.pd = Bv.desc + (size_t)b * KP;
    c.np = np; c.b = b; return c;
}
// No row violates a bound: optimal, or unbounded on an active artificial bound.  Beta is recomputed first (a full read of the tableau) unless
// it is fresh or this solve made only a few pivots since k_init computed it (rank-1 updates: ~1e-15 against tolerances of 1e-9; not after a start on an artificial bound, 1e7 leaves debris of 1e-9)
__device__ __forceinline__ void conclude_optimal(const LpView &L, const BatchView &Bv, const SelCtx &c, const int iters, const int verified, const int nt, double *sv)
{
    const int tid = threadIdx.x, b = c.b;
    if (!(verified & 1) && (iters > REFRESH_AFTER || (verified & 2))) { if (tid == 0) Bv.mode[b] = MODE_REFRESH; return; }      // k_flush applies what is pending and recomputes beta
    double flag = 0.0;
    for (int j = tid; j < L.N; j += nt) {
        int st = c.nstat[j];
        unsigned char a = L.art[c.nh[j]];
        if (((st == NS_L && (a & 1)) || (st == NS_U && (a & 2))) && fabs(c.drow[j]) > TOL_DJ) flag = 1.0;
    }
    flag = block_max(flag, sv);
    if (tid == 0) { Bv.status[b] = flag > 0.0 ? BSLV_LP_UNBOUNDED : BSLV_LP_OPTIMAL; Bv.mode[b] = MODE_NONE; }
}
// No entering candidate: primal infeasible -- unless the violation is rounding debris in beta: recompute it first
// (r, below, np: the row at hand, for the ray record)
__device__ __forceinline__ void conclude_infeasible(const BatchView &Bv, const int b, const int verified, const int r, const bool below, const int np)
{
    if (threadIdx.x == 0) { if (!(verified & 1)) Bv.mode[b] = MODE_REFRESH; else { Bv.status[b] = BSLV_LP_INFEASIBLE; Bv.mode[b] = MODE_NONE; Bv.stall[b] = ray_record(RAY_ROW, r, np, below); } }
}
__device__ __noinline__ void trace_pivot(int b, int iters, bool primal, int r, int kb, bool below, double viol, int q, int kn, double trq, double dq, int nflip, double obj, bool bland, bool perturbed)
{
    printf("lp %d it %d%s r %d (var %d, %s by %.3e) q %d (var %d) alpha %.3e d %.3e step %.3e flips %d obj %.12g%s%s\n", b, iters, primal ? " primal" : "", r, kb, below ? "below" : "above", viol, q, kn, trq, dq, fabs(dq / trq), nflip, obj, bland ? " bland" : "", perturbed ? " perturbed" : "");
}
// Phase C, by ONE thread: descriptor of the pivot (r, q), basis heads, the leaving variable's new status (dwork, primal, nflip, perturbed: trace line only)
__device__ __forceinline__ PivDesc commit_pivot(const LpView &L, const BatchView &Bv, const SelCtx &c, const int r, const int q, const bool below, const bool bland,
                                                const int iters, const int verified, const int mode, const double *dwork, const bool primal, const int nflip, const bool perturbed)
{
    const int b = c.b;
    int kb = c.bh[r], kn = c.nh[q];
    double lo = LO(L, Bv, b, kb), up = UP(L, Bv, b, kb);
    double target = below ? lo : up, trq = c.row[q], br = c.beta[r];
    PivDesc d;
    d.r = r; d.q = q; d.p = 1.0 / trq; d.pbeta = br - target; d.enter_val = c.xN[q] + (target - br) / trq;
    Bv.desc[(size_t)b * KP + c.np] = d;
    c.bh[r] = kn; c.nh[q] = kb;
    c.pos[kn] = r; c.pos[kb] = -1 - q;
    if (lo == up) { c.nstat[q] = NS_S; c.xN[q] = lo; }
    else if (below) { c.nstat[q] = NS_L; c.xN[q] = lo; }
    else { c.nstat[q] = NS_U; c.xN[q] = up; }
    if (L.trace == b && (iters < 300 || iters % 997 == 0)) trace_pivot(b, iters, primal, r, kb, below, below ? lo - br : br - up, q, kn, trq, dwork[q], nflip, c.beta[L.M], bland, perturbed);
    Bv.mode[b] = mode; Bv.verified[b] = verified & 2; Bv.iters[b] = iters + 1;
    return d;
}

// ---- row r / column q of the tableau as it is after the pending pivots, by the whole workgroup (barriers inside) ----
__device__ __forceinline__ void fetch_row_tableau(const LpView &L, const SelCtx &c, const int r)
{
    for (int j = threadIdx.x; j < L.ld; j += (int)blockDim.x) c.row[j] = j < L.N ? virt_entry(c.T0[(size_t)r * L.ld + j], r, j, c.np, c.pd, c.prow0, c.pcol0, L.ld, L.Mp1p) : 0.0;
}
// revised form: rho = row r of B^-1, then one sparse product per column -- by this workgroup, or dealt in slices to it and its helpers.
// Two halves: rev_form_rho leaves rho of row r where the helpers look for it -- the place of the next pending row, prow0 + np * ldt, free
// until k_flush reads it as row np -- and in the LDS copy at L.rho_off when there is one, and returns the copy to gather from (brow);
// rev_row_of_rho makes the tableau row c.row[j] = -(rho . K[nh_j]) of whatever lies there.  The second half is shared with phase 1 of the revised form, whose pricing
// vector is the row of a synthesised rho (phase1_prepare), and it is the one place where the mailbox protocol of the helpers is stated.
// (XS: as rev_take_slices_in; xr: the request number, the late flag and the ticket, xdyn: the kernel's dynamic LDS)
template <bool XS = false>
__device__ __forceinline__ const double *rev_form_rho(const LpView &L, const SelCtx &c, const int r, unsigned char *xdyn = nullptr)
{
    unsigned char *dyn;
    if constexpr (XS) dyn = xdyn;
    else { extern __shared__ unsigned char dyn_sel[]; dyn = dyn_sel; }
    const int tid = threadIdx.x, NT = (int)blockDim.x, np = c.np, ldt = L.ldt;
    double *brow_g = c.prow0 + (size_t)np * ldt;
    // rho also goes to LDS when it fits (ex09: 37 KB): the sparse products below gather from it ~200 000 times per selection
    double *srho = L.rho_off >= 0 ? reinterpret_cast<double *>(dyn + L.rho_off) : nullptr;
    for (int i = tid; i < ldt; i += NT) {
        const double v = i < L.M ? virt_entry_b(c.T0[(size_t)r * ldt + i], r, i, np, c.pd, c.prow0, c.pcol0, ldt, L.Mp1p) : 0.0;
        brow_g[i] = v;
        if (srho) srho[i] = v;
    }
    __syncthreads();
    return srho ? srho : brow_g;
}
template <bool XS = false>
__device__ __forceinline__ void rev_row_of_rho(const LpView &L, const BatchView &Bv, const SelCtx &c, const double *brow, int *xr = nullptr)
{
    int *p_n, *p_late;
    if constexpr (XS) { p_n = xr; p_late = xr + 2; }
    else { __shared__ int l_n, l_late; p_n = &l_n; p_late = &l_late; }
    int &s_n = *p_n, &s_late = *p_late;
    const int tid = threadIdx.x, b = c.b, np = c.np;
    if (L.helpers <= 1) { rev_row_slice<XS>(L, brow, c.nh, c.row, 0, 1, XS ? xr + 3 : nullptr); return; }
    // hand the row out in slices (rev_take_slices): rho is in global memory (brow_g), the request goes out, this workgroup takes
    // slices like everyone else and then waits for the ones others took
    unsigned long long tf = ((L.probe & 8) && b == 0) ? wall_clock64() : 0ull;
    int *mb = Bv.hmail + (size_t)b * 8;
    __threadfence();
    __syncthreads();
    phase_mark(L, Bv, b, 8, tf);
    if (tid == 0) {
        const int old = __hip_atomic_load(&mb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int n = ((old >> 8) == L.launch_id ? (old & 0xFF) : 0) + 1;      // (at most 2 * KP requests per launch: far from 0xFF)
        s_n = n;
        __hip_atomic_store(&mb[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mb[2], np, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mb[3], n << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&mb[0], (L.launch_id << 8) | n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    phase_mark(L, Bv, b, 9, tf);
    if constexpr (XS) rev_take_slices_in<true>(L, mb, s_n, brow, c.nh, c.row, ((L.probe & 8) && b == 0) ? &Bv.dbg[13] : nullptr, xr + 1);
    else rev_take_slices(L, mb, s_n, brow, c.nh, c.row, ((L.probe & 8) && b == 0) ? &Bv.dbg[13] : nullptr);
    phase_mark(L, Bv, b, 10, tf);
    if (tid == 0) {
        const int ns = rev_nslices(L);
        long w = 0;
        while (__hip_atomic_load(&mb[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < ns && ++w < 50000000L) __builtin_amdgcn_s_sleep(2);      // (every slice counted here was taken by a workgroup that is running)
        s_late = w >= 50000000L;
    }
    __syncthreads();
    phase_mark(L, Bv, b, 11, tf);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (the slices the others wrote)
    phase_mark(L, Bv, b, 12, tf);
    if (s_late) { rev_row_slice<XS>(L, brow, c.nh, c.row, 0, 1, XS ? xr + 3 : nullptr); __syncthreads(); }      // (never seen; the row is this workgroup's to deliver either way)
}
template <bool XS = false>
__device__ __forceinline__ void fetch_row_revised(const LpView &L, const BatchView &Bv, const SelCtx &c, const int r, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    const double *brow = rev_form_rho<XS>(L, c, r, xdyn);
    rev_row_of_rho<XS>(L, Bv, c, brow, xr);
}
// (TABLEAU: an instance that never sees the revised form -- k_select_p1 -- leaves its code, and the LDS it declares, out)
template <bool TABLEAU = false, bool XS = false>
__device__ __forceinline__ void fetch_row(const LpView &L, const BatchView &Bv, const SelCtx &c, const int r, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    if (TABLEAU || !L.rev) fetch_row_tableau(L, c, r); else fetch_row_revised<XS>(L, Bv, c, r, xr, xdyn); __syncthreads();
}
__device__ __forceinline__ void fetch_col_tableau(const LpView &L, const SelCtx &c, const int q)
{
    for (int i = threadIdx.x; i < L.M; i += (int)blockDim.x) c.pc[i] = virt_entry(c.T0[(size_t)i * L.ld + q], i, q, c.np, c.pd, c.prow0, c.pcol0, L.ld, L.Mp1p);
}
// revised form: T[:, q] = -B^-1 K_kq
__device__ __forceinline__ void fetch_col_revised(const LpView &L, const SelCtx &c, const int q)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, M = L.M, ldt = L.ldt;
    double *pc = c.pc;
    const int kq = c.nh[q];
    const int cb = kq >= M ? L.cptr[kq - M] : 0, ce = kq >= M ? L.cptr[kq - M + 1] : 0;
    for (int i0 = tid; i0 < M; i0 += 2 * NT) {    // (B^-1 as stored) K_kq: two rows per thread, the gathers of eight non-zeros of each in flight together
        const int i1 = i0 + NT;
        const double *B0 = c.T0 + (size_t)i0 * ldt, *B1 = c.T0 + (size_t)(i1 < M ? i1 : i0) * ldt;
        double v0 = 0.0, v1 = 0.0;
        if (kq < M) { v0 = B0[kq]; v1 = B1[kq]; }
        else for (int t0 = cb; t0 < ce; t0 += 8) {
            double g0[8], g1[8], cv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const bool in = t0 + u < ce; const int k = in ? L.cidx[t0 + u] : 0; cv[u] = in ? L.cval[t0 + u] : 0.0; g0[u] = B0[k]; g1[u] = B1[k]; }
#pragma unroll
            for (int u = 0; u < 8; u++) { v0 = fma(-cv[u], g0[u], v0); v1 = fma(-cv[u], g1[u], v1); }
        }
        pc[i0] = v0;
        if (i1 < M) pc[i1] = v1;
    }
    for (int sp = 0; sp < c.np; sp++) {              // ... through the pending pivots, in order
        __syncthreads();
        const PivDesc d = c.pd[sp];
        const double vr = pc[d.r];
        __syncthreads();
        for (int i = tid; i < M; i += NT) pc[i] = i == d.r ? -d.p * vr : fma(-c.pcol0[(size_t)sp * L.Mp1p + i], vr, pc[i]);
    }
    __syncthreads();
    for (int i = tid; i < M; i += NT) pc[i] = -pc[i];
}
template <bool TABLEAU = false>
__device__ __forceinline__ void fetch_col(const LpView &L, const SelCtx &c, const int q)
{
    if (TABLEAU || !L.rev) fetch_col_tableau(L, c, q); else fetch_col_revised(L, c, q); __syncthreads();
}

// the perturbed reduced costs dp, from the true ones
__device__ __forceinline__ void apply_perturbation(const LpView &L, const SelCtx &c, double *dp)
{
    const int NT = (int)blockDim.x;
    for (int j = threadIdx.x; j < L.ld; j += NT) {
        double v = j < L.N ? c.drow[j] : 0.0;
        if (j < L.N) {
            const int st = c.nstat[j];
            const double eps = 5e-7 * L.pert_scale * (1.0 + hash01(c.nh[j]));
            if (st == NS_L) v = fmax(v, 0.0) + eps;
            else if (st == NS_U) v = fmin(v, 0.0) - eps;
        }
        dp[j] = v;
    }
    __syncthreads();
}
// The perturbed problem is solved: perturbation off (pf); true when wrong signs of the true reduced costs end this selection (primal steps or bound switches repair them)
// (P1: k_select_p1's instance reduces through sv -- __syncthreads_or keeps its word in LDS of its own, see SelShared)
template <bool P1 = false>
__device__ __forceinline__ bool perturbation_off(const LpView &L, const BatchView &Bv, const SelCtx &c, int &pf, double *sv = nullptr)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, b = c.b, N = L.N;
    int wrong1 = 0, wrongb = 0;
    for (int j = tid; j < N; j += NT) {
        const int st = c.nstat[j];
        const double v = c.drow[j];
        if ((st == NS_L && v < -TOL_DJ) || (st == NS_U && v > TOL_DJ) || (st == NS_F && fabs(v) > TOL_DJ)) {
            const int k = c.nh[j];
            if (st != NS_F && !isinf(LO(L, Bv, b, k)) && !isinf(UP(L, Bv, b, k)) && !L.art[k]) wrongb = 1; else wrong1 = 1;
        }
    }
    if constexpr (P1) { wrong1 = block_max(wrong1 ? 1.0 : 0.0, sv) > 0.0; wrongb = block_max(wrongb ? 1.0 : 0.0, sv) > 0.0; }
    else { wrong1 = __syncthreads_or(wrong1); wrongb = __syncthreads_or(wrongb); }
    pf &= ~PF_PERT;
    if (tid == 0 && (wrong1 || wrongb)) atomicAdd(&Bv.xstat[3], 1);
    if (wrong1) {
        if (tid == 0) { Bv.pflags[b] = pf | PF_PRIMAL; Bv.stall[b] = 0; if (L.trace == b) printf("lp %d it %d perturbation off -> primal clean-up\n", b, Bv.iters[b]); }
        return true;
    }
    if (tid == 0) Bv.pflags[b] = pf;
    if (wrongb) {
        for (int j = tid; j < N; j += NT) {
            const int st = c.nstat[j], k = c.nh[j];
            const double v = c.drow[j];
            if (st == NS_L && v < -TOL_DJ) { c.nstat[j] = NS_U; c.xN[j] = UP(L, Bv, b, k); }
            else if (st == NS_U && v > TOL_DJ) { c.nstat[j] = NS_L; c.xN[j] = LO(L, Bv, b, k); }
        }
        if (tid == 0) { Bv.mode[b] = MODE_REFRESH; Bv.verified[b] &= 2; if (L.trace == b) printf("lp %d it %d perturbation off -> bound switches\n", b, Bv.iters[b]); }
        return true;
    }
    return false;
}
// -1: the basic value bt is below its lower bound, +1: above its upper bound, 0: inside (oracle/lp_dense.c infeas_sign)
__device__ __forceinline__ int infeas_sign(double lo, double up, double bt)
{
    if (!isinf(lo) && bt < lo - btol(lo)) return -1;
    if (!isinf(up) && bt > up + btol(up)) return +1;
    return 0;
}
// Phase 1 of LP b, before a step: sg[i] = infeas_sign of row i (as a double; sg is the entering column's place, free until the column
// is fetched).  With an infeasible row the LP is in phase 1 (true) and d1[j] = sum_i sg_i T[i][j] prices it -- T as it is after the pending
// pivots.  d1 is rebuilt from the rows on entry, after a pass over the tableau (nothing pending) and when the last step moved a row
// other than the leaving one across a bound (PF_P1_STALE); between those it follows every pivot like the reduced costs do (select_once).
// REV (k_select_p1_rev: a slot holds B^-1 and no tableau row to walk): with T[i][j] = -rho_i . K[nh_j] the same vector is ONE tableau row,
// the one of the synthesised y1 = sum over the infeasible rows of sg_i rho_i (what rev_price_y does with the costs of an objective
// batch): d1[j] = -(y1 . K[nh_j]).  A thread owns columns of B^-1 and adds the rows in ascending order, so the reads of a row are
// coalesced and the sum has a fixed order; y1 lies where a pivot row's rho would (rev_form_rho) and its products take the pivot rows'
// path, helpers included (rev_row_of_rho).  They write the LP's scratch row (c.row, free until the step fetches its pivot row), from
// which d1 is copied.  The rebuild rule is the tableau form's.  (xr, xdyn: the LDS of the row fetch, see fetch_row_revised)
template <bool REV = false>
__device__ __forceinline__ bool phase1_prepare(const LpView &L, const BatchView &Bv, const SelCtx &c, int &pf, double *sg, double *d1, double *sv, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, b = c.b, M = L.M;
    int ninf = 0;
    for (int i = tid; i < M; i += NT) {
        const int k = c.bh[i];
        const int s = infeas_sign(LO(L, Bv, b, k), UP(L, Bv, b, k), c.beta[i]);
        sg[i] = (double)s;
        ninf |= s != 0;
    }
    ninf = block_max(ninf ? 1.0 : 0.0, sv) > 0.0;      // (its barriers also put sg in front of the whole workgroup)
    const int pf0 = pf;
    if (!ninf) {
        if (pf & PF_PHASE1) {      // feasible: phase 2, on the true reduced costs
            pf &= ~(PF_PHASE1 | PF_P1_STALE | PF_P1_KEEP);
            if (tid == 0) { Bv.pflags[b] = pf; Bv.stall[b] = 0; if (L.trace == b) printf("lp %d it %d phase 1 ends: primal feasible\n", b, Bv.iters[b]); }
        }
        return false;
    }
    const bool enter = !(pf & PF_PHASE1);
    if (enter || (pf & PF_P1_STALE) || (c.np == 0 && !(pf & PF_P1_KEEP))) {
        if constexpr (REV) {
            unsigned long long tp = ((L.probe & 8) && b == 0) ? wall_clock64() : 0ull;      // (BSLV_REV_PROBE & 8: clock ticks and number of LP 0's rebuilds in dbg[14], dbg[15])
            const int ldt = L.ldt;
            double *y_g = c.prow0 + (size_t)c.np * ldt;
            double *sy = L.rho_off >= 0 ? reinterpret_cast<double *>(xdyn + L.rho_off) : nullptr;
            for (int col = tid; col < ldt; col += NT) {
                double acc = 0.0;
                if (col < M)
                    for (int i = 0; i < M; i++) {
                        const double s = sg[i];
                        if (s != 0.0) acc += s * virt_entry_b(c.T0[(size_t)i * ldt + col], i, col, c.np, c.pd, c.prow0, c.pcol0, ldt, L.Mp1p);
                    }
                y_g[col] = acc;
                if (sy) sy[col] = acc;
            }
            __syncthreads();
            rev_row_of_rho<true>(L, Bv, c, sy ? sy : y_g, xr);
            __syncthreads();
            for (int j = tid; j < L.ld; j += NT) d1[j] = j < L.N ? c.row[j] : 0.0;
            phase_mark(L, Bv, b, 14, tp);
            if ((L.probe & 8) && b == 0 && tid == 0) Bv.dbg[15] += 1;
        } else
        for (int j = tid; j < L.ld; j += NT) {
            double acc = 0.0;
            if (j < L.N)
                for (int i = 0; i < M; i++) {
                    const double s = sg[i];
                    if (s != 0.0) acc += s * virt_entry(c.T0[(size_t)i * L.ld + j], i, j, c.np, c.pd, c.prow0, c.pcol0, L.ld, L.Mp1p);
                }
            d1[j] = acc;
        }
        if (tid == 0) {
            atomicAdd(&Bv.xstat[7], 1);
            if (!(pf & PF_P1_SEEN)) atomicAdd(&Bv.xstat[5], 1);
            if (enter && L.trace == b) printf("lp %d it %d phase 1 starts\n", b, Bv.iters[b]);
        }
        pf = (pf & ~(PF_PERT | PF_PERT_PENDING | PF_P1_STALE)) | PF_PHASE1 | PF_P1_SEEN;      // (phase 1 and a cost perturbation exclude each other: they share dper)
        if (enter && tid == 0) Bv.stall[b] = 0;
    }
    pf &= ~PF_P1_KEEP;
    if (pf != pf0 && tid == 0) Bv.pflags[b] = pf;
    __syncthreads();
    return true;
}
// Primal simplex step: true with the pivot (r, q), column in pc, row fetched; false: no pivot.  On the true reduced costs from a primal
// feasible basis (clean-up after a perturbation, new objectives) -- and, P1 (bslv_lpq_set_method), from any basis: while a basic variable
// is outside its bounds the step is one of PHASE 1, priced by d1 (phase1_prepare), with the SAME ratio test except that an infeasible
// basic variable blocks where it reaches the bound it violates and nowhere else (oracle/lp_dense.c primal_simplex).  rsig: infeas_sign
// the leaving variable had.
// (DVX: the instances of dual Devex pricing, which hand in the LDS of a row fetch -- see fetch_row_revised)
// (PDV: the instances of primal Devex pricing, bslv_lpq_set_primal_pricing -- see select_once.  They hand in their LDS as DVX does, and
//  the entering column is the eligible one with the largest score / t_j instead of the largest score; Bland's rule takes no notice)
// (P1R, with P1: the instance of k_select_p1_rev, phase 1 in the revised form -- rows and columns come from fetch_row / fetch_col's revised
//  variants, and it hands in the LDS of a row fetch as DVX does)
template <bool P1, bool DVX = false, bool PDV = false, bool P1R = false>
__device__ __forceinline__ bool primal_step(const LpView &L, const BatchView &Bv, const SelCtx &c, int &pf, const bool bland, double *sv, int *si,
                                            int &r, int &q, bool &below, double &pstep, int &rsig, int *xr = nullptr, unsigned char *xdyn = nullptr, const NormView *nv = nullptr)
{
    static_assert(!(DVX && PDV), "one rule per instance: nv holds the norms of one");
    const int tid = threadIdx.x, NT = (int)blockDim.x, b = c.b, M = L.M, N = L.N;
    const double *pc = c.pc;
    double *beta = c.beta;
    const double *dj = c.drow;               // what prices the step
    bool ph1 = false;
    if constexpr (P1) {
        double *d1 = Bv.dper + (size_t)b * L.ld;
        ph1 = phase1_prepare<P1R>(L, Bv, c, pf, c.pc, d1, sv, xr, xdyn);
        if (ph1) dj = d1;
    }
    ValIdx ent{0.0, -1};
    bool other_col = false;                  // primal Devex pricing: the weighted rule chose another column than the largest score's
    if constexpr (PDV) {
        // (four columns per thread with all loads issued first, as the passes of the dual selection; the column of the largest
        //  unweighted score is found beside it, for the statistics only: bslv_lpq_last_primal_pricing_stats)
        const double *tn = nv->norm + (size_t)b * L.ld;
        ValIdx plain{0.0, -1};
        constexpr int PU = 4;
        for (int j0 = tid; j0 < N; j0 += PU * NT) {
            int stv[PU]; double vv[PU], tv[PU];
#pragma unroll
            for (int u = 0; u < PU; u++) {
                const int j = j0 + u * NT;
                const bool in = j < N;
                stv[u] = in ? c.nstat[j] : NS_S; vv[u] = in ? dj[j] : 0.0; tv[u] = in ? tn[j] : 1.0;
            }
#pragma unroll
            for (int u = 0; u < PU; u++) {
                const int j = j0 + u * NT, st = stv[u];
                if (st == NS_S) continue;
                const double v = vv[u];
                double sc = 0.0;
                if (st == NS_L) { if (v < -TOL_DJ) sc = -v; }
                else if (st == NS_U) { if (v > TOL_DJ) sc = v; }
                else if (fabs(v) > TOL_DJ) sc = fabs(v);
                if (sc > 0.0) {
                    ent = better_max(ent, ValIdx{bland ? (double)(L.M + L.N - c.nh[j]) : sc / tv[u], j});      // (t == 1: sc / t is sc bit for bit)
                    plain = better_max(plain, ValIdx{sc, j});
                }
            }
        }
        ent = block_argmax(ent, sv, si);
        plain = block_argmax(plain, sv, si);
        other_col = !bland && ent.i != plain.i;
    } else {
    for (int j = tid; j < N; j += NT) {
        const int st = c.nstat[j];
        if (st == NS_S) continue;
        const double v = dj[j];
        double sc = 0.0;
        if (st == NS_L) { if (v < -TOL_DJ) sc = -v; }
        else if (st == NS_U) { if (v > TOL_DJ) sc = v; }
        else if (fabs(v) > TOL_DJ) sc = fabs(v);
        if (sc > 0.0) ent = better_max(ent, ValIdx{bland ? (double)(L.M + L.N - c.nh[j]) : sc, j});
    }
    ent = block_argmax(ent, sv, si);
    }
    if (ent.i < 0) {
        if (P1 && ph1) {
            // nothing lowers the sum of infeasibilities: primal infeasible -- on a recomputed beta (the pass leaves nothing pending: d1 is rebuilt too)
            if (tid == 0) {
                if (!(Bv.verified[b] & 1)) { Bv.mode[b] = MODE_REFRESH; Bv.pflags[b] = pf | PF_P1_STALE; }
                else { Bv.status[b] = BSLV_LP_INFEASIBLE; Bv.mode[b] = MODE_NONE; Bv.stall[b] = ray_record(RAY_P1, 0, c.np, false); }      // (sg is in c.pc, d1 in dper)
            }
            return false;
        }
        // dual feasible: the dual selection takes over again (it concludes, or repairs what rounding left infeasible)
        if (tid == 0) { Bv.pflags[b] = pf & ~PF_PRIMAL; Bv.stall[b] = 0; }
        return false;
    }
    if (Bv.iters[b] >= L.maxit) { if (tid == 0) { Bv.status[b] = BSLV_LP_UNDEFINED; Bv.mode[b] = MODE_NONE; } return false; }
    q = ent.i;
    if constexpr (PDV) if (tid == 0 && !bland) { atomicAdd(&nv->stat[0], 1); if (other_col) atomicAdd(&nv->stat[1], 1); }      // (a selection priced by the norms: it ends in a pivot, a bound switch or a ray)
    const int stq = c.nstat[q], kq = c.nh[q];
    const double dq = dj[q];
    const double dir = (stq == NS_U || (stq == NS_F && dq > 0.0)) ? -1.0 : 1.0;
    fetch_col<P1 && !P1R>(L, c, q);
    double cmax = 0.0;
    for (int i = tid; i < M; i += NT) cmax = fmax(cmax, fabs(pc[i]));
    cmax = block_max(cmax, sv);
    const double ptol = TOL_PIV * (1.0 + cmax);
    const double gap = UP(L, Bv, b, kq) - LO(L, Bv, b, kq);     // inf unless both bounds are finite
    double tmax = gap;
    for (int i = tid; i < M; i += NT) {
        const double a = pc[i] * dir;
        if (fabs(a) < ptol) continue;
        const int k = c.bh[i];
        const double bt = beta[i];
        int sg = 0;                          // (phase 1: below its lower bound it blocks there, coming from below, and not at the upper one; above likewise)
        if constexpr (P1) if (ph1) sg = infeas_sign(LO(L, Bv, b, k), UP(L, Bv, b, k), bt);
        if (a > 0) {
            if (P1 && sg < 0) { const double lo = LO(L, Bv, b, k); tmax = fmin(tmax, (lo + (bland ? 0.0 : btol(lo)) - bt) / a); }
            else if (!(P1 && sg > 0)) { const double up = UP(L, Bv, b, k); if (!isinf(up)) tmax = fmin(tmax, fmax(up + (bland ? 0.0 : btol(up)) - bt, 0.0) / a); }
        } else {
            if (P1 && sg > 0) { const double up = UP(L, Bv, b, k); tmax = fmin(tmax, (bt - up + (bland ? 0.0 : btol(up))) / -a); }
            else if (!(P1 && sg < 0)) { const double lo = LO(L, Bv, b, k); if (!isinf(lo)) tmax = fmin(tmax, fmax(bt - lo + (bland ? 0.0 : btol(lo)), 0.0) / -a); }
        }
    }
    tmax = block_min(tmax, sv);
    if (isinf(tmax)) {
        if (tid == 0) { Bv.status[b] = (P1 && ph1) ? BSLV_LP_UNEXPECTED : BSLV_LP_UNBOUNDED; Bv.mode[b] = MODE_NONE; Bv.stall[b] = ray_record(RAY_DIR, q, c.np, dir > 0.0); }      // (phase 1 has a bounded objective: the oracle says UNEXPECTED too)
        return false;
    }
    ValIdx lv{0.0, -1};
    for (int i = tid; i < M; i += NT) {
        const double a = pc[i] * dir;
        if (fabs(a) < ptol) continue;
        const int k = c.bh[i];
        const double bt = beta[i];
        int sg = 0;
        if constexpr (P1) if (ph1) sg = infeas_sign(LO(L, Bv, b, k), UP(L, Bv, b, k), bt);
        if (a > 0) {
            if (P1 && sg < 0) { const double lo = LO(L, Bv, b, k); if ((lo - bt) / a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(L.M + L.N - k) : a, 2 * i}); }
            else if (!(P1 && sg > 0)) { const double up = UP(L, Bv, b, k); if (!isinf(up) && (up - bt) / a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(L.M + L.N - k) : a, 2 * i + 1}); }
        } else {
            if (P1 && sg > 0) { const double up = UP(L, Bv, b, k); if ((bt - up) / -a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(L.M + L.N - k) : -a, 2 * i + 1}); }
            else if (!(P1 && sg < 0)) { const double lo = LO(L, Bv, b, k); if (!isinf(lo) && (bt - lo) / -a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(L.M + L.N - k) : -a, 2 * i}); }
        }
    }
    lv = block_argmax(lv, sv, si);
    double tstep = INFINITY;
    rsig = 0;
    if (lv.i >= 0) {
        const int i = lv.i >> 1, k = c.bh[i];
        const double a = pc[i] * dir;
        tstep = fmax(((lv.i & 1) ? UP(L, Bv, b, k) - beta[i] : beta[i] - LO(L, Bv, b, k)) / fabs(a), 0.0);
        if constexpr (P1) if (ph1) {
            rsig = infeas_sign(LO(L, Bv, b, k), UP(L, Bv, b, k), beta[i]);
            if (rsig) tstep = ((lv.i & 1) ? beta[i] - UP(L, Bv, b, k) : LO(L, Bv, b, k) - beta[i]) / fabs(a);      // (from outside to the bound it violates)
        }
    }
    if (lv.i < 0 || gap <= tstep) {
        // the entering variable reaches its own other bound first: no pivot
        __syncthreads();
        int moved = 0;                       // phase 1: a row crossed a bound (under the ratio test above none should)
        for (int i = tid; i < M; i += NT) {
            const double bn = fma(pc[i], dir * gap, beta[i]);
            if constexpr (P1) if (ph1) { const int k = c.bh[i]; const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k); moved |= infeas_sign(lo, up, beta[i]) != infeas_sign(lo, up, bn); }
            beta[i] = bn;
        }
        if constexpr (P1) if (ph1) {
            moved = block_max(moved ? 1.0 : 0.0, sv) > 0.0;
            pf = (pf | PF_P1_KEEP) | (moved ? PF_P1_STALE : 0);      // (no pivot: d1 stands as it is)
            if (tid == 0) { Bv.pflags[b] = pf; atomicAdd(&Bv.xstat[6], 1); }
        }
        if (tid == 0) {
            beta[M] = fma((P1 && ph1) ? c.drow[q] : dq, dir * gap, beta[M]);      // (the objective moves by the TRUE reduced cost)
            if (stq == NS_L) { c.nstat[q] = NS_U; c.xN[q] = UP(L, Bv, b, kq); } else { c.nstat[q] = NS_L; c.xN[q] = LO(L, Bv, b, kq); }
            if (L.trace == b) printf("lp %d it %d primal: column %d (var %d) d %.3e switches bound\n", b, Bv.iters[b], q, kq, dq);
            Bv.verified[b] &= 2;
            Bv.iters[b] += 1;
            atomicAdd(&Bv.xstat[2], 1);
        }
        return false;
    }
    r = lv.i >> 1;
    below = !(lv.i & 1);                   // the leaving variable goes to its lower bound
    pstep = fabs(dq) * tstep / (1.0 + fabs(beta[M]));      // (what the step moves the objective by, relative: the ratio test's tolerance gives a degenerate step a length of 1e-9, not 0)
    if constexpr (P1) if (ph1) { pstep = fabs(dq) * tstep; if (tid == 0) atomicAdd(&Bv.xstat[6], 1); }      // (phase 1: by how much the sum of infeasibilities falls)
    fetch_row<P1 && !P1R, DVX || PDV || P1R>(L, Bv, c, r, xr, xdyn);
    return true;
}
// Bound flipping ratio test: sorted breakpoints of row r; a boxed candidate switches bound (sflag) while the row stays infeasible.  Returns the number of switches (the first of sidx)
// (P1: the instance of k_select_p1, which hands in its counters -- see SelShared)
template <bool P1 = false>
__device__ __forceinline__ int flip_breakpoints(const LpView &L, const BatchView &Bv, const SelCtx &c, const int r, const bool below, const double sgn, const double ptol,
                                                const double *dwork, const int cap2, double *skey, int *sidx, unsigned char *sflag, int *cnt3 = nullptr)
{
    int *p_cnt, *p_nboxed, *p_stop;
    if constexpr (P1) { p_cnt = cnt3; p_nboxed = cnt3 + 1; p_stop = cnt3 + 2; }
    else { __shared__ int l_cnt, l_nboxed, l_stop; p_cnt = &l_cnt; p_nboxed = &l_nboxed; p_stop = &l_stop; }
    int &s_cnt = *p_cnt, &s_nboxed = *p_nboxed, &s_stop = *p_stop;
    const int tid = threadIdx.x, NT = (int)blockDim.x, b = c.b, N = L.N;
    const double *row = c.row;
    if (tid == 0) { s_cnt = 0; s_nboxed = 0; s_stop = 0; }
    for (int j = tid; j < N; j += NT) sflag[j] = 0;
    __syncthreads();
    if (cap2 > 0) for (int j = tid; j < N; j += NT) {
        int st = c.nstat[j];
        double a = sgn * row[j];
        if (is_candidate(st, a, ptol)) {
            const int at = atomicAdd(&s_cnt, 1);
            skey[at] = fabs(dwork[j]) / fabs(a);
            sidx[at] = j;
            const int k = c.nh[j];
            const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k);
            if (st != NS_F && !isinf(lo) && !isinf(up) && !L.art[k]) atomicAdd(&s_nboxed, 1);
        }
    }
    __syncthreads();
    const int C = s_cnt;
    if (s_nboxed == 0) return 0;              // nothing to flip at all
    int n2 = 2;
    while (n2 < C) n2 <<= 1;
    for (int i = C + tid; i < n2; i += NT) { skey[i] = INFINITY; sidx[i] = 0x7fffffff; }
    __syncthreads();
    // bitonic sort by (breakpoint, column): the order, and with it every decision below, is unique
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int i = tid; i < n2; i += NT) {
                const int x = i ^ jj;
                if (x > i) {
                    const double ka = skey[i], kb2 = skey[x];
                    const int ia = sidx[i], ib = sidx[x];
                    const bool gt = ka > kb2 || (ka == kb2 && ia > ib);
                    if (((i & kk) == 0) == gt) { skey[i] = kb2; skey[x] = ka; sidx[i] = ib; sidx[x] = ia; }
                }
            }
            __syncthreads();
        }
    if (tid == 0) {
        // walk the breakpoints
        const int kb0 = c.bh[r];
        double slope = below ? LO(L, Bv, b, kb0) - c.beta[r] : c.beta[r] - UP(L, Bv, b, kb0);
        int k = 0;
        for (; k < C; k++) {
            const int j = sidx[k], kv = c.nh[j];
            const double lo = LO(L, Bv, b, kv), up = UP(L, Bv, b, kv);
            if (c.nstat[j] == NS_F || isinf(lo) || isinf(up) || L.art[kv]) break;
            const double dec = (up - lo) * fabs(row[j]);
            if (slope - dec < 0.0) break;
            slope -= dec;
            sflag[j] = 1;
        }
        s_stop = k;
    }
    __syncthreads();
    return s_stop;
}
// The switches: other bound, other status.  A few: beta follows as a vector update over the nflip columns of the tableau as it is after the pending
// pivots, and the LP keeps selecting (true).  Many, or the revised form (a column is a product, not a gather): false, the caller asks for MODE_REFRESH.
// beta is recomputed from the tableau before any status is reported (verified), so the update cannot end in a result.
__device__ __forceinline__ bool switch_bounds(const LpView &L, const BatchView &Bv, const SelCtx &c, const int r, const int nflip, double *skey, const int *sidx)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, b = c.b, M = L.M;
    for (int k = tid; k < nflip; k += NT) {
        const int j = sidx[k], kv = c.nh[j];
        const double lo = LO(L, Bv, b, kv), up = UP(L, Bv, b, kv);
        if (c.nstat[j] == NS_L) { c.nstat[j] = NS_U; c.xN[j] = up; skey[k] = up - lo; }
        else { c.nstat[j] = NS_L; c.xN[j] = lo; skey[k] = lo - up; }
    }
    if (!(nflip > 0 && nflip <= FLIP_INCR_MAX && !L.rev)) return false;
    __syncthreads();
    for (int i = tid; i <= M; i += NT) {
        double acc = 0.0;
        for (int k = 0; k < nflip; k++) {
            const int j = sidx[k];
            const double t = i == M ? c.drow[j] : (i == r ? c.row[j] : virt_entry(c.T0[(size_t)i * L.ld + j], i, j, c.np, c.pd, c.prow0, c.pcol0, L.ld, L.Mp1p));
            acc = fma(t, skey[k], acc);
        }
        c.beta[i] += acc;
    }
    __syncthreads();
    return true;
}

// Workgroup: NT threads; NT_BIG for rows of 1536 columns and more (S-degenerate: 2011, ex09: 36 939) -- an LP's selection is a chain
// of passes over N entries by ONE workgroup, and four times the threads shorten every pass.
// ONE selection of LP b by the calling workgroup (every `return` below is taken by the whole workgroup).  Returns false when the LP
// cannot select again before the next pass over its tableau (finished, waiting for a refresh, KP pivots pending).
// P1 (with EXT): the primal steps include phase 1 (bslv_lpq_set_method; k_select_p1) -- an instance of its own, so that the kernels of
// the default method stay what they were.
// The LDS of a selection is declared where it is used, in select_once and flip_breakpoints, for the kernels that always were.  A device
// function that is not inlined and declares LDS is laid out per MODULE, though: one more kernel calling one (select_once_p1) would
// move the others' variables into a table looked up by kernel.  So k_select_p1 declares everything itself and hands it down.
struct SelShared { double sv[NT_BIG / WAVE]; int si[NT_BIG / WAVE]; PivDesc d; int cnt3[3]; unsigned char *dyn; };
// DVX: DUAL DEVEX PRICING (bslv_lpq_set_pricing; Forrest and Goldfarb's reference framework, dual form).  Every basis row i of the LP
// has a reference norm s_i >= 1 (NormView::norm; the square root of the usual weight), 1 in the reference framework: the basis the solve starts
// from.  Phase A takes the violated row with the largest violation / s_i (leave_candidate_dvx), and a dual pivot on row r with the
// multipliers f_i of Phase D (|f_i| = |alpha_iq / alpha_rq|) and p = 1 / alpha_rq leaves
//   s_i = max(s_i, |f_i| s_r)  (i != r),      s_r = max(s_r |p|, 1)
// in the loop that updates beta: no entry of the tableau is read for it.  A basis change that is no such dual step -- a primal clean-up
// or phase-1 pivot here, a refactorisation replay on the host side -- starts a new framework (all s_i = 1); bound switches change
// nothing.  Instances of their own (k_select_priced<RULE_DVX, ..>), so that the kernels of the default rule stay what they were; like P1
// they get their LDS handed down (SelSharedDvx: also the words of the revised form's row fetch).
struct SelSharedDvx : SelShared { int rv[3 + REV_HQ + 1]; };      // rv: request word of a helper / request number of the LP's own workgroup, slice ticket, late flag; rev_row_slice's queue and its length
// PDV: PRIMAL DEVEX PRICING (bslv_lpq_set_primal_pricing; the same framework, primal form).  Every nonbasic column position j of the LP
// has a reference norm t_j >= 1 (NormView::norm), 1 in the reference framework: the basis the solve starts from.  A primal step, of phase
// 1 or 2, takes the eligible column with the largest score / t_j (primal_step), and a primal pivot (r, q) with the pivot row alpha_r that
// fetch_row has just produced leaves
//   t_j = max(t_j, |alpha_rj / alpha_rq| t_q)  (j != q),      t_q = max(t_q / |alpha_rq|, 1)   (position q now holds the leaving variable)
// in one more pass over the row: no further entry of the tableau is read for it.  The norms do not depend on the cost, so phase 1 and
// phase 2 share them.  A dual pivot of the LP here, a refactorisation replay on the host side, start a new framework (all t_j = 1); bound
// switches change nothing.  Instances of their own again (k_select_priced<RULE_PDV, ..>), which take the LDS of the DVX ones; no
// instance carries both rules.
// P1R (with P1): phase 1 in the revised form (bslv_lpq_solve_batch_method; k_select_p1_rev) -- and, with DVX or PDV, under the rule of one
// call (bslv_lpq_solve_batch_method_priced; k_select_priced_p1_rev<RULE>).  P1 alone stays the tableau form's instance, with the revised
// form's code left out (TAB below).
template <bool EXT, bool P1 = false, bool DVX = false, bool PDV = false, bool P1R = false>
__device__ __forceinline__ bool select_once(const LpView &L, const BatchView &Bv, const int b, const int cap2, SelShared *xs = nullptr, const NormView *nv = nullptr)
{
    static_assert(EXT || !P1, "phase 1 lives in the extended selection");
    static_assert(!(DVX && PDV) && (EXT || !PDV), "one rule per instance; primal steps live in the extended selection");
    static_assert(!P1R || P1, "the revised form's phase 1 is a phase-1 instance, under at most one rule (above)");
    constexpr bool XS = P1 || DVX || PDV;     // the LDS comes from the kernel
    constexpr bool TAB = P1 && !P1R;          // an instance that never sees the revised form
    double *sv; int *si; PivDesc *p_d; unsigned char *dyn;
    int *xr = nullptr;
    if constexpr (((DVX || PDV) && !P1) || P1R) xr = static_cast<SelSharedDvx *>(xs)->rv;      // (P1 without P1R: tableau form only, no row fetch of the revised form)
    if constexpr (XS) { sv = xs->sv; si = xs->si; p_d = &xs->d; dyn = xs->dyn; }
    else {
        __shared__ double l_sv[NT_BIG / WAVE];
        __shared__ int l_si[NT_BIG / WAVE];
        __shared__ PivDesc l_d;
        extern __shared__ unsigned char dyn_sel[];
        sv = l_sv; si = l_si; p_d = &l_d; dyn = dyn_sel;
    }
    PivDesc &s_d = *p_d;
    const int NT = (int)blockDim.x;
    double *skey = reinterpret_cast<double *>(dyn);          // [cap2] breakpoints |d_j| / |alpha_j| of the candidates
    int *sidx = reinterpret_cast<int *>(skey + cap2);             // [cap2] their columns
    unsigned char *sflag = reinterpret_cast<unsigned char *>(sidx + cap2);   // [N] 1 = column switches bound in this iteration
    if (Bv.status[b] != ST_RUNNING || Bv.mode[b] == MODE_REFRESH) return false;
    const int np = Bv.npend[b];
    if (np >= KP) return false;                // waits for the pass over its tableau
    const int tid = threadIdx.x;
    const int slot = Bv.dst[b];
    const SelCtx c = sel_ctx(L, Bv, b, np, slot, Bv.flushed[b] ? slot : Bv.src[b]);
    const int M = L.M, N = L.N, ld = L.ld;
    double *const beta = c.beta, *const drow = c.drow, *const row = c.row, *const pc = c.pc;
    double *dwork = drow;                      // the reduced costs the dual ratio test works with
    int pf = 0;
    if constexpr (EXT) {
        pf = Bv.pflags[b];
        double *dp = Bv.dper + (size_t)b * ld;
        if (pf & PF_PERT_PENDING) {
            apply_perturbation(L, c, dp);
            pf = (pf & ~PF_PERT_PENDING) | PF_PERT;
            if (tid == 0) { Bv.pflags[b] = pf; atomicAdd(&Bv.xstat[1], 1); }
        }
        if (pf & PF_PERT) dwork = dp;
    }
    // anti-cycling: after `bland_after` pivots (a healthy solve needs far fewer) switch to Bland's rule --
    // smallest variable id among the infeasible rows, exact minimum ratio with smallest id among ties
    // (and while a primal clean-up is in a streak of PRIMAL_STALL degenerate steps: ex09 in the revised form met clean-ups that cycled on a
    //  degenerate face for 166 000 pivots, until bland_after ended them within 500.  Bland's rule from the first clean-up step on is no
    //  answer -- 2 M pivots, it crawls while there is progress to be made -- so it holds only as long as the steps have length zero)
    const bool bland = (Bv.iters[b] >= L.bland_after || (EXT && (pf & PF_PRIMAL) && Bv.stall[b] >= PRIMAL_STALL)) && !(pf & PF_PERT);     // (perturbed costs break the ties themselves)
    int r = -1, q = -1, nflip = 0;
    bool below = false, incr = false;        // incr: bound switches of this iteration already carried into beta
    const bool primal = EXT && (pf & PF_PRIMAL);
    double pstep = 1.0;                      // length of a primal step (clean-up)
    int rsig = 0;                            // phase 1: which bound the leaving variable violated
    double *const snorm = DVX ? nv->norm + (size_t)b * L.Mp1p : nullptr;      // dual Devex pricing: the reference norms of the rows
    bool other_row = false;                  // ... the weighted rule chose another row than the largest violation's
    double *const tnorm = PDV ? nv->norm + (size_t)b * ld : nullptr;          // primal Devex pricing: the reference norms of the column positions
    double tq = 1.0;                         // ... the entering position's norm as it was (read by all, barriers before the update writes it)

    if (primal) {
        if (!primal_step<P1, DVX, PDV, P1R>(L, Bv, c, pf, bland, sv, si, r, q, below, pstep, rsig, xr, dyn, nv)) return true;
        if constexpr (PDV) tq = tnorm[q];
    } else {
    // ---- dual simplex step ----
    unsigned long long tk = (L.probe & 8) ? wall_clock64() : 0ull;
    // Phase A: the leaving row
    ValIdx best{0.0, -1};
    if constexpr (DVX) {
        // (the row of the largest violation is found beside it, for the statistics only: bslv_lpq_last_pricing_stats)
        ValIdx plain{0.0, -1};
        for (int i = tid; i < M; i += NT) {
            int k = c.bh[i];
            const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k), bt = beta[i];
            best = leave_candidate_dvx(best, lo, up, bt, snorm[i], k, i, bland, L.M + L.N);
            plain = leave_candidate(plain, lo, up, bt, k, i, bland, L.M + L.N);
        }
        best = block_argmax(best, sv, si);
        plain = block_argmax(plain, sv, si);
        other_row = !bland && best.i >= 0 && (best.i >> 1) != (plain.i >> 1);
    } else {
    for (int i = tid; i < M; i += NT) {
        int k = c.bh[i];
        best = leave_candidate(best, LO(L, Bv, b, k), UP(L, Bv, b, k), beta[i], k, i, bland, L.M + L.N);
    }
    best = block_argmax(best, sv, si);
    }
    if (best.i < 0) {
        if (EXT && (pf & PF_PERT)) {
            if (perturbation_off<XS>(L, Bv, c, pf, sv)) return true;
            dwork = drow;
        }
        conclude_optimal(L, Bv, c, Bv.iters[b], Bv.verified[b], NT, sv);
        return true;
    }
    if (Bv.iters[b] >= L.maxit) { if (tid == 0) { Bv.status[b] = BSLV_LP_UNDEFINED; Bv.mode[b] = MODE_NONE; } return true; }
    r = best.i >> 1; below = best.i & 1;
    const double sgn = below ? 1.0 : -1.0;
    phase_mark(L, Bv, b, 0, tk);
    fetch_row<TAB, DVX || PDV || P1R>(L, Bv, c, r, xr, dyn);
    phase_mark(L, Bv, b, 1, tk);

    // pass 0: row scale for the relative pivot tolerance
    double rmax = 0.0;
    for (int j = tid; j < N; j += NT) rmax = fmax(rmax, fabs(row[j]));
    rmax = block_max(rmax, sv);
    const double ptol = TOL_PIV * (1.0 + rmax);
    if constexpr (EXT) nflip = flip_breakpoints<XS>(L, Bv, c, r, below, sgn, ptol, dwork, cap2, skey, sidx, sflag, XS ? xs->cnt3 : nullptr);
    // pass 1: Harris bound on the dual step
    phase_mark(L, Bv, b, 2, tk);
    // (both passes fetch FOUR columns per thread and iteration with all loads issued first: on wide problems -- ex09: 37 000 columns,
    // 36 per thread -- a column after the other, its reduced cost loaded behind two branches, was a chain of ~100 memory latencies;
    // min and the (value, index) arg-max do not depend on the order)
    constexpr int PU = 4;
    double th = INFINITY;
    for (int j0 = tid; j0 < N; j0 += PU * NT) {
        int stv[PU]; double av[PU], dv[PU]; bool skip[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int j = j0 + u * NT;
            const bool in = j < N;
            stv[u] = in ? c.nstat[j] : NS_S; av[u] = in ? sgn * row[j] : 0.0; dv[u] = in ? dwork[j] : 0.0;
            skip[u] = !in || (EXT && sflag[in ? j : 0]);
        }
#pragma unroll
        for (int u = 0; u < PU; u++)
            if (!skip[u] && is_candidate(stv[u], av[u], ptol)) th = fmin(th, harris_key(dv[u], av[u], bland));
    }
    th = block_min(th, sv);
    phase_mark(L, Bv, b, 3, tk);
    if (isinf(th)) { conclude_infeasible(Bv, b, Bv.verified[b], r, below, np); return true; }
    // pass 2: largest |pivot| within the bound
    ValIdx piv{0.0, -1};
    for (int j0 = tid; j0 < N; j0 += PU * NT) {
        int stv[PU]; double av[PU], dv[PU]; bool skip[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int j = j0 + u * NT;
            const bool in = j < N;
            stv[u] = in ? c.nstat[j] : NS_S; av[u] = in ? sgn * row[j] : 0.0; dv[u] = in ? dwork[j] : 0.0;
            skip[u] = !in || (EXT && sflag[in ? j : 0]);
        }
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int j = j0 + u * NT;
            if (!skip[u] && is_candidate(stv[u], av[u], ptol) && within_bound(dv[u], av[u], th))
                piv = better_max(piv, ValIdx{bland ? (double)(L.M + L.N - c.nh[j]) : fabs(av[u]), j});
        }
    }
    piv = block_argmax(piv, sv, si);
    phase_mark(L, Bv, b, 4, tk);
    q = piv.i;
    if constexpr (EXT) incr = switch_bounds(L, Bv, c, r, nflip, skey, sidx);
    }
    bool col_ready = primal;                                         // pc[] holds the entering column (primal steps fetch it first)
    unsigned long long tk2 = (L.probe & 8) ? wall_clock64() : 0ull;
    if (!TAB && L.rev && !col_ready) { fetch_col(L, c, q); col_ready = true; }    // (the tableau form gathers its column in Phase D)
    phase_mark(L, Bv, b, 5, tk2);
    double sr = 1.0;                                                 // dual Devex pricing: the leaving row's norm as it was (read by all before Phase D writes it)
    if constexpr (DVX) sr = snorm[r];
    // Phase C: the descriptor, the basis heads
    if (tid == 0) {
        const double trq = row[q];
        // revised form: the pivot element comes out of TWO products -- rho K_q (the row) and the column B^-1 K_q -- which agree as long as
        // B^-1 is accurate.  Within a solve nothing refactorises it; when the two drift apart the LP is given up as UNDEFINED and the caller's
        // retry (bslv_lp.c:222-227: from the standard basis, an exact identity) takes over instead of a solve on a corrupted inverse -- or,
        // with bslv_lpq_set_refactor, the LP is marked and the call itself rebuilds the inverse from the heads and solves it again
        // (BSLV_LP_REV_DRIFT: the test hook that takes the check as failed at a given pivot of a given LP)
        if (!TAB && L.rev && (!(fabs(trq - pc[r]) <= 1e-8 * (1.0 + fabs(trq))) || (b == L.drift_b && Bv.iters[b] + 1 == L.drift_p))) {
            Bv.status[b] = BSLV_LP_UNDEFINED; Bv.mode[b] = MODE_NONE;
            if (L.rfx) Bv.rmark[b] = 1;
            if (L.trace == b) printf("lp %d it %d: pivot element from the row %.17g, from the column %.17g: B^-1 has drifted\n", b, Bv.iters[b], trq, pc[r]);
            s_d.r = -1;
        } else {
            s_d = commit_pivot(L, Bv, c, r, q, below, bland, Bv.iters[b], Bv.verified[b], (nflip > 0 && !incr) ? MODE_REFRESH : MODE_PIVOT, dwork, primal, nflip, pf & PF_PERT);
            if constexpr (DVX) {
                if (primal) atomicAdd(&nv->stat[2], 1);           // (a primal or phase-1 pivot: a new reference framework, see Phase D)
                else if (!bland) { atomicAdd(&nv->stat[0], 1); if (other_row) atomicAdd(&nv->stat[1], 1); }
            }
            if constexpr (EXT) {
                if (nflip > 0) atomicAdd(&Bv.xstat[0], 1);
                if (incr) atomicAdd(&Bv.xstat[4], 1);
                if (primal) { atomicAdd(&Bv.xstat[2], 1); Bv.stall[b] = pstep <= 1e-7 ? Bv.stall[b] + 1 : 0; }      // (streak of degenerate steps of this primal clean-up)
                else {      // dual degenerate stalling: perturb the costs from the next selection on
                    int stl = fabs(dwork[q] / trq) <= 1e-11 ? Bv.stall[b] + 1 : 0;
                    if (stl >= L.stall_limit && !(pf & PF_PERT) && (pf >> PF_USES_SHIFT) < PERT_MAX_USES) { Bv.pflags[b] = (pf | PF_PERT_PENDING) + (1 << PF_USES_SHIFT); stl = 0; }
                    Bv.stall[b] = stl;
                }
            }
        }
    }
    __syncthreads();
    const PivDesc d = s_d;
    if (d.r < 0) return true;                      // (given up: see above)
    if constexpr (PDV) {
        // primal Devex pricing: the norms follow a primal pivot along the pivot row (four columns per thread, loads first; a max, so
        // the order does not matter); a dual pivot starts a new framework
        if (primal) {
            constexpr int PU = 4;
            const double tnew = fmax(tq * fabs(d.p), 1.0);
            for (int j0 = tid; j0 < N; j0 += PU * NT) {
                double av[PU], tv[PU];
#pragma unroll
                for (int u = 0; u < PU; u++) {
                    const int j = j0 + u * NT;
                    const bool in = j < N;
                    av[u] = in ? row[j] : 0.0; tv[u] = in ? tnorm[j] : 1.0;
                }
#pragma unroll
                for (int u = 0; u < PU; u++) {
                    const int j = j0 + u * NT;
                    if (j < N) tnorm[j] = j == q ? tnew : fmax(tv[u], fabs(av[u] * d.p) * tq);
                }
            }
        } else {
            for (int j = tid; j < N; j += NT) tnorm[j] = 1.0;
            if (tid == 0) atomicAdd(&nv->stat[2], 1);
        }
    }
    // Phase D: the entering column as it is after the pending pivots -> multipliers of all rows, beta; the reduced-cost row
    for (int i = tid; i <= M; i += NT) {
        if (i == r) {
            pc[i] = 0.0; beta[i] = d.enter_val;
            if constexpr (DVX) snorm[i] = primal ? 1.0 : fmax(sr * fabs(d.p), 1.0);
            continue;
        }
        const double f = (i == M ? drow[q] : (col_ready ? pc[i] : virt_entry(c.T0[(size_t)i * ld + q], i, q, np, c.pd, c.prow0, c.pcol0, ld, L.Mp1p))) * d.p;
        pc[i] = f;
        if constexpr (DVX) { if (i < M) snorm[i] = primal ? 1.0 : fmax(snorm[i], fabs(f) * sr); }
        if constexpr (P1) {      // phase 1: did the step move a row other than the leaving one across a bound?  (d1 is then rebuilt)
            if ((pf & PF_PHASE1) && i < M) {
                const int k = c.bh[i];
                const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k);
                if (infeas_sign(lo, up, beta[i]) != infeas_sign(lo, up, fma(-f, d.pbeta, beta[i]))) Bv.pflags[b] = pf | PF_P1_STALE;      // (every writer writes the same word)
            }
        }
        beta[i] = fma(-f, d.pbeta, beta[i]);
    }
    __syncthreads();
    {
        const double fM = pc[M];
        for (int j = tid; j < N; j += NT) drow[j] = j == q ? fM : fma(-fM, row[j], drow[j]);
        if constexpr (EXT) {
            if (pf & (PF_PERT | (P1 ? PF_PHASE1 : 0))) {
                double *dp = Bv.dper + (size_t)b * ld;
                const double fP = dp[q] * d.p;
                __syncthreads();
                // (phase 1: d1 follows the pivot as the reduced costs do; the leaving variable's phase-1 cost drops to zero, which is its own entry's alone)
                for (int j = tid; j < N; j += NT) dp[j] = j == q ? ((P1 && (pf & PF_PHASE1)) ? fP - (double)rsig : fP) : fma(-fP, row[j], dp[j]);
            }
        }
    }
    if (tid == 0) Bv.npend[b] = np + 1;
    phase_mark(L, Bv, b, 6, tk2);
    if ((L.probe & 8) && b == 0 && tid == 0) Bv.dbg[7] += 1;
    return true;
}
// ---- select_once<false> of the tableau form with a pivot's row and column state kept on chip (k_select_cached) ----
// (select_once goes to global memory for every row entry, status and reduced cost in each pass, and per pending pivot in virt_entry: DESIGN 4e, 4b.)  Here
//  * thread tid owns the columns tid + u NT, u < CPT, from the row fetch to the reduced-cost update: row entry, reduced cost and status
//    stay in registers; whether a column is a candidate (status, sign, pivot tolerance) is decided once; the row goes to prow once
//    (k_flush reads it there) and the reduced costs to dcur once;
//  * the pending descriptors are staged in LDS once per selection, the multipliers that are the same for the whole workgroup
//    (pcol[s][r] for the row, prow[s][q] for the column) as soon as r / q is known, and the per-entry loads of ALL pending pivots
//    (and of all owned columns / four rows) are issued before the first is used;
//  * the entering column's loads are in flight while thread 0 writes the descriptor and the basis heads.
// Same helpers, same order of operations, same reductions as select_once: no pivot and no bit differs (tests/test_lp_select_cache_gpu.py).
// For workgroups of NT threads and N <= CPT * NT; everything else (1024 threads, extended selection, revised form) stays with select_once.
template <int CPT>
__device__ __forceinline__ bool select_once_cached(const LpView &L, const BatchView &Bv, const int b)
{
    __shared__ double sv[NT / WAVE]; __shared__ int si[NT / WAVE];
    __shared__ PivDesc s_pd[KP];             // the pending pivots
    __shared__ double s_mul[KP];             // of pending pivot s: pcol[s][r] while the row is built, prow[s][q] for the column
    __shared__ PivDesc s_d; __shared__ double s_fM;
    constexpr int RU = 4;                    // rows per thread in flight
    const int tid = threadIdx.x;
    // (one trip for everything the LP's state decides)
    const int status = Bv.status[b], mode = Bv.mode[b], np = Bv.npend[b], slot = Bv.dst[b], srcslot = Bv.src[b], flushed = Bv.flushed[b];
    const int iters = Bv.iters[b], verified = Bv.verified[b];
    if (status != ST_RUNNING || mode == MODE_REFRESH) return false;
    if (np >= KP) return false;                // waits for the pass over its tableau
    const SelCtx c = sel_ctx(L, Bv, b, np, slot, flushed ? slot : srcslot);
    const int M = L.M, N = L.N, ld = L.ld, Mp1p = L.Mp1p;
    const double *const T0 = c.T0, *const prow0 = c.prow0, *const pcol0 = c.pcol0;
    double *const beta = c.beta, *const drow = c.drow, *const row = c.row, *const pc = c.pc;
    if (tid < np) s_pd[tid] = c.pd[tid];       // (read after the barriers of Phase A's reduction)
    const bool bland = iters >= L.bland_after;
    unsigned long long tk = (L.probe & 8) ? wall_clock64() : 0ull;

    // Phase A: the leaving row
    ValIdx best{0.0, -1};
    for (int i0 = tid; i0 < M; i0 += RU * NT) {
        int kv[RU]; double lov[RU], upv[RU], btv[RU];
#pragma unroll
        for (int u = 0; u < RU; u++) { const int i = i0 + u * NT; kv[u] = i < M ? c.bh[i] : -1; btv[u] = i < M ? beta[i] : 0.0; }
#pragma unroll
        for (int u = 0; u < RU; u++) { lov[u] = kv[u] >= 0 ? LO(L, Bv, b, kv[u]) : -INFINITY; upv[u] = kv[u] >= 0 ? UP(L, Bv, b, kv[u]) : INFINITY; }
#pragma unroll
        for (int u = 0; u < RU; u++) best = leave_candidate(best, lov[u], upv[u], btv[u], kv[u], i0 + u * NT, bland, M + N);
    }
    best = block_argmax(best, sv, si);
    if (best.i < 0) { conclude_optimal(L, Bv, c, iters, verified, NT, sv); return true; }
    if (iters >= L.maxit) { if (tid == 0) { Bv.status[b] = BSLV_LP_UNDEFINED; Bv.mode[b] = MODE_NONE; } return true; }
    const int r = best.i >> 1; const bool below = best.i & 1;
    const double sgn = below ? 1.0 : -1.0;
    phase_mark(L, Bv, b, 0, tk);

    // the pivot row as it is after the pending pivots: stored entry, the pending rows' entries, status and reduced cost of every owned
    // column in one round of loads
    double rowv[CPT], dv[CPT]; int stv[CPT];
    {
        double t0v[CPT], pr[KP - 1][CPT];
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int j = tid + u * NT;
            const bool in = j < N;
            t0v[u] = in ? T0[(size_t)r * ld + j] : 0.0;
            stv[u] = in ? c.nstat[j] : NS_S;
            dv[u] = in ? drow[j] : 0.0;
#pragma unroll
            for (int s = 0; s < KP - 1; s++) pr[s][u] = (in && s < np) ? prow0[(size_t)s * ld + j] : 0.0;
        }
        if (tid < np) s_mul[tid] = pcol0[(size_t)tid * Mp1p + r];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int j = tid + u * NT;
            double v = t0v[u];
#pragma unroll
            for (int s = 0; s < KP - 1; s++) {
                if (s < np) {
                    const PivDesc d = s_pd[s];
                    v = apply_pending(v, r == d.r, j == d.q, d.p, s_mul[s], pr[s][u]);
                }
            }
            rowv[u] = j < N ? v : 0.0;
            if (j < ld) row[j] = rowv[u];
        }
    }
    phase_mark(L, Bv, b, 1, tk);

    // pass 0: row scale for the relative pivot tolerance
    double rmax = 0.0;
#pragma unroll
    for (int u = 0; u < CPT; u++) if (tid + u * NT < N) rmax = fmax(rmax, fabs(rowv[u]));
    rmax = block_max(rmax, sv);             // (its barriers also order the reads of s_mul above before the next write below)
    const double ptol = TOL_PIV * (1.0 + rmax);
    phase_mark(L, Bv, b, 2, tk);
    // the candidates, decided once; pass 1: Harris bound on the dual step
    bool cand[CPT];
    double th = INFINITY;
#pragma unroll
    for (int u = 0; u < CPT; u++) {
        const double a = sgn * rowv[u];
        cand[u] = tid + u * NT < N && is_candidate(stv[u], a, ptol);
        if (cand[u]) th = fmin(th, harris_key(dv[u], a, bland));
    }
    th = block_min(th, sv);
    phase_mark(L, Bv, b, 3, tk);
    if (isinf(th)) { conclude_infeasible(Bv, b, verified, r, below, np); return true; }
    // pass 2: largest |pivot| within the bound
    ValIdx piv{0.0, -1};
    if (bland) {
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int j = tid + u * NT;
            const double a = sgn * rowv[u];
            if (cand[u] && within_bound(dv[u], a, th)) piv = better_max(piv, ValIdx{(double)(M + N - c.nh[j]), j});
        }
    } else {
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const double a = sgn * rowv[u];
            if (cand[u] && within_bound(dv[u], a, th)) piv = better_max(piv, ValIdx{fabs(a), tid + u * NT});
        }
    }
    piv = block_argmax(piv, sv, si);
    phase_mark(L, Bv, b, 4, tk);
    const int q = piv.i;
    unsigned long long tk2 = (L.probe & 8) ? wall_clock64() : 0ull;

    // Phase D's loads first -- the entering column of the stored tableau, the pending multipliers of its rows, beta -- so that they
    // are in flight while thread 0 is in Phase C
    double c0[RU], btd[RU], pcl[KP - 1][RU];
    auto load_rows = [&](const int i0) {
#pragma unroll
        for (int u = 0; u < RU; u++) {
            const int i = i0 + u * NT;
            c0[u] = i < M ? T0[(size_t)i * ld + q] : (i == M ? drow[q] : 0.0);
            btd[u] = i <= M ? beta[i] : 0.0;
#pragma unroll
            for (int s = 0; s < KP - 1; s++) pcl[s][u] = (i < M && s < np) ? pcol0[(size_t)s * Mp1p + i] : 0.0;
        }
    };
    load_rows(tid);
    if (tid < np) s_mul[tid] = prow0[(size_t)tid * ld + q];
    // Phase C: the descriptor, the basis heads
    if (tid == 0) s_d = commit_pivot(L, Bv, c, r, q, below, bland, iters, verified, MODE_PIVOT, drow, false, 0, false);
    __syncthreads();
    const PivDesc d = s_d;
    phase_mark(L, Bv, b, 5, tk2);
    // Phase D: the entering column as it is after the pending pivots -> multipliers of all rows, beta; the reduced-cost row
    for (int i0 = tid; ; ) {
#pragma unroll
        for (int u = 0; u < RU; u++) {
            const int i = i0 + u * NT;
            if (i > M) continue;
            if (i == r) { pc[i] = 0.0; beta[i] = d.enter_val; continue; }
            double v = c0[u];
            if (i < M) {
#pragma unroll
                for (int s = 0; s < KP - 1; s++) {
                    if (s < np) {
                        const PivDesc ds = s_pd[s];
                        v = apply_pending(v, i == ds.r, q == ds.q, ds.p, pcl[s][u], s_mul[s]);
                    }
                }
            }
            const double f = v * d.p;
            pc[i] = f;
            beta[i] = fma(-f, d.pbeta, btd[u]);
            if (i == M) s_fM = f;
        }
        i0 += RU * NT;
        if (i0 > M) break;
        load_rows(i0);
    }
    __syncthreads();
    {
        const double fM = s_fM;
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int j = tid + u * NT;
            if (j < N) drow[j] = j == q ? fM : fma(-fM, rowv[u], dv[u]);
        }
    }
    if (tid == 0) Bv.npend[b] = np + 1;
    phase_mark(L, Bv, b, 6, tk2);
    if ((L.probe & 8) && b == 0 && tid == 0) Bv.dbg[7] += 1;
    return true;
}
// (the extended instance is a function of its own, as the compiler always had it: inlined into the 1024-thread kernel it spills 300 registers, called none)
__device__ __noinline__ bool select_once_ext(const LpView &L, const BatchView &Bv, const int b, const int cap2) { return select_once<true>(L, Bv, b, cap2); }
__device__ __noinline__ bool select_once_p1(const LpView &L, const BatchView &Bv, const int b, const int cap2, SelShared *xs) { return select_once<true, true>(L, Bv, b, cap2, xs); }
__device__ __noinline__ bool select_once_p1_rev(const LpView &L, const BatchView &Bv, const int b, const int cap2, SelShared *xs) { return select_once<true, true, false, false, true>(L, Bv, b, cap2, xs); }
// (Devex pricing: the extended and the phase-1 shape of either rule)
template <int RULE, bool P1>
__device__ __noinline__ bool select_once_priced(const LpView &L, const BatchView &Bv, const int b, const int cap2, SelShared *xs, const NormView *nv) { return select_once<true, P1, RULE == RULE_DVX, RULE == RULE_PDV>(L, Bv, b, cap2, xs, nv); }
// One launch selects up to nsel pivots per LP, one after the other, by the same workgroup: the KP selections between two passes
// over the tableau depend only on the LP's own vectors (beta, the reduced-cost row, the pending pivot rows and multipliers) -- no
// grid-wide dependency asks for a launch each (rounds 1-3 launched this kernel KP times per pass, 17 % of all GPU time in
// launches of 25 us; BSLV_SELECT_FUSE=0 brings that form back: the results are the same bit for bit, tests/test_lp_gpu.py).
template <bool EXT>
__global__ __launch_bounds__(NT_BIG) void k_select(LpView L, BatchView Bv, const int *active, int nact, int cap2, int nsel)
{
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];          // compacted list of the LPs still running
    if (blockIdx.y > 0) { rev_helper(L, Bv, b); return; }      // (revised form: helps with the sparse products of LP b's tableau rows until told to leave)
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();              // (what thread 0 / every thread wrote for the LP -- status, mode, pending count, beta, reduced costs -- is read by all)
        if (!(EXT ? select_once_ext(L, Bv, b, cap2) : select_once<false>(L, Bv, b, cap2))) break;
    }
    if (L.helpers > 1) {                       // every path of the LP's own workgroup ends here: the helpers may go
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// k_select<true> with phase 1 in its primal steps: what the PRIMAL and REPAIR methods launch (tableau form; the LPs of a batch that
// are in phase 1, in phase 2 and in the dual simplex share the launch)
__global__ __launch_bounds__(NT_BIG) void k_select_p1(LpView L, BatchView Bv, const int *active, int nact, int cap2, int nsel)
{
    __shared__ SelShared xs;
    extern __shared__ unsigned char dyn_p1[];
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if (threadIdx.x == 0) xs.dyn = dyn_p1;
    __syncthreads();
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!select_once_p1(L, Bv, b, cap2, &xs)) break;
    }
}

// k_select_p1 for the revised form: what a PRIMAL or REPAIR call of bslv_lpq_solve_batch_method launches there.  The extended selection
// with phase 1, rows and columns by fetch_row / fetch_col's revised variants, the phase-1 pricing vector as the tableau row of a
// synthesised rho (phase1_prepare<true>), helper workgroups for the sparse products as in k_select.  The default pricing rule only.  Like
// the priced instances it declares its LDS itself -- the words of the revised form's row fetch with it -- and hands it down, under a
// dynamic-LDS name of its own: the kernels above compile to what they always did.
extern __shared__ unsigned char dyn_p1_rev[];
__global__ __launch_bounds__(NT_BIG) void k_select_p1_rev(LpView L, BatchView Bv, const int *active, int nact, int cap2, int nsel)
{
    __shared__ SelSharedDvx xs;
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if (blockIdx.y > 0) { rev_helper<true>(L, Bv, b, xs.rv, dyn_p1_rev); return; }
    if (threadIdx.x == 0) xs.dyn = dyn_p1_rev;
    __syncthreads();
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!select_once_p1_rev(L, Bv, b, cap2, &xs)) break;
    }
    if (L.helpers > 1) {                       // every path of the LP's own workgroup ends here: the helpers may go
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// k_select<false> for the tableau form in workgroups of NT threads and rows of at most CPT * NT columns (CPT = 2, 4, 6: every row
// length below the 1536 columns from which a selection takes NT_BIG threads).  A kernel of its own: k_select is compiled for 1024
// threads, 128 registers, and carries the revised form's sparse products; this one holds its state in registers without spilling.
template <int CPT>
__global__ __launch_bounds__(NT) void k_select_cached(LpView L, BatchView Bv, const int *active, int nact, int nsel)
{
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!select_once_cached<CPT>(L, Bv, b)) break;
    }
}

// k_select<EXT> and k_select_p1 under Devex pricing (select_once<.., DVX> or <.., PDV>), in both forms and at both block sizes, the
// helpers of the revised form included.  RULE_DVX (bslv_lpq_set_pricing): what a batch launches while the switch is on, in the three
// shapes plain, EXT and P1.  RULE_PDV (bslv_lpq_set_primal_pricing): what an objective batch launches while the switch is on, and a
// PRIMAL / REPAIR batch while the dual rule is the default one; EXT and P1 only, primal steps live in the extended selection.  Kernels
// of their own, with their LDS declared here and handed down (see SelShared), so that the ones above compile to what they always did.
// k_select_cached has no such instance: with a switch on, the plan does not take it.  P1 is the tableau form alone: no helpers, and
// no words of a row fetch in its LDS.
// (the dynamic LDS of an instance under a name of its own, as the kernels above have it: with one name for all five the compiler no
//  longer knows its address where a pointer to it is made, and the helper branch and the extended instances get other code)
template <int RULE, bool P1, bool EXT> extern __shared__ unsigned char dyn_priced[];
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-var-template"      // (dynamic LDS has no definition)
template <int RULE, bool P1, bool EXT>
__global__ __launch_bounds__(NT_BIG) void k_select_priced(LpView L, BatchView Bv, NormView Nv, const int *active, int nact, int cap2, int nsel)
{
    static_assert(RULE == RULE_DVX ? EXT || !P1 : RULE == RULE_PDV && EXT, "the five instances: DVX plain, EXT, P1; PDV EXT, P1");
    __shared__ std::conditional_t<P1, SelShared, SelSharedDvx> xs;
    unsigned char *const dyn = dyn_priced<RULE, P1, EXT>;
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if constexpr (!P1) if (blockIdx.y > 0) { rev_helper<true>(L, Bv, b, xs.rv, dyn); return; }
    if (threadIdx.x == 0) xs.dyn = dyn;
    __syncthreads();
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!(EXT ? select_once_priced<RULE, P1>(L, Bv, b, cap2, &xs, &Nv) : select_once<false, false, true>(L, Bv, b, cap2, &xs, &Nv))) break;
    }
    if constexpr (!P1) if (L.helpers > 1) {
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#pragma clang diagnostic pop

// k_select_p1_rev under Devex pricing: what a PRIMAL or REPAIR call of bslv_lpq_solve_batch_method_priced launches in the revised form
// (select_once<true, true, DVX, PDV, true>; the rule of the CALL -- the engine's two switches do not reach such a batch).  Rows, columns
// and the phase-1 pricing vector as in k_select_p1_rev, helper workgroups included; under RULE_PDV the norms follow a primal pivot in one
// more pass over the pivot row rev_row_of_rho has just completed (the helpers' slices are in: fetch_row ends behind its barrier), and
// phase 1 weights its own pricing vector by them; under RULE_DVX they follow a dual pivot with the multipliers of Phase D.  Kernels of
// their own again, LDS declared here and handed down, the dynamic LDS under a name per instance (see k_select_priced).
template <int RULE>
__device__ __noinline__ bool select_once_priced_p1_rev(const LpView &L, const BatchView &Bv, const int b, const int cap2, SelShared *xs, const NormView *nv) { return select_once<true, true, RULE == RULE_DVX, RULE == RULE_PDV, true>(L, Bv, b, cap2, xs, nv); }
template <int RULE> extern __shared__ unsigned char dyn_priced_p1_rev[];
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-var-template"      // (dynamic LDS has no definition)
template <int RULE>
__global__ __launch_bounds__(NT_BIG) void k_select_priced_p1_rev(LpView L, BatchView Bv, NormView Nv, const int *active, int nact, int cap2, int nsel)
{
    static_assert(RULE == RULE_DVX || RULE == RULE_PDV, "the two instances: one rule each");
    __shared__ SelSharedDvx xs;
    unsigned char *const dyn = dyn_priced_p1_rev<RULE>;
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if (blockIdx.y > 0) { rev_helper<true>(L, Bv, b, xs.rv, dyn); return; }
    if (threadIdx.x == 0) xs.dyn = dyn;
    __syncthreads();
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!select_once_priced_p1_rev<RULE>(L, Bv, b, cap2, &xs, &Nv)) break;
    }
    if (L.helpers > 1) {                       // every path of the LP's own workgroup ends here: the helpers may go
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#pragma clang diagnostic pop

// the reference norms (rows of ld values) of LP list[k] (nullptr: LP k) of the batch, k < n, back to 1: the start of a solve, and a refactorisation replay
__global__ void k_norm_ones(NormView Nv, int ld, const int *list, int n, int count)
{
    if ((int)blockIdx.y >= n) return;
    const int b = list ? list[blockIdx.y] : (int)blockIdx.y;
    double *t = Nv.norm + (size_t)b * ld;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ld; j += gridDim.x * blockDim.x) t[j] = 1.0;
    if (count && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&Nv.stat[2], 1);
}

// ---- TIE PHASE (bslv_lpq_set_canonical): the canonical optimal basis of a primal degenerate LP ----
// An LP whose optimum lies on several bounds at once (beta_i on a bound for basic i) has a whole face of optimal duals, and the basis the
// pivoting happened to end in names one of its vertices.  The canonical one is the basis that STAYS optimal when the per-LP bounds move
// to vlo + t dir, vup + t dir for every small t > 0 -- applied symbolically, no t is ever formed: beta(t) = beta + t g with
//   g_i = sum over the nonbasic per-LP variables j that sit on a (finite, hence shifted) bound of T[i][j] dir_j,
// a basic per-LP variable's own bounds move by its dir, and a TIED row (beta_i within btol of a bound) is WRONG when it would cross that
// bound for t > 0: g_i - shift_i < -tol at the lower bound, > tol at the upper one.  The phase is the dual simplex on that second level:
// the wrong tied row with the largest |g_i - shift_i| leaves (Bland's rule after PRIMAL_STALL steps), the entering column comes from the
// Harris ratio test of the dual selection (same helpers, the true reduced costs, no long steps), and the step has length ZERO: beta, the
// objective and every primal value stay what they were bit for bit (the leaving variable keeps its value, within btol of the bound it
// now sits on); the reduced costs, g and the pivot descriptor follow the pivot as always, so k_flush, lazy tableaux and warm starts see
// an ordinary pivot.  The phase ends OPTIMAL in every case: no wrong tied row (canonical), no entering candidate (the shifted LP is
// infeasible for t > 0), or the cap on its pivots.  It runs as kernel instances of its own after the rounds of the batch are over, on
// the LPs that ended OPTIMAL (an LP is ST_RUNNING again while it is in the phase, so that the pass kernels treat it as they treat any LP
// that still pivots) -- the kernels of a solve without the switch are not touched.
constexpr int TIE_NEW = 0, TIE_RUN = 1, TIE_DONE = 2;      // TieView::state
// one view for this phase and for the tie phase of an objective batch below (after the semicolon: what the member is there)
struct TieView {
    const double *dir;      // [vcnt] direction of the shift, per variable of the per-LP range; [ccnt] ddir, per variable of the cost range
    double *g;              // [B][Mp1p] d beta / d t; [B][ld] reduced-cost row of ddir
    int *state, *iters;     // [B] TIE_*; tie pivots of the LP; tie iterations (pivots + bound switches)
    int *stat;              // [4] LPs that entered the phase, tie pivots (iterations), LPs that ended without an entering candidate (on a column
                            // without a blocking row), LPs that gave up at the cap
    int cap;                // tie pivots (iterations) per LP
};
__device__ __forceinline__ double tie_shift(const LpView &L, const TieView &Tv, int k)
{
    const int j = k - L.vfirst;
    return (j >= 0 && j < L.vcnt) ? Tv.dir[j] : 0.0;
}
// the phase of LP b is over (why: the counter of Tv.stat that says so, or -1)
__device__ __forceinline__ void tie_finish(const BatchView &Bv, const TieView &Tv, const int b, const int why)
{
    if (threadIdx.x == 0) {
        Tv.state[b] = TIE_DONE; Bv.status[b] = BSLV_LP_OPTIMAL; Bv.mode[b] = MODE_NONE;
        if (why >= 0) atomicAdd(&Tv.stat[why], 1);
    }
}
// revised form, entry of the tie phase: g = sum over the shifted nonbasic per-LP variables of T[:, j] dir, T[:, j] = -B^-1 K_k through the
// pending steps.  The columns are combined first, u = sum dir_t K_kt in ascending t (K_k = e_k for k < M, a CSC column of -A otherwise:
// the unit vectors come first and touch a row each, the CSC columns follow one after the other, so every u_i is summed in that order),
// then ONE product with B^-1 as stored and the pending steps in order -- fetch_col_revised with u in place of K_kq -- instead of a
// column fetch per variable: the per-LP range can be as long as M.  u lies where the next pivot row's rho will (free until then).
__device__ __forceinline__ void tie_entry_revised(const LpView &L, const TieView &Tv, const SelCtx &c, double *g)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x, M = L.M, ldt = L.ldt;
    double *u = c.prow0 + (size_t)c.np * ldt;
    for (int i = tid; i < M; i += NT) u[i] = 0.0;
    __syncthreads();
    for (int t = tid; t < L.vcnt; t += NT) {
        const int k = L.vfirst + t, p = c.pos[k];
        if (k < M && p < 0 && c.nstat[-1 - p] != NS_F) u[k] = Tv.dir[t];
    }
    for (int t = max(0, M - L.vfirst); t < L.vcnt; t++) {
        const int k = L.vfirst + t, p = c.pos[k];
        if (p >= 0 || c.nstat[-1 - p] == NS_F) continue;      // (basic, or free at zero: no bound to move with -- the same for every thread)
        __syncthreads();
        const double dt = Tv.dir[t];
        for (int e = L.cptr[k - M] + tid; e < L.cptr[k - M + 1]; e += NT) u[L.cidx[e]] = fma(-L.cval[e], dt, u[L.cidx[e]]);
    }
    __syncthreads();
    for (int i = tid; i < M; i += NT) {           // (B^-1 as stored) u, in ascending k
        const double *Bi = c.T0 + (size_t)i * ldt;
        double v = 0.0;
        for (int k = 0; k < M; k++) { const double uk = u[k]; if (uk != 0.0) v = fma(uk, Bi[k], v); }
        g[i] = v;
    }
    for (int sp = 0; sp < c.np; sp++) {           // ... through the pending pivots, in order
        __syncthreads();
        const PivDesc d = c.pd[sp];
        const double vr = g[d.r];
        __syncthreads();
        for (int i = tid; i < M; i += NT) g[i] = i == d.r ? -d.p * vr : fma(-c.pcol0[(size_t)sp * L.Mp1p + i], vr, g[i]);
    }
    __syncthreads();
    for (int i = tid; i < M; i += NT) g[i] = -g[i];
}
// One tie pivot of LP b by the calling workgroup; false when the LP cannot select again before the next pass (finished, KP pivots pending).
// sv, si, p_d, s_g: LDS of the kernel (see SelShared for why it is handed down).
// REV (k_select_tie_rev: a slot holds B^-1): g on entry from one product with B^-1 (tie_entry_revised), the pivot row and the entering
// column by fetch_row / fetch_col's revised variants (xr, xdyn: the LDS of the row fetch, see fetch_row_revised), and select_once's
// cross-check of the pivot element between the two -- an LP that fails it commits nothing and leaves the phase OPTIMAL on the basis
// it had reached (Tv.stat[3]).  Everything else is the one text of both forms.
template <bool REV = false>
__device__ __forceinline__ bool tie_once(const LpView &L, const BatchView &Bv, const TieView &Tv, const int b, double *sv, int *si, PivDesc *p_d, double *s_g, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x;
    const int state = Tv.state[b], np = Bv.npend[b], titer = Tv.iters[b];
    if (state == TIE_DONE || np >= KP) return false;
    const int slot = Bv.dst[b];
    const SelCtx c = sel_ctx(L, Bv, b, np, slot, Bv.flushed[b] ? slot : Bv.src[b]);
    const int M = L.M, N = L.N, ld = L.ld;
    double *const g = Tv.g + (size_t)b * L.Mp1p;
    double *const beta = c.beta, *const drow = c.drow, *const row = c.row, *const pc = c.pc;
    __syncthreads();                           // (everyone has read the LP's state before thread 0 changes it)
    if (state == TIE_NEW) {
        // entry: g through the pending pivots, one column gather per nonbasic per-LP variable
        if constexpr (REV) tie_entry_revised(L, Tv, c, g);
        else
        for (int i = tid; i < M; i += NT) {
            double acc = 0.0;
            for (int t = 0; t < L.vcnt; t++) {
                const int p = c.pos[L.vfirst + t];
                if (p >= 0) continue;
                const int j = -1 - p;
                if (c.nstat[j] == NS_F) continue;      // (free at zero: no bound to move with)
                acc = fma(virt_entry(c.T0[(size_t)i * ld + j], i, j, np, c.pd, c.prow0, c.pcol0, ld, L.Mp1p), Tv.dir[t], acc);
            }
            g[i] = acc;
        }
        if (tid == 0) { Tv.state[b] = TIE_RUN; Bv.status[b] = ST_RUNNING; atomicAdd(&Tv.stat[0], 1); }
        __syncthreads();
    }
    const bool bland = titer >= PRIMAL_STALL;
    // Phase A: the leaving row -- the wrong tied row with the largest rate; id = 2*i + (below ? 1 : 0) as in leave_candidate
    ValIdx best{0.0, -1};
    for (int i = tid; i < M; i += NT) {
        const int k = c.bh[i];
        const double lo = LO(L, Bv, b, k), up = UP(L, Bv, b, k), bt = beta[i], gi = g[i], sh = tie_shift(L, Tv, k);
        const double rate = gi - sh, tol = TOL_BND * (1.0 + fabs(gi) + fabs(sh));
        if (!isinf(lo) && fabs(bt - lo) <= btol(lo) && rate < -tol) best = better_max(best, ValIdx{bland ? (double)(M + N - k) : -rate, 2 * i + 1});
        if (!isinf(up) && fabs(bt - up) <= btol(up) && rate > tol) best = better_max(best, ValIdx{bland ? (double)(M + N - k) : rate, 2 * i});
    }
    best = block_argmax(best, sv, si);
    if (best.i < 0) { tie_finish(Bv, Tv, b, -1); return false; }          // the basis is canonical
    if (titer >= Tv.cap) { tie_finish(Bv, Tv, b, 3); return false; }
    const int r = best.i >> 1; const bool below = best.i & 1;
    const double sgn = below ? 1.0 : -1.0;
    if constexpr (REV) fetch_row<false, true>(L, Bv, c, r, xr, xdyn); else fetch_row<true>(L, Bv, c, r);
    // the dual ratio test of select_once, on the true reduced costs
    double rmax = 0.0;
    for (int j = tid; j < N; j += NT) rmax = fmax(rmax, fabs(row[j]));
    rmax = block_max(rmax, sv);
    const double ptol = TOL_PIV * (1.0 + rmax);
    double th = INFINITY;
    for (int j = tid; j < N; j += NT) {
        const double a = sgn * row[j];
        if (is_candidate(c.nstat[j], a, ptol)) th = fmin(th, harris_key(drow[j], a, bland));
    }
    th = block_min(th, sv);
    if (isinf(th)) { tie_finish(Bv, Tv, b, 2); return false; }           // the shifted LP is infeasible for t > 0: the basis reached stays
    ValIdx piv{0.0, -1};
    for (int j = tid; j < N; j += NT) {
        const double a = sgn * row[j];
        if (is_candidate(c.nstat[j], a, ptol) && within_bound(drow[j], a, th)) piv = better_max(piv, ValIdx{bland ? (double)(M + N - c.nh[j]) : fabs(a), j});
    }
    piv = block_argmax(piv, sv, si);
    const int q = piv.i;
    if constexpr (REV) fetch_col(L, c, q);      // (the tableau form gathers its column in Phase D)
    // Phase C: the descriptor, the basis heads -- and the step of length zero
    if (tid == 0) {
        // (revised form: select_once's cross-check of the pivot element, the row's against the column's, with its test hook)
        if (REV && (!(fabs(row[q] - pc[r]) <= 1e-8 * (1.0 + fabs(row[q]))) || (b == L.drift_b && Bv.iters[b] + 1 == L.drift_p))) {
            if (L.trace == b) printf("lp %d it %d (tie phase): pivot element from the row %.17g, from the column %.17g: B^-1 has drifted\n", b, Bv.iters[b], row[q], pc[r]);
            p_d->r = -1;
        } else {
        const double sk = tie_shift(L, Tv, c.bh[r]), sq = c.nstat[q] == NS_F ? 0.0 : tie_shift(L, Tv, c.nh[q]);
        const double br = beta[r], xq = c.xN[q], gr = g[r];
        PivDesc d = commit_pivot(L, Bv, c, r, q, below, bland, Bv.iters[b], Bv.verified[b], MODE_PIVOT, drow, false, 0, false);
        d.pbeta = 0.0; d.enter_val = xq;       // nothing moves at t = 0: the entering variable keeps its value ...
        c.xN[q] = br;                          // ... and so does the leaving one, on its bound within btol
        Bv.desc[(size_t)b * KP + np] = d;
        *p_d = d;
        s_g[0] = gr - sk; s_g[1] = sq;
        Tv.iters[b] = titer + 1;
        atomicAdd(&Tv.stat[1], 1);
        }
    }
    __syncthreads();
    const PivDesc d = *p_d;
    if constexpr (REV) if (d.r < 0) { tie_finish(Bv, Tv, b, 3); return false; }      // (given up: the optimum is known, the basis reached stays)
    const double gp = s_g[0], sq = s_g[1];     // rate at which the leaving row crosses its bound; shift of the entering variable's own bound
    // Phase D: the multipliers of all rows; g follows the pivot as beta does in select_once (beta itself: a step of length zero)
    for (int i = tid; i <= M; i += NT) {
        if (i == r) { pc[i] = 0.0; beta[i] = d.enter_val; g[i] = fma(-gp, d.p, sq); continue; }
        const double f = (i == M ? drow[q] : (REV ? pc[i] : virt_entry(c.T0[(size_t)i * ld + q], i, q, np, c.pd, c.prow0, c.pcol0, ld, L.Mp1p))) * d.p;
        pc[i] = f;
        if (i < M) g[i] = fma(-f, gp, g[i]);
    }
    __syncthreads();
    {
        const double fM = pc[M];
        for (int j = tid; j < N; j += NT) drow[j] = j == q ? fM : fma(-fM, row[j], drow[j]);
    }
    if (tid == 0) Bv.npend[b] = np + 1;
    return true;
}
// Launched only while the switch is on (tableau form), with the workgroup size of the batch's selections
__global__ __launch_bounds__(NT_BIG) void k_select_tie(LpView L, BatchView Bv, TieView Tv, const int *active, int nact, int nsel)
{
    __shared__ double sv[NT_BIG / WAVE];
    __shared__ int si[NT_BIG / WAVE];
    __shared__ PivDesc s_d;
    __shared__ double s_g[2];
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!tie_once(L, Bv, Tv, b, sv, si, &s_d, s_g)) break;
    }
}
// k_select_tie for the revised form: what bslv_lpq_solve_batch_canonical launches there (tie_once<true>), with helper workgroups for the
// sparse products of the pivot rows as in k_select.  Like k_select_p1_rev it declares its LDS itself -- the words of the revised form's
// row fetch with it -- and hands it down, under a dynamic-LDS name of its own (rho alone): the kernels above compile to what they always
// did.  A tie pivot is a rank-1 step on B^-1 like any other and counts in the slot's age; no periodic refactorisation runs inside the phase.
extern __shared__ unsigned char dyn_tie_rev[];
__global__ __launch_bounds__(NT_BIG) void k_select_tie_rev(LpView L, BatchView Bv, TieView Tv, const int *active, int nact, int nsel)
{
    __shared__ SelSharedDvx xs;
    __shared__ double s_g[2];
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if (blockIdx.y > 0) { rev_helper<true>(L, Bv, b, xs.rv, dyn_tie_rev); return; }
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!tie_once<true>(L, Bv, Tv, b, xs.sv, xs.si, &xs.d, s_g, xs.rv, dyn_tie_rev)) break;
    }
    if (L.helpers > 1) {                       // every path of the LP's own workgroup ends here: the helpers may go
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- TIE PHASE OF AN OBJECTIVE BATCH (bslv_lpq_set_canonical_obj): the canonical optimal POINT of a dual degenerate LP ----
// The transposed case: an LP of solve_batch_obj whose costs are normal to a whole face of the feasible set's image has a face of optimal
// points, and the vertex the pivoting ended in is whichever it reached.  The canonical one is the vertex that STAYS optimal for the costs
// c + t ddir (ddir: ccnt values on the variables of the cost range) for every small t > 0 -- the lexicographic minimum of (c . x, ddir . x)
// -- again without ever forming t: the engine keeps g, the reduced-cost row of ddir at the current basis,
//   g_j = ddir_{nh[j]} + sum over the basic variables k of the cost range of ddir_k T[row of k][j]
// (built on entry through the pending pivots, as k_prep builds the reduced costs of a new objective; afterwards it follows every pivot by
// the pivot row, as the reduced costs do).  A nonbasic column is TIED when |d_j| <= TOL_DJ on the true reduced costs and WRONG when g_j
// has the sign primal_step's optimality test rejects for its status.  The phase is the primal simplex on that second level: the wrong
// tied column with the largest |g_j| enters (Bland's rule after PRIMAL_STALL steps), the leaving row comes from primal_step's Harris
// two-pass ratio test (phase 2's: restated here, so that the kernels that inline primal_step stay what they were), the entering variable
// switches bound without a pivot where its own box is the tightest ratio.  Unlike the tie phase above the steps HAVE A LENGTH: x moves
// along the optimal face, beta, x_N and the objective (by at most TOL_DJ x step) follow as in any primal step, and the step is an
// ordinary PivDesc for k_flush, lazy tableaux, parked passes and warm starts.  The phase ends OPTIMAL in every case: no wrong tied
// column (canonical), an entering column without a blocking row (ddir . x is unbounded on the optimal face: the basis reached stays), or
// the cap on its iterations -- after conclude_optimal's recomputation of beta where the solve has made that many pivots.  (TieView: above)
// the phase of LP b ends (why: the counter of Tv.stat that says so, or -1) -- on a recomputed beta by conclude_optimal's rule: false when
// the LP waits for that pass first (the selection after it comes to the same end)
__device__ __forceinline__ bool tie_obj_finish(const BatchView &Bv, const TieView &Tv, const int b, const int why)
{
    const int verified = Bv.verified[b], iters = Bv.iters[b];
    __syncthreads();
    if (!(verified & 1) && (iters > REFRESH_AFTER || (verified & 2))) { if (threadIdx.x == 0) Bv.mode[b] = MODE_REFRESH; return false; }
    if (threadIdx.x == 0) {
        Tv.state[b] = TIE_DONE; Bv.status[b] = BSLV_LP_OPTIMAL; Bv.mode[b] = MODE_NONE;
        if (why >= 0) atomicAdd(&Tv.stat[why], 1);
    }
    return true;
}
// One tie iteration of LP b by the calling workgroup; false when the LP cannot select again before the next pass (finished, waiting for
// a refresh, KP pivots pending).  sv, si, p_d: LDS of the kernel (see SelShared for why it is handed down).
// REV (k_select_tie_obj_rev: a slot holds B^-1 and no tableau row to walk): with T[r][j] = -rho_r . K[nh_j] the row g on entry is ONE
// tableau row, the one of the synthesised y = sum over the basic variables of the cost range of ddir_t rho_pos(cfirst + t), in ascending
// t (what rev_price_y does with the costs of the batch, here through the pending pivots): g_j = ddir_{nh[j]} - y . K[nh_j].  y lies
// where a pivot row's rho would (rev_form_rho) and its products take the pivot rows' path, helpers included (rev_row_of_rho); they
// write the LP's scratch row (c.row, free until a step fetches its pivot row), from which g is copied.  The entering column and the
// pivot row come from fetch_col / fetch_row's revised variants (xr, xdyn: the LDS of the row fetch, see fetch_row_revised), with
// select_once's cross-check of the pivot element between the two -- an LP that fails it commits nothing and leaves the phase OPTIMAL
// on the basis it had reached (Tv.stat[3]): every step of the phase keeps optimality.  A bound switch fetches no row and has no
// check.  Everything else is the one text of both forms.
template <bool REV = false>
__device__ __forceinline__ bool tie_obj_once(const LpView &L, const BatchView &Bv, const TieView &Tv, const int b, double *sv, int *si, PivDesc *p_d, int *xr = nullptr, unsigned char *xdyn = nullptr)
{
    const int tid = threadIdx.x, NT = (int)blockDim.x;
    const int state = Tv.state[b], np = Bv.npend[b], titer = Tv.iters[b], mode = Bv.mode[b];
    if (state == TIE_DONE || mode == MODE_REFRESH || np >= KP) return false;
    const int slot = Bv.dst[b];
    const SelCtx c = sel_ctx(L, Bv, b, np, slot, Bv.flushed[b] ? slot : Bv.src[b]);
    const int M = L.M, N = L.N, ld = L.ld;
    double *const g = Tv.g + (size_t)b * ld;
    double *const beta = c.beta, *const drow = c.drow, *const row = c.row, *const pc = c.pc;
    __syncthreads();                           // (everyone has read the LP's state before thread 0 changes it)
    if (state == TIE_NEW) {
        // entry: g through the pending pivots, at most ccnt tableau rows
        if constexpr (REV) {
            const int ldt = L.ldt;
            double *y_g = c.prow0 + (size_t)np * ldt;
            double *sy = L.rho_off >= 0 ? reinterpret_cast<double *>(xdyn + L.rho_off) : nullptr;
            for (int col = tid; col < ldt; col += NT) {      // (a thread owns columns of B^-1 and adds the rows in ascending t: a fixed order)
                double acc = 0.0;
                if (col < M)
                    for (int t = 0; t < L.ccnt; t++) {
                        const int pr = c.pos[L.cfirst + t];
                        if (pr >= 0) acc = fma(Tv.dir[t], virt_entry_b(c.T0[(size_t)pr * ldt + col], pr, col, np, c.pd, c.prow0, c.pcol0, ldt, L.Mp1p), acc);
                    }
                y_g[col] = acc;
                if (sy) sy[col] = acc;
            }
            __syncthreads();
            rev_row_of_rho<true>(L, Bv, c, sy ? sy : y_g, xr);
            __syncthreads();
            for (int j = tid; j < ld; j += NT) {
                double v = 0.0;
                if (j < N) {
                    v = row[j];
                    const int kj = c.nh[j] - L.cfirst;
                    if (kj >= 0 && kj < L.ccnt) v += Tv.dir[kj];      // (as k_rev_price adds the costs)
                }
                g[j] = v;
            }
        } else
        for (int j = tid; j < ld; j += NT) {
            double v = 0.0;
            if (j < N) {
                const int kj = c.nh[j] - L.cfirst;
                if (kj >= 0 && kj < L.ccnt) v = Tv.dir[kj];
                for (int t = 0; t < L.ccnt; t++) {
                    const int pr = c.pos[L.cfirst + t];
                    if (pr >= 0) v = fma(Tv.dir[t], virt_entry(c.T0[(size_t)pr * ld + j], pr, j, np, c.pd, c.prow0, c.pcol0, ld, L.Mp1p), v);
                }
            }
            g[j] = v;
        }
        if (tid == 0) { Tv.state[b] = TIE_RUN; Bv.status[b] = ST_RUNNING; atomicAdd(&Tv.stat[0], 1); }
        __syncthreads();
    }
    const bool bland = titer >= PRIMAL_STALL;
    // the entering column: the wrong tied column with the largest rate
    ValIdx ent{0.0, -1};
    for (int j = tid; j < N; j += NT) {
        const int st = c.nstat[j];
        if (st == NS_S || fabs(drow[j]) > TOL_DJ) continue;
        const double v = g[j], tol = TOL_DJ * (1.0 + fabs(v));
        double sc = 0.0;
        if (st == NS_L) { if (v < -tol) sc = -v; }
        else if (st == NS_U) { if (v > tol) sc = v; }
        else if (fabs(v) > tol) sc = fabs(v);
        if (sc > 0.0) ent = better_max(ent, ValIdx{bland ? (double)(M + N - c.nh[j]) : sc, j});
    }
    ent = block_argmax(ent, sv, si);
    if (ent.i < 0) { tie_obj_finish(Bv, Tv, b, -1); return false; }      // the point is canonical
    if (titer >= Tv.cap) { tie_obj_finish(Bv, Tv, b, 3); return false; }
    const int q = ent.i;
    const int stq = c.nstat[q], kq = c.nh[q];
    const double gq = g[q], dq = drow[q];
    const double dir = (stq == NS_U || (stq == NS_F && gq > 0.0)) ? -1.0 : 1.0;
    if constexpr (REV) fetch_col(L, c, q); else fetch_col<true>(L, c, q);
    // primal_step's ratio test (phase 2), on the entering column
    double cmax = 0.0;
    for (int i = tid; i < M; i += NT) cmax = fmax(cmax, fabs(pc[i]));
    cmax = block_max(cmax, sv);
    const double ptol = TOL_PIV * (1.0 + cmax);
    const double gap = UP(L, Bv, b, kq) - LO(L, Bv, b, kq);     // inf unless both bounds are finite
    double tmax = gap;
    for (int i = tid; i < M; i += NT) {
        const double a = pc[i] * dir;
        if (fabs(a) < ptol) continue;
        const int k = c.bh[i];
        const double bt = beta[i];
        if (a > 0) { const double up = UP(L, Bv, b, k); if (!isinf(up)) tmax = fmin(tmax, fmax(up + (bland ? 0.0 : btol(up)) - bt, 0.0) / a); }
        else { const double lo = LO(L, Bv, b, k); if (!isinf(lo)) tmax = fmin(tmax, fmax(bt - lo + (bland ? 0.0 : btol(lo)), 0.0) / -a); }
    }
    tmax = block_min(tmax, sv);
    if (isinf(tmax)) { tie_obj_finish(Bv, Tv, b, 2); return false; }     // no blocking row: ddir . x is unbounded on the optimal face
    ValIdx lv{0.0, -1};
    for (int i = tid; i < M; i += NT) {
        const double a = pc[i] * dir;
        if (fabs(a) < ptol) continue;
        const int k = c.bh[i];
        const double bt = beta[i];
        if (a > 0) { const double up = UP(L, Bv, b, k); if (!isinf(up) && (up - bt) / a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(M + N - k) : a, 2 * i + 1}); }
        else { const double lo = LO(L, Bv, b, k); if (!isinf(lo) && (bt - lo) / -a <= tmax) lv = better_max(lv, ValIdx{bland ? (double)(M + N - k) : -a, 2 * i}); }
    }
    lv = block_argmax(lv, sv, si);
    double tstep = INFINITY;
    if (lv.i >= 0) {
        const int i = lv.i >> 1, k = c.bh[i];
        tstep = fmax(((lv.i & 1) ? UP(L, Bv, b, k) - beta[i] : beta[i] - LO(L, Bv, b, k)) / fabs(pc[i] * dir), 0.0);
    }
    if (lv.i < 0 || gap <= tstep) {
        // the entering variable reaches its own other bound first: no pivot, g stands as it is
        __syncthreads();
        for (int i = tid; i < M; i += NT) beta[i] = fma(pc[i], dir * gap, beta[i]);
        if (tid == 0) {
            beta[M] = fma(dq, dir * gap, beta[M]);
            if (stq == NS_L) { c.nstat[q] = NS_U; c.xN[q] = UP(L, Bv, b, kq); } else { c.nstat[q] = NS_L; c.xN[q] = LO(L, Bv, b, kq); }
            if (L.trace == b) printf("lp %d it %d tie: column %d (var %d) g %.3e switches bound\n", b, Bv.iters[b], q, kq, gq);
            Bv.verified[b] &= 2;
            Bv.iters[b] += 1;
            Tv.iters[b] = titer + 1;
            atomicAdd(&Tv.stat[1], 1);
        }
        return true;
    }
    const int r = lv.i >> 1;
    const bool below = !(lv.i & 1);          // the leaving variable goes to its lower bound
    if constexpr (REV) fetch_row<false, true>(L, Bv, c, r, xr, xdyn); else fetch_row<true>(L, Bv, c, r);
    // the descriptor, the basis heads
    if (tid == 0) {
        // (revised form: select_once's cross-check of the pivot element, the row's against the column's, with its test hook)
        if (REV && (!(fabs(row[q] - pc[r]) <= 1e-8 * (1.0 + fabs(row[q]))) || (b == L.drift_b && Bv.iters[b] + 1 == L.drift_p))) {
            if (L.trace == b) printf("lp %d it %d (tie phase of an objective batch): pivot element from the row %.17g, from the column %.17g: B^-1 has drifted\n", b, Bv.iters[b], row[q], pc[r]);
            p_d->r = -1;
        } else {
        *p_d = commit_pivot(L, Bv, c, r, q, below, bland, Bv.iters[b], Bv.verified[b], MODE_PIVOT, g, true, 0, false);
        Tv.iters[b] = titer + 1;
        atomicAdd(&Tv.stat[1], 1);
        }
    }
    __syncthreads();
    const PivDesc d = *p_d;
    if constexpr (REV) if (d.r < 0) { tie_obj_finish(Bv, Tv, b, 3); return false; }      // (given up: the optimum is known, the basis reached stays)
    // the multipliers of all rows, beta; the reduced-cost row and g follow the pivot (select_once, Phase D)
    for (int i = tid; i <= M; i += NT) {
        if (i == r) { pc[i] = 0.0; beta[i] = d.enter_val; continue; }
        const double f = (i == M ? dq : pc[i]) * d.p;
        pc[i] = f;
        beta[i] = fma(-f, d.pbeta, beta[i]);
    }
    __syncthreads();
    {
        const double fM = pc[M], fG = gq * d.p;
        for (int j = tid; j < N; j += NT) {
            const double rj = row[j];
            drow[j] = j == q ? fM : fma(-fM, rj, drow[j]);
            g[j] = j == q ? fG : fma(-fG, rj, g[j]);
        }
    }
    if (tid == 0) Bv.npend[b] = np + 1;
    return true;
}
// Launched only while the switch is on (tableau form, objective batches), with the workgroup size of the batch's selections
__global__ __launch_bounds__(NT_BIG) void k_select_tie_obj(LpView L, BatchView Bv, TieView Tv, const int *active, int nact, int nsel)
{
    __shared__ double sv[NT_BIG / WAVE];
    __shared__ int si[NT_BIG / WAVE];
    __shared__ PivDesc s_d;
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!tie_obj_once(L, Bv, Tv, b, sv, si, &s_d)) break;
    }
}
// k_select_tie_obj for the revised form: what bslv_lpq_solve_batch_obj_canonical launches there (tie_obj_once<true>), with helper
// workgroups for the sparse products of g and of the pivot rows as in k_select.  Like k_select_tie_rev it declares its LDS itself -- the
// words of the revised form's row fetch with it -- and hands it down, under a dynamic-LDS name of its own (rho alone): the kernels above
// compile to what they always did.  A tie pivot is a rank-1 step on B^-1 like any other and counts in the slot's age; no periodic
// refactorisation runs inside the phase.  A slot of this form has no row M: the reduced costs reach it by k_rev_store_d, as after any solve.
extern __shared__ unsigned char dyn_tie_obj_rev[];
__global__ __launch_bounds__(NT_BIG) void k_select_tie_obj_rev(LpView L, BatchView Bv, TieView Tv, const int *active, int nact, int nsel)
{
    __shared__ SelSharedDvx xs;
    if ((int)blockIdx.x >= nact) return;
    const int b = active[blockIdx.x];
    if (blockIdx.y > 0) { rev_helper<true>(L, Bv, b, xs.rv, dyn_tie_obj_rev); return; }
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();
        if (!tie_obj_once<true>(L, Bv, Tv, b, xs.sv, xs.si, &xs.d, xs.rv, dyn_tie_obj_rev)) break;
    }
    if (L.helpers > 1) {                       // every path of the LP's own workgroup ends here: the helpers may go
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&Bv.hmail[(size_t)b * 8], (L.launch_id << 8) | 0xFF, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- which LPs need a pass over their tableau: pending pivots to apply, or beta to recompute ----
__global__ void k_list_pending(BatchView Bv, const int *active, int nact, int it)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nact) return;
    const int b = active[k];
    if (Bv.npend[b] > 0 || Bv.mode[b] == MODE_REFRESH) {
        // lazy: a pass over the tableau is for LPs that go on pivoting (or work in place); one that is finished keeps its <= KP pending
        // pivots -- values, duals and objective are all in its vectors -- and most such tableaux are never looked at again
        if (Bv.lazy && Bv.status[b] != ST_RUNNING && Bv.src[b] != Bv.dst[b] && Bv.mode[b] != MODE_REFRESH) return;
        Bv.work[atomicAdd(&Bv.nwork[it], 1)] = b;
    }
}
// lazy: the LPs list[0..n) (batch indices) whose slot still lacks its tableau -> work list of counter slot cnt_slot
__global__ void k_list_given(BatchView Bv, const int *list, int n, int cnt_slot)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int b = list[k];
    if (Bv.npend[b] > 0 || !Bv.flushed[b]) Bv.work[atomicAdd(&Bv.nwork[cnt_slot], 1)] = b;
}
// lazy: the reduced costs of every LP go to row M of its slot (k_flush would have left them there; the getters read them from there)
__global__ void k_store_d(LpView L, BatchView Bv, int B)
{
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && j < L.ld) L.T[(size_t)Bv.dst[b] * L.slotT + (size_t)L.M * L.ld + j] = Bv.dcur[(size_t)b * L.ld + j];
}
__global__ void k_after_flush(BatchView Bv, int it)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Bv.nwork[it]) return;
    const int b = Bv.work[k];
    Bv.npend[b] = 0;
    Bv.flushed[b] = 1;
    if (Bv.mode[b] == MODE_REFRESH) { Bv.verified[b] |= 1; Bv.mode[b] = MODE_NONE; }
}
// parked passes (bslv_lpq_park): what the pass of LP pairs[2k] of the batch needs goes to record pairs[2k+1] of the store -- its
// counters, the descriptors, pivot rows and multiplier columns of its pending pivots, its reduced-cost row.  One workgroup per LP.
__global__ __launch_bounds__(NT) void k_park_copy(LpView L, BatchView Bv, BatchView Pv, const int *pairs, int n)
{
    if ((int)blockIdx.x >= n) return;
    const int b = pairs[2 * blockIdx.x], rec = pairs[2 * blockIdx.x + 1];
    const int np = Bv.npend[b];
    if (threadIdx.x == 0) {
        Pv.npend[rec] = np; Pv.flushed[rec] = Bv.flushed[b]; Pv.mode[rec] = Bv.mode[b]; Pv.verified[rec] = Bv.verified[b];
        const_cast<int *>(Pv.src)[rec] = Bv.src[b]; const_cast<int *>(Pv.dst)[rec] = Bv.dst[b];
    }
    if ((int)threadIdx.x < np) Pv.desc[(size_t)rec * KP + threadIdx.x] = Bv.desc[(size_t)b * KP + threadIdx.x];
    const int ld2 = L.ldt >> 1, mp2 = L.Mp1p >> 1, d2 = L.ld >> 1;
    const double2 *pr = reinterpret_cast<const double2 *>(Bv.prow + (size_t)b * KP * L.ldt), *pc = reinterpret_cast<const double2 *>(Bv.pcol + (size_t)b * KP * L.Mp1p);
    const double2 *dc = reinterpret_cast<const double2 *>(Bv.dcur + (size_t)b * L.ld);
    double2 *qr = reinterpret_cast<double2 *>(Pv.prow + (size_t)rec * KP * L.ldt), *qc = reinterpret_cast<double2 *>(Pv.pcol + (size_t)rec * KP * L.Mp1p);
    double2 *qd = reinterpret_cast<double2 *>(Pv.dcur + (size_t)rec * L.ld);
    for (int k = threadIdx.x; k < np * ld2; k += NT) qr[k] = pr[k];
    for (int k = threadIdx.x; k < np * mp2; k += NT) qc[k] = pc[k];
    for (int k = threadIdx.x; k < d2; k += NT) qd[k] = dc[k];
}
// k_store_d for the LPs list[0..n) of a view (the records of an unpark pass)
__global__ void k_store_d_list(LpView L, BatchView Bv, const int *list, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if ((int)blockIdx.y >= n || j >= L.ld) return;
    const int b = list[blockIdx.y];
    L.T[(size_t)Bv.dst[b] * L.slotT + (size_t)L.M * L.ld + j] = Bv.dcur[(size_t)b * L.ld + j];
}

// ---- k_flush: the HBM-bound kernel.  Persistent grid over (LP of the work list x row tile).  Every row of the stored
//      tableau (the parent's slot on the first pass of a solve) is read once, the pending pivots are applied to it in order
//        row r_s:  T[r][j] = -prow_s[j] * p_s (j != q_s),  T[r][q_s] = p_s
//        others:   T[i][j] -= f_si * prow_s[j] (j != q_s), T[i][q_s] = f_si          (f_si from k_select)
//      and the row is written to the LP's own slot; with MODE_REFRESH beta_i = T_i . xN is recomputed from the finished row.
//      Algorithmic traffic of one pass: one read + one write of the tableau, whatever the number of pending pivots. ----
//      wide != 0 (rows of more than ~3000 columns: KP pivot rows do not fit in LDS): the pivot rows are read from global
//      memory instead -- every row tile of an LP reads the same KP rows, which the L2 / MALL serve after the first tile. ----
//      Workgroup size: NT threads, or NT_BIG where the KP pivot rows take so much LDS that fewer than 3 workgroups fit on a CU
//      (rows of more than ~850 columns): with 4 waves per CU the pass is latency-bound (S-degenerate, 2011 columns: 1.8 TB/s);
//      16 waves share one copy of the rows instead.
template <bool WIDE>
__global__ __launch_bounds__(NT_BIG) void k_flush(LpView L, BatchView Bv, int it, int tiles, int tr /* rows per work item: 8 .. 128 */)
{
    const int NT = (int)blockDim.x;
    extern __shared__ double s_rows[];           // KP pivot rows
    __shared__ PivDesc s_pd[KP];
    const int nitems = Bv.nwork[it] * tiles;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ld = L.ldt, ld2 = ld >> 1;         // (row length of the slot matrix: the tableau, or B^-1 in the revised form)
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int b = Bv.work[item / tiles], tile = item % tiles;
        const int np = Bv.npend[b];
        const bool refresh = Bv.mode[b] == MODE_REFRESH;
        const int slot = Bv.dst[b];
        const double *Tin = L.T + (size_t)(Bv.flushed[b] ? slot : Bv.src[b]) * L.slotT;
        double *T = L.T + (size_t)slot * L.slotT;
        double *beta = L.beta + (size_t)slot * L.Mp1p;
        const double *pcol0 = Bv.pcol + (size_t)b * KP * L.Mp1p;
        const double *rowsg = Bv.prow + (size_t)b * KP * ld;
        {
            const double2 *g = reinterpret_cast<const double2 *>(Bv.prow + (size_t)b * KP * ld);
            double2 *s2 = reinterpret_cast<double2 *>(s_rows);
            if (!WIDE) for (int j2 = threadIdx.x; j2 < np * ld2; j2 += NT) s2[j2] = g[j2];
            if (threadIdx.x < np) s_pd[threadIdx.x] = Bv.desc[(size_t)b * KP + threadIdx.x];
        }
        __syncthreads();
        const double2 *x2 = reinterpret_cast<const double2 *>(L.rev ? Bv.uvec + (size_t)b * ld : L.xN + (size_t)slot * ld);      // (rev: beta = B^-1 uvec, k_rev_u)
        const bool same = Tin == T;
        for (int rr = wave; rr < tr; rr += NT / WAVE) {
            const int i = tile * tr + rr;
            if (i >= L.mrows) break;
            double f[KP];
            bool isr[KP], any = false;
#pragma unroll
            for (int s = 0; s < KP; s++) {
                isr[s] = s < np && i == s_pd[s].r;
                f[s] = (s < np && !isr[s]) ? pcol0[(size_t)s * L.Mp1p + i] : 0.0;
                any |= isr[s] || f[s] != 0.0;
            }
            if (!any && same && !refresh) continue;               // row untouched by the pending pivots and already in place
            const double2 *t_in = reinterpret_cast<const double2 *>(Tin + (size_t)i * ld);
            double2 *t_out = reinterpret_cast<double2 *>(T + (size_t)i * ld);
            double acc = 0.0;
            for (int j2 = lane; j2 < ld2; j2 += WAVE) {
                double2 v = t_in[j2];
#pragma unroll
                for (int s = 0; s < KP; s++) {
                    if (s >= np) break;
                    const double2 pr = WIDE ? reinterpret_cast<const double2 *>(rowsg + (size_t)s * ld)[j2] : reinterpret_cast<const double2 *>(s_rows + (size_t)s * ld)[j2];
                    const int q2 = L.rev ? -1 : s_pd[s].q >> 1, qodd = s_pd[s].q & 1;       // (B^-1 has no column swap)
                    if (isr[s]) { const double p = s_pd[s].p; v.x = -pr.x * p; v.y = -pr.y * p; if (j2 == q2) { if (qodd) v.y = p; else v.x = p; } }
                    else { const double fs = f[s]; v.x = fma(-fs, pr.x, v.x); v.y = fma(-fs, pr.y, v.y); if (j2 == q2) { if (qodd) v.y = fs; else v.x = fs; } }
                }
                t_out[j2] = v;
                if (refresh) { const double2 x = x2[j2]; acc = fma(v.x, x.x, acc); acc = fma(v.y, x.y, acc); }
            }
            if (refresh) { acc = wave_sum(acc); if (lane == 0) beta[i] = acc; }
        }
        __syncthreads();          // the pivot rows in LDS are reused by the next work item
    }
}

// ---- solves that ended without a pivot never left the parent's slot (see k_init): give them their own copy ----
__global__ void k_list_unpivoted(BatchView Bv, int B, int slot_of_count)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (slot_of_count < 0 || !Bv.flushed[b]) && Bv.src[b] != Bv.dst[b]) Bv.work[atomicAdd(&Bv.nwork[slot_of_count < 0 ? -slot_of_count : slot_of_count], 1)] = b;
}
__global__ __launch_bounds__(NT) void k_copy_unpivoted(LpView L, BatchView Bv, int slot_of_count, int tiles)
{
    const int nitems = Bv.nwork[slot_of_count] * tiles;
    const int ld2 = L.ldt >> 1;
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int b = Bv.work[item / tiles], tile = item % tiles;
        const double2 *s = reinterpret_cast<const double2 *>(L.T + (size_t)Bv.src[b] * L.slotT);
        double2 *d = reinterpret_cast<double2 *>(L.T + (size_t)Bv.dst[b] * L.slotT);
        const int i0 = tile * TR, i1 = min(i0 + TR, L.M);            // row M is already there
        for (size_t k = (size_t)i0 * ld2 + threadIdx.x; k < (size_t)i1 * ld2; k += NT) d[k] = s[k];
    }
}

// ---- getters ----
__global__ void k_get(LpView L, const int *slots, int B, int first, int cnt, int what, double *out)
{
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * cnt) return;
    int b = idx / cnt, k = first + idx % cnt;
    int slot = slots[b];
    int p = L.pos[(size_t)slot * (L.M + L.N) + k];
    double v;
    if (what == 0) v = p >= 0 ? L.beta[(size_t)slot * L.Mp1p + p] : L.xN[(size_t)slot * L.ld + (-1 - p)];
    else v = p >= 0 ? 0.0 : (L.rev ? L.dsl[(size_t)slot * L.ld + (-1 - p)] : L.T[(size_t)slot * L.slotT + (size_t)L.M * L.ld + (-1 - p)]);
    out[idx] = v;
}
__global__ void k_get_obj(LpView L, const int *slots, int B, double c0, double *out)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[b] = L.beta[(size_t)slots[b] * L.Mp1p + L.M] + c0;
}
// ---- k_ray (bslv_lpq_set_rays): the Farkas vector or recession direction of every LP of the batch that concluded with one in hand
// (the ray record in Bv.stall, see RAY_REC) -> the ray store of its slot, in the engine's own indices; kind NONE for every other LP.
// One workgroup per LP, once after the rounds of the call.  With x_B = T x_N (T = -B^-1 N: what row[] and pc[] hold a row / column of)
//   RAY_ROW  basic variable k = bh[r] below its lower bound:  z_k = 1, z_{nh[j]} = -row[j];  above its upper bound: the negative
//   RAY_P1   z_{bh[i]} = -sg_i (sg = infeas_sign: -1 below), z_{nh[j]} = d1[j] = sum_i sg_i T[i][j]
//   RAY_DIR  delta_{nh[q]} = dir, delta_{bh[i]} = pc[i] dir
// then every entry is divided by the largest absolute entry (a value: which entry holds it does not matter; ties need no rule).
// THE VECTORS ARE STILL THERE: an LP whose status has left ST_RUNNING is skipped by every selection at its first line (select_once,
// select_once_cached), so row[] (prow at the record's pending count, or trow in the revised form -- select_once_cached stores it too), pc[]
// and dper stand as the concluding selection left them; k_flush and k_park_copy only READ prow / pcol / desc, k_rev_u writes uvec / xfull,
// the refactorisation during a solve lists running LPs only, and the tie phases (which run after this kernel) take OPTIMAL LPs only.
// The heads bh / nh of the slot follow committed pivots alone.
struct RayView { int *kind; double *ray; int *stat; };      // [slots], [slots][M + N]; [3] of the call: FARKAS stored, DIRECTION stored, conclusions without a ray
__global__ __launch_bounds__(NT) void k_ray(LpView L, BatchView Bv, RayView R, int B)
{
    __shared__ double sv[NT / WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;
    const int slot = Bv.dst[b], st = Bv.status[b], rec = Bv.stall[b], M = L.M, N = L.N;
    const bool has = (st == BSLV_LP_INFEASIBLE || st == BSLV_LP_UNBOUNDED) && (rec & RAY_REC);
    if (!has) {
        if (tid == 0) { R.kind[slot] = BSLV_LP_RAY_NONE; if (st == BSLV_LP_INFEASIBLE || st == BSLV_LP_UNBOUNDED) atomicAdd(&R.stat[2], 1); }
        return;
    }
    const int what = rec & 3, np = min((rec >> 3) & 15, KP - 1), idx = (rec >> 7) & (RAY_IDX_MAX - 1);
    const double sgn = (rec & 4) ? 1.0 : -1.0;
    const double *row = L.rev ? Bv.trow + (size_t)b * L.ld : Bv.prow + ((size_t)b * KP + np) * L.ld;
    const double *pc = Bv.pcol + ((size_t)b * KP + np) * L.Mp1p, *d1 = Bv.dper + (size_t)b * L.ld;
    const int *bh = L.bh + (size_t)slot * M, *nh = L.nh + (size_t)slot * N;
    double *z = R.ray + (size_t)slot * (M + N);
    // (every vector is loaded whatever the record says -- all three are the batch's own, allocated in both forms -- and the entry is a
    // SELECT among the three rules: a branch on `what` inside these loops left the index of the store undefined on the RAY_DIR path in the
    // code the compiler made of it, and the first objective batch with an unbounded LP wrote to a wild address)
    const bool is_row = what == RAY_ROW, is_p1 = what == RAY_P1;
    double amax = 0.0;
    for (int i = tid; i < M; i += NT) {
        const double c = pc[i];
        const int k = bh[i];
        const double v_row = i == idx ? sgn : 0.0, v_p1 = c == 0.0 ? 0.0 : -c, v_dir = c * sgn;
        const double v = is_row ? v_row : (is_p1 ? v_p1 : v_dir);
        z[k] = v;
        amax = fmax(amax, fabs(v));
    }
    for (int j = tid; j < N; j += NT) {
        const double a = row[j], d = d1[j];
        const int k = nh[j];
        const double v_dir = j == idx ? sgn : 0.0;
        const double v = is_row ? -sgn * a : (is_p1 ? d : v_dir);
        z[k] = v;
        amax = fmax(amax, fabs(v));
    }
    amax = block_max(amax, sv);      // (its barriers also put z in front of the whole workgroup)
    if (amax > 0.0 && amax < INFINITY) for (int k = tid; k < M + N; k += NT) z[k] = z[k] / amax;
    if (tid == 0) {
        const int kind = what == RAY_DIR ? BSLV_LP_RAY_DIRECTION : BSLV_LP_RAY_FARKAS;
        R.kind[slot] = kind;
        atomicAdd(&R.stat[kind == BSLV_LP_RAY_FARKAS ? 0 : 1], 1);
    }
}
// the kinds and vectors of the listed slots, gathered for one copy to the host (bslv_lpq_get_ray)
__global__ void k_ray_get(RayView R, const int *slots, int B, int nv, int *kind, double *out)
{
    const size_t n = (size_t)B * nv, idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int b = (int)(idx / nv), k = (int)(idx % nv), slot = slots[b];
    if (k == 0) kind[b] = R.kind[slot];
    if (out) out[idx] = R.kind[slot] == BSLV_LP_RAY_NONE ? 0.0 : R.ray[(size_t)slot * nv + k];
}

__global__ void k_std_heads(LpView L, int slot)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L.M) { L.bh[(size_t)slot * L.M + i] = i; L.pos[(size_t)slot * (L.M + L.N) + i] = i; }
    if (i < L.N) {
        L.nh[(size_t)slot * L.N + i] = L.M + i;
        L.pos[(size_t)slot * (L.M + L.N) + L.M + i] = -1 - i;
        L.nstat[(size_t)slot * L.N + i] = NS_L;
    }
    if (i < L.ld) L.xN[(size_t)slot * L.ld + i] = 0.0;
    if (i < L.Mp1p) L.beta[(size_t)slot * L.Mp1p + i] = 0.0;
}

// ---- REFACTORISATION of the revised form (bslv_lpq_refactor): B^-1 of a slot rebuilt from its basis heads alone ----
// The target X satisfies X K[:, bh] = I with K = [I | -A] (see LpView).  It is reached by REPLAYING the basis on the engine's own
// machinery: the slot starts as the identity (the all-slack basis, row i <-> auxiliary variable i), the structural basic variables of
// the target enter one after the other in ascending variable id, each on the row partial pivoting chooses -- the largest |v_i| of the
// column v = X K_k (fetch_col_revised, through the pending steps) among the rows whose auxiliary variable is nonbasic in the target and
// that have not been pivoted yet, ties to the smallest i -- and every step is recorded as an ordinary pending pivot (PivDesc, rho = row
// r of X as virt_entry_b sees it, multipliers v_i / v_r), KP of them between two passes of k_flush.  Nothing numeric in the slot is
// read before the identity is written, no atomics enter the arithmetic and every reduction has a fixed order: the result is a function
// of the heads and the model.  One workgroup per LP and selection; no helper workgroups, no mailbox, no polling loop: a replay step
// needs the column only.
// cnt: [B][4] = structural basics to enter, entered so far, state (RFX_*), unused; enter / rowvar / elig: [B][M]
constexpr int RFX_RUN = 0, RFX_SINGULAR = 2, RFX_HEADS = 3;
struct RfxView { int *enter, *rowvar, *elig, *cnt; const double *cost; };
__global__ __launch_bounds__(NT) void k_rfx_setup(LpView L, BatchView Bv, RfxView R, int n)
{
    __shared__ int s_cnt[NT];
    __shared__ int s_ne;
    const int b = blockIdx.x, tid = threadIdx.x, M = L.M, N = L.N;
    if (b >= n) return;
    const int slot = Bv.dst[b];
    const int *pos = L.pos + (size_t)slot * (M + N);
    int *enter = R.enter + (size_t)b * M, *rowvar = R.rowvar + (size_t)b * M, *elig = R.elig + (size_t)b * M;
    // the structural basic variables in ascending id: thread t counts its stretch of the columns, a scan places it
    const int chunk = (N + NT - 1) / NT, j0 = min(N, tid * chunk), j1 = min(N, j0 + chunk);
    int c = 0;
    for (int j = j0; j < j1; j++) c += pos[M + j] >= 0;
    s_cnt[tid] = c;
    if (tid == 0) s_ne = 0;
    __syncthreads();
    if (tid == 0) { int o = 0; for (int t = 0; t < NT; t++) { const int v = s_cnt[t]; s_cnt[t] = o; o += v; } }
    __syncthreads();
    int o = s_cnt[tid];
    for (int j = j0; j < j1; j++) if (pos[M + j] >= 0) { if (o < M) enter[o] = M + j; o++; }
    __shared__ int s_k;
    if (tid == NT - 1) s_k = o;                 // (the last stretch ends where the list does)
    // the eligible rows: the auxiliary variable is nonbasic in the target basis
    int ne = 0;
    for (int i = tid; i < M; i += NT) { const int e = pos[i] < 0; elig[i] = e; rowvar[i] = i; ne += e; }
    if (ne) atomicAdd(&s_ne, ne);
    __syncthreads();
    if (tid == 0) {
        int *cnt = R.cnt + (size_t)b * 4;
        cnt[0] = s_k; cnt[1] = 0; cnt[2] = (s_k == s_ne && s_k <= M) ? RFX_RUN : RFX_HEADS; cnt[3] = 0;
        Bv.status[b] = ST_RUNNING; Bv.iters[b] = 0; Bv.mode[b] = MODE_NONE; Bv.verified[b] = 0;
        Bv.npend[b] = 0; Bv.pflags[b] = 0; Bv.stall[b] = 0; Bv.flushed[b] = 1;      // (in place: every pass reads and writes the slot itself)
    }
}
__global__ void k_rfx_identity(LpView L, BatchView Bv, RfxView R, int n)
{
    const int b = blockIdx.y;
    if (b >= n || R.cnt[(size_t)b * 4 + 2] != RFX_RUN) return;
    double *X = L.T + (size_t)Bv.dst[b] * L.slotT;
    const size_t total = (size_t)L.M * L.ldt;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (size_t)gridDim.x * blockDim.x) X[k] = (int)(k / L.ldt) == (int)(k % L.ldt) ? 1.0 : 0.0;
}
// up to nsel replay steps of LP b by one workgroup (256 or 1024 threads)
__global__ __launch_bounds__(NT_BIG) void k_rfx_select(LpView L, BatchView Bv, RfxView R, int n, int nsel)
{
    __shared__ double sv[NT_BIG / WAVE];
    __shared__ int si[NT_BIG / WAVE];
    const int b = blockIdx.x, tid = threadIdx.x, NT = (int)blockDim.x, M = L.M, ldt = L.ldt;
    if (b >= n) return;
    int *cnt = R.cnt + (size_t)b * 4, *elig = R.elig + (size_t)b * M;
    const int slot = Bv.dst[b];
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();              // (what thread 0 wrote for the LP in the last step is read by all)
        const int np = Bv.npend[b], t = cnt[1];
        if (cnt[2] != RFX_RUN || np >= KP || t >= cnt[0]) break;
        SelCtx c = sel_ctx(L, Bv, b, np, slot, slot);
        c.nh = R.enter + (size_t)b * M;        // (fetch_col_revised takes the variable of "column" t from here: the t-th to enter)
        const int kq = c.nh[t];
        fetch_col_revised(L, c, t);            // pc = -(X K_kq) through the pending steps: the tableau column, as a pivot of the engine has it
        __syncthreads();
        double *pc = c.pc;
        ValIdx best{-1.0, -1};
        double cmax = 0.0;
        for (int i = tid; i < M; i += NT) {
            const double a = fabs(pc[i]);
            cmax = fmax(cmax, a);
            if (elig[i]) best = better_max(best, ValIdx{a, i});
        }
        best = block_argmax(best, sv, si);
        cmax = block_max(cmax, sv);
        const int r = best.i;
        if (r < 0 || !(best.v > TOL_PIV * (1.0 + cmax))) { if (tid == 0) cnt[2] = RFX_SINGULAR; break; }
        const double p = 1.0 / pc[r];
        double *rho = c.prow0 + (size_t)np * ldt;
        for (int i = tid; i < ldt; i += NT) rho[i] = i < M ? virt_entry_b(c.T0[(size_t)r * ldt + i], r, i, np, c.pd, c.prow0, c.pcol0, ldt, L.Mp1p) : 0.0;
        __syncthreads();                       // (everyone has read pc[r])
        for (int i = tid; i <= M; i += NT) pc[i] = (i == r || i == M) ? 0.0 : pc[i] * p;
        if (tid == 0) {
            PivDesc d;
            d.r = r; d.q = -1; d.p = p; d.pbeta = 0.0; d.enter_val = 0.0;
            Bv.desc[(size_t)b * KP + np] = d;
            elig[r] = 0; R.rowvar[(size_t)b * M + r] = kq;
            cnt[1] = t + 1; Bv.npend[b] = np + 1; Bv.mode[b] = MODE_PIVOT;
        }
    }
}
// after the last pass: the heads of the basic variables follow the rows they ended in; a slot that is done asks for the refresh pass
__global__ __launch_bounds__(NT) void k_rfx_finish(LpView L, BatchView Bv, RfxView R, int n)
{
    const int b = blockIdx.x, M = L.M;
    if (b >= n) return;
    int *cnt = R.cnt + (size_t)b * 4;
    const bool ok = cnt[2] == RFX_RUN && cnt[1] == cnt[0] && Bv.npend[b] == 0;
    __syncthreads();
    if (!ok) { if (threadIdx.x == 0) { if (cnt[2] == RFX_RUN) cnt[2] = RFX_SINGULAR; Bv.npend[b] = 0; Bv.mode[b] = MODE_NONE; Bv.status[b] = BSLV_LP_UNDEFINED; } return; }
    const int slot = Bv.dst[b];
    int *bh = L.bh + (size_t)slot * M, *pos = L.pos + (size_t)slot * (M + L.N);
    const int *rowvar = R.rowvar + (size_t)b * M;
    for (int i = threadIdx.x; i < M; i += NT) { const int k = rowvar[i]; bh[i] = k; pos[k] = i; }
    if (threadIdx.x == 0) Bv.mode[b] = MODE_REFRESH;
}
// The explicit rebuild's price: d_j = c[nh_j] - y . K[nh_j] into dcur for the engine's own cost vector, by column slices as k_rev_price
// has them.  NOT k_per_price with the identity list: that one adds per_cost to every column, 0.0 for an auxiliary variable, and
// (-0.0) + 0.0 = +0.0 -- here an auxiliary column keeps what rev_row_slice wrote (-y_k, -0.0 where y_k is an exact zero), and the
// getters hand dsl out as it is.  It also prices an LP whose replay failed (y = 0 then), which k_per_price leaves alone.
__global__ __launch_bounds__(NT) void k_rfx_price(LpView L, BatchView Bv, RfxView R, int n)
{
    const int b = blockIdx.y, M = L.M;
    if (b >= n) return;
    const int *nh = L.nh + (size_t)Bv.dst[b] * L.N;
    double *dc = Bv.dcur + (size_t)b * L.ld;
    rev_row_slice(L, Bv.uvec + (size_t)b * L.ldt, nh, dc, blockIdx.x, gridDim.x);        // dc[j] = -(y . K[nh_j]), 0 on the padding (barrier at its end)
    for (int j = blockIdx.x + gridDim.x * threadIdx.x; j < L.N; j += gridDim.x * blockDim.x) {
        const int k = nh[j];
        if (k >= M) dc[j] += R.cost[k - M + 1];
    }
}
// test support (bslv_lpq_debug_perturb_inverse): a deterministic stand-in for drift
__global__ void k_rfx_perturb(LpView L, int slot, double rel)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t)L.M * L.M) return;
    const int i = (int)(k / L.M), c = (int)(k % L.M);
    L.T[(size_t)slot * L.slotT + (size_t)i * L.ldt + c] *= 1.0 + rel * (1.0 + hash01(i * L.M + c));
}

// ---- the AGE of a slot's matrix, and the PERIODIC refactorisation (bslv_lpq_set_refactor_period) ----
// age[slot]: rank-1 steps applied to the slot's B^-1 since it was last built from the identity.  A solve carries, per LP of its batch,
// age0[b] = (age of the matrix the LP stands on when it was last built or inherited) - (the LP's pivots at that moment), so that the age
// of the LP's matrix is age0[b] + iters[b] wherever nothing is pending: k_age_begin takes it from the parent, a refactorisation inside
// the solve sets it to -iters[b] (k_per_resume), k_age_end leaves the sum in the LP's own slot.  Maintained in every solve of the revised
// form, period or not; the default kernels do not know about it.  (iters[] is what the selection counts: a primal step in which the entering
// variable only switches bound counts as well, although no step is applied -- the age never underestimates.)
__global__ void k_age_begin(BatchView Bv, const long long *age, long long *age0, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) age0[b] = age[Bv.src[b]];
}
__global__ void k_age_end(BatchView Bv, long long *age, const long long *age0, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) age[Bv.dst[b]] = age0[b] + Bv.iters[b];
}
__global__ void k_age_zero(const int *slots, int n, long long *age)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) age[slots[k]] = 0;
}
// The LPs of the active list that are DUE: running, nothing pending, age >= K -- in the order of the list (ONE workgroup, a scan: the
// replay index of an LP is a function of the batch).  stat[0] = their number; stat[1] = the largest age met so far among the LPs of the
// list that a selection saw or will see at that age (at the start of a call the due ones and the ones k_prep refused are left out: no
// selection is made on them as they stand).  Called where the host reads the status vector, after the pass of the round.
__global__ __launch_bounds__(NT) void k_per_due(BatchView Bv, const int *active, int nact, const long long *age0, long long K, int at_start, int *due, long long *stat)
{
    __shared__ int s_cnt[NT];
    __shared__ long long s_max[NT];
    const int tid = threadIdx.x;
    const int chunk = (nact + NT - 1) / NT, k0 = min(nact, tid * chunk), k1 = min(nact, k0 + chunk);
    int c = 0;
    long long mx = 0;
    for (int k = k0; k < k1; k++) {
        const int b = active[k];
        const long long a = age0[b] + Bv.iters[b];
        const bool run = Bv.status[b] == ST_RUNNING, is_due = run && Bv.npend[b] == 0 && a >= K;
        c += is_due;
        if (!at_start || (run && !is_due)) mx = max(mx, a);
    }
    s_cnt[tid] = c; s_max[tid] = mx;
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        long long m = stat[1];
        for (int t = 0; t < NT; t++) { const int v = s_cnt[t]; s_cnt[t] = o; o += v; m = max(m, s_max[t]); }
        stat[0] = o; stat[1] = m;
    }
    __syncthreads();
    int o = s_cnt[tid];
    for (int k = k0; k < k1; k++) {
        const int b = active[k];
        if (Bv.status[b] == ST_RUNNING && Bv.npend[b] == 0 && age0[b] + Bv.iters[b] >= K) due[o++] = b;
    }
}
// The replay (k_rfx_*) runs on a view of its own, Rv, whose LP k is LP due[k] of the batch: in place on that LP's dst slot.  Everything
// else of Rv's LP k is k_rfx_setup's to set.
__global__ void k_per_setup(BatchView Bv, BatchView Rv, const int *due, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int slot = Bv.dst[due[k]];
    const_cast<int *>(Rv.src)[k] = slot; const_cast<int *>(Rv.dst)[k] = slot;
}
// the cost of variable k in LP b of the batch: the engine's vector, in an objective batch with the LP's own values on their range
__device__ __forceinline__ double per_cost(const LpView &L, const BatchView &Bv, const double *cost, const int b, const int k)
{
    if (L.objmode) { const int t = k - L.cfirst; if (t >= 0 && t < L.ccnt) return Bv.cvals[(size_t)b * L.ccnt + t]; }
    return k >= L.M ? cost[k - L.M + 1] : 0.0;
}
// y of a rebuilt inverse, for both callers of the replay.  The periodic refactorisation runs it on its own view Rv with the list of the
// due LPs; the explicit rebuild (refactor_impl) with Rv = Bv and the identity list, in a batch without objective values (objmode 0),
// where per_cost is the engine's cost vector (cost[0] is the constant, auxiliary variables cost nothing): the same sums in the same order
// as the kernel the explicit rebuild had of its own.
// y = sum over the rows i of c[bh_i] X[i, :] for the LP's OWN cost, rows in ascending order, zero costs skipped, into Rv's scratch vector
// uvec (free until k_rev_u): what rev_price_y does for the cost range of an objective batch.  Grid (column blocks, n).
__global__ void k_per_y(LpView L, BatchView Bv, BatchView Rv, const int *due, const double *cost, int n)
{
    const int k = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x, M = L.M;
    if (k >= n || c >= L.ldt) return;
    double v = 0.0;
    if (c < M && Rv.mode[k] == MODE_REFRESH) {
        const int slot = Rv.dst[k], b = due[k];
        const int *bh = L.bh + (size_t)slot * M;
        const double *X = L.T + (size_t)slot * L.slotT;
        for (int i = 0; i < M; i++) {
            const double ck = per_cost(L, Bv, cost, b, bh[i]);
            if (ck != 0.0) v = fma(ck, X[(size_t)i * L.ldt + c], v);
        }
    }
    Rv.uvec[(size_t)k * L.ldt + c] = v;
}
// The LP goes on: its TRUE reduced costs d_j = c[nh_j] - y . K[nh_j] from the rebuilt inverse, by column slices as k_rfx_price has
// them, into the batch's dcur; a perturbed row keeps its offsets to the true one, dper_new = d_new + (dper_old - d_old).  Rv's dcur
// gets the row too: k_rev_u, which runs on Rv next, takes beta[M] = d . x_N from there.  A replay that failed leaves the LP's vectors alone.
// (An LP in phase 1 keeps its pricing vector d1 in dper, which is no perturbed cost row and must not be shifted like one: PF_PERT and
// PF_PHASE1 exclude each other -- phase1_prepare clears the perturbation bits where it sets PF_PHASE1, and no perturbation starts from a
// primal step -- so `pert` is false for it; k_per_resume has d1 rebuilt instead.)
__global__ __launch_bounds__(NT) void k_per_price(LpView L, BatchView Bv, BatchView Rv, const int *due, const double *cost, int n)
{
    const int k = blockIdx.y;
    if (k >= n || Rv.mode[k] != MODE_REFRESH) return;
    const int b = due[k];
    const int *nh = L.nh + (size_t)Rv.dst[k] * L.N;
    double *dn = Rv.dcur + (size_t)k * L.ld;
    rev_row_slice(L, Rv.uvec + (size_t)k * L.ldt, nh, dn, blockIdx.x, gridDim.x);        // dn[j] = -(y . K[nh_j]), 0 on the padding (barrier at its end)
    double *dc = Bv.dcur + (size_t)b * L.ld, *dp = Bv.dper + (size_t)b * L.ld;
    const bool pert = Bv.pflags[b] & PF_PERT;
    for (int j = blockIdx.x + gridDim.x * threadIdx.x; j < L.N; j += gridDim.x * blockDim.x) {
        const double d = dn[j] + per_cost(L, Bv, cost, b, nh[j]);
        if (pert) dp[j] = d + (dp[j] - dc[j]);
        dc[j] = d; dn[j] = d;
    }
}
// after the refresh pass of the replay: LP due[k] has its own, fresh matrix and a fresh beta, or ends UNDEFINED (singular basis; the
// host resets its slot when the call is over).  res[k]: the replay's pivots, or -1.
__global__ void k_per_resume(BatchView Bv, BatchView Rv, RfxView R, const int *due, int n, long long *age0, int *res)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int b = due[k];
    if (R.cnt[(size_t)k * 4 + 2] == RFX_RUN && Rv.status[k] == ST_RUNNING) {
        Bv.flushed[b] = 1; Bv.verified[b] = (Bv.verified[b] & 2) | 1;
        // (phase 1, revised form: the replay has moved the basic variables to other rows; the signs and d1 are rebuilt from the new
        // inverse before the next selection)
        { const int pf = Bv.pflags[b]; if (pf & PF_PHASE1) Bv.pflags[b] = pf | PF_P1_STALE; }
        age0[b] = -(long long)Bv.iters[b];
        res[k] = R.cnt[(size_t)k * 4 + 1];
    } else { Bv.status[b] = BSLV_LP_UNDEFINED; Bv.mode[b] = MODE_NONE; res[k] = -1; }
}

}  // namespace bslv

using namespace bslv;

// What the engine keeps for a Devex rule: the reference norms and counters of a batch (NormView; allocated by the first batch that runs
// under the rule, for Bcap LPs), the size of the last batch that ran under the rule (0: none did), the counters of the last solve call
struct DevexNorms {
    double *norm_d = nullptr; int *stat_d = nullptr; int Bcap = 0;
    int B = 0;
    long last[3] = {0, 0, 0};
    NormView view() const { return NormView{norm_d, stat_d}; }
};
// What the engine keeps for a tie phase (bslv_lpq_set_canonical; objective batches: bslv_lpq_set_canonical_obj): the switch, the
// direction (host / device, room for dir_cap values), the per-LP state of a batch (TieView; for Bcap LPs), the counters of the last batch
// the phase could have run in (every solve_batch; every solve_batch_obj)
struct TiePhase {
    bool on = false;
    std::vector<double> dir;
    double *dir_d = nullptr; size_t dir_cap = 0;
    double *g_d = nullptr; int *state_d = nullptr, *iters_d = nullptr, *stat_d = nullptr; int Bcap = 0;
    long last[4] = {0, 0, 0, 0};
    TieView view(int cap) const { return TieView{dir_d, g_d, state_d, iters_d, stat_d, cap}; }
};
// The counters of a batch, as solve_batch_impl gathers them: lock-step rounds, pivots, (LP, pass) pairs (how many tableaux k_flush read
// and wrote), k_flush launches (one per round; a pass made on request, bslv_lpq_materialise, adds itself to the last call's), HIP-event
// time of the passes (set_profile) and host wall clock, the extended selection's five counters, phase 1: LPs that entered it, its
// iterations, rebuilds of its pricing vector
struct BatchStats {
    int iters = 0;
    long pivots = 0, passes = 0, launches = 0;
    double update_ms = 0, total_ms = 0;
    long ext[5] = {0, 0, 0, 0, 0}, p1[3] = {0, 0, 0};
    long objm[4] = {0, 0, 0, 0};      // an objective batch under DUAL / REPAIR: LPs started dual, variables moved at the start, LPs handed to the primal start, dual pivots
    void add(const BatchStats &o)
    {
        for (int k = 0; k < 4; k++) objm[k] += o.objm[k];
        iters += o.iters; pivots += o.pivots; passes += o.passes; launches += o.launches; update_ms += o.update_ms; total_ms += o.total_ms;
        for (int k = 0; k < 5; k++) ext[k] += o.ext[k];
        for (int k = 0; k < 3; k++) p1[k] += o.p1[k];
    }
};
// ... and of a solve call: its first batch stored, the re-solves of the rescue added (solve_batch_impl); beside them what the call adds
// to where it is produced, zeroed by solve_batch_rescue: the refactorisations (rfx; bslv_lpq_refactor: of that call), the periodic
// refactorisation (per; [3] is a maximum) and the ray store (ray)
struct CallStats : BatchStats {
    long rfx[4] = {0, 0, 0, 0}, per[4] = {0, 0, 0, 0}, ray[3] = {0, 0, 0};
};

struct bslv_lpq {
    LpView L{};
    int slots = 0;
    double c0 = 0;
    hipStream_t stream = nullptr;
    double *Tstd = nullptr;           // (M+1) x ld image of [A ; cost] (tableau form)
    // revised form: A once as CSC and CSR, the cost vector, per-slot reduced costs, per-LP scratch
    int *cptr_d = nullptr, *cidx_d = nullptr, *rptr_d = nullptr, *ridx_d = nullptr; double *cval_d = nullptr, *rval_d = nullptr, *cost_d = nullptr, *dsl_d = nullptr;
    unsigned long long *dbg_d = nullptr;
    // LAZY tableaux (bslv_lpq_set_lazy; the Benson driver's mode): see bslv_lpq_materialise
    bool lazy = false, lazy_open = false;          // lazy_open: the last batch left slots without their tableau
    std::vector<int> last_dst;                     // dst slots of the last batch (host copy)
    int *list_d = nullptr; int listcap = 0;
    long lazy_skipped = 0, lazy_materialised = 0;  // LPs whose pass was skipped / asked for afterwards (totals)
    double lazy_ms = 0;                            // host wall clock spent in bslv_lpq_materialise and bslv_lpq_park (total)
    std::vector<int> park_src, last_npend;         // src and npend of the last batch as the solve left them (host copies, lazy with park on), behind npend ...
    size_t last_flushed_at = 0;                    // ... from this index on: flushed
    // PARKED passes (bslv_lpq_park): see the comment above park_alloc
    struct Park {
        bool on = true, failed = false;            // the switch (bslv_lpq_set_park, BSLV_LP_PARK); the store could not be allocated: park() materialises
        int cap = 0;                               // records of the store (one per pool slot), 0: not allocated yet
        int *src = nullptr, *dst = nullptr, *npend = nullptr, *flushed = nullptr, *mode = nullptr, *ver = nullptr, *work = nullptr, *nwork = nullptr;
        PivDesc *desc = nullptr; double *prow = nullptr, *pcol = nullptr, *dcur = nullptr;
        int *pairs_d = nullptr, *pairs_h = nullptr;      // (batch index, record) of a park call (device / pinned)
        int *list_d = nullptr, *list_h = nullptr;        // records of an unpark pass (device / pinned)
        std::vector<int> free_recs, live, pos_in_live;   // free records; records in use, and where each of them stands in `live`
        std::vector<int> rec_of_slot;                    // slot -> its record, or -1
        std::vector<int> slot_of, src_of, flushed_of;    // per record: its slot, the slot its pass reads when flushed_of is 0
        std::vector<char> mark, listed;                  // scratch per slot / per record (zero between calls)
        bool list_inflight = false, pairs_inflight = false;      // the pinned lists may still be read by a copy on the stream (cleared where a batch has waited for it)
        long stats[4] = {0, 0, 0, 0};                    // parked, unparked for a child, unparked because their source was about to be overwritten, dropped unused
        long pre_passes = 0, pre_launches = 0;           // unpark passes since the last batch: they count in the statistics of the batch they precede
        std::vector<std::pair<hipEvent_t, hipEvent_t>> pre_ev;      // ... and their events (set_profile)
    } park;
    double *trow_d = nullptr, *uvec_d = nullptr, *xfull_d = nullptr;
    int *hmail_d = nullptr; int launch_seq = 0;      // revised form: mailboxes of k_select's helper workgroups; launches so far
    long nnzA = 0;
    double *lb_d = nullptr, *ub_d = nullptr;
    unsigned char *art_d = nullptr;
    std::vector<double> cost;         // N+1
    // batch buffers
    int Bcap = 0;
    int *qslot_d = nullptr;           // slots of a getter call (batch-sized, like src_d)
    int *src_d = nullptr, *dst_d = nullptr, *status_d = nullptr, *iters_d = nullptr, *mode_d = nullptr, *ver_d = nullptr;
    int *work_d = nullptr, *nwork_d = nullptr; int nworkcap = 0;
    int *npend_d = nullptr, *flushed_d = nullptr; double *pcol_d = nullptr, *dcur_d = nullptr;     // delayed update (see BatchView)
    double *dper_d = nullptr; int *pflags_d = nullptr, *stall_d = nullptr, *xstat_d = nullptr;
    double *cvals_d = nullptr; size_t cvals_cap = 0;     // objective coefficients of solve_batch_obj
    // bslv_lpq_solve_batch_obj_method: the method of the objective batch in flight (PRIMAL: solve_batch_obj as it always was; the rescue's
    // re-solves included), and the call's own copy of the bounds, artificial ones added (k_obj_art)
    int call_obj_method = BSLV_LP_METHOD_PRIMAL;
    bool obj_call_dual = false;        // a DUAL / REPAIR call of bslv_lpq_solve_batch_obj_method is in flight (its polish, a PRIMAL batch, included)
    double *clb_d = nullptr, *cub_d = nullptr; unsigned char *cart_d = nullptr;
    CallStats last;                    // the counters of the last solve call (bslv_lpq_last_stats and the getters beside it)
    int method = BSLV_LP_METHOD_DUAL;  // bslv_lpq_set_method (BSLV_LP_METHOD at create)
    bool call_priced = false;               // the solve call in flight is bslv_lpq_solve_batch_method_priced: pricing / ppricing hold ITS rules until it returns
    int call_method = BSLV_LP_METHOD_DUAL;  // the method of the solve call in flight: `method`, or what bslv_lpq_solve_batch_method was given (the rescue's re-solves included)
    // dual Devex pricing (bslv_lpq_set_pricing, BSLV_LP_PRICING at create) and primal Devex pricing (bslv_lpq_set_primal_pricing,
    // BSLV_LP_PRIMAL_PRICING at create): the rule and what the engine keeps for it (DevexNorms); pdv_dst: the slots of the LPs of the
    // last batch that ran under the primal rule (bslv_lpq_last_primal_pricing_norms answers by variable)
    int pricing = BSLV_LP_PRICING_DANTZIG, ppricing = BSLV_LP_PRICING_DANTZIG;
    DevexNorms dvx, pdv;
    std::vector<int> pdv_dst;
    // the tie phases (TiePhase): of solve_batch (bslv_lpq_set_canonical) and of objective batches (bslv_lpq_set_canonical_obj), with the
    // cost range that one was set for (indices of the model as given)
    TiePhase tie, tie_obj;
    int cobj_first = 0, cobj_cnt = 0;
    // bslv_lpq_solve_batch_canonical: the direction of the call (device; on while the call runs).  The per-LP state and the counters of
    // its phase are `tie`'s, whose switch and direction the call leaves alone.  tie_call_obj: the same for
    // bslv_lpq_solve_batch_obj_canonical and `tie_obj` (the call's cost range is the batch's own, L.cfirst / L.ccnt)
    TiePhase tie_call, tie_call_obj;
    // refactorisation of the revised form (bslv_lpq_refactor, bslv_lpq_set_refactor): the switch, the marks of the last batch (device / host),
    // the replay's per-LP lists (the counters of the last solve call or explicit refactor: last.rfx)
    bool refactor_on = false;
    int *rmark_d = nullptr; std::vector<int> rmark_h; bool rmark_valid = false;
    int *rfx_i_d = nullptr, *rfx_c_d = nullptr; int rfx_Bcap = 0;
    // age of the slots' matrices (revised form: [slots], and per LP of a batch, see k_age_begin) and the periodic refactorisation
    // (bslv_lpq_set_refactor_period): the period, the replay's own batch view (see period_view) (the counters of the last solve call: last.per)
    long long *age_d = nullptr, *age0_d = nullptr;
    int period = 0;
    struct Period {
        int cap = 0, nwcap = 0;
        int *src = nullptr, *dst = nullptr, *status = nullptr, *iters = nullptr, *mode = nullptr, *ver = nullptr, *npend = nullptr, *flushed = nullptr, *pflags = nullptr, *stall = nullptr;
        int *work = nullptr, *nwork = nullptr, *iota = nullptr, *due = nullptr, *res = nullptr;
        long long *stat = nullptr;                   // [2]: k_per_due's count and largest age
        PivDesc *desc = nullptr; double *prow = nullptr, *pcol = nullptr, *dcur = nullptr, *uvec = nullptr, *xfull = nullptr;
        long passes = 0, launches = 0; double ms = 0;      // of the call at hand: the replay's (LP, pass) pairs, its k_flush launches, host wall clock
        std::vector<int> failed;                     // batch indices whose replay found the basis singular (their slots are reset when the call is over)
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;      // events around the replay's passes (set_profile)
    } per;
    // a basis loaded into a slot (bslv_lpq_load_basis, bslv_lpq_rebuild; lp_basis.inc): per LP of a call the nonbasic status (-1: basic)
    // and value of every variable, and the counters of the last call
    int *lb_nst_d = nullptr; double *lb_xv_d = nullptr; size_t lb_cap = 0;
    long last_rebuild[4] = {0, 0, 0, 0};
    // dynamic LDS (candidate sort of the bound flipping ratio test; revised form: rho) that each selection kernel may use so far, indexed as select_kernel is
    size_t select_lds_max[3][6] = {{64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024}, {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024}, {64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024, 64 * 1024}};
    size_t price_lds_max = 64 * 1024;  // ... of k_rev_price (revised form, new objective: y)
    int obj_batches = 0;               // solve_batch_obj calls so far (BSLV_LP_OBJ_UNDEFINED counts them)
    bool has_boxed = false;            // some variable outside the per-LP range has two finite, non-artificial bounds
    bool force_ext = false;            // extended selection (perturbation, primal clean-up) also without a boxed variable: bslv_lpq_set_extended,
                                       // and by itself for tableaux of 1 GiB and more (every pivot costs a millisecond there: no stalling)
    size_t flush_lds_max = 64 * 1024;  // dynamic LDS k_flush may use (raised to 144 KB at create when the runtime allows)
    int upd_grid = 32768;             // workgroups of the persistent k_flush (BSLV_UPD_GRID; 1024..32768 measured equal within 2 %)
    int *active_d = nullptr, *active_h = nullptr;       // compacted indices of the LPs still running (device / pinned)
    int *init_d = nullptr, *init_h = nullptr;           // the batch ordered by parent and its chunks for k_init_grouped: [B] order, [B] InitChunk (device / pinned, plan_init)
    std::vector<int> init_at, init_seen;                // plan_init's scratch: per slot a count / write position (zero between calls), the parents of the batch
    int last_init_parents = 0, last_init_family = 0, last_init_chunks = 0;      // distinct src slots of the last batch, its largest family; chunks k_init_grouped ran on (0: k_init ran)
    double *vlo_d = nullptr, *vup_d = nullptr, *prow_d = nullptr, *out_d = nullptr;
    size_t out_cap = 0;
    // bslv_lpq_certify (lp_certify.inc): its scratch, grown to the largest call and released with the engine; the counters of the last call
    void *cert_d = nullptr; size_t cert_cap = 0;
    long last_cert[3] = {0, 0, 0};
    // the ray store (bslv_lpq_set_rays, BSLV_LP_RAYS at create): per slot a kind and a vector of M + N doubles beside the pool (like the
    // ages: no part of bslv_lpq_slot_bytes), the call's counters on the device; the counters of the last bslv_lpq_certify_rays (of the
    // last solve call: last.ray)
    bool rays_on = false;
    int *raykind_d = nullptr, *raystat_d = nullptr; double *ray_d = nullptr;
    long last_raycert[3] = {0, 0, 0};
    PivDesc *desc_d = nullptr;
    int *status_h = nullptr;          // pinned
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evpool;
    // PRESOLVE at the boundary (round 3): a row of A with a single non-zero outside the per-LP range is a bound on that column
    // (the hypercube rows `d 0 1` of ex/example10.m:21-24 and of S-degenerate); it is folded into the column's bounds and leaves the
    // tableau.  The callers keep the model they handed over (GLPK's, bslv_lp.c:60-70,219-308): every index that crosses the
    // boundary is an index of THAT model, the primal value of a folded row is a_ij x_j, and its dual is the column's reduced cost
    // over a_ij whenever the bound the column sits on is the row's and not its own.
    struct Presolve {
        int M0 = 0, N0 = 0, nfold = 0;                 // the model as given; rows folded
        bool empty_box = false;                         // bounds set later made the box of a folded row's column empty: every LP is infeasible (the row would have said so)
        std::vector<int> row_in;                       // given row -> row of the engine's model, or -1 (folded)
        std::vector<int> fold_col;                     // given row -> column it bounds (folded rows)
        std::vector<double> fold_a;                    //              its coefficient
        std::vector<double> lb0, ub0;                  // bounds as given (M0 + N0), kept for set_bounds
        std::vector<int> lo_src, up_src;               // per column: the folded row whose bound is the tighter one, or -1 (its own)
        std::vector<double> clo, cup;                  // per column: folded bounds
        int map_var(int v) const { return v < M0 ? row_in[v] : (M0 - nfold) + (v - M0); }
    } ps;
};

static int materialise_indices(bslv_lpq *h, const int *list, int n);
static void park_release(bslv_lpq *h, int rec);
static int park_before(bslv_lpq *h, int nuse, const int *use, int nover, const int *over);
static void park_free(bslv_lpq *h);
static void period_free(bslv_lpq *h);
static int ensure_batch(bslv_lpq *h, int B)
{
    if (B <= h->Bcap) return 0;
    if (h->lazy_open) { const int rc = materialise_indices(h, nullptr, 0); if (rc) return rc; h->lazy_open = false; }      // (the buffers below hold the pending pivots of the last batch)
    int cap = std::max(B, h->Bcap * 2);
    // every pointer is cleared as it is freed: when one of the allocations below fails, destroy() and a later ensure_batch()
    // see nullptr for what is gone instead of freeing it a second time
    auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    fr(h->src_d); fr(h->dst_d); fr(h->status_d); fr(h->iters_d); fr(h->mode_d); fr(h->ver_d); fr(h->active_d); fr(h->work_d); fr(h->qslot_d); fr(h->init_d);
    fr(h->vlo_d); fr(h->vup_d); fr(h->prow_d); fr(h->desc_d); fr(h->npend_d); h->flushed_d = nullptr; fr(h->pcol_d); fr(h->dcur_d); fr(h->dper_d); fr(h->pflags_d); fr(h->stall_d);
    fr(h->trow_d); fr(h->uvec_d); fr(h->xfull_d); fr(h->hmail_d); fr(h->rmark_d); fr(h->age0_d);
    if (h->status_h) { (void)hipHostFree(h->status_h); h->status_h = nullptr; }
    if (h->active_h) { (void)hipHostFree(h->active_h); h->active_h = nullptr; }
    if (h->init_h) { (void)hipHostFree(h->init_h); h->init_h = nullptr; }
    h->Bcap = 0;
    HIP_TRY(malloc0(&h->src_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->qslot_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->dst_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->status_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->iters_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->mode_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->work_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->ver_d, cap * sizeof(int)));
    size_t vc = (size_t)std::max(1, h->L.vcnt);
    HIP_TRY(malloc0(&h->vlo_d, cap * vc * sizeof(double)));
    HIP_TRY(malloc0(&h->vup_d, cap * vc * sizeof(double)));
    HIP_TRY(malloc0(&h->prow_d, (size_t)cap * KP * h->L.ldt * sizeof(double)));
    if (h->L.rev) {
        HIP_TRY(malloc0(&h->trow_d, (size_t)cap * h->L.ld * sizeof(double)));
        HIP_TRY(malloc0(&h->uvec_d, (size_t)cap * h->L.ldt * sizeof(double)));
        HIP_TRY(malloc0(&h->xfull_d, (size_t)cap * h->L.N * sizeof(double)));
        HIP_TRY(malloc0(&h->hmail_d, (size_t)cap * 8 * sizeof(int)));
        HIP_TRY(malloc0(&h->rmark_d, (size_t)cap * sizeof(int)));
        HIP_TRY(malloc0(&h->age0_d, (size_t)cap * sizeof(long long)));
    }
    HIP_TRY(malloc0(&h->desc_d, (size_t)cap * KP * sizeof(PivDesc)));
    HIP_TRY(malloc0(&h->pcol_d, (size_t)cap * KP * h->L.Mp1p * sizeof(double)));
    HIP_TRY(malloc0(&h->dcur_d, (size_t)cap * h->L.ld * sizeof(double)));
    HIP_TRY(malloc0(&h->dper_d, (size_t)cap * h->L.ld * sizeof(double)));
    HIP_TRY(malloc0(&h->pflags_d, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->stall_d, cap * sizeof(int)));
    if (!h->xstat_d) HIP_TRY(malloc0(&h->xstat_d, 12 * sizeof(int)));      // (8: the selections'; 3 more: the start of an objective batch under a method)
    if (!h->dbg_d) HIP_TRY(malloc0(&h->dbg_d, 16 * sizeof(unsigned long long)));
    HIP_TRY(malloc0(&h->npend_d, (size_t)2 * cap * sizeof(int)));      // (npend and flushed in one piece: bslv_lpq_park's copy of both is one readback)
    h->flushed_d = h->npend_d + cap;
    HIP_TRY(hipHostMalloc(&h->status_h, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->active_d, cap * sizeof(int)));
    HIP_TRY(hipHostMalloc(&h->active_h, cap * sizeof(int)));
    HIP_TRY(malloc0(&h->init_d, (size_t)cap * 3 * sizeof(int)));
    HIP_TRY(hipHostMalloc(&h->init_h, (size_t)cap * 3 * sizeof(int)));
    h->Bcap = cap;
    return 0;
}

// the work-list lengths (nwork_d, one counter per pass of a call): room for `need` of them, the first `zero` zeroed on the stream
static int ensure_nwork(bslv_lpq *h, int need, int zero)
{
    hipStream_t s = h->stream;
    if (need > h->nworkcap) { if (h->nwork_d) (void)hipFree(h->nwork_d); h->nwork_d = nullptr; HIP_TRY(malloc0s(&h->nwork_d, need * sizeof(int), s)); h->nworkcap = need; }
    HIP_TRY(hipMemsetAsync(h->nwork_d, 0, (size_t)zero * sizeof(int), s));
    return 0;
}
static BatchView bview(bslv_lpq *h)
{
    BatchView v;
    v.src = h->src_d; v.dst = h->dst_d; v.vlo = h->vlo_d; v.vup = h->vup_d;
    v.status = h->status_d; v.iters = h->iters_d; v.mode = h->mode_d; v.verified = h->ver_d;
    v.desc = h->desc_d; v.prow = h->prow_d; v.pcol = h->pcol_d; v.dcur = h->dcur_d; v.npend = h->npend_d; v.flushed = h->flushed_d;
    v.work = h->work_d; v.nwork = h->nwork_d;
    v.dper = h->dper_d; v.pflags = h->pflags_d; v.stall = h->stall_d; v.xstat = h->xstat_d;
    v.trow = h->trow_d; v.uvec = h->uvec_d; v.xfull = h->xfull_d; v.dbg = h->dbg_d; v.hmail = h->hmail_d; v.rmark = h->rmark_d;
    v.lazy = (h->lazy && !h->L.rev) ? 1 : 0;
    return v;
}

static int upload_bounds(bslv_lpq *h, const double *lb, const double *ub)
{
    int M = h->L.M, N = h->L.N;
    std::vector<double> lo(lb, lb + M + N), up(ub, ub + M + N);
    std::vector<unsigned char> art(M + N, 0);
    // artificial bounds: a structural column with non-zero cost and no bound on the side its
    // reduced cost needs would be dual infeasible in the standard basis (oracle: primal phase 1)
    for (int j = 0; j < N; j++) {
        double c = h->cost[j + 1];
        int k = M + j;
        if (c > 0 && std::isinf(lo[k])) { lo[k] = -BIG; art[k] |= 1; }
        if (c < 0 && std::isinf(up[k])) { up[k] = BIG; art[k] |= 2; }
    }
    h->has_boxed = false;
    for (int k = 0; k < M + N; k++) if (!art[k] && std::isfinite(lo[k]) && std::isfinite(up[k]) && lo[k] < up[k]) h->has_boxed = true;
    HIP_TRY(hipMemcpyAsync(h->lb_d, lo.data(), (M + N) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ub_d, up.data(), (M + N) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->art_d, art.data(), (M + N), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" {

const char *bslv_last_error(void) { return g_err; }

int bslv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bslv_set_device(int device)
{
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { set_error("bslv_set_device: device %d of %d", device, n); return BSLV_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    return 0;
}

int bslv_device_info(char *name, int name_len, int *cus, size_t *mem_bytes)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) { strncpy(name, p.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    if (cus) *cus = p.multiProcessorCount;
    if (mem_bytes) *mem_bytes = p.totalGlobalMem;
    return 0;
}

static int raw_create(bslv_lpq **out, int M, int N, const double *A, const double *lb, const double *ub,
                      const double *cost, int var_first, int var_cnt, int pool_slots)
{
    if (!out || M < 1 || N < 1 || !A || !lb || !ub || !cost || pool_slots < 1 || var_cnt < 0 ||
        (var_cnt > 0 && (var_first < 0 || var_first + var_cnt > M + N))) {
        set_error("bslv_lpq_create: bad argument");
        return BSLV_E_ARG;
    }
    if (bslv_device_count() < 1) { set_error("no HIP device available"); return BSLV_E_NODEVICE; }
    bslv_lpq *h = new bslv_lpq();
    LpView &L = h->L;
    L.M = M; L.N = N;
    L.ld = (N + 15) / 16 * 16;
    L.Mp1 = M + 1;
    L.Mp1p = (M + 1 + 15) / 16 * 16;
    L.vfirst = var_first; L.vcnt = var_cnt;
    L.maxit = 50 * (M + N) + 1000;
    L.bland_after = 4 * (M + N) + 200;
    // tableau or revised form?  The revised form pays a sparse product per tableau row / column it looks at and moves M x M instead of
    // (M + 1) x N doubles per pass: for wide (N >= 2 M) and sparse (< 2 % non-zeros) problems.  BSLV_LP_REV=0/1 forces it.
    long nnz = 0;
    for (size_t k = 0; k < (size_t)M * N; k++) nnz += A[k] != 0.0;
    h->nnzA = nnz;
    // (by itself only where tableaux are out of reach -- 4 GiB and more each; ex09's 1.36 GB tableaux still fit 140 times into 288 GB and
    // the tableau form is the faster one for its one-LP-at-a-time phases and needs no refactorisation: DESIGN.md section 5)
    bool rev = N >= 2 * M && nnz * 50 < (long)M * N && (size_t)(M + 1) * (size_t)L.ld * sizeof(double) >= ((size_t)4 << 30);
    if (const char *e = getenv("BSLV_LP_REV")) rev = atoi(e) != 0;
    L.rev = rev ? 1 : 0;
    L.ldt = rev ? (M + 15) / 16 * 16 : L.ld;
    L.mrows = rev ? M : L.Mp1;
    L.slotT = (size_t)L.mrows * L.ldt;
    h->slots = pool_slots;
    h->cost.assign(cost, cost + N + 1);
    h->c0 = cost[0];
    int rc = 0;
    auto fail = [&](int code) { bslv_lpq_destroy(h); return code; };
    // BSLV_LP_CUMASK=<hex word>: the engine's stream may only use the CUs whose bit is set in the word (repeated over all CUs), e.g.
    // 77777777 = three of every four.  For the pipelined driver: the tableau passes saturate HBM from fewer CUs than the chip
    // has, and the small kernels of the cut phase, on their own stream, find free CUs instead of queueing behind them.
    if (const char *cm = getenv("BSLV_LP_CUMASK")) {
        const unsigned word = (unsigned)strtoul(cm, nullptr, 16);
        unsigned mask[16];
        for (int k = 0; k < 16; k++) mask[k] = word;
        if (hipExtStreamCreateWithCUMask(&h->stream, 16, mask) != hipSuccess) { (void)hipGetLastError(); h->stream = nullptr; }
    }
    if (!h->stream && hipStreamCreate(&h->stream) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(BSLV_E_NODEVICE); }
#define TRYF(e) do { hipError_t _e = (e); if (_e != hipSuccess) { set_error("%s failed: %s", #e, hipGetErrorString(_e)); return fail(_e == hipErrorOutOfMemory ? BSLV_E_NOMEM : BSLV_E_NODEVICE); } } while (0)
    TRYF(malloc0(&L.T, (size_t)pool_slots * L.slotT * sizeof(double)));
    TRYF(malloc0(&L.beta, (size_t)pool_slots * L.Mp1p * sizeof(double)));
    TRYF(malloc0(&L.xN, (size_t)pool_slots * L.ld * sizeof(double)));
    TRYF(malloc0(&L.bh, (size_t)pool_slots * M * sizeof(int)));
    TRYF(malloc0(&L.nh, (size_t)pool_slots * N * sizeof(int)));
    TRYF(malloc0(&L.nstat, (size_t)pool_slots * N * sizeof(int)));
    TRYF(malloc0(&L.pos, (size_t)pool_slots * (M + N) * sizeof(int)));
    if (!rev) TRYF(malloc0(&h->Tstd, L.slotT * sizeof(double)));
    else {
        TRYF(malloc0(&h->dsl_d, (size_t)pool_slots * L.ld * sizeof(double)));
        TRYF(malloc0(&h->age_d, (size_t)pool_slots * sizeof(long long)));
        TRYF(hipMemset(h->age_d, 0, (size_t)pool_slots * sizeof(long long)));      // (whatever malloc0 fills with: a slot nobody has built yet has no age)
        TRYF(malloc0(&h->cost_d, (size_t)(N + 1) * sizeof(double)));
        TRYF(malloc0(&h->cptr_d, (size_t)(N + 1) * sizeof(int)));
        TRYF(malloc0(&h->rptr_d, (size_t)(M + 1) * sizeof(int)));
        TRYF(malloc0(&h->cidx_d, (size_t)std::max(nnz, 1L) * sizeof(int)));
        TRYF(malloc0(&h->ridx_d, (size_t)std::max(nnz, 1L) * sizeof(int)));
        TRYF(malloc0(&h->cval_d, (size_t)std::max(nnz, 1L) * sizeof(double)));
        TRYF(malloc0(&h->rval_d, (size_t)std::max(nnz, 1L) * sizeof(double)));
    }
    TRYF(malloc0(&h->lb_d, (M + N) * sizeof(double)));
    TRYF(malloc0(&h->ub_d, (M + N) * sizeof(double)));
    TRYF(malloc0(&h->art_d, (M + N)));
#undef TRYF
    L.lb = h->lb_d; L.ub = h->ub_d; L.art = h->art_d;
    L.dsl = h->dsl_d; L.cptr = h->cptr_d; L.cidx = h->cidx_d; L.cval = h->cval_d; L.rptr = h->rptr_d; L.ridx = h->ridx_d; L.rval = h->rval_d;
    if (rev) {
        std::vector<int> cptr(N + 1, 0), rptr(M + 1, 0), cidx((size_t)nnz), ridx((size_t)nnz);
        std::vector<double> cval((size_t)nnz), rval((size_t)nnz);
        size_t t = 0;
        for (int i = 0; i < M; i++) { rptr[i] = (int)t; for (int j = 0; j < N; j++) { const double a = A[(size_t)i * N + j]; if (a != 0.0) { ridx[t] = j; rval[t] = a; t++; cptr[j + 1]++; } } }
        rptr[M] = (int)t;
        for (int j = 0; j < N; j++) cptr[j + 1] += cptr[j];
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int i = 0; i < M; i++) for (int u = rptr[i]; u < rptr[i + 1]; u++) { const int j = ridx[u]; cidx[fill[j]] = i; cval[fill[j]] = rval[u]; fill[j]++; }
        bool okc = hipMemcpy(h->cptr_d, cptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(h->rptr_d, rptr.data(), (M + 1) * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                   hipMemcpy(h->cost_d, cost, (N + 1) * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (nnz) okc = okc && hipMemcpy(h->cidx_d, cidx.data(), nnz * sizeof(int), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(h->ridx_d, ridx.data(), nnz * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                             hipMemcpy(h->cval_d, cval.data(), nnz * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(h->rval_d, rval.data(), nnz * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (!okc) { set_error("upload of A (CSC / CSR) failed"); return fail(BSLV_E_NODEVICE); }
    } else {
        std::vector<double> img(L.slotT, 0.0);
        for (int i = 0; i < M; i++) memcpy(&img[(size_t)i * L.ld], A + (size_t)i * N, N * sizeof(double));
        for (int j = 0; j < N; j++) img[(size_t)M * L.ld + j] = cost[j + 1];
        if (hipMemcpy(h->Tstd, img.data(), L.slotT * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("upload of A failed");
            return fail(BSLV_E_NODEVICE);
        }
    }
    if ((rc = upload_bounds(h, lb, ub))) return fail(rc);
    if ((rc = ensure_batch(h, 64))) return fail(rc);
    h->force_ext = L.slotT * sizeof(double) >= ((size_t)1 << 30) || (rev && (size_t)(M + 1) * L.ld * sizeof(double) >= ((size_t)1 << 30));     // (large problems are degenerate problems: no stalling at a millisecond per pivot)
    {   // k_flush stages KP pivot rows in LDS: wide problems (N > ~1300) need more than the default 64 KB
        const size_t want = (size_t)KP * h->L.ldt * sizeof(double);
        if (want > h->flush_lds_max) {
            if (want <= 144 * 1024 && hipFuncSetAttribute((const void *)k_flush<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) h->flush_lds_max = want;
            else (void)hipGetLastError();
        }
    }
    // BSLV_LP_METHOD=dual|primal|repair: the method the engine starts with (bslv_lpq_set_method); the revised form has the dual one only
    if (const char *e = getenv("BSLV_LP_METHOD")) {
        if (!rev) h->method = !strcmp(e, "primal") ? BSLV_LP_METHOD_PRIMAL : !strcmp(e, "repair") ? BSLV_LP_METHOD_REPAIR : BSLV_LP_METHOD_DUAL;
    }
    // BSLV_LP_PRICING=dantzig|devex: the rule for the leaving row of a dual step (bslv_lpq_set_pricing), in both forms
    if (const char *e = getenv("BSLV_LP_PRICING")) h->pricing = !strcmp(e, "devex") ? BSLV_LP_PRICING_DEVEX : BSLV_LP_PRICING_DANTZIG;
    // BSLV_LP_PRIMAL_PRICING=dantzig|devex: the rule for the entering column of a primal step (bslv_lpq_set_primal_pricing), in both forms
    if (const char *e = getenv("BSLV_LP_PRIMAL_PRICING")) h->ppricing = !strcmp(e, "devex") ? BSLV_LP_PRICING_DEVEX : BSLV_LP_PRICING_DANTZIG;
    // BSLV_LP_REFACTOR=1: the in-call rescue of bslv_lpq_set_refactor, for an engine in the revised form (the tableau form has no inverse to rebuild)
    L.rfx = 0; L.drift_b = -1; L.drift_p = -1;
    if (const char *e = getenv("BSLV_LP_REFACTOR")) { if (rev) h->refactor_on = atoi(e) != 0; }
    // BSLV_LP_REFACTOR_EVERY=K: the period of bslv_lpq_set_refactor_period, for an engine in the revised form (the tableau form ignores it)
    if (const char *e = getenv("BSLV_LP_REFACTOR_EVERY")) { if (rev) h->period = std::max(0, atoi(e)); }
    // BSLV_LP_PARK=0: bslv_lpq_park makes the passes at once, as bslv_lpq_materialise does (bslv_lpq_set_park)
    if (const char *e = getenv("BSLV_LP_PARK")) h->park.on = atoi(e) != 0;
    // BSLV_LP_RAYS=1: the ray store of bslv_lpq_set_rays, in both forms
    if (const char *e = getenv("BSLV_LP_RAYS")) if (atoi(e) != 0 && (rc = bslv_lpq_set_rays(h, 1))) return fail(rc);
    *out = h;
    return 0;
}

void bslv_lpq_destroy(bslv_lpq *h)
{
    if (!h) return;
    park_free(h);
    period_free(h);
    auto fr = [](void *p) { if (p) (void)hipFree(p); };
    fr(h->raykind_d); fr(h->raystat_d); fr(h->ray_d); fr(h->lb_nst_d); fr(h->lb_xv_d);
    fr(h->age_d); fr(h->age0_d); fr(h->cert_d);
    for (const DevexNorms *r : {&h->dvx, &h->pdv}) { fr(r->norm_d); fr(r->stat_d); }
    for (const TiePhase *r : {&h->tie, &h->tie_obj, &h->tie_call, &h->tie_call_obj}) { fr(r->dir_d); fr(r->g_d); fr(r->state_d); fr(r->iters_d); fr(r->stat_d); }
    fr(h->L.T); fr(h->L.beta); fr(h->L.xN); fr(h->L.bh); fr(h->L.nh); fr(h->L.nstat); fr(h->L.pos);
    fr(h->Tstd); fr(h->lb_d); fr(h->ub_d); fr(h->art_d);
    fr(h->dbg_d); fr(h->list_d); fr(h->cptr_d); fr(h->cidx_d); fr(h->rptr_d); fr(h->ridx_d); fr(h->cval_d); fr(h->rval_d); fr(h->cost_d); fr(h->dsl_d); fr(h->trow_d); fr(h->uvec_d); fr(h->xfull_d); fr(h->hmail_d);
    fr(h->src_d); fr(h->dst_d); fr(h->status_d); fr(h->iters_d); fr(h->mode_d); fr(h->ver_d); fr(h->qslot_d); fr(h->init_d);
    fr(h->rmark_d); fr(h->rfx_i_d); fr(h->rfx_c_d);
    fr(h->vlo_d); fr(h->vup_d); fr(h->prow_d); fr(h->desc_d); fr(h->out_d); fr(h->active_d); fr(h->work_d); fr(h->nwork_d); fr(h->npend_d); fr(h->pcol_d); fr(h->dcur_d); fr(h->dper_d); fr(h->pflags_d); fr(h->stall_d); fr(h->xstat_d); fr(h->cvals_d); fr(h->clb_d); fr(h->cub_d); fr(h->cart_d);
    if (h->status_h) (void)hipHostFree(h->status_h);
    if (h->active_h) (void)hipHostFree(h->active_h);
    if (h->init_h) (void)hipHostFree(h->init_h);
    for (auto &e : h->evpool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int bslv_lpq_pool_slots(const bslv_lpq *h) { return h ? h->slots : 0; }
size_t bslv_lpq_slot_bytes(const bslv_lpq *h)
{
    if (!h) return 0;
    const LpView &L = h->L;
    return (L.slotT + L.Mp1p + L.ld + (L.rev ? L.ld : 0)) * sizeof(double) + (size_t)(2 * (L.M + L.N) + L.N) * sizeof(int);
}

// bounds of the engine's model from the bounds of the model as given: the folded rows tighten their columns
static void fold_bounds(bslv_lpq *h, const double *lb, const double *ub, std::vector<double> &lo, std::vector<double> &up)
{
    bslv_lpq::Presolve &P = h->ps;
    const int M0 = P.M0, N0 = P.N0, Mi = M0 - P.nfold;
    P.lb0.assign(lb, lb + M0 + N0); P.ub0.assign(ub, ub + M0 + N0);
    lo.assign((size_t)Mi + N0, 0.0); up.assign((size_t)Mi + N0, 0.0);
    P.clo.assign(lb + M0, lb + M0 + N0); P.cup.assign(ub + M0, ub + M0 + N0);
    P.lo_src.assign(N0, -1); P.up_src.assign(N0, -1);
    for (int i = 0; i < M0; i++) {
        if (P.row_in[i] >= 0) { lo[P.row_in[i]] = lb[i]; up[P.row_in[i]] = ub[i]; continue; }
        const int j = P.fold_col[i];
        const double a = P.fold_a[i];
        const double l = a > 0 ? lb[i] / a : ub[i] / a, u = a > 0 ? ub[i] / a : lb[i] / a;
        if (l > P.clo[j]) { P.clo[j] = l; P.lo_src[j] = i; }
        if (u < P.cup[j]) { P.cup[j] = u; P.up_src[j] = i; }
    }
    // new bounds may leave a folded row no room (the fold set is fixed at create time): the model as given is infeasible -- reported as
    // such by solve_batch; the engine itself gets a consistent (degenerate) box
    P.empty_box = false;
    for (int j = 0; j < N0; j++) {
        if (P.clo[j] > P.cup[j] + TOL_BND * (1.0 + fabs(P.cup[j]))) { P.empty_box = true; P.cup[j] = P.clo[j]; }
        lo[Mi + j] = P.clo[j]; up[Mi + j] = P.cup[j];
    }
}
int bslv_lpq_set_bounds(bslv_lpq *h, const double *lb, const double *ub)
{
    if (!h || !lb || !ub) { set_error("bslv_lpq_set_bounds: bad argument"); return BSLV_E_ARG; }
    if (h->ps.nfold == 0) { h->ps.lb0.assign(lb, lb + h->ps.M0 + h->ps.N0); h->ps.ub0.assign(ub, ub + h->ps.M0 + h->ps.N0); return upload_bounds(h, lb, ub); }
    std::vector<double> lo, up;
    fold_bounds(h, lb, ub, lo, up);
    return upload_bounds(h, lo.data(), up.data());
}
int bslv_lpq_rows_folded(const bslv_lpq *h) { return h ? h->ps.nfold : 0; }
int bslv_lpq_is_revised(const bslv_lpq *h) { return h ? h->L.rev : 0; }

int bslv_lpq_create(bslv_lpq **out, int M, int N, const double *A, const double *lb, const double *ub,
                    const double *cost, int var_first, int var_cnt, int pool_slots)
{
    if (!out || M < 1 || N < 1 || !A || !lb || !ub || !cost || pool_slots < 1 || var_cnt < 0 ||
        (var_cnt > 0 && (var_first < 0 || var_first + var_cnt > M + N))) {
        set_error("bslv_lpq_create: bad argument");
        return BSLV_E_ARG;
    }
    bslv_lpq::Presolve P;
    P.M0 = M; P.N0 = N;
    P.row_in.assign(M, 0); P.fold_col.assign(M, -1); P.fold_a.assign(M, 0.0);
    std::vector<double> clo(lb + M, lb + M + N), cup(ub + M, ub + M + N);
    const bool off = getenv("BSLV_NO_PRESOLVE") != nullptr;
    int kept = 0;
    for (int i = 0; i < M; i++) {
        bool fold = false;
        const bool per_lp = var_cnt > 0 && i >= var_first && i < var_first + var_cnt;
        if (!off && !per_lp && M - P.nfold > 1) {
            int nz = 0, jj = -1;
            const double *row = A + (size_t)i * N;
            for (int j = 0; j < N && nz < 2; j++) if (row[j] != 0.0) { nz++; jj = j; }
            // (a column whose bounds are given per LP keeps its rows: solve_batch would overwrite the folded bound)
            const bool col_per_lp = nz == 1 && var_cnt > 0 && M + jj >= var_first && M + jj < var_first + var_cnt;
            if (nz == 1 && !col_per_lp) {
                const double a = row[jj];
                const double l = std::max(clo[jj], a > 0 ? lb[i] / a : ub[i] / a), u = std::min(cup[jj], a > 0 ? ub[i] / a : lb[i] / a);
                if (l <= u) { fold = true; clo[jj] = l; cup[jj] = u; P.fold_col[i] = jj; P.fold_a[i] = a; }      // (an empty box stays a row: the LP reports it)
            }
        }
        if (fold) { P.row_in[i] = -1; P.nfold++; } else P.row_in[i] = kept++;
    }
    if (P.nfold == 0) {
        const int rc = raw_create(out, M, N, A, lb, ub, cost, var_first, var_cnt, pool_slots);
        if (rc) return rc;
        (*out)->ps = P;
        (*out)->ps.lb0.assign(lb, lb + M + N); (*out)->ps.ub0.assign(ub, ub + M + N);
        return 0;
    }
    const int Mi = M - P.nfold;
    std::vector<double> Ai((size_t)Mi * N);
    for (int i = 0; i < M; i++) if (P.row_in[i] >= 0) memcpy(&Ai[(size_t)P.row_in[i] * N], A + (size_t)i * N, (size_t)N * sizeof(double));
    // the per-LP range keeps its place among the rows that stay (no row inside it is folded); a range over columns moves with them
    int vf = var_first;
    if (var_cnt > 0) vf = var_first < M ? P.row_in[var_first] : Mi + (var_first - M);
    std::vector<double> lo0((size_t)Mi + N, 0.0), up0((size_t)Mi + N, 0.0);
    for (int i = 0; i < M; i++) if (P.row_in[i] >= 0) { lo0[P.row_in[i]] = lb[i]; up0[P.row_in[i]] = ub[i]; }
    for (int j = 0; j < N; j++) { lo0[Mi + j] = clo[j]; up0[Mi + j] = cup[j]; }
    const int rc = raw_create(out, Mi, N, Ai.data(), lo0.data(), up0.data(), cost, vf, var_cnt, pool_slots);
    if (rc) return rc;
    (*out)->ps = P;
    std::vector<double> lo, up;
    fold_bounds(*out, lb, ub, lo, up);                    // (fills lo_src / up_src and the record of the bounds as given)
    return 0;
}

int bslv_lpq_set_profile(bslv_lpq *h, int on)
{
    if (!h) return BSLV_E_ARG;
    h->profile = on != 0;
    return 0;
}

int bslv_lpq_reset_slot(bslv_lpq *h, int slot)
{
    if (!h || slot < 0 || slot >= h->slots) { set_error("bslv_lpq_reset_slot: bad slot %d", slot); return BSLV_E_ARG; }
    if (h->lazy_open) { const int rc = materialise_indices(h, nullptr, 0); if (rc) return rc; h->lazy_open = false; }      // (a pending pass must not land on the slot after it has been reset)
    { const int rc = park_before(h, 0, nullptr, 1, &slot); if (rc) return rc; }      // (nor may a parked pass read it afterwards)
    LpView &L = h->L;
    if (L.rev) {
        const size_t nk = std::max((size_t)L.M * L.ldt, (size_t)L.ld);
        hipLaunchKernelGGL(k_rev_identity, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, L, slot, (const double *)h->cost_d);
    } else HIP_TRY(hipMemcpyAsync(L.T + (size_t)slot * L.slotT, h->Tstd, L.slotT * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    int n = std::max(std::max(L.M, L.N), std::max(L.ld, L.Mp1p));
    hipLaunchKernelGGL(k_std_heads, dim3((n + 255) / 256), dim3(256), 0, h->stream, L, slot);
    HIP_TRY(hipGetLastError());
    if (L.rev) HIP_TRY(hipMemsetAsync(h->age_d + slot, 0, sizeof(long long), h->stream));      // (the identity: no step applied)
    if (h->rays_on) HIP_TRY(hipMemsetAsync(h->raykind_d + slot, 0, sizeof(int), h->stream));     // (BSLV_LP_RAY_NONE)
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- lazy tableaux -----------------------------------------------------------------------------------------------------------
// The first pass of a solve streams the parent's tableau into the LP's own slot (k_flush): 8 MB written per LP on S-mid, 17 GB per
// batch of 2048 -- the largest single item of the LP phase -- and for nothing where nobody reads the slot again: only the LP of a
// vertex that yields a NEW cut becomes the parent of later LPs (28 % of a batch on S-mid; the rest confirm their vertex or return a
// cut a sibling delivered).  Values, duals and the objective of a finished LP are all in its vectors.  With bslv_lpq_set_lazy(h, 1)
// an LP that is finished when its pass would be due keeps its pending pivots (<= KP; one that needs more passes as before), and the
// caller names the slots it will use as parents: bslv_lpq_materialise(h, n, slots) gives those their tableau -- the same pass, the
// same arithmetic -- and bslv_lpq_discard_pending(h) drops the rest.  A batch that is started while slots are still open gives all
// of them their tableau first (the retry batches of the driver).  Slots that were neither materialised nor parked (below) must not be used as `src`.
typedef std::pair<hipEvent_t, hipEvent_t> EventPair;
static int event_pair(EventPair *ev)
{
    HIP_TRY(hipEventCreate(&ev->first)); HIP_TRY(hipEventCreate(&ev->second));
    return 0;
}
// One pass over the work list of counter slot cnt_slot of a view (at most `upper` LPs): every pass of the engine is launched here.
// ev: the caller's events, recorded around the pass (set_profile), or nullptr.  refresh: the work list again where the pass belongs to
// a round of a solve of the revised form -- k_rev_u for the LPs of the list that asked for a refresh of beta, inside the events (its
// batch-size argument is read only without a list: `upper` stands in).  The geometry below is worked out per pass, a few host
// instructions and one getenv beside four launches, so that BSLV_FLUSH_NT and the LDS limit act wherever a pass is made.
static int flush_launch(bslv_lpq *h, const BatchView &bv, int cnt_slot, int upper, const EventPair *ev, const int *refresh = nullptr)
{
    LpView &L = h->L;
    hipStream_t s = h->stream;
    const int wide = (size_t)KP * L.ldt * sizeof(double) > h->flush_lds_max;      // pivot rows from global memory in k_flush
    const size_t lds = wide ? 0 : (size_t)KP * L.ldt * sizeof(double);
    // (160 KB of LDS per CU: three workgroups of NT threads need lds <= ~53 KB)
    const char *e = getenv("BSLV_FLUSH_NT");
    const bool big_flush = e ? atoi(e) > NT : lds > 53 * 1024;
    const int tiles = (L.mrows + TR - 1) / TR;
    // few LPs left: smaller row tiles keep >= ~2k workgroups in flight
    int tr = upper * tiles >= 2048 ? 32 : (upper * tiles * 2 >= 2048 ? 16 : (upper * tiles * 4 >= 2048 ? 8 : 4));      // (4: one row per wave -- a single LP of a few thousand rows)
    if (big_flush) {                                            // 16 waves per workgroup: at least one row per wave, more where the batch still fills the chip
        const long rows = (long)upper * L.mrows;
        tr = rows >= 2048L * 128 ? 128 : rows >= 2048L * 64 ? 64 : rows >= 2048L * 32 ? 32 : 16;
    }
    const int ntile = (L.mrows + tr - 1) / tr, fnt = big_flush ? NT_BIG : NT;
    if (ev) HIP_TRY(hipEventRecord(ev->first, s));
    if (refresh) hipLaunchKernelGGL(k_rev_u, dim3(upper), dim3(NT), 0, s, L, bv, upper, refresh, cnt_slot);
    if (wide) hipLaunchKernelGGL(k_flush<true>, dim3(std::min(upper * ntile, h->upd_grid)), dim3(fnt), 0, s, L, bv, cnt_slot, ntile, tr);
    else hipLaunchKernelGGL(k_flush<false>, dim3(std::min(upper * ntile, h->upd_grid)), dim3(fnt), lds, s, L, bv, cnt_slot, ntile, tr);
    if (ev) HIP_TRY(hipEventRecord(ev->second, s));
    hipLaunchKernelGGL(k_after_flush, dim3((upper + 255) / 256), dim3(256), 0, s, bv, cnt_slot);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int flush_list(bslv_lpq *h, int cnt_slot, int upper, bool account = true)      // (account: the pass counts in the statistics of the lazy tableaux and of the last batch)
{
    hipStream_t s = h->stream;
    EventPair ev{nullptr, nullptr};
    int rc;
    if (h->profile && (rc = event_pair(&ev))) return rc;
    if ((rc = flush_launch(h, bview(h), cnt_slot, upper, h->profile ? &ev : nullptr))) return rc;
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, h->nwork_d + cnt_slot, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (account) { h->last.passes += n; h->last.launches += 1; h->lazy_materialised += n; }
    if (h->profile) { float t = 0; (void)hipEventElapsedTime(&t, ev.first, ev.second); h->last.update_ms += t; (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    return 0;
}
// batch indices list[0..n) of the last batch (nullptr: all of it): their slots get their tableau
static int materialise_indices(bslv_lpq *h, const int *list, int n)
{
    if (!h->lazy_open || (list && n == 0)) return 0;
    hipStream_t s = h->stream;
    BatchView bv = bview(h);
    const int B = (int)h->last_dst.size();
    std::vector<int> all;
    if (!list) { all.resize(B); for (int b = 0; b < B; b++) all[b] = b; list = all.data(); n = B; }
    if (n > h->listcap) { if (h->list_d) (void)hipFree(h->list_d); h->list_d = nullptr; HIP_TRY(malloc0s(&h->list_d, (size_t)std::max(n, 1024) * sizeof(int), s)); h->listcap = std::max(n, 1024); }
    const int cnt_slot = h->L.maxit + 42;
    HIP_TRY(hipMemcpyAsync(h->list_d, list, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(h->nwork_d + cnt_slot, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_list_given, dim3((n + 255) / 256), dim3(256), 0, s, bv, (const int *)h->list_d, n, cnt_slot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));              // (`all` / the caller's list may go out of scope)
    int rc = flush_list(h, cnt_slot, n);
    if (rc) return rc;
    // row M again: the pass has applied the pending pivots to the row it found -- for an LP that had passed once before and finished
    // with pivots pending that was ALREADY the final row (k_store_d at the end of the solve), now updated twice; the vector is the truth
    hipLaunchKernelGGL(k_store_d, dim3((h->L.ld + 255) / 256, B), dim3(256), 0, s, h->L, bv, B);
    HIP_TRY(hipGetLastError());
    // (a slot of this batch that was parked has its tableau now: its record must not make the pass a second time)
    if (h->park.cap) for (int k = 0; k < n; k++) { const int r = h->park.rec_of_slot[h->last_dst[list[k]]]; if (r >= 0) { park_release(h, r); h->park.stats[3]++; } }
    return 0;
}
// ---- parked passes -----------------------------------------------------------------------------------------------------------
// bslv_lpq_materialise gives every slot the driver keeps its tableau at once, because any of them MAY become a parent; most never do
// (a batch takes the children of a few of them, the pool evicts the others first).  bslv_lpq_park(h, n, slots) postpones the pass
// instead: what it needs -- npend, flushed, src, dst, the descriptors, pivot rows and multiplier columns of the pending pivots, the
// reduced-cost row -- is copied to a record of a store beside the pool (k_park_copy, ~2 % of the pool's bytes), shaped like the batch
// arrays, so that k_flush and k_after_flush run on a BatchView that points into the store.  The pass is made (unparked: park_pass,
// the same arithmetic on the same inputs) when a batch names the slot as `src`, and, for a record that has not passed before and so
// still reads its parent's slot, before that slot is overwritten; a record whose own slot is overwritten or that the caller gives
// up (bslv_lpq_drop_parked) is dropped without a pass.  The host knows what is parked (rec_of_slot and, per record, slot, source and
// flushed): no readback, no host wait.  Tableau form only; the revised form and an engine whose store does not fit materialise.
static void park_free(bslv_lpq *h)
{
    bslv_lpq::Park &P = h->park;
    auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    fr(P.src); fr(P.dst); fr(P.npend); fr(P.flushed); fr(P.mode); fr(P.ver); fr(P.work); fr(P.nwork); fr(P.desc); fr(P.prow); fr(P.pcol); fr(P.dcur); fr(P.pairs_d); fr(P.list_d);
    if (P.pairs_h) (void)hipHostFree(P.pairs_h);
    if (P.list_h) (void)hipHostFree(P.list_h);
    P.pairs_h = P.list_h = nullptr;
    for (auto &e : P.pre_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    P.pre_ev.clear();
    P.cap = 0;
}
static bool park_alloc(bslv_lpq *h)
{
    bslv_lpq::Park &P = h->park;
    if (P.cap) return true;
    if (P.failed) return false;
    const LpView &L = h->L;
    const size_t n = (size_t)h->slots;
    hipStream_t s = h->stream;
    const bool ok = malloc0s(&P.src, n * sizeof(int), s) == hipSuccess && malloc0s(&P.dst, n * sizeof(int), s) == hipSuccess && malloc0s(&P.npend, n * sizeof(int), s) == hipSuccess &&
                    malloc0s(&P.flushed, n * sizeof(int), s) == hipSuccess && malloc0s(&P.mode, n * sizeof(int), s) == hipSuccess && malloc0s(&P.ver, n * sizeof(int), s) == hipSuccess &&
                    malloc0s(&P.work, n * sizeof(int), s) == hipSuccess && malloc0s(&P.nwork, sizeof(int), s) == hipSuccess && malloc0s(&P.pairs_d, 2 * n * sizeof(int), s) == hipSuccess &&
                    malloc0s(&P.list_d, n * sizeof(int), s) == hipSuccess && malloc0s(&P.desc, n * KP * sizeof(PivDesc), s) == hipSuccess && malloc0s(&P.dcur, n * L.ld * sizeof(double), s) == hipSuccess &&
                    malloc0s(&P.prow, n * KP * L.ldt * sizeof(double), s) == hipSuccess && malloc0s(&P.pcol, n * KP * L.Mp1p * sizeof(double), s) == hipSuccess &&
                    hipHostMalloc(&P.pairs_h, 2 * n * sizeof(int)) == hipSuccess && hipHostMalloc(&P.list_h, n * sizeof(int)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); park_free(h); P.failed = true; return false; }      // (park() materialises from now on)
    P.cap = (int)n;
    P.free_recs.resize(n); for (size_t k = 0; k < n; k++) P.free_recs[k] = (int)(n - 1 - k);
    P.live.clear(); P.pos_in_live.assign(n, -1); P.rec_of_slot.assign(n, -1);
    P.slot_of.assign(n, -1); P.src_of.assign(n, -1); P.flushed_of.assign(n, 0);
    P.mark.assign(n, 0); P.listed.assign(n, 0);
    return true;
}
static void park_release(bslv_lpq *h, int rec)
{
    bslv_lpq::Park &P = h->park;
    const int at = P.pos_in_live[rec], last = P.live.back();
    P.live[at] = last; P.pos_in_live[last] = at; P.live.pop_back(); P.pos_in_live[rec] = -1;
    P.rec_of_slot[P.slot_of[rec]] = -1; P.slot_of[rec] = -1;
    P.free_recs.push_back(rec);
}
static BatchView park_view(bslv_lpq *h)
{
    const bslv_lpq::Park &P = h->park;
    BatchView v = bview(h);
    v.src = P.src; v.dst = P.dst; v.npend = P.npend; v.flushed = P.flushed; v.mode = P.mode; v.verified = P.ver; v.work = P.work; v.nwork = P.nwork;
    v.desc = P.desc; v.prow = P.prow; v.pcol = P.pcol; v.dcur = P.dcur;
    return v;
}
// The pass of the records recs[0..n) (distinct, live), then they are free: one k_flush launch, row M again from the record's reduced
// costs (as materialise_indices does).  No host wait: the pass counts in the statistics of the batch that follows (pre_*).
static int park_pass(bslv_lpq *h, const int *recs, int n)
{
    if (n == 0) return 0;
    bslv_lpq::Park &P = h->park;
    hipStream_t s = h->stream;
    const BatchView pv = park_view(h);
    if (P.list_inflight) HIP_TRY(hipStreamSynchronize(s));      // (the pinned list of the last pass may not have been read yet: only where two passes follow each other without a batch between them)
    P.list_inflight = true;
    memcpy(P.list_h, recs, (size_t)n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(P.list_d, P.list_h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(P.nwork, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_list_given, dim3((n + 255) / 256), dim3(256), 0, s, pv, (const int *)P.list_d, n, 0);
    EventPair ev{nullptr, nullptr};
    int rc;
    if (h->profile && (rc = event_pair(&ev))) return rc;
    if ((rc = flush_launch(h, pv, 0, n, h->profile ? &ev : nullptr))) return rc;
    if (h->profile) P.pre_ev.push_back(ev);
    hipLaunchKernelGGL(k_store_d_list, dim3((h->L.ld + 255) / 256, n), dim3(256), 0, s, h->L, pv, (const int *)P.list_d, n);
    HIP_TRY(hipGetLastError());
    P.pre_passes += n; P.pre_launches += 1; h->lazy_materialised += n;      // (every record needs its pass: that is why it was parked)
    for (int k = 0; k < n; k++) park_release(h, recs[k]);
    return 0;
}
// Before the slots over[0..nover) are overwritten and the slots use[0..nuse) are read as parents: the records of `use` make their
// pass, so do the records that have not passed before and read one of `over`; then the records of `over` themselves are dropped.
static int park_before(bslv_lpq *h, int nuse, const int *use, int nover, const int *over)
{
    bslv_lpq::Park &P = h->park;
    if (!P.cap || P.live.empty()) return 0;
    std::vector<int> recs;
    for (int k = 0; k < nuse; k++) { const int r = P.rec_of_slot[use[k]]; if (r >= 0 && !P.listed[r]) { P.listed[r] = 1; recs.push_back(r); } }
    const size_t for_child = recs.size();
    for (int k = 0; k < nover; k++) P.mark[over[k]] = 1;
    for (int r : P.live) if (!P.listed[r] && !P.flushed_of[r] && P.mark[P.src_of[r]] && !P.mark[P.slot_of[r]]) { P.listed[r] = 1; recs.push_back(r); }
    for (int k = 0; k < nover; k++) P.mark[over[k]] = 0;
    for (int r : recs) P.listed[r] = 0;
    P.stats[1] += (long)for_child; P.stats[2] += (long)(recs.size() - for_child);
    const int rc = park_pass(h, recs.data(), (int)recs.size());
    if (rc) return rc;
    for (int k = 0; k < nover; k++) { const int r = P.rec_of_slot[over[k]]; if (r >= 0) { park_release(h, r); P.stats[3]++; } }
    return 0;
}
// Which kernel starts the LPs of a batch (beta = T_parent x_N, row M): k_init_grouped where it has an instance -- rows of at most
// 16 x 64 double2 (2048 columns: S-degenerate's 2011 are in, ex09's revised form with ldt ~ 4 600 is not), the reduced-cost row
// not rebuilt per child (objmode: k_prep wrote it into the child's own slot) -- and BSLV_INIT_GROUP is not 0; k_init otherwise.
// Same results bit for bit (tests/test_lp_init_group_gpu.py).  For k_init_grouped the batch is ordered by parent here (stable) and
// every family cut into chunks of children, short enough that the chunks x row tiles fill the chip when the parents are few.
struct InitPlan {
    int epl, rows;          // k_init_grouped<epl, rows>: double2 entries of a row per lane, rows per wave; epl 0: k_init
    int tiles, chunks;      // its grid
};
static void plan_init(bslv_lpq *h, int B, const int *src, InitPlan *plan)
{
    const LpView &L = h->L;
    int *order = h->init_h;
    InitChunk *chunks = reinterpret_cast<InitChunk *>(h->init_h + B);
    // counting sort by parent slot, the families in the order of their first LP: O(B), and it runs while k_prep does
    std::vector<int> &at = h->init_at, &seen = h->init_seen;
    at.resize(h->slots, 0); seen.clear();
    for (int b = 0; b < B; b++) if (at[src[b]]++ == 0) seen.push_back(src[b]);
    { int off = 0; for (int p : seen) { const int n = at[p]; at[p] = off; off += n; } }
    for (int b = 0; b < B; b++) order[at[src[b]]++] = b;
    for (int p : seen) at[p] = 0;
    const int ld2 = L.ldt >> 1;
    const bool on = !(getenv("BSLV_INIT_GROUP") && atoi(getenv("BSLV_INIT_GROUP")) == 0);
    plan->epl = (!on || L.objmode || ld2 > 16 * WAVE) ? 0 : ld2 <= WAVE ? 1 : ld2 <= 2 * WAVE ? 2 : ld2 <= 4 * WAVE ? 4 : ld2 <= 8 * WAVE ? 8 : 16;
    plan->rows = plan->epl == 16 ? 2 : plan->epl == 8 ? 4 : 8;       // (32 double2 of the parent per lane)
    plan->tiles = (L.mrows + plan->rows * (NT / WAVE) - 1) / (plan->rows * (NT / WAVE));
    const int per_chunk = std::max(4, std::min(32, (int)((long)B * plan->tiles / 4096)));      // (S-mid: 2048 LPs x 32 tiles: 16 children)
    int parents = 0, family = 0, n = 0;
    for (int a = 0; a < B;) {
        int e = a;
        while (e < B && src[order[e]] == src[order[a]]) e++;
        parents++; family = std::max(family, e - a);
        for (int c = a; c < e; c += per_chunk) chunks[n++] = InitChunk{c, std::min(per_chunk, e - c)};
        a = e;
    }
    plan->chunks = n;
    h->last_init_parents = parents; h->last_init_family = family; h->last_init_chunks = plan->epl ? n : 0;
}
// How the selections of a batch are launched: plan_select decides once per solve_batch (every environment switch is read at every
// solve: the tests change them between solves of one process), launch_select launches once per round
struct SelectPlan {
    const void *fn;         // the kernel of the batch (select_kernel), unless cpt names k_select_cached
    bool helper_dim;        // its grid has the dimension of the revised form's helper workgroups (every shape but P1, the tableau form's alone)
    const DevexNorms *norms; // it takes the NormView of this record after the BatchView; nullptr: a kernel of the default rule
    int cap2;               // the candidate arrays of an extended selection in LDS (0: a plain selection, or rows too long for the in-LDS sort: no long-step part)
    int nt, per_launch; size_t lds;     // threads per workgroup; selections per launch; dynamic LDS of a k_select launch
    int cpt;                // columns per thread of k_select_cached (plain dual selection of the default rule, tableau form, NT threads), 0: fn
};
// The selection kernels by rule (0: the default one, RULE_DVX, RULE_PDV) and shape; bslv_lpq::select_lds_max has the same indices
// k_select<false>; the extended selection k_select<true>; ... with phase 1 in its primal steps, the PRIMAL and REPAIR methods: k_select_p1
// in the tableau form, k_select_p1_rev in the revised form (k_select_priced_p1_rev<RULE> under the rule of a call: plan_select gives such a
// batch no other rule than the one bslv_lpq_solve_batch_method_priced came with)
// (SHAPE_TIE_REV, SHAPE_TIE_OBJ_REV: k_select_tie_rev and k_select_tie_obj_rev, the tie phases of the revised form -- no selections
// of a plan, listed here for their LDS limits)
enum { SHAPE_PLAIN, SHAPE_EXT, SHAPE_P1, SHAPE_P1_REV, SHAPE_TIE_REV, SHAPE_TIE_OBJ_REV };
static const void *select_kernel(int rule, int shape)
{
    static const void *const k[3][6] = {
        {(const void *)k_select<false>, (const void *)k_select<true>, (const void *)k_select_p1, (const void *)k_select_p1_rev, (const void *)k_select_tie_rev, (const void *)k_select_tie_obj_rev},
        {(const void *)k_select_priced<RULE_DVX, false, false>, (const void *)k_select_priced<RULE_DVX, false, true>, (const void *)k_select_priced<RULE_DVX, true, true>, (const void *)k_select_priced_p1_rev<RULE_DVX>, nullptr, nullptr},
        {nullptr, (const void *)k_select_priced<RULE_PDV, false, true>, (const void *)k_select_priced<RULE_PDV, true, true>, (const void *)k_select_priced_p1_rev<RULE_PDV>, nullptr, nullptr}};      // (primal steps live in the extended selection: without one the batch is refused, plan_select)
    return k[rule][shape];
}
// the kernel of (rule, shape) may be launched with `want` bytes of dynamic LDS, its limit raised if need be
static bool select_lds_fits(bslv_lpq *h, int rule, int shape, size_t want)
{
    size_t &lim = h->select_lds_max[rule][shape];
    if (want <= lim) return true;
    if (want <= 144 * 1024 && hipFuncSetAttribute(select_kernel(rule, shape), hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess) { lim = want; return true; }
    (void)hipGetLastError();
    return false;
}
// Which batches run under primal Devex pricing: objective batches whenever the primal rule is DEVEX (their steps are primal ones and the
// dual rule does not reach them); PRIMAL / REPAIR batches (k_select_p1: tableau form) when the dual rule is DANTZIG -- with both rules on
// they keep the dual-Devex instance, no instance carries both; DUAL-method batches never (their clean-up steps stay as they are)
static bool pdv_batch(const bslv_lpq *h)
{
    const LpView &L = h->L;
    if (h->ppricing != BSLV_LP_PRICING_DEVEX) return false;
    // (an objective batch under a method, bslv_lpq_solve_batch_obj_method: PRIMAL is the objective batch it always was; DUAL makes dual
    //  steps, its clean-up steps stay as they are; REPAIR is a PRIMAL / REPAIR batch: the primal rule unless the dual one is on)
    if (L.objmode) return h->call_obj_method == BSLV_LP_METHOD_PRIMAL || (h->call_obj_method == BSLV_LP_METHOD_REPAIR && h->pricing != BSLV_LP_PRICING_DEVEX);
    return h->call_method != BSLV_LP_METHOD_DUAL && (!L.rev || h->call_priced) && h->pricing != BSLV_LP_PRICING_DEVEX;
}
// A PRIMAL / REPAIR batch of the revised form (bslv_lpq_solve_batch_method): k_select_p1_rev, the instance of the default rule, whatever
// the ENGINE's two pricing switches say, and both counter triples read 0.  The Devex instances of the revised form's phase 1
// (k_select_priced_p1_rev) are reached per call only: under bslv_lpq_solve_batch_method_priced `pricing` and `ppricing` hold the rules
// of the call (call_priced), and the mapping is the tableau form's.
static bool rev_p1_batch(const bslv_lpq *h) { return h->L.rev && !h->L.objmode && h->call_method != BSLV_LP_METHOD_DUAL; }
// ... and the batches under dual Devex pricing (objective batches make primal steps only: they keep the kernels they had -- unless the
// call gave them the method DUAL or REPAIR, bslv_lpq_solve_batch_obj_method: then their steps are a DUAL solve_batch's)
static bool dvx_batch(const bslv_lpq *h) { return h->pricing == BSLV_LP_PRICING_DEVEX && (!h->L.objmode || h->call_obj_method != BSLV_LP_METHOD_PRIMAL) && (!rev_p1_batch(h) || h->call_priced); }
static int plan_select(bslv_lpq *h, int B, const double *vlo, const double *vup, SelectPlan *plan)
{
    LpView &L = h->L;
    // bound flipping ratio test only where a variable has two finite, non-artificial bounds
    const bool p1 = h->call_method != BSLV_LP_METHOD_DUAL && !L.objmode;      // (objective batches keep their own start)
    bool bfrt = h->has_boxed || L.objmode || h->force_ext || p1;        // (the primal steps live in the extended selection)
    if (!bfrt && L.vcnt > 0)
        for (size_t k = 0; k < (size_t)B * L.vcnt && !bfrt; k++) bfrt = std::isfinite(vlo[k]) && std::isfinite(vup[k]) && vlo[k] < vup[k];
    if (getenv("BSLV_LP_EXT")) bfrt = p1 || atoi(getenv("BSLV_LP_EXT")) != 0;      // test hook: force the extended selection on / off
    const bool dvx = dvx_batch(h);
    const bool pdv = pdv_batch(h);
    const int rule = pdv ? RULE_PDV : dvx ? RULE_DVX : 0;
    int cap2 = 2;
    while (cap2 < L.N) cap2 <<= 1;
    size_t sel_lds = (size_t)cap2 * (sizeof(double) + sizeof(int)) + (size_t)L.N;
    if (bfrt && sel_lds > 144 * 1024) { cap2 = 0; sel_lds = (size_t)L.N; }     // rows too long for the in-LDS sort: extended selection without the long-step part
    const int shape_p1 = L.rev ? SHAPE_P1_REV : SHAPE_P1;
    if (bfrt && !select_lds_fits(h, rule, p1 ? shape_p1 : SHAPE_EXT, sel_lds)) bfrt = false;
    if (p1 && !bfrt) { set_error("bslv_lpq_solve_batch: rows too long for the extended selection the primal method needs (N=%d)", L.N); return BSLV_E_CAPACITY; }
    if (L.objmode && !bfrt) { set_error("bslv_lpq_solve_batch_obj: rows too long for the extended selection (N=%d)", L.N); return BSLV_E_CAPACITY; }
    const int shape = p1 ? shape_p1 : bfrt ? SHAPE_EXT : SHAPE_PLAIN;      // (settled: the kernel whose limit is raised below is the kernel launched)
    // revised form: rho (a row of B^-1) in LDS behind the selection's own arrays, when there is room
    plan->lds = bfrt ? sel_lds : 0;
    L.rho_off = -1;
    if (L.rev) {
        const size_t off = bfrt ? (sel_lds + 15) / 16 * 16 : 0, want = off + (size_t)L.ldt * sizeof(double);
        if (select_lds_fits(h, rule, shape, want)) { L.rho_off = (int)off; plan->lds = want; }
    }
    plan->fn = select_kernel(rule, shape); plan->helper_dim = shape != SHAPE_P1; plan->norms = pdv ? &h->pdv : dvx ? &h->dvx : nullptr;
    plan->cap2 = bfrt ? cap2 : 0;
    // (measured, BSLV_SELECT_NT: S-degenerate, 2011 columns, 64 LPs per step: LP phase 67.6 / 52.0 / 46.6 ms with 256 / 512 / 1024 threads;
    //  S-degenerate-q4 to termination with 256 LPs per step 12.1 -> 10.4 s; same pivots)
    plan->nt = getenv("BSLV_SELECT_NT") ? atoi(getenv("BSLV_SELECT_NT")) : (L.N >= 1536 ? NT_BIG : NT);
    plan->per_launch = (getenv("BSLV_SELECT_FUSE") && atoi(getenv("BSLV_SELECT_FUSE")) == 0) ? 1 : KP;
    const bool cache = !(getenv("BSLV_SELECT_CACHE") && atoi(getenv("BSLV_SELECT_CACHE")) == 0);      // 0: k_select<false> where k_select_cached would run (same results bit for bit, tests/test_lp_select_cache_gpu.py)
    plan->cpt = (cache && !dvx && !bfrt && !L.rev && plan->nt == NT && L.N <= 6 * NT) ? (L.N <= 2 * NT ? 2 : (L.N <= 4 * NT ? 4 : 6)) : 0;
    return 0;
}
// revised form: helper workgroups for the sparse products of a tableau row (rev_helper), as many per LP as the chip holds beside the
// `running` LPs' own workgroups (of nt threads) without anyone waiting for a place
static int rev_helper_count(const LpView &L, int nt, int running)
{
    if (!L.rev || nt != NT_BIG) return 1;
    static const int hmax = getenv("BSLV_REV_HELPERS") ? std::max(1, atoi(getenv("BSLV_REV_HELPERS"))) : 32;
    return std::max(1, std::min(std::min(hmax, (L.ld + 2047) / 2048), 256 / std::max(1, running)));
}
// the KP selections of one round for the `running` LPs of the active list
static void launch_select(bslv_lpq *h, const SelectPlan &p, const BatchView &bv, int running)
{
    LpView &L = h->L; hipStream_t s = h->stream;
    for (int lev = 0; lev < KP; lev += p.per_launch) {
        const int helpers = rev_helper_count(L, p.nt, running);
        L.helpers = helpers; L.launch_id = (++h->launch_seq) & 0x3FFFFF;
        if (p.cpt == 2) hipLaunchKernelGGL(k_select_cached<2>, dim3(running), dim3(NT), 0, s, L, bv, h->active_d, running, p.per_launch);
        else if (p.cpt == 4) hipLaunchKernelGGL(k_select_cached<4>, dim3(running), dim3(NT), 0, s, L, bv, h->active_d, running, p.per_launch);
        else if (p.cpt == 6) hipLaunchKernelGGL(k_select_cached<6>, dim3(running), dim3(NT), 0, s, L, bv, h->active_d, running, p.per_launch);
        else {
            // (LpView, BatchView, [NormView,] active, nact, cap2, nsel)
            NormView nv = p.norms ? p.norms->view() : NormView{};
            void *priced[] = {&L, (void *)&bv, &nv, &h->active_d, &running, (void *)&p.cap2, (void *)&p.per_launch};
            void *plain[] = {&L, (void *)&bv, &h->active_d, &running, (void *)&p.cap2, (void *)&p.per_launch};
            (void)hipLaunchKernel(p.fn, dim3(running, p.helper_dim ? helpers : 1), dim3(p.nt), p.norms ? priced : plain, p.lds, s);
        }
    }
}
// Devex pricing, the steps of a batch that keeps reference norms (rec: bslv_lpq::dvx with rows of ld = Mp1p values, ::pdv with ld = ld).
// The start of a solve: room for the engine's largest batch, counters at zero, every norm at 1; rec.B = 0 for a batch not under the rule
static int devex_begin(bslv_lpq *h, DevexNorms &rec, bool on, int B, int ld, hipStream_t s)
{
    rec.B = on ? B : 0;
    if (!on) return 0;
    if (rec.Bcap < h->Bcap) {
        if (rec.norm_d) (void)hipFree(rec.norm_d);
        rec.norm_d = nullptr; rec.Bcap = 0;
        HIP_TRY(malloc0s(&rec.norm_d, (size_t)h->Bcap * ld * sizeof(double), s));
        rec.Bcap = h->Bcap;
    }
    if (!rec.stat_d) HIP_TRY(malloc0s(&rec.stat_d, 4 * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(rec.stat_d, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(k_norm_ones, dim3((ld + 255) / 256, B), dim3(256), 0, s, rec.view(), ld, (const int *)nullptr, B, 0);
    return 0;
}
// a new reference framework, counted, for the n LPs of the device list `due` (a refactorisation replay in the rounds)
static void devex_reframe(bslv_lpq *h, const DevexNorms &rec, int ld, const int *due, int n)
{
    if (rec.B > 0) hipLaunchKernelGGL(k_norm_ones, dim3((ld + 255) / 256, n), dim3(256), 0, h->stream, rec.view(), ld, due, n, 1);
}
// the end of a solve: the batch's counters are added to those of the call (added: the rescue's solves count with the call)
static int devex_collect(bslv_lpq *h, DevexNorms &rec)
{
    if (rec.B <= 0) return 0;
    int ds[3];
    HIP_TRY(hipMemcpy(ds, rec.stat_d, sizeof ds, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) rec.last[k] += ds[k];
    return 0;
}
// the norms of a batch (what bslv_lpq_last_pricing_norms and .._primal_pricing_norms answer from) across the re-solves of a rescue, each
// a batch of its own whose LP k is LP lps[k] of this one: kept on the host, the re-solved LPs' rows taken over, put back when all is done
struct SavedNorms {
    DevexNorms &rec; const int ld, B; std::vector<double> v;
    SavedNorms(DevexNorms &r, int ld_) : rec(r), ld(ld_), B(r.B) {}
    int save() { if (B > 0) { v.resize((size_t)B * ld); HIP_TRY(hipMemcpy(v.data(), rec.norm_d, v.size() * sizeof(double), hipMemcpyDeviceToHost)); } return 0; }
    int take(const std::vector<int> &lps, int m)      // (after a re-solve of m LPs that ran under the rule)
    {
        if (B > 0 && rec.B == m) for (int k = 0; k < m; k++) HIP_TRY(hipMemcpy(&v[(size_t)lps[k] * ld], rec.norm_d + (size_t)k * ld, (size_t)ld * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    int restore() { if (B > 0) { HIP_TRY(hipMemcpy(rec.norm_d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice)); rec.B = B; } return 0; }
};
static int solve_batch_rescue(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                              int cfirst, int ccnt, const double *cvals, int *status, int *iters);
// ---- periodic refactorisation inside a solve (bslv_lpq_set_refactor_period): host side (the kernels: k_per_*, k_rfx_*) ----
// The replay of k_rfx_* overwrites, for the batch indices it runs on, everything a batch keeps per LP.  In the middle of a batch those
// belong to running LPs, so it gets a BatchView of its own, as the parked passes have (park_view): its LP k is LP due[k] of the batch,
// in place on that LP's slot, with its own counters, pending pivots, reduced-cost row and work lists (so its passes do not count into
// the work lists of the rounds).  Sized with the batch buffers BEFORE the rounds start: nothing is allocated while a batch is in flight.
static int ensure_rfx(bslv_lpq *h);
static void period_free(bslv_lpq *h)
{
    bslv_lpq::Period &P = h->per;
    auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    fr(P.src); fr(P.dst); fr(P.status); fr(P.iters); fr(P.mode); fr(P.ver); fr(P.npend); fr(P.flushed); fr(P.pflags); fr(P.stall);
    fr(P.work); fr(P.nwork); fr(P.iota); fr(P.due); fr(P.res); fr(P.stat); fr(P.desc); fr(P.prow); fr(P.pcol); fr(P.dcur); fr(P.uvec); fr(P.xfull);
    for (auto &e : P.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    P.ev.clear();
    P.cap = 0; P.nwcap = 0;
}
// the rounds of a replay at most (a round = KP replay steps on vectors, one pass); its refresh pass counts in work list replay_rounds_max + 1
static int replay_rounds_max(const LpView &L) { return (L.M + KP - 1) / KP + 2; }
static int ensure_period(bslv_lpq *h)
{
    bslv_lpq::Period &P = h->per;
    const LpView &L = h->L;
    int rc;
    if ((rc = ensure_rfx(h))) return rc;
    if (P.cap >= h->Bcap && P.src) return 0;
    period_free(h);
    const size_t cap = (size_t)h->Bcap;
    for (int **p : {&P.src, &P.dst, &P.status, &P.iters, &P.mode, &P.ver, &P.npend, &P.flushed, &P.pflags, &P.stall, &P.work, &P.iota, &P.due, &P.res}) HIP_TRY(malloc0(p, cap * sizeof(int)));
    P.nwcap = replay_rounds_max(L) + 2;
    HIP_TRY(malloc0(&P.nwork, (size_t)P.nwcap * sizeof(int)));
    HIP_TRY(malloc0(&P.stat, 2 * sizeof(long long)));
    HIP_TRY(malloc0(&P.desc, cap * KP * sizeof(PivDesc)));
    HIP_TRY(malloc0(&P.prow, cap * KP * L.ldt * sizeof(double)));
    HIP_TRY(malloc0(&P.pcol, cap * KP * L.Mp1p * sizeof(double)));
    HIP_TRY(malloc0(&P.dcur, cap * L.ld * sizeof(double)));
    HIP_TRY(malloc0(&P.uvec, cap * L.ldt * sizeof(double)));
    HIP_TRY(malloc0(&P.xfull, cap * L.N * sizeof(double)));
    std::vector<int> iota(cap);
    for (size_t k = 0; k < cap; k++) iota[k] = (int)k;
    HIP_TRY(hipMemcpy(P.iota, iota.data(), cap * sizeof(int), hipMemcpyHostToDevice));
    P.cap = h->Bcap;
    return 0;
}
static BatchView period_view(bslv_lpq *h, const BatchView &bv)
{
    const bslv_lpq::Period &P = h->per;
    BatchView v = bv;      // (bounds, costs and the selection's scratch stay the batch's: the replay reads none of them)
    v.src = P.src; v.dst = P.dst; v.status = P.status; v.iters = P.iters; v.mode = P.mode; v.verified = P.ver; v.npend = P.npend; v.flushed = P.flushed;
    v.pflags = P.pflags; v.stall = P.stall; v.work = P.work; v.nwork = P.nwork;
    v.desc = P.desc; v.prow = P.prow; v.pcol = P.pcol; v.dcur = P.dcur; v.uvec = P.uvec; v.xfull = P.xfull;
    v.lazy = 0;
    return v;
}
static RfxView rfx_view(const bslv_lpq *h)
{
    const size_t BM = (size_t)h->Bcap * h->L.M;
    RfxView R;
    R.enter = h->rfx_i_d; R.rowvar = h->rfx_i_d + BM; R.elig = h->rfx_i_d + 2 * BM; R.cnt = h->rfx_c_d; R.cost = h->cost_d;
    return R;
}
}  // extern "C"
// THE REPLAY (the kernels: k_rfx_*), for the explicit rebuild and the periodic refactorisation alike, in two pieces with the pricing,
// which differs, between them.  replay_rebuild: B^-1 of the n LPs of the view rv is rebuilt in their dst slots from the heads there
// (through k_rfx_finish); returns the rounds made in *rounds.  replay_refresh: k_rev_u and the refresh pass for beta.  iota: 0..n-1 on
// the device, the active list of the replay's passes.  pass(cnt_slot): one tableau pass over the work list that k_list_pending has
// just written there -- the callers differ in how they launch and account it.
template <class Pass>
static int replay_pass(bslv_lpq *h, const BatchView &rv, const int *iota, int n, int cnt_slot, Pass &pass)
{
    hipLaunchKernelGGL(k_list_pending, dim3((n + 255) / 256), dim3(256), 0, h->stream, rv, iota, n, cnt_slot);
    return pass(cnt_slot);
}
template <class Pass>
static int replay_rebuild(bslv_lpq *h, const BatchView &rv, const int *iota, int n, Pass &pass, int *rounds_out = nullptr)
{
    LpView &L = h->L;
    hipStream_t s = h->stream;
    const int M = L.M;
    int rc;
    const RfxView R = rfx_view(h);
    hipLaunchKernelGGL(k_rfx_setup, dim3(n), dim3(NT), 0, s, L, rv, R, n);
    {
        const size_t total = (size_t)M * L.ldt;
        hipLaunchKernelGGL(k_rfx_identity, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096), n), dim3(256), 0, s, L, rv, R, n);
    }
    HIP_TRY(hipGetLastError());
    std::vector<int> cnt((size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(cnt.data(), h->rfx_c_d, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int kmax = 0;
    for (int k = 0; k < n; k++) if (cnt[(size_t)k * 4 + 2] == RFX_RUN) kmax = std::max(kmax, cnt[(size_t)k * 4]);
    // one round = KP replay steps on vectors, one pass; an LP with fewer structural basics is done earlier and is passed over
    const int rounds = std::min((kmax + KP - 1) / KP, replay_rounds_max(L));
    const int snt = M >= 1536 ? NT_BIG : NT;
    for (int it = 0; it < rounds; it++) {
        hipLaunchKernelGGL(k_rfx_select, dim3(n), dim3(snt), 0, s, L, rv, R, n, KP);
        if ((rc = replay_pass(h, rv, iota, n, it, pass))) return rc;
    }
    hipLaunchKernelGGL(k_rfx_finish, dim3(n), dim3(NT), 0, s, L, rv, R, n);
    if (rounds_out) *rounds_out = rounds;
    return 0;
}
// after the caller's pricing (y, the reduced costs): uvec = -K_N x_N and beta[M], then the refresh pass for beta
template <class Pass>
static int replay_refresh(bslv_lpq *h, const BatchView &rv, const int *iota, int n, Pass &pass)
{
    hipLaunchKernelGGL(k_rev_u, dim3(n), dim3(NT), 0, h->stream, h->L, rv, n, (const int *)nullptr, 0);
    return replay_pass(h, rv, iota, n, replay_rounds_max(h->L) + 1, pass);
}
// y for the replay's LP k = LP due[k] of the batch view bv (the explicit rebuild: rv = bv, due = iota), into rv's uvec
static void replay_y(bslv_lpq *h, const BatchView &bv, const BatchView &rv, const int *due, int n)
{
    hipLaunchKernelGGL(k_per_y, dim3((h->L.ldt + 255) / 256, n), dim3(256), 0, h->stream, h->L, bv, rv, due, (const double *)h->cost_d, n);
}
extern "C" {
// The n LPs of the batch that k_per_due listed (per.due, batch indices in the order of the active list) are refactorised in their dst
// slots and go on -- bounds, nonbasic statuses and values, iteration count, pflags, stall and Bland state and their place in the batch are
// not touched; the matrix, the heads of the basic variables, beta and the true reduced costs are rebuilt before the next selection.  An
// LP whose basis the replay finds singular ends UNDEFINED (status_h follows).  at_start: counts in out[0], else in out[1].
static int period_refactor(bslv_lpq *h, const BatchView &bv, int n, bool at_start)
{
    bslv_lpq::Period &P = h->per;
    hipStream_t s = h->stream;
    const auto t0 = std::chrono::steady_clock::now();
    int rc, rounds = 0;
    const BatchView rv = period_view(h, bv);
    HIP_TRY(hipMemsetAsync(P.nwork, 0, (size_t)P.nwcap * sizeof(int), s));
    hipLaunchKernelGGL(k_per_setup, dim3((n + 255) / 256), dim3(256), 0, s, bv, rv, (const int *)P.due, n);
    // no host wait after a pass; its events are read when the call is over.  All of the replay is on the stream before the next selection.
    auto pass = [&](int cnt_slot) -> int {
        if (h->profile) { P.ev.emplace_back(nullptr, nullptr); if ((rc = event_pair(&P.ev.back()))) return rc; }
        return flush_launch(h, rv, cnt_slot, n, h->profile ? &P.ev.back() : nullptr);
    };
    if ((rc = replay_rebuild(h, rv, P.iota, n, pass, &rounds))) return rc;
    // the LP's own costs on the rebuilt inverse -> its reduced costs (and the perturbed row's offsets), then beta
    replay_y(h, bv, rv, P.due, n);
    hipLaunchKernelGGL(k_per_price, dim3((h->L.ld + REV_PRICE_SLICE - 1) / REV_PRICE_SLICE, n), dim3(NT), 0, s, h->L, bv, rv, (const int *)P.due, (const double *)h->cost_d, n);
    if ((rc = replay_refresh(h, rv, P.iota, n, pass))) return rc;
    hipLaunchKernelGGL(k_per_resume, dim3((n + 255) / 256), dim3(256), 0, s, bv, rv, rfx_view(h), (const int *)P.due, n, h->age0_d, P.res);
    // Devex pricing: the replay may have moved heads between rows, so the LPs go on in a new reference framework (at the start they are in one)
    if (!at_start) { devex_reframe(h, h->pdv, h->L.ld, P.due, n); devex_reframe(h, h->dvx, h->L.Mp1p, P.due, n); }
    HIP_TRY(hipGetLastError());
    std::vector<int> due(n), res(n), nw(P.nwcap);
    HIP_TRY(hipMemcpyAsync(due.data(), P.due, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(res.data(), P.res, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nw.data(), P.nwork, (size_t)P.nwcap * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < n; k++) {
        if (res[k] >= 0) { h->last.per[at_start ? 0 : 1] += 1; h->last.per[2] += res[k]; }
        else { P.failed.push_back(due[k]); h->status_h[due[k]] = BSLV_LP_UNDEFINED; }
    }
    for (int k = 0; k < P.nwcap; k++) P.passes += nw[k];
    P.launches += rounds + 1;
    P.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
// tie phase: pivots an LP may spend in it (Bland's rule holds from PRIMAL_STALL on), and the rounds that leaves a batch at most --
// every round an LP of the phase is in makes a pivot or ends it, except the one it waits in for a pass with KP pivots pending
static int tie_cap(const LpView &L) { return 2 * PRIMAL_STALL + 2 * (L.M + L.N); }
static int tie_rounds_max(const LpView &L) { return tie_cap(L) + 8; }
// the per-LP vectors of a tie phase, for batches as large as the batch buffers (gstride doubles of g per LP: Mp1p, objective batches ld)
static int ensure_tie(bslv_lpq *h, TiePhase &r, int gstride)
{
    if (r.Bcap >= h->Bcap && r.g_d) return 0;
    auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    fr(r.g_d); fr(r.state_d); fr(r.iters_d);
    r.Bcap = 0;
    HIP_TRY(malloc0s(&r.g_d, (size_t)h->Bcap * gstride * sizeof(double), h->stream));
    HIP_TRY(malloc0s(&r.state_d, (size_t)h->Bcap * sizeof(int), h->stream));
    HIP_TRY(malloc0s(&r.iters_d, (size_t)h->Bcap * sizeof(int), h->stream));
    if (!r.stat_d) HIP_TRY(malloc0s(&r.stat_d, 4 * sizeof(int), h->stream));
    r.Bcap = h->Bcap;
    return 0;
}
// host wall clock of the calls an apply() makes for its tableaux (bslv_lpq_materialise, bslv_lpq_park): lazy_stats[2]
struct LazyClock { bslv_lpq *h; std::chrono::steady_clock::time_point t; ~LazyClock() { h->lazy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); } };
int bslv_lpq_set_lazy(bslv_lpq *h, int on)
{
    if (!h) return BSLV_E_ARG;
    if (!on && h->lazy_open) { int rc = materialise_indices(h, nullptr, 0); if (rc) return rc; h->lazy_open = false; }
    h->lazy = on != 0;
    return 0;
}
int bslv_lpq_materialise(bslv_lpq *h, int n, const int *slots)
{
    if (!h || n < 0 || (n && !slots)) { set_error("bslv_lpq_materialise: bad argument"); return BSLV_E_ARG; }
    if (n == 0 || (!h->lazy_open && h->park.live.empty())) return 0;
    std::vector<int> idx, parked;
    LazyClock clock{h, std::chrono::steady_clock::now()};
    {
        std::vector<int> where(h->slots, -1);
        if (h->lazy_open) for (size_t b = 0; b < h->last_dst.size(); b++) where[h->last_dst[b]] = (int)b;
        for (int k = 0; k < n; k++) {
            if (slots[k] < 0 || slots[k] >= h->slots) continue;
            if (where[slots[k]] >= 0) idx.push_back(where[slots[k]]);      // (a slot of the open batch, parked or not: materialise_indices)
            else if (h->park.cap && h->park.rec_of_slot[slots[k]] >= 0) parked.push_back(slots[k]);      // (parked by an earlier batch; the other slots of earlier batches have their tableau)
        }
    }
    if (!parked.empty()) {
        const int rc = park_before(h, (int)parked.size(), parked.data(), 0, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return materialise_indices(h, idx.data(), (int)idx.size());
}
int bslv_lpq_park(bslv_lpq *h, int n, const int *slots)
{
    if (!h || n < 0 || (n && !slots)) { set_error("bslv_lpq_park: bad argument"); return BSLV_E_ARG; }
    if (!h->lazy_open || n == 0) return 0;
    if (!h->park.on || h->L.rev || h->last_npend.size() != h->last_flushed_at + h->last_dst.size() || !park_alloc(h)) return bslv_lpq_materialise(h, n, slots);
    bslv_lpq::Park &P = h->park;
    LazyClock clock{h, std::chrono::steady_clock::now()};
    hipStream_t s = h->stream;
    if (P.pairs_inflight) HIP_TRY(hipStreamSynchronize(s));      // (a second park call for one batch: the pinned list of the first may not have been read yet)
    std::vector<int> where(h->slots, -1);
    for (size_t b = 0; b < h->last_dst.size(); b++) where[h->last_dst[b]] = (int)b;
    const int *npend = h->last_npend.data(), *flushed = npend + h->last_flushed_at;
    int m = 0;
    for (int k = 0; k < n; k++) {
        if (slots[k] < 0 || slots[k] >= h->slots || where[slots[k]] < 0 || P.rec_of_slot[slots[k]] >= 0) continue;
        const int b = where[slots[k]];
        if (!(npend[b] > 0 || !flushed[b])) continue;      // (k_list_given's condition: this slot has its tableau)
        const int rec = P.free_recs.back();
        P.free_recs.pop_back();
        P.rec_of_slot[slots[k]] = rec; P.slot_of[rec] = slots[k]; P.src_of[rec] = h->park_src[b]; P.flushed_of[rec] = flushed[b];
        P.pos_in_live[rec] = (int)P.live.size(); P.live.push_back(rec);
        P.pairs_h[2 * m] = b; P.pairs_h[2 * m + 1] = rec; m++;
    }
    if (m == 0) return 0;
    P.pairs_inflight = true;
    HIP_TRY(hipMemcpyAsync(P.pairs_d, P.pairs_h, (size_t)2 * m * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_park_copy, dim3(m), dim3(NT), 0, s, h->L, bview(h), park_view(h), (const int *)P.pairs_d, m);
    HIP_TRY(hipGetLastError());
    P.stats[0] += m;
    return 0;
}
int bslv_lpq_drop_parked(bslv_lpq *h, int n, const int *slots)
{
    if (!h || n < 0 || (n && !slots)) { set_error("bslv_lpq_drop_parked: bad argument"); return BSLV_E_ARG; }
    bslv_lpq::Park &P = h->park;
    if (!P.cap) return 0;
    for (int k = 0; k < n; k++) {
        if (slots[k] < 0 || slots[k] >= h->slots) continue;
        const int r = P.rec_of_slot[slots[k]];
        if (r >= 0) { park_release(h, r); P.stats[3]++; }
    }
    return 0;
}
int bslv_lpq_park_stats(const bslv_lpq *h, long out[5])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->park.stats[k];
    out[4] = (long)h->park.live.size();
    return 0;
}
int bslv_lpq_set_park(bslv_lpq *h, int on)
{
    if (!h) return BSLV_E_ARG;
    bslv_lpq::Park &P = h->park;
    if (!on && !P.live.empty()) {      // what is parked gets its tableau now, as if it had never been parked
        const std::vector<int> recs(P.live);
        P.stats[1] += (long)recs.size();
        const int rc = park_pass(h, recs.data(), (int)recs.size());
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    P.on = on != 0;
    return 0;
}
int bslv_lpq_get_park(const bslv_lpq *h) { return h && h->park.on; }
int bslv_lpq_discard_pending(bslv_lpq *h)
{
    if (!h) return BSLV_E_ARG;
    h->lazy_open = false;
    return 0;
}
int bslv_lpq_lazy_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    out[0] = h->lazy_skipped; out[1] = h->lazy_materialised; out[2] = (long)(h->lazy_ms * 1000.0);
    return 0;
}
int bslv_lpq_solve_batch(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo,
                         const double *vup, int *status, int *iters)
{
    if (h) h->call_method = h->method;
    return solve_batch_rescue(h, B, src, dst, vlo, vup, 0, 0, nullptr, status, iters);
}
// ... under `method` for this call only: see bslv_hip.h.  The engine's own method is neither read nor changed; in the revised form this
// is the way to PRIMAL and REPAIR (k_select_p1_rev), which bslv_lpq_set_method refuses there.
int bslv_lpq_solve_batch_method(bslv_lpq *h, int method, int B, const int *src, const int *dst, const double *vlo,
                                const double *vup, int *status, int *iters)
{
    if (!h || method < BSLV_LP_METHOD_DUAL || method > BSLV_LP_METHOD_REPAIR) { set_error("bslv_lpq_solve_batch_method: bad argument (method %d)", method); return BSLV_E_ARG; }
    h->call_method = method;
    return solve_batch_rescue(h, B, src, dst, vlo, vup, 0, 0, nullptr, status, iters);
}
// ... under `method` AND the two pricing rules of this call only: see bslv_hip.h.  The engine's method and switches are what they were
// when the call returns; while it runs `pricing` / `ppricing` hold the call's rules, so every batch of the call -- the rescue's re-solves
// included -- is planned under them (dvx_batch, pdv_batch), and call_priced lets them reach a PRIMAL / REPAIR batch of the revised form.
int bslv_lpq_solve_batch_method_priced(bslv_lpq *h, int method, int dual_rule, int primal_rule, int B, const int *src, const int *dst,
                                       const double *vlo, const double *vup, int *status, int *iters)
{
    const auto rule_ok = [](int r) { return r == BSLV_LP_PRICING_DANTZIG || r == BSLV_LP_PRICING_DEVEX; };
    if (!h || method < BSLV_LP_METHOD_DUAL || method > BSLV_LP_METHOD_REPAIR || !rule_ok(dual_rule) || !rule_ok(primal_rule)) {
        set_error("bslv_lpq_solve_batch_method_priced: bad argument (method %d, dual rule %d, primal rule %d)", method, dual_rule, primal_rule);
        return BSLV_E_ARG;
    }
    const int pricing0 = h->pricing, ppricing0 = h->ppricing;
    h->pricing = dual_rule; h->ppricing = primal_rule; h->call_priced = true;
    h->call_method = method;
    const int rc = solve_batch_rescue(h, B, src, dst, vlo, vup, 0, 0, nullptr, status, iters);
    h->pricing = pricing0; h->ppricing = ppricing0; h->call_priced = false;
    return rc;
}
// The LPs of the batch differ in their OBJECTIVE (lp_set_obj_coeffs + lp_solve, bslv_lp.c:141-151,219: what phase2_dual
// does per vertex, bslv_algs.c:1469-1477): cost costs[b*cost_cnt + t] on variable cost_first + t, 0 elsewhere (the engine's
// own cost vector must be zero).  Bounds: those of the last solve_batch / set_bounds for the per-LP range (vlo/vup may be
// NULL when the engine has no such range).  LP b starts from the basis of slot src[b], which must be primal feasible for
// these bounds (an optimal slot of any objective is), and runs primal simplex steps.
// (own_range: bslv_lpq_solve_batch_obj_canonical, whose tie phase takes the range of the call and not the one the engine's switch was set for)
static int solve_batch_obj_ranged(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                                  int cost_first, int cost_cnt, const double *costs, int *status, int *iters, bool own_range)
{
    if (!h || cost_cnt < 1 || cost_first < 0 || cost_first + cost_cnt > h->ps.M0 + h->ps.N0 || !costs) { set_error("bslv_lpq_solve_batch_obj: bad argument"); return BSLV_E_ARG; }
    if (!own_range && h->tie_obj.on && (cost_first != h->cobj_first || cost_cnt != h->cobj_cnt)) { set_error("bslv_lpq_solve_batch_obj: the cost range (%d, %d) is not the one bslv_lpq_set_canonical_obj was set for (%d, %d)", cost_first, cost_cnt, h->cobj_first, h->cobj_cnt); return BSLV_E_ARG; }
    if (h->ps.nfold) {      // indices of the model as given -> the engine's (a cost on a folded row would be a cost on its column: not asked for by any caller)
        for (int t = 0; t < cost_cnt; t++) if (h->ps.map_var(cost_first + t) != h->ps.map_var(cost_first) + t) { set_error("bslv_lpq_solve_batch_obj: the cost range covers rows the presolve folded into column bounds"); return BSLV_E_ARG; }
        cost_first = h->ps.map_var(cost_first);
    }
    for (size_t j = 0; j < h->cost.size(); j++) if (h->cost[j] != 0.0) { set_error("bslv_lpq_solve_batch_obj: the engine was created with a non-zero cost vector"); return BSLV_E_STATE; }
    h->call_method = h->method;
    const int rc = solve_batch_rescue(h, B, src, dst, vlo, vup, cost_first, cost_cnt, costs, status, iters);
    ++h->obj_batches;
    // test hook BSLV_LP_OBJ_UNDEFINED=K:b -- LP b of the K-th objective batch of this engine is REPORTED as UNDEFINED (as when the pivot
    // cross-check of the revised form gives it up): the callers' retry runs.  Only the status changes; the slot keeps what the solve left.
    if (const char *e = getenv("BSLV_LP_OBJ_UNDEFINED")) {
        int k = 0, lp = 0;
        if (!rc && status && sscanf(e, "%d:%d", &k, &lp) >= 1 && k == h->obj_batches && lp >= 0 && lp < B) status[lp] = BSLV_LP_UNDEFINED;
    }
    return rc;
}
int bslv_lpq_solve_batch_obj(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                             int cost_first, int cost_cnt, const double *costs, int *status, int *iters)
{
    return solve_batch_obj_ranged(h, B, src, dst, vlo, vup, cost_first, cost_cnt, costs, status, iters, false);
}
// ... under `method` for this call only: see bslv_hip.h.  PRIMAL is bslv_lpq_solve_batch_obj; DUAL and REPAIR make the parent's basis dual
// feasible for the new objective (k_obj_art, k_obj_start) and run dual simplex steps
int bslv_lpq_solve_batch_obj_method(bslv_lpq *h, int method, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                                    int cost_first, int cost_cnt, const double *costs, int *status, int *iters)
{
    if (!h || method < BSLV_LP_METHOD_DUAL || method > BSLV_LP_METHOD_REPAIR) { set_error("bslv_lpq_solve_batch_obj_method: bad argument (method %d)", method); return BSLV_E_ARG; }
    if (method != BSLV_LP_METHOD_PRIMAL && h->tie_obj.on) { set_error("bslv_lpq_solve_batch_obj_method: the tie phase of bslv_lpq_set_canonical_obj follows a PRIMAL objective solve only (method %d)", method); return BSLV_E_ARG; }
    h->call_obj_method = method;
    h->obj_call_dual = method != BSLV_LP_METHOD_PRIMAL;
    const int rc = solve_batch_obj_ranged(h, B, src, dst, vlo, vup, cost_first, cost_cnt, costs, status, iters, false);
    h->call_obj_method = BSLV_LP_METHOD_PRIMAL;
    h->obj_call_dual = false;
    return rc;
}
int bslv_lpq_last_obj_method_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->last.objm[k];
    return 0;
}
// One batch.  Its counters (BatchStats) are gathered in a record of its own and become the call's (h->last) when the batch is over:
// stored, or added for a re-solve of the rescue (resolve)
static int solve_batch_impl(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                            int cfirst, int ccnt, const double *cvals, int *status, int *iters, bool resolve)
{
    if (h && h->ps.empty_box && B > 0 && status) {        // (bslv_lpq_set_bounds left a folded row no room: fold_bounds)
        for (int b = 0; b < B; b++) { status[b] = BSLV_LP_INFEASIBLE; if (iters) iters[b] = 0; }
        h->last.iters = 0; h->last.pivots = 0; h->last.passes = 0; h->last.launches = 0;
        for (int k = 0; k < 3; k++) h->last.p1[k] = 0;
        for (int k = 0; k < 4; k++) h->tie.last[k] = 0;
        if (cvals) for (int k = 0; k < 4; k++) h->tie_obj.last[k] = 0;
        if (h->rays_on) h->last.ray[2] += B;      // (no slot is touched: nothing to hang a ray on)
        return 0;
    }
    if (!h || B < 0 || (B > 0 && (!src || !dst)) || (B > 0 && h->L.vcnt > 0 && (!vlo || !vup))) {
        set_error("bslv_lpq_solve_batch: bad argument");
        return BSLV_E_ARG;
    }
    if (B == 0) return 0;
    for (int b = 0; b < B; b++)
        if (src[b] < 0 || src[b] >= h->slots || dst[b] < 0 || dst[b] >= h->slots) {
            set_error("bslv_lpq_solve_batch: slot out of range at %d (src %d dst %d, pool %d)", b, src[b], dst[b], h->slots);
            return BSLV_E_ARG;
        }
    int rc;
    if (h->lazy_open) {        // a batch while slots of the last one are still without their tableau (a retry of the driver): all of them get it now
        if ((rc = materialise_indices(h, nullptr, 0))) return rc;
        h->lazy_open = false;
    }
    if ((rc = ensure_batch(h, B))) return rc;
    // periodic refactorisation: the replay's buffers are sized now, nothing is allocated once the batch is in flight
    const int period = h->L.rev ? h->period : 0;
    if (period > 0 && (rc = ensure_period(h))) return rc;
    h->per.passes = 0; h->per.launches = 0; h->per.ms = 0; h->per.failed.clear();
    // parked passes: the parents of this batch get their tableau, and so does whoever still reads a slot this batch overwrites
    // (before k_prep: the pass reads and writes slots the batch touches)
    if ((rc = park_before(h, B, src, B, dst))) return rc;
    LpView &L = h->L;
    auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = h->stream;
    // An objective batch under DUAL / REPAIR (bslv_lpq_solve_batch_obj_method): the kernels of the call see the call's own copy of the
    // bounds, to which k_obj_art adds its artificial ones; the engine's are put back when the call returns, on every path
    const int objm = cvals ? h->call_obj_method : BSLV_LP_METHOD_PRIMAL;
    struct BoundsBack { LpView &L; const double *lb, *ub; const unsigned char *art; ~BoundsBack() { L.lb = lb; L.ub = ub; L.art = art; } } bounds_back{L, L.lb, L.ub, L.art};
    if (objm != BSLV_LP_METHOD_PRIMAL) {
        const size_t n = (size_t)L.M + L.N, na = (n + 3) / 4 * 4;
        if (!h->clb_d) { HIP_TRY(malloc0s(&h->clb_d, n * sizeof(double), s)); HIP_TRY(malloc0s(&h->cub_d, n * sizeof(double), s)); HIP_TRY(malloc0s(&h->cart_d, na, s)); }
        HIP_TRY(hipMemcpyAsync(h->clb_d, h->lb_d, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->cub_d, h->ub_d, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->cart_d, h->art_d, n, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(h->src_d, src, B * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->dst_d, dst, B * sizeof(int), hipMemcpyHostToDevice, s));
    if (L.vcnt > 0) {
        HIP_TRY(hipMemcpyAsync(h->vlo_d, vlo, (size_t)B * L.vcnt * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->vup_d, vup, (size_t)B * L.vcnt * sizeof(double), hipMemcpyHostToDevice, s));
    }
    L.objmode = cvals ? 1 : 0; L.cfirst = cfirst; L.ccnt = ccnt;
    if (cvals) {
        const size_t need = (size_t)B * ccnt;
        if (need > h->cvals_cap) { if (h->cvals_d) (void)hipFree(h->cvals_d); h->cvals_d = nullptr; HIP_TRY(malloc0s(&h->cvals_d, need * sizeof(double), s)); h->cvals_cap = need; }
        HIP_TRY(hipMemcpyAsync(h->cvals_d, cvals, need * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (const char *e = getenv("BSLV_UPD_GRID")) h->upd_grid = std::max(64, atoi(e));
    {   // one work-list length per lock-step iteration, zeroed here: no reset between iterations
        const int need = L.maxit + 64 + ((h->tie.on || h->tie_obj.on || h->tie_call.on || h->tie_call_obj.on) ? tie_rounds_max(L) : 0);      // (the rounds of a tie phase count on behind the others')
        if ((rc = ensure_nwork(h, need, need))) return rc;
    }
    HIP_TRY(hipMemsetAsync(h->xstat_d, 0, 12 * sizeof(int), s));
    if (L.rfx) HIP_TRY(hipMemsetAsync(h->rmark_d, 0, (size_t)B * sizeof(int), s));
    // Devex pricing: the reference norms of the batch start at 1
    const bool dvx = dvx_batch(h);
    const bool pdv = pdv_batch(h);
    if ((rc = devex_begin(h, h->dvx, dvx, B, L.Mp1p, s)) || (rc = devex_begin(h, h->pdv, pdv, B, L.ld, s))) return rc;
    BatchView bv = bview(h);
    bv.cvals = h->cvals_d;
    const int tiles = (L.mrows + TR - 1) / TR;
    if (L.rev) hipLaunchKernelGGL(k_age_begin, dim3((B + 255) / 256), dim3(256), 0, s, bv, (const long long *)h->age_d, h->age0_d, B);      // the age of every LP's matrix: its parent's
    {   // (objective batches keep their own start; both forms take the call's method: the engine's own, or bslv_lpq_solve_batch_method's)
        const int method = L.objmode ? BSLV_LP_METHOD_DUAL : h->call_method;
        if (method == BSLV_LP_METHOD_PRIMAL) hipLaunchKernelGGL(k_prep<BSLV_LP_METHOD_PRIMAL>, dim3(B), dim3(NT), 0, s, L, bv, B);
        else if (method == BSLV_LP_METHOD_REPAIR) hipLaunchKernelGGL(k_prep<BSLV_LP_METHOD_REPAIR>, dim3(B), dim3(NT), 0, s, L, bv, B);
        else hipLaunchKernelGGL(k_prep<BSLV_LP_METHOD_DUAL>, dim3(B), dim3(NT), 0, s, L, bv, B);
    }
    if (L.rev && L.objmode) {      // new objective: the reduced-cost row from the parent's B^-1 (k_rev_u takes beta[M] = d . x_N from it)
        const size_t ylds = (size_t)L.ldt * sizeof(double);
        bool in_lds = ylds <= h->price_lds_max;
        if (!in_lds && ylds <= 144 * 1024) {
            in_lds = hipFuncSetAttribute((const void *)k_rev_price, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ylds) == hipSuccess;
            if (in_lds) h->price_lds_max = ylds; else (void)hipGetLastError();
        }
        if (const char *e = getenv("BSLV_REV_PRICE_LDS")) in_lds = in_lds && atoi(e) != 0;      // test hook: 0 = y from global scratch (k_rev_y), as for M > ~18 000
        if (!in_lds) hipLaunchKernelGGL(k_rev_y, dim3(B), dim3(NT), 0, s, L, bv, B);
        hipLaunchKernelGGL(k_rev_price, dim3((L.ld + REV_PRICE_SLICE - 1) / REV_PRICE_SLICE, B), dim3(NT), in_lds ? ylds : 0, s, L, bv, B, in_lds ? 1 : 0);
    }
    if (objm != BSLV_LP_METHOD_PRIMAL) {      // the dual start: row first (k_prep / k_rev_price above), then the call's artificial bounds, then the sides; beta follows from them (k_rev_u, k_init)
        hipLaunchKernelGGL(k_obj_art, dim3(B), dim3(NT), 0, s, L, bv, B, reinterpret_cast<unsigned *>(h->cart_d), h->clb_d, h->cub_d);
        L.lb = h->clb_d; L.ub = h->cub_d; L.art = h->cart_d;
        if (objm == BSLV_LP_METHOD_DUAL) hipLaunchKernelGGL(k_obj_start<BSLV_LP_METHOD_DUAL>, dim3(B), dim3(NT), 0, s, L, bv, B);
        else hipLaunchKernelGGL(k_obj_start<BSLV_LP_METHOD_REPAIR>, dim3(B), dim3(NT), 0, s, L, bv, B);
    }
    if (L.rev) hipLaunchKernelGGL(k_rev_u, dim3(B), dim3(NT), 0, s, L, bv, B, (const int *)nullptr, 0);      // beta = B^-1 uvec (k_init)
    if (L.objmode && !L.rev) {      // new objective: the tableau rows are copied up front (the reduced-cost row is rebuilt by k_prep, not streamed from the parent)
        const int cnt_slot = L.maxit + 41;
        hipLaunchKernelGGL(k_list_unpivoted, dim3((B + 255) / 256), dim3(256), 0, s, bv, B, -cnt_slot);
        hipLaunchKernelGGL(k_copy_unpivoted, dim3(std::min(B * tiles, 2048)), dim3(NT), 0, s, L, bv, cnt_slot, tiles);
    }
    InitPlan ip;
    plan_init(h, B, src, &ip);
    if (ip.epl) {
        HIP_TRY(hipMemcpyAsync(h->init_d, h->init_h, ((size_t)B + 2 * (size_t)ip.chunks) * sizeof(int), hipMemcpyHostToDevice, s));
        const int *order = h->init_d;
        const InitChunk *chunks = reinterpret_cast<const InitChunk *>(h->init_d + B);
        const dim3 grid(ip.tiles, ip.chunks);
        if (ip.epl == 1) hipLaunchKernelGGL((k_init_grouped<1, 8>), grid, dim3(NT), 0, s, L, bv, order, chunks);
        else if (ip.epl == 2) hipLaunchKernelGGL((k_init_grouped<2, 8>), grid, dim3(NT), 0, s, L, bv, order, chunks);
        else if (ip.epl == 4) hipLaunchKernelGGL((k_init_grouped<4, 8>), grid, dim3(NT), 0, s, L, bv, order, chunks);
        else if (ip.epl == 8) hipLaunchKernelGGL((k_init_grouped<8, 4>), grid, dim3(NT), 0, s, L, bv, order, chunks);
        else hipLaunchKernelGGL((k_init_grouped<16, 2>), grid, dim3(NT), 0, s, L, bv, order, chunks);
    } else hipLaunchKernelGGL(k_init, dim3(tiles, B), dim3(NT), 0, s, L, bv, B);
    HIP_TRY(hipGetLastError());
    SelectPlan plan;
    if ((rc = plan_select(h, B, vlo, vup, &plan))) return rc;
    L.trace = getenv("BSLV_LP_TRACE") ? atoi(getenv("BSLV_LP_TRACE")) : -1;
    L.stall_limit = getenv("BSLV_STALL_LIMIT") ? atoi(getenv("BSLV_STALL_LIMIT")) : STALL_LIMIT;
    L.pert_scale = getenv("BSLV_PERT_SCALE") ? atof(getenv("BSLV_PERT_SCALE")) : 1.0;
    // One ROUND = KP lock-step selections on vectors (launch_select), then one pass over the tableaux of the LPs that have something
    // pending (k_flush).  The status vector is read back every 1, 2, 4, ... rounds.
    int it = 0, chunk = 1, running = B;
    for (int b = 0; b < B; b++) h->active_h[b] = b;
    HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, B * sizeof(int), hipMemcpyHostToDevice, s));
    size_t nev = 0;
    BatchStats st;
    static const int max_rounds = getenv("BSLV_LP_MAXROUNDS") ? atoi(getenv("BSLV_LP_MAXROUNDS")) : 0;      // (timing experiments)
    L.probe = getenv("BSLV_REV_PROBE") ? atoi(getenv("BSLV_REV_PROBE")) : 0;
    // PERIODIC REFACTORISATION (bslv_lpq_set_refactor_period): the LPs of the active list that are due are listed on the stream
    // (period_list, before a readback) and, once the host knows their number, refactorised in their slots and go on (period_refactor).
    // At the start of the call that is every LP k_prep accepted whose parent's matrix is old enough: it is rebuilt from the heads
    // k_prep left in dst before the first selection, and nothing of the parent's matrix enters what the LP computes.
    auto period_list = [&](const int nact, const bool at_start) {
        hipLaunchKernelGGL(k_per_due, dim3(1), dim3(NT), 0, s, bv, (const int *)h->active_d, nact, (const long long *)h->age0_d, (long long)period, at_start ? 1 : 0, h->per.due, h->per.stat);
    };
    long long per_stat[2] = {0, 0};
    if (period > 0) {
        HIP_TRY(hipMemsetAsync(h->per.stat, 0, sizeof per_stat, s));
        period_list(B, true);
        HIP_TRY(hipMemcpyAsync(per_stat, h->per.stat, sizeof per_stat, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (per_stat[0] > 0 && (rc = period_refactor(h, bv, (int)per_stat[0], true))) return rc;
    }
    // the pass of round `it` over the tableaux of the `running` LPs of the active list that have something pending
    auto pass_round = [&](const int running, const int it) -> int {
        hipLaunchKernelGGL(k_list_pending, dim3((running + 255) / 256), dim3(256), 0, s, bv, h->active_d, running, it);
        if (h->profile && nev == h->evpool.size()) {      // (pooled: no event is created per round once the pool has grown)
            EventPair ev;
            if ((rc = event_pair(&ev))) return rc;
            h->evpool.push_back(ev);
        }
        // (revised form: only the LPs that asked for a refresh of beta are done by k_rev_u)
        if ((rc = flush_launch(h, bv, it, running, h->profile ? &h->evpool[nev] : nullptr, L.rev ? h->work_d : nullptr))) return rc;
        if (h->profile) nev++;
        return 0;
    };
    while (running > 0 && it < L.maxit + 8 && !(max_rounds && it >= max_rounds)) {
        for (int c = 0; c < chunk; c++, it++) {
            launch_select(h, plan, bv, running);
            if ((rc = pass_round(running, it))) return rc;
        }
        HIP_TRY(hipGetLastError());
        if (period > 0) { period_list(running, false); HIP_TRY(hipMemcpyAsync(per_stat, h->per.stat, sizeof per_stat, hipMemcpyDeviceToHost, s)); }
        HIP_TRY(hipMemcpyAsync(h->status_h, h->status_d, B * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // (the pass of the round has just been made: nothing is pending for any running LP)
        if (period > 0 && per_stat[0] > 0 && (rc = period_refactor(h, bv, (int)per_stat[0], false))) return rc;
        running = 0;
        for (int b = 0; b < B; b++) if (h->status_h[b] == ST_RUNNING) h->active_h[running++] = b;
        if (running) HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, running * sizeof(int), hipMemcpyHostToDevice, s));
        if (chunk < 16) chunk *= 2;
        // with a period the status vector is read at least every max(1, K / KP) rounds: an LP below K at one readback has made at most
        // max(KP, K) pivots more at the next, so no selection is made on a matrix older than 2 K + KP
        if (period > 0) chunk = std::min(chunk, std::max(1, period / KP));
    }
    // the ray store: kind and vector of every dst slot (k_ray; before the tie phases, which reuse the scratch of their OPTIMAL LPs)
    if (h->rays_on) {
        static const bool tm = getenv("BSLV_LP_RAY_TIMING") != nullptr;      // one line per solve call on stderr: the HIP-event time of k_ray
        EventPair ev{nullptr, nullptr};
        if (tm && (rc = event_pair(&ev))) return rc;
        HIP_TRY(hipMemsetAsync(h->raystat_d, 0, 3 * sizeof(int), s));
        if (tm) HIP_TRY(hipEventRecord(ev.first, s));
        hipLaunchKernelGGL(k_ray, dim3(B), dim3(NT), 0, s, L, bv, RayView{h->raykind_d, h->ray_d, h->raystat_d}, B);
        if (tm) HIP_TRY(hipEventRecord(ev.second, s));
        HIP_TRY(hipGetLastError());
        int rs[3];
        HIP_TRY(hipMemcpyAsync(rs, h->raystat_d, sizeof rs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 3; k++) h->last.ray[k] += rs[k];      // (added: the rescue's solves count with the call)
        if (tm) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev.first, ev.second);
            (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second);
            fprintf(stderr, "bslv_lpq k_ray: %d LPs (%s form, %d x %d), %d FARKAS, %d DIRECTION, %d without a ray: %.3f ms\n", B, L.rev ? "revised" : "tableau", L.M, L.N, rs[0], rs[1], rs[2], ms);
        }
    }
    // TIE PHASE (bslv_lpq_set_canonical; objective batches: bslv_lpq_set_canonical_obj): the LPs that ended OPTIMAL go on to their
    // canonical basis, in rounds of the same shape -- KP tie pivots on vectors (k_select_tie / k_select_tie_obj), one pass.  Their work
    // lists count on from L.maxit + 64.
    int tie_rounds = 0;
    const int tie_base = L.maxit + 64;
    // the rounds of the tie phase r: launch(nt) selects for the nt LPs of the active list
    auto tie_phase = [&](TiePhase &r, auto launch) -> int {
        HIP_TRY(hipMemsetAsync(r.state_d, 0, (size_t)B * sizeof(int), s));
        HIP_TRY(hipMemsetAsync(r.iters_d, 0, (size_t)B * sizeof(int), s));
        HIP_TRY(hipMemsetAsync(r.stat_d, 0, 4 * sizeof(int), s));
        int nt = 0;
        for (int b = 0; b < B; b++) if (h->status_h[b] == BSLV_LP_OPTIMAL) h->active_h[nt++] = b;
        if (nt) HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, nt * sizeof(int), hipMemcpyHostToDevice, s));
        std::vector<int> tstate(B);
        const int rounds_max = tie_rounds_max(L);
        int tchunk = 1;
        while (nt > 0 && tie_rounds < rounds_max) {
            for (int c = 0; c < tchunk && tie_rounds < rounds_max; c++, tie_rounds++) {
                launch(nt);
                if ((rc = pass_round(nt, tie_base + tie_rounds))) return rc;
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(tstate.data(), r.state_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            int left = 0;
            for (int k = 0; k < nt; k++) { const int b = h->active_h[k]; if (tstate[b] != TIE_DONE) h->active_h[left++] = b; }
            nt = left;
            if (nt) HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, nt * sizeof(int), hipMemcpyHostToDevice, s));
            if (tchunk < 16) tchunk *= 2;
        }
        HIP_TRY(hipMemcpyAsync(h->status_h, h->status_d, B * sizeof(int), hipMemcpyDeviceToHost, s));
        int ts[4];
        HIP_TRY(hipMemcpyAsync(ts, r.stat_d, sizeof ts, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 4; k++) r.last[k] = ts[k];
        // (the cap on the pivots of an LP ends every phase long before the rounds run out; an LP still in it would keep the basis reached)
        for (int k = 0; k < nt; k++) { const int b = h->active_h[k]; if (h->status_h[b] == ST_RUNNING) { h->status_h[b] = BSLV_LP_OPTIMAL; r.last[3]++; HIP_TRY(hipMemcpy(h->status_d + b, h->status_h + b, sizeof(int), hipMemcpyHostToDevice)); } }
        return 0;
    };
    long tie_before[4] = {0, 0, 0, 0};
    if (resolve && h->tie_call.on) for (int k = 0; k < 4; k++) tie_before[k] = h->tie.last[k];      // (bslv_lpq_solve_batch_canonical: the rescue's solves count with the call)
    long tie_obj_before[4] = {0, 0, 0, 0};
    if (resolve && h->tie_call_obj.on) for (int k = 0; k < 4; k++) tie_obj_before[k] = h->tie_obj.last[k];      // (bslv_lpq_solve_batch_obj_canonical: likewise)
    for (int k = 0; k < 4; k++) h->tie.last[k] = 0;
    if (L.objmode) for (int k = 0; k < 4; k++) h->tie_obj.last[k] = 0;
    // (the engine's switch is the tableau form's alone: bslv_lpq_set_canonical; the call's own direction holds in both forms)
    if ((h->tie.on || h->tie_call.on) && !L.objmode && L.vcnt > 0 && !max_rounds) {
        if ((rc = ensure_tie(h, h->tie, L.Mp1p))) return rc;
        TieView tv = h->tie.view(tie_cap(L));
        if (h->tie_call.on) tv.dir = h->tie_call.dir_d;
        if (!L.rev) {
            if ((rc = tie_phase(h->tie, [&](int nt) { hipLaunchKernelGGL(k_select_tie, dim3(nt), dim3(plan.nt), 0, s, L, bv, tv, h->active_d, nt, KP); }))) return rc;
        } else {
            // revised form: the dynamic LDS is rho alone; helpers and the launch number per launch, as launch_select sets them
            const size_t want = (size_t)L.ldt * sizeof(double);
            L.rho_off = select_lds_fits(h, 0, SHAPE_TIE_REV, want) ? 0 : -1;
            const size_t lds = L.rho_off == 0 ? want : 0;
            if ((rc = tie_phase(h->tie, [&](int nt) {
                    const int helpers = rev_helper_count(L, plan.nt, nt);
                    L.helpers = helpers; L.launch_id = (++h->launch_seq) & 0x3FFFFF;
                    hipLaunchKernelGGL(k_select_tie_rev, dim3(nt, helpers), dim3(plan.nt), lds, s, L, bv, tv, h->active_d, nt, KP);
                }))) return rc;
        }
    }
    for (int k = 0; k < 4; k++) h->tie.last[k] += tie_before[k];
    // (again the engine's switch is the tableau form's alone, bslv_lpq_set_canonical_obj, and the call's own direction holds in both forms)
    if ((h->tie_obj.on || h->tie_call_obj.on) && L.objmode && !max_rounds) {
        if ((rc = ensure_tie(h, h->tie_obj, L.ld))) return rc;
        TieView tv = h->tie_obj.view(tie_cap(L));
        if (h->tie_call_obj.on) tv.dir = h->tie_call_obj.dir_d;
        if (!L.rev) {
            if ((rc = tie_phase(h->tie_obj, [&](int nt) { hipLaunchKernelGGL(k_select_tie_obj, dim3(nt), dim3(plan.nt), 0, s, L, bv, tv, h->active_d, nt, KP); }))) return rc;
        } else {
            const size_t want = (size_t)L.ldt * sizeof(double);
            L.rho_off = select_lds_fits(h, 0, SHAPE_TIE_OBJ_REV, want) ? 0 : -1;
            const size_t lds = L.rho_off == 0 ? want : 0;
            if ((rc = tie_phase(h->tie_obj, [&](int nt) {
                    const int helpers = rev_helper_count(L, plan.nt, nt);
                    L.helpers = helpers; L.launch_id = (++h->launch_seq) & 0x3FFFFF;
                    hipLaunchKernelGGL(k_select_tie_obj_rev, dim3(nt, helpers), dim3(plan.nt), lds, s, L, bv, tv, h->active_d, nt, KP);
                }))) return rc;
        }
    }
    if (L.objmode) for (int k = 0; k < 4; k++) h->tie_obj.last[k] += tie_obj_before[k];
    {   // tableau passes of this batch: sum of the work-list lengths of the rounds
        std::vector<int> nw(std::max(it, 1), 0);
        if (it > 0) HIP_TRY(hipMemcpy(nw.data(), h->nwork_d, (size_t)it * sizeof(int), hipMemcpyDeviceToHost));
        long passes = 0;
        for (int k = 0; k < it; k++) passes += nw[k];
        if (tie_rounds > 0) {
            nw.assign(tie_rounds, 0);
            HIP_TRY(hipMemcpy(nw.data(), h->nwork_d + tie_base, (size_t)tie_rounds * sizeof(int), hipMemcpyDeviceToHost));
            for (int k = 0; k < tie_rounds; k++) passes += nw[k];
        }
        st.passes = passes + h->per.passes;      // (the replay's passes count in work lists of their own)
    }
    if (L.rev) hipLaunchKernelGGL(k_rev_store_d, dim3((L.ld + 255) / 256, B), dim3(256), 0, s, L, bv, B);       // the reduced costs of every LP go to its slot
    if (bv.lazy) {
        // the slots keep what they hold; the reduced costs go to row M (the getters read them there), the rest waits for bslv_lpq_materialise
        hipLaunchKernelGGL(k_store_d, dim3((L.ld + 255) / 256, B), dim3(256), 0, s, L, bv, B);
        HIP_TRY(hipGetLastError());
        h->last_dst.assign(dst, dst + B);
        h->park_src.assign(src, src + B);
        h->lazy_open = true;
        h->last_npend.clear();
        if (h->park.on) {      // which LPs still need a pass, and whether it reads their parent's slot: bslv_lpq_park decides on the host
            h->last_flushed_at = (size_t)h->Bcap;
            h->last_npend.resize(h->last_flushed_at + B);
            HIP_TRY(hipMemcpy(h->last_npend.data(), h->npend_d, h->last_npend.size() * sizeof(int), hipMemcpyDeviceToHost));
        }
        h->lazy_skipped += B - std::min<long>(B, st.passes);
    } else {   // tableaux of the solves that made no pivot
        const int cnt_slot = L.maxit + 40;
        hipLaunchKernelGGL(k_list_unpivoted, dim3((B + 255) / 256), dim3(256), 0, s, bv, B, cnt_slot);
        hipLaunchKernelGGL(k_copy_unpivoted, dim3(std::min(B * tiles, 2048)), dim3(NT), 0, s, L, bv, cnt_slot, tiles);
        HIP_TRY(hipGetLastError());
    }
    if (L.rev) hipLaunchKernelGGL(k_age_end, dim3((B + 255) / 256), dim3(256), 0, s, bv, h->age_d, (const long long *)h->age0_d, B);
    if (period > 0) {
        HIP_TRY(hipMemcpy(per_stat, h->per.stat, sizeof per_stat, hipMemcpyDeviceToHost));
        h->last.per[3] = std::max(h->last.per[3], (long)per_stat[1]);
        // a slot whose replay failed holds a half-built matrix: it is reset, as bslv_lpq_refactor does (now: the solve has left its vectors in it)
        for (int b : h->per.failed) if ((rc = bslv_lpq_reset_slot(h, dst[b]))) return rc;
    }
    if (status) for (int b = 0; b < B; b++) status[b] = h->status_h[b] == ST_RUNNING ? BSLV_LP_UNDEFINED : h->status_h[b];
    if (L.rfx) { h->rmark_h.resize(B); HIP_TRY(hipMemcpy(h->rmark_h.data(), h->rmark_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost)); h->rmark_valid = true; }      // (the LPs the pivot cross-check gave up: solve_batch_rescue)
    {
        std::vector<int> itv(B);
        HIP_TRY(hipMemcpy(itv.data(), h->iters_d, B * sizeof(int), hipMemcpyDeviceToHost));
        long piv = 0;
        for (int b = 0; b < B; b++) piv += itv[b];
        st.pivots = piv;
        if (iters) memcpy(iters, itv.data(), B * sizeof(int));
    }
    st.iters = it + tie_rounds;
    st.launches = it + tie_rounds + h->per.launches;
    {   // the unpark passes made since the last batch count with this one (they ran on the stream before its first kernel)
        bslv_lpq::Park &P = h->park;
        st.passes += P.pre_passes; st.launches += P.pre_launches;
        P.pre_passes = 0; P.pre_launches = 0;
        P.list_inflight = false; P.pairs_inflight = false;      // (the readbacks above have waited for the stream)
    }
    { int xs[8]; HIP_TRY(hipMemcpy(xs, h->xstat_d, sizeof xs, hipMemcpyDeviceToHost)); for (int k = 0; k < 5; k++) st.ext[k] = xs[k]; for (int k = 0; k < 3; k++) st.p1[k] = xs[5 + k]; }
    if (objm != BSLV_LP_METHOD_PRIMAL) {      // (every iteration counts in iters[]; the primal ones, pivots and bound switches, in ext[2] as well)
        int xs[3];
        HIP_TRY(hipMemcpy(xs, h->xstat_d + 8, sizeof xs, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) st.objm[k] = xs[k];
    }
    if (cvals && h->obj_call_dual) st.objm[3] = st.pivots - st.ext[2];      // (the polish below, a PRIMAL batch of the same call, counts its dual steps here too)
    // ... and which of its LPs started on an artificial bound and ended OPTIMAL (bit 1 of `verified` stays through a solve): the polish
    std::vector<int> polish;
    if (objm != BSLV_LP_METHOD_PRIMAL) {
        std::vector<int> ver(B);
        HIP_TRY(hipMemcpy(ver.data(), h->ver_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++) if (h->status_h[b] == BSLV_LP_OPTIMAL && (ver[b] & 2)) polish.push_back(b);
    }
    if ((rc = devex_collect(h, h->dvx)) || (rc = devex_collect(h, h->pdv))) return rc;
    if (pdv) h->pdv_dst.assign(dst, dst + B);
    if (h->profile) {
        double ms = 0;
        for (size_t e = 0; e < nev; e++) { float t = 0; (void)hipEventElapsedTime(&t, h->evpool[e].first, h->evpool[e].second); ms += t; }
        for (auto &e : h->park.pre_ev) { float t = 0; (void)hipEventElapsedTime(&t, e.first, e.second); ms += t; }
        for (auto &e : h->per.ev) { float t = 0; (void)hipEventElapsedTime(&t, e.first, e.second); ms += t; }
        st.update_ms = ms;
    }
    for (auto &e : h->per.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    h->per.ev.clear();
    for (auto &e : h->park.pre_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    h->park.pre_ev.clear();
    st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (resolve) h->last.add(st); else static_cast<BatchStats &>(h->last) = st;
    // THE POLISH of a dual start on artificial bounds.  A variable that was put on one and never entered the basis -- a free column
    // ends with d_j = 0 wherever it stands -- is still there: an optimal point of the LP, 1e7 away on its optimal face, and everything
    // computed from such values carries 1e7 x 1e-16 x the row length (measured: row residuals of 1e-8 .. 2e-5).  Those LPs are solved
    // once more in their own slots as the PRIMAL objective batch they would have been, under the engine's own bounds: k_prep takes the
    // variables back to their natural side, beta is formed anew, and the few steps that follow (0 .. 7 measured) end in a basis of the
    // LP as given.  Their iterations and counters count with the call.
    if (!polish.empty()) {
        L.lb = bounds_back.lb; L.ub = bounds_back.ub; L.art = bounds_back.art;
        const int m = (int)polish.size(), vc = L.vcnt;
        std::vector<int> sl(m), st2(m), it2(m);
        std::vector<double> lo2((size_t)m * std::max(vc, 1)), up2((size_t)m * std::max(vc, 1)), cv2((size_t)m * ccnt);
        for (int k = 0; k < m; k++) {
            sl[k] = dst[polish[k]];
            if (vc > 0) { memcpy(&lo2[(size_t)k * vc], vlo + (size_t)polish[k] * vc, vc * sizeof(double)); memcpy(&up2[(size_t)k * vc], vup + (size_t)polish[k] * vc, vc * sizeof(double)); }
            memcpy(&cv2[(size_t)k * ccnt], cvals + (size_t)polish[k] * ccnt, ccnt * sizeof(double));
        }
        const std::vector<int> marks = h->rmark_h; const bool marks_valid = h->rmark_valid;      // (of THIS batch: the rescue reads them)
        h->call_obj_method = BSLV_LP_METHOD_PRIMAL;
        rc = solve_batch_impl(h, m, sl.data(), sl.data(), vc > 0 ? lo2.data() : nullptr, vc > 0 ? up2.data() : nullptr, cfirst, ccnt, cv2.data(), st2.data(), it2.data(), true);
        h->call_obj_method = objm;
        h->rmark_h = marks; h->rmark_valid = marks_valid;
        if (rc) return rc;
        // (a polish that does not end OPTIMAL -- the basis the dual steps reached was not primal feasible once the variables were back on
        //  their natural sides, and the primal steps did not mend it -- leaves no certified optimum in the slot: UNDEFINED, never the
        //  OPTIMAL of before and never the polish's own verdict on an LP the dual steps had found an optimum for)
        for (int k = 0; k < m; k++) { if (status) status[polish[k]] = st2[k] == BSLV_LP_OPTIMAL ? BSLV_LP_OPTIMAL : BSLV_LP_UNDEFINED; if (iters) iters[polish[k]] += it2[k]; }
    }
    if (L.probe & 8) {
        unsigned long long dg[16];
        HIP_TRY(hipMemcpy(dg, h->dbg_d, sizeof dg, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(h->dbg_d, 0, sizeof dg));
        const double n = (double)std::max<unsigned long long>(dg[7], 1) * 100.0;       // ticks of 10 ns -> us per selection
        fprintf(stderr, "lp select phases (LP 0, %llu selections, us each): leaving row %.1f | tableau row %.1f | row scale + candidates %.1f | Harris pass %.1f | pivot choice %.1f | column %.1f | descriptor + vector updates %.1f\n",
                dg[7], dg[0] / n, dg[1] / n, dg[2] / n, dg[3] / n, dg[4] / n, dg[5] / n, dg[6] / n);
        if (L.rev && dg[15]) fprintf(stderr, "   phase-1 pricing vector of LP 0 (revised form): %llu rebuilds, %.1f us each, %.3f ms in all\n", dg[15], dg[14] / (dg[15] * 100.0), dg[14] / 1e5);
        if (L.rev) fprintf(stderr, "   tableau row with helpers: rho + release fence %.1f | request %.1f | own slices %.1f | wait for the others %.1f | acquire fence %.1f; slices taken by the LP's own workgroup %.2f of %d\n", dg[8] / n, dg[9] / n, dg[10] / n, dg[11] / n, dg[12] / n, dg[13] * 100.0 / n, (L.ld + 2047) / 2048);
    }
    {
        static const bool tm = getenv("BSLV_LP_TIMING") != nullptr;
        if (tm) fprintf(stderr, "lp solve_batch: %s form %d x %d, B %d, %d lock-step rounds, %ld pivots, %ld passes, %.1f ms; %d parents, largest family %d, %s\n", L.rev ? "revised" : "tableau", L.M, L.N, B, it, st.pivots, st.passes, st.total_ms, h->last_init_parents, h->last_init_family, h->last_init_chunks ? "k_init_grouped" : "k_init");
        if (tm && (h->tie.on || h->tie_call.on) && !L.objmode) fprintf(stderr, "lp tie phase%s: %ld LPs entered, %ld tie pivots, %ld without an entering candidate, %ld gave up, %d rounds\n", h->tie_call.on ? " (per call)" : "", h->tie.last[0], h->tie.last[1], h->tie.last[2], h->tie.last[3], tie_rounds);
        if (tm && h->tie_call_obj.on && L.objmode) fprintf(stderr, "lp tie phase of an objective batch (per call): %ld LPs entered, %ld tie iterations, %ld on a column without a blocking row, %ld gave up, %d rounds\n", h->tie_obj.last[0], h->tie_obj.last[1], h->tie_obj.last[2], h->tie_obj.last[3], tie_rounds);
        if (tm && period > 0) fprintf(stderr, "lp period %d: %ld refactorisations at the start, %ld during the rounds, %ld replay pivots, largest age at a selection %ld, %ld replay passes, %.1f ms in refactorisations\n", period, h->last.per[0], h->last.per[1], h->last.per[2], h->last.per[3], h->per.passes, h->per.ms);
        if (tm && h->park.cap) fprintf(stderr, "lp park (totals): %ld parked, %ld unparked for a child, %ld because their source was about to be overwritten, %ld dropped unused, %zu live\n", h->park.stats[0], h->park.stats[1], h->park.stats[2], h->park.stats[3], h->park.live.size());
    }
    return 0;
}

// ---- refactorisation of the revised form: host side (the kernels: k_rfx_*, k_per_y; the sequence: replay_rebuild, replay_refresh) ----
static int ensure_rfx(bslv_lpq *h)
{
    if (h->rfx_Bcap >= h->Bcap && h->rfx_i_d) return 0;
    auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    fr(h->rfx_i_d); fr(h->rfx_c_d);
    h->rfx_Bcap = 0;
    HIP_TRY(malloc0s(&h->rfx_i_d, (size_t)h->Bcap * 3 * h->L.M * sizeof(int), h->stream));
    HIP_TRY(malloc0s(&h->rfx_c_d, (size_t)h->Bcap * 4 * sizeof(int), h->stream));
    h->rfx_Bcap = h->Bcap;
    return 0;
}
// B^-1 of the n slots (distinct, in range) rebuilt in place from their heads, in lock step; status_out[b]: 0, or BSLV_LP_UNDEFINED for a
// slot whose basis is singular or whose heads are inconsistent (it is reset to the standard basis).  ok / pivots / failed: the counters.
static int refactor_impl(bslv_lpq *h, int n, const int *slots, int *status_out, long *ok_out, long *pivots_out, long *failed_out)
{
    LpView &L = h->L;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = ensure_batch(h, n))) return rc;
    if ((rc = ensure_rfx(h))) return rc;
    const int rounds_max = replay_rounds_max(L);
    if ((rc = ensure_nwork(h, std::max(L.maxit + 64, rounds_max + 2), rounds_max + 2))) return rc;      // the work lists of the rounds and of the refresh pass behind them
    L.objmode = 0;                                  // (the engine's own cost vector: per_cost)
    for (int b = 0; b < n; b++) h->active_h[b] = b;
    HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, n * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->src_d, slots, n * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->dst_d, slots, n * sizeof(int), hipMemcpyHostToDevice, s));
    const BatchView bv = bview(h);
    // in place on the batch view, LP b = slot b of the list; every pass waits on the host and counts in no statistics
    auto pass = [&](int cnt_slot) { return flush_list(h, cnt_slot, n, false); };
    if ((rc = replay_rebuild(h, bv, h->active_d, n, pass))) return rc;
    // the reduced costs of the engine's own cost vector -> dsl, then beta
    replay_y(h, bv, bv, h->active_d, n);
    hipLaunchKernelGGL(k_rfx_price, dim3((L.ld + REV_PRICE_SLICE - 1) / REV_PRICE_SLICE, n), dim3(NT), 0, s, L, bv, rfx_view(h), n);
    hipLaunchKernelGGL(k_rev_store_d, dim3((L.ld + 255) / 256, n), dim3(256), 0, s, L, bv, n);
    if ((rc = replay_refresh(h, bv, h->active_d, n, pass))) return rc;
    hipLaunchKernelGGL(k_age_zero, dim3((n + 255) / 256), dim3(256), 0, s, (const int *)h->dst_d, n, h->age_d);      // built from the identity (a failed slot is reset below)
    std::vector<int> cnt((size_t)n * 4);
    HIP_TRY(hipMemcpy(cnt.data(), h->rfx_c_d, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; b++) {
        const bool ok = cnt[(size_t)b * 4 + 2] == RFX_RUN;
        if (status_out) status_out[b] = ok ? 0 : BSLV_LP_UNDEFINED;
        if (ok) { *ok_out += 1; *pivots_out += cnt[(size_t)b * 4 + 1]; if (h->rays_on) HIP_TRY(hipMemsetAsync(h->raykind_d + slots[b], 0, sizeof(int), s)); }
        else { *failed_out += 1; if ((rc = bslv_lpq_reset_slot(h, slots[b]))) return rc; }      // (nothing can read a half-built inverse)
    }
    return 0;
}
// solve_batch_impl, and with bslv_lpq_set_refactor the rescue behind it: every LP the pivot cross-check gave up has its slot refactorised
// in place (the slot's heads, statuses and values are current: they follow every committed pivot; what is pending for its matrix is
// dropped) and is solved again in place with its own bounds and costs by the ordinary batch path, at most RESCUE_MAX times per call.
constexpr int RESCUE_MAX = 3;
static int solve_batch_rescue(bslv_lpq *h, int B, const int *src, const int *dst, const double *vlo, const double *vup,
                              int cfirst, int ccnt, const double *cvals, int *status, int *iters)
{
    if (h) {
        LpView &L = h->L;
        for (int k = 0; k < 4; k++) h->last.rfx[k] = 0;
        for (int k = 0; k < 4; k++) h->last.per[k] = 0;      // (solve_batch_impl adds to them: the rescue's solves count with the call)
        for (DevexNorms *r : {&h->dvx, &h->pdv}) { r->B = 0; for (int k = 0; k < 3; k++) r->last[k] = 0; }
        for (int k = 0; k < 3; k++) h->last.ray[k] = 0;
        h->rmark_valid = false;
        L.rfx = (h->refactor_on && L.rev) ? 1 : 0;
        L.drift_b = -1; L.drift_p = -1;
        if (L.rev) if (const char *e = getenv("BSLV_LP_REV_DRIFT")) { int lp = -1, p = -1; if (sscanf(e, "%d:%d", &lp, &p) == 2 && lp >= 0 && p >= 1) { L.drift_b = lp; L.drift_p = p; } }
    }
    int rc = solve_batch_impl(h, B, src, dst, vlo, vup, cfirst, ccnt, cvals, status, iters, false);
    if (!h) return rc;
    LpView &L = h->L;
    L.drift_b = -1; L.drift_p = -1;             // (once per call: not again in the rescue)
    if (rc || !L.rfx || !h->rmark_valid || B <= 0) return rc;
    std::vector<int> todo;
    {
        std::vector<char> taken(h->slots, 0);
        for (int b = 0; b < B; b++) if (h->rmark_h[b]) { if (taken[dst[b]]) h->last.rfx[3]++; else { taken[dst[b]] = 1; todo.push_back(b); } }
    }
    if (todo.empty()) return 0;
    const int vc = L.vcnt;
    // Devex pricing: the norms of the batch (the re-solve runs in the LP's own slot, so the slots of the batch stand)
    SavedNorms sn(h->dvx, L.Mp1p), tn(h->pdv, L.ld);
    const std::vector<int> tn_dst = h->pdv_dst;
    if ((rc = sn.save()) || (rc = tn.save())) return rc;
    for (int attempt = 0; attempt < RESCUE_MAX && !todo.empty(); attempt++) {
        const auto t0 = std::chrono::steady_clock::now();
        const int n = (int)todo.size();
        std::vector<int> slots(n), rst(n);
        for (int k = 0; k < n; k++) slots[k] = dst[todo[k]];
        const double upd = h->last.update_ms;      // (set_profile: the replay's passes are in the call's wall clock only)
        if ((rc = refactor_impl(h, n, slots.data(), rst.data(), &h->last.rfx[0], &h->last.rfx[1], &h->last.rfx[3]))) return rc;
        h->last.update_ms = upd;
        h->last.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::vector<int> lps, sl;
        for (int k = 0; k < n; k++) if (rst[k] == 0) { lps.push_back(todo[k]); sl.push_back(slots[k]); }
        todo.clear();
        const int m = (int)lps.size();
        if (m == 0) break;
        std::vector<double> lo2((size_t)m * std::max(vc, 1)), up2((size_t)m * std::max(vc, 1)), cv2((size_t)m * std::max(ccnt, 1));
        for (int k = 0; k < m; k++) {
            if (vc > 0) { memcpy(&lo2[(size_t)k * vc], vlo + (size_t)lps[k] * vc, vc * sizeof(double)); memcpy(&up2[(size_t)k * vc], vup + (size_t)lps[k] * vc, vc * sizeof(double)); }
            if (cvals) memcpy(&cv2[(size_t)k * ccnt], cvals + (size_t)lps[k] * ccnt, ccnt * sizeof(double));
        }
        std::vector<int> st2(m), it2(m);
        h->rmark_valid = false;
        if ((rc = solve_batch_impl(h, m, sl.data(), sl.data(), vc > 0 ? lo2.data() : nullptr, vc > 0 ? up2.data() : nullptr, cfirst, ccnt, cvals ? cv2.data() : nullptr, st2.data(), it2.data(), true))) return rc;
        if ((rc = sn.take(lps, m)) || (rc = tn.take(lps, m))) return rc;
        for (int k = 0; k < m; k++) {
            const int b = lps[k];
            if (iters) iters[b] += it2[k];
            if (st2[k] != BSLV_LP_UNDEFINED) { if (status) status[b] = st2[k]; h->last.rfx[2]++; }
            else if (h->rmark_valid && h->rmark_h[k] && attempt + 1 < RESCUE_MAX) todo.push_back(b);      // (drifted again: once more)
            else h->last.rfx[3]++;                 // (k_prep refused the restart, or the cap: the LP stays UNDEFINED, as without the switch)
        }
    }
    if ((rc = sn.restore()) || (rc = tn.restore())) return rc;
    if (tn.B > 0) h->pdv_dst = tn_dst;
    return 0;
}
int bslv_lpq_refactor(bslv_lpq *h, int n, const int *slots, int *status_out)
{
    if (!h) { set_error("bslv_lpq_refactor: no engine"); return BSLV_E_ARG; }
    if (!h->L.rev) { set_error("bslv_lpq_refactor: the engine is in the tableau form, which keeps no basis inverse to rebuild"); return BSLV_E_ARG; }
    if (n < 0 || (n > 0 && !slots)) { set_error("bslv_lpq_refactor: bad argument (n = %d)", n); return BSLV_E_ARG; }
    std::vector<char> taken(h->slots, 0);
    for (int b = 0; b < n; b++) {
        if (slots[b] < 0 || slots[b] >= h->slots) { set_error("bslv_lpq_refactor: bad slot %d at %d (pool %d)", slots[b], b, h->slots); return BSLV_E_ARG; }
        if (taken[slots[b]]) { set_error("bslv_lpq_refactor: bad slot %d at %d: named twice", slots[b], b); return BSLV_E_ARG; }
        taken[slots[b]] = 1;
    }
    for (int k = 0; k < 4; k++) h->last.rfx[k] = 0;
    if (n == 0) return 0;
    return refactor_impl(h, n, slots, status_out, &h->last.rfx[0], &h->last.rfx[1], &h->last.rfx[3]);
}
int bslv_lpq_set_refactor(bslv_lpq *h, int on)
{
    if (!h) { set_error("bslv_lpq_set_refactor: no engine"); return BSLV_E_ARG; }
    if (on && !h->L.rev) { set_error("bslv_lpq_set_refactor: the engine is in the tableau form, which keeps no basis inverse to rebuild"); return BSLV_E_ARG; }
    h->refactor_on = on != 0;
    return 0;
}
int bslv_lpq_get_refactor(const bslv_lpq *h) { return h && h->refactor_on; }
int bslv_lpq_last_refactor_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->last.rfx[k];
    return 0;
}
int bslv_lpq_set_refactor_period(bslv_lpq *h, int pivots)
{
    if (!h) { set_error("bslv_lpq_set_refactor_period: no engine"); return BSLV_E_ARG; }
    if (pivots < 0) { set_error("bslv_lpq_set_refactor_period: bad argument (pivots = %d)", pivots); return BSLV_E_ARG; }
    if (pivots > 0 && !h->L.rev) { set_error("bslv_lpq_set_refactor_period: the engine is in the tableau form, which keeps no basis inverse to rebuild"); return BSLV_E_ARG; }
    h->period = pivots;
    return 0;
}
int bslv_lpq_get_refactor_period(const bslv_lpq *h) { return h ? h->period : 0; }
int bslv_lpq_slot_age(const bslv_lpq *h, int slot, long *age)
{
    if (!h || !age) { set_error("bslv_lpq_slot_age: bad argument"); return BSLV_E_ARG; }
    if (slot < 0 || slot >= h->slots) { set_error("bslv_lpq_slot_age: bad slot %d", slot); return BSLV_E_ARG; }
    *age = 0;
    if (!h->L.rev) return 0;               // (the tableau form keeps no inverse: nothing ages)
    long long a = 0;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(&a, h->age_d + slot, sizeof a, hipMemcpyDeviceToHost));
    *age = (long)a;
    return 0;
}
int bslv_lpq_last_period_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->last.per[k];
    return 0;
}
int bslv_lpq_get_inverse(bslv_lpq *h, int slot, int *heads, double *X)
{
    if (!h || !heads) { set_error("bslv_lpq_get_inverse: bad argument"); return BSLV_E_ARG; }
    if (!h->L.rev) { set_error("bslv_lpq_get_inverse: the engine is in the tableau form, which keeps no basis inverse"); return BSLV_E_ARG; }
    if (slot < 0 || slot >= h->slots) { set_error("bslv_lpq_get_inverse: bad slot %d", slot); return BSLV_E_ARG; }
    const LpView &L = h->L;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(heads, L.bh + (size_t)slot * L.M, (size_t)L.M * sizeof(int), hipMemcpyDeviceToHost));
    if (X) HIP_TRY(hipMemcpy2D(X, (size_t)L.M * sizeof(double), L.T + (size_t)slot * L.slotT, (size_t)L.ldt * sizeof(double), (size_t)L.M * sizeof(double), (size_t)L.M, hipMemcpyDeviceToHost));
    return 0;
}
int bslv_lpq_debug_perturb_inverse(bslv_lpq *h, int slot, double rel)
{
    if (!h) { set_error("bslv_lpq_debug_perturb_inverse: no engine"); return BSLV_E_ARG; }
    if (!h->L.rev) { set_error("bslv_lpq_debug_perturb_inverse: the engine is in the tableau form, which keeps no basis inverse"); return BSLV_E_ARG; }
    if (slot < 0 || slot >= h->slots) { set_error("bslv_lpq_debug_perturb_inverse: bad slot %d", slot); return BSLV_E_ARG; }
    const size_t nk = (size_t)h->L.M * h->L.M;
    hipLaunchKernelGGL(k_rfx_perturb, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, h->stream, h->L, slot, rel);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}
// test support: another basis in the heads of a slot, for bslv_lpq_refactor to build (or to refuse).  A host-side edit of the slot's
// small arrays: the matrix, the reduced costs and the basic values stay what they were and belong to the old basis.
int bslv_lpq_debug_swap_heads(bslv_lpq *h, int slot, int r, int q)
{
    if (!h) { set_error("bslv_lpq_debug_swap_heads: no engine"); return BSLV_E_ARG; }
    if (!h->L.rev) { set_error("bslv_lpq_debug_swap_heads: the engine is in the tableau form, whose heads cannot change without their tableau"); return BSLV_E_ARG; }
    const LpView &L = h->L;
    if (slot < 0 || slot >= h->slots) { set_error("bslv_lpq_debug_swap_heads: bad slot %d", slot); return BSLV_E_ARG; }
    if (r < 0 || r >= L.M || q < 0 || q >= L.N) { set_error("bslv_lpq_debug_swap_heads: row %d of %d, position %d of %d", r, L.M, q, L.N); return BSLV_E_ARG; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    int *bh = L.bh + (size_t)slot * L.M + r, *nh = L.nh + (size_t)slot * L.N + q, *pos = L.pos + (size_t)slot * (L.M + L.N);
    int leave = -1, enter = -1;
    HIP_TRY(hipMemcpy(&leave, bh, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&enter, nh, sizeof(int), hipMemcpyDeviceToHost));
    if (leave < 0 || leave >= L.M + L.N || enter < 0 || enter >= L.M + L.N) { set_error("bslv_lpq_debug_swap_heads: slot %d holds no basis", slot); return BSLV_E_ARG; }
    double lo = 0.0, up = 0.0;              // the model's own bounds (the artificial ones included): a per-LP range gets its bounds with the next solve
    HIP_TRY(hipMemcpy(&lo, h->lb_d + leave, sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&up, h->ub_d + leave, sizeof(double), hipMemcpyDeviceToHost));
    const int st = lo == up ? NS_S : (std::isinf(lo) && std::isinf(up)) ? NS_F : std::isinf(lo) ? NS_U : NS_L;
    const double x = st == NS_F ? 0.0 : (st == NS_U ? up : lo);
    const int prow = r, pnb = -1 - q;
    HIP_TRY(hipMemcpy(bh, &enter, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(nh, &leave, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pos + enter, &prow, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pos + leave, &pnb, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(L.nstat + (size_t)slot * L.N + q, &st, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(L.xN + (size_t)slot * L.ld + q, &x, sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

static int ensure_out(bslv_lpq *h, size_t n)
{
    if (n <= h->out_cap) return 0;
    if (h->out_d) (void)hipFree(h->out_d);
    h->out_d = nullptr; h->out_cap = 0;
    HIP_TRY(malloc0(&h->out_d, n * sizeof(double)));
    h->out_cap = n;
    return 0;
}

static int get_common(bslv_lpq *h, int B, const int *slot, int first, int cnt, int what, double *out)
{
    if (!h || B < 0 || cnt < 0 || !slot || !out || first < 0 || first + cnt > h->L.M + h->L.N) { set_error("bslv_lpq_get: bad argument"); return BSLV_E_ARG; }
    if (B == 0 || cnt == 0) return 0;
    for (int b = 0; b < B; b++) if (slot[b] < 0 || slot[b] >= h->slots) { set_error("bslv_lpq_get: bad slot"); return BSLV_E_ARG; }
    int rc;
    if ((rc = ensure_batch(h, B))) return rc;
    if ((rc = ensure_out(h, (size_t)B * cnt))) return rc;
    HIP_TRY(hipMemcpyAsync(h->qslot_d, slot, B * sizeof(int), hipMemcpyHostToDevice, h->stream));      // (not src_d: the batch arrays stay what the last solve left, bslv_lpq_materialise reads them)
    int n = B * cnt;
    hipLaunchKernelGGL(k_get, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->L, h->qslot_d, B, first, cnt, what, h->out_d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->out_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// values of the variables first .. first + cnt - 1 OF THE MODEL AS GIVEN.  A range without folded rows is one call into the
// engine; otherwise the folded rows are rebuilt from their columns: primal a_ij x_j; dual d_j / a_ij when the column sits on the
// bound the row gave it (the column's own reduced cost is then zero: it would be basic in the model as given), else 0.
static int get_mapped(bslv_lpq *h, int B, const int *slot, int first, int cnt, int what, double *out)
{
    if (!h) { set_error("bslv_lpq_get: bad argument"); return BSLV_E_ARG; }
    const bslv_lpq::Presolve &P = h->ps;
    if (first < 0 || cnt < 0 || first + cnt > P.M0 + P.N0) { set_error("bslv_lpq_get: bad argument"); return BSLV_E_ARG; }
    if (P.nfold == 0) return get_common(h, B, slot, first, cnt, what, out);
    if (B == 0 || cnt == 0) return 0;
    bool plain = true;
    for (int t = 0; t < cnt && plain; t++) { const int v = first + t; if (v < P.M0 && P.row_in[v] < 0) plain = false; }
    // (columns whose bound comes from a folded row need the split of their reduced cost as well)
    if (plain && what == 1) for (int t = 0; t < cnt && plain; t++) { const int v = first + t; if (v >= P.M0 && (P.lo_src[v - P.M0] >= 0 || P.up_src[v - P.M0] >= 0)) plain = false; }
    if (plain) {
        // contiguous in the engine's model too: rows keep their order, columns follow the rows that stay
        const int f2 = P.map_var(first);
        bool contiguous = true;
        for (int t = 0; t < cnt && contiguous; t++) if (P.map_var(first + t) != f2 + t) contiguous = false;
        if (contiguous) return get_common(h, B, slot, f2, cnt, what, out);
    }
    const int Mi = P.M0 - P.nfold, NV = Mi + P.N0;
    std::vector<double> prim((size_t)B * NV), dual;
    int rc;
    if ((rc = get_common(h, B, slot, 0, NV, 0, prim.data()))) return rc;
    if (what == 1) { dual.resize((size_t)B * NV); if ((rc = get_common(h, B, slot, 0, NV, 1, dual.data()))) return rc; }
    for (int b = 0; b < B; b++) {
        const double *x = &prim[(size_t)b * NV], *d = what == 1 ? &dual[(size_t)b * NV] : nullptr;
        // which bound a column sits on: the nearer one (a basic column has d = 0 and the answer does not matter)
        auto on_row_bound = [&](int j) -> int {            // folded row whose bound column j sits on, or -1
            if (!(d[Mi + j] != 0.0)) return -1;
            const double xl = std::fabs(x[Mi + j] - P.clo[j]), xu = std::fabs(x[Mi + j] - P.cup[j]);
            // (on both at once -- the folded rows left the column no room, lower bound from one source, upper from another: the
            // reduced cost belongs to the bound of its sign, d > 0 to the lower one)
            const bool at_lo = xl == xu ? d[Mi + j] > 0.0 : !(xu < xl);
            const int src = at_lo ? P.lo_src[j] : P.up_src[j];
            if (src < 0) return -1;
            // (the row's bound and the column's own may coincide: then the column keeps the reduced cost -- either split is a dual solution)
            const double own = at_lo ? P.lb0[P.M0 + j] : P.ub0[P.M0 + j], folded = at_lo ? P.clo[j] : P.cup[j];
            return own == folded ? -1 : src;
        };
        for (int t = 0; t < cnt; t++) {
            const int v = first + t;
            double val;
            if (v < P.M0 && P.row_in[v] >= 0) val = what == 0 ? x[P.row_in[v]] : d[P.row_in[v]];
            else if (v < P.M0) {
                const int j = P.fold_col[v];
                if (what == 0) val = P.fold_a[v] * x[Mi + j];
                else val = on_row_bound(j) == v ? d[Mi + j] / P.fold_a[v] : 0.0;
            } else {
                const int j = v - P.M0;
                if (what == 0) val = x[Mi + j];
                else val = on_row_bound(j) >= 0 ? 0.0 : d[Mi + j];
            }
            out[(size_t)b * cnt + t] = val;
        }
    }
    return 0;
}
int bslv_lpq_get_primal(bslv_lpq *h, int B, const int *slot, int first, int cnt, double *out) { return get_mapped(h, B, slot, first, cnt, 0, out); }
int bslv_lpq_get_dual(bslv_lpq *h, int B, const int *slot, int first, int cnt, double *out) { return get_mapped(h, B, slot, first, cnt, 1, out); }

int bslv_lpq_get_obj(bslv_lpq *h, int B, const int *slot, double *out)
{
    if (!h || B < 0 || !slot || !out) { set_error("bslv_lpq_get_obj: bad argument"); return BSLV_E_ARG; }
    if (B == 0) return 0;
    for (int b = 0; b < B; b++) if (slot[b] < 0 || slot[b] >= h->slots) { set_error("bslv_lpq_get_obj: bad slot"); return BSLV_E_ARG; }
    int rc;
    if ((rc = ensure_batch(h, B))) return rc;
    if ((rc = ensure_out(h, (size_t)B))) return rc;
    HIP_TRY(hipMemcpyAsync(h->qslot_d, slot, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_get_obj, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->L, h->qslot_d, B, h->c0, h->out_d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->out_d, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

long bslv_lpq_last_passes(const bslv_lpq *h) { return h ? h->last.passes : 0; }
long bslv_lpq_last_launches(const bslv_lpq *h) { return h ? h->last.launches : 0; }
long bslv_lpq_last_flip_updates(const bslv_lpq *h) { return h ? h->last.ext[4] : 0; }
long bslv_lpq_last_init_chunks(const bslv_lpq *h) { return h ? h->last_init_chunks : 0; }
// The extended selection for every LP of this engine from now on (on != 0) or only where a variable is boxed (0, the default
// below 1 GiB per tableau).  It changes the pivots taken, not the optimal value: used by the callers' retry when the plain
// dual simplex runs into its iteration limit on a degenerate LP.
int bslv_lpq_set_extended(bslv_lpq *h, int on)
{
    if (!h) { set_error("bslv_lpq_set_extended: bad argument"); return BSLV_E_ARG; }
    h->force_ext = on != 0;
    return 0;
}
int bslv_lpq_get_extended(const bslv_lpq *h) { return h && h->force_ext; }
// The simplex method of every later solve_batch (lp_set_options, bslv_lp.c:153-217, is where the reference chooses GLPK's): see bslv_hip.h
int bslv_lpq_set_method(bslv_lpq *h, int method)
{
    if (!h || method < BSLV_LP_METHOD_DUAL || method > BSLV_LP_METHOD_REPAIR) { set_error("bslv_lpq_set_method: bad argument (method %d)", method); return BSLV_E_ARG; }
    if (h->L.rev && method != BSLV_LP_METHOD_DUAL) { set_error("bslv_lpq_set_method: the revised form solves by the dual simplex only (method %d asked for)", method); return BSLV_E_ARG; }
    h->method = method;
    return 0;
}
int bslv_lpq_get_method(const bslv_lpq *h) { return h ? h->method : BSLV_LP_METHOD_DUAL; }
int bslv_lpq_last_phase1_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->last.p1[k];
    return 0;
}
// The pricing rule of the dual steps (select_once<.., DVX>): see bslv_hip.h
int bslv_lpq_set_pricing(bslv_lpq *h, int rule)
{
    if (!h || (rule != BSLV_LP_PRICING_DANTZIG && rule != BSLV_LP_PRICING_DEVEX)) { set_error("bslv_lpq_set_pricing: bad argument (rule %d)", rule); return BSLV_E_ARG; }
    h->pricing = rule;
    return 0;
}
int bslv_lpq_get_pricing(const bslv_lpq *h) { return h ? h->pricing : BSLV_LP_PRICING_DANTZIG; }
int bslv_lpq_last_pricing_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->dvx.last[k];
    return 0;
}
int bslv_lpq_last_pricing_norms(bslv_lpq *h, int b, double *s)
{
    if (!h || !s) { set_error("bslv_lpq_last_pricing_norms: bad argument"); return BSLV_E_ARG; }
    if (h->dvx.B <= 0 || !h->dvx.norm_d) { set_error("bslv_lpq_last_pricing_norms: the last solve call did not run under Devex pricing"); return BSLV_E_STATE; }
    if (b < 0 || b >= h->dvx.B) { set_error("bslv_lpq_last_pricing_norms: LP %d of a batch of %d", b, h->dvx.B); return BSLV_E_ARG; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(s, h->dvx.norm_d + (size_t)b * h->L.Mp1p, (size_t)h->L.M * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
// The pricing rule of the primal steps (select_once<.., PDV>): see bslv_hip.h
int bslv_lpq_set_primal_pricing(bslv_lpq *h, int rule)
{
    if (!h || (rule != BSLV_LP_PRICING_DANTZIG && rule != BSLV_LP_PRICING_DEVEX)) { set_error("bslv_lpq_set_primal_pricing: bad argument (rule %d)", rule); return BSLV_E_ARG; }
    h->ppricing = rule;
    return 0;
}
int bslv_lpq_get_primal_pricing(const bslv_lpq *h) { return h ? h->ppricing : BSLV_LP_PRICING_DANTZIG; }
int bslv_lpq_last_primal_pricing_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->pdv.last[k];
    return 0;
}
int bslv_lpq_last_primal_pricing_norms(bslv_lpq *h, int b, double *t)
{
    if (!h || !t) { set_error("bslv_lpq_last_primal_pricing_norms: bad argument"); return BSLV_E_ARG; }
    if (h->pdv.B <= 0 || !h->pdv.norm_d || (int)h->pdv_dst.size() != h->pdv.B) { set_error("bslv_lpq_last_primal_pricing_norms: the last solve call did not run under primal Devex pricing"); return BSLV_E_STATE; }
    if (b < 0 || b >= h->pdv.B) { set_error("bslv_lpq_last_primal_pricing_norms: LP %d of a batch of %d", b, h->pdv.B); return BSLV_E_ARG; }
    const LpView &L = h->L;
    HIP_TRY(hipStreamSynchronize(h->stream));
    // by position -> by variable: the heads of the LP's slot name the variable at every nonbasic position
    std::vector<double> tp(L.N); std::vector<int> nh(L.N);
    HIP_TRY(hipMemcpy(tp.data(), h->pdv.norm_d + (size_t)b * L.ld, (size_t)L.N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nh.data(), L.nh + (size_t)h->pdv_dst[b] * L.N, (size_t)L.N * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < L.M + L.N; k++) t[k] = 0.0;
    for (int j = 0; j < L.N; j++) if (nh[j] >= 0 && nh[j] < L.M + L.N) t[nh[j]] = tp[j];
    return 0;
}
// the direction of a tie phase, n values: the host copy, and the device's (at least one double; grown when n outgrows it)
static int tie_upload_dir(bslv_lpq *h, TiePhase &r, const double *dir, int n)
{
    if (!r.dir_d || (size_t)n > r.dir_cap) {
        if (r.dir_d) (void)hipFree(r.dir_d);
        r.dir_d = nullptr; r.dir_cap = 0;
        HIP_TRY(malloc0(&r.dir_d, (size_t)std::max(1, n) * sizeof(double)));
        r.dir_cap = (size_t)std::max(1, n);
    }
    r.dir.assign(dir, dir + n);
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(r.dir_d, r.dir.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
}
// The canonical optimal basis (tie phase) for every later solve_batch: see bslv_hip.h; the cut of a vertex is built from these duals (bslv_algs.c:1050)
int bslv_lpq_set_canonical(bslv_lpq *h, int on, const double *dir)
{
    if (!h || (on && !dir)) { set_error("bslv_lpq_set_canonical: bad argument"); return BSLV_E_ARG; }
    if (h->L.rev && on) { set_error("bslv_lpq_set_canonical: the revised form has no tie phase (the canonical dual is the tableau form's)"); return BSLV_E_ARG; }
    if (!on) { h->tie.on = false; return 0; }
    const int vc = h->L.vcnt;
    for (int j = 0; j < vc; j++) if (!std::isfinite(dir[j])) { set_error("bslv_lpq_set_canonical: dir[%d] is not finite", j); return BSLV_E_ARG; }
    if (const int rc = tie_upload_dir(h, h->tie, dir, vc)) return rc;
    h->tie.on = true;
    return 0;
}
int bslv_lpq_get_canonical(const bslv_lpq *h) { return h && h->tie.on; }
// ... for this call only, towards the canonical basis for `dir`: see bslv_hip.h.  The engine's own switch and direction are neither read
// nor changed (the phase runs with the call's direction, in `tie`'s per-LP state and counters); in the revised form this is the way to
// the tie phase (k_select_tie_rev), which bslv_lpq_set_canonical refuses there.
int bslv_lpq_solve_batch_canonical(bslv_lpq *h, const double *dir, int B, const int *src, const int *dst, const double *vlo,
                                   const double *vup, int *status, int *iters)
{
    if (!h || (!dir && h->L.vcnt > 0)) { set_error("bslv_lpq_solve_batch_canonical: bad argument"); return BSLV_E_ARG; }
    const int vc = h->L.vcnt;
    for (int j = 0; j < vc; j++) if (!std::isfinite(dir[j])) { set_error("bslv_lpq_solve_batch_canonical: dir[%d] is not finite", j); return BSLV_E_ARG; }
    if (vc > 0) { if (const int rc = tie_upload_dir(h, h->tie_call, dir, vc)) return rc; }
    h->call_method = h->method;
    h->tie_call.on = vc > 0;
    const int rc = solve_batch_rescue(h, B, src, dst, vlo, vup, 0, 0, nullptr, status, iters);
    h->tie_call.on = false;
    return rc;
}
int bslv_lpq_last_canonical_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->tie.last[k];
    return 0;
}
// The canonical optimal point (tie phase of objective batches) for every later solve_batch_obj: see bslv_hip.h; the dual variant's cut is built from this point (bslv_algs.c:1479-1486)
int bslv_lpq_set_canonical_obj(bslv_lpq *h, int on, int cost_first, int cost_cnt, const double *ddir)
{
    if (!h || (on && !ddir)) { set_error("bslv_lpq_set_canonical_obj: bad argument"); return BSLV_E_ARG; }
    if (!on) { h->tie_obj.on = false; return 0; }
    if (h->L.rev) { set_error("bslv_lpq_set_canonical_obj: the revised form has no tie phase for objective batches (the canonical point is the tableau form's)"); return BSLV_E_ARG; }
    if (cost_cnt < 1 || cost_first < 0 || cost_first + cost_cnt > h->ps.M0 + h->ps.N0) { set_error("bslv_lpq_set_canonical_obj: bad cost range (%d, %d)", cost_first, cost_cnt); return BSLV_E_ARG; }
    for (int j = 0; j < cost_cnt; j++) if (!std::isfinite(ddir[j])) { set_error("bslv_lpq_set_canonical_obj: ddir[%d] is not finite", j); return BSLV_E_ARG; }
    if (const int rc = tie_upload_dir(h, h->tie_obj, ddir, cost_cnt)) return rc;
    h->cobj_first = cost_first; h->cobj_cnt = cost_cnt;
    h->tie_obj.on = true;
    return 0;
}
int bslv_lpq_get_canonical_obj(const bslv_lpq *h) { return h && h->tie_obj.on; }
// ... for this call only, towards the canonical optimal point for `ddir` on the call's own cost range: see bslv_hip.h.  The engine's own
// switch, range and direction are neither read nor changed (the phase runs with the call's direction, in `tie_obj`'s per-LP state and
// counters); in the revised form this is the way to the phase (k_select_tie_obj_rev), which bslv_lpq_set_canonical_obj refuses there.
int bslv_lpq_solve_batch_obj_canonical(bslv_lpq *h, const double *ddir, int B, const int *src, const int *dst, const double *vlo,
                                       const double *vup, int cost_first, int cost_cnt, const double *costs, int *status, int *iters)
{
    if (!h || !ddir) { set_error("bslv_lpq_solve_batch_obj_canonical: bad argument"); return BSLV_E_ARG; }
    if (cost_cnt < 1 || cost_first < 0 || cost_first + cost_cnt > h->ps.M0 + h->ps.N0) { set_error("bslv_lpq_solve_batch_obj_canonical: bad cost range (%d, %d)", cost_first, cost_cnt); return BSLV_E_ARG; }
    for (int j = 0; j < cost_cnt; j++) if (!std::isfinite(ddir[j])) { set_error("bslv_lpq_solve_batch_obj_canonical: ddir[%d] is not finite", j); return BSLV_E_ARG; }
    if (const int rc = tie_upload_dir(h, h->tie_call_obj, ddir, cost_cnt)) return rc;
    h->tie_call_obj.on = true;
    const int rc = solve_batch_obj_ranged(h, B, src, dst, vlo, vup, cost_first, cost_cnt, costs, status, iters, true);
    h->tie_call_obj.on = false;
    return rc;
}
int bslv_lpq_last_canonical_obj_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->tie_obj.last[k];
    return 0;
}
// The ray store: see bslv_hip.h
int bslv_lpq_set_rays(bslv_lpq *h, int on)
{
    if (!h) { set_error("bslv_lpq_set_rays: no engine"); return BSLV_E_ARG; }
    if (!on) {
        if (h->rays_on) HIP_TRY(hipStreamSynchronize(h->stream));
        auto fr = [](void *p) { if (p) (void)hipFree(p); };
        fr(h->raykind_d); fr(h->raystat_d); fr(h->ray_d);
        h->raykind_d = nullptr; h->raystat_d = nullptr; h->ray_d = nullptr;
        h->rays_on = false;
        return 0;
    }
    if (h->rays_on) return 0;
    const LpView &L = h->L;
    if (std::max(L.M, L.N) >= RAY_IDX_MAX || KP > 15) { set_error("bslv_lpq_set_rays: %d x %d is beyond the ray record's index range", L.M, L.N); return BSLV_E_ARG; }
    HIP_TRY(malloc0(&h->raykind_d, (size_t)h->slots * sizeof(int)));
    HIP_TRY(malloc0(&h->raystat_d, 4 * sizeof(int)));
    HIP_TRY(malloc0(&h->ray_d, (size_t)h->slots * (L.M + L.N) * sizeof(double)));
    h->rays_on = true;
    return 0;
}
int bslv_lpq_get_rays(const bslv_lpq *h) { return h && h->rays_on; }
int bslv_lpq_last_ray_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->last.ray[k];
    return 0;
}
// kinds and vectors of the listed slots IN THE INDICES OF THE MODEL AS GIVEN.  Folded rows: a column entry whose needed bound (the lower
// one for z_j > 0, the upper one for z_j < 0) came from folded row i moves there, z_i = z_j / a_ij, z_j = 0 -- the rule get_mapped and
// k_cert_expand apply to duals, with the sign of the entry in the place of the side the column sits on; a DIRECTION has
// delta r_i = a_ij delta x_j on folded rows.
int bslv_lpq_get_ray(bslv_lpq *h, int B, const int *slot, int *kind, double *ray)
{
    if (!h || B < 0) { set_error("bslv_lpq_get_ray: bad argument"); return BSLV_E_ARG; }
    if (!h->rays_on) { set_error("bslv_lpq_get_ray: the ray store is off (bslv_lpq_set_rays)"); return BSLV_E_STATE; }
    if (B == 0) return 0;
    if (!slot || !kind) { set_error("bslv_lpq_get_ray: bad argument"); return BSLV_E_ARG; }
    for (int b = 0; b < B; b++) if (slot[b] < 0 || slot[b] >= h->slots) { set_error("bslv_lpq_get_ray: bad slot %d at %d (pool %d)", slot[b], b, h->slots); return BSLV_E_ARG; }
    const bslv_lpq::Presolve &P = h->ps;
    const int NE = h->L.M + h->L.N, NG = P.M0 + P.N0, Mi = h->L.M, M0 = P.M0;
    int rc;
    if ((rc = ensure_batch(h, B))) return rc;
    const size_t nd = (size_t)B * NE;
    if ((rc = ensure_out(h, nd + (size_t)(B + 1) / 2))) return rc;      // (the kinds behind the vectors)
    int *kind_d = reinterpret_cast<int *>(h->out_d + nd);
    hipStream_t s = h->stream;
    HIP_TRY(hipMemcpyAsync(h->qslot_d, slot, B * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ray_get, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, RayView{h->raykind_d, h->ray_d, h->raystat_d}, (const int *)h->qslot_d, B, NE, kind_d, ray ? h->out_d : (double *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(kind, kind_d, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    std::vector<double> ze;
    double *dstp = ray;
    if (ray && P.nfold) { ze.resize(nd); dstp = ze.data(); }
    if (ray) HIP_TRY(hipMemcpyAsync(dstp, h->out_d, nd * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!ray || !P.nfold) return 0;
    for (int b = 0; b < B; b++) {
        const double *e = &ze[(size_t)b * NE];
        double *g = ray + (size_t)b * NG;
        for (int i = 0; i < M0; i++) g[i] = P.row_in[i] >= 0 ? e[P.row_in[i]] : 0.0;
        for (int j = 0; j < P.N0; j++) g[M0 + j] = e[Mi + j];
        if (kind[b] == BSLV_LP_RAY_DIRECTION) { for (int i = 0; i < M0; i++) if (P.row_in[i] < 0) g[i] = P.fold_a[i] * e[Mi + P.fold_col[i]]; continue; }
        if (kind[b] != BSLV_LP_RAY_FARKAS) continue;
        for (int j = 0; j < P.N0; j++) {
            const double zj = e[Mi + j];
            if (!(zj != 0.0)) continue;
            const bool at_lo = zj > 0.0;
            const int src = at_lo ? P.lo_src[j] : P.up_src[j];
            if (src < 0) continue;
            const double own = at_lo ? P.lb0[M0 + j] : P.ub0[M0 + j], folded = at_lo ? P.clo[j] : P.cup[j];
            if (own == folded) continue;      // (the column's own bound says the same: the entry stays, as a dual does)
            g[src] = zj / P.fold_a[src]; g[M0 + j] = 0.0;
        }
    }
    return 0;
}
int bslv_lpq_last_ext_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->last.ext[k];
    return 0;
}
int bslv_lpq_last_stats(const bslv_lpq *h, int *lockstep_iters, long *pivots, double *update_ms, double *total_ms)
{
    if (!h) return BSLV_E_ARG;
    if (lockstep_iters) *lockstep_iters = h->last.iters;
    if (pivots) *pivots = h->last.pivots;
    if (update_ms) *update_ms = h->last.update_ms;
    if (total_ms) *total_ms = h->last.total_ms;
    return 0;
}

}  // extern "C"

#include "lp_certify.inc"
#include "lp_basis.inc"
