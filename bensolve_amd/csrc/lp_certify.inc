// lp_certify.inc -- optimality certificate of solved slots on the device (bslv_lpq_certify); included at the end of lp_engine.hip.
// The LP twin of poly_check.inc: read-only, off unless asked for.  From the model and the vectors the getters would return it
// computes, per LP, the five residuals tests/lp_cases.py: certify defines (rows, feas, dj, side, gap; see bslv_hip.h).  Kernels:
//   k_cert_gather    p and y of every listed LP in the engine's own indices, read through `pos` exactly as k_get does
//   k_cert_expand    ... in the indices of the model AS GIVEN, by the rule of get_mapped (engines with folded rows only)
//   k_cert_rowcost   the costs an objective batch puts on rows, as a vector over the engine's rows
//   k_cert_dense     A X or A' Lambda of a GROUP of CERT_G LPs from the dense image Tstd (tableau form): a workgroup stages a tile of
//                    CERT_TK x CERT_TO elements of A in LDS ONCE and every lane carries the accumulators of CERT_LPT LPs of the group
//   k_cert_sparse    the same from the CSR / CSC of the revised form: CERT_SR rows per workgroup, the CERT_G lanes of a row stage
//                    CERT_G non-zeros at a time in LDS -- every word of A is read from memory once per group, by one lane
//   k_cert_final     one workgroup per LP: the residuals of the products, feas, side, P, D, the gap, max and argmax per kind (ties to
//                    the smaller variable), the verdict
// COMPENSATED ARITHMETIC.  Every sum -- the products, P and D -- is Ogita-Rump-Oishi's Dot2: TwoProd through an explicit fma, TwoSum,
// the errors collected in a second word.  The result is as accurate as if formed in twice the working precision and rounded once: a
// residual of 1e-12 on terms of size 1e2 over 37 000 columns means nothing in plain double.  This rests on the build: -ffp-contract=off
// and no fast-math (Makefile), so that no TwoSum is simplified away and no product is contracted behind our back.  Keep it that way.
// No f64 MFMA: profiles/r02_f64_pipes.json found no gain, and MFMA cannot carry the compensation.
// DETERMINISTIC.  Every sum has one owner lane and a fixed order, every reduction a fixed tree in LDS; no floating-point atomics.  The
// same call on the same state returns the same bits.
// Folded rows (single non-zero rows the presolve turned into column bounds) are handled elementwise in k_cert_final, outside the products.
namespace bslv {

constexpr int CERT_G = 16;                        // LPs of a group: they share every tile of A
constexpr int CERT_TO = 64;                       // dense: outputs (rows of A X, columns of A' Lambda) per workgroup
constexpr int CERT_TK = 32;                       // dense: terms of the sums per staged tile
constexpr int CERT_LPT = CERT_G * CERT_TO / NT;   // dense: LPs per lane (4: 8 accumulator doubles, no pressure on occupancy)
constexpr int CERT_SR = NT / CERT_G;              // sparse: rows (CSR) or columns (CSC) per workgroup
static_assert(CERT_LPT * NT == CERT_G * CERT_TO && CERT_SR * CERT_G == NT, "certificate tiles");
static_assert((CERT_TK * CERT_TO) % NT == 0 && (CERT_G * CERT_TK) % NT == 0, "certificate tile loads");

// error-free transformations (Knuth's TwoSum, TwoProd by fma)
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) { s = a + b; const double bb = s - a; e = (a - (s - bb)) + (b - bb); }
__device__ __forceinline__ void dd_add(double &s, double &c, double x) { double t, e; two_sum(s, x, t, e); s = t; c += e; }
__device__ __forceinline__ void dd_mad(double &s, double &c, double a, double b)
{
    const double p = a * b, e = fma(a, b, -p);
    double t, err;
    two_sum(s, p, t, err);
    s = t; c += e + err;
}
__device__ __forceinline__ void dd_join(double &s, double &c, double s2, double c2) { double t, e; two_sum(s, s2, t, e); s = t; c += c2 + e; }

__global__ void k_cert_gather(LpView L, const int *slots, int B, double *pe, double *ye)
{
    const size_t n = (size_t)B * (L.M + L.N), idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int b = (int)(idx / (L.M + L.N)), k = (int)(idx % (L.M + L.N));
    const int slot = slots[b];
    const int p = L.pos[(size_t)slot * (L.M + L.N) + k];            // (as k_get)
    pe[idx] = p >= 0 ? L.beta[(size_t)slot * L.Mp1p + p] : L.xN[(size_t)slot * L.ld + (-1 - p)];
    ye[idx] = p >= 0 ? 0.0 : (L.rev ? L.dsl[(size_t)slot * L.ld + (-1 - p)] : L.T[(size_t)slot * L.slotT + (size_t)L.M * L.ld + (-1 - p)]);
}

// the model as given beside the engine's own (Presolve, on the device)
struct CertFold {
    int M0, N0, Mi;
    const int *row_in, *fold_col, *lo_src, *up_src;     // null without folded rows
    const double *fold_a, *clo, *cup;
    const int *fptr, *frow;                             // per column: its folded rows, ascending
    const double *lb0, *ub0;                            // bounds as given (M0 + N0)
};
// get_mapped's on_row_bound: the folded row whose bound column j sits on, or -1
__device__ __forceinline__ int cert_on_row_bound(const CertFold &F, const double *x, const double *d, int j)
{
    const int Mi = F.Mi;
    if (!(d[Mi + j] != 0.0)) return -1;
    const double xl = fabs(x[Mi + j] - F.clo[j]), xu = fabs(x[Mi + j] - F.cup[j]);
    const bool at_lo = xl == xu ? d[Mi + j] > 0.0 : !(xu < xl);
    const int src = at_lo ? F.lo_src[j] : F.up_src[j];
    if (src < 0) return -1;
    const double own = at_lo ? F.lb0[F.M0 + j] : F.ub0[F.M0 + j], folded = at_lo ? F.clo[j] : F.cup[j];
    return own == folded ? -1 : src;
}
__global__ void k_cert_expand(CertFold F, int B, const double *pe, const double *ye, double *pg, double *yg)
{
    const int NG = F.M0 + F.N0, NE = F.Mi + F.N0;
    const size_t n = (size_t)B * NG, idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int b = (int)(idx / NG), v = (int)(idx % NG);
    const double *x = pe + (size_t)b * NE, *d = ye + (size_t)b * NE;
    double pv, yv;
    if (v < F.M0 && F.row_in[v] >= 0) { pv = x[F.row_in[v]]; yv = d[F.row_in[v]]; }
    else if (v < F.M0) {
        const int j = F.fold_col[v];
        pv = F.fold_a[v] * x[F.Mi + j];
        yv = cert_on_row_bound(F, x, d, j) == v ? d[F.Mi + j] / F.fold_a[v] : 0.0;
    } else {
        const int j = v - F.M0;
        pv = x[F.Mi + j];
        yv = cert_on_row_bound(F, x, d, j) >= 0 ? 0.0 : d[F.Mi + j];
    }
    pg[idx] = pv; yg[idx] = yv;
}
// costs of an objective batch that lie on rows: crow[b][i] over the engine's rows (the range holds no folded row)
__global__ void k_cert_rowcost(int B, int Mi, int cfirst_e, int ccnt, const double *costs, double *crow)
{
    const size_t n = (size_t)B * Mi, idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int b = (int)(idx / Mi), i = (int)(idx % Mi), t = i - cfirst_e;
    crow[idx] = (t >= 0 && t < ccnt) ? costs[(size_t)b * ccnt + t] : 0.0;
}

// out[b][o] = sum_k a(o, k) v[b][k] as a pair (hi, lo), a(o, k) = A[o][k] (TRANS = false: A X) or A[k][o] (TRANS = true: A' Lambda).
// grid (ceil(nout / CERT_TO), ceil(B / CERT_G)).  Lane t owns output o0 + t % CERT_TO of the LPs (t / CERT_TO) * CERT_LPT + 0 .. CERT_LPT-1 of
// the group and adds its terms in ascending k.  The tile is stored as a_s[k][o], CERT_TO + 1 doubles per line: the lanes of a wave read
// 64 consecutive doubles of one line (no bank conflict), v_s is a broadcast.
template <bool TRANS>
__global__ __launch_bounds__(NT) void k_cert_dense(const double *__restrict__ A, int ld, int nout, int nred, const double *__restrict__ v, size_t vstride, int B,
                                                   double *__restrict__ hi, double *__restrict__ lo, size_t ostride)
{
    __shared__ double a_s[CERT_TK][CERT_TO + 1];
    __shared__ double v_s[CERT_G][CERT_TK];
    const int t = threadIdx.x, o0 = blockIdx.x * CERT_TO, b0 = blockIdx.y * CERT_G;
    const int ol = t % CERT_TO, q = t / CERT_TO;
    double s[CERT_LPT], c[CERT_LPT];
#pragma unroll
    for (int u = 0; u < CERT_LPT; u++) { s[u] = 0.0; c[u] = 0.0; }
    for (int k0 = 0; k0 < nred; k0 += CERT_TK) {
#pragma unroll
        for (int e = t; e < CERT_TK * CERT_TO; e += NT) {
            const int kk = TRANS ? e / CERT_TO : e % CERT_TK, oo = TRANS ? e % CERT_TO : e / CERT_TK;      // (the fast index is the one that is contiguous in memory)
            const int o = o0 + oo, k = k0 + kk;
            double a = 0.0;
            if (o < nout && k < nred) a = TRANS ? A[(size_t)k * ld + o] : A[(size_t)o * ld + k];
            a_s[kk][oo] = a;
        }
#pragma unroll
        for (int e = t; e < CERT_G * CERT_TK; e += NT) {
            const int kk = e % CERT_TK, bb = e / CERT_TK;
            const int b = b0 + bb, k = k0 + kk;
            v_s[bb][kk] = (b < B && k < nred) ? v[(size_t)b * vstride + k] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < CERT_TK; kk++) {
            const double a = a_s[kk][ol];
#pragma unroll
            for (int u = 0; u < CERT_LPT; u++) dd_mad(s[u], c[u], a, v_s[q * CERT_LPT + u][kk]);
        }
        __syncthreads();
    }
    const int o = o0 + ol;
    if (o < nout) {
#pragma unroll
        for (int u = 0; u < CERT_LPT; u++) {
            const int b = b0 + q * CERT_LPT + u;
            if (b < B) { hi[(size_t)b * ostride + o] = s[u]; lo[(size_t)b * ostride + o] = c[u]; }
        }
    }
}
// the same from a compressed matrix: out[b][o] = sum over the entries u of line o of val[u] v[b][idx[u]] (CSR: A X, CSC: A' Lambda).
// grid (ceil(nout / CERT_SR), ceil(B / CERT_G)).  Lane t owns line o0 + t / CERT_G of LP t % CERT_G of the group.  The CERT_G lanes of a
// line stage CERT_G of its entries at a time; the number of stages is the longest line's, the same for the whole workgroup.
__global__ __launch_bounds__(NT) void k_cert_sparse(const int *__restrict__ ptr, const int *__restrict__ idx, const double *__restrict__ val, int nout,
                                                    const double *__restrict__ v, size_t vstride, int B, double *__restrict__ hi, double *__restrict__ lo, size_t ostride)
{
    __shared__ double val_s[CERT_SR][CERT_G];
    __shared__ int idx_s[CERT_SR][CERT_G];
    __shared__ int len_s[CERT_SR];
    const int t = threadIdx.x, bl = t % CERT_G, ol = t / CERT_G;
    const int o = blockIdx.x * CERT_SR + ol, b = blockIdx.y * CERT_G + bl;
    const int u0 = o < nout ? ptr[o] : 0, u1 = o < nout ? ptr[o + 1] : 0, len = u1 - u0;
    if (bl == 0) len_s[ol] = len;
    __syncthreads();
    int maxlen = 0;
#pragma unroll
    for (int r = 0; r < CERT_SR; r++) maxlen = max(maxlen, len_s[r]);
    const double *vb = v + (size_t)min(b, B - 1) * vstride;          // (a lane beyond the batch reads the last LP's and writes nothing)
    double s = 0.0, c = 0.0;
    for (int c0 = 0; c0 < maxlen; c0 += CERT_G) {
        const int u = u0 + c0 + bl;
        val_s[ol][bl] = (c0 + bl < len) ? val[u] : 0.0;
        idx_s[ol][bl] = (c0 + bl < len) ? idx[u] : 0;
        __syncthreads();
        const int n = min(CERT_G, len - c0);
        for (int e = 0; e < n; e++) dd_mad(s, c, val_s[ol][e], vb[idx_s[ol][e]]);
        __syncthreads();
    }
    if (o < nout && b < B) { hi[(size_t)b * ostride + o] = s; lo[(size_t)b * ostride + o] = c; }
}

struct CertView {
    CertFold F;
    int vfirst0, vcnt;                  // the per-LP range in the indices of the model as given
    const double *vlo, *vup;            // [B][vcnt]
    const double *cost;                 // N0 + 1, the engine's own
    int cfirst0, ccnt, rowcost;         // an objective batch's range (as given); rowcost: it holds rows (g = A' crow is there)
    const double *costs;                // [B][ccnt]
    const double *crow;                 // [B][Mi]
    const double *pg, *yg;              // [B][M0 + N0] as given
    const double *pe;                   // [B][Mi + N0] the engine's
    const double *ax_hi, *ax_lo;        // [B][Mi]
    const double *aty_hi, *aty_lo;      // [B][N0]
    const double *g_hi, *g_lo;          // [B][N0]
    double tol[6], c0;
    const int *slots;
    double *res; int *at, *verdict;
};
__device__ __forceinline__ ValIdx cert_block_argmax(ValIdx x, ValIdx *sh)
{
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) { if (t < off) sh[t] = better_max(sh[t], sh[t + off]); __syncthreads(); }
    const ValIdx r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ void cert_block_sum(double &s, double &c, double *sh, double *sl)
{
    const int t = threadIdx.x;
    sh[t] = s; sl[t] = c;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) { double a = sh[t], e = sl[t]; dd_join(a, e, sh[t + off], sl[t + off]); sh[t] = a; sl[t] = e; }
        __syncthreads();
    }
    s = sh[0]; c = sl[0];
    __syncthreads();
}
// (lo - p) / (1 + |lo|) resp. (p - up) / (1 + |up|), numerator and denominator exact as pairs, the quotient rounded once
__device__ __forceinline__ double cert_excess(double a, double b, double bnd)
{
    double nh, nl, dh, dl;
    two_sum(a, -b, nh, nl);
    two_sum(1.0, fabs(bnd), dh, dl);
    const double q0 = nh / dh;
    const double r = fma(-q0, dh, nh) + (nl - q0 * dl);
    return q0 + r / dh;
}
__global__ __launch_bounds__(NT) void k_cert_final(LpView L, CertView C)
{
    __shared__ ValIdx vi_s[NT];
    __shared__ double sh_s[NT], sl_s[NT];
    const CertFold &F = C.F;
    const int b = blockIdx.x, t = threadIdx.x;
    const int M0 = F.M0, N0 = F.N0, Mi = F.Mi, NG = M0 + N0;
    const double *p = C.pg + (size_t)b * NG, *y = C.yg + (size_t)b * NG;
    const double *xe = C.pe + (size_t)b * (Mi + N0) + Mi;
    ValIdx rows{-1.0, -1}, feas{-INFINITY, -1}, dj{-1.0, -1}, side{-1.0, -1};
    double Ds = 0.0, Dc = 0.0, Ps = 0.0, Pc = 0.0;
    for (int k = t; k < NG; k += NT) {
        const int jv = k - C.vfirst0;
        const bool per_lp = jv >= 0 && jv < C.vcnt;
        const double lo = per_lp ? C.vlo[(size_t)b * C.vcnt + jv] : F.lb0[k], up = per_lp ? C.vup[(size_t)b * C.vcnt + jv] : F.ub0[k];
        const double pk = p[k], yk = y[k];
        if (k < M0) {                       // rows: r - A x
            const int i = F.row_in ? F.row_in[k] : k;
            double val;
            if (i >= 0) {
                double s, e;
                two_sum(pk, -C.ax_hi[(size_t)b * Mi + i], s, e);
                val = fabs(s + (e - C.ax_lo[(size_t)b * Mi + i]));
            } else {                        // folded: r - a x_j, the product exact
                const double a = F.fold_a[k], x = xe[F.fold_col[k]], h = a * x, e = fma(a, x, -h);
                val = fabs((pk - h) - e);
            }
            rows = better_max(rows, ValIdx{val, k});
        } else {                            // dj: d - (c - A' lambda), and the column's term of P
            const int j = k - M0, tc = k - C.cfirst0;
            const double cj = C.ccnt > 0 ? ((tc >= 0 && tc < C.ccnt) ? C.costs[(size_t)b * C.ccnt + tc] : 0.0) : C.cost[j + 1];
            double s = 0.0, c = 0.0;
            dd_add(s, c, yk);
            dd_add(s, c, -cj);
            dd_add(s, c, C.aty_hi[(size_t)b * N0 + j]);
            c += C.aty_lo[(size_t)b * N0 + j];
            dd_mad(Ps, Pc, cj, pk);
            if (C.rowcost) {                // c'_j = c_j + (A' crow)_j, lp_cases.fold's column cost
                const double gh = C.g_hi[(size_t)b * N0 + j], gl = C.g_lo[(size_t)b * N0 + j];
                dd_add(s, c, -gh);
                c -= gl;
                dd_mad(Ps, Pc, gh, pk);
                Pc += gl * pk;
            }
            if (F.fptr) for (int u = F.fptr[j]; u < F.fptr[j + 1]; u++) dd_mad(s, c, F.fold_a[F.frow[u]], y[F.frow[u]]);
            dj = better_max(dj, ValIdx{fabs(s + c), k});
        }
        if (isfinite(lo)) feas = better_max(feas, ValIdx{cert_excess(lo, pk, lo), k});
        if (isfinite(up)) feas = better_max(feas, ValIdx{cert_excess(pk, up, up), k});
        const double bnd = yk > 0.0 ? lo : up;
        if (fabs(yk) > C.tol[5]) side = better_max(side, ValIdx{isfinite(bnd) ? fabs(pk - bnd) : INFINITY, k});
        if (isfinite(bnd)) dd_mad(Ds, Dc, yk, bnd);
    }
    rows = cert_block_argmax(rows, vi_s);
    feas = cert_block_argmax(feas, vi_s);
    dj = cert_block_argmax(dj, vi_s);
    side = cert_block_argmax(side, vi_s);
    cert_block_sum(Ds, Dc, sh_s, sl_s);
    cert_block_sum(Ps, Pc, sh_s, sl_s);
    if (t) return;
    dd_add(Ds, Dc, C.c0);
    dd_add(Ps, Pc, C.c0);
    const double z = L.beta[(size_t)C.slots[b] * L.Mp1p + L.M] + C.c0;       // (k_get_obj's)
    double s, e;
    two_sum(Ds, -Ps, s, e);
    const double g1 = fabs(s + (e + (Dc - Pc)));
    two_sum(Ps, -z, s, e);
    const double g2 = fabs(s + (e + Pc));
    double r[5] = {rows.i < 0 ? 0.0 : rows.v, feas.i < 0 ? 0.0 : fmax(feas.v, 0.0), dj.i < 0 ? 0.0 : dj.v, side.i < 0 ? 0.0 : side.v, fmax(g1, g2)};
    if (g1 != g1 || g2 != g2) r[4] = NAN;
    const int a[5] = {rows.i, feas.i, dj.i, side.i, -1};
    int verdict = 0;
    for (int k = 0; k < 5; k++) {
        const double tol = k == 4 ? C.tol[4] * (1.0 + fabs(z)) : C.tol[k];
        if (!(r[k] <= tol)) verdict |= 1 << k;
        C.res[(size_t)b * 5 + k] = r[k];
        C.at[(size_t)b * 5 + k] = a[k];
    }
    C.verdict[b] = verdict;
}

// ---- bslv_lpq_certify_rays: the residuals of the stored rays (see bslv_hip.h), from the vectors bslv_lpq_get_ray returns (the model as
// given).  The products are k_cert_dense / k_cert_sparse's, over the FARKAS LPs of the call (A' z) and over its DIRECTION LPs (A delta x),
// each kind compacted: pidx[b] is the place of LP b among the LPs of its kind.  k_cert_ray_final: one workgroup per LP, as k_cert_final.
struct RayCertView {
    CertFold F;
    int vfirst0, vcnt;
    const double *vlo, *vup;
    const double *cost;                 // N0 + 1, the engine's own
    int cfirst0, ccnt;
    const double *costs;                // [B][ccnt]
    const double *zg;                   // [B][M0 + N0] as given
    const int *kind, *pidx;
    const double *f_hi, *f_lo;          // [nF][N0]  sum over the engine's rows of a_ij z_i
    const double *d_hi, *d_lo;          // [nD][Mi]  sum_j a_ij delta x_j
    double tol[4];
    double *res; int *at, *verdict;
};
__global__ __launch_bounds__(NT) void k_cert_ray_final(RayCertView C)
{
    __shared__ ValIdx vi_s[NT];
    __shared__ double sh_s[NT], sl_s[NT];
    const CertFold &F = C.F;
    const int b = blockIdx.x, t = threadIdx.x;
    const int M0 = F.M0, N0 = F.N0, Mi = F.Mi, NG = M0 + N0;
    const int kind = C.kind[b];
    if (kind == BSLV_LP_RAY_NONE) {
        if (t == 0) { for (int k = 0; k < 4; k++) { C.res[(size_t)b * 4 + k] = NAN; C.at[(size_t)b * 4 + k] = -1; } C.verdict[b] = 15; }
        return;
    }
    const bool farkas = kind == BSLV_LP_RAY_FARKAS;
    const double *z = C.zg + (size_t)b * NG;
    const size_t p = (size_t)C.pidx[b];
    ValIdx r0{-1.0, -1}, r1{0.0, -1}, nan{0.0, -1};
    double Ss = 0.0, Sc = 0.0, As = 0.0, Ac = 0.0;
    // (one loop per kind, chosen outside: the two share no load but z, lo and up)
    if (farkas) {
        for (int k = t; k < NG; k += NT) {
            const int jv = k - C.vfirst0;
            const bool per_lp = jv >= 0 && jv < C.vcnt;
            const double lo = per_lp ? C.vlo[(size_t)b * C.vcnt + jv] : F.lb0[k], up = per_lp ? C.vup[(size_t)b * C.vcnt + jv] : F.ub0[k];
            const double zk = z[k];
            if (zk != zk) nan = ValIdx{1.0, k};
            if (k >= M0) {                  // ident: z_{M+j} + sum_i a_ij z_i, the folded rows' terms elementwise
                const int j = k - M0;
                double s = 0.0, c = 0.0;
                dd_add(s, c, zk);
                dd_add(s, c, C.f_hi[p * N0 + j]);
                c += C.f_lo[p * N0 + j];
                if (F.fptr) for (int u = F.fptr[j]; u < F.fptr[j + 1]; u++) dd_mad(s, c, F.fold_a[F.frow[u]], z[F.frow[u]]);
                r0 = better_max(r0, ValIdx{fabs(s + c), k});
            }
            if (fabs(zk) > C.tol[2]) {
                const double bnd = zk > 0.0 ? lo : up;
                if (isfinite(bnd)) { dd_mad(Ss, Sc, zk, bnd); dd_mad(As, Ac, fabs(zk), fabs(bnd)); }
                else r1 = better_max(r1, ValIdx{fabs(zk), k});
            }
        }
    } else {
        for (int k = t; k < NG; k += NT) {
            const int jv = k - C.vfirst0;
            const bool per_lp = jv >= 0 && jv < C.vcnt;
            const double lo = per_lp ? C.vlo[(size_t)b * C.vcnt + jv] : F.lb0[k], up = per_lp ? C.vup[(size_t)b * C.vcnt + jv] : F.ub0[k];
            const double zk = z[k];
            if (zk != zk) nan = ValIdx{1.0, k};
            if (k < M0) {                   // rows: delta r - A delta x
                const int i = F.row_in ? F.row_in[k] : k;
                double val;
                if (i >= 0) {
                    double s, e;
                    two_sum(zk, -C.d_hi[p * Mi + i], s, e);
                    val = fabs(s + (e - C.d_lo[p * Mi + i]));
                } else {                    // folded: delta r - a delta x_j, the product exact
                    const double a = F.fold_a[k], x = z[M0 + F.fold_col[k]], h = a * x, e = fma(a, x, -h);
                    val = fabs((zk - h) - e);
                }
                r0 = better_max(r0, ValIdx{val, k});
            }
            if (isfinite(lo)) r1 = better_max(r1, ValIdx{-zk, k});
            if (isfinite(up)) r1 = better_max(r1, ValIdx{zk, k});
            const int tc = k - C.cfirst0;
            const double ck = C.ccnt > 0 ? ((tc >= 0 && tc < C.ccnt) ? C.costs[(size_t)b * C.ccnt + tc] : 0.0) : (k >= M0 ? C.cost[k - M0 + 1] : 0.0);
            dd_mad(Ss, Sc, -ck, zk);
            dd_mad(As, Ac, fabs(ck), fabs(zk));
        }
    }
    r0 = cert_block_argmax(r0, vi_s);
    r1 = cert_block_argmax(r1, vi_s);
    nan = cert_block_argmax(nan, vi_s);
    cert_block_sum(Ss, Sc, sh_s, sl_s);
    cert_block_sum(As, Ac, sh_s, sl_s);
    if (t) return;
    double r[4] = {r0.i < 0 ? 0.0 : r0.v, r1.v > 0.0 ? r1.v : 0.0, Ss + Sc, As + Ac};      // (not below 0, and no -0)
    if (nan.v > 0.0) { r[0] = NAN; r[1] = NAN; }
    const int a[4] = {r0.i, r1.v > 0.0 ? r1.i : -1, -1, -1};
    int verdict = 0;
    if (!(r[0] <= (farkas ? C.tol[0] : C.tol[1]))) verdict |= 1;
    if (!(r[1] <= C.tol[2])) verdict |= 2;
    if (!(r[2] > C.tol[3] * (1.0 + r[3]))) verdict |= 4;
    for (int k = 0; k < 4; k++) { C.res[(size_t)b * 4 + k] = r[k]; C.at[(size_t)b * 4 + k] = a[k]; }
    C.verdict[b] = verdict;
}

}  // namespace bslv

struct CertTimer {          // BSLV_LP_CERTIFY_TIMING=1: HIP events around each kernel
    bool on; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr; float ms[5] = {0, 0, 0, 0, 0};
    CertTimer(bool o, hipStream_t st) : on(o), s(st) { if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) on = false; }
    ~CertTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    void start() { if (on) (void)hipEventRecord(e0, s); }
    void stop(int k) { if (!on) return; (void)hipEventRecord(e1, s); float t = 0; if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[k] += t; }
};

// the scratch of bslv_lpq_certify: one piece, grown to the largest call, carved per call
static int cert_ensure(bslv_lpq *h, size_t bytes)
{
    if (bytes <= h->cert_cap) return 0;
    if (h->cert_d) (void)hipFree(h->cert_d);
    h->cert_d = nullptr; h->cert_cap = 0;
    HIP_TRY(malloc0s(&h->cert_d, bytes, h->stream));
    h->cert_cap = bytes;
    return 0;
}

extern "C" {

int bslv_lpq_certify(bslv_lpq *h, int B, const int *slot, const double *vlo, const double *vup, int cost_first, int cost_cnt, const double *costs,
                     const double *tol, double *res, int *at, int *verdict)
{
    if (!h || B < 0) { set_error("bslv_lpq_certify: bad argument"); return BSLV_E_ARG; }
    const LpView &L = h->L;
    const bslv_lpq::Presolve &P = h->ps;
    const int M0 = P.M0, N0 = P.N0, Mi = L.M, NG = M0 + N0, NE = Mi + N0, vcnt = L.vcnt;
    if (cost_cnt < 0 || cost_first < 0 || cost_first + cost_cnt > NG || (cost_cnt > 0 && !costs)) { set_error("bslv_lpq_certify: bad cost range (%d, %d)", cost_first, cost_cnt); return BSLV_E_ARG; }
    if (B == 0) return 0;
    if (!slot || !res || (vcnt > 0 && (!vlo || !vup))) { set_error("bslv_lpq_certify: bad argument"); return BSLV_E_ARG; }
    for (int b = 0; b < B; b++) if (slot[b] < 0 || slot[b] >= h->slots) { set_error("bslv_lpq_certify: bad slot"); return BSLV_E_ARG; }
    if (P.nfold) for (int t = 0; t < cost_cnt; t++) if (P.map_var(cost_first + t) != P.map_var(cost_first) + t) { set_error("bslv_lpq_certify: the cost range covers rows the presolve folded into column bounds"); return BSLV_E_ARG; }
    const bool rowcost = cost_cnt > 0 && cost_first < M0;
    // the per-LP range in the indices of the model as given (no row inside it is folded)
    int vfirst0 = 0;
    if (vcnt > 0) {
        if (L.vfirst >= Mi) vfirst0 = M0 + (L.vfirst - Mi);
        else for (int i = 0; i < M0; i++) if (P.row_in[i] == L.vfirst) vfirst0 = i;
    }
    // the scratch: what every LP of the call shares, then what a chunk of LPs needs; every piece a multiple of 256 bytes
    auto al = [](size_t n) { return (n + 255) / 256 * 256; };
    std::vector<int> fptr, frow;
    if (P.nfold) {
        fptr.assign(N0 + 1, 0);
        for (int i = 0; i < M0; i++) if (P.row_in[i] < 0) fptr[P.fold_col[i] + 1]++;
        for (int j = 0; j < N0; j++) fptr[j + 1] += fptr[j];
        frow.resize(P.nfold);
        std::vector<int> fill(fptr.begin(), fptr.end() - 1);
        for (int i = 0; i < M0; i++) if (P.row_in[i] < 0) frow[fill[P.fold_col[i]]++] = i;
    }
    const size_t per_lp = 8 * ((size_t)2 * NE + (P.nfold ? 2 * NG : 0) + 2 * Mi + 2 * N0 + (rowcost ? 2 * N0 + Mi : 0) + 2 * vcnt + cost_cnt + 5) + 4 * 7;
    size_t budget = (size_t)256 << 20;      // of a chunk's scratch; a call with more LPs than fit runs in chunks
    if (const char *e = getenv("BSLV_LP_CERTIFY_SCRATCH_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    size_t Bc = std::max<size_t>(1, budget / per_lp);
    if (Bc >= (size_t)CERT_G) Bc = Bc / CERT_G * CERT_G;
    if (const char *e = getenv("BSLV_LP_CERTIFY_CHUNK")) Bc = (size_t)std::max(1, atoi(e));      // (tests: LPs per chunk)
    Bc = std::min(Bc, (size_t)B);
    size_t cur = 0;
    auto take = [&](size_t bytes) { const size_t at = cur; cur += al(std::max<size_t>(bytes, 1)); return at; };
    const size_t o_lb0 = take((size_t)NG * 8), o_ub0 = take((size_t)NG * 8), o_cost = take((size_t)(N0 + 1) * 8);
    const size_t nf = P.nfold ? 1 : 0;      // (the presolve record only where rows were folded)
    const size_t o_row_in = take(nf * M0 * 4), o_fold_col = take(nf * M0 * 4), o_fold_a = take(nf * M0 * 8), o_clo = take(nf * N0 * 8), o_cup = take(nf * N0 * 8),
                 o_lo_src = take(nf * N0 * 4), o_up_src = take(nf * N0 * 4), o_fptr = take(nf * (N0 + 1) * 4), o_frow = take(nf * P.nfold * 4);
    const size_t o_slots = take(Bc * 4), o_verdict = take(Bc * 4), o_at = take(Bc * 5 * 4), o_res = take(Bc * 5 * 8);
    const size_t o_vlo = take(Bc * 8 * vcnt), o_vup = take(Bc * 8 * vcnt), o_costs = take(Bc * 8 * cost_cnt);
    const size_t o_pe = take(Bc * 8 * NE), o_ye = take(Bc * 8 * NE), o_pg = take(nf * Bc * 8 * NG), o_yg = take(nf * Bc * 8 * NG);
    const size_t o_axh = take(Bc * 8 * Mi), o_axl = take(Bc * 8 * Mi), o_ath = take(Bc * 8 * N0), o_atl = take(Bc * 8 * N0);
    const size_t rc1 = rowcost ? 1 : 0;
    const size_t o_gh = take(rc1 * Bc * 8 * N0), o_gl = take(rc1 * Bc * 8 * N0), o_crow = take(rc1 * Bc * 8 * Mi);
    hipStream_t s = h->stream;
    int rc;
    if ((rc = cert_ensure(h, cur))) return rc;
    char *base = (char *)h->cert_d;
    CertView C{};
    CertFold &F = C.F;
    F.M0 = M0; F.N0 = N0; F.Mi = Mi;
    double *lb0_d = (double *)(base + o_lb0), *ub0_d = (double *)(base + o_ub0), *cost_d = (double *)(base + o_cost);
    HIP_TRY(hipMemcpyAsync(lb0_d, P.lb0.data(), (size_t)NG * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ub0_d, P.ub0.data(), (size_t)NG * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(cost_d, h->cost.data(), (size_t)(N0 + 1) * 8, hipMemcpyHostToDevice, s));
    F.lb0 = lb0_d; F.ub0 = ub0_d; C.cost = cost_d;
    if (P.nfold) {
        HIP_TRY(hipMemcpyAsync(base + o_row_in, P.row_in.data(), (size_t)M0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fold_col, P.fold_col.data(), (size_t)M0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fold_a, P.fold_a.data(), (size_t)M0 * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_clo, P.clo.data(), (size_t)N0 * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_cup, P.cup.data(), (size_t)N0 * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_lo_src, P.lo_src.data(), (size_t)N0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_up_src, P.up_src.data(), (size_t)N0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fptr, fptr.data(), (size_t)(N0 + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_frow, frow.data(), (size_t)P.nfold * 4, hipMemcpyHostToDevice, s));
        F.row_in = (const int *)(base + o_row_in); F.fold_col = (const int *)(base + o_fold_col); F.fold_a = (const double *)(base + o_fold_a);
        F.clo = (const double *)(base + o_clo); F.cup = (const double *)(base + o_cup); F.lo_src = (const int *)(base + o_lo_src); F.up_src = (const int *)(base + o_up_src);
        F.fptr = (const int *)(base + o_fptr); F.frow = (const int *)(base + o_frow);
    }
    int *slots_d = (int *)(base + o_slots), *verdict_d = (int *)(base + o_verdict), *at_d = (int *)(base + o_at);
    double *res_d = (double *)(base + o_res), *vlo_d = (double *)(base + o_vlo), *vup_d = (double *)(base + o_vup), *costs_d = (double *)(base + o_costs);
    double *pe_d = (double *)(base + o_pe), *ye_d = (double *)(base + o_ye);
    double *pg_d = P.nfold ? (double *)(base + o_pg) : pe_d, *yg_d = P.nfold ? (double *)(base + o_yg) : ye_d;
    double *axh_d = (double *)(base + o_axh), *axl_d = (double *)(base + o_axl), *ath_d = (double *)(base + o_ath), *atl_d = (double *)(base + o_atl);
    double *gh_d = rowcost ? (double *)(base + o_gh) : nullptr, *gl_d = rowcost ? (double *)(base + o_gl) : nullptr, *crow_d = rowcost ? (double *)(base + o_crow) : nullptr;
    const double deflt[6] = {1e-9, 1e-8, 1e-8, 1e-7, 1e-9, 1e-9};
    for (int k = 0; k < 6; k++) C.tol[k] = (tol && tol[k] > 0.0) ? tol[k] : deflt[k];
    C.c0 = h->c0;
    C.vfirst0 = vfirst0; C.vcnt = vcnt; C.vlo = vlo_d; C.vup = vup_d;
    C.cfirst0 = cost_first; C.ccnt = cost_cnt; C.rowcost = rowcost ? 1 : 0; C.costs = costs_d; C.crow = crow_d;
    C.pg = pg_d; C.yg = yg_d; C.pe = pe_d; C.ax_hi = axh_d; C.ax_lo = axl_d; C.aty_hi = ath_d; C.aty_lo = atl_d; C.g_hi = gh_d; C.g_lo = gl_d;
    C.slots = slots_d; C.res = res_d; C.at = at_d; C.verdict = verdict_d;
    const bool timing = getenv("BSLV_LP_CERTIFY_TIMING") != nullptr;
    CertTimer T(timing, s);
    long launches = 0, bad = 0;
    std::vector<int> vd(Bc);
    for (size_t b0 = 0; b0 < (size_t)B; b0 += Bc) {
        const int nb = (int)std::min(Bc, (size_t)B - b0);
        HIP_TRY(hipMemcpyAsync(slots_d, slot + b0, (size_t)nb * 4, hipMemcpyHostToDevice, s));
        if (vcnt > 0) {
            HIP_TRY(hipMemcpyAsync(vlo_d, vlo + b0 * vcnt, (size_t)nb * vcnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(vup_d, vup + b0 * vcnt, (size_t)nb * vcnt * 8, hipMemcpyHostToDevice, s));
        }
        if (cost_cnt > 0) HIP_TRY(hipMemcpyAsync(costs_d, costs + b0 * cost_cnt, (size_t)nb * cost_cnt * 8, hipMemcpyHostToDevice, s));
        const size_t ne = (size_t)nb * NE, ng = (size_t)nb * NG;
        T.start();
        hipLaunchKernelGGL(k_cert_gather, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, L, slots_d, nb, pe_d, ye_d);
        launches++;
        if (P.nfold) { hipLaunchKernelGGL(k_cert_expand, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, F, nb, pe_d, ye_d, pg_d, yg_d); launches++; }
        if (rowcost) { hipLaunchKernelGGL(k_cert_rowcost, dim3((unsigned)(((size_t)nb * Mi + 255) / 256)), dim3(256), 0, s, nb, Mi, P.map_var(cost_first), cost_cnt, costs_d, crow_d); launches++; }
        T.stop(0);
        const int groups = (nb + CERT_G - 1) / CERT_G;
        // the products: x = the columns' part of p, lambda = the rows' part of y, both in the engine's own indices
        for (int which = 0; which < (rowcost ? 3 : 2); which++) {
            const bool trans = which > 0;
            const double *v = which == 0 ? pe_d + Mi : which == 1 ? ye_d : crow_d;
            const size_t vstride = which == 2 ? (size_t)Mi : (size_t)NE;
            double *hi = which == 0 ? axh_d : which == 1 ? ath_d : gh_d, *lo = which == 0 ? axl_d : which == 1 ? atl_d : gl_d;
            const int nout = trans ? N0 : Mi;
            T.start();
            if (!L.rev) {
                const dim3 grid((nout + CERT_TO - 1) / CERT_TO, groups);
                if (trans) hipLaunchKernelGGL(k_cert_dense<true>, grid, dim3(NT), 0, s, h->Tstd, L.ld, nout, Mi, v, vstride, nb, hi, lo, (size_t)nout);
                else hipLaunchKernelGGL(k_cert_dense<false>, grid, dim3(NT), 0, s, h->Tstd, L.ld, nout, N0, v, vstride, nb, hi, lo, (size_t)nout);
            } else {
                const dim3 grid((nout + CERT_SR - 1) / CERT_SR, groups);
                if (trans) hipLaunchKernelGGL(k_cert_sparse, grid, dim3(NT), 0, s, L.cptr, L.cidx, L.cval, nout, v, vstride, nb, hi, lo, (size_t)nout);
                else hipLaunchKernelGGL(k_cert_sparse, grid, dim3(NT), 0, s, L.rptr, L.ridx, L.rval, nout, v, vstride, nb, hi, lo, (size_t)nout);
            }
            launches++;
            T.stop(which == 0 ? 1 : 2);
        }
        T.start();
        hipLaunchKernelGGL(k_cert_final, dim3(nb), dim3(NT), 0, s, L, C);
        launches++;
        T.stop(3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(res + b0 * 5, res_d, (size_t)nb * 5 * 8, hipMemcpyDeviceToHost, s));
        if (at) HIP_TRY(hipMemcpyAsync(at + b0 * 5, at_d, (size_t)nb * 5 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(vd.data(), verdict_d, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int b = 0; b < nb; b++) { bad += vd[b] != 0; if (verdict) verdict[b0 + b] = vd[b]; }
    }
    h->last_cert[0] = B; h->last_cert[1] = bad; h->last_cert[2] = launches;
    if (timing) fprintf(stderr, "bslv_lpq_certify: %d LPs (%s form, %d x %d, chunks of %zu) gather %.3f ms, A x %.3f ms, A' lambda %.3f ms, final %.3f ms; %ld launches, %ld not certified\n",
                        B, L.rev ? "revised" : "tableau", Mi, N0, Bc, T.ms[0], T.ms[1], T.ms[2], T.ms[3], launches, bad);
    return 0;
}

int bslv_lpq_last_certify_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->last_cert[k];
    return 0;
}

int bslv_lpq_certify_rays(bslv_lpq *h, int B, const int *slot, const double *vlo, const double *vup, int cost_first, int cost_cnt, const double *costs,
                          const double *tol, double *res, int *at, int *verdict)
{
    if (!h || B < 0) { set_error("bslv_lpq_certify_rays: bad argument"); return BSLV_E_ARG; }
    if (!h->rays_on) { set_error("bslv_lpq_certify_rays: the ray store is off (bslv_lpq_set_rays)"); return BSLV_E_STATE; }
    const LpView &L = h->L;
    const bslv_lpq::Presolve &P = h->ps;
    const int M0 = P.M0, N0 = P.N0, Mi = L.M, NG = M0 + N0, vcnt = L.vcnt;
    if (cost_cnt < 0 || cost_first < 0 || cost_first + cost_cnt > NG || (cost_cnt > 0 && !costs)) { set_error("bslv_lpq_certify_rays: bad cost range (%d, %d)", cost_first, cost_cnt); return BSLV_E_ARG; }
    if (B == 0) return 0;
    if (!slot || !res || (vcnt > 0 && (!vlo || !vup))) { set_error("bslv_lpq_certify_rays: bad argument"); return BSLV_E_ARG; }
    for (int b = 0; b < B; b++) if (slot[b] < 0 || slot[b] >= h->slots) { set_error("bslv_lpq_certify_rays: bad slot"); return BSLV_E_ARG; }
    int vfirst0 = 0;
    if (vcnt > 0) {
        if (L.vfirst >= Mi) vfirst0 = M0 + (L.vfirst - Mi);
        else for (int i = 0; i < M0; i++) if (P.row_in[i] == L.vfirst) vfirst0 = i;
    }
    auto al = [](size_t n) { return (n + 255) / 256 * 256; };
    std::vector<int> fptr, frow;
    if (P.nfold) {
        fptr.assign(N0 + 1, 0);
        for (int i = 0; i < M0; i++) if (P.row_in[i] < 0) fptr[P.fold_col[i] + 1]++;
        for (int j = 0; j < N0; j++) fptr[j + 1] += fptr[j];
        frow.resize(P.nfold);
        std::vector<int> fill(fptr.begin(), fptr.end() - 1);
        for (int i = 0; i < M0; i++) if (P.row_in[i] < 0) frow[fill[P.fold_col[i]]++] = i;
    }
    const int NP = std::max(Mi, N0);      // (an LP has one kind: its product's input and output fit in 3 NP)
    const size_t per_lp = 8 * ((size_t)NG + 3 * NP + 2 * vcnt + cost_cnt + 4) + 4 * 7;
    size_t budget = (size_t)256 << 20;
    if (const char *e = getenv("BSLV_LP_CERTIFY_SCRATCH_MB")) budget = (size_t)std::max(1, atoi(e)) << 20;
    size_t Bc = std::max<size_t>(1, budget / per_lp);
    if (Bc >= (size_t)CERT_G) Bc = Bc / CERT_G * CERT_G;
    if (const char *e = getenv("BSLV_LP_CERTIFY_CHUNK")) Bc = (size_t)std::max(1, atoi(e));
    Bc = std::min(Bc, (size_t)B);
    size_t cur = 0;
    auto take = [&](size_t bytes) { const size_t at = cur; cur += al(std::max<size_t>(bytes, 1)); return at; };
    const size_t o_lb0 = take((size_t)NG * 8), o_ub0 = take((size_t)NG * 8), o_cost = take((size_t)(N0 + 1) * 8);
    const size_t nf = P.nfold ? 1 : 0;
    const size_t o_row_in = take(nf * M0 * 4), o_fold_col = take(nf * M0 * 4), o_fold_a = take(nf * M0 * 8), o_fptr = take(nf * (N0 + 1) * 4), o_frow = take(nf * P.nfold * 4);
    const size_t o_kind = take(Bc * 4), o_pidx = take(Bc * 4), o_verdict = take(Bc * 4), o_at = take(Bc * 4 * 4), o_res = take(Bc * 4 * 8);
    const size_t o_vlo = take(Bc * 8 * vcnt), o_vup = take(Bc * 8 * vcnt), o_costs = take(Bc * 8 * cost_cnt);
    const size_t o_zg = take(Bc * 8 * NG), o_v = take(Bc * 8 * NP), o_hi = take(Bc * 8 * NP), o_lo = take(Bc * 8 * NP);
    hipStream_t s = h->stream;
    int rc;
    if ((rc = cert_ensure(h, cur))) return rc;
    char *base = (char *)h->cert_d;
    RayCertView C{};
    CertFold &F = C.F;
    F.M0 = M0; F.N0 = N0; F.Mi = Mi;
    HIP_TRY(hipMemcpyAsync(base + o_lb0, P.lb0.data(), (size_t)NG * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_ub0, P.ub0.data(), (size_t)NG * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_cost, h->cost.data(), (size_t)(N0 + 1) * 8, hipMemcpyHostToDevice, s));
    F.lb0 = (const double *)(base + o_lb0); F.ub0 = (const double *)(base + o_ub0); C.cost = (const double *)(base + o_cost);
    if (P.nfold) {
        HIP_TRY(hipMemcpyAsync(base + o_row_in, P.row_in.data(), (size_t)M0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fold_col, P.fold_col.data(), (size_t)M0 * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fold_a, P.fold_a.data(), (size_t)M0 * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_fptr, fptr.data(), (size_t)(N0 + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_frow, frow.data(), (size_t)P.nfold * 4, hipMemcpyHostToDevice, s));
        F.row_in = (const int *)(base + o_row_in); F.fold_col = (const int *)(base + o_fold_col); F.fold_a = (const double *)(base + o_fold_a);
        F.fptr = (const int *)(base + o_fptr); F.frow = (const int *)(base + o_frow);
    }
    int *kind_d = (int *)(base + o_kind), *pidx_d = (int *)(base + o_pidx), *verdict_d = (int *)(base + o_verdict), *at_d = (int *)(base + o_at);
    double *res_d = (double *)(base + o_res), *vlo_d = (double *)(base + o_vlo), *vup_d = (double *)(base + o_vup), *costs_d = (double *)(base + o_costs);
    double *zg_d = (double *)(base + o_zg), *v_d = (double *)(base + o_v), *hi_d = (double *)(base + o_hi), *lo_d = (double *)(base + o_lo);
    const double deflt[4] = {1e-8, 1e-9, 1e-9, 1e-9};      // (bslv_lpq_certify's dj, rows, dual-zero and gap numbers)
    for (int k = 0; k < 4; k++) C.tol[k] = (tol && tol[k] > 0.0) ? tol[k] : deflt[k];
    C.vfirst0 = vfirst0; C.vcnt = vcnt; C.vlo = vlo_d; C.vup = vup_d;
    C.cfirst0 = cost_first; C.ccnt = cost_cnt; C.costs = costs_d;
    C.zg = zg_d; C.kind = kind_d; C.pidx = pidx_d;
    C.res = res_d; C.at = at_d; C.verdict = verdict_d;
    const bool timing = getenv("BSLV_LP_CERTIFY_TIMING") != nullptr;
    CertTimer T(timing, s);
    long launches = 0, bad = 0;
    std::vector<int> vd(Bc), kd(Bc), px(Bc);
    std::vector<double> zg(Bc * NG), v(Bc * NP);
    for (size_t b0 = 0; b0 < (size_t)B; b0 += Bc) {
        const int nb = (int)std::min(Bc, (size_t)B - b0);
        if ((rc = bslv_lpq_get_ray(h, nb, slot + b0, kd.data(), zg.data()))) return rc;
        // the LPs of each kind, compacted: the FARKAS ones from the front of v, the DIRECTION ones behind them
        int nF = 0, nD = 0;
        for (int b = 0; b < nb; b++) nF += kd[b] == BSLV_LP_RAY_FARKAS;
        double *vF = v.data(), *vD = v.data() + (size_t)nF * Mi;
        for (int b = 0, f = 0; b < nb; b++) {
            const double *z = &zg[(size_t)b * NG];
            px[b] = -1;
            if (kd[b] == BSLV_LP_RAY_FARKAS) { for (int i = 0; i < M0; i++) if (P.row_in[i] >= 0) vF[(size_t)f * Mi + P.row_in[i]] = z[i]; px[b] = f++; }
            else if (kd[b] == BSLV_LP_RAY_DIRECTION) { memcpy(vD + (size_t)nD * N0, z + M0, (size_t)N0 * 8); px[b] = nD++; }
        }
        HIP_TRY(hipMemcpyAsync(kind_d, kd.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(pidx_d, px.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(zg_d, zg.data(), (size_t)nb * NG * 8, hipMemcpyHostToDevice, s));
        if (nF + nD) HIP_TRY(hipMemcpyAsync(v_d, v.data(), ((size_t)nF * Mi + (size_t)nD * N0) * 8, hipMemcpyHostToDevice, s));
        if (vcnt > 0) {
            HIP_TRY(hipMemcpyAsync(vlo_d, vlo + b0 * vcnt, (size_t)nb * vcnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(vup_d, vup + b0 * vcnt, (size_t)nb * vcnt * 8, hipMemcpyHostToDevice, s));
        }
        if (cost_cnt > 0) HIP_TRY(hipMemcpyAsync(costs_d, costs + b0 * cost_cnt, (size_t)nb * cost_cnt * 8, hipMemcpyHostToDevice, s));
        // A' z of the FARKAS LPs, A delta x of the DIRECTION LPs (outputs side by side as the inputs are)
        double *fh = hi_d, *fl = lo_d, *dh = hi_d + (size_t)nF * N0, *dl = lo_d + (size_t)nF * N0;
        C.f_hi = fh; C.f_lo = fl; C.d_hi = dh; C.d_lo = dl;
        for (int which = 0; which < 2; which++) {
            const bool trans = which == 0;
            const int n = trans ? nF : nD;
            if (n == 0) continue;
            const int groups = (n + CERT_G - 1) / CERT_G, nout = trans ? N0 : Mi, nred = trans ? Mi : N0;
            const double *vin = trans ? v_d : v_d + (size_t)nF * Mi;
            double *hi = trans ? fh : dh, *lo = trans ? fl : dl;
            T.start();
            if (!L.rev) {
                const dim3 grid((nout + CERT_TO - 1) / CERT_TO, groups);
                if (trans) hipLaunchKernelGGL(k_cert_dense<true>, grid, dim3(NT), 0, s, h->Tstd, L.ld, nout, nred, vin, (size_t)nred, n, hi, lo, (size_t)nout);
                else hipLaunchKernelGGL(k_cert_dense<false>, grid, dim3(NT), 0, s, h->Tstd, L.ld, nout, nred, vin, (size_t)nred, n, hi, lo, (size_t)nout);
            } else {
                const dim3 grid((nout + CERT_SR - 1) / CERT_SR, groups);
                if (trans) hipLaunchKernelGGL(k_cert_sparse, grid, dim3(NT), 0, s, L.cptr, L.cidx, L.cval, nout, vin, (size_t)nred, n, hi, lo, (size_t)nout);
                else hipLaunchKernelGGL(k_cert_sparse, grid, dim3(NT), 0, s, L.rptr, L.ridx, L.rval, nout, vin, (size_t)nred, n, hi, lo, (size_t)nout);
            }
            launches++;
            T.stop(which);
        }
        T.start();
        hipLaunchKernelGGL(k_cert_ray_final, dim3(nb), dim3(NT), 0, s, C);
        launches++;
        T.stop(2);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(res + b0 * 4, res_d, (size_t)nb * 4 * 8, hipMemcpyDeviceToHost, s));
        if (at) HIP_TRY(hipMemcpyAsync(at + b0 * 4, at_d, (size_t)nb * 4 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(vd.data(), verdict_d, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int b = 0; b < nb; b++) { bad += vd[b] != 0; if (verdict) verdict[b0 + b] = vd[b]; }
    }
    h->last_raycert[0] = B; h->last_raycert[1] = bad; h->last_raycert[2] = launches;
    if (timing) fprintf(stderr, "bslv_lpq_certify_rays: %d LPs (%s form, %d x %d, chunks of %zu) A' z %.3f ms, A delta x %.3f ms, final %.3f ms; %ld launches, %ld not certified\n",
                        B, L.rev ? "revised" : "tableau", Mi, N0, Bc, T.ms[0], T.ms[1], T.ms[2], launches, bad);
    return 0;
}

int bslv_lpq_last_ray_certify_stats(const bslv_lpq *h, long out[3])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 3; k++) out[k] = h->last_raycert[k];
    return 0;
}

}  // extern "C"

// The drivers' helper (benson_driver.hip, vlp_phases.hip): an LP came back INFEASIBLE or UNBOUNDED and that ends the run.  While the
// engine keeps rays (BSLV_LP_RAYS=1 arranges that), one line on stderr says what the stored ray proves for the model as given; with the
// switch off nothing is done and nothing is printed.
namespace bslv {
void report_ray(bslv_lpq *lp, const char *phase, int status, int slot, const double *vlo, const double *vup, int cost_first, int cost_cnt, const double *costs)
{
    if (!lp || !bslv_lpq_get_rays(lp) || (status != BSLV_LP_INFEASIBLE && status != BSLV_LP_UNBOUNDED)) return;
    int kind = BSLV_LP_RAY_NONE, at[4] = {-1, -1, -1, -1}, verdict = -1;
    double res[4] = {NAN, NAN, NAN, NAN};
    if (bslv_lpq_get_ray(lp, 1, &slot, &kind, nullptr) || bslv_lpq_certify_rays(lp, 1, &slot, vlo, vup, cost_first, cost_cnt, costs, nullptr, res, at, &verdict)) {
        fprintf(stderr, "BSLV_LP_RAYS: %s: LP status %s, the ray could not be examined (%s)\n", phase, status == BSLV_LP_INFEASIBLE ? "INFEASIBLE" : "UNBOUNDED", bslv_last_error());
        return;
    }
    const bool dir = kind == BSLV_LP_RAY_DIRECTION;
    fprintf(stderr, "BSLV_LP_RAYS: %s: LP status %s, ray kind %s, %s %.3e at %d, %s %.3e at %d, margin %.3e, scale %.3e, verdict %d: %s\n", phase,
            status == BSLV_LP_INFEASIBLE ? "INFEASIBLE" : "UNBOUNDED", kind == BSLV_LP_RAY_FARKAS ? "FARKAS" : dir ? "DIRECTION" : "NONE",
            dir ? "rows" : "ident", res[0], at[0], dir ? "cross" : "open", res[1], at[1], res[2], res[3], verdict, verdict == 0 ? "certified" : "not certified");
}
}  // namespace bslv

extern "C" {

// for tests only: plain copies, no kernel
int bslv_lpq_debug_poke(bslv_lpq *h, int slot, int what, int var, double delta)
{
    if (!h || slot < 0 || slot >= h->slots || what < 0 || what > 1 || var < 0 || var >= h->L.M + h->L.N) { set_error("bslv_lpq_debug_poke: bad argument"); return BSLV_E_ARG; }
    if (h->ps.nfold) { set_error("bslv_lpq_debug_poke: the engine has folded rows (the indices of its own model are not the caller's)"); return BSLV_E_ARG; }
    const LpView &L = h->L;
    HIP_TRY(hipStreamSynchronize(h->stream));
    int p = 0;
    HIP_TRY(hipMemcpy(&p, L.pos + (size_t)slot * (L.M + L.N) + var, sizeof(int), hipMemcpyDeviceToHost));
    if (what == 1 && p >= 0) { set_error("bslv_lpq_debug_poke: variable %d of slot %d is basic (no stored reduced cost)", var, slot); return BSLV_E_ARG; }
    double *where;
    if (what == 0) where = p >= 0 ? L.beta + (size_t)slot * L.Mp1p + p : L.xN + (size_t)slot * L.ld + (-1 - p);
    else where = L.rev ? L.dsl + (size_t)slot * L.ld + (-1 - p) : L.T + (size_t)slot * L.slotT + (size_t)L.M * L.ld + (-1 - p);
    double v = 0;
    HIP_TRY(hipMemcpy(&v, where, sizeof(double), hipMemcpyDeviceToHost));
    v += delta;
    HIP_TRY(hipMemcpy(where, &v, sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

}  // extern "C"
