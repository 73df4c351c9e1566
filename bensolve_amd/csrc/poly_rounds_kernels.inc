// poly_rounds_kernels.inc -- kernels of the multi-cut path (included inside namespace bslv).
//
// Two cuts of a batch are INDEPENDENT when no live element is non-PLUS for both and no edge joins
// a non-PLUS element of one to a non-PLUS element of the other.  Then the elements each cut removes,
// moves onto its plane or creates, the edges it drops or adds and the incidence lists it rewrites are
// disjoint, every new vertex of one is PLUS for the other (it lies between two PLUS elements), and
// the cuts commute: applying them in ONE pass gives exactly what poly__add_vrtx gives one at a time.
// A round = classify all remaining cuts (the batched incidence kernel), find the conflicts, apply the
// independent ones (smallest index first, so the sequential order is kept among conflicting cuts) in
// one pass of the same four phases, re-classify the rest.

// non-PLUS cuts of element i from its class words (at most `cap` collected); returns the count found
__device__ __forceinline__ int touch_list(const unsigned long long *words, int capv, int nw, int i, int *out, int cap)
{
    int n = 0;
    for (int w = 0; w < nw; w++) {
        unsigned long long word = words[(size_t)w * capv + i];
        // class 1 (01) or 2 (10): exactly one of the two bits set
        unsigned long long m = (word ^ (word >> 1)) & 0x5555555555555555ull;
        while (m) {
            int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            if (n < cap) out[n] = w * 32 + (bit >> 1);
            n++;
        }
    }
    return n;
}

struct ConfBuf { int2 *pairs; int *count; int cap; int *overflow; };
__device__ __forceinline__ void conf_emit(const ConfBuf &C, int a, int b)
{
    if (a == b) return;
    int p = atomicAdd(C.count, 1);
    if (p < C.cap) C.pairs[p] = int2{min(a, b), max(a, b)};
    else *C.overflow = 1;
}
constexpr int TCAP = 24;
__global__ __launch_bounds__(PB) void k_conflict_v(PolyView P, const unsigned long long *words, int nw, int nv, const int *tc, ConfBuf C)
{
    int i = blockIdx.x * PB + threadIdx.x;
    if (i >= nv || tc[i] < 2) return;
    int L[TCAP];
    int n = touch_list(words, P.cap, nw, i, L, TCAP);
    if (n > TCAP) { *C.overflow = 1; return; }
    for (int a = 0; a < n; a++) for (int b = a + 1; b < n; b++) conf_emit(C, L[a], L[b]);
}
__global__ __launch_bounds__(PB) void k_conflict_e(PolyView P, const unsigned long long *words, int nw, const int2 *E, int ne, const int *tc,
                                                    const int *t1, ConfBuf C)
{
    int e = blockIdx.x * PB + threadIdx.x;
    if (e >= ne) return;
    int2 ed = E[e];
    const int ta = tc[ed.x], tb = tc[ed.y];
    if (ta == 0 || tb == 0) return;
    if (ta == 1 && tb == 1) { conf_emit(C, t1[ed.x], t1[ed.y]); return; }      // the common case: no word scan
    int A[TCAP], Bl[TCAP];
    int na = touch_list(words, P.cap, nw, ed.x, A, TCAP), nb = touch_list(words, P.cap, nw, ed.y, Bl, TCAP);
    if (na > TCAP || nb > TCAP) { *C.overflow = 1; return; }
    for (int a = 0; a < na; a++) for (int b = 0; b < nb; b++) conf_emit(C, A[a], Bl[b]);
}

// per element: the selected cut that touches it (at most one by independence) and its class for it
// counters: [0] MINUS elements, [1] ZERO elements, [2] sum over ZERO of (inc_len + 1), [3] error flag
__global__ __launch_bounds__(PB) void k_assign(PolyView P, const unsigned long long *words, int nw, int nv, const int *tc, const int *t1,
                                               const int *selmap /* per classified cut: index among the selected or -1 */,
                                               int *cutof, int *counters)
{
    int i = blockIdx.x * PB + threadIdx.x;
    if (i >= nv) return;
    unsigned char fl = P.flag[i];
    signed char c = 2;
    int owner = -1;
    if (fl & F_USED) {
        c = 1;
        if (tc[i] > 0) {
            int L[TCAP];
            int n = 1;
            L[0] = t1[i];
            if (tc[i] > 1) n = touch_list(words, P.cap, nw, i, L, TCAP);
            if (n > TCAP) atomicExch(&counters[3], 1);
            for (int k = 0; k < n && k < TCAP; k++) {
                int s = selmap[L[k]];
                if (s < 0) continue;
                if (owner >= 0) atomicExch(&counters[3], 2);          // two selected cuts touch one element: not independent
                owner = s;
                unsigned long long word = words[(size_t)(L[k] >> 5) * P.cap + i];
                int cl = (int)((word >> (2 * (L[k] & 31))) & 3ull);
                c = (cl == 1) ? -1 : 0;
            }
        }
    }
    P.cls[i] = c;
    cutof[i] = owner;
    if (c == -1) atomicAdd(&counters[0], 1);
    if (c == 0) { atomicAdd(&counters[1], 1); atomicAdd(&counters[2], P.inc_len[i] + 1); }
}

struct SelView {
    const double *hps;      // halfspaces of the classified cuts, (d+3) each (normal, alpha, alpha+-EPS)
    const int *selb;        // per selected cut: index into hps
    const int *self;        // per selected cut: global facet id
};

// multi-cut edge emit pass (survivors compacted, one vertex per crossing edge): halfspace and facet id come from the cut that owns the MINUS end
__global__ __launch_bounds__(PB) void k_edge_emit_m(PolyView P, SelView S, int *cutof, const int2 *E, int ne, const unsigned char *eflag,
                                                     const Tri *bpre, const Tri *totals, int2 *Enew, int nv0, unsigned pool0, int *err)
{
    __shared__ Tri lds[16];
    int e = blockIdx.x * PB + threadIdx.x;
    Tri t{0, 0, 0};
    unsigned char f = 0;
    int2 ed{0, 0};
    if (e < ne) {
        f = eflag[e]; ed = E[e];
        if (f == 1 || f == 4) t.a = 1;
        else if (f >= 2) {
            t.b = 1;
            t.c = isect_count(P.pool + P.inc_off[ed.x], P.inc_len[ed.x], P.pool + P.inc_off[ed.y], P.inc_len[ed.y]) + 1;
        }
    }
    Tri tot;
    Tri ex = block_exscan(t, &tot, lds);
    if (e >= ne) return;
    ex = tri_add(ex, bpre[blockIdx.x]);
    const int d = P.d;
    if (f == 1) Enew[ex.a] = ed;
    else if (f == 4) {
        Enew[ex.a] = ed;
        signed char ca = P.cls[ed.x], cb = P.cls[ed.y];
        int z = -1, pl = -1;
        if (ca == 0 && cb == 1) { z = ed.x; pl = ed.y; }
        else if (ca == 1 && cb == 0) { z = ed.y; pl = ed.x; }
        if (z >= 0) {
            const int *A = P.pool + P.inc_off[z], *Bp = P.pool + P.inc_off[pl];
            unsigned char *K = P.keep + P.inc_off[z];
            int na = P.inc_len[z], nb = P.inc_len[pl], i = 0, j = 0;
            while (i < na && j < nb) {
                int x = A[i], y = Bp[j];
                if (x == y) K[i] = 1;
                i += (x <= y);
                j += (y <= x);
            }
        }
    } else if (f == 2 || f == 3) {
        const int mi = (f == 2) ? ed.x : ed.y, pl = (f == 2) ? ed.y : ed.x;
        const int s = cutof[mi];
        if (s < 0 || (cutof[pl] >= 0 && cutof[pl] != s)) { *err = 3; return; }
        const double *hp = S.hps + (size_t)S.selb[s] * (d + 3);
        const int facet = S.self[s];
        const int w = nv0 + ex.b;
        const bool im = P.flag[mi] & F_IDEAL, ip = P.flag[pl] & F_IDEAL;
        double xm[MAXD], xp[MAXD];
        for (int k = 0; k < d; k++) { xm[k] = P.X[(size_t)k * P.cap + mi]; xp[k] = P.X[(size_t)k * P.cap + pl]; }
        double hb = 0.0, hd = 0.0, a2 = hp[d];
        unsigned char nf = F_USED;
        if (ip && im) {
            a2 = 0.0;
            for (int k = 0; k < d; k++) hd = fma(hp[k], xp[k] - xm[k], hd);
            for (int k = 0; k < d; k++) hb = fma(hp[k], xm[k], hb);
            double mu = (a2 - hb) / hd;
            for (int k = 0; k < d; k++) P.X[(size_t)k * P.cap + w] = fma(mu, xp[k] - xm[k], xm[k]);
            nf |= F_IDEAL;
        } else if (!ip && !im) {
            for (int k = 0; k < d; k++) hd = fma(hp[k], xm[k] - xp[k], hd);
            for (int k = 0; k < d; k++) hb = fma(hp[k], xp[k], hb);
            double mu = (a2 - hb) / hd;
            for (int k = 0; k < d; k++) P.X[(size_t)k * P.cap + w] = fma(mu, xm[k] - xp[k], xp[k]);
        } else {
            const double *base = ip ? xm : xp, *dirv = ip ? xp : xm;
            for (int k = 0; k < d; k++) hd = fma(hp[k], dirv[k], hd);
            for (int k = 0; k < d; k++) hb = fma(hp[k], base[k], hb);
            double mu = (a2 - hb) / hd;
            for (int k = 0; k < d; k++) P.X[(size_t)k * P.cap + w] = fma(mu, dirv[k], base[k]);
        }
        P.flag[w] = nf;
        P.cls[w] = 0;
        cutof[w] = s;
        const unsigned off = pool0 + (unsigned)ex.c;
        int *out = P.pool + off;
        const int *A = P.pool + P.inc_off[mi], *Bp = P.pool + P.inc_off[pl];
        int na = P.inc_len[mi], nb = P.inc_len[pl], i = 0, j = 0, n = 0;
        while (i < na && j < nb) {
            int x = A[i], y = Bp[j];
            if (x == y) out[n++] = x;
            i += (x <= y);
            j += (y <= x);
        }
        out[n++] = facet;
        P.inc_off[w] = off;
        P.inc_len[w] = n;
        Enew[totals[0].a + ex.b] = int2{w, pl};
    }
}

// multi-cut on-plane pass (incidence lists rebuilt from the keep marks): ZERO elements join the facet of their owner cut; zlist = ZERO elements in slot order
__global__ __launch_bounds__(PB) void k_vert_emit_m(PolyView P, SelView S, const int *cutof, int nv0, const Tri *bpre, int *zlist, unsigned pool0)
{
    __shared__ Tri lds[16];
    int i = blockIdx.x * PB + threadIdx.x;
    Tri t{0, 0, 0};
    signed char c = 2;
    if (i < nv0) {
        c = P.cls[i];
        if (c == 0) {
            const unsigned char *K = P.keep + P.inc_off[i];
            int n = P.inc_len[i], kept = 0;
            for (int j = 0; j < n; j++) kept += K[j];
            t.a = 1; t.c = kept + 1;
        }
    }
    Tri tot;
    Tri ex = block_exscan(t, &tot, lds);
    if (i >= nv0) return;
    if (c == -1) { P.flag[i] &= ~F_USED; return; }
    if (c != 0) return;
    ex = tri_add(ex, bpre[blockIdx.x]);
    zlist[ex.a] = i;
    const int facet = S.self[cutof[i]];
    const unsigned off_old = P.inc_off[i], off_new = pool0 + (unsigned)ex.c;
    const int n = P.inc_len[i];
    int m = 0;
    for (int j = 0; j < n; j++)
        if (P.keep[off_old + j]) { P.pool[off_new + m++] = P.pool[off_old + j]; P.keep[off_old + j] = 0; }
    P.pool[off_new + m++] = facet;
    P.inc_off[i] = off_new;
    P.inc_len[i] = m;
}

// members of the new facets, grouped by cut: count, scatter, then sort each group by element id
// (= ZERO elements in slot order followed by the new vertices: the sequential member order)
__global__ void k_mcount(const int *zlist, int nzero, int nv0, int ncross, const int *cutof, int *mcnt)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nzero + ncross) return;
    int v = k < nzero ? zlist[k] : nv0 + (k - nzero);
    atomicAdd(&mcnt[cutof[v]], 1);
}
__global__ void k_mscatter(const int *zlist, int nzero, int nv0, int ncross, const int *cutof, const int *moff, int *mfill, int *mem)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nzero + ncross) return;
    int v = k < nzero ? zlist[k] : nv0 + (k - nzero);
    int s = cutof[v];
    mem[moff[s] + atomicAdd(&mfill[s], 1)] = v;
}
__device__ __forceinline__ unsigned long long facet_bit(int f) { return 1ull << (((unsigned)f * 0x9E3779B1u) >> 26); }
// one workgroup per cut: rank sort of its members (ids are distinct), then a 64-bit signature of each
// member's incidence list (OR of one hashed bit per facet) for the superset sweep of the pair test
__global__ __launch_bounds__(PB) void k_msort_sig(PolyView P, const int *moff, const int *mem_in, int *mem, unsigned long long *msig)
{
    const int s = blockIdx.x;
    const int o = moff[s], n = moff[s + 1] - o;
    for (int k = threadIdx.x; k < n; k += PB) {
        int v = mem_in[o + k], r = 0;
        for (int j = 0; j < n; j++) r += (mem_in[o + j] < v);
        mem[o + r] = v;
        const int *L = P.pool + P.inc_off[v];
        int len = P.inc_len[v];
        unsigned long long sg = 0;
        for (int j = 0; j < len; j++) sg |= facet_bit(L[j]);
        msig[o + r] = sg;
    }
}

struct PairBlkM { int s, i, j0; };
// multi-cut adjacency prune: exact sorted-list prefilter per lane, wave-cooperative superset sweep
// over the members of the SAME cut, accelerated by the signatures (exact list check only on a hit)
__global__ __launch_bounds__(PB) void k_pair_flags_m(PolyView P, const int *moff, const int *mem, const unsigned long long *msig,
                                                      const PairBlkM *blks, unsigned char *pflag, Tri *bsum)
{
    __shared__ Tri lds[16];
    __shared__ int s_row[1024];
    const PairBlkM pb = blks[blockIdx.x];
    const int o = moff[pb.s], nm = moff[pb.s + 1] - o;
    const int vi = mem[o + pb.i];
    const int ni = P.inc_len[vi];
    const int *Li = P.pool + P.inc_off[vi];
    const bool cached = ni <= 1024;
    if (cached) for (int t = threadIdx.x; t < ni; t += PB) s_row[t] = Li[t];
    __syncthreads();
    const int *A = cached ? s_row : Li;
    const int j = pb.j0 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int vj = -1, nmut = 0;
    unsigned long long sigM = 0;
    bool cand = false;
    if (j < nm) {
        vj = mem[o + j];
        const int *Lj = P.pool + P.inc_off[vj];
        const int nj = P.inc_len[vj];
        int a = 0, b = 0;
        while (a < ni && b < nj) {
            int x = A[a], y = Lj[b];
            if (x == y) { nmut++; sigM |= facet_bit(x); }
            a += (x <= y);
            b += (y <= x);
        }
        cand = (P.d == 1) || (nmut >= P.d - 1);
    }
    bool adj = cand;
    unsigned long long todo = __ballot(cand && P.d > 1);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int cj = __shfl(vj, src, WAVE);
        const int cn = __shfl(nmut, src, WAVE);
        const unsigned long long cs = __shfl(sigM, src, WAVE);
        bool found = false;
        for (int base = 0; base < nm; base += WAVE) {
            const int w = base + lane;
            bool hit = false;
            if (w < nm && (cs & ~msig[o + w]) == 0ull) {
                const int vw = mem[o + w];
                if (vw != vi && vw != cj) {
                    const int nw_ = P.inc_len[vw];
                    if (nw_ >= cn)
                        hit = isect3_count(A, ni, P.pool + P.inc_off[cj], P.inc_len[cj], P.pool + P.inc_off[vw], nw_) == cn;
                }
            }
            if (__ballot(hit)) { found = true; break; }
        }
        if (lane == src) adj = !found;
    }
    Tri t{adj ? 1 : 0, 0, 0};
    pflag[(size_t)blockIdx.x * PB + threadIdx.x] = adj ? 1 : 0;
    Tri tot;
    (void)block_exscan(t, &tot, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(PB) void k_pair_emit_m(const int *moff, const int *mem, const PairBlkM *blks, const unsigned char *pflag,
                                                     const Tri *bpre, int2 *E, int ebase)
{
    __shared__ Tri lds[16];
    const PairBlkM pb = blks[blockIdx.x];
    unsigned char f = pflag[(size_t)blockIdx.x * PB + threadIdx.x];
    Tri t{f, 0, 0};
    Tri tot;
    Tri ex = block_exscan(t, &tot, lds);
    if (!f) return;
    const int o = moff[pb.s];
    E[ebase + bpre[blockIdx.x].a + ex.a] = int2{mem[o + pb.i], mem[o + pb.j0 + threadIdx.x]};
}
