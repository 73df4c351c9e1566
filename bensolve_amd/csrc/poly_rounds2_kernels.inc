// poly_rounds2_kernels.inc -- rounds of independent cuts INSIDE a hot chunk, chosen and applied on the device
// (included inside namespace bslv, after the single-cut pipeline).
//
// Why: on the bench workload a batch of 2048 LPs yields ~600 distinct cuts that all act on one neighbourhood of the
// polyhedron (~13 000 of its elements); the single-cut pipeline applies them one after the other at ~40 us each -- a
// latency chain with the chip idle.  The conflict graph of such a batch (two cuts conflict when an element is non-PLUS for
// both or an edge joins their non-PLUS regions) has ~16 % of all pairs, cliques of ~90 cuts, and falls apart into ~100-150
// rounds of mutually independent cuts.  Independent cuts commute exactly (poly_rounds_kernels.inc), so one ROUND applies
// several of them in the passes of ONE cut:
//
//   k_r2_prep     per hot element: the alive cut of highest priority that touches it (its owner candidate), which alive cuts
//                 have a MINUS element at all; per hot element / hot edge: every cut that meets a cut of higher priority
//                 on an element or across an edge is marked `bad` -- O(touches), no pair enumeration, no conflict matrix
//   k_r2_select   one workgroup: selected = alive, not redundant, not bad (the local minima of a fixed pseudo-random
//                 priority: an independent set that always holds the alive cut of highest priority), ranks, bookkeeping
//   k_r2_assign   per hot element: class (-1 / 0 / +1) and owner among the selected cuts -> P.cls, cutof
//   k_flags2      (the single-cut kernel, unchanged) flags, list lengths, keep marks
//   k_r2_emit     the single-cut emit pass with the halfspace and the facet rank of the OWNER of each crossing edge / on-plane
//                 element; verdict on the capacities
//   k_r2_prune_classify  one launch of two kinds of workgroups, which do not depend on each other:
//                 one workgroup per selected cut: the adjacency prune of its new facet, result as a bitmap (k2_fused_body<true>);
//                 behind them: the new vertices against the alive cuts of the chunk, which of their words hold a touch (r2_classify3_body)
//                 (BSLV_R2_RIDE=0: as two launches, k_r2_classify3 and k2_fused_t<true>)
//   k_r2_k2emit  ordered emission of the adjacent pairs of all selected cuts, commit of the sizes, mailbox to the host
//
// The classes of an element against the cuts of the chunk never change (coordinates are immutable), so the class words of
// the chunk's batched classification serve every round; only the vertices a round creates are classified (once).

struct RState {
    // committed sizes (inputs of a round; k_r2_k2emit commits the outputs at its end)
    int nv, ne, nranks;
    unsigned poolused;
    // selection of the round (k_r2_select)
    int round, S, rank_base, napplied, nredundant, nalive, stuck;
    // verdict and sizes of the round (k_r2_emit, workgroup 0)
    int go, declined, nminus, nzero, zero_ub, nsurv, ncross, newlen;
    int nv_next, ne_next; unsigned pool_next, pool_e, pool_z;
    // adjacency prunes of the round (k2_fused_t<true> / k_r2_k2emit)
    int epairs, eover, k2abort;
    long long pair_tests;
    // Rounds are queued ahead of the host (round r+1 behind round r before r's mailbox has been read).  Whatever the host would have
    // to deal with first -- a capacity that is short (1), adjacent pairs that did not fit or a prune that needs its fallback (1), a
    // grid that is too small for what the rounds before created (2), a round that selected nothing (3) -- raises `halt`: every
    // kernel queued behind returns at once (k_r2_k2emit still publishes the mailbox), the host clears it when it has caught up.
    int halt;
    int halt2;                   // raised by k_r2_k2emit: ITS sequence number, so that its own workgroups -- which may start after workgroup 0 has raised it -- go on
    int err, err_info[7];        // first inconsistency a kernel of the round saw (0: none)
    double err_d[12];
    unsigned chk;                // sum over the words of the state (chk = seq = 0 while it is taken) + the sequence number: see r2_wait
    int seq;
};
static_assert(offsetof(RState, halt2) == offsetof(RState, halt) + sizeof(int), "k_flags2 reads (halt, halt2) as two consecutive ints");
// The state reaches the host through mapped pinned memory and spans four cache lines.  The writer stores the struct, fences, stores
// seq -- but posted writes of different lines may still land out of order on some hosts (seen as a round whose seq had arrived while
// S / nalive were those of the previous mailbox: the chunk "ended" after its first round).  So the struct carries a checksum that
// includes the sequence number, and the host re-reads until a copy with the awaited seq also has the matching sum.
__host__ __device__ __forceinline__ unsigned rstate_sum(const RState &s, int seq)
{
    const unsigned *w = reinterpret_cast<const unsigned *>(&s);
    unsigned c = 0x9E3779B9u;
    for (unsigned i = 0; i < sizeof(RState) / 4; i++) c = c * 31u + w[i];
    return c + (unsigned)seq * 2654435761u;
}
__device__ __forceinline__ void rstate_publish(RState *st, RState *mail, int seq)
{
    st->seq = 0; st->chk = 0;
    st->chk = rstate_sum(*st, seq);
    *mail = *st;
    __threadfence_system();
    mail->seq = seq;
}

__device__ __forceinline__ bool r2_halted(const RState *st) { return st->halt != 0 || st->halt2 != 0; }
// PRIORITY = INDEX: the host shuffles the cuts of a chunk (pseudo-random, the same on every rank) before they are
// classified, so the index order of the class words is the priority order.  The owner candidate of an element is then the
// LOWEST set bit of (its non-PLUS cuts & alive), and "every cut of lower priority that touches this element" is a bit mask:
// the prep pass has no loop over touches at all (with a priority table it spent 60 us walking the ~90 touches of the most
// crowded elements).
// hw: ELEMENT-major copy of the class words, hw[i * nw + w] (the words of one element are two cache lines).
// The class words of an element are fetched R2B at a time with independent loads: a loop that stops at the first non-zero
// word is a chain of dependent memory latencies (it cost 30 us per pass).
constexpr int R2B = 8;
__device__ __forceinline__ void r2_load(const unsigned long long *hw, int nw, int i, const unsigned *alive, int w0, unsigned (&t)[R2B])
{
    unsigned long long raw[R2B];
#pragma unroll
    for (int j = 0; j < R2B; j++) raw[j] = (w0 + j < nw && alive[w0 + j]) ? hw[(size_t)i * nw + w0 + j] : 0ull;
#pragma unroll
    for (int j = 0; j < R2B; j++) t[j] = (w0 + j < nw) ? compress32((raw[j] ^ (raw[j] >> 1)) & 0x5555555555555555ull) & alive[w0 + j] : 0u;
}
// alive cut of highest priority (lowest index) touching element i, or -1
__device__ __forceinline__ int r2_owner(const unsigned long long *hw, int nw, int i, const unsigned *alive)
{
    for (int w0 = 0; w0 < nw; w0 += R2B) {
        unsigned t[R2B];
        r2_load(hw, nw, i, alive, w0, t);
#pragma unroll
        for (int j = 0; j < R2B; j++) if (t[j]) return (w0 + j) * 32 + __ffs((int)t[j]) - 1;
    }
    return -1;
}
// every alive cut touching element i with an index above o loses this round (bad: LDS bit mask, one word per 32 cuts)
__device__ __forceinline__ void r2_mark_above(const unsigned long long *hw, int nw, int i, const unsigned *alive, int o, unsigned *bad)
{
    for (int w0 = (o >> 5) & ~(R2B - 1); w0 < nw; w0 += R2B) {
        unsigned t[R2B];
        r2_load(hw, nw, i, alive, w0, t);
#pragma unroll
        for (int j = 0; j < R2B; j++) {
            const int w = w0 + j;
            unsigned m = t[j];
            if (w < (o >> 5)) m = 0u;
            else if (w == (o >> 5)) m &= ~((2u << (o & 31)) - 1u);      // bits above o (o itself excluded)
            if (w < nw && (m & ~bad[w])) atomicOr(&bad[w], m);
        }
    }
}
// dynamic LDS: alive[nw] | bad[nw] | anyminus[nw]
// tc: touch counts of the chunk's classification (an element that is neither touched -- tc 0 -- nor new has no class words in hw:
// it is PLUS for every cut, and what hw holds for it is left over from an earlier chunk)
__global__ __launch_bounds__(PB) void k_r2_prep(PolyView P, const unsigned long long *__restrict__ hw, int nw, const RState *st, const int2 *__restrict__ E, int nbe,
                                                const unsigned *__restrict__ alive_g, unsigned *anym_g, unsigned *bad_g, int *own, const int *__restrict__ tc, RState *st_w)
{
    extern __shared__ unsigned r2_lds[];
    if (r2_halted(st)) return;
    unsigned *alive = r2_lds, *bad = r2_lds + nw, *anym = r2_lds + 2 * nw;
    for (int w = threadIdx.x; w < nw; w += PB) { alive[w] = alive_g[w]; bad[w] = 0u; anym[w] = 0u; }
    __syncthreads();
    const int nv = st->nv, ne = st->ne;
    // queued before the host knew the sizes: the grid must cover them (the same nbe / grid serves every kernel of the round)
    if (blockIdx.x == 0 && threadIdx.x == 0 && ((ne + PB - 1) / PB > nbe || (vm_count(P, nv) + PB - 1) / PB > (int)gridDim.x - nbe)) st_w->halt = 2;
    if ((int)blockIdx.x < nbe) {
        const int e = blockIdx.x * PB + threadIdx.x;
        if (e < ne) {
            const int2 ed = E[e];
            const bool hu = ed.x >= P.nv_base || tc[ed.x] > 0, hv2 = ed.y >= P.nv_base || tc[ed.y] > 0;
            const int ou = (hu && hv2) ? r2_owner(hw, nw, ed.x, alive) : -1;
            const int ov = ou >= 0 ? r2_owner(hw, nw, ed.y, alive) : -1;
            if (ov >= 0) {
                // a cut on one end meets the owner candidate of the other end across this edge: the lower priority loses
                r2_mark_above(hw, nw, ed.x, alive, ov, bad);
                r2_mark_above(hw, nw, ed.y, alive, ou, bad);
            }
        }
    } else {
        const int idx = ((int)blockIdx.x - nbe) * PB + threadIdx.x;
        const bool valid = idx < vm_count(P, nv);
        const int i = valid ? vm_id(P, idx) : 0;
        const bool live = valid && (P.flag[i] & F_USED);
        int o = -1;
        for (int w0 = 0; w0 < nw; w0 += R2B) {
            unsigned long long raw[R2B];
#pragma unroll
            for (int j = 0; j < R2B; j++) raw[j] = (live && w0 + j < nw && alive[w0 + j]) ? hw[(size_t)i * nw + w0 + j] : 0ull;
#pragma unroll
            for (int j = 0; j < R2B; j++) {
                const int w = w0 + j;
                if (w >= nw) continue;
                const unsigned a = alive[w];
                unsigned t = compress32((raw[j] ^ (raw[j] >> 1)) & 0x5555555555555555ull) & a;
                const unsigned minus = compress32(raw[j] & ~(raw[j] >> 1)) & a;              // class 01
                if (minus & ~anym[w]) atomicOr(&anym[w], minus);
                if (t) {
                    if (o < 0) { o = w * 32 + __ffs((int)t) - 1; t &= t - 1; }      // the owner candidate; every other toucher loses
                    if (t & ~bad[w]) atomicOr(&bad[w], t);
                }
            }
        }
        if (valid) own[i] = o;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < nw; w += PB) {
        if (bad[w] & ~__hip_atomic_load(&bad_g[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&bad_g[w], bad[w]);
        if (anym[w] & ~__hip_atomic_load(&anym_g[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&anym_g[w], anym[w]);
    }
}

// one workgroup.  selected = alive, has a MINUS element, not bad; redundant = alive without a MINUS element (no live element
// violates it, and by convexity none ever will); the others stay alive for the next round.
__global__ __launch_bounds__(1024) void k_r2_select(int Bc, unsigned *alive, unsigned *alive_prev, unsigned *anym, unsigned *bad, int *selmap, int *sel, int *order,
                                                    int *rcflag, RState *st, int spec)
{
    __shared__ Tri lds[16];
    if (r2_halted(st)) return;
    const int napplied0 = st->napplied;
    Tri carry{0, 0, 0};
    for (int base = 0; base < Bc; base += 1024) {
        const int k = base + threadIdx.x;
        int a = 0, m = 0, b = 0;
        if (k < Bc) { a = (alive[k >> 5] >> (k & 31)) & 1u; m = (anym[k >> 5] >> (k & 31)) & 1u; b = (bad[k >> 5] >> (k & 31)) & 1u; }
        const int s = a && m && !b, r = a && !m, keep = a && !s && !r;
        Tri t{s, r, keep};
        Tri tot;
        const Tri ex = block_exscan(t, &tot, lds);                 // (barriers inside: every thread has read its bits)
        if (k < Bc) {
            selmap[k] = s ? carry.a + ex.a : -1;
            if (s) { sel[carry.a + ex.a] = k; order[napplied0 + carry.a + ex.a] = k; rcflag[k] = 0; }
            if (r) rcflag[k] = 1;
        }
        const unsigned long long ba = __ballot(a), bk = __ballot(keep);
        if ((threadIdx.x & 63) == 0 && k < Bc) {
            const int w0 = k >> 5;
            alive_prev[w0] = (unsigned)ba; alive[w0] = (unsigned)bk;
            if (k + 32 < ((Bc + 31) & ~31)) { alive_prev[w0 + 1] = (unsigned)(ba >> 32); alive[w0 + 1] = (unsigned)(bk >> 32); }
        }
        carry = tri_add(carry, tot);
        __syncthreads();
    }
    for (int w = threadIdx.x; w < (Bc + 31) / 32; w += 1024) { anym[w] = 0u; bad[w] = 0u; }
    if (threadIdx.x == 0) {
        st->round += 1;
        st->S = carry.a;
        st->rank_base = st->nranks;
        st->nranks += carry.a;
        st->napplied = napplied0 + carry.a;
        st->nredundant += carry.b;
        st->nalive = carry.c;
        st->stuck = (carry.a == 0 && carry.b == 0 && carry.c > 0) ? 1 : 0;
        st->go = 0; st->declined = 0; st->epairs = 0; st->eover = 0; st->k2abort = 0; st->ncross = 0; st->nzero = 0;
        if (spec && carry.a == 0) st->halt = 3;          // (nothing selected: the buffers do not change over, which a round queued behind assumed)
    }
}
// a round whose capacities were short is taken back: the selected cuts are alive again
__global__ void k_r2_undo(int Bc, unsigned *alive, const unsigned *alive_prev, const int *selmap, RState *st)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < Bc && selmap[k] >= 0) atomicOr(&alive[k >> 5], 1u << (k & 31));
    if (k == 0) { st->nranks -= st->S; st->napplied -= st->S; st->S = 0; st->declined = 0; }
}

// class and owner of every hot element for the selected cuts of the round; counters as k_classify leaves them
// ([0] MINUS, [1] ZERO, [2] list bound of the ZERO elements, [3] long ZERO elements, the first ZMAX of them in zlist)
__global__ __launch_bounds__(PB) void k_r2_assign(PolyView P, const unsigned long long *__restrict__ words, int nw, const RState *st, const int *__restrict__ own,
                                                  const int *__restrict__ selmap, int *cutof, int *counters, int *zlist)
{
    const int idx = blockIdx.x * PB + threadIdx.x;
    int isminus = 0, iszero = 0, zlen = 0;
    if (r2_halted(st)) return;
    if (idx < vm_count(P, st->nv)) {
        const int i = vm_id(P, idx);
        signed char c = 2;
        int s = -1;
        if (P.flag[i] & F_USED) {
            c = 1;
            const int o = st->S > 0 ? own[i] : -1;
            if (o >= 0 && (s = selmap[o]) >= 0) {
                const unsigned long long word = words[(size_t)i * nw + (o >> 5)];
                const int cl = (int)((word >> (2 * (o & 31))) & 3ull);
                c = (cl == 1) ? -1 : 0;
                isminus = c < 0; iszero = c == 0;
                if (iszero) {
                    zlen = zero_room(P, i, 1);
                    // on-plane elements with long lists get a row of facet stamps (ZMarks), as in k_classify
                    if (P.inc_len[i] > LONGN) { const int k = atomicAdd(&counters[3], 1); if (k < ZMAX) zlist[k] = i; }
                }
            }
        }
        P.cls[i] = c;
        cutof[i] = s;
    }
    const unsigned long long bm = __ballot(isminus), bz = __ballot(iszero);
    if (bz) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) zlen += __shfl_xor(zlen, o, WAVE);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bm) atomicAdd(&counters[0], __popcll(bm));
        if (bz) { atomicAdd(&counters[1], __popcll(bz)); atomicAdd(&counters[2], zlen); }
    }
}

// emit pass of a round: k_emit2 with the halfspace and the facet rank of the owner cut (hps: (d+3) doubles per classified
// cut, sel: classified index of each selected cut).  Every workgroup sums the block sums of k_flags2 itself; workgroup 0
// publishes the verdict.  Nothing is committed here: the sizes of the next round are written by k_r2_k2emit.
template <int D>
__global__ __launch_bounds__(PB) void k_r2_emit(PolyView P, const double *__restrict__ hps, const int *__restrict__ sel, int *cutof, const int2 *E, int nbe,
                                                const unsigned char *eflag, const int *ecount, const Tri *ebsum, const Tri *vbsum, int2 *Enew, int *members,
                                                const int *counters, RState *st, int vcap, int ecap, unsigned poolcap, const int *EPold, int *EPnew, ZMarks Z,
                                                const unsigned long long *__restrict__ hw, const unsigned *__restrict__ wm, int nw, int *mcnt,
                                                const unsigned *__restrict__ selw, const int *__restrict__ selmap)
{
    __shared__ Tri lds[16];
    if (st->S <= 0 || r2_halted(st)) return;
    const int nv0 = st->nv, ne = st->ne, rank_base = st->rank_base;
    const unsigned poolused = st->poolused;
    const bool eblock = (int)blockIdx.x < nbe;
    const int mye = eblock ? nbe - 1 - (int)blockIdx.x : 0, myv = eblock ? 0 : (int)gridDim.x - 1 - (int)blockIdx.x;
    Tri pe{0, 0, 0}, te{0, 0, 0}, pv{0, 0, 0};
    for (int i = threadIdx.x; i < nbe; i += PB) { const Tri v = ebsum[i]; te = tri_add(te, v); if (eblock && i < mye) pe = tri_add(pe, v); }
    if (!eblock) for (int i = threadIdx.x; i < myv; i += PB) pv = tri_add(pv, vbsum[i]);
    te = block_sum(te, lds);
    Tri pre_e{0, 0, 0}, pre_v{0, 0, 0};
    if (eblock) pre_e = block_sum(pe, lds); else pre_v = block_sum(pv, lds);
    const int zero_ub = counters[2];
    const bool go = nv0 + te.b <= vcap && te.a + te.b <= ecap && (unsigned long long)poolused + (unsigned)te.c + (unsigned)zero_ub <= poolcap;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->go = go; st->declined = !go;
        if (!go) st->halt = 1;
        st->nminus = counters[0]; st->nzero = counters[1]; st->zero_ub = zero_ub;
        st->nsurv = te.a; st->ncross = te.b; st->newlen = te.c;
        st->nv_next = nv0 + te.b; st->ne_next = te.a + te.b;
        st->pool_e = poolused; st->pool_z = poolused + (unsigned)te.c; st->pool_next = poolused + (unsigned)te.c + (unsigned)zero_ub;
    }
    if (!go) return;
    const unsigned pool_e = poolused, pool_z = poolused + (unsigned)te.c;
    const int nsurv_all = te.a;
    const int d = D > 0 ? D : P.d;
    Tri t{0, 0, 0};
    Tri tot;
    if (eblock) {
        const int eb = nbe - 1 - (int)blockIdx.x;
        const int e = eb * PB + threadIdx.x;
        unsigned char f = 0;
        int2 ed{0, 0};
        if (e < ne) {
            f = eflag[e]; ed = E[e];
            if (f == 1 || f == 4 || f == 5) t.a = 1;
            else if (f >= 2) { t.b = 1; t.c = ecount[e]; }
        }
        Tri ex = block_exscan(t, &tot, lds);
        if (e >= ne) return;
        ex = tri_add(ex, pre_e);
        if (f == 1 || f == 4 || f == 5) { Enew[ex.a] = ed; if (EPold) EPnew[ex.a] = EPold[e]; }
        else if (f == 2 || f == 3) {
            const int mi = (f == 2) ? ed.x : ed.y, pl = (f == 2) ? ed.y : ed.x;
            const int s = cutof[mi];
            const double *hp = hps + (size_t)sel[s] * (d + 3);
            const int facet = rank_base + s;
            const int w = nv0 + ex.b;
            const bool im = P.flag[mi] & F_IDEAL, ip = P.flag[pl] & F_IDEAL;
            constexpr int DD = D > 0 ? D : MAXD;
            double xm[DD], xp[DD], base[DD], dirv[DD], hh[DD];
#pragma unroll
            for (int k = 0; k < DD; k++) { xm[k] = k < d ? P.X[(size_t)k * P.cap + mi] : 0.0; xp[k] = k < d ? P.X[(size_t)k * P.cap + pl] : 0.0; hh[k] = k < d ? hp[k] : 0.0; }
            double hb = 0.0, hd = 0.0, a2 = hp[d];
            unsigned char nf = F_USED;
            // new vertex on the edge (bslv_poly.c:597-627); same operation order as oracle/poly_dd.c and k_emit2
            if (ip && im) {
                a2 = 0.0; nf |= F_IDEAL;
#pragma unroll
                for (int k = 0; k < DD; k++) { base[k] = xm[k]; dirv[k] = xp[k] - xm[k]; }
            } else if (!ip && !im) {
#pragma unroll
                for (int k = 0; k < DD; k++) { base[k] = xp[k]; dirv[k] = xm[k] - xp[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < DD; k++) { base[k] = ip ? xm[k] : xp[k]; dirv[k] = ip ? xp[k] : xm[k]; }
            }
#pragma unroll
            for (int k = 0; k < DD; k++) if (k < d) hd = fma(hh[k], dirv[k], hd);
#pragma unroll
            for (int k = 0; k < DD; k++) if (k < d) hb = fma(hh[k], base[k], hb);
            const double mu = (a2 - hb) / hd;
            if (!(fabs(mu) < 1e300) && atomicCAS(&st->err, 0, 1) == 0) {          // (never seen with consistent classes: reported, not repaired)
                st->err_info[0] = e; st->err_info[1] = mi; st->err_info[2] = pl; st->err_info[3] = s; st->err_info[4] = sel[s];
                st->err_info[5] = P.cls[mi] * 16 + P.cls[pl]; st->err_info[6] = (int)f;
                st->err_d[0] = hb; st->err_d[1] = hd; st->err_d[2] = a2; st->err_d[3] = (double)(im * 2 + ip);
                for (int k = 0; k < 4 && k < d; k++) { st->err_d[4 + k] = xm[k]; st->err_d[8 + k] = xp[k]; }
            }
#pragma unroll
            for (int k = 0; k < DD; k++) if (k < d) P.X[(size_t)k * P.cap + w] = fma(mu, dirv[k], base[k]);
            P.flag[w] = nf;
            P.cls[w] = 0;
            cutof[w] = s;
            // incidence = inc(minus) & inc(plus) + new facet (bslv_poly.c:634-665)
            const unsigned off = pool_e + (unsigned)ex.c;
            int *out = P.pool + off;
            const int *A = P.pool + P.inc_off[mi], *Bp = P.pool + P.inc_off[pl];
            int na = P.inc_len[mi], nb = P.inc_len[pl], n = 0;
            if (na <= LCAP && nb <= LCAP) {
                int RA[LCAP], RB[LCAP];
                load_list(A, na, RA); load_list(Bp, nb, RB);
                const unsigned m = match_mask(RA, na, RB);
#pragma unroll
                for (int a = 0; a < LCAP; a++) if ((m >> a) & 1u) out[n++] = RA[a];
            } else if (na <= LCAP || nb <= LCAP) {
                const bool ashort = na <= nb;
                int S2[LCAP], pos[LCAP];
                load_list(ashort ? A : Bp, ashort ? na : nb, S2);
                const unsigned *row = lrow(P, ashort ? pl : mi);
                const unsigned m = row ? match_mask_bits(S2, ashort ? na : nb, row)
                                       : match_mask_long(S2, ashort ? na : nb, ashort ? Bp : A, ashort ? nb : na, pos);
#pragma unroll
                for (int a = 0; a < LCAP; a++) if ((m >> a) & 1u) out[n++] = S2[a];
            } else {
                const bool ashort = na <= nb;
                const int ns = ashort ? na : nb;
                const unsigned *row = ns <= LONGN ? lrow(P, ashort ? pl : mi) : nullptr;
                if (row) {
                    const int *S2 = ashort ? A : Bp;
                    for (int c0 = 0; c0 < ns; c0 += LCAP) {
                        const int nc = ns - c0 < LCAP ? ns - c0 : LCAP;
                        int RS[LCAP];
                        load_list(S2 + c0, nc, RS);
                        const unsigned m = match_mask_bits(RS, nc, row);
#pragma unroll
                        for (int a = 0; a < LCAP; a++) if ((m >> a) & 1u) out[n++] = RS[a];
                    }
                } else isect_each(A, na, Bp, nb, [&](int x, int, int) { out[n++] = x; });
            }
            out[n++] = facet;
            P.inc_off[w] = off;
            P.inc_len[w] = n;
            Enew[nsurv_all + ex.b] = int2{w, pl};
            if (EPold) EPnew[nsurv_all + ex.b] = -1;
        }
        return;
    }
    // ---- vertex blocks ----
    const int b = (int)gridDim.x - 1 - (int)blockIdx.x, idx = b * PB + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = idx < vm_count(P, nv0);
    const int i = valid ? vm_id(P, idx) : -1;
    signed char c = 2;
    int n = 0, co = -1;
    unsigned off_old = 0;
    if (valid) {
        c = P.cls[i];
        if (c == 0) { off_old = P.inc_off[i]; n = P.inc_len[i]; co = cutof[i]; t.a = 1; t.c = zero_room(P, i, co < -1 ? -1 - co : 1); }
    }
    const int room = t.c;                      // (0: a long list with slack, rebuilt where it lies)
    Tri ex = block_exscan(t, &tot, lds);
    ex = tri_add(ex, pre_v);
    const unsigned off_new = (c == 0 && room == 0) ? off_old : pool_z + (unsigned)ex.c;
    const bool shared = (c == 0) && co < -1;       // on the planes of several cuts of the round: the whole list stays, their facets are appended in rank order
    const int facet = (c == 0 && !shared) ? rank_base + co : 0;
    const bool longz = (c == 0) && n > LONGN;
    // the facets of the owners of a shared element, appended at P.pool[at ..) by the calling lane; returns their number
    auto append_owners = [&](int v, unsigned at, unsigned *lb) -> int {
        int cnt = 0;
        r2_for_owners(hw, wm, nw, selw, v, [&](int o) {
            const int g = rank_base + selmap[o];
            P.pool[at + cnt++] = g;
            if (lb) atomicOr(&lb[g >> 5], 1u << (g & 31));
        });
        return cnt;
    };
    {   // long lists (extreme directions): ordered compaction by the whole wave (ballot ranks), then the new facet(s)
        unsigned long long todo = __ballot(longz);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned oo = __shfl(off_old, src, WAVE), on = __shfl(off_new, src, WAVE);
            const int nn = __shfl(n, src, WAVE), vv = __shfl(i, src, WAVE), ff = __shfl(facet, src, WAVE), rm = __shfl(room, src, WAVE);
            const bool sh = __shfl((int)shared, src, WAVE) != 0;
            const int zid = sh ? -1 : zmarks_find(Z, counters, vv);
            const int *row = zid >= 0 ? Z.rows + (size_t)zid * Z.stride : nullptr;
            unsigned *lb = const_cast<unsigned *>(lrow(P, vv));
            if (lb && !sh) {          // (a shared element keeps every entry: its membership bitmap only gains bits)
                for (int w = lane; w < P.lstride; w += WAVE) lb[w] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            int base = 0;
            constexpr int LIT = 16;                     // lists of up to 1024 facets: all entries and all marks are fetched first
            if (nn <= LIT * WAVE) {                     // (two memory latencies in all instead of two per 64 entries: as k_emit2 -- one
                int g[LIT];                             //  entry batch after the other cost 120-180 us per round on covering problems,
                bool k[LIT];                            //  whose extreme directions lie on thousands of facets)
#pragma unroll
                for (int it = 0; it < LIT; it++) { const int j = it * WAVE + lane; g[it] = j < nn ? P.pool[oo + j] : 0; }
#pragma unroll
                for (int it = 0; it < LIT; it++) { const int j = it * WAVE + lane; k[it] = j < nn && (sh || (row ? row[g[it]] == Z.stamp : P.keep[oo + j] != 0)); }
#pragma unroll
                for (int it = 0; it < LIT; it++) {
                    if (it * WAVE >= nn) break;
                    const unsigned long long bm = __ballot(k[it]);
                    if (k[it]) {
                        P.pool[on + base + __popcll(bm & ((1ull << lane) - 1ull))] = g[it];
                        if (!row && !sh) P.keep[oo + it * WAVE + lane] = 0;
                        if (lb && !sh) atomicOr(&lb[g[it] >> 5], 1u << (g[it] & 31));
                    }
                    base += __popcll(bm);
                }
            } else
            for (int j0 = 0; j0 < nn; j0 += LIT * WAVE) {          // longer lists: batches of LIT x 64 entries
                int g[LIT];
                bool k[LIT];
#pragma unroll
                for (int it = 0; it < LIT; it++) { const int j = j0 + it * WAVE + lane; g[it] = j < nn ? P.pool[oo + j] : 0; }
#pragma unroll
                for (int it = 0; it < LIT; it++) { const int j = j0 + it * WAVE + lane; k[it] = j < nn && (sh || (row ? row[g[it]] == Z.stamp : P.keep[oo + j] != 0)); }
#pragma unroll
                for (int it = 0; it < LIT; it++) {
                    if (j0 + it * WAVE >= nn) break;
                    const unsigned long long bm = __ballot(k[it]);
                    if (k[it]) {
                        P.pool[on + base + __popcll(bm & ((1ull << lane) - 1ull))] = g[it];
                        if (!row && !sh) P.keep[oo + j0 + it * WAVE + lane] = 0;
                        if (lb && !sh) atomicOr(&lb[g[it] >> 5], 1u << (g[it] & 31));
                    }
                    base += __popcll(bm);
                }
            }
            if (lane == 0) {
                int added = 1;
                if (sh) added = append_owners(vv, on + base, lb);
                else { P.pool[on + base] = ff; if (lb) atomicOr(&lb[ff >> 5], 1u << (ff & 31)); }
                P.inc_off[vv] = on; P.inc_len[vv] = base + added;
                if (rm > 0) P.capx[vv] = ((unsigned long long)on << 32) | (unsigned)rm;       // (moved: the room reserved for it, slack included)
            }
        }
    }
    if (!valid) return;
    if (c == -1) {
        P.flag[i] &= ~F_USED;
        if (mcnt) {                      // (conflict-matrix rounds) the element takes its MINUS marks with it
            unsigned m = wm[i];
            while (m) {
                const int w = __ffs((int)m) - 1;
                m &= m - 1;
                unsigned mi = r2_minus32(hw[(size_t)i * nw + w]);
                while (mi) { const int b = __ffs((int)mi) - 1; mi &= mi - 1; atomicSub(&mcnt[w * 32 + b], 1); }
            }
        }
        return;
    }
    if (c != 0) return;
    members[ex.a] = i;
    if (longz) return;
    int m = 0;
    if (shared) {
        for (int j = 0; j < n; j++) P.pool[off_new + m++] = P.pool[off_old + j];
        m += append_owners(i, off_new + (unsigned)m, nullptr);
    } else {
        if (n <= LCAP) {
            int lst[LCAP];
            unsigned keptmask = 0;
            const unsigned char *K = P.keep + off_old;
            load_list(P.pool + off_old, n, lst);
#pragma unroll
            for (int j = 0; j < LCAP; j++) { unsigned k = (j < n) ? K[j] : 0; keptmask |= (k & 1u) << j; }
#pragma unroll
            for (int j = 0; j < LCAP; j++) if ((keptmask >> j) & 1u) { P.pool[off_new + m++] = lst[j]; P.keep[off_old + j] = 0; }
        } else
            for (int j = 0; j < n; j++)
                if (P.keep[off_old + j]) { P.pool[off_new + m++] = P.pool[off_old + j]; P.keep[off_old + j] = 0; }
        P.pool[off_new + m++] = facet;
    }
    P.inc_off[i] = off_new;
    P.inc_len[i] = m;
    relist_bitmap(P, i, off_new, m);
}

// ------------------------------------------------------------------------------------------------------------------
// Round 3: selection from a CONFLICT MATRIX (replaces k_r2_prep + k_r2_select; BSLV_R2_MIS=0 brings those back).
//
// The local minima of one random order are a small part of a maximal independent set (measured on an S-mid batch of 553
// cuts: 129 rounds against 59 for a maximal set per round).  Finding the maximal set with the element / edge passes would
// take one pass per Luby iteration; instead the conflict relation itself is written down, as a bit matrix over the cuts of
// the chunk (<= 1024 cuts: 128 KB, it fits the LDS of one CU), and ONE workgroup iterates "local minima of the candidates,
// drop them and their neighbours" to the end in LDS:
//   k_r2_minit    every round: every pair of alive cuts that meets on a hot element or across a hot edge (row ORs: every toucher
//                 of an element gets the element's whole touch mask -- no pair enumeration), live MINUS elements per cut
//   k_r2_select3  the maximal independent set of the alive cuts that still have a MINUS element, ranks, bookkeeping; hands the
//                 matrix and the counts back zeroed
// (A matrix kept across the rounds and extended by the new edges of each round was tried first: conflicts through elements that
// have left stay in it, after a few dozen rounds of a chunk that reworks its whole neighbourhood nearly every pair is marked,
// and extending it per adjacent pair costs more than writing it afresh.)
// element-major copy of the class words of the hot elements at the start of a chunk + which words hold a touch (wm)
__global__ __launch_bounds__(PB) void k_r2_words3(PolyView P, const unsigned long long *__restrict__ words, int nw, int nv, unsigned long long *__restrict__ hw, unsigned *__restrict__ wm)
{
    const int idx = blockIdx.x * PB + threadIdx.x;
    if (idx >= vm_count(P, nv)) return;
    const int i = vm_id(P, idx);
    unsigned m = 0u;
    for (int w = 0; w < nw; w++) {
        const unsigned long long word = r2_pack(words[(size_t)w * P.cap + i]);
        hw[(size_t)i * nw + w] = word;
        if (r2_touch32(word)) m |= 1u << w;
    }
    wm[i] = m;
}
// k_r2_minit: every workgroup gathers the conflicts of ITS items in a private copy of the matrix in LDS (Bc x nw words, at most
// 128 KB: LDS atomics, no traffic) and ORs the non-zero words into the matrix in global memory at the end.  Writing the rows in
// global memory directly -- a relaxed load and, where bits were missing, an atomic OR per (toucher, class word), chains of L2 round
// trips on a few hot rows -- cost 106 us per round with one thread per (item, class word), 190 us with one thread per item and a
// second launch for the items with many touches, and 1.8 ms with one thread per item alone (the edges of an extreme direction that
// lies on the plane of a hundred cuts: thousands of edges with 10^4 row words each; in LDS those are a few microseconds).
// dynamic LDS: Ml[Bc * (nw + 1)] | cnt[Bc] | alive[nw]
// the touch masks of an element with at most 4 class words that hold a touch: all four words are fetched at once (independent
// loads; a loop over the set bits of wi is a chain of dependent memory latencies)
struct R2T4 { unsigned t[4], m[4]; int w[4]; };          // per class word that holds a touch: the alive touchers (MINUS or ZERO), the alive MINUS ones
__device__ __forceinline__ R2T4 r2_touch4(const unsigned long long *__restrict__ hw, int nw, int i, unsigned wi, const unsigned *alive)
{
    R2T4 r;
    unsigned long long raw[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { r.w[k] = wi ? __ffs((int)wi) - 1 : -1; wi &= wi - 1; }
#pragma unroll
    for (int k = 0; k < 4; k++) raw[k] = r.w[k] >= 0 ? hw[(size_t)i * nw + r.w[k]] : 0ull;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.t[k] = r.w[k] >= 0 ? (r2_touch32(raw[k]) & alive[r.w[k]]) : 0u; r.m[k] = r.w[k] >= 0 ? (r2_minus32(raw[k]) & alive[r.w[k]]) : 0u; }
    return r;
}
// every cut of the masks a[] conflicts with every cut of the masks b[] (both with at most 4 words): row[cut of a] |= b
__device__ __forceinline__ void r2_cross4(const unsigned (&a)[4], const int (&aw)[4], const unsigned (&b)[4], const int (&bw)[4], int ld, unsigned *Ml)
{
#pragma unroll
    for (int ka = 0; ka < 4; ka++) {
        unsigned t = a[ka];
        while (t) {
            const int c = aw[ka] * 32 + __ffs((int)t) - 1;
            t &= t - 1;
#pragma unroll
            for (int kb = 0; kb < 4; kb++) if (b[kb]) { unsigned *w = &Ml[c * ld + bw[kb]]; if (b[kb] & ~*w) atomicOr(w, b[kb]); }
        }
    }
}
// The conflict relation: two cuts conflict only when a MINUS element is involved -- an element that is MINUS for one and non-PLUS
// for the other, or an edge from a MINUS element of one to a non-PLUS element of the other (r2_give).  Elements that are merely ON
// the planes of several cuts (the extreme directions of an upper image for most cuts of a covering problem) and edges between such
// elements do not separate cuts: see "Elements shared by the cuts of a round" below.  (The strict relation of rounds 2-3 -- any
// non-PLUS element in common -- was slower on whole runs with the same final sets and has been removed.)
// The rows of the alive MINUS cuts of element x get the alive non-PLUS cuts of element y (y = x: the element itself, else
// its neighbour across an edge).  ONE direction only -- the rows of the cuts that own a MINUS element; k_r2_select3 makes the
// relation symmetric in LDS.  (Writing both directions here cost what the strict relation costs: every edge of an extreme direction
// that is ON the planes of a hundred cuts touched a hundred rows; this way such an edge costs one row per MINUS cut of its other end.)
__device__ __forceinline__ void r2_give(const unsigned long long *__restrict__ hw, int nw, int x, unsigned wx, int y, unsigned wy, const unsigned *alive, unsigned *Ml, int ld)
{
    while (wx) {
        const int wa = __ffs((int)wx) - 1;
        wx &= wx - 1;
        const unsigned mn = r2_minus32(hw[(size_t)x * nw + wa]) & alive[wa];
        if (!mn) continue;
        unsigned m2 = wy;
        while (m2) {
            const int wb = __ffs((int)m2) - 1;
            m2 &= m2 - 1;
            const unsigned tb = r2_touch32(hw[(size_t)y * nw + wb]) & alive[wb];
            if (!tb) continue;
            unsigned t = mn;
            while (t) {
                const int a = wa * 32 + __ffs((int)t) - 1;
                t &= t - 1;
                unsigned *w = &Ml[a * ld + wb];
                if (tb & ~*w) atomicOr(w, tb);
            }
        }
    }
}
constexpr int R2_QCAP = 3072;                          // items of one workgroup that are left to whole waves
__global__ __launch_bounds__(1024) void k_r2_minit(PolyView P, const unsigned long long *__restrict__ hw, const unsigned *__restrict__ wm, int nw, int Bc, const RState *st,
                                                   const int2 *__restrict__ E, const unsigned *__restrict__ alive_g, unsigned *M, int *mcnt, const int *__restrict__ tc, RState *st_w,
                                                   int ne_ub, int nel_ub, unsigned long long *probe)
{
    extern __shared__ unsigned r2_lds[];
    __shared__ int q_item[R2_QCAP];
#define MINIT_STAMP(k) do { if (probe) { __syncthreads(); if (threadIdx.x == 0) probe[blockIdx.x * 16 + (k)] = wall_clock64(); } } while (0)
    MINIT_STAMP(0);
    __shared__ int q_n;
    __shared__ int q_rows[16][64];                 // per wave: the rows of one queued item, the non-empty words of what they get
    __shared__ unsigned q_tw[16][32], q_tv[16][32];
    __shared__ int q_nr[16];
    const int ld = nw + 1;                           // (rows one word apart in the banks: the queued items write a column of rows at a time)
    unsigned *Ml = r2_lds, *cnt = r2_lds + Bc * ld, *alive = cnt + Bc;
    if (r2_halted(st)) return;
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int k = tid; k < Bc * ld + Bc; k += nthr) r2_lds[k] = 0u;
    for (int w = tid; w < nw; w += nthr) alive[w] = alive_g[w];
    if (tid == 0) q_n = 0;
    __syncthreads();
    MINIT_STAMP(1);
    const int nv = st->nv, ne = st->ne, nel = vm_count(P, nv);
    // queued before the host knew the sizes: the launch was sized for ne_ub edges and nel_ub elements (every kernel of the round shares the bound)
    if (blockIdx.x == 0 && tid == 0 && (ne > ne_ub || nel > nel_ub)) st_w->halt = 2;
    // an item with many touches (an edge of an extreme direction that lies on the plane of a hundred cuts) is thousands of dependent
    // LDS operations for one thread -- 190 us per launch, whatever the number of workgroups -- and a microsecond for a wave
    // items are dealt to the workgroups a wave (64 consecutive items) at a time, round robin: the few thousand edges of one extreme
    // direction sit next to each other in the list, and a workgroup that got them all would still be at them when the others are done
    const int nwaves = nthr >> 6, gw = (tid >> 6) * (int)gridDim.x + (int)blockIdx.x, stride = nwaves * (int)gridDim.x * 64;
    for (int it = gw * 64 + (tid & 63); it < ne + nel; it += stride) {
        if (it < ne) {
            const int2 ed = E[it];
            const bool hu = ed.x >= P.nv_base || tc[ed.x] > 0, hv2 = ed.y >= P.nv_base || tc[ed.y] > 0;
            if (!(hu && hv2)) continue;
            const unsigned wu = wm[ed.x], wv = wm[ed.y];
            if (!wu || !wv) continue;
            if (__popc(wu) <= 4 && __popc(wv) <= 4) {          // rows of the MINUS cuts of either end <- the non-PLUS cuts of the other end
                const R2T4 A = r2_touch4(hw, nw, ed.x, wu, alive), B2 = r2_touch4(hw, nw, ed.y, wv, alive);
                if (A.m[0] | A.m[1] | A.m[2] | A.m[3]) r2_cross4(A.m, A.w, B2.t, B2.w, ld, Ml);
                if (B2.m[0] | B2.m[1] | B2.m[2] | B2.m[3]) r2_cross4(B2.m, B2.w, A.t, A.w, ld, Ml);
                continue;
            }
            const int k = atomicAdd(&q_n, 1);
            if (k < R2_QCAP) { q_item[k] = it; continue; }
            r2_give(hw, nw, ed.x, wu, ed.y, wv, alive, Ml, ld); r2_give(hw, nw, ed.y, wv, ed.x, wu, alive, Ml, ld);
        } else {
            const int i = vm_id(P, it - ne);
            const unsigned wi = wm[i];
            if (!wi || !(P.flag[i] & F_USED)) continue;
            unsigned m = wi, anym = 0u;
            while (m) {
                const int w = __ffs((int)m) - 1;
                m &= m - 1;
                unsigned mi = r2_minus32(hw[(size_t)i * nw + w]) & alive[w];
                anym |= mi;
                while (mi) { const int b = __ffs((int)mi) - 1; mi &= mi - 1; atomicAdd(&cnt[w * 32 + b], 1u); }
            }
            if (!anym) continue;
            if (__popc(wi) <= 4) { const R2T4 A = r2_touch4(hw, nw, i, wi, alive); r2_cross4(A.m, A.w, A.t, A.w, ld, Ml); continue; }
            const int k = atomicAdd(&q_n, 1);
            if (k < R2_QCAP) { q_item[k] = -1 - i; continue; }
            r2_give(hw, nw, i, wi, i, wi, alive, Ml, ld);
        }
    }
    __syncthreads();
    MINIT_STAMP(2);
    if (probe && tid == 0) probe[blockIdx.x * 16 + 6] = (unsigned long long)q_n;
    {
        // The queued items.  What they cost is their row operations -- an edge whose ends are MINUS for dozens of cuts each (the cuts of
        // a batch come in families of near-parallel planes) is a hundred rows to OR a mask into, each an LDS read, a compare and now and
        // then an atomic: ~6 us per item when a wave takes the rows one after the other (round 0 of a chunk: 500 items per workgroup,
        // 200 us, three quarters of the kernel).  A row is at most 32 words, so the two halves of the wave take different rows, two
        // each per trip: four rows in flight.  The lanes resolve the entries of a wave side by side (one chain of loads for all of
        // them) and the class words of item k + 1 are on their way while item k is written.  Entries are dealt to the waves
        // round robin: neighbours in the queue are edges of the same element and equally heavy.
        const int nq = min(q_n, R2_QCAP), lane = tid & 63, wv = tid >> 6, nwv = nthr >> 6, wl = lane & 31, half = lane >> 5;
        const unsigned al = wl < nw ? alive[wl] : 0u;
        for (int base = wv; base < nq; base += nwv * 64) {
            const int cntb = min(64, (nq - base + nwv - 1) / nwv);      // entries base, base + nwv, ... of this wave
            int x = 0, y = 0;
            unsigned wx = 0u, wy = 0u;
            if (lane < cntb) {
                const int code = q_item[base + lane * nwv];
                if (code >= 0) { const int2 ed = E[code]; x = ed.x; y = ed.y; } else { x = -1 - code; y = x; }
                wx = wm[x];
                wy = x == y ? wx : wm[y];
            }
            auto fetch = [&](int k, unsigned long long &rx, unsigned long long &ry) {      // (both halves hold the same words)
                const int xx = __shfl(x, k, WAVE), yy = __shfl(y, k, WAVE);
                const unsigned a = (unsigned)__shfl((int)wx, k, WAVE), b2 = (unsigned)__shfl((int)wy, k, WAVE);
                rx = (wl < nw && ((a >> wl) & 1u)) ? hw[(size_t)xx * nw + wl] : 0ull;
                ry = xx == yy ? rx : ((wl < nw && ((b2 >> wl) & 1u)) ? hw[(size_t)yy * nw + wl] : 0ull);
            };
            // the rows of the cuts in `from` get the cuts in `to` (lane & 31 = class word in both; both halves hold the same).  The kernel
            // is bound by the instructions its waves issue (16 waves on the 4 SIMDs of a CU: one instruction per wave every ~16 cycles),
            // and a row at a time -- a read, a compare, an OR by the few lanes whose word of `to` is not empty -- was ~38 instructions per
            // row: 6-8 us for an item of 28 rows, 200 us for the 500 items a workgroup meets in round 0 of a chunk, three quarters of the
            // kernel.  So the (row, word of `to`) pairs are spread over all 64 lanes: the rows and the non-empty words of `to` are listed in
            // a few words of LDS per wave, lane l takes word l mod ntp of row l / ntp (ntp = the words of `to`, rounded up to a power of
            // two), 64 / ntp rows per trip, ORs without reading first and waits for nothing.
            auto give = [&](unsigned from, unsigned to) {
                const unsigned fm = (unsigned)__ballot(from != 0u), tm = (unsigned)__ballot(to != 0u);      // (the low halves: the words)
                if (fm == 0u || tm == 0u) return;
                const int nt = __popc(tm);
                if (half == 0 && to) { const int r = __popc(tm & ((1u << wl) - 1u)); q_tw[wv][r] = (unsigned)wl; q_tv[wv][r] = to; }
                int sh = 0;
                while ((1 << sh) < nt) sh++;
                const int myw = lane & ((1 << sh) - 1), rsub = lane >> sh, rpp = 64 >> sh;
                // (ranks of the rows: a ticket per class word from a counter of the wave -- one trip to the LDS; their order does not matter)
                if (lane == 0) q_nr[wv] = 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int excl = (half == 0 && from) ? atomicAdd(&q_nr[wv], __popc(from)) : 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int nr = q_nr[wv];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const unsigned myv = myw < nt ? q_tv[wv][myw] : 0u;
                const int mywb = myw < nt ? (int)q_tw[wv][myw] : 0;
                for (int lo = 0; lo < nr; lo += 64) {
                    if (half == 0) {
                        unsigned t = from;
                        int r = excl - lo;
                        while (t) { const int bq = __ffs((int)t) - 1; t &= t - 1; if (r >= 0 && r < 64) q_rows[wv][r] = wl * 32 + bq; r++; }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const int n = min(64, nr - lo);
                    for (int rb = 0; rb < n; rb += rpp) {
                        const int ri = rb + rsub;
                        if (ri < n && myv) atomicOr(&Ml[q_rows[wv][ri] * ld + mywb], myv);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            };
            unsigned long long rx, ry, nrx = 0ull, nry = 0ull;
            unsigned long long tq0 = probe ? wall_clock64() : 0ull, t_give = 0ull, t_wait = 0ull;
            fetch(0, rx, ry);
            if (probe) { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t = wall_clock64(); if (lane == 0) atomicAdd(&probe[blockIdx.x * 16 + 8], t - tq0); tq0 = t; }
            for (int k = 0; k < cntb; k++) {
                const bool same = __shfl(x, k, WAVE) == __shfl(y, k, WAVE);
                if (k + 1 < cntb) fetch(k + 1, nrx, nry);
                const unsigned long long tg0 = probe ? wall_clock64() : 0ull;
                const unsigned tx = r2_touch32(rx) & al, ty = r2_touch32(ry) & al;
                // one direction: the rows of the MINUS cuts (k_r2_select3 mirrors them)
                give(r2_minus32(rx) & al, ty);
                if (!same) give(r2_minus32(ry) & al, tx);
                if (probe) {
                    __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): the LDS operations are through
                    const unsigned long long tg1 = wall_clock64();
                    __builtin_amdgcn_s_waitcnt(0);           // and the class words of the next item
                    const unsigned long long tg2 = wall_clock64();
                    t_give += tg1 - tg0; t_wait += tg2 - tg1;
                }
                rx = nrx; ry = nry;
            }
            if (probe && lane == 0) { atomicAdd(&probe[blockIdx.x * 16 + 9], t_give); atomicAdd(&probe[blockIdx.x * 16 + 10], t_wait); atomicMax(&probe[blockIdx.x * 16 + 11], t_give + t_wait); }
        }
    }
    __syncthreads();
    MINIT_STAMP(3);
    int nzw = 0;
    {                                              // (by rows, a thread per word: k / nw and k % nw for a flat index were 20 us of integer division)
        const int w = tid & 31, rstep = nthr >> 5;
        for (int r0 = tid >> 5; r0 < Bc && w < nw; r0 += 4 * rstep) {
            unsigned v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int r = r0 + u * rstep; v[u] = r < Bc ? Ml[r * ld + w] : 0u; }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (v[u]) { (void)__hip_atomic_fetch_or(&M[(r0 + u * rstep) * nw + w], v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); nzw++; }      // (no return value used: nothing waits for it)
        }
    }
    for (int k = tid; k < Bc; k += nthr) { const unsigned c = cnt[k]; if (c) (void)__hip_atomic_fetch_add(&mcnt[k], (int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    if (probe) { atomicAdd(&probe[blockIdx.x * 16 + 7], (unsigned long long)nzw); __threadfence(); }
    MINIT_STAMP(4);
#undef MINIT_STAMP
}
// One workgroup, one thread per cut (Bc <= 1024).  Dynamic LDS: the rows of the alive cuts, transposed (word-major, stride
// R2_MLD: consecutive cuts in consecutive banks).  Priority = index (the host shuffles the chunk).
constexpr int R2_MAXC = 1024, R2_MLD = R2_MAXC + 1;
__global__ __launch_bounds__(1024) void k_r2_select3(int Bc, int nw, unsigned *alive, unsigned *alive_prev, unsigned *M, int *mcnt,
                                                     int *selmap, int *sel, int *order, int *rcflag, RState *st, unsigned *selw_g, int spec)
{
    extern __shared__ unsigned r2m[];
    __shared__ unsigned s_alive[32], s_cand[32], s_new[32];
    __shared__ Tri lds[16];
    if (r2_halted(st)) return;                     // (queued behind a round the host has to deal with first; k_r2_minit did nothing either)
    const int tid = threadIdx.x, k = tid, lane = tid & 63, wv = tid >> 6;
    if (tid < 32) { s_alive[tid] = tid < nw ? alive[tid] : 0u; s_cand[tid] = 0u; s_new[tid] = 0u; }
    __syncthreads();
    {
        // the matrix into LDS (transposed), four words per thread in flight; (row, word) of a flat index advance without a division
        const int total = Bc * nw, q = 1024 / nw, rm = 1024 - q * nw;
        int kk = tid / nw, w = tid - kk * nw;
        for (int idx = tid; idx < total; idx += 4096) {
            unsigned v[4]; int at[4]; bool al[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int id = idx + u * 1024;
                al[u] = id < total && ((s_alive[kk >> 5] >> (kk & 31)) & 1u);
                at[u] = w * R2_MLD + kk;
                v[u] = al[u] ? M[id] : 0u;
                kk += q; w += rm;
                if (w >= nw) { w -= nw; kk++; }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (al[u]) { r2m[at[u]] = v[u]; M[idx + u * 1024] = 0u; }      // (k_r2_minit of the next round starts from zero)
        }
    }
    const bool a = k < Bc && ((s_alive[k >> 5] >> (k & 31)) & 1u);
    const int mc = a ? mcnt[k] : 0;
    if (a) mcnt[k] = 0;
    bool cand = a && mc > 0;
    const bool red = a && mc <= 0;
    {
        const unsigned long long bc = __ballot(cand);
        if (lane == 0) { s_cand[2 * wv] = (unsigned)bc; s_cand[2 * wv + 1] = (unsigned)(bc >> 32); }
    }
    __syncthreads();
    // k_r2_minit wrote the relation one way round -- into the rows of the cuts that own a MINUS element: make it symmetric
    if (a) for (int w = 0; w < nw; w++) {
        unsigned bits = r2m[w * R2_MLD + k];
        while (bits) {
            const int j = w * 32 + __ffs((int)bits) - 1;
            bits &= bits - 1;
            atomicOr(&r2m[(k >> 5) * R2_MLD + j], 1u << (k & 31));
        }
    }
    __syncthreads();
    bool selected = false;
    const int wk = k >> 5;
    const unsigned below = (1u << (k & 31)) - 1u;
    for (int it = 0; it < 1024; it++) {
        // local minima of the candidates ...
        bool dom = false;
        if (cand) {
            for (int w = 0; w < wk; w++) dom |= (r2m[w * R2_MLD + k] & s_cand[w]) != 0u;
            dom |= (r2m[wk * R2_MLD + k] & s_cand[wk] & below) != 0u;
        }
        const bool pick = cand && !dom;
        const unsigned long long bn = __ballot(pick);
        __syncthreads();                                    // (every read of s_cand is done)
        if (lane == 0) { s_new[2 * wv] = (unsigned)bn; s_new[2 * wv + 1] = (unsigned)(bn >> 32); }
        __syncthreads();
        // ... leave the candidates together with their neighbours
        bool blocked = false;
        if (cand && !pick) for (int w = 0; w < nw; w++) blocked |= (r2m[w * R2_MLD + k] & s_new[w]) != 0u;
        selected |= pick;
        cand = cand && !pick && !blocked;
        const unsigned long long bc = __ballot(cand);
        if (lane == 0) { s_cand[2 * wv] = (unsigned)bc; s_cand[2 * wv + 1] = (unsigned)(bc >> 32); }
        if (!__syncthreads_or(cand ? 1 : 0)) break;
    }
    const int napplied0 = st->napplied;
    const int s = selected, r = red, keep = a && !selected && !red;
    Tri tot;
    const Tri ex = block_exscan(Tri{s, r, keep}, &tot, lds);
    if (k < Bc) {
        selmap[k] = s ? ex.a : -1;
        if (s) { sel[ex.a] = k; order[napplied0 + ex.a] = k; rcflag[k] = 0; }
        if (r) rcflag[k] = 1;
    }
    const unsigned long long ba = __ballot(a), bk = __ballot(keep), bs = __ballot(s);
    if (lane == 0) {
        const int w0 = 2 * wv;
        if (w0 < nw) { alive_prev[w0] = (unsigned)ba; alive[w0] = (unsigned)bk; selw_g[w0] = (unsigned)bs; }
        if (w0 + 1 < nw) { alive_prev[w0 + 1] = (unsigned)(ba >> 32); alive[w0 + 1] = (unsigned)(bk >> 32); selw_g[w0 + 1] = (unsigned)(bs >> 32); }
    }
    if (tid == 0) {
        st->round += 1;
        st->S = tot.a;
        st->rank_base = st->nranks;
        st->nranks += tot.a;
        st->napplied = napplied0 + tot.a;
        st->nredundant += tot.b;
        st->nalive = tot.c;
        st->stuck = (tot.a == 0 && tot.b == 0 && tot.c > 0) ? 1 : 0;
        st->go = 0; st->declined = 0; st->epairs = 0; st->eover = 0; st->k2abort = 0; st->ncross = 0; st->nzero = 0;
        if (spec && tot.a == 0) st->halt = 3;            // (nothing selected: the buffers do not change over, which a round queued behind assumed)
    }
}
// ---- Elements shared by the cuts of a round (round 4) -------------------------------------------------------------------------
// With the relaxed conflict relation (k_r2_minit) the selected cuts of a round may have elements in common that are ON
// the plane of each of them (class ZERO), and edges may join an on-plane element of one cut to an on-plane element of another.  No
// neighbour of a shared element is MINUS for any of its cuts (that would be a conflict), so every one of its cuts merely TOUCHES the
// polyhedron there: applied one after the other, in rank order, each would append its facet to the element's list and filter
// nothing (bslv_poly.c:634-652 keeps the facets shared with a PLUS neighbour; a facet whose neighbours are all ON the cut's plane
// lies IN that plane, i.e. the cut would repeat it and cut nothing), would drop the element's edges to the other elements on its plane
// and have them re-derived by its adjacency prune.  The round does the same in one pass:
//   owners of a ZERO element = the selected cuts it is ZERO for, from its class words (hw, wm) and the selection (selw, selmap)
//   cutof[i] = s >= 0   MINUS or ZERO for the one selected cut s (as before: list filtered by the keep marks, facet of s appended)
//   cutof[i] = -1 - k   ZERO for k >= 2 selected cuts: the whole list is kept and the k facets are appended in rank order
//   an edge between two ZERO elements is dropped (and re-derived by a prune) iff the two have an owner in common; otherwise it
//   stays, and each single-owner end keeps the facets it shares with the other end (which is PLUS for its owner): k_flags2
//   an element is a member of the prune of EACH of its owners; a pair of members with several owners in common is emitted by the
//   prune of the LAST of them (the one that would have the final word one cut at a time): k2_fused_body<true>, `later`
// class and owner(s) of every hot element for the selected cuts of the round (selw: their bit mask).  The selected cuts are
// independent: a MINUS element is touched by one of them only; a ZERO element may be ZERO for several (see above).
__global__ __launch_bounds__(PB) void k_r2_assign3(PolyView P, const unsigned long long *__restrict__ words, const unsigned *__restrict__ wm, int nw, const RState *st,
                                                   const unsigned *__restrict__ selw_g, const int *__restrict__ selmap, int *cutof, int *counters, int *zlist)
{
    __shared__ unsigned selw[32];
    if (r2_halted(st)) return;
    if (threadIdx.x < 32) selw[threadIdx.x] = (int)threadIdx.x < nw ? selw_g[threadIdx.x] : 0u;
    __syncthreads();
    const int idx = blockIdx.x * PB + threadIdx.x;
    int isminus = 0, iszero = 0, zlen = 0;
    if (idx < vm_count(P, st->nv)) {
        const int i = vm_id(P, idx);
        signed char c = 2;
        int s = -1;
        if (P.flag[i] & F_USED) {
            c = 1;
            unsigned m = st->S > 0 ? wm[i] : 0u;
            int nown = 0, ofirst = -1, ominus = -1;
            while (m) {
                const int w = __ffs((int)m) - 1;
                m &= m - 1;
                if (!selw[w]) continue;
                const unsigned long long word = words[(size_t)i * nw + w];
                const unsigned t = r2_touch32(word) & selw[w];
                if (!t) continue;
                const unsigned mn = r2_minus32(word) & selw[w];
                if (mn) ominus = w * 32 + __ffs((int)mn) - 1;
                if (ofirst < 0) ofirst = w * 32 + __ffs((int)t) - 1;
                nown += __popc(t);
            }
            if (ominus >= 0) { c = -1; s = selmap[ominus]; isminus = 1; }
            else if (nown > 0) {
                c = 0; iszero = 1;
                s = nown == 1 ? selmap[ofirst] : -1 - nown;
                zlen = zero_room(P, i, nown);
                // on-plane elements with long lists and ONE owner get a row of facet stamps (ZMarks), as in k_classify; shared ones keep their whole list
                if (nown == 1 && P.inc_len[i] > LONGN) { const int k = atomicAdd(&counters[3], 1); if (k < ZMAX) zlist[k] = i; }
            }
        }
        P.cls[i] = c;
        cutof[i] = s;
    }
    const unsigned long long bm = __ballot(isminus), bz = __ballot(iszero);
    if (bz) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) zlen += __shfl_xor(zlen, o, WAVE);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bm) atomicAdd(&counters[0], __popcll(bm));
        if (bz) { atomicAdd(&counters[1], __popcll(bz)); atomicAdd(&counters[2], zlen); }
    }
}
// classes of the vertices a round created against the alive cuts of the chunk + which of their words hold a touch (wm) + their
// MINUS marks (mcnt).  A workgroup takes PB / nwp vertices at a time (nwp = nw rounded up to a power of two: the lanes of one
// vertex are neighbours in a wave), the workgroups stride over all new vertices: whatever a round creates is covered by ONE launch.
// The next round's k_r2_minit is the first to read these words (k_r2_k2emit reads none).
// block / nblocks: this workgroup's number among those that classify; nthr: its threads (PB in k_r2_classify3, K2T when it rides along
// with the prunes in k_r2_prune_classify).  No barrier in here: workgroups of another kernel call it from a role branch.
// LDSH: `hps` is the LDS image of the chunk's halfspaces that r2_stage_hps made (component-major, the class word fastest: the lanes
// of a vertex read consecutive doubles); the operands, the order of the fma over k and the thresholds are those of the global-memory
// path, so the class words are bit-identical.
__device__ __forceinline__ int r2_hps_lds_stride(int nw) { return nw | 1; }      // odd: the staging stores of a wave spread over the banks
__device__ __forceinline__ void r2_stage_hps(const double *__restrict__ hps, int B, int nw, int d, double *lh)
{
    const int nwl = r2_hps_lds_stride(nw), n = B * (d + 3);
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int c = e / (d + 3), k = e - c * (d + 3);
        lh[((c & 31) * (d + 3) + k) * nwl + (c >> 5)] = hps[e];
    }
}
template <int D, bool LDSH = false>
__device__ __forceinline__ void r2_classify3_body(const PolyView &P, const double *__restrict__ hps, int B, int nw, int nwp, const RState *st, const unsigned *__restrict__ alive,
                                                  unsigned long long *__restrict__ hw, unsigned *__restrict__ wm, int *mcnt, int block, int nblocks, int nthr, int packed = 1)
{
    if (!st->go || r2_halted(st)) return;
    const int hstride = LDSH ? r2_hps_lds_stride(nw) : 1;
    const int vpb = nthr / nwp, w = threadIdx.x & (nwp - 1), lv = threadIdx.x / nwp, lane = threadIdx.x & 63;
    const int ncross = st->ncross, first = st->nv_next - ncross;
    const int d = D > 0 ? D : P.d;
    const unsigned aw = w < nw ? alive[w] : 0u;
    for (int base = block * vpb; base < ncross; base += nblocks * vpb) {
        const bool act = base + lv < ncross;
        const int i = first + base + lv;
        unsigned touch = 0u;
        if (act && aw) {
            double x[D > 0 ? D : MAXD];
#pragma unroll
            for (int k = 0; k < (D > 0 ? D : MAXD); k++) x[k] = k < d ? P.X[(size_t)k * P.cap + i] : 0.0;
            const bool ideal = P.flag[i] & F_IDEAL;
            const int bend = min(32, B - w * 32);
            unsigned plus = 0, notminus = 0;
            for (int bb = 0; bb < bend; bb++) {
                // component k of halfspace w * 32 + bb is h[k * hstride]
                const double *h = LDSH ? hps + (size_t)bb * (d + 3) * hstride + w : hps + (size_t)(w * 32 + bb) * (d + 3);
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < (D > 0 ? D : MAXD); k++) if (k < d) s = fma(h[k * hstride], x[k], s);
                const double hi = ideal ? 0.0 + POLY_EPS : h[(d + 1) * hstride], lo = ideal ? 0.0 - POLY_EPS : h[(d + 2) * hstride];
                plus |= (unsigned)(s > hi) << bb;
                notminus |= (unsigned)(s > lo) << bb;
            }
            const unsigned valid = bend == 32 ? 0xFFFFFFFFu : ((1u << bend) - 1u);
            const unsigned lowb = (plus | ~notminus) & valid, highb = notminus & valid;
            // conflict-matrix rounds: the two masks (r2_pack of the classes); the local-minima rule of round 2 (r2_mis off) reads two-bit classes,
            // as k_r2_words copies them -- until the second session of round 4 this wrote the masks for both, and that arm classified its new
            // vertices wrongly (nothing tested it; bench.py's "rounds 1-2 rule" leg reported 0 LPs/s)
            hw[(size_t)i * nw + w] = packed ? (unsigned long long)(lowb ^ highb) | ((unsigned long long)(lowb & ~highb) << 32) : spread32(lowb) | (spread32(highb) << 1);
            touch = (lowb ^ highb) & aw;
            unsigned mi = mcnt ? (lowb & ~highb & aw) : 0u;
            while (mi) { const int b = __ffs((int)mi) - 1; mi &= mi - 1; atomicAdd(&mcnt[w * 32 + b], 1); }
        }
        const unsigned long long bt = __ballot(touch != 0u);
        if (act && w == 0) wm[i] = (unsigned)((bt >> (lane & ~(nwp - 1))) & (nwp == 32 ? 0xFFFFFFFFull : ((1ull << nwp) - 1ull)));
    }
}
template <int D>
__global__ __launch_bounds__(PB) void k_r2_classify3(PolyView P, const double *__restrict__ hps, int B, int nw, int nwp, const RState *st, const unsigned *__restrict__ alive,
                                                     unsigned long long *__restrict__ hw, unsigned *__restrict__ wm, int *mcnt, int packed)
{
    r2_classify3_body<D>(P, hps, B, nw, nwp, st, alive, hw, wm, mcnt, (int)blockIdx.x, (int)gridDim.x, PB, packed);
}
// A round's prunes and the classification of its new vertices in ONE launch (BSLV_R2_RIDE, the default): the two do not depend on
// each other -- a prune reads incidence lists, owners and the on-plane list and writes mem_g / adj_g / cnt_g / nm_g, the
// classification writes only the class words (hw, wm) of the new vertices, which nothing reads before the next round's k_r2_minit.
// The roles come from the DEVICE's S (the grid is sized for the S_ub the host knows, up to the whole chunk), so that the
// classification is dispatched directly behind the real prunes:
//   blockIdx.x < S            the prune of selected cut blockIdx.x (k2_fused_body<true>, as k2_fused_t<true> runs it)
//   S <= blockIdx.x < S + G   workgroup blockIdx.x - S of G that classify; the body strides over the new vertices, any G >= 1 covers them
//   the rest                  returns
// Workgroup 0 enters the prune body whatever S is: it clears the other round's ticket there, and the body returns at once when
// the round does not go ahead or S is 0.  r2_classify3_body has no barrier, so the (workgroup-uniform) role branch is safe.
template <int D>
__global__ __launch_bounds__(K2T) void k_r2_prune_classify(PolyView P, int *members, int *fcount, int *flocal, int lds_words, int2 *E, Tri *totals, Mail *mail, unsigned long long *dbg,
                                                           int *abort_flag, Hp hn, K2V2 V, const double *__restrict__ hps, int B, int nw, int nwp, const unsigned *__restrict__ alive,
                                                           unsigned long long *__restrict__ hw, unsigned *__restrict__ wm, int G, int nthr, int packed, int hps_lds)
{
    extern __shared__ unsigned long long k2_dyn[];
    const int S = max(V.st->S, 0), H = V.helpers, b = (int)blockIdx.x;
    if (b >= S + H) {
        if (b < S + H + G) {
            // hps_lds: the workgroup has a CU's LDS to itself (the dynamic LDS of the prunes), so when the chunk's halfspaces fit there
            // (uniform over the launch) it stages them once with coalesced loads and classifies from the image -- read from global
            // memory, every load of a wave touches 32 cache lines for 8 bytes each.  All threads stage, and meet at the one barrier
            // (the conditions are those under which r2_classify3_body returns at once: uniform).
            const int d = D > 0 ? D : P.d;
            const bool staged = hps_lds && (long long)r2_hps_lds_stride(nw) * 32 * (d + 3) <= (long long)lds_words && V.st->go && !r2_halted(V.st);
            if (staged) {
                r2_stage_hps(hps, B, nw, d, (double *)k2_dyn);
                __syncthreads();
            }
            // only the first nthr threads (whole waves) of a classifying workgroup work: the classification is bound by the loads of the
            // halfspaces per CU (every lane of a wave reads another halfspace), so it wants few waves on MANY CUs, and a workgroup of this launch
            // has a CU to itself -- with all K2T threads at work a round's new vertices sat on 57 CUs, 16 waves each, and took twice the prunes' time
            if ((int)threadIdx.x < nthr) {
                if (staged) r2_classify3_body<D, true>(P, (const double *)k2_dyn, B, nw, nwp, V.st, alive, hw, wm, (int *)nullptr, b - S - H, G, nthr, packed);
                else r2_classify3_body<D>(P, hps, B, nw, nwp, V.st, alive, hw, wm, (int *)nullptr, b - S - H, G, nthr, packed);
            }
        }
        if (b > 0) return;
    }
    // b < S: prune b; S <= b < S + H: helper b - S of the pool (k2v2_assign).  Workgroup 0 is never a helper: with S = 0 it enters as a prune
    k2_fused_body<true>(P, members, 0, 0, 0, fcount, flocal, lds_words, E, 0, (int *)nullptr, totals, mail, 0, dbg, (const CutDev *)nullptr, abort_flag, (int *)nullptr, hn, (int *)nullptr,
                        (int *)nullptr, V, b >= S && b > 0 ? b - S : -1);
}

// The cuts still alive when a chunk hands them back (bslv_poly_set_defer) WILL be applied, with a later batch: every element that is
// MINUS for one of them will be removed then.  It is marked as processed now, so that no batch in between spends an LP on it
// (whose cut would be a valid but needless refinement next to the waiting one).
__global__ __launch_bounds__(PB) void k_r2_mark_doomed(PolyView P, const unsigned long long *__restrict__ hw, const unsigned *__restrict__ wm, int nw, int nv,
                                                       const unsigned *__restrict__ alive, int *count)
{
    const int idx = blockIdx.x * PB + threadIdx.x;
    if (idx >= vm_count(P, nv)) return;
    const int i = vm_id(P, idx);
    const unsigned char fl = P.flag[i];
    if (!(fl & F_USED) || (fl & F_SLTN)) return;
    unsigned m = wm ? wm[i] : 0xFFFFFFFFu;
    bool doomed = false;
    for (int w = 0; w < nw && !doomed; w++) {
        if (!((m >> w) & 1u) || alive[w] == 0u) continue;
        const unsigned long long word = hw[(size_t)i * nw + w];      // (conflict-matrix rounds: packed masks; else the two-bit classes)
        doomed = ((wm ? r2_minus32(word) : compress32(word & ~(word >> 1))) & alive[w]) != 0u;
    }
    if (doomed) { P.flag[i] = fl | F_SLTN; atomicAdd(count, 1); }
}

// element-major copy of the class words of the hot elements at the start of a chunk
__global__ __launch_bounds__(PB) void k_r2_words(PolyView P, const unsigned long long *__restrict__ words, int nw, int nv, unsigned long long *__restrict__ hw)
{
    const long long t = (long long)blockIdx.x * PB + threadIdx.x;
    const int w = (int)(t % nw);
    const long long idx = t / nw;
    if (idx >= vm_count(P, nv)) return;
    const int i = vm_id(P, (int)idx);
    hw[(size_t)i * nw + w] = words[(size_t)w * P.cap + i];
}

// ordered emission of the adjacent pairs of every selected cut (cut by cut in selection order, pairs in lexicographic order
// of the member positions: what a sequence of k2_fused launches appends), commit of the round, mailbox
__global__ __launch_bounds__(K2T) void k_r2_k2emit(RState *st, const int *__restrict__ cnt_g, const int *__restrict__ nm_g, unsigned *__restrict__ adj_g,
                                                   const int *__restrict__ npart_g, const int *__restrict__ cntx_g, const int *__restrict__ mem_g, int adjw_cap, int2 *E, int *EP, int ecap, RState *mail, int seq)
{
    __shared__ Tri lds[16];
    __shared__ int s_carry;
    // (it reads no class words: the conflict matrix is rebuilt every round, there is nothing to add for the new edges here)
    const int S = st->S, s = blockIdx.x, tid = threadIdx.x;
    const int h2 = st->halt2;
    if (S <= 0 || !st->go || st->halt || (h2 != 0 && h2 != seq)) {
        if (s == 0 && tid == 0) rstate_publish(st, mail, seq);
        return;
    }
    // pairs of the cuts before this one, of all cuts; prunes that asked for their fallback count nothing here
    Tri part{0, 0, 0};
    // (a prune worked in parts: its own workgroup's pairs and, beside them, those of each further part)
    auto pairs_of = [&](int k) { int c = cnt_g[k]; if (c >= 0) for (int p = 1; p < npart_g[k]; p++) c += cntx_g[k * (K2_MAXPARTS - 1) + p - 1]; return c; };
    for (int k = tid; k < S; k += K2T) { const int c = pairs_of(k); if (c > 0) { part.b += c; if (k < s) part.a += c; } if (c < 0) part.c += 1; }
    part = block_sum(part, lds);
    const int ebase = st->ne_next, before = part.a, total = part.b;
    const bool over = (long long)ebase + total > ecap;
    if (s == 0 && tid == 0) {
        st->epairs = total; st->eover = over; st->k2abort = part.c;
        if (over || part.c > 0) st->halt2 = seq;
        if (!over) { st->nv = st->nv_next; st->ne = ebase + total; st->poolused = st->pool_next; }
        rstate_publish(st, mail, seq);
    }
    if (over || s >= S) return;
    const int cnt = pairs_of(s);
    if (cnt <= 0) return;
    const int nm = nm_g[s];
    const int nadjw = (int)(((long long)nm * (nm - 1) / 2 + 31) / 32);
    // The parts of a split prune OR their words into a bitmap that must be zero: the words go back to zero here, where they are read
    // for the last time (when the pairs did not fit, `over`, this kernel runs again on the same bitmaps and clears them then)
    unsigned *adj = adj_g + (size_t)s * adjw_cap;
    const int *mem = mem_g + (size_t)s * K2_MAXNM;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int w0 = 0; w0 < nadjw; w0 += K2T) {
        const int ww = w0 + tid;
        unsigned word = ww < nadjw ? adj[ww] : 0u;
        if (word) adj[ww] = 0u;
        Tri t{(int)__popc(word), 0, 0};
        Tri tot;
        const Tri ex = block_exscan(t, &tot, lds);
        int at = ebase + before + s_carry + ex.a;
        while (word) {
            const int bbit = __ffs((int)word) - 1;
            word &= word - 1;
            int i, j;
            pair_decode32(ww * 32 + bbit, nm, i, j);
            E[at] = int2{mem[i], mem[j]};
            if (EP) EP[at] = -1;
            at++;
        }
        __syncthreads();
        if (tid == 0) s_carry += tot.a;
        __syncthreads();
    }
}

// members of one selected cut, in slot order (on-plane elements, then the new vertices), for the multi-kernel prune
__global__ __launch_bounds__(1024) void k_r2_gather(PolyView P, const int *zsrc, int nzero, int nv0, int ncross, const int *cutof, int s, int *members, int *out /* nm, list bound */,
                                                    int rank_base)
{
    __shared__ Tri lds[16];
    __shared__ int s_base, s_len;
    if (threadIdx.x == 0) { s_base = 0; s_len = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < nzero + ncross; c0 += 1024) {
        const int c = c0 + threadIdx.x;
        int v = -1;
        if (c < nzero + ncross) { v = c < nzero ? zsrc[c] : nv0 + (c - nzero); if (!k2v2_member(P, v, cutof[v], s, rank_base + s)) v = -1; }
        Tri t{v >= 0, v >= 0 ? P.inc_len[v] : 0, 0};
        Tri tot;
        const Tri ex = block_exscan(t, &tot, lds);
        if (v >= 0) members[s_base + ex.a] = v;
        __syncthreads();
        if (threadIdx.x == 0) { s_base += tot.a; s_len += tot.b; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = s_base; out[1] = s_len; }
}

// The multi-kernel prune of a selected cut (fallback of k2_fused_t<true>) knows nothing of the other cuts of the round: a pair of
// SHARED on-plane members that also lie on the plane of a LATER cut of the round is that cut's to emit (k2_fused_body, `later`).
// Of the pairs E[e0 .. e0 + n) it appended, those are dropped here: flags + block sums, then ordered compaction into `out`.
__device__ __forceinline__ bool r2_pair_is_later(const PolyView &P, const int *cutof, int2 pr, int myrank)
{
    const int cu = cutof[pr.x], cv = cutof[pr.y];
    if (cu >= -1 || cv >= -1) return false;                 // only elements shared by several cuts carry the rank of another cut of the round
    const int ku = -1 - cu, kv = -1 - cv;
    const int *tu = P.pool + P.inc_off[pr.x] + P.inc_len[pr.x] - ku, *tv = P.pool + P.inc_off[pr.y] + P.inc_len[pr.y] - kv;
    for (int a = 0; a < ku; a++) { const int g = tu[a]; if (g <= myrank) continue; for (int b = 0; b < kv; b++) if (tv[b] == g) return true; }
    return false;
}
__global__ __launch_bounds__(PB) void k_r2_dedupe_flags(PolyView P, const int *cutof, const int2 *E, int e0, int n, int myrank, Tri *bsum)
{
    __shared__ Tri lds[16];
    const int k = blockIdx.x * PB + threadIdx.x;
    Tri t{0, 0, 0};
    if (k < n) t.a = r2_pair_is_later(P, cutof, E[e0 + k], myrank) ? 0 : 1;
    Tri tot;
    (void)block_exscan(t, &tot, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(PB) void k_r2_dedupe_emit(PolyView P, const int *cutof, const int2 *E, int e0, int n, int myrank, const Tri *bpre, int2 *out)
{
    __shared__ Tri lds[16];
    const int k = blockIdx.x * PB + threadIdx.x;
    Tri t{0, 0, 0};
    int2 pr{0, 0};
    if (k < n) { pr = E[e0 + k]; t.a = r2_pair_is_later(P, cutof, pr, myrank) ? 0 : 1; }
    Tri tot;
    const Tri ex = block_exscan(t, &tot, lds);
    if (t.a) out[bpre[blockIdx.x].a + ex.a] = pr;
}

// debugging aid (BSLV_R2_DEBUG=2): every edge of the list joins two live elements
__global__ void k_r2_check_edges(PolyView P, const int2 *E, int ne, int *out /* [0] count, [1..3] first bad edge, its ends */)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const int2 ed = E[e];
    const bool ok = (P.flag[ed.x] & F_USED) && (P.flag[ed.y] & F_USED) && ed.x != ed.y;
    if (!ok && atomicAdd(&out[0], 1) == 0) { out[1] = e; out[2] = ed.x; out[3] = ed.y; }
}
