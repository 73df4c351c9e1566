// poly_compact.inc -- reclaim the slots of cut-off elements and the garbage of the incidence pool (bslv_poly_garbage,
// bslv_poly_compact; include/bslv_hip.h); included at the end of poly_engine.hip.  Out of place: every new array is allocated before
// anything moves, the old ones are freed after the last kernel has run, so the peak is old + new.  Kernels, all bandwidth-bound:
//   k_cmp_totals   one pass over the element slots and the edge list: live elements, the pool words their lists hold (64-bit), edges
//                  with an end that is no live element, lists that do not lie inside the pool -- the figures of bslv_poly_garbage and
//                  the verdict "nothing to refuse" of bslv_poly_compact BEFORE it allocates
//   (a) CompactLive through k_compact_count / k_compact_emit: old_of_new (ascending) and its inverse new_of_old, -1 on a dead slot
//   (b) k_cmp_gather   lane j of column blockIdx.y reads X[y][old_of_new[j]] and writes X'[y][j]: the writes are coalesced, the reads
//                  ascend with j (a gather along one column, never a stride across columns); the last y moves flag, cls and inc_len
//   (c) k_cmp_lensum, k_cmp_scan64, k_cmp_lists   two-level exclusive scan of the new inc_len in 64 bits (pool words can pass 2^31; Tri
//                  holds ints), then the copy: a lane per list up to LONGN entries, the whole wave in coalesced chunks per longer list
//   (d) k_cmp_edges    both ends of E[ecur][0 .. ne) through new_of_old
namespace bslv {

enum { CMP_LIVE = 0, CMP_WORDS, CMP_DEADENDS, CMP_BADLISTS, CMP_UNMAPPED, CMP_NCNT };
typedef unsigned long long cmp_u64;

__device__ __forceinline__ cmp_u64 cmp_wave_sum(cmp_u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__global__ __launch_bounds__(PB) void k_cmp_totals(PolyView P, int nv, unsigned poolused, const int2 *__restrict__ E, int ne, cmp_u64 *cnt)
{
    const int i = blockIdx.x * PB + threadIdx.x;
    cmp_u64 live = 0, words = 0, dead = 0, bad = 0;
    if (i < nv && (P.flag[i] & F_USED)) {
        const int n = P.inc_len[i];
        live = 1;
        if (n < 0 || (cmp_u64)P.inc_off[i] + (cmp_u64)(n < 0 ? 0 : n) > (cmp_u64)poolused) bad = 1;
        else words = (cmp_u64)n;
    }
    if (i < ne) {
        const int2 ed = E[i];
        if (ed.x < 0 || ed.x >= nv || ed.y < 0 || ed.y >= nv || !(P.flag[ed.x] & F_USED) || !(P.flag[ed.y] & F_USED)) dead = 1;
    }
    live = cmp_wave_sum(live); words = cmp_wave_sum(words); dead = cmp_wave_sum(dead); bad = cmp_wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (live) atomicAdd(&cnt[CMP_LIVE], live);
        if (words) atomicAdd(&cnt[CMP_WORDS], words);
        if (dead) atomicAdd(&cnt[CMP_DEADENDS], dead);
        if (bad) atomicAdd(&cnt[CMP_BADLISTS], bad);
    }
}
// (a) the live slots in ascending order and the inverse map
struct CompactLive : CompactOp {
    const unsigned char *flag; int *old_of_new, *new_of_old;
    __device__ __forceinline__ Tri pick(int i) const { return Tri{(flag[i] & F_USED) ? 1 : 0, 0, 0}; }
    __device__ __forceinline__ void seen_emit(int i, const Tri &t) const { if (!t.a) new_of_old[i] = -1; }
    __device__ __forceinline__ void put(int i, int pos, const Tri &) const { old_of_new[pos] = i; new_of_old[i] = pos; }
};
// (b)
struct CmpElems { double *X; unsigned char *flag; signed char *cls; int *inc_len; int cap; };
__global__ __launch_bounds__(PB) void k_cmp_gather(PolyView P, const int *__restrict__ old_of_new, int live, CmpElems N)
{
    const int j = blockIdx.x * PB + threadIdx.x;
    if (j >= live) return;
    const int o = old_of_new[j], y = blockIdx.y;
    if (y < P.d) N.X[(size_t)y * N.cap + j] = P.X[(size_t)y * P.cap + o];
    else { N.flag[j] = P.flag[o]; N.cls[j] = P.cls[o]; N.inc_len[j] = P.inc_len[o]; }
}
// (c) exclusive scan of one 64-bit value per thread over the workgroup (blockDim.x a multiple of 64, <= 1024)
__device__ cmp_u64 cmp_block_exscan(cmp_u64 v, cmp_u64 *tot, cmp_u64 *lds /* >= 16 */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    cmp_u64 inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const cmp_u64 y = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += y;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    cmp_u64 base = 0, total = 0;
    for (int w = 0; w < nw; w++) {
        if (w < wave) base += lds[w];
        total += lds[w];
    }
    *tot = total;
    return base + inc - v;
}
__global__ __launch_bounds__(PB) void k_cmp_lensum(const int *__restrict__ len, int live, cmp_u64 *bsum)
{
    __shared__ cmp_u64 lds[16];
    const int j = blockIdx.x * PB + threadIdx.x;
    cmp_u64 tot;
    (void)cmp_block_exscan(j < live ? (cmp_u64)len[j] : 0ull, &tot, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
// one workgroup: bsum[0 .. nb) become exclusive prefixes, bsum[nb] the total
__global__ __launch_bounds__(1024) void k_cmp_scan64(cmp_u64 *bsum, int nb)
{
    __shared__ cmp_u64 lds[16];
    __shared__ cmp_u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const cmp_u64 v = b < nb ? bsum[b] : 0ull;
        cmp_u64 tot;
        const cmp_u64 ex = cmp_block_exscan(v, &tot, lds);
        if (b < nb) bsum[b] = s_carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = s_carry;
}
__global__ __launch_bounds__(PB) void k_cmp_lists(PolyView P, const int *__restrict__ old_of_new, int live, const int *__restrict__ len_new, const cmp_u64 *__restrict__ bpre,
                                                  unsigned *__restrict__ off_new, int *__restrict__ pool_new)
{
    __shared__ cmp_u64 lds[16];
    const int j = blockIdx.x * PB + threadIdx.x, lane = threadIdx.x & 63;
    int n = 0;
    unsigned src = 0;
    if (j < live) { n = len_new[j]; src = P.inc_off[old_of_new[j]]; }
    cmp_u64 tot;
    const cmp_u64 dst = bpre[blockIdx.x] + cmp_block_exscan((cmp_u64)n, &tot, lds);
    if (j < live) off_new[j] = (unsigned)dst;
    if (n > 0 && n <= LONGN) {                    // a lane per short list
        const int *__restrict__ L = P.pool + src;
        int *__restrict__ D = pool_new + dst;
        for (int k = 0; k < n; k++) D[k] = L[k];
    }
    cmp_u64 longs = __ballot(n > LONGN);          // the whole wave per long list, coalesced
    while (longs) {
        const int l = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const int nl = __shfl(n, l, WAVE);
        const unsigned sl = __shfl(src, l, WAVE);
        const cmp_u64 dl = __shfl(dst, l, WAVE);
        const int *__restrict__ L = P.pool + sl;
        int *__restrict__ D = pool_new + dl;
        for (int k = lane; k < nl; k += WAVE) D[k] = L[k];
    }
}
// (d)
__global__ __launch_bounds__(PB) void k_cmp_edges(const int2 *__restrict__ E, int ne, const int *__restrict__ new_of_old, int2 *__restrict__ Enew, cmp_u64 *cnt)
{
    const int e = blockIdx.x * PB + threadIdx.x;
    if (e >= ne) return;
    const int2 ed = E[e];
    const int2 m = int2{new_of_old[ed.x], new_of_old[ed.y]};      // (k_cmp_totals found both ends in range and alive)
    if (m.x < 0 || m.y < 0) atomicAdd(&cnt[CMP_UNMAPPED], 1ull);
    Enew[e] = m;
}

}  // namespace bslv

// device bytes of the element, pool and edge arrays at their current capacities
static long cmp_bytes(const bslv_poly *h)
{
    const size_t cap = (size_t)h->P.cap;
    size_t b = (size_t)h->d * cap * sizeof(double) + cap * (1 + 1 + sizeof(unsigned) + sizeof(int) + sizeof(unsigned long long) + sizeof(int)) + (size_t)h->lslotcap * sizeof(int);
    if (h->poolcap) b += ((size_t)h->poolcap + 64) * sizeof(int) + (size_t)h->poolcap;
    if (!h->hot) b += (size_t)h->ecap * (2 * sizeof(int2) + 1);
    return (long)b;
}
// the counters of k_cmp_totals (one launch, one synchronise) and the six figures of bslv_poly_garbage
static int cmp_figures(bslv_poly *h, cmp_u64 cnt[CMP_NCNT], long out[6])
{
    hipStream_t s = h->stream;
    if (!h->cmp_d) HIP_TRY(malloc0s(&h->cmp_d, CMP_NCNT * sizeof(cmp_u64), s));
    HIP_TRY(hipMemsetAsync(h->cmp_d, 0, CMP_NCNT * sizeof(cmp_u64), s));
    const int n = std::max(h->nv, h->ne);
    hipLaunchKernelGGL(k_cmp_totals, dim3(std::max(1, (n + PB - 1) / PB)), dim3(PB), 0, s, h->P, h->nv, h->poolused, (const int2 *)h->E[h->ecur], h->ne, h->cmp_d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cnt, h->cmp_d, CMP_NCNT * sizeof(cmp_u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out[0] = h->nv; out[1] = (long)cnt[CMP_LIVE]; out[2] = (long)h->poolused; out[3] = (long)cnt[CMP_WORDS]; out[4] = h->ne; out[5] = cmp_bytes(h);
    return 0;
}

extern "C" {

int bslv_poly_garbage(bslv_poly *h, long out[6])
{
    if (!h || !out) { set_error("bslv_poly_garbage: bad argument"); return BSLV_E_ARG; }
    for (int k = 0; k < 6; k++) out[k] = 0;
    if (!h->initialised || h->nv == 0) return 0;
    if (h->hot) { set_error("bslv_poly_garbage: a chunk of cuts is open"); return BSLV_E_STATE; }
    int rc;
    if ((rc = settle_k2(h))) return rc;
    cmp_u64 cnt[CMP_NCNT];
    return cmp_figures(h, cnt, out);
}

int bslv_poly_last_compact_stats(const bslv_poly *h, long out[8])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 8; k++) out[k] = h->cmp_stats[k];
    return 0;
}

int bslv_poly_compact(bslv_poly *h, int *new_of_old, long out[6])
{
    if (!h) { set_error("bslv_poly_compact: bad argument"); return BSLV_E_ARG; }
    long fig[6] = {0, 0, 0, 0, 0, 0};
    if (out) for (int k = 0; k < 6; k++) out[k] = 0;
    if (!h->initialised || h->nv == 0) return 0;
    if (h->hot) { set_error("bslv_poly_compact: a chunk of cuts is open (the call is legal between bslv_poly_add / bslv_poly_add_cuts calls only)"); return BSLV_E_STATE; }
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = h->stream;
    int rc;
    if ((rc = settle_k2(h))) return rc;
    cmp_u64 cnt[CMP_NCNT];
    if ((rc = cmp_figures(h, cnt, fig))) return rc;
    if (cnt[CMP_DEADENDS]) { set_error("bslv_poly_compact: %llu edge(s) with an end that is no live element; nothing was moved (bslv_poly_check names them)", cnt[CMP_DEADENDS]); return BSLV_E_STATE; }
    if (cnt[CMP_BADLISTS] || cnt[CMP_WORDS] > (cmp_u64)h->poolused) { set_error("bslv_poly_compact: %llu incidence list(s) outside the pool, or lists that overlap; nothing was moved", cnt[CMP_BADLISTS]); return BSLV_E_STATE; }
    const int nv0 = h->nv, ne = h->ne, d = h->d, live = (int)cnt[CMP_LIVE];
    const cmp_u64 words = cnt[CMP_WORDS];
    const unsigned pool0 = h->poolused;
    const long bytes0 = fig[5];
    h->pre_f = -1;                     // a halfspace classified ahead of its turn is classified again: its classes are not moved
    long *S = h->cmp_stats;
    auto book = [&](long slots, long pw, long bytes) {
        const long us = (long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        S[0]++; S[1] = slots; S[2] = pw; S[3] = bytes; S[4] += slots; S[5] += pw; S[6] = us; S[7] += us;
    };
    if (live == nv0 && words == (cmp_u64)pool0) {          // nothing dead, no slack, no garbage: the identity, and no allocation
        if (new_of_old) for (int i = 0; i < nv0; i++) new_of_old[i] = i;
        if (out) for (int k = 0; k < 6; k++) out[k] = fig[k];
        book(0, 0, 0);
        return 0;
    }
    // (a), count pass: the prefixes of the emit pass (bsum)
    CompactLive op{{}, h->P.flag, nullptr, nullptr};
    Tri t;
    if ((rc = compact_count(h, op, nv0, &t))) return rc;
    if (t.a != live) { set_error("bslv_poly_compact: internal: %d live elements counted, then %d", live, t.a); return BSLV_E_STATE; }
    // new capacities: max(the engine's minimum, twice what is needed), never above the old ones
    const bool keepc = h->cmp_keep_cap;       // (test hook, bslv_poly_debug_set key 21)
    const int vcap = keepc ? h->P.cap : (int)std::min<long long>(h->P.cap, std::max<long long>(1024, 2ll * live));
    const size_t pcap = keepc ? (size_t)h->poolcap : std::min<size_t>(h->poolcap, std::max<size_t>(1 << 16, 2 * (size_t)words));
    const int ecap = keepc ? h->ecap : (int)std::min<long long>(h->ecap, std::max<long long>(4096, 2ll * ne));
    const int nbl = compact_blocks(live);
    double *X = nullptr; unsigned char *flag = nullptr, *keep = nullptr, *eflag = nullptr; signed char *cls = nullptr; unsigned *inc_off = nullptr;
    int *inc_len = nullptr, *members = nullptr, *lslot = nullptr, *pool = nullptr, *o2n = nullptr, *n2o = nullptr; unsigned long long *capx = nullptr; cmp_u64 *bsum64 = nullptr;
    int2 *E0 = nullptr, *E1 = nullptr;
    auto free_new = [&]() {
        void *all[] = {X, flag, keep, eflag, cls, inc_off, inc_len, members, lslot, pool, capx, E0, E1};
        for (void *p : all) if (p) (void)hipFree(p);
    };
    auto free_scratch = [&]() { void *all[] = {o2n, n2o, bsum64}; for (void *p : all) if (p) (void)hipFree(p); };
    // every new array before anything moves; a failure leaves the polyhedron as it was
#define CMP_ALLOC(p, bytes) \
    if (malloc0s(&p, (bytes), s) != hipSuccess) { (void)hipGetLastError(); free_new(); free_scratch(); set_error("bslv_poly_compact: allocation of %zu bytes failed (%s); the polyhedron is unchanged", (size_t)(bytes), #p); return BSLV_E_NODEVICE; }
    CMP_ALLOC(X, (size_t)d * vcap * sizeof(double))
    CMP_ALLOC(flag, (size_t)vcap)
    CMP_ALLOC(cls, (size_t)vcap)
    CMP_ALLOC(inc_off, (size_t)vcap * sizeof(unsigned))
    CMP_ALLOC(inc_len, (size_t)vcap * sizeof(int))
    CMP_ALLOC(capx, (size_t)vcap * sizeof(unsigned long long))
    CMP_ALLOC(members, (size_t)vcap * sizeof(int))
    CMP_ALLOC(lslot, (size_t)vcap * sizeof(int))
    CMP_ALLOC(pool, (pcap + 64) * sizeof(int))
    CMP_ALLOC(keep, pcap)
    CMP_ALLOC(E0, (size_t)ecap * sizeof(int2))
    CMP_ALLOC(E1, (size_t)ecap * sizeof(int2))
    CMP_ALLOC(eflag, (size_t)ecap)
    CMP_ALLOC(o2n, (size_t)std::max(1, live) * sizeof(int))
    CMP_ALLOC(n2o, (size_t)nv0 * sizeof(int))
    CMP_ALLOC(bsum64, ((size_t)nbl + 1) * sizeof(cmp_u64))
#undef CMP_ALLOC
    auto fail = [&](int code) { (void)hipStreamSynchronize(s); free_new(); free_scratch(); return code; };
#define CMP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { set_error("bslv_poly_compact: %s failed: %s; the polyhedron is unchanged", #expr, hipGetErrorString(e_)); return fail(BSLV_E_NODEVICE); } } while (0)
    // what later kernels rely on and a fresh allocation does not give (BSLV_FILL): flag, capx and keep zero, no membership bitmap row
    CMP_TRY(hipMemsetAsync(flag, 0, (size_t)vcap, s));
    CMP_TRY(hipMemsetAsync(capx, 0, (size_t)vcap * sizeof(unsigned long long), s));
    CMP_TRY(hipMemsetAsync(lslot, 0xFF, (size_t)vcap * sizeof(int), s));
    CMP_TRY(hipMemsetAsync(keep, 0, pcap, s));
    op.old_of_new = o2n; op.new_of_old = n2o;
    if ((rc = compact_emit(h, op, nv0))) return fail(rc);
    if (live > 0) {
        hipLaunchKernelGGL(k_cmp_gather, dim3(nbl, d + 1), dim3(PB), 0, s, h->P, (const int *)o2n, live, CmpElems{X, flag, cls, inc_len, vcap});
        hipLaunchKernelGGL(k_cmp_lensum, dim3(nbl), dim3(PB), 0, s, (const int *)inc_len, live, bsum64);
        hipLaunchKernelGGL(k_cmp_scan64, dim3(1), dim3(1024), 0, s, bsum64, nbl);
        hipLaunchKernelGGL(k_cmp_lists, dim3(nbl), dim3(PB), 0, s, h->P, (const int *)o2n, live, (const int *)inc_len, (const cmp_u64 *)bsum64, inc_off, pool);
    } else CMP_TRY(hipMemsetAsync(bsum64, 0, ((size_t)nbl + 1) * sizeof(cmp_u64), s));
    int2 *Enew = h->ecur == 0 ? E0 : E1;
    if (ne > 0) hipLaunchKernelGGL(k_cmp_edges, dim3((ne + PB - 1) / PB), dim3(PB), 0, s, (const int2 *)h->E[h->ecur], ne, (const int *)n2o, Enew, h->cmp_d);
    CMP_TRY(hipGetLastError());
    cmp_u64 words_new = 0;
    CMP_TRY(hipMemcpyAsync(&words_new, bsum64 + nbl, sizeof(cmp_u64), hipMemcpyDeviceToHost, s));
    CMP_TRY(hipMemcpyAsync(cnt, h->cmp_d, CMP_NCNT * sizeof(cmp_u64), hipMemcpyDeviceToHost, s));
    if (new_of_old) CMP_TRY(hipMemcpyAsync(new_of_old, n2o, (size_t)nv0 * sizeof(int), hipMemcpyDeviceToHost, s));
    CMP_TRY(hipStreamSynchronize(s));
#undef CMP_TRY
    if (cnt[CMP_UNMAPPED] || words_new != words) {
        set_error("bslv_poly_compact: internal: %llu edge end(s) without a new name, %llu pool words packed where %llu were counted; the polyhedron is unchanged", cnt[CMP_UNMAPPED], words_new, words);
        return fail(BSLV_E_STATE);
    }
    // the old arrays go, the new ones take their place
    PolyView &P = h->P;
    void *old[] = {P.X, P.flag, P.cls, P.inc_off, P.inc_len, P.capx, P.pool, P.keep, h->members, h->lslot_d, h->E[0], h->E[1], h->eflag};
    for (void *p : old) if (p) (void)hipFree(p);
    free_scratch();
    P.X = X; P.flag = flag; P.cls = cls; P.inc_off = inc_off; P.inc_len = inc_len; P.capx = capx; P.pool = pool; P.keep = keep; P.cap = vcap;
    h->members = members; h->lslot_d = lslot; h->lslotcap = vcap;
    h->E[0] = E0; h->E[1] = E1; h->eflag = eflag; h->ecap = ecap;
    h->poolcap = (unsigned)pcap; h->poolused = (unsigned)words;
    h->nv = live;
    fig[0] = live; fig[1] = live; fig[2] = (long)words; fig[3] = (long)words; fig[4] = ne; fig[5] = cmp_bytes(h);
    if (out) for (int k = 0; k < 6; k++) out[k] = fig[k];
    book(nv0 - live, (long)pool0 - (long)words, bytes0 - fig[5]);
    return 0;
}

}  // extern "C"
