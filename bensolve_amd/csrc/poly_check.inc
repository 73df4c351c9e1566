// poly_check.inc -- consistency check of the resident polyhedron (poly__polyck, bslv_poly.c:940-990, and its converse); included at the
// end of poly_engine.hip.  Three kernels:
//   k_check_incidence    one wave per live element walks its incidence list: every entry is a valid rank of an applied facet, the list
//                        ascends strictly, and the element lies on the facet's hyperplane within tol
//   k_check_halfspaces   dense scan, one element per lane against a tile of hyperplanes in LDS: an element on a facet's hyperplane
//                        (POLY_EPS) must list it, and no element lies on the wrong side of a facet by more than tol
//   k_check_pairs        edge_test (bslv_poly.c:467-512) over all pairs of the examined rows, structured as k_dpair_flags: row i's list
//                        in LDS, lane j intersects, and for every candidate pair the wave sweeps the elements ON THE PAIR'S FIRST MUTUAL
//                        FACET for a third element that lies on all mutual facets; a pair that passes is looked up in the edge list
// READ-ONLY and BOUNDED: the kernels write nothing but their own counters, flags and offender buffer.  A list that does not lie inside
// the pool, an entry that is no rank, an edge endpoint that is no live element are COUNTED ([3], [7]) and never dereferenced: the list
// lengths every later step uses are the sanitised ones k_check_incidence leaves in clen (0 for a dead element or a list outside the
// pool), facet-major member lists and the edge table are built on the host from entries that passed the same range checks, and a first
// mutual facet that is no rank has no member list.
namespace bslv {

constexpr unsigned char CK_APPLIED = 1, CK_NOGEO = 2;      // per dual slot: applied (fapplied); the facet at infinity, which has no hyperplane of its own
constexpr int CK_FT = 64;                                  // hyperplanes per LDS tile of k_check_halfspaces
enum { CK_N_INC = 0, CK_N_BADINC, CK_N_UNLISTED, CK_N_INFEAS, CK_WORST_RES, CK_WORST_NEG, CK_N_PASS, CK_N_BOTH, CK_N_OFF, CK_NCNT };

struct CheckView {
    int nv, nranks;                 // element slots, facet ranks
    unsigned poolused;
    const int *r2f;                 // dual slot of a rank (r2f_d)
    const double *hp;               // hyperplane of every dual slot, (d+1) doubles each (h->hp)
    const unsigned char *fst;       // CK_* per dual slot
    int *clen;                      // per element slot: the length the check walks (written by k_check_incidence)
    unsigned long long *cnt;        // CK_NCNT counters; the two `worst` entries hold the bits of a non-negative double
    int *off;                       // offenders kept: (kind, a, b), the first max_off that arrive
    int max_off;
    double tol;
};
__device__ __forceinline__ void ck_offender(const CheckView &C, int kind, int a, int b)
{
    const unsigned long long k = atomicAdd(&C.cnt[CK_N_OFF], 1ull);
    if (k < (unsigned long long)C.max_off) { int *o = C.off + 3 * k; o[0] = kind; o[1] = a; o[2] = b; }
}
// coordinates of element i in registers (static indices: d <= MAXD)
__device__ __forceinline__ void ck_load_x(const PolyView &P, int i, double (&x)[MAXD])
{
#pragma unroll
    for (int k = 0; k < MAXD; k++) x[k] = k < P.d ? P.X[(size_t)k * P.cap + i] : 0.0;
}
// hp . x - alpha (alpha = 0 for an ideal element), the fma chain of classify_one
__device__ __forceinline__ double ck_slack(const double *hp, const double (&x)[MAXD], int d, bool ideal)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < MAXD; k++) if (k < d) s = fma(hp[k], x[k], s);
    return s - (ideal ? 0.0 : hp[d]);
}
__device__ __forceinline__ void ck_add(const CheckView &C, int which, int v) { if (v) atomicAdd(&C.cnt[which], (unsigned long long)v); }
__device__ __forceinline__ void ck_max(const CheckView &C, int which, double v) { if (v > 0.0) atomicMax(&C.cnt[which], (unsigned long long)__double_as_longlong(v)); }

__global__ __launch_bounds__(PB) void k_check_incidence(PolyView P, CheckView C)
{
    __shared__ Tri lds[16];
    const int i = blockIdx.x * (PB / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    Tri t{0, 0, 0};          // a: entries examined, b: bad entries
    double worst = 0.0;
    if (i < C.nv && (P.flag[i] & F_USED)) {
        const unsigned o = P.inc_off[i];
        const int n = P.inc_len[i];
        const bool inpool = n >= 0 && (unsigned long long)o + (unsigned long long)n <= (unsigned long long)C.poolused;
        if (lane == 0) C.clen[i] = inpool ? n : 0;
        if (!inpool) { if (lane == 0) { t.b = 1; ck_offender(C, 3, i, -1); } }
        else {
            const int *L = P.pool + o;
            const bool ideal = P.flag[i] & F_IDEAL;
            double x[MAXD];
            ck_load_x(P, i, x);
            for (int j = lane; j < n; j += WAVE) {
                const int r = L[j];
                const bool isrank = r >= 0 && r < C.nranks;
                bool bad = !isrank || (j > 0 && L[j - 1] >= r);
                int f = -1;
                if (isrank) {
                    f = C.r2f[r];
                    const unsigned char st = C.fst[f];
                    if (!(st & CK_APPLIED)) bad = true;
                    else if (!(st & CK_NOGEO)) {
                        const double res = fabs(ck_slack(C.hp + (size_t)f * (P.d + 1), x, P.d, ideal));
                        worst = fmax(worst, res);
                        if (!(res <= C.tol)) bad = true;
                    }
                }
                t.a++;
                if (bad) { t.b++; ck_offender(C, 3, i, f); }
            }
        }
    }
    worst = wave_max(worst);
    if (lane == 0) ck_max(C, CK_WORST_RES, worst);
    t = block_sum(t, lds);
    if (threadIdx.x == 0) { ck_add(C, CK_N_INC, t.a); ck_add(C, CK_N_BADINC, t.b); }
}

// gfac: the ranks of the live facets that have a hyperplane; blockIdx.y = tile of CK_FT of them
__global__ __launch_bounds__(PB) void k_check_halfspaces(PolyView P, CheckView C, const int *__restrict__ gfac, int ng)
{
    __shared__ Tri lds[16];
    __shared__ double s_hp[CK_FT * (MAXD + 1)];
    __shared__ int s_rank[CK_FT], s_slot[CK_FT];
    const int i = blockIdx.x * PB + threadIdx.x;
    const int t0 = blockIdx.y * CK_FT, nt = min(CK_FT, ng - t0), d1 = P.d + 1;
    for (int t = threadIdx.x; t < nt; t += PB) { const int r = gfac[t0 + t]; s_rank[t] = r; s_slot[t] = C.r2f[r]; }
    __syncthreads();
    for (int e = threadIdx.x; e < nt * d1; e += PB) { const int t = e / d1, k = e - t * d1; s_hp[t * (MAXD + 1) + k] = C.hp[(size_t)s_slot[t] * d1 + k]; }
    __syncthreads();
    Tri c{0, 0, 0};          // a: unlisted incidences, b: violated halfspaces
    double worst = 0.0;
    if (i < C.nv && (P.flag[i] & F_USED)) {
        const bool ideal = P.flag[i] & F_IDEAL;
        const int *L = P.pool + P.inc_off[i];
        const int n = C.clen[i];
        double x[MAXD];
        ck_load_x(P, i, x);
        for (int t = 0; t < nt; t++) {
            const double slack = ck_slack(s_hp + t * (MAXD + 1), x, P.d, ideal);
            if (slack < -C.tol) { c.b++; worst = fmax(worst, -slack); ck_offender(C, 5, i, s_slot[t]); }
            if (fabs(slack) <= POLY_EPS) {
                const int r = s_rank[t];
                int lo = 0, hi = n;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (L[mid] < r) lo = mid + 1; else hi = mid; }
                if (!(lo < n && L[lo] == r)) { c.a++; ck_offender(C, 4, i, s_slot[t]); }
            }
        }
    }
    worst = wave_max(worst);
    if ((threadIdx.x & 63) == 0) ck_max(C, CK_WORST_NEG, worst);
    c = block_sum(c, lds);
    if (threadIdx.x == 0) { ck_add(C, CK_N_UNLISTED, c.a); ck_add(C, CK_N_INFEAS, c.b); }
}

struct PairCk {
    const int *rows; int L;                             // live element slots, ascending: row -> slot
    const unsigned *fm_off; const int *fm_list;         // per facet rank: the live elements on it (slots, ascending)
    const unsigned *eoff; const int *eb;                // the distinct edges a < b between live elements, sorted: eb[eoff[a] .. eoff[a + 1]) = the b of a
    unsigned char *ehit;                                // per such edge: the pair passed the test
};
// one workgroup = row pb.i against the 256 rows from pb.j0 on (pb.j0 > pb.i)
__global__ __launch_bounds__(PB) void k_check_pairs(PolyView P, CheckView C, PairCk Q, const PairBlk *__restrict__ blks)
{
    __shared__ Tri lds[16];
    __shared__ int s_row[1024];
    const PairBlk pb = blks[blockIdx.x];
    const int a = Q.rows[pb.i];
    const int ni = C.clen[a];
    const int *Li = P.pool + P.inc_off[a];
    const bool cached = ni <= 1024;
    if (cached) for (int t = threadIdx.x; t < ni; t += PB) s_row[t] = Li[t];
    __syncthreads();
    const int *A = cached ? s_row : Li;
    const int jr = pb.j0 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int b = -1, nmut = 0, first = -1;
    bool cand = false;
    if (jr < Q.L) {
        b = Q.rows[jr];
        nmut = isect_count_first(A, ni, P.pool + P.inc_off[b], C.clen[b], &first);
        cand = (P.d == 1) || (nmut >= P.d - 1);
    }
    bool adj = cand;
    unsigned long long todo = __ballot(cand && P.d > 1);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int cb = __shfl(b, src, WAVE);
        const int cn = __shfl(nmut, src, WAVE);
        const int cf = __shfl(first, src, WAVE);
        const int *cL = P.pool + P.inc_off[cb];
        const int cnb = C.clen[cb];
        const bool isrank = cf >= 0 && cf < C.nranks;
        const int *M = Q.fm_list + (isrank ? Q.fm_off[cf] : 0u);
        const int nm = isrank ? (int)(Q.fm_off[cf + 1] - Q.fm_off[cf]) : 0;
        bool found = false;
        for (int base = 0; base < nm; base += WAVE) {
            const int k = base + lane;
            bool hit = false;
            if (k < nm) {
                const int w = M[k];
                const int nw = C.clen[w];
                if (w != a && w != cb && nw >= cn) hit = isect3_count(A, ni, cL, cnb, P.pool + P.inc_off[w], nw) == cn;
            }
            if (__ballot(hit)) { found = true; break; }
        }
        if (lane == src) adj = !found;
    }
    int listed = 0;
    if (adj) {
        unsigned lo = Q.eoff[a], hi = Q.eoff[a + 1];
        const unsigned end = hi;
        while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (Q.eb[mid] < b) lo = mid + 1; else hi = mid; }
        if (lo < end && Q.eb[lo] == b) { listed = 1; Q.ehit[lo] = 1; }
        else ck_offender(C, 10, a, b);
    }
    const Tri t = block_sum(Tri{adj ? 1 : 0, listed, 0}, lds);
    if (threadIdx.x == 0) { ck_add(C, CK_N_PASS, t.a); ck_add(C, CK_N_BOTH, t.b); }
}

}  // namespace bslv

namespace {
// device scratch of one check: freed when the call returns, however it returns
struct CkScratch {
    std::vector<void *> ptrs;
    hipStream_t s;
    explicit CkScratch(hipStream_t st) : s(st) {}
    ~CkScratch() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T>
    hipError_t get(T **p, size_t n, const T *src = nullptr)          // n elements (at least one is allocated): zeros, or a copy of src
    {
        hipError_t e = hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) return e;
        ptrs.push_back((void *)*p);
        if (!src || n == 0) return hipMemsetAsync((void *)*p, 0, std::max<size_t>(n, 1) * sizeof(T), s);
        return hipMemcpyAsync((void *)*p, src, n * sizeof(T), hipMemcpyHostToDevice, s);
    }
};
struct CkTimer {          // BSLV_POLY_CHECK_TIMING=1: HIP events around each kernel
    bool on; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr; float ms[3] = {0, 0, 0};
    CkTimer(bool o, hipStream_t st) : on(o), s(st) { if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) on = false; }
    ~CkTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    void begin() { if (on) (void)hipEventRecord(e0, s); }
    void end(int k) { if (!on) return; float t = 0; if (hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[k] += t; }
};
}  // namespace

extern "C" {

int bslv_poly_check(bslv_poly *h, double tol, int row_first, int row_count, long out[12], double worst[2], int *offenders, int max_off, int *n_off)
{
    if (!h || !out || max_off < 0 || (max_off > 0 && !offenders)) { set_error("bslv_poly_check: bad argument"); return BSLV_E_ARG; }
    if (!h->initialised) { set_error("bslv_poly_check: called before bslv_poly_init"); return BSLV_E_STATE; }
    if (!(tol > 0)) tol = 1e-6;
    int rc;
    if ((rc = settle_k2(h))) return rc;
    if (h->hot) { set_error("bslv_poly_check: a chunk of cuts is open"); return BSLV_E_STATE; }
    const auto th0 = std::chrono::steady_clock::now();
    const int d = h->d, nv = h->nv, nf = h->nf, nranks = (int)h->facet_of_rank.size(), ne = h->ne;
    hipStream_t s = h->stream;
    std::vector<unsigned char> fl; std::vector<unsigned> off; std::vector<int> len, pool;
    if ((rc = fetch_inc(h, fl, off, len, pool))) return rc;
    // rows = live elements in ascending slot order; the list lengths as k_check_incidence sanitises them
    std::vector<int> rows, rowof(nv, -1);
    for (int i = 0; i < nv; i++) {
        if (fl[i] & F_USED) { rowof[i] = (int)rows.size(); rows.push_back(i); }
        if (!(fl[i] & F_USED) || len[i] < 0 || (unsigned long long)off[i] + (unsigned long long)len[i] > (unsigned long long)h->poolused) len[i] = 0;
    }
    const int L = (int)rows.size();
    if (row_first < 0 || row_first > L || (row_count >= 0 && row_count > L - row_first)) { set_error("bslv_poly_check: rows [%d, %d + %d) of %d live elements", row_first, row_first, row_count, L); return BSLV_E_ARG; }
    const int row_end = row_count < 0 ? L : row_first + row_count;
    // per dual slot: applied, and whether it has a hyperplane (dual slot 0 while it is ideal is the facet at infinity, bslv_poly.c:83-92)
    std::vector<unsigned char> fst(std::max(nf, 1), 0);
    for (int f = 0; f < nf; f++) fst[f] = (h->fapplied[f] ? CK_APPLIED : 0) | ((f == 0 && h->fideal[0]) ? CK_NOGEO : 0);
    // facet-major member lists over the ranks, and which ranks are live (bslv_poly_get_dual: applied, and a live element lies on it)
    std::vector<unsigned> fm_off((size_t)nranks + 1, 0);
    for (int i : rows) for (int j = 0; j < len[i]; j++) { const int r = pool[off[i] + j]; if (r >= 0 && r < nranks) fm_off[r + 1]++; }
    for (int r = 0; r < nranks; r++) fm_off[r + 1] += fm_off[r];
    std::vector<int> fm_list(fm_off[nranks]);
    {
        std::vector<unsigned> fill(fm_off.begin(), fm_off.end() - 1);
        for (int i : rows) for (int j = 0; j < len[i]; j++) { const int r = pool[off[i] + j]; if (r >= 0 && r < nranks) fm_list[fill[r]++] = i; }
    }
    std::vector<int> gfac;
    long nlive_f = 0;
    for (int r = 0; r < nranks; r++) {
        const int f = h->facet_of_rank[r];
        if (fm_off[r + 1] == fm_off[r] || !(fst[f] & CK_APPLIED)) continue;
        nlive_f++;
        if (!(fst[f] & CK_NOGEO)) gfac.push_back(r);
    }
    // the edge list: [7] bad endpoints, [8] repeated pairs; what is left, sorted, is the table the pair kernel looks a passing pair up in
    std::vector<int> host_off;                      // (kind, a, b) found on the host; at most max_off per kind are kept
    long host_n_off = 0, keep7 = 0, keep8 = 0, keep11 = 0;
    auto note = [&](int kind, int a, int b, long &kept) { host_n_off++; if (kept < max_off) { kept++; host_off.insert(host_off.end(), {kind, a, b}); } };
    std::vector<int2> E((size_t)std::max(ne, 1));
    if (ne > 0) HIP_TRY(hipMemcpy(E.data(), h->E[h->ecur], (size_t)ne * sizeof(int2), hipMemcpyDeviceToHost));
    std::vector<unsigned long long> keys;
    keys.reserve((size_t)ne);
    long nbad_e = 0, ndup_e = 0;
    for (int e = 0; e < ne; e++) {
        const int a = E[e].x, b = E[e].y;
        if (a < 0 || b < 0 || a >= nv || b >= nv || a == b || rowof[a] < 0 || rowof[b] < 0) { nbad_e++; note(7, a, b, keep7); continue; }
        keys.push_back((unsigned long long)std::min(a, b) << 32 | (unsigned)std::max(a, b));
    }
    std::sort(keys.begin(), keys.end());
    {
        size_t w = 0;
        for (size_t k = 0; k < keys.size(); k++) {
            if (w > 0 && keys[w - 1] == keys[k]) { ndup_e++; note(8, (int)(keys[k] >> 32), (int)(keys[k] & 0xFFFFFFFFull), keep8); }
            else keys[w++] = keys[k];
        }
        keys.resize(w);
    }
    const size_t nedge = keys.size();
    std::vector<unsigned> eoff((size_t)nv + 1, 0);
    std::vector<int> eb(nedge);
    long listed_in_rows = 0;
    for (size_t k = 0; k < nedge; k++) {
        const int a = (int)(keys[k] >> 32);
        eoff[a + 1]++; eb[k] = (int)(keys[k] & 0xFFFFFFFFull);
        if (rowof[a] >= row_first && rowof[a] < row_end) listed_in_rows++;
    }
    for (int i = 0; i < nv; i++) eoff[i + 1] += eoff[i];
    // device side
    if ((rc = sync_r2f(h))) return rc;
    CkScratch M(s);
    const int max_off_d = std::min(max_off, 1 << 20);
    CheckView C{};
    PairCk Q{};
    double *hp_d = nullptr; unsigned char *fst_d = nullptr, *ehit_d = nullptr; int *clen_d = nullptr, *off_d = nullptr, *rows_d = nullptr, *gfac_d = nullptr, *fm_list_d = nullptr, *eb_d = nullptr;
    unsigned *fm_off_d = nullptr, *eoff_d = nullptr; unsigned long long *cnt_d = nullptr; PairBlk *blks_d = nullptr;
    HIP_TRY(M.get(&hp_d, (size_t)nf * (d + 1), h->hp.data()));
    HIP_TRY(M.get(&fst_d, (size_t)nf, fst.data()));
    HIP_TRY(M.get(&clen_d, (size_t)nv));
    HIP_TRY(M.get(&cnt_d, (size_t)CK_NCNT));
    HIP_TRY(M.get(&off_d, (size_t)3 * max_off_d));
    HIP_TRY(M.get(&rows_d, (size_t)L, rows.data()));
    HIP_TRY(M.get(&gfac_d, gfac.size(), gfac.data()));
    HIP_TRY(M.get(&fm_off_d, fm_off.size(), fm_off.data()));
    HIP_TRY(M.get(&fm_list_d, fm_list.size(), fm_list.data()));
    HIP_TRY(M.get(&eoff_d, eoff.size(), eoff.data()));
    HIP_TRY(M.get(&eb_d, nedge, eb.data()));
    HIP_TRY(M.get(&ehit_d, nedge));
    C.nv = nv; C.nranks = nranks; C.poolused = h->poolused; C.r2f = h->r2f_d; C.hp = hp_d; C.fst = fst_d; C.clen = clen_d; C.cnt = cnt_d; C.off = off_d; C.max_off = max_off_d; C.tol = tol;
    Q.rows = rows_d; Q.L = L; Q.fm_off = fm_off_d; Q.fm_list = fm_list_d; Q.eoff = eoff_d; Q.eb = eb_d; Q.ehit = ehit_d;
    const bool timing = getenv("BSLV_POLY_CHECK_TIMING") != nullptr;
    CkTimer T(timing, s);
    const double ms_prep = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    if (nv > 0) {
        T.begin();
        hipLaunchKernelGGL(k_check_incidence, dim3((nv + PB / WAVE - 1) / (PB / WAVE)), dim3(PB), 0, s, h->P, C);
        HIP_TRY(hipGetLastError());
        T.end(0);
        if (!gfac.empty()) {
            T.begin();
            hipLaunchKernelGGL(k_check_halfspaces, dim3((nv + PB - 1) / PB, ((int)gfac.size() + CK_FT - 1) / CK_FT), dim3(PB), 0, s, h->P, C, (const int *)gfac_d, (int)gfac.size());
            HIP_TRY(hipGetLastError());
            T.end(1);
        }
    }
    // the pair scan: rows [row_first, row_end) in slabs of at most 2^20 pair blocks, so that no block index leaves 32 bits
    const long max_blocks = 1 << 20;
    long launches = 0;
    int row = row_first;
    const int last_row = std::min(row_end, L - 1);       // (the last live element has no partner behind it)
    std::vector<PairBlk> blks;
    while (row < last_row) {
        blks.clear();
        int r1 = row;
        while (r1 < last_row && (long)blks.size() + (L - r1 - 1 + PB - 1) / PB <= max_blocks) {
            for (int j0 = r1 + 1; j0 < L; j0 += PB) blks.push_back(PairBlk{r1, j0});
            r1++;
        }
        if (r1 == row) { set_error("bslv_poly_check: a single row exceeds the block budget"); return BSLV_E_CAPACITY; }
        if (!blks_d) HIP_TRY(M.get(&blks_d, r1 < last_row ? (size_t)max_blocks : blks.size()));      // (more slabs follow: none is larger than the budget)
        HIP_TRY(hipMemcpyAsync(blks_d, blks.data(), blks.size() * sizeof(PairBlk), hipMemcpyHostToDevice, s));
        T.begin();
        hipLaunchKernelGGL(k_check_pairs, dim3((unsigned)blks.size()), dim3(PB), 0, s, h->P, C, Q, (const PairBlk *)blks_d);
        HIP_TRY(hipGetLastError());
        T.end(2);
        HIP_TRY(hipStreamSynchronize(s));          // (blks is reused by the next slab)
        launches++;
        row = r1;
    }
    unsigned long long cnt[CK_NCNT];
    HIP_TRY(hipMemcpyAsync(cnt, cnt_d, sizeof cnt, hipMemcpyDeviceToHost, s));
    std::vector<unsigned char> ehit(std::max<size_t>(nedge, 1));
    if (nedge) HIP_TRY(hipMemcpyAsync(ehit.data(), ehit_d, nedge, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const auto th1 = std::chrono::steady_clock::now();
    const long kept_d = (long)std::min<unsigned long long>(cnt[CK_N_OFF], (unsigned long long)max_off_d);
    std::vector<int> all((size_t)3 * kept_d);
    if (kept_d) HIP_TRY(hipMemcpy(all.data(), off_d, (size_t)3 * kept_d * sizeof(int), hipMemcpyDeviceToHost));
    // [11]: the listed edges of the examined rows (counted under the smaller endpoint) that did not pass
    for (size_t k = 0; k < nedge; k++) {
        const int a = (int)(keys[k] >> 32);
        if (rowof[a] >= row_first && rowof[a] < row_end && !ehit[k]) note(11, a, eb[k], keep11);
    }
    out[0] = L; out[1] = nlive_f; out[2] = (long)cnt[CK_N_INC]; out[3] = (long)cnt[CK_N_BADINC]; out[4] = (long)cnt[CK_N_UNLISTED]; out[5] = (long)cnt[CK_N_INFEAS];
    out[6] = ne; out[7] = nbad_e; out[8] = ndup_e;
    out[9] = (long)cnt[CK_N_PASS]; out[10] = (long)(cnt[CK_N_PASS] - cnt[CK_N_BOTH]); out[11] = listed_in_rows - (long)cnt[CK_N_BOTH];
    if (worst) {
        double w0, w1;
        memcpy(&w0, &cnt[CK_WORST_RES], sizeof w0); memcpy(&w1, &cnt[CK_WORST_NEG], sizeof w1);
        worst[0] = w0; worst[1] = w1 > 0 ? -w1 : 0.0;
    }
    // offenders, sorted by (kind, a, b)
    all.insert(all.end(), host_off.begin(), host_off.end());
    const size_t nall = all.size() / 3;
    std::vector<size_t> ord(nall);
    for (size_t k = 0; k < nall; k++) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return std::lexicographical_compare(&all[3 * x], &all[3 * x] + 3, &all[3 * y], &all[3 * y] + 3); });
    for (size_t k = 0; k < nall && k < (size_t)max_off; k++) memcpy(offenders + 3 * k, &all[3 * ord[k]], 3 * sizeof(int));
    if (n_off) *n_off = (int)std::min<unsigned long long>(cnt[CK_N_OFF] + (unsigned long long)host_n_off, 0x7FFFFFFFull);
    if (timing)
        fprintf(stderr, "poly check: %d elements, %ld live facets, %d edges, rows [%d, %d) | host preparation %.3f ms, k_check_incidence %.3f ms, k_check_halfspaces %.3f ms, k_check_pairs %.3f ms in %ld launches, host tail %.3f ms\n",
                L, nlive_f, ne, row_first, row_end, ms_prep, T.ms[0], T.ms[1], T.ms[2], launches, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th1).count());
    return 0;
}

// TESTS ONLY: damage the resident state for bslv_poly_check to find.  Plain copies between host and device, no kernel.
int bslv_poly_debug_corrupt(bslv_poly *h, int what, int a, int b, double x)
{
    if (!h) { set_error("bslv_poly_debug_corrupt: bad argument"); return BSLV_E_ARG; }
    if (!h->initialised) { set_error("bslv_poly_debug_corrupt: called before bslv_poly_init"); return BSLV_E_STATE; }
    int rc;
    if ((rc = settle_k2(h))) return rc;
    if (h->hot) { set_error("bslv_poly_debug_corrupt: a chunk of cuts is open"); return BSLV_E_STATE; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    auto bad = [&]() { set_error("bslv_poly_debug_corrupt: what = %d, a = %d, b = %d out of range", what, a, b); return BSLV_E_ARG; };
    switch (what) {
    case 0: {        // delete edge number a: the last edge takes its place
        if (a < 0 || a >= h->ne) return bad();
        if (a != h->ne - 1) HIP_TRY(hipMemcpy(h->E[h->ecur] + a, h->E[h->ecur] + (h->ne - 1), sizeof(int2), hipMemcpyDeviceToDevice));
        h->ne--;
        return 0;
    }
    case 1: {        // append edge (a, b)
        if (a < 0 || b < 0 || a >= h->nv || b >= h->nv) return bad();
        if ((rc = ensure_ecap(h, h->ne + 1))) return rc;
        const int2 e{a, b};
        HIP_TRY(hipMemcpy(h->E[h->ecur] + h->ne, &e, sizeof e, hipMemcpyHostToDevice));
        h->ne++;
        return 0;
    }
    case 2: {        // drop the last entry of element a's incidence list
        if (a < 0 || a >= h->nv) return bad();
        int n = 0;
        HIP_TRY(hipMemcpy(&n, h->P.inc_len + a, sizeof n, hipMemcpyDeviceToHost));
        if (n < 1) return bad();
        n--;
        HIP_TRY(hipMemcpy(h->P.inc_len + a, &n, sizeof n, hipMemcpyHostToDevice));
        return 0;
    }
    case 3: {        // add x to coordinate b of element a
        if (a < 0 || a >= h->nv || b < 0 || b >= h->d) return bad();
        double v = 0;
        HIP_TRY(hipMemcpy(&v, h->P.X + (size_t)b * h->P.cap + a, sizeof v, hipMemcpyDeviceToHost));
        v += x;
        HIP_TRY(hipMemcpy(h->P.X + (size_t)b * h->P.cap + a, &v, sizeof v, hipMemcpyHostToDevice));
        return 0;
    }
    default: return bad();
    }
}

}  // extern "C"
