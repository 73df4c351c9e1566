#include <string>
#include <deque>
// poly_rounds2_host.inc -- host side of the device-selected rounds inside a hot chunk (kernels: poly_rounds2_kernels.inc).
// Included after poly_rounds_host.inc (RoundsBuf) and the single-cut pipeline (do_cut, k2_multi, hot_begin).

struct Rounds2Buf {
    RState *st_d = nullptr;
    RState *mail_h = nullptr, *mail_d = nullptr;          // mapped pinned copy of the state, written at the end of every round
    unsigned *alive = nullptr, *alive_prev = nullptr, *anym = nullptr, *bad = nullptr;
    int *selmap = nullptr, *sel = nullptr, *order = nullptr, *rcflag = nullptr;
    int bcap = 0;
    int *own = nullptr; int vcap = 0;
    unsigned long long *hw = nullptr; size_t hwcap = 0;     // element-major class words (hot elements and what the chunk creates)
    int *cnt_g = nullptr, *nm_g = nullptr, *mem_g = nullptr; unsigned *adj_g = nullptr; int scap = 0;
    int *npart_g = nullptr, *cntx_g = nullptr, *split_stat = nullptr;      // prunes worked in parts (K2V2)
    int *gout = nullptr, *gout_h = nullptr;
    int seq = 0;
    unsigned chunk_seed = 0;
    // conflict-matrix rounds (k_r2_select3): matrix over the cuts of the chunk, live MINUS elements per cut, selected cuts of the
    // round as a bit mask, per element the class words that hold a touch
    unsigned *M = nullptr, *selw = nullptr, *wm = nullptr; int *mcnt = nullptr; int wmcap = 0;
    int *fc2 = nullptr, *fl2 = nullptr, *fc_ticket = nullptr; int fc_slices = 0, fc_stride = 0;      // K2V2: counters of prunes with long member lists
    size_t ride_lds = 128 * 1024;     // dynamic LDS granted to k_r2_prune_classify
};
constexpr int R2_ADJW = (K2_MAXNM * (K2_MAXNM - 1) / 2 + 31) / 32;
constexpr int R2_MAILS = 4;

static void rounds2_free(Rounds2Buf &V)
{
    auto fr = [](void *p) { if (p) (void)hipFree(p); };
    fr(V.st_d); fr(V.alive); fr(V.alive_prev); fr(V.anym); fr(V.bad); fr(V.selmap); fr(V.sel); fr(V.order); fr(V.rcflag); fr(V.own);
    fr(V.cnt_g); fr(V.nm_g); fr(V.npart_g); fr(V.cntx_g); fr(V.split_stat); fr(V.mem_g); fr(V.adj_g); fr(V.gout); fr(V.hw); fr(V.M); fr(V.selw); fr(V.wm); fr(V.mcnt); fr(V.fc2); fr(V.fl2); fr(V.fc_ticket);
    if (V.mail_h) (void)hipHostFree(V.mail_h);
    if (V.gout_h) (void)hipHostFree(V.gout_h);
    V = Rounds2Buf();
}
static hipError_t r2_prune_classify_grant(int d, int lds);
static int rounds2_split_stats(bslv_poly *h, long out[2])
{
    int c[2] = {0, 0};
    if (h->rounds2 && h->rounds2->split_stat) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(c, h->rounds2->split_stat, sizeof c, hipMemcpyDeviceToHost));
    }
    out[0] = c[0]; out[1] = c[1];
    return 0;
}
static int rounds2_ensure(bslv_poly *h, Rounds2Buf &V, int Bc)
{
    hipStream_t s = h->stream;
    int rc;
    if (!V.st_d) {
        HIP_TRY(malloc0(&V.st_d, sizeof(RState)));
        HIP_TRY(hipHostMalloc(&V.mail_h, R2_MAILS * sizeof(RState), hipHostMallocMapped | hipHostMallocCoherent));       // (a ring: rounds are queued ahead of the host)
        HIP_TRY(hipHostGetDevicePointer((void **)&V.mail_d, V.mail_h, 0));
        memset(V.mail_h, 0, R2_MAILS * sizeof(RState));
        HIP_TRY(malloc0(&V.gout, 4 * sizeof(int)));
        HIP_TRY(malloc0(&V.split_stat, 2 * sizeof(int)));
        HIP_TRY(hipMemsetAsync(V.split_stat, 0, 2 * sizeof(int), s));
        HIP_TRY(hipHostMalloc(&V.gout_h, 4 * sizeof(int)));
        HIP_TRY(malloc0(&V.M, (size_t)R2_MAXC * (R2_MAXC / 32) * sizeof(unsigned)));
        HIP_TRY(malloc0(&V.selw, 64 * sizeof(unsigned)));
        HIP_TRY(malloc0(&V.mcnt, (size_t)R2_MAXC * sizeof(int)));
        if (hipFuncSetAttribute((const void *)k_r2_select3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((R2_MAXC / 32) * R2_MLD * sizeof(unsigned))) != hipSuccess ||
            hipFuncSetAttribute((const void *)k_r2_minit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(((size_t)R2_MAXC * (R2_MAXC / 32 + 1) + R2_MAXC + 64) * sizeof(unsigned))) != hipSuccess) {
            (void)hipGetLastError();
            h->r2_mis = false;               // (no room for the matrix in LDS: the local-minima rule of round 2)
        }
        // the prunes' LDS for the kernel that also classifies, as bslv_poly_create asks for k2_fused_t (refused: two launches when the prunes want more than 48 KB)
        if (r2_prune_classify_grant(h->d, 128 * 1024) != hipSuccess) { (void)hipGetLastError(); V.ride_lds = 48 * 1024; }
    }
    if (h->P.cap > V.wmcap) { if ((rc = grow(&V.wm, (size_t)V.wmcap, (size_t)h->P.cap, s, true))) return rc; V.wmcap = h->P.cap; }
    if (Bc > V.bcap) {
        const int nc = std::max(Bc, 1024), nw = (nc + 31) / 32 + 2;
        if ((rc = grow(&V.alive, 0, (size_t)nw, s))) return rc;
        if ((rc = grow(&V.alive_prev, 0, (size_t)nw, s))) return rc;
        if ((rc = grow(&V.anym, 0, (size_t)nw, s))) return rc;
        if ((rc = grow(&V.bad, 0, (size_t)nw, s))) return rc;
        if ((rc = grow(&V.selmap, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.sel, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.order, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.rcflag, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.cnt_g, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.nm_g, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&V.mem_g, 0, (size_t)nc * K2_MAXNM, s))) return rc;
        if ((rc = grow(&V.adj_g, 0, (size_t)nc * R2_ADJW, s, true))) return rc;         // (zero: what the parts of a split prune rely on, k_r2_k2emit keeps it so)
        if ((rc = grow(&V.npart_g, 0, (size_t)nc, s, true))) return rc;
        if ((rc = grow(&V.cntx_g, 0, (size_t)nc * (K2_MAXPARTS - 1), s, true))) return rc;
        V.bcap = nc; V.scap = nc;
    }
    if (h->P.cap > V.vcap) { if ((rc = grow(&V.own, 0, (size_t)h->P.cap, s))) return rc; V.vcap = h->P.cap; }
    return 0;
}
template <class... A>
static void launch_r2_emit(int d, dim3 grid, hipStream_t s, A... a)
{
    switch (d) {
#define CASE(D) case D: hipLaunchKernelGGL(k_r2_emit<D>, grid, dim3(PB), 0, s, a...); break;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
    default: hipLaunchKernelGGL(k_r2_emit<0>, grid, dim3(PB), 0, s, a...); break;
    }
}
template <class... A>
static void launch_r2_classify3(int d, dim3 grid, hipStream_t s, A... a)
{
    switch (d) {
#define CASE(D) case D: hipLaunchKernelGGL(k_r2_classify3<D>, grid, dim3(PB), 0, s, a...); break;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
    default: hipLaunchKernelGGL(k_r2_classify3<0>, grid, dim3(PB), 0, s, a...); break;
    }
}
// the kernel of a round's prunes with the classification riding along: launch / grant of its dynamic LDS, by dimension
template <class... A>
static void launch_r2_prune_classify(int d, dim3 grid, size_t lds, hipStream_t s, A... a)
{
    switch (d) {
#define CASE(D) case D: hipLaunchKernelGGL(k_r2_prune_classify<D>, grid, dim3(K2T), lds, s, a...); break;
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
    default: hipLaunchKernelGGL(k_r2_prune_classify<0>, grid, dim3(K2T), lds, s, a...); break;
    }
}
static hipError_t r2_prune_classify_grant(int d, int lds)
{
    switch (d) {
#define CASE(D) case D: return hipFuncSetAttribute((const void *)k_r2_prune_classify<D>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
    default: return hipFuncSetAttribute((const void *)k_r2_prune_classify<0>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
}
// host: one attempt to take the round state for `seq` (as mail_try_read does for a Mail)
static inline bool rstate_try_read(const volatile RState *m, int seq, RState *out, long *torn)
{
    if (m->seq != seq) return false;
    __sync_synchronize();
    RState c;
    memcpy((void *)&c, (const void *)m, sizeof c);
    if (c.seq == seq) {
        const unsigned chk = c.chk;
        c.chk = 0; c.seq = 0;
        if (rstate_sum(c, seq) == chk) { c.chk = chk; c.seq = seq; *out = c; return true; }
    }
    if (torn) ++*torn;                                 // seq is there, (part of) the state is not yet: read again
    return false;
}
static int r2_wait(bslv_poly *h, Rounds2Buf &V, int seq, RState *out)
{
    volatile RState *m = V.mail_h + (seq % R2_MAILS);
    long torn = 0, drained = 0;
    for (long spin = 0; !rstate_try_read(m, seq, out, &torn); spin++) {
        if ((spin & 0xFFFF) == 0xFFFF) {
            hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess && ++drained > 1024) {      // the stream has long drained: nothing more will arrive
                set_error("poly engine: the round mailbox never reached a consistent state for seq %d (seq there: %d, %ld torn reads)", seq, (int)m->seq, torn);
                return BSLV_E_STATE;
            }
            if (e != hipSuccess && e != hipErrorNotReady) { set_error("poly engine: stream error %s", hipGetErrorString(e)); return BSLV_E_NODEVICE; }
        }
    }
    h->r2_torn_reads += torn;
    if (torn) { static const bool rep = getenv("BSLV_R2_REPORT") != nullptr; if (rep) fprintf(stderr, "r2: mailbox seq %d arrived before its state: %ld reads repeated\n", seq, torn); }
    return 0;
}

// The cuts todo[] (indices into the chunk's classification: h->clsw holds the class words of every element for its Bc cuts,
// h->hps_d their halfspaces) in rounds of independent cuts.  Precondition: hot mode, no prune in flight.
// left_out: cuts that were NOT dealt with (the element arrays would have had to grow, which moves the class words): the
// caller applies them one at a time.  Ranks are given in the order of application; h->facet_of_rank is extended here.
static int run_rounds2(bslv_poly *h, RoundsBuf &R, const std::vector<int> &todo, const std::vector<int> &fid_local, const std::vector<int> &rem, int *rc_out,
                       int Bc, int nw, std::vector<int> &left_out)
{
    left_out.clear();
    h->r2_deferred = false;
    if (!h->hot || h->pend_k2) { set_error("internal: run_rounds2 in the wrong state"); return BSLV_E_STATE; }
    if (!h->rounds2) h->rounds2 = new Rounds2Buf();
    Rounds2Buf &V = *h->rounds2;
    hipStream_t s = h->stream;
    const int d = h->d;
    int rc;
    if ((rc = rounds2_ensure(h, V, Bc))) return rc;
    if ((rc = rounds_ensure(h, R, Bc))) return rc;
    const int nw32 = (Bc + 31) / 32;
    const bool mis = h->r2_mis && Bc <= R2_MAXC;
    int nwp = 1;
    while (nwp < nw) nwp <<= 1;
    {   // alive set (the priority of a cut is its index: the caller has shuffled the chunk), state
        std::vector<unsigned> alive(nw32 + 2, 0u);
        for (int k : todo) alive[k >> 5] |= 1u << (k & 31);
        HIP_TRY(hipMemcpyAsync(V.alive, alive.data(), (nw32 + 2) * sizeof(unsigned), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(V.anym, 0, (nw32 + 2) * sizeof(unsigned), s));
        HIP_TRY(hipMemsetAsync(V.bad, 0, (nw32 + 2) * sizeof(unsigned), s));
        HIP_TRY(hipMemsetAsync(V.rcflag, 0xFF, (size_t)Bc * sizeof(int), s));
        RState st0;
        memset(&st0, 0, sizeof st0);
        st0.nv = h->nv; st0.ne = h->ne; st0.nranks = (int)h->facet_of_rank.size(); st0.poolused = h->poolused;
        HIP_TRY(hipMemcpyAsync(V.st_d, &st0, sizeof st0, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));              // (the staging vectors die here)
    }
    {   // element-major copy of the class words of the hot elements
        const size_t need = (size_t)h->P.cap * nw;
        if (need > V.hwcap) { if ((rc = grow(&V.hw, 0, need, s))) return rc; V.hwcap = need; }
        const long long items = (long long)vm_count(h->P, h->nv) * nw;
        if (mis) {
            const int nel = vm_count(h->P, h->nv);
            if (nel > 0) hipLaunchKernelGGL(k_r2_words3, dim3((nel + PB - 1) / PB), dim3(PB), 0, s, h->P, (const unsigned long long *)h->clsw, nw, h->nv, V.hw, V.wm);
        } else if (items > 0) hipLaunchKernelGGL(k_r2_words, dim3((unsigned)((items + PB - 1) / PB)), dim3(PB), 0, s, h->P, (const unsigned long long *)h->clsw, nw, h->nv, V.hw);
        HIP_TRY(hipGetLastError());
    }
    if (mis) {   // conflict matrix and MINUS counts start from zero (k_r2_select3 hands them back that way after every round)
        HIP_TRY(hipMemsetAsync(V.M, 0, (size_t)Bc * nw * sizeof(unsigned), s));
        HIP_TRY(hipMemsetAsync(V.mcnt, 0, (size_t)Bc * sizeof(int), s));
    }
    const int rank0 = (int)h->facet_of_rank.size();
    {   // arrays indexed by facet rank: every cut of the chunk may add one
        const int nranks = rank0 + Bc + 1;
        if (nranks > h->fcap) {
            int nc = std::max(nranks + 1024, h->fcap * 2);
            if ((rc = grow(&h->fstamp, (size_t)h->fcap, (size_t)nc, s, true))) return rc;
            if ((rc = grow(&h->flocal, 0, (size_t)nc, s))) return rc;
            if ((rc = grow(&h->zrows, 0, (size_t)ZMAX * nc, s, true))) return rc;
            if ((rc = grow(&h->fcount, 0, (size_t)nc, s, true))) return rc;
            if (!h->nlocal && (rc = grow(&h->nlocal, 0, 4, s, true))) return rc;
            h->fcap = nc;
        }
    }
    {   // slices of facet counters for the prunes whose member lists do not fit the LDS hash table (K2V2::fc2): zero between uses
        static const int want = getenv("BSLV_R2_FC_SLICES") ? std::max(0, atoi(getenv("BSLV_R2_FC_SLICES"))) : 64;
        if (want > 0 && V.fc_stride < h->fcap) {
            if (V.fc2) (void)hipFree(V.fc2);
            if (V.fl2) (void)hipFree(V.fl2);
            V.fc2 = V.fl2 = nullptr; V.fc_slices = 0;
            const size_t stride = (size_t)h->fcap;
            const int nsl = (int)std::max<size_t>(4, std::min<size_t>((size_t)want, ((size_t)1 << 30) / (stride * sizeof(int))));      // at most 1 GiB per array
            if (hipMalloc((void **)&V.fc2, (size_t)nsl * stride * sizeof(int)) == hipSuccess && malloc0s(&V.fl2, (size_t)nsl * stride * sizeof(int), s) == hipSuccess) {
                HIP_TRY(hipMemsetAsync(V.fc2, 0, (size_t)nsl * stride * sizeof(int), s));       // (the prunes rely on these zeros and leave them behind)
                V.fc_slices = nsl; V.fc_stride = (int)stride;
            } else {                                       // (no memory for them: such prunes take the multi-kernel path, as before)
                (void)hipGetLastError();
                if (V.fc2) (void)hipFree(V.fc2);
                V.fc2 = V.fl2 = nullptr; V.fc_stride = h->fcap;
            }
        }
        if (!V.fc_ticket) { HIP_TRY(malloc0s(&V.fc_ticket, 2 * sizeof(int), s)); }
        HIP_TRY(hipMemsetAsync(V.fc_ticket, 0, 2 * sizeof(int), s));
    }
    h->pre_f = -1;
    const bool dbg = getenv("BSLV_R2_DEBUG") != nullptr;
    int napplied = 0, nredundant = 0;
    long rounds = 0;
    int last_ncross = 0, max_S = 0;
    bool stop = false;                 // the element arrays would have to grow
    std::vector<int> order_h;
    auto pull_order = [&](int upto) -> int {          // ranks rank0.. -> dual slots, for everything applied so far
        if (upto <= (int)order_h.size()) return 0;
        const int from = (int)order_h.size();
        order_h.resize(upto);
        HIP_TRY(hipMemcpy(order_h.data() + from, V.order + from, (size_t)(upto - from) * sizeof(int), hipMemcpyDeviceToHost));
        for (int j = from; j < upto; j++) h->facet_of_rank.push_back(fid_local[order_h[j]]);
        return 0;
    };
    bool reported = false;
    auto check_edges = [&](const char *where, long round) -> int {
        if (!dbg || atoi(getenv("BSLV_R2_DEBUG")) < 2 || h->ne == 0) return 0;
        HIP_TRY(hipMemsetAsync(V.gout, 0, 4 * sizeof(int), s));
        hipLaunchKernelGGL(k_r2_check_edges, dim3((h->ne + 255) / 256), dim3(256), 0, s, h->P, (const int2 *)h->E[h->ecur], h->ne, V.gout);
        HIP_TRY(hipMemcpyAsync(V.gout_h, V.gout, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (V.gout_h[0]) {
            fprintf(stderr, "r2 check (%s, round %ld): %d edges with a dead end; first: edge %d = (%d, %d), ne %d nv %d nv_base %d\n", where, round, V.gout_h[0], V.gout_h[1], V.gout_h[2], V.gout_h[3], h->ne, h->nv, h->P.nv_base);
            if (!reported) {
                reported = true;
                RState mm = V.mail_h[V.seq % R2_MAILS];
                std::vector<int> mem((size_t)std::max(mm.nzero, 1)), cnt(mm.S), nmv(mm.S);
                (void)hipMemcpy(mem.data(), h->members, (size_t)mm.nzero * 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(cnt.data(), V.cnt_g, (size_t)mm.S * 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(nmv.data(), V.nm_g, (size_t)mm.S * 4, hipMemcpyDeviceToHost);
                fprintf(stderr, "  ZERO list (%d):", mm.nzero);
                for (int k = 0; k < mm.nzero; k++) { int co = -9; (void)hipMemcpy(&co, h->rounds->cutof + mem[k], 4, hipMemcpyDeviceToHost); fprintf(stderr, " %d/%d", mem[k], co); }
                fprintf(stderr, "\n");
                for (int sx = 0; sx < mm.S; sx++) {
                    std::vector<int> mg((size_t)std::max(nmv[sx], 1));
                    (void)hipMemcpy(mg.data(), V.mem_g + (size_t)sx * K2_MAXNM, (size_t)std::min(nmv[sx], K2_MAXNM) * 4, hipMemcpyDeviceToHost);
                    fprintf(stderr, "  cut %d: nm %d adjacent pairs %d members:", sx, nmv[sx], cnt[sx]);
                    for (int k = 0; k < std::min(nmv[sx], K2_MAXNM); k++) fprintf(stderr, " %d", mg[k]);
                    fprintf(stderr, "\n");
                }
            }
        }
        return 0;
    };
    if ((rc = check_edges("start of the chunk", 0))) return rc;
    // ---- the rounds.  Round r + 1 is queued BEHIND round r before the host has read r's mailbox (h->r2_spec; the kernels take
    // their sizes from the device state, the grids are sized for what a round may add, and whatever the host would have to
    // deal with first raises `halt` on the device: see RState).  The host follows one round behind.
    const int depth = (h->r2_spec && !dbg) ? 1 : 0;
    std::deque<std::pair<int, int>> inflight;      // (sequence number, S_ub of the launch)
    int cur = h->ecur;                              // buffer the next launch reads (every launch assumes the one before it went ahead)
    int gv = 8192, ge = 16384;                      // what a round may add to the elements / edges: bounds of the grids of a launch queued ahead
    int max_dv = 0, max_de = 0;
    bool stop_enq = false;
    auto clear_halt = [&]() -> int { HIP_TRY(hipMemsetAsync(&V.st_d->halt, 0, 2 * sizeof(int), s)); return 0; };      // (halt, halt2)
    auto drain = [&]() -> int {                      // rounds queued behind an exception found the device halted and did nothing
        while (!inflight.empty()) {
            RState x;
            if ((rc = r2_wait(h, V, inflight.front().first, &x))) return rc;
            inflight.pop_front();
            h->r2_spec_void++;
        }
        cur = h->ecur;
        return 0;
    };
    auto launch_round = [&](bool ahead, int *seq_out, int *sub_out) -> int {
        // sizes: confirmed ones when nothing is in flight, else what the round in flight may have made of them
        const int nv = h->nv + (ahead ? gv : 0), ne = h->ne + (ahead ? ge : 0);
        const int nbv = (vm_count(h->P, std::min(nv, h->P.cap)) + PB - 1) / PB, nbe = std::max(1, (std::min(ne, h->ecap) + PB - 1) / PB);
        Tri *ebsum = h->bsum, *vbsum = h->bsum + nbe + 1;
        const int cslot = next_counter_slot(h);
        if (cslot < 0) { set_error("hipMemsetAsync failed"); return BSLV_E_NODEVICE; }
        int *counters = h->counters + CSTRIDE * cslot;
        const ZMarks Z{h->zlist + ZMAX * cslot, h->zrows, h->fcap, (int)h->cutseq};
        const int2 *Eold = h->E[cur];
        int2 *Enew = h->E[1 - cur];
        if (mis) {
            {
                const int items = ne + vm_count(h->P, std::min(nv, h->P.cap));
                static const int wgmax = getenv("BSLV_R2_MINIT_WG") ? std::max(1, atoi(getenv("BSLV_R2_MINIT_WG"))) : 256;
                const int nwg = std::max(1, std::min(wgmax, (items + 1023) / 1024));
                static const int probe_at = getenv("BSLV_R2_MINIT_PROBE") ? atoi(getenv("BSLV_R2_MINIT_PROBE")) : -1;
                static int probe_n = 0;
                static unsigned long long *probe_d = nullptr;
                unsigned long long *probe = nullptr;
                if (probe_at >= 0) {
                    if (!probe_d) (void)hipMalloc(&probe_d, 256 * 16 * sizeof(unsigned long long));
                    const int pos = (int)rounds + (int)inflight.size();      // (round of the chunk)
                    if (probe_n++ >= probe_at && pos == (getenv("BSLV_R2_MINIT_PROBE_POS") ? atoi(getenv("BSLV_R2_MINIT_PROBE_POS")) : 0) && probe_n < 1000000) {
                        probe = probe_d; probe_n = 1000000;
                        (void)hipMemsetAsync(probe_d, 0, 256 * 16 * sizeof(unsigned long long), s);
                    }
                }
                hipLaunchKernelGGL(k_r2_minit, dim3(nwg), dim3(1024), ((size_t)Bc * (nw + 1) + Bc + nw) * sizeof(unsigned), s, h->P, (const unsigned long long *)V.hw, (const unsigned *)V.wm, nw, Bc,
                                   (const RState *)V.st_d, Eold, (const unsigned *)V.alive, V.M, V.mcnt, (const int *)R.tc, V.st_d, std::min(ne, h->ecap), vm_count(h->P, std::min(nv, h->P.cap)), probe);
                if (probe) {
                    std::vector<unsigned long long> pr(256 * 16);
                    (void)hipStreamSynchronize(s);
                    (void)hipMemcpy(pr.data(), probe_d, pr.size() * 8, hipMemcpyDeviceToHost);
                    unsigned long long t0 = ~0ull, t4 = 0;
                    for (int g = 0; g < nwg; g++) { t0 = std::min(t0, pr[g * 16]); t4 = std::max(t4, pr[g * 16 + 4]); }
                    fprintf(stderr, "minit probe: nwg %d items %d (ne %d) Bc %d nw %d round %d, whole %.1f us\n", nwg, items, ne, Bc, nw, (int)rounds + (int)inflight.size(), (t4 - t0) / 100.0);
                    const char *nm[4] = {"zero", "items", "queue", "or"};
                    for (int k = 0; k < 4; k++) {
                        double mn = 1e30, mx = 0, sm = 0;
                        for (int g = 0; g < nwg; g++) { const double d = (pr[g * 16 + k + 1] - pr[g * 16 + k]) / 100.0; mn = std::min(mn, d); mx = std::max(mx, d); sm += d; }
                        fprintf(stderr, "  %-6s min %.1f mean %.1f max %.1f us\n", nm[k], mn, sm / nwg, mx);
                    }
                    double st_mn = 1e30, st_mx = 0, qs = 0, qmx = 0, nz = 0;
                    for (int g = 0; g < nwg; g++) { const double d = (pr[g * 16] - t0) / 100.0; st_mn = std::min(st_mn, d); st_mx = std::max(st_mx, d); qs += pr[g * 16 + 6]; qmx = std::max(qmx, (double)pr[g * 16 + 6]); nz += pr[g * 16 + 7]; }
                    { double a = 0, b2 = 0, c = 0, d2 = 0; for (int g = 0; g < nwg; g++) { a += pr[g * 16 + 8]; b2 += pr[g * 16 + 9]; c += pr[g * 16 + 10]; d2 = std::max(d2, (double)pr[g * 16 + 11]); }
                      fprintf(stderr, "  per wave (mean over %d waves): resolve + first fetch %.1f us, giving %.1f us, waiting for the next item's words %.1f us; slowest wave %.1f us\n", nwg * 16, a / nwg / 16 / 100, b2 / nwg / 16 / 100, c / nwg / 16 / 100, d2 / 100); }
                    fprintf(stderr, "  start skew max %.1f us; queue items mean %.0f max %.0f; non-zero words per wg %.0f\n", st_mx, qs / nwg, qmx, nz / nwg);
                }
            }
            hipLaunchKernelGGL(k_r2_select3, dim3(1), dim3(1024), (size_t)nw * R2_MLD * sizeof(unsigned), s, Bc, nw, V.alive, V.alive_prev, V.M, V.mcnt,
                               V.selmap, V.sel, V.order, V.rcflag, V.st_d, V.selw, depth);
            hipLaunchKernelGGL(k_r2_assign3, dim3(nbv), dim3(PB), 0, s, h->P, (const unsigned long long *)V.hw, (const unsigned *)V.wm, nw, (const RState *)V.st_d, (const unsigned *)V.selw,
                               (const int *)V.selmap, R.cutof, counters, h->zlist + ZMAX * cslot);
        } else {
            hipLaunchKernelGGL(k_r2_prep, dim3(nbe + nbv), dim3(PB), (size_t)(3 * nw + 2) * sizeof(unsigned), s, h->P, (const unsigned long long *)V.hw, nw,
                               (const RState *)V.st_d, Eold, nbe, (const unsigned *)V.alive, V.anym, V.bad, V.own, (const int *)R.tc, V.st_d);
            hipLaunchKernelGGL(k_r2_select, dim3(1), dim3(1024), 0, s, Bc, V.alive, V.alive_prev, V.anym, V.bad, V.selmap, V.sel, V.order, V.rcflag, V.st_d, depth);
            hipLaunchKernelGGL(k_r2_assign, dim3(nbv), dim3(PB), 0, s, h->P, (const unsigned long long *)V.hw, nw, (const RState *)V.st_d, (const int *)V.own,
                               (const int *)V.selmap, R.cutof, counters, h->zlist + ZMAX * cslot);
        }
        hipLaunchKernelGGL(k_flags2, dim3(nbe + nbv), dim3(PB), 0, s, h->P, Eold, ne, (const int *)&V.st_d->ne, nbe, nv, (const int *)counters, h->eflag, h->ecount, ebsum, vbsum, Z, (const int *)&V.st_d->nv,
                           (const int *)&V.st_d->halt, mis ? R2Own{(const int *)R.cutof, (const unsigned long long *)V.hw, (const unsigned *)V.wm, (const unsigned *)V.selw, (const int *)V.selmap, nw}
                                                           : R2Own{nullptr, nullptr, nullptr, nullptr, nullptr, 0});
        launch_r2_emit(d, dim3(nbe + nbv), s, h->P, (const double *)h->hps_d, (const int *)V.sel, R.cutof, Eold, nbe, (const unsigned char *)h->eflag, (const int *)h->ecount,
                       (const Tri *)ebsum, (const Tri *)vbsum, Enew, h->members, (const int *)counters, V.st_d, h->P.cap, h->ecap, h->poolcap,
                       (const int *)h->EP[cur], h->EP[1 - cur], Z, (const unsigned long long *)V.hw, (const unsigned *)V.wm, nw, (int *)nullptr,
                       (const unsigned *)V.selw, (const int *)V.selmap);
        const int S_ub = std::max(1, std::min(Bc - napplied - nredundant, V.scap));
        const K2V2 KV{V.st_d, R.cutof, V.mem_g, V.adj_g, V.cnt_g, V.nm_g, R2_ADJW, &V.st_d->pair_tests, V.fc2, V.fl2, V.fc_ticket, V.fc2 ? V.fc_slices : 0, V.fc_stride,
                      V.npart_g, V.cntx_g, 0, h->r2_split_min, h->r2_split_parts, V.split_stat};
        const int seq = ++V.seq;
        // the new vertices of the round against the cuts that are still alive: workgroups that stride over whatever the round made.  Nothing
        // reads these class words before the next round's k_r2_minit, and the prunes read none: the classification rides along in
        // the launch of the prunes (k_r2_prune_classify) unless BSLV_R2_RIDE=0 asks for the two launches
        const int want = std::max(2048, 2 * last_ncross);
        if (h->r2_ride && h->k2_lds <= V.ride_lds) {
            // G workgroups, in each of which r2_ride_threads threads work (PB, the shape of k_r2_classify3: see the kernel), enough for `want`
            // vertices in one pass, at most r2_ride_gmax: each holds the LDS of a CU like a prune does; the prunes are dispatched first
            const int nthr = std::max(h->r2_ride_threads, std::min(nwp, K2T));
            const int vpb = std::max(1, nthr / nwp), G = std::max(1, std::min(h->r2_ride_gmax, (want + vpb - 1) / vpb));
            // ... and behind the prunes a pool of helper workgroups, which take parts of the round's large prunes (k2v2_assign); a helper
            // with nothing dealt to it returns after its scan of the candidates
            K2V2 KH = KV;
            KH.helpers = h->r2_split ? h->r2_split_helpers : 0;
            launch_r2_prune_classify(d, dim3(S_ub + KH.helpers + G), h->k2_lds, s, h->P, h->members, h->fcount, h->flocal, (int)(h->k2_lds / 8), Enew, h->totals + 2, h->k2mail_d, h->k2dbg, h->abort_d,
                                     Hp{}, KH, (const double *)h->hps_d, Bc, nw, nwp, (const unsigned *)V.alive, V.hw, V.wm, G, nthr, mis ? 1 : 0, h->r2_ride_lds ? 1 : 0);
        } else {
            launch_r2_classify3(d, dim3(std::max(1, std::min(4096, (want + PB / nwp - 1) / (PB / nwp)))), s, h->P, (const double *)h->hps_d, Bc, nw, nwp, (const RState *)V.st_d,
                                (const unsigned *)V.alive, V.hw, V.wm, (int *)nullptr, mis ? 1 : 0);
            hipLaunchKernelGGL(k2_fused_t<true>, dim3(S_ub), dim3(K2T), h->k2_lds, s, h->P, h->members, 0, 0, 0, h->fcount, h->flocal, (int)(h->k2_lds / 8), Enew, 0,
                               (int *)nullptr, h->totals + 2, h->k2mail_d, 0, h->k2dbg, (const CutDev *)nullptr, h->abort_d, (int *)nullptr, Hp{}, (int *)nullptr,
                               (int *)nullptr, KV);
        }
        hipLaunchKernelGGL(k_r2_k2emit, dim3(S_ub), dim3(K2T), 0, s, V.st_d, (const int *)V.cnt_g, (const int *)V.nm_g, V.adj_g, (const int *)V.npart_g, (const int *)V.cntx_g,
                           (const int *)V.mem_g, R2_ADJW, Enew, h->EP[1 - cur], h->ecap, V.mail_d + (seq % R2_MAILS), seq);
        HIP_TRY(hipGetLastError());
        cur = 1 - cur;
        *seq_out = seq; *sub_out = S_ub;
        return 0;
    };
    // what must hold before a round is queued: capacities that only the host can raise (nothing may be in flight while it does)
    auto prepare = [&](bool ahead) -> int {            // 0 ok, -1 "not now" (ahead only), > 0 error
        const int nv = h->nv + (ahead ? gv : 0), ne = h->ne + (ahead ? ge : 0);
        const int nbv = (vm_count(h->P, std::min(nv, h->P.cap)) + PB - 1) / PB, nbe = std::max(1, (std::min(ne, h->ecap) + PB - 1) / PB);
        const size_t pool_need = (size_t)h->poolused + (size_t)(ahead ? 4 : 1) * 65536;
        if (ahead) {
            if (nbe + nbv + 2 > h->bsumcap || pool_need > h->poolcap || h->ecap > h->ecountcap) return -1;
            return 0;
        }
        // head-room of a round; the pool may grow (a pointer in the view), the element arrays may not (stride of the class words)
        if ((rc = ensure_pool(h, pool_need + (depth ? 8 * 65536 : 0)))) return rc;
        if (h->ecap > h->ecountcap) { if ((rc = grow(&h->ecount, 0, (size_t)h->ecap, s))) return rc; h->ecountcap = h->ecap; }
        const int nbv2 = (vm_count(h->P, std::min(h->nv + 2 * gv, h->P.cap)) + PB - 1) / PB, nbe2 = std::max(1, (std::min(h->ne + 2 * ge, h->ecap) + PB - 1) / PB);
        if ((rc = ensure_bsum(h, std::max(nbe + nbv, depth ? nbe2 + nbv2 : 0) + 2))) return rc;
        return 0;
    };
    for (;;) {
        // queue: one round when nothing is in flight, one more behind it when the rounds run ahead of the host
        while (!stop_enq && (int)inflight.size() <= depth) {
            const bool ahead = !inflight.empty();
            const int pr = prepare(ahead);
            if (pr < 0) break;
            if (pr > 0) return pr;
            int sq = 0, sub = 0;
            if ((rc = launch_round(ahead, &sq, &sub))) return rc;
            inflight.emplace_back(sq, sub);
        }
        if (inflight.empty()) break;                       // (stop_enq and everything queued has been dealt with)
        int seq = inflight.front().first;
        const int S_ub = inflight.front().second;
        inflight.pop_front();
        const int nv = h->nv, ne = h->ne;
        RState m;
        if ((rc = r2_wait(h, V, seq, &m))) return rc;
        if (m.halt == 2) {
            // a round queued ahead found its grids too small for what the round before it had made: nothing but marks was written
            if ((rc = drain())) return rc;
            HIP_TRY(hipMemsetAsync(V.anym, 0, (nw32 + 2) * sizeof(unsigned), s));
            HIP_TRY(hipMemsetAsync(V.bad, 0, (nw32 + 2) * sizeof(unsigned), s));
            if (mis) {
                HIP_TRY(hipMemsetAsync(V.M, 0, (size_t)Bc * nw * sizeof(unsigned), s));
                HIP_TRY(hipMemsetAsync(V.mcnt, 0, (size_t)Bc * sizeof(int), s));
            }
            if ((rc = clear_halt())) return rc;
            gv *= 4; ge *= 4;
            h->r2_spec_void++;
            continue;
        }
        if (dbg) fprintf(stderr, "r2 round %d: S %d alive %d redundant %d | go %d declined %d nminus %d nzero %d nsurv %d ncross %d pairs %d eover %d k2abort %d | nv %d ne %d pool %u\n",
                         m.round, m.S, m.nalive, m.nredundant, m.go, m.declined, m.nminus, m.nzero, m.nsurv, m.ncross, m.epairs, m.eover, m.k2abort, m.nv, m.ne, m.poolused);
        if (m.err && getenv("BSLV_R2_DEBUG")) {
            for (int which = 0; which < 2; which++) {
                const int el = m.err_info[1 + which], k = m.err_info[4];
                unsigned char fl = 0; int tcv = -7, ownv = -7; unsigned long long wm = 0, we = 0; signed char cl = 0; int co = -7;
                (void)hipMemcpy(&fl, h->P.flag + el, 1, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&tcv, R.tc + el, 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&ownv, V.own + el, 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&co, R.cutof + el, 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&cl, h->P.cls + el, 1, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&wm, h->clsw + (size_t)(k >> 5) * h->P.cap + el, 8, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&we, V.hw + (size_t)el * nw + (k >> 5), 8, hipMemcpyDeviceToHost);
                std::vector<double> hp(d + 3), x(d);
                (void)hipMemcpy(hp.data(), h->hps_d + (size_t)k * (d + 3), (d + 3) * 8, hipMemcpyDeviceToHost);
                for (int c = 0; c < d; c++) (void)hipMemcpy(&x[c], h->P.X + (size_t)c * h->P.cap + el, 8, hipMemcpyDeviceToHost);
                double sdot = 0; for (int c = 0; c < d; c++) sdot = fma(hp[c], x[c], sdot);
                int hvpos = -1;
                { std::vector<int> hv(h->P.nhv); if (h->P.nhv) (void)hipMemcpy(hv.data(), h->hv_d, (size_t)h->P.nhv * 4, hipMemcpyDeviceToHost); for (int t = 0; t < h->P.nhv; t++) if (hv[t] == el) hvpos = t; }
                fprintf(stderr, "r2 debug: element %d flag %d tc %d own %d cutof %d cls %d | class of cut %d: word-major %d, element-major %d | s %.17g alpha %.17g hi %.17g lo %.17g | position in hot list %d (nhv %d, nv_base %d, nv %d, cap %d)\n",
                        el, fl, tcv, ownv, co, cl, k, (int)((wm >> (2 * (k & 31))) & 3), (int)((we >> (2 * (k & 31))) & 3), sdot, hp[d], hp[d + 1], hp[d + 2], hvpos, h->P.nhv, h->P.nv_base, h->nv, h->P.cap);
            }
        }
        if (m.err == 4) {
            {
                const int el = m.err_info[3];
                std::vector<int> hv(std::max(h->P.nhv, 1));
                if (h->P.nhv) (void)hipMemcpy(hv.data(), h->hv_d, (size_t)h->P.nhv * 4, hipMemcpyDeviceToHost);
                int dups = 0, nondec = 0;
                std::string pos;
                for (int t = 0; t < h->P.nhv; t++) { if (hv[t] == el) pos += " " + std::to_string(t); if (t && hv[t] <= hv[t - 1]) nondec++; }
                std::vector<int> sorted(hv.begin(), hv.begin() + h->P.nhv); std::sort(sorted.begin(), sorted.end());
                for (int t = 1; t < h->P.nhv; t++) dups += sorted[t] == sorted[t - 1];
                std::vector<int> mem((size_t)std::max(m.nzero, 1));
                (void)hipMemcpy(mem.data(), h->members, (size_t)m.nzero * 4, hipMemcpyDeviceToHost);
                fprintf(stderr, "r2 debug: element %d in the hot list at:%s; hot list: %d entries, %d duplicates, %d not ascending; nv_base %d nv %d host nv %d; on-plane list:", el, pos.c_str(), h->P.nhv, dups, nondec,
                        h->P.nv_base, m.nv, h->nv);
                for (int t = 0; t < m.nzero; t++) fprintf(stderr, " %d", mem[t]);
                fprintf(stderr, "\n");
            }
            set_error("internal: round %d: member list of selected cut %d holds element %d twice (positions %d, %d); in the on-plane list at %d and %d of %d", m.round, m.err_info[0],
                      m.err_info[3], m.err_info[1], m.err_info[2], m.err_info[4], m.err_info[5], m.err_info[6]);
            return BSLV_E_STATE;
        }
        if (m.err == 3) {
            set_error("internal: round %d: the prune of selected cut %d emitted the pair (%d, %d) of its %d members: both are element %d (nzero %d)", m.err_info[6], m.err_info[0],
                      m.err_info[1], m.err_info[2], m.err_info[3], m.err_info[4], m.err_info[5]);
            return BSLV_E_STATE;
        }
        if (m.err) {
            set_error("internal: round %d: inconsistent crossing edge %d (minus end %d, plus end %d, selected cut %d = classified %d, classes %d, flag %d) hb %g hd %g a2 %g ideal %g xm %g %g %g %g xp %g %g %g %g nv_base %d nhv %d",
                      m.round, m.err_info[0], m.err_info[1], m.err_info[2], m.err_info[3], m.err_info[4], m.err_info[5], m.err_info[6],
                      m.err_d[0], m.err_d[1], m.err_d[2], m.err_d[3], m.err_d[4], m.err_d[5], m.err_d[6], m.err_d[7], m.err_d[8], m.err_d[9], m.err_d[10], m.err_d[11], h->P.nv_base, h->P.nhv);
            return BSLV_E_STATE;
        }
        if (m.stuck) { set_error("internal: a round selected no cut although %d are alive", m.nalive); return BSLV_E_STATE; }
        const bool removed_some = m.nredundant > nredundant;
        nredundant = m.nredundant;
        if (m.S == 0) {
            if ((rc = drain())) return rc;                    // (a round queued behind this one found the device halted)
            if ((m.halt || m.halt2) && (rc = clear_halt())) return rc;
            if (m.nalive == 0) break;                         // every cut is applied or redundant
            if (removed_some) continue;                       // (the round only retired redundant cuts, which had kept the others waiting)
            set_error("internal: a round selected no cut although %d are alive", m.nalive);
            return BSLV_E_STATE;
        }
        if (m.declined) {
            // a capacity was short: nothing but keep marks and the selection was written; take the selection back, grow, repeat
            h->r2_declined++;
            if ((rc = drain())) return rc;
            if ((rc = clear_halt())) return rc;
            hipLaunchKernelGGL(k_r2_undo, dim3((Bc + 255) / 256), dim3(256), 0, s, Bc, V.alive, (const unsigned *)V.alive_prev, (const int *)V.selmap, V.st_d);
            HIP_TRY(hipGetLastError());
            if (nv + m.ncross > h->P.cap) { stop = true; break; }
            if ((rc = ensure_pool(h, (size_t)h->poolused + (size_t)m.newlen + (size_t)m.zero_ub + 65536))) return rc;
            continue;
        }
        rounds++;
        napplied = m.napplied;
        // the round went ahead: the new lists are in the other buffers
        h->ecur = 1 - h->ecur;
        h->ne = m.ne_next;
        if (m.eover || m.k2abort > 0) {                      // (both raised halt2: whatever was queued behind did nothing)
            if ((rc = drain())) return rc;
            if ((rc = clear_halt())) return rc;
        }
        if (m.eover) {
            // the adjacent pairs did not fit behind the edges: grow (copies the new list) and emit again (the bitmaps are still there)
            if ((rc = ensure_ecap(h, m.ne_next + m.epairs + 1))) return rc;
            seq = ++V.seq;
            hipLaunchKernelGGL(k_r2_k2emit, dim3(S_ub), dim3(K2T), 0, s, V.st_d, (const int *)V.cnt_g, (const int *)V.nm_g, V.adj_g, (const int *)V.npart_g, (const int *)V.cntx_g,
                               (const int *)V.mem_g, R2_ADJW, h->E[h->ecur], h->EP[h->ecur], h->ecap, V.mail_d + (seq % R2_MAILS), seq);
            HIP_TRY(hipGetLastError());
            if ((rc = r2_wait(h, V, seq, &m))) return rc;
            if (m.eover) { set_error("internal: the edge list is still too short after growing"); return BSLV_E_STATE; }
            if (m.k2abort > 0 && (rc = clear_halt())) return rc;       // (the second emission raised it again for its fallback prunes)
        }
        max_dv = std::max(max_dv, m.nv - nv); max_de = std::max(max_de, m.ne - ne);
        gv = std::max(gv, 2 * max_dv + 2048); ge = std::max(ge, 2 * max_de + 4096);
        h->nv = m.nv; h->ne = m.ne; h->poolused = m.poolused;
        h->new_vertices += m.ncross;
        last_ncross = m.ncross;
        if (m.k2abort > 0) {
            // prunes that need the multi-kernel path (a facet too large for one workgroup, a bit matrix beyond LDS): one at a time
            if ((rc = pull_order(napplied))) return rc;
            std::vector<int> cnt(m.S), nmv(m.S);
            HIP_TRY(hipMemcpy(cnt.data(), V.cnt_g, (size_t)m.S * sizeof(int), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(nmv.data(), V.nm_g, (size_t)m.S * sizeof(int), hipMemcpyDeviceToHost));
            for (int sidx = 0; sidx < m.S; sidx++) if (cnt[sidx] < 0) {
                h->r2_fb_reason[std::min(4, -cnt[sidx])]++;
                int lg = 0; while ((1 << (lg + 1)) <= std::max(1, nmv[sidx]) && lg < 19) lg++;
                h->r2_fb_nm[lg]++;
            }
            const int nv0 = m.nv_next - m.ncross;
            if (m.nzero > 0) HIP_TRY(hipMemcpyAsync(R.zlist, h->members, (size_t)m.nzero * sizeof(int), hipMemcpyDeviceToDevice, s));
            for (int sidx = 0; sidx < m.S; sidx++) {
                if (cnt[sidx] >= 0) continue;
                hipLaunchKernelGGL(k_r2_gather, dim3(1), dim3(1024), 0, s, h->P, (const int *)R.zlist, m.nzero, nv0, m.ncross, (const int *)R.cutof, sidx, h->members, V.gout, m.rank_base);
                HIP_TRY(hipMemcpyAsync(V.gout_h, V.gout, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                const int nm = V.gout_h[0];
                const long long len_ub = V.gout_h[1];
                // a fresh stamp for the facet ids of this prune: the cut counter moves only through next_counter_slot(), which also
                // clears the ring of counters quarter by quarter (a bare ++ skipped a quarter boundary once in a while, and rounds
                // thousands of cuts later started from non-zero counters)
                if (next_counter_slot(h) < 0) { set_error("hipMemsetAsync failed"); return BSLV_E_NODEVICE; }
                h->pair_tests += (long)nm * (nm - 1) / 2;
                h->r2_fallback_prunes++;
                const int ne_before = h->ne;
                if (nm >= 2 && (rc = k2_multi(h, nm, len_ub, (int)(4 * h->cutseq + 3)))) return rc;
                if (mis && h->ne > ne_before) {
                    // pairs of shared on-plane members that a later cut of the round has the final word on (k_r2_dedupe_flags)
                    const int nadd = h->ne - ne_before, nbd = (nadd + PB - 1) / PB, myrank = m.rank_base + sidx;
                    if ((rc = ensure_bsum(h, nbd + 1))) return rc;
                    Tri td;
                    hipLaunchKernelGGL(k_r2_dedupe_flags, dim3(nbd), dim3(PB), 0, s, h->P, (const int *)R.cutof, (const int2 *)h->E[h->ecur], ne_before, nadd, myrank, h->bsum);
                    if ((rc = scan_totals(h, nbd, &td))) return rc;
                    if (td.a < nadd) {
                        int2 *scratch = h->E[1 - h->ecur];          // (the list the round has replaced: free until the next round writes it)
                        hipLaunchKernelGGL(k_r2_dedupe_emit, dim3(nbd), dim3(PB), 0, s, h->P, (const int *)R.cutof, (const int2 *)h->E[h->ecur], ne_before, nadd, myrank, (const Tri *)h->bsum, scratch);
                        HIP_TRY(hipGetLastError());
                        if (td.a > 0) HIP_TRY(hipMemcpyAsync(h->E[h->ecur] + ne_before, scratch, (size_t)td.a * sizeof(int2), hipMemcpyDeviceToDevice, s));
                        HIP_TRY(hipStreamSynchronize(s));
                        h->ne = ne_before + td.a;
                    }
                }
            }
            HIP_TRY(hipMemcpyAsync(&V.st_d->ne, &h->ne, sizeof(int), hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if ((rc = check_edges(m.k2abort ? "after a round with fallback prunes" : (m.eover ? "after a round with a second emission" : "after a round"), rounds))) return rc;
        if (h->P.cap - h->nv < 4096) { stop = true; stop_enq = true; continue; }      // (next to no room for another round's vertices; a round already queued is still dealt with)
        // a round costs about two single cuts.  When the cuts of a chunk form one clique (every round holds a single cut) what
        // is left goes through the single-cut pipeline; BSLV_R2_MIN_CUTS / debug key 8 set a stricter rule for experiments
        // thin rounds at the end of a chunk (its cliques: one cut each per round) are not worth their passes: the cuts still alive go
        // back to the caller, who hands them in again with the next batch, where they share rounds with cuts of other regions
        // (thin relative to what the chunk's rounds held at their best: a chunk of one clique has nothing but thin rounds)
        max_S = std::max(max_S, m.S);
        if (h->r2_defer > 0 && m.S < h->r2_defer && m.S * 5 < max_S && m.nalive > 0 && rounds >= 4) { stop = true; stop_enq = true; h->r2_deferred = true; }
        if (h->r2_min_cuts >= 0 && m.nalive >= 8 && rounds >= 16 && napplied * 4 < rounds * 5) { stop = true; stop_enq = true; }
        if (h->r2_min_cuts > 0 && m.nalive >= 8 && rounds >= 2 && napplied < h->r2_min_cuts * rounds) { stop = true; stop_enq = true; }
    }
    if (h->r2_deferred && h->r2_defer_mark) {
        // the elements the cuts handed back will remove take no LP in the meantime (k_r2_mark_doomed)
        const int nel = vm_count(h->P, h->nv);
        HIP_TRY(hipMemsetAsync(V.gout, 0, sizeof(int), s));
        if (nel > 0) hipLaunchKernelGGL(k_r2_mark_doomed, dim3((nel + PB - 1) / PB), dim3(PB), 0, s, h->P, (const unsigned long long *)V.hw, mis ? (const unsigned *)V.wm : (const unsigned *)nullptr, nw, h->nv,
                                        (const unsigned *)V.alive, V.gout);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(V.gout_h, V.gout, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->r2_doomed += V.gout_h[0];
    }
    // results: order of application -> ranks; per cut 0 applied / 1 redundant; what is left goes back to the caller
    if ((rc = pull_order(napplied))) return rc;
    std::vector<int> rcf(Bc);
    std::vector<unsigned> alive(nw32 + 2);
    HIP_TRY(hipMemcpy(rcf.data(), V.rcflag, (size_t)Bc * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(alive.data(), V.alive, (size_t)nw32 * sizeof(unsigned), hipMemcpyDeviceToHost));
    long long pt = 0;
    HIP_TRY(hipMemcpy(&pt, &V.st_d->pair_tests, sizeof pt, hipMemcpyDeviceToHost));
    h->pair_tests += (long)pt;
    for (int k : todo) {
        if ((alive[k >> 5] >> (k & 31)) & 1u) {
            left_out.push_back(k);                  // (its flag may be stale: a selection that was declined and taken back leaves it set)
            continue;
        }
        if (rcf[k] == 1) { h->fapplied[fid_local[k]] = 0; rc_out[rem[k]] = 1; }
        else if (rcf[k] == 0) rc_out[rem[k]] = 0;
        else { set_error("internal: cut %d of the chunk was neither applied nor found redundant", k); return BSLV_E_STATE; }
    }
    if (!stop && !left_out.empty()) {
        // The loop ended on "no cut alive" and yet the device's list holds untouched cuts.  Round 2 met this once and handed the
        // cuts back to the one-cut pipeline; the cause found since -- the host acting on the PREVIOUS mailbox content under the new
        // sequence number -- is excluded by the checksum of r2_wait, so this is an invariant again: an error with the mailbox in it.
        h->r2_late_left += (long)left_out.size();
        const RState mm = *const_cast<const RState *>(V.mail_h + (V.seq % R2_MAILS));
        set_error("internal: the rounds of a chunk ended on 'none alive' with %zu cuts still alive (mailbox: seq %d round %d S %d nalive %d napplied %d nredundant %d; host: seq %d napplied %d nredundant %d)",
                  left_out.size(), mm.seq, mm.round, mm.S, mm.nalive, mm.napplied, mm.nredundant, V.seq, napplied, nredundant);
        return BSLV_E_STATE;
    }
    h->cuts_applied += napplied;
    h->r2_rounds += rounds; h->r2_cuts += napplied; h->r2_chunks++;
    h->pre_f = -1;
    return 0;
}
