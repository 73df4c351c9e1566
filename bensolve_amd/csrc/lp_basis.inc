// lp_basis.inc -- a basis taken out of a slot and put into one (bslv_lpq_get_basis, bslv_lpq_load_basis, bslv_lpq_rebuild); included at
// the end of lp_engine.hip.  The tableau form's counterpart of the revised form's refactorisation (k_rfx_*): a slot's tableau rebuilt on
// the device from a list of statuses and the model, nothing numeric of the slot read.
// THE REPLAY OF THE TABLEAU FORM.  The slot starts as the standard image Tstd ([A ; cost]: basic = the auxiliary variables, nonbasic
// position j = structural j).  The structural basic variables of the target enter one after the other in ascending variable id, each on
// the row partial pivoting chooses -- the largest |v_i| of column q = k - M as it is after the pending steps (virt_entry) among the rows
// whose auxiliary variable is nonbasic in the target and that have not been pivoted yet, ties to the smallest i -- and every step is an
// ordinary pending pivot of the engine: a PivDesc, the pivot row as virt_entry sees it, the multipliers v_i / v_r with row M (the cost row
// of the image) among them.  KP steps between two passes of the existing k_flush, one refresh pass of it for the basic values and the
// objective at the end (beta = T x_N).  The heads move with the pivots as in a solve: position q ends holding structural q, or the
// auxiliary variable that left when structural q entered; statuses and values follow their variable (k_lb_finish).
// One workgroup per LP (NT_BIG threads from 1536 rows or columns on), no atomics in the arithmetic, every reduction in a fixed order: the
// result is a function of the statuses, the model and the bounds.  No existing kernel is changed.
// The revised form: k_lb_heads writes heads, positions, statuses and values from the list, then refactor_impl runs as it is.
namespace bslv {

// per LP of a call and variable of the engine's own model: the nonbasic status NS_* (-1: basic) and the nonbasic value
struct LbView { const int *nst; const double *xv; };

// tableau form: the standard heads into the slot, the entering list and the eligible rows from the statuses, the LP's batch record
// (RfxView as k_rfx_setup fills it: cnt = structural basics to enter, entered so far, state RFX_*, unused)
__global__ __launch_bounds__(NT) void k_lb_setup(LpView L, BatchView Bv, RfxView R, LbView Lb, int n)
{
    __shared__ int s_cnt[NT];
    __shared__ int s_ne, s_k;
    const int b = blockIdx.x, tid = threadIdx.x, M = L.M, N = L.N;
    if (b >= n) return;
    const int slot = Bv.dst[b];
    const int *nst = Lb.nst + (size_t)b * (M + N);
    int *enter = R.enter + (size_t)b * M, *rowvar = R.rowvar + (size_t)b * M, *elig = R.elig + (size_t)b * M;
    int *bh = L.bh + (size_t)slot * M, *nh = L.nh + (size_t)slot * N, *pos = L.pos + (size_t)slot * (M + N);
    // the structural basic variables in ascending id: thread t counts its stretch of the columns, a scan places it
    const int chunk = (N + NT - 1) / NT, j0 = min(N, tid * chunk), j1 = min(N, j0 + chunk);
    int c = 0;
    for (int j = j0; j < j1; j++) c += nst[M + j] < 0;
    s_cnt[tid] = c;
    if (tid == 0) s_ne = 0;
    __syncthreads();
    if (tid == 0) { int o = 0; for (int t = 0; t < NT; t++) { const int v = s_cnt[t]; s_cnt[t] = o; o += v; } }
    __syncthreads();
    int o = s_cnt[tid];
    for (int j = j0; j < j1; j++) if (nst[M + j] < 0) { if (o < M) enter[o] = M + j; o++; }
    if (tid == NT - 1) s_k = o;                 // (the last stretch ends where the list does)
    int ne = 0;
    for (int i = tid; i < M; i += NT) { const int e = nst[i] >= 0; elig[i] = e; rowvar[i] = i; ne += e; bh[i] = i; pos[i] = i; }
    for (int j = tid; j < N; j += NT) { nh[j] = M + j; pos[M + j] = -1 - j; }
    if (ne) atomicAdd(&s_ne, ne);               // (a count of rows: whole numbers, any order)
    __syncthreads();
    if (tid == 0) {
        int *cnt = R.cnt + (size_t)b * 4;
        cnt[0] = s_k; cnt[1] = 0; cnt[2] = (s_k == s_ne && s_k <= M) ? RFX_RUN : RFX_HEADS; cnt[3] = 0;
        Bv.status[b] = ST_RUNNING; Bv.iters[b] = 0; Bv.mode[b] = MODE_NONE; Bv.verified[b] = 0;
        Bv.npend[b] = 0; Bv.pflags[b] = 0; Bv.stall[b] = 0; Bv.flushed[b] = 1;      // (in place: every pass reads and writes the slot itself)
    }
}
// up to nsel replay steps of LP b by one workgroup (256 or 1024 threads)
__global__ __launch_bounds__(NT_BIG) void k_lb_select(LpView L, BatchView Bv, RfxView R, int n, int nsel)
{
    __shared__ double sv[NT_BIG / WAVE];
    __shared__ int si[NT_BIG / WAVE];
    const int b = blockIdx.x, tid = threadIdx.x, NT = (int)blockDim.x, M = L.M, ld = L.ld;
    if (b >= n) return;
    int *cnt = R.cnt + (size_t)b * 4, *elig = R.elig + (size_t)b * M;
    const int *enter = R.enter + (size_t)b * M;
    const int slot = Bv.dst[b];
    for (int sdx = 0; sdx < nsel; sdx++) {
        if (sdx) __syncthreads();              // (what the last step left -- heads, counters, its row and multipliers -- is read by all)
        const int np = Bv.npend[b], t = cnt[1];
        if (cnt[2] != RFX_RUN || np >= KP || t >= cnt[0]) break;
        const SelCtx c = sel_ctx(L, Bv, b, np, slot, slot);
        const int kq = enter[t], q = kq - M;   // (position q still holds structural q: every structural enters once, from its own place)
        double *pc = c.pc;
        // column q through the pending steps, the cost row (row M) with it
        for (int i = tid; i <= M; i += NT) pc[i] = virt_entry(c.T0[(size_t)i * ld + q], i, q, np, c.pd, c.prow0, c.pcol0, ld, L.Mp1p);
        __syncthreads();
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
        if (r < 0 || r >= M || !(best.v > TOL_PIV * (1.0 + cmax))) { if (tid == 0) cnt[2] = RFX_SINGULAR; break; }
        fetch_row_tableau(L, c, r);            // the pivot row where k_flush reads it (padding 0)
        const double p = 1.0 / pc[r];
        __syncthreads();                       // (everyone has read pc[r])
        for (int i = tid; i <= M; i += NT) pc[i] = i == r ? 0.0 : pc[i] * p;
        if (tid == 0) {
            PivDesc d;
            d.r = r; d.q = q; d.p = p; d.pbeta = 0.0; d.enter_val = 0.0;
            Bv.desc[(size_t)b * KP + np] = d;
            const int kb = c.bh[r];            // (the auxiliary variable of row r: an eligible row has not been pivoted)
            c.bh[r] = kq; c.nh[q] = kb; c.pos[kq] = r; c.pos[kb] = -1 - q;
            elig[r] = 0;
            cnt[1] = t + 1; Bv.npend[b] = np + 1; Bv.mode[b] = MODE_PIVOT;
        }
    }
}
// after the last pass: statuses and values follow their variable to the position it ended in; a slot that is done asks for the refresh pass
__global__ __launch_bounds__(NT) void k_lb_finish(LpView L, BatchView Bv, RfxView R, LbView Lb, int n)
{
    const int b = blockIdx.x, M = L.M, N = L.N;
    if (b >= n) return;
    int *cnt = R.cnt + (size_t)b * 4;
    const bool ok = cnt[2] == RFX_RUN && cnt[1] == cnt[0] && Bv.npend[b] == 0;
    __syncthreads();
    if (!ok) { if (threadIdx.x == 0) { if (cnt[2] == RFX_RUN) cnt[2] = RFX_SINGULAR; Bv.npend[b] = 0; Bv.mode[b] = MODE_NONE; Bv.status[b] = BSLV_LP_UNDEFINED; } return; }
    const int slot = Bv.dst[b];
    const int *nh = L.nh + (size_t)slot * N, *nst = Lb.nst + (size_t)b * (M + N);
    const double *xv = Lb.xv + (size_t)b * (M + N);
    int *nstat = L.nstat + (size_t)slot * N;
    double *xN = L.xN + (size_t)slot * L.ld;
    for (int j = threadIdx.x; j < L.ld; j += NT) {
        if (j >= N) { xN[j] = 0.0; continue; }
        const int k = nh[j];
        nstat[j] = nst[k]; xN[j] = xv[k];
    }
    if (threadIdx.x == 0) Bv.mode[b] = MODE_REFRESH;
}
// revised form: heads, positions, statuses and values of the slot from the list.  The basic variables take the rows in ascending id (the
// replay of refactor_impl moves them to the rows it pivots on), the nonbasic ones the positions in ascending id.
__global__ __launch_bounds__(NT) void k_lb_heads(LpView L, BatchView Bv, LbView Lb, int n)
{
    __shared__ int s_cnt[NT];
    const int b = blockIdx.x, tid = threadIdx.x, M = L.M, N = L.N, V = M + N;
    if (b >= n) return;
    const int slot = Bv.dst[b];
    const int *nst = Lb.nst + (size_t)b * V;
    const double *xv = Lb.xv + (size_t)b * V;
    int *bh = L.bh + (size_t)slot * M, *nh = L.nh + (size_t)slot * N, *pos = L.pos + (size_t)slot * V, *nstat = L.nstat + (size_t)slot * N;
    double *xN = L.xN + (size_t)slot * L.ld;
    const int chunk = (V + NT - 1) / NT, k0 = min(V, tid * chunk), k1 = min(V, k0 + chunk);
    int c = 0;
    for (int k = k0; k < k1; k++) c += nst[k] < 0;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) { int o = 0; for (int t = 0; t < NT; t++) { const int v = s_cnt[t]; s_cnt[t] = o; o += v; } }
    __syncthreads();
    int o = s_cnt[tid];                         // basic variables below k0
    for (int k = k0; k < k1; k++) {
        if (nst[k] < 0) { if (o < M) { bh[o] = k; pos[k] = o; } o++; }
        else { const int j = k - o; if (j < N) { nh[j] = k; pos[k] = -1 - j; nstat[j] = nst[k]; xN[j] = xv[k]; } }
    }
    for (int j = N + tid; j < L.ld; j += NT) xN[j] = 0.0;
}

}  // namespace bslv

extern "C" {

int bslv_lpq_var_map(const bslv_lpq *h, int *own_of_given)
{
    if (!h || !own_of_given) { set_error("bslv_lpq_var_map: bad argument"); return BSLV_E_ARG; }
    const bslv_lpq::Presolve &P = h->ps;
    for (int v = 0; v < P.M0 + P.N0; v++) own_of_given[v] = P.map_var(v);
    return 0;
}

static const char *lb_slots_ok(const bslv_lpq *h, int n, const int *slots, int *at)
{
    std::vector<char> taken(h->slots, 0);
    for (int b = 0; b < n; b++) {
        *at = b;
        if (slots[b] < 0 || slots[b] >= h->slots) return "out of range";
        if (taken[slots[b]]) return "named twice";
        taken[slots[b]] = 1;
    }
    return nullptr;
}

int bslv_lpq_get_basis(bslv_lpq *h, int slot, int *vstat, int *row_of)
{
    if (!h || !vstat) { set_error("bslv_lpq_get_basis: bad argument"); return BSLV_E_ARG; }
    if (slot < 0 || slot >= h->slots) { set_error("bslv_lpq_get_basis: bad slot %d", slot); return BSLV_E_ARG; }
    const LpView &L = h->L;
    const int V = L.M + L.N;
    // (the heads, statuses and values of a slot follow every committed pivot: a parked or lazily open slot answers as after its pass)
    std::vector<int> pos(V), nstat(L.N);
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(pos.data(), L.pos + (size_t)slot * V, (size_t)V * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nstat.data(), L.nstat + (size_t)slot * L.N, (size_t)L.N * sizeof(int), hipMemcpyDeviceToHost));
    static const int code_of[4] = {BSLV_LP_VS_LOWER, BSLV_LP_VS_UPPER, BSLV_LP_VS_FREE, BSLV_LP_VS_FIXED};      // NS_L, NS_U, NS_F, NS_S
    for (int k = 0; k < V; k++) {
        const int p = pos[k];
        if (p >= 0) { if (p >= L.M) { set_error("bslv_lpq_get_basis: slot %d holds no basis", slot); return BSLV_E_ARG; } vstat[k] = BSLV_LP_VS_BASIC; }
        else {
            const int j = -1 - p;
            if (j >= L.N || nstat[j] < 0 || nstat[j] > 3) { set_error("bslv_lpq_get_basis: slot %d holds no basis", slot); return BSLV_E_ARG; }
            vstat[k] = code_of[nstat[j]];
        }
        if (row_of) row_of[k] = p >= 0 ? p : -1;
    }
    return 0;
}

// The basis nst / xv (n lists over the engine's variables: nonbasic status or -1, nonbasic value) installed in the n slots (distinct, in
// range), in lock step.  status_out[b]: 0, or BSLV_LP_UNDEFINED for a singular basis (the slot is reset to the standard basis).
static int basis_install(bslv_lpq *h, int n, const int *slots, const int *nst, const double *xv, int *status_out)
{
    LpView &L = h->L;
    hipStream_t s = h->stream;
    const int V = L.M + L.N;
    int rc;
    // the call works on the batch buffers: slots of the last batch that still wait for their tableau get it first, as before a solve;
    // whoever still reads one of the slots as its parent makes its pass, and the slots' own records go (they are overwritten)
    if (h->lazy_open) { if ((rc = materialise_indices(h, nullptr, 0))) return rc; h->lazy_open = false; }
    if ((rc = park_before(h, 0, nullptr, n, slots))) return rc;
    if ((rc = ensure_batch(h, n))) return rc;
    if ((rc = ensure_rfx(h))) return rc;
    const size_t need = (size_t)n * V;
    if (need > h->lb_cap) {
        auto fr = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
        fr(h->lb_nst_d); fr(h->lb_xv_d); h->lb_cap = 0;
        HIP_TRY(malloc0s(&h->lb_nst_d, need * sizeof(int), s));
        HIP_TRY(malloc0s(&h->lb_xv_d, need * sizeof(double), s));
        h->lb_cap = need;
    }
    HIP_TRY(hipMemcpyAsync(h->lb_nst_d, nst, need * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->lb_xv_d, xv, need * sizeof(double), hipMemcpyHostToDevice, s));
    const LbView Lb{h->lb_nst_d, h->lb_xv_d};
    const int rounds_max = replay_rounds_max(L);
    long ok_n = 0, pivots = 0, failed = 0;
    if (L.rev) {
        HIP_TRY(hipMemcpyAsync(h->dst_d, slots, n * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_lb_heads, dim3(n), dim3(NT), 0, s, L, bview(h), Lb, n);
        HIP_TRY(hipGetLastError());
        if ((rc = refactor_impl(h, n, slots, status_out, &ok_n, &pivots, &failed))) return rc;      // (age 0, the own-cost reduced costs, beta; a singular basis: the slot reset)
    } else {
        if ((rc = ensure_nwork(h, std::max(L.maxit + 64, rounds_max + 2), rounds_max + 2))) return rc;
        L.objmode = 0;
        for (int b = 0; b < n; b++) h->active_h[b] = b;
        HIP_TRY(hipMemcpyAsync(h->active_d, h->active_h, n * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->src_d, slots, n * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->dst_d, slots, n * sizeof(int), hipMemcpyHostToDevice, s));
        for (int b = 0; b < n; b++) HIP_TRY(hipMemcpyAsync(L.T + (size_t)slots[b] * L.slotT, h->Tstd, L.slotT * sizeof(double), hipMemcpyDeviceToDevice, s));
        BatchView bv = bview(h);
        bv.lazy = 0;
        const RfxView R = rfx_view(h);
        // BSLV_LP_BASIS_TIMING=1: one line per call on stderr, HIP events around the whole replay and around each of its passes (the
        // last one is the refresh pass: a plain pass of k_flush over the same slots, nothing pending)
        const bool timing = getenv("BSLV_LP_BASIS_TIMING") != nullptr;
        std::vector<EventPair> tev;
        EventPair whole{nullptr, nullptr};
        if (timing) { if ((rc = event_pair(&whole))) return rc; HIP_TRY(hipEventRecord(whole.first, s)); }
        // in place; every pass waits on the host and counts in no statistics of a batch
        auto pass = [&](int cnt_slot) -> int {
            if (!timing) return flush_list(h, cnt_slot, n, false);
            tev.emplace_back(nullptr, nullptr);
            int r2 = event_pair(&tev.back());
            if (r2 || (r2 = flush_launch(h, bv, cnt_slot, n, &tev.back()))) return r2;
            HIP_TRY(hipStreamSynchronize(s));
            return 0;
        };
        hipLaunchKernelGGL(k_lb_setup, dim3(n), dim3(NT), 0, s, L, bv, R, Lb, n);
        HIP_TRY(hipGetLastError());
        std::vector<int> cnt((size_t)n * 4);
        HIP_TRY(hipMemcpyAsync(cnt.data(), h->rfx_c_d, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int kmax = 0;
        for (int k = 0; k < n; k++) if (cnt[(size_t)k * 4 + 2] == RFX_RUN) kmax = std::max(kmax, cnt[(size_t)k * 4]);
        const int rounds = std::min((kmax + KP - 1) / KP, rounds_max);
        const int snt = std::max(L.M, L.N) >= 1536 ? NT_BIG : NT;
        for (int it = 0; it < rounds; it++) {
            hipLaunchKernelGGL(k_lb_select, dim3(n), dim3(snt), 0, s, L, bv, R, n, KP);
            if ((rc = replay_pass(h, bv, h->active_d, n, it, pass))) return rc;
        }
        hipLaunchKernelGGL(k_lb_finish, dim3(n), dim3(NT), 0, s, L, bv, R, Lb, n);
        if ((rc = replay_pass(h, bv, h->active_d, n, rounds_max + 1, pass))) return rc;      // the refresh pass: beta = T x_N, the objective with it
        if (timing) {
            HIP_TRY(hipEventRecord(whole.second, s));
            HIP_TRY(hipStreamSynchronize(s));
            float all = 0, last = 0, sum = 0;
            (void)hipEventElapsedTime(&all, whole.first, whole.second);
            for (size_t k = 0; k < tev.size(); k++) { float t = 0; (void)hipEventElapsedTime(&t, tev[k].first, tev[k].second); sum += t; if (k + 1 == tev.size()) last = t; }
            fprintf(stderr, "bslv_lpq_load_basis: %d slots M %d N %d: replay %.4f ms (host waits included), %zu passes %.4f ms, the refresh pass alone %.4f ms\n",
                    n, L.M, L.N, all, tev.size(), sum, last);
            tev.push_back(whole);
            for (auto &e : tev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        }
        HIP_TRY(hipMemcpy(cnt.data(), h->rfx_c_d, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < n; b++) {
            const bool ok = cnt[(size_t)b * 4 + 2] == RFX_RUN;
            if (status_out) status_out[b] = ok ? 0 : BSLV_LP_UNDEFINED;
            if (ok) { ok_n += 1; pivots += cnt[(size_t)b * 4 + 1]; if (h->rays_on) HIP_TRY(hipMemsetAsync(h->raykind_d + slots[b], 0, sizeof(int), s)); }
            else { failed += 1; if ((rc = bslv_lpq_reset_slot(h, slots[b]))) return rc; }      // (nothing can read a half-built tableau)
        }
    }
    std::vector<int> nw(rounds_max + 2);
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(nw.data(), h->nwork_d, nw.size() * sizeof(int), hipMemcpyDeviceToHost));
    long passes = 0;
    for (int v : nw) passes += v;
    h->last_rebuild[0] = ok_n; h->last_rebuild[1] = pivots; h->last_rebuild[2] = passes; h->last_rebuild[3] = failed;
    return 0;
}

int bslv_lpq_load_basis(bslv_lpq *h, int n, const int *slots, const int *vstat, const double *vlo, const double *vup, int *status_out)
{
    if (!h) { set_error("bslv_lpq_load_basis: no engine"); return BSLV_E_ARG; }
    if (n < 0 || (n > 0 && (!slots || !vstat)) || (vlo == nullptr) != (vup == nullptr)) { set_error("bslv_lpq_load_basis: bad argument (n = %d)", n); return BSLV_E_ARG; }
    { int at = 0; if (const char *why = lb_slots_ok(h, n, slots, &at)) { set_error("bslv_lpq_load_basis: bad slot %d at %d: %s (pool %d)", slots[at], at, why, h->slots); return BSLV_E_ARG; } }
    for (int k = 0; k < 4; k++) h->last_rebuild[k] = 0;
    if (n == 0) return 0;
    const LpView &L = h->L;
    const int M = L.M, N = L.N, V = M + N;
    // the bounds the engine works with: the model's, the artificial ones of upload_bounds in place of an infinite bound on a cost's side
    std::vector<double> lb(V), ub(V);
    std::vector<unsigned char> art(V);
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(lb.data(), h->lb_d, (size_t)V * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ub.data(), h->ub_d, (size_t)V * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(art.data(), h->art_d, (size_t)V, hipMemcpyDeviceToHost));
    std::vector<int> nst((size_t)n * V);
    std::vector<double> xv((size_t)n * V);
    for (int b = 0; b < n; b++) {
        int basic = 0;
        for (int k = 0; k < V; k++) {
            const int code = vstat[(size_t)b * V + k], j = k - L.vfirst;
            const bool per_lp = vlo && j >= 0 && j < L.vcnt;
            const double lo = per_lp ? vlo[(size_t)b * L.vcnt + j] : lb[k], up = per_lp ? vup[(size_t)b * L.vcnt + j] : ub[k];
            const unsigned char a = per_lp ? 0 : art[k];
            int st = -1;
            double x = 0.0;
            const char *why = nullptr;
            switch (code) {
            case BSLV_LP_VS_BASIC: basic++; break;
            case BSLV_LP_VS_LOWER: if (std::isinf(lo) || std::isnan(lo)) why = "LOWER names an infinite bound"; else { st = lo == up ? NS_S : NS_L; x = lo; } break;
            case BSLV_LP_VS_UPPER: if (std::isinf(up) || std::isnan(up)) why = "UPPER names an infinite bound"; else { st = lo == up ? NS_S : NS_U; x = up; } break;
            case BSLV_LP_VS_FREE:  if (!((std::isinf(lo) || (a & 1)) && (std::isinf(up) || (a & 2)))) why = "FREE on a bounded variable"; else st = NS_F; break;
            case BSLV_LP_VS_FIXED: if (!(lo == up) || std::isinf(lo)) why = "FIXED on a variable whose bounds differ"; else { st = NS_S; x = lo; } break;
            default: why = "unknown status code";
            }
            if (why) { set_error("bslv_lpq_load_basis: LP %d, variable %d, status %d: %s", b, k, code, why); return BSLV_E_ARG; }
            nst[(size_t)b * V + k] = st; xv[(size_t)b * V + k] = x;
        }
        if (basic != M) { set_error("bslv_lpq_load_basis: LP %d names %d basic variables, the model has %d rows", b, basic, M); return BSLV_E_ARG; }
    }
    return basis_install(h, n, slots, nst.data(), xv.data(), status_out);
}

int bslv_lpq_rebuild(bslv_lpq *h, int n, const int *slots, int *status_out)
{
    if (!h) { set_error("bslv_lpq_rebuild: no engine"); return BSLV_E_ARG; }
    if (n < 0 || (n > 0 && !slots)) { set_error("bslv_lpq_rebuild: bad argument (n = %d)", n); return BSLV_E_ARG; }
    { int at = 0; if (const char *why = lb_slots_ok(h, n, slots, &at)) { set_error("bslv_lpq_rebuild: bad slot %d at %d: %s (pool %d)", slots[at], at, why, h->slots); return BSLV_E_ARG; } }
    for (int k = 0; k < 4; k++) h->last_rebuild[k] = 0;
    if (n == 0) return 0;
    const LpView &L = h->L;
    int rc;
    if (L.rev) {      // the revised form's rebuild IS its refactorisation
        if ((rc = bslv_lpq_refactor(h, n, slots, status_out))) return rc;
        std::vector<int> nw(replay_rounds_max(L) + 2);
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(nw.data(), h->nwork_d, nw.size() * sizeof(int), hipMemcpyDeviceToHost));
        long passes = 0;
        for (int v : nw) passes += v;
        h->last_rebuild[0] = h->last.rfx[0]; h->last_rebuild[1] = h->last.rfx[1]; h->last_rebuild[2] = passes; h->last_rebuild[3] = h->last.rfx[3];
        return 0;
    }
    // a slot whose pass is parked or pending gets its tableau first; then its own basis is read back: every variable keeps its
    // nonbasic status and value
    if ((rc = bslv_lpq_materialise(h, n, slots))) return rc;
    const int M = L.M, N = L.N, V = M + N;
    std::vector<int> nst((size_t)n * V), pos(V), nstat(N);
    std::vector<double> xv((size_t)n * V, 0.0), xN(N);
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int b = 0; b < n; b++) {
        const int slot = slots[b];
        HIP_TRY(hipMemcpy(pos.data(), L.pos + (size_t)slot * V, (size_t)V * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(nstat.data(), L.nstat + (size_t)slot * N, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(xN.data(), L.xN + (size_t)slot * L.ld, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        int basic = 0;
        for (int k = 0; k < V; k++) {
            const int p = pos[k];
            if (p >= 0) { basic++; nst[(size_t)b * V + k] = -1; continue; }
            const int j = -1 - p;
            if (j >= N || nstat[j] < 0 || nstat[j] > 3) { set_error("bslv_lpq_rebuild: slot %d holds no basis", slot); return BSLV_E_ARG; }
            nst[(size_t)b * V + k] = nstat[j]; xv[(size_t)b * V + k] = xN[j];
        }
        if (basic != M) { set_error("bslv_lpq_rebuild: slot %d holds no basis", slot); return BSLV_E_ARG; }
    }
    return basis_install(h, n, slots, nst.data(), xv.data(), status_out);
}

int bslv_lpq_last_rebuild_stats(const bslv_lpq *h, long out[4])
{
    if (!h || !out) return BSLV_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = h->last_rebuild[k];
    return 0;
}

}  // extern "C"
