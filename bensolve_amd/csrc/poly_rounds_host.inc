// poly_rounds_host.inc -- host side of the multi-cut path (included after do_cut in poly_engine.hip)

struct RoundsBuf {
    int *tc = nullptr, *t1 = nullptr, *cutof = nullptr, *zlist = nullptr, *mem_in = nullptr, *mem = nullptr; int vcap = 0;
    unsigned long long *msig = nullptr;
    int2 *conf = nullptr; int confcap = 0;
    int *ints = nullptr;          // [0] conf count, [1] overflow, [2..5] counters, [6] err
    unsigned *nminus = nullptr; int *selmap = nullptr, *selb = nullptr, *self = nullptr, *mcnt = nullptr, *mfill = nullptr, *moff = nullptr; int bcap = 0;
    PairBlkM *blks = nullptr; int blkcap = 0;
    // pinned host mirrors
    int *h_ints = nullptr, *h_mcnt = nullptr; unsigned *h_nminus = nullptr; int2 *h_conf = nullptr;
};

static int rounds_ensure(bslv_poly *h, RoundsBuf &R, int B)
{
    int rc;
    hipStream_t s = h->stream;
    if (h->P.cap > R.vcap) {
        // cutof/tc of the pass in flight must survive a re-allocation
        if ((rc = grow(&R.tc, (size_t)R.vcap, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.t1, (size_t)R.vcap, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.cutof, (size_t)R.vcap, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.zlist, 0, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.mem_in, 0, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.mem, 0, (size_t)h->P.cap, s))) return rc;
        if ((rc = grow(&R.msig, 0, (size_t)h->P.cap, s))) return rc;
        R.vcap = h->P.cap;
    }
    if (!R.conf) {
        R.confcap = 1 << 20;
        if ((rc = grow(&R.conf, 0, (size_t)R.confcap, s))) return rc;
        if ((rc = grow(&R.ints, 0, 16, s, true))) return rc;
        HIP_TRY(hipHostMalloc(&R.h_ints, 16 * sizeof(int)));
        HIP_TRY(hipHostMalloc(&R.h_conf, (size_t)R.confcap * sizeof(int2)));
    }
    if (B > R.bcap) {
        int nc = std::max(B, 1024);
        if ((rc = grow(&R.nminus, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.selmap, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.selb, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.self, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.mcnt, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.mfill, 0, (size_t)nc, s))) return rc;
        if ((rc = grow(&R.moff, 0, (size_t)nc + 1, s))) return rc;
        if (R.h_nminus) (void)hipHostFree(R.h_nminus);
        if (R.h_mcnt) (void)hipHostFree(R.h_mcnt);
        HIP_TRY(hipHostMalloc(&R.h_nminus, (size_t)nc * sizeof(unsigned)));
        HIP_TRY(hipHostMalloc(&R.h_mcnt, (size_t)(nc + 1) * sizeof(int)));
        R.bcap = nc;
    }
    return 0;
}

static void rounds_free(RoundsBuf &R)
{
    auto fr = [](void *p) { if (p) (void)hipFree(p); };
    fr(R.tc); fr(R.t1); fr(R.cutof); fr(R.zlist); fr(R.mem_in); fr(R.mem); fr(R.msig); fr(R.conf); fr(R.ints);
    fr(R.nminus); fr(R.selmap); fr(R.selb); fr(R.self); fr(R.mcnt); fr(R.mfill); fr(R.moff); fr(R.blks);
    if (R.h_ints) (void)hipHostFree(R.h_ints);
    if (R.h_nminus) (void)hipHostFree(R.h_nminus);
    if (R.h_mcnt) (void)hipHostFree(R.h_mcnt);
    if (R.h_conf) (void)hipHostFree(R.h_conf);
    R = RoundsBuf();
}

static int scan_sync(bslv_poly *h, int nb, int slot, Tri *out)
{
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, h->stream, h->bsum, nb, h->totals + slot, (Mail *)nullptr, (const int *)nullptr, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->totals_h, h->totals + slot, sizeof(Tri), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = h->totals_h[0];
    return 0;
}

// one multi-cut pass over the selected cuts (indices `sel` into the classified array of this round)
static int apply_selected(bslv_poly *h, RoundsBuf &R, const std::vector<int> &sel, const std::vector<int> &fid_of_local, int Bcls, int nw)
{
    const int S = (int)sel.size(), nv0 = h->nv, ne0 = h->ne;
    hipStream_t s = h->stream;
    int rc;
    std::vector<int> selmap(Bcls, -1), selfv(S);
    for (int k = 0; k < S; k++) {
        selmap[sel[k]] = k;
        selfv[k] = (int)h->facet_of_rank.size();            // rank = order of application (keeps lists sorted)
        h->facet_of_rank.push_back(fid_of_local[sel[k]]);
    }
    HIP_TRY(hipMemcpyAsync(R.selmap, selmap.data(), Bcls * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(R.selb, sel.data(), S * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(R.self, selfv.data(), S * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(R.ints + 2, 0, 5 * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(R.mcnt, 0, S * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(R.mfill, 0, S * sizeof(int), s));
    const int nbv = (nv0 + PB - 1) / PB, nbe = std::max(1, (ne0 + PB - 1) / PB);
    if ((rc = ensure_bsum(h, std::max(nbe, nbv) + 1))) return rc;
    SelView SV{h->hps_d, R.selb, R.self};
    const int2 *Eold = h->E[h->ecur];
    int2 *Enew = h->E[1 - h->ecur];
    hipLaunchKernelGGL(k_assign, dim3(nbv), dim3(PB), 0, s, h->P, h->clsw, nw, nv0, R.tc, R.t1, R.selmap, R.cutof, R.ints + 2);
    hipLaunchKernelGGL(k_edge_flags, dim3(nbe), dim3(PB), 0, s, h->P, Eold, ne0, h->eflag, h->bsum);
    Tri te;
    if ((rc = scan_sync(h, nbe, 0, &te))) return rc;
    HIP_TRY(hipMemcpy(R.h_ints, R.ints, 8 * sizeof(int), hipMemcpyDeviceToHost));
    const int nzero = R.h_ints[3], zero_ub = R.h_ints[4];
    if (R.h_ints[5]) { set_error("multi-cut pass: selected cuts are not independent (code %d)", R.h_ints[5]); return BSLV_E_STATE; }
    const int nsurv = te.a, ncross = te.b;
    if ((rc = ensure_vcap(h, nv0 + ncross))) return rc;
    if ((rc = rounds_ensure(h, R, Bcls))) return rc;
    if ((rc = ensure_pool(h, (size_t)h->poolused + te.c + zero_ub))) return rc;
    const unsigned pool_e = h->poolused, pool_z = h->poolused + (unsigned)te.c;
    hipLaunchKernelGGL(k_edge_emit_m, dim3(nbe), dim3(PB), 0, s, h->P, SV, R.cutof, Eold, ne0, h->eflag, h->bsum, h->totals + 0, Enew, nv0, pool_e, R.ints + 6);
    hipLaunchKernelGGL(k_vert_flags, dim3(nbv), dim3(PB), 0, s, h->P, nv0, h->bsum);
    Tri tz;
    if ((rc = scan_sync(h, nbv, 1, &tz))) return rc;
    if (tz.a != nzero) { set_error("multi-cut pass: ZERO count mismatch %d vs %d", tz.a, nzero); return BSLV_E_STATE; }
    hipLaunchKernelGGL(k_vert_emit_m, dim3(nbv), dim3(PB), 0, s, h->P, SV, R.cutof, nv0, h->bsum, R.zlist, pool_z);
    const int nmem = nzero + ncross;
    h->poolused += (unsigned)te.c + (unsigned)tz.c;
    h->nv = nv0 + ncross;
    h->ne = nsurv + ncross;
    h->ecur = 1 - h->ecur;
    h->new_vertices += ncross;
    if (nmem > 0) {
        const int nbm = (nmem + 255) / 256;
        hipLaunchKernelGGL(k_mcount, dim3(nbm), dim3(256), 0, s, R.zlist, nzero, nv0, ncross, R.cutof, R.mcnt);
        HIP_TRY(hipMemcpyAsync(R.h_mcnt, R.mcnt, S * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(R.h_ints, R.ints, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (R.h_ints[6]) { set_error("multi-cut pass: edge joins two selected cuts (code %d)", R.h_ints[6]); return BSLV_E_STATE; }
        std::vector<int> moff(S + 1, 0);
        for (int k = 0; k < S; k++) moff[k + 1] = moff[k] + R.h_mcnt[k];
        if (moff[S] != nmem) { set_error("multi-cut pass: member count mismatch %d vs %d", moff[S], nmem); return BSLV_E_STATE; }
        HIP_TRY(hipMemcpyAsync(R.moff, moff.data(), (S + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_mscatter, dim3(nbm), dim3(256), 0, s, R.zlist, nzero, nv0, ncross, R.cutof, R.moff, R.mfill, R.mem_in);
        hipLaunchKernelGGL(k_msort_sig, dim3(S), dim3(PB), 0, s, h->P, R.moff, R.mem_in, R.mem, R.msig);
        std::vector<PairBlkM> blks;
        long pairs = 0;
        for (int k = 0; k < S; k++) {
            const int nm = R.h_mcnt[k];
            pairs += (long)nm * (nm - 1) / 2;
            for (int i = 0; i + 1 < nm; i++) for (int j0 = i + 1; j0 < nm; j0 += PB) blks.push_back(PairBlkM{k, i, j0});
        }
        h->pair_tests += pairs;
        const int nbp = (int)blks.size();
        if (nbp > 0) {
            if (nbp > R.blkcap) { int nc = std::max(nbp, R.blkcap * 2); if ((rc = grow(&R.blks, 0, (size_t)nc, s))) return rc; R.blkcap = nc; }
            if ((size_t)nbp * PB > h->pflagcap) { size_t nc = std::max((size_t)nbp * PB, h->pflagcap * 2); if ((rc = grow(&h->pflag, 0, nc, s))) return rc; h->pflagcap = nc; }
            if ((rc = ensure_bsum(h, nbp + 1))) return rc;
            HIP_TRY(hipMemcpyAsync(R.blks, blks.data(), (size_t)nbp * sizeof(PairBlkM), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_pair_flags_m, dim3(nbp), dim3(PB), 0, s, h->P, R.moff, R.mem, R.msig, R.blks, h->pflag, h->bsum);
            Tri tp;
            if ((rc = scan_sync(h, nbp, 2, &tp))) return rc;      // also orders the pageable blks upload before `blks` dies
            if (tp.a > 0) {
                if ((rc = ensure_ecap(h, h->ne + tp.a))) return rc;
                hipLaunchKernelGGL(k_pair_emit_m, dim3(nbp), dim3(PB), 0, s, R.moff, R.mem, R.blks, h->pflag, h->bsum, h->E[h->ecur], h->ne);
                HIP_TRY(hipGetLastError());
                h->ne += tp.a;
            }
        } else HIP_TRY(hipStreamSynchronize(s));
    }
    if ((rc = ensure_ecap(h, h->ne + 1))) return rc;
    h->cuts_applied += S;
    return 0;
}

// the cuts todo[] of the classified chunk one after the other (index order), in hot mode when that pays: R.tc holds
// the touch counts of the whole chunk, a superset of what these cuts can reach
static int run_rounds2(bslv_poly *h, RoundsBuf &R, const std::vector<int> &todo, const std::vector<int> &fid_local, const std::vector<int> &rem, int *rc_out,
                       int Bc, int nw, std::vector<int> &left_out);
// Bc, nw: size of the chunk's classification (class words in h->clsw); 0: the class words are not available
static int run_sequence(bslv_poly *h, RoundsBuf &R, const std::vector<int> &todo_in, const std::vector<int> &fid_local, const std::vector<int> &rem, int *rc_out,
                        int Bc = 0, int nw = 0)
{
    int rc;
    const bool hot = h->hot_enabled && todo_in.size() >= 8;
    auto t0 = std::chrono::steady_clock::now();
    if (hot && (rc = hot_begin(h, R.tc))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    std::vector<int> left;
    const std::vector<int> *todo_p = &todo_in;
    if (hot && h->rounds2_enabled && Bc > 0 && todo_in.size() >= 16 && Bc <= 4096) {
        // rounds of independent cuts, chosen and applied on the device (poly_rounds2_*.inc); whatever it leaves goes one at a time
        if ((rc = run_rounds2(h, R, todo_in, fid_local, rem, rc_out, Bc, nw, left))) return rc;
        // (the chunk was shuffled for the rounds; one at a time the cuts go in the order they were given)
        std::sort(left.begin(), left.end(), [&](int a, int b) { return rem[a] < rem[b]; });
        if (h->r2_deferred) {
            // handed back: the dual slots stay behind unused, as those of redundant cuts do
            for (int k : left) { h->fapplied[fid_local[k]] = 0; rc_out[rem[k]] = 2; }
            h->r2_deferred_cuts += (long)left.size();
            left.clear();
        }
        todo_p = &left;
    }
    const std::vector<int> &todo = *todo_p;
    for (size_t t = 0; t < todo.size(); t++) {
        int r1;
        if ((rc = do_cut(h, fid_local[todo[t]], &r1, t + 1 < todo.size() ? fid_local[todo[t + 1]] : -1))) return rc;
        rc_out[rem[todo[t]]] = r1;
    }
    if ((rc = settle_k2(h))) return rc;
    auto t2 = std::chrono::steady_clock::now();
    if (hot && (rc = hot_end(h))) return rc;
    auto t3 = std::chrono::steady_clock::now();
    h->tm_hot_begin += std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->tm_seq += std::chrono::duration<double, std::milli>(t2 - t1).count();
    h->tm_hot_end += std::chrono::duration<double, std::milli>(t3 - t2).count();
    h->tm_seq_cuts += (long)todo_in.size();
    return 0;
}

// apply the cuts fids[0..B) (dual slots already created) in rounds of independent cuts
static int apply_cuts_rounds(bslv_poly *h, const std::vector<int> &fids, int *rc_out)
{
    const int d = h->d, B = (int)fids.size();
    RoundsBuf &R = *h->rounds;
    hipStream_t s = h->stream;
    const int chunkB = std::min(std::max(h->chunk_cuts, 32), 4096);
    int rc;
    for (int b0 = 0; b0 < B; b0 += chunkB) {
        std::vector<int> rem;                       // indices into fids
        for (int b = b0; b < std::min(B, b0 + chunkB); b++) rem.push_back(b);
        bool first_round = true;                    // of this chunk
        if (h->rounds2_enabled && h->hot_enabled && (int)rem.size() >= 16) {
            // device-selected rounds take the index of a cut within the chunk as its priority (poly_rounds2_kernels.inc): a
            // pseudo-random order of the chunk, the same on every rank (Fisher-Yates with a counter-based generator)
            unsigned long long x = 0x9E3779B97F4A7C15ull * (unsigned long long)(++h->shuffle_seq);
            for (size_t k = rem.size() - 1; k > 0; k--) {
                x += 0x9E3779B97F4A7C15ull;
                unsigned long long z = x;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
                std::swap(rem[k], rem[(size_t)(z % (k + 1))]);
            }
        }
        while (!rem.empty()) {
            const auto tp0 = std::chrono::steady_clock::now();
            const int Bc = (int)rem.size(), nw = (Bc + 31) / 32, nv = h->nv;
            size_t need = (size_t)nw * h->P.cap;
            if (need > h->clswcap) { if ((rc = grow(&h->clsw, 0, std::max(need, (size_t)16 * h->P.cap), s))) return rc; h->clswcap = std::max(need, (size_t)16 * h->P.cap); }
            if ((rc = rounds_ensure(h, R, chunkB))) return rc;
            std::vector<double> hps((size_t)Bc * (d + 1));
            std::vector<int> fid_local(Bc);
            for (int k = 0; k < Bc; k++) { fid_local[k] = fids[rem[k]]; memcpy(&hps[(size_t)k * (d + 1)], &h->hp[(size_t)fid_local[k] * (d + 1)], (d + 1) * sizeof(double)); }
            if ((rc = upload_hps(h, hps.data(), Bc))) return rc;
            HIP_TRY(hipMemsetAsync(R.nminus, 0, nw * sizeof(unsigned), s));
            HIP_TRY(hipMemsetAsync(R.ints, 0, 2 * sizeof(int), s));
            const int nbv = (nv + PB - 1) / PB, nbe = std::max(1, (h->ne + PB - 1) / PB);
            // batches of neighbouring vertices keep producing complete conflict graphs (see below): after two such
            // chunks in a row the conflict pass is skipped for a while (1, 2, 4, 8, 15 chunks), then probed again
            // device-selected rounds inside a hot chunk (poly_rounds2_*.inc) replace the conflict pass and the multi-cut passes over
            // the whole polyhedron: the chunk goes to run_sequence as it is
            const bool use_r2 = h->rounds2_enabled && h->hot_enabled && Bc >= 16;
            const bool probe = h->dense_skip == 0 && !use_r2;
            if (!probe && !use_r2) h->dense_skip--;
            if (use_r2) {
                // the class words are laid out with the stride of the element arrays: room for the vertices of the chunk up front
                if ((rc = ensure_vcap(h, nv + std::max(1 << 17, 512 * Bc)))) return rc;
                need = (size_t)nw * h->P.cap;
                if (need > h->clswcap) { if ((rc = grow(&h->clsw, 0, need, s))) return rc; h->clswcap = need; }
                if ((rc = rounds_ensure(h, R, chunkB))) return rc;
            }
            if ((rc = launch_classify_batch(h, Bc, nv, h->clsw, R.nminus, R.tc, R.t1))) return rc;      // (touch counts: conflict pass and hot mode)
            ConfBuf C{R.conf, R.ints + 0, R.confcap, R.ints + 1};
            if (Bc > 1 && probe) {
                hipLaunchKernelGGL(k_conflict_v, dim3(nbv), dim3(PB), 0, s, h->P, h->clsw, nw, nv, R.tc, C);
                hipLaunchKernelGGL(k_conflict_e, dim3(nbe), dim3(PB), 0, s, h->P, h->clsw, nw, h->E[h->ecur], h->ne, R.tc, R.t1, C);
            }
            HIP_TRY(hipGetLastError());
            const auto tp1 = std::chrono::steady_clock::now();
            HIP_TRY(hipMemcpyAsync(R.h_nminus, R.nminus, nw * sizeof(unsigned), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(R.h_ints, R.ints, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            h->tm_prep += std::chrono::duration<double, std::milli>(tp1 - tp0).count();
            h->tm_classify_wait += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp1).count();
            const int nconf = std::min(R.h_ints[0], R.confcap), overflow = R.h_ints[1];
            // redundant cuts: no live element violates them, and by convexity none ever will
            std::vector<char> alive(Bc, 1);
            for (int k = 0; k < Bc; k++) if (((R.h_nminus[k >> 5] >> (k & 31)) & 1u) == 0) { alive[k] = 0; h->fapplied[fid_local[k]] = 0; rc_out[rem[k]] = 1; }
            std::vector<int> sel;
            if (!probe) {
                std::vector<int> todo;
                for (int k = 0; k < Bc; k++) if (alive[k]) todo.push_back(k);
                const long r2r = h->r2_rounds, r2c = h->r2_cuts, r2d = h->r2_deferred_cuts;
                if ((rc = run_sequence(h, R, todo, fid_local, rem, rc_out, use_r2 ? Bc : 0, nw))) return rc;
                h->rounds_run += (h->r2_rounds - r2r) + ((long)todo.size() - (h->r2_cuts - r2c) - (h->r2_deferred_cuts - r2d));      // passes: rounds + cuts applied one at a time (not those handed back)
                rem.clear();
                continue;
            }
            if (overflow) {
                for (int k = 0; k < Bc && sel.empty(); k++) if (alive[k]) sel.push_back(k);      // degenerate crowd: one cut per round
            } else {
                if (nconf > 0) HIP_TRY(hipMemcpy(R.h_conf, R.conf, (size_t)nconf * sizeof(int2), hipMemcpyDeviceToHost));
                // greedy maximal independent set in index order (deterministic, identical on every rank).
                // The intersection of halfspaces does not depend on the order of conflicting cuts; only
                // slot numbers and which of two duplicate halfspaces is kept do.
                std::vector<std::vector<int>> adj(Bc);
                for (int p = 0; p < nconf; p++) { int2 c = R.h_conf[p]; if (alive[c.x] && alive[c.y]) { adj[c.x].push_back(c.y); adj[c.y].push_back(c.x); } }
                std::vector<char> taken(Bc, 0), blocked(Bc, 0);
                for (int k = 0; k < Bc; k++) {
                    if (!alive[k] || blocked[k]) continue;
                    taken[k] = 1; sel.push_back(k);
                    for (int o : adj[k]) blocked[o] = 1;
                }
                h->conf_pairs += nconf; h->conf_cuts += Bc;
            }
            if (getenv("BSLV_ROUNDS_DEBUG")) {
                int na = 0; for (int k = 0; k < Bc; k++) na += alive[k];
                fprintf(stderr, "round: classified %d alive %d conflicts %d overflow %d selected %zu nv %d ne %d\n", Bc, na, nconf, overflow, sel.size(), h->nv, h->ne);
            }
            // dense conflicts (a batch of neighbouring vertices: all cuts act on one region): grouping buys
            // nothing and every further round would pay a classification of the whole polyhedron, so the
            // rest of the chunk goes through the one-cut pipeline in index order
            {
                int na = 0; for (int k = 0; k < Bc; k++) na += alive[k];
                if (na >= 8 && (int)sel.size() * 4 < na && (int)sel.size() < 16) {
                    std::vector<int> todo;
                    for (int k = 0; k < Bc; k++) if (alive[k]) todo.push_back(k);
                    if ((rc = run_sequence(h, R, todo, fid_local, rem, rc_out))) return rc;
                    h->rounds_run += na;
                    rem.clear();
                    // only a chunk that is crowded as a whole counts (the leftovers of a well-separated chunk are always
                    // a few mutually conflicting cuts)
                    // back off: skip 1, 2, 4, 8, then 15 chunks between probes while the chunks stay crowded
                    if (first_round && ++h->dense_streak >= 2) h->dense_skip = std::min(15, 1 << std::min(h->dense_streak - 2, 4));
                    continue;
                }
            }
            if (first_round) h->dense_streak = 0;
            first_round = false;
            std::vector<int> next;
            if (!sel.empty()) {
                if (sel.size() == 1) {
                    int r1;
                    if ((rc = do_cut(h, fid_local[sel[0]], &r1))) return rc;
                    if ((rc = settle_k2(h))) return rc;
                    rc_out[rem[sel[0]]] = r1;
                } else {
                    if ((rc = apply_selected(h, R, sel, fid_local, Bc, nw))) return rc;
                    for (int k : sel) rc_out[rem[k]] = 0;
                }
                std::vector<char> done(Bc, 0);
                for (int k : sel) done[k] = 1;
                for (int k = 0; k < Bc; k++) if (alive[k] && !done[k]) next.push_back(rem[k]);
                h->rounds_run++;
            }
            rem.swap(next);
        }
    }
    return 0;
}
