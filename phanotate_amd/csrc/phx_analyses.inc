// phx_analyses.inc — the analyses of a finished run: per-ORF margins, gene drop margins, drop replacements, masked re-annotation and its margins.
// Host code, included by phx_api.cpp inside its extern "C" block, behind the taps.  Each analysis is an ensure_* that computes once per
// run on the context's stream (outside the captured run graph) and an entry point that lays the records out for the caller.

// ---- what the analyses share ----
// the bit of a limb class in the launchers' nl_mask (bit k: 2, 4, 8, 17 limbs)
static inline int nl_class_bit(int sssp_nl) { return sssp_nl == 2 ? 1 : sssp_nl == 4 ? 2 : sssp_nl == 8 ? 4 : 8; }

static int analysis_events(phx_ctx *c) { // phx_ctx::aev, created at the first analysis of a context
    for (hipEvent_t &e : c->aev) if (!e) HIPCHK(c, hipEventCreate(&e));
    return PHX_OK;
}
static float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f; }
// the *_ms and *_stats getters: N values of the context's, those at src(c)
extern "C++" template <int N, class T, class F> static int values_out(const phx_ctx *c, T *out, F src) {
    if (!c || !out) return PHX_E_ARG;
    for (int k = 0; k < N; k++) out[k] = src(c)[k];
    return PHX_OK;
}
// a contig of the last re-annotation call that was not solved again: the run's result stands for it
static bool any_unsolved(const phx_ctx *c) {
    for (size_t i = 0; i < (size_t)c->n; i++) if (!c->h_qsel[i]) return true;
    return false;
}

// the run's group records on the host, once per run
static int ensure_grp_host(phx_ctx *c) {
    if (c->done.grp) return PHX_OK;
    c->h_grp.resize((size_t)c->tot_grp);
    if (c->tot_grp) HIPCHK(c, hipMemcpy(c->h_grp.data(), c->b_grp.p, (size_t)c->tot_grp * sizeof(DGrp), hipMemcpyDeviceToHost));
    c->done.grp = true;
    return PHX_OK;
}
// Contig i's groups in the reference's iter_orfs order (phx_tap_orfs: ascending DGrp.evkey; the ORFs of a group are contiguous in that
// order and in the device's): fn(the group's first ORF in the contig's device order, its ORFs).  After ensure_grp_host; order: scratch.
extern "C++" template <class F> static void each_group_in_reference_order(const phx_ctx *c, size_t i, std::vector<int> &order, F fn) {
    const DGrp *grp = c->h_grp.data() + c->meta[i].grp_off;
    reference_sort(grp, (size_t)c->meta[i].n_grp, order);
    for (const int g : order) fn(grp[(size_t)g].orf_begin, grp[(size_t)g].n);
}

// the sorted keys of the CDS genes phx_download* deliver for contig i (after stage_run_genes): what `called` is looked up in
static inline uint64_t gene_key(int32_t left, int32_t right, int32_t strand) { return ((uint64_t)(uint32_t)left << 33) | ((uint64_t)(uint32_t)right << 1) | (strand < 0 ? 1u : 0u); }
static void called_keys(const phx_ctx *c, int i, std::vector<uint64_t> &keys) {
    int64_t ng = 0;
    const DGene *src = delivered_genes(c, i, &ng);
    keys.clear();
    for (int64_t k = 0; k < ng; k++) if (src[k].frame >= -3 && src[k].frame <= 3) keys.push_back(gene_key(src[k].left, src[k].right, src[k].strand)); // (tRNA path edges, frame +-4, are no ORFs)
    std::sort(keys.begin(), keys.end());
}
static inline bool is_called(const std::vector<uint64_t> &keys, int32_t left, int32_t right, int32_t strand) { return std::binary_search(keys.begin(), keys.end(), gene_key(left, right, strand)); }

// ---- per-ORF path margins (phx_margins.inc, DESIGN.md §11) ----
// limb classes of the contigs that have device distances
static int margins_nl_mask(const phx_ctx *c) {
    int nlm = 0;
    for (size_t i = 0; i < (size_t)c->n; i++) {
        const DMeta &m = c->meta[i];
        if (m.status < 0 || m.n_node <= 2 || m.sssp_mode == 4) continue;
        nlm |= nl_class_bit(m.sssp_nl);
    }
    return nlm;
}

static void margins_args(phx_ctx *c, DMarg *g) {
    g->out_off = (uint32_t *)c->b_mo.p; g->out_dst = (uint32_t *)c->b_md.p; g->out_w = (long long *)c->b_mw.p;
    g->dist_t = (uint64_t *)c->b_mdt.p; g->rec = (phx_orf_margin *)c->b_mrec.p; g->mstat = (int32_t *)c->b_mstat.p;
}

// The shared part of the margins and the drop margins, once per run: the out-edge CSR, d_t and the reverse pass's per-contig verdicts
// (c->mstat), kernel by kernel on the context's stream, outside the captured run graph.
static int ensure_rev(phx_ctx *c) {
    if (c->done.rev) return PHX_OK;
    { const int rf = fetch_meta(c); if (rf) return rf; }
    const size_t n = (size_t)c->n, V = (size_t)c->tot_node, E = (size_t)c->tot_edge, N = (size_t)c->tot_orf;
    const size_t limbs = (size_t)std::max(c->n_limbs, 2);
    const int nlm = margins_nl_mask(c);
    int rc;
    if ((rc = ensure(c, c->b_mo, (V + n + 1) * 4))) return rc;
    if ((rc = ensure(c, c->b_md, (E + 1) * 4))) return rc;
    if ((rc = ensure(c, c->b_mw, (E + 1) * 8))) return rc;
    if ((rc = ensure(c, c->b_mdt, (V + 1) * limbs * 8))) return rc;
    if ((rc = ensure(c, c->b_mrec, (N + 1) * sizeof(phx_orf_margin)))) return rc;
    if ((rc = ensure(c, c->b_mstat, (n + 1) * 4))) return rc;
    if ((rc = analysis_events(c))) return rc;
    c->mstat.assign(n, 0);
    DBatch b;
    fill_batch(c, &b);
    DMarg g;
    margins_args(c, &g);
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(c->aev[0], s));
    HIPCHK(c, hipMemsetAsync(c->b_mo.p, 0, (V + n + 1) * 4, s));
    HIPCHK(c, hipMemsetAsync(c->b_mstat.p, 0, (n + 1) * 4, s));
    phxk_margins_transpose(&b, &g, s);
    HIPCHK(c, hipEventRecord(c->aev[1], s));
    phxk_sssp_rev(&b, &g, nlm, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->aev[2], s));
    if (n) HIPCHK(c, hipMemcpyAsync(c->mstat.data(), c->b_mstat.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int k = 0; k < 2; k++) c->rev_ms[k] = ev_ms(c->aev[k], c->aev[k + 1]);
    c->done.rev = true;
    return PHX_OK;
}

// The device's records of every ORF of the batch (device order) into c->h_mrec, once per run, on top of ensure_rev.
static int ensure_margins(phx_ctx *c) {
    if (c->done.margins) return PHX_OK;
    { const int rr = ensure_rev(c); if (rr) return rr; }
    const size_t N = (size_t)c->tot_orf;
    const int nlm = margins_nl_mask(c);
    { const int rp = ensure_pinned(c, c->h_mrec, (N + 1) * sizeof(phx_orf_margin), (N + N / 4 + 1024) * sizeof(phx_orf_margin)); if (rp) return rp; }
    DBatch b;
    fill_batch(c, &b);
    DMarg g;
    margins_args(c, &g);
    hipStream_t s = c->stream;
    HIPCHK(c, hipEventRecord(c->aev[2], s));
    phxk_margins(&b, &g, nlm, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->aev[3], s));
    if (N) HIPCHK(c, hipMemcpyAsync(c->h_mrec.p, c->b_mrec.p, N * sizeof(phx_orf_margin), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->aev[4], s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->margins_ms[0] = c->rev_ms[0]; c->margins_ms[1] = c->rev_ms[1];
    for (int k = 2; k < 4; k++) c->margins_ms[k] = ev_ms(c->aev[k], c->aev[k + 1]);
    c->done.margins = true;
    return PHX_OK;
}

// status of contig i's margins (include/phx.h)
static int32_t margins_status(const phx_ctx *c, int i) {
    const int32_t r = c->res[(size_t)i].status;
    if (r < 0) return r;
    const DMeta &m = c->meta[(size_t)i];
    if (m.sssp_mode == 4 && m.n_node > 2) return PHX_S_OVERFLOW;
    if (c->mstat[(size_t)i]) return PHX_S_NEGCYCLE;
    return r;
}

static int margins_out(phx_ctx *c, const char *who, bool again, phx_orf_margin *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out);
int phx_margins_flat(phx_ctx *c, phx_orf_margin *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rx = ensure_exact(c); if (rx) return rx; } // `called` is against the genes phx_download* deliver
    { const int rm = ensure_margins(c); if (rm) return rm; }
    return margins_out(c, "phx_margins_flat", false, rec, nullptr, cap, offsets, status, total_out);
}

int phx_tap_dist_target(phx_ctx *c, int32_t contig, uint64_t *dist_limbs, int64_t cap_words) {
    TAP_PRE(c, contig);
    if (m.status < 0 || m.n_node <= 2 || m.sssp_mode == 4) return PHX_OK;
    const size_t words = (size_t)m.n_node * (size_t)m.sssp_nl;
    if (!dist_limbs || cap_words < (int64_t)words) return PHX_E_ARG;
    { const int rm = ensure_rev(c); if (rm) return rm; }
    HIPCHK(c, hipMemcpy(dist_limbs, (uint64_t *)c->b_mdt.p + (size_t)m.node_off * (size_t)c->n_limbs, words * 8, hipMemcpyDeviceToHost));
    return PHX_OK;
}

int phx_margins_ms(phx_ctx *c, float *ms) { return values_out<4>(c, ms, [](const phx_ctx *x) { return x->margins_ms; }); }

// ---- gene drop margins (phx_drop.inc, DESIGN.md §12; on a re-annotation's graph §29, §32): the pass and the rows; the families: below ----
static int64_t drop_cells(int n_path) { int lv = 1; while ((2 << (lv - 1)) <= n_path) lv++; return (int64_t)n_path * lv; }
static int drop_layered() { const char *ly = getenv("PHX_DROP_LAYERED"); return ly && *ly && strcmp(ly, "0") != 0 ? 1 : 0; }

// the kernels' view of a set (after drop_pass laid it out: roff has n + 1 entries); trees: with the one-hop trees
static void drop_args(const phx_ctx::DropSet &D, bool trees, DDrop *q) {
    const int64_t *off = (const int64_t *)D.b_off.p;
    q->pidx = (int32_t *)D.b_pi.p; q->js = (int32_t *)D.b_js.p; q->jt = (int32_t *)D.b_jt.p; q->first = (int32_t *)D.b_fi.p; q->last = (int32_t *)D.b_la.p;
    q->slot = (uint64_t *)D.b_slot.p; q->gtab = (uint64_t *)D.b_gtab.p;
    q->toff = off; q->roff = off ? off + (D.roff.size() - 1) : nullptr; // (no buffers: no contig is covered, and no kernel reads the set)
    q->sx = (uint64_t *)D.b_sx.p; q->cx = (uint64_t *)D.b_cx.p; q->da = (uint64_t *)D.b_da.p; q->db = (uint64_t *)D.b_db.p;
    q->rec = (phx_gene_drop *)D.b_rec.p; q->stats = (unsigned long long *)D.b_stats.p;
    q->layered = drop_layered();
    q->ps = trees ? (int32_t *)D.b_ps.p : nullptr; q->ts = trees ? (int32_t *)D.b_ts.p : nullptr;
}

// The drop pass, once for the three families (§12 on the run's graph, §29 and §32 on a re-annotation's): layout -> trees + labels -> candidates ->
// fix-ups -> copies.  D: the set the pass writes and what it leaves on the host — the records of every pair of every covered path in D.h_rec
// (at D.roff); covered(i): contig i's n_path, 0 when the kernels do not cover it; launch(step, q): step 0 k_dp_tree, 1 k_dp_cand, 2 the
// fix-ups, under the caller's policy; done / has_trees: the caller's flags in RunDone.  trees: the one-hop trees too (DDrop.ps / ts, for the
// replacements); a set computed without them gets k_dp_tree once more, which rewrites the same labels and counts into the second half of
// S.b_cnt (S: the replacement set that goes with D), so that the pass's own counters stay as they were.
extern "C++" template <class C, class L> static int drop_pass(phx_ctx *c, phx_ctx::DropSet &D, phx_ctx::ReplSet &S, bool &done, bool &has_trees, bool trees, const C &covered, const L &launch) {
    const size_t n = (size_t)c->n, V = (size_t)c->tot_node, nv = (V + n + 1) * 4;
    int rc;
    DDrop q;
    if (done) { // (asked for the trees alone)
        if (D.nlm) {
            if ((rc = ensure(c, D.b_ps, nv)) || (rc = ensure(c, D.b_ts, nv)) || (rc = ensure(c, S.b_cnt, 2 * RP_NCNT * 8))) return rc;
            drop_args(D, true, &q);
            q.stats = (unsigned long long *)S.b_cnt.p + RP_NCNT;
            launch(0, q);
            HIPCHK(c, hipGetLastError());
        }
        has_trees = true;
        return PHX_OK;
    }
    const size_t limbs = (size_t)std::max(c->n_limbs, 2) + (size_t)D.wide; // (the pinned set: DPmarg.dt_stride words per record and node)
    std::vector<int64_t> off(2 * n + 2, 0); // toff[n], roff[n + 1]
    D.roff.assign(n + 1, 0);
    D.nlm = 0;
    int64_t tcells = 0, R = 0;
    for (size_t i = 0; i < n; i++) {
        off[n + i] = R; D.roff[i] = R;
        const int np = covered(i);
        if (!np) continue;
        D.nlm |= nl_class_bit(c->meta[i].sssp_nl);
        const int64_t cells = drop_cells(np);
        if (cells > DP_TAB_LDS) { off[i] = tcells; tcells += cells; }
        R += (np - 1) / 2;
    }
    off[2 * n] = R; D.roff[n] = R;
    for (int k = 0; k < 4; k++) { D.ms[k] = 0; D.stats[k] = 0; }
    if (D.nlm) {
        if ((rc = ensure(c, D.b_pi, nv)) || (rc = ensure(c, D.b_js, nv)) || (rc = ensure(c, D.b_jt, nv)) || (rc = ensure(c, D.b_fi, nv)) || (rc = ensure(c, D.b_la, nv))) return rc;
        if ((rc = ensure(c, D.b_slot, (V + 1) * 8))) return rc;
        if ((rc = ensure(c, D.b_gtab, ((size_t)tcells + 1) * 8))) return rc;
        if ((rc = ensure(c, D.b_off, (2 * n + 2) * 8))) return rc;
        if ((rc = ensure(c, D.b_sx, ((size_t)R + 1) * limbs * 8)) || (rc = ensure(c, D.b_cx, ((size_t)R + 1) * limbs * 8))) return rc;
        if ((rc = ensure(c, D.b_da, (V + 1) * limbs * 8)) || (rc = ensure(c, D.b_db, (V + 1) * limbs * 8))) return rc;
        if ((rc = ensure(c, D.b_rec, ((size_t)R + 1) * sizeof(phx_gene_drop)))) return rc;
        if ((rc = ensure(c, D.b_stats, 4 * 8))) return rc;
        if (trees && ((rc = ensure(c, D.b_ps, nv)) || (rc = ensure(c, D.b_ts, nv)))) return rc;
        if (D.wide) {
            if ((rc = ensure(c, D.b_lost, ((size_t)R + 1) * 4))) return rc;
            try { D.h_lost.resize((size_t)R + 1); } catch (const std::bad_alloc &) { c->err = "out of memory in the drop margins"; return PHX_E_NOMEM; }
        }
        if ((rc = ensure_pinned(c, D.h_rec, ((size_t)R + 1) * sizeof(phx_gene_drop), ((size_t)R + (size_t)R / 4 + 1024) * sizeof(phx_gene_drop)))) return rc;
        if ((rc = analysis_events(c))) return rc;
        drop_args(D, trees, &q);
        hipStream_t s = c->stream;
        unsigned long long st[4] = {0, 0, 0, 0};
        HIPCHK(c, hipEventRecord(c->aev[0], s));
        HIPCHK(c, hipMemcpyAsync(D.b_off.p, off.data(), (2 * n + 2) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(D.b_stats.p, 0, 4 * 8, s));
        launch(0, q);
        HIPCHK(c, hipEventRecord(c->aev[1], s));
        launch(1, q);
        HIPCHK(c, hipEventRecord(c->aev[2], s));
        launch(2, q);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->aev[3], s));
        if (R) HIPCHK(c, hipMemcpyAsync(D.h_rec.p, D.b_rec.p, (size_t)R * sizeof(phx_gene_drop), hipMemcpyDeviceToHost, s));
        if (R && D.wide) HIPCHK(c, hipMemcpyAsync(D.h_lost.data(), D.b_lost.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->aev[4], s));
        HIPCHK(c, hipMemcpyAsync(st, D.b_stats.p, sizeof st, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int k = 0; k < 4; k++) { D.ms[k] = ev_ms(c->aev[k], c->aev[k + 1]); D.stats[k] = (int64_t)st[k]; }
    } // (else no contig is covered: nothing is allocated or launched)
    done = true;
    has_trees = trees;
    return PHX_OK;
}

// What the flat calls lay out of a contig's device records [k0, k1) of D: those of CDS genes (the pairs of the path that are), in path
// order, `called` from the sorted keys of the genes the contig's result delivers.
static int64_t drop_count(const phx_ctx::DropSet &D, int64_t k0, int64_t k1) {
    const phx_gene_drop *src = (const phx_gene_drop *)D.h_rec.p;
    int64_t k = 0;
    for (int64_t r = k0; r < k1; r++) k += src[r].called >= 0;
    return k;
}
// (lost: null, or where the rows' `lost` go — a set without one gives 0)
static void drop_rows(const phx_ctx::DropSet &D, int64_t k0, int64_t k1, const std::vector<uint64_t> &keys, phx_gene_drop *dst, int32_t *lost = nullptr) {
    const phx_gene_drop *src = (const phx_gene_drop *)D.h_rec.p;
    for (int64_t k = k0; k < k1; k++) {
        const phx_gene_drop &x = src[k];
        if (x.called < 0) continue;
        *dst = x;
        dst->called = is_called(keys, x.left, x.right, x.strand) ? 1 : 0;
        dst++;
        if (lost) *lost++ = D.wide ? D.h_lost[(size_t)k] : 0;
    }
}

// ---- coding profiles (phx_profile.inc, DESIGN.md §34) ----
// the contigs the profile kernels cover (pf_on): device distances and a settled reverse pass; a contig without a path is one of them
static bool profile_contig(const phx_ctx *c, size_t i) {
    const DMeta &m = c->meta[i];
    return m.status >= 0 && m.n_node > 2 && m.sssp_mode != 4 && !c->mstat[i];
}
static int64_t profile_cells(int n_slot) { int lv = 1; while ((2 << (lv - 1)) <= n_slot) lv++; return (int64_t)n_slot * lv; } // one track's table (k_pf_cand)

// The slots' records of every covered contig into c->pf.h_rec (at pf.roff), once per run, on top of ensure_rev: layout -> candidates,
// tables and push-down -> bounds -> copy.  It writes its own set only: the margins' and the drop margins' buffers are read.
static int ensure_profile(phx_ctx *c) {
    if (c->done.profile) return PHX_OK;
    { const int rr = ensure_rev(c); if (rr) return rr; }
    phx_ctx::ProfSet &P = c->pf;
    const size_t n = (size_t)c->n;
    std::vector<int64_t> off(2 * n + 2, 0); // toff[n], roff[n + 1]
    P.roff.assign(n + 1, 0);
    int nlm = 0;
    int64_t tcells = 0, R = 0;
    for (size_t i = 0; i < n; i++) {
        off[n + i] = R; P.roff[i] = R;
        if (!profile_contig(c, i)) continue;
        nlm |= nl_class_bit(c->meta[i].sssp_nl);
        const int ns = c->meta[i].n_node - 1;
        const int64_t cells = profile_cells(ns);
        if (cells > PF_TAB_LDS) { off[i] = tcells; tcells += cells; }
        R += ns;
    }
    off[2 * n] = R; P.roff[n] = R;
    for (float &m : P.ms) m = 0;
    if (nlm) {
        int rc;
        if ((rc = ensure(c, P.b_tab, ((size_t)tcells + 1) * 8))) return rc;
        if ((rc = ensure(c, P.b_off, (2 * n + 2) * 8))) return rc;
        if ((rc = ensure(c, P.b_rec, ((size_t)R + 1) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = ensure_pinned(c, P.h_rec, ((size_t)R + 1) * sizeof(phx_profile_slot), ((size_t)R + (size_t)R / 4 + 1024) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = analysis_events(c))) return rc;
        DBatch b;
        fill_batch(c, &b);
        DMarg g;
        margins_args(c, &g);
        DProf q;
        q.gtab = (uint64_t *)P.b_tab.p; q.toff = (const int64_t *)P.b_off.p; q.roff = q.toff + n; q.rec = (phx_profile_slot *)P.b_rec.p;
        hipStream_t s = c->stream;
        HIPCHK(c, hipEventRecord(c->aev[0], s));
        HIPCHK(c, hipMemcpyAsync(P.b_off.p, off.data(), (2 * n + 2) * 8, hipMemcpyHostToDevice, s));
        phxk_profile_cand(&b, &g, &q, nlm, s);
        HIPCHK(c, hipEventRecord(c->aev[1], s));
        phxk_profile_rec(&b, &g, &q, s);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->aev[2], s));
        if (R) HIPCHK(c, hipMemcpyAsync(P.h_rec.p, P.b_rec.p, (size_t)R * sizeof(phx_profile_slot), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->aev[3], s));
        HIPCHK(c, hipStreamSynchronize(s)); // (`off` is read by the copy until here)
        for (int k = 0; k < 3; k++) P.ms[k] = ev_ms(c->aev[k], c->aev[k + 1]);
    } // (else no contig is covered: nothing is allocated or launched)
    c->done.profile = true;
    return PHX_OK;
}

int phx_profile_flat(phx_ctx *c, phx_profile_slot *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rp = ensure_profile(c); if (rp) return rp; }
    const phx_ctx::ProfSet &P = c->pf;
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) { // V - 1 records for every covered contig (status 0 or PHX_S_NOPATH)
        offsets[i] = total;
        status[i] = margins_status(c, i);
        if (status[i] >= 0 && profile_contig(c, (size_t)i)) total += P.roff[(size_t)i + 1] - P.roff[(size_t)i];
    }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!rec) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    for (int i = 0; i < c->n; i++)
        if (offsets[i + 1] > offsets[i]) memcpy(rec + offsets[i], (const phx_profile_slot *)P.h_rec.p + P.roff[(size_t)i], (size_t)(offsets[i + 1] - offsets[i]) * sizeof(phx_profile_slot));
    return PHX_OK;
}

int phx_profile_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->pf.ms; }); }


// ---- drop replacements (phx_replace.inc, DESIGN.md §13) ----
// The replacement pass, once for the three families (§13 on the run's graph, §30 and §33 on a re-annotation's): pick -> cross -> regrowth -> counting
// walk -> offsets -> filling walk -> copies.  S: the DRepl set the pass writes and what it leaves on the host; R: the records of the DDrop set
// the launchers read (one per pair of every covered path); launch(step, r): step 0 k_rp_pick, 1 k_rp_cross, 2 / 3 k_rp_walk counting / filling,
// under the caller's policy; what / who: the feature and the entry point in the error texts.
extern "C++" template <class L> static int replacement_pass(phx_ctx *c, phx_ctx::ReplSet &S, size_t R, const L &launch, const char *what, const char *who) {
    const size_t n = (size_t)c->n, V = (size_t)c->tot_node;
    int rc;
    if ((rc = ensure(c, S.b_win, (R + 1) * 8)) || (rc = ensure(c, S.b_xs, (R + 1) * 4)) || (rc = ensure(c, S.b_coff, (R + 1) * 8)) ||
        (rc = ensure(c, S.b_cm, (R + 1) * 4)) || (rc = ensure(c, S.b_rnd, (V + n + 1) * 4)) || (rc = ensure(c, S.b_info, (R + 1) * 16)) ||
        (rc = ensure(c, S.b_doff, (2 * R + 2) * 8)) || (rc = ensure(c, S.b_rec, (R + 1) * sizeof(phx_gene_repl))) || (rc = ensure(c, S.b_cnt, 2 * RP_NCNT * 8)))
        return rc;
    if (!S.b_chain.p) { // room for this many delta-chain nodes (env PHX_REPL_CHAIN_CAP, the tests: fewer, so that the regrowth below runs)
        const char *cc = getenv("PHX_REPL_CHAIN_CAP");
        S.chain_cap = cc && *cc ? std::max<int64_t>(1, atoll(cc)) : (int64_t)V + 1;
        if ((rc = ensure(c, S.b_chain, ((size_t)S.chain_cap + 1) * 4))) return rc;
    }
    if ((rc = analysis_events(c))) return rc;
    try { S.h_path.assign(n, std::vector<int32_t>()); } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    DRepl r;
    auto args = [&]() {
        r.win = (uint64_t *)S.b_win.p; r.xs = (int32_t *)S.b_xs.p; r.coff = (int64_t *)S.b_coff.p; r.cm = (int32_t *)S.b_cm.p;
        r.chain = (int32_t *)S.b_chain.p; r.ccap = S.chain_cap; // (b_chain was ensured for chain_cap + 1 entries)
        r.rnd = (int32_t *)S.b_rnd.p; r.info = (int32_t *)S.b_info.p;
        r.doff = (const int64_t *)S.b_doff.p; r.goff = (const int64_t *)S.b_doff.p + R + 1;
        r.det = (int32_t *)S.b_det.p; r.genes = (phx_gene *)S.b_genes.p; r.rec = (phx_gene_repl *)S.b_rec.p;
        r.cnt = (unsigned long long *)S.b_cnt.p;
    };
    args();
    hipStream_t s = c->stream;
    // The event pairs bracket device work only: the host's read-backs and offsets between the passes fall outside every pair.
    unsigned long long cnt[RP_NCNT] = {0};
    hipEvent_t *ev = c->aev;
    bool regrown = false;
    HIPCHK(c, hipEventRecord(ev[0], s));
    HIPCHK(c, hipMemsetAsync(S.b_cnt.p, 0, RP_NCNT * 8, s));
    HIPCHK(c, hipMemsetAsync(S.b_win.p, 0xff, (R + 1) * 8, s));
    launch(0, r);
    launch(1, r);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[1], s));
    HIPCHK(c, hipMemcpyAsync(cnt, S.b_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((int64_t)cnt[0] > r.ccap) { // the delta chains did not fit: room for all of them, and the cross winners once more
        S.chain_cap = (int64_t)cnt[0];
        if ((rc = ensure(c, S.b_chain, ((size_t)S.chain_cap + 1) * 4))) return rc;
        args();
        regrown = true;
        HIPCHK(c, hipEventRecord(ev[2], s));
        HIPCHK(c, hipMemsetAsync(S.b_cnt.p, 0, RP_NCNT * 8, s));
        launch(1, r);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev[3], s));
        HIPCHK(c, hipMemcpyAsync(cnt, S.b_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if ((int64_t)cnt[0] > r.ccap) { c->err = std::string(what) + ": the delta chains outgrew their buffer twice"; return PHX_E_STATE; }
    }
    // counting pass, offsets, filling pass
    HIPCHK(c, hipEventRecord(ev[4], s));
    launch(2, r);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[5], s));
    S.h_info.resize(4 * R + 4);
    if (R) HIPCHK(c, hipMemcpyAsync(S.h_info.data(), S.b_info.p, R * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(cnt, S.b_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (cnt[1]) { c->err = std::string(what) + ": a slot with a bypass has no witness"; return PHX_E_STATE; }
    S.stats[0] = (int64_t)cnt[2]; S.stats[1] = (int64_t)cnt[0]; S.stats[2] = (int64_t)cnt[3]; S.stats[3] = (int64_t)cnt[4];
    S.stats[4] = regrown ? 1 : 0;
    try {
        std::vector<int64_t> off(2 * R + 2);
        int64_t nd = 0, ng = 0;
        for (size_t k = 0; k < R; k++) { off[k] = nd; off[R + 1 + k] = ng; nd += S.h_info[4 * k + 2]; ng += S.h_info[4 * k + 3]; }
        off[R] = nd; off[2 * R + 1] = ng;
        S.h_doff.assign(off.begin(), off.begin() + (R + 1));
        if ((rc = ensure(c, S.b_det, ((size_t)nd + 1) * 4)) || (rc = ensure(c, S.b_genes, ((size_t)ng + 1) * sizeof(phx_gene)))) return rc;
        args();
        HIPCHK(c, hipMemcpyAsync(S.b_doff.p, off.data(), (2 * R + 2) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(ev[6], s));
        launch(3, r);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev[7], s));
        S.h_rec.resize(R + 1); S.h_det.resize((size_t)nd + 1); S.h_genes.resize((size_t)ng + 1);
        if (R) HIPCHK(c, hipMemcpyAsync(S.h_rec.data(), S.b_rec.p, R * sizeof(phx_gene_repl), hipMemcpyDeviceToHost, s));
        if (nd) HIPCHK(c, hipMemcpyAsync(S.h_det.data(), S.b_det.p, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
        if (ng) HIPCHK(c, hipMemcpyAsync(S.h_genes.data(), S.b_genes.p, (size_t)ng * sizeof(phx_gene), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(ev[8], s));
        HIPCHK(c, hipStreamSynchronize(s));
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    auto span = [&](int k0, int k1) { return ev_ms(ev[k0], ev[k1]); };
    S.ms[0] = span(0, 1) + (regrown ? span(2, 3) : 0.0f);
    S.ms[1] = span(4, 5) + span(6, 7);
    S.ms[2] = span(7, 8);
    return PHX_OK;
}

// The layout the flat calls share: the records of contig i (device records [k0, k1) of S, those of CDS genes) to dst, `called` from the
// drop records dd they go with (whose `lost` is theirs too), their genes appended to `genes` at *go, gene_off rebased.
static void replacement_rows(const phx_ctx::ReplSet &S, int64_t k0, int64_t k1, const phx_gene_drop *dd, phx_gene_repl *dst, phx_gene *genes, int64_t *go) {
    for (int64_t k = k0; k < k1; k++) {
        const phx_gene_repl &x = S.h_rec[(size_t)k];
        if (x.called < 0) continue;
        *dst = x;
        dst->called = dd->called;
        dst->gene_off = *go;
        const int64_t ng = x.n_removed + x.n_added;
        if (ng) memcpy(genes + *go, S.h_genes.data() + x.gene_off, (size_t)ng * sizeof(phx_gene));
        *go += ng;
        dst++; dd++;
    }
}
static int64_t replacement_genes(const phx_ctx::ReplSet &S, int64_t k0, int64_t k1) {
    int64_t gt = 0;
    for (int64_t k = k0; k < k1; k++) if (S.h_rec[(size_t)k].called >= 0) gt += S.h_rec[(size_t)k].n_removed + S.h_rec[(size_t)k].n_added;
    return gt;
}
// The path of the k-th record of a contig, every tap: device records [k0, k1) of S, on the path of n_path nodes at dpath (device).
static int replacement_tap(phx_ctx *c, phx_ctx::ReplSet &S, const char *who, int32_t contig, int64_t k0, int64_t k1, int32_t k, const int32_t *dpath, int np, int32_t *path, int32_t cap, int32_t *n_path) {
    int64_t rk = -1;
    for (int64_t q = k0, seen = 0; q < k1; q++)
        if (S.h_rec[(size_t)q].called >= 0 && seen++ == k) { rk = q; break; }
    if (rk < 0) return PHX_E_ARG;
    if (!S.h_rec[(size_t)rk].bypass) return PHX_OK;
    const int a = S.h_info[4 * rk], b = S.h_info[4 * rk + 1], nd = S.h_info[4 * rk + 2];
    const int len = (a + 1) + nd + (np - b);
    *n_path = len;
    if (!path) return PHX_OK;
    if (cap < len) return PHX_E_ARG;
    std::vector<int32_t> &P = S.h_path[(size_t)contig]; // (the contig's device path, fetched at its first tap of this result)
    if (P.empty()) {
        try { P.resize((size_t)np); } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
        HIPCHK(c, hipMemcpy(P.data(), dpath, (size_t)np * 4, hipMemcpyDeviceToHost));
    }
    int32_t *o = path;
    for (int t = 0; t <= a; t++) *o++ = P[(size_t)t];
    for (int t = 0; t < nd; t++) *o++ = S.h_det[(size_t)S.h_doff[(size_t)rk] + t];
    for (int t = b; t < np; t++) *o++ = P[(size_t)t];
    return PHX_OK;
}

// ---- masked re-annotation (phx_resolve.inc, DESIGN.md §14) ----
// status of contig i's re-annotation before any kernel: a run error, PHX_S_OVERFLOW without device distances, else the run's status
static int32_t reann_status(const phx_ctx *c, int i) {
    const DMeta &m = c->meta[(size_t)i];
    if (m.sssp_mode == 4 && m.n_node > 2 && m.status >= 0) return PHX_S_OVERFLOW;
    const int32_t r = c->res[(size_t)i].status;
    return r < 0 ? r : m.status; // (the device's own status: exactness does not enter)
}
static bool reann_contig(const phx_ctx *c, int i) { const DMeta &m = c->meta[(size_t)i]; return reann_status(c, i) >= 0 && m.n_node > 2; }

// A re-solve's view of the batch: the run's graph, read only, with totals, gene records, gene counter and tie scratch of the solve's own
// (reann_batch for the re-annotation, scen_compute for a chunk of scenario slots) — nothing the run's results live in is written.
static void resolve_batch(phx_ctx *c, DBatch *b, const DevBuf &tot, const DevBuf &genes, const DevBuf &gtot, const DevBuf &tie) {
    fill_batch(c, b);
    b->tot = (DTotals *)tot.p; b->res = nullptr; b->sord = nullptr; b->lpart = nullptr;
    b->genes = (DGene *)genes.p; b->genes_c = nullptr; b->gpack = 0; b->gene_total = (uint32_t *)gtot.p;
    b->tie = (uint8_t *)tie.p; b->tie_cap = cap_of(tie, 1, 0);
}
// The re-annotation's: records, distances, parents and paths of its own besides.  b_qsel holds mode | nreq | kreq, n + 1 entries each;
// b_qmask the refused, the required and the biased bitmap (the evidence buffers exist once a call has biased a contig; no kernel reads them before).
static void reann_batch(phx_ctx *c, DBatch *b, DReann *q) {
    resolve_batch(c, b, c->b_qtot, c->b_qgenes, c->b_qgtot, c->b_qtie);
    b->meta = (DMeta *)c->b_qmeta.p;
    b->dist = (uint64_t *)c->b_qdist.p; b->parent = (int32_t *)c->b_qparent.p; b->path = (int32_t *)c->b_qpath.p;
    b->dist_stride = c->qstride; // (one limb wider than the run's when a contig is solved under the required policy, §16)
    const size_t n1 = (size_t)c->n + 1, mw = (size_t)c->tot_edge / 32 + 2;
    q->mode = (const int32_t *)c->b_qsel.p; q->nreq = q->mode + n1; q->kreq = (int32_t *)c->b_qsel.p + 2 * n1;
    q->forb = (const uint8_t *)c->b_qforb.p; q->bias = (const long long *)c->b_qbias.p;
    q->mask = (uint32_t *)c->b_qmask.p; q->req = q->mask + mw; q->bbit = q->mask + 2 * mw;
    q->bval = (long long *)c->b_qbval.p; q->bsum = (unsigned long long *)c->b_qbsum.p;
    q->gplan = (uint8_t *)c->b_qplan.p; q->dist0 = (const uint64_t *)c->b_dist.p; q->stride0 = c->n_limbs; q->rec = (DReannRec *)c->b_qrec.p;
}

// What one re-solve — the re-annotation's, or a chunk of scenario slots — owns on the device and reads back.
struct ReSolve {
    const char *what, *unit;             // the error texts' prefix ("re-annotation" / "scenarios") and what a record stands for
    DevBuf &tot, &gtot, &tie, &rec, &genes;
    DTotals &h_tot;                      // the totals and the gene count as read back: members of the context (see h_qdforb)
    uint32_t &h_gtot;
    DReannRec *h_rec;                    // the n_rec records as read back
    size_t n_rec, gene_bound;            // ... and how many gene records the solve may write
    std::vector<DGene> &h_genes;         // the gene records are appended here (gene_off of a record counts from where they start)
};
// One re-solve with its tie-scratch retry.  begin(attempt): the caller's views of the buffers (the tie scratch may have grown) and the reset
// of whatever its mask kernels count or sum; launch(step): its mask (0), solve (1) and finish (2) kernels.  ms[3]: device time of mask,
// solve and finish + gene copy of the attempt that settled.
extern "C++" template <class Begin, class Launch> static int resolve_attempts(phx_ctx *c, const ReSolve &R, float *ms, Begin begin, Launch launch) {
    int rc;
    hipStream_t s = c->stream;
    DTotals &tot = R.h_tot;
    uint32_t &gtot = R.h_gtot;
    gtot = 0;
    for (int attempt = 0;; attempt++) {
        HIPCHK(c, hipEventRecord(c->aev[0], s));
        HIPCHK(c, hipMemsetAsync(R.tot.p, 0, sizeof(DTotals), s));
        HIPCHK(c, hipMemsetAsync(R.gtot.p, 0, 16, s));
        if ((rc = begin(attempt))) return rc;
        launch(0);
        HIPCHK(c, hipEventRecord(c->aev[1], s));
        launch(1);
        HIPCHK(c, hipEventRecord(c->aev[2], s));
        launch(2);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(R.h_rec, R.rec.p, R.n_rec * sizeof(DReannRec), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->aev[3], s));
        HIPCHK(c, hipMemcpyAsync(&tot, R.tot.p, sizeof(DTotals), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&gtot, R.gtot.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (!(tot.overflow & 4)) break;
        // the in-order pass's scratch was too small for the contigs with equal-length alternatives: grow it and solve again
        if (attempt >= 2) { c->err = std::string(R.what) + ": the tie scratch did not settle"; return PHX_E_STATE; }
        if ((rc = ensure(c, R.tie, (size_t)tot.tie_need + (size_t)tot.tie_need / 4 + 4096))) return rc;
    }
    if ((size_t)gtot > R.gene_bound) { c->err = std::string(R.what) + ": gene records beyond the buffer"; return PHX_E_STATE; }
    const size_t base = R.h_genes.size();
    R.h_genes.resize(base + gtot);
    HIPCHK(c, hipEventRecord(c->aev[4], s));
    if (gtot) HIPCHK(c, hipMemcpyAsync(R.h_genes.data() + base, R.genes.p, (size_t)gtot * sizeof(DGene), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->aev[5], s));
    HIPCHK(c, hipStreamSynchronize(s));
    ms[0] = ev_ms(c->aev[0], c->aev[1]);
    ms[1] = ev_ms(c->aev[1], c->aev[2]);
    ms[2] = ev_ms(c->aev[2], c->aev[3]) + ev_ms(c->aev[4], c->aev[5]);
    for (size_t k = 0; k < R.n_rec; k++) {
        const DReannRec &r = R.h_rec[k];
        if (r.n_genes < 0 || r.gene_off < 0 || (uint64_t)r.gene_off + (uint64_t)r.n_genes > (uint64_t)gtot) { c->err = std::string(R.what) + ": a " + R.unit + "'s gene records lie outside the buffer"; return PHX_E_STATE; }
    }
    return PHX_OK;
}

// Solves the contigs of h_qsel again (1: masked, 2: under the required policy, 3: under the bias policy, 4: under both, §22) with the ORFs of `forb` (tap order;
// 1 = refused, 2 = required, h_qnreq of them per contig) and the integers of `bias` (tap order; null: none); the records into h_qrec, the
// genes into h_qgenes.
static int reann_compute(phx_ctx *c, const uint8_t *forb, const int64_t *bias, const int64_t *orf_offsets) {
    const size_t n = (size_t)c->n, V = (size_t)c->tot_node, E = (size_t)c->tot_edge, N = (size_t)c->tot_orf;
    const size_t limbs = (size_t)std::max(c->n_limbs, 2);
    { const int rg = ensure_grp_host(c); if (rg) return rg; }
    // the mask in device ORF order: the inverse of the permutation phx_margins_flat applies to its records
    std::vector<uint8_t> &dforb = c->h_qdforb;
    dforb.assign(N + 1, 0);
    std::vector<int> order;
    int nlm[RE_MODES] = {0, 0, 0, 0, 0}; // per mode: the limb classes of its contigs
    bool any = false, any_req = false, any_bias = false;
    std::vector<int32_t> &dsel = c->h_qdsel; // what the kernels read: mode | nreq | kreq (zero), n + 1 entries each
    dsel.assign(3 * (n + 1), 0);
    std::vector<int64_t> &dbias = c->h_qdbias;
    if (bias) dbias.assign(N + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if (!c->h_qsel[i]) continue;
        any = true;
        const DMeta &m = c->meta[i];
        const int mode = c->h_qsel[i];
        nlm[mode] |= nl_class_bit(m.sssp_nl);
        dsel[i] = mode;
        if (re_mode_req(mode)) { any_req = true; dsel[n + 1 + i] = c->h_qnreq[i]; }
        any_bias = any_bias || re_mode_bias(mode);
        const uint8_t *from = forb + orf_offsets[i];
        const int64_t *bfrom = bias ? bias + orf_offsets[i] : nullptr;
        each_group_in_reference_order(c, i, order, [&](int32_t first, int32_t k) {
            if (k > 0 && first >= 0 && (int64_t)first + k <= m.n_orf) {
                memcpy(dforb.data() + m.orf_off + first, from, (size_t)k);
                if (bfrom) memcpy(dbias.data() + m.orf_off + first, bfrom, (size_t)k * 8);
            }
            from += k;
            if (bfrom) bfrom += k;
        });
    }
    c->h_qrec.assign(n, DReannRec{});
    c->h_qgenes.clear();
    if (!any) return PHX_OK;
    int rc;
    c->qstride = (int)limbs + (any_req ? 1 : 0);
    const size_t mw = E / 32 + 2; // words of one bitmap; the required ORFs' follows the refused ORFs' in b_qmask
    if ((rc = ensure(c, c->b_qmeta, (n + 1) * sizeof(DMeta))) || (rc = ensure(c, c->b_qtot, sizeof(DTotals))) || (rc = ensure(c, c->b_qdist, (V + 1) * (size_t)c->qstride * 8)) ||
        (rc = ensure(c, c->b_qparent, (V + 1) * 4)) || (rc = ensure(c, c->b_qpath, (V + 1) * 4)) || (rc = ensure(c, c->b_qgenes, (V + n + 1) * sizeof(DGene))) || // (a path has at most V / 2 pairs, one replaced by k_rs_inorder takes new slots)
        (rc = ensure(c, c->b_qgtot, 16)) || (rc = ensure(c, c->b_qmask, 3 * mw * 4)) || (rc = ensure(c, c->b_qforb, N + 1)) || (rc = ensure(c, c->b_qsel, 3 * (n + 1) * 4)) ||
        (rc = ensure(c, c->b_qplan, V / 32 + n + 2)) || (rc = ensure(c, c->b_qrec, (n + 1) * sizeof(DReannRec))))
        return rc;
    if (!c->b_qtie.p && (rc = ensure(c, c->b_qtie, (size_t)std::max<int64_t>(c->tie_seen, 1 << 20)))) return rc;
    if (any_bias && ((rc = ensure(c, c->b_qbias, (N + 1) * 8)) || (rc = ensure(c, c->b_qbval, (E + 1) * 8)) || (rc = ensure(c, c->b_qbsum, 2 * (n + 1) * 8)))) return rc;
    if ((rc = analysis_events(c))) return rc;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->b_qforb.p, dforb.data(), N + 1, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->b_qsel.p, dsel.data(), 3 * (n + 1) * 4, hipMemcpyHostToDevice, s));
    if (any_bias) HIPCHK(c, hipMemcpyAsync(c->b_qbias.p, dbias.data(), (N + 1) * 8, hipMemcpyHostToDevice, s));
    DBatch b;
    DReann q;
    const ReSolve R{"re-annotation", "contig", c->b_qtot, c->b_qgtot, c->b_qtie, c->b_qrec, c->b_qgenes, c->h_qtot, c->h_qgtot, c->h_qrec.data(), n, V + n, c->h_qgenes};
    return resolve_attempts(c, R, c->reann_ms, [&](int attempt) -> int {
        reann_batch(c, &b, &q);
        HIPCHK(c, hipMemcpyAsync(c->b_qmeta.p, c->b_meta.p, n * sizeof(DMeta), hipMemcpyDeviceToDevice, s)); // the layout and the run's verdicts; the kernels write this copy
        HIPCHK(c, hipMemsetAsync(c->b_qrec.p, 0, (n + 1) * sizeof(DReannRec), s));
        HIPCHK(c, hipMemsetAsync(c->b_qmask.p, 0, (any_bias ? 3 : any_req ? 2 : 1) * mw * 4, s));
        if (any_req && attempt) HIPCHK(c, hipMemsetAsync((int32_t *)c->b_qsel.p + 2 * (n + 1), 0, (n + 1) * 4, s)); // k_rs_mask counts again
        if (any_bias) HIPCHK(c, hipMemsetAsync(c->b_qbsum.p, 0, 2 * (n + 1) * 8, s)); // (... and sums again)
        return PHX_OK;
    }, [&](int step) {
        if (step == 0) phxk_reann_mask(&b, &q, s);
        else if (step == 1) phxk_reann_solve(&b, &q, nlm, s);
        else phxk_reann_finish(&b, &q, nlm, s);
    });
}

// The caller's orf_offsets must be the batch's cumulative ORF counts (what phx_margins_flat reports): nothing from the caller indexes device
// memory unchecked.  *total: their sum.
static bool orf_offsets_ok(const phx_ctx *c, const int64_t *orf_offsets, int64_t *total) {
    int64_t acc = 0;
    for (int i = 0; i < c->n; i++) {
        if (orf_offsets[i] != acc) return false;
        if (reann_status(c, i) >= 0) acc += c->meta[(size_t)i].n_orf;
    }
    *total = acc;
    return c->n <= 0 || orf_offsets[c->n] == acc;
}
// One entry of a re-solve's layout for the caller: contig i's result under record r, or with r null — not solved again — the run's (the
// device's lists: no host re-solve enters); n_req: the required ORFs named for it.  Returns the entry's gene count; resolve_genes: where they lie.
static int64_t resolve_entry(const phx_ctx *c, int i, const DReannRec *r, int64_t n_req, int32_t *status, double *delta, int32_t *unmet) {
    const int32_t st = reann_status(c, i);
    *status = st; *delta = std::numeric_limits<double>::infinity();
    if (unmet) *unmet = (int32_t)n_req; // (no result: every required ORF is unmet)
    if (st < 0) return 0;
    if (!r) { if (st != PHX_S_NOPATH) *delta = 0.0; return std::max(c->res[(size_t)i].n_genes, 0); }
    *status = r->status; *delta = r->delta;
    if (unmet) *unmet = r->unmet;
    return r->status >= 0 ? r->n_genes : 0;
}
static const DGene *resolve_genes(const phx_ctx *c, int i, const DReannRec *r, const std::vector<DGene> &again) { return r ? again.data() + r->gene_off : (const DGene *)c->h_genes.p + (size_t)c->res[(size_t)i].gene_off; }

// phx_reannotate_flat (require and unmet null, forbid needed), phx_constrain_flat (either set may be null: empty), phx_evidence_flat (bias
// and forbid may be null, require is) and phx_curate_flat (any of the three may be null) are one solve on one set of buffers; the cached result is keyed on both sets (h_qforb holds 1 = refused,
// 2 = required per ORF) and on the bias (h_qbias; empty when every B is zero, which makes the call phx_reannotate_flat).
#define PHX_BIAS_MAX (1ll << 52) // |B| beyond it is PHX_E_ARG: the sum of a contig's |B| stays below 2^83, and ew_decode never reads a B as a wide row
static int reann_flat(phx_ctx *c, const char *who, bool need_forbid, const uint8_t *forbid, const uint8_t *require, const int64_t *bias, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes,
                      int64_t cap, int64_t *offsets, int32_t *status, double *delta, int32_t *unmet, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status || !delta || !orf_offsets))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rf = fetch_meta(c); if (rf) return rf; }
    try {
    int64_t acc = 0;
    if (!orf_offsets_ok(c, orf_offsets, &acc)) return PHX_E_ARG;
    if (acc > 0 && need_forbid && !forbid) return PHX_E_ARG;
    const size_t N = (size_t)acc;
    std::vector<uint8_t> &code = c->h_qcode; // per ORF: 1 = refused, 2 = required
    code.assign(N, 0);
    for (size_t k = 0; k < N; k++) {
        const bool f = forbid && forbid[k], r = require && require[k];
        if (f && r) { c->err = std::string(who) + ": an ORF is both refused and required"; return PHX_E_ARG; } // before any kernel
        code[k] = f ? 1 : (r ? 2 : 0);
    }
    std::vector<int64_t> &bcur = c->h_qbcur;
    bcur.clear();
    if (bias) {
        bool some = false;
        for (size_t k = 0; k < N; k++) {
            if (bias[k] > PHX_BIAS_MAX || bias[k] < -PHX_BIAS_MAX) { c->err = std::string(who) + ": a bias beyond 2^52"; return PHX_E_ARG; } // before any kernel
            some = some || bias[k] != 0;
        }
        if (some) bcur.assign(bias, bias + N);
    }
    if (!(c->done.reann && c->h_qflags == flags && c->h_qforb == code && c->h_qbias == bcur)) {
        c->done.reann = false;
        c->done.remarg = false; // (the re-annotation margins are this solve's)
        c->done.pinmarg = false;
        c->done.pinprofile = false;
        c->done.pindrop = false;
        c->done.pintrees = false;
        c->done.pinrepl = false;
        c->done.redrop = false;
        c->done.retrees = false;
        c->done.rerepl = false;
        c->done.reprofile = false;
        c->h_qsel.assign((size_t)c->n, 0);
        c->h_qnreq.assign((size_t)c->n, 0);
        for (int i = 0; i < c->n; i++) {
            int32_t nf = 0, nr = 0, nb = 0, nbk = 0; // (nbk: the biases that count beside a required set — a refused ORF's is ignored)
            for (int64_t k = orf_offsets[i]; k < orf_offsets[i + 1]; k++) {
                const bool bk = !bcur.empty() && bcur[(size_t)k] != 0;
                nf += code[(size_t)k] == 1; nr += code[(size_t)k] == 2; nb += bk; nbk += bk && code[(size_t)k] != 1;
            }
            c->h_qnreq[(size_t)i] = nr;
            if (!reann_contig(c, i)) continue;
            c->h_qsel[(size_t)i] = nr ? (nbk ? 4 : 2) : (nb ? 3 : ((flags & 1u) != 0 || nf ? 1 : 0)); // (4: required and biased ORFs in one contig, phx_curate_flat alone brings both)
        }
        { const int rq = reann_compute(c, code.data(), bcur.empty() ? nullptr : bcur.data(), orf_offsets); if (rq) { (void)hipStreamSynchronize(c->stream); return rq; } } // (nothing of a failed solve stays in flight)
        c->h_qbias = bcur;
        c->h_qforb = code;
        c->h_qflags = flags;
        c->done.reann = true;
    }
    // the run's own genes for the contigs that were not solved again
    auto rec_of = [&](int i) { return c->h_qsel[(size_t)i] ? &c->h_qrec[(size_t)i] : nullptr; };
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) {
        offsets[i] = total;
        total += resolve_entry(c, i, rec_of(i), c->h_qnreq[(size_t)i], status + i, delta + i, unmet ? unmet + i : nullptr);
    }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!genes) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    { const int rg = stage_run_genes(c, c->h_qsel.data()); if (rg) return rg; } // (of the contigs that were not solved again)
    for (int i = 0; i < c->n; i++) {
        const int64_t k = offsets[i + 1] - offsets[i];
        if (k <= 0) continue;
        memcpy(genes + offsets[i], resolve_genes(c, i, rec_of(i), c->h_qgenes), sizeof(phx_gene) * (size_t)k);
    }
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    return PHX_OK;
}

int phx_reannotate_flat(phx_ctx *c, const uint8_t *forbid, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status,
                        double *delta, int64_t *total_out) {
    return reann_flat(c, "phx_reannotate_flat", true, forbid, nullptr, nullptr, orf_offsets, flags, genes, cap, offsets, status, delta, nullptr, total_out);
}

int phx_constrain_flat(phx_ctx *c, const uint8_t *forbid, const uint8_t *require, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets,
                       int32_t *status, double *delta, int32_t *unmet, int64_t *total_out) {
    if (!c || (c->n > 0 && !unmet)) return PHX_E_ARG;
    return reann_flat(c, "phx_constrain_flat", false, forbid, require, nullptr, orf_offsets, flags, genes, cap, offsets, status, delta, unmet, total_out);
}

int phx_evidence_flat(phx_ctx *c, const int64_t *bias, const uint8_t *forbid, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status,
                      double *delta, int64_t *total_out) {
    return reann_flat(c, "phx_evidence_flat", false, forbid, nullptr, bias, orf_offsets, flags, genes, cap, offsets, status, delta, nullptr, total_out);
}

int phx_curate_flat(phx_ctx *c, const int64_t *bias, const uint8_t *forbid, const uint8_t *require, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap,
                    int64_t *offsets, int32_t *status, double *delta, int32_t *unmet, int64_t *total_out) {
    if (!c || (c->n > 0 && !unmet)) return PHX_E_ARG;
    return reann_flat(c, "phx_curate_flat", false, forbid, require, bias, orf_offsets, flags, genes, cap, offsets, status, delta, unmet, total_out);
}

int phx_orf_offsets(phx_ctx *c, int64_t *orf_offsets) {
    if (!c || !orf_offsets) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rf = fetch_meta(c); if (rf) return rf; }
    int64_t acc = 0;
    for (int i = 0; i < c->n; i++) { orf_offsets[i] = acc; if (reann_status(c, i) >= 0) acc += c->meta[(size_t)i].n_orf; }
    orf_offsets[c->n] = acc;
    return PHX_OK;
}

int phx_tap_repath(phx_ctx *c, int32_t contig, int32_t *path, int32_t cap, int32_t *n_path, uint64_t *dist_limbs, int32_t cap_limbs) {
    if (c && c->ran && !c->in_flight && !c->done.reann) return PHX_E_STATE; // no re-annotation of this run
    TAP_PRE(c, contig);
    if (!c->done.reann) return PHX_E_STATE;
    if (!c->h_qsel[(size_t)contig]) { // the run's result stands
        if (reann_status(c, contig) < 0) { if (n_path) *n_path = 0; return PHX_OK; }
        return phx_tap_path(c, contig, path, cap, n_path, dist_limbs, cap_limbs);
    }
    const DReannRec &r = c->h_qrec[(size_t)contig];
    if (n_path) *n_path = 0;
    if (r.status < 0 || r.n_path <= 0) return PHX_OK;
    if (n_path) *n_path = r.n_path;
    if (path) {
        if (cap < r.n_path) return PHX_E_ARG;
        HIPCHK(c, hipMemcpy(path, (int32_t *)c->b_qpath.p + m.node_off, (size_t)r.n_path * 4, hipMemcpyDeviceToHost));
    }
    if (dist_limbs) {
        if (cap_limbs < m.sssp_nl) return PHX_E_ARG;
        // (a contig solved under the required policy keeps one limb more per node: the W-sum is the low sssp_nl limbs of its distance)
        const size_t tgt = (size_t)m.node_off * (size_t)c->qstride + ((size_t)m.n_node - 1) * (size_t)(m.sssp_nl + (re_mode_req(c->h_qsel[(size_t)contig]) ? 1 : 0));
        HIPCHK(c, hipMemcpy(dist_limbs, (uint64_t *)c->b_qdist.p + tgt, (size_t)m.sssp_nl * 8, hipMemcpyDeviceToHost));
    }
    return PHX_OK;
}

int phx_reannotate_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->reann_ms; }); }

// ---- the conditioned margins (phx_margins.inc): per-ORF path margins on the last re-annotation's graph ----
// Two policies share one driver.  The re-annotation margins (DESIGN.md §21) cover the contigs solved again without a required ORF (modes 1
// and 3, the MgCond kernels, c->xm); the pinned margins (§24) the contigs solved under the required policy (modes 2 and 4, the MgPin
// kernels on one limb more, c->pm, with a third bitmap and `lost`).
#define WINF_TOP_HOST 0x7fffffffffffffffull // the solver's "unreached" top limb (WINF_TOP, phx_sssp.inc)
struct CmPlain {
    typedef DRmarg Rec;
    static constexpr bool pinned = false;
    static constexpr const char *who = "phx_remargins_flat";
    static constexpr auto apply = phxk_remarg_apply;
    static constexpr auto rev = phxk_remarg_rev, records = phxk_remarg_records;
};
struct CmPin {
    typedef DPmarg Rec;
    static constexpr bool pinned = true;
    static constexpr const char *who = "phx_pinmargins_flat";
    static constexpr auto apply = phxk_pinmarg_apply;
    static constexpr auto rev = phxk_pinmarg_rev, records = phxk_pinmarg_records;
};
// PHX_OK when the context holds a re-annotation the re-annotation margins are defined for
static int remarg_state(phx_ctx *c, const char *who) {
    if (!c->done.reann) { c->err = std::string(who) + ": no re-annotation of this run (call phx_reannotate_flat or phx_evidence_flat first)"; return PHX_E_STATE; }
    for (int i = 0; i < c->n; i++)
        if (re_mode_req(c->h_qsel[(size_t)i])) { c->err = std::string(who) + ": the last re-annotation solved a contig under the required policy; margins under required ORFs are not defined here"; return PHX_E_STATE; }
    return PHX_OK;
}

// The records of every ORF of the policy's contigs (device order) into m.h_rec (`lost` into m.h_lost) and the pass's verdicts into m.mstat,
// once per re-annotation solve.  CmPlain builds on ensure_margins — that gives the out-edge CSR, the run's records for the contigs that were
// not solved again and the run's mstat —, CmPin on CmPlain.  Reads what the solve left resident (b_qforb, b_qbias, b_qmask, b_qbval,
// b_qdist: nothing between a re-annotation and this call writes them — only reann_compute does, and the scenario batches own b_sc_*);
// writes only m's buffers.  m.ms: the device time; the pinned margins' is that of both parts as computed for this solve.
// the kernels' view of a policy's buffers (the fields DRmarg and DPmarg share; mw: words of one bitmap over the out-edge positions)
extern "C++" template <class R> static void condmargins_args(const phx_ctx *c, const phx_ctx::CondMarg &m, size_t mw, R *r) {
    r->sel = (const int32_t *)m.b_sel.p; r->ds = (const uint64_t *)c->b_qdist.p; r->ds_stride = c->qstride;
    r->fbit = (uint32_t *)m.b_bit.p; r->bbit = r->fbit + mw; r->bval = (long long *)m.b_bval.p;
    r->dist_t = (uint64_t *)m.b_dt.p; r->rec = (phx_orf_margin *)m.b_rec.p; r->mstat = (int32_t *)m.b_mstat.p;
}
extern "C++" template <class P> static int ensure_condmargins(phx_ctx *c) {
    phx_ctx::CondMarg &m = P::pinned ? c->pm : c->xm;
    bool &done = P::pinned ? c->done.pinmarg : c->done.remarg;
    if (done) return PHX_OK;
    const bool fresh = P::pinned && !c->done.remarg; // the re-annotation margins are computed by this same call
    { const int rm = P::pinned ? ensure_condmargins<CmPlain>(c) : ensure_margins(c); if (rm) return rm; }
    const size_t n = (size_t)c->n, V = (size_t)c->tot_node, E = (size_t)c->tot_edge, N = (size_t)c->tot_orf;
    const size_t limbs = (size_t)std::max(c->n_limbs, 2) + (P::pinned ? 1 : 0);
    const size_t mw = E / 32 + 2, nbit = P::pinned ? 3 : 2; // words of one bitmap over the out-edge positions; refused, biased, required
    int rev_nlm = 0, rec_nlm = 0;
    bool biased = false;
    m.h_sel.assign(n + 1, 0);
    m.mstat.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if (!c->h_qsel[i] || re_mode_req(c->h_qsel[i]) != P::pinned || !reann_contig(c, (int)i)) continue;
        const int32_t st = c->h_qrec[i].status;
        if (st < 0) continue;
        m.h_sel[i] = st == 0 ? 1 : 2; // (PHX_S_NOPATH: records only, D' is unreached)
        rec_nlm |= nl_class_bit(c->meta[i].sssp_nl);
        if (st == 0) { rev_nlm |= nl_class_bit(c->meta[i].sssp_nl); biased = biased || re_mode_bias(c->h_qsel[i]); }
    }
    for (int k = 0; k < 4; k++) m.ms[k] = fresh ? c->xm.ms[k] : 0;
    if (!rec_nlm) { done = true; return PHX_OK; }
    int rc;
    if ((rc = ensure(c, m.b_sel, (n + 1) * 4)) || (rc = ensure(c, m.b_bit, nbit * mw * 4)) || (biased && (rc = ensure(c, m.b_bval, (E + 1) * 8))) ||
        (rc = ensure(c, m.b_dt, (V + 1) * limbs * 8)) || (rc = ensure(c, m.b_rec, (N + 1) * sizeof(phx_orf_margin))) || (P::pinned && (rc = ensure(c, m.b_lost, (N + 1) * 4))) ||
        (rc = ensure(c, m.b_mstat, (n + 1) * 4)))
        return rc;
    if ((rc = analysis_events(c))) return rc;
    try { m.h_rec.resize(N + 1); if (P::pinned) m.h_lost.resize(N + 1); } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + P::who; return PHX_E_NOMEM; }
    DBatch b;
    fill_batch(c, &b);
    DMarg g;
    margins_args(c, &g);
    DBatch qb;
    DReann q;
    reann_batch(c, &qb, &q);
    typename P::Rec r;
    condmargins_args(c, m, mw, &r);
    if constexpr (P::pinned) { r.dt_stride = b.dist_stride + 1; r.rbit = r.fbit + 2 * mw; r.lost = (int32_t *)m.b_lost.p; }
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(m.b_sel.p, m.h_sel.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->aev[0], s));
    HIPCHK(c, hipMemsetAsync(m.b_bit.p, 0, nbit * mw * 4, s));
    HIPCHK(c, hipMemsetAsync(m.b_mstat.p, 0, (n + 1) * 4, s));
    if (rev_nlm) P::apply(&b, &g, &q, &r, s);
    HIPCHK(c, hipEventRecord(c->aev[1], s));
    if (rev_nlm) P::rev(&b, &g, &q, &r, rev_nlm, s);
    HIPCHK(c, hipEventRecord(c->aev[2], s));
    P::records(&b, &g, &q, &r, rec_nlm, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->aev[3], s));
    if (N) HIPCHK(c, hipMemcpyAsync(m.h_rec.data(), m.b_rec.p, N * sizeof(phx_orf_margin), hipMemcpyDeviceToHost, s));
    if (P::pinned && N) HIPCHK(c, hipMemcpyAsync(m.h_lost.data(), m.b_lost.p, N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(m.mstat.data(), m.b_mstat.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->aev[4], s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int k = 0; k < 4; k++) m.ms[k] += ev_ms(c->aev[k], c->aev[k + 1]);
    done = true;
    return PHX_OK;
}

// status of contig i's margins after a re-annotation (include/phx.h): the run's for a contig that was not solved again
static int32_t condmargins_status(const phx_ctx *c, int i) {
    const int mode = c->h_qsel[(size_t)i];
    if (!mode) return margins_status(c, i);
    const int32_t r = c->res[(size_t)i].status;
    if (r < 0) return r;
    const int32_t q = c->h_qrec[(size_t)i].status;
    if (q != 0) return q;
    return (re_mode_req(mode) ? c->pm : c->xm).mstat[(size_t)i] ? PHX_S_NEGCYCLE : 0;
}

// the sorted keys of the CDS genes the last re-annotation call returns for contig i (mode: its h_qsel; 0: the run's device list)
static void resolve_keys(const phx_ctx *c, int i, int mode, std::vector<uint64_t> &keys) {
    const DGene *src = resolve_genes(c, i, mode ? &c->h_qrec[(size_t)i] : nullptr, c->h_qgenes);
    const int64_t ng = mode ? (int64_t)c->h_qrec[(size_t)i].n_genes : (int64_t)std::max(c->res[(size_t)i].n_genes, 0);
    keys.clear();
    for (int64_t k = 0; k < ng; k++) if (src[k].frame >= -3 && src[k].frame <= 3) keys.push_back(gene_key(src[k].left, src[k].right, src[k].strand));
    std::sort(keys.begin(), keys.end());
}

// The layout of phx_margins_flat, phx_remargins_flat and phx_pinmargins_flat, behind their ensure_*: offsets and statuses, then the records
// in reference order with `called` set.  again: false for the run's margins (no contig counts as solved again, `called` is against the genes
// phx_download* deliver), else against the genes the re-annotation call returns — the device's lists, no host re-solve enters.  lost: null
// but for phx_pinmargins_flat, else parallel to rec.
static int margins_out(phx_ctx *c, const char *who, bool again, phx_orf_margin *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    try {
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) { offsets[i] = total; status[i] = again ? condmargins_status(c, i) : margins_status(c, i); if (status[i] >= 0) total += c->meta[(size_t)i].n_orf; }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!rec) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    { const int rg = stage_run_genes(c, again ? c->h_qsel.data() : nullptr); if (rg) return rg; } // (of the contigs that were not solved again)
    { const int rg = ensure_grp_host(c); if (rg) return rg; }
    std::vector<uint64_t> keys;
    std::vector<int> order;
    for (int i = 0; i < c->n; i++) {
        if (status[i] < 0) continue;
        const int mode = again ? c->h_qsel[(size_t)i] : 0;
        const bool pinned = re_mode_req(mode);
        if (!again) called_keys(c, i, keys);
        else resolve_keys(c, i, mode, keys);
        // the device's records, in the reference's order
        phx_orf_margin *dst = rec + offsets[i];
        int32_t *ldst = lost ? lost + offsets[i] : nullptr;
        const phx_orf_margin *from = (pinned ? c->pm.h_rec.data() : mode ? c->xm.h_rec.data() : (const phx_orf_margin *)c->h_mrec.p) + c->meta[(size_t)i].orf_off;
        const int32_t *lfrom = pinned ? c->pm.h_lost.data() + c->meta[(size_t)i].orf_off : nullptr;
        each_group_in_reference_order(c, (size_t)i, order, [&](int32_t first, int32_t k) { // (records and `lost` are permuted together)
            if (k > 0) {
                memcpy(dst, from + first, sizeof(phx_orf_margin) * (size_t)k);
                if (ldst && lfrom) memcpy(ldst, lfrom + first, 4 * (size_t)k);
                else if (ldst) memset(ldst, 0, 4 * (size_t)k);
                dst += k;
                if (ldst) ldst += k;
            }
        });
        for (int64_t k = offsets[i]; k < offsets[i + 1]; k++) rec[k].called = is_called(keys, rec[k].left, rec[k].right, rec[k].strand) ? 1 : 0;
    }
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    return PHX_OK;
}

int phx_remargins_flat(phx_ctx *c, phx_orf_margin *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rs = remarg_state(c, "phx_remargins_flat"); if (rs) return rs; } // before any kernel
    { const int rm = ensure_condmargins<CmPlain>(c); if (rm) return rm; }
    return margins_out(c, "phx_remargins_flat", true, rec, nullptr, cap, offsets, status, total_out);
}

int phx_pinmargins_flat(phx_ctx *c, phx_orf_margin *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status)) || (rec && !lost)) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    if (!c->done.reann) { c->err = "phx_pinmargins_flat: no re-annotation of this run (call phx_constrain_flat or phx_curate_flat first)"; return PHX_E_STATE; } // before any kernel
    { const int rm = ensure_condmargins<CmPin>(c); if (rm) return rm; }
    return margins_out(c, "phx_pinmargins_flat", true, rec, lost, cap, offsets, status, total_out);
}

// d_s' / d_t' of a contig to the caller (who has checked the state and `which`), or every node unreached where there is no such vector.  A
// contig solved under the required policy has one word more per node; one that was not solved again has the run's vectors.
static int tap_redist(phx_ctx *c, int32_t contig, int32_t which, uint64_t *dist_limbs, int64_t cap_words) {
    const DMeta &m = c->meta[(size_t)contig];
    const int mode = c->h_qsel[(size_t)contig];
    if (!mode) return which ? phx_tap_dist_target(c, contig, dist_limbs, cap_words) : phx_tap_dist(c, contig, dist_limbs, cap_words); // the run's vectors stand
    const bool pinned = re_mode_req(mode);
    const size_t nl = (size_t)m.sssp_nl + (pinned ? 1 : 0), words = (size_t)m.n_node * nl;
    if (!dist_limbs || cap_words < (int64_t)words) return PHX_E_ARG;
    if (which) { const int rm = pinned ? ensure_condmargins<CmPin>(c) : ensure_condmargins<CmPlain>(c); if (rm) return rm; }
    const phx_ctx::CondMarg &cm = pinned ? c->pm : c->xm;
    const bool have = which ? (cm.h_sel[(size_t)contig] == 1 && !cm.mstat[(size_t)contig]) : c->h_qrec[(size_t)contig].status >= 0;
    if (!have) { // no such vector (the re-solve ended with an error; no path, so no d_t'): every node unreached
        for (size_t v = 0; v < (size_t)m.n_node; v++) for (size_t k = 0; k < nl; k++) dist_limbs[v * nl + k] = k + 1 == nl ? WINF_TOP_HOST : 0;
        return PHX_OK;
    }
    const uint64_t *from = which ? (const uint64_t *)cm.b_dt.p + (size_t)m.node_off * (size_t)(c->n_limbs + (pinned ? 1 : 0)) : (const uint64_t *)c->b_qdist.p + (size_t)m.node_off * (size_t)c->qstride;
    HIPCHK(c, hipMemcpy(dist_limbs, from, words * 8, hipMemcpyDeviceToHost));
    return PHX_OK;
}

int phx_tap_redist(phx_ctx *c, int32_t contig, int32_t which, uint64_t *dist_limbs, int64_t cap_words) {
    TAP_PRE(c, contig);
    (void)m;
    if (which != 0 && which != 1) return PHX_E_ARG;
    { const int rs = remarg_state(c, "phx_tap_redist"); if (rs) return rs; }
    return tap_redist(c, contig, which, dist_limbs, cap_words);
}

int phx_tap_pindist(phx_ctx *c, int32_t contig, int32_t which, uint64_t *dist_limbs, int64_t cap_words, int32_t *words_per_node) {
    TAP_PRE(c, contig);
    if (which != 0 && which != 1) return PHX_E_ARG;
    if (!c->done.reann) { c->err = "phx_tap_pindist: no re-annotation of this run (call phx_constrain_flat or phx_curate_flat first)"; return PHX_E_STATE; }
    if (words_per_node) *words_per_node = m.sssp_nl + (re_mode_req(c->h_qsel[(size_t)contig]) ? 1 : 0);
    return tap_redist(c, contig, which, dist_limbs, cap_words);
}

int phx_remargins_ms(phx_ctx *c, float *ms) { return values_out<4>(c, ms, [](const phx_ctx *x) { return x->xm.ms; }); }
int phx_pinmargins_ms(phx_ctx *c, float *ms) { return values_out<4>(c, ms, [](const phx_ctx *x) { return x->pm.ms; }); }

// ---- re-annotation profiles (phx_profile.inc under MgCond, DESIGN.md §36) ----
// the contigs the conditioned profile kernels cover (pf_on<MgCond>; after ensure_condmargins<CmPlain>): solved again without an error, and
// — where the re-solve found a path — with a conditioned reverse pass that settled
static bool reprofile_contig(const phx_ctx *c, size_t i) {
    if (!c->h_qsel[i]) return false;
    const int32_t sel = c->xm.h_sel[i];
    return sel != 0 && (sel == 2 || !c->xm.mstat[i]);
}
// The slots' records of every contig of the last re-annotation that was solved again into c->rpf.h_rec (at rpf.roff), once per
// re-annotation solve, on top of its margins (the conditioned d_t' and the pass's verdicts) and, when a contig the run's profile covers was
// not solved again, of the run's profile, whose records stand for it.  Reads what the solve and its margins left resident; writes its own
// set only.  (reprofile_pass: the pass itself, for a caller that has checked the state — the pinned profiles run it for the contigs solved
// again without a required ORF beside pinned ones, where remarg_state refuses.)
static int reprofile_pass(phx_ctx *c) {
    if (c->done.reprofile) return PHX_OK;
    { const int rm = ensure_condmargins<CmPlain>(c); if (rm) return rm; }
    const size_t n = (size_t)c->n;
    for (size_t i = 0; i < n; i++)
        if (!c->h_qsel[i] && profile_contig(c, i)) { const int rp = ensure_profile(c); if (rp) return rp; break; }
    phx_ctx::ProfSet &P = c->rpf;
    std::vector<int64_t> off(2 * n + 2, 0); // toff[n], roff[n + 1]
    P.roff.assign(n + 1, 0);
    int nlm = 0;
    int64_t tcells = 0, R = 0;
    for (size_t i = 0; i < n; i++) {
        off[n + i] = R; P.roff[i] = R;
        if (!reprofile_contig(c, i)) continue;
        nlm |= nl_class_bit(c->meta[i].sssp_nl);
        const int ns = c->meta[i].n_node - 1;
        const int64_t cells = profile_cells(ns);
        if (cells > PF_TAB_LDS) { off[i] = tcells; tcells += cells; }
        R += ns;
    }
    off[2 * n] = R; P.roff[n] = R;
    for (float &m : P.ms) m = 0;
    if (nlm) {
        int rc;
        if ((rc = ensure(c, P.b_tab, ((size_t)tcells + 1) * 8))) return rc;
        if ((rc = ensure(c, P.b_off, (2 * n + 2) * 8))) return rc;
        if ((rc = ensure(c, P.b_rec, ((size_t)R + 1) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = ensure_pinned(c, P.h_rec, ((size_t)R + 1) * sizeof(phx_profile_slot), ((size_t)R + (size_t)R / 4 + 1024) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = analysis_events(c))) return rc;
        DBatch b, qb;
        fill_batch(c, &b);
        DMarg g;
        margins_args(c, &g);
        DReann rq;
        reann_batch(c, &qb, &rq);
        DRmarg r;
        condmargins_args(c, c->xm, (size_t)c->tot_edge / 32 + 2, &r);
        DProf q;
        q.gtab = (uint64_t *)P.b_tab.p; q.toff = (const int64_t *)P.b_off.p; q.roff = q.toff + n; q.rec = (phx_profile_slot *)P.b_rec.p;
        hipStream_t s = c->stream;
        HIPCHK(c, hipEventRecord(c->aev[0], s));
        HIPCHK(c, hipMemcpyAsync(P.b_off.p, off.data(), (2 * n + 2) * 8, hipMemcpyHostToDevice, s));
        phxk_reprofile_cand(&b, &g, &rq, &r, &q, nlm, s);
        HIPCHK(c, hipEventRecord(c->aev[1], s));
        phxk_reprofile_rec(&b, &g, &rq, &r, &q, s);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->aev[2], s));
        if (R) HIPCHK(c, hipMemcpyAsync(P.h_rec.p, P.b_rec.p, (size_t)R * sizeof(phx_profile_slot), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->aev[3], s));
        HIPCHK(c, hipStreamSynchronize(s)); // (`off` is read by the copy until here)
        for (int k = 0; k < 3; k++) P.ms[k] = ev_ms(c->aev[k], c->aev[k + 1]);
    } // (else no contig was solved again to a result: nothing is allocated or launched)
    c->done.reprofile = true;
    return PHX_OK;
}
static int ensure_reprofile(phx_ctx *c, const char *who) {
    { const int rs = remarg_state(c, who); if (rs) return rs; } // before any kernel
    return reprofile_pass(c);
}

int phx_reprofile_flat(phx_ctx *c, phx_profile_slot *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rp = ensure_reprofile(c, "phx_reprofile_flat"); if (rp) return rp; }
    auto set_of = [&](int i) -> const phx_ctx::ProfSet * { // the set that holds contig i's records: the run's for a contig that was not solved again
        if (!c->h_qsel[(size_t)i]) return profile_contig(c, (size_t)i) ? &c->pf : nullptr;
        return reprofile_contig(c, (size_t)i) ? &c->rpf : nullptr;
    };
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) { // V - 1 records for every covered contig (status 0 or PHX_S_NOPATH)
        offsets[i] = total;
        status[i] = condmargins_status(c, i);
        const phx_ctx::ProfSet *P = set_of(i);
        if (status[i] >= 0 && P) total += P->roff[(size_t)i + 1] - P->roff[(size_t)i];
    }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!rec) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    for (int i = 0; i < c->n; i++)
        if (offsets[i + 1] > offsets[i]) memcpy(rec + offsets[i], (const phx_profile_slot *)set_of(i)->h_rec.p + set_of(i)->roff[(size_t)i], (size_t)(offsets[i + 1] - offsets[i]) * sizeof(phx_profile_slot));
    return PHX_OK;
}

int phx_reprofile_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->rpf.ms; }); }

// ---- pinned profiles (phx_profile.inc under MgPinProf, DESIGN.md §37) ----
// the contigs the pinned profile kernels cover (pf_on<MgPinProf>; after ensure_condmargins<CmPin>): solved again under the required policy
// without an error, and — where the re-solve found a path — with a pinned reverse pass that settled
static bool pinprofile_contig(const phx_ctx *c, size_t i) {
    if (!re_mode_req(c->h_qsel[i])) return false;
    const int32_t sel = c->pm.h_sel[i];
    return sel != 0 && (sel == 2 || !c->pm.mstat[i]);
}
// The slots' records and `lost` of every contig the last re-annotation solved under the required policy into c->ppf.h_rec / ppf_h_lost (at
// ppf.roff), once per re-annotation solve, on top of the pinned margins (d_t' on one limb more, the pass's verdicts).  The contigs solved
// again without a required ORF get the re-annotation profiles' pass (rpf), the others the run's profile (pf); both stand as they are.  Reads
// what the solve and its margins left resident; writes its own set only.
static int ensure_pinprofile(phx_ctx *c) {
    if (!c->done.reann) { c->err = "phx_pinprofile_flat: no re-annotation of this run (call phx_constrain_flat or phx_curate_flat first)"; return PHX_E_STATE; } // before any kernel
    { const int rm = ensure_condmargins<CmPin>(c); if (rm) return rm; }
    { const int rp = reprofile_pass(c); if (rp) return rp; }
    if (c->done.pinprofile) return PHX_OK;
    const size_t n = (size_t)c->n;
    phx_ctx::ProfSet &P = c->ppf;
    std::vector<int64_t> off(2 * n + 2, 0); // toff[n], roff[n + 1]
    P.roff.assign(n + 1, 0);
    int nlm = 0;
    int64_t tcells = 0, R = 0, covered = 0;
    for (size_t i = 0; i < n; i++) {
        off[n + i] = R; P.roff[i] = R;
        if (!pinprofile_contig(c, i)) continue;
        nlm |= nl_class_bit(c->meta[i].sssp_nl);
        const int ns = c->meta[i].n_node - 1;
        const int64_t cells = profile_cells(ns);
        if (cells > PF_TAB_LDS) { off[i] = tcells; tcells += cells; }
        R += ns;
        covered++;
    }
    off[2 * n] = R; P.roff[n] = R;
    for (float &m : P.ms) m = 0;
    for (int64_t &v : c->ppf_stats) v = 0;
    if (nlm) {
        int rc;
        if ((rc = ensure(c, P.b_tab, ((size_t)tcells + 1) * 8))) return rc;
        if ((rc = ensure(c, P.b_off, (2 * n + 2) * 8))) return rc;
        if ((rc = ensure(c, P.b_rec, ((size_t)R + 1) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = ensure(c, c->ppf_b_lost, (3 * (size_t)R + 1) * 4))) return rc;
        if ((rc = ensure(c, c->ppf_b_rounds, (n + 1) * 4))) return rc;
        if ((rc = ensure_pinned(c, P.h_rec, ((size_t)R + 1) * sizeof(phx_profile_slot), ((size_t)R + (size_t)R / 4 + 1024) * sizeof(phx_profile_slot)))) return rc;
        if ((rc = ensure_pinned(c, c->ppf_h_lost, (3 * (size_t)R + 1) * 4, (3 * ((size_t)R + (size_t)R / 4) + 1024) * 4))) return rc;
        if ((rc = analysis_events(c))) return rc;
        try { c->ppf_h_rounds.assign(n + 1, 0); } catch (const std::bad_alloc &) { c->err = "out of memory in phx_pinprofile_flat"; return PHX_E_NOMEM; }
        DBatch b, qb;
        fill_batch(c, &b);
        DMarg g;
        margins_args(c, &g);
        DReann rq;
        reann_batch(c, &qb, &rq);
        const size_t mw = (size_t)c->tot_edge / 32 + 2;
        DPmarg r;
        condmargins_args(c, c->pm, mw, &r);
        r.dt_stride = b.dist_stride + 1; r.rbit = r.fbit + 2 * mw; r.lost = (int32_t *)c->pm.b_lost.p; // (as ensure_condmargins<CmPin> laid them out)
        DProf q;
        q.gtab = (uint64_t *)P.b_tab.p; q.toff = (const int64_t *)P.b_off.p; q.roff = q.toff + n; q.rec = (phx_profile_slot *)P.b_rec.p;
        hipStream_t s = c->stream;
        HIPCHK(c, hipEventRecord(c->aev[0], s));
        HIPCHK(c, hipMemcpyAsync(P.b_off.p, off.data(), (2 * n + 2) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->ppf_b_rounds.p, 0, (n + 1) * 4, s));
        phxk_pinprofile_cand(&b, &g, &rq, &r, &q, (int32_t *)c->ppf_b_lost.p, (int32_t *)c->ppf_b_rounds.p, nlm, s);
        HIPCHK(c, hipEventRecord(c->aev[1], s));
        phxk_pinprofile_rec(&b, &g, &rq, &r, &q, s);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->aev[2], s));
        if (R) HIPCHK(c, hipMemcpyAsync(P.h_rec.p, P.b_rec.p, (size_t)R * sizeof(phx_profile_slot), hipMemcpyDeviceToHost, s));
        if (R) HIPCHK(c, hipMemcpyAsync(c->ppf_h_lost.p, c->ppf_b_lost.p, 3 * (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(c->ppf_h_rounds.data(), c->ppf_b_rounds.p, n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipEventRecord(c->aev[3], s));
        HIPCHK(c, hipStreamSynchronize(s)); // (`off` is read by the copy until here)
        for (int k = 0; k < 3; k++) P.ms[k] = ev_ms(c->aev[k], c->aev[k + 1]);
        c->ppf_stats[0] = covered;
        for (size_t i = 0; i < n; i++) c->ppf_stats[1] += c->ppf_h_rounds[i];
        const int32_t *hl = (const int32_t *)c->ppf_h_lost.p;
        for (int64_t k = 0; k < R; k++) c->ppf_stats[2] += (hl[3 * k] | hl[3 * k + 1] | hl[3 * k + 2]) != 0; // (lost >= 0)
    } // (else no contig was solved under the required policy to a result: nothing is allocated or launched)
    c->done.pinprofile = true;
    return PHX_OK;
}

int phx_pinprofile_flat(phx_ctx *c, phx_profile_slot *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status)) || (rec && !lost)) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rp = ensure_pinprofile(c); if (rp) return rp; }
    auto set_of = [&](int i) -> const phx_ctx::ProfSet * { // the set that holds contig i's records (phx_reprofile_flat's two, and the pinned set)
        if (!c->h_qsel[(size_t)i]) return profile_contig(c, (size_t)i) ? &c->pf : nullptr;
        if (re_mode_req(c->h_qsel[(size_t)i])) return pinprofile_contig(c, (size_t)i) ? &c->ppf : nullptr;
        return reprofile_contig(c, (size_t)i) ? &c->rpf : nullptr;
    };
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) { // V - 1 records for every covered contig (status 0 or PHX_S_NOPATH)
        offsets[i] = total;
        status[i] = condmargins_status(c, i);
        const phx_ctx::ProfSet *P = set_of(i);
        if (status[i] >= 0 && P) total += P->roff[(size_t)i + 1] - P->roff[(size_t)i];
    }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!rec) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    for (int i = 0; i < c->n; i++) {
        const int64_t k = offsets[i + 1] - offsets[i];
        if (k <= 0) continue;
        const phx_ctx::ProfSet *P = set_of(i);
        memcpy(rec + offsets[i], (const phx_profile_slot *)P->h_rec.p + P->roff[(size_t)i], (size_t)k * sizeof(phx_profile_slot));
        if (P == &c->ppf) memcpy(lost + 3 * offsets[i], (const int32_t *)c->ppf_h_lost.p + 3 * P->roff[(size_t)i], 3 * (size_t)k * 4);
        else memset(lost + 3 * offsets[i], 0, 3 * (size_t)k * 4);
    }
    return PHX_OK;
}

int phx_pinprofile_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->ppf.ms; }); }
int phx_pinprofile_stats(phx_ctx *c, int64_t *out) { return values_out<3>(c, out, [](const phx_ctx *x) { return x->ppf_stats; }); }

// ---- the three families of the drop margins and the drop replacements (DESIGN.md §35) ----
// The run's (§12 / §13: policy DMarg on the run's graph, sets dp / rp), the re-annotation's (§29 / §30: MgDrop, rd / rr — the contigs solved
// again without a required ORF) and the pinned (§32 / §33: MgPinDrop, pd / pr — the contigs solved under the required policy, values on one
// limb more, `lost` beside the records).  The values are the `family` of phxk_drop_step and phxk_repl_step.
enum { FAM_RUN = 0, FAM_RE = 1, FAM_PIN = 2 };
struct FamilySets { // a family's two sets and its flags in RunDone
    phx_ctx::DropSet &D;
    phx_ctx::ReplSet &S;
    bool &drops, &trees, &repl;
};
static FamilySets family_sets(phx_ctx *c, int f) {
    if (f == FAM_RUN) return {c->dp, c->rp, c->done.drops, c->done.trees, c->done.repl};
    if (f == FAM_RE) return {c->rd, c->rr, c->done.redrop, c->done.retrees, c->done.rerepl};
    return {c->pd, c->pr, c->done.pindrop, c->done.pintrees, c->done.pinrepl};
}
// family f's kernels cover contig i (dp_on<G>; after the margins the family builds on: ensure_rev, ensure_condmargins<CmPlain> / <CmPin>)
static bool family_covers(const phx_ctx *c, int f, size_t i) {
    if (f == FAM_RUN) { const DMeta &m = c->meta[i]; return m.status >= 0 && m.n_node > 2 && m.sssp_mode != 4 && !c->mstat[i] && m.n_path >= 3; }
    const phx_ctx::CondMarg &m = f == FAM_PIN ? c->pm : c->xm;
    return (f == FAM_PIN ? re_mode_req(c->h_qsel[i]) : c->h_qsel[i] != 0) && m.h_sel[i] == 1 && !m.mstat[i] && c->h_qrec[i].n_path >= 3;
}
static int family_npath(const phx_ctx *c, int f, size_t i) { return f == FAM_RUN ? c->meta[i].n_path : c->h_qrec[i].n_path; } // contig i's n_path in f
// the family whose sets hold contig i's records, for an entry point of level `top`: a contig that was not solved again keeps the run's.
// (top FAM_RE never meets a pinned contig, whose sets it has not brought up: remarg_state refuses such a solve ahead of every caller — an
// entry point of that level that skips the rule must not come here.)
static int family_of(const phx_ctx *c, int top, size_t i) {
    if (top == FAM_RUN || !c->h_qsel[i]) return FAM_RUN;
    return re_mode_req(c->h_qsel[i]) ? FAM_PIN : FAM_RE;
}
static int32_t family_status(const phx_ctx *c, int f, int i) { return f == FAM_RUN ? margins_status(c, i) : condmargins_status(c, i); } // status of contig i's records in f
// PHX_OK when the context holds a re-annotation the pinned entry points are defined for
static int pin_state(phx_ctx *c, const char *who) {
    if (!c->done.reann) { c->err = std::string(who) + ": no re-annotation of this run (call phx_constrain_flat or phx_curate_flat first)"; return PHX_E_STATE; }
    return PHX_OK;
}

// family f's kernels' view of the run's batch and of what the last re-annotation and its margins left resident (after the margins f builds
// on); v.lost is the launch's to set.  The view points into itself: it is filled in place and not copied.
struct FamilyView {
    DBatch b, qb;
    DMarg g;
    DReann rq;
    DRmarg r;
    DPmarg p;
    DCondView v; // (the run's family: all null)
};
static void cond_view(phx_ctx *c, int f, FamilyView *w) {
    fill_batch(c, &w->b);
    margins_args(c, &w->g);
    w->v = DCondView{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (f == FAM_RUN) return;
    reann_batch(c, &w->qb, &w->rq);
    const size_t mw = (size_t)c->tot_edge / 32 + 2;
    w->v.rq = &w->rq; w->v.qpath = (const int32_t *)c->b_qpath.p;
    if (f == FAM_RE) { condmargins_args(c, c->xm, mw, &w->r); w->v.r = &w->r; return; }
    condmargins_args(c, c->pm, mw, &w->p);
    w->p.dt_stride = w->b.dist_stride + 1; w->p.rbit = w->p.fbit + 2 * mw; w->p.lost = (int32_t *)c->pm.b_lost.p; // (as ensure_condmargins<CmPin> laid them out)
    w->v.p = &w->p;
}

// Family f's drop set, once per run (the run's) or per re-annotation solve, on top of the margins it reads and of the sets the contigs it
// does not cover are laid out from: the run's on ensure_rev; the re-annotation's on its margins (the out-edge bitmaps, d_t' and the pass's
// verdicts) and, when a contig was not solved again, on the run's set; the pinned on the pinned margins and on the re-annotation's set.
// Reads what the solve and its margins left resident; writes only f's own set (trees: with the one-hop trees b_ps / b_ts, for the
// replacements — a set computed without them gets k_dp_tree once more, counting into f's replacement set).  The run's kernels are launched
// for the limb classes of every contig that has device distances, the others for those of the contigs they cover.
static int ensure_dropset(phx_ctx *c, int f, bool trees = false) {
    const FamilySets F = family_sets(c, f);
    if (F.drops && (!trees || F.trees)) return PHX_OK;
    int rc;
    if (f == FAM_RUN) rc = ensure_rev(c);
    else if (f == FAM_RE) { rc = ensure_condmargins<CmPlain>(c); if (!rc && any_unsolved(c)) rc = ensure_dropset(c, FAM_RUN); }
    else { rc = ensure_condmargins<CmPin>(c); if (!rc) rc = ensure_dropset(c, FAM_RE); }
    if (rc) return rc;
    if (f == FAM_PIN) F.D.wide = 1;
    const int run_nlm = f == FAM_RUN ? margins_nl_mask(c) : 0;
    FamilyView w;
    cond_view(c, f, &w);
    hipStream_t s = c->stream;
    return drop_pass(c, F.D, F.S, F.drops, F.trees, trees, [&](size_t i) { return family_covers(c, f, i) ? family_npath(c, f, i) : 0; }, [&](int step, const DDrop &q) {
        w.v.lost = (int32_t *)F.D.b_lost.p; // (the pinned set's, as the pass laid it out; no other set has one)
        phxk_drop_step(f, step, &w.b, &w.g, &w.v, &q, f == FAM_RUN ? run_nlm : F.D.nlm, s);
    });
}

// The layout of phx_drop_margins_flat (top FAM_RUN), phx_redrops_flat (FAM_RE) and phx_pindrops_flat (FAM_PIN), behind their
// ensure_dropset: offsets and statuses, then every contig's CDS records from the set of its family, in path order.  `called` of a contig at
// the run's level is against the genes phx_download* deliver — so ensure_exact and stage_run_genes run when there is such a contig, and only
// then —, of a contig that was solved again against the genes the re-annotation call returns.  lost: null, or parallel to rec (0 outside
// the pinned set).
static int drops_out(phx_ctx *c, const char *who, int top, phx_gene_drop *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    const bool run_level = top == FAM_RUN || any_unsolved(c);
    if (run_level) { const int rx = ensure_exact(c); if (rx) return rx; }
    try {
    int64_t total = 0;
    for (int i = 0; i < c->n; i++) { // records for every contig with status 0
        const int f = family_of(c, top, (size_t)i);
        offsets[i] = total;
        status[i] = family_status(c, f, i);
        if (status[i] != 0 || !family_covers(c, f, (size_t)i)) continue;
        const phx_ctx::DropSet &D = family_sets(c, f).D;
        total += drop_count(D, D.roff[(size_t)i], D.roff[(size_t)i + 1]);
    }
    offsets[c->n] = total;
    if (total_out) *total_out = total;
    if (!rec) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    if (run_level) { const int rg = stage_run_genes(c); if (rg) return rg; }
    std::vector<uint64_t> keys;
    for (int i = 0; i < c->n; i++) {
        if (offsets[i + 1] == offsets[i]) continue;
        const int f = family_of(c, top, (size_t)i);
        if (f == FAM_RUN) called_keys(c, i, keys);
        else resolve_keys(c, i, c->h_qsel[(size_t)i], keys);
        const phx_ctx::DropSet &D = family_sets(c, f).D;
        drop_rows(D, D.roff[(size_t)i], D.roff[(size_t)i + 1], keys, rec + offsets[i], lost ? lost + offsets[i] : nullptr); // (records and `lost` are dropped together)
    }
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    return PHX_OK;
}

int phx_drop_margins_flat(phx_ctx *c, phx_gene_drop *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rx = ensure_exact(c); if (rx) return rx; } // (ahead of the drop kernels here, as ever; drops_out asks again and finds it done)
    { const int rd = ensure_dropset(c, FAM_RUN); if (rd) return rd; }
    return drops_out(c, "phx_drop_margins_flat", FAM_RUN, rec, nullptr, cap, offsets, status, total_out);
}

int phx_redrops_flat(phx_ctx *c, phx_gene_drop *rec, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rs = remarg_state(c, "phx_redrops_flat"); if (rs) return rs; } // before any kernel
    { const int rd = ensure_dropset(c, FAM_RE); if (rd) return rd; }
    return drops_out(c, "phx_redrops_flat", FAM_RE, rec, nullptr, cap, offsets, status, total_out);
}

int phx_pindrops_flat(phx_ctx *c, phx_gene_drop *rec, int32_t *lost, int64_t cap, int64_t *offsets, int32_t *status, int64_t *total_out) {
    if (!c || (c->n > 0 && (!offsets || !status)) || (rec && !lost)) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rs = pin_state(c, "phx_pindrops_flat"); if (rs) return rs; } // before any kernel
    { const int rd = ensure_dropset(c, FAM_PIN); if (rd) return rd; }
    return drops_out(c, "phx_pindrops_flat", FAM_PIN, rec, lost, cap, offsets, status, total_out);
}

int phx_drop_ms(phx_ctx *c, float *ms) { return values_out<4>(c, ms, [](const phx_ctx *x) { return x->dp.ms; }); }
int phx_drop_stats(phx_ctx *c, int64_t *out) { return values_out<4>(c, out, [](const phx_ctx *x) { return x->dp.stats; }); }
int phx_redrops_ms(phx_ctx *c, float *ms) { return values_out<4>(c, ms, [](const phx_ctx *x) { return x->rd.ms; }); }
int phx_redrop_stats(phx_ctx *c, int64_t *out) { return values_out<4>(c, out, [](const phx_ctx *x) { return x->rd.stats; }); }
// device time and counters of the last phx_pindrops_flat over the contigs that were solved again: the pinned pass's, plus §29's for the
// contigs solved again without a required ORF (a batch without a pinned contig: phx_redrops_ms / phx_redrop_stats)
int phx_pindrops_ms(phx_ctx *c, float *ms) {
    float v[4];
    if (c) for (int k = 0; k < 4; k++) v[k] = c->pd.ms[k] + c->rd.ms[k];
    return values_out<4>(c, ms, [&](const phx_ctx *) { return v; });
}
int phx_pindrop_stats(phx_ctx *c, int64_t *out) {
    int64_t v[4];
    if (c) for (int k = 0; k < 4; k++) v[k] = c->pd.stats[k] + c->rd.stats[k];
    return values_out<4>(c, out, [&](const phx_ctx *) { return v; });
}

// Family f's replacement set: every record of its drop set gets its replacement (h_rec / h_genes / h_det at the drop set's roff), once per
// run or per re-annotation solve, on top of ensure_dropset with the one-hop trees and of the replacements of the contigs f does not cover
// (the re-annotation's: the run's when a contig was not solved again; the pinned: the re-annotation's, whose times and counters are then
// this solve's).  Writes f's set and its drop set's b_ps / b_ts only (and the scratch the drop kernels left there: js / jt / gtab).
// k_rp_walk follows DDrop.ps / ts until it meets a path node, so it may run only on trees a k_dp_tree of the same family wrote for this
// solve: the launch below is reached only with the family's `trees` flag set by drop_pass and with both pointers of the DDrop it passes
// non-null — the flag is reset with the family's `drops`, and drop_args gives the pointers for `trees` alone.
static int ensure_replset(phx_ctx *c, int f) {
    static const char *const what[3] = {"drop replacements", "re-annotation replacements", "pinned replacements"};
    static const char *const over[3] = {"drop margins", "re-annotation drop margins", "pinned drop margins"};
    static const char *const who[3] = {"phx_replacements_flat", "phx_rereplacements_flat", "phx_pinreplacements_flat"};
    const FamilySets F = family_sets(c, f);
    if (F.repl) return PHX_OK;
    int rc = ensure_dropset(c, f, true);
    if (!rc && f == FAM_RE && any_unsolved(c)) rc = ensure_replset(c, FAM_RUN);
    if (!rc && f == FAM_PIN) rc = ensure_replset(c, FAM_RE);
    if (rc) return rc;
    for (int k = 0; k < 3; k++) F.S.ms[k] = 0;
    for (int k = 0; k < 5; k++) F.S.stats[k] = 0;
    if (!F.D.nlm) { F.repl = true; return PHX_OK; } // (f covers no contig: nothing is allocated or launched)
    DDrop q;
    drop_args(F.D, true, &q);
    if (!F.drops || !F.trees || !q.ps || !q.ts) { c->err = std::string(what[f]) + ": the " + over[f] + " kept no one-hop trees"; return PHX_E_STATE; }
    const int nlm = f == FAM_RUN ? margins_nl_mask(c) : F.D.nlm;
    FamilyView w;
    cond_view(c, f, &w);
    w.v.lost = (int32_t *)F.D.b_lost.p; // (k_dp_rec's: no kernel here writes it)
    hipStream_t s = c->stream;
    rc = replacement_pass(c, F.S, (size_t)F.D.roff[(size_t)c->n], [&](int step, const DRepl &r) { phxk_repl_step(f, step, &w.b, &w.g, &w.v, &q, &r, nlm, s); }, what[f], who[f]);
    if (rc) return rc;
    F.repl = true;
    return PHX_OK;
}

// The layout of phx_replacements_flat, phx_rereplacements_flat and phx_pinreplacements_flat (top as drops_out's), behind their
// ensure_replset: statuses, offsets, `called` and `lost` exactly as the drop records of the same level have them — one size query and one
// fill of drops_out —, rows and genes from the replacement set of every contig's family.
static int replacements_out(phx_ctx *c, const char *who, int top, phx_gene_repl *rec, int32_t *lost, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets, int32_t *status,
                            int64_t *total_out, int64_t *gene_total_out) {
    int64_t total = 0, gt = 0;
    { const int rd = drops_out(c, who, top, nullptr, nullptr, 0, offsets, status, &total); if (rd) return rd; }
    auto each_contig = [&](auto fn) { // fn(contig, its family's sets) for every contig with records
        for (int i = 0; i < c->n; i++) if (offsets[i + 1] != offsets[i]) fn((size_t)i, family_sets(c, family_of(c, top, (size_t)i)));
    };
    each_contig([&](size_t i, const FamilySets &F) { gt += replacement_genes(F.S, F.D.roff[i], F.D.roff[i + 1]); });
    if (total_out) *total_out = total;
    if (gene_total_out) *gene_total_out = gt;
    if (!rec || !genes) return PHX_OK; // size query
    if (cap < total || gene_cap < gt) return PHX_E_ARG;
    try {
    std::vector<phx_gene_drop> drec((size_t)total + 1);
    { const int rd = drops_out(c, who, top, drec.data(), lost, total, offsets, status, &total); if (rd) return rd; }
    int64_t go = 0;
    each_contig([&](size_t i, const FamilySets &F) { replacement_rows(F.S, F.D.roff[i], F.D.roff[i + 1], drec.data() + offsets[i], rec + offsets[i], genes, &go); });
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    return PHX_OK;
}

int phx_replacements_flat(phx_ctx *c, phx_gene_repl *rec, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets, int32_t *status,
                          int64_t *total_out, int64_t *gene_total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rr = ensure_replset(c, FAM_RUN); if (rr) return rr; }
    return replacements_out(c, "phx_replacements_flat", FAM_RUN, rec, nullptr, cap, genes, gene_cap, offsets, status, total_out, gene_total_out);
}

int phx_rereplacements_flat(phx_ctx *c, phx_gene_repl *rec, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets, int32_t *status,
                            int64_t *total_out, int64_t *gene_total_out) {
    if (!c || (c->n > 0 && (!offsets || !status))) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rs = remarg_state(c, "phx_rereplacements_flat"); if (rs) return rs; } // before any kernel
    { const int rr = ensure_replset(c, FAM_RE); if (rr) return rr; }
    return replacements_out(c, "phx_rereplacements_flat", FAM_RE, rec, nullptr, cap, genes, gene_cap, offsets, status, total_out, gene_total_out);
}

int phx_pinreplacements_flat(phx_ctx *c, phx_gene_repl *rec, int32_t *lost, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets, int32_t *status,
                             int64_t *total_out, int64_t *gene_total_out) {
    if (!c || (c->n > 0 && (!offsets || !status)) || (rec && !lost)) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rs = pin_state(c, "phx_pinreplacements_flat"); if (rs) return rs; } // before any kernel
    { const int rr = ensure_replset(c, FAM_PIN); if (rr) return rr; }
    return replacements_out(c, "phx_pinreplacements_flat", FAM_PIN, rec, lost, cap, genes, gene_cap, offsets, status, total_out, gene_total_out);
}

// The three path taps.  The head they share: the arguments, *n_path = 0 and the run ...
static int replacement_tap_pre(phx_ctx *c, int32_t contig, int32_t k, int32_t *n_path) {
    if (!c || !n_path) return PHX_E_ARG;
    *n_path = 0;
    { const int ra = after_run(c); if (ra) return ra; }
    return contig < 0 || contig >= c->n || k < 0 ? PHX_E_ARG : PHX_OK;
}
// ... and, behind the entry point's state rule, the rest: a contig that was not solved again is the run's tap's (its result stands); any
// other gets the replacements of level `top` and is read from its family's sets, on the re-annotation's path.
static int replacement_path_out(phx_ctx *c, const char *who, int top, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path) {
    const size_t i = (size_t)contig;
    const int f = family_of(c, top, i);
    if (f != top && f == FAM_RUN) return phx_tap_replacement(c, contig, k, path, cap, n_path);
    { const int rr = ensure_replset(c, top); if (rr) return rr; }
    if (!family_covers(c, f, i) || family_status(c, f, contig) != 0) return PHX_E_ARG;
    const FamilySets F = family_sets(c, f);
    const int32_t *dpath = (const int32_t *)(f == FAM_RUN ? c->b_path.p : c->b_qpath.p) + c->meta[i].node_off;
    return replacement_tap(c, F.S, who, contig, F.D.roff[i], F.D.roff[i + 1], k, dpath, family_npath(c, f, i), path, cap, n_path);
}

int phx_tap_replacement(phx_ctx *c, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path) {
    { const int rp = replacement_tap_pre(c, contig, k, n_path); if (rp) return rp; }
    return replacement_path_out(c, "phx_tap_replacement", FAM_RUN, contig, k, path, cap, n_path);
}

int phx_tap_rereplacement(phx_ctx *c, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path) {
    { const int rp = replacement_tap_pre(c, contig, k, n_path); if (rp) return rp; }
    { const int rs = remarg_state(c, "phx_tap_rereplacement"); if (rs) return rs; }
    return replacement_path_out(c, "phx_tap_rereplacement", FAM_RE, contig, k, path, cap, n_path);
}

// (a contig of mode 1 / 3: §30's records in the rr set — phx_tap_rereplacement itself refuses a solve that pinned another contig)
int phx_tap_pinreplacement(phx_ctx *c, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path) {
    { const int rp = replacement_tap_pre(c, contig, k, n_path); if (rp) return rp; }
    { const int rs = pin_state(c, "phx_tap_pinreplacement"); if (rs) return rs; }
    return replacement_path_out(c, "phx_tap_pinreplacement", FAM_PIN, contig, k, path, cap, n_path);
}

int phx_replacements_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->rp.ms; }); }
int phx_replacement_stats(phx_ctx *c, int64_t *out) { return values_out<5>(c, out, [](const phx_ctx *x) { return x->rp.stats; }); }
int phx_rereplacements_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->rr.ms; }); }
int phx_rereplacement_stats(phx_ctx *c, int64_t *out) { return values_out<5>(c, out, [](const phx_ctx *x) { return x->rr.stats; }); }
// device time and counters of the last phx_pinreplacements_flat over the contigs that were solved again: the pinned pass's, plus §30's for the
// contigs solved again without a required ORF (a batch without a pinned contig: phx_rereplacements_ms / phx_rereplacement_stats)
int phx_pinreplacements_ms(phx_ctx *c, float *ms) {
    float v[3];
    if (c) for (int k = 0; k < 3; k++) v[k] = c->pr.ms[k] + c->rr.ms[k];
    return values_out<3>(c, ms, [&](const phx_ctx *) { return v; });
}
int phx_pinreplacement_stats(phx_ctx *c, int64_t *out) {
    int64_t v[5];
    if (c) for (int k = 0; k < 5; k++) v[k] = c->pr.stats[k] + c->rr.stats[k];
    return values_out<5>(c, out, [&](const phx_ctx *) { return v; });
}

// ---- scenario batches (phx_resolve.inc, DESIGN.md §17), with required ORFs (§18), biased ORFs (§20) or both (§27) per scenario ----
// h_srec[j].status before the solve: the scenario gets a slot / its contig is not solved again and the run's verdict stands (neither is a status the device reports)
static const int32_t SC_SLOT = -99, SC_NOSLOT = -100;
// Device bytes of one slot of contig i: distances, parent, path, bitmap slice, window plan, gene records, the record copy; a pinned slot
// (§18) has one limb more per node, a second bitmap slice and its entries of DScen.req0 / nreq / kreq; a biased slot (§20) with n_bias
// listed ORFs has a bias slice, its DScBias and per ORF a triple, a list pair and a staging pair of 16 bytes each; a slot that is both (§27)
// has both parts.
static size_t scen_slot_bytes(const phx_ctx *c, int i, bool pinned = false, size_t n_bias = 0) {
    const DMeta &m = c->meta[(size_t)i];
    const size_t V = (size_t)m.n_node, E = (size_t)m.n_edge;
    return V * ((size_t)m.sssp_nl * 8 + 4 + 4) + (E / 32 + 3) * 4 + (V / 32 + 2) + (V + 1) * sizeof(DGene) + sizeof(DMeta) + sizeof(DScSlot) + sizeof(DReannRec) +
           (pinned ? V * 8 + (E / 32 + 3) * 4 + 16 : 0) + (n_bias ? (E / 32 + 3) * 4 + sizeof(DScBias) + n_bias * 48 : 0);
}

// Solves the scenarios with a slot (h_srec[j].status == SC_SLOT) in chunks under the budget; records into h_srec, genes into h_sgenes.
// perm: per contig named, tap index -> ORF in the contig's device order (-1: no such ORF in the device's groups).  req_off / req_orf: the
// required lists without duplicates; a scenario with a non-empty one gets a pinned slot.  In a chunk's slot table the pinned slots follow
// the plain ones (the slices keep the scenarios' order): the solve's kernels get the table range by range (phxk_scen_solve).  bs_off / bs_orf / bs_val: the
// merged bias lists (no duplicates, no zero, no ORF the scenario refuses); a scenario with a non-empty one gets a biased slot, and the
// biased slots follow the pinned ones.  A scenario with both lists non-empty (phx_curate_scenarios_flat, §27) gets a slot that is pinned AND
// biased — both parts of scen_slot_bytes — in a fourth range directly behind the biased one.
static int scen_compute(phx_ctx *c, int64_t S, const int32_t *scen_contig, const int64_t *scen_off, const int32_t *scen_orf, const int64_t *req_off, const int32_t *req_orf,
                        const int64_t *bs_off, const int32_t *bs_orf, const int64_t *bs_val, const std::vector<std::vector<int32_t>> &perm) {
    int rc;
    hipStream_t s = c->stream;
    c->scen_chunks = 0;
    c->scen_ms[0] = c->scen_ms[1] = c->scen_ms[2] = 0;
    c->h_sgenes.clear();
    c->h_sslot.assign((size_t)S, DScSlot{});
    c->h_schunk_of.assign((size_t)S, 0);
    if ((rc = analysis_events(c))) return rc;
    const int EV0 = 1 << 30;            // a chunk has fewer slots
    std::vector<DScSlot> slots, pslots, eslots, bslots; // plain, pinned, biased, both
    std::vector<int2> pairs, rpairs;    // (a pinned slot's index: -1 - its place among the pinned ones, a biased slot's: EV0 + its place among the biased ones, a "both" slot's: -1 - EV0 - its place among those, until the chunk is closed)
    std::vector<int64_t> which, pwhich, ewhich, bwhich; // scenario of every slot of the chunk
    std::vector<DScBias> ebs, bbs;      // per biased slot, per "both" slot: its DScBias
    std::vector<DScTrip> &trips = c->h_strip; // the chunk's triples and the table's DScBias as uploaded (members: see h_qdforb)
    std::vector<DScBias> &bsv = c->h_sbs;
    std::vector<int64_t> preq0, breq0;  // per pinned slot, per "both" slot: DScen.req0
    std::vector<int32_t> pnreq, bnreq;  //   ... and nreq
    std::vector<uint8_t> &pin = c->h_spin; // what the kernels read per slot: req0 (int64), nreq, kreq (int32)
    for (int64_t j0 = 0; j0 < S;) {
        // ---- the chunk: scenarios j0 .. j1 with a slot, as many as the budget holds (at least one) ----
        slots.clear(); pslots.clear(); pairs.clear(); rpairs.clear(); which.clear(); pwhich.clear(); preq0.clear(); pnreq.clear();
        eslots.clear(); ewhich.clear(); ebs.clear(); trips.clear();
        bslots.clear(); bwhich.clear(); bbs.clear(); breq0.clear(); bnreq.clear();
        size_t bytes = 0, nodes = 0, words = 0, mwords = 0, rwords = 0, bwords = 0, plan = 0;
        int nlm = 0, pinm = 0, evm = 0, bom = 0;
        int64_t j1 = j0;
        for (; j1 < S; j1++) {
            if (c->h_srec[(size_t)j1].status != SC_SLOT) continue;
            const int i = scen_contig[j1];
            const DMeta &m = c->meta[(size_t)i];
            const int32_t nreq = (int32_t)(req_off[j1 + 1] - req_off[j1]);
            const bool pinned = nreq > 0;
            const size_t nbias = (size_t)(bs_off[j1 + 1] - bs_off[j1]);
            const bool biased = nbias > 0, both = pinned && biased;
            const size_t need = scen_slot_bytes(c, i, pinned, nbias);
            const size_t have = slots.size() + pslots.size() + eslots.size() + bslots.size();
            if (have && (bytes + need > (size_t)c->scen_budget || have + 1 >= (size_t)EV0)) break;
            bytes += need;
            DScSlot sl;
            sl.contig = i; sl.pinned = pinned ? 1 : 0;
            sl.node0 = (int64_t)nodes; sl.dist0 = (int64_t)words; sl.mask0 = (int64_t)mwords; sl.plan0 = (int64_t)plan;
            const size_t mw = (((size_t)m.edge_off & 31) + (size_t)m.n_edge) / 32 + 2;
            nodes += (size_t)m.n_node;
            words += ((size_t)m.n_node * (size_t)(m.sssp_nl + (pinned ? 1 : 0)) + 1) & ~(size_t)1;
            mwords += mw;
            plan += (size_t)m.n_node / 32 + 2;
            (both ? bom : pinned ? pinm : biased ? evm : nlm) |= nl_class_bit(m.sssp_nl);
            const int id = both ? -1 - EV0 - (int)bslots.size() : pinned ? -1 - (int)pslots.size() : biased ? EV0 + (int)eslots.size() : (int)slots.size();
            const std::vector<int32_t> &pm = perm[(size_t)i];
            for (int64_t k = scen_off[j1]; k < scen_off[j1 + 1]; k++) {
                const int32_t d = pm[(size_t)scen_orf[k]];
                if (d >= 0) pairs.push_back(make_int2(id, d));
            }
            for (int64_t k = req_off[j1]; k < req_off[j1 + 1]; k++) {
                const int32_t d = pm[(size_t)req_orf[k]];
                if (d >= 0) rpairs.push_back(make_int2(id, d));
            }
            if (pinned) { (both ? breq0 : preq0).push_back((int64_t)rwords); (both ? bnreq : pnreq).push_back(nreq); rwords += mw; }
            if (pinned && !both) { pslots.push_back(sl); pwhich.push_back(j1); }
            else if (biased) {
                DScBias e{};
                e.bbit0 = (int64_t)bwords; e.list0 = (int64_t)trips.size();
                for (int64_t k = bs_off[j1]; k < bs_off[j1 + 1]; k++) {
                    const int32_t d = pm[(size_t)bs_orf[k]];
                    if (d >= 0) trips.push_back(DScTrip{id, d, (long long)bs_val[k]});
                }
                e.n_trip = (int32_t)(trips.size() - (size_t)e.list0);
                bwords += mw;
                if (both) { bbs.push_back(e); bslots.push_back(sl); bwhich.push_back(j1); }
                else { ebs.push_back(e); eslots.push_back(sl); ewhich.push_back(j1); }
            } else { slots.push_back(sl); which.push_back(j1); }
        }
        j0 = j1;
        // the table: plain, pinned, biased, both.  n_pin and n_ev below count the slots WITH a required slice / WITH a list: a "both" slot is either
        const size_t n_plain = slots.size(), n_pin1 = pslots.size(), n_ev1 = eslots.size(), n_bo = bslots.size(), n_head = n_plain + n_pin1, n_first3 = n_head + n_ev1, ns = n_first3 + n_bo;
        const size_t n_pin = n_pin1 + n_bo, n_ev = n_ev1 + n_bo;
        if (!ns) break;
        slots.insert(slots.end(), pslots.begin(), pslots.end());
        slots.insert(slots.end(), eslots.begin(), eslots.end());
        slots.insert(slots.end(), bslots.begin(), bslots.end());
        which.insert(which.end(), pwhich.begin(), pwhich.end());
        which.insert(which.end(), ewhich.begin(), ewhich.end());
        which.insert(which.end(), bwhich.begin(), bwhich.end());
        // a slot's index in the table from its index until the chunk is closed
        auto place = [&](int x) -> int { return x < -EV0 ? (int)n_first3 + (-1 - EV0 - x) : x < 0 ? (int)n_plain + (-1 - x) : x >= EV0 ? (int)n_head + (x - EV0) : x; };
        for (int2 &pr : pairs) pr.x = place(pr.x);
        for (int2 &pr : rpairs) pr.x = place(pr.x);
        for (DScTrip &t : trips) t.slot = place(t.slot);
        int max_list = 0; // the longest list of the chunk: how many workgroups k_sce_sort gives a slot
        for (const DScBias &e : ebs) max_list = std::max(max_list, (int)e.n_trip);
        for (const DScBias &e : bbs) max_list = std::max(max_list, (int)e.n_trip);
        bsv.assign(n_ev ? ns : 0, DScBias{});
        std::copy(ebs.begin(), ebs.end(), bsv.begin() + (ptrdiff_t)(n_ev ? n_head : 0));
        std::copy(bbs.begin(), bbs.end(), bsv.begin() + (ptrdiff_t)(n_ev ? n_first3 : 0));
        pin.assign(ns * 16, 0);
        for (size_t k = 0; k < n_pin1; k++) {
            memcpy(pin.data() + (n_plain + k) * 8, &preq0[k], 8);
            memcpy(pin.data() + ns * 8 + (n_plain + k) * 4, &pnreq[k], 4);
        }
        for (size_t k = 0; k < n_bo; k++) {
            memcpy(pin.data() + (n_first3 + k) * 8, &breq0[k], 8);
            memcpy(pin.data() + ns * 8 + (n_first3 + k) * 4, &bnreq[k], 4);
        }
        c->scen_chunks++;
        if ((rc = ensure(c, c->b_sc_slot, ns * sizeof(DScSlot))) || (rc = ensure(c, c->b_sc_pair, (pairs.size() + rpairs.size() + 1) * sizeof(int2))) ||
            (rc = ensure(c, c->b_sc_meta, ns * sizeof(DMeta))) || (rc = ensure(c, c->b_sc_dist, (words + 2) * 8)) || (rc = ensure(c, c->b_sc_parent, (nodes + 1) * 4)) ||
            (rc = ensure(c, c->b_sc_path, (nodes + 1) * 4)) || (rc = ensure(c, c->b_sc_mask, (mwords + 2 + rwords + 2 + bwords + 2) * 4)) || (rc = ensure(c, c->b_sc_plan, plan + 2)) ||
            (rc = ensure(c, c->b_sc_genes, (nodes + ns + 1) * sizeof(DGene))) || (rc = ensure(c, c->b_sc_rec, ns * sizeof(DReannRec))) ||
            (rc = ensure(c, c->b_sc_tot, sizeof(DTotals))) || (rc = ensure(c, c->b_sc_gtot, 16)) || (n_pin && (rc = ensure(c, c->b_sc_pin, ns * 16))) ||
            (n_ev && ((rc = ensure(c, c->b_sc_bs, ns * sizeof(DScBias))) || (rc = ensure(c, c->b_sc_trip, (trips.size() + 1) * sizeof(DScTrip))) ||
                      (rc = ensure(c, c->b_sc_blist, 2 * (trips.size() + 1) * 16)))))
            return rc;
        if (!c->b_sc_tie.p && (rc = ensure(c, c->b_sc_tie, (size_t)std::max<int64_t>(c->tie_seen, 1 << 20)))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->b_sc_slot.p, slots.data(), ns * sizeof(DScSlot), hipMemcpyHostToDevice, s));
        if (!pairs.empty()) HIPCHK(c, hipMemcpyAsync(c->b_sc_pair.p, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        if (!rpairs.empty()) HIPCHK(c, hipMemcpyAsync((int2 *)c->b_sc_pair.p + pairs.size(), rpairs.data(), rpairs.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        if (n_pin) HIPCHK(c, hipMemcpyAsync(c->b_sc_pin.p, pin.data(), ns * 16, hipMemcpyHostToDevice, s));
        if (!trips.empty()) HIPCHK(c, hipMemcpyAsync(c->b_sc_trip.p, trips.data(), trips.size() * sizeof(DScTrip), hipMemcpyHostToDevice, s));
        c->h_schunk.assign(ns, DReannRec{});
        // the slots' view of the batch: the run's graph and records (read only), totals / genes / counter / tie scratch of the scenarios' own
        DBatch b;
        DScen q;
        const int n_range[4] = {(int)n_plain, (int)n_pin1, (int)n_ev1, (int)n_bo}, nlms[4] = {nlm, pinm, evm, bom}; // the plain head, the pinned and the biased middle and the "both" tail of the slot table
        const size_t base = c->h_sgenes.size();
        const ReSolve R{"scenarios", "slot", c->b_sc_tot, c->b_sc_gtot, c->b_sc_tie, c->b_sc_rec, c->b_sc_genes, c->h_stot, c->h_sgtot, c->h_schunk.data(), ns, nodes + ns, c->h_sgenes};
        float ms[3] = {0, 0, 0};
        rc = resolve_attempts(c, R, ms, [&](int) -> int {
            resolve_batch(c, &b, c->b_sc_tot, c->b_sc_genes, c->b_sc_gtot, c->b_sc_tie);
            q.slot = (const DScSlot *)c->b_sc_slot.p; q.pair = (const int2 *)c->b_sc_pair.p; q.n_pair = (int64_t)pairs.size(); q.n_slot = (int32_t)ns;
            q.stride0 = c->n_limbs; q.meta = (DMeta *)c->b_sc_meta.p; q.dist = (uint64_t *)c->b_sc_dist.p; q.parent = (int32_t *)c->b_sc_parent.p;
            q.path = (int32_t *)c->b_sc_path.p; q.mask = (uint32_t *)c->b_sc_mask.p; q.gplan = (uint8_t *)c->b_sc_plan.p;
            q.dist0 = (const uint64_t *)c->b_dist.p; q.rec = (DReannRec *)c->b_sc_rec.p;
            q.req = nullptr; q.req0 = nullptr; q.nreq = nullptr; q.kreq = nullptr; q.rpair = nullptr; q.n_rpair = 0;
            if (n_pin) {
                q.req = q.mask + (mwords + 2); q.req0 = (const int64_t *)c->b_sc_pin.p; q.nreq = (const int32_t *)((const uint8_t *)c->b_sc_pin.p + ns * 8);
                q.kreq = (int32_t *)((uint8_t *)c->b_sc_pin.p + ns * 12); q.rpair = q.pair + pairs.size(); q.n_rpair = (int64_t)rpairs.size();
            }
            q.bbit = nullptr; q.bs = nullptr; q.blist = nullptr; q.bstage = nullptr; q.trip = nullptr; q.n_trip = 0;
            if (n_ev) {
                q.bbit = q.mask + (mwords + 2 + rwords + 2); q.bs = (DScBias *)c->b_sc_bs.p; q.blist = (long long *)c->b_sc_blist.p;
                q.bstage = q.blist + 2 * (trips.size() + 1); q.trip = (const DScTrip *)c->b_sc_trip.p; q.n_trip = (int64_t)trips.size();
            }
            HIPCHK(c, hipMemsetAsync(c->b_sc_mask.p, 0, (mwords + 2 + (n_pin || n_ev ? rwords + 2 : 0) + (n_ev ? bwords + 2 : 0)) * 4, s));
            if (n_ev) HIPCHK(c, hipMemcpyAsync(c->b_sc_bs.p, bsv.data(), ns * sizeof(DScBias), hipMemcpyHostToDevice, s)); // (counts and sums at zero: k_sce_mask appends again, also on a tie-scratch retry)
            if (n_pin) HIPCHK(c, hipMemsetAsync(q.kreq, 0, ns * 4, s)); // k_scp_mask counts again (also on a tie-scratch retry)
            return PHX_OK;
        }, [&](int step) {
            if (step == 0) phxk_scen_mask(&b, &q, n_range, max_list, s);
            else if (step == 1) phxk_scen_solve(&b, &q, n_range, nlms, s);
            else phxk_scen_finish(&b, &q, n_range, nlms, s);
        });
        if (rc) return rc;
        for (int k = 0; k < 3; k++) c->scen_ms[k] += ms[k];
        for (size_t k = 0; k < ns; k++) {
            DReannRec r = c->h_schunk[k];
            r.gene_off += (int64_t)base;
            c->h_srec[(size_t)which[k]] = r;
            c->h_sslot[(size_t)which[k]] = slots[k];
            c->h_schunk_of[(size_t)which[k]] = c->scen_chunks;
        }
    }
    return PHX_OK;
}

// phx_scenarios_flat (no required lists: require_off, require_orf and unmet null), phx_pinned_scenarios_flat, phx_evidence_scenarios_flat
// (bias lists instead of required ones) and phx_curate_scenarios_flat (all three lists) are one solve on one set of buffers; the cached result is keyed on all the lists (as reann_flat
// serves phx_reannotate_flat, phx_constrain_flat and phx_evidence_flat).
static int scen_flat(phx_ctx *c, const char *who, int64_t n_scen, const int32_t *scen_contig, const int64_t *scen_off, const int32_t *scen_orf, const int64_t *req_off_in,
                     const int32_t *req_orf_in, const int64_t *bias_off_in, const int32_t *bias_orf_in, const int64_t *bias_val_in, const int64_t *orf_offsets, phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status, double *delta, int32_t *unmet,
                     int64_t *total_out) {
    if (!c || n_scen < 0 || !offsets || !scen_off || (n_scen > 0 && (!status || !delta || !scen_contig)) || (c->n > 0 && !orf_offsets)) return PHX_E_ARG;
    { const int ra = after_run(c); if (ra) return ra; }
    { const int rf = fetch_meta(c); if (rf) return rf; }
    try {
    // ---- argument checks, all before any kernel: nothing from the caller indexes device memory unchecked ----
    int64_t acc = 0;
    if (!orf_offsets_ok(c, orf_offsets, &acc)) return PHX_E_ARG;
    const size_t S = (size_t)n_scen;
    for (int pass = 0; pass < 3; pass++) { // the refused lists, then the required ones, then the biased ones
        const int64_t *off = pass == 2 ? bias_off_in : pass ? req_off_in : scen_off;
        const int32_t *orf = pass == 2 ? bias_orf_in : pass ? req_orf_in : scen_orf;
        if (!off) continue;
        if (pass == 2 && off[S] > 0 && !bias_val_in) return PHX_E_ARG;
        if (off[0] != 0) return PHX_E_ARG;
        for (size_t j = 0; j < S; j++) {
            if (off[j + 1] < off[j]) return PHX_E_ARG;
            const int32_t i = scen_contig[j];
            if (i < 0 || i >= c->n) return PHX_E_ARG;
            if (off[j + 1] > off[j] && !orf) return PHX_E_ARG;
            const int64_t cnt = orf_offsets[i + 1] - orf_offsets[i];
            for (int64_t k = off[j]; k < off[j + 1]; k++) if (orf[k] < 0 || (int64_t)orf[k] >= cnt) return PHX_E_ARG;
        }
    }
    // the required lists without duplicates (|R| counts ORFs), and no ORF of a scenario in both of its lists
    std::vector<int64_t> &rq_off = c->h_srq_off;
    std::vector<int32_t> &rq_orf = c->h_srq_orf;
    rq_off.assign(S + 1, 0);
    rq_orf.clear();
    if (req_off_in) {
        std::vector<int32_t> f;
        for (size_t j = 0; j < S; j++) {
            const size_t r0 = rq_orf.size();
            rq_orf.insert(rq_orf.end(), req_orf_in + req_off_in[j], req_orf_in + req_off_in[j + 1]);
            std::sort(rq_orf.begin() + (ptrdiff_t)r0, rq_orf.end());
            rq_orf.erase(std::unique(rq_orf.begin() + (ptrdiff_t)r0, rq_orf.end()), rq_orf.end());
            rq_off[j + 1] = (int64_t)rq_orf.size();
            if (rq_orf.size() == r0 || scen_off[j + 1] == scen_off[j]) continue;
            f.assign(scen_orf + scen_off[j], scen_orf + scen_off[j + 1]);
            std::sort(f.begin(), f.end());
            for (size_t k = r0; k < rq_orf.size(); k++)
                if (std::binary_search(f.begin(), f.end(), rq_orf[k])) { c->err = std::string(who) + ": an ORF is both refused and required in one scenario"; return PHX_E_ARG; } // before any kernel
        }
    }
    // the bias lists merged (§20): per scenario one entry per ORF in ascending order, its B the sum of the ORF's pairs; zero sums and the
    // ORFs the scenario refuses are dropped, so the device never arbitrates
    std::vector<int64_t> &bs_off = c->h_sbs_off, &bs_val = c->h_sbs_val;
    std::vector<int32_t> &bs_orf = c->h_sbs_orf;
    bs_off.assign(S + 1, 0);
    bs_orf.clear(); bs_val.clear();
    if (bias_off_in) {
        std::vector<std::pair<int32_t, int64_t>> pb;
        std::vector<int32_t> f;
        for (size_t j = 0; j < S; j++) {
            pb.clear();
            for (int64_t k = bias_off_in[j]; k < bias_off_in[j + 1]; k++) pb.emplace_back(bias_orf_in[k], bias_val_in[k]);
            std::sort(pb.begin(), pb.end());
            f.assign(scen_orf + scen_off[j], scen_orf + scen_off[j + 1]);
            std::sort(f.begin(), f.end());
            for (size_t k = 0; k < pb.size();) {
                __int128 sum = 0;
                size_t k1 = k;
                for (; k1 < pb.size() && pb[k1].first == pb[k].first; k1++) sum += pb[k1].second;
                if (sum > (__int128)PHX_BIAS_MAX || sum < -(__int128)PHX_BIAS_MAX) { c->err = std::string(who) + ": a bias beyond 2^52"; return PHX_E_ARG; } // before any kernel
                if (sum != 0 && !std::binary_search(f.begin(), f.end(), pb[k].first)) { bs_orf.push_back(pb[k].first); bs_val.push_back((int64_t)sum); }
                k = k1;
            }
            bs_off[j + 1] = (int64_t)bs_orf.size();
        }
    }
    const size_t P = (size_t)scen_off[S];
    const bool same = c->h_skey_boff == bs_off && c->h_skey_borf == bs_orf && c->h_skey_bval == bs_val && c->done.scen && c->h_skey_contig.size() == S && c->h_skey_orf.size() == P &&
                      std::equal(scen_contig, scen_contig + S, c->h_skey_contig.begin()) && std::equal(scen_off, scen_off + S + 1, c->h_skey_off.begin()) &&
                      std::equal(scen_orf, scen_orf + P, c->h_skey_orf.begin()) && c->h_skey_roff == rq_off && c->h_skey_rorf == rq_orf;
    if (!same) {
        c->done.scen = false;
        { const int rg = ensure_grp_host(c); if (rg) return rg; }
        // tap order -> device ORF order of every contig named: the inverse of the permutation phx_margins_flat applies (as reann_compute)
        std::vector<std::vector<int32_t>> perm((size_t)c->n);
        std::vector<int> order;
        DReannRec none{};
        none.status = SC_NOSLOT; none.delta = std::numeric_limits<double>::infinity();
        c->h_srec.assign(S, none);
        for (size_t j = 0; j < S; j++) {
            const int i = scen_contig[j];
            if (!reann_contig(c, i)) continue; // (the run's verdict stands: a run error, no device distances, an empty graph)
            c->h_srec[j].status = SC_SLOT;
            std::vector<int32_t> &pm = perm[(size_t)i];
            if (!pm.empty() || (scen_off[j + 1] == scen_off[j] && rq_off[j + 1] == rq_off[j] && bs_off[j + 1] == bs_off[j])) continue;
            const DMeta &m = c->meta[(size_t)i];
            pm.assign((size_t)m.n_orf, -1);
            size_t t = 0;
            each_group_in_reference_order(c, (size_t)i, order, [&](int32_t first, int32_t k) {
                for (int32_t x = 0; x < k && t + (size_t)x < pm.size(); x++) pm[t + (size_t)x] = first >= 0 && (int64_t)first + k <= m.n_orf ? first + x : -1;
                t += (size_t)(k > 0 ? k : 0);
            });
        }
        { const int rq = scen_compute(c, n_scen, scen_contig, scen_off, scen_orf, rq_off.data(), rq_orf.data(), bs_off.data(), bs_orf.data(), bs_val.data(), perm); if (rq) { (void)hipStreamSynchronize(c->stream); return rq; } }
        c->h_skey_contig.assign(scen_contig, scen_contig + S);
        c->h_skey_off.assign(scen_off, scen_off + S + 1);
        c->h_skey_orf.assign(scen_orf, scen_orf + P);
        c->h_skey_roff = rq_off;
        c->h_skey_rorf = rq_orf;
        c->h_skey_boff = bs_off; c->h_skey_borf = bs_orf; c->h_skey_bval = bs_val;
        c->done.scen = true;
    }
    // ---- the caller's layout: per scenario what phx_reannotate_flat / phx_constrain_flat reports for its contig ----
    auto rec_of = [&](size_t j) { return c->h_srec[j].status != SC_NOSLOT ? &c->h_srec[j] : nullptr; }; // (no slot: the run's result, as the sibling delivers it)
    int64_t total = 0;
    bool run_genes = false;
    for (size_t j = 0; j < S; j++) {
        offsets[j] = total;
        const int64_t k = resolve_entry(c, scen_contig[j], rec_of(j), rq_off[j + 1] - rq_off[j], status + j, delta + j, unmet ? unmet + j : nullptr);
        run_genes = run_genes || (k > 0 && !rec_of(j));
        total += k;
    }
    offsets[S] = total;
    if (total_out) *total_out = total;
    if (!genes) return PHX_OK; // size query
    if (cap < total) return PHX_E_ARG;
    if (run_genes) { const int rg = stage_run_genes(c); if (rg) return rg; }
    for (size_t j = 0; j < S; j++) {
        const int64_t k = offsets[j + 1] - offsets[j];
        if (k <= 0) continue;
        memcpy(genes + offsets[j], resolve_genes(c, scen_contig[j], rec_of(j), c->h_sgenes), sizeof(phx_gene) * (size_t)k);
    }
    } catch (const std::bad_alloc &) { c->err = std::string("out of memory in ") + who; return PHX_E_NOMEM; }
    return PHX_OK;
}

int phx_scenarios_flat(phx_ctx *c, int64_t n_scen, const int32_t *scen_contig, const int64_t *scen_off, const int32_t *scen_orf, const int64_t *orf_offsets,
                       uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status, double *delta, int64_t *total_out) {
    (void)flags; // reserved
    return scen_flat(c, "phx_scenarios_flat", n_scen, scen_contig, scen_off, scen_orf, nullptr, nullptr, nullptr, nullptr, nullptr, orf_offsets, genes, cap, offsets, status, delta, nullptr, total_out);
}

int phx_pinned_scenarios_flat(phx_ctx *c, int64_t n_scen, const int32_t *scen_contig, const int64_t *forbid_off, const int32_t *forbid_orf, const int64_t *require_off,
                              const int32_t *require_orf, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status,
                              double *delta, int32_t *unmet, int64_t *total_out) {
    (void)flags; // reserved
    if (!c || !require_off || (n_scen > 0 && !unmet)) return PHX_E_ARG;
    return scen_flat(c, "phx_pinned_scenarios_flat", n_scen, scen_contig, forbid_off, forbid_orf, require_off, require_orf, nullptr, nullptr, nullptr, orf_offsets, genes, cap, offsets,
                     status, delta, unmet, total_out);
}

int phx_evidence_scenarios_flat(phx_ctx *c, int64_t n_scen, const int32_t *scen_contig, const int64_t *forbid_off, const int32_t *forbid_orf, const int64_t *bias_off,
                                const int32_t *bias_orf, const int64_t *bias_val, const int64_t *orf_offsets, uint32_t flags, phx_gene *genes, int64_t cap, int64_t *offsets,
                                int32_t *status, double *delta, int64_t *total_out) {
    (void)flags; // reserved
    if (!c || !bias_off) return PHX_E_ARG;
    return scen_flat(c, "phx_evidence_scenarios_flat", n_scen, scen_contig, forbid_off, forbid_orf, nullptr, nullptr, bias_off, bias_orf, bias_val, orf_offsets, genes, cap, offsets,
                     status, delta, nullptr, total_out);
}

// (§27) all three lists per scenario: a scenario with a required ORF and a surviving bias takes a "both" slot, any other reduces to its sibling's
int phx_curate_scenarios_flat(phx_ctx *c, int64_t n_scen, const int32_t *scen_contig, const int64_t *forbid_off, const int32_t *forbid_orf, const int64_t *require_off,
                              const int32_t *require_orf, const int64_t *bias_off, const int32_t *bias_orf, const int64_t *bias_val, const int64_t *orf_offsets, uint32_t flags,
                              phx_gene *genes, int64_t cap, int64_t *offsets, int32_t *status, double *delta, int32_t *unmet, int64_t *total_out) {
    (void)flags; // reserved
    if (!c || !require_off || !bias_off || (n_scen > 0 && !unmet)) return PHX_E_ARG;
    return scen_flat(c, "phx_curate_scenarios_flat", n_scen, scen_contig, forbid_off, forbid_orf, require_off, require_orf, bias_off, bias_orf, bias_val, orf_offsets, genes, cap,
                     offsets, status, delta, unmet, total_out);
}

int phx_tap_scenario_path(phx_ctx *c, int64_t scen, int32_t *path, int32_t cap, int32_t *n_path, uint64_t *dist_limbs, int32_t cap_limbs) {
    if (!c || !n_path) return PHX_E_ARG;
    *n_path = 0;
    { const int ra = after_run(c); if (ra) return ra; }
    if (!c->done.scen) return PHX_E_STATE;
    if (scen < 0 || (size_t)scen >= c->h_srec.size()) return PHX_E_ARG;
    const DReannRec &r = c->h_srec[(size_t)scen];
    if (r.status == SC_NOSLOT || r.status < 0 || r.n_path <= 0) return PHX_OK; // no slot, or no path
    if (c->h_schunk_of[(size_t)scen] != c->scen_chunks) return PHX_E_STATE; // its chunk's slices have been reused
    const DScSlot &sl = c->h_sslot[(size_t)scen];
    const DMeta &m = c->meta[(size_t)sl.contig];
    *n_path = r.n_path;
    if (path) {
        if (cap < r.n_path) return PHX_E_ARG;
        HIPCHK(c, hipMemcpy(path, (int32_t *)c->b_sc_path.p + sl.node0, (size_t)r.n_path * 4, hipMemcpyDeviceToHost));
    }
    if (dist_limbs) {
        if (cap_limbs < m.sssp_nl) return PHX_E_ARG;
        // (a pinned slot keeps one limb more per node: the W-sum is the low sssp_nl limbs of its distance, as phx_tap_repath reports it)
        HIPCHK(c, hipMemcpy(dist_limbs, (uint64_t *)c->b_sc_dist.p + sl.dist0 + ((size_t)m.n_node - 1) * (size_t)(m.sssp_nl + (sl.pinned ? 1 : 0)), (size_t)m.sssp_nl * 8, hipMemcpyDeviceToHost));
    }
    return PHX_OK;
}

int phx_scenarios_ms(phx_ctx *c, float *ms) { return values_out<3>(c, ms, [](const phx_ctx *x) { return x->scen_ms; }); }

int64_t phx_scenario_chunks(phx_ctx *c) { return c ? c->scen_chunks : (int64_t)PHX_E_ARG; } // (as phx_plan_timeouts: a NULL context is refused)
