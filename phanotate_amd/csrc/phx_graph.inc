// phx_graph.inc — k_node_*, k_edges*: nodes and in-edge lists (CSR by destination) (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// Nodes: one per ORF start and one per stop-group, sorted by position (then forward before reverse).
// k_orf<true> has set one bit per node in two position bitmaps (forward-strand slot, reverse-strand slot); a node's
// id is its rank = popcounts below it.  k_node_cov marks the bases covered by the longest ORF of every stop-group
// in a third bitmap; k_node_rank turns the per-word popcounts into bases and finds the >500 bp uncovered runs of
// functions.py:320-334; k_node_build lets every ORF / group write its own node; k_node_attr adds other_end and o1/o2.
struct LinkInfo { int time; int val; bool stop; int idx; int far; };
// time = when the reference wrote other_end[pos] for this slot (all ORFs of one group are added by one
// event, so the group's evkey orders the writers); val = what it wrote last; far = index of the group's
// farthest ORF when the slot is a stop node.
__device__ __forceinline__ LinkInfo link_info(uint32_t link, const DOrf *orf, const DGrp *grp) {
    LinkInfo r;
    r.idx = (int)LINK_IDX(link);
    if (LINK_KIND(link) == LINK_START) { r.stop = false; r.far = -1; r.time = grp[orf[r.idx].grp].evkey; r.val = orf[r.idx].stop; }
    else { r.stop = true; const DGrp g = grp[r.idx]; r.far = g.orf_begin + g.n - 1; r.time = g.evkey; r.val = orf[r.far].start; }
    return r;
}

// plane of a tRNA node in DBatch.tbits: forward start, forward stop, reverse start, reverse stop
__device__ __forceinline__ int tnode_plane(int info) { return (NFRAME(info) > 0 ? 0 : 2) + (NTYPE(info) == 1 ? 1 : 0); }

// coverage by the longest ORF of every stop-group (functions.py:321-330), 16 lanes per group, one atomicOr per word
template <int T = NT> // T: threads of the workgroup (the staged kernels: NT; k_graph_chain: its own)
__device__ __forceinline__ void b_node_cov(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0) return;
    const int L = meta->L;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    unsigned long long *cov = (unsigned long long *)(b.nbits + meta->nbits_off) + 6 * (size_t)meta->nw;
    if (b.tnode && by == 0) { // the nodes add_trnas inserts (functions.py:497-508): one bit per node in its (strand, type) plane
        unsigned long long *tb = (unsigned long long *)(b.tbits + meta->nbits_off / 3 * 4);
        const DTNode *tn = b.tnode + meta->tn_off;
        for (int k = threadIdx.x; k < meta->n_tnode; k += T) {
            const int q = tn[k].pos - 1;
            atomicOr(&tb[(size_t)tnode_plane(tn[k].info) * 3 * meta->nw + (q >> 6)], 1ull << (q & 63));
        }
    }
    const int sub = threadIdx.x & 15;
    for (int g = (int)by * (T / 16) + ((int)threadIdx.x >> 4); g < meta->n_grp; g += (int)gy * (T / 16)) {
        const DGrp G = grp[g];
        const DOrf *r = &orf[G.orf_begin + G.n - 1];
        int mi = r->start < r->stop ? r->start : r->stop;
        int ma = r->start > r->stop ? r->start : r->stop;
        if (ma > L - 1) ma = L - 1;
        if (ma <= mi) continue;
        for (int w = (mi >> 6) + sub; w <= ((ma - 1) >> 6); w += 16) atomicOr(&cov[w], range_mask(w, mi, ma - 1)); // bases[n] = n for n in [mi, ma)
    }
}
__global__ __launch_bounds__(NT) void k_node_cov(DBatch b) { b_node_cov(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// per-word node-rank bases, and the bridge events (a covered base more than 500 after the previous covered base)
template <int T = NT>
__device__ __forceinline__ void b_node_rank(const DBatch &b, const int bx) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    __shared__ uint32_t s_scan[T / 64 + 1];
    DMeta *meta = &b.meta[bx];
    const int tid = threadIdx.x;
    if (meta->status < 0) {
        if (tid == 0) { meta->n_node = 0; meta->n_edge = 0; }
        return;
    }
    const int nwp = 3 * meta->nw;
    const uint64_t *nbF = b.nbits + meta->nbits_off, *nbR = nbF + nwp, *cov = nbR + nwp;
    const uint64_t *tb = (b.tnode && meta->n_tnode) ? b.tbits + meta->nbits_off / 3 * 4 : nullptr;
    uint32_t *nbase = b.nbase + meta->nbits_off / 3;
    auto ldcov = [&](int w) -> uint64_t { return __hip_atomic_load(&cov[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }; // written by L2 atomics (k_node_cov): read at L2
    if (tid == 0) meta->n_bridge = 0;
    __syncthreads();
    const int per = (nwp + T - 1) / T;
    const int a = tid * per, e = a + per < nwp ? a + per : nwp;
    uint32_t cnt = 0, lastc = 0; // nodes in my words; last covered base in my words (0 = none; base 0 is never covered)
    for (int w = a; w < e; w++) {
        cnt += (uint32_t)(__popcll(nbF[w]) + __popcll(nbR[w]));
        if (tb) cnt += (uint32_t)(__popcll(tb[w]) + __popcll(tb[nwp + w]) + __popcll(tb[2 * nwp + w]) + __popcll(tb[3 * nwp + w]));
        const uint64_t cw = ldcov(w);
        if (cw) lastc = (uint32_t)(w * 64 + 63 - __clzll((long long)cw));
    }
    uint32_t tot, mtot;
    uint32_t ex = block_excl_scan<T>(cnt, s_scan, &tot);
    uint32_t pm = block_excl_max<T>(lastc, s_scan, &mtot);
    for (int w = a; w < e; w++) {
        nbase[w] = ex;
        ex += (uint32_t)(__popcll(nbF[w]) + __popcll(nbR[w]));
        if (tb) ex += (uint32_t)(__popcll(tb[w]) + __popcll(tb[nwp + w]) + __popcll(tb[2 * nwp + w]) + __popcll(tb[3 * nwp + w]));
        const uint64_t cw = ldcov(w);
        if (cw) {
            const int first = w * 64 + __ffsll((long long)cw) - 1;
            if (first - (int)pm > 500) { // functions.py:334 (gaps inside one 64-base word cannot exceed 500)
                const int k = atomicAdd(&meta->n_bridge, 1);
                if (k < meta->bridge_cap) { DBridge *br = b.bridge + meta->bridge_off; br[k].last = (int)pm; br[k].base = first; }
            }
            pm = (uint32_t)(w * 64 + 63 - __clzll((long long)cw));
        }
    }
    if (tid == 0) {
        const int run = (int)tot, L = meta->L;
        DNode *nd = b.node + meta->node_off;
        double *no = b.no + meta->node_off;
        const double pgap = contig_pstop(meta->gc, L);
        if (run + 2 != meta->n_node) meta->status = PHX_E_STATE; // n_node was sized as n_orf + n_grp + n_tnode + 2
        else {
            nd[run] = DNode{0, NINFO(2, 0), 0u, -1}; no[run] = pgap;             // source, functions.py:440
            nd[run + 1] = DNode{L + 1, NINFO(3, 0), 0u, -1}; no[run + 1] = pgap; // target
        }
    }
    __syncthreads();
    if (tid == 0 && meta->n_bridge > meta->bridge_cap) meta->status = PHX_S_OVERFLOW; // cannot happen: every bridge spans > 500 bases
}
__global__ __launch_bounds__(NT) void k_node_rank(DBatch b) { b_node_rank(b, (int)blockIdx.x); }


// node id of the node at 0-based key position q in the forward (rev = false) or reverse slot
__device__ __forceinline__ int node_rank(const uint64_t *nbF, const uint64_t *nbR, const uint32_t *nbase, int q, bool rev) {
    const int w = q >> 6;
    const uint64_t below = (q & 63) ? (~0ull >> (64 - (q & 63))) : 0ull;
    int id = (int)nbase[w] + __popcll(nbF[w] & below) + __popcll(nbR[w] & below);
    if (rev) id += (int)((nbF[w] >> (q & 63)) & 1ull);
    return id;
}

// the same with tRNA nodes in the graph (tb: their four bitmaps, nwp words each): slot 0 forward CDS node, 1 reverse CDS node,
// 2 + plane for a tRNA node; nodes at one position are ordered by slot
__device__ __forceinline__ int node_rank_t(const uint64_t *nbF, const uint64_t *nbR, const uint32_t *nbase, const uint64_t *tb, int nwp, int q, int slot) {
    const int w = q >> 6, bit = q & 63;
    const uint64_t below = bit ? (~0ull >> (64 - bit)) : 0ull;
    int id = (int)nbase[w] + __popcll(nbF[w] & below) + __popcll(nbR[w] & below);
    if (slot >= 1) id += (int)((nbF[w] >> bit) & 1ull);
    if (slot >= 2) id += (int)((nbR[w] >> bit) & 1ull);
    if (tb) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            id += __popcll(tb[(size_t)k * nwp + w] & below);
            if (slot >= 3 + k) id += (int)((tb[(size_t)k * nwp + w] >> bit) & 1ull);
        }
    }
    return id;
}

// every ORF writes its start node, every stop-group its stop node (functions.py:311-318)
template <int T = NT>
__device__ __forceinline__ void b_node_build(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0 || meta->n_node <= 2) return;
    const int nwp = 3 * meta->nw;
    const uint64_t *nbF = b.nbits + meta->nbits_off, *nbR = nbF + nwp;
    const uint32_t *nbase = b.nbase + meta->nbits_off / 3;
    const uint64_t *tb = (b.tnode && meta->n_tnode) ? b.tbits + meta->nbits_off / 3 * 4 : nullptr;
    const DOrf *orf = b.orf + meta->orf_off;
    int32_t *onode = b.onode + meta->orf_off;
    DGrp *grp = b.grp + meta->grp_off;
    DNode *nd = b.node + meta->node_off;
    const int gtid = (int)by * T + (int)threadIdx.x, gstride = (int)gy * T;
    if (tb) { // the tRNA nodes (not in the close-node bitmaps: the connect rules for them differ, see k_edges)
        const DTNode *tn = b.tnode + meta->tn_off;
        int32_t *tnid = b.tnid + meta->tn_off;
        for (int k = gtid; k < meta->n_tnode; k += gstride) {
            const int id = node_rank_t(nbF, nbR, nbase, tb, nwp, tn[k].pos - 1, 2 + tnode_plane(tn[k].info));
            nd[id] = DNode{tn[k].pos, tn[k].info, LINK_TRNA | (uint32_t)k, tn[k].other};
            tnid[k] = id;
        }
    }
    for (int k = gtid; k < meta->n_orf; k += gstride) {
        const DOrf *r = &orf[k];
        const int id = node_rank_t(nbF, nbR, nbase, tb, nwp, r->start - 1, r->frame < 0 ? 1 : 0);
        nd[id] = DNode{r->start, NINFO(0, r->frame), LINK_START | (uint32_t)k, 0}; // one 16-byte store; other_end follows in k_node_attr
        onode[k] = id;
    }
    for (int g = gtid; g < meta->n_grp; g += gstride) {
        DGrp *G = &grp[g];
        const int id = node_rank_t(nbF, nbR, nbase, tb, nwp, G->stop - 1, G->frame < 0 ? 1 : 0);
        nd[id] = DNode{G->stop, NINFO(1, G->frame), LINK_STOP | (uint32_t)g, 0};
        G->node = id;
    }
}
__global__ __launch_bounds__(NT) void k_node_build(DBatch b) { b_node_build(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// Node order for the edge kernels: the open nodes (targets of connector edges: ~14 in-edges each and ~27 candidates to
// test) first, then the target, then the close nodes (1-2 ORF in-edges), so that a wavefront of k_edges works on nodes of
// one kind instead of idling half its lanes.  One workgroup per contig walks the close-node bitmaps.
template <int T = NT>
__device__ __forceinline__ void b_node_order(const DBatch &b, const int bx) {
    if (b.tot->overflow) return;
    __shared__ uint32_t s_scan[T / 64 + 1];
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0 || meta->n_node < 2) { if (threadIdx.x == 0) meta->n_open = 0; return; }
    const int V = meta->n_node, ncds = V - 2, TGT = V - 1;
    int32_t *olist = b.olist + meta->node_off;
    const int nwd = (ncds + 63) >> 6;
    // the close-node bitmaps over node ids (forward stops, reverse starts; CDS nodes only), one ballot per 64 node records: every word
    // of the contig is written here, so the buffer needs no clearing and k_node_build no atomics
    {
        uint64_t *wF = b.cbits + meta->cb_off, *wR = wF + meta->ncw;
        const DNode *nd = b.node + meta->node_off;
        for (int v0 = 0; v0 < 64 * meta->ncw; v0 += T) {
            const int v = v0 + (int)threadIdx.x;
            bool fs = false, rs = false;
            if (v < ncds) {
                const DNode n = nd[v];
                if (LINK_KIND(n.link) != LINK_TRNA) { fs = NTYPE(n.info) == 1 && NFRAME(n.info) > 0; rs = NTYPE(n.info) == 0 && NFRAME(n.info) < 0; }
            }
            const uint64_t bF = __ballot(fs), bR = __ballot(rs);
            if ((threadIdx.x & 63) == 0 && (v >> 6) < meta->ncw) { wF[v >> 6] = bF; wR[v >> 6] = bR; }
        }
        __syncthreads();
    }
    const uint64_t *cF = b.cbits + meta->cb_off, *cR = cF + meta->ncw;
    const int per = (nwd + T - 1) / T;
    const int a = (int)threadIdx.x * per, e = a + per < nwd ? a + per : nwd;
    uint32_t no_ = 0, nc_ = 0;
    for (int w = a; w < e; w++) {
        const uint64_t valid = range_mask(w, 0, ncds - 1), c = (cF[w] | cR[w]) & valid;
        nc_ += (uint32_t)__popcll(c);
        no_ += (uint32_t)__popcll(~c & valid);
    }
    uint32_t to, tc;
    uint32_t eo = block_excl_scan<T>(no_, s_scan, &to);
    uint32_t ec = block_excl_scan<T>(nc_, s_scan, &tc);
    const int n_open = (int)to + 1; // + the target
    for (int w = a; w < e; w++) {
        const uint64_t valid = range_mask(w, 0, ncds - 1), c = (cF[w] | cR[w]) & valid;
        uint64_t m = ~c & valid;
        while (m) { olist[eo++] = (w << 6) + __ffsll((long long)m) - 1; m &= m - 1; }
        m = c;
        while (m) { olist[n_open + ec++] = (w << 6) + __ffsll((long long)m) - 1; m &= m - 1; }
    }
    if (threadIdx.x == 0) { olist[to] = TGT; meta->n_open = n_open; }
}
__global__ __launch_bounds__(NT) void k_node_order(DBatch b) { b_node_order(b, (int)blockIdx.x); }


// The four node stages of one contig by ONE workgroup (round 5): coverage -> ranks -> records -> order were four launches on the side
// stream beside k_orf_stats (34 + 16 + 53 + 26 us alone, 180 us while sharing the device, with a kernel boundary's tail and start between
// each); a contig's stages only depend on each other, so a workgroup per contig walks them with workgroup barriers and every contig
// proceeds on its own.  (A workgroup's plain stores are write-through and its own CU's later loads see them; the coverage bits arrive
// by L2 atomics, which never touch an L1: k_node_rank reads them with loads that go to L2.)
__global__ __launch_bounds__(NT) void k_nodes_fused(DBatch b) {
    const int bx = blockIdx.x;
    auto stage_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // (NOT agent scope: that writes back the XCD's whole L2, which k_orf_stats is filling beside this kernel — measured: the pair 0.17 -> 0.76 ms)
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    b_node_cov(b, bx, 0, 1);
    stage_sync();
    b_node_rank(b, bx);
    stage_sync();
    b_node_build(b, bx, 0, 1);
    stage_sync();
    b_node_order(b, bx);
}

// other_end[pos] as get_graph sees it (last writer wins, orfs.py:19-30) and WHICH ORF's p_stop is the o1 / o2 term of a node
// (functions.py:373-384): its index, or -1 for pgap.  lmine: the node's link; lother: the link of the CDS node of the other strand at
// the same position (0: none).
__device__ __forceinline__ int o_link(uint32_t lmine, uint32_t lother, const DOrf *orf, const DGrp *grp, int &oe) {
    const LinkInfo a = link_info(lmine, orf, grp);
    oe = a.val;
    int o = -1;
    if (!lother) {
        if (a.stop) o = a.far; // longest ORF of the group
    } else {
        const LinkInfo c = link_info(lother, orf, grp);
        const bool other_wins = c.time > a.time;
        if (other_wins) oe = c.val;
        if (a.stop || c.stop) {
            const LinkInfo sl = a.stop ? a : c; // the slot that makes `l in my_orfs` true
            const LinkInfo st = a.stop ? c : a;
            const DGrp G = grp[sl.idx];
            int hit = -1;
            for (int k = 0; k < G.n; k++)
                if (orf[G.orf_begin + k].start == oe) { hit = G.orf_begin + k; break; }
            if (hit >= 0) o = hit;            // get_orf(other_end[l], l)
            else if (!st.stop) o = st.idx;    // get_orf(l, other_end[l])
        }
    }
    return o;
}
// the link of the CDS node of the other strand at node v's position (its neighbour in the id order: forward first; tRNA nodes follow), 0: none
__device__ __forceinline__ uint32_t other_strand_link(const DNode *nd, int v, int run, const DNode &me) {
    const int fr = NFRAME(me.info);
    if (fr > 0) { if (v + 1 < run && nd[v + 1].pos == me.pos && LINK_KIND(nd[v + 1].link) != LINK_TRNA) return nd[v + 1].link; }
    else { if (v >= 1 && nd[v - 1].pos == me.pos && LINK_KIND(nd[v - 1].link) != LINK_TRNA) return nd[v - 1].link; }
    return 0u;
}

// other_end[pos] (last writer wins, orfs.py:19-30) and WHICH ORF gives the o1/o2 term (functions.py:373-384), thread per node.  Needs the ORF and
// group records only, not their statistics: the term itself (one p_stop per node, read by the filling pass alone) follows in b_node_oterm, so that
// the chain nodes -> attributes -> edge count -> scan never waits for k_orf_stats.
template <int T = NT>
__device__ __forceinline__ void b_node_attr(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0 || meta->n_node <= 2) return;
    const int L = meta->L;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    DNode *nd = b.node + meta->node_off;
    int32_t *olink = b.olink + meta->node_off;
    int32_t *npos = b.npos + meta->node_off;
    const int run = meta->n_node - 2;
    if (by == 0 && threadIdx.x == 0) { npos[run] = 0; npos[run + 1] = L + 1; } // source, target
    const int Vn = meta->n_node;
    uint64_t *ehit0 = b.ehit + meta->node_off;
    for (int v = (int)by * T + (int)threadIdx.x; v < Vn; v += (int)gy * T) ehit0[v] = 0ull; // (only open CDS nodes get verdict bits in k_edges<false>)
    for (int v = (int)by * T + (int)threadIdx.x; v < run; v += (int)gy * T) {
        DNode me = nd[v];
        npos[v] = me.pos;
        const int fr = NFRAME(me.info);
        const uint32_t lmine = me.link;
        if (LINK_KIND(lmine) == LINK_TRNA) { olink[v] = OLINK_NONE; continue; } // its other_end came with the node; the o1/o2 term is unused for tRNA pairs (functions.py:388-399)
        // the node of the other strand at the same position, if any, is my neighbour in the id order (forward first; tRNA nodes follow)
        uint32_t lother = 0;
        if (fr > 0) { if (v + 1 < run && nd[v + 1].pos == me.pos && LINK_KIND(nd[v + 1].link) != LINK_TRNA) lother = nd[v + 1].link; }
        else { if (v >= 1 && nd[v - 1].pos == me.pos && LINK_KIND(nd[v - 1].link) != LINK_TRNA) lother = nd[v - 1].link; }
        int oe;
        const int ok = o_link(lmine, lother, orf, grp, oe);
        me.other = oe;
        nd[v] = me; // whole records: coalesced 16-byte stores
        olink[v] = ok; // (-1: pgap)
    }
}
// the o1/o2 term of every CDS node: p_stop of the ORF b_node_attr named (DBatch.olink), thread per node (the mapping of b_node_attr: k_front calls
// the two in one stage).  Source and target keep the pgap of b_node_rank; tRNA nodes have no term.
__device__ __forceinline__ void b_node_oterm(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return;
    const DMeta *meta = &b.meta[bx];
    if (meta->status < 0 || meta->n_node <= 2) return;
    const DOrfStat *ostat = b.ostat + meta->orf_off;
    const int32_t *olink = b.olink + meta->node_off;
    double *no = b.no + meta->node_off;
    const double pgap = contig_pstop(meta->gc, meta->L);
    const int run = meta->n_node - 2;
    for (int v = (int)by * NT + (int)threadIdx.x; v < run; v += (int)gy * NT) {
        const int ok = olink[v];
        if (ok == OLINK_NONE) continue;
        no[v] = ok < 0 ? pgap : ostat[ok].pstop;
    }
}
__global__ __launch_bounds__(NT) void k_node_oterm(DBatch b) { b_node_oterm(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }
__global__ __launch_bounds__(NT) void k_node_attr(DBatch b) { b_node_attr(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// ------------------------------------------------------------------------------------------------
// Edges, enumerated per destination node (CSR by destination).
// score_gap functions.py:36-46, score_overlap functions.py:26-34.
__device__ __forceinline__ double score_gap(int length, bool diff, double pgap) {
    const double g = 1.0 - pgap;
    if (length > 300) return pow(g, 100.0) + (double)length;
    double s = 1.0 / pow(g, (double)length / 3.0);
    if (diff) s += 20.0;
    return s;
}
__device__ __forceinline__ double score_overlap(int length, bool diff, double pstop) {
    double s = 1.0 / pow(1.0 - pstop, (double)length);
    if (diff) s += 20.0;
    return s;
}

#define OFLAG_BITS(f) (((uint32_t)(f) & 3u) << 30) // DBatch.oflag (bit 0 wide, bit 1 inexact) -> esrc bits 30 (off-path), 31 (inexact)
struct EdgeSink {
    uint32_t *esrc;         // source node | flags (ESRC_F_*)
    unsigned long long *ew; // the encoded integer weight (the tap variant: the bits of the fp64 weight)
    int n;
    bool defer;    // overlap weights are evaluated after the neighbour scan, with every lane busy (node ids must fit 21 bits)
    uint4 *q;      // the workgroup's queue of such edges (LDS): {slot in the contig's edge arrays, source | length << 21 | other strand << 30, pstop}
    uint32_t *qn;  // entries taken (may run past EQ_CAP: those edges were evaluated in place)
    uint32_t row;  // first slot of this node's row, relative to the contig's edge arrays
    double cc;     // CERT_C: scale of the inexact test
};
template <bool FILL>
__device__ __forceinline__ void emit_edge(EdgeSink &s, int src, const EWt &w) {
    if (FILL) {
        if (w.code >= 0) s.esrc[s.n] = ESRC_GAP_WORD(src, w.code); // a gap edge by table code: 4 bytes, no weight
        else { s.esrc[s.n] = (uint32_t)src | w.fl; s.ew[s.n] = w.bits; }
    }
    s.n++;
}
// Overlap edge r -> l: 1/(1-pstop)^length (+20 across strands), functions.py:26-34.  pow() inside the divergent
// neighbour scan would run for the whole wavefront whenever one lane needs it, so the scan only queues
// (slot, source, length, direction, pstop) in LDS and the workgroup evaluates the powers after the scan with every lane
// busy (finish_overlaps), writing source and weight of the slot then.  A full queue: evaluated in place.
#ifndef EQ_CAP
#define EQ_CAP 2048
#endif
template <bool TAPW>
__device__ __forceinline__ void queue_overlap(EdgeSink &s, uint32_t slot, int k, int src, int length, bool diff, double ps) {
    if (slot < EQ_CAP) {
        const unsigned long long pb = (unsigned long long)__double_as_longlong(ps);
        s.q[slot] = make_uint4(s.row + (uint32_t)k, (uint32_t)src | ((uint32_t)length << 21) | (diff ? 0x40000000u : 0u), (uint32_t)pb, (uint32_t)(pb >> 32));
    } else { const EWt w = make_ew<TAPW>(score_overlap(length, diff, ps), s.cc); s.esrc[k] = (uint32_t)src | w.fl; s.ew[k] = w.bits; }
}
template <bool FILL, bool TAPW>
__device__ __forceinline__ void emit_overlap(EdgeSink &s, int src, int length, bool diff, double ps) {
    if (FILL) {
        if (s.defer) queue_overlap<TAPW>(s, atomicAdd(s.qn, 1u), s.n, src, length, diff, ps);
        else { const EWt w = make_ew<TAPW>(score_overlap(length, diff, ps), s.cc); s.esrc[s.n] = (uint32_t)src | w.fl; s.ew[s.n] = w.bits; }
    }
    s.n++;
}
// the queued overlap edges of the workgroup (all threads call it, between the node batches)
template <bool TAPW>
__device__ __forceinline__ void finish_overlaps(uint4 *q, uint32_t *qn, uint32_t *esrc, unsigned long long *ew, double cc) {
    __syncthreads();
    const uint32_t n = *qn < EQ_CAP ? *qn : EQ_CAP;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint4 r = q[i];
        const EWt w = make_ew<TAPW>(score_overlap((int)((r.y >> 21) & 511u), (r.y & 0x40000000u) != 0, __longlong_as_double((long long)(((unsigned long long)r.w << 32) | r.z))), cc);
        esrc[r.x] = (r.y & 0x1fffffu) | w.fl;
        ew[r.x] = w.bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) *qn = 0;
    __syncthreads();
}

// Thread per destination node.  Every connector edge ends in an open node (forward start, reverse stop, target) and
// starts in a close node (forward stop, reverse start) less than 500 bp away, so the candidates of a node are the set
// bits of two node-id bitmaps (close nodes of either strand, written by k_node_order) inside an id range that the
// position-rank structure gives in O(1):
//   * left neighbours (gap edges, functions.py:401-405,417-419,427-433): EVERY close node in the range is an edge
//     (one exception: forward start <- reverse start needs r-l > 2), so the count is a popcount;
//   * right neighbours (overlap edges, functions.py:406-416,423-426,434-438): the other_end tests decide per candidate.
#ifndef EDGE_ABL
#define EDGE_ABL 0 // development (timing only, the graph is wrong): bit 0 no gap edges, bit 1 no overlap edges, bit 2 no ORF edges — in both passes
#endif
#ifndef EDGE_RANKS
#define EDGE_RANKS 1 // the filling pass takes the id ranges of a node's two neighbour scans from the counting pass (DBatch.erank) instead of ranking again
#endif
#ifndef EDGE_WPS
#define EDGE_WPS 4 // wavefronts per SIMD the register allocation must allow
#endif
// TAPW (with FILL): the tap variant — the same rows once more, with the fp64 weights themselves and plain source nodes, into
// DBatch.ewf / esrcf (phx_tap_edges; the run keeps integers only).
// CODED (with FILL, not TAPW): gap edges may go out in the 4-byte coded form (ESRC_F_GAP; DBatch.gap_code says whether they do in this batch);
// without it the kernel is the plain-row kernel of rounds 2-5, instruction for instruction.
// T: threads of the workgroup.  INWG: the stages in front ran in this very launch (k_graph_chain): what they left by L2 atomics is read at L2.
// A value every lane holds alike, moved to scalar registers.  Behind stores of the same launch (k_graph_chain) the compiler reads a contig's record with
// vector loads and keeps every offset and pointer made of it once per LANE: the counting pass then holds twenty pointers in forty VGPRs and spills.
// ON = false (the staged kernels, whose loads of the record are scalar anyway): the value as it is.
template <bool ON, class V>
__device__ __forceinline__ V wg_uniform(V x) {
    if constexpr (!ON) return x;
    else if constexpr (sizeof(V) == 4) {
        int w;
        __builtin_memcpy(&w, &x, 4);
        w = __builtin_amdgcn_readfirstlane(w);
        __builtin_memcpy(&x, &w, 4);
        return x;
    } else {
        static_assert(sizeof(V) == 8, "32- or 64-bit values");
        int w[2];
        __builtin_memcpy(w, &x, 8);
        w[0] = __builtin_amdgcn_readfirstlane(w[0]);
        w[1] = __builtin_amdgcn_readfirstlane(w[1]);
        __builtin_memcpy(&x, w, 8);
        return x;
    }
}
template <bool FILL, bool TAPW, bool CODED = false, int T = NT, bool INWG = false>
__device__ __forceinline__ void b_edges(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    DMeta *meta = &b.meta[bx];
    auto U = [](auto x) { return wg_uniform<INWG>(x); }; // (the contig's record: see wg_uniform)
    if (U(meta->status) < 0 || U(meta->n_node) <= 0) return;
    const int L = U(meta->L);
    const int V = U(meta->n_node), ncds = V - 2, SRC = V - 2, TGT = V - 1;
    const DOrf *orf = b.orf + U(meta->orf_off);
    const int32_t *onode = b.onode + U(meta->orf_off);
    const double *oweight = b.oweight + U(meta->orf_off);
    const long long *owi = b.owi + U(meta->orf_off);
    const uint8_t *oflag = b.oflag + U(meta->orf_off);
    const double cc = CERT_C(b);
    const DGrp *grp = b.grp + U(meta->grp_off);
    const DNode *nd = b.node + U(meta->node_off);
    const double *no = b.no + U(meta->node_off);
    const int32_t *npos = b.npos + U(meta->node_off);
    uint32_t *in_off = b.in_off + U(meta->node_off) + bx; // V+1 entries per contig
    uint64_t *ehit = b.ehit + U(meta->node_off);                   // per open node: which of its first 64 overlap candidates are edges
    const int nwp = 3 * U(meta->nw);
    const uint64_t *nbF = b.nbits + U(meta->nbits_off), *nbR = nbF + nwp;
    const uint32_t *nbase = b.nbase + U(meta->nbits_off) / 3;
    const uint64_t *tb = (b.tnode && U(meta->n_tnode)) ? b.tbits + U(meta->nbits_off) / 3 * 4 : nullptr;
    const int ntn = tb ? U(meta->n_tnode) : 0;
    const DTNode *tn = tb ? b.tnode + U(meta->tn_off) : nullptr;
    const int32_t *tnid = tb ? b.tnid + U(meta->tn_off) : nullptr;
    const uint64_t *cF = b.cbits + U(meta->cb_off), *cR = cF + U(meta->ncw); // close nodes by node id: forward stops / reverse starts (CDS only)
    const double pgap = contig_pstop(U(meta->gc), L);
    const int nbr = INWG ? U(__hip_atomic_load(&meta->n_bridge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : meta->n_bridge; // (k_node_rank counts them by atomicAdd)
    const DBridge *bridges = b.bridge + U(meta->bridge_off);
    bool parallel = false, dense = false, mr_partial = false;
    // score_gap depends only on (length, direction): tabulated once per workgroup, as the record the edge arrays take (encoded
    // integer + inexact flag), instead of one pow and one conversion per gap edge: same strand for length -2..497 (beyond 300 it
    // is (1-pgap)^100 + length, functions.py:40-41, without the 'diff' penalty), across strands (+20) for length -2..300
    constexpr int GAPN = 500, GAPD = 303;
    __shared__ unsigned long long s_gap[FILL ? GAPN + GAPD : 1];
    __shared__ uint16_t s_gapf[FILL ? GAPN + GAPD : 1]; // per entry the high part of the source word, >> 19: flags (bits 11-12 <- 30-31) | coded (bit 10 <- ESRC_F_GAP) | code (bits 0-9)
    __shared__ double s_g100;
    __shared__ uint4 s_q[FILL ? EQ_CAP : 1];
    __shared__ uint32_t s_qn, s_anyf;
    if (FILL && threadIdx.x == 0) { s_qn = 0; s_anyf = 0; }
    if (FILL && !TAPW) { // the contig's table, made by k_edges_scan
        __syncthreads();
        const long long *gt = b.gtab + (size_t)bx * GT_N;
        const uint16_t *gf = b.gtabf + (size_t)bx * GT_N;
        for (int i = threadIdx.x; i < GAPN + GAPD; i += T) { s_gap[i] = (unsigned long long)gt[i]; s_gapf[i] = gf[i]; }
        if (threadIdx.x == 0) { s_g100 = __longlong_as_double(gt[GT_N - 1]); s_anyf = (uint32_t)gt[GT_N - 2]; }
        __syncthreads();
    } else if (FILL) { // the tap variant: the fp64 weights themselves
        __syncthreads();
        const double g100 = pow(1.0 - pgap, 100.0);
        for (int i = threadIdx.x; i < GAPN + GAPD; i += T) {
            const int length = (i < GAPN ? i : i - GAPN) - 2;
            double w = length > 300 ? g100 + (double)length : 1.0 / pow(1.0 - pgap, (double)length / 3.0);
            if (i >= GAPN) w += 20.0;
            const EWt e = make_ew<TAPW>(w, cc);
            s_gap[i] = e.bits;
            s_gapf[i] = 0; // (make_ew<true> never flags)
        }
        if (threadIdx.x == 0) s_g100 = g100;
        __syncthreads();
    }
    static_assert(GAPN == GT_SAME && GAPD == GT_DIFF && GAPN + GAPD <= GT_N && GAPN + GAPD <= 1024, "the gap table as the consumers index it");
    const bool gap_coded = CODED && FILL && !TAPW && b.gap_code && 2 * (int64_t)L + 2 <= ESRC_GAP_NODES; // (as b_gap_table decides)
    auto gap = [&](int length, bool diff) -> EWt {
        EWt r; r.bits = 0; r.fl = 0; r.code = -1;
        if (!FILL) return r;
        if (length > GAPN - 3) return make_ew<TAPW>(s_g100 + (double)length, cc); // terminal edges and bridges: up to 2000 bp
        const int i = (diff && length <= 300) ? GAPN + length + 2 : length + 2;
        r.bits = s_gap[i];
        if (CODED) { const uint32_t h = s_gapf[i]; r.fl = (h >> 11) << 30; if (h & (1u << 10)) r.code = i; }
        else if (s_anyf) r.fl = (uint32_t)(s_gapf[i] >> 11) << 30; // (uniform: the flag table is only read when it holds a flag at all)
        return r;
    };
    const EWt trna_w = make_ew<TAPW>(-20.0, cc);
    // number of nodes whose 1-based position is < p1  (= id of the first node at position >= p1)
    auto rank_lt = [&](int p1) -> int {
        if (p1 <= 1) return 0;
        if (p1 > L) return ncds;
        return node_rank_t(nbF, nbR, nbase, tb, nwp, p1 - 1, 0);
    };
    // tRNA masking, functions.py:388-399: a pair with a tRNA node on either side gets one kind of edge only: left close node
    // (forward stop / reverse start) -> right open node (forward start / reverse stop), 0 < r-l < 500, score_gap(r-l-3, 'same')
    // on both strand combinations; no overlap edges.  The few tRNA nodes of a contig are scanned as a list.
    auto t_close = [&](int k) { const int i = tn[k].info; return (NTYPE(i) == 1 && NFRAME(i) > 0) || (NTYPE(i) == 0 && NFRAME(i) < 0); };
    const int32_t *olist = b.olist + U(meta->node_off); // open nodes, target, close nodes (k_node_order); the source has no in-edge
    if (!FILL && by == 0 && threadIdx.x == 0) in_off[SRC] = 0u;
    // (DBatch.orf_rows: the close CDS nodes — the tail of the list — get their rows from k_edges_orf, a thread per ORF)
    const int n_list = (FILL && !TAPW && b.orf_rows) ? U(meta->n_open) : V - 1;
    for (int base = (int)by * T; base < n_list; base += (int)gy * T) {
        const int li = base + (int)threadIdx.x;
        const int v = li < n_list ? olist[li] : V;
        EdgeSink sink;
        sink.n = 0;
        sink.defer = b.defer_overlap != 0;
        sink.q = s_q; sink.qn = &s_qn; sink.row = 0; sink.cc = cc;
        if (FILL && v < V) {
            sink.row = in_off[v];
            sink.esrc = (TAPW ? b.esrcf : b.esrc) + U(meta->edge_off) + sink.row;
            sink.ew = (TAPW ? (unsigned long long *)b.ewf : (unsigned long long *)b.ew) + U(meta->edge_off) + sink.row;
        }
        if (v < V && v != SRC) {
            if (v == TGT) {
                // functions.py:449-452: every close node with L - pos <= 2000
                const int a = rank_lt(L - 2000);
                for (int w = a >> 6; w <= (ncds - 1) >> 6 && ncds > 0; w++) {
                    uint64_t m = (cF[w] | cR[w]) & range_mask(w, a, ncds - 1);
                    if (!FILL) sink.n += __popcll(m);
                    else
                        while (m) { const int u = (w << 6) + __ffsll((long long)m) - 1; m &= m - 1; emit_edge<FILL>(sink, u, gap(L - npos[u], false)); }
                }
                for (int k = 0; k < ntn; k++)
                    if (t_close(k) && L - tn[k].pos <= 2000) emit_edge<FILL>(sink, FILL ? tnid[k] : 0, gap(L - tn[k].pos, false));
            } else {
                const int iv = nd[v].info;
                const int t = NTYPE(iv), f = NFRAME(iv), pos = nd[v].pos;
                const bool open = (t == 0 && f > 0) || (t == 1 && f < 0);
                if (LINK_KIND(nd[v].link) == LINK_TRNA) {
                    if (!open) { // the tRNA edge(s) that end here: weight -20 (functions.py:509)
                        const DTEdge *te = b.tedge + U(meta->te_off);
                        for (int k = 0; k < U(meta->n_tedge); k++)
                            if (tnid[te[k].dst] == v) emit_edge<FILL>(sink, tnid[te[k].src], trna_w);
                    } else {
                        if (pos <= 2000) { EWt w0 = gap(pos, false); w0.fl |= ESRC_F_OFFPATH; w0.code = -1; emit_edge<FILL>(sink, SRC, w0); } // functions.py:445-448 (explicit: the flag says it leaves the source node)
                        const int a = rank_lt(pos - 499), e = rank_lt(pos) - 1; // every close CDS node to the left, 0 < r-l < 500
                        for (int w = e >> 6; e >= a && w >= (a >> 6); w--) {
                            uint64_t m = (cF[w] | cR[w]) & range_mask(w, a, e);
                            if (!FILL) sink.n += __popcll(m);
                            else
                                while (m) { const int j = 63 - __clzll((long long)m); m &= ~(1ull << j); const int u = (w << 6) + j; emit_edge<FILL>(sink, u, gap(pos - npos[u] - 3, false)); }
                        }
                        for (int k = 0; k < ntn; k++)
                            if (t_close(k) && pos - tn[k].pos > 0 && pos - tn[k].pos < 500) emit_edge<FILL>(sink, FILL ? tnid[k] : 0, gap(pos - tn[k].pos - 3, false));
                    }
                } else if (!open) {
                    // ORF edges, functions.py:311-318
                    if (EDGE_ABL & 4) { }
                    else if (t == 1) { // forward stop: one edge per start of the group
                        const DGrp G = grp[LINK_IDX(nd[v].link)];
                        if (!FILL) sink.n += G.n;
                        else {
                            auto orf_w = [&](int i) { EWt r; if (TAPW) { r.bits = (unsigned long long)__double_as_longlong(oweight[i]); r.fl = 0u; } else { r.bits = (unsigned long long)owi[i]; r.fl = OFLAG_BITS(oflag[i]); } return r; };
                            int k = 0;
                            for (; k + 4 <= G.n; k += 4) { // the group's start nodes and weights are consecutive: four slots per copy
                                uint4 us; unsigned long long wt[4]; uint32_t fl = 0;
                                __builtin_memcpy(&us, onode + G.orf_begin + k, 16);
                                __builtin_memcpy(wt, TAPW ? (const void *)(oweight + G.orf_begin + k) : (const void *)(owi + G.orf_begin + k), 32);
                                if (!TAPW) { __builtin_memcpy(&fl, oflag + G.orf_begin + k, 4); us.x |= OFLAG_BITS(fl); us.y |= OFLAG_BITS(fl >> 8); us.z |= OFLAG_BITS(fl >> 16); us.w |= OFLAG_BITS(fl >> 24); }
                                __builtin_memcpy(sink.esrc + sink.n, &us, 16);
                                __builtin_memcpy(sink.ew + sink.n, wt, 32);
                                sink.n += 4;
                            }
                            for (; k < G.n; k++) emit_edge<FILL>(sink, onode[G.orf_begin + k], orf_w(G.orf_begin + k));
                        }
                    } else { // reverse start: from the group's stop node
                        const uint32_t k = LINK_IDX(nd[v].link);
                        EWt w; w.bits = 0; w.fl = 0;
                        if (FILL) { if (TAPW) w.bits = (unsigned long long)__double_as_longlong(oweight[k]); else { w.bits = (unsigned long long)owi[k]; w.fl = OFLAG_BITS(oflag[k]); } }
                        emit_edge<FILL>(sink, FILL ? grp[orf[k].grp].node : 0, w);
                    }
                } else {
                    if (pos <= 2000) { EWt w0 = gap(pos, false); w0.fl |= ESRC_F_OFFPATH; w0.code = -1; emit_edge<FILL>(sink, SRC, w0); } // functions.py:445-448 (explicit: the flag says it leaves the source node)
                    for (int k = 0; k < ntn; k++) // close tRNA nodes to the left
                        if (t_close(k) && pos - tn[k].pos > 0 && pos - tn[k].pos < 500) emit_edge<FILL>(sink, FILL ? tnid[k] : 0, gap(pos - tn[k].pos - 3, false));
                    // ---- v as right node: gap edges from every close node l with 0 < r-l < 500 ----
                    int4 rk = make_int4(0, 0, 0, 0);
                    if (EDGE_RANKS && FILL && !TAPW) rk = b.erank[U(meta->node_off) + v];
                    if (!(EDGE_ABL & 1)) {
                        const int a = (EDGE_RANKS && FILL && !TAPW) ? rk.x : rank_lt(pos - 499), e = (EDGE_RANKS && FILL && !TAPW) ? rk.y : rank_lt(pos) - 1; // ids [a, e]
                        if (EDGE_RANKS && !FILL) { rk.x = a; rk.y = e; }
                        // same strand as v: forward stop -> forward start, reverse start -> reverse stop; other strand: +20
                        const uint64_t *same = t == 0 ? cF : cR, *diff = t == 0 ? cR : cF;
                        for (int w = e >> 6; e >= a && w >= (a >> 6); w--) {
                            const uint64_t rm = range_mask(w, a, e);
                            uint64_t ms = same[w] & rm, md = diff[w] & rm;
                            if (!FILL) {
                                sink.n += __popcll(ms) + __popcll(md);
                                if (t == 0) // forward start <- reverse start needs r-l > 2 (functions.py:431): look at the nearest ones only
                                    while (md) { const int j = 63 - __clzll((long long)md); md &= ~(1ull << j); if (pos - npos[(w << 6) + j] > 2) break; sink.n--; }
                            } else {
                                uint64_t m = ms | md;
                                while (m) { // descending ids = nearest first; four candidates per step: their positions are fetched together
                                    int jj[4], pp[4], cnt = 0;
#pragma unroll
                                    for (int g = 0; g < 4; g++) {
                                        jj[g] = g ? jj[g - 1] : 0;
                                        if (m) { jj[g] = 63 - __clzll((long long)m); m &= ~(1ull << jj[g]); cnt = g + 1; }
                                    }
#pragma unroll
                                    for (int g = 0; g < 4; g++) pp[g] = npos[(w << 6) + jj[g]];
                                    bool keep[4];
                                    if (CODED && gap_coded) { // the coded form: the high part of the source word by table index (0 < d < 500: always a table entry), no weights
                                        uint32_t hw[4]; int gi[4];
#pragma unroll
                                        for (int g = 0; g < 4; g++) {
                                            const int d = pos - pp[g];
                                            const bool isd = (md >> jj[g]) & 1ull;
                                            keep[g] = g < cnt && !(isd && t == 0 && d <= 2);
                                            gi[g] = (isd && d <= 303) ? GAPN + d - 1 : d - 1; // (length = d - 3; index = length + 2)
                                            hw[g] = ((uint32_t)s_gapf[gi[g]] << 19) | (uint32_t)((w << 6) + jj[g]);
                                        }
                                        if (keep[0] && keep[1] && keep[2] && keep[3]) {
                                            const uint4 us = make_uint4(hw[0], hw[1], hw[2], hw[3]);
                                            __builtin_memcpy(sink.esrc + sink.n, &us, 16);
                                            if (!(hw[0] & hw[1] & hw[2] & hw[3] & ESRC_F_GAP)) { // (a flagged table entry among them: nearly never)
#pragma unroll
                                                for (int g = 0; g < 4; g++) if (!(hw[g] & ESRC_F_GAP)) sink.ew[sink.n + g] = s_gap[gi[g]];
                                            }
                                            sink.n += 4;
                                        } else {
#pragma unroll
                                            for (int g = 0; g < 4; g++)
                                                if (keep[g]) { sink.esrc[sink.n] = hw[g]; if (!(hw[g] & ESRC_F_GAP)) sink.ew[sink.n] = s_gap[gi[g]]; sink.n++; }
                                        }
                                        continue;
                                    }
                                    EWt wt[4];
#pragma unroll
                                    for (int g = 0; g < 4; g++) {
                                        const int d = pos - pp[g];
                                        const bool isd = (md >> jj[g]) & 1ull;
                                        keep[g] = g < cnt && !(isd && t == 0 && d <= 2);
                                        wt[g] = gap(d - 3, isd);
                                    }
                                    if (keep[0] && keep[1] && keep[2] && keep[3]) { // four slots of the row with one store for the sources (round 6: coded gap edges have no weights to store)
                                        const uint4 us = make_uint4((uint32_t)((w << 6) + jj[0]) | wt[0].fl, (uint32_t)((w << 6) + jj[1]) | wt[1].fl, (uint32_t)((w << 6) + jj[2]) | wt[2].fl, (uint32_t)((w << 6) + jj[3]) | wt[3].fl);
                                        const unsigned long long wb[4] = {wt[0].bits, wt[1].bits, wt[2].bits, wt[3].bits};
                                        __builtin_memcpy(sink.esrc + sink.n, &us, 16);
                                        __builtin_memcpy(sink.ew + sink.n, wb, 32);
                                        sink.n += 4;
                                    } else {
#pragma unroll
                                        for (int g = 0; g < 4; g++)
                                            if (keep[g]) emit_edge<FILL>(sink, (w << 6) + jj[g], wt[g]);
                                    }
                                }
                            }
                        }
                    }
                    // ---- v as left node: overlap edges from close nodes r with 0 < r-l < 500 that pass the other_end tests ----
                    // The counting pass keeps the verdicts of the first 64 candidates as a bit mask per node (ehit); the
                    // filling pass then visits only the hits and never loads the records of the ~75 % that fail.
                    if (!(EDGE_ABL & 2)) {
                        const int my_other = nd[v].other;
                        const double my_o = FILL ? no[v] : 0.0;
                        // every test below asks for r < my other end: the candidates end there (for half the nodes well before 500 bp)
                        const bool have = EDGE_RANKS && FILL && !TAPW;
                        const int a = have ? rk.z : rank_lt(pos + 1), e500 = FILL ? 0 : rank_lt(pos + 500) - 1;
                        const int e = have ? rk.w : (my_other < pos + 500 ? (my_other > pos + 1 ? rank_lt(my_other) - 1 : a - 1) : (FILL ? rank_lt(pos + 500) - 1 : e500)); // ids [a, e]
                        if (EDGE_RANKS && !FILL) { rk.z = a; rk.w = e; b.erank[U(meta->node_off) + v] = rk; }
                        uint64_t hm = FILL ? ehit[v] : 0ull;
                        int n_close_ahead = 0;
                        if (!FILL)
                            for (int w = a >> 6; e500 >= a && w <= (e500 >> 6); w++) n_close_ahead += __popcll((cF[w] | cR[w]) & range_mask(w, a, e500));
                        for (int w = a >> 6; e >= a && w <= (e >> 6); w++) {
                            const uint64_t wF = cF[w], wR = cR[w];
                            uint64_t m = (wF | wR) & range_mask(w, a, e);
                            const int off = (w << 6) - a; // candidate index (relative to a) of bit 0 of this word
                            if (FILL) { // cached verdicts for candidate indices 0..63
                                const uint64_t cached = w > ((a + 63) >> 6) ? 0ull : range_mask(w, a, a + 63); // range_mask only clips the first / last word
                                const uint64_t hw = off <= -64 || off >= 64 ? 0ull : (off < 0 ? hm << (-off) : hm >> off);
                                uint64_t mh = m & cached & hw;
                                m &= ~cached;
                                while (mh) { // four hits per step: their positions and o-terms are fetched together
                                    int jj[4], pp[4], cnt = 0;
                                    double oo[4];
#pragma unroll
                                    for (int g = 0; g < 4; g++) {
                                        jj[g] = g ? jj[g - 1] : 0;
                                        if (mh) { jj[g] = __ffsll((long long)mh) - 1; mh &= mh - 1; cnt = g + 1; }
                                    }
#pragma unroll
                                    for (int g = 0; g < 4; g++) { pp[g] = npos[(w << 6) + jj[g]]; oo[g] = no[(w << 6) + jj[g]]; }
                                    if (cnt == 4 && sink.defer) { // four queue entries with one LDS atomic
                                        const uint32_t slot = atomicAdd(sink.qn, 4u);
#pragma unroll
                                        for (int g = 0; g < 4; g++) {
                                            const bool inF = (wF >> jj[g]) & 1ull; // forward stop; else reverse start
                                            queue_overlap<TAPW>(sink, slot + (uint32_t)g, sink.n + g, (w << 6) + jj[g], pp[g] - pos + 3, t == 0 ? !inF : inF, (my_o + oo[g]) / 2.0); // ave([o1,o2]), functions.py:385
                                        }
                                        sink.n += 4;
                                    } else {
#pragma unroll
                                        for (int g = 0; g < 4; g++)
                                            if (g < cnt) {
                                                const bool inF = (wF >> jj[g]) & 1ull;
                                                emit_overlap<FILL, TAPW>(sink, (w << 6) + jj[g], pp[g] - pos + 3, t == 0 ? !inF : inF, (my_o + oo[g]) / 2.0);
                                            }
                                    }
                                }
                            }
                            while (m) { // four candidates per step: their node records are fetched together (the pass waits on these gathers)
                                int uu[4], cnt = 0;
#pragma unroll
                                for (int g = 0; g < 4; g++) {
                                    uu[g] = g ? uu[g - 1] : 0;
                                    if (m) { uu[g] = (w << 6) + __ffsll((long long)m) - 1; m &= m - 1; cnt = g + 1; }
                                }
                                DNode RR[4];
#pragma unroll
                                for (int g = 0; g < 4; g++) RR[g] = nd[uu[g]];
#pragma unroll
                                for (int g = 0; g < 4; g++) {
                                    if (g >= cnt) continue;
                                    const int u = uu[g];
                                    const DNode R = RR[g];
                                    const int r = R.pos, rf = NFRAME(R.info), r_other = R.other;
                                    const int d = r - pos;
                                    bool hit, diff;
                                    if (t == 1) { // v = reverse stop (l), lf < 0
                                        if (rf < 0) { hit = f != rf && r < my_other && r_other < pos; diff = false; }  // right is a reverse start
                                        else { hit = r_other + 3 < pos && r < my_other; diff = true; }                 // right is a forward stop
                                    } else { // v = forward start (l), lf > 0
                                        if (rf > 0) { hit = f != rf && r < my_other && r_other < pos; diff = false; }  // right is a forward stop
                                        else { hit = r_other < pos && r < my_other; diff = true; }                     // right is a reverse start
                                    }
                                    if (!FILL && hit && u - a < 64) hm |= 1ull << (u - a);
                                    if (!FILL && hit && u - a >= 64) mr_partial = true; // (an overlap edge beyond the verdict mask: k_edges_scan cannot see it)
                                    if (hit) emit_overlap<FILL, TAPW>(sink, u, d + 3, diff, FILL ? (my_o + no[u]) / 2.0 : 0.0);
                                }
                            }
                        }
                        if (!FILL) {
                            ehit[v] = hm;
                            // a window of k_sssp_wave that starts at (or just before) v must hold every node of the next 500 bp:
                            // at most 64 close and 64 open ones.  Contigs that break this go to k_sssp_lds from the start.
                            const int n_ahead = e500 >= a ? e500 - a + 1 : 0;
                            if (n_close_ahead > 61 || n_ahead - n_close_ahead > 60) dense = true;
                        }
                    }
                    // long non-coding bridges, functions.py:334-354 (v as right node)
                    for (int k = 0; k < nbr; k++) {
                        const int last = bridges[k].last, bs = bridges[k].base;
                        if (!(bs - 1 <= pos && pos < bs + 500)) continue;
                        // left nodes with last-500 < l <= last+1
                        for (int u = rank_lt(last - 499); u < ncds && nd[u].pos <= last + 1; u++) {
                            if (LINK_KIND(nd[u].link) == LINK_TRNA) continue; // the bridges are laid before add_trnas runs (functions.py:320-357)
                            const int lt = NTYPE(nd[u].info), lf = NFRAME(nd[u].info);
                            const int d = pos - nd[u].pos;
                            bool hit = false, diff = false;
                            if (t == 0) { // v forward start
                                if (lt == 1 && lf > 0) hit = true;
                                else if (lt == 0 && lf < 0) { hit = true; diff = true; }
                            } else { // v reverse stop
                                if (lt == 0 && lf < 0) hit = true;
                                else if (lt == 1 && lf > 0) { hit = true; diff = true; }
                            }
                            if (hit) {
                                if (d < 500) parallel = true; // the connect loop adds the same edge again: ValueError graphs.py:74
                                emit_edge<FILL>(sink, u, gap(d - 3, diff));
                            }
                        }
                    }
                }
            }
        }
        if (!FILL && v < V) in_off[v] = (uint32_t)sink.n; // in-degree; k_edges_scan turns it into an offset

        if (FILL && b.defer_overlap) finish_overlaps<TAPW>(s_q, &s_qn, (TAPW ? b.esrcf : b.esrc) + U(meta->edge_off), (TAPW ? (unsigned long long *)b.ewf : (unsigned long long *)b.ew) + U(meta->edge_off), cc);
    }
    if (parallel) atomicMin(&meta->status, PHX_S_PARALLEL);
    if (!FILL && dense) atomicOr(&meta->dense, 1);
    if (!FILL && mr_partial) atomicOr(&meta->dense, 2); // the step-back table of k_edges_scan is incomplete for this contig: the solver falls back on positions
}
template <bool FILL, bool TAPW = false, bool CODED = false>
__global__ __launch_bounds__(NT, EDGE_WPS) void k_edges(DBatch b) { b_edges<FILL, TAPW, CODED>(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// The ORF edges (functions.py:311-318: start node -> stop node of every ORF; on the reverse strand the stop node is the source) are the whole rows of
// the close CDS nodes.  As a thread per close NODE (k_edges<true> until round 6) a row costs three dependent gathers — node record, group record, the
// group's start nodes / weights — with 64 lanes on 64 lines each; as a thread per ORF the ORF arrays are read in order, the ORFs of a group are
// neighbours (one group record, one row offset, consecutive slots), and the 1.25 M close nodes leave the neighbour-scan kernel: DBatch.orf_rows.
__global__ __launch_bounds__(NT) void k_edges_orf(DBatch b) {
    if (b.tot->overflow) return;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (meta->status < 0 || meta->n_node <= 2) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const long long *owi = b.owi + meta->orf_off;
    const uint8_t *oflag = b.oflag + meta->orf_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    uint32_t *esrc = b.esrc + meta->edge_off;
    long long *ew = b.ew + meta->edge_off;
    for (int i = (int)blockIdx.y * NT + (int)threadIdx.x; i < meta->n_orf; i += (int)gridDim.y * NT) {
        const DOrf o = orf[i];
        const DGrp G = grp[o.grp];
        const int start_node = onode[i];
        const bool fwd = o.frame > 0;
        const int dst = fwd ? G.node : start_node, src = fwd ? start_node : G.node; // (reverse strand: the edge runs from the group's stop node to the start node)
        const uint32_t e = in_off[dst] + (fwd ? (uint32_t)(i - G.orf_begin) : 0u);
        esrc[e] = (uint32_t)src | OFLAG_BITS(oflag[i]);
        ew[e] = owi[i];
    }
}

// score_gap (functions.py:36-46) depends only on (length, strand pair): the contig's gap table, as the records the edge arrays take — the encoded
// integer per entry for k_edges<true> and for every reader of a coded gap edge, and per entry the high part of the source word.  Needs the
// contig's g+c count only: a kernel of its own on the side stream of k_bit_prefix, beside the ORF scan (in k_edges_scan, one workgroup per
// contig on the critical path, the 803 powers cost 16 us; beside k_orf_stats / k_score 16 us as well; in k_edges<true>, where every workgroup
// made its own until round 6, 15 % of that kernel's VALU instructions).
__device__ __forceinline__ void b_gap_table(const DBatch &b, const int bx, const int nthreads) {
    if (b.tot->overflow) return;
    const DMeta *meta = &b.meta[bx];
    if (meta->status < 0) return;
    long long *gt = b.gtab + (size_t)bx * GT_N;
    uint16_t *gf = b.gtabf + (size_t)bx * GT_N;
    const double pgap = contig_pstop(meta->gc, meta->L), cc = CERT_C(b);
    const double g100 = pow(1.0 - pgap, 100.0);
    const bool may_code = b.gap_code && 2 * (int64_t)meta->L + 2 <= ESRC_GAP_NODES; // the source of a coded gap edge has 19 bits (a contig has at most 2 L + 2 nodes; the node count itself is not known yet where this runs)
    int anyf = 0;
    for (int i = threadIdx.x; i < GT_SAME + GT_DIFF; i += nthreads) {
        const int length = (i < GT_SAME ? i : i - GT_SAME) - 2;
        double w = length > 300 ? g100 + (double)length : 1.0 / pow(1.0 - pgap, (double)length / 3.0);
        if (i >= GT_SAME) w += 20.0;
        const EWt e = make_ew<false>(w, cc);
        // (a flagged entry — inexact, or beyond 2^51 — keeps the explicit form: k_refine and the solver's slow path read DBatch.ew; one beyond 31 bits too)
        const bool coded = may_code && !e.fl && !(e.bits >> 31);
        gt[i] = (long long)e.bits;
        gf[i] = (uint16_t)(((e.fl >> 30) << 11) | (coded ? (1u << 10) | (uint32_t)i : 0u));
        if (e.fl) anyf = 1; // (nearly never: a tabulated weight within its error bound of an integer)
    }
    anyf = __syncthreads_or(anyf);
    if (threadIdx.x == 0) { gt[GT_N - 1] = __double_as_longlong(g100); gt[GT_N - 2] = anyf ? 1ll : 0ll; }
}
__global__ __launch_bounds__(NT) void k_gap_table(DBatch b) { b_gap_table(b, (int)blockIdx.x, NT); }

// The same for ONE contig by the workgroup (or wavefront) that is about to solve it with a kernel that reads plain rows (k_sssp_wave, k_sssp_lds, k_sssp: the
// roomy / wide / fallback kernels of a batch whose gap edges are coded): no launch of its own — two empty launches per run were 8 us of a lone genome's
// 330.  The caller synchronises its threads behind it.
__device__ __forceinline__ void expand_contig(const DBatch &b, const DMeta *meta, const int tid, const int nthreads) {
    if (!b.gap_code || !b.gtab) return;
    const uint32_t E = (uint32_t)meta->n_edge;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    long long *ew = b.ew + meta->edge_off;
    const long long *gt = b.gtab + (size_t)(meta - b.meta) * GT_N;
    for (uint32_t e = (uint32_t)tid; e < E; e += (uint32_t)nthreads) {
        const uint32_t sw = esrc[e];
        if (ESRC_IS_GAP(sw)) ew[e] = gt[ESRC_GAP_CODE(sw)];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // (this CU reads them back: its L1 writes through and holds none of these lines yet)
}

// DBatch.ew of the coded gap edges, for the consumers that read plain (source, weight) rows: the taps (the solver kernels other than k_sssp_duo
// k_sssp_lds and k_sssp complete their own contigs, expand_contig; k_sssp_wave, a 256-register kernel that the loop cost six more spilled registers and a
// 1250-contig batch 0.06 ms, gets a launch of this kernel in front of it).  nl > 0: only the contigs of that limb class and solver kernel `mode`.
__global__ __launch_bounds__(NT) void k_edges_expand(DBatch b, int nl, int mode) {
    if (b.tot->overflow) return;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (meta->status < 0 || meta->n_node <= 2) return;
    if (nl > 0 && (meta->sssp_nl != nl || meta->sssp_mode != mode)) return;
    const uint32_t E = (uint32_t)meta->n_edge;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    long long *ew = b.ew + meta->edge_off;
    const long long *gt = b.gtab + (size_t)blockIdx.x * GT_N;
    for (uint32_t e = blockIdx.y * NT + threadIdx.x; e < E; e += gridDim.y * NT) {
        const uint32_t sw = esrc[e];
        if (ESRC_IS_GAP(sw)) ew[e] = gt[ESRC_GAP_CODE(sw)];
    }
}

// in-degrees -> exclusive offsets (CSR by destination), one workgroup per contig
#ifndef ES_T
#define ES_T 512 // threads of a k_edges_scan workgroup (one per contig; 256: edge count + scan + layout 0.141 ms, 512: 0.134, 1024: 0.137)
#endif
// INWG: behind the counting pass in one launch (k_graph_chain): the status, which that pass lowers by atomicMin, is read at L2
template <int EST, bool INWG = false>
__device__ __forceinline__ void b_edges_scan(const DBatch &b, const int bx) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    __shared__ uint32_t s_scan[EST / 64 + 1];
    DMeta *meta = &b.meta[bx];
    const int status = INWG ? __hip_atomic_load(&meta->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : meta->status;
    if (status < 0 || meta->n_node <= 0) {
        if (threadIdx.x == 0) meta->n_edge = 0;
        return;
    }
    const int V = meta->n_node;
    uint32_t *in_off = b.in_off + meta->node_off + bx;
    const int per = (V + EST - 1) / EST;
    const int a = (int)threadIdx.x * per, e = a + per < V ? a + per : V;
    uint32_t sum = 0;
    for (int v = a; v < e; v++) sum += in_off[v];
    // The lowest head of the overlap (backward) edges out of every close node, from the verdict masks of the open nodes (bit j of
    // ehit[l] = an edge from node a + j, a = the first node right of l's position): k_wave_plan watches a close node only where
    // that reaches into the part of the sweep that is already final, and k_sssp_wave steps back exactly to it.  LDS window over
    // the node ids, moved along in segments (a head's sources lie less than 128 ids above it: 64 bits of mask + the nodes at its
    // own position); no global atomics.  (An overlap edge beyond a node's first 64 candidates has no bit: k_edges<false> marks such
    // a contig, DMeta.dense bit 1, and the solver keeps to the position rule there.)
    {
        constexpr int SEG = 4096, OVH = 128;
        __shared__ uint32_t s_mr[SEG + OVH];
        uint32_t *mreach = b.mreach + 4 * (size_t)meta->node_off;
        const uint64_t *ehit = b.ehit + meta->node_off;
        const int32_t *npos = b.npos + meta->node_off;
        const int ncds = V - 2;
        for (int i = threadIdx.x; i < SEG + OVH; i += EST) s_mr[i] = ~0u;
        __syncthreads();
        for (int s0 = 0; s0 < ncds; s0 += SEG) {
            for (int l = s0 + (int)threadIdx.x; l < s0 + SEG && l < ncds; l += EST) {
                uint64_t hm = ehit[l];
                if (!hm) continue;
                int fa = l + 1;
                const int pl = npos[l];
                while (fa < ncds && npos[fa] == pl) fa++; // the other nodes at l's position come first
                while (hm) { const int j = __ffsll((long long)hm) - 1; hm &= hm - 1; const int r = fa + j - s0; if (r < SEG + OVH) atomicMin(&s_mr[r], (uint32_t)l); }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < SEG && s0 + i < ncds; i += EST) mreach[s0 + i] = s_mr[i]; // (every entry: nothing presets the table)
            if (s0 + SEG >= ncds) break;
            __syncthreads();
            const uint32_t carry = (int)threadIdx.x < OVH ? s_mr[SEG + threadIdx.x] : ~0u; // the overhang opens the next segment
            __syncthreads();
            for (int i = threadIdx.x; i < SEG + OVH; i += EST) s_mr[i] = ~0u;
            __syncthreads();
            if ((int)threadIdx.x < OVH) s_mr[threadIdx.x] = carry;
            __syncthreads();
        }
    }
    uint32_t tot;
    uint32_t ex = block_excl_scan<EST>(sum, s_scan, &tot);
    for (int v = a; v < e; v++) { const uint32_t d = in_off[v]; in_off[v] = ex; ex += d; }
    if (threadIdx.x == 0) { in_off[V] = tot; meta->n_edge = (int)tot; }
}
__global__ __launch_bounds__(ES_T) void k_edges_scan(DBatch b) { b_edges_scan<ES_T>(b, (int)blockIdx.x); }
// a few long contigs: 1024 threads per contig (T4: 11 nodes per thread on 512)
__global__ __launch_bounds__(1024) void k_edges_scan_big(DBatch b) { b_edges_scan<1024>(b, (int)blockIdx.x); }



// Nodes -> attributes -> edge count -> scan of one contig by ONE workgroup: the whole stretch between the ORF scan and k_layout2 needs the ORF and
// group records only (since the o-term left b_node_attr) and a contig's stages depend on that contig's earlier stages alone, so the four launches
// k_nodes_fused, k_node_attr, k_edges<false>, k_edges_scan are one, every contig proceeds on its own, and nothing waits for the slowest contig of
// a stage three times over.  Between the bodies the workgroup-scope fence and barrier of k_nodes_fused (see there: never agent scope); a field a
// stage in front changed by L2 atomics (n_bridge, status) is read at L2 (INWG).  No atomics on batch totals, no workgroup waits for another.
#ifndef CHAIN_T
#define CHAIN_T 512 // threads of its workgroup (1000 x 50 kb, step: 256: 1.572 ms, 512: 1.504, 1024: 1.571; the four staged launches on the same streams: 1.539)
#endif
#ifndef CHAIN_WPS
#define CHAIN_WPS 8 // wavefronts per SIMD the register allocation must allow (64 VGPRs)
#endif
template <int T>
__global__ __launch_bounds__(T, CHAIN_WPS) void k_graph_chain(DBatch b) {
    const int bx = blockIdx.x;
    auto stage_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    b_node_cov<T>(b, bx, 0, 1);
    stage_sync();
    b_node_rank<T>(b, bx);
    stage_sync();
    b_node_build<T>(b, bx, 0, 1);
    stage_sync();
    b_node_order<T>(b, bx);
    stage_sync();
    b_node_attr<T>(b, bx, 0, 1);
    stage_sync();
    b_edges<false, false, false, T, true>(b, bx, 0, 1);
    stage_sync();
    b_edges_scan<T, true>(b, bx);
}
