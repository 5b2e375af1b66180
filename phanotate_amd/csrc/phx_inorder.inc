// phx_inorder.inc — k_inorder: parents as an in-place Bellman-Ford leaves them (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// With exact integers the distance vector is unique, the path is not: when two in-edges of a node are both tight
// (d[u] + w == d[v]) either may be its parent.  The reference's solver (fastpathz, phanotate.py:56-64; restated by the
// golden generator) relaxes the edges in place, in Graph.iteredges order (graphs.py:121-126), round after round, with a
// strict '<': the parent of v is the edge that FIRST brings d[v] down to its final value.  That edge is determined by
// the final distances alone:
//   * an edge e = (u -> v) can write the final d[v] only if it is tight and d[u] is already final when e is visited;
//   * let T(v) = (round, index of the edge) at which v became final, T(source) = (0, before every edge).  A tight edge e
//     fires at next(e, T(u)) = (round(u) + [e comes before parent_edge(u) in the edge order], e), and
//     T(v) = min over the tight in-edges of v, parent(v) = the arg min.
// Edges are ordered by (insertion rank of the source node, ...) and two edges that are ever compared here have different
// sources (in-edges of one node; an edge and the parent edge of its source), so the insertion rank of the source node is
// all that is needed: node_refkey() — the stop-groups in discovery order (DGrp.evkey), inside a group the nodes as
// functions.py:311-318 inserts them.  phx_solve passes the caller's edge order instead (DBatch.ekey).
//
// The kernels before this one pick the lowest in-edge index as parent.  Nearly always no node on the path has a second
// tight in-edge (none of the benchmark's contigs; ~2 % of tools/fuzz_gpu.py's): then the path is the only shortest
// path and this kernel only checks that (one pass over the in-edges of the path's nodes).  Otherwise it builds the set A
// of tight ancestors of the target (the path + what branches off), computes T on A — a node becomes final when all its
// tight in-neighbours are, a Dijkstra step on the earliest firing edge breaks the deadlock of a zero-length cycle — and
// walks the parents again.
#define IO_T_FULL 256 // threads of a k_inorder workgroup (64 for batches of short contigs: a workgroup is one contig)
#define IO_T_BIG 1024 // ... for the few long contigs of a small batch (T4 alone: 5519 nodes, 594 on the path): the parents of 8192 nodes staged at once, 1024 path nodes checked per pass (0.12 -> see DESIGN.md §7)
#ifndef IO_SKIP_T
#define IO_SKIP_T IO_T_BIG // workgroup sizes from which the path is walked in strides (needs a second table of WALK entries in LDS)
#endif
#define IO_WALK 4096 // parents staged per chunk of the path walk,
#define IO_PATH 2048 // nodes of the path kept in LDS while it is walked (a quarter of both in the one-wavefront variant for short contigs)

// insertion rank of node v in the reference graph as an order-preserving key (>= 1)
__device__ __forceinline__ uint64_t node_refkey(const DNode *nd, const DOrf *orf, const DGrp *grp, const DTNode *tn, int v, int V) {
    if (v >= V - 2) return ~0ull - (uint64_t)(V - 1 - v); // source, then target (functions.py:440-443)
    const uint32_t link = nd[v].link;
    if (LINK_KIND(link) == LINK_TRNA) return (0xC0000000ull << 32) | (uint32_t)tn[LINK_IDX(link)].rank; // after every CDS node (functions.py:357)
    uint32_t g, sub;
    if (LINK_KIND(link) == LINK_STOP) { g = LINK_IDX(link); sub = grp[g].frame > 0 ? 1u : 0u; }
    else {
        const uint32_t k = LINK_IDX(link);
        g = (uint32_t)orf[k].grp;
        const uint32_t mth = k - (uint32_t)grp[g].orf_begin;
        // forward group: start of the first ORF, the stop, the other starts; reverse group: the stop, the starts
        sub = grp[g].frame > 0 ? (mth == 0 ? 0u : 1u + mth) : 1u + mth;
    }
    return (((uint64_t)(uint32_t)grp[g].evkey + 1ull) << 32) | sub;
}

template <int IO_T>
struct IoShared {
    int flag, nA, ne, prog, hi, changed, np, fail;
    long long off;
    uint32_t g0;
    uint32_t scan[IO_T / 64 + 1];
    uint32_t e0[IO_T + 1]; // chunk of the path: running count of in-edges,
    uint32_t ef[IO_T];     //   first in-edge,
    uint32_t pe[IO_T];     //   parent edge,
    int32_t v[IO_T];       //   node
    int32_t wv, wn, wcb, wstate; // walk_path: current node, hops so far, first node of the staged chunk, 0 walking / 1 reload / 2 done / 3 cycle
    static constexpr int WALK = IO_T >= IO_T_BIG ? 2 * IO_WALK : (IO_T >= IO_T_FULL ? IO_WALK : IO_WALK / 4), PATH = IO_T >= IO_T_FULL ? IO_PATH : IO_PATH / 4;
    int32_t pc[WALK];      //   parent NODE of the nodes [wcb, wcb + WALK)
    int32_t rpath[PATH];   //   the path, target first (longer paths continue in global memory)
    static constexpr int SKIP = IO_T >= IO_SKIP_T ? WALK : 1, NCP = IO_T >= IO_SKIP_T ? WALK / 8 + 2 : 1;
    int32_t pj[SKIP];      //   (the 1024-thread variant, a contig that fits one chunk) 8th ancestor of every node: the path is walked 8 hops at a time,
    int32_t cp[NCP];       //   the nodes at hops 0, 8, 16, ... are check points, and one thread per check point fills in the 8 hops behind it
};

// Path walk for the contigs k_sssp_wave solved (it leaves n_path = -2): target -> source along the parent edges, path[] in
// source..target order, status / gene records as the other solver kernels write them (phanotate.py:63-76).  The parents of
// IO_WALK consecutive nodes are staged in LDS (two dependent loads per node, all in flight at once) and one thread chases them
// there; the path runs right to left (a connector reaches back < 500 bp), so a 50 kb contig needs one or two chunks.
template <int NL, int IO_T>
__device__ void walk_path(const DBatch &b, DMeta *meta, IoShared<IO_T> *sh) {
    const int tid = threadIdx.x;
    constexpr int WALK = IoShared<IO_T>::WALK, PATH = IoShared<IO_T>::PATH;
    const int V = meta->n_node, SRC = V - 2, TGT = V - 1;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const int32_t *gpe = b.parent + meta->node_off;
    int32_t *path = b.path + meta->node_off;
    if (tid == 0) { sh->wv = TGT; sh->wn = 0; sh->wcb = V > WALK ? V - WALK : 0; sh->wstate = 1; sh->rpath[0] = TGT; }
    __syncthreads();
    while (sh->wstate == 1) {
        const int cb = sh->wcb;
        for (int i0 = 0; i0 < WALK && cb + i0 < V; i0 += 8 * IO_T) { // eight loads in flight per round trip
            int32_t x[8];
#pragma unroll
            for (int g = 0; g < 8; g++) { const int i = i0 + g * IO_T + tid; x[g] = (i < WALK && cb + i < V) ? gpe[cb + i] : -1; }
#pragma unroll
            for (int g = 0; g < 8; g++) x[g] = x[g] >= 0 ? (int32_t)ESRC_NODE(esrc[x[g]]) : -1; // parent edge -> parent node
#pragma unroll
            for (int g = 0; g < 8; g++) { const int i = i0 + g * IO_T + tid; if (i < WALK) sh->pc[i] = x[g]; }
        }
        __syncthreads();
        if constexpr (IO_T >= IO_SKIP_T) {
            // One thread chasing ~600 parents through LDS was half of this kernel for T4 (594 hops of ~180 clocks).  When the contig fits the chunk:
            // 8th ancestors by three rounds of pointer doubling (a node without a parent, and the source, point at themselves), the walk in strides
            // of 8, the hops between by one thread per stride.
            if (cb == 0 && V <= WALK) {
                for (int v = tid; v < V; v += IO_T) { const int pv = sh->pc[v]; sh->pj[v] = (v == SRC || pv < 0) ? v : pv; }
                __syncthreads();
                for (int r = 0; r < 3; r++) {
                    int32_t nx[(WALK + IO_T - 1) / IO_T];
                    int k = 0;
                    for (int v = tid; v < V; v += IO_T) nx[k++] = sh->pj[sh->pj[v]];
                    __syncthreads();
                    k = 0;
                    for (int v = tid; v < V; v += IO_T) sh->pj[v] = nx[k++];
                    __syncthreads();
                }
                if (tid == 0) { // check points: cp[k] = the node 8k hops from the target (a chain that has ended stays where it ended)
                    int v = TGT, k = 0;
                    sh->cp[0] = v;
                    while (v != SRC && k < V / 8 + 1) { v = sh->pj[v]; sh->cp[++k] = v; }
                    sh->np = k; // strides taken
                    sh->fail = 0;
                }
                __syncthreads();
                const int nst = sh->np;
                if (8 * (nst + 1) < PATH) { // (the path fits rpath; else: the walk below)
                    bool dead = false; // a node without a parent in front of the source
                    for (int k = tid; k < nst; k += IO_T) {
                        int v = sh->cp[k];
                        for (int h = 1; h <= 8; h++) {
                            if (v == SRC) break;
                            const int pv = sh->pc[v];
                            if (pv < 0) { dead = true; break; }
                            v = pv;
                            sh->rpath[8 * k + h] = v;
                        }
                    }
                    if (dead) sh->fail = 1;
                    __syncthreads();
                    if (tid == 0) {
                        int st = 2, n = 0;
                        if (sh->fail || sh->cp[nst] != SRC) st = 3; // a dead end, or V hops without meeting the source: the parents run in a circle
                        else if (nst > 0) { // hops: 8 per stride, the last stride up to where it met the source
                            n = 8 * (nst - 1);
                            for (int v = sh->cp[nst - 1]; v != SRC; v = sh->pc[v]) n++;
                        }
                        sh->fail = 0;
                        sh->wv = SRC; sh->wn = n; sh->wstate = st;
                    }
                    __syncthreads();
                    continue;
                }
            }
        }
        if (tid == 0) { // hop n is kept at rpath[n] (LDS) or, past PATH, reversed at the tail of path[]
            int v = sh->wv, n = sh->wn, st = 0;
            while (true) {
                if (v == SRC) { st = 2; break; }
                if (v < cb) { sh->wcb = v + 256 > WALK ? v + 256 - WALK : 0; st = 1; break; } // the chunk that ends just above v
                if (++n >= V) { st = 3; break; }
                v = sh->pc[v - cb];
                if (v < 0) { st = 3; break; }
                if (n < PATH) sh->rpath[n] = v; else path[V - 1 - n] = v;
            }
            sh->wv = v; sh->wn = n; sh->wstate = st;
        }
        __syncthreads();
    }
    const int n = sh->wn; // n edges, n + 1 nodes
    if (sh->wstate == 3) { if (tid == 0) meta->n_path = -1; return; } // the lowest-index parents run in a circle (zero-length cycle): see inorder_contig
    if (n >= PATH) { // the part that went to global memory: path[V-1-k] (k = PATH..n) -> path[n-k]
        __threadfence_block();
        const int shift = V - 1 - n;
        if (shift > 0)
            for (int k0 = 0; k0 <= n - PATH; k0 += IO_T) {
                const int k = k0 + tid;
                int x = 0;
                if (k <= n - PATH) x = path[shift + k];
                __syncthreads();
                if (k <= n - PATH) path[k] = x;
                __syncthreads();
            }
    }
    for (int k = tid; k <= n && k < PATH; k += IO_T) path[n - k] = sh->rpath[k];
    const int np = n / 2; // shortest_path[1:] taken two at a time (file_handling.pairwise)
    if (tid == 0) { const uint32_t g0 = !b.genes ? 0u : (b.gpack ? (uint32_t)(meta->grp_off + meta->tn_off) : atomicAdd(b.gene_total, (uint32_t)np)); sh->g0 = g0; meta->n_path = n + 1; meta->n_genes = b.genes ? np : 0; meta->gene_off = g0; }
    __syncthreads();
    __threadfence_block();
    if (b.genes && np > 0) emit_genes(b, meta, path, np, (size_t)sh->g0, tid, IO_T);
    __syncthreads();
}

// P: the policy of the sweep that made the distances (phx_sssp.inc: SwRun for the run, whose instantiations look at none of the pointers
// below; RePol for a re-solve, phx_resolve.inc).  A row is tight iff d[u] + w == d[v] with w as that sweep added it:
// MASKED: `mask` holds one bit per in-edge slot of the batch (bit edge_off + e); a refused edge is no edge — it is never tight, whatever the
// distances say.  REQ (on one limb more than the contig's class): a row whose bit is set in `req` weighs W - 2^(64 (NL - 1)).  BIAS: a row
// whose bit is set in `bbit` weighs W + B, B the word of its in-edge slot in `bval` — under BLIST the entry of the solve's sorted list of
// nbl (in-edge slot, B) pairs (bias_at, phx_sssp.inc).  REQ and BIAS are independent: a row that is both weighs W + B - 2^(64 (NL - 1)).
// ci: the contig's index in the batch (blockIdx.x where a workgroup is a contig; a scenario slot passes its slot's contig).
template <int NL, int IO_T, class P = SwRun>
__device__ void inorder_contig(const DBatch &b, DMeta *meta, const uint32_t ci, IoShared<IO_T> *sh, const uint32_t *mask = nullptr, const uint32_t *req = nullptr, const uint32_t *bbit = nullptr, const long long *bval = nullptr, const int nbl = 0) {
    constexpr bool MASKED = P::MASKED, REQ = P::REQ, BIAS = P::BIAS, BLIST = P::BLIST;
    const int tid = threadIdx.x;
    const uint64_t mbase = MASKED ? (uint64_t)meta->edge_off : 0ull;
    auto refused = [&](uint32_t e) -> bool { const uint64_t x = mbase + e; return ((mask[x >> 5] >> (x & 31)) & 1u) != 0; };
    auto required = [&](uint32_t e) -> bool { const uint64_t x = mbase + e; return ((req[x >> 5] >> (x & 31)) & 1u) != 0; };
    auto biased = [&](uint32_t e) -> bool { const uint64_t x = mbase + e; return ((bbit[x >> 5] >> (x & 31)) & 1u) != 0; };
    const int V = meta->n_node;
    const bool walked = meta->n_path >= 2; // else the solver's parents run in a circle (a zero-length cycle of tight edges): start from source and target alone
    const int n = walked ? meta->n_path : 2; // path[0] = source ... path[n-1] = target
    const uint32_t *in_off = b.in_off + meta->node_off + ci;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const uint64_t *ewl = b.ewl ? b.ewl + (size_t)meta->edge_off * NL : nullptr;
    const uint32_t *ekey_arr = b.ekey ? b.ekey + meta->edge_off : nullptr;
    const uint64_t *dist = b.dist + (size_t)meta->node_off * b.dist_stride;
    const DNode *nd = b.node ? b.node + meta->node_off : nullptr;
    const DOrf *orf = b.orf ? b.orf + meta->orf_off : nullptr;
    const DGrp *grp = b.grp ? b.grp + meta->grp_off : nullptr;
    const DTNode *tn = b.tnode ? b.tnode + meta->tn_off : nullptr;
    int32_t *path = b.path + meta->node_off;
    const long long *gt = gtab_at(b, ci);
    auto tight = [&](uint32_t e, const WInt<NL> &dv) -> bool {
        if constexpr (MASKED) { if (refused(e)) return false; }
        const uint32_t sw = esrc[e];
        const WInt<NL> du = wi_load<NL>(dist + (size_t)ESRC_NODE(sw) * NL);
        WInt<NL> w = ewl ? wi_load<NL>(ewl + (size_t)e * NL) : ew_decode<NL>(edge_wenc(sw, ew, e, gt));
        if constexpr (REQ) { if (required(e)) w.v[NL - 1] -= 1ull; }
        if constexpr (BIAS) {
            if (biased(e)) {
                if constexpr (BLIST) w = wi_add<NL>(w, ew_decode<NL>(bias_at<true>(bval, mbase + e, nbl)));
                else w = wi_add<NL>(w, ew_decode<NL>(bval[mbase + e])); // (bias_at<false>, written out: through the call the biased k_rs_inorder came out with other scalar registers than it had)
            }
        }
        return !wi_unreached<NL>(du) && wi_eq<NL>(wi_add<NL>(du, w), dv);
    };
    // ---- 1. does any node of the path have a tight in-edge besides its parent edge? ----
    // 256 path nodes at a time; their in-edges are spread evenly over the threads (a node has 1 to ~75 of them)
    const uint32_t *pedge = (const uint32_t *)(b.parent + meta->node_off);
    bool mine = !walked;
    for (int c0 = 1; c0 < n && walked; c0 += IO_T) { // path[0] is the source
        const int i = c0 + tid;
        uint32_t deg = 0;
        if (i < n) {
            const int v = path[i];
            const uint32_t f = in_off[v];
            deg = in_off[v + 1] - f;
            sh->v[tid] = v; sh->ef[tid] = f; sh->pe[tid] = pedge[v];
        }
        uint32_t total;
        const uint32_t ex = block_excl_scan<IO_T>(deg, sh->scan, &total);
        sh->e0[tid] = ex;
        if (tid == 0) sh->e0[IO_T] = total;
        __syncthreads();
        for (uint32_t f0 = (uint32_t)tid; f0 < total; f0 += 4 * IO_T) {
            uint32_t e[4]; int j[4]; bool on[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t f = f0 + (uint32_t)q * IO_T;
                on[q] = f < total;
                int lo = 0, hi = IO_T; // last j with e0[j] <= f
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sh->e0[mid] <= f) lo = mid; else hi = mid; }
                if (!on[q]) lo = 0; // (entry 0 of the chunk always exists)
                j[q] = lo;
                e[q] = sh->ef[lo] + (f - sh->e0[lo]);
                on[q] = on[q] && e[q] != sh->pe[lo];
                if constexpr (MASKED) { if (on[q] && refused(e[q])) on[q] = false; }
            }
            uint32_t u[4]; WInt<NL> w[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t ee = on[q] ? e[q] : 0u;
                const uint32_t sw = esrc[ee];
                u[q] = ESRC_NODE(sw);
                w[q] = ewl ? wi_load<NL>(ewl + (size_t)ee * NL) : ew_decode<NL>(edge_wenc(sw, ew, ee, gt));
                if constexpr (REQ) { if (required(ee)) w[q].v[NL - 1] -= 1ull; }
                if constexpr (BIAS) {
                    if (biased(ee)) {
                        if constexpr (BLIST) w[q] = wi_add<NL>(w[q], ew_decode<NL>(bias_at<true>(bval, mbase + ee, nbl)));
                        else w[q] = wi_add<NL>(w[q], ew_decode<NL>(bval[mbase + ee]));
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const WInt<NL> du = wi_load<NL>(dist + (size_t)u[q] * NL), dv = wi_load<NL>(dist + (size_t)sh->v[j[q]] * NL);
                mine |= on[q] && !wi_unreached<NL>(du) && wi_eq<NL>(wi_add<NL>(du, w[q]), dv);
            }
        }
        __syncthreads();
    }
    if (mine) sh->flag = 1;
    __syncthreads();
    if (!sh->flag) return;

    // ---- 2. scratch for this contig ----
    const size_t sz4 = ((size_t)V * 4 + 7) & ~(size_t)7, E = (size_t)meta->n_edge;
    if (tid == 0) {
        const unsigned long long bytes = ((size_t)V * 8 + 7 * sz4 + E * 12 + 15) & ~(size_t)15;
        const unsigned long long off = atomicAdd((unsigned long long *)&b.tot->tie_need, bytes);
        sh->off = off + bytes <= (unsigned long long)b.tie_cap ? (long long)off : -1;
        if (sh->off < 0) atomicOr(&b.tot->overflow, 4); // the host grows the scratch buffer and runs the batch again
        meta->tie = 1;
    }
    __syncthreads();
    if (sh->off < 0) return;
    uint8_t *scr = b.tie + sh->off;
    uint64_t *Tk = (uint64_t *)scr;                 // per node of A: key of its parent edge
    int32_t *amap = (int32_t *)(scr + (size_t)V * 8); // node id -> index in A, -1: not in A
    int32_t *anode = (int32_t *)((uint8_t *)amap + sz4);
    uint32_t *estart = (uint32_t *)((uint8_t *)anode + sz4), *ecnt = (uint32_t *)((uint8_t *)estart + sz4);
    uint32_t *Tr = (uint32_t *)((uint8_t *)ecnt + sz4);  // round in which the node became final
    int32_t *par = (int32_t *)((uint8_t *)Tr + sz4);     // index in A of the parent
    uint32_t *done = (uint32_t *)((uint8_t *)par + sz4); // 0, or 1 + the iteration that made the node final
    uint64_t *ek = (uint64_t *)((uint8_t *)done + sz4);  // tight in-edges of A's nodes: key,
    int32_t *eu = (int32_t *)(ek + E);                   //   source (node id, then index in A)

    // ---- 3. A = the path + every tight ancestor of one of its nodes ----
    for (int v = tid; v < V; v += IO_T) amap[v] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += IO_T) { const int v = walked ? path[i] : (i == 0 ? V - 2 : V - 1); anode[i] = v; amap[v] = i; }
    if (tid == 0) { sh->nA = n; sh->ne = 0; }
    __syncthreads();
    for (int lo = 0, hi = n; lo < hi;) {
        for (int a = lo + tid; a < hi; a += IO_T) {
            const int x = anode[a];
            const WInt<NL> dv = wi_load<NL>(dist + (size_t)x * NL);
            const uint32_t e0 = in_off[x], e1 = in_off[x + 1];
            int c = 0;
            for (uint32_t e = e0; e < e1; e++) c += tight(e, dv) ? 1 : 0;
            int k = atomicAdd(&sh->ne, c);
            estart[a] = (uint32_t)k; ecnt[a] = (uint32_t)c;
            for (uint32_t e = e0; e < e1; e++)
                if (tight(e, dv)) {
                    const int u = (int)ESRC_NODE(esrc[e]);
                    eu[k] = u;
                    ek[k] = ekey_arr ? (uint64_t)ekey_arr[e] + 1ull : node_refkey(nd, orf, grp, tn, u, V);
                    k++;
                    if (atomicCAS(&amap[u], -1, -2) == -1) { const int idx = atomicAdd(&sh->nA, 1); anode[idx] = u; amap[u] = idx; }
                }
        }
        __syncthreads();
        lo = hi; hi = sh->nA;
        __syncthreads();
    }
    const int nA = sh->nA, ne = sh->ne;
    for (int k = tid; k < ne; k += IO_T) eu[k] = amap[eu[k]];
    for (int a = tid; a < nA; a += IO_T) { done[a] = a == 0 ? 1u : 0u; Tr[a] = 0; Tk[a] = 0; par[a] = -1; }
    if (tid == 0) { sh->fail = 0; sh->changed = 0; }
    __syncthreads();

    // ---- 4. T on A ----
    const int tgt = n - 1;
    for (uint32_t iter = 1;; iter++) {
        if (tid == 0) sh->prog = 0;
        __syncthreads();
        for (int a = tid; a < nA; a += IO_T) {
            if (done[a] || !ecnt[a]) continue;
            bool all = true;
            uint32_t br = ~0u; uint64_t bk = ~0ull; int bu = -1;
            for (uint32_t k = estart[a], k1 = k + ecnt[a]; k < k1; k++) {
                const int u = eu[k];
                const uint32_t d = done[u];
                if (d == 0 || d > iter) { all = false; break; } // not final, or final since this very iteration (its T may not be visible yet)
                const uint32_t r = Tr[u] + (ek[k] < Tk[u] ? 1u : 0u);
                if (r < br || (r == br && ek[k] < bk)) { br = r; bk = ek[k]; bu = u; }
            }
            if (all) { Tr[a] = br; Tk[a] = bk; par[a] = bu; done[a] = iter + 1; sh->prog = 1; }
        }
        __syncthreads();
        const bool fin = done[tgt] != 0, prog = sh->prog != 0;
        __syncthreads();
        if (fin) break;
        if (!prog) { // a cycle of tight edges (length 0): the earliest firing edge out of the final set is right (Dijkstra)
            if (tid == 0) {
                uint32_t br = ~0u; uint64_t bk = ~0ull; int bu = -1, ba = -1;
                for (int a = 0; a < nA; a++) {
                    if (done[a]) continue;
                    for (uint32_t k = estart[a], k1 = k + ecnt[a]; k < k1; k++) {
                        const int u = eu[k];
                        if (!done[u]) continue;
                        const uint32_t r = Tr[u] + (ek[k] < Tk[u] ? 1u : 0u);
                        if (r < br || (r == br && ek[k] < bk)) { br = r; bk = ek[k]; bu = u; ba = a; }
                    }
                }
                if (ba < 0) sh->fail = 1; // cannot happen: the target is reachable inside A
                else { Tr[ba] = br; Tk[ba] = bk; par[ba] = bu; done[ba] = iter + 1; }
            }
            __syncthreads();
            if (sh->fail) break;
        }
        if (iter > 2u * (uint32_t)nA + 8u) { if (tid == 0) sh->fail = 1; __syncthreads(); break; }
    }
    if (sh->fail) { if (tid == 0) { meta->tie = -1; if (!walked) { meta->status = PHX_S_NEGCYCLE; meta->n_path = 0; } } return; } // the path of the solver stands

    // ---- 5. walk the parents; rewrite path and genes if the path differs ----
    if (tid == 0) {
        int m = 0;
        bool same = true;
        for (int a = tgt; a != 0 && m <= nA; a = par[a]) m++;
        if (m > nA) { sh->fail = 1; meta->tie = -1; if (!walked) { meta->status = PHX_S_NEGCYCLE; meta->n_path = 0; } }
        else {
            same = walked && m == n - 1;
            if (same) { int j = n - 1; for (int a = tgt; a != 0; a = par[a], j--) if (a != j) { same = false; break; } } // anode[j] = old path[j]: same path <=> A indices count down
            if (!same) {
                int k = m;
                for (int a = tgt;; a = par[a]) { path[k--] = anode[a]; if (a == 0) break; }
                meta->n_path = m + 1;
                const int np = m / 2;
                uint32_t g0 = (uint32_t)meta->gene_off;
                if (b.genes && np > meta->n_genes && !b.gpack) g0 = atomicAdd(b.gene_total, (uint32_t)np); // (gpack: the contig's place holds any path of its)
                meta->gene_off = g0; meta->n_genes = b.genes ? np : 0;
                sh->np = np; sh->g0 = g0; sh->changed = 1;
                meta->tie = 2;
            }
        }
    }
    __syncthreads();
    if (sh->changed && b.genes) {
        __threadfence_block();
        emit_genes(b, meta, path, sh->np, (size_t)sh->g0, tid, IO_T);
    }
}

// one instantiation per integer class (the launcher starts those that occur in the batch): the 1088-bit one would
// otherwise set the register budget of all
template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_inorder(DBatch b) {
    __shared__ IoShared<IO_T> sh;
    if (b.tot->overflow & 3) return; // (bit 2 is raised by this kernel itself)
    DMeta *meta = &b.meta[blockIdx.x];
    if (meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (meta->status < 0 || (meta->n_node <= 2 && !b.ewl)) return;
    if (meta->n_path == -2) walk_path<NL, IO_T>(b, meta, &sh); // solved by k_sssp_wave: not walked yet
    __syncthreads();
    if (meta->n_path < 2 && meta->n_path != -1) return; // no path; -1: the walk along the lowest-index parents cycled
    inorder_contig<NL, IO_T>(b, meta, blockIdx.x, &sh);
}
