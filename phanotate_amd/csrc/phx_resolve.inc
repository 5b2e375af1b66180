// phx_resolve.inc — re-annotation: the best path of a contig's graph with chosen ORFs refused, required or biased (included by phx_kernels.hip;
// DESIGN.md §14, §16-§20, §22, §23, §27).
// ------------------------------------------------------------------------------------------------
// On demand after a run, kernel by kernel on the context's stream; never in phx_run, the captured graph or the certificate path.
// The kernels get TWO views of the batch: the graph (in_off / esrc / ew / gtab, nodes, ORFs, groups) is the run's, read only; every output
// (DMeta, DTotals, dist, parent, path, genes, gene_total, the tie scratch) is the re-annotation's own — the DBatch they receive is the run's with
// those pointers replaced (phx_analyses.inc, reann_batch), so the device code shared with the run (lds_sweep, inorder_contig, emit_genes)
// writes nothing the run's results live in.
//
// One chain — mark, sweep, in-order parents, record — serves every re-solve.  Two things choose among its instantiations:
//
//   a POLICY (RePol<REQ, BIAS, BLIST>) says what a marked row means.  Every re-solve is MASKED: an explicit row whose bit is set in `mask` is
//     no edge (§14).  REQ: a row whose bit is set in `req` weighs W - M, M = 2^(64 NL), on one limb more than the contig's class NL, so that
//     the top limb of a distance counts the required edges behind it (§16).  BIAS: a row whose bit is set in `bbit` weighs W + B, B a signed
//     integer of the caller's with |B| <= 2^52 (§19); REQ and BIAS together: W + B - M (§22).  BLIST: B comes from a sorted list of the
//     solve's own instead of a word per in-edge slot of the batch (§20; with REQ: a scenario slot that is pinned and biased, §27).  The policy's MODE (1 masked, 2 REQ, 3 BIAS, 4 both) is what the
//     host writes per contig (DReann.mode); ReSw<NL, Pol> adds the ring, the tile and the occupancy of the sweep per limb class.
//   a VIEW says where one workgroup's solve lives.  BatchView: the workgroup is a contig of the batch, its marks are DReann's batch-wide
//     bitmaps, and it takes part when the contig's mode is the policy's.  SlotView: the workgroup is a scenario slot (§17), its contig record
//     a copy of its own, its outputs and marks slices of DScen's buffers moved so that the shared code indexes them as it indexes the batch's.
//     A view yields meta, ci, mask, gplan, req, kreq, bbit, bval, nbl and the sum of |B|.
//
//   k_rs_mask, k_sc_mask / k_scp_mask / k_sce_mask   the marks: an ORF finds its edge (re_orf_edge) and sets that in-edge slot's bit.
//   k_rs_lds, k_sc_lds<NL, Pol>           RE_SWEEP: lds_sweep (phx_sssp.inc) under the policy, behind the limb test on the sum of |B|.
//   k_rs_inorder, k_sc_inorder<NL, IO_T, Pol>   RE_INORDER: inorder_contig (phx_inorder.inc) under the policy, the reference's parent rule.
//   k_rs_fin, k_sc_fin                    re_record: status, delta = float(D' - D) / 1000.0, unmet — what the host reads.
// The rules that decide bit-exactness live once each: refusal wins over a bias and an ORF without an edge is ignored (k_rs_mask / the slot mask
// kernels), only explicit rows are marked (re_orf_edge), the limb test before a biased sweep (RE_SWEEP).
// The bitmaps only ever hold bits of explicit rows: an ORF edge runs open -> close and a coded gap edge (a connector) close -> open, so no
// ORF shares both ends with a coded row, and re_orf_edge skips coded rows besides.  lds_sweep therefore tests explicit rows only, and the
// masked inorder_contig, which tests every row, sees the same graph.
// Bounds: the sweep and round caps of k_sssp_lds (PHX_S_NEGCYCLE), no waiting between workgroups, no index from the caller on the device
// (the host checks the offsets; `forb` is one byte and `bias` one word per ORF of the batch, `mode` one int per contig).

// ---- the policy ----
template <bool REQ_, bool BIAS_, bool BLIST_ = false>
struct RePol {
    static constexpr bool MASKED = true, REQ = REQ_, BIAS = BIAS_, BLIST = BLIST_;
    static constexpr int MODE = 1 + (REQ_ ? 1 : 0) + (BIAS_ ? 2 : 0); // DReann.mode of the contigs it solves
};
// The sweep's sizes for a contig of limb class NL under Pol: what lds_sweep reads as its policy.  The sweep runs on SNL limbs.  The 1088-bit
// class has a quarter of the ring and half the tile (109 KB of LDS instead of 283); under REQ the ring of the 320-bit solve is halved (66 KB,
// two workgroups per CU, where 1024 entries would leave one).  OCC, the wavefronts per SIMD of the launch bounds: five in the 128-bit class —
// two workgroups per CU where k_sssp_lds has three — (at k_sssp_lds' six the mask word and the row decoding cost ten spilled registers),
// four under REQ.
template <int NL, class Pol>
struct ReSw : Pol {
    static constexpr int SNL = NL + (Pol::REQ ? 1 : 0);
    static constexpr int RING = NL == 17 ? 256 : (Pol::REQ && NL == 4 ? 512 : 1024), ECAP = NL == 17 ? 512 : 1024;
    static constexpr int OCC = NL == 2 ? (Pol::REQ ? 4 : 5) : (NL == 4 && !Pol::REQ ? 4 : 2);
    static constexpr size_t LDS = (size_t)(RING + 1) * SNL * 8 + (size_t)ECAP * ((size_t)SNL * 8 + 4) + RS_PLAN_LDS + 64; // dynamic LDS bytes
};

// ---- the lookup ----
// The in-edge slot (contig-relative) of the explicit row of ORF k of the contig `meta` (index ci in the batch), or -1: the ORF's edge runs
// start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316), and is found among the in-edges of its head node
// by its source, as k_margins finds it.  k is within the contig's ORFs (the caller's check); u and v are checked against V here.
__device__ __forceinline__ int64_t re_orf_edge(const DBatch &b, const DMeta *meta, const uint32_t ci, const int k) {
    const DOrf o = b.orf[meta->orf_off + k];
    const int V = meta->n_node;
    const int sn = b.onode[meta->orf_off + k], tn = b.grp[meta->grp_off + o.grp].node;
    const bool fwd = o.frame > 0;
    const int u = fwd ? sn : tn, v = fwd ? tn : sn;
    if (u < 0 || v < 0 || u >= V || v >= V) return -1;
    const uint32_t *in_off = b.in_off + meta->node_off + ci;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
        if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) return (int64_t)x;
    return -1; // (no such edge: the ORF is ignored, a required one stays unmet)
}

// ---- the batch's marks ----
// A thread per ORF of a contig that is solved again, driven by the contig's mode.  A refused ORF (forb 1) sets its slot's bit in `mask` and
// nothing else: refusal wins over a bias.  A required one (forb 2, modes with REQ) sets the bit in `req` and counts for kreq, the k of §16:
// the required edges that exist.  A biased one (modes with BIAS; required or not) writes B to the slot's word, sets the bit in `bbit` and
// adds |B| to the contig's sums — in two halves, which a contig's ORFs (< 2^31) cannot overflow.  A contig whose mode has no bias reads
// nothing from `bias`, one whose mode has no required set never counts.
__global__ __launch_bounds__(NT) void k_rs_mask(DBatch b, DReann q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    const int mode = q.mode[blockIdx.x];
    if (!mode || !mg_contig(meta)) return;
    const bool has_req = re_mode_req(mode), has_bias = re_mode_bias(mode);
    const uint8_t *forb = q.forb + meta->orf_off;
    const long long *bias = q.bias + meta->orf_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        const long long B = has_bias ? bias[k] : 0ll;
        if (!(f == 1 || (f == 2 && has_req)) && B == 0) continue;
        const int64_t e = re_orf_edge(b, meta, blockIdx.x, k);
        if (e < 0) continue;
        const uint64_t x = ebase + (uint64_t)e;
        const uint32_t bit = 1u << (x & 31);
        if (f == 1) { atomicOr(&q.mask[x >> 5], bit); continue; }
        if (f == 2 && has_req) { atomicOr(&q.req[x >> 5], bit); atomicAdd(&q.kreq[blockIdx.x], 1); }
        if (B != 0) {
            const unsigned long long a = (unsigned long long)(B < 0 ? -B : B);
            q.bval[x] = B;
            atomicOr(&q.bbit[x >> 5], bit);
            atomicAdd(&q.bsum[2 * blockIdx.x], a & 0xffffffffull);
            atomicAdd(&q.bsum[2 * blockIdx.x + 1], a >> 32);
        }
    }
}

// ---- the views ----
template <class Pol>
struct BatchView {
    static_assert(!Pol::BLIST, "the batch keeps a word per in-edge slot, no list");
    const DReann &q;
    DMeta *meta;
    uint32_t ci;
    __device__ __forceinline__ BatchView(DBatch &b, const DReann &q_) : q(q_), meta(&b.meta[blockIdx.x]), ci(blockIdx.x) {}
    __device__ __forceinline__ bool mine() const { return q.mode[blockIdx.x] == Pol::MODE; }
    __device__ __forceinline__ void load_bias() {}
    __device__ __forceinline__ const uint32_t *mask() const { return q.mask; }
    __device__ __forceinline__ uint8_t *gplan() const { return q.gplan; }
    __device__ __forceinline__ const uint32_t *req() const { return Pol::REQ ? q.req : nullptr; }
    __device__ __forceinline__ int kreq() const { return Pol::REQ ? q.kreq[blockIdx.x] : 0; }
    __device__ __forceinline__ const uint32_t *bbit() const { return Pol::BIAS ? q.bbit : nullptr; }
    __device__ __forceinline__ const long long *bval() const { return Pol::BIAS ? q.bval : nullptr; }
    __device__ __forceinline__ int nbl() const { return 0; }
    __device__ __forceinline__ double bsum() const { return (double)q.bsum[2 * blockIdx.x + 1] * 4294967296.0 + (double)q.bsum[2 * blockIdx.x]; }
};

// The slot's view of the batch.  Its kernels are entered with the slot's contig as their contig index (`ci`: the in_off row, the gap table
// and the global plan slice hang on it); the graph arrays are the run's, read only and shared by all slots of a contig; the per-contig record
// is the slot's own copy (DScen.meta), and the output pointers of the by-value DBatch are moved to where the contig's `node_off` lands on the
// slot's slices of dist / parent / path — what reann_batch does for the re-annotation as a whole, per slot.  Bitmap and plan pointers are
// shifted the same way (bit edge_off + e, byte node_off / 32 + ci).  Returns the slot's record; *mask and *gplan are what lds_sweep /
// inorder_contig index with edge_off + e and node_off / 32 + ci.
__device__ __forceinline__ DMeta *sc_view(DBatch &b, const DScen &q, uint32_t *ci, const uint32_t **mask, uint8_t **gplan) {
    const DScSlot sl = q.slot[blockIdx.x];
    DMeta *meta = &q.meta[blockIdx.x];
    const int64_t node_off = meta->node_off;
    b.dist = q.dist + (sl.dist0 - node_off * b.dist_stride);
    b.parent = q.parent + (sl.node0 - node_off);
    b.path = q.path + (sl.node0 - node_off);
    *ci = (uint32_t)sl.contig;
    *mask = q.mask + (sl.mask0 - (meta->edge_off >> 5));
    *gplan = q.gplan + (sl.plan0 - (node_off >> 5) - (int64_t)sl.contig);
    return meta;
}
// the slot's required slice and its bias slice, shifted by sc_view's rule
__device__ __forceinline__ const uint32_t *scp_req(const DScen &q, const DMeta *meta) { return q.req + (q.req0[blockIdx.x] - (meta->edge_off >> 5)); }
__device__ __forceinline__ const uint32_t *sce_bbit(const DScen &q, const DScBias &bs, const DMeta *meta) { return q.bbit + (bs.bbit0 - (meta->edge_off >> 5)); }
// pairs a biased slot's list holds: what k_sce_mask appended, never beyond the list
__device__ __forceinline__ int sce_count(const DScBias &bs) { return bs.cnt < bs.n_trip ? bs.cnt : bs.n_trip; }

// blockIdx.x is a slot of the range the launcher hands over (plain, pinned, biased or both: phx_kernels.hip, scen_range), whose policy is Pol
template <class Pol>
struct SlotView {
    static_assert(!Pol::BIAS || Pol::BLIST, "a biased slot keeps a list, no word per in-edge slot");
    const DScen &q;
    DMeta *meta;
    uint32_t ci;
    const uint32_t *mask_;
    uint8_t *gplan_;
    DScBias bs; // (biased slots, once load_bias has run)
    __device__ __forceinline__ SlotView(DBatch &b, const DScen &q_) : q(q_) { meta = sc_view(b, q, &ci, &mask_, &gplan_); }
    __device__ __forceinline__ bool mine() const { return true; }
    __device__ __forceinline__ void load_bias() { if constexpr (Pol::BIAS) bs = q.bs[blockIdx.x]; }
    __device__ __forceinline__ const uint32_t *mask() const { return mask_; }
    __device__ __forceinline__ uint8_t *gplan() const { return gplan_; }
    __device__ __forceinline__ const uint32_t *req() const { return Pol::REQ ? scp_req(q, meta) : nullptr; }
    __device__ __forceinline__ int kreq() const { return Pol::REQ ? q.kreq[blockIdx.x] : 0; }
    __device__ __forceinline__ const uint32_t *bbit() const { return Pol::BIAS ? sce_bbit(q, bs, meta) : nullptr; }
    __device__ __forceinline__ const long long *bval() const { return Pol::BIAS ? q.blist + 2 * bs.list0 : nullptr; }
    __device__ __forceinline__ int nbl() const { return Pol::BIAS ? sce_count(bs) : 0; }
    __device__ __forceinline__ double bsum() const { return (double)bs.bsum[1] * 4294967296.0 + (double)bs.bsum[0]; }
};

// ---- the solvers ----
// The two steps of a solve, written out per view: through a function of their own the kernels came out with other instructions than they
// had (as at bias_at in phx_inorder.inc), so the shared text is a macro.  V: the view.  NL: the contig's class; the sweep and the parent rule
// run on one limb more under REQ.  (No `overflow` test: the totals are the re-annotation's own, zeroed per call.)
#define RE_SWEEP(V) \
    DMeta *meta = (V).meta; \
    const int n_node = meta->n_node; \
    if (!(V).mine() || !mg_contig(meta) || meta->sssp_nl != NL) return; \
    if constexpr (Pol::BIAS) { \
        /* the limb test before a biased sweep: the layout's bound plus the sum of |B| must fit the contig's own class.  Beyond it there is no */ \
        /* promotion, the contig ends before its sweep — and under REQ M = 2^(64 NL) then exceeds every sum of W + B, so the top limb stays */ \
        /* the count of required edges */ \
        (V).load_bias(); \
        if (contig_sum_bits(b, meta, (V).bsum()) > 64 * NL) { \
            __syncthreads(); /* (every thread has read the status) */ \
            if (threadIdx.x == 0) { meta->status = PHX_S_OVERFLOW; meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0; } \
            return; \
        } \
    } \
    lds_sweep<ReSw<NL, Pol>::SNL, ReSw<NL, Pol>>(b, meta, (V).ci, n_node, (V).mask(), (V).gplan(), (V).req(), (V).kreq(), (V).bbit(), (V).bval(), (V).nbl())
#define RE_INORDER(V) \
    __shared__ IoShared<IO_T> sh; \
    DMeta *meta = (V).meta; \
    if (!(V).mine() || meta->sssp_nl != NL) return; \
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; } \
    __syncthreads(); \
    if (!mg_contig(meta)) return; /* (a cycle of negative length, or the biased bound beyond the class: the solver has set the status) */ \
    if (meta->n_path < 2 && meta->n_path != -1) return; /* no path; -1: the walk along the lowest-index parents cycled */ \
    (V).load_bias(); \
    inorder_contig<ReSw<NL, Pol>::SNL, IO_T, Pol>(b, meta, (V).ci, &sh, (V).mask(), (V).req(), (V).bbit(), (V).bval(), (V).nbl())

// the batch: a workgroup per contig, the contigs whose mode is the policy's
template <int NL, class Pol>
__global__ __launch_bounds__(SW_THREADS, (ReSw<NL, Pol>::OCC)) void k_rs_lds(DBatch b, DReann q) {
    BatchView<Pol> v(b, q);
    RE_SWEEP(v);
}
template <int NL, int IO_T, class Pol>
__global__ __launch_bounds__(IO_T) void k_rs_inorder(DBatch b, DReann q) {
    BatchView<Pol> v(b, q);
    RE_INORDER(v);
}
// the scenario slots (§17, §18, §20, §27): a workgroup per slot of the range
template <int NL, class Pol>
__global__ __launch_bounds__(SW_THREADS, (ReSw<NL, Pol>::OCC)) void k_sc_lds(DBatch b, DScen q) {
    SlotView<Pol> v(b, q);
    RE_SWEEP(v);
}
template <int NL, int IO_T, class Pol>
__global__ __launch_bounds__(IO_T) void k_sc_inorder(DBatch b, DScen q) {
    SlotView<Pol> v(b, q);
    RE_INORDER(v);
}
#undef RE_SWEEP
#undef RE_INORDER

// ---- the record ----
// the count of required edges on the best path: the top limb of the NL + 1 limbs at df
template <int NL>
__device__ int64_t rc_count(const uint64_t *df) { return rq_count<NL + 1>(wi_load<NL + 1>(df)); }

// float(D' - D) / 1000.0 as §11-12 round it; it may be negative under a bias: wi_to_double_rn rounds the magnitude to nearest-even and puts
// the sign back, which is what float() of a negative python integer does
template <int NL>
__device__ double rs_delta(const uint64_t *df, const uint64_t *d0) {
    const WInt<NL> DF = wi_load<NL>(df), D = wi_load<NL>(d0);
    return wi_to_double_rn<NL>(wi_add<NL>(DF, wi_neg<NL>(D))) / 1000.0;
}

// What the host reads of one solve.  dist: the solve's distances of the contig's node 0 — the contig's limbs per node, and one limb more
// when the solve had a required set (the W-sum, with any B, is then the low nl limbs and the top limb the count); dist0: the run's.
// nreq: the required ORFs of the solve (|R|), or null: no required set.
__device__ __forceinline__ DReannRec re_record(const DMeta *meta, const uint64_t *dist, const uint64_t *dist0, const int32_t *nreq) {
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = nreq ? *nreq : 0; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const uint64_t *df = dist + (size_t)(V - 1) * (nl + (nreq ? 1 : 0)); // the target's distance
        const uint64_t *d0 = dist0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        if (nreq) r.unmet -= (int32_t)(nl == 2 ? rc_count<2>(df) : nl == 4 ? rc_count<4>(df) : nl == 8 ? rc_count<8>(df) : rc_count<17>(df));
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    return r;
}

// a thread per contig: every contig solved again, whatever its mode
__global__ __launch_bounds__(64) void k_rs_fin(DBatch b, DReann q) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= b.n_contig || !q.mode[c]) return;
    const DMeta *meta = &b.meta[c];
    q.rec[c] = re_record(meta, b.dist + (size_t)meta->node_off * b.dist_stride, q.dist0 + (size_t)meta->node_off * q.stride0, re_mode_req(q.mode[c]) ? &q.nreq[c] : nullptr);
}

// a thread per slot of the whole table: plain, pinned, biased or both
__global__ __launch_bounds__(64) void k_sc_fin(DBatch b, DScen q) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= q.n_slot) return;
    const DMeta *meta = &q.meta[s];
    q.rec[s] = re_record(meta, q.dist + q.slot[s].dist0, q.dist0 + (size_t)meta->node_off * q.stride0, q.slot[s].pinned ? &q.nreq[s] : nullptr);
}

// ---- the slots' marks (DESIGN.md §17, §18, §20, §27) ----
// A chunk's slot table holds the plain slots, then the pinned ones (required ORFs, solved under REQ: n_node x (NL + 1) words of distances
// and a required slice, DScen.req at req0), then the biased ones (solved under BIAS with BLIST), then the ones that are both (pinned = 1 AND
// a DScBias: everything a pinned and everything a biased slot owns, solved under REQ with BIAS and BLIST).  A biased slot keeps no word per in-edge
// slot (a dense slice would be 8 E bytes, more than everything else the slot owns): it has a bias bitmap slice (DScen.bbit at DScBias.bbit0)
// and a list of (in-edge slot of the batch, B) pairs sorted by in-edge slot, which the shared code searches where the slot's bit is set
// (bias_at under BLIST, phx_sssp.inc).  The three mask kernels below get the whole table, so a "both" slot is marked by all three (a pair's or a triple's slot is its index in it);
// a slot's refused slice is set by k_sc_mask whatever its range.  Gene records come from the chunk's shared counter as in §14; the tie
// scratch from the chunk's bump allocator (DTotals.tie_need).

// a thread block per slot: the slot's copy of its contig's record, as the run left it
__global__ __launch_bounds__(64) void k_sc_meta(DBatch b, DScen q) {
    const int s = (int)blockIdx.x;
    const int c = q.slot[s].contig;
    if (c < 0 || c >= b.n_contig) return; // (the host has checked it)
    const uint64_t *from = (const uint64_t *)&b.meta[c];
    uint64_t *to = (uint64_t *)&q.meta[s];
    static_assert(sizeof(DMeta) % 8 == 0, "DMeta is copied in 64-bit words");
    for (int k = (int)threadIdx.x; k < (int)(sizeof(DMeta) / 8); k += 64) to[k] = from[k];
}

// Slot s of the table and ORF k of its contig's device order: the slot, its contig's record as the run left it, and the bit of the ORF's
// edge in a slice of the slot's — a slice keeps edge_off's position in a word, so in-edge slot x is bit (edge_off & 31) + x.  bit < 0:
// nothing to mark (an index out of range — the host has checked them —, a contig without a graph, an ORF without an edge).
struct ScMark { DScSlot sl; const DMeta *meta; int64_t x, bit; };
__device__ __forceinline__ ScMark sc_orf(const DBatch &b, const DScen &q, const int s, const int k) {
    ScMark m;
    m.meta = nullptr; m.x = m.bit = -1;
    if (s < 0 || s >= q.n_slot) return m;
    m.sl = q.slot[s];
    if (m.sl.contig < 0 || m.sl.contig >= b.n_contig) return m;
    m.meta = &b.meta[m.sl.contig];
    if (!mg_contig(m.meta) || k < 0 || k >= m.meta->n_orf) return m;
    m.x = re_orf_edge(b, m.meta, (uint32_t)m.sl.contig, k);
    if (m.x >= 0) m.bit = (int64_t)((uint64_t)m.meta->edge_off & 31u) + m.x;
    return m;
}

// a thread per listed (slot, ORF) pair: the ORF's edge sets its bit in the slot's refused slice
__global__ __launch_bounds__(NT) void k_sc_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_pair) return;
    const int2 pr = q.pair[p];
    const ScMark m = sc_orf(b, q, pr.x, pr.y);
    if (m.bit < 0) return;
    atomicOr(&q.mask[m.sl.mask0 + (m.bit >> 5)], 1u << (m.bit & 31));
}

// a thread per required (slot, ORF) pair: the ORF's edge sets its bit in the slot's required slice and counts for the slot's kreq, the k
// of the solver's cycle guard (an ORF without an edge stays unmet)
__global__ __launch_bounds__(NT) void k_scp_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_rpair) return;
    const int2 pr = q.rpair[p];
    const ScMark m = sc_orf(b, q, pr.x, pr.y);
    if (m.bit < 0 || !m.sl.pinned) return;
    const uint32_t bit = 1u << (m.bit & 31);
    if (!(atomicOr(&q.req[q.req0[pr.x] + (m.bit >> 5)], bit) & bit)) atomicAdd(&q.kreq[pr.x], 1); // (an ORF listed twice counts once)
}

// a thread per (slot, ORF, B) triple: the ORF's edge sets its bit in the slot's bias slice, appends (in-edge slot, B) to the slot's list
// and adds |B| to the slot's sums as k_rs_mask does.  A slot with one triple needs no sorting and appends to its list proper, any other
// to its staging area.
__global__ __launch_bounds__(NT) void k_sce_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_trip) return;
    const DScTrip tr = q.trip[p];
    const ScMark m = sc_orf(b, q, tr.slot, tr.orf);
    if (m.bit < 0) return;
    DScBias *bs = &q.bs[tr.slot];
    const int at = atomicAdd(&bs->cnt, 1);
    if (at >= bs->n_trip) return; // (the host sized the list by the slot's triples)
    atomicOr(&q.bbit[bs->bbit0 + (m.bit >> 5)], 1u << (m.bit & 31));
    long long *to = (bs->n_trip == 1 ? q.blist : q.bstage) + 2 * (bs->list0 + at);
    to[0] = (long long)((uint64_t)m.meta->edge_off + (uint64_t)m.x); to[1] = tr.B; // (the batch's in-edge slot, as the shared code counts them)
    const unsigned long long a = (unsigned long long)(tr.B < 0 ? -tr.B : tr.B);
    atomicAdd(&bs->bsum[0], a & 0xffffffffull);
    atomicAdd(&bs->bsum[1], a >> 32);
}

// the staged pairs of a biased slot into its list in ascending order of their in-edge slot.  A pair's place is the number of pairs in
// front of it (an equal in-edge slot: the one staged earlier), found by counting — a list is at most a contig's ORFs.  gridDim.y
// workgroups share a slot's pairs, NT at a time; the keys they count over pass through LDS in tiles of NT.  q: the biased range with the
// "both" range directly behind it (one launch sorts the lists of either).
__global__ __launch_bounds__(NT) void k_sce_sort(DScen q) {
    __shared__ long long s_key[NT];
    const DScBias bs = q.bs[blockIdx.x];
    if (bs.n_trip <= 1) return; // (k_sce_mask wrote the list itself)
    const int n = sce_count(bs);
    const int tid = (int)threadIdx.x;
    const long long *from = q.bstage + 2 * bs.list0;
    long long *to = q.blist + 2 * bs.list0;
    for (int i0 = (int)blockIdx.y * NT; i0 < n; i0 += (int)gridDim.y * NT) { // (i0, n: the same in every thread, so are the barriers)
        const int i = i0 + tid;
        const long long key = i < n ? from[2 * i] : 0ll;
        int at = 0;
        for (int j0 = 0; j0 < n; j0 += NT) {
            __syncthreads();
            if (j0 + tid < n) s_key[tid] = from[2 * (j0 + tid)];
            __syncthreads();
            const int m = n - j0 < NT ? n - j0 : NT;
            for (int j = 0; j < m; j++) { const long long kj = s_key[j]; at += kj < key || (kj == key && j0 + j < i); }
        }
        if (i < n) { to[2 * at] = key; to[2 * at + 1] = from[2 * i + 1]; }
    }
}
