// phx_drop.inc — gene drop margins: the exact cost of removing each called gene (included by phx_kernels.hip, after phx_margins.inc).
// ------------------------------------------------------------------------------------------------
// On demand after a run and after the margins' shared part (out-edge CSR, d_t: phx_margins.inc), never inside a run.  For one contig with
// the device path P = p_0 (source) ... p_K (target), D = d_s(target), and a CDS gene of P whose stop node is p_j (p_{j+1} of a forward gene
// start -> stop, p_j of a reverse gene stop -> start), D_{-g} is the shortest source -> target distance in G without p_j; the record carries
// float(D_{-g} - D) / 1000 (DESIGN.md §12).
//
//   1. k_dp_tree: two shortest-path trees that contain P — T_s (lowest-index tight in-edge) and T_t (tight out-edge to the smallest head id) —
//      and the labels first(x) (index of the P node x's T_s chain leaves P at) and last(z) (index of the P node z's T_t chain joins P at),
//      by pointer doubling; a chain that does not reach P (tight edges closing a zero-length cycle) rebuilds that tree layer by layer.
//   2. k_dp_cand: every edge x -> z with first(x) + 1 <= last(z) - 1 bounds the slots between them by d_s(x) + W + d_t(z) - D: range
//      minimum by a two-entry sparse table (64-bit atomicMin, saturated at 2^63), pushed down level by level.
//   3. k_dp_rescan: a gene slot whose minimum saturated is recomputed exactly, one wavefront over the candidates that cover it.
//   4. k_dp_cross: the nodes y with last(y) <= j <= first(y) (they lie on a cycle through p_j): Bellman-Ford inside that set, seeded from the
//      edges x -> y with first(x) < j, leaving by edges y -> z with last(z) > j.
//   5. k_dp_rec: one record per gene pair of P.
// Widths: d_s, d_t, |W| and D are each below B (|B| < 2^(64 NL - 5), DESIGN.md §11), so a candidate of step 3 is below 4B in magnitude; a
// settled delta of step 4 is a seed d_s(x) + W plus a simple path inside Y_j (below 3B), its candidates below 6B: the contig's own NL limbs
// hold every value in two's complement.

#define DP_SAT (1ull << 63)      // a range minimum >= 2^63: recomputed exactly (k_dp_rescan)
#define DP_NONE (~0ull)          // no candidate covers the slot
#define DP_CROSS_LDS 64          // cross nodes whose two delta buffers live in LDS; beyond: DDrop.da / db

// the contigs the pass covers: device distances, a settled reverse pass, a path with at least one pair
__device__ __forceinline__ bool dp_contig(const DBatch &b, const DMarg &g, const DMeta *meta) {
    return mg_contig(meta) && !g.mstat[meta - b.meta] && meta->n_path >= 3;
}

// pair i of P (path[2i+1] -> path[2i+2], the genes of file_handling.pairwise): a CDS gene?  *j its stop node's index on P, *k its ORF
__device__ __forceinline__ bool dp_gene(const DBatch &b, const DMeta *meta, const int32_t *path, int i, int *j, int *k) {
    const DNode *nd = b.node + meta->node_off;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int a = path[2 * i + 1], bb = path[2 * i + 2];
    const int ta = NTYPE(nd[a].info), fr = NFRAME(nd[a].info);
    if (ta == 0 && fr > 0 && fr <= 3 && LINK_KIND(nd[a].link) == LINK_START) {
        const int o = (int)LINK_IDX(nd[a].link);
        if (grp[orf[o].grp].node == bb) { *j = 2 * i + 2; *k = o; return true; }
    } else if (ta == 1 && fr < 0 && fr >= -3 && LINK_KIND(nd[bb].link) == LINK_START) {
        const int o = (int)LINK_IDX(nd[bb].link);
        if (grp[orf[o].grp].node == a) { *j = 2 * i + 1; *k = o; return true; }
    }
    return false;
}

template <int W>
__device__ __forceinline__ WInt<W> wi_from_u64(uint64_t x) {
    WInt<W> r;
    r.v[0] = x;
#pragma unroll
    for (int i = 1; i < W; i++) r.v[i] = 0;
    return r;
}
// a non-negative candidate as a 64-bit key: itself below 2^63, else DP_SAT
template <int W>
__device__ __forceinline__ uint64_t wi_sat64(const WInt<W> &x) {
    bool big = (x.v[0] >> 63) != 0;
#pragma unroll
    for (int i = 1; i < W; i++) big = big || x.v[i] != 0;
    return big ? DP_SAT : x.v[0];
}
// minimum over the 64 lanes of a wavefront (every lane gets it)
template <int W>
__device__ __forceinline__ WInt<W> wave_min(WInt<W> x) {
    for (int m = 32; m >= 1; m >>= 1) {
        WInt<W> y;
#pragma unroll
        for (int i = 0; i < W; i++) y.v[i] = (uint64_t)__shfl_xor((unsigned long long)x.v[i], m);
        if (wi_lt<W>(y, x)) x = y;
    }
    return x;
}
__device__ __forceinline__ uint64_t ld_l2(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The policy of the five kernels is the type of their second argument, as for k_sssp_rev and k_margins (phx_margins.inc).  DMarg: the run's
// graph and path, the kernels as §12 describes them.  MgDrop (the re-annotation drop margins, DESIGN.md §29): MgCond — the graph G' = G_{F,B}
// of the last re-annotation — and the re-annotation's device path P' (MgCond has every other input; the path is the one pointer it lacks, and
// a field added to DRmarg or DDrop would move the argument blocks of kernels that exist).  Everything the policy adds sits behind
// if constexpr (mg_cond<G>): the DMarg instantiations are the code they were without it.  Under MgDrop
//   the path is g.path, its length DReannRec.n_path; d_s' comes from DRmarg.ds (ds_stride words per node reserved), d_t' from DRmarg.dist_t,
//   D' = d_s'(target); the contigs are those with DRmarg.sel == 1 whose conditioned reverse pass settled;
//   a node outside R (d_s' unreached) has no d_t' either — k_sssp_rev<NL, MgCond> never relaxes it — so it gets no label, no candidate,
//   no place among the cross nodes: the values are those of G'[R];
//   in-edge slot e (bit edge_off + e) is skipped where it is set in DReann.mask and weighs W + DReann.bval where it is set in DReann.bbit
//   (read for a contig solved under the bias policy only: no call clears that bitmap before one biases a contig); out-edge position e is
//   treated likewise through DRmarg.fbit / bbit / bval.  As in k_sssp_rev, the bitmaps are read per edge only for a node whose edge range
//   shares a bitmap word with a refused or biased slot (`special`): a re-annotation's are a handful per contig.
struct MgDrop : MgCond { const int32_t *path; };
// MgPinDrop (the pinned drop margins, DESIGN.md §32): MgPin — a contig solved under the required policy (DReann.mode 2 or 4) — with the
// re-annotation's device path and the place of `lost`, the two pointers MgPin lacks (no struct that exists grows).  It is a policy of its
// own with a trait of its own: mg_pin<G> keeps meaning MgPin, and mg_cond<G> holds, so everything MgDrop adds applies.  What dp_pin<G> adds:
//   a value has WL = NL + 1 limbs in all five kernels, the top limb minus the count of required edges (§16); d_s' comes from DPmarg.ds with
//   NL + 1 limbs per node used, d_t' from DPmarg.dist_t at DPmarg.dt_stride words per node reserved;
//   an in-edge slot set in DReann.req / an out-edge position set in DPmarg.rbit weighs W + B - M, M = 2^(64 NL): one off the top limb.  The
//   req / rbit words are part of the per-node `special` test, so nearly every node keeps the plain loops;
//   DDrop.sx / cx are indexed at DPmarg.dt_stride words per record and DDrop.da / db per node (dp_stride; the host sizes the set so);
//   k_dp_rec decodes Delta = lost * M + s as k_margins<NL, MgPin> decodes Delta'': lost to MgPinDrop.lost (parallel to DDrop.rec), drop =
//   float(s) / 1000.0 with s the low NL limbs as the class's two's complement (negative where lost > 0 and the low part went down).
// wi_sat64 saturates whenever a limb above the first is non-zero, so every candidate with lost > 0 — and every one with lost = 0 and
// s >= 2^63 — is DP_SAT in the sparse table, and a candidate that is not saturated has lost = 0 and s < 2^63: it is below each of them in
// the (lost, s) order as well.  A slot whose minimum is not DP_SAT therefore holds its exact minimum; one that is DP_SAT is recomputed by
// k_dp_rescan in WL limbs, where two's-complement order on lost * M + s is the lexicographic order.
struct MgPinDrop : MgPin { const int32_t *path; int32_t *lost; };
struct MgPinProf; // (the pinned profiles' policy, phx_profile.inc: MgPin with pointers of its own; what dp_pin<G> adds below holds for it as well)
template <class G> constexpr bool dp_pin = std::is_same<G, MgPinDrop>::value || std::is_same<G, MgPinProf>::value;
template <int NL, class G> constexpr int dp_wl = NL + (dp_pin<G> ? 1 : 0); // limbs of a value
template <class G>
__device__ __forceinline__ bool dp_on(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (mg_cond<G>) { const int i = (int)(meta - b.meta); return g.r.sel[i] == 1 && mg_contig(meta) && !g.r.mstat[i] && g.q.rec[i].n_path >= 3; }
    else return dp_contig(b, g, meta);
}
template <class G>
__device__ __forceinline__ int dp_npath(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (mg_cond<G>) return g.q.rec[meta - b.meta].n_path;
    else return meta->n_path;
}
template <class G>
__device__ __forceinline__ const int32_t *dp_path(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (mg_cond<G>) return g.path + meta->node_off;
    else return b.path + meta->node_off;
}
template <class G>
__device__ __forceinline__ const uint64_t *dp_ds(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (mg_cond<G>) return g.r.ds + (size_t)meta->node_off * g.r.ds_stride;
    else return b.dist + (size_t)meta->node_off * b.dist_stride;
}
template <class G>
__device__ __forceinline__ const uint64_t *dp_dt(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (dp_pin<G>) return g.r.dist_t + (size_t)meta->node_off * g.r.dt_stride;
    else if constexpr (mg_cond<G>) return g.r.dist_t + (size_t)meta->node_off * b.dist_stride;
    else return g.dist_t + (size_t)meta->node_off * b.dist_stride;
}
// words reserved per record of DDrop.sx / cx and per node of DDrop.da / db
template <class G>
__device__ __forceinline__ size_t dp_stride(const DBatch &b, const G &g) {
    if constexpr (dp_pin<G>) return (size_t)g.r.dt_stride;
    else return (size_t)b.dist_stride;
}
// `special` of a node's in-edge slots / out-edge positions [e0, e1) (MgDrop and MgPinDrop only)
template <class G>
__device__ __forceinline__ bool dp_sp_in(const G &g, bool biased, uint64_t ebase, uint32_t e0, uint32_t e1) {
    bool sp = false;
    if (e1 > e0)
        for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) sp = sp || (g.q.mask[x] | (biased ? g.q.bbit[x] : 0u)) != 0u;
    if constexpr (dp_pin<G>) { // (the required slots are a handful as well: the same test covers them)
        if (e1 > e0)
            for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) sp = sp || g.q.req[x] != 0u;
    }
    return sp;
}
template <class G>
__device__ __forceinline__ bool dp_sp_out(const G &g, uint64_t ebase, uint32_t e0, uint32_t e1) {
    bool sp = false;
    if (e1 > e0)
        for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) sp = sp || (g.r.fbit[x] | g.r.bbit[x]) != 0u;
    if constexpr (dp_pin<G>) {
        if (e1 > e0)
            for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) sp = sp || g.r.rbit[x] != 0u;
    }
    return sp;
}
// W' of in-edge slot x / out-edge position x of the batch, given W (the caller has skipped a refused one); under DMarg: W.  A call stands
// where the weight stood, so that the DMarg code keeps its order of loads.
template <int W, class G>
__device__ __forceinline__ WInt<W> dp_w_in(const G &g, bool sp, bool biased, uint64_t x, WInt<W> w) {
    if constexpr (mg_cond<G>) { if (sp && biased && mg_bit(g.q.bbit, x)) w = wi_add<W>(w, ew_decode<W>(g.q.bval[x])); }
    if constexpr (dp_pin<G>) { if (sp && mg_bit(g.q.req, x)) w.v[W - 1] -= 1ull; } // required: W' = W + B - M, one off the top limb
    return w;
}
template <int W, class G>
__device__ __forceinline__ WInt<W> dp_w_out(const G &g, bool sp, uint64_t x, WInt<W> w) {
    if constexpr (mg_cond<G>) { if (sp && mg_bit(g.r.bbit, x)) w = wi_add<W>(w, ew_decode<W>(g.r.bval[x])); }
    if constexpr (dp_pin<G>) { if (sp && mg_bit(g.r.rbit, x)) w.v[W - 1] -= 1ull; }
    return w;
}

// ---- 1. k_dp_tree<NL>: trees and labels, one workgroup per contig ----
// DDrop.js / jt: the jump pointers (a node on P points at itself; -1: unreached), then first / last.  DDrop.ps / ts, when not null,
// keep the one-hop parents / successors the labels were built from (the layered build: the node a node joined through).  The doubling
// reads and writes js in place: a value read mid-round is a later ancestor on the same chain, so the rounds only get shorter.
// ceil(log2 V) + 1 rounds reach P from any chain that reaches it at all; a node whose pointer is then still off P sits on a tight
// zero-length cycle of the chosen parents, and the tree is rebuilt by layers: round r lets a node join through a tight edge to a node that joined before round r (P itself is layer 0),
// which cannot close a cycle.  DDrop.layered forces the layered build (env PHX_DROP_LAYERED, the tests).
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_dp_tree(DBatch b, G g, DDrop q) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    __shared__ int s_fail[2], s_chg;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, n = dp_npath<G>(b, g, meta), tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint32_t *oo = g.out_off + no + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const long long *ow = g.out_w + meta->edge_off;
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    int32_t *pidx = q.pidx + no, *js = q.js + no, *jt = q.jt + no, *first = q.first + no, *last = q.last + no;
    for (int v = tid; v < V; v += NT) pidx[v] = -1;
    if (tid < 2) s_fail[tid] = q.layered;
    __syncthreads();
    for (int j = tid; j < n; j += NT) pidx[path[j]] = j;
    __syncthreads();
    // parents / successors
    for (int v = tid; v < V; v += NT) {
        int ps = -1, ts = -1;
        if (pidx[v] >= 0) ps = ts = v;
        else {
            const WInt<WL> dv = wi_load<WL>(ds + (size_t)v * WL);
            if (!wi_unreached<WL>(dv)) {
                ps = -2; // (a reached node without a tight in-edge cannot occur: the layered build then leaves it out)
                [[maybe_unused]] bool sp = false;
                if constexpr (COND) sp = dp_sp_in(g, biased, ebase, in_off[v], in_off[v + 1]);
                for (uint32_t e = in_off[v], e1 = in_off[v + 1]; e < e1; e++) {
                    const uint32_t sw = esrc[e];
                    if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                    const WInt<WL> du = wi_load<WL>(ds + (size_t)ESRC_NODE(sw) * WL);
                    if (!wi_unreached<WL>(du) && wi_eq<WL>(wi_add<WL>(du, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), dv)) { ps = (int)ESRC_NODE(sw); break; }
                }
            }
            const WInt<WL> tv = wi_load<WL>(dt + (size_t)v * WL);
            if (!wi_unreached<WL>(tv)) {
                ts = -2;
                [[maybe_unused]] bool sp = false;
                if constexpr (COND) sp = dp_sp_out(g, ebase, oo[v], oo[v + 1]);
                for (uint32_t e = oo[v], e1 = oo[v + 1]; e < e1; e++) {
                    const int z = (int)od[e];
                    if (ts >= 0 && z >= ts) continue;
                    if constexpr (COND) { if (sp && mg_bit(g.r.fbit, ebase + e)) continue; }
                    const WInt<WL> tz = wi_load<WL>(dt + (size_t)z * WL);
                    if (!wi_unreached<WL>(tz) && wi_eq<WL>(wi_add<WL>(tz, dp_w_out<WL>(g, sp, ebase + e, ew_decode<WL>(ow[e]))), tv)) ts = z;
                }
            }
        }
        js[v] = ps; jt[v] = ts;
        if (q.ps) { q.ps[no + v] = ps; q.ts[no + v] = ts; } // (the replacements' one-hop trees, §13)
        if (ps == -2) s_fail[0] = 1;
        if (ts == -2) s_fail[1] = 1;
    }
    __syncthreads();
    int rounds = 1;
    for (int x = V; x > 1; x = (x + 1) >> 1) rounds++;
    for (int r = 0; r < rounds; r++) {
        for (int v = tid; v < V; v += NT) {
            const int a = js[v], c = jt[v];
            if (a >= 0 && pidx[a] < 0) js[v] = js[a];
            if (c >= 0 && pidx[c] < 0) jt[v] = jt[c];
        }
        __syncthreads();
    }
    for (int v = tid; v < V; v += NT) {
        const int a = js[v], c = jt[v];
        if (a == -2 || (a >= 0 && pidx[a] < 0)) s_fail[0] = 1;
        if (c == -2 || (c >= 0 && pidx[c] < 0)) s_fail[1] = 1;
        first[v] = a >= 0 ? pidx[a] : -1;
        last[v] = c >= 0 ? pidx[c] : -1;
    }
    __syncthreads();
    const bool fs = s_fail[0] != 0, ft = s_fail[1] != 0;
    if (!fs && !ft) return;
    if (tid == 0) atomicAdd(&q.stats[3], 1ull);
    // layered rebuild of the tree(s) that failed: js / jt now hold the layer a node joined in (0: P; INT_MAX: not yet, or unreached)
    for (int v = tid; v < V; v += NT) {
        if (fs) { js[v] = pidx[v] >= 0 ? 0 : 0x7fffffff; if (pidx[v] < 0) first[v] = -1; }
        if (ft) { jt[v] = pidx[v] >= 0 ? 0 : 0x7fffffff; if (pidx[v] < 0) last[v] = -1; }
    }
    __syncthreads();
    for (int r = 1; r <= V + 1; r++) {
        if (tid == 0) s_chg = 0;
        __syncthreads();
        for (int v = tid; v < V; v += NT) {
            if (fs && js[v] == 0x7fffffff) {
                const WInt<WL> dv = wi_load<WL>(ds + (size_t)v * WL);
                [[maybe_unused]] bool sp = false;
                if constexpr (COND) { if (!wi_unreached<WL>(dv)) sp = dp_sp_in(g, biased, ebase, in_off[v], in_off[v + 1]); }
                if (!wi_unreached<WL>(dv))
                    for (uint32_t e = in_off[v], e1 = in_off[v + 1]; e < e1; e++) {
                        const uint32_t sw = esrc[e];
                        const int u = (int)ESRC_NODE(sw);
                        if (js[u] >= r) continue;
                        if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                        const WInt<WL> du = wi_load<WL>(ds + (size_t)u * WL);
                        if (!wi_unreached<WL>(du) && wi_eq<WL>(wi_add<WL>(du, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), dv)) {
                            first[v] = first[u]; js[v] = r; s_chg = 1;
                            if (q.ps) q.ps[no + v] = u;
                            break;
                        }
                    }
            }
            if (ft && jt[v] == 0x7fffffff) {
                const WInt<WL> tv = wi_load<WL>(dt + (size_t)v * WL);
                if (!wi_unreached<WL>(tv)) {
                    int best = -1;
                    [[maybe_unused]] bool sp = false;
                    if constexpr (COND) sp = dp_sp_out(g, ebase, oo[v], oo[v + 1]);
                    for (uint32_t e = oo[v], e1 = oo[v + 1]; e < e1; e++) {
                        const int z = (int)od[e];
                        if ((best >= 0 && z >= best) || jt[z] >= r) continue;
                        if constexpr (COND) { if (sp && mg_bit(g.r.fbit, ebase + e)) continue; }
                        const WInt<WL> tz = wi_load<WL>(dt + (size_t)z * WL);
                        if (!wi_unreached<WL>(tz) && wi_eq<WL>(wi_add<WL>(tz, dp_w_out<WL>(g, sp, ebase + e, ew_decode<WL>(ow[e]))), tv)) best = z;
                    }
                    if (best >= 0) { last[v] = last[best]; jt[v] = r; s_chg = 1; if (q.ts) q.ts[no + v] = best; }
                }
            }
        }
        __syncthreads();
        if (!s_chg) break;
        __syncthreads();
    }
}

// ---- 2. k_dp_cand<NL>: candidates and the sparse table, one workgroup per contig ----
// Level k holds n entries; entry i covers slots [i, i + 2^k).  A candidate for the open range (first(x), last(z)) = slots [a, z] goes to
// level floor(log2(z - a + 1)) at both ends.  The push-down gathers: level k-1 entry i takes the minimum of level k at i and at i - 2^(k-1).
// The atomics stay per contig: in LDS up to DP_TAB_LDS entries, else in the contig's own slice of DDrop.gtab (read back through L2).
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_dp_cand(DBatch b, G g, DDrop q) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    __shared__ unsigned long long s_tab[DP_TAB_LDS];
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, n = dp_npath<G>(b, g, meta), tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const int32_t *first = q.first + no, *last = q.last + no;
    int lv = 1;
    while ((2 << (lv - 1)) <= n) lv++; // floor(log2 n) + 1
    const int cells = n * lv;
    unsigned long long *tab = cells <= DP_TAB_LDS ? s_tab : (unsigned long long *)(q.gtab + q.toff[blockIdx.x]);
    for (int i = tid; i < cells; i += NT) tab[i] = DP_NONE;
    __syncthreads();
    const WInt<WL> negD = wi_neg<WL>(wi_load<WL>(ds + (size_t)(V - 1) * WL));
    for (int z = tid; z < V; z += NT) {
        const int lz = last[z];
        if (lz < 2) continue; // (no slot strictly between first(x) >= 0 and last(z))
        const WInt<WL> tz = wi_add<WL>(wi_load<WL>(dt + (size_t)z * WL), negD);
        [[maybe_unused]] bool sp = false;
        if constexpr (COND) sp = dp_sp_in(g, biased, ebase, in_off[z], in_off[z + 1]);
        for (uint32_t e = in_off[z], e1 = in_off[z + 1]; e < e1; e++) {
            const uint32_t sw = esrc[e];
            const int x = (int)ESRC_NODE(sw);
            const int fx = first[x];
            if (fx < 0 || fx + 1 > lz - 1) continue;
            if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
            const int a = fx + 1, len = lz - 1 - a + 1;
            const WInt<WL> c = wi_add<WL>(wi_add<WL>(wi_load<WL>(ds + (size_t)x * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), tz);
            const unsigned long long key = wi_sat64<WL>(c);
            const int k = 31 - __clz(len);
            atomicMin(&tab[k * n + a], key);
            atomicMin(&tab[k * n + (lz - 1) - (1 << k) + 1], key);
        }
    }
    __syncthreads();
    for (int k = lv - 1; k >= 1; k--) {
        const int h = 1 << (k - 1);
        for (int i = tid; i < n; i += NT) {
            uint64_t m = ld_l2((const uint64_t *)&tab[k * n + i]);
            if (i >= h) { const uint64_t m2 = ld_l2((const uint64_t *)&tab[k * n + i - h]); m = m2 < m ? m2 : m; }
            if (m != DP_NONE) atomicMin(&tab[(k - 1) * n + i], (unsigned long long)m);
        }
        __syncthreads();
    }
    uint64_t *slot = q.slot + no;
    for (int i = tid; i < n; i += NT) slot[i] = ld_l2((const uint64_t *)&tab[i]);
}

// ---- 3. k_dp_rescan<NL>: the gene slots whose range minimum saturated, exactly; a wavefront per slot ----
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_dp_rescan(DBatch b, G g, DDrop q) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, np = (dp_npath<G>(b, g, meta) - 1) / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const int32_t *first = q.first + no, *last = q.last + no;
    const uint64_t *slot = q.slot + no;
    const WInt<WL> negD = wi_neg<WL>(wi_load<WL>(ds + (size_t)(V - 1) * WL));
    for (int i = wv; i < np; i += NT / 64) {
        int j, k;
        if (!dp_gene(b, meta, path, i, &j, &k) || slot[j] != DP_SAT) continue;
        WInt<WL> best = wi_inf<WL>();
        for (int z = lane; z < V; z += 64) {
            if (last[z] <= j) continue;
            const WInt<WL> tz = wi_add<WL>(wi_load<WL>(dt + (size_t)z * WL), negD);
            [[maybe_unused]] bool sp = false;
            if constexpr (COND) sp = dp_sp_in(g, biased, ebase, in_off[z], in_off[z + 1]);
            for (uint32_t e = in_off[z], e1 = in_off[z + 1]; e < e1; e++) {
                const uint32_t sw = esrc[e];
                const int x = (int)ESRC_NODE(sw);
                const int fx = first[x];
                if (fx < 0 || fx >= j) continue;
                if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                const WInt<WL> c = wi_add<WL>(wi_add<WL>(wi_load<WL>(ds + (size_t)x * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), tz);
                if (wi_lt<WL>(c, best)) best = c;
            }
        }
        best = wave_min<WL>(best);
        if (lane == 0) {
            wi_store<WL>(q.sx + ((size_t)q.roff[blockIdx.x] + i) * dp_stride<G>(b, g), best);
            atomicAdd(&q.stats[2], 1ull);
        }
    }
}

// ---- 4. k_dp_cross<NL>: the cross nodes of each gene slot, one workgroup per contig ----
// The cross nodes of the contig (last(y) <= first(y), off P, reached both ways) go to a list (DDrop.js reused) with their list position per
// node (DDrop.jt reused); Y_j is the part of the list with last(y) <= j <= first(y).  Per gene slot with Y_j non-empty: delta(y) seeded from
// the edges x -> y with first(x) < j, Jacobi rounds within Y_j on two buffers (LDS up to DP_CROSS_LDS list entries, else DDrop.da / db),
// then the edges y -> z with last(z) > j give delta(y) + W + d_t(z) - D.  Every gene slot gets its cross minimum (inf: none) in DDrop.cx.
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_dp_cross(DBatch b, G g, DDrop q) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    __shared__ uint64_t s_d[2][DP_CROSS_LDS * WL];
    __shared__ uint64_t s_red[NT / 64][WL];
    __shared__ int s_nc, s_any, s_chg;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, np = (dp_npath<G>(b, g, meta) - 1) / 2, tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint32_t *oo = g.out_off + no + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const long long *ow = g.out_w + meta->edge_off;
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const int32_t *first = q.first + no, *last = q.last + no, *pidx = q.pidx + no;
    int32_t *clist = q.js + no, *cpos = q.jt + no;
    uint64_t *cx = q.cx + (size_t)q.roff[blockIdx.x] * dp_stride<G>(b, g);
    if (tid == 0) s_nc = 0;
    __syncthreads();
    for (int v = tid; v < V; v += NT) {
        const int f = first[v], l = last[v];
        int p = -1;
        if (pidx[v] < 0 && f >= 0 && l >= 0 && l <= f) { p = atomicAdd(&s_nc, 1); clist[p] = v; }
        cpos[v] = p;
    }
    __syncthreads();
    const int nc = s_nc;
    uint64_t *bufA = nc <= DP_CROSS_LDS ? s_d[0] : q.da + no * dp_stride<G>(b, g), *bufB = nc <= DP_CROSS_LDS ? s_d[1] : q.db + no * dp_stride<G>(b, g);
    const WInt<WL> negD = wi_neg<WL>(wi_load<WL>(ds + (size_t)(V - 1) * WL));
    for (int i = 0; i < np; i++) {
        int j, k;
        if (!dp_gene(b, meta, path, i, &j, &k)) continue; // (uniform over the workgroup)
        if (tid == 0) s_any = 0;
        __syncthreads();
        for (int p = tid; p < nc; p += NT) { const int y = clist[p]; if (last[y] <= j && j <= first[y]) s_any = 1; }
        __syncthreads();
        const bool any = s_any != 0;
        __syncthreads(); // (read by all before thread 0 resets it)
        if (!any) { if (tid == 0) wi_store<WL>(cx + (size_t)i * dp_stride<G>(b, g), wi_inf<WL>()); continue; }
        if (tid == 0) atomicAdd(&q.stats[1], 1ull);
        auto in_y = [&](int y) { return cpos[y] >= 0 && last[y] <= j && j <= first[y]; };
        // seed
        for (int p = tid; p < nc; p += NT) {
            const int y = clist[p];
            WInt<WL> d = wi_inf<WL>();
            [[maybe_unused]] bool sp = false;
            if constexpr (COND) { if (in_y(y)) sp = dp_sp_in(g, biased, ebase, in_off[y], in_off[y + 1]); }
            if (in_y(y))
                for (uint32_t e = in_off[y], e1 = in_off[y + 1]; e < e1; e++) {
                    const uint32_t sw = esrc[e];
                    const int x = (int)ESRC_NODE(sw);
                    const int fx = first[x];
                    if (fx < 0 || fx >= j) continue;
                    if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                    const WInt<WL> c = wi_add<WL>(wi_load<WL>(ds + (size_t)x * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt))));
                    if (wi_lt<WL>(c, d)) d = c;
                }
            wi_store<WL>(bufA + (size_t)p * WL, d);
        }
        __syncthreads();
        // Jacobi within Y_j (no cycle of negative length: settles in |Y_j| rounds)
        uint64_t *cur = bufA, *nxt = bufB;
        for (int r = 0; r <= nc + 1; r++) {
            if (tid == 0) s_chg = 0;
            __syncthreads();
            for (int p = tid; p < nc; p += NT) {
                const int y = clist[p];
                WInt<WL> d = wi_load<WL>(cur + (size_t)p * WL);
                [[maybe_unused]] bool sp = false;
                if constexpr (COND) { if (in_y(y)) sp = dp_sp_in(g, biased, ebase, in_off[y], in_off[y + 1]); }
                if (in_y(y))
                    for (uint32_t e = in_off[y], e1 = in_off[y + 1]; e < e1; e++) {
                        const uint32_t sw = esrc[e];
                        const int x = (int)ESRC_NODE(sw);
                        if (!in_y(x)) continue;
                        if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                        const WInt<WL> dx = wi_load<WL>(cur + (size_t)cpos[x] * WL);
                        if (wi_is_inf<WL>(dx)) continue;
                        const WInt<WL> c = wi_add<WL>(dx, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt))));
                        if (wi_lt<WL>(c, d)) { d = c; s_chg = 1; }
                    }
                wi_store<WL>(nxt + (size_t)p * WL, d);
            }
            __syncthreads();
            uint64_t *t = cur; cur = nxt; nxt = t;
            const bool chg = s_chg != 0;
            __syncthreads();
            if (!chg) break;
        }
        // leave Y_j
        WInt<WL> best = wi_inf<WL>();
        for (int p = tid; p < nc; p += NT) {
            const int y = clist[p];
            if (!in_y(y)) continue;
            const WInt<WL> d = wi_load<WL>(cur + (size_t)p * WL);
            if (wi_is_inf<WL>(d)) continue;
            [[maybe_unused]] bool sp = false;
            if constexpr (COND) sp = dp_sp_out(g, ebase, oo[y], oo[y + 1]);
            for (uint32_t e = oo[y], e1 = oo[y + 1]; e < e1; e++) {
                const int z = (int)od[e];
                if (last[z] <= j) continue;
                if constexpr (COND) { if (sp && mg_bit(g.r.fbit, ebase + e)) continue; }
                const WInt<WL> c = wi_add<WL>(wi_add<WL>(d, dp_w_out<WL>(g, sp, ebase + e, ew_decode<WL>(ow[e]))), wi_add<WL>(wi_load<WL>(dt + (size_t)z * WL), negD));
                if (wi_lt<WL>(c, best)) best = c;
            }
        }
        best = wave_min<WL>(best);
        if ((tid & 63) == 0) wi_store<WL>(s_red[tid >> 6], best);
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; w++) { const WInt<WL> o = wi_load<WL>(s_red[w]); if (wi_lt<WL>(o, best)) best = o; }
            wi_store<WL>(cx + (size_t)i * dp_stride<G>(b, g), best);
        }
        __syncthreads();
    }
}

// ---- 5. k_dp_rec<NL>: a record per pair of P (called = -1: no CDS gene, dropped by the host) ----
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_dp_rec(DBatch b, G g, DDrop q) {
    constexpr int WL = dp_wl<NL, G>;
    __shared__ int s_cnt;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int np = (dp_npath<G>(b, g, meta) - 1) / 2, tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const DNode *nd = b.node + no;
    const double *oweight = b.oweight + meta->orf_off;
    const uint64_t *slot = q.slot + no;
    const int64_t r0 = q.roff[blockIdx.x];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < np; i += NT) {
        phx_gene_drop r;
        const int a = path[2 * i + 1], bb = path[2 * i + 2];
        r.left = nd[a].pos; r.right = nd[bb].pos + 2; // as emit_genes
        r.frame = NFRAME(nd[a].info);
        r.strand = r.frame < 0 ? -1 : 1;
        r.score = 0.0; r.drop = __builtin_inf(); r.called = -1; r.bypass = 0;
        [[maybe_unused]] int32_t lost = 0;
        int j, k;
        if (dp_gene(b, meta, path, i, &j, &k)) {
            cnt++;
            r.score = oweight[k];
            r.called = 0; // (the host's)
            const uint64_t s = slot[j];
            WInt<WL> best = s == DP_SAT ? wi_load<WL>(q.sx + ((size_t)r0 + i) * dp_stride<G>(b, g)) : (s == DP_NONE ? wi_inf<WL>() : wi_from_u64<WL>(s));
            const WInt<WL> c = wi_load<WL>(q.cx + ((size_t)r0 + i) * dp_stride<G>(b, g));
            if (wi_lt<WL>(c, best)) best = c;
            if constexpr (dp_pin<G>) { // Delta = lost * M + s: the kept pins the best annotation without this stop gives up, and the class's own signed sum
                if (!wi_is_inf<WL>(best)) {
                    lost = (int32_t)(int64_t)(best.v[WL - 1] + (best.v[NL - 1] >> 63));
                    WInt<NL> sl;
#pragma unroll
                    for (int t = 0; t < NL; t++) sl.v[t] = best.v[t];
                    r.bypass = 1; r.drop = wi_to_double_rn<NL>(sl) / 1000.0;
                }
            } else
            if (!wi_is_inf<WL>(best)) { r.bypass = 1; r.drop = wi_to_double_rn<WL>(best) / 1000.0; }
        }
        q.rec[r0 + i] = r;
        if constexpr (dp_pin<G>) g.lost[r0 + i] = lost;
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(&q.stats[0], (unsigned long long)s_cnt);
}
