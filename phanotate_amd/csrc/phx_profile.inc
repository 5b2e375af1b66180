// phx_profile.inc — coding profiles: what each stretch of a contig costs as forward gene, as reverse gene or as gap; the re-annotation profiles: both kernels under MgCond; the pinned profiles: both under MgPinProf (included by phx_kernels.hip, after phx_drop.inc).
// ------------------------------------------------------------------------------------------------
// On demand after a run and after the margins' shared part (out-edge CSR, d_t: phx_margins.inc), never inside a run.  For one contig with
// V nodes (real nodes 0 .. m-1, m = V - 2, position-sorted; source V-2, target V-1) every edge e = (u -> v), ORF edge or connector, has
//     Delta(e) = d_s(u) + W(e) + d_t(v) - D >= 0,   mu(e) = float(Delta(e)) / 1000.0 as k_margins rounds it (+inf: u or v unreached)
// the length of the best source -> target walk forced through e, over the best path (DESIGN.md §34).  With rank(v) = v for a real node,
// rank(source) = -1 and rank(target) = m, the contig has n = m + 1 slots (slot s between node s-1 and node s), and an edge with
// rank(u) < rank(v) covers the slots rank(u)+1 .. rank(v).  Per slot and track — gene edges of the forward strand, of the reverse strand,
// connectors — the record carries the minimum mu over the covering edges.
//
// The key of the range minimum is the bit pattern of mu itself: rounding to a double and the division are monotone in Delta, and the
// patterns of non-negative doubles order like unsigned integers, so the minimum of the patterns is the pattern of mu(min Delta); +inf
// (PF_NONE) is "no edge".  No saturation marker and no exact rescan (§12's) are needed.
//
// One table serves the three tracks one after the other: a track's table is n (floor(log2 n) + 1) cells, indexed as k_dp_cand's — level k
// entry i covers the slots [i, i + 2^k); an edge goes to level floor(log2 len) at both ends of its range; the push-down gathers level k-1
// entry i from level k at i and at i - 2^(k-1).  Up to PF_TAB_LDS cells the table is in LDS, beyond in the contig's own slice of
// DProf.gtab (read back through L2): no atomic ever targets an address another contig uses.

#define PF_NONE 0x7ff0000000000000ull // the pattern of +inf: nothing of the track covers the slot

// The policy of the two kernels is the type of their second argument, as for k_sssp_rev and k_margins (phx_margins.inc).  DMarg: the run's
// graph, the kernels as §34 describes them.  MgCond (the re-annotation profiles, DESIGN.md §36): the graph G' = G_{F,B} of the last
// re-annotation, restricted to R — d_s' from DRmarg.ds, d_t' from DRmarg.dist_t (dp_ds / dp_dt), D' = d_s'(target); an in-edge slot whose bit
// is set in DReann.mask is no edge of G', one whose bit is set in DReann.bbit weighs W + DReann.bval (a contig solved under the bias policy
// only: dp_w_in), both read per edge only where the head node's slots share a bitmap word with such a slot (dp_sp_in).  A node outside R has
// no d_s' and no d_t' (k_sssp_rev<NL, MgCond> never relaxes it): its edges take no part.  Delta' >= 0 inside R (§21's lemma), so the key
// argument above carries over.  Everything the policy adds sits behind if constexpr (mg_cond<G>): the DMarg instantiations are the code they
// were without it.
//
// MgPinProf (the pinned profiles, DESIGN.md §37): MgPin — a contig solved under the required policy (DReann.mode 2 or 4) — with the place of
// `lost` and of the contig's round count, the two pointers MgPin lacks (no struct that exists grows).  dp_pin<G> holds for it: d_s' from
// DPmarg.ds on NL + 1 limbs, d_t' from DPmarg.dist_t at DPmarg.dt_stride, the DReann.req words inside dp_sp_in's test and one off the top limb
// of a required slot (dp_w_in).  Every edge has Delta'' = lost * M + s >= 0 on WL = NL + 1 limbs, decoded as k_margins<NL, MgPin> decodes it;
// per slot and track the record carries the lexicographic minimum of (lost, s): mu(s) in the record's field, lost in MgPinProf.lost, three
// int32 per slot (fwd, rev, gap).  A 64-bit key cannot order the pairs, so a track takes 1 + (distinct lost > 0 among its slots) rounds over
// the same table:
//   round 0      every edge of the track.  lost = 0: s >= 0 (Delta'' >= 0), the key is §34's, the pattern of mu, at most PF_NONE (+inf).
//                lost = l > 0: the marker PF_NONE + l — above every such pattern, ordered by l; "none" is PF_PNONE, above every marker.  After the
//                push-down a slot whose key is a pattern holds its exact result (0, mu); one that holds a marker knows L(i) = l, the least
//                lost among its covering edges, and gets (l, +inf) for now.
//   round l      for each level l some slot of the track holds, ascending (the block-wide least L(i) above the level just done): the table
//                is cleared, the edges with lost == l alone enter, keyed by pf_skey(mu) — the order-preserving map of a signed double —, and
//                after the push-down the slots with L(i) = l take pf_sval(key).  Exact, because every covering edge of slot i has
//                lost >= L(i): among the edges that entered, those covering i are exactly its covering edges of least lost, and rounding
//                is monotone in s.
// MgPinProf.rounds gets 3 + the level rounds of the three tracks.  All of it sits behind if constexpr (pf_pin<G>).
struct MgPinProf : MgPin { int32_t *lost; int32_t *rounds; };
template <class G> constexpr bool pf_pin = std::is_same<G, MgPinProf>::value;
#define PF_PNONE 0xffffffffffffffffull // MgPinProf: nothing of the track (round 0) / of the level (later rounds) covers the slot
// a signed double's pattern as an unsigned key of the same order (-0.0 below +0.0; no NaN enters), and back
__device__ __forceinline__ unsigned long long pf_skey(double x) { const unsigned long long p = (unsigned long long)__double_as_longlong(x); return (p >> 63) ? ~p : (p | 0x8000000000000000ull); }
__device__ __forceinline__ double pf_sval(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k)); }
// the contigs the pass covers: device distances and a settled reverse pass (a contig without a path is covered: every value is +inf); under
// MgCond the contigs solved again (DRmarg.sel 1: with a path, and a conditioned reverse pass that settled; 2: without one, D' unreached);
// under MgPinProf the same test on DPmarg.sel / mstat
template <class G>
__device__ __forceinline__ bool pf_on(const DBatch &b, const G &g, const DMeta *meta) {
    if constexpr (mg_cond<G>) { const int i = (int)(meta - b.meta), sel = g.r.sel[i]; return sel != 0 && mg_contig(meta) && (sel == 2 || !g.r.mstat[i]); }
    else return mg_contig(meta) && !g.mstat[meta - b.meta];
}
// rank of node v among the slots' bounds: source -1, real node v, target m
__device__ __forceinline__ int pf_rank(int v, int V) { return v < V - 2 ? v : (v == V - 2 ? -1 : V - 2); }
// track of an edge by its tail, as cbits and emit_genes tell an open node (forward start, reverse stop; tRNA nodes, frame +-4, alike):
// 0 a gene edge of the forward strand, 1 of the reverse strand, 2 a connector
__device__ __forceinline__ int pf_track(int32_t info) {
    const int ty = NTYPE(info), fr = NFRAME(info);
    if (ty == 0 && fr > 0) return 0;
    if (ty == 1 && fr < 0) return 1;
    return 2;
}

// a table cell as the workgroup's atomics left it (a global table: through L2, as k_dp_cand reads its own)
__device__ __forceinline__ uint64_t pf_ld(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- k_pf_cand<NL>: candidates, tables and push-down of the three tracks, one workgroup per contig ----
// Every in-edge of every node, once per track: classified by its tail, skipped when it covers nothing, is not of the track at hand or has
// mu = +inf; a coded gap edge reads the contig's gap table (edge_wenc).  The track's slot minima go to their field of the records.
// Every index is checked against the contig's own ranges before use.
// The body is instantiated once per placement of the table (pf_tracks: LDS or global memory), so that the LDS table is reached by LDS
// instructions and the global one by global ones; a table index is formed in unsigned 32-bit arithmetic, complete before it meets the
// base.  (As one body over a generic pointer the compiler split the source's rank -1 off the index: flat_atomic ... offset:8 on a base
// register 8 bytes below an LDS table that starts at the bottom of the LDS aperture — an address outside every aperture.)
template <int NL, class G, class T>
__device__ __forceinline__ void pf_tracks(const DBatch &b, const G &g, const DProf &q, const DMeta *meta, T *tab, int lv) {
    constexpr int WL = NL + (pf_pin<G> ? 1 : 0); // limbs of a value
    constexpr unsigned long long NONE = pf_pin<G> ? PF_PNONE : PF_NONE;
    const int V = meta->n_node, n = V - 1, tid = threadIdx.x;
    const uint32_t un = (uint32_t)n, cells = un * (uint32_t)lv;
    const size_t no = (size_t)meta->node_off;
    const DNode *nd = b.node + no;
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    const uint32_t E = (uint32_t)meta->n_edge;
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (mg_cond<G>) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    double *val = (double *)(q.rec + q.roff[blockIdx.x]); // four doubles per record: (lo, hi), fwd, rev, gap
    const WInt<WL> D = wi_load<WL>(ds + (size_t)(V - 1) * WL);
    const bool d_ok = !wi_unreached<WL>(D);
    const WInt<WL> negD = wi_neg<WL>(D);
    [[maybe_unused]] int32_t *lost = nullptr; // MgPinProf: three per slot, parallel to the records
    [[maybe_unused]] int rounds = 0;
    if constexpr (pf_pin<G>) lost = g.lost + 3 * (size_t)q.roff[blockIdx.x];
    [[maybe_unused]] int level = 0; // MgPinProf: the round's level (0: every edge of the track); a track is left when no level is pending
    // One loop serves the tracks and, under MgPinProf, a track's rounds: the step stays on the track while a level is pending.  (A loop
    // statement of its own around the rounds would change the DMarg and MgCond bodies: the compiler numbers a function's jump destinations.)
    for (int t = 0; t < 3; t += pf_pin<G> && level > 0 ? 0 : 1) {
        for (uint32_t i = (uint32_t)tid; i < cells; i += NT) tab[i] = NONE;
        __syncthreads();
        for (int v = tid; v < V && d_ok; v += NT) {
            const int rv = pf_rank(v, V);
            if (rv < 0) continue; // (the source: no in-edge, and nothing ends left of slot 0)
            uint32_t e = in_off[v], e1 = in_off[v + 1];
            if (e1 > E) e1 = E; // (the contig's own edges)
            bool have = false;
            WInt<WL> tz = negD;
            [[maybe_unused]] bool sp = false;
            if constexpr (mg_cond<G>) sp = dp_sp_in(g, biased, ebase, e, e1);
            for (; e < e1; e++) {
                const uint32_t sw = esrc[e];
                const int u = (int)ESRC_NODE(sw);
                if (u >= V) continue;
                if constexpr (mg_cond<G>) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; } // refused: no edge of G'
                const int ru = pf_rank(u, V);
                if (ru >= rv || pf_track(nd[u].info) != t) continue; // covers nothing (overlap connectors, equal ranks) / another track's
                if (!have) { // d_t(v) - D, at the first edge that asks for it
                    const WInt<WL> dv = wi_load<WL>(dt + (size_t)v * WL);
                    if (wi_unreached<WL>(dv)) break; // mu = +inf for every in-edge of v
                    tz = wi_add<WL>(dv, negD);
                    have = true;
                }
                const WInt<WL> du = wi_load<WL>(ds + (size_t)u * WL);
                if (wi_unreached<WL>(du)) continue;
                const WInt<WL> delta = wi_add<WL>(wi_add<WL>(du, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), tz);
                unsigned long long key;
                if constexpr (pf_pin<G>) { // Delta'' = lost * M + s, as k_margins<NL, MgPin> decodes it
                    const int32_t el = (int32_t)(int64_t)(delta.v[WL - 1] + (delta.v[NL - 1] >> 63));
                    if (level ? el != level : el > 0) {
                        if (level) continue; // another level's
                        key = PF_NONE + (unsigned long long)(uint32_t)el; // the marker of lost = el
                    } else {
                        WInt<NL> sl;
#pragma unroll
                        for (int i = 0; i < NL; i++) sl.v[i] = delta.v[i];
                        const double mu = wi_to_double_rn<NL>(sl) / 1000.0;
                        key = level ? pf_skey(mu) : (unsigned long long)__double_as_longlong(mu); // (lost = 0: s >= 0)
                    }
                } else
                key = (unsigned long long)__double_as_longlong(wi_to_double_rn<NL>(delta) / 1000.0);
                const uint32_t a = (uint32_t)(ru + 1), z = (uint32_t)rv, k = 31u - (uint32_t)__clz((int)(z - a + 1u)); // slots [a, z], 0 <= a <= z <= n - 1; 2^k <= z - a + 1 <= n: k < lv
                const uint32_t ia = k * un + a, iz = k * un + (z + 1u - (1u << k));                                     // (a <= z + 1 - 2^k <= z)
                if (ia >= cells || iz >= cells) continue; // (cannot happen)
                atomicMin(&tab[ia], key);
                atomicMin(&tab[iz], key);
            }
        }
        __syncthreads();
        for (uint32_t k = (uint32_t)lv - 1u; k >= 1u; k--) {
            const uint32_t h = 1u << (k - 1u);
            for (uint32_t i = (uint32_t)tid; i < un; i += NT) {
                uint64_t m = pf_ld(&tab[k * un + i]);
                if (i >= h) { const uint64_t m2 = pf_ld(&tab[k * un + (i - h)]); m = m2 < m ? m2 : m; }
                if (m != NONE) atomicMin(&tab[(k - 1u) * un + i], (unsigned long long)m);
            }
            __syncthreads();
        }
        if constexpr (pf_pin<G>) {
            __shared__ int s_next; // the least L(i) above `level` among the track's slots (a slot is its own thread's in every round)
            if (tid == 0) s_next = 0x7fffffff;
            __syncthreads();
            int next = 0x7fffffff;
            for (uint32_t i = (uint32_t)tid; i < un; i += NT) {
                const unsigned long long k = pf_ld(&tab[i]);
                int32_t L;
                if (level == 0) { // a pattern: (0, mu), exact; a marker: (l, for now +inf); none: (0, +inf)
                    L = k > PF_NONE && k != PF_PNONE ? (int32_t)(uint32_t)(k - PF_NONE) : 0;
                    val[4 * (size_t)i + 1 + t] = __longlong_as_double((long long)(k < PF_NONE ? k : PF_NONE));
                    lost[3 * (size_t)i + t] = L;
                } else {
                    L = lost[3 * (size_t)i + t];
                    if (L == level && k != PF_PNONE) val[4 * (size_t)i + 1 + t] = pf_sval(k);
                }
                if (L > level && L < next) next = L;
            }
            if (next != 0x7fffffff) atomicMin(&s_next, next);
            __syncthreads(); // (and every read of the table is done before the next round clears it)
            level = s_next == 0x7fffffff ? 0 : s_next;
            rounds++;
            __syncthreads(); // (s_next is read before the next round resets it)
        } else {
        for (uint32_t i = (uint32_t)tid; i < un; i += NT) val[4 * (size_t)i + 1 + t] = __longlong_as_double((long long)pf_ld(&tab[i]));
        __syncthreads(); // (every read of the table is done before the next track clears it)
        }
    }
    if constexpr (pf_pin<G>) { if (tid == 0) g.rounds[blockIdx.x] = rounds; }
}
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_pf_cand(DBatch b, G g, DProf q) {
    __shared__ unsigned long long s_tab[PF_TAB_LDS];
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!pf_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int n = meta->n_node - 1;
    int lv = 1;
    while ((2 << (lv - 1)) <= n) lv++; // floor(log2 n) + 1
    if (n * lv <= PF_TAB_LDS) pf_tracks<NL, G>(b, g, q, meta, s_tab, lv); // (uniform over the workgroup)
    else pf_tracks<NL, G>(b, g, q, meta, (unsigned long long *)(q.gtab + q.toff[blockIdx.x]), lv);
}

// ---- k_pf_rec: the bounds of every slot, a thread per slot ----
// lo / hi: the positions of the nodes left and right of the slot (phx_tap_nodes pos); slot 0 starts at the source's (0), the last slot ends
// at the target's (L + 1).
template <class G = DMarg>
__global__ __launch_bounds__(NT) void k_pf_rec(DBatch b, G g, DProf q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!pf_on<G>(b, g, meta)) return;
    const int V = meta->n_node, n = V - 1;
    const DNode *nd = b.node + meta->node_off;
    phx_profile_slot *rec = q.rec + q.roff[blockIdx.x];
    for (int i = (int)blockIdx.y * NT + (int)threadIdx.x; i < n; i += (int)gridDim.y * NT) {
        rec[i].lo = nd[i == 0 ? V - 2 : i - 1].pos;
        rec[i].hi = nd[i == n - 1 ? V - 1 : i].pos;
    }
}
