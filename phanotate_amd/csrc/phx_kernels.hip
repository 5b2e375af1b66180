// phx_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels for PHANOTATE's per-contig hot path; one translation
// unit, the stages live in the .inc files below.
//
// Stage            kernels                                  file               reference code restated
// --------------   --------------------------------------   ----------------   ------------------------------------------
// features         k_features                               phx_features.inc   functions.py:158-171 (per-base loop),
//                                                                              score_rbs 48-138, gc_frame_plot.py:29-74
// ORF scan         k_orf<EMIT>                              phx_orf.inc        functions.py:184-251, orfs.py:17-32
// ORF statistics   k_orf_stats                              phx_orf.inc        orfs.py:162-173, functions.py:261-279,286-298
// ORF weight       k_score                                  phx_orf.inc        functions.py:254-257,281-284,300-301, orfs.py:122-127
// nodes            k_node_cov/_rank/_build/_attr            phx_graph.inc      functions.py:311-318 (nodes), 320-333 (coverage),
//                                                                              363-384 (other_end / o1,o2)
// edges            k_edges<FILL>, k_edges_scan              phx_graph.inc      functions.py:334-354, 360-452
// layout           k_layout1, k_layout2, k_sssp_order,      phx_layout.inc     (offsets, integer class and solver per contig; launch order of the
//                  k_gene_pack, k_results                                      solver and gene slots for large batches; result records)
// shortest path    k_wave_plan + k_sssp_wave<2> (wavefront  phx_sssp_wave.inc  fastpathz (phanotate.py:56-64), exact NL x 64-bit
//                  / contig)
//                  k_sssp_lds<NL> (workgroup / contig),     phx_sssp.inc       integers; path -> genes phanotate.py:65-76,
//                  k_sssp<NL> + k_path<NL> (global memory)                     locus.py:29-37
//                  k_inorder (ties between equal-length paths)  phx_inorder.inc    relaxation order of the reference's solver
//                  k_refine (flagged edges in double-double) phx_refine.inc    functions.py:26-46,286-301: bounds on the reference's integers
//                  k_certify (fp64 vs Decimal weights)      phx_certify.inc    edges.py:17-23: the integers the reference solves on
//
// No MFMA anywhere: the path has no dense contraction.  All integer outputs are
// bit-exact with the reference; fp64 is used where the reference uses Decimal (edge weights only).
#include <hip/hip_runtime.h>
#include <type_traits>

#include "phx_internal.h"

#define NT PHX_CTG_THREADS

// ------------------------------------------------------------------------------------------------
// wave / block primitives (wave64)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d);
        if (lane >= d) v = v > t ? v : t;
    }
    return v;
}
// Exclusive block sum-scan over N threads (N multiple of 64, <= 1024). lds: N/64+1 words.
template <int N>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < N / 64; i++) { uint32_t t = lds[i]; lds[i] = s; s += t; }
        lds[N / 64] = s;
    }
    __syncthreads();
    uint32_t r = inc - v + lds[w];
    *total = lds[N / 64];
    __syncthreads();
    return r;
}
// Exclusive block max-scan (identity 0).
template <int N>
__device__ __forceinline__ uint32_t block_excl_max(uint32_t v, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_max(v);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < N / 64; i++) { uint32_t t = lds[i]; lds[i] = s; s = s > t ? s : t; }
        lds[N / 64] = s;
    }
    __syncthreads();
    uint32_t prev = __shfl_up(inc, 1);
    if (lane == 0) prev = 0;
    uint32_t r = prev > lds[w] ? prev : lds[w];
    *total = lds[N / 64];
    __syncthreads();
    return r;
}

// value of the lane `n` places to the left inside the 16-lane DPP row (own value for the first n lanes)
template <int N>
__device__ __forceinline__ uint32_t dpp_row_shr(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x110 + N, 0xf, 0xf, false); }
template <int N>
__device__ __forceinline__ uint64_t dpp_row_shr64(uint64_t x) { return ((uint64_t)dpp_row_shr<N>((uint32_t)(x >> 32)) << 32) | dpp_row_shr<N>((uint32_t)x); }
// sum over a 16-lane DPP row; the total lands in lane 15 of the row (sub = lane & 15)
__device__ __forceinline__ uint64_t row16_sum_u64(uint64_t x, int sub) {
    uint64_t y;
    y = dpp_row_shr64<1>(x); if (sub >= 1) x += y;
    y = dpp_row_shr64<2>(x); if (sub >= 2) x += y;
    y = dpp_row_shr64<4>(x); if (sub >= 4) x += y;
    y = dpp_row_shr64<8>(x); if (sub >= 8) x += y;
    return x;
}

// ------------------------------------------------------------------------------------------------
// Edge records as the kernels keep them (DBatch.esrc / DBatch.ew, 4 + 8 bytes per edge).
//   ew: the integer the solver works on, W = trunc(w * 1000) (edges.py:22), so that no consumer converts fp64 again: a value with
//       |W| < 2^62 as it is (bits 63 and 62 equal); a wider one as the bit pattern of the double p = trunc(w * 1000) — whose bit 62 is
//       always set, |p| >= 2^62 — with bit 62 forced to differ from bit 63, which marks it (ew_decode, phx_sssp.inc, restores it).
//   esrc: source node in bits 0..29; bit 30 = "off the solver's common path": |W| >= 2^51 (its integer is not the low half of a narrow
//       128-bit value) or the edge leaves the source node (whose distance has its own ring slot), so that k_sssp_wave tests one
//       bit per in-edge; bit 31 = "inexact": the reference's integer trunc(Decimal(w) * 1000) may differ from W
//       (k_certify's eps_e > 0, phx_certify.inc) — decided here, where the fp64 weight still exists.
// The fp64 weights themselves are not kept: the taps recompute them (k_edges<true, true>).
#define EW_WIDE(x) (((((unsigned long long)(x)) >> 63) ^ (((unsigned long long)(x)) >> 62)) & 1ull)
__device__ __forceinline__ long long ew_encode(double w) {
    const double t = trunc(w * 1000.0);
    if (fabs(t) < 2251799813685248.0) return __double_as_longlong(t + 6755399441055744.0) - 0x4338000000000000ll; // |t| < 2^51: the integer sits in the low mantissa bits of t + 1.5 * 2^52
    if (fabs(t) < 4611686018427387904.0) return (long long)t;
    const long long bits = __double_as_longlong(t);
    return bits < 0 ? (bits & ~(1ll << 62)) : bits;
}
__device__ __forceinline__ bool ew_narrow51(long long w) { return (unsigned long long)(w + (1ll << 51)) < (1ull << 52); }
// cert_eps(w) == 0 (phx_certify.inc): p = w * 1000 is farther from the next integer than an upper bound of its error bound
// |p| (|exponent| + 8) 2^-46 x scale — |exponent| + 8 <= 60 for 1/2 <= |p| < 2^52, and a |p| below 1/2 truncates to 0 on both sides
// whatever its exponent —, so the reference's truncation cannot differ.  c = scale * 2^-46.
__device__ __forceinline__ bool cert_eps_is_zero_fast(double w, double c) {
#ifdef EW_NOCHECK
    return true;
#endif
    const double p = w * 1000.0, a = fabs(p);
    const double f = a - fabs(trunc(p));
    const bool far = (f < 1.0 - f ? f : 1.0 - f) > a * (60.0 * c);
    return w == -20.0 || (a < 4503599627370496.0 && far);
}
#define CERT_C(b) ((b).cert_scale * 1.4210854715202004e-14) // 2^-46
// one edge weight in registers: what goes to DBatch.ew (the encoded integer; the fp64 bits in the tap variant) and the inexact flag
struct EWt { unsigned long long bits; uint32_t fl; int code; }; // code >= 0: an entry of the contig's gap table (the edge goes out in the ESRC_F_GAP form)
template <bool TAPW>
__device__ __forceinline__ EWt make_ew(double w, double c) {
    EWt r;
    r.code = -1;
    if (TAPW) { r.bits = (unsigned long long)__double_as_longlong(w); r.fl = 0u; }
    else {
        r.bits = (unsigned long long)ew_encode(w);
        r.fl = (cert_eps_is_zero_fast(w, c) ? 0u : ESRC_F_INEXACT) | (ew_narrow51((long long)r.bits) ? 0u : ESRC_F_OFFPATH);
    }
    return r;
}

// the encoded integer weight of edge e (contig-relative) whose source word is sw: a coded gap edge (ESRC_F_GAP) has it in the contig's gap table
__device__ __forceinline__ long long edge_wenc(uint32_t sw, const long long *ew, uint32_t e, const long long *gt) { return ESRC_IS_GAP(sw) ? gt[ESRC_GAP_CODE(sw)] : ew[e]; }
__device__ __forceinline__ const long long *gtab_of(const DBatch &b, const DMeta *meta) { return b.gtab ? b.gtab + (size_t)(meta - b.meta) * GT_N : nullptr; } // (phx_solve: no table, no coded edge)
__device__ __forceinline__ const long long *gtab_at(const DBatch &b, uint32_t ci) { return b.gtab ? b.gtab + (size_t)ci * GT_N : nullptr; } // ... by the contig's index (where `meta` is not an entry of b.meta: scenario slots)

// functions.py:174-178: both strands are counted, so Pa == Pt and Pg == Pc.
__device__ __forceinline__ double contig_pstop(uint32_t gc, int L) {
    double fa = (double)((uint32_t)L - gc), fg = (double)gc;
    double d = (double)((int64_t)L * 2);
    double Pa = fa / d, Pt = fa / d, Pg = fg / d;
    return Pt * Pa * Pa + Pt * Pg * Pa + Pt * Pa * Pg;
}
// gc_frame_plot.py:7-28
__device__ __forceinline__ int max_idx(int a, int b, int c) { return a > b ? (a > c ? 1 : 3) : (b > c ? 2 : 3); }
__device__ __forceinline__ int min_idx(int a, int b, int c) { return a > b ? (b > c ? 3 : 2) : (a > c ? 3 : 1); }

#include "phx_features.inc"
#include "phx_orf.inc"
#include "phx_graph.inc"
#include "phx_sssp.inc"
#include "phx_layout.inc"
#include "phx_front.inc"
#include "phx_sssp_seg.inc"
#include "phx_sssp_wave.inc"
#include "phx_sssp_duo.inc"
#include "phx_inorder.inc"
#include "phx_refine.inc"
#include "phx_certify.inc"
#include "phx_margins.inc"
#include "phx_drop.inc"
#include "phx_profile.inc"
#include "phx_replace.inc"
#include "phx_resolve.inc"

// ------------------------------------------------------------------------------------------------
// launchers
// fn(std::integral_constant<int, NL>) for every limb class of nlm (bit k: 2, 4, 8, 17 limbs), in that order: the one place that turns a
// mask of classes into launches of K<NL>
template <class F>
static void each_limb_class(int nlm, F fn) {
    if (nlm & 1) fn(std::integral_constant<int, 2>());
    if (nlm & 2) fn(std::integral_constant<int, 4>());
    if (nlm & 4) fn(std::integral_constant<int, 8>());
    if (nlm & 8) fn(std::integral_constant<int, 17>());
}
static int limb_class_bit(int nl) { return nl == 2 ? 1 : nl == 4 ? 2 : nl == 8 ? 4 : 8; } // ... and the mask of the one class nl (any other count: 17 limbs)
template <int NL>
static void launch_certify(const DBatch *b, int vcap, hipStream_t s) {
    const size_t lds = (size_t)vcap * 12 + 16;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_certify<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_certify<NL>, dim3(b->n_contig), dim3(CERT_T), lds, s, *b, vcap);
    hipLaunchKernelGGL(k_certify_wide<NL>, dim3(b->n_contig), dim3(CERT_T), 0, s, *b);
}
// `grid` workgroups of SW_THREADS with `lds` bytes of dynamic LDS (k_sssp_lds, k_rs_lds, k_sc_lds: one instantiation per limb class)
template <class... A>
static void launch_lds(void (*k)(A...), size_t lds, unsigned grid, hipStream_t s, A... args) {
    (void)hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(grid), dim3(SW_THREADS), lds, s, args...);
}
// k_sssp_wave<NL, CFG>, a wavefront per contig, with its dynamic LDS; beside: its variant that follows the counter of the planner it is
// launched beside (FOLLOWS: the configuration has one — the roomy 128-bit one has not, and none is to be instantiated)
template <int NL, int CFG, bool FOLLOWS>
static void launch_wave(const DBatch *b, bool beside, hipStream_t s) {
    const size_t lb = wv_lds_bytes<NL, CFG>();
    (void)hipFuncSetAttribute((const void *)k_sssp_wave<NL, CFG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    if constexpr (FOLLOWS) {
        if (beside) {
            (void)hipFuncSetAttribute((const void *)k_sssp_wave<NL, CFG, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
            hipLaunchKernelGGL((k_sssp_wave<NL, CFG, true>), dim3(b->n_contig), dim3(64), lb, s, *b);
            return;
        }
    }
    hipLaunchKernelGGL((k_sssp_wave<NL, CFG>), dim3(b->n_contig), dim3(64), lb, s, *b);
}
// The re-annotation's two solver kernels by what they are launched on: DReann — the batch, a workgroup per contig —, DScen — a range of a
// chunk's slot table, a workgroup per slot (phx_resolve.inc).
template <int NL, class Pol> static auto re_lds_kernel(const DReann *) { return k_rs_lds<NL, Pol>; }
template <int NL, class Pol> static auto re_lds_kernel(const DScen *) { return k_sc_lds<NL, Pol>; }
template <int NL, int T, class Pol> static auto re_inorder_kernel(const DReann *) { return k_rs_inorder<NL, T, Pol>; }
template <int NL, int T, class Pol> static auto re_inorder_kernel(const DScen *) { return k_sc_inorder<NL, T, Pol>; }
// the sweep under Pol for every limb class of nlm (bit k: 2, 4, 8, 17 limbs), `grid` workgroups
template <class Pol, class Q>
static void re_solve(const DBatch *b, const Q *q, unsigned grid, int nlm, hipStream_t s) {
    if (!grid) return;
    each_limb_class(nlm, [&](auto nl) { launch_lds(re_lds_kernel<decltype(nl)::value, Pol>(q), ReSw<decltype(nl)::value, Pol>::LDS, grid, s, *b, *q); });
}
// ... and the in-order pass: as phxk_inorder, one wavefront per short contig, else 256 threads
template <int T, class Pol, class Q>
static void re_inorder_t(const DBatch *b, const Q *q, unsigned grid, int nlm, hipStream_t s) {
    each_limb_class(nlm, [&](auto nl) { hipLaunchKernelGGL((re_inorder_kernel<decltype(nl)::value, T, Pol>(q)), dim3(grid), dim3(T), 0, s, *b, *q); });
}
template <class Pol, class Q>
static void re_inorder_launch(const DBatch *b, const Q *q, unsigned grid, int nlm, hipStream_t s) {
    if (!grid) return;
    if (b->mean_len < 8192) re_inorder_t<64, Pol>(b, q, grid, nlm, s);
    else re_inorder_t<IO_T_FULL, Pol>(b, q, grid, nlm, s);
}
// Range r of a chunk's slot table (0 plain, 1 pinned, 2 biased, 3 both: pinned and biased; n_range: their slot counts) as a table of its
// own, so that blockIdx.x is a slot of the range: the per-slot arrays moved to the range's first slot.  The pair and triple lists stay the
// whole table's.
static DScen scen_range(const DScen &q, const int *n_range, int r) {
    DScen t = q;
    const int first = (r > 0 ? n_range[0] : 0) + (r > 1 ? n_range[1] : 0) + (r > 2 ? n_range[2] : 0);
    t.n_slot = n_range[r];
    t.slot += first; t.meta += first; t.rec += first;
    if (t.req0) { t.req0 += first; t.nreq += first; t.kreq += first; }
    if (t.bs) t.bs += first;
    return t;
}
extern "C" {
void phxk_features(const DBatch *b, uint32_t v_begin, uint32_t v_end, void *stream) {
    if (v_end <= v_begin) return;
    const unsigned g = (v_end - 1) / FEAT_SPAN - v_begin / FEAT_SPAN + 1;
    if (b->defcod) hipLaunchKernelGGL((k_features<false, true>), dim3(g), dim3(64), 0, (hipStream_t)stream, *b, v_begin, v_end, (uint32_t *)nullptr, -1);
    else hipLaunchKernelGGL((k_features<false, false>), dim3(g), dim3(64), 0, (hipStream_t)stream, *b, v_begin, v_end, (uint32_t *)nullptr, -1);
}
// (host copies of voff are the caller's: it passes the contig's range)
void phxk_features_tap(const DBatch *b, int contig, uint32_t v_begin, uint32_t v_end, uint32_t *tapbuf, void *stream) {
    if (v_end <= v_begin) return;
    const unsigned g = (v_end - 1) / FEAT_SPAN - v_begin / FEAT_SPAN + 1;
    hipLaunchKernelGGL((k_features<true, false>), dim3(g), dim3(64), 0, (hipStream_t)stream, *b, v_begin, v_end, tapbuf, contig);
}
void phxk_pack_planes(const DBatch *b, const void *letters, void *stream) {
    if (b->n_contig > 0) hipLaunchKernelGGL(k_pack_planes, dim3(b->n_contig, 8), dim3(64), 0, (hipStream_t)stream, *b, (const uint8_t *)letters);
}
// Workgroups per contig of the per-contig kernels: `full` for the benchmark's 50 kb contigs, fewer for batches of short contigs
// (a 2 kb contig has ~100 nodes: four workgroups of 256 threads would leave three idle), by the batch's mean contig length.
#ifndef YS_EMIT
#define YS_EMIT 6
#endif
#ifndef YS_STATS
#define YS_STATS 8
#endif
static unsigned ysplit(const DBatch *b, unsigned full) {
    const unsigned y = (unsigned)((b->mean_len + 8191) / 8192);
    // a few long contigs (T4 alone: 21 pieces of 8 kb) leave the chip empty: four times as many workgroups per contig while they all fit at once
    const unsigned cap = (unsigned)b->n_contig * 4u * full <= 256u ? 4u * full : full;
    return y < 1u ? 1u : (y > cap ? cap : y);
}
void phxk_orf_count(const DBatch *b, void *stream) {
    if (b->mean_len < 16384) hipLaunchKernelGGL((k_orf<false, 256>), dim3(b->n_contig), dim3(256), 0, (hipStream_t)stream, *b);
    else hipLaunchKernelGGL((k_orf<false, ORF_COUNT_T>), dim3(b->n_contig), dim3(ORF_COUNT_T), 0, (hipStream_t)stream, *b);
}
void phxk_orf_emit(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_orf<true>, dim3(b->n_contig, ysplit(b, YS_EMIT)), dim3(NT), 0, (hipStream_t)stream, *b); }
void phxk_bit_prefix(const DBatch *b, void *stream) {
    hipLaunchKernelGGL(k_bit_prefix, dim3(b->n_contig, 7), dim3(64), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_gap_table, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b); // (needs the g+c counts of k_features only: here it hides beside the ORF scan)
}
void phxk_orf_stats(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_orf_stats, dim3(b->n_contig, ysplit(b, YS_STATS)), dim3(NT), 0, (hipStream_t)stream, *b); }
void phxk_score(const DBatch *b, void *stream) {
    if (b->n_contig <= 16 && b->mean_len >= 32768) { hipLaunchKernelGGL(k_score_big, dim3(b->n_contig), dim3(1024), 0, (hipStream_t)stream, *b); return; }
    hipLaunchKernelGGL(k_score, dim3(b->n_contig), dim3(b->mean_len >= 8192 ? NT : 64), 0, (hipStream_t)stream, *b);
}
// node stage, part 1: needs the ORF / group records of k_orf<true> only (not their statistics), so the launcher runs it
// beside k_orf_stats / k_score
// one workgroup per contig runs the node bodies in a row — unless the batch is a few LONG contigs (T4: one 256-thread workgroup then takes
// 111 us and k_node_attr waits for it; the staged kernels spread coverage and records over four workgroups per contig: 60 us)
static bool nodes_per_contig(const DBatch *b) {
#ifndef NODES_STAGED
    return !(b->n_contig <= 16 && b->mean_len >= 32768);
#else
    return false;
#endif
}
int phxk_chain_ok(const DBatch *b) { return nodes_per_contig(b) ? 1 : 0; }
void phxk_graph_chain(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_graph_chain<CHAIN_T>, dim3(b->n_contig), dim3(CHAIN_T), 0, (hipStream_t)stream, *b); }
void phxk_nodes(const DBatch *b, void *stream) {
    if (nodes_per_contig(b)) {
        hipLaunchKernelGGL(k_nodes_fused, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b);
        return;
    }
    hipLaunchKernelGGL(k_node_cov, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_node_rank, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_node_build, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_node_order, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b);
}
// part 2: other_end of every node and which ORF's p_stop is its o1/o2 term; part 3, behind k_orf_stats: the term itself
void phxk_node_attr(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_node_attr, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b); }
void phxk_node_oterm(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_node_oterm, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b); }
void phxk_edges_count(const DBatch *b, void *stream) {
    hipLaunchKernelGGL(k_edges<false>, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b);
    if (b->n_contig <= 16 && b->mean_len >= 32768) hipLaunchKernelGGL(k_edges_scan_big, dim3(b->n_contig), dim3(1024), 0, (hipStream_t)stream, *b);
    else hipLaunchKernelGGL(k_edges_scan, dim3(b->n_contig), dim3(ES_T), 0, (hipStream_t)stream, *b);
}
void phxk_edges_fill(const DBatch *b, void *stream) {
    if (b->gap_code) hipLaunchKernelGGL((k_edges<true, false, true>), dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b); // gap edges in the coded form
    else hipLaunchKernelGGL(k_edges<true>, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b);
}
void phxk_edges_orf(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_edges_orf, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b); }
void phxk_edges_expand(const DBatch *b, int nl, int mode, void *stream) { hipLaunchKernelGGL(k_edges_expand, dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b, nl, mode); }
void phxk_edges_tap(const DBatch *b, void *stream) { hipLaunchKernelGGL((k_edges<true, true>), dim3(b->n_contig, ysplit(b, 4)), dim3(NT), 0, (hipStream_t)stream, *b); }
// phx_solve: relaxation, path walk (no genes: DBatch.genes is null), in-order parents
void phxk_sssp_only(const DBatch *b, int nl, void *stream) {
    phxk_sssp(b, nl, 0, 0, stream);
    phxk_inorder(b, limb_class_bit(nl), stream);
}

// nl_mask: bit k set = some contig of the batch has 2 / 4 / 8 / 17 limbs (k = 0..3)
void phxk_inorder(const DBatch *b, int nl_mask, void *stream) {
    dim3 g(b->n_contig);
    hipStream_t s = (hipStream_t)stream;
    // the benchmark's kind of contig: 256 threads; batches of short contigs (a workgroup is one contig with a hundred nodes): one wavefront
    // and a quarter of the LDS for the path walk, so that four times as many contigs are in flight
    const bool small = b->mean_len < 8192;
    const bool big = (b->n_contig <= 64 && b->mean_len >= 65536) || (b->n_contig <= 8 && b->mean_len >= 16384); // a handful of long contigs (or a few of any length: Lambda): the chip is empty, a contig's one workgroup may as well be a large one — and its path walk goes in strides
    if (big && (nl_mask & 1)) { hipLaunchKernelGGL((k_inorder<2, IO_T_BIG>), g, dim3(IO_T_BIG), 0, s, *b); nl_mask &= ~1; }
    if (small) each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_inorder<decltype(nl)::value, 64>), g, dim3(64), 0, s, *b); });
    else each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_inorder<decltype(nl)::value, IO_T_FULL>), g, dim3(IO_T_FULL), 0, s, *b); });
}

// vmax: the largest node count the batch is expected to hold (the last run's): sizes the LDS tables of k_certify (12 bytes per node, at
// most 144 KB); a contig with more nodes than that goes through k_certify_wide, launched right behind (it returns at once otherwise)
void phxk_certify(const DBatch *b, int nl_mask, int vmax, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int vcap = ((vmax > 1024 ? vmax : 1024) + 255) & ~255;
    if (vcap > 12288) vcap = 12288;
    if (vmax < 0) vcap = 0; // (test switch: everything to k_certify_wide)
    each_limb_class(nl_mask, [&](auto nl) { launch_certify<decltype(nl)::value>(b, vcap, s); });
}

void phxk_refine(const DBatch *b, void *stream) {
    // (one workgroup per contig; a few long contigs — T4 alone: 29 000 edges, 15 rounds of its scan — get up to 16: 97 -> see DESIGN.md §7)
    const unsigned y = b->n_contig <= 16 ? ysplit(b, 4) : 1u;
    hipLaunchKernelGGL(k_refine, dim3(b->n_contig, y), dim3(RF_T), 0, (hipStream_t)stream, *b);
}

void phxk_gene_pack(const DBatch *b, void *stream) {
    const unsigned g = (unsigned)((b->n_contig + LMB_T - 1) / LMB_T);
    hipLaunchKernelGGL(k_gene_pack_a, dim3(g), dim3(LMB_T), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_gene_pack_b, dim3(g, 8), dim3(LMB_T), 0, (hipStream_t)stream, *b);
}
void phxk_reset(const DBatch *b, const void *meta0, unsigned long long nbits_words, unsigned long long tbits_words, void *stream) {
    unsigned long long work = nbits_words / 2 + tbits_words / 2 + (unsigned long long)b->n_contig * (sizeof(DMeta) / 8);
    unsigned g = (unsigned)((work + 255) / 256);
    g = g < 1u ? 1u : (g > 4096u ? 4096u : g);
    hipLaunchKernelGGL(k_reset, dim3(g), dim3(256), 0, (hipStream_t)stream, *b, (const DMeta *)meta0, nbits_words, tbits_words);
}
int phxk_front_blocks_y(const DBatch *b) {
    if (b->n_contig < 1 || b->n_contig > FRONT_MAX_CONTIGS || b->mean_len * b->n_contig > (40 << 10)) return 0; // (since the staged kernels of a few long contigs run with four times as many workgroups per contig — ysplit — they win from ~32 kb on: 8 / 16 / 24 kb fused 0.273 / 0.304 / 0.307 ms against 0.291 / 0.314 / 0.314 staged, 32 kb 0.313 / 0.312, Lambda 0.369 / 0.360, 2 x 50 kb 0.395 / 0.376)
    unsigned y = ysplit(b, 8);
    while (y > 1 && (unsigned)b->n_contig * y > FRONT_MAX_BLOCKS) y--;
    return (unsigned)b->n_contig * y <= FRONT_MAX_BLOCKS ? (int)y : 0;
}
void phxk_front(const DBatch *b, void *stream) {
    const int y = phxk_front_blocks_y(b);
    if (y > 0) hipLaunchKernelGGL(k_front, dim3(b->n_contig, y), dim3(NT), 0, (hipStream_t)stream, *b);
}
void phxk_seg_merge(const DBatch *b, int vmax, void *stream) {
    // workgroups per contig of the join: one per 16 nodes of the largest contig the last run saw (a workgroup walks its share in rounds of four
    // dependent loads: T4 on 64 workgroups took 5.4 rounds, 22 us), at most 4096 in all
    const int n = b->n_contig > 0 ? b->n_contig : 1;
    int y = vmax > 0 ? (vmax + SEGJ_T / SEGJ_LPN - 1) / (SEGJ_T / SEGJ_LPN) : 64;
    const int cap = 4096 / n;
    y = y > cap ? cap : y;
    y = y < 4 ? 4 : y;
    hipLaunchKernelGGL(k_seg_join, dim3(b->n_contig, y), dim3(SEGJ_T), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_seg_close, dim3(b->n_contig), dim3(SEGM_T), 0, (hipStream_t)stream, *b);
}
int phxk_seg_kmax(void) { return SEG_KMAX; }
void phxk_seg_fallback(const DBatch *b, void *stream) {
    hipLaunchKernelGGL((k_wave_plan<2, 0>), dim3(b->n_contig), dim3(64), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL((k_sssp_duo<0, false>), dim3(b->n_contig), dim3(128), 0, (hipStream_t)stream, *b);
}
void phxk_results(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_results, dim3((unsigned)((b->n_contig + LMB_T - 1) / LMB_T)), dim3(LMB_T), 0, (hipStream_t)stream, *b); }
// per-ORF margins (phx_margins.inc): three launches for the out-edge CSR, one reverse pass per limb class, one for the records
void phxk_margins_transpose(const DBatch *b, const DMarg *g, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const unsigned y = ysplit(b, 4);
    hipLaunchKernelGGL(k_mg_count, dim3(b->n_contig, y), dim3(NT), 0, s, *b, *g);
    hipLaunchKernelGGL(k_mg_scan, dim3(b->n_contig), dim3(NT), 0, s, *b, *g);
    hipLaunchKernelGGL(k_mg_fill, dim3(b->n_contig, y), dim3(NT), 0, s, *b, *g);
}
void phxk_sssp_rev(const DBatch *b, const DMarg *g, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL(k_sssp_rev<decltype(nl)::value>, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b, *g); });
}
void phxk_margins(const DBatch *b, const DMarg *g, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL(k_margins<decltype(nl)::value>, dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, *g); });
}
}
// The conditioned margins (phx_margins.inc): k_sssp_rev and k_margins under a policy Mg whose DMarg part is the run's (the out-edge CSR) —
// MgCond with DRmarg for the re-annotation margins (§21), MgPin with DPmarg for the contigs solved under the required policy (§24) —
// behind the policy's own apply kernel.
template <class Mg, class R> static Mg mg_args(const DMarg *g, const DReann *q, const R *r) { Mg c; static_cast<DMarg &>(c) = *g; c.q = *q; c.r = *r; return c; }
static auto mg_apply_kernel(const DRmarg *) { return k_rmg_apply; }
static auto mg_apply_kernel(const DPmarg *) { return k_pmg_apply; }
template <class R> static void mg_apply(const DBatch *b, const DMarg *g, const DReann *q, const R *r, void *stream) {
    hipLaunchKernelGGL(mg_apply_kernel(r), dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, *g, *q, *r);
}
template <class Mg, class R> static void mg_rev(const DBatch *b, const DMarg *g, const DReann *q, const R *r, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_sssp_rev<decltype(nl)::value, Mg>), dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b, mg_args<Mg>(g, q, r)); });
}
template <class Mg, class R> static void mg_records(const DBatch *b, const DMarg *g, const DReann *q, const R *r, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_margins<decltype(nl)::value, Mg>), dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, mg_args<Mg>(g, q, r)); });
}
// The gene drop margins (phx_drop.inc) and the drop replacements (phx_replace.inc) under a policy G, a workgroup per contig and the argument
// block by value: DMarg on the run's graph (§12, §13); MgDrop on a re-annotation's (§29, §30) — the run's graph and out-edge CSR, the
// re-annotation's policy, d_s', d_t' and path (qpath: its path buffer, laid out like DBatch.path); MgPinDrop for the contigs solved under the
// required policy (§32, §33) — values on one limb more, DPmarg's d_t' and bitmaps, `lost` one int32 per record of the DDrop set, parallel to
// DDrop.rec, written by k_dp_rec alone.
static MgDrop dp_args(const DMarg *g, const DReann *rq, const DRmarg *r, const int32_t *qpath) { MgDrop c = mg_args<MgDrop>(g, rq, r); c.path = qpath; return c; }
static MgPinDrop pdp_args(const DMarg *g, const DReann *rq, const DPmarg *r, const int32_t *qpath, int32_t *lost) { MgPinDrop c = mg_args<MgPinDrop>(g, rq, r); c.path = qpath; c.lost = lost; return c; }
// fn(the argument block of family 0: the run's, 1: the re-annotation's, 2: the pinned)
template <class F> static void with_family(int family, const DMarg *g, const DCondView *v, F fn) {
    if (family == 0) fn(*g);
    else if (family == 1) fn(dp_args(g, v->rq, v->r, v->qpath));
    else fn(pdp_args(g, v->rq, v->p, v->qpath, v->lost));
}
// step 0: trees + labels, 1: candidates + sparse table, 2: saturated slots, cross nodes, records; one launch per limb class and kernel
template <class G> static void dp_step(int step, const DBatch *b, const G &args, const DDrop *q, int nl_mask, hipStream_t s) {
    const dim3 grid(b->n_contig), block(NT);
    if (step == 0) each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_dp_tree<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q); });
    else if (step == 1) each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_dp_cand<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q); });
    else {
        each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_dp_rescan<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q); });
        each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_dp_cross<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q); });
        each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_dp_rec<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q); });
    }
}
// step 0: winners, 1: cross winners and their delta chains, 2: detour lengths, 3: detours, genes, records (the walks: one launch for every class)
template <class G> static void rp_step(int step, const DBatch *b, const G &args, const DDrop *q, const DRepl *r, int nl_mask, hipStream_t s) {
    const dim3 grid(b->n_contig), block(NT);
    if (step == 0) each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_rp_pick<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q, *r); });
    else if (step == 1) each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_rp_cross<decltype(nl)::value, G>), grid, block, 0, s, *b, args, *q, *r); });
    // (k_rp_walk<1> is named ahead of <0>, as it always was: the order of instantiation is the order of the symbols in the code object)
    else if (step == 3) hipLaunchKernelGGL((k_rp_walk<1, G>), grid, block, 0, s, *b, args, *q, *r);
    else hipLaunchKernelGGL((k_rp_walk<0, G>), grid, block, 0, s, *b, args, *q, *r);
}
extern "C" {
void phxk_remarg_apply(const DBatch *b, const DMarg *g, const DReann *q, const DRmarg *r, void *stream) { mg_apply(b, g, q, r, stream); }
void phxk_remarg_rev(const DBatch *b, const DMarg *g, const DReann *q, const DRmarg *r, int nl_mask, void *stream) { mg_rev<MgCond>(b, g, q, r, nl_mask, stream); }
void phxk_remarg_records(const DBatch *b, const DMarg *g, const DReann *q, const DRmarg *r, int nl_mask, void *stream) { mg_records<MgCond>(b, g, q, r, nl_mask, stream); }
void phxk_pinmarg_apply(const DBatch *b, const DMarg *g, const DReann *q, const DPmarg *r, void *stream) { mg_apply(b, g, q, r, stream); }
void phxk_pinmarg_rev(const DBatch *b, const DMarg *g, const DReann *q, const DPmarg *r, int nl_mask, void *stream) { mg_rev<MgPin>(b, g, q, r, nl_mask, stream); }
void phxk_pinmarg_records(const DBatch *b, const DMarg *g, const DReann *q, const DPmarg *r, int nl_mask, void *stream) { mg_records<MgPin>(b, g, q, r, nl_mask, stream); }
// gene drop margins (§12), the re-annotation's (§29) and the pinned (§32): one step of family `family` on its DDrop set q
void phxk_drop_step(int family, int step, const DBatch *b, const DMarg *g, const DCondView *v, const DDrop *q, int nl_mask, void *stream) {
    with_family(family, g, v, [&](const auto &args) { dp_step(step, b, args, q, nl_mask, (hipStream_t)stream); });
}
// coding profiles (phx_profile.inc): a workgroup per contig and limb class for the tables, then a thread per slot
void phxk_profile_cand(const DBatch *b, const DMarg *g, const DProf *q, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL(k_pf_cand<decltype(nl)::value>, dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b, *g, *q); });
}
void phxk_profile_rec(const DBatch *b, const DMarg *g, const DProf *q, void *stream) {
    hipLaunchKernelGGL(k_pf_rec<DMarg>, dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, *g, *q);
}
// re-annotation profiles (§36): the same two under MgCond, on the graph and distances the last re-annotation and its margins left resident
void phxk_reprofile_cand(const DBatch *b, const DMarg *g, const DReann *rq, const DRmarg *r, const DProf *q, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_pf_cand<decltype(nl)::value, MgCond>), dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b, mg_args<MgCond>(g, rq, r), *q); });
}
void phxk_reprofile_rec(const DBatch *b, const DMarg *g, const DReann *rq, const DRmarg *r, const DProf *q, void *stream) {
    hipLaunchKernelGGL(k_pf_rec<MgCond>, dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, mg_args<MgCond>(g, rq, r), *q);
}
// pinned profiles (§37): the same two under MgPinProf, for the contigs solved under the required policy — values on one limb more, `lost`
// three int32 per slot parallel to DProf.rec, `rounds` one int32 per contig, both written by k_pf_cand alone
static MgPinProf ppf_args(const DMarg *g, const DReann *rq, const DPmarg *r, int32_t *lost, int32_t *rounds) { MgPinProf c = mg_args<MgPinProf>(g, rq, r); c.lost = lost; c.rounds = rounds; return c; }
void phxk_pinprofile_cand(const DBatch *b, const DMarg *g, const DReann *rq, const DPmarg *r, const DProf *q, int32_t *lost, int32_t *rounds, int nl_mask, void *stream) {
    each_limb_class(nl_mask, [&](auto nl) { hipLaunchKernelGGL((k_pf_cand<decltype(nl)::value, MgPinProf>), dim3(b->n_contig), dim3(NT), 0, (hipStream_t)stream, *b, ppf_args(g, rq, r, lost, rounds), *q); });
}
void phxk_pinprofile_rec(const DBatch *b, const DMarg *g, const DReann *rq, const DPmarg *r, const DProf *q, void *stream) {
    hipLaunchKernelGGL(k_pf_rec<MgPinProf>, dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, ppf_args(g, rq, r, nullptr, nullptr), *q);
}
// drop replacements (§13), the re-annotation's (§30) and the pinned (§33): one step of family `family` on its DDrop set q (with the one-hop
// trees: the walk follows DDrop.ps / ts and is launched only behind a k_dp_tree of the same family that wrote them) and its DRepl set r
void phxk_repl_step(int family, int step, const DBatch *b, const DMarg *g, const DCondView *v, const DDrop *q, const DRepl *r, int nl_mask, void *stream) {
    with_family(family, g, v, [&](const auto &args) { rp_step(step, b, args, q, r, nl_mask, (hipStream_t)stream); });
}
size_t phxk_sssp_lds_bytes(int V, int nl) { return sssp_lds_bytes(V, nl); }
// re-annotation (phx_resolve.inc): b is the re-annotation's view of the batch (outputs of its own)
void phxk_reann_mask(const DBatch *b, const DReann *q, void *stream) { hipLaunchKernelGGL(k_rs_mask, dim3(b->n_contig, ysplit(b, 8)), dim3(NT), 0, (hipStream_t)stream, *b, *q); }
void phxk_reann_solve(const DBatch *b, const DReann *q, const int *nl_masks, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = (unsigned)b->n_contig;
    re_solve<RePol<false, false>>(b, q, g, nl_masks[1], s);
    re_solve<RePol<true, false>>(b, q, g, nl_masks[2], s);
    re_solve<RePol<false, true>>(b, q, g, nl_masks[3], s);
    re_solve<RePol<true, true>>(b, q, g, nl_masks[4], s);
}
void phxk_reann_finish(const DBatch *b, const DReann *q, const int *nl_masks, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const unsigned g = (unsigned)b->n_contig;
    re_inorder_launch<RePol<false, false>>(b, q, g, nl_masks[1], s);
    re_inorder_launch<RePol<true, false>>(b, q, g, nl_masks[2], s);
    re_inorder_launch<RePol<false, true>>(b, q, g, nl_masks[3], s);
    re_inorder_launch<RePol<true, true>>(b, q, g, nl_masks[4], s);
    hipLaunchKernelGGL(k_rs_fin, dim3((g + 63) / 64), dim3(64), 0, s, *b, *q);
}
// scenario batches: the grids are a range's slots (pairs and triples for the mask kernels), not the batch's contigs
void phxk_scen_mask(const DBatch *b, const DScen *q, const int *n_range, int max_list, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (q->n_slot <= 0) return;
    hipLaunchKernelGGL(k_sc_meta, dim3((unsigned)q->n_slot), dim3(64), 0, s, *b, *q);
    if (q->n_pair > 0) hipLaunchKernelGGL(k_sc_mask, dim3((unsigned)((q->n_pair + NT - 1) / NT)), dim3(NT), 0, s, *b, *q);
    if (n_range[1] + n_range[3] > 0 && q->n_rpair > 0) hipLaunchKernelGGL(k_scp_mask, dim3((unsigned)((q->n_rpair + NT - 1) / NT)), dim3(NT), 0, s, *b, *q);
    const int n_listed = n_range[2] + n_range[3]; // the "both" slots sit directly behind the biased ones: one launch sorts the lists of both ranges
    if (n_listed <= 0 || q->n_trip <= 0) return;
    hipLaunchKernelGGL(k_sce_mask, dim3((unsigned)((q->n_trip + NT - 1) / NT)), dim3(NT), 0, s, *b, *q);
    if (max_list > 1) hipLaunchKernelGGL(k_sce_sort, dim3((unsigned)n_listed, (unsigned)std::min((max_list + NT - 1) / NT, 16)), dim3(NT), 0, s, scen_range(*q, n_range, 2)); // (up to 16 workgroups share the longest list)
}
void phxk_scen_solve(const DBatch *b, const DScen *q, const int *n_range, const int *nl_masks, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const DScen plain = scen_range(*q, n_range, 0), pinned = scen_range(*q, n_range, 1), biased = scen_range(*q, n_range, 2), both = scen_range(*q, n_range, 3);
    re_solve<RePol<false, false>>(b, &plain, (unsigned)n_range[0], nl_masks[0], s);
    re_solve<RePol<true, false>>(b, &pinned, (unsigned)n_range[1], nl_masks[1], s);
    re_solve<RePol<false, true, true>>(b, &biased, (unsigned)n_range[2], nl_masks[2], s);
    re_solve<RePol<true, true, true>>(b, &both, (unsigned)n_range[3], nl_masks[3], s);
}
void phxk_scen_finish(const DBatch *b, const DScen *q, const int *n_range, const int *nl_masks, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (q->n_slot <= 0) return;
    const DScen plain = scen_range(*q, n_range, 0), pinned = scen_range(*q, n_range, 1), biased = scen_range(*q, n_range, 2), both = scen_range(*q, n_range, 3);
    re_inorder_launch<RePol<false, false>>(b, &plain, (unsigned)n_range[0], nl_masks[0], s);
    re_inorder_launch<RePol<true, false>>(b, &pinned, (unsigned)n_range[1], nl_masks[1], s);
    re_inorder_launch<RePol<false, true, true>>(b, &biased, (unsigned)n_range[2], nl_masks[2], s);
    re_inorder_launch<RePol<true, true, true>>(b, &both, (unsigned)n_range[3], nl_masks[3], s);
    hipLaunchKernelGGL(k_sc_fin, dim3((unsigned)((q->n_slot + 63) / 64)), dim3(64), 0, s, *b, *q);
}
// one workgroup for up to 1024 contigs; larger batches in two passes of a workgroup per 256 contigs
void phxk_layout1(const DBatch *b, void *stream) {
    if (b->n_contig <= LAYOUT_T) { hipLaunchKernelGGL(k_layout1, dim3(1), dim3(LAYOUT_T), 0, (hipStream_t)stream, *b); return; }
    const unsigned g = (unsigned)((b->n_contig + LMB_T - 1) / LMB_T);
    hipLaunchKernelGGL(k_layout1_a, dim3(g), dim3(LMB_T), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_layout1_b, dim3(g), dim3(LMB_T), 0, (hipStream_t)stream, *b);
}
void phxk_layout2(const DBatch *b, void *stream) {
    if (b->n_contig <= LAYOUT_T) { hipLaunchKernelGGL(k_layout2, dim3(1), dim3(LAYOUT_T), 0, (hipStream_t)stream, *b); return; }
    const unsigned g = (unsigned)((b->n_contig + LMB_T - 1) / LMB_T);
    hipLaunchKernelGGL(k_layout2_a, dim3(g), dim3(LMB_T), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL(k_layout2_b, dim3(g), dim3(LMB_T), 0, (hipStream_t)stream, *b);
}

void phxk_sssp_order(const DBatch *b, void *stream) { hipLaunchKernelGGL(k_sssp_order, dim3(1), dim3(LMB_T), 0, (hipStream_t)stream, *b); }

int phxk_sssp_wave_ok(int nl) { return nl == 2 || nl == 4 || nl == 8; }
// windows and lane assignments of k_sssp_wave (needs the node records and in-edge offsets, not the edges); wide_too: the batch
// (may) hold 256-bit contigs for the wavefront kernel, whose lanes keep fewer in-edges
void phxk_wave_plan(const DBatch *b, int wide_too, void *stream) {
    if (b->seg) hipLaunchKernelGGL((k_wave_plan<2, 0, true>), dim3(b->n_contig * b->seg), dim3(64), 0, (hipStream_t)stream, *b); // one wavefront per segment
    else hipLaunchKernelGGL((k_wave_plan<2, 0>), dim3(b->n_contig), dim3(64), 0, (hipStream_t)stream, *b);
    hipLaunchKernelGGL((k_wave_plan<2, 1>), dim3(b->n_contig), dim3(64), 0, (hipStream_t)stream, *b); // the contigs the tight configuration could not take
    if (wide_too & 1) hipLaunchKernelGGL((k_wave_plan<4, 1>), dim3(b->n_contig), dim3(64), 0, (hipStream_t)stream, *b);
    if (wide_too & 2) hipLaunchKernelGGL((k_wave_plan<8, 1>), dim3(b->n_contig), dim3(64), 0, (hipStream_t)stream, *b);
}

// mode 0: global-memory kernel (+ k_path); mode 1: workgroup-per-contig LDS kernel with `lds_bytes` of dynamic LDS;
// mode 2: wavefront-per-contig kernel (contigs it hands back carry their fallback mode in sssp_mode afterwards); mode 3: the same
// kernel in its roomy configuration (128-bit contigs that k_wave_plan could not lay out in the tight one)
void phxk_sssp(const DBatch *b, int nl, int mode, size_t lds_bytes, void *stream) {
    dim3 g(b->n_contig), t(NT);
    hipStream_t s = (hipStream_t)stream;
    // k_sssp_duo reads the weights of the coded gap edges from the contig's gap table; every other solver kernel reads plain (source, weight) rows:
    // k_sssp_lds and k_sssp complete DBatch.ew of the contigs they take themselves (expand_contig), k_sssp_wave gets it completed by a launch in front of it
    if ((mode == 2 || mode == 3) && !(mode == 2 && nl == 2 && b->duo) && b->gtab && b->gap_code) phxk_edges_expand(b, nl, mode, stream);
    if (mode == 2 || mode == 3) {
        if (nl == 2 && mode == 2 && b->duo) { // two wavefronts per contig: the feeder prepares the windows, the solver runs the phases (phx_sssp_duo.inc).
            // (The roomy configuration — the few contigs whose windows need more spill entries than the tight one holds — stays with k_sssp_wave<2, 1>.)
            dim3 t2(128);
            if (b->seg && b->seg_stream) hipLaunchKernelGGL((k_sssp_duo<0, true, true>), dim3(b->n_contig * b->seg), t2, 0, s, *b); // ... beside their planner wavefronts
            else if (b->seg) hipLaunchKernelGGL((k_sssp_duo<0, false, true>), dim3(b->n_contig * b->seg), t2, 0, s, *b); // a wavefront pair per segment (phx_sssp_seg.inc)
            else if (b->plan_stream == 2) hipLaunchKernelGGL((k_sssp_duo<0, true>), g, t2, 0, s, *b);
            else hipLaunchKernelGGL((k_sssp_duo<0, false>), g, t2, 0, s, *b);
        } else if (nl == 2 && mode == 2) launch_wave<2, 0, true>(b, b->plan_stream == 2, s); // small batches: beside k_wave_plan<2,0>, following its counter
        else if (nl == 2) launch_wave<2, 1, false>(b, false, s);
        else if (nl == 4) launch_wave<4, 1, true>(b, b->plan_stream == 4, s);
        else launch_wave<8, 1, true>(b, b->plan_stream == 8, s);
        return;
    }
    if (mode == 0) {
        dim3 gp((b->n_contig + 63) / 64), tp(64);
        each_limb_class(limb_class_bit(nl), [&](auto c) {
            hipLaunchKernelGGL(k_sssp<decltype(c)::value>, g, t, 0, s, *b);
            hipLaunchKernelGGL(k_path<decltype(c)::value>, gp, tp, 0, s, *b);
        });
        return;
    }
    each_limb_class(limb_class_bit(nl), [&](auto c) { launch_lds(k_sssp_lds<decltype(c)::value>, lds_bytes, (unsigned)b->n_contig, s, *b, mode, (int)lds_bytes); });
}
}

