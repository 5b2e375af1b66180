// phx_sssp_wave.inc — exact shortest path, one wavefront per contig (included by phx_kernels.hip).
//
// Why one wavefront: the relaxation is a chain of small dependent steps (a window of ~90 nodes, ~9 half-rounds
// each); with a workgroup per contig every half-round paid a barrier and 8 wavefronts' worth of reduction
// instructions.  Here a contig is one wavefront: no barriers, the window's in-edges live in registers, the
// distances of the last 512 nodes in an LDS ring, and a batch of 1000 contigs is 1000 independent wavefronts
// (one per SIMD) that are all resident at once.
//
// Schedule (same fixed point as k_sssp / k_sssp_lds, fastpathz semantics phanotate.py:56-64):
//  * Nodes are position-sorted.  A window [v0,v1) = up to 64 nodes to advance by + every node of the next
//    500 bp (every connector edge that points backwards spans < 500 bp, functions.py:372); at most 64 close
//    nodes (forward stops / reverse starts: targets of ORF edges) and 64 open nodes (targets of connectors).
//  * The graph is bipartite close/open, so a round = phase A (all close nodes) + phase B (all open nodes), each
//    node taking the minimum over all its in-edges; a phase that changes nothing ends the window.
//  * Lanes are assigned per phase to (node, chunk of <= CA / CB in-edges); nodes with more in-edges get helper
//    lanes (partial minima are combined by a log-step segmented minimum over ds_bpermute) and, beyond that, a spill
//    list in LDS; the planner sizes a window so that both phases fit 64 lanes.
//  * After a window has converged its advance nodes are final unless a close node near the window start (one
//    that already-final open nodes may depend on through a backward edge) has just improved; in that case the
//    sweep steps back to the first node that could be affected and continues from there (rare: ~0.3 per 50 kb
//    contig).  No separate verification pass is needed: forward edges see final sources by construction, and
//    every backward edge's source is re-checked by this rule each time it changes.
//  * The parent of a node is its lowest-index in-edge that attains the minimum (the canonical tie-break of the
//    other kernels), recorded as an edge index when the node is advanced and resolved by the path walk.
//  * The windows and the lane assignment do not depend on distances: k_wave_plan lays them out beforehand (beside
//    k_edges<true>); k_sssp_wave loads a window's records.  Window k+1's in-edges and lane records are DMA'd
//    (global_load_lds) into LDS while window k iterates.
//  * While all weights and distances in play are narrow the phases run in 64-bit arithmetic (phase64).
// A contig these kernels cannot take (a single node's 500 bp neighbourhood exceeds a window, spill overflow, no
// convergence) is handed on by setting sssp_mode = sssp_fb (k_sssp_lds, or k_sssp for huge contigs); the launcher
// runs those kernels right after on the same stream.

typedef unsigned __int128 wv_u128;
#ifndef WV_CA
#define WV_CA 4 // in-edges a lane of the close-node phase keeps (a multiple of 4)
#endif
#ifndef WV_ADV
#define WV_ADV 64
#endif
#define WV_WIN 128
#define WV_META 192
#ifndef WV_WPE
#define WV_WPE 2 // wavefronts per SIMD the register allocation of k_sssp_wave must allow: 256 registers, so that two 128-register
                 // wavefronts of another context's kernels fit beside it
#endif
// Per integer width and configuration: slots of the distance ring, entries of the spill list, in-edges a window may stage.
//  * CFG 0 (128-bit contigs only), "tight": 29 KB of LDS per wavefront, so that beside the four wavefronts of a CU (one per SIMD) a 40 KB
//    workgroup of another batch's k_edges<true> / k_features still fits (two batches in flight, pipeline.py);
//  * CFG 1, "roomy": just under 40 KB, for the few contigs whose windows need more in-edges or spill entries than that (k_wave_plan
//    decides: DMeta.sssp_mode 2 -> 3), and for the 256-bit contigs.
template <int NL, int CFG> struct WvDims;
#ifndef WV_T_RING
#define WV_T_RING 512
#define WV_T_OV 192
#define WV_T_ECAP 1024
#endif
template <> struct WvDims<2, 0> { static constexpr int RING = WV_T_RING, OV = WV_T_OV, ECAP = WV_T_ECAP, MODE = 2; };
template <> struct WvDims<2, 1> { static constexpr int RING = 512, OV = 512, ECAP = 1280, MODE = 3; };
#ifndef WV_W_RING // 256-bit contigs: with 64-bit cached weights the LDS goes to a full 512-slot ring (fewer folded sources) rather than to staging
#define WV_W_RING 512
#define WV_W_OV 224
#define WV_W_ECAP 768
#endif
template <> struct WvDims<8, 1> { static constexpr int RING = 256, OV = 448, ECAP = 768, MODE = 2; }; // (OV: a stop node behind a 9000-codon ORF collects an in-edge from every in-frame start: ~450 at 5 % starts; 59 KB — 512-bit contigs are too few per batch for their LDS to matter)
template <> struct WvDims<4, 1> { static constexpr int RING = WV_W_RING, OV = WV_W_OV, ECAP = WV_W_ECAP, MODE = 2; };
#define WV_POS_INF 0x3fffffff
#define WV_PLAN_DONE (1 << 30) // DMeta.plan_prog: the planner has finished (low bits: the number of windows)
#ifndef WV_PLAN_SPINS
#define WV_PLAN_SPINS 20000    // polls (an acquire load at agent scope + s_sleep 4: 1.4 us each, measured with the silent planner of tools/nopub_check.py, i.e. ~28 ms) after which k_sssp_wave stops waiting for the planner and hands the contig on
#endif
#define WV_NARROW (1ll << 55)                // relative ring: real entries are |d - base| < 2^55
#define WV_BIAS (1ll << 58)
#define WV_REL(v) (((long long)(v) + WV_BIAS) << 4) // entry of the relative ring for the relative value v (low 4 bits free)
// (RING + 2 slots: the ring + the constant 0 of the source + a constant "unreached" that pads a lane's in-edge list)
#define WV_VAL_BIG (1ll << 57)               // relative value that stands for "unreached",
#define WV_VAL_WIDE (1ll << 56)              //   for a real distance that does not fit base +- 2^55
#define WV_REL_BIG WV_REL(WV_VAL_BIG)
#define WV_REL_WIDE WV_REL(WV_VAL_WIDE)

template <int NL>
struct WvNum;
// 128-bit two's complement as two 64-bit halves.  Written with 64-bit adds and three independent compares
// (no v_addc/v_subb carry chains): a wavefront that has its SIMD to itself is bound by dependent-issue latency,
// and carry chains through VCC serialise and need wait states on gfx950.
struct Wv2 { uint64_t lo, hi; };
template <>
struct WvNum<2> {
    typedef Wv2 T;
    static constexpr int CA = WV_CA, CB = 16;
    static __device__ __forceinline__ T load(const void *p) { const uint4 v = *(const uint4 *)p; T r; r.lo = ((uint64_t)v.y << 32) | v.x; r.hi = ((uint64_t)v.w << 32) | v.z; return r; }
    static __device__ __forceinline__ void store(void *p, T x) { *(uint4 *)p = make_uint4((uint32_t)x.lo, (uint32_t)(x.lo >> 32), (uint32_t)x.hi, (uint32_t)(x.hi >> 32)); }
    static __device__ __forceinline__ T add(T a, T b) { T r; r.lo = a.lo + b.lo; r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull); return r; }
    static __device__ __forceinline__ bool lt(T a, T b) { return ((int64_t)a.hi < (int64_t)b.hi) | ((a.hi == b.hi) & (a.lo < b.lo)); }
    static __device__ __forceinline__ T sel(bool c, T a, T b) { T r; r.lo = c ? a.lo : b.lo; r.hi = c ? a.hi : b.hi; return r; }
    static __device__ __forceinline__ T zero() { T r; r.lo = 0; r.hi = 0; return r; }
    // "unreached" = 2^126 + 2^62 and "above every candidate": the low halves alone play the same roles for the
    // 64-bit phases (k_sssp_wave: narrow windows), so one ring and one set of cached weights serve both
    static __device__ __forceinline__ T big() { T r; r.lo = WBIG_TOP; r.hi = WBIG_TOP; return r; }
    static __device__ __forceinline__ T top() { T r; r.lo = 0x6000000000000000ull; r.hi = 0x6000000000000000ull; return r; }
    static __device__ __forceinline__ bool unreached(T a) { return (int64_t)a.hi >= (int64_t)0x2000000000000000ll; }
    // x integer-valued, |x| < 2^125
    static __device__ __forceinline__ T from_double(double x) {
        const uint64_t bits = (uint64_t)__double_as_longlong(x);
        const int ef = (int)((bits >> 52) & 0x7ff);
        const uint64_t m = ef ? ((bits & 0xfffffffffffffull) | (1ull << 52)) : 0ull;
        const int e = ef - 1075; // value = m * 2^e, -1075 <= e < 73
        const int sl = e < 0 ? 0 : e, sr = e < 0 ? (e > -64 ? -e : 63) : 0;
        wv_u128 r = (wv_u128)(m >> sr) << sl;
        if (e <= -64) r = 0;
        if (bits >> 63) r = (wv_u128)0 - r;
        T t; t.lo = (uint64_t)r; t.hi = (uint64_t)(r >> 64);
        return t;
    }
    // the same for |x| < 2^51 (nearly every edge): adding 1.5 * 2^52 leaves the integer in the low mantissa bits,
    // a 64-bit subtraction of the constant's bit pattern extracts it (no fp64 -> int64 conversion sequence)
    static __device__ __forceinline__ bool small(double x) { return fabs(x) < 2251799813685248.0; }
    static __device__ __forceinline__ T from_small(double x) {
        const long long v = __double_as_longlong(x + 6755399441055744.0) - 0x4338000000000000ll;
        T t; t.lo = (uint64_t)v; t.hi = (uint64_t)(v >> 63);
        return t;
    }
    static __device__ __forceinline__ T from_i64(long long v) { T t; t.lo = (uint64_t)v; t.hi = (uint64_t)(v >> 63); return t; }
    static __device__ __forceinline__ T with_lo64(T a, uint64_t lo) { a.lo = lo; return a; }
    static __device__ __forceinline__ uint64_t lo64(T a) { return a.lo; }
    static __device__ __forceinline__ T sub(T a, T b) { T x; x.lo = a.lo - b.lo; x.hi = a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull); return x; }
    static __device__ __forceinline__ bool is_i64(T x) { return x.hi == (uint64_t)((int64_t)x.lo >> 63); } // the value fits 64 bits
    static __device__ __forceinline__ bool negative(T x) { return (int64_t)x.hi < 0; }
    template <class F>
    static __device__ __forceinline__ T map32(T a, F f) { // f on every 32-bit half (lane shuffles)
        T c;
        c.lo = ((uint64_t)(uint32_t)f((int)(a.lo >> 32)) << 32) | (uint32_t)f((int)a.lo);
        c.hi = ((uint64_t)(uint32_t)f((int)(a.hi >> 32)) << 32) | (uint32_t)f((int)a.hi);
        return c;
    }
};

// 256-bit two's complement, four 64-bit limbs: contigs with an ORF of ~2000 codons or more (weights beyond 2^100).  Same kernel:
// most of their phases still run on the 64-bit relative ring; the exact phases are four limbs wide.  Same lanes and windows as the
// 128-bit kernel (16 cached in-edges per lane of the open-node phase: the compiler parks ~30 of the 320 live values in AGPRs,
// which a lone wavefront per SIMD has to spare; with 8 or 12 per lane the spill list overflowed on ordinary windows), half the ring.
template <int K> struct WvK { uint64_t v[K]; };
template <int K>
struct WvNumK {
    typedef WvK<K> T;
    static constexpr int CA = WV_CA, CB = 16;
    static_assert(K % 2 == 0, "16-byte pieces");
    static __device__ __forceinline__ T load(const void *p) {
        T r;
#pragma unroll
        for (int i = 0; i < K; i += 2) { const uint4 a = ((const uint4 *)p)[i / 2]; r.v[i] = ((uint64_t)a.y << 32) | a.x; r.v[i + 1] = ((uint64_t)a.w << 32) | a.z; }
        return r;
    }
    static __device__ __forceinline__ void store(void *p, T x) {
#pragma unroll
        for (int i = 0; i < K; i += 2) ((uint4 *)p)[i / 2] = make_uint4((uint32_t)x.v[i], (uint32_t)(x.v[i] >> 32), (uint32_t)x.v[i + 1], (uint32_t)(x.v[i + 1] >> 32));
    }
    static __device__ __forceinline__ T add(T a, T b) {
        T r; uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < K; i++) { const uint64_t s1 = a.v[i] + b.v[i]; const uint64_t s2 = s1 + c; c = (s1 < a.v[i] ? 1ull : 0ull) | (s2 < s1 ? 1ull : 0ull); r.v[i] = s2; }
        return r;
    }
    static __device__ __forceinline__ T sub(T a, T b) {
        T r; uint64_t br = 0;
#pragma unroll
        for (int i = 0; i < K; i++) { const uint64_t d1 = a.v[i] - b.v[i]; const uint64_t d2 = d1 - br; br = (a.v[i] < b.v[i] ? 1ull : 0ull) | (d1 < br ? 1ull : 0ull); r.v[i] = d2; }
        return r;
    }
    static __device__ __forceinline__ bool lt(T a, T b) {
        bool l = a.v[0] < b.v[0];
#pragma unroll
        for (int i = 1; i < K - 1; i++) l = (a.v[i] < b.v[i]) | ((a.v[i] == b.v[i]) & l);
        return ((int64_t)a.v[K - 1] < (int64_t)b.v[K - 1]) | ((a.v[K - 1] == b.v[K - 1]) & l);
    }
    static __device__ __forceinline__ T sel(bool c, T a, T b) { T r;
#pragma unroll
        for (int i = 0; i < K; i++) r.v[i] = c ? a.v[i] : b.v[i];
        return r; }
    static __device__ __forceinline__ T zero() { T r;
#pragma unroll
        for (int i = 0; i < K; i++) r.v[i] = 0;
        return r; }
    static __device__ __forceinline__ T big() { T r = zero(); r.v[0] = WBIG_TOP; r.v[K - 1] = WBIG_TOP; return r; }
    static __device__ __forceinline__ T top() { T r = zero(); r.v[0] = 0x6000000000000000ull; r.v[K - 1] = 0x6000000000000000ull; return r; }
    static __device__ __forceinline__ bool unreached(T a) { return (int64_t)a.v[K - 1] >= (int64_t)0x2000000000000000ll; }
    static __device__ __forceinline__ T from_double(double x) { const WInt<K> w = wi_from_double<K>(x); T t;
#pragma unroll
        for (int i = 0; i < K; i++) t.v[i] = w.v[i];
        return t; }
    static __device__ __forceinline__ bool small(double x) { return fabs(x) < 2251799813685248.0; }
    static __device__ __forceinline__ T from_i64(long long v) { T t; t.v[0] = (uint64_t)v;
#pragma unroll
        for (int i = 1; i < K; i++) t.v[i] = (uint64_t)(v >> 63);
        return t; }
    static __device__ __forceinline__ T with_lo64(T a, uint64_t lo) { a.v[0] = lo; return a; }
    static __device__ __forceinline__ T from_small(double x) { return from_i64(__double_as_longlong(x + 6755399441055744.0) - 0x4338000000000000ll); }
    static __device__ __forceinline__ uint64_t lo64(T a) { return a.v[0]; }
    static __device__ __forceinline__ bool is_i64(T x) { const uint64_t sx = (uint64_t)((int64_t)x.v[0] >> 63); bool r = true;
#pragma unroll
        for (int i = 1; i < K; i++) r = r & (x.v[i] == sx);
        return r; }
    static __device__ __forceinline__ bool negative(T x) { return (int64_t)x.v[K - 1] < 0; }
    template <class F>
    static __device__ __forceinline__ T map32(T a, F f) {
        T c;
#pragma unroll
        for (int i = 0; i < K; i++) c.v[i] = ((uint64_t)(uint32_t)f((int)(a.v[i] >> 32)) << 32) | (uint32_t)f((int)a.v[i]);
        return c;
    }
};
template <> struct WvNum<4> : WvNumK<4> {};
template <> struct WvNum<8> : WvNumK<8> {}; // 512-bit contigs (an ORF of ~4000-9000 codons)

// LDS DMA (global_load_lds): every active lane moves 16 (4) bytes from its global address to l + 16 (4) * lane.
// Issued as inline assembly on purpose: through the builtin the compiler orders every later LDS read behind the
// transfer (s_waitcnt vmcnt(0) in front of the first ds_read), which serialises the prefetch of window k+1 with
// the phases of window k.  The kernels wait themselves (s_waitcnt 0) before they read a staged block, and drain
// their LDS reads (lgkmcnt(0)) before a block is overwritten.
__device__ __forceinline__ void wv_dma16(const void *g, void *l) {
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)l);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(base), "v"(g) : "memory", "m0");
}
__device__ __forceinline__ void wv_dma4(const void *g, void *l) {
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)l);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" ::"s"(base), "v"(g) : "memory", "m0");
}
// inclusive wavefront sum-scan on the DPP network (no LDS round trips): shifts inside the rows of 16, then the
// row totals are broadcast into the following rows (row_bcast:15 / row_bcast:31, gfx9 encodings)
__device__ __forceinline__ uint32_t wv_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ int wv_last(int v) { return __builtin_amdgcn_readlane(v, 63); }
// lane i takes lane i+1's value (DPP wave_shl:1; lane 63 gets 0)
__device__ __forceinline__ int wv_next(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }
// the same, lane 63 keeps its own value (no register to preset)
__device__ __forceinline__ int wv_next_self(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xf, 0xf, false); }
// Orders the LDS accesses of the lanes of one wavefront: what any lane wrote before is visible to every lane after.
// (The hardware executes a wavefront's LDS instructions in order; this keeps the compiler from moving or sinking them
// across the point, e.g. into the two sides of a divergent branch.)
__device__ __forceinline__ void wv_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// wavefront maximum of small non-negative values, same network
__device__ __forceinline__ int wv_max(int x) {
    uint32_t v = (uint32_t)x, o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = o > v ? o : v;
    return __builtin_amdgcn_readlane((int)v, 63);
}

// A cached in-edge weight, in one of two forms.  WvCw<2>, the form of k_sssp_wave's 128-bit contigs, keeps it at the ring's width (two registers
// more per in-edge, and a folded source distance fits).  WvCw64 keeps 64 bits at any ring width — the wider contigs of k_sssp_wave, and
// k_sssp_duo — and is a form with a SIDE list: the few in-edges that do not fit (|W| >= 2^51, or a final distance folded in) go to the side list
// in LDS (k_sssp_wave: gather; k_sssp_duo: the feeder's side).
struct WvCw64 {
    typedef long long CW;
    static constexpr bool SIDE = true;
    static __device__ __forceinline__ CW from_i64(long long v) { return v; }
    template <class N> static __device__ __forceinline__ typename N::T to_T(CW c) { return N::from_i64(c); }
    static __device__ __forceinline__ uint64_t lo(CW c) { return (uint64_t)c; }
    static __device__ __forceinline__ CW with_lo(CW, uint64_t l) { return (long long)l; }
};
template <int NL> struct WvCw : WvCw64 {};
template <> struct WvCw<2> {
    typedef Wv2 CW;
    static constexpr bool SIDE = false;
    static __device__ __forceinline__ CW from_i64(long long v) { return WvNum<2>::from_i64(v); }
    template <class N> static __device__ __forceinline__ Wv2 to_T(CW c) { return c; }
    static __device__ __forceinline__ uint64_t lo(CW c) { return c.lo; }
    static __device__ __forceinline__ CW with_lo(CW c, uint64_t l) { c.lo = l; return c; }
};
// the lanes of one phase: a lane works on (node, chunk of its in-edges)
struct WvLane {
    int sd0, sd1;       // (C::SIDE) this lane's entries of the side list
    int cnt;            // cached in-edges of this lane
    int ebase;          // window-relative index of this lane's first in-edge
    int node;           // window-relative node index, -1: lane idle in this phase
    int ch;             // chunk of the node's in-edge list this lane holds
    bool head;          // first chunk of its node: owns the result
    bool watch;         // head of a close node that already-final open nodes may depend on (see k_wave_plan)
    bool nextf;         // the next lane is a helper of this lane's node
    int nfollow;        // helper lanes that follow a head
    int sp0, sp1;       // head: spill entries (in-edges beyond the helpers)
    int spe;            // window-relative edge index of spill entry sp0
    uint32_t slot;      // head: byte offset of the node's own distance in the ring
    int pe;             // head: window-relative index of the in-edge that attains the minimum
    int maxcnt;         // largest cnt of any lane (wave-uniform)
    int maxfollow;      // wave-uniform
};
// ... and keeps that chunk's in-edges in registers (C: the form of a cached weight).  k_sssp_wave's lanes are WvRoles; k_sssp_duo keeps
// a WvLane and the two arrays beside it: as members of one object they cost its streamed instantiations 136-160 bytes of scratch per
// lane (12 -> 172 / 148), so the phases of WvSolver take (lane, cw, cs)
template <class C, int CAP_>
struct WvRole : WvLane {
    static constexpr int CAP = CAP_;
    typename C::CW cw[CAP]; // cached weights,
    uint32_t cs[CAP];       //   byte offsets of their sources' distances in the ring
};
// A lane's record as k_wave_plan stores it (WIN_ROLES per window: phase A lanes, then phase B lanes):
//   x: node 0..6 | chunk 7..12 | helper lanes 13..18 | cached in-edges 19..23 | active 24 | watch 25
//   y: first in-edge 0..10 | first spill entry 11..20 | spill entries 21..30
__device__ __forceinline__ uint2 wv_role_pack(bool act, int node, int ch, int nfollow, int cnt, bool watch, int ebase, int sp0, int spn) {
    uint2 r;
    r.x = !act ? 0u : ((uint32_t)node | ((uint32_t)ch << 7) | ((uint32_t)nfollow << 13) | ((uint32_t)cnt << 19) | (1u << 24) | (watch ? 1u << 25 : 0u));
    r.y = !act ? 0u : ((uint32_t)ebase | (((uint32_t)sp0 & 1023u) << 11) | (((uint32_t)spn & 1023u) << 21));
    return r;
}
__device__ __forceinline__ int wv_role_node(uint2 rc) { return (int)(rc.x & 127u); }
__device__ __forceinline__ int wv_role_ch(uint2 rc) { return (int)((rc.x >> 7) & 63u); }
__device__ __forceinline__ int wv_role_nfollow(uint2 rc) { return (int)((rc.x >> 13) & 63u); }
__device__ __forceinline__ int wv_role_cnt(uint2 rc) { return (int)((rc.x >> 19) & 31u); }
__device__ __forceinline__ bool wv_role_act(uint2 rc) { return (rc.x >> 24) & 1u; }
__device__ __forceinline__ bool wv_role_watch(uint2 rc) { return (rc.x >> 25) & 1u; }
__device__ __forceinline__ int wv_role_ebase(uint2 rc) { return (int)(rc.y & 2047u); }
__device__ __forceinline__ int wv_role_sp0(uint2 rc) { return (int)((rc.y >> 11) & 1023u); }
__device__ __forceinline__ int wv_role_spn(uint2 rc) { return (int)((rc.y >> 21) & 1023u); }
// a window record's per-phase summary word (k_wave_plan: lanes in use | largest cnt << 8 | most helper lanes << 16)
__device__ __forceinline__ int wv_sum_maxcnt(uint32_t summary) { return (int)((summary >> 8) & 255u); }
__device__ __forceinline__ int wv_sum_maxfollow(uint32_t summary) { return (int)((summary >> 16) & 255u); }

// ------------------------------------------------------------------------------------------------
// k_wave_plan: the part of k_sssp_wave's sweep that does not depend on distances: the sequence of windows and, per
// window and phase, which lane works on which (node, chunk of in-edges).  One wavefront per contig walks the
// position-sorted node records and the in-edge offsets (both exist once the edges are counted), so the launcher
// runs it on a side stream beside k_edges<true>; k_sssp_wave then only loads a window's records.
//  * window that starts at node s: up to 128 candidate nodes; the lane budget (one lane per chunk of CA / CB in-edges,
//    64 lanes per phase), the class capacities (64 close, 64 open nodes) and the staging capacity (ECAP in-edges)
//    bound it; a node may be advanced when every node of its next 500 bp is inside the window.
//  * `watch`: a close node left of pos(v0-1)+500 may be the source of a backward edge into a node that is already
//    final; if such a node improves, k_sssp_wave steps back.
// A contig whose windows cannot be built (a node's 500 bp neighbourhood exceeds a window, too many spill entries,
// more windows than n_node/16 + 7) goes to the workgroup kernel: sssp_mode = sssp_fb.
#define PL_BUF ((WV_META + 4) * 4 + (WV_META + 1) * 16)
// SEG (phx_sssp_seg.inc): one wavefront per SEGMENT of a contig — the windows of the node range [ns, ne) only, laid out from ns as if the
// contig began there, into the segment's own slice of DBatch.swin / swrole; the count goes to DBatch.segw (-1: this segment cannot be laid out)
template <int NL, int CFG, bool SEG = false>
__global__ __launch_bounds__(64) void k_wave_plan(DBatch b) {
    typedef WvDims<NL, CFG> D;
    constexpr int CA = WvNum<NL>::CA, CB = WvNum<NL>::CB, WV_OV = D::OV, WV_ECAP = D::ECAP;
    static_assert(WV_ECAP % 256 == 0, "k_sssp_wave stages whole 1 KB pieces");
    static_assert(!SEG || (NL == 2 && CFG == 0), "segments: the tight 128-bit configuration only");
    __shared__ __align__(16) uint8_t smem[2 * PL_BUF + 2 * 128 + 64 * 16 + 64];
    const int ci = SEG ? (int)blockIdx.x / b.seg : (int)blockIdx.x;
    DMeta *meta = &b.meta[ci];
    const int V = meta->n_node;
    if (b.tot->overflow || meta->status < 0 || V <= 2 || meta->sssp_nl != NL || meta->sssp_mode != D::MODE) return;
    if (!SEG && NL == 2 && CFG == 0 && b.seg && !meta->seg_fail) return; // (DBatch.seg: this launch is the one sweep behind the segments, for the contigs they could not take)
    const int lane = threadIdx.x;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int SRC = V - 2;
    int seg_ns = 0, seg_ne = V;       // the node range this wavefront lays out (SEG: the segment's, margin and overlap included)
    size_t seg_w = 0;                 // (SEG) first window record of the segment
    int32_t *seg_rec = nullptr;       // (SEG) {windows, solver status} of the segment
    if constexpr (SEG) {
        if (V > SEG_VMAX) return;
        const SegGeo geo = seg_geo(b, meta);
        const int sg = (int)blockIdx.x % b.seg;
        if (sg >= geo.K) return;
        int cs_;
        const SegRank rk(b, meta);
        seg_range(geo, rk, V, sg, seg_ns, cs_, seg_ne);
        seg_w = seg_win_off(b, meta, sg);
        seg_rec = b.segw + SEG_REC * (size_t)blockIdx.x;
        if (threadIdx.x == 0) { seg_rec[1] = -1; seg_rec[2] = seg_ns; seg_rec[3] = seg_ne; } // (status: not solved yet; the range, for the record)
    }
    const uint32_t *in_off = b.in_off + meta->node_off + ci;
    const DNode *nd = b.node + meta->node_off;
    const uint32_t *mreach = b.mreach + 4 * (size_t)meta->node_off; // per close node: the lowest head of its overlap edges (k_edges_scan)
    const bool mr_partial = (meta->dense & 2) != 0;                  // ... not known for every edge of this contig: positions decide
    DWin *win = SEG ? b.swin + seg_w : b.win + meta->win_off;
    uint2 *wrole = SEG ? b.swrole + seg_w * WIN_ROLES : b.wrole + (size_t)meta->win_off * WIN_ROLES;
    const int win_cap = V / 16 + 7;

    // two staged blocks of node records ([base, base+META]: in-edge offsets, node records), used alternately
    uint8_t *s_listA = smem + 2 * PL_BUF;                       // close / open nodes of the window, compacted
    uint8_t *s_listB = s_listA + 128;
    uint4 *s_rec = (uint4 *)(s_listB + 128);                    // per node of a phase: its record, written by its owner lane
    uint8_t *s_head = (uint8_t *)(s_rec + 64);                  // marks the first lane of every node of a phase
    auto blk_off = [&](int q) { return (uint32_t *)(smem + (size_t)q * PL_BUF); };
    auto blk_node = [&](int q) { return (const DNode *)(smem + (size_t)q * PL_BUF + (size_t)(WV_META + 4) * 4); };

    // stage the node records of [base, base+META] (the offset loads may run up to 1 KB past the contig: next contig or buffer slack)
    auto stage_meta = [&](int base, int q) {
        uint32_t *m_off = blk_off(q);
        const DNode *m_node = blk_node(q);
        if (4 * lane < WV_META) wv_dma16(in_off + base + 4 * lane, m_off);
        if (lane == 0) wv_dma4(in_off + base + WV_META, m_off + WV_META);
        for (int i = 0; i <= WV_META; i += 64) // records base .. base+META inclusive: plan() reads the one just past a full window
            if (i + lane <= WV_META && base + i + lane < V) wv_dma16(nd + base + i + lane, (void *)(m_node + i)); // one 16-byte node record per lane; nothing is read past the contig
    };
    // window that starts at node s = (first node of block q) + rel, rel <= META - WIN: advance end, window end
    auto plan = [&](int s, int q, int rel, int &pa, int &p1, int &plim) -> bool {
        const uint32_t *m_off = blk_off(q);
        const DNode *m_node = blk_node(q);
        const int c1 = s + lane, c2 = s + 64 + lane;
        const bool in1 = c1 < V, in2 = c2 < V;
        const int i1 = in1 ? m_node[rel + lane].info : 0, i2 = in2 ? m_node[rel + 64 + lane].info : 0;
        const bool k1 = in1 && ((NTYPE(i1) == 1 && NFRAME(i1) > 0) || (NTYPE(i1) == 0 && NFRAME(i1) < 0));
        const bool k2 = in2 && ((NTYPE(i2) == 1 && NFRAME(i2) > 0) || (NTYPE(i2) == 0 && NFRAME(i2) < 0));
        const int p1v = !in1 ? WV_POS_INF : (c1 >= SRC ? WV_POS_INF : m_node[rel + lane].pos);
        const int p2v = !in2 ? WV_POS_INF : (c2 >= SRC ? WV_POS_INF : m_node[rel + 64 + lane].pos);
        const uint64_t mc1 = __ballot(k1), mo1 = __ballot(in1 && !k1), mc2 = __ballot(k2), mo2 = __ballot(in2 && !k2);
        const uint64_t le = below | (1ull << lane);
        const uint32_t eb = m_off[rel];
        const uint32_t f1 = m_off[rel + lane], h1 = m_off[rel + lane + 1], f2 = m_off[rel + 64 + lane], h2 = m_off[rel + 64 + lane + 1];
        // lanes a node needs in its phase: one per chunk of CA (close) / CB (open) in-edges; a phase has 64 lanes.
        // (a single node that needs more than a whole wavefront still gets its own window: the rest goes to the spill list)
        const int d1 = in1 ? (int)(h1 - f1) : 0, d2 = in2 ? (int)(h2 - f2) : 0;
        const int q1 = !in1 ? 0 : (k1 ? (d1 > CA ? (d1 + CA - 1) / CA : 1) : (d1 > CB ? (d1 + CB - 1) / CB : 1));
        const int q2 = !in2 ? 0 : (k2 ? (d2 > CA ? (d2 + CA - 1) / CA : 1) : (d2 > CB ? (d2 + CB - 1) / CB : 1));
        const int qa1 = (int)wv_scan((uint32_t)(k1 ? q1 : 0)), qb1 = (int)wv_scan((uint32_t)(k1 ? 0 : q1));
        const int qa2 = wv_last(qa1) + (int)wv_scan((uint32_t)(k2 ? q2 : 0)), qb2 = wv_last(qb1) + (int)wv_scan((uint32_t)(k2 ? 0 : q2));
        const bool ok1 = in1 && (h1 - eb) <= (uint32_t)WV_ECAP && (lane == 0 || (qa1 <= 64 && qb1 <= 64));
        const bool ok2 = in2 && (h2 - eb) <= (uint32_t)WV_ECAP && qa2 <= 64 && qb2 <= 64 &&
                         __popcll(mc1) + __popcll(mc2 & le) <= 64 && __popcll(mo1) + __popcll(mo2 & le) <= 64;
        // the same without the lane budget (class and staging capacities only): used when the budget would leave a
        // node's 500 bp look-ahead outside the window; the excess then goes to the spill list
        const bool un1 = in1 && (h1 - eb) <= (uint32_t)WV_ECAP;
        const bool un2 = in2 && (h2 - eb) <= (uint32_t)WV_ECAP && __popcll(mc1) + __popcll(mc2 & le) <= 64 && __popcll(mo1) + __popcll(mo2 & le) <= 64;
        int nmax = 0, amax = 0;
        for (int pass = 0; pass < 2; pass++) {
            const uint64_t g1 = __ballot(pass ? un1 : ok1), g2 = __ballot(pass ? un2 : ok2);
            nmax = g1 != ~0ull ? __ffsll((long long)~g1) - 1 : (g2 != ~0ull ? 64 + __ffsll((long long)~g2) - 1 : 128);
            // nodes that may be advanced: their 500 bp look-ahead ends inside [s, s+nmax)
            int lim = 0x7fffffff;
            if (s + nmax < V) { const int qn = s + nmax; lim = qn >= SRC ? WV_POS_INF : m_node[rel + nmax].pos; }
            const uint64_t a1 = __ballot(lane < nmax && p1v + 500 <= lim), a2 = __ballot(64 + lane < nmax && p2v + 500 <= lim);
            amax = __popcll(a1) + __popcll(a2);
            if (s + nmax >= V) amax = nmax;
            if (amax >= 8) break; // a useful window within the lane budget
        }
        const int a = amax < WV_ADV ? amax : WV_ADV;
        if (a <= 0) return false;
        // position of the last advanced node
        const int la = a - 1;
        const int pl = __shfl(p1v, la & 63) + 500; // a <= 64, so the node is one of the first 64 candidates
        const uint64_t w1 = __ballot(lane < nmax && (lane < a || p1v < pl)), w2 = __ballot(64 + lane < nmax && p2v < pl);
        pa = s + a;
        p1 = s + __popcll(w1) + __popcll(w2);
        plim = pl;
        return true;
    };

    int v0 = seg_ns, va = 0, v1 = 0, cur_lim = 0, prev_lim = -1; // prev_lim = pos(v0-1) + 500
    int nva = 0, nv1 = 0, nlim = 0;                          // next window
    int k = 0, q = 0, fail_code = 0;
    // DBatch.plan_stream: the solver of this contig is already running and takes the windows as they are published (release at agent
    // scope: the records were stored by the whole wavefront, the s_waitcnt in front of every publication has seen them complete)
    // The records then leave as agent-scope stores (written through to memory: visible to a solver on another XCD once they are
    // acknowledged), so that publishing needs no release fence at agent scope — that fence writes back the whole L2 of the XCD, which
    // k_edges<true> is filling at that moment (measured with it: edge fill 0.08 -> 0.11 ms at 64 contigs, 0.43 -> 1.9 ms at 1000).
    const bool pub = SEG ? b.seg_stream != 0 : (b.plan_stream == NL && CFG == (NL == 2 ? 0 : 1)); // (DBatch.plan_stream: the limb count of the class whose solver follows its planner; SEG: DBatch.seg_stream)
    auto publish = [&](int v) { // call after an s_waitcnt(0): every record store of this wavefront has been acknowledged
        if (!pub) return;
#ifdef WV_PLAN_TEST_NOPUB // test builds: the planner stays silent, every streamed solver must run into its time-out and hand its contig on
        return;
#endif
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // (orders the compiler; the hardware part is the wait above)
        if (lane == 0) __hip_atomic_store(SEG ? seg_rec : &meta->plan_prog, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto put64 = [&](void *p, uint32_t lo, uint32_t hi) {
        const uint64_t v = ((uint64_t)hi << 32) | lo;
        if (pub) __hip_atomic_store((uint64_t *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *(uint64_t *)p = v;
    };
    uint2 keepA = make_uint2(0, 0), keepB = make_uint2(0, 0);
    uint4 keepW0 = make_uint4(0, 0, 0, 0), keepW1 = make_uint4(0, 0, 0, 0);
    bool have = false;
    auto flush = [&]() { // the records of window k-1 (kept in registers so that their stores are old when the DMA wait comes)
        if (!have) return;
        put64(&wrole[(size_t)(k - 1) * WIN_ROLES + lane], keepA.x, keepA.y);
        put64(&wrole[(size_t)(k - 1) * WIN_ROLES + 64 + lane], keepB.x, keepB.y);
        if (lane == 0) {
            uint64_t *w = (uint64_t *)(win + (k - 1));
            put64(w, keepW0.x, keepW0.y); put64(w + 1, keepW0.z, keepW0.w); put64(w + 2, keepW1.x, keepW1.y); put64(w + 3, keepW1.z, keepW1.w);
        }
        have = false;
    };
    stage_meta(seg_ns, 0);
    __builtin_amdgcn_s_waitcnt(0);
    if (!plan(seg_ns, 0, 0, va, v1, cur_lim)) fail_code = 1;
    while (!fail_code) {
        if (k >= win_cap) { fail_code = 1; break; }
        // ---- the next window, from the block this one was staged with; then its own block goes in flight ----
        const bool last = va >= seg_ne;
        if (!last && !plan(va, q, va - v0, nva, nv1, nlim)) { fail_code = 1; break; }
        flush();
        if (!last) {
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): the other block is no longer read
            stage_meta(va, q ^ 1);
        }
        // ---- window [v0, v1): classes and compact node lists ----
        const uint32_t *m_off = blk_off(q);
        const DNode *m_node = blk_node(q);
        const int nwin = v1 - v0;
        const uint32_t e0 = m_off[0];
        const bool in1 = lane < nwin, in2 = 64 + lane < nwin;
        const int i1 = in1 ? m_node[lane].info : 0, i2 = in2 ? m_node[64 + lane].info : 0;
        const bool k1 = in1 && ((NTYPE(i1) == 1 && NFRAME(i1) > 0) || (NTYPE(i1) == 0 && NFRAME(i1) < 0));
        const bool k2 = in2 && ((NTYPE(i2) == 1 && NFRAME(i2) > 0) || (NTYPE(i2) == 0 && NFRAME(i2) < 0));
        const uint64_t mc1 = __ballot(k1), mo1 = __ballot(in1 && !k1), mc2 = __ballot(k2), mo2 = __ballot(in2 && !k2);
        const int nc = __popcll(mc1) + __popcll(mc2), no = __popcll(mo1) + __popcll(mo2);
        wv_sync();
        if (in1) { if (k1) s_listA[__popcll(mc1 & below)] = (uint8_t)lane; else s_listB[__popcll(mo1 & below)] = (uint8_t)lane; }
        if (in2) { if (k2) s_listA[__popcll(mc1) + __popcll(mc2 & below)] = (uint8_t)(64 + lane); else s_listB[__popcll(mo1) + __popcll(mo2 & below)] = (uint8_t)(64 + lane); }
        wv_sync();
        int n_spill = 0; // spill entries in use (wave-uniform)
        // ---- lanes of a phase: one per (node, chunk), chunks of cap in-edges ----
        auto setup = [&](const uint8_t *list, int n, const int cap, const bool close, uint32_t &summary) -> uint2 {
            const bool own = lane < n;
            const int jn = own ? list[lane] : 0;
            const uint32_t o0 = own ? m_off[jn] : 0u, o1 = own ? m_off[jn + 1] : 0u;
            const int deg = (int)(o1 - o0), i0 = (int)(o0 - e0);
            const int want = own ? (deg > cap ? (deg + cap - 1) / cap : 1) : 0;
            const int extra = want - (own ? 1 : 0);
            const int ex_incl = (int)wv_scan((uint32_t)extra);
            int got = (64 - n) - (ex_incl - extra); // helper lanes still free when this node is served
            got = got < 0 ? 0 : (got > extra ? extra : got);
            const int items = (own ? 1 : 0) + got;
            const int it_incl = (int)wv_scan((uint32_t)items);
            const int off = it_incl - items;
            const int total = wv_last(it_incl);
            const int spill = own ? (deg - items * cap > 0 ? deg - items * cap : 0) : 0;
            const int sp_incl = (int)wv_scan((uint32_t)spill);
            const int sp_off = n_spill + sp_incl - spill;
            n_spill += wv_last(sp_incl);
            // every node's first lane publishes one record (node, chunks, first lane | first in-edge | in-degree | spill
            // range) and marks its first lane; a lane finds its node by counting the marks at or left of it
            wv_sync();
            s_head[lane] = 0;
            wv_sync();
            if (own) {
                s_rec[lane] = make_uint4((uint32_t)jn | ((uint32_t)off << 8) | ((uint32_t)items << 16), (uint32_t)i0, (uint32_t)deg, (uint32_t)(sp_off & 0xffff) | ((uint32_t)spill << 16));
                s_head[off] = 1;
            }
            wv_sync();
            const uint64_t hm = __ballot(s_head[lane] != 0);
            const bool act = lane < total;
            const int ow = __popcll(hm & (below | (1ull << lane))) - 1;
            const uint4 rc = act ? s_rec[ow] : make_uint4(0, 0, 0, 0);
            const int o_j = (int)(rc.x & 255), ch = act ? lane - (int)((rc.x >> 8) & 255) : 0, o_items = (int)(rc.x >> 16);
            const int o_i0 = (int)rc.y, o_deg = (int)rc.z, o_sp = (int)(rc.w & 0xffff), o_spn = (int)(rc.w >> 16);
            const bool head = act && ch == 0;
            const int nfollow = head ? o_items - 1 : 0;
            int cnt = o_deg - ch * cap;
            cnt = !act ? 0 : (cnt > cap ? cap : (cnt < 0 ? 0 : cnt));
            const int apos = (head && close && v0 + o_j < SRC) ? m_node[o_j].pos : WV_POS_INF;
            // a close node left of pos(v0-1)+500 may be the source of a backward edge into a node that is already final: watched —
            // if it really has one (its lowest overlap head lies in front of the window)
            const bool watch = prev_lim >= 0 && apos < prev_lim && (mr_partial || mreach[v0 + o_j] < (uint32_t)v0);
            summary = (uint32_t)total | ((uint32_t)wv_max(cnt) << 8) | ((uint32_t)wv_max(nfollow) << 16);
            return wv_role_pack(act, o_j, ch, nfollow, cnt, watch, o_i0 + ch * cap, head ? o_sp : 0, head ? o_spn : 0);
        };
        uint32_t sumA = 0, sumB = 0;
        keepA = setup(s_listA, nc, CA, true, sumA);
        keepB = setup(s_listB, no, CB, false, sumB);
        if (n_spill > WV_OV) { fail_code = 2; break; }
        keepW0 = make_uint4((uint32_t)v0, (uint32_t)va, (uint32_t)v1, e0);
        keepW1 = make_uint4(m_off[nwin] - e0, sumA, sumB, (uint32_t)n_spill);
        have = true;
        k++;
        if (last) break;
        __builtin_amdgcn_s_waitcnt(0); // the next block has landed (and the stores above it in program order are long done)
        if (k >= 2) publish(k - 1);     // windows 0 .. k-2 are in memory (k-1 is still in registers)
        prev_lim = cur_lim; cur_lim = nlim;
        v0 = va; va = nva; v1 = nv1;
        q ^= 1;
    }
    if constexpr (SEG) { // a segment that cannot be laid out: the merge kernel sees it and the host runs the batch again without segments
        if (fail_code) { if (lane == 0) { seg_rec[1] = -1; __hip_atomic_store(seg_rec, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } return; }
        flush();
        if (pub) { __builtin_amdgcn_s_waitcnt(0); publish(k | WV_PLAN_DONE); } // (a solver that follows reads the count with the flag; one launched behind: masks it)
        else if (lane == 0) seg_rec[0] = k | WV_PLAN_DONE;
        return;
    }
    if (fail_code) {
        if (lane == 0) {
            // (compare-and-swap where a solver may follow this plan: if it has timed out and handed the contig on meanwhile, that stands)
            if (NL == 2 && CFG == 0 && b.seg) atomicOr(&b.tot->seg_abort, 32); // (behind the segments nobody launches the roomy pair: the host runs the batch again without segments)
            if (NL == 2 && CFG == 0) { // the tight configuration cannot take it: the roomy one tries (k_wave_plan<2, 1>, launched next)
                if (!pub) meta->sssp_mode = 3; else atomicCAS(&meta->sssp_mode, 2, 3);
                meta->n_win = 0;
                atomicOr(&b.tot->class_mask, 1 << 3);
                publish(-1); // a solver that follows this plan stops and leaves the contig alone
            } else {
                if (!pub) meta->sssp_mode = meta->sssp_fb; else atomicCAS(&meta->sssp_mode, D::MODE, meta->sssp_fb);
                meta->sssp_why = fail_code; meta->n_win = 0;
                atomicOr(&b.tot->class_mask, 1 << (20 + (NL == 2 ? 0 : NL == 4 ? 1 : 2))); // this class has contigs for the workgroup kernel from the start: worth a launch beside the wavefront kernel
                publish(-1); // (a 256- / 512-bit solver that follows this plan leaves: the workgroup kernel has the contig)
            }
        }
        return;
    }
    flush();
    if (lane == 0) meta->n_win = k;
    if (pub) { __builtin_amdgcn_s_waitcnt(0); publish(k | WV_PLAN_DONE); }
}

// ------------------------------------------------------------------------------------------------
// WvSolver: the solver half of a window sweep — everything between "a window's lanes have their in-edges" and "its results are
// stored" — once, for k_sssp_wave (which also prepares every window itself) and for the solver wavefront of k_sssp_duo (whose
// feeder prepares them).  N: the ring's integers, C: the form of a cached weight, PARENTS: parent edges are stored (not for the
// segments of phx_sssp_seg.inc), PROF: the profile hook.  All members are inlined into the one wavefront that owns the object;
// the kernels keep what differs between them: where a window's records and in-edges come from, and who is told about a step-back.

// polls a planner's progress word until windows [0, need) are published or it has finished.  0: go on; 1: the planner gave the contig
// up (it has redirected it itself: leave); 2: no progress for >= 20 ms (the planner is not running beside this kernel: hand the
// contig on rather than hang)
__device__ __forceinline__ int wv_wait_plan(const int *word, int need, int &n_win, bool &plan_done) {
    for (int spins = 0;; spins++) {
        const int p = __hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (p < 0) return 1;
        n_win = p & (WV_PLAN_DONE - 1);
        plan_done = (p & WV_PLAN_DONE) != 0;
        if (plan_done || n_win >= need) return 0;
        if (spins > WV_PLAN_SPINS) return 2;
        __builtin_amdgcn_s_sleep(4);
    }
}
// minimum of two positive 64-bit patterns (ordered like positive normal doubles)
__device__ __forceinline__ uint64_t wv_min64(uint64_t a, uint64_t b) { uint64_t r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// the profile hook of normal builds: nothing (-DWV_PROFILE / -DDUO_PROFILE builds put their clocks and counters behind the same names)
struct WvNoProf {
    __device__ __forceinline__ void tick(int) {}                        // a point between the parts of a window
    __device__ __forceinline__ void fine(int) {}                        // a point inside a phase
    __device__ __forceinline__ void rebase() {}                         // the base has moved
    __device__ __forceinline__ void phase_done(int, bool, bool, int) {} // after a phase: A / B, ran in 64 bits, ran exact, its helper lanes
};
template <class N, class C, int RING, int OV, bool PARENTS, class PROF>
struct WvSolver {
    typedef typename N::T T;
    static constexpr int NL = (int)(sizeof(T) / 8);
    static constexpr uint32_t ZERO = (uint32_t)RING * NL * 8, INF = (uint32_t)(RING + 1) * NL * 8; // ring offsets of the constant 0 (source) and "unreached"
    uint8_t *ring, *rel;  // exact distances of the last RING nodes; the same relative to `base` as 64-bit entries (slot i at byte 8 i)
    uint8_t *ov_w;        // spill (+ side) list: weight,
    uint32_t *ov_s;       //   ring offset of the source (| slot << 24 on the side list)
    uint64_t *gdist;      // where distances go
    int32_t *gpe;         // (PARENTS) where parent edges go (contig-relative, -1: none)
    int lane;
    T base;
    bool wide;            // a distance far below `base` was stored: exact phases until the base has moved (next window)
    bool has_spill, narrow_w; // of the window (uniform): some node has entries on the spill list; every cached weight is (w << 4) | slot, |w| < 2^51
    uint64_t again_mask;  // heads of the last 64-bit phase that need the exact ring, see phase64
    int phases, rollbacks;
    int pend_dv, pend_av, pend_bv, pend_ae, pend_be; // results of the last window, not yet stored
    T pend_d;
    PROF prof;

    __device__ __forceinline__ void init(uint8_t *ring_, uint8_t *rel_, uint8_t *ov_w_, uint32_t *ov_s_, uint64_t *gdist_, int32_t *gpe_, int lane_) {
        ring = ring_; rel = rel_; ov_w = ov_w_; ov_s = ov_s_; gdist = gdist_; gpe = gpe_; lane = lane_;
        base = N::zero();
        wide = false; has_spill = false; narrow_w = false; again_mask = 0;
        phases = 0; rollbacks = 0;
        pend_dv = -1; pend_av = -1; pend_bv = -1; pend_ae = -1; pend_be = -1;
        pend_d = N::zero();
        for (int i = lane; i < RING; i += 64) { N::store(ring + (size_t)i * NL * 8, N::big()); *(long long *)(rel + (size_t)i * 8) = WV_REL_BIG; }
        if (lane == 0) {
            N::store(ring + ZERO, N::zero()); *(long long *)(rel + ZERO / NL) = WV_REL(0);
            N::store(ring + INF, N::big()); *(long long *)(rel + INF / NL) = WV_REL_BIG;
        }
    }
    // d (real or unreached) -> its entry in the relative ring; low: d lies more than 2^60 below base (the base must move)
    __device__ __forceinline__ long long to_rel(T d, bool &low) const {
        const T x = N::sub(d, base);
        const long long xl = (long long)N::lo64(x);
        const bool fits = N::is_i64(x) && xl < WV_NARROW && xl > -WV_NARROW;
        low = !fits && N::negative(x);
        return N::unreached(d) ? WV_REL_BIG : (fits ? WV_REL(xl) : WV_REL_WIDE);
    }
    // top of a window, once its nodes have entered the ring: if a phase has asked for it, move the base to the lowest real distance in
    // the ring (and the source's 0): nothing lies below it afterwards
    __device__ __forceinline__ void move_base() {
        if (!wide) return;
        T mn = N::load(ring + ZERO);
        for (int i = lane; i < RING; i += 64) { const T d = N::load(ring + (size_t)i * NL * 8); mn = N::sel(N::lt(d, mn), d, mn); }
        for (int st = 32; st >= 1; st >>= 1) {
            const T c = N::map32(mn, [&](int w) { return __shfl_xor(w, st); });
            mn = N::sel(N::lt(c, mn), c, mn);
        }
        base = mn;
        prof.rebase();
        bool low;
        for (int i = lane; i < RING + 1; i += 64) *(long long *)(rel + (size_t)i * 8) = to_rel(N::load(ring + (size_t)i * NL * 8), low);
        wide = false;
        wv_sync();
    }
    // the lane of a phase (chunks of `cap` in-edges) from its record (k_wave_plan) and the window's summary word; its cached in-edges are the kernel's to fill
    __device__ __forceinline__ void decode(WvLane &R, const uint2 rc, const uint32_t summary, const int v0, const int cap) const {
        const bool act = wv_role_act(rc);
        const int o_j = wv_role_node(rc);
        R.node = act ? o_j : -1;
        R.ch = wv_role_ch(rc);
        R.head = act && R.ch == 0;
        R.nextf = wv_next(act ? R.ch : 0) >= 1;
        R.watch = wv_role_watch(rc);
        R.nfollow = wv_role_nfollow(rc);
        R.cnt = wv_role_cnt(rc);
        R.ebase = wv_role_ebase(rc);
        R.sp0 = wv_role_sp0(rc);
        R.sp1 = R.sp0 + wv_role_spn(rc);
        R.spe = R.ebase + (R.nfollow + 1) * cap;
        R.slot = (uint32_t)((v0 + o_j) & (RING - 1)) * NL * 8;
        R.pe = -1;
        R.maxcnt = wv_sum_maxcnt(summary);
        R.maxfollow = wv_sum_maxfollow(summary);
        R.sd0 = 0; R.sd1 = 0;
    }
    // one phase on the exact ring: every node of the phase takes the minimum over all its in-edges
    // (phase and phase64 are plain `inline`, like the lambdas they replace: the optimiser then simplifies each on its own before it inlines it into
    //  its one call site.  Forced in first, the index array `xa` of the group minimum turns into chains of selects: +3 % instructions in all eleven kernels)
    template <int cap>
    __device__ inline bool phase(WvLane &R, const typename C::CW *cw, const uint32_t *cs) {
        T m = N::top();
        int arg = 0;
        constexpr int G = cap < 8 ? cap : (NL > 2 ? 4 : 8); // distances are fetched G at a time: one LDS round trip per group
#pragma unroll
        for (int t0 = 0; t0 < cap; t0 += G) {
            if (t0 >= R.maxcnt) break;
            T x[G];
            int xa[G];
#pragma unroll
            for (int g = 0; g < G; g++) x[g] = N::load(ring + cs[t0 + g]);
#pragma unroll
            for (int g = 0; g < G; g++) xa[g] = t0 + g;
            if (narrow_w) { // (uniform) the cached weights are in the form of a narrow window
#pragma unroll
                for (int g = 0; g < G; g++) {
                    uint64_t lo = C::lo(cw[t0 + g]);
                    asm volatile("" : "+v"(lo)); // (keeps the shift inside this rare phase: hoisted out of the phase loop it costs every window)
                    x[g] = N::add(x[g], N::from_i64((long long)lo >> 4));
                }
            } else {
#pragma unroll
                for (int g = 0; g < G; g++) x[g] = N::add(x[g], C::template to_T<N>(cw[t0 + g]));
            }
            // minimum of the group as a tree (independent compares); ties keep the lower index
#pragma unroll
            for (int w = 1; w < G; w <<= 1)
#pragma unroll
                for (int g = 0; g + w < G; g += 2 * w) {
                    const bool l = N::lt(x[g + w], x[g]);
                    x[g] = N::sel(l, x[g + w], x[g]);
                    xa[g] = l ? xa[g + w] : xa[g];
                }
            const bool l = N::lt(x[0], m);
            m = N::sel(l, x[0], m);
            arg = l ? xa[0] : arg;
        }
        if constexpr (C::SIDE) {
            if (!narrow_w) { // (uniform) this lane's entries of the side list; an equal candidate wins if its slot is the lower one
                for (int i = R.sd0; i < R.sd1; i++) {
                    const uint32_t sv = ov_s[i];
                    const int t = (int)(sv >> 24);
                    const T c = N::add(N::load(ring + (sv & 0xffffffu)), N::load(ov_w + (size_t)i * NL * 8));
                    const bool l = N::lt(c, m) || (!N::lt(m, c) && t < arg);
                    m = N::sel(l, c, m);
                    arg = l ? t : arg;
                }
            }
        }
        prof.fine(6);
        int e = R.ebase + arg;
        if (R.maxfollow > 0) {
            // segmented minimum over a head and the helper lanes that follow it: log2 steps, each lane takes the
            // value `st` lanes to its right if that lane belongs to the same node (its chunk index is >= st);
            // the left operand keeps ties, so the lowest in-edge index survives
            for (int st = 1; st <= R.maxfollow; st <<= 1) {
                const int src = (lane + st) & 63;
                const int och = __shfl(R.node >= 0 ? R.ch : 0, src);
                const T c = N::map32(m, [&](int w) { return __shfl(w, src); });
                const int ce = __shfl(e, src);
                const bool l = lane + st < 64 && och >= st && N::lt(c, m);
                m = N::sel(l, c, m);
                e = l ? ce : e;
            }
        }
        prof.fine(7);
        bool coop = false; // this lane's spill entries were taken by the whole wavefront (below)
        if constexpr (NL >= 8) {
            // A stop node behind a 9000-codon ORF collects an in-edge from every in-frame start (~450): beyond its 63 helper lanes ~200 entries sit on the
            // spill list, and one lane walked them two at a time in every close-node phase of the window (~8 us each).  Lists of more than 8
            // entries are reduced by all 64 lanes instead: a strided pass, then a butterfly on (value, edge index) — the lowest index among equals, as
            // the walk in order finds it.
            if (has_spill) {
                uint64_t bigm = __ballot(R.head && R.sp1 - R.sp0 > 8);
                while (bigm) {
                    const int Ln = __ffsll((long long)bigm) - 1;
                    bigm &= bigm - 1;
                    const int s0 = __builtin_amdgcn_readlane(R.sp0, Ln), s1 = __builtin_amdgcn_readlane(R.sp1, Ln), spe0 = __builtin_amdgcn_readlane(R.spe, Ln);
                    T mm = N::top();
                    int ee = 0x7fffffff;
                    for (int i = s0 + lane; i < s1; i += 64) {
                        const T c = N::add(N::load(ring + ov_s[i]), N::load(ov_w + (size_t)i * NL * 8));
                        const bool l = N::lt(c, mm);
                        mm = N::sel(l, c, mm);
                        ee = l ? spe0 + (i - s0) : ee;
                    }
                    for (int st = 32; st >= 1; st >>= 1) {
                        const T c = N::map32(mm, [&](int w) { return __shfl_xor(w, st); });
                        const int ce = __shfl_xor(ee, st);
                        const bool l = N::lt(c, mm) || (!N::lt(mm, c) && ce < ee);
                        mm = N::sel(l, c, mm);
                        ee = l ? ce : ee;
                    }
                    if (lane == Ln) { const bool l = N::lt(mm, m); m = N::sel(l, mm, m); e = l ? ee : e; coop = true; }
                }
            }
        }
        if (has_spill) {
            for (int i = coop ? R.sp1 : R.sp0; i < R.sp1; i += 2) { // spill list, two entries per pair of LDS round trips
                const bool two = i + 1 < R.sp1;
                const uint32_t s0 = ov_s[i], s1 = two ? ov_s[i + 1] : INF;
                const T w0 = N::load(ov_w + (size_t)i * NL * 8), w1 = N::sel(two, N::load(ov_w + (size_t)(i + 1 < OV ? i + 1 : i) * NL * 8), N::zero());
                const T c0 = N::add(N::load(ring + s0), w0), c1 = N::add(N::load(ring + s1), w1);
                bool l = N::lt(c0, m);
                m = N::sel(l, c0, m);
                e = l ? R.spe + (i - R.sp0) : e;
                l = N::lt(c1, m);
                m = N::sel(l, c1, m);
                e = l ? R.spe + (i + 1 - R.sp0) : e;
            }
        }
        prof.fine(8);
        bool chg = false, widen = false;
        if (R.head) {
            R.pe = e;
            const T d0 = N::load(ring + R.slot);
            // (a candidate over an unreached source is not a distance: the ring holds real distances or exactly big())
            if (N::lt(m, d0) && !N::unreached(m)) {
                N::store(ring + R.slot, m); chg = true;
                *(long long *)(rel + R.slot / NL) = to_rel(m, widen);
            }
        }
        wv_sync(); // the next phase reads what this one wrote
        const bool any = __ballot(chg) != 0;
        if (__ballot(widen)) wide = true;
        prof.fine(9);
        return any;
    }
    // The same phase on the relative ring, for windows whose cached weights are all narrow (|w| < 2^51) while no distance
    // lies far below the base.  A candidate is entry + (w << 4) + slot: one 64-bit shift-add; the entries are positive and
    // below 2^63, so as bit patterns they are ordered like positive normal doubles and the minimum of a lane's
    // candidates is a chain of v_min_f64 - the winning slot rides in the low 4 bits, ties go to the lower slot.
    // A candidate over an unreached source is >= WV_VAL_BIG - 2^51 and never stored; one over a WV_REL_WIDE source (a real
    // distance more than 2^55 above the base) loses against every narrow candidate, and a node that has none but has such
    // a source makes the phase run again on the exact ring (`again_mask`).  Otherwise: the same numbers.
    template <int cap>
    __device__ inline bool phase64(WvLane &R, const typename C::CW *cw, const uint32_t *cs) { // true: some distance improved
        uint64_t mm = 0x7000000000000000ull;
        // every load of the phase is in flight before the first use (unused slots point at the constant "unreached" entry)
        const long long d0 = *(const long long *)(rel + R.slot / NL);
        uint64_t x[cap];
#pragma unroll
        for (int t = 0; t < cap; t++) x[t] = *(const uint64_t *)(rel + cs[t] / NL);
#pragma unroll
        for (int t = 0; t < cap; t++) x[t] += C::lo(cw[t]);
#pragma unroll
        for (int w = 1; w < cap; w <<= 1)
#pragma unroll
            for (int t = 0; t + w < cap; t += 2 * w) x[t] = wv_min64(x[t], x[t + w]);
        mm = wv_min64(mm, x[0]);
        prof.fine(6);
        int e = R.ebase + (int)(mm & 15u);
        long long m = (long long)mm >> 4; // relative value + WV_BIAS
        if (R.maxfollow > 0 && R.maxfollow <= 4) {
            // few helper lanes: one DPP shift (lane i <- lane i+1) per helper instead of log-steps over ds_bpermute
            for (int q = 0; q < R.maxfollow; q++) {
                const long long c = (long long)(((uint64_t)(uint32_t)wv_next_self((int)((uint64_t)m >> 32)) << 32) | (uint32_t)wv_next_self((int)m));
                const int ce = wv_next_self(e);
                const bool l = R.nextf && c < m;
                m = l ? c : m;
                e = l ? ce : e;
            }
        } else if (R.maxfollow > 0) {
            for (int st = 1; st <= R.maxfollow; st <<= 1) {
                const int src = (lane + st) & 63;
                const int och = __shfl(R.node >= 0 ? R.ch : 0, src);
                const long long c = (long long)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)m >> 32), src) << 32) | (uint32_t)__shfl((int)m, src));
                const int ce = __shfl(e, src);
                const bool l = lane + st < 64 && och >= st && c < m;
                m = l ? c : m;
                e = l ? ce : e;
            }
        }
        prof.fine(7);
        if (has_spill) {
            for (int i = R.sp0; i < R.sp1; i++) {
                const long long c0 = (long long)((*(const uint64_t *)(ov_w + (size_t)i * NL * 8) << 4) + *(const uint64_t *)(rel + ov_s[i] / NL)) >> 4;
                const bool l = c0 < m;
                m = l ? c0 : m;
                e = l ? R.spe + (i - R.sp0) : e;
            }
        }
        prof.fine(8);
        // a head whose best candidate sits on a wide source, or is itself 2^55 or more above the base (its slot may hold
        // a wide distance it cannot be compared with here): the phase is run again on the exact ring; what the other
        // heads store meanwhile are valid improvements
        const bool again = R.head && m >= WV_BIAS + WV_NARROW && m < WV_BIAS + WV_VAL_BIG - (1ll << 52);
        // d0 real: compare; d0 unreached or wide (more than 2^55 above the base): any real candidate is lower.
        // (lane predicates and votes straight from the compares: no flags carried out of a divergent region)
        const bool store = R.head && m < WV_BIAS + WV_NARROW && m < (d0 >> 4);
        const long long v = m - WV_BIAS;
        const bool fits = v > -WV_NARROW;
        R.pe = R.head ? e : R.pe;
        if (store) {
            N::store(ring + R.slot, N::add(base, N::from_i64(v)));
            *(long long *)(rel + R.slot / NL) = fits ? (long long)((uint64_t)m << 4) : WV_REL_WIDE;
        }
        const uint64_t cm = __ballot(store);
        again_mask = __ballot(again);
        wv_sync();
        if (cm && __ballot(store && !fits)) wide = true;
        prof.fine(9);
        return cm != 0;
    }
    // a window to its fixed point: phase A (close nodes), phase B (open nodes), ... until a phase changes nothing; in 64 bits while the
    // window's weights are narrow and no distance lies far below the base.  false: no convergence (sssp_why 3)
    template <int CA, int CB>
    __device__ __forceinline__ bool iterate(WvLane &A, const typename C::CW (&cwA)[CA], const uint32_t (&csA)[CA], WvLane &B, const typename C::CW (&cwB)[CB], const uint32_t (&csB)[CB]) {
        again_mask = 0;
        int inner = 0;
        for (int ph = 0;; ph ^= 1) {
            bool chg = false;
            const bool n64 = narrow_w && !wide;
            if (n64) chg = ph ? phase64<CB>(B, cwB, csB) : phase64<CA>(A, cwA, csA);
            const bool exact = !n64 || again_mask != 0; // run the exact phase
            if (exact) chg |= ph ? phase<CB>(B, cwB, csB) : phase<CA>(A, cwA, csA);
            prof.phase_done(ph, n64, exact, ph ? B.maxfollow : A.maxfollow);
            phases++;
            if (!chg && (ph == 1 || inner > 0)) return true;
            if (++inner > 4 * WV_WIN + 16) return false;
        }
    }
    // results of the advanced nodes [v0, va): distance, parent edge (contig-relative, the convention of k_sssp / k_sssp_lds; the walk
    // at the end resolves it).  Kept in registers; flush_results stores them behind the next window's wait, when their stores cost nothing.
    __device__ __forceinline__ void keep_results(const WvLane &A, const WvLane &B, const int v0, const int va, const uint32_t e0, const int SRC) {
        pend_dv = v0 + lane < va ? v0 + lane : -1;
        pend_d = N::load(ring + (size_t)((v0 + lane) & (RING - 1)) * NL * 8);
        if constexpr (PARENTS) {
            auto parents = [&](const auto &R, int &pv, int &pe) {
                pv = (R.head && v0 + R.node < va) ? v0 + R.node : -1;
                pe = (pv >= 0 && pv != SRC && R.pe >= 0 && !N::unreached(N::load(ring + (R.head ? R.slot : ZERO)))) ? (int)(e0 + (uint32_t)R.pe) : -1;
            };
            parents(A, pend_av, pend_ae);
            parents(B, pend_bv, pend_be);
        }
    }
    __device__ __forceinline__ void flush_results() {
        if (pend_dv >= 0) N::store(gdist + (size_t)pend_dv * NL, pend_d);
        if (PARENTS && pend_av >= 0) gpe[pend_av] = pend_ae;
        if (PARENTS && pend_bv >= 0) gpe[pend_bv] = pend_be;
        pend_dv = -1; pend_av = -1; pend_bv = -1;
    }
    // did a close node that final nodes may depend on improve in this window?  (a_old: its distance before the phases)  Then the sweep steps back
    __device__ __forceinline__ bool watch_improved(const WvLane &A, const T a_old) const {
#ifdef WV_NO_WATCH // development: how much the step-backs cost (results are then wrong where one was needed)
        return false;
#else
        return A.head && A.watch && N::lt(N::load(ring + A.slot), a_old);
#endif
    }
    // ... to this node, at least `lo`: the lowest final node an overlap edge out of an improved, watched node ends in (k_edges_scan recorded it)
    __device__ __forceinline__ int step_back_node(const WvLane &A, const bool trig, const uint64_t tm, const int v0, const DBatch &b, const DMeta *meta, const int lo) const {
        uint32_t mr = trig ? b.mreach[4 * (size_t)meta->node_off + (size_t)(v0 + A.node)] : ~0u;
        for (int st = 32; st >= 1; st >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)mr, st); mr = o < mr ? o : mr; }
        int rr = (int)mr < v0 ? (int)mr : v0;
        if (meta->dense & 2) { // the table is incomplete for this contig: the first node less than 500 bp left of the improved one
            const DNode *nd = b.node + meta->node_off;
            const int tl = __ffsll((long long)tm) - 1;
            const int xpos = nd[v0 + __shfl(A.node, tl)].pos; // a watched node is not the source / target
            rr = v0;
            while (rr > 0) {
                const int q = rr - 1 - lane;
                const bool aff = q >= 0 && nd[q].pos > xpos - 500;
                const uint64_t am = __ballot(aff);
                if (am == ~0ull) { rr -= 64; continue; }
                rr -= am ? (__ffsll((long long)~am) - 1) : 0;
                break;
            }
        }
        return rr < lo ? lo : rr;
    }
    // the sweep is over: the contig's records (the path walk and the genes, phanotate.py:64-76, are left to k_inorder: one lane chasing
    // parents while 63 idle cost every contig ~50 us of a latency-bound kernel; there the walk runs with a workgroup per contig at full occupancy)
    __device__ __forceinline__ void finish(DMeta *meta, const int V) const {
        if (lane != 0) return;
        meta->sweeps = 1 + rollbacks;
        meta->sssp_iters = phases;
        meta->n_genes = 0; meta->gene_off = 0;
        // the target's distance is still in the ring (it was advanced by the last window)
        if (N::unreached(N::load(ring + (size_t)((V - 1) & (RING - 1)) * NL * 8))) { meta->status = PHX_S_NOPATH; meta->n_path = 0; }
        else meta->n_path = -2; // distances and parent edges are final; not walked yet
    }
};
// hands a contig to the kernel it falls back to (lane 0 calls).  Where somebody else may be redirecting the contig at this moment — the
// planner a streamed kernel follows, or (code 5, a planner that made no progress) one that may yet wake up — a compare-and-swap: whoever
// comes first decides
__device__ __forceinline__ void wv_hand_back(DMeta *meta, DTotals *tot, const int mode, const int code, const bool streamed) {
    if (code != 5 && !streamed) { meta->sssp_mode = meta->sssp_fb; meta->sssp_why = code; return; }
    if (atomicCAS(&meta->sssp_mode, mode, meta->sssp_fb) != mode) return;
    meta->sssp_why = code;
    if (code == 5) atomicAdd(&tot->plan_timeouts, 1);
}

template <int NL, int CFG>
constexpr size_t wv_lds_bytes() {
    typedef WvDims<NL, CFG> D;
    return (size_t)(D::RING + 2) * NL * 8 + (size_t)D::ECAP * 12 + (size_t)D::OV * (NL * 8 + 4) + (size_t)WIN_ROLES * 8 + (size_t)(D::RING + 2) * 8 + 64;
}

// four wavefronts of this kernel per CU (one per SIMD): 1024 contigs are resident at once only while 4 x LDS fits 160 KB
static_assert(4 * wv_lds_bytes<2, 1>() <= 160 * 1024 && 4 * wv_lds_bytes<4, 1>() <= 160 * 1024 && wv_lds_bytes<8, 1>() <= 64 * 1024, "k_sssp_wave: LDS per wavefront");
static_assert(4 * wv_lds_bytes<2, 0>() + 40 * 1024 + 64 <= 160 * 1024, "k_sssp_wave, tight configuration: a 40 KB workgroup fits beside four wavefronts");
#ifdef WV_PROFILE // clocks and counters behind WvSolver's hook (tools/wave_balance.py reads what the kernel's tail copies to DMeta)
struct WvProf {
    long long tp[12], tmark, t_begin;
    int n_p64, n_redo, n_p128, n_rebase, mfA, mfB, bigA, bigB;
    __device__ __forceinline__ void start() { for (int i = 0; i < 12; i++) tp[i] = 0; tmark = t_begin = wall_clock64(); n_p64 = n_redo = n_p128 = n_rebase = mfA = mfB = bigA = bigB = 0; }
    __device__ __forceinline__ void tick(int k) { const long long t_ = wall_clock64(); tp[k] += t_ - tmark; tmark = t_; }
    __device__ __forceinline__ void fine(int k) { // ticks inside the phases (they cost about as much as a 64-bit phase's arithmetic)
#ifdef WV_PROFILE_FINE
        tick(k);
#endif
    }
    __device__ __forceinline__ void rebase() { n_rebase++; }
    __device__ __forceinline__ void phase_done(int ph, bool n64, bool exact, int maxfollow) {
        n_p64 += n64; n_redo += n64 && exact; n_p128 += exact;
#ifdef WV_PROFILE_AB
        tick(ph ? 7 : 6);
        if (ph) { mfB += maxfollow; bigB += maxfollow > 4; } else { mfA += maxfollow; bigA += maxfollow > 4; }
#endif
    }
};
#define WV_TICK(k) S.prof.tick(k);
#else
typedef WvNoProf WvProf;
#define WV_TICK(k)
#endif
#ifdef WV_PROFILE_GATHER // ticks inside the gather: cached in-edges / slow conversions / spill list (reported in the slots of WV_PROFILE_FINE)
#define WV_GTICK(k) WV_TICK(k)
#else
#define WV_GTICK(k)
#endif
// STREAM: the instantiation that follows its planner's progress counter (DBatch.plan_stream; a kernel of its own so that the other's
// code — the benchmark batch's — is exactly what it was: with the test at run time the 1000-contig launch took 0.476-0.49 instead of 0.457-0.462 ms)
template <int NL, int CFG, bool STREAM = false>
__global__ __launch_bounds__(64, NL == 2 ? WV_WPE : 1) void k_sssp_wave(DBatch b) {
    typedef WvDims<NL, CFG> D;
    typedef WvCw<NL> C;
    typedef typename C::CW CW;
    constexpr int WV_ECAP = D::ECAP;
    typedef WvNum<NL> N;
    typedef typename N::T T;
    constexpr int CA = N::CA, CB = N::CB;
    constexpr int WV_RING = D::RING, WV_OV = D::OV, WV_SLOTS = WV_RING + 2;
    extern __shared__ __align__(16) uint8_t smem[];
    if (b.tot->overflow) return; // a buffer of this run is too small (and k_sssp_order has not run): the host grows it and runs again
    DMeta *meta = &b.meta[b.sord ? b.sord[blockIdx.x] : (int)blockIdx.x]; // (large batches: most in-edges first, k_sssp_order)
    const int V = meta->n_node;
    if (meta->status < 0 || V <= 2 || meta->sssp_nl != NL || meta->sssp_mode != D::MODE) return;
    const int lane = threadIdx.x;
    const int SRC = V - 2;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off; // integer weights, encoded (ew_encode)
    // (node positions are no longer needed here: the step-back target comes from mreach)
    uint64_t *gdist = b.dist + (size_t)meta->node_off * b.dist_stride;
    int32_t *gpe = b.parent + meta->node_off; // parent edge of every node (contig-relative), -1: none
    const DWin *win = b.win + meta->win_off;
    const uint2 *wrole = b.wrole + (size_t)meta->win_off * WIN_ROLES;
    // DBatch.plan_stream (tight 128-bit configuration, small batches): the planner of this contig may still be running — n_win is then the
    // number of windows it has published so far, and wv_wait_plan polls DMeta.plan_prog.
    static_assert(!STREAM || (NL == 2 && CFG == 0) || ((NL == 4 || NL == 8) && CFG == 1), "the tight 128-bit configuration and the 256- / 512-bit kernels can follow their planner");
    constexpr bool streamed = STREAM;
    typename std::conditional<STREAM, int, const int>::type n_win = streamed ? 0 : meta->n_win;
    bool plan_done = !streamed;
    if constexpr (streamed) {
        const int w = wv_wait_plan(&meta->plan_prog, 1, n_win, plan_done);
        if (w == 1) return;
        if (w == 2) { // (a compare-and-swap: the planner may be redirecting the contig itself at this moment — whoever comes first decides)
            if (lane == 0) wv_hand_back(meta, b.tot, D::MODE, 5, true);
            return;
        }
    }

    // ---- LDS ----
    uint8_t *ring = smem;                                       // (RING+1) distances; slot RING = the constant 0 (source)
    long long *st_w = (long long *)(ring + (size_t)WV_SLOTS * NL * 8); // staged in-edges of the window: weight (encoded integer),
    uint32_t *st_src = (uint32_t *)(st_w + WV_ECAP);            //   source node (| inexact << 31: masked when it is read)
    uint8_t *ov_w = (uint8_t *)(st_src + WV_ECAP);              // spill list: weight,
    uint32_t *ov_s = (uint32_t *)(ov_w + (size_t)WV_OV * NL * 8); //   ring offset of the source
    uint2 *s_role = (uint2 *)(ov_s + WV_OV);                    // lane records of the window (k_wave_plan)
    // The same distances relative to `base`, as 64-bit integers (slot i at byte 8 i = the byte offset in `ring` / NL): a real
    // distance d with |d - base| < 2^55 is stored as WV_REL(d - base) = (d - base + 2^58) << 4, an unreached one as
    // WV_REL_BIG, any other as WV_REL_WIDE: all positive, ordered like the values, low 4 bits free for an in-edge slot.
    // Windows whose weights are narrow iterate on this ring (phase64); `ring` stays exact at all times.
    uint8_t *rel = (uint8_t *)(s_role + WIN_ROLES);
    typedef WvSolver<N, C, WV_RING, WV_OV, true, WvProf> Solver;
    constexpr uint32_t ZERO = Solver::ZERO, INF = Solver::INF;
    Solver S;
    S.init(ring, rel, ov_w, ov_s, gdist, gpe, lane);

    int loaded = 0;
    bool fail = n_win <= 0;
    int fail_code = fail ? 1 : 0;
#ifdef WV_PROFILE
    S.prof.start();
#endif

    // window records: lane l keeps the record of window cbase + l
    int cbase = 0, rec_hi = 0; // windows [cbase, rec_hi) are in the registers
    uint4 wr0 = make_uint4(0, 0, 0, 0), wr1 = make_uint4(0, 0, 0, 0);
    auto load_recs = [&](int base) {
        cbase = base;
        if constexpr (STREAM) rec_hi = base + 64 < n_win ? base + 64 : n_win;
        const int i = base + lane;
        if (i < n_win) { wr0 = ((const uint4 *)(win + i))[0]; wr1 = ((const uint4 *)(win + i))[1]; }
        __builtin_amdgcn_s_waitcnt(0);
    };
    // put window k's in-edges and lane records in flight (its record is among the loaded ones)
    auto stage = [&](int k) {
        const int l = k - cbase;
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)wr0.w, l);
        const int ne = __builtin_amdgcn_readlane((int)wr1.x, l);
        // whole 1 KB pieces, no per-lane bounds: the tail reads at most 1 KB past the window's in-edges (the next window's, the
        // next contig's, or the 2 KB slack behind every buffer) into staging space that exists (ECAP is a multiple of 256)
        for (int i = 0; i < ne; i += 256) wv_dma16(esrc + e0 + i + 4 * lane, st_src + i);
        for (int i = 0; i < ne; i += 128) wv_dma16(ew + e0 + i + 2 * lane, st_w + i);
        wv_dma16(wrole + (size_t)k * WIN_ROLES + 2 * lane, s_role);
    };

    int k = 0;
    if (!fail) { load_recs(0); stage(0); }
    while (!fail) {
        // ================= window [v0, v1), advance to va =================
        WV_TICK(5)
        int l = k - cbase;
        const int v0 = __builtin_amdgcn_readlane((int)wr0.x, l), va = __builtin_amdgcn_readlane((int)wr0.y, l), v1 = __builtin_amdgcn_readlane((int)wr0.z, l);
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)wr0.w, l);
        const uint32_t sumA = (uint32_t)__builtin_amdgcn_readlane((int)wr1.y, l), sumB = (uint32_t)__builtin_amdgcn_readlane((int)wr1.z, l);
        int sd_next = __builtin_amdgcn_readlane((int)wr1.w, l); // spill entries the planner laid out; (C::SIDE) the side list of wide in-edges follows them
        S.has_spill = sd_next != 0; // some node of the window has in-edges on the spill list
        __builtin_amdgcn_s_waitcnt(0); // the DMA of this window has landed
        S.flush_results(); // the previous window's results leave now: their stores are old when the next wait comes
        WV_TICK(0)
        // ---- nodes that enter the ring ----
        for (int i = loaded + lane; i < v1; i += 64) {
            const T d = N::sel(i == SRC, N::zero(), N::big());
            bool low;
            N::store(ring + (size_t)(i & (WV_RING - 1)) * NL * 8, d);
            *(long long *)(rel + (size_t)(i & (WV_RING - 1)) * 8) = S.to_rel(d, low);
        }
        if (v1 > loaded) loaded = v1;
        wv_sync();
        S.move_base();
        const int ring_lo = loaded - WV_RING;

        // one in-edge: staged (source node, integer weight) -> (ring offset of the source, weight as a T).  The weights arrive as
        // integers (k_edges / k_score encode trunc(w * 1000) once, ew_encode): a narrow one (|W| < 2^51, nearly every edge) is its own
        // low half.  convert_fast is branch-free and covers |W| < 2^62 with the source in the ring (or the source node, or beyond
        // the window); it reports the rest (a source that left the ring, a weight kept as a double's bit pattern) so that the
        // caller fixes those up afterwards, off the common path.
        auto convert_fast = [&](bool on, uint32_t u, long long wi, uint32_t &cs, CW &cw) -> bool {
            const bool isrc = u == (uint32_t)SRC;
            const bool beyond = !on || ((int)u >= loaded && !isrc); // padding / source beyond the window (look-ahead nodes only): not there yet
            const bool far = on && !isrc && (int)u < ring_lo;        // left the ring long ago: final, folded into the weight
            cs = beyond ? INF : ((isrc || far) ? ZERO : (u & (WV_RING - 1)) * NL * 8);
            cw = C::from_i64(beyond ? 0ll : wi);
            return on && (far || !ew_narrow51(wi));
        };
        auto convert_slow = [&](uint32_t u, long long wi, T &cw) {
            T w = EW_WIDE(wi) ? N::from_double(__longlong_as_double(wi | (1ll << 62))) : N::from_i64(wi);
            if (u != (uint32_t)SRC && (int)u < ring_lo) w = N::add(w, N::load(gdist + (size_t)u * NL));
            cw = w;
        };
        auto gather = [&](auto &R) -> bool { // true: some in-edge of the window took the slow conversion (a wide weight, or a folded distance)
            constexpr int cap = std::remove_reference_t<decltype(R)>::CAP;
            bool wide_w = false;
            uint32_t slow = 0; // bit t: cached in-edge t needs the slow conversion
            // slots past a lane's count read staged data of other lanes (or the arrays that follow): they become a source that is
            // never loaded (-> the constant "unreached" entry) with weight 0, so that nothing below needs the count again
            constexpr uint32_t PADU = 0x3ffffffeu;
            uint32_t ru[cap];
            long long rw[cap];
#pragma unroll
            for (int t0 = 0; t0 < cap; t0 += 4) { // every staged read of the lane is in flight before the first conversion
                if (t0 >= R.maxcnt) break;
#pragma unroll
                for (int g = 0; g < 4; g++) { ru[t0 + g] = st_src[R.ebase + t0 + g]; rw[t0 + g] = st_w[R.ebase + t0 + g]; }
            }
#ifdef WV_PROFILE_GATHER
            __builtin_amdgcn_s_waitcnt(0xc07f);
            WV_GTICK(9)
#endif
#pragma unroll
            for (int t0 = 0; t0 < cap; t0 += 4) {
                if (t0 >= R.maxcnt) {
#pragma unroll
                    for (int g = 0; g < 4; g++) { R.cs[t0 + g] = INF; R.cw[t0 + g] = C::from_i64(0ll); }
                    continue;
                }
                uint32_t u[4];
                long long wt[4];
                // nearly every group holds only in-edges with a narrow weight whose source is in the ring or still ahead: those
                // need neither the source-node / folded-source cases nor the slow-conversion bookkeeping.  k_edges / k_score marked
                // the others (ESRC_OFFPATH), so the test is one OR per in-edge (a slot past the lane's count is tested with what
                // it happens to hold: another lane's in-edge).
                uint32_t acc = 0;
                bool special = false;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const bool on = t0 + g < R.cnt;
                    acc |= ru[t0 + g];
                    u[g] = on ? ESRC_NODE(ru[t0 + g]) : PADU;
                    wt[g] = on ? rw[t0 + g] : 0ll;
                    special |= (int)u[g] < ring_lo;
                }
                special |= ESRC_OFFPATH(acc) != 0u;
                if (__ballot(special) == 0ull) {
#pragma unroll
                    for (int g = 0; g < 4; g++) { // (a source beyond the window keeps its weight: a candidate over "unreached" is never stored)
                        R.cs[t0 + g] = (int)u[g] >= loaded ? INF : (u[g] & (WV_RING - 1)) * NL * 8;
                        R.cw[t0 + g] = C::from_i64(wt[g]);
                    }
                    continue;
                }
#pragma unroll
                for (int g = 0; g < 4; g++)
                    if (convert_fast(t0 + g < R.cnt, u[g], wt[g], R.cs[t0 + g], R.cw[t0 + g])) slow |= 1u << (t0 + g);
            }
            WV_GTICK(6)
            R.sd0 = 0; R.sd1 = 0;
            if (__ballot(slow != 0)) {
                wide_w = true;
                if constexpr (!C::SIDE) {
#pragma unroll
                    for (int t = 0; t < cap; t++)
                        if (__ballot((slow >> t) & 1)) {
                            if ((slow >> t) & 1) convert_slow(ESRC_NODE(st_src[R.ebase + t]), st_w[R.ebase + t], R.cw[t]);
                        }
                } else {
                    // (rare) in-edges whose weight is not a narrow integer, or whose source left the ring: exact-width candidates
                    // "ring[source] + weight" on the side list in LDS, behind the planner's spill entries; the register slot is
                    // disabled.  Nearly all of them come from a node left of the window (a long ORF's start): that node is final,
                    // distance + weight is a constant while the window iterates, and the lane keeps only the best of them (lowest
                    // slot among equals) as one entry over the constant-0 slot.
                    uint32_t side = 0;
                    T fc = N::top();
                    int fce = -1;
#pragma unroll
                    for (int t = 0; t < cap; t++)
                        if (__ballot((slow >> t) & 1)) {
                            if ((slow >> t) & 1) {
                                const uint32_t u = ESRC_NODE(st_src[R.ebase + t]);
                                const long long wi = st_w[R.ebase + t];
                                if (u == (uint32_t)SRC || (int)u < v0) {
                                    const T w = EW_WIDE(wi) ? N::from_double(__longlong_as_double(wi | (1ll << 62))) : N::from_i64(wi);
                                    const T d = u == (uint32_t)SRC ? N::zero() : ((int)u < ring_lo ? N::load(gdist + (size_t)u * NL) : N::load(ring + (size_t)(u & (WV_RING - 1)) * NL * 8));
                                    const T c = N::add(d, w);
                                    if (!N::unreached(d) && N::lt(c, fc)) { fc = c; fce = t; }
                                    R.cs[t] = INF;
                                } else side |= 1u << t;
                                R.cw[t] = C::from_i64(0ll);
                            }
                        }
                    const int c = __popc(side) + (fce >= 0 ? 1 : 0);
                    const int incl = (int)wv_scan((uint32_t)c);
                    const int total = wv_last(incl);
                    R.sd0 = sd_next + incl - c; R.sd1 = R.sd0 + c;
                    if (sd_next + total > WV_OV) { fail = true; fail_code = 2; }
                    else {
                        int i = R.sd0;
                        if (fce >= 0) { ov_s[i] = ZERO | ((uint32_t)fce << 24); N::store(ov_w + (size_t)i * NL * 8, fc); i++; }
                        if (__ballot(side != 0)) {
#pragma unroll
                            for (int t = 0; t < cap; t++)
                                if (__ballot((side >> t) & 1)) {
                                    if ((side >> t) & 1) {
                                        T w;
                                        convert_slow(ESRC_NODE(st_src[R.ebase + t]), st_w[R.ebase + t], w);
                                        ov_s[i] = R.cs[t] | ((uint32_t)t << 24);
                                        N::store(ov_w + (size_t)i * NL * 8, w);
                                        i++;
                                        R.cs[t] = INF;
                                    }
                                }
                        }
                        sd_next += total;
                    }
                }
            }
            WV_GTICK(7)
            if (S.has_spill)
            for (int i = R.sp0; i < R.sp1 && i < WV_OV; i++) {
                uint32_t sl; CW wl;
                const int idx = R.spe + (i - R.sp0);
                const uint32_t u = ESRC_NODE(st_src[idx]);
                const long long wd = st_w[idx];
                const bool slow_e = convert_fast(true, u, wd, sl, wl);
                T w = C::template to_T<N>(wl);
                if (slow_e) { convert_slow(u, wd, w); wide_w = true; }
                ov_s[i] = sl;
                N::store(ov_w + (size_t)i * NL * 8, w);
            }
            WV_GTICK(8)
            return __ballot(wide_w) != 0;
        };
        // ---- lanes of a phase: one per (node, chunk), as laid out by k_wave_plan ----
        WvRole<C, CA> A;
        WvRole<C, CB> B;
        S.decode(A, s_role[lane], sumA, v0, CA);
        S.decode(B, s_role[64 + lane], sumB, v0, CB);
        WV_TICK(1)
        const bool wide_a = gather(A);
        const bool wide_b = gather(B);
        if (fail) break; // (C::SIDE) the side list does not fit: the contig goes to the kernel it falls back to
        S.narrow_w = !wide_a && !wide_b; // every cached weight is a sign-extended |w| < 2^51
        // In such a window a lane keeps (w << 4) + in-edge slot in the low half of each cached weight: the 64-bit phases then
        // form a candidate with one add, and the (rare) exact phase of the window shifts back.
        if (S.narrow_w) {
#pragma unroll
            for (int t = 0; t < CA; t++) A.cw[t] = C::with_lo(A.cw[t], (C::lo(A.cw[t]) << 4) | (uint64_t)t);
#pragma unroll
            for (int t = 0; t < CB; t++) B.cw[t] = C::with_lo(B.cw[t], (C::lo(B.cw[t]) << 4) | (uint64_t)t);
        }
        wv_sync();
        const T a_old = N::load(ring + (A.head ? A.slot : ZERO));

        WV_TICK(2)
        // ---- put the next window in flight ----
        const bool last = streamed ? va >= V : k + 1 >= n_win; // (k_wave_plan ends with the window that advances to the last node)
        if (!last) {
            if constexpr (STREAM) {
                if (!plan_done && k + 2 > n_win) { // the record of window k+1 is not published yet
                    const int w = wv_wait_plan(&meta->plan_prog, k + 2, n_win, plan_done);
                    if (w == 1) { __builtin_amdgcn_s_waitcnt(0); return; } // the planner gave up after all: the contig is somebody else's now, nothing of this sweep is needed (no DMA may be in flight into LDS when the wavefront ends)
                    if (w == 2) { fail = true; fail_code = 5; break; }
                }
                if (k + 1 >= rec_hi) load_recs(k);
            } else if (k + 1 - cbase >= 64) load_recs(k);
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): every LDS read of the staged data is done
            stage(k + 1);
        }

        WV_TICK(3)
        // ---- iterate to the fixed point ----
        if (!S.iterate(A, A.cw, A.cs, B, B.cw, B.cs)) { fail = true; fail_code = 3; break; }

        WV_TICK(4)
        // ---- results of the advanced nodes: distance, parent edge (contig-relative, the convention of k_sssp / k_sssp_lds;
        //      the walk at the end resolves it).  Kept in registers and stored after the next window's DMA wait. ----
        S.keep_results(A, B, v0, va, e0, SRC);

        // ---- did a close node that final nodes may depend on improve?  then step back ----
        const bool trig = S.watch_improved(A, a_old);
        const uint64_t tm = __ballot(trig);
        if (tm) {
            if (++S.rollbacks > 4 * (V / WV_ADV + 4)) { fail = true; fail_code = 4; break; }
            const int rr = S.step_back_node(A, trig, tm, v0, b, meta, 0);
            __builtin_amdgcn_s_waitcnt(0); // the DMA that is in flight lands in buffers we are about to reuse
            // the window that advances node rr: the last one that starts at or left of it
            int j = -1;
            while (true) {
                const uint64_t m = __ballot(cbase + lane <= k && (int)wr0.x <= rr);
                if (m) { j = cbase + 63 - __clzll((long long)m); break; }
                load_recs(cbase > 63 ? cbase - 63 : 0); // window 0 starts at node 0 <= rr
            }
            k = j;
            if constexpr (STREAM) { if (k + 1 >= rec_hi && rec_hi < n_win) load_recs(k); }
            else if (k + 1 - cbase >= 64) load_recs(k);
            stage(k);
            continue;
        }
        if (last) break;
        k++;
    }

    S.flush_results();
    if (fail) { // hand the contig to the workgroup kernel
        if (lane == 0) wv_hand_back(meta, b.tot, D::MODE, fail_code, streamed);
        return;
    }

#ifdef WV_PROFILE
    WV_TICK(5)
    if (lane == 0) {
        const WvProf &P = S.prof;
        S.prof.tick(10);
        for (int k = 0; k < 4; k++) meta->pmax[k] = (uint32_t)P.tp[k];
        meta->tr[0] = P.n_p64; meta->tr[1] = P.n_redo; meta->tr[2] = P.n_p128; meta->tr[3] = P.n_rebase;
        meta->tr[4] = P.mfA; meta->tr[5] = P.mfB; meta->tr[6] = P.bigA; meta->tr[7] = P.bigB;
        meta->bg[5] = (uint32_t)P.tp[10];
        meta->bg[6] = (uint32_t)(wall_clock64() - P.t_begin); meta->bg[7] = (uint32_t)n_win;
        meta->pmin[0] = (uint32_t)(P.tp[4] + P.tp[6] + P.tp[7] + P.tp[8] + P.tp[9]); meta->pmin[1] = (uint32_t)P.tp[5];
        meta->bg[0] = (uint32_t)P.tp[6]; meta->bg[1] = (uint32_t)P.tp[7]; meta->bg[2] = (uint32_t)P.tp[8]; meta->bg[3] = (uint32_t)P.tp[9]; meta->bg[4] = (uint32_t)P.tp[4];
    }
#endif
    S.finish(meta, V);
}
