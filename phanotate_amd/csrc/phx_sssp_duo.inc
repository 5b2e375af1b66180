// phx_sssp_duo.inc — k_sssp_wave's sweep for 128-bit contigs by TWO wavefronts per contig (included by phx_kernels.hip after
// phx_sssp_wave.inc, whose windows, lane records, rings and phases it shares: k_wave_plan, WvNum<2>, WvRole, wv_* helpers).
//
// Why: a contig's relaxation is a chain of ~370 dependent phases (fastpathz semantics, phanotate.py:56-64), and in k_sssp_wave the
// same wavefront also prepared every window — staged its in-edges, turned (source node, integer weight) into (ring slot, cached
// weight) per lane, read the window and lane records: per 50 kb contig 85 us of conversion and ~60 us of bookkeeping beside 220 us
// of phases, none of which depends on a distance.  Here the workgroup is two wavefronts:
//   * the SOLVER wavefront is a WvSolver (phx_sssp_wave.inc) over WvNum<2> and WvCw64 — the ring and the relative ring, the base move, the
//     lane-record decode, phase / phase64 and the phase loop, the pending results and parents, the step-back target, the tail and the
//     hand-back are k_sssp_wave's, one definition —, and per window only copies the lane pack out of LDS;
//   * the FEEDER wavefront runs one window ahead: it reads the window record, the lane records and the lanes' in-edges straight from
//     global memory (no staging area), converts them in registers and, as soon as the solver has taken the previous pack, writes the
//     next one to LDS: 20 cached (weight, source slot) pairs per lane, the lane records, a header.
// The two talk through a mailbox in LDS (sequence numbers, no s_barrier after the first): P_READY = packs published, C_ACK = packs
// taken or rejected, C_CMD what the solver wants after the pack it acknowledged.  The feeder speculates "the next window"; when the
// solver steps back (a watched close node improved, see k_sssp_wave) it rejects the speculated pack and names the node to step back
// to; the feeder finds the window.  Entries of the spill / side list (ov_*) are read by the phases, so a pack that needs them is
// written only after the solver has finished the window before (C_DONE): rare (nodes with more in-edges than a phase has lanes,
// weights beyond 2^51, sources that left the ring).
// Every spin is bounded: a hand-shake that does not complete hands the contig to the workgroup kernel (sssp_why 6) instead of hanging.
//
// Differences to k_sssp_wave<2>: cached weights are 64 bits wide (WvCw64) and the few in-edges that do not fit go to
// the side list in LDS, as in the 256- / 512-bit kernels; a final source is folded into a constant only when it has left the ring
// (its distance is in global memory, stored windows ago) or is the source node — the ring itself belongs to the solver.

template <int CFG> struct DuoDims;
template <> struct DuoDims<0> { static constexpr int RING = 512, OV = 192, MODE = 2; };
#define DUO_SLOTS 20 // cached in-edges per lane: 4 of phase A + 16 of phase B
#ifndef DUO_GT_LDS
#define DUO_GT_LDS 0 // 1: the contig's gap table (the weights of its coded gap edges, ESRC_F_GAP) as 32-bit entries in LDS; 0: the feeder reads DBatch.gtab — the
                     // source words first, then ONE load per in-edge from wherever its weight is.  Measured (1000 x 50 kb, A/B on one box): solver stage 0.41 ms
                     // as before with the table in global memory (6.4 KB per contig: it stays in the CU's L1), 0.425 with it in LDS (16 more LDS reads per
                     // window on the pipe the solver's phases live on, and 3.2 KB that a workgroup of another batch no longer finds beside four contigs)
#endif
template <int CFG>
constexpr size_t duo_lds_bytes() {
    typedef DuoDims<CFG> D;
    return (DUO_GT_LDS ? (size_t)GT_N * 4 : 0) + (size_t)(D::RING + 2) * 16 + (size_t)(D::RING + 2) * 8 + (size_t)DUO_SLOTS * 64 * 8 + (size_t)(DUO_SLOTS / 2) * 64 * 4 + 2 * 64 * 4 +
           (size_t)WIN_ROLES * 8 + (size_t)D::OV * 20 + 64 + 64;
}
static_assert(DUO_GT_LDS || 4 * duo_lds_bytes<0>() + 40 * 1024 + 64 <= 160 * 1024, "k_sssp_duo, tight configuration: a 40 KB workgroup fits beside four contigs per CU");

// mailbox words (LDS)
#define DUO_P_READY 0  // feeder -> solver: packs published
#define DUO_C_ACK 1    // solver -> feeder: packs taken or rejected
#define DUO_C_CMD 2    //   what comes after the acknowledged pack: -1 the next window (the feeder's guess), >= 0: step back to this node
#define DUO_C_LOADED 3 //   (with a step-back) nodes that have entered the solver's ring
#define DUO_C_DONE 4   // solver -> feeder: packs whose phases are over (or that were rejected)
#define DUO_C_EXIT 5   // solver -> feeder: leave
#define DUO_GO 6       // thread 0 -> all: this workgroup has a contig to solve
#define DUO_NWIN 7     //   (not streamed) its number of windows
// header words of a pack (LDS)
#define DUO_H_V0 0
#define DUO_H_VA 1
#define DUO_H_V1 2
#define DUO_H_E0 3
#define DUO_H_SUMA 4
#define DUO_H_SUMB 5
#define DUO_H_SPILL 6 // spill entries the planner laid out
#define DUO_H_FLAGS 7
#define DUO_F_NARROW 1  // every cached weight is (w << 4) | slot
#define DUO_F_LAST 2    // this window advances to the last node
#define DUO_F_END 4     // no window: the sweep is over unless the solver steps back
#define DUO_F_FAIL 8    // the feeder gives the contig up: code in DUO_H_CODE
#define DUO_F_ABANDON 16 // (streamed) the planner has redirected the contig itself: leave without a trace
#define DUO_H_CODE 8
#ifndef DUO_SPINS
#define DUO_SPINS (1 << 22) // polls of a mailbox word before a wavefront gives up (several ms; a hand-shake takes microseconds)
#endif

__device__ __forceinline__ uint32_t duo_peek(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void duo_poke(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// LDS only: what this wavefront wrote to LDS before is visible to a wavefront that sees what it writes after (no wait on global stores)
__device__ __forceinline__ void duo_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); }
__device__ __forceinline__ void duo_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); }

#ifdef DUO_PROFILE // the solver wavefront's clocks behind WvSolver's hook (tools/duo_balance.py reads what the kernel's tail copies to DMeta)
struct DuoProf {
    long long tp[4], tmark, t_begin, tab[2], tmark_ab;
    int nab[3];
    __device__ __forceinline__ void start() { for (int i = 0; i < 4; i++) tp[i] = 0; tab[0] = tab[1] = 0; nab[0] = nab[1] = nab[2] = 0; tmark = t_begin = tmark_ab = wall_clock64(); }
    __device__ __forceinline__ void tick(int k) { const long long t_ = wall_clock64(); tp[k] += t_ - tmark; tmark = t_; }
    __device__ __forceinline__ void fine(int) {}
    __device__ __forceinline__ void rebase() {}
    __device__ __forceinline__ void phase_done(int ph, bool, bool exact, int) {
#ifdef DUO_PROFILE_AB
        const long long t_ = wall_clock64(); tab[ph ? 1 : 0] += t_ - tmark_ab; tmark_ab = t_; nab[ph ? 1 : 0]++; if (exact) nab[2]++;
#endif
    }
};
#define DUO_TICK(k) S.prof.tick(k);
#else
typedef WvNoProf DuoProf;
#define DUO_TICK(k)
#endif

// SEG (phx_sssp_seg.inc): a workgroup solves one SEGMENT [ns, ne) of a contig in a frame of its own — nodes left of ns (and, beyond the
// first segment, the source node) count as unreached, the nodes of the first window start at distance 0 —, writes the distances to its
// slice of DBatch.sdist and its status to DBatch.segw; parents and the contig's records are k_seg_merge's.
template <int CFG, bool STREAM, bool SEG = false>
__global__ __launch_bounds__(128, 2) void k_sssp_duo(DBatch b) {
    // (SEG && STREAM: launched beside the segments' planner wavefronts, following DBatch.segw[segment][0] — batches behind k_front)
    typedef DuoDims<CFG> D;
    typedef WvNum<2> N;
    typedef N::T T;
    typedef WvCw64 C;
    typedef C::CW CW;
    constexpr int NL = 2, CA = N::CA, CB = N::CB, WV_RING = D::RING, WV_OV = D::OV, WV_SLOTS = WV_RING + 2;
    static_assert(CA == 4 && CB == 16 && CA + CB == DUO_SLOTS, "the lane pack holds 4 + 16 cached in-edges");
    __shared__ __align__(16) uint8_t smem[duo_lds_bytes<CFG>()]; // static: the kernel's only LDS, so every address below is a compile-time constant + lane part
    uint32_t *s_gt = (uint32_t *)smem;                               // (DUO_GT_LDS) the gap table; a code past it — only a slot beyond a lane's count holds one — reads the ring behind
    uint8_t *ring = smem + (DUO_GT_LDS ? (size_t)GT_N * 4 : 0);      // exact distances of the last RING nodes; slot RING = 0 (source), RING+1 = unreached
    uint8_t *rel = ring + (size_t)WV_SLOTS * NL * 8;                 // the same relative to `base`, 64 bits (k_sssp_wave)
    unsigned long long *pk_cw = (unsigned long long *)(rel + (size_t)WV_SLOTS * 8); // lane pack: cached weight of slot t of lane l at [t * 64 + l],
    uint32_t *pk_cs = (uint32_t *)(pk_cw + DUO_SLOTS * 64);          //   ring offsets of slots 2i, 2i+1 at [i * 64 + l] (16 bits each),
    uint32_t *pk_sd = pk_cs + (DUO_SLOTS / 2) * 64;                  //   side-list ranges of the lane's phase A / phase B role (first | end << 16)
    uint2 *s_role = (uint2 *)(pk_sd + 2 * 64);                       // lane records of the window (k_wave_plan)
    uint8_t *ov_w = (uint8_t *)(s_role + WIN_ROLES);                 // spill + side list: weight,
    uint32_t *ov_s = (uint32_t *)(ov_w + (size_t)WV_OV * NL * 8);    //   ring offset of the source (| slot << 24 on the side list)
    int *hdr = (int *)(ov_s + WV_OV);
    uint32_t *mb = (uint32_t *)(hdr + 16);

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const bool feeder = tid >= 64;
    DMeta *meta = &b.meta[SEG ? (int)blockIdx.x / b.seg : (b.sord ? b.sord[blockIdx.x] : (int)blockIdx.x)];
    const int seg_s = SEG ? (int)blockIdx.x % b.seg : 0;
    int32_t *seg_rec = SEG ? b.segw + SEG_REC * (size_t)blockIdx.x : nullptr; // (SEG) {windows of the segment, status of its solver}
    // one thread decides whether this workgroup runs: in a streamed launch the planner may redirect the contig (sssp_mode) at any moment,
    // and the two wavefronts must not see different answers
    if (tid == 0) {
        int go = 0, nw = 0;
        if (!b.tot->overflow) {
            const int V0 = meta->n_node;
            if (meta->status >= 0 && V0 > 2 && meta->sssp_nl == NL && meta->sssp_mode == D::MODE) { go = 1; nw = STREAM ? 0 : meta->n_win; }
            if (!SEG && b.seg && !meta->seg_fail) go = 0; // (DBatch.seg: this launch is the one sweep behind the segments, for the contigs they could not take)
            if constexpr (SEG) {
                if (go) {
                    go = V0 <= SEG_VMAX && seg_s < seg_geo(b, meta).K;
                    if (!STREAM) { nw = go ? seg_rec[0] : 0; if (nw <= 0) go = 0; else nw &= WV_PLAN_DONE - 1; } // (a segment without windows: k_seg_join gives the contig up)
                }
            }
        }
        for (int i = 0; i < 16; i++) mb[i] = 0;
        mb[DUO_GO] = (uint32_t)go; mb[DUO_NWIN] = (uint32_t)nw;
    }
    __syncthreads();
    if (!mb[DUO_GO]) return;
    const int V = meta->n_node;
    const int SRC = V - 2;
    typedef WvSolver<N, C, WV_RING, WV_OV, !SEG, DuoProf> Solver;
    constexpr uint32_t ZERO = Solver::ZERO, INF = Solver::INF;
    int seg_ns = 0, seg_ne = V; // the node range of this sweep
    size_t seg_w = 0;
    if constexpr (SEG) { int cs_; const SegRank rk(b, meta); seg_range(seg_geo(b, meta), rk, V, seg_s, seg_ns, cs_, seg_ne); seg_w = seg_win_off(b, meta, seg_s); } // (the same cut as the segment's planner)
    uint64_t *gdist = SEG ? b.sdist + ((size_t)seg_s * (size_t)b.sdist_nodes + (size_t)meta->node_off) * NL : b.dist + (size_t)meta->node_off * b.dist_stride;
    constexpr uint32_t PADU_ = 0x3ffffffeu; // a source that is never loaded: pads a lane's in-edge list

#ifdef DUO_HWID // development: where the hardware put the two wavefronts (tools/duo_hwid.py): HW_ID (wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13) and XCC_ID
    if (lane == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        meta->tr[feeder ? 21 : 20] = hw; meta->tr[feeder ? 23 : 22] = xcc;
    }
#endif
    if (feeder) {
        // =========================================== the feeder ===========================================
        const uint32_t *esrc = b.esrc + meta->edge_off;
        const long long *ew = b.ew + meta->edge_off;
        const long long *gt = b.gtab + (size_t)(meta - b.meta) * GT_N; // weights of the coded gap edges (k_edges<true>; all below 2^31 where an edge refers to them)
        if (DUO_GT_LDS) for (int i = lane; i < GT_N; i += 64) s_gt[i] = (uint32_t)gt[i];
        auto gap_w = [&](uint32_t sw) -> long long { return DUO_GT_LDS ? (long long)s_gt[ESRC_GAP_CODE(sw)] : gt[ESRC_GAP_CODE(sw) < GT_N ? ESRC_GAP_CODE(sw) : 0u]; };
        const DWin *win = SEG ? b.swin + seg_w : b.win + meta->win_off;
        const uint2 *wrole = SEG ? b.swrole + seg_w * WIN_ROLES : b.wrole + (size_t)meta->win_off * WIN_ROLES;
        int n_win = STREAM ? 0 : (int)mb[DUO_NWIN];
        bool plan_done = !STREAM;
        auto wait_plan = [&](int need) { return wv_wait_plan(SEG ? seg_rec : &meta->plan_prog, need, n_win, plan_done); }; // (the word the planner this feeder follows publishes)
        int pseq = 0; // packs published
#ifdef DUO_PROFILE
        long long ft[4] = {0, 0, 0, 0}, fmark = wall_clock64(); int f_ov = 0;
#define DUO_FTICK(k) { const long long t_ = wall_clock64(); ft[k] += t_ - fmark; fmark = t_; }
#define DUO_FDUMP() { if (lane == 0) { for (int q_ = 0; q_ < 4; q_++) meta->tr[q_] = (uint32_t)ft[q_]; meta->tr[4] = (uint32_t)f_ov; meta->tr[5] = (uint32_t)pseq; } }
#else
#define DUO_FTICK(k)
#define DUO_FDUMP()
#endif
        // a pack that is only a header (end of the sweep, failure): the solver has nothing else to read
        auto publish_flags = [&](int flags, int code) -> bool { // false: the solver has left
            for (int spins = 0; (int)duo_peek(&mb[DUO_C_ACK]) != pseq; spins++) {
                if (duo_peek(&mb[DUO_C_EXIT]) || spins > DUO_SPINS) return false;
                __builtin_amdgcn_s_sleep(2);
            }
            duo_acquire();
            if (lane == 0) { hdr[DUO_H_FLAGS] = flags; hdr[DUO_H_CODE] = code; }
            duo_release();
            pseq++;
            if (lane == 0) duo_poke(&mb[DUO_P_READY], (uint32_t)pseq);
            return true;
        };
        if (!STREAM && n_win <= 0) { publish_flags(DUO_F_FAIL, 1); return; }
        if (STREAM) {
            const int wp = wait_plan(1);
            if (wp == 1) { publish_flags(DUO_F_ABANDON, 0); return; }
            if (wp == 2) { publish_flags(DUO_F_FAIL, 5); return; }
        }
        int pl_loaded = seg_ns; // nodes in the solver's ring once it has taken every pack published so far
        int w = 0;         // window to produce; -1: the end marker
        int last_w = 0;    // the last real window a pack was published for
        for (;;) {
            // ---------- part 1, in registers, while the solver is still busy with the pack before ----------
            int v0 = 0, va = 0, v1 = 0, n_spill = 0, loaded = pl_loaded, flags = 0;
            uint32_t e0 = 0, sumA = 0, sumB = 0;
            uint2 rcA = make_uint2(0, 0), rcB = make_uint2(0, 0);
            uint32_t ruA[CA], ruB[CB], csA[CA], csB[CB];
            long long rwA[CA], rwB[CB];
            CW cwA[CA], cwB[CB];
            uint32_t slowA = 0, slowB = 0;
            int ring_lo = 0;
            if (w >= 0) {
                if (STREAM && !plan_done && w + 1 > n_win) {
                    const int wp = wait_plan(w + 1);
                    if (wp == 1) { publish_flags(DUO_F_ABANDON, 0); return; }
                    if (wp == 2) { publish_flags(DUO_F_FAIL, 5); return; }
                }
                const uint4 r0 = ((const uint4 *)(win + w))[0], r1 = ((const uint4 *)(win + w))[1];
                rcA = wrole[(size_t)w * WIN_ROLES + lane];
                rcB = wrole[(size_t)w * WIN_ROLES + 64 + lane];
                v0 = __builtin_amdgcn_readfirstlane((int)r0.x); va = __builtin_amdgcn_readfirstlane((int)r0.y); v1 = __builtin_amdgcn_readfirstlane((int)r0.z);
                e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r0.w);
                sumA = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1.y); sumB = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1.z);
                n_spill = __builtin_amdgcn_readfirstlane((int)r1.w);
                if (v1 > loaded) loaded = v1;
                ring_lo = loaded - WV_RING;
                const int maxA = wv_sum_maxcnt(sumA), maxB = wv_sum_maxcnt(sumB);
                const int cntA = wv_role_cnt(rcA), cntB = wv_role_cnt(rcB);
                const uint32_t ebA = e0 + (uint32_t)wv_role_ebase(rcA), ebB = e0 + (uint32_t)wv_role_ebase(rcB);
                // the lanes' in-edges, all in flight together (slots past a lane's count read what follows: other lanes' in-edges, the next
                // contig's, or the slack behind the arrays; they are masked below)
#pragma unroll
                for (int t = 0; t < CA; t++) { ruA[t] = PADU_; rwA[t] = 0; }
#pragma unroll
                for (int t = 0; t < CB; t++) { ruB[t] = PADU_; rwB[t] = 0; }
                if (DUO_GT_LDS) {
                    if (maxA > 0) {
#pragma unroll
                        for (int t = 0; t < CA; t++) { ruA[t] = esrc[ebA + t]; rwA[t] = ew[ebA + t]; }
                    }
#pragma unroll
                    for (int t0 = 0; t0 < CB; t0 += 4) {
                        if (t0 >= maxB) break;
#pragma unroll
                        for (int g = 0; g < 4; g++) { ruB[t0 + g] = esrc[ebB + t0 + g]; rwB[t0 + g] = ew[ebB + t0 + g]; }
                    }
                    // a coded gap edge has no entry in DBatch.ew (what was loaded for it is whatever an earlier batch left there): its weight is the table's
                    if (maxA > 0) {
#pragma unroll
                        for (int t = 0; t < CA; t++) if (ESRC_IS_GAP(ruA[t])) rwA[t] = gap_w(ruA[t]);
                    }
#pragma unroll
                    for (int t0 = 0; t0 < CB; t0 += 4) {
                        if (t0 >= maxB) break;
#pragma unroll
                        for (int g = 0; g < 4; g++) if (ESRC_IS_GAP(ruB[t0 + g])) rwB[t0 + g] = gap_w(ruB[t0 + g]);
                    }
                } else { // the source words first, then ONE load per in-edge from wherever its weight is
                    if (maxA > 0) {
#pragma unroll
                        for (int t = 0; t < CA; t++) ruA[t] = esrc[ebA + t];
                    }
#pragma unroll
                    for (int t0 = 0; t0 < CB; t0 += 4) {
                        if (t0 >= maxB) break;
#pragma unroll
                        for (int g = 0; g < 4; g++) ruB[t0 + g] = esrc[ebB + t0 + g];
                    }
                    if (maxA > 0) {
#pragma unroll
                        for (int t = 0; t < CA; t++) rwA[t] = *(ESRC_IS_GAP(ruA[t]) ? gt + (ESRC_GAP_CODE(ruA[t]) < GT_N ? ESRC_GAP_CODE(ruA[t]) : 0u) : ew + ebA + t);
                    }
#pragma unroll
                    for (int t0 = 0; t0 < CB; t0 += 4) {
                        if (t0 >= maxB) break;
#pragma unroll
                        for (int g = 0; g < 4; g++) rwB[t0 + g] = *(ESRC_IS_GAP(ruB[t0 + g]) ? gt + (ESRC_GAP_CODE(ruB[t0 + g]) < GT_N ? ESRC_GAP_CODE(ruB[t0 + g]) : 0u) : ew + ebB + t0 + g);
                    }
                }
                // (source node, integer weight) -> (ring offset, cached weight): k_sssp_wave's gather, common path
                auto convert = [&](auto capc, const int cnt, const int maxcnt, const uint32_t *ru, const long long *rw, uint32_t *cs, CW *cw) -> uint32_t {
                    constexpr int cap = decltype(capc)::value;
                    uint32_t slow = 0;
#pragma unroll
                    for (int t0 = 0; t0 < cap; t0 += 4) {
                        if (t0 >= maxcnt) {
#pragma unroll
                            for (int g = 0; g < 4; g++) { cs[t0 + g] = INF; cw[t0 + g] = 0; }
                            continue;
                        }
                        uint32_t u[4];
                        long long wt[4];
                        uint32_t acc = 0;
                        bool special = false;
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const bool on = t0 + g < cnt;
                            acc |= ru[t0 + g];
                            u[g] = on ? ESRC_NODE(ru[t0 + g]) : PADU_;
                            wt[g] = on ? rw[t0 + g] : 0ll;
                            special |= (int)u[g] < ring_lo;
                        }
                        special |= ESRC_OFFPATH(acc) != 0u;
                        if (__ballot(special) == 0ull) {
#pragma unroll
                            for (int g = 0; g < 4; g++) {
                                cs[t0 + g] = (int)u[g] >= loaded ? INF : (u[g] & (WV_RING - 1)) * NL * 8;
                                cw[t0 + g] = wt[g];
                            }
                            continue;
                        }
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            const bool on = t0 + g < cnt;
                            const bool isrc = u[g] == (uint32_t)SRC;
                            const bool outside = SEG && on && (isrc ? seg_s > 0 : (int)u[g] < seg_ns); // (SEG) a source this segment's frame does not reach
                            const bool beyond = !on || ((int)u[g] >= loaded && !isrc) || outside;
                            const bool far = on && !isrc && (int)u[g] < ring_lo && !outside;
                            cs[t0 + g] = beyond ? INF : ((isrc || far) ? ZERO : (u[g] & (WV_RING - 1)) * NL * 8);
                            cw[t0 + g] = beyond ? 0ll : wt[g];
                            if (on && !outside && (far || !ew_narrow51(wt[g]))) slow |= 1u << (t0 + g);
                        }
                    }
                    return slow;
                };
                slowA = convert(std::integral_constant<int, CA>(), cntA, maxA, ruA, rwA, csA, cwA);
                slowB = convert(std::integral_constant<int, CB>(), cntB, maxB, ruB, rwB, csB, cwB);
                if (va >= seg_ne) flags |= DUO_F_LAST;
            } else flags = DUO_F_END;
            const bool any_slow = __ballot((slowA | slowB) != 0u) != 0ull;
            DUO_FTICK(0)
            const bool needs_ov = w >= 0 && (any_slow || n_spill != 0);

            // ---------- the solver has taken (or rejected) the pack before ----------
            bool gone = false;
            for (int spins = 0; (int)duo_peek(&mb[DUO_C_ACK]) != pseq; spins++) {
                if (duo_peek(&mb[DUO_C_EXIT]) || spins > DUO_SPINS) { gone = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (gone) { DUO_FDUMP() return; }
            duo_acquire();
            DUO_FTICK(1)
            if (pseq > 0) {
                const int cmd = (int)duo_peek(&mb[DUO_C_CMD]);
                if (cmd >= 0) { // rejected: the solver steps back to node cmd — the last window that starts at or left of it
                    pl_loaded = (int)duo_peek(&mb[DUO_C_LOADED]);
                    int j = 0;
                    for (int hi = last_w;; hi -= 64) {
                        const int idx = hi - 63 + lane;
                        const bool ok = idx >= 0 && win[idx < 0 ? 0 : idx].v0 <= cmd;
                        const uint64_t m = __ballot(ok);
                        if (m) { j = hi - 63 + (63 - __clzll((long long)m)); break; }
                        if (hi < 64) break; // (window 0 starts at node 0: not reached)
                    }
                    w = j;
                    // the rejected pack counts as taken: produce window j in its place
                    if (lane == 0) duo_poke(&mb[DUO_C_CMD], 0xffffffffu);
                    duo_release();
                    continue;
                }
            }
            if (w < 0) { // the end marker: published once, then the solver either leaves (C_EXIT) or steps back
                if (lane == 0) { hdr[DUO_H_FLAGS] = DUO_F_END; hdr[DUO_H_CODE] = 0; }
                duo_release();
                pseq++;
                if (lane == 0) duo_poke(&mb[DUO_P_READY], (uint32_t)pseq);
                // wait for its rejection (a step-back) or the exit
                for (int spins = 0; (int)duo_peek(&mb[DUO_C_ACK]) != pseq; spins++) {
                    if (duo_peek(&mb[DUO_C_EXIT]) || spins > DUO_SPINS) { DUO_FDUMP() return; }
                    __builtin_amdgcn_s_sleep(4);
                }
                duo_acquire();
                const int cmd = (int)duo_peek(&mb[DUO_C_CMD]);
                if (cmd < 0) return; // (an accepted end marker does not exist)
                pl_loaded = (int)duo_peek(&mb[DUO_C_LOADED]);
                int j = 0;
                for (int hi = last_w;; hi -= 64) {
                    const int idx = hi - 63 + lane;
                    const bool ok = idx >= 0 && win[idx < 0 ? 0 : idx].v0 <= cmd;
                    const uint64_t m = __ballot(ok);
                    if (m) { j = hi - 63 + (63 - __clzll((long long)m)); break; }
                    if (hi < 64) break;
                }
                w = j;
                if (lane == 0) duo_poke(&mb[DUO_C_CMD], 0xffffffffu);
                duo_release();
                continue;
            }

            // ---------- part 2 (rare): in-edges that do not fit a cached slot, spill entries: the phases of the window before must be over ----------
            uint32_t sdA = 0, sdB = 0;
            bool wide_w = false;
            int fail_code = 0;
            if (needs_ov) {
#ifdef DUO_PROFILE
                f_ov++;
#endif
                bool gone2 = false;
                for (int spins = 0; (int)duo_peek(&mb[DUO_C_DONE]) < pseq; spins++) {
                    if (duo_peek(&mb[DUO_C_EXIT]) || spins > DUO_SPINS) { gone2 = true; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (gone2) return;
                duo_acquire();
                int sd_next = n_spill;
                auto side = [&](auto capc, const uint32_t slow, const uint32_t *ru, const long long *rw, uint32_t *cs, CW *cw) -> uint32_t {
                    constexpr int cap = decltype(capc)::value;
                    if (__ballot(slow != 0u) == 0ull) return 0u;
                    wide_w = true;
                    // a final source outside the ring (or the source node): distance + weight is a constant while the window iterates; the lane
                    // keeps the best of them (lowest slot among equals) as one entry over the constant-0 slot.  Every other one: ring[source] +
                    // exact weight on the side list; the register slot is disabled.
                    uint32_t sidem = 0;
                    T fc = N::top();
                    int fce = -1;
#pragma unroll
                    for (int t = 0; t < cap; t++)
                        if (__ballot((slow >> t) & 1u)) {
                            if ((slow >> t) & 1u) {
                                const uint32_t u = ESRC_NODE(ru[t]);
                                const long long wi = rw[t];
                                if (u == (uint32_t)SRC || (int)u < ring_lo) {
                                    const T wv = EW_WIDE(wi) ? N::from_double(__longlong_as_double(wi | (1ll << 62))) : N::from_i64(wi);
                                    T d = N::zero();
                                    if (u != (uint32_t)SRC) { // stored by the solver several windows ago; read past this CU's L1
                                        d.lo = __hip_atomic_load(gdist + (size_t)u * NL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        d.hi = __hip_atomic_load(gdist + (size_t)u * NL + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    }
                                    const T c = N::add(d, wv);
                                    if (!N::unreached(d) && N::lt(c, fc)) { fc = c; fce = t; }
                                    cs[t] = INF;
                                } else sidem |= 1u << t;
                                cw[t] = 0ll;
                            }
                        }
                    const int c = __popc(sidem) + (fce >= 0 ? 1 : 0);
                    const int incl = (int)wv_scan((uint32_t)c);
                    const int total = wv_last(incl);
                    const int s0 = sd_next + incl - c, s1 = s0 + c;
                    if (sd_next + total > WV_OV) { fail_code = 2; return 0u; }
                    int i = s0;
                    if (fce >= 0) { ov_s[i] = ZERO | ((uint32_t)fce << 24); N::store(ov_w + (size_t)i * NL * 8, fc); i++; }
                    if (__ballot(sidem != 0u)) {
#pragma unroll
                        for (int t = 0; t < cap; t++)
                            if (__ballot((sidem >> t) & 1u)) {
                                if ((sidem >> t) & 1u) {
                                    const long long wi = rw[t];
                                    const T wv = EW_WIDE(wi) ? N::from_double(__longlong_as_double(wi | (1ll << 62))) : N::from_i64(wi);
                                    ov_s[i] = cs[t] | ((uint32_t)t << 24);
                                    N::store(ov_w + (size_t)i * NL * 8, wv);
                                    i++;
                                    cs[t] = INF;
                                }
                            }
                    }
                    sd_next += total;
                    return (uint32_t)s0 | ((uint32_t)s1 << 16);
                };
                // the planner's spill entries of a head lane: in-edges beyond its helper lanes
                auto spill = [&](const int cap, const uint2 rc) {
                    if (!wv_role_act(rc) || wv_role_ch(rc) != 0) return;
                    const int sp0 = wv_role_sp0(rc), sp1 = sp0 + wv_role_spn(rc);
                    const uint32_t spe = e0 + (uint32_t)wv_role_ebase(rc) + (uint32_t)((wv_role_nfollow(rc) + 1) * cap);
                    for (int i = sp0; i < sp1 && i < WV_OV; i++) {
                        const uint32_t sws = esrc[spe + (uint32_t)(i - sp0)];
                        const uint32_t u = ESRC_NODE(sws);
                        const long long wd = ESRC_IS_GAP(sws) ? gap_w(sws) : ew[spe + (uint32_t)(i - sp0)];
                        const bool isrc = u == (uint32_t)SRC;
                        const bool outside = SEG && (isrc ? seg_s > 0 : (int)u < seg_ns);
                        const bool beyond = ((int)u >= loaded && !isrc) || outside;
                        const bool far = !isrc && (int)u < ring_lo && !outside;
                        const uint32_t sl = beyond ? INF : ((isrc || far) ? ZERO : (u & (WV_RING - 1)) * NL * 8);
                        T wv = N::from_i64(beyond ? 0ll : wd);
                        if (!outside && (far || !ew_narrow51(wd))) {
                            wv = EW_WIDE(wd) ? N::from_double(__longlong_as_double(wd | (1ll << 62))) : N::from_i64(wd);
                            if (far) {
                                T d;
                                d.lo = __hip_atomic_load(gdist + (size_t)u * NL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                d.hi = __hip_atomic_load(gdist + (size_t)u * NL + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                wv = N::add(wv, d);
                            }
                            wide_w = true;
                        }
                        ov_s[i] = sl;
                        N::store(ov_w + (size_t)i * NL * 8, wv);
                    }
                };
                sdA = side(std::integral_constant<int, CA>(), slowA, ruA, rwA, csA, cwA);
                if (!fail_code) sdB = side(std::integral_constant<int, CB>(), slowB, ruB, rwB, csB, cwB);
                if (!fail_code && n_spill != 0) { spill(CA, rcA); spill(CB, rcB); }
                fail_code = __ballot(fail_code != 0) ? 2 : 0;
                wide_w = __ballot(wide_w) != 0ull;
            }
            if (fail_code) { // the side list does not fit: the contig goes to the kernel it falls back to
                if (lane == 0) { hdr[DUO_H_FLAGS] = DUO_F_FAIL; hdr[DUO_H_CODE] = fail_code; }
                duo_release();
                pseq++;
                if (lane == 0) duo_poke(&mb[DUO_P_READY], (uint32_t)pseq);
                return;
            }
            DUO_FTICK(2)
            if (!wide_w) {
                flags |= DUO_F_NARROW;
#pragma unroll
                for (int t = 0; t < CA; t++) cwA[t] = (CW)(((uint64_t)cwA[t] << 4) | (uint64_t)t);
#pragma unroll
                for (int t = 0; t < CB; t++) cwB[t] = (CW)(((uint64_t)cwB[t] << 4) | (uint64_t)t);
            }
            // ---------- the pack ----------
            {
                const int maxA = wv_sum_maxcnt(sumA), maxB = wv_sum_maxcnt(sumB);
                if (maxA > 0) {
#pragma unroll
                    for (int t = 0; t < CA; t++) pk_cw[t * 64 + lane] = (unsigned long long)cwA[t];
#pragma unroll
                    for (int t = 0; t < CA; t += 2) pk_cs[(t / 2) * 64 + lane] = csA[t] | (csA[t + 1] << 16);
                }
#pragma unroll
                for (int t0 = 0; t0 < CB; t0 += 4) {
                    if (t0 >= maxB) break;
#pragma unroll
                    for (int g = 0; g < 4; g++) pk_cw[(CA + t0 + g) * 64 + lane] = (unsigned long long)cwB[t0 + g];
#pragma unroll
                    for (int g = 0; g < 4; g += 2) pk_cs[((CA + t0 + g) / 2) * 64 + lane] = csB[t0 + g] | (csB[t0 + g + 1] << 16);
                }
                pk_sd[lane] = sdA; pk_sd[64 + lane] = sdB;
                s_role[lane] = rcA; s_role[64 + lane] = rcB;
                if (lane == 0) {
                    hdr[DUO_H_V0] = v0; hdr[DUO_H_VA] = va; hdr[DUO_H_V1] = v1; hdr[DUO_H_E0] = (int)e0;
                    hdr[DUO_H_SUMA] = (int)sumA; hdr[DUO_H_SUMB] = (int)sumB; hdr[DUO_H_SPILL] = n_spill; hdr[DUO_H_FLAGS] = flags; hdr[DUO_H_CODE] = 0;
                }
            }
            duo_release();
            pseq++;
            if (lane == 0) duo_poke(&mb[DUO_P_READY], (uint32_t)pseq);
            DUO_FTICK(3)
            pl_loaded = loaded;
            last_w = w;
            w = (flags & DUO_F_LAST) ? -1 : w + 1;
        }
        return;
    }

    // =========================================== the solver ===========================================
    __builtin_amdgcn_s_setprio(3); // the phases are the critical path: this wavefront goes first wherever it shares a SIMD with feeders (or another batch's kernels)
    int32_t *gpe = b.parent + meta->node_off; // parent edge of every node (contig-relative), -1: none (SEG: k_seg_merge picks them)
    Solver S;
    S.init(ring, rel, ov_w, ov_s, gdist, gpe, lane);
    int loaded = seg_ns;
    const long long seg_t0 = SEG ? wall_clock64() : 0ll;
    bool seed = SEG && seg_s > 0; // (SEG) the nodes of the frame's first 500 bp start at 0: any frame will do, the paths behind them merge within the margin
    bool fail = false;
    int fail_code = 0;
    int seq = 0;      // packs taken or rejected
    int pend_rr = -1; // a step-back is pending: the next pack is the feeder's guess and is rejected
    bool abandoned = false;
#ifdef DUO_PROFILE
    S.prof.start();
#endif
    wv_sync();
    while (true) {
        DUO_TICK(3)
        // ---- the next pack ----
        const int want = seq + 1;
        {
            bool lost = false;
            for (int spins = 0; (int)duo_peek(&mb[DUO_P_READY]) != want; spins++)
                if (spins > DUO_SPINS) { lost = true; break; }
            if (lost) { fail = true; fail_code = 6; break; }
        }
        duo_acquire();
        DUO_TICK(0)
        const int flags = __builtin_amdgcn_readfirstlane(hdr[DUO_H_FLAGS]);
        if (flags & DUO_F_ABANDON) { abandoned = true; break; }
        if (flags & DUO_F_FAIL) { fail = true; fail_code = __builtin_amdgcn_readfirstlane(hdr[DUO_H_CODE]); break; }
        if (pend_rr >= 0) { // not the window this sweep continues with: name the node to step back to
            if (lane == 0) { duo_poke(&mb[DUO_C_CMD], (uint32_t)pend_rr); duo_poke(&mb[DUO_C_LOADED], (uint32_t)loaded); duo_poke(&mb[DUO_C_DONE], (uint32_t)want); }
            duo_release();
            if (lane == 0) duo_poke(&mb[DUO_C_ACK], (uint32_t)want);
            seq = want; pend_rr = -1;
            continue;
        }
        // (DUO_F_END cannot arrive here: after the last window the solver leaves or steps back)
        const int v0 = __builtin_amdgcn_readfirstlane(hdr[DUO_H_V0]), va = __builtin_amdgcn_readfirstlane(hdr[DUO_H_VA]), v1 = __builtin_amdgcn_readfirstlane(hdr[DUO_H_V1]);
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane(hdr[DUO_H_E0]);
        const uint32_t sumA = (uint32_t)__builtin_amdgcn_readfirstlane(hdr[DUO_H_SUMA]), sumB = (uint32_t)__builtin_amdgcn_readfirstlane(hdr[DUO_H_SUMB]);
        S.has_spill = __builtin_amdgcn_readfirstlane(hdr[DUO_H_SPILL]) != 0;
        S.narrow_w = (flags & DUO_F_NARROW) != 0;
        const bool last = (flags & DUO_F_LAST) != 0;
        __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0): the results stored a window ago are in memory (the feeder may read them windows later)
        S.flush_results();
        // ---- nodes that enter the ring ----
        int seed_end = loaded; // (SEG, first window of a frame without the source) the nodes of its first 500 bp start at distance 0
        if constexpr (SEG) {
            if (seed) {
                const DNode *nd = b.node + meta->node_off;
                const int p0 = nd[seg_ns].pos + SEG_SEED_BP;
                const int i1 = seg_ns + lane, i2 = seg_ns + 64 + lane;
                const bool s1 = i1 < v1 && i1 < SRC && nd[i1].pos < p0, s2 = i2 < v1 && i2 < SRC && nd[i2].pos < p0;
                seed_end = seg_ns + __popcll(__ballot(s1)) + __popcll(__ballot(s2)); // (positions ascend: the seeds are a prefix)
                seed = false;
            }
        }
        for (int i = loaded + lane; i < v1; i += 64) { // unreached, all of them ...
            const bool sd = SEG && i < seed_end;
            N::store(ring + (size_t)(i & (WV_RING - 1)) * NL * 8, sd ? N::zero() : N::big());
            *(long long *)(rel + (size_t)(i & (WV_RING - 1)) * 8) = sd ? WV_REL(0) : WV_REL_BIG;
        }
        if (SRC >= loaded && SRC < v1 && lane == 0 && seg_s == 0) { // ... but the source node (the last but one node: one of the last windows)
            bool low;
            N::store(ring + (size_t)(SRC & (WV_RING - 1)) * NL * 8, N::zero());
            *(long long *)(rel + (size_t)(SRC & (WV_RING - 1)) * 8) = S.to_rel(N::zero(), low);
        }
        if (v1 > loaded) loaded = v1;
        wv_sync();
        S.move_base();
        // ---- the lanes of the two phases: records and cached in-edges from the pack ----
        WvLane A, B;
        CW cwA[CA], cwB[CB]; // (beside the lanes, not inside a WvRole: see there for what that cost)
        uint32_t csA[CA], csB[CB];
        S.decode(A, s_role[lane], sumA, v0, CA);
        S.decode(B, s_role[64 + lane], sumB, v0, CB);
        { const uint32_t sa = pk_sd[lane], sb = pk_sd[64 + lane]; A.sd0 = (int)(sa & 0xffffu); A.sd1 = (int)(sa >> 16); B.sd0 = (int)(sb & 0xffffu); B.sd1 = (int)(sb >> 16); }
        if (A.maxcnt > 0) {
#pragma unroll
            for (int t = 0; t < CA; t++) cwA[t] = (CW)pk_cw[t * 64 + lane];
#pragma unroll
            for (int t = 0; t < CA; t += 2) { const uint32_t p = pk_cs[(t / 2) * 64 + lane]; csA[t] = p & 0xffffu; csA[t + 1] = p >> 16; }
        } else {
#pragma unroll
            for (int t = 0; t < CA; t++) { cwA[t] = 0; csA[t] = INF; }
        }
#pragma unroll
        for (int t0 = 0; t0 < CB; t0 += 4) {
            if (t0 >= B.maxcnt) {
#pragma unroll
                for (int g = 0; g < 4; g++) { cwB[t0 + g] = 0; csB[t0 + g] = INF; }
                continue;
            }
#pragma unroll
            for (int g = 0; g < 4; g++) cwB[t0 + g] = (CW)pk_cw[(CA + t0 + g) * 64 + lane];
#pragma unroll
            for (int g = 0; g < 4; g += 2) { const uint32_t p = pk_cs[((CA + t0 + g) / 2) * 64 + lane]; csB[t0 + g] = p & 0xffffu; csB[t0 + g + 1] = p >> 16; }
        }
        const T a_old = N::load(ring + (A.head ? A.slot : ZERO));
        // the pack is in registers: the feeder may write the next one
        duo_release();
        if (lane == 0) { duo_poke(&mb[DUO_C_CMD], 0xffffffffu); duo_poke(&mb[DUO_C_ACK], (uint32_t)want); }
        seq = want;
        DUO_TICK(1)

        // ---- iterate to the fixed point ----
#ifdef DUO_PROFILE_AB
        S.prof.tmark_ab = wall_clock64();
#endif
        if (!S.iterate(A, cwA, csA, B, cwB, csB)) { fail = true; fail_code = 3; break; }
        DUO_TICK(2)
        // the phases of this pack are over: the spill / side list may be rewritten
        if (lane == 0) duo_poke(&mb[DUO_C_DONE], (uint32_t)seq);

        // ---- results of the advanced nodes (stored at the top of the next window) ----
        S.keep_results(A, B, v0, va, e0, SRC);

        // ---- did a close node that final nodes may depend on improve?  then step back (k_sssp_wave) ----
        const bool trig = S.watch_improved(A, a_old);
        const uint64_t tm = __ballot(trig);
        if (tm) {
            if (++S.rollbacks > 4 * (V / WV_ADV + 4)) { fail = true; fail_code = 4; break; }
            pend_rr = S.step_back_node(A, trig, tm, v0, b, meta, seg_ns);
            continue;
        }
        if (last) break;
    }
    if (lane == 0) duo_poke(&mb[DUO_C_EXIT], 1u);
    if (abandoned) return;
    S.flush_results();
    if constexpr (SEG) {
        if (lane == 0) {
            seg_rec[1] = fail ? (fail_code ? fail_code : 7) : 0; atomicAdd(&meta->sssp_iters, S.phases);
            seg_rec[4] = (int32_t)(wall_clock64() - seg_t0); seg_rec[5] = S.phases; seg_rec[6] = seq; seg_rec[7] = S.rollbacks;
            if (fail && fail_code == 5) atomicAdd(&b.tot->plan_timeouts, 1); // (the planner it follows made no progress: the host stops launching solvers beside planners on this context)
        }
        return;
    }
    if (fail) { // hand the contig to the workgroup kernel
        if (lane == 0) wv_hand_back(meta, b.tot, D::MODE, fail_code, STREAM);
        return;
    }
#ifdef DUO_PROFILE
    if (lane == 0) {
        const DuoProf &P = S.prof;
        S.prof.tick(3);
        for (int q_ = 0; q_ < 4; q_++) meta->pmax[q_] = (uint32_t)P.tp[q_];
        meta->bg[6] = (uint32_t)(wall_clock64() - P.t_begin); meta->bg[7] = (uint32_t)seq;
#ifdef DUO_PROFILE_AB
        meta->bg[0] = (uint32_t)P.tab[0]; meta->bg[1] = (uint32_t)P.tab[1]; meta->bg[2] = (uint32_t)P.nab[0]; meta->bg[3] = (uint32_t)P.nab[1]; meta->bg[4] = (uint32_t)P.nab[2];
#endif
    }
#endif
    S.finish(meta, V);
}
