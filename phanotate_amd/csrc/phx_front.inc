// phx_front.inc — k_front: the front end of a SMALL batch in one launch (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// A lone contig (BASELINE configs 2-3) or a handful of them leave the chip empty: between k_features and the shortest path a run is
// two dozen kernels of 6-25 us each (Lambda: 0.25 of 0.61 ms).  VERDICT r4 #3 took that for launch latency; measured (round 5,
// -DFRONT_PROFILE, tools/front_dbg.py: time stamps around every stage and barrier of this kernel, Lambda): the grid barriers cost
// 1.2-2.7 us each, the STAGES cost what they cost as kernels — ORF count 22 us, emit 14, statistics + coverage 21, score 18, node order
// 11, edge count 11, edge scan 17, edge fill 29: 185 us in all — because each is a chain of dependent loads through one contig's
// records, not a launch.  One launch instead of twenty saves 7-12 us of a lone contig's run (Lambda 0.607 -> 0.600 ms, phiX174 0.278 ->
// 0.266) and loses beyond a few contigs (8 x 50 kb: 0.731 -> 0.743; 64 x 50 kb: 0.78 -> 1.14 ms: the grid is bounded by what must be
// resident at once).  It is therefore used for batches of up to FRONT_MAX_CONTIGS = 4 contigs and (round 5, later: the staged kernels of a few long
// contigs got four times as many workgroups per contig) 40 kb in all only.  For those the same stage bodies (b_orf, b_orf_stats, b_node_*, b_edges, ... : the code the staged kernels run,
// phx_orf.inc / phx_graph.inc / phx_layout.inc) are called from ONE kernel of n_contig x Y workgroups, separated by grid barriers
// (a counter in DTotals; release / acquire fences at agent scope around it: the XCDs' L2s are not coherent with each other).
// Every workgroup must be resident for a grid barrier to complete: the grid is small (<= FRONT_MAX_BLOCKS workgroups, a third of what
// the device holds), and a workgroup that waits longer than ~4 ms — other contexts or processes held the CUs — raises
// DTotals.front_abort: every workgroup leaves, the host runs the batch again with the staged kernels and stops using this kernel on
// the context (the same safety net as the planner / solver hand-shake, DESIGN.md §4).
#define FRONT_MAX_CONTIGS 4
#define FRONT_MAX_BLOCKS 64
#ifndef FRONT_SPINS
#define FRONT_SPINS 8000
#endif

__device__ __forceinline__ bool front_sync(DTotals *tot, const uint32_t nblocks, uint32_t &target, const int max_spins) {
    __shared__ int s_abort;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // this thread's stores of the stage are visible to the other XCDs
    __syncthreads();
    target += nblocks;
    if (threadIdx.x == 0) {
        atomicAdd(&tot->gsync, 1u);
        int ab = 0;
        for (uint32_t spins = 0; __hip_atomic_load(&tot->gsync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; spins++) {
            if (__hip_atomic_load(&tot->front_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ab = 1; break; }
            if ((int)spins > max_spins) { atomicExch(&tot->front_abort, 1); ab = 1; break; }
            __builtin_amdgcn_s_sleep(16);
        }
        s_abort = ab;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); // nothing this wavefront reads from here on comes from a stale line
    return s_abort != 0;
}

__global__ __launch_bounds__(NT, EDGE_WPS) void k_front(DBatch b) {
    const int bx = blockIdx.x, by = blockIdx.y, gy = gridDim.y;
    const uint32_t nblocks = gridDim.x * gridDim.y;
    uint32_t target = 0;
    DTotals *tot = b.tot;
#ifdef FRONT_PROFILE
    int stamp_k = 0;
#define FRONT_STAMP() do { if (bx == 0 && by == 0 && threadIdx.x == 0) b.lpart[16 + stamp_k] = (int64_t)wall_clock64(); stamp_k++; } while (0)
#else
#define FRONT_STAMP() do { } while (0)
#endif
    FRONT_STAMP();
#define FRONT_SYNC() do { FRONT_STAMP(); if (front_sync(tot, nblocks, target, b.front_spins)) return; FRONT_STAMP(); } while (0)
    // ---- ORF count (one workgroup per contig) beside the prefix popcounts (a wavefront per plane: k_bit_prefix) ----
    if (by == 0) b_orf<false, NT>(b, bx, 0, 1);
    if (gy == 1 || by >= 1) {
        const int wv = (int)threadIdx.x >> 6, nwv = NT / 64;
        const int first = gy == 1 ? 0 : (by - 1) * nwv, step = gy == 1 ? nwv : (gy - 1) * nwv;
        for (int plane = first + wv; plane < 7; plane += step) b_bit_prefix(b, bx, plane, (int)threadIdx.x & 63);
    }
    FRONT_SYNC();
    if (bx == 0 && by == 0) { // ORF / group / node offsets: the two-pass layout of large batches, both passes by this one workgroup
        b_layout1_a(b, 0, 1);
        __threadfence_block();
        __syncthreads();
        b_layout1_b(b, 0, 1);
    }
    FRONT_SYNC();
    b_orf<true, NT>(b, bx, by, gy);
    FRONT_SYNC();
    b_orf_stats(b, bx, by, gy);
    b_node_cov(b, bx, by, gy);
    FRONT_SYNC();
    if (by == 0) b_node_rank(b, bx);
    if (by == (gy > 1 ? 1 : 0)) b_score(b, bx);
    if (by == gy - 1) b_gap_table(b, bx, NT);
    FRONT_SYNC();
    b_node_build(b, bx, by, gy);
    FRONT_SYNC();
    if (by == 0) b_node_order(b, bx);
    FRONT_SYNC();
    b_node_attr(b, bx, by, gy);
    b_node_oterm(b, bx, by, gy); // (the same thread per node: no barrier between them; b_orf_stats ran stages ago)
    FRONT_SYNC();
    b_edges<false, false>(b, bx, by, gy);
    FRONT_SYNC();
    if (by == 0) b_edges_scan<NT>(b, bx);
    FRONT_SYNC();
    if (bx == 0 && by == 0) {
        b_layout2_a(b, 0, 1);
        __threadfence_block();
        __syncthreads();
        b_layout2_b(b, 0, 1);
    }
    FRONT_SYNC();
    b_edges<true, false, true>(b, bx, by, gy);
    FRONT_STAMP();
#undef FRONT_SYNC
}
