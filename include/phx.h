/* phx.h — C-ABI of libphx, the MI355X-native drop-in for PHANOTATE's per-contig hot path.
 *
 * What it replaces in the reference (all paths under /root/reference):
 *   phanotate.py:45      orfs  = functions.get_orfs(locus)        functions.py:143-303
 *   phanotate.py:49      graph = functions.get_graph(orfs)        functions.py:307-454
 *   phanotate.py:56-64   fz.empty_graph / fz.add_edge / fz.get_path   (external `fastpathz`)
 *   phanotate.py:65-76   path -> (start, stop, strand, score) features   locus.py:29-37
 * The reference has no FFI of its own for this path (it is pure Python plus the fastpathz
 * CPython module); these entry points are what a ctypes binding in phanotate.py would call —
 * see INTEGRATION.md for the stub.
 *
 * Conventions: extern "C", plain pointers and sizes, no exceptions, no global state.  Every
 * function returns 0 (PHX_OK) or a negative PHX_E_*.  Per-contig problems (the inputs on which the
 * reference raises a Python exception) are reported in phx_result.status and never fail the batch.
 * There is NO CPU execution path in this library: without a usable HIP device phx_create fails with
 * PHX_E_NODEVICE.
 *
 * Threading: one phx_ctx per (host thread, device).  Calls on one ctx must not overlap.
 */
#ifndef PHX_H
#define PHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_VERSION 410 /* 0.2.0: phx_create_ex, phx_set_trnas, phx_tap_dist, host I/O; phx_globals and PHX_N_STAGES grew; 0.2.1: phx_run_async, phx_wait;
                         * 0.3.0: phx_certified, phx_globals.certified, PHX_S_BADTRNA, more PHX_CREATE_* flags;
                         * 0.4.0: phx_params.start_w_text (the struct grew), phx_params_from_flags, the exact re-solve moved below the ABI
                         *        (phx_download* deliver reference-exact genes; phx_certified reports 2), phx_dump_text, PHX_CREATE_NO_EXACT;
                         *        (0.4.0 also REMOVED phx_rbs_table — an ABI break for a C caller that bound it: the table was a test hook of the Python Decimal
                         *        replay, which moved to tests/decimal_replay.py and computes it itself);
                         * 0.4.1: phx_run_async puts the certificate kernels behind the run unless exactness is off; env PHX_FRONT_SPINS (tests);
                         *        (additions, version unchanged) phx_orf_margin, phx_margins_flat, phx_tap_dist_target, phx_margins_ms, phx_format_margins;
 *        (additions, version unchanged) phx_gene_drop, phx_drop_margins_flat, phx_drop_ms, phx_drop_stats, phx_format_drops;
 *        (additions, version unchanged) phx_gene_repl, phx_replacements_flat, phx_tap_replacement, phx_replacements_ms,
 *        phx_replacement_stats, phx_format_replacements;
 *        (additions, version unchanged) phx_reannotate_flat, phx_orf_offsets, phx_tap_repath, phx_reannotate_ms;
 *        (addition, version unchanged: the suite pins 410) phx_constrain_flat — probe for the symbol, not for a version;
 *        (addition, version unchanged) phx_evidence_flat — likewise;
 *        (addition, version unchanged) phx_curate_flat — likewise;
 *        (additions, version unchanged) phx_scenarios_flat, phx_scenarios_ms, phx_scenario_chunks, phx_tap_scenario_path — probe for the symbol;
 *        (addition, version unchanged) phx_pinned_scenarios_flat — probe for the symbol;
 *        (addition, version unchanged) phx_evidence_scenarios_flat — probe for the symbol;
 *        (additions, version unchanged) phx_remargins_flat, phx_remargins_ms, phx_tap_redist — probe for the symbol;
 *        (additions, version unchanged) phx_pinmargins_flat, phx_pinmargins_ms, phx_tap_pindist — probe for the symbol;
 *        (addition, version unchanged) phx_curate_scenarios_flat — probe for the symbol;
 *        (additions, version unchanged) phx_redrops_flat, phx_redrops_ms, phx_redrop_stats — probe for the symbol
 *        (additions, version unchanged) phx_rereplacements_flat, phx_tap_rereplacement, phx_rereplacements_ms, phx_rereplacement_stats — probe for the symbol
 *        (additions, version unchanged) phx_pindrops_flat, phx_pindrops_ms, phx_pindrop_stats — probe for the symbol
 *        (additions, version unchanged) phx_pinreplacements_flat, phx_tap_pinreplacement, phx_pinreplacements_ms, phx_pinreplacement_stats — probe for the symbol
 *        (additions, version unchanged) phx_profile_slot, phx_profile_flat, phx_profile_ms — probe for the symbol
 *        (additions, version unchanged) phx_reprofile_flat, phx_reprofile_ms — probe for the symbol
 *        (additions, version unchanged) phx_pinprofile_flat, phx_pinprofile_ms, phx_pinprofile_stats — probe for the symbol */
#define PHX_MAX_CODONS 16

/* library-level errors */
#define PHX_OK 0
#define PHX_E_ARG (-1)      /* bad argument */
#define PHX_E_NODEVICE (-10) /* no HIP device / device index out of range */
#define PHX_E_HIP (-11)      /* a HIP runtime call failed; see phx_last_error() */
#define PHX_E_NOMEM (-12)
#define PHX_E_STATE (-13) /* call sequence error (e.g. run before upload) */
#define PHX_E_PARAM (-14) /* codon tables must be 3 letters of acgt; 1..16 starts/stops; minlen >= 6 */
#define PHX_E_IO (-15)    /* a file could not be opened or read */

/* per-contig status (phx_result.status); the reference's behaviour in brackets */
#define PHX_S_OK 0
#define PHX_S_BADLETTER (-2) /* letter outside acgtnryswkmbvdh [KeyError, functions.py:20-24] */
#define PHX_S_TOOSHORT (-3)  /* L < 6 [UnboundLocalError/KeyError in GCframe.get, gc_frame_plot.py:53-69] */
#define PHX_S_BADTRNA (-4)   /* phx_set_trnas: a hit of this contig has an end outside 1..L (no node can be placed there) */
#define PHX_S_PARALLEL (-6)  /* a bridge edge duplicates a connect edge [ValueError, graphs.py:74] */
#define PHX_S_OVERFLOW (-7)  /* path sums exceed the widest integer kernel (1088 bit: an ORF weight beyond ~1e300) AND the contig was not solved on the host: phx_download* solve such a contig in the reference's own unbounded arithmetic (phx_certified then reports 2) unless the context was created with PHX_CREATE_NO_EXACT / NO_CERTIFY */
#define PHX_S_LONGORF (-8)   /* (no longer produced: until 0.3.0 an ORF of more than 65535 codons — 196 kb without an in-frame stop, a scaffold's N run —
                              * overflowed the 16-bit class counters; such ORFs are now counted in 32 bits, functions.py:286-298 has no limit) */
#define PHX_S_NEGCYCLE (-9)  /* relaxation did not converge in V rounds */
#define PHX_S_NOPATH 1       /* warning: target unreachable from source; 0 genes reported */

typedef struct phx_ctx phx_ctx;

/* Flags of the reference CLI that reach the path (file_handling.py:51-66, phanotate.py:42-44). */
typedef struct phx_params {
    int32_t minlen;                        /* -l/--minlen, default 90 */
    int32_t n_start;                       /* -s/--start_codons */
    char start[PHX_MAX_CODONS][4];         /* lower-case, NUL-terminated */
    double start_w[PHX_MAX_CODONS];        /* weight / max(weight), file_handling.py:58-62 */
    int32_t n_stop;                        /* -e/--stop_codons */
    char stop[PHX_MAX_CODONS][4];
    /* The weights as the user wrote them on -s (before the division by their maximum), e.g. "0.85", "0.10", "0.05": the reference
     * holds Decimal(text) / max (file_handling.py:58-62), 28 digits that a double cannot carry, and the exactness guarantee of
     * phx_download* / phx_certified is stated against THAT value.  An entry left empty means "the shortest decimal that reads back as
     * start_w[i]" (what Decimal(repr(x)) would be).  phx_default_params and phx_params_from_flags fill both. */
    char start_w_text[PHX_MAX_CODONS][32];
} phx_params;

/* One called gene = one ORF edge on the shortest path (phanotate.py:71-76, locus.py:29-37).
 * left/right are 1-based inclusive coordinates, left < right on both strands; the tabular writer
 * (locus.py:39-56) prints left,right for '+' and right,left for '-'. */
typedef struct phx_gene {
    int32_t left;
    int32_t right;
    int32_t strand; /* +1 / -1 */
    int32_t frame;  /* reference Node.frame of the left node: +-1..3 for a CDS, +-4 for a tRNA (left.gene == 'tRNA', phanotate.py:75;
                     * Locus.tabular prints CDS features only, locus.py:42) */
    double score;   /* ORF edge weight, what the reference prints with '%E' */
} phx_gene;

typedef struct phx_result {
    int32_t status;  /* PHX_S_* */
    int32_t n_genes;
    phx_gene *genes; /* library-owned; in path order (ascending right coordinate), as phanotate.py:71-76 adds them */
} phx_result;

/* ---- stage-tap records (parity tests; layout is part of the ABI) ---- */
typedef struct phx_orf {
    int32_t start; /* Orf.start (1-based; fwd: first base of the start codon, rev: leftmost base of its reverse complement) */
    int32_t stop;  /* Orf.stop  (dict key: fwd first base of the stop codon, rev leftmost base of the rc stop codon / 1,2,3) */
    int32_t frame; /* +-1..3 */
    int32_t length;
    int32_t rbs;      /* score_rbs bin 0..27 */
    int32_t startidx; /* index into params.start of Orf.start_codon(), or -1 */
    int32_t group;    /* stop-group rank in reference insertion order */
    int32_t hist[9];  /* GC-frame class counts, (max_idx-1)*3 + (min_idx-1) */
    double pstop;
    double weight_rbs;
    double S; /* sum over sense codons of pos_max[max_idx]*pos_min[min_idx] */
    double weight;
} phx_orf;

typedef struct phx_node {
    int32_t pos;
    int8_t type;  /* 0 start, 1 stop, 2 source, 3 target */
    int8_t frame; /* +-1..3 CDS, +-4 tRNA (Node.gene == 'tRNA', functions.py:500-505), 0 for source/target */
    int16_t pad;
    int32_t other; /* Orfs.other_end[pos] (tRNA nodes: other_end['t' + str(pos)]) as seen by get_graph (functions.py:363-371); -1 for source/target */
    int32_t refidx; /* rank of this node in the reference's Graph.iternodes() order */
    double o;      /* the o1/o2 term of functions.py:373-384 for this position */
} phx_node;

typedef struct phx_edge { /* in-edge list order of the device graph: grouped by dst */
    int32_t src, dst;     /* device node ids (position-sorted; source = V-2, target = V-1) */
    double w;             /* Decimal weight of the reference, in fp64 (the solver adds trunc(w * 1000), edges.py:22: the device keeps
                           * that integer, the tap recomputes w and checks the two against each other) */
    int32_t inexact;      /* 1: the reference's integer W* = trunc(Decimal(w) * 1000) is not known to equal the solver's W = trunc(w * 1000).
                           * Before the certificate has been asked for (phx_certified / phx_download* / phx_tap_globals): the verdict of the fp64
                           * pipeline; after it: of the double-double evaluation (csrc/phx_refine.inc), which clears most flags and leaves, for the rest, */
    int32_t pad;
    double d1, d2, err;   /* W* in [W + D - eps, W + D + eps], D = d1 + d2 (both integer-valued), eps = 0 if err == 0 else floor(err) + 1 (err = inf: unknown) */
} phx_edge;

typedef struct phx_globals {
    int64_t L;
    double pstop;               /* functions.py:178, also pgap (functions.py:309) */
    double background_rbs[28];  /* functions.py:180-181, normalised */
    double training_rbs[28];    /* functions.py:254-255, normalised */
    double pos_max[4], pos_min[4]; /* functions.py:281-284 */
    int32_t n_orf, n_group, n_node, n_edge, n_bridge;
    int32_t n_limbs;     /* 64-bit limbs of the integer kernel that solved this batch */
    int32_t sssp_sweeps; /* outer sweeps of the device relaxation */
    int32_t sssp_iters;  /* relaxation rounds summed over all windows and sweeps */
    int32_t status;
    int32_t sssp_kernel; /* which kernel solved it: 0 global memory, 1 workgroup per contig, 2 wavefront per contig, 3 the same in its roomy configuration */
    int32_t sssp_handed_back; /* != 0: the wavefront kernel passed the contig on: 1 a node's 500 bp neighbourhood exceeds a window,
                               * 2 spill list full, 3 no convergence, 4 too many step-backs, 5 its planner made no progress for 20 ms
                               * (small batches run the two side by side; never seen outside test builds) */
    int32_t tie; /* equal-length alternatives to the shortest path (the reference's relaxation order decides, see phx_inorder.inc):
                  * 0 none, 1 they exist and the solver's path already was the reference's, 2 the path was replaced by the reference's */
    int32_t certified; /* phx_certified's verdict for this contig (1 / 0 / -1) */
    /* the integer counters behind the fp64 globals above (what a Decimal restatement of the reference starts from, see
     * tests/decimal_replay.py): RBS bin counts without the pseudo-count (functions.py:155-156,168-169,211), GC-frame training
     * counts (functions.py:261-279, index 1..3), g+c over the contig after the counting remap of functions.py:159-163 */
    uint32_t rbs_background_count[28], rbs_training_count[28];
    uint32_t gc_max_count[4], gc_min_count[4];
    int64_t gc_count;
} phx_globals;

/* ---- library ---- */
int phx_version(void);
int phx_device_count(void);
const char *phx_strerror(int code);
/* Text of the last failing HIP call on this ctx (or on the last failed phx_create when ctx==NULL). */
const char *phx_last_error(const phx_ctx *ctx);

/* Fills *p with the reference defaults: atg:0.85,gtg:0.10,ttg:0.05 / tag,tga,taa / minlen 90. */
void phx_default_params(phx_params *p);
/* The same from the reference's flags (file_handling.py:51-66): start_codons "atg:0.85,gtg:0.10,ttg:0.05" (codon:weight pairs; a
 * repeated codon keeps its first place and its last weight, like the dict the reference builds), stop_codons "tag,tga,taa", minlen.
 * NULL strings mean the defaults.  Codons are lower-cased; PHX_E_PARAM on anything that is not 3 letters of acgt / a decimal number. */
int phx_params_from_flags(const char *start_codons, const char *stop_codons, int32_t minlen, phx_params *p);

/* device: HIP ordinal.  stream: a hipStream_t the caller owns, or NULL to let the ctx create its own (non-blocking: it
 * does NOT synchronise with HIP's null stream).  All kernels and copies of this ctx are issued on it. */
int phx_create(const phx_params *params, int device, void *stream, phx_ctx **out);
/* The same with flags.  PHX_CREATE_USE_STREAM: `stream` is used exactly as given, and a NULL handle then means HIP's null
 * (legacy default) stream — which is what torch.cuda.current_stream().cuda_stream is unless the caller switched streams —
 * so that work of this ctx is ordered after whatever the caller enqueued there before (e.g. the kernels that produce a
 * buffer handed to phx_attach).  On the null stream the run is enqueued kernel by kernel (HIP cannot capture it into a graph). */
#define PHX_CREATE_USE_STREAM 1u
/* Development / test switches (results are the same with any of them): enqueue every run kernel by kernel instead of replaying a
 * captured HIP graph; size the buffers between kernels on every run (two host round trips) instead of only on the first; solve every
 * contig with the global-memory shortest-path kernel; keep contigs off the wavefront-per-contig kernel. */
#define PHX_CREATE_NO_GRAPH 2u
#define PHX_CREATE_SIZE_EVERY_RUN 4u
#define PHX_CREATE_SOLVER_GLOBAL 8u
#define PHX_CREATE_SOLVER_NO_WAVE 16u
/* NO_CERTIFY: phx_certified reports -1 (and the kernel's scratch, 20 + 32 bytes per node, is not allocated).  It also turns the
 * exactness machinery off as a whole — without a certificate nothing says which contigs would need the host re-solve —: the gene lists
 * of phx_download* are then the fp64-derived integers' shortest paths, WITHOUT the guarantee that they are the reference's.
 * CERT_TIGHT multiplies its error bounds by 2^36, so that ordinary inputs come out uncertified (tests of the host re-solve). */
#define PHX_CREATE_NO_CERTIFY 32u
#define PHX_CREATE_CERT_TIGHT 64u
#define PHX_CREATE_POISON 256u    /* every device buffer the context allocates is filled with the byte 0xA5 first: the library must not depend on fresh memory being zero */
#define PHX_CREATE_ONE_STREAM 512u /* no side streams: every kernel of a run on the context's one stream, in program order */
#define PHX_CREATE_CERT_WIDE 128u /* every contig through the certificate's general kernel (otherwise only contigs of more than 12288 nodes) */
#define PHX_CREATE_NO_DUO 4096u /* 128-bit contigs are solved by k_sssp_wave<2> (one wavefront per contig) instead of k_sssp_duo (a feeder and a solver wavefront per contig) */
#define PHX_CREATE_NO_SEG 8192u /* small batches solve every contig by one sweep (one wavefront pair), not by up to 16 segments side by side that k_seg_merge joins and proves (phx_sssp_seg.inc) */
#define PHX_CREATE_NO_CHAIN 16384u /* nodes, node attributes, edge count and scan of a contig as four staged launches, not as the one launch with a workgroup per contig (k_graph_chain); env PHX_NO_CHAIN=1 does the same */
#define PHX_CREATE_NO_FUSE 2048u /* batches of up to 4 contigs and 40 kb in all run their front end (ORF count ... edge fill) as the staged kernels of large batches, not as the one fused launch (k_front) */
#define PHX_CREATE_NO_EXACT 1024u /* phx_download* hand out the device's gene lists as they are: no certificate is asked for and no contig is solved again on the host */
int phx_create_ex(const phx_params *params, int device, void *stream, uint32_t flags, phx_ctx **out);
void phx_destroy(phx_ctx *ctx);

/* ---- the whole path, batched (replaces phanotate.py:40-76 for n contigs) ---- */
/* seq[i]: ASCII, any case, len[i] characters, not NUL-terminated; borrowed for the call. */
int phx_annotate(phx_ctx *ctx, int32_t n, const char *const *seq, const int64_t *len, phx_result *out /* [n] */);
void phx_free_results(phx_result *res, int32_t n);

/* The same in three steps, so a caller can keep inputs resident in HBM and time phx_run alone. */
/* phx_upload: the letters are packed on the host — worker threads, into pinned memory — into the form the kernels read (residue-split
 * bit planes, 3 bits per base: DESIGN.md §3) and copied piece by piece; it returns when the caller's strings are free again, the copies
 * are ordered before the run on the context's stream. */
int phx_upload(phx_ctx *ctx, int32_t n, const char *const *seq, const int64_t *len);
/* Alternative to phx_upload: the concatenated ASCII is already in device memory (offsets on host, n+1 entries); a kernel at the head
 * of every run packs it (the caller's buffer is only read, and must stay valid until the runs on it have ended). */
int phx_attach(phx_ctx *ctx, int32_t n, const void *d_ascii, const int64_t *offsets);
/* tRNA masking (functions.add_trnas, functions.py:457-509): the hits of an external tRNA finder for the contigs of the batch just
 * uploaded / attached, as the reference holds them in `trnas`: hits of contig i are (start[k], stop[k]) for k in
 * [offsets[i], offsets[i+1]); start < stop for a hit on the forward strand, start > stop (the pair reversed) for a complement hit;
 * 1-based, inside the contig (a contig with a hit outside 1..L gets status PHX_S_BADTRNA; the batch goes on).  The device then adds the tRNA nodes (frame +-4), their edges of weight -20 and the connect rules
 * of functions.py:388-399.  Call after phx_upload / phx_attach and before phx_run; a new upload forgets the hits.  Not calling
 * it (or offsets == NULL) is "no tRNA finder installed" (functions.py:493-495).  Running the finders is the caller's business
 * (phanotate_amd/trna.py does what functions.py:457-491 does). */
int phx_set_trnas(phx_ctx *ctx, const int64_t *offsets /* [n+1] */, const int32_t *start, const int32_t *stop);
int phx_run(phx_ctx *ctx);                        /* every kernel of the path; blocks until results are in HBM */
/* The same in two halves, for keeping two batches in flight on one GPU (two contexts on their own streams: while the latency-bound
 * shortest-path kernel of one batch runs, the other context's upload and throughput kernels fill the device; on the benchmark
 * batch two contexts alternating take 1.8 ms per batch instead of 2.3).  phx_run_async enqueues the run and returns; phx_wait
 * blocks until the results are in HBM and does what a run that did not fit needs (buffers grown, run repeated).  The first run
 * of a context is synchronous (it sizes the buffers between kernels).  Every other entry point on a context with a run in flight
 * waits for it first, so the pair is an optimisation, never a requirement.  phx_wait without a run: PHX_OK if results are there.
 * Unless exactness is off (PHX_CREATE_NO_EXACT / NO_CERTIFY, phx_set_exact(ctx, 0)) phx_run_async also enqueues the certificate kernels
 * (k_refine, k_certify) behind the run on the context's stream: the download that follows finds the certificate done instead of waiting
 * for it, and with two batches in flight it runs beside the other context's kernels (a stream of batches host to host: 2.6 -> 2.0 ms
 * per 1000 x 50 kb).  phx_run never does: the certificate stays on demand there (phx_certified / phx_download*). */
int phx_run_async(phx_ctx *ctx);
int phx_wait(phx_ctx *ctx);
/* Both download calls deliver gene lists that are the reference's: they ask for the certificate (phx_certified) and a contig the
 * device could not certify is solved again on the host, inside this call, on the reference's own Decimal-derived integers
 * (csrc/phx_exact.inc; worker threads, one contig each) — expected for none of a batch's contigs, see phx_certified.  A context
 * created with PHX_CREATE_NO_CERTIFY or PHX_CREATE_NO_EXACT skips both and hands out the device's lists. */
int phx_download(phx_ctx *ctx, phx_result *out);  /* D2H of the gene lists, [n] */
/* The same into caller-owned flat arrays (what a language binding wants: no per-contig allocation): genes of contig i are
 * genes[offsets[i] .. offsets[i+1]), in path order; status[i] as phx_result.status.  offsets has n+1 entries.  With
 * genes == NULL only offsets, status and total are filled (size query); cap = number of phx_gene records genes can take. */
int phx_download_flat(phx_ctx *ctx, phx_gene *genes, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);

/* ---- one process, several GPUs (contigs never interact, phanotate.py:40,56) ----
 * A pool = one host thread and two contexts per listed device (an ordinal may repeat).  phx_pool_annotate cuts the n contigs into
 * consecutive batches of at most batch_bases bases (<= 0: 4e8; with several devices at least two batches per device), sends batch k
 * to device k mod n_dev with two batches in flight per device (phx_run_async), and fills out[0..n) in input order exactly as
 * phx_annotate would (the reference's genes, see phx_download).  No process group, no collective.  trna_*: as phx_set_trnas for the
 * whole input (offsets has n + 1 entries), or NULL.  On an error every result is freed and the first error code is returned.
 * flags: PHX_CREATE_* without USE_STREAM. */
typedef struct phx_pool phx_pool;
int phx_pool_create(const phx_params *params, int32_t n_dev, const int32_t *devices, uint32_t flags, phx_pool **out);
void phx_pool_destroy(phx_pool *pool);
const char *phx_pool_last_error(const phx_pool *pool);
int phx_pool_annotate(phx_pool *pool, int32_t n, const char *const *seq, const int64_t *len, int64_t batch_bases,
                      const int64_t *trna_offsets, const int32_t *trna_start, const int32_t *trna_stop, phx_result *out /* [n] */);

/* Is every gene list what the REFERENCE'S integers give?  The reference solves on trunc(Decimal(w) * 1000) with 28 digits
 * (edges.py:17-23); the device derives its integers in fp64 and, where fp64 cannot decide the truncation, in double-double, and
 * flags the edges whose integer it still cannot prove equal to the reference's (the error bound of the Decimal chain
 * itself).  After the solve it proves, per contig and in exact integer arithmetic, that no difference inside those bounds can change
 * the path (an optimality certificate, csrc/phx_certify.inc).  cert[i] =
 *   1: proven on the device (also for contigs with an error status or without a path);
 *   2: not proven on the device, so the contig was solved again on the host on the reference's own integers (the Decimal chain
 *      replayed by csrc/phx_dec.c + phx_exact.inc) and phx_download* deliver THAT result;
 *   0: not proven and not solved again (context created with PHX_CREATE_NO_EXACT, or the replay met an operation it does not restate:
 *      never on the reference's inputs) — the genes are the exact solution for the device's integers;
 *  -1: the context was created with PHX_CREATE_NO_CERTIFY.
 * The proof is computed when it is first asked for after a run (here, by phx_download*, or by phx_tap_globals), from the state the
 * run left on the device — ~0.2 ms for a thousand 50 kb contigs; phx_run itself does not pay for it. */
int phx_certified(phx_ctx *ctx, int8_t *cert /* [n] */);
/* on = 0: phx_download* / phx_certified stop short of the host re-solve (as PHX_CREATE_NO_EXACT) and hand out the device's lists
 * for every contig, also for those already solved again; on = 1 (the default) switches it back.  For tests and measurements. */
int phx_set_exact(phx_ctx *ctx, int on);

/* ---- stage taps on the batch last processed by phx_run (parity tests) ---- */
int phx_tap_globals(phx_ctx *ctx, int32_t contig, phx_globals *out);
/* per 0-based position, each array L bytes (any may be NULL):
 *   cls  bits0-2 codon class at p (0 none,1 fwd start,2 rev start,3 fwd stop,4 rev stop; elif order of functions.py:198-215)
 *   gcc  low nibble fwd (max_idx-1)*3+(min_idx-1) of gc_pos_freq[p+1], high nibble the reversed triple
 *   binF/binR  score_rbs of dna[p-20:p+1] / rev_comp(dna[p:p+21]) */
int phx_tap_positions(phx_ctx *ctx, int32_t contig, uint8_t *cls, uint8_t *gcc, uint8_t *binF, uint8_t *binR);
int phx_tap_orfs(phx_ctx *ctx, int32_t contig, phx_orf *out /* [n_orf], reference iter_orfs order */);
int phx_tap_nodes(phx_ctx *ctx, int32_t contig, phx_node *out /* [n_node], device order */);
int phx_tap_edges(phx_ctx *ctx, int32_t contig, phx_edge *out /* [n_edge] */);
/* path as device node ids, source first; dist_limbs receives n_limbs 64-bit words (two's complement) */
int phx_tap_path(phx_ctx *ctx, int32_t contig, int32_t *path, int32_t cap, int32_t *n_path, uint64_t *dist_limbs, int32_t cap_limbs);
/* exact distance of every node from the source: n_node x n_limbs 64-bit words (two's complement, device node order);
 * an unreached node has a top word >= 2^61 */
int phx_tap_dist(phx_ctx *ctx, int32_t contig, uint64_t *dist_limbs, int64_t cap_words);

/* ---- per-ORF path margins, on demand after a run ----
 * For one contig, with W(e) the solver's integer trunc(fp64 w * 1000) of edge e (the integers phx_tap_dist is exact for):
 *   d_s(v)  the shortest source -> v distance (phx_tap_dist);
 *   d_t(v)  the shortest v -> target distance, exact, in the contig's limb class; "unreached" when no path leads from v to the target;
 *   D       = d_s(target) = d_t(source).
 * An ORF's edge e = (u -> v) runs start -> stop on the forward strand and stop -> start on the reverse strand (functions.py:310-316).
 *   Delta(e) = d_s(u) + W(e) + d_t(v) - D, an integer >= 0 (no cycle of negative length): how much longer the best source -> target path
 *   becomes when it is forced through the ORF.  margin = float(Delta) / 1000.0 exactly as Python computes it (the integer correctly rounded
 *   to a double, then one correctly rounded division), in the units of SCORE.  d_s(u) or d_t(v) unreached: no path runs through the ORF,
 *   through = 0 and margin = +inf.
 * These are margins over the device's integers W, not over the reference's trunc(Decimal(w) * 1000): on a contig the certificate proves
 * (phx_certified 1) every called ORF has margin 0 exactly; on one solved again on the host (phx_certified 2) a called ORF may carry a small
 * positive margin, bounded by the |D| + eps bounds phx_tap_edges reports over the edges of the device's and the delivered path. */
typedef struct phx_orf_margin {
    int32_t left, right, strand, frame; /* as phx_gene (right includes the stop codon) */
    double score;                       /* the ORF's edge weight, as phx_gene.score */
    double margin;                      /* float(Delta)/1000, >= 0; +inf when through == 0 */
    int32_t called;                     /* 1: one of the genes phx_download* delivers for this contig */
    int32_t through;                    /* 1: some source->target path runs through this ORF */
} phx_orf_margin;
/* Margins of every CDS ORF of the batch last run, flat like phx_download_flat (rec == NULL: size query): the records of contig i are
 * rec[offsets[i] .. offsets[i+1]), in phx_tap_orfs order (the reference's iter_orfs order), so that a caller can zip the two.  status[i]:
 * the contig's run status when it is an error (< 0, no records; PHX_S_NEGCYCLE among them); PHX_S_OVERFLOW (no records) for a contig
 * without device distances (path sums beyond 1088 bits, solved on the host); PHX_S_NEGCYCLE (no records) when the reverse pass meets a
 * cycle of negative length the forward one could not reach; else the run status (0, or PHX_S_NOPATH: records with through = 0).
 * The first call after a run computes them (out-edge CSR, a reverse shortest-path pass in the contig's wide integers, one thread per ORF:
 * kernel by kernel on the context's stream, never inside phx_run; buffers allocated at the first call of a context); later calls reuse
 * them.  Like every entry point it waits for a run in flight; a new upload invalidates the results. */
int phx_margins_flat(phx_ctx *ctx, phx_orf_margin *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* exact distance of every node TO the target: n_node x sssp_nl words, like phx_tap_dist (an unreached node has a top word >= 2^61) */
int phx_tap_dist_target(phx_ctx *ctx, int32_t contig, uint64_t *dist_limbs, int64_t cap_words);
/* device time of the last computation of the margins (HIP events on the context's stream), ms[4]: out-edge CSR, reverse pass, records,
 * the copy of the records to the host.  All 0 before the first. */
int phx_margins_ms(phx_ctx *ctx, float *ms /* [4] */);

/* ---- gene drop margins, on demand after a run ----
 * For one contig, with W, d_s, d_t and D as for the margins and P = p_0 (source) ... p_K (target) the device's shortest path (phx_tap_path):
 * a called gene is a CDS ORF edge of P; its stop node is p_{j+1} of a forward gene (start p_j -> stop p_{j+1}) and p_j of a reverse gene
 * (stop p_j -> start p_{j+1}).  D_{-g} is the shortest source -> target distance in the graph without that stop node: no ORF that ends at
 * this stop is called, at any start.  drop = float(D_{-g} - D) / 1000.0 exactly as Python computes it, >= 0 (0: an equal-length path
 * without the gene exists); bypass = 0 and drop = +inf when no path avoids the stop node. */
typedef struct phx_gene_drop {
    int32_t left, right, strand, frame; /* as phx_gene (right includes the stop codon) */
    double score;                       /* the gene's edge weight, as phx_gene.score */
    double drop;                        /* float(D_{-g} - D)/1000, >= 0; +inf when bypass == 0 */
    int32_t called;                     /* 1: one of the genes phx_download* delivers for this contig (on a phx_certified 2 contig the
                                         *    delivered genes may differ from the device path) */
    int32_t bypass;                     /* 1: some source->target path avoids the stop node */
} phx_gene_drop;
/* Drop margins of every CDS gene of the device path of every contig of the batch last run, flat like phx_margins_flat (rec == NULL: size
 * query): the records of contig i are rec[offsets[i] .. offsets[i+1]), in path order (left to right).  status[i] as phx_margins_flat:
 * a run error (< 0), PHX_S_OVERFLOW (sssp_mode 4), PHX_S_NEGCYCLE from the reverse pass, all without records; PHX_S_NOPATH without
 * records; else 0.  The first call after a run computes them (the margins' out-edge CSR and reverse pass when they are not there yet, then
 * trees, labels, candidates and fixups: kernel by kernel on the context's stream, never inside phx_run); later calls reuse them.  The
 * margins of phx_margins_flat are the same whichever of the two calls comes first. */
int phx_drop_margins_flat(phx_ctx *ctx, phx_gene_drop *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the drop margins (HIP events), ms[4]: trees + labels, candidates + sparse table, fixups (saturated
 * slots, cross nodes, records), the copy of the records to the host.  All 0 before the first. */
int phx_drop_ms(phx_ctx *ctx, float *ms /* [4] */);
/* counters of the last computation, out[4]: gene slots, slots with cross nodes (step 4 of DESIGN.md §12), saturated slots rescanned
 * exactly, contigs whose trees were built layer by layer (a zero-length cycle of tight edges, or env PHX_DROP_LAYERED=1) */
int phx_drop_stats(phx_ctx *ctx, int64_t *out /* [4] */);

/* ---- coding profiles, on demand after a run ----
 * What each stretch of a contig costs as part of a forward gene, of a reverse gene, or between genes.  With W, d_s, d_t and D as for the
 * margins, EVERY edge e = (u -> v) of the device graph — ORF edge, tRNA edge or connector (gap, overlap, bridge, source and target edges) —
 * has Delta(e) = d_s(u) + W(e) + d_t(v) - D >= 0 and mu(e) = float(Delta(e)) / 1000.0 as phx_margins_flat rounds it (+inf when d_s(u) or
 * d_t(v) is unreached).  As for the margins, Delta is the length of the best source -> target WALK forced through e, over D: the graph has
 * backward (overlap) edges, so the forced walk may meet a node twice.
 *   Slots.  A contig with V nodes (phx_tap_nodes order: the real nodes 0 .. m-1 position-sorted, m = V - 2, then source and target) has
 *   m + 1 = V - 1 slots: slot 0 left of node 0, slot s between node s-1 and node s, slot m right of node m-1.  With rank(v) = v for a real
 *   node, rank(source) = -1 and rank(target) = m, an edge with rank(u) < rank(v) covers the slots rank(u)+1 .. rank(v); any other edge
 *   (overlap connectors, equal ranks) covers nothing.  Every source -> target path crosses every slot by at least one covering edge.
 *   Tracks.  An edge whose tail is an open node (forward start or reverse stop; tRNA nodes alike) is a gene edge, of the strand of its
 *   tail's frame; every other edge is a connector.  fwd / rev / gap of a slot: the minimum mu over the forward gene edges / reverse gene
 *   edges / connectors that cover it, +inf where none does — how much worse the best annotation becomes when the stretch must lie inside a
 *   forward gene / inside a reverse gene / between genes.  On a contig with status 0 the device path crosses every slot: min(fwd, rev,
 *   gap) = 0.  The minimum of mu equals mu of the exact minimum Delta (rounding and division are monotone).
 * lo / hi are NODE positions (phx_tap_nodes pos), not gene coordinates: a forward gene's record in phx_download* has right = its stop
 * node's pos + 2 (right includes the stop codon), so a gene [left, right] covers the slots with left <= lo and hi <= right - 2.  lo == hi
 * happens (both strands at one position, tRNA nodes); such a slot is still a record.
 * As the margins, the profile is over the device's integers W and the device path, also on a phx_certified 2 contig. */
typedef struct phx_profile_slot {
    int32_t lo, hi;       /* phx_tap_nodes pos of the bounding nodes; slot 0: lo = 0 (the source's pos); last slot: hi = L + 1 (the target's) */
    double fwd, rev, gap; /* >= 0, +inf: nothing of that kind covers the slot */
} phx_profile_slot;
/* Profiles of every contig of the batch last run, flat like phx_margins_flat (rec == NULL: size query): the n_node - 1 records of contig i
 * are rec[offsets[i] .. offsets[i+1]), slot 0 first.  status[i] as phx_margins_flat: a run error (< 0), PHX_S_OVERFLOW (no device
 * distances) and PHX_S_NEGCYCLE from the reverse pass without records; a contig without a graph (n_node <= 2): the run's status, no
 * records; PHX_S_NOPATH: V - 1 records with all three values +inf; else 0.  The first call after a run computes them (the margins'
 * out-edge CSR and reverse pass when they are not there yet, then one sparse table per contig and track: kernel by kernel on the context's
 * stream, never inside phx_run; buffers allocated at the first call of a context); later calls reuse them, a new upload or run invalidates
 * them.  phx_margins_flat, phx_drop_margins_flat and their timings are the same whichever call comes first. */
int phx_profile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the profiles (HIP events), ms[3]: candidates + tables with their push-down (one launch per limb
 * class: a table lives in LDS where it fits), the slots' bounds (records), the copy of the records to the host.  All 0 before the first. */
int phx_profile_ms(phx_ctx *ctx, float *ms /* [3] */);

/* ---- drop replacements, on demand after a run ----
 * For every record of phx_drop_margins_flat with bypass = 1 a replacement path R_g: a simple source -> target path of the device graph
 * that avoids the gene's stop node p_j and whose integer length is exactly D_{-g}.  It has the form p_0 .. p_a, r_1 .. r_m, p_b .. p_K
 * (a < j < b, no r_i on the device path P), so its genes (pairs R[2i+1] -> R[2i+2], the rule of phx_download) are P's genes with the
 * pairs of P between p_a and p_b ("removed", the dropped gene among them) replaced by the pairs of the detour p_a, r_1 .. r_m, p_b
 * ("added").  Among equal-length witnesses the rule of DESIGN.md §13 picks one, so the bytes do not depend on the batch or the flags. */
typedef struct phx_gene_repl {
    int32_t left, right, strand, frame; /* the dropped gene, as phx_gene_drop */
    double drop;                        /* bit-equal to phx_gene_drop.drop */
    int32_t called, bypass;             /* as phx_gene_drop */
    int32_t span_left, span_right;      /* min left / max right over the removed and added genes (bypass = 0: the gene's own) */
    int32_t n_removed, n_added;         /* genes[gene_off .. + n_removed): P's genes in the span, path order; then n_added genes of the
                                         * detour, path order (both 0 when bypass = 0) */
    int64_t gene_off;
} phx_gene_repl;
/* Replacements of every record of phx_drop_margins_flat, flat: records rec[offsets[i] .. offsets[i+1]) of contig i as the drop records
 * (same order, statuses, offsets, drop, called, bypass); their genes in genes[0 .. gene_total), at each record's gene_off.  rec == NULL
 * or genes == NULL: size query (offsets, status, total, gene_total).  The first call after a run computes them (the drop margins first
 * when they are not there yet), kernel by kernel on the context's stream, never inside phx_run; later calls reuse them. */
int phx_replacements_flat(phx_ctx *ctx, phx_gene_repl *rec, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets /* [n+1] */,
                          int32_t *status /* [n] */, int64_t *total, int64_t *gene_total);
/* R_g of record k of contig `contig` (k counts the contig's records of phx_replacements_flat): device node ids, source first.  path ==
 * NULL: *n_path only; bypass = 0: *n_path = 0. */
int phx_tap_replacement(phx_ctx *ctx, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path);
/* device time of the last computation of the replacements (HIP events around the kernels only), ms[3]: argmin (winners of every slot,
 * cross winners), walk + genes (counting pass, filling pass with its offsets' upload), the copy to the host.  All 0 before the first. */
int phx_replacements_ms(phx_ctx *ctx, float *ms /* [3] */);
/* counters of the last computation of the replacements, out[5]: slots won by a cross candidate (step 4 of DESIGN.md §12), delta-chain
 * nodes of those winners, cross winners whose path keeps its delta chain, walks whose zero-length loop was cut, 1 when the delta-chain
 * buffer had to grow (the cross winners were then computed a second time). */
int phx_replacement_stats(phx_ctx *ctx, int64_t *out /* [5] */);

/* ---- masked re-annotation, on demand after a run ----
 * The general operation the margins above are special cases of: take a set F of candidate ORFs out of the resident device graph G and
 * solve again.  G_F is G without the ORF edges of F (nodes, connectors, bridges and tRNA edges stay; an ORF without an edge in the graph
 * is ignored), D_F the shortest source -> target distance in G_F in the contig's own limb class, delta = float(D_F - D) / 1000.0 as the
 * margins round it (>= 0; +inf with PHX_S_NOPATH when G_F has no path).  The path is the one an in-place Bellman-Ford over
 * Graph.iteredges order restricted to G_F leaves (strict <): with F empty the device path byte for byte, ties included.  The genes are
 * that path's, in the record format and order of phx_download_flat with exactness off.  It is over the device's integers and the device
 * graph (no certificate, no host re-solve), and it is not a re-run of the front end: GC-frame training and connector edges are those of
 * the full ORF set.
 *   forbid       one byte per ORF of the batch (non-zero: refused), contig i's at orf_offsets[i] .. orf_offsets[i+1], in phx_tap_orfs order
 *   orf_offsets  [n+1]: must equal the cumulative ORF counts of the batch last run (the offsets phx_margins_flat reports), else PHX_E_ARG
 *                and no kernel has run
 *   flags        bit 0: solve every contig again, also one whose mask is empty (without it such a contig's result is copied from the run)
 *   genes        NULL: size query (offsets, status, delta, total are filled in)
 * status[i]: a run error (< 0) passes through without genes; PHX_S_OVERFLOW for a contig without device distances; PHX_S_NOPATH when the
 * run had no path or G_F has none (0 genes, delta +inf; delta is +inf for every contig without a result); PHX_S_NEGCYCLE when a sweep or
 * round cap ended the solve; else 0.  Neighbours are unaffected.  Buffers are allocated at the first call; the result is invalidated by
 * the next upload or run; nothing phx_download*, the taps, the margins, the drops, the replacements or the certificate return changes. */
int phx_reannotate_flat(phx_ctx *ctx, const uint8_t *forbid, const int64_t *orf_offsets /* [n+1] */, uint32_t flags, phx_gene *genes, int64_t cap,
                        int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, double *delta /* [n] */, int64_t *total);
/* ---- pinned re-annotation: the best annotation that KEEPS chosen ORFs ----
 * phx_reannotate_flat with a second set: F (forbid) is refused as above, R (require, disjoint from F) is to be kept.  R' = the ORFs of R whose
 * edge exists in G_F.  Paths of G_F are ordered by (-c(P), W(P)), c(P) = edges of R' on P, W(P) the sum of W: the result is the minimum,
 * i.e. the shortest path under W'(e) = W(e) - M [e in R'] for any M above every walk sum.  The device solves such a contig on one limb more
 * than its class with M = 2^(64 NL) — the top limb of a distance is the count, the limbs below the W-sum, both exact; 128 / 256 / 512 / 1088
 * bits become 192 / 320 / 576 / 1152, no class overflows — and picks the path by the in-order rule of §14 on W'.  With R empty it is
 * phx_reannotate_flat byte for byte (the same kernels).
 *   forbid, require  one byte per ORF each (non-zero: in the set), laid out as `forbid` above; either may be NULL (empty).  An ORF in both:
 *                    PHX_E_ARG before any kernel.
 *   delta[i]         float(W(P) - D) / 1000.0 (M does not enter), >= 0; +inf without a result
 *   unmet[i]         |R| - c(P): the required ORFs of contig i the result does not call — without an edge in the graph, on no source ->
 *                    target path, or not compatible with the rest of R (the genes are the best annotation that keeps as many as can be
 *                    kept together).  All of R where there is no result.
 * status[i] as above, and PHX_S_NEGCYCLE (no genes, delta +inf) when a cycle of G_F that the source reaches runs through an edge of R' (nodes are shared within
 * stop groups): no path is best then.  The solver ends such a contig as soon as a distance counts more required edges than exist.
 * The two calls share their buffers and their cached result (keyed on both sets and flags); phx_tap_repath and phx_reannotate_ms serve the
 * last solve of either kind, and the distance phx_tap_repath reports is the W-sum W(P). */
int phx_constrain_flat(phx_ctx *ctx, const uint8_t *forbid, const uint8_t *require, const int64_t *orf_offsets /* [n+1] */, uint32_t flags, phx_gene *genes,
                       int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, double *delta /* [n] */, int32_t *unmet /* [n] */, int64_t *total);
/* ---- evidence-weighted re-annotation: a bonus or a penalty per ORF ----
 * phx_reannotate_flat with soft evidence beside the refused set: B(k), a signed integer in the solver's units (1/1000 of a SCORE unit; 0: no
 * evidence, negative: support, positive: doubt), is added to the weight of ORF k's edge.  G_{F,B} is G_F with those weights, D_B its
 * shortest source -> target distance in the contig's own limb class, the path the in-order rule of §14 on the new integers, delta =
 * float(D_B - D) / 1000.0, which may be negative.  With every B zero it is phx_reannotate_flat byte for byte (the same kernels).
 *   bias         one int64 per ORF of the batch, laid out as `forbid`; NULL: all zero.  |B| > 2^52: PHX_E_ARG before any kernel
 *   forbid       as above; may be NULL (empty).  A refused ORF's bias is ignored
 *   flags, genes, orf_offsets and the state rules as phx_reannotate_flat
 * status[i] as there; PHX_S_NEGCYCLE (no genes, delta +inf) now also when bonuses make a cycle that the source reaches negative — no path is
 * best then, and the reference's in-place Bellman-Ford does not settle either; PHX_S_OVERFLOW (no genes, delta +inf) also when the layout's
 * bound plus the sum of |B| over the contig's biased edges no longer fits the contig's limb class (there is no promotion to a wider one).
 * The three calls share their buffers and their cached result (keyed on the sets, the bias and the flags); phx_tap_repath, whose distance
 * is then D_B, and phx_reannotate_ms serve the last solve of any kind.  (Addition, version unchanged: probe for the symbol.) */
int phx_evidence_flat(phx_ctx *ctx, const int64_t *bias, const uint8_t *forbid, const int64_t *orf_offsets /* [n+1] */, uint32_t flags, phx_gene *genes, int64_t cap,
                      int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, double *delta /* [n] */, int64_t *total);
/* ---- combined re-annotation: required, refused and biased ORFs in one solve ----
 * phx_constrain_flat on phx_evidence_flat's graph: among the paths of G_{F,B} those that use the most edges of the required set are
 * compared by S(P), the sum of W + B over the path — the shortest path under W(e) + B(e) - M·[e required], M above every walk sum.  An ORF
 * may be required and biased; a refused ORF's bias is ignored; an ORF both refused and required, or |B| > 2^52, is PHX_E_ARG before any
 * kernel.  delta = float(S(P) - D) / 1000.0 (may be negative), unmet[i] = |R| - (required ORFs the path calls), |R| where there is no result;
 * phx_tap_repath reports S(P).  Any of bias, forbid and require may be NULL (empty).
 * status[i] as phx_constrain_flat and phx_evidence_flat: PHX_S_NEGCYCLE (no genes, delta +inf) when the source reaches a cycle through a
 * required ORF's edge or one that the biases make negative; PHX_S_OVERFLOW when the layout's bound plus the sum of |B| does not fit the
 * contig's limb class.
 * Reductions, byte for byte and per contig: every B zero is phx_constrain_flat, nothing required is phx_evidence_flat (unmet 0), both is
 * phx_reannotate_flat — a contig runs the combined kernels only when it has a required and a biased ORF.  The calls share their buffers and
 * their cached result (keyed on the three arrays and the flags).  phx_remargins_flat is PHX_E_STATE after a solve with a contig that had
 * required ORFs, as after phx_constrain_flat.  (Addition, version unchanged: probe for the symbol.) */
int phx_curate_flat(phx_ctx *ctx, const int64_t *bias, const uint8_t *forbid, const uint8_t *require, const int64_t *orf_offsets /* [n+1] */, uint32_t flags, phx_gene *genes,
                    int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, double *delta /* [n] */, int32_t *unmet /* [n] */, int64_t *total);
/* orf_offsets[n+1] of the batch last run as phx_reannotate_flat expects them: cumulative ORF counts, a contig with a run error or without
 * device distances counting none (the offsets phx_margins_flat reports, without computing the margins or the certificate). */
int phx_orf_offsets(phx_ctx *ctx, int64_t *orf_offsets /* [n+1] */);
/* path and D_F of the last re-annotation, like phx_tap_path (a contig that was not solved again: the run's).  PHX_E_STATE without one. */
int phx_tap_repath(phx_ctx *ctx, int32_t contig, int32_t *path, int32_t cap, int32_t *n_path, uint64_t *dist_limbs, int32_t cap_limbs);
/* device time of the last re-annotation (HIP events around device work only), ms[3]: mask build, masked solve, in-order parents + path +
 * genes + the copies to the host.  All 0 before the first. */
int phx_reannotate_ms(phx_ctx *ctx, float *ms /* [3] */);

/* ---- re-annotation margins: per-ORF path margins under a mask or bias ----
 * The margins of phx_margins_flat on the graph of the last re-annotation of the batch last run — phx_reannotate_flat or phx_evidence_flat,
 * or phx_constrain_flat where no ORF is required: how sure every other call is, given this evidence.  For a contig that was solved again
 * under the refused set F and the bias B, G' = G_{F,B} is the graph of §14 / §19, and
 *   d_s'(v)  the re-solve's distance source -> v;  R the nodes it reached;
 *   d_t'(v)  the shortest v -> target distance in the subgraph of G' induced by R, exact, in the contig's limb class; "unreached" when no
 *            such path exists.  A node outside R is never given a value: a cycle of negative length the source does not reach is none of
 *            the forward solve's, and a cycle with one node in R lies in R entirely, so the restricted pass settles whenever the solve did;
 *   D'       = d_s'(target).
 * For ORF k with edge e = (u -> v) in G':  Delta'(k) = d_s'(u) + W(e) + B(k) + d_t'(v) - D', an integer >= 0; margin = float(Delta') / 1000.0
 * as phx_margins_flat rounds it, through = 1.  through = 0 and margin = +inf when the ORF is refused, has no edge, u or v is unreached on
 * its side, or D' is unreached.  called = 1 iff the ORF is among the genes the re-annotation call returns for the contig (the device's
 * lists; no host re-solve enters).  The smallest further bonus that gets an uncalled ORF called on top of this evidence is its margin here
 * (§19's theorem on G').  Delta' fits the contig's own limbs: phx_evidence_flat lets a contig through only if the layout's bound on
 * simple-path sums plus the sum of |B| fits its class with 5 spare bits, and d_s', d_t', |W + B| and D' each obey that bound.
 * Records as phx_margins_flat (rec == NULL: size query; phx_tap_orfs order).  status[i]:
 *   a run error (< 0) or PHX_S_OVERFLOW without device distances: that status, no records (as phx_margins_flat);
 *   a contig that was not solved again: phx_margins_flat's status and records, with `called` as above;
 *   solved again with a status < 0 (PHX_S_NEGCYCLE, PHX_S_OVERFLOW from the biased bound): that status, no records;
 *   solved again, PHX_S_NOPATH: status 1, every record through = 0 and +inf;  solved again, status 0: the records as defined.
 *   PHX_S_NEGCYCLE (no records) also if the reverse pass hits its caps (the lemma above says it never does; the caps stay).
 * PHX_E_STATE, before any kernel, without a re-annotation of this run, and when a contig of the last one was solved under the required
 * policy (margins under an infinite bonus are a different definition).  Computed at the first call after a re-annotation solve (on top
 * of phx_margins_flat's shared part), kept until the next solve or run; a re-annotation call that hits its cache keeps it.  Nothing the
 * other entry points return changes.  (Additions, version unchanged: probe for the symbol.) */
int phx_remargins_flat(phx_ctx *ctx, phx_orf_margin *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the re-annotation margins (HIP events), ms[4]: apply (the refused / biased out-edges), the
 * conditioned reverse pass, records, the copy to the host.  All 0 before the first. */
int phx_remargins_ms(phx_ctx *ctx, float *ms /* [4] */);
/* d_s' (which 0) or d_t' (which 1) of every node of a contig of the last re-annotation, like phx_tap_dist (sssp_nl words per node; an
 * unreached node has a top word >= 2^61).  A contig that was not solved again: the run's vectors (phx_tap_dist / phx_tap_dist_target);
 * one whose re-solve left no such vector (an error; no path for d_t'): every node unreached.  PHX_E_STATE as phx_remargins_flat. */
int phx_tap_redist(phx_ctx *ctx, int32_t contig, int32_t which, uint64_t *dist_limbs, int64_t cap_words);

/* ---- re-annotation drop margins: the support of every call under a mask or bias ----
 * phx_drop_margins_flat on the graph of the last re-annotation of the batch last run — the re-annotations phx_remargins_flat covers.  For a
 * contig solved again under the refused set F and the bias B with status 0, G', R, d_s', d_t' and D' are phx_remargins_flat's and
 * P' = p_0 ... p_K is the re-annotation's device path (phx_tap_repath).  A called gene is a CDS ORF edge of P', its stop node p_j as for
 * phx_drop_margins_flat; D'_{-g} is the shortest source -> target distance under W' = W + B in G' without p_j, which is the D of
 * phx_evidence_flat(B, F + every ORF of the gene's stop group).  drop = float(D'_{-g} - D') / 1000.0 as phx_drop_margins_flat rounds it,
 * >= 0, bypass = 1; bypass = 0 and drop = +inf when no path of G' avoids the stop node.  score is what the re-annotation call's gene
 * record carries (the ORF's weight without the bias); called = 1 iff the gene is among the genes that call returns for the contig (the
 * device's lists; no host re-solve enters).  Every value fits the contig's own limbs (§29, with phx_evidence_flat's biased bound).
 * Records as phx_drop_margins_flat (rec == NULL: size query), in path order.  status[i]:
 *   a run error (< 0) or PHX_S_OVERFLOW without device distances: that status, no records;
 *   a contig that was not solved again: phx_drop_margins_flat's status and records, byte for byte;
 *   solved again with a status < 0: that status, no records;  solved again, PHX_S_NOPATH: status 1, no records (no gene is called);
 *   solved again, status 0: the records as defined; PHX_S_NEGCYCLE without records if the conditioned reverse pass hit its caps.
 * PHX_E_STATE, before any kernel, without a re-annotation of this run, and when a contig of the last one was solved under the required
 * policy (drops under required ORFs, where the dropped gene may be a pin, are a different definition).  Computed at the first call after a
 * re-annotation solve, on top of phx_remargins_flat's computation (and phx_drop_margins_flat's when a contig was not solved again), in
 * buffers of its own; kept until the next solve or run.  Nothing the other entry points return changes.  (Additions, version unchanged:
 * probe for the symbol.) */
int phx_redrops_flat(phx_ctx *ctx, phx_gene_drop *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the re-annotation drop margins (HIP events), ms[4]: trees + labels, candidates + sparse table,
 * fixups, the copy of the records to the host — the conditioned kernels alone (phx_remargins_ms and phx_drop_ms have the parts below
 * them).  All 0 before the first. */
int phx_redrops_ms(phx_ctx *ctx, float *ms /* [4] */);
/* counters of the last computation, out[4], as phx_drop_stats, over the contigs that were solved again */
int phx_redrop_stats(phx_ctx *ctx, int64_t *out /* [4] */);

/* ---- re-annotation replacements: the best path without each call of a re-annotation ----
 * phx_replacements_flat on the graph of the last re-annotation phx_redrops_flat is defined for.  For every record of phx_redrops_flat
 * with bypass = 1 a replacement path R'_g: a simple source -> target path of G' — every edge an edge of the device graph, none an ORF edge
 * the call refused — that does not visit the gene's stop node p_j, of weight exactly D'_{-g} under W' = W + B; it leaves the
 * re-annotation's path P' (phx_tap_repath) at one node before p_j, rejoins it at one node behind, and no node of the detour lies on P'.
 * Records are phx_gene_repl: drop / called / bypass bit-equal to phx_redrops_flat's, the removed and the added genes as for
 * phx_replacements_flat, score what the re-annotation call's gene records carry (the ORF's weight without the bias, -20 for a tRNA pair).
 * The bytes do not depend on the batch or on the create flags (tie rule of DESIGN.md §13).  Order, offsets, statuses and the PHX_E_STATE
 * rule are phx_redrops_flat's; a contig that was not solved again gets phx_replacements_flat's records and genes, byte for byte but for
 * gene_off.  Size query, argument checks and caps as phx_replacements_flat.  Computed at the first call after a re-annotation solve, on top
 * of phx_redrops_flat's computation (and phx_replacements_flat's when a contig was not solved again), in buffers of its own; kept until the
 * next solve or run.  Nothing the other entry points return changes.  (Additions, version unchanged: probe for the symbol.) */
int phx_rereplacements_flat(phx_ctx *ctx, phx_gene_repl *rec, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets /* [n+1] */,
                            int32_t *status /* [n] */, int64_t *total, int64_t *gene_total);
/* R'_g of record k of contig `contig` (k counts the contig's records of phx_rereplacements_flat), as phx_tap_replacement: the prefix and
 * the suffix are the re-annotation's path.  For a contig that was not solved again: phx_tap_replacement's result. */
int phx_tap_rereplacement(phx_ctx *ctx, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path);
/* device time of the last computation, ms[3], and its counters, out[5], as phx_replacements_ms / phx_replacement_stats, over the contigs
 * that were solved again.  All 0 before the first and when no contig was. */
int phx_rereplacements_ms(phx_ctx *ctx, float *ms /* [3] */);
int phx_rereplacement_stats(phx_ctx *ctx, int64_t *out /* [5] */);

/* ---- re-annotation profiles: the coding profile under a mask or bias ----
 * phx_profile_flat on the graph of the last re-annotation of the batch last run — the re-annotations phx_remargins_flat covers: now that
 * this hit is in, or this call refused, is the gap beside it still a gap?  For a contig solved again under the refused set F and the bias
 * B, G', R, d_s', d_t' and D' are phx_remargins_flat's, and EVERY edge e = (u -> v) of G' — ORF edge, tRNA edge or connector — has
 *   Delta'(e) = d_s'(u) + W(e) + B(e) + d_t'(v) - D' >= 0 (inside R),  mu(e) = float(Delta'(e)) / 1000.0 as phx_margins_flat rounds it.
 * An edge takes no part when it is refused or when u or v is unreached on its side; when D' is unreached every value is +inf.  Slots,
 * ranks, the three tracks, lo / hi and the record are phx_profile_flat's.  On a contig whose re-solve has status 0 the re-annotation's
 * device path (phx_tap_repath) crosses every slot at Delta' = 0: min(fwd, rev, gap) = 0.
 * Records as phx_profile_flat (rec == NULL: size query; the same argument checks).  status[i] is phx_remargins_flat's, with n_node - 1
 * records wherever it is >= 0 and the contig has a graph:
 *   a contig that was not solved again: phx_profile_flat's status and records, byte for byte;
 *   solved again with a status < 0: that status, no records;  solved again, PHX_S_NOPATH: status 1, all three values +inf in every slot,
 *   lo / hi filled;  solved again, status 0: the records as defined; PHX_S_NEGCYCLE without records if the conditioned reverse pass hit
 *   its caps.
 * PHX_E_STATE, before any kernel, without a re-annotation of this run, and when a contig of the last one was solved under the required
 * policy (a profile under pins is a minimum over (lost, s) pairs: a different definition).  Computed at the first call after a
 * re-annotation solve, on top of phx_remargins_flat's computation (and phx_profile_flat's when a contig was not solved again), in buffers
 * of its own; kept until the next solve or run.  Nothing the other entry points return changes.  (Additions, version unchanged: probe for
 * the symbol.) */
int phx_reprofile_flat(phx_ctx *ctx, phx_profile_slot *rec, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the re-annotation profiles (HIP events), ms[3], as phx_profile_ms: tables, bounds, copy — the
 * conditioned kernels alone (phx_remargins_ms and phx_profile_ms have the parts below them).  All 0 before the first and when no contig
 * was solved again. */
int phx_reprofile_ms(phx_ctx *ctx, float *ms /* [3] */);

/* ---- pinned profiles: the coding profile under required ORFs ----
 * phx_reprofile_flat for every re-annotation of the batch last run, phx_constrain_flat and phx_curate_flat with required ORFs included:
 * now that these genes are pinned, is the gap beside them still a gap — and what does the stretch under a pin cost as anything but that
 * gene, and how many pins would that give up?  For a contig solved again under the required policy (F, B and R), G', R_n, W', M, d_s',
 * d_t' and D' are phx_pinmargins_flat's, and EVERY edge e = (u -> v) of G' — ORF edge, tRNA edge or connector — has
 *   Delta''(e) = d_s'(u) + W'(e) + d_t'(v) - D' = lost(e)·M + s(e) >= 0   (NL + 1 limbs),
 * decoded as phx_pinmargins_flat decodes it: lost the top limb plus the sign bit of limb NL - 1, s the low NL limbs as the class's two's
 * complement, mu(e) = float(s) / 1000.0.  An edge takes no part when it is refused or when u or v is unreached on its side.  Slots, ranks,
 * the three tracks, lo / hi and the record are phx_profile_flat's.  Per slot and track the result is the LEXICOGRAPHIC minimum of
 * (lost(e), s(e)) over the covering edges of the track: mu of that minimum in the record's fwd / rev / gap, its lost in lost[3 k + 0 / 1 / 2]
 * for record k.  A value may be negative where lost > 0 (a path that drops a pin can be cheaper); where no edge of the track covers the
 * slot the value is +inf and lost 0.  On a contig whose re-solve has status 0 the minimum over the three tracks is (0, 0.0) in every slot.
 * rec has cap entries, lost 3 * cap (rec == NULL: size query; with rec, lost is needed: PHX_E_ARG).  status[i] is phx_pinmargins_flat's:
 *   a contig that was not solved again: phx_profile_flat's status and records, lost 0;
 *   solved again without a required ORF: what phx_reprofile_flat returns for it after the same call without the other contigs' required
 *   ORFs, lost 0;
 *   solved under the required policy, status 0, the pinned reverse pass settled: n_node - 1 records as defined;  PHX_S_NOPATH: status 1,
 *   every value +inf, lost 0, lo / hi filled;  a re-solve error: that status, no records;  the pinned reverse pass hit its caps:
 *   PHX_S_NEGCYCLE, no records.
 * When no contig of the last re-annotation was solved under the required policy the three arrays are phx_reprofile_flat's byte for byte
 * and lost is all 0.  PHX_E_STATE, before any kernel, only without a re-annotation of this run; phx_reprofile_flat keeps refusing a solve
 * with required ORFs.  Computed at the first call after a re-annotation solve, on top of phx_pinmargins_flat's computation, in buffers of
 * its own; kept until the next solve or run.  Nothing the other entry points return changes.  (Additions, version unchanged: probe for
 * the symbol.) */
int phx_pinprofile_flat(phx_ctx *ctx, phx_profile_slot *rec, int32_t *lost /* [3 * cap] */, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the pinned profiles (HIP events), ms[3]: tables, records, copy — the pinned kernels alone.  All 0
 * before the first and when no contig was solved under the required policy. */
int phx_pinprofile_ms(phx_ctx *ctx, float *ms /* [3] */);
/* counters of the last computation, out[3]: contigs the pinned kernels covered; table rounds they ran (3 per contig, and one more per
 * distinct lost > 0 that a track's slots hold); slots with lost > 0 on any track. */
int phx_pinprofile_stats(phx_ctx *ctx, int64_t *out /* [3] */);

/* ---- pinned margins: per-ORF path margins under required ORFs ----
 * phx_remargins_flat for every re-annotation of the batch last run, phx_constrain_flat and phx_curate_flat with required ORFs included.  A
 * contig solved again under F, B and R has W'(e) = W(e) + B(e) - M·[e required and present], M = 2^(64 NL) for its limb class NL, and
 *   d_s'(v)  the solve's distance, NL + 1 limbs: the top limb is minus the number of required edges behind v;  R_n the nodes it reached;
 *   d_t'(v)  the exact shortest v -> target distance under W' in the subgraph induced by R_n, NL + 1 limbs;  D' = d_s'(target).
 * For ORF k with edge e = (u -> v):  Delta''(k) = d_s'(u) + W'(e) + d_t'(v) - D' >= 0 = lost·M + s with s the low NL limbs read as the
 * class's two's complement:  lost[k] >= 0 is the number of kept required ORFs that the best path through k gives up, margin =
 * float(s) / 1000.0 as phx_margins_flat rounds it — negative margins occur where lost > 0 (a path that drops a pin can be cheaper); the
 * order is (lost, margin) >= (0, 0.0), which a called gene has.  through = 0, margin +inf, lost 0 as phx_remargins_flat has them.
 * Requiring one more ORF k (through = 1, neither refused nor required) on top of F, B, R gives the smaller of the present optimum and
 * (kept - lost + 1 required ORFs, sum + s): with lost = 0 an uncalled k gets called, unmet does not grow and delta grows by margin —
 * unless k lies on a cycle the source reaches (PHX_S_NEGCYCLE).
 * rec and lost are parallel, cap entries each (rec == NULL: size query; with rec, lost is needed); phx_tap_orfs order; status[i] as
 * phx_remargins_flat's table with "solved again" covering every mode.  A contig that was not solved under the required policy has
 * phx_remargins_flat's records (those of the same call without the other contigs' required ORFs) and lost 0; when no contig was, the
 * three arrays are phx_remargins_flat's byte for byte.  PHX_E_STATE only without a re-annotation of this run.  Computed at the first call
 * after a re-annotation solve, kept until the next solve or run.  phx_remargins_flat and phx_tap_redist keep refusing a solve with
 * required ORFs.  (Additions, version unchanged: probe for the symbol.) */
int phx_pinmargins_flat(phx_ctx *ctx, phx_orf_margin *rec, int32_t *lost, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation of the pinned margins (HIP events), ms[4]: apply, reverse pass, records, copy — both kernel sets. */
int phx_pinmargins_ms(phx_ctx *ctx, float *ms /* [4] */);
/* phx_tap_redist for every re-annotation: *words_per_node (may be NULL) is sssp_nl + 1 for a contig solved under the required policy —
 * the top word carries the count, an unreached node has a top word >= 2^61 — and sssp_nl otherwise. */
int phx_tap_pindist(phx_ctx *ctx, int32_t contig, int32_t which, uint64_t *dist_limbs, int64_t cap_words, int32_t *words_per_node);

/* ---- pinned drop margins: the support of every call under required ORFs ----
 * phx_redrops_flat for every re-annotation of the batch last run, phx_constrain_flat and phx_curate_flat with required ORFs included.  For
 * a contig solved again under F, B and R with status 0, G', R_n, W', d_s', d_t' and D' are phx_pinmargins_flat's and P' = p_0 ... p_K is
 * the re-annotation's device path.  A called gene is a CDS ORF edge of P', its stop node p_j as for phx_drop_margins_flat; D'_{-g} is the
 * shortest source -> target distance under W' in G'[R_n] without p_j, in NL + 1 limbs, and Delta = D'_{-g} - D' >= 0 = lost·M + s, decoded
 * as phx_pinmargins_flat decodes Delta'':  lost[k] >= 0 is the number of kept required ORFs that the best annotation without a gene at
 * this stop gives up (net: a kept pin at the stop is lost, a required ORF that comes in instead counts against it), drop = float(s) / 1000.0 — negative drops occur where
 * lost > 0; the order is (lost, drop) >= (0, 0.0).  No such path: bypass = 0, drop = +inf, lost = 0.  With grp the ORFs of the gene's stop
 * group, D'_{-g} is the optimum of phx_curate_flat(B, F + grp, R - grp): lost = the difference of the two calls' (required - unmet), drop =
 * the difference of their delta sums.  score and called as phx_redrops_flat; records in path order, a tRNA pair gets none.
 * rec and lost are parallel, cap entries each (rec == NULL: size query; with rec, lost is needed).  status[i] as phx_redrops_flat's table
 * with "solved again" covering every mode.  A contig that was solved again without a required ORF has phx_redrops_flat's records (those of
 * the same call without the other contigs' required ORFs) and lost 0, one that was not solved again phx_drop_margins_flat's and lost 0;
 * when no contig was solved under the required policy, the arrays are phx_redrops_flat's byte for byte.  PHX_E_STATE only without a
 * re-annotation of this run.  Computed at the first call after a re-annotation solve, on top of phx_pinmargins_flat's computation, in
 * buffers of its own; kept until the next solve or run.  Nothing the other entry points return changes: phx_redrops_flat,
 * phx_rereplacements_flat and their taps keep refusing a solve with required ORFs.  (Additions, version unchanged: probe for the symbol.) */
int phx_pindrops_flat(phx_ctx *ctx, phx_gene_drop *rec, int32_t *lost, int64_t cap, int64_t *offsets /* [n+1] */, int32_t *status /* [n] */, int64_t *total);
/* device time of the last computation (HIP events), ms[4], as phx_redrops_ms: trees + labels, candidates + sparse table, fixups, the copy
 * of the records — and its counters, out[4], as phx_drop_stats, both over the contigs that were solved again: the pinned kernels' over
 * the contigs solved under the required policy plus phx_redrops_ms / phx_redrop_stats' over the others. */
int phx_pindrops_ms(phx_ctx *ctx, float *ms /* [4] */);
int phx_pindrop_stats(phx_ctx *ctx, int64_t *out /* [4] */);

/* ---- pinned replacements: the best path without each call, under required ORFs ----
 * phx_rereplacements_flat for every re-annotation of the batch last run, phx_constrain_flat and phx_curate_flat with required ORFs included.
 * For every record of phx_pindrops_flat with bypass = 1 of a contig solved under the required policy (status 0) a replacement path R'_g: a
 * simple source -> target path of G'[R_n] — every edge an edge of the device graph, none an ORF edge the call refused — that does not visit
 * the gene's stop node p_j, of weight exactly D'_{-g} in NL + 1 limbs under W' = W + B - M·[required]: it carries (the required ORFs on P')
 * - lost required ORF edges, and S(R'_g) - S(P') is the integer whose rounding is the record's drop.  It leaves the re-annotation's path
 * P' (phx_tap_repath) at one node before p_j, rejoins it at one node behind, and no node of the detour lies on P'.  Records are
 * phx_gene_repl, unchanged, with a parallel int32 lost[]: drop / called / bypass / lost bit-equal to phx_pindrops_flat's, the removed and
 * the added genes as for phx_replacements_flat, score the ORF's weight without the bias (-20 for a tRNA pair).  The bytes do not depend
 * on the batch or on the create flags (tie rule of DESIGN.md §13 with "cost" read in the (lost, s) order).  Order, offsets, statuses and the
 * PHX_E_STATE rule (only without a re-annotation of this run) are phx_pindrops_flat's.  A contig that was solved again without a required
 * ORF has phx_rereplacements_flat's records and genes (those of the same call without the other contigs' required ORFs) and lost 0, one
 * that was not solved again phx_replacements_flat's and lost 0, byte for byte but for gene_off; when no contig was solved under the
 * required policy, the arrays are phx_rereplacements_flat's.  rec and lost are parallel, cap entries each (rec or genes NULL: size query;
 * with rec, lost is needed); caps as phx_rereplacements_flat.  Computed at the first call after a re-annotation solve, on top of
 * phx_pindrops_flat's computation, in buffers of its own; kept until the next solve or run.  Nothing the other entry points return changes:
 * phx_redrops_flat, phx_rereplacements_flat and their taps keep refusing a solve with required ORFs.  (Additions, version unchanged: probe
 * for the symbol.) */
int phx_pinreplacements_flat(phx_ctx *ctx, phx_gene_repl *rec, int32_t *lost, int64_t cap, phx_gene *genes, int64_t gene_cap, int64_t *offsets /* [n+1] */,
                             int32_t *status /* [n] */, int64_t *total, int64_t *gene_total);
/* R'_g of record k of contig `contig` (k counts the contig's records of phx_pinreplacements_flat), as phx_tap_rereplacement: the prefix and
 * the suffix are the re-annotation's path.  A contig solved again without a required ORF gives what phx_tap_rereplacement gives for it,
 * one that was not solved again phx_tap_replacement's result. */
int phx_tap_pinreplacement(phx_ctx *ctx, int32_t contig, int32_t k, int32_t *path, int32_t cap, int32_t *n_path);
/* device time of the last computation, ms[3], and its counters, out[5], as phx_replacements_ms / phx_replacement_stats, both over the
 * contigs that were solved again: the pinned kernels' over the contigs solved under the required policy plus phx_rereplacements_ms /
 * phx_rereplacement_stats' over the others. */
int phx_pinreplacements_ms(phx_ctx *ctx, float *ms /* [3] */);
int phx_pinreplacement_stats(phx_ctx *ctx, int64_t *out /* [5] */);

/* ---- scenario batches: many masked re-annotations of the batch last run in one call ----
 * n_scen scenarios, each a contig of the batch last run and a set F of its ORFs, solved side by side on the resident graph, one
 * workgroup per scenario.  Scenario j is, by definition, the masked re-annotation above applied to contig scen_contig[j] with F = its
 * listed ORFs: status[j], delta[j] and genes[offsets[j] .. offsets[j+1]) are byte for byte what phx_reannotate_flat returns for that
 * contig when the mask holds exactly F on that contig and bit 0 of its flags is set — format, order, tie rule, PHX_S_NOPATH with +inf,
 * PHX_S_OVERFLOW and a run error passed through.  Scenarios are independent of each other: several may name the same contig and may
 * overlap; an empty list is solved like any other (the device path); duplicates inside a list are allowed.  Only refused sets here:
 * phx_pinned_scenarios_flat below takes required ORFs per scenario as well.
 *   scen_contig  [n_scen]: contig of the batch last run
 *   scen_off     [n_scen+1]: scenario j lists scen_orf[scen_off[j] .. scen_off[j+1]); starts at 0, non-decreasing
 *   scen_orf     indices into phx_tap_orfs order of the scenario's contig
 *   orf_offsets  [n+1]: as phx_reannotate_flat (must equal phx_orf_offsets)
 *   flags        reserved: pass 0
 *   genes        NULL: size query (offsets, status, delta, total are filled in); the fetch with the same arguments reuses the solve
 * PHX_E_ARG before any kernel for wrong orf_offsets, a contig outside [0, n), an ORF index outside its contig's count, or scen_off
 * not starting at 0 or decreasing: nothing from the caller indexes device memory unchecked.  PHX_E_STATE before a run; the result is
 * invalidated by the next upload or run.  The scenarios are solved in chunks under a device-memory budget (an internal default;
 * PHX_SCEN_BYTES in the environment, read by phx_create*, overrides it); the result does not depend on the chunking, and a scenario
 * larger than the budget is solved alone.  The solve owns its buffers: nothing phx_download*, the taps, the margins, the drops, the
 * replacements, phx_reannotate_flat's cached result or the certificate return changes. */
int phx_scenarios_flat(phx_ctx *ctx, int64_t n_scen, const int32_t *scen_contig /* [n_scen] */, const int64_t *scen_off /* [n_scen+1] */,
                       const int32_t *scen_orf, const int64_t *orf_offsets /* [n+1] */, uint32_t flags, phx_gene *genes, int64_t cap,
                       int64_t *offsets /* [n_scen+1] */, int32_t *status /* [n_scen] */, double *delta /* [n_scen] */, int64_t *total);
/* ---- pinned scenario batches: many pinned re-annotations of the batch last run in one call ----
 * phx_scenarios_flat with a second list per scenario: scenario j refuses F_j = forbid_orf[forbid_off[j] .. forbid_off[j+1]) and requires
 * R_j = require_orf[require_off[j] .. require_off[j+1]), both indices in phx_tap_orfs order of contig scen_contig[j].  It is, by
 * definition, phx_constrain_flat applied to that contig with exactly these two sets and bit 0 of its flags set: status[j], delta[j],
 * unmet[j] and genes[offsets[j] .. offsets[j+1]) are byte for byte that call's for the contig — PHX_S_NOPATH with +inf, PHX_S_NEGCYCLE
 * (no genes, +inf, unmet = |R_j|) when a cycle the source reaches runs through a required edge, PHX_S_OVERFLOW and a run error passed
 * through, unmet = |R_j| wherever there is no result.  |R_j| counts ORFs: duplicates inside a list are allowed and count once.  A scenario
 * with R_j empty is phx_scenarios_flat's scenario byte for byte (the same kernels), unmet 0.  Scenarios are independent: the same ORF may
 * be refused in one and required in another; the same ORF in both lists of ONE scenario is PHX_E_ARG before any kernel.
 * Calling convention (size query with genes NULL, then the fetch), argument checks (on both lists), state rules, chunking and the
 * device-memory budget are those of phx_scenarios_flat; require_off and unmet must not be NULL.  The two calls are one solve on one set
 * of buffers with one cached result keyed on both lists: phx_scenarios_ms, phx_scenario_chunks and phx_tap_scenario_path report on the
 * last scenario solve of either kind, and for a scenario with required ORFs the distance phx_tap_scenario_path reports is the W-sum W(P)
 * in the contig's own limbs, as phx_tap_repath does after phx_constrain_flat. */
int phx_pinned_scenarios_flat(phx_ctx *ctx, int64_t n_scen, const int32_t *scen_contig /* [n_scen] */, const int64_t *forbid_off /* [n_scen+1] */,
                              const int32_t *forbid_orf, const int64_t *require_off /* [n_scen+1] */, const int32_t *require_orf,
                              const int64_t *orf_offsets /* [n+1] */, uint32_t flags /* reserved: 0 */, phx_gene *genes, int64_t cap,
                              int64_t *offsets /* [n_scen+1] */, int32_t *status /* [n_scen] */, double *delta /* [n_scen] */, int32_t *unmet /* [n_scen] */,
                              int64_t *total);
/* ---- evidence scenario batches: many evidence-weighted re-annotations of the batch last run in one call ----
 * phx_scenarios_flat with a list of (ORF, B) pairs per scenario: scenario j refuses F_j = forbid_orf[forbid_off[j] .. forbid_off[j+1]) and
 * biases ORF bias_orf[k] by bias_val[k] for k in [bias_off[j], bias_off[j+1]), indices in phx_tap_orfs order of contig scen_contig[j], B a
 * signed integer in the solver's units.  The bias of an ORF is the sum of the B of its pairs; a refused ORF's bias is ignored.  It is, by
 * definition, phx_evidence_flat applied to that contig with exactly that bias, that refused set and bit 0 of its flags set: status[j],
 * delta[j] (which may be negative) and genes[offsets[j] .. offsets[j+1]) are byte for byte that call's for the contig — PHX_S_NOPATH with
 * +inf, PHX_S_NEGCYCLE (no genes, +inf), PHX_S_OVERFLOW from the limb-class test and a run error passed through.  A scenario whose summed
 * biases are all zero is phx_scenarios_flat's scenario byte for byte (the same kernels).  Scenarios are independent; they may repeat a
 * contig, overlap, be empty and hold duplicates.
 * Calling convention, argument checks (on both lists: both offset arrays start at 0 and never decrease), state rules, chunking and the
 * device-memory budget are those of phx_scenarios_flat; bias_off must not be NULL, and a summed |B| > 2^52 is PHX_E_ARG before any kernel.
 * It is one solve with the two calls above on one set of buffers, with one cached result keyed on the refused lists and the merged bias
 * lists: phx_scenarios_ms, phx_scenario_chunks and phx_tap_scenario_path, whose distance is then D_B, report on the last scenario solve of
 * any kind.  No required list per scenario (since added: phx_curate_scenarios_flat below).  (Addition, version unchanged: probe for the symbol.) */
int phx_evidence_scenarios_flat(phx_ctx *ctx, int64_t n_scen, const int32_t *scen_contig /* [n_scen] */, const int64_t *forbid_off /* [n_scen+1] */,
                                const int32_t *forbid_orf, const int64_t *bias_off /* [n_scen+1] */, const int32_t *bias_orf, const int64_t *bias_val,
                                const int64_t *orf_offsets /* [n+1] */, uint32_t flags /* reserved: 0 */, phx_gene *genes, int64_t cap,
                                int64_t *offsets /* [n_scen+1] */, int32_t *status /* [n_scen] */, double *delta /* [n_scen] */, int64_t *total);
/* ---- combined scenario batches: many combined re-annotations of the batch last run in one call ----
 * All three lists per scenario: scenario j refuses F_j (forbid_*), requires R_j (require_*) and biases the ORFs of its (ORF, B) pairs
 * (bias_*), each as in the two calls above.  It is, by definition, phx_curate_flat applied to contig scen_contig[j] with exactly that bias,
 * that refused set, that required set and bit 0 of its flags set: status[j], delta[j], unmet[j] and genes[offsets[j] .. offsets[j+1]) are
 * byte for byte that call's for the contig, and phx_tap_scenario_path returns the path and S(P) in the contig's own limbs as
 * phx_tap_repath does after phx_curate_flat.  The order (-c(P), S(P)), the tie rule, PHX_S_NOPATH, PHX_S_NEGCYCLE of both kinds (a cycle
 * the source reaches through a required edge, or one a bonus has made negative; never for a cycle the source does not reach),
 * PHX_S_OVERFLOW from the limb-class test before the sweep and unmet = |R_j| wherever there is no result are those of DESIGN.md §22.
 * An ORF may be required and biased, its bias then counts; a refused ORF's bias is ignored; duplicates in a required list count once,
 * duplicate bias pairs are summed.  Per scenario the call reduces, by the same kernels and byte for byte, to
 * phx_pinned_scenarios_flat's scenario when no summed bias outside F_j is non-zero, to phx_evidence_scenarios_flat's (unmet 0) when R_j
 * is empty, and to phx_scenarios_flat's when both hold; one call may mix all four kinds.
 * Calling convention, argument checks (on all three lists, all before any kernel; an ORF in F_j and R_j, or a summed |B| > 2^52, is
 * PHX_E_ARG), state rules, chunking and the device-memory budget are those of the calls above; require_off, bias_off and unmet must not
 * be NULL.  It is one solve with the three calls above on one set of buffers, with one cached result keyed on all three lists — a call
 * is served from a sibling's cached result exactly when it reduces to it.  (Addition, version unchanged: probe for the symbol.) */
int phx_curate_scenarios_flat(phx_ctx *ctx, int64_t n_scen, const int32_t *scen_contig /* [n_scen] */, const int64_t *forbid_off /* [n_scen+1] */,
                              const int32_t *forbid_orf, const int64_t *require_off /* [n_scen+1] */, const int32_t *require_orf,
                              const int64_t *bias_off /* [n_scen+1] */, const int32_t *bias_orf, const int64_t *bias_val,
                              const int64_t *orf_offsets /* [n+1] */, uint32_t flags /* reserved: 0 */, phx_gene *genes, int64_t cap,
                              int64_t *offsets /* [n_scen+1] */, int32_t *status /* [n_scen] */, double *delta /* [n_scen] */, int32_t *unmet /* [n_scen] */,
                              int64_t *total);
/* device time of the last scenario solve (of any kind), summed over its chunks, ms[3]: slot records + bitmap slices, masked solve, in-order parents +
 * path + genes + the copies to the host.  All 0 before the first. */
int phx_scenarios_ms(phx_ctx *ctx, float *ms /* [3] */);
/* path and D_F of scenario `scen` of the last scenario solve, like phx_tap_repath (n_path 0: no path, or a scenario whose contig was not
 * solved).  The slices of the last chunk are the ones still on the device: PHX_E_STATE for a scenario of an earlier chunk (with the default
 * budget a call is one chunk), and without a scenario solve of this run. */
int phx_tap_scenario_path(phx_ctx *ctx, int64_t scen, int32_t *path, int32_t cap, int32_t *n_path, uint64_t *dist_limbs, int32_t cap_limbs);
/* chunks the last scenario solve was split into (0 before the first, and when no scenario needed the device; PHX_E_ARG without a context) */
int64_t phx_scenario_chunks(phx_ctx *ctx);

/* -d/--dump of the reference (phanotate.py:58,61) for one contig of the batch last run: one line per edge of its graph,
 *     repr(source) TAB repr(target) TAB str(weight * 1000)                                   (edges.py:17-23, nodes.py:14-21)
 * in Graph.iteredges order, the weights as the reference's 28-digit Decimals (the chain replayed by csrc/phx_dec.c on the integers
 * the device delivers, csrc/phx_exact.inc) — byte for byte what an upstream install prints.  *text is malloc'ed (NUL-terminated),
 * release with phx_free_text.  Host-side formatting, ~0.3 s for a 170 kb genome. */
int phx_dump_text(phx_ctx *ctx, int32_t contig, char **text, int64_t *text_len);

/* ---- the solver alone (the fastpathz boundary, phanotate.py:56-64) ----
 * Edges (src[i] -> dst[i]) over nodes 0..V-1 with integer weights given as n_limbs little-endian
 * 64-bit words each (two's complement).  Writes the node ids of the shortest path source..target to
 * path_out (cap entries) and its length to *n_path (0 if unreachable).  V < 2^29 (PHX_E_ARG beyond). */
int phx_solve(phx_ctx *ctx, int32_t V, int32_t E, const int32_t *src, const int32_t *dst, const uint64_t *w_limbs,
              int32_t n_limbs, int32_t source, int32_t target, int32_t *path_out, int32_t cap, int32_t *n_path,
              uint64_t *dist_limbs);

/* ---- measurement ---- */
#define PHX_N_STAGES 14
/* When on, every kernel launch of phx_run is bracketed by hipEvents on the ctx stream. */
int phx_set_profiling(phx_ctx *ctx, int on);
/* The same for a subset of the stages (bit k = stage k; 0 switches profiling off): two events per run instead of two per stage. */
int phx_set_profiling_stages(phx_ctx *ctx, uint32_t stage_mask);
/* ms[k] = accumulated GPU time of stage k since the last reset; names via phx_stage_name(k).  (Stage 10 was "edge_weights" and keeps its
   index and now times k_refine + k_certify: the overlap weights are evaluated inside the edge fill.  Stage 13, "wave_plan", runs on a side
   stream BESIDE stage 8, "edges_fill": it is in the table, not in the sum of the main stream's stages.) */
int phx_get_stage_ms(phx_ctx *ctx, float *ms /* [PHX_N_STAGES] */, int32_t *launches /* [PHX_N_STAGES] */, int reset);
const char *phx_stage_name(int k);
/* Contigs, over the life of the context, whose shortest-path wavefront was launched beside the planner of its windows (batches of up to
 * 3/4 of the device's SIMDs: DESIGN.md §4), saw no progress from it for ~20 ms and handed the contig to the workgroup kernel instead
 * (phx_globals.sssp_handed_back == 5; the results are the same).  That only happens when the planner's wavefronts were not resident
 * beside the solver's — other contexts or processes holding the SIMDs —, and after the first such run the context launches the solver
 * behind its planner.  0 on an undisturbed GPU. */
int64_t phx_plan_timeouts(phx_ctx *ctx);
/* Runs of this context whose front end was the single fused launch of small batches (k_front: steady-state runs of up to 4 contigs and 40 kb in all).
 * Negative (-(runs) - 1): that kernel once waited ~4 ms at a grid barrier because its workgroups were not all resident (the GPU was
 * shared), the run was repeated with the staged kernels, and the context has used those since. */
int64_t phx_front_runs(phx_ctx *ctx);
/* Runs of this context whose nodes, node attributes, edge count and scan were the one launch k_graph_chain (steady-state runs of batches that are
 * neither a few long contigs nor k_front's; 0 under PHX_CREATE_NO_CHAIN). */
int64_t phx_chain_runs(phx_ctx *ctx);
/* Runs of this context whose 128-bit contigs were solved in segments (batches of up to 32 contigs with a contig of 10 kb or more: a contig's
 * shortest path by up to 32 wavefront pairs side by side in frames of their own, joined by a constant each and PROVEN by one pass over the
 * edges — k_seg_join / k_seg_close, phx_sssp_seg.inc).  A contig whose segments cannot be joined or proven (about 2 % of random contigs:
 * every path downstream runs over an ORF edge from in front of a segment's margin) is solved by the one-sweep kernels in the same run —
 * phx_seg_fallbacks counts them — and later runs of that batch take the one-sweep kernels.  Either way the delivered distances, parents
 * and genes are the one-sweep solver's bit for bit.  PHX_CREATE_NO_SEG / env PHX_NO_SEG=1: never. */
int64_t phx_seg_runs(phx_ctx *ctx);
int64_t phx_seg_fallbacks(phx_ctx *ctx);
/* development: the per-segment records of contig i in the run last made (8 ints each: windows | done flag, solver status, first node, end node, the solver's time in
 * 10 ns ticks, phases, packs taken, step-backs); returns the number of records (0: that run did not use segments) */
int phx_seg_stats(phx_ctx *ctx, int32_t i, int32_t *out, int32_t cap_records);
/* sizes of the batch last run: positions, ORFs, nodes, edges (for the algorithmic-byte formula) */
int phx_batch_sizes(phx_ctx *ctx, int64_t *L, int64_t *n_orf, int64_t *n_node, int64_t *n_edge);

/* ---- host utilities (no device needed) ---- */
/* Deterministic synthetic phage-like contig: exactly L lower-case acgt chars. */
int phx_synth_contig(uint64_t seed, int64_t L, char *out);
/* The reference's number type on the host (csrc/phx_dec.c: Python's decimal.Decimal at prec 28, ROUND_HALF_EVEN), for the tests:
 * op = "add" "sub" "mul" "div" "pow" "ln" "exp" on the decimal texts a (and b) at `prec` digits, "str" (a as Decimal.__str__ prints
 * it), "float" (Decimal(float(a))), "repr" (repr(float(a))), "trunc1000" (int(a * 1000) as 18 hex words), "dd" (a as a double-double).
 * The result text goes to out; returns its length or a negative error. */
int phx_dec_eval(const char *op, const char *a, const char *b, int prec, char *out, int cap);
/* The double-double arithmetic of k_refine (csrc/phx_dd.h; it compiles for the host too), for the tests: op = "add" "sub" "mul" "div"
 * "exp" "log" on (ah + al) and (bh + bl), "repr" = the decimal value Decimal(repr(ah)) holds; phx_dd_shortest: the digits and decimal
 * exponent of repr(x) for 1e-10 <= x <= 1e10 (returns the number of digits, 0 outside that range). */
int phx_dd_eval(const char *op, double ah, double al, double bh, double bl, double *rh, double *rl);
int phx_dd_shortest(double x, uint64_t *digits, int32_t *exp10);

/* ---- host I/O of the CLI (no device needed; phx_host.c) ----
 * Files and texts beyond a few MB are parsed / formatted by worker threads (one per online core, at most 16; the environment
 * variable PHX_HOST_THREADS overrides the count): the results do not depend on it. */
/* FASTA, plain or gzip, read whole: what phanotate.py:32-35 gets from the external `genbank` package.  A record's name is the
 * first token of its header line (README.md:45); sequence lines are stripped of surrounding white space and joined, case kept
 * (the kernels lower-case); text before the first header is ignored. */
typedef struct phx_fasta phx_fasta;
int phx_fasta_read(const char *path, phx_fasta **out);
int32_t phx_fasta_count(const phx_fasta *f);
/* name: NUL-terminated; seq: *len characters, NOT terminated; both owned by f */
int phx_fasta_record(const phx_fasta *f, int32_t i, const char **name, const char **seq, int64_t *len);
/* all records at once, in the form phx_upload / phx_format_tabular take (any array may be NULL) */
int phx_fasta_arrays(const phx_fasta *f, const char **names, const char **seqs, int64_t *lens);
void phx_fasta_free(phx_fasta *f);
/* The reference's default output (Locus.tabular, locus.py:39-56) for n contigs from the flat arrays of phx_download_flat:
 * "#id:\t<name>", the column header, then START STOP FRAME CONTIG SCORE per gene ('%E' score; START > STOP on the reverse
 * strand).  Contigs with a negative status are skipped.  *text is malloc'ed (NUL-terminated), release with phx_free_text. */
int phx_format_tabular(int32_t n, const char *const *names, const phx_gene *genes, const int64_t *offsets, const int32_t *status, char **text, int64_t *text_len);
/* --margins FILE of the CLI for n contigs from the flat arrays of phx_margins_flat: per contig with status >= 0 "#id:\t<name>", the
 * header "#START\tSTOP\tFRAME\tCONTIG\tSCORE\tMARGIN\tCALLED", then one row per record with through == 1, ordered by left, right, strand
 * (START > STOP on the reverse strand, as the tabular writer; SCORE and MARGIN '%E'; CALLED 0 / 1).  Worker threads like
 * phx_format_tabular.  *text is malloc'ed (NUL-terminated), release with phx_free_text. */
int phx_format_margins(int32_t n, const char *const *names, const phx_orf_margin *rec, const int64_t *offsets, const int32_t *status, char **text, int64_t *text_len);
/* --drop-margins FILE of the CLI for n contigs from the flat arrays of phx_drop_margins_flat: per contig with status >= 0 "#id:\t<name>",
 * the header "#START\tSTOP\tFRAME\tCONTIG\tSCORE\tDROP\tCALLED", then one row per record in the given order (START > STOP on the reverse
 * strand; SCORE and DROP '%E'; CALLED 0 / 1).  Worker threads like phx_format_tabular.  *text is malloc'ed (NUL-terminated), release
 * with phx_free_text. */
int phx_format_drops(int32_t n, const char *const *names, const phx_gene_drop *rec, const int64_t *offsets, const int32_t *status, char **text, int64_t *text_len);
/* --drop-replacements FILE of the CLI from the flat arrays of phx_replacements_flat: per contig with status >= 0 "#id:\t<name>", the
 * header "#START\tSTOP\tFRAME\tCONTIG\tDROP\tREMOVED\tADDED", then one row per record in the given order (START > STOP on the reverse
 * strand; DROP '%E'; REMOVED / ADDED comma-separated START..STOP with START > STOP on the reverse strand, "tRNA:" in front of a tRNA pair,
 * "-" for none).  Worker threads like phx_format_tabular.  *text is malloc'ed (NUL-terminated), release with phx_free_text. */
int phx_format_replacements(int32_t n, const char *const *names, const phx_gene_repl *rec, const phx_gene *genes, const int64_t *offsets,
                            const int32_t *status, char **text, int64_t *text_len);
void phx_free_text(char *text);

#ifdef __cplusplus
}
#endif
#endif /* PHX_H */
