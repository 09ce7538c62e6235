/*
 * graphwalk.h — C ABI of the MI355X-native node2vec walk generator (H1) and
 * TopSim random-walk SimRank (H2).
 *
 * Drop-in boundary.  The reference has no FFI on this path; its interfaces are
 * a Python class (H1) and Java classes (H2).  Every entry point below names
 * the reference symbol it replaces (file:line relative to the reference
 * checkout).  A maintainer binds these from Python with ctypes (see
 * graph-embedding_amd/gwamd/_lib.py) or from Java with the JNI stub shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; opaque handles; every call returns an int status
 *     (GW_OK == 0, negative = error); gw_last_error() gives the message.
 *   - no global mutable state: seeds, modes and device ordinals are explicit;
 *     one handle may be used from one thread at a time.
 *   - every call that touches a device runs on the graph's device (or the
 *     `device` argument) and restores the caller's current device on return.
 *   - "_dev" pointers are device (HBM) pointers on the graph's device,
 *     "stream" is a hipStream_t (NULL = the default stream).  gw_n2v_walks and
 *     gw_simrank_naive (after its first call sized the workspace) are
 *     asynchronous and launch-only (no allocation, no synchronisation), so they
 *     can be captured in a HIP graph.  The TopSim calls (gw_topsim,
 *     gw_topsim_dense, gw_topsim_m, gw_topsim_double, gw_topsim_dev,
 *     gw_double_random_walk) synchronise the stream before returning (they
 *     read the kernels' capacity flag to fail loudly) and size their
 *     workspace on first use (gw_topsim_prepare does it ahead of time).
 *   - all other pointers are host pointers, caller-allocated; size them with
 *     gw_graph_info() / the documented formulas.
 *   - vertex ids crossing the boundary are dense ids in [0, n) unless a
 *     function says "labels"; gw_graph_export_csr() gives the label map.
 */
#ifndef GRAPHWALK_H
#define GRAPHWALK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define GW_OK 0
#define GW_ERR_INVALID (-1)     /* bad argument (Python ValueError)            */
#define GW_ERR_IO (-2)          /* file open/read/write (Java IOException)     */
#define GW_ERR_PARSE (-3)       /* malformed edge line (NumberFormatException) */
#define GW_ERR_NOMEM (-4)       /* host or device allocation failed            */
#define GW_ERR_DEVICE (-5)      /* HIP runtime error / no GPU                  */
#define GW_ERR_STATE (-6)       /* call order (e.g. walks before prepare)      */
#define GW_ERR_UNSUPPORTED (-7) /* option not supported for this graph/mode    */
#define GW_ERR_RANGE (-8)       /* id out of [0,V) (ArrayIndexOutOfBounds)     */
#define GW_ERR_KEY (-9)         /* missing edge key (Python KeyError)          */
#define GW_ERR_ZERODIV (-10)    /* weights sum to 0 (ZeroDivisionError)        */
#define GW_ERR_CAPACITY (-11)   /* workspace too small for the frontier        */
#define GW_ERR_INTERNAL (-12)   /* a bounded device loop ended unfinished      */

/* ---- graph semantics ------------------------------ */
/* networkx simple graph as built by read_graph (node2vec/src/main.py:76-89):
 * duplicates merge (last weight wins, to_undirected resolves reciprocal pairs
 * by node order), node order = first appearance, neighbours sorted by label,
 * original integer labels kept.                                             */
#define GW_SEM_NX_SIMPLE 0
/* structures.Graph (DeepSim/TopSimAll/src/structures/Graph.java:28-57): each
 * line appends both directions, duplicates kept, insertion order, ids dense
 * in [0,V), V given by the caller.                                          */
#define GW_SEM_JAVA_MULTI 1
/* structures.WGraph (DeepSim/TopSimAll/src/structures/WGraph.java:35-67): the
 * JAVA_MULTI adjacency of the first two fields of every line (both
 * directions appended, duplicates kept, insertion order) plus one fp64 weight
 * per unordered pair: the last line that names the pair, either way round,
 * sets it for both directions; a 2-field line sets 0.0 (the two-argument
 * addEdge).  The handle holds that weight once per adjacency entry and one
 * total per vertex (the sum over its distinct neighbours, ascending id).
 * Lines have 2 or 3 fields (anything else: GW_ERR_IO); the weight is what
 * Double.valueOf reads (surrounding whitespace, sign, decimal / exponent
 * forms, NaN, Infinity, a trailing d D f F) except hexadecimal floating-point
 * literals, which are refused with GW_ERR_PARSE.  Undirected only.  Every
 * family other than gw_simrank_weighted sees the JAVA_MULTI multigraph of the
 * adjacency lists (WGraph.randNeighbor is uniform over them).               */
#define GW_SEM_JAVA_WGRAPH 2

/* ---- node2vec modes ------------------------------------------------------ */
/* exact reference replay: per-node AND per-edge alias tables
 * (node2vec.py:83-113), uniforms supplied by the caller (MT19937 stream of
 * np.random, node2vec.py:156-157).  Needs sum(deg^2) table entries.        */
#define GW_N2V_REPLAY 0
/* scale mode: per-node alias only (or none when unweighted); second-order
 * bias by exact rejection sampling with the return edge as an outlier;
 * Philox4x32-10 keyed by (seed, walk, step, trial).  Unweighted undirected
 * NX_SIMPLE graphs: prepare builds 16 B slot entries {x, deg x, offsets x}
 * and per-row neighbour hash sets (16 B buckets); at q > 1 a step whose
 * deg(prev) < deg(cur) draws from the exact N(cur)/N(prev) mixture proposal,
 * otherwise from the uniform proposal with a lazy has_edge probe.  64 B
 * listed entries (common neighbours of each edge when they fit 40 B, which
 * answer most lazy probes) are built for q < 1 only, whatever
 * gw_options_t.listed says (at q >= 1 they would answer no probe), and are
 * skipped (same walks, 16 B entries) when they exceed half of the free HBM.
 * The walks never depend on which tables were built.                       */
#define GW_N2V_REJECTION 1
/* exact second-order sampling from per-edge common-neighbour bitsets (the
 * reference's per-edge alias tables compressed to 1 bit per entry, sum(deg^2)
 * bits; unweighted undirected NX_SIMPLE graphs): a step is a 3-way mixture
 * (return / common neighbour / other) with no has_edge probes.  Philox keyed
 * like GW_N2V_REJECTION.                                                   */
#define GW_N2V_BITSET 2
/* pick BITSET or REJECTION by modelled end-to-end time (prepare + the walk
 * steps announced in gw_options_t.expected_steps): the rejection sampler is
 * prepared (milliseconds) and a pilot of its walks counts its trials per
 * step (time = trials x a measured cost per trial); the bitset sampler's
 * time is its build model (sum over edges of min(deg u, deg v)) plus the
 * steps at its measured rate.  The choice is a function of the graph, p, q
 * and expected_steps (no timing), so runs repeat.  With expected_steps = 0
 * (unknown) the bitset sampler is taken whenever it applies and fits (the
 * throughput choice).  gw_graph_info().n2v_mode reports the choice.       */
#define GW_N2V_AUTO 3

/* ---- TopSim variants (DeepSim/TopSimAll/src/simrank/) --------------------- */
#define GW_TOPSIM_SINGLE_SAMPLE 0 /* TopSim_singleSample.java:62-203 (= _Basic) */
#define GW_TOPSIM_ENUMERATE 1     /* TopSim_Enumerate.java:61-136 (always enumerate) */
#define GW_TOPSIM_SINGLE_RW 2     /* SingleRandomWalk.java:53-92 (plain Monte-Carlo) */

typedef struct gw_graph gw_graph;

typedef struct gw_graph_info_t {
  int64_t n;          /* vertices (dense ids 0..n-1)                        */
  int64_t nnz;        /* adjacency entries (directed slots)                 */
  int64_t max_degree;
  int64_t edge_alias_entries; /* sum over slots of deg(dst); 0 until prepared */
  int32_t semantics;  /* GW_SEM_*                                           */
  int32_t directed;
  int32_t weighted;
  int32_t device;     /* -1 when not resident                               */
  int64_t sampler_bytes; /* HBM held by the prepared n2v sampler's per-slot tables
                            (bitset entries + regions, or rejection slot entries) */
  int32_t n2v_mode;   /* GW_N2V_* the last gw_n2v_prepare built (-1: none)    */
  int32_t listed;     /* 1: the rejection sampler has 64 B listed entries      */
} gw_graph_info_t;

/* Per-handle tuning (gw_graph_set_options).  Sizes and sampler choices
 * only: the walks and scores a call returns do not depend on any of them
 * (tested).  These replace what earlier versions read from environment
 * variables, so the library reads no process-global state.               */
typedef struct gw_options_t {
  /* cap on the node2vec sampler's per-slot tables (bitset entries + regions,
   * listed entries, 16 B slot entries); 0 = half of the free HBM at prepare */
  int64_t table_budget_bytes;
  /* walk steps the caller intends to run on one gw_n2v_prepare; with
   * listed = -1, GW_N2V_REJECTION builds its 64 B listed entries only when
   * their modelled build time is paid back over these steps; 0 = unknown   */
  int64_t expected_steps;
  /* GW_N2V_REJECTION listed entries, considered for q < 1 only (never built
   * at q >= 1): -1 = by expected_steps (unknown: build whenever they fit),
   * 0 = never, 1 = whenever they fit                                       */
  int32_t listed;
  /* gw_simrank_naive input row: 0 = in LDS when it fits, 1 = in HBM (same
   * result bits; exists for tests and very large m)                        */
  int32_t simrank_hbm_row;
  /* gw_n2v_walks_host staging chunk in bytes; 0 = 256 MB                   */
  int64_t host_chunk_bytes;
  /* TopSim (pipelined kernel, STEP >= 4): a heavy source's key-hash
   * partitions get 2^-k of their room (0..8; 0 = all).  A partition that
   * fills makes the call re-run without the append path (same scores);
   * exists to test that fallback                                          */
  int32_t topsim_part_shrink;
  /* gw_simrank_naive: rows per output window of the gather kernel.  0 = as
   * many as the LDS budget allows; a positive value is clamped to that
   * automatic size; negative = GW_ERR_INVALID.  Scores do not depend on it
   * beyond fp64 reassociation (a window's entries are re-sliced over the
   * waves); exists so tests reach the multi-window passes on small graphs  */
  int32_t simrank_window;
} gw_options_t;

typedef struct gw_topsim_stats_t {
  int64_t extensions;   /* path extensions (queue.add, TopSim_singleSample.java:115,147) */
  int64_t pair_updates; /* executions of TopSim_singleSample.java:189                     */
  int64_t max_frontier; /* largest per-source level size seen                             */
  int64_t walkers;      /* random children spawned (mass < degree branch)                 */
} gw_topsim_stats_t;

/* ---- library -------------------------------------------------------------- */
const char* gw_version(void);
/* message of the last failing call made with this handle (NULL: the last
 * failing handle-less call on this thread).                                 */
const char* gw_last_error(const gw_graph* g);
const char* gw_strerror(int code);
/* number of visible GPUs (0 and GW_ERR_DEVICE when none)                    */
int gw_device_count(int* count);
/* The counter-based generator behind every scale-mode draw (Philox4x32-10,
 * Salmon et al. SC'11; csrc/gw_philox.h), so a host can reproduce the walks'
 * and TopSim's draws: for i < n, in[6i..6i+5] = (c0, c1, c2, c3, k0, k1) ->
 * out[4i..4i+3] = (x, y, z, w).  device >= 0 evaluates the kernels' own
 * device build on that GPU; device = -1 evaluates the same source on the host
 * (no GPU needed).  Replaces no reference symbol (the reference draws from
 * np.random / java.util.Random streams, node2vec.py:156-157, Graph.java:17);
 * pinned to Random123's published known-answer vectors (tests).            */
int gw_philox4x32(int device, const uint32_t* in, int64_t n, uint32_t* out);

/* ---- graph construction (host) ------------------------------------------ */
/* Replaces read_graph (node2vec/src/main.py:76-89, sem NX_SIMPLE) and
 * new structures.Graph(path, V) (Graph.java:28-42, sem JAVA_MULTI).
 * delim: separator string (NULL or "" = any whitespace, as nx delimiter=None).
 * vcount: JAVA_MULTI / JAVA_WGRAPH only (ids must lie in [0,vcount)); pass -1
 * otherwise.  JAVA_MULTI ignores a third column; JAVA_WGRAPH (new
 * structures.WGraph(path, V), WGraph.java:35-54) reads it as the weight
 * whatever `weighted` says, and refuses directed != 0.                      */
int gw_graph_load_edgelist(const char* path, const char* delim, int semantics,
                           int directed, int weighted, int64_t vcount,
                           gw_graph** out);
/* Same semantics from in-memory edge arrays (labels for NX_SIMPLE, dense ids
 * for JAVA_MULTI / JAVA_WGRAPH).  w may be NULL (unweighted, every weight 1;
 * JAVA_WGRAPH: every weight 0.0, the two-argument addEdge).                 */
int gw_graph_from_edges(int64_t m, const int64_t* src, const int64_t* dst,
                        const double* w, int semantics, int directed,
                        int64_t vcount, gw_graph** out);
/* A graph whose semantics are already resolved by the caller (e.g. a
 * networkx graph handed to node2vec.Graph, node2vec.py:7-11): CSR over dense
 * ids with rows in draw order (NX_SIMPLE: sorted by dense id, dense id order
 * == label order), weights[nnz] (NULL = unweighted), labels[n] (NULL =
 * identity), node_order[n] = dense ids in G.nodes() order (NULL = 0..n-1). */
int gw_graph_from_csr(int64_t n, const int64_t* offsets, const int32_t* nbrs,
                      const double* weights, const int64_t* labels,
                      const int32_t* node_order, int semantics, int directed,
                      gw_graph** out);
/* Graph500 R-MAT (a,b,c; d = 1-a-b-c), 2^scale vertices, edge_factor*2^scale
 * generated edges, symmetrised, deduplicated, self-loops dropped, isolated
 * vertices removed; NX_SIMPLE semantics, labels = generator ids.  Philox
 * keyed by seed: identical on every host.                                   */
int gw_graph_rmat(int scale, int edge_factor, double a, double b, double c,
                  uint64_t seed, gw_graph** out);
/* R-MAT over an arbitrary vertex count n with m generated lines, Java
 * multigraph semantics (the reference generator's quadrant recursion,
 * RMATGraphGenerator.java:119-145; each line added both ways, duplicates and
 * self loops kept), V = n.  TopSim synthetic input (P10M: n=1e7, m=1e8).  */
int gw_graph_rmat_java(int64_t n, int64_t m, double a, double b, double c,
                       uint64_t seed, gw_graph** out);
int gw_graph_info(const gw_graph* g, gw_graph_info_t* info);
/* offsets[n+1], nbrs[nnz] (dense ids, row order = draw order), weights[nnz]
 * (NULL ok), labels[n] (NULL ok), node_order[n] (dense ids in the
 * reference's G.nodes() order; NULL ok).                                    */
int gw_graph_export_csr(const gw_graph* g, int64_t* offsets, int32_t* nbrs,
                        double* weights, int64_t* labels, int32_t* node_order);
/* totals[n]: the per-vertex weight totals gw_simrank_weighted divides by.
 * JAVA_WGRAPH: the sum of a vertex's distinct-neighbour weights in ascending
 * id order (WeightedSimRank.java:72-79 sums a HashMap's values; its iteration
 * order is not reproduced, the difference is fp64 reassociation).  Weighted
 * NX_SIMPLE: the sum of the row's weights in row order.  Unweighted handle:
 * GW_ERR_STATE.                                                             */
int gw_graph_export_weight_totals(const gw_graph* g, double* totals);
int gw_graph_free(gw_graph* g);

/* Options of this handle (defaults: all zero, listed = -1); opt NULL resets
 * the defaults.  Take effect at the next call that uses them.               */
int gw_graph_set_options(gw_graph* g, const gw_options_t* opt);
int gw_graph_get_options(const gw_graph* g, gw_options_t* opt);

/* Upload CSR (+degree, weight sums) to HBM of `device`.                     */
int gw_graph_to_device(gw_graph* g, int device);

/* ---- node2vec (H1) ------------------------------------------------------- */
/* Replaces Graph.preprocess_transition_probs (node2vec.py:83-113): builds the
 * alias tables on the GPU (alias_setup node2vec.py:116-147, get_alias_edge
 * :61-81).  mode GW_N2V_REPLAY builds per-edge tables (bit-exact with the
 * reference); GW_N2V_REJECTION builds only what rejection sampling needs.   */
int gw_n2v_prepare(gw_graph* g, double p, double q, int mode);
/* Copy the alias tables back (node2vec.py:112-113 alias_nodes/alias_edges):
 * node_J/node_q [nnz] in CSR slot order; edge_off [nnz+1], edge_J/edge_q
 * [edge_alias_entries] (REPLAY only; pass NULL to skip).                    */
int gw_n2v_export_alias(const gw_graph* g, int32_t* node_J, double* node_q,
                        int64_t* edge_off, int32_t* edge_J, double* edge_q);
/* Copy the per-slot tables of GW_N2V_BITSET, or of GW_N2V_REJECTION's listed
 * entries, back to host memory, unchanged (for tests that decode them):
 * entries [nnz x 64 B] in CSR slot order; region (NULL to skip) the region
 * pool, (sampler_bytes - 64 nnz) / 4 words in GW_N2V_BITSET mode, the one
 * placeholder word of a listed build.  GW_ERR_STATE when no such tables are
 * resident (not prepared, REPLAY, rejection without listed entries, p = q = 1,
 * weighted or directed graphs).                                             */
int gw_n2v_export_bitset(const gw_graph* g, void* entries, uint32_t* region);
/* Standalone alias_setup (node2vec.py:116-147) of one distribution on the
 * GPU: J[K], q[K] (J as int64 like np.int).                                 */
int gw_alias_setup(int device, const double* probs, int64_t K, int64_t* J,
                   double* q);

/* Exact reference replay of Graph.simulate_walks/node2vec_walk
 * (node2vec.py:13-59) for nwalks walks whose start vertices (dense ids, the
 * shuffled orders concatenated iteration-major) are given, consuming the
 * caller's uniform stream (np.random.rand() values in draw order, 2 per
 * step).  Host buffers: out_walks[nwalks*walk_len] (dense ids, -1 padded),
 * out_len[nwalks]; *uniforms_used = values consumed.  Requires
 * gw_n2v_prepare(..., GW_N2V_REPLAY).                                        */
int gw_n2v_walks_replay(gw_graph* g, int walk_len, int64_t nwalks,
                        const int32_t* starts, const double* uniforms,
                        int64_t n_uniforms, int32_t* out_walks, int32_t* out_len,
                        int64_t* uniforms_used);

/* Scale-mode walks (GW_N2V_REJECTION or REPLAY tables), device-resident.
 * Global walk index w in [walk_begin, walk_begin+walk_count): iteration
 * it = w / n, start = node_order[perm_it(w % n)] (shuffle != 0; perm is the
 * keyed Feistel bijection) or node_order[w % n] (shuffle == 0).  Output
 * row-major [walk_count][walk_len] dense ids (-1 padded), lens optional.
 * counters_dev (optional, 2 x uint64): += steps taken, += rejection trials. */
int gw_n2v_walks(gw_graph* g, int walk_len, uint64_t seed, int64_t walk_begin,
                 int64_t walk_count, int shuffle, int32_t* out_walks_dev,
                 int32_t* out_len_dev, uint64_t* counters_dev, void* stream);

/* Host-buffer form of gw_n2v_walks (stages through HBM in ~1 GB chunks and
 * synchronises): out_walks[walk_count*walk_len], out_len[walk_count] (NULL
 * ok), counters[2] (NULL ok).  For JNI / CLI callers.                       */
int gw_n2v_walks_host(gw_graph* g, int walk_len, uint64_t seed,
                      int64_t walk_begin, int64_t walk_count, int shuffle,
                      int32_t* out_walks, int32_t* out_len, uint64_t* counters);

/* ---- TopSim (H2) ------------------------------------------------------------ */
/* Allocate the per-workgroup workspace for up to `sample`/`step` (kept in the
 * handle; sizes the level arrays and the accumulator rows).                 */
int gw_topsim_prepare(gw_graph* g, int variant, int sample, int step, int topk);
/* Name of the kernel the handle's prepared TopSim workspace launches (e.g.
 * "k_topsim_pipe<5>", "k_topsim_2wg<5, 2>", "k_topsim_pipe_row<5>"; "" before
 * the first gw_topsim_prepare / gw_topsim* call).  Diagnostic: the choice
 * depends on V, SAMPLE and STEP (no reference counterpart).                 */
const char* gw_topsim_kernel(const gw_graph* g);
/* Kernel launches the last gw_topsim / gw_topsim_dense / gw_topsim_sparse
 * call on this handle made: 1, or 2 when a heavy source's partition filled
 * and the launch was re-run without the append path (0 before the first call
 * and after a call with no sources).  The host-buffer forms (gw_topsim_host,
 * gw_topsim_write_text) report their last batch.                            */
int gw_topsim_last_launches(const gw_graph* g);
/* Registers per lane, private segment (scratch) bytes per lane and LDS bytes
 * per workgroup (static + dynamic) of that kernel (hipFuncGetAttributes).   */
int gw_topsim_kernel_attrs(gw_graph* g, int32_t* vgprs, int32_t* scratch_bytes, int32_t* lds_bytes);
/* Replaces new TopSim_singleSample(g, sample, step).compute() +
 * Print.printByOrder's per-row FixedMaxPQ (TopSim_singleSample.java:35-54,
 * Print.java:25-53) for the given sources: out_ids_dev[nsrc*topk],
 * out_scores_dev[nsrc*topk], rows sorted by score desc then id asc, padded
 * with (-1, 0.0).  Scores are NOT divided by sample for SINGLE_SAMPLE /
 * ENUMERATE (as the reference); SINGLE_RW divides (SingleRandomWalk.java:89).
 * C: decay (MyConfiguration.C = 0.6).  stats_dev (optional, 4 x int64):
 * gw_topsim_stats_t accumulated on the device.                              */
int gw_topsim(gw_graph* g, int variant, int sample, int step, double C,
              uint64_t seed, const int32_t* sources_dev, int64_t nsrc, int topk,
              int32_t* out_ids_dev, double* out_scores_dev, int64_t* stats_dev,
              void* stream);
/* Dense rows for small graphs (getResult(), TopSim_singleSample.java:235):
 * out_rows_dev[nsrc*n] doubles, row r = sim[sources[r]][*], diagonal 0.     */
int gw_topsim_dense(gw_graph* g, int variant, int sample, int step, double C,
                    uint64_t seed, const int32_t* sources_dev, int64_t nsrc,
                    double* out_rows_dev, int64_t* stats_dev, void* stream);

/* Sparse rows, the input of the Java-exact writer at any V (Print.java:25-53
 * needs every nonzero score of a row, not only its top k): per source r its
 * nonzero entries sim[sources[r]][id] > 0, in no particular order, at
 * out_ids_dev / out_scores_dev[row_begin_dev[r] .. + row_len_dev[r]).  Rows
 * are packed at offsets claimed in completion order, up to `capacity`
 * entries; *used_dev (one int64, zeroed by the call) ends as the room ALL rows
 * needed.  A row that did not fit gets row_begin = row_len = -1 and the call
 * returns GW_ERR_CAPACITY (re-run with capacity >= *used).  Same walks, sums
 * and stats as gw_topsim; synchronises the stream.                          */
int gw_topsim_sparse(gw_graph* g, int variant, int sample, int step, double C,
                     uint64_t seed, const int32_t* sources_dev, int64_t nsrc,
                     int64_t capacity, int64_t* row_begin_dev,
                     int32_t* row_len_dev, int32_t* out_ids_dev,
                     double* out_scores_dev, int64_t* used_dev,
                     int64_t* stats_dev, void* stream);
/* new TopSim_singleSample(g, sample, step).compute() followed by
 * Print.printByOrder(sim, path, topk, ...) (TopSim_singleSample.java:47-54,
 * Print.java:25-53) for the given sources (host array), Java-exact at any V:
 * batches of sparse rows replayed through FixedMaxPQ on the host, rows
 * written in source order.  Writes path and path+".sim.txt" (sep, %.<decimals>f);
 * stats[4] optional.                                                        */
int gw_topsim_write_text(gw_graph* g, int variant, int sample, int step,
                         double C, uint64_t seed, const int32_t* sources,
                         int64_t nsrc, int topk, const char* path,
                         const char* sep, int decimals, int64_t* stats);

/* Host-buffer form of gw_topsim / gw_topsim_dense for JNI and C++ callers:
 * sources[nsrc] on the host; either out_rows[nsrc*n] (dense, getResult())
 * or out_ids/out_scores[nsrc*topk] (top-k); stats[4] optional.            */
int gw_topsim_host(gw_graph* g, int variant, int sample, int step, double C,
                   uint64_t seed, const int32_t* sources, int64_t nsrc,
                   int topk, int32_t* out_ids, double* out_scores,
                   double* out_rows, int64_t* stats);

/* ---- bounded-memory variants with FixedCacheMap (§8f-3) -------------------- */
/* Replaces new TopSim_singleSample_M(g, M, sample).compute() (variant
 * GW_TOPSIM_SINGLE_SAMPLE; TopSim_singleSample_M.java:33-239, the reference
 * fixes STEP = 5) and new SingleRandomWalk_M(g, M, sample).compute()
 * (GW_TOPSIM_SINGLE_RW; SingleRandomWalk_M.java:24-92): every pair update
 * (float)(... / SAMPLE) is put() into a lxctools.FixedCacheMap(capacity =
 * TOPK*M) in the reference's order (FixedCacheMap.java:32-50: add to a
 * present key, insert while not full, else replace the minimum when larger).
 * Per source r the map is then iterated (delMin, ascending) into
 * out_keys_dev/out_vals_dev[r*capacity + i], i < out_size_dev[r] (-1 / 0
 * padded).  Same Philox walks as gw_topsim.  capacity <= 4096.             */
int gw_topsim_m(gw_graph* g, int variant, int capacity, int sample, int step,
                double C, uint64_t seed, const int32_t* sources_dev, int64_t nsrc,
                int32_t* out_keys_dev, float* out_vals_dev, int32_t* out_size_dev,
                int64_t* stats_dev, void* stream);
/* Host-buffer form (synchronous).                                           */
int gw_topsim_m_host(gw_graph* g, int variant, int capacity, int sample,
                     int step, double C, uint64_t seed, const int32_t* sources,
                     int64_t nsrc, int32_t* out_keys, float* out_vals,
                     int32_t* out_size, int64_t* stats);

/* ---- double-walk variants (§8f-4) ------------------------------------------ */
/* kinds for gw_double_sim_host                                              */
#define GW_DOUBLE_SAMPLE 0      /* TopSim_doubleSample */
#define GW_DOUBLE_DEV 1         /* TopSim_Dev          */
#define GW_DOUBLE_RANDOM_WALK 2 /* DoubleRandomWalk    */
/* Replaces new TopSim_doubleSample(g, sample, step).compute() + getResult()
 * (TopSim_doubleSample.java:30-197): per vertex the TopSim BFS over `step`
 * levels, paths[src][target][s] = mass of the LAST queued path reaching
 * target at level s; sim[i][j] = sum_x sum_s C^s P[i][x][s] P[j][x][s]
 * (i < j, mirrored, diag 0).  sim_dev[n*n]; Philox keys as gw_topsim.       */
int gw_topsim_double(gw_graph* g, int sample, int step, double C,
                     uint64_t seed, double* sim_dev, void* stream);
/* Replaces new TopSim_Dev(g, sample, step, topK, singleStep).compute(cand)
 * (TopSim_Dev.java:31-95): SAMPLE = (int)((step-singleStep)*sample*2 /
 * (step*(topK+1))); for every i its candidates cand_dev[i*topK + r] (as
 * gw_select_fixed_max_pq gives them, -1 padded) are each freshly sampled
 * (Philox call 1 + i*topK + r) and sim[i][j] = getSim; other entries 0.    */
int gw_topsim_dev(gw_graph* g, int sample, int step, int topK, int singleStep,
                  double C, uint64_t seed, const int32_t* cand_dev,
                  double* sim_dev, void* stream);
/* Replaces new DoubleRandomWalk(g, sample, step).compute()
 * (DoubleRandomWalk.java:25-91): `sample` uniform walks of `step` steps per
 * vertex, sim[v][w] = sum over walk pairs of C^(t+1) at their first meeting
 * step t, / sample^2 (v < w, mirrored, diag 0).                            */
int gw_double_random_walk(gw_graph* g, int sample, int step, double C,
                          uint64_t seed, double* sim_dev, void* stream);
/* Host-buffer form of the three (kind = GW_DOUBLE_*): sim[n*n] on the host,
 * cand[n*topK] on the host for GW_DOUBLE_DEV (ignored otherwise).           */
int gw_double_sim_host(gw_graph* g, int kind, int sample, int step, int topK,
                       int singleStep, double C, uint64_t seed,
                       const int32_t* cand, double* sim);
/* TopSim_Dev's candidate choice (TopSim_Dev.java:64-71): per row a
 * FixedMaxPQ(k) offered every (j, rows[r][j] >= min_score) in j order, then
 * sortedElement() -> out_ids[r*k + i] (-1 padded).  Host code.             */
int gw_select_fixed_max_pq(const double* rows, int64_t nrows, int64_t n, int k,
                           double min_score, int32_t* out_ids);
/* Java's Double.toString of v (string concatenation "" + v), as
 * Eval.precision writes its scores (Eval.java:118, :128): shortest round-trip
 * digits, plain for 1e-3 <= |v| < 1e7 (at least one fraction digit), else
 * "d.dddE[-]n".  NUL-terminated into buf[buflen]; GW_ERR_RANGE if too small. */
int gw_format_java_double(double v, char* buf, int64_t buflen);

/* ---- naive SimRank (TopSim ground truth) ------------------------------------ */
/* Replaces new SimRank(g).compute() + getResult() (SimRank.java:21-57, 79):
 * S := I; `iters` rounds (the reference's STEP = 3) of
 *   S'[v][w] = C * sum_{a in N(v), b in N(w)} S[a][b] / (deg(v)*deg(w)),
 * S'[v][v] = 1, 0 for isolated v or w; then diag := 0 (postProcess, :62-65).
 * sim_dev: n*n doubles row-major on the graph's device (symmetric).  Needs an
 * undirected graph (Java multigraph: duplicate entries count).  The n*n fp64
 * workspace is kept in the handle.  fp64 result equals the reference up to
 * summation order (tested at rtol 1e-12).                                   */
int gw_simrank_naive(gw_graph* g, double C, int iters, double* sim_dev,
                     void* stream);
/* Host-buffer form (synchronous): sim[n*n].                                 */
int gw_simrank_naive_host(gw_graph* g, double C, int iters, double* sim);

/* ---- weighted SimRank --------------------------------------------------------- */
/* Replaces new WeightedSimRank(wg).compute() + getResult()
 * (simrank/weighted/WeightedSimRank.java:25-58, 95; the reference's STEP = 50):
 * S := I; `iters` rounds of
 *   S'[v][w] = C * sum_{a in adjs(v), b in adjs(w)} wt(v,a) wt(w,b) S[a][b]
 *              / (T[v] * T[w]),
 * S'[v][v] = 1, 0 when v or w has no adjacency entry; then diag := 0.  wt is
 * the handle's weight per adjacency entry, T its per-vertex total
 * (gw_graph_export_weight_totals).  No guards: totals that are 0 give NaN or
 * +-Inf as IEEE arithmetic does, and they propagate (:92).  Accepts
 * JAVA_WGRAPH handles and undirected weighted NX_SIMPLE handles; an
 * unweighted handle is GW_ERR_UNSUPPORTED (use gw_simrank_naive), a directed
 * one GW_ERR_UNSUPPORTED, iters < 0 GW_ERR_INVALID, a handle that is not on a
 * device GW_ERR_STATE.  sim_dev: n*n doubles row-major on the graph's device,
 * symmetric.  The fp64 workspace (two m*m matrices at most, m = vertices with
 * an adjacency entry) is kept in the handle.  gw_options_t.simrank_hbm_row and
 * simrank_window apply as they do to gw_simrank_naive.                       */
int gw_simrank_weighted(gw_graph* g, double C, int iters, double* sim_dev,
                        void* stream);
/* Host-buffer form (synchronous): sim[n*n].                                 */
int gw_simrank_weighted_host(gw_graph* g, double C, int iters, double* sim);
/* The same two-pass sparse evaluation in fp64 on the host (OpenMP, nthreads
 * <= 0: the runtime's default): entry order within a row, rows ascending.
 * Needs no device.  Equal to the kernel up to summation order, not bit for
 * bit.  sim[n*n].                                                           */
int gw_simrank_weighted_ref(const gw_graph* g, double C, int iters, int nthreads,
                            double* sim);
/* Registers per lane, scratch bytes per lane and static LDS bytes of the four
 * instantiations of the weighted gather kernel, in the order (LDS row, pass
 * 1), (HBM row, pass 1), (LDS row, pass 2), (HBM row, pass 2)
 * (hipFuncGetAttributes on the graph's device; any output may be NULL).      */
int gw_simrank_weighted_kernel_attrs(gw_graph* g, int32_t vgprs[4], int32_t scratch_bytes[4],
                                     int32_t lds_bytes[4]);

/* ---- output writers (host) ------------------------------------------------ */
/* DeepSim save_list format (DeepSim/src/main.py:237-243): one walk per line,
 * every label followed by '\t', then '\n'.  walks: dense ids (-1 padded).   */
int gw_write_walks_text(const gw_graph* g, const char* path,
                        const int32_t* walks, const int32_t* lens,
                        int64_t nwalks, int walk_len);
/* Print.printByOrder format (Print.java:25-53): per row "v,id,id,...\r\n" to
 * path and "v,id:%.6f,...\r\n" to path+".sim.txt".  Rows come from dense
 * score rows (java_exact: emulate FixedMaxPQ/PriorityQueue tie order and
 * Java's HALF_UP %.6f exactly) given as [nrows][n] host doubles.            */
int gw_write_sim_text_dense(const char* path, const double* rows,
                            const int32_t* row_ids, int64_t nrows, int64_t n,
                            int topk, const char* sep, int decimals);
/* Same format from sparse rows (gw_topsim_sparse, copied to the host): row r
 * = sim[row_ids[r]][*] with the listed nonzero entries and 0.0 elsewhere
 * (n columns).  FixedMaxPQ(topk) is replayed exactly — the first min(topk, n)
 * ids fill the heap (zero scores included), later offers enter only when
 * strictly larger than the heap minimum — and written in sortedElement()
 * order: min(topk, n) entries per row, byte-identical to
 * gw_write_sim_text_dense on the same rows.                                */
int gw_write_sim_text_sparse(const char* path, const int64_t* row_begin,
                             const int32_t* row_len, const int32_t* ids,
                             const double* scores, const int32_t* row_ids,
                             int64_t nrows, int64_t n, int topk,
                             const char* sep, int decimals);
/* Same format from top-k rows as produced by gw_topsim (score desc, id asc,
 * -1 padding dropped).  NOT Java-exact: a top-k row carries neither the
 * zero-score ids FixedMaxPQ keeps when a row has fewer than topk nonzeros
 * nor the heap history that orders ties; use gw_write_sim_text_sparse /
 * gw_topsim_write_text for the reference's bytes.                          */
int gw_write_sim_text_topk(const char* path, const int32_t* ids,
                           const double* scores, const int32_t* row_ids,
                           int64_t nrows, int topk, const char* sep,
                           int decimals);

/* Print.printByOrder(FixedCacheMap[] sim, outPath, topk) (Print.java:94-124):
 * per row the last `topk` entries of the ascending iteration, "%.6f" of the
 * float values; rows as produced by gw_topsim_m.                            */
int gw_write_sim_text_cachemap(const char* path, const int32_t* keys,
                               const float* vals, const int32_t* sizes,
                               const int32_t* row_ids, int64_t nrows,
                               int capacity, int topk, const char* sep);

/* ---- embeddings: skip-gram with negative sampling ---------------------------- */
/* Replaces learn_embeddings (node2vec/src/main.py:92-101; DeepSim/src/
 * main.py:215-216): Word2Vec(walks, size, window, min_count=0, sg=1, iter)
 * and save_word2vec_format, trained on the walk matrix gw_n2v_walks writes
 * (int32 dense ids, -1 padded; a walk ends at its first -1).  The law is
 * gensim's sg=1, hs=0, negative=K training made counter-based
 * (csrc/gw_sgns_law.h holds the one definition host and kernel share):
 *   vocabulary  cnt[v] = occurrences of v, every vertex that occurs is kept;
 *   subsampling keep probability min(1, (sqrt(cnt/(sample*T)) + 1) *
 *               (sample*T)/cnt), T = sum cnt (sample = 0: keep all), computed
 *               in fp64 on the host and stored as floor(p * 2^32)
 *               (0xFFFFFFFF = always); a token is kept iff its word < it;
 *   negatives   P(v) ~ cnt[v]^0.75 (fp64 on the host), Vose alias table with
 *               q stored as floor(q * 2^32); a draw from Philox words (x, y)
 *               is k = (x * n) >> 32, t = y < thr[k] ? k : J[k]; a negative
 *               equal to the centre word is skipped;
 *   windows     per kept token i of a walk's kept sequence s: b = y % window;
 *               for j in [i-window+b, i+window-b], j != i, ascending: the pair
 *               (input row syn0[s[j]]; target s[i] with label 1, then the K
 *               negatives with label 0);
 *   target      f = dot(l1, syn1neg[t]); |f| >= 6 skips it; else g = (label -
 *               expTable[int((f+6)*(1000/12))]) * alpha; neu1e += g*syn1neg[t];
 *               syn1neg[t] += g*l1; after a pair's targets syn0[s[j]] += neu1e;
 *   alpha(e,w)  alpha - (alpha - min_alpha) * (e*nwalks + w) / (epochs*nwalks)
 *               in fp64, cast to fp32 (e = epoch, w = walk index);
 *   initial     syn0[v][d] = (u - 0.5) / dim, syn1neg = 0.
 * Philox4x32-10 keying (k0 = seed low, k1 = seed high ^ tag; never the launch
 * geometry), w = global walk index, pos = position in the walk as given:
 *   token    tag "sgT0": counter (w low, w high, pos, epoch) -> x: subsampling
 *            word, y: window word;
 *   negative tag "sgN0": counter (w low, w high, centre pos, epoch << 20 |
 *            slot << 9 | k), slot = j - (i - window) in [0, 2*window], k the
 *            negative's index in [0, K) -> (x, y) of the alias draw;
 *   initial  tag "sgI0": counter (v, 0, d, 0) -> x, u = x * 2^-32.
 * Hence window <= 1023, negative <= 511, epochs <= 4096, walk_len <= 2^20
 * (the kernel: walk_len <= 2048, its kept sequence lives in LDS).
 * Sequential order: epochs, walks, positions, pairs, targets ascending; a
 * dot product sums 64 lane-strided partials (16 B chunks) and then a fixed
 * butterfly; the host evaluation (device = -1) runs the same order, so it
 * equals the kernel at concurrency = 1 bit for bit (tested).               */
typedef struct gw_sgns gw_sgns;
typedef struct gw_sgns_params_t {
  int32_t struct_size; /* sizeof(gw_sgns_params_t) as the caller compiled it:
                          min(struct_size, the library's size) bytes are read,
                          the rest keeps the defaults below                    */
  int32_t dim;         /* 1..1024 (default 128)                                 */
  int32_t window;      /* 1..1023 (5)                                           */
  int32_t negative;    /* 0..511 (5)                                            */
  int32_t epochs;      /* 1..4096: the schedule's length (5)                    */
  int32_t reserved0;   /* 0                                                     */
  double alpha;        /* 0.025                                                 */
  double min_alpha;    /* 0.0001                                                */
  double sample;       /* 1e-3; 0 disables subsampling                          */
  uint64_t seed;       /* 0                                                     */
} gw_sgns_params_t;
typedef struct gw_sgns_stats_t {
  int64_t tokens_kept;      /* tokens that survived subsampling                */
  int64_t pairs;            /* (input, centre) pairs trained                   */
  int64_t negatives;        /* negatives drawn (K per pair)                    */
  int64_t negatives_centre; /* of those, skipped as equal to the centre word   */
  int64_t targets_clipped;  /* targets skipped at |f| >= 6                     */
} gw_sgns_stats_t;
/* device >= 0: a GPU; device = -1: host evaluation of the same law (no GPU
 * needed; walks are then host pointers).  params NULL = the defaults.  n =
 * vertices (ids in [0, n)).                                                 */
int gw_sgns_create(int device, int64_t n, const gw_sgns_params_t* params, gw_sgns** out);
int gw_sgns_free(gw_sgns* m);
/* message of the last failing call on this handle (NULL: the last failing
 * handle-less call on this thread, as gw_last_error(NULL))                   */
const char* gw_sgns_last_error(const gw_sgns* m);
/* Counts, keep thresholds, alias sampler, exp table and the initial syn0 /
 * syn1neg (the histogram and the initialisation run on the device).  An id
 * outside [0, n) (other than the -1 padding) gives GW_ERR_RANGE.
 * Synchronous.                                                               */
int gw_sgns_build_vocab(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len);
/* Epochs [epoch_begin, epoch_begin + epoch_count) of params.epochs over the
 * corpus (the one build_vocab counted).  `concurrency` waves train at once,
 * Hogwild like gensim's workers: wave c takes walks c, c + concurrency, ...
 * of each epoch; 1 is exactly the sequential law.  0 = auto:
 * min(nwalks, 16 * compute units, max(1, n / 32)) - never more than one wave
 * per 32 vertices, so that rows are rarely trained by two waves at once.
 * Rows are loaded and stored with 16 B agent-scope (sc1) accesses, so a wave
 * never trains against a copy older than the L2 / memory holds.  The draws
 * do not depend on concurrency.  stats (optional) += this call's counts.
 * Runs on `stream` and synchronises it.  GW_ERR_STATE before build_vocab.    */
int gw_sgns_train(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len, int epoch_begin,
                  int epoch_count, int concurrency, gw_sgns_stats_t* stats, void* stream);
/* Host copies: syn0[n*dim], syn1neg[n*dim] (dense rows), counts[n]; NULL skips */
int gw_sgns_export(gw_sgns* m, float* syn0, float* syn1neg, int64_t* counts);
/* The negative sampler and the keep thresholds: J[n], thr[n], keep_thr[n]   */
int gw_sgns_sampler_export(const gw_sgns* m, int32_t* J, uint32_t* thr, uint32_t* keep_thr);
/* syn0 where it lives (HBM of the handle's device, or host memory at device
 * = -1): row v at ptr + v * pitch floats, dim used (zero-copy for torch)     */
int gw_sgns_vectors_dev(gw_sgns* m, float** ptr, int64_t* pitch);
/* concurrency an auto (0) gw_sgns_train call over nwalks walks uses          */
int gw_sgns_auto_concurrency_for(const gw_sgns* m, int64_t nwalks, int32_t* concurrency);
/* Registers per lane, scratch bytes per lane (expected 0) and LDS bytes per
 * workgroup of the training kernel this handle launches for walk_len
 * (hipFuncGetAttributes).                                                    */
int gw_sgns_kernel_attrs(gw_sgns* m, int walk_len, int32_t* vgprs, int32_t* scratch_bytes, int32_t* lds_bytes);
/* save_word2vec_format(path) (main.py:99): "<V'> <dim>\n", V' = vertices with
 * counts > 0, then one row per such vertex "<label> v v ... v\n" (%f, single
 * spaces), by count descending, ties by label ascending (gensim's own tie
 * order follows its vocabulary dict's iteration order, which is arbitrary
 * under the Python the reference ran on).  syn0[n*dim] host rows, labels NULL
 * = dense ids.                                                               */
int gw_write_word2vec_text(const char* path, const float* syn0, const int64_t* counts, const int64_t* labels,
                           int64_t n, int dim);

/* ---- embeddings: DeepSim (SimRank-guided one-hidden-layer net) --------------- */
/* Replaces DeepSim.main (DeepSim/src/DeepSim.py:386-422): per step a batch of
 * `batch` distinct walks, one centre position each, targets y[j] = sim(c, j)
 * for the distinct vertices j of the centre's window (2*window+1 tokens);
 *   hidden = relu(w1[c] + b1), logits = hidden . w2 + b2,
 *   loss = mean_b( -sum_j y[b][j] * log softmax(logits[b])[j] ),
 * TF1 Adam (lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = step + 1) dense
 * over w1 [V][dim], b1 [dim], w2 [dim][V], b2 [V]; the embedding is w1.
 * csrc/gw_deepsim_law.h holds the one definition (draws, float order) that
 * the kernels and the host evaluation (device = -1) share; they agree bit for
 * bit (tested).  Everything is in vertex-index space [0, V): the row numbers
 * of the .sim.txt.  Philox4x32-10 keying (k0 = seed low, k1 = seed high ^ tag):
 *   walk     tag "dsP0": slot s of step t takes eligible[gw_feistel_perm(s,
 *            n_eligible, k0 ^ t high, k1, tweak = t low)];
 *   position tag "dsB0": counter (t low, t high, s, 0) -> x,
 *            pos = window + ((x * (len - 2*window)) >> 32);
 *   initial  tag "dsI0": counter (index low, index high, tensor, attempt),
 *            tensor 0 = w1, 2 = w2; Box-Muller in fp64 on u1 = (x+1) * 2^-32,
 *            u2 = y * 2^-32, redrawn (attempt + 1) while |z| > 2; 0.1 * z.
 * Device path: dim and batch multiples of 32 in [32, 128], window <= 64,
 * topk <= 1024 (else GW_ERR_UNSUPPORTED); the host path takes any positive
 * values.  HBM: 24 * V * dim + 12 * (V + dim) bytes of parameters and Adam
 * state, 4 * V * dim for the w1 gradient rows, 4 * batch * V logits,
 * 4 * ceil(V / 64) * batch * (dim + 2) of per-tile partials and the table's
 * 8 * V * topk.                                                               */
#define GW_DEEPSIM_FALLBACK_ROW_MIN 0  /* absent id: tem[centre] (get_input_output :242-245) */
#define GW_DEEPSIM_FALLBACK_POSITION 1 /* absent id: tem[pos] (get_batch :319 read literally) */
typedef struct gw_deepsim gw_deepsim;
typedef struct gw_deepsim_params_t {
  int32_t struct_size;  /* as gw_sgns_params_t.struct_size                        */
  int32_t dim;          /* 128                                                    */
  int32_t window;       /* 10                                                     */
  int32_t batch;        /* 128                                                    */
  int32_t fallback;     /* GW_DEEPSIM_FALLBACK_ROW_MIN                            */
  int32_t reserved0;    /* 0                                                      */
  int64_t vertex_num;   /* V (required)                                           */
  double learning_rate; /* 0.001                                                  */
  double beta1;         /* 0.9                                                    */
  double beta2;         /* 0.999                                                  */
  double epsilon;       /* 1e-8                                                   */
  double score_scale;   /* 1.0; 1 / SAMPLE turns gw_topsim scores into SimRank    */
  uint64_t seed;        /* 0                                                      */
} gw_deepsim_params_t;
/* device >= 0: a GPU; -1: the host evaluation.  Initialises w1, w2 (biases and
 * Adam state 0).                                                               */
int gw_deepsim_create(int device, const gw_deepsim_params_t* params, gw_deepsim** out);
int gw_deepsim_free(gw_deepsim* m);
const char* gw_deepsim_last_error(const gw_deepsim* m);
/* The SimRank table: ids[V][topk] (-1 padded) and fp64 scores[V][topk] in the
 * order gw_topsim / the .sim.txt give them (score descending); device pointers
 * for device >= 0, host pointers for device = -1.  Scores are multiplied by
 * score_scale, entries <= 1e-8 are dropped, tem[v] = the last kept value in
 * that order (0 for an empty row), rows are then sorted by id, values stored
 * as fp32.  The build itself runs on the host (one copy each way).  An id
 * outside [-1, V) gives GW_ERR_RANGE.  Synchronous.                           */
int gw_deepsim_set_simrank(gw_deepsim* m, const int32_t* ids, const double* scores, int topk);
/* The walk matrix [nwalks][walk_len] (int32, -1 padded; device memory for
 * device >= 0) stays where it is and must outlive the training calls; only
 * the list of eligible walks (len >= 2*window+1) is built.  labels (host,
 * [n_labels] or NULL = identity) maps a token to its vertex index; a token
 * outside [0, n_labels) or a mapped one outside [0, V) gives GW_ERR_RANGE.
 * Fewer eligible walks than `batch` gives GW_ERR_INVALID.  Synchronous.       */
int gw_deepsim_set_walks(gw_deepsim* m, const int32_t* walks, int64_t nwalks, int walk_len, const int64_t* labels,
                         int64_t n_labels);
/* Steps [step_begin, step_begin + step_count); pieces equal one call.
 * loss_out[step_count] (host, optional): each step's loss before its update.
 * Runs on `stream` and synchronises it.                                       */
int gw_deepsim_train(gw_deepsim* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream);
/* Gradient of step's batch at the current parameters (host copies, NULL
 * skips): gw1[V*dim], gb1[dim], gw2[dim*V], gb2[V].  Nothing is updated.      */
int gw_deepsim_gradients(gw_deepsim* m, int64_t step, float* gw1, float* gb1, float* gw2, float* gb2);
/* Host copies of step's batch: centre[batch], tgt_id / tgt_val
 * [batch][2*window+1] (the first tgt_n[b] of a row are used, the rest -1 / 0),
 * tgt_n[batch], ysum[batch].  NULL skips.                                     */
int gw_deepsim_batch(gw_deepsim* m, int64_t step, int32_t* centre, int32_t* tgt_id, float* tgt_val, int32_t* tgt_n,
                     float* ysum);
/* Host copies, reference shapes (NULL skips): par / adam_m / adam_v each
 * {w1[V*dim], b1[dim], w2[dim*V], b2[V]}.                                     */
int gw_deepsim_export(gw_deepsim* m, float* const par[4], float* const adam_m[4], float* const adam_v[4]);
/* w1 where it lives: row v at ptr + v * pitch floats                          */
int gw_deepsim_vectors_dev(gw_deepsim* m, float** ptr, int64_t* pitch);
/* Per kernel of the step chain (up to `cap`): name, registers per lane,
 * scratch bytes per lane, LDS bytes per workgroup; *count = kernels.          */
int gw_deepsim_kernel_attrs(gw_deepsim* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                            int32_t* lds_bytes, int32_t* count);
/* save_embeddings (DeepSim.py:344-362): "<n> <dim>\n" (the reference writes
 * the literal 128), then "<i> v v ... v\n" per row, each value as
 * str(numpy.float32) prints it (shortest round-trip digits; positional for
 * 1e-4 <= |x| < 1e16, else scientific with a two-digit exponent).             */
int gw_write_deepsim_text(const char* path, const float* w1, int64_t n, int dim);

/* ---- embeddings: SDNE (four-layer dense autoencoder) -------------------------- */
/* Replaces SDNE (SDNE/SDNE.py:66-176).  units = {u0, u1, u2, u3, u4}, u4 = u0;
 * rows of width u0, dense or sparse (a graph's adjacency, top-k rows):
 *   h1 = relu(x . w1 + b1), z2 = h1 . w2 + b2 (the embedding, before the relu),
 *   h2 = relu(z2), h3 = relu(h2 . w3 + b3), y = h3 . w4 + b4,
 *   loss = sum((y - x)^2) / 2 / batch + weight_decay * sum_theta sum(theta^2) / 2
 *          + kl_weight * KL(kl_target || mean(h2)),
 * TF1 Adam (lr_t as gw_deepsim) dense over all eight tensors.  Step t trains on
 * rows [(t mod nb) * batch, +batch), nb = floor(N / batch): the last N mod batch
 * rows are never trained on but are encoded.  Three options, all off by default
 * (the reference's law), make it the SDNE paper's loss for graphs:
 *   nonzero_weight (beta): the reconstruction term weighs an entry with x != 0
 *            by beta^2: sum(w * (y - x)^2) / 2 / batch;
 *   first_order (alpha): adds (alpha / batch) * sum over rows i, j of the batch
 *            of a_ij * |z2_i - z2_j|^2, a_ij = x_i[row(j)]: the rows must be a
 *            square matrix (N = u0), else set_rows_* gives GW_ERR_INVALID;
 *   shuffle: slot s = (t mod nb) * batch + i of epoch e = t / nb trains on row
 *            perm_e(s), a keyed permutation of all N rows (tag "sdP0", iteration
 *            e), so every row is trained on and edges fall inside batches;
 *            gw_sdne_batch_rows names a step's rows.  Encodings stay in row order.
 * csrc/gw_sdne_law.h holds the one definition (float order, draws) that the
 * kernels and the host evaluation (device = -1) share; they agree bit for bit
 * (tested).  Every product reduces in chunks of 128 along its reduction index:
 * an fmaf chain per chunk (chunk 0 from the bias, or +0 backward), the chunks
 * added in ascending order.  Philox4x32-10 keying as gw_deepsim:
 *   initial  tag "sdI0": counter (index low, index high, tensor, attempt),
 *            tensor 0, 2, 4, 6 = w1..w4; truncated normal, stddev 0.1.
 * Device path: u1, u2, u3 <= 1024 and batch <= 128 (else GW_ERR_UNSUPPORTED);
 * u0 is bounded by memory; the host path takes any positive values.  HBM:
 * 12 bytes per parameter (value and Adam moments), 12 * batch * (u0 + u1 + u2
 * + u3) of activations and their gradients, 4 * ceil(u0 / 128) * batch *
 * max(u1, u3) of chunk partials when u0 > 512, and 4 * N * u2 for the encoding. */
typedef struct gw_sdne gw_sdne;
typedef struct gw_sdne_params_t {
  int32_t struct_size;  /* as gw_sgns_params_t.struct_size                        */
  int32_t units[5];     /* {u0 (required), 400, 100, 300, u4 (0 = u0)}            */
  int32_t batch;        /* 100                                                    */
  int32_t shuffle;      /* 0 (ordered batches); 1: a row permutation per epoch    */
  double learning_rate; /* 0.01                                                   */
  double beta1;         /* 0.9                                                    */
  double beta2;         /* 0.999                                                  */
  double epsilon;       /* 1e-8                                                   */
  double weight_decay;  /* 0.1                                                    */
  double kl_weight;     /* 0.1                                                    */
  double kl_target;     /* 0.005 (p)                                              */
  uint64_t seed;        /* 0                                                      */
  double nonzero_weight; /* 1.0 (beta; finite, > 0)                               */
  double first_order;   /* 0.0 (alpha; finite, >= 0)                              */
} gw_sdne_params_t;
/* device >= 0: a GPU; -1: the host evaluation.  Initialises w1..w4 (biases and
 * Adam state 0).  u4 != u0, a beta that is not finite and positive, an alpha
 * that is not finite and non-negative, or a shuffle outside {0, 1} give
 * GW_ERR_INVALID.  A struct_size that ends before a field leaves its default;
 * a zeroed struct of the full size must set nonzero_weight itself.             */
int gw_sdne_create(int device, const gw_sdne_params_t* params, gw_sdne** out);
int gw_sdne_free(gw_sdne* m);
const char* gw_sdne_last_error(const gw_sdne* m);
/* The rows: a dense fp32 matrix, row r at rows + r * pitch floats (device
 * memory for device >= 0).  It stays where it is and must outlive the calls
 * that read it.  n < batch gives GW_ERR_INVALID.  Replaces earlier rows.       */
int gw_sdne_set_rows_dense(gw_sdne* m, const float* rows, int64_t n, int64_t pitch);
/* The rows as CSR (host pointers, copied): offsets[n + 1], cols, vals (NULL =
 * 1).  A column outside [0, u0) gives GW_ERR_RANGE, a column twice in one row
 * GW_ERR_INVALID, n < batch GW_ERR_INVALID.  Replaces earlier rows.            */
int gw_sdne_set_rows_csr(gw_sdne* m, const int64_t* offsets, const int32_t* cols, const float* vals, int64_t n);
/* Steps [step_begin, step_begin + step_count); pieces equal one call.
 * loss_out[step_count] (host, optional): each step's loss before its update.
 * Runs on `stream` and synchronises it.                                       */
int gw_sdne_train(gw_sdne* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream);
/* The rows step trains on, in slot order, into rows[batch] (host), for either
 * setting of shuffle; a device handle stages the batch and reads the ids back. */
int gw_sdne_batch_rows(gw_sdne* m, int64_t step, int64_t* rows);
/* Gradient of step's batch at the current parameters (host copies, NULL
 * skips), weight decay included: grads = {w1[u0*u1], b1[u1], w2[u1*u2], b2,
 * w3[u2*u3], b3, w4[u3*u4], b4}.  Nothing is updated.                          */
int gw_sdne_gradients(gw_sdne* m, int64_t step, float* const grads[8]);
/* z2 of rows [row_begin, row_begin + row_count) of the current rows into the
 * handle's [N][u2] matrix and, when out is not NULL, into out[row_count][u2]
 * (host).                                                                      */
int gw_sdne_encode(gw_sdne* m, int64_t row_begin, int64_t row_count, float* out);
/* Host copies (NULL skips): par / adam_m / adam_v each in the order of
 * gw_sdne_gradients.                                                           */
int gw_sdne_export(gw_sdne* m, float* const par[8], float* const adam_m[8], float* const adam_v[8]);
/* The encoded [N][u2] matrix where it lives (HBM for device >= 0), complete
 * after an encode of all rows: row r at ptr + r * pitch floats.               */
int gw_sdne_vectors_dev(gw_sdne* m, float** ptr, int64_t* pitch);
/* As gw_deepsim_kernel_attrs.                                                  */
int gw_sdne_kernel_attrs(gw_sdne* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                         int32_t* lds_bytes, int32_t* count);

/* ---- scoring: one-vs-rest logistic regression, top-k prediction, F1 ---------- */
/* Replaces classify.scoring (node2vec/src/classify.py, DeepSim/src/classify.py):
 * TopKRanker(LogisticRegression(penalty='l2')) fitted one-vs-rest on a share of
 * the embedding rows, as many labels predicted per held-out row as it really
 * has, micro- and macro-F1.  csrc/gw_ovr_law.h holds the one definition the
 * kernels and the host evaluation (device = -1) share; they agree bit for bit
 * (tested).
 *   problem     per label c over the training rows T, x~ = (x, 1), s = +-1:
 *               f_c(w) = 1/2 w.w + C * sum_{i in T} log(1 + exp(-s_ic w.x~_i)),
 *               liblinear's primal L2 logistic regression as the reference's
 *               sklearn ran it (C = 1, bias regularised, intercept_scaling 1);
 *               the minimiser is unique.
 *   constant    a label with no positive, or no negative, training row is not
 *               fitted: its decision value is -inf / +inf (sklearn's
 *               _ConstantPredictor).
 *   arithmetic  features are the caller's fp32 widened, everything else fp64;
 *               only + - * /, sqrt and the law's own exp (range reduction by
 *               ln 2, degree-13 Taylor polynomial, all in explicit fma), built
 *               with -ffp-contract=off; no libm on either side.
 *   solver      Newton-CG from w = 0.  Per Newton step: CG on
 *               (I + C X~'DX~) s = -g from s = 0, stopped at |r| <= 0.1 |g| or
 *               after max_cg products; then w + alpha s, alpha = 1, 1/2, ...
 *               (at most 30 halvings) until |grad| decreases strictly - the
 *               merit is the gradient norm, so no logarithm is needed, and
 *               g.H s <= -0.9 |g|^2 makes a small step acceptable.  Stop:
 *               |grad f_c(w)| <= gtol * |grad f_c(0)|; a label that has not met
 *               it after max_newton accepted steps (or 30 halvings) is
 *               reported GW_OVR_NOT_CONVERGED.  All labels of a fit advance
 *               together through shared passes over the gathered rows (one
 *               pass = for every running label either the gradient at its
 *               trial point or one Hessian-vector product); a finished label
 *               is frozen, and no label's arithmetic reads another's, so a
 *               label fitted alone gives the same bits.
 *   sum orders  x~.v: fma over the dim columns ascending from +0, then + v[dim];
 *               coefficient * x~ summed over the rows of a block of 64 gathered
 *               rows ascending (fma from +0), blocks then added ascending; dot
 *               products over the dim + 1 entries ascending (fma from +0).
 *               Nothing depends on the grid.
 *   prediction  a row with k true labels gets the k labels of largest decision
 *               value w.x~ (not the sigmoid, which saturates); k = 0 predicts
 *               nothing; of equal values the larger label index wins, which is
 *               argsort()[-k:] under a stable sort (numpy's default sort
 *               promises no order among equals).
 *   counts      tp, fp, fn per label over the scored rows; micro = 2 sum tp /
 *               (2 sum tp + sum fp + sum fn); macro = mean over all labels of
 *               2 tp / (2 tp + fp + fn), 0 where that is 0 / 0.  (The
 *               reference's old sklearn averaged over the labels present in
 *               truth or prediction: form it from the same counts.)
 *   shuffle     order[i] = gw_feistel_perm(i, n, seed low ^ shuffle low,
 *               seed high ^ "ovS0", tweak = shuffle high); the reference's
 *               skshuffle is unseeded.
 * Device path: dim <= 1024 and labels <= 1024 (else GW_ERR_UNSUPPORTED); the
 * host path takes any size.  HBM of a fit over T rows: 17 * T * labels bytes
 * (y, z, D), 8 * ceil(T / 64) * labels * (dim + 1) of block partials.         */
#define GW_OVR_CONST_NEG 0     /* no positive training row: decision -inf      */
#define GW_OVR_CONST_POS 1     /* no negative training row: decision +inf      */
#define GW_OVR_FITTED 2        /* met the stop condition                       */
#define GW_OVR_NOT_CONVERGED 3 /* weights are the last accepted iterate        */
typedef struct gw_ovr gw_ovr;
typedef struct gw_ovr_params_t {
  int32_t struct_size; /* as gw_sgns_params_t.struct_size                      */
  int32_t dim;         /* columns read of a feature row (128)                  */
  int32_t labels;      /* L (required)                                         */
  int32_t max_newton;  /* accepted Newton steps per label (100)                */
  int32_t max_cg;      /* Hessian-vector products per Newton step (200)        */
  int32_t reserved0;   /* 0                                                    */
  double C;            /* 1.0                                                  */
  double gtol;         /* 1e-8                                                 */
  uint64_t seed;       /* 0: not used by the fit; kept for gw_ovr_order callers */
} gw_ovr_params_t;
typedef struct gw_ovr_stats_t {
  int64_t passes;        /* shared passes over the training rows               */
  int32_t fitted;        /* labels per final state                             */
  int32_t constant;
  int32_t not_converged;
  int32_t newton_max;    /* largest accepted-step count of a label             */
} gw_ovr_stats_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = rows of the feature matrix */
int gw_ovr_create(int device, int64_t n, const gw_ovr_params_t* params, gw_ovr** out);
int gw_ovr_free(gw_ovr* m);
const char* gw_ovr_last_error(const gw_ovr* m);
/* Row v at x + v * pitch floats (pitch >= dim): device memory for device >= 0,
 * read where it lies (zero-copy from gw_sgns_vectors_dev /
 * gw_deepsim_vectors_dev), host memory for device = -1.  It must outlive the
 * calls; only dim floats of a row are ever read.                             */
int gw_ovr_set_features(gw_ovr* m, const float* x, int64_t pitch);
/* Host CSR of the true labels: row v has ids[row_off[v] .. row_off[v + 1]),
 * distinct within a row.  An id outside [0, labels) gives GW_ERR_RANGE.       */
int gw_ovr_set_labels(gw_ovr* m, const int64_t* row_off, const int32_t* ids);
/* The law's permutation of [0, n) for (seed, shuffle) into order[n] (host)    */
int gw_ovr_order(uint64_t seed, uint64_t shuffle, int64_t n, int64_t* order);
/* Fits every label on the rows order[0 .. train_count) (host array),
 * 1 <= train_count <= n; a row outside [0, n) gives GW_ERR_RANGE, a repeated
 * one GW_ERR_INVALID.  stats is optional.  Runs on `stream` and synchronises
 * it.  GW_ERR_STATE before set_features and set_labels; a failing fit leaves
 * the handle unfitted.                                                        */
int gw_ovr_fit(gw_ovr* m, const int64_t* order, int64_t train_count, gw_ovr_stats_t* stats, void* stream);
/* Predicts rows[0 .. count) (host array, count >= 0) by the top-k rule and
 * counts on the device: counts[labels][3] = tp, fp, fn (host).  GW_ERR_STATE
 * before gw_ovr_fit.                                                          */
int gw_ovr_score(gw_ovr* m, const int64_t* rows, int64_t count, int64_t* counts, void* stream);
/* Host copy of the decision values z[count][labels] of rows (tests)           */
int gw_ovr_decision(gw_ovr* m, const int64_t* rows, int64_t count, double* z);
/* Host copies (NULL skips): W[labels][dim + 1] (bias last; 0 for a constant
 * label), state[labels] (GW_OVR_*), newton_iters[labels], gnorm[labels]
 * (the law's own |grad f_c(w)| at the returned weights).                      */
int gw_ovr_export(gw_ovr* m, double* W, int32_t* state, int32_t* newton_iters, double* gnorm);
/* Per kernel (up to `cap`): name, registers per lane, scratch bytes per lane,
 * LDS bytes per workgroup; *count = kernels.                                  */
int gw_ovr_kernel_attrs(gw_ovr* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                        int32_t* lds_bytes, int32_t* count);

/* ---- nearest neighbours of an embedding -------------------------------------- */
/* Replaces KeyedVectors.most_similar (DeepSim/src/main.py:287 loads the result
 * as KeyedVectors; cosine top-n) and IsoMap_LE/LE.py:53-60 knn: for every
 * source row the topk other rows of largest similarity, in gw_topsim's row
 * layout, so gw_write_sim_text_topk and topsim.precision read them as they are.
 * csrc/gw_knn_law.h holds the one definition the kernels and the host
 * evaluation (device = -1) share; they agree bit for bit (tested).
 *   arithmetic  features are the caller's fp32 widened, everything else fp64;
 *   dot(i,j)    fma over k = 0 .. dim-1 ascending from +0: no split-K, no
 *               reassociation, dot(i,j) and dot(j,i) have the same bits;
 *   nrm(i)      sqrt(dot(i,i)), correctly rounded;
 *   GW_KNN_DOT     s(i,j) = dot(i,j);
 *   GW_KNN_COSINE  s(i,j) = dot(i,j) / (nrm(i) * nrm(j)), one multiply and one
 *               divide; a row with nrm == 0 has no neighbours and is nobody's;
 *   row of v    the topk candidates j != v of largest s(v,j); a NaN score is
 *               never listed; score descending, then id ascending (a total
 *               order: nothing depends on tiles, grid or timing); a row with
 *               fewer listed candidates is padded with (-1, 0.0).
 * Device path: 1 <= dim <= 1024, 1 <= topk <= 128, n < 2^31 (else
 * GW_ERR_UNSUPPORTED); the host path takes any size.                          */
#define GW_KNN_COSINE 0
#define GW_KNN_DOT 1
typedef struct gw_knn gw_knn;
typedef struct gw_knn_params_t {
  int32_t struct_size; /* as gw_sgns_params_t.struct_size                      */
  int32_t dim;         /* columns read of a row (128)                          */
  int32_t topk;        /* entries per output row (20)                          */
  int32_t metric;      /* GW_KNN_COSINE (default) or GW_KNN_DOT                */
} gw_knn_params_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = rows of the matrix         */
int gw_knn_create(int device, int64_t n, const gw_knn_params_t* params, gw_knn** out);
int gw_knn_free(gw_knn* m);
const char* gw_knn_last_error(const gw_knn* m);
/* As gw_ovr_set_features: row v at x + v * pitch floats (pitch >= dim), device
 * memory for device >= 0 and read where it lies (zero-copy from
 * gw_sgns_vectors_dev / gw_deepsim_vectors_dev), host memory for device = -1.
 * It must outlive the queries; only dim floats of a row are ever read.
 * gw_knn_set_rows changes n for a handle that is used again on another matrix
 * (call it before gw_knn_set_vectors).                                        */
int gw_knn_set_vectors(gw_knn* m, const float* x, int64_t pitch);
int gw_knn_set_rows(gw_knn* m, int64_t n);
/* out_ids[r * topk + t] (int32) and out_scores[r * topk + t] (double) of the
 * source sources[r], r < nsrc.  sources, out_ids and out_scores are device
 * memory for device >= 0 and host memory for -1.  sources == NULL: all of
 * 0 .. n-1 (nsrc is ignored).  Sources may repeat, in any order.  nsrc == 0
 * returns GW_OK and does nothing.  A source outside [0, n) gives GW_ERR_RANGE
 * and nothing is written.  GW_ERR_STATE before gw_knn_set_vectors.  Runs on
 * `stream` and synchronises it.                                               */
int gw_knn_query(gw_knn* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_scores,
                 void* stream);
/* As gw_ovr_kernel_attrs                                                      */
int gw_knn_kernel_attrs(gw_knn* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                        int32_t* lds_bytes, int32_t* count);
/* Launch geometry of the main kernel (tests place their shapes on its edges):
 * tq source rows per workgroup, tc candidate rows per tile, kc columns per LDS
 * chunk, buf = entries of a row's candidate buffer for this handle's topk.
 * GW_ERR_STATE for a host handle.                                             */
int gw_knn_tiles(const gw_knn* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf);
/* Measurement aid (tools/bench_knn.py): the fp64 fma rate of this GPU under
 * the main loop's instruction mix at its best - `blocks` workgroups of 256
 * lanes, 16 independent fma chains per lane, `iters` rounds; one warm-up
 * launch, one timed with device events.  GW_ERR_STATE for a host handle.      */
int gw_knn_fma_rate(gw_knn* m, int blocks, int iters, double* fma_per_second);
/* preprocess_simrank (DeepSim/src/main.py:132-167) on top-k rows: for
 * t = 1 .. topk, acc[t-1] = the share, among the first min(t, listed)
 * neighbours of every row, of those that have a label in common with the
 * row's vertex (0 / 0 -> 0).  ids: [nrows][topk], -1 padded; row_ids: the
 * vertex of each row (NULL: row r is vertex r); lab_off / lab_ids: CSR of the
 * labels of the n vertices, ids ascending within a vertex.  Host code.  An id
 * outside [-1, n) gives GW_ERR_RANGE.                                         */
int gw_topk_label_agreement(const int32_t* ids, int64_t nrows, int topk, const int32_t* row_ids,
                            const int64_t* lab_off, const int32_t* lab_ids, int64_t n, double* acc);

/* ---- Laplacian eigenmaps of top-k rows ---------------------------------------- */
/* Replaces IsoMap_LE/simRank.py:95-123 (general form IsoMap_LE/LE.py:35-51): the
 * eigenvectors of D^-1 L, L = D - W, for the smallest eigenvalues above
 * min_eigenvalue, W built from top-k rows (gw_topsim's / gw_knn_query's layout)
 * or from a CSR.  The reference forms W and D densely and calls np.linalg.eig;
 * here W is sparse, symmetrised, and the pairs come from Chebyshev-filtered
 * block subspace iteration on S = D^-1/2 W D^-1/2 (D^-1 L f = lambda f  <=>
 * S u = (1 - lambda) u, f = s o u, s_i = 1 / sqrt(d_i)).  csrc/gw_le_law.h holds
 * the one definition kernels and host evaluation (device = -1) share; every sum
 * has one order, so the two agree bit for bit (tested).  All arithmetic is fp64.
 *   input     an entry with id -1 ends its row; an id equal to the row (unless
 *             self_loops = 1, below) and a score that is NaN or <= 0 are
 *             dropped; of the entries that remain
 *             a repeated id keeps the last value; an id outside [-1, n) gives
 *             GW_ERR_RANGE;
 *   W         w_ij = (a_ij + a_ji) / 2 (GW_LE_SYM_MEAN) or max(a_ij, a_ji)
 *             (GW_LE_SYM_MAX): the reference uses the asymmetric matrix as it is;
 *   isolated  a row with d_i = 0 is left out of the spectrum and its output row
 *             is all zeros (the reference gives it D_ii = 1e-6);
 *   output    eigenvalues ascending; f_c = s o u_c scaled to unit 2-norm, the
 *             entry of largest magnitude positive (lowest row wins ties); the
 *             fp32 copy is the fp64 one rounded once.
 * Limits: n < 2^31; device path block <= 256 (GW_ERR_UNSUPPORTED); dim < block. */
#define GW_LE_SYM_MEAN 0
#define GW_LE_SYM_MAX 1
#define GW_LE_CONVERGED 0
#define GW_LE_NOT_CONVERGED 1 /* max_iters reached: the output is the last iterate */
typedef struct gw_le gw_le;
typedef struct gw_le_params_t {
  int32_t struct_size;   /* as gw_sgns_params_t.struct_size                    */
  int32_t dim;           /* eigenpairs returned (128)                          */
  int32_t block;         /* width of the iterated block (0: dim + 32), clamped
                            to the number of non-isolated rows                 */
  int32_t cheb_degree;   /* operator applications per filter (20)              */
  int32_t max_iters;     /* Rayleigh-Ritz steps (100)                          */
  int32_t symmetrize;    /* GW_LE_SYM_MEAN (default) or GW_LE_SYM_MAX          */
  double tol;            /* residual ||S u - theta u||_2 of every kept pair (1e-8) */
  double min_eigenvalue; /* leading eigenvalues <= this are skipped (1e-5,
                            LE.py:74; simRank.py:137 uses 1e-2)                */
  uint64_t seed;         /* of the Philox start block                          */
  int32_t self_loops;    /* 0 (default): an id equal to its row is dropped;
                            1: it is kept as w_ii, counts in d_i and becomes a
                            diagonal entry of S (IsoMap_LE/LE.py's matrix, whose
                            knn lists the point itself); a caller passing a
                            struct_size that ends before this field gets 0     */
} gw_le_params_t;
typedef struct gw_le_stats_t {
  int32_t state;       /* GW_LE_CONVERGED / GW_LE_NOT_CONVERGED                */
  int32_t iters;       /* Rayleigh-Ritz steps taken                            */
  int64_t applies;     /* applications of S to the block                       */
  int32_t skipped;     /* leading eigenvalues <= min_eigenvalue                */
  int32_t block_used;  /* block after clamping                                 */
  int64_t isolated;    /* rows with d_i = 0                                    */
  double max_residual; /* over the skipped and the returned pairs              */
} gw_le_stats_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = rows = vertices            */
int gw_le_create(int device, int64_t n, const gw_le_params_t* params, gw_le** out);
int gw_le_free(gw_le* m);
const char* gw_le_last_error(const gw_le* m);
/* W from rows (ids[n][topk] int32, scores[n][topk] double, row r = vertex r) or
 * from a CSR (offsets[n + 1] int64, nbrs int32, weights double or NULL = 1.0).
 * Host pointers in both modes: the operator is validated and assembled on the
 * host and, for device >= 0, uploaded.                                          */
int gw_le_set_rows(gw_le* m, const int32_t* ids, const double* scores, int topk);
int gw_le_set_csr(gw_le* m, const int64_t* offsets, const int32_t* nbrs, const double* weights);
/* Runs the solver on `stream` and synchronises it.  GW_ERR_STATE before set_*;
 * GW_ERR_CAPACITY when the block cannot hold the skipped pairs, dim and one
 * more (the message names the block needed) or the graph has fewer pairs above
 * min_eigenvalue than dim.  stats is optional.  GW_LE_NOT_CONVERGED is a state,
 * not an error.                                                               */
int gw_le_solve(gw_le* m, gw_le_stats_t* stats, void* stream);
/* Host arrays, each optional: eigenvalues[dim], vectors[n][dim], residuals[dim] */
int gw_le_export(gw_le* m, double* eigenvalues, double* vectors, double* residuals);
/* The fp32 vectors [n][dim] where they lie (device memory for device >= 0), for
 * gw_knn_set_vectors / gw_ovr_set_features; valid until the next solve or free. */
int gw_le_vectors_dev(gw_le* m, float** ptr, int64_t* pitch);
/* y = S x for a caller's block [n][cols], row-major; device pointers for
 * device >= 0, host pointers for -1.  x and y must not overlap.  Synchronous.   */
int gw_le_apply(gw_le* m, const double* x, double* y, int cols);
/* Launch geometry (tests place their shapes on its edges): rows of S per
 * workgroup of k_le_apply, the law's row chunk GW_LE_CHUNK of the tall-skinny
 * products, columns per lane pass of k_le_apply.  Valid for host handles too.  */
int gw_le_tiles(const gw_le* m, int32_t* rows_per_wg, int32_t* chunk, int32_t* cols_per_pass);
/* As gw_ovr_kernel_attrs                                                      */
int gw_le_kernel_attrs(gw_le* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                       int32_t* lds_bytes, int32_t* count);
/* Measurement aid (tools/bench_le.py): times `reps` launches of one kernel on
 * the solver's own buffers with device events; which: 0 apply (Chebyshev
 * combine), 1 gram + reduce, 2 rotate.  After gw_le_solve; the blocks are
 * overwritten, the exported results are not.  ms = mean per launch.           */
int gw_le_time_kernel(gw_le* m, int which, int reps, double* ms);

/* ---- neighbour graph of points ---------------------------------------------- */
/* Replaces the first two steps of IsoMap_LE/LE.py:35-60 (laplaEigen's knn and its
 * heat-kernel weights): for every source row of an fp32 matrix the topk rows at
 * the smallest Euclidean distance and W = exp(-|x_i - x_j|^2 / t), in gw_topsim's
 * row layout, so gw_le_set_rows (with self_loops = 1: LE.py's own matrix) and
 * gw_write_sim_text_topk take them as they are.  csrc/gw_nng_law.h holds the one
 * definition the kernels and the host evaluation (device = -1) share; they agree
 * bit for bit (tested).
 *   arithmetic  features are the caller's fp32 widened, everything else fp64;
 *   d2(i,j)     e = x[i][k] - x[j][k], acc = fma(e, e, acc) over k = 0 .. dim-1
 *               ascending from +0 (the reference's difference form): never
 *               negative, exactly 0 for equal rows, d2(i,j) and d2(j,i) have the
 *               same bits; no split-K, no reassociation;
 *   row of v    the candidates j != v with d2(v,j) neither NaN nor +inf, by d2
 *               ascending, then id ascending (a total order: nothing depends on
 *               tiles, grid or timing).  include_self = 0: the first topk of
 *               them.  include_self = 1 (LE.py's knn: a point is its own nearest
 *               neighbour): entry 0 is (v, d2 0, weight 1.0), then the first
 *               topk - 1 candidates.  Where other rows equal row v exactly,
 *               numpy's argsort may list one of them first and leave v out of the
 *               reference's row; here v always leads.  A row with fewer listed
 *               entries is padded with (-1, 0.0), d2 0.0;
 *   weight      heat_t > 0: exp(-(d2 / heat_t)) by the project's fp64 exp
 *               (gw_ovr_law.h): exactly 1.0 at d2 = 0 and +0 once d2 / heat_t
 *               exceeds 700 (listed, but no edge for gw_le); heat_t == 0: every
 *               listed weight is 1.0.
 * Device path: 1 <= dim <= 1024, 1 <= topk <= 128, n < 2^31 (else
 * GW_ERR_UNSUPPORTED); the host path takes any size.                          */
typedef struct gw_nng gw_nng;
typedef struct gw_nng_params_t {
  int32_t struct_size;  /* as gw_sgns_params_t.struct_size                     */
  int32_t dim;          /* columns read of a row (3)                           */
  int32_t topk;         /* entries per output row, the source included (10)    */
  int32_t include_self; /* 1 (default): the source is entry 0 of its row; 0    */
  double heat_t;        /* t of the heat kernel; 0 (default): unit weights;
                           negative or NaN: GW_ERR_INVALID                     */
} gw_nng_params_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = rows of the matrix         */
int gw_nng_create(int device, int64_t n, const gw_nng_params_t* params, gw_nng** out);
int gw_nng_free(gw_nng* m);
const char* gw_nng_last_error(const gw_nng* m);
/* As gw_knn_set_vectors / gw_knn_set_rows: the matrix is read where it lies
 * (zero-copy from gw_sgns_vectors_dev, gw_le_vectors_dev, ...), only dim floats
 * of a row are ever read, and it must outlive the queries.                    */
int gw_nng_set_vectors(gw_nng* m, const float* x, int64_t pitch);
int gw_nng_set_rows(gw_nng* m, int64_t n);
/* out_ids[r * topk + t] (int32), out_weights[r * topk + t] (double) and, where
 * out_d2 is not NULL, out_d2[r * topk + t] (double, the squared distance) of the
 * source sources[r], r < nsrc.  Pointers, sources == NULL, repeated sources,
 * nsrc == 0, GW_ERR_RANGE with nothing written, GW_ERR_STATE and the stream are
 * as in gw_knn_query.                                                         */
int gw_nng_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                 double* out_d2, void* stream);
/* As gw_ovr_kernel_attrs: this family's kernels only                          */
int gw_nng_kernel_attrs(gw_nng* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                        int32_t* lds_bytes, int32_t* count);
/* As gw_knn_tiles: tq source rows per workgroup, tc candidate rows per tile, kc
 * columns per LDS chunk, buf = entries of a row's candidate buffer for this
 * handle's topk.  GW_ERR_STATE for a host handle.                             */
int gw_nng_tiles(const gw_nng* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf);

/* ---- geodesics on a sparse graph -------------------------------------------- */
/* Isomap's hot path (the method IsoMap_LE's README names first): shortest-path
 * distances from many sources over a sparse graph with non-negative fp64
 * lengths, for full Isomap (every vertex a source) and landmark Isomap (L << n
 * sources).  csrc/gw_geo_law.h holds the one definition the kernels and the host
 * evaluation (device = -1) share; they agree bit for bit (tested).
 *   rows        top-k rows as gw_le_set_rows takes them, or a CSR: an id of -1 ends
 *               a row, an id equal to its row is dropped, a value that is NaN,
 *               negative or +inf is dropped, -0.0 counts as +0.0, a repeated id
 *               keeps the smallest value, an id outside [-1, n) gives GW_ERR_RANGE;
 *   squared     1: the values are squared distances (gw_nng_query's out_d2) and the
 *               length is their square root, taken on the host while the graph is
 *               assembled; 0: the values are the lengths;
 *   symmetrize  GW_GEO_SYM_UNION: l_ij = min of the listed a_ij and a_ji, an edge
 *               listed one way stands both ways; GW_GEO_DIRECTED: as listed;
 *   distance    dist(s, s) = +0; dist(s, v) = the minimum over all paths of the
 *               lengths added left to right from +0; +inf where there is no path or
 *               where every path's sum overflows.  Rounding of + is monotone and the
 *               lengths are >= 0, so this minimum is the only fixed point of
 *               dist[v] = min(dist[v], dist[u] + l(u,v)): no schedule changes a bit;
 *   components  of the symmetrised graph; a component's id is its lowest vertex, the
 *               main component is the largest, the lowest id winning ties.
 * Limits: n < 2^31.                                                            */
#define GW_GEO_SYM_UNION 0
#define GW_GEO_DIRECTED 1
typedef struct gw_geo gw_geo;
typedef struct gw_geo_params_t {
  int32_t struct_size; /* as gw_sgns_params_t.struct_size                      */
  int32_t symmetrize;  /* GW_GEO_SYM_UNION (default) | GW_GEO_DIRECTED         */
  int32_t squared;     /* 1: values are squared lengths; 0 (default): lengths  */
  double delta;        /* bucket width of the device schedule; 0 (default) =
                          chosen from the mean edge length; it never changes a
                          result; negative or NaN: GW_ERR_INVALID              */
  int32_t round_cap;   /* measurement aid of the tests: 0 (default) = the device
                          schedule's own round cap; c > 0: cap = c - 1 (1: every
                          source ends as Bellman-Ford, counted in fallbacks); it
                          never changes a result                               */
} gw_geo_params_t;
typedef struct gw_geo_stats_t {
  int64_t entries;             /* directed entries of the assembled graph      */
  int64_t components;
  int64_t main_component_size;
  int64_t rounds_max;          /* most rounds any source of the last query took
                                  (device; 0 on the host)                      */
  int64_t relaxations;         /* entries read by the last query, all sources  */
  int32_t fallbacks;           /* sources that reached the round cap and ended
                                  as plain Bellman-Ford (device)               */
} gw_geo_stats_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = vertices                    */
int gw_geo_create(int device, int64_t n, const gw_geo_params_t* params, gw_geo** out);
int gw_geo_free(gw_geo* m);
const char* gw_geo_last_error(const gw_geo* m);
/* Host pointers in both modes: the graph is assembled on the host and, for a
 * device handle, uploaded.  values == NULL in gw_geo_set_csr: every value 1.     */
int gw_geo_set_rows(gw_geo* m, const int32_t* ids, const double* values, int topk);
int gw_geo_set_csr(gw_geo* m, const int64_t* offsets, const int32_t* nbrs, const double* values);
/* component_of[n] (host, may be NULL) and the main component's id (may be NULL) */
int gw_geo_components(gw_geo* m, int32_t* component_of, int32_t* main_component);
/* out[r * pitch + v] = dist(sources[r], v), r < nsrc, v < n; pitch >= n and the
 * columns n .. pitch-1 are not touched.  Pointers are device memory for
 * device >= 0 and host memory for -1.  sources == NULL: every vertex, nsrc is
 * ignored.  Repeated and unordered sources are allowed; nsrc == 0 returns GW_OK and
 * does nothing.  A source outside [0, n) gives GW_ERR_RANGE and nothing is written.
 * GW_ERR_STATE before gw_geo_set_*.  Runs on `stream` and synchronises it.  A source
 * the bounded device schedule left unfinished gives GW_ERR_INTERNAL (never seen;
 * the bound is proven sufficient in csrc/gw_geo.hip).                           */
int gw_geo_query(gw_geo* m, const int32_t* sources, int64_t nsrc, double* out, int64_t pitch, void* stream);
/* entries, components and main_component_size of the graph; the rest of the last
 * query                                                                        */
int gw_geo_stats(gw_geo* m, gw_geo_stats_t* stats);
/* As gw_ovr_kernel_attrs: this family's kernels only                          */
int gw_geo_kernel_attrs(gw_geo* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                        int32_t* lds_bytes, int32_t* count);
/* lanes = threads of a workgroup (one workgroup per source; a lane scans 64
 * vertices of the bitmap per trip), lds_rows = the largest n whose distance row
 * and bitmaps are kept in LDS (above it they lie in the source's output row and
 * in device scratch), sources_per_launch = the grid's bound (a workgroup takes
 * further sources by stride).  GW_ERR_STATE for a host handle.                  */
int gw_geo_tiles(const gw_geo* m, int32_t* lanes, int32_t* lds_rows, int32_t* sources_per_launch);

/* ---- spring layout of a graph ------------------------------------------------ */
/* The layout under IsoMap_LE/simRank.py:show's picture: the Fruchterman-Reingold
 * force simulation networkx's spring_layout runs (its dense _fruchterman_reingold,
 * fp64), stated for a sparse matrix.  csrc/gw_layout_law.h holds the one
 * definition, every order of summation included, that the kernels and the host
 * evaluation (device = -1) share; they agree bit for bit (tested).
 *   matrix   a CSR or top-k rows as gw_le_set_rows takes them, used as listed (no
 *            symmetrisation): an id of -1 ends a row, an id equal to its row is
 *            dropped, repeated ids add, a negative value repels, a value that is
 *            not finite gives GW_ERR_INVALID, an id outside [-1, n) GW_ERR_RANGE;
 *   iteration  disp_i = sum_j (pos_i - pos_j) k^2 / max(d2_ij, 1e-4)
 *                     - sum_{e in row i} (pos_i - pos_e) a_e max(sqrt(d2), 0.01) / k;
 *            len_i = |disp_i|, replaced by 0.1 where below 0.01; pos_i += disp_i t / len_i
 *            (not for a fixed vertex); t -= dt; stop when sqrt(sum step^2) / n < threshold;
 *   cooling  t0 = 0.1 max(extent of coordinate 0, extent of coordinate 1),
 *            dt = t0 / (iterations + 1).
 * Limits: n < 2^31, dim 2 or 3.  A device handle holds ceil(n / 1024) * n * dim
 * doubles of scratch (the all-pairs kernel's chunk sums): 157 MB at n = 100,000
 * and dim 2, 15.6 GB at n = 1,000,000; gw_layout_create gives GW_ERR_NOMEM
 * when it does not fit.                                                         */
typedef struct gw_layout gw_layout;
typedef struct gw_layout_params_t {
  int32_t struct_size; /* as gw_sgns_params_t.struct_size                      */
  int32_t reserved;    /* 0                                                    */
} gw_layout_params_t;
/* device >= 0: a GPU; -1: the host evaluation.  n = vertices, dim = 2 or 3 (else
 * GW_ERR_INVALID)                                                              */
int gw_layout_create(int device, int64_t n, int dim, const gw_layout_params_t* params, gw_layout** out);
int gw_layout_free(gw_layout* m);
const char* gw_layout_last_error(const gw_layout* m);
/* Host pointers in both modes: the matrix is checked on the host and, for a device
 * handle, uploaded.  values == NULL in gw_layout_set_csr: every value 1.          */
int gw_layout_set_csr(gw_layout* m, const int64_t* offsets, const int32_t* nbrs, const double* values);
int gw_layout_set_rows(gw_layout* m, const int32_t* ids, const double* values, int topk);
/* ids[count] (host): the vertices that do not move; count == 0 clears the list.
 * An id outside [0, n) gives GW_ERR_RANGE.                                      */
int gw_layout_set_fixed(gw_layout* m, const int32_t* ids, int64_t count);
/* pos[n][dim], updated in place: device memory for device >= 0, host memory for
 * -1.  k == 0: sqrt(1.0 / n); k < 0 or NaN, threshold NaN, iterations < 0 give
 * GW_ERR_INVALID; iterations == 0 leaves pos untouched.  The iterations are
 * launched back to back on `stream`; once the stop test has set a device flag every
 * later launch exits at once, and the host reads the count once at the end.
 * *iterations_done (may be NULL) = iterations carried out.  Synchronises the stream.  GW_ERR_STATE before gw_layout_set_*.            */
int gw_layout_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, void* stream,
                  int32_t* iterations_done);
/* One iteration at temperature t, without the cooling and the stop test:
 * disp_out[n][dim] (may be NULL) = disp, pos_out[n][dim] = pos_in + step.  pos_out
 * must not be pos_in.  Pointers as in gw_layout_run.  Synchronises the stream.    */
int gw_layout_step(gw_layout* m, const double* pos_in, double k, double t, double* disp_out, double* pos_out,
                   void* stream);
/* networkx's rescale_layout and the shift that follows it: subtract the column
 * means, multiply by scale / max|pos| where that maximum is > 0, add center[dim]
 * (host memory in both modes; NULL: zeros).  pos as in gw_layout_run.
 * Synchronises the stream.                                                      */
int gw_layout_rescale(gw_layout* m, double* pos, double scale, const double* center, void* stream);
/* As gw_ovr_kernel_attrs: this family's kernels only                          */
int gw_layout_kernel_attrs(gw_layout* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                           int32_t* lds_bytes, int32_t* count);
/* rows = rows of a workgroup of the all-pairs kernel (one per thread), chunk = the
 * law's column chunk (a workgroup streams one chunk through LDS), strands = the
 * interleaved partial sums of a chunk, block = vertices of a block in the law's
 * sums over vertices.  The last three are the law's constants: also for a host
 * handle, where rows is 0.                                                      */
int gw_layout_tiles(const gw_layout* m, int32_t* rows, int32_t* chunk, int32_t* strands, int32_t* block);

/* ---- multi-GPU exchange (RCCL over xGMI) ---------------------------------- */
/* the graph is replicated and units (walks, TopSim sources) are
 * sharded by global index with no data-path collective; the only exchange is
 * an all-gather of emitted blocks for hosts that need every walk on every
 * rank.  One process (or thread) per GPU; RCCL (librccl.so.1) is loaded on
 * first use, so the library itself carries no link-time RCCL dependency.
 * Rank 0 calls gw_comm_unique_id and hands the GW_COMM_ID_BYTES bytes to the
 * other ranks out of band (MPI, a file, torch.distributed, ...).            */
#define GW_COMM_ID_BYTES 128
#define GW_DTYPE_I32 0
#define GW_DTYPE_F64 1
typedef struct gw_comm gw_comm;
int gw_comm_unique_id(uint8_t* id);
int gw_comm_init(const uint8_t* id, int nranks, int rank, int device, gw_comm** out);
/* recv_dev[nranks * count] = concatenation of every rank's send_dev[count]
 * in rank order (ncclAllGather); asynchronous on `stream` (NULL = default). */
int gw_comm_allgather(gw_comm* c, const void* send_dev, void* recv_dev, int64_t count, int dtype, void* stream);
int gw_comm_free(gw_comm* c);
const char* gw_comm_last_error(const gw_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHWALK_H */
