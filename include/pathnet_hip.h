/*
 * pathnet_hip.h -- C ABI of libpathnet_hip.so, the MI355X (gfx950) implementation of PathNet's
 * path-aggregation hot path: the MERW path sampler and the PAGG aggregator forward/backward.
 *
 * The reference (Sunefei/PathNet) has no FFI for this path: its two seams are a text file on disk
 * between the C++ sampler and the Python trainer, and a Python nn.Module surface.
 * Every entry point below names the reference code it stands in for.  The Python host side in
 * pathnet_amd/ binds these with ctypes; INTEGRATION.md shows the stubs.
 *
 * Conventions
 *   - plain C: pointers, sizes, PODs.  No exceptions cross the boundary.
 *   - every function returns an int status: PN_OK (0) or a negative PN_ERR_*; pn_last_error()
 *     returns a thread-local, human readable description of the last failure.
 *   - the caller owns every buffer (inputs, outputs, workspaces).  The library never frees or
 *     retains a pointer past the call.  "dev" in a comment = device (HBM) pointer, "host" = host.
 *   - device work is enqueued on the hipStream_t passed as `stream` (void* here so the header
 *     needs no HIP include; pass torch.cuda.current_stream().cuda_stream).  Device entry points
 *     are asynchronous with respect to the host.
 *   - the library has NO process-global state.  What outlives a call -- the second stream
 *     pn_pagg_forward/backward fork a few independent launches onto (joined back with events before
 *     they return, so all their work is ordered before whatever the caller enqueues on `stream`
 *     next) and the per-stage timing records -- lives in an opaque pn_context the caller creates for
 *     one device and destroys when done.  A context serialises nothing: two host threads may drive
 *     the same device through two contexts; one context must not be used by two threads at once.
 *     Every device entry point accepts ctx = NULL: everything then runs on `stream` alone, untimed.
 *   - the host-only entry points (files, tables) are re-entrant and use up to PN_HOST_THREADS threads.
 *   - sizes: n nodes, m edge rows, W walks per node (path_num), L path length, S masked nodes,
 *     P = S*W paths, H hidden size, F input features, C classes.
 */
#ifndef PATHNET_HIP_H_
#define PATHNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_ABI_VERSION 12 /* 2: pn_sampler_tables gained draws_per_step; pn_pairs_*, pn_uniform_*, pn_merw_*, pn_cross_entropy, pn_adam_step
                          * 4: pn_context (no process-global state); pn_pagg_shape gained S_total / group_begin / batch_groups
                          *    (micro-batches, exact sharding of the hetero class); pn_pagg_args gained reuse_tables; 64-bit
                          *    offsets throughout; pn_clock_probe
                          * 5: pn_pagg_shape gained deterministic; pn_linear_backward gained workspace / workspace_bytes;
                          *    pn_pagg_train_step
                          * 6: pn_pagg_shape gained compact / seq_math (decisions that shape the workspace travel with the
                          *    shape, not with the environment); pn_pagg_args.reuse_tables = 2; pn_pagg_shape_info; pn_pagg_args gained
                          *    Xh_ready / g_Xh_ready (events that let the node-sharded path overlap its collectives)
                          * 7: pn_context_set_knob / pn_context_get_knob: the kernel-selection knobs are part of the context (read
                          *    from the environment once, when it is created); no call reads the environment any more
                          * 8: pn_seq_range / pn_pagg_range_offset (the fp16 recurrence's operand range and the spread of the gathered
                          *    rows' magnitudes, for callers that want to fall back to bf16x3 on pathological inputs)
                          * 9: pn_adam_step_advance (the optimizer's last launch moves the step state on)
                          * 10: pn_pagg_paths_stream (where a call reads its path arrays: a sampler enqueued there needs no event)
                          * 11: pn_tables_workspace_bytes, pn_alias_build_device, pn_csr_build_device, pn_hops_dense_device (the
                          *     sampler's tables built on the device, bit-identical to the host builders)
                          * 12: pn_pagg_args gained out_embed / out_path_weight / out_path_state / g_embed (the classifier input
                          *     and the pooling coefficients and final hidden states of the paths, and a gradient on the first) */

#define PN_OK 0
#define PN_ERR_ARG (-1)          /* bad argument / unsupported shape */
#define PN_ERR_IO (-2)           /* file could not be opened / read / written */
#define PN_ERR_FORMAT (-3)       /* malformed text */
#define PN_ERR_HIP (-4)          /* a HIP runtime call or kernel launch failed */
#define PN_ERR_EMPTY_TABLE (-5)  /* a walk reached a node with no outgoing rows (gen_merw.cpp:84-87) */
#define PN_ERR_NOMEM (-6)
#define PN_ERR_CAPACITY (-7)     /* caller buffer too small; the required size is reported */

int pn_abi_version(void);
const char *pn_last_error(void);

/* GPU the library will launch on (current HIP device): name/arch and CU count, for bench reports. */
typedef struct pn_device_info {
    char name[128];
    char arch[64];
    int32_t compute_units;
    int32_t lds_bytes_per_block;
    int64_t hbm_bytes;
    int32_t clock_khz;
} pn_device_info;
int pn_device_query(pn_device_info *out);

/* Per-device, per-caller state: one internal non-blocking stream with its fork/join events and the records of
 * pn_profile_*.  Created on the current HIP device; every call that is handed the context must run with that
 * device current (checked).  pn_context_destroy waits for the context's own stream and releases it. */
typedef struct pn_context pn_context;
int pn_context_create(pn_context **out);
int pn_context_destroy(pn_context *ctx);
/* Kernel-selection knobs for A/B measurements and tests (none changes a result beyond rounding): PN_NODE_GEMM3, PN_EVAL_ZW,
 * PN_POOL_STEP, PN_EVENT_DEVICE_SCOPE, PN_NODE_RGRAD, PN_SAMPLER_STAGE, PN_SEQ4, PN_FC0_SPARSE (pn_internal.h: struct Knobs).  A context
 * takes its values from the environment variables of the same names ONCE, in pn_context_create; afterwards only these two
 * calls read or change them -- device entry points never call getenv, so a captured step keeps its selection and a setenv
 * on another thread cannot race a launch.  get accepts ctx = NULL (the defaults a NULL context runs with). */
int pn_context_set_knob(pn_context *ctx, const char *name, int32_t value);
int pn_context_get_knob(const pn_context *ctx, const char *name, int32_t *value);

/* Per-step values kept in DEVICE memory, so that a whole training step captured into a hipGraph (every launch below is
 * capturable: no allocation, no synchronisation, the second stream joins the capture through its fork / join events) can
 * be replayed with fresh values: the sampler's epoch, the dropout seed and Adam's step count are read by the kernels
 * when they run, not baked into the launch.  pn_step_state_advance (one tiny launch, the first node of the graph) moves
 * to the next step: epoch += 1, adam_step += 1, seed = splitmix64(seed). */
typedef struct pn_step_state {
    int64_t epoch;      /* pn_sample_paths: epoch_begin */
    uint64_t seed;      /* pn_sample_paths (Philox seed) and pn_pagg_* (dropout seed) */
    int64_t adam_step;  /* pn_adam_step: the step count (from 1) */
    int64_t reserved;
} pn_step_state;
int pn_step_state_advance(pn_step_state *dev_state, void *stream);

/* Shader clock the device sustains right now (MHz), measured by a short kernel that reads the shader-cycle counter
 * (s_memtime) against the 100 MHz wall clock -- bench reports carry it so that box-to-box differences can be told
 * from code differences.  Synchronises `stream`. */
int pn_clock_probe(double *mhz, void *stream);

/* ================================================================================================
 * Sampler, host side.  Replaces the set-up half of preprocess/gen_merw.cpp main() (:162-179).
 * ============================================================================================== */

/* Edge file "<n> <m>\n" then m rows "u v p"  (gen_merw.cpp:162-172, gen_epoch_merw.cpp:145-155).
 * Call with cap = 0 to read only n and m; then with cap >= m to fill u, v, p (host, file order). */
int pn_edges_read_text(const char *path, int32_t *n, int64_t *m, int32_t *u, int32_t *v, double *p, int64_t cap);

/* ---- the uniform random-walk sampler ("RW-PathNet" ablation): preprocess/gen.cpp, gen_epoch.cpp ------------------
 * Pair file "<n> <m>" then m pairs "u v", read the way gen.cpp:80-92 reads it (scanf("%d%d")).  cap = 0 reads only
 * n and m; cap >= m fills u, v (host, file order). */
int pn_pairs_read_text(const char *path, int32_t *n, int64_t *m, int32_t *u, int32_t *v, int64_t cap);

/* The graph gen.cpp:83-94 walks on: list i starts with the self loop i, every pair with u != v then appends v to list
 * u and u to list v, in file order, repeated pairs kept.  off[n+1] prefixes the lists; packed[total*4] is the list
 * in the walker's 16-byte triple layout {nbr, nbr, 0, 0}; src/nbr (each [total], may be NULL) is the same graph as a
 * directed edge list for pn_hops_dense / pn_csr_build.  cap = 0 only sizes (*total). */
int pn_uniform_build(int32_t n, int64_t m, const int32_t *u, const int32_t *v, int64_t *off, int32_t *packed,
                     int32_t *src, int32_t *nbr, int64_t cap, int64_t *total);

/* Alias tables of every node, bit-identical to AliasTable::init (gen_merw.cpp:23-79) run on the
 * per-node lists that link() (:95-99) builds in file order.  off[n+1] is the per-node prefix of the
 * triple arrays.  A/B are the two candidate next nodes, S the fp64 split value, and
 * thr = the smallest 31-bit draw r for which (1.0 * r / RAND_MAX > S), so that roll() (:81-91)
 * becomes the integer test  r >= thr ? A : B  (thr = 2^31 when no draw qualifies).
 * Call with cap = 0 to get *total (and off[]); then with cap >= *total.  S may be NULL. */
int pn_alias_build(int32_t n, int64_t m, const int32_t *u, const int32_t *v, const double *p, int64_t *off,
                   int32_t *A, int32_t *B, double *S, uint32_t *thr, int64_t cap, int64_t *total);

/* Dense hop table dis[n*n] (host, uint8): dis[s*n + x] = 1 + (hops from s to x) for every x within
 * seq_len-1 hops of s, 0 otherwise -- the values bfs() (gen_merw.cpp:101-123) leaves in dis[][] for
 * every node a walk of length seq_len can visit.  The emitted distance code is dis - 1. */
int pn_hops_dense(int32_t n, int64_t m, const int32_t *u, const int32_t *v, int32_t seq_len, uint8_t *dis);

/* Sorted, duplicate-free adjacency in CSR form (host): for reverse = 0 the out-neighbours of every node
 * (row "u v p" puts v into list u), for reverse = 1 the in-neighbours.  Used instead of the dense hop
 * table when n*n bytes is too much (the reference's dis[N][N], gen_merw.cpp:10, caps n at 100050):
 * the walker then derives dis[st][x] - 1 exactly from these lists (see pn_sampler_tables).
 * Call with cap = 0 to get *count (and off[]); then with cap >= *count. */
int pn_csr_build(int32_t n, int64_t m, const int32_t *u, const int32_t *v, int32_t reverse, int64_t *off,
                 int32_t *adj, int64_t cap, int64_t *count);

/* The first `count` values rand() returns after srand(seed), starting at stream position `first`
 * (host, int32).  Uses the same jump algebra as the device generator (glibc TYPE_3 recurrence as
 * a polynomial over Z/2^32), so any window of the reference's draw stream (gen_merw.cpp:88-89) can
 * be produced without replaying the stream from the start. */
int pn_glibc_draws(uint32_t seed, uint64_t first, int64_t count, int32_t *out);

/* ================================================================================================
 * Sampler, device side.  Replaces the walk loop gen_merw.cpp:182-209 (and the per-epoch variant
 * gen_epoch_merw.cpp:164-206): one walk per GPU lane.
 * ============================================================================================== */

#define PN_DRAW_GLIBC_REPLAY 0 /* draws = glibc rand() after srand(seed): bit-exact to the reference binary */
#define PN_DRAW_PHILOX 1       /* draws = rocRAND Philox4x32-10, subsequence = global walk index (throughput) */

typedef struct pn_sampler_tables {
    int32_t n;               /* nodes */
    int64_t total;           /* alias triples */
    const int64_t *off;      /* dev [n+1]  prefix into the triple array */
    const int32_t *triples;  /* dev [total*4] packed {A, B, thr, 0} (one 16-byte load per roll) */
    const uint8_t *dis;      /* dev [n*n]  dense hop table from pn_hops_dense, or NULL: */
    /* dis == NULL selects on-the-fly hop codes (any n): exact hops(st -> x) by meeting in the middle of the
     * <=2-hop out-ball of the source (a hash table in LDS, built once per source node) and a bounded
     * search over the in-neighbours of x.  Needs both CSR lists from pn_csr_build (device copies). */
    const int64_t *adj_off;  /* dev [n+1] */
    const int32_t *adj;      /* dev out-neighbours, sorted per node */
    const int64_t *radj_off; /* dev [n+1] */
    const int32_t *radj;     /* dev in-neighbours, sorted per node */
    /* draws per walk step: 0 or 2 = the MERW alias roll (slot draw + probability draw, gen_merw.cpp:81-91);
     * 1 = the uniform sampler's single rand() % deg (gen.cpp:113-114) over tables from pn_uniform_build. */
    int32_t draws_per_step;
    /* dev [n][2] uint32 {first triple, number of triples} of every node (pn_node_ref_pack), or NULL: with it a roll
     * fetches a node's table position with ONE 8-byte load instead of two words of off[] (total < 2^32 triples). */
    const uint32_t *node_ref;
} pn_sampler_tables;

/* host: off[n+1] -> ref[n][2] = {off[i], off[i+1] - off[i]}.  Fails when the table holds 2^32 triples or more. */
int pn_node_ref_pack(int32_t n, const int64_t *off, uint32_t *ref);

/* Pack host A/B/thr arrays into the 16-byte device layout (host helper, dst is a host buffer of
 * total*4 int32 that the caller then copies to the device). */
int pn_alias_pack(int64_t total, const int32_t *A, const int32_t *B, const uint32_t *thr, int32_t *dst);

/* ---- the same tables built on the device (pn_tables.hip), bit-identical to the host builders above ------------------
 * Every pointer is a device pointer; every call enqueues on `stream` and takes a caller-owned workspace of at least
 * pn_tables_workspace_bytes(n, m) bytes (a bound that needs no device; one workspace serves the alias and CSR calls).
 * The edge rows are checked first: the first row whose source or target lies outside [0, n) fails with PN_ERR_ARG
 * naming it, as the host builders do.  That check reads one word back, so these two calls synchronise with the stream.
 * m >= 2^31 (the radix sort's range) fails with PN_ERR_ARG. */
int pn_tables_workspace_bytes(int32_t n, int64_t m, int64_t *bytes);

/* pn_alias_build + pn_alias_pack + pn_node_ref_pack on the device: off[n+1], triples[total*4] in the walker's packed
 * {A, B, thr, 0} layout (16-byte aligned), node_ref[n][2] (may be NULL) and the fp64 splits S[total] (may be NULL).
 * A node with k rows has exactly k triples (every triple retires one of its pending items), so *total = m and off[]
 * is the per-source prefix of the rows; total < 2^31 always fits node_ref.  cap = 0 only sizes (*total, off[]); then
 * call with cap >= *total, which redoes the bucketing. */
int pn_alias_build_device(int32_t n, int64_t m, const int32_t *u, const int32_t *v, const double *p, int64_t *off,
                          int32_t *triples, uint32_t *node_ref, double *S, int64_t cap, int64_t *total, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* pn_csr_build on the device: sorted, duplicate-free out-lists (reverse = 0) or in-lists (reverse = 1), off[n+1] and
 * adj[*count].  Returning *count synchronises with the stream.  cap = 0 only sizes (*count, off[]); a call with
 * cap >= *count (any upper bound, m included) also writes adj. */
int pn_csr_build_device(int32_t n, int64_t m, const int32_t *u, const int32_t *v, int32_t reverse, int64_t *off,
                        int32_t *adj, int64_t cap, int64_t *count, void *workspace, int64_t workspace_bytes, void *stream);

/* pn_hops_dense on the device, from the out-lists of pn_csr_build_device (off[n+1], adj with entries in [0, n); NULL
 * when the lists are empty):
 * dis[n*n] uint8 with the same values.  seq_len outside 1..254 fails with PN_ERR_ARG.  Needs no workspace and does
 * not synchronise. */
int pn_hops_dense_device(int32_t n, const int64_t *off, const int32_t *adj, int32_t seq_len, uint8_t *dis, void *stream);

/* Bytes of device scratch pn_sample_paths needs for this window (0 for PN_DRAW_PHILOX). */
int pn_sample_workspace_bytes(int32_t W, int32_t L, int32_t draw_source, int64_t epoch_count, int32_t node_count,
                              int64_t *bytes);

/* Sample paths for epochs [epoch_begin, epoch_begin+epoch_count) and source nodes
 * [node_begin, node_begin+node_count) -- or, with node_list (dev int32 [node_count], PN_DRAW_PHILOX only: a walk's draws
 * are a function of (epoch, source node, walk index), whatever else is sampled beside it), the listed source nodes in
 * list order: a training step samples the paths of its masked nodes only (PathNet_run.py:345 indexes them out of the
 * epoch's file).  ids/codes are dev [epoch_count, node_count, W, L]
 * (int32 node ids, uint8 distance codes = dis - 1), i.e. exactly the numbers the reference prints,
 * in the reference's order.  The draw index of (epoch e, node st, walk i, step t) is
 * 2*(((e*n + st)*W + i)*L + t) (+1 for the probability draw), as in the reference where the last
 * roll of each walk is drawn and discarded (:195-196).
 * status_flag (dev int32, may be NULL) is set to PN_ERR_EMPTY_TABLE if any walk reaches a node with
 * an empty table (the reference exits there). */
int pn_sample_paths(pn_context *ctx, const pn_sampler_tables *tables, int32_t W, int32_t L, int32_t draw_source, uint64_t seed,
                    int64_t epoch_begin, int64_t epoch_count, int32_t node_begin, int32_t node_count, int32_t *ids,
                    uint8_t *codes, void *workspace, int64_t workspace_bytes, int32_t *status_flag,
                    const pn_step_state *step_state /* dev or NULL: PN_DRAW_PHILOX only; replaces seed / epoch_begin */,
                    const int32_t *node_list /* dev [node_count] or NULL */, void *stream);

/* ---- distance codes and walk checks for paths that did not come from pn_sample_paths (pn_codes.hip) ----------------
 * Paths of another sampler, of an ids-only file, or sampled before edges were hidden or added carry node ids only;
 * this annotates them from the walker's hop source and counts what is wrong with them.  Added without an ABI bump:
 * symbols only, no existing struct changed.
 *
 * Only the hop source of `tables` is read: dis, or (dis == NULL) the four CSR arrays; off / triples / node_ref may be
 * NULL.  The source of row s is sources[s] when given, else ids[s, 0, 0].
 *   codes[s, w, t] = min(hops(source -> ids[s, w, t]), L-1) over the directed edges the tables were built from.  A node
 *     that is further away or unreachable gets L-1 and counts in `far`; an id outside [0, n) gets L-1, counts in
 *     `out_of_range` and never indexes a table.  A source outside [0, n) (possible only through `sources`; it is not
 *     an element of ids and is not counted as one) leaves every node of its row `far`.
 *   non_edges counts the steps t -> t+1 whose two nodes are in range and more than one hop apart; staying in place is
 *     accepted, because the dense table cannot tell a self loop from identity.
 * Both modes give the same numbers, and for paths pn_sample_paths produced from the same tables the codes are the
 * walker's, bit for bit.  A dense table must have been built with seq_len >= L (this cannot be seen from the struct:
 * a table built for shorter paths reports nodes beyond its own radius as far); on-the-fly keeps the walker's limits
 * (n < 2^28, L <= 8, and fewer than 2^32 entries in each CSR list: positions in them are kept as 32-bit words, which
 * the call cannot check) and is exact for every source, hubs whose out-ball does not fit the LDS table included.  Its cost
 * per node grows with the number of in-neighbour chains of length L-1-(ball radius): see pn_codes.hip.
 * Asynchronous: nothing is read back.  `report` (may be NULL) is zeroed by the call, first_bad set to -1.  The workspace
 * (its size from the function below, which needs no device) receives the counters of a call without a report; a missing
 * or short one fails with PN_ERR_ARG. */
typedef struct pn_path_report {   /* device memory, caller-owned, zeroed by the call */
    int64_t out_of_range;         /* ids < 0 or >= n */
    int64_t non_edges;            /* consecutive (ids[t], ids[t+1]) with hops > 1 */
    int64_t far;                  /* nodes more than L-1 hops from the row's source */
    int64_t first_bad;            /* flat index of the first out_of_range id, or -1 */
} pn_path_report;

int pn_path_codes_workspace_bytes(const pn_sampler_tables *tables, int32_t W, int32_t L, int32_t rows, int64_t *bytes);
int pn_path_codes(pn_context *ctx, const pn_sampler_tables *tables, int32_t W, int32_t L, int32_t rows,
                  const int32_t *ids /* dev [rows, W, L] */, const int32_t *sources /* dev [rows] or NULL */,
                  uint8_t *codes /* dev [rows, W, L] */, pn_path_report *report /* dev or NULL */,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* ---- second-order (return / in-out biased) walks (pn_bias.hip) ----------------------------------------------------
 * node2vec's bias over the walker's own tables.  Added without an ABI bump: three symbols, no existing struct changed.
 * Step t >= 1 of a walk at node cur that came from prev has the target distribution
 *     P(x) ~ P_table(cur -> x) * a(prev, x),  a = 1/p when x == prev (class 0, return), 1 when the hop source has the
 *     directed edge prev -> x (class 1, near), 1/q otherwise (class 2, far);
 * step 0 is the plain table step.  p = +inf never returns (non-backtracking), q = +inf never leaves prev's
 * neighbourhood -- as far as the table allows, see the trial cap.
 *
 * Realisation: rejection sampling from the table.  pn_bias_thresholds (host, fp64, no device) gives the accept
 * thresholds T_c = floor(2^32 * w_c / max(w)), w = {1/p, 1, 1/q} with weight 0 for an infinite parameter; the largest
 * class gets exactly 2^32 (always accepted).  p and q must be > 0; 0, negatives and NaN fail with PN_ERR_ARG.
 * A walk's Philox subsequence is the plain walker's global walk index ((epoch*n + st)*W + wi), the key is the seed.
 * The trials of one walk are numbered j = 0, 1, 2, .. across all its steps; trial j reads Philox block j (draws
 * 4j .. 4j+2 of the subsequence): word 0 >> 1 is the slot draw (% table length), word 1 >> 1 the alias probability draw
 * (>= thr ? A : B; both candidates are the same node in uniform tables), the full word 2 the accept draw -- the proposal
 * is taken iff word 2 < T_class -- and word 3 is unused.  Step 0 takes its first proposal.
 * A step takes at most PN_BIAS_MAX_TRIALS trials: a step that comes to its 64th trial takes that proposal whatever the
 * accept draw says and is counted in *exhausted.  So the realised distribution differs from the target on at most the
 * `exhausted` share of the steps, and a walk at a leaf under p = inf returns to where it came from (after 64 trials).
 * A walk of length L makes L-1 transitions and, unlike pn_sample_paths, draws nothing after its last node.  A node with
 * an empty table at a step that needs one sets status_flag = PN_ERR_EMPTY_TABLE; the rest of that path repeats the
 * node and no further draws are made.
 *
 * ids / codes are dev [epoch_count, node_count, W, L] as for pn_sample_paths, and the codes are those pn_path_codes
 * gives for the ids over the same tables, bit for bit (on the fly they come from that very launch, enqueued by this
 * call behind the walk).  exhausted (dev int64, may be NULL) is zeroed by the call.  node_list and step_state as for
 * pn_sample_paths.  Asynchronous: nothing is read back.  The workspace (size from the query, which needs no device:
 * 0 with a dense table) may be NULL when the query says 0.  Argument errors -- null tables, W < 1, L < 1, no hop source,
 * half a CSR, on-the-fly L > 8, bad p / q, a short or missing workspace -- fail with PN_ERR_ARG before any device
 * call. */
#define PN_BIAS_MAX_TRIALS 64
int pn_bias_thresholds(double p, double q, uint64_t thr[3]);
int pn_sample_paths_biased_workspace_bytes(const pn_sampler_tables *tables, int32_t W, int32_t L, int64_t epoch_count,
                                           int32_t node_count, int64_t *bytes);
int pn_sample_paths_biased(pn_context *ctx, const pn_sampler_tables *tables, int32_t W, int32_t L, uint64_t seed,
                           int64_t epoch_begin, int64_t epoch_count, int32_t node_begin, int32_t node_count, double p,
                           double q, int32_t *ids, uint8_t *codes, int64_t *exhausted /* dev or NULL */, void *workspace,
                           int64_t workspace_bytes, int32_t *status_flag, const pn_step_state *step_state,
                           const int32_t *node_list, void *stream);

/* ---- the synthetic-label generator (pn_census.hip): synthetic_data/gen_cora_syn.cpp, gen_citeseer_syn.cpp ------------
 * For every node, the walks of walk_len steps binned by the symbols of the nodes they visit, and the most frequent bin.
 * Added without an ABI bump: four new symbols, no existing struct or signature changed, so a caller built against
 * version 12 runs unchanged and pn_abi_version keeps answering 12.
 *
 * pn_census_lists builds the graph the reference walks on from the m rows (u, v) of a pair file (device int32 arrays):
 * every row puts v into u's list AND u into v's, duplicates are kept (a multigraph) and a row with u == v adds two
 * entries to that node's list -- unlike pn_csr_build_device, which removes duplicates and is directed.  off[n+1] int64,
 * adj[2m] int32, order inside a list unspecified.  The rows are checked as the table builders check theirs: the first
 * row with a node outside [0, n) fails with PN_ERR_ARG naming it, and that check reads one word back, so this call
 * synchronises with the stream.  m >= 2^30 (2m entries: the radix sort's range) fails with PN_ERR_ARG.  The workspace
 * size needs no device. */
int pn_census_lists_workspace_bytes(int32_t n, int64_t m, int64_t *bytes);
int pn_census_lists(pn_context *ctx, int32_t n, int64_t m, const int32_t *u, const int32_t *v, int64_t *off, int32_t *adj,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* counts[i][p] (dev int64 [n, B^k], may be NULL) = the number of walks i -> v1 -> ... -> vk along list entries, with
 * multiplicity, whose pattern sum_j s[v_j] * B^(k-j) is p (the first step is the most significant digit; B =
 * num_symbols, k = walk_len).  labels[i] (dev int64 [n], may be NULL) = the SMALLEST pattern among those with the
 * largest count, so an isolated node gets 0; with counts == NULL the n * B^k table is never written.  At least one of
 * the two must be given.  symbols: dev uint8 [n] with values in [0, B) (a larger value counts as B - 1), or NULL for
 * the reference's s[v] = v & 1.  off / adj as pn_census_lists writes them (entries in [0, n) are the caller's promise).
 * Limits, checked with PN_ERR_ARG: walk_len >= 1, 2 <= num_symbols <= 16, B^k <= 1024.  Counts are exact int64 sums
 * (the reference counts in int): they stay below 2^63 when (longest list)^k does, which the caller checks.
 * One launch per level, asynchronous, nothing read back; the workspace holds two level tables of n * B^(k-1) counts
 * (size from the function below, which needs no device; none is needed for walk_len = 1). */
int pn_pattern_census_workspace_bytes(int32_t n, int32_t num_symbols, int32_t walk_len, int64_t *bytes);
int pn_pattern_census(pn_context *ctx, int32_t n, const int64_t *off, const int32_t *adj,
                      const uint8_t *symbols /* dev [n] or NULL */, int32_t num_symbols, int32_t walk_len,
                      int64_t *counts /* dev [n, B^k] or NULL */, int64_t *labels /* dev [n] or NULL */, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* ---- walk statistics (pn_stats.hip): what sampled paths look like, counted on the device ----------------------------
 * pn_path_codes counts what is wrong with paths; this describes paths that are right.  Added without an ABI bump: two new
 * symbols and one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * One pass over ids / codes [rows, W, L]; a row is the W paths of one (epoch, source node), and the source of row s is
 * sources[s] when given, else ids[s, 0, 0].  Every result is an exact integer count: it depends neither on the launch
 * geometry nor on the order of the atomics.  The outputs are caller-owned device memory, described by one
 * pn_walk_stats_out; each pointer may be NULL, meaning "not wanted, never written".
 *   step_code[t][d]      path nodes at step t whose code is d.  A code >= L counts in counters[1] (bad_codes) and nowhere
 *                        else: such a node is in neither step_code, label_pairs nor unlabeled.
 *   label_pairs[d][a][b] path nodes with code d whose row's source has label a and which themselves have label b; needs
 *                        labels (dev int32 [n]) and C.  A node or source outside [0, n), or whose label lies outside
 *                        [0, C) (-1 = unlabelled), counts in unlabeled[d] instead, so label_pairs[d].sum() + unlabeled[d]
 *                        = step_code[:, d].sum().  Edge homophily by distance is trace / sum per d.
 *   stay[t], back[t]     stay[t], t >= 1: ids[t] == ids[t-1].  back[t], t >= 2: ids[t] == ids[t-2] and ids[t] != ids[t-1].
 *                        The other entries are 0.
 *   distinct_hist[k]     paths that visit exactly k distinct ids (k = 1 .. L; entry 0 stays 0).
 *   unique_paths[s]      distinct id sequences among the W paths of row s.
 *   cover[s]             distinct ids among the W * L entries of row s.
 *   visits[v]            times node v occurs at a step t >= 1.
 *   counters             {out_of_range, bad_codes}: entries of ids outside [0, n) / entries of codes >= L.
 * An id outside [0, n) never indexes labels or visits; in the distinct, unique and cover counts it is an ordinary integer.
 * A source outside [0, n) (possible only through `sources`) is no entry of ids and is not counted in out_of_range.
 * accumulate == 0: the call zeroes the global tables (every output but unique_paths and cover) before it counts;
 * accumulate != 0: it adds to what they hold, so a loop over epochs profiles a run without keeping its paths.
 * Limits, refused with PN_ERR_ARG before any device call: 1 <= L <= 16, W >= 1, W * L <= 8192, rows >= 0, n >= 1,
 * 1 <= C <= 64 when labels are given (C is ignored without them); label_pairs or unlabeled without labels; NULL ids or
 * codes with rows > 0; NULL out.  rows == 0 is valid: it zeroes the tables when not accumulating and launches nothing
 * over rows.  Asynchronous on `stream`: nothing is read back.  The workspace size comes from the query, which needs no
 * device and answers 0 today (a row is counted in LDS); the workspace may be NULL when it does. */
typedef struct pn_walk_stats_out {   /* device pointers, caller-owned, each may be NULL */
    int64_t *step_code;              /* [L, L] */
    int64_t *label_pairs;            /* [L, C, C] */
    int64_t *unlabeled;              /* [L] */
    int64_t *stay;                   /* [L] */
    int64_t *back;                   /* [L] */
    int64_t *distinct_hist;          /* [L + 1] */
    int32_t *unique_paths;           /* [rows] */
    int32_t *cover;                  /* [rows] */
    int64_t *visits;                 /* [n] */
    int64_t *counters;               /* [2] */
} pn_walk_stats_out;

int pn_walk_stats_workspace_bytes(int32_t n, int32_t W, int32_t L, int64_t rows, int32_t C, int64_t *bytes);
int pn_walk_stats(pn_context *ctx, int32_t n, int32_t W, int32_t L, int64_t rows,
                  const int32_t *ids /* dev [rows, W, L] */, const uint8_t *codes /* dev [rows, W, L] */,
                  const int32_t *sources /* dev [rows] or NULL */, const int32_t *labels /* dev [n] or NULL */, int32_t C,
                  int32_t accumulate, const pn_walk_stats_out *out, void *workspace, int64_t workspace_bytes,
                  void *stream);

/* Path multiplicities: mult[r, j] (dev fp32 [rows, W]) = the number of paths k of row r whose id sequence -- and code
 * sequence, when codes is not NULL -- equals path j's, when j is the lowest such index; otherwise 0.  Every row sums to W
 * exactly.  As pn_path_weights.weight with PN_PATH_NORM_SUM the result pools a row's distinct paths once each, weighted
 * by how often they were drawn: the same value as the unweighted pooling of the row (HOMO / PAGG, where a row's entries are
 * its own paths).  Limits as pn_walk_stats: 1 <= L <= 16, W >= 1, W * L <= 8192, rows >= 0, else PN_ERR_ARG; rows == 0
 * launches nothing.  Asynchronous on `stream`: nothing is read back.  A new symbol: pn_abi_version keeps answering 12. */
int pn_path_multiplicity(pn_context *ctx, int32_t W, int32_t L, int64_t rows, const int32_t *ids /* dev [rows, W, L] */,
                         const uint8_t *codes /* dev [rows, W, L] or NULL */, float *mult /* dev [rows, W] */, void *stream);

/* ---- transition probabilities and path likelihoods (pn_prob.hip): the walker's tables, evaluated --------------------
 * pn_sample_paths draws from the tables; this says how likely given paths are under them.  Added without an ABI bump: two
 * new symbols and one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * The walker's step at a node cur whose table holds k triples {A, B, thr} is  slot = r0 % k,  next = r1 >= thr[slot] ? A : B
 * with r0, r1 uniform on [0, 2^31) -- glibc replay and Philox word >> 1 alike, in pn_sample_paths and in
 * pn_sample_paths_biased.  So the realised probability of cur -> x is the integer
 *     N(cur -> x) = sum_s c_s * (max(0, 2^31 - thr_s) * [A_s == x] + min(thr_s, 2^31) * [B_s == x]),
 *     c_s = 2^31 / k + (s < 2^31 % k),
 * over 2^62; the N of a non-empty table sum to exactly 2^62.  Uniform tables have A = B, so the same sum serves them.
 * ids is dev [rows, W, L]; a path of L nodes has L-1 transitions, and transition t is ids[t] -> ids[t+1].
 *   num[r, w, t]      N(ids[t] -> ids[t+1]).
 *   second_order != 0 (the biased walker's view; reads the hop source as well): for t >= 1, prev = ids[t-1], a node y is
 *     of class 0 when y == prev (also when prev has a self loop), 1 when the hop source has the directed edge prev -> y
 *     (dis[prev][y] == 2, or y in prev's sorted out-list: the test pn_sample_paths_biased makes), 2 otherwise.
 *   mass[r, w, t, c]  the sum of N(ids[t] -> y) over the y of class c; the three sum to 2^62 over a non-empty table.
 *   cls[r, w, t]      the class of ids[t+1]; 3 = none.
 *     Transition 0 has no prev, and a prev outside [0, n) classifies nothing: cls = 3 and mass = 0 there.
 *     p and q do not enter: the accept probabilities are applied by the caller (pathnet_amd/pathprob.py), so one call
 *     serves every (p, q).
 *   counters          {bad_ids, empty_tables, impossible, 0}.  A transition with ids[t] or ids[t+1] outside [0, n) has
 *     num = 0, mass = 0, cls = 3, adds the number of its ids that are outside (1 or 2) to bad_ids -- so a bad id in the
 *     middle of a path is seen by the two transitions it belongs to -- and never indexes a table.  A transition inside the
 *     graph from a node with an empty table has num = 0 and counts in empty_tables; one from a non-empty table with N = 0
 *     counts in impossible.
 * Every output pointer may be NULL: not wanted, never written.  No floating point is used: every sum is a 64-bit integer
 * add, so the result depends neither on the launch geometry nor on any order.
 * Asynchronous on `stream`: nothing is read back.  counters is zeroed by the call.  L == 1 or rows == 0 is valid and only
 * zeroes the counters.  Argument errors fail with PN_ERR_ARG before any device call: null tables or out, null ids with
 * rows > 0; n < 1, W < 1, L < 1, rows < 0; null triples, or neither off nor node_ref; second_order with neither a dense hop table nor all four
 * CSR arrays (the walker's notion of a hop source, though only the out-lists are read); mass or cls without second_order;
 * a negative workspace size, or a short or missing workspace when the query asks for one.  The query needs no device
 * and answers 0 today (a transition is summed in registers); the workspace may be NULL when it does. */
typedef struct pn_path_prob_out {      /* device pointers, caller-owned; NULL = not wanted, never written */
    int64_t *num;                      /* [rows, W, L-1]     N(ids[t] -> ids[t+1]), numerator over 2^62 */
    int64_t *mass;                     /* [rows, W, L-1, 3]  second order only: class masses given prev */
    uint8_t *cls;                      /* [rows, W, L-1]     second order only: class of ids[t+1]; 3 = none */
    int64_t *counters;                 /* [4] zeroed by the call: {bad_ids, empty_tables, impossible, reserved 0} */
} pn_path_prob_out;

int pn_path_prob_workspace_bytes(const pn_sampler_tables *tables, int32_t W, int32_t L, int64_t rows, int32_t second_order,
                                 int64_t *bytes);
int pn_path_prob(pn_context *ctx, const pn_sampler_tables *tables, int32_t W, int32_t L, int64_t rows,
                 const int32_t *ids /* dev [rows, W, L] */, int32_t second_order, const pn_path_prob_out *out,
                 void *workspace, int64_t workspace_bytes, void *stream);

/* ================================================================================================
 * Path file.  The on-disk interface between sampler and trainer: one line per path,
 * "[v0, v1, ..., v_{L-1}, d0, ..., d_{L-1}]\n"  (writer gen_merw.cpp:189-206; reader
 * PathNet_run.py:418-423 and :325-334, which requires the trailing "]\n").
 * ============================================================================================== */
int pn_paths_write_text(const char *path, const int32_t *ids, const uint8_t *codes, int64_t npaths, int32_t L,
                        int32_t append);
/* cap = 0: count lines only (ids/codes may be NULL).  Otherwise fills up to cap paths. */
int pn_paths_read_text(const char *path, int32_t L, int32_t *ids, uint8_t *codes, int64_t cap, int64_t *npaths);

/* Binary sidecar of the same content (the reference re-parses 10^7..10^8 text lines per run,
 * PathNet_run.py:418-423 / :325-334).  Layout: 32-byte header {char magic[8] = "PNPATHS1", int32 L, int32 reserved,
 * int64 npaths, int64 reserved}, then npaths*L int32 ids, then npaths*L uint8 codes.  Lossless w.r.t. the text. */
int pn_paths_write_bin(const char *path, const int32_t *ids, const uint8_t *codes, int64_t npaths, int32_t L);
/* cap = 0: read only the header (*npaths, *L_out).  Otherwise fills ids/codes (cap >= npaths). */
int pn_paths_read_bin(const char *path, int32_t *L_out, int32_t *ids, uint8_t *codes, int64_t cap, int64_t *npaths);

/* ================================================================================================
 * Aggregator ("PAGG"): the forward() of PathNet (PathNet_run.py:172-211), PathNet_homo (:239-278)
 * and PAGG (baseline/GPRGNN/src/copy.py:327-359), and its backward (autograd in the reference,
 * PathNet_run.py:351).
 * ============================================================================================== */
#define PN_VARIANT_HETERO 0 /* class PathNet      : LSTM, flip/time-major quirk, softmax(LeakyReLU) attention */
#define PN_VARIANT_HOMO 1   /* class PathNet_homo : LSTM, ReLU after fc0 and after the bank, (1+att) attention */
#define PN_VARIANT_PAGG 2   /* class PAGG         : tanh RNN, plain mean over paths */

typedef struct pn_pagg_shape {
    int32_t variant;
    int32_t N, F, H, C; /* nodes, input features, hidden (a multiple of 32: fused recurrent kernels up to 256, a
                         * step-by-step recurrence on the fp32 MFMA GEMM up to 1024), classes */
    int32_t S, W, L;    /* masked nodes this call aggregates (rows of out), paths per node, path length */
    /* A call may aggregate a slice of a larger batch: S_total masked nodes in the batch (0 means S), of which this
     * call computes the pooling groups [group_begin, group_begin + S).  ids / codes / sel / the explicit masks always
     * describe the WHOLE batch ([S_total, ...]); out / g_out are the S rows of the slice.  For HOMO / PAGG a group
     * only reads its own rows; HETERO's [W, S] re-view (PathNet_run.py:196-197) makes group g read paths of other
     * masked nodes of the batch -- with the whole batch's index arrays at hand a slice is still exactly the rows the
     * reference computes for the whole batch.  This is what node sharding across GPUs (pathnet_amd/dist.py) and the
     * micro-batches below rely on.  Dropout counters are functions of the position in the whole batch. */
    int32_t S_total, group_begin;
    /* > 0: the library walks the S groups in micro-batches of at most batch_groups groups, so that the per-path
     * tensors of the workspace are sized by batch_groups * W paths instead of S * W (configs with more paths than
     * HBM holds saved tensors for).  With more than one micro-batch the forward keeps no per-path tensors and the
     * backward re-runs each micro-batch's recurrence before its BPTT (same seed, same masks); gradients accumulate
     * across micro-batches and the node-level backward (bank, fc0) runs once at the end.  0: one batch. */
    int32_t batch_groups;
    /* The path encoder between the distance bank and the pooling.  0: the variant's own (LSTM for PathNet / PathNet_homo,
     * tanh RNN for PAGG).  The others are the ablation rows of the paper's table ("Changing the PAGG class can deliver
     * other variants", README.md:118; no code in the reference): GRU = torch.nn.GRU's cell (weights [3H, H], gate order
     * r, z, n), MEAN / SUM = the mean / the sum of a path's (dropped-out) step rows, no recurrent weights (w_* / b_* NULL). */
    int32_t cell;
    /* Non-zero: the backward adds in a fixed order -- bitwise identical gradients from run to run for the same inputs,
     * seed and shape (torch.use_deterministic_algorithms for this path).  The default backward scatters the gather's
     * gradient and splits the weight-gradient reductions with fp32 atomics, whose order the hardware picks; here the
     * scatter contributions are stored, sorted by destination row (stable radix sort) and summed in the order of the
     * path steps, and every split reduction stores its chunk sums and adds them in chunk order.  Costs workspace
     * (pn_pagg_workspace_bytes accounts for it: ~600 B per path step at H = 128) and time; the
     * forward computes the same values either way. */
    int32_t deterministic;
    /* Touched-row compaction of the distance bank (Z / dZ hold only the (node, code) rows this call's paths gather,
     * DESIGN.md section 3): 0 = the library decides from the shape (when the path steps cannot touch half of the N * L
     * rows), 1 = always, 2 = never.  The decision is part of the workspace layout, so pn_pagg_workspace_bytes, the
     * forward and the backward of one call must be given the same value. */
    int32_t compact;
    /* Arithmetic of the three recurrent GEMMs (hidden size <= 256; inputs, outputs and accumulation are fp32 either way):
     *   0 / PN_SEQ_MATH_F16X2: every fp32 product as THREE fp16 MFMAs over two-plane splits of both operands
     *       (a = a_hi + a_lo, |a_lo| <= 2^-12 |a|; a.b = a_hi b_hi + a_hi b_lo + a_lo b_hi + O(2^-24 |a||b|)), each operand
     *       scaled by a power of two taken from its largest magnitude so that the planes sit at the top of fp16's range;
     *   PN_SEQ_MATH_BF16X3: SIX bf16 MFMAs over three-plane splits, no scaling (rounds 1-3).
     * Both are as accurate as an fp32 FMA chain for operands whose magnitudes span less than ~2^16 below the largest
     * (DESIGN.md section 4); the bf16 mode keeps that for any span.  Explicit dropout masks must satisfy |m| <= 16. */
    int32_t seq_math;
} pn_pagg_shape;
#define PN_SEQ_MATH_DEFAULT 0
#define PN_SEQ_MATH_BF16X3 1
#define PN_SEQ_MATH_F16X2 2
#define PN_COMPACT_AUTO 0
#define PN_COMPACT_ON 1
#define PN_COMPACT_OFF 2
/* pn_path_weights.norm */
#define PN_PATH_NORM_SUM 0    /* the weights of a group are scaled to sum to W (integer weights = repeated paths) */
#define PN_PATH_NORM_COUNT 1  /* the weights are applied as given: a group with fewer live paths pools less */
#define PN_CELL_DEFAULT 0
#define PN_CELL_LSTM 1
#define PN_CELL_RNN 2
#define PN_CELL_GRU 3
#define PN_CELL_MEAN 4
#define PN_CELL_SUM 5

/* All pointers are device pointers.  Weights use the reference state_dict layout
 * (nn.Linear weight [out, in]; LSTM/RNN weight_ih/hh [G*H, H] with torch gate order i,f,g,o).
 * Gradient pointers (g_*) may be NULL in forward; in backward a NULL gradient is skipped. */
typedef struct pn_pagg_args {
    pn_pagg_shape shape;
    /* inputs */
    const float *X;       /* [N, F] */
    const int32_t *ids;   /* [S_total, W, L] path node ids of the whole batch, path-major as in the path file */
    const uint8_t *codes; /* [S_total, W, L] distance codes */
    const int32_t *sel;   /* [S_total] node index of each masked node (nonzero(indices));
                           * with index_rows_local: the slice's rows only ([S, ...]) */
    /* parameters */
    const float *fc0_w, *fc0_b;   /* [H, F], [H] */
    const float *bank_w, *bank_b; /* [L, H, H], [L, H]   nets.<d> / nei<d> stacked by d */
    const float *w_ih, *w_hh;     /* [G*H, H]            G = 4 (LSTM), 1 (RNN), 3 (GRU); NULL for the mean / sum cells */
    const float *b_ih, *b_hh;     /* [G*H] */
    const float *att_w, *att_b;   /* [2H], [1]           unused for PN_VARIANT_PAGG */
    const float *fc2_w, *fc2_b;   /* [C, 2H], [C] */
    /* dropout (F.dropout(training=True) on the recurrent input [L,P,H] and on the classifier input
     * [S,2H]): p = 0 disables.  With mask pointers set, those multiplicative masks (already scaled by
     * 1/(1-p)) are used instead of the built-in Philox masks -- this is how parity tests inject the
     * reference's mask. */
    float p_seq, p_cls;
    uint64_t seed;
    const float *mask_seq; /* [L, S_total*W, H] (positions in the whole batch) or NULL */
    const float *mask_cls; /* [S_total, 2H] or NULL */
    /* outputs */
    float *out; /* [S, C] logits of the slice's masked nodes */
    /* saved-for-backward + scratch, sized by pn_pagg_workspace_bytes */
    void *workspace;
    int64_t workspace_bytes;
    /* backward only */
    const float *g_out; /* [S, C] upstream gradient */
    float *g_X;         /* [N, F] or NULL */
    float *g_fc0_w, *g_fc0_b, *g_bank_w, *g_bank_b, *g_w_ih, *g_w_hh, *g_b_ih, *g_b_hh, *g_att_w, *g_att_b,
        *g_fc2_w, *g_fc2_b;
    /* node-sharded multi-GPU use (pathnet_amd/dist.py): when Xh_in is set the projected feature matrix
     * Xh [N, H] (fc0 output, after ReLU for HOMO) is taken from the caller -- every rank projects its
     * own rows with pn_gemm_f32 and the rows are all-gathered over RCCL -- and X / fc0_* are ignored.
     * In backward g_Xh [N, H] then receives d loss / d Xh (to be reduce-scattered to the row owners and
     * finished with pn_linear_backward) instead of g_fc0_* / g_X. */
    const float *Xh_in;
    float *g_Xh;
    /* Overlap of those two collectives with the library's own work (both may be NULL; hipEvent_t handles, not captured into
     * graphs).  Xh_ready: recorded by the caller on ITS communication stream after the all-gather -- the forward makes `stream`
     * wait for it only where Xh_in is first read (the distance bank), so the touched-row marking, the index plan and the
     * weight packing run under the all-gather.  g_Xh_ready: recorded by the backward on `stream` as soon as g_Xh is complete
     * -- before the distance bank's and the recurrent weight gradients, which then run under the caller's reduce-scatter. */
    void *Xh_ready;
    void *g_Xh_ready;
    /* inference: non-zero skips writing the saved-for-backward tensors (gates, cell states, [x|h] rows --
     * ~3.6 KB per path step); pn_pagg_backward must not follow such a forward. */
    int32_t no_save;
    /* 1: Xh AND the dense Z = bank(Xh) [N * L, H] of the previous pn_pagg_forward on this workspace are still valid (same
     * X, same fc0 / bank weights, same N, H, L, and that forward was NOT compact): skip fc0 and the bank.
     * 2: only Xh is valid (the previous forward ran over compact rows, whose Z belongs to its own batch): skip fc0,
     * compute the bank.  A compact call always computes its own rows of the bank, whatever the value.
     * The validation and test forwards of an epoch (PathNet_run.py:362, :378) share the tables this way; the caller
     * vouches for the precondition -- pn_pagg_shape_info tells whether a shape runs compact. */
    int32_t reuse_tables;
    /* non-zero: ids / codes / sel hold only the rows of this call's slice ([S, W, L] / [S]: rows group_begin ..
     * group_begin + S of the batch) instead of the whole batch.  HOMO / PAGG only (a group reads nothing but its own
     * rows there); positions in the batch -- dropout counters, explicit masks -- stay batch-wide.  This is what a rank
     * of the node-sharded path passes: its own paths, no exchange of index arrays. */
    int32_t index_rows_local;
    /* dev or NULL: the dropout seed is step_state->seed, read when the kernels run (hipGraph replay), instead of `seed` */
    const pn_step_state *step_state;
    /* Optional outputs of pn_pagg_forward (dev or NULL; NULL: not written, the forward is what it is without them), rows of
     * the slice's S masked nodes like `out`:
     *   out_embed [S, 2H]: the classifier input BEFORE the classifier's dropout, [Xh[sel[s]] | pooled paths of s] (layer1 =
     *       torch.cat((ego, h_n), dim=1) at PathNet_run.py:207 / :275, copy.py:355, ahead of F.dropout); in training it
     *       holds the sequence dropout of the same call.
     *   out_path_weight [S, W]: the coefficient that multiplies member j's final hidden state in row s's mean -- the softmax
     *       weight (HETERO), 1 + att (HOMO), 1 (PAGG).
     *   out_path_state [S, W, H]: member j's final hidden state.
     * Members are in the reference's order: for HOMO / PAGG member j of row s is path j of masked node s; for HETERO it is
     * slot q = j * S_total + (group_begin + s) of the reference's scrambled LSTM batch (the [W, S] re-view of
     * PathNet_run.py:196-197), whose steps come from other masked nodes' paths (oracle/pagg_oracle.py: plan).
     * pn_pagg_backward's re-runs of micro-batches write none of them.
     * g_embed [S, 2H] (pn_pagg_backward, dev or NULL): upstream gradient on out_embed.  The backward computes the gradients
     * of sum(out * g_out) + sum(out_embed * g_embed); one of g_out / g_embed may be NULL (g_out NULL: g_fc2_* are zero).
     * pn_pagg_train_step refuses all four (PN_ERR_ARG). */
    float *out_embed;
    float *out_path_weight;
    float *out_path_state;
    const float *g_embed;
} pn_pagg_args;

int pn_pagg_workspace_bytes(const pn_pagg_shape *shape, int64_t *bytes);
/* What the library decides from a shape: out[0] = 1 when the call runs over compact rows of the distance bank, out[1] =
 * rows of Z / dZ, out[2] = micro-batches, out[3] = PN_SEQ_MATH_* the recurrent GEMMs will use (0: the shape has none). */
int pn_pagg_shape_info(const pn_pagg_shape *shape, int64_t out[4]);
/* The operand ranges of the fp16 x 2 recurrent kernels (seq_math = PN_SEQ_MATH_F16X2) live in the workspace, in device memory,
 * written by the forward's kernels.  x_bits: bit pattern of max |Z| over the distance-bank rows the call gathers from (the
 * power-of-two scale of the gathered rows is taken from it).  x_esum / x_cnt: sum and count of the biased fp32 exponents of the
 * non-zero maxima of a sample of tiles of Z, so that  ((x_bits >> 23) & 255) - x_esum / x_cnt  is how far, in bits, the largest
 * value sits above the typical tile.  The two-plane fp16 split keeps 22 bits of a row within ~2^18 of the maximum and loses one
 * bit per factor of two below that: a caller that sees a spread beyond ~18 bits (a single spike row 2^20 times the typical one)
 * should run the call with seq_math = PN_SEQ_MATH_BF16X3, whose planes carry fp32's own exponent range.  The library itself never
 * reads x_esum / x_cnt (no host round trip in a call); pathnet_amd/modules.py reads them back asynchronously. */
typedef struct pn_seq_range {
    uint32_t x_bits;
    int32_t x_esum;
    uint32_t x_cnt;
    uint32_t w_ih_bits, w_hh_bits, dg_bits;     /* max |W_ih|, max |W_hh|, max |dG| of the last BPTT */
} pn_seq_range;
/* *offset = byte offset of the call's pn_seq_range in its workspace, or -1 when the shape runs no fp16 recurrent kernel */
int pn_pagg_range_offset(const pn_pagg_shape *shape, int64_t *offset);
/* The stream on which a call with this shape, made on `stream`, READS its path arrays (ids / codes: the index plan and the
 * touched-row marks): the context's second stream when the call forks them off (a context, one micro-batch, stages not timed one
 * by one), else `stream` itself.  A producer of the paths enqueued THERE -- the sampler of a training loop: pn_sample_paths with
 * *out as its stream, right before the call -- is ordered before its readers and behind those of the previous call without an
 * event on `stream`, and runs under whatever that stream still holds of the previous step (the recurrent weight gradient):
 * the walk leaves the step's critical path.  Ask before every call (the answer follows pn_profile_configure).  A call that
 * reads the paths on `stream` before it forks (the touched-row marks of a compact shape) first waits for the work already on
 * the second stream, so a producer placed there by the answer for another shape is still ordered before it.  A sampler driven
 * by a pn_step_state reads epoch and seed from device memory: it stays on the stream that advances the state
 * (pn_step_state_advance, pn_adam_step_advance), not on *out. */
int pn_pagg_paths_stream(pn_context *ctx, const pn_pagg_shape *shape, void *stream, void **out);
/* out = forward(...) (and the optional out_embed / out_path_weight / out_path_state).  Leaves what backward needs in the
 * workspace. */
int pn_pagg_forward(pn_context *ctx, const pn_pagg_args *args, void *stream);
/* Gradients of sum(out * g_out) [+ sum(out_embed * g_embed)] w.r.t. every parameter (overwritten, not accumulated) and X.
 * Must follow a pn_pagg_forward (no_save = 0) on the same args/workspace with the same weights: the saved tensors, the index
 * plan and -- fp16 mode -- the weights' operand ranges and their packed planes for the BPTT (written by the forward's packing
 * stream, off the backward's critical path) live there. */
int pn_pagg_backward(pn_context *ctx, const pn_pagg_args *args, void *stream);
/* One call for the aggregator's part of a training step (PathNet_run.py:343-351: forward, CrossEntropyLoss, backward):
 *   out [S, C] = forward(...);  loss[0] = grad_scale * sum over the S rows of softmax-cross-entropy(out[r], target[r]);
 *   every g_* of args = d loss / d parameter (g_out is not read).
 * grad_scale = 1 / S gives torch.nn.CrossEntropyLoss()'s mean (a rank of the node-sharded step passes 1 / S_total).
 * target: dev int64 [S] class indices of the slice's rows; loss: dev float.  Same values as pn_pagg_forward +
 * pn_cross_entropy + pn_pagg_backward; what it saves is the second forward of every micro-batch: with batch_groups > 0
 * pn_pagg_forward keeps no per-path tensors and pn_pagg_backward has to re-run each micro-batch's recurrence, here a
 * micro-batch's forward, loss gradient and backward follow each other on the tensors still in the workspace.
 * A target outside [0, C) is handled as by pn_cross_entropy: *loss is NaN, the row's d loss / d logits is zero (every
 * gradient stays finite: the recurrent kernels' range scaling is not specified for non-finite values).  Class weights,
 * ignore_index and label smoothing: pn_pagg_train_step_loss (with pn_loss_spec, below). */
int pn_pagg_train_step(pn_context *ctx, const pn_pagg_args *args, const int64_t *target, float grad_scale, float *loss,
                       void *stream);

/* ---- fc0 over prepared sparse features (pn_sparse.hip): bag-of-words X, its non-zeros extracted once -------------------
 * Cora's feature matrix is 98.7 % zeros, and it is the dataset: the same tensor in every step of a training run.  Its
 * structure is extracted ONCE into two indexes in device memory, and the three calls above then have a twin that takes
 * them and runs fc0's forward and weight gradient over the non-zeros instead of the dense GEMMs.  Added without an ABI
 * bump: five new symbols and one new struct, no existing struct or signature changed (pn_pagg_args is as it was: the
 * features travel as an argument of their own), so pn_abi_version keeps answering 12.
 *
 * An element is a non-zero when x != 0.0f: -0.0f is not one, NaN and Inf are.
 *   CSR: row_off int32 [N + 1]; col / val [nnz]: the features and values of row n at row_off[n] .. row_off[n + 1], features
 *        ascending.
 *   CSC: col_off int32 [F + 1]; row / valc [nnz]: the nodes and values of column f at col_off[f] .. col_off[f + 1], nodes
 *        ascending.
 * Two steps, because the caller owns every buffer: pn_sparse_count fills and scans both offset arrays (asynchronous); the
 * caller reads nnz = row_off[N] (= col_off[F]) back, allocates the four [nnz] arrays and calls pn_sparse_fill, which
 * writes them from the same X.  Positions come from integer counts and prefix sums alone: the same index in every run.
 * Limits, PN_ERR_ARG before any launch: N, F >= 1 and N * F <= 2^28 (positions stay in int32; the build is a one-time
 * cost and is not tuned: a lane per column walks the rows).  nnz = 0 is valid (the [nnz] pointers may then be NULL). */
typedef struct pn_sparse_features {   /* device pointers, caller-owned */
    int64_t nnz;
    int32_t *row_off;                 /* [N + 1] */
    int32_t *col;                     /* [nnz] */
    float *val;                       /* [nnz] */
    int32_t *col_off;                 /* [F + 1] */
    int32_t *row;                     /* [nnz] */
    float *valc;                      /* [nnz] */
} pn_sparse_features;
int pn_sparse_count(pn_context *ctx, const float *X, int32_t N, int32_t F, int32_t *row_off, int32_t *col_off, void *stream);
int pn_sparse_fill(pn_context *ctx, const float *X, int32_t N, int32_t F, const pn_sparse_features *features, void *stream);
/* pn_pagg_forward / pn_pagg_backward / pn_pagg_train_step with the prepared features of args->X (features = NULL: exactly
 * those calls).  The caller vouches that the features were built from the X the call is given, with its N and F.  With them
 *   Xh[n, :] = act(fc0_b + sum_k val_k * fc0_w[:, col_k])          fp32 FMAs in ascending feature order,
 *   g_fc0_w[h, f] = sum over column f of valc * dXh'[n, h]          four interleaved partial sums added in a fixed order,
 * g_fc0_b is the column sum of dXh' and g_X stays the dense GEMM.  Every sum has a fixed order, so the deterministic mode
 * takes the same route.  The features are ignored -- the dense kernels run, unchanged -- when Xh_in is set, when the hidden
 * size is above 256, and when the context knob PN_FC0_SPARSE is 0 (default 1; the A/B switch).  The one place where the
 * routes differ beyond rounding: a zero of X times a non-finite weight is NaN on the dense route and absent here.  The
 * forward transposes fc0_w into the workspace on every call (the weights change from step to step; X does not). */
int pn_pagg_forward_sparse(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *features, void *stream);
int pn_pagg_backward_sparse(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *features, void *stream);
int pn_pagg_train_step_sparse(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *features,
                              const int64_t *target, float grad_scale, float *loss, void *stream);

/* Stand-alone stages of the same path, exposed for measurement and tests. */
/* rows[q, t, :] = table[(node(q,t) * L + code(q,t)), :] for the variant's index plan: the
 * [P, L, H] path-feature gather with the distance code fused in (PathNet_run.py:179 / :246). */
int pn_pagg_gather(pn_context *ctx, const pn_pagg_shape *shape, const float *table /* [N, L, H] */, const int32_t *ids,
                   const uint8_t *codes, float *rows /* [P, L, H] */, void *stream);

/* C[m*ldc + n] = act( sum_k A[m*sAm + k*sAk] * B[n*sBn + k*sBk] + bias[n] ): the fp32 MFMA GEMM
 * every dense layer of the path uses (nn.Linear: sAk = sBk = 1).  One stride of each operand must
 * be 1.  bias may be NULL; relu != 0 applies max(0, .). */
int pn_gemm_f32(const float *A, int64_t sAm, int64_t sAk, const float *B, int64_t sBn, int64_t sBk, float *C,
                int64_t ldc, const float *bias, int32_t M, int32_t N, int32_t K, int32_t relu, void *stream);

/* Y [rows, out_f] = act(X [rows, in_f] . W^T + b): nn.Linear (+ReLU when relu != 0), fc0 of the path for a block of
 * rows (PathNet_run.py:175 / :242) -- what a rank computes before the all-gather of the node-sharded path.  With a
 * device workspace of at least PN_LINEAR_SPLIT_MAX * rows * out_f * 4 bytes the reduction dimension is split over
 * workgroups (deterministic: chunk sums + a fixed-order finish), which is what fills the GPU when rows * out_f is
 * small; workspace may be NULL (one workgroup per output tile). */
#define PN_LINEAR_SPLIT_MAX 8
int pn_linear_forward(pn_context *ctx, const float *X, const float *W, const float *b, int32_t rows, int32_t in_f, int32_t out_f,
                      int32_t relu, float *Y, void *workspace, int64_t workspace_bytes, void *stream);

/* Backward of Y = act(X . W^T + b) for `rows` rows (nn.Linear, fc0 of the path: PathNet_run.py:175 / :242):
 * dY [rows, out_f] is gated by [gate > 0] when gate != NULL (ReLU backward, gate = Y), then
 * g_W [out_f, in_f] = dY^T . X,  g_b [out_f] = colsum(dY),  g_X [rows, in_f] = dY . W.  Any output may be NULL.
 * The weight gradient splits the `rows` reduction over workgroups.  With a device workspace of at least
 * PN_LINEAR_BWD_SPLIT_MAX * (out_f * in_f + out_f) * 4 bytes the chunk sums are stored and added in a fixed order --
 * bitwise reproducible, what the deterministic mode of the aggregator (pn_pagg_shape.deterministic) pairs with on the
 * node-sharded path; with workspace NULL the chunks are added with fp32 atomics (last bits vary from run to run). */
#define PN_LINEAR_BWD_SPLIT_MAX 32
int pn_linear_backward(pn_context *ctx, const float *dY, const float *gate, const float *X, const float *W, int32_t rows, int32_t in_f,
                       int32_t out_f, float *g_W, float *g_b, float *g_X, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the MERW transition probabilities: what writes edge_input/<name>.in ----------------------
 * preprocess/compute_merw.py:107-121 compute_merw(A), as init_rw.py:76 calls it: (lambda, psi) = dominant eigenpair of
 * the symmetric adjacency matrix, p[k] = A[i,j] psi[j] / (lambda psi[i]) for every stored entry k = (i, j).
 * A is CSR on the device (row_off [n+1], col [nnz], val [nnz] or NULL for all ones).  Power iteration on A + I in fp64,
 * deterministic; converged when |A x - lambda x| <= tol (lambda + 1) (tol <= 0: 1e-13; max_iter < 1: 100000).
 * Outputs: p dev [nnz], psi dev [n] (unit 2-norm, positive), *lambda and *iters on the host.  Fails with the residual in
 * pn_last_error() when it does not converge.  Call it per CONNECTED component: on a disconnected graph the reference's one
 * eigenpair is exact on the dominant component only and eigensolver noise elsewhere (the negative and > 1 "probabilities" of
 * the shipped cora.in / citeseer.in); pathnet_amd/merw_init.py splits the graph and documents what it writes there. */
int pn_merw_workspace_bytes(int32_t n, int64_t *bytes);
int pn_merw_probabilities(int32_t n, int64_t nnz, const int64_t *row_off, const int32_t *col, const double *val,
                          double *p, double *psi, double *lambda, int32_t max_iter, double tol, int32_t *iters,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* ---- training-step glue: the loss and the optimizer of PathNet_run.py:295-297, :346-352 ------
 * Mean softmax cross entropy over `rows` rows of `classes` logits (torch.nn.CrossEntropyLoss(), :297; int64 class
 * targets, no ignore_index / label smoothing -- the reference uses neither): *loss (device float) receives the mean,
 * g_logits [rows, classes] (may be NULL) d loss / d logits = (softmax - onehot) / rows.  The log softmax is formed as
 * (x - max) - log(sum exp(x - max)): its error does not grow with the size of the logits.
 * A target outside [0, classes) -- the -1 that graph datasets give unlabelled nodes, torch's ignore_index = -100 -- is
 * never used as an index: its row contributes NaN to the loss (so *loss is NaN) and zeros to its row of g_logits.  This
 * call has no options; class weights, ignore_index and label smoothing are pn_cross_entropy_ex's (below). */
int pn_cross_entropy(const float *logits, const int64_t *target, int32_t rows, int32_t classes, float *loss,
                     float *g_logits, void *stream);

/* ---- loss options: class weights, ignore_index, label smoothing (torch.nn.CrossEntropyLoss's arguments) ---------------
 * With p = softmax(x_r), lp = (x - max) - log sum exp(x - max), w the class weights (all ones when weight is NULL),
 * Wsum = sum_c w[c], e = label_smoothing, C = classes, and row r KEPT iff has_ignore == 0 or target[r] != ignore_index:
 *   row loss   l_r         = kept * [ (1 - e) w[t] (-lp[t])  +  (e / C) sum_c w[c] (-lp[c]) ]
 *   d l_r / d x_c          = kept * [ (1 - e) w[t] (p_c - [c == t])  +  (e / C) (Wsum p_c - w[c]) ]
 *   D                      = sum over the kept rows of w[t_r]            (the weighted mean's denominator)
 *   loss                   = k * sum_r l_r,   k = grad_scale / D (PN_LOSS_MEAN)  or  grad_scale (PN_LOSS_SUM)
 * which is torch.nn.functional.cross_entropy(weight, ignore_index, label_smoothing, reduction) for grad_scale = 1, but
 * for two cases, where this library's rule -- every gradient stays finite -- wins:
 *   - a target outside [0, C) that is not the ignore value is handled as by pn_cross_entropy: NaN into the loss, a zero
 *     gradient row; it adds nothing to D.  The ignore test comes first: an ignore_index that is a valid class drops that
 *     class's rows.  No address is formed from an unchecked target (a clamped index and selects).
 *   - D == 0 under PN_LOSS_MEAN (every row ignored, or only zero-weight classes among the kept rows): the loss is NaN and
 *     every gradient is ZERO (torch: NaN gradients in the zero-weight case).
 * An ignored row's logits are never looked at for the loss (they may be NaN).  D depends on the targets and is formed ON
 * THE DEVICE, by one workgroup in a fixed order at any row count (the same bits in every run), into the caller's
 * `denominator`; the kernels read it from there, so nothing is read back and a step captured in a hipGraph follows
 * targets whose ignored count changes between replays.  With denominator_given != 0 the calls read the value that is
 * there instead (a rank of a sharded step passes the all-reduced D).  Added without an ABI bump: three new symbols and
 * one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12. */
#define PN_LOSS_MEAN 0
#define PN_LOSS_SUM 1
typedef struct pn_loss_spec {
    const float *weight;        /* dev [C] or NULL */
    int64_t ignore_index;
    int32_t has_ignore;
    float label_smoothing;      /* [0, 1] */
    int32_t reduction;          /* PN_LOSS_MEAN (weighted mean, /D) | PN_LOSS_SUM */
    float grad_scale;           /* multiplies the loss and every gradient; 1 = torch */
    float *denominator;         /* dev float, caller-owned; written with D by the call ... */
    int32_t denominator_given;  /* ... or, when != 0, read (a rank of a sharded step passes the all-reduced D) */
} pn_loss_spec;
/* Argument errors of the three calls, PN_ERR_ARG before any launch: spec NULL, label_smoothing outside [0, 1] (or NaN),
 * a reduction that is neither value, PN_LOSS_MEAN without a denominator. */
/* spec->denominator[0] = D of target[0 .. rows) (needs the denominator whatever the reduction; denominator_given is not
 * looked at). */
int pn_loss_denominator(const int64_t *target, int32_t rows, int32_t classes, const pn_loss_spec *spec, void *stream);
/* pn_cross_entropy with the options: *loss and g_logits [rows, classes] (may be NULL) as above.  Writes D first unless
 * denominator_given (PN_LOSS_SUM: only when a denominator is set).  With every option off (weight NULL, has_ignore 0,
 * label_smoothing 0, PN_LOSS_MEAN, grad_scale 1) the loss and the gradient have pn_cross_entropy's bits. */
int pn_cross_entropy_ex(const float *logits, const int64_t *target, int32_t rows, int32_t classes, const pn_loss_spec *spec,
                        float *loss, float *g_logits, void *stream);
/* pn_pagg_train_step_sparse (features may be NULL: pn_pagg_train_step) with the options: spec->grad_scale stands where
 * grad_scale stood, but multiplies the REDUCED loss (1 with PN_LOSS_MEAN = torch's weighted mean; the plain call's
 * grad_scale = 1 / S is PN_LOSS_MEAN's 1 when no row is ignored and no weight given).  D is formed once, over the call's
 * whole S rows, before the micro-batch loop.  Every route of the plain call has its option-aware twin (the one-launch
 * pooling step, the three launches of the deterministic mode and PN_POOL_STEP=0/2); the deterministic mode is bitwise
 * reproducible with options as without. */
int pn_pagg_train_step_loss(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *features /* may be NULL */,
                            const pn_loss_spec *spec, const int64_t *target, float *loss, void *stream);

/* ---- per-path weights in the pooling (pn_pool.hip) --------------------------------------------------------------------
 * The aggregators pool a node's W paths with fixed coefficients (pn_pagg_args.out_path_weight); a pn_path_weights lets the
 * caller weigh every path, or leave paths out.  It travels as an argument of its own, like the prepared sparse features:
 * four new symbols and one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 * (pn_pagg_args ends with the version-12 fields, and bindings written against it stay valid.)
 *
 * weight: dev fp32, one entry per sequence slot q of the batch, laid out like ids without its last axis: [S_total, W], or
 * the slice's rows [S, W] with index_rows_local (the same q - first-row indexing as ids).  For HOMO / PAGG entry [s, w]
 * belongs to path w of masked node s; for HETERO it belongs to slot q of the reference's scrambled batch (see
 * out_path_weight), the slot whose final hidden state the pooling reads -- NOT to path w of row s.  A weight that is no
 * finite positive number counts as 0.  With a group's live weights w_m, their sum Om and kappa = W / Om (norm =
 * PN_PATH_NORM_SUM) or 1 (PN_PATH_NORM_COUNT), kappa = 0 for an empty group (Om = 0: pooled = 0, no gradient):
 *   PAGG    pooled = (1/W) sum kappa w_m h_m
 *   HOMO    pooled = (1/W) sum kappa w_m (1 + s_m) h_m
 *   HETERO  pooled = (1/W) sum kappa a_m h_m,  a_m = w_m e_m / sum_k w_k e_k,  e_m = exp(l_m - max_k l_k), l = LeakyReLU(score)
 *           (the maximum over all members, live or not; every a_m is 0 when the denominator is)
 * All-one weights give the unweighted values bit for bit on the same kernels; integer weights with PN_PATH_NORM_SUM give
 * the unweighted pooling of a row in which path m is written w_m times (pn_path_multiplicity counts them).
 * out_path_weight then reports the coefficient applied: kappa w_m c_m, or kappa a_m for HETERO.  The entry points below treat
 * the weights as data; pn_pagg_backward_paths / pn_pagg_train_step_paths (further down) also return d loss / d weight.  A path
 * of weight 0 still runs through the recurrence and gets d h_n = 0.
 * pw == NULL, or pw->weight == NULL: the unweighted call, exactly.  The backward takes the array its forward took.
 * Micro-batches (the backward's re-runs included), group_begin slices, the deterministic mode, every cell and every H are
 * covered; the training step runs a weighted node through pool_step_kernel (pn_pool.h), never the register-resident one. */
typedef struct pn_path_weights {
    const float *weight;
    int32_t norm;           /* PN_PATH_NORM_* */
} pn_path_weights;
int pn_pagg_forward_weighted(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp /* or NULL */,
                             const pn_path_weights *pw /* or NULL */, void *stream);
int pn_pagg_backward_weighted(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp,
                              const pn_path_weights *pw, void *stream);
int pn_pagg_train_step_weighted(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp,
                                const pn_path_weights *pw, const int64_t *target, float grad_scale, float *loss, void *stream);
int pn_pagg_train_step_loss_weighted(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp,
                                     const pn_loss_spec *spec, const pn_path_weights *pw, const int64_t *target, float *loss,
                                     void *stream);

/* ---- gradients at the per-path interface (pn_pool.hip: pool_bwd_wg_body) -------------------------------------------------
 * The backward with the upstream gradients of out_path_state / out_path_weight as further inputs and d loss / d weight as a
 * further output.  Two new symbols and one new struct; pn_abi_version keeps answering 12.  pg == NULL: pn_pagg_backward_weighted
 * / pn_pagg_train_step_weighted / pn_pagg_train_step_loss_weighted, exactly.
 *   g_path_state   dev fp32 [S, W, H], laid out like out_path_state (rows of the call's groups), 16-byte aligned; added to d h_n
 *   g_path_weight  dev fp32 [S, W], laid out like out_path_weight; with D_m = h_m . d pooled / W + g_path_weight[m] the
 *                  attention's chain and g_weight see D
 *   g_weight       out, dev fp32, laid out and indexed like pn_path_weights.weight, which it needs (else PN_ERR_ARG).  The
 *                  call stores the entry of every member of its S groups (plain stores, no atomics: the same bits in every
 *                  run) and touches no other: the caller of a group_begin slice zero-fills the rest.  0 where the weight is not
 *                  live and in an empty group.  With T = sum_m coef_m D_m, r_j = coef_j / w_j:
 *                      PAGG / HOMO   "count"  r_j D_j           "sum"  r_j D_j - T / Om
 *                      HETERO        "count"  r_j (D_j - T)     "sum"  r_j (D_j - T / kappa) - T / Om
 * pn_pagg_backward_paths takes any subset of g_out, g_embed, g_path_state and g_path_weight (at least one).
 * pn_pagg_train_step_paths (spec == NULL: the plain mean with grad_scale; else the options, whose grad_scale counts) takes
 * g_weight only -- g_path_state / g_path_weight there are PN_ERR_ARG -- and g_weight carries the step's grad_scale and loss
 * options like every other gradient of the step.  Micro-batches (the re-runs included), group_begin slices, index_rows_local,
 * the deterministic mode, every cell and every H are covered. */
typedef struct pn_path_grads {
    const float *g_path_state;
    const float *g_path_weight;
    float *g_weight;
} pn_path_grads;
int pn_pagg_backward_paths(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp, const pn_path_weights *pw,
                           const pn_path_grads *pg /* or NULL */, void *stream);
int pn_pagg_train_step_paths(pn_context *ctx, const pn_pagg_args *args, const pn_sparse_features *sp,
                             const pn_loss_spec *spec /* or NULL */, const pn_path_weights *pw, const pn_path_grads *pg,
                             const int64_t *target, float grad_scale, float *loss, void *stream);

/* One Adam update of a list of tensors in a single launch, with the semantics of torch.optim.Adam(lr, betas, eps,
 * weight_decay) (:295-296): g += weight_decay * p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).  `step` counts from 1.  All pointers are device
 * fp32 arrays of `count` elements; exp_avg / exp_avg_sq are the caller-owned optimizer state (zero before step 1). */
#define PN_ADAM_MAX_TENSORS 32
typedef struct pn_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t count;
} pn_adam_tensor;
int pn_adam_step(const pn_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int64_t step, const pn_step_state *step_state /* dev or NULL: replaces step */,
                 void *stream);
/* The same update with step_state's step count, after which the state is moved to the NEXT step by the update's own last
 * launch (the workgroup that finishes last does what pn_step_state_advance does): a training loop whose steps end in this call
 * needs no pn_step_state_advance launch in front of the next one -- ~7 us of a 0.93 ms step at the headline shape.  Uses the
 * low 32 bits of step_state->reserved as a ticket counter (zero between calls). */
int pn_adam_step_advance(const pn_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                         float weight_decay, pn_step_state *step_state /* dev */, void *stream);

/* ---- optimizer options (pn_optim.hip): gradient-norm clipping, decoupled weight decay, amsgrad, a device-side learning-
 * rate schedule and a non-finite guard -----------------------------------------------------------------------------------
 * Added without an ABI bump: six new symbols and three new structs, no existing struct or signature changed, so
 * pn_abi_version keeps answering 12.  pn_adam_step / pn_adam_step_advance are untouched; a call with every option off
 * (flags 0, max_grad_norm 0, PN_LR_CONSTANT, warmup_steps 0) is their update on the new kernel (the same operations, not
 * promised to round the same: the bias corrections are always formed on the device here).
 * Everything here is asynchronous on `stream` and capturable: no allocation, no synchronisation, no memset, nothing read
 * back.  No workgroup waits for another: the norm is handed from launch to launch through the state buffer.
 *
 * The state buffer (dev, caller-owned, pn_optim_state_bytes bytes, 8-byte aligned, ZERO before its first use) starts with a
 * pn_optim_report and continues with the partial sums of squares (double, one per workgroup of pn_grad_norm's launches).
 *
 * Order of one update, per element (fp32; coef, lr_now and the bias corrections are formed in double, once per workgroup):
 *   1. g = coef * grad                         coef = min(1, max_grad_norm / (norm + 1e-6)), torch's clip_grad_norm_;
 *                                              the gradient in memory is NOT modified
 *   2. L2:        g += weight_decay * p        (torch.optim.Adam)
 *      decoupled: p *= 1 - lr_now * weight_decay, g as it is   (torch.optim.AdamW)
 *   3. m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
 *   4. amsgrad: vmax = max(vmax, v), and vmax stands under the square root
 *   5. p -= lr_now / (1 - b1^step) * m / (sqrt(v or vmax) / sqrt(1 - b2^step) + eps)
 * Schedule, with e = step - 1 (step from step_state->adam_step when a step state is given, else the argument):
 *   lr_now = lr * warm(e) * decay(max(e - warmup_steps, 0))
 *   warm(e) = start_factor + (1 - start_factor) * min(e, warmup_steps) / warmup_steps      (1 when warmup_steps == 0)
 *   decay(e): PN_LR_CONSTANT 1 | PN_LR_STEP gamma^floor(e / step_size) | PN_LR_EXPONENTIAL gamma^e |
 *             PN_LR_COSINE (lr_min + (lr - lr_min) (1 + cos(pi min(e, t_max) / t_max)) / 2) / lr
 * The cosine stays at lr_min after t_max: the closed form of torch's CosineAnnealingLR, clamped (torch's recursion turns
 * upwards again there; this does not).
 * Non-finite guard, active whenever max_grad_norm != 0 (+inf: the guard alone, coef is exactly 1): when the sum of squares is
 * not finite the call updates NOTHING -- param, exp_avg, exp_avg_sq and max_exp_avg_sq keep their bits -- and the report's
 * `skipped` goes up by one.  The step count advances as it always does (pn_adam_step_ex_advance moves the state, the caller
 * of pn_adam_step_ex passes the next step next time): a skipped step still uses up its place in the schedule and in the
 * bias corrections. */
#define PN_OPTIM_DECOUPLED_WD 1 /* pn_optim_spec.flags */
#define PN_OPTIM_AMSGRAD 2
#define PN_OPTIM_NO_REPORT 4    /* not the step's first update call (a further parameter group): leave the report alone */
#define PN_LR_CONSTANT 0        /* pn_optim_spec.schedule */
#define PN_LR_STEP 1
#define PN_LR_EXPONENTIAL 2
#define PN_LR_COSINE 3
typedef struct pn_optim_spec {
    int32_t flags;          /* PN_OPTIM_* */
    int32_t schedule;       /* PN_LR_* */
    float max_grad_norm;    /* 0: no clipping, the state's partial sums are not read; +inf: the non-finite guard alone */
    int32_t reserved;       /* 0 */
    int64_t warmup_steps;   /* >= 0 */
    double start_factor;    /* [0, 1]: warm(0) */
    int64_t step_size;      /* PN_LR_STEP: >= 1 */
    double gamma;           /* PN_LR_STEP, PN_LR_EXPONENTIAL: > 0 */
    int64_t t_max;          /* PN_LR_COSINE: >= 1 */
    double lr_min;          /* PN_LR_COSINE: 0 <= lr_min <= lr */
} pn_optim_spec;
typedef struct pn_adam_tensor_ex {      /* pn_adam_tensor and amsgrad's running maximum (torch's state key max_exp_avg_sq) */
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *max_exp_avg_sq;  /* PN_OPTIM_AMSGRAD: dev fp32 [count], zero before step 1; otherwise not looked at */
    int64_t count;
} pn_adam_tensor_ex;
typedef struct pn_optim_report {        /* the head of the state buffer; written with plain stores, read by nobody here */
    double grad_norm;       /* the norm of the last pn_grad_norm / pn_clip_grad_norm as the last update saw it; NaN: none taken */
    double lr;              /* lr_now of the last update */
    float clip_coef;        /* coef of the last update (1 without clipping) */
    int32_t n_partials;     /* partial sums behind this struct (pn_grad_norm) */
    int64_t skipped;        /* updates the guard has skipped since the buffer was zeroed */
} pn_optim_report;
/* *bytes = size of the state buffer for lists of up to n_tensors tensors (total_elements: their element count, >= 0).
 * The partial count is bounded by the launch count, not by the model: 256 per PN_ADAM_MAX_TENSORS tensors. */
int pn_optim_state_bytes(int64_t total_elements, int32_t n_tensors, int64_t *bytes);
/* The sum of squares of every grad of the list, accumulated in double, as per-workgroup partials in `state` (only grad and
 * count of each tensor are looked at; at most 256 workgroups per launch, one launch per PN_ADAM_MAX_TENSORS tensors, each
 * summing in a fixed order: the same bits in every run).  The norm itself is formed by the launches that consume it. */
int pn_grad_norm(const pn_adam_tensor *tensors, int32_t n_tensors, void *state, void *stream);
/* The update above.  max_grad_norm != 0 needs `state` and a pn_grad_norm on the same stream before it (taken over every
 * parameter group's gradients when there are several: the norm is global); `state` may be NULL otherwise, and then no
 * report is written.  Argument errors, PN_ERR_ARG before any launch: a null list / spec / pointer of a non-empty tensor,
 * unknown flags or schedule, a negative or NaN max_grad_norm, schedule parameters outside the ranges above, step < 1
 * without a step state. */
int pn_adam_step_ex(const pn_adam_tensor_ex *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                    float weight_decay, const pn_optim_spec *spec, void *state /* dev or NULL */, int64_t step,
                    const pn_step_state *step_state /* dev or NULL: replaces step */, void *stream);
/* ... and the step state moved on by the update's last launch, exactly as pn_adam_step_advance does it (the same ticket
 * in step_state->reserved) -- also on a skipped step. */
int pn_adam_step_ex_advance(const pn_adam_tensor_ex *tensors, int32_t n_tensors, float lr, float beta1, float beta2,
                            float eps, float weight_decay, const pn_optim_spec *spec, void *state,
                            pn_step_state *step_state /* dev */, void *stream);
/* torch.nn.utils.clip_grad_norm_(max_norm) in place in two launches (per PN_ADAM_MAX_TENSORS tensors): pn_grad_norm, then
 * grad *= coef.  The report's grad_norm and clip_coef are written; max_norm > 0, +inf allowed.  A non-finite norm leaves
 * the gradients as they are (clip_coef 1; torch would turn all of them into NaN): test grad_norm. */
int pn_clip_grad_norm(const pn_adam_tensor *tensors, int32_t n_tensors, float max_norm, void *state, void *stream);

/* ---- ensemble prediction over resampled paths (pn_ensemble.hip) ---------------------------------------------------------
 * The logits of a node depend on the W paths the sampler drew for it.  K draws give K logit rows per node; these calls
 * average their class probabilities on the device and say how much the draws disagree.  Added without an ABI bump: four
 * new symbols and one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * The state is ONE caller-owned device allocation of pn_ensemble_state_bytes(rows, C) = rows * (12 C + 16) bytes, 8-byte
 * aligned, laid out as
 *     double  psum [rows, C]   sum over the samples of the class probabilities
 *     double  hsum [rows]      sum over the samples of the sample's entropy
 *     int32_t votes[rows, C]   samples whose largest logit is class c
 *     int32_t count[rows]      samples added
 *     int32_t bad  [rows]      samples refused because a logit was not finite
 * in that order without padding.  All zeros is the empty ensemble: the caller clears it with a memset.
 *
 * pn_ensemble_add: logits is dev fp32 [R, S, C], R samples of the same S rows, sample-major, contiguous.  Logits row s
 * belongs to state row index[s] (dev int32 [S]; NULL: row s, which needs S <= rows).  For every (r, s), in ascending r for
 * a fixed s, by the one thread group that owns the row:
 *   - any of the C logits NaN or +-inf: bad[row] += 1 and nothing else of the row is touched for this sample;
 *   - otherwise, in fp64 on the converted logits: m = max x, e_c = exp(x_c - m), Z = sum e_c, p_c = e_c / Z;
 *     psum[row, c] += p_c;  votes[row, argmax_c x_c] += 1 (the logits themselves, lowest c on ties);
 *     hsum[row] += -sum_c p_c log p_c (0 log 0 = 0);  count[row] += 1.
 * Sums over c: ascending c for C <= 16; above that every lane adds its classes (lane, lane + 64 ... or + 256 ...) in
 * ascending c, the lanes meet in a fixed butterfly and a workgroup's four waves as (w0 + w1) + (w2 + w3): an order that
 * depends on C alone.  There is no floating-point atomic, the result does not depend on the launch geometry, and one call
 * with [R, S, C] leaves the bits of R calls with [1, S, C] in the same order.
 * An index entry outside [0, rows) skips its logits rows and adds R (one per skipped logits row) to status[0] (dev int32,
 * may be NULL).  The same state row named twice in one call is a caller error (two groups would own it).
 *
 * pn_ensemble_finish reads the state and writes what pn_ensemble_out names; every pointer may be NULL = not written.
 * Without a subset it finishes rows 0 .. rows-1 and output j describes row j; with subset (dev int32 [subset_rows]) output j
 * describes row subset[j] (repeats allowed; an entry outside [0, rows) is an empty row), so one state of N rows serves a
 * validation and a test mask.  With n = count[row], for n > 0:
 *   prob[j, c]      fp32   psum / n
 *   label[j]        int64  argmax_c psum, lowest c on ties
 *   vote_label[j]   int64  argmax_c votes, lowest c on ties
 *   confidence[j]   fp32   psum[label] / n
 *   entropy[j]      fp32   -sum_c q log q of the mean distribution q = psum / n, in fp64, rounded once
 *   mutual_info[j]  fp32   max(0, entropy - hsum / n): the part of the uncertainty that comes from the path draw
 *   agreement[j]    fp32   votes[label] / n
 * and for n == 0 zeros and the labels -1.  target (dev int64 [rows], indexed by STATE row, may be NULL) adds
 *   confusion[t, label] += 1 (int64 [C, C]) for rows with 0 <= t < C and label >= 0, t = target[row];
 *   skipped[0] += 1 for a target outside [0, C), skipped[1] += 1 for label == -1 (a row can count in both).
 * Both are ADDED to with integer atomics (exact, order-free): the caller zeroes them, or keeps them to sum several calls.
 *
 * Limits, refused with PN_ERR_ARG before any device call: 1 <= C <= 4096, 0 <= rows, S, subset_rows < 2^31, R >= 1, S > rows
 * without an index, confusion or skipped without a target, subset_rows != 0 without a subset, NULL logits / state / out
 * where they would be read.  rows == 0 and S == 0 are valid and launch nothing.  Asynchronous on `stream`; nothing is read
 * back and nothing is allocated, so a captured step may contain them.  pn_ensemble_state_bytes and pn_ensemble_route need
 * no device.  The route is the work split a shape takes (it depends on C; rows == 0 launches nothing): */
#define PN_ENSEMBLE_ROUTE_NONE 0   /* rows == 0 */
#define PN_ENSEMBLE_ROUTE_THREAD 1 /* C <= 16: a thread per row */
#define PN_ENSEMBLE_ROUTE_WAVE 2   /* 16 < C <= 1024: a wave per row */
#define PN_ENSEMBLE_ROUTE_BLOCK 3  /* 1024 < C <= 4096: a workgroup per row */
typedef struct pn_ensemble_out {   /* device pointers, caller-owned, each may be NULL; n = rows, or subset_rows with a subset */
    float *prob;                   /* [n, C] */
    int64_t *label;                /* [n] */
    int64_t *vote_label;           /* [n] */
    float *confidence;             /* [n] */
    float *entropy;                /* [n] */
    float *mutual_info;            /* [n] */
    float *agreement;              /* [n] */
    int64_t *confusion;            /* [C, C], added to; needs target */
    int64_t *skipped;              /* [2], added to; needs target */
} pn_ensemble_out;
int pn_ensemble_state_bytes(int64_t rows, int32_t C, int64_t *bytes);
int pn_ensemble_route(int64_t rows, int32_t C, int32_t *route);
int pn_ensemble_add(pn_context *ctx, const float *logits /* dev [R, S, C] */, int32_t R, int64_t S, int32_t C,
                    const int32_t *index /* dev [S] or NULL */, int64_t rows, void *state, int32_t *status /* dev or NULL */,
                    void *stream);
int pn_ensemble_finish(pn_context *ctx, int64_t rows, int32_t C, const void *state,
                       const int32_t *subset /* dev [subset_rows] or NULL */, int64_t subset_rows,
                       const int64_t *target /* dev [rows] or NULL */, const pn_ensemble_out *out, void *stream);

/* ---- calibration of ensemble predictions (pn_calib.hip; pn_ensemble_add_scaled in pn_ensemble.hip) ---------------------------
 * Does a confidence of 0.9 mean "right nine times out of ten"?  These calls fit one temperature on validation logits, apply
 * it inside the ensemble and measure the result, all on the device.  Added without an ABI bump: five new symbols and two
 * new structs, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * pn_ensemble_add_scaled is pn_ensemble_add with e_c = exp((x_c - m) * inv), inv = 1 / *tau (dev fp64 [1], read on the
 * device: a fitted temperature never visits the host).  Votes still use the logits themselves.  (x_c - m) * 1.0 is exact,
 * so *tau == 1.0 leaves the bits pn_ensemble_add leaves.  A *tau that is not a finite positive number touches nothing and
 * adds R * S (saturating at 2^31 - 1) to status[0].  Limits as for pn_ensemble_add, and tau must not be NULL.
 *
 * pn_calib_sweep: logits dev fp32 [R, S, C] as for pn_ensemble_add, target dev int64 [S], temps dev fp64 [T], 1 <= T <= 256.
 * For every (row s, temperature t), by the one thread group that owns the pair (G by C alone as in pn_ensemble_route, and
 * the same order of the class sums), in fp64:
 *   per sample r whose C logits are all finite (n_ok of them), in ascending r:
 *       m = max_c x_c, inv = 1 / temps[t], e_c = exp((x_c - m) * inv), p_y = e_y / sum_c e_c        (y = target[s])
 *   row_nll[s, t] = -log((sum_r p_y) / n_ok)
 * A row with a target outside [0, C) (checked first; its logits are not read) or with n_ok == 0 is unused: row_nll = 0.
 * counts (int64 [3], WRITTEN) = {rows used, rows with a bad target, rows without a finite sample}.  A temps[t] that is not a
 * finite positive number is refused: its row_nll entries are 0 and nll[t] = +inf.
 * The workspace (caller-owned, 8-byte aligned, pn_calib_sweep_workspace_bytes(S, T) bytes) starts with row_nll, fp64 [S, T],
 * which the caller may read; the rest is private.  Column sums: the rows are cut into partials of 256 (rows 256 p ..
 * 256 p + 255); a partial adds its rows in ascending s starting from 0.0, and nll[t] adds the partials in ascending p
 * starting from 0.0: an order that depends on S alone.  Then
 *   best (int32 [1])  argmin_t nll[t] over the finite entries, lowest t on ties; -1 when none is finite or no row is used
 *   tau  (fp64 [1])   temps[best], or 1.0 for best == -1
 * so tau is always a member of the grid: a discrete output.  Refinement is a second sweep over a finer grid.
 * S == 0 launches no kernel: best = -1, tau = 1.0, nll and counts zero (memsets on the stream).
 *
 * pn_calib_stats: confidence dev fp32 [n], label and target dev int64 [n], prob dev fp32 [n, C] or NULL, 1 <= B <= 1024 bins.
 * A row is used when label >= 0, 0 <= target < C and confidence is in [0, 1] (NaN is not).  counts (int64 [5], added to,
 * may be NULL) = {used, label < 0, target out of range, confidence refused, prob[target] == 0}; an unused row counts in the
 * first of the three reasons that holds, in that order; the last entry counts the used rows that sums[0] leaves out (with
 * prob only; they stay used everywhere else).  For a used row:
 *   b = min(B - 1, floor((double)conf * B));  bin_count[b] += 1;  bin_correct[b] += (label == target);
 *   bin_conf[b] += llrint((double)conf * 2^32)                    fixed point, 2^-32 units
 * all int64 [B], ADDED to with integer atomics (exact, order-free): the caller zeroes them or keeps them across calls.
 * With prob, for the used rows (sums fp64 [2], added to by one thread):
 *   sums[0] += sum of -log((double)prob[i, target]) over the rows with prob[i, target] > 0
 *   sums[1] += sum of  sum_c ((double)prob[i, c] - [c == target])^2        (classes in ascending c)
 * Rows are cut into partials of 256; a partial is the halving tree (slot j += slot j + h for h = 128, 64, ..., 1) over its
 * 256 row terms, rows past n and unused rows holding 0.0; the partials are added in ascending order starting from 0.0, and
 * that total is added to sums: an order that depends on n alone.
 * With out->order (risk-coverage; err_prefix and aurc need it):
 *   order      int32 [n]  the used rows by descending confidence, ties by ascending row, then the unused rows by ascending
 *                         row (a stable radix sort of key 0x3F800000 - bits(conf), INT32_MAX for an unused row)
 *   err_prefix int32 [n]  rows with label != target among order[0 .. k]
 *   aurc       fp64 [1]   (1 / m) sum_{k = 1 .. m} err_prefix[k - 1] / k over the m used rows (written; 0 for m == 0); the
 *                         terms meet in partials of 256 positions as above
 * The workspace is pn_calib_stats_workspace_bytes(n, B) bytes, 8-byte aligned, private.  n == 0 launches no kernel (aurc = 0).
 *
 * Limits, refused with PN_ERR_ARG before any device call: 1 <= C <= 4096, 0 <= S < 2^31, 0 <= n <= 2 000 000 000, R >= 1, T
 * and B as above, a workspace that is too small or misaligned, NULL where something would be read or must be written (the
 * three bin arrays; sums with prob; order with err_prefix or aurc).  Asynchronous on `stream`, nothing read back, nothing
 * allocated.  The *_workspace_bytes calls need no device. */
typedef struct pn_calib_sweep_out { /* device pointers, caller-owned, each may be NULL */
    double *nll;                    /* [T] */
    int32_t *best;                  /* [1] */
    double *tau;                    /* [1] */
    int64_t *counts;                /* [3], written */
} pn_calib_sweep_out;
typedef struct pn_calib_stats_out { /* device pointers, caller-owned */
    int64_t *bin_count;             /* [B], added to */
    int64_t *bin_correct;           /* [B], added to */
    int64_t *bin_conf;              /* [B], added to */
    int64_t *counts;                /* [5], added to; may be NULL */
    double *sums;                   /* [2], added to; needed with prob */
    int32_t *order;                 /* [n] or NULL */
    int32_t *err_prefix;            /* [n] or NULL; needs order */
    double *aurc;                   /* [1] or NULL; needs order */
} pn_calib_stats_out;
int pn_ensemble_add_scaled(pn_context *ctx, const float *logits /* dev [R, S, C] */, int32_t R, int64_t S, int32_t C,
                           const int32_t *index /* dev [S] or NULL */, int64_t rows, void *state,
                           int32_t *status /* dev or NULL */, const double *tau /* dev [1] */, void *stream);
int pn_calib_sweep_workspace_bytes(int64_t S, int32_t T, int64_t *bytes);
int pn_calib_sweep(pn_context *ctx, const float *logits /* dev [R, S, C] */, int32_t R, int64_t S, int32_t C,
                   const int64_t *target /* dev [S] */, const double *temps /* dev [T] */, int32_t T, void *workspace,
                   int64_t workspace_bytes, const pn_calib_sweep_out *out, void *stream);
int pn_calib_stats_workspace_bytes(int64_t n, int32_t B, int64_t *bytes);
int pn_calib_stats(pn_context *ctx, const float *confidence, const int64_t *label, const int64_t *target,
                   const float *prob /* dev [n, C] or NULL */, int64_t n, int32_t C, int32_t B, void *workspace,
                   int64_t workspace_bytes, const pn_calib_stats_out *out, void *stream);

/* ---- self-supervised pretraining: the contrastive loss between two path draws (pn_contrast.hip) -----------------------------
 * NT-Xent / InfoNCE between two views A, B (dev fp32 [S, D], row strides lda, ldb >= D) of the same S nodes, forward and
 * backward, without an S x S array in memory.  Added without an ABI bump: four new symbols and one new struct, no existing
 * struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * Pair i is LIVE when valid[i] != 0 (valid dev uint8 [S], or NULL: all), every entry of a_i and b_i is finite and both norms,
 * formed in fp64, are finite and > 0.  M = live pairs; bad = pairs that are not live only because of their data.  The unit
 * rows stack as z_r = a_r / |a_r| for r < S and b_{r-S} / |b_{r-S}| otherwise (z = (float)((double)x / norm)); the partner is
 * p(r) = r +- S, the logit s_rc = <z_r, z_c> / tau (fp32: one k-ordered fma chain per element on the fp32-input MFMA, then one
 * multiplication by (float)(1 / tau)), and N(r) is every live c != r -- with intra == 0 only those of the other view (the
 * symmetric cross-view form; intra != 0 is SimCLR / GRACE NT-Xent).
 *   lse_r      = log sum_{c in N(r)} exp(s_rc)           an online softmax per lane in fp32, lse = m + log(sum) in fp64
 *   row_loss_r = lse_r - s_{r,p(r)}                      fp32 [2S], 0 for a row that is not live
 *   loss       = (1 / 2M) sum_{live r} row_loss_r        fp64 [1], 0 when M == 0
 *   hits       = rows with s_{r,p(r)} >= s_rc for every c in N(r), on the kernel's own fp32 logits      int64 [1], written
 *   counts     = {M, bad}                                int64 [2], written
 * Order: one workgroup owns a row tile and walks the column tiles in ascending order; the lanes of a row meet in a fixed
 * butterfly; the loss adds the fp64 row losses in partials of 256 rows (halving tree, absent rows 0.0) and the partials in
 * ascending order.  All of it depends on (S, D, intra) alone, and there is no floating-point atomic: the same bits every run.
 * pn_contrast_backward reads what the forward left in the SAME workspace (unit rows, norms, liveness, lse, M) and
 * grad_loss (dev fp32 [1]) and writes every element of dA, dB (dev fp32 [S, D], contiguous) with plain stores:
 *   dz_r = g / (2 M tau) [ sum_{c in N(r)} (P_rc + P_cr) z_c - 2 z_{p(r)} ],   P_rc = exp(s_rc - lse_r)
 *   dx_r = (dz_r - z_r <z_r, dz_r>) / |x_r|              exactly 0 for a row that is not live, and when M == 0
 * The bracket is one exact-fp32 MFMA product W Z per row tile (W_rc = P_rc + P_cr - 2 [c == p(r)], both terms from one pass:
 * s is symmetric bit for bit); the projection and the scaling run in fp64.
 * The workspace: pn_contrast_workspace_bytes(S, D) = 64 + 2 (2S D 4) + 24 (2S) + 8 ceil(2S / 256) bytes, 8-byte aligned,
 * private; nothing in it is quadratic in S.  pn_contrast_tiles: {row tile, column tile, K chunk} of the kernels.
 * Refused with PN_ERR_ARG before any device call: S < 0 or 2S >= 2^31, D outside 1 .. 8192, tau not finite and positive, a
 * row stride below D, a workspace that is too small or misaligned, NULL A / B / workspace / out (S > 0), NULL grad_loss / dA /
 * dB in the backward.  S == 0 launches no kernel: loss, hits and counts are zeroed.  Asynchronous on `stream`, nothing read
 * back, nothing allocated; M is consumed on the device.  pn_contrast_workspace_bytes and pn_contrast_tiles need no device. */
typedef struct pn_contrast_out {    /* device pointers, caller-owned, each may be NULL */
    double *loss;                   /* [1] */
    float *row_loss;                /* [2S] */
    int64_t *hits;                  /* [1], written */
    int64_t *counts;                /* [2] = {M, bad}, written */
} pn_contrast_out;
int pn_contrast_workspace_bytes(int64_t S, int32_t D, int64_t *bytes);
int pn_contrast_tiles(int32_t out[3]);
int pn_contrast_forward(pn_context *ctx, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t S, int32_t D,
                        double tau, int32_t intra, const uint8_t *valid /* dev [S] or NULL */, void *workspace,
                        int64_t workspace_bytes, const pn_contrast_out *out, void *stream);
int pn_contrast_backward(pn_context *ctx, const float *A, int64_t lda, const float *B, int64_t ldb, int64_t S, int32_t D,
                         double tau, int32_t intra, void *workspace, int64_t workspace_bytes,
                         const float *grad_loss /* dev [1] */, float *dA, float *dB, void *stream);

/* ---- nearest neighbours: exact k best bank rows per query, and the weighted vote over their labels (pn_knn.hip) ---------------
 * The k nearest rows of a bank X (dev fp32 [N, D], row stride ldx >= D) for every row of Q (dev fp32 [Sq, D], row stride ldq
 * >= D) by cosine or dot product, without an Sq x N array in memory, and the weighted k-NN classifier over the result: the
 * label-free monitor of contrastive pretraining.  Added without an ABI bump: four new symbols, one new struct and three
 * constants, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * A row is LIVE when every entry is finite and, for PN_KNN_COSINE, its norm, formed in fp64, is finite and > 0 (the rule of the
 * contrastive loss).  A bank row must also pass bank_valid (dev uint8 [N], != 0; NULL: all).  exclude (dev int64 [Sq] or NULL)
 * names one bank index per query that is no candidate of that query (-1 or anything outside [0, N): none): the leave-one-out
 * case, where the queries sit inside the bank.  The candidates of a live query are the live bank rows but the excluded one; a
 * dead query has none.  Score of (query r, bank row c), fp32:
 *   PN_KNN_COSINE   s = <z_r, z_c>,  z = (float)((double)x / norm)
 *   PN_KNN_DOT      s = <q_r, x_c>,  the operands as they are
 * one k-ordered fma chain per pair on the fp32-input MFMA (K chunks of 16, zeros past D): the tile of the contrastive loss, so
 * in pn_knn_search(X, X) cosine the score of (i, j) has the bits of (j, i).
 * The order is TOTAL: the higher fp32 score first and, on equal bits, the lower bank index.  -0.0 is taken as +0.0 (they tie,
 * and +0.0 is what is returned); a NaN score -- possible only with PN_KNN_DOT, when products overflow with both signs -- is
 * taken, ranked and returned as -inf.  With n = min(k, candidates):
 *   index  int64 [Sq, k]   slot j: the j-th neighbour's bank index; -1 for j >= n
 *   score  fp32  [Sq, k]   its score; -inf for j >= n
 *   count  int32 [Sq]      n; 0 for a dead query
 *   counts int64 [2]       {dead queries, bank rows that pass bank_valid and are dead for their data's sake}; written
 * How it runs: the grid is (row tiles of 64 queries, splits); a workgroup walks its contiguous share of the column tiles of 128
 * bank rows, keeps every row's k best (score, index) keys in LDS and writes a partial list; a second kernel merges the
 * `splits` partial lists of a query.  The k best of a set of distinct keys do not depend on how the set is cut: the outputs are
 * bit-identical for every `splits`, for any Sq a row is queried within, and across runs.  splits = 0: the library chooses --
 * enough for two workgroups per CU of an MI355X (512) where N allows -- and any value is lowered to one split per column
 * tile at most.  pn_knn_plan: out = {splits used, workgroups of the search, row tile, column tile}.
 * The workspace: pn_knn_workspace_bytes(Sq, N, D, k, splits) = 64 + 8 s Sq k + 4 (Sq + N) D + 4 (Sq + N) bytes, rounded up to
 * 8, with s the splits used; 8-byte aligned, private; nothing in it is Sq x N.
 *
 * pn_knn_vote: the weighted vote of a search's neighbours.  bank_labels dev int64 [N]; for query q, slot j < count[q] whose
 * index is inside [0, N) and whose label y_j is inside [0, C) VOTES with
 *   w_j = exp(((double)s_j - (double)s_0) / T)        (s_0: the query's best score, so w_0 = 1 and nothing overflows; T = +inf: 1)
 * and no memory is touched for a slot that does not.  One wave per query adds the slots in ascending j into its fp64 [C]:
 *   prob  fp64  [Sq, C]    votes / sum of the voting weights (added in ascending j); all 0 when that sum is 0
 *   label int64 [Sq]       argmax_c votes, the lowest class on ties; -1 when the sum is 0
 * labels (dev int64 [Sq], the queries' own, or NULL) adds confusion[t, label] += 1 (int64 [C, C]) for 0 <= t < C and label >= 0
 * and skipped[0] += 1 (int64 [1]) for every other query, with integer atomics (exact, order-free): the caller zeroes them or
 * keeps them across calls, as with pn_ensemble_finish.
 *
 * Refused with PN_ERR_ARG before any device call: Sq or N outside [0, 2^31), D outside 1 .. 8192, k outside 1 .. PN_KNN_MAX_K,
 * splits outside 0 .. 1024, an unknown metric, a row stride below D, a workspace that is NULL, too small or misaligned, NULL Q
 * (Sq > 0) / X (N > 0) / out; in the vote C outside 1 .. 4096, T not > 0 (NaN included), NULL index / score / count (Sq > 0)
 * or bank_labels (Sq, N > 0), confusion or skipped without labels.  Sq == 0 or N == 0 launch only what fills the outputs
 * (every slot empty, counts still exact); the vote launches nothing for Sq == 0.  Asynchronous on `stream`, nothing read back,
 * nothing allocated.  pn_knn_workspace_bytes and pn_knn_plan need no device. */
#define PN_KNN_COSINE 0
#define PN_KNN_DOT 1
#define PN_KNN_MAX_K 64
typedef struct pn_knn_out {         /* device pointers, caller-owned, each may be NULL */
    int64_t *index;                 /* [Sq, k] */
    float *score;                   /* [Sq, k] */
    int32_t *count;                 /* [Sq] */
    int64_t *counts;                /* [2] = {dead queries, dead bank rows}, written */
} pn_knn_out;
int pn_knn_workspace_bytes(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits, int64_t *bytes);
int pn_knn_plan(int64_t Sq, int64_t N, int32_t D, int32_t k, int32_t splits_in, int64_t out[4]);
int pn_knn_search(pn_context *ctx, const float *Q, int64_t ldq, int64_t Sq, const float *X, int64_t ldx, int64_t N, int32_t D,
                  int32_t k, int32_t metric, const uint8_t *bank_valid /* dev [N] or NULL */,
                  const int64_t *exclude /* dev [Sq] or NULL */, int32_t splits, void *workspace, int64_t workspace_bytes,
                  const pn_knn_out *out, void *stream);
int pn_knn_vote(pn_context *ctx, const int64_t *index, const float *score, const int32_t *count, int64_t Sq, int32_t k,
                const int64_t *bank_labels /* dev [N] */, int64_t N, int32_t C, double T,
                const int64_t *labels /* dev [Sq] or NULL */, double *prob, int64_t *label, int64_t *confusion, int64_t *skipped,
                void *stream);

/* ---- clustering: k-means of embeddings, and the scores of a grouping against labels (pn_kmeans.hip) -------------------------
 * Lloyd's k-means with k-means++ seeding over rows X (dev fp32 [N, D], row stride ldx >= D) by cosine or squared euclidean
 * distance, without an N x K array in memory, and NMI / ARI / purity of a grouping against labels: the third label-free
 * judgement of contrastive pretraining beside the linear and the k-NN probe.  Added without an ABI bump: new symbols, two new
 * structs and four constants, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * Definitions.
 * - Live row.  Every entry is finite.  For PN_KMEANS_COSINE, the norm formed in fp64 is also finite and > 0 (knn's rule, and
 *   knn's order of additions: the same unit rows bit for bit).  The row must pass `valid` (dev uint8 [N] or NULL).  A dead row
 *   gets label = -1, costs nothing and enters no mean.
 * - Prepared rows z, written once per run into the workspace (zeros for a dead row).
 *     Cosine: (float)((double)x / norm).
 *     PN_KMEANS_EUCLIDEAN: x as it is, with q_r = sum_d (double)x_rd^2 kept beside it, added in ascending d.
 * - Score.  s(r, c) = <z_r, m_c> in fp32, for centroids m fp32 [K, D]: logits_tile of pn_simtile.h over the stacked array
 *   [z; m] in the workspace, row tiles from the rows, column tiles from the centroids -- knn's and the contrastive loss's
 *   arithmetic (exact fp32 products, one k-ordered fma chain per pair, K chunks of 16, zeros past D).  A NaN score is possible
 *   only for euclidean, when products overflow with both signs.  It counts as -inf, as in knn.
 * - Key.  e(r, c) = (double)s(r, c) - h_c.  Cosine: h_c = 0.  Euclidean: h_c = 0.5 * sum_d (double)m_cd^2, in ascending d.
 *   h_c = +inf, and e = -inf whatever the score, for a centroid that is itself not live (an entry not finite; cosine: all
 *   zeros).  That happens only with caller-supplied centroids, so such a centroid wins nothing.
 * - Assignment.  label(r) = argmax_c e(r, c), the lowest c on equal values.  -0.0 equals +0.0.
 * - Row cost, fp64.  Cosine: d_r = max(0, 1 - e).  Euclidean: d_r = max(0, q_r - 2 e).
 * - Inertia.  The fp64 sum of d_r over the live rows (a dead row adds 0.0): fixed blocks of 256 consecutive rows added in
 *   ascending order, then the block sums in ascending order.  The order depends on N alone.
 * - Moved.  The number of live rows whose label differs from prev_label (prev_label NULL: every live row); exact integers.
 * - Update.  For every cluster with members: coordinate d of the sum is the fp64 sum of z_rd over the members in ascending
 *   row index -- the cluster's sorted member list is cut into chunks of 64 (pn_kmeans_plan reports it), each chunk is added
 *   in ascending order, then the chunk partials in ascending order -- so the order depends on the assignment alone, never on
 *   the grid or timing, and there is no floating-point atomic.  mean = sum / count in fp64.  Euclidean: m = (float)mean.
 *   Cosine: m = (float)(mean / ||mean||), ||mean||^2 in fp64 as mean_d^2 (rounded) added per residue of d mod 256 in
 *   ascending d, the 256 residues then by a halving tree (t += t + 128, 64, .. 1).  A cluster keeps its previous centroid
 *   and adds 1 to `empty` when it has no member, or when the cosine mean has no finite positive norm.  The member lists come
 *   from the stable radix sort of (key = label, dead rows and labels outside [0, K) keyed K; value = row).
 *
 * The workspace carries a run: the prepared rows, liveness, q, the WORKING CENTROIDS (rows N .. N + K - 1 of the stacked
 * array) and scratch.  pn_kmeans_prepare fills the rows; pn_kmeans_seed or pn_kmeans_set_centroids the centroids; assign
 * reads them and update replaces them in place.  All calls of a run pass the same N, D, K, metric and workspace.
 *   pn_kmeans_prepare        prepared rows, liveness, q_r; counts[0] (int64, may be NULL) = rows that are not live
 *   pn_kmeans_set_centroids  the working centroids = the caller's [K, D] (row stride ldc >= D), as they are
 *   pn_kmeans_seed           k-means++ on the device, nothing read back.  Round j of restart rho draws
 *                            w = philox4(seed, ((uint64)rho << 32) | j, PN_KMEANS_STREAM) (the dropout masks' hash, a stream of
 *                            its own) and r53 = ((w.x | (uint64)w.y << 32) >> 11).  Round 0 weighs every live row 1; round
 *                            j >= 1 weighs row r with mind_r = min_{i < j} d(r, chosen_i), d as above on the key
 *                            <z_r, z_c> - h_c with the products and sums in fp64 (per residue of d mod 64 in ascending d, the 64
 *                            residues by an xor butterfly 32, 16, .. 1; h_c = q_c / 2).  Prefix sums P of the weights are fp64
 *                            in a fixed two-level order: within blocks of 256 rows in ascending order, then the block sums in
 *                            ascending order; P_r = (sum of the earlier blocks) + (the prefix inside r's block).
 *                            t = ((double)r53 * 2^-53) * P_total, one multiplication; the pick is the first row with P_r > t
 *                            (t rounded up to P_total: the highest row with a weight).  If P_total is 0 or not finite: the
 *                            lowest live row not yet chosen; if none remains, the lowest live row; if no row is live at all,
 *                            zeros as the centroid and -1 as chosen[j].  The working centroids become copies of the prepared
 *                            rows; centroid (fp32 [K, D], contiguous) and chosen (int64 [K]) receive copies, each may be NULL.
 *                            Cost: K passes over N x D.
 *   pn_kmeans_assign         one workgroup per row tile of 64 walks all ceil(K / 128) column tiles and keeps one (key, index)
 *                            best per row in registers.  out: label int32 or int64 [N] by label_bits, key fp64 [N] (-inf
 *                            for dead rows), moved int64 [1], inertia fp64 [1], iterations int32 [1] (+= 1), each may be NULL.
 *                            prev_label (same width, or NULL) may be the label array itself.  done (dev int32 [1] or NULL):
 *                            the call returns at once, every output byte untouched, when it is set, and sets it when
 *                            moved == 0.
 *   pn_kmeans_update         sort, then the segmented sums above from `label`.  centroid (fp32 [K, D], a copy of the working
 *                            centroids afterwards), count int64 [K], empty int64 [1], each may be NULL.  Obeys `done`: nothing
 *                            but the private sort scratch is written when it is set.
 *   pn_kmeans_run            the loop in one call, nothing read back: prepare; per restart rho: seed (or, with init, the caller's
 *                            centroids; then restarts must be 1), then for t = 1 .. iters: assign, and if t < iters, update.
 *                            Kernels after a converged assign are no-ops by the device flag, so a run always ends on an assign:
 *                            the returned labels are the nearest centroids of the returned centroids and inertia belongs to
 *                            exactly that pair.  After restart rho the result takes its labels, centroids, counts, inertia,
 *                            iterations and moved history when its inertia is lower than the one held: a non-finite inertia
 *                            loses to any finite one, on equal values the earlier restart stays.  iterations = the assigns that
 *                            did work; moved[t] = -1 for an assign that did none.
 * Why assign is a kernel of its own and not pn_knn_search(k = 1): the search re-normalises both operands on every call, keeps
 * k-best lists in LDS and merges splits, and has no per-column offset, no previous-label compare and no cost sum, while a run
 * calls assign up to iters x restarts times over the same rows.  What the two share is the tile, and it stays shared.
 *
 * pn_cluster_scores(pred int64 [S], K, truth int64 [S], C): table int64 [K, C] += 1 at [pred, truth] by integer atomics (the
 * caller zeroes it or keeps it across calls, as with the confusion matrices); skipped[0] += 1 (may be NULL) for a pair with
 * either side outside its range.  Then, with scores != NULL, a one-workgroup finish in fp64 over the WHOLE table, terms
 * added in row-major order of the table, writes scores fp64 [4] = {nmi, ari, purity, n}; a_i, b_j the row and column sums:
 *   nmi    = MI / ((H_pred + H_true) / 2) in natural logs, MI = sum (n_ij / n) log((n n_ij) / (a_i b_j)); 1 when both entropies
 *            are 0
 *   ari    = (sum C(n_ij, 2) - E) / ((A + B) / 2 - E), A = sum C(a_i, 2), B = sum C(b_j, 2), E = A B / C(n, 2); the three
 *            binomial sums are exact int64; 1 when the denominator is 0
 *   purity = sum_i max_j n_ij / n
 * n == 0 gives NaN scores.
 *
 * Limits, refused with PN_ERR_ARG before any device call, outputs untouched: N outside [0, 2^31), D outside 1 .. 8192, K
 * outside 1 .. PN_KMEANS_MAX_K, an unknown metric, label_bits other than 32 or 64, a stride below D, a NULL, short or misaligned
 * workspace, NULLs where something would be read (X with N > 0, centroids to set, labels to update from, the output
 * description), iters outside 1 .. 65536 or restarts < 1 in pn_kmeans_run, restarts != 1 with init, a negative restart index;
 * in the scores S outside [0, 2^31), K outside 1 .. 1024, C outside 1 .. 4096, a NULL table, NULL pred / truth with S > 0.
 * N == 0 launches only what fills the outputs.  Asynchronous on `stream`, nothing allocated, nothing read back.
 *
 * The workspace, 8-byte aligned, private, nothing in it N x K; with r8(b) = b rounded up to 8 and T = ceil(N / 64):
 *   pn_kmeans_workspace_bytes(N, D, K, iters) = 64 + r8(4 (N + K) D) + 6 r8(4 N) + 24 N + 16 K + 8 ceil(N / 256) + r8(4 T)
 *                                               + r8(N) + 8 iters + 2 r8(4 (K + 2)) + 8 (T + K) D + r8(20 N) + 8 MiB
 * (iters: that of pn_kmeans_run, 0 for the single steps; the last two terms are the radix sort's reserve).
 * pn_kmeans_plan: out = {workgroups of assign, row tile, column tile, K chunk, update chunk, inertia block}.  Neither needs a
 * device. */
#define PN_KMEANS_COSINE 0
#define PN_KMEANS_EUCLIDEAN 1
#define PN_KMEANS_MAX_K 1024
#define PN_KMEANS_STREAM 0x4B4Du    /* philox4's stream word; the dropout masks use 1 and 2 */
typedef struct pn_kmeans_assign_out { /* device pointers, caller-owned, each may be NULL */
    void *label;                    /* [N] int32 or int64 */
    double *key;                    /* [N] */
    int64_t *moved;                 /* [1], written */
    double *inertia;                /* [1], written */
    int32_t *iterations;            /* [1], += 1 */
} pn_kmeans_assign_out;
typedef struct pn_kmeans_out {      /* device pointers, caller-owned, each may be NULL */
    void *label;                    /* [N] int32 or int64 */
    float *centroid;                /* [K, D] */
    int64_t *count;                 /* [K] members of the returned labels */
    double *inertia;                /* [1] */
    int32_t *iterations;            /* [1] */
    int64_t *moved;                 /* [iters] */
    int64_t *counts;                /* [1] = {rows that are not live} */
    int32_t *restart;               /* [1] the restart the result is from */
} pn_kmeans_out;
int pn_kmeans_workspace_bytes(int64_t N, int32_t D, int32_t K, int32_t iters, int64_t *bytes);
int pn_kmeans_plan(int64_t N, int32_t D, int32_t K, int64_t out[6]);
int pn_kmeans_prepare(pn_context *ctx, const float *X, int64_t ldx, int64_t N, int32_t D, int32_t K, int32_t metric,
                      const uint8_t *valid /* dev [N] or NULL */, void *workspace, int64_t workspace_bytes,
                      int64_t *counts /* dev [1] or NULL */, void *stream);
int pn_kmeans_set_centroids(pn_context *ctx, const float *centroid, int64_t ldc, int64_t N, int32_t D, int32_t K,
                            void *workspace, int64_t workspace_bytes, void *stream);
int pn_kmeans_seed(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, uint64_t seed, int32_t restart,
                   void *workspace, int64_t workspace_bytes, float *centroid, int64_t *chosen, void *stream);
int pn_kmeans_assign(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, void *workspace, int64_t workspace_bytes,
                     const void *prev_label, int32_t label_bits, const pn_kmeans_assign_out *out, int32_t *done, void *stream);
int pn_kmeans_update(pn_context *ctx, int64_t N, int32_t D, int32_t K, int32_t metric, void *workspace, int64_t workspace_bytes,
                     const void *label, int32_t label_bits, float *centroid, int64_t *count, int64_t *empty,
                     const int32_t *done, void *stream);
int pn_kmeans_run(pn_context *ctx, const float *X, int64_t ldx, int64_t N, int32_t D, int32_t K, int32_t metric,
                  const uint8_t *valid /* dev [N] or NULL */, const float *init /* dev [K, D] or NULL */, int64_t ld_init,
                  int32_t iters, int32_t restarts, uint64_t seed, void *workspace, int64_t workspace_bytes, int32_t label_bits,
                  const pn_kmeans_out *out, void *stream);
int pn_cluster_scores(pn_context *ctx, const int64_t *pred, int32_t K, const int64_t *truth, int32_t C, int64_t S, int64_t *table,
                      int64_t *skipped, double *scores, void *stream);

/* ---- explanations: exact path and group occlusion (pn_explain.hip) --------------------------------------------------------
 * What would the model say without some of a node's paths, or with those paths alone?  pn_path_weights answers with one
 * forward per question.  None of that is needed: the recurrence never sees the pooling, leaving members out of a row changes
 * only the pooling's normalisation and which terms enter the sum, and the classifier is linear after it.  These calls
 * evaluate the closed form for all groups of all rows in one pass over the final hidden states.  Added without an ABI bump:
 * three new symbols and one new struct, no existing struct or signature changed, so pn_abi_version keeps answering 12.
 *
 * Row s has members j = 0 .. W-1 in encode()'s member order (out_path_weight's): for HOMO / PAGG path j of masked node s,
 * for HETERO slot q = j * S + s.  Inputs, dev fp32 unless noted:
 *   state  [S, W, ld_state]  final hidden states, the first H entries of a member's row are used
 *   coef   [S, W]            the coefficient applied (out_path_weight: already kappa w c)
 *   ego    [S, ld_ego]       the first H entries of a row are used (the ego half of the embedding)
 *   fc2_w  [C, ld_w]         columns 0 .. H-1 multiply ego, columns H .. 2H-1 multiply pooled;  fc2_b [C]
 *   weight [S, W] or NULL    the caller's path weights IN MEMBER ORDER.  A member is live when weight is NULL or its entry is a
 *                            finite positive number
 *   group  [S, W] int32      a value outside [0, G): the member belongs to no group -- never removed, never kept alone
 *   norm   PN_PATH_NORM_*;   renorm  1 for HETERO, whose softmax renormalises over the remaining members, 0 for HOMO / PAGG
 *   target [S] int64 or NULL NULL: the argmax of the full logits, lowest class on ties
 * All arithmetic is fp64 on the converted inputs:
 *   t_j[c] = sum_h fc2_w[c, H+h] state[s,j,h]            e[c] = fc2_b[c] + sum_h fc2_w[c,h] ego[s,h]
 *   contribution[s,j,c] = coef_j t_j[c] / W               full[c] = e[c] + sum_j contribution[s,j,c]     (every j)
 *   R = live members with group_j == g;   present[s,g] = |R|
 *   Om = sum_live w_j (w = 1 without weights), Om_R, Om_rest (live, not in R);   K = sum_live coef_j, K_R, K_rest
 *   drop_g[c] = e[c] + rho_d sum_{live, not in R} contribution[.,c],  rho_d = (norm == SUM ? Om / Om_rest : 1) (renorm ? K / K_rest : 1)
 *   keep_g[c] = e[c] + rho_k sum_{j in R} contribution[.,c],           rho_k = (norm == SUM ? Om / Om_R : 1) (renorm ? K / K_R : 1)
 * Edge rules.  R empty: drop_g = full, bit for bit (rho_d = 1 exactly and the sum runs over every j, as full's does; a dead
 * member's coefficient is 0 in what the library reports).  No live member remains, or renorm and the remaining coefficient
 * mass is not > 0: the pooled part is zero and the logits are e -- the library's rule for a group without a live path.  The
 * sums Om_rest, K_rest and the logit sum over the remaining members are formed by direct summation, never by subtraction.
 * With lp(x) = x_t - logsumexp(x) for the row's target t:
 *   drop_delta[s,g] = lp(full) - lp(drop_g)     positive: the group supports the class
 *   keep_gain[s,g]  = lp(keep_g) - lp(e)
 *   flip[s,g]       = argmax(drop_g) != argmax(full) (lowest class on ties) and present > 0
 *   target_used[s]  = t
 * A target outside [0, C): the row's drop_delta and keep_gain are 0, flip is 0 and status[0] += 1 (dev int32 [2], may be
 * NULL; added to).  A row in which any value read of state, coef, ego, fc2_w or fc2_b is not finite is a bad row: every float
 * output of the row is NaN, flip is 0, present is still counted, status[1] += 1 (and not status[0]), and target_used is the
 * target given, or -1 without one.
 * fp32 outputs are the fp64 value rounded once; a NULL pointer of pn_explain_out is not computed and not written, and
 * drop_delta / keep_gain / flip need no logits stored.
 *
 * Order of the sums: dot products in ascending h; sums over members in ascending j; a logit vector's logsumexp by the
 * lanes that share it (8 for C <= 8, 16 for C <= 16, else 64), each keeping a running (max, sum of exp) over its classes
 * c = lane, lane + lanes, ...; the lanes' maxima meet in a butterfly, every lane rescales its sum to the common maximum,
 * the sums meet in a butterfly, and with class chunks one further merge per chunk.  All of it
 * depends on (W, H, C, G) alone: there is no floating-point atomic, a row's result does not depend on the launch geometry or
 * on the other rows of the call, and the rows split over two calls leave the bits of one call.
 * Work split: one workgroup owns a row; the row's states go through LDS once, in 16-byte loads where ld_state and the
 * address allow, fc2_w's rows beside them, t_j stays in LDS.  pn_explain_route reports {route, lanes, class chunk, H tile}:
 * the class chunk is min(C, 4096 / (W + 1)) -- below C the route is CHUNKED and state is read once per chunk -- and the H tile
 * the largest Ht with (W + 1 + 2 chunk) (Ht | 1) <= 7168, a multiple of 4 when below H.
 *
 * pn_explain_totals adds a call's rows (all S, or rows [n_rows] int32; an entry outside [0, S) is skipped) into a caller-
 * zeroed state of 40 G bytes, 8-byte aligned:
 *     int64 rows_present[G], members[G], flips[G];  double drop_delta_sum[G], keep_gain_sum[G]
 * over the rows with present > 0 and finite drop_delta and keep_gain.  One workgroup owns a group: it adds the call's rows in
 * ascending order in fp64, then adds once into the running total, so the bits depend on the sequence of calls alone.  The
 * integer totals are exact.
 *
 * Limits, refused with PN_ERR_ARG before any device call: 1 <= W, G <= 1024, 1 <= H <= 4096, 1 <= C <= 1024, 0 <= S < 2^31,
 * ld_state, ld_ego >= H, ld_w >= 2 H, norm and renorm as above, NULL where something would be read, n_rows != 0 without rows.
 * S == 0 launches nothing.  Asynchronous on `stream`, nothing read back, nothing allocated. */
#define PN_EXPLAIN_ROUTE_NONE 0    /* S == 0 */
#define PN_EXPLAIN_ROUTE_ROW 1     /* every class in one chunk: state is read once */
#define PN_EXPLAIN_ROUTE_CHUNKED 2 /* (W + 1) * C > 4096: classes in chunks */
typedef struct pn_explain_out {    /* device pointers, caller-owned, each may be NULL */
    float *full;                   /* [S, C] */
    float *contribution;           /* [S, W, C] */
    float *drop_logits;            /* [S, G, C] */
    float *keep_logits;            /* [S, G, C] */
    float *drop_delta;             /* [S, G] */
    float *keep_gain;              /* [S, G] */
    uint8_t *flip;                 /* [S, G] */
    int32_t *present;              /* [S, G] */
    int64_t *target_used;          /* [S] */
} pn_explain_out;
int pn_explain_route(int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t route[4]);
int pn_explain_groups(pn_context *ctx, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, const float *state,
                      int64_t ld_state, const float *coef, const float *ego, int64_t ld_ego, const float *fc2_w, int64_t ld_w,
                      const float *fc2_b, const float *weight /* or NULL */, const int32_t *group, int32_t norm, int32_t renorm,
                      const int64_t *target /* or NULL */, const pn_explain_out *out, int32_t *status /* dev [2] or NULL */,
                      void *stream);
int pn_explain_totals(pn_context *ctx, int64_t S, int32_t G, const float *drop_delta, const float *keep_gain,
                      const uint8_t *flip, const int32_t *present, const int32_t *rows /* dev [n_rows] or NULL */,
                      int64_t n_rows, void *totals, void *stream);

/* ---- explanations by node and by edge: overlapping-group occlusion (pn_explain_units.hip, pn_explain.hip) ------------------
 * Paths are redrawn every epoch; what stays is the graph.  Removing node u from a row means removing every member that
 * passed through u, and nothing in the closed form above needs the groups to be disjoint.  Added without an ABI bump: three
 * new symbols, no struct or signature changed, pn_abi_version keeps answering 12.
 *
 * pn_explain_units turns a row's ids into its units and every step's label.  node [S, W, L] int32 is in MEMBER order: the
 * node whose table row member j of row s consumed at step t (HOMO / PAGG: the path array itself; HETERO: slot q = j S + s
 * reads ids_flat[(q L + t) % P, L - 1 - (q L + t) / P], P = S W of the whole batch).
 *   PN_UNIT_NODE  M = L.  The key of step t is the node id.  No unit (label -1) when the id is negative, or equals
 *                 exclude[s] (dev int32 [S] or NULL: the row's own node, which sits on every path of a HOMO / PAGG row and
 *                 also enters through the ego half of the embedding).
 *   PN_UNIT_EDGE  M = L - 1.  The key of step t >= 1 (label column t - 1) is the undirected pair of the ids of steps t - 1
 *                 and t: ((int64)min << 32) | max.  No unit when either end is negative.  A stay step (u, u) is a unit like
 *                 any other (the shipped tables have self loops).  exclude must be NULL.
 *   unit  [S, G] int64, G = W M    unit[s, 0 .. count[s]) the row's distinct keys in ascending order, the rest -1
 *   count [S] int32
 *   label [S, W, M] int32          the position of the step's key in unit[s], or -1
 * Exact integers, a function of the row alone (not of S or the grid).  One workgroup owns a row and sorts its keys in LDS:
 * no workspace.  Limits: 1 <= W, 1 <= L <= 16 (L >= 2 for edges), W M <= 1024, 0 <= S < 2^31.
 *
 * pn_explain_overlap is pn_explain_groups, definition, edge rules, bad rows, target, status, rounding and sum orders, with
 * ONE line changed:
 *   R = the live members j with label[s, j, m] == g for some m      (label [S, W, M] int32)
 * A label outside [0, G) is no membership; a member with no valid label is never removed and never kept alone.  A label
 * repeated within a member counts once: present[s, g] counts members, not steps.  The sum orders are fixed by
 * (W, H, C, G, M) alone.  With M = 1 and label = group every output has pn_explain_groups' bits.  It follows
 * pn_explain_route's route.  Limits: those of pn_explain_groups, and 1 <= M <= 16, W M <= 1024.
 *
 * pn_explain_node_totals adds a call's rows (all S, or rows [n_rows] int32; an entry outside [0, S) is skipped) into a
 * caller-zeroed table int64 [4, N]: rows_present[N], members[N], flips[N], top[N].  A unit (s, g) qualifies when
 * present > 0, drop_delta and keep_gain are finite (pn_explain_totals' rule) and its key u = unit[s, g] lies in [0, N); it
 * adds 1 to rows_present[u], present to members[u] and (flip != 0) to flips[u].  top[u] += 1 for the one qualifying unit of
 * the row with the largest drop_delta, the lowest position among equals.  64-bit integer atomics: the table is exact and
 * independent of order, which is why it holds counts only -- per-node sums of scores would need floating-point atomics or a
 * global sort (the caller has unit and drop_delta on the device).  There are no per-edge totals: an edge has no dense index.
 * Limits: 1 <= G <= 1024, N >= 1, rows / n_rows as pn_explain_totals.
 *
 * All three: refused with PN_ERR_ARG before any device call (NULL where something would be read included), S == 0 launches
 * nothing, asynchronous on `stream`, nothing read back, nothing allocated. */
#define PN_UNIT_NODE 0
#define PN_UNIT_EDGE 1
int pn_explain_units(pn_context *ctx, int64_t S, int32_t W, int32_t L, int32_t kind,
                     const int32_t *node /* dev [S, W, L] */, const int32_t *exclude /* dev [S] or NULL; PN_UNIT_NODE only */,
                     int64_t *unit /* dev [S, G], G = W * M */, int32_t *count /* dev [S] */,
                     int32_t *label /* dev [S, W, M] */, void *stream);
int pn_explain_overlap(pn_context *ctx, int64_t S, int32_t W, int32_t H, int32_t C, int32_t G, int32_t M, const float *state,
                       int64_t ld_state, const float *coef, const float *ego, int64_t ld_ego, const float *fc2_w, int64_t ld_w,
                       const float *fc2_b, const float *weight /* or NULL */, const int32_t *label /* dev [S, W, M] */,
                       int32_t norm, int32_t renorm, const int64_t *target /* or NULL */, const pn_explain_out *out,
                       int32_t *status /* dev [2] or NULL */, void *stream);
int pn_explain_node_totals(pn_context *ctx, int64_t S, int32_t G, int32_t N, const int64_t *unit /* dev [S, G] */,
                           const float *drop_delta, const float *keep_gain, const uint8_t *flip, const int32_t *present,
                           const int32_t *rows /* dev [n_rows] or NULL */, int64_t n_rows,
                           int64_t *table /* dev [4, N], caller-zeroed, added to */, void *stream);

/* Byte offsets inside the aggregator workspace of the intermediates tests look at:
 * out[0] Xh [N,H], out[1] Z [N,L,H], out[2] hn [P,H] (pooling-group order), out[3] layer1 [S,2H]. */
int pn_pagg_debug_offsets(const pn_pagg_shape *shape, int64_t out[4]);

/* ================================================================================================
 * Per-stage timing with HIP events recorded on the caller's stream (measurement only; state in the context).
 * mode 0: off (default).  mode 1: bracket every stage.  mode 2: bracket only stage `stage`.
 * pn_profile_read waits for the recorded events, adds the elapsed times into ms_sum[i] / count[i]
 * (arrays of pn_profile_stage_count() entries) and clears the recording.
 * ============================================================================================== */
int pn_profile_configure(pn_context *ctx, int32_t mode, int32_t stage);
int pn_profile_stage_count(void);
const char *pn_profile_stage_name(int32_t stage);
int pn_profile_read(pn_context *ctx, double *ms_sum, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* PATHNET_HIP_H_ */
