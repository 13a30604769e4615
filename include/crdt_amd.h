/*
 * crdt_amd.h -- C-ABI of the MI355X-native batched CRDT merge engine.
 *
 * This is the drop-in boundary for the merge/compare path of
 * anuragsarkar97/crdt (/root/reference/main.go).  The reference exposes no
 * FFI: its path is the unexported Go method `func (server *Server) merge()`
 * (main.go:35-100) over a gods treemap ordered by `utils.Int64Comparator`
 * (main.go:106-107).  Every entry point below names the reference interface
 * it replaces; INTEGRATION.md shows the cgo binding a maintainer would add.
 *
 * Conventions:
 *   - plain pointers and sizes; no C++/torch types cross the boundary;
 *   - every call returns int: 0 = CRDT_OK, < 0 = crdt_status (never aborts,
 *     never throws);
 *   - "dev" pointers are device (HBM) addresses; work is enqueued on the
 *     context's stream and is asynchronous unless the name says _sync/_host;
 *   - the library never retains caller pointers past a call (cgo rule);
 *   - a context is single-stream and not thread-safe: one context per
 *     Server/goroutine, mirroring the reference's one mutex per Server
 *     (main.go:32, :43-44).
 */
#ifndef CRDT_AMD_H
#define CRDT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRDT_AMD_ABI_VERSION 1

typedef enum crdt_status {
    CRDT_OK = 0,
    CRDT_E_INVAL = -1,      /* bad argument (null pointer, size overflow, bad option) */
    CRDT_E_HIP = -2,        /* HIP runtime error; see crdt_ctx_last_hip_error() */
    CRDT_E_NOMEM = -3,      /* device allocation failed */
    CRDT_E_NODEV = -4,      /* no usable gfx950 device */
    CRDT_E_UNSORTED = -5,   /* input violates the documented sort order */
    CRDT_E_RANGE = -6,      /* an index/size does not fit the kernel's integer width */
    CRDT_E_COMM = -7,       /* RCCL error; see crdt_shard_comm_last_error() */
    CRDT_E_DEVICE = -8      /* a kernel raised a device-side failure flag (CRDT_DEV_*): output invalid */
} crdt_status;

typedef struct crdt_ctx crdt_ctx;

/* ---------------------------------------------------------------- library */
int         crdt_abi_version(void);
const char *crdt_status_str(int status);
int         crdt_device_count(int *count);

/* ---------------------------------------------------------------- context */
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream), or
 * NULL for the device's default (null) stream.  The context never creates a
 * stream of its own: its work is ordered with the caller's copies. */
int crdt_ctx_create(int device, void *stream, crdt_ctx **out);
int crdt_ctx_destroy(crdt_ctx *ctx);
int crdt_ctx_set_stream(crdt_ctx *ctx, void *stream);
/* A non-blocking stream for hosts that want one (e.g. to overlap merges with
 * copies); pass it to crdt_ctx_create / crdt_ctx_set_stream. */
int crdt_stream_create(int device, void **stream);
int crdt_stream_destroy(void *stream);
int crdt_ctx_sync(crdt_ctx *ctx);
/* Device-side failure flags raised by kernels since the last clear (the
 * kernels cannot return an error): synchronises the context's stream, then
 * *flags = CRDT_DEV_* bits; clear != 0 resets them.  A set merge whose
 * decoupled look-back exceeded its bounded wait (a scheduling fault, never
 * expected) raises CRDT_DEV_LOOKBACK and its output is invalid. */
#define CRDT_DEV_LOOKBACK 1u
#define CRDT_DEV_RANGE 2u          /* a batch exceeded a per-replica kernel limit, or a pass found its
                                      inputs inconsistent (merge bitmaps): the output is invalid */
#define CRDT_DEV_PLAN 4u           /* a planned D2 merge's inputs fell outside its plan (or an OR-Set key
                                      chunk outgrew its LDS): that call's output is invalid, its count ~0 */
int crdt_ctx_device_status(crdt_ctx *ctx, uint32_t *flags, int clear);
int crdt_ctx_last_hip_error(const crdt_ctx *ctx);
/* Pre-size the context's device workspace so that later calls never
 * allocate (needed before graph capture). */
int crdt_ctx_reserve(crdt_ctx *ctx, size_t bytes);
/* Kernel-shape knobs (crdt_amd/csrc/knobs.inc: "join.unroll", "sets.lww_parts",
 * "sort.plan_cache", "codec.short_tab", ...).  In the product library
 * (libcrdt_amd.so) they are compile-time constants at their measured
 * defaults: crdt_set_option refuses every name with CRDT_E_INVAL, so no
 * process-global state is shared between contexts and no timing diagnostic
 * or failpoint can reach a caller.  The diagnostic build (libcrdt_amd_diag.so,
 * -DCRDT_DIAG; linked by tests and tools only) accepts them process-wide for
 * A/B runs, plus the timing diagnostics ("sort.rdd_diag",
 * "refmerge.diag_fold": kernels skip work, output wrong) and the failpoints
 * "fail.refmerge" (n: the next n RefMerge calls return CRDT_E_NOMEM before
 * touching the device) and "fail.zero_bits" (n: the next n two-pass merges
 * zero their merge bitmaps between the passes: the write pass must raise
 * CRDT_DEV_RANGE, never read out of range).  CRDT_E_INVAL for an unknown
 * name or value. */
int crdt_set_option(const char *name, int64_t value);
/* The knob's value in this build; "build.diag" reads 1 in the diagnostic
 * build, 0 in the product.  CRDT_E_INVAL for an unknown name. */
int crdt_get_option(const char *name, int64_t *value);

/* Device memory for hosts without an allocator of their own (the Go side). */
int crdt_dev_alloc(crdt_ctx *ctx, size_t bytes, void **dev);
int crdt_dev_free(crdt_ctx *ctx, void *dev);
int crdt_memcpy_h2d(crdt_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int crdt_memcpy_d2h(crdt_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
int crdt_memset(crdt_ctx *ctx, void *dev_dst, int byte, size_t bytes);

/* ------------------------------------------------------- compare (a2)
 * utils.Int64Comparator (main.go:106-107): signed total order, -1/0/+1. */
int crdt_compare_int64(int64_t a, int64_t b);

/* ------------------------------------------------ G-Counter / PN-Counter (a6)
 * Replica population state: row-major [rows x nodes] uint64 in HBM.
 * No reference code: build-defined state-based CRDT joins. */

/* out[r][n] = max(a[r][n], b[r][n]) (unsigned).  out may alias a or b. */
int crdt_gcounter_join(crdt_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev,
                       uint64_t *out_dev, size_t rows, size_t nodes);
/* out[n] = max_r a[r][n]  (the join of a whole population; identity 0). */
int crdt_gcounter_fold(crdt_ctx *ctx, const uint64_t *a_dev, size_t rows, size_t nodes,
                       uint64_t *out_dev);
/* out[r] = sum_n a[r][n] (uint64 wrap): the G-Counter value of every replica. */
int crdt_gcounter_value(crdt_ctx *ctx, const uint64_t *a_dev, size_t rows, size_t nodes,
                        uint64_t *out_dev);
/* PN-Counter = (P, N) pair: both joined in one launch.  Outputs may alias. */
int crdt_pncounter_join(crdt_ctx *ctx, const uint64_t *pa_dev, const uint64_t *na_dev,
                        const uint64_t *pb_dev, const uint64_t *nb_dev,
                        uint64_t *pout_dev, uint64_t *nout_dev, size_t rows, size_t nodes);
/* out[r] = (int64)(sum_n P[r][n] - sum_n N[r][n]) with uint64 wrap (main.go:95). */
int crdt_pncounter_value(crdt_ctx *ctx, const uint64_t *p_dev, const uint64_t *n_dev,
                         int64_t *out_dev, size_t rows, size_t nodes);

/* ---------------------------------------------- keyed PN-Counter map (cmap)
 * The sparse form of the counters above: "key k is a number that many replicas
 * increment concurrently" -- the convergent form of the per-key curr + change
 * fold of the reference's replay (main.go:75-98), which depends on the log's
 * order and on every entry arriving once.  Structure-of-arrays cells: replica
 * rep's increments p and decrements n of key.
 * A state is STRICTLY ASCENDING by (key, rep), both compared unsigned, each
 * cell at most once: a precondition of every call below on every side, and a
 * property of every output.  For an input that breaks it the result is
 * unspecified, but no kernel reads or writes outside the given lengths and
 * count <= na + nb still holds.  All arithmetic is modulo 2^64.
 * Lengths, as for the set ops: n_max is the buffer's length, an optional
 * n_dev (device uint64, may be NULL) the length on the device; *n_dev > n_max
 * touches no cell, stores *count_dev = ~0 and raises CRDT_DEV_RANGE; no kernel
 * reads at or past min(*n_dev, n_max); n_max == 0 launches nothing but the
 * count store.  Every call is stream-ordered with no host synchronisation;
 * workspace from the context only (capturable after crdt_ctx_reserve).
 * CRDT_E_INVAL: a NULL ctx, state or count_dev, NULL fields of a side with a
 * non-zero length, key / rep / p / n not naturally aligned (8 / 4 / 8 / 8), a
 * length or count pointer not 8-byte aligned, any output overlapping any input
 * or another output.  CRDT_E_RANGE: a length >= 2^62 or more tiles than a
 * launch holds. */
typedef struct crdt_cmap {
    uint64_t *key;
    uint32_t *rep;
    uint64_t *p;
    uint64_t *n;
} crdt_cmap;
/* The join: the union of the cells; a cell held by both sides gets p = max(p_a,
 * p_b), n = max(n_a, n_b), unsigned.  out holds >= na_max + nb_max cells;
 * out == NULL: the count alone. */
int crdt_cmap_merge(crdt_ctx *ctx, const crdt_cmap *a, size_t na_max, const uint64_t *na_dev,
                    const crdt_cmap *b, size_t nb_max, const uint64_t *nb_dev,
                    const crdt_cmap *out, uint64_t *count_dev);
/* Replica rep's batch of m increments, op_key strictly ascending: cell
 * (op_key[i], rep) becomes (p + op_dp[i], n + op_dn[i]); an absent cell is
 * created from (0, 0), also by an op with dp == dn == 0.  out holds >= n_max +
 * m cells; out == NULL: the count alone. */
int crdt_cmap_apply(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev, uint32_t rep,
                    const uint64_t *op_key_dev, const uint64_t *op_dp_dev, const uint64_t *op_dn_dev,
                    size_t m, const crdt_cmap *out, uint64_t *count_dev);
/* One row per distinct key, in key order: the key, P = the sum of p and N =
 * the sum of n over its cells, value = (int64)(P - N).  Every output (n_max
 * rows each) may be NULL; all NULL: the number of distinct keys alone. */
int crdt_cmap_values(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                     uint64_t *keys_out, uint64_t *p_out, uint64_t *n_out, int64_t *value_out,
                     uint64_t *count_dev);
/* m probe keys, any order, repeats allowed: value_out[i] = the counter of
 * probes[i], 0 where the key is absent; found_out (may be NULL) 1 / 0.  A
 * device length out of range: every value 0, every found 0, CRDT_DEV_RANGE. */
int crdt_cmap_lookup(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                     const uint64_t *probes_dev, size_t m, int64_t *value_out, uint8_t *found_out);
/* The smallest D with merge(dst, D) == merge(dst, src): a cell of src ships,
 * with src's own p and n, when dst has no such cell, or p_s > p_d, or n_s >
 * n_d.  out holds >= ns_max cells; out == NULL: the count alone (0: in sync). */
int crdt_cmap_delta(crdt_ctx *ctx, const crdt_cmap *src, size_t ns_max, const uint64_t *ns_dev,
                    const crdt_cmap *dst, size_t nd_max, const uint64_t *nd_dev,
                    const crdt_cmap *out, uint64_t *count_dev);

/* Range digests of a counter map, for anti-entropy between replicas that share
 * no memory: both cut the key space with the same m ascending splitters,
 * bucket(key) = #{ j : splitters[j] <= key } compared unsigned (crdt_set_digest's
 * buckets: m + 1 of them, equal neighbouring splitters give empty ones, all
 * cells of one key share a bucket), fingerprint their cells per bucket,
 * exchange the fingerprints (16 bytes a bucket), flag the buckets that differ
 * with crdt_set_digest_diff -- it compares plain hash[] / count[] arrays and
 * serves both digests -- and ship crdt_cmap_select's cells alone.  The merge
 * is monotone, so crdt_cmap_merge(dst, selection) is the whole of the
 * receiver's side.  With sm = SplitMix64's output function
 *   h(key, rep, p, n) = sm( sm( sm( sm(key) ^ (uint64)rep ) ^ p ) ^ n ),
 * hash[b] is the sum mod 2^64 of h over the cells in bucket b and count[b]
 * their number, bit-exact whatever the order of the adds.
 * crdt_cmap_digest writes all m + 1 entries of both outputs (n_max == 0 zeroes
 * them); it needs no workspace.  *n_dev > n_max touches no cell, stores ~0 in
 * every entry of both outputs and raises CRDT_DEV_RANGE.  Every search stays
 * inside [0, m] whatever the splitters hold: unsorted splitters give
 * unspecified digests, never an access outside the splitter, flag or cell
 * arrays, and every cell still lands in exactly one bucket.
 * CRDT_E_INVAL beyond the family's: NULL outputs or flags, m != 0 with NULL
 * splitters, a splitter or output pointer not 8-byte aligned.  CRDT_E_RANGE
 * beyond the family's: m >= 2^24. */
int crdt_cmap_digest(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                     const uint64_t *splitters_dev, size_t m,
                     uint64_t *hash_out_dev, uint64_t *count_out_dev);          /* m + 1 entries each */
/* The cells of t whose bucket has flags[b] != 0 (m + 1 flags, e.g.
 * crdt_set_digest_diff's), in order, all four fields unchanged, into out,
 * their number to *count_dev.  out holds >= n_max cells; out == NULL: the
 * count alone. */
int crdt_cmap_select(crdt_ctx *ctx, const crdt_cmap *t, size_t n_max, const uint64_t *n_dev,
                     const uint64_t *splitters_dev, size_t m, const uint8_t *flags_dev, /* m + 1 */
                     const crdt_cmap *out, uint64_t *count_dev);                /* out >= n_max cells; NULL: count alone */

/* Counter-map state from increment logs: the per-key sum of the reference's
 * replay (main.go:87-96) over a log in any order.  crdt_cmap_apply takes one
 * replica's batch, strictly ascending, each key once; the three calls below
 * take what a log, a Diff or a gossip body really is -- cells (key, rep, p,
 * n) with repeats and many replicas interleaved.  All sums are modulo 2^64,
 * all orders unsigned; lengths, refusals, alignment and synchronisation are
 * the family's (above) unless said otherwise.
 *
 * crdt_cmap_combine: `in` ascending by (key, rep) but NOT strictly -- runs of
 * equal (key, rep) of any length, a whole input that is one run included.
 * out = one cell per distinct (key, rep), ascending, p = the sum of p and n =
 * the sum of n over the run: a valid state.  A run whose sums are 0 still
 * yields its cell (crdt_cmap_apply's rule).  idx_dev == NULL: position i
 * contributes in->p[i], in->n[i].  idx_dev != NULL (n_max uint32 values,
 * 4-byte aligned): position i contributes in->p[idx[i]], in->n[idx[i]], in->p
 * / in->n being columns of n_src elements -- the gather fused behind an
 * index-carrying sort.  Every idx[i] is checked against n_src before the
 * load; one at or past it contributes 0 and raises CRDT_DEV_RANGE, every
 * other cell is still exact.  out holds >= n_max cells and overlaps nothing;
 * out == NULL: the count alone.  *n_dev > n_max touches no cell, stores a
 * count of ~0 and raises CRDT_DEV_RANGE; n_max == 0 stores count 0.  Never
 * synchronises, workspace from the context only, capturable after
 * crdt_ctx_reserve.  For an input that is not ascending the result is
 * unspecified, but no access leaves the given lengths and count <= n.
 * CRDT_E_INVAL beyond the family's: idx_dev with n_max != 0 and n_src == 0. */
int crdt_cmap_combine(crdt_ctx *ctx, const crdt_cmap *in, size_t n_max, const uint64_t *n_dev,
                      const uint32_t *idx_dev, size_t n_src,
                      const crdt_cmap *out, uint64_t *count_dev);
/* The additive join of two states (both strictly ascending): the union of the
 * cells; a cell held by both sides gets (p_t + p_d, n_t + n_d); a cell held by
 * d alone is created with d's values, zeros included.  crdt_cmap_apply(t, rep,
 * keys, dp, dn) equals crdt_cmap_add(t, {keys, rep ..., dp, dn}) bit for bit.
 * NOT idempotent, unlike crdt_cmap_merge: d is a batch of increments, and each
 * batch must be delivered exactly once -- the caller's obligation, as for any
 * op-based input.  out holds >= nt_max + nd_max cells; out == NULL: the count
 * alone. */
int crdt_cmap_add(crdt_ctx *ctx, const crdt_cmap *t, size_t nt_max, const uint64_t *nt_dev,
                  const crdt_cmap *d, size_t nd_max, const uint64_t *nd_dev,
                  const crdt_cmap *out, uint64_t *count_dev);
/* m operations (op_key[i], op_rep[i], +op_dp[i], -op_dn[i]) in ANY order, with
 * repeats and any mix of replicas: out = the state whose cell (k, r) holds the
 * sums of dp / dn over the operations with that key and replica, whatever the
 * operations' order.  out (not NULL) holds >= m cells.  The operations are
 * ordered by crdt_tuples_sort's machinery, as tuples (key, ts = rep widened,
 * rep = operation index, tomb = 0), then combined with the sorted index column
 * as idx over op_dp / op_dn.  SYNCHRONISES ONCE, for the sort's plan
 * read-back: the one call of the family that is not capturable.  CRDT_E_RANGE:
 * m >= 2^32.  CRDT_E_INVAL: a NULL out or count_dev, NULL operation columns or
 * out fields with m != 0, misalignment, any output overlapping an input or
 * another output. */
int crdt_cmap_from_ops(crdt_ctx *ctx, const uint64_t *op_key_dev, const uint32_t *op_rep_dev,
                       const uint64_t *op_dp_dev, const uint64_t *op_dn_dev, size_t m,
                       const crdt_cmap *out, uint64_t *count_dev);

/* ------------------------------------------- streaming peaks
 * Measurement utilities, no reference counterpart: the bench reports every
 * kernel's fraction of a self-measured copy-kernel peak beside the spec peak.
 * crdt_stream_copy: dst = src, `bytes` (multiple of 16, 16-B aligned), 16-B
 * nontemporal loads / stores, `unroll` in {1,2,4,8} vectors in flight per
 * lane, grid = CUs x blocks_per_cu workgroups of 256.
 * crdt_stream_read: reads `bytes` of src, writes one word per workgroup to
 * sink_dev (sink_words >= CUs x blocks_per_cu). */
int crdt_stream_copy(crdt_ctx *ctx, const void *src_dev, void *dst_dev, size_t bytes, int unroll,
                     int blocks_per_cu);
int crdt_stream_read(crdt_ctx *ctx, const void *src_dev, size_t bytes, uint64_t *sink_dev, size_t sink_words,
                     int unroll, int blocks_per_cu);

/* ------------------------------------------------------ vector clocks (a7) */
typedef enum crdt_vc_class {
    CRDT_VC_EQUAL = 0,      /* a == b                  */
    CRDT_VC_BEFORE = 1,     /* a <  b  (a happened-before b) */
    CRDT_VC_AFTER = 2,      /* a >  b                  */
    CRDT_VC_CONCURRENT = 3  /* neither dominates        */
} crdt_vc_class;
/* Join of vector clocks is the elementwise max: crdt_gcounter_join. */
/* The causal-stability cut of a population of [rows x nodes] uint64 clocks:
 * out[c] = min_r clocks[r][c] (unsigned) -- the number of node c's events that
 * every replica has seen; what crdt_set_compact takes as its cut.  The
 * column-min twin of crdt_gcounter_fold (same two paths: nodes a power of two
 * in [2, 512] on a 16-byte aligned base streams 16-byte loads, anything else
 * takes the generic kernel).  rows == 0 is CRDT_E_INVAL: the minimum over no
 * replica is all-ones, a cut under which every tombstone could go.  nodes ==
 * 0, a NULL pointer or rows * nodes overflowing: CRDT_E_INVAL.  Stream-ordered,
 * no host synchronisation (capturable after crdt_ctx_reserve). */
int crdt_vclock_stable_cut(crdt_ctx *ctx, const uint64_t *clocks_dev, size_t rows, size_t nodes,
                           uint64_t *out_dev);
/* cls[p] = classify(a[p], b[p]) for [pairs x nodes] uint64 clocks.  With
 * nodes == 1 this is the sign of Int64Comparator (main.go:106) on unsigned
 * values, mapped EQUAL/BEFORE/AFTER. */
int crdt_vclock_classify(crdt_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev,
                         uint8_t *cls_dev, size_t pairs, size_t nodes);

/* ---------------------------------------------- LWW-Element-Set / OR-Set (a8)
 * Structure-of-arrays tuples, sorted ascending by (key, ts, rep).
 * Tie rule: on an exactly equal (ts, rep) the left operand (a, the local
 * replica) wins, as the reference keeps the local value on an equal
 * timestamp (main.go:54-65). */
typedef struct crdt_tuples {
    uint64_t *key;
    uint64_t *ts;
    uint32_t *rep;
    uint8_t  *tomb;
} crdt_tuples;

/* LWW: one tuple per distinct key = the max (ts, rep) element (left wins an
 * exact tie; tombstoned winners are kept).  out capacity >= na + nb;
 * *out_count_dev (device uint64) receives the output length.  key / ts / rep
 * must be naturally aligned (8 / 8 / 4 bytes; CRDT_E_INVAL otherwise): the
 * passes stage them by LDS-DMA from any element offset. */
int crdt_lww_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b,
                   size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
/* OR-Set: union of unique tags (key, ts, rep); tomb OR-ed over equal tags. */
int crdt_orset_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b,
                     size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
/* ---- merges that carry a payload: where every output tuple came from (the
 * reference's state is key -> value, Diff.Put of a value with its key at
 * main.go:60-64 and :187; a tuple has no value column, so the merge names
 * the input tuple and crdt_src_gather moves any number of value columns).
 * crdt_lww_merge_src / crdt_orset_merge_src write out and *out_count_dev bit
 * for bit as crdt_lww_merge / crdt_orset_merge do for the same inputs, under
 * the same preconditions, alignment rules, error codes and (no)
 * synchronisation, and also src_out_dev[i] = the source of out[i], encoded as
 * crdt_refmerge_out.src: >= 0 an index into a; < 0 b's index j as -(j + 1).
 * src_out_dev holds >= na + nb int64, 8-byte aligned; entries at or past the
 * count are unspecified.  Which copy is the source -- merged order is the
 * stable merge of a and b by (key, ts, rep): a's copies of an equal tag before
 * b's, each side in its input order:
 *   LWW    : the first element in merged order that carries the key's maximal
 *            (ts, rep); all four output fields are that element's.
 *   OR-Set : the first element in merged order of the tag; key, ts and rep
 *            are that element's, tomb stays the OR over all copies (it may be
 *            1 where the source's is 0).
 * CRDT_E_INVAL besides the plain merges' cases: src_out_dev NULL with na + nb
 * > 0, misaligned, or overlapping a, b or out. */
int crdt_lww_merge_src(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                       crdt_tuples *out, int64_t *src_out_dev, uint64_t *out_count_dev);
int crdt_orset_merge_src(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                         crdt_tuples *out, int64_t *src_out_dev, uint64_t *out_count_dev);
/* out_col[i] = src[i] >= 0 ? a_col[src[i]] : b_col[-(src[i] + 1)] for i < n,
 * elements of elem_size in {1, 2, 4, 8, 16} bytes: one payload column moved
 * by a merge's source indices (one call per column; columns naturally aligned
 * to elem_size).  n from n_max / n_dev exactly as in crdt_set_elements: NULL
 * -> n_max; *n_dev <= n_max -> the first *n_dev (pass the merge's
 * out_count_dev: no read-back between the merge and the gather); *n_dev >
 * n_max (the ~0 of a plan miss included) -> nothing is touched and
 * CRDT_DEV_RANGE is raised.  An index outside its side (src >= na, or
 * -(src + 1) >= nb) is never dereferenced: its output element is left as it
 * was and CRDT_DEV_RANGE is raised; every other element is still written.
 * Stream-ordered, no host synchronisation, no workspace (capturable).
 * CRDT_E_INVAL: a bad elem_size, a NULL src / out_col or a NULL side with a
 * nonzero length, misalignment (src and n_dev to 8 bytes, the columns to
 * elem_size), out_col overlapping an input column or src; CRDT_E_RANGE: n_max
 * >= 2^62 (or a side of 2^59 elements or more).  n_max == 0 launches nothing. */
int crdt_src_gather(crdt_ctx *ctx, const int64_t *src_dev, size_t n_max, const uint64_t *n_dev,
                    const void *a_col_dev, size_t na, const void *b_col_dev, size_t nb,
                    void *out_col_dev, size_t elem_size);
/* The same two merges on UNSORTED inputs (config D2), as one device sort of
 * both sides together with a side bit between rep and tomb -- composite
 * order (key, ts, rep, side, tomb) is the stable merge of the two sorted
 * sides -- followed by a neighbour dedup of the sorted composites.  Where
 * the key offsets are dense enough no radix pass runs: the tuples are
 * grouped per tile by the key's top byte, then LWW gathers each byte's runs
 * into an LDS table of per-key winners and OR-Set gathers them into 2^9-key
 * chunks sorted in LDS; on large calls those forms are planned from a
 * sample of the inputs that the grouping pass checks (a miss redoes the
 * call from the exact ranges), and a context keeps the last sampled plan
 * per mode and size (later calls of that size launch from it with no
 * sample and no read-back; a tuple outside its ranges is a miss).  Output identical to
 * crdt_tuples_sort of each side then crdt_lww_merge / crdt_orset_merge.
 * Synchronises once at the end in the dense-key forms (the sample's check,
 * the OR-Set chunks' LDS limits), once more to read a plan the context does
 * not hold, and once to size the radix passes otherwise.  na + nb < 2^32; out capacity >=
 * na + nb; out must not overlap a or b (CRDT_E_INVAL: the dense-key forms
 * store before they know whether the call is redone from the inputs). */
int crdt_lww_merge_unsorted(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b,
                            size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
int crdt_orset_merge_unsorted(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b,
                              size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
/* Stream-ordered D2 merges (no host synchronisation: a HIP graph can capture
 * them).  The calls above may read their plan -- field ranges, composite
 * layout, which dense-key form applies -- back from the device and check the
 * sampled ranges at the end (one synchronisation each).  A host that merges
 * the same shape repeatedly (a replica population's key space; the gossip
 * loop of main.go:226-258 calls merge() every round) plans once:
 * crdt_set_merge_plan (mode 0 = LWW, 1 = OR-Set; synchronises once) computes
 * the exact plan of a, b -- widen != 0 widens each field range by 1/256 of
 * its span, for later inputs that drift -- and reserves the context's
 * workspace for it.  The _planned calls then enqueue the merge with no
 * read-back, for inputs of the same na / nb (CRDT_E_INVAL otherwise): the
 * composing pass checks every tuple against the plan, and a tuple outside it
 * (or an OR-Set key chunk over its LDS limits) raises CRDT_DEV_PLAN in the
 * context's status word and sets *out_count_dev = ~0 -- run the unplanned
 * call then.  Otherwise the output is the unplanned call's, bit for bit. */
typedef struct crdt_set_plan {
    uint64_t w[24];
} crdt_set_plan;
int crdt_set_merge_plan(crdt_ctx *ctx, int mode, const crdt_tuples *a, size_t na, const crdt_tuples *b,
                        size_t nb, uint32_t widen, crdt_set_plan *plan);
int crdt_lww_merge_unsorted_planned(crdt_ctx *ctx, const crdt_set_plan *plan, const crdt_tuples *a, size_t na,
                                    const crdt_tuples *b, size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
int crdt_orset_merge_unsorted_planned(crdt_ctx *ctx, const crdt_set_plan *plan, const crdt_tuples *a, size_t na,
                                      const crdt_tuples *b, size_t nb, crdt_tuples *out, uint64_t *out_count_dev);
/* Sort n SoA tuples (device) into ascending (key, ts, rep, tomb) order --
 * the merge input order, with tomb (0/1) breaking exact tag ties so the
 * result does not depend on the input order (config D2: unsorted state).
 * LSD radix sort of a packed composite of the fields' offsets from their
 * minima; synchronises the stream once (to size the passes).  in and out
 * must not overlap.  n < 2^32. */
int crdt_tuples_sort(crdt_ctx *ctx, const crdt_tuples *in, size_t n, crdt_tuples *out);
/* out[i] = lower_bound(sorted[0..n), probes[i]) in unsigned order, for m
 * probes (device arrays): key-range sharding of a sorted set (§8(e) D). */
int crdt_u64_lower_bound(crdt_ctx *ctx, const uint64_t *sorted_dev, size_t n, const uint64_t *probes_dev,
                         size_t m, uint64_t *out_dev);
/* ---- set reads: which keys are in a merged set state (the reference serves
 * its materialised CurrentState on GET /data, main.go:129-139).
 * Live keys of a set state t sorted by (key, ts, rep), ascending, each once,
 * into keys_out_dev; their number into *count_dev (device uint64).  mode as
 * in crdt_set_merge_plan.  OR-Set: a tag is live iff none of its copies is
 * tombstoned, a key is a member iff it has a live tag.  LWW: a key is a
 * member iff the first copy of its maximal (ts, rep) tag has tomb == 0 (the
 * winner crdt_lww_merge keeps).  Either way the keys of merge(t, {}) whose
 * (OR-Set: any) output tuple has tomb == 0.  keys_out_dev may be NULL:
 * cardinality only (one pass, nothing written but the count).
 * n_dev (device uint64, may be NULL) gives the tuple count on the device, as
 * crdt_seg_gather2_n does: NULL -> n_max tuples; *n_dev <= n_max -> the first
 * *n_dev (pass a merge's out_count_dev and its output capacity: no read-back
 * between the merge and the read); *n_dev > n_max (the ~0 a planned merge
 * leaves on a plan miss included) -> no tuple is touched, *count_dev = ~0 and
 * CRDT_DEV_RANGE is raised.  No kernel reads at or past min(*n_dev, n_max).
 * Stream-ordered, no host synchronisation (capturable after
 * crdt_ctx_reserve).  keys_out_dev holds >= n_max keys and must not overlap
 * t; key / ts / rep naturally aligned (the merges' rule).  CRDT_E_INVAL: NULL
 * ctx / t / count_dev, bad mode, misalignment, overlap; CRDT_E_RANGE: n_max
 * >= 2^62.  n_max == 0 launches nothing but the count store. */
#define CRDT_SET_LWW   0
#define CRDT_SET_ORSET 1
int crdt_set_elements(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                      uint64_t *keys_out_dev, uint64_t *count_dev);
/* out[i] = 1 iff probes[i] occurs in sorted_dev[0 .. n) (unsigned order), for
 * m probes; n from n_max / n_dev as above (*n_dev > n_max: out all zero and
 * CRDT_DEV_RANGE).  Membership in the keys crdt_set_elements wrote, with its
 * count_dev as n_dev.  Stream-ordered, no host synchronisation. */
int crdt_u64_contains(crdt_ctx *ctx, const uint64_t *sorted_dev, size_t n_max, const uint64_t *n_dev,
                      const uint64_t *probes_dev, size_t m, uint8_t *out_dev);
/* ---- map reads: the key -> value view of a set state that keeps a value
 * column beside its tuples (what the reference serves: CurrentState on GET
 * /data, main.go:129-139).  t[0 .. n) sorted ascending by (key, ts, rep),
 * copies of one tag in any order and number; n from n_max / n_dev exactly as
 * in crdt_set_elements; mode CRDT_SET_LWW or CRDT_SET_ORSET (a causal-form
 * state, whose tombs are all 0, is read with CRDT_SET_ORSET).
 *   member keys : exactly those of crdt_set_elements(mode, t), ascending, one
 *                 row each.
 *   winner      : OR-Set -- the greatest (ts, rep) live tag of the key; a tag
 *                 is live iff none of its copies is tombstoned.  LWW -- the
 *                 key's maximal tag; the key is a member iff the tomb of that
 *                 tag's first copy is 0.
 *   win (int64) : the index in t of the first copy of the winner tag: the
 *                 a-side encoding of crdt_src_gather, so
 *                 crdt_src_gather(win, n_max, count_dev, val, n, NULL, 0,
 *                 out_val, elem) yields the map's values with no read-back.
 *   nsib (u32)  : OR-Set -- the number of distinct live tags of the key, at
 *                 least 1, saturating at 2^32 - 1; LWW -- 1.  nsib > 1 marks a
 *                 key that concurrent puts left multi-valued.
 * crdt_map_read writes one row per member key, in ascending key order, and
 * their number to *count_dev (device uint64).  keys_out_dev and nsib_out_dev
 * may each be NULL (a NULL nsib_out_dev costs nothing: the sibling walk is
 * compiled out); win_out_dev is required when n_max > 0.  Each output holds at
 * least n_max rows, is naturally aligned, and overlaps neither t nor another
 * output.  *n_dev > n_max: no tuple is touched, nothing is written to the
 * outputs, *count_dev = ~0 and CRDT_DEV_RANGE is raised.  No kernel reads a
 * tuple at or past min(*n_dev, n_max) or before 0.  Stream-ordered, no host
 * synchronisation (capturable after crdt_ctx_reserve).  CRDT_E_INVAL: NULL ctx
 * / t / count_dev, bad mode, NULL fields of t or a NULL win_out_dev with n_max
 * > 0, misalignment, overlap; CRDT_E_RANGE: n_max >= 2^62 or more tiles than a
 * launch holds.  n_max == 0 launches nothing but the count store. */
int crdt_map_read(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                  uint64_t *keys_out_dev, int64_t *win_out_dev, uint32_t *nsib_out_dev, uint64_t *count_dev);
/* Point lookup against the same state: m probe keys in any order, duplicates
 * allowed.  win_out_dev[i] = the win crdt_map_read gives probes_dev[i], or -1
 * if the key is not a member; nsib_out_dev (may be NULL) its nsib, 0 for a
 * non-member.  To crdt_src_gather -1 is element 0 of the b side, so a gather
 * by win_out_dev with a one-element b_col writes a caller-chosen default for
 * the missing keys and raises nothing.  *n_dev > n_max: every win_out is -1,
 * every nsib_out 0, and CRDT_DEV_RANGE is raised (as crdt_u64_contains).  One
 * thread per probe: a binary search on t.key clamped to the length, then the
 * key's tags from its run's end; no workspace, no synchronisation; m == 0
 * launches nothing.  CRDT_E_INVAL: NULL ctx / t, bad mode, and with m > 0 a
 * NULL probes_dev / win_out_dev, NULL fields of t with n_max > 0,
 * misalignment, an output overlapping t, probes_dev or the other output;
 * CRDT_E_RANGE: n_max >= 2^62 or m >= 2^60. */
int crdt_map_lookup(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                    const uint64_t *probes_dev, size_t m, int64_t *win_out_dev, uint32_t *nsib_out_dev);
/* ---- set deltas: the tuples of one set state that another lacks (the
 * reference's gossip pull ships the entire Diff every round, main.go:153-170
 * and :245-256).  delta(src, dst) = the smallest set of tuples D with
 * merge(dst, D) == merge(dst, src) bit for bit, dst the left (tie-winning)
 * operand of crdt_lww_merge / crdt_orset_merge; both sides sorted by (key, ts,
 * rep), copies of one tag in any order on either side.  OR-Set: a tag of src
 * ships iff dst holds no copy of it, or the OR of src's copies' tombs is 1 and
 * that of dst's is 0; once, with src's tomb-OR.  LWW: src's winner of a key
 * (its maximal (ts, rep) tag, the tomb of that tag's first copy) ships iff dst
 * holds no tuple of the key or src's maximal tag is strictly greater than
 * dst's (an equal tag stays: the merge keeps dst's copy).  D is written to
 * out in ascending tuple order, its size to *count_dev (device uint64);
 * delta(src, {}) == merge(src, {}), delta({}, dst) and delta(src, merge(dst,
 * src)) are empty -- the in-sync test.  out may be NULL: the count alone (no
 * bitmaps, no offsets, nothing stored but *count_dev).
 * ns_dev / nd_dev follow crdt_set_elements' n_dev, each on its own: NULL ->
 * all n_max tuples of the side; <= n_max -> the first so many; > n_max on
 * either side -> no tuple of either side is touched, nothing is written to
 * out, *count_dev = ~0 and CRDT_DEV_RANGE is raised.  No kernel reads an index
 * at or past min(*n_dev, n_max) of its side.  Stream-ordered, no host
 * synchronisation (capturable after crdt_ctx_reserve).  out holds >= ns_max
 * tuples and must not overlap src or dst.  CRDT_E_INVAL: NULL ctx / src / dst
 * / count_dev, bad mode, NULL fields of a side with n_max > 0, key / ts / rep
 * of any operand not naturally aligned, out overlapping an input;
 * CRDT_E_RANGE: ns_max or nd_max >= 2^62 or more tiles than a launch holds.
 * ns_max == 0 launches nothing but the count store. */
int crdt_set_delta(crdt_ctx *ctx, int mode, const crdt_tuples *src, size_t ns_max, const uint64_t *ns_dev,
                   const crdt_tuples *dst, size_t nd_max, const uint64_t *nd_dev, const crdt_tuples *out,
                   uint64_t *count_dev);
/* ---- tombstone compaction under a causal-stability cut (no reference
 * counterpart: the reference's Diff only grows).  The merges keep tombstoned
 * LWW winners and every OR-Set tag ever seen; this call drops the dead tuples
 * that every replica is known to hold.
 * Stable: for a cut cut_dev[0 .. n_cut) of uint64, a tag (key, ts, rep) is
 * stable iff rep < n_cut and ts <= cut[rep] (unsigned compare).  A rep at or
 * past n_cut is never stable; n_cut == 0 (cut_dev may then be NULL): nothing is.
 * compact(t, cut), t sorted ascending by (key, ts, rep), copies of one tag in
 * any order, is merge(t, {}) with the stable dead tuples removed:
 *   OR-Set : per distinct tag, tomb = the OR over its copies; the tag is
 *            dropped iff that OR is 1 and the tag is stable, otherwise written
 *            once with that OR.
 *   LWW    : per distinct key, the winner is the maximal (ts, rep) tag with the
 *            tomb of that tag's first copy (crdt_lww_merge's winner); the key
 *            is dropped iff the winner's tomb is 1 and the winner is stable,
 *            otherwise the winner is written.
 * out receives the kept tuples in ascending tuple order, *count_dev (device
 * uint64) their number: a sorted state the merges, reads and deltas accept.
 * compact(t, no cut) == merge(t, {}) bit for bit; crdt_set_elements of the
 * result equals that of t for every cut; compact is idempotent; a cut that is
 * column-wise >= another yields a subsequence of the other's result.
 * THE CALLER'S OBLIGATION (not enforced): the cut must cover the REMOVE as
 * well as the add -- every replica already holds the tombstone of every tag
 * the cut makes stable (e.g. ts counts rep's events, add and remove alike, and
 * the cut is crdt_vclock_stable_cut of the replicas' clocks).  A dropped
 * tombstone that some replica has not seen lets that replica's live copy
 * resurrect the element at the next merge.
 * src_out_dev (may be NULL): per output tuple the index into t of the tuple it
 * is -- LWW: the first copy of the winner tag; OR-Set: the first copy of the
 * tag (its tomb may be 0 where the output's OR is 1) -- the copies
 * crdt_*_merge_src(t, {}) names, encoded as that call's a-side (>= 0), so
 * crdt_src_gather(src, n_max, count_dev, col, n, NULL, 0, out_col, elem)
 * compacts a value column with no read-back.
 * out may be NULL: the count alone (no bitmaps, no offsets, nothing stored but
 * *count_dev); src_out_dev must then be NULL too.
 * n_dev follows crdt_set_elements' n_dev: NULL -> n_max tuples; *n_dev <= n_max
 * -> the first *n_dev; *n_dev > n_max -> no tuple is touched, nothing is
 * written to out or src_out_dev, *count_dev = ~0 and CRDT_DEV_RANGE is raised.
 * No kernel reads a tuple at or past min(*n_dev, n_max) or before 0 (the write
 * pass checks every position of its bitmaps against that length before it
 * loads), nor cut_dev at or past n_cut.  Stream-ordered, no host
 * synchronisation (capturable after crdt_ctx_reserve).  out holds >= n_max
 * tuples, src_out_dev >= n_max int64; neither may overlap t, cut_dev or the
 * other.  CRDT_E_INVAL: NULL ctx / t / count_dev, bad mode, NULL fields of t
 * or out with n_max > 0, key / ts / rep of t or out not naturally aligned,
 * cut_dev NULL with n_cut > 0, cut_dev or src_out_dev not 8-byte aligned,
 * src_out_dev without out, an overlap as above; CRDT_E_RANGE: n_max >= 2^62,
 * n_cut >= 2^32, or more tiles than a launch holds.  n_max == 0 launches
 * nothing but the count store. */
int crdt_set_compact(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                     const uint64_t *cut_dev, size_t n_cut, const crdt_tuples *out, int64_t *src_out_dev,
                     uint64_t *count_dev);
/* ---- the tombstone-free OR-Set: a causal merge under version vectors (no
 * reference counterpart; the optimised OR-Set of Bieniusa et al., Riak's
 * ORSWOT).  crdt_set_compact drops a tombstone only under a cut over ALL
 * replicas' clocks; here every state carries its own causal context instead
 * and a remove leaves nothing behind, so state is proportional to the live
 * tags and no population-wide cut is ever needed.
 * A causal state is a pair (tuples, context): tuples sorted ascending by (key,
 * ts, rep), copies of one tag in any order and any number on either side; the
 * context ctx_dev[0 .. n_ctx) of uint64, ctx[r] = the events of replica r the
 * state has seen (n_ctx == 0: ctx_dev may be NULL).
 * Present: side X holds tag g = (key, ts, rep) as present iff it holds at least
 * one copy of g and the OR of its copies' tombs is 0 -- crdt_set_elements' live
 * tag.  A tombstoned tag counts as absent, which is also the way in from the
 * tombstone form: merge a tombstone-form state with its replica's clock.
 * Covered: covered(g, v, n) iff g.rep < n and g.ts <= v[g.rep] (unsigned
 * compare) -- crdt_set_compact's "stable".  A rep at or past n is never
 * covered; with n == 0 nothing is.
 * Merge rule: tag g is in merge(a, b) iff
 *   g is present in a and in b, or
 *   g is present in a and not covered by b's context, or
 *   g is present in b and not covered by a's context
 * (a side whose context covers a tag it does not hold has seen and removed it).
 * out receives each surviving tag once, in ascending tuple order, with tomb =
 * 0; *count_dev (device uint64) their number: a sorted state the merges, reads,
 * deltas and digests accept.
 * src_out_dev (may be NULL): per output tuple the input tuple it is, in
 * crdt_orset_merge_src's encoding (>= 0 an index into a; < 0 b's index j as
 * -(j + 1)), so crdt_src_gather moves value columns with no read-back.  Merged
 * order is the stable merge of a and b: a's copies of a tag before b's, each
 * side in its input order.  The copy named is the first copy, in merged order,
 * ON A SIDE WHERE THE TAG IS PRESENT: a's first copy of the tag when a holds it
 * present, otherwise b's first copy.  So with a tombstoned copy on a and the
 * live one on b (a surviving tag then: present in b, not covered by a's
 * context) b's first copy is named, not the tag's first copy in merged order;
 * the copy named may itself carry tomb = 0 only (a present side has no other).
 * ctx_out_dev (may be NULL): max(n_ctx_a, n_ctx_b) uint64, ctx_out[c] =
 * max(c < n_ctx_a ? ctx_a[c] : 0, c < n_ctx_b ? ctx_b[c] : 0).  It depends on
 * the contexts only and is written whatever the lengths are (a poisoned length
 * included).  It must not overlap any input.
 * out may be NULL: the count alone (no bitmaps, no offsets); src_out_dev must
 * then be NULL too and nothing is stored but *count_dev and ctx_out_dev.
 * THE CALLER'S OBLIGATION (not enforced): every present tag of a state is
 * covered by that state's own context, and contexts are contiguous -- v[r] = n
 * means the state has seen events 1 .. n of r (ts counts rep's events, as in
 * crdt_set_compact's contract).  Under these the merge is commutative (equal
 * tuples and equal ctx_out for either operand order), associative and
 * idempotent (merge(A, A) = A's present tags), and (out, ctx_out) is again
 * such a state.  Local adds and removes are crdt_set_apply's (below): every
 * operation of replica r, add and remove alike, is r's next event ++ctx[r]; an
 * add inserts (key, that event, r), a remove deletes the key's tuples, and an
 * event number with no tag is "seen and removed", so the context stays
 * contiguous.
 * na_dev / nb_dev follow crdt_set_delta's ns_dev, each on its own: NULL -> all
 * n_max tuples of the side; <= n_max -> the first so many; > n_max on either
 * side -> no tuple of either side is touched, nothing is written to out or
 * src_out_dev, *count_dev = ~0 and CRDT_DEV_RANGE is raised.  No kernel reads a
 * tuple at or past min(*n_dev, n_max) of its side or before 0 (the write pass
 * checks every position of its bitmaps against those lengths before it loads),
 * nor a context at or past its n_ctx.  Stream-ordered, no host synchronisation;
 * workspace from the context only (capturable after crdt_ctx_reserve).  key /
 * ts / rep naturally aligned but otherwise at arbitrary offsets.  out holds >=
 * na_max + nb_max tuples, src_out_dev as many int64; neither may overlap an
 * input, ctx_out_dev or the other.
 * CRDT_E_INVAL: NULL ctx / a / b / count_dev, NULL fields of a side with n_max
 * > 0 or of out with na_max + nb_max > 0, key / ts / rep of any operand not
 * naturally aligned, a context NULL with its n_ctx > 0, a context, na_dev,
 * nb_dev, src_out_dev, ctx_out_dev or count_dev not 8-byte aligned, src_out_dev
 * without out, an overlap as above; CRDT_E_RANGE: na_max or nb_max >= 2^62,
 * n_ctx_a or n_ctx_b >= 2^32, or more tiles than a launch holds.  na_max +
 * nb_max == 0 launches nothing but the count store and the ctx_out write. */
int crdt_orset_merge_causal(crdt_ctx *ctx,
                            const crdt_tuples *a, size_t na_max, const uint64_t *na_dev,
                            const uint64_t *ctx_a_dev, size_t n_ctx_a,
                            const crdt_tuples *b, size_t nb_max, const uint64_t *nb_dev,
                            const uint64_t *ctx_b_dev, size_t n_ctx_b,
                            const crdt_tuples *out, int64_t *src_out_dev, uint64_t *ctx_out_dev,
                            uint64_t *count_dev);
/* ---- the causal merge restricted to key ranges: digest anti-entropy for the
 * tombstone-free OR-Set.  crdt_orset_merge_causal is not monotone: a tag a
 * holds and b's context covers is dropped unless b's copy of it is in the
 * operand, so merging a with a SELECTION of b (crdt_set_select of the buckets
 * whose digests differ) would delete tags wherever the replicas already agree.
 * This call takes the buckets along and does not.
 * a is the receiver's whole causal state with its context; b is whatever the
 * peer shipped, normally crdt_set_select(B, CRDT_SET_ORSET, splitters, flags);
 * ctx_b the peer's WHOLE context.  Buckets are crdt_set_digest's, exactly:
 * bucket(key) = #{ j : splitters_dev[j] <= key } under unsigned compare, m + 1
 * buckets, equal neighbouring splitters allowed; m == 0: one bucket
 * (splitters_dev may then be NULL).  flags_dev[bk] != 0 (m + 1 uint8, e.g.
 * crdt_set_digest_diff's): bucket bk is flagged.
 * For a tag g with bucket(g.key) flagged, crdt_orset_merge_causal's rule applies
 * unchanged.  For a tag g with bucket(g.key) NOT flagged, b is taken to hold
 * what a holds: g survives iff it is present in a.  b's copies in such a bucket
 * are ignored entirely -- they add nothing to the tag's state, are never
 * emitted, are never named by src_out_dev and do not revive a tag tombstoned
 * on a -- and neither context is read there.
 * Everything else is crdt_orset_merge_causal's: ascending output, each survivor
 * once, tomb = 0; src_out_dev's encoding and "the first copy on a side where
 * the tag is present, a before b"; ctx_out_dev the element-wise maximum,
 * written whatever the lengths are; out == NULL: the count alone (src_out_dev
 * NULL too); na_dev / nb_dev (nb_dev: crdt_set_select's count_dev, so the
 * selection needs no read-back), a value past its n_max storing *count_dev =
 * ~0 and raising CRDT_DEV_RANGE with out untouched; stream-ordered, no host
 * synchronisation, workspace from the context only (capturable after
 * crdt_ctx_reserve); out holds >= na_max + nb_max tuples.
 * Identities: with every flag set the call equals crdt_orset_merge_causal(a, b)
 * bit for bit (tuples, src, ctx_out, count); with no flag set it gives a's
 * present tags and the merged context.  The call is not symmetric in a and b;
 * a round of it in both directions is (both replicas end with merge(A, B)).
 * THE CALLER'S OBLIGATION (not enforced), besides crdt_orset_merge_causal's: in
 * every unflagged bucket the two replicas' canonical OR-Set tuples (canon
 * below) are equal -- what equal digests say, with probability about 1 - 2^-64
 * per bucket.
 * No kernel reads a splitter at or past m or a flag at or past m + 1, whatever
 * the splitters hold; unsorted splitters are the caller's error: the result is
 * then unspecified, but every access stays in range.
 * CRDT_E_INVAL, CRDT_E_RANGE as crdt_orset_merge_causal, and: CRDT_E_INVAL for
 * flags_dev NULL, splitters_dev NULL with m > 0 or not 8-byte aligned, out /
 * src_out_dev / ctx_out_dev overlapping the splitters or the flags;
 * CRDT_E_RANGE for m >= 2^24. */
int crdt_orset_merge_causal_ranges(crdt_ctx *ctx,
                                   const crdt_tuples *a, size_t na_max, const uint64_t *na_dev,
                                   const uint64_t *ctx_a_dev, size_t n_ctx_a,
                                   const crdt_tuples *b, size_t nb_max, const uint64_t *nb_dev,
                                   const uint64_t *ctx_b_dev, size_t n_ctx_b,
                                   const uint64_t *splitters_dev, size_t m, const uint8_t *flags_dev,
                                   const crdt_tuples *out, int64_t *src_out_dev,
                                   uint64_t *ctx_out_dev, uint64_t *count_dev);
/* ---- the OR-Set mutators: a batch of local adds and removes applied on the
 * device (the reference's local write, AddCommand, main.go:173-207, is
 * crdt_local_apply for its log; this is the same step for the OR-Set, in the
 * tombstone form and in the causal form).  An LWW add or remove needs no call
 * of its own: it is a one-tuple state under crdt_lww_merge.
 * t is a state sorted ascending by (key, ts, rep), copies of one tag in any
 * order and number, its length n_max / n_dev as in crdt_set_compact.  rep is
 * the applying replica and clock_dev[0 .. n_clock) its clock row -- a
 * vector-clock row or a causal context, the same thing here.  The batch is m
 * operations (m a host value): op_key_dev[m] uint64, NON-DECREASING, and
 * op_kind_dev[m] uint8, 0 = add, nonzero = remove.  form is
 * CRDT_APPLY_TOMBSTONE or CRDT_APPLY_CAUSAL.
 * The result is the batch applied one operation at a time in index order.
 * With ts0 = clock[rep] (read on the device), operation i is event e_i = ts0 +
 * 1 + i of rep: EVERY operation is an event, add and remove alike, in both
 * forms -- so ts counts rep's events as crdt_set_compact's contract asks, and
 * a causal context stays contiguous (an event number with no tag is "seen and
 * removed").
 *   add(k)     inserts the tag (k, e_i, rep) with tomb 0.
 *   remove(k)  tombstone form: sets tomb = 1 on every tag of k held at that
 *              point, tags added earlier in the batch included;
 *              causal form: deletes every tag of k held at that point.
 * The output is canonical, as crdt_set_compact(t, no cut) /
 * crdt_orset_merge_causal write it: each tag once, in ascending tuple order;
 * tombstone form: tomb = the OR over the tag's copies, then the removes;
 * causal form: a tag whose tomb-OR in t is 1 counts as absent and is dropped,
 * and every output tomb is 0.  In closed form (what the kernels compute): a
 * tag of t is tombstoned / dropped iff the batch holds any remove of its key;
 * the tag of add i iff a remove of its key sits at an index > i; the output is
 * the sorted union of the survivors.
 * out holds >= n_max + m tuples; *count_dev (device uint64) receives the
 * length.  src_out_dev (may be NULL; n_max + m int64): per output tuple >= 0
 * the index in t of the tag's first copy (crdt_set_compact's choice), or -(i +
 * 1) for the add at batch index i, so crdt_src_gather(src, n_max + m,
 * count_dev, state values, n, per-operation values, m, ...) moves a value
 * column: an OR-Map put with no read-back.  clock_out_dev (may be NULL;
 * n_clock uint64) = clock with [rep] = ts0 + m.  out may be NULL: the count
 * alone; src_out_dev must then be NULL too, clock_out_dev is still written.
 * Poison: *n_dev > n_max, or ts0 + m wrapping past 2^64, touches no tuple,
 * stores *count_dev = ~0 and raises CRDT_DEV_RANGE; out, src_out_dev and
 * clock_out_dev are left as they were.
 * THE CALLER'S OBLIGATION (not enforced): every tag of rep in t has ts <=
 * clock[rep], so a new tag never equals an existing one; the operation keys
 * are non-decreasing.  If either is broken the result is unspecified, but
 * every access stays in range.
 * Identities: m == 0, tombstone form: crdt_orset_merge_src(t, {}) bit for bit
 * (tuples, src, count); m == 0, causal form: the tuples of
 * crdt_orset_merge_causal(t, clock, {}, no context); an adds-only batch,
 * tombstone form: crdt_orset_merge(t, the batch's tags) bit for bit.
 * Stream-ordered, no host synchronisation; workspace from the context only
 * (capturable after crdt_ctx_reserve).  No kernel reads t at or past
 * min(*n_dev, n_max), an operation at or past m or the clock at or past
 * n_clock.  key / ts / rep naturally aligned but otherwise at arbitrary
 * offsets.
 * CRDT_E_INVAL: NULL ctx / t / count_dev / clock_dev, rep >= n_clock, a bad
 * form, NULL fields of t with n_max > 0 or of out with n_max + m > 0, NULL
 * operation arrays with m > 0, key / ts / rep of t or out not naturally
 * aligned, op_key_dev, clock_dev, clock_out_dev, src_out_dev, n_dev or
 * count_dev not 8-byte aligned, src_out_dev without out, any output
 * overlapping any input or another output; CRDT_E_RANGE: n_max or m >= 2^62,
 * n_clock >= 2^32, or more tiles than a launch holds.  n_max + m == 0 launches
 * nothing but the count store and the clock write. */
#define CRDT_APPLY_TOMBSTONE 0
#define CRDT_APPLY_CAUSAL 1
int crdt_set_apply(crdt_ctx *ctx, int form, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                   const uint64_t *clock_dev, size_t n_clock, uint32_t rep,
                   const uint64_t *op_key_dev, const uint8_t *op_kind_dev, size_t m,
                   const crdt_tuples *out, int64_t *src_out_dev, uint64_t *clock_out_dev,
                   uint64_t *count_dev);
/* ---- range digests: find the key ranges in which two set states differ
 * without shipping either (the reference's gossip pull ships the entire Diff
 * every round, main.go:153-170 and :245-256; crdt_set_delta needs both states
 * in one memory).  Both replicas reduce their state to one small fingerprint
 * per key range, exchange the fingerprints (16 bytes a range), ship only the
 * ranges whose fingerprints differ, and may recurse with finer splitters
 * inside those.
 * Canonical form: canon(t, mode) is the tuples of merge(t, {}), t sorted
 * ascending by (key, ts, rep), copies of one tag in any order:
 *   OR-Set : each distinct tag once, tomb = the OR over its copies.
 *   LWW    : per distinct key the maximal (ts, rep) tag, with the tomb of that
 *            tag's FIRST copy (crdt_lww_merge's winner).
 * Buckets: splitters_dev[0 .. m) are ascending uint64 (equal neighbours are
 * allowed and give empty buckets); they define m + 1 buckets, bucket(key) =
 * #{ j : splitters[j] <= key } under unsigned compare.  m == 0 (splitters_dev
 * may then be NULL): one bucket, the whole state.  Unsorted splitters are the
 * caller's error: the digests are then unspecified, but every access stays in
 * range.
 * Tuple hash: with sm(x) the SplitMix64 output function,
 *   x += 0x9E3779B97F4A7C15;
 *   x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *   x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *   sm = x ^ (x >> 31)                                 (all mod 2^64),
 *   h(key, ts, rep, tomb) = sm( sm( sm(key) ^ ts ) ^ ((uint64)rep << 1 | tomb) ).
 * Digest: for every bucket b, hash_out_dev[b] = the sum mod 2^64 of h over
 * canon(t)'s tuples in b and count_out_dev[b] = their number.  Wrapping adds
 * are associative and commutative, so the result is bit-exact however the adds
 * are ordered.  Hence digest(t) == digest(merge(t, {})) == digest(t with any
 * tuples duplicated); two states agree in a bucket with probability about 1 -
 * 2^-64 iff their canonical tuples there are equal.  It is a checksum: it
 * offers no protection against an adversary.
 * crdt_set_digest writes all m + 1 entries of both outputs (it zeroes them
 * itself); n_max == 0: all zero.  n_dev follows crdt_set_compact's: NULL ->
 * n_max tuples; *n_dev <= n_max -> the first *n_dev; *n_dev > n_max -> no tuple
 * is touched, every entry of both outputs = ~0 and CRDT_DEV_RANGE is raised.
 * Common to the three calls: stream-ordered, no host synchronisation
 * (capturable after crdt_ctx_reserve); no kernel reads a tuple at or past
 * min(*n_dev, n_max), a splitter at or past m or a flag at or past m + 1; key /
 * ts / rep naturally aligned but otherwise arbitrary (offset views).
 * CRDT_E_INVAL: NULL ctx / t / an output, bad mode, NULL fields of t or out
 * with n_max > 0, splitters_dev NULL with m > 0, misalignment (key / ts / rep;
 * every uint64 / int64 array to 8 bytes), an output overlapping an input or
 * another output; CRDT_E_RANGE: n_max >= 2^62, m >= 2^24 (n_buckets > 2^24),
 * or more tiles than a launch holds. */
int crdt_set_digest(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                    const uint64_t *splitters_dev, size_t m, uint64_t *hash_out_dev, uint64_t *count_out_dev);
/* flags_out_dev[b] = 1 iff the two digests differ in bucket b -- the hashes or
 * the counts differ, or either count is ~0 (a poisoned digest flags every
 * bucket, even against another poisoned one) -- else 0, for b < n_buckets;
 * *n_diff_dev (device uint64) = the number of flagged buckets.  n_buckets ==
 * 0 stores *n_diff_dev = 0 alone. */
int crdt_set_digest_diff(crdt_ctx *ctx, const uint64_t *hash_a_dev, const uint64_t *count_a_dev,
                         const uint64_t *hash_b_dev, const uint64_t *count_b_dev, size_t n_buckets,
                         uint8_t *flags_out_dev, uint64_t *n_diff_dev);
/* canon(t) restricted to the buckets with flags_dev[b] != 0 (m + 1 flags, e.g.
 * crdt_set_digest_diff's), in ascending tuple order into out, their number to
 * *count_dev: what a replica ships for the differing ranges.  All flags set
 * equals merge(t, {}) bit for bit; no flag set gives count 0.  src_out_dev
 * (may be NULL) has crdt_set_compact's meaning and encoding (the index in t of
 * the first copy of the output's tag), so crdt_src_gather moves value columns
 * with no read-back.  out may be NULL: the count alone; src_out_dev must then
 * be NULL.  out holds >= n_max tuples, src_out_dev >= n_max int64.  *n_dev >
 * n_max: nothing is written to out or src_out_dev, *count_dev = ~0 and
 * CRDT_DEV_RANGE is raised.  n_max == 0 launches nothing but the count store. */
int crdt_set_select(crdt_ctx *ctx, int mode, const crdt_tuples *t, size_t n_max, const uint64_t *n_dev,
                    const uint64_t *splitters_dev, size_t m, const uint8_t *flags_dev,
                    const crdt_tuples *out, int64_t *src_out_dev, uint64_t *count_dev);
/* Sortedness check (host-facing validation): *bad_dev = number of adjacent
 * pairs with t[i] > t[i+1]. */
int crdt_tuples_count_unsorted(crdt_ctx *ctx, const crdt_tuples *t, size_t n,
                               uint64_t *bad_dev);
/* Stable merge of two sorted tuple arrays, every tuple kept (on an equal tag
 * a's copies first): out[0 .. na + nb).  The key-range owner's rank-order
 * merge of received runs in crdt_shard_*_merge_local (the population's side
 * = the stable merge of every rank's side in rank order); its length is known
 * on the host, so a tree of these merges needs no read-back. */
int crdt_tuples_merge(crdt_ctx *ctx, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                      const crdt_tuples *out);

/* ------------------------------------------------ RefMerge (a1-a5)
 * Batched, bit-exact (*Server).merge() (main.go:35-100) for many replicas.
 * Each replica's Diff (L) and RemoteDiff (R) are ascending unique int64 ts
 * arrays (treemap keys under Int64Comparator, main.go:106), concatenated
 * over replicas with CSR offsets.  Entry e owns key/value pairs
 * [kv_off[e], kv_off[e+1]) of one kv arena (L entries' ranges and R
 * entries' ranges both index it).  kv_key is a key SLOT: the host interns
 * each replica's key strings into its own disjoint slot range.  kv_val is a
 * value string id into (str_bytes, str_off).
 * origin: 1 = local write (*Command, main.go:187) -- skipped by the replay
 * (main.go:80); 0 = remote map (main.go:245-255). */
typedef struct crdt_refmerge_in {
    uint32_t replicas;
    uint32_t n_slots;
    uint64_t n_l, n_r, n_kv, n_str;
    const uint64_t *l_off;      /* [replicas+1] */
    const int64_t  *l_ts;       /* [n_l] */
    const uint8_t  *l_origin;   /* [n_l] */
    const uint64_t *l_kv;       /* [n_l+1] */
    const uint64_t *r_off;      /* [replicas+1] */
    const int64_t  *r_ts;       /* [n_r] */
    const uint64_t *r_kv;       /* [n_r+1] */
    const uint32_t *kv_key;     /* [n_kv] slot id < n_slots */
    const uint32_t *kv_val;     /* [n_kv] string id < n_str */
    const uint8_t  *str_bytes;
    const uint64_t *str_off;    /* [n_str+1] */
} crdt_refmerge_in;

typedef struct crdt_refmerge_out {
    uint64_t *off;      /* [replicas+1] new Diff ranges */
    int64_t  *ts;       /* capacity n_l + n_r: new Diff keys, ascending per replica */
    uint8_t  *origin;   /* origin of each new Diff entry */
    int64_t  *src;      /* >= 0: index into L; < 0: R index j encoded as -(j+1) */
    uint8_t  *st_kind;  /* [n_slots] CurrentState: 0 absent, 1 verbatim, 2 sum */
    uint32_t *st_str;   /* [n_slots] verbatim value string id (kind 1) */
    int64_t  *st_sum;   /* [n_slots] Itoa() operand (kind 2) */
} crdt_refmerge_out;

/* All pointers in `in` / `out` are device pointers. */
int crdt_refmerge_batch(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_refmerge_out *out);
/* crdt_refmerge_batch that also materialises the new Diff's kv pairs (the
 * values the reference's Diff.Put carries along with each key, main.go:60-64):
 * new entry i owns kv_key/kv_val[kv_off[i] .. kv_off[i+1]), a copy of its
 * source entry's pairs (out.src), and kv_off[out.off[replicas]] = the total
 * (also written at kv_off[n_l + n_r]).
 * The kv offsets come out of the merge's own passes, so the separate
 * segmented gather over out.src (crdt_seg_gather2_n) is not needed.
 * kv_off: capacity n_l + n_r + 1; kv_key / kv_val: capacity kv_cap (a total
 * over kv_cap raises CRDT_DEV_RANGE, nothing written past it). */
typedef struct crdt_refmerge_kv_out {
    uint64_t *kv_off;
    uint32_t *kv_key;
    uint32_t *kv_val;
    uint64_t kv_cap;
} crdt_refmerge_kv_out;
int crdt_refmerge_batch_kv(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_refmerge_out *out,
                           const crdt_refmerge_kv_out *kv);
/* In-place pulls (an anti-entropy round, main.go:226-261, where every
 * replica's RemoteDiff is a peer's whole Diff already in HBM): replica p's R
 * is r_ts / r_kv [r_off[p] .. r_end[p]) -- ranges may overlap and r_ts /
 * r_kv / the kv arena may alias the L arrays, so no RemoteDiff is
 * assembled.  r_slot_delta (nullable) is added (mod 2^32) to the key slot
 * of every R pair of replica p (a peer's slots re-based to p's).  in->n_r
 * MUST equal the total of the R ranges (outputs sized n_l + n_r): ranges
 * summing past it, or a reversed range (r_end < r_off), raise CRDT_DEV_RANGE
 * and nothing is merged.  out.src of an R entry is -(its index in r_ts) - 1.
 * kv: as crdt_refmerge_batch_kv; REQUIRED (CRDT_E_INVAL otherwise) when
 * r_slot_delta is given -- a gather of the new Diff's pairs by src after
 * the merge cannot re-base the pulled slots. */
typedef struct crdt_refmerge_pull {
    const uint64_t *r_end;          /* [replicas] */
    const uint32_t *r_slot_delta;   /* [replicas] or NULL */
} crdt_refmerge_pull;
int crdt_refmerge_batch_pull(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_refmerge_out *out,
                             const crdt_refmerge_pull *pull, const crdt_refmerge_kv_out *kv);
/* ts-range-sharded RefMerge (§8(e)): one batch of replicas whose logs are
 * split by ts range over G shards (one per GPU).  Steps per shard:
 *   1. crdt_refmerge_local_maxl -> all-reduce(MAX) over shards: max(L) per replica;
 *   2. crdt_refmerge_batch_ex(maxl = that, acc = per-slot accumulators): the
 *      shard's slice of the new Diff (shards concatenate in ts order) and its
 *      unreduced replay fold (state outputs untouched);
 *   3. acc_rank -> all-reduce(MAX) = cmax; acc_owner_str -> all-reduce(SUM);
 *      all-reduce(SUM) of acc.sum and acc.npar; acc_set_best;
 *   4. crdt_refmerge_finalize: CurrentState (st_*) from the reduced accumulators.
 * Integer-only reductions: bit-exact for any shard count. */
typedef struct crdt_refmerge_acc {
    uint64_t *best;     /* [n_slots] 0 = no remote holder; else rank << 32 | string id */
    int64_t  *sum;      /* [n_slots] wrapped sum of the parsable values (main.go:95) */
    uint32_t *npar;     /* [n_slots] number of parsable values */
} crdt_refmerge_acc;
/* maxl_dev (nullable): per-replica max(L) replacing the local L's last key
 * (INT64_MIN: none).  acc (nullable): per-slot accumulators written there
 * instead of finalising st_kind/st_str/st_sum. */
int crdt_refmerge_batch_ex(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_refmerge_out *out,
                           const int64_t *maxl_dev, const crdt_refmerge_acc *acc);
int crdt_refmerge_local_maxl(crdt_ctx *ctx, const crdt_refmerge_in *in, int64_t *maxl_dev);
/* c[s] = best ? shard << 40 | rank : 0  (shards in ts order; shard < 2^23) */
int crdt_refmerge_acc_rank(crdt_ctx *ctx, const crdt_refmerge_acc *acc, size_t n_slots, uint32_t shard,
                           int64_t *c_dev);
/* v[s] = the string id if this shard holds the global max (c == cmax), else 0 */
int crdt_refmerge_acc_owner_str(crdt_ctx *ctx, const crdt_refmerge_acc *acc, size_t n_slots, const int64_t *c_dev,
                                const int64_t *cmax_dev, int64_t *v_dev);
/* acc.best[s] = cmax ? 1 << 32 | v : 0 (the reduced accumulator) */
int crdt_refmerge_acc_set_best(crdt_ctx *ctx, const crdt_refmerge_acc *acc, size_t n_slots, const int64_t *cmax_dev,
                               const int64_t *v_dev);
int crdt_refmerge_finalize(crdt_ctx *ctx, const crdt_refmerge_acc *acc, size_t n_slots, const uint8_t *str_bytes_dev,
                           const uint64_t *str_off_dev, uint64_t n_str, const crdt_refmerge_out *out);

/* Incremental replay (§8(f) row 3).  The reference re-folds the whole Diff
 * on every merge (main.go:76); a merge only adds remote entries, so a
 * per-key state keyed by ts can be carried across merges:
 *   crdt_replay_state_init(L)     -- state of the L logs' remote entries;
 *   crdt_refmerge_delta(L, R, st) -- the merge of crdt_refmerge_batch, but
 *       the replay folds only the inserted R entries into st (updated in
 *       place) and CurrentState (st_*) is finalised from st.
 * Bit-exact with crdt_refmerge_batch as long as st describes the L passed
 * in: after a delta merge the caller's next L is the new Diff.  A local
 * write that replaces a remote entry at the same ms (main.go:187) removes a
 * holder: rebuild st with crdt_replay_state_init then. */
typedef struct crdt_replay_state {
    uint64_t *best_key;  /* [n_slots] max over remote holders of ts ^ 2^63 (order-preserving) */
    uint32_t *best_str;  /* [n_slots] string id of that holder */
    int64_t  *sum;       /* [n_slots] wrapped sum of the parsable values */
    uint32_t *npar;      /* [n_slots] parsable holders */
    uint32_t *nhold;     /* [n_slots] remote holders (0: key absent from CurrentState) */
} crdt_replay_state;
int crdt_replay_state_init(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_replay_state *st);
int crdt_refmerge_delta(crdt_ctx *ctx, const crdt_refmerge_in *in, const crdt_refmerge_out *out,
                        const crdt_replay_state *st);
/* Batched local apply (§8(f) row 1): AddCommand (main.go:173-215) for many
 * replicas in one call.  Replica p's commands are c_off[p] .. c_off[p+1] in
 * ARRIVAL order, command j = (c_ts[j], pairs [c_kv[j], c_kv[j+1]) of the
 * kv_key / kv_val arena, applied in the order given).  Per command, as the
 * handler does: Diff.Put(ts, &data) (main.go:187: an equal ts is REPLACED, so
 * of several same-ms commands the last stays), then the CurrentState apply
 * (main.go:188-207): an absent key is set verbatim and the command stops
 * (status 200); else Atoi(current) + Atoi(value) -> Itoa (int64 wrap), an
 * Atoi failure stops it with status 500.  The new Diff is written like a
 * RefMerge output (src >= 0: Diff index, < 0: command j as -(j+1)); the
 * state (kind/str/sum per key slot, as crdt_refmerge_out) is updated in
 * place.  At most 4096 commands per replica per call: a replica over the
 * limit raises CRDT_DEV_RANGE and nothing of it is applied (its Diff range
 * is empty, its state untouched, its commands' status 0), so the caller can
 * split its commands over several calls; the Alive check (502) is the
 * host's. */
typedef struct crdt_local_in {
    uint32_t replicas;
    uint32_t n_slots;
    uint64_t n_l, n_c, n_kv, n_str;
    const uint64_t *l_off;      /* [replicas+1] the Diffs (ascending unique ts per replica) */
    const int64_t  *l_ts;
    const uint8_t  *l_origin;
    const uint64_t *c_off;      /* [replicas+1] commands per replica */
    const int64_t  *c_ts;       /* [n_c] */
    const uint64_t *c_kv;       /* [n_c+1] pair ranges */
    const uint32_t *kv_key;     /* [n_kv] key slot */
    const uint32_t *kv_val;     /* [n_kv] value string id */
    const uint8_t  *str_bytes;
    const uint64_t *str_off;    /* [n_str+1] */
} crdt_local_in;
typedef struct crdt_local_out {
    uint64_t *off;              /* [replicas+1] */
    int64_t  *ts;               /* capacity n_l + n_c */
    uint8_t  *origin;
    int64_t  *src;
    uint16_t *status;           /* [n_c] HTTP status of each command: 200 / 500 */
    uint8_t  *st_kind;          /* [n_slots] CurrentState, in / out */
    uint32_t *st_str;
    int64_t  *st_sum;
} crdt_local_out;
int crdt_local_apply(crdt_ctx *ctx, const crdt_local_in *in, const crdt_local_out *out);

/* Go strconv.Atoi over a string arena: ok[s] = parsable, val[s] = value. */
int crdt_atoi_batch(crdt_ctx *ctx, const uint8_t *str_bytes_dev, const uint64_t *str_off_dev,
                    uint64_t n_str, uint8_t *ok_dev, int64_t *val_dev);

/* ------------------------------------------------ Server (a4): host mirror
 * The reference's state holder (main.go:23-33) kept on the host, with
 * merge() routed to crdt_refmerge_batch.  Key/value arguments are parallel
 * arrays of (pointer, length) byte strings; a repeated key overwrites (Go
 * map semantics).  All functions lock the server's mutex (main.go:32). */
typedef struct crdt_server crdt_server;
/* NewServer(port, initialState, friendList) (main.go:102-113).  ctx may be
 * NULL for a host-only server (gossip codec, AddCommand): merge() then
 * returns CRDT_E_INVAL. */
int crdt_server_new(crdt_ctx *ctx, int port, crdt_server **out);
int crdt_server_free(crdt_server *srv);
int crdt_server_init_state(crdt_server *srv, const char *const *keys, const size_t *key_lens,
                           const char *const *vals, const size_t *val_lens, size_t n);
/* Diff.Put(ts, value): local != 0 stores a *Command (main.go:187), else a
 * remote map (as merge inserts it, main.go:68).  Replaces an equal ts. */
int crdt_server_diff_put(crdt_server *srv, int64_t ts, int local, const char *const *keys,
                         const size_t *key_lens, const char *const *vals, const size_t *val_lens,
                         size_t n);
/* RemoteDiff.Put(int64(atoi(key)), value): gossip ingest (main.go:250-256). */
int crdt_server_remote_put(crdt_server *srv, int64_t ts, const char *const *keys,
                           const size_t *key_lens, const char *const *vals,
                           const size_t *val_lens, size_t n);
/* AddCommand after JSON decode (main.go:173-215): Diff.Put(ts_ms, &data) and
 * the local apply; *http_status = 200, 500 or 502. */
int crdt_server_add_command(crdt_server *srv, int64_t ts_ms, const char *const *keys,
                            const size_t *key_lens, const char *const *vals,
                            const size_t *val_lens, size_t n, int *http_status);
/* (*Server).merge() (main.go:35-100) on the GPU. */
int crdt_server_merge(crdt_server *srv);
/* merge() of n distinct servers (same device) in ONE batched device call. */
int crdt_servers_merge(crdt_server *const *servers, size_t n);
int crdt_server_diff_len(crdt_server *srv, size_t *n);
int crdt_server_remote_len(crdt_server *srv, size_t *n);
/* Ascending Diff keys and origins (1 = *Command); writes min(cap, len). */
int crdt_server_diff_keys(crdt_server *srv, int64_t *ts, uint8_t *local, size_t cap, size_t *n);
int crdt_server_state_len(crdt_server *srv, size_t *n);
/* i-th CurrentState entry in key order; pointers valid until the next
 * mutation of the server. */
int crdt_server_state_at(crdt_server *srv, size_t i, const char **key, size_t *key_len,
                         const char **val, size_t *val_len);

/* ------------------------------------------------ sharding (a9)
 * Contiguous row range [*begin, *end) of rank `rank` in a world of `world`
 * ranks (replica populations shard by contiguous rows). */
int crdt_shard_range(uint64_t rows, int world, int rank, uint64_t *begin, uint64_t *end);
/* Order-preserving map between uint64 and int64 (x ^ 2^63): lets a signed
 * int64 MAX all-reduce (RCCL/gloo) compute the unsigned max exactly. */
int crdt_u64_to_ordered_i64(crdt_ctx *ctx, const uint64_t *in_dev, int64_t *out_dev, size_t n);
int crdt_ordered_i64_to_u64(crdt_ctx *ctx, const int64_t *in_dev, uint64_t *out_dev, size_t n);

/* Multi-GPU joins over RCCL (xGMI).  The reference's analog is pull gossip of
 * whole logs over HTTP (main.go:226-258); there is no reference collective.
 * A communicator has one or more LOCAL members (a GPU, its crdt_ctx and its
 * RCCL rank):
 *   crdt_shard_comm_create    -- ONE process drives every listed GPU
 *                                (ncclCommInitAll; calls are RCCL groups);
 *   crdt_shard_comm_init_rank -- one member per process (one process per GPU,
 *                                ncclCommInitRank); `id` is rank 0's
 *                                crdt_shard_unique_id, shipped to every rank
 *                                by the host (any channel).
 * Per-member arguments are arrays indexed by member; pointers in them are
 * device pointers on that member's GPU.  Work is enqueued on each member's
 * context stream (crdt_shard_member_ctx) unless a call says it synchronises. */
typedef struct crdt_comm crdt_comm;
#define CRDT_SHARD_ID_BYTES 128
int crdt_shard_unique_id(void *id, size_t cap);
int crdt_shard_comm_create(const int *devices, int n, crdt_comm **out);
int crdt_shard_comm_init_rank(crdt_ctx *ctx, const void *id, int nranks, int rank, crdt_comm **out);
/* Loopback communicator: `members` ranks (1 .. 64) on ONE device in this
 * process, each with its own context and stream; the collectives are device
 * copies and a reduction kernel on a transport stream, ordered against the
 * member streams by events (no host synchronisation).  Every crdt_shard_*
 * protocol runs unchanged on it, so its multi-rank planning, offsets, tree
 * merges and reductions run at R > 1 on one GPU.  Real multi-GPU
 * communicators (the two calls above) use RCCL. */
int crdt_shard_comm_create_loopback(int device, int members, crdt_comm **out);
int crdt_shard_comm_destroy(crdt_comm *comm);
int crdt_shard_comm_info(const crdt_comm *comm, int *members, int *nranks, int *rank0);
enum { CRDT_SHARD_RCCL = 0, CRDT_SHARD_LOOPBACK = 1 };
int crdt_shard_comm_transport(const crdt_comm *comm, int *kind);
/* The RCCL this process runs: *version = ncclGetVersion (e.g. 22606 for
 * 2.26.6) and path (NUL-terminated, truncated to cap) = the shared object
 * the dynamic linker resolved ncclGetVersion to.  The library is linked
 * against /opt/rocm/lib/librccl, but in a process that already loaded
 * another librccl of the same soname (PyTorch's) that one is used. */
int crdt_rccl_info(int *version, char *path, size_t cap);
int crdt_shard_member_ctx(crdt_comm *comm, int member, crdt_ctx **ctx);
int crdt_shard_comm_last_error(const crdt_comm *comm);     /* last ncclResult_t */
int crdt_shard_sync(crdt_comm *comm);
/* Config E1: member i folds its [rows[i] x nodes] row shard (crdt_gcounter_fold),
 * then an all-reduce(max) of the nodes-long folds (RCCL: ncclAllReduce(ncclUint64,
 * ncclMax)): every
 * member's out[i] holds the global join of the whole population. */
int crdt_shard_fold_max_u64(crdt_comm *comm, const uint64_t *const *shard_dev, const size_t *rows, size_t nodes,
                            uint64_t *const *out_dev);
/* Config E2: divergent full-state copies joined in place,
 * ncclAllReduce(ncclUint64, ncclMax). */
int crdt_shard_allreduce_max_u64(crdt_comm *comm, uint64_t *const *buf_dev, size_t n);
/* Generic in-place all-reduce for the sharded RefMerge accumulators. */
enum { CRDT_SHARD_I64 = 0, CRDT_SHARD_U64 = 1, CRDT_SHARD_U32 = 2, CRDT_SHARD_I32 = 3 };
enum { CRDT_SHARD_SUM = 0, CRDT_SHARD_MAX = 1 };
int crdt_shard_allreduce(crdt_comm *comm, void *const *buf_dev, size_t n, int type, int op);
/* Keyed sets: member i contributes local[i] (n_local[i] tuples); every
 * member's out[i] (capacity cap) receives all ranks' tuples concatenated in
 * rank order; *n_total = that length (CRDT_E_RANGE if > cap).  Synchronises. */
int crdt_shard_set_allgather_v(crdt_comm *comm, const crdt_tuples *local, const size_t *n_local,
                               const crdt_tuples *out, size_t cap, size_t *n_total);
/* Key-range-sharded LWW / OR-Set merge of sorted inputs that EVERY member
 * holds in full (a[i], b[i]): splitters = rank quantiles of a sample of both
 * key arrays (identical data, so no exchange), each member merges its range,
 * then crdt_shard_set_allgather_v.  out[i] == crdt_lww_merge / crdt_orset_merge
 * of the whole inputs on every member.  Synchronises. */
int crdt_shard_lww_merge(crdt_comm *comm, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                         const crdt_tuples *out, size_t cap, size_t *n_out);
int crdt_shard_orset_merge(crdt_comm *comm, const crdt_tuples *a, size_t na, const crdt_tuples *b, size_t nb,
                           const crdt_tuples *out, size_t cap, size_t *n_out);

/* All-to-all-v: member i sends send_counts[i * nranks + q] elements of
 * elem_size bytes to global rank q (its send buffer holds the segments in
 * rank order) and receives recv_counts[i * nranks + p] elements from rank p
 * into its recv buffer (segments in rank order); grouped ncclSend / ncclRecv
 * on the member streams, enqueued. */
int crdt_shard_alltoallv(crdt_comm *comm, const void *const *send, const size_t *send_counts, void *const *recv,
                         const size_t *recv_counts, size_t elem_size);
/* Keyed-set merge of a DISTRIBUTED population (the reference
 * analog is the whole-log exchange of main.go:226-258): member i holds only
 * its own tuples a[i] (na[i]) and b[i] (nb[i]), each sorted by (key, ts,
 * rep).  The population's A is the stable merge of every rank's A in rank
 * order (B likewise) and the result is crdt_lww_merge / crdt_orset_merge of
 * the two -- computed by key-range owners: sampled splitters weighted by the
 * ranks' sizes (one ncclAllGather), every rank's tuples sent to their owner
 * (crdt_shard_alltoallv), the owner's merge of the received runs (rank-order
 * pairwise merges of A's runs and of B's, then A with B).  gather != 0:
 * every member's out[i] receives the whole merged state, n_out[i] its
 * length; gather == 0: out[i] / n_out[i] = the member's own key range of it
 * (ranges ascend with rank).  CRDT_E_RANGE if a result exceeds cap.
 * Synchronises. */
int crdt_shard_lww_merge_local(crdt_comm *comm, const crdt_tuples *a, const size_t *na, const crdt_tuples *b,
                               const size_t *nb, const crdt_tuples *out, size_t cap, size_t *n_out, int gather);
int crdt_shard_orset_merge_local(crdt_comm *comm, const crdt_tuples *a, const size_t *na, const crdt_tuples *b,
                                 const size_t *nb, const crdt_tuples *out, size_t cap, size_t *n_out, int gather);
/* The same, each member's own key range only (gather == 0), its length
 * written to n_out_dev[i] (a device uint64 on member i's GPU) on the member
 * stream: no trailing synchronisation (with nranks > 1 planning still reads
 * back the samples and the count matrix).  CRDT_E_RANGE if cap is below a
 * member's received tuples.  Device-side failures: crdt_ctx_device_status. */
int crdt_shard_lww_merge_local_dev(crdt_comm *comm, const crdt_tuples *a, const size_t *na, const crdt_tuples *b,
                                   const size_t *nb, const crdt_tuples *out, size_t cap, uint64_t *const *n_out_dev);
int crdt_shard_orset_merge_local_dev(crdt_comm *comm, const crdt_tuples *a, const size_t *na, const crdt_tuples *b,
                                     const size_t *nb, const crdt_tuples *out, size_t cap,
                                     uint64_t *const *n_out_dev);
/* (*Server).merge() (main.go:35-100) of ONE batch of replicas whose Diff /
 * RemoteDiff logs are split by ts range over the ranks (global rank g holds
 * the g-th ts range of every replica; every member's kv_val ids index the
 * same string table): in[i] / out[i] are member i's slice and outputs in the
 * crdt_refmerge_batch layout.  One call runs the whole protocol on the
 * communicator's streams, no host synchronisation: all-reduce(MAX) of each
 * replica's max(L) (remote ts above the global max are dropped, main.go:49),
 * the local merge, the replay accumulators reduced across ranks (MAX of the
 * holder rank, SUM of its string id, of the wrapped sums and of the
 * parsable counts), CurrentState finalised on every member.  out[i].off /
 * ts / origin / src = member i's slice of the new Diffs (slices concatenate
 * in rank order); st_* = the whole CurrentState.  Bit-exact with
 * crdt_refmerge_batch of the unsharded batch. */
int crdt_shard_refmerge(crdt_comm *comm, const crdt_refmerge_in *in, const crdt_refmerge_out *out);

/* ------------------------------------------------ anti-entropy rounds (§8(f) row 4)
 * The gossip loop of main.go:226-261 for a whole replica population at once:
 * every round each replica pulls one friend's whole Diff (main.go:230, :159),
 * ingests it as remote maps (main.go:245-256) and merges (main.go:257); a
 * dead friend (-1) skips the round (main.go:234-239) -- Diff and CurrentState
 * unchanged.  Rounds are synchronous: every pull sees the Diffs as of the
 * round's start (one legal schedule of the reference's goroutines).  The
 * population's Diffs, string arena and CurrentState stay in HBM between
 * rounds; a round that raises a device flag returns CRDT_E_DEVICE and
 * leaves the population as it was.
 *
 * init (host arrays, the crdt_refmerge_in layout of ONE block of replicas):
 * replicas P, K = keys per replica (local replica i's key k is slot i*K + k),
 * first = the global id of local replica 0; l_off [P + 1] (l_off[0] = 0),
 * l_ts / l_origin (1 = *Command) [n_l], l_kv [n_l + 1] (l_kv[0] = 0),
 * kv_key (local slot ids) / kv_val (string ids) [l_kv[n_l]], the string
 * arena str_bytes / str_off [n_str + 1].  CurrentState starts empty
 * (NewServer with an empty initialState, main.go:102-105). */
typedef struct crdt_population crdt_population;
typedef struct crdt_strtab crdt_strtab;           /* (string tables: below, with the gossip decode) */
typedef struct crdt_population_init {
    uint32_t replicas;
    uint32_t keys_per_replica;
    uint64_t first;
    uint64_t n_str;
    const uint64_t *l_off;
    const int64_t *l_ts;
    const uint8_t *l_origin;
    const uint64_t *l_kv;
    const uint32_t *kv_key;
    const uint32_t *kv_val;
    const uint8_t *str_bytes;
    const uint64_t *str_off;
} crdt_population_init;
int crdt_population_create(crdt_ctx *ctx, const crdt_population_init *init, crdt_population **out);
int crdt_population_destroy(crdt_population *pop);
int crdt_population_info(const crdt_population *pop, uint32_t *replicas, size_t *n_entries, size_t *n_kv);
/* Copy the Diffs (init layout; kv_key as local slot ids) and CurrentState
 * (st_kind 0 absent / 1 string id st_str / 2 decimal st_sum, per slot) to
 * host buffers sized by crdt_population_info; any pointer may be NULL.
 * Synchronises. */
int crdt_population_read(crdt_population *pop, uint64_t *l_off, int64_t *ts, uint8_t *origin, uint64_t *l_kv,
                         uint32_t *kv_key, uint32_t *kv_val, uint8_t *st_kind, uint32_t *st_str, int64_t *st_sum);
/* One round with every peer on this population: local replica i pulls global
 * replica peers[i] (host array of P; == first + i: a self-pull, merge() runs
 * and rebuilds CurrentState, main.go:76; -1: dead).  The merge reads the
 * peers' Diffs in place (crdt_refmerge_batch_pull, key slots re-based, kv
 * pairs from its own passes).  The per-replica arrays go up through a
 * staging kernel that reads them from coherent pinned memory, and the last
 * kernel writes the next Diffs' bounds back into it with a completion word
 * the call polls (no copy-engine transfers; option pop.direct = 0 restores
 * hipMemcpyAsync + hipStreamSynchronize).  Returns once the round is done. */
int crdt_population_round(crdt_population *pop, const int64_t *peers);
/* POST /data on every replica at once (AddCommand, main.go:173-215, through
 * crdt_local_apply): replica p's commands c_off[p] .. c_off[p+1] in ARRIVAL
 * order (host arrays), command j = (c_ts[j], pairs [c_kv[j], c_kv[j+1]) of
 * kv_key (local slot ids of replica p's range) / kv_val (string ids of the
 * population's arena)).  Diff.Put of the *Command (an equal ts replaced,
 * main.go:187), then the CurrentState apply with the early return after a
 * new key and the 500 on an unparsable value (main.go:188-207);
 * status[j] = 200 / 500.  Any number of commands per replica (chunks of
 * 4096 per device call: chunk r = commands r*4096 .. of every replica).  On
 * an error the chunks before the failing one stay applied (their status
 * 200 / 500) and every command of the failing and later chunks has status 0
 * (not applied); a failed call leaves nothing to undo.  Synchronises. */
typedef struct crdt_population_cmds {
    const uint64_t *c_off;      /* [replicas + 1] */
    const int64_t *c_ts;        /* [n_c] */
    const uint64_t *c_kv;       /* [n_c + 1], c_kv[0] = 0 */
    const uint32_t *kv_key;
    const uint32_t *kv_val;
} crdt_population_cmds;
int crdt_population_add_commands(crdt_population *pop, const crdt_population_cmds *cmds, uint16_t *status);
/* Undo the last round (local or sharded): the Diffs and CurrentState as they
 * were before it -- they stay in the population's spare buffers until the
 * next round; CRDT_E_INVAL when there is nothing to undo.  Host bookkeeping
 * only (no synchronisation: later work is ordered on the population's stream). */
int crdt_population_undo(crdt_population *pop);
/* One round over a communicator (main.go:226-258 across GPUs): member i's
 * population (created on crdt_shard_member_ctx(comm, i)) holds global
 * replicas crdt_shard_range(total, nranks, rank0 + i); peers_all [total]
 * (host) is every replica's draw, identical on every rank.  The per-replica
 * counts are all-gathered, every rank sends only the Diffs others pull (one
 * point-to-point group) and merges what it received in place.
 * Synchronises. */
int crdt_population_round_sharded(crdt_comm *comm, crdt_population *const *pops, const int64_t *peers_all,
                                  uint64_t total);
/* One round whose pulls arrive on the wire (main.go:226-258 with the
 * Gossip body of main.go:159 in the binary form of crdt_server_gossip_binary):
 * body i = bodies[body_off[i], body_off[i+1]) (device memory; body_off host,
 * replicas + 1) is local replica i's pulled Diff, an empty body a failed GET
 * (the round skipped for i, main.go:234-239).  Decoded on the device against
 * the string tables (keys: key id k of replica i -> slot i*K + k, ids < K;
 * vals: the value ids -- the first wire round checks that vals holds the
 * population's strings at their ids and adopts its arena), the pulled pairs
 * behind the current Diff's, then merged as crdt_population_round.  A body
 * the device decode does not take (malformed, a nil map, unsorted, a key id
 * >= K) fails the call with CRDT_E_UNSORTED, its status in body_status[i]
 * (host, replicas words): nothing is committed (the previous round can no
 * longer be undone: the merge may already have run into the spare buffers).
 * Synchronises. */
int crdt_population_round_wire(crdt_population *pop, crdt_strtab *keys, crdt_strtab *vals, const uint8_t *bodies,
                               const uint64_t *body_off, uint32_t *body_status);

/* ------------------------------------------------ synthetic state (bench/tests)
 * SplitMix64-seeded generators; identical to the numpy
 * restatement in crdt_amd/synth.py. */
int crdt_synth_counters(crdt_ctx *ctx, uint64_t seed, uint32_t stream, uint64_t *out_dev,
                        size_t n, uint64_t index_base);
int crdt_synth_vclock_pairs(crdt_ctx *ctx, uint64_t seed, uint64_t *a_dev, uint64_t *b_dev,
                            size_t pairs, size_t nodes, uint64_t pair_base);
int crdt_synth_set_tuples(crdt_ctx *ctx, uint64_t seed, uint32_t side, const crdt_tuples *out,
                          size_t n, uint64_t key_space);

/* ------------------------------------------------ anti-entropy rounds (§8(f) row 4)
 * Device assembly of gossip pull rounds (main.go:226-261) for a replica
 * population held in the crdt_refmerge_in layout (crdt_amd/gossip.py).
 * Segmented copy with two sources: segment s copies source segment code[s]
 * (>= 0: A's segment code[s]; < 0: B's segment -code[s]-1, B may be NULL
 * when no code is negative) of elem_size-byte elements (1, 4 or 8) to
 * dst + dst_off[s] * elem_size; with delta (4-byte elements only) each
 * element of segment s gets + delta[s] (mod 2^32: key-slot re-basing).
 * wide = 1: one workgroup per segment (long segments), else one thread. */
int crdt_seg_offsets(crdt_ctx *ctx, size_t n_seg, const int64_t *code_dev, const uint64_t *a_off_dev,
                     const uint64_t *b_off_dev, uint64_t base, uint64_t *dst_off_dev);
int crdt_seg_copy(crdt_ctx *ctx, size_t n_seg, const int64_t *code_dev, const uint64_t *a_off_dev,
                  const uint64_t *b_off_dev, const uint64_t *dst_off_dev, size_t elem_size, const void *a_dev,
                  const void *b_dev, void *dst_dev, const uint32_t *delta_dev, int wide);
/* Two arrays by the same segment map in one pass: segment s of a0/b0 ->
 * dst0 with + delta0[s] (an elem_size-byte integer, mod 2^(8*elem_size);
 * delta0 may be NULL) and, when dst1 != NULL, of a1/b1 -> dst1 verbatim. */
int crdt_seg_copy2(crdt_ctx *ctx, size_t n_seg, const int64_t *code_dev, const uint64_t *a_off_dev,
                   const uint64_t *b_off_dev, const uint64_t *dst_off_dev, size_t elem_size, const void *a0_dev,
                   const void *b0_dev, void *dst0_dev, const void *delta0_dev, const void *a1_dev,
                   const void *b1_dev, void *dst1_dev, int wide);
/* crdt_seg_offsets and a one-thread-per-segment crdt_seg_copy2 (no delta)
 * fused into one pass: each segment is copied as soon as its scanned offset
 * is known (dst_off[n_seg] = base + total). */
int crdt_seg_gather2(crdt_ctx *ctx, size_t n_seg, const int64_t *code_dev, const uint64_t *a_off_dev,
                     const uint64_t *b_off_dev, uint64_t base, uint64_t *dst_off_dev, size_t elem_size,
                     const void *a0_dev, const void *b0_dev, void *dst0_dev, const void *a1_dev,
                     const void *b1_dev, void *dst1_dev);
/* crdt_seg_gather2 for 4-byte elements over the first *n_dev (device
 * memory, <= n_max) of n_max segments, base 0: the count stays on the device
 * (segments past it scan as empty, dst_off[i] = the total for i >= *n_dev),
 * so a caller needs no host round trip between the merge that wrote the
 * count and this gather (the gossip round's next-Diff kv pairs). */
int crdt_seg_gather2_n(crdt_ctx *ctx, size_t n_max, const uint64_t *n_dev, const int64_t *code_dev,
                       const uint64_t *a_off_dev, const uint64_t *b_off_dev, uint64_t *dst_off_dev,
                       const uint32_t *a0_dev, const uint32_t *b0_dev, uint32_t *dst0_dev, const uint32_t *a1_dev,
                       const uint32_t *b1_dev, uint32_t *dst1_dev);
/* dst[dst_off[s] .. dst_off[s+1]) = val[s] */
int crdt_seg_fill_u32(crdt_ctx *ctx, size_t n_seg, const uint64_t *dst_off_dev, const uint32_t *val_dev,
                      uint32_t *dst_dev);
/* off[i] = base + sum(counts[0..i)), off[n] = base + total; and back. */
int crdt_counts_to_offsets(crdt_ctx *ctx, const uint32_t *counts_dev, size_t n, uint64_t base, uint64_t *off_dev);
int crdt_offsets_to_counts(crdt_ctx *ctx, const uint64_t *off_dev, size_t n, uint32_t *counts_dev);

/* ------------------------------------------------ gossip wire codec (§8(f) row 2)
 * Gossip handler (main.go:153-170): *http_status = 502 ("Unreachable")
 * unless Alive, else 200 with server.Diff.ToJSON() (main.go:159): gods
 * treemap ToJSON -> json.Marshal of {FormatInt(ts): value}, keys sorted as
 * byte strings, Go 1.18 encoding/json escaping.  The body goes to buf when
 * cap allows (else CRDT_E_RANGE, *len = size needed). */
int crdt_server_gossip_json(crdt_server *srv, char *buf, size_t cap, size_t *len, int *http_status);
/* Gossip pull decode (main.go:245-256): json.Unmarshal into
 * map[string]map[string]string, then RemoteDiff.Put(int64(Atoi(key)), value).
 * *outcome: 0 ingested (call merge next, main.go:257); 1 invalid JSON or shape,
 * round skipped (main.go:247-249); 2 a key failed Atoi, the reference's
 * gossip goroutine returns (main.go:252-253), nothing ingested. */
int crdt_server_ingest_json(crdt_server *srv, const char *data, size_t len, int *outcome);
/* Binary SoA form of the same Diff (§8(f) row 2: keep JSON for
 * compatibility, add a binary codec): "CRDTSOA1", u64 n_entries, n_pairs,
 * n_bytes, i64 ts[], u32 pairs[], u32 klen[], u32 vlen[], bytes (little
 * endian).  Ingest: *outcome 0 = put into RemoteDiff, 1 = malformed. */
int crdt_server_gossip_binary(crdt_server *srv, char *buf, size_t cap, size_t *len, int *http_status);
int crdt_server_ingest_binary(crdt_server *srv, const char *data, size_t len, int *outcome);
/* Device string tables (string -> dense id in first-seen order, bytes in an
 * append-only arena; str_off[n] = bytes used): the key dictionary and the
 * value arena the device gossip decode interns into.  A table belongs to one
 * device; calls that add strings synchronise and refresh a host mirror
 * (crdt_strtab_get). */
/* (crdt_strtab: declared with crdt_population above) */
int crdt_strtab_create(crdt_ctx *ctx, size_t cap_strings, size_t cap_bytes, crdt_strtab **out);
int crdt_strtab_destroy(crdt_strtab *tab);
/* counts and the device arena (bytes_dev / off_dev nullable): off_dev[0..n_str]
 * is the crdt_refmerge_in str_off of the table's strings. */
int crdt_strtab_info(const crdt_strtab *tab, uint64_t *n_str, uint64_t *n_bytes, const uint8_t **bytes_dev,
                     const uint64_t **off_dev);
int crdt_strtab_get(const crdt_strtab *tab, uint64_t id, const char **p, size_t *len);
/* Intern the n strings [off_host[i], off_host[i+1]) of a device byte arena:
 * ids_dev[i] = the string's id (new strings appended).  Synchronises. */
int crdt_strtab_intern(crdt_ctx *ctx, crdt_strtab *tab, const uint8_t *bytes_dev, const uint64_t *off_host, size_t n,
                       uint32_t *ids_dev);

/* Gossip pull decoded on the device (§8(f) row 2; main.go:245-256): binary SoA
 * bodies (crdt_server_gossip_binary) concatenated in HBM become the
 * crdt_refmerge_in R arrays of one replica each: r_off (0-based entry ranges
 * per body), r_ts, r_kv (= kv_base + pair offsets), and at
 * [kv_base, kv_base + pairs) the kv arena's key slots (slot_base[b] + the
 * key's id in `keys`) and value string ids (ids in `vals`: the merge's string
 * arena is that table's).  body_status[b] (host): 0 decoded; 1 malformed
 * (nothing of it is usable, as crdt_server_ingest_binary's outcome 1); 2 valid
 * but not taken by the device path (a nil map, ts not strictly ascending,
 * keys of an entry not strictly ascending, a key id >= key_cap): decode that
 * body on the host; 4 a table was full.  The decoded arrays of a non-zero
 * body are not valid.  Synchronises once (once more for the headers when
 * host_hdr is NULL, and once more when new strings were interned). */
typedef struct crdt_gossip_bodies {
    uint32_t n_bodies;
    uint32_t key_cap;           /* key ids >= key_cap: status 2 (the replica's slot range is full) */
    uint64_t kv_base;           /* first kv-arena index of the decoded pairs */
    const uint8_t *data;        /* device: the bodies, concatenated */
    const uint64_t *body_off;   /* host [n_bodies+1]: byte ranges of the bodies in data */
    const uint32_t *slot_base;  /* host [n_bodies]: key slot of key id 0, per body */
    const uint8_t *host_hdr;    /* host [32*n_bodies] or NULL: each body's first 32 bytes, when the caller
                                   already holds them (skips the header gather and its wait) */
} crdt_gossip_bodies;
typedef struct crdt_gossip_decoded {
    uint64_t *r_off;            /* device [n_bodies+1] */
    int64_t  *r_ts;             /* device [entries] */
    uint64_t *r_kv;             /* device [entries+1] */
    uint32_t *kv_key;           /* device, written at [kv_base, kv_base + pairs) */
    uint32_t *kv_val;
} crdt_gossip_decoded;
int crdt_gossip_decode(crdt_ctx *ctx, const crdt_gossip_bodies *in, crdt_strtab *keys, crdt_strtab *vals,
                       const crdt_gossip_decoded *out, uint32_t *body_status);

/* AliveState handler (main.go:141-151), after strconv.ParseBool. */
int crdt_server_set_alive(crdt_server *srv, int alive);
/* Ascending RemoteDiff keys; writes min(cap, len). */
int crdt_server_remote_keys(crdt_server *srv, int64_t *ts, size_t cap, size_t *n);
/* treemap Get(ts) on Diff (remote = 0) / RemoteDiff (remote = 1): CRDT_E_RANGE
 * if absent; else *npairs and, when i < *npairs, the i-th (key, value) pair. */
int crdt_server_entry_at(crdt_server *srv, int remote, int64_t ts, size_t i, const char **key,
                         size_t *key_len, const char **val, size_t *val_len, size_t *npairs);

#ifdef __cplusplus
}
#endif
#endif /* CRDT_AMD_H */
