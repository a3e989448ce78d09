/*
 * knn.h -- C ABI of libknn, the MI355X-native all-kNN engine.
 *
 * Drop-in boundary for the hot path of yiapou13/mpi-knn (snapshot
 * 2025-02-12).  The reference has no library API: its boundary is the
 * MATLAB MAT-API it consumes, the stage structure inside main() and the
 * CLI/stdout contract.  Each entry point below names the
 * reference lines it replaces.  Citations: serial:L = knn-serial.c,
 * blk:L = mpi-knn-parallel_blocking.c, nb:L = mpi-knn-parallel_non_blocking.c.
 *
 * Conventions
 *  - Every function returns an int status (KNN_OK == 0); nothing aborts and
 *    no C++ exception crosses the ABI.  knn_strerror() names a status.
 *  - Outputs are caller-owned.  The library owns device buffers it allocates.
 *  - "stream" arguments are hipStream_t passed as void* (NULL = default).
 *  - A context is used from one host thread at a time (not re-entrant).
 *  - Results follow the reference's SERIAL semantics (serial:72-93) for every
 *    device count: per query the k smallest distances sqrt(S), S = sum_j
 *    (x_qj - x_ij)^2 accumulated in j order in fp64 without FMA; exact
 *    zero distances (the point itself and exact duplicates) excluded; ties
 *    ordered by lower 1-based index; missing slots {INFINITY, 0, 0}.
 *
 * Environment switches read by the library (none changes a result; each
 * selects among exact code paths, for tests and diagnosis):
 *   KNN_NO_I8=1 / KNN_NO_H16=1 / KNN_NO_SHADOW=1 / KNN_NO_SPLIT=1
 *                         disable the int8 / fp16 contraction / fp16 shadow
 *                         rows / split fp16 filter (the next exact
 *                         contraction in line runs)
 *   KNN_I8_KL=17          17-entry int8 lane lists instead of 12
 *   KNN_SPLITS=s          corpus splits per launch instead of the model's
 *   KNN_ORDER=1 / KNN_NO_ORDER=1
 *                         GEMM-mode merge in the clustered query order
 *                         (default past 64 MB blocks) / always index order
 *   KNN_I8_QG1=1          one query group a wave on rows of <= 128 bytes
 *                         (the half-tile kernel otherwise carries two: 256
 *                         queries a workgroup sharing each staged row)
 *   KNN_FORCE_RESCAN=1    send every query through the exact rescan pass
 *   KNN_NO_RESEARCH8=1    no int8 re-search (65-entry lists) of uncertified
 *                         queries of a single-block search before the rescan
 *   KNN_FORCE_RING=1      knn_search runs the ring driver on one GPU
 *   KNN_RING_SCHEDULE=ring|direct
 *                         ring driver schedule: "ring" = the reference's
 *                         neighbour rotation (blk:187-244), "direct" = every
 *                         block to every rank at once (default; bit-identical
 *                         results, tested through the loopback transport and
 *                         gloo -- no multi-GPU node has run it yet)
 *   KNN_RING_FUSE=rest|all direct schedule: own block folded beside the
 *                         exchange (rest) or with the received blocks (all)
 *   KNN_RING_TIMEOUT_S=t  bound (seconds, default 300) on every wait for the
 *                         ring's transfers: RCCL asynchronous errors are
 *                         polled beside it, and a failed or stalled transfer
 *                         aborts the communicators and returns KNN_ERR_RCCL
 *                         (mpiknn/ring.py: RingError; bench.py: the process
 *                         group's timeout)
 *   KNN_RING_LOOPBACK=1   P virtual ranks on device 0 (tests)
 *   KNN_NO_SHADOW_RING=1  ring moves element blocks, not shadow/byte blocks
 *   KNN_XCD_ORDER=1 / 0   distance launches in the XCD-grouped / the
 *                         split-major workgroup order (unset: XCD-grouped
 *                         for split-filter launches of <= 2 splits)
 *   KNN_QUERY_BLOCK=rows  knn_query and knn_index_create fold / pack the corpus
 *                         in blocks of this many rows instead of the capacity
 *                         they choose
 *   KNN_QUERY_TILE=rows   knn_query and knn_index_query search the queries in
 *                         tiles of this many rows instead of all at once (up
 *                         to 2^18)
 *   KNN_MAT / KNN_MPI_COMPAT  the CLIs: .mat path, bug-compatible mode
 *   (mpiknn/ring.py: KNN_NO_S8=1 packs element blocks, not the byte block
 *   of knn_block_pack_s8)
 */
#ifndef KNN_H
#define KNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Only the entry points below are exported (libknn builds with
 * -fvisibility=hidden). */
#ifndef KNN_API
#define KNN_API __attribute__((visibility("default")))
#endif

/* blk:15-20 {double distance; int idx; int label;}.  serial:14-18 has the
 * same size and offsets for {distance, idx}. */
typedef struct {
    double  distance;
    int32_t idx;     /* 1-based global row (serial:89, blk:175), 0 = empty */
    int32_t label;   /* class label of that row (blk:176), 0 if unknown    */
} knn_neighbour_t;

enum knn_status {
    KNN_OK = 0,
    KNN_ERR_INVALID = 1,     /* bad argument / shape                      */
    KNN_ERR_NOMEM = 2,       /* host or device allocation failed          */
    KNN_ERR_HIP = 3,         /* HIP runtime error                         */
    KNN_ERR_IO = 4,          /* file could not be opened / read           */
    KNN_ERR_FORMAT = 5,      /* not a MAT-v5/v7 file, or variable missing */
    KNN_ERR_UNSUPPORTED = 6, /* valid request this build does not serve   */
    KNN_ERR_NODEVICE = 7,    /* no usable MI355X (gfx950) device          */
    KNN_ERR_RCCL = 8         /* RCCL ring error                           */
};

enum knn_layout { KNN_COLMAJOR = 0, KNN_ROWMAJOR = 1 };
/* KNN_U8: unsigned 8-bit elements.  A SOURCE type only (src_dtype of
 * knn_block_pack_dt / knn_block_pack_s8, and of the knn_index_* calls): no
 * block, context or search has it as its dtype. */
enum knn_dtype  { KNN_F64 = 0, KNN_F32 = 1, KNN_U8 = 2 };
enum knn_vote   { KNN_VOTE_SERIAL = 0, KNN_VOTE_MPI = 1, KNN_VOTE_MAJORITY = 2 };
/* what a neighbour counts in knn_classify_weighted / knn_regress and the
 * knn_index_* calls on top of them: one ballot, or 1 / distance */
enum knn_weights { KNN_WEIGHT_UNIFORM = 0, KNN_WEIGHT_DISTANCE = 1 };

/* Largest k served: KNN_F64 32 (the reference fixes NN = 30, serial:8 /
 * blk:9); KNN_F32 128 (BASELINE configs[4]: k = 100). */
#define KNN_MAX_K 32
#define KNN_MAX_K_F32 128

KNN_API const char *knn_strerror(int status);

/* ---------------------------------------------------------------------- *
 * Ingest -- replaces matOpen / matGetVariable / mxGetM / mxGetN / mxGetPr /
 * mxDestroyArray / matClose (serial:38-52, 100-109; blk:63-68, 72-79, 113-116;
 * nb:73-78, 82-89, 123-126).  Reads MAT-v5 (uncompressed) and v7 (zlib
 * miCOMPRESSED) files; any real numeric class is converted to double.
 * *X is column-major m x n (like mxGetPr of train_X), *labels has the
 * numel of lvar (m x 1).  lvar may be NULL.  Free both with knn_free().
 * ---------------------------------------------------------------------- */
KNN_API int  knn_load_mat(const char *path, const char *xvar, const char *lvar,
                  double **X, size_t *m, size_t *n, double **labels, size_t *nlabels);
KNN_API void knn_free(void *p);

/* ---------------------------------------------------------------------- *
 * Element type of the search (dtype):
 *   KNN_F64  the reference's arithmetic (results as described above).
 *   KNN_F32  the points are rounded to fp32 and filtered with fp32 MFMA
 *            (v_mfma_f32_16x16x4f32, 2x the fp64 rate).  Results are the
 *            exact k nearest neighbours OF THE fp32-ROUNDED POINTS under the
 *            reference's semantics: candidates are re-ranked by the
 *            reference-order fp64 sum S over the rounded values, certified,
 *            and rescanned when uncertified, exactly like the fp64 GEMM mode.
 *            Integer data with n*max|x|^2 <= 2^23 and n*(max-min)^2 <= 2^24
 *            (e.g. 8-bit pixels at n <= 128) is exact in fp32 arithmetic:
 *            identical to KNN_F64.  Otherwise the only deviation from the
 *            fp64 reference is the input rounding: |x - fp32(x)| <=
 *            2^-24 |x| per coordinate, so each reported distance is within
 *            2^-24 * (|q| + |c|) of the reference's (tests/test_gpu_f32.py).
 * ---------------------------------------------------------------------- */

/* ---------------------------------------------------------------------- *
 * One-call search on host arrays -- replaces the search section of
 * serial:54-93 and the whole ring of blk:81-244 / nb:91-259.
 * X: m x n fp64 in `layout`; labels (nullable, m doubles) fill .label;
 * ngpus >= 1 GPUs of this node (the corpus rotates over an RCCL ring when
 * ngpus > 1; results are byte-identical for every ngpus); dtype KNN_F64 or
 * KNN_F32 (above).  out: caller-owned m*k records.
 * ---------------------------------------------------------------------- */
KNN_API int knn_search(const double *X, size_t m, size_t n, int layout,
               const double *labels, int k, int ngpus, int dtype,
               knn_neighbour_t *out);

/* Bug-compatible mode (opt-in): the lists mpi-knn-parallel_
 * blocking.c / _non_blocking.c with `procs` ranks actually compute.  Rank
 * r keeps R = floor(m/procs) rows (the rest dropped, blk:81), folds its own
 * block, then the blocks of ranks r-2, r-3, ..., r-procs (= r again), each
 * truncated by the short first hop (blk:130-146: last ~2R/(n+2) rows zero)
 * and carrying idx 0 / label 0 (blk:169,231); block r-1 is never seen.
 * Ties keep scan order (blk:24-31).  fp64, k <= KNN_MAX_K, procs >= 2; the
 * ranks run one after another on device 0.  out: procs*R*k records, rank r
 * at out + r*R*k.  labels (nullable) fill .label of own-block records. */
KNN_API int knn_search_mpi_compat(const double *X, size_t m, size_t n, int layout,
                                  const double *labels, int k, int procs,
                                  knn_neighbour_t *out);

/* ---------------------------------------------------------------------- *
 * Out-of-sample queries -- the fold of blk:217-242 (a rank's own block
 * against the blocks it receives) with a query block that is no part of the
 * corpus: for every row of Q (mq x n, same layout as X) the k nearest of the
 * m corpus rows of X, on one GPU (several GPUs: the device-resident API
 * below, each rank a slice of Q or of X, as the ring does).  out: mq*k
 * records, idx the 1-based CORPUS row, label from labels[idx - 1] when labels
 * (nullable, m doubles) is given.  Semantics, order, arithmetic and empty
 * slots as knn_search; dtype as knn_search.
 *
 * flags = 0 keeps the reference's zero rule (blk:217-242 admits a distance
 * only if it is not 0: a corpus row equal to the query is left out, as
 * every exact duplicate is in knn_search).  KNN_QUERY_KEEP_ZERO makes S == 0
 * an ordinary result: distance 0.0, ordered by lower idx among equals -- a
 * test point identical to a training point gets that point as its nearest
 * neighbour.  Nothing else changes.
 *
 * The queries take the ids m .. m+mq-1 inside the engine (no query id equals
 * a corpus id; m + mq <= INT32_MAX).  The corpus is folded in blocks of a
 * capacity the call chooses (KNN_QUERY_BLOCK overrides it), the meta is the
 * MAX-reduction over every corpus block and the queries, and the int8 / fp16
 * / split-filter paths are taken when that meta allows, with the int8
 * re-search and the exact rescan behind them -- the same exact results on
 * every path.  Query sets too large for one context are tiled
 * (KNN_QUERY_TILE sets the tile); every tile's records stay on the device
 * until the last is done, so the reported span holds no copy to the host.
 * KNN_ERR_INVALID: NULL X, Q or out, zero m, mq or n, k <= 0, a bad layout,
 * unknown flag bits; KNN_ERR_UNSUPPORTED: an unknown dtype, k above the
 * dtype's limit -- all before any device call.
 * knn_last_search_seconds() reports its device span as for knn_search.
 * ---------------------------------------------------------------------- */
#define KNN_QUERY_KEEP_ZERO 1   /* flags bit; 0 = the reference's rule (zeros excluded, blk:217-242) */
KNN_API int knn_query(const double *X, size_t m, const double *Q, size_t mq, size_t n, int layout,
                      const double *labels, int k, int dtype, int flags, knn_neighbour_t *out);

/* ---------------------------------------------------------------------- *
 * Resident corpus index -- knn_query split where a server needs it split:
 * the corpus is uploaded, packed and reduced ONCE (knn_index_create) and
 * stays on the device; each knn_index_query then costs its own queries only
 * (blk:217-242 with the received blocks already in place).
 *
 * knn_index_create: X is m x n in `layout`, of src_dtype KNN_F64, KNN_F32 or
 * KNN_U8, uploaded in that type (no widening on the host; with
 * KNN_INDEX_DEVICE_SRC X is a device pointer on device 0 and is read in
 * place).  The index holds the element blocks of `dtype` (KNN_F64 / KNN_F32,
 * as knn_search; capacity as knn_query chooses it, KNN_QUERY_BLOCK overrides),
 * the byte blocks too when the corpus's own reduced meta passes
 * knn_s8_spec_ok, the host copy of that meta and a copy of labels (nullable,
 * m doubles).  The uploaded source is freed before the call returns: the
 * caller may free or overwrite X.
 *
 * knn_index_query: knn_query's sequence for one batch against the resident
 * blocks -- pack the query tiles (Q: mq x n in `layout`, of src_dtype, its
 * own; KNN_QUERY_TILE and the 2^18 limit as in knn_query), MAX-reduce their
 * meta with the stored corpus meta, take the byte path when the index has
 * byte blocks and the reduced meta passes knn_s8_spec_ok (else the element
 * path), then per tile begin, fold, end, int8 re-search, exact rescan.  out:
 * mq*k records, exactly those of knn_query(X, Q, ...) on the same values on
 * every path; queries take the ids m.. as there; .label from the index's
 * labels (0 without).  flags: KNN_QUERY_KEEP_ZERO as in knn_query;
 * KNN_INDEX_DEVICE_SRC: Q is a device pointer; KNN_INDEX_DEVICE_OUT: out is
 * a device pointer, written by the search itself (.label stays 0:
 * knn_classify_device fills it).  The context and the query-tile buffers are
 * kept between calls and recreated only when k changes or a batch needs more
 * tile capacity than is allocated (capacity grows geometrically from 128
 * rows); no result depends on the calls before it.
 * knn_last_search_seconds() reports the call's device span, query pack
 * through the last tile's records -- no corpus work, because none is done.
 *
 * knn_index_info (every output nullable): the shape, the number of resident
 * corpus blocks, the device bytes the index holds (element blocks, byte
 * blocks, tile buffers, records, and the context's buffers as an estimate
 * restated from their sizes) and knn_ctx_contraction_bits of
 * the last query (8, 16, 32 or 64; 0 before the first).
 *
 * knn_index_add: rows that arrive later (blk:100-109's pack, without
 * repacking what is resident).  X is rows x n in `layout`, of src_dtype, its
 * own (KNN_INDEX_DEVICE_SRC: a device pointer); the rows take the 1-based ids
 * last_id+1 .. last_id+rows (knn_index_last_id: m while nothing was removed),
 * m grows, and later queries take their ids from the new m.
 * The source is uploaded in its own type and packed into the last block's free
 * rows (knn_block_append_dt), then into new blocks of the index's capacity;
 * the touched blocks' meta is MAX-reduced into the corpus meta; an index with
 * byte blocks appends the same rows to them straight from the source
 * (knn_block_append_s8) as long as the corpus meta still passes
 * knn_s8_spec_ok.  When it no longer does -- a row outside [0, 255] or not an
 * integer was added -- the byte blocks are freed and never come back: queries
 * take the element path from then on, exact as ever, and an index created
 * without byte blocks never gains them.  labels: rows doubles when the index
 * holds labels, NULL when it holds none.  Every block keeps one capacity.
 * With KNN_QUERY_BLOCK set it is fixed; otherwise, when the add would leave
 * more than 8 blocks (one fused byte launch) and the capacity is below
 * knn_query's choice for n, the index is first re-blocked: the capacity
 * doubles until at most 8 blocks remain (or that limit is reached), the rows
 * and norms move device to device, the byte blocks are converted again from
 * the element blocks, and the kept context and tile buffers are dropped (the
 * next query recreates them) -- moved bytes stay O(rows added) amortised.
 * The caller may free or overwrite X when the call returns.  If the call
 * fails after its argument checks, the index answers queries as before it.
 * KNN_ERR_INVALID: NULL index or X, rows == 0, a bad layout, unknown flag bits,
 * last_id + rows > INT32_MAX, labels where the index has none or none where it
 * has; KNN_ERR_UNSUPPORTED: an unknown src_dtype -- before any device call.
 *
 * knn_index_remove: forget rows, by id.  A row keeps for its whole life the
 * 1-based id it got at creation or at its add; ids are never reused
 * (knn_index_last_id: the highest id handed out so far), and results keep
 * reporting them.  ids: `count` ids on the host, each in [1, last_id], in any
 * order; ids that are no longer live and repeats inside the list are skipped,
 * *removed (nullable) gets the number of rows actually removed, and a call that
 * removes nothing returns KNN_OK.  flags must be 0.  The survivors keep their
 * order (a stable compaction on the device), so their positions in the blocks
 * stay monotone in their ids and equal distances still come lower id first.
 * Blocks in front of the first removed row are not touched; every block from
 * there on is built again in a fresh buffer by knn_block_gather_dt (and
 * knn_block_gather_s8 where the index has byte blocks), its meta the max of
 * the blocks it drew from; old and new buffers of those blocks are resident
 * together until the call's one wait.  When only the last rows go, nothing is
 * moved.  The capacity stays (so do the kept context and tile buffers); blocks
 * past the new count are freed; a later add fills the last block's free rows.
 * The corpus meta is left as it is: it is a MAX-reduction, so a value that
 * has only become too large is conservative -- it can cost a faster path or a
 * rescan, never exactness.  In particular byte blocks that an add dropped do
 * not come back through a removal.  From the first removal on the index keeps
 * the live ids, ascending, on the host and on the device (counted in
 * knn_index_info's device_bytes), and knn_index_query ends its span with one
 * small kernel that turns each record's position into its id (host and
 * KNN_INDEX_DEVICE_OUT calls alike; empty slots stay {INFINITY, 0, 0}); an
 * index that never removed holds no such map and launches what it always
 * launched.  Labels stay indexed by id (a knn_classify_device caller's
 * d_labels by id stays valid); knn_index_info's m is the number of live rows.
 * If the call fails after its argument checks, the index answers as before it.
 * KNN_ERR_INVALID, before any device call and with nothing changed: NULL index
 * or ids, count == 0, flags != 0, an id outside [1, last_id], a call that
 * would leave no live row.
 *
 * knn_index_update: give rows new coordinates, by id, in place.  X is count x
 * n in `layout`, of src_dtype (fp64, fp32 or KNN_U8; KNN_INDEX_DEVICE_SRC: a
 * device pointer -- no other flag), and its row i becomes the row with id
 * ids[i] (`count` ids on the host, in any order).  Ids, last_id, m, the number
 * of blocks, the capacity and every row's position stay, so equal distances
 * still come lower id first, and so do the kept context and tile buffers; a
 * caller's tables by id (d_labels of knn_classify_device) stay valid, which a
 * remove + add of the same rows cannot offer: that pair hands out new ids and
 * rebuilds every block from the first removed row on.  Here the ids are mapped
 * to positions and grouped by block on the host (knn_update_plan.h), source
 * and lists are uploaded, and each touched block takes one
 * knn_block_scatter_dt: the moved bytes are the updated rows' own.  The touched
 * blocks' meta is MAX-reduced into the corpus meta, which therefore only grows
 * -- conservative, as after a removal: it can cost a faster path or a rescan,
 * never exactness.  An index with byte blocks scatters the same rows into them
 * straight from the source (knn_block_scatter_s8) while the corpus meta still
 * passes knn_s8_spec_ok; when it no longer does the byte blocks are freed as
 * in knn_index_add and never come back.  labels: count doubles that replace
 * the labels of those ids, or NULL to leave the labels as they are.  The caller
 * may free or overwrite X when the call returns.  A failure before the first
 * overwritten row (every allocation and upload comes before it) leaves the
 * index answering as before; a HIP error after it returns KNN_ERR_HIP and the
 * index is then fit only for knn_index_destroy -- rows are written in place,
 * so there is no older state to go back to.  Unlike knn_index_remove, ids that
 * are no longer live and repeats are refused, not skipped: a silently dropped
 * update is data loss.  KNN_ERR_INVALID, before any device call and with
 * nothing changed: NULL index, ids or X, count == 0, a bad layout, unknown flag
 * bits, an id outside [1, last_id], an id that is no longer live, an id twice
 * in the list, labels where the index has none; KNN_ERR_UNSUPPORTED: an unknown
 * src_dtype.
 *
 * knn_index_neighbours: the neighbours of resident rows, by id -- knn_search's
 * all-kNN (serial:72-93) over the corpus the index holds, after any add,
 * remove or update, with no host copy of the rows and nothing uploaded but the
 * ids.  For each listed live id the k nearest OTHER live rows; out holds
 * count*k records, row i those of ids[i].  Ids come in any order and may
 * repeat (the call only reads: a repeated id gets the same records twice).
 * ids == NULL (count must then be 0) means every live row in ascending id, m*k
 * records: the corpus's kNN graph.  idx is the neighbour's id, as in
 * knn_index_query after a removal; .label from the index's labels on host-out
 * calls; semantics, ordering, arithmetic and empty slots are knn_search's.
 * flags: 0 drops every zero distance -- the row itself and its exact
 * duplicates, the reference's leave-one-out rule as in knn_search;
 * KNN_QUERY_KEEP_ZERO leaves out only the row itself, and exact duplicates
 * come back at distance 0.0, lower id first (what knn_ctx_set_keep_zero
 * documents for in-corpus ids); KNN_INDEX_DEVICE_OUT as in knn_index_query.
 * There is no KNN_INDEX_DEVICE_SRC: there is no source.  How: ids are mapped to
 * positions on the host (knn_neighbours_plan.h), the query tiles are filled
 * from the resident blocks device to device (knn_block_gather_pos_dt, and
 * knn_block_gather_pos_s8 when the index has byte blocks and its meta passes
 * knn_s8_spec_ok), the batch's reduced meta is the corpus meta itself, and each
 * tile is searched as in knn_index_query, with ids past the corpus.  Under
 * flags 0 a row's own distance is exactly 0 on every path and the rule drops
 * it.  Under KNN_QUERY_KEEP_ZERO the engine searches k + 1 and one kernel takes
 * the row itself out of its records (and writes the ids): records are ordered
 * by (distance, id) and the row sits at distance 0, so if it is among the k + 1
 * the rest are the k nearest others, and if it is not, all k + 1 are duplicates
 * with lower ids and the first k are the answer.  So under KNN_QUERY_KEEP_ZERO
 * k + 1 must be within the dtype's limit: k = 32 on KNN_F64 and k = 128 on
 * KNN_F32 are KNN_ERR_UNSUPPORTED there (and served under flags 0).  The kept
 * context is keyed by the engine's k, which is k + 1 under KNN_QUERY_KEEP_ZERO:
 * a caller who alternates knn_index_query(k) and keep-zero neighbours(k)
 * recreates it each time.  knn_last_search_seconds() reports the span from the
 * gather through the last records.  A failed call leaves the index answering
 * as before (it drops the kept query state, as knn_index_query does).
 * KNN_ERR_INVALID, before any device call: NULL index or out, ids == NULL with
 * count != 0, ids != NULL with count == 0, k <= 0, unknown flag bits, an id
 * outside [1, last_id], an id that is no longer live (refused as in
 * knn_index_update, not skipped: a missing answer row would shift every later
 * one); KNN_ERR_UNSUPPORTED: k (k + 1 under KNN_QUERY_KEEP_ZERO) above the
 * dtype's limit.
 *
 * knn_index_classify: the vote (serial:104-130, blk:252-270) on the index's
 * own state -- knn_index_query's call for the batch, unchanged (paths, tiling,
 * KNN_QUERY_TILE, keep-zero rule, id remap after removals), then one vote
 * launch over the records while they are still on the device; nothing comes
 * back but the answers.  pred: mq predictions, exactly what
 * knn_classify_query returns for that call's records with the index's labels
 * by id (knn_index_last_id of them) as its table; vote_rule as there.
 * qlabels (nullable): the batch's own labels, mq doubles, always on the host;
 * *matches (nullable, always a host size_t): the q with pred[q] == qlabels[q],
 * 0 without qlabels.  counts (nullable): mq x nclasses ints, counts[q nclasses
 * + j] the number of query q's neighbours with label j + 1 -- the histogram
 * the vote ran on (divided by the number of non-empty slots: what other
 * libraries call predict_proba).  out (nullable): the mq*k records, .label
 * filled on host-out and device-out calls alike (the vote kernel writes it, as
 * knn_classify_device does).  flags: KNN_QUERY_KEEP_ZERO and
 * KNN_INDEX_DEVICE_SRC as in knn_index_query; KNN_INDEX_DEVICE_OUT makes pred,
 * counts and out device pointers on the index's device, and no copy back is
 * made.  The labels get a device copy, by id, at the index's first classify
 * call -- not in knn_index_create: an index that never classifies makes the
 * device calls it always made -- counted in knn_index_info's device_bytes from
 * then on; knn_index_add and knn_index_update with labels mark the ids they
 * wrote, and the next classify call uploads that range in front of its span;
 * knn_index_remove changes nothing (labels stay indexed by id, and removed ids
 * never appear in records).  The vote's own buffers live for the call.
 * knn_last_search_seconds() keeps reporting the search span alone: the vote is
 * outside it, as serial:94-98 stops its timer in front of the vote.  Every
 * output is complete on return; a failed call leaves the index answering as
 * before, and has written none of its host outputs (pred, counts, out,
 * *matches); under KNN_INDEX_DEVICE_OUT the caller's device arrays may hold
 * what the vote wrote before the failure.
 *
 * knn_index_classify_rows: the same behind knn_index_neighbours -- ids, count,
 * ids == NULL, the keep-zero rule and its k + 1 limit as there; row i's own
 * label is the index's label of ids[i], and *matches counts the rows predicted
 * as their own label.  There is no source flag.  With ids == NULL, flags 0 and
 * no removal it is the reference's whole program on the resident corpus:
 * knn_search plus knn_classify.
 *
 * Both, before any device call: KNN_ERR_INVALID for a NULL index or pred, an
 * index made without labels, nclasses <= 0, an unknown vote_rule, unknown flag
 * bits and everything knn_index_query / knn_index_neighbours refuse (their
 * NULL out excepted); KNN_ERR_UNSUPPORTED for nclasses > KNN_VOTE_MAX_CLASSES
 * and for k above the limit (k + 1 under KNN_QUERY_KEEP_ZERO, for rows).
 *
 * knn_index_classify_weighted, knn_index_classify_weighted_rows,
 * knn_index_regress, knn_index_regress_rows: the index as a predictor.  They
 * are knn_index_classify / knn_index_classify_rows with another vote behind
 * the same search -- paths, tiling, KNN_QUERY_TILE, the keep-zero rule and its
 * k + 1 limit for rows, the id remap, the labels' device copy, the staging of
 * host outputs, both device flags, knn_last_search_seconds() all as there --
 * and that vote is knn_classify_weighted / knn_regress (below, where the
 * semantics are written down) of the call's records with the index's labels by
 * id, bit for bit.  weights: enum knn_weights.  Weighted classification: pred
 * (mq ints), sums (nullable, mq x nclasses doubles: sums[q nclasses + j] the
 * weight of class j + 1, the weighted counterpart of counts), *matches and
 * qlabels as in knn_index_classify; the records' .label is filled.
 * Regression reads the index's labels as real-valued targets: pred is mq
 * doubles, and the records' .label stays as the search left it (0), on host-out
 * calls too.  Under KNN_INDEX_DEVICE_OUT pred, sums and out are device
 * pointers.  All four, before any device call: what the classify pair refuses
 * (regression has no class checks), and KNN_ERR_INVALID for an unknown weights;
 * an index made without labels is KNN_ERR_INVALID here too.
 *
 * knn_index_radius_count, knn_index_radius, knn_index_radius_rows_count,
 * knn_index_radius_rows: radius search -- which live rows lie within distance
 * r of a point, and how many (scikit-learn's radius_neighbors, FAISS's
 * range_search); there is no k and no k limit.  For a query row q and radius
 * r a hit is a live corpus row x with sqrt(S) <= r, S = sum_j (q_j - x_j)^2
 * accumulated in j order in fp64 without FMA: knn_search's arithmetic, over
 * the fp32-rounded values on an index of dtype KNN_F32 as in knn_index_query.
 * The comparison is made on the reported distance, so no returned distance
 * exceeds r; NaN and infinite distances are no hits.  r: a finite double >= 0.
 * The zero rule is knn_index_query's: flags 0 -- a zero distance is no hit
 * (the reference's rule); KNN_QUERY_KEEP_ZERO -- a hit at distance 0.0.  The
 * _rows forms follow knn_index_neighbours: flags 0 drops the row itself and
 * its exact duplicates; KNN_QUERY_KEEP_ZERO leaves out only the row itself, by
 * position, and duplicates are hits at 0.0.  A query's hits come ordered by
 * (distance, id), lower id first on ties; idx is the row's id (the stable id
 * after removals, as in knn_index_query); .label is filled from the index's
 * labels on host-out calls and is 0 on device-out calls or without labels.
 *
 * Output is CSR, caller-owned, in two calls, so that nothing is sized by
 * guess: the _count call is the first distance pass and writes counts[q], the
 * number of hits of query q (mq int32), and nothing else.  The caller makes
 * indptr (mq + 1 int64), the exclusive prefix sum of those counts from any
 * offset indptr[0] >= 0, non-decreasing, and the fill call -- the second
 * distance pass and a per-query sort -- writes query q's hits to the records
 * indptr[q] - indptr[0] .. indptr[q + 1] - indptr[0] - 1 of out, which holds
 * indptr[mq] - indptr[0] records; it never writes outside a query's segment.
 * If any query's number of hits differs from its segment's length (the index
 * was changed between the two calls, or the arguments were) the fill call
 * returns KNN_ERR_INVALID and out's content is unspecified.  A segment of
 * length 0 is legal, and mq queries without a single hit are KNN_OK.
 * KNN_INDEX_DEVICE_SRC (query forms) as in knn_index_query;
 * KNN_INDEX_DEVICE_OUT makes counts, indptr and out device pointers on the
 * index's device, and nothing is copied back.  ids, ids == NULL (every live
 * row in ascending id), repeats and dead ids as in knn_index_neighbours;
 * KNN_QUERY_TILE and the 2^18 tile limit as in knn_index_query.  How: the
 * queries are packed (or gathered by position) into tile buffers the radius
 * calls keep for themselves -- no context is made, and the one
 * knn_index_query keeps is not touched -- and searched by distance kernels of
 * their own (knn_radius.hip): on the byte path (the index has byte blocks and
 * the batch's reduced meta passes knn_s8_spec_ok) an int8 MFMA kernel whose
 * exact integer d^2 is compared with the one integer T that has sqrt(T) <= r <
 * sqrt(T + 1); otherwise an exact scan in the reference's arithmetic.
 * knn_last_search_seconds() reports the call's device span, pack or gather
 * through the last kernel.  A failed call leaves the index answering as
 * before.  KNN_ERR_INVALID, before any device call: a NULL index, Q, counts,
 * indptr or out, mq == 0, a bad layout, unknown flag bits, a radius that is
 * negative, NaN or infinite, a host indptr that decreases or starts below 0,
 * m + mq > INT32_MAX, and the id errors of knn_index_neighbours;
 * KNN_ERR_UNSUPPORTED: an unknown src_dtype.
 *
 * knn_index_dbscan, knn_dbscan_graph: DBSCAN over the index's live rows (not
 * in the reference), exact on every path.  The definition, in one place: take
 * the m live rows at positions 0 .. m-1 in ascending id, eps a finite double
 * >= 0 and min_pts an int >= 1.
 *   Distance: d(x, y) = sqrt(S), S as in knn_index_radius* (the fp64 sum in j
 *     order without FMA, over the fp32-rounded values on a KNN_F32 index); y
 *     is a neighbour of x when d <= eps and d is finite.
 *   Neighbourhood size N(x): the number of live rows y with d(x, y) <= eps,
 *     x itself and its exact duplicates INCLUDED (scikit-learn's min_samples
 *     convention; there is no zero rule to choose).  N(x) =
 *     knn_index_radius_rows_count(ids = NULL, KNN_QUERY_KEEP_ZERO)[x] + 1.
 *   Core row: N(x) >= min_pts.
 *   Clusters: the connected components of the graph whose vertices are the
 *     core rows and whose edges join two core rows with d <= eps, numbered
 *     1 .. C in ascending order of each component's lowest position.
 *   Border row: not core, with at least one core neighbour.  It takes the
 *     cluster of its nearest core neighbour by (distance, id), lower id on
 *     equal distances -- the order of every other answer of this library: the
 *     first core row in the row's knn_index_radius_rows segment.
 *   Noise: every other row, cluster 0 (this library's "nothing", as idx 0 and
 *     pred 0; scikit-learn writes -1).
 * The result is a function of the data, eps and min_pts alone: it does not
 * depend on scheduling, block capacity, path or launch count.
 * knn_index_dbscan: cluster (m int32, by ascending live id), neighbours
 * (nullable, m int32: N(x)) and *nclusters (nullable, always host: C).  flags:
 * 0 or KNN_INDEX_DEVICE_OUT (cluster and neighbours are device pointers and
 * nothing is copied back but *nclusters).  How: two distance passes over the
 * square of the corpus and O(m) work around them; nothing has size m * n or
 * "number of pairs".  Each resident block, byte or element form, is the query
 * tile of its own rows (no gather, no second copy of the corpus); the count
 * pass gives N(x); the link pass, a third form of the two radius kernels,
 * consumes each hit where it is found: two core rows are united in a lock-free
 * union-find whose roots are lowest positions, a core row is offered to a row
 * that is not core, which keeps the minimum by (distance, position); then the
 * roots are ranked by a prefix sum and the clusters written.  Path and
 * threshold as in knn_index_radius_rows.  knn_last_search_seconds() reports
 * the device span, first kernel through last.  No context is made and the kept
 * one is not touched; nothing of the index changes but buffers it owns (counted
 * in knn_index_info's device_bytes); a failed call leaves the index answering
 * as before and has written none of its host outputs.  KNN_ERR_INVALID, before
 * any device call: a NULL index or cluster, min_pts < 1, an eps that is
 * negative, NaN or infinite, unknown flag bits.
 * knn_dbscan_graph: the same clustering on the host, without a device call,
 * from the CSR knn_index_radius_rows(ids = NULL, KNN_QUERY_KEEP_ZERO) returns
 * (indptr: m + 1 offsets, rec: indptr[m] - indptr[0] records, each segment by
 * (distance, id)); ids: the m live ids ascending (NULL: 1 .. m).  N(x) =
 * segment length + 1; a union-find over the records that join two core rows;
 * a border row takes the first core record of its segment.  KNN_ERR_INVALID,
 * with no output written: NULL indptr, rec (when there are records) or
 * cluster, m == 0, min_pts < 1, an indptr that decreases, a record whose idx
 * is no live id.
 *
 * KNN_ERR_INVALID: NULL index, X, Q or out, zero m, mq or n, k <= 0, a bad
 * layout, unknown flag bits, m + mq > INT32_MAX; KNN_ERR_UNSUPPORTED: an
 * unknown src_dtype, dtype not KNN_F64 / KNN_F32, k above the dtype's limit
 * -- all before any device call.  An index is used from one host thread at a
 * time.  (Integer corpora inside an 8-bit window but outside [0, 255] are not
 * knn_s8_spec_ok: the engine converts their element blocks to byte blocks
 * inside each search, as in knn_query -- exact, but per call.)
 * ---------------------------------------------------------------------- */
typedef struct knn_index knn_index_t;
#define KNN_INDEX_DEVICE_SRC 2   /* X / Q is a device pointer on the index's device        */
#define KNN_INDEX_DEVICE_OUT 4   /* out (classify, regress: pred, counts / sums too) is a device pointer */
KNN_API int knn_index_create(knn_index_t **index, const void *X, size_t m, size_t n, int layout,
                             int src_dtype, const double *labels, int dtype, int flags);
KNN_API int knn_index_query(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                            int k, int flags, knn_neighbour_t *out);
KNN_API int knn_index_add(knn_index_t *index, const void *X, size_t rows, int layout, int src_dtype,
                          const double *labels, int flags);
KNN_API int knn_index_remove(knn_index_t *index, const int32_t *ids, size_t count, int flags,
                             size_t *removed /* nullable */);
KNN_API int knn_index_update(knn_index_t *index, const int32_t *ids, size_t count, const void *X, int layout,
                             int src_dtype, const double *labels /* nullable */, int flags);
KNN_API int knn_index_neighbours(knn_index_t *index, const int32_t *ids /* nullable */, size_t count, int k,
                                 int flags, knn_neighbour_t *out);
KNN_API int knn_index_classify(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                               int k, int nclasses, int vote_rule, int flags,
                               const double *qlabels /* nullable, host, mq */,
                               int *pred, int *counts /* nullable, mq*nclasses */,
                               size_t *matches /* nullable */, knn_neighbour_t *out /* nullable, mq*k */);
KNN_API int knn_index_classify_rows(knn_index_t *index, const int32_t *ids /* nullable */, size_t count,
                                    int k, int nclasses, int vote_rule, int flags,
                                    int *pred, int *counts, size_t *matches, knn_neighbour_t *out);
KNN_API int knn_index_classify_weighted(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                                        int k, int nclasses, int weights, int flags,
                                        const double *qlabels /* nullable, host, mq */,
                                        int *pred, double *sums /* nullable, mq*nclasses */,
                                        size_t *matches /* nullable */, knn_neighbour_t *out /* nullable, mq*k */);
KNN_API int knn_index_classify_weighted_rows(knn_index_t *index, const int32_t *ids /* nullable */, size_t count,
                                             int k, int nclasses, int weights, int flags,
                                             int *pred, double *sums, size_t *matches, knn_neighbour_t *out);
KNN_API int knn_index_regress(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                              int k, int weights, int flags, double *pred, knn_neighbour_t *out /* nullable */);
KNN_API int knn_index_regress_rows(knn_index_t *index, const int32_t *ids /* nullable */, size_t count,
                                   int k, int weights, int flags, double *pred, knn_neighbour_t *out);
KNN_API int knn_index_radius_count(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                                   double radius, int flags, int32_t *counts /* mq */);
KNN_API int knn_index_radius(knn_index_t *index, const void *Q, size_t mq, int layout, int src_dtype,
                             double radius, int flags, const int64_t *indptr /* mq + 1 */,
                             knn_neighbour_t *out /* indptr[mq] - indptr[0] records */);
KNN_API int knn_index_radius_rows_count(knn_index_t *index, const int32_t *ids /* nullable */, size_t count,
                                        double radius, int flags, int32_t *counts);
KNN_API int knn_index_radius_rows(knn_index_t *index, const int32_t *ids /* nullable */, size_t count,
                                  double radius, int flags, const int64_t *indptr, knn_neighbour_t *out);
KNN_API int knn_index_dbscan(knn_index_t *index, double eps, int min_pts, int flags,
                             int32_t *cluster /* m, by ascending live id */,
                             int32_t *neighbours /* nullable, m: N(x) */,
                             int *nclusters /* nullable, always host */);
KNN_API int knn_dbscan_graph(const int64_t *indptr, const knn_neighbour_t *rec,
                             const int32_t *ids /* nullable: the m live ids ascending; NULL = 1..m */,
                             size_t m, int min_pts, int32_t *cluster, int32_t *neighbours /* nullable */,
                             int *nclusters /* nullable */);
KNN_API int knn_index_last_id(const knn_index_t *index, size_t *last_id);
KNN_API int knn_index_info(const knn_index_t *index, size_t *m, size_t *n, int *nblocks,
                           size_t *device_bytes, int *last_bits);
KNN_API int knn_index_destroy(knn_index_t *index);

/* Search wall time of the last knn_search() / knn_query() / knn_index_query() / knn_index_neighbours() /
 * knn_index_classify() / knn_index_classify_rows() / knn_index_radius*() on this thread, seconds: the
 * span the reference times (serial:70-98, blk:120-250) -- device compute
 * only, excluding load, H2D, D2H and vote. */
KNN_API double knn_last_search_seconds(void);

/* ---------------------------------------------------------------------- *
 * Vote + accuracy -- replaces serial:104-130 (rule SERIAL), blk:252-270 /
 * nb:269-288 (rule MPI); rule MAJORITY is a true majority (not in the
 * reference).  labels: per-row class labels (1..nclasses, as stored in the
 * .mat).  pred (nullable): m predicted labels.  *matches: rows whose
 * prediction equals their own label.  Empty slots (idx 0) are skipped where
 * the reference would read out of bounds.
 * ---------------------------------------------------------------------- */
KNN_API int knn_classify(const knn_neighbour_t *nb, size_t m, int k, int nclasses,
                 int vote_rule, const double *labels, int *pred, size_t *matches);
/* The same vote for knn_query's records: nb holds mq*k records whose idx are
 * corpus rows, labels the m corpus labels (idx 0 and idx > m are skipped as
 * empty), qlabels (nullable) the mq query labels.  pred (nullable): mq
 * predictions; *matches: queries whose prediction equals qlabels[q] (0 when
 * qlabels is NULL -- only pred is written then). */
KNN_API int knn_classify_query(const knn_neighbour_t *nb, size_t mq, int k, int nclasses, int vote_rule,
                               const double *labels, size_t m, const double *qlabels,
                               int *pred, size_t *matches);

/* ---------------------------------------------------------------------- *
 * The records as a predictor (not in the reference): the distance-weighted
 * vote and kNN regression, on the host.  nb: mq*k records as a search wrote
 * them (ascending distance, then id) whose idx index labels / targets by id,
 * as in knn_classify_query.  One definition, which the device vote of
 * knn_index_classify_weighted / knn_index_regress repeats bit for bit:
 *
 *   valid    record i counts when 1 <= idx <= nlabels; empty slots
 *            {INFINITY, 0, 0} and stray ids are skipped.
 *   weights  KNN_WEIGHT_UNIFORM: w_i = 1.0.  KNN_WEIGHT_DISTANCE: w_i =
 *            1.0 / distance_i, one correctly rounded fp64 division -- unless a
 *            valid record of the query has distance exactly 0.0: then every
 *            valid record at distance 0 gets w = 1.0 and every other one
 *            w = 0.0 (an exact match decides; scikit-learn's rule).
 *   classify lab_i = (int)labels[idx_i - 1] is counted when 1 <= lab_i <=
 *            nclasses.  sums[q nclasses + j]: the fp64 sum of w_i over the
 *            counted records of class j + 1, added in record order.  pred[q]:
 *            the class with the largest sum if that is > 0, ties to the tied
 *            class met first in record order (KNN_VOTE_MAJORITY's rule), 0
 *            when nothing was counted.  *matches: the q with pred[q] ==
 *            qlabels[q] (0 without qlabels).
 *   regress  y_i = targets[idx_i - 1] of every valid record, any double.
 *            pred[q] = (sum of w_i * y_i) / (sum of w_i): each product
 *            rounded on its own (no fused multiply-add), both sums fp64 in
 *            record order; NaN (the positive quiet one) without a valid record.
 *
 * pred, sums (mq x nclasses doubles) and matches of knn_classify_weighted
 * are nullable.  KNN_ERR_INVALID: NULL nb, labels or targets, k <= 0,
 * nclasses <= 0, an unknown weights, nlabels / ntargets == 0, a NULL pred of
 * knn_regress.  No device call.
 * ---------------------------------------------------------------------- */
KNN_API int knn_classify_weighted(const knn_neighbour_t *nb, size_t mq, int k, int nclasses, int weights,
                                  const double *labels, size_t nlabels, const double *qlabels /* nullable */,
                                  int *pred, double *sums, size_t *matches);
KNN_API int knn_regress(const knn_neighbour_t *nb, size_t mq, int k, int weights, const double *targets,
                        size_t ntargets, double *pred);

/* The same vote on the device, on the records knn_ctx_end / rescan_end
 * wrote (no host round trip).  d_nb: m*k records of queries with global ids
 * q_base..q_base+m-1, whose .label it fills (blk:176); d_labels: nlabels
 * row labels (global id i at d_labels[i-1]; ids > nlabels count as empty);
 * d_pred (nullable): m predictions; d_matches (nullable): one device
 * counter, set to the number of queries predicted as their own label.
 * nclasses <= KNN_VOTE_MAX_CLASSES (else KNN_ERR_UNSUPPORTED: use the host
 * knn_classify).  Out-of-sample queries need no other entry point: with
 * q_base = m and d_labels = the m corpus labels followed by the mq query
 * labels (nlabels = m + mq), query q's own label is d_labels[m + q] and its
 * neighbours' are corpus labels -- knn_classify_query's result on the
 * device. */
#define KNN_VOTE_MAX_CLASSES 1024
KNN_API int knn_classify_device(knn_neighbour_t *d_nb, size_t m, int k, int nclasses,
                        int vote_rule, const double *d_labels, size_t nlabels, size_t q_base,
                        int *d_pred, unsigned long long *d_matches, void *stream);

/* ---------------------------------------------------------------------- *
 * Device-resident API (the engine underneath knn_search; used by the
 * per-rank RCCL ring driver and by bench.py).  All pointers named d_* are
 * device pointers on the context's device.
 *
 * A "packed block" holds up to `cap` points (its capacity) laid out for
 * the kernels:
 *   [cap_pad x n_pad fp64 row-major, zero padded][cap_pad fp64 squared
 *   norms][KNN_META_DOUBLES fp64 meta], cap_pad = cap rounded up to 128,
 *   n_pad = n rounded up to 16.  One contiguous buffer, so a ring hop moves
 *   a block with one send (blk:195-212 moved R*(n+2) doubles).  Every block
 *   of one ring has the same capacity, hence the same byte size.
 * ---------------------------------------------------------------------- */
#define KNN_META_DOUBLES 8

KNN_API size_t knn_block_bytes(size_t cap, size_t n);
/* Offset (bytes) of the meta doubles inside a packed block.  The meta of
 * all blocks of one search must be MAX-reduced into the d_meta passed to
 * knn_ctx_begin (a one-shot all-reduce of 8 doubles across ranks). */
KNN_API size_t knn_block_meta_offset(size_t cap, size_t n);
/* The same for blocks of element type dtype (KNN_F64 blocks above; KNN_F32
 * blocks hold fp32 rows padded to 32 features and fp32 norms, then the
 * same 8 fp64 meta words).  0 for an unknown dtype. */
KNN_API size_t knn_block_bytes_dt(size_t cap, size_t n, int dtype);
KNN_API size_t knn_block_meta_offset_dt(size_t cap, size_t n, int dtype);

/* Ring wire form of a packed block: the elements as int16, norms and meta
 * verbatim -- a quarter (fp64) or half (fp32) of the block bytes on the
 * link.  Exact only when knn_wire_ok(host copy of the reduced meta): every
 * value an integer with max|x| <= 32767.  knn_wire_unpack restores the
 * block bit for bit.  Used by mpiknn/ring.py between RCCL hops. */
KNN_API size_t knn_wire_bytes(size_t cap, size_t n, int dtype);
KNN_API int knn_wire_ok(const double *h_meta);
KNN_API int knn_wire_pack(void *d_wire, const void *d_block, size_t cap, size_t n, int dtype,
                          void *stream);
KNN_API int knn_wire_unpack(void *d_block, const void *d_wire, size_t cap, size_t n, int dtype,
                            void *stream);

/* Shadow block of a packed block: its rows as fp16 (round_up(n, 64) halves
 * a row), norms and meta verbatim.  When knn_ctx_shadow(ctx) is 1 after
 * knn_ctx_begin (the fp16 contraction is exact for this search and staged
 * from shadow rows), knn_ctx_step_shadow folds a shadow block instead of
 * the element block -- the ring then moves shadow blocks (2 bytes an
 * element).  The exact rescan (knn_ctx_rescan_step) still takes element
 * blocks. */
KNN_API size_t knn_shadow_bytes(size_t cap, size_t n, int dtype);
KNN_API size_t knn_shadow_norm_offset(size_t cap, size_t n);
KNN_API int knn_shadow_pack(void *d_sblock, const void *d_block, size_t cap, size_t n, int dtype,
                            void *stream);

/* Split fp16 rows of a packed block (the split-fp16 filter's form of
 * real-valued data): for rows_pad(cap) rows, per 32 features the 32 halves
 * hi = RN16(scale x) then the 32 halves lo = RN16(scale x - hi), each
 * rounded once from the block's precision, zero past n; rows of round_up(n, 32) * 4 bytes (knn_split_bytes).
 * scale: a power of two.  The engine converts the blocks of a split-filter
 * search itself; this entry point exposes the same conversion for tests
 * and tools. */
KNN_API size_t knn_split_bytes(size_t cap, size_t n);
KNN_API int knn_split_pack(void *d_dst, const void *d_block, size_t cap, size_t n, int dtype, double scale,
                           void *stream);

/* Pack rows (<= cap) points from a device source.  layout KNN_COLMAJOR:
 * element (i, j) at d_src[i + j*ld] (ld >= rows; the .mat layout,
 * serial:82); KNN_ROWMAJOR: d_src[i*ld + j] (ld >= n; blk:81-109).
 * Computes norms and meta.  Replaces blk:100-109 / nb:110-119. */
KNN_API int knn_block_pack(void *d_block, size_t cap, size_t rows, size_t n, const double *d_src,
                   size_t ld, int layout, void *stream);
/* Pack into a block of element type dtype from a source of src_dtype
 * (fp64, fp32 or KNN_U8 device array, same layouts).  For the same values the
 * block from a KNN_U8 source is byte for byte the block from the fp64 one. */
KNN_API int knn_block_pack_dt(void *d_block, int dtype, size_t cap, size_t rows, size_t n,
                      const void *d_src, int src_dtype, size_t ld, int layout, void *stream);
/* Rows that arrive later: write block rows row0 .. row0+rows-1 of a block
 * packed before with the same cap, n and dtype, from a rows x n source
 * (layouts, ld and source types as knn_block_pack_dt) -- the rows, their
 * norms, and the meta atomicMax'ed into the words already there; nothing else
 * of the block is touched.  A block packed over its first rows and appended
 * to in any pieces is byte for byte the block one knn_block_pack_dt of all
 * the rows writes (a row's norm is summed in the same order wherever the row
 * lands).  Launches are sized by `rows`, not cap.  KNN_ERR_INVALID: row0 +
 * rows > cap, rows == 0, a NULL pointer, dtype or src_dtype as
 * knn_block_pack_dt. */
KNN_API int knn_block_append_dt(void *d_block, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                                const void *d_src, int src_dtype, size_t ld, int layout, void *stream);
/* Rows given new values in place: work item i < rows reads row d_srow[i] (a
 * NULL d_srow: row i) of the src_rows x n source and writes block row d_pos[i]
 * of a block packed before with the same cap, n and dtype (layouts, ld and
 * source types as knn_block_pack_dt; d_pos and d_srow are device int32 arrays
 * of `rows` entries).  Otherwise an append: only the listed rows, their norms
 * and the meta are touched -- no padding, no other row -- and launches are
 * sized by `rows`.  A block packed before and scattered into with distinct
 * positions is, outside its 8 meta doubles, byte for byte the block one
 * knn_block_pack_dt of the updated array writes (a row's norm is summed by the
 * same lanes in the same order wherever it lands and whichever source row it
 * comes from); its meta is, word by word, max(the meta before, the meta of a
 * pack of the listed source rows alone), word 7 as it was.  Repeated positions
 * leave one of their rows, unspecified which.  A d_pos[i] outside [0, cap)
 * writes nothing (the row's values may still reach the meta, which is
 * conservative); a d_srow[i] outside [0, src_rows) reads nothing and writes
 * nothing.  KNN_ERR_INVALID, before any device call: a NULL block, d_pos or
 * d_src, rows, n or src_rows zero, cap or src_rows above INT32_MAX, a bad
 * layout, ld below src_rows (column-major) or n (row-major), a dtype other
 * than KNN_F64 / KNN_F32, an unknown src_dtype. */
KNN_API int knn_block_scatter_dt(void *d_block, int dtype, size_t cap, const int32_t *d_pos,
                                 const int32_t *d_srow /* nullable */, size_t rows, size_t n, const void *d_src,
                                 size_t src_rows, int src_dtype, size_t ld, int layout, void *stream);
/* Rows from another block: block row row0 + i of d_dst becomes row d_list[i]
 * of d_src, i < rows.  Both are packed blocks of the given capacities with the
 * same n and dtype; d_list is a device array of local source rows, each below
 * src_cap, in any order and with repeats (a gather, not only a compaction).
 * The n_pad elements and the norm of each row are copied bit for bit; nothing
 * else of d_dst is touched -- not its other rows, not its padding, not its
 * meta, which stays the caller's business.  Launches are sized by `rows`.
 * KNN_ERR_INVALID, before any device call: a NULL pointer, rows == 0, row0 +
 * rows > dst_cap, d_dst == d_src, a capacity above INT32_MAX, an unknown dtype. */
KNN_API int knn_block_gather_dt(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                                const int32_t *d_list, size_t rows, size_t n, int dtype, void *stream);
/* Rows from a corpus held as several blocks: block row row0 + i of d_dst
 * becomes the row at global position d_pos[i], i < rows, of nblk packed blocks
 * of one capacity src_cap -- row d_pos[i] % src_cap of block d_pos[i] /
 * src_cap.  d_tab: the nblk block pointers, a device array; d_pos: device
 * int32 positions in any order, with repeats.  Otherwise knn_block_gather_dt:
 * rows and norms bit for bit, nothing else of d_dst touched, launches sized by
 * `rows`.  A position outside [0, nblk * src_cap) writes nothing.
 * KNN_ERR_INVALID as knn_block_gather_dt, and for a NULL d_tab or nblk == 0. */
KNN_API int knn_block_gather_pos_dt(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab,
                                    size_t src_cap, size_t nblk, const int32_t *d_pos, size_t rows, size_t n,
                                    int dtype, void *stream);

typedef struct knn_ctx knn_ctx_t;

/* nq queries of dimension n; corpus blocks are packed with capacity
 * block_cap (knn_block_pack's cap) and hold at most block_cap rows. */
KNN_API int knn_ctx_create(knn_ctx_t **ctx, int device, size_t nq, size_t n,
                   size_t block_cap, int k);
/* A context over blocks of element type dtype (knn_ctx_create: KNN_F64). */
KNN_API int knn_ctx_create_dt(knn_ctx_t **ctx, int device, size_t nq, size_t n,
                      size_t block_cap, int k, int dtype);
KNN_API int knn_ctx_destroy(knn_ctx_t *ctx);

/* Start: the queries are the first nq rows of packed block d_qblock
 * (capacity q_cap) with global ids q_base..q_base+nq-1; d_meta = the
 * max-reduced meta of every corpus block. */
KNN_API int knn_ctx_begin(knn_ctx_t *ctx, const void *d_qblock, size_t q_cap, size_t q_base,
                  const double *d_meta, void *stream);
/* The same with the host copy of the reduced meta (h_meta, 8 doubles; the
 * ring drivers hold it after their all-reduce), so begin does not read it
 * back from the device (no stream synchronisation).  h_meta NULL = begin. */
KNN_API int knn_ctx_begin_meta(knn_ctx_t *ctx, const void *d_qblock, size_t q_cap, size_t q_base,
                               const double *d_meta, const double *h_meta, void *stream);

/* Speculative byte block (the int8 contraction's form) straight from the
 * source -- the fast path for 8-bit integer data (MNIST pixels, SIFT
 * descriptors).  Writes knn_s8_block_bytes(cap, n) bytes: rows of x - 128 as
 * int8, the int8 kernel's norm words, and at knn_s8_block_meta_offset the
 * block's 8 meta doubles (the same values knn_block_pack_dt computes, and
 * word 7 = 1: after the MAX-reduction it says some block was packed this
 * way; reduce them across blocks as usual).  The bytes are the int8 path's rows exactly
 * when knn_s8_spec_ok(reduced meta) -- every value an integer in [0, 255]
 * and the search int8-eligible; then knn_ctx_begin_s8 starts the search from
 * it (no element block, no conversion; a ring moves it as the shadow block),
 * otherwise pack the element block (knn_block_pack_dt) and knn_ctx_begin_meta.
 * One read of the source, 1 byte written an element (replaces the pack of
 * blk:100-109 plus the element -> byte conversion).  src_dtype KNN_U8: the
 * bytes are x ^ 0x80, norms and meta in integer arithmetic -- byte for byte
 * the block packed from the fp64 array of the same values (1 byte read, 1
 * written an element). */
KNN_API size_t knn_s8_block_bytes(size_t cap, size_t n);
KNN_API size_t knn_s8_block_meta_offset(size_t cap, size_t n);
KNN_API int knn_block_pack_s8(void *d_sblock, int dtype, size_t cap, size_t rows, size_t n, const void *d_src,
                              int src_dtype, size_t ld, int layout, void *stream);
/* knn_block_append_dt for a byte block packed by knn_block_pack_s8: the byte
 * rows, both norm words of each row and the meta (word 7 stays 1); the same
 * byte-for-byte contract against one knn_block_pack_s8 of all the rows. */
KNN_API int knn_block_append_s8(void *d_sblock, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                                const void *d_src, int src_dtype, size_t ld, int layout, void *stream);
/* knn_block_scatter_dt for a byte block packed by knn_block_pack_s8: the byte
 * rows and both norm words of each listed row (made for the position it lands
 * at) and the meta (word 7 stays 1); the same contract against one
 * knn_block_pack_s8 of the updated array.  KNN_ERR_INVALID also for n > 896. */
KNN_API int knn_block_scatter_s8(void *d_sblock, int dtype, size_t cap, const int32_t *d_pos,
                                 const int32_t *d_srow /* nullable */, size_t rows, size_t n, const void *d_src,
                                 size_t src_rows, int src_dtype, size_t ld, int layout, void *stream);
/* knn_block_gather_dt for byte blocks: the row bytes are copied verbatim, and
 * both norm words are made again for the new row (they depend on the row's
 * position) from the norm the source's words hold.  KNN_ERR_INVALID also for
 * n > 896, the byte path's limit. */
KNN_API int knn_block_gather_s8(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                                const int32_t *d_list, size_t rows, size_t n, void *stream);
/* knn_block_gather_pos_dt for byte blocks (d_tab: nblk byte blocks), the norm
 * words made again for the destination row as in knn_block_gather_s8. */
KNN_API int knn_block_gather_pos_s8(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab,
                                    size_t src_cap, size_t nblk, const int32_t *d_pos, size_t rows, size_t n,
                                    void *stream);
KNN_API int knn_s8_spec_ok(const double *h_meta, size_t n, int dtype);
/* begin from the query block's speculative byte block (h_meta: the reduced
 * meta, host; KNN_ERR_INVALID unless knn_s8_spec_ok).  The element block is
 * needed only by the exact rescan: pack it and knn_ctx_attach_qblock before
 * knn_ctx_rescan_step when knn_ctx_end reports unresolved queries. */
KNN_API int knn_ctx_begin_s8(knn_ctx_t *ctx, const void *d_sblock, size_t q_cap, size_t q_base,
                             const double *d_meta, const double *h_meta, void *stream);
KNN_API int knn_ctx_attach_qblock(knn_ctx_t *ctx, const void *d_qblock, size_t q_cap);

/* Fold one packed corpus block (nc rows, global ids c_base..) into the
 * running neighbour lists.  Blocks may come in any order (ring order).
 * Asynchronous and overlapped: the step's distance kernel may start while
 * earlier steps still run (internal streams), and `stream` is made to wait
 * for step s - KNN_STEP_LAG only.  So work enqueued on `stream` after step
 * s returns may overwrite the blocks of steps <= s - KNN_STEP_LAG and no
 * later one: a ring rotates KNN_STEP_LAG + 2 receive buffers (knn_ring.c,
 * mpiknn/ring.py).  knn_ctx_end orders `stream` after every step. */
#define KNN_STEP_LAG 2
/* Shadow-block form of knn_ctx_step; valid while knn_ctx_shadow(ctx) is
 * nonzero after knn_ctx_begin: 1 = fp16 shadow blocks (knn_shadow_pack),
 * 2 = byte blocks of the int8 contraction (8-bit-window integer data, n <=
 * 896: rows as int8 x - o, o from the reduced meta, plus int32 norms).
 * knn_ctx_shadow_bytes / knn_ctx_shadow_pack size and pack a block of
 * capacity cap in the context's current form (the form a ring moves). */
KNN_API int knn_ctx_shadow(const knn_ctx_t *ctx);
KNN_API size_t knn_ctx_shadow_bytes(const knn_ctx_t *ctx, size_t cap);
KNN_API int knn_ctx_shadow_pack(knn_ctx_t *ctx, void *d_sblock, const void *d_block, size_t cap,
                                void *stream);
KNN_API int knn_ctx_step_shadow(knn_ctx_t *ctx, const void *d_sblock, size_t nc, size_t c_base,
                                void *stream);
KNN_API int knn_ctx_step(knn_ctx_t *ctx, const void *d_cblock, size_t nc,
                 size_t c_base, void *stream);
/* Fold nblk resident shadow-form blocks (d_sblocks[b]: nc[b] rows, global
 * ids c_base[b]..; any order) -- the direct-exchange ring's step over every
 * block received from the other ranks (blk:217-242 for all of them at
 * once).  Byte blocks (knn_ctx_shadow == 2) share one distance launch per 8
 * blocks, which counts as ONE step of the lag rule above: none of the
 * blocks may be overwritten before KNN_STEP_LAG further steps (or
 * knn_ctx_end).  fp16 shadow blocks fold one block a step. */
KNN_API int knn_ctx_step_shadow_n(knn_ctx_t *ctx, int nblk, const void *const *d_sblocks,
                                  const size_t *nc, const size_t *c_base, void *stream);
/* The same for nblk resident element blocks (d_cblocks[b]: packed blocks of
 * capacity block_cap): a search on the split-fp16 filter (real-valued data,
 * knn_ctx_split) folds up to 8 of them in one distance launch and one merge,
 * which count as ONE step of the lag rule; other searches fold one block a
 * step. */
KNN_API int knn_ctx_step_n(knn_ctx_t *ctx, int nblk, const void *const *d_cblocks, const size_t *nc,
                           const size_t *c_base, void *stream);

/* Finish: write nq*k records to d_out.  Returns in *unresolved (host; the
 * call synchronises the stream) the number of queries whose candidate set
 * could not be certified exact; if > 0 the caller runs one more pass over
 * every block with knn_ctx_rescan_step() then knn_ctx_rescan_end().  The
 * records are written behind the last merge on the context's own stream,
 * which first waits for `stream` as it stands at the call (so d_out may have
 * just been allocated, cleared or read on `stream`); `stream` is ordered
 * after the records on return.  A search begun with knn_ctx_begin_s8 whose
 * device meta turns out not to be INT-exact reports every query unresolved
 * (nothing is read through the missing element block). */
KNN_API int knn_ctx_end(knn_ctx_t *ctx, knn_neighbour_t *d_out, size_t *unresolved,
                void *stream);
KNN_API int knn_ctx_rescan_step(knn_ctx_t *ctx, const void *d_cblock, size_t nc,
                        size_t c_base, void *stream);
KNN_API int knn_ctx_rescan_end(knn_ctx_t *ctx, knn_neighbour_t *d_out, void *stream);
/* A ring rank's int8 re-search, between knn_ctx_end and the rescan pass:
 * the queries knn_ctx_end left uncertified are searched again on the int8
 * contraction with 65-entry lane lists (as a single-block search does inside
 * knn_ctx_end) against the nblk byte blocks the rank still holds (d_sblocks:
 * its own and the received ones, nc[b] rows from global id c_base[b] --
 * together every row of the corpus); certified queries get their records
 * in d_out.  *unresolved (host; the call synchronises the stream) is the
 * count the rescan pass still has to resolve -- 0 spares the rank the
 * element-block exchange of mpi-knn-parallel_blocking.c:187-214's repeat.
 * A no-op (returning the unchanged count) unless the search ran on the int8
 * contraction in INT mode (knn_ctx_shadow == 2) with k <= 32. */
KNN_API int knn_ctx_research_blocks(knn_ctx_t *ctx, int nblk, const void *const *d_sblocks, const size_t *nc,
                                    const size_t *c_base, knn_neighbour_t *d_out, size_t *unresolved,
                                    void *stream);

/* Convenience: the whole single-device pipeline on one packed block of
 * capacity m (queries == corpus == rows 0..m-1), including the rescan pass
 * when needed.  ctx must have nq == block_cap == m. */
KNN_API int knn_search_packed(knn_ctx_t *ctx, const void *d_block, size_t m,
                      knn_neighbour_t *d_out, void *stream);

/* Diagnostics of the last knn_ctx_end: engine mode (0 integer-exact,
 * 1 fp64 GEMM + exact re-rank, 2 exact scan) and the corpus split count. */
KNN_API int knn_ctx_info(const knn_ctx_t *ctx, int *mode, int *splits);

/* Input width in bits of the MFMA contraction of the current search: 64
 * (fp64 blocks), 32 (fp32 blocks), 16 when it runs on fp16 MFMA because
 * that is exact for the data (integers with max|x| <= 256 (fp64) / 2048
 * (fp32) in the exact-integer range; KNN_NO_H16=1 disables it), or 8 when
 * it runs on int8 MFMA (integers inside a window of 256 values, n <= 896:
 * exact int32 dot products; KNN_NO_I8=1 disables it).  Set by
 * knn_ctx_begin.  0 for a NULL context. */
KNN_API int knn_ctx_contraction_bits(const knn_ctx_t *ctx);
/* 1 when the current search filters with the split fp16 contraction: fp32
 * blocks in GEMM mode (non-integer data), each value scaled by a power of
 * two S and split as S x = hi + lo in fp16, hi.hi + hi.lo + lo.hi on fp16
 * MFMA (fp32 accumulate); the candidates are re-ranked by the exact fp64 S
 * and certified with that filter's error bound (knn_cert_E), so results are
 * those of the fp32 MFMA filter, bit for bit.  KNN_NO_SPLIT=1 disables it. */
KNN_API int knn_ctx_split(const knn_ctx_t *ctx);

/* Kernel timing with HIP events on the launch streams (the timers of
 * serial:70-98 at kernel granularity).  enable = 1 starts recording and
 * zeroes the totals, 0 stops (totals kept), -1 only reads.  Totals (ms) cover
 * every step since the last reset whose knn_ctx_end has returned: dist_ms is
 * the time during which some k_dist_topk runs (the union of their
 * intervals per search -- steps overlap, knn_ctx_step), merge_ms the time
 * k_merge work adds outside it; *launches counts k_dist_topk launches. */
KNN_API int knn_ctx_profile(knn_ctx_t *ctx, int enable, double *dist_ms, double *merge_ms,
                    int *launches);
/* The merge kernels' own time over the same steps (recorded while
 * knn_ctx_profile is on): *merge_kernel_ms sums the durations of every
 * k_merge / k_merge_rank launch (the exact fp64 re-rank of knn-serial.c:
 * 86-91 in GEMM mode; in INT mode the rank merge, which also finalizes at
 * the search's end), bracketed by events on the merge's stream; *merges
 * counts them and *bytes sums their algorithmic bytes (partial lists and
 * bounds read, state read and written or records written, and in GEMM mode
 * the query's and its k neighbours' rows for the exact S) -- bench.py
 * prices them against HBM. */
KNN_API int knn_ctx_profile_merge(knn_ctx_t *ctx, double *merge_kernel_ms, int *merges, double *bytes);

/* on != 0: the context's searches fold ONE block in one step (a P = 1
 * search, knn-serial.c:72-93 over the whole corpus): the step's distance
 * kernel and knn_ctx_end's merge run on the caller's stream, back to back,
 * with no event record or cross-stream wait between them, and end() does
 * not wait for the caller's stream on the host first.  A second step in such
 * a search falls back to the step schedule (exact either way).  Default 0. */
KNN_API int knn_ctx_set_solo(knn_ctx_t *ctx, int on);
/* The keep-zero distance rule (knn_query's KNN_QUERY_KEEP_ZERO) for the
 * context's searches: read by knn_ctx_begin* and held for the search begun,
 * its re-search and its rescan.  Default 0, the reference's rule (blk:217-242,
 * serial:86: S == 0 is no result).  on != 0: a candidate with S == 0 is a
 * result like any other (distance 0.0, lower idx first).  Under either rule a
 * query's own global id (q_base + its row) is never a candidate: the kernels
 * leave it out by id, so the rule only shows on OTHER rows at distance 0 --
 * for queries outside the corpus give them ids past it (q_base = m). */
KNN_API int knn_ctx_set_keep_zero(knn_ctx_t *ctx, int on);
/* The 8 meta doubles the last search's kernels read (copied to mapped host
 * memory by its last kernel; valid after knn_ctx_end returned KNN_OK): a
 * caller that began the search from a meta hint checks it with this,
 * without a read-back copy of its own on the stream. */
KNN_API int knn_ctx_search_meta(const knn_ctx_t *ctx, double *meta);

#ifdef __cplusplus
}
#endif
#endif /* KNN_H */
