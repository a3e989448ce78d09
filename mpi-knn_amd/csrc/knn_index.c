/*
 * knn_index.c -- out-of-sample queries (include/knn.h): the resident corpus
 * index knn_index_* and the one-call knn_query() on top of it.
 *
 * One implementation of the sequence serves both.  build_pack / build_finish
 * pack the corpus from a device source into resident blocks of one capacity
 * (KNN_QUERY_BLOCK=rows overrides the choice): element blocks, their meta
 * MAX-reduced on the host, and byte blocks when that meta passes
 * knn_s8_spec_ok.  run_pack / run_finish pack a batch of queries into tiles of at most
 * KNN_QUERY_TILE_MAX rows (KNN_QUERY_TILE=rows overrides that, for tests)
 * with ids m.. (past every corpus id, so no row is ever "the query itself"),
 * MAX-reduces their meta with the corpus's, and runs the ring rank's sequence
 * against foreign blocks per tile (blk:217-242): begin, the fold of every
 * corpus block, end, the int8 re-search where it applies, then the exact
 * rescan over every block.  The records of every tile stay on the device
 * until the last tile is done: a timed span holds no copy to the host.
 * knn_index_add repeats build_pack / build_finish for rows that arrive later,
 * with the packs at a row offset (knn_block_append_dt / _s8, defined here).
 * knn_index_remove compacts the blocks from the first removed row on with the
 * block gathers (knn_block_gather_dt / _s8, defined here; its host planning:
 * knn_remove_plan.h) and from then on keeps the live rows' ids, which a small
 * kernel writes into every batch's records.
 * knn_index_update writes listed rows in place, one scatter a touched block
 * (knn_block_scatter_dt / _s8, defined here; its host planning:
 * knn_update_plan.h), in knn_index_add's two parts.
 * knn_index_neighbours searches resident rows themselves: its query tiles are
 * filled from the blocks by position (knn_block_gather_pos_dt / _s8, defined
 * here; its host planning: knn_neighbours_plan.h), searched by the same
 * query_tile, and under the keep-zero rule searched at k + 1 with the row
 * itself taken out of its records afterwards (k_drop_self).
 */
#include "knn_internal.h"
#include "knn_remove_plan.h"
#include "knn_update_plan.h"
#include "knn_neighbours_plan.h"

#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>

#define RCHK(x)                  \
    do {                         \
        int rc_ = (x);           \
        if (rc_) return rc_;     \
    } while (0)

#define KNN_QUERY_BYTES_MAX ((size_t)1 << 30)   /* element bytes of one block / tile */
#define KNN_QUERY_TILE_MAX ((size_t)1 << 18)
#define KNN_INDEX_TILE_MIN 128                  /* tile capacity grows from here, doubling */

struct knn_index {
    int dtype;
    size_t m, n;
    /* the corpus: nblk blocks of capacity cap; s8[] only when have_s8 */
    size_t cap, nblk;
    size_t nalloc;                    /* entries of the per-block arrays (>= nblk: knn_index_add grows them) */
    void **blk, **s8;
    size_t *cnc, *cbase;
    int have_s8;
    double cmeta[KNN_META_DOUBLES];   /* host copy of the corpus's reduced meta */
    double *chm;                      /* the blocks' meta as read back (8 doubles a block) */
    double *labels;
    size_t lab_cap;                   /* doubles allocated at labels (>= last_id: labels are indexed by id) */
    /* ids: row p (0-based position in the blocks) has the 1-based id ids[p],
     * ascending.  NULL until the first removal: the id is then p + 1 and
     * last_id == m.  d_ids: its device copy (both of ids_cap entries). */
    size_t last_id;
    int32_t *ids, *d_ids;
    size_t ids_cap;
    /* kept between queries: the context (for k, tile_cap query rows), ntile
     * tile buffers of capacity tile_cap (byte forms allocated on first use),
     * the records of a host-out call, the reduced meta, the span's events */
    knn_ctx_t *ctx;
    int k;
    size_t tile_cap, ntile;
    void **tblk, **ts8;
    double *thm;                      /* the tiles' meta as read back */
    knn_neighbour_t *d_out;
    size_t out_recs;
    double *d_meta, *red;             /* the reduced meta of the batch: device, and its pinned host copy */
    hipEvent_t e0, e1;
    int last_bits;
};

static int dtype_ok(int dtype) { return dtype == KNN_F64 || dtype == KNN_F32; }

static size_t fit_rows(size_t n, int dtype)
{
    /* block and tile capacities: at most KNN_QUERY_BYTES_MAX of elements each */
    const size_t row_bytes = knn_n_pad_dt(n, dtype) * knn_esize(dtype);
    const size_t fit = KNN_QUERY_BYTES_MAX / row_bytes;
    return fit < 1024 ? 1024 : fit;
}

static size_t env_rows(const char *name, size_t dflt, size_t limit)
{
    const char *e = getenv(name);
    if (e && atol(e) > 0) return (size_t)atol(e) < limit ? (size_t)atol(e) : limit;
    return dflt;
}

static void free_query_state(knn_index_t *ix)
{
    for (size_t t = 0; t < ix->ntile; t++) {
        hipFree(ix->tblk[t]);
        hipFree(ix->ts8[t]);
    }
    free(ix->tblk);
    free(ix->ts8);
    free(ix->thm);
    ix->tblk = ix->ts8 = NULL;
    ix->thm = NULL;
    ix->ntile = 0;
    knn_ctx_destroy(ix->ctx);
    ix->ctx = NULL;
}

static void index_free(knn_index_t *ix)
{
    if (!ix) return;
    free_query_state(ix);
    for (size_t b = 0; b < ix->nblk; b++) {
        if (ix->blk) hipFree(ix->blk[b]);
        if (ix->s8) hipFree(ix->s8[b]);
    }
    hipFree(ix->d_out);
    hipFree(ix->d_meta);
    hipFree(ix->d_ids);
    free(ix->ids);
    if (ix->red) hipHostFree(ix->red);
    if (ix->e0) hipEventDestroy(ix->e0);
    if (ix->e1) hipEventDestroy(ix->e1);
    free(ix->blk);
    free(ix->s8);
    free(ix->cnc);
    free(ix->chm);
    free(ix->labels);
    free(ix);
}

/* the host side of an index over an m x n corpus on device 0 (the first
 * device call of every entry point: KNN_ERR_NODEVICE without a gfx950) */
static int index_alloc(knn_index_t **out, size_t m, size_t n, int dtype)
{
    RCHK(knn_device_probe(0, NULL));
    if (hipSetDevice(0) != hipSuccess) return KNN_ERR_HIP;
    knn_index_t *ix = (knn_index_t *)calloc(1, sizeof(*ix));
    if (!ix) return KNN_ERR_NOMEM;
    ix->dtype = dtype;
    ix->m = ix->last_id = m;
    ix->n = n;
    const size_t fit = fit_rows(n, dtype);
    ix->cap = env_rows("KNN_QUERY_BLOCK", m < fit ? m : fit, m);
    ix->nblk = (m + ix->cap - 1) / ix->cap;   /* (<= INT32_MAX) */
    ix->nalloc = ix->nblk;
    ix->blk = (void **)calloc(ix->nblk, sizeof(void *));
    ix->s8 = (void **)calloc(ix->nblk, sizeof(void *));
    ix->cnc = (size_t *)calloc(2 * ix->nblk, sizeof(size_t));
    ix->chm = (double *)calloc(ix->nblk * KNN_META_DOUBLES, sizeof(double));
    if (!ix->blk || !ix->s8 || !ix->cnc || !ix->chm) {
        index_free(ix);
        return KNN_ERR_NOMEM;
    }
    ix->cbase = ix->cnc + ix->nblk;
    if (hipMalloc((void **)&ix->d_meta, KNN_META_DOUBLES * sizeof(double)) != hipSuccess ||
        hipHostMalloc((void **)&ix->red, KNN_META_DOUBLES * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        index_free(ix);
        return KNN_ERR_NOMEM;
    }
    if (hipEventCreate(&ix->e0) != hipSuccess || hipEventCreate(&ix->e1) != hipSuccess) {
        index_free(ix);
        return KNN_ERR_HIP;
    }
    *out = ix;
    return KNN_OK;
}

/* Pack rows r0.. of a `tot`-row device source into nb buffers of capacity bc
 * (buffer b: rows r0 = b * step ..), element blocks (s8 = 0; their meta
 * words gathered behind each pack into hm, 8 doubles a buffer) or byte
 * blocks (s8 = 1).  All on the NULL stream, no wait. */
static int pack_rows(void *const *buf, size_t nb, size_t bc, size_t step, const void *d_src, size_t tot, size_t n,
                     int layout, int src_dtype, int dtype, int s8, double *hm)
{
    const size_t es = knn_src_esize(src_dtype);
    for (size_t b = 0; b < nb; b++) {
        const size_t r0 = b * step, rows = tot - r0 < step ? tot - r0 : step;
        const char *src = (const char *)d_src + (layout == KNN_COLMAJOR ? r0 : r0 * n) * es;
        const size_t ld = layout == KNN_COLMAJOR ? tot : n;
        if (s8) {
            RCHK(knn_block_pack_s8(buf[b], dtype, bc, rows, n, src, src_dtype, ld, layout, NULL));
            continue;
        }
        RCHK(knn_block_pack_dt(buf[b], dtype, bc, rows, n, src, src_dtype, ld, layout, NULL));
        if (hipMemcpyAsync(hm + b * KNN_META_DOUBLES, (const char *)buf[b] + knn_block_meta_offset_dt(bc, n, dtype),
                           KNN_META_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, NULL) != hipSuccess)
            return KNN_ERR_HIP;
    }
    return KNN_OK;
}

/* red = max(red, every buffer's meta) word by word */
static void meta_max(double *red, const double *hm, size_t nb)
{
    for (size_t b = 0; b < nb; b++)
        for (int j = 0; j < KNN_META_DOUBLES; j++)
            if (hm[b * KNN_META_DOUBLES + j] > red[j]) red[j] = hm[b * KNN_META_DOUBLES + j];
}

/* the element blocks' memory (knn_query: ahead of its span) */
static int index_alloc_blocks(knn_index_t *ix)
{
    for (size_t b = 0; b < ix->nblk; b++) {
        ix->cbase[b] = b * ix->cap;
        ix->cnc[b] = ix->m - ix->cbase[b] < ix->cap ? ix->m - ix->cbase[b] : ix->cap;
        if (!ix->blk[b] && hipMalloc(&ix->blk[b], knn_block_bytes_dt(ix->cap, ix->n, ix->dtype)) != hipSuccess)
            return KNN_ERR_NOMEM;
    }
    return KNN_OK;
}

/* The resident corpus blocks from the device source d_X, in two parts around
 * one wait for the NULL stream (knn_query shares that wait with its queries'
 * part): the element packs and their meta on their way to the host ... */
static int build_pack(knn_index_t *ix, const void *d_X, int layout, int src_dtype)
{
    RCHK(index_alloc_blocks(ix));
    return pack_rows(ix->blk, ix->nblk, ix->cap, ix->cap, d_X, ix->m, ix->n, layout, src_dtype, ix->dtype, 0, ix->chm);
}

/* ... and, the meta arrived: its reduction, and for 8-bit data the byte blocks
 * straight from the source (knn_block_pack_s8), resident for every search and
 * re-search */
static int build_finish(knn_index_t *ix, const void *d_X, int layout, int src_dtype, const double *batch_hm,
                        size_t batch_n)
{
    memset(ix->cmeta, 0, sizeof(ix->cmeta));   /* (every meta word is >= 0) */
    meta_max(ix->cmeta, ix->chm, ix->nblk);
    /* knn_query knows its only batch already (batch_hm: its tiles' meta): no
     * byte blocks for a corpus whose queries will not take the byte path */
    double joint[KNN_META_DOUBLES];
    memcpy(joint, ix->cmeta, sizeof(joint));
    if (batch_hm) meta_max(joint, batch_hm, batch_n);
    ix->have_s8 = knn_s8_spec_ok(joint, ix->n, ix->dtype);
    if (!ix->have_s8) return KNN_OK;
    for (size_t b = 0; b < ix->nblk; b++)
        if (hipMalloc(&ix->s8[b], knn_s8_bytes(ix->cap, ix->n)) != hipSuccess) return KNN_ERR_NOMEM;
    return pack_rows(ix->s8, ix->nblk, ix->cap, ix->cap, d_X, ix->m, ix->n, layout, src_dtype, ix->dtype, 1, NULL);
}

/* a batch of mq queries: tiles of *tcap rows, *ntile of them */
static void tile_shape(const knn_index_t *ix, size_t mq, size_t *tcap, size_t *ntile)
{
    const size_t fit = fit_rows(ix->n, ix->dtype);
    size_t t = mq < fit ? mq : fit;
    if (t > KNN_QUERY_TILE_MAX) t = KNN_QUERY_TILE_MAX;
    *tcap = env_rows("KNN_QUERY_TILE", t, mq);
    *ntile = (mq + *tcap - 1) / *tcap;
}

/* The context and the tile buffers for a batch of mq queries at k.  grow: the
 * tile capacity doubles from KNN_INDEX_TILE_MIN rows, so that a stream of
 * varying batch sizes does not reallocate every call (knn_query, one batch:
 * the capacity it needs). */
static int index_reserve(knn_index_t *ix, size_t mq, int k, int grow)
{
    size_t tcap, ntile;
    tile_shape(ix, mq, &tcap, &ntile);
    if (ix->ctx && (k != ix->k || tcap > ix->tile_cap)) free_query_state(ix);
    if (!ix->ctx) {
        size_t cap = grow ? (ix->tile_cap ? ix->tile_cap : KNN_INDEX_TILE_MIN) : tcap;
        while (cap < tcap) cap *= 2;
        RCHK(knn_ctx_create_dt(&ix->ctx, 0, cap, ix->n, ix->cap, k, ix->dtype));
        ix->tile_cap = cap;
        ix->k = k;
    }
    if (ntile > ix->ntile) {
        void **a = (void **)calloc(ntile, sizeof(void *)), **b = (void **)calloc(ntile, sizeof(void *));
        double *hm = (double *)calloc(ntile * KNN_META_DOUBLES, sizeof(double));
        if (!a || !b || !hm) {
            free(a);
            free(b);
            free(hm);
            return KNN_ERR_NOMEM;
        }
        free(ix->thm);
        ix->thm = hm;
        if (ix->ntile) {
            memcpy(a, ix->tblk, ix->ntile * sizeof(void *));
            memcpy(b, ix->ts8, ix->ntile * sizeof(void *));
        }
        free(ix->tblk);
        free(ix->ts8);
        ix->tblk = a;
        ix->ts8 = b;
        ix->ntile = ntile;
    }
    for (size_t t = 0; t < ntile; t++)
        if (!ix->tblk[t] && hipMalloc(&ix->tblk[t], knn_block_bytes_dt(ix->tile_cap, ix->n, ix->dtype)) != hipSuccess)
            return KNN_ERR_NOMEM;
    return KNN_OK;
}

static int query_tile(knn_ctx_t *ctx, size_t nblk, void *const *cblk, void *const *cs8,
                      const size_t *cnc, const size_t *cbase, const void *qblk, const void *qs8, size_t tcap,
                      size_t rows, size_t q_base, const double *d_meta, const double *h_meta,
                      knn_neighbour_t *d_out)
{
    /* the tile's rows within the context's capacity */
    RCHK(knn_ctx_set_rows(ctx, rows));
    size_t unresolved = 0;
    if (qs8) {
        RCHK(knn_ctx_begin_s8(ctx, qs8, tcap, q_base, d_meta, h_meta, NULL));
        RCHK(knn_ctx_step_shadow_n(ctx, (int)nblk, (const void *const *)cs8, cnc, cbase, NULL));
    } else {
        RCHK(knn_ctx_begin_meta(ctx, qblk, tcap, q_base, d_meta, h_meta, NULL));
        RCHK(knn_ctx_step_n(ctx, (int)nblk, (const void *const *)cblk, cnc, cbase, NULL));
    }
    RCHK(knn_ctx_end(ctx, d_out, &unresolved, NULL));
    if (unresolved && qs8) {
        /* the re-search takes every block at once: together they are the corpus */
        RCHK(knn_ctx_attach_qblock(ctx, qblk, tcap));
        RCHK(knn_ctx_research_blocks(ctx, (int)nblk, (const void *const *)cs8, cnc, cbase, d_out, &unresolved, NULL));
    }
    if (unresolved) {
        for (size_t b = 0; b < nblk; b++) RCHK(knn_ctx_rescan_step(ctx, cblk[b], cnc[b], cbase[b], NULL));
        RCHK(knn_ctx_rescan_end(ctx, d_out, NULL));
    }
    return KNN_OK;
}

/* One batch against the resident blocks, mq queries from the device source
 * d_Q, in two parts around one wait for the NULL stream: the tiles' element
 * packs and their meta on their way to the host (the context and the tile
 * buffers reserved by the caller) ... */
static int run_pack(knn_index_t *ix, const void *d_Q, size_t mq, int layout, int src_dtype)
{
    size_t tcap, ntile;
    tile_shape(ix, mq, &tcap, &ntile);
    return pack_rows(ix->tblk, ntile, ix->tile_cap, tcap, d_Q, mq, ix->n, layout, src_dtype, ix->dtype, 0, ix->thm);
}

/* ... and, the meta arrived: its MAX-reduction with the corpus's, the path
 * that allows, and the tiles' searches -- their records into d_out (device),
 * complete on return (knn_ctx_end waits for each tile's). */
static int run_finish(knn_index_t *ix, const void *d_Q, size_t mq, int layout, int src_dtype, int flags,
                      knn_neighbour_t *d_out)
{
    const size_t n = ix->n;
    size_t tcap, ntile;
    tile_shape(ix, mq, &tcap, &ntile);
    knn_ctx_set_keep_zero(ix->ctx, (flags & KNN_QUERY_KEEP_ZERO) != 0);
    /* (pinned, and its last reader done with the call before this one: the
     * copy is enqueued without a wait for the packs in front of it) */
    double *red = ix->red;
    memcpy(red, ix->cmeta, KNN_META_DOUBLES * sizeof(double));
    meta_max(red, ix->thm, ntile);
    if (hipMemcpyAsync(ix->d_meta, red, KNN_META_DOUBLES * sizeof(double), hipMemcpyHostToDevice, NULL) != hipSuccess)
        return KNN_ERR_HIP;
    /* the byte path: the corpus has its byte blocks and the batch is 8-bit too */
    const int use_s8 = ix->have_s8 && knn_s8_spec_ok(red, n, ix->dtype);
    if (use_s8) {
        for (size_t t = 0; t < ntile; t++)
            if (!ix->ts8[t] && hipMalloc(&ix->ts8[t], knn_s8_bytes(ix->tile_cap, n)) != hipSuccess)
                return KNN_ERR_NOMEM;
        RCHK(pack_rows(ix->ts8, ntile, ix->tile_cap, tcap, d_Q, mq, n, layout, src_dtype, ix->dtype, 1, NULL));
    }
    for (size_t t = 0; t < ntile; t++) {
        const size_t r0 = t * tcap, rows = mq - r0 < tcap ? mq - r0 : tcap;
        RCHK(query_tile(ix->ctx, ix->nblk, ix->blk, use_s8 ? ix->s8 : NULL, ix->cnc, ix->cbase, ix->tblk[t],
                        use_s8 ? ix->ts8[t] : NULL, ix->tile_cap, rows, ix->m + r0, ix->d_meta, red,
                        d_out + r0 * (size_t)ix->k));
    }
    ix->last_bits = knn_ctx_contraction_bits(ix->ctx);
    return KNN_OK;
}

static int stream_wait(void) { return hipStreamSynchronize(NULL) == hipSuccess ? KNN_OK : KNN_ERR_HIP; }

/* the index's own record buffer, for cnt records */
static int index_out(knn_index_t *ix, size_t cnt)
{
    if (cnt <= ix->out_recs) return KNN_OK;
    hipFree(ix->d_out);
    ix->d_out = NULL;
    ix->out_recs = 0;
    if (hipMalloc((void **)&ix->d_out, cnt * sizeof(knn_neighbour_t)) != hipSuccess) return KNN_ERR_NOMEM;
    ix->out_recs = cnt;
    return KNN_OK;
}

/* a host array on the device (*d: to hipFree) */
static int upload(void **d, const void *h, size_t bytes)
{
    if (hipMalloc(d, bytes) != hipSuccess) return KNN_ERR_NOMEM;
    return hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

/* the span e0 .. e1 (e1 recorded here) into knn_last_search_seconds() */
static int span_end(knn_index_t *ix)
{
    float ms = 0.f;
    hipEventRecord(ix->e1, NULL);
    if (hipEventSynchronize(ix->e1) != hipSuccess || hipEventElapsedTime(&ms, ix->e0, ix->e1) != hipSuccess)
        return KNN_ERR_HIP;
    knn_set_last_search_seconds(ms * 1e-3);
    return KNN_OK;
}

static void fill_labels(knn_neighbour_t *out, size_t cnt, const double *labels)
{
    for (size_t i = 0; i < cnt; i++) out[i].label = out[i].idx > 0 ? (int32_t)labels[out[i].idx - 1] : 0;
}

int knn_index_create(knn_index_t **index, const void *X, size_t m, size_t n, int layout, int src_dtype,
                     const double *labels, int dtype, int flags)
{
    if (!index || !X || m == 0 || n == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype) || !dtype_ok(dtype)) return KNN_ERR_UNSUPPORTED;
    if (layout != KNN_COLMAJOR && layout != KNN_ROWMAJOR) return KNN_ERR_INVALID;
    if (flags & ~KNN_INDEX_DEVICE_SRC) return KNN_ERR_INVALID;
    if (m > 0x7fffffffULL || n > 0x7fffffffULL) return KNN_ERR_INVALID;
    knn_index_t *ix = NULL;
    RCHK(index_alloc(&ix, m, n, dtype));
    int rc = KNN_OK;
    void *d_X = NULL;
    if (labels) {
        ix->labels = (double *)malloc(m * sizeof(double));
        ix->lab_cap = m;
        if (ix->labels) memcpy(ix->labels, labels, m * sizeof(double));
        else rc = KNN_ERR_NOMEM;
    }
    if (!rc && !(flags & KNN_INDEX_DEVICE_SRC)) rc = upload(&d_X, X, m * n * knn_src_esize(src_dtype));
    const void *src = (flags & KNN_INDEX_DEVICE_SRC) ? X : d_X;
    if (!rc) rc = build_pack(ix, src, layout, src_dtype);
    if (!rc) rc = stream_wait();
    if (!rc) rc = build_finish(ix, src, layout, src_dtype, NULL, 0);
    /* the packs have read the source before the index is handed out */
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    hipFree(d_X);
    if (rc) {
        index_free(ix);
        return rc;
    }
    *index = ix;
    return KNN_OK;
}

int knn_index_query(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int flags,
                    knn_neighbour_t *out)
{
    if (!ix || !Q || !out || mq == 0 || k <= 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (k > (ix->dtype == KNN_F32 ? KNN_MAX_K_F32 : KNN_MAX_K)) return KNN_ERR_UNSUPPORTED;
    if (layout != KNN_COLMAJOR && layout != KNN_ROWMAJOR) return KNN_ERR_INVALID;
    if (flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_SRC | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    if (hipSetDevice(0) != hipSuccess) return KNN_ERR_HIP;
    const size_t cnt = mq * (size_t)k;
    const int dev_out = (flags & KNN_INDEX_DEVICE_OUT) != 0;
    void *d_Q = NULL;
    int rc = dev_out ? KNN_OK : index_out(ix, cnt);
    if (!rc && !(flags & KNN_INDEX_DEVICE_SRC)) rc = upload(&d_Q, Q, mq * ix->n * knn_src_esize(src_dtype));
    if (!rc) rc = index_reserve(ix, mq, k, 1);
    if (!rc) {
        knn_neighbour_t *d_out = dev_out ? out : ix->d_out;
        const void *src = (flags & KNN_INDEX_DEVICE_SRC) ? Q : d_Q;
        hipEventRecord(ix->e0, NULL);
        rc = run_pack(ix, src, mq, layout, src_dtype);
        if (!rc) rc = stream_wait();
        if (!rc) rc = run_finish(ix, src, mq, layout, src_dtype, flags, d_out);
        /* rows were removed: positions -> the ids the caller knows */
        if (!rc && ix->ids) rc = knn_launch_remap_idx(d_out, cnt, ix->d_ids, ix->m, NULL);
        if (!rc) rc = span_end(ix);
        if (!rc && !dev_out && hipMemcpy(out, d_out, cnt * sizeof(knn_neighbour_t), hipMemcpyDeviceToHost) != hipSuccess)
            rc = KNN_ERR_HIP;
    }
    if (rc) {   /* nothing of a failed call is kept */
        hipStreamSynchronize(NULL);
        free_query_state(ix);
    }
    hipFree(d_Q);
    if (!rc && !dev_out && ix->labels) fill_labels(out, cnt, ix->labels);
    return rc;
}

/* ------------------------------------------------------------------ add */

/* Rows that arrive later: block rows row0 .. of a block packed before
 * (include/knn.h).  The entry points live here, beside their first user, and
 * not with knn_block_pack_* in knn_engine.c: that file is also built on its
 * own against stub launchers (tests/engine_trace). */
int knn_block_append_dt(void *d_block, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                        const void *d_src, int src_dtype, size_t ld, int layout, void *stream)
{
    if (!d_block || !d_src || rows == 0 || n == 0 || cap > 0x7fffffffULL || row0 > cap || rows > cap - row0 ||
        n > 0x7fffffffULL || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return KNN_ERR_INVALID;
    if (layout == KNN_COLMAJOR ? ld < rows : (layout == KNN_ROWMAJOR ? ld < n : 1)) return KNN_ERR_INVALID;
    return knn_launch_append(d_block, dtype, cap, row0, rows, n, d_src, src_dtype, ld, layout, stream);
}

int knn_block_append_s8(void *d_sblock, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                        const void *d_src, int src_dtype, size_t ld, int layout, void *stream)
{
    if (!d_sblock || !d_src || rows == 0 || n == 0 || cap > 0x7fffffffULL || row0 > cap || rows > cap - row0 ||
        n > KNN_I8_MAX_N || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return KNN_ERR_INVALID;
    if (layout == KNN_COLMAJOR ? ld < rows : (layout == KNN_ROWMAJOR ? ld < n : 1)) return KNN_ERR_INVALID;
    return knn_launch_append_s8(d_sblock, dtype, cap, row0, rows, n, d_src, src_dtype, ld, layout, stream);
}

/* Block row d_pos[i] <- source row d_srow[i] (include/knn.h).  Beside the
 * appends for the same reason. */
static int scatter_args_ok(const void *d_block, int dtype, size_t cap, const int32_t *d_pos, size_t rows, size_t n,
                           const void *d_src, size_t src_rows, int src_dtype, size_t ld, int layout, size_t n_max)
{
    if (!d_block || !d_pos || !d_src || rows == 0 || n == 0 || src_rows == 0 || cap > 0x7fffffffULL ||
        src_rows > 0x7fffffffULL || n > n_max || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return 0;
    return layout == KNN_COLMAJOR ? ld >= src_rows : (layout == KNN_ROWMAJOR ? ld >= n : 0);
}

int knn_block_scatter_dt(void *d_block, int dtype, size_t cap, const int32_t *d_pos, const int32_t *d_srow,
                         size_t rows, size_t n, const void *d_src, size_t src_rows, int src_dtype, size_t ld,
                         int layout, void *stream)
{
    if (!scatter_args_ok(d_block, dtype, cap, d_pos, rows, n, d_src, src_rows, src_dtype, ld, layout, 0x7fffffffULL))
        return KNN_ERR_INVALID;
    return knn_launch_scatter(d_block, dtype, cap, d_pos, d_srow, rows, n, d_src, src_rows, src_dtype, ld, layout,
                              stream);
}

int knn_block_scatter_s8(void *d_sblock, int dtype, size_t cap, const int32_t *d_pos, const int32_t *d_srow,
                         size_t rows, size_t n, const void *d_src, size_t src_rows, int src_dtype, size_t ld,
                         int layout, void *stream)
{
    if (!scatter_args_ok(d_sblock, dtype, cap, d_pos, rows, n, d_src, src_rows, src_dtype, ld, layout, KNN_I8_MAX_N))
        return KNN_ERR_INVALID;
    return knn_launch_scatter_s8(d_sblock, dtype, cap, d_pos, d_srow, rows, n, d_src, src_rows, src_dtype, ld, layout,
                                 stream);
}

/* Block row row0 + i of d_dst <- row d_list[i] of d_src (include/knn.h).
 * Beside the appends for the same reason. */
static int gather_args_ok(const void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                          const int32_t *d_list, size_t rows, size_t n)
{
    return d_dst && d_src && d_list && d_dst != d_src && rows != 0 && n != 0 && dst_cap <= 0x7fffffffULL &&
           src_cap <= 0x7fffffffULL && src_cap != 0 && row0 <= dst_cap && rows <= dst_cap - row0;
}

int knn_block_gather_dt(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                        const int32_t *d_list, size_t rows, size_t n, int dtype, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n) || !dtype_ok(dtype) ||
        n > 0x7fffffffULL / 8)
        return KNN_ERR_INVALID;
    return knn_launch_gather(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, dtype, stream);
}

int knn_block_gather_s8(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                        const int32_t *d_list, size_t rows, size_t n, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n) || n > KNN_I8_MAX_N)
        return KNN_ERR_INVALID;
    return knn_launch_gather_rows8(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, stream);
}

/* The same out of a corpus held as nblk blocks of capacity src_cap, by global
 * position (include/knn.h).  d_tab: the blocks' pointers, a device array. */
int knn_block_gather_pos_dt(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab, size_t src_cap,
                            size_t nblk, const int32_t *d_pos, size_t rows, size_t n, int dtype, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_tab, src_cap, d_pos, rows, n) || nblk == 0 || !dtype_ok(dtype) ||
        n > 0x7fffffffULL / 8)
        return KNN_ERR_INVALID;
    return knn_launch_gather_pos(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, dtype, stream);
}

int knn_block_gather_pos_s8(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab, size_t src_cap,
                            size_t nblk, const int32_t *d_pos, size_t rows, size_t n, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_tab, src_cap, d_pos, rows, n) || nblk == 0 || n > KNN_I8_MAX_N)
        return KNN_ERR_INVALID;
    return knn_launch_gather_pos8(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, stream);
}

/* the id map (host and device) for at least `need` entries, its m entries kept */
static int index_ids_reserve(knn_index_t *ix, size_t need)
{
    if (need <= ix->ids_cap) return KNN_OK;
    const size_t nc = 2 * ix->ids_cap > need ? 2 * ix->ids_cap : need;
    int32_t *d = NULL;
    if (hipMalloc((void **)&d, nc * sizeof(int32_t)) != hipSuccess) return KNN_ERR_NOMEM;
    int32_t *h = (int32_t *)realloc(ix->ids, nc * sizeof(int32_t));
    if (!h) {
        hipFree(d);
        return KNN_ERR_NOMEM;
    }
    ix->ids = h;   /* (the same entries, whatever follows) */
    if (hipMemcpy(d, h, ix->m * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return KNN_ERR_HIP;
    }
    hipFree(ix->d_ids);
    ix->d_ids = d;
    ix->ids_cap = nc;
    return KNN_OK;
}

/* the per-block arrays for at least nb blocks, their nblk entries kept */
static int index_grow_arrays(knn_index_t *ix, size_t nb)
{
    if (nb <= ix->nalloc) return KNN_OK;
    const size_t na = 2 * ix->nalloc > nb ? 2 * ix->nalloc : nb;
    void **blk = (void **)calloc(na, sizeof(void *)), **s8 = (void **)calloc(na, sizeof(void *));
    size_t *cnc = (size_t *)calloc(2 * na, sizeof(size_t));
    double *chm = (double *)calloc(na * KNN_META_DOUBLES, sizeof(double));
    if (!blk || !s8 || !cnc || !chm) {
        free(blk);
        free(s8);
        free(cnc);
        free(chm);
        return KNN_ERR_NOMEM;
    }
    memcpy(blk, ix->blk, ix->nblk * sizeof(void *));
    memcpy(s8, ix->s8, ix->nblk * sizeof(void *));
    memcpy(cnc, ix->cnc, ix->nblk * sizeof(size_t));
    memcpy(cnc + na, ix->cbase, ix->nblk * sizeof(size_t));
    memcpy(chm, ix->chm, ix->nblk * KNN_META_DOUBLES * sizeof(double));
    free(ix->blk);
    free(ix->s8);
    free(ix->cnc);
    free(ix->chm);
    ix->blk = blk;
    ix->s8 = s8;
    ix->cnc = cnc;
    ix->cbase = cnc + na;
    ix->chm = chm;
    ix->nalloc = na;
    return KNN_OK;
}

/* The corpus in blocks of capacity ncap (> cap): element rows and norms move
 * device to device, a new block's meta is the max of the blocks merged into
 * it, and the byte blocks are converted again from the new element blocks
 * (knn_launch_shadow8 with the corpus meta: for knn_s8_spec_ok data the image
 * the source pack writes on every corpus row; rows past a block's nc are not
 * searched).  No search reads a corpus byte block's trailing meta (begin_s8
 * and step_shadow_n take the reduced meta as arguments), but a later
 * knn_block_append_s8 takes its atomicMax into it: it is written.  Old and new
 * blocks are resident together until the last copy is done.  All or nothing. */
static int index_reblock(knn_index_t *ix, size_t ncap)
{
    const size_t n = ix->n, es = knn_esize(ix->dtype), np = knn_n_pad_dt(n, ix->dtype);
    const size_t nb = (ix->m + ncap - 1) / ncap;
    const size_t orp = knn_rows_pad(ix->cap), nrp = knn_rows_pad(ncap);
    void **blk = (void **)calloc(nb, sizeof(void *)), **s8 = (void **)calloc(nb, sizeof(void *));
    size_t *cnc = (size_t *)calloc(2 * nb, sizeof(size_t));
    double *chm = (double *)calloc(nb * KNN_META_DOUBLES, sizeof(double));
    int rc = blk && s8 && cnc && chm ? KNN_OK : KNN_ERR_NOMEM;
    for (size_t b = 0; b < nb && !rc; b++) {
        const size_t bytes = knn_block_bytes_dt(ncap, n, ix->dtype);
        if (hipMalloc(&blk[b], bytes) != hipSuccess) rc = KNN_ERR_NOMEM;
        else if (hipMemsetAsync(blk[b], 0, bytes, NULL) != hipSuccess) rc = KNN_ERR_HIP;
        if (!rc && ix->have_s8 && hipMalloc(&s8[b], knn_s8_bytes(ncap, n)) != hipSuccess) rc = KNN_ERR_NOMEM;
    }
    /* runs of rows that lie in one old and one new block */
    for (size_t g = 0; g < ix->m && !rc;) {
        const size_t ob = g / ix->cap, oo = g % ix->cap, b = g / ncap, no = g % ncap;
        const size_t len = ix->cnc[ob] - oo < ncap - no ? ix->cnc[ob] - oo : ncap - no;
        const char *src = (const char *)ix->blk[ob];
        char *dst = (char *)blk[b];
        if (hipMemcpyAsync(dst + no * np * es, src + oo * np * es, len * np * es, hipMemcpyDeviceToDevice, NULL) !=
                hipSuccess ||
            hipMemcpyAsync(dst + (nrp * np + no) * es, src + (orp * np + oo) * es, len * es, hipMemcpyDeviceToDevice,
                           NULL) != hipSuccess)
            rc = KNN_ERR_HIP;
        meta_max(chm + b * KNN_META_DOUBLES, ix->chm + ob * KNN_META_DOUBLES, 1);
        g += len;
    }
    if (!rc && ix->have_s8) {
        memcpy(ix->red, ix->cmeta, KNN_META_DOUBLES * sizeof(double));
        if (hipMemcpyAsync(ix->d_meta, ix->red, KNN_META_DOUBLES * sizeof(double), hipMemcpyHostToDevice, NULL) !=
            hipSuccess)
            rc = KNN_ERR_HIP;
    }
    for (size_t b = 0; b < nb && !rc; b++) {
        double hm[KNN_META_DOUBLES];
        memcpy(hm, chm + b * KNN_META_DOUBLES, sizeof(hm));
        hm[KNN_META_S8] = 0.0;   /* (an element block's word 7) */
        if (hipMemcpy((char *)blk[b] + knn_block_meta_offset_dt(ncap, n, ix->dtype), hm, sizeof(hm),
                      hipMemcpyHostToDevice) != hipSuccess)
            rc = KNN_ERR_HIP;
        if (rc || !ix->have_s8) continue;
        rc = knn_launch_shadow8(s8[b], blk[b], ix->dtype, nrp, n, ix->d_meta, NULL);
        hm[KNN_META_S8] = 1.0;
        if (!rc && hipMemcpy((char *)s8[b] + knn_s8_meta_offset(ncap, n), hm, sizeof(hm), hipMemcpyHostToDevice) !=
                       hipSuccess)
            rc = KNN_ERR_HIP;
    }
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    if (rc) {
        for (size_t b = 0; b < nb; b++) {
            if (blk) hipFree(blk[b]);
            if (s8) hipFree(s8[b]);
        }
        free(blk);
        free(s8);
        free(cnc);
        free(chm);
        return rc;
    }
    /* the context was made for the old capacity */
    free_query_state(ix);
    for (size_t b = 0; b < ix->nblk; b++) {
        hipFree(ix->blk[b]);
        hipFree(ix->s8[b]);
    }
    free(ix->blk);
    free(ix->s8);
    free(ix->cnc);
    free(ix->chm);
    ix->blk = blk;
    ix->s8 = s8;
    ix->cnc = cnc;
    ix->cbase = cnc + nb;
    ix->chm = chm;
    ix->cap = ncap;
    ix->nblk = ix->nalloc = nb;
    for (size_t b = 0; b < nb; b++) {
        ix->cbase[b] = b * ncap;
        ix->cnc[b] = ix->m - ix->cbase[b] < ncap ? ix->m - ix->cbase[b] : ncap;
    }
    return KNN_OK;
}

/* `rows` new rows (global rows m ..) from the device source d_X into buf[]:
 * the last block's free rows by an append, then fresh blocks of the index's
 * capacity by a pack; element blocks (s8 = 0: the touched blocks' meta on its
 * way to chm) or byte blocks.  NULL stream, no wait. */
static int add_rows(knn_index_t *ix, void **buf, const void *d_X, size_t rows, int layout, int src_dtype, int s8)
{
    const size_t es = knn_src_esize(src_dtype), n = ix->n, cap = ix->cap;
    const size_t ld = layout == KNN_COLMAJOR ? rows : n;
    for (size_t r = 0; r < rows;) {
        const size_t g = ix->m + r, b = g / cap, off = g % cap;
        const size_t len = cap - off < rows - r ? cap - off : rows - r;
        const char *src = (const char *)d_X + (layout == KNN_COLMAJOR ? r : r * n) * es;
        if (b < ix->nblk) {
            RCHK(s8 ? knn_block_append_s8(buf[b], ix->dtype, cap, off, len, n, src, src_dtype, ld, layout, NULL)
                    : knn_block_append_dt(buf[b], ix->dtype, cap, off, len, n, src, src_dtype, ld, layout, NULL));
        } else {
            const size_t bytes = s8 ? knn_s8_bytes(cap, n) : knn_block_bytes_dt(cap, n, ix->dtype);
            if (!buf[b] && hipMalloc(&buf[b], bytes) != hipSuccess) return KNN_ERR_NOMEM;
            RCHK(s8 ? knn_block_pack_s8(buf[b], ix->dtype, cap, len, n, src, src_dtype, ld, layout, NULL)
                    : knn_block_pack_dt(buf[b], ix->dtype, cap, len, n, src, src_dtype, ld, layout, NULL));
        }
        if (!s8 && hipMemcpyAsync(ix->chm + b * KNN_META_DOUBLES,
                                  (const char *)buf[b] + knn_block_meta_offset_dt(cap, n, ix->dtype),
                                  KNN_META_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, NULL) != hipSuccess)
            return KNN_ERR_HIP;
        r += len;
    }
    return KNN_OK;
}

int knn_index_add(knn_index_t *ix, const void *X, size_t rows, int layout, int src_dtype, const double *labels,
                  int flags)
{
    if (!ix || !X || rows == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (layout != KNN_COLMAJOR && layout != KNN_ROWMAJOR) return KNN_ERR_INVALID;
    if (flags & ~KNN_INDEX_DEVICE_SRC) return KNN_ERR_INVALID;
    if (rows > 0x7fffffffULL || ix->last_id + rows > 0x7fffffffULL) return KNN_ERR_INVALID;
    if ((ix->labels != NULL) != (labels != NULL)) return KNN_ERR_INVALID;
    if (hipSetDevice(0) != hipSuccess) return KNN_ERR_HIP;
    const size_t m1 = ix->m + rows;
    /* one capacity for every block: fixed under KNN_QUERY_BLOCK; else doubled
     * while the add would leave more than one fused byte launch of blocks */
    const size_t fit = fit_rows(ix->n, ix->dtype);
    if (!env_rows("KNN_QUERY_BLOCK", 0, (size_t)-1) && (m1 + ix->cap - 1) / ix->cap > KNN_I8_MAXBLK && ix->cap < fit) {
        size_t ncap = ix->cap;
        while ((m1 + ncap - 1) / ncap > KNN_I8_MAXBLK && ncap < fit) ncap = 2 * ncap < fit ? 2 * ncap : fit;
        RCHK(index_reblock(ix, ncap));
    }
    const size_t nb0 = ix->nblk, nb1 = (m1 + ix->cap - 1) / ix->cap;
    RCHK(index_grow_arrays(ix, nb1));
    const size_t id1 = ix->last_id + rows;   /* (labels are indexed by id) */
    if (labels && id1 > ix->lab_cap) {
        const size_t lc = 2 * ix->lab_cap > id1 ? 2 * ix->lab_cap : id1;
        double *l = (double *)realloc(ix->labels, lc * sizeof(double));
        if (!l) return KNN_ERR_NOMEM;
        ix->labels = l;
        ix->lab_cap = lc;
    }
    if (ix->ids) RCHK(index_ids_reserve(ix, m1));
    void *d_X = NULL;
    int rc = KNN_OK;
    if (!(flags & KNN_INDEX_DEVICE_SRC)) rc = upload(&d_X, X, rows * ix->n * knn_src_esize(src_dtype));
    const void *src = (flags & KNN_INDEX_DEVICE_SRC) ? X : d_X;
    /* build_pack / build_finish's two parts for the new rows: the element
     * rows and the touched blocks' meta, one wait, the corpus meta, the byte
     * rows while it still allows them */
    if (!rc) rc = add_rows(ix, ix->blk, src, rows, layout, src_dtype, 0);
    if (!rc) rc = stream_wait();
    double cmeta[KNN_META_DOUBLES];
    memcpy(cmeta, ix->cmeta, sizeof(cmeta));
    int keep_s8 = 0;
    if (!rc) {
        meta_max(cmeta, ix->chm + ix->m / ix->cap * KNN_META_DOUBLES, nb1 - ix->m / ix->cap);
        keep_s8 = ix->have_s8 && knn_s8_spec_ok(cmeta, ix->n, ix->dtype);
        if (keep_s8) rc = add_rows(ix, ix->s8, src, rows, layout, src_dtype, 1);
    }
    /* the new rows' ids last_id + 1 .. behind the live ones (entries past m
     * are read by nothing until m is committed below) */
    if (!rc && ix->ids) {
        for (size_t r = 0; r < rows; r++) ix->ids[ix->m + r] = (int32_t)(ix->last_id + 1 + r);
        if (hipMemcpyAsync(ix->d_ids + ix->m, ix->ids + ix->m, rows * sizeof(int32_t), hipMemcpyHostToDevice, NULL) !=
            hipSuccess)
            rc = KNN_ERR_HIP;
    }
    /* the packs have read the source before the call returns */
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    hipFree(d_X);
    if (rc) {
        /* rows written past a block's nc are never read, and its meta only grew */
        for (size_t b = nb0; b < nb1; b++) {
            hipFree(ix->blk[b]);
            hipFree(ix->s8[b]);
            ix->blk[b] = ix->s8[b] = NULL;
        }
        return rc;
    }
    if (ix->have_s8 && !keep_s8) {
        /* a value outside the byte image arrived: the element path from now on */
        for (size_t b = 0; b < nb0; b++) {
            hipFree(ix->s8[b]);
            ix->s8[b] = NULL;
        }
        ix->have_s8 = 0;
    }
    if (labels) memcpy(ix->labels + ix->last_id, labels, rows * sizeof(double));
    memcpy(ix->cmeta, cmeta, sizeof(cmeta));
    ix->nblk = nb1;
    ix->m = m1;
    ix->last_id = id1;
    for (size_t b = 0; b < nb1; b++) {
        ix->cbase[b] = b * ix->cap;
        ix->cnc[b] = m1 - ix->cbase[b] < ix->cap ? m1 - ix->cbase[b] : ix->cap;
    }
    return KNN_OK;
}

/* --------------------------------------------------------------- remove */

/* The device side of a plan that moves rows: every block from pl->b0 on is
 * built again in a fresh, zeroed buffer by one gather a run (and one of the
 * byte rows where the index has byte blocks), its meta the max of the blocks
 * it drew from.  Old and new buffers are resident together until the one wait
 * at the end; on success the new ones are in nblk[] / ns8[] / nhm (entries
 * b0 .. nb1-1), on failure everything made here is freed. */
static int remove_move(knn_index_t *ix, const knn_rm_plan_t *pl, void **nblk, void **ns8, double *nhm)
{
    const size_t n = ix->n, cap = ix->cap, b0 = pl->b0, nb1 = pl->nb1;
    const size_t ebytes = knn_block_bytes_dt(cap, n, ix->dtype), sbytes = knn_s8_bytes(cap, n);
    int32_t *d_list = NULL;
    double *hm = (double *)calloc(2 * (nb1 - b0) * KNN_META_DOUBLES, sizeof(double));   /* staged until the wait */
    int rc = hm ? KNN_OK : KNN_ERR_NOMEM;
    for (size_t b = b0; b < nb1 && !rc; b++) {
        if (hipMalloc(&nblk[b], ebytes) != hipSuccess) rc = KNN_ERR_NOMEM;
        else if (hipMemsetAsync(nblk[b], 0, ebytes, NULL) != hipSuccess) rc = KNN_ERR_HIP;
        if (rc || !ix->have_s8) continue;
        if (hipMalloc(&ns8[b], sbytes) != hipSuccess) rc = KNN_ERR_NOMEM;
        else if (hipMemsetAsync(ns8[b], 0, sbytes, NULL) != hipSuccess) rc = KNN_ERR_HIP;
    }
    /* the runs' lists, one array */
    if (!rc && hipMalloc((void **)&d_list, pl->nlist * sizeof(int32_t)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc && hipMemcpyAsync(d_list, pl->list, pl->nlist * sizeof(int32_t), hipMemcpyHostToDevice, NULL) != hipSuccess)
        rc = KNN_ERR_HIP;
    for (size_t r = 0; r < pl->nruns && !rc; r++) {
        const knn_rm_run_t *run = &pl->runs[r];
        rc = knn_block_gather_dt(nblk[run->nb], cap, run->dst0, ix->blk[run->ob], cap, d_list + run->list0, run->rows,
                                 n, ix->dtype, NULL);
        if (!rc && ix->have_s8)
            rc = knn_block_gather_s8(ns8[run->nb], cap, run->dst0, ix->s8[run->ob], cap, d_list + run->list0,
                                     run->rows, n, NULL);
        meta_max(nhm + run->nb * KNN_META_DOUBLES, ix->chm + run->ob * KNN_META_DOUBLES, 1);
    }
    /* the trailing meta words, as index_reblock writes them (a later append
     * takes its atomicMax into them) */
    for (size_t b = b0; b < nb1 && !rc; b++) {
        double *e = hm + 2 * (b - b0) * KNN_META_DOUBLES, *s = e + KNN_META_DOUBLES;
        memcpy(e, nhm + b * KNN_META_DOUBLES, KNN_META_DOUBLES * sizeof(double));
        e[KNN_META_S8] = 0.0;
        if (hipMemcpyAsync((char *)nblk[b] + knn_block_meta_offset_dt(cap, n, ix->dtype), e,
                           KNN_META_DOUBLES * sizeof(double), hipMemcpyHostToDevice, NULL) != hipSuccess)
            rc = KNN_ERR_HIP;
        if (rc || !ix->have_s8) continue;
        memcpy(s, e, KNN_META_DOUBLES * sizeof(double));
        s[KNN_META_S8] = 1.0;
        if (hipMemcpyAsync((char *)ns8[b] + knn_s8_meta_offset(cap, n), s, KNN_META_DOUBLES * sizeof(double),
                           hipMemcpyHostToDevice, NULL) != hipSuccess)
            rc = KNN_ERR_HIP;
    }
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    hipFree(d_list);
    free(hm);
    if (rc)
        for (size_t b = b0; b < nb1; b++) {
            hipFree(nblk[b]);
            hipFree(ns8[b]);
            nblk[b] = ns8[b] = NULL;
        }
    return rc;
}

int knn_index_remove(knn_index_t *ix, const int32_t *ids, size_t count, int flags, size_t *removed)
{
    if (!ix || !ids || count == 0 || flags != 0) return KNN_ERR_INVALID;
    for (size_t i = 0; i < count; i++)
        if (ids[i] < 1 || (size_t)ids[i] > ix->last_id) return KNN_ERR_INVALID;
    /* the plan, on the host alone (knn_remove_plan.h) */
    int32_t *pos = (int32_t *)malloc(count * sizeof(int32_t));
    if (!pos) return KNN_ERR_NOMEM;
    memcpy(pos, ids, count * sizeof(int32_t));
    const size_t npos = knn_rm_positions(ix->ids, ix->m, pos, knn_rm_sort_dedupe(pos, count));
    if (npos == 0 || npos >= ix->m) {
        /* nothing live in the list; or no live row would be left */
        free(pos);
        if (npos == 0 && removed) *removed = 0;
        return npos == 0 ? KNN_OK : KNN_ERR_INVALID;
    }
    knn_rm_plan_t pl;
    const int prc = knn_rm_plan(&pl, ix->ids, ix->m, ix->cap, pos, npos);
    free(pos);
    if (prc) return KNN_ERR_NOMEM;
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    /* the new id map beside the old one, and the moved blocks beside theirs */
    const size_t icap = ix->ids_cap > pl.m1 ? ix->ids_cap : pl.m1;
    int32_t *d_ids = NULL, *h_ids = NULL;
    void **nblk = (void **)calloc(2 * ix->nblk, sizeof(void *)), **ns8 = nblk ? nblk + ix->nblk : NULL;
    double *nhm = (double *)calloc(ix->nblk * KNN_META_DOUBLES, sizeof(double));
    if (!rc && (!nblk || !nhm)) rc = KNN_ERR_NOMEM;
    if (!rc && !(h_ids = (int32_t *)malloc(icap * sizeof(int32_t)))) rc = KNN_ERR_NOMEM;
    if (!rc && hipMalloc((void **)&d_ids, icap * sizeof(int32_t)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc) {
        memcpy(h_ids, pl.ids, pl.m1 * sizeof(int32_t));
        if (hipMemcpy(d_ids, h_ids, pl.m1 * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) rc = KNN_ERR_HIP;
    }
    if (!rc && pl.moves) rc = remove_move(ix, &pl, nblk, ns8, nhm);
    if (rc) {   /* the index answers as before the call */
        hipFree(d_ids);
        free(h_ids);
        free(nblk);
        free(nhm);
        knn_rm_plan_free(&pl);
        return rc;
    }
    /* commit: the moved blocks in place of the old ones, the blocks past the
     * new count released, then m, cnc, cbase, nblk and the id map.  cmeta
     * stays: a MAX that has only become too large is conservative. */
    if (pl.moves)
        for (size_t b = pl.b0; b < pl.nb1; b++) {
            hipFree(ix->blk[b]);
            hipFree(ix->s8[b]);
            ix->blk[b] = nblk[b];
            ix->s8[b] = ns8[b];
            memcpy(ix->chm + b * KNN_META_DOUBLES, nhm + b * KNN_META_DOUBLES, KNN_META_DOUBLES * sizeof(double));
        }
    for (size_t b = pl.nb1; b < ix->nblk; b++) {
        hipFree(ix->blk[b]);
        hipFree(ix->s8[b]);
        ix->blk[b] = ix->s8[b] = NULL;
    }
    ix->m = pl.m1;
    ix->nblk = pl.nb1;
    for (size_t b = 0; b < ix->nblk; b++) {
        ix->cbase[b] = b * ix->cap;
        ix->cnc[b] = ix->m - ix->cbase[b] < ix->cap ? ix->m - ix->cbase[b] : ix->cap;
    }
    hipFree(ix->d_ids);
    free(ix->ids);
    ix->ids = h_ids;
    ix->d_ids = d_ids;
    ix->ids_cap = icap;
    if (removed) *removed = pl.removed;
    free(nblk);
    free(nhm);
    knn_rm_plan_free(&pl);
    return KNN_OK;
}

/* --------------------------------------------------------------- update */

/* one scatter a run of the plan, into the element blocks (s8 = 0: the touched
 * blocks' meta on its way to chm) or the byte blocks; d_list: the plan's pos
 * then its srow.  NULL stream, no wait. */
static int update_rows(knn_index_t *ix, const knn_up_plan_t *pl, const int32_t *d_list, const void *d_X, int layout,
                       int src_dtype, int s8)
{
    const size_t n = ix->n, cap = ix->cap, count = pl->count;
    const size_t ld = layout == KNN_COLMAJOR ? count : n;
    for (size_t r = 0; r < pl->nruns; r++) {
        const knn_up_run_t *run = &pl->runs[r];
        const int32_t *pos = d_list + run->list0, *srow = d_list + count + run->list0;
        void *blk = s8 ? ix->s8[run->blk] : ix->blk[run->blk];
        RCHK(s8 ? knn_block_scatter_s8(blk, ix->dtype, cap, pos, srow, run->rows, n, d_X, count, src_dtype, ld, layout,
                                       NULL)
                : knn_block_scatter_dt(blk, ix->dtype, cap, pos, srow, run->rows, n, d_X, count, src_dtype, ld, layout,
                                       NULL));
        if (!s8 && hipMemcpyAsync(ix->chm + run->blk * KNN_META_DOUBLES,
                                  (const char *)blk + knn_block_meta_offset_dt(cap, n, ix->dtype),
                                  KNN_META_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, NULL) != hipSuccess)
            return KNN_ERR_HIP;
    }
    return KNN_OK;
}

int knn_index_update(knn_index_t *ix, const int32_t *ids, size_t count, const void *X, int layout, int src_dtype,
                     const double *labels, int flags)
{
    if (!ix || !ids || !X || count == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (layout != KNN_COLMAJOR && layout != KNN_ROWMAJOR) return KNN_ERR_INVALID;
    if (flags & ~KNN_INDEX_DEVICE_SRC) return KNN_ERR_INVALID;
    if (count > ix->m || (labels && !ix->labels)) return KNN_ERR_INVALID;   /* (more ids than live rows: a repeat) */
    for (size_t i = 0; i < count; i++)
        if (ids[i] < 1 || (size_t)ids[i] > ix->last_id) return KNN_ERR_INVALID;
    /* the plan, on the host alone (knn_update_plan.h) */
    knn_up_plan_t pl;
    const int prc = knn_up_plan(&pl, ix->ids, ix->m, ix->cap, ids, count);
    if (prc) return prc == KNN_UP_NOMEM ? KNN_ERR_NOMEM : KNN_ERR_INVALID;
    /* every allocation and upload in front of the first overwritten row: up
     * to there a failure leaves the index as it was */
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    void *d_X = NULL;
    int32_t *d_list = NULL;
    if (!rc && !(flags & KNN_INDEX_DEVICE_SRC)) rc = upload(&d_X, X, count * ix->n * knn_src_esize(src_dtype));
    if (!rc && hipMalloc((void **)&d_list, 2 * count * sizeof(int32_t)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc && (hipMemcpy(d_list, pl.pos, count * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_list + count, pl.srow, count * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess))
        rc = KNN_ERR_HIP;
    if (rc) {
        hipFree(d_X);
        hipFree(d_list);
        knn_up_plan_free(&pl);
        return rc;
    }
    const void *src = (flags & KNN_INDEX_DEVICE_SRC) ? X : d_X;
    /* knn_index_add's two parts for the listed rows: the element rows and the
     * touched blocks' meta, one wait, the corpus meta, the byte rows while it
     * still allows them.  From here on a failure leaves rows half written:
     * KNN_ERR_HIP, and the index is fit only for knn_index_destroy. */
    rc = update_rows(ix, &pl, d_list, src, layout, src_dtype, 0);
    if (!rc) rc = stream_wait();
    double cmeta[KNN_META_DOUBLES];
    memcpy(cmeta, ix->cmeta, sizeof(cmeta));
    int keep_s8 = 0;
    if (!rc) {
        for (size_t r = 0; r < pl.nruns; r++) meta_max(cmeta, ix->chm + pl.runs[r].blk * KNN_META_DOUBLES, 1);
        keep_s8 = ix->have_s8 && knn_s8_spec_ok(cmeta, ix->n, ix->dtype);
        if (keep_s8) rc = update_rows(ix, &pl, d_list, src, layout, src_dtype, 1);
    }
    /* the scatters have read the source and the lists before the call returns */
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    hipFree(d_X);
    hipFree(d_list);
    if (rc) {
        knn_up_plan_free(&pl);
        return KNN_ERR_HIP;
    }
    if (ix->have_s8 && !keep_s8) {
        /* a value outside the byte image arrived: the element path from now on */
        for (size_t b = 0; b < ix->nblk; b++) {
            hipFree(ix->s8[b]);
            ix->s8[b] = NULL;
        }
        ix->have_s8 = 0;
    }
    if (labels)
        for (size_t i = 0; i < count; i++) ix->labels[ids[i] - 1] = labels[i];
    memcpy(ix->cmeta, cmeta, sizeof(cmeta));
    knn_up_plan_free(&pl);
    return KNN_OK;
}

/* ----------------------------------------------------------- neighbours */

/* The query tiles of knn_index_neighbours: tile t's rows are the resident
 * rows at positions d_pos[t tcap ..], copied out of the blocks (d_tab: the
 * element blocks' pointers, then the byte blocks' when s8).  Device to device
 * on the NULL stream, no wait, nothing read back.
 *
 * A gather writes the listed rows and their norms only, where a pack writes
 * the whole padded tile, and the tile buffers are kept between calls: past
 * `rows` they hold whatever an earlier, larger batch left there.  What reads
 * those rows: the element kernels (k_dist_topk and its fp16 / fp32 / split
 * forms) stage a tile's rows and norms up to round_up(rows, KNN_TQ) -- the
 * padding queries reject every candidate and write nothing, so the values
 * never reach a result -- and the query block's conversions in knn_ctx_begin*
 * (fp16, split and byte shadows) convert every padded row for the same
 * readers.  k_dist_topk_i8 reads row rows - 1 in their place, and the
 * re-search and the rescan read listed queries only.  The element rows and
 * norms in [rows, round_up(rows, KNN_TQ)) are cleared all the same, to the
 * zeros a pack leaves there: no kernel then computes on stale or never
 * written memory, whatever it does with the result.  The byte tile needs
 * nothing. */
static int gather_tiles(knn_index_t *ix, const void *const *d_tab, const int32_t *d_pos, size_t mq, int s8)
{
    const size_t n = ix->n, es = knn_esize(ix->dtype), np = knn_n_pad_dt(n, ix->dtype);
    const size_t trp = knn_rows_pad(ix->tile_cap);
    size_t tcap, ntile;
    tile_shape(ix, mq, &tcap, &ntile);
    for (size_t t = 0; t < ntile; t++) {
        const size_t r0 = t * tcap, rows = mq - r0 < tcap ? mq - r0 : tcap;
        const size_t pad = knn_round_up(rows, KNN_TQ) - rows;   /* (round_up(rows, KNN_TQ) <= trp) */
        char *blk = (char *)ix->tblk[t];
        RCHK(knn_block_gather_pos_dt(blk, ix->tile_cap, 0, d_tab, ix->cap, ix->nblk, d_pos + r0, rows, n, ix->dtype,
                                     NULL));
        if (pad && (hipMemsetAsync(blk + rows * np * es, 0, pad * np * es, NULL) != hipSuccess ||
                    hipMemsetAsync(blk + (trp * np + rows) * es, 0, pad * es, NULL) != hipSuccess))
            return KNN_ERR_HIP;
        if (s8)
            RCHK(knn_block_gather_pos_s8(ix->ts8[t], ix->tile_cap, 0, d_tab + ix->nblk, ix->cap, ix->nblk, d_pos + r0,
                                         rows, n, NULL));
    }
    return KNN_OK;
}

int knn_index_neighbours(knn_index_t *ix, const int32_t *ids, size_t count, int k, int flags, knn_neighbour_t *out)
{
    if (!ix || !out || k <= 0 || (ids ? count == 0 : count != 0)) return KNN_ERR_INVALID;
    if (flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    /* keep-zero: the row itself comes back among its own neighbours and is
     * taken out afterwards, so the engine searches one more */
    const int kz = (flags & KNN_QUERY_KEEP_ZERO) != 0, dev_out = (flags & KNN_INDEX_DEVICE_OUT) != 0;
    if (k > (ix->dtype == KNN_F32 ? KNN_MAX_K_F32 : KNN_MAX_K) - kz) return KNN_ERR_UNSUPPORTED;
    const int ke = k + kz;
    const size_t mq = ids ? count : ix->m;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    for (size_t i = 0; i < count; i++)
        if (ids[i] < 1 || (size_t)ids[i] > ix->last_id) return KNN_ERR_INVALID;
    /* the positions, on the host alone (knn_neighbours_plan.h) */
    int32_t *pos = (int32_t *)malloc(mq * sizeof(int32_t));
    if (!pos) return KNN_ERR_NOMEM;
    if (knn_nb_positions(ix->ids, ix->m, ids, count, pos)) {
        free(pos);
        return KNN_ERR_INVALID;
    }
    const size_t n = ix->n, cnt = mq * (size_t)k, wide = kz ? mq * (size_t)ke : 0;
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    /* every allocation and upload in front of the span: the positions, the
     * blocks' pointers (element, then byte), the records of a host-out call
     * and behind them the k + 1 wide ones of a keep-zero call */
    const int use_s8 = ix->have_s8 && knn_s8_spec_ok(ix->cmeta, n, ix->dtype);
    int32_t *d_pos = NULL;
    void **d_tab = NULL;
    if (!rc) rc = index_out(ix, (dev_out ? 0 : cnt) + wide);
    if (!rc && hipMalloc((void **)&d_pos, mq * sizeof(int32_t)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc && hipMalloc((void **)&d_tab, 2 * ix->nblk * sizeof(void *)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc && (hipMemcpy(d_pos, pos, mq * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_tab, ix->blk, ix->nblk * sizeof(void *), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_tab + ix->nblk, ix->s8, ix->nblk * sizeof(void *), hipMemcpyHostToDevice) != hipSuccess))
        rc = KNN_ERR_HIP;
    free(pos);
    if (!rc) rc = index_reserve(ix, mq, ke, 1);
    size_t tcap = 0, ntile = 0;
    if (!rc) tile_shape(ix, mq, &tcap, &ntile);
    for (size_t t = 0; t < ntile && !rc && use_s8; t++)
        if (!ix->ts8[t] && hipMalloc(&ix->ts8[t], knn_s8_bytes(ix->tile_cap, n)) != hipSuccess) rc = KNN_ERR_NOMEM;
    if (!rc) {
        knn_neighbour_t *d_out = dev_out ? out : ix->d_out;
        knn_neighbour_t *d_rec = kz ? ix->d_out + (dev_out ? 0 : cnt) : d_out;   /* what the tiles write */
        hipEventRecord(ix->e0, NULL);
        /* the batch's reduced meta is the corpus's: the queries are corpus
         * rows and cmeta only grows.  No tile meta is read back, so the host
         * does not wait between the gathers and the searches. */
        memcpy(ix->red, ix->cmeta, KNN_META_DOUBLES * sizeof(double));
        if (hipMemcpyAsync(ix->d_meta, ix->red, KNN_META_DOUBLES * sizeof(double), hipMemcpyHostToDevice, NULL) !=
            hipSuccess)
            rc = KNN_ERR_HIP;
        if (!rc) rc = gather_tiles(ix, (const void *const *)d_tab, d_pos, mq, use_s8);
        knn_ctx_set_keep_zero(ix->ctx, kz);
        for (size_t t = 0; t < ntile && !rc; t++) {
            const size_t r0 = t * tcap, rows = mq - r0 < tcap ? mq - r0 : tcap;
            rc = query_tile(ix->ctx, ix->nblk, ix->blk, use_s8 ? ix->s8 : NULL, ix->cnc, ix->cbase, ix->tblk[t],
                            use_s8 ? ix->ts8[t] : NULL, ix->tile_cap, rows, ix->m + r0, ix->d_meta, ix->red,
                            d_rec + r0 * (size_t)ke);
        }
        if (!rc) ix->last_bits = knn_ctx_contraction_bits(ix->ctx);
        /* keep-zero: the row itself out of its k + 1 records, positions -> ids
         * in the same pass; else the ids as knn_index_query writes them */
        if (!rc && kz) rc = knn_launch_drop_self(d_out, d_rec, d_pos, mq, k, ix->ids ? ix->d_ids : NULL, ix->m, NULL);
        else if (!rc && ix->ids) rc = knn_launch_remap_idx(d_out, cnt, ix->d_ids, ix->m, NULL);
        if (!rc) rc = span_end(ix);
        if (!rc && !dev_out && hipMemcpy(out, d_out, cnt * sizeof(knn_neighbour_t), hipMemcpyDeviceToHost) != hipSuccess)
            rc = KNN_ERR_HIP;
    }
    if (rc) {   /* nothing of a failed call is kept */
        hipStreamSynchronize(NULL);
        free_query_state(ix);
    }
    hipFree(d_pos);
    hipFree(d_tab);
    if (!rc && !dev_out && ix->labels) fill_labels(out, cnt, ix->labels);
    return rc;
}

int knn_index_last_id(const knn_index_t *ix, size_t *last_id)
{
    if (!ix || !last_id) return KNN_ERR_INVALID;
    *last_id = ix->last_id;
    return KNN_OK;
}

int knn_index_info(const knn_index_t *ix, size_t *m, size_t *n, int *nblocks, size_t *device_bytes, int *last_bits)
{
    if (!ix) return KNN_ERR_INVALID;
    if (m) *m = ix->m;
    if (n) *n = ix->n;
    if (nblocks) *nblocks = (int)ix->nblk;
    if (last_bits) *last_bits = ix->last_bits;
    if (device_bytes) {
        size_t b = ix->nblk * knn_block_bytes_dt(ix->cap, ix->n, ix->dtype) + KNN_META_DOUBLES * sizeof(double);
        if (ix->have_s8) b += ix->nblk * knn_s8_bytes(ix->cap, ix->n);
        for (size_t t = 0; t < ix->ntile; t++) {
            if (ix->tblk[t]) b += knn_block_bytes_dt(ix->tile_cap, ix->n, ix->dtype);
            if (ix->ts8[t]) b += knn_s8_bytes(ix->tile_cap, ix->n);
        }
        b += ix->out_recs * sizeof(knn_neighbour_t);
        if (ix->d_ids) b += ix->ids_cap * sizeof(int32_t);
        *device_bytes = b + knn_ctx_device_bytes(ix->ctx);
    }
    return KNN_OK;
}

int knn_index_destroy(knn_index_t *ix)
{
    if (!ix) return KNN_ERR_INVALID;
    hipSetDevice(0);
    index_free(ix);
    return KNN_OK;
}

/* knn_query: an index that lives for one call.  Both uploads come first, so
 * the span -- corpus pack through the last tile's records -- holds no copy
 * from or to the host. */
int knn_query(const double *X, size_t m, const double *Q, size_t mq, size_t n, int layout, const double *labels,
              int k, int dtype, int flags, knn_neighbour_t *out)
{
    if (!X || !Q || !out || m == 0 || mq == 0 || n == 0 || k <= 0) return KNN_ERR_INVALID;
    if (!dtype_ok(dtype)) return KNN_ERR_UNSUPPORTED;
    if (k > (dtype == KNN_F32 ? KNN_MAX_K_F32 : KNN_MAX_K)) return KNN_ERR_UNSUPPORTED;
    if (layout != KNN_COLMAJOR && layout != KNN_ROWMAJOR) return KNN_ERR_INVALID;
    if (flags & ~KNN_QUERY_KEEP_ZERO) return KNN_ERR_INVALID;
    if (m > 0x7fffffffULL || mq > 0x7fffffffULL || m + mq > 0x7fffffffULL || n > 0x7fffffffULL)
        return KNN_ERR_INVALID;
    knn_index_t *ix = NULL;
    RCHK(index_alloc(&ix, m, n, dtype));
    const size_t cnt = mq * (size_t)k;
    void *d_X = NULL, *d_Q = NULL;
    /* every allocation, then the uploads: the span starts behind a copy, with
     * no fresh memory still to be mapped in front of its first kernel */
    int rc = index_reserve(ix, mq, k, 0);
    if (!rc) rc = index_out(ix, cnt);
    if (!rc) rc = index_alloc_blocks(ix);
    if (!rc) rc = upload(&d_X, X, m * n * sizeof(double));
    if (!rc) rc = upload(&d_Q, Q, mq * n * sizeof(double));
    if (!rc) {
        /* every block and tile packed, one wait for their meta, then the byte
         * forms and the searches */
        hipEventRecord(ix->e0, NULL);
        rc = build_pack(ix, d_X, layout, KNN_F64);
        if (!rc) rc = run_pack(ix, d_Q, mq, layout, KNN_F64);
        if (!rc) rc = stream_wait();
        if (!rc) rc = build_finish(ix, d_X, layout, KNN_F64, ix->thm, ix->ntile);
        if (!rc) rc = run_finish(ix, d_Q, mq, layout, KNN_F64, flags, ix->d_out);
        if (!rc) rc = span_end(ix);
    }
    if (!rc && hipMemcpy(out, ix->d_out, cnt * sizeof(knn_neighbour_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = KNN_ERR_HIP;
    if (rc) hipStreamSynchronize(NULL);
    hipFree(d_X);
    hipFree(d_Q);
    index_free(ix);
    if (!rc && labels) fill_labels(out, cnt, labels);
    return rc;
}
