/*
 * knn_index.c -- out-of-sample queries (include/knn.h): the resident corpus
 * index knn_index_* and the one-call knn_query() on top of it.
 *
 * The corpus is resident as blocks of one capacity (KNN_QUERY_BLOCK=rows
 * overrides the choice): element blocks, their meta MAX-reduced on the host,
 * and byte blocks while that meta passes knn_s8_spec_ok.  The per-block host
 * arrays are one blocks_t; set_counts, fresh_blocks, write_meta_words,
 * read_meta and drop_s8 are what every entry point does with them.  The device
 * memory the index holds between calls has one owner: the byte count
 * dev_bytes, kept by knn_buf_alloc / knn_buf_release (knn_buf.h, shared with
 * the context) under own_grow, own_grow_keep (d_meta, d_out, d_ids, d_labels:
 * each a knn_buf_t that knows its size) and image_alloc, images_release (the
 * blocks and tiles, by their set's capacity); knn_index_info reports that
 * count and the context's.  What a call allocates for itself (scratch) is
 * freed on every exit and not counted.  A batch of queries is a batch_t: tiles of at most
 * KNN_QUERY_TILE_MAX rows (KNN_QUERY_TILE=rows overrides that, for tests) with
 * ids m.. (past every corpus id, so no row is ever "the query itself").
 * Every entry point reads: checks, plan, reserve, enqueue, wait, commit.
 * create, knn_query: build_pack / build_finish pack the corpus from a device
 * source (dev_src_t) in two parts around one wait.  query: run_pack /
 * run_finish pack the tiles, MAX-reduce their meta with the corpus's
 * (put_meta) and run search_tiles -- per tile the ring rank's sequence against
 * foreign blocks (blk:217-242; query_tile) -- and finish_search ends every
 * search call: ids for positions, the span, a classify call's vote, the
 * records, which stay on the device until the last tile is done (a timed span
 * holds no copy to the host), and on failure a wait and the query state
 * dropped.  add: the
 * two parts again for rows that arrive later, the packs at a row offset, behind
 * index_reblock where the blocks would become too many.  remove: compacts the
 * blocks from the first removed row on with the block gathers
 * (knn_remove_plan.h) and from then on keeps the live rows' ids.  update: one
 * scatter a touched block (knn_update_plan.h) in add's two parts (s8_stays,
 * commit_meta).  neighbours: tiles filled from the blocks by position
 * (knn_neighbours_plan.h), the same search_tiles, and under the keep-zero rule
 * k + 1 with the row itself taken out afterwards (k_drop_self).  classify,
 * classify_rows: query's and neighbours' calls (query_call, rows_call) with a
 * vote_t: vote_begin in front of the span -- the labels' device copy, which
 * the first such call makes and add / update keep marked (labels_sync,
 * labels_stale), and the vote's scratch -- and the vote over the records on
 * the device behind it, its host outputs through a staging array so that a
 * failed call has written none of them.  classify_weighted, regress and their
 * _rows forms: the same two calls with the same vote_t, its launch the
 * weighted vote or the regression (knn_predict.hip) and its outputs of 8-byte
 * entries where those are doubles.  radius_count,
 * radius and their _rows forms: distance kernels of their own with CSR output
 * (knn_radius.hip) behind query's packs / neighbours' gathers into tile
 * buffers of their own, no context (radius_run).  dbscan: the same distance
 * kernels with the resident blocks as their own query tiles, a count and a
 * link pass and O(m) kernels around them, no tile, no context (dbscan_run).  The
 * knn_block_* operations are in knn_blocks.c; what a failed call leaves behind
 * is swept on a CPU by tests/index_trace.
 */
#include "knn_internal.h"
#include "knn_buf.h"
#include "knn_remove_plan.h"
#include "knn_update_plan.h"
#include "knn_neighbours_plan.h"
#include "knn_radius_plan.h"

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
#define META_BYTES (KNN_META_DOUBLES * sizeof(double))

/* the per-block host arrays: each contiguous (knn_ctx_step_n takes them as
 * arrays), cbase behind cnc in one allocation, chm 8 doubles a block */
typedef struct {
    void **blk, **s8;
    size_t *cnc, *cbase;
    double *chm;   /* the blocks' meta as read back */
} blocks_t;

struct knn_index {
    int dtype;
    size_t m, n;
    /* the corpus: nblk blocks of capacity cap; b.s8[] only when have_s8 */
    size_t cap, nblk;
    size_t nalloc;                    /* entries of the per-block arrays (>= nblk: knn_index_add grows them) */
    blocks_t b;
    int have_s8;
    double cmeta[KNN_META_DOUBLES];   /* host copy of the corpus's reduced meta */
    /* every byte of device memory the index holds between calls, the
     * context's aside (kept by knn_buf_alloc / knn_buf_release alone) */
    size_t dev_bytes;
    double *labels;
    size_t lab_cap;                   /* doubles allocated at labels (>= last_id: labels are indexed by id) */
    /* d_labels: the labels' device copy, made by the first classify call
     * (labels_sync); entries lab_lo .. lab_hi-1 of it are stale, marked by add
     * and update and uploaded by the next classify call */
    knn_buf_t d_labels;
    size_t lab_lo, lab_hi;
    /* ids: row p (0-based position in the blocks) has the 1-based id ids[p],
     * ascending.  NULL until the first removal: the id is then p + 1 and
     * last_id == m.  d_ids: its device copy, of ids_cap() entries (the host
     * array has at least as many). */
    size_t last_id;
    int32_t *ids;
    knn_buf_t d_ids;
    /* kept between queries: the context (for k, tile_cap query rows), ntile
     * tile buffers of capacity tile_cap (byte forms allocated on first use),
     * the records of a host-out call, the reduced meta, the span's events */
    knn_ctx_t *ctx;
    int k;
    size_t tile_cap, ntile;
    void **tblk, **ts8;
    double *thm;                      /* the tiles' meta as read back */
    knn_buf_t d_out;
    knn_buf_t d_meta;                 /* the reduced meta of the batch on the device ... */
    double *red;                      /* ... and its pinned host copy */
    hipEvent_t e0, e1;
    int last_bits;
    /* the radius calls' own (no context goes with them, and the kept one
     * stays as it is): rt_n tile buffers of capacity rt_cap, and d_rad: the
     * offsets, the counters or cursors and the mismatch flag of a call */
    size_t rt_cap, rt_n;
    void **rtblk, **rts8;
    double *rthm;
    knn_buf_t d_rad;
    /* knn_index_dbscan's own: its O(m) arrays and the element path's table */
    knn_buf_t d_dbs;
};

/* a batch of mq queries: ntile tiles of tcap rows */
typedef struct {
    size_t mq, tcap, ntile;
} batch_t;

static int dtype_ok(int dtype) { return dtype == KNN_F64 || dtype == KNN_F32; }
static int layout_ok(int layout) { return layout == KNN_COLMAJOR || layout == KNN_ROWMAJOR; }
static int k_max(int dtype) { return dtype == KNN_F32 ? KNN_MAX_K_F32 : KNN_MAX_K; }

static int ids_ok(const knn_index_t *ix, const int32_t *ids, size_t count)
{
    for (size_t i = 0; i < count; i++)
        if (ids[i] < 1 || (size_t)ids[i] > ix->last_id) return 0;
    return 1;
}

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

static int stream_wait(void) { return hipStreamSynchronize(NULL) == hipSuccess ? KNN_OK : KNN_ERR_HIP; }

static void blocks_free_arrays(blocks_t *b)
{
    free(b->blk);
    free(b->s8);
    free(b->cnc);
    free(b->chm);
    memset(b, 0, sizeof(*b));
}

/* arrays for na blocks, zeroed; all or nothing */
static int blocks_alloc(blocks_t *b, size_t na)
{
    b->blk = (void **)calloc(na, sizeof(void *));
    b->s8 = (void **)calloc(na, sizeof(void *));
    b->cnc = (size_t *)calloc(2 * na, sizeof(size_t));
    b->chm = (double *)calloc(na * KNN_META_DOUBLES, sizeof(double));
    if (!b->blk || !b->s8 || !b->cnc || !b->chm) {
        blocks_free_arrays(b);
        return KNN_ERR_NOMEM;
    }
    b->cbase = b->cnc + na;
    return KNN_OK;
}

/* ---- the index's device memory (dev_bytes) ------------------------------- */

/* at least `need` bytes in b; what it held is gone when it grows */
static int own_grow(knn_index_t *ix, knn_buf_t *b, size_t need)
{
    if (need <= b->bytes) return KNN_OK;
    knn_buf_release(&ix->dev_bytes, b);
    return knn_buf_alloc(&ix->dev_bytes, b, need);
}

/* b anew with `bytes` bytes, the first `keep` of them uploaded from the host
 * copy; the old memory goes once the new one is filled.  All or nothing. */
static int own_grow_keep(knn_index_t *ix, knn_buf_t *b, size_t bytes, const void *host, size_t keep)
{
    knn_buf_t nb = {0};
    RCHK(knn_buf_alloc(&ix->dev_bytes, &nb, bytes));
    if (hipMemcpy(nb.p, host, keep, hipMemcpyHostToDevice) != hipSuccess) {
        knn_buf_release(&ix->dev_bytes, &nb);
        return KNN_ERR_HIP;
    }
    knn_buf_release(&ix->dev_bytes, b);
    *b = nb;
    return KNN_OK;
}

/* one image of a block or tile of capacity cap: elements and norms, or bytes */
static size_t image_bytes(const knn_index_t *ix, size_t cap, int s8)
{
    return s8 ? knn_s8_bytes(cap, ix->n) : knn_block_bytes_dt(cap, ix->n, ix->dtype);
}

/* *p: that image's memory, where it has none yet */
static int image_alloc(knn_index_t *ix, void **p, size_t cap, int s8)
{
    knn_buf_t b = {0};
    if (*p) return KNN_OK;
    RCHK(knn_buf_alloc(&ix->dev_bytes, &b, image_bytes(ix, cap, s8)));
    *p = b.p;
    return KNN_OK;
}

/* the device memory of buffers b0 .. b1-1 of capacity cap: both images, or
 * the one whose array is given */
static void images_release(knn_index_t *ix, void **blk, void **s8, size_t cap, size_t b0, size_t b1)
{
    for (size_t b = b0; b < b1; b++)
        for (int i = 0; i < 2; i++) {
            void **a = i ? s8 : blk;
            if (!a || !a[b]) continue;
            knn_buf_t t = {a[b], image_bytes(ix, cap, i)};
            knn_buf_release(&ix->dev_bytes, &t);
            a[b] = NULL;
        }
}

/* Per-call scratch -- an uploaded source, id and position lists, the vote's
 * buffer: not counted, and freed (scratch_free; NULL is fine) on every exit of
 * the call that made it. */
static int scratch(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? KNN_OK : KNN_ERR_NOMEM; }
static void scratch_free(void *p) { hipFree(p); }

static int upload(void *dst, const void *src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

static size_t ids_cap(const knn_index_t *ix) { return ix->d_ids.bytes / sizeof(int32_t); }

/* cnc / cbase of the nblk blocks that hold m rows */
static void set_counts(knn_index_t *ix)
{
    for (size_t b = 0; b < ix->nblk; b++) {
        ix->b.cbase[b] = b * ix->cap;
        ix->b.cnc[b] = ix->m - ix->b.cbase[b] < ix->cap ? ix->m - ix->b.cbase[b] : ix->cap;
    }
}

/* a value outside the byte image arrived: the element path from now on */
static void drop_s8(knn_index_t *ix)
{
    images_release(ix, NULL, ix->b.s8, ix->cap, 0, ix->nblk);
    ix->have_s8 = 0;
}

/* Fresh buffers for rebuilt blocks b0 .. b1-1 of capacity cap, into blk[] and
 * (where the index has byte blocks) s8[]: the element image zeroed, the byte
 * image when zero_s8.  On failure the caller releases what was made. */
static int fresh_blocks(knn_index_t *ix, size_t cap, size_t b0, size_t b1, void **blk, void **s8, int zero_s8)
{
    for (size_t b = b0; b < b1; b++) {
        RCHK(image_alloc(ix, &blk[b], cap, 0));
        if (hipMemsetAsync(blk[b], 0, image_bytes(ix, cap, 0), NULL) != hipSuccess) return KNN_ERR_HIP;
        if (!ix->have_s8) continue;
        RCHK(image_alloc(ix, &s8[b], cap, 1));
        if (zero_s8 && hipMemsetAsync(s8[b], 0, image_bytes(ix, cap, 1), NULL) != hipSuccess) return KNN_ERR_HIP;
    }
    return KNN_OK;
}

/* A rebuilt block's trailing meta words at `at`: hm, its word KNN_META_S8 0
 * (an element block) or 1 (a byte block).  No search reads a corpus block's
 * trailing meta, but a later append takes its atomicMax into it.  stage: 8
 * doubles of the caller's that live until its wait. */
static int write_meta_words(void *at, const double *hm, int s8, double *stage)
{
    memcpy(stage, hm, META_BYTES);
    stage[KNN_META_S8] = s8;
    return hipMemcpyAsync(at, stage, META_BYTES, hipMemcpyHostToDevice, NULL) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

/* an element block's meta words on their way to the host (NULL stream, no wait) */
static int read_meta(const knn_index_t *ix, const void *blk, size_t cap, double *dst)
{
    const char *at = (const char *)blk + knn_block_meta_offset_dt(cap, ix->n, ix->dtype);
    return hipMemcpyAsync(dst, at, META_BYTES, hipMemcpyDeviceToHost, NULL) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

/* red = max(red, every buffer's meta) word by word */
static void meta_max(double *red, const double *hm, size_t nb)
{
    for (size_t b = 0; b < nb; b++)
        for (int j = 0; j < KNN_META_DOUBLES; j++)
            if (hm[b * KNN_META_DOUBLES + j] > red[j]) red[j] = hm[b * KNN_META_DOUBLES + j];
}

/* red = max(the corpus meta, nb buffers' meta at hm), and on its way to
 * d_meta (red is pinned, and its last reader done with the call before this
 * one: the copy is enqueued without a wait for what is in front of it) */
static int put_meta(knn_index_t *ix, const double *hm, size_t nb)
{
    memcpy(ix->red, ix->cmeta, META_BYTES);
    meta_max(ix->red, hm, nb);
    return hipMemcpyAsync(ix->d_meta.p, ix->red, META_BYTES, hipMemcpyHostToDevice, NULL) == hipSuccess ? KNN_OK
                                                                                                        : KNN_ERR_HIP;
}

/* a caller's array on the device: X itself under KNN_INDEX_DEVICE_SRC, else
 * an uploaded copy (zero-initialize; dev_src_free on every exit) */
typedef struct {
    const void *src;
    void *own;
} dev_src_t;

static int dev_src(dev_src_t *d, const void *X, size_t bytes, int flags)
{
    d->src = X;
    if (flags & KNN_INDEX_DEVICE_SRC) return KNN_OK;
    RCHK(scratch(&d->own, bytes));
    d->src = d->own;
    return upload(d->own, X, bytes);
}

static void dev_src_free(dev_src_t *d) { scratch_free(d->own); }

static void free_query_state(knn_index_t *ix)
{
    images_release(ix, ix->tblk, ix->ts8, ix->tile_cap, 0, ix->ntile);
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
    if (ix->b.blk) images_release(ix, ix->b.blk, ix->b.s8, ix->cap, 0, ix->nblk);
    knn_buf_release(&ix->dev_bytes, &ix->d_out);
    knn_buf_release(&ix->dev_bytes, &ix->d_meta);
    knn_buf_release(&ix->dev_bytes, &ix->d_ids);
    knn_buf_release(&ix->dev_bytes, &ix->d_labels);
    if (ix->rt_n) images_release(ix, ix->rtblk, ix->rts8, ix->rt_cap, 0, ix->rt_n);
    if (ix->d_rad.p) knn_buf_release(&ix->dev_bytes, &ix->d_rad);
    if (ix->d_dbs.p) knn_buf_release(&ix->dev_bytes, &ix->d_dbs);
    free(ix->rtblk);
    free(ix->rts8);
    free(ix->rthm);
    free(ix->ids);
    if (ix->red) hipHostFree(ix->red);
    if (ix->e0) hipEventDestroy(ix->e0);
    if (ix->e1) hipEventDestroy(ix->e1);
    blocks_free_arrays(&ix->b);
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
    int rc = blocks_alloc(&ix->b, ix->nblk);
    if (!rc && (own_grow(ix, &ix->d_meta, META_BYTES) ||
                hipHostMalloc((void **)&ix->red, META_BYTES, hipHostMallocDefault) != hipSuccess))
        rc = KNN_ERR_NOMEM;
    if (!rc && (hipEventCreate(&ix->e0) != hipSuccess || hipEventCreate(&ix->e1) != hipSuccess)) rc = KNN_ERR_HIP;
    if (rc) {
        index_free(ix);
        return rc;
    }
    *out = ix;
    return KNN_OK;
}

/* the per-block arrays for at least nb blocks, their nblk entries kept */
static int index_grow_arrays(knn_index_t *ix, size_t nb)
{
    if (nb <= ix->nalloc) return KNN_OK;
    const size_t na = 2 * ix->nalloc > nb ? 2 * ix->nalloc : nb;
    blocks_t g;
    RCHK(blocks_alloc(&g, na));
    memcpy(g.blk, ix->b.blk, ix->nblk * sizeof(void *));
    memcpy(g.s8, ix->b.s8, ix->nblk * sizeof(void *));
    memcpy(g.cnc, ix->b.cnc, ix->nblk * sizeof(size_t));
    memcpy(g.cbase, ix->b.cbase, ix->nblk * sizeof(size_t));
    memcpy(g.chm, ix->b.chm, ix->nblk * META_BYTES);
    blocks_free_arrays(&ix->b);
    ix->b = g;
    ix->nalloc = na;
    return KNN_OK;
}

/* the id map (host and device) for at least `need` entries, its m entries kept */
static int index_ids_reserve(knn_index_t *ix, size_t need)
{
    if (need <= ids_cap(ix)) return KNN_OK;
    const size_t nc = 2 * ids_cap(ix) > need ? 2 * ids_cap(ix) : need;
    int32_t *h = (int32_t *)realloc(ix->ids, nc * sizeof(int32_t));
    if (!h) return KNN_ERR_NOMEM;
    ix->ids = h;   /* (the same entries, whatever follows) */
    return own_grow_keep(ix, &ix->d_ids, nc * sizeof(int32_t), h, ix->m * sizeof(int32_t));
}

/* the index's own record buffer, for cnt records */
static int index_out(knn_index_t *ix, size_t cnt) { return own_grow(ix, &ix->d_out, cnt * sizeof(knn_neighbour_t)); }

/* Pack rows r0.. of a `tot`-row device source into nb buffers of capacity bc
 * (buffer b: rows r0 = b * step ..), element blocks (s8 = 0; their meta
 * words gathered behind each pack into hm, 8 doubles a buffer) or byte
 * blocks (s8 = 1).  All on the NULL stream, no wait. */
static int pack_rows(const knn_index_t *ix, void *const *buf, size_t nb, size_t bc, size_t step, const void *d_src,
                     size_t tot, int layout, int src_dtype, int s8, double *hm)
{
    const size_t es = knn_src_esize(src_dtype), n = ix->n;
    for (size_t b = 0; b < nb; b++) {
        const size_t r0 = b * step, rows = tot - r0 < step ? tot - r0 : step;
        const char *src = (const char *)d_src + (layout == KNN_COLMAJOR ? r0 : r0 * n) * es;
        const size_t ld = layout == KNN_COLMAJOR ? tot : n;
        if (s8) {
            RCHK(knn_block_pack_s8(buf[b], ix->dtype, bc, rows, n, src, src_dtype, ld, layout, NULL));
            continue;
        }
        RCHK(knn_block_pack_dt(buf[b], ix->dtype, bc, rows, n, src, src_dtype, ld, layout, NULL));
        RCHK(read_meta(ix, buf[b], bc, hm + b * KNN_META_DOUBLES));
    }
    return KNN_OK;
}

/* the element blocks' memory (knn_query: ahead of its span) */
static int index_alloc_blocks(knn_index_t *ix)
{
    set_counts(ix);
    for (size_t b = 0; b < ix->nblk; b++) RCHK(image_alloc(ix, &ix->b.blk[b], ix->cap, 0));
    return KNN_OK;
}

/* The resident corpus blocks from the device source d_X, in two parts around
 * one wait for the NULL stream (knn_query shares that wait with its queries'
 * part): the element packs and their meta on their way to the host ... */
static int build_pack(knn_index_t *ix, const void *d_X, int layout, int src_dtype)
{
    RCHK(index_alloc_blocks(ix));
    return pack_rows(ix, ix->b.blk, ix->nblk, ix->cap, ix->cap, d_X, ix->m, layout, src_dtype, 0, ix->b.chm);
}

/* ... and, the meta arrived: its reduction, and for 8-bit data the byte blocks
 * straight from the source (knn_block_pack_s8), resident for every search and
 * re-search */
static int build_finish(knn_index_t *ix, const void *d_X, int layout, int src_dtype, const double *batch_hm,
                        size_t batch_n)
{
    memset(ix->cmeta, 0, sizeof(ix->cmeta));   /* (every meta word is >= 0) */
    meta_max(ix->cmeta, ix->b.chm, ix->nblk);
    /* knn_query knows its only batch already (batch_hm: its tiles' meta): no
     * byte blocks for a corpus whose queries will not take the byte path */
    double joint[KNN_META_DOUBLES];
    memcpy(joint, ix->cmeta, sizeof(joint));
    if (batch_hm) meta_max(joint, batch_hm, batch_n);
    ix->have_s8 = knn_s8_spec_ok(joint, ix->n, ix->dtype);
    if (!ix->have_s8) return KNN_OK;
    for (size_t b = 0; b < ix->nblk; b++) RCHK(image_alloc(ix, &ix->b.s8[b], ix->cap, 1));
    return pack_rows(ix, ix->b.s8, ix->nblk, ix->cap, ix->cap, d_X, ix->m, layout, src_dtype, 1, NULL);
}

static batch_t tile_shape(const knn_index_t *ix, size_t mq)
{
    const size_t fit = fit_rows(ix->n, ix->dtype);
    size_t t = mq < fit ? mq : fit;
    if (t > KNN_QUERY_TILE_MAX) t = KNN_QUERY_TILE_MAX;
    batch_t bt = {mq, env_rows("KNN_QUERY_TILE", t, mq), 0};
    bt.ntile = (mq + bt.tcap - 1) / bt.tcap;
    return bt;
}

/* The context and the tile buffers for the batch at k.  grow: the tile
 * capacity doubles from KNN_INDEX_TILE_MIN rows, so that a stream of varying
 * batch sizes does not reallocate every call (knn_query, one batch: the
 * capacity it needs). */
static int index_reserve(knn_index_t *ix, const batch_t *bt, int k, int grow)
{
    const size_t ntile = bt->ntile;
    if (ix->ctx && (k != ix->k || bt->tcap > ix->tile_cap)) free_query_state(ix);
    if (!ix->ctx) {
        size_t cap = grow ? (ix->tile_cap ? ix->tile_cap : KNN_INDEX_TILE_MIN) : bt->tcap;
        while (cap < bt->tcap) cap *= 2;
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
    for (size_t t = 0; t < ntile; t++) RCHK(image_alloc(ix, &ix->tblk[t], ix->tile_cap, 0));
    return KNN_OK;
}

/* the byte forms of the batch's tiles, allocated on first use */
static int reserve_ts8(knn_index_t *ix, size_t ntile)
{
    for (size_t t = 0; t < ntile; t++) RCHK(image_alloc(ix, &ix->ts8[t], ix->tile_cap, 1));
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

/* The batch's tiles against the resident blocks under the reduced meta in
 * red / d_meta, on the byte path when use_s8: tile t's records (the
 * context's k a query) to d_rec, complete on return (knn_ctx_end waits for
 * each tile's). */
static int search_tiles(knn_index_t *ix, const batch_t *bt, int use_s8, knn_neighbour_t *d_rec)
{
    for (size_t t = 0; t < bt->ntile; t++) {
        const size_t r0 = t * bt->tcap, rows = bt->mq - r0 < bt->tcap ? bt->mq - r0 : bt->tcap;
        RCHK(query_tile(ix->ctx, ix->nblk, ix->b.blk, use_s8 ? ix->b.s8 : NULL, ix->b.cnc, ix->b.cbase, ix->tblk[t],
                        use_s8 ? ix->ts8[t] : NULL, ix->tile_cap, rows, ix->m + r0, (const double *)ix->d_meta.p, ix->red,
                        d_rec + r0 * (size_t)ix->k));
    }
    ix->last_bits = knn_ctx_contraction_bits(ix->ctx);
    return KNN_OK;
}

/* One batch against the resident blocks, its queries from the device source
 * d_Q, in two parts around one wait for the NULL stream: the tiles' element
 * packs and their meta on their way to the host (the context and the tile
 * buffers reserved by the caller) ... */
static int run_pack(knn_index_t *ix, const void *d_Q, const batch_t *bt, int layout, int src_dtype)
{
    return pack_rows(ix, ix->tblk, bt->ntile, ix->tile_cap, bt->tcap, d_Q, bt->mq, layout, src_dtype, 0, ix->thm);
}

/* ... and, the meta arrived: its MAX-reduction with the corpus's, the path
 * that allows, and the tiles' searches -- their records into d_out (device) */
static int run_finish(knn_index_t *ix, const void *d_Q, const batch_t *bt, int layout, int src_dtype, int flags,
                      knn_neighbour_t *d_out)
{
    knn_ctx_set_keep_zero(ix->ctx, (flags & KNN_QUERY_KEEP_ZERO) != 0);
    RCHK(put_meta(ix, ix->thm, bt->ntile));
    /* the byte path: the corpus has its byte blocks and the batch is 8-bit too */
    const int use_s8 = ix->have_s8 && knn_s8_spec_ok(ix->red, ix->n, ix->dtype);
    if (use_s8) {
        RCHK(reserve_ts8(ix, bt->ntile));
        RCHK(pack_rows(ix, ix->ts8, bt->ntile, ix->tile_cap, bt->tcap, d_Q, bt->mq, layout, src_dtype, 1, NULL));
    }
    return search_tiles(ix, bt, use_s8, d_out);
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

/* ---- the vote of a classify call ----------------------------------------- */

/* The labels' device copy, by id: made here at the first classify call (room
 * for lab_cap labels, as on the host), made again when the ids have outgrown
 * it, and otherwise brought up to date by what add and update marked stale.
 * In front of the span; a failure leaves the marks for the next call. */
static int labels_sync(knn_index_t *ix)
{
    if (ix->d_labels.bytes / sizeof(double) < ix->last_id)
        RCHK(own_grow_keep(ix, &ix->d_labels, ix->lab_cap * sizeof(double), ix->labels, ix->last_id * sizeof(double)));
    else if (ix->lab_lo < ix->lab_hi)
        RCHK(upload((double *)ix->d_labels.p + ix->lab_lo, ix->labels + ix->lab_lo,
                    (ix->lab_hi - ix->lab_lo) * sizeof(double)));
    ix->lab_lo = ix->lab_hi = 0;
    return KNN_OK;
}

/* A classify call's vote: its arguments (by_row: a row's own label is the
 * index's label of its id -- ids, or every live row's), and what it holds on
 * the device besides its records, in one scratch allocation: the match counter
 * (d_matches: NULL when the call counts none), the batch's own labels (d_qlab)
 * or the listed rows' ids, and pred and tally of a host-out call -- under
 * KNN_INDEX_DEVICE_OUT those two are the caller's.  An output (vote_out_t) is
 * `per` entries of `es` bytes a query: pred one int, or one double for a
 * regression; tally (to NULL: none) the nclasses ints of counts, or the
 * nclasses doubles of sums.  launch: knn_launch_vote_index, named by the
 * classify entry points alone, so that a program which links only the others
 * needs no vote kernel; predict (launch NULL): knn_launch_predict, named by
 * the classify_weighted and regress entry points alone, rule then an enum
 * knn_weights and nclasses 0 for a regression. */
typedef struct {
    void *to;        /* the caller's array: host, or device under KNN_INDEX_DEVICE_OUT */
    size_t es, per;
    void *d;         /* where the vote writes */
} vote_out_t;

typedef struct {
    int (*launch)(knn_neighbour_t *, size_t, int, int, int, const double *, size_t, const double *, const int32_t *,
                  int *, int *, unsigned long long *, void *);
    int (*predict)(knn_neighbour_t *, size_t, int, int, int, const double *, size_t, const double *, const int32_t *,
                   void *, double *, unsigned long long *, void *);
    int nclasses, rule, by_row;
    const double *qlabels;
    const int32_t *ids;
    vote_out_t pred, tally;
    size_t *matches;
    void *buf;
    unsigned long long *d_matches;
    double *d_qlab;
    const int32_t *d_own;   /* the rows' ids (by_row; NULL: q + 1, nothing was removed) */
} vote_t;

/* the bytes of an output of mq queries that the call holds or copies: none of
 * one that is absent */
static size_t vote_out_bytes(const vote_out_t *o, size_t mq) { return o->to ? mq * o->per * o->es : 0; }

/* the labels and the vote's buffer, in front of the span */
static int vote_begin(knn_index_t *ix, vote_t *v, size_t mq, int dev_out)
{
    RCHK(labels_sync(ix));
    /* 8-byte entries first, then the 4-byte ones: an output is among the
     * ones or the others by its entry size */
    const size_t nq = v->qlabels ? mq : 0, nown = v->ids ? mq : 0;
    const size_t pred_b = dev_out ? 0 : vote_out_bytes(&v->pred, mq);
    const size_t tally_b = dev_out ? 0 : vote_out_bytes(&v->tally, mq);
    const size_t p8 = v->pred.es == 8 ? pred_b : 0, t8 = v->tally.es == 8 ? tally_b : 0;
    RCHK(scratch(&v->buf,
                 sizeof(unsigned long long) + nq * sizeof(double) + nown * sizeof(int32_t) + pred_b + tally_b));
    unsigned long long *m8 = (unsigned long long *)v->buf;
    double *ql = (double *)(m8 + 1);
    char *o8 = (char *)(ql + nq);
    int32_t *i4 = (int32_t *)(o8 + p8 + t8);
    char *o4 = (char *)(i4 + nown);
    v->d_matches = v->matches && (v->qlabels || v->by_row) ? m8 : NULL;
    v->d_qlab = v->qlabels ? ql : NULL;
    v->d_own = v->ids ? i4 : v->by_row && ix->ids ? (const int32_t *)ix->d_ids.p : NULL;
    v->pred.d = dev_out ? v->pred.to : p8 ? (void *)o8 : (void *)o4;
    v->tally.d = dev_out || !v->tally.to ? v->tally.to : t8 ? (void *)(o8 + p8) : (void *)(o4 + (pred_b - p8));
    if (v->qlabels) RCHK(upload(ql, v->qlabels, mq * sizeof(double)));
    if (v->ids) RCHK(upload(i4, v->ids, mq * sizeof(int32_t)));
    return KNN_OK;
}

static int download(void *dst, const void *src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

/* The end of a search call that stands at rc, its mq x k records due in d_out:
 * positions -> ids where rows were removed (the tiles wrote k + 1 wide records
 * to d_rec != d_out: the row itself, d_pos, out of them in the same pass) and
 * the span's end; then records and labels to the host.  With a vote (v, whose
 * buffer is freed here): the vote behind the span (serial:94-98 stops its timer
 * in front of it), pred and counts to the host in front of the records, the
 * match count behind them, and a wait.  A failed call keeps no query state and
 * writes no output of a classify call: those arrive in a staging array. */
static int finish_search(knn_index_t *ix, int rc, vote_t *v, knn_neighbour_t *out, int dev_out,
                         knn_neighbour_t *d_out, const knn_neighbour_t *d_rec, const int32_t *d_pos, size_t mq, int k)
{
    const int32_t *d_ids = ix->ids ? (const int32_t *)ix->d_ids.p : NULL;
    const size_t cnt = mq * (size_t)k, out_b = !dev_out && out ? cnt * sizeof(knn_neighbour_t) : 0;
    const size_t pred_b = v && !dev_out ? vote_out_bytes(&v->pred, mq) : 0;
    const size_t counts_b = pred_b ? vote_out_bytes(&v->tally, mq) : 0;
    const double *d_labels = (const double *)ix->d_labels.p;
    unsigned long long hit = 0;
    char *stage = NULL;
    if (!rc && d_rec != d_out) rc = knn_launch_drop_self(d_out, d_rec, d_pos, mq, k, d_ids, ix->m, NULL);
    else if (!rc && d_ids) rc = knn_launch_remap_idx(d_out, cnt, d_ids, ix->m, NULL);
    if (!rc) rc = span_end(ix);
    if (!rc && v && v->launch)
        rc = v->launch(d_out, mq, k, v->nclasses, v->rule, d_labels, ix->last_id, v->d_qlab, v->d_own,
                       (int *)v->pred.d, (int *)v->tally.d, v->d_matches, NULL);
    else if (!rc && v)
        rc = v->predict(d_out, mq, k, v->nclasses, v->rule, d_labels, ix->last_id, v->d_qlab, v->d_own, v->pred.d,
                        (double *)v->tally.d, v->d_matches, NULL);
    if (!rc && pred_b && !(stage = (char *)malloc(pred_b + counts_b + out_b))) rc = KNN_ERR_NOMEM;
    if (!rc && pred_b) rc = download(stage, v->pred.d, pred_b);
    if (!rc && counts_b) rc = download(stage + pred_b, v->tally.d, counts_b);
    if (!rc && out_b) rc = download(stage ? stage + pred_b + counts_b : (char *)out, d_out, out_b);
    if (!rc && v && v->d_matches) rc = download(&hit, v->d_matches, sizeof(hit));
    if (!rc && v) rc = stream_wait();
    if (rc) {
        hipStreamSynchronize(NULL);
        free_query_state(ix);
    } else if (v) {
        if (stage) memcpy(v->pred.to, stage, pred_b);
        if (counts_b) memcpy(v->tally.to, stage + pred_b, counts_b);
        if (stage && out_b) memcpy(out, stage + pred_b + counts_b, out_b);
        if (v->matches) *v->matches = (size_t)hit;
    } else if (out_b && ix->labels) {
        fill_labels(out, cnt, ix->labels);
    }
    free(stage);
    if (v) scratch_free(v->buf);
    return rc;
}

int knn_index_create(knn_index_t **index, const void *X, size_t m, size_t n, int layout, int src_dtype,
                     const double *labels, int dtype, int flags)
{
    if (!index || !X || m == 0 || n == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype) || !dtype_ok(dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
    if (flags & ~KNN_INDEX_DEVICE_SRC) return KNN_ERR_INVALID;
    if (m > 0x7fffffffULL || n > 0x7fffffffULL) return KNN_ERR_INVALID;
    knn_index_t *ix = NULL;
    RCHK(index_alloc(&ix, m, n, dtype));
    int rc = KNN_OK;
    dev_src_t x = {0};
    if (labels) {
        ix->labels = (double *)malloc(m * sizeof(double));
        ix->lab_cap = m;
        if (ix->labels) memcpy(ix->labels, labels, m * sizeof(double));
        else rc = KNN_ERR_NOMEM;
    }
    if (!rc) rc = dev_src(&x, X, m * n * knn_src_esize(src_dtype), flags);
    if (!rc) rc = build_pack(ix, x.src, layout, src_dtype);
    if (!rc) rc = stream_wait();
    if (!rc) rc = build_finish(ix, x.src, layout, src_dtype, NULL, 0);
    /* the packs have read the source before the index is handed out */
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    dev_src_free(&x);
    if (rc) {
        index_free(ix);
        return rc;
    }
    *index = ix;
    return KNN_OK;
}

/* what knn_index_query refuses before any device call (its caller: a NULL out) */
static int query_check(const knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int flags)
{
    if (!ix || !Q || mq == 0 || k <= 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (k > k_max(ix->dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
    if (flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_SRC | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    return KNN_OK;
}

/* knn_index_query from its reservations through the last tile's search: the
 * records go to dst (device), or to the index's own buffer (dst NULL), *d_out.
 * The caller ends the call (finish_search) and frees *q, whatever is returned
 * here. */
static int query_search(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int flags,
                        knn_neighbour_t *dst, dev_src_t *q, knn_neighbour_t **d_out)
{
    const batch_t bt = tile_shape(ix, mq);
    int rc = dst ? KNN_OK : index_out(ix, mq * (size_t)k);
    if (!rc) rc = dev_src(q, Q, mq * ix->n * knn_src_esize(src_dtype), flags);
    if (!rc) rc = index_reserve(ix, &bt, k, 1);
    *d_out = dst ? dst : (knn_neighbour_t *)ix->d_out.p;
    if (!rc) {
        hipEventRecord(ix->e0, NULL);
        rc = run_pack(ix, q->src, &bt, layout, src_dtype);
        if (!rc) rc = stream_wait();
        if (!rc) rc = run_finish(ix, q->src, &bt, layout, src_dtype, flags, *d_out);
    }
    return rc;
}

/* knn_index_query, and with a vote (v) knn_index_classify: the labels and the
 * vote's buffers in front of the span, the same call, the vote behind it */
static int query_call(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int flags, vote_t *v,
                      knn_neighbour_t *out)
{
    if (hipSetDevice(0) != hipSuccess) return KNN_ERR_HIP;
    const int dev_out = (flags & KNN_INDEX_DEVICE_OUT) != 0;
    dev_src_t q = {0};
    knn_neighbour_t *d_out = NULL;
    int rc = v ? vote_begin(ix, v, mq, dev_out) : KNN_OK;
    if (!rc) rc = query_search(ix, Q, mq, layout, src_dtype, k, flags, dev_out ? out : NULL, &q, &d_out);
    rc = finish_search(ix, rc, v, out, dev_out, d_out, d_out, NULL, mq, k);
    dev_src_free(&q);
    return rc;
}

int knn_index_query(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int flags,
                    knn_neighbour_t *out)
{
    if (!out) return KNN_ERR_INVALID;
    RCHK(query_check(ix, Q, mq, layout, src_dtype, k, flags));
    return query_call(ix, Q, mq, layout, src_dtype, k, flags, NULL, out);
}

static int vote_check(const knn_index_t *ix, const int *pred, int nclasses, int vote_rule)
{
    if (!ix || !pred || !ix->labels || nclasses <= 0) return KNN_ERR_INVALID;
    if (vote_rule != KNN_VOTE_SERIAL && vote_rule != KNN_VOTE_MPI && vote_rule != KNN_VOTE_MAJORITY)
        return KNN_ERR_INVALID;
    return nclasses > KNN_VOTE_MAX_CLASSES ? KNN_ERR_UNSUPPORTED : KNN_OK;
}

int knn_index_classify(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int nclasses,
                       int vote_rule, int flags, const double *qlabels, int *pred, int *counts, size_t *matches,
                       knn_neighbour_t *out)
{
    RCHK(vote_check(ix, pred, nclasses, vote_rule));
    RCHK(query_check(ix, Q, mq, layout, src_dtype, k, flags));
    vote_t v = {.launch = knn_launch_vote_index, .nclasses = nclasses, .rule = vote_rule, .qlabels = qlabels,
                .pred = {pred, sizeof(int), 1, NULL}, .tally = {counts, sizeof(int), (size_t)nclasses, NULL},
                .matches = matches};
    return query_call(ix, Q, mq, layout, src_dtype, k, flags, &v, out);
}

/* what the weighted vote and the regression refuse on top of their search's
 * checks (nclasses 0: a regression, which has no class checks) */
static int predict_check(const knn_index_t *ix, const void *pred, int nclasses, int weights, int regress)
{
    if (!ix || !pred || !ix->labels) return KNN_ERR_INVALID;
    if (weights != KNN_WEIGHT_UNIFORM && weights != KNN_WEIGHT_DISTANCE) return KNN_ERR_INVALID;
    if (regress) return KNN_OK;
    if (nclasses <= 0) return KNN_ERR_INVALID;
    return nclasses > KNN_VOTE_MAX_CLASSES ? KNN_ERR_UNSUPPORTED : KNN_OK;
}

int knn_index_classify_weighted(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k,
                                int nclasses, int weights, int flags, const double *qlabels, int *pred, double *sums,
                                size_t *matches, knn_neighbour_t *out)
{
    RCHK(predict_check(ix, pred, nclasses, weights, 0));
    RCHK(query_check(ix, Q, mq, layout, src_dtype, k, flags));
    vote_t v = {.predict = knn_launch_predict, .nclasses = nclasses, .rule = weights, .qlabels = qlabels,
                .pred = {pred, sizeof(int), 1, NULL}, .tally = {sums, sizeof(double), (size_t)nclasses, NULL},
                .matches = matches};
    return query_call(ix, Q, mq, layout, src_dtype, k, flags, &v, out);
}

int knn_index_regress(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, int k, int weights,
                      int flags, double *pred, knn_neighbour_t *out)
{
    RCHK(predict_check(ix, pred, 0, weights, 1));
    RCHK(query_check(ix, Q, mq, layout, src_dtype, k, flags));
    vote_t v = {.predict = knn_launch_predict, .rule = weights, .pred = {pred, sizeof(double), 1, NULL}};
    return query_call(ix, Q, mq, layout, src_dtype, k, flags, &v, out);
}

/* ------------------------------------------------------------------ add */

/* The corpus in blocks of capacity ncap (> cap): element rows and norms move
 * device to device, a new block's meta is the max of the blocks merged into
 * it, and the byte blocks are converted again from the new element blocks
 * (knn_launch_shadow8 with the corpus meta: for knn_s8_spec_ok data the image
 * the source pack writes on every corpus row; rows past a block's nc are not
 * searched).  Old and new blocks are resident together until the last copy is
 * done.  All or nothing. */
static int index_reblock(knn_index_t *ix, size_t ncap)
{
    const size_t n = ix->n, es = knn_esize(ix->dtype), np = knn_n_pad_dt(n, ix->dtype);
    const size_t nb = (ix->m + ncap - 1) / ncap;
    const size_t orp = knn_rows_pad(ix->cap), nrp = knn_rows_pad(ncap);
    blocks_t g = {0};
    double *stage = (double *)calloc(2 * nb * KNN_META_DOUBLES, sizeof(double));   /* until the wait */
    int rc = stage ? blocks_alloc(&g, nb) : KNN_ERR_NOMEM;
    if (!rc) rc = fresh_blocks(ix, ncap, 0, nb, g.blk, g.s8, 0);
    /* runs of rows that lie in one old and one new block */
    for (size_t r = 0; r < ix->m && !rc;) {
        const size_t ob = r / ix->cap, oo = r % ix->cap, b = r / ncap, no = r % ncap;
        const size_t len = ix->b.cnc[ob] - oo < ncap - no ? ix->b.cnc[ob] - oo : ncap - no;
        const char *src = (const char *)ix->b.blk[ob];
        char *dst = (char *)g.blk[b];
        if (hipMemcpyAsync(dst + no * np * es, src + oo * np * es, len * np * es, hipMemcpyDeviceToDevice, NULL) !=
                hipSuccess ||
            hipMemcpyAsync(dst + (nrp * np + no) * es, src + (orp * np + oo) * es, len * es, hipMemcpyDeviceToDevice,
                           NULL) != hipSuccess)
            rc = KNN_ERR_HIP;
        meta_max(g.chm + b * KNN_META_DOUBLES, ix->b.chm + ob * KNN_META_DOUBLES, 1);
        r += len;
    }
    if (!rc && ix->have_s8) rc = put_meta(ix, NULL, 0);
    for (size_t b = 0; b < nb && !rc; b++) {
        const double *hm = g.chm + b * KNN_META_DOUBLES;
        double *st = stage + 2 * b * KNN_META_DOUBLES;
        rc = write_meta_words((char *)g.blk[b] + knn_block_meta_offset_dt(ncap, n, ix->dtype), hm, 0, st);
        if (rc || !ix->have_s8) continue;
        rc = knn_launch_shadow8(g.s8[b], g.blk[b], ix->dtype, nrp, n, (const double *)ix->d_meta.p, NULL);
        if (!rc) rc = write_meta_words((char *)g.s8[b] + knn_s8_meta_offset(ncap, n), hm, 1, st + KNN_META_DOUBLES);
    }
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    free(stage);
    if (rc) {
        if (g.blk) images_release(ix, g.blk, g.s8, ncap, 0, nb);
        blocks_free_arrays(&g);
        return rc;
    }
    /* commit; the context was made for the old capacity */
    free_query_state(ix);
    images_release(ix, ix->b.blk, ix->b.s8, ix->cap, 0, ix->nblk);
    blocks_free_arrays(&ix->b);
    ix->b = g;
    ix->cap = ncap;
    ix->nblk = ix->nalloc = nb;
    set_counts(ix);
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
            RCHK(image_alloc(ix, &buf[b], cap, s8));
            RCHK(s8 ? knn_block_pack_s8(buf[b], ix->dtype, cap, len, n, src, src_dtype, ld, layout, NULL)
                    : knn_block_pack_dt(buf[b], ix->dtype, cap, len, n, src, src_dtype, ld, layout, NULL));
        }
        if (!s8) RCHK(read_meta(ix, buf[b], cap, ix->b.chm + b * KNN_META_DOUBLES));
        r += len;
    }
    return KNN_OK;
}

/* A write into resident blocks (add, update) in build_pack / build_finish's two
 * parts: element rows and the touched blocks' meta, one wait, s8_stays of the
 * candidate corpus meta, the byte rows where it does, a wait, commit_meta. */
static int s8_stays(const knn_index_t *ix, const double *cmeta)
{
    return ix->have_s8 && knn_s8_spec_ok(cmeta, ix->n, ix->dtype);
}

static void commit_meta(knn_index_t *ix, const double *cmeta, int keep_s8)
{
    if (ix->have_s8 && !keep_s8) drop_s8(ix);
    memcpy(ix->cmeta, cmeta, META_BYTES);
}

/* labels lo .. hi-1 (0-based: id - 1) changed on the host: the device copy's
 * stale range grows to hold them (a host flag; labels_sync uploads) */
static void labels_stale(knn_index_t *ix, size_t lo, size_t hi)
{
    if (ix->lab_lo == ix->lab_hi) {
        ix->lab_lo = lo;
        ix->lab_hi = hi;
        return;
    }
    if (lo < ix->lab_lo) ix->lab_lo = lo;
    if (hi > ix->lab_hi) ix->lab_hi = hi;
}

int knn_index_add(knn_index_t *ix, const void *X, size_t rows, int layout, int src_dtype, const double *labels,
                  int flags)
{
    if (!ix || !X || rows == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
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
    const size_t nb0 = ix->nblk, nb1 = (m1 + ix->cap - 1) / ix->cap, bf = ix->m / ix->cap;   /* bf: the first touched */
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
    dev_src_t x = {0};
    double cmeta[KNN_META_DOUBLES];
    memcpy(cmeta, ix->cmeta, sizeof(cmeta));
    int keep_s8 = 0;
    int rc = dev_src(&x, X, rows * ix->n * knn_src_esize(src_dtype), flags);
    if (!rc) rc = add_rows(ix, ix->b.blk, x.src, rows, layout, src_dtype, 0);
    if (!rc) rc = stream_wait();
    if (!rc) {
        meta_max(cmeta, ix->b.chm + bf * KNN_META_DOUBLES, nb1 - bf);
        keep_s8 = s8_stays(ix, cmeta);
        if (keep_s8) rc = add_rows(ix, ix->b.s8, x.src, rows, layout, src_dtype, 1);
    }
    /* the new rows' ids last_id + 1 .. behind the live ones (entries past m
     * are read by nothing until m is committed below) */
    if (!rc && ix->ids) {
        for (size_t r = 0; r < rows; r++) ix->ids[ix->m + r] = (int32_t)(ix->last_id + 1 + r);
        if (hipMemcpyAsync((int32_t *)ix->d_ids.p + ix->m, ix->ids + ix->m, rows * sizeof(int32_t),
                           hipMemcpyHostToDevice, NULL) != hipSuccess)
            rc = KNN_ERR_HIP;
    }
    /* the packs have read the source before the call returns */
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    dev_src_free(&x);
    if (rc) {
        /* rows written past a block's nc are never read, and its meta only grew */
        images_release(ix, ix->b.blk, ix->b.s8, ix->cap, nb0, nb1);
        return rc;
    }
    commit_meta(ix, cmeta, keep_s8);
    if (labels) {
        memcpy(ix->labels + ix->last_id, labels, rows * sizeof(double));
        labels_stale(ix, ix->last_id, id1);
    }
    ix->nblk = nb1;
    ix->m = m1;
    ix->last_id = id1;
    set_counts(ix);
    return KNN_OK;
}

/* --------------------------------------------------------------- remove */

/* The device side of a plan that moves rows: every block from pl->b0 on is
 * built again in a fresh, zeroed buffer by one gather a run (and one of the
 * byte rows where the index has byte blocks), its meta the max of the blocks
 * it drew from.  Old and new buffers are resident together until the one wait
 * at the end; on success the new ones are in g (entries b0 .. nb1-1), on
 * failure everything made here is freed. */
static int remove_move(knn_index_t *ix, const knn_rm_plan_t *pl, blocks_t *g)
{
    const size_t n = ix->n, cap = ix->cap, b0 = pl->b0, nb1 = pl->nb1;
    int32_t *d_list = NULL;
    double *stage = (double *)calloc(2 * (nb1 - b0) * KNN_META_DOUBLES, sizeof(double));   /* until the wait */
    int rc = stage ? fresh_blocks(ix, cap, b0, nb1, g->blk, g->s8, 1) : KNN_ERR_NOMEM;
    /* the runs' lists, one array */
    if (!rc) rc = scratch((void **)&d_list, pl->nlist * sizeof(int32_t));
    if (!rc && hipMemcpyAsync(d_list, pl->list, pl->nlist * sizeof(int32_t), hipMemcpyHostToDevice, NULL) != hipSuccess)
        rc = KNN_ERR_HIP;
    for (size_t r = 0; r < pl->nruns && !rc; r++) {
        const knn_rm_run_t *run = &pl->runs[r];
        rc = knn_block_gather_dt(g->blk[run->nb], cap, run->dst0, ix->b.blk[run->ob], cap, d_list + run->list0,
                                 run->rows, n, ix->dtype, NULL);
        if (!rc && ix->have_s8)
            rc = knn_block_gather_s8(g->s8[run->nb], cap, run->dst0, ix->b.s8[run->ob], cap, d_list + run->list0,
                                     run->rows, n, NULL);
        meta_max(g->chm + run->nb * KNN_META_DOUBLES, ix->b.chm + run->ob * KNN_META_DOUBLES, 1);
    }
    for (size_t b = b0; b < nb1 && !rc; b++) {
        const double *hm = g->chm + b * KNN_META_DOUBLES;
        double *st = stage + 2 * (b - b0) * KNN_META_DOUBLES;
        rc = write_meta_words((char *)g->blk[b] + knn_block_meta_offset_dt(cap, n, ix->dtype), hm, 0, st);
        if (!rc && ix->have_s8)
            rc = write_meta_words((char *)g->s8[b] + knn_s8_meta_offset(cap, n), hm, 1, st + KNN_META_DOUBLES);
    }
    if (!rc) rc = stream_wait();
    else hipStreamSynchronize(NULL);
    scratch_free(d_list);
    free(stage);
    if (rc) images_release(ix, g->blk, g->s8, cap, b0, nb1);
    return rc;
}

int knn_index_remove(knn_index_t *ix, const int32_t *ids, size_t count, int flags, size_t *removed)
{
    if (!ix || !ids || count == 0 || flags != 0) return KNN_ERR_INVALID;
    if (!ids_ok(ix, ids, count)) return KNN_ERR_INVALID;
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
    const size_t icap = ids_cap(ix) > pl.m1 ? ids_cap(ix) : pl.m1;
    knn_buf_t d_ids = {0};
    int32_t *h_ids = NULL;
    blocks_t g = {0};
    if (!rc) rc = blocks_alloc(&g, ix->nblk);
    if (!rc && !(h_ids = (int32_t *)malloc(icap * sizeof(int32_t)))) rc = KNN_ERR_NOMEM;
    if (!rc) rc = knn_buf_alloc(&ix->dev_bytes, &d_ids, icap * sizeof(int32_t));
    if (!rc) {
        memcpy(h_ids, pl.ids, pl.m1 * sizeof(int32_t));
        rc = upload(d_ids.p, h_ids, pl.m1 * sizeof(int32_t));
    }
    if (!rc && pl.moves) rc = remove_move(ix, &pl, &g);
    if (rc) {   /* the index answers as before the call */
        knn_buf_release(&ix->dev_bytes, &d_ids);
        free(h_ids);
    } else {
        /* commit: the moved blocks in place of the old ones, the blocks past
         * the new count released, then m, cnc, cbase, nblk and the id map.
         * cmeta stays: a MAX that has only become too large is conservative. */
        if (pl.moves) {
            images_release(ix, ix->b.blk, ix->b.s8, ix->cap, pl.b0, pl.nb1);
            for (size_t b = pl.b0; b < pl.nb1; b++) {
                ix->b.blk[b] = g.blk[b];
                ix->b.s8[b] = g.s8[b];
            }
            memcpy(ix->b.chm + pl.b0 * KNN_META_DOUBLES, g.chm + pl.b0 * KNN_META_DOUBLES,
                   (pl.nb1 - pl.b0) * META_BYTES);
        }
        images_release(ix, ix->b.blk, ix->b.s8, ix->cap, pl.nb1, ix->nblk);
        ix->m = pl.m1;
        ix->nblk = pl.nb1;
        set_counts(ix);
        knn_buf_release(&ix->dev_bytes, &ix->d_ids);
        free(ix->ids);
        ix->ids = h_ids;
        ix->d_ids = d_ids;
        if (removed) *removed = pl.removed;
    }
    blocks_free_arrays(&g);
    knn_rm_plan_free(&pl);
    return rc;
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
        void *blk = s8 ? ix->b.s8[run->blk] : ix->b.blk[run->blk];
        RCHK(s8 ? knn_block_scatter_s8(blk, ix->dtype, cap, pos, srow, run->rows, n, d_X, count, src_dtype, ld, layout,
                                       NULL)
                : knn_block_scatter_dt(blk, ix->dtype, cap, pos, srow, run->rows, n, d_X, count, src_dtype, ld, layout,
                                       NULL));
        if (!s8) RCHK(read_meta(ix, blk, cap, ix->b.chm + run->blk * KNN_META_DOUBLES));
    }
    return KNN_OK;
}

int knn_index_update(knn_index_t *ix, const int32_t *ids, size_t count, const void *X, int layout, int src_dtype,
                     const double *labels, int flags)
{
    if (!ix || !ids || !X || count == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
    if (flags & ~KNN_INDEX_DEVICE_SRC) return KNN_ERR_INVALID;
    if (count > ix->m || (labels && !ix->labels)) return KNN_ERR_INVALID;   /* (more ids than live rows: a repeat) */
    if (!ids_ok(ix, ids, count)) return KNN_ERR_INVALID;
    /* the plan, on the host alone (knn_update_plan.h) */
    knn_up_plan_t pl;
    const int prc = knn_up_plan(&pl, ix->ids, ix->m, ix->cap, ids, count);
    if (prc) return prc == KNN_UP_NOMEM ? KNN_ERR_NOMEM : KNN_ERR_INVALID;
    /* every allocation and upload in front of the first overwritten row: up
     * to there a failure leaves the index as it was */
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    dev_src_t x = {0};
    int32_t *d_list = NULL;
    if (!rc) rc = dev_src(&x, X, count * ix->n * knn_src_esize(src_dtype), flags);
    if (!rc) rc = scratch((void **)&d_list, 2 * count * sizeof(int32_t));
    if (!rc) rc = upload(d_list, pl.pos, count * sizeof(int32_t));
    if (!rc) rc = upload(d_list + count, pl.srow, count * sizeof(int32_t));
    /* From here on a failure leaves rows half written: KNN_ERR_HIP, and the
     * index is fit only for knn_index_destroy. */
    double cmeta[KNN_META_DOUBLES];
    memcpy(cmeta, ix->cmeta, sizeof(cmeta));
    int keep_s8 = 0;
    if (!rc) {
        rc = update_rows(ix, &pl, d_list, x.src, layout, src_dtype, 0);
        if (!rc) rc = stream_wait();
        if (!rc) {
            for (size_t r = 0; r < pl.nruns; r++) meta_max(cmeta, ix->b.chm + pl.runs[r].blk * KNN_META_DOUBLES, 1);
            keep_s8 = s8_stays(ix, cmeta);
            if (keep_s8) rc = update_rows(ix, &pl, d_list, x.src, layout, src_dtype, 1);
        }
        /* the scatters have read the source and the lists before the call returns */
        if (!rc) rc = stream_wait();
        else hipStreamSynchronize(NULL);
        if (rc) rc = KNN_ERR_HIP;
    }
    dev_src_free(&x);
    scratch_free(d_list);
    if (!rc) {
        commit_meta(ix, cmeta, keep_s8);
        if (labels)
            for (size_t i = 0; i < count; i++) {
                ix->labels[ids[i] - 1] = labels[i];
                labels_stale(ix, (size_t)ids[i] - 1, (size_t)ids[i]);
            }
    }
    knn_up_plan_free(&pl);
    return rc;
}

/* ----------------------------------------------------------- neighbours */

/* The query tiles of knn_index_neighbours (tblk, ts8 of capacity tile_cap: the
 * index's query tiles, or the radius calls' own): tile t's rows are the resident
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
static int gather_tiles(knn_index_t *ix, void *const *tblk, void *const *ts8, size_t tile_cap,
                        const void *const *d_tab, const int32_t *d_pos, const batch_t *bt, int s8)
{
    const size_t n = ix->n, es = knn_esize(ix->dtype), np = knn_n_pad_dt(n, ix->dtype);
    const size_t trp = knn_rows_pad(tile_cap);
    for (size_t t = 0; t < bt->ntile; t++) {
        const size_t r0 = t * bt->tcap, rows = bt->mq - r0 < bt->tcap ? bt->mq - r0 : bt->tcap;
        const size_t pad = knn_round_up(rows, KNN_TQ) - rows;   /* (round_up(rows, KNN_TQ) <= trp) */
        char *blk = (char *)tblk[t];
        RCHK(knn_block_gather_pos_dt(blk, tile_cap, 0, d_tab, ix->cap, ix->nblk, d_pos + r0, rows, n, ix->dtype,
                                     NULL));
        if (pad && (hipMemsetAsync(blk + rows * np * es, 0, pad * np * es, NULL) != hipSuccess ||
                    hipMemsetAsync(blk + (trp * np + rows) * es, 0, pad * es, NULL) != hipSuccess))
            return KNN_ERR_HIP;
        if (s8)
            RCHK(knn_block_gather_pos_s8(ts8[t], tile_cap, 0, d_tab + ix->nblk, ix->cap, ix->nblk, d_pos + r0,
                                         rows, n, NULL));
    }
    return KNN_OK;
}

/* what knn_index_neighbours refuses before any device call (its caller: a
 * NULL out) */
static int rows_check(const knn_index_t *ix, const int32_t *ids, size_t count, int k, int flags)
{
    if (!ix || k <= 0 || (ids ? count == 0 : count != 0)) return KNN_ERR_INVALID;
    if (flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    /* keep-zero: the row itself comes back among its own neighbours and is
     * taken out afterwards, so the engine searches one more */
    if (k > k_max(ix->dtype) - ((flags & KNN_QUERY_KEEP_ZERO) != 0)) return KNN_ERR_UNSUPPORTED;
    const size_t mq = ids ? count : ix->m;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    if (!ids_ok(ix, ids, count)) return KNN_ERR_INVALID;
    return KNN_OK;
}

/* what a rows call holds until its end: the rows' positions and the blocks'
 * pointers on the device; where the records are due (d_out) and where the
 * tiles write them (d_rec) */
typedef struct {
    int32_t *d_pos;
    void **d_tab;
    knn_neighbour_t *d_out, *d_rec;
} rows_t;

static void rows_free(rows_t *r)
{
    scratch_free(r->d_pos);
    scratch_free(r->d_tab);
}

/* the listed rows' positions (ids NULL: every live row's), on the host alone
 * (knn_neighbours_plan.h); KNN_ERR_INVALID for an id that is not live */
static int rows_plan(const knn_index_t *ix, const int32_t *ids, size_t count, int32_t **pos)
{
    *pos = (int32_t *)malloc((ids ? count : ix->m) * sizeof(int32_t));
    if (!*pos) return KNN_ERR_NOMEM;
    if (knn_nb_positions(ix->ids, ix->m, ids, count, *pos)) {
        free(*pos);
        return KNN_ERR_INVALID;
    }
    return KNN_OK;
}

/* knn_index_neighbours behind its plan (pos, mq positions, freed here) through
 * the last tile's search; the records are due in dst (device), or in the
 * index's own buffer (dst NULL).  The caller ends the call (finish_search) and
 * frees *r, whatever is returned here. */
static int rows_search(knn_index_t *ix, int32_t *pos, size_t mq, int k, int kz, knn_neighbour_t *dst, rows_t *r)
{
    const size_t cnt = mq * (size_t)k, wide = kz ? mq * (size_t)(k + 1) : 0;
    const batch_t bt = tile_shape(ix, mq);
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    /* every allocation and upload in front of the span: the positions, the
     * blocks' pointers (element, then byte), the records of a call without
     * dst and behind them the k + 1 wide ones of a keep-zero call */
    const int use_s8 = s8_stays(ix, ix->cmeta);
    if (!rc) rc = index_out(ix, (dst ? 0 : cnt) + wide);
    if (!rc) rc = scratch((void **)&r->d_pos, mq * sizeof(int32_t));
    if (!rc) rc = scratch((void **)&r->d_tab, 2 * ix->nblk * sizeof(void *));
    if (!rc) rc = upload(r->d_pos, pos, mq * sizeof(int32_t));
    if (!rc) rc = upload(r->d_tab, ix->b.blk, ix->nblk * sizeof(void *));
    if (!rc) rc = upload(r->d_tab + ix->nblk, ix->b.s8, ix->nblk * sizeof(void *));
    free(pos);
    if (!rc) rc = index_reserve(ix, &bt, k + kz, 1);
    if (!rc && use_s8) rc = reserve_ts8(ix, bt.ntile);
    r->d_out = dst ? dst : (knn_neighbour_t *)ix->d_out.p;
    r->d_rec = r->d_out;   /* what the tiles write */
    if (!rc && kz) r->d_rec = (knn_neighbour_t *)ix->d_out.p + (dst ? 0 : cnt);
    if (!rc) {
        hipEventRecord(ix->e0, NULL);
        /* the batch's reduced meta is the corpus's: the queries are corpus
         * rows and cmeta only grows.  No tile meta is read back, so the host
         * does not wait between the gathers and the searches. */
        rc = put_meta(ix, NULL, 0);
        if (!rc)
            rc = gather_tiles(ix, ix->tblk, ix->ts8, ix->tile_cap, (const void *const *)r->d_tab, r->d_pos, &bt, use_s8);
        knn_ctx_set_keep_zero(ix->ctx, kz);
        if (!rc) rc = search_tiles(ix, &bt, use_s8, r->d_rec);
    }
    return rc;
}

/* knn_index_neighbours, and with a vote (v) knn_index_classify_rows */
static int rows_call(knn_index_t *ix, const int32_t *ids, size_t count, int k, int flags, vote_t *v,
                     knn_neighbour_t *out)
{
    const int kz = (flags & KNN_QUERY_KEEP_ZERO) != 0, dev_out = (flags & KNN_INDEX_DEVICE_OUT) != 0;
    const size_t mq = ids ? count : ix->m;
    int32_t *pos = NULL;
    RCHK(rows_plan(ix, ids, count, &pos));
    rows_t r = {0};
    int rc = KNN_OK;
    if (v) rc = hipSetDevice(0) == hipSuccess ? vote_begin(ix, v, mq, dev_out) : KNN_ERR_HIP;
    if (!rc) rc = rows_search(ix, pos, mq, k, kz, dev_out ? out : NULL, &r);
    else free(pos);
    rc = finish_search(ix, rc, v, out, dev_out, r.d_out, r.d_rec, r.d_pos, mq, k);
    rows_free(&r);
    return rc;
}

int knn_index_neighbours(knn_index_t *ix, const int32_t *ids, size_t count, int k, int flags, knn_neighbour_t *out)
{
    if (!out) return KNN_ERR_INVALID;
    RCHK(rows_check(ix, ids, count, k, flags));
    return rows_call(ix, ids, count, k, flags, NULL, out);
}

int knn_index_classify_rows(knn_index_t *ix, const int32_t *ids, size_t count, int k, int nclasses, int vote_rule,
                            int flags, int *pred, int *counts, size_t *matches, knn_neighbour_t *out)
{
    RCHK(vote_check(ix, pred, nclasses, vote_rule));
    RCHK(rows_check(ix, ids, count, k, flags));
    vote_t v = {.launch = knn_launch_vote_index, .nclasses = nclasses, .rule = vote_rule, .by_row = 1, .ids = ids,
                .pred = {pred, sizeof(int), 1, NULL}, .tally = {counts, sizeof(int), (size_t)nclasses, NULL},
                .matches = matches};
    return rows_call(ix, ids, count, k, flags, &v, out);
}

int knn_index_classify_weighted_rows(knn_index_t *ix, const int32_t *ids, size_t count, int k, int nclasses,
                                     int weights, int flags, int *pred, double *sums, size_t *matches,
                                     knn_neighbour_t *out)
{
    RCHK(predict_check(ix, pred, nclasses, weights, 0));
    RCHK(rows_check(ix, ids, count, k, flags));
    vote_t v = {.predict = knn_launch_predict, .nclasses = nclasses, .rule = weights, .by_row = 1, .ids = ids,
                .pred = {pred, sizeof(int), 1, NULL}, .tally = {sums, sizeof(double), (size_t)nclasses, NULL},
                .matches = matches};
    return rows_call(ix, ids, count, k, flags, &v, out);
}

/* (a regression compares nothing with a row's own target: no by_row, no ids) */
int knn_index_regress_rows(knn_index_t *ix, const int32_t *ids, size_t count, int k, int weights, int flags,
                           double *pred, knn_neighbour_t *out)
{
    RCHK(predict_check(ix, pred, 0, weights, 1));
    RCHK(rows_check(ix, ids, count, k, flags));
    vote_t v = {.predict = knn_launch_predict, .rule = weights, .pred = {pred, sizeof(double), 1, NULL}};
    return rows_call(ix, ids, count, k, flags, &v, out);
}

/* --------------------------------------------------------------- radius */

/* Radius search (knn_radius.hip): which live rows lie within `radius` of each
 * query, in two calls that share everything but their last steps -- count
 * (the first distance pass: counts) and fill (the second, its hits into the
 * caller's CSR segments, then the segments' sort).  No context is involved
 * and the kept one is not touched: the calls have tile buffers of their own
 * (rtblk, rts8: filled by pack_rows / gather_tiles as query's and neighbours'
 * are) and one buffer d_rad for the offsets, the counters and the flag.  The
 * launchers are named by radius_run alone, which only the four radius entry
 * points reach. */
typedef struct {
    double radius;
    int flags, fill;
    int32_t *counts;         /* count: mq entries (device under KNN_INDEX_DEVICE_OUT) */
    const int64_t *indptr;   /* fill: mq + 1 offsets */
    knn_neighbour_t *out;    /* fill: indptr[mq] - indptr[0] records */
} radius_t;

/* what all four refuse that is not about their queries: the outputs, the
 * radius (a NaN fails both comparisons), a host indptr that decreases */
static int radius_check(const radius_t *a, size_t mq)
{
    if (a->fill ? !a->indptr || !a->out : !a->counts) return KNN_ERR_INVALID;
    if (!(a->radius >= 0.0) || !(a->radius <= 1.7976931348623157e308)) return KNN_ERR_INVALID;
    if (a->fill && !(a->flags & KNN_INDEX_DEVICE_OUT)) {
        if (a->indptr[0] < 0) return KNN_ERR_INVALID;
        for (size_t q = 0; q < mq; q++)
            if (a->indptr[q + 1] < a->indptr[q]) return KNN_ERR_INVALID;
    }
    return KNN_OK;
}

/* the calls' tile buffers for the batch: capacity doubling from
 * KNN_INDEX_TILE_MIN as index_reserve's; the byte forms when s8 */
static int radius_reserve(knn_index_t *ix, const batch_t *bt, int s8)
{
    if (bt->tcap > ix->rt_cap) {
        if (ix->rt_n) images_release(ix, ix->rtblk, ix->rts8, ix->rt_cap, 0, ix->rt_n);
        size_t cap = ix->rt_cap ? ix->rt_cap : KNN_INDEX_TILE_MIN;
        while (cap < bt->tcap) cap *= 2;
        ix->rt_cap = cap;
    }
    if (bt->ntile > ix->rt_n) {
        void **a = (void **)calloc(bt->ntile, sizeof(void *)), **b = (void **)calloc(bt->ntile, sizeof(void *));
        double *hm = (double *)calloc(bt->ntile * KNN_META_DOUBLES, sizeof(double));
        if (!a || !b || !hm) {
            free(a);
            free(b);
            free(hm);
            return KNN_ERR_NOMEM;
        }
        if (ix->rt_n) {
            memcpy(a, ix->rtblk, ix->rt_n * sizeof(void *));
            memcpy(b, ix->rts8, ix->rt_n * sizeof(void *));
        }
        free(ix->rtblk);
        free(ix->rts8);
        free(ix->rthm);
        ix->rtblk = a;
        ix->rts8 = b;
        ix->rthm = hm;
        ix->rt_n = bt->ntile;
    }
    for (size_t t = 0; t < bt->ntile; t++) {
        RCHK(image_alloc(ix, &ix->rtblk[t], ix->rt_cap, 0));
        if (s8) RCHK(image_alloc(ix, &ix->rts8[t], ix->rt_cap, 1));
    }
    return KNN_OK;
}

/* the table of one launch: the (at most KNN_RADIUS_MAXBLK) blocks from b0 on */
static void radius_table(const knn_index_t *ix, size_t b0, int use_s8, knn_radius_blocks_t *cb)
{
    memset(cb, 0, sizeof(*cb));
    cb->nblk = (int)(ix->nblk - b0 < KNN_RADIUS_MAXBLK ? ix->nblk - b0 : KNN_RADIUS_MAXBLK);
    for (int j = 0; j < cb->nblk; j++) {
        cb->ptr[j] = use_s8 ? ix->b.s8[b0 + j] : ix->b.blk[b0 + j];
        cb->base[j] = (int64_t)ix->b.cbase[b0 + j];
        cb->nc[j] = (int)ix->b.cnc[b0 + j];
    }
}

/* one pass (count or fill) of every tile against every block, KNN_RADIUS_MAXBLK
 * blocks a launch: d_cnt the counters / cursors, d_ip the offsets, d_self the
 * rows' own positions (rows forms), all by query */
static int radius_pass(const knn_index_t *ix, const batch_t *bt, int use_s8, const radius_t *a, int thr,
                       const int32_t *d_self, int32_t *d_cnt, const int64_t *d_ip, knn_neighbour_t *d_rec)
{
    const int keep0 = (a->flags & KNN_QUERY_KEEP_ZERO) != 0;
    for (size_t t = 0; t < bt->ntile; t++) {
        const size_t r0 = t * bt->tcap, rows = bt->mq - r0 < bt->tcap ? bt->mq - r0 : bt->tcap;
        for (size_t b0 = 0; b0 < ix->nblk; b0 += KNN_RADIUS_MAXBLK) {
            knn_radius_blocks_t cb;
            radius_table(ix, b0, use_s8, &cb);
            if (use_s8)
                RCHK(knn_launch_radius_i8(a->fill, ix->rts8[t], knn_rows_pad(ix->rt_cap), (int)rows,
                                          d_self ? d_self + r0 : NULL, &cb, knn_rows_pad(ix->cap), (int)ix->n, thr,
                                          keep0, d_cnt + r0, d_ip ? d_ip + r0 : NULL, d_ip, d_rec, NULL));
            else
                RCHK(knn_launch_radius_scan(a->fill, ix->dtype, ix->rtblk[t], (int)rows, d_self ? d_self + r0 : NULL,
                                            &cb, (int)ix->n, a->radius, keep0, d_cnt + r0, d_ip ? d_ip + r0 : NULL,
                                            d_ip, d_rec, NULL));
        }
    }
    return KNN_OK;
}

/* A radius call behind its checks.  Q: the query forms' source; pos: the rows
 * forms' positions (mq of them, freed here).  Every allocation and upload in
 * front of the span; the span from the pack or gather through the last kernel;
 * then the answers to the host (none under KNN_INDEX_DEVICE_OUT, the fill's
 * flag excepted: the call's status depends on it). */
static int radius_run(knn_index_t *ix, const void *Q, int32_t *pos, size_t mq, int layout, int src_dtype,
                      const radius_t *a)
{
    const int dev_out = (a->flags & KNN_INDEX_DEVICE_OUT) != 0;
    const batch_t bt = tile_shape(ix, mq);
    const size_t ip_b = (mq + 1) * sizeof(int64_t), cnt_b = mq * sizeof(int32_t);
    const size_t nrec = a->fill && !dev_out ? (size_t)(a->indptr[mq] - a->indptr[0]) : 0;
    dev_src_t q = {0};
    int32_t *d_pos = NULL;
    void **d_tab = NULL;
    int use_s8 = pos ? s8_stays(ix, ix->cmeta) : 0, flag = 0;
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    if (!rc) rc = own_grow(ix, &ix->d_rad, ip_b + cnt_b + sizeof(int32_t));
    if (!rc && nrec) rc = index_out(ix, nrec);
    /* d_rad: the offsets of a host-out fill, the call's counters or cursors,
     * the flag; under KNN_INDEX_DEVICE_OUT counts and offsets are the caller's */
    int32_t *d_own = ix->d_rad.p ? (int32_t *)((char *)ix->d_rad.p + ip_b) : NULL;
    int32_t *d_cnt = !a->fill && dev_out ? a->counts : d_own;
    int *d_flag = d_own ? (int *)(d_own + mq) : NULL;
    const int64_t *d_ip = !a->fill ? NULL : dev_out ? a->indptr : (const int64_t *)ix->d_rad.p;
    knn_neighbour_t *d_rec = dev_out ? a->out : (knn_neighbour_t *)ix->d_out.p;
    if (!rc && pos) {
        rc = scratch((void **)&d_pos, mq * sizeof(int32_t));
        if (!rc) rc = scratch((void **)&d_tab, 2 * ix->nblk * sizeof(void *));
        if (!rc) rc = upload(d_pos, pos, mq * sizeof(int32_t));
        if (!rc) rc = upload(d_tab, ix->b.blk, ix->nblk * sizeof(void *));
        if (!rc) rc = upload(d_tab + ix->nblk, ix->b.s8, ix->nblk * sizeof(void *));
    } else if (!rc) {
        rc = dev_src(&q, Q, mq * ix->n * knn_src_esize(src_dtype), a->flags);
    }
    free(pos);
    if (!rc) rc = radius_reserve(ix, &bt, use_s8);
    if (!rc && a->fill && !dev_out) rc = upload(ix->d_rad.p, a->indptr, ip_b);
    if (!rc) {
        hipEventRecord(ix->e0, NULL);
        if (hipMemsetAsync(d_cnt, 0, cnt_b, NULL) != hipSuccess ||
            (a->fill && hipMemsetAsync(d_flag, 0, sizeof(int), NULL) != hipSuccess))
            rc = KNN_ERR_HIP;
        if (!rc && d_pos) {
            /* the queries are corpus rows: the batch's meta is the corpus's */
            rc = gather_tiles(ix, ix->rtblk, ix->rts8, ix->rt_cap, (const void *const *)d_tab, d_pos, &bt, use_s8);
        } else if (!rc) {
            /* query's two parts: the element tiles and their meta, one wait,
             * the path the reduced meta allows, the byte tiles for it */
            rc = pack_rows(ix, ix->rtblk, bt.ntile, ix->rt_cap, bt.tcap, q.src, mq, layout, src_dtype, 0, ix->rthm);
            if (!rc) rc = stream_wait();
            if (!rc) {
                double red[KNN_META_DOUBLES];
                memcpy(red, ix->cmeta, META_BYTES);
                meta_max(red, ix->rthm, bt.ntile);
                use_s8 = ix->have_s8 && knn_s8_spec_ok(red, ix->n, ix->dtype);
            }
            if (!rc && use_s8) rc = radius_reserve(ix, &bt, 1);
            if (!rc && use_s8)
                rc = pack_rows(ix, ix->rts8, bt.ntile, ix->rt_cap, bt.tcap, q.src, mq, layout, src_dtype, 1, NULL);
        }
        const int thr = use_s8 ? (int)knn_radius_threshold(a->radius, knn_radius_d2max(ix->n)) : 0;
        if (!rc) rc = radius_pass(ix, &bt, use_s8, a, thr, d_pos, d_cnt, d_ip, d_rec);
        if (!rc && a->fill)
            rc = knn_launch_radius_sort(mq, d_cnt, d_ip, d_rec, ix->ids ? (const int32_t *)ix->d_ids.p : NULL, d_flag,
                                        NULL);
        if (!rc) rc = span_end(ix);
    }
    if (!rc && !a->fill && !dev_out) rc = download(a->counts, d_cnt, cnt_b);
    if (!rc && a->fill) rc = download(&flag, d_flag, sizeof(flag));
    if (!rc && flag) rc = KNN_ERR_INVALID;   /* a segment is not its query's number of hits */
    if (!rc && nrec) rc = download(a->out, d_rec, nrec * sizeof(knn_neighbour_t));
    if (rc) hipStreamSynchronize(NULL);
    else if (nrec && ix->labels) fill_labels(a->out, nrec, ix->labels);
    dev_src_free(&q);
    scratch_free(d_pos);
    scratch_free(d_tab);
    return rc;
}

/* the query forms: knn_index_query's checks without a k */
static int radius_query(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, const radius_t *a)
{
    if (!ix || !Q || mq == 0) return KNN_ERR_INVALID;
    if (!knn_src_esize(src_dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
    if (a->flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_SRC | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    RCHK(radius_check(a, mq));
    return radius_run(ix, Q, NULL, mq, layout, src_dtype, a);
}

/* the rows forms: knn_index_neighbours' checks without a k, and its plan */
static int radius_rows(knn_index_t *ix, const int32_t *ids, size_t count, const radius_t *a)
{
    if (!ix || (ids ? count == 0 : count != 0)) return KNN_ERR_INVALID;
    if (a->flags & ~(KNN_QUERY_KEEP_ZERO | KNN_INDEX_DEVICE_OUT)) return KNN_ERR_INVALID;
    const size_t mq = ids ? count : ix->m;
    if (mq > 0x7fffffffULL || ix->m + mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    if (!ids_ok(ix, ids, count)) return KNN_ERR_INVALID;
    RCHK(radius_check(a, mq));
    int32_t *pos = NULL;
    RCHK(rows_plan(ix, ids, count, &pos));
    return radius_run(ix, NULL, pos, mq, 0, 0, a);
}

int knn_index_radius_count(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, double radius,
                           int flags, int32_t *counts)
{
    const radius_t a = {.radius = radius, .flags = flags, .counts = counts};
    return radius_query(ix, Q, mq, layout, src_dtype, &a);
}

int knn_index_radius(knn_index_t *ix, const void *Q, size_t mq, int layout, int src_dtype, double radius, int flags,
                     const int64_t *indptr, knn_neighbour_t *out)
{
    const radius_t a = {.radius = radius, .flags = flags, .fill = 1, .indptr = indptr, .out = out};
    return radius_query(ix, Q, mq, layout, src_dtype, &a);
}

int knn_index_radius_rows_count(knn_index_t *ix, const int32_t *ids, size_t count, double radius, int flags,
                                int32_t *counts)
{
    const radius_t a = {.radius = radius, .flags = flags, .counts = counts};
    return radius_rows(ix, ids, count, &a);
}

int knn_index_radius_rows(knn_index_t *ix, const int32_t *ids, size_t count, double radius, int flags,
                          const int64_t *indptr, knn_neighbour_t *out)
{
    const radius_t a = {.radius = radius, .flags = flags, .fill = 1, .indptr = indptr, .out = out};
    return radius_rows(ix, ids, count, &a);
}

/* --------------------------------------------------------------- dbscan */

/* DBSCAN (include/knn.h has the definition; the kernels are in knn_radius.hip).
 * Two distance passes over the square of the corpus, each resident block the
 * query tile of its own rows -- no gather, no tile buffer, no context -- and
 * KNN_RADIUS_MAXBLK corpus blocks a launch: count (the radius calls' count
 * form with the row itself and its duplicates counted: N(x)), then link, which
 * consumes every hit where it is found; O(m) kernels in front (init) and
 * behind (resolve).  One buffer, d_dbs, holds everything: five int32 arrays
 * by position (nbr, parent, root, rank, cluster), the block sums of the rank's
 * prefix sum with the number of clusters behind them, the border slots (16
 * bytes a row) and, on the element path, the table of the largest launch's
 * per-chunk minima.  Under KNN_INDEX_DEVICE_OUT cluster and nbr are the
 * caller's.  Every allocation in front of the span, nothing uploaded; the host
 * outputs arrive through a staging array, so that a failed call has written
 * none.  The dbscan launchers are named here alone, and only
 * knn_index_dbscan reaches this function. */
static int dbscan_run(knn_index_t *ix, double eps, int min_pts, int dev_out, int32_t *cluster, int32_t *neighbours,
                      int *nclusters)
{
    const size_t m = ix->m, nb256 = (m + 255) / 256, rp = knn_rows_pad(ix->cap);
    const int use_s8 = s8_stays(ix, ix->cmeta);
    const int thr = use_s8 ? (int)knn_radius_threshold(eps, knn_radius_d2max(ix->n)) : 0;
    /* the element path's table: nq records a chunk of the largest launch.  Every
     * block but the last is full (set_counts), so the first and the last block
     * are the two query sizes there are, and a launch's largest block is its
     * first.  (Both sizes: with fewer query workgroups a launch takes more
     * chunks a block, so the smaller tile can need the larger table.) */
    size_t tab_cap = 0;
    for (int last = 0; last < 2 && !use_s8; last++) {
        const size_t nq = ix->b.cnc[last ? ix->nblk - 1 : 0];
        for (size_t b0 = 0; b0 < ix->nblk && nq; b0 += KNN_RADIUS_MAXBLK) {
            const int nl = (int)(ix->nblk - b0 < KNN_RADIUS_MAXBLK ? ix->nblk - b0 : KNN_RADIUS_MAXBLK);
            int rpc;
            unsigned gy;
            if (!ix->b.cnc[b0]) continue;
            knn_radius_chunks((unsigned)((nq + 15) / 16), nl, (int)ix->b.cnc[b0], 64, &rpc, &gy);
            if (nq * gy * (size_t)nl > tab_cap) tab_cap = nq * gy * (size_t)nl;
        }
    }
    const size_t ints = knn_round_up(5 * m + nb256 + 1, 4);   /* (the records behind them: 16-byte aligned) */
    /* the host outputs' staging: cluster, neighbours, the number of clusters
     * (that alone under KNN_INDEX_DEVICE_OUT) */
    const size_t nst = dev_out ? 1 : 2 * m + 1;
    int32_t *stage = (int32_t *)malloc(nst * sizeof(int32_t));
    if (!stage) return KNN_ERR_NOMEM;
    int rc = hipSetDevice(0) == hipSuccess ? KNN_OK : KNN_ERR_HIP;
    if (!rc) rc = own_grow(ix, &ix->d_dbs, ints * sizeof(int32_t) + (m + tab_cap) * sizeof(knn_neighbour_t));
    int32_t *nbr = NULL, *lab = NULL, *bsum = NULL;
    if (!rc) {
        int32_t *own = (int32_t *)ix->d_dbs.p, *parent = own + m, *root = own + 2 * m, *rank = own + 3 * m;
        knn_neighbour_t *border = (knn_neighbour_t *)(own + ints), *tab = border + m;
        nbr = dev_out && neighbours ? neighbours : own;
        lab = dev_out ? cluster : own + 4 * m;
        bsum = own + 5 * m;
        hipEventRecord(ix->e0, NULL);
        rc = knn_launch_dbscan_init(nbr, parent, border, use_s8, m, NULL);
        for (int link = 0; link < 2 && !rc; link++)
            for (size_t bq = 0; bq < ix->nblk && !rc; bq++) {
                const int nq = (int)ix->b.cnc[bq];
                const int64_t qbase = (int64_t)ix->b.cbase[bq];
                for (size_t b0 = 0; b0 < ix->nblk && nq && !rc; b0 += KNN_RADIUS_MAXBLK) {
                    knn_radius_blocks_t cb;
                    radius_table(ix, b0, use_s8, &cb);
                    if (use_s8 && !link)
                        rc = knn_launch_radius_i8(0, ix->b.s8[bq], rp, nq, NULL, &cb, rp, (int)ix->n, thr, 1,
                                                  nbr + qbase, NULL, NULL, NULL, NULL);
                    else if (use_s8)
                        rc = knn_launch_dbscan_link_i8(ix->b.s8[bq], rp, nq, qbase, &cb, rp, (int)ix->n, thr, nbr,
                                                       min_pts, parent, border, NULL);
                    else if (!link)
                        rc = knn_launch_radius_scan(0, ix->dtype, ix->b.blk[bq], nq, NULL, &cb, (int)ix->n, eps, 1,
                                                    nbr + qbase, NULL, NULL, NULL, NULL);
                    else
                        rc = knn_launch_dbscan_link_scan(ix->dtype, ix->b.blk[bq], nq, qbase, &cb, (int)ix->n, eps,
                                                         nbr, min_pts, parent, border, tab, tab_cap, NULL);
                }
            }
        if (!rc) rc = knn_launch_dbscan_resolve(nbr, min_pts, parent, border, use_s8, m, root, rank, bsum, lab, NULL);
        if (!rc) rc = span_end(ix);
    }
    if (!rc && !dev_out) rc = download(stage, lab, m * sizeof(int32_t));
    if (!rc && !dev_out && neighbours) rc = download(stage + m, nbr, m * sizeof(int32_t));
    if (!rc && nclusters) rc = download(stage + nst - 1, bsum + nb256, sizeof(int32_t));
    if (rc) {
        hipStreamSynchronize(NULL);
    } else {
        if (!dev_out) memcpy(cluster, stage, m * sizeof(int32_t));
        if (!dev_out && neighbours) memcpy(neighbours, stage + m, m * sizeof(int32_t));
        if (nclusters) *nclusters = (int)stage[nst - 1];
    }
    free(stage);
    return rc;
}

int knn_index_dbscan(knn_index_t *ix, double eps, int min_pts, int flags, int32_t *cluster, int32_t *neighbours,
                     int *nclusters)
{
    if (!ix || !cluster || min_pts < 1) return KNN_ERR_INVALID;
    if (!(eps >= 0.0) || !(eps <= 1.7976931348623157e308)) return KNN_ERR_INVALID;   /* (a NaN fails both) */
    if (flags & ~KNN_INDEX_DEVICE_OUT) return KNN_ERR_INVALID;
    if (ix->m == 0) {   /* nothing to cluster */
        if (nclusters) *nclusters = 0;
        return KNN_OK;
    }
    return dbscan_run(ix, eps, min_pts, (flags & KNN_INDEX_DEVICE_OUT) != 0, cluster, neighbours, nclusters);
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
    if (device_bytes) *device_bytes = ix->dev_bytes + knn_ctx_device_bytes(ix->ctx);
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
    if (k > k_max(dtype)) return KNN_ERR_UNSUPPORTED;
    if (!layout_ok(layout)) return KNN_ERR_INVALID;
    if (flags & ~KNN_QUERY_KEEP_ZERO) return KNN_ERR_INVALID;
    if (m > 0x7fffffffULL || mq > 0x7fffffffULL || m + mq > 0x7fffffffULL || n > 0x7fffffffULL)
        return KNN_ERR_INVALID;
    knn_index_t *ix = NULL;
    RCHK(index_alloc(&ix, m, n, dtype));
    const size_t cnt = mq * (size_t)k;
    const batch_t bt = tile_shape(ix, mq);
    dev_src_t x = {0}, q = {0};
    /* every allocation, then the uploads: the span starts behind a copy, with
     * no fresh memory still to be mapped in front of its first kernel */
    int rc = index_reserve(ix, &bt, k, 0);
    if (!rc) rc = index_out(ix, cnt);
    if (!rc) rc = index_alloc_blocks(ix);
    if (!rc) rc = dev_src(&x, X, m * n * sizeof(double), 0);
    if (!rc) rc = dev_src(&q, Q, mq * n * sizeof(double), 0);
    if (!rc) {
        /* every block and tile packed, one wait for their meta, then the byte
         * forms and the searches */
        hipEventRecord(ix->e0, NULL);
        rc = build_pack(ix, x.src, layout, KNN_F64);
        if (!rc) rc = run_pack(ix, q.src, &bt, layout, KNN_F64);
        if (!rc) rc = stream_wait();
        if (!rc) rc = build_finish(ix, x.src, layout, KNN_F64, ix->thm, ix->ntile);
        if (!rc) rc = run_finish(ix, q.src, &bt, layout, KNN_F64, flags, (knn_neighbour_t *)ix->d_out.p);
        if (!rc) rc = span_end(ix);
    }
    if (!rc) rc = download(out, ix->d_out.p, cnt * sizeof(knn_neighbour_t));
    if (rc) hipStreamSynchronize(NULL);
    dev_src_free(&x);
    dev_src_free(&q);
    index_free(ix);
    if (!rc && labels) fill_labels(out, cnt, labels);
    return rc;
}
