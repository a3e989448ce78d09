/*
 * index_trace.c -- knn_index.c's device calls, traced on a CPU, and its
 * failure paths swept.
 *
 * A stand-alone program: linked with knn_index.c and knn_blocks.c and nothing
 * of HIP.  It stubs the hip* calls those files use, the engine boundary they
 * call (knn_ctx_*, knn_block_pack_*, knn_device_probe) and the knn_launch_*
 * launchers; the size and predicate helpers (knn_block_bytes_dt,
 * knn_block_meta_offset_dt, knn_s8_spec_ok) are knn_engine.c's own: that file
 * is linked behind this one, the definitions here win, and what nothing
 * references is dropped (test_index_trace.py has the link line).
 *
 * The line buffer, the live set, the fault knob and the plain HIP stubs are
 * tests/trace_common.h's (shared with engine_trace.c): hipMalloc returns
 * zeroed host memory, entered in a live set under an ordinal name (A1, A2,
 * ...; pinned memory P, events E, the caller's own device buffers U); hipFree
 * of a pointer that is neither live nor NULL ends the program.  The copies and
 * memsets copy and set, checked against the live set.
 * The pack, append and scatter stubs write the meta the step chose into
 * the block's meta words -- 8-bit integer data (knn_s8_spec_ok holds) or real
 * data -- and knn_ctx_end reports the unresolved count the step chose, so the
 * index decides its paths as on a device.  Every stub appends one line to the
 * trace: its name and its arguments, pointers as name+offset ("H": host
 * memory, "0": NULL).
 *
 *   index_trace             every scenario's trace ("## name" opens one,
 *                           "# ..." marks each call into the index)
 *   index_trace NAME...     the named ones
 *   index_trace --sweep     the fault sweep; exit status 1 on a violation
 *
 * The sweep: the stubs count every call whose failure the index can see
 * (hipMalloc, hipHostMalloc, copies, memsets, launchers, knn_ctx_*), and can
 * fail the N-th with its natural error.  For every step but a destroy, with C
 * its count on a clean run, and for N = 1 .. C, the step runs on a rebuilt
 * pre-state with fault N and must: return non-zero; free nothing twice; leave
 * knn_index_info's m and block count and knn_index_last_id as they were (the
 * block count may be the reblocked one when an add failed behind its
 * reblock); leave live exactly the device bytes knn_index_info accounts for
 * -- the blocks, the id map, and whatever query state the index still owns
 * (a failed search may drop it; record buffer and id map may have grown);
 * succeed on a clean retry whose trace from the first enqueue on (allocations
 * aside, names in order of appearance) is that of a first clean run, or its
 * end where the failed call's reblock stayed; and leave nothing live behind
 * knn_index_destroy.  A knn_index_update that failed behind its first
 * enqueued scatter is fit only for destroy: return value, frees and the
 * empty live set alone are checked.  A failed classify call must also leave
 * its host outputs (pred, counts, the records, *matches; filled with a
 * sentinel in front of the call) as they were, and every vote, the clean
 * retry's included, must be handed the labels a model of the index's labels
 * by id holds (run_step keeps it; every call brings other label values, so a
 * stale range that was not uploaded shows).
 */
#define TRACE_PROG "index_trace"
/* (a knn_index_update that fails behind its first enqueued scatter) */
static int g_scattered, g_fault_behind_scatter;
#define FAULT_HOOK() (g_fault_behind_scatter = g_scattered)
#include "../trace_common.h"

#include "knn_internal.h"

/* ---- the engine boundary ------------------------------------------------ */

enum { INT8, REAL };   /* the data a step's packs, appends and scatters see */
static int g_kind;
static size_t g_unres_end, g_unres_research;

/* a writer's meta into the block's meta words: set (a pack) or MAX-ed in */
static void write_meta(void *blk, size_t off, size_t n, int s8, int set, const char *who)
{
    double v[KNN_META_DOUBLES] = {0};
    need(blk, off + sizeof(v), who);
    if (g_kind == INT8) {   /* integers in [0, 255] */
        v[KNN_META_MAXABS] = v[KNN_META_MAXPOS] = 255.0;
        v[KNN_META_MAXNORM] = 255.0 * 255.0 * (double)n;
    } else {                /* real values in (-1, 1) */
        v[KNN_META_MAXABS] = v[KNN_META_MAXPOS] = v[KNN_META_MAXNEG] = 0.75;
        v[KNN_META_MAXNORM] = (double)n;
        v[KNN_META_NONINT] = 1.0;
    }
    v[KNN_META_S8] = s8;
    double *m = (double *)((char *)blk + off);
    for (int j = 0; j < KNN_META_DOUBLES; j++)
        if (set || v[j] > m[j]) m[j] = v[j];
}

int knn_device_probe(int device, int *cus)
{
    L("knn_device_probe %d", device);
    if (cus) *cus = 256;
    return KNN_OK;
}

void knn_set_last_search_seconds(double s) { L("knn_set_last_search_seconds %g", s); }

int knn_block_pack_dt(void *blk, int dtype, size_t cap, size_t rows, size_t n, const void *src, int src_dtype,
                      size_t ld, int layout, void *stream)
{
    FALLIBLE("knn_block_pack_dt", KNN_ERR_HIP);
    L("knn_block_pack_dt %s %d %zu %zu %zu %s %d %zu %d %s", N(blk), dtype, cap, rows, n, N(src), src_dtype, ld, layout,
      N(stream));
    write_meta(blk, knn_block_meta_offset_dt(cap, n, dtype), n, 0, 1, "knn_block_pack_dt");
    return KNN_OK;
}

int knn_block_pack_s8(void *blk, int dtype, size_t cap, size_t rows, size_t n, const void *src, int src_dtype,
                      size_t ld, int layout, void *stream)
{
    FALLIBLE("knn_block_pack_s8", KNN_ERR_HIP);
    L("knn_block_pack_s8 %s %d %zu %zu %zu %s %d %zu %d %s", N(blk), dtype, cap, rows, n, N(src), src_dtype, ld, layout,
      N(stream));
    write_meta(blk, knn_s8_meta_offset(cap, n), n, 1, 1, "knn_block_pack_s8");
    return KNN_OK;
}

int knn_launch_append(void *blk, int dtype, size_t cap, size_t row0, size_t rows, size_t n, const void *src,
                      int src_dtype, size_t ld, int layout, void *stream)
{
    FALLIBLE("knn_launch_append", KNN_ERR_HIP);
    L("knn_launch_append %s %d %zu %zu %zu %zu %s %d %zu %d %s", N(blk), dtype, cap, row0, rows, n, N(src), src_dtype,
      ld, layout, N(stream));
    write_meta(blk, knn_block_meta_offset_dt(cap, n, dtype), n, 0, 0, "knn_launch_append");
    return KNN_OK;
}

int knn_launch_append_s8(void *blk, int dtype, size_t cap, size_t row0, size_t rows, size_t n, const void *src,
                         int src_dtype, size_t ld, int layout, void *stream)
{
    FALLIBLE("knn_launch_append_s8", KNN_ERR_HIP);
    L("knn_launch_append_s8 %s %d %zu %zu %zu %zu %s %d %zu %d %s", N(blk), dtype, cap, row0, rows, n, N(src),
      src_dtype, ld, layout, N(stream));
    write_meta(blk, knn_s8_meta_offset(cap, n), n, 1, 0, "knn_launch_append_s8");
    return KNN_OK;
}

int knn_launch_scatter(void *blk, int dtype, size_t cap, const int32_t *pos, const int32_t *srow, size_t rows,
                       size_t n, const void *src, size_t src_rows, int src_dtype, size_t ld, int layout, void *stream)
{
    FALLIBLE("knn_launch_scatter", KNN_ERR_HIP);
    L("knn_launch_scatter %s %d %zu %s %s %zu %zu %s %zu %d %zu %d %s", N(blk), dtype, cap, N(pos), N(srow), rows, n,
      N(src), src_rows, src_dtype, ld, layout, N(stream));
    need(pos, rows * sizeof(int32_t), "knn_launch_scatter");
    write_meta(blk, knn_block_meta_offset_dt(cap, n, dtype), n, 0, 0, "knn_launch_scatter");
    g_scattered = 1;
    return KNN_OK;
}

int knn_launch_scatter_s8(void *blk, int dtype, size_t cap, const int32_t *pos, const int32_t *srow, size_t rows,
                          size_t n, const void *src, size_t src_rows, int src_dtype, size_t ld, int layout,
                          void *stream)
{
    FALLIBLE("knn_launch_scatter_s8", KNN_ERR_HIP);
    L("knn_launch_scatter_s8 %s %d %zu %s %s %zu %zu %s %zu %d %zu %d %s", N(blk), dtype, cap, N(pos), N(srow), rows, n,
      N(src), src_rows, src_dtype, ld, layout, N(stream));
    need(pos, rows * sizeof(int32_t), "knn_launch_scatter_s8");
    write_meta(blk, knn_s8_meta_offset(cap, n), n, 1, 0, "knn_launch_scatter_s8");
    g_scattered = 1;
    return KNN_OK;
}

int knn_launch_gather(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap, const int32_t *list,
                      size_t rows, size_t n, int dtype, void *stream)
{
    FALLIBLE("knn_launch_gather", KNN_ERR_HIP);
    L("knn_launch_gather %s %zu %zu %s %zu %s %zu %zu %d %s", N(dst), dst_cap, row0, N(src), src_cap, N(list), rows, n,
      dtype, N(stream));
    need(dst, knn_block_bytes_dt(dst_cap, n, dtype), "knn_launch_gather");
    need(src, knn_block_bytes_dt(src_cap, n, dtype), "knn_launch_gather");
    need(list, rows * sizeof(int32_t), "knn_launch_gather");
    return KNN_OK;
}

int knn_launch_gather_rows8(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap,
                            const int32_t *list, size_t rows, size_t n, void *stream)
{
    FALLIBLE("knn_launch_gather_rows8", KNN_ERR_HIP);
    L("knn_launch_gather_rows8 %s %zu %zu %s %zu %s %zu %zu %s", N(dst), dst_cap, row0, N(src), src_cap, N(list), rows,
      n, N(stream));
    need(dst, knn_s8_bytes(dst_cap, n), "knn_launch_gather_rows8");
    need(src, knn_s8_bytes(src_cap, n), "knn_launch_gather_rows8");
    need(list, rows * sizeof(int32_t), "knn_launch_gather_rows8");
    return KNN_OK;
}

int knn_launch_gather_pos(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap, size_t nblk,
                          const int32_t *pos, size_t rows, size_t n, int dtype, void *stream)
{
    FALLIBLE("knn_launch_gather_pos", KNN_ERR_HIP);
    L("knn_launch_gather_pos %s %zu %zu %s %zu %zu %s %zu %zu %d %s", N(dst), dst_cap, row0, N(tab), src_cap, nblk,
      N(pos), rows, n, dtype, N(stream));
    need(dst, knn_block_bytes_dt(dst_cap, n, dtype), "knn_launch_gather_pos");
    need(tab, nblk * sizeof(void *), "knn_launch_gather_pos");
    need(pos, rows * sizeof(int32_t), "knn_launch_gather_pos");
    return KNN_OK;
}

int knn_launch_gather_pos8(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap,
                           size_t nblk, const int32_t *pos, size_t rows, size_t n, void *stream)
{
    FALLIBLE("knn_launch_gather_pos8", KNN_ERR_HIP);
    L("knn_launch_gather_pos8 %s %zu %zu %s %zu %zu %s %zu %zu %s", N(dst), dst_cap, row0, N(tab), src_cap, nblk, N(pos),
      rows, n, N(stream));
    need(dst, knn_s8_bytes(dst_cap, n), "knn_launch_gather_pos8");
    need(tab, nblk * sizeof(void *), "knn_launch_gather_pos8");
    need(pos, rows * sizeof(int32_t), "knn_launch_gather_pos8");
    return KNN_OK;
}

int knn_launch_shadow8(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, const double *meta,
                       void *stream)
{
    FALLIBLE("knn_launch_shadow8", KNN_ERR_HIP);
    L("knn_launch_shadow8 %s %s %d %zu %zu %s %s", N(dst), N(blk), dtype, rows_pad, n, N(meta), N(stream));
    need(dst, rows_pad * knn_s8_rs(n) + rows_pad * 8, "knn_launch_shadow8");
    return KNN_OK;
}

int knn_launch_remap_idx(knn_neighbour_t *nb, size_t cnt, const int32_t *ids, size_t nids, void *stream)
{
    FALLIBLE("knn_launch_remap_idx", KNN_ERR_HIP);
    L("knn_launch_remap_idx %s %zu %s %zu %s", N(nb), cnt, N(ids), nids, N(stream));
    need(nb, cnt * sizeof(*nb), "knn_launch_remap_idx");
    need(ids, nids * sizeof(int32_t), "knn_launch_remap_idx");
    return KNN_OK;
}

int knn_launch_drop_self(knn_neighbour_t *out, const knn_neighbour_t *in, const int32_t *pos, size_t nq, int k,
                         const int32_t *ids, size_t nids, void *stream)
{
    FALLIBLE("knn_launch_drop_self", KNN_ERR_HIP);
    L("knn_launch_drop_self %s %s %s %zu %d %s %zu %s", N(out), N(in), N(pos), nq, k, N(ids), nids, N(stream));
    need(out, nq * (size_t)k * sizeof(*out), "knn_launch_drop_self");
    need(in, nq * (size_t)(k + 1) * sizeof(*in), "knn_launch_drop_self");
    return KNN_OK;
}

/* the labels by id as the calls so far have left them (run_step keeps it), and
 * how often the vote saw another device copy than that */
#define MAX_LABELS 4096
static double g_model[MAX_LABELS];
static int g_bad_labels;
#define VOTE_MATCHES 7   /* what the vote leaves in the match counter */

int knn_launch_vote_index(knn_neighbour_t *nb, size_t mq, int k, int nclasses, int rule, const double *labels,
                          size_t nlabels, const double *qlab, const int32_t *own_ids, int *pred, int *counts,
                          unsigned long long *matches, void *stream)
{
    FALLIBLE("knn_launch_vote_index", KNN_ERR_HIP);
    L("knn_launch_vote_index %s %zu %d %d %d %s %zu %s %s %s %s %s %s", N(nb), mq, k, nclasses, rule, N(labels), nlabels,
      N(qlab), N(own_ids), N(pred), N(counts), N(matches), N(stream));
    need(nb, mq * (size_t)k * sizeof(*nb), "knn_launch_vote_index");
    need(labels, nlabels * sizeof(double), "knn_launch_vote_index");
    if (qlab) need(qlab, mq * sizeof(double), "knn_launch_vote_index");
    if (own_ids) need(own_ids, mq * sizeof(int32_t), "knn_launch_vote_index");
    need(pred, mq * sizeof(int), "knn_launch_vote_index");
    if (counts) need(counts, mq * (size_t)nclasses * sizeof(int), "knn_launch_vote_index");
    if (nlabels > MAX_LABELS || memcmp(labels, g_model, nlabels * sizeof(double))) g_bad_labels++;
    if (matches) {
        need(matches, sizeof(*matches), "knn_launch_vote_index");
        *matches = VOTE_MATCHES;
    }
    return KNN_OK;
}

/* the context: one device buffer, and the form of its last begin */
struct knn_ctx {
    void *buf;
    int s8;
};
#define CTX_BYTES 4096
static int g_nctx;

int knn_ctx_create_dt(knn_ctx_t **out, int device, size_t nq, size_t n, size_t block_cap, int k, int dtype)
{
    FALLIBLE("knn_ctx_create_dt", KNN_ERR_NOMEM);
    knn_ctx_t *c = (knn_ctx_t *)calloc(1, sizeof(*c));
    if (!c) DIE("out of memory");
    c->buf = live_new(CTX_BYTES, 'A');
    g_nctx++;
    L("knn_ctx_create_dt %s %d %zu %zu %zu %d %d", N(c->buf), device, nq, n, block_cap, k, dtype);
    *out = c;
    return KNN_OK;
}

int knn_ctx_destroy(knn_ctx_t *c)
{
    if (!c) return KNN_ERR_INVALID;
    L("knn_ctx_destroy %s", N(c->buf));
    live_free(c->buf, "knn_ctx_destroy");
    free(c);
    g_nctx--;
    return KNN_OK;
}

size_t knn_ctx_device_bytes(const knn_ctx_t *c) { return c ? CTX_BYTES : 0; }
int knn_ctx_contraction_bits(const knn_ctx_t *c) { return c->s8 ? 8 : 64; }

int knn_ctx_set_keep_zero(knn_ctx_t *c, int on)
{
    L("knn_ctx_set_keep_zero %s %d", N(c->buf), on);
    return KNN_OK;
}

int knn_ctx_set_rows(knn_ctx_t *c, size_t rows)
{
    FALLIBLE("knn_ctx_set_rows", KNN_ERR_INVALID);
    L("knn_ctx_set_rows %s %zu", N(c->buf), rows);
    return KNN_OK;
}

int knn_ctx_begin_s8(knn_ctx_t *c, const void *qs8, size_t q_cap, size_t q_base, const double *d_meta,
                     const double *h_meta, void *stream)
{
    FALLIBLE("knn_ctx_begin_s8", KNN_ERR_HIP);
    L("knn_ctx_begin_s8 %s %s %zu %zu %s %s %s", N(c->buf), N(qs8), q_cap, q_base, N(d_meta), N(h_meta), N(stream));
    c->s8 = 1;
    return KNN_OK;
}

int knn_ctx_begin_meta(knn_ctx_t *c, const void *qblk, size_t q_cap, size_t q_base, const double *d_meta,
                       const double *h_meta, void *stream)
{
    FALLIBLE("knn_ctx_begin_meta", KNN_ERR_HIP);
    L("knn_ctx_begin_meta %s %s %zu %zu %s %s %s", N(c->buf), N(qblk), q_cap, q_base, N(d_meta), N(h_meta), N(stream));
    c->s8 = 0;
    return KNN_OK;
}

static void log_blocks(const char *name, knn_ctx_t *c, int nblk, const void *const *blk, const size_t *nc,
                       const size_t *base, const void *d_out, void *stream)
{
    char buf[900];
    int at = snprintf(buf, sizeof(buf), "%s %s %s %s blocks %d", name, N(c->buf), N(d_out), N(stream), nblk);
    for (int b = 0; b < nblk && at < (int)sizeof(buf) - 64; b++)
        at += snprintf(buf + at, sizeof(buf) - (size_t)at, " [ %s %zu %zu ]", N(blk[b]), nc[b], base[b]);
    L("%s", buf);
}

int knn_ctx_step_n(knn_ctx_t *c, int nblk, const void *const *blk, const size_t *nc, const size_t *base, void *stream)
{
    FALLIBLE("knn_ctx_step_n", KNN_ERR_HIP);
    log_blocks("knn_ctx_step_n", c, nblk, blk, nc, base, NULL, stream);
    return KNN_OK;
}

int knn_ctx_step_shadow_n(knn_ctx_t *c, int nblk, const void *const *blk, const size_t *nc, const size_t *base,
                          void *stream)
{
    FALLIBLE("knn_ctx_step_shadow_n", KNN_ERR_HIP);
    log_blocks("knn_ctx_step_shadow_n", c, nblk, blk, nc, base, NULL, stream);
    return KNN_OK;
}

int knn_ctx_end(knn_ctx_t *c, knn_neighbour_t *d_out, size_t *unresolved, void *stream)
{
    FALLIBLE("knn_ctx_end", KNN_ERR_HIP);
    L("knn_ctx_end %s %s %s -> %zu", N(c->buf), N(d_out), N(stream), g_unres_end);
    *unresolved = g_unres_end;
    return KNN_OK;
}

int knn_ctx_attach_qblock(knn_ctx_t *c, const void *qblk, size_t q_cap)
{
    FALLIBLE("knn_ctx_attach_qblock", KNN_ERR_INVALID);
    L("knn_ctx_attach_qblock %s %s %zu", N(c->buf), N(qblk), q_cap);
    return KNN_OK;
}

int knn_ctx_research_blocks(knn_ctx_t *c, int nblk, const void *const *blk, const size_t *nc, const size_t *base,
                            knn_neighbour_t *d_out, size_t *unresolved, void *stream)
{
    FALLIBLE("knn_ctx_research_blocks", KNN_ERR_HIP);
    log_blocks("knn_ctx_research_blocks", c, nblk, blk, nc, base, d_out, stream);
    *unresolved = g_unres_research;
    return KNN_OK;
}

int knn_ctx_rescan_step(knn_ctx_t *c, const void *blk, size_t nc, size_t base, void *stream)
{
    FALLIBLE("knn_ctx_rescan_step", KNN_ERR_HIP);
    L("knn_ctx_rescan_step %s %s %zu %zu %s", N(c->buf), N(blk), nc, base, N(stream));
    return KNN_OK;
}

int knn_ctx_rescan_end(knn_ctx_t *c, knn_neighbour_t *d_out, void *stream)
{
    FALLIBLE("knn_ctx_rescan_end", KNN_ERR_HIP);
    L("knn_ctx_rescan_end %s %s %s", N(c->buf), N(d_out), N(stream));
    return KNN_OK;
}

/* ---- the scenarios ------------------------------------------------------ */

#define DIMS 16
#define MAX_ROWS 2048
#define MAX_RECS (1 << 15)
#define MAX_IDS 128
#define SRC (KNN_INDEX_DEVICE_SRC)
#define OUT (KNN_INDEX_DEVICE_OUT)
#define KZ (KNN_QUERY_KEEP_ZERO)

enum { CREATE, QUERY, ADD, REMOVE, UPDATE, NEIGHBOURS, CLASSIFY_ROWS, CLASSIFY, ONECALL, DESTROY };
static const char *const op_name[] = {"create", "query", "add", "remove", "update", "neighbours", "classify_rows",
                                      "classify", "knn_query", "destroy"};
#define NCLS 10

typedef struct {
    int op;
    size_t rows;             /* rows, queries or listed ids (neighbours, 0: the whole corpus) */
    int k, flags, kind;
    size_t unres, unres2;    /* what knn_ctx_end and the re-search report */
    const char *tile;        /* KNN_QUERY_TILE */
    int id0, idstep;         /* the ids id0, id0 + idstep, ... */
    int may_reblock;         /* an add whose reblock may outlive its failure */
    int nolab;               /* an update that leaves the labels as they are */
    /* classify: the rule, and which of qlabels, matches, counts and out are given
     * (nclasses: NCLS) */
    int rule, qlab, matches, counts, out;
} step_t;

typedef struct {
    const char *name;
    const char *block;       /* KNN_QUERY_BLOCK */
    int f32, labels;
    step_t s[12];            /* up to the destroy */
} scn_t;

static const scn_t g_scn[] = {
    {"create_int8", "256", 0, 1, {{.op = CREATE, .rows = 600, .kind = INT8}, {.op = DESTROY}}},
    {"create_real_f32", "256", 1, 0, {{.op = CREATE, .rows = 600, .kind = REAL}, {.op = DESTROY}}},
    {"create_device_src", "256", 0, 0, {{.op = CREATE, .rows = 300, .kind = INT8, .flags = SRC}, {.op = DESTROY}}},
    {"query_host", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .flags = KZ},
      {.op = QUERY, .rows = 100, .k = 5, .kind = REAL},   /* a batch off the byte image */
      {.op = DESTROY}}},
    {"query_device", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .flags = SRC | OUT | KZ},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .flags = SRC},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .flags = OUT},
      {.op = DESTROY}}},
    {"query_two_tiles", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .tile = "64"},
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .tile = "64", .unres = 3},             /* re-search */
      {.op = QUERY, .rows = 100, .k = 5, .kind = INT8, .tile = "64", .unres = 3, .unres2 = 1}, /* and rescan */
      {.op = DESTROY}}},
    {"query_real", "256", 1, 0,
     {{.op = CREATE, .rows = 600, .kind = REAL},
      {.op = QUERY, .rows = 100, .k = 40, .kind = REAL},
      {.op = QUERY, .rows = 100, .k = 40, .kind = REAL, .unres = 2},   /* rescan */
      {.op = DESTROY}}},
    {"query_reuse", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 300, .k = 5, .kind = INT8},
      {.op = QUERY, .rows = 50, .k = 5, .kind = INT8},    /* the tile buffers again */
      {.op = QUERY, .rows = 50, .k = 7, .kind = INT8},    /* another k: another context */
      {.op = QUERY, .rows = 700, .k = 7, .kind = INT8},   /* past the tile capacity */
      {.op = DESTROY}}},
    {"add_fill_open", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = ADD, .rows = 100, .kind = INT8},                 /* inside the last block */
      {.op = ADD, .rows = 400, .kind = INT8, .flags = SRC},   /* fills it and opens two */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = DESTROY}}},
    {"add_drop_s8", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = ADD, .rows = 300, .kind = REAL},
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = ADD, .rows = 10, .kind = INT8},
      {.op = DESTROY}}},
    {"add_reblock", NULL, 0, 1,
     {{.op = CREATE, .rows = 200, .kind = INT8},
      {.op = ADD, .rows = 1300, .kind = INT8},   /* 8 blocks of 200 */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = ADD, .rows = 300, .kind = INT8, .may_reblock = 1},   /* a ninth: blocks of 400 */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = DESTROY}}},
    {"add_reblock_real", NULL, 1, 0,
     {{.op = CREATE, .rows = 200, .kind = REAL},
      {.op = ADD, .rows = 1500, .kind = REAL, .may_reblock = 1},
      {.op = DESTROY}}},
    {"add_after_remove", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = REMOVE, .rows = 2, .id0 = 5, .idstep = 295},
      {.op = ADD, .rows = 100, .kind = INT8},   /* the id map grows */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = ADD, .rows = 10, .kind = INT8},
      {.op = DESTROY}}},
    {"remove_last_block", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = REMOVE, .rows = 6, .id0 = 590, .idstep = 1},
      {.op = REMOVE, .rows = 4, .id0 = 597, .idstep = 1},   /* the last rows: nothing moves */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = DESTROY}}},
    {"remove_first_block", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = REMOVE, .rows = 2, .id0 = 3, .idstep = 257},
      {.op = REMOVE, .rows = 100, .id0 = 1, .idstep = 2},   /* a block fewer */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = DESTROY}}},
    {"remove_real", "256", 1, 0,
     {{.op = CREATE, .rows = 600, .kind = REAL}, {.op = REMOVE, .rows = 3, .id0 = 100, .idstep = 200}, {.op = DESTROY}}},
    {"remove_not_live", "256", 0, 0,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = REMOVE, .rows = 1, .id0 = 5},
      {.op = REMOVE, .rows = 1, .id0 = 5},
      {.op = DESTROY}}},
    {"update", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = UPDATE, .rows = 3, .id0 = 10, .idstep = 290, .kind = INT8},   /* every block */
      {.op = REMOVE, .rows = 1, .id0 = 7},
      {.op = UPDATE, .rows = 2, .id0 = 10, .idstep = 290, .kind = INT8, .flags = SRC},
      {.op = UPDATE, .rows = 2, .id0 = 10, .idstep = 290, .kind = REAL},   /* drops the byte blocks */
      {.op = QUERY, .rows = 20, .k = 5, .kind = INT8},
      {.op = DESTROY}}},
    {"neighbours", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = NEIGHBOURS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5},
      {.op = NEIGHBOURS, .rows = 0, .k = 5, .flags = KZ, .tile = "512", .unres = 2},
      {.op = NEIGHBOURS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .flags = KZ | OUT},
      {.op = REMOVE, .rows = 1, .id0 = 7},
      {.op = NEIGHBOURS, .rows = 0, .k = 5},
      {.op = NEIGHBOURS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .flags = KZ},
      {.op = DESTROY}}},
    {"neighbours_real", "256", 1, 0,
     {{.op = CREATE, .rows = 300, .kind = REAL},
      {.op = NEIGHBOURS, .rows = 0, .k = 5, .flags = OUT},
      {.op = NEIGHBOURS, .rows = 2, .id0 = 2, .idstep = 270, .k = 5, .flags = KZ, .unres = 1},
      {.op = DESTROY}}},
    {"knn_query", "256", 0, 1,
     {{.op = ONECALL, .rows = 100, .k = 5, .kind = INT8, .flags = KZ},
      {.op = ONECALL, .rows = 100, .k = 5, .kind = INT8, .tile = "64", .unres = 2, .unres2 = 1},
      {.op = ONECALL, .rows = 100, .k = 5, .kind = REAL},
      {.op = DESTROY}}},
    {"classify_host", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},   /* makes the labels' copy */
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .rule = KNN_VOTE_MPI, .qlab = 1, .matches = 1, .counts = 1,
       .out = 1},                                                                    /* uploads nothing */
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = REAL, .rule = KNN_VOTE_MAJORITY, .matches = 1},   /* counts none */
      {.op = DESTROY}}},
    {"classify_device", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .flags = SRC | OUT, .qlab = 1, .matches = 1, .counts = 1,
       .out = 1},
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .flags = KZ, .qlab = 1, .matches = 1},
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .flags = OUT},   /* the records in the index's buffer */
      {.op = DESTROY}}},
    {"classify_two_tiles", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = CLASSIFY, .rows = 100, .k = 5, .kind = INT8, .tile = "64", .unres = 3, .unres2 = 1, .qlab = 1,
       .matches = 1, .out = 1},   /* re-search and rescan ahead of the vote */
      {.op = DESTROY}}},
    {"classify_stale", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = ADD, .rows = 100, .kind = INT8},   /* room for 1200 labels */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = ADD, .rows = 50, .kind = INT8},    /* inside the device copy: a stale range */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = ADD, .rows = 20, .kind = INT8},
      {.op = UPDATE, .rows = 1, .id0 = 3, .kind = INT8},   /* the range grows downwards ... */
      {.op = ADD, .rows = 10, .kind = INT8},               /* ... and upwards */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = ADD, .rows = 500, .kind = INT8},   /* ids past the device copy: made again */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = DESTROY}}},
    {"classify_update", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .counts = 1},
      {.op = UPDATE, .rows = 3, .id0 = 10, .idstep = 290, .kind = INT8},
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .counts = 1},
      {.op = UPDATE, .rows = 2, .id0 = 10, .idstep = 290, .kind = INT8, .nolab = 1},
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .counts = 1},   /* uploads nothing */
      {.op = DESTROY}}},
    {"classify_rows", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = CLASSIFY_ROWS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .matches = 1},
      {.op = CLASSIFY_ROWS, .rows = 0, .k = 5, .rule = KNN_VOTE_MPI, .matches = 1, .counts = 1, .out = 1},
      {.op = CLASSIFY_ROWS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .flags = KZ, .matches = 1, .out = 1},
      {.op = CLASSIFY_ROWS, .rows = 0, .k = 5, .flags = KZ | OUT, .tile = "512", .unres = 2, .matches = 1, .counts = 1,
       .out = 1},
      {.op = CLASSIFY_ROWS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .flags = OUT},
      {.op = DESTROY}}},
    {"classify_rows_real", "256", 1, 1,
     {{.op = CREATE, .rows = 300, .kind = REAL},
      {.op = CLASSIFY_ROWS, .rows = 0, .k = 5, .matches = 1, .out = 1},
      {.op = CLASSIFY_ROWS, .rows = 2, .id0 = 2, .idstep = 270, .k = 5, .flags = KZ, .unres = 1, .matches = 1},
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = REAL, .qlab = 1, .matches = 1},
      {.op = DESTROY}}},
    {"classify_after_remove", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = REMOVE, .rows = 1, .id0 = 7},
      {.op = CLASSIFY_ROWS, .rows = 0, .k = 5, .matches = 1},   /* own labels through the id map */
      {.op = CLASSIFY_ROWS, .rows = 3, .id0 = 1, .idstep = 299, .k = 5, .flags = KZ, .matches = 1},   /* the uploaded ids */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = DESTROY}}},
    {"classify_drop_s8", "256", 0, 1,
     {{.op = CREATE, .rows = 600, .kind = INT8},
      {.op = ADD, .rows = 300, .kind = REAL},   /* drops the byte blocks */
      {.op = CLASSIFY, .rows = 20, .k = 5, .kind = INT8, .qlab = 1, .matches = 1},
      {.op = CLASSIFY_ROWS, .rows = 0, .k = 5, .matches = 1},
      {.op = DESTROY}}},
};
#define NSCN ((int)(sizeof(g_scn) / sizeof(g_scn[0])))
#define ONECALL_M 600   /* knn_query's corpus rows */

static double g_X[MAX_ROWS * DIMS], g_lab[MAX_ROWS];
static knn_neighbour_t g_out[MAX_RECS];
static int g_pred[MAX_ROWS], g_counts[MAX_ROWS * NCLS];
static int g_step_no;    /* calls into the index so far: every call brings other labels */
static int g_touched;    /* a failed classify wrote one of its host outputs */
#define SENTINEL 0x5a

static int all_sentinel(const void *p, size_t bytes)
{
    for (size_t i = 0; i < bytes; i++)
        if (((const unsigned char *)p)[i] != SENTINEL) return 0;
    return 1;
}

static void *user_alloc(size_t bytes) { return live_new(bytes, 'U'); }

static void user_free_all(void)
{
    for (int i = g_nlive - 1; i >= 0; i--)
        if (g_live[i].kind == 'U') live_free(g_live[i].base, "user_free_all");
    g_ord['U'] = 0;
}

/* one call into the index; "# info ..." behind it when it left one */
static int run_step(const scn_t *sc, knn_index_t **ix, const step_t *s)
{
    const int dt = sc->f32 ? KNN_F32 : KNN_F64, lay = KNN_ROWMAJOR;
    const int dev = s->flags & (SRC | OUT), flags = s->op == CREATE || s->op == ADD || s->op == UPDATE
                                                        ? s->flags & SRC
                                                        : s->flags;
    int32_t ids[MAX_IDS];
    g_kind = s->kind;
    g_unres_end = s->unres;
    g_unres_research = s->unres2;
    if (s->tile) setenv("KNN_QUERY_TILE", s->tile, 1);
    else unsetenv("KNN_QUERY_TILE");
    if (s->rows > MAX_ROWS || (s->op >= REMOVE && s->op <= CLASSIFY_ROWS && s->rows > MAX_IDS)) DIE("step too large");
    for (size_t i = 0; i < s->rows && i < MAX_IDS; i++) ids[i] = s->id0 + (int32_t)i * s->idstep;
    const int cls = s->op == CLASSIFY || s->op == CLASSIFY_ROWS;
    L("# %s %zu k %d flags %d", op_name[s->op], s->rows, s->k, s->flags);
    if (cls) L("# rule %d qlabels %d matches %d counts %d out %d", s->rule, s->qlab, s->matches, s->counts, s->out);
    size_t mq = s->rows;
    if ((s->op == NEIGHBOURS || s->op == CLASSIFY_ROWS) && !mq) knn_index_info(*ix, &mq, NULL, NULL, NULL, NULL);
    if (mq * (size_t)(s->k ? s->k : 1) > MAX_RECS || (cls && mq > MAX_ROWS)) DIE("step too large");
    /* other labels with every call, so that a stale device copy shows */
    g_step_no++;
    for (size_t i = 0; i < MAX_ROWS; i++) g_lab[i] = (double)((i + 3 * (size_t)g_step_no) % NCLS);
    const void *src = (dev & SRC) ? user_alloc(s->rows * DIMS * sizeof(double)) : (void *)g_X;
    knn_neighbour_t *out = (dev & OUT) ? (knn_neighbour_t *)user_alloc(mq * (size_t)s->k * sizeof(*out)) : g_out;
    const double *lab = sc->labels && !s->nolab ? g_lab : NULL;
    size_t removed = 0, last = 0;
    int rc = KNN_OK;
    if (*ix) knn_index_last_id(*ix, &last);
    /* classify's outputs: the caller's device buffers under OUT, else host
     * arrays that a failed call must leave as they are */
    const size_t pred_b = mq * sizeof(int), counts_b = mq * NCLS * sizeof(int), out_b = mq * (size_t)s->k * sizeof(*out);
    int *pred = g_pred, *counts = s->counts ? g_counts : NULL;
    size_t hit = 0;
    if (cls && (dev & OUT)) {
        pred = (int *)user_alloc(pred_b);
        if (s->counts) counts = (int *)user_alloc(counts_b);
    } else if (cls) {
        memset(g_pred, SENTINEL, pred_b);
        memset(g_counts, SENTINEL, counts_b);
        memset(g_out, SENTINEL, out_b);
    }
    memset(&hit, SENTINEL, sizeof(hit));
    if (cls && !s->out) out = NULL;
    switch (s->op) {
    case CREATE: rc = knn_index_create(ix, src, s->rows, DIMS, lay, dt, lab, dt, flags); break;
    case QUERY: rc = knn_index_query(*ix, src, s->rows, lay, dt, s->k, flags, out); break;
    case ADD: rc = knn_index_add(*ix, src, s->rows, lay, dt, lab, flags); break;
    case REMOVE:
        rc = knn_index_remove(*ix, ids, s->rows, 0, &removed);
        if (!rc) L("# removed %zu", removed);
        break;
    case UPDATE: rc = knn_index_update(*ix, ids, s->rows, src, lay, dt, lab, flags); break;
    case NEIGHBOURS: rc = knn_index_neighbours(*ix, s->rows ? ids : NULL, s->rows, s->k, flags, out); break;
    case CLASSIFY_ROWS:
        rc = knn_index_classify_rows(*ix, s->rows ? ids : NULL, s->rows, s->k, NCLS, s->rule, flags, pred, counts,
                                     s->matches ? &hit : NULL, out);
        break;
    case CLASSIFY:
        rc = knn_index_classify(*ix, src, s->rows, lay, dt, s->k, NCLS, s->rule, flags, s->qlab ? g_lab : NULL, pred,
                                counts, s->matches ? &hit : NULL, out);
        break;
    case ONECALL: rc = knn_query(g_X, ONECALL_M, g_X, s->rows, DIMS, lay, lab, s->k, dt, flags, g_out); break;
    default:
        if (*ix) rc = knn_index_destroy(*ix);
        *ix = NULL;
    }
    user_free_all();
    if (cls && rc) {
        g_touched = !all_sentinel(&hit, sizeof(hit));
        if (!(dev & OUT)) g_touched |= !all_sentinel(g_pred, pred_b) || !all_sentinel(g_counts, counts_b) || !all_sentinel(g_out, out_b);
    }
    if (cls && !rc && s->matches) L("# matches %zu", all_sentinel(&hit, sizeof(hit)) ? (size_t)-1 : hit);
    /* the labels by id as the call left them */
    if (!rc && lab && s->op == CREATE) memcpy(g_model, g_lab, s->rows * sizeof(double));
    if (!rc && lab && s->op == ADD) memcpy(g_model + last, g_lab, s->rows * sizeof(double));
    if (!rc && lab && s->op == UPDATE)
        for (size_t i = 0; i < s->rows; i++) g_model[ids[i] - 1] = g_lab[i];
    if (g_bad_labels && g_echo) DIE("%s: the vote saw labels that are not the index's", sc->name);
    if (rc) L("# -> %d", rc);
    else if (*ix) {
        size_t m = 0, bytes = 0;
        int nblk = 0, bits = 0;
        knn_index_info(*ix, &m, NULL, &nblk, &bytes, &bits);
        knn_index_last_id(*ix, &last);
        L("# info m %zu blocks %d last_id %zu bytes %zu bits %d", m, nblk, last, bytes, bits);
        if (bytes != live_bytes('A')) DIE("%s: the index accounts for %zu bytes, %zu are live", sc->name, bytes, live_bytes('A'));
    }
    return rc;
}

static void scn_open(const scn_t *sc)
{
    if (g_nlive || g_nevents || g_nctx) DIE("%s: something is live in front of it", sc->name);
    memset(g_ord, 0, sizeof(g_ord));
    if (sc->block) setenv("KNN_QUERY_BLOCK", sc->block, 1);
    else unsetenv("KNN_QUERY_BLOCK");
}

static int nsteps(const scn_t *sc)
{
    int i = 0;
    while (sc->s[i].op != DESTROY) i++;
    return i + 1;
}

static void trace(const scn_t *sc)
{
    knn_index_t *ix = NULL;
    scn_open(sc);
    printf("## %s\n", sc->name);
    g_echo = 1;
    for (int i = 0; i < nsteps(sc); i++)
        if (run_step(sc, &ix, &sc->s[i])) DIE("%s: step %d failed", sc->name, i);
    g_echo = 0;
    lines_clear();
    if (g_nlive || g_nevents || g_nctx) DIE("%s: something is live behind it", sc->name);
}

/* ---- the sweep ---------------------------------------------------------- */

static int g_violations;

static void violation(const scn_t *sc, int step, long n, const char *what)
{
    printf("VIOLATION %s step %d (%s) fault %ld: %s\n", sc->name, step, op_name[sc->s[step].op], n, what);
    g_violations++;
}

static void sweep_step(const scn_t *sc, int step, long *faults)
{
    const step_t *s = &sc->s[step];
    knn_index_t *ix = NULL;
    char **clean = NULL;
    int nclean = 0;
    long count = 0;
    for (long n = 0; n <= count; n++) {   /* n = 0: the clean run that counts */
        scn_open(sc);
        for (int i = 0; i < step; i++)
            if (run_step(sc, &ix, &sc->s[i])) DIE("%s: step %d failed", sc->name, i);
        size_t m0 = 0, last0 = 0, m1 = 0, last1 = 0, bytes = 0;
        int nblk0 = 0, nblk1 = 0;
        if (ix) {
            knn_index_info(ix, &m0, NULL, &nblk0, NULL, NULL);
            knn_index_last_id(ix, &last0);
        }
        lines_clear();
        g_calls = g_scattered = g_fault_behind_scatter = 0;
        g_touched = g_bad_labels = 0;
        g_fail_at = n;
        int rc = run_step(sc, &ix, s);
        g_fail_at = 0;
        if (n == 0) {
            if (rc) DIE("%s: step %d failed", sc->name, step);
            count = g_calls;
            nclean = g_nline;
            clean = (char **)malloc((size_t)nclean * sizeof(char *));
            memcpy(clean, g_line, (size_t)nclean * sizeof(char *));
            g_nline = 0;
        } else {
            ++*faults;
            if (!rc) violation(sc, step, n, "the call succeeded");
            if (g_touched) violation(sc, step, n, "a failed classify wrote pred, matches, counts or out");
            const int ruined = s->op == UPDATE && g_fault_behind_scatter;
            if ((s->op == CREATE || s->op == ONECALL) && ix) violation(sc, step, n, "an index came out of a failed create");
            if (ix && !ruined) {
                knn_index_info(ix, &m1, NULL, &nblk1, &bytes, NULL);
                knn_index_last_id(ix, &last1);
                if (m1 != m0 || last1 != last0 || (s->may_reblock ? nblk1 > nblk0 : nblk1 != nblk0))
                    violation(sc, step, n, "m, the block count or the last id changed");
                if (bytes != live_bytes('A')) violation(sc, step, n, "live device memory is not what the index accounts for");
            } else if (!ix && live_bytes('A') + live_bytes('P')) {
                violation(sc, step, n, "a failed create left memory behind");
            }
            if (!ruined) {
                lines_clear();
                int nr = 0, nc = 0;
                if (run_step(sc, &ix, s)) {
                    violation(sc, step, n, "the clean retry failed");
                } else {
                    char *r = tail_of(g_line, g_nline, 0, &nr), *c = tail_of(clean, nclean, nr, &nc);
                    if (nr == 0 ? nc != 0 : (strcmp(r, c) || (nr != nc && !s->may_reblock)))
                        violation(sc, step, n, "the clean retry's trace differs");
                    free(r);
                    free(c);
                }
            }
        }
        if (g_bad_labels) violation(sc, step, n, "the vote saw labels that are not the index's");
        if (ix) knn_index_destroy(ix);
        ix = NULL;
        lines_clear();
        if (g_nlive || g_nevents || g_nctx) {
            violation(sc, step, n, "something is live behind knn_index_destroy");
            while (g_nlive) live_free(g_live[0].base, "sweep");
            g_nevents = g_nctx = 0;
        }
    }
    for (int i = 0; i < nclean; i++) free(clean[i]);
    free(clean);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--sweep")) {
        long faults = 0;
        int steps = 0;
        for (int i = 0; i < NSCN; i++)
            for (int st = 0; g_scn[i].s[st].op != DESTROY; st++, steps++) sweep_step(&g_scn[i], st, &faults);
        printf("sweep: %d steps, %ld faults, %d violations\n", steps, faults, g_violations);
        return g_violations != 0;
    }
    for (int i = 0; i < NSCN; i++) {
        int wanted = argc < 2;
        for (int a = 1; a < argc; a++) wanted |= !strcmp(argv[a], g_scn[i].name);
        if (wanted) trace(&g_scn[i]);
    }
    return 0;
}
