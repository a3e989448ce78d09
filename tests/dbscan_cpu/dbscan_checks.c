/*
 * dbscan_checks.c -- knn_index_dbscan on a CPU: every argument refusal comes
 * before any device call, a call makes the device calls it should (an init,
 * the count and link forms against every block table, one resolve) and leaves
 * the kept context alone, the index accounts for every byte the call keeps, a
 * second call allocates nothing, and a call that fails anywhere leaves the
 * index answering and has written none of its host outputs.
 *
 * A stand-alone program on tests/index_trace/index_trace.c's harness (its
 * stubs of the HIP runtime, the engine boundary and the launchers, its live
 * set and fault knob; its main is not used), with stubs of the launchers a
 * dbscan names: every stub logs a line, so "no device call" is "no new line".
 * Prints "ok: R refusals, F faults" or the first failure.
 */
#define main index_trace_main
#include "../index_trace/index_trace.c"
#undef main

#include <math.h>

static int g_ncount, g_nlink, g_ninit, g_nresolve;

int knn_launch_radius_i8(int fill, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
                         const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, int keep0, int32_t *counts,
                         const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream)
{
    (void)q_rows_pad, (void)c_rows_pad, (void)n, (void)indptr, (void)indptr0, (void)out, (void)stream;
    L("knn_launch_radius_i8 fill %d q %s nq %d self %s nblk %d T %d keep0 %d counts %s", fill, N(qs8), nq,
      N(self_pos), cb->nblk, T, keep0, N(counts));
    FALLIBLE("knn_launch_radius_i8", KNN_ERR_HIP);
    need(counts, (size_t)nq * sizeof(int32_t), "knn_launch_radius_i8");
    g_ncount++;
    return KNN_OK;
}

int knn_launch_radius_scan(int fill, int dtype, const void *qblk, int nq, const int32_t *self_pos,
                           const knn_radius_blocks_t *cb, int n, double radius, int keep0, int32_t *counts,
                           const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream)
{
    (void)dtype, (void)n, (void)indptr, (void)indptr0, (void)out, (void)stream;
    L("knn_launch_radius_scan fill %d q %s nq %d self %s nblk %d r %g keep0 %d counts %s", fill, N(qblk), nq,
      N(self_pos), cb->nblk, radius, keep0, N(counts));
    FALLIBLE("knn_launch_radius_scan", KNN_ERR_HIP);
    need(counts, (size_t)nq * sizeof(int32_t), "knn_launch_radius_scan");
    g_ncount++;
    return KNN_OK;
}

int knn_launch_dbscan_init(int32_t *nbr, int32_t *parent, void *border, int s8, size_t m, void *stream)
{
    (void)stream;
    L("knn_launch_dbscan_init nbr %s parent %s border %s s8 %d m %zu", N(nbr), N(parent), N(border), s8, m);
    FALLIBLE("knn_launch_dbscan_init", KNN_ERR_HIP);
    need(nbr, m * sizeof(int32_t), "knn_launch_dbscan_init");
    need(parent, m * sizeof(int32_t), "knn_launch_dbscan_init");
    need(border, m * sizeof(knn_neighbour_t), "knn_launch_dbscan_init");
    g_ninit++;
    return KNN_OK;
}

int knn_launch_dbscan_link_i8(const void *qs8, size_t q_rows_pad, int nq, int64_t qbase,
                              const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, const int32_t *nbr,
                              int min_pts, int32_t *parent, void *border, void *stream)
{
    (void)q_rows_pad, (void)c_rows_pad, (void)n, (void)stream;
    L("knn_launch_dbscan_link_i8 q %s nq %d qbase %lld nblk %d T %d min_pts %d nbr %s parent %s border %s", N(qs8), nq,
      (long long)qbase, cb->nblk, T, min_pts, N(nbr), N(parent), N(border));
    FALLIBLE("knn_launch_dbscan_link_i8", KNN_ERR_HIP);
    need(nbr + qbase, (size_t)nq * sizeof(int32_t), "knn_launch_dbscan_link_i8");
    need(parent + qbase, (size_t)nq * sizeof(int32_t), "knn_launch_dbscan_link_i8");
    g_nlink++;
    return KNN_OK;
}

int knn_launch_dbscan_link_scan(int dtype, const void *qblk, int nq, int64_t qbase, const knn_radius_blocks_t *cb,
                                int n, double eps, const int32_t *nbr, int min_pts, int32_t *parent, void *border,
                                void *tab, size_t tab_cap, void *stream)
{
    (void)dtype, (void)n, (void)stream;
    L("knn_launch_dbscan_link_scan q %s nq %d qbase %lld nblk %d eps %g min_pts %d nbr %s parent %s border %s tab %s "
      "cap %zu", N(qblk), nq, (long long)qbase, cb->nblk, eps, min_pts, N(nbr), N(parent), N(border), N(tab), tab_cap);
    FALLIBLE("knn_launch_dbscan_link_scan", KNN_ERR_HIP);
    need(nbr + qbase, (size_t)nq * sizeof(int32_t), "knn_launch_dbscan_link_scan");
    need(tab, tab_cap * sizeof(knn_neighbour_t), "knn_launch_dbscan_link_scan");
    if (tab_cap < (size_t)nq * (size_t)cb->nblk) DIE("knn_launch_dbscan_link_scan: a table of %zu records", tab_cap);
    g_nlink++;
    return KNN_OK;
}

int knn_launch_dbscan_resolve(const int32_t *nbr, int min_pts, const int32_t *parent, const void *border, int s8,
                              size_t m, int32_t *root, int32_t *rank, int32_t *bsum, int32_t *cluster, void *stream)
{
    (void)border, (void)stream;
    L("knn_launch_dbscan_resolve nbr %s min_pts %d parent %s s8 %d m %zu root %s rank %s bsum %s cluster %s", N(nbr),
      min_pts, N(parent), s8, m, N(root), N(rank), N(bsum), N(cluster));
    FALLIBLE("knn_launch_dbscan_resolve", KNN_ERR_HIP);
    need(root, m * sizeof(int32_t), "knn_launch_dbscan_resolve");
    need(rank, m * sizeof(int32_t), "knn_launch_dbscan_resolve");
    need(bsum, ((m + 255) / 256 + 1) * sizeof(int32_t), "knn_launch_dbscan_resolve");
    need(cluster, m * sizeof(int32_t), "knn_launch_dbscan_resolve");
    g_nresolve++;
    return KNN_OK;
}

#define ROWS 600
#define MQ 40
#define MARK 0x5a5a5a5a
static knn_index_t *g_ix;
static int32_t g_cl[ROWS], g_nb[ROWS];
static int g_nc, g_refusals;

/* the call returned `want` and made no device call */
#define REFUSED(want, call)                                                                      \
    do {                                                                                         \
        const int before_ = g_nline, rc_ = (call);                                               \
        if (rc_ != (want) || g_nline != before_) {                                               \
            printf("FAIL line %d: %s -> %d (want %d), %d device calls\n", __LINE__, #call, rc_,  \
                   (int)(want), g_nline - before_);                                              \
            return 1;                                                                            \
        }                                                                                        \
        g_refusals++;                                                                            \
    } while (0)

#define MUST(cond)                                             \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAIL line %d: %s\n", __LINE__, #cond);     \
            return 1;                                          \
        }                                                      \
    } while (0)

static size_t index_bytes(void)
{
    size_t bytes = 0;
    knn_index_info(g_ix, NULL, NULL, NULL, &bytes, NULL);
    return bytes;
}

static int accounted(void) { return index_bytes() == live_bytes('A'); }

static int has_line(int from, const char *prefix)
{
    for (int i = from; i < g_nline; i++)
        if (starts(g_line[i], prefix)) return 1;
    return 0;
}

static void mark(void)
{
    for (int i = 0; i < ROWS; i++) g_cl[i] = g_nb[i] = MARK;
    g_nc = MARK;
}

static int marked(void)
{
    for (int i = 0; i < ROWS; i++)
        if (g_cl[i] != MARK || g_nb[i] != MARK) return 0;
    return g_nc == MARK;
}

/* a dbscan, clean or with fault number `fault`; -1: past its last fallible step */
static int dbscan(long fault)
{
    g_calls = 0;
    g_fail_at = fault;
    int rc = knn_index_dbscan(g_ix, 3.0, 5, 0, g_cl, g_nb, &g_nc);
    if (g_fail_at && g_calls < g_fail_at) rc = -1;
    g_fail_at = 0;
    return rc;
}

int main(void)
{
    const int lay = KNN_ROWMAJOR;
    setenv("KNN_QUERY_BLOCK", "256", 1);
    unsetenv("KNN_QUERY_TILE");
    unsetenv("KNN_NO_I8");
    g_kind = INT8;
    MUST(knn_index_create(&g_ix, g_X, ROWS, DIMS, lay, KNN_F64, NULL, KNN_F64, 0) == KNN_OK);

    /* ---- refusals */
    mark();
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(NULL, 1.0, 5, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, 5, 0, NULL, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, 0, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, -3, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, -1.0, 5, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, -0.5, 5, KNN_INDEX_DEVICE_OUT, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, (double)NAN, 5, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, (double)INFINITY, 5, 0, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, 5, KNN_QUERY_KEEP_ZERO, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, 5, KNN_INDEX_DEVICE_SRC, g_cl, g_nb, &g_nc));
    REFUSED(KNN_ERR_INVALID, knn_index_dbscan(g_ix, 1.0, 5, 8, g_cl, g_nb, &g_nc));
    MUST(marked() && accounted());

    /* ---- a query, a dbscan, the query again: the context stays, and the
     * second query's trace holds no create */
    MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK);
    const int nctx = g_nctx;
    int at = g_nline;
    MUST(dbscan(0) == KNN_OK);
    /* 3 blocks: one table a query block and pass */
    MUST(g_ninit == 1 && g_ncount == 3 && g_nlink == 3 && g_nresolve == 1);
    MUST(has_line(at, "knn_launch_radius_i8 fill 0") && has_line(at, "knn_launch_dbscan_link_i8"));
    MUST(!has_line(at, "knn_launch_radius_scan") && !has_line(at, "knn_launch_dbscan_link_scan"));
    MUST(!has_line(at, "knn_launch_gather") && !has_line(at, "knn_block_pack"));          /* no gather, no pack */
    MUST(!has_line(at, "knn_ctx_") && g_nctx == nctx);
    MUST(has_line(at, "knn_set_last_search_seconds") && accounted() && !marked());
    /* a second call allocates nothing */
    const size_t kept = index_bytes();
    at = g_nline;
    MUST(dbscan(0) == KNN_OK && !has_line(at, "hipMalloc") && index_bytes() == kept);
    MUST(knn_index_dbscan(g_ix, 3.0, 5, 0, g_cl, NULL, NULL) == KNN_OK);                     /* the nullable outputs */
    at = g_nline;
    MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK);
    MUST(!has_line(at, "knn_ctx_create") && !has_line(at, "knn_ctx_destroy") && has_line(at, "knn_ctx_end"));
    MUST(accounted());

    /* ---- every fallible step of a call failed in turn */
    long faults = 0;
    for (long f = 1;; f++) {
        mark();
        const int rc = dbscan(f);
        if (rc == -1) break;
        faults++;
        MUST(rc != KNN_OK);
        MUST(marked());                                   /* none of the host outputs written */
        MUST(accounted());
        MUST(dbscan(0) == KNN_OK && !marked());
        MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK && g_nctx == nctx);
        lines_clear();
    }
    MUST(faults >= 10);

    /* ---- after a removal: every live row, no more */
    size_t removed = 0;
    const int32_t dead[1] = {7};
    MUST(knn_index_remove(g_ix, dead, 1, 0, &removed) == KNN_OK && removed == 1);
    at = g_nline;
    MUST(dbscan(0) == KNN_OK && has_line(at, "knn_launch_dbscan_init") && accounted());
    int saw = 0;
    for (int i = at; i < g_nline; i++)
        if (starts(g_line[i], "knn_launch_dbscan_resolve") && strstr(g_line[i], " m 599 ")) saw = 1;
    MUST(saw);
    MUST(knn_index_destroy(g_ix) == KNN_OK);
    MUST(g_nlive == 0 && g_nevents == 0 && g_nctx == 0);

    /* ---- a real-valued index: the element path, its table inside the buffer */
    g_kind = REAL;
    MUST(knn_index_create(&g_ix, g_X, ROWS, DIMS, lay, KNN_F64, NULL, KNN_F64, 0) == KNN_OK);
    at = g_nline;
    g_ncount = g_nlink = 0;
    MUST(dbscan(0) == KNN_OK && g_ncount == 3 && g_nlink == 3);
    MUST(has_line(at, "knn_launch_radius_scan fill 0") && has_line(at, "knn_launch_dbscan_link_scan"));
    MUST(!has_line(at, "knn_launch_radius_i8") && !has_line(at, "knn_launch_dbscan_link_i8") && accounted());
    for (long f = 1;; f++) {
        mark();
        const int rc = dbscan(f);
        if (rc == -1) break;
        faults++;
        MUST(rc != KNN_OK && marked() && accounted());
        MUST(dbscan(0) == KNN_OK);
        lines_clear();
    }
    MUST(knn_index_destroy(g_ix) == KNN_OK);
    MUST(g_nlive == 0 && g_nevents == 0 && g_nctx == 0);
    printf("ok: %d refusals, %ld faults\n", g_refusals, faults);
    return 0;
}
