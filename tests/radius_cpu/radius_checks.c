/*
 * radius_checks.c -- the four knn_index_radius* entry points on a CPU: every
 * argument refusal comes before any device call, a count / fill pair makes
 * the device calls it should and leaves the kept context alone, the index
 * accounts for every byte the calls keep, and a call that fails anywhere
 * leaves the index answering.
 *
 * A stand-alone program on tests/index_trace/index_trace.c's harness (its
 * stubs of the HIP runtime, the engine boundary and the launchers, its live
 * set and fault knob; its main is not used), with stubs of the three radius
 * launchers: every stub logs a line, so "no device call" is "no new line".
 * Prints "ok: R refusals, F faults" or the first failure.
 */
#define main index_trace_main
#include "../index_trace/index_trace.c"
#undef main

#include <math.h>

static int g_radius_launches, g_sorts;

int knn_launch_radius_i8(int fill, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
                         const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, int keep0, int32_t *counts,
                         const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream)
{
    (void)q_rows_pad, (void)c_rows_pad, (void)n, (void)indptr0, (void)out, (void)stream;
    L("knn_launch_radius_i8 fill %d q %s nq %d self %s nblk %d T %d keep0 %d counts %s indptr %s", fill, N(qs8), nq,
      N(self_pos), cb->nblk, T, keep0, N(counts), N(indptr));
    FALLIBLE("knn_launch_radius_i8", KNN_ERR_HIP);
    need(counts, (size_t)nq * sizeof(int32_t), "knn_launch_radius_i8");
    g_radius_launches++;
    return KNN_OK;
}

int knn_launch_radius_scan(int fill, int dtype, const void *qblk, int nq, const int32_t *self_pos,
                           const knn_radius_blocks_t *cb, int n, double radius, int keep0, int32_t *counts,
                           const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream)
{
    (void)dtype, (void)n, (void)indptr0, (void)out, (void)stream;
    L("knn_launch_radius_scan fill %d q %s nq %d self %s nblk %d r %g keep0 %d counts %s indptr %s", fill, N(qblk), nq,
      N(self_pos), cb->nblk, radius, keep0, N(counts), N(indptr));
    FALLIBLE("knn_launch_radius_scan", KNN_ERR_HIP);
    need(counts, (size_t)nq * sizeof(int32_t), "knn_launch_radius_scan");
    g_radius_launches++;
    return KNN_OK;
}

int knn_launch_radius_sort(size_t mq, const int32_t *cursor, const int64_t *indptr, knn_neighbour_t *out,
                           const int32_t *ids, int *flag, void *stream)
{
    (void)out, (void)stream;
    L("knn_launch_radius_sort mq %zu cursor %s indptr %s ids %s flag %s", mq, N(cursor), N(indptr), N(ids), N(flag));
    FALLIBLE("knn_launch_radius_sort", KNN_ERR_HIP);
    need(indptr, (mq + 1) * sizeof(int64_t), "knn_launch_radius_sort");
    need(flag, sizeof(int), "knn_launch_radius_sort");
    g_sorts++;
    return KNN_OK;
}

#define ROWS 600
#define MQ 40
static knn_index_t *g_ix;
static int32_t g_cnt[ROWS];
static int64_t g_ip[ROWS + 1];
static knn_neighbour_t g_rec[8];
static int g_refusals;

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

static int accounted(void)
{
    size_t bytes = 0;
    knn_index_info(g_ix, NULL, NULL, NULL, &bytes, NULL);
    return bytes == live_bytes('A');
}

static int has_line(int from, const char *prefix)
{
    for (int i = from; i < g_nline; i++)
        if (starts(g_line[i], prefix)) return 1;
    return 0;
}

/* the four calls, clean or with fault number `fault` in the one chosen */
static int four(int which, long fault, int flags)
{
    const int lay = KNN_ROWMAJOR;
    const int32_t ids[3] = {5, 300, 5};
    int rc[4];
    for (int i = 0; i < 4; i++) {
        g_calls = 0;
        g_fail_at = i == which ? fault : 0;
        rc[i] = i == 0   ? knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, 3.0, flags, g_cnt)
                : i == 1 ? knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 3.0, flags, g_ip, g_rec)
                : i == 2 ? knn_index_radius_rows_count(g_ix, ids, 3, 3.0, flags, g_cnt)
                         : knn_index_radius_rows(g_ix, NULL, 0, 3.0, flags, g_ip, g_rec);
        if (g_fail_at && g_calls < g_fail_at) rc[i] = -1;   /* past the call's last fallible step */
        g_fail_at = 0;
    }
    return which < 0 ? rc[0] | rc[1] | rc[2] | rc[3] : rc[which];
}

int main(void)
{
    const int lay = KNN_ROWMAJOR, KZ_ = KNN_QUERY_KEEP_ZERO;
    const double inf = INFINITY, nan_ = NAN;
    const int32_t ids[3] = {5, 300, 5}, bad_id[2] = {5, ROWS + 1}, dead[2] = {5, 7};
    int64_t down[MQ + 1] = {0}, neg[MQ + 1] = {0};
    down[1] = 1;   /* 0 1 0 ..: decreases */
    neg[0] = -1;
    setenv("KNN_QUERY_BLOCK", "256", 1);
    unsetenv("KNN_QUERY_TILE");
    unsetenv("KNN_NO_I8");
    g_kind = INT8;
    MUST(knn_index_create(&g_ix, g_X, ROWS, DIMS, lay, KNN_F64, NULL, KNN_F64, 0) == KNN_OK);

    /* ---- refusals: the query forms */
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(NULL, g_X, MQ, lay, KNN_F64, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, NULL, MQ, lay, KNN_F64, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 0, NULL));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, 0, lay, KNN_F64, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, 7, KNN_F64, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 8, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, -1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, -0.5, KZ_, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, nan_, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, inf, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_count(g_ix, g_X, (size_t)0x7fffffff - ROWS + 1, lay, KNN_F64, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_UNSUPPORTED, knn_index_radius_count(g_ix, g_X, MQ, lay, 9, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(NULL, g_X, MQ, lay, KNN_F64, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, NULL, MQ, lay, KNN_F64, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 0, NULL, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 0, g_ip, NULL));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, 0, lay, KNN_F64, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, 7, KNN_F64, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 16, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, -1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, nan_, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, inf, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 0, down, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, MQ, lay, KNN_F64, 1.0, 0, neg, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius(g_ix, g_X, (size_t)0x7fffffff, lay, KNN_F64, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_UNSUPPORTED, knn_index_radius(g_ix, g_X, MQ, lay, 9, 1.0, 0, g_ip, g_rec));

    /* ---- refusals: the rows forms (there is no source flag) */
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(NULL, ids, 3, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 3, 1.0, 0, NULL));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 0, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, NULL, 3, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 3, 1.0, KNN_INDEX_DEVICE_SRC, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 3, -1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 3, nan_, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, ids, 3, inf, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, bad_id, 2, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(NULL, ids, 3, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 3, 1.0, 0, NULL, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 3, 1.0, 0, g_ip, NULL));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 0, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, NULL, 3, 1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 3, 1.0, 32, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 3, -1.0, 0, g_ip, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, ids, 3, 1.0, 0, down, g_rec));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, bad_id, 2, 1.0, 0, g_ip, g_rec));
    MUST(accounted());

    /* ---- a query, the four calls, the query again: the context stays, and
     * the second query's trace is the first one's second half (no create) */
    MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK);
    const int nctx = g_nctx;
    int at = g_nline;
    MUST(four(-1, 0, KZ_) == KNN_OK);
    MUST(g_radius_launches == 4 && g_sorts == 2);             /* 3 blocks: one table a call */
    MUST(has_line(at, "knn_launch_radius_i8 fill 0") && has_line(at, "knn_launch_radius_i8 fill 1"));
    MUST(!has_line(at, "knn_launch_radius_scan") && !has_line(at, "knn_ctx_") && g_nctx == nctx);
    MUST(has_line(at, "knn_set_last_search_seconds") && accounted());
    at = g_nline;
    MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK);
    MUST(!has_line(at, "knn_ctx_create") && !has_line(at, "knn_ctx_destroy") && has_line(at, "knn_ctx_end"));
    MUST(accounted());

    /* ---- real-valued queries: the element path for the query forms only */
    g_kind = REAL;
    at = g_nline;
    g_radius_launches = 0;
    MUST(knn_index_radius_count(g_ix, g_X, MQ, lay, KNN_F64, 3.0, 0, g_cnt) == KNN_OK);
    MUST(has_line(at, "knn_launch_radius_scan fill 0") && !has_line(at, "knn_launch_radius_i8"));
    g_kind = INT8;

    /* ---- a dead id is refused before any device call */
    size_t removed = 0;
    MUST(knn_index_remove(g_ix, dead + 1, 1, 0, &removed) == KNN_OK && removed == 1);
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows_count(g_ix, dead, 2, 1.0, 0, g_cnt));
    REFUSED(KNN_ERR_INVALID, knn_index_radius_rows(g_ix, dead, 2, 1.0, 0, g_ip, g_rec));
    at = g_nline;
    MUST(four(-1, 0, 0) == KNN_OK && has_line(at, "knn_launch_radius_sort mq 599"));   /* every live row */

    /* ---- every fallible step of every call failed in turn */
    long faults = 0;
    for (int which = 0; which < 4; which++)
        for (long f = 1;; f++) {
            const int rc = four(which, f, KZ_);
            if (rc == -1) break;
            faults++;
            MUST(rc != KNN_OK);
            MUST(accounted());
            MUST(four(-1, 0, KZ_) == KNN_OK);
            MUST(knn_index_query(g_ix, g_X, MQ, lay, KNN_F64, 5, 0, g_out) == KNN_OK && g_nctx == nctx);
            lines_clear();
        }
    MUST(faults >= 40);
    MUST(knn_index_destroy(g_ix) == KNN_OK);
    MUST(g_nlive == 0 && g_nevents == 0 && g_nctx == 0);
    printf("ok: %d refusals, %ld faults\n", g_refusals, faults);
    return 0;
}
