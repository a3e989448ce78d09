/*
 * dbscan_graph.c -- knn_dbscan_graph (mpi-knn_amd/csrc/knn_cluster.c, compiled
 * alone with this file) on small hand-made epsilon-graphs: core, border and
 * noise rows, a border row between two clusters with and without a tie, the
 * clusters' numbering, live ids that are not 1 .. m, a shifted indptr, the
 * nullable outputs, and every refusal with no output written.
 * Prints "ok: G graphs, R refusals" or the first failure.
 */
#include "knn.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MAXM 16
#define MAXREC 256
#define MARK 0x5a5a5a5a

typedef struct {
    int a, b;   /* 0-based positions */
    double d;
} edge_t;

static int64_t g_ip[MAXM + 1];
static knn_neighbour_t g_rec[MAXREC];
static int g_graphs, g_refusals;

static int by_distance_id(const void *x, const void *y)
{
    const knn_neighbour_t *a = (const knn_neighbour_t *)x, *b = (const knn_neighbour_t *)y;
    if (a->distance != b->distance) return a->distance < b->distance ? -1 : 1;
    return a->idx < b->idx ? -1 : a->idx > b->idx;
}

/* the symmetric graph's CSR from offset `start`, idx the id (ids, or position + 1),
 * each segment by (distance, id) */
static void build(const edge_t *e, int ne, int m, const int32_t *ids, int64_t start)
{
    int64_t at = 0;
    for (int x = 0; x < m; x++) {
        g_ip[x] = start + at;
        const int64_t lo = at;
        for (int i = 0; i < ne; i++)
            for (int s = 0; s < 2; s++) {
                const int from = s ? e[i].b : e[i].a, to = s ? e[i].a : e[i].b;
                if (from != x) continue;
                g_rec[at].distance = e[i].d;
                g_rec[at].idx = ids ? ids[to] : to + 1;
                g_rec[at].label = 0;
                at++;
            }
        qsort(g_rec + lo, (size_t)(at - lo), sizeof(knn_neighbour_t), by_distance_id);
    }
    g_ip[m] = start + at;
}

#define MUST(cond)                                             \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAIL line %d: %s\n", __LINE__, #cond);     \
            return 1;                                          \
        }                                                      \
    } while (0)

static int expect(int line, int m, int min_pts, const int32_t *ids, const int *cluster, const int *nbr, int nc)
{
    int32_t cl[MAXM], nb[MAXM];
    int got = MARK;
    if (knn_dbscan_graph(g_ip, g_rec, ids, (size_t)m, min_pts, cl, nb, &got) != KNN_OK) {
        printf("FAIL line %d: not KNN_OK\n", line);
        return 1;
    }
    for (int x = 0; x < m; x++)
        if (cl[x] != cluster[x] || nb[x] != nbr[x]) {
            printf("FAIL line %d: row %d: cluster %d (want %d), neighbours %d (want %d)\n", line, x, cl[x], cluster[x],
                   nb[x], nbr[x]);
            return 1;
        }
    if (got != nc) {
        printf("FAIL line %d: %d clusters, want %d\n", line, got, nc);
        return 1;
    }
    /* the nullable outputs */
    int32_t cl2[MAXM];
    if (knn_dbscan_graph(g_ip, g_rec, ids, (size_t)m, min_pts, cl2, NULL, NULL) != KNN_OK ||
        memcmp(cl, cl2, (size_t)m * sizeof(int32_t))) {
        printf("FAIL line %d: without neighbours and nclusters\n", line);
        return 1;
    }
    g_graphs++;
    return 0;
}

static int32_t g_cl[MAXM], g_nb[MAXM];
static int g_nc;

static void mark(void)
{
    for (int i = 0; i < MAXM; i++) g_cl[i] = g_nb[i] = MARK;
    g_nc = MARK;
}

static int marked(void)
{
    for (int i = 0; i < MAXM; i++)
        if (g_cl[i] != MARK || g_nb[i] != MARK) return 0;
    return g_nc == MARK;
}

#define REFUSED(call)                                                                 \
    do {                                                                              \
        mark();                                                                       \
        const int rc_ = (call);                                                       \
        if (rc_ != KNN_ERR_INVALID || !marked()) {                                    \
            printf("FAIL line %d: %s -> %d, outputs %s\n", __LINE__, #call, rc_,      \
                   marked() ? "untouched" : "written");                               \
            return 1;                                                                 \
        }                                                                             \
        g_refusals++;                                                                 \
    } while (0)

int main(void)
{
    /* a triangle (core at min_pts 3), a row next to one corner (border), two rows alone (noise) */
    const edge_t tri[] = {{0, 1, 1.0}, {0, 2, 1.5}, {1, 2, 1.0}, {2, 3, 2.0}};
    build(tri, 4, 6, NULL, 0);
    MUST(!expect(__LINE__, 6, 3, NULL, (int[]){1, 1, 1, 1, 0, 0}, (int[]){3, 3, 4, 2, 1, 1}, 1));
    /* min_pts 1: every row core, no noise: the single rows are clusters of their own */
    MUST(!expect(__LINE__, 6, 1, NULL, (int[]){1, 1, 1, 1, 2, 3}, (int[]){3, 3, 4, 2, 1, 1}, 3));
    /* min_pts 4: row 2 alone is core; its neighbours are border rows */
    MUST(!expect(__LINE__, 6, 4, NULL, (int[]){1, 1, 1, 1, 0, 0}, (int[]){3, 3, 4, 2, 1, 1}, 1));
    /* min_pts 5: nothing is core */
    MUST(!expect(__LINE__, 6, 5, NULL, (int[]){0, 0, 0, 0, 0, 0}, (int[]){3, 3, 4, 2, 1, 1}, 0));

    /* two 4-cliques, rows 0 .. 3 and rows 5 .. 8, and row 4 between them, next
     * to row 3 and row 5 */
    edge_t two[14];
    int ne = 0;
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < 4; i++)
            for (int j = i + 1; j < 4; j++) two[ne++] = (edge_t){5 * c + i, 5 * c + j, 1.0};
    two[ne++] = (edge_t){4, 3, 2.0};
    two[ne++] = (edge_t){4, 5, 2.0};
    const int nb2[] = {4, 4, 4, 5, 3, 5, 4, 4, 4};
    build(two, ne, 9, NULL, 0);
    /* a tie at 2.0: the lower id, row 3's */
    MUST(!expect(__LINE__, 9, 4, NULL, (int[]){1, 1, 1, 1, 1, 2, 2, 2, 2}, nb2, 2));
    /* row 5 nearer: its cluster */
    two[ne - 1].d = 1.75;
    build(two, ne, 9, NULL, 0);
    MUST(!expect(__LINE__, 9, 4, NULL, (int[]){1, 1, 1, 1, 2, 2, 2, 2, 2}, nb2, 2));
    /* from any offset */
    build(two, ne, 9, NULL, 12345);
    MUST(!expect(__LINE__, 9, 4, NULL, (int[]){1, 1, 1, 1, 2, 2, 2, 2, 2}, nb2, 2));
    /* min_pts 3: row 4 is core and joins the two */
    MUST(!expect(__LINE__, 9, 3, NULL, (int[]){1, 1, 1, 1, 1, 1, 1, 1, 1}, nb2, 1));
    /* live ids after removals */
    const int32_t ids[9] = {2, 3, 5, 8, 13, 21, 34, 55, 89};
    build(two, ne, 9, ids, 7);
    MUST(!expect(__LINE__, 9, 4, ids, (int[]){1, 1, 1, 1, 2, 2, 2, 2, 2}, nb2, 2));
    /* a single row, no record */
    g_ip[0] = g_ip[1] = 0;
    MUST(!expect(__LINE__, 1, 1, NULL, (int[]){1}, (int[]){1}, 1));
    MUST(!expect(__LINE__, 1, 2, NULL, (int[]){0}, (int[]){1}, 0));
    mark();
    MUST(knn_dbscan_graph(g_ip, NULL, NULL, 1, 1, g_cl, NULL, NULL) == KNN_OK && g_cl[0] == 1);   /* rec unused */

    /* ---- refusals: nothing written */
    build(two, ne, 9, NULL, 0);
    REFUSED(knn_dbscan_graph(NULL, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc));
    REFUSED(knn_dbscan_graph(g_ip, NULL, NULL, 9, 4, g_cl, g_nb, &g_nc));
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 0, 4, g_cl, g_nb, &g_nc));
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 0, g_cl, g_nb, &g_nc));
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, -1, g_cl, g_nb, &g_nc));
    mark();
    MUST(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, NULL, g_nb, &g_nc) == KNN_ERR_INVALID && marked());
    g_refusals++;
    const int64_t keep = g_ip[3];
    g_ip[3] = g_ip[2] - 1;   /* decreases */
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc));
    g_ip[3] = keep;
    const int32_t was = g_rec[5].idx;
    g_rec[5].idx = 0;
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc));
    g_rec[5].idx = 10;   /* past m */
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc));
    g_rec[5].idx = -4;
    REFUSED(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc));
    g_rec[5].idx = was;
    REFUSED(knn_dbscan_graph(g_ip, g_rec, ids, 9, 4, g_cl, g_nb, &g_nc));   /* 1 .. 9 are not all live ids */
    MUST(knn_dbscan_graph(g_ip, g_rec, NULL, 9, 4, g_cl, g_nb, &g_nc) == KNN_OK && g_nc == 2);
    printf("ok: %d graphs, %d refusals\n", g_graphs, g_refusals);
    return 0;
}
