/*
 * knn_cluster.c -- knn_dbscan_graph(): knn_index_dbscan's clustering
 * (include/knn.h has the definition) from the epsilon-graph
 * knn_index_radius_rows returns, on the host alone.  Host-only source: it
 * includes nothing but the public header, so that a stand-alone CPU program
 * can compile it by itself.
 *
 * The rules applied literally: N(x) = segment length + 1; a union-find over
 * the records that join two core rows, the larger root hooked under the
 * smaller, so that a component's root is its lowest position and the clusters
 * number themselves in one ascending walk; a border row takes the first core
 * record of its segment, the segments being ordered by (distance, id).
 */
#include "knn.h"

#include <stdlib.h>

/* the position of live id `id` (ids: m ascending ids, NULL = 1 .. m); -1: none */
static long long position_of(const int32_t *ids, size_t m, int32_t id)
{
    if (id < 1) return -1;
    if (!ids) return (size_t)id <= m ? (long long)id - 1 : -1;
    size_t lo = 0, hi = m;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < m && ids[lo] == id ? (long long)lo : -1;
}

static int32_t find(int32_t *parent, int32_t x)
{
    int32_t r = x;
    while (parent[r] != r) r = parent[r];
    while (parent[x] != r) {   /* compression */
        const int32_t next = parent[x];
        parent[x] = r;
        x = next;
    }
    return r;
}

int knn_dbscan_graph(const int64_t *indptr, const knn_neighbour_t *rec, const int32_t *ids, size_t m, int min_pts,
                     int32_t *cluster, int32_t *neighbours, int *nclusters)
{
    if (!indptr || !cluster || m == 0 || m > 0x7fffffffULL || min_pts < 1) return KNN_ERR_INVALID;
    for (size_t x = 0; x < m; x++)
        if (indptr[x + 1] < indptr[x]) return KNN_ERR_INVALID;
    const int64_t base = indptr[0], nrec = indptr[m] - base;
    if (nrec > 0 && !rec) return KNN_ERR_INVALID;
    /* pos[r]: record r's row as a position; parent, lab: by position */
    int32_t *pos = (int32_t *)malloc(((size_t)nrec + 1) * sizeof(int32_t));
    int32_t *parent = (int32_t *)malloc(2 * m * sizeof(int32_t));
    if (!pos || !parent) {
        free(pos);
        free(parent);
        return KNN_ERR_NOMEM;
    }
    int32_t *lab = parent + m;
    for (int64_t r = 0; r < nrec; r++) {
        const long long p = position_of(ids, m, rec[r].idx);
        if (p < 0) {
            free(pos);
            free(parent);
            return KNN_ERR_INVALID;
        }
        pos[r] = (int32_t)p;
    }
#define CORE(x_) (indptr[(x_) + 1] - indptr[x_] + 1 >= (int64_t)min_pts)
    for (size_t x = 0; x < m; x++) parent[x] = (int32_t)x;
    for (size_t x = 0; x < m; x++) {
        if (!CORE(x)) continue;
        for (int64_t r = indptr[x] - base; r < indptr[x + 1] - base; r++) {
            const size_t y = (size_t)pos[r];
            if (!CORE(y)) continue;
            const int32_t a = find(parent, (int32_t)x), b = find(parent, (int32_t)y);
            if (a < b) parent[b] = a;
            else if (b < a) parent[a] = b;
        }
    }
    int c = 0;
    for (size_t x = 0; x < m; x++) {   /* a root is met before its component's other rows */
        lab[x] = 0;
        if (!CORE(x)) continue;
        const int32_t r = find(parent, (int32_t)x);
        lab[x] = (size_t)r == x ? ++c : lab[r];
    }
    for (size_t x = 0; x < m; x++) {
        int32_t out = lab[x];
        if (!CORE(x))
            for (int64_t r = indptr[x] - base; r < indptr[x + 1] - base; r++)
                if (CORE((size_t)pos[r])) {
                    out = lab[pos[r]];
                    break;
                }
        cluster[x] = out;
        if (neighbours) neighbours[x] = (int32_t)(indptr[x + 1] - indptr[x] + 1);
    }
#undef CORE
    if (nclusters) *nclusters = c;
    free(pos);
    free(parent);
    return KNN_OK;
}
