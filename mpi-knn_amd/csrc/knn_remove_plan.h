/*
 * knn_remove_plan.h -- the host planning of knn_index_remove (knn_index.c):
 * sort and dedupe the ids, ids to internal positions, the survivors' local
 * source rows, and the (new block, old block, run) table of the stable
 * compaction.  Pure host code, static, no HIP call: knn_index.c includes it,
 * and so does the stand-alone program of tests/remove_plan.
 *
 * Terms.  The index holds m live rows at internal positions 0 .. m-1, in
 * blocks of `cap` rows (block b: positions b cap ..).  Row p carries the
 * external id map[p] (ascending in p), or p + 1 while the index has no map.
 * Removing a set of positions moves every survivor p to p - (removed
 * positions below p): survivors keep their order.
 */
#ifndef KNN_REMOVE_PLAN_H
#define KNN_REMOVE_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* `rows` rows of new block nb, from its row dst0 on, are the rows
 * list[list0 .. list0 + rows - 1] (local rows, ascending) of old block ob */
typedef struct {
    size_t nb, ob, dst0, rows, list0;
} knn_rm_run_t;

typedef struct {
    size_t removed;      /* live rows the call removes */
    size_t m1;           /* live rows after it */
    size_t p0;           /* the first removed position (removed > 0) */
    size_t b0;           /* the first rebuilt block, p0 / cap (moves) */
    size_t nb1;          /* blocks after the call */
    int moves;           /* 0: only trailing rows go, nothing is moved */
    int32_t *list;       /* the survivors from block b0 on: their local rows, run after run */
    size_t nlist;
    knn_rm_run_t *runs;
    size_t nruns;
    int32_t *ids;        /* the live ids after the call, ascending (m1 entries) */
} knn_rm_plan_t;

static int knn_rm_cmp_i32(const void *a, const void *b)
{
    const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
    return (x > y) - (x < y);
}

/* ids[0 .. count) sorted ascending, repeats dropped; returns the new count */
static size_t knn_rm_sort_dedupe(int32_t *ids, size_t count)
{
    if (count == 0) return 0;
    qsort(ids, count, sizeof(int32_t), knn_rm_cmp_i32);
    size_t w = 1;
    for (size_t i = 1; i < count; i++)
        if (ids[i] != ids[w - 1]) ids[w++] = ids[i];
    return w;
}

/* the position of a live id, or (size_t)-1: identity without a map (map ==
 * NULL: ids 1 .. m are live), binary search in the ascending map with one */
static size_t knn_rm_position(const int32_t *map, size_t m, int32_t id)
{
    if (!map) return id >= 1 && (size_t)id <= m ? (size_t)id - 1 : (size_t)-1;
    size_t lo = 0, hi = m;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (map[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < m && map[lo] == id ? lo : (size_t)-1;
}

/* sorted, deduped ids -> the ascending positions of those that are live (in
 * place: position <= id - 1 fits the entry); returns their count */
static size_t knn_rm_positions(const int32_t *map, size_t m, int32_t *ids, size_t count)
{
    size_t w = 0;
    for (size_t i = 0; i < count; i++) {
        const size_t p = knn_rm_position(map, m, ids[i]);
        if (p != (size_t)-1) ids[w++] = (int32_t)p;
    }
    return w;
}

static void knn_rm_plan_free(knn_rm_plan_t *pl)
{
    free(pl->list);
    free(pl->runs);
    free(pl->ids);
    memset(pl, 0, sizeof(*pl));
}

/* The plan of removing the ascending, distinct positions pos[0 .. npos), all
 * below m, from m live rows in blocks of cap (map: the live ids, or NULL).
 * npos == 0 gives an empty plan (removed = 0, m1 = m, no arrays).  Returns 0,
 * or -1 out of memory (the plan is then empty). */
static int knn_rm_plan(knn_rm_plan_t *pl, const int32_t *map, size_t m, size_t cap, const int32_t *pos, size_t npos)
{
    memset(pl, 0, sizeof(*pl));
    pl->removed = npos;
    pl->m1 = m - npos;
    pl->nb1 = (pl->m1 + cap - 1) / cap;
    if (npos == 0) return 0;
    pl->p0 = (size_t)pos[0];
    pl->b0 = pl->p0 / cap;
    /* the removed positions are the last npos ones: no survivor moves */
    pl->moves = pl->p0 != pl->m1;
    pl->ids = (int32_t *)malloc((pl->m1 ? pl->m1 : 1) * sizeof(int32_t));
    if (!pl->ids) return -1;
    {
        size_t w = 0, j = 0;
        for (size_t p = 0; p < m; p++) {
            if (j < npos && (size_t)pos[j] == p) {
                j++;
                continue;
            }
            pl->ids[w++] = map ? map[p] : (int32_t)(p + 1);
        }
    }
    if (!pl->moves) return 0;
    /* survivors from block b0 on; a run ends where the old or the new block does */
    const size_t first = pl->b0 * cap, nsurv = pl->m1 - first;
    const size_t maxruns = 2 * ((m - first + cap - 1) / cap) + 1;
    pl->list = (int32_t *)malloc(nsurv * sizeof(int32_t));
    pl->runs = (knn_rm_run_t *)malloc(maxruns * sizeof(knn_rm_run_t));
    if (!pl->list || !pl->runs) {
        knn_rm_plan_free(pl);
        return -1;
    }
    size_t q = first, j = 0;
    for (size_t p = first; p < m; p++) {
        if (j < npos && (size_t)pos[j] == p) {
            j++;
            continue;
        }
        knn_rm_run_t *r = pl->nruns ? &pl->runs[pl->nruns - 1] : NULL;
        if (!r || r->ob != p / cap || r->nb != q / cap) {
            r = &pl->runs[pl->nruns++];
            r->nb = q / cap;
            r->ob = p / cap;
            r->dst0 = q % cap;
            r->rows = 0;
            r->list0 = pl->nlist;
        }
        pl->list[pl->nlist++] = (int32_t)(p % cap);
        r->rows++;
        q++;
    }
    return 0;
}

#endif
