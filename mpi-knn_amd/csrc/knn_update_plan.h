/*
 * knn_update_plan.h -- the host planning of knn_index_update (knn_index.c):
 * ids to internal positions, the items grouped by block, and per touched
 * block one run of (local position, source row) pairs for one scatter
 * (knn_block_scatter_dt / _s8).  Pure host code, static, no HIP call:
 * knn_index.c includes it, and so does the stand-alone program of
 * tests/update_plan.  Terms and the id lookup: knn_remove_plan.h.
 *
 * Item i of an update gives the row with id ids[i] the values of source row
 * i.  No row moves, so the plan is a permutation of the items: stable by
 * block, source order kept inside a block.  Unlike a removal, an id that is
 * not live and an id given twice are errors: a dropped update is data loss.
 */
#ifndef KNN_UPDATE_PLAN_H
#define KNN_UPDATE_PLAN_H
#include "knn_remove_plan.h"

/* block blk: its rows pos[list0 .. list0 + rows) (local, in source order)
 * take the source rows srow[list0 .. list0 + rows) */
typedef struct {
    size_t blk, rows, list0;
} knn_up_run_t;

typedef struct {
    size_t count;        /* items: entries of pos and of srow */
    int32_t *pos;        /* local block rows, run after run */
    int32_t *srow;       /* the source rows they take */
    knn_up_run_t *runs;  /* one a touched block, ascending blocks */
    size_t nruns;
} knn_up_plan_t;

#define KNN_UP_OK 0
#define KNN_UP_NOMEM (-1)
#define KNN_UP_DEAD 1     /* an id that is not live (never was, or removed) */
#define KNN_UP_REPEAT 2   /* an id twice in the list */

typedef struct {
    int32_t p, i;   /* global position, item */
} knn_up_item_t;

static int knn_up_cmp_pos(const void *a, const void *b)
{
    const knn_up_item_t *x = (const knn_up_item_t *)a, *y = (const knn_up_item_t *)b;
    return (x->p > y->p) - (x->p < y->p);
}

static int knn_up_cmp_item(const void *a, const void *b)
{
    const knn_up_item_t *x = (const knn_up_item_t *)a, *y = (const knn_up_item_t *)b;
    return (x->i > y->i) - (x->i < y->i);
}

static void knn_up_plan_free(knn_up_plan_t *pl)
{
    free(pl->pos);
    free(pl->srow);
    free(pl->runs);
    memset(pl, 0, sizeof(*pl));
}

/* The plan of giving the rows ids[0 .. count) of m live rows in blocks of cap
 * (map: the live ids, or NULL) the source rows 0 .. count-1; count in
 * [1, INT32_MAX].  Returns KNN_UP_OK, or KNN_UP_DEAD / KNN_UP_REPEAT /
 * KNN_UP_NOMEM with the plan empty. */
static int knn_up_plan(knn_up_plan_t *pl, const int32_t *map, size_t m, size_t cap, const int32_t *ids, size_t count)
{
    memset(pl, 0, sizeof(*pl));
    knn_up_item_t *it = (knn_up_item_t *)malloc(count * sizeof(*it));
    if (!it) return KNN_UP_NOMEM;
    for (size_t i = 0; i < count; i++) {
        const size_t p = knn_rm_position(map, m, ids[i]);
        if (p == (size_t)-1) {
            free(it);
            return KNN_UP_DEAD;
        }
        it[i].p = (int32_t)p;
        it[i].i = (int32_t)i;
    }
    /* by position: a repeat is two neighbours, a block is a stretch */
    qsort(it, count, sizeof(*it), knn_up_cmp_pos);
    size_t nruns = 1;
    for (size_t i = 1; i < count; i++) {
        if (it[i].p == it[i - 1].p) {
            free(it);
            return KNN_UP_REPEAT;
        }
        nruns += (size_t)it[i].p / cap != (size_t)it[i - 1].p / cap;
    }
    pl->pos = (int32_t *)malloc(count * sizeof(int32_t));
    pl->srow = (int32_t *)malloc(count * sizeof(int32_t));
    pl->runs = (knn_up_run_t *)malloc(nruns * sizeof(knn_up_run_t));
    if (!pl->pos || !pl->srow || !pl->runs) {
        free(it);
        knn_up_plan_free(pl);
        return KNN_UP_NOMEM;
    }
    /* inside a block, back to source order (distinct items: the order is
     * total), and the positions to their block's base */
    for (size_t a = 0; a < count;) {
        const size_t b = (size_t)it[a].p / cap;
        size_t e = a;
        knn_up_run_t *r = &pl->runs[pl->nruns++];
        r->blk = b;
        r->list0 = a;
        while (e < count && (size_t)it[e].p / cap == b) e++;
        r->rows = e - a;
        qsort(it + a, e - a, sizeof(*it), knn_up_cmp_item);
        for (size_t x = a; x < e; x++) {
            pl->srow[x] = it[x].i;
            pl->pos[x] = (int32_t)((size_t)it[x].p - b * cap);
        }
        a = e;
    }
    pl->count = count;
    free(it);
    return KNN_UP_OK;
}

#endif
