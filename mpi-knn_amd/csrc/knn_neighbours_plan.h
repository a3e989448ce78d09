/*
 * knn_neighbours_plan.h -- the host planning of knn_index_neighbours
 * (knn_index.c): the listed ids to internal positions, in the caller's order.
 * Pure host code, static, no HIP call: knn_index.c includes it, and so does
 * the stand-alone program of tests/neighbours_plan.  Terms and the id lookup:
 * knn_remove_plan.h.
 *
 * The call only reads, so unlike an update a repeated id is no error: it gets
 * the same position again, and the answer rows come in the order of the list.
 * An id that is not live is refused, not skipped, as in an update: a missing
 * answer row would shift every later one.
 */
#ifndef KNN_NEIGHBOURS_PLAN_H
#define KNN_NEIGHBOURS_PLAN_H
#include "knn_remove_plan.h"

#define KNN_NB_OK 0
#define KNN_NB_DEAD 1   /* an id that is not live (never was, or removed) */

/* pos[i] = the position of the row with id ids[i], i < count, of m live rows
 * (map: the live ids, or NULL: id p + 1 at position p).  ids == NULL: every
 * live row in ascending id, pos[i] = i for i < m (count is not read; pos holds
 * m entries).  Returns KNN_NB_OK, or KNN_NB_DEAD at the first id that is not
 * live (pos is then unspecified). */
static int knn_nb_positions(const int32_t *map, size_t m, const int32_t *ids, size_t count, int32_t *pos)
{
    if (!ids) {
        for (size_t p = 0; p < m; p++) pos[p] = (int32_t)p;
        return KNN_NB_OK;
    }
    for (size_t i = 0; i < count; i++) {
        const size_t p = knn_rm_position(map, m, ids[i]);
        if (p == (size_t)-1) return KNN_NB_DEAD;
        pos[i] = (int32_t)p;
    }
    return KNN_NB_OK;
}

#endif
