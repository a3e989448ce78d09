/*
 * knn_radius_plan.h -- the integer threshold of the byte-path radius search
 * (knn_index_radius*, knn_radius.hip), on the host alone so that a CPU test
 * can compile it.
 *
 * On the byte path d^2 is an exact int32 and the reported distance is
 * sqrt((double)d^2), correctly rounded.  sqrt is monotone, so
 *     sqrt((double)d^2) <= r   <=>   d^2 <= T
 * for the one integer T with sqrt((double)T) <= r < sqrt((double)(T + 1)).
 * floor(r * r) is that T or next to it (r * r is rounded once); the loops below
 * settle it by comparing the correctly rounded square roots themselves, the
 * very comparison the element path makes.  d2max: the largest d^2 the data
 * can give (n * 255^2); an r at or past sqrt(d2max) is clamped to it, every
 * pair being a hit then.  r: finite, >= 0.
 */
#ifndef KNN_RADIUS_PLAN_H
#define KNN_RADIUS_PLAN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static inline int64_t knn_radius_d2max(size_t n) { return (int64_t)n * 255 * 255; }

static inline int64_t knn_radius_threshold(double r, int64_t d2max)
{
    if (!(r < sqrt((double)d2max))) return d2max;
    int64_t t = (int64_t)floor(r * r);   /* (r < sqrt(d2max) <= 2^13: no overflow) */
    if (t > d2max) t = d2max;
    while (t > 0 && sqrt((double)t) > r) t--;
    while (t < d2max && sqrt((double)(t + 1)) <= r) t++;
    return t;
}

/* The grid of a distance launch (knn_radius.hip): gx workgroups of queries
 * against nblk blocks of at most max_nc rows.  Rows of a chunk (a multiple of
 * `unit`) and the chunks a block, so that the launch has about 2048
 * workgroups.  On the host as well: knn_index_dbscan sizes its table of
 * per-chunk minima from *gy before the launch. */
static inline void knn_radius_chunks(unsigned gx, int nblk, int max_nc, int unit, int *rows_per_chunk, unsigned *gy)
{
    const long long wg = (long long)gx * nblk;
    long long chunks = (2048 + wg - 1) / wg;
    const long long most = (max_nc + unit - 1) / unit;
    if (chunks > most) chunks = most;
    if (chunks < 1) chunks = 1;
    const long long rpc = ((max_nc + chunks - 1) / chunks + unit - 1) / unit * unit;
    *rows_per_chunk = (int)rpc;
    *gy = (unsigned)((max_nc + rpc - 1) / rpc);
}

#endif
