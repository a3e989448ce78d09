/*
 * radius_threshold.c -- knn_radius_threshold (mpi-knn_amd/csrc/knn_radius_plan.h)
 * against its defining inequality, a stand-alone program:
 *     sqrt((double)T) <= r < sqrt((double)(T + 1)),   0 <= T <= d2max,
 * the right half waived only where T is the clamp d2max.  Swept: r =
 * sqrt((double)S) exactly for every integer S in a few ranges up to 896 *
 * 255^2, the doubles just below and just above each, r = 0, radii between
 * integers' roots, and radii at and beyond the clamp, for several d2max.
 * Prints "ok: N" (N radii checked) or the first failure.
 */
#include "knn_radius_plan.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>

static long g_n;

static void check(double r, int64_t d2max)
{
    const int64_t t = knn_radius_threshold(r, d2max);
    g_n++;
    if (t < 0 || t > d2max || !(sqrt((double)t) <= r) || (t < d2max && !(r < sqrt((double)(t + 1))))) {
        printf("FAIL: r = %.17g d2max = %lld T = %lld\n", r, (long long)d2max, (long long)t);
        exit(1);
    }
    /* the clamp takes every pair: nothing is cut off that could be a hit */
    if (t == d2max && !(r >= sqrt((double)d2max))) {
        printf("FAIL: clamped below sqrt(d2max): r = %.17g d2max = %lld\n", r, (long long)d2max);
        exit(1);
    }
}

static void around(int64_t s, int64_t d2max)
{
    const double r = sqrt((double)s);
    check(r, d2max);
    check(nextafter(r, 0.0), d2max);
    check(nextafter(r, INFINITY), d2max);
}

int main(void)
{
    const int64_t top = knn_radius_d2max(896);   /* 896 * 255^2 */
    const int64_t d2[] = {top, knn_radius_d2max(784), knn_radius_d2max(128), knn_radius_d2max(1), 1};
    if (top != 58262400) {
        printf("FAIL: d2max(896) = %lld\n", (long long)top);
        return 1;
    }
    for (size_t i = 0; i < sizeof(d2) / sizeof(d2[0]); i++) {
        const int64_t m = d2[i];
        check(0.0, m);
        check(DBL_MIN, m);
        check(0.5, m);
        check(DBL_MAX, m);
        check(1e9, m);
        around(m, m);
        around(m + 1, m);
        around(2 * m, m);
        for (int64_t s = 0; s <= 70000 && s <= m + 2; s++) around(s, m);
        for (int64_t s = m > 70000 ? m - 70000 : 0; s <= m + 2; s++) around(s, m);
    }
    /* ranges in the middle, perfect squares included, and a coarse walk over all of it */
    for (int64_t s = 3400000; s <= 3420000; s++) around(s, top);       /* around 1845^2: MNIST-like radii */
    for (int64_t s = 33554432 - 20000; s <= 33554432 + 20000; s++) around(s, top);   /* 2^25 */
    for (int64_t s = 0; s <= top; s += 977) around(s, top);
    for (int64_t k = 0; k <= 7633; k++) around(k * k, top);
    /* radii that are no integer's root */
    for (int i = 0; i < 200000; i++) check(7700.0 * (double)rand() / (double)RAND_MAX, top);
    printf("ok: %ld\n", g_n);
    return 0;
}
