/*
 * neighbours_plan.c -- the host planning of knn_index_neighbours
 * (mpi-knn_amd/csrc/knn_neighbours_plan.h) against a brute-force restatement.
 *
 * The model is the list of live ids in position order.  A list of ids must
 * come back as the positions a linear search finds, in the order of the list
 * and with repeats kept; a NULL list as every position 0 .. m-1; and a list
 * with an id that is not live -- never handed out, out of range, or (a map) a
 * gap left by a removal -- must be reported.  Entries past `count` are never
 * written.  Built by tests/test_index_neighbours_cpu.py, with the address and
 * undefined-behaviour sanitizers where the toolchain links them.
 */
#include <stdio.h>

#include "knn_neighbours_plan.h"

static int failures, cases;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, what);  \
            failures++;                                                      \
            return -1;                                                       \
        }                                                                    \
    } while (0)

static unsigned rng_state = 2463534242u;
static unsigned rnd(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

/* brute force: the position of a live id, or -1 */
static long find(const int32_t *live, size_t m, int32_t id)
{
    for (size_t p = 0; p < m; p++)
        if (live[p] == id) return (long)p;
    return -1;
}

#define GUARD ((int32_t)0x5a5a5a5a)

/* the ids raw[0 .. count) over the live ids live[0 .. m) */
static int list_case(const int32_t *live, size_t m, int has_map, const int32_t *raw, size_t count, const char *what)
{
    cases++;
    int want = KNN_NB_OK;
    for (size_t i = 0; i < count; i++)
        if (find(live, m, raw[i]) < 0) want = KNN_NB_DEAD;
    /* exactly count entries, a guard behind them (the sanitizer sees the rest) */
    int32_t *pos = (int32_t *)malloc((count + 1) * sizeof(int32_t));
    for (size_t i = 0; i <= count; i++) pos[i] = GUARD;
    const int got = knn_nb_positions(has_map ? live : NULL, m, raw, count, pos);
    CHECK(got == want);
    CHECK(pos[count] == GUARD);
    if (got == KNN_NB_OK)
        for (size_t i = 0; i < count; i++) CHECK((long)pos[i] == find(live, m, raw[i]));   /* list order, repeats kept */
    free(pos);
    return 0;
}

/* ids == NULL: every live row, ascending */
static int all_case(const int32_t *live, size_t m, int has_map, const char *what)
{
    cases++;
    int32_t *pos = (int32_t *)malloc((m + 1) * sizeof(int32_t));
    for (size_t i = 0; i <= m; i++) pos[i] = GUARD;
    CHECK(knn_nb_positions(has_map ? live : NULL, m, NULL, 0, pos) == KNN_NB_OK);
    for (size_t p = 0; p < m; p++) CHECK(pos[p] == (int32_t)p);
    CHECK(pos[m] == GUARD);
    free(pos);
    return 0;
}

static void shuffle(int32_t *a, size_t n)
{
    for (size_t i = n; i > 1; i--) {
        const size_t j = rnd() % i;
        const int32_t t = a[i - 1];
        a[i - 1] = a[j];
        a[j] = t;
    }
}

static void run_shape(size_t m, int has_map)
{
    char what[96];
    /* the live ids: 1 .. m, or (a map) an ascending selection of 1 .. 3 m */
    int32_t *live = (int32_t *)malloc(m * sizeof(int32_t));
    int32_t *raw = (int32_t *)malloc((2 * m + 4) * sizeof(int32_t));
    int32_t last = 0;
    for (size_t p = 0; p < m; p++) live[p] = has_map ? (last += 1 + (int32_t)(rnd() % 3)) : (int32_t)(p + 1);
    const int32_t last_id = has_map ? last + 2 : (int32_t)m;
    snprintf(what, sizeof what, "m %zu map %d", m, has_map);

    all_case(live, m, has_map, what);
    /* count = 1: the first row, the last */
    raw[0] = live[0];
    list_case(live, m, has_map, raw, 1, what);
    raw[0] = live[m - 1];
    list_case(live, m, has_map, raw, 1, what);
    /* every row: ascending, descending, shuffled, and twice over */
    for (size_t p = 0; p < m; p++) raw[p] = live[p];
    list_case(live, m, has_map, raw, m, what);
    for (size_t p = 0; p < m; p++) raw[p] = live[m - 1 - p];
    list_case(live, m, has_map, raw, m, what);
    shuffle(raw, m);
    list_case(live, m, has_map, raw, m, what);
    for (size_t p = 0; p < m; p++) raw[m + p] = raw[p];
    list_case(live, m, has_map, raw, 2 * m, what);
    for (int round = 0; round < 12; round++) {
        /* random lists with repeats, in random order */
        const size_t c = 1 + rnd() % (2 * m);
        for (size_t i = 0; i < c; i++) raw[i] = live[rnd() % m];
        list_case(live, m, has_map, raw, c, what);
        /* one id repeated back to back, at both ends */
        raw[c - 1] = raw[0];
        if (c >= 2) raw[1] = raw[0];
        list_case(live, m, has_map, raw, c, what);
        /* an id that is not live: past the last one, 0, negative, INT32 limits, and (a map) a gap */
        int32_t dead[6] = {last_id + 1, 0, -5, INT32_MAX, INT32_MIN, 0};
        size_t nd = 5;
        for (int32_t id = 1; has_map && id < last; id++)
            if (find(live, m, id) < 0) {
                dead[nd++] = id;
                break;
            }
        for (size_t d = 0; d < nd; d++) {
            const size_t at = d == 0 ? 0 : d == 1 ? c - 1 : rnd() % c;
            const int32_t keep = raw[at];
            raw[at] = dead[d];
            list_case(live, m, has_map, raw, c, what);
            raw[at] = keep;
        }
    }
    free(live);
    free(raw);
}

int main(void)
{
    static const size_t ms[] = {1, 2, 7, 128, 129, 700};
    for (int k = 0; k < 6; k++)
        for (int map = 0; map < 2; map++) run_shape(ms[k], map);
    printf("%s: %d cases, %d failures\n", failures ? "FAILED" : "ok", cases, failures);
    return failures ? 1 : 0;
}
