/*
 * update_plan.c -- the host planning of knn_index_update
 * (mpi-knn_amd/csrc/knn_update_plan.h) against a brute-force restatement.
 *
 * The model is the list of live ids in position order.  An update is stated
 * twice: by knn_up_plan, whose runs are then carried out on blocks of item
 * numbers exactly as the device scatters carry them out on rows, and as "the
 * row whose id is ids[i] takes source row i".  Both must leave the same item
 * in the same position, every other position untouched; the plan must keep
 * source order inside a block, visit blocks in ascending order, and report
 * ids that are not live and ids given twice.  Built by
 * tests/test_index_update_cpu.py, with the address and undefined-behaviour
 * sanitizers where the toolchain links them.
 */
#include <stdio.h>

#include "knn_update_plan.h"

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

/* one update of the ids raw[0 .. count) over the live ids live[0 .. m) */
static int update_case(const int32_t *live, size_t m, size_t cap, int has_map, const int32_t *raw, size_t count,
                       const char *what)
{
    cases++;
    /* brute force: what the call has to say, and which item lands where */
    int want = KNN_UP_OK;
    for (size_t i = 0; i < count && want != KNN_UP_DEAD; i++)
        if (find(live, m, raw[i]) < 0) want = KNN_UP_DEAD;
    for (size_t i = 0; i < count && want == KNN_UP_OK; i++)
        for (size_t j = 0; j < i; j++)
            if (raw[i] == raw[j]) want = KNN_UP_REPEAT;
    knn_up_plan_t pl;
    const int got = knn_up_plan(&pl, has_map ? live : NULL, m, cap, raw, count);
    CHECK(got == want);
    if (got != KNN_UP_OK) {
        CHECK(!pl.pos && !pl.srow && !pl.runs && pl.nruns == 0 && pl.count == 0);
        return 0;
    }
    const size_t nb = (m + cap - 1) / cap;
    long *land = (long *)malloc(nb * cap * sizeof(long));   /* the item a scatter wrote there, -1: none */
    for (size_t p = 0; p < nb * cap; p++) land[p] = -1;
    CHECK(pl.count == count && pl.nruns >= 1 && pl.nruns <= nb);
    size_t listed = 0;
    for (size_t r = 0; r < pl.nruns; r++) {
        const knn_up_run_t *run = &pl.runs[r];
        CHECK(run->rows > 0 && run->list0 == listed && run->list0 + run->rows <= count && run->blk < nb);
        if (r) CHECK(run->blk > run[-1].blk);   /* one run a touched block, ascending */
        for (size_t x = 0; x < run->rows; x++) {
            const int32_t lp = pl.pos[run->list0 + x], sr = pl.srow[run->list0 + x];
            CHECK(lp >= 0 && (size_t)lp < cap && run->blk * cap + (size_t)lp < m);
            CHECK(sr >= 0 && (size_t)sr < count);
            if (x) CHECK(pl.srow[run->list0 + x - 1] < sr);   /* source order inside a block */
            CHECK(land[run->blk * cap + (size_t)lp] == -1);   /* written once */
            land[run->blk * cap + (size_t)lp] = sr;
        }
        listed += run->rows;
    }
    CHECK(listed == count);
    /* every item where its id lives, nothing anywhere else */
    for (size_t i = 0; i < count; i++) CHECK(land[find(live, m, raw[i])] == (long)i);
    size_t written = 0;
    for (size_t p = 0; p < nb * cap; p++) written += land[p] >= 0;
    CHECK(written == count);
    free(land);
    knn_up_plan_free(&pl);
    CHECK(!pl.pos && !pl.srow && !pl.runs);
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

static void run_shape(size_t cap, size_t m, int has_map)
{
    char what[96];
    /* the live ids: 1 .. m, or (a map) an ascending selection of 1 .. 2 m */
    int32_t *live = (int32_t *)malloc(m * sizeof(int32_t));
    int32_t *raw = (int32_t *)malloc((m + 4) * sizeof(int32_t));
    int32_t last = 0;
    for (size_t p = 0; p < m; p++) live[p] = has_map ? (last += 1 + (int32_t)(rnd() % 3)) : (int32_t)(p + 1);
    const int32_t last_id = has_map ? last + 2 : (int32_t)m;
    snprintf(what, sizeof what, "cap %zu m %zu map %d", cap, m, has_map);

    /* the first row, the last, both sides of every block boundary */
    raw[0] = live[0];
    update_case(live, m, cap, has_map, raw, 1, what);
    raw[0] = live[m - 1];
    update_case(live, m, cap, has_map, raw, 1, what);
    for (size_t b = cap; b < m; b += cap) {
        size_t c = 0;
        if (b + 1 < m) raw[c++] = live[b + 1];
        raw[c++] = live[b - 1];
        raw[c++] = live[b];
        update_case(live, m, cap, has_map, raw, c, what);
    }
    /* every row: ascending, descending, shuffled */
    for (size_t p = 0; p < m; p++) raw[p] = live[p];
    update_case(live, m, cap, has_map, raw, m, what);
    for (size_t p = 0; p < m; p++) raw[p] = live[m - 1 - p];
    update_case(live, m, cap, has_map, raw, m, what);
    shuffle(raw, m);
    update_case(live, m, cap, has_map, raw, m, what);
    /* random subsets in random order */
    for (int round = 0; round < 12; round++) {
        for (size_t p = 0; p < m; p++) raw[p] = live[p];
        shuffle(raw, m);
        const size_t c = 1 + rnd() % m;
        update_case(live, m, cap, has_map, raw, c, what);
        /* a repeat, at both ends and in the middle */
        if (c >= 2) {
            int32_t keep = raw[c - 1];
            raw[c - 1] = raw[0];
            update_case(live, m, cap, has_map, raw, c, what);
            raw[c - 1] = keep;
            keep = raw[c / 2];
            raw[c / 2] = raw[c / 2 ? c / 2 - 1 : 1];
            update_case(live, m, cap, has_map, raw, c, what);
            raw[c / 2] = keep;
        }
        /* an id that is not live: past the last one, 0, negative, and (a map) a gap */
        int32_t dead[4] = {last_id + 1, 0, -5, 0};
        size_t nd = 3;
        for (int32_t id = 1; has_map && id < last; id++)
            if (find(live, m, id) < 0) {
                dead[nd++] = id;
                break;
            }
        for (size_t d = 0; d < nd; d++) {
            const size_t at = rnd() % c;
            const int32_t keep = raw[at];
            raw[at] = dead[d];
            update_case(live, m, cap, has_map, raw, c, what);
            raw[at] = keep;
        }
        /* dead and repeated: the dead id is what is reported */
        if (c >= 3) {
            raw[0] = raw[1];
            raw[2] = last_id + 1;
            update_case(live, m, cap, has_map, raw, c, what);
        }
    }
    free(live);
    free(raw);
}

int main(void)
{
    static const size_t caps[] = {1, 3, 128}, ms[] = {1, 2, 7, 128, 129, 700};
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 6; k++)
            for (int map = 0; map < 2; map++) run_shape(caps[c], ms[k], map);
    printf("%s: %d cases, %d failures\n", failures ? "FAILED" : "ok", cases, failures);
    return failures ? 1 : 0;
}
