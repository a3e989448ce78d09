/*
 * remove_plan.c -- the host planning of knn_index_remove
 * (mpi-knn_amd/csrc/knn_remove_plan.h) against a brute-force restatement.
 *
 * The model is the list of live ids in position order.  A removal is stated
 * twice: by the planning functions, whose run table is then carried out on
 * blocks of ids exactly as the device gathers carry it out on rows, and as
 * "keep every live id that is not in the list".  Both must leave the same ids
 * in the same positions.  Built by tests/test_index_remove_cpu.py, with the
 * address and undefined-behaviour sanitizers where the toolchain links them.
 */
#include <stdio.h>

#include "knn_remove_plan.h"

static int failures, cases;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, what);  \
            failures++;                                                      \
            return -1;                                                       \
        }                                                                    \
    } while (0)

typedef struct {
    int32_t *live;   /* ids in position order */
    size_t m, cap;
    int has_map;     /* the index keeps a map from its first removal on */
} model_t;

static int in_list(const int32_t *raw, size_t count, int32_t id)
{
    for (size_t i = 0; i < count; i++)
        if (raw[i] == id) return 1;
    return 0;
}

/* one removal of the raw id list; the model moves on to the survivors */
static int remove_case(model_t *M, const int32_t *raw, size_t count, const char *what)
{
    cases++;
    const size_t m = M->m, cap = M->cap;
    /* brute force: the survivors, in order */
    int32_t *want = (int32_t *)malloc((m + 1) * sizeof(int32_t));
    size_t m1 = 0, first_gone = m;
    for (size_t p = 0; p < m; p++) {
        if (in_list(raw, count, M->live[p])) {
            if (first_gone == m) first_gone = p;
        } else
            want[m1++] = M->live[p];
    }
    /* the planning */
    int32_t *pos = (int32_t *)malloc((count + 1) * sizeof(int32_t));
    memcpy(pos, raw, count * sizeof(int32_t));
    const size_t nu = knn_rm_sort_dedupe(pos, count);
    for (size_t i = 1; i < nu; i++) CHECK(pos[i - 1] < pos[i]);
    for (size_t i = 0; i < count; i++) CHECK(in_list(pos, nu, raw[i]));
    const size_t npos = knn_rm_positions(M->has_map ? M->live : NULL, m, pos, nu);
    CHECK(npos == m - m1);
    for (size_t i = 0; i < npos; i++) {
        CHECK(pos[i] >= 0 && (size_t)pos[i] < m && in_list(raw, count, M->live[pos[i]]));
        CHECK(i == 0 || pos[i - 1] < pos[i]);
    }
    knn_rm_plan_t pl;
    CHECK(knn_rm_plan(&pl, M->has_map ? M->live : NULL, m, cap, pos, npos) == 0);
    CHECK(pl.removed == npos && pl.m1 == m1 && pl.nb1 == (m1 + cap - 1) / cap);
    if (npos == 0) {
        CHECK(!pl.moves && !pl.ids && !pl.list && !pl.runs && pl.nruns == 0);
    } else {
        CHECK(pl.p0 == first_gone && pl.b0 == first_gone / cap);
        for (size_t p = 0; p < m1; p++) CHECK(pl.ids[p] == want[p]);
        /* only trailing rows go exactly when the survivors are a prefix */
        CHECK(pl.moves == (first_gone != m1));
        if (!pl.moves) CHECK(!pl.list && !pl.runs && pl.nruns == 0);
    }
    if (pl.moves) {
        /* carry the run table out on blocks of ids, as the gathers do on rows */
        const size_t nb0 = (m + cap - 1) / cap;
        int32_t *nw = (int32_t *)calloc(nb0 * cap, sizeof(int32_t));   /* 0: a row no gather wrote */
        size_t listed = 0;
        for (size_t r = 0; r < pl.nruns; r++) {
            const knn_rm_run_t *run = &pl.runs[r];
            CHECK(run->rows > 0 && run->list0 == listed && run->list0 + run->rows <= pl.nlist);
            CHECK(run->nb >= pl.b0 && run->nb < pl.nb1 && run->ob >= run->nb && run->ob < nb0);
            CHECK(run->dst0 + run->rows <= cap);
            /* one run for each (new block, old block) pair, in order */
            if (r) CHECK(run->nb > run[-1].nb || (run->nb == run[-1].nb && run->ob > run[-1].ob));
            for (size_t i = 0; i < run->rows; i++) {
                const int32_t l = pl.list[run->list0 + i];
                CHECK(l >= 0 && (size_t)l < cap && run->ob * cap + (size_t)l < m);
                CHECK(i == 0 || pl.list[run->list0 + i - 1] < l);
                CHECK(nw[run->nb * cap + run->dst0 + i] == 0);   /* written once */
                nw[run->nb * cap + run->dst0 + i] = M->live[run->ob * cap + (size_t)l];
            }
            listed += run->rows;
        }
        CHECK(listed == pl.nlist && pl.nlist == m1 - pl.b0 * cap);
        /* blocks in front of b0 stay; from b0 on the new blocks hold the survivors */
        for (size_t p = 0; p < pl.b0 * cap; p++) CHECK(M->live[p] == want[p]);
        for (size_t p = pl.b0 * cap; p < nb0 * cap; p++) CHECK(nw[p] == (p < m1 ? want[p] : 0));
        free(nw);
    }
    knn_rm_plan_free(&pl);
    free(pos);
    /* a removal that removed something leaves a map */
    if (npos) {
        memcpy(M->live, want, m1 * sizeof(int32_t));
        M->m = m1;
        M->has_map = 1;
    }
    free(want);
    return 0;
}

static model_t fresh(size_t cap, size_t nblk)
{
    model_t M;
    M.cap = cap;
    M.m = nblk * cap - 37;   /* a partial last block */
    M.live = (int32_t *)malloc(M.m * sizeof(int32_t));
    for (size_t p = 0; p < M.m; p++) M.live[p] = (int32_t)(p + 1);
    M.has_map = 0;
    return M;
}

static unsigned rng_state = 12345u;
static unsigned rnd(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static void run_shape(size_t cap, size_t nblk)
{
    char what[96];
    const size_t m = nblk * cap - 37;
    int32_t *raw = (int32_t *)malloc((2 * m + 8) * sizeof(int32_t));
    model_t M;

    /* the first row, then (on the map) the new first row and a stale id */
    snprintf(what, sizeof what, "cap %zu blocks %zu first row", cap, nblk);
    M = fresh(cap, nblk);
    raw[0] = 1;
    remove_case(&M, raw, 1, what);
    raw[0] = 1, raw[1] = 2, raw[2] = 2;
    remove_case(&M, raw, 3, what);
    /* only stale ids, repeated: empty after the lookup */
    raw[0] = 1, raw[1] = 2, raw[2] = 1;
    remove_case(&M, raw, 3, what);
    free(M.live);

    /* the last row; then the new last rows through the map: nothing moves */
    snprintf(what, sizeof what, "cap %zu blocks %zu last row", cap, nblk);
    M = fresh(cap, nblk);
    raw[0] = (int32_t)m;
    remove_case(&M, raw, 1, what);
    raw[0] = (int32_t)m - 1, raw[1] = (int32_t)m, raw[2] = (int32_t)m - 2;
    remove_case(&M, raw, 3, what);
    free(M.live);

    /* ids around a block boundary, descending and repeated */
    snprintf(what, sizeof what, "cap %zu blocks %zu boundary", cap, nblk);
    M = fresh(cap, nblk);
    if (nblk > 1) {
        raw[0] = (int32_t)cap + 1, raw[1] = (int32_t)cap, raw[2] = (int32_t)cap - 1, raw[3] = (int32_t)cap;
        remove_case(&M, raw, 4, what);
    }
    free(M.live);

    /* a whole block: the first, a middle one, the last (partial) one */
    for (int w = 0; w < 3 && nblk > 1; w++) {
        const size_t b = w == 0 ? 0 : w == 1 ? nblk / 2 : nblk - 1;
        if (w == 2 && b == nblk / 2) continue;
        snprintf(what, sizeof what, "cap %zu blocks %zu whole block %zu", cap, nblk, b);
        M = fresh(cap, nblk);
        size_t c = 0;
        for (size_t p = b * cap; p < (b + 1) * cap && p < m; p++) raw[c++] = (int32_t)(p + 1);
        remove_case(&M, raw, c, what);
        /* again: every id stale now */
        remove_case(&M, raw, c, what);
        free(M.live);
    }

    /* all rows but one: the first, one in the middle, the last */
    for (int w = 0; w < 3; w++) {
        snprintf(what, sizeof what, "cap %zu blocks %zu all but one (%d)", cap, nblk, w);
        M = fresh(cap, nblk);
        const size_t keep = w == 0 ? 0 : w == 1 ? m / 2 : m - 1;
        size_t c = 0;
        for (size_t p = m; p-- > 0;)
            if (p != keep) raw[c++] = (int32_t)(p + 1);
        remove_case(&M, raw, c, what);
        free(M.live);
    }

    /* random sets with repeats, one on top of the other (the second meets a
     * map, stale ids and ids of rows that moved) */
    for (int round = 0; round < 6; round++) {
        snprintf(what, sizeof what, "cap %zu blocks %zu random %d", cap, nblk, round);
        M = fresh(cap, nblk);
        for (int step = 0; step < 3 && M.m > 8; step++) {
            const size_t c = 1 + rnd() % (round < 2 ? 4 : M.m / 3 + 1);
            for (size_t i = 0; i < c; i++) raw[i] = 1 + (int32_t)(rnd() % m);
            if (c > 2) raw[c - 1] = raw[0];
            /* never every live row: the entry point refuses that before it plans */
            size_t gone = 0;
            for (size_t p = 0; p < M.m; p++) gone += (size_t)in_list(raw, c, M.live[p]);
            if (gone == M.m) continue;
            remove_case(&M, raw, c, what);
        }
        free(M.live);
    }
    free(raw);
}

int main(void)
{
    static const size_t caps[] = {128, 256}, blocks[] = {1, 2, 6};
    for (int c = 0; c < 2; c++)
        for (int b = 0; b < 3; b++) run_shape(caps[c], blocks[b]);
    /* the lookups on their own */
    {
        const char *what = "lookup";
        const int32_t map[] = {2, 3, 7, 11};
        cases++;
        if (knn_rm_position(map, 4, 7) != 2 || knn_rm_position(map, 4, 1) != (size_t)-1 ||
            knn_rm_position(map, 4, 12) != (size_t)-1 || knn_rm_position(map, 4, 5) != (size_t)-1 ||
            knn_rm_position(NULL, 4, 4) != 3 || knn_rm_position(NULL, 4, 5) != (size_t)-1 ||
            knn_rm_position(NULL, 4, 0) != (size_t)-1) {
            printf("FAIL %s\n", what);
            failures++;
        }
    }
    printf("%s: %d cases, %d failures\n", failures ? "FAILED" : "ok", cases, failures);
    return failures ? 1 : 0;
}
