/*
 * knn_vote.c -- knn_classify(): the label vote + accuracy stage.
 *
 * Rule SERIAL restates serial:104-130 and rule MPI blk:252-270 / nb:269-288,
 * including their quirk: `most` is compared as a vote count but
 * assigned a label, and ties go to the nearest neighbour's label (SERIAL) or
 * to that label minus one (MPI, blk:265).  Rule MAJORITY is a true
 * majority with ties to the tied label met first in neighbour order (not in
 * the reference).  Host code: m*k small integers, negligible next to the
 * search, and the reference excludes it from its timer (serial:94-98).
 */
#include "knn.h"
#include "knn_internal.h"

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* m queries' votes over `labels` (nlabels of them; 0: unchecked, as the
 * reference reads them); qlabels (nullable): the queries' own labels */
static int vote(const knn_neighbour_t *nb, size_t m, int k, int nclasses, int vote_rule,
                const double *labels, size_t nlabels, const double *qlabels, int *pred, size_t *matches)
{
    if (!nb || !labels || k <= 0 || nclasses <= 0 || nclasses > 65536) return KNN_ERR_INVALID;
    if (vote_rule != KNN_VOTE_SERIAL && vote_rule != KNN_VOTE_MPI &&
        vote_rule != KNN_VOTE_MAJORITY)
        return KNN_ERR_INVALID;
    int *cls = (int *)calloc((size_t)nclasses, sizeof(int));
    if (!cls) return KNN_ERR_NOMEM;
    size_t hit = 0;
    for (size_t q = 0; q < m; q++) {
        const knn_neighbour_t *L = nb + q * (size_t)k;
        memset(cls, 0, (size_t)nclasses * sizeof(int));          /* serial:114 */
        for (int i = 0; i < k; i++) {                             /* serial:116-119 */
            if (L[i].idx <= 0 || (nlabels && (size_t)L[i].idx > nlabels)) continue;   /* empty slot */
            const int lab = (int)labels[L[i].idx - 1];
            if (lab >= 1 && lab <= nclasses) cls[lab - 1]++;      /* F6: no class[-1] */
        }
        int most = 0;
        if (vote_rule == KNN_VOTE_MAJORITY) {
            int best = 0;
            for (int j = 0; j < nclasses; j++)
                if (cls[j] > best) best = cls[j];
            for (int i = 0; i < k && best > 0; i++) {
                if (L[i].idx <= 0 || (nlabels && (size_t)L[i].idx > nlabels)) continue;
                const int lab = (int)labels[L[i].idx - 1];
                if (lab >= 1 && lab <= nclasses && cls[lab - 1] == best) {
                    most = lab;
                    break;
                }
            }
        } else {
            const int nn0 = (L[0].idx > 0 && !(nlabels && (size_t)L[0].idx > nlabels)) ? (int)labels[L[0].idx - 1] : 0;
            const int tie = vote_rule == KNN_VOTE_MPI ? nn0 - 1 : nn0;  /* blk:265 vs serial:123 */
            for (int j = 0; j < nclasses; j++)                          /* serial:121-124 */
                if (cls[j] > most || ((cls[j] == most) && ((j + 1) == tie))) most = j + 1;
        }
        if (pred) pred[q] = most;
        if (qlabels && most == qlabels[q]) hit++;                 /* serial:126-127 */
    }
    free(cls);
    if (matches) *matches = hit;
    return KNN_OK;
}

int knn_classify(const knn_neighbour_t *nb, size_t m, int k, int nclasses, int vote_rule,
                 const double *labels, int *pred, size_t *matches)
{
    return vote(nb, m, k, nclasses, vote_rule, labels, 0, labels, pred, matches);
}

/* The vote of out-of-sample queries (knn_query's records): neighbours are
 * corpus rows 1..m with labels[idx - 1], the prediction is compared with
 * qlabels[q] (NULL: *matches = 0, only pred is written). */
int knn_classify_query(const knn_neighbour_t *nb, size_t mq, int k, int nclasses, int vote_rule,
                       const double *labels, size_t m, const double *qlabels, int *pred, size_t *matches)
{
    if (m == 0) return KNN_ERR_INVALID;
    return vote(nb, mq, k, nclasses, vote_rule, labels, m, qlabels, pred, matches);
}

/* The same stage on device-resident records (k_vote in knn_kernels.hip):
 * one wave per query, no host round trip between search and vote. */
int knn_classify_device(knn_neighbour_t *d_nb, size_t m, int k, int nclasses, int vote_rule,
                        const double *d_labels, size_t nlabels, size_t q_base, int *d_pred,
                        unsigned long long *d_matches, void *stream)
{
    if (!d_nb || !d_labels || k <= 0 || nclasses <= 0) return KNN_ERR_INVALID;
    if (vote_rule != KNN_VOTE_SERIAL && vote_rule != KNN_VOTE_MPI &&
        vote_rule != KNN_VOTE_MAJORITY)
        return KNN_ERR_INVALID;
    if (nclasses > KNN_VOTE_MAX_CLASSES) return KNN_ERR_UNSUPPORTED;
    return knn_launch_vote(d_nb, m, k, nclasses, vote_rule, d_labels, nlabels, q_base, d_pred,
                           d_matches, stream);
}

/* ---- the records as a predictor: knn_classify_weighted, knn_regress --------
 * include/knn.h has the definition; k_predict_classify / k_predict_regress
 * (knn_predict.hip) give these results bit for bit.  Every product and sum
 * below is a statement of its own, and the compiler may not fuse them. */
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

static int weights_ok(int weights) { return weights == KNN_WEIGHT_UNIFORM || weights == KNN_WEIGHT_DISTANCE; }

static int rec_valid(const knn_neighbour_t *r, size_t n) { return r->idx >= 1 && (size_t)r->idx <= n; }

/* a query's zero rule: a valid record at distance exactly 0 */
static int any_zero(const knn_neighbour_t *L, int k, size_t n)
{
    for (int i = 0; i < k; i++)
        if (rec_valid(L + i, n) && L[i].distance == 0.0) return 1;
    return 0;
}

static double rec_weight(double d, int weights, int zero)
{
    if (weights != KNN_WEIGHT_DISTANCE) return 1.0;
    if (zero) return d == 0.0 ? 1.0 : 0.0;
    const double w = 1.0 / d;
    return w;
}

int knn_classify_weighted(const knn_neighbour_t *nb, size_t mq, int k, int nclasses, int weights,
                          const double *labels, size_t nlabels, const double *qlabels, int *pred, double *sums,
                          size_t *matches)
{
    if (!nb || !labels || k <= 0 || nclasses <= 0 || nlabels == 0 || !weights_ok(weights)) return KNN_ERR_INVALID;
    double *own = sums ? NULL : (double *)malloc((size_t)nclasses * sizeof(double));
    if (!sums && !own) return KNN_ERR_NOMEM;
    size_t hit = 0;
    for (size_t q = 0; q < mq; q++) {
        const knn_neighbour_t *L = nb + q * (size_t)k;
        double *s = sums ? sums + q * (size_t)nclasses : own;
        const int zero = weights == KNN_WEIGHT_DISTANCE && any_zero(L, k, nlabels);
        for (int j = 0; j < nclasses; j++) s[j] = 0.0;
        for (int i = 0; i < k; i++) {
            if (!rec_valid(L + i, nlabels)) continue;
            const int lab = (int)labels[L[i].idx - 1];
            if (lab < 1 || lab > nclasses) continue;
            const double w = rec_weight(L[i].distance, weights, zero);
            const double t = s[lab - 1] + w;
            s[lab - 1] = t;
        }
        double best = 0.0;
        for (int j = 0; j < nclasses; j++)
            if (s[j] > best) best = s[j];
        int most = 0;
        for (int i = 0; i < k && best > 0.0; i++) {
            if (!rec_valid(L + i, nlabels)) continue;
            const int lab = (int)labels[L[i].idx - 1];
            if (lab >= 1 && lab <= nclasses && s[lab - 1] == best) {
                most = lab;
                break;
            }
        }
        if (pred) pred[q] = most;
        if (qlabels && most == qlabels[q]) hit++;
    }
    free(own);
    if (matches) *matches = hit;
    return KNN_OK;
}

int knn_regress(const knn_neighbour_t *nb, size_t mq, int k, int weights, const double *targets, size_t ntargets,
                double *pred)
{
    if (!nb || !targets || !pred || k <= 0 || ntargets == 0 || !weights_ok(weights)) return KNN_ERR_INVALID;
    for (size_t q = 0; q < mq; q++) {
        const knn_neighbour_t *L = nb + q * (size_t)k;
        const int zero = weights == KNN_WEIGHT_DISTANCE && any_zero(L, k, ntargets);
        double num = 0.0, den = 0.0;
        int seen = 0;
        for (int i = 0; i < k; i++) {
            if (!rec_valid(L + i, ntargets)) continue;
            const double w = rec_weight(L[i].distance, weights, zero);
            const double p = w * targets[L[i].idx - 1];
            num = num + p;
            den = den + w;
            seen = 1;
        }
        const double r = num / den;
        pred[q] = seen ? r : (double)NAN;
    }
    return KNN_OK;
}
