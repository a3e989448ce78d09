// knn_predict.hip -- the index as a predictor: the distance-weighted vote and
// kNN regression over records that are still on the device
// (knn_index_classify_weighted / knn_index_regress and their _rows forms).
// Host twins: knn_classify_weighted / knn_regress in knn_vote.c, whose results
// these kernels give bit for bit; include/knn.h has the definition.
//
// k_vote_index's layout: one wave a query, four queries a workgroup.  The
// wave's lanes stride over the query's k <= 128 records and leave each one's
// weight, class (or target) in LDS; the zero-distance rule is one wave vote in
// between.  Classification: the lanes then stride over the CLASSES, and each
// walks the k cached records in record order, so every class sum is added in
// the order the host adds it whatever the lane count -- no atomics, no
// histogram in LDS (1024 doubles a wave would be 32 KiB a workgroup; this is
// 10 KiB).  The winner needs no histogram either: a lane remembers where it
// first met each of its classes, the largest sum is a wave maximum, and the
// tied class met first is a wave minimum over those positions.  Regression:
// lane 0 walks the cached records, two sums and one division.
//
// Nothing here may be fused or reordered: contraction is off for the whole
// file (the pragma below; the Makefile passes -ffp-contract=off as well), so a
// product and the sum it goes into are two roundings, as on the host.
#include "knn_device.h"

#pragma clang fp contract(off)

#define PREDICT_MAX_K 128   // KNN_MAX_K_F32: the records a wave caches

// w of a record at distance d; zero: the query has a valid record at distance 0
__device__ __forceinline__ double predict_weight(double d, int weights, bool zero)
{
    if (weights != KNN_WEIGHT_DISTANCE) return 1.0;
    if (zero) return d == 0.0 ? 1.0 : 0.0;
    return 1.0 / d;
}

// What the two kernels share: the lanes stride over query L's k records and
// cache w[i] and tag[i] -- REGRESS: tag 1 for a valid record, its target in
// y[i]; else tag the record's class when it is counted (1 .. nclasses), 0 when
// not, and .label written as vote_fill writes it.  Every lane may read the
// arrays on return.
template <bool REGRESS>
__device__ __forceinline__ void predict_fill(knn_neighbour_t *L, int k, int lane, int nclasses, int weights,
                                             const double *__restrict__ labels, long long nlabels, double *w,
                                             double *y, int *tag)
{
    bool zero = false;
    for (int i = lane; i < k; i += 64) {
        const int id = L[i].idx;
        const double d = L[i].distance;
        int t = 0;
        if (id > 0 && id <= nlabels) {
            const double v = labels[id - 1];
            if constexpr (REGRESS) {
                y[i] = v;
                t = 1;
            } else {
                const int lab = (int)v;
                L[i].label = lab;
                t = lab >= 1 && lab <= nclasses ? lab : 0;
            }
            zero |= d == 0.0;
        }
        w[i] = d;
        tag[i] = t;
    }
    zero = weights == KNN_WEIGHT_DISTANCE && __any(zero);
    for (int i = lane; i < k; i += 64) w[i] = predict_weight(w[i], weights, zero);   // (a lane's own entries)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void k_predict_classify(knn_neighbour_t *__restrict__ nb, int m, int k, int nclasses,
                                                          int weights, const double *__restrict__ labels,
                                                          long long nlabels, const double *__restrict__ qlab,
                                                          const int *__restrict__ own_ids, int *__restrict__ pred,
                                                          double *__restrict__ sums,
                                                          unsigned long long *__restrict__ matches)
{
    __shared__ double sw[4][PREDICT_MAX_K];
    __shared__ int stag[4][PREDICT_MAX_K];
    __shared__ unsigned hits[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    unsigned hit = 0;
    if (q < m) {
        const double *w = sw[wave];
        const int *tag = stag[wave];
        predict_fill<false>(nb + (size_t)q * k, k, lane, nclasses, weights, labels, nlabels, sw[wave], nullptr,
                            stag[wave]);
        // this lane's classes: each one's sum in record order, the largest of
        // them, and where the classes that reach it were first met
        double best = 0.0;
        int first = k;
        for (int j = lane; j < nclasses; j += 64) {
            double s = 0.0;
            int at = k;
            for (int i = 0; i < k; i++)
                if (tag[i] == j + 1) {
                    s = s + w[i];
                    at = at < i ? at : i;
                }
            if (sums) sums[(size_t)q * nclasses + j] = s;
            if (s > best) {
                best = s;
                first = at;
            } else if (s == best && at < first) {
                first = at;
            }
        }
        // the wave's: a NaN sum is nobody's maximum, as on the host
        double top = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(top, off);
            top = o > top ? o : top;
        }
        int at = top > 0.0 && best == top ? first : k;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(at, off);
            at = o < at ? o : at;
        }
        if (lane == 0) {
            const int most = at < k ? tag[at] : 0;
            pred[q] = most;
            if (matches) {
                if (qlab) {
                    hit = (double)most == qlab[q] ? 1u : 0u;
                } else {
                    const long long id = own_ids ? own_ids[q] : q + 1;
                    hit = (id >= 1 && id <= nlabels && (double)most == labels[id - 1]) ? 1u : 0u;
                }
            }
        }
    }
    if (lane == 0) hits[wave] = hit;
    __syncthreads();
    if (threadIdx.x == 0 && matches) {
        const unsigned h = hits[0] + hits[1] + hits[2] + hits[3];
        if (h) atomicAdd(matches, (unsigned long long)h);
    }
}

__global__ __launch_bounds__(256) void k_predict_regress(knn_neighbour_t *__restrict__ nb, int m, int k, int weights,
                                                         const double *__restrict__ targets, long long ntargets,
                                                         double *__restrict__ pred)
{
    __shared__ double sw[4][PREDICT_MAX_K];
    __shared__ double sy[4][PREDICT_MAX_K];
    __shared__ int stag[4][PREDICT_MAX_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= m) return;   // (no workgroup barrier below)
    predict_fill<true>(nb + (size_t)q * k, k, lane, 0, weights, targets, ntargets, sw[wave], sy[wave], stag[wave]);
    if (lane != 0) return;
    double num = 0.0, den = 0.0;
    bool seen = false;
    for (int i = 0; i < k; i++) {
        if (!stag[wave][i]) continue;
        const double w = sw[wave][i];
        const double p = w * sy[wave][i];
        num = num + p;
        den = den + w;
        seen = true;
    }
    pred[q] = seen ? num / den : __longlong_as_double(0x7ff8000000000000LL);
}

extern "C" int knn_launch_predict(knn_neighbour_t *nb, size_t mq, int k, int nclasses, int weights,
                                  const double *labels, size_t nlabels, const double *qlab, const int32_t *own_ids,
                                  void *pred, double *sums, unsigned long long *matches, void *stream)
{
    if (mq == 0) return KNN_OK;
    if (!nb || !labels || !pred || k <= 0 || nclasses < 0) return KNN_ERR_INVALID;
    if (weights != KNN_WEIGHT_UNIFORM && weights != KNN_WEIGHT_DISTANCE) return KNN_ERR_INVALID;
    if (k > PREDICT_MAX_K || nclasses > KNN_VOTE_MAX_CLASSES || mq > 0x7fffffffULL) return KNN_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((mq + 3) / 4)), block(256);
    if (nclasses == 0) {
        hipLaunchKernelGGL(k_predict_regress, grid, block, 0, s, nb, (int)mq, k, weights, labels, (long long)nlabels,
                           (double *)pred);
        return hip_status();
    }
    if (matches && hipMemsetAsync(matches, 0, sizeof(unsigned long long), s) != hipSuccess) return KNN_ERR_HIP;
    hipLaunchKernelGGL(k_predict_classify, grid, block, 0, s, nb, (int)mq, k, nclasses, weights, labels,
                       (long long)nlabels, qlab, own_ids, (int *)pred, sums, matches);
    return hip_status();
}
