// knn_radius.hip -- radius search over the resident index (knn_index_radius*,
// include/knn.h): which live rows lie within distance r of a query, and how
// many.  Two distance kernels with variable-length output and a per-query
// sort; each distance kernel has a count form and a fill form (one template
// flag), and a call runs the same pass twice: count, then -- the caller having
// made the CSR offsets from the counts -- fill.
//
//   k_radius_i8    byte path: v_mfma_i32_32x32x32_i8 over the resident byte
//                  blocks and the byte query tile.  d^2 = |q'|^2 + |c'|^2 -
//                  2 q'.c' is an exact int32, and a pair is a hit when d^2 <= T,
//                  T the host's integer threshold (knn_radius_plan.h):
//                  sqrt((double)d^2) <= r exactly.
//   k_radius_scan  element path: the reference's arithmetic on every pair --
//                  S = S + (a - b)^2 in j order in fp64, no FMA -- and
//                  d = sqrt(S); d <= r && d < inf.  No filter: exact for all
//                  data.
//   k_radius_sort  each query's segment by (distance, position) -- positions
//                  ascend with ids, so this is the (distance, id) order -- and
//                  the records' idx from position to id.
//
// Count: per-lane counters, reduced, one integer add a query (integer sums:
// the result does not depend on the order).  Fill: a hit takes the next slot
// of its query's cursor (atomicAdd) and is written only when that slot lies
// inside the query's segment [indptr[q], indptr[q + 1]); the cursor ends at
// the query's number of hits, and k_radius_sort raises the call's flag where
// that differs from the segment's length.  The order in which the cursors
// hand out slots is arbitrary; the sort's keys (distance, position) are
// unique within a query, so the sorted segment is not.
//
// Both distance kernels take several corpus blocks in one launch through a
// block table (knn_radius_blocks_t: grid.z the block, grid.y a chunk of its
// rows); a block's rows past nc never hit.
//
// A third form of the same two loops, link, is knn_index_dbscan's second pass
// (include/knn.h has the definition): the queries are a resident block's own
// rows, and a hit is consumed where it is found -- two core rows are united in
// a lock-free union-find over parent[], a core row is offered to a row that
// is not core as its border winner -- and never written.  The O(m) kernels
// around the two passes (k_dbscan_*) are at the end of the file.
#include "knn_device.h"
#include "knn_i8_dev.h"
#include "knn_radius_plan.h"

#include <type_traits>

namespace {

// the launch's block blockIdx.z, picked with static indices (the kernel
// argument is never indexed dynamically)
struct radius_blk {
    const void *ptr;
    long long base;
    int nc;
};
__device__ __forceinline__ radius_blk radius_pick(const knn_radius_blocks_t &cb, int b)
{
    radius_blk o = {cb.ptr[0], cb.base[0], cb.nc[0]};
#pragma unroll
    for (int j = 1; j < KNN_RADIUS_MAXBLK; j++)
        if (j == b) {
            o.ptr = cb.ptr[j];
            o.base = cb.base[j];
            o.nc = cb.nc[j];
        }
    return o;
}

// what a distance kernel does with a hit
enum { RADIUS_COUNT = 0, RADIUS_FILL = 1, RADIUS_LINK = 2 };

// The link form's own arguments.  The queries are the rows at positions
// qbase .. of the index; nbr: every row's N(x) by position, a row is core when
// nbr >= min_pts.  border: the byte path's slot a row, the minimum of
// d^2 << 32 | position over the row's core neighbours (one 64-bit atomicMin is
// the whole (distance, id) rule: d^2 is an exact non-negative int32).  tab:
// the element path's minima, tab[chunk * nq + q] the (distance, position)
// minimum of query q over workgroup chunk blockIdx.z * gridDim.y + blockIdx.y
// (k_dbscan_border folds them: an (fp64, int32) key fits no atomic).
struct radius_link {
    const int32_t *nbr;
    int32_t *parent;
    unsigned long long *border;
    knn_neighbour_t *tab;
    int min_pts, qbase;
};

// Union-find over parent[], parent[x] <= x at all times: the only writes are a
// compare-and-swap that hooks a root under a lower position and an atomicMin
// that moves a row's parent to one of its ancestors.  So there are no cycles,
// a component's root is its lowest position, and no thread waits for another:
// a failed swap means another thread hooked that root, and the loop goes on
// from where it now points.  Reads are device-scope atomic loads (they are not
// served from a CU's L1, which nothing keeps coherent with another CU's
// atomics); a value read late is still an ancestor.
__device__ __forceinline__ int uf_load(const int32_t *parent, int x)
{
    return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    const int p0 = uf_load(parent, x);
    int r = p0, p;
    while ((p = uf_load(parent, r)) != r) r = p;
    if (r != p0) atomicMin(&parent[x], r);   // compression: x straight under the root found
    return r;
}

__device__ __forceinline__ void uf_union(int32_t *parent, int a, int b)
{
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(&parent[a], a, b);   // the larger root under the smaller
        if (old == a) return;
        a = uf_find(parent, old);
    }
}

// a hit (query at position qpos, row at position pos, pos != qpos) of the
// byte path's link form
__device__ __forceinline__ void link_hit_i8(const radius_link &lk, bool qcore, int qpos, int pos, int d2)
{
    if (lk.nbr[pos] < lk.min_pts) return;
    if (qcore) {
        if (pos < qpos) uf_union(lk.parent, qpos, pos);
    } else {
        atomicMin(&lk.border[qpos], ((unsigned long long)(unsigned)d2 << 32) | (unsigned)pos);
    }
}

// a hit of query q in fill mode: its slot from the cursor, written when inside
// the segment
__device__ __forceinline__ void radius_emit(int32_t *cursor, const int64_t *indptr, const int64_t *indptr0,
                                            knn_neighbour_t *out, int q, double d, int pos)
{
    const long long slot = atomicAdd(&cursor[q], 1);
    const long long lo = indptr[q], len = indptr[q + 1] - lo;
    if (slot < len) {
        knn_neighbour_t rec;
        rec.distance = d;
        rec.idx = pos;   // the position: k_radius_sort makes it the id
        rec.label = 0;
        out[lo - indptr0[0] + slot] = rec;
    }
}

// ---------------------------------------------------------------------------
// Byte path.  Workgroup: 4 waves, 128 queries (wave w: queries 32 w .. +31,
// held in VGPRs for the whole launch: KC chunks of 4 K-steps, 16 bytes a lane
// a K-step) against rows [row0, row1) of one block, 32 rows (one m-block) at a
// time.  Operands as k_dist_topk_i8: A = 32 corpus rows, B = the wave's 32
// queries, lane l (r = l & 31, h = l >> 5) supplies bytes [32 s + 16 h, +16)
// of K-step s of row r / query r; D: lane l holds query r, rows 8 (reg >> 2) +
// 4 h + (reg & 3) of the m-block.  The A fragments come straight from global
// memory, 16 bytes a lane: the 4 waves walk the same rows in step, so three
// of four reads hit the CU's cache.  |x'|^2 comes back out of the two norm
// words (i8_norm_of; rows of more than 4 K-steps keep a zero init word, which
// is not read), 16 consecutive words a lane (i8_norm_pos order).
// ---------------------------------------------------------------------------
template <int MODE, int KC>
__global__ __launch_bounds__(256) void k_radius_i8(const signed char *__restrict__ qrows,
                                                   const int *__restrict__ qnorm, int q_rows_pad, int nq,
                                                   const int32_t *__restrict__ self_pos, knn_radius_blocks_t cb,
                                                   int c_rows_pad, int rs, int rows_per_chunk, int T, int keep0,
                                                   int32_t *counts, const int64_t *indptr, const int64_t *indptr0,
                                                   knn_neighbour_t *out, radius_link lk)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int ks = rs >> 5;
    const bool longrow = i8_long_rows(rs);
    const radius_blk blk = radius_pick(cb, blockIdx.z);
    const int row0 = blockIdx.y * rows_per_chunk;   // (a multiple of 32)
    const int row1 = min(blk.nc, row0 + rows_per_chunk);
    if (row0 >= row1) return;                       // workgroup-uniform
    const int q = blockIdx.x * 128 + wave * 32 + r;
    const bool qv = q < nq;
    const int qc = qv ? q : nq - 1;                 // rows past nq: stale tile memory, not read
    knn_v4i qf[KC * 4];
#pragma unroll
    for (int s = 0; s < KC * 4; s++)
        qf[s] = s < ks ? *(const knn_v4i *)(qrows + (size_t)qc * rs + 32 * s + 16 * h) : (knn_v4i){0, 0, 0, 0};
    const int qn = i8_norm_of(qnorm[i8_norm_pos(qc)], longrow ? 0 : qnorm[q_rows_pad + i8_norm_pos(qc)]);
    int self = self_pos ? self_pos[qc] : -1;
    bool qcore = false;
    if constexpr (MODE == RADIUS_LINK) {
        self = lk.qbase + qc;   // the query is that row
        qcore = lk.nbr[self] >= lk.min_pts;
    }
    const signed char *crow = (const signed char *)blk.ptr;
    const int *cnorm = (const int *)(crow + (size_t)c_rows_pad * rs);
    int cnt = 0;
    for (int mb = row0; mb < row1; mb += 32) {
        const signed char *ar = crow + (size_t)(mb + r) * rs + 16 * h;
        knn_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < KC; c++) {
            knn_v4i a[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c < KC - 1 || 4 * c + u < ks) a[u] = *(const knn_v4i *)(ar + 32 * (4 * c + u));
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c < KC - 1 || 4 * c + u < ks)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], qf[4 * c + u], acc, 0, 0, 0);
        }
        // the lane's 16 rows' norm words: 16 consecutive ints
        const int *nw = cnorm + i8_norm_pos(mb + 4 * h);
        knn_v4i k2[4], iw[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            k2[j] = *(const knn_v4i *)(nw + 4 * j);
            iw[j] = longrow ? (knn_v4i){0, 0, 0, 0} : *(const knn_v4i *)(nw + c_rows_pad + 4 * j);
        }
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int row = mb + 8 * (reg >> 2) + 4 * h + (reg & 3);
            const int d2 = qn + i8_norm_of(k2[reg >> 2][reg & 3], iw[reg >> 2][reg & 3]) - 2 * acc[reg];
            const int pos = (int)(blk.base + row);
            const bool hit = qv && row < blk.nc && d2 <= T && (keep0 || d2 != 0) && pos != self;
            if constexpr (MODE == RADIUS_FILL) {
                if (hit) radius_emit(counts, indptr, indptr0, out, q, sqrt((double)d2), pos);
            } else if constexpr (MODE == RADIUS_LINK) {
                if (hit) link_hit_i8(lk, qcore, self, pos, d2);
            } else {
                cnt += hit ? 1 : 0;
            }
        }
    }
    if constexpr (MODE == RADIUS_COUNT) {
        cnt += __shfl_xor(cnt, 32);   // the query's other lane
        if (h == 0 && qv && cnt) atomicAdd(&counts[q], cnt);
    }
}

// ---------------------------------------------------------------------------
// Element path: k_rescan_step's loop.  A 256-thread workgroup takes 16
// queries, 4 a wave; the wave's query rows are wave-uniform (scalar loads),
// lane l streams rows l, l + 64, .. of the chunk with 16-byte loads and
// accumulates the 4 S in registers, so each streamed row serves 4 queries.
// Rows are zero padded to n_pad (whole 128 bytes) in query tiles and corpus
// blocks alike, and S + (0 - 0)^2 = S.
// ---------------------------------------------------------------------------
template <typename TE, int MODE>
__global__ __launch_bounds__(256) void k_radius_scan(const TE *__restrict__ qblk, int nq,
                                                     const int32_t *__restrict__ self_pos, knn_radius_blocks_t cb,
                                                     int n_pad, int rows_per_chunk, double radius, int keep0,
                                                     int32_t *counts, const int64_t *indptr, const int64_t *indptr0,
                                                     knn_neighbour_t *out, radius_link lk)
{
#pragma clang fp contract(off)
    constexpr int QW = 4, U = 8;
    constexpr int V = 16 / (int)sizeof(TE);
    typedef typename std::conditional<sizeof(TE) == 8, dbl2, flt4>::type vec_t;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int slot0 = blockIdx.x * 16 + wave * QW;
    if (slot0 >= nq) return;                          // wave-uniform (no workgroup barrier below)
    const radius_blk blk = radius_pick(cb, blockIdx.z);
    const int row0 = blockIdx.y * rows_per_chunk;
    const int row1 = min(blk.nc, row0 + rows_per_chunk);
    const TE *cblk = (const TE *)blk.ptr;
    const int nr = n_pad / V;
    const TE *qp[QW];
    int self[QW], cnt[QW];
    bool done[QW];
    // link: the query's core flag, and the lane's best core neighbour so far
    bool qcore[QW];
    double bd[QW];
    int bp[QW];
#pragma unroll
    for (int x = 0; x < QW; x++) {
        done[x] = slot0 + x >= nq;
        const int q = done[x] ? slot0 : slot0 + x;
        qp[x] = qblk + (size_t)q * n_pad;
        self[x] = self_pos ? self_pos[q] : -1;
        cnt[x] = 0;
        qcore[x] = false;
        bd[x] = KNN_INF;
        bp[x] = -1;
        if constexpr (MODE == RADIUS_LINK) {
            self[x] = lk.qbase + q;   // the query is that row
            qcore[x] = lk.nbr[self[x]] >= lk.min_pts;
        }
    }
    for (int row = row0 + lane; row < row1; row += 64) {
        const vec_t *cr = (const vec_t *)(cblk + (size_t)row * n_pad);
        double S[QW] = {0.0, 0.0, 0.0, 0.0};
        for (int p = 0; p < nr; p += U) {
            vec_t c[U];
#pragma unroll
            for (int u = 0; u < U; u++) c[u] = cr[p + u];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int x = 0; x < QW; x++) {
                    const vec_t a = ((const vec_t *)qp[x])[p + u];
#pragma unroll
                    for (int e = 0; e < V; e++) {
                        const double t = (double)a[e] - (double)c[u][e];
                        const double t2 = t * t;
                        S[x] = S[x] + t2;
                    }
                }
        }
        const int pos = (int)(blk.base + row);
#pragma unroll
        for (int x = 0; x < QW; x++) {
            const double d = sqrt(S[x]);
            const bool hit = !done[x] && d <= radius && d < KNN_INF && (keep0 || d != 0.0) && pos != self[x];
            if constexpr (MODE == RADIUS_FILL) {
                if (hit) radius_emit(counts, indptr, indptr0, out, slot0 + x, d, pos);
            } else if constexpr (MODE == RADIUS_LINK) {
                if (hit && lk.nbr[pos] >= lk.min_pts) {
                    if (qcore[x]) {
                        if (pos < self[x]) uf_union(lk.parent, self[x], pos);
                    } else if (bp[x] < 0 || d < bd[x]) {   // (the lane's positions ascend)
                        bd[x] = d;
                        bp[x] = pos;
                    }
                }
            } else {
                cnt[x] += hit ? 1 : 0;
            }
        }
    }
    if constexpr (MODE == RADIUS_LINK) {
        // Every wave that has queries writes its record a query, idx -1 where
        // the chunk is empty (row0 >= row1) or holds no core neighbour:
        // k_dbscan_border reads all gridDim.y * gridDim.z chunks of a query
        // and the table is never cleared.  This kernel must therefore keep no
        // early return for an empty chunk (k_radius_i8 has one).
        const size_t chunk = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
#pragma unroll
        for (int x = 0; x < QW; x++) {
            double d = bd[x];
            int p = bp[x];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double od = __shfl_xor(d, off);
                const int op = __shfl_xor(p, off);
                if (op >= 0 && (p < 0 || od < d || (od == d && op < p))) {
                    d = od;
                    p = op;
                }
            }
            if (lane == 0 && !done[x]) {
                knn_neighbour_t rec;
                rec.distance = d;
                rec.idx = p;
                rec.label = 0;
                lk.tab[chunk * (size_t)nq + slot0 + x] = rec;
            }
        }
    }
    if constexpr (MODE == RADIUS_COUNT) {
#pragma unroll
        for (int x = 0; x < QW; x++) {
            int c = cnt[x];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0 && !done[x] && c) atomicAdd(&counts[slot0 + x], c);
        }
    }
}

// ---------------------------------------------------------------------------
// Segment sort: one workgroup a query.  A bitonic network whose every
// compare-exchange puts the smaller key at the lower index (each merge opens
// with a "flip" step i <-> block end - i, then half-cleaners), so a segment of
// any length sorts as if padded with +inf to a power of two: a pair whose
// upper index is past the end is left alone.  Segments of at most
// KNN_RADIUS_SORT_LDS records are sorted in LDS, longer ones in place in
// global memory (the workgroup's barrier orders its own global accesses).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool radius_after(const knn_neighbour_t &a, const knn_neighbour_t &b)
{
    return a.distance > b.distance || (a.distance == b.distance && a.idx > b.idx);
}

template <typename P>
__device__ __forceinline__ void radius_sort_net(P a, size_t len)
{
    size_t pw = 1;
    while (pw < len) pw <<= 1;
    for (size_t k = 2; k <= pw; k <<= 1) {
        for (size_t j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == k >> 1;
            for (size_t t = threadIdx.x; t < pw >> 1; t += blockDim.x) {
                const size_t lo = 2 * j * (t / j) + t % j;
                const size_t hi = flip ? 2 * j * (t / j) + (2 * j - 1 - t % j) : lo + j;
                if (hi < len) {
                    const knn_neighbour_t x = a[lo], y = a[hi];
                    if (radius_after(x, y)) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_radius_sort(const int32_t *__restrict__ cursor,
                                                     const int64_t *__restrict__ indptr, knn_neighbour_t *out,
                                                     const int32_t *__restrict__ ids, int *flag)
{
    __shared__ knn_neighbour_t s[KNN_RADIUS_SORT_LDS];
    const size_t q = blockIdx.x;
    const long long lo = indptr[q], len = indptr[q + 1] - lo;
    if ((long long)cursor[q] != len) {                 // workgroup-uniform
        if (threadIdx.x == 0) atomicOr(flag, 1);
        return;
    }
    if (len <= 0) return;
    knn_neighbour_t *seg = out + (lo - indptr[0]);
    if (len <= KNN_RADIUS_SORT_LDS) {
        for (size_t i = threadIdx.x; i < (size_t)len; i += blockDim.x) s[i] = seg[i];
        __syncthreads();
        radius_sort_net(&s[0], (size_t)len);
        for (size_t i = threadIdx.x; i < (size_t)len; i += blockDim.x) {
            knn_neighbour_t rec = s[i];
            rec.idx = ids ? ids[rec.idx] : rec.idx + 1;
            seg[i] = rec;
        }
    } else {
        radius_sort_net(seg, (size_t)len);
        for (size_t i = threadIdx.x; i < (size_t)len; i += blockDim.x)
            seg[i].idx = ids ? ids[seg[i].idx] : seg[i].idx + 1;
    }
}

int radius_blocks_ok(const knn_radius_blocks_t *cb, int *max_nc)
{
    if (!cb || cb->nblk < 1 || cb->nblk > KNN_RADIUS_MAXBLK) return 0;
    *max_nc = 0;
    for (int b = 0; b < cb->nblk; b++) {
        if (!cb->ptr[b] || cb->nc[b] < 0) return 0;
        if (cb->nc[b] > *max_nc) *max_nc = cb->nc[b];
    }
    return 1;
}

template <int MODE, int KC>
void launch_radius_i8(dim3 grid, hipStream_t s, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
                      const knn_radius_blocks_t *cb, size_t c_rows_pad, int rs, int rpc, int T, int keep0,
                      int32_t *counts, const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out,
                      const radius_link &lk)
{
    const signed char *qrows = (const signed char *)qs8;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radius_i8<MODE, KC>), grid, dim3(256), 0, s, qrows,
                       (const int *)(qrows + q_rows_pad * (size_t)rs), (int)q_rows_pad, nq, self_pos, *cb,
                       (int)c_rows_pad, rs, rpc, T, keep0, counts, indptr, indptr0, out, lk);
}

#define RADIUS_I8_CASE(KC_)                                                                                          \
    case KC_:                                                                                                        \
        if (mode == RADIUS_FILL)                                                                                     \
            launch_radius_i8<RADIUS_FILL, KC_>(grid, s, qs8, q_rows_pad, nq, self_pos, cb, c_rows_pad, rs, rpc, T,   \
                                               keep0, counts, indptr, indptr0, out, lk);                             \
        else if (mode == RADIUS_LINK)                                                                                \
            launch_radius_i8<RADIUS_LINK, KC_>(grid, s, qs8, q_rows_pad, nq, self_pos, cb, c_rows_pad, rs, rpc, T,   \
                                               keep0, counts, indptr, indptr0, out, lk);                             \
        else                                                                                                         \
            launch_radius_i8<RADIUS_COUNT, KC_>(grid, s, qs8, q_rows_pad, nq, self_pos, cb, c_rows_pad, rs, rpc, T,  \
                                                keep0, counts, indptr, indptr0, out, lk);                            \
        break;

// the byte path's launch in any mode (lk: the link form's arguments, which
// stands in for counts there)
int radius_i8(int mode, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
              const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, int keep0, int32_t *counts,
              const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, const radius_link &lk, void *stream)
{
    int max_nc = 0;
    if (!qs8 || nq <= 0 || n <= 0 || n > KNN_I8_MAX_N || !radius_blocks_ok(cb, &max_nc)) return KNN_ERR_INVALID;
    if (mode == RADIUS_LINK ? !lk.nbr || !lk.parent || !lk.border || lk.qbase < 0 : !counts) return KNN_ERR_INVALID;
    if ((size_t)nq > q_rows_pad || (size_t)max_nc > c_rows_pad || T < 0) return KNN_ERR_INVALID;
    if (mode == RADIUS_FILL && (!indptr || !indptr0)) return KNN_ERR_INVALID;
    if (max_nc == 0) return KNN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int rs = (int)knn_s8_rs((size_t)n);
    const unsigned gx = (unsigned)((nq + 127) / 128);
    int rpc;
    unsigned gy;
    knn_radius_chunks(gx, cb->nblk, max_nc, 32, &rpc, &gy);
    const dim3 grid(gx, gy, (unsigned)cb->nblk);
    switch ((rs / 32 + 3) / 4) {
        RADIUS_I8_CASE(1)
        RADIUS_I8_CASE(2)
        RADIUS_I8_CASE(3)
        RADIUS_I8_CASE(4)
        RADIUS_I8_CASE(5)
        RADIUS_I8_CASE(6)
        RADIUS_I8_CASE(7)
    default:
        return KNN_ERR_INVALID;
    }
    return hip_status();
}

// the element path's launch in any mode; tab_cap: the entries lk.tab has room
// for (link: nq a chunk, *nchunk chunks)
int radius_scan(int mode, int dtype, const void *qblk, int nq, const int32_t *self_pos, const knn_radius_blocks_t *cb,
                int n, double radius, int keep0, int32_t *counts, const int64_t *indptr, const int64_t *indptr0,
                knn_neighbour_t *out, const radius_link &lk, size_t tab_cap, int *nchunk, void *stream)
{
    int max_nc = 0;
    if (!qblk || nq <= 0 || n <= 0 || !radius_blocks_ok(cb, &max_nc)) return KNN_ERR_INVALID;
    if (mode == RADIUS_LINK ? !lk.nbr || !lk.parent || !lk.tab || lk.qbase < 0 : !counts) return KNN_ERR_INVALID;
    if (dtype != KNN_F64 && dtype != KNN_F32) return KNN_ERR_INVALID;
    if (mode == RADIUS_FILL && (!indptr || !indptr0)) return KNN_ERR_INVALID;
    if (nchunk) *nchunk = 0;
    if (max_nc == 0) return KNN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int n_pad = (int)knn_n_pad_dt((size_t)n, dtype);
    const unsigned gx = (unsigned)((nq + 15) / 16);
    int rpc;
    unsigned gy;
    knn_radius_chunks(gx, cb->nblk, max_nc, 64, &rpc, &gy);
    const dim3 grid(gx, gy, (unsigned)cb->nblk);
    if (mode == RADIUS_LINK && (size_t)gy * (size_t)cb->nblk * (size_t)nq > tab_cap) return KNN_ERR_INVALID;
    if (nchunk) *nchunk = (int)(gy * (unsigned)cb->nblk);
#define RADIUS_SCAN(TE_, MODE_)                                                                                     \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radius_scan<TE_, MODE_>), grid, dim3(256), 0, s, (const TE_ *)qblk, nq,    \
                       self_pos, *cb, n_pad, rpc, radius, keep0, counts, indptr, indptr0, out, lk)
    if (dtype == KNN_F64) {
        if (mode == RADIUS_FILL) RADIUS_SCAN(double, RADIUS_FILL);
        else if (mode == RADIUS_LINK) RADIUS_SCAN(double, RADIUS_LINK);
        else RADIUS_SCAN(double, RADIUS_COUNT);
    } else {
        if (mode == RADIUS_FILL) RADIUS_SCAN(float, RADIUS_FILL);
        else if (mode == RADIUS_LINK) RADIUS_SCAN(float, RADIUS_LINK);
        else RADIUS_SCAN(float, RADIUS_COUNT);
    }
#undef RADIUS_SCAN
    return hip_status();
}

// ---------------------------------------------------------------------------
// knn_index_dbscan's O(m) kernels, one thread a row (position).
// ---------------------------------------------------------------------------

// the exclusive prefix of v over the workgroup's 256 threads; *sum: the total
__device__ __forceinline__ int block_scan_excl(int v, int *sum)
{
    __shared__ int ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) base += ws[w];
        tot += ws[w];
    }
    __syncthreads();   // ws is free for the next call
    *sum = tot;
    return base + inc - v;
}

// every row its own root, no border winner yet, no neighbour counted
__global__ __launch_bounds__(256) void k_dbscan_init(int32_t *nbr, int32_t *parent, void *border, int s8, int m)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    nbr[i] = 0;
    parent[i] = i;
    if (s8) {
        ((unsigned long long *)border)[i] = ~0ULL;
    } else {
        knn_neighbour_t none;
        none.distance = KNN_INF;
        none.idx = -1;
        none.label = 0;
        ((knn_neighbour_t *)border)[i] = none;
    }
}

// element path, behind each link launch: the launch's per-chunk minima of query
// q folded into the row's slot by (distance, position)
__global__ __launch_bounds__(256) void k_dbscan_border(const knn_neighbour_t *__restrict__ tab, int nq, int nchunk,
                                                       knn_neighbour_t *border, int qbase)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    knn_neighbour_t best = border[qbase + q];
    for (int c = 0; c < nchunk; c++) {
        const knn_neighbour_t t = tab[(size_t)c * nq + q];
        if (t.idx >= 0 && (best.idx < 0 || t.distance < best.distance ||
                           (t.distance == best.distance && t.idx < best.idx)))
            best = t;
    }
    border[qbase + q] = best;
}

// root[i]: a core row's component, its lowest position (parent is only read
// here); -1 for the others.  bsum[workgroup]: its rows that are their own root.
__global__ __launch_bounds__(256) void k_dbscan_roots(const int32_t *__restrict__ parent,
                                                      const int32_t *__restrict__ nbr, int min_pts, int m,
                                                      int32_t *root, int32_t *bsum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (i < m && nbr[i] >= min_pts) {
        r = i;
        int p;
        while ((p = parent[r]) != r) r = p;
    }
    if (i < m) root[i] = r;
    int tot;
    block_scan_excl(i < m && r == i, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// bsum -> its exclusive prefix, in place; bsum[nb]: the total, the number of
// clusters.  One workgroup.
__global__ __launch_bounds__(256) void k_dbscan_scan(int32_t *bsum, int nb)
{
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {   // (workgroup-uniform)
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        int tot;
        const int ex = block_scan_excl(v, &tot);
        if (b < nb) bsum[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

// rank[i]: a root's cluster number, 1 .. C in ascending position
__global__ __launch_bounds__(256) void k_dbscan_rank(const int32_t *__restrict__ root,
                                                     const int32_t *__restrict__ bsum, int m, int32_t *rank)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int is_root = i < m && root[i] == i;
    int tot;
    const int ex = block_scan_excl(is_root, &tot);
    if (i < m) rank[i] = is_root ? bsum[blockIdx.x] + ex + 1 : 0;
}

// cluster[i]: a core row's root's rank; a border row's winner's root's rank; 0
__global__ __launch_bounds__(256) void k_dbscan_label(const int32_t *__restrict__ root,
                                                      const int32_t *__restrict__ rank, const void *border, int s8,
                                                      int m, int32_t *cluster)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int at = root[i];
    if (at < 0) {
        int win;
        if (s8) {
            const unsigned long long key = ((const unsigned long long *)border)[i];
            win = key == ~0ULL ? -1 : (int)(unsigned)(key & 0xffffffffULL);
        } else {
            win = ((const knn_neighbour_t *)border)[i].idx;
        }
        at = win >= 0 ? root[win] : -1;
    }
    cluster[i] = at >= 0 ? rank[at] : 0;
}

}   // namespace

extern "C" int knn_launch_radius_i8(int fill, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
                                    const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, int keep0,
                                    int32_t *counts, const int64_t *indptr, const int64_t *indptr0,
                                    knn_neighbour_t *out, void *stream)
{
    const radius_link none = {};
    return radius_i8(fill ? RADIUS_FILL : RADIUS_COUNT, qs8, q_rows_pad, nq, self_pos, cb, c_rows_pad, n, T, keep0,
                     counts, indptr, indptr0, out, none, stream);
}

extern "C" int knn_launch_radius_scan(int fill, int dtype, const void *qblk, int nq, const int32_t *self_pos,
                                      const knn_radius_blocks_t *cb, int n, double radius, int keep0,
                                      int32_t *counts, const int64_t *indptr, const int64_t *indptr0,
                                      knn_neighbour_t *out, void *stream)
{
    const radius_link none = {};
    return radius_scan(fill ? RADIUS_FILL : RADIUS_COUNT, dtype, qblk, nq, self_pos, cb, n, radius, keep0, counts,
                       indptr, indptr0, out, none, 0, NULL, stream);
}

// ---- knn_index_dbscan's launchers (knn_internal.h) --------------------------

extern "C" int knn_launch_dbscan_init(int32_t *nbr, int32_t *parent, void *border, int s8, size_t m, void *stream)
{
    if (!nbr || !parent || !border || m == 0 || m > 0x7fffffffULL) return KNN_ERR_INVALID;
    hipLaunchKernelGGL(k_dbscan_init, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nbr, parent,
                       border, s8, (int)m);
    return hip_status();
}

extern "C" int knn_launch_dbscan_link_i8(const void *qs8, size_t q_rows_pad, int nq, int64_t qbase,
                                         const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T,
                                         const int32_t *nbr, int min_pts, int32_t *parent, void *border, void *stream)
{
    if (qbase < 0 || qbase > 0x7fffffffLL) return KNN_ERR_INVALID;
    const radius_link lk = {nbr, parent, (unsigned long long *)border, NULL, min_pts, (int)qbase};
    return radius_i8(RADIUS_LINK, qs8, q_rows_pad, nq, NULL, cb, c_rows_pad, n, T, 1, NULL, NULL, NULL, NULL, lk,
                     stream);
}

extern "C" int knn_launch_dbscan_link_scan(int dtype, const void *qblk, int nq, int64_t qbase,
                                           const knn_radius_blocks_t *cb, int n, double eps, const int32_t *nbr,
                                           int min_pts, int32_t *parent, void *border, void *tab, size_t tab_cap,
                                           void *stream)
{
    if (qbase < 0 || qbase > 0x7fffffffLL || !border) return KNN_ERR_INVALID;
    const radius_link lk = {nbr, parent, NULL, (knn_neighbour_t *)tab, min_pts, (int)qbase};
    int nchunk = 0;
    const int rc = radius_scan(RADIUS_LINK, dtype, qblk, nq, NULL, cb, n, eps, 1, NULL, NULL, NULL, NULL, lk, tab_cap,
                               &nchunk, stream);
    if (rc || !nchunk) return rc;
    hipLaunchKernelGGL(k_dbscan_border, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const knn_neighbour_t *)tab, nq, nchunk, (knn_neighbour_t *)border, (int)qbase);
    return hip_status();
}

extern "C" int knn_launch_dbscan_resolve(const int32_t *nbr, int min_pts, const int32_t *parent, const void *border,
                                         int s8, size_t m, int32_t *root, int32_t *rank, int32_t *bsum,
                                         int32_t *cluster, void *stream)
{
    if (!nbr || !parent || !border || !root || !rank || !bsum || !cluster || m == 0 || m > 0x7fffffffULL)
        return KNN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(k_dbscan_roots, dim3(nb), dim3(256), 0, s, parent, nbr, min_pts, (int)m, root, bsum);
    hipLaunchKernelGGL(k_dbscan_scan, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(k_dbscan_rank, dim3(nb), dim3(256), 0, s, (const int32_t *)root, (const int32_t *)bsum, (int)m,
                       rank);
    hipLaunchKernelGGL(k_dbscan_label, dim3(nb), dim3(256), 0, s, (const int32_t *)root, (const int32_t *)rank, border,
                       s8, (int)m, cluster);
    return hip_status();
}

extern "C" int knn_launch_radius_sort(size_t mq, const int32_t *cursor, const int64_t *indptr, knn_neighbour_t *out,
                                      const int32_t *ids, int *flag, void *stream)
{
    if (mq == 0) return KNN_OK;
    if (!cursor || !indptr || !flag || mq > 0x7fffffffULL) return KNN_ERR_INVALID;
    hipLaunchKernelGGL(k_radius_sort, dim3((unsigned)mq), dim3(256), 0, (hipStream_t)stream, cursor, indptr, out, ids,
                       flag);
    return hip_status();
}
