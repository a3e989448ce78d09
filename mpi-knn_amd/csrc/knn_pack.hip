// knn_pack.hip -- the block writers: every kernel that writes a block image
// from a source array or from another block, and their launchers.  The
// search kernels (knn_kernels.hip, knn_i8.hip, knn_split.hip) only read what
// is written here (and k_shadow8's byte blocks, knn_i8.hip).
//
//   k_pack_col / k_pack_row      source -> element block (replaces the packing
//                of mpi-knn-parallel_blocking.c:100-109)
//   k_pack8_col / k_pack8_row / k_pack8_row_u8
//                source -> speculative byte block (knn_block_pack_s8)
//   k_shadow     element block -> fp16 shadow rows (the H16 == 2 contraction)
//   k_shadow_split   element blocks -> split fp16 rows (k_dist_split)
//   k_wire_pack / k_wire_unpack  element array <-> int16 ring wire form
//   k_gather_rows    listed rows of a block -> rows row0 .. of another block
//                (element and byte blocks: knn_block_gather_dt / _s8; from
//                several blocks by global position: knn_block_gather_pos_dt /
//                _s8)
//
// A source is fp64, fp32 or unsigned char (KNN_U8), column-major (ld >= rows)
// or row-major (ld >= n).  The images, rows_pad = round_up(capacity, 128):
//
//   element block of T (fp64 / fp32): rows_pad rows of n_pad = round_up(n,
//       128 / sizeof(T)) elements, zero past n and past the source's rows;
//       rows_pad squared norms as T; 8 meta doubles (KNN_META_*,
//       knn_internal.h).
//   byte block: rows_pad rows of rs = round_up(n, 32) bytes x - 128; rows_pad
//       slot words then rows_pad init words (int32, in i8_norm_pos order:
//       knn_device.h, 'Byte blocks'); the same 8 meta doubles, word
//       KNN_META_S8 set.
//   fp16 shadow: rows_pad rows of round_up(n, 64) halves.
//   split rows: rows_pad rows of round_up(n, 32) * 4 bytes: per 32 features,
//       32 halves hi then 32 halves lo.
//
// Pack, append and scatter are one launch path (launch_pack, launch_pack8): an
// append runs the kernels' KNN_APPEND instantiations over `rows` instead of
// rows_pad, at row0, without zeroing the meta first; a scatter runs the
// KNN_SCATTER ones the same way, with a listed block row (and source row) for
// every work item instead of row0.
#include "knn_device.h"

// The three forms of every pack kernel (its MODE argument) and where their
// rows go (its last argument): a pack's and an append's first block row (0 in a
// pack: the argument is not read), a scatter's lists.
enum { KNN_PACK = 0, KNN_APPEND = 1, KNN_SCATTER = 2 };
template <int MODE>
struct knn_dst_t {
    size_t row0;
};
template <>
struct knn_dst_t<KNN_SCATTER> {
    const int *pos;    // item i writes block row pos[i]; outside [0, cap): writes nothing
    const int *srow;   // and reads source row srow[i] (NULL: i); outside [0, src_rows): no row at all
    int src_rows, cap;
};
template <int MODE>
__device__ __forceinline__ size_t knn_dst_row0(const knn_dst_t<MODE> &d)
{
    if constexpr (MODE == KNN_SCATTER) return 0;
    else return d.row0;
}
// Item i of a scatter.  In: live = i < rows.  Out: live, it has a source row,
// sr; wr, it is written, to block row dr.  (An item without a source row is
// not written; one with a source row and no block row still reaches the meta.)
__device__ __forceinline__ void knn_scatter_item(const knn_dst_t<KNN_SCATTER> &d, size_t i, bool &live, size_t &sr,
                                                 size_t &dr, bool &wr)
{
    const int s = !live ? -1 : d.srow ? d.srow[i] : i < (size_t)d.src_rows ? (int)i : -1;
    const int p = live ? d.pos[i] : -1;
    live = (unsigned)s < (unsigned)d.src_rows;
    sr = live ? (size_t)s : 0;
    wr = live && (unsigned)p < (unsigned)d.cap;
    dr = wr ? (size_t)p : 0;
}
// the block rows of a workgroup's 64 items, -1 where none is written (the
// column kernels' SCATTER form: the thread that stores a row is not the one
// that read its item)
__device__ __forceinline__ int *knn_scatter_rows64()
{
    __shared__ int dp[64];
    return dp;
}

// ---------------------------------------------------------------------------
// Packing (blk:100-109): src (S = fp64, fp32 or unsigned char; col-major, ld >= rows |
// row-major, ld >= n) -> padded row-major block of T, the squared norms
// (fp64 accumulate, stored as T) and the meta (max|x|, max norm,
// non-integer, non-finite, max(x)+, max(-x)+), in ONE pass over the source
// (the norms are taken from the stored T values).  Per workgroup the meta
// is reduced, then one atomicMax per word (non-negative doubles order like
// their bits; the caller zeroes the meta).
// ---------------------------------------------------------------------------
// The meta words a lane accumulates, in two forms that compute the same
// values.  SEL = false, the branches, serves the pack instantiations
// (MODE = KNN_PACK), whose code was tuned and measured with it.  SEL = true,
// every update a select, serves the APPEND and SCATTER instantiations: there the
// compiler ends the branches in a store through a selected address, which
// keeps the struct in scratch memory, 24 bytes a lane; as selects it stays in
// registers.  One form for both would change the pack kernels' code.
template <bool SEL>
struct knn_meta_acc_t {
    double mabs = 0.0, nonint = 0.0, nonfin = 0.0, mpos = 0.0, mneg = 0.0;
    __device__ __forceinline__ void add(double v, double &s)
    {
        s = fma(v, v, s);
        if constexpr (SEL) {
            const bool fin = __builtin_isfinite(v);
            const double a = fabs(v);
            nonfin = fin ? nonfin : 1.0;
            mabs = fin && a > mabs ? a : mabs;
            mpos = fin && v > mpos ? v : mpos;
            mneg = fin && -v > mneg ? -v : mneg;
            nonint = fin && v != rint(v) ? 1.0 : nonint;
        } else if (!__builtin_isfinite(v)) nonfin = 1.0;
        else {
            const double a = fabs(v);
            mabs = a > mabs ? a : mabs;
            mpos = v > mpos ? v : mpos;
            mneg = -v > mneg ? -v : mneg;
            if (v != rint(v)) nonint = 1.0;
        }
    }
};

// workgroup reduction of the 6 meta words (64 W threads) + atomicMax
template <int W, typename A>
__device__ __forceinline__ void knn_meta_flush_w(const A &a, double mnorm, double *meta)
{
    __shared__ double red[W][6];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double w[6] = {a.mabs, mnorm, a.nonint, a.nonfin, a.mpos, a.mneg};
#pragma unroll
    for (int q = 0; q < 6; q++)
        for (int off = 32; off > 0; off >>= 1) w[q] = fmax(w[q], __shfl_xor(w[q], off));
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; q++) red[wave][q] = w[q];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int x = 1; x < W; x++) v = fmax(v, red[x][threadIdx.x]);
        if (!(v >= 0.0)) v = __builtin_inf();   // NaN norm -> treat as overflow
        atomicMax((unsigned long long *)&meta[threadIdx.x], (unsigned long long)__double_as_longlong(v));
    }
}
template <typename A>
__device__ __forceinline__ void knn_meta_flush(const A &a, double mnorm, double *meta)
{
    knn_meta_flush_w<4>(a, mnorm, meta);
}

// Column-major source (the .mat layout): a workgroup owns 64 rows and walks
// the columns in 64 x 64 tiles through LDS (reads: 64 consecutive rows of a
// column, 512 B; writes: 64 consecutive features of a row).  Thread (ty,
// tx) accumulates row tx's squared terms over columns = ty mod 4; the four
// partials are summed at the end (a fixed order).
//
// APPEND (knn_block_append_dt / _s8, every pack kernel below): the source's
// rows 0 .. rows-1 land at block rows row0 .. of a block packed before.  Only
// those rows, their norms and the meta are written (the grid covers `rows`,
// not rows_pad: padding rows are the first pack's), and the meta is
// atomicMax'ed into the words already there.  A row is summed by the same
// lanes in the same order wherever it lands, so pack + appends write the
// bytes one pack of all the rows writes.
//
// SCATTER (knn_block_scatter_dt / _s8, every pack kernel below): an append
// whose work item i reads source row srow[i] (i without a list) of a src_rows-row
// source and lands at block row pos[i] -- rows given new values in place.  The
// same lanes sum a row in the same order whichever source row it is and
// wherever it lands, so a block scattered into is, outside its meta, the block
// one pack of the updated array writes.
template <typename T, typename S, int MODE>
__global__ __launch_bounds__(256) void k_pack_col(T *__restrict__ blk, size_t rows, size_t rows_pad, int n,
                                                  int n_pad, const S *__restrict__ src, size_t ld,
                                                  const knn_dst_t<MODE> dst)
{
    constexpr bool SCATTER = MODE == KNN_SCATTER;
    __shared__ T tile[64][65];
    __shared__ double part[4][64];
    T *norms = blk + rows_pad * (size_t)n_pad;
    double *meta = (double *)(norms + rows_pad);
    const size_t lim = MODE != KNN_PACK ? rows : rows_pad;   // rows written; the first one's block row
    size_t d0 = 0;
    if constexpr (MODE == KNN_APPEND) d0 = dst.row0;
    const size_t i0 = (size_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t i = i0 + tx;
    size_t si = i;          // the item's source row
    bool live = i < rows;   // it has one
    int *dp = nullptr;
    if constexpr (SCATTER) {
        size_t dr;
        bool wr;
        knn_scatter_item(dst, i, live, si, dr, wr);
        dp = knn_scatter_rows64();
        if (ty == 0) dp[tx] = wr ? (int)dr : -1;   // (read behind the loop's first barrier)
    }
    knn_meta_acc_t<MODE != KNN_PACK> ma;
    double s = 0.0;
    for (int j0 = 0; j0 < n_pad; j0 += 64) {
#pragma unroll 4
        for (int jj = ty; jj < 64; jj += 4) {
            const int j = j0 + jj;
            const T v = (live && j < n) ? (T)src[si + (size_t)j * ld] : (T)0;
            tile[jj][tx] = v;
            ma.add((double)v, s);
        }
        __syncthreads();
        const int j = j0 + tx;
#pragma unroll 4
        for (int ii = ty; ii < 64; ii += 4) {
            if constexpr (SCATTER) {
                if (dp[ii] >= 0 && j < n_pad) blk[(size_t)dp[ii] * n_pad + j] = tile[tx][ii];
            } else if (i0 + ii < lim && j < n_pad)
                blk[(d0 + i0 + ii) * n_pad + j] = tile[tx][ii];
        }
        __syncthreads();
    }
    part[ty][tx] = s;
    __syncthreads();
    double mnorm = 0.0;
    if (ty == 0 && (SCATTER ? live : i < lim)) {
        const double nr = (part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]);
        if constexpr (SCATTER) {
            if (dp[tx] >= 0) norms[dp[tx]] = (T)nr;
        } else
            norms[d0 + i] = (T)nr;
        if (nr == nr) mnorm = nr;
        else ma.nonfin = 1.0;
    }
    knn_meta_flush(ma, mnorm, meta);
}

// ---------------------------------------------------------------------------
// Speculative byte block straight from the source (knn_block_pack_s8): the
// int8 contraction's rows x' = x - 128 (rows of rs = round_up(n, 32) bytes,
// zero past n and on padding rows), its norm words (i8_norm_word of the
// exact int32 |x'|^2) and the block meta of the element pack above (the same
// six words over the values as T).  The shift the int8 path uses is
// o = 128 - max(-x)+ of the reduced meta (knn_i8.hip), so the image is the
// one k_shadow8 would write exactly when every value is an integer in
// [0, 255] -- knn_s8_spec_ok on the reduced meta (MNIST pixels, SIFT
// descriptors); otherwise the caller packs the element block after all.  One
// read of the source and 1 byte written an element, instead of the element
// block (8 or 4 bytes written, read back by k_shadow8).
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ int knn_spec8(T v)
{
    // x - 128 of an in-window integer; anything else gives garbage the meta
    // rejects: NaN -> 0 and a clamp to [-32640, 32895], so the conversion is
    // defined and (x - 128)^2 < 2^31 (the squares are summed as unsigned)
    const T c = v == v ? (v < (T)-32640 ? (T)-32640 : (v > (T)32895 ? (T)32895 : v)) : (T)0;
    return (int)c - 128;
}

// col-major source (the .mat layout): a workgroup owns RW rows and walks
// the columns in 64-column tiles (RW = 64: each wave reads 64 consecutive
// rows of one column, 512-byte runs; RW = 32: two columns of 32 rows a
// wave), all of a thread's loads of a tile in flight before their
// conversion; bytes go through LDS into 16-byte row stores.  Thread (ty, tx)
// sums row tx's squares over columns = ty mod (256 / RW); the partials add
// exactly for the integer data the byte block holds (the meta decides
// that; rejected data is packed again from elements).
// (Issuing the next tile's loads before converting this one -- 32 in
// flight at RW = 64 -- measured slower: 106 -> 130 us for MNIST, rocprofv3.)
template <typename T, typename S, int RW, int MODE>
__global__ __launch_bounds__(256) void k_pack8_col(signed char *__restrict__ dst, size_t rows, size_t rows_pad,
                                                   int n, int rs, const S *__restrict__ src, size_t ld,
                                                   const knn_dst_t<MODE> to)
{
    constexpr bool SCATTER = MODE == KNN_SCATTER;
    static_assert(!SCATTER || RW == 64, "knn_scatter_rows64");
    constexpr int CG = 256 / RW;      // column groups
    const size_t lim = MODE != KNN_PACK ? rows : rows_pad;
    size_t d0 = 0;
    if constexpr (MODE == KNN_APPEND) d0 = to.row0;
    constexpr int NE = 64 / CG;       // loads a thread a tile
    __shared__ unsigned char tb[64][RW + 4];   // [column of the tile][row]
    __shared__ double part[CG][RW];
    __shared__ unsigned ipart[CG][RW];
    int *norms = (int *)(dst + rows_pad * (size_t)rs);
    double *meta = (double *)(norms + 2 * rows_pad);
    const size_t i0 = (size_t)blockIdx.x * RW;
    const int tx = threadIdx.x % RW, ty = threadIdx.x / RW;
    const size_t i = i0 + tx;
    bool live = i < rows;   // the item has a source row
    const S *xp = src + (live ? i : 0);
    int *dp = nullptr;
    if constexpr (SCATTER) {
        size_t sr, dr;
        bool wr;
        knn_scatter_item(to, i, live, sr, dr, wr);
        xp = src + sr;
        dp = knn_scatter_rows64();
        if (ty == 0) dp[tx] = wr ? (int)dr : -1;   // (read behind the loop's first barrier)
    }
    knn_meta_acc_t<MODE != KNN_PACK> ma;
    double s = 0.0;
    unsigned si = 0u;
    for (int j0 = 0; j0 < rs; j0 += 64) {
        S v[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int j = j0 + ty + CG * e;
            v[e] = (live && j < n) ? __builtin_nontemporal_load(xp + (size_t)j * ld) : (S)0;
        }
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const T x = (T)v[e];
            ma.add((double)x, s);
            const int xi = (live && j0 + ty + CG * e < n) ? knn_spec8(x) : 0;
            si += (unsigned)(xi * xi);
            tb[ty + CG * e][tx] = (unsigned char)xi;
        }
        __syncthreads();
        // row r = t / 4: 16 bytes at column 16 (t % 4) of the tile
        const int r = threadIdx.x >> 2, c0 = 16 * (threadIdx.x & 3);
        auto put = [&](size_t dr) {   // item i0 + r to block row dr
            unsigned w4[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
                w4[q] = (unsigned)tb[c0 + 4 * q][r] | ((unsigned)tb[c0 + 4 * q + 1][r] << 8) |
                        ((unsigned)tb[c0 + 4 * q + 2][r] << 16) | ((unsigned)tb[c0 + 4 * q + 3][r] << 24);
            *(knn_v4i *)(dst + dr * (size_t)rs + j0 + c0) = (knn_v4i){(int)w4[0], (int)w4[1], (int)w4[2], (int)w4[3]};
        };
        if constexpr (SCATTER) {
            if (dp[r] >= 0 && j0 + c0 < rs) put((size_t)dp[r]);
        } else if (r < RW && i0 + r < lim && j0 + c0 < rs)
            put(d0 + i0 + r);
        __syncthreads();
    }
    part[ty][tx] = s;
    ipart[ty][tx] = si;
    __syncthreads();
    double mnorm = 0.0;
    if (ty == 0 && (SCATTER ? live : i < lim)) {
        double nr = 0.0;
        unsigned ni = 0u;
        if constexpr (CG == 4) {
            nr = (part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]);
            ni = (ipart[0][tx] + ipart[1][tx]) + (ipart[2][tx] + ipart[3][tx]);
        } else {
#pragma unroll
            for (int q = 0; q < CG; q++) {
                nr += part[q][tx];
                ni += ipart[q][tx];
            }
        }
        if constexpr (SCATTER) {
            if (dp[tx] >= 0) {
                norms[i8_norm_pos(dp[tx])] = i8_norm_word(dp[tx], (int)ni, rs);
                norms[rows_pad + i8_norm_pos(dp[tx])] = i8_init_word((int)ni, rs);
            }
        } else {
            norms[i8_norm_pos((int)(d0 + i))] = i8_norm_word((int)(d0 + i), (int)ni, rs);
            norms[rows_pad + i8_norm_pos((int)(d0 + i))] = i8_init_word((int)ni, rs);
        }
        if (nr == nr) mnorm = nr;
        else ma.nonfin = 1.0;
    }
    knn_meta_flush(ma, mnorm, meta);
    if (MODE == KNN_PACK && blockIdx.x == 0 && threadIdx.x == 0) meta[KNN_META_S8] = 1.0;   // (an append finds it set)
}

// row-major source: one wave per row, lane l converts the 8-element groups
// l, l + 64, ... (one 8-byte store each); VEC: 16-byte-aligned rows, whole
// groups read as 16-byte vectors (sift: 0.68 ms for 512 MB with scalar loads)
template <typename T, typename S, bool VEC, int MODE>
__global__ __launch_bounds__(256) void k_pack8_row(signed char *__restrict__ dst, size_t rows, size_t rows_pad,
                                                   int n, int rs, const S *__restrict__ src, size_t ld,
                                                   const knn_dst_t<MODE> to)
{
    typedef typename std::conditional<sizeof(S) == 8, dbl2, flt4>::type svec_t;
    constexpr bool SCATTER = MODE == KNN_SCATTER;
    const size_t lim = MODE != KNN_PACK ? rows : rows_pad;
    size_t d0 = 0;
    if constexpr (MODE == KNN_APPEND) d0 = to.row0;
    constexpr int SV = 16 / (int)sizeof(S);
    int *norms = (int *)(dst + rows_pad * (size_t)rs);
    double *meta = (double *)(norms + 2 * rows_pad);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ng = rs / 8;
    knn_meta_acc_t<MODE != KNN_PACK> ma;
    double mnorm = 0.0;
    for (size_t r = (size_t)blockIdx.x * 4 + wave; r < lim; r += (size_t)gridDim.x * 4) {
        double s = 0.0;
        unsigned si = 0u;
        size_t sr = r, dr = d0 + r;   // the item's source row and block row
        bool live = r < rows, wr = true;
        if constexpr (SCATTER) knn_scatter_item(to, r, live, sr, dr, wr);
        const S *x = src + sr * ld;
        for (int g = lane; g < ng; g += 64) {
            unsigned lo = 0u, hi = 0u;
            S sv[8];
            if (VEC && live && 8 * g + 8 <= n) {
#pragma unroll
                for (int q = 0; q < 8 / SV; q++) {
                    const svec_t w = *(const svec_t *)(x + 8 * g + SV * q);
#pragma unroll
                    for (int e = 0; e < SV; e++) sv[SV * q + e] = w[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) sv[e] = (live && 8 * g + e < n) ? x[8 * g + e] : (S)0;
            }
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int j = 8 * g + e;
                const bool in = live && j < n;
                const T v = in ? (T)sv[e] : (T)0;
                ma.add((double)v, s);
                const int xi = in ? knn_spec8(v) : 0;
                si += (unsigned)(xi * xi);
                if (e < 4) lo |= ((unsigned)xi & 0xffu) << (8 * e);
                else hi |= ((unsigned)xi & 0xffu) << (8 * (e - 4));
            }
            typedef unsigned u2 __attribute__((ext_vector_type(2)));
            if (!SCATTER || wr) *(u2 *)(dst + dr * (size_t)rs + 8 * g) = (u2){lo, hi};
        }
        for (int off = 32; off > 0; off >>= 1) {
            s += __shfl_xor(s, off);
            si += (unsigned)__shfl_xor((int)si, off);
        }
        if (lane == 0 && (!SCATTER || wr)) {
            norms[i8_norm_pos((int)dr)] = i8_norm_word((int)dr, (int)si, rs);
            norms[rows_pad + i8_norm_pos((int)dr)] = i8_init_word((int)si, rs);
        }
        if (s == s) mnorm = s > mnorm ? s : mnorm;
        else ma.nonfin = 1.0;
    }
    knn_meta_flush(ma, mnorm, meta);
    if (MODE == KNN_PACK && blockIdx.x == 0 && threadIdx.x == 0) meta[KNN_META_S8] = 1.0;
}

// row-major KNN_U8 source: the byte image is x ^ 0x80 (x - 128 as int8), so a
// lane moves one 16-byte group of a row, read as one vector and written as
// one (2 bytes of traffic an element).  LPR lanes (a power of two >= rs / 16,
// at most 64) share a row and a wave carries 64 / LPR rows at once: SIFT's
// 128-byte rows 8 to a wave, MNIST's 800-byte rows one (four such row groups
// in flight).  Everything is
// integer arithmetic: sum (x - 128)^2 for the norm words, sum x^2 (< 2^26 at
// n <= 896) and max x for the meta -- the words the fp64 source gives for the
// same values, whatever the order of summation (exact integers below 2^53).
// VEC: the source and ld are multiples of 16 bytes, so every whole group
// inside n is read as a 16-byte vector; otherwise, in a row's tail group and
// past n (ld > n), byte by byte.
typedef unsigned knn_v4u __attribute__((ext_vector_type(4)));
// APPEND: row groups are cut at `rows`, which a group may straddle: the rows
// past it are neither stored nor given norm words.  SCATTER: the same for its
// items; each row group looks its source and block rows up once.
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void k_pack8_row_u8(signed char *__restrict__ dst, size_t rows, size_t rows_pad,
                                                      int n, int rs, const unsigned char *__restrict__ src,
                                                      size_t ld, int lpr, const knn_dst_t<MODE> to)
{
    constexpr bool APPEND = MODE != KNN_PACK, SCATTER = MODE == KNN_SCATTER;
    const size_t lim = APPEND ? rows : rows_pad, d0 = MODE == KNN_APPEND ? knn_dst_row0(to) : 0;
    int *norms = (int *)(dst + rows_pad * (size_t)rs);
    double *meta = (double *)(norms + 2 * rows_pad);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rpw = 64 / lpr;               // rows a wave
    const int sub = lane / lpr, g = lane % lpr;
    const bool has = 16 * g < rs;           // this lane's group lies inside the row
    unsigned mx = 0u, mnorm = 0u;
    // U row groups a wave in flight: their vector loads issue before the first
    // conversion (one load a lane a row left the wave waiting on each row in
    // turn).  rows_pad is a multiple of 128 and rpw divides 64, so a row group
    // lies below rows_pad as a whole or not at all (wave-uniform).
    constexpr int U = 4;
    for (size_t rb = ((size_t)blockIdx.x * 4 + wave) * U * rpw; rb < lim;
         rb += (size_t)gridDim.x * 4 * U * rpw) {
        knn_v4u v[U];
        bool full[U];
        // SCATTER: item r's source row, block row, and whether it has the one and is written to the other
        size_t srs[SCATTER ? U : 1], drs[SCATTER ? U : 1];
        bool lvs[SCATTER ? U : 1], wrs[SCATTER ? U : 1];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t r = rb + (size_t)u * rpw + sub;
            v[u] = (knn_v4u){0u, 0u, 0u, 0u};
            if constexpr (SCATTER) {
                lvs[u] = r < rows;
                knn_scatter_item(to, r, lvs[u], srs[u], drs[u], wrs[u]);
                full[u] = VEC && has && lvs[u] && 16 * g + 16 <= n;
                if (full[u]) v[u] = *(const knn_v4u *)(src + srs[u] * ld + 16 * g);
            } else {
                full[u] = VEC && has && r < rows && 16 * g + 16 <= n;
                if (full[u]) v[u] = *(const knn_v4u *)(src + r * ld + 16 * g);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (rb + (size_t)u * rpw >= lim) break;
            const size_t r = rb + (size_t)u * rpw + sub;
            const bool wr = SCATTER ? wrs[SCATTER ? u : 0] : !APPEND || r < rows;
            const bool lv = SCATTER ? lvs[SCATTER ? u : 0] : r < rows;
            const size_t sr = SCATTER ? srs[SCATTER ? u : 0] : r, dr = SCATTER ? drs[SCATTER ? u : 0] : d0 + r;
            // bytes, and 0xff where a byte is data
            unsigned w[4] = {v[u][0], v[u][1], v[u][2], v[u][3]};
            const unsigned fm = full[u] ? 0xffffffffu : 0u;
            unsigned live[4] = {fm, fm, fm, fm};
            if (!full[u] && has && lv) {
                const unsigned char *x = src + sr * ld + 16 * g;
#pragma unroll
                for (int e = 0; e < 16; e++)
                    if (16 * g + e < n) {
                        w[e >> 2] |= (unsigned)x[e] << (8 * (e & 3));
                        live[e >> 2] |= 0xffu << (8 * (e & 3));
                    }
            }
            unsigned sx = 0u, si = 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const unsigned b = (w[q] >> (8 * e)) & 0xffu;
                    const int xi = ((live[q] >> (8 * e)) & 1u) ? (int)b - 128 : 0;
                    sx += b * b;
                    si += (unsigned)(xi * xi);
                    mx = b > mx ? b : mx;
                }
                w[q] = (w[q] ^ 0x80808080u) & live[q];
            }
            if (has && wr) *(knn_v4u *)(dst + dr * (size_t)rs + 16 * g) = (knn_v4u){w[0], w[1], w[2], w[3]};
            for (int off = lpr >> 1; off > 0; off >>= 1) {
                sx += (unsigned)__shfl_xor((int)sx, off);
                si += (unsigned)__shfl_xor((int)si, off);
            }
            if (g == 0 && wr) {
                norms[i8_norm_pos((int)dr)] = i8_norm_word((int)dr, (int)si, rs);
                norms[rows_pad + i8_norm_pos((int)dr)] = i8_init_word((int)si, rs);
            }
            mnorm = sx > mnorm ? sx : mnorm;
        }
    }
    knn_meta_acc_t<APPEND> ma;
    ma.mabs = ma.mpos = (double)mx;
    knn_meta_flush(ma, (double)mnorm, meta);
    if (!APPEND && blockIdx.x == 0 && threadIdx.x == 0) meta[KNN_META_S8] = 1.0;
}

// Row-major source: one wave per row (lane-strided features, butterfly sum).
template <typename T, typename S, int MODE>
__global__ __launch_bounds__(256) void k_pack_row(T *__restrict__ blk, size_t rows, size_t rows_pad, int n,
                                                  int n_pad, const S *__restrict__ src, size_t ld,
                                                  const knn_dst_t<MODE> dst)
{
    constexpr bool SCATTER = MODE == KNN_SCATTER;
    T *norms = blk + rows_pad * (size_t)n_pad;
    double *meta = (double *)(norms + rows_pad);
    const size_t lim = MODE != KNN_PACK ? rows : rows_pad;
    size_t d0 = 0;
    if constexpr (MODE == KNN_APPEND) d0 = dst.row0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    knn_meta_acc_t<MODE != KNN_PACK> ma;
    double mnorm = 0.0;
    for (size_t i = (size_t)blockIdx.x * 4 + wave; i < lim; i += (size_t)gridDim.x * 4) {
        double s = 0.0;
        size_t sr = i, dr = d0 + i;   // the item's source row and block row
        bool live = i < rows, wr = true;
        if constexpr (SCATTER) knn_scatter_item(dst, i, live, sr, dr, wr);
        const S *x = src + sr * ld;
        T *o = blk + dr * (size_t)n_pad;
        for (int j = lane; j < n_pad; j += 64) {
            const T v = (live && j < n) ? (T)x[j] : (T)0;
            if (!SCATTER || wr) o[j] = v;
            ma.add((double)v, s);
        }
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0 && (!SCATTER || wr)) norms[dr] = (T)s;
        if (s == s) mnorm = s > mnorm ? s : mnorm;
        else ma.nonfin = 1.0;
    }
    knn_meta_flush(ma, mnorm, meta);
}

// ---------------------------------------------------------------------------
// Launchers of the pack kernels.  A pack, an append (rows row0 .. of a
// block packed before, knn_block_append_dt / _s8) and a scatter (listed rows of
// one, knn_block_scatter_dt / _s8) take the same path and
// differ in the kernels' MODE argument, in the rows a grid covers (gr:
// rows_pad for a pack, which also zeroes the padding rows; `rows` for the
// other two), in where the rows go (knn_pack_to_t), and in the meta: a pack
// zeroes it first, the others leave it (the meta is max(old, new rows); the
// byte kernels set KNN_META_S8 in a pack only).
// ---------------------------------------------------------------------------
// a bool as a template argument: f(std::true_type()) or f(std::false_type())
template <typename F>
static int with_bool(bool b, F f)
{
    return b ? f(std::true_type()) : f(std::false_type());
}
// where a launch's rows go: the mode, an append's row0, a scatter's lists
// (device arrays of `rows` entries; srow nullable) and its source's row count
struct knn_pack_to_t {
    int mode;
    size_t row0;
    const int32_t *pos, *srow;
    size_t src_rows;
};
// the mode as a template argument, and the kernels' last argument for it
template <typename F>
static int with_mode(int mode, F f)
{
    if (mode == KNN_PACK) return f(std::integral_constant<int, KNN_PACK>());
    if (mode == KNN_APPEND) return f(std::integral_constant<int, KNN_APPEND>());
    return f(std::integral_constant<int, KNN_SCATTER>());
}
template <int MODE>
static knn_dst_t<MODE> dst_arg(const knn_pack_to_t &to, size_t cap)
{
    if constexpr (MODE == KNN_SCATTER) return knn_dst_t<MODE>{to.pos, to.srow, (int)to.src_rows, (int)cap};
    else return knn_dst_t<MODE>{to.row0};
}

// grid of the kernels that give a wave a row at a time: 4 rows a workgroup
static unsigned grid_wave_rows(size_t gr) { return (unsigned)((gr + 3) / 4 < 8192 ? (gr + 3) / 4 : 8192); }

template <typename T, typename S>
static int launch_pack(T *blk, size_t cap, size_t rows, size_t n, const S *src, size_t ld, int layout,
                       hipStream_t s, const knn_pack_to_t &to)
{
    constexpr int dt = sizeof(T) == 8 ? KNN_F64 : KNN_F32;
    const size_t rp = knn_rows_pad(cap), np = knn_n_pad_dt(n, dt);
    const bool pack = to.mode == KNN_PACK;
    const size_t gr = pack ? rp : rows;
    double *meta = (double *)(blk + rp * np + rp);
    if (pack && hipMemsetAsync(meta, 0, KNN_META_DOUBLES * sizeof(double), s) != hipSuccess)
        return KNN_ERR_HIP;
    return with_mode(to.mode, [&](auto md) {
        constexpr int MD = decltype(md)::value;
        if (layout == KNN_COLMAJOR)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack_col<T, S, MD>), dim3((unsigned)((gr + 63) / 64)), dim3(256), 0,
                               s, blk, rows, rp, (int)n, (int)np, src, ld, dst_arg<MD>(to, cap));
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack_row<T, S, MD>), dim3(grid_wave_rows(gr)), dim3(256), 0, s, blk,
                               rows, rp, (int)n, (int)np, src, ld, dst_arg<MD>(to, cap));
        return hip_status();
    });
}

template <typename T, typename S>
static int launch_pack8(signed char *dst, size_t cap, size_t rows, size_t n, const S *src, size_t ld, int layout,
                        hipStream_t s, const knn_pack_to_t &to)
{
    const size_t rp = knn_rows_pad(cap), rs = knn_s8_rs(n);
    const bool pack = to.mode == KNN_PACK;
    const size_t gr = pack ? rp : rows;
    double *meta = (double *)(dst + knn_s8_meta_offset(cap, n));
    if (pack && hipMemsetAsync(meta, 0, KNN_META_DOUBLES * sizeof(double), s) != hipSuccess) return KNN_ERR_HIP;
    // row-major: rows that start on 16 bytes are read as vectors (ld % 16 for
    // a byte source).  (An append's source that starts at row0 * n of a larger
    // array is rarely 16-byte aligned.)  (A scatter reads any row of its
    // source: the same condition holds for each.)
    const bool vec = ((uintptr_t)src % 16 == 0) && (ld * sizeof(S)) % 16 == 0;
    return with_mode(to.mode, [&](auto md) {
        return with_bool(vec, [&](auto vc) -> int {
            constexpr int MD = decltype(md)::value;
            constexpr bool VEC = decltype(vc)::value;
            if (layout == KNN_COLMAJOR) {
                // (32-row workgroups, twice as many: 107.5 against 105.7 us for MNIST)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack8_col<T, S, 64, MD>), dim3((unsigned)((gr + 63) / 64)),
                                   dim3(256), 0, s, dst, rows, rp, (int)n, (int)rs, src, ld, dst_arg<MD>(to, cap));
            } else if constexpr (sizeof(S) == 1) {
                // KNN_U8: lpr lanes a row (a power of two >= rs / 16), 64 / lpr rows a wave
                int lpr = 1;
                while (lpr < 64 && 16 * (size_t)lpr < rs) lpr *= 2;
                if (16 * (size_t)lpr < rs) return KNN_ERR_INVALID;   // (rs <= 1024: n <= KNN_I8_MAX_N)
                // waves for one pass at 4 row groups a wave; 2048 workgroups (8 a CU) at most:
                // every workgroup ends in six atomics on the same meta words
                const size_t nw = (gr * lpr + 255) / 256;
                const unsigned nb = (unsigned)((nw + 3) / 4 < 2048 ? (nw + 3) / 4 : 2048);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack8_row_u8<VEC, MD>), dim3(nb), dim3(256), 0, s, dst, rows, rp,
                                   (int)n, (int)rs, src, ld, lpr, dst_arg<MD>(to, cap));
            } else {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack8_row<T, S, VEC, MD>), dim3(grid_wave_rows(gr)), dim3(256), 0,
                                   s, dst, rows, rp, (int)n, (int)rs, src, ld, dst_arg<MD>(to, cap));
            }
            return hip_status();
        });
    });
}

// f(block element, typed source pointer) for the served (dtype, src_dtype)
// pairs: fp64 and fp32 blocks from fp64, fp32 and KNN_U8 sources.  (A byte
// block's bytes do not depend on the block's element type: every value is
// exact in both.)
template <typename F>
static int pack_dispatch(int dtype, const void *src, int src_dtype, F f)
{
    auto with_src = [&](auto te) -> int {
        if (src_dtype == KNN_F64) return f(te, (const double *)src);
        if (src_dtype == KNN_F32) return f(te, (const float *)src);
        if (src_dtype == KNN_U8) return f(te, (const unsigned char *)src);
        return KNN_ERR_INVALID;
    };
    if (dtype == KNN_F64) return with_src(double());
    if (dtype == KNN_F32) return with_src(float());
    return KNN_ERR_INVALID;
}

// the element block (s8 = false) or the byte block of `dtype` at blk
static int pack_any(bool s8, void *blk, int dtype, size_t cap, size_t rows, size_t n, const void *src,
                    int src_dtype, size_t ld, int layout, void *stream, const knn_pack_to_t &to)
{
    hipStream_t s = (hipStream_t)stream;
    return pack_dispatch(dtype, src, src_dtype, [&](auto te, auto *sp) {
        typedef decltype(te) T;
        return s8 ? launch_pack8<T>((signed char *)blk, cap, rows, n, sp, ld, layout, s, to)
                  : launch_pack((T *)blk, cap, rows, n, sp, ld, layout, s, to);
    });
}
extern "C" int knn_launch_pack(void *blk, int dtype, size_t cap, size_t rows, size_t n,
                               const void *src, int src_dtype, size_t ld, int layout, void *stream)
{
    return pack_any(false, blk, dtype, cap, rows, n, src, src_dtype, ld, layout, stream, {KNN_PACK, 0, NULL, NULL, 0});
}
extern "C" int knn_launch_append(void *blk, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                                 const void *src, int src_dtype, size_t ld, int layout, void *stream)
{
    return pack_any(false, blk, dtype, cap, rows, n, src, src_dtype, ld, layout, stream,
                    {KNN_APPEND, row0, NULL, NULL, 0});
}
extern "C" int knn_launch_pack_s8(void *dst, int dtype, size_t cap, size_t rows, size_t n, const void *src,
                                  int src_dtype, size_t ld, int layout, void *stream)
{
    return pack_any(true, dst, dtype, cap, rows, n, src, src_dtype, ld, layout, stream, {KNN_PACK, 0, NULL, NULL, 0});
}
extern "C" int knn_launch_append_s8(void *dst, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                                    const void *src, int src_dtype, size_t ld, int layout, void *stream)
{
    return pack_any(true, dst, dtype, cap, rows, n, src, src_dtype, ld, layout, stream,
                    {KNN_APPEND, row0, NULL, NULL, 0});
}
// (cap and src_rows <= INT32_MAX: the entry points check)
extern "C" int knn_launch_scatter(void *blk, int dtype, size_t cap, const int32_t *pos, const int32_t *srow,
                                  size_t rows, size_t n, const void *src, size_t src_rows, int src_dtype, size_t ld,
                                  int layout, void *stream)
{
    return pack_any(false, blk, dtype, cap, rows, n, src, src_dtype, ld, layout, stream,
                    {KNN_SCATTER, 0, pos, srow, src_rows});
}
extern "C" int knn_launch_scatter_s8(void *dst, int dtype, size_t cap, const int32_t *pos, const int32_t *srow,
                                     size_t rows, size_t n, const void *src, size_t src_rows, int src_dtype,
                                     size_t ld, int layout, void *stream)
{
    return pack_any(true, dst, dtype, cap, rows, n, src, src_dtype, ld, layout, stream,
                    {KNN_SCATTER, 0, pos, srow, src_rows});
}

// Ring wire form of a packed block (knn_wire_pack / knn_wire_unpack): the
// element array as int16 (exact for integer data with max|x| <= 32767),
// 8 elements a thread; norms and meta travel verbatim (hipMemcpyAsync).
typedef short knn_s8v __attribute__((ext_vector_type(8)));
template <typename T>
__global__ __launch_bounds__(256) void k_wire_pack(knn_s8v *__restrict__ w, const T *__restrict__ b,
                                                   size_t n8)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        knn_s8v v;
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = (short)b[8 * i + e];
        w[i] = v;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_wire_unpack(T *__restrict__ b, const knn_s8v *__restrict__ w,
                                                     size_t n8)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const knn_s8v v = w[i];
#pragma unroll
        for (int e = 0; e < 8; e++) b[8 * i + e] = (T)v[e];
    }
}

extern "C" int knn_launch_wire(int unpack, void *dst, const void *src, int dtype, size_t cnt,
                               void *stream)
{
    if (cnt % 8) return KNN_ERR_INVALID;
    const size_t n8 = cnt / 8;
    const unsigned grid = (unsigned)(n8 / 256 + 1 < 4096 ? n8 / 256 + 1 : 4096);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KNN_F64 && !unpack)
        hipLaunchKernelGGL(k_wire_pack<double>, dim3(grid), dim3(256), 0, s, (knn_s8v *)dst,
                           (const double *)src, n8);
    else if (dtype == KNN_F64)
        hipLaunchKernelGGL(k_wire_unpack<double>, dim3(grid), dim3(256), 0, s, (double *)dst,
                           (const knn_s8v *)src, n8);
    else if (dtype == KNN_F32 && !unpack)
        hipLaunchKernelGGL(k_wire_pack<float>, dim3(grid), dim3(256), 0, s, (knn_s8v *)dst,
                           (const float *)src, n8);
    else if (dtype == KNN_F32)
        hipLaunchKernelGGL(k_wire_unpack<float>, dim3(grid), dim3(256), 0, s, (float *)dst,
                           (const knn_s8v *)src, n8);
    else
        return KNN_ERR_INVALID;
    return hip_status();
}

// fp16 shadow rows of a packed block for the H16 == 2 contraction: rows
// of round_up(n, 64) halves (zero padded), converted with v_cvt_pkrtz
// (exact: shadows are only made for integer data with max|x| <= 2048).
template <typename T>
__global__ __launch_bounds__(256) void k_shadow(knn_h8 *__restrict__ dst, const T *__restrict__ src,
                                                size_t rows, int n, int nps, int npd)
{
    const size_t per = (size_t)npd / 8, tot = rows * per;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (size_t)gridDim.x * 256) {
        const size_t r = i / per;
        const int c = (int)(i - r * per) * 8;
        const T *row = src + r * (size_t)nps;
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int j = c + 2 * e;
            const float x0 = j < n ? (float)row[j] : 0.f;
            const float x1 = j + 1 < n ? (float)row[j + 1] : 0.f;
            w[e] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0, x1));
        }
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        dst[i] = __builtin_bit_cast(knn_h8, (u4){w[0], w[1], w[2], w[3]});
    }
}

extern "C" int knn_launch_shadow(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n,
                                 void *stream)
{
    const int npd = (int)knn_round_up(n, 64), nps = (int)knn_n_pad_dt(n, dtype);
    const size_t tot = rows_pad * (size_t)npd / 8;
    const unsigned grid = (unsigned)(tot / 256 + 1 < 8192 ? tot / 256 + 1 : 8192);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KNN_F64)
        hipLaunchKernelGGL(k_shadow<double>, dim3(grid), dim3(256), 0, s, (knn_h8 *)dst,
                           (const double *)blk, rows_pad, (int)n, nps, npd);
    else if (dtype == KNN_F32)
        hipLaunchKernelGGL(k_shadow<float>, dim3(grid), dim3(256), 0, s, (knn_h8 *)dst,
                           (const float *)blk, rows_pad, (int)n, nps, npd);
    else
        return KNN_ERR_INVALID;
    return hip_status();
}

// Split fp16 shadow rows (the split filter) of fp32 / fp64 blocks: per row
// and 32-feature group, the 32 halves hi = RN16(S x) then the 32 halves lo =
// RN16(S x - hi), each rounded once from the block's precision (S x - hi is
// exact there: Sterbenz); zero past n.  One thread per 16 bytes
// of source row (V = 2 fp64 / 4 fp32 features): a wave reads 1 KiB of a row
// contiguously and its 16-lane groups write whole 64-byte hi and lo runs.
// (Round 4's form, one thread per 8 features with 8-byte loads 64 bytes
// apart, moved a 7552 x 784 fp64 block in 35 us, 2 TB/s.)  Up to
// KNN_SPLIT_MAXBLK blocks per launch (a ring rank's received blocks).
struct knn_split_conv_t {
    char *dst[KNN_SPLIT_MAXBLK];
    const void *src[KNN_SPLIT_MAXBLK];
    long long i0[KNN_SPLIT_MAXBLK + 1];   // first flat work item of block b
    int nblk;
};

template <typename T>
__global__ __launch_bounds__(256) void k_shadow_split(const knn_split_conv_t cv, int n, int nps, int npd, float S)
{
    constexpr int V = 16 / (int)sizeof(T);
    typedef typename std::conditional<sizeof(T) == 8, dbl2, flt4>::type vec_t;
    typedef _Float16 hv_t __attribute__((ext_vector_type(V)));
    const int per = npd / V;   // work items a row
    const long long tot = cv.i0[cv.nblk];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long long)gridDim.x * 256) {
        int b = 0;
#pragma unroll
        for (int x = 1; x < KNN_SPLIT_MAXBLK; x++) b = (x < cv.nblk && i >= cv.i0[x]) ? x : b;
        const long long li = i - cv.i0[b];
        const long long r = li / per;
        const int j0 = (int)(li - r * per) * V;
        vec_t v{};
        if (j0 < n) v = *(const vec_t *)((const T *)cv.src[b] + r * (long long)nps + j0);
        hv_t hi, lo;
#pragma unroll
        for (int e = 0; e < V; e++) {
            // one rounding each, from the block's precision (x - hi is exact
            // in it: Sterbenz).  (Written as conversions through fp32, the
            // compiler folds them into these single roundings anyway.)
            const T x = (j0 + e < n) ? v[e] * (T)S : (T)0;
            const _Float16 h = (_Float16)x;
            hi[e] = h;
            lo[e] = (_Float16)(x - (T)h);
        }
        char *o = cv.dst[b] + r * (long long)npd * 4 + (long long)(j0 >> 5) * 128 + 2 * (j0 & 31);
        *(hv_t *)o = hi;
        *(hv_t *)(o + 64) = lo;
    }
}

// nblk blocks: dst[b] <- split rows of src[b] (rows_pad[b] rows each)
extern "C" int knn_launch_shadow_split_n(int nblk, void *const *dst, const void *const *src, const size_t *rows_pad,
                                         int dtype, size_t n, float S, void *stream)
{
    if (nblk < 1 || nblk > KNN_SPLIT_MAXBLK || n == 0) return KNN_ERR_INVALID;
    const int npd = (int)knn_round_up(n, 32), nps = (int)knn_n_pad_dt(n, dtype);
    const int V = dtype == KNN_F64 ? 2 : 4;
    knn_split_conv_t cv{};
    cv.nblk = nblk;
    cv.i0[0] = 0;
    for (int b = 0; b < nblk; b++) {
        if (!dst[b] || !src[b]) return KNN_ERR_INVALID;
        cv.dst[b] = (char *)dst[b];
        cv.src[b] = src[b];
        cv.i0[b + 1] = cv.i0[b] + (long long)rows_pad[b] * (npd / V);
    }
    for (int b = nblk + 1; b <= KNN_SPLIT_MAXBLK; b++) cv.i0[b] = cv.i0[nblk];
    const long long tot = cv.i0[nblk];
    const unsigned grid = (unsigned)(tot / 256 + 1 < 16384 ? tot / 256 + 1 : 16384);
    if (dtype == KNN_F32)
        hipLaunchKernelGGL(k_shadow_split<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, cv, (int)n, nps,
                           npd, S);
    else if (dtype == KNN_F64)
        hipLaunchKernelGGL(k_shadow_split<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, cv, (int)n, nps,
                           npd, S);
    else
        return KNN_ERR_INVALID;
    return hip_status();
}

extern "C" int knn_launch_shadow_split(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n,
                                       float S, void *stream)
{
    return knn_launch_shadow_split_n(1, &dst, &blk, &rows_pad, dtype, n, S, stream);
}

// ---------------------------------------------------------------------------
// Block gathers (knn_block_gather_dt / knn_block_gather_s8): block row
// row0 + i of dst becomes row list[i] of src, i < rows -- the stable
// compaction of knn_index_remove, and any other selection of rows.  Pure
// copies: a row is rb bytes, whole 128-byte chunks in an element block and a
// multiple of 32 bytes in a byte block, so a lane moves 16 bytes per load and
// store.  lpr lanes (a power of two >= rb / 16, at most 64) share a row and a
// wave carries 64 / lpr rows at once, as k_pack8_row_u8 does; a longer row is
// walked by its 64 lanes, four 16-byte pieces a lane in flight.  Only the
// listed rows and their norms are written: no padding, no meta.  A list entry
// outside [0, src_cap) writes nothing.  knn_block_gather_pos_dt / _s8 are the
// same copies out of several source blocks at once (the kernel's MULTI form):
// the query tiles of knn_index_neighbours, filled from the resident corpus.
//
//   element block: the norm (one T) is copied with the row, bit for bit (es =
//       sizeof(T): the kernel never looks at the values).
//   byte block: both norm words depend on the row's position (i8_norm_word's
//       slot, i8_norm_pos); they are made again for row0 + i from the norm the
//       source words hold (i8_norm_of), as k_gather8 does.
// ---------------------------------------------------------------------------
// MULTI (knn_block_gather_pos_dt / _s8): the source is a corpus held as blocks
// of one capacity src_cap, their pointers in a device table (srcp), and
// list[i] is a global position: row list[i] % src_cap of block list[i] /
// src_cap.  lim: the first position that is no row (src_cap without MULTI);
// an entry outside [0, lim) writes nothing.  Everything else is the one body.
template <bool S8, bool MULTI>
__global__ __launch_bounds__(256) void k_gather_rows(char *__restrict__ dst, const void *__restrict__ srcp,
                                                     const int *__restrict__ list, size_t rows, size_t row0,
                                                     int src_cap, unsigned lim, int rb, int es, size_t dst_rp,
                                                     size_t src_rp, int lpr)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rpw = 64 / lpr;               // rows a wave
    const int sub = lane / lpr, g = lane % lpr;
    const int c16 = rb / 16;                // 16-byte pieces a row
    char *dn = dst + dst_rp * (size_t)rb;
    for (size_t rbase = ((size_t)blockIdx.x * 4 + wave) * rpw; rbase < rows; rbase += (size_t)gridDim.x * 4 * rpw) {
        const size_t r = rbase + sub;
        int q = r < rows ? list[r] : -1;
        if ((unsigned)q >= lim) continue;
        const char *src;
        if constexpr (MULTI) {
            src = ((const char *const *)srcp)[q / src_cap];
            q %= src_cap;
        } else
            src = (const char *)srcp;
        const char *sn = src + src_rp * (size_t)rb;
        const knn_v4u *s = (const knn_v4u *)(src + (size_t)q * rb);
        knn_v4u *d = (knn_v4u *)(dst + (row0 + r) * (size_t)rb);
        for (int c = g; c < c16; c += 4 * lpr) {
            knn_v4u v[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c + u * lpr < c16) v[u] = __builtin_nontemporal_load(s + c + u * lpr);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c + u * lpr < c16) d[c + u * lpr] = v[u];
        }
        if (g != 0) continue;
        const size_t t = row0 + r;
        if constexpr (S8) {
            const int *snw = (const int *)sn;
            int *dnw = (int *)dn;
            const int nrm = i8_norm_of(snw[i8_norm_pos(q)], snw[src_rp + i8_norm_pos(q)]);
            dnw[i8_norm_pos((int)t)] = i8_norm_word((int)t, nrm, rb);
            dnw[dst_rp + i8_norm_pos((int)t)] = i8_init_word(nrm, rb);
        } else if (es == 8) {
            ((unsigned long long *)dn)[t] = ((const unsigned long long *)sn)[q];
        } else {
            ((unsigned *)dn)[t] = ((const unsigned *)sn)[q];
        }
    }
}

// rb: the row bytes of both blocks (a multiple of 32); es: the element block's
// element size, 0 for a byte block.  nblk == 0: src is the one source block
// and list holds its local rows; nblk > 0: src is a device table of nblk block
// pointers and list holds global positions (positions are int32: the limit
// stops there).
static int launch_gather(bool s8, void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap,
                         size_t nblk, const int32_t *list, size_t rows, size_t rb, int es, void *stream)
{
    if (rb > 0x7fffffffULL) return KNN_ERR_INVALID;
    int lpr = 1;
    while (lpr < 64 && 16 * (size_t)lpr < rb) lpr *= 2;
    // waves for one pass: 64 / lpr rows a wave, 4 waves a workgroup
    const size_t nw = (rows * lpr + 63) / 64;
    const unsigned nb = (unsigned)((nw + 3) / 4 < 16384 ? (nw + 3) / 4 : 16384);
    const size_t drp = knn_rows_pad(dst_cap), srp = knn_rows_pad(src_cap);
    const size_t tot = nblk ? nblk * src_cap : src_cap;
    const unsigned lim = (unsigned)(tot < 0x80000000ULL ? tot : 0x80000000ULL);
    return with_bool(s8, [&](auto b8) {
        return with_bool(nblk != 0, [&](auto mu) -> int {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather_rows<decltype(b8)::value, decltype(mu)::value>), dim3(nb),
                               dim3(256), 0, (hipStream_t)stream, (char *)dst, src, list, rows, row0, (int)src_cap, lim,
                               (int)rb, es, drp, srp, lpr);
            return hip_status();
        });
    });
}

extern "C" int knn_launch_gather(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap,
                                 const int32_t *list, size_t rows, size_t n, int dtype, void *stream)
{
    if (dtype != KNN_F64 && dtype != KNN_F32) return KNN_ERR_INVALID;
    const int es = (int)knn_esize(dtype);
    return launch_gather(false, dst, dst_cap, row0, src, src_cap, 0, list, rows, knn_n_pad_dt(n, dtype) * es, es,
                         stream);
}

extern "C" int knn_launch_gather_rows8(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap,
                                       const int32_t *list, size_t rows, size_t n, void *stream)
{
    return launch_gather(true, dst, dst_cap, row0, src, src_cap, 0, list, rows, knn_s8_rs(n), 0, stream);
}

// the same from nblk blocks of capacity src_cap (tab: their pointers, a device
// array), by global position (knn_block_gather_pos_dt / _s8)
extern "C" int knn_launch_gather_pos(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap,
                                     size_t nblk, const int32_t *pos, size_t rows, size_t n, int dtype, void *stream)
{
    if ((dtype != KNN_F64 && dtype != KNN_F32) || nblk == 0) return KNN_ERR_INVALID;
    const int es = (int)knn_esize(dtype);
    return launch_gather(false, dst, dst_cap, row0, tab, src_cap, nblk, pos, rows, knn_n_pad_dt(n, dtype) * es, es,
                         stream);
}

extern "C" int knn_launch_gather_pos8(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap,
                                      size_t nblk, const int32_t *pos, size_t rows, size_t n, void *stream)
{
    if (nblk == 0) return KNN_ERR_INVALID;
    return launch_gather(true, dst, dst_cap, row0, tab, src_cap, nblk, pos, rows, knn_s8_rs(n), 0, stream);
}
