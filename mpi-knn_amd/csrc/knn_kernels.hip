// knn_kernels.hip -- CDNA4 (gfx950) kernels of the all-kNN engine.
//
// Hot path of yiapou13/mpi-knn: the distance loop + k-smallest insertion of
// knn-serial.c:72-93 (and its per-block copies mpi-knn-parallel_blocking.c:
// 155-181, 217-242).  Re-designed for MI355X:
//
//   (packing: knn_pack.hip writes the blocks these kernels read)
//   k_dist_topk  fused fp64-MFMA contraction G = C.Q^T (v_mfma_f64_16x16x4)
//                with d^2 = |q|^2 + |c|^2 - 2G and a per-lane register top-k
//                (insertion network) behind a shared threshold.  One
//                workgroup = 128 queries x a corpus split; tiles of 128 rows
//                stream through a 4-stage LDS ring filled by global_load_lds.
//   k_merge      per query: tournament merge of the split/lane lists with
//                the running state (ring steps), exact re-rank of new
//                entries in reference order (GEMM mode).
//   k_finalize   order by (sqrt(S), idx), drop S == 0, certify that no
//                unseen candidate can enter the top-k, emit records.
//   k_rescan_*   exact reference-order scan for the (rare) queries the
//                certificate could not clear.
//
// Layout and roofline notes: DESIGN.md sec.4.
#include "knn_device.h"

// ---------------------------------------------------------------------------
// Element-type traits.  A staged chunk is 128 bytes of every row: 16 fp64
// or 32 fp32 features.  One 16-byte LDS fragment holds KSF k-steps of the
// 16x16x4 MFMA (2 fp64 / 4 fp32).  Result register r of lane group g holds
// tile row ROW(g, r) (probed: tools/probe/mfma_probe, mfma_f32_probe).
// ---------------------------------------------------------------------------
template <typename T> struct KT;
template <> struct KT<double> {
    typedef dbl4 acc_t;
    typedef dbl2 frag_t;
    static constexpr int KSF = 2;
    static constexpr double U = 1.1102230246251565e-16;   // 2^-53
    __device__ static __forceinline__ acc_t mfma(double a, double b, acc_t c)
    {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    __device__ static constexpr int row(int g, int r) { return g + 4 * r; }
};
template <> struct KT<float> {
    typedef flt4 acc_t;
    typedef flt4 frag_t;
    static constexpr int KSF = 4;
    static constexpr double U = 5.9604644775390625e-08;   // 2^-24
    __device__ static __forceinline__ acc_t mfma(float a, float b, acc_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    __device__ static constexpr int row(int g, int r) { return 4 * g + r; }
};
template <typename T> static constexpr int knn_bk() { return 128 / (int)sizeof(T); }

// fp16 contraction of fp32 blocks (H16): INT-mode data with |x| <= 2048 is
// exact in fp16, every product exact in fp32 and every partial sum an
// integer <= n max|x|^2 <= 2^23, so v_mfma_f32_16x16x32_f16 yields the same
// dot products as the fp32 MFMA chain, bit for bit, in any summation order.
// Lane (row, g) converts its two 16-byte fp32 slots of a chunk (features
// 4g..4g+3 of pieces 0 and 1) into one 8-half operand; the query side is
// converted identically, so each chunk's 32 features are summed once.
// (knn_h8: knn_device.h)
typedef _Float16 knn_h4 __attribute__((ext_vector_type(4)));
// fp64 blocks (H16 with ES 8): integer data with max|x| <= 256.  A chunk is
// 16 features; lane (row, g) converts its two 16-byte slots (features
// 2g, 2g+1 of pieces 0 and 1) into one 4-half operand of
// v_mfma_f32_16x16x16_f16.  Its fp32 sums are exact over 16 chunks (256
// features: |partial| <= 256 * 2^16 = 2^24), then flushed into the fp64
// accumulators, so the tile's dot products are the fp64 path's, bit for bit.
// Hardware conversions only: a plain (_Float16)(double) cast is folded
// into one f64->f16 rounding, which hipcc emulates in ~30 integer
// instructions (measured 2.5x slower than the fp64 kernel).  Here
// v_cvt_f32_f64 then v_cvt_pkrtz_f16_f32 -- exact for these integers.
typedef __fp16 knn_hp2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ knn_h4 knn_to_h4(dbl2 a, dbl2 b)
{
    const knn_hp2 lo = __builtin_amdgcn_cvt_pkrtz((float)a.x, (float)a.y);
    const knn_hp2 hi = __builtin_amdgcn_cvt_pkrtz((float)b.x, (float)b.y);
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    u2 w;
    w.x = __builtin_bit_cast(unsigned int, lo);
    w.y = __builtin_bit_cast(unsigned int, hi);
    return __builtin_bit_cast(knn_h4, w);
}
__device__ __forceinline__ knn_h8 knn_to_h8(flt4 a, flt4 b)
{
    knn_h8 r;
    r[0] = (_Float16)a.x; r[1] = (_Float16)a.y; r[2] = (_Float16)a.z; r[3] = (_Float16)a.w;
    r[4] = (_Float16)b.x; r[5] = (_Float16)b.y; r[6] = (_Float16)b.z; r[7] = (_Float16)b.w;
    return r;
}

// (knn_mode: the search mode from the reduced meta, knn_device.h)

// Reference-order exact squared distance: S = S + (a-b)^2 over j = 0..n-1,
// two roundings per feature, no FMA (knn-serial.c:76-85; pow(x,2) -> x*x),
// in fp64 on the block's values (fp32 blocks: the fp32-rounded inputs).
// Rows are zero padded to n_pad (a multiple of 128 bytes) and S + (0-0)^2 =
// S, so the loop runs over whole 128-byte pieces, S bit-identical.  The sum
// is one dependent chain, and each lane's candidate row is its own gather:
// 8 pieces of 16 bytes of both rows are loaded before any is used (16 loads
// in flight a lane), so the chain waits on one memory latency every 128
// bytes instead of every 16 (k_merge's re-rank was latency-bound on those
// loads).
template <typename T>
__device__ __forceinline__ double knn_exact_sq_v(const T *__restrict__ a, const T *__restrict__ b,
                                                 int n_pad)
{
#pragma clang fp contract(off)
    typedef typename std::conditional<sizeof(T) == 8, dbl2, flt4>::type vec_t;
    constexpr int V = 16 / (int)sizeof(T), U = 8;
    const int nr = n_pad / V;   // a multiple of U (n_pad: 128-byte rows)
    double S = 0.0;
    for (int p = 0; p < nr; p += U) {
        vec_t va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            va[u] = ((const vec_t *)a)[p + u];
            vb[u] = ((const vec_t *)b)[p + u];
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int e = 0; e < V; e++) {
                const double t = (double)va[u][e] - (double)vb[u][e];
                const double t2 = t * t;
                S = S + t2;
            }
    }
    return S;
}

// Certificate margin: |GEMM-form d^2 - exact S| plus the reference's own
// rounding, for any candidate c of the search (|c|^2 <= maxnorm):
//   fp32 filter: fma-chain dot gamma_n (|q|^2+|c|^2), norm roundings and the
//   two final roundings 4u (|q|^2+|c|^2), times (1 + 2(n+4)u) for the
//   second-order terms; the reference's fp64 S: 4(n+2) 2^-53 (|q|^2+|c|^2).
//   fp64 filter: both at u = 2^-53, 8(n+4)u (|q|^2+|c|^2).
//   split fp16 filter (fp32 blocks, knn_shadow_split): each value scaled by
//   S = 2^e (maxabs S in [2^13, 2^14)) and split x S = hi + lo in fp16;
//   hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_f16.  Per element
//   |xS - hi - lo| <= 2^-22 |xS| + 2^-25 and the dropped lo.lo <=
//   2^-22 |q_j c_j| (+ subnormal terms): 3 2^-22 sum|q_j c_j|, 12u qc for d^2.
//   fp16 products are exact in fp32; each 32-feature chunk's 96 products
//   are summed apart in fp32 (any order: <= 95u sum|chunk terms|) and the
//   n/32 chunk sums added to the fp32 accumulator (<= (n/32) u sum|q_j
//   c_j|), so d^2 is off by (97 + n/32) 1.01 u qc; norms (fp64 blocks: their
//   fp64 norms rounded to fp32), qn + cn and the final fma 4u qc.  With a
//   20% margin (the MFMA's internal order is not specified; its precision
//   is at least fp32): ((136 + n/25) u + 4 (n+4) 2^-53) qc, fp32 and fp64
//   blocks alike.  Subnormal fp16 halves may be flushed by the MFMA:
//   then up to 2^-14 / S <= 2^-27 maxabs is lost per element, the absolute
//   part 2^-26 maxabs sqrt(n) (|q| + |c|).  The fp32 filter's is ~ (n + 4)
//   u qc.
template <typename TE>
__device__ __forceinline__ double knn_cert_E(int n, double qn, double maxnorm, int split = 0,
                                             double maxabs = 0.0)
{
    const double u = KT<TE>::U;
    const double nn = (double)n + 4.0, qc = qn + maxnorm;
    if (split) {
        const double ul = 5.9604644775390625e-08;   // 2^-24
        // the n/32 chunk sums are added in fp32 (k_dist_split, fp32 and fp64
        // blocks alike)
        const double acc = (double)n / 25.0;
        return ((136.0 + acc) * ul + 4.0 * nn * 1.1102230246251565e-16) * qc * (1.0 + 1e-6) +
               1.4901161193847656e-08 * maxabs * sqrt((double)n) * (sqrt(qn) + sqrt(maxnorm));
    }
    if constexpr (sizeof(TE) == 8) return 8.0 * nn * u * qc;
    else return nn * qc * (u * (1.0 + 2.0 * nn * u) + 4.0 * 1.1102230246251565e-16);
}

// ---------------------------------------------------------------------------
// k_dist_topk
//
// Workgroup: 512 threads = 8 waves; 128 queries (wave w: queries 16w..16w+15)
// x corpus tiles of 128 rows (8 m-tiles of 16).  Per wave per 16-feature
// chunk: 8 m-tiles x 4 k-steps = 32 v_mfma_f64_16x16x4_f64.
//
// f64 MFMA operand map (probed, tools/probe): lane l supplies A[l&15][l>>4]
// and B[l>>4][l&15]; D reg r of lane l is D[(l>>4)+4r][l&15].  A = corpus
// rows, B = queries, so lane l ends with 32 d^2 of ONE query (l&15) against
// corpus rows 16mt + (l>>4) + 4r.  The 4 lanes sharing a query (g = l>>4)
// keep separate lists over disjoint row sets; they share a threshold.
//
// k-permutation: in a 16-feature chunk, k-step s = 2p+e of lane group g uses
// feature 8p + 2g + e, so each lane's two k-steps of piece p are one 16-byte
// slot (segment 4p+g of the row's 128 bytes): one ds_read_b128.
//
// Staging: a 4-deep ring of 32 KiB LDS stages filled by LDS-DMA
// (buffer_load_dwordx4 ... lds).  One load instruction moves 8 rows x 128
// contiguous bytes (full lines: lane 8r+s fetches 16-byte segment s^(r&7) of
// row r), so a 16-row block is two loads and its LDS image is
// [row][segment ^ (row&7)] -- the XOR keeps the fragment reads conflict-free.
// Each wave stages its own m-tile (loads 0,1) and its own 16 queries
// (loads 2,3): 4 instructions per chunk, scalar addressing.
//
// The schedule is branch-free: chunk x's load 0 issues in segment S3 of
// chunk x-4 (after the barrier that freed its stage) and loads 1..3 in
// S0..S2 of chunk x-3, one per segment.  Chunks past the end re-load the
// last valid chunk (clamped address) into their stage, so every chunk issues
// the same loads and "chunk c+1 landed" is always one static
// `s_waitcnt vmcnt(8)` (guide sec.5 'Pipelining across barriers'; LDS-DMA
// stays in flight across barriers).  A straight-line body keeps the
// accumulators in place: the previous loop (one flat loop with a conditional
// epilogue and a last-chunk branch) made the register allocator shuttle them
// with v_mov + s_nop after every S1/S3 MFMA.
//
// Corpus norms: one 1 KiB slice per tile, loaded two tiles ahead at the
// start of a tile into a ring [tile&7][g][32] (row 4k+g at [g][k]; waves
// 4..7 repeat the bytes of waves 0..3); the >= 8 loads that follow it before
// that tile's epilogue make the vmcnt(8) waits cover it.
//
// Segments per chunk, 8 MFMAs each (an m-tile's two k-steps back to back:
// measured 1.2% faster than splitting the dependent pair) with the LDS
// reads of the next segment's fragments between them:
//   S0 (p0, mt0-3) S1 (p0, mt4-7) S2 (p1, mt0-3) | lgkmcnt(0), vmcnt(8),
//   barrier | S3 (p1, mt4-7) reading chunk c+1's first fragments.
//
// LDS (one array, guide 'second __shared__ object' trap):
//   stage s at s*32K: C [mt][row 16][128 B] (16 KiB), Q [w][row 16][128 B]
//   4*32K:            corpus norms ring [tile&7][g][32]
// ---------------------------------------------------------------------------
#define KNN_NST 4
// STG = 1: waves 0..3 stage the chunk pieces of their SIMD partners w + 4 too
// (fp16 shadow rows of fp32 blocks: sift 607 vs 691 ms); STG = 0: every wave
// stages its own.  Round-1 ablations of this kernel (no staging, no barrier,
// no insertion, setprio, MFMA orders: DESIGN.md sec.4) were measured with the
// tuning harness at commit 1e35c3d; the product source carries no hooks.
template <typename T, int KL, int KS, int STG = 0, int H16 = 0>
__global__ __launch_bounds__(512, 2) void k_dist_topk(
    const T *__restrict__ qblk, const T *__restrict__ qnorm, size_t q_base, int nq,
    const T *__restrict__ cblk, const T *__restrict__ cnorm, size_t c_base, int nc,
    int n, int n_pad, int ntiles, int nsplit, int nqb, const double *__restrict__ meta,
    double *__restrict__ part_d, int *__restrict__ part_i, double *__restrict__ part_T,
    int nq_pad, unsigned long long *__restrict__ qthr, int uj, int xord)
{
    constexpr int NST = KNN_NST;
    // H16 2: qblk / cblk are fp16 shadow rows (k_shadow), n_pad their row
    // length; the norms stay in the element blocks.  (Split fp16 rows have a
    // kernel of their own, k_dist_split in knn_split.hip.)
    constexpr int RS = H16 == 2 ? 2 : (int)sizeof(T);   // bytes per staged element
    constexpr int BK = 128 / RS;                      // features per 128-B chunk
    // fp64 H16 (knn_to_h4): the fp32 MFMA output layout, row 4g + r of a
    // 16-row m-tile in lane group g, register r, instead of fp64's g + 4r
    constexpr bool H16D = H16 != 0 && sizeof(T) == 8;
    constexpr bool F32L = H16 != 0 && sizeof(T) == 8;   // fp64 accumulators, fp32 MFMA layout
    auto rowmap = [](int gg, int r) { return F32L ? 4 * gg + r : KT<T>::row(gg, r); };
    constexpr int ES = (int)sizeof(T);
    typedef typename KT<T>::acc_t acc_t;
    typedef typename KT<T>::frag_t frag_t;
    constexpr int KSF = KT<T>::KSF;
    __shared__ __attribute__((aligned(16))) char smem[NST * 32768 + 8192];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, j16 = lane & 15;
    // xord 0, split-major: the first resident wave of workgroups shares one
    // corpus split, so its tiles are read from L2 by every XCD's workgroups.
    // xord 1, XCD-grouped: workgroups go to XCDs round-robin (blockIdx % 8),
    // so the nsplit workgroups of query block qb get ids 8(j nsplit + s) +
    // (qb % 8): one XCD, dispatched back to back -- they stream the same
    // query chunks in step (L2 hits), and co-resident blocks of one split
    // share corpus tiles.  The grid is padded to whole groups of 8 blocks.
    // (xord bit 1, KNN_KARG_KEEP0: the keep-zero rule, below)
    int qb, split;
    if (xord & 1) {
        const int slot = blockIdx.x >> 3;
        split = slot % nsplit;
        qb = ((slot / nsplit) << 3) + (blockIdx.x & 7);
        if (qb >= nqb) return;
    } else {
        qb = blockIdx.x % nqb;
        split = blockIdx.x / nqb;
    }
    // long splits first: splits 0..tr-1 take tb+1 tiles, the rest tb, so in
    // split-major order the longest workgroups are dispatched first and the
    // short ones fill the tail (knn_engine.c: choose_splits models this)
    const int tb = ntiles / nsplit, tr = ntiles - tb * nsplit;
    const int t_lo = split * tb + (split < tr ? split : tr);
    const int t_hi = t_lo + tb + (split < tr ? 1 : 0);
    const int mode = knn_mode<T>(meta, n);
    const int qrow0 = qb * KNN_TQ;
    const int myq = qrow0 + 16 * wave + j16;          // block-local query row
    const long gq = (long)q_base + myq;
    const T qn = qnorm[myq];
    // consume qn here: its first real use (the epilogue) would otherwise get
    // a vmcnt(0) from hipcc that drains the staging ring once per tile
    asm volatile("" ::"v"(qn));
    const int nfc = n_pad / BK;
    // lane list slot behind the shared bound: INT mode k+1 candidates (exact
    // keys, tightest filter); GEMM mode the whole state (slack for the
    // certificate's error margin)
    const int ujm = (mode == KNN_MODE_INT) ? (uj & 255) : (uj >> 8);

    T L[KL];
    int I[KL];
#pragma unroll
    for (int e = 0; e < KL; e++) { L[e] = KNN_INF; I[e] = -1; }
    // Shared per-query bound across splits and ring steps (qthr, bits of a
    // non-negative double, atomicMin).  Any split's thr bounds the query's
    // (k+1)-th candidate over ALL rows (>= k+1 distinct candidates lie below
    // it), so a split may start filtering at the smallest bound published so
    // far.  Every value ever stored is a valid bound, so a stale read only
    // costs filter strength; the returning atomic reads it at the memory
    // side.  part_T still records the bound this split filtered with.
    // (fp32: every published value came from an fp32 bound, so the
    // conversion back is exact)
    T thr = (T)KNN_INF;
    if (qthr != nullptr && myq < nq)
        thr = (T)__longlong_as_double((long long)atomicMin(qthr + myq, 0x7ff0000000000000ull));
    if (myq >= nq) thr = -(T)KNN_INF;   // padding queries reject every candidate
    asm volatile("" ::"v"(thr));

    const int total = (mode == KNN_MODE_SCAN || t_hi <= t_lo) ? 0 : (t_hi - t_lo) * nfc;

    acc_t acc[8];
#pragma unroll
    for (int mt = 0; mt < 8; mt++) acc[mt] = (acc_t){0, 0, 0, 0};
    // fp64 H16: fp32 partial sums of up to 16 chunks (see knn_to_h4)
    flt4 acc32[H16D ? 8 : 1];
#pragma unroll
    for (int mt = 0; mt < (H16D ? 8 : 1); mt++) acc32[mt] = (flt4){0, 0, 0, 0};
    int grp = 0;
    auto flush32 = [&]() {
        if constexpr (H16D) {
#pragma unroll
            for (int mt = 0; mt < 8; mt++) {
#pragma unroll
                for (int r = 0; r < 4; r++) acc[mt][r] += (double)acc32[H16D ? mt : 0][r];
                acc32[H16D ? mt : 0] = (flt4){0, 0, 0, 0};
            }
            grp = 0;
        }
    };

    LDS_AS char *lds = (LDS_AS char *)smem;

    // ---- staging cursor (wave-uniform; clamps at the last chunk) ---------
    const int lr = lane >> 3, ls = lane & 7;
    const int seg_b = 16 * (ls ^ lr);                        // byte offset within the 128-B row
    // norms land permuted as [g][k] = norm of tile row 16(k>>2) + ROW(g, k&3)
    // (the rows lane group g holds, in register order), in 4-byte pieces:
    // 256 pieces a tile for fp64 (waves 0..3), 128 for fp32 (waves 0,1);
    // the other waves repeat the same bytes
    constexpr int NU = 128 * ES / 4;                         // 4-byte pieces per tile
    const int cn_unit = (__builtin_amdgcn_readfirstlane(wave) & (NU / 64 - 1)) * 64 + lane;
    const int cn_p = ES == 8 ? cn_unit >> 1 : cn_unit;       // norm index g*32 + k
    const int cn_k = cn_p & 31;
    const int cn_src_off = (16 * (cn_k >> 2) + rowmap(cn_p >> 5, cn_k & 3)) * ES +
                           (ES == 8 ? (cn_unit & 1) * 4 : 0);
    int s_c = 0, s_t = t_lo, s_fc = 0;                       // chunk being staged
    // Every wave stages its own m-tile and its own 16 queries.  All staging
    // addresses are scalar (wave_s, not the VGPR wave index): deriving the
    // LDS destination per load from a VGPR (v_readfirstlane into M0) cost
    // 2.9 ms.  STG = 1 moves all staging to waves 0..3 (they load for
    // their SIMD partner w+4 too): 0.6 ms slower on fp64 element rows once
    // addressing is scalar.
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    constexpr bool SELF = STG == 0;
    const bool loader = SELF || wave_s < 4;
    auto glds1 = [&](int i) {
        if (!loader) return;
        const unsigned r8 = 8u * RS * (unsigned)n_pad;             // 8 rows, bytes
        const size_t fo = (size_t)128 * s_fc;                      // chunk offset, bytes
        const char *cb = (const char *)cblk +
                         (size_t)s_t * KNN_TC * n_pad * RS + fo;
        const char *qb0 = (const char *)qblk + (size_t)qrow0 * n_pad * RS + fo;
#pragma unroll
        for (int hw = 0; hw < (SELF ? 1 : 2); hw++) {
            const int ww = SELF ? wave_s : (wave_s & 3) + 4 * hw;
            const unsigned dst = (unsigned)(uintptr_t)lds + (unsigned)(s_c & (NST - 1)) * 32768u +
                                 (unsigned)ww * 2048u;
            const unsigned vo = (unsigned)((16 * ww + lr) * n_pad * RS + seg_b);
            if (i == 0) bglds16(knn_rsrc(cb), vo, dst);
            if (i == 1) bglds16(knn_rsrc(cb), vo + r8, dst + 1024);
            if (i == 2) bglds16(knn_rsrc(qb0), vo, dst + 16384);
            if (i == 3) bglds16(knn_rsrc(qb0), vo + r8, dst + 17408);
        }
    };
    auto advance = [&]() {
        s_c++;
        if (s_c < total) {
            if (++s_fc == nfc) {
                s_fc = 0;
                s_t++;
            }
        }
    };
    // norm slice of tile t (clamped to the split) into ring slot `slot`
    auto gnorm = [&](int t, int slot) {
        if (!loader) return;
        const int ts = t < t_hi ? t : t_hi - 1;
        const unsigned ndst = (unsigned)(uintptr_t)lds + NST * 32768u + (unsigned)(slot & 7) * 1024u +
                              (unsigned)(wave_s & (NU / 64 - 1)) * 256u;
        glds4((const char *)(cnorm + (size_t)ts * KNN_TC) + cn_src_off, ndst);
    };

    // ---- epilogue of tile t: d^2, threshold filter, insertion ------------
    // Common case (late in the scan): d^2, one masked-tile test on SGPRs,
    // the lane minimum against the bound, one ballot.  The per-candidate
    // pending mask is built only when some lane has a survivor.
    auto epilogue = [&](int t, acc_t (&A)[8]) {
        const LDS_AS T *cng = (const LDS_AS T *)(lds + NST * 32768 + (t & 7) * 1024) + 32 * g;
        const T lim = L[KL - 1] < thr ? L[KL - 1] : thr;
        // wave-uniform (scalar): only the block's last tile has rows >= nc,
        // and only tiles holding one of this wave's queries contain a self
        // pair.  Derived from wave_s, not the VGPR wave index, so it is a
        // scalar branch -- from the VGPR form hipcc predicated all 32
        // elements with exec masks (~9 issued instructions each).
        const int row0 = t * KNN_TC;
        const long gt0 = (long)c_base + row0, gw0 = (long)q_base + qrow0 + 16 * wave_s;
        const bool masked = (row0 + KNN_TC > nc) || (gw0 < gt0 + KNN_TC && gt0 < gw0 + 16);
        // d^2 overwrites the accumulators in place; the norms are read in
        // two halves of 4 m-tiles (one wait each, 16 temporaries)
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            T cnr[4][4];
#pragma unroll
            for (int m4 = 0; m4 < 4; m4++) {
                const int mt = 4 * hh + m4;
                if constexpr (ES == 8) {
                    const dbl2 n01 = ((const LDS_AS dbl2 *)cng)[2 * mt];
                    const dbl2 n23 = ((const LDS_AS dbl2 *)cng)[2 * mt + 1];
                    cnr[m4][0] = n01.x; cnr[m4][1] = n01.y; cnr[m4][2] = n23.x; cnr[m4][3] = n23.y;
                } else {
                    const flt4 n4 = ((const LDS_AS flt4 *)cng)[mt];
                    cnr[m4][0] = n4.x; cnr[m4][1] = n4.y; cnr[m4][2] = n4.z; cnr[m4][3] = n4.w;
                }
            }
#pragma unroll
            for (int m4 = 0; m4 < 4; m4++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    A[4 * hh + m4][r] = fma((T)-2, A[4 * hh + m4][r], qn + cnr[m4][r]);
        }
        T lanemin = A[0][0];
#pragma unroll
        for (int mt = 0; mt < 8; mt++)
#pragma unroll
            for (int r = (mt == 0 ? 1 : 0); r < 4; r++) lanemin = fmin(lanemin, A[mt][r]);
        // zeros (INT-mode exact duplicates) and masked tiles only send the
        // wave down the slow path, where d^2 > 0 and the row mask are
        // applied (masking here made hipcc copy all 32 d^2 at the join)
        const bool any = masked || __ballot(lanemin <= lim) != 0ull;   // rare late in the scan
        if (any) {
            // INT mode: d^2 is exact and >= 0, so "S != 0" (serial:86) is d^2 > 0;
            // keep-zero (knn_ctx_set_keep_zero): no floor, a zero is a result
            const T zfloor = (mode == KNN_MODE_INT && !(xord & KNN_KARG_KEEP0)) ? (T)0 : (T)-KNN_INF;
            unsigned pend_all = 0;
#pragma unroll
            for (int mt = 0; mt < 8; mt++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    pend_all |= (A[mt][r] <= lim) ? (1u << (4 * mt + r)) : 0u;
            if (masked) {
#pragma unroll
                for (int mt = 0; mt < 8; mt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = row0 + 16 * mt + rowmap(g, r);
                        if (!(row < nc && (long)c_base + row != gq)) pend_all &= ~(1u << (4 * mt + r));
                    }
            }
            // one wave round per survivor of the busiest lane: each lane
            // takes its lowest pending candidate (= lowest row: the stable
            // tie order) through a 5-level select tree over the 32 d^2
            while (__ballot(pend_all != 0) != 0ull) {
                const int b = pend_all ? __builtin_ctz(pend_all) : 0;
                const bool b0 = b & 1, b1 = b & 2, b2 = b & 4, b3 = b & 8, b4 = b & 16;
                T v[8];
#pragma unroll
                for (int mt = 0; mt < 8; mt++) {
                    const T lo = b0 ? A[mt][1] : A[mt][0];
                    const T hi = b0 ? A[mt][3] : A[mt][2];
                    v[mt] = b1 ? hi : lo;
                }
                const T w0 = b2 ? v[1] : v[0], w1 = b2 ? v[3] : v[2];
                const T w2 = b2 ? v[5] : v[4], w3 = b2 ? v[7] : v[6];
                const T x0 = b3 ? w1 : w0, x1 = b3 ? w3 : w2;
                // d^2 <= zfloor (INT mode: an exact duplicate, S == 0) is
                // dropped here rather than in the survivor mask (rare)
                const T dsel = b4 ? x1 : x0;
                const T dd = (pend_all && dsel > zfloor) ? dsel : (T)KNN_INF;
                const int ii = (int)(c_base + row0 + 16 * (b >> 2) + rowmap(g, b & 3));
                pend_all &= pend_all - 1;
                list_insert<KL>(L, I, dd, ii);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 8; mt++) A[mt] = (acc_t){0, 0, 0, 0};
        if (!any) return;
        // shared threshold of the query's 4 lanes: their union holds
        // >= 4(ujm+1) >= k+1 entries <= max_h L_h[ujm], and every lane
        // already rejects >= min_h L_h[KL-1]
        T lmin = L[KL - 1], u = L[0];
#pragma unroll
        for (int e = 1; e < KL; e++) u = (e == ujm) ? L[e] : u;
        lmin = fmin(lmin, __shfl_xor(lmin, 16));
        lmin = fmin(lmin, __shfl_xor(lmin, 32));
        u = fmax(u, __shfl_xor(u, 16));
        u = fmax(u, __shfl_xor(u, 32));
        thr = fmin(thr, fmin(lmin, u));   // monotone: rejections so far stay above it
    };

    // ---- fragments: quarter (p, h) = m-tiles 4h..4h+3 of piece p ---------
    auto cs_of = [&](int c) { return lds + (c & (NST - 1)) * 32768; };
    // 16-byte slot of (row, segment 4p+g) in a 16-row image
    const int fslot = j16 * 128 + 16 * ((4 * 0 + g) ^ (j16 & 7));
    const int fslot1 = j16 * 128 + 16 * ((4 * 1 + g) ^ (j16 & 7));
    frag_t f0[4], f1[4];
    frag_t b0, b1;
    auto rd = [&](LDS_AS char *st, int p, int h, frag_t (&f)[4], int j) {
        f[j] = *(const LDS_AS frag_t *)(st + (4 * h + j) * 2048 + (p ? fslot1 : fslot));
    };
    auto rdq = [&](LDS_AS char *st, int p) {
        return *(const LDS_AS frag_t *)(st + 16384 + wave * 2048 + (p ? fslot1 : fslot));
    };
    // one segment: 8 MFMAs on quarter h with fragments f and query piece b;
    // between them the reads `rdj(j)` of the next segment and one staging
    // load `stage()` (sched_barrier-pinned order)
    constexpr int SJ = 2;   // m-tile pair after which a segment's load issues
    // fp64: an m-tile's two k-steps back to back (measured 1.2% faster than
    // interleaving); fp32: v_mfma_f32_16x16x4 has a 40-cycle dependent
    // latency against a 32-cycle issue, so its 4 k-steps go round-robin
    // over the 4 m-tiles.
    constexpr bool PAIRS = ES == 8;
    auto segment = [&](const frag_t (&f)[4], const frag_t &b, int h, auto &&rdj, auto &&stage) {
        if constexpr (PAIRS) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                rdj(j);
                if (j == SJ) stage();
#pragma unroll
                for (int e = 0; e < KSF; e++) acc[4 * h + j] = KT<T>::mfma(f[j][e], b[e], acc[4 * h + j]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[4 * h + j] = KT<T>::mfma(f[j][0], b[0], acc[4 * h + j]);
                rdj(j);
                if (j == SJ) stage();
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int e = 1; e < KSF; e++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[4 * h + j] = KT<T>::mfma(f[j][e], b[e], acc[4 * h + j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto nothing = [&]() {};

    if (total > 0) {
        // prologue: norms of the first two tiles, chunks 0..2 whole and
        // chunk 3's load 0 (its loads 1..3 belong to S0..S2 of chunk 0)
        gnorm(t_lo, t_lo);
        gnorm(t_lo + 1, t_lo + 1);
#pragma unroll
        for (int x = 0; x < NST - 1; x++) {
#pragma unroll
            for (int i = 0; i < 4; i++) glds1(i);
            advance();
        }
        glds1(0);
        // norms + chunk 0 landed: younger are chunks 1, 2 and chunk 3's
        // load 0 -- 9 instructions per staged wave (18 for a loader of two)
        if constexpr (SELF) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        b0 = rdq(cs_of(0), 0);
#pragma unroll
        for (int j = 0; j < 4; j++) rd(cs_of(0), 0, 0, f0, j);

        int c = 0;
        for (int t = t_lo; t < t_hi; t++) {
            gnorm(t + 2, t + 2);
            for (int fc = 0; fc < nfc; fc++, c++) {
                LDS_AS char *cs = cs_of(c);
                if constexpr (H16 == 2) {
                    // fp16 shadow rows: a 16-byte slot is a whole 8-half
                    // operand, two v_mfma_f32_16x16x32_f16 per m-tile per
                    // 64-feature chunk, no conversion.  fp64: fp32 partial
                    // sums flushed every 4 chunks (256 features, knn_to_h4)
                    glds1(1);
                    glds1(2);
                    glds1(3);
                    const knn_h8 q0 = *(const LDS_AS knn_h8 *)(cs + 16384 + wave * 2048 + fslot);
                    const knn_h8 q1 = *(const LDS_AS knn_h8 *)(cs + 16384 + wave * 2048 + fslot1);
#pragma unroll
                    for (int mt = 0; mt < 8; mt++) {
                        const knn_h8 a0 = *(const LDS_AS knn_h8 *)(cs + mt * 2048 + fslot);
                        const knn_h8 a1 = *(const LDS_AS knn_h8 *)(cs + mt * 2048 + fslot1);
                        if constexpr (H16D) {
                            acc32[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, q0, acc32[mt], 0, 0, 0);
                            acc32[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, q1, acc32[mt], 0, 0, 0);
                        } else {
                            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, q0, acc[mt], 0, 0, 0);
                            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, q1, acc[mt], 0, 0, 0);
                        }
                    }
                    if constexpr (H16D) {
                        if (++grp == 4) flush32();
                    }
                    advance();
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    if constexpr (SELF) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    glds1(0);
                    continue;
                }
                if constexpr (H16 == 1 && H16D) {
                    // fp16 MFMA on converted fp64 fragments (knn_to_h4); the
                    // output is in the fp32 layout (rowmap)
                    glds1(1);
                    glds1(2);
                    glds1(3);
                    const knn_h4 bh = knn_to_h4(rdq(cs, 0), rdq(cs, 1));
#pragma unroll
                    for (int mt = 0; mt < 8; mt++) {
                        const frag_t a0 = *(const LDS_AS frag_t *)(cs + mt * 2048 + fslot);
                        const frag_t a1 = *(const LDS_AS frag_t *)(cs + mt * 2048 + fslot1);
                        acc32[H16D ? mt : 0] = __builtin_amdgcn_mfma_f32_16x16x16f16(
                            knn_to_h4(a0, a1), bh, acc32[H16D ? mt : 0], 0, 0, 0);
                    }
                    if (++grp == 16) flush32();
                    advance();
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    if constexpr (SELF) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    glds1(0);
                    continue;
                }
                if constexpr (H16 == 1 && ES == 4) {
                    // fp16 MFMA on converted fp32 fragments (knn_to_h8): one
                    // 16x16x32 per m-tile per chunk.  Same staging sequence
                    // as below: loads 1..3 of chunk c+3, the chunk barrier,
                    // then load 0 of chunk c+4 into the freed stage.
                    glds1(1);
                    glds1(2);
                    glds1(3);
                    const knn_h8 bh = knn_to_h8(rdq(cs, 0), rdq(cs, 1));
#pragma unroll
                    for (int h = 0; h < 2; h++) {
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            rd(cs, 0, h, f0, j);
                            rd(cs, 1, h, f1, j);
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            acc[4 * h + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                knn_to_h8(f0[j], f1[j]), bh, acc[4 * h + j], 0, 0, 0);
                    }
                    advance();
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    if constexpr (SELF) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    glds1(0);
                    continue;
                }
                // one staging load per segment, mid-segment: loads 1..3 of
                // chunk c+3 in S0..S2, load 0 of chunk c+4 in S3 (after the
                // barrier that freed its stage).  All 8 waves issuing right
                // after the barrier cost 4% (measured); spread, ~1%.
                // S0: (p0, mt0-3) on f0 || read (p0, mt4-7) into f1
                segment(f0, b0, 0, [&](int j) { rd(cs, 0, 1, f1, j); }, [&]() { glds1(1); });
                // S1: (p0, mt4-7) on f1 || read (p1, mt0-3) + B p1
                b1 = rdq(cs, 1);
                segment(f1, b0, 1, [&](int j) { rd(cs, 1, 0, f0, j); }, [&]() { glds1(2); });
                // S2: (p1, mt0-3) on f0 || read (p1, mt4-7) into f1
                segment(f0, b1, 0, [&](int j) { rd(cs, 1, 1, f1, j); }, [&]() { glds1(3); });
                advance();
                {
                    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this stage's reads done
                    // chunk c+1 landed: chunks c+2, c+3 may stay in flight
                    if constexpr (SELF) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    __builtin_amdgcn_s_barrier();         // chunk c+1 visible; stage c%4 free
                }
                LDS_AS char *cs1 = cs_of(c + 1);
                b0 = rdq(cs1, 0);
                // S3: (p1, mt4-7) on f1 || read (p0, mt0-3) of chunk c+1
                segment(f1, b1, 1, [&](int j) { rd(cs1, 0, 0, f0, j); }, [&]() { glds1(0); });
            }
            flush32();
            epilogue(t, acc);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no LDS-DMA left in flight
    }

    // INT mode, exact d^2: if no lane's list ends at thr, nothing equal to
    // thr was ever turned away (the filter rejects only d^2 > thr, and a
    // full list only what ranks after its last entry), so every rejected
    // candidate has d^2 >= next(thr).  Publishing that lets the certificate
    // accept a k-th entry equal to thr -- on integer data with the top k
    // split evenly over the 4 lanes, thr IS the k-th value.
    T lastmin = L[KL - 1];
    lastmin = fmin(lastmin, __shfl_xor(lastmin, 16));
    lastmin = fmin(lastmin, __shfl_xor(lastmin, 32));
    T pub = thr;
    if (mode == KNN_MODE_INT && lastmin > thr && thr < (T)KNN_INF) pub = nextafter(thr, (T)KNN_INF);
    if (myq < nq) {
        const size_t base = (((size_t)split * nq_pad + myq) * 4 + g) * KL;
#pragma unroll
        for (int e = 0; e < KL; e++) {
            part_d[base + e] = (double)L[e];
            part_i[base + e] = I[e];
        }
        if (g == 0) {
            part_T[(size_t)split * nq_pad + myq] = (double)pub;
            if (qthr != nullptr && thr < (T)KNN_INF)
                atomicMin(qthr + myq, (unsigned long long)__double_as_longlong((double)thr));
        }
    }
}

// One step of a DPP argmin by (d, idx): lanes the row/bank masks leave out,
// and lanes whose source lies outside their row, see (+inf, INT_MAX)
template <int CTRL, int RM, int BM>
__device__ __forceinline__ void dpp_argmin_step(double &d, int &i)
{
    const int lo = __double2loint(d), hi = __double2hiint(d);
    const int olo = __builtin_amdgcn_update_dpp(0, lo, CTRL, RM, BM, false);
    const int ohi = __builtin_amdgcn_update_dpp(0x7ff00000, hi, CTRL, RM, BM, false);
    const int oi = __builtin_amdgcn_update_dpp(0x7fffffff, i, CTRL, RM, BM, false);
    const double od = __hiloint2double(ohi, olo);
    const bool take = (od < d) || (od == d && oi < i);
    d = take ? od : d;
    i = take ? oi : i;
}
// the same on packed (d^2 << 32 | idx) keys (INT mode with d^2 < 2^32)
template <int CTRL, int RM, int BM>
__device__ __forceinline__ void dpp_min_u64_step(unsigned long long &key)
{
    const unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)lo, CTRL, RM, BM, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)hi, CTRL, RM, BM, false);
    const unsigned long long ok = ((unsigned long long)ohi << 32) | olo;
    key = ok < key ? ok : key;
}
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
}

// ---------------------------------------------------------------------------
// k_merge: one wave per query.  Lane j < lpq*nsplit owns partial list j
// (lpq lists per query and split: 4 from k_dist_topk, 2 from k_dist_topk_i8),
// lane lpq*nsplit the running state; KP+1 rounds of a wave argmin over the
// heads select the new state (KP entries by (d^2, idx)) and the smallest
// dropped value, which lowers the rejection bound T.  GEMM mode: entries
// new in this step get their exact reference-order S from the resident
// block (the only step at which their rows are on this device).
// ---------------------------------------------------------------------------
// PF > 0: each lane's next PF entries are loaded up front, unconditionally
// (lanes without a list read a +inf list), and shifted as its head is taken;
// the running state is split over KP / PF lanes (sorted runs of PF), so a
// lane only goes back to memory after PF wins.  PF = 0: the head is loaded
// as it is consumed (one memory latency on every one of the KP + 1 rounds).
__device__ const double k_inf_d[8] = {KNN_INF, KNN_INF, KNN_INF, KNN_INF, KNN_INF, KNN_INF, KNN_INF, KNN_INF};
__device__ const int k_inf_i[8] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff,
                                   0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
template <typename TE, int KP, int S, int PF = 0>
__global__ __launch_bounds__(256) void k_merge(
    const double *__restrict__ part_d, const int *__restrict__ part_i,
    const double *__restrict__ part_T, int nsplit, int lpq, int kl, int nq, int nq_pad, int first_step,
    double *__restrict__ st_d, double *__restrict__ st_x, int *__restrict__ st_i,
    double *__restrict__ st_T, const TE *__restrict__ qblk, size_t qnorm_off,
    const knn_merge_blocks_t mb, int n, int n_pad,
    const double *__restrict__ meta, int k, unsigned long long *__restrict__ qthr, int filt,
    const int *__restrict__ qperm)
{
    // S lanes a query (64, or 32 when nl + 1 <= 32: two queries a wave, so
    // twice the independent argmin chains a SIMD interleaves -- the merge is
    // bound by the latency of its KP + 1 dependent rounds, not by issue)
    constexpr int QPW = 64 / S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int seg = lane / S, sl = lane - seg * S;
    const int q0 = (blockIdx.x * 4 + wave) * QPW;
    if (q0 >= nq) return;
    // qperm (knn_order.hip): the wave's queries in a cache-friendly order
    const int qi = q0 + seg;
    const bool qv = qi < nq;
    const int q = (qperm != nullptr && qv) ? qperm[qi] : qi;
    const unsigned long long segm = (S == 64) ? ~0ull : (0xffffffffull << (32 * seg));
    const int mode = knn_mode<TE>(meta, n);
    const int nl = lpq * nsplit;   // partial lists: [split][query][lpq][kl]
    // keep-zero (bit 1 of filt, wave-uniform): an S == 0 candidate is a
    // result like any other, so no slot is set aside for excluded zeros --
    // z = 0 in the window, the early stop and the publication below.  The
    // state still keeps k + 1 entries and publishes the (k+1)-th: the
    // certificates compare the k-th kept key with the bound the filters
    // rejected at (tau < T), which the k-th itself as the bound would fail.
    const bool keep0 = (filt & KNN_KARG_KEEP0) != 0;
    filt &= 1;

    static_assert(PF == 0 || (PF == 8 && KP % PF == 0), "prefetch depth");
    constexpr int NST = PF > 0 ? KP / PF : 1;   // state lanes
    const double *src_d = nullptr;
    const int *src_i = nullptr;
    int len = KP, opos0 = 0;   // opos0: the lane's first slot in the old state
    if (qv && sl < nl) {
        const int s = sl / lpq, gg = sl - s * lpq;
        const size_t base = (((size_t)s * nq_pad + q) * lpq + gg) * kl;
        src_d = part_d + base;
        src_i = part_i + base;
        len = kl;
    } else if (qv && !first_step && sl >= nl && sl < nl + NST) {
        opos0 = (sl - nl) * (KP / NST);
        src_d = st_d + (size_t)q * KP + opos0;
        src_i = st_i + (size_t)q * KP + opos0;
        len = KP / NST;
    }
    int pos = 0;
    constexpr int R = PF > 0 ? PF : 1;
    double Ld[R];
    int Li[R];
    double hd;
    int hi;
    if constexpr (PF > 0) {
        if (!src_d) {
            src_d = k_inf_d;
            src_i = k_inf_i;
            len = 0;
        }
#pragma unroll
        for (int j = 0; j < R; j++) {   // unconditional: one latency for all
            Ld[j] = src_d[j];
            Li[j] = src_i[j];
        }
#pragma unroll
        for (int j = 0; j < R; j++) Ld[j] = j < len ? Ld[j] : KNN_INF;
        hd = Ld[0];
        hi = hd == KNN_INF ? 0x7fffffff : Li[0];
    } else {
        hd = src_d ? src_d[0] : KNN_INF;
        hi = src_d ? src_i[0] : 0x7fffffff;
        if (hd == KNN_INF) hi = 0x7fffffff;
    }

    // T: rejection bound of the lane filters (every candidate a lane turned
    // away has d^2 >= T); Td: smallest d^2 dropped by a merge (those rank
    // after every kept entry by (d^2, idx), so only the GEMM certificate
    // needs them).
    double T = KNN_INF, Td = KNN_INF;
    if (qv && sl < nsplit) T = part_T[(size_t)sl * nq_pad + q];
    if (qv && sl == nl && !first_step) { T = st_T[2 * (size_t)q]; Td = st_T[2 * (size_t)q + 1]; }
    for (int off = S / 2; off > 0; off >>= 1) {
        T = fmin(T, __shfl_xor(T, off));
        Td = fmin(Td, __shfl_xor(Td, off));
    }

    // state slot r (0..KP-1) is kept by segment lane r % S in register r / S
    constexpr int NS = (KP + S - 1) / S;
    double sd[NS];
    int si[NS], ssrc[NS], spos[NS];
#pragma unroll
    for (int x = 0; x < NS; x++) { sd[x] = KNN_INF; si[x] = -1; ssrc[x] = 0; spos[x] = 0; }
    // INT mode: the state only needs the k + 1 smallest (exact keys, zeros
    // never admitted: k_finalize reads the k-th, the publication below the
    // (k+1)-th, and a later merge's top k + 1 comes from these and its new
    // lists); Td, the smallest dropped value, is a GEMM-certificate term
    const int rmax = (mode == KNN_MODE_INT && k + 1 < KP) ? k : KP;
    // INT mode with every d^2 below 2^32 ((|q| + |c|)^2 <= 4 max|x|^2 <
    // 2^32; list keys are exact integers, idx >= 0): argmin on packed keys
    const bool small_keys = mode == KNN_MODE_INT && 4.0 * meta[KNN_META_MAXNORM] < 4294967295.0;
    // GEMM mode: selection stops once the head passes the exact-S window of
    // the k-th kept entry (dk + 2E, below): such an entry can never reach
    // the top k, now or after a later merge (d^2_k only falls), so it is
    // dropped with everything behind it and the head becomes Td, the
    // smallest dropped value -- a query takes ~k + 1 rounds instead of
    // KP + 1, and only a query whose near ties crowd the window fills the
    // state.  dkc = the (k + z)-th selected entry, z = those <= E (d^2 <= E:
    // possibly S == 0, excluded results), as the window below.
    const bool gstop = mode == KNN_MODE_GEMM && qblk != nullptr;
    const double Eq = (gstop && qv) ? knn_cert_E<TE>(n, (double)qblk[qnorm_off + q], meta[KNN_META_MAXNORM],
                                                     filt, meta[KNN_META_MAXABS])
                                    : 0.0;
    int nsel = 0, nzs = 0;
    double dkc = KNN_INF;
    bool done = false;
    for (int r = 0; r <= rmax; r++) {
        // segment argmin of the heads by (d^2, idx): DPP row shifts (the
        // minimum of each 16-lane row in its lane 15), row broadcasts into
        // the segment's last lane, read back as scalars -- no LDS permutes
        double wd = hd;
        int wi = hi;
        if (small_keys) {
            // one 64-bit key per head: (d^2, idx) order is u64 order
            unsigned long long key = hd == KNN_INF ? ~0ull
                                                   : ((unsigned long long)(unsigned)hd << 32) | (unsigned)hi;
            dpp_min_u64_step<0x111, 0xf, 0xf>(key);
            dpp_min_u64_step<0x112, 0xf, 0xf>(key);
            dpp_min_u64_step<0x114, 0xf, 0xf>(key);
            dpp_min_u64_step<0x118, 0xf, 0xf>(key);
            dpp_min_u64_step<0x142, 0xa, 0xf>(key);
            if constexpr (S == 64) dpp_min_u64_step<0x143, 0xc, 0xf>(key);
            wd = key == ~0ull ? KNN_INF : (double)(unsigned)(key >> 32);
            wi = key == ~0ull ? 0x7fffffff : (int)(unsigned)key;
        } else {
            dpp_argmin_step<0x111, 0xf, 0xf>(wd, wi);   // row_shr:1
            dpp_argmin_step<0x112, 0xf, 0xf>(wd, wi);   // row_shr:2
            dpp_argmin_step<0x114, 0xf, 0xf>(wd, wi);   // row_shr:4
            dpp_argmin_step<0x118, 0xf, 0xf>(wd, wi);   // row_shr:8
            dpp_argmin_step<0x142, 0xa, 0xf>(wd, wi);   // row_bcast:15 -> rows 1, 3
            if constexpr (S == 64) dpp_argmin_step<0x143, 0xc, 0xf>(wd, wi);   // row_bcast:31 -> rows 2, 3
        }
        {
            const double d1 = readlane_f64(wd, 63);
            const int i1 = __builtin_amdgcn_readlane(wi, 63);
            if constexpr (S == 32) {
                const double d0 = readlane_f64(wd, 31);
                const int i0 = __builtin_amdgcn_readlane(wi, 31);
                wd = seg ? d1 : d0;
                wi = seg ? i1 : i0;
            } else {
                wd = d1;
                wi = i1;
            }
        }
        if (gstop && !done && dkc < KNN_INF && wd != KNN_INF &&
            wd > (dkc + 2.0 * Eq) * (1.0 + 1.0 / 524288.0)) {
            Td = fmin(Td, wd);   // every later head is >= wd
            done = true;
        }
        const bool live = wd != KNN_INF && !done;   // this query still has heads
        if (__ballot(live) == 0ull) break;
        const unsigned long long wall = __ballot(live && hd == wd && hi == wi);
        const unsigned long long who = wall & segm;
        const int wl = who ? __builtin_ctzll(who) : lane;   // wave lane of the winner
        int wpos;
        if constexpr (S == 32) {
            const unsigned w0 = (unsigned)wall, w1 = (unsigned)(wall >> 32);
            const int p0 = __builtin_amdgcn_readlane(pos, w0 ? __builtin_ctz(w0) : 0);
            const int p1 = __builtin_amdgcn_readlane(pos, w1 ? 32 + __builtin_ctz(w1) : 32);
            wpos = seg ? p1 : p0;
        } else {
            wpos = __builtin_amdgcn_readlane(pos, wall ? __builtin_ctzll(wall) : 0);
        }
        if constexpr (PF > 0) wpos += __shfl(opos0, wl);   // state runs: slot in the old state
        if (live) {
            if (r < KP) {
                nsel++;
                if (!keep0 && wd <= Eq) nzs++;
                else if (nsel - nzs == k) dkc = wd;
                if (sl == r % S) {
#pragma unroll
                    for (int x = 0; x < NS; x++) {
                        if (r / S == x) {
                            sd[x] = wd;
                            si[x] = wi;
                            ssrc[x] = (wl - seg * S >= nl && !first_step) ? 1 : 0;
                            spos[x] = wpos;
                        }
                    }
                }
            } else {
                Td = fmin(Td, wd);
            }
            if (lane == wl) {
                pos++;
                if constexpr (PF > 0) {
#pragma unroll
                    for (int j = 0; j + 1 < R; j++) {
                        Ld[j] = Ld[j + 1];
                        Li[j] = Li[j + 1];
                    }
                    Ld[R - 1] = KNN_INF;
                    if (pos % R == 0 && pos < len) {   // the prefetched run is used up (rare)
#pragma unroll
                        for (int j = 0; j < R; j++) {
                            const int pj = pos + j < len ? pos + j : len - 1;
                            Ld[j] = pos + j < len ? src_d[pj] : KNN_INF;
                            Li[j] = src_i[pj];
                        }
                    }
                    hd = Ld[0];
                    hi = hd == KNN_INF ? 0x7fffffff : Li[0];
                } else {
                    hd = (pos < len) ? src_d[pos] : KNN_INF;
                    hi = (pos < len) ? src_i[pos] : 0x7fffffff;
                    if (hd == KNN_INF) hi = 0x7fffffff;
                }
            }
        }
    }

    // INT mode (exact d^2): the new state's (k+1)-th nonzero entry bounds
    // the query's (k+1)-th candidate over all rows (k+1 distinct rows lie at
    // or below it) -- the distance kernels' qthr contract.  Published, it
    // lets every later ring step filter with the running answer instead of
    // the bound one split's lane lists reach (about the 32nd of that split's
    // rows).  fp32 blocks: rounded up to an fp32 value, as the kernels read
    // it back in fp32.
    if (qthr != nullptr && mode == KNN_MODE_INT) {
        int z = 0;
#pragma unroll
        for (int x = 0; x < NS; x++) z += __popcll(__ballot(sl + S * x < KP && sd[x] == 0.0) & segm);
        const int rk = keep0 ? k : k + z;
        if (rk < KP) {
            double u = KNN_INF;
#pragma unroll
            for (int x = 0; x < NS; x++) {
                const double v = __shfl(sd[x], seg * S + rk % S);
                if (rk / S == x) u = v;
            }
            if constexpr (sizeof(TE) == 4) u = (double)__double2float_ru(u);
            if (qv && sl == 0 && u < KNN_INF)
                atomicMin(qthr + q, (unsigned long long)__double_as_longlong(u));
        }
    }

    // GEMM mode: exact S of the new entries, from the resident block.  Let
    // z = the entries with d^2 <= E (possibly S == 0: excluded results) and
    // d^2_k the (k+z)-th d^2 of the new state.  An entry with d^2 > d^2_k +
    // 2E has S > d^2_k + E >= the k-th smallest nonzero S of the state, now
    // and after any later merge (d^2_k only falls), so it can never reach
    // the top k: its S is skipped and marked +inf (k_finalize ignores it).
    // A context begun from a byte block alone (knn_ctx_begin_s8) holds no
    // element rows: if the device meta says GEMM after all (a speculative
    // begin on data that did not qualify), no exact S is computed -- the new
    // entries get S = +inf and k_finalize fails every query (it sees no
    // query norms either) instead of reading through a null block
    const bool exact_ok = mode == KNN_MODE_GEMM && qblk != nullptr;
    double win = KNN_INF;
    if (exact_ok) {
        const double E = qv ? knn_cert_E<TE>(n, (double)qblk[qnorm_off + q], meta[KNN_META_MAXNORM], filt,
                                             meta[KNN_META_MAXABS])
                            : 0.0;
        int z = 0;
#pragma unroll
        for (int x = 0; x < NS; x++) z += __popcll(__ballot(sl + S * x < KP && sd[x] <= E) & segm);
        const int rk = keep0 ? k - 1 : k - 1 + z;
        double dk = KNN_INF;
        if (rk < KP) {
#pragma unroll
            for (int x = 0; x < NS; x++) {
                const double v = __shfl(sd[x], seg * S + rk % S);
                if (rk / S == x) dk = v;
            }
        }
        if (dk < KNN_INF) win = (dk + 2.0 * E) * (1.0 + 1.0 / 1048576.0);
    }
    double sx[NS];
#pragma unroll
    for (int x = 0; x < NS; x++) {
        sx[x] = sd[x];
        if (qv && sl + S * x < KP && mode == KNN_MODE_GEMM && si[x] >= 0) {
            if (ssrc[x]) {
                sx[x] = st_x[(size_t)q * KP + spos[x]];
            } else if (exact_ok && sd[x] <= win) {
                // the row's block (new entries come from this step's blocks)
                const TE *crow = (const TE *)mb.ptr[0];
                long row = 0;
#pragma unroll
                for (int j = 0; j < KNN_SPLIT_MAXBLK; j++)
                    if (j < mb.nblk && (long)si[x] >= mb.base[j] && (long)si[x] < mb.base[j] + mb.nc[j]) {
                        crow = (const TE *)mb.ptr[j];
                        row = (long)si[x] - mb.base[j];
                    }
                sx[x] = knn_exact_sq_v<TE>(qblk + (size_t)q * n_pad, crow + (size_t)row * n_pad, n_pad);
            } else {
                sx[x] = KNN_INF;
            }
        }
    }
    // every read of the old state (any lane, any slot) completes before the
    // first write (wave-private queries)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (qv) {
#pragma unroll
        for (int x = 0; x < NS; x++) {
            const int r = sl + S * x;
            if (r < KP) {
                st_d[(size_t)q * KP + r] = sd[x];
                st_x[(size_t)q * KP + r] = sx[x];
                st_i[(size_t)q * KP + r] = (sd[x] == KNN_INF) ? -1 : si[x];
            }
        }
        if (sl == 0) { st_T[2 * (size_t)q] = T; st_T[2 * (size_t)q + 1] = Td; }
    }
}

// ---------------------------------------------------------------------------
// The rank merge (k_merge_rank, k_merge_rank16): the INT-mode merge of int8
// lane lists (k_dist_topk_i8: exact integer d^2 < 2^31; zeros never admitted,
// or -- keep-zero -- admitted as the results they are: nothing here tells
// them apart) by ranking instead of k_merge's argmin rounds (k + 1 dependent
// wave-argmins of ~2k cycles each: 33 us for 7500 queries, 0.19 ms for 60000,
// rocprofv3).  G lanes serve a query; a lane holds one list, and -- after the
// first step of a ring -- one entry of the query's state.
//
// Bounds.  The shared bound qthr[q] is an upper bound on the query's (k+1)-th
// smallest d^2 over all rows (k + 1 distinct rows lie at or below it), so no
// entry above it can be among the k + 1 smallest.  The (k+1)-th smallest key
// among the lists' first HD entries and the state is a second such bound (a
// subset's (k+1)-th is never below the whole set's), usually far tighter: the
// shared bound alone admitted ~100-170 entries a query at P = 1 (7 splits x
// 2 lists x 12), and the rank loop's broadcast LDS reads grow with C^2 / 64
// (89 us a merge of 60000 queries, nearly all of it those reads; round 6).
//
// Ranks.  Every list and state entry at or below both bounds is compacted
// into the group's LDS buffer as a u64 key (d^2 << 32 | idx: u64 order is the
// reference's (d, idx) order; keys are distinct).  A candidate's
// rank is the number of smaller keys: C compares a candidate (~31..60 at the
// end of a search), 64 / G candidates a lane a round.
//
// Outcome.  Not the search's last merge (fin == 0): rank r < k + 1 goes to
// state slot r, T and Td are kept, and the rank-k key is published into qthr,
// as k_merge's INT mode does.  The last merge (fin != 0, knn_ctx_end) does
// k_finalize's INT-mode work in the same pass instead: rank r < k is record
// r, slots past the candidates are {inf, 0, 0}, and the query is certified
// (tau_k < T) or put on the rescan list with the bounds its rescan (fbound)
// and int8 re-search (qthr) start from.  With fewer than k + 1 candidates
// under the bounds those come from a fallback pass over every entry of the
// lists and the state -- with +inf instead they scanned cold (2.8 ms of
// k_rescan_step for two MNIST queries).
// ---------------------------------------------------------------------------
typedef unsigned long long knn_u64x2 __attribute__((ext_vector_type(2)));
struct knn_fin_args {
    knn_neighbour_t *out;
    int *fail_count, *fail_list, *mode_out;
    double *fbound;
    const double *meta;
    double lim;   // 2^51 / 4n, knn_mode_lim
    int n, force_fail;
};
// list entries as 32-bit d^2 (exact integers < 2^31; +inf -> RANK_DINF, above
// every bound): half the registers of doubles, 5 -> 6 waves a SIMD
constexpr unsigned RANK_DINF = 0xffffffffu;
constexpr unsigned long long RANK_NOKEY = ~0ull;   // above every key

__device__ __forceinline__ unsigned long long rank_key(unsigned d, int id)
{
    return ((unsigned long long)d << 32) | (unsigned)id;
}
__device__ __forceinline__ double rank_key_d2(unsigned long long key) { return (double)(unsigned)(key >> 32); }

// list l of a query: split l / lpq, list l % lpq of that split
__device__ __forceinline__ size_t rank_list_base(int l, int lpq, int q, int nq_pad, int kl)
{
    const int s = lpq == 2 ? l >> 1 : lpq == 4 ? l >> 2 : l / lpq, g = l - s * lpq;
    return (((size_t)s * nq_pad + q) * lpq + g) * kl;
}

// List l of query q (l < nl; other lanes hold none) and the number of its
// entries at or below Bu -- a prefix: the list is sorted, +inf past its end.
// Its first 4 entries, then the rest in one round if the 4th is still at or
// below the bound (two dependent rounds at most: the merge is latency-bound);
// full: all at once.
template <int KL>
__device__ __forceinline__ int rank_load_lists(const double *__restrict__ part_d, const int *__restrict__ part_i,
                                               int l, int nl, int lpq, int q, int nq_pad, unsigned Bu, bool full,
                                               unsigned (&d)[KL], int (&id)[KL])
{
#pragma unroll
    for (int e = 0; e < KL; e++) {
        d[e] = RANK_DINF;
        id[e] = 0;
    }
    int c = 0;
    if (l < nl) {
        constexpr int H = KL < 4 ? KL : 4;
        const size_t base = rank_list_base(l, lpq, q, nq_pad, KL);
        auto load = [&](int e) {
            const double v = part_d[base + e];
            d[e] = v < 4294967295.0 ? (unsigned)v : RANK_DINF;
            id[e] = part_i[base + e];
        };
#pragma unroll
        for (int e = 0; e < H; e++) load(e);
        if (KL > H && (full || d[H - 1] <= Bu)) {
#pragma unroll
            for (int e = H; e < KL; e++) load(e);
        }
#pragma unroll
        for (int e = 0; e < KL; e++) c += d[e] <= Bu ? 1 : 0;
    }
    return c;
}

// the lanes of this lane's group of G
template <int G>
__device__ __forceinline__ unsigned long long rank_gmask()
{
    if constexpr (G == 64) return ~0ull;
    else return ((1ull << G) - 1ull) << (threadIdx.x & 63 & ~(G - 1));
}

// exclusive prefix within the group of the per-lane counts ct < 2^NB, and
// their sum: bit-sliced through ballots (a whole wave: mbcnt)
template <int G, int NB>
__device__ __forceinline__ int rank_prefix(int ct, int &sum)
{
    int pre = 0;
    sum = 0;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const unsigned long long m = __ballot((ct >> b) & 1) & rank_gmask<G>();
        if constexpr (G == 64)
            pre += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) << b;
        else
            pre += __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull)) << b;
        sum += __popcll(m) << b;
    }
    return pre;
}

// the group's LDS writes are visible to its reads
__device__ __forceinline__ void rank_lds_sync()
{
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// One round of ranks: lane gl takes the keys x[t] = buf[b0 + gl + G t] (past
// C: RANK_NOKEY) and counts the keys of buf[0, C) below each -- broadcast
// reads, 2 keys each.  skip: leave the slots out that are dead in the whole
// group this round (it costs a test a slot; C and b0 are group-uniform).
template <int G>
__device__ __forceinline__ void rank_count(const LDS_AS unsigned long long *buf, int C, int b0, int gl, bool skip,
                                           unsigned long long (&x)[64 / G], int (&r)[64 / G])
{
    constexpr int NT = 64 / G;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int my = b0 + gl + G * t;
        x[t] = my < C ? buf[my] : RANK_NOKEY;
        r[t] = 0;
    }
    const int nt = skip ? (int)((unsigned)(C - b0 + G - 1) / G) : NT;   // live slots a lane
    int j = 0;
    for (; j + 4 <= C; j += 4) {
        const knn_u64x2 u = *(const LDS_AS knn_u64x2 *)(buf + j);
        const knn_u64x2 w = *(const LDS_AS knn_u64x2 *)(buf + j + 2);
#pragma unroll
        for (int t = 0; t < NT; t++)
            if (NT == 1 || t < nt)
                r[t] += (u.x < x[t] ? 1 : 0) + (u.y < x[t] ? 1 : 0) + (w.x < x[t] ? 1 : 0) + (w.y < x[t] ? 1 : 0);
    }
    for (; j < C; j++) {
        const unsigned long long u = buf[j];
#pragma unroll
        for (int t = 0; t < NT; t++) r[t] += u < x[t] ? 1 : 0;
    }
}

// the key of the group's lane with hit set (at most one), if any
template <int G>
__device__ __forceinline__ bool rank_pick(bool hit, unsigned long long x, unsigned long long &key)
{
    const unsigned long long at = __ballot(hit) & rank_gmask<G>();
    if (at) key = __shfl(x, __builtin_ctzll(at));
    return at != 0;
}

// The keys at ranks k - 1 and k among buf[0, C), as d^2: tau (the k-th kept)
// and tk1 (the (k+1)-th); left alone where C has no such rank.
template <int G>
__device__ __forceinline__ void rank_pick_tau(bool hit0, bool hit1, unsigned long long x, double &tau, double &tk1)
{
    unsigned long long key;
    if (rank_pick<G>(hit0, x, key)) tau = rank_key_d2(key);
    if (rank_pick<G>(hit1, x, key)) tk1 = rank_key_d2(key);
}

// The merge of one query by the G lanes gl = 0 .. G - 1 of a wave (qv: the
// group has a query; lanes of groups without one run along with nothing).
// buf: the group's LDS, room for every list and state entry.  first_step and
// fin as compile-time constants (k_merge_rank16) remove the state's code.
template <typename TE, int KP, int KL, int G>
__device__ __forceinline__ void rank_merge(
    LDS_AS unsigned long long *buf, int q, bool qv, int gl, const double *__restrict__ part_d,
    const int *__restrict__ part_i, const double *__restrict__ part_T, int nsplit, int lpq, int nq_pad,
    int first_step, double *__restrict__ st_d, double *__restrict__ st_x, int *__restrict__ st_i,
    double *__restrict__ st_T, int k, unsigned long long *__restrict__ qthr, int fin, const knn_fin_args &fa)
{
    constexpr int NT = 64 / G;
    const int nl = qv ? lpq * nsplit : 0;
    // any value read is a valid bound (it only falls); floor: d^2 are integers
    const double qb = __longlong_as_double((long long)qthr[qv ? q : 0]);
    const double B = qb >= 4294967294.0 ? 4294967294.0 : floor(qb);
    const unsigned Bu = (unsigned)B;
    // T: the smallest rejection bound of the merged lanes (and the state, on
    // the group's last lane); read with the lists (one round of loads)
    double T = KNN_INF, Td = KNN_INF;
    if (qv && gl < nsplit) T = part_T[(size_t)gl * nq_pad + q];
    if (!first_step && gl == G - 1) {
        T = fmin(T, st_T[2 * (size_t)q]);
        Td = st_T[2 * (size_t)q + 1];
    }
    const int mode = fin ? knn_mode_lim<TE>(fa.meta, fa.n, fa.lim) : KNN_MODE_INT;
    unsigned d[KL];
    int id[KL];
    int c = rank_load_lists<KL>(part_d, part_i, gl, nl, lpq, q, nq_pad, Bu, false, d, id);
    // the lane's state entry, if any (d^2 < 2^31 or +inf), and whether it
    // lies at or below the bounds
    unsigned long long skey = RANK_NOKEY;
    if (!first_step && gl < KP) {
        const double sdv = st_d[(size_t)q * KP + gl];
        const int siv = st_i[(size_t)q * KP + gl];
        if (siv >= 0 && sdv < 4294967295.0) skey = rank_key((unsigned)sdv, siv);
    }
    int cs = (skey != RANK_NOKEY && (unsigned)(skey >> 32) <= Bu) ? 1 : 0;

    // the tighter bound: rank k among the lists' first HD entries and the
    // state.  Groups of one wave differ in CH > k: the writes are predicated
    // and the barriers unconditional.
    unsigned long long lim = RANK_NOKEY;
    {
        constexpr int HD = KL < 4 ? KL : 4;
        const int hh = c < HD ? c : HD;
        int CH;
        const int preh = rank_prefix<G, 3>(hh + cs, CH);
        const bool tight = CH > k;
#pragma unroll
        for (int e = 0; e < HD; e++)
            if (tight && e < hh) buf[preh + e] = rank_key(d[e], id[e]);
        if (tight && cs) buf[preh + hh] = skey;
        rank_lds_sync();
        if (tight) {
            for (int b0 = 0; b0 < CH; b0 += 64) {
                unsigned long long x[NT];
                int r[NT];
                rank_count<G>(buf, CH, b0, gl, false, x, r);   // (nearly every slot is live)
#pragma unroll
                for (int t = 0; t < NT; t++) rank_pick<G>(b0 + gl + G * t < CH && r[t] == k, x[t], lim);
            }
            // keep the entries at or below it (the lists are sorted by d, so
            // a prefix up to ties: counted and written entry by entry)
            int c2 = 0;
#pragma unroll
            for (int e = 0; e < KL; e++) c2 += (e < c && rank_key(d[e], id[e]) <= lim) ? 1 : 0;
            c = c2;
            if (skey > lim) cs = 0;
        }
        __builtin_amdgcn_wave_barrier();   // (the subset's slots are overwritten below)
    }
    // compaction: the group's entries at or below both bounds
    int C;
    {
        int w = rank_prefix<G, 5>(c + cs, C);   // (c + cs <= KL + 1 < 32)
#pragma unroll
        for (int e = 0; e < KL; e++) {
            const unsigned long long key = rank_key(d[e], id[e]);
            if (d[e] <= Bu && key <= lim) buf[w++] = key;
        }
        if (cs) buf[w] = skey;
    }
    rank_lds_sync();

    const int kk = k + 1 < KP ? k + 1 : KP;   // entries the state keeps
    for (int off = G / 2; off > 0; off >>= 1) {
        T = fmin(T, __shfl_xor(T, off));
        Td = fmin(Td, __shfl_xor(Td, off));
    }
    // fin: the records are written as the ranks come out; the query is
    // certified (or put on the rescan list, whose pass rewrites them) after
    if (fin) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *fa.mode_out = mode;
        for (int p = gl; p < k; p += G)
            if (qv && p >= C) {   // slots past the candidates
                knn_neighbour_t rec;
                rec.distance = KNN_INF;
                rec.idx = 0;
                rec.label = 0;
                fa.out[(size_t)q * k + p] = rec;
            }
    }
    double tau = KNN_INF, tk1 = KNN_INF;
    for (int b0 = 0; b0 < C; b0 += 64) {   // (group-uniform trip count)
        unsigned long long x[NT];
        int r[NT];
        rank_count<G>(buf, C, b0, gl, true, x, r);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const bool live = b0 + gl + G * t < C;
            const double dv = rank_key_d2(x[t]);
            if (live && fin) {
                if (r[t] < k) {
                    knn_neighbour_t rec;
                    rec.distance = sqrt(dv);
                    rec.idx = (int)(unsigned)x[t] + 1;
                    rec.label = 0;
                    fa.out[(size_t)q * k + r[t]] = rec;
                }
            } else if (live) {
                if (r[t] < kk) {
                    st_d[(size_t)q * KP + r[t]] = dv;
                    st_x[(size_t)q * KP + r[t]] = dv;
                    st_i[(size_t)q * KP + r[t]] = (int)(unsigned)x[t];
                }
                if (r[t] == k) {   // the (k+1)-th: a bound on the query's (k+1)-th over all rows
                    double u = dv;
                    if constexpr (sizeof(TE) == 4) u = (double)__double2float_ru(u);
                    atomicMin(qthr + q, (unsigned long long)__double_as_longlong(u));
                }
            }
            if (fin) rank_pick_tau<G>(live && r[t] == k - 1, live && r[t] == k, x[t], tau, tk1);
        }
    }
    if (fin) {
        // k_finalize, INT mode: zeros were never admitted, so the rank-(k-1)
        // candidate is tau; a candidate a lane turned away has d^2 >= T, and
        // with d^2 == T it may precede the k-th by index: certify tau < T
        const bool intm = mode == KNN_MODE_INT && !fa.force_fail;
        const bool ok = intm && (T == KNN_INF || (C >= k && tau < T));
        if (qv && !ok && intm && C < k + 1) {
            // the fallback: the k-th and (k+1)-th over every entry -- still
            // bounds on the query's k-th / (k+1)-th over all rows
            const int c2 = rank_load_lists<KL>(part_d, part_i, gl, nl, lpq, q, nq_pad, RANK_DINF - 1, true, d, id);
            const int cs2 = skey != RANK_NOKEY ? 1 : 0;
            int C2;
            const int pre2 = rank_prefix<G, 5>(c2 + cs2, C2);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int e = 0; e < KL; e++)
                if (e < c2) buf[pre2 + e] = rank_key(d[e], id[e]);
            if (cs2) buf[pre2 + c2] = skey;
            rank_lds_sync();
            for (int b0 = 0; b0 < C2; b0 += 64) {
                unsigned long long x[NT];
                int r[NT];
                rank_count<G>(buf, C2, b0, gl, true, x, r);
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const bool live = b0 + gl + G * t < C2;
                    rank_pick_tau<G>(live && r[t] == k - 1, live && r[t] == k, x[t], tau, tk1);
                }
            }
        }
        if (qv && !ok && gl == 0) {
            fa.fail_list[atomicAdd(fa.fail_count, 1)] = q;
            fa.fbound[q] = intm ? sqrt(tau) : KNN_INF;
            // k + 1 distinct rows lie at or below the (k+1)-th kept key: a
            // valid bound for the int8 re-search to start from (knn_engine.c
            // research8; INT mode only, the search is over)
            if (intm)
                qthr[q] = (unsigned long long)__double_as_longlong(sizeof(TE) == 4 ? (double)__double2float_ru(tk1) : tk1);
        }
        return;
    }
    if (gl < KP && gl >= (C < kk ? C : kk)) {
        st_d[(size_t)q * KP + gl] = KNN_INF;
        st_x[(size_t)q * KP + gl] = KNN_INF;
        st_i[(size_t)q * KP + gl] = -1;
    }
    if (gl == 0) {
        st_T[2 * (size_t)q] = T;
        st_T[2 * (size_t)q + 1] = Td;
    }
}

// k_merge_rank: one wave a query, 4 queries a workgroup; any merge of a
// search (a state is read after the first step and written unless fin).
// Dynamic LDS: cap keys a wave (every list and state entry).
template <typename TE, int KP, int KL>
__global__ __launch_bounds__(256) void k_merge_rank(
    const double *__restrict__ part_d, const int *__restrict__ part_i, const double *__restrict__ part_T,
    int nsplit, int lpq, int nq, int nq_pad, int first_step, double *__restrict__ st_d,
    double *__restrict__ st_x, int *__restrict__ st_i, double *__restrict__ st_T, int k,
    unsigned long long *__restrict__ qthr, int cap, int fin, knn_fin_args fa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long mr_buf[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;   // wave-uniform, and no workgroup barrier below
    rank_merge<TE, KP, KL, 64>((LDS_AS unsigned long long *)mr_buf + (size_t)wave * cap, q, true, lane, part_d, part_i,
                               part_T, nsplit, lpq, nq_pad, first_step, st_d, st_x, st_i, st_T, k, qthr, fin, fa);
}

// k_merge_rank16: 16 lanes a query, 4 queries a wave, 16 a workgroup; the
// search's only merge (a P = 1 search: no state, fin) when a query has at
// most 16 lists.  k_merge_rank ran one wave a query with 14 of 64 lanes
// holding lists: 651 VALU instructions a query, most of them per-query work
// (loads, conversions, compaction, the records' sqrt) done once a wave (SQ
// counters, round 6).  Static LDS: CAPG keys a group.
template <typename TE, int KL>
__global__ __launch_bounds__(256) void k_merge_rank16(
    const double *__restrict__ part_d, const int *__restrict__ part_i, const double *__restrict__ part_T,
    int nsplit, int lpq, int nq, int nq_pad, int k, unsigned long long *__restrict__ qthr, knn_fin_args fa)
{
    constexpr int CAPG = 16 * KL + 4;   // a group's keys (+ pad: groups 32 bytes apart mod 256)
    __shared__ __attribute__((aligned(16))) unsigned long long r16_buf[16 * CAPG];
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
    const int q = blockIdx.x * 16 + grp;
    const bool qv = q < nq;
    if (__ballot(qv) == 0ull) return;   // wave-uniform; no workgroup barrier below
    rank_merge<TE, 0, KL, 16>((LDS_AS unsigned long long *)r16_buf + (size_t)grp * CAPG, q, qv, gl, part_d, part_i,
                              part_T, nsplit, lpq, nq_pad, 1, nullptr, nullptr, nullptr, nullptr, k, qthr, 1, fa);
}

// ---------------------------------------------------------------------------
// k_finalize: one wave per query.  Order by (sqrt(S), idx) -- the key the
// reference keeps (knn-serial.c:86-90) -- drop S == 0, and certify: every
// candidate outside the state has approx d^2 >= T, hence exact S >= T - E
// (E bounds the GEMM-form plus the reference's own rounding); if
// T - E > tau (the k-th kept S, with a margin so sqrt cannot collapse
// them) nothing unseen can enter the list.  Uncertified queries go to the
// rescan list.
// ---------------------------------------------------------------------------
template <typename TE, int KP>
__global__ __launch_bounds__(256) void k_finalize(
    const double *__restrict__ st_d, const double *__restrict__ st_x,
    const int *__restrict__ st_i, const double *__restrict__ st_T,
    const TE *__restrict__ qnorm, int nq, int n, int k,
    const double *__restrict__ meta, knn_neighbour_t *__restrict__ out,
    int *__restrict__ fail_count, int *__restrict__ fail_list, int *__restrict__ mode_out,
    double *__restrict__ fbound, int force_fail, int filt)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const int mode = knn_mode<TE>(meta, n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *mode_out = mode;
    if (q >= nq) return;
    knn_neighbour_t *o = out + (size_t)q * k;
    // keep-zero (bit 1 of filt): S == 0 is a result, distance 0.0
    const bool keep0 = (filt & KNN_KARG_KEEP0) != 0;
    filt &= 1;

    // force_fail: tests of the rescan pass; no query norms (a context begun
    // from a byte block alone, knn_ctx_begin_s8) outside INT mode: nothing
    // exact to certify with -- every query takes the rescan
    if (mode == KNN_MODE_SCAN || force_fail || (mode != KNN_MODE_INT && qnorm == nullptr)) {
        if (lane == 0) {
            fail_list[atomicAdd(fail_count, 1)] = q;
            fbound[q] = KNN_INF;
        }
        return;
    }
    constexpr int NS = (KP + 63) / 64;   // state slot r on lane r & 63, register r >> 6
    double sd[NS], sx[NS];
    int si[NS];
#pragma unroll
    for (int x = 0; x < NS; x++) {
        const int r = lane + 64 * x;
        sd[x] = KNN_INF;
        sx[x] = KNN_INF;
        si[x] = -1;
        if (r < KP) {
            sd[x] = st_d[(size_t)q * KP + r];
            sx[x] = st_x[(size_t)q * KP + r];
            si[x] = st_i[(size_t)q * KP + r];
        }
    }
    const double T = st_T[2 * (size_t)q], Td = st_T[2 * (size_t)q + 1];
    const int kl = k - 1;
    if (mode == KNN_MODE_INT) {
        // state is sorted by exact (d^2, idx) and zeros were never admitted
        // (or, with keep-zero, admitted as the results they are).
        // A candidate a lane filter turned away has d^2 >= T; with d^2 == T
        // it may precede the k-th by index, so certify only tau < T.
        bool valid[NS];
        int nnz = 0;
#pragma unroll
        for (int x = 0; x < NS; x++) {
            valid[x] = si[x] >= 0 && sd[x] < KNN_INF;
            nnz += __popcll(__ballot(valid[x]));
        }
        bool ok;
        double tau = KNN_INF;   // k-th exact d^2 kept: the rescan's bound
        if (nnz >= k) {
#pragma unroll
            for (int x = 0; x < NS; x++) {
                const double v = __shfl(sd[x], kl & 63);
                if ((kl >> 6) == x) tau = v;
            }
            ok = (T == KNN_INF) || (tau < T);
        } else {
            ok = (T == KNN_INF);
        }
        if (!ok) {
            if (lane == 0) {
                fail_list[atomicAdd(fail_count, 1)] = q;
                fbound[q] = sqrt(tau);
            }
            return;
        }
#pragma unroll
        for (int x = 0; x < NS; x++) {
            const int r = lane + 64 * x;
            if (r < k) {
                knn_neighbour_t rec;
                rec.distance = valid[x] ? sqrt(sd[x]) : KNN_INF;
                rec.idx = valid[x] ? si[x] + 1 : 0;
                rec.label = 0;
                o[r] = rec;
            }
        }
        return;
    }
    // GEMM mode
    bool valid[NS];
    double key[NS];
    int kid[NS], rank[NS];
#pragma unroll
    for (int x = 0; x < NS; x++) {
        valid[x] = (si[x] >= 0) && (sx[x] == sx[x]) && (keep0 || sx[x] != 0.0) && (sx[x] < KNN_INF);
        key[x] = valid[x] ? sqrt(sx[x]) : KNN_INF;
        kid[x] = valid[x] ? si[x] : 0x7fffffff;
        rank[x] = 0;
    }
    // rank = number of entries before this one by (sqrt(S), idx); unused
    // slots (key inf, id max) precede nothing
    for (int j = 0; j < 64; j++) {
#pragma unroll
        for (int y = 0; y < NS; y++) {
            const double kj = __shfl(key[y], j);
            const int ij = __shfl(kid[y], j);
#pragma unroll
            for (int x = 0; x < NS; x++)
                rank[x] += (kj < key[x] || (kj == key[x] && ij < kid[x])) ? 1 : 0;
        }
    }
    int nnz = 0;
#pragma unroll
    for (int x = 0; x < NS; x++) nnz += __popcll(__ballot(valid[x]));
    const double Tb = fmin(T, Td);
    bool ok;
    double tau = KNN_INF;   // exact S of the k-th kept: the rescan's bound
    if (nnz >= k) {
#pragma unroll
        for (int x = 0; x < NS; x++) {
            const unsigned long long at = __ballot(valid[x] && rank[x] == kl);
            if (at) tau = __shfl(sx[x], __builtin_ctzll(at));
        }
        // E (knn_cert_E): |GEMM-form d^2 - exact S| plus the reference's
        // own rounding; T and Td are GEMM-form values
        const double E = knn_cert_E<TE>(n, (double)qnorm[q], meta[KNN_META_MAXNORM], filt, meta[KNN_META_MAXABS]);
        ok = (Tb == KNN_INF) || ((Tb - E) > tau * (1.0 + 1.7763568394002505e-15));
    } else {
        ok = (Tb == KNN_INF);
    }
    if (!ok) {
        if (lane == 0) {
            fail_list[atomicAdd(fail_count, 1)] = q;
            fbound[q] = sqrt(tau);
        }
        return;
    }
#pragma unroll
    for (int x = 0; x < NS; x++) {
        if (valid[x] && rank[x] < k) {
            knn_neighbour_t rec;
            rec.distance = key[x];
            rec.idx = si[x] + 1;
            rec.label = 0;
            o[rank[x]] = rec;
        }
        const int r = lane + 64 * x;
        if (r >= nnz && r < k) {
            knn_neighbour_t rec;
            rec.distance = KNN_INF;
            rec.idx = 0;
            rec.label = 0;
            o[r] = rec;
        }
    }
}

// ---------------------------------------------------------------------------
// Exact rescan (uncertified queries): the reference's arithmetic on every
// (query, row) pair -- S = S + (a-b)^2 in j order in fp64, key sqrt(S),
// 0 < key < inf as serial:86 admits -- merged into the query's running
// rescan list (its first k entries ordered by (key, idx)).
//
// A 256-thread workgroup takes 16 queries, 4 per wave.  The wave's 4 query
// rows are wave-uniform, so hipcc reads them with scalar loads into SGPRs;
// lane l streams rows l, l+64, ... with 16-byte loads and accumulates all 4
// S in registers, so each row is read once per 4 queries (and the 4 waves
// walk the rows in step, sharing L2/L1 lines).  Zero padding past n adds
// (0-0)^2 = 0, leaving S bit-identical, so the loop runs to a whole 16 B.
//
// Filter: only keys <= dcut can reach the top k, dcut = min(the bound
// k_finalize left in fbound (the k-th key of the uncertified state: k real
// candidates lie at or below it), the k-th key of the running list).  Each
// lane keeps its KT smallest admitted keys above a floor; the merge (wave
// argmin rounds, one query at a time) takes entries only up to B, the
// smallest KT-th key of any lane that dropped one, and if the list is not
// complete by then the wave scans again above the last key taken.
// ---------------------------------------------------------------------------
template <typename TE, int KP>
__global__ __launch_bounds__(256) void k_rescan_step(
    const int *__restrict__ fail_list, int nfail, const double *__restrict__ fbound,
    const TE *__restrict__ qblk, int n_pad_q, const TE *__restrict__ cblk, size_t c_base,
    int nc, int n, int n_pad, int k, const double *rs_bound, double *rs_d, int *rs_i,
    int rows_per_chunk, size_t chunk_stride, long long self_base)
{
#pragma clang fp contract(off)
    constexpr int KT = 4, QW = 4;
    constexpr int V = 16 / (int)sizeof(TE);          // elements per 16-byte load
    constexpr int NS = (KP + 63) / 64;                // list slot r: lane r & 63, reg r >> 6
    typedef typename std::conditional<sizeof(TE) == 8, dbl2, flt4>::type vec_t;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int slot0 = blockIdx.x * 16 + wave * QW;
    if (slot0 >= nfail) return;                       // wave-uniform
    // 16-byte pieces per row, whole 128-byte pieces: rows are zero padded to
    // n_pad (query and corpus blocks alike) and S + (0-0)^2 = S
    constexpr int U = 8;
    const int nr = n_pad / V;
    // corpus chunk blockIdx.y: rows [row0, row1) into its own list set
    const int row0 = blockIdx.y * rows_per_chunk;
    const int row1 = min(nc, row0 + rows_per_chunk);
    rs_d += blockIdx.y * chunk_stride;
    rs_i += blockIdx.y * chunk_stride;

    // self_base >= 0: keep-zero -- a zero distance is admitted, and the
    // query's own row (global id self_base + q) is left out by id instead
    const bool keep0 = self_base >= 0;
    const TE *qp[QW];
    double dcut[QW];
    int slot[QW], self[QW];
    bool done[QW];
#pragma unroll
    for (int x = 0; x < QW; x++) {
        slot[x] = slot0 + x;
        done[x] = slot[x] >= nfail;
        const int q = done[x] ? fail_list[slot0] : fail_list[slot[x]];
        self[x] = keep0 ? (int)(self_base + q) : -1;
        qp[x] = qblk + (size_t)q * n_pad_q;
        const double kth = rs_bound[(size_t)(done[x] ? slot0 : slot[x]) * KP + (k - 1)];
        dcut[x] = fmin(fbound[q], kth);
    }
    // running list of each query: old (read) and new (written at the end)
    double nd[QW][NS];
    int ni[QW][NS];
    int produced[QW], pos_old[QW];
    double fd[QW];
    int fi[QW];
#pragma unroll
    for (int x = 0; x < QW; x++) {
#pragma unroll
        for (int s = 0; s < NS; s++) { nd[x][s] = KNN_INF; ni[x][s] = -1; }
        produced[x] = 0;
        pos_old[x] = 0;
        fd[x] = -1.0;
        fi[x] = -1;
    }

    for (;;) {
        double L[QW][KT];
        int I[QW][KT], cnt[QW];
#pragma unroll
        for (int x = 0; x < QW; x++) {
            cnt[x] = 0;
#pragma unroll
            for (int e = 0; e < KT; e++) { L[x][e] = KNN_INF; I[x][e] = 0x7fffffff; }
        }
        for (int row = row0 + lane; row < row1; row += 64) {
            const vec_t *cr = (const vec_t *)(cblk + (size_t)row * n_pad);
            double S[QW] = {0.0, 0.0, 0.0, 0.0};
            // 8 pieces of the row in flight before any is used (the sums are
            // dependent chains; one memory latency every 128 bytes, not 16)
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
            const int id = (int)(c_base + row);
#pragma unroll
            for (int x = 0; x < QW; x++) {
                const double d = sqrt(S[x]);
                if (!done[x] && (keep0 ? id != self[x] : d != 0.0) && d < KNN_INF && d <= dcut[x] &&
                    (d > fd[x] || (d == fd[x] && id > fi[x]))) {
                    cnt[x]++;
                    list_insert<KT>(L[x], I[x], d, id);   // rows ascend: ties stay in id order
                }
            }
        }
        bool again_any = false;
#pragma unroll
        for (int x = 0; x < QW; x++) {
            if (done[x]) continue;                        // wave-uniform
            double Bd = (cnt[x] > KT) ? L[x][KT - 1] : KNN_INF;
            int Bi = (cnt[x] > KT) ? I[x][KT - 1] : 0x7fffffff;
            wave_argmin(Bd, Bi);
            const double *od = rs_d + (size_t)slot[x] * KP;
            const int *oi = rs_i + (size_t)slot[x] * KP;
            int pos = 0;
            bool again = false;
            while (produced[x] < k) {
                double hd = (pos < KT) ? L[x][0] : KNN_INF;
                int hi = (pos < KT) ? I[x][0] : 0x7fffffff;
                if (hd == KNN_INF) hi = 0x7fffffff;
                bool mine = true;
                if (lane == 0 && pos_old[x] < k) {
                    const double v = od[pos_old[x]];
                    const int vi = (v == KNN_INF) ? 0x7fffffff : oi[pos_old[x]];
                    if (v < hd || (v == hd && vi < hi)) { hd = v; hi = vi; mine = false; }
                }
                double wd = hd;
                int wi = hi;
                wave_argmin(wd, wi);
                if (wd == KNN_INF) break;                                  // both sources empty
                if (Bd < wd || (Bd == wd && Bi < wi)) { again = true; break; }  // past B
                const int r = produced[x];
#pragma unroll
                for (int s = 0; s < NS; s++)
                    if (lane == (r & 63) && (r >> 6) == s) { nd[x][s] = wd; ni[x][s] = wi; }
                produced[x]++;
                fd[x] = wd;
                fi[x] = wi;
                const bool took = (hd == wd && hi == wi);
                const unsigned long long who = __ballot(took);
                const int wl = __builtin_ctzll(who);
                const bool from_old = __shfl((int)(!mine), wl) != 0;
                if (from_old) {
                    pos_old[x]++;
                } else if (lane == wl) {
                    // pop the lane's head (lists are shifted so L[0] is the head)
#pragma unroll
                    for (int e = 0; e < KT - 1; e++) { L[x][e] = L[x][e + 1]; I[x][e] = I[x][e + 1]; }
                    L[x][KT - 1] = KNN_INF;
                    I[x][KT - 1] = 0x7fffffff;
                    pos++;
                }
            }
            if (!again) done[x] = true;
            again_any |= again;
        }
        if (!again_any) break;
    }
    // all old-list reads precede the writes (the wave owns these slots)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int x = 0; x < QW; x++) {
        if (slot[x] >= nfail) continue;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int r = lane + 64 * s;
            if (r < KP) {
                rs_d[(size_t)slot[x] * KP + r] = nd[x][s];
                rs_i[(size_t)slot[x] * KP + r] = (nd[x][s] == KNN_INF) ? -1 : ni[x][s];
            }
        }
    }
}

__global__ void k_fill_inf(double *p, int count)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = KNN_INF;
}

// begin(): the shared bounds (+inf), the int8 kernel's cross-split summaries
// (0x7f7f7f7f pairs: above every int8-mode d^2) and the two counters
// (unresolved queries, mode) in one launch instead of three
__global__ void k_begin_init(double *qthr, unsigned long long *qsum, int nq_pad, int *counts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq_pad) qthr[i] = KNN_INF;
    if (qsum != nullptr && i < nq_pad) {
#pragma unroll
        for (int j = 0; j < 4; j++) qsum[4 * (size_t)i + j] = 0x7f7f7f7f7f7f7f7full;
    }
    if (i < 2) counts[i] = 0;
}

// the search's (unresolved, mode) pair and the meta its kernels read into
// mapped host memory (knn_ctx_end reads them after synchronising with the
// stream; the meta is knn_ctx_search_meta's -- no separate read-back copy)
__global__ void k_count_out(const int *__restrict__ src, int *__restrict__ dst, const double *__restrict__ meta,
                            double *__restrict__ dst_meta)
{
    if (threadIdx.x < 2) dst[threadIdx.x] = src[threadIdx.x];
    if (meta != nullptr && threadIdx.x < KNN_META_DOUBLES) dst_meta[threadIdx.x] = meta[threadIdx.x];
}

extern "C" int knn_launch_count_out(const int *d_count, int *mapped, const double *meta, double *mapped_meta,
                                    void *stream)
{
    hipLaunchKernelGGL(k_count_out, dim3(1), dim3(64), 0, (hipStream_t)stream, d_count, mapped, meta, mapped_meta);
    return hipGetLastError() == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

extern "C" int knn_launch_begin_init(double *qthr, unsigned long long *qsum, int nq_pad, int *counts,
                                     void *stream)
{
    const int n = nq_pad > 2 ? nq_pad : 2;
    hipLaunchKernelGGL(k_begin_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       qthr, qsum, nq_pad, counts);
    return hipGetLastError() == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

extern "C" int knn_launch_fill_inf(double *p, int count, void *stream)
{
    if (count <= 0) return KNN_OK;
    hipLaunchKernelGGL(k_fill_inf, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, p, count);
    return hipGetLastError() == hipSuccess ? KNN_OK : KNN_ERR_HIP;
}

__global__ void k_rescan_init(double *rs_d, int *rs_i, int count)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { rs_d[i] = KNN_INF; rs_i[i] = -1; }
}

// Chunked rescan, second half: per query, the running list (list 0) and the
// C chunk lists (each already the exact top k of its rows, ordered by
// (key, idx)) merge into the running list.  One wave per query; lane j
// holds the head of list j; k argmin rounds.  Row ids are disjoint across
// lists, so no entry appears twice.
template <int KP>
__global__ __launch_bounds__(256) void k_rescan_merge(int nfail, int k, int nchunk,
                                                      double *__restrict__ rs_d,
                                                      int *__restrict__ rs_i)
{
    constexpr int NS = (KP + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= nfail) return;                        // wave-uniform
    const size_t stride = (size_t)nfail * KP;
    const bool live = lane <= nchunk;
    const double *ld = rs_d + (size_t)lane * stride + (size_t)slot * KP;
    const int *li = rs_i + (size_t)lane * stride + (size_t)slot * KP;
    double nd[NS];
    int ni[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) { nd[s] = KNN_INF; ni[s] = -1; }
    int pos = 0;
    for (int r = 0; r < k; r++) {
        double hd = (live && pos < k) ? ld[pos] : KNN_INF;
        int hi = (hd == KNN_INF) ? 0x7fffffff : li[pos];
        const double md = hd;
        const int mi = hi;
        wave_argmin(hd, hi);
        if (hd == KNN_INF) break;                     // every list exhausted
#pragma unroll
        for (int s = 0; s < NS; s++)
            if (lane == (r & 63) && (r >> 6) == s) { nd[s] = hd; ni[s] = hi; }
        if (md == hd && mi == hi) pos++;             // ids are unique: one winner
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // reads of list 0 before its rewrite
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int r = lane + 64 * s;
        if (r < KP) {
            rs_d[(size_t)slot * KP + r] = nd[s];
            rs_i[(size_t)slot * KP + r] = (nd[s] == KNN_INF) ? -1 : ni[s];
        }
    }
}

__global__ void k_rescan_end(const int *__restrict__ fail_list, int nfail, int KP,
                             const double *__restrict__ rs_d, const int *__restrict__ rs_i,
                             int k, knn_neighbour_t *__restrict__ out)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nfail * k) return;
    const int slot = t / k, r = t % k;
    const int q = fail_list[slot];
    knn_neighbour_t rec;
    const double d = rs_d[(size_t)slot * KP + r];
    const int id = rs_i[(size_t)slot * KP + r];
    const bool ok = d < KNN_INF && id >= 0;
    rec.distance = ok ? d : KNN_INF;
    rec.idx = ok ? id + 1 : 0;
    rec.label = 0;
    out[(size_t)q * k + r] = rec;
}

// ---------------------------------------------------------------------------
// C launchers
// ---------------------------------------------------------------------------
template <typename T, int KL, int KP>
static int launch_dist_topk(const T *qblk, size_t q_rows_pad, size_t q_base, int nq, const T *cblk,
                            size_t c_rows_pad, size_t c_base, int nc, int n, const double *meta,
                            int nsplit, double *part_d, int *part_i, double *part_T, int nq_pad,
                            double *qthr, int k, const void *qsh, const void *csh,
                            const void *cn_ptr, int flags, float m2s, hipStream_t s)
{
    const int xord = flags & 1;
    // the kernels' xord argument: bit 0 the workgroup order, bit 1 keep-zero
    const int xarg = xord | ((flags & KNN_DIST_KEEP0) ? KNN_KARG_KEEP0 : 0);
    constexpr int dt = sizeof(T) == 8 ? KNN_F64 : KNN_F32;
    const int np = (int)knn_n_pad_dt(n, dt);
    const int nqb = (nq + KNN_TQ - 1) / KNN_TQ;
    const int ntiles = (nc + KNN_TC - 1) / KNN_TC;
    if (nqb <= 0 || nsplit <= 0 || k <= 0 || k > KP) return KNN_ERR_INVALID;
    // lane list slot of the shared bound (k_dist_topk): INT mode the max
    // over lanes covers >= k+1 candidates, GEMM mode >= max(KP, k+1)
    int uj_int = (k + 1 + 3) / 4 - 1;
    if (uj_int > KL - 1) uj_int = KL - 1;
    int uj_gemm = KP / 4 - 1 > uj_int ? KP / 4 - 1 : uj_int;
    // split fp16 filter: its error margin is ~2^-24 relative, not 2^-53, so
    // the published bound sits at the lanes' last entries (more distance
    // between the k-th and the bound for the certificate)
    if (flags & KNN_DIST_SPLIT) uj_gemm = KL - 1;
    if (uj_gemm > KL - 1) uj_gemm = KL - 1;
    const int uj = uj_int | (uj_gemm << 8);
    // geometry checks the kernel relies on (no out-of-bounds staging)
    if ((size_t)nqb * KNN_TQ > q_rows_pad || (size_t)ntiles * KNN_TC > c_rows_pad ||
        nq_pad < nqb * KNN_TQ)
        return KNN_ERR_INVALID;
    const T *qnorm = qblk + q_rows_pad * np;
    const T *cnorm = cn_ptr ? (const T *)cn_ptr : cblk + c_rows_pad * np;
    const int nqb_grid = xord ? (nqb + 7) / 8 * 8 : nqb;
    const dim3 grid((unsigned)(nqb_grid * nsplit));
    if (flags & KNN_DIST_SPLIT) {
        // split fp16 shadow rows (4 bytes a feature); m2s = -2 / S^2 undoes
        // the scaling in the epilogue's fma (a power of two: exact)
        if (!qsh || !csh) return KNN_ERR_INVALID;
        knn_split_blocks_t cb{};
        cb.nblk = 1;
        cb.sp[0] = csh;
        cb.nrm[0] = cnorm;
        cb.base[0] = (int64_t)c_base;
        cb.nc[0] = nc;
        cb.lim[0] = (int)c_rows_pad;
        return knn_launch_dist_split(dt, KL, qsh, qnorm, q_base, nq, &cb, n, meta, nsplit, part_d, part_i, part_T,
                                     nq_pad, qthr, uj, xarg, m2s, s);
    }
    // k_dist_topk<.., STG, H16> over the rows q / c (their row length `len`)
    auto launch = [&](auto stg, auto h16, const T *q, const T *c, int len) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dist_topk<T, KL, KP, decltype(stg)::value, decltype(h16)::value>), grid,
                           dim3(512), 0, s, q, qnorm, q_base, nq, c, cnorm, c_base, nc, n, len, ntiles, nsplit,
                           nqb, meta, part_d, part_i, part_T, nq_pad, (unsigned long long *)qthr, uj, xarg);
        return hip_status();
    };
    using std::integral_constant;
    if ((flags & KNN_DIST_SHADOW) && (flags & KNN_DIST_H16)) {
        if (!qsh || !csh) return KNN_ERR_INVALID;
        const int nps = (int)knn_round_up((size_t)n, 64);   // shadow row length (halves)
        // shadow rows: waves 0..3 may stage for their SIMD partners too (STG
        // 1; partial lists byte-identical)
        // Every wave stages its own rows (STG 0) for fp64 blocks (mnist 10.0
        // vs 10.1 ms); fp32 (sift) 607 vs 691 ms with waves 0..3 staging.
        return launch(integral_constant<int, sizeof(T) == 8 ? 0 : 1>(), integral_constant<int, 2>(),
                      (const T *)qsh, (const T *)csh, nps);
    }
    if (flags & KNN_DIST_H16)   // host-checked: INT mode and max|x| <= 2048 (fp64: 256)
        return launch(integral_constant<int, 0>(), integral_constant<int, 1>(), qblk, cblk, np);
    return launch(integral_constant<int, 0>(), integral_constant<int, 0>(), qblk, cblk, np);
}

// The served (element type, state capacity) pairs: fp64 k <= 16, 32 (16-deep
// lane lists); fp32 k <= 16, 32, 128.
#define KNN_DISPATCH(dtype, kp, CALL)                                          \
    do {                                                                       \
        if ((dtype) == KNN_F64 && (kp) == KNN_KP) { CALL(double, KNN_KL, KNN_KP); }       \
        else if ((dtype) == KNN_F64 && (kp) == KNN_KP_M) { CALL(double, KNN_KL, KNN_KP_M); } \
        else if ((dtype) == KNN_F32 && (kp) == KNN_KP) { CALL(float, KNN_KL, KNN_KP); }   \
        else if ((dtype) == KNN_F32 && (kp) == KNN_KP_M) { CALL(float, KNN_KL_M, KNN_KP_M); } \
        else if ((dtype) == KNN_F32 && (kp) == KNN_KP_L) { CALL(float, KNN_KL_L, KNN_KP_L); } \
        else return KNN_ERR_INVALID;                                           \
    } while (0)

extern "C" int knn_launch_dist_topk(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad,
                                    size_t q_base, int nq, const void *cblk, size_t c_rows_pad,
                                    size_t c_base, int nc, int n, const double *meta, int nsplit,
                                    double *part_d, int *part_i, double *part_T, int nq_pad,
                                    double *qthr, const void *qsh, const void *csh,
                                    const void *cn_ptr, int flags, float m2s, void *stream)
{
#define CALL(T, KL, KP)                                                                        \
    return launch_dist_topk<T, KL, KP>((const T *)qblk, q_rows_pad, q_base, nq, (const T *)cblk, \
                                       c_rows_pad, c_base, nc, n, meta, nsplit, part_d, part_i,  \
                                       part_T, nq_pad, qthr, k, qsh, csh, cn_ptr, flags, m2s,     \
                                       (hipStream_t)stream)
    KNN_DISPATCH(dtype, kp, CALL);
#undef CALL
}

// the split filter over a table of element blocks (the engine's fused GEMM
// step): the same lane-list slot of the shared bound and query norms as
// launch_dist_topk's KNN_DIST_SPLIT branch
template <typename T, int KL, int KP>
static int launch_split_n(const T *qblk, size_t q_rows_pad, size_t q_base, int nq, const void *qsp,
                          const knn_split_blocks_t *cb, int n, const double *meta, int nsplit, double *part_d,
                          int *part_i, double *part_T, int nq_pad, double *qthr, int k, int xord, float m2s,
                          hipStream_t s)
{
    constexpr int dt = sizeof(T) == 8 ? KNN_F64 : KNN_F32;
    const int np = (int)knn_n_pad_dt(n, dt);
    const int nqb = (nq + KNN_TQ - 1) / KNN_TQ;
    if (nqb <= 0 || k <= 0 || k > KP || (size_t)nqb * KNN_TQ > q_rows_pad || nq_pad < nqb * KNN_TQ || !qsp)
        return KNN_ERR_INVALID;
    int uj_int = (k + 1 + 3) / 4 - 1;
    if (uj_int > KL - 1) uj_int = KL - 1;
    const int uj = uj_int | ((KL - 1) << 8);
    return knn_launch_dist_split(dt, KL, qsp, qblk + q_rows_pad * np, q_base, nq, cb, n, meta, nsplit, part_d, part_i,
                                 part_T, nq_pad, qthr, uj, xord, m2s, s);
}

extern "C" int knn_launch_dist_split_n(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base,
                                       int nq, const void *qsp, const knn_split_blocks_t *cb, int n,
                                       const double *meta, int nsplit, double *part_d, int *part_i, double *part_T,
                                       int nq_pad, double *qthr, int xord, float m2s, void *stream)
{
#define CALL(T, KL, KP)                                                                                    \
    return launch_split_n<T, KL, KP>((const T *)qblk, q_rows_pad, q_base, nq, qsp, cb, n, meta, nsplit, part_d, \
                                     part_i, part_T, nq_pad, qthr, k, xord, m2s, (hipStream_t)stream)
    KNN_DISPATCH(dtype, kp, CALL);
#undef CALL
}

extern "C" int knn_launch_merge_n(int dtype, int kp, int k, const double *part_d, const int *part_i,
                                  const double *part_T, int nsplit, int lpq, int kl, int nq, int nq_pad,
                                  int first_step, double *st_d, double *st_x, int *st_i, double *st_T,
                                  const void *qblk, size_t q_rows_pad, const knn_merge_blocks_t *mbp, int n,
                                  const double *meta, double *qthr, int filt, const int *qperm, void *stream)
{
    if (!mbp || mbp->nblk < 1 || mbp->nblk > KNN_SPLIT_MAXBLK) return KNN_ERR_INVALID;
    const knn_merge_blocks_t mb = *mbp;
    if (lpq < 1 || kl < 1 || lpq * nsplit + 1 > 64 || k <= 0 || k > kp) return KNN_ERR_INVALID;
    const int np = (int)knn_n_pad_dt(n, dtype);
    const size_t qn_off = q_rows_pad * (size_t)np;
    // prefetched heads (KP = 32: the state as 4 runs of 8) when the lists
    // and state lanes fit; two queries a wave when they fit 32 lanes
    const int pf = kp == 32 && kl >= 8 && lpq * nsplit + 4 <= 64;
    const int two = lpq * nsplit + (pf ? 4 : 1) <= 32;
    const dim3 grid((unsigned)((nq + (two ? 7 : 3)) / (two ? 8 : 4)));
    hipStream_t s = (hipStream_t)stream;
    // k_merge<element, KP, S lanes a query, PF>: pf is the 32-entry state's own
    // form (kp == 32), two packs a query into 32 lanes
    auto launch = [&](auto te, auto kpc, auto sc, auto pfc) {
        typedef decltype(te) T;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge<T, decltype(kpc)::value, decltype(sc)::value, decltype(pfc)::value>),
                           grid, dim3(256), 0, s, part_d, part_i, part_T, nsplit, lpq, kl, nq, nq_pad, first_step,
                           st_d, st_x, st_i, st_T, (const T *)qblk, qn_off, mb, n, np, meta, k,
                           (unsigned long long *)qthr, filt, qperm);
        return hip_status();
    };
    using std::integral_constant;
    const integral_constant<int, 32> c32;
    const integral_constant<int, 64> c64;
#define CALL(T, KL, KP)                                                                    \
    if (pf && two) return launch(T(), c32, c32, integral_constant<int, 8>());              \
    if (pf) return launch(T(), c32, c64, integral_constant<int, 8>());                     \
    if (two) return launch(T(), integral_constant<int, KP>(), c32, integral_constant<int, 0>()); \
    return launch(T(), integral_constant<int, KP>(), c64, integral_constant<int, 0>())
    KNN_DISPATCH(dtype, kp, CALL);
#undef CALL
}

// f(element, KP, KL) with the rank kernels' template arguments as values:
// double or float, KNN_KP_M or KNN_KP, KNN_I8_KL_S or KNN_I8_KL
template <typename F>
static void rank_dispatch(bool f64, bool kp_m, bool kl_s, F f)
{
    auto with_kl = [&](auto te, auto kp) {
        if (kl_s) f(te, kp, std::integral_constant<int, KNN_I8_KL_S>());
        else f(te, kp, std::integral_constant<int, KNN_I8_KL>());
    };
    auto with_kp = [&](auto te) {
        if (kp_m) with_kl(te, std::integral_constant<int, KNN_KP_M>());
        else with_kl(te, std::integral_constant<int, KNN_KP>());
    };
    if (f64) with_kp(double());
    else with_kp(float());
}

extern "C" int knn_launch_merge_rank(int dtype, int kp, int kl, int k, const double *part_d, const int *part_i,
                                     const double *part_T, int nsplit, int lpq, int nq, int nq_pad,
                                     int first_step, double *st_d, double *st_x, int *st_i, double *st_T,
                                     double *qthr, knn_neighbour_t *fin_out, int *fail_count, int *fail_list,
                                     int *mode_out, double *fbound, const double *meta, int n, int force_fail,
                                     void *stream)
{
    knn_fin_args fa;
    fa.out = fin_out;
    fa.fail_count = fail_count;
    fa.fail_list = fail_list;
    fa.mode_out = mode_out;
    fa.fbound = fbound;
    fa.meta = meta;
    fa.n = n;
    fa.lim = 2251799813685248.0 / (4.0 * (double)n);
    fa.force_fail = force_fail;
    const int fin = fin_out != nullptr;
    if (lpq < 1 || nsplit < 1 || lpq * nsplit > 64 || k <= 0 || k > kp || kp > 64 || nsplit > 64 ||
        (kl != KNN_I8_KL_S && kl != KNN_I8_KL))
        return KNN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *qt = (unsigned long long *)qthr;
    if (fin && first_step && lpq * nsplit <= 16) {
        // the search's only merge (P = 1): 16 lanes a query (no state: any kp)
        const dim3 grid((unsigned)((nq + 15) / 16));
        rank_dispatch(dtype == KNN_F64, false, kl == KNN_I8_KL_S, [&](auto te, auto, auto klc) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_rank16<decltype(te), decltype(klc)::value>), grid, dim3(256),
                               0, s, part_d, part_i, part_T, nsplit, lpq, nq, nq_pad, k, qt, fa);
        });
        return hip_status();
    }
    if ((dtype != KNN_F64 && dtype != KNN_F32) || (kp != KNN_KP && kp != KNN_KP_M)) return KNN_ERR_INVALID;
    const int cap = (lpq * nsplit * kl + kp + 1) & ~1;   // every candidate; 16-byte rows
    const size_t lds = 4 * (size_t)cap * sizeof(unsigned long long);
    const dim3 grid((unsigned)((nq + 3) / 4));
    rank_dispatch(dtype == KNN_F64, kp == KNN_KP_M, kl == KNN_I8_KL_S, [&](auto te, auto kpc, auto klc) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_rank<decltype(te), decltype(kpc)::value, decltype(klc)::value>),
                           grid, dim3(256), lds, s, part_d, part_i, part_T, nsplit, lpq, nq, nq_pad, first_step,
                           st_d, st_x, st_i, st_T, k, qt, cap, fin, fa);
    });
    return hip_status();
}

extern "C" int knn_launch_finalize(int dtype, int kp, const double *st_d, const double *st_x,
                                   const int *st_i, const double *st_T, const void *qblk,
                                   size_t q_rows_pad, int nq, int n, int k, const double *meta,
                                   knn_neighbour_t *out, int *fail_count, int *fail_list,
                                   int *mode_out, double *fbound, int force_fail, int filt, void *stream)
{
    if (k <= 0 || k > kp) return KNN_ERR_INVALID;
    const size_t off = q_rows_pad * knn_n_pad_dt(n, dtype);
    const dim3 grid((unsigned)((nq + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
#define CALL(T, KL, KP)                                                                        \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_finalize<T, KP>), grid, dim3(256), 0, s, st_d, st_x,   \
                       st_i, st_T, qblk ? (const T *)qblk + off : nullptr, nq, n, k, meta, out,  \
                       fail_count,                                                               \
                       fail_list, mode_out, fbound, force_fail, filt);                           \
    return hip_status()
    KNN_DISPATCH(dtype, kp, CALL);
#undef CALL
}

extern "C" int knn_launch_rescan_init(int kp, double *rs_d, int *rs_i, int nfail, void *stream)
{
    const int cnt = nfail * kp;
    if (cnt <= 0) return KNN_OK;
    hipLaunchKernelGGL(k_rescan_init, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, rs_d, rs_i, cnt);
    return hip_status();
}

extern "C" int knn_launch_rescan_step(int dtype, int kp, const int *fail_list, int nfail,
                                      const double *fbound, const void *qblk, const void *cblk,
                                      size_t c_base, int nc, int n, int k, double *rs_d,
                                      int *rs_i, long long self_base, void *stream)
{
    if (nfail <= 0) return KNN_OK;
    if (k <= 0 || k > kp || nc <= 0) return KNN_ERR_INVALID;
    const int np = (int)knn_n_pad_dt(n, dtype);
    hipStream_t s = (hipStream_t)stream;
    // Few uncertified queries give few workgroups (16 queries each): split
    // the block's rows over C chunks too (knn_rescan_chunks; the caller
    // sized rs_d/rs_i for 1 + C list sets), then merge the chunk lists.
    int C = knn_rescan_chunks(nfail);
    const int min_rows = 256;
    if (C > (nc + min_rows - 1) / min_rows) C = (nc + min_rows - 1) / min_rows;
    if (C < 1) C = 1;
    const int rpc = (nc + C - 1) / C;
    C = (nc + rpc - 1) / rpc;
    const size_t stride = (size_t)nfail * kp;
    if (C > 1) {
        hipLaunchKernelGGL(k_rescan_init, dim3((unsigned)((C * stride + 255) / 256)), dim3(256), 0, s,
                           rs_d + stride, rs_i + stride, (int)(C * stride));
    }
    double *ld = C > 1 ? rs_d + stride : rs_d;
    int *li = C > 1 ? rs_i + stride : rs_i;
#define CALL(T, KL, KP)                                                                          \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rescan_step<T, KP>),                                    \
                       dim3((unsigned)((nfail + 15) / 16), (unsigned)C), dim3(256), 0, s,         \
                       fail_list, nfail, fbound, (const T *)qblk, np, (const T *)cblk, c_base, nc, \
                       n, np, k, rs_d, ld, li, rpc, C > 1 ? stride : 0, self_base);               \
    if (C > 1)                                                                                   \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rescan_merge<KP>), dim3((unsigned)((nfail + 3) / 4)), \
                           dim3(256), 0, s, nfail, k, C, rs_d, rs_i);                            \
    return hip_status()
    KNN_DISPATCH(dtype, kp, CALL);
#undef CALL
}

extern "C" int knn_launch_rescan_end(int kp, const int *fail_list, int nfail, const double *rs_d,
                                     const int *rs_i, int k, knn_neighbour_t *out, void *stream)
{
    const int cnt = nfail * k;
    if (cnt <= 0) return KNN_OK;
    hipLaunchKernelGGL(k_rescan_end, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, fail_list, nfail, kp, rs_d, rs_i, k, out);
    return hip_status();
}

// ---------------------------------------------------------------------------
// k_vote: the label vote + accuracy stage on the device (knn_classify_device;
// host twin knn_vote.c, same rules).  One wave per query: the k neighbour
// labels are counted into the wave's LDS histogram (nclasses <= 1024), lane
// 0 walks the classes in label order exactly like serial:121-124 /
// blk:263-266 (SERIAL / MPI, with their count-vs-label quirk) or
// takes a true majority (MAJORITY), then compares with the query's own
// label (serial:126-127).  The neighbour records get their .label filled
// (blk:176).  Empty slots and idx > nlabels are skipped.
// ---------------------------------------------------------------------------
// What k_vote and k_vote_index share.  vote_fill: the wave's lanes stride over
// query L's k records, write each one's .label and count it into the wave's
// histogram c, which every lane may read on return.  vote_pick: one lane's walk
// over that histogram, knn_vote.c's to the letter.
__device__ __forceinline__ void vote_fill(knn_neighbour_t *L, int k, int lane, int *c, int nclasses,
                                          const double *__restrict__ labels, long long nlabels)
{
    for (int i = lane; i < k; i += 64) {
        const int id = L[i].idx;
        int lab = 0;
        if (id > 0 && id <= nlabels) {
            lab = (int)labels[id - 1];
            L[i].label = lab;
            if (lab >= 1 && lab <= nclasses) atomicAdd(&c[lab - 1], 1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int vote_pick(const knn_neighbour_t *L, int k, const int *c, int nclasses, int rule,
                                         const double *__restrict__ labels, long long nlabels)
{
    int most = 0;
    if (rule == KNN_VOTE_MAJORITY) {
        int best = 0;
        for (int j = 0; j < nclasses; j++) best = c[j] > best ? c[j] : best;
        for (int i = 0; i < k && best > 0; i++) {
            const int id = L[i].idx;
            if (id <= 0 || id > nlabels) continue;
            const int lab = (int)labels[id - 1];
            if (lab >= 1 && lab <= nclasses && c[lab - 1] == best) {
                most = lab;
                break;
            }
        }
    } else {
        const int id0 = L[0].idx;
        const int nn0 = (id0 > 0 && id0 <= nlabels) ? (int)labels[id0 - 1] : 0;
        const int tie = rule == KNN_VOTE_MPI ? nn0 - 1 : nn0;
        for (int j = 0; j < nclasses; j++)
            if (c[j] > most || (c[j] == most && (j + 1) == tie)) most = j + 1;
    }
    return most;
}

__global__ __launch_bounds__(256) void k_vote(knn_neighbour_t *__restrict__ nb, int m, int k,
                                              int nclasses, int rule,
                                              const double *__restrict__ labels,
                                              long long nlabels, long long q_base,
                                              int *__restrict__ pred,
                                              unsigned long long *__restrict__ matches)
{
    __shared__ int cls[4][KNN_VOTE_MAX_CLASSES];
    __shared__ unsigned hits[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    int *c = cls[wave];
    for (int j = lane; j < nclasses; j += 64) c[j] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    unsigned hit = 0;
    if (q < m) {
        knn_neighbour_t *L = nb + (size_t)q * k;
        vote_fill(L, k, lane, c, nclasses, labels, nlabels);
        if (lane == 0) {
            const int most = vote_pick(L, k, c, nclasses, rule, labels, nlabels);
            if (pred) pred[q] = most;
            const long long g = q_base + q;
            hit = (g < nlabels && (double)most == labels[g]) ? 1u : 0u;
        }
    }
    if (lane == 0) hits[wave] = hit;
    __syncthreads();
    if (threadIdx.x == 0 && matches) {
        const unsigned h = hits[0] + hits[1] + hits[2] + hits[3];
        if (h) atomicAdd(matches, (unsigned long long)h);
    }
}

extern "C" int knn_launch_vote(knn_neighbour_t *nb, size_t m, int k, int nclasses, int rule,
                               const double *labels, size_t nlabels, size_t q_base, int *pred,
                               unsigned long long *matches, void *stream)
{
    if (m == 0) return KNN_OK;
    if (nclasses > KNN_VOTE_MAX_CLASSES || m > 0x7fffffffULL) return KNN_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (matches && hipMemsetAsync(matches, 0, sizeof(unsigned long long), s) != hipSuccess)
        return KNN_ERR_HIP;
    hipLaunchKernelGGL(k_vote, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, nb, (int)m, k,
                       nclasses, rule, labels, (long long)nlabels, (long long)q_base, pred, matches);
    return hip_status();
}

// ---------------------------------------------------------------------------
// k_vote_index: the vote of knn_index_classify / knn_index_classify_rows, on
// the records behind the id remap.  k_vote's layout (one wave a query, four
// queries a workgroup, the wave's LDS histogram, lanes striding over k) and its
// fill and walk; what differs is where a query's own label comes from -- qlab[q]
// (the batch's labels, uploaded), or labels[id - 1] of the resident row it is,
// id = own_ids[q] (NULL: q + 1, every row of an index that removed nothing), or
// nowhere (matches == NULL) -- and counts (nullable): the histogram itself,
// nclasses ints a query, stored behind the wave's barrier.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vote_index(knn_neighbour_t *__restrict__ nb, int m, int k, int nclasses,
                                                    int rule, const double *__restrict__ labels, long long nlabels,
                                                    const double *__restrict__ qlab,
                                                    const int *__restrict__ own_ids, int *__restrict__ pred,
                                                    int *__restrict__ counts,
                                                    unsigned long long *__restrict__ matches)
{
    __shared__ int cls[4][KNN_VOTE_MAX_CLASSES];
    __shared__ unsigned hits[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    int *c = cls[wave];
    for (int j = lane; j < nclasses; j += 64) c[j] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    unsigned hit = 0;
    if (q < m) {
        knn_neighbour_t *L = nb + (size_t)q * k;
        vote_fill(L, k, lane, c, nclasses, labels, nlabels);
        if (counts)
            for (int j = lane; j < nclasses; j += 64) counts[(size_t)q * nclasses + j] = c[j];
        if (lane == 0) {
            const int most = vote_pick(L, k, c, nclasses, rule, labels, nlabels);
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

extern "C" int knn_launch_vote_index(knn_neighbour_t *nb, size_t mq, int k, int nclasses, int rule,
                                     const double *labels, size_t nlabels, const double *qlab,
                                     const int32_t *own_ids, int *pred, int *counts, unsigned long long *matches,
                                     void *stream)
{
    if (mq == 0) return KNN_OK;
    if (k <= 0 || nclasses <= 0 || !pred) return KNN_ERR_INVALID;
    if (nclasses > KNN_VOTE_MAX_CLASSES || mq > 0x7fffffffULL) return KNN_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (matches && hipMemsetAsync(matches, 0, sizeof(unsigned long long), s) != hipSuccess) return KNN_ERR_HIP;
    hipLaunchKernelGGL(k_vote_index, dim3((unsigned)((mq + 3) / 4)), dim3(256), 0, s, nb, (int)mq, k, nclasses, rule,
                       labels, (long long)nlabels, qlab, own_ids, pred, counts, matches);
    return hip_status();
}

// k_remap_idx: the records of an index that removed rows (knn_index_remove)
// carry internal positions; ids[] (ascending, one a live row) gives each its
// external id.  Empty slots (idx 0) stay {inf, 0, 0}.
__global__ __launch_bounds__(256) void k_remap_idx(knn_neighbour_t *__restrict__ nb, size_t cnt,
                                                   const int *__restrict__ ids, int nids)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    const int idx = nb[i].idx;
    nb[i].idx = idx > 0 && idx <= nids ? ids[idx - 1] : 0;
}

extern "C" int knn_launch_remap_idx(knn_neighbour_t *nb, size_t cnt, const int32_t *ids, size_t nids, void *stream)
{
    if (cnt == 0) return KNN_OK;
    if (nids > 0x7fffffffULL || (cnt + 255) / 256 > 0x7fffffffULL) return KNN_ERR_INVALID;
    hipLaunchKernelGGL(k_remap_idx, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nb, cnt,
                       ids, (int)nids);
    return hip_status();
}

// k_drop_self: knn_index_neighbours under the keep-zero rule.  The queries
// are corpus rows searched with ids past the corpus, so a query meets its own
// row as a candidate at distance 0; it was searched at k + 1.  Records come
// ordered by (distance, idx), so either the own row (idx == pos[q] + 1) is
// among the k + 1 -- without it they are the k nearest others -- or all k + 1
// are duplicates at distance 0 with lower idx, and the first k are the answer.
// A wave a query, a 16-byte record a lane, k + 1 records in passes of 64: a
// ballot finds the own row, the records behind it move up by one.  idx goes
// through ids[] as in k_remap_idx (ids == NULL: kept); empty slots stay
// {inf, 0, 0}.
typedef unsigned knn_rec4u __attribute__((ext_vector_type(4)));   // {distance lo, hi, idx, label}
__global__ __launch_bounds__(256) void k_drop_self(knn_rec4u *__restrict__ out, const knn_rec4u *__restrict__ in,
                                                   const int *__restrict__ pos, size_t nq, int k,
                                                   const int *__restrict__ ids, int nids)
{
    static_assert(sizeof(knn_neighbour_t) == sizeof(knn_rec4u), "a record is one 16-byte vector");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (size_t q = (size_t)blockIdx.x * 4 + wave; q < nq; q += (size_t)gridDim.x * 4) {
        const knn_rec4u *r = in + q * ((size_t)k + 1);
        knn_rec4u *o = out + q * (size_t)k;
        const int self = pos[q] + 1;
        int s = -1;   // the own row's record, once met (wave-uniform)
        for (int e0 = 0; e0 <= k; e0 += 64) {
            const int e = e0 + lane;
            knn_rec4u v = {0u, 0u, 0u, 0u};
            if (e <= k) v = r[e];
            const unsigned long long hit = __ballot(e <= k && (int)v[2] == self);
            if (s < 0 && hit) s = e0 + (int)__ffsll((long long)hit) - 1;
            const int w = (s >= 0 && e > s) ? e - 1 : e;   // where record e goes
            if (e > k || e == s || w >= k) continue;
            const int idx = (int)v[2];
            if (ids != nullptr) v[2] = (unsigned)(idx > 0 && idx <= nids ? ids[idx - 1] : 0);
            o[w] = v;
        }
    }
}

extern "C" int knn_launch_drop_self(knn_neighbour_t *out, const knn_neighbour_t *in, const int32_t *pos, size_t nq,
                                    int k, const int32_t *ids, size_t nids, void *stream)
{
    if (nq == 0) return KNN_OK;
    if (k <= 0 || nids > 0x7fffffffULL) return KNN_ERR_INVALID;
    const unsigned grid = (unsigned)((nq + 3) / 4 < 16384 ? (nq + 3) / 4 : 16384);
    hipLaunchKernelGGL(k_drop_self, dim3(grid), dim3(256), 0, (hipStream_t)stream, (knn_rec4u *)out,
                       (const knn_rec4u *)in, pos, nq, k, ids, (int)nids);
    return hip_status();
}
