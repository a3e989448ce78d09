/*
 * knn_internal.h -- launchers exported by the kernel units (knn_pack.hip,
 * knn_kernels.hip, knn_i8.hip, knn_split.hip, knn_order.hip) to the host C
 * engine (knn_engine.c, knn_index.c).  Plain C ABI, device pointers, hipStream_t as void*.
 */
#ifndef KNN_INTERNAL_H
#define KNN_INTERNAL_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tile geometry shared by host and device. */
#define KNN_TQ 128        /* queries per workgroup (8 waves x 16)      */
#define KNN_TC 128        /* corpus rows per tile                      */
#define KNN_BK 16         /* fp64 features per LDS chunk (128 B a row) */
#define KNN_KL 16         /* per-lane candidate list capacity, k <= 32 */
#define KNN_KP 32         /* per-query state / selection capacity      */
#define KNN_KL_M 24       /* fp32, 16 < k <= 32: a lane list overflows */
#define KNN_KP_M 64       /*   when > KL of the k fall in its quarter   */
#define KNN_KL_L 40       /* fp32, 32 < k <= 128:                        */
#define KNN_KP_L 128      /*   P(Bin(100, 1/4) > 40) ~ 3e-4 per lane   */
#define KNN_ROW_ALIGN 128 /* packed-block row padding                  */

/* meta doubles of a packed block */
#define KNN_META_MAXABS    0
#define KNN_META_MAXNORM   1
#define KNN_META_NONINT    2
#define KNN_META_NONFINITE 3
#define KNN_META_MAXPOS    4   /* max(x, 0)  */
#define KNN_META_MAXNEG    5   /* max(-x, 0) */
#define KNN_META_S8        7   /* 1: a speculative byte block (knn_block_pack_s8); MAX-reduced, so a
                                * ring knows whether any rank packed one */

/* engine modes (decided on device from the reduced meta) */
#define KNN_MODE_INT  0   /* integer data: GEMM-form d^2 is exact         */
#define KNN_MODE_GEMM 1   /* fp64 GEMM-form filter + exact re-rank        */
#define KNN_MODE_SCAN 2   /* non-finite / huge data: exact scan only      */

static inline size_t knn_round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline size_t knn_rows_pad(size_t rows) { return knn_round_up(rows ? rows : 1, KNN_ROW_ALIGN); }
static inline size_t knn_n_pad(size_t n) { return knn_round_up(n ? n : 1, KNN_BK); }
/* element size and padded row length of a packed block of `dtype`
 * (KNN_F64 / KNN_F32): rows are padded to whole 128-byte chunks */
/* state capacity and per-lane list length serving k */
/* State capacity serving k.  With one corpus split, 16-deep lane lists
 * overflow for P(Bin(32, 1/4) >= 16) * 4 = 0.8% of queries at k = 32 (each
 * a rescan); fp32 has the registers for deeper lists, fp64 (k <= 32) not.
 * fp64 16 < k <= 32 keeps 16-deep lane lists but a 64-entry state: the
 * GEMM certificate's Td (the smallest value a merge drops) then sits past
 * the (k + 1)-th candidate's near ties -- with a 32-entry state at k = 30,
 * 228 of the 60000 real-valued MNIST-shape queries had their 33rd filter
 * value within 2E of the 30th and took the exact rescan. */
static inline int knn_kp_for(int k, int dtype)
{
    if (k <= 16) return KNN_KP;
    if (dtype != KNN_F32) return KNN_KP_M;
    return k <= 32 ? KNN_KP_M : KNN_KP_L;
}
static inline int knn_kl_for(int kp, int dtype)
{
    if (dtype != KNN_F32) return KNN_KL;
    return kp == KNN_KP ? KNN_KL : kp == KNN_KP_M ? KNN_KL_M : KNN_KL_L;
}
/* Corpus chunks of one exact rescan launch (k_rescan_step's grid.y): enough
 * that (nfail / 16) x C workgroups fill the chip, at most 32.  The rescan
 * list buffers hold 1 + C list sets (the running one, then one per chunk). */
static inline int knn_rescan_chunks(int nfail)
{
    const int wg = (nfail + 15) / 16;
    int c = wg > 0 ? (1024 + wg - 1) / wg : 1;
    return c > 32 ? 32 : (c < 1 ? 1 : c);
}
static inline size_t knn_esize(int dtype) { return dtype == KNN_F32 ? 4 : 8; }

/* Byte block (knn_i8.hip): the int8 form of a packed block for the int8
 * MFMA contraction of 8-bit-window integer data.  Rows of knn_s8_rs(n)
 * bytes (x - o, o = 128 - meta[MAXNEG]; 0 past n), then two int32 words per
 * row, each array in the per-tile order of i8_norm_pos: the slot/parity
 * words (i8_norm_word), then the accumulator init words (i8_init_word,
 * -floor(|x - o|^2 / 2)); then the block's 8 meta doubles. */
#define KNN_I8_MAX_N 896  /* 7 chunks of 128 features: queries stay in VGPRs */
#define KNN_I8_KL_S 12    /* per-lane list, k <= 32: 8-wave kernel, 4 lists a query  */
                          /* (4 KL >= k + 1: the 4-lane bound; no 2-lane bound)     */
#define KNN_I8_KL   17    /* the same with 17-entry lists (KNN_I8_KL=17)             */
#define KNN_I8_KL_L 65    /* k <= 128: 4-wave kernel, 2 lists a query (2 KL > k)    */
/* row bytes: whole K-steps of 32 */
static inline size_t knn_s8_rs(size_t n) { return knn_round_up(n ? n : 1, 32); }
static inline size_t knn_s8_norm_offset(size_t cap, size_t n) { return knn_rows_pad(cap) * knn_s8_rs(n); }
static inline size_t knn_s8_meta_offset(size_t cap, size_t n) { return knn_s8_norm_offset(cap, n) + knn_rows_pad(cap) * 8; }
static inline size_t knn_s8_bytes(size_t cap, size_t n)
{
    return knn_round_up(knn_s8_meta_offset(cap, n) + 8 * sizeof(double), 16);
}
/* Corpus blocks of one k_dist_topk_i8 launch (a fused ring step): byte
 * blocks of one capacity, ascending global base (so every lane meets its
 * candidates in increasing row order: the stable tie rule), block b holding
 * global tiles [t0[b], t0[b+1]) of the launch.  An entry may also be a
 * whole-tile range of a block: ptr / nptr / base advanced by its first tile. */
#define KNN_I8_MAXBLK 8
typedef struct {
    const void *ptr[KNN_I8_MAXBLK];   /* row 0 of the block (or of a tile range of it) */
    const void *nptr[KNN_I8_MAXBLK];  /* its norms; NULL: the block's, ptr + cap_pad * row bytes */
    int64_t base[KNN_I8_MAXBLK];
    int nc[KNN_I8_MAXBLK];
    int t0[KNN_I8_MAXBLK + 1];
    int nblk;
} knn_i8_blocks_t;
static inline int knn_i8_kl(int kp) { return kp <= KNN_KP_M ? KNN_I8_KL_S : KNN_I8_KL_L; }
/* lists per query: 2 for the 65-entry lists (k > 32) and for the 12-entry
 * lists on 64-row half tiles (the k <= 32 default); 4 for the 8-wave
 * kernel on 128-row tiles (17-entry lists) */
static inline int knn_i8_lpq(int kp, int kl) { return kp <= KNN_KP_M && kl != KNN_I8_KL_S ? 4 : 2; }
/* query groups a wave of the int8 kernel: 2 for the half-tile kernel on
 * rows of <= 4 K-steps (SIFT's n = 128: a workgroup of 256 queries, A
 * fragments and init words shared by both groups), else 1
 * (KNN_I8_QG1=1 forces 1).  A workgroup covers 128 qg queries. */
static inline int knn_i8_qg(int kl, int lpq, size_t n)
{
    const char *e = getenv("KNN_I8_QG1");
    return kl == KNN_I8_KL_S && lpq == 2 && knn_s8_rs(n) / 32 <= 4 && !(e && *e && *e != '0') ? 2 : 1;
}
static inline size_t knn_n_pad_dt(size_t n, int dtype)
{
    return knn_round_up(n ? n : 1, 128 / knn_esize(dtype));
}

/* Launchers.  dtype = element type of the packed blocks (KNN_F64 /
 * KNN_F32); block pointers are untyped device pointers. */
int knn_launch_pack(void *blk, int dtype, size_t cap, size_t rows, size_t n, const void *src,
                    int src_dtype, size_t ld, int layout, void *stream);
int knn_launch_dist_topk(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                         const void *cblk, size_t c_rows_pad, size_t c_base, int nc,
                         int n, const double *meta, int nsplit,
                         double *part_d, int *part_i, double *part_T, int nq_pad,
                         double *qthr, const void *qsh, const void *csh, const void *cn_ptr,
                         int flags, float m2s, void *stream);
/* knn_launch_dist_topk flags */
#define KNN_DIST_XORD   1  /* XCD-grouped workgroup order                        */
#define KNN_DIST_H16    2  /* fp16 MFMA contraction (exact data only)             */
#define KNN_DIST_SHADOW 4  /* with H16: stage the fp16 shadow rows qsh / csh      */
#define KNN_DIST_SPLIT  8  /* fp32 blocks: split fp16 filter on the split shadow rows
                              qsh / csh (knn_launch_shadow_split); m2s = -2 / S^2   */
#define KNN_DIST_KEEP0 16  /* the keep-zero rule (knn_ctx_set_keep_zero)               */
/* The keep-zero rule reaches the kernels inside an int argument they already
 * take, so a search with the rule off launches with exactly the arguments it
 * always had: bit 1 of `xord` (k_dist_topk, k_dist_split; knn_launch_dist_split
 * and _split_n take the argument as is), bit 1 of `filt` (k_merge, k_finalize),
 * bit 17 of `uj` (k_dist_topk_i8).  k_rescan_step takes self_base: -1, or the
 * search's q_base when zeros are kept (the query's own row is then left out
 * by id, as the distance kernels do, not by its zero distance). */
#define KNN_KARG_KEEP0 2
#define KNN_I8_UJ_KEEP0 (1 << 17)
/* k_dist_split (knn_split.hip): the split fp16 filter on 256-row tiles,
 * over up to KNN_SPLIT_MAXBLK corpus blocks in one launch (block b: split
 * rows sp[b], norms nrm[b] of its element block, global ids base[b].., nc[b]
 * rows, lim[b] rows allocated; tiles [t0[b], t0[b+1]) of the launch -- the
 * launcher fills t0) */
#define KNN_SPLIT_TC 256
#define KNN_SPLIT_MAXBLK 8
typedef struct {
    const void *sp[KNN_SPLIT_MAXBLK];
    const void *nrm[KNN_SPLIT_MAXBLK];
    int64_t base[KNN_SPLIT_MAXBLK];
    int nc[KNN_SPLIT_MAXBLK];
    int lim[KNN_SPLIT_MAXBLK];
    int t0[KNN_SPLIT_MAXBLK + 1];
    int nblk;
} knn_split_blocks_t;
/* the element blocks a GEMM-mode merge re-ranks from (k_merge's exact S):
 * block j holds global ids base[j] .. base[j] + nc[j] - 1 (one entry: a
 * single-block step) */
typedef struct {
    const void *ptr[KNN_SPLIT_MAXBLK];
    int64_t base[KNN_SPLIT_MAXBLK];
    int nc[KNN_SPLIT_MAXBLK];
    int nblk;
} knn_merge_blocks_t;
int knn_launch_merge_n(int dtype, int kp, int k, const double *part_d, const int *part_i, const double *part_T,
                       int nsplit, int lpq, int kl, int nq, int nq_pad, int first_step, double *st_d, double *st_x,
                       int *st_i, double *st_T, const void *qblk, size_t q_rows_pad, const knn_merge_blocks_t *mb,
                       int n, const double *meta, double *qthr, int filt, const int *qperm, void *stream);
/* the split filter over several element blocks (their split rows in sp[],
 * their norms in nrm[]): knn_launch_dist_topk's KNN_DIST_SPLIT for a table */
int knn_launch_dist_split_n(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                            const void *qsp, const knn_split_blocks_t *cb, int n, const double *meta, int nsplit,
                            double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr, int xord,
                            float m2s, void *stream);
int knn_launch_dist_split(int dtype, int kl, const void *qsp, const void *qnorm, size_t q_base, int nq,
                          const knn_split_blocks_t *cb, int n, const double *meta, int nsplit, double *part_d,
                          int *part_i, double *part_T, int nq_pad, double *qthr, int uj, int xord, float m2s,
                          void *stream);
/* fp16 shadow rows (round_up(n, 64) halves a row) of a packed block */
int knn_launch_shadow(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, void *stream);
int knn_launch_fill_inf(double *p, int count, void *stream);
/* int8 re-search of uncertified queries (knn_i8.hip) */
int knn_launch_gather8(void *dst, const void *src, const int *list, int cnt, size_t n, size_t src_rows_pad,
                       size_t dst_rows_pad, const double *src_qthr, double *dst_qthr, void *stream);
int knn_launch_resolve8(unsigned char *flag, const int *list, int cnt, const int *sub_fail, const int *sub_cnt,
                        const knn_neighbour_t *sub_out, int k, knn_neighbour_t *out, int *new_list, int *new_cnt,
                        void *stream);
/* speculative byte block straight from the source (knn_block_pack_s8) */
int knn_launch_pack_s8(void *dst, int dtype, size_t cap, size_t rows, size_t n, const void *src, int src_dtype,
                       size_t ld, int layout, void *stream);
/* rows row0 .. row0 + rows - 1 of a block / byte block packed before, from a
 * rows x n source (knn_block_append_dt / knn_block_append_s8): no meta memset,
 * grids over `rows` */
int knn_launch_append(void *blk, int dtype, size_t cap, size_t row0, size_t rows, size_t n, const void *src,
                      int src_dtype, size_t ld, int layout, void *stream);
int knn_launch_append_s8(void *dst, int dtype, size_t cap, size_t row0, size_t rows, size_t n, const void *src,
                         int src_dtype, size_t ld, int layout, void *stream);
/* listed rows of a block / byte block packed before (knn_block_scatter_dt /
 * knn_block_scatter_s8): item i < rows reads row srow[i] (NULL: i) of a
 * src_rows-row source and writes block row pos[i] (device lists); otherwise an
 * append: no meta memset, grids over `rows` */
int knn_launch_scatter(void *blk, int dtype, size_t cap, const int32_t *pos, const int32_t *srow, size_t rows,
                       size_t n, const void *src, size_t src_rows, int src_dtype, size_t ld, int layout, void *stream);
int knn_launch_scatter_s8(void *dst, int dtype, size_t cap, const int32_t *pos, const int32_t *srow, size_t rows,
                          size_t n, const void *src, size_t src_rows, int src_dtype, size_t ld, int layout,
                          void *stream);
/* knn_pack.hip: block row row0 + i of dst <- row list[i] of src, i < rows
 * (knn_block_gather_dt / knn_block_gather_s8): element rows and norms bit for
 * bit; byte rows verbatim, their norm words made again for the new row.  Only
 * those rows are written; grids over `rows` */
int knn_launch_gather(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap, const int32_t *list,
                      size_t rows, size_t n, int dtype, void *stream);
int knn_launch_gather_rows8(void *dst, size_t dst_cap, size_t row0, const void *src, size_t src_cap,
                            const int32_t *list, size_t rows, size_t n, void *stream);
/* the same from a corpus held as nblk blocks of capacity src_cap (tab: their
 * pointers, a device array): block row row0 + i of dst <- the row at global
 * position pos[i] (knn_block_gather_pos_dt / knn_block_gather_pos_s8); a
 * position outside [0, nblk * src_cap) writes nothing */
int knn_launch_gather_pos(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap, size_t nblk,
                          const int32_t *pos, size_t rows, size_t n, int dtype, void *stream);
int knn_launch_gather_pos8(void *dst, size_t dst_cap, size_t row0, const void *const *tab, size_t src_cap,
                           size_t nblk, const int32_t *pos, size_t rows, size_t n, void *stream);
/* knn_kernels.hip: knn_index_neighbours under the keep-zero rule.  Query q's
 * k + 1 records at in + q (k + 1) -> its k records at out + q k: the first
 * record whose idx is pos[q] + 1 (the query's own row) left out, else the
 * last; idx through ids[] (nids entries; NULL: kept) as knn_launch_remap_idx */
int knn_launch_drop_self(knn_neighbour_t *out, const knn_neighbour_t *in, const int32_t *pos, size_t nq, int k,
                         const int32_t *ids, size_t nids, void *stream);
/* knn_kernels.hip: the records' idx from internal position to external id
 * (knn_index_query of an index that removed rows): idx = ids[idx - 1], empty
 * slots (idx 0) kept */
int knn_launch_remap_idx(knn_neighbour_t *nb, size_t cnt, const int32_t *ids, size_t nids, void *stream);
/* INT-mode merge of int8 lane lists (kl = KNN_I8_KL_S / KNN_I8_KL, kp <= 64)
 * by ranking the candidates at or below the shared bound (k_merge_rank) */
int knn_launch_merge_rank(int dtype, int kp, int kl, int k, const double *part_d, const int *part_i,
                          const double *part_T, int nsplit, int lpq, int nq, int nq_pad, int first_step,
                          double *st_d, double *st_x, int *st_i, double *st_T, double *qthr,
                          knn_neighbour_t *fin_out, int *fail_count, int *fail_list, int *mode_out, double *fbound,
                          const double *meta, int n, int force_fail, void *stream);
/* qthr = +inf, qsum (may be NULL) = empty summaries, counts[0..1] = 0 */
int knn_launch_begin_init(double *qthr, unsigned long long *qsum, int nq_pad, int *counts, void *stream);
/* counts[0..1] -> mapped host memory, and the meta (8 doubles; NULL: none)
 * -> mapped_meta (k_count_out) */
int knn_launch_count_out(const int *d_count, int *mapped, const double *meta, double *mapped_meta, void *stream);
/* split fp16 shadow rows of an fp32 / fp64 block: per 32 features 32 halves hi =
 * RN16(S x), then 32 halves lo = RN16(S x - hi); rows of round_up(n, 32) * 4
 * bytes; S a power of two (knn_engine.c: maxabs S in [2^13, 2^14)) */
static inline size_t knn_split_rs(size_t n) { return knn_round_up(n ? n : 1, 32) * 4; }
int knn_launch_shadow_split(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, float S,
                            void *stream);
/* the same for nblk <= KNN_SPLIT_MAXBLK blocks in one launch */
int knn_launch_shadow_split_n(int nblk, void *const *dst, const void *const *src, const size_t *rows_pad,
                              int dtype, size_t n, float S, void *stream);
/* knn_i8.hip: element block -> byte block (meta = the reduced meta) and the
 * int8 distance + top-k kernel (partial lists [split][query][2][kl]) */
int knn_launch_shadow8(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n,
                       const double *meta, void *stream);
int knn_launch_dist_i8(int kp, int kl, int lpq, int k, const void *qsh, size_t q_rows_pad, size_t q_base, int nq,
                       const knn_i8_blocks_t *cb, size_t c_rows_pad, int n, int nsplit,
                       double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr,
                       unsigned long long *qsum, int keep_zero, void *stream);
/* knn_order.hip: a query order for the GEMM-mode merge (queries grouped by
 * the clusters their list heads connect) */
size_t knn_order_tmp_bytes(int nq);
int knn_launch_order(const int *part_i, int nsplit, int lpq, int kl, int nq, int nq_pad, long long q_base,
                     int rounds, int *lab, int *keys, int *iota, int *perm, void *tmp, size_t tmp_bytes,
                     void *stream);
int knn_launch_finalize(int dtype, int kp, const double *st_d, const double *st_x, const int *st_i,
                        const double *st_T, const void *qblk, size_t q_rows_pad,
                        int nq, int n, int k, const double *meta,
                        knn_neighbour_t *out, int *fail_count, int *fail_list,
                        int *mode_out, double *fbound, int force_fail, int filt, void *stream);
int knn_launch_rescan_init(int kp, double *rs_d, int *rs_i, int nfail, void *stream);
int knn_launch_rescan_step(int dtype, int kp, const int *fail_list, int nfail,
                           const double *fbound, const void *qblk, const void *cblk,
                           size_t c_base, int nc, int n, int k, double *rs_d, int *rs_i,
                           long long self_base, void *stream);
int knn_launch_rescan_end(int kp, const int *fail_list, int nfail, const double *rs_d,
                          const int *rs_i, int k, knn_neighbour_t *out, void *stream);
int knn_launch_vote(knn_neighbour_t *nb, size_t m, int k, int nclasses, int rule,
                    const double *labels, size_t nlabels, size_t q_base, int *pred,
                    unsigned long long *matches, void *stream);
/* knn_kernels.hip: the vote of knn_index_classify / knn_index_classify_rows
 * (k_vote_index) over mq x k records whose idx are ids into labels (nlabels of
 * them, by id).  A query's own label: qlab[q] (device, nullable), else
 * labels[own_ids[q] - 1] (own_ids NULL: labels[q]); read only when matches
 * (nullable, one device counter, zeroed here) is given.  pred: mq ints; counts
 * (nullable): mq x nclasses ints, each query's histogram; .label is filled */
int knn_launch_vote_index(knn_neighbour_t *nb, size_t mq, int k, int nclasses, int rule, const double *labels,
                          size_t nlabels, const double *qlab, const int32_t *own_ids, int *pred, int *counts,
                          unsigned long long *matches, void *stream);
/* knn_predict.hip: the weighted vote and the regression of the
 * knn_index_classify_weighted / knn_index_regress calls (k_predict_classify,
 * k_predict_regress; host twins knn_classify_weighted / knn_regress, bit for
 * bit) over the same records, with k_vote_index's arguments.  weights: enum
 * knn_weights.  nclasses > 0: pred is mq ints, sums (nullable) mq x nclasses
 * doubles, .label is filled.  nclasses == 0: regression -- pred is mq doubles,
 * labels are the targets, sums, qlab, own_ids and matches are not read and
 * .label stays */
int knn_launch_predict(knn_neighbour_t *nb, size_t mq, int k, int nclasses, int weights, const double *labels,
                       size_t nlabels, const double *qlab, const int32_t *own_ids, void *pred, double *sums,
                       unsigned long long *matches, void *stream);
/* knn_radius.hip: radius search over the resident index (knn_index_radius*).
 * The corpus blocks of one launch: block b holds the rows at global positions
 * base[b] .. base[b] + nc[b] - 1 (byte blocks for knn_launch_radius_i8,
 * element blocks for knn_launch_radius_scan). */
#define KNN_RADIUS_MAXBLK 8
/* segments of at most this many records are sorted in LDS (16 bytes each),
 * longer ones in place in global memory */
#define KNN_RADIUS_SORT_LDS 2048
typedef struct {
    const void *ptr[KNN_RADIUS_MAXBLK];
    int64_t base[KNN_RADIUS_MAXBLK];
    int nc[KNN_RADIUS_MAXBLK];
    int nblk;
} knn_radius_blocks_t;
/* nq queries of a tile (their rows 0 .. nq-1 of the byte tile qs8 / the
 * element tile qblk) against the table's blocks.  fill == 0: counts[q] +=
 * query q's hits (the caller zeroes counts).  fill != 0: counts is the
 * queries' cursor (zeroed by the caller; it ends at the number of hits), and
 * hit number s of query q, s < indptr[q + 1] - indptr[q], becomes the record
 * {distance, position, 0} at out[indptr[q] - indptr0[0] + s].  counts, indptr
 * and self_pos (nullable: the position a query leaves out, its own) are the
 * tile's: entry 0 is its first query's.  keep0: a zero distance is a hit.
 * Byte path: T the integer threshold on d^2 (knn_radius_plan.h). */
int knn_launch_radius_i8(int fill, const void *qs8, size_t q_rows_pad, int nq, const int32_t *self_pos,
                         const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, int keep0, int32_t *counts,
                         const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream);
int knn_launch_radius_scan(int fill, int dtype, const void *qblk, int nq, const int32_t *self_pos,
                           const knn_radius_blocks_t *cb, int n, double radius, int keep0, int32_t *counts,
                           const int64_t *indptr, const int64_t *indptr0, knn_neighbour_t *out, void *stream);
/* every query's segment out[indptr[q] - indptr[0] ..) sorted by (distance,
 * position), idx then position -> id (ids[position]; NULL: position + 1);
 * *flag |= 1 where cursor[q] is not the segment's length (that segment is left
 * as it is) */
int knn_launch_radius_sort(size_t mq, const int32_t *cursor, const int64_t *indptr, knn_neighbour_t *out,
                           const int32_t *ids, int *flag, void *stream);
/* knn_radius.hip: knn_index_dbscan's launches (include/knn.h has the
 * definition).  All arrays are by position, m entries.  init: nbr 0, parent[i]
 * = i, no border winner (border: 16 bytes a row; the byte path, s8, uses 8).
 * The count pass is knn_launch_radius_i8 / _scan with fill 0, keep0 1, no
 * self_pos and counts = nbr + qbase.  link: the third form of the same two
 * distance loops, the nq rows of a resident block (positions qbase ..) as the
 * queries against the table's blocks -- two core rows (nbr >= min_pts) at
 * distance <= eps are united in parent (lock-free, the lower position the
 * root); a core row is offered to a query that is not core, which keeps the
 * minimum by (distance, position) in border.  The element form passes through
 * tab, room for tab_cap records: nq a chunk of the launch's grid
 * (knn_radius_chunks, unit 64: gy chunks a block), folded into border by a
 * small kernel behind the launch.  resolve: root (a core row's lowest
 * position), rank (the roots numbered 1 .. C in ascending position, by a
 * prefix sum through bsum: ceil(m / 256) + 1 entries, the last one C) and
 * cluster. */
int knn_launch_dbscan_init(int32_t *nbr, int32_t *parent, void *border, int s8, size_t m, void *stream);
int knn_launch_dbscan_link_i8(const void *qs8, size_t q_rows_pad, int nq, int64_t qbase,
                              const knn_radius_blocks_t *cb, size_t c_rows_pad, int n, int T, const int32_t *nbr,
                              int min_pts, int32_t *parent, void *border, void *stream);
int knn_launch_dbscan_link_scan(int dtype, const void *qblk, int nq, int64_t qbase, const knn_radius_blocks_t *cb,
                                int n, double eps, const int32_t *nbr, int min_pts, int32_t *parent, void *border,
                                void *tab, size_t tab_cap, void *stream);
int knn_launch_dbscan_resolve(const int32_t *nbr, int min_pts, const int32_t *parent, const void *border, int s8,
                              size_t m, int32_t *root, int32_t *rank, int32_t *bsum, int32_t *cluster, void *stream);
/* knn_pack.hip: block elements <-> int16 wire elements (cnt % 8 == 0) */
int knn_launch_wire(int unpack, void *dst, const void *src, int dtype, size_t cnt, void *stream);
/* knn_engine.c: the value knn_last_search_seconds() returns (this thread) */
void knn_set_last_search_seconds(double s);
/* knn_engine.c, for knn_index.c: KNN_OK when `device` is a gfx950 (*cus,
 * nullable: its compute units), else KNN_ERR_NODEVICE; the context's next
 * searches over `rows` queries within its capacity; the device bytes it holds */
int knn_device_probe(int device, int *cus);
int knn_ctx_set_rows(knn_ctx_t *ctx, size_t rows);
size_t knn_ctx_device_bytes(const knn_ctx_t *ctx);
/* bytes of one element of a pack source (KNN_F64 / KNN_F32 / KNN_U8), 0 = unknown */
static inline size_t knn_src_esize(int src_dtype)
{
    return src_dtype == KNN_F64 ? 8 : src_dtype == KNN_F32 ? 4 : src_dtype == KNN_U8 ? 1 : 0;
}

#ifdef __cplusplus
}
#endif

#endif
