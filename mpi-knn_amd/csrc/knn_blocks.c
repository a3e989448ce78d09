/*
 * knn_blocks.c -- the block operations on blocks packed before
 * (include/knn.h): knn_block_append_*, knn_block_scatter_*,
 * knn_block_gather_* and knn_block_gather_pos_*.  Each checks its arguments
 * and calls its launcher in knn_pack.hip; knn_index.c is their first user.
 * They are not with knn_block_pack_* in knn_engine.c: that file is also
 * built on its own against stub launchers (tests/engine_trace).
 */
#include "knn_internal.h"

static int dtype_ok(int dtype) { return dtype == KNN_F64 || dtype == KNN_F32; }

/* Rows that arrive later: block rows row0 .. of a block packed before
 * (include/knn.h). */
int knn_block_append_dt(void *d_block, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                        const void *d_src, int src_dtype, size_t ld, int layout, void *stream)
{
    if (!d_block || !d_src || rows == 0 || n == 0 || cap > 0x7fffffffULL || row0 > cap || rows > cap - row0 ||
        n > 0x7fffffffULL || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return KNN_ERR_INVALID;
    if (layout == KNN_COLMAJOR ? ld < rows : (layout == KNN_ROWMAJOR ? ld < n : 1)) return KNN_ERR_INVALID;
    return knn_launch_append(d_block, dtype, cap, row0, rows, n, d_src, src_dtype, ld, layout, stream);
}

int knn_block_append_s8(void *d_sblock, int dtype, size_t cap, size_t row0, size_t rows, size_t n,
                        const void *d_src, int src_dtype, size_t ld, int layout, void *stream)
{
    if (!d_sblock || !d_src || rows == 0 || n == 0 || cap > 0x7fffffffULL || row0 > cap || rows > cap - row0 ||
        n > KNN_I8_MAX_N || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return KNN_ERR_INVALID;
    if (layout == KNN_COLMAJOR ? ld < rows : (layout == KNN_ROWMAJOR ? ld < n : 1)) return KNN_ERR_INVALID;
    return knn_launch_append_s8(d_sblock, dtype, cap, row0, rows, n, d_src, src_dtype, ld, layout, stream);
}

/* Block row d_pos[i] <- source row d_srow[i] (include/knn.h). */
static int scatter_args_ok(const void *d_block, int dtype, size_t cap, const int32_t *d_pos, size_t rows, size_t n,
                           const void *d_src, size_t src_rows, int src_dtype, size_t ld, int layout, size_t n_max)
{
    if (!d_block || !d_pos || !d_src || rows == 0 || n == 0 || src_rows == 0 || cap > 0x7fffffffULL ||
        src_rows > 0x7fffffffULL || n > n_max || !dtype_ok(dtype) || !knn_src_esize(src_dtype))
        return 0;
    return layout == KNN_COLMAJOR ? ld >= src_rows : (layout == KNN_ROWMAJOR ? ld >= n : 0);
}

int knn_block_scatter_dt(void *d_block, int dtype, size_t cap, const int32_t *d_pos, const int32_t *d_srow,
                         size_t rows, size_t n, const void *d_src, size_t src_rows, int src_dtype, size_t ld,
                         int layout, void *stream)
{
    if (!scatter_args_ok(d_block, dtype, cap, d_pos, rows, n, d_src, src_rows, src_dtype, ld, layout, 0x7fffffffULL))
        return KNN_ERR_INVALID;
    return knn_launch_scatter(d_block, dtype, cap, d_pos, d_srow, rows, n, d_src, src_rows, src_dtype, ld, layout,
                              stream);
}

int knn_block_scatter_s8(void *d_sblock, int dtype, size_t cap, const int32_t *d_pos, const int32_t *d_srow,
                         size_t rows, size_t n, const void *d_src, size_t src_rows, int src_dtype, size_t ld,
                         int layout, void *stream)
{
    if (!scatter_args_ok(d_sblock, dtype, cap, d_pos, rows, n, d_src, src_rows, src_dtype, ld, layout, KNN_I8_MAX_N))
        return KNN_ERR_INVALID;
    return knn_launch_scatter_s8(d_sblock, dtype, cap, d_pos, d_srow, rows, n, d_src, src_rows, src_dtype, ld, layout,
                                 stream);
}

/* Block row row0 + i of d_dst <- row d_list[i] of d_src (include/knn.h). */
static int gather_args_ok(const void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                          const int32_t *d_list, size_t rows, size_t n)
{
    return d_dst && d_src && d_list && d_dst != d_src && rows != 0 && n != 0 && dst_cap <= 0x7fffffffULL &&
           src_cap <= 0x7fffffffULL && src_cap != 0 && row0 <= dst_cap && rows <= dst_cap - row0;
}

int knn_block_gather_dt(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                        const int32_t *d_list, size_t rows, size_t n, int dtype, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n) || !dtype_ok(dtype) ||
        n > 0x7fffffffULL / 8)
        return KNN_ERR_INVALID;
    return knn_launch_gather(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, dtype, stream);
}

int knn_block_gather_s8(void *d_dst, size_t dst_cap, size_t row0, const void *d_src, size_t src_cap,
                        const int32_t *d_list, size_t rows, size_t n, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n) || n > KNN_I8_MAX_N)
        return KNN_ERR_INVALID;
    return knn_launch_gather_rows8(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, stream);
}

/* The same out of a corpus held as nblk blocks of capacity src_cap, by global
 * position (include/knn.h).  d_tab: the blocks' pointers, a device array. */
int knn_block_gather_pos_dt(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab, size_t src_cap,
                            size_t nblk, const int32_t *d_pos, size_t rows, size_t n, int dtype, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_tab, src_cap, d_pos, rows, n) || nblk == 0 || !dtype_ok(dtype) ||
        n > 0x7fffffffULL / 8)
        return KNN_ERR_INVALID;
    return knn_launch_gather_pos(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, dtype, stream);
}

int knn_block_gather_pos_s8(void *d_dst, size_t dst_cap, size_t row0, const void *const *d_tab, size_t src_cap,
                            size_t nblk, const int32_t *d_pos, size_t rows, size_t n, void *stream)
{
    if (!gather_args_ok(d_dst, dst_cap, row0, d_tab, src_cap, d_pos, rows, n) || nblk == 0 || n > KNN_I8_MAX_N)
        return KNN_ERR_INVALID;
    return knn_launch_gather_pos8(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, stream);
}
