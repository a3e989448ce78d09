/*
 * knn_buf.h -- a device buffer with an owner: its pointer and its bytes, and
 * the two functions that allocate and free one while they keep the owner's
 * byte count in step.  The context (knn_engine.c) and the index (knn_index.c)
 * each keep one count over everything they hold between calls; no other code
 * calls hipMalloc or hipFree on that memory, so the count is what is live.
 */
#ifndef KNN_BUF_H
#define KNN_BUF_H

#include "knn.h"

#include <hip/hip_runtime_api.h>
#include <stddef.h>

typedef struct {
    void *p;
    size_t bytes;
} knn_buf_t;

/* `bytes` bytes for the empty buffer b, or KNN_ERR_NOMEM and b still empty */
static inline int knn_buf_alloc(size_t *count, knn_buf_t *b, size_t bytes)
{
    if (hipMalloc(&b->p, bytes) != hipSuccess) {
        b->p = NULL;
        return KNN_ERR_NOMEM;
    }
    b->bytes = bytes;
    *count += bytes;
    return KNN_OK;
}

static inline void knn_buf_release(size_t *count, knn_buf_t *b)
{
    hipFree(b->p);
    *count -= b->bytes;
    b->p = NULL;
    b->bytes = 0;
}

#endif
