/*
 * engine_trace.c -- knn_engine.c's step schedule, traced on a CPU.
 *
 * A stand-alone program: linked with knn_engine.c and nothing of HIP, it
 * stubs the ~25 hip* calls and the knn_launch_* functions the engine uses.
 * hipMalloc is calloc, the copies are memcpy, the device reports 256 CUs, and
 * every stub appends one line to the trace on stdout: the call's name, its
 * streams (s), events (e) and buffers (b; other pointers p) as ids numbered
 * in order of first appearance, and its scalar arguments.  main() drives the
 * scenarios of test_engine_trace.py ("## name" opens one, "# call" marks
 * each call into the engine), each from a block whose meta doubles are
 * filled in by hand to select the contraction.
 *
 *   engine_trace            every scenario
 *   engine_trace NAME...    the named ones
 */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "knn_internal.h"

/* ---- the trace ---------------------------------------------------------- */

#define MAX_OBJ 4096
static struct {
    const char *base;
    size_t size;
    char kind;
    int id, live;
} g_obj[MAX_OBJ];
static int g_nobj, g_next[128];

static void reset_ids(void)
{
    /* (live allocations of an earlier scenario are all freed by then) */
    g_nobj = 0;
    memset(g_next, 0, sizeof(g_next));
}

static int obj_add(const void *p, size_t size, char kind)
{
    if (g_nobj == MAX_OBJ) {
        fprintf(stderr, "engine_trace: object table full\n");
        exit(2);
    }
    g_obj[g_nobj].base = (const char *)p;
    g_obj[g_nobj].size = size ? size : 1;
    g_obj[g_nobj].kind = kind;
    g_obj[g_nobj].id = g_next[(int)kind]++;
    g_obj[g_nobj].live = 1;
    return g_nobj++;
}

/* an id for a stream, event or pointer (into a buffer: b3+4096) */
static void P(const void *p, char kind)
{
    if (!p) {
        printf(" %c-", kind);
        return;
    }
    int o = -1;
    for (int i = 0; i < g_nobj && o < 0; i++)
        if (g_obj[i].live && (const char *)p >= g_obj[i].base && (const char *)p < g_obj[i].base + g_obj[i].size)
            o = i;
    if (o < 0) o = obj_add(p, 1, kind == 'b' ? 'p' : kind);
    printf(" %c%d", g_obj[o].kind, g_obj[o].id);
    if ((const char *)p != g_obj[o].base) printf("+%zu", (size_t)((const char *)p - g_obj[o].base));
}
#define S(x) P((const void *)(x), 's')
#define E(x) P((const void *)(x), 'e')
#define B(x) P((const void *)(x), 'b')
static void T(const char *name) { printf("%s", name); }
static void I(long long v) { printf(" %lld", v); }
static void F(double v) { printf(" %.9g", v); }
static void END(void) { printf("\n"); }

static void *obj_new(size_t size, char kind)
{
    void *p = calloc(size ? size : 1, 1);
    if (p) obj_add(p, size, kind);
    return p;
}

static void obj_free(void *p)
{
    for (int i = 0; i < g_nobj; i++)
        if (g_obj[i].live && g_obj[i].base == (const char *)p) g_obj[i].live = 0;
    free(p);
}

/* ---- HIP ---------------------------------------------------------------- */

hipError_t hipSetDevice(int d) { T("hipSetDevice"); I(d); END(); return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int d)
{
    (void)d;
    memset(prop, 0, sizeof(*prop));
    strcpy(prop->gcnArchName, "gfx950:sramecc+:xnack-");
    prop->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int *lo, int *hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { T("hipDeviceSynchronize"); END(); return hipSuccess; }

hipError_t hipMalloc(void **p, size_t size)
{
    *p = obj_new(size, 'b');
    T("hipMalloc"); B(*p); I((long long)size); END();
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p)
{
    if (!p) return hipSuccess;
    T("hipFree"); B(p); END();
    obj_free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t size, unsigned int flags)
{
    (void)flags;
    *p = obj_new(size, 'b');
    T("hipHostMalloc"); B(*p); I((long long)size); END();
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *p) { T("hipHostFree"); B(p); END(); obj_free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int flags)
{
    (void)flags;
    *dev = host;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    T("hipMemcpy"); B(dst); B(src); I((long long)n); I(kind); END();
    memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    /* (the destination may be the engine's stack: named by the copy's kind alone) */
    T("hipMemcpyAsync");
    if (kind == hipMemcpyDeviceToHost) printf(" host"); else B(dst);
    B(src); I((long long)n); I(kind); S(s); END();
    memcpy(dst, src, n);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags)
{
    *s = (hipStream_t)obj_new(1, 's');
    T("hipStreamCreateWithFlags"); S(*s); I(flags); END();
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int prio)
{
    *s = (hipStream_t)obj_new(1, 's');
    T("hipStreamCreateWithPriority"); S(*s); I(flags); I(prio); END();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { T("hipStreamDestroy"); S(s); END(); obj_free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { T("hipStreamSynchronize"); S(s); END(); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags)
{
    T("hipStreamWaitEvent"); S(s); E(e); I(flags); END();
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e)
{
    *e = (hipEvent_t)obj_new(1, 'e');
    T("hipEventCreate"); E(*e); END();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int flags)
{
    *e = (hipEvent_t)obj_new(1, 'e');
    T("hipEventCreateWithFlags"); E(*e); I(flags); END();
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { T("hipEventDestroy"); E(e); END(); obj_free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { T("hipEventRecord"); E(e); S(s); END(); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { T("hipEventSynchronize"); E(e); END(); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    T("hipEventElapsedTime"); E(a); E(b); END();
    *ms = 0.f;
    return hipSuccess;
}

/* ---- the launchers of knn_internal.h ------------------------------------ */

int knn_launch_begin_init(double *qthr, unsigned long long *qsum, int nq_pad, int *counts, void *stream)
{
    T("knn_launch_begin_init"); B(qthr); B(qsum); I(nq_pad); B(counts); S(stream); END();
    counts[0] = counts[1] = 0;
    return KNN_OK;
}

int knn_launch_count_out(const int *d_count, int *mapped, const double *meta, double *mapped_meta, void *stream)
{
    T("knn_launch_count_out"); B(d_count); B(mapped); B(meta); B(mapped_meta); S(stream); END();
    mapped[0] = 0;   /* no unresolved query */
    mapped[1] = d_count[1];
    if (meta) memcpy(mapped_meta, meta, KNN_META_DOUBLES * sizeof(double));
    return KNN_OK;
}

int knn_launch_dist_topk(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                         const void *cblk, size_t c_rows_pad, size_t c_base, int nc, int n, const double *meta,
                         int nsplit, double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr,
                         const void *qsh, const void *csh, const void *cn_ptr, int flags, float m2s, void *stream)
{
    T("knn_launch_dist_topk"); I(dtype); I(kp); I(k); B(qblk); I((long long)q_rows_pad); I((long long)q_base); I(nq);
    B(cblk); I((long long)c_rows_pad); I((long long)c_base); I(nc); I(n); B(meta); I(nsplit); B(part_d); B(part_i);
    B(part_T); I(nq_pad); B(qthr); B(qsh); B(csh); B(cn_ptr); I(flags); F(m2s); S(stream); END();
    return KNN_OK;
}

int knn_launch_dist_split_n(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                            const void *qsp, const knn_split_blocks_t *cb, int n, const double *meta, int nsplit,
                            double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr, int xord,
                            float m2s, void *stream)
{
    T("knn_launch_dist_split_n"); I(dtype); I(kp); I(k); B(qblk); I((long long)q_rows_pad); I((long long)q_base);
    I(nq); B(qsp); I(n); B(meta); I(nsplit); B(part_d); B(part_i); B(part_T); I(nq_pad); B(qthr); I(xord); F(m2s);
    S(stream);
    printf(" blocks %d", cb->nblk);
    for (int b = 0; b < cb->nblk; b++) {
        printf(" [");
        B(cb->sp[b]); B(cb->nrm[b]); I(cb->base[b]); I(cb->nc[b]); I(cb->lim[b]);
        printf(" ]");
    }
    END();
    return KNN_OK;
}

int knn_launch_dist_i8(int kp, int kl, int lpq, int k, const void *qsh, size_t q_rows_pad, size_t q_base, int nq,
                       const knn_i8_blocks_t *cb, size_t c_rows_pad, int n, int nsplit, double *part_d, int *part_i,
                       double *part_T, int nq_pad, double *qthr, unsigned long long *qsum, int keep_zero, void *stream)
{
    T("knn_launch_dist_i8"); I(kp); I(kl); I(lpq); I(k); B(qsh); I((long long)q_rows_pad); I((long long)q_base); I(nq);
    I((long long)c_rows_pad); I(n); I(nsplit); B(part_d); B(part_i); B(part_T); I(nq_pad); B(qthr); B(qsum);
    I(keep_zero); S(stream);
    printf(" blocks %d", cb->nblk);
    for (int b = 0; b < cb->nblk; b++) {
        printf(" [");
        B(cb->ptr[b]); B(cb->nptr[b]); I(cb->base[b]); I(cb->nc[b]);
        printf(" ]");
    }
    END();
    return KNN_OK;
}

int knn_launch_merge_n(int dtype, int kp, int k, const double *part_d, const int *part_i, const double *part_T,
                       int nsplit, int lpq, int kl, int nq, int nq_pad, int first_step, double *st_d, double *st_x,
                       int *st_i, double *st_T, const void *qblk, size_t q_rows_pad, const knn_merge_blocks_t *mb,
                       int n, const double *meta, double *qthr, int filt, const int *qperm, void *stream)
{
    T("knn_launch_merge_n"); I(dtype); I(kp); I(k); B(part_d); B(part_i); B(part_T); I(nsplit); I(lpq); I(kl); I(nq);
    I(nq_pad); I(first_step); B(st_d); B(st_x); B(st_i); B(st_T); B(qblk); I((long long)q_rows_pad); I(n); B(meta);
    B(qthr); I(filt); B(qperm); S(stream);
    printf(" blocks %d", mb->nblk);
    for (int b = 0; b < mb->nblk; b++) {
        printf(" [");
        B(mb->ptr[b]); I(mb->base[b]); I(mb->nc[b]);
        printf(" ]");
    }
    END();
    return KNN_OK;
}

int knn_launch_merge_rank(int dtype, int kp, int kl, int k, const double *part_d, const int *part_i,
                          const double *part_T, int nsplit, int lpq, int nq, int nq_pad, int first_step, double *st_d,
                          double *st_x, int *st_i, double *st_T, double *qthr, knn_neighbour_t *fin_out,
                          int *fail_count, int *fail_list, int *mode_out, double *fbound, const double *meta, int n,
                          int force_fail, void *stream)
{
    T("knn_launch_merge_rank"); I(dtype); I(kp); I(kl); I(k); B(part_d); B(part_i); B(part_T); I(nsplit); I(lpq); I(nq);
    I(nq_pad); I(first_step); B(st_d); B(st_x); B(st_i); B(st_T); B(qthr); printf(" fin"); B(fin_out); B(fail_count);
    B(fail_list); B(mode_out); B(fbound); B(meta); I(n); I(force_fail); S(stream); END();
    return KNN_OK;
}

int knn_launch_finalize(int dtype, int kp, const double *st_d, const double *st_x, const int *st_i, const double *st_T,
                        const void *qblk, size_t q_rows_pad, int nq, int n, int k, const double *meta,
                        knn_neighbour_t *out, int *fail_count, int *fail_list, int *mode_out, double *fbound,
                        int force_fail, int filt, void *stream)
{
    T("knn_launch_finalize"); I(dtype); I(kp); B(st_d); B(st_x); B(st_i); B(st_T); B(qblk); I((long long)q_rows_pad);
    I(nq); I(n); I(k); B(meta); B(out); B(fail_count); B(fail_list); B(mode_out); B(fbound); I(force_fail); I(filt);
    S(stream); END();
    return KNN_OK;
}

size_t knn_order_tmp_bytes(int nq) { return (size_t)nq * 8; }

int knn_launch_order(const int *part_i, int nsplit, int lpq, int kl, int nq, int nq_pad, long long q_base, int rounds,
                     int *lab, int *keys, int *iota, int *perm, void *tmp, size_t tmp_bytes, void *stream)
{
    T("knn_launch_order"); B(part_i); I(nsplit); I(lpq); I(kl); I(nq); I(nq_pad); I(q_base); I(rounds); B(lab);
    B(keys); B(iota); B(perm); B(tmp); I((long long)tmp_bytes); S(stream); END();
    return KNN_OK;
}

int knn_launch_shadow(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, void *stream)
{
    T("knn_launch_shadow"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); S(stream); END();
    return KNN_OK;
}

int knn_launch_shadow8(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, const double *meta,
                       void *stream)
{
    T("knn_launch_shadow8"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); B(meta); S(stream);
    END();
    return KNN_OK;
}

int knn_launch_shadow_split(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, float scale, void *stream)
{
    T("knn_launch_shadow_split"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); F(scale); S(stream);
    END();
    return KNN_OK;
}

int knn_launch_shadow_split_n(int nblk, void *const *dst, const void *const *src, const size_t *rows_pad, int dtype,
                              size_t n, float scale, void *stream)
{
    T("knn_launch_shadow_split_n"); I(dtype); I((long long)n); F(scale); S(stream);
    printf(" blocks %d", nblk);
    for (int b = 0; b < nblk; b++) {
        printf(" [");
        B(dst[b]); B(src[b]); I((long long)rows_pad[b]);
        printf(" ]");
    }
    END();
    return KNN_OK;
}

/* the rest of the engine's imports: no scenario reaches them */
#define UNREACHED(name)                                          \
    do {                                                         \
        fprintf(stderr, "engine_trace: unexpected " name "\n");  \
        exit(2);                                                 \
    } while (0)

int knn_launch_pack(void *blk, int dtype, size_t cap, size_t rows, size_t n, const void *src, int src_dtype, size_t ld,
                    int layout, void *stream)
{
    (void)blk, (void)dtype, (void)cap, (void)rows, (void)n, (void)src, (void)src_dtype, (void)ld, (void)layout,
        (void)stream;
    UNREACHED("knn_launch_pack");
}
int knn_launch_pack_s8(void *dst, int dtype, size_t cap, size_t rows, size_t n, const void *src, int src_dtype,
                       size_t ld, int layout, void *stream)
{
    (void)dst, (void)dtype, (void)cap, (void)rows, (void)n, (void)src, (void)src_dtype, (void)ld, (void)layout,
        (void)stream;
    UNREACHED("knn_launch_pack_s8");
}
int knn_launch_gather8(void *dst, const void *src, const int *list, int cnt, size_t n, size_t src_rows_pad,
                       size_t dst_rows_pad, const double *src_qthr, double *dst_qthr, void *stream)
{
    (void)dst, (void)src, (void)list, (void)cnt, (void)n, (void)src_rows_pad, (void)dst_rows_pad, (void)src_qthr,
        (void)dst_qthr, (void)stream;
    UNREACHED("knn_launch_gather8");
}
int knn_launch_resolve8(unsigned char *flag, const int *list, int cnt, const int *sub_fail, const int *sub_cnt,
                        const knn_neighbour_t *sub_out, int k, knn_neighbour_t *out, int *new_list, int *new_cnt,
                        void *stream)
{
    (void)flag, (void)list, (void)cnt, (void)sub_fail, (void)sub_cnt, (void)sub_out, (void)k, (void)out,
        (void)new_list, (void)new_cnt, (void)stream;
    UNREACHED("knn_launch_resolve8");
}
int knn_launch_rescan_init(int kp, double *rs_d, int *rs_i, int nfail, void *stream)
{
    (void)kp, (void)rs_d, (void)rs_i, (void)nfail, (void)stream;
    UNREACHED("knn_launch_rescan_init");
}
int knn_launch_rescan_step(int dtype, int kp, const int *fail_list, int nfail, const double *fbound, const void *qblk,
                           const void *cblk, size_t c_base, int nc, int n, int k, double *rs_d, int *rs_i,
                           long long self_base, void *stream)
{
    (void)dtype, (void)kp, (void)fail_list, (void)nfail, (void)fbound, (void)qblk, (void)cblk, (void)c_base, (void)nc,
        (void)n, (void)k, (void)rs_d, (void)rs_i, (void)self_base, (void)stream;
    UNREACHED("knn_launch_rescan_step");
}
int knn_launch_rescan_end(int kp, const int *fail_list, int nfail, const double *rs_d, const int *rs_i, int k,
                          knn_neighbour_t *out, void *stream)
{
    (void)kp, (void)fail_list, (void)nfail, (void)rs_d, (void)rs_i, (void)k, (void)out, (void)stream;
    UNREACHED("knn_launch_rescan_end");
}
int knn_launch_wire(int unpack, void *dst, const void *src, int dtype, size_t cnt, void *stream)
{
    (void)unpack, (void)dst, (void)src, (void)dtype, (void)cnt, (void)stream;
    UNREACHED("knn_launch_wire");
}
int knn_search_ring_host(const double *X, size_t m, size_t n, int layout, int k, int ngpus, int dtype,
                         knn_neighbour_t *out, double *seconds)
{
    (void)X, (void)m, (void)n, (void)layout, (void)k, (void)ngpus, (void)dtype, (void)out, (void)seconds;
    UNREACHED("knn_search_ring_host");
}

/* ---- the scenarios ------------------------------------------------------ */

#define ROWS 1024   /* rows of every block, and the queries */
#define DIMS 64
#define K 10
#define MAXB 9

enum { INT8, SCAN64, SPLIT32 };   /* the contraction the meta selects */

#define CHECK(x)                                                              \
    do {                                                                      \
        const int rc_ = (x);                                                  \
        if (rc_) {                                                            \
            fprintf(stderr, "engine_trace: %s -> %d\n", #x, rc_);             \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static void mark(const char *what) { printf("# %s\n", what); }

typedef struct {
    knn_ctx_t *c;
    int mode, dtype;
    void *stream, *stream2;   /* the caller's stream, and a second one */
    void *blk[1 + MAXB];      /* [0] the own (query) block, then foreign ones */
    void *sblk[1 + MAXB];     /* their byte blocks (INT8) */
    size_t nc[1 + MAXB], base[1 + MAXB];
    const double *meta;
    void *out;
} run_t;

static void run_begin(run_t *r);

static void run_open(run_t *r, int mode, int solo, int prof)
{
    memset(r, 0, sizeof(*r));
    r->mode = mode;
    reset_ids();
    r->dtype = mode == SPLIT32 ? KNN_F32 : KNN_F64;
    r->stream = obj_new(1, 's');
    r->stream2 = obj_new(1, 's');
    const size_t moff = knn_block_meta_offset_dt(ROWS, DIMS, r->dtype);
    for (int b = 0; b <= MAXB; b++) {
        CHECK(hipMalloc(&r->blk[b], knn_block_bytes_dt(ROWS, DIMS, r->dtype)) != hipSuccess);
        r->nc[b] = ROWS;
        r->base[b] = (size_t)b * ROWS;
    }
    double *m = (double *)((char *)r->blk[0] + moff);
    r->meta = m;
    if (mode == INT8) {          /* integers in [0, 255] */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 255.0;
        m[KNN_META_MAXNORM] = 255.0 * 255.0 * DIMS;
    } else if (mode == SCAN64) { /* a non-finite value: no fast contraction */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 1.0;
        m[KNN_META_NONFINITE] = 1.0;
    } else {                     /* real values in [0, 1): the split fp16 filter */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 0.75;
        m[KNN_META_MAXNORM] = DIMS;
        m[KNN_META_NONINT] = 1.0;
    }
    CHECK(hipMalloc(&r->out, (size_t)ROWS * K * sizeof(knn_neighbour_t)) != hipSuccess);
    mark("create");
    CHECK(knn_ctx_create_dt(&r->c, 0, ROWS, DIMS, ROWS, K, r->dtype));
    CHECK(knn_ctx_set_solo(r->c, solo));
    if (prof) {
        mark("profile");
        CHECK(knn_ctx_profile(r->c, 1, NULL, NULL, NULL));
    }
    run_begin(r);
}

static void run_begin(run_t *r)
{
    mark("begin");
    CHECK(knn_ctx_begin(r->c, r->blk[0], ROWS, 0, r->meta, r->stream));
    const int want = r->mode == INT8 ? 8 : (r->mode == SPLIT32 ? 16 : 64);
    if (knn_ctx_contraction_bits(r->c) != want || knn_ctx_split(r->c) != (r->mode == SPLIT32)) {
        fprintf(stderr, "engine_trace: the meta selected another contraction\n");
        exit(1);
    }
}

/* byte blocks of the first n blocks (the int8 direct exchange) */
static void run_byte_blocks(run_t *r, int n)
{
    for (int b = 0; b < n; b++) {
        CHECK(hipMalloc(&r->sblk[b], knn_ctx_shadow_bytes(r->c, ROWS)) != hipSuccess);
        mark("shadow_pack");
        CHECK(knn_ctx_shadow_pack(r->c, r->sblk[b], r->blk[b], ROWS, r->stream));
    }
}

static void run_step(run_t *r, int b)
{
    mark("step");
    CHECK(knn_ctx_step(r->c, r->blk[b], r->nc[b], r->base[b], r->stream));
}

static void run_end(run_t *r, void *end_stream, int prof)
{
    size_t unresolved = 0;
    mark("end");
    CHECK(knn_ctx_end(r->c, (knn_neighbour_t *)r->out, &unresolved, end_stream));
    if (prof) {
        int merges = 0, launches = 0;
        CHECK(knn_ctx_profile(r->c, -1, NULL, NULL, &launches));
        CHECK(knn_ctx_profile_merge(r->c, NULL, &merges, NULL));
        printf("# profiled steps %d merges %d\n", launches, merges);
    }
}

static void run_close(run_t *r, void *end_stream, int prof)
{
    run_end(r, end_stream, prof);
    mark("destroy");
    CHECK(knn_ctx_destroy(r->c));
    for (int b = 0; b <= MAXB; b++) {
        hipFree(r->blk[b]);
        hipFree(r->sblk[b]);
    }
    hipFree(r->out);
    obj_free(r->stream);
    obj_free(r->stream2);
}

static void solo1_i8(int prof)
{
    run_t r;
    run_open(&r, INT8, 1, prof);
    run_step(&r, 0);
    run_close(&r, r.stream, prof);
}

static void solo2_i8(int prof)
{
    run_t r;
    run_open(&r, INT8, 1, prof);
    run_step(&r, 0);
    run_step(&r, 1);
    run_close(&r, r.stream, prof);
}

static void solo1_end_other_stream(int prof)
{
    run_t r;
    run_open(&r, INT8, 1, prof);
    run_step(&r, 0);
    run_close(&r, r.stream2, prof);
}

static void six_steps(int mode, int prof)
{
    run_t r;
    run_open(&r, mode, 0, prof);
    for (int b = 0; b < 6; b++) run_step(&r, b);
    run_close(&r, r.stream, prof);
}

/* The direct exchange: the own block, then every received block in one fused
 * step.  Two searches on one context: the first grows the pair's lists under
 * the pending own-block step (which is then merged alone), the second -- a
 * ring's steady state -- shares one merge between both steps. */
static void shadow_own_then_7(int prof)
{
    run_t r;
    run_open(&r, INT8, 0, prof);
    run_byte_blocks(&r, 8);
    for (int pass = 0; pass < 2; pass++) {
        if (pass) run_begin(&r);
        mark("step");
        CHECK(knn_ctx_step_shadow(r.c, r.sblk[0], r.nc[0], r.base[0], r.stream));
        mark("step");
        CHECK(knn_ctx_step_shadow_n(r.c, 7, (const void *const *)(r.sblk + 1), r.nc + 1, r.base + 1, r.stream));
        if (!pass) run_end(&r, r.stream, prof);
    }
    run_close(&r, r.stream, prof);
}

/* rows: of each foreign block (their ids follow the own block's) */
static void split_own_then_n(int solo, int nblk, size_t rows, int prof)
{
    run_t r;
    run_open(&r, SPLIT32, solo, prof);
    for (int b = 1; b <= nblk; b++) {
        r.nc[b] = rows;
        r.base[b] = ROWS + (size_t)(b - 1) * rows;
    }
    for (int pass = 0; pass < 2; pass++) {
        if (pass) run_begin(&r);
        run_step(&r, 0);
        mark("step");
        CHECK(knn_ctx_step_n(r.c, nblk, (const void *const *)(r.blk + 1), r.nc + 1, r.base + 1, r.stream));
        if (!pass) run_end(&r, r.stream, prof);
    }
    run_close(&r, r.stream, prof);
}

static void split_9(int prof)
{
    run_t r;
    run_open(&r, SPLIT32, 0, prof);
    mark("step");
    CHECK(knn_ctx_step_n(r.c, 9, (const void *const *)(r.blk + 1), r.nc + 1, r.base + 1, r.stream));
    run_close(&r, r.stream, prof);
}

int main(int argc, char **argv)
{
    static const char *names[] = {"solo1_i8", "solo2_i8", "solo1_end_other_stream", "six_i8", "six_f64",
                                  "shadow_own_then_7", "split_own_then_7", "split_9", "split_own_then_2",
                                  "solo_split_own_then_2"};
    const int nnames = (int)(sizeof(names) / sizeof(names[0]));
    for (int prof = 0; prof < 2; prof++)
        for (int i = 0; i < nnames; i++) {
            char full[64];
            snprintf(full, sizeof(full), "%s%s", names[i], prof ? "+prof" : "");
            int wanted = argc < 2;
            for (int a = 1; a < argc; a++) wanted |= !strcmp(argv[a], full);
            if (!wanted) continue;
            printf("## %s\n", full);
            switch (i) {
            case 0: solo1_i8(prof); break;
            case 1: solo2_i8(prof); break;
            case 2: solo1_end_other_stream(prof); break;
            case 3: six_steps(INT8, prof); break;
            case 4: six_steps(SCAN64, prof); break;
            case 5: shadow_own_then_7(prof); break;
            case 6: split_own_then_n(0, 7, ROWS, prof); break;
            case 7: split_9(prof); break;
            case 8: split_own_then_n(0, 2, ROWS / 2, prof); break;
            case 9: split_own_then_n(1, 2, ROWS / 2, prof); break;
            }
        }
    return 0;
}
