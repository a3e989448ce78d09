/*
 * engine_trace.c -- knn_engine.c's step schedule and device memory, traced on
 * a CPU, and its failure paths swept.
 *
 * A stand-alone program: linked with knn_engine.c and nothing of HIP.  The
 * line buffer, the live set, the fault knob and the plain HIP stubs are
 * tests/trace_common.h's (shared with index_trace.c); this file adds the
 * stream and event stubs the engine needs (streams are S1, S2, ... in the
 * live set) and the knn_launch_* functions.  The device reports 256 CUs.  The
 * launchers compute nothing: k_count_out's stub writes the unresolved count
 * the scenario chose into the mapped words, and resolve8's the count behind
 * the re-search, so the engine decides its paths as on a device.
 *
 * A scenario is a table of calls into the engine ("# call" marks each in the
 * trace, "# live N" the device bytes live behind it), from blocks whose meta
 * doubles are filled in by hand to select the contraction.  The harness's own
 * buffers (the blocks, the byte blocks, the output) are kind U, its two
 * streams S1 and S2, so kind A is exactly what the engine allocated.
 *
 *   engine_trace            every scenario's trace ("## name" opens one);
 *                           exit status 1 when knn_ctx_device_bytes differed
 *                           from the live bytes behind some call
 *   engine_trace NAME...    the named ones
 *   engine_trace --sweep    the fault sweep; exit status 1 on a violation
 *
 * The sweep: the stubs count every call whose failure the engine can see
 * (allocations, pinned allocations, stream and event creation, event records
 * and waits, synchronisations, copies, launchers) and can fail the N-th.  For
 * every call of every scenario, with C its count on a clean run, and for
 * N = 1 .. C, the call runs on a rebuilt pre-state with fault N, and then:
 *  (a) it returned non-zero -- unless the fault fell into the int8 re-search
 *      (from behind knn_ctx_end's read of the count, or from the start of
 *      knn_ctx_research_blocks, to the read of the count behind resolve8, as
 *      the clean run numbered those calls), which both absorb by design (the
 *      exact rescan resolves the same queries): counted as "absorbed";
 *  (b) nothing was freed that was not live;
 *  (c) the live device bytes are what knn_ctx_device_bytes reports;
 *  (d) the scenario's first search, run again from its begin on the same
 *      context, succeeds, and its lines from the first enqueue on are those of
 *      that search on a fresh context -- or (counted as "warm": how steps
 *      pair and what sizes the launches get depends on how far the buffers
 *      have grown) of its second run there, or of that search behind the
 *      scenario's clean calls up to the failed one, or up to and with it.
 *      Set aside: allocations and frees; a host wait directly in front of one
 *      and not directly behind a copy or k_count_out (a buffer's grow wait,
 *      never the wait for a result); creation and destruction of streams and
 *      events, hipSetDevice, hipEventElapsedTime; names in order of appearance;
 *  (e) knn_ctx_destroy leaves nothing live: no device memory, no pinned memory,
 *      no event, no stream.
 */
#define TRACE_PROG "engine_trace"
#define FALLIBLE_ORDER
#define TRACE_NAME_KINDS "APES"
static int g_bad_free, g_absorbed;
/* The counted calls of the int8 re-search inside the call under way, first to
 * last: as the stubs see them (g_span_*), and as the clean run had them, for
 * the fault (g_abs_*). */
static long g_span_lo, g_span_hi, g_abs_lo, g_abs_hi;
#define LIVE_BAD_FREE(who) \
    do {                   \
        (void)(who);       \
        g_bad_free++;      \
    } while (0)
#define FAULT_HOOK() (g_absorbed = g_abs_lo > 0 && g_calls >= g_abs_lo && g_calls <= g_abs_hi)
#include "../trace_common.h"

#include "knn_internal.h"

/* ---- HIP: devices, streams, events -------------------------------------- */

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
hipError_t hipDeviceSynchronize(void)
{
    FALLIBLE("hipDeviceSynchronize", hipErrorUnknown);
    L("hipDeviceSynchronize");
    return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int flags)
{
    (void)flags;
    *dev = host;
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags)
{
    FALLIBLE("hipStreamCreateWithFlags", hipErrorOutOfMemory);
    *s = (hipStream_t)live_new(1, 'S');
    L("hipStreamCreateWithFlags %s %u", N(*s), flags);
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int prio)
{
    FALLIBLE("hipStreamCreateWithPriority", hipErrorOutOfMemory);
    *s = (hipStream_t)live_new(1, 'S');
    L("hipStreamCreateWithPriority %s %u %d", N(*s), flags, prio);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    L("hipStreamDestroy %s", N(s));
    live_free(s, "hipStreamDestroy");
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags)
{
    FALLIBLE("hipStreamWaitEvent", hipErrorUnknown);
    L("hipStreamWaitEvent %s %s %u", N(s), EV(e), flags);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int flags)
{
    FALLIBLE("hipEventCreateWithFlags", hipErrorOutOfMemory);
    int *p = (int *)malloc(sizeof(int));
    if (!p) DIE("out of memory");
    *p = ++g_ord['E'];
    g_nevents++;
    *e = (hipEvent_t)p;
    L("hipEventCreateWithFlags %s %u", EV(*e), flags);
    return hipSuccess;
}

/* ---- the launchers of knn_internal.h ------------------------------------ */

/* one line, built argument by argument */
static char g_buf[1000];
static size_t g_at;
static void A(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (g_at < sizeof(g_buf)) g_at += (size_t)vsnprintf(g_buf + g_at, sizeof(g_buf) - g_at, fmt, ap);
    va_end(ap);
}
static void T(const char *name) { g_at = 0; A("%s", name); }
static void I(long long v) { A(" %lld", v); }
static void F(double v) { A(" %.9g", v); }
static void B(const void *p) { A(" %s", N(p)); }
#define S(x) B((const void *)(x))
static void EOL(void) { L("%s", g_buf); }

/* what the scenario chose: the unresolved queries k_count_out reports, and
 * those resolve8 leaves behind the re-search */
static int g_unres, g_unres2;

/* a launch's partial lists: nsplit splits of nq_pad x per entries and nq_pad bounds */
static void need_lists(const char *who, const double *part_d, const int *part_i, const double *part_T, int nsplit,
                       int per, int nq_pad)
{
    const size_t cnt = (size_t)nsplit * (size_t)nq_pad;
    need(part_d, cnt * (size_t)per * sizeof(double), who);
    need(part_i, cnt * (size_t)per * sizeof(int), who);
    need(part_T, cnt * sizeof(double), who);
}

int knn_launch_begin_init(double *qthr, unsigned long long *qsum, int nq_pad, int *counts, void *stream)
{
    FALLIBLE("knn_launch_begin_init", KNN_ERR_HIP);
    T("knn_launch_begin_init"); B(qthr); B(qsum); I(nq_pad); B(counts); S(stream); EOL();
    counts[0] = counts[1] = 0;
    return KNN_OK;
}

int knn_launch_count_out(const int *d_count, int *mapped, const double *meta, double *mapped_meta, void *stream)
{
    FALLIBLE("knn_launch_count_out", KNN_ERR_HIP);
    T("knn_launch_count_out"); B(d_count); B(mapped); B(meta); B(mapped_meta); S(stream); EOL();
    mapped[0] = g_unres;
    mapped[1] = d_count[1];
    if (meta) memcpy(mapped_meta, meta, KNN_META_DOUBLES * sizeof(double));
    g_span_lo = g_calls + 2;   /* (behind this launch's host wait knn_ctx_end re-searches) */
    return KNN_OK;
}

int knn_launch_dist_topk(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                         const void *cblk, size_t c_rows_pad, size_t c_base, int nc, int n, const double *meta,
                         int nsplit, double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr,
                         const void *qsh, const void *csh, const void *cn_ptr, int flags, float m2s, void *stream)
{
    FALLIBLE("knn_launch_dist_topk", KNN_ERR_HIP);
    T("knn_launch_dist_topk"); I(dtype); I(kp); I(k); B(qblk); I((long long)q_rows_pad); I((long long)q_base); I(nq);
    B(cblk); I((long long)c_rows_pad); I((long long)c_base); I(nc); I(n); B(meta); I(nsplit); B(part_d); B(part_i);
    B(part_T); I(nq_pad); B(qthr); B(qsh); B(csh); B(cn_ptr); I(flags); F(m2s); S(stream); EOL();
    need_lists("knn_launch_dist_topk", part_d, part_i, part_T, nsplit, 4 * knn_kl_for(kp, dtype), nq_pad);
    return KNN_OK;
}

int knn_launch_dist_split_n(int dtype, int kp, int k, const void *qblk, size_t q_rows_pad, size_t q_base, int nq,
                            const void *qsp, const knn_split_blocks_t *cb, int n, const double *meta, int nsplit,
                            double *part_d, int *part_i, double *part_T, int nq_pad, double *qthr, int xord,
                            float m2s, void *stream)
{
    FALLIBLE("knn_launch_dist_split_n", KNN_ERR_HIP);
    T("knn_launch_dist_split_n"); I(dtype); I(kp); I(k); B(qblk); I((long long)q_rows_pad); I((long long)q_base);
    I(nq); B(qsp); I(n); B(meta); I(nsplit); B(part_d); B(part_i); B(part_T); I(nq_pad); B(qthr); I(xord); F(m2s);
    S(stream);
    A(" blocks %d", cb->nblk);
    for (int b = 0; b < cb->nblk; b++) {
        A(" [");
        B(cb->sp[b]); B(cb->nrm[b]); I(cb->base[b]); I(cb->nc[b]); I(cb->lim[b]);
        A(" ]");
    }
    EOL();
    need_lists("knn_launch_dist_split_n", part_d, part_i, part_T, nsplit, 4 * knn_kl_for(kp, dtype), nq_pad);
    for (int b = 0; b < cb->nblk; b++) need(cb->sp[b], (size_t)cb->lim[b] * knn_split_rs((size_t)n), "knn_launch_dist_split_n");
    return KNN_OK;
}

int knn_launch_dist_i8(int kp, int kl, int lpq, int k, const void *qsh, size_t q_rows_pad, size_t q_base, int nq,
                       const knn_i8_blocks_t *cb, size_t c_rows_pad, int n, int nsplit, double *part_d, int *part_i,
                       double *part_T, int nq_pad, double *qthr, unsigned long long *qsum, int keep_zero, void *stream)
{
    FALLIBLE("knn_launch_dist_i8", KNN_ERR_HIP);
    T("knn_launch_dist_i8"); I(kp); I(kl); I(lpq); I(k); B(qsh); I((long long)q_rows_pad); I((long long)q_base); I(nq);
    I((long long)c_rows_pad); I(n); I(nsplit); B(part_d); B(part_i); B(part_T); I(nq_pad); B(qthr); B(qsum);
    I(keep_zero); S(stream);
    A(" blocks %d", cb->nblk);
    for (int b = 0; b < cb->nblk; b++) {
        A(" [");
        B(cb->ptr[b]); B(cb->nptr[b]); I(cb->base[b]); I(cb->nc[b]);
        A(" ]");
    }
    EOL();
    need_lists("knn_launch_dist_i8", part_d, part_i, part_T, nsplit, lpq * kl, nq_pad);
    for (int b = 0; b < cb->nblk; b++) need(cb->ptr[b], knn_s8_meta_offset(c_rows_pad, (size_t)n), "knn_launch_dist_i8");
    return KNN_OK;
}

int knn_launch_merge_n(int dtype, int kp, int k, const double *part_d, const int *part_i, const double *part_T,
                       int nsplit, int lpq, int kl, int nq, int nq_pad, int first_step, double *st_d, double *st_x,
                       int *st_i, double *st_T, const void *qblk, size_t q_rows_pad, const knn_merge_blocks_t *mb,
                       int n, const double *meta, double *qthr, int filt, const int *qperm, void *stream)
{
    FALLIBLE("knn_launch_merge_n", KNN_ERR_HIP);
    T("knn_launch_merge_n"); I(dtype); I(kp); I(k); B(part_d); B(part_i); B(part_T); I(nsplit); I(lpq); I(kl); I(nq);
    I(nq_pad); I(first_step); B(st_d); B(st_x); B(st_i); B(st_T); B(qblk); I((long long)q_rows_pad); I(n); B(meta);
    B(qthr); I(filt); B(qperm); S(stream);
    A(" blocks %d", mb->nblk);
    for (int b = 0; b < mb->nblk; b++) {
        A(" [");
        B(mb->ptr[b]); I(mb->base[b]); I(mb->nc[b]);
        A(" ]");
    }
    EOL();
    return KNN_OK;
}

int knn_launch_merge_rank(int dtype, int kp, int kl, int k, const double *part_d, const int *part_i,
                          const double *part_T, int nsplit, int lpq, int nq, int nq_pad, int first_step, double *st_d,
                          double *st_x, int *st_i, double *st_T, double *qthr, knn_neighbour_t *fin_out,
                          int *fail_count, int *fail_list, int *mode_out, double *fbound, const double *meta, int n,
                          int force_fail, void *stream)
{
    FALLIBLE("knn_launch_merge_rank", KNN_ERR_HIP);
    T("knn_launch_merge_rank"); I(dtype); I(kp); I(kl); I(k); B(part_d); B(part_i); B(part_T); I(nsplit); I(lpq); I(nq);
    I(nq_pad); I(first_step); B(st_d); B(st_x); B(st_i); B(st_T); B(qthr); A(" fin"); B(fin_out); B(fail_count);
    B(fail_list); B(mode_out); B(fbound); B(meta); I(n); I(force_fail); S(stream); EOL();
    return KNN_OK;
}

int knn_launch_finalize(int dtype, int kp, const double *st_d, const double *st_x, const int *st_i, const double *st_T,
                        const void *qblk, size_t q_rows_pad, int nq, int n, int k, const double *meta,
                        knn_neighbour_t *out, int *fail_count, int *fail_list, int *mode_out, double *fbound,
                        int force_fail, int filt, void *stream)
{
    FALLIBLE("knn_launch_finalize", KNN_ERR_HIP);
    T("knn_launch_finalize"); I(dtype); I(kp); B(st_d); B(st_x); B(st_i); B(st_T); B(qblk); I((long long)q_rows_pad);
    I(nq); I(n); I(k); B(meta); B(out); B(fail_count); B(fail_list); B(mode_out); B(fbound); I(force_fail); I(filt);
    S(stream); EOL();
    return KNN_OK;
}

/* (no scratch for a few queries: the engine then allocates its 16-byte minimum) */
size_t knn_order_tmp_bytes(int nq) { return nq <= 512 ? 0 : (size_t)nq * 8; }

int knn_launch_order(const int *part_i, int nsplit, int lpq, int kl, int nq, int nq_pad, long long q_base, int rounds,
                     int *lab, int *keys, int *iota, int *perm, void *tmp, size_t tmp_bytes, void *stream)
{
    FALLIBLE("knn_launch_order", KNN_ERR_HIP);
    T("knn_launch_order"); B(part_i); I(nsplit); I(lpq); I(kl); I(nq); I(nq_pad); I(q_base); I(rounds); B(lab);
    B(keys); B(iota); B(perm); B(tmp); I((long long)tmp_bytes); S(stream); EOL();
    return KNN_OK;
}

int knn_launch_shadow(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, void *stream)
{
    FALLIBLE("knn_launch_shadow", KNN_ERR_HIP);
    T("knn_launch_shadow"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); S(stream); EOL();
    return KNN_OK;
}

int knn_launch_shadow8(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, const double *meta,
                       void *stream)
{
    FALLIBLE("knn_launch_shadow8", KNN_ERR_HIP);
    T("knn_launch_shadow8"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); B(meta); S(stream);
    EOL();
    return KNN_OK;
}

int knn_launch_shadow_split(void *dst, const void *blk, int dtype, size_t rows_pad, size_t n, float scale, void *stream)
{
    FALLIBLE("knn_launch_shadow_split", KNN_ERR_HIP);
    T("knn_launch_shadow_split"); B(dst); B(blk); I(dtype); I((long long)rows_pad); I((long long)n); F(scale); S(stream);
    EOL();
    return KNN_OK;
}

int knn_launch_shadow_split_n(int nblk, void *const *dst, const void *const *src, const size_t *rows_pad, int dtype,
                              size_t n, float scale, void *stream)
{
    FALLIBLE("knn_launch_shadow_split_n", KNN_ERR_HIP);
    T("knn_launch_shadow_split_n"); I(dtype); I((long long)n); F(scale); S(stream);
    A(" blocks %d", nblk);
    for (int b = 0; b < nblk; b++) {
        A(" [");
        B(dst[b]); B(src[b]); I((long long)rows_pad[b]);
        A(" ]");
    }
    EOL();
    return KNN_OK;
}

int knn_launch_gather8(void *dst, const void *src, const int *list, int cnt, size_t n, size_t src_rows_pad,
                       size_t dst_rows_pad, const double *src_qthr, double *dst_qthr, void *stream)
{
    FALLIBLE("knn_launch_gather8", KNN_ERR_HIP);
    T("knn_launch_gather8"); B(dst); B(src); B(list); I(cnt); I((long long)n); I((long long)src_rows_pad);
    I((long long)dst_rows_pad); B(src_qthr); B(dst_qthr); S(stream); EOL();
    need(dst, knn_s8_meta_offset(dst_rows_pad, n), "knn_launch_gather8");
    need(list, (size_t)cnt * sizeof(int), "knn_launch_gather8");
    need(dst_qthr, (size_t)cnt * sizeof(double), "knn_launch_gather8");
    return KNN_OK;
}

int knn_launch_resolve8(unsigned char *flag, const int *list, int cnt, const int *sub_fail, const int *sub_cnt,
                        const knn_neighbour_t *sub_out, int k, knn_neighbour_t *out, int *new_list, int *new_cnt,
                        void *stream)
{
    FALLIBLE("knn_launch_resolve8", KNN_ERR_HIP);
    T("knn_launch_resolve8"); B(flag); B(list); I(cnt); B(sub_fail); B(sub_cnt); B(sub_out); I(k); B(out); B(new_list);
    B(new_cnt); S(stream); A(" -> %d", g_unres2); EOL();
    need(flag, (size_t)cnt, "knn_launch_resolve8");
    need(sub_out, (size_t)cnt * (size_t)k * sizeof(*sub_out), "knn_launch_resolve8");
    need(new_list, (size_t)cnt * sizeof(int), "knn_launch_resolve8");
    new_cnt[0] = g_unres2;
    g_span_hi = g_calls + 2;   /* (the count's copy and its host wait end the re-search) */
    return KNN_OK;
}

int knn_launch_rescan_init(int kp, double *rs_d, int *rs_i, int nfail, void *stream)
{
    FALLIBLE("knn_launch_rescan_init", KNN_ERR_HIP);
    T("knn_launch_rescan_init"); I(kp); B(rs_d); B(rs_i); I(nfail); S(stream); EOL();
    const size_t sets = (size_t)nfail * (1 + (size_t)knn_rescan_chunks(nfail)) * (size_t)kp;
    need(rs_d, sets * sizeof(double), "knn_launch_rescan_init");
    need(rs_i, sets * sizeof(int), "knn_launch_rescan_init");
    return KNN_OK;
}

int knn_launch_rescan_step(int dtype, int kp, const int *fail_list, int nfail, const double *fbound, const void *qblk,
                           const void *cblk, size_t c_base, int nc, int n, int k, double *rs_d, int *rs_i,
                           long long self_base, void *stream)
{
    FALLIBLE("knn_launch_rescan_step", KNN_ERR_HIP);
    T("knn_launch_rescan_step"); I(dtype); I(kp); B(fail_list); I(nfail); B(fbound); B(qblk); B(cblk);
    I((long long)c_base); I(nc); I(n); I(k); B(rs_d); B(rs_i); I(self_base); S(stream); EOL();
    return KNN_OK;
}

int knn_launch_rescan_end(int kp, const int *fail_list, int nfail, const double *rs_d, const int *rs_i, int k,
                          knn_neighbour_t *out, void *stream)
{
    FALLIBLE("knn_launch_rescan_end", KNN_ERR_HIP);
    T("knn_launch_rescan_end"); I(kp); B(fail_list); I(nfail); B(rs_d); B(rs_i); I(k); B(out); S(stream); EOL();
    return KNN_OK;
}

/* the rest of the engine's imports: no scenario reaches them */
#define UNREACHED(name) DIE("unexpected " name)

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

#define ROWS 1024   /* rows of every block, and the context's queries */
#define K 10
#define MAXB 9
#define MAXOPS 24

enum { INT8, SCAN64, SPLIT32, H16 };   /* the contraction the meta selects */

/* the calls into the engine (META: the harness rewrites the meta doubles) */
enum { CREATE = 1, PROFILE, META, SET_ROWS, BEGIN, PACK, STEP, STEP_N, SSTEP, SSTEP_N, END, RSTEP, REND, RESEARCH, DESTROY };

typedef struct {
    int op;
    int a, b;            /* a block (and a count), rows, a mode, or the stream END gets */
    int unres, unres2;   /* END: the unresolved queries; END / RESEARCH: those behind the re-search */
} op_t;

typedef struct {
    const char *name;
    int mode, solo, n;
    size_t frows;        /* rows of the foreign blocks (0: ROWS) */
    const char *env;     /* set to 1 for the scenario */
    op_t ops[MAXOPS];    /* from behind the create up to the destroy */
} scn_t;

#define SEARCH6 {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = STEP, 2}, {.op = STEP, 3}, {.op = STEP, 4}, {.op = STEP, 5}, {.op = END}, {.op = DESTROY}
#define PACK8 {.op = PACK, 0}, {.op = PACK, 1}, {.op = PACK, 2}, {.op = PACK, 3}, {.op = PACK, 4}, {.op = PACK, 5}, {.op = PACK, 6}, {.op = PACK, 7}

static const scn_t g_scn[] = {
    /* the first ten also run with knn_ctx_profile on (NAME+prof) */
    {"solo1_i8", INT8, 1, 64, 0, NULL, {{.op = BEGIN}, {.op = STEP, 0}, {.op = END}, {.op = DESTROY}}},
    {"solo2_i8", INT8, 1, 64, 0, NULL, {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = DESTROY}}},
    {"solo1_end_other_stream", INT8, 1, 64, 0, NULL, {{.op = BEGIN}, {.op = STEP, 0}, {.op = END, 1}, {.op = DESTROY}}},
    /* element blocks converted for the int8 contraction (cs8) */
    {"six_i8", INT8, 0, 64, 0, NULL, {SEARCH6}},
    {"six_f64", SCAN64, 0, 64, 0, NULL, {SEARCH6}},
    /* The direct exchange: the own block, then every received block in one
     * fused step.  Two searches on one context: the first grows the pair's
     * lists under the pending own-block step (which is then merged alone), the
     * second -- a ring's steady state -- shares one merge between both. */
    {"shadow_own_then_7", INT8, 0, 64, 0, NULL,
     {{.op = BEGIN}, PACK8, {.op = SSTEP, 0}, {.op = SSTEP_N, 1, 7}, {.op = END}, {.op = BEGIN}, {.op = SSTEP, 0}, {.op = SSTEP_N, 1, 7}, {.op = END}, {.op = DESTROY}}},
    {"split_own_then_7", SPLIT32, 0, 64, 0, NULL,
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 7}, {.op = END}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 7}, {.op = END}, {.op = DESTROY}}},
    {"split_9", SPLIT32, 0, 64, 0, NULL, {{.op = BEGIN}, {.op = STEP_N, 1, 9}, {.op = END}, {.op = DESTROY}}},
    {"split_own_then_2", SPLIT32, 0, 64, ROWS / 2, NULL,
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 2}, {.op = END}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 2}, {.op = END}, {.op = DESTROY}}},
    {"solo_split_own_then_2", SPLIT32, 1, 64, ROWS / 2, NULL,
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 2}, {.op = END}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP_N, 1, 2}, {.op = END}, {.op = DESTROY}}},
#define NPROF 10
    /* 1024 rows of 2 x 12 lists, 384 rows of 4 x 16 (as many list entries a
     * split: the pair stays), 1024 rows of 4 x 16 (the pair is freed and grown) */
    {"set_rows", INT8, 0, 784, 0, NULL,
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = SET_ROWS, 384}, {.op = META, SCAN64}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END},
      {.op = SET_ROWS, 1024}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = DESTROY}}},
    /* element blocks converted to fp16 shadow rows (csh), to split rows (csp) */
    {"h16_own_then_1", H16, 0, 128, 0, NULL, {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = DESTROY}}},
    {"split_own_then_1", SPLIT32, 0, 128, 0, NULL, {{.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = DESTROY}}},
    /* a fused split step whose second call needs a larger cspm */
    {"split_grow", SPLIT32, 0, 128, 0, NULL,
     {{.op = BEGIN}, {.op = STEP_N, 1, 2}, {.op = END}, {.op = BEGIN}, {.op = STEP_N, 1, 3}, {.op = END}, {.op = DESTROY}}},
    /* the GEMM-mode merge's query order, grown with the rows (and the query
     * block's split rows with its capacity) */
    {"order_split", SPLIT32, 0, 128, 0, "KNN_ORDER",
     {{.op = SET_ROWS, 384}, {.op = BEGIN, 384}, {.op = STEP, 0}, {.op = STEP, 1}, {.op = END}, {.op = SET_ROWS, 1024}, {.op = BEGIN}, {.op = STEP, 0}, {.op = STEP, 1},
      {.op = END}, {.op = DESTROY}}},
    /* the int8 re-search: its sub-context made, used again, made larger */
    {"research8", INT8, 1, 128, 0, NULL,
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = END, 0, 0, 3, 0}, {.op = BEGIN}, {.op = STEP, 0}, {.op = END, 0, 0, 3, 0}, {.op = BEGIN}, {.op = STEP, 0},
      {.op = END, 0, 0, 200, 1}, {.op = RSTEP, 0}, {.op = REND}, {.op = DESTROY}}},
    /* the exact rescan's lists, grown */
    {"rescan", INT8, 1, 128, 0, "KNN_NO_RESEARCH8",
     {{.op = BEGIN}, {.op = STEP, 0}, {.op = END, 0, 0, 3, 0}, {.op = RSTEP, 0}, {.op = REND}, {.op = BEGIN}, {.op = STEP, 0}, {.op = END, 0, 0, 40, 0}, {.op = RSTEP, 0},
      {.op = REND}, {.op = DESTROY}}},
    /* a ring rank's re-search over the byte blocks it holds */
    {"research_blocks", INT8, 0, 128, 0, NULL,
     {{.op = BEGIN}, {.op = PACK, 0}, {.op = PACK, 1}, {.op = PACK, 2}, {.op = PACK, 3}, {.op = SSTEP, 0}, {.op = SSTEP_N, 1, 3}, {.op = END, 0, 0, 3, 0},
      {.op = RESEARCH, 1, 3, 0, 1}, {.op = RSTEP, 0}, {.op = REND}, {.op = BEGIN}, {.op = SSTEP, 0}, {.op = SSTEP_N, 1, 3}, {.op = END, 0, 0, 5, 0},
      {.op = RESEARCH, 1, 3, 0, 0}, {.op = DESTROY}}},
};
#define NSCN ((int)(sizeof(g_scn) / sizeof(g_scn[0])))

static const char *const op_name[] = {"",      "create", "profile",      "meta", "set_rows", "begin",  "shadow_pack", "step",
                                      "step",  "step",   "step",         "end",  "rescan_step", "rescan_end", "research_blocks",
                                      "destroy"};

typedef struct {
    const scn_t *sc;
    knn_ctx_t *c;
    int mode, dtype, prof;    /* prof: knn_ctx_profile is on */
    void *stream[2];          /* the caller's stream, and a second one */
    void *blk[1 + MAXB];      /* [0] the own (query) block, then foreign ones */
    void *sblk[1 + MAXB];     /* their byte blocks (INT8) */
    size_t nc[1 + MAXB], base[1 + MAXB];
    double *meta;
    knn_neighbour_t *out;
} run_t;

static int g_mismatch;   /* clean calls behind which knn_ctx_device_bytes was not the live bytes */

static void set_meta(run_t *r, int mode)
{
    double *m = r->meta;
    const double n = (double)r->sc->n;
    memset(m, 0, KNN_META_DOUBLES * sizeof(double));
    r->mode = mode;
    if (mode == INT8) {          /* integers in [0, 255] */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 255.0;
        m[KNN_META_MAXNORM] = 255.0 * 255.0 * n;
    } else if (mode == H16) {    /* integers in [-256, 256]: no byte window, exact in fp16 */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = m[KNN_META_MAXNEG] = 256.0;
        m[KNN_META_MAXNORM] = 256.0 * 256.0 * n;
    } else if (mode == SCAN64) { /* a non-finite value: no fast contraction */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 1.0;
        m[KNN_META_NONFINITE] = 1.0;
    } else {                     /* real values in [0, 1): the split fp16 filter */
        m[KNN_META_MAXABS] = m[KNN_META_MAXPOS] = 0.75;
        m[KNN_META_MAXNORM] = n;
        m[KNN_META_NONINT] = 1.0;
    }
}

/* the harness's own buffers and streams; nothing of the engine's */
static void run_open(run_t *r, const scn_t *sc)
{
    if (g_nlive || g_nevents) DIE("%s: something is live in front of it", sc->name);
    memset(g_ord, 0, sizeof(g_ord));
    memset(r, 0, sizeof(*r));
    r->sc = sc;
    r->dtype = sc->mode == SPLIT32 ? KNN_F32 : KNN_F64;
    r->stream[0] = live_new(1, 'S');
    r->stream[1] = live_new(1, 'S');
    const size_t frows = sc->frows ? sc->frows : ROWS;
    for (int b = 0; b <= MAXB; b++) {
        r->blk[b] = live_new(knn_block_bytes_dt(ROWS, (size_t)sc->n, r->dtype), 'U');
        r->sblk[b] = live_new(knn_s8_bytes(ROWS, (size_t)sc->n), 'U');
        r->nc[b] = b ? frows : ROWS;
        r->base[b] = b ? ROWS + (size_t)(b - 1) * frows : 0;
    }
    r->meta = (double *)((char *)r->blk[0] + knn_block_meta_offset_dt(ROWS, (size_t)sc->n, r->dtype));
    set_meta(r, sc->mode);
    r->out = (knn_neighbour_t *)live_new((size_t)ROWS * K * sizeof(knn_neighbour_t), 'U');
    if (sc->env) setenv(sc->env, "1", 1);
}

/* what is live behind the harness's own: nothing when the engine kept (e) */
static int run_shut(run_t *r)
{
    if (r->sc->env) unsetenv(r->sc->env);
    for (int i = g_nlive - 1; i >= 0; i--)
        if (g_live[i].kind == 'U') live_free(g_live[i].base, "run_shut");
    live_free(r->stream[0], "run_shut");
    live_free(r->stream[1], "run_shut");
    const int left = g_nlive + g_nevents;
    while (g_nlive) live_free(g_live[0].base, "run_shut");
    g_nevents = 0;
    return left;
}

/* one call into the engine */
static int run_op(run_t *r, const op_t *o)
{
    knn_ctx_t *c = r->c;
    const void *const *blk = (const void *const *)r->blk, *const *sblk = (const void *const *)r->sblk;
    void *s = r->stream[0];
    size_t unres = 0;
    int rc = KNN_OK;
    if (o->op != META) L("# %s", op_name[o->op]);
    g_span_lo = o->op == RESEARCH;
    g_span_hi = 0;
    switch (o->op) {
    case CREATE:
        rc = knn_ctx_create_dt(&r->c, 0, ROWS, (size_t)r->sc->n, ROWS, K, r->dtype);
        if (!rc) rc = knn_ctx_set_solo(r->c, r->sc->solo);
        break;
    case PROFILE:
        rc = knn_ctx_profile(c, 1, NULL, NULL, NULL);
        r->prof = !rc;
        break;
    case META: set_meta(r, o->a); break;
    case SET_ROWS: rc = knn_ctx_set_rows(c, (size_t)o->a); break;
    case BEGIN:
        rc = knn_ctx_begin(c, r->blk[0], o->a ? (size_t)o->a : ROWS, 0, r->meta, s);
        if (!rc) {
            const int want = r->mode == INT8 ? 8 : (r->mode == SCAN64 ? 64 : 16);
            if (knn_ctx_contraction_bits(c) != want || knn_ctx_split(c) != (r->mode == SPLIT32))
                DIE("%s: the meta selected another contraction", r->sc->name);
        }
        break;
    case PACK:
        if (knn_ctx_shadow_bytes(c, ROWS) != knn_s8_bytes(ROWS, (size_t)r->sc->n)) DIE("%s: no byte blocks", r->sc->name);
        rc = knn_ctx_shadow_pack(c, r->sblk[o->a], r->blk[o->a], ROWS, s);
        break;
    case STEP: rc = knn_ctx_step(c, r->blk[o->a], r->nc[o->a], r->base[o->a], s); break;
    case STEP_N: rc = knn_ctx_step_n(c, o->b, blk + o->a, r->nc + o->a, r->base + o->a, s); break;
    case SSTEP: rc = knn_ctx_step_shadow(c, r->sblk[o->a], r->nc[o->a], r->base[o->a], s); break;
    case SSTEP_N: rc = knn_ctx_step_shadow_n(c, o->b, sblk + o->a, r->nc + o->a, r->base + o->a, s); break;
    case END:
        g_unres = o->unres;
        g_unres2 = o->unres2;
        rc = knn_ctx_end(c, r->out, &unres, r->stream[o->a]);
        if (!rc) L("# unresolved %zu", unres);
        if (!rc && r->prof) {
            int merges = 0, launches = 0;
            knn_ctx_profile(c, -1, NULL, NULL, &launches);
            knn_ctx_profile_merge(c, NULL, &merges, NULL);
            L("# profiled steps %d merges %d", launches, merges);
        }
        break;
    case RSTEP: rc = knn_ctx_rescan_step(c, r->blk[o->a], r->nc[o->a], r->base[o->a], s); break;
    case REND: rc = knn_ctx_rescan_end(c, r->out, s); break;
    case RESEARCH:
        g_unres2 = o->unres2;
        rc = knn_ctx_research_blocks(c, o->b, sblk + o->a, r->nc + o->a, r->base + o->a, r->out, &unres, s);
        if (!rc) L("# unresolved %zu", unres);
        break;
    default:
        rc = knn_ctx_destroy(c);
        r->c = NULL;
    }
    if (rc) L("# -> %d", rc);
    else if (o->op != META) L("# live %zu", live_bytes('A'));
    return rc;
}

/* the scenario's calls, a profile behind the create when asked for */
static int scn_ops(const scn_t *sc, int prof, op_t *ops)
{
    int n = 0;
    ops[n++] = (op_t){CREATE, 0, 0, 0, 0};
    if (prof) ops[n++] = (op_t){PROFILE, 0, 0, 0, 0};
    for (int i = 0; i == 0 || sc->ops[i - 1].op != DESTROY; i++) ops[n++] = sc->ops[i];
    return n;
}

/* (c): the context accounts for the device bytes that are live */
static int bytes_ok(const run_t *r) { return !r->c || knn_ctx_device_bytes(r->c) == live_bytes('A'); }

/* The lines so far, to stdout.  Events created or destroyed one after the
 * other (knn_ctx_profile's 320) take one line: "hipEventCreate E11 .. E330". */
static void print_lines(void)
{
    for (int i = 0; i < g_nline;) {
        static const char *const run[] = {"hipEventCreate E", "hipEventDestroy E"};
        int j = i + 1;
        for (int k = 0; k < 2; k++) {
            const size_t len = strlen(run[k]);
            if (strncmp(g_line[i], run[k], len)) continue;
            const int e0 = atoi(g_line[i] + len);
            char next[64];
            for (;; j++) {
                snprintf(next, sizeof(next), "%s%d", run[k], e0 + j - i);
                if (j == g_nline || strcmp(g_line[j], next)) break;
            }
            if (j - i >= 3) printf("%s .. E%d\n", g_line[i], e0 + j - i - 1);
            else j = i + 1;
        }
        if (j == i + 1) puts(g_line[i]);
        i = j;
    }
    lines_clear();
}

static void trace(const scn_t *sc, int prof)
{
    run_t r;
    op_t ops[MAXOPS + 2];
    const int nops = scn_ops(sc, prof, ops);
    run_open(&r, sc);
    printf("## %s%s\n", sc->name, prof ? "+prof" : "");
    for (int i = 0; i < nops; i++) {
        if (run_op(&r, &ops[i])) DIE("%s: call %d failed", sc->name, i);
        print_lines();
        if (!bytes_ok(&r)) {
            fprintf(stderr, "MISMATCH %s%s call %d (%s): %zu bytes live, knn_ctx_device_bytes %zu\n", sc->name,
                    prof ? "+prof" : "", i, op_name[ops[i].op], live_bytes('A'), knn_ctx_device_bytes(r.c));
            g_mismatch++;
        }
    }
    if (run_shut(&r)) DIE("%s: something is live behind it", sc->name);
}

/* ---- the sweep ---------------------------------------------------------- */

static int g_violations, g_warm[4], g_nabsorbed;   /* g_warm: by the reference (d) met, [0] the fresh context's */

static void violation(const scn_t *sc, int prof, int call, const op_t *o, long n, const char *what)
{
    printf("VIOLATION %s%s call %d (%s) fault %ld: %s\n", sc->name, prof ? "+prof" : "", call, op_name[o->op], n, what);
    g_violations++;
}

/* the lines (d) compares, as tail_of gives them */
static char *search_lines(void)
{
    static const char *const aside[] = {"hipHostMalloc", "hipHostFree", "hipStreamCreate", "hipStreamDestroy",
                                        "hipEventCreate", "hipEventDestroy", "hipSetDevice", "hipEventElapsedTime", "!"};
    char **keep = (char **)malloc((size_t)(g_nline + 1) * sizeof(char *));
    int n = 0, cnt = 0;
    for (int i = 0; i < g_nline; i++) {
        int drop = 0;
        for (size_t a = 0; a < sizeof(aside) / sizeof(aside[0]); a++) drop |= starts(g_line[i], aside[a]);
        /* the host wait a buffer is freed or grown behind -- never one for a
         * result, which stands right behind the copy or launch that delivers it */
        if ((starts(g_line[i], "hipStreamSynchronize") || starts(g_line[i], "hipDeviceSynchronize")) && i + 1 < g_nline &&
            !(i > 0 && (starts(g_line[i - 1], "hipMemcpyAsync") || starts(g_line[i - 1], "knn_launch_count_out"))))
            drop |= starts(g_line[i + 1], "hipMalloc") || starts(g_line[i + 1], "hipFree");
        if (!drop) keep[n++] = g_line[i];
    }
    char *out = tail_of(keep, n, 0, &cnt);
    free(keep);
    return out;
}

/* The scenario's first search: its calls from behind the create (and the
 * profile) up to its first end and the rescan calls behind that, on a
 * context put back to the scenario's first rows and meta. */
static int first_search(run_t *r, const op_t *ops, int nops)
{
    int i = 1 + (ops[1].op == PROFILE), ended = 0;
    set_meta(r, r->sc->mode);
    if (knn_ctx_set_rows(r->c, ROWS)) return KNN_ERR_INVALID;
    lines_clear();
    for (; i < nops && ops[i].op != DESTROY; i++) {
        if (ended && ops[i].op != RSTEP && ops[i].op != REND && ops[i].op != RESEARCH) break;
        ended |= ops[i].op == END;
        const int rc = run_op(r, &ops[i]);
        if (rc) return rc;
    }
    return KNN_OK;
}

/* that search's lines on a fresh context ([0]) and run once more ([1]) */
static void references(const scn_t *sc, int prof, char *ref[2])
{
    run_t r;
    op_t ops[MAXOPS + 2];
    const int nops = scn_ops(sc, prof, ops);
    run_open(&r, sc);
    for (int i = 0; i < 1 + prof; i++)
        if (run_op(&r, &ops[i])) DIE("%s: call %d failed", sc->name, i);
    for (int pass = 0; pass < 2; pass++) {
        if (first_search(&r, ops, nops)) DIE("%s: the first search failed", sc->name);
        ref[pass] = search_lines();
    }
    knn_ctx_destroy(r.c);
    lines_clear();
    if (run_shut(&r)) DIE("%s: something is live behind it", sc->name);
}

static void sweep_scn(const scn_t *sc, int prof, long *faults, int *calls)
{
    op_t ops[MAXOPS + 2];
    const int nops = scn_ops(sc, prof, ops);
    char *ref[2][2];   /* [profile on][fresh, once more] */
    references(sc, 0, ref[0]);
    references(sc, prof, ref[1]);
    for (int call = 0; call < nops; call++) {
        const op_t *o = &ops[call];
        if (o->op == META) continue;
        ++*calls;
        long count = 0, span_lo = 0, span_hi = 0;
        char *grown[2] = {NULL, NULL};   /* the first search behind the clean calls in front of this one, and behind it */
        /* n = 0: the clean run that counts; -1: one that stops in front of the
         * call; -2: one that is destroyed there, as it stands */
        for (long n = -2; n <= count; n++) {
            run_t r;
            run_open(&r, sc);
            for (int i = 0; i < call; i++)
                if (run_op(&r, &ops[i])) DIE("%s: call %d failed", sc->name, i);
            if (n < 0) {
                if (n == -1 && r.c && !first_search(&r, ops, nops)) grown[0] = search_lines();
                g_bad_free = 0;
                if (r.c) knn_ctx_destroy(r.c);
                lines_clear();
                if (run_shut(&r) || g_bad_free) violation(sc, prof, call, o, n, "(e) knn_ctx_destroy in front of the call left something live");
                continue;
            }
            lines_clear();
            g_calls = g_bad_free = g_absorbed = 0;
            g_abs_lo = g_abs_hi = 0;
            if (n > 0) g_abs_lo = span_lo, g_abs_hi = span_hi;
            g_fail_at = n;
            const int rc = run_op(&r, o);
            g_fail_at = 0;
            if (n == 0) {
                if (rc) DIE("%s: call %d failed", sc->name, call);
                count = g_calls;
                span_lo = g_span_hi ? g_span_lo : 0;
                span_hi = g_span_hi;
                if (!bytes_ok(&r)) violation(sc, prof, call, o, n, "(c) a clean call left other bytes live than accounted for");
                if (r.c && !first_search(&r, ops, nops)) grown[1] = search_lines();
            } else {
                ++*faults;
                if (!rc && g_absorbed) g_nabsorbed++;
                else if (!rc) violation(sc, prof, call, o, n, "(a) the call succeeded");
                if (o->op == CREATE && rc) r.c = NULL;
                if (g_bad_free) violation(sc, prof, call, o, n, "(b) a pointer was freed that is not live");
                if (!bytes_ok(&r)) violation(sc, prof, call, o, n, "(c) live device bytes are not what the context accounts for");
                if (r.c && o->op != DESTROY) {
                    if (first_search(&r, ops, nops)) {
                        violation(sc, prof, call, o, n, "(d) a new search failed");
                    } else {
                        char *got = search_lines();
                        const char *const refs[4] = {ref[r.prof][0], ref[r.prof][1], grown[0], grown[1]};
                        int met = -1;
                        for (int q = 3; q >= 0; q--)
                            if (refs[q] && !strcmp(got, refs[q])) met = q;
                        if (met < 0) violation(sc, prof, call, o, n, "(d) a new search's trace differs");
                        else g_warm[met]++;
                        free(got);
                        if (!bytes_ok(&r)) violation(sc, prof, call, o, n, "(c) live device bytes differ behind the new search");
                    }
                }
            }
            g_bad_free = 0;
            if (r.c) knn_ctx_destroy(r.c);
            if (g_bad_free) violation(sc, prof, call, o, n, "(b) knn_ctx_destroy freed a pointer that is not live");
            lines_clear();
            if (run_shut(&r)) violation(sc, prof, call, o, n, "(e) something is live behind knn_ctx_destroy");
        }
        free(grown[0]);
        free(grown[1]);
    }
    for (int i = 0; i < 4; i++) free(ref[i / 2][i % 2]);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--sweep")) {
        long faults = 0;
        int calls = 0;
        for (int i = 0; i < NSCN; i++)
            for (int prof = 0; prof <= (i < NPROF); prof++) sweep_scn(&g_scn[i], prof, &faults, &calls);
        printf("(d) met by the first search on a fresh context %d times, run again there %d, behind the clean calls in front "
               "of the failed one %d, behind them and it %d\n", g_warm[0], g_warm[1], g_warm[2], g_warm[3]);
        printf("sweep: %d calls, %ld faults, %d absorbed, %d warm, %d violations\n", calls, faults, g_nabsorbed,
               g_warm[1] + g_warm[2] + g_warm[3], g_violations);
        return g_violations != 0;
    }
    for (int prof = 0; prof < 2; prof++)
        for (int i = 0; i < (prof ? NPROF : NSCN); i++) {
            char full[64];
            snprintf(full, sizeof(full), "%s%s", g_scn[i].name, prof ? "+prof" : "");
            int wanted = argc < 2;
            for (int a = 1; a < argc; a++) wanted |= !strcmp(argv[a], full);
            if (wanted) trace(&g_scn[i], prof);
        }
    return g_mismatch != 0;
}
