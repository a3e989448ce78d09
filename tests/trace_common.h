/*
 * trace_common.h -- what the CPU trace programs share (index_trace.c,
 * engine_trace.c): the line buffer, the live set, the fault knob, the plain
 * HIP stubs and the comparison of two traces.  Included once by a program,
 * which may define in front of it:
 *
 *   TRACE_PROG            its name in messages (a string literal; required)
 *   FAULT_HOOK()          run when the fault fires
 *   FALLIBLE_ORDER        defined: event creation, records and host waits
 *                         count as fallible calls too
 *   LIVE_BAD_FREE(who)    a free of a pointer that is not live (default: the
 *                         program ends)
 *   TRACE_NAME_KINDS      the kinds whose names tail_of numbers in order of
 *                         appearance (default "APE")
 *
 * hipMalloc returns zeroed host memory, entered in a live set under an ordinal
 * name (A1, A2, ...; pinned memory P, and whatever kinds the program adds
 * with live_new); events are E1, E2, ....  The copies and memsets copy and
 * set, checked against the live set.  Every stub appends one line to the
 * trace: its name and its arguments, pointers as name+offset ("H": host
 * memory, "0": NULL).
 */
#ifndef TRACE_COMMON_H
#define TRACE_COMMON_H

#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define DIE(...)                                  \
    do {                                          \
        fprintf(stderr, TRACE_PROG ": " __VA_ARGS__); \
        fprintf(stderr, "\n");                    \
        exit(2);                                  \
    } while (0)

/* ---- the trace ---------------------------------------------------------- */

#define MAX_LINES 8192
static char *g_line[MAX_LINES];
static int g_nline, g_echo;

static void L(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (g_echo) puts(buf);
    if (g_nline == MAX_LINES) DIE("trace too long");
    if (!(g_line[g_nline++] = strdup(buf))) DIE("out of memory");
}

static void lines_clear(void)
{
    for (int i = 0; i < g_nline; i++) free(g_line[i]);
    g_nline = 0;
}

/* ---- the live set ------------------------------------------------------- */

#define MAX_LIVE 1024
static struct {
    char *base;
    size_t size;
    int ord;
    char kind;   /* A: hipMalloc, P: hipHostMalloc, others: the program's own */
} g_live[MAX_LIVE];
static int g_nlive, g_ord[128];

static int live_find(const void *p)
{
    for (int i = 0; i < g_nlive; i++)
        if ((const char *)p >= g_live[i].base && (const char *)p < g_live[i].base + g_live[i].size) return i;
    return -1;
}

static void *live_new(size_t size, char kind)
{
    if (g_nlive == MAX_LIVE) DIE("live set full");
    char *p = (char *)calloc(size ? size : 1, 1);
    if (!p) DIE("out of memory");
    g_live[g_nlive].base = p;
    g_live[g_nlive].size = size ? size : 1;
    g_live[g_nlive].ord = ++g_ord[(int)kind];
    g_live[g_nlive++].kind = kind;
    return p;
}

#ifndef LIVE_BAD_FREE
#define LIVE_BAD_FREE(who) DIE("%s of a pointer that is not live", who)
#endif

static void live_free(void *p, const char *who)
{
    const int i = live_find(p);
    if (i < 0 || g_live[i].base != (char *)p) {
        LIVE_BAD_FREE(who);
        return;
    }
    free(p);
    g_live[i] = g_live[--g_nlive];
}

static size_t live_bytes(char kind)
{
    size_t b = 0;
    for (int i = 0; i < g_nlive; i++)
        if (g_live[i].kind == kind) b += g_live[i].size;
    return b;
}

/* a pointer's name (up to 8 of them in one line) */
static const char *N(const void *p)
{
    static char buf[8][48];
    static int at;
    char *s = buf[at++ % 8];
    const int i = p ? live_find(p) : -1;
    if (!p) return "0";
    if (i < 0) return "H";
    const size_t off = (size_t)((const char *)p - g_live[i].base);
    if (off) snprintf(s, 48, "%c%d+%zu", g_live[i].kind, g_live[i].ord, off);
    else snprintf(s, 48, "%c%d", g_live[i].kind, g_live[i].ord);
    return s;
}

/* [p, p + bytes) lies in one live allocation */
static void need(const void *p, size_t bytes, const char *who)
{
    const int i = p ? live_find(p) : -1;
    if (i < 0 || (const char *)p + bytes > g_live[i].base + g_live[i].size)
        DIE("%s: %zu bytes at %s are not inside a live allocation", who, bytes, N(p));
}

/* ---- the fault knob ----------------------------------------------------- */

static long g_calls, g_fail_at;

#ifndef FAULT_HOOK
#define FAULT_HOOK() ((void)0)
#endif

#define FALLIBLE(name, err)                           \
    do {                                              \
        if (++g_calls == g_fail_at) {                 \
            FAULT_HOOK();                             \
            L("! %s", name);                          \
            return err;                               \
        }                                             \
    } while (0)

#ifdef FALLIBLE_ORDER
#define ORDER_FALLIBLE(name, err) FALLIBLE(name, err)
#else
#define ORDER_FALLIBLE(name, err) ((void)0)
#endif

/* ---- HIP ---------------------------------------------------------------- */

static int g_nevents;

hipError_t hipSetDevice(int d) { L("hipSetDevice %d", d); return hipSuccess; }

hipError_t hipMalloc(void **p, size_t size)
{
    FALLIBLE("hipMalloc", hipErrorOutOfMemory);
    *p = live_new(size, 'A');
    L("hipMalloc %s %zu", N(*p), size);
    return hipSuccess;
}

hipError_t hipFree(void *p)
{
    if (!p) return hipSuccess;
    L("hipFree %s", N(p));
    live_free(p, "hipFree");
    return hipSuccess;
}

hipError_t hipHostMalloc(void **p, size_t size, unsigned int flags)
{
    (void)flags;
    FALLIBLE("hipHostMalloc", hipErrorOutOfMemory);
    *p = live_new(size, 'P');
    L("hipHostMalloc %s %zu", N(*p), size);
    return hipSuccess;
}

hipError_t hipHostFree(void *p)
{
    L("hipHostFree %s", N(p));
    live_free(p, "hipHostFree");
    return hipSuccess;
}

static void copy(const char *who, void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    if (kind != hipMemcpyDeviceToHost) need(dst, n, who);
    if (kind != hipMemcpyHostToDevice) need(src, n, who);
    memmove(dst, src, n);
}

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    FALLIBLE("hipMemcpy", hipErrorInvalidValue);
    L("hipMemcpy %s %s %zu %d", N(dst), N(src), n, (int)kind);
    copy("hipMemcpy", dst, src, n, kind);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    FALLIBLE("hipMemcpyAsync", hipErrorInvalidValue);
    L("hipMemcpyAsync %s %s %zu %d %s", N(dst), N(src), n, (int)kind, N(s));
    copy("hipMemcpyAsync", dst, src, n, kind);
    return hipSuccess;
}

hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s)
{
    FALLIBLE("hipMemsetAsync", hipErrorInvalidValue);
    L("hipMemsetAsync %s %d %zu %s", N(dst), v, n, N(s));
    need(dst, n, "hipMemsetAsync");
    memset(dst, v, n);
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s)
{
    ORDER_FALLIBLE("hipStreamSynchronize", hipErrorUnknown);
    L("hipStreamSynchronize %s", N(s));
    return hipSuccess;
}

/* an event: its ordinal */
static const char *EV(hipEvent_t e)
{
    static char buf[4][16];
    static int at;
    char *s = buf[at++ % 4];
    snprintf(s, 16, "E%d", *(int *)e);
    return s;
}

hipError_t hipEventCreate(hipEvent_t *e)
{
    ORDER_FALLIBLE("hipEventCreate", hipErrorOutOfMemory);
    int *p = (int *)malloc(sizeof(int));
    if (!p) DIE("out of memory");
    *p = ++g_ord['E'];
    g_nevents++;
    *e = (hipEvent_t)p;
    L("hipEventCreate %s", EV(*e));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { L("hipEventDestroy %s", EV(e)); free(e); g_nevents--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    ORDER_FALLIBLE("hipEventRecord", hipErrorUnknown);
    L("hipEventRecord %s %s", EV(e), N(s));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    ORDER_FALLIBLE("hipEventSynchronize", hipErrorUnknown);
    L("hipEventSynchronize %s", EV(e));
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    L("hipEventElapsedTime %s %s", EV(a), EV(b));
    *ms = 0.f;
    return hipSuccess;
}

/* ---- two traces compared ------------------------------------------------ */

static int starts(const char *s, const char *p) { return !strncmp(s, p, strlen(p)); }

#ifndef TRACE_NAME_KINDS
#define TRACE_NAME_KINDS "APE"
#endif

/* The lines from the first enqueue on, without marks and allocations, as one
 * string, the last `keep` of them (0: all) with their names numbered in
 * order of appearance.  *cnt: how many lines there are. */
static char *tail_of(char **line, int nline, int keep, int *cnt)
{
    static const char *const first[] = {"hipEventRecord", "hipMemcpyAsync", "hipMemsetAsync", "knn_launch_", "knn_block_"};
    int at = nline, n = 0;
    for (int i = 0; i < nline && at == nline; i++)
        for (size_t f = 0; f < sizeof(first) / sizeof(first[0]); f++)
            if (starts(line[i], first[f])) at = i;
    int *sel = (int *)malloc((size_t)(nline + 1) * sizeof(int));
    size_t len = 1;
    for (int i = at; i < nline; i++)
        if (line[i][0] != '#' && !starts(line[i], "hipMalloc") && !starts(line[i], "hipFree")) {
            sel[n++] = i;
            len += strlen(line[i]) + 1;
        }
    *cnt = n;
    char *out = (char *)calloc(3 * len + 16, 1), *o = out;   /* (a name grows by a character or two) */
    char seen[256][16];
    int nseen = 0;
    for (int j = keep && keep < n ? n - keep : 0; j < n; j++) {
        for (const char *p = line[sel[j]]; *p;) {
            const int name = (p == line[sel[j]] || p[-1] == ' ') && strchr(TRACE_NAME_KINDS, *p) && p[1] >= '0' && p[1] <= '9';
            if (!name) {
                *o++ = *p++;
                continue;
            }
            char tok[16] = {*p++};
            int tl = 1, id = -1;
            while (*p >= '0' && *p <= '9' && tl < 15) tok[tl++] = *p++;
            for (int q = 0; q < nseen; q++)
                if (!strcmp(seen[q], tok)) id = q;
            if (id < 0 && nseen < 256) strcpy(seen[id = nseen++], tok);
            o += sprintf(o, "%c#%d", tok[0], id);
        }
        *o++ = '\n';
    }
    free(sel);
    return out;
}

#endif
