"""mpiknn -- Python host mirror of libknn (include/knn.h) over ctypes.

The product is the C-ABI library ``mpi-knn_amd/lib/libknn.so`` (HIP kernels
for gfx950 + a C host engine).  This module only binds it: numpy arrays for
the host API, raw device pointers (e.g. ``torch.Tensor.data_ptr()``) for the
device-resident API used by the per-rank RCCL ring (``mpiknn.ring``) and by
bench.py.  There is no CPU fallback: if the library is missing, importing
this module raises.

Reference (yiapou13/mpi-knn): serial:L = knn-serial.c,
blk:L = mpi-knn-parallel_blocking.c, nb:L = mpi-knn-parallel_non_blocking.c.
"""
import atexit
import collections
import ctypes
import os
import sys
import weakref

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (KNN_LIB_PATH: another build of the same library, for A/B timing runs)
LIB_PATH = os.environ.get("KNN_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libknn.so")

# knn_neighbour_t (blk:15-20): {double distance; int32 idx (1-based); int32 label}
NB_DTYPE = np.dtype([("distance", "<f8"), ("idx", "<i4"), ("label", "<i4")])

OK, ERR_INVALID, ERR_NOMEM, ERR_HIP, ERR_IO, ERR_FORMAT, ERR_UNSUPPORTED, ERR_NODEVICE, ERR_RCCL = range(9)
COLMAJOR, ROWMAJOR = 0, 1
F64, F32, U8 = 0, 1, 2
VOTE_SERIAL, VOTE_MPI, VOTE_MAJORITY = 0, 1, 2
WEIGHT_UNIFORM, WEIGHT_DISTANCE = 0, 1   # enum knn_weights
MAX_K = 32          # KNN_MAX_K (fp64)
MAX_K_F32 = 128     # KNN_MAX_K_F32
META_DOUBLES = 8
STEP_LAG = 2        # KNN_STEP_LAG: a ring rotates STEP_LAG + 2 receive buffers
MODE_NAMES = {0: "int-exact", 1: "gemm+rerank", 2: "exact-scan"}

# every symbol include/knn.h declares (checked by tests/test_abi.py)
API_SYMBOLS = (
    "knn_strerror", "knn_load_mat", "knn_free", "knn_search", "knn_last_search_seconds",
    "knn_classify", "knn_block_bytes", "knn_block_meta_offset", "knn_block_pack",
    "knn_ctx_create", "knn_ctx_destroy", "knn_ctx_begin", "knn_ctx_step", "knn_ctx_end",
    "knn_ctx_rescan_step", "knn_ctx_rescan_end", "knn_search_packed", "knn_ctx_info",
    "knn_ctx_profile", "knn_block_bytes_dt", "knn_block_meta_offset_dt", "knn_block_pack_dt",
    "knn_ctx_create_dt", "knn_classify_device", "knn_search_mpi_compat",
    "knn_ctx_contraction_bits", "knn_wire_bytes", "knn_wire_ok", "knn_wire_pack",
    "knn_wire_unpack", "knn_shadow_bytes", "knn_shadow_norm_offset", "knn_shadow_pack", "knn_split_bytes", "knn_split_pack",
    "knn_ctx_shadow", "knn_ctx_step_shadow", "knn_ctx_begin_meta", "knn_ctx_shadow_bytes",
    "knn_ctx_shadow_pack", "knn_ctx_step_shadow_n", "knn_ctx_split", "knn_s8_block_bytes",
    "knn_s8_block_meta_offset", "knn_block_pack_s8", "knn_s8_spec_ok", "knn_ctx_begin_s8",
    "knn_ctx_attach_qblock", "knn_ctx_research_blocks", "knn_ctx_step_n", "knn_ctx_profile_merge",
    "knn_ctx_set_solo", "knn_ctx_search_meta", "knn_query", "knn_classify_query", "knn_ctx_set_keep_zero",
    "knn_index_create", "knn_index_query", "knn_index_info", "knn_index_destroy",
    "knn_index_add", "knn_block_append_dt", "knn_block_append_s8",
    "knn_index_remove", "knn_index_last_id", "knn_block_gather_dt", "knn_block_gather_s8",
    "knn_index_update", "knn_block_scatter_dt", "knn_block_scatter_s8",
    "knn_index_neighbours", "knn_block_gather_pos_dt", "knn_block_gather_pos_s8",
    "knn_index_classify", "knn_index_classify_rows",
    "knn_classify_weighted", "knn_regress", "knn_index_classify_weighted", "knn_index_classify_weighted_rows",
    "knn_index_regress", "knn_index_regress_rows",
    "knn_index_radius_count", "knn_index_radius", "knn_index_radius_rows_count", "knn_index_radius_rows",
    "knn_index_dbscan", "knn_dbscan_graph",
)
DTYPES = {"f64": F64, "f32": F32, F64: F64, F32: F32}
# a pack / index SOURCE may also be unsigned bytes (KNN_U8: never a block or search dtype)
SRC_DTYPES = dict(DTYPES)
SRC_DTYPES.update({"u8": U8, U8: U8})


class KnnError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__("%s: %s (status %d)" % (what, strerror(status), status))


def _share_torch_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own
    libamdhip64/librccl with the same sonames as /opt/rocm's; if libknn
    pulled in the system copies first, torch would later load a second HIP
    runtime (no GPU found, heap corruption at exit).  Importing torch first
    (no device is touched) makes libknn bind to torch's copies; without
    torch the system ROCm libraries are used."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libknn not built: %s missing (run `make -C mpi-knn_amd` or "
                          "__graft_entry__.build())" % LIB_PATH)
    _share_torch_runtime()
    L = ctypes.CDLL(LIB_PATH)
    p, sz, i, d = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    pp = ctypes.POINTER(ctypes.c_void_p)
    psz = ctypes.POINTER(ctypes.c_size_t)
    sig = {
        "knn_strerror": ([i], ctypes.c_char_p),
        "knn_load_mat": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, pp, psz, psz, pp, psz], i),
        "knn_free": ([p], None),
        "knn_search": ([p, sz, sz, i, p, i, i, i, p], i),
        "knn_search_mpi_compat": ([p, sz, sz, i, p, i, i, p], i),
        "knn_last_search_seconds": ([], d),
        "knn_classify": ([p, sz, i, i, i, p, p, psz], i),
        "knn_block_bytes": ([sz, sz], sz),
        "knn_block_meta_offset": ([sz, sz], sz),
        "knn_block_pack": ([p, sz, sz, sz, p, sz, i, p], i),
        "knn_ctx_create": ([pp, i, sz, sz, sz, i], i),
        "knn_block_bytes_dt": ([sz, sz, i], sz),
        "knn_block_meta_offset_dt": ([sz, sz, i], sz),
        "knn_block_pack_dt": ([p, i, sz, sz, sz, p, i, sz, i, p], i),
        "knn_ctx_create_dt": ([pp, i, sz, sz, sz, i, i], i),
        "knn_ctx_destroy": ([p], i),
        "knn_classify_device": ([p, sz, i, i, i, p, sz, sz, p, p, p], i),
        "knn_ctx_begin": ([p, p, sz, sz, p, p], i),
        "knn_ctx_begin_meta": ([p, p, sz, sz, p, p, p], i),
        "knn_ctx_shadow_bytes": ([p, sz], sz),
        "knn_ctx_shadow_pack": ([p, p, p, sz, p], i),
        "knn_ctx_step": ([p, p, sz, sz, p], i),
        "knn_ctx_end": ([p, p, psz, p], i),
        "knn_ctx_rescan_step": ([p, p, sz, sz, p], i),
        "knn_ctx_rescan_end": ([p, p, p], i),
        "knn_search_packed": ([p, p, sz, p, p], i),
        "knn_ctx_info": ([p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], i),
        "knn_ctx_contraction_bits": ([p], i),
        "knn_ctx_split": ([p], i),
        "knn_wire_bytes": ([sz, sz, i], sz),
        "knn_wire_ok": ([p], i),
        "knn_wire_pack": ([p, p, sz, sz, i, p], i),
        "knn_wire_unpack": ([p, p, sz, sz, i, p], i),
        "knn_shadow_bytes": ([sz, sz, i], sz),
        "knn_shadow_norm_offset": ([sz, sz], sz),
        "knn_shadow_pack": ([p, p, sz, sz, i, p], i),
        "knn_split_bytes": ([sz, sz], sz),
        "knn_split_pack": ([p, p, sz, sz, i, ctypes.c_double, p], i),
        "knn_ctx_shadow": ([p], i),
        "knn_ctx_step_shadow": ([p, p, sz, sz, p], i),
        "knn_ctx_step_shadow_n": ([p, i, pp, psz, psz, p], i),
        "knn_ctx_profile": ([p, i, ctypes.POINTER(d), ctypes.POINTER(d), ctypes.POINTER(i)], i),
        "knn_ctx_profile_merge": ([p, ctypes.POINTER(d), ctypes.POINTER(i), ctypes.POINTER(d)], i),
        "knn_ctx_set_solo": ([p, i], i),
        "knn_ctx_search_meta": ([p, ctypes.POINTER(d)], i),
        "knn_s8_block_bytes": ([sz, sz], sz),
        "knn_s8_block_meta_offset": ([sz, sz], sz),
        "knn_block_pack_s8": ([p, i, sz, sz, sz, p, i, sz, i, p], i),
        "knn_s8_spec_ok": ([p, sz, i], i),
        "knn_ctx_begin_s8": ([p, p, sz, sz, p, p, p], i),
        "knn_ctx_attach_qblock": ([p, p, sz], i),
        "knn_ctx_research_blocks": ([p, i, pp, psz, psz, p, psz, p], i),
        "knn_ctx_step_n": ([p, i, pp, psz, psz, p], i),
        "knn_query": ([p, sz, p, sz, sz, i, p, i, i, i, p], i),
        "knn_classify_query": ([p, sz, i, i, i, p, sz, p, p, psz], i),
        "knn_ctx_set_keep_zero": ([p, i], i),
        "knn_index_create": ([pp, p, sz, sz, i, i, p, i, i], i),
        "knn_index_query": ([p, p, sz, i, i, i, i, p], i),
        "knn_index_info": ([p, psz, psz, ctypes.POINTER(i), psz, ctypes.POINTER(i)], i),
        "knn_index_destroy": ([p], i),
        "knn_index_add": ([p, p, sz, i, i, p, i], i),
        "knn_block_append_dt": ([p, i, sz, sz, sz, sz, p, i, sz, i, p], i),
        "knn_block_append_s8": ([p, i, sz, sz, sz, sz, p, i, sz, i, p], i),
        "knn_index_remove": ([p, p, sz, i, psz], i),
        "knn_index_last_id": ([p, psz], i),
        "knn_block_gather_dt": ([p, sz, sz, p, sz, p, sz, sz, i, p], i),
        "knn_block_gather_s8": ([p, sz, sz, p, sz, p, sz, sz, p], i),
        "knn_index_update": ([p, p, sz, p, i, i, p, i], i),
        "knn_block_scatter_dt": ([p, i, sz, p, p, sz, sz, p, sz, i, sz, i, p], i),
        "knn_block_scatter_s8": ([p, i, sz, p, p, sz, sz, p, sz, i, sz, i, p], i),
        "knn_index_neighbours": ([p, p, sz, i, i, p], i),
        "knn_index_classify": ([p, p, sz, i, i, i, i, i, i, p, p, p, psz, p], i),
        "knn_index_classify_rows": ([p, p, sz, i, i, i, i, p, p, psz, p], i),
        "knn_classify_weighted": ([p, sz, i, i, i, p, sz, p, p, p, psz], i),
        "knn_regress": ([p, sz, i, i, p, sz, p], i),
        "knn_index_classify_weighted": ([p, p, sz, i, i, i, i, i, i, p, p, p, psz, p], i),
        "knn_index_classify_weighted_rows": ([p, p, sz, i, i, i, i, p, p, psz, p], i),
        "knn_index_regress": ([p, p, sz, i, i, i, i, i, p, p], i),
        "knn_index_regress_rows": ([p, p, sz, i, i, i, p, p], i),
        "knn_index_radius_count": ([p, p, sz, i, i, d, i, p], i),
        "knn_index_radius": ([p, p, sz, i, i, d, i, p, p], i),
        "knn_index_radius_rows_count": ([p, p, sz, d, i, p], i),
        "knn_index_radius_rows": ([p, p, sz, d, i, p, p], i),
        "knn_index_dbscan": ([p, d, i, i, p, p, p], i),
        "knn_dbscan_graph": ([p, p, p, sz, i, p, p, p], i),
        "knn_block_gather_pos_dt": ([p, sz, sz, p, sz, sz, p, sz, sz, i, p], i),
        "knn_block_gather_pos_s8": ([p, sz, sz, p, sz, sz, p, sz, sz, p], i),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    return L


lib = _load()


def strerror(status):
    return lib.knn_strerror(status).decode()


def _check(rc, what):
    if rc != OK:
        raise KnnError(rc, what)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------- host API

def dbscan_graph(indptr, records, min_pts, ids=None):
    """knn_dbscan_graph: Index.dbscan's clustering on the host, from the CSR
    Index.radius_rows(None, eps, keep_zero=True) returns (ids: the live ids
    ascending after removals; None: 1 .. m).  Returns DbscanResult(cluster,
    neighbours, nclusters, None)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    records = np.ascontiguousarray(records, dtype=NB_DTYPE)
    if indptr.ndim != 1 or len(indptr) < 2:
        raise ValueError("indptr must have m + 1 >= 2 entries, got shape %r" % (indptr.shape,))
    m = len(indptr) - 1
    a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    if a is not None and a.shape != (m,):
        raise ValueError("ids must have %d entries, got %r" % (m, a.shape))
    cl = np.zeros(m, dtype=np.int32)
    nb = np.zeros(m, dtype=np.int32)
    nc = ctypes.c_int(0)
    _check(lib.knn_dbscan_graph(_ptr(indptr), _ptr(records) if len(records) else None, _ptr(a), m, min_pts,
                                _ptr(cl), _ptr(nb), ctypes.byref(nc)), "knn_dbscan_graph")
    return DbscanResult(cl, nb, nc.value, None)


def load_mat(path, xvar="train_X", lvar="train_labels"):
    """knn_load_mat (replaces matOpen/matGetVariable/mxGetPr, serial:40-52).

    Returns (X (m, n) float64 -- a C-ordered copy of the column-major data,
    labels (numel,) float64 or None)."""
    Xp, Lp = ctypes.c_void_p(), ctypes.c_void_p()
    m, n, nl = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.knn_load_mat(path.encode(), xvar.encode(), lvar.encode() if lvar else None,
                          ctypes.byref(Xp), ctypes.byref(m), ctypes.byref(n),
                          ctypes.byref(Lp), ctypes.byref(nl))
    _check(rc, "knn_load_mat(%s)" % path)
    try:
        cnt = m.value * n.value
        flat = np.ctypeslib.as_array(ctypes.cast(Xp, ctypes.POINTER(ctypes.c_double)),
                                     shape=(max(cnt, 1),))[:cnt].copy()
        X = flat.reshape((n.value, m.value)).T.copy()  # column-major m x n
        labels = None
        if Lp.value:
            labels = np.ctypeslib.as_array(ctypes.cast(Lp, ctypes.POINTER(ctypes.c_double)),
                                           shape=(max(nl.value, 1),))[:nl.value].copy()
    finally:
        lib.knn_free(Xp)
        lib.knn_free(Lp)
    return X, labels


def search(X, k=30, ngpus=1, labels=None, layout="row", dtype="f64"):
    """knn_search: all-kNN with the reference's serial semantics.

    X: (m, n) float64.  layout="row" passes C order, "col" Fortran order (the
    .mat layout).  dtype "f64" (reference arithmetic) or "f32" (fp32 MFMA
    filter; exact kNN of the fp32-rounded points, include/knn.h).
    Returns (neighbours (m, k) NB_DTYPE, search seconds)."""
    X = np.asarray(X, dtype=np.float64)
    m, n = X.shape
    if layout == "col":
        buf, lay = np.asfortranarray(X), COLMAJOR
    else:
        buf, lay = np.ascontiguousarray(X), ROWMAJOR
    out = np.zeros((m, k), dtype=NB_DTYPE)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
    rc = lib.knn_search(_ptr(buf), m, n, lay, _ptr(lab), k, ngpus, DTYPES[dtype], _ptr(out))
    _check(rc, "knn_search")
    return out, lib.knn_last_search_seconds()


QUERY_KEEP_ZERO = 1  # KNN_QUERY_KEEP_ZERO


def query(X, Q, k=30, labels=None, layout="row", dtype="f64", keep_zero=True):
    """knn_query: the k nearest corpus rows (of X, (m, n)) of every row of Q
    ((mq, n)) -- queries that are no part of the corpus (blk:217-242 with a
    foreign query block).  keep_zero=True returns a corpus row equal to the
    query at distance 0.0; False keeps the reference's rule (zero distances
    excluded).  idx is the 1-based corpus row; labels ((m,), optional) fill
    .label.  Returns (neighbours (mq, k) NB_DTYPE, search seconds)."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    m, n = X.shape
    mq = Q.shape[0]
    if Q.ndim != 2 or Q.shape[1] != n:
        raise ValueError("Q must be (mq, %d), got %r" % (n, Q.shape))
    if layout == "col":
        xb, qb, lay = np.asfortranarray(X), np.asfortranarray(Q), COLMAJOR
    else:
        xb, qb, lay = np.ascontiguousarray(X), np.ascontiguousarray(Q), ROWMAJOR
    out = np.zeros((mq, k), dtype=NB_DTYPE)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
    rc = lib.knn_query(_ptr(xb), m, _ptr(qb), mq, n, lay, _ptr(lab), k, DTYPES[dtype],
                       QUERY_KEEP_ZERO if keep_zero else 0, _ptr(out))
    _check(rc, "knn_query")
    return out, lib.knn_last_search_seconds()


def classify_query(nb, labels, qlabels=None, nclasses=10, rule=VOTE_SERIAL):
    """knn_classify_query: the vote of query()'s records over the corpus
    labels; matches counts predictions equal to qlabels (0 without them).
    Returns (pred, matches)."""
    nb = np.ascontiguousarray(nb)
    mq, k = nb.shape
    lab = np.ascontiguousarray(labels, dtype=np.float64)
    ql = None if qlabels is None else np.ascontiguousarray(qlabels, dtype=np.float64)
    pred = np.zeros(mq, dtype=np.int32)
    matches = ctypes.c_size_t()
    rc = lib.knn_classify_query(_ptr(nb), mq, k, nclasses, rule, _ptr(lab), lab.shape[0], _ptr(ql),
                                _ptr(pred), ctypes.byref(matches))
    _check(rc, "knn_classify_query")
    return pred, matches.value


def search_mpi_compat(X, k=30, procs=2, labels=None, layout="row"):
    """knn_search_mpi_compat: the lists the reference MPI programs compute
    with `procs` ranks, bugs included (include/knn.h).  Returns
    (neighbours (procs*floor(m/procs), k) NB_DTYPE, search seconds)."""
    X = np.asarray(X, dtype=np.float64)
    m, n = X.shape
    if layout == "col":
        buf, lay = np.asfortranarray(X), COLMAJOR
    else:
        buf, lay = np.ascontiguousarray(X), ROWMAJOR
    R = m // procs if procs > 0 else 0
    out = np.zeros((max(procs * R, 1), k), dtype=NB_DTYPE)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
    rc = lib.knn_search_mpi_compat(_ptr(buf), m, n, lay, _ptr(lab), k, procs, _ptr(out))
    _check(rc, "knn_search_mpi_compat")
    return out[: procs * R], lib.knn_last_search_seconds()


def classify(nb, labels, nclasses=10, rule=VOTE_SERIAL):
    """knn_classify (serial:104-130 / blk:252-270).  Returns (pred, matches)."""
    nb = np.ascontiguousarray(nb)
    m, k = nb.shape
    lab = np.ascontiguousarray(labels, dtype=np.float64)
    pred = np.zeros(m, dtype=np.int32)
    matches = ctypes.c_size_t()
    rc = lib.knn_classify(_ptr(nb), m, k, nclasses, rule, _ptr(lab), _ptr(pred), ctypes.byref(matches))
    _check(rc, "knn_classify")
    return pred, matches.value


def classify_weighted(nb, labels, qlabels=None, nclasses=10, weights=WEIGHT_DISTANCE):
    """knn_classify_weighted: the weighted vote of query()'s records over the
    labels by id -- WEIGHT_DISTANCE: a neighbour at distance d counts 1/d, and
    an exact match decides; WEIGHT_UNIFORM: one ballot each (include/knn.h).
    Returns (pred int32 (mq,), sums float64 (mq, nclasses), matches)."""
    nb = np.ascontiguousarray(nb)
    mq, k = nb.shape
    lab = np.ascontiguousarray(labels, dtype=np.float64)
    ql = None if qlabels is None else np.ascontiguousarray(qlabels, dtype=np.float64)
    pred = np.zeros(mq, dtype=np.int32)
    sums = np.zeros((mq, max(nclasses, 0)), dtype=np.float64)
    matches = ctypes.c_size_t()
    rc = lib.knn_classify_weighted(_ptr(nb), mq, k, nclasses, weights, _ptr(lab), lab.shape[0], _ptr(ql),
                                   _ptr(pred), _ptr(sums), ctypes.byref(matches))
    _check(rc, "knn_classify_weighted")
    return pred, sums, matches.value


def regress(nb, targets, weights=WEIGHT_UNIFORM):
    """knn_regress: the uniform or distance-weighted mean of the neighbours'
    targets (by id; include/knn.h), NaN for a query without a neighbour.
    Returns pred float64 (mq,)."""
    nb = np.ascontiguousarray(nb)
    mq, k = nb.shape
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    pred = np.zeros(mq, dtype=np.float64)
    rc = lib.knn_regress(_ptr(nb), mq, k, weights, _ptr(tg), tg.shape[0], _ptr(pred))
    _check(rc, "knn_regress")
    return pred


# ------------------------------------------------------ device-resident API

VOTE_MAX_CLASSES = 1024


def classify_device(d_nb, m, k, nclasses, rule, d_labels, nlabels, q_base=0, d_pred=None,
                    d_matches=None, stream=0):
    """knn_classify_device on device pointers (ints): fills the records'
    labels, writes m predictions to d_pred and the match count (uint64) to
    d_matches (both nullable)."""
    _check(lib.knn_classify_device(d_nb, m, k, nclasses, rule, d_labels, nlabels, q_base,
                                   d_pred or None, d_matches or None, stream or None),
           "knn_classify_device")

def block_bytes(cap, n, dtype="f64"):
    return lib.knn_block_bytes_dt(cap, n, DTYPES[dtype])


def block_meta_offset(cap, n, dtype="f64"):
    return lib.knn_block_meta_offset_dt(cap, n, DTYPES[dtype])


def wire_bytes(cap, n, dtype="f64"):
    return lib.knn_wire_bytes(cap, n, DTYPES[dtype])


def wire_ok(meta_host):
    """meta_host: the reduced block meta as a float64 numpy array."""
    m = np.ascontiguousarray(meta_host, dtype=np.float64)
    return bool(lib.knn_wire_ok(_ptr(m)))


def wire_pack(d_wire, d_block, cap, n, dtype="f64", stream=0):
    _check(lib.knn_wire_pack(d_wire, d_block, cap, n, DTYPES[dtype], stream or None), "knn_wire_pack")


def wire_unpack(d_block, d_wire, cap, n, dtype="f64", stream=0):
    _check(lib.knn_wire_unpack(d_block, d_wire, cap, n, DTYPES[dtype], stream or None),
           "knn_wire_unpack")


def shadow_bytes(cap, n, dtype="f64"):
    return lib.knn_shadow_bytes(cap, n, DTYPES[dtype])


def shadow_pack(d_sblock, d_block, cap, n, dtype="f64", stream=0):
    _check(lib.knn_shadow_pack(d_sblock, d_block, cap, n, DTYPES[dtype], stream or None),
           "knn_shadow_pack")


def split_bytes(cap, n):
    return lib.knn_split_bytes(cap, n)


def split_pack(d_dst, d_block, cap, n, dtype="f64", scale=1.0, stream=0):
    _check(lib.knn_split_pack(d_dst, d_block, cap, n, DTYPES[dtype], float(scale), stream or None),
           "knn_split_pack")


def block_pack(d_block, cap, rows, n, d_src, ld, layout, stream=0, dtype="f64", src_dtype="f64"):
    """knn_block_pack_dt on device pointers (ints).  layout COLMAJOR/ROWMAJOR;
    dtype = block element type, src_dtype = that of d_src ("f64", "f32" or "u8")."""
    _check(lib.knn_block_pack_dt(d_block, DTYPES[dtype], cap, rows, n, d_src, SRC_DTYPES[src_dtype],
                                 ld, layout, stream or None), "knn_block_pack_dt")


def block_append(d_block, cap, row0, rows, n, d_src, ld, layout, stream=0, dtype="f64", src_dtype="f64"):
    """knn_block_append_dt: rows row0 .. row0+rows-1 of a block packed before,
    from a rows x n device source (arguments as block_pack)."""
    _check(lib.knn_block_append_dt(d_block, DTYPES[dtype], cap, row0, rows, n, d_src, SRC_DTYPES[src_dtype],
                                   ld, layout, stream or None), "knn_block_append_dt")


def block_scatter(d_block, cap, d_pos, d_srow, rows, n, d_src, src_rows, ld, layout, stream=0, dtype="f64",
                  src_dtype="f64"):
    """knn_block_scatter_dt: block row d_pos[i] of a block packed before <- row
    d_srow[i] (0 / None: row i) of the src_rows x n device source, i < rows
    (d_pos, d_srow: device int32 arrays; the other arguments as block_pack)."""
    _check(lib.knn_block_scatter_dt(d_block, DTYPES[dtype], cap, d_pos, d_srow or None, rows, n, d_src, src_rows,
                                    SRC_DTYPES[src_dtype], ld, layout, stream or None), "knn_block_scatter_dt")


def block_gather(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, stream=0, dtype="f64"):
    """knn_block_gather_dt: block row row0 + i of d_dst <- row d_list[i] of
    d_src, i < rows (device pointers; d_list: int32 local source rows)."""
    _check(lib.knn_block_gather_dt(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, DTYPES[dtype],
                                   stream or None), "knn_block_gather_dt")


def block_gather_pos(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, stream=0, dtype="f64"):
    """knn_block_gather_pos_dt: block row row0 + i of d_dst <- the row at global
    position d_pos[i] of nblk blocks of capacity src_cap, i < rows (d_tab: a
    device array of the nblk block pointers; d_pos: device int32 positions)."""
    _check(lib.knn_block_gather_pos_dt(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, DTYPES[dtype],
                                       stream or None), "knn_block_gather_pos_dt")


_live_contexts = weakref.WeakSet()


def s8_block_bytes(cap, n):
    return lib.knn_s8_block_bytes(cap, n)


def s8_block_meta_offset(cap, n):
    return lib.knn_s8_block_meta_offset(cap, n)


def block_pack_s8(d_sblock, cap, rows, n, d_src, ld, layout, stream=0, dtype="f64", src_dtype="f64"):
    """knn_block_pack_s8: the speculative byte block (x - 128) + meta straight
    from the source (valid for the search iff s8_spec_ok(reduced meta));
    src_dtype "f64", "f32" or "u8"."""
    _check(lib.knn_block_pack_s8(d_sblock, DTYPES[dtype], cap, rows, n, d_src, SRC_DTYPES[src_dtype], ld, layout,
                                 stream or None), "knn_block_pack_s8")


def block_append_s8(d_sblock, cap, row0, rows, n, d_src, ld, layout, stream=0, dtype="f64", src_dtype="f64"):
    """knn_block_append_s8: the same rows of a byte block packed by block_pack_s8."""
    _check(lib.knn_block_append_s8(d_sblock, DTYPES[dtype], cap, row0, rows, n, d_src, SRC_DTYPES[src_dtype], ld,
                                   layout, stream or None), "knn_block_append_s8")


def block_scatter_s8(d_sblock, cap, d_pos, d_srow, rows, n, d_src, src_rows, ld, layout, stream=0, dtype="f64",
                     src_dtype="f64"):
    """knn_block_scatter_s8: the same rows of a byte block packed by block_pack_s8."""
    _check(lib.knn_block_scatter_s8(d_sblock, DTYPES[dtype], cap, d_pos, d_srow or None, rows, n, d_src, src_rows,
                                    SRC_DTYPES[src_dtype], ld, layout, stream or None), "knn_block_scatter_s8")


def block_gather_s8(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, stream=0):
    """knn_block_gather_s8: the same rows of byte blocks, their norm words made
    again for the new rows."""
    _check(lib.knn_block_gather_s8(d_dst, dst_cap, row0, d_src, src_cap, d_list, rows, n, stream or None),
           "knn_block_gather_s8")


def block_gather_pos_s8(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, stream=0):
    """knn_block_gather_pos_s8: the same rows out of nblk byte blocks, their norm
    words made again for the new rows."""
    _check(lib.knn_block_gather_pos_s8(d_dst, dst_cap, row0, d_tab, src_cap, nblk, d_pos, rows, n, stream or None),
           "knn_block_gather_pos_s8")


def s8_spec_ok(meta_host, n, dtype="f64"):
    m = np.ascontiguousarray(meta_host, dtype=np.float64)
    return bool(lib.knn_s8_spec_ok(_ptr(m), n, DTYPES[dtype]))


@atexit.register
def _close_all():
    # release device buffers while the HIP runtime is still up (its own
    # teardown runs after Python's atexit handlers)
    for c in list(_live_contexts):
        c.close()


INDEX_DEVICE_SRC = 2  # KNN_INDEX_DEVICE_SRC
INDEX_DEVICE_OUT = 4  # KNN_INDEX_DEVICE_OUT
IndexInfo = collections.namedtuple("IndexInfo", "m n nblocks device_bytes last_bits")
ClassifyResult = collections.namedtuple("ClassifyResult", "pred matches counts neighbours seconds")
WeightedResult = collections.namedtuple("WeightedResult", "pred matches sums neighbours seconds")
RegressResult = collections.namedtuple("RegressResult", "pred neighbours seconds")
DbscanResult = collections.namedtuple("DbscanResult", "cluster neighbours nclusters seconds")
_NP_SRC = {np.dtype(np.uint8): U8, np.dtype(np.float32): F32, np.dtype(np.float64): F64}


def _is_device_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr") and a.is_cuda


def _on_index_device(t, what):
    """the index lives on device 0: a pointer into another device's memory is
    no argument for it.  Work pending on torch's current stream is waited for
    (the library reads and writes on the NULL stream)."""
    import torch
    if t.device.index != 0:
        raise ValueError("%s must be on cuda:0 (the index's device), got %s" % (what, t.device))
    torch.cuda.current_stream(t.device).synchronize()


def _index_source(A, layout, what):
    """(pointer, keep-alive, rows, n, layout code, src dtype, device flag) of a
    corpus or query array: uint8 / float32 / float64 numpy arrays and torch GPU
    tensors go in their own type, anything else as float64 on the host."""
    if _is_device_tensor(A):
        import torch
        code = {torch.uint8: U8, torch.float32: F32, torch.float64: F64}.get(A.dtype)
        if code is None:
            A = A.to(torch.float64)
            code = F64
        if A.dim() != 2:
            raise ValueError("%s must be 2-D, got %r" % (what, tuple(A.shape)))
        buf = A.t().contiguous() if layout == "col" else A.contiguous()
        _on_index_device(buf, what)
        return (ctypes.c_void_p(buf.data_ptr()), buf, A.shape[0], A.shape[1],
                COLMAJOR if layout == "col" else ROWMAJOR, code, INDEX_DEVICE_SRC)
    A = np.asarray(A)
    if A.dtype not in _NP_SRC:
        A = A.astype(np.float64)
    if A.ndim != 2:
        raise ValueError("%s must be 2-D, got %r" % (what, A.shape))
    buf = np.asfortranarray(A) if layout == "col" else np.ascontiguousarray(A)
    return _ptr(buf), buf, A.shape[0], A.shape[1], COLMAJOR if layout == "col" else ROWMAJOR, _NP_SRC[A.dtype], 0


class Index:
    """knn_index_t: a corpus packed once and resident on the device, queried
    many times (include/knn.h).  X: (m, n) numpy array or torch GPU tensor of
    uint8, float32 or float64 (other types: float64 on the host); the index
    keeps nothing of X after the constructor returns."""

    def __init__(self, X, labels=None, layout="row", dtype="f64"):
        self._h = ctypes.c_void_p()
        ptr, keep, m, n, lay, src, dev = _index_source(X, layout, "X")
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
        if lab is not None and lab.shape[0] != m:
            raise ValueError("labels must have %d entries, got %d" % (m, lab.shape[0]))
        _check(lib.knn_index_create(ctypes.byref(self._h), ptr, m, n, lay, src, _ptr(lab), DTYPES[dtype], dev),
               "knn_index_create")
        del keep
        self.m, self.n, self.layout, self.dtype = m, n, layout, dtype
        _live_contexts.add(self)

    def close(self):
        if self._h:
            lib.knn_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if not sys.is_finalizing():
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def query(self, Q, k=30, keep_zero=True, out=None):
        """knn_index_query: the k nearest corpus rows of every row of Q
        ((mq, n), in the index's layout argument; types as X, its own).
        out: a torch GPU uint8 buffer of mq*k*16 bytes receives the records on
        the device (labels left 0) and is returned; otherwise a (mq, k)
        NB_DTYPE array.  Returns (neighbours, device seconds of this call)."""
        if not self._h:
            raise ValueError("the index is closed")
        ptr, keep, mq, n, lay, src, flags = _index_source(Q, self.layout, "Q")
        if n != self.n:
            raise ValueError("Q must be (mq, %d), got (%d, %d)" % (self.n, mq, n))
        if keep_zero:
            flags |= QUERY_KEEP_ZERO
        if out is not None:
            if not _is_device_tensor(out) or not out.is_contiguous() or \
                    out.numel() * out.element_size() < mq * k * NB_DTYPE.itemsize:
                raise ValueError("out must be a contiguous torch GPU buffer of >= %d bytes" %
                                 (mq * k * NB_DTYPE.itemsize))
            _on_index_device(out, "out")
            flags |= INDEX_DEVICE_OUT
            res, optr = out, ctypes.c_void_p(out.data_ptr())
        else:
            res = np.zeros((mq, k), dtype=NB_DTYPE)
            optr = _ptr(res)
        _check(lib.knn_index_query(self._h, ptr, mq, lay, src, k, flags, optr), "knn_index_query")
        del keep
        return res, lib.knn_last_search_seconds()

    def add(self, X, labels=None):
        """knn_index_add: append the rows of X ((rows, n), in the index's
        layout argument; types as the constructor's X, its own) without
        repacking what is resident.  labels: one a row when the index was
        made with labels, else None.  Returns the 1-based id of the first
        added row (last_id + 1: ids are never reused); the index keeps nothing
        of X after the call returns."""
        if not self._h:
            raise ValueError("the index is closed")
        ptr, keep, rows, n, lay, src, dev = _index_source(X, self.layout, "X")
        if n != self.n:
            raise ValueError("X must be (rows, %d), got (%d, %d)" % (self.n, rows, n))
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
        if lab is not None and lab.shape[0] != rows:
            raise ValueError("labels must have %d entries, got %d" % (rows, lab.shape[0]))
        first = self.last_id + 1
        _check(lib.knn_index_add(self._h, ptr, rows, lay, src, _ptr(lab), dev), "knn_index_add")
        del keep
        self.m += rows
        return first

    def remove(self, ids):
        """knn_index_remove: forget the rows with these 1-based ids (any integer
        sequence or array; sent as int32).  Ids no longer live and repeats are
        skipped; an id outside [1, last_id], or a list that would leave no row,
        raises KnnError(ERR_INVALID) and changes nothing.  The other rows keep
        their ids.  Returns the number of rows removed."""
        if not self._h:
            raise ValueError("the index is closed")
        a = np.asarray(ids).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("ids must be integers, got %s" % a.dtype)
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise KnnError(ERR_INVALID, "knn_index_remove")
        a = np.ascontiguousarray(a, dtype=np.int32)
        removed = ctypes.c_size_t()
        _check(lib.knn_index_remove(self._h, _ptr(a), a.size, 0, ctypes.byref(removed)), "knn_index_remove")
        self.m -= removed.value
        return removed.value

    def update(self, ids, X, labels=None):
        """knn_index_update: row i of X ((count, n), in the index's layout
        argument; types as the constructor's X, its own) becomes the row with
        the 1-based id ids[i], in place: ids, positions and m stay.  labels:
        count values that replace those rows' labels, or None to leave them.
        An id outside [1, last_id], one that is no longer live or one given
        twice raises KnnError(ERR_INVALID) and changes nothing."""
        if not self._h:
            raise ValueError("the index is closed")
        a = np.asarray(ids).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("ids must be integers, got %s" % a.dtype)
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise KnnError(ERR_INVALID, "knn_index_update")
        a = np.ascontiguousarray(a, dtype=np.int32)
        ptr, keep, rows, n, lay, src, dev = _index_source(X, self.layout, "X")
        if n != self.n or rows != a.size:
            raise ValueError("X must be (%d, %d), got (%d, %d)" % (a.size, self.n, rows, n))
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.float64)
        if lab is not None and lab.shape[0] != rows:
            raise ValueError("labels must have %d entries, got %d" % (rows, lab.shape[0]))
        _check(lib.knn_index_update(self._h, _ptr(a), a.size, ptr, lay, src, _ptr(lab), dev), "knn_index_update")
        del keep

    def neighbours(self, ids=None, k=30, keep_zero=True, out=None):
        """knn_index_neighbours: for each listed 1-based id (any order, repeats
        allowed) the k nearest OTHER live rows of the index; ids=None: every
        live row in ascending id, the corpus's kNN graph.  keep_zero=False
        drops every zero distance (the row itself and its exact duplicates:
        knn_search's leave-one-out rule); keep_zero=True leaves out only the
        row itself (k + 1 must then be within the dtype's limit).  out as in
        query.  An id outside [1, last_id] or one that is no longer live raises
        KnnError(ERR_INVALID).  Returns (neighbours, device seconds)."""
        if not self._h:
            raise ValueError("the index is closed")
        if ids is None:
            a, rows = None, self.m
        else:
            a = np.asarray(ids).reshape(-1)
            if a.size and a.dtype.kind not in "iu":
                raise ValueError("ids must be integers, got %s" % a.dtype)
            if a.size == 0 or a.min() < -2 ** 31 or a.max() >= 2 ** 31:   # (an empty list is not ids=None)
                raise KnnError(ERR_INVALID, "knn_index_neighbours")
            a = np.ascontiguousarray(a, dtype=np.int32)
            rows = a.size
        flags = QUERY_KEEP_ZERO if keep_zero else 0
        if out is not None:
            if not _is_device_tensor(out) or not out.is_contiguous() or \
                    out.numel() * out.element_size() < rows * k * NB_DTYPE.itemsize:
                raise ValueError("out must be a contiguous torch GPU buffer of >= %d bytes" %
                                 (rows * k * NB_DTYPE.itemsize))
            _on_index_device(out, "out")
            flags |= INDEX_DEVICE_OUT
            res, optr = out, ctypes.c_void_p(out.data_ptr())
        else:
            res = np.zeros((rows, max(k, 0)), dtype=NB_DTYPE)
            optr = _ptr(res)
        _check(lib.knn_index_neighbours(self._h, _ptr(a), rows if a is not None else 0, k, flags, optr),
               "knn_index_neighbours")
        return res, lib.knn_last_search_seconds()

    def _vote_outputs(self, rows, k, nclasses, counts, neighbours, out, flags):
        """pred, counts and records of a classify call, on the device when out
        (as in query) is given, with their pointers and the call's flags"""
        if out is not None:
            import torch
            if not _is_device_tensor(out) or not out.is_contiguous() or \
                    out.numel() * out.element_size() < rows * k * NB_DTYPE.itemsize:
                raise ValueError("out must be a contiguous torch GPU buffer of >= %d bytes" %
                                 (rows * k * NB_DTYPE.itemsize))
            _on_index_device(out, "out")
            pred = torch.empty(rows, dtype=torch.int32, device=out.device)
            cnt = torch.empty((rows, max(nclasses, 0)), dtype=torch.int32, device=out.device) if counts else None
            ptrs = [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (pred, cnt, out)]
            return pred, cnt, out, ptrs, flags | INDEX_DEVICE_OUT
        pred = np.zeros(rows, dtype=np.int32)
        cnt = np.zeros((rows, max(nclasses, 0)), dtype=np.int32) if counts else None
        nb = np.zeros((rows, max(k, 0)), dtype=NB_DTYPE) if neighbours else None
        return pred, cnt, nb, [_ptr(pred), _ptr(cnt), _ptr(nb)], flags

    def classify(self, Q, k=30, keep_zero=True, qlabels=None, nclasses=10, rule=VOTE_SERIAL, counts=False,
                 out=None, neighbours=False):
        """knn_index_classify: query's search for the rows of Q (handled as
        there), then the vote among each one's k neighbours with the index's
        own labels, on the device.  qlabels: the rows' true labels (host), for
        matches.  Returns ClassifyResult(pred, matches, counts, neighbours,
        seconds): pred a numpy int32 array of mq predictions (what
        classify_query gives for query's records); matches the number of
        pred[q] == qlabels[q] (0 without qlabels); counts (counts=True) the
        (mq, nclasses) int32 histogram each vote ran on, else None; neighbours
        (neighbours=True) the (mq, k) records with their labels, else None;
        seconds the search's device span (the vote is outside it).  out: a
        torch GPU uint8 buffer of mq*k*16 bytes as in query -- it receives the
        records (labels filled) and is returned as neighbours, and pred and
        counts are then torch int32 tensors on the same device: the whole
        result stays there."""
        if not self._h:
            raise ValueError("the index is closed")
        ptr, keep, mq, n, lay, src, flags = _index_source(Q, self.layout, "Q")
        if n != self.n:
            raise ValueError("Q must be (mq, %d), got (%d, %d)" % (self.n, mq, n))
        if keep_zero:
            flags |= QUERY_KEEP_ZERO
        ql = None if qlabels is None else np.ascontiguousarray(qlabels, dtype=np.float64)
        if ql is not None and ql.shape != (mq,):
            raise ValueError("qlabels must have %d entries, got %r" % (mq, ql.shape))
        pred, cnt, nb, (pp, cp, op), flags = self._vote_outputs(mq, k, nclasses, counts, neighbours, out, flags)
        hit = ctypes.c_size_t()
        _check(lib.knn_index_classify(self._h, ptr, mq, lay, src, k, nclasses, rule, flags, _ptr(ql), pp, cp,
                                      ctypes.byref(hit), op), "knn_index_classify")
        del keep
        return ClassifyResult(pred, hit.value, cnt, nb, lib.knn_last_search_seconds())

    def classify_rows(self, ids=None, k=30, keep_zero=True, nclasses=10, rule=VOTE_SERIAL, counts=False, out=None,
                      neighbours=False):
        """knn_index_classify_rows: neighbours' search for the listed ids
        (ids=None: every live row in ascending id), then the vote; a row's own
        label is the index's.  With ids=None and keep_zero=False on an index
        that removed nothing: search plus classify, the reference's whole
        program.  Arguments and the ClassifyResult as in classify; matches
        counts the rows predicted as their own label."""
        if not self._h:
            raise ValueError("the index is closed")
        if ids is None:
            a, rows = None, self.m
        else:
            a = np.asarray(ids).reshape(-1)
            if a.size and a.dtype.kind not in "iu":
                raise ValueError("ids must be integers, got %s" % a.dtype)
            if a.size == 0 or a.min() < -2 ** 31 or a.max() >= 2 ** 31:   # (an empty list is not ids=None)
                raise KnnError(ERR_INVALID, "knn_index_classify_rows")
            a = np.ascontiguousarray(a, dtype=np.int32)
            rows = a.size
        pred, cnt, nb, (pp, cp, op), flags = self._vote_outputs(rows, k, nclasses, counts, neighbours, out,
                                                                QUERY_KEEP_ZERO if keep_zero else 0)
        hit = ctypes.c_size_t()
        _check(lib.knn_index_classify_rows(self._h, _ptr(a), rows if a is not None else 0, k, nclasses, rule, flags,
                                           pp, cp, ctypes.byref(hit), op), "knn_index_classify_rows")
        return ClassifyResult(pred, hit.value, cnt, nb, lib.knn_last_search_seconds())

    # -- the index as a predictor: distance-weighted vote, regression

    def _predict_outputs(self, rows, k, pred_dtype, nsums, neighbours, out, flags):
        """_vote_outputs for the weighted vote and the regression: pred of
        pred_dtype, float64 sums ((rows, nsums); nsums None: no sums)"""
        if out is not None:
            import torch
            if not _is_device_tensor(out) or not out.is_contiguous() or \
                    out.numel() * out.element_size() < rows * k * NB_DTYPE.itemsize:
                raise ValueError("out must be a contiguous torch GPU buffer of >= %d bytes" %
                                 (rows * k * NB_DTYPE.itemsize))
            _on_index_device(out, "out")
            pred = torch.empty(rows, dtype={np.int32: torch.int32, np.float64: torch.float64}[pred_dtype],
                               device=out.device)
            sums = None if nsums is None else torch.empty((rows, nsums), dtype=torch.float64, device=out.device)
            ptrs = [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in (pred, sums, out)]
            return pred, sums, out, ptrs, flags | INDEX_DEVICE_OUT
        pred = np.zeros(rows, dtype=pred_dtype)
        sums = None if nsums is None else np.zeros((rows, nsums), dtype=np.float64)
        nb = np.zeros((rows, max(k, 0)), dtype=NB_DTYPE) if neighbours else None
        return pred, sums, nb, [_ptr(pred), _ptr(sums), _ptr(nb)], flags

    def _query_source(self, Q, keep_zero):
        if not self._h:
            raise ValueError("the index is closed")
        ptr, keep, mq, n, lay, src, flags = _index_source(Q, self.layout, "Q")
        if n != self.n:
            raise ValueError("Q must be (mq, %d), got (%d, %d)" % (self.n, mq, n))
        return ptr, keep, mq, lay, src, flags | (QUERY_KEEP_ZERO if keep_zero else 0)

    def _id_list(self, ids, what):
        """(int32 array or None, rows) of a rows call's ids argument"""
        if not self._h:
            raise ValueError("the index is closed")
        if ids is None:
            return None, self.m
        a = np.asarray(ids).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("ids must be integers, got %s" % a.dtype)
        if a.size == 0 or a.min() < -2 ** 31 or a.max() >= 2 ** 31:   # (an empty list is not ids=None)
            raise KnnError(ERR_INVALID, what)
        return np.ascontiguousarray(a, dtype=np.int32), a.size

    def classify_weighted(self, Q, k=30, keep_zero=True, qlabels=None, nclasses=10, weights=WEIGHT_DISTANCE,
                          sums=False, out=None, neighbours=False):
        """knn_index_classify_weighted: classify's call with the weighted vote
        behind the search -- WEIGHT_DISTANCE: a neighbour at distance d counts
        1/d and an exact match (distance 0 under keep_zero) decides;
        WEIGHT_UNIFORM: one ballot each, ties to the class met first.  Returns
        WeightedResult(pred, matches, sums, neighbours, seconds), classify's
        result with sums (sums=True: the (mq, nclasses) float64 class weights,
        bit for bit what the module's classify_weighted gives for query's
        records) in place of counts.  out as in classify: pred and sums are
        then torch tensors on that device."""
        ptr, keep, mq, lay, src, flags = self._query_source(Q, keep_zero)
        ql = None if qlabels is None else np.ascontiguousarray(qlabels, dtype=np.float64)
        if ql is not None and ql.shape != (mq,):
            raise ValueError("qlabels must have %d entries, got %r" % (mq, ql.shape))
        pred, sm, nb, (pp, sp, op), flags = self._predict_outputs(mq, k, np.int32, max(nclasses, 0) if sums else None,
                                                                  neighbours, out, flags)
        hit = ctypes.c_size_t()
        _check(lib.knn_index_classify_weighted(self._h, ptr, mq, lay, src, k, nclasses, weights, flags, _ptr(ql),
                                               pp, sp, ctypes.byref(hit), op), "knn_index_classify_weighted")
        del keep
        return WeightedResult(pred, hit.value, sm, nb, lib.knn_last_search_seconds())

    def classify_weighted_rows(self, ids=None, k=30, keep_zero=True, nclasses=10, weights=WEIGHT_DISTANCE, sums=False,
                               out=None, neighbours=False):
        """knn_index_classify_weighted_rows: classify_rows' call (ids, the
        keep-zero rule and its k + 1 limit as there) with the weighted vote;
        the WeightedResult as in classify_weighted, matches counting the rows
        predicted as their own label."""
        a, rows = self._id_list(ids, "knn_index_classify_weighted_rows")
        pred, sm, nb, (pp, sp, op), flags = self._predict_outputs(rows, k, np.int32,
                                                                  max(nclasses, 0) if sums else None, neighbours, out,
                                                                  QUERY_KEEP_ZERO if keep_zero else 0)
        hit = ctypes.c_size_t()
        _check(lib.knn_index_classify_weighted_rows(self._h, _ptr(a), rows if a is not None else 0, k, nclasses,
                                                    weights, flags, pp, sp, ctypes.byref(hit), op),
               "knn_index_classify_weighted_rows")
        return WeightedResult(pred, hit.value, sm, nb, lib.knn_last_search_seconds())

    def regress(self, Q, k=30, keep_zero=True, weights=WEIGHT_UNIFORM, out=None, neighbours=False):
        """knn_index_regress: query's search for the rows of Q, then the mean of
        each one's neighbours' targets -- the index's labels, read as real
        values -- uniform or weighted by 1/distance (an exact match decides),
        on the device.  Returns RegressResult(pred, neighbours, seconds): pred
        mq float64 values (NaN for a query without a neighbour), bit for bit
        what the module's regress gives for query's records; neighbours
        (neighbours=True, or out as in classify: pred is then a torch float64
        tensor there) the records, their .label left 0."""
        ptr, keep, mq, lay, src, flags = self._query_source(Q, keep_zero)
        pred, _, nb, (pp, _, op), flags = self._predict_outputs(mq, k, np.float64, None, neighbours, out, flags)
        _check(lib.knn_index_regress(self._h, ptr, mq, lay, src, k, weights, flags, pp, op), "knn_index_regress")
        del keep
        return RegressResult(pred, nb, lib.knn_last_search_seconds())

    def regress_rows(self, ids=None, k=30, keep_zero=True, weights=WEIGHT_UNIFORM, out=None, neighbours=False):
        """knn_index_regress_rows: neighbours' search for the listed ids
        (ids=None: every live row), then regress' mean over the OTHER rows'
        targets: the leave-one-out prediction of each row.  The RegressResult
        as in regress."""
        a, rows = self._id_list(ids, "knn_index_regress_rows")
        pred, _, nb, (pp, _, op), flags = self._predict_outputs(rows, k, np.float64, None, neighbours, out,
                                                                QUERY_KEEP_ZERO if keep_zero else 0)
        _check(lib.knn_index_regress_rows(self._h, _ptr(a), rows if a is not None else 0, k, weights, flags, pp, op),
               "knn_index_regress_rows")
        return RegressResult(pred, nb, lib.knn_last_search_seconds())

    def _radius_count(self, call, rows, flags, out):
        """the count pass: counts as an int32 array, or into / as a torch GPU
        int32 tensor (out: the tensor, or True to make one)"""
        if out is not None and out is not False:
            import torch
            if out is True:
                out = torch.empty(rows, dtype=torch.int32, device="cuda:0")
            if not _is_device_tensor(out) or not out.is_contiguous() or out.dtype != torch.int32 or \
                    out.numel() < rows:
                raise ValueError("out must be a contiguous torch GPU int32 tensor of >= %d entries" % rows)
            _on_index_device(out, "out")
            call(flags | INDEX_DEVICE_OUT, ctypes.c_void_p(out.data_ptr()))
            return out
        counts = np.zeros(rows, dtype=np.int32)
        call(flags, _ptr(counts))
        return counts

    def _radius_fill(self, count_call, fill_call, rows, flags, indptr, out, device):
        """count (unless indptr is given), the offsets, fill; on the device
        when device is set or indptr / out are torch GPU tensors"""
        t0 = 0.0
        if device or _is_device_tensor(indptr) or _is_device_tensor(out):
            import torch
            if indptr is None:
                counts = self._radius_count(count_call, rows, flags, True)
                t0 = lib.knn_last_search_seconds()
                indptr = torch.zeros(rows + 1, dtype=torch.int64, device=counts.device)
                indptr[1:] = torch.cumsum(counts[:rows], 0, dtype=torch.int64)
            if not _is_device_tensor(indptr) or not indptr.is_contiguous() or indptr.dtype != torch.int64 or \
                    indptr.numel() != rows + 1:
                raise ValueError("indptr must be a contiguous torch GPU int64 tensor of %d entries" % (rows + 1))
            total = int(indptr[-1] - indptr[0])
            if out is None:
                out = torch.zeros(max(total, 1) * NB_DTYPE.itemsize, dtype=torch.uint8, device=indptr.device)
            if not _is_device_tensor(out) or not out.is_contiguous() or \
                    out.numel() * out.element_size() < total * NB_DTYPE.itemsize:
                raise ValueError("out must be a contiguous torch GPU buffer of >= %d bytes" %
                                 (total * NB_DTYPE.itemsize))
            _on_index_device(indptr, "indptr")
            _on_index_device(out, "out")
            fill_call(flags | INDEX_DEVICE_OUT, ctypes.c_void_p(indptr.data_ptr()), ctypes.c_void_p(out.data_ptr()))
            self.radius_seconds = (t0, lib.knn_last_search_seconds())
            return indptr, out
        if indptr is None:
            counts = self._radius_count(count_call, rows, flags, None)
            t0 = lib.knn_last_search_seconds()
            indptr = np.zeros(rows + 1, dtype=np.int64)
            np.cumsum(counts, out=indptr[1:])
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        if indptr.shape != (rows + 1,):
            raise ValueError("indptr must have %d entries, got %r" % (rows + 1, indptr.shape))
        # (one record more than asked for: a zero-size array has no address to pass)
        rec = np.zeros(max(int(indptr[-1] - indptr[0]), 0) + 1, dtype=NB_DTYPE)
        fill_call(flags, _ptr(indptr), _ptr(rec))
        self.radius_seconds = (t0, lib.knn_last_search_seconds())
        return indptr, rec[:-1]

    def radius_count(self, Q, radius, keep_zero=True, out=None):
        """knn_index_radius_count: for every row of Q (handled as in query) the
        number of live rows within `radius` (sqrt(S) <= radius; a zero distance
        counts only under keep_zero).  Returns an int32 array; out: a torch GPU
        int32 tensor (or True) receives the counts on the device and is
        returned."""
        ptr, keep, mq, lay, src, flags = self._query_source(Q, keep_zero)

        def call(fl, cp):
            _check(lib.knn_index_radius_count(self._h, ptr, mq, lay, src, radius, fl, cp), "knn_index_radius_count")
        res = self._radius_count(call, mq, flags, out)
        del keep
        return res

    def radius(self, Q, radius, keep_zero=True, indptr=None, out=None, device=False):
        """knn_index_radius_count, the offsets by cumulative sum, and
        knn_index_radius: every row of Q's hits within `radius`, ordered by
        (distance, id).  Returns (indptr, records): query q's hits are
        records[indptr[q] - indptr[0]:indptr[q + 1] - indptr[0]], indptr int64
        of mq + 1 entries, records of NB_DTYPE.  indptr given: the count is
        skipped (the offsets of an earlier radius_count of the same call;
        KnnError(ERR_INVALID) if a segment is not its query's number of hits).
        device=True, or indptr / out as torch GPU tensors (int64 offsets, a
        byte buffer for the records as in query): counts, offsets and records
        stay on the device.  The two calls' device seconds are kept in
        self.radius_seconds."""
        ptr, keep, mq, lay, src, flags = self._query_source(Q, keep_zero)

        def count(fl, cp):
            _check(lib.knn_index_radius_count(self._h, ptr, mq, lay, src, radius, fl, cp), "knn_index_radius_count")

        def fill(fl, ip, op):
            _check(lib.knn_index_radius(self._h, ptr, mq, lay, src, radius, fl, ip, op), "knn_index_radius")
        res = self._radius_fill(count, fill, mq, flags, indptr, out, device)
        del keep
        return res

    def radius_rows_count(self, ids=None, radius=0.0, keep_zero=True, out=None):
        """knn_index_radius_rows_count: radius_count for resident rows, by id
        (ids=None: every live row in ascending id); the row itself never
        counts, its exact duplicates only under keep_zero."""
        a, rows = self._id_list(ids, "knn_index_radius_rows_count")

        def call(fl, cp):
            _check(lib.knn_index_radius_rows_count(self._h, _ptr(a), rows if a is not None else 0, radius, fl, cp),
                   "knn_index_radius_rows_count")
        return self._radius_count(call, rows, QUERY_KEEP_ZERO if keep_zero else 0, out)

    def radius_rows(self, ids=None, radius=0.0, keep_zero=True, indptr=None, out=None, device=False):
        """knn_index_radius_rows: radius for resident rows, by id -- with
        ids=None the corpus's epsilon-graph in CSR.  Arguments and result as
        in radius, ids as in neighbours."""
        a, rows = self._id_list(ids, "knn_index_radius_rows")
        cnt = rows if a is not None else 0

        def count(fl, cp):
            _check(lib.knn_index_radius_rows_count(self._h, _ptr(a), cnt, radius, fl, cp),
                   "knn_index_radius_rows_count")

        def fill(fl, ip, op):
            _check(lib.knn_index_radius_rows(self._h, _ptr(a), cnt, radius, fl, ip, op), "knn_index_radius_rows")
        return self._radius_fill(count, fill, rows, QUERY_KEEP_ZERO if keep_zero else 0, indptr, out, device)

    def dbscan(self, eps, min_pts=5, neighbours=False, device=False):
        """knn_index_dbscan: DBSCAN over the live rows, on the device, without
        the epsilon-graph (include/knn.h has the definition).  A row is core
        when at least min_pts live rows -- itself and its exact duplicates
        included, scikit-learn's min_samples convention -- lie within eps of
        it; clusters are the connected components of the core rows, numbered
        1 .. nclusters in ascending order of their lowest id; a border row takes
        the cluster of its nearest core neighbour by (distance, id); noise is
        cluster 0 (scikit-learn writes -1 there).  Returns DbscanResult(cluster,
        neighbours, nclusters, seconds): cluster an int32 array by ascending
        live id, neighbours (on request) every row's neighbourhood size, both
        torch GPU tensors with device=True."""
        if not self._h:
            raise ValueError("the index is closed")
        m = self.info().m
        nc = ctypes.c_int(0)
        if device:
            import torch
            cl = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda:0")
            nb = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda:0") if neighbours else None
            _check(lib.knn_index_dbscan(self._h, eps, min_pts, INDEX_DEVICE_OUT, ctypes.c_void_p(cl.data_ptr()),
                                        ctypes.c_void_p(nb.data_ptr()) if neighbours else None, ctypes.byref(nc)),
                   "knn_index_dbscan")
            cl, nb = cl[:m], nb[:m] if neighbours else None
        else:
            # (one entry more than asked for: a zero-size array has no address to pass)
            cl = np.zeros(m + 1, dtype=np.int32)
            nb = np.zeros(m + 1, dtype=np.int32) if neighbours else None
            _check(lib.knn_index_dbscan(self._h, eps, min_pts, 0, _ptr(cl), _ptr(nb), ctypes.byref(nc)),
                   "knn_index_dbscan")
            cl, nb = cl[:m], nb[:m] if neighbours else None
        return DbscanResult(cl, nb, nc.value, lib.knn_last_search_seconds())

    @property
    def last_id(self):
        """knn_index_last_id: the highest id handed out so far (m while nothing
        was removed)."""
        if not self._h:
            raise ValueError("the index is closed")
        v = ctypes.c_size_t()
        _check(lib.knn_index_last_id(self._h, ctypes.byref(v)), "knn_index_last_id")
        return v.value

    def info(self):
        """knn_index_info: IndexInfo(m, n, nblocks, device_bytes, last_bits)."""
        m, n, db = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        nb, bits = ctypes.c_int(), ctypes.c_int()
        _check(lib.knn_index_info(self._h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(nb), ctypes.byref(db),
                                  ctypes.byref(bits)), "knn_index_info")
        return IndexInfo(m.value, n.value, nb.value, db.value, bits.value)


class Context:
    """knn_ctx_t: running neighbour lists of nq queries on one device."""

    def __init__(self, device, nq, n, block_cap, k, dtype="f64"):
        self._h = ctypes.c_void_p()
        _check(lib.knn_ctx_create_dt(ctypes.byref(self._h), device, nq, n, block_cap, k,
                                     DTYPES[dtype]), "knn_ctx_create_dt")
        self.nq, self.n, self.block_cap, self.k, self.dtype = nq, n, block_cap, k, dtype
        _live_contexts.add(self)

    def close(self):
        if self._h:
            lib.knn_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if not sys.is_finalizing():
            self.close()

    def begin(self, d_qblock, q_cap, q_base, d_meta, stream=0, h_meta=None):
        """knn_ctx_begin; with h_meta (host float64 copy of the reduced meta)
        knn_ctx_begin_meta, which needs no device read-back."""
        if h_meta is None:
            _check(lib.knn_ctx_begin(self._h, d_qblock, q_cap, q_base, d_meta, stream or None),
                   "knn_ctx_begin")
        else:
            hm = np.ascontiguousarray(h_meta, dtype=np.float64)
            _check(lib.knn_ctx_begin_meta(self._h, d_qblock, q_cap, q_base, d_meta, _ptr(hm),
                                          stream or None), "knn_ctx_begin_meta")

    def begin_s8(self, d_sblock, q_cap, q_base, d_meta, h_meta, stream=0):
        """knn_ctx_begin_s8: start from the query block's speculative byte block"""
        hm = np.ascontiguousarray(h_meta, dtype=np.float64)
        _check(lib.knn_ctx_begin_s8(self._h, d_sblock, q_cap, q_base, d_meta, _ptr(hm), stream or None),
               "knn_ctx_begin_s8")

    def attach_qblock(self, d_qblock, q_cap):
        _check(lib.knn_ctx_attach_qblock(self._h, d_qblock, q_cap), "knn_ctx_attach_qblock")

    def step(self, d_cblock, nc, c_base, stream=0):
        _check(lib.knn_ctx_step(self._h, d_cblock, nc, c_base, stream or None), "knn_ctx_step")

    def step_shadow(self, d_sblock, nc, c_base, stream=0):
        _check(lib.knn_ctx_step_shadow(self._h, d_sblock, nc, c_base, stream or None),
               "knn_ctx_step_shadow")

    def step_shadow_n(self, d_sblocks, ncs, c_bases, stream=0):
        """several resident shadow-form blocks in one step (int8 byte
        blocks: one fused distance launch per 8 blocks)"""
        nb = len(d_sblocks)
        ptrs = (ctypes.c_void_p * nb)(*d_sblocks)
        ncv = (ctypes.c_size_t * nb)(*ncs)
        cbv = (ctypes.c_size_t * nb)(*c_bases)
        _check(lib.knn_ctx_step_shadow_n(self._h, nb, ptrs, ncv, cbv, stream or None),
               "knn_ctx_step_shadow_n")

    def step_n(self, d_cblocks, ncs, c_bases, stream=0):
        """several resident element blocks in one step (split-filter
        searches: one fused distance launch and merge per 8 blocks)"""
        nb = len(d_cblocks)
        ptrs = (ctypes.c_void_p * nb)(*d_cblocks)
        ncv = (ctypes.c_size_t * nb)(*ncs)
        cbv = (ctypes.c_size_t * nb)(*c_bases)
        _check(lib.knn_ctx_step_n(self._h, nb, ptrs, ncv, cbv, stream or None), "knn_ctx_step_n")

    def research_blocks(self, d_sblocks, ncs, c_bases, d_out, stream=0):
        """A ring rank's int8 re-search of the queries end() left
        uncertified, against the byte blocks it holds (knn_ctx_research_blocks);
        returns the count the rescan pass still has to resolve."""
        nb = len(d_sblocks)
        ptrs = (ctypes.c_void_p * nb)(*d_sblocks)
        ncv = (ctypes.c_size_t * nb)(*ncs)
        cbv = (ctypes.c_size_t * nb)(*c_bases)
        u = ctypes.c_size_t(0)
        _check(lib.knn_ctx_research_blocks(self._h, nb, ptrs, ncv, cbv, d_out, ctypes.byref(u), stream or None),
               "knn_ctx_research_blocks")
        return u.value

    def shadow(self):
        """Shadow form of this search (after begin): 0 none, 1 fp16 shadow
        rows, 2 byte blocks of the int8 contraction."""
        return lib.knn_ctx_shadow(self._h)

    def shadow_bytes(self, cap):
        return lib.knn_ctx_shadow_bytes(self._h, cap)

    def shadow_pack(self, d_sblock, d_block, cap, stream=0):
        _check(lib.knn_ctx_shadow_pack(self._h, d_sblock, d_block, cap, stream or None),
               "knn_ctx_shadow_pack")

    def end(self, d_out, stream=0):
        u = ctypes.c_size_t()
        _check(lib.knn_ctx_end(self._h, d_out, ctypes.byref(u), stream or None), "knn_ctx_end")
        return u.value

    def rescan_step(self, d_cblock, nc, c_base, stream=0):
        _check(lib.knn_ctx_rescan_step(self._h, d_cblock, nc, c_base, stream or None),
               "knn_ctx_rescan_step")

    def rescan_end(self, d_out, stream=0):
        _check(lib.knn_ctx_rescan_end(self._h, d_out, stream or None), "knn_ctx_rescan_end")

    def search_packed(self, d_block, m, d_out, stream=0):
        _check(lib.knn_search_packed(self._h, d_block, m, d_out, stream or None),
               "knn_search_packed")

    def profile(self, enable=-1):
        """knn_ctx_profile: (dist_ms, merge_ms, launches); enable 1 resets+starts."""
        dm, mm, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _check(lib.knn_ctx_profile(self._h, enable, ctypes.byref(dm), ctypes.byref(mm),
                                   ctypes.byref(n)), "knn_ctx_profile")
        return dm.value, mm.value, n.value

    def set_solo(self, on):
        """knn_ctx_set_solo: one-step searches (P = 1) on the caller's stream."""
        _check(lib.knn_ctx_set_solo(self._h, 1 if on else 0), "knn_ctx_set_solo")

    def set_keep_zero(self, on):
        """knn_ctx_set_keep_zero: S == 0 candidates are results (searches
        begun after the call)."""
        _check(lib.knn_ctx_set_keep_zero(self._h, 1 if on else 0), "knn_ctx_set_keep_zero")

    def search_meta(self):
        """knn_ctx_search_meta: the meta the last search's kernels read."""
        out = (ctypes.c_double * META_DOUBLES)()
        _check(lib.knn_ctx_search_meta(self._h, out), "knn_ctx_search_meta")
        return np.frombuffer(out, dtype=np.float64).copy()

    def profile_merge(self):
        """knn_ctx_profile_merge: (merge kernel ms, merge launches,
        algorithmic bytes) over the profiled steps."""
        mm, n, b = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        _check(lib.knn_ctx_profile_merge(self._h, ctypes.byref(mm), ctypes.byref(n), ctypes.byref(b)),
               "knn_ctx_profile_merge")
        return mm.value, n.value, b.value

    def info(self):
        mode, splits = ctypes.c_int(), ctypes.c_int()
        _check(lib.knn_ctx_info(self._h, ctypes.byref(mode), ctypes.byref(splits)), "knn_ctx_info")
        return mode.value, splits.value

    def contraction_bits(self):
        """64 / 32, 16 (exact fp16 MFMA, or the split fp16 filter) or 8 (exact
        int8 MFMA) for this search."""
        return lib.knn_ctx_contraction_bits(self._h)

    def split(self):
        """1 when this search filters with the split fp16 contraction."""
        return lib.knn_ctx_split(self._h)
