"""Plain-numpy model of the GEMM-mode certificate (no GPU): knn_cert_E term
for term, the state capacity rule of knn_kp_for, and an optimistic prediction
of which queries the first pass certifies.  Also the seeded data makers and
the offset lists shared by test_cert_cpu.py (which proves from this model
alone that the sweeps cross the certificate's transition) and
test_gpu_cert.py (which runs them)."""
import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53


def cert_E(n, qn, maxnorm, filt, maxabs=0.0):
    """knn_cert_E (knn_kernels.hip): the bound on |GEMM-form d^2 - exact S|.
    filt: "f64" (fp64 MFMA filter), "f32" (fp32 MFMA filter) or "split" (the
    split fp16 filter, fp32 and fp64 blocks alike).  qn may be an array."""
    qn = np.asarray(qn, dtype=np.float64)
    nn = float(n) + 4.0
    qc = qn + maxnorm
    if filt == "split":
        acc = float(n) / 25.0
        return (((136.0 + acc) * U24 + 4.0 * nn * U53) * qc * (1.0 + 1e-6) +
                2.0 ** -26 * maxabs * np.sqrt(float(n)) * (np.sqrt(qn) + np.sqrt(maxnorm)))
    if filt == "f64":
        return 8.0 * nn * U53 * qc
    if filt == "f32":
        return nn * qc * (U24 * (1.0 + 2.0 * nn * U24) + 4.0 * U53)
    raise ValueError(filt)


def kp_for(k, dtype):
    """knn_kp_for (knn_internal.h): the per-query state capacity serving k"""
    if k <= 16:
        return 32
    if dtype != "f32":
        return 64
    return 64 if k <= 32 else 128


def stored(X, dtype):
    """the values a block of `dtype` holds, as fp64"""
    X = np.asarray(X, dtype=np.float64)
    return X.astype(np.float32).astype(np.float64) if dtype == "f32" else X


def exact_S(X, centre=True):
    """S[i, j] = sum_t (x_it - x_jt)^2 in t order in fp64 (elementwise numpy
    only: no FMA, no pairwise sums), on the centred points by default (S
    does not depend on a common shift; centred, the differences carry no
    cancellation)."""
    X = np.asarray(X, dtype=np.float64)
    if centre:
        X = X - X.mean(axis=0)
    m, n = X.shape
    S = np.zeros((m, m), dtype=np.float64)
    for t in range(n):
        d = X[:, t, None] - X[None, :, t]
        S += d * d
    return S


def gram_S(X):
    """S of the centred points in the Gram form |a|^2 + |b|^2 - 2 a.b in
    fp64: centred, the form loses ~2^-50 (|a|^2 + |b|^2) of the centred norms,
    far below any E of the uncentred ones -- exact_S's values for the model's
    purpose at a hundredth of its time.  Entries the form cannot tell from 0
    (exact duplicates) are set to 0."""
    X = np.asarray(X, dtype=np.float64)
    X = X - X.mean(axis=0)
    nrm = (X * X).sum(axis=1)
    S = nrm[:, None] + nrm[None, :] - 2.0 * (X @ X.T)
    S[S <= 2.0 ** -40 * (nrm[:, None] + nrm[None, :])] = 0.0
    return S


def query_E(X, filt):
    """E of every row of X as a query of the all-kNN search over X"""
    n = X.shape[1]
    qn = (X * X).sum(axis=1)
    return cert_E(n, qn, qn.max(), filt, np.abs(X).max())


def predicted_certified(X, k, kp, filt, exact=False):
    """Fraction of queries with S_(kp+1) - E > S_(k), ranks over the nonzero
    fp64 S of the query's row on the centred points (zeros are dropped
    results; exact=True: exact_S's j-ordered sums instead of gram_S -- the
    fractions agree, test_cert_cpu.py checks it).  Optimistic: the
    engine's T / Td are GEMM-form values of candidates a lane list or a merge
    dropped, at most the (kp+1)-th smallest."""
    X = np.asarray(X, dtype=np.float64)
    S = exact_S(X) if exact else gram_S(X)
    S[S == 0.0] = np.inf
    S.sort(axis=1)
    E = query_E(X, filt)
    return float(np.mean(S[:, kp] - E > S[:, k - 1]))


# ---- data makers (all seeded) ---------------------------------------------

def mixed_gap(m=1200, n=64, seed=1, clusters=8, lo=0.2, hi=2.0):
    """Gaussian clusters of m / clusters rows (more than any kp + 1 here)
    around centres N(0, 1), their spreads log-spaced over a decade, [0.2, 2]:
    the gap between a query's k-th and (kp+1)-th neighbour, both inside its
    cluster, scales with the spread squared -- two decades -- so the
    certificate fails cluster by cluster as E grows instead of all at once.
    Rows are dealt to the clusters in random order: a cluster that follows
    the row index (i mod 8) puts all of a query's neighbours into one lane's
    candidate list of the distance kernels, which overflows -- uncertified
    queries that have nothing to do with E."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.0, (clusters, n))
    spread = np.geomspace(lo, hi, clusters)
    lab = rng.permutation(np.arange(m) % clusters)
    return centres[lab] + spread[lab, None] * rng.normal(0.0, 1.0, (m, n))


TIE_CLUSTER = 41   # rows of one tie cluster: the centre and two shells of 20


def tie_data(n=64, seed=2, clusters=29):
    """Clusters of 41 rows on a grid of eighths: a centre c (multiples of 1/8
    in [-2, 2]), 20 rows c + e_t / 8 and 20 rows c + e_t / 4 (t distinct, n >=
    40).  Within a cluster S is 1, 2, 4, 5 or 8 sixty-fourths, exact in any
    summation order and at any offset that keeps off + j / 8 exact: every
    query has a tie set of 19 or 20 rows across rank 30, and the next cluster
    lies ~170 away, past the (kp+1)-th neighbour.  Rows are shuffled, so the
    index order of a tie set is not the order it was made in."""
    assert n >= 40
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(clusters):
        c = rng.integers(-16, 17, n) / 8.0
        coords = rng.permutation(n)[:40]
        rows.append(c)
        for i, t in enumerate(coords):
            r = c.copy()
            r[t] += 0.125 if i < 20 else 0.25
            rows.append(r)
    X = np.array(rows)
    return X[rng.permutation(len(X))]


def crowd_data(n=64, seed=3, crowds=40, size=70, dups=3):
    """`crowds` crowds of `size` rows: a centre N(0, 2) plus N(0, 0.05) on a
    grid of 2^-11 (exact in fp32 at an offset of 4096, in fp64 at 2^24), the
    first `dups` rows of each crowd one row repeated.  Within a crowd S ~ 0.3;
    the crowds themselves lie ~500 apart."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(crowds):
        c = np.rint(rng.normal(0.0, 2.0, n) * 2048.0) / 2048.0
        P = c + np.rint(rng.normal(0.0, 0.05, (size, n)) * 2048.0) / 2048.0
        P[1:dups] = P[0]
        parts.append(P)
    X = np.vstack(parts)
    return X[rng.permutation(len(X))]


def with_outlier(Z, scale, row=17):
    """Z with one row multiplied by `scale`: that row alone sets the meta's
    MAXNORM and maxabs"""
    X = np.array(Z, dtype=np.float64)
    X[row] *= scale
    return X


# ---- the sweeps -----------------------------------------------------------
# (block dtype, filter, KNN_NO_SPLIT) of the four filter configurations
CONFIGS = {
    "f64-mfma": ("f64", "f64", True),
    "f32-mfma": ("f32", "f32", True),
    "f32-split": ("f32", "split", False),
    "f64-split": ("f64", "split", False),
}
# half-octave steps through the modelled transition of the mixed-gap data
# (fp32 and split filters: offsets 32 to 128; the fp64 filter: 2^18 to 2^20)
OFFSETS_F32 = [0.0, 8.0, 32.0, 45.0, 64.0, 90.0, 128.0, 256.0, 4096.0]
OFFSETS_F64 = [0.0, 2.0 ** 16, 2.0 ** 18, 2.0 ** 19, 741455.25, 2.0 ** 20, 2.0 ** 22, 2.0 ** 26]


def offsets_for(filt):
    return OFFSETS_F64 if filt == "f64" else OFFSETS_F32


# (config, n, k) of every sweep
SWEEPS = ([(c, n, 30) for c in CONFIGS for n in (64, 200)] +
          [(c, n, 100) for c in ("f32-mfma", "f32-split") for n in (64, 200)])
# one offset at the modelled mid-transition for the ragged and the long rows
MID = {
    ("f64-mfma", 33): 2.0 ** 20, ("f32-mfma", 33): 128.0, ("f32-split", 33): 64.0, ("f64-split", 33): 64.0,
    ("f64-mfma", 960): 2.0 ** 17, ("f32-mfma", 960): 11.0, ("f32-split", 960): 22.0, ("f64-split", 960): 22.0,
}
# the sweep's mid-transition offset (n = 64) for the P = 3 block rotation
RING_MID = {"f64-mfma": 741455.25, "f32-split": 64.0, "f64-split": 64.0}
# (certified, past the transition) offsets of the tie and crowd cases
TIE_OFFSETS = {"f64": (2.0 ** 16, 2.0 ** 24), "f32": (8.0, 4096.0), "split": (8.0, 4096.0)}
CROWD_OFFSET = {"f64": 2.0 ** 24, "f32": 4096.0, "split": 4096.0}
M_SWEEP = 1200


def sweep_points(config, n, off, m=M_SWEEP):
    """the sweep's points at one offset, as the block dtype stores them"""
    dtype = CONFIGS[config][0]
    return stored(mixed_gap(m, n, seed=n) + off, dtype)
