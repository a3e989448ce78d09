"""The certificate sweeps of test_gpu_cert.py are not vacuous: shown from the
numpy model of tests/cert_ref.py alone (knn_cert_E restated, exact fp64 S),
no GPU.  For every (data, filter, offset list) the GPU tests use, the model
certifies nearly every query at the first offset, nearly none at the last and
a share strictly in between at some offset; the tie cases hold exact S ties
at rank k; the crowd cases hold more than kp pairs a query inside (0, E).
These are conditions on the test data: if one fails, the data or the offsets
change, not the condition."""
import functools

import numpy as np
import pytest

import cert_ref as cr


def test_cert_E_terms():
    """each form against its terms written out once more, and their order
    at n = 64"""
    n, qn, mx, ma = 200, 3.0e5, 4.0e5, 70.0
    qc = qn + mx
    assert cr.cert_E(n, qn, mx, "f64") == 8.0 * 204.0 * 2.0 ** -53 * qc
    assert cr.cert_E(n, qn, mx, "f32") == 204.0 * qc * (2.0 ** -24 * (1.0 + 408.0 * 2.0 ** -24) + 2.0 ** -51)
    rel = ((136.0 + 8.0) * 2.0 ** -24 + 816.0 * 2.0 ** -53) * qc * (1.0 + 1e-6)
    ab = 2.0 ** -26 * ma * np.sqrt(200.0) * (np.sqrt(qn) + np.sqrt(mx))
    assert cr.cert_E(n, qn, mx, "split", ma) == rel + ab
    # n = 64: (n + 4) u for the fp32 filter, (136 + n / 25) u for the split one
    assert cr.cert_E(64, qn, mx, "f64") < cr.cert_E(64, qn, mx, "f32") < cr.cert_E(64, qn, mx, "split", ma)
    # vectorised over the queries' norms
    assert cr.cert_E(n, np.array([qn, 0.0]), mx, "split", ma)[0] == rel + ab


def test_kp_for_rule():
    got = [(k, dt, cr.kp_for(k, dt)) for dt in ("f64", "f32") for k in (1, 16, 17, 30, 32, 33, 100, 128)]
    assert got == [(1, "f64", 32), (16, "f64", 32), (17, "f64", 64), (30, "f64", 64), (32, "f64", 64),
                   (33, "f64", 64), (100, "f64", 64), (128, "f64", 64),
                   (1, "f32", 32), (16, "f32", 32), (17, "f32", 64), (30, "f32", 64), (32, "f32", 64),
                   (33, "f32", 128), (100, "f32", 128), (128, "f32", 128)]


def _pred(config, n, k, off):
    dtype, filt, _ = cr.CONFIGS[config]
    return cr.predicted_certified(cr.sweep_points(config, n, off), k, cr.kp_for(k, dtype), filt)


@pytest.mark.parametrize("config,n,k", cr.SWEEPS)
def test_sweep_crosses_the_transition(config, n, k):
    offs = cr.offsets_for(cr.CONFIGS[config][1])
    p = [_pred(config, n, k, off) for off in offs]
    print(config, n, k, ["%g: %.2f" % (o, v) for o, v in zip(offs, p)])
    assert p[0] >= 0.9
    assert p[-1] <= 0.1
    assert any(0.1 < v < 0.9 for v in p)
    # E grows with the offset: no query comes back
    assert all(b <= a + 0.02 for a, b in zip(p, p[1:]))


@pytest.mark.parametrize("config,n", sorted(cr.MID))
def test_mid_offsets_are_mid_transition(config, n):
    p = _pred(config, n, 30, cr.MID[(config, n)])
    print(config, n, cr.MID[(config, n)], p)
    assert 0.1 < p < 0.9


@pytest.mark.parametrize("config", sorted(cr.RING_MID))
def test_ring_offset_is_mid_transition(config):
    off = cr.RING_MID[config]
    assert off in cr.offsets_for(cr.CONFIGS[config][1])
    assert 0.1 < _pred(config, 64, 30, off) < 0.9


def test_gram_form_agrees_with_exact_sums():
    """the model's fast S (centred Gram form) against the j-ordered sums"""
    X = cr.sweep_points("f32-split", 64, 64.0)
    a, b = cr.gram_S(X), cr.exact_S(X)
    assert np.abs(a - b).max() <= 2.0 ** -40 * b.max()
    assert cr.predicted_certified(X, 30, 64, "split") == cr.predicted_certified(X, 30, 64, "split", exact=True)


# ---- ties -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tie_S(off):
    return cr.exact_S(cr.tie_data() + off, centre=False)


@pytest.mark.parametrize("config", sorted(cr.CONFIGS))
def test_tie_data_has_exact_ties_at_rank_k(config):
    dtype, filt, _ = cr.CONFIGS[config]
    k, kp = 30, cr.kp_for(30, dtype)
    Z = cr.tie_data()
    base = None
    for which, off in enumerate(cr.TIE_OFFSETS[filt]):
        X = Z + off
        assert np.array_equal(X - off, Z), "off + j/8 must be exact"
        assert np.array_equal(cr.stored(X, dtype), X), "and in the block's type"
        assert (X != np.rint(X)).any(), "non-integer: GEMM mode"
        S = _tie_S(off)
        if base is None:
            base = S
        assert np.array_equal(S, base), "the same exact S at every offset"
        Ss = np.where(S == 0.0, np.inf, S)
        Ss.sort(axis=1)
        # a tie set across rank k for every query, at least 10 rows of it
        assert (Ss[:, k - 1] == Ss[:, k]).all()
        ties = (Ss == Ss[:, k - 1, None]).sum(axis=1)
        assert ties.min() >= 10 and (Ss[:, kp] > Ss[:, k - 1]).all()
        p = cr.predicted_certified(X, k, kp, filt)
        assert p >= 0.9 if which == 0 else p <= 0.1, (off, p)


# ---- crowds ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _crowd_S(off):
    X = cr.crowd_data() + off
    return X, cr.exact_S(X, centre=False)


@pytest.mark.parametrize("filt,dtype,k", [("f64", "f64", 30), ("f32", "f32", 30), ("f32", "f32", 100),
                                          ("split", "f32", 30), ("split", "f32", 100), ("split", "f64", 30)])
def test_crowds_sit_inside_E(filt, dtype, k):
    off = cr.CROWD_OFFSET[filt]
    X, S = _crowd_S(off)
    assert np.array_equal(X - off, cr.crowd_data()) and np.array_equal(cr.stored(X, dtype), X)
    kp = cr.kp_for(k, dtype)
    E = cr.query_E(X, filt)[:, None]
    inside = ((S > 0.0) & (S < E)).sum(axis=1)
    assert inside.min() > kp, (inside.min(), kp)
    # the query's own crowd within E / 100: 70 rows less itself and, for a
    # duplicated row, its 2 copies (S == 0)
    near = ((S > 0.0) & (S < E / 100.0)).sum(axis=1)
    assert near.min() >= 67, near.min()
    # 3 exact duplicates a crowd: 120 rows with two S == 0 partners
    zeros = (S == 0.0).sum(axis=1) - 1
    assert (zeros == 2).sum() == 120 and ((zeros == 0) | (zeros == 2)).all()


# ---- the outlier ----------------------------------------------------------

@pytest.mark.parametrize("scale", [2.0 ** 10, 2.0 ** 20])
def test_outlier_owns_the_meta(scale):
    Z = cr.stored(cr.mixed_gap(cr.M_SWEEP, 64, seed=64), "f32")
    X = cr.stored(cr.with_outlier(Z, scale), "f32")
    nrm = (X * X).sum(axis=1)
    assert nrm.argmax() == 17 and np.abs(X).max(axis=1).argmax() == 17
    rest = np.delete(np.arange(len(X)), 17)
    assert nrm[17] >= 2.0 ** 14 * nrm[rest].max() and np.abs(X[17]).max() >= 2.0 ** 7 * np.abs(X[rest]).max()
    # the split pre-scale (maxabs S in [2^13, 2^14)) and the fp16 halves
    S = 2.0 ** (14 - np.frexp(np.abs(X).max())[1])
    xs = X[rest] * S
    with np.errstate(over="ignore"):
        hi = xs.astype(np.float16).astype(np.float64)
        lo = (xs - hi).astype(np.float16).astype(np.float64)
    share = float(np.mean(np.abs(lo) < 2.0 ** -14))
    print("scale 2^%d: %.3f of the other rows' lo halves subnormal or zero" % (np.log2(scale), share))
    if scale == 2.0 ** 20:
        assert share == 1.0
        assert float(np.mean(hi == 0.0)) < 0.01, "hi halves still carry the values"
