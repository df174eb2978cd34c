"""numpy/fp64 restatement of the source-count criterion of doa.source_count (include/doa_hip.h), for its tests
(importable like scenarios.py and calibration_ref.py).  Not a block of the reference: the definition is this project's,
stated once in the header, and written out here literally.

For one covariance item (column-major N x N complex64, only the upper triangle significant) with eigenvalues
l_0 <= ... <= l_{N-1} (numpy.linalg.eigvalsh of the Hermitian matrix built from the upper triangle, in double):

    status  a non-finite entry, or l_{N-1} <= 0      ->  count -1 (eigenvalues NaN for a non-finite item)
    floor   l_i <- max(l_i, l_{N-1} * 2^-40)
    L_k   = sum log l_i - m log((sum l_i) / m)  over the m = N - k smallest, summed in ascending index order
    MDL_k = -K L_k + 0.5 k (2N - k) log K        AIC_k = -2K L_k + 2 k (2N - k)
    count = the smallest k in 0 .. kmax that attains the minimum
"""
import math

import numpy as np

MDL, AIC = 0, 1
FLOOR = 2.0 ** -40


def hermitian_from_upper(item, N):
    """The N x N complex128 Hermitian matrix an item's upper triangle defines (diagonal: real parts)."""
    A = np.asarray(item).reshape(N, N, order="F").astype(np.complex128)
    U = np.triu(A, 1)
    return U + U.conj().T + np.diag(A.diagonal().real)


def eigenvalues(item, N):
    """Ascending eigenvalues in double; all NaN when the upper triangle holds a non-finite entry."""
    A = np.asarray(item).reshape(N, N, order="F")
    if not np.all(np.isfinite(A[np.triu_indices(N)])):
        return np.full(N, np.nan)
    return np.linalg.eigvalsh(hermitian_from_upper(item, N))


def log_likelihood(l, k):
    """L_k on floored ascending eigenvalues l."""
    m = len(l) - k
    slog, ssum = 0.0, 0.0
    for i in range(m):                       # ascending index order
        slog += math.log(l[i])
        ssum += l[i]
    return slog - m * math.log(ssum / m)


def criterion(l, K, method, kmax=None):
    """(values [kmax + 1] or None, count) from ascending eigenvalues l."""
    l = [float(v) for v in l]
    N = len(l)
    kmax = N - 1 if kmax is None else kmax
    top = l[-1]
    if not all(math.isfinite(v) for v in l) or not top > 0.0:
        return None, -1
    l = [max(v, top * FLOOR) for v in l]
    vals = []
    for k in range(kmax + 1):
        Lk = log_likelihood(l, k)
        pen = k * (2 * N - k)
        vals.append(-2.0 * K * Lk + 2.0 * pen if method == AIC else -K * Lk + 0.5 * pen * math.log(K))
    vals = np.array(vals)
    return vals, int(np.argmin(vals))        # argmin: the first (smallest k) of the minima


def margin(vals):
    """(best - runner-up distance, scale max(1, |best|)) of one item's criterion values."""
    s = np.sort(vals)
    return (float(s[1] - s[0]) if len(s) > 1 else math.inf), max(1.0, abs(float(s[0])))


def source_count(R_items, N, K, method, kmax=None):
    """counts int32 [n], eigenvalues float64 [n, N], decided [n] bool: items whose margin exceeds 1e-6 max(1, |best|)
    (or whose status is -1), i.e. those on which a double implementation of the same criterion must agree."""
    R = np.asarray(R_items).reshape(-1, N * N)
    n = R.shape[0]
    counts = np.empty(n, np.int32)
    eig = np.empty((n, N))
    decided = np.ones(n, bool)
    for i in range(n):
        eig[i] = eigenvalues(R[i], N)
        vals, counts[i] = criterion(eig[i], K, method, kmax)
        if vals is not None:
            gap, scale = margin(vals)
            decided[i] = gap > 1e-6 * scale
    return counts, eig, decided
