"""numpy restatement of every output of the batched online evaluation (``pgd_eval_batch`` / ``PGD.evaluate_many``), given
the mode matrix F (n x K), the coefficients C (K x S) and a threshold.

Integer data: the product in int64, exact.  Floating-point data: the product in ``np.longdouble`` (64-bit mantissa here,
asserted) or, where the platform's long double is no wider than a double, in ``fractions.Fraction``.  The same call
returns B[i, j] = sum_k |C_kj| |F_ik|, the scale of the rounding-error bound (K + 2) 2^-53 B that holds for any summation
order, fused or not."""
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53


def product(F, C):
    F, C = np.asarray(F), np.asarray(C)
    if np.issubdtype(F.dtype, np.integer) and np.issubdtype(C.dtype, np.integer):
        return F.astype(np.int64) @ C.astype(np.int64)
    if np.finfo(np.longdouble).nmant >= 63:
        return F.astype(np.longdouble) @ C.astype(np.longdouble)
    Ff = [[Fraction(float(v)) for v in row] for row in F]
    Cf = [[Fraction(float(v)) for v in row] for row in C]
    out = np.empty((F.shape[0], C.shape[1]), dtype=object)
    for i in range(F.shape[0]):
        for j in range(C.shape[1]):
            out[i, j] = sum(Ff[i][k] * Cf[k][j] for k in range(F.shape[1]))
    return out


def evaluate_many_reference(F, C, threshold):
    """dict: U (n x S), min / max / max_abs (S), env_min / env_max (n), exceed (n, counts of U > threshold), B (n x S)."""
    U = product(F, C)
    if U.dtype == object:
        V = np.array([[float(v) for v in row] for row in U])
        exceed = np.array([[v > Fraction(float(threshold)) for v in row] for row in U]).sum(axis=1)
        U = V
    else:
        exceed = (U > threshold).sum(axis=1)
    B = np.abs(np.asarray(F, dtype=np.float64)) @ np.abs(np.asarray(C, dtype=np.float64))
    return {"U": U, "min": U.min(axis=0), "max": U.max(axis=0), "max_abs": np.abs(U).max(axis=0),
            "env_min": U.min(axis=1), "env_max": U.max(axis=1), "exceed": exceed, "B": B}


def bound(K, B):
    """|fl(sum_k c_k f_k) - exact| <= (K + 2) 2^-53 sum_k |c_k| |f_k| for any order of K products and K - 1 additions
    (gamma_K <= K u / (1 - K u); the two spare units cover the 1 / (1 - K u) factor and the rounding of the reference)."""
    return (K + 2) * U53 * B
