"""Helpers of tests/test_eval_gradient_fused_gpu.py: the calls of pgd_eval_batch_grad with every output, the same inputs through
the two stored stages, and the references - per mode ``planes`` and then ``evaluate_norm_reference`` of
tests/eval_gradient_reference.py, which is what the entry point is specified by."""
import numpy as np

from tests.eval_gradient_reference import LD, evaluate_norm_reference, norm_bound, plane_bound, planes
from tests.eval_many_reference import U53

POISON = -12345.678
KEYS = ("stats", "env_min", "env_max", "exceed", "fields")


class Layouts:
    """The scalar layout of a mesh and its blocked layouts on the device, freed on the way out."""

    def __init__(self, ctx, X, cells):
        self.ctx, self.h = ctx, {1: ctx.mesh_upload(X, cells)}

    def __getitem__(self, ncomp):
        if ncomp not in self.h:
            self.h[ncomp] = self.ctx.mesh_blocked(self.h[1], ncomp)
        return self.h[ncomp]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in list(self.h.values())[::-1]:
            self.ctx.mesh_free(h)


def upload_nodal(ctx, U):
    """U: (K, nodes, ncomp) -> one vector of nodes * ncomp entries per mode (node * ncomp + c)."""
    return [ctx.vec_from(np.ascontiguousarray(U[k], dtype=np.float64).reshape(-1)) for k in range(U.shape[0])]


def _outputs(ctx, nc, S, call):
    emn, emx, exc, fld = ctx.vec_alloc(nc), ctx.vec_alloc(nc), ctx.vec_alloc(nc), ctx.vec_alloc(nc * S)
    try:
        for v in (emn, emx, exc, fld):
            ctx.vec_fill(v, POISON)                       # an entry the kernel fails to write must not look like a result
        try:
            st = call(emn, emx, exc, fld)
        except Exception as exc_:
            st = exc_
        out = {"stats": st, "env_min": ctx.vec_download(emn), "env_max": ctx.vec_download(emx), "exceed": ctx.vec_download(exc),
               "fields": ctx.vec_download(fld).reshape(S, nc)}
    finally:
        for v in (emn, emx, exc, fld):
            ctx.vec_free(v)
    return out


def run_fused(ctx, lay, modes, L, Cm, nc, threshold, scale=0):
    """Every output of one pgd_eval_batch_grad call: dict of numpy arrays (fields as (S, cells)); where the call raises, "stats" is
    the exception and the vectors are as the call left them."""
    Cm = np.asarray(Cm, dtype=np.float64)
    return _outputs(ctx, nc, Cm.shape[1], lambda emn, emx, exc, fld: ctx.eval_batch_grad(
        lay, modes, np.asarray(L, dtype=np.float64), Cm, scale=scale, stats=True, env_min=emn, env_max=emx, exceed=exc,
        threshold=threshold, fields=fld))


def run_stored(ctx, lay, modes, L, Cm, nc, threshold, scale=0):
    """The same outputs from pgd_cell_gradient per mode and pgd_eval_batch_norm on the planes."""
    L, Cm = np.asarray(L, dtype=np.float64), np.asarray(Cm, dtype=np.float64)
    q = L.shape[0]
    pl = [ctx.vec_alloc(q * nc) for _ in modes]
    try:
        for m, p in zip(modes, pl):
            ctx.cell_gradient(lay, m, L, p, scale)
        return _outputs(ctx, nc, Cm.shape[1], lambda emn, emx, exc, fld: ctx.eval_batch_norm(
            pl, q, Cm, stats=True, env_min=emn, env_max=emx, exceed=exc, threshold=threshold, fields=fld))
    finally:
        for p in pl:
            ctx.vec_free(p)


def integer_data(rng, nv, nc, G, ncomp, q, K, S, with_scale):
    """Integer nodal values in [-7, 7], L in [-4, 4], scale in [-3, 3] or none, coefficients in [-7, 7]."""
    U = rng.integers(-7, 8, size=(K, nv, ncomp))
    L = rng.integers(-4, 5, size=(q, ncomp * G))
    scale = rng.integers(-3, 4, size=nc) if with_scale else None
    return U, L, scale, rng.integers(-7, 8, size=(K, S))


def integer_reference(X, cells, U, L, scale, Cm):
    """(reference dict, threshold) on integer data: the planes per mode in int64 (verified exact), the sums of squares in int64, the
    threshold sqrt(N + 0.5) with N an integer near the median of the sums - no value is nearer to it than about 0.25 / sqrt(N)."""
    P = np.stack([planes(X, cells, U[k], L, scale) for k in range(U.shape[0])])          # (K, q, cells)
    assert P.dtype == np.int64
    ref = evaluate_norm_reference(P, Cm, None)
    assert ref["SS"].dtype == np.int64 and int(ref["SS"].max()) < 2 ** 53
    spread = np.sort(ref["SS"].reshape(-1))
    threshold = float(np.sqrt(float(spread[len(spread) // 2]) + 0.5))
    return evaluate_norm_reference(P, Cm, threshold), threshold


def close(got, want):
    """Within one ulp of the correctly rounded root of the exact integer (the root is the one rounded operation)."""
    return bool(np.all(np.abs(got - want) <= np.spacing(want)))


def assert_integer_outputs(out, ref, tag):
    assert not isinstance(out["stats"], Exception), (tag, out["stats"])
    assert close(out["fields"], ref["V"].T), tag
    assert close(out["stats"][0], ref["min"]) and close(out["stats"][1], ref["max"]), tag
    assert np.array_equal(out["stats"][2], out["stats"][1]), tag
    assert close(out["env_min"], ref["env_min"]) and close(out["env_max"], ref["env_max"]), tag
    assert np.array_equal(out["exceed"], ref["exceed"]), tag


def float_reference(X, cells, U, L, scale, Cm, threshold):
    """(reference dict, bound (cells, S)) on floating-point data against long double: with P_t the planes of mode t and b_t =
    ``plane_bound`` of mode t (what the per-cell arithmetic may be off by), a code that forms the planes per mode and combines them
    has u_i off by at most e_i = sum_t |c_t| b_t,i + (K + 2) u sum_t |c_t| (|P_t,i| + b_t,i) - the terms of ``loop_reference`` that
    belong to this path (it gets the nodal modes themselves, so nothing shifts them) - and the value by ``norm_bound(e, V)``."""
    K = U.shape[0]
    P = np.stack([planes(X, cells, U[k], L, scale) for k in range(K)])                   # (K, q, cells), long double
    assert P.dtype == LD
    b = np.stack([plane_bound(X, cells, U[k], L, scale) for k in range(K)])              # (K, q, cells)
    ref = evaluate_norm_reference(P, Cm, threshold)
    ca = np.abs(np.asarray(Cm, dtype=np.float64))                                        # (K, S)
    Pa = np.abs(P.astype(np.float64))
    e = np.einsum("tie,ts->ies", b, ca) + (K + 2) * U53 * np.einsum("tie,ts->ies", Pa + b, ca)
    return ref, norm_bound(e, ref["V"])
