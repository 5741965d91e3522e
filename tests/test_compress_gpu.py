"""PGD.compress and the Gram calls through the frontend on the MI355X: the fixed dimension just above DEVICE_EVAL_MIN_DOFS, so
its Gram matrix comes from pgd_vec_gram and its new modes from pgd_eval_batch + ranged copies; the same model through the
numpy route (DEVICE_EVAL_MIN_DOFS raised out of reach) is the comparison."""
import numpy as np
import pytest

from pgdrome_amd import fem, model
from pgdrome_amd.model import PGD

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def hip():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def synthetic(V, Vp, seed):
    """12 modes of rank 5 plus a perturbation of 1e-9 of the modes: F = Q A + 1e-9 E on the fixed space, Q' A' on the parameter's."""
    rng = np.random.default_rng(seed)
    K, r = 12, 5
    mats = []
    for W, eps in ((V, 1e-9), (Vp, 0.0)):
        n = W.dim()
        Q = np.linalg.qr(rng.standard_normal((n, r)))[0]
        E = rng.standard_normal((n, K))
        mats.append(Q @ rng.standard_normal((r, K)) + eps * E / np.linalg.norm(E, axis=0))
    modes = []
    for W, F in zip((V, Vp), mats):
        fs = []
        for k in range(K):
            f = fem.Function(W)
            f.vector()._host = np.ascontiguousarray(F[:, k])
            f.vector().touched_host()
            fs.append(f)
        modes.append(fs)
    return PGD(name="synthetic", n_modes=K, fmeshes=[V.mesh(), Vp.mesh()], pgd_modes=modes, name_coord=["x", "p"],
               modes_info=["U", "Node", "Vector" if V._ncomp > 1 else "Scalar"])


def host_modes(sol, d):
    return np.stack([f.vector().host() for f in sol.mesh[d].attributes[0].interpolationfct[:sol.used_numModes]], axis=1)


@pytest.mark.parametrize("space", ["scalar-41", "vector-29"])
def test_compress_on_the_device_equals_the_numpy_route(hip, monkeypatch, space):
    if space == "scalar-41":
        V = fem.FunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 40, 40, 40), "CG", 1)
        assert V.dim() == 68921
    else:
        V = fem.VectorFunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 28, 28, 28), "CG", 1)
        assert V.dim() == 3 * 24389
    assert V.dim() >= model.DEVICE_EVAL_MIN_DOFS
    Vp = fem.FunctionSpace(fem.IntervalMesh(32, 0.0, 1.0), "CG", 1)
    sol = synthetic(V, Vp, 41 if space == "scalar-41" else 29)

    calls, batches = fem.STATS.get("gram_calls", 0), fem.STATS.get("compress_eval_batch_calls", 0)
    dev = sol.compress(tol=TOL)
    assert fem.STATS.get("gram_calls", 0) == calls + 1                       # the fixed dimension; the 33 nodes stay in numpy
    assert fem.STATS.get("compress_eval_batch_calls", 0) == batches + 1
    G_dev = sol.mode_gram(0)
    with monkeypatch.context() as m:
        m.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 40)
        calls = fem.STATS.get("gram_calls", 0)
        ref = sol.compress(tol=TOL)
        G_np = sol.mode_gram(0)
        assert fem.STATS.get("gram_calls", 0) == calls
    a, b = dev.compression, ref.compression
    print("device:", a, "\nnumpy: ", b, "\nGram blocks differ by", np.abs(G_dev - G_np).max() / np.abs(G_np).max())
    assert np.array_equal(G_dev, G_dev.T) and np.abs(G_dev - G_np).max() <= 1e-13 * np.abs(G_np).max()
    assert a["modes_out"] == 5 == b["modes_out"] == dev.numModes and a["converged"] and a["modes_in"] == 12
    assert a["ranks"] == b["ranks"] == [5, 5]
    assert abs(a["rel_error"] - b["rel_error"]) <= 1e-9 * abs(b["rel_error"])
    # the same modes from both routes: every mode within 1e-9 of its norm (Euclidean distance of the dof vectors; PGD.distance
    # of the two results is printed - it cannot resolve 1e-9)
    for d in (0, 1):
        Fd, Fr = host_modes(dev, d), host_modes(ref, d)
        assert Fd.shape == Fr.shape == (sol.mesh[d].attributes[0].interpolationfct[0].function_space().dim(), 5)
        gap = np.linalg.norm(Fd - Fr, axis=0) / np.linalg.norm(Fr, axis=0)
        print("dimension", d, "modes differ by", gap.max())
        assert np.all(gap <= 1e-9)
    print("distance(device, numpy) =", dev.distance(ref))
    # the modes own their vectors on the fixed space
    f0 = dev.mesh[0].attributes[0].interpolationfct
    assert all(isinstance(f, fem.Function) and f.function_space() is V for f in f0) and len({id(f.vector()) for f in f0}) == 5

    # online evaluation of the compressed model against the original
    coords = np.random.default_rng(17).uniform(0.0, 1.0, size=(17, 1))
    full, small = (s.evaluate_many(0, [1], coords, 0, fields=True) for s in (sol, dev))
    U = np.array([f.vector().host() for f in full.fields])
    Uc = np.array([f.vector().host() for f in small.fields])
    print("max field difference / max |u| =", np.abs(U - Uc).max() / np.abs(U).max())
    assert np.abs(U - Uc).max() <= 2 * TOL * np.abs(U).max()
    dist = sol.distance(dev)
    print("distance(original, compressed) =", dist)
    assert dist <= TOL + 1e-7
    # the norms of those fields from one Gram matrix
    norms = sol.evaluate_norm_many(0, [1], coords, 0)
    assert np.all(np.abs(norms - np.linalg.norm(U, axis=1)) <= 1e-12 * np.linalg.norm(U, axis=1).max())
