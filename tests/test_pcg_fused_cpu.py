"""The overlapped tiles of the fused PCG march (PGD_TUNE_PCG_FUSED_MARCH), restated in numpy (tests/pcg_fused_tiles.py): per tile and
z-chunk, with a halo of two, q = A p, r' = r - alpha q and p' = r' + beta p on patch + ring and then A p' on the patch.  Checked on the
grids, Dirichlet sets and march lengths of tests/test_pcg_fused_gpu.py:
  * the per-tile results assemble to the global r - alpha A p, r' + beta p and A p' with np.array_equal (the same operation order on
    both sides);
  * every row is owned by exactly one tile;
  * no tile reads outside its windows: everything outside them is NaN when the tile computes.
No GPU."""
import numpy as np
import pytest

from tests.pcg_fused_tiles import global_results, tile_results, tiles

GRIDS = {"130x37x41": (130, 37, 41), "65x4x9": (65, 4, 9)}


def system(name, bc):
    nx, ny, nz = GRIDS[name]
    shape = (nz, ny, nx)
    free = np.zeros(shape, bool)
    free[1:-1, 1:-1, 1:-1] = True                                           # the hull is eliminated
    if bc == "hull+column":
        free[:, min(2, ny - 2), min(5, nx - 2)] = False                     # an interior column through all planes
    rng = np.random.default_rng(57)
    c = rng.uniform(-1, 1, 8)
    c[0] = 9.0
    p, r = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)             # non-zero on the eliminated rows too
    return shape, free, c, p, r


@pytest.mark.parametrize("py", [16, 8])
@pytest.mark.parametrize("L", [3, 7, 1000])
@pytest.mark.parametrize("bc", ["hull", "hull+column"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_overlapped_tiles_assemble_to_the_global_update_and_product(name, bc, L, py):
    shape, free, c, p, r = system(name, bc)
    alpha, beta = 0.37, 0.81
    rn_ref, pn_ref, apn_ref = global_results(c, free, p, r, alpha, beta, py)
    assert np.isfinite(apn_ref).all()
    rn, pn, apn = (np.full(shape, np.nan) for _ in range(3))
    owners = np.zeros(shape, int)
    for tile in tiles(shape, L, py):
        own, t_rn, t_pn, t_apn = tile_results(c, free, p, r, alpha, beta, tile, py)
        owners[own] += 1
        rn[own], pn[own], apn[own] = t_rn, t_pn, t_apn
    assert (owners == 1).all()
    assert np.array_equal(rn, rn_ref) and np.array_equal(pn, pn_ref) and np.array_equal(apn, apn_ref)


def test_the_poison_is_seen():
    """A tile that reached one cell beyond its halo of two would read NaN: shrink the window by hand and the result is not finite."""
    shape, free, c, p, r = system("130x37x41", "hull")
    own, t_rn, t_pn, t_apn = tile_results(c, free, p, r, 0.3, 0.7, (64, 16, 7, 14))
    assert np.isfinite(t_apn).all()
    p2 = p.copy()
    p2[6, 14, 62] = np.nan                                                  # plane za - 1, the ring's corner (y0 - 1, x0 - 1)'s own neighbour
    p2[5, 14, 62] = np.nan                                                  # plane za - 2, halo of two
    _, _, _, t2 = tile_results(c, free, p2, r, 0.3, 0.7, (64, 16, 7, 14))
    assert np.isnan(t2).any()
    p3 = p.copy()
    p3[4, :, :] = np.nan                                                    # plane za - 3: never read
    p3[:, 13, :] = np.nan                                                   # row y0 - 3
    p3[:, :, 61] = np.nan                                                   # column x0 - 3
    _, _, _, t3 = tile_results(c, free, p3, r, 0.3, 0.7, (64, 16, 7, 14))
    assert np.array_equal(t3, t_apn)
