// Point sets: which cell of a mesh holds a point, with which barycentric coordinates (pgd_points_locate), and the values or the
// gradients of a nodal field there (pgd_points_sample).  The sensor side of the online phase: a few hundred points of the large
// dimension, all modes - the modes stay on the device, a sampled mode is a vector of points x components entries.
//
//   - ONE routine forms the affine map of a cell from its own vertices (cell_map: edge matrix, cofactors, determinant - what
//     cell_inverse of pgd_eval.hip computes for the cell gradients) and one the barycentric coordinates of a point under it
//     (cell_bary).  Both are compiled with contraction off and spell their fused operations out, so the general kernel, the lattice
//     path, the finishing pass and the sampling kernel get the same bits from the same cell and point wherever they are inlined.
//   - The rule: the cell with the largest smallest barycentric coordinate, the lowest cell index among equal minima; -1 where
//     that maximum is below -tol or is not a number.  (minimum, cell) pairs under "larger minimum, then lower cell" are totally
//     ordered and taking the best of two is exact, associative and commutative: no floating-point sum is involved, so the result
//     cannot depend on how the cells are dealt over threads and workgroups.
//   - k_locate_cells (any mesh): a tile of LOC_PT points per launch in LDS, read at addresses that are uniform across the wave;
//     persistent workgroups stride over the cells, a thread forms the map of a cell once and tests the whole tile against it,
//     keeping the best pair per point in registers.  One row of LOC_PT pairs per workgroup, k_locate_finish takes the rows in
//     ascending order (no atomics), applies tol and writes cell and lam of the winner - recomputed by cell_bary, the same bits.
//   - k_locate_lattice (Mesh::lattice_regular): a thread per point, the 6 tetrahedra of the up to 27 cubes around the point's cube
//     in ascending cell order under the same rule.
//   - k_locate_index (any 2-D or 3-D mesh, PGD_TUNE_LOCATE_INDEX): a thread per point over the cells registered in the point's bin
//     of a uniform grid over the mesh's bounding box (Mesh::loc_index, built on the device once per mesh: k_index_bounds,
//     k_index_count, scan, k_index_fill), under the same rule.
#include "pgd_internal.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace pgd {

constexpr int LOC_PT = 32;                 // points per launch of k_locate_cells: 3 registers each for the running best (96 of ~150 VGPRs: 3 waves per SIMD)
constexpr double LOC_LATTICE_TOL = 0.125;  // the lattice path serves tolerances up to here (why: k_locate_lattice)
constexpr double LOC_INDEX_TOL = 0x1p-10;  // the bin index serves tolerances up to here (why: k_locate_index)
constexpr double LOC_INDEX_SLACK = 0x1p-20;      // ... and edge matrices of condition up to about 2^30 (part (b) of the argument there)
constexpr int LOC_INDEX_TARGET_3D = 48, LOC_INDEX_TARGET_2D = 8;      // cells per bin the grid aims at: a bin edge of two lattice steps
constexpr int64_t LOC_INDEX_CAP = 16;      // entries per cell beyond which the grid is coarsened

struct Points : Obj {
    int gdim = 0;
    int64_t npts = 0, nc = 0;       // nc: cells of the mesh the set was made on
    int64_t first_outside = -1;     // first point whose cell is -1 (host knowledge: pgd_points_sample refuses without a launch)
    int *cells = nullptr;           // npts
    double *lam = nullptr;          // npts x (gdim + 1), row-major
    size_t cells_bytes = 0, lam_bytes = 0;
    ~Points() override {
        if (cells) dev_release(ctx, cells, cells_bytes);
        if (lam) dev_release(ctx, lam, lam_bytes);
    }
};
constexpr Obj::Kind POINTS = Obj::POINTS;
static inline Points *get_points(Ctx *c, pgd_handle h) { return static_cast<Points *>(get_obj(c, h, POINTS)); }

// the vertices of cell e: the first G + 1 entries of its record, whichever way the layout stores it
template <int G>
__device__ __forceinline__ void cell_vertices(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn, int64_t e, int (&v)[G + 1]) {
    if (cellsN) {
        const int *rec = cellsN + e * nn;
#pragma unroll
        for (int a = 0; a <= G; ++a) v[a] = rec[a];
    } else {
        const int4 r = cells4[e];
        const int u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int a = 0; a <= G; ++a) v[a] = u[a];
    }
}

// J[a][d] = d xi_a / d x_d = inv(E^T), E[a][d] = x_{a+1}[d] - x_0[d], from cofactors and the determinant; x0 = vertex 0.
// false: the determinant is zero or not finite (a degenerate cell: never chosen by the location; a set made by pgd_points_from may
// name one - its caller answers for it, the gradients sampled there are not numbers)
template <int G>
__device__ __forceinline__ bool cell_map(const int (&v)[G + 1], const double *__restrict__ coords, int64_t nv, double (&J)[G][G], double (&x0)[G]) {
#pragma clang fp contract(off)
    double E[G][G];
#pragma unroll
    for (int d = 0; d < G; ++d) {
        const double *x = coords + (int64_t)d * nv;
        x0[d] = x[v[0]];
#pragma unroll
        for (int a = 0; a < G; ++a) E[a][d] = x[v[a + 1]] - x0[d];
    }
    double det;
    if constexpr (G == 1) {
        det = E[0][0];
        J[0][0] = 1.0 / det;
    } else if constexpr (G == 2) {
        det = fma(E[0][0], E[1][1], -(E[0][1] * E[1][0]));
        const double inv = 1.0 / det;
        J[0][0] = E[1][1] * inv;  J[0][1] = -E[1][0] * inv;
        J[1][0] = -E[0][1] * inv; J[1][1] = E[0][0] * inv;
    } else {
        double C[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
                C[a][d] = fma(E[a1][d1], E[a2][d2], -(E[a1][d2] * E[a2][d1]));
            }
        }
        det = fma(E[0][2], C[0][2], fma(E[0][1], C[0][1], E[0][0] * C[0][0]));
        const double inv = 1.0 / det;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) J[a][d] = C[a][d] * inv;
    }
    return det != 0.0 && fabs(det) <= 1.79769313486231570e308;      // (a NaN fails both)
}

// lam_{a+1} = sum_d J[a][d] (x_d - x0_d), lam_0 = 1 - sum_a lam_{a+1}; returns the smallest - a NaN where any of them is one
template <int G>
__device__ __forceinline__ double cell_bary(const double (&J)[G][G], const double (&x0)[G], const double (&x)[G], double (&lam)[G + 1]) {
#pragma clang fp contract(off)
    double dx[G];
#pragma unroll
    for (int d = 0; d < G; ++d) dx[d] = x[d] - x0[d];
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < G; ++a) {
        double acc = J[a][0] * dx[0];
#pragma unroll
        for (int d = 1; d < G; ++d) acc = fma(J[a][d], dx[d], acc);
        lam[a + 1] = acc;
        sum = sum + acc;
    }
    lam[0] = 1.0 - sum;
    double mn = lam[0];
    bool nan = !(mn == mn);
#pragma unroll
    for (int a = 1; a <= G; ++a) {
        nan = nan || !(lam[a] == lam[a]);
        mn = lam[a] < mn ? lam[a] : mn;
    }
    return nan ? __builtin_nan("") : mn;
}

// is (m, e) better than (bm, be)?  A NaN minimum never is
__device__ __forceinline__ bool loc_better(double m, int e, double bm, int be) { return m > bm || (m == bm && be >= 0 && e >= 0 && e < be); }

constexpr double LOC_NONE = -std::numeric_limits<double>::infinity();

// ---- the general kernel: cells over persistent workgroups, a tile of np <= LOC_PT points (pts + p0 G ...) per launch
template <int G>
__global__ __launch_bounds__(TPB) void k_locate_cells(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                      const double *__restrict__ coords, int64_t nv, int64_t nc, const double *__restrict__ pts,
                                                      int np, double *__restrict__ part_min, int *__restrict__ part_cell) {
    __shared__ double s_x[LOC_PT * G];
    __shared__ double s_min[TPB / WAVE][LOC_PT];
    __shared__ int s_cell[TPB / WAVE][LOC_PT];
    for (int i = threadIdx.x; i < LOC_PT * G; i += TPB) s_x[i] = i < np * G ? pts[i] : __builtin_nan("");
    __syncthreads();
    double bm[LOC_PT];
    int bc[LOC_PT];
#pragma unroll
    for (int p = 0; p < LOC_PT; ++p) { bm[p] = LOC_NONE; bc[p] = -1; }
    const int64_t stride = (int64_t)gridDim.x * TPB;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < nc; e += stride) {      // ascending per thread: a strict > keeps the lowest cell
        int v[G + 1];
        double J[G][G], x0[G];
        cell_vertices<G>(cells4, cellsN, nn, e, v);
        if (!cell_map<G>(v, coords, nv, J, x0)) continue;
        // the tile is read from LDS for every cell (broadcast reads, a few per ~30 f64 operations): hoisted out of the loop it would
        // take 2 G LOC_PT registers per lane and leave one wave per SIMD to hide the gathers of cell_map
        __asm__ volatile("" ::: "memory");
#pragma unroll
        for (int p = 0; p < LOC_PT; ++p) {
            double x[G], lam[G + 1];
#pragma unroll
            for (int d = 0; d < G; ++d) x[d] = s_x[p * G + d];      // the same address in every lane
            const double m = cell_bary<G>(J, x0, x, lam);
            if (m > bm[p]) { bm[p] = m; bc[p] = (int)e; }
        }
    }
    // the best pair per point over the workgroup: across the wave by shuffles, across the four waves in thread order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < LOC_PT; ++p) {
        double m = bm[p];
        int e = bc[p];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double m2 = __shfl_down(m, off, 64);
            const int e2 = __shfl_down(e, off, 64);
            if (loc_better(m2, e2, m, e)) { m = m2; e = e2; }
        }
        if (lane == 0) { s_min[wv][p] = m; s_cell[wv][p] = e; }
    }
    __syncthreads();
    if (threadIdx.x < LOC_PT) {
        const int p = threadIdx.x;
        double m = s_min[0][p];
        int e = s_cell[0][p];
#pragma unroll
        for (int w = 1; w < TPB / WAVE; ++w)
            if (loc_better(s_min[w][p], s_cell[w][p], m, e)) { m = s_min[w][p]; e = s_cell[w][p]; }
        part_min[(int64_t)blockIdx.x * LOC_PT + p] = m;
        part_cell[(int64_t)blockIdx.x * LOC_PT + p] = e;
    }
}

// the cell of a point once its best pair is known: -1 below -tol (or where nothing was comparable), else lam from cell_bary again
template <int G>
__device__ __forceinline__ void locate_store(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn, const double *__restrict__ coords,
                                             int64_t nv, const double (&x)[G], double m, int e, double tol, int *__restrict__ cell_out,
                                             double *__restrict__ lam_out) {
    double lam[G + 1];
#pragma unroll
    for (int a = 0; a <= G; ++a) lam[a] = 0.0;
    if (e >= 0 && m >= -tol) {
        int v[G + 1];
        double J[G][G], x0[G];
        cell_vertices<G>(cells4, cellsN, nn, e, v);
        (void)cell_map<G>(v, coords, nv, J, x0);
        (void)cell_bary<G>(J, x0, x, lam);
    } else {
        e = -1;
    }
    *cell_out = e;
#pragma unroll
    for (int a = 0; a <= G; ++a) lam_out[a] = lam[a];
}

// the rows of the g workgroups in ascending order, a thread per point of the tile
template <int G>
__global__ __launch_bounds__(WAVE) void k_locate_finish(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                        const double *__restrict__ coords, int64_t nv, const double *__restrict__ pts, int np,
                                                        const double *__restrict__ part_min, const int *__restrict__ part_cell, int g, double tol,
                                                        int *__restrict__ cell_out, double *__restrict__ lam_out) {
    const int p = threadIdx.x;
    if (p >= np) return;
    double m = LOC_NONE;
    int e = -1;
    for (int b = 0; b < g; ++b) {
        const double m2 = part_min[(int64_t)b * LOC_PT + p];
        const int e2 = part_cell[(int64_t)b * LOC_PT + p];
        if (loc_better(m2, e2, m, e)) { m = m2; e = e2; }      // (a pair with a cell has a minimum above LOC_NONE)
    }
    double x[G];
#pragma unroll
    for (int d = 0; d < G; ++d) x[d] = pts[p * G + d];
    locate_store<G>(cells4, cellsN, nn, coords, nv, x, m, e, tol, cell_out + p, lam_out + (int64_t)p * (G + 1));
}

// ---- the lattice path: cell 6 q + t is tetrahedron t of cube q, cubes in vertex order (Mesh::lattice_regular).  A thread per point.
// The cube of the point follows from (x - origin) / h, clamped to the lattice; the candidates are the cubes within one step of it.
// Why they suffice for tol <= LOC_LATTICE_TOL: a cell of cube c with all lam >= -tol holds x = sum_i lam_i v_i with every vertex
// coordinate c_a or c_a + h_a, so (x_a - c_a) / h_a is a sum of at most three lam_i (not all four, or the cell were flat) and lies in
// [-3 tol, 1 + 3 tol], inside (-0.4, 1.4): the exact cube index of x differs from c by at most one per axis, and clamping towards
// the lattice - c is on it - never increases the difference.  The vertices lie within 8 eps times the EXTENT of the lattice of their
// exact places (the check at upload, k_lattice_verify), which is 8 eps n steps for n vertices along the axis, and the subtraction and
// the division add a few units in the last place of the quotient (at most n): the computed quotient is off by about 10 eps n steps,
// 1e-8 of a step at n = 10^7, so its floor can be off by one only where x is within that distance of a cube boundary - there the cells with lam >= -tol lie in the two cubes on either side
// of it, both within one step of either floor.  Off by more than one would take an error of 0.6 steps: impossible for finite
// input.  An infinite coordinate is clamped like any other and fails every test, a NaN fails every test from any cube.
__global__ __launch_bounds__(TPB) void k_locate_lattice(const int4 *__restrict__ cells4, const double *__restrict__ coords, int64_t nv, int nx, int ny,
                                                        int nz, double hx, double hy, double hz, const double *__restrict__ pts, int64_t npts,
                                                        double tol, int *__restrict__ cell_out, double *__restrict__ lam_out) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= npts) return;
    const double x[3] = {pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2]};
    const double h[3] = {hx, hy, hz};
    const int ncube[3] = {nx - 1, ny - 1, nz - 1};
    int q0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double o = coords[(int64_t)a * nv];                  // vertex 0 is the lattice's origin
        double f = floor((x[a] - o) / h[a]);
        f = f >= 0.0 ? f : 0.0;                                    // (a NaN becomes 0)
        f = f <= (double)(ncube[a] - 1) ? f : (double)(ncube[a] - 1);
        q0[a] = (int)f;
    }
    double bm = LOC_NONE;
    int be = -1;
    for (int dz = -1; dz <= 1; ++dz) {
        const int cz = q0[2] + dz;
        if (cz < 0 || cz >= ncube[2]) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int cy = q0[1] + dy;
            if (cy < 0 || cy >= ncube[1]) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int cx = q0[0] + dx;
                if (cx < 0 || cx >= ncube[0]) continue;
                const int64_t q = cx + (int64_t)ncube[0] * (cy + (int64_t)ncube[1] * cz);
                for (int t = 0; t < 6; ++t) {                      // ascending cell index throughout: a strict > keeps the lowest
                    const int64_t e = 6 * q + t;
                    int v[4];
                    double J[3][3], x0[3], lam[4];
                    cell_vertices<3>(cells4, nullptr, 0, e, v);
                    if (!cell_map<3>(v, coords, nv, J, x0)) continue;
                    const double m = cell_bary<3>(J, x0, x, lam);
                    if (m > bm) { bm = m; be = (int)e; }
                }
            }
        }
    }
    locate_store<3>(cells4, nullptr, 0, coords, nv, x, bm, be, tol, cell_out + p, lam_out + p * 4);
}

// ---- the bin index: a uniform grid of n[0] x n[1] x n[2] bins over the bounding box of the mesh (origin o, inv = n / extent per
// axis; n = 1 and inv = 0 on an axis the mesh does not have or does not extend along), CSR-like: the cells registered in bin b are
// bin_cells[bin_ptr[b] .. bin_ptr[b + 1]).  A cell is registered in every bin that its INFLATED bounding box touches.
struct LocGrid {
    double o[3], inv[3];
    int n[3];
};

// the bin of a coordinate along one axis - the ONE function that the count, the fill and the query share.  Clamped: a coordinate
// outside the box lands in the first or last bin, a NaN (also inf * 0 on a flat axis) in bin 0
__device__ __forceinline__ int bin_of(double x, double o, double inv, int n) {
#pragma clang fp contract(off)
    double f = floor((x - o) * inv);
    f = f >= 0.0 ? f : 0.0;                                    // (a NaN becomes 0)
    f = f <= (double)(n - 1) ? f : (double)(n - 1);
    return (int)f;
}

// the bounding box of cell e over its vertices (the first G + 1 record entries); comparisons only
template <int G>
__device__ __forceinline__ void cell_box(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn, const double *__restrict__ coords,
                                         int64_t nv, int64_t e, double (&lo)[G], double (&hi)[G]) {
    int v[G + 1];
    cell_vertices<G>(cells4, cellsN, nn, e, v);
#pragma unroll
    for (int d = 0; d < G; ++d) {
        const double *x = coords + (int64_t)d * nv;
        lo[d] = hi[d] = x[v[0]];
#pragma unroll
        for (int a = 1; a <= G; ++a) {
            const double t = x[v[a]];
            lo[d] = t < lo[d] ? t : lo[d];
            hi[d] = t > hi[d] ? t : hi[d];
        }
    }
}

// the bins [r0[a], r1[a]] per axis of cell e: those of its box inflated by m_a = (G + 1) (LOC_INDEX_TOL + LOC_INDEX_SLACK) (hi_a - lo_a)
// on either side.  Contraction off, every rounding spelt out: hi - lo, K times that, lo - m, hi + m
template <int G>
__device__ __forceinline__ void index_range(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn, const double *__restrict__ coords,
                                            int64_t nv, int64_t e, const LocGrid &g, int (&r0)[3], int (&r1)[3]) {
#pragma clang fp contract(off)
    constexpr double K = (G + 1) * (LOC_INDEX_TOL + LOC_INDEX_SLACK);      // exact
    double lo[G], hi[G];
    cell_box<G>(cells4, cellsN, nn, coords, nv, e, lo, hi);
#pragma unroll
    for (int a = 0; a < 3; ++a) { r0[a] = 0; r1[a] = 0; }
#pragma unroll
    for (int a = 0; a < G; ++a) {
        const double d = hi[a] - lo[a];
        const double m = K * d;
        r0[a] = bin_of(lo[a] - m, g.o[a], g.inv[a], g.n[a]);
        r1[a] = bin_of(hi[a] + m, g.o[a], g.inv[a], g.n[a]);
    }
}

// the global box: minima and maxima of the cell boxes, per workgroup one row lo[0..G), hi[0..G) of `part` (exact and order-free:
// comparisons, no sums; the host takes the rows together)
template <int G>
__global__ __launch_bounds__(TPB) void k_index_bounds(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                      const double *__restrict__ coords, int64_t nv, int64_t nc, double *__restrict__ part) {
    __shared__ double s_box[TPB / WAVE][2 * G];
    const double inf = std::numeric_limits<double>::infinity();
    double lo[G], hi[G];
#pragma unroll
    for (int d = 0; d < G; ++d) { lo[d] = inf; hi[d] = -inf; }
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < nc; e += (int64_t)gridDim.x * TPB) {
        double l[G], h[G];
        cell_box<G>(cells4, cellsN, nn, coords, nv, e, l, h);
#pragma unroll
        for (int d = 0; d < G; ++d) {
            lo[d] = l[d] < lo[d] ? l[d] : lo[d];
            hi[d] = h[d] > hi[d] ? h[d] : hi[d];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < G; ++d) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double l2 = __shfl_down(lo[d], off, 64), h2 = __shfl_down(hi[d], off, 64);
            lo[d] = l2 < lo[d] ? l2 : lo[d];
            hi[d] = h2 > hi[d] ? h2 : hi[d];
        }
        if (lane == 0) { s_box[wv][d] = lo[d]; s_box[wv][G + d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x < G) {
        const int d = threadIdx.x;
        double l = s_box[0][d], h = s_box[0][G + d];
#pragma unroll
        for (int w = 1; w < TPB / WAVE; ++w) {
            l = s_box[w][d] < l ? s_box[w][d] : l;
            h = s_box[w][G + d] > h ? s_box[w][G + d] : h;
        }
        part[(int64_t)blockIdx.x * 2 * G + d] = l;
        part[(int64_t)blockIdx.x * 2 * G + G + d] = h;
    }
}

// cnt[b] += 1 for every bin b in the ranges of a cell; total: all registrations, in 64 bits (it decides whether the grid stands
// before anything is sized by it)
template <int G>
__global__ __launch_bounds__(TPB) void k_index_count(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                     const double *__restrict__ coords, int64_t nv, int64_t nc, LocGrid g, int *__restrict__ cnt,
                                                     unsigned long long *__restrict__ total) {
    unsigned long long mine = 0;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < nc; e += (int64_t)gridDim.x * TPB) {
        int r0[3], r1[3];
        index_range<G>(cells4, cellsN, nn, coords, nv, e, g, r0, r1);
        for (int bz = r0[2]; bz <= r1[2]; ++bz)
            for (int by = r0[1]; by <= r1[1]; ++by)
                for (int bx = r0[0]; bx <= r1[0]; ++bx) {
                    atomicAdd(&cnt[bx + g.n[0] * (by + g.n[1] * bz)], 1);
                    ++mine;
                }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, mine);
}

// the same ranges from the same function; the order inside a bin is the order of arrival.  A registration past the end of its
// bin's list cannot happen while count and fill agree - it is dropped, not stored, all the same
template <int G>
__global__ __launch_bounds__(TPB) void k_index_fill(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                    const double *__restrict__ coords, int64_t nv, int64_t nc, LocGrid g,
                                                    const int *__restrict__ bin_ptr, int *__restrict__ cursor, int *__restrict__ bin_cells) {
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < nc; e += (int64_t)gridDim.x * TPB) {
        int r0[3], r1[3];
        index_range<G>(cells4, cellsN, nn, coords, nv, e, g, r0, r1);
        for (int bz = r0[2]; bz <= r1[2]; ++bz)
            for (int by = r0[1]; by <= r1[1]; ++by)
                for (int bx = r0[0]; bx <= r1[0]; ++bx) {
                    const int b = bx + g.n[0] * (by + g.n[1] * bz);
                    const int first = bin_ptr[b], len = bin_ptr[b + 1] - first;
                    const int pos = atomicAdd(&cursor[b], 1);
                    if (pos < len) bin_cells[first + pos] = (int)e;
                }
    }
}

__global__ __launch_bounds__(TPB) void k_index_longest(const int *__restrict__ cnt, int64_t nbins, int *__restrict__ longest) {
    int m = 0;
    for (int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x; b < nbins; b += (int64_t)gridDim.x * TPB) m = cnt[b] > m ? cnt[b] : m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int m2 = __shfl_down(m, off, 64);
        m = m2 > m ? m2 : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(longest, m);
}

// ---- the indexed path: a thread per point, the cells of the point's bin under the rule.  No LDS, no barrier, no atomics.
// Why the bin's list suffices for tol <= LOC_INDEX_TOL (t below), on any mesh:
// (a) The inflated box holds the point.  A cell with all exact lam_i >= -t and sum lam = 1: write lam_i = -t + mu_i, mu >= 0,
//     sum mu = 1 + (G + 1) t.  Then x_a = sum lam_i v_ia = sum mu_i v_ia - t sum v_ia <= hi_a sum mu_i - t sum v_ia
//     = hi_a + t sum_i (hi_a - v_ia) <= hi_a + (G + 1) t (hi_a - lo_a), and likewise x_a >= lo_a - (G + 1) t (hi_a - lo_a).
// (b) The slack covers the rounding of cell_bary.  A COMPUTED minimum >= -tol means an exact minimum >= -tol - c u kappa(E), c a few
//     tens (the error of the cofactor solve, relative to lam of order one): the margin is formed with LOC_INDEX_TOL + 2^-20 in
//     place of t, which covers edge matrices of condition up to about 2^30 - THE LIMIT of this path; a mesh with worse cells keeps
//     the general kernel.  (The margin itself and lo - m, hi + m round by a relative 2^-52, far inside the 2^-20.)
// (c) Bins are monotone.  Subtracting a constant, multiplying by a non-negative constant, floor and the clamp are monotone in
//     floating point, so lo' <= x <= hi' gives bin_of(lo') <= bin_of(x) <= bin_of(hi') on every axis - no epsilon, and also for a
//     point that is clamped into the grid from outside the box: the bin of x is among those the cell was registered in.
// (d) The winner is the general kernel's.  Every cell whose computed minimum is >= -tol is therefore in the list of the point's
//     bin.  If the general kernel's winner has a minimum >= -tol, it is in the list, and so is every cell tied with it (the same
//     minimum); the best pair over a subset that holds the overall best pair is that pair - loc_better is a total order, and the
//     list is walked with it because the list is not ascending.  Otherwise no listed cell reaches -tol either (the list is a
//     subset), and both paths store -1 and zeros.  A NaN or infinite coordinate fails every test in any bin, as in any cell.
template <int G>
__global__ __launch_bounds__(TPB) void k_locate_index(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, int nn,
                                                      const double *__restrict__ coords, int64_t nv, LocGrid g, const int *__restrict__ bin_ptr,
                                                      const int *__restrict__ bin_cells, const double *__restrict__ pts, int64_t npts, double tol,
                                                      int *__restrict__ cell_out, double *__restrict__ lam_out) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= npts) return;
    double x[G];
    int q[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < G; ++d) {
        x[d] = pts[p * G + d];
        q[d] = bin_of(x[d], g.o[d], g.inv[d], g.n[d]);
    }
    const int b = q[0] + g.n[0] * (q[1] + g.n[1] * q[2]);
    const int k1 = bin_ptr[b + 1];
    double bm = LOC_NONE;
    int be = -1;
    for (int k = bin_ptr[b]; k < k1; ++k) {
        const int e = bin_cells[k];
        int v[G + 1];
        double J[G][G], x0[G], lam[G + 1];
        cell_vertices<G>(cells4, cellsN, nn, e, v);
        if (!cell_map<G>(v, coords, nv, J, x0)) continue;
        const double m = cell_bary<G>(J, x0, x, lam);
        if (loc_better(m, e, bm, be)) { bm = m; be = e; }
    }
    locate_store<G>(cells4, cellsN, nn, coords, nv, x, bm, be, tol, cell_out + p, lam_out + p * (G + 1));
}

// ---- sampling: a thread per point, the components in a loop.  P2 shape functions l (2 l - 1) and 4 l_a l_b; the edge order of the
// records (pgd_cell_gradient_p2; interval: the one edge (0, 1))
__host__ __device__ constexpr int loc_nodes(int G, int deg) { return deg == 1 ? G + 1 : (G + 1) * (G + 2) / 2; }
__host__ __device__ constexpr int loc_edge_a(int G, int k) { return G == 1 ? 0 : G == 2 ? (k == 0 ? 1 : 0) : (k == 0 ? 2 : k < 3 ? 1 : 0); }
__host__ __device__ constexpr int loc_edge_b(int G, int k) { return G == 1 ? 1 : G == 2 ? (k == 2 ? 1 : 2) : (k == 2 || k == 4 ? 2 : k == 5 ? 1 : 3); }

template <int G, int DEG>
__global__ __launch_bounds__(TPB) void k_points_sample(const int4 *__restrict__ cells4, const int *__restrict__ cellsN, const double *__restrict__ coords,
                                                       int64_t nv, const int *__restrict__ pcell, const double *__restrict__ plam, int64_t npts,
                                                       int ncomp, const double *__restrict__ u, int what, double *__restrict__ out) {
#pragma clang fp contract(off)
    constexpr int NN = loc_nodes(G, DEG);
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= npts) return;
    const int64_t e = pcell[p];       // (a set with a -1 was refused on the host: e is a cell)
    int r[NN];
    if (cellsN) {
#pragma unroll
        for (int j = 0; j < NN; ++j) r[j] = cellsN[e * NN + j];
    } else {
        const int4 rec = cells4[e];
        const int t[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
        for (int j = 0; j < NN; ++j) r[j] = t[j];
    }
    double l[G + 1];
#pragma unroll
    for (int a = 0; a <= G; ++a) l[a] = plam[p * (G + 1) + a];
    if (what == 0) {
        double N[NN];
        if constexpr (DEG == 1) {
#pragma unroll
            for (int a = 0; a <= G; ++a) N[a] = l[a];
        } else {
#pragma unroll
            for (int a = 0; a <= G; ++a) N[a] = l[a] * (2.0 * l[a] - 1.0);
#pragma unroll
            for (int k = 0; k < NN - (G + 1); ++k) N[G + 1 + k] = 4.0 * l[loc_edge_a(G, k)] * l[loc_edge_b(G, k)];
        }
        for (int c = 0; c < ncomp; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NN; ++j) acc = fma(N[j], u[(int64_t)r[j] * ncomp + c], acc);
            out[p * ncomp + c] = acc;
        }
        return;
    }
    int v[G + 1];
#pragma unroll
    for (int a = 0; a <= G; ++a) v[a] = r[a];
    double J[G][G], x0[G];
    (void)cell_map<G>(v, coords, nv, J, x0);
    for (int c = 0; c < ncomp; ++c) {
        double du[G];      // d u_c / d xi_a
        if constexpr (DEG == 1) {
            const double u0 = u[(int64_t)r[0] * ncomp + c];
#pragma unroll
            for (int a = 0; a < G; ++a) du[a] = u[(int64_t)r[a + 1] * ncomp + c] - u0;
        } else {
            // as p2_planes of pgd_eval.hip: dl_{a+1} - dl_0, the node of the edge (0, a + 1) entering once with 4 l_0 - 4 l_{a+1}
            double un[NN], w[G + 1], l4[G + 1];
#pragma unroll
            for (int j = 0; j < NN; ++j) un[j] = u[(int64_t)r[j] * ncomp + c];
#pragma unroll
            for (int a = 0; a <= G; ++a) { l4[a] = 4.0 * l[a]; w[a] = l4[a] - 1.0; }
#pragma unroll
            for (int a = 0; a < G; ++a) {
                double hi = un[a + 1] * w[a + 1], lo = un[0] * w[0], shared = 0.0;
#pragma unroll
                for (int k = 0; k < NN - (G + 1); ++k) {
                    const int ea = loc_edge_a(G, k), eb = loc_edge_b(G, k);      // ea < eb
                    const double ue = un[G + 1 + k];
                    if (ea == 0 && eb == a + 1) shared = ue;
                    else if (ea == 0) lo = fma(ue, l4[eb], lo);
                    else if (ea == a + 1) hi = fma(ue, l4[eb], hi);
                    else if (eb == a + 1) hi = fma(ue, l4[ea], hi);
                }
                du[a] = fma(shared, l4[0] - l4[a + 1], hi - lo);
            }
        }
#pragma unroll
        for (int d = 0; d < G; ++d) {
            double acc = du[0] * J[0][d];
#pragma unroll
            for (int a = 1; a < G; ++a) acc = fma(du[a], J[a][d], acc);
            out[(p * ncomp + c) * G + d] = acc;
        }
    }
}

// the scalar layout behind a layout handle (its own, or the base of a blocked one) with cell records and coordinates
static const Mesh *points_base(Ctx *c, const char *fn, pgd_handle mh, const Mesh **layout) {
    const Mesh *m = get_mesh(c, mh);
    if (!m) { fail(c, PGD_ERR_INVALID, "%s: invalid mesh handle", fn); return nullptr; }
    const Mesh *b = m->ncomp > 1 ? get_mesh(c, m->base) : m;
    if (!b) { fail(c, PGD_ERR_INVALID, "%s: the blocked layout's base is gone", fn); return nullptr; }
    if ((!b->cells && !b->cellsN) || !b->coords) { fail(c, PGD_ERR_INVALID, "%s: the layout has no cell records", fn); return nullptr; }
    if (layout) *layout = m;
    return b;
}

static int points_new(Ctx *c, int gdim, int64_t npts, int64_t nc, std::unique_ptr<Points> &P) {
    P.reset(new Points);
    P->kind = POINTS;
    P->ctx = c;
    P->gdim = gdim; P->npts = npts; P->nc = nc;
    void *q;
    P->cells_bytes = (size_t)(npts > 0 ? npts : 1) * sizeof(int);
    PGD_TRY(dev_alloc(c, &q, P->cells_bytes)); P->cells = (int *)q;
    P->lam_bytes = (size_t)(npts > 0 ? npts : 1) * (gdim + 1) * sizeof(double);
    PGD_TRY(dev_alloc(c, &q, P->lam_bytes)); P->lam = (double *)q;
    return PGD_OK;
}

template <int G>
static int locate_general(Ctx *c, const Mesh *b, const double *pts_dev, int64_t npts, double tol, Points *P) {
    int64_t g = (b->nc + TPB - 1) / TPB;
    const int64_t resident = (int64_t)c->num_cu * 3;      // three workgroups of four waves per CU at ~150 VGPRs
    if (g > resident) g = resident;
    if (c->locate_grid_max > 0 && g > c->locate_grid_max) g = c->locate_grid_max;
    if (g < 1) g = 1;
    void *q;
    const size_t pm_bytes = (size_t)g * LOC_PT * sizeof(double), pc_bytes = (size_t)g * LOC_PT * sizeof(int);
    PGD_TRY(dev_alloc(c, &q, pm_bytes));
    double *part_min = (double *)q;
    int rc = dev_alloc(c, &q, pc_bytes);
    if (rc != PGD_OK) { dev_release(c, part_min, pm_bytes); return rc; }
    int *part_cell = (int *)q;
    const int nn = b->cellsN ? b->nvpc : 0;
    for (int64_t p0 = 0; p0 < npts; p0 += LOC_PT) {      // one launch per tile: no launch grows with npts * nc
        const int np = (int)(npts - p0 < LOC_PT ? npts - p0 : LOC_PT);
        k_locate_cells<G><<<(int)g, TPB, 0, c->stream>>>(b->cells, b->cellsN, nn, b->coords, b->nv, b->nc, pts_dev + p0 * G, np, part_min, part_cell);
        k_locate_finish<G><<<1, WAVE, 0, c->stream>>>(b->cells, b->cellsN, nn, b->coords, b->nv, pts_dev + p0 * G, np, part_min, part_cell, (int)g, tol,
                                                     P->cells + p0, P->lam + p0 * (G + 1));
    }
    const hipError_t launched = hipGetLastError();
    dev_release(c, part_min, pm_bytes);      // (stream-ordered pool: a later user queues behind these launches)
    dev_release(c, part_cell, pc_bytes);
    if (launched != hipSuccess) return fail(c, PGD_ERR_HIP, "points_locate: launch failed: %s", hipGetErrorString(launched));
    return PGD_OK;
}

// ---- the bin index, host side
// bins per axis from the number of cells and the extents of the box: about `target` cells per bin, bins as cubic as the box allows.
// An axis without extent has one bin and inv = 0.  Plain double arithmetic, restated by the tests: pow, nearbyint
static void index_grid(int G, int64_t nc, int64_t target, const double *lo, const double *top, LocGrid &g, double (&L)[3]) {
    int live = 0;
    double prod = 1.0;
    for (int a = 0; a < 3; ++a) {
        L[a] = a < G ? top[a] - lo[a] : 0.0;
        if (!(L[a] > 0.0) || !std::isfinite(L[a])) L[a] = 0.0;
        g.o[a] = a < G ? lo[a] : 0.0;
        g.n[a] = 1;
        g.inv[a] = 0.0;
        if (L[a] > 0.0) { ++live; prod *= L[a]; }
    }
    if (!live) return;
    const double B = (double)nc / (double)target;
    const double s = std::pow(B / prod, 1.0 / live);
    for (int a = 0; a < 3; ++a) {
        if (!(L[a] > 0.0)) continue;
        double f = std::nearbyint(L[a] * s);
        if (!(f >= 1.0)) f = 1.0;
        if (f > 1073741824.0) f = 1073741824.0;
        g.n[a] = (int)f;
    }
    while ((double)g.n[0] * g.n[1] * g.n[2] >= 2147483647.0)
        for (int a = 0; a < 3; ++a) g.n[a] = g.n[a] > 1 ? g.n[a] / 2 : 1;
    for (int a = 0; a < 3; ++a) g.inv[a] = L[a] > 0.0 ? (double)g.n[a] / L[a] : 0.0;
}

// builds Mesh::loc_index of the scalar layout b under the current target.  Everything is queued on c->stream; the host waits for
// the box and for the number of registrations (once per coarsening).  On an error the mesh holds no index and no allocation of the build is left
template <int G>
static int index_build(Ctx *c, const Mesh *b) {
    Mesh::LocIndex &ix = b->loc_index;
    hipStream_t st = c->stream;
    const int nn = b->cellsN ? b->nvpc : 0;
    const int64_t nc = b->nc;
    const int grid = grid_for(nc);
    double *part = nullptr;
    int *cnt = nullptr, *bin_ptr = nullptr, *bin_cells = nullptr;
    unsigned long long *stats = nullptr;      // [0] registrations, [1] (as int) the longest list
    size_t part_bytes = (size_t)grid * 2 * G * sizeof(double), cnt_bytes = 0;
    auto cleanup = [&](int rc) {
        (void)hipStreamSynchronize(st);
        if (part) dev_release(c, part, part_bytes);
        if (cnt) dev_release(c, cnt, cnt_bytes);
        if (stats) (void)hipFree(stats);
        if (rc != PGD_OK) {
            if (bin_ptr) (void)hipFree(bin_ptr);
            if (bin_cells) (void)hipFree(bin_cells);
        }
        return rc;
    };
#define PGD_IX(call)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess) return cleanup(fail(c, PGD_ERR_HIP, "points index: %s", hipGetErrorString(e_)));        \
    } while (0)
#define PGD_IX_TRY(call)                                \
    do {                                                \
        const int rc_ = (call);                         \
        if (rc_ != PGD_OK) return cleanup(rc_);         \
    } while (0)
    void *q;
    PGD_IX_TRY(dev_alloc(c, &q, part_bytes)); part = (double *)q;
    PGD_IX_TRY(dev_alloc(c, &q, 2 * sizeof(unsigned long long))); stats = (unsigned long long *)q;
    k_index_bounds<G><<<grid, TPB, 0, st>>>(b->cells, b->cellsN, nn, b->coords, b->nv, nc, part);
    PGD_IX(hipGetLastError());
    std::vector<double> rows((size_t)grid * 2 * G);
    PGD_IX(hipMemcpyAsync(rows.data(), part, part_bytes, hipMemcpyDeviceToHost, st));
    PGD_IX(hipStreamSynchronize(st));
    double lo[3] = {0, 0, 0}, top[3] = {0, 0, 0};
    for (int d = 0; d < G; ++d) {
        lo[d] = rows[d]; top[d] = rows[G + d];
        for (int r = 1; r < grid; ++r) {
            const double l = rows[(size_t)r * 2 * G + d], h = rows[(size_t)r * 2 * G + G + d];
            lo[d] = l < lo[d] ? l : lo[d];
            top[d] = h > top[d] ? h : top[d];
        }
    }
    const int64_t knob = c->locate_index_target;
    const int64_t target = knob > 0 ? knob : (G == 3 ? LOC_INDEX_TARGET_3D : LOC_INDEX_TARGET_2D);
    LocGrid g;
    double L[3];
    index_grid(G, nc, target, lo, top, g, L);
    int64_t bins = (int64_t)g.n[0] * g.n[1] * g.n[2];
    cnt_bytes = (size_t)(bins + 1) * sizeof(int);      // (coarsening only shrinks the grid: sized once)
    PGD_IX_TRY(dev_alloc(c, &q, cnt_bytes)); cnt = (int *)q;
    unsigned long long total = 0;
    for (;;) {
        bins = (int64_t)g.n[0] * g.n[1] * g.n[2];
        PGD_IX(hipMemsetAsync(cnt, 0, (size_t)(bins + 1) * sizeof(int), st));
        PGD_IX(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), st));
        k_index_count<G><<<grid, TPB, 0, st>>>(b->cells, b->cellsN, nn, b->coords, b->nv, nc, g, cnt, stats);
        PGD_IX(hipGetLastError());
        PGD_IX(hipMemcpyAsync(&total, stats, sizeof total, hipMemcpyDeviceToHost, st));
        PGD_IX(hipStreamSynchronize(st));
        if (total <= (unsigned long long)(LOC_INDEX_CAP * nc) && total <= 2147483647ull) break;
        if (bins == 1) return cleanup(fail(c, PGD_ERR_LIMIT, "points index: %llu registrations in one bin", total));      // (nc < 2^31: not reached)
        for (int a = 0; a < 3; ++a) {
            g.n[a] = g.n[a] > 1 ? g.n[a] / 2 : 1;
            g.inv[a] = L[a] > 0.0 ? (double)g.n[a] / L[a] : 0.0;
        }
    }
    const size_t ptr_bytes = (size_t)(bins + 1) * sizeof(int), list_bytes = (size_t)(total > 0 ? total : 1) * sizeof(int);
    PGD_IX_TRY(dev_alloc(c, &q, ptr_bytes)); bin_ptr = (int *)q;
    PGD_IX_TRY(dev_alloc(c, &q, list_bytes)); bin_cells = (int *)q;
    PGD_IX_TRY(scan_exclusive_i32(c, cnt, bin_ptr, bins));
    k_index_longest<<<grid_for(bins), TPB, 0, st>>>(cnt, bins, (int *)(stats + 1));
    PGD_IX(hipMemsetAsync(cnt, 0, (size_t)(bins + 1) * sizeof(int), st));
    PGD_IX(hipMemsetAsync(bin_cells, 0, list_bytes, st));
    k_index_fill<G><<<grid, TPB, 0, st>>>(b->cells, b->cellsN, nn, b->coords, b->nv, nc, g, bin_ptr, cnt, bin_cells);
    PGD_IX(hipGetLastError());
    int longest = 0;
    PGD_IX(hipMemcpyAsync(&longest, stats + 1, sizeof longest, hipMemcpyDeviceToHost, st));
    PGD_IX(hipStreamSynchronize(st));
#undef PGD_IX
#undef PGD_IX_TRY
    for (int a = 0; a < 3; ++a) { ix.o[a] = g.o[a]; ix.inv[a] = g.inv[a]; ix.n[a] = g.n[a]; }
    ix.bin_ptr = bin_ptr; ix.bin_cells = bin_cells;
    ix.bins = bins; ix.entries = (int64_t)total; ix.longest = longest;
    ix.bytes = ptr_bytes + list_bytes;
    ix.target = knob;
    ix.built = true;
    ++ix.builds;
    return cleanup(PGD_OK);
}

// the index of b under the current target: the one it holds, or a new one
static int index_ensure(Ctx *c, const Mesh *b) {
    Mesh::LocIndex &ix = b->loc_index;
    if (ix.built && ix.target == c->locate_index_target) return PGD_OK;
    if (ix.built) {
        (void)hipStreamSynchronize(c->stream);
        ix.release();
    }
    return b->gdim == 2 ? index_build<2>(c, b) : index_build<3>(c, b);
}

template <int G>
static int locate_index(Ctx *c, const Mesh *b, const double *pts_dev, int64_t npts, double tol, Points *P) {
    const Mesh::LocIndex &ix = b->loc_index;
    LocGrid g;
    for (int a = 0; a < 3; ++a) { g.o[a] = ix.o[a]; g.inv[a] = ix.inv[a]; g.n[a] = ix.n[a]; }
    k_locate_index<G><<<(int)((npts + TPB - 1) / TPB), TPB, 0, c->stream>>>(b->cells, b->cellsN, b->cellsN ? b->nvpc : 0, b->coords, b->nv, g, ix.bin_ptr,
                                                                           ix.bin_cells, pts_dev, npts, tol, P->cells, P->lam);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, PGD_ERR_HIP, "points_locate: launch failed: %s", hipGetErrorString(e));
    return PGD_OK;
}

// the host's copy of the cells decides what pgd_points_sample may do with the set
static int points_scan(Ctx *c, Points *P) {
    P->first_outside = -1;
    if (P->npts == 0) return PGD_OK;
    std::vector<int> host((size_t)P->npts);
    PGD_HIP(c, hipMemcpyAsync(host.data(), P->cells, host.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    for (int64_t p = 0; p < P->npts; ++p)
        if (host[(size_t)p] < 0) { P->first_outside = p; break; }
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_points_locate(pgd_handle h, pgd_handle mh, const double *pts, int64_t npts, double tol, pgd_handle *out) {
    PGD_CTX(c, h);
    const Mesh *b = points_base(c, "points_locate", mh, nullptr);
    if (!b) return PGD_ERR_INVALID;
    if (!out) return fail(c, PGD_ERR_INVALID, "points_locate: null output");
    if (npts < 0 || (npts > 0 && !pts)) return fail(c, PGD_ERR_INVALID, "points_locate: %lld points, pts %s", (long long)npts, pts ? "given" : "missing");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(c, PGD_ERR_INVALID, "points_locate: tol = %g, a finite tolerance >= 0 is needed", tol);
    if (npts >= ((int64_t)1 << 31) / 4) return fail(c, PGD_ERR_LIMIT, "points_locate: %lld points exceed the int32 index range", (long long)npts);
    const int G = b->gdim;
    std::unique_ptr<Points> P;
    PGD_TRY(points_new(c, G, npts, b->nc, P));
    c->locate_last_path = 0;
    if (npts > 0) {
        void *q;
        const size_t bytes = (size_t)npts * G * sizeof(double);
        PGD_TRY(dev_alloc(c, &q, bytes));
        double *pts_dev = (double *)q;
        hipError_t e = hipMemcpyAsync(pts_dev, pts, bytes, hipMemcpyHostToDevice, c->stream);
        int rc = e == hipSuccess ? PGD_OK : fail(c, PGD_ERR_HIP, "points_locate: upload failed: %s", hipGetErrorString(e));
        if (rc == PGD_OK) {
            const bool lattice = c->locate_lattice && b->lattice_regular && b->cells && G == 3 && b->nvpc == 4 && tol <= LOC_LATTICE_TOL;
            if (lattice) {
                const int nx = b->sym_nx, ny = b->sym_ny, nz = (int)(b->nv / ((int64_t)nx * ny));
                k_locate_lattice<<<(int)((npts + TPB - 1) / TPB), TPB, 0, c->stream>>>(b->cells, b->coords, b->nv, nx, ny, nz, b->lat_h[0], b->lat_h[1],
                                                                                       b->lat_h[2], pts_dev, npts, tol, P->cells, P->lam);
                e = hipGetLastError();
                if (e != hipSuccess) rc = fail(c, PGD_ERR_HIP, "points_locate: launch failed: %s", hipGetErrorString(e));
                c->locate_last_path = 2;
            } else if (c->locate_index && (G == 2 || G == 3) && tol <= LOC_INDEX_TOL) {
                rc = index_ensure(c, b);
                if (rc == PGD_OK) rc = G == 2 ? locate_index<2>(c, b, pts_dev, npts, tol, P.get()) : locate_index<3>(c, b, pts_dev, npts, tol, P.get());
                c->locate_last_path = 3;
            } else {
                rc = G == 1 ? locate_general<1>(c, b, pts_dev, npts, tol, P.get()) : G == 2 ? locate_general<2>(c, b, pts_dev, npts, tol, P.get())
                                                                                            : locate_general<3>(c, b, pts_dev, npts, tol, P.get());
                c->locate_last_path = 1;
            }
        }
        if (rc == PGD_OK) rc = points_scan(c, P.get());      // (synchronises: pts_dev is no longer read)
        else (void)hipStreamSynchronize(c->stream);
        dev_release(c, pts_dev, bytes);
        if (rc != PGD_OK) return rc;
    }
    *out = put_obj(c, P.release());
    return PGD_OK;
}

int pgd_points_from(pgd_handle h, pgd_handle mh, const int32_t *cells, const double *lam, int64_t npts, pgd_handle *out) {
    PGD_CTX(c, h);
    const Mesh *b = points_base(c, "points_from", mh, nullptr);
    if (!b) return PGD_ERR_INVALID;
    if (!out) return fail(c, PGD_ERR_INVALID, "points_from: null output");
    if (npts < 0 || (npts > 0 && (!cells || !lam))) return fail(c, PGD_ERR_INVALID, "points_from: %lld points need cells and lam", (long long)npts);
    if (npts >= ((int64_t)1 << 31) / 4) return fail(c, PGD_ERR_LIMIT, "points_from: %lld points exceed the int32 index range", (long long)npts);
    int64_t first = -1;
    for (int64_t p = 0; p < npts; ++p) {
        if (cells[p] < -1 || cells[p] >= b->nc)
            return fail(c, PGD_ERR_INVALID, "points_from: point %lld names cell %d, the mesh has %lld", (long long)p, cells[p], (long long)b->nc);
        if (cells[p] < 0 && first < 0) first = p;
    }
    std::unique_ptr<Points> P;
    PGD_TRY(points_new(c, b->gdim, npts, b->nc, P));
    P->first_outside = first;
    if (npts > 0) {
        PGD_HIP(c, hipMemcpyAsync(P->cells, cells, (size_t)npts * sizeof(int), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(P->lam, lam, (size_t)npts * (b->gdim + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipStreamSynchronize(c->stream));      // (the host arrays are the caller's again)
    }
    *out = put_obj(c, P.release());
    return PGD_OK;
}

int pgd_points_download(pgd_handle h, pgd_handle ph, int32_t *cells_out, double *lam_out) {
    PGD_CTX(c, h);
    Points *P = get_points(c, ph);
    if (!P) return fail(c, PGD_ERR_INVALID, "points_download: invalid point set handle");
    if (P->npts == 0) return PGD_OK;
    if (cells_out) PGD_HIP(c, hipMemcpyAsync(cells_out, P->cells, (size_t)P->npts * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (lam_out) PGD_HIP(c, hipMemcpyAsync(lam_out, P->lam, (size_t)P->npts * (P->gdim + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    return PGD_OK;
}

int pgd_points_info(pgd_handle h, pgd_handle ph, int64_t *npts, int *gdim, int64_t *first_outside) {
    PGD_CTX(c, h);
    Points *P = get_points(c, ph);
    if (!P) return fail(c, PGD_ERR_INVALID, "points_info: invalid point set handle");
    PGD_PUT(npts, P->npts); PGD_PUT(gdim, P->gdim); PGD_PUT(first_outside, P->first_outside);
    return PGD_OK;
}

int pgd_points_last_path(pgd_handle h, int *path) {
    PGD_CTX(c, h);
    if (!path) return fail(c, PGD_ERR_INVALID, "points_last_path: null output");
    *path = c->locate_last_path;
    return PGD_OK;
}

int pgd_points_index_info(pgd_handle h, pgd_handle mh, int64_t *out) {
    PGD_CTX(c, h);
    const Mesh *b = points_base(c, "points_index_info", mh, nullptr);
    if (!b) return PGD_ERR_INVALID;
    if (!out) return fail(c, PGD_ERR_INVALID, "points_index_info: null output");
    const Mesh::LocIndex &ix = b->loc_index;
    out[0] = ix.built ? 1 : 0;
    out[1] = ix.builds;
    for (int a = 0; a < 3; ++a) out[2 + a] = ix.built ? ix.n[a] : 0;
    out[5] = ix.entries;
    out[6] = ix.longest;
    out[7] = (int64_t)ix.bytes;
    return PGD_OK;
}

int pgd_points_index_download(pgd_handle h, pgd_handle mh, int32_t *bin_ptr, int32_t *bin_cells, double *geom) {
    PGD_CTX(c, h);
    const Mesh *b = points_base(c, "points_index_download", mh, nullptr);
    if (!b) return PGD_ERR_INVALID;
    const Mesh::LocIndex &ix = b->loc_index;
    if (!ix.built) return fail(c, PGD_ERR_INVALID, "points_index_download: the mesh holds no index");
    if (bin_ptr) PGD_HIP(c, hipMemcpyAsync(bin_ptr, ix.bin_ptr, (size_t)(ix.bins + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (bin_cells && ix.entries > 0)
        PGD_HIP(c, hipMemcpyAsync(bin_cells, ix.bin_cells, (size_t)ix.entries * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    if (geom)
        for (int a = 0; a < 3; ++a) { geom[a] = ix.o[a]; geom[3 + a] = ix.inv[a]; geom[6 + a] = (double)ix.n[a]; }
    return PGD_OK;
}

int pgd_points_index_drop(pgd_handle h, pgd_handle mh) {
    PGD_CTX(c, h);
    const Mesh *b = points_base(c, "points_index_drop", mh, nullptr);
    if (!b) return PGD_ERR_INVALID;
    if (b->loc_index.built) {
        (void)hipStreamSynchronize(c->stream);      // (the arrays go straight back to HIP)
        b->loc_index.release();
    }
    b->loc_index.builds = 0;
    return PGD_OK;
}

int pgd_points_sample(pgd_handle h, pgd_handle ph, pgd_handle mh, pgd_handle uh, int what, pgd_handle oh) {
    PGD_CTX(c, h);
    Points *P = get_points(c, ph);
    if (!P) return fail(c, PGD_ERR_INVALID, "points_sample: invalid point set handle");
    const Mesh *m = nullptr;
    const Mesh *b = points_base(c, "points_sample", mh, &m);
    if (!b) return PGD_ERR_INVALID;
    const int G = b->gdim, NC = m->ncomp;
    if (b->nc != P->nc || G != P->gdim)
        return fail(c, PGD_ERR_INVALID, "points_sample: the point set was made on a mesh of %lld cells in %d-D, the layout has %lld in %d-D",
                    (long long)P->nc, P->gdim, (long long)b->nc, G);
    const int deg = b->nvpc == G + 1 ? 1 : b->nvpc == loc_nodes(G, 2) ? 2 : 0;
    if (!deg || (deg == 2 && G > 1 && !b->cellsN) || ((deg == 1 || G == 1) && !b->cells))
        return fail(c, PGD_ERR_INVALID, "points_sample: a layout of %d nodes per cell in %d-D is neither P1 nor P2", b->nvpc, G);
    if (what != 0 && what != 1) return fail(c, PGD_ERR_INVALID, "points_sample: what = %d (0: values, 1: gradients)", what);
    Vec *u = get_vec(c, uh), *out = get_vec(c, oh);
    if (!u || u->n != b->nv * NC)
        return fail(c, PGD_ERR_INVALID, "points_sample: u is a vector of %lld entries (nodes x components)", (long long)(b->nv * NC));
    const int64_t need = P->npts * NC * (what ? G : 1);
    if (!out || out->n != need)
        return fail(c, PGD_ERR_INVALID, "points_sample: out is a vector of points x components%s = %lld entries", what ? " x gdim" : "", (long long)need);
    if (out == u) return fail(c, PGD_ERR_INVALID, "points_sample: out aliases u");
    if (P->first_outside >= 0)
        return fail(c, PGD_ERR_INVALID, "points_sample: point %lld of the set lies outside the mesh (cell -1)", (long long)P->first_outside);
    if (P->npts == 0) return PGD_OK;
    const int grid = (int)((P->npts + TPB - 1) / TPB);
#define PGD_SAMPLE(GG, DD) k_points_sample<GG, DD><<<grid, TPB, 0, c->stream>>>(b->cells, b->cellsN, b->coords, b->nv, P->cells, P->lam, P->npts, NC, u->d, what, out->d)
    switch (G * 10 + deg) {
        case 11: PGD_SAMPLE(1, 1); break;
        case 12: PGD_SAMPLE(1, 2); break;
        case 21: PGD_SAMPLE(2, 1); break;
        case 22: PGD_SAMPLE(2, 2); break;
        case 31: PGD_SAMPLE(3, 1); break;
        default: PGD_SAMPLE(3, 2); break;
    }
#undef PGD_SAMPLE
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

int pgd_points_free(pgd_handle h, pgd_handle ph) {
    PGD_CTX(c, h);
    return free_obj(c, ph, POINTS);
}

}  // extern "C"
