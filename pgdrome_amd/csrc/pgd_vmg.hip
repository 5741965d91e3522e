// Geometric multigrid preconditioner for pgd_pcg_solve on VARIABLE-COEFFICIENT operators (PGD_TUNE_PCG_PRECOND = 2; the frontend's
// settings["preconditioner"] = "vmg").  The cycle of pgd_mg.hip holds ONE stencil in registers and needs the hull eliminated; this
// one works on the diagonal form with per-row coefficients - weighted atoms, several materials, Robin terms, any Dirichlet set.
//
// What it rests on: P1 on the 6-tets-per-cube lattice is nested under doubling of the spacing, the interpolation P has weight 1 at
// the node and 1/2 at the 14 neighbours along the mesh edges, and for ANY 15-point operator A the Galerkin operator P^T A P is
// again a 15-point operator: (P^T A P)_IJ sums a_ij over i = 2I + e, j = 2J + f with e, f and j - i in the pattern
// E = {+-(dx, dy, dz), d in {0,1}^3}, so 2 (J - I) = (j - i) + e - f, and a J - I with components of both signs would need four
// contributions of the right sign from three pattern vectors that can each give one.  That argument only uses the sparsity of P
// and A, so it also holds where rows of P are dropped (eliminated nodes) or cut off (a far face with an even node count).
//
//   * Level 0 is the scaled operator of the solve, D^-1/2 A D^-1/2, in the operator's own slot arrays (not copied).
//   * An ELIMINATED node is a row without couplings (the Dirichlet rows of pgd_op_combine: identity rows, columns zeroed).  Every
//     level carries a byte per node; coarse node k is fine node 2k and is eliminated iff that node is.  Every vector of the cycle
//     is zero on eliminated nodes.  A far face with an even node count has no coarse counterpart: the last coarse node keeps its
//     own state and what lies beyond it reads as zero (the rule of pgd_mg.hip).
//   * k_vmg_galerkin forms the 8 slot arrays of P^T A P from the level above, one coarse row per thread, gathering the 15 fine
//     rows around node 2k through their 15-point rows: no atomics, no CSR.  Once per solve (the operator changes with every
//     fixed-point pass).
//   * Smoother: l1-Jacobi, w_i = 1 / sum_j |a_ij| from the level's own rows (k_vmg_rowsum).  D_l1 >= A for every symmetric A, so
//     the step converges without an eigenvalue estimate, without a reduction over the level and without a tuned factor - the
//     bound lambda_max(D^-1 A) = 2 of the constant stencils does not hold here.  It is a diagonal matrix: the cycle stays
//     symmetric positive definite.
//   * V(1,1), the pre-smoothing step from a zero start folded into the residual (u = W b: t = b - A u) and into the prolongation
//     (v = u + P e), then x = v + W (b - A v); the coarsest level - the first with at most 4096 nodes - is 24 sweeps
//     inside one workgroup.  A lattice of at most 4096 nodes has no hierarchy: Jacobi-PCG.
// Levels with at least mg_march_min nodes along x and y run their two passes in k_vmg_march: the z-march of the diagonal form
// (dia_march2 of pgd_dia_march.h, the one body it shares with k_spmv_dia_march2: planes of the input staged in an LDS ring, the
// plane-below couplings handed on through LDS) with the two epilogues of the cycle; smaller levels in the plain kernels.
#include "pgd_vmg.h"
#include "pgd_dia_march.h"

#include <cmath>
#include <cstring>
#include <type_traits>

namespace pgd {

// (VGrid, VLevel, Vmg and the pattern vectors: pgd_vmg.h, shared with pgd_pmg.hip)

// pcg_precond = 3: one hierarchy per displacement component of a blocked P1 operator (the diagonal blocks of its scaled form)
struct Cmg {
    int ncomp = 0;
    Vmg *comp[3] = {nullptr, nullptr, nullptr};
    double *s = nullptr;                                // d^-1/2 of the block operator, one per dof
    int *bad = nullptr;                                 // device flag: a diagonal block holds an entry off the 15-point pattern
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
};

// does fine node 2K + c lie in the support of one of the coarse basis functions K + D, D in {0,1}^3?
__device__ __host__ constexpr bool vmg_reaches(int cx, int cy, int cz) {
    for (int D = 0; D < 8; ++D)
        if (vp_in(cx - 2 * (D & 1), cy - 2 * ((D >> 1) & 1), cz - 2 * (D >> 2))) return true;
    return false;
}
template <int T, int N, class F>
__device__ __forceinline__ void vmg_static_for(F &&f) {
    if constexpr (T < N) { f(std::integral_constant<int, T>{}); vmg_static_for<T + 1, N>(f); }
}

// a(i, i + g) of a level in diagonal form; both nodes inside the lattice
__device__ __forceinline__ double vmg_entry(const double *__restrict__ a, int64_t stride, int unit, int64_t i, int t, int nx, int64_t P) {
    if (t == 0) return unit ? 1.0 : a[i];
    if (t < 8) return a[(int64_t)t * stride + i];
    const int s = t - 7;
    const int64_t off = (s & 1) + (int64_t)nx * ((s >> 1) & 1) + P * (s >> 2);
    return a[(int64_t)s * stride + i - off];
}

// The 8 slot arrays of P^T A P and the coarse level's eliminated bytes: one coarse node per thread.
__global__ __launch_bounds__(256) void k_vmg_galerkin(VGrid gf, const double *__restrict__ af, int64_t sf, int unit, const uint8_t *__restrict__ elf,
                                                      VGrid gc, double *__restrict__ ac, int64_t sc, uint8_t *__restrict__ elc) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), Z = blockIdx.z;
    if (X >= gc.nx || Y >= gc.ny) return;
    const int64_t Pc = (int64_t)gc.nx * gc.ny, I = Pc * Z + (int64_t)gc.nx * Y + X;
    const int64_t Pf = (int64_t)gf.nx * gf.ny, i0 = Pf * (2 * Z) + (int64_t)gf.nx * (2 * Y) + 2 * X;
    const bool el = elf[i0] != 0;
    elc[I] = el ? 1 : 0;
    double acc[8];
#pragma unroll
    for (int D = 0; D < 8; ++D) acc[D] = 0.0;
    if (el) acc[0] = 1.0;
    else {
        // which coarse neighbours K + D carry a coupling: inside the coarse lattice and free
        bool cok[8];
#pragma unroll
        for (int D = 0; D < 8; ++D) {
            const int dx = D & 1, dy = (D >> 1) & 1, dz = D >> 2;
            cok[D] = X + dx < gc.nx && Y + dy < gc.ny && Z + dz < gc.nz;
            if (cok[D] && D) cok[D] = elf[i0 + 2 * (dx + (int64_t)gf.nx * dy + Pf * dz)] == 0;
        }
        const int fx = 2 * X, fy = 2 * Y, fz = 2 * Z;
        vmg_static_for<0, 15>([&](auto ec) {
            constexpr int e = decltype(ec)::value, ex = vp_x(e), ey = vp_y(e), ez = vp_z(e);
            const int ix = fx + ex, iy = fy + ey, iz = fz + ez;
            const bool iok = ix >= 0 && iy >= 0 && iz >= 0 && ix < gf.nx && iy < gf.ny && iz < gf.nz;
            const int64_t i = i0 + ex + (int64_t)gf.nx * ey + Pf * ez;
            if (iok && !elf[i]) {                                           // (an eliminated node's row of P is dropped)
                constexpr double pe = e ? 0.5 : 1.0;
                vmg_static_for<0, 15>([&](auto gc2) {
                    constexpr int g = decltype(gc2)::value, cx = ex + vp_x(g), cy = ey + vp_y(g), cz = ez + vp_z(g);      // j = 2K + c
                    if constexpr (vmg_reaches(cx, cy, cz)) {
                        const int jx = fx + cx, jy = fy + cy, jz = fz + cz;
                        if (jx >= 0 && jy >= 0 && jz >= 0 && jx < gf.nx && jy < gf.ny && jz < gf.nz) {
                            const double aij = pe * vmg_entry(af, sf, unit, i, g, gf.nx, Pf);
                            vmg_static_for<0, 8>([&](auto dc) {
                                constexpr int D = decltype(dc)::value, hx = cx - 2 * (D & 1), hy = cy - 2 * ((D >> 1) & 1), hz = cz - 2 * (D >> 2);
                                if constexpr (vp_in(hx, hy, hz)) {
                                    constexpr double pf = (hx || hy || hz) ? 0.5 : 1.0;
                                    if (cok[D]) acc[D] = fma(pf, aij, acc[D]);
                                }
                            });
                        }
                    }
                });
            }
        });
    }
#pragma unroll
    for (int D = 0; D < 8; ++D) ac[(int64_t)D * sc + I] = acc[D];
}

// w_i = 1 / sum_j |a_ij|, 0 on eliminated nodes.  FIND: level 0 - a row without couplings IS an eliminated node (el is written);
// else el is given.
template <bool FIND>
__global__ __launch_bounds__(256) void k_vmg_rowsum(VGrid g, const double *__restrict__ a, int64_t stride, int unit, uint8_t *__restrict__ el,
                                                    double *__restrict__ w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (x >= g.nx || y >= g.ny) return;
    const int64_t P = (int64_t)g.nx * g.ny, i = P * z + (int64_t)g.nx * y + x;
    double off = 0.0;
#pragma unroll
    for (int t = 1; t < 15; ++t) {
        const int jx = x + vp_x(t), jy = y + vp_y(t), jz = z + vp_z(t);
        if (jx < 0 || jy < 0 || jz < 0 || jx >= g.nx || jy >= g.ny || jz >= g.nz) continue;
        off += fabs(vmg_entry(a, stride, unit, i, t, g.nx, P));
    }
    bool e;
    if (FIND) { e = off == 0.0; el[i] = e ? 1 : 0; }
    else e = el[i] != 0;
    w[i] = e ? 0.0 : 1.0 / (fabs(unit ? 1.0 : a[i]) + off);
}

// (A v)_i in row order, every neighbour checked against the lattice
__device__ __forceinline__ double vmg_apply(const VGrid &g, const double *__restrict__ a, int64_t stride, int unit, const double *__restrict__ v,
                                            int x, int y, int z, int64_t i, int64_t P) {
    double acc = 0.0;
#pragma unroll
    for (int s = 7; s >= 1; --s) {
        const int dx = s & 1, dy = (s >> 1) & 1, dz = s >> 2;
        const int64_t off = dx + (int64_t)g.nx * dy + P * dz;
        if (x >= dx && y >= dy && z >= dz) acc = fma(a[(int64_t)s * stride + i - off], v[i - off], acc);
    }
    acc = fma(unit ? 1.0 : a[i], v[i], acc);
#pragma unroll
    for (int s = 1; s < 8; ++s) {
        const int dx = s & 1, dy = (s >> 1) & 1, dz = s >> 2;
        const int64_t off = dx + (int64_t)g.nx * dy + P * dz;
        if (x + dx < g.nx && y + dy < g.ny && z + dz < g.nz) acc = fma(a[(int64_t)s * stride + i], v[i + off], acc);
    }
    return acc;
}

// u = w in  (the folded pre-smoothing step; small levels only - the march forms it while staging)
__global__ __launch_bounds__(TPB) void k_vmg_wmul(const double *__restrict__ w, const double *__restrict__ in, double *__restrict__ u, int64_t n,
                                                  const int *__restrict__ flags) {
    if (flags && flags[0]) return;
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) u[i] = w[i] * in[i];
}

// MODE 0: out = b - A in          (in = W b: the residual behind the pre-smoothing step from a zero start)
// MODE 1: out = in + w (b - A in) (post-smoothing step);  DOT: partial sums of b . out per workgroup
template <int MODE, bool DOT>
__global__ __launch_bounds__(256) void k_vmg_pass(VGrid g, const double *__restrict__ a, int64_t stride, int unit, const double *__restrict__ w,
                                                  const double *__restrict__ in, const double *__restrict__ b, double *__restrict__ out,
                                                  double *__restrict__ partials, const int *__restrict__ flags) {
    __shared__ double s_red[4];
    if (flags && flags[0]) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    double d = 0.0;
    if (x < g.nx && y < g.ny) {
        const int64_t P = (int64_t)g.nx * g.ny, i = P * z + (int64_t)g.nx * y + x;
        const double wi = w[i];
        double o = 0.0;
        if (wi != 0.0) {
            const double av = vmg_apply(g, a, stride, unit, in, x, y, z, i, P), bi = b[i];
            if (MODE == 0) o = bi - av;
            else { o = fma(wi, bi - av, in[i]); if (DOT) d = bi * o; }
        }
        out[i] = o;
    }
    if (DOT) {
        d = block_sum(d, s_red);
        if (threadIdx.x == 0) partials[(int64_t)blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z)] = d;
    }
}

// bc = P^T t: the node's own value + half of its 14 neighbours along the mesh edges (those inside the fine lattice)
__global__ __launch_bounds__(256) void k_vmg_restrict(VGrid gc, VGrid gf, const uint8_t *__restrict__ elc, const double *__restrict__ t,
                                                      double *__restrict__ bc, const int *__restrict__ flags) {
    if (flags && flags[0]) return;
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), Z = blockIdx.z;
    if (X >= gc.nx || Y >= gc.ny) return;
    const int64_t Pc = (int64_t)gc.nx * gc.ny, I = Pc * Z + (int64_t)gc.nx * Y + X;
    double o = 0.0;
    if (!elc[I]) {
        const int64_t Pf = (int64_t)gf.nx * gf.ny, i = Pf * (2 * Z) + (int64_t)gf.nx * (2 * Y) + 2 * X;
        double h = 0.0;
#pragma unroll
        for (int e = 1; e < 15; ++e) {
            const int ix = 2 * X + vp_x(e), iy = 2 * Y + vp_y(e), iz = 2 * Z + vp_z(e);
            if (ix < 0 || iy < 0 || iz < 0 || ix >= gf.nx || iy >= gf.ny || iz >= gf.nz) continue;
            h += t[i + vp_x(e) + (int64_t)gf.nx * vp_y(e) + Pf * vp_z(e)];
        }
        o = fma(0.5, h, t[i]);
    }
    bc[I] = o;
}

// v = w b + P e on the fine lattice: a fine node is a coarse node (all coordinates even) or the midpoint of ONE coarse edge
__global__ __launch_bounds__(256) void k_vmg_prolong(VGrid gf, VGrid gc, const double *__restrict__ w, const double *__restrict__ b,
                                                     const double *__restrict__ e, double *__restrict__ v, const int *__restrict__ flags) {
    if (flags && flags[0]) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (x >= gf.nx || y >= gf.ny) return;
    const int64_t Pf = (int64_t)gf.nx * gf.ny, i = Pf * z + (int64_t)gf.nx * y + x;
    const double wi = w[i];
    double o = 0.0;
    if (wi != 0.0) {
        const int64_t Pc = (int64_t)gc.nx * gc.ny;
        const int bx = (x + 1) >> 1, by = (y + 1) >> 1, bz = (z + 1) >> 1;
        const double ea = e[Pc * (z >> 1) + (int64_t)gc.nx * (y >> 1) + (x >> 1)];
        const double eb = (bx < gc.nx && by < gc.ny && bz < gc.nz) ? e[Pc * bz + (int64_t)gc.nx * by + bx] : 0.0;      // (ea == eb on a coarse node)
        o = fma(wi, b[i], 0.5 * (ea + eb));
    }
    v[i] = o;
}

// the coarsest level inside one workgroup: `sweeps` l1-Jacobi steps from a zero start (the iterate in LDS, the rows'
// coefficients - 256 KB at most - from the caches)
__global__ __launch_bounds__(1024) void k_vmg_bottom(VGrid g, const double *__restrict__ a, int64_t stride, const double *__restrict__ w,
                                                     const double *__restrict__ b, double *__restrict__ x, int sweeps, const int *__restrict__ flags) {
    __shared__ double s_v[2][VMG_BOTTOM_MAX];
    if (flags && flags[0]) return;
    const int P = g.nx * g.ny, n = P * g.nz;
    for (int i = threadIdx.x; i < n; i += 1024) s_v[0][i] = w[i] * b[i];          // (w = 0 on eliminated nodes)
    __syncthreads();
    int cur = 0;
    for (int sw = 1; sw < sweeps; ++sw) {
#pragma unroll 1
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int z = i / P, rem = i - z * P, y = rem / g.nx, xx = rem - y * g.nx;
            const double wi = w[i];
            double o = 0.0;
            if (wi != 0.0) o = fma(wi, b[i] - vmg_apply(g, a, stride, 0, s_v[cur], xx, y, z, i, P), s_v[cur][i]);
            s_v[cur ^ 1][i] = o;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int i = threadIdx.x; i < n; i += 1024) x[i] = s_v[cur][i];
}

// x = s b on the eliminated rows: their exact solution in the scaled unknowns (s = 1 on a Dirichlet row), so that the residual, and
// with it every vector of the cycle, vanishes there
__global__ __launch_bounds__(TPB) void k_vmg_fix_start(const uint8_t *__restrict__ el, const double *__restrict__ sc, const double *__restrict__ b,
                                                       double *__restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n && el[i]) x[i] = sc[i] * b[i];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Component-wise cycle for blocked (vector-valued) P1 operators (PGD_TUNE_PCG_PRECOND = 3): the block diagonal of an elasticity
// operator - its ncomp diagonal blocks A_cc - is spectrally equivalent to it (Korn), and every A_cc is a scalar operator on the
// 15-point pattern of the base lattice.  B_c = (S A S)[c::ncomp, c::ncomp], S = diag(A)^-1/2, gets a hierarchy of its own
// (eliminated sets may differ between components), z[c::ncomp] = s_c M_c (s_c r[c::ncomp]).
struct CmgPtrs { double *p[3]; };
struct CmgConst { const double *p[3]; };
struct CmgElim { const uint8_t *p[3]; };

// The 8 upper slot arrays of every B_c from the CSR values of the block operator (rows ncomp i + c, node-major): one lattice node
// per thread, one pass over its ncomp rows.  Slot 0 is 1, a coupling the row does not store is an exact 0; s = dinv^1/2 is kept
// for the split and the merge.  A stored non-zero of a diagonal block that is off the pattern raises *bad.
__global__ __launch_bounds__(256) void k_cmg_extract(VGrid g, int ncomp, const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                     const double *__restrict__ vals, const double *__restrict__ dinv, CmgPtrs a,
                                                     double *__restrict__ s, int *__restrict__ bad) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (x >= g.nx || y >= g.ny) return;
    const int64_t P = (int64_t)g.nx * g.ny, n = P * g.nz, i = P * z + (int64_t)g.nx * y + x;
    for (int c = 0; c < ncomp; ++c) {
        const int64_t row = (int64_t)ncomp * i + c;
        const double si = sqrt(dinv[row]);
        double acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = 0.0;
        for (int k = row_ptr[row]; k < row_ptr[row + 1]; ++k) {
            const int col = cols[k];
            const int j = col / ncomp;
            if (col - j * ncomp != c) continue;                               // another block
            const int jz = (int)(j / P), rem = (int)(j - jz * P), jy = rem / g.nx, jx = rem - jy * g.nx;
            const int dx = jx - x, dy = jy - y, dz = jz - z;
            const double v = vals[k];
            if (dx >= 0 && dy >= 0 && dz >= 0 && dx <= 1 && dy <= 1 && dz <= 1) {
                const int t = dx + 2 * dy + 4 * dz;
                const double e = (si * v) * sqrt(dinv[col]);
#pragma unroll
                for (int u = 1; u < 8; ++u) if (u == t) acc[u] = e;
            } else if (!(dx <= 0 && dy <= 0 && dz <= 0 && dx >= -1 && dy >= -1 && dz >= -1) && v != 0.0) *bad = 1;
        }
        double *ac = a.p[c];
        ac[i] = 1.0;
#pragma unroll
        for (int t = 1; t < 8; ++t) ac[(int64_t)t * n + i] = acc[t];
        s[row] = si;
    }
}

// b_c = s_c r[c::ncomp]: the level-0 right-hand sides of the component cycles
__global__ __launch_bounds__(TPB) void k_cmg_split(int ncomp, const double *__restrict__ r, const double *__restrict__ s, CmgPtrs b, int64_t n,
                                                   const int *__restrict__ flags) {
    if (flags && flags[0]) return;
    for (int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x; d < n; d += (int64_t)gridDim.x * TPB) {
        const int64_t i = d / ncomp;
        b.p[d - i * ncomp][i] = s[d] * r[d];
    }
}

// z[c::ncomp] = s_c x_c, partial sums of r . z per workgroup (fixed order)
__global__ __launch_bounds__(TPB) void k_cmg_merge(int ncomp, CmgConst xc, const double *__restrict__ s, const double *__restrict__ r,
                                                   double *__restrict__ z, int64_t n, double *__restrict__ partials, const int *__restrict__ flags) {
    __shared__ double s_red[4];
    if (flags && flags[0]) return;
    double acc = 0.0;
    for (int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x; d < n; d += (int64_t)gridDim.x * TPB) {
        const int64_t i = d / ncomp;
        const double zd = s[d] * xc.p[d - i * ncomp][i];
        z[d] = zd;
        acc = fma(r[d], zd, acc);
    }
    acc = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// x = b on the dofs a component hierarchy has eliminated (identity rows): their exact solution; the cycle never moves them
__global__ __launch_bounds__(TPB) void k_cmg_fix_start(int ncomp, CmgElim el, const double *__restrict__ b, double *__restrict__ x, int64_t n) {
    const int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (d >= n) return;
    const int64_t i = d / ncomp;
    if (el.p[d - i * ncomp][i]) x[d] = b[d];
}

// ------------------------------------------------------------------------------------------------------------------------------
// The two level passes of the cycle in the z-march of the diagonal form (dia_march2, pgd_dia_march.h: the body of the product
// k_spmv_dia_march2 - a 64 x 8 patch per 256-thread workgroup, two rows per thread, three planes of the input in an LDS ring, the
// plane-below couplings handed on through LDS) with its epilogues 1 and 2:
//   EPI 1: staged u = w in;  out = in - A u on free rows, 0 on eliminated ones                   (in = the level's right-hand side)
//   EPI 2: staged v = in;    out = v + w (b - A v);  DOT: partial sums of b . out per workgroup  (in = the prolongated vector)
template <int EPI, bool DOT>
__global__ __launch_bounds__(256) void k_vmg_march(DiaArgs A) { dia_march2<DOT, true, EPI>(A); }

void vmg_free(Vmg *&M) {
    if (!M) return;
    for (size_t l = 0; l < M->lv.size(); ++l) {
        VLevel &L = M->lv[l];
        if ((l > 0 || M->own0) && L.a) (void)hipFree(L.a);
        for (void *p : {(void *)L.w, (void *)L.el, (void *)L.b, (void *)L.x, (void *)L.t}) if (p) (void)hipFree(p);
    }
    if (M->ev0) (void)hipEventDestroy(M->ev0);
    if (M->ev1) (void)hipEventDestroy(M->ev1);
    delete M;
    M = nullptr;
}

static void cmg_free(Cmg *&G) {
    if (!G) return;
    for (Vmg *&M : G->comp) vmg_free(M);
    if (G->s) (void)hipFree(G->s);
    if (G->bad) (void)hipFree(G->bad);
    if (G->ev0) (void)hipEventDestroy(G->ev0);
    if (G->ev1) (void)hipEventDestroy(G->ev1);
    delete G;
    G = nullptr;
}

void vmg_release(Ctx *c) { vmg_free(c->vmg); cmg_free(c->cmg); pmg_release(c); }

double *vmg_result(Vmg *M) { return M && !M->lv.empty() ? M->lv[0].x : nullptr; }

dim3 vmg_grid(const VGrid &g) { return dim3((unsigned)((g.nx + 63) / 64), (unsigned)((g.ny + 3) / 4), (unsigned)g.nz); }

static bool vmg_marches(const Ctx *c, const VLevel &L, int *zchunk, int *wgs) {
    if (!(c->mg_march_min > 0 && L.g.nx >= c->mg_march_min && L.g.ny >= c->mg_march_min && L.g.nz >= 8)) return false;
    const int64_t tiles = (int64_t)((L.g.nx + 63) / 64) * ((L.g.ny + 7) / 8);
    // planes per march: about two workgroups per CU in the launch, between 3 (a shorter march pays its prologue too often) and 8
    const int zc = (int)std::max<int64_t>(3, std::min<int64_t>(8, tiles * L.g.nz / (2 * (int64_t)std::max(1, c->num_cu))));
    const int64_t g = (int64_t)((L.g.nz + zc - 1) / zc) * tiles;
    if (g >= ((int64_t)1 << 30)) return false;
    *zchunk = zc; *wgs = (int)g;
    return true;
}

// the lattices the cycle takes: at least 8 nodes along every axis, within the grid limits of its launches
bool vmg_lattice_ok(int64_t nv, int nx, int ny, int nz) {
    return (int64_t)nx * ny * nz == nv && std::min(nx, std::min(ny, nz)) >= 8 && nz <= 65535 && ny <= 4 * 65535;
}

// levels and buffers of M for this lattice (kept where M already has them); own0: level 0 gets slot arrays and a right-hand side of
// its own.  false: no hierarchy (at most 4096 nodes) or no memory - M is released
bool vmg_levels_alloc(Vmg *&M, int nx, int ny, int nz, bool own0) {
    if (M && M->nx == nx && M->ny == ny && M->nz == nz && M->own0 == own0) return true;
    vmg_free(M);                                                            // another lattice: new levels and buffers
    M = new Vmg();
    M->own0 = own0;
    VGrid g{nx, ny, nz};
    for (;;) {
        VLevel L;
        L.g = g;
        L.n = (int64_t)g.nx * g.ny * g.nz;
        M->lv.push_back(L);
        if (L.n <= VMG_BOTTOM_MAX) break;                                   // the first level one workgroup can hold is the coarsest
        g = VGrid{(g.nx + 1) / 2, (g.ny + 1) / 2, (g.nz + 1) / 2};
    }
    if (M->lv.size() < 2) { vmg_free(M); return false; }                   // (at most 4096 nodes: no hierarchy, Jacobi)
    bool ok = hipEventCreate(&M->ev0) == hipSuccess && hipEventCreate(&M->ev1) == hipSuccess;
    for (size_t l = 0; ok && l < M->lv.size(); ++l) {
        VLevel &L = M->lv[l];
        const bool last = l + 1 == M->lv.size();
        const size_t bytes = (size_t)L.n * sizeof(double) + PAD_BYTES;
        auto get = [&](void **p, size_t nbytes) { ok = ok && hipMalloc(p, nbytes) == hipSuccess; };
        if (l > 0 || own0) { get((void **)&L.a, 8 * (size_t)L.n * sizeof(double) + PAD_BYTES); L.stride = L.n; get((void **)&L.b, bytes); }
        get((void **)&L.w, bytes);
        get((void **)&L.el, (size_t)L.n + PAD_BYTES);
        get((void **)&L.x, bytes);
        if (!last) get((void **)&L.t, bytes);
    }
    if (!ok) { (void)hipGetLastError(); vmg_free(M); return false; }
    M->nx = nx; M->ny = ny; M->nz = nz;
    return true;
}

// the hierarchy of the operator level 0 holds NOW: eliminated nodes and weights of level 0, then level by level P^T A P and its weights
bool vmg_form(Ctx *c, Vmg *M, bool timed) {
    VLevel &L0 = M->lv[0];
    M->timed = timed && hipEventRecord(M->ev0, c->stream) == hipSuccess;
    k_vmg_rowsum<true><<<vmg_grid(L0.g), 256, 0, c->stream>>>(L0.g, L0.a, L0.stride, L0.unit, L0.el, L0.w);
    for (size_t l = 1; l < M->lv.size(); ++l) {
        VLevel &F = M->lv[l - 1], &C = M->lv[l];
        k_vmg_galerkin<<<vmg_grid(C.g), 256, 0, c->stream>>>(F.g, F.a, F.stride, F.unit, F.el, C.g, C.a, C.stride, C.el);
        k_vmg_rowsum<false><<<vmg_grid(C.g), 256, 0, c->stream>>>(C.g, C.a, C.stride, 0, C.el, C.w);
    }
    M->timed = M->timed && hipEventRecord(M->ev1, c->stream) == hipSuccess;
    if (hipGetLastError() != hipSuccess) return false;
    int zc = 0, wgs = 0;
    const dim3 g0 = vmg_grid(L0.g);
    M->np0 = vmg_marches(c, L0, &zc, &wgs) ? wgs : (int)((int64_t)g0.x * g0.y * g0.z);
    if (ensure_partials(c, std::max<int64_t>(M->np0 + 64, 4 * (int64_t)MAX_VEC_BLOCKS)) != PGD_OK) return false;
    return true;
}

// true: the cycle applies to this solve - hierarchy formed from the operator's CURRENT (scaled) slot values, buffers there
bool vmg_prepare(Ctx *c, Vmg *&M, const Mesh *m, const Csr *a) {
    if (!m || !a || m->sym_nx <= 0 || !a->uvals || !a->uvals_valid || !a->uvals_scaled) return false;
    const int nx = m->sym_nx, ny = m->sym_ny, nz = (int)(m->nv / ((int64_t)nx * ny));
    if (!vmg_lattice_ok(m->nv, nx, ny, nz)) return false;
    if (!vmg_levels_alloc(M, nx, ny, nz, false)) return false;
    VLevel &L0 = M->lv[0];
    L0.a = a->uvals; L0.stride = a->uvals_stride; L0.unit = a->uvals_unit ? 1 : 0;
    return vmg_form(c, M, true);
}

// after the solve's last synchronisation: the hierarchy's setup time joins the context's sum (pgd_vmg_counts)
void vmg_note_setup(Ctx *c) {
    Vmg *M = c->vmg;
    if (!M || !M->timed) return;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, M->ev0, M->ev1) == hipSuccess) c->cycle[PGD_PCG_PRECOND_VMG].setup_ms += (double)ms;
    else (void)hipGetLastError();
    M->timed = false;
}

int vmg_fix_start(Ctx *c, Vmg *M, const double *sc, const double *b, double *x, int64_t n) {
    if (!M || M->lv.empty() || M->lv[0].n != n) return fail(c, PGD_ERR_INVALID, "vmg_fix_start: no hierarchy");
    k_vmg_fix_start<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, c->stream>>>(M->lv[0].el, sc, b, x, n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

int vmg_levels(const Vmg *M) { return M ? (int)M->lv.size() : 0; }

// z = M r: the cycle from level 0 down and back up; the result lands in z_out (default: vmg_result(c)), the partial sums of
// r . z in c->partials (*nparts of them); the level passes issued to k_vmg_march are counted in *marches
int vmg_vcycle(Ctx *c, Vmg *M, const double *r, bool dot, int *nparts, double *z_out, int64_t *marches) {
    if (!M || M->lv.size() < 2) return fail(c, PGD_ERR_INVALID, "vmg_vcycle: no hierarchy");
    const int nl = (int)M->lv.size();
    const dim3 blk(256, 1, 1);
    const int *flags = c->flags;
    int np_dot = M->np0;
    // The march orders its LDS traffic only (lds_barrier) and does not wait for its stores of `out`: no launch below passes an `out`
    // that aliases in, b, w or the slot arrays.  Down: in = r / L.b, out = L.t.  Up: in = L.t, b = r / L.b, out = L.x or z_out, the
    // caller's own vector (pgd_pcg_solve: its p, never r; cmg_apply: r is a component's level-0 L.b, z_out is null, out = L.x).
    // L.a, L.w, L.b, L.x, L.t are separate allocations of the level.
    auto march = [&](const VLevel &L, int epi, const double *in, const double *b, double *out, bool d) -> bool {
        int zc = 0, wgs = 0;
        if (!vmg_marches(c, L, &zc, &wgs)) return false;
        DiaArgs A{};
        A.uvals = L.a; A.ew = L.w; A.x = in; A.eb = b; A.y = out; A.partials = c->partials; A.flags = flags; A.n = L.stride;
        A.nx = L.g.nx; A.ny = L.g.ny; A.nz = L.g.nz; A.z0 = 0; A.z1 = L.g.nz; A.zchunk = zc;
        A.tiles_x = (L.g.nx + 63) / 64; A.tiles_y = (L.g.ny + 7) / 8; A.unit_diag = L.unit;
        if (epi == 1) k_vmg_march<1, false><<<wgs, 256, 0, c->stream>>>(A);
        else if (d) k_vmg_march<2, true><<<wgs, 256, 0, c->stream>>>(A);
        else k_vmg_march<2, false><<<wgs, 256, 0, c->stream>>>(A);
        *marches += 1;
        return true;
    };
    // down: residual behind the folded pre-smoothing step, restriction
    for (int l = 0; l + 1 < nl; ++l) {
        VLevel &L = M->lv[l], &C = M->lv[l + 1];
        const double *b = l == 0 ? r : L.b;
        if (!march(L, 1, b, nullptr, L.t, false)) {
            k_vmg_wmul<<<(unsigned)((L.n + TPB - 1) / TPB), TPB, 0, c->stream>>>(L.w, b, L.x, L.n, flags);
            k_vmg_pass<0, false><<<vmg_grid(L.g), blk, 0, c->stream>>>(L.g, L.a, L.stride, L.unit, L.w, L.x, b, L.t, nullptr, flags);
        }
        k_vmg_restrict<<<vmg_grid(C.g), blk, 0, c->stream>>>(C.g, L.g, C.el, L.t, C.b, flags);
    }
    {
        VLevel &B = M->lv[nl - 1];
        k_vmg_bottom<<<1, 1024, 0, c->stream>>>(B.g, B.a, B.stride, B.w, B.b, B.x, VMG_SWEEPS, flags);
    }
    // up: v = w b + P e, one more l1-Jacobi step
    for (int l = nl - 2; l >= 0; --l) {
        VLevel &L = M->lv[l], &C = M->lv[l + 1];
        const double *b = l == 0 ? r : L.b;
        k_vmg_prolong<<<vmg_grid(L.g), blk, 0, c->stream>>>(L.g, C.g, L.w, b, C.x, L.t, flags);
        double *out = l == 0 && z_out ? z_out : L.x;
        const bool d = l == 0 && dot;
        if (!march(L, 2, L.t, b, out, d)) {
            if (d) k_vmg_pass<1, true><<<vmg_grid(L.g), blk, 0, c->stream>>>(L.g, L.a, L.stride, L.unit, L.w, L.t, b, out, c->partials, flags);
            else k_vmg_pass<1, false><<<vmg_grid(L.g), blk, 0, c->stream>>>(L.g, L.a, L.stride, L.unit, L.w, L.t, b, out, nullptr, flags);
        }
    }
    if (nparts) *nparts = np_dot;
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

// true: the component-wise cycle applies to this solve - a blocked P1 layout over a 3-D box lattice with a hierarchy, the diagonal
// blocks of D^-1/2 A D^-1/2 extracted from the CSR values (a->vals, a->dinv are current) and their hierarchies formed
bool cmg_prepare(Ctx *c, const Mesh *m, const Mesh *base, const Csr *a) {
    if (!m || !base || !a || m->ncomp < 2 || m->ncomp > 3 || base->ncomp != 1 || base->gdim != 3 || base->cellsN || base->sym_nx <= 0 ||
        !a->vals || !a->dinv || !a->dinv_valid || m->nv != base->nv * m->ncomp) return false;
    const int nx = base->sym_nx, ny = base->sym_ny, nz = (int)(base->nv / ((int64_t)nx * ny)), nc = m->ncomp;
    if (!vmg_lattice_ok(base->nv, nx, ny, nz) || base->nv <= VMG_BOTTOM_MAX) return false;
    Cmg *G = c->cmg;
    if (!G || G->ncomp != nc || !G->comp[0] || G->comp[0]->nx != nx || G->comp[0]->ny != ny || G->comp[0]->nz != nz) {
        cmg_free(c->cmg);
        G = c->cmg = new Cmg();
        G->ncomp = nc;
        bool ok = hipEventCreate(&G->ev0) == hipSuccess && hipEventCreate(&G->ev1) == hipSuccess;
        ok = ok && hipMalloc((void **)&G->s, (size_t)m->nv * sizeof(double) + PAD_BYTES) == hipSuccess;
        ok = ok && hipMalloc((void **)&G->bad, PAD_BYTES) == hipSuccess;
        for (int k = 0; ok && k < nc; ++k) ok = vmg_levels_alloc(G->comp[k], nx, ny, nz, true);
        if (!ok) { (void)hipGetLastError(); cmg_free(c->cmg); return false; }
    }
    const VGrid g{nx, ny, nz};
    CmgPtrs ap{{nullptr, nullptr, nullptr}};
    for (int k = 0; k < nc; ++k) { VLevel &L0 = G->comp[k]->lv[0]; L0.unit = 1; ap.p[k] = L0.a; }
    G->timed = hipEventRecord(G->ev0, c->stream) == hipSuccess;
    if (hipMemsetAsync(G->bad, 0, sizeof(int), c->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    k_cmg_extract<<<vmg_grid(g), 256, 0, c->stream>>>(g, nc, m->row_ptr, m->cols, a->vals, a->dinv, ap, G->s, G->bad);
    if (hipGetLastError() != hipSuccess) return false;
    for (int k = 0; k < nc; ++k)
        if (!vmg_form(c, G->comp[k], false)) return false;
    G->timed = G->timed && hipEventRecord(G->ev1, c->stream) == hipSuccess;
    int bad = 0;
    if (hipMemcpyAsync(&bad, G->bad, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return bad == 0;
}

void cmg_note_setup(Ctx *c) {
    Cmg *G = c->cmg;
    if (!G || !G->timed) return;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, G->ev0, G->ev1) == hipSuccess) c->cycle[PGD_PCG_PRECOND_CMG].setup_ms += (double)ms;
    else (void)hipGetLastError();
    G->timed = false;
}

int cmg_fix_start(Ctx *c, const double *b, double *x, int64_t n) {
    Cmg *G = c->cmg;
    if (!G || !G->comp[0] || G->comp[0]->lv[0].n * G->ncomp != n) return fail(c, PGD_ERR_INVALID, "cmg_fix_start: no hierarchy");
    CmgElim el{{nullptr, nullptr, nullptr}};
    for (int k = 0; k < G->ncomp; ++k) el.p[k] = G->comp[k]->lv[0].el;
    k_cmg_fix_start<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, c->stream>>>(G->ncomp, el, b, x, n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

// z = M r: split, one cycle per component (one after the other on the stream), merge; the partial sums of r . z in c->partials
int cmg_apply(Ctx *c, const double *r, double *z, int64_t n, int *nparts) {
    Cmg *G = c->cmg;
    if (!G || !G->comp[0] || G->comp[0]->lv[0].n * G->ncomp != n) return fail(c, PGD_ERR_INVALID, "cmg_apply: no hierarchy");
    CmgPtrs bp{{nullptr, nullptr, nullptr}};
    CmgConst xp{{nullptr, nullptr, nullptr}};
    for (int k = 0; k < G->ncomp; ++k) { bp.p[k] = G->comp[k]->lv[0].b; xp.p[k] = G->comp[k]->lv[0].x; }
    const int g = grid_for(n);
    k_cmg_split<<<g, TPB, 0, c->stream>>>(G->ncomp, r, G->s, bp, n, c->flags);
    PGD_LAUNCH_CHECK(c);
    for (int k = 0; k < G->ncomp; ++k) PGD_TRY(vmg_vcycle(c, G->comp[k], bp.p[k], false, nullptr, nullptr, &c->cycle[PGD_PCG_PRECOND_CMG].marches));
    k_cmg_merge<<<g, TPB, 0, c->stream>>>(G->ncomp, xp, G->s, r, z, n, c->partials, c->flags);
    PGD_LAUNCH_CHECK(c);
    if (nparts) *nparts = g;
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_vmg_counts(pgd_handle h, int64_t *solves, int64_t *fallbacks, int64_t *levels) {
    PGD_CTX(c, h);
    PGD_PUT(levels, vmg_levels(c->vmg));
    return cycle_read(c->cycle[PGD_PCG_PRECOND_VMG], solves, fallbacks, nullptr, nullptr);
}

int pgd_vmg_times(pgd_handle h, double *setup_ms, int64_t *march_passes) {
    PGD_CTX(c, h);
    return cycle_read(c->cycle[PGD_PCG_PRECOND_VMG], nullptr, nullptr, setup_ms, march_passes);
}

int pgd_cmg_counts(pgd_handle h, int64_t *solves, int64_t *fallbacks, int64_t *levels) {
    PGD_CTX(c, h);
    PGD_PUT(levels, c->cmg ? vmg_levels(c->cmg->comp[0]) : 0);
    return cycle_read(c->cycle[PGD_PCG_PRECOND_CMG], solves, fallbacks, nullptr, nullptr);
}

int pgd_cmg_times(pgd_handle h, double *setup_ms, int64_t *march_passes) {
    PGD_CTX(c, h);
    return cycle_read(c->cycle[PGD_PCG_PRECOND_CMG], nullptr, nullptr, setup_ms, march_passes);
}

}  // extern "C"
