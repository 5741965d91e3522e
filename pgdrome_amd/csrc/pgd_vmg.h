// The hierarchy of the variable-coefficient V-cycle (pgd_vmg.hip) as the files that build level 0 themselves see it: pgd_vmg.hip
// (Ctx::vmg on the operator's slot arrays, Ctx::cmg on the diagonal blocks of a blocked P1 operator) and pgd_pmg.hip (Ctx::pmg on
// the Galerkin blocks P^T A P of a P2 operator).  The kernels of the cycle stay in pgd_vmg.hip.
#pragma once
#include "pgd_internal.h"

namespace pgd {

struct VGrid { int nx, ny, nz; };

struct VLevel {
    VGrid g{0, 0, 0};
    int64_t n = 0, stride = 0;
    double *a = nullptr;                                // 8 slot arrays (level 0: the operator's, not owned)
    int unit = 0;                                       // slot 0 is exactly 1 and is not loaded
    double *w = nullptr;                                // l1-Jacobi weights, 0 on eliminated nodes
    uint8_t *el = nullptr;                              // 1 = eliminated
    double *b = nullptr, *x = nullptr, *t = nullptr;    // right-hand side, result, work (level 0: b is the caller's r)
};

struct Vmg {
    int nx = 0, ny = 0, nz = 0;
    std::vector<VLevel> lv;
    int np0 = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool own0 = false;                                  // level 0 owns its slot arrays and a right-hand side (a component hierarchy of Cmg / Pmg)
};

constexpr int VMG_BOTTOM_MAX = 4096, VMG_SWEEPS = 24;

// pattern vector t: 0..7 = +(dx, dy, dz) with the bits of t, 8..14 = -(bits of t - 7)
__device__ __host__ constexpr int vp_x(int t) { return t < 8 ? (t & 1) : -((t - 7) & 1); }
__device__ __host__ constexpr int vp_y(int t) { return t < 8 ? ((t >> 1) & 1) : -(((t - 7) >> 1) & 1); }
__device__ __host__ constexpr int vp_z(int t) { return t < 8 ? ((t >> 2) & 1) : -(((t - 7) >> 2) & 1); }
// is (cx, cy, cz) a pattern vector?  (all components in {0, 1} or all in {0, -1})
__device__ __host__ constexpr bool vp_in(int cx, int cy, int cz) {
    return (cx >= 0 && cy >= 0 && cz >= 0 && cx <= 1 && cy <= 1 && cz <= 1) || (cx <= 0 && cy <= 0 && cz <= 0 && cx >= -1 && cy >= -1 && cz >= -1);
}

void vmg_free(Vmg *&M);
dim3 vmg_grid(const VGrid &g);                                            // one node per thread, 64 x 4 nodes of a plane per workgroup
bool vmg_lattice_ok(int64_t nv, int nx, int ny, int nz);                   // the lattices the cycle takes
bool vmg_levels_alloc(Vmg *&M, int nx, int ny, int nz, bool own0);         // false: no hierarchy (at most 4096 nodes) or no memory - M is released
bool vmg_form(Ctx *c, Vmg *M, bool timed);                                 // the hierarchy of the operator level 0 holds NOW
int vmg_levels(const Vmg *M);

}  // namespace pgd
