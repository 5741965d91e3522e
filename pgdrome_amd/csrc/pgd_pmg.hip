// p-multigrid preconditioner for pgd_pcg_solve on P2 operators over a 3-D box lattice (PGD_TUNE_PCG_PRECOND = 4; the frontend's
// settings["preconditioner"] = "pmg"), scalar or blocked with 2 or 3 components.
//
// What it rests on: P1 is nested in P2 on the same mesh.  With the frontend's node numbering - the vertices first, in lattice order,
// then one node per mesh edge - the interpolation P from P1 has weight 1 from a vertex to its own node and 1/2 from each end vertex
// to an edge node, so P^T A P is the P1 operator of the same form: on the 6-tets-per-cube box a 15-point operator on the vertex
// lattice, which is what the V-cycle of pgd_vmg.hip takes as its level 0 (a hierarchy with own0, as Ctx::cmg holds them).
//
//   * pgd_mesh_p2_bind (once per layout, host): every edge joins two vertices that differ by one of the 14 pattern vectors of the
//     lattice and no (vertex, pattern vector) slot is taken twice; then two parent ints per node and a vertex -> edge-node table
//     of 14 arrays go to the device.  A layout that fails a check is remembered as refused and its solves fall back.
//   * An ELIMINATED dof is a CSR row without a non-zero off-diagonal entry (the identity rows of pgd_op_combine): k_pmg_scan.
//   * B_c = P^T A[c::ncomp, c::ncomp] P per component, rows of eliminated P2 dofs and columns of eliminated vertex dofs of P dropped,
//     the identity on eliminated vertices: k_pmg_galerkin, one vertex per thread, the 8 upper slots of the diagonal form, no atomics.
//     A is unscaled: level 0 has unit = 0.  A term off the pattern raises a device flag and the solve falls back.
//   * z = D^-1 r + P (M_c (P^T r)_c)_c, M_c one V(1,1) cycle on B_c, z = 0 on eliminated dofs: k_pmg_restrict, vmg_vcycle per
//     component, k_pmg_prolong (with the fixed-order partial sums of r . z).  Additive: no product beyond the iteration's own.
// The iteration is the unscaled textbook recurrence (PGD_PCG_FORM_PRECOND), x = b on the eliminated dofs from the start.
#include "pgd_vmg.h"

#include <vector>

namespace pgd {

struct Pmg {
    int ncomp = 0;
    int64_t n = 0, nvert = 0;                           // dofs, vertices of the lattice
    Vmg *comp[3] = {nullptr, nullptr, nullptr};
    uint8_t *el = nullptr;                              // one byte per dof: 1 = eliminated
    int *bad = nullptr;                                 // device flag: a term of a Galerkin block fell off the 15-point pattern
    const int *par = nullptr, *v2e = nullptr;           // the bound layout's tables (Mesh::p2_par, Mesh::p2_v2e) of the current solve
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
};

struct PmgPtrs { double *p[3]; };
struct PmgConst { const double *p[3]; };

// el[d] = 1 where row d stores no non-zero off-diagonal entry: one lane per dof
__global__ __launch_bounds__(TPB) void k_pmg_scan(const int *__restrict__ row_ptr, const int *__restrict__ cols, const double *__restrict__ vals,
                                                  uint8_t *__restrict__ el, int64_t n) {
    const int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (d >= n) return;
    bool coupled = false;
    for (int k = row_ptr[d]; k < row_ptr[d + 1] && !coupled; ++k) coupled = cols[k] != (int)d && vals[k] != 0.0;
    el[d] = coupled ? 0 : 1;
}

// The 8 upper slot arrays of every B_c: one lattice vertex I per thread.  Per component it walks the CSR rows of the dofs with a
// non-zero in column I of P - the vertex's own dof (weight 1) and the dofs of the at most 14 edge nodes around it (weight 1/2) -
// skips eliminated rows and the columns of eliminated dofs (A need not be symmetric for that), takes the entries of the row's own component (in a blocked row every NC-th entry, verified), and sends
// each through the one or two parents J of its column node.  J - I is told from the index difference and the position of I (the
// lattice has at least 8 nodes per axis: the 15 differences are distinct); J >= I on the pattern is accumulated, J < I on the
// pattern belongs to the thread of J, anything else raises *bad.  The weights 1, 1/2 and 1/4 are exact and the walk is sequential:
// only the additions round, in a fixed order.  (The loop over the 15 rows stays rolled - its body is a row walk; the slot
// selection is unrolled so that the sums stay in registers.)
template <int NC>
__global__ __launch_bounds__(256) void k_pmg_galerkin(VGrid g, int64_t nvert, const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                      const double *__restrict__ vals, const uint8_t *__restrict__ el,
                                                      const int *__restrict__ par, int64_t nnode, const int *__restrict__ v2e, PmgPtrs a,
                                                      int *__restrict__ bad) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), Z = blockIdx.z;
    if (X >= g.nx || Y >= g.ny) return;
    const int P = g.nx * g.ny, I = P * Z + g.nx * Y + X;
    int off[8];
    bool up[8], dn[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int dx = t & 1, dy = (t >> 1) & 1, dz = t >> 2;
        off[t] = dx + g.nx * dy + P * dz;
        up[t] = X + dx < g.nx && Y + dy < g.ny && Z + dz < g.nz;
        dn[t] = X >= dx && Y >= dy && Z >= dz;
    }
    bool off_pattern = false;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = 0.0;
        if (el[(int64_t)NC * I + c]) acc[0] = 1.0;
        else {
#pragma unroll 1
            for (int s = 0; s < 15; ++s) {
                const int node = s == 0 ? I : v2e[(int64_t)(s - 1) * nvert + I];
                if (node < 0) continue;
                const int64_t i = (int64_t)NC * node + c;
                if (el[i]) continue;                                            // (an eliminated dof's row of P is dropped)
                const double pe = s == 0 ? 1.0 : 0.5;
                const int k1 = row_ptr[i + 1];
                for (int k = row_ptr[i] + c; k < k1; k += NC) {
                    const int col = cols[k], jn = col / NC;
                    if (col - jn * NC != c) { off_pattern = true; continue; }   // (not the blocked pattern of pgd_mesh_blocked)
                    const double v = vals[k];
                    if (v == 0.0 || el[col]) continue;                          // (an eliminated dof's row of P is dropped: its column of A does not enter)
                    const int q0 = par[jn], q1 = par[nnode + jn];
                    const double w = q0 == q1 ? pe * v : 0.5 * (pe * v);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int J = h ? q1 : q0;
                        if (h && q1 == q0) continue;
                        if (el[(int64_t)NC * J + c]) continue;                  // (an eliminated vertex's column of P is dropped)
                        const int diff = J - I;
                        bool hit = false;
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            if (diff == off[t] && up[t]) { acc[t] += w; hit = true; }
                            if (t > 0 && diff == -off[t] && dn[t]) hit = true;
                        }
                        if (!hit) off_pattern = true;
                    }
                }
            }
        }
        double *ac = a.p[c];
#pragma unroll
        for (int t = 0; t < 8; ++t) ac[(int64_t)t * nvert + I] = acc[t];
    }
    if (off_pattern) *bad = 1;
}

// b_c[I] = r[(I, c)] + 1/2 sum of r[(e, c)] over the free edge dofs e around vertex I (the table's order), 0 on eliminated vertices:
// the level-0 right-hand sides of the component cycles
template <int NC>
__global__ __launch_bounds__(256) void k_pmg_restrict(VGrid g, int64_t nvert, const double *__restrict__ r, const uint8_t *__restrict__ el,
                                                      const int *__restrict__ v2e, PmgPtrs b, const int *__restrict__ flags) {
    if (flags && flags[0]) return;
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), Z = blockIdx.z;
    if (X >= g.nx || Y >= g.ny) return;
    const int64_t I = (int64_t)g.nx * g.ny * Z + (int64_t)g.nx * Y + X;
    int en[14];
#pragma unroll
    for (int t = 0; t < 14; ++t) en[t] = v2e[(int64_t)t * nvert + I];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double o = 0.0;
        if (!el[NC * I + c]) {
            double h = 0.0;
#pragma unroll
            for (int t = 0; t < 14; ++t) {
                const int64_t d = (int64_t)NC * en[t] + c;
                if (en[t] >= 0 && !el[d]) h += r[d];                            // (an eliminated dof's row of P is dropped)
            }
            o = fma(0.5, h, r[NC * I + c]);
        }
        b.p[c][I] = o;
    }
}

// z[d] = dinv[d] r[d] + the cycle's value at the vertex, or half the sum at the two end vertices of the edge; 0 on eliminated dofs.
// Partial sums of r . z per workgroup (shuffle, LDS, fixed order).
template <int NC>
__global__ __launch_bounds__(TPB) void k_pmg_prolong(int64_t n, int64_t nnode, const int *__restrict__ par, const uint8_t *__restrict__ el,
                                                     const double *__restrict__ dinv, const double *__restrict__ r, PmgConst x,
                                                     double *__restrict__ z, double *__restrict__ partials, const int *__restrict__ flags) {
    __shared__ double s_red[4];
    if (flags && flags[0]) return;
    double acc = 0.0;
    for (int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x; d < n; d += (int64_t)gridDim.x * TPB) {
        const int64_t node = d / NC;
        const int c = (int)(d - node * NC);
        double zd = 0.0;
        const double rd = r[d];
        if (!el[d]) {
            const double *__restrict__ xc = (NC == 1 || c == 0) ? x.p[0] : (NC == 2 || c == 1) ? x.p[1] : x.p[2];
            const int q0 = par[node], q1 = par[nnode + node];
            const double e = q0 == q1 ? xc[q0] : 0.5 * (xc[q0] + xc[q1]);
            zd = fma(dinv[d], rd, e);
        }
        z[d] = zd;
        acc = fma(rd, zd, acc);
    }
    acc = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// x = b on the eliminated dofs (identity rows): their exact solution; no vector of the iteration moves them
__global__ __launch_bounds__(TPB) void k_pmg_fix_start(const uint8_t *__restrict__ el, const double *__restrict__ b, double *__restrict__ x, int64_t n) {
    const int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (d < n && el[d]) x[d] = b[d];
}

static void pmg_free(Pmg *&G) {
    if (!G) return;
    for (Vmg *&M : G->comp) vmg_free(M);
    if (G->el) (void)hipFree(G->el);
    if (G->bad) (void)hipFree(G->bad);
    if (G->ev0) (void)hipEventDestroy(G->ev0);
    if (G->ev1) (void)hipEventDestroy(G->ev1);
    delete G;
    G = nullptr;
}

void pmg_release(Ctx *c) { pmg_free(c->pmg); }

// the scalar P2 layout that carries the binding of m: m itself, or the base of a blocked layout
static const Mesh *pmg_bound_base(Ctx *c, const Mesh *m) {
    const Mesh *base = m && m->ncomp > 1 ? get_mesh(c, m->base) : m;
    return base && base->ncomp == 1 && base->p2_bound == 1 && base->p2_par && base->p2_v2e ? base : nullptr;
}

// true: the cycle applies to this solve - a P2 layout (scalar, or blocked with 2 or 3 components) bound to a box lattice with a
// hierarchy, no Galerkin term off the pattern, buffers there
bool pmg_prepare(Ctx *c, const Mesh *m, const Csr *a) {
    const Mesh *base = pmg_bound_base(c, m);
    if (!base || !a || !a->vals || !a->dinv || !a->dinv_valid || m->ncomp < 1 || m->ncomp > 3 || m->nv != base->nv * m->ncomp) return false;
    const int nx = base->p2_nx, ny = base->p2_ny, nz = base->p2_nz, nc = m->ncomp;
    const int64_t nvert = base->p2_nvert;
    if (!vmg_lattice_ok(nvert, nx, ny, nz) || nvert <= VMG_BOTTOM_MAX) return false;
    Pmg *G = c->pmg;
    if (!G || G->ncomp != nc || G->n != m->nv || !G->comp[0] || G->comp[0]->nx != nx || G->comp[0]->ny != ny || G->comp[0]->nz != nz) {
        pmg_free(c->pmg);
        G = c->pmg = new Pmg();
        G->ncomp = nc; G->n = m->nv; G->nvert = nvert;
        bool ok = hipEventCreate(&G->ev0) == hipSuccess && hipEventCreate(&G->ev1) == hipSuccess;
        ok = ok && hipMalloc((void **)&G->el, (size_t)m->nv + PAD_BYTES) == hipSuccess;
        ok = ok && hipMalloc((void **)&G->bad, PAD_BYTES) == hipSuccess;
        for (int k = 0; ok && k < nc; ++k) ok = vmg_levels_alloc(G->comp[k], nx, ny, nz, true);
        if (!ok) { (void)hipGetLastError(); pmg_free(c->pmg); return false; }
    }
    G->par = base->p2_par; G->v2e = base->p2_v2e;
    const VGrid g{nx, ny, nz};
    PmgPtrs ap{{nullptr, nullptr, nullptr}};
    for (int k = 0; k < nc; ++k) { VLevel &L0 = G->comp[k]->lv[0]; L0.unit = 0; ap.p[k] = L0.a; }
    G->timed = hipEventRecord(G->ev0, c->stream) == hipSuccess;
    if (hipMemsetAsync(G->bad, 0, sizeof(int), c->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
    k_pmg_scan<<<(unsigned)((m->nv + TPB - 1) / TPB), TPB, 0, c->stream>>>(m->row_ptr, m->cols, a->vals, G->el, m->nv);
    if (nc == 1) k_pmg_galerkin<1><<<vmg_grid(g), 256, 0, c->stream>>>(g, nvert, m->row_ptr, m->cols, a->vals, G->el, G->par, base->nv, G->v2e, ap, G->bad);
    else if (nc == 2) k_pmg_galerkin<2><<<vmg_grid(g), 256, 0, c->stream>>>(g, nvert, m->row_ptr, m->cols, a->vals, G->el, G->par, base->nv, G->v2e, ap, G->bad);
    else k_pmg_galerkin<3><<<vmg_grid(g), 256, 0, c->stream>>>(g, nvert, m->row_ptr, m->cols, a->vals, G->el, G->par, base->nv, G->v2e, ap, G->bad);
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

void pmg_note_setup(Ctx *c) {
    Pmg *G = c->pmg;
    if (!G || !G->timed) return;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, G->ev0, G->ev1) == hipSuccess) c->cycle[PGD_PCG_PRECOND_PMG].setup_ms += (double)ms;
    else (void)hipGetLastError();
    G->timed = false;
}

int pmg_fix_start(Ctx *c, const double *b, double *x, int64_t n) {
    Pmg *G = c->pmg;
    if (!G || !G->comp[0] || G->n != n) return fail(c, PGD_ERR_INVALID, "pmg_fix_start: no hierarchy");
    k_pmg_fix_start<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, c->stream>>>(G->el, b, x, n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

// z = M r: restriction, one cycle per component (one after the other on the stream), prolongation + D^-1 r; launches only
int pmg_apply(Ctx *c, const Csr *a, const double *r, double *z, int64_t n, int *nparts) {
    Pmg *G = c->pmg;
    if (!G || !G->comp[0] || G->n != n || !a || !a->dinv) return fail(c, PGD_ERR_INVALID, "pmg_apply: no hierarchy");
    PmgPtrs bp{{nullptr, nullptr, nullptr}};
    PmgConst xp{{nullptr, nullptr, nullptr}};
    for (int k = 0; k < G->ncomp; ++k) { bp.p[k] = G->comp[k]->lv[0].b; xp.p[k] = G->comp[k]->lv[0].x; }
    const VGrid g = G->comp[0]->lv[0].g;
    const int64_t nnode = n / G->ncomp;
    const int gp = grid_for(n);
    const int *flags = c->flags;
    if (G->ncomp == 1) k_pmg_restrict<1><<<vmg_grid(g), 256, 0, c->stream>>>(g, G->nvert, r, G->el, G->v2e, bp, flags);
    else if (G->ncomp == 2) k_pmg_restrict<2><<<vmg_grid(g), 256, 0, c->stream>>>(g, G->nvert, r, G->el, G->v2e, bp, flags);
    else k_pmg_restrict<3><<<vmg_grid(g), 256, 0, c->stream>>>(g, G->nvert, r, G->el, G->v2e, bp, flags);
    PGD_LAUNCH_CHECK(c);
    for (int k = 0; k < G->ncomp; ++k) PGD_TRY(vmg_vcycle(c, G->comp[k], bp.p[k], false, nullptr, nullptr, &c->cycle[PGD_PCG_PRECOND_PMG].marches));
    if (G->ncomp == 1) k_pmg_prolong<1><<<gp, TPB, 0, c->stream>>>(n, nnode, G->par, G->el, a->dinv, r, xp, z, c->partials, flags);
    else if (G->ncomp == 2) k_pmg_prolong<2><<<gp, TPB, 0, c->stream>>>(n, nnode, G->par, G->el, a->dinv, r, xp, z, c->partials, flags);
    else k_pmg_prolong<3><<<gp, TPB, 0, c->stream>>>(n, nnode, G->par, G->el, a->dinv, r, xp, z, c->partials, flags);
    PGD_LAUNCH_CHECK(c);
    if (nparts) *nparts = gp;
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_mesh_p2_bind(pgd_handle h, pgd_handle p2h, pgd_handle p1h, const int32_t *edge_vertices, int64_t n_edges, int *bound) {
    PGD_CTX(c, h);
    Mesh *p2 = get_mesh(c, p2h);
    const Mesh *p1 = get_mesh(c, p1h);
    if (!p2 || !p1 || !bound || n_edges < 0 || (n_edges > 0 && !edge_vertices)) return fail(c, PGD_ERR_INVALID, "mesh_p2_bind: invalid arguments");
    *bound = 0;
    // a new decision replaces the last one
    if (p2->p2_par) { (void)hipFree(p2->p2_par); p2->p2_par = nullptr; }
    if (p2->p2_v2e) { (void)hipFree(p2->p2_v2e); p2->p2_v2e = nullptr; }
    p2->p2_bound = -1;
    p2->p2_lat = 0;
    if (p2->ncomp != 1 || p2->gdim != 3 || !p2->cellsN || p2->nvpc != 10) return PGD_OK;
    if (p1->ncomp != 1 || p1->gdim != 3 || p1->cellsN || p1->sym_nx <= 0 || p1->sym_ny <= 0) return PGD_OK;
    const int nx = p1->sym_nx, ny = p1->sym_ny;
    const int64_t nvert = p1->nv, plane = (int64_t)nx * ny, nnode = p2->nv;
    if (nvert <= 0 || nvert % plane || nnode != nvert + n_edges || nnode >= (int64_t)1 << 31) return PGD_OK;
    const int nz = (int)(nvert / plane);
    std::vector<int> par((size_t)(2 * nnode)), v2e((size_t)(14 * nvert), -1);
    for (int64_t i = 0; i < nvert; ++i) par[(size_t)i] = par[(size_t)(nnode + i)] = (int)i;
    // (for the row-class form of pgd_p2lat.hip: is the edge list strictly ascending in (va, vb) with va < vb?)
    bool ascending = true;
    for (int64_t e = 0; e < n_edges; ++e) {
        const int64_t va = edge_vertices[2 * e], vb = edge_vertices[2 * e + 1];
        ascending = ascending && va < vb && (e == 0 || edge_vertices[2 * e - 2] < va || (edge_vertices[2 * e - 2] == va && edge_vertices[2 * e - 1] < vb));
        if (va < 0 || vb < 0 || va >= nvert || vb >= nvert || va == vb) return PGD_OK;
        const int az = (int)(va / plane), ay = (int)((va - az * plane) / nx), ax = (int)(va - az * plane - (int64_t)ay * nx);
        const int bz = (int)(vb / plane), by = (int)((vb - bz * plane) / nx), bx = (int)(vb - bz * plane - (int64_t)by * nx);
        const int dx = bx - ax, dy = by - ay, dz = bz - az;
        if (!vp_in(dx, dy, dz)) return PGD_OK;                                  // the edge leaves the pattern
        int t = 0;
        for (int s = 1; s < 15; ++s) if (vp_x(s) == dx && vp_y(s) == dy && vp_z(s) == dz) t = s;
        const int tb = t < 8 ? t + 7 : t - 7;                                   // the same edge seen from its other end
        int &sa = v2e[(size_t)((t - 1) * nvert + va)], &sb = v2e[(size_t)((tb - 1) * nvert + vb)];
        if (sa != -1 || sb != -1) return PGD_OK;                                // a (vertex, pattern vector) slot taken twice
        sa = sb = (int)(nvert + e);
        par[(size_t)(nvert + e)] = (int)va;
        par[(size_t)(nnode + nvert + e)] = (int)vb;
    }
    bool ok = hipMalloc((void **)&p2->p2_par, par.size() * sizeof(int) + PAD_BYTES) == hipSuccess;
    ok = ok && hipMalloc((void **)&p2->p2_v2e, v2e.size() * sizeof(int) + PAD_BYTES) == hipSuccess;
    ok = ok && hipMemcpyAsync(p2->p2_par, par.data(), par.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(p2->p2_v2e, v2e.data(), v2e.size() * sizeof(int), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;                   // (the host arrays go out of scope)
    if (!ok) {
        (void)hipGetLastError();
        if (p2->p2_par) { (void)hipFree(p2->p2_par); p2->p2_par = nullptr; }
        if (p2->p2_v2e) { (void)hipFree(p2->p2_v2e); p2->p2_v2e = nullptr; }
        return PGD_OK;
    }
    p2->p2_nx = nx; p2->p2_ny = ny; p2->p2_nz = nz; p2->p2_nvert = nvert;
    p2->p2_bound = 1;
    if (ascending && nx >= 3 && ny >= 3 && nz >= 3)
        p2->p2_lat = 3 * nnode < ((int64_t)1 << 31) ? 3 : 2 * nnode < ((int64_t)1 << 31) ? 2 : 1;
    *bound = 1;
    return PGD_OK;
}

int pgd_pmg_counts(pgd_handle h, int64_t *solves, int64_t *fallbacks, int64_t *levels) {
    PGD_CTX(c, h);
    PGD_PUT(levels, c->pmg ? vmg_levels(c->pmg->comp[0]) : 0);
    return cycle_read(c->cycle[PGD_PCG_PRECOND_PMG], solves, fallbacks, nullptr, nullptr);
}

int pgd_pmg_times(pgd_handle h, double *setup_ms, int64_t *march_passes) {
    PGD_CTX(c, h);
    return cycle_read(c->cycle[PGD_PCG_PRECOND_PMG], nullptr, nullptr, setup_ms, march_passes);
}

int pgd_pmg_coarse(pgd_handle h, int comp, double *slots_out, uint8_t *el_out) {
    PGD_CTX(c, h);
    Pmg *G = c->pmg;
    if (!G || comp < 0 || comp >= G->ncomp || !G->comp[comp] || !slots_out || !el_out) return fail(c, PGD_ERR_INVALID, "pmg_coarse: no such component hierarchy");
    const VLevel &L0 = G->comp[comp]->lv[0];
    PGD_HIP(c, hipMemcpyAsync(slots_out, L0.a, 8 * (size_t)L0.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipMemcpyAsync(el_out, L0.el, (size_t)L0.n, hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    return PGD_OK;
}

}  // extern "C"
