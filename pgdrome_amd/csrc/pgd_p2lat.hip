// k_spmv_p2lat - the product of an operator on a P2 layout (scalar, or blocked with 2 or 3 components) over a 3-D box lattice from its
// row-class form (PGD_TUNE_SPMV_P2_LATTICE, opt-in).
//
// A P2 row on the 6-tetrahedra-per-cube box carries 19 to 65 entries per component, so k_spmv_csr (pgd_spmv.hip), which stages 16
// entries per row, walks such rows straight from global memory: every lane its own segment of `vals` and `cols`, 12 B per entry,
// every x gathered through a column index read from memory.  On a bound box lattice (pgd_mesh_p2_bind, pgd_pmg.hip) the columns
// need no index.  The frontend numbers the vertices first, in lattice order, then the edges with their keys lo * nvert + hi
// ascending, so every node is a pair (anchor vertex I, class g): g = 0 the vertex itself, g = dx + 2 dy + 4 dz in 1..7 the midpoint
// of the edge from I to I + (dx, dy, dz), and the edge nodes ascend with I first, then with g.  In half steps the node sits at
// 2 I + (dx, dy, dz): the P2 nodes fill the lattice of half steps, and the columns of a row of class g are a FIXED table of
// (vertex offset in {-1, 0, 1}^3, class) pairs - 65 for a vertex, 27 for an edge along an axis or along the cube's diagonal, 19 for
// an edge along a face diagonal.  The tables are built on the host from the six tetrahedra of the unit cube (p2lat_tables).  Slot
// order - the vertex columns first in lattice order of the offset, then the edge columns in lattice order of the anchor's offset
// and ascending class inside it - is ascending node order once every axis has 3 vertices, so the slots a row stores, in slot
// order, are its sorted CSR row.
//
// The operator is then one double per (row, slot, column component), in arrays indexed by row (Csr::p2lat): 65 ncomp arrays over the
// vertex rows and 27 ncomp arrays over the edge rows (the 19-wide classes padded with an exact 0.0), about 1.12 times the CSR value
// array, read fully coalesced: 8 B per slot, no column stream.  The neighbour's node id comes per node pair, not per entry: the
// anchor's lattice position plus the table's offset, and for an edge column one read of Mesh::p2_v2e (L1 / L2: the ncomp^2
// entries of a node pair and the neighbouring lanes share it).
//
// The kernel runs the chain k_spmv_csr runs - one row per lane, lane = row in the frontend's numbering, acc = 0.0, one fma per entry
// in ascending column order - on the same rows per workgroup with the same epilogue.  A slot the row does not store holds 0.0 and
// meets a finite x (the row's own): fma(0.0, x, acc) = acc, up to the sign of a zero.  y and the partial sums are those of the CSR
// launch; every solve on top of them is the CSR-product solve bit for bit.  No lane forms an address from a position outside the
// lattice or from a -1 of p2_v2e: such a slot reads index 0 of the table and the row's own x.
#include "pgd_internal.h"

#include <algorithm>
#include <vector>

namespace pgd {

constexpr int P2L_WV = 65, P2L_WE = 27;                 // slots of a vertex row, of an edge row (19-wide classes padded)
constexpr int P2L_TAB = 8 * P2L_WV;                     // entries of the (offset, class)-of-a-slot table: [class][slot]
constexpr int P2L_SLOT = 8 * 27 * 8;                    // ... and of its inverse: [class][offset code][class]
constexpr uint16_t P2L_NONE = 0xffff;

// (offset, class) in 9 bits: class | ox + 1 << 3 | oy + 1 << 5 | oz + 1 << 7
__host__ __device__ constexpr int p2l_code(int ox, int oy, int oz, int g) { return g | (ox + 1) << 3 | (oy + 1) << 5 | (oz + 1) << 7; }
__host__ __device__ constexpr int p2l_offcode(int ox, int oy, int oz) { return (ox + 1) + 3 * (oy + 1) + 9 * (oz + 1); }

struct P2Lattice {
    const int *par, *v2e;        // Mesh::p2_par, Mesh::p2_v2e of the bound scalar layout
    int nvert, nnode, nx, ny, nz;
};

struct P2Args {
    const double *av, *ae, *x, *w;
    double *y, *partials;
    const int *flags;
    const uint16_t *tab;
    int64_t sv, se;              // doubles between two arrays of the vertex / edge segment
    int n, nvr;                  // rows, vertex rows (ncomp nvert)
    P2Lattice L;
};

// (anchor vertex, class) of a node: the binding has checked that an edge node's parents differ by a positive pattern vector
__device__ __forceinline__ void p2l_node(const P2Lattice &L, int node, int *I, int *g) {
    if (node < L.nvert) { *I = node; *g = 0; return; }
    const int va = L.par[node], vb = L.par[L.nnode + node];
    const int P = L.nx * L.ny;
    int diff = vb - va;
    const int dz = diff >= P ? 1 : 0;
    diff -= dz * P;
    const int dy = diff >= L.nx ? 1 : 0;
    diff -= dy * L.nx;
    *I = va;
    *g = ((diff & 1) | dy << 1 | dz << 2) & 7;
}

__device__ __forceinline__ void p2l_pos(const P2Lattice &L, int i, int *ix, int *iy, int *iz) {
    const int P = L.nx * L.ny;
    *iz = i / P;
    const int rem = i - *iz * P;
    *iy = rem / L.nx;
    *ix = rem - *iy * L.nx;
}

// CSR values -> the zeroed arrays: one lane per row walks its entries and writes its own row's slots (no atomics).  flag[0] is
// raised by a stored entry without a slot in the row's class, a column out of range, a blocked row whose entries do not come in
// runs of nc components, and slots of consecutive entries that do not ascend: the operator keeps the CSR product.
__global__ __launch_bounds__(TPB) void k_p2lat_extract(const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                       const double *__restrict__ vals, int n, int nc, P2Lattice L,
                                                       const int16_t *__restrict__ slot_of, double *__restrict__ av, int64_t sv,
                                                       double *__restrict__ ae, int64_t se, int *__restrict__ flag) {
    const int r = blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    const int node = r / nc, nvr = nc * L.nvert;
    int I, g, ix, iy, iz;
    p2l_node(L, node, &I, &g);
    p2l_pos(L, I, &ix, &iy, &iz);
    bool bad = false;
    int last = -1;
    const int a0 = row_ptr[r], a1 = row_ptr[r + 1];
    for (int k = a0; k < a1; ++k) {
        const int col = cols[k];
        if (col < 0 || col >= n) { bad = true; continue; }
        const int cn = col / nc, d = col - cn * nc;
        int J, gc, jx, jy, jz;
        p2l_node(L, cn, &J, &gc);
        p2l_pos(L, J, &jx, &jy, &jz);
        const int ox = jx - ix, oy = jy - iy, oz = jz - iz;
        if (ox < -1 || ox > 1 || oy < -1 || oy > 1 || oz < -1 || oz > 1) { bad = true; continue; }
        const int s = slot_of[(g * 27 + p2l_offcode(ox, oy, oz)) * 8 + gc];
        if (s < 0 || s >= (r < nvr ? P2L_WV : P2L_WE)) { bad = true; continue; }      // (the second: never on a bound layout; no write outside the segment)
        const int idx = s * nc + d;
        if (idx <= last || d != (k - a0) % nc) bad = true;
        last = idx;
        if (r < nvr) av[(int64_t)idx * sv + r] = vals[k];
        else ae[(int64_t)idx * se + (r - nvr)] = vals[k];
    }
    if (bad) flag[0] = 1;
}

// K slots of the table: the NC values per slot (coalesced, 8 B per lane and array) and the NC x per slot
template <int NC, int K>
__device__ __forceinline__ void p2l_load(const P2Args &A, const double *__restrict__ a, int64_t stride, int64_t rl, const uint16_t *tab,
                                         int s0, int r, int I, int ix, int iy, int iz, double *v, double *xv) {
    const P2Lattice &L = A.L;
    const int P = L.nx * L.ny;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int d = 0; d < NC; ++d) v[j * NC + d] = a[(int64_t)((s0 + j) * NC + d) * stride + rl];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int code = tab[s0 + j];
        const int gc = code & 7, ox = ((code >> 3) & 3) - 1, oy = ((code >> 5) & 3) - 1, oz = ((code >> 7) & 3) - 1;
        const int jx = ix + ox, jy = iy + oy, jz = iz + oz;
        const bool in = code != P2L_NONE && jx >= 0 && jx < L.nx && jy >= 0 && jy < L.ny && jz >= 0 && jz < L.nz;
        const int J = I + ox + L.nx * oy + P * oz;
        // an edge column: its node from the anchor's table (index 0 where there is no anchor: no address from outside the lattice)
        const int e = L.v2e[(in && gc) ? (int64_t)(gc - 1) * L.nvert + J : 0];
        const int nd = !in ? -1 : gc ? e : J;
        // no such neighbour: the coefficient is 0.0, the lane reads its own row's x instead
#pragma unroll
        for (int d = 0; d < NC; ++d) xv[j * NC + d] = A.x[nd >= 0 ? NC * nd + d : r];
    }
}

// the chain over the W slots of a row in blocks of K, the next block's loads in flight while this one is multiplied
template <int NC, int W, int K>
__device__ __forceinline__ double p2l_chain(const P2Args &A, const double *__restrict__ a, int64_t stride, int64_t rl, const uint16_t *tab,
                                            int r, int I, int ix, int iy, int iz) {
    static_assert(W % K == 0, "whole blocks");
    double cv[K * NC], cx[K * NC], nv[K * NC], nx[K * NC];
    p2l_load<NC, K>(A, a, stride, rl, tab, 0, r, I, ix, iy, iz, cv, cx);
    double acc = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < W; s0 += K) {
        if (s0 + K < W) p2l_load<NC, K>(A, a, stride, rl, tab, s0 + K, r, I, ix, iy, iz, nv, nx);
#pragma unroll
        for (int k = 0; k < K * NC; ++k) acc = fma(cv[k], cx[k], acc);
#pragma unroll
        for (int k = 0; k < K * NC; ++k) { cv[k] = nv[k]; cx[k] = nx[k]; }
    }
    return acc;
}

template <bool DOT, bool STORE, int R, int NC>
__global__ __launch_bounds__(R) void k_spmv_p2lat(P2Args A) {
    if (A.flags && A.flags[0]) return;   // PCG already converged: uniform early exit
    // the lanes of a wave carry mixed classes on the edge rows: the table is read per lane, from LDS
    __shared__ __align__(16) uint16_t s_tab[P2L_TAB];
    __shared__ double s_red[R / 64];
    const int tid = threadIdx.x;
    for (int k = tid; k < P2L_TAB / 2; k += R)
        reinterpret_cast<unsigned *>(s_tab)[k] = reinterpret_cast<const unsigned *>(A.tab)[k];
    __syncthreads();
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int r0 = b * R;
    const int nr = min(R, A.n - r0);
    const int r = r0 + (tid < nr ? tid : 0);      // (lanes past the last row re-read the workgroup's first: no predicated loads)
    const int node = r / NC;
    int I, g, ix, iy, iz;
    p2l_node(A.L, node, &I, &g);
    p2l_pos(A.L, I, &ix, &iy, &iz);
    // blocks of 13 / 5 slots of the 65 and 9 / 3 of the 27: 9 to 15 entries (and as many x) per block in flight
    constexpr int KV = NC == 1 ? 13 : 5, KE = NC == 1 ? 9 : 3;
    double acc;
    if (r < A.nvr) acc = p2l_chain<NC, P2L_WV, KV>(A, A.av, A.sv, r, s_tab, r, I, ix, iy, iz);
    else acc = p2l_chain<NC, P2L_WE, KE>(A, A.ae, A.se, r - A.nvr, s_tab + g * P2L_WV, r, I, ix, iy, iz);
    if (STORE && tid < nr) A.y[r0 + tid] = acc;
    if (DOT) {
        const double t = (tid < nr) ? acc * A.w[r0 + tid] : 0.0;
        const double sum = block_sum_n<R / 64>(t, s_red);
        if (tid == 0) A.partials[b] = sum;
    }
}

// The class slot tables from the six tetrahedra of the unit cube - the monotone paths 0 -> e_a -> e_a + e_b -> (1, 1, 1): all pairs
// among the 10 nodes of a tetrahedron in half steps, translated so that the row's anchor is the origin, merged per class.
static void p2lat_tables_host(std::vector<uint16_t> &tab, std::vector<int16_t> &slot_of, int *widths) {
    std::vector<int> codes[8];
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (const int *perm : perms) {
        int v[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int k = 1; k < 4; ++k) {
            for (int a = 0; a < 3; ++a) v[k][a] = v[k - 1][a];
            v[k][perm[k - 1]] = 1;
        }
        int nodes[10][3], nn = 0;
        for (int i = 0; i < 4; ++i, ++nn)
            for (int a = 0; a < 3; ++a) nodes[nn][a] = 2 * v[i][a];
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j, ++nn)
                for (int a = 0; a < 3; ++a) nodes[nn][a] = v[i][a] + v[j][a];
        for (int p = 0; p < 10; ++p) {
            const int g = (nodes[p][0] & 1) | (nodes[p][1] & 1) << 1 | (nodes[p][2] & 1) << 2;
            for (int q = 0; q < 10; ++q) {
                int off[3], cls = 0;
                for (int a = 0; a < 3; ++a) {
                    const int h = (nodes[p][a] & 1) + nodes[q][a] - nodes[p][a];      // -2 .. 2
                    off[a] = (h + 2) / 2 - 1;                                         // floor(h / 2)
                    cls |= (h & 1) << a;
                }
                const int code = p2l_code(off[0], off[1], off[2], cls);
                if (std::find(codes[g].begin(), codes[g].end(), code) == codes[g].end()) codes[g].push_back(code);
            }
        }
    }
    tab.assign(P2L_TAB, P2L_NONE);
    slot_of.assign(P2L_SLOT, (int16_t)-1);
    for (int g = 0; g < 8; ++g) {
        // the vertex columns first, then (offset in lattice order, class): the bit layout of the code orders both
        std::sort(codes[g].begin(), codes[g].end(), [](int a, int b) {
            const bool ea = (a & 7) != 0, eb = (b & 7) != 0;
            return ea != eb ? eb : (a >> 3) != (b >> 3) ? (a >> 3) < (b >> 3) : a < b;
        });
        widths[g] = (int)codes[g].size();
        for (int s = 0; s < widths[g] && s < P2L_WV; ++s) {
            const int code = codes[g][s];
            tab[g * P2L_WV + s] = (uint16_t)code;
            const int oc = ((code >> 3) & 3) + 3 * ((code >> 5) & 3) + 9 * ((code >> 7) & 3);
            slot_of[(g * 27 + oc) * 8 + (code & 7)] = (int16_t)s;
        }
    }
}

// the tables on the device, each direction uploaded once per context; false: they do not have the expected widths or no memory
static bool p2lat_tables(Ctx *c) {
    if (c->p2lat_tab && c->p2lat_slot) return true;
    std::vector<uint16_t> tab;
    std::vector<int16_t> slot_of;
    int widths[8];
    p2lat_tables_host(tab, slot_of, widths);
    static const int expect[8] = {65, 27, 27, 19, 27, 19, 19, 27};
    for (int g = 0; g < 8; ++g)
        if (widths[g] != expect[g]) return false;
    bool ok = hipMalloc((void **)&c->p2lat_tab, tab.size() * sizeof(uint16_t) + PAD_BYTES) == hipSuccess;
    ok = ok && hipMalloc((void **)&c->p2lat_slot, slot_of.size() * sizeof(int16_t) + PAD_BYTES) == hipSuccess;
    ok = ok && hipMemcpyAsync(c->p2lat_tab, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(c->p2lat_slot, slot_of.data(), slot_of.size() * sizeof(int16_t), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;                   // (the host arrays go out of scope)
    if (!ok) { (void)hipGetLastError(); p2lat_release(c); }
    return ok;
}

void p2lat_release(Ctx *c) {
    if (c->p2lat_tab) { (void)hipFree(c->p2lat_tab); c->p2lat_tab = nullptr; }
    if (c->p2lat_slot) { (void)hipFree(c->p2lat_slot); c->p2lat_slot = nullptr; }
    for (hipEvent_t &e : c->p2lat_ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
}

// the scalar layout under m: m itself, or the base of a blocked layout
static const Mesh *p2lat_base(Ctx *c, const Mesh *m) {
    if (m->ncomp == 1) return m;
    const Mesh *base = get_mesh(c, m->base);
    return base && base->ncomp == 1 && m->nv == base->nv * m->ncomp ? base : nullptr;
}

bool p2lat_degree2(Ctx *c, const Mesh *m) {
    const Mesh *base = p2lat_base(c, m);
    return base && base->cellsN && (base->nvpc == 6 || base->nvpc == 10);
}

// the bound lattice under the layout, or false: scalar, or 2 or 3 components over a scalar P2 layout that pgd_mesh_p2_bind has bound
// and found fit for the form
static bool p2lat_lattice(Ctx *c, const Mesh *m, P2Lattice *L) {
    const Mesh *base = p2lat_base(c, m);
    if (!base || m->ncomp < 1 || m->ncomp > 3 || base->p2_bound != 1 || base->p2_lat < m->ncomp || !base->p2_par || !base->p2_v2e) return false;
    if (m->nv >= (int64_t)1 << 31 || base->p2_nx < 3 || base->p2_ny < 3 || base->p2_nz < 3) return false;
    L->par = base->p2_par; L->v2e = base->p2_v2e;
    L->nvert = (int)base->p2_nvert; L->nnode = (int)base->nv;
    L->nx = base->p2_nx; L->ny = base->p2_ny; L->nz = base->p2_nz;
    return true;
}

// the form of the operator's current values: extracted once per `version` (every writer of the CSR values of an operator bumps it)
static int p2lat_ensure(Ctx *c, const Mesh *m, Csr *a, const P2Lattice &L) {
    a->p2lat_seen = a->version;
    a->p2lat_ok = false;
    if (!p2lat_tables(c)) return PGD_OK;
    const int nc = m->ncomp;
    const int64_t nvr = (int64_t)nc * L.nvert, ner = m->nv - nvr;
    const int64_t sv = (nvr + 63) / 64 * 64, se = (ner + 63) / 64 * 64;
    const size_t bytes = ((size_t)P2L_WV * nc * (size_t)sv + (size_t)P2L_WE * nc * (size_t)se) * sizeof(double);
    if (a->p2lat && a->p2lat_bytes != bytes) { dev_release(c, a->p2lat, a->p2lat_bytes); a->p2lat = nullptr; }
    if (!a->p2lat) {
        void *p;
        if (dev_alloc(c, &p, bytes) != PGD_OK) { (void)hipGetLastError(); return PGD_OK; }      // no memory for it: the CSR product
        a->p2lat = (double *)p;
        a->p2lat_bytes = bytes;
    }
    a->p2lat_sv = sv; a->p2lat_se = se;
    PGD_TRY(ensure_vals(c, m, a));
    for (hipEvent_t &e : c->p2lat_ev)
        if (!e) PGD_HIP(c, hipEventCreate(&e));
    int *flag = c->flags + 7;
    PGD_HIP(c, hipEventRecord(c->p2lat_ev[0], c->stream));
    PGD_HIP(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    PGD_HIP(c, hipMemsetAsync(a->p2lat, 0, bytes, c->stream));
    k_p2lat_extract<<<(int)((m->nv + TPB - 1) / TPB), TPB, 0, c->stream>>>(m->row_ptr, m->cols, a->vals, (int)m->nv, nc, L, c->p2lat_slot,
                                                                         a->p2lat, sv, a->p2lat + (size_t)P2L_WV * nc * (size_t)sv, se, flag);
    PGD_LAUNCH_CHECK(c);
    PGD_HIP(c, hipEventRecord(c->p2lat_ev[1], c->stream));
    int bad = 0;
    PGD_HIP(c, hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->p2lat_ev[0], c->p2lat_ev[1]) == hipSuccess) c->form[FORM_P2LAT].extract_ms += (double)ms;
    else (void)hipGetLastError();
    if (bad) {      // the form would not be the operator: it is dropped
        dev_release(c, a->p2lat, a->p2lat_bytes);
        a->p2lat = nullptr;
        a->p2lat_bytes = 0;
        return PGD_OK;
    }
    a->p2lat_ok = true;
    c->form[FORM_P2LAT].forms += 1;
    return PGD_OK;
}

int launch_spmv_p2lat(Ctx *c, const Mesh *m, Csr *a, const double *x, double *y, const double *w, bool dot, bool store,
                      const int *flags, int *nparts_out, bool *done) {
    *done = false;
    P2Lattice L;
    if (a->p2lat_seen != a->version) {
        // decided once per operator, by its first whole-range product.  (A product inside a stream capture cannot synchronise: it
        // takes the CSR form and leaves the decision to the next one outside - pgd_pcg_solve starts with one.)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) { (void)hipGetLastError(); return PGD_OK; }
        if (cap != hipStreamCaptureStatusNone) return PGD_OK;
        if (p2lat_lattice(c, m, &L)) PGD_TRY(p2lat_ensure(c, m, a, L));
        else { a->p2lat_seen = a->version; a->p2lat_ok = false; }
        if (!a->p2lat_ok) c->form[FORM_P2LAT].fallbacks += 1;
    }
    if (!a->p2lat_ok || !a->p2lat || !c->p2lat_tab || !p2lat_lattice(c, m, &L)) return PGD_OK;
    const int R = c->spmv_rows;
    const int nblk = (int)((m->nv + R - 1) / R);
    if (nparts_out) *nparts_out = nblk;
    *done = true;
    if (nblk == 0) return PGD_OK;
    if (dot) PGD_TRY(ensure_partials(c, std::max<int64_t>(c->partials_off + nblk, 4 * MAX_VEC_BLOCKS)));
    P2Args A;
    A.av = a->p2lat; A.ae = a->p2lat + (size_t)P2L_WV * m->ncomp * (size_t)a->p2lat_sv;
    A.x = x; A.w = w; A.y = y; A.partials = c->partials + c->partials_off; A.flags = flags; A.tab = c->p2lat_tab;
    A.sv = a->p2lat_sv; A.se = a->p2lat_se; A.n = (int)m->nv; A.nvr = m->ncomp * L.nvert; A.L = L;
    bool timed = false;
    PGD_TRY(prof_begin(c, dot, store, &timed));
#define PGD_P2LAT_R(D, S, NC)                                                               \
    do {                                                                                    \
        if (R == 256) k_spmv_p2lat<D, S, 256, NC><<<nblk, 256, 0, c->stream>>>(A);          \
        else if (R == 128) k_spmv_p2lat<D, S, 128, NC><<<nblk, 128, 0, c->stream>>>(A);     \
        else k_spmv_p2lat<D, S, 64, NC><<<nblk, 64, 0, c->stream>>>(A);                     \
    } while (0)
#define PGD_P2LAT_LAUNCH(D, S)                                                              \
    do {                                                                                    \
        if (m->ncomp == 3) PGD_P2LAT_R(D, S, 3);                                            \
        else if (m->ncomp == 2) PGD_P2LAT_R(D, S, 2);                                       \
        else PGD_P2LAT_R(D, S, 1);                                                          \
    } while (0)
    if (dot && store) PGD_P2LAT_LAUNCH(true, true);
    else if (dot) PGD_P2LAT_LAUNCH(true, false);
    else PGD_P2LAT_LAUNCH(false, true);
#undef PGD_P2LAT_LAUNCH
#undef PGD_P2LAT_R
    c->form[FORM_P2LAT].products += 1;
    if (timed) {
        const double per_row = 8.0 * ((double)P2L_WV * A.nvr + (double)P2L_WE * (m->nv - A.nvr)) * m->ncomp / (double)std::max<int64_t>(m->nv, 1);
        PGD_TRY(prof_end(c, m, m->nv, per_row + 16.0 + (dot && w != x ? 8.0 : 0.0)));
    }
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_p2lat_counts(pgd_handle h, int64_t *forms_built, int64_t *products, int64_t *fallbacks) {
    PGD_CTX(c, h);
    return form_read(c->form[FORM_P2LAT], forms_built, products, fallbacks, nullptr);
}

int pgd_p2lat_times(pgd_handle h, double *extract_ms) {
    PGD_CTX(c, h);
    return form_read(c->form[FORM_P2LAT], nullptr, nullptr, nullptr, extract_ms);
}

}  // extern "C"
