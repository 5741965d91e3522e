// k_spmv_bdia - the product of an operator on a BLOCKED (vector-valued) P1 layout over a 3-D box lattice from its row-diagonal
// form (PGD_TUNE_SPMV_BLOCK_DIA, opt-in).
//
// A blocked row over the 15-point lattice pattern has up to 15 ncomp entries, so k_spmv_csr (pgd_spmv.hip), which stages 16 entries
// per row, walks such rows straight from global memory: every lane its own segment of `vals` and `cols`, 12 B per entry and
// 15 ncomp * 12 B from the next lane's, every x gathered through a column index read from memory.  On a box lattice the columns of
// row r = ncomp i + c need no index: they are ncomp (i + off_t) + d for the 15 pattern offsets off_t and d < ncomp.  The operator
// is then 15 ncomp arrays of one double per row (Csr::bdia), read fully coalesced: 8 B per stored slot, no column stream.
//
// t = 0..14 numbers the offsets in ascending node offset, -P-nx-1, -P-nx, -P-1, -P, -nx-1, -nx, -1, 0, +1, +nx, +nx+1, +P, +P+1,
// +P+nx, +P+nx+1 (P = nx ny): offset t is sign (dx + nx dy + P dz) with s = |t - 7| = dx + 2 dy + 4 dz, the slot numbering of the
// scalar diagonal form.  With nx, ny >= 2 these are strictly ascending, so t ascending and d ascending inside t is the sorted CSR
// row.  The kernel runs the chain k_spmv_csr runs - one row per lane, acc = 0.0, one fma per entry in ascending column order - on
// the same row-to-lane and row-to-workgroup assignment, with the same epilogue.  A slot the row does not store holds an exact 0.0
// and meets a finite x (the row's own): fma(0.0, x, acc) = acc, up to the sign of a zero.  y and the partial sums are those of the
// CSR launch; every solve on top of them is the CSR-product solve bit for bit.
#include "pgd_internal.h"

#include <algorithm>

namespace pgd {

struct BdiaArgs {
    const double *bd, *x, *w;
    double *y, *partials;
    const int *flags;
    int64_t stride;          // doubles between two of the 15 ncomp arrays
    int nv, nx, ny, nz;
};

// lattice position of node i
__device__ __forceinline__ void bdia_node(int i, int nx, int ny, int *ix, int *iy, int *iz) {
    const int P = nx * ny;
    *iz = i / P;
    const int rem = i - *iz * P;
    *iy = rem / nx;
    *ix = rem - *iy * nx;
}

// CSR values -> the zeroed arrays: one lane per row walks its entries and writes its own row's slots (no atomics).  A stored entry
// whose column is not a pattern neighbour of the row's node raises flag[0]: the operator keeps the CSR product.
__global__ __launch_bounds__(TPB) void k_bdia_extract(const int *__restrict__ row_ptr, const int *__restrict__ cols,
                                                      const double *__restrict__ vals, int nv, int nc, int nx, int ny,
                                                      int64_t stride, double *__restrict__ bd, int *__restrict__ flag) {
    const int r = blockIdx.x * TPB + threadIdx.x;
    if (r >= nv) return;
    const int i = r / nc;
    int ix, iy, iz;
    bdia_node(i, nx, ny, &ix, &iy, &iz);
    bool bad = false;
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; ++k) {
        const int col = cols[k];
        const int j = col / nc, d = col - j * nc;
        int jx, jy, jz;
        bdia_node(j, nx, ny, &jx, &jy, &jz);
        const int dx = jx - ix, dy = jy - iy, dz = jz - iz;
        const int lo = min(dx, min(dy, dz)), hi = max(dx, max(dy, dz));
        // the pattern: all three steps in {0, +1} or all three in {0, -1}
        if (col < 0 || col >= nv || lo < -1 || hi > 1 || (lo < 0 && hi > 0)) { bad = true; continue; }
        const int s = abs(dx) + 2 * abs(dy) + 4 * abs(dz);
        const int t = lo < 0 ? 7 - s : 7 + s;
        bd[(int64_t)(t * nc + d) * stride + r] = vals[k];
    }
    if (bad) flag[0] = 1;
}

template <bool DOT, bool STORE, int R, int NC>
__global__ __launch_bounds__(R) void k_spmv_bdia(BdiaArgs A) {
    if (A.flags && A.flags[0]) return;   // PCG already converged: uniform early exit
    __shared__ double s_red[R / 64];
    const int tid = threadIdx.x;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int r0 = b * R;
    const int nr = min(R, A.nv - r0);
    const int r = r0 + (tid < nr ? tid : 0);      // (lanes past the last row re-read the workgroup's first: no predicated loads)
    const int i = r / NC;
    int ix, iy, iz;
    bdia_node(i, A.nx, A.ny, &ix, &iy, &iz);
    const int P = A.nx * A.ny;
    // all 15 NC value loads (coalesced, 8 B per lane and array) and all x loads (L1 / L2: the rows of a node and the neighbouring
    // waves share them) are issued before the chain starts
    double av[15 * NC], xv[15 * NC];
#pragma unroll
    for (int k = 0; k < 15 * NC; ++k) av[k] = A.bd[(int64_t)k * A.stride + r];
#pragma unroll
    for (int t = 0; t < 15; ++t) {
        const int s = t < 7 ? 7 - t : t - 7;
        const int dx = s & 1, dy = (s >> 1) & 1, dz = s >> 2;
        const int off = dx + A.nx * dy + P * dz;
        const bool ok = t < 7 ? (ix >= dx && iy >= dy && iz >= dz) : (ix + dx < A.nx && iy + dy < A.ny && iz + dz < A.nz);
        const int j = t < 7 ? i - off : i + off;
        // a neighbour outside the lattice: the coefficient is 0.0, the lane reads its own row's x instead
#pragma unroll
        for (int d = 0; d < NC; ++d) xv[t * NC + d] = A.x[ok ? NC * j + d : r];
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 15 * NC; ++k) acc = fma(av[k], xv[k], acc);
    if (STORE && tid < nr) A.y[r0 + tid] = acc;
    if (DOT) {
        const double t = (tid < nr) ? acc * A.w[r0 + tid] : 0.0;
        const double sum = block_sum_n<R / 64>(t, s_red);
        if (tid == 0) A.partials[b] = sum;
    }
}

// the lattice under a blocked layout, or false: 2 or 3 components over a scalar 3-D P1 layout in diagonal form, at least two nodes
// along every axis
static bool bdia_lattice(Ctx *c, const Mesh *m, int *nx, int *ny, int *nz) {
    if (m->ncomp < 2 || m->ncomp > 3) return false;
    const Mesh *base = get_mesh(c, m->base);
    if (!base || base->ncomp != 1 || base->gdim != 3 || base->cellsN || base->sym_nx <= 0 || base->sym_ny <= 0 ||
        m->nv != base->nv * m->ncomp) return false;
    const int64_t plane = (int64_t)base->sym_nx * base->sym_ny;
    if (base->nv % plane != 0) return false;
    *nx = base->sym_nx; *ny = base->sym_ny; *nz = (int)(base->nv / plane);
    return *nx >= 2 && *ny >= 2 && *nz >= 2;
}

// the form of the operator's current values: extracted once per `version` (every writer of the CSR values of an operator bumps it)
static int bdia_ensure(Ctx *c, const Mesh *m, Csr *a, int nx, int ny) {
    a->bdia_seen = a->version;
    a->bdia_ok = false;
    const int64_t stride = (m->nv + 63) / 64 * 64;
    const size_t bytes = (size_t)15 * (size_t)m->ncomp * (size_t)stride * sizeof(double);
    if (a->bdia && a->bdia_bytes != bytes) { dev_release(c, a->bdia, a->bdia_bytes); a->bdia = nullptr; }
    if (!a->bdia) {
        void *p;
        if (dev_alloc(c, &p, bytes) != PGD_OK) { (void)hipGetLastError(); return PGD_OK; }      // no memory for it: the CSR product
        a->bdia = (double *)p;
        a->bdia_bytes = bytes;
    }
    a->bdia_stride = stride;
    PGD_TRY(ensure_vals(c, m, a));
    for (hipEvent_t &e : c->bdia_ev)
        if (!e) PGD_HIP(c, hipEventCreate(&e));
    int *flag = c->flags + 6;
    PGD_HIP(c, hipEventRecord(c->bdia_ev[0], c->stream));
    PGD_HIP(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    PGD_HIP(c, hipMemsetAsync(a->bdia, 0, bytes, c->stream));
    k_bdia_extract<<<(int)((m->nv + TPB - 1) / TPB), TPB, 0, c->stream>>>(m->row_ptr, m->cols, a->vals, (int)m->nv, m->ncomp, nx, ny,
                                                                        stride, a->bdia, flag);
    PGD_LAUNCH_CHECK(c);
    PGD_HIP(c, hipEventRecord(c->bdia_ev[1], c->stream));
    int bad = 0;
    PGD_HIP(c, hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->bdia_ev[0], c->bdia_ev[1]) == hipSuccess) c->form[FORM_BDIA].extract_ms += (double)ms;
    else (void)hipGetLastError();
    if (bad) {      // an entry off the pattern: the form is dropped
        dev_release(c, a->bdia, a->bdia_bytes);
        a->bdia = nullptr;
        a->bdia_bytes = 0;
        return PGD_OK;
    }
    a->bdia_ok = true;
    c->form[FORM_BDIA].forms += 1;
    return PGD_OK;
}

int launch_spmv_bdia(Ctx *c, const Mesh *m, Csr *a, const double *x, double *y, const double *w, bool dot, bool store,
                     const int *flags, int *nparts_out, bool *done) {
    *done = false;
    int nx = 0, ny = 0, nz = 0;
    if (a->bdia_seen != a->version) {
        // decided once per operator, by its first whole-range product.  (A product inside a stream capture cannot synchronise: it
        // takes the CSR form and leaves the decision to the next one outside - pgd_pcg_solve starts with one.)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) { (void)hipGetLastError(); return PGD_OK; }
        if (cap != hipStreamCaptureStatusNone) return PGD_OK;
        if (bdia_lattice(c, m, &nx, &ny, &nz)) PGD_TRY(bdia_ensure(c, m, a, nx, ny));
        else { a->bdia_seen = a->version; a->bdia_ok = false; }
        if (!a->bdia_ok) c->form[FORM_BDIA].fallbacks += 1;
    }
    if (!a->bdia_ok || !a->bdia || !bdia_lattice(c, m, &nx, &ny, &nz)) return PGD_OK;
    const int R = c->spmv_rows;
    const int nblk = (int)((m->nv + R - 1) / R);
    if (nparts_out) *nparts_out = nblk;
    *done = true;
    if (nblk == 0) return PGD_OK;
    if (dot) PGD_TRY(ensure_partials(c, std::max<int64_t>(c->partials_off + nblk, 4 * MAX_VEC_BLOCKS)));
    BdiaArgs A;
    A.bd = a->bdia; A.x = x; A.w = w; A.y = y; A.partials = c->partials + c->partials_off; A.flags = flags;
    A.stride = a->bdia_stride; A.nv = (int)m->nv; A.nx = nx; A.ny = ny; A.nz = nz;
    bool timed = false;
    PGD_TRY(prof_begin(c, dot, store, &timed));
#define PGD_BDIA_R(D, S, NC)                                                               \
    do {                                                                                   \
        if (R == 256) k_spmv_bdia<D, S, 256, NC><<<nblk, 256, 0, c->stream>>>(A);          \
        else if (R == 128) k_spmv_bdia<D, S, 128, NC><<<nblk, 128, 0, c->stream>>>(A);     \
        else k_spmv_bdia<D, S, 64, NC><<<nblk, 64, 0, c->stream>>>(A);                     \
    } while (0)
#define PGD_BDIA_LAUNCH(D, S)                                                              \
    do {                                                                                   \
        if (m->ncomp == 3) PGD_BDIA_R(D, S, 3);                                            \
        else PGD_BDIA_R(D, S, 2);                                                          \
    } while (0)
    if (dot && store) PGD_BDIA_LAUNCH(true, true);
    else if (dot) PGD_BDIA_LAUNCH(true, false);
    else PGD_BDIA_LAUNCH(false, true);
#undef PGD_BDIA_LAUNCH
#undef PGD_BDIA_R
    c->form[FORM_BDIA].products += 1;
    if (timed) PGD_TRY(prof_end(c, m, m->nv, 8.0 * 15.0 * m->ncomp + 16.0 + (dot && w != x ? 8.0 : 0.0)));
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_bdia_counts(pgd_handle h, int64_t *forms_built, int64_t *products, int64_t *fallbacks) {
    PGD_CTX(c, h);
    return form_read(c->form[FORM_BDIA], forms_built, products, fallbacks, nullptr);
}

int pgd_bdia_times(pgd_handle h, double *extract_ms) {
    PGD_CTX(c, h);
    return form_read(c->form[FORM_BDIA], nullptr, nullptr, nullptr, extract_ms);
}

}  // extern "C"
