// The z-march of the diagonal form, two rows per thread: ONE body for the product (k_spmv_dia_march2, pgd_spmv.hip) and for the two
// level passes of the variable-coefficient V-cycle (k_vmg_march, pgd_vmg.hip).  Both kernels are __global__ wrappers around it.
#pragma once

#include "pgd_internal.h"

namespace pgd {

struct DiaArgs {
    const double *uvals, *x, *w;
    double *y, *partials;
    const int *flags;
    int64_t n;              // slot stride in doubles
    int nx, ny, nz;         // vertex grid of the (local) mesh
    int row_begin, row_end; // k_spmv_dia_rows
    int nblk1, row_begin2, row_end2;   // ... with a second row range from workgroup nblk1 on (nblk1 < 0: one range)
    int z0, z1, zchunk, tiles_x, tiles_y;   // k_spmv_dia_march
    int unit_diag;          // the operator is D^-1/2 A D^-1/2 of the scaled recurrence: its diagonal is 1 and is not loaded
    int qq;                 // DOT launches: partial sums in pairs (w . y, y . y) per workgroup (single-sync recurrence)
    const double *eb = nullptr, *ew = nullptr;   // epilogues of the cycle (dia_march2 with EPI != 0): right-hand side b, weights w
};

constexpr int DM_HX = 66;            // cells per line of the staged x patch: 64 + one halo cell each way

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a workgroup-scope fence + s_barrier, and on gfx9
// the fence waits with vmcnt(0), i.e. also for the acknowledgement of the y store issued just before it in every step
// of the march.  Nothing another wave reads through LDS depends on that store, so the march waits for its LDS
// operations only (measured A/B in one process at 256^3: no difference with five workgroups per CU to overlap the
// wait; kept because it is the weaker - and sufficient - ordering).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Two rows per thread: the march on a 64 x 8 patch with 256 threads - thread (lane, wave) owns the rows y0 + 2 wave and
// y0 + 2 wave + 1 and marches through the planes [z0 + chunk zchunk, ...) of its workgroup.  Three planes of the input live in an
// LDS ring, the plane-below couplings are the LDS copy of the workgroup's own slots 4..7 of one step earlier; the upper row takes
// its (0, -1, 0) coupling from the lower row's registers and its plane-below (0, -1, -1) coupling from the thread's own LDS cell.
// Same per-row arithmetic and order as k_spmv_dia_march (ascending columns): bit-identical to it.
//   EPI 0: y = A x;  DOT: partial sums of y . x (qq: in pairs with y . y) per workgroup; STORE: y is written
//   EPI 1: staged u = ew x;  y = x - A u on rows with ew != 0, 0 on the others                    (x = the level's right-hand side)
//   EPI 2: staged v = x;     y = v + ew (eb - A v), 0 where ew = 0;  DOT: partial sums of eb . y  (x = the prolongated vector)
// EPI 1 and 2 always store; y must not alias x, eb, ew or the slot arrays (lds_barrier does not wait for the y stores).
template <bool DOT, bool STORE, int EPI>
__device__ __forceinline__ void dia_march2(const DiaArgs &A) {
    constexpr int NT = 256, PY = 8, HY = PY + 2, SLICE = DM_HX * HY;        // 660 cells per plane
    __shared__ double s_x[3 * SLICE];
    __shared__ double s_lo[2 * 4 * NT];                     // [row of the pair][slot 4..7][thread]
    __shared__ double s_red[4];
    if (A.flags && A.flags[0]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int per_chunk = A.tiles_x * A.tiles_y;
    const int chunk = b / per_chunk, tile = b - chunk * per_chunk;
    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int x0 = tx * 64, y0 = ty * PY;
    const int x = x0 + lane, ya = y0 + 2 * wv;
    const bool live0 = x < A.nx && ya < A.ny, live1 = x < A.nx && ya + 1 < A.ny;
    const bool inx0 = live0 && x > 0, inx1 = live1 && x > 0;
    const bool iny0 = live0 && ya > 0;                      // the upper row of the pair always has its y - 1 neighbour: the lower row
    const bool ldx = lane > 0, ldy = wv > 0;
    const int64_t nx = A.nx, P = (int64_t)A.nx * A.ny, n = A.n;
    const int64_t base0 = live0 ? x + nx * ya : 0, base1 = live1 ? x + nx * (ya + 1) : 0;
    const int centre = (2 * wv + 1) * DM_HX + lane + 1;     // the lower row of the pair; the upper one at + DM_HX
    const int za = A.z0 + chunk * A.zchunk, zb = min(A.z1, za + A.zchunk);
    int64_t goff[3];
    bool gok[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = tid + q * NT;
        const int ly = i / DM_HX, lx = i - ly * DM_HX;
        const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
        gok[q] = i < SLICE && gx >= 0 && gx < A.nx && gy >= 0 && gy < A.ny;
        goff[q] = gok[q] ? gx + nx * gy : 0;
    }
    auto fetch = [&](int z, double v[3]) {
        const bool zok = z >= 0 && z < A.nz;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if constexpr (EPI == 1) v[q] = (zok && gok[q]) ? A.ew[goff[q] + P * z] * A.x[goff[q] + P * z] : 0.0;      // staged u = w x
            else v[q] = (zok && gok[q]) ? A.x[goff[q] + P * z] : 0.0;
        }
    };
    auto put = [&](int z, const double v[3]) {
        const int sl = ((z % 3) + 3) % 3;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (tid + q * NT < SLICE) s_x[sl * SLICE + tid + q * NT] = v[q];
    };
    double dot = 0.0, dot2 = 0.0;
    if (za < zb) {
        double v[3];
        for (int z = za - 1; z <= za + 1; ++z) { fetch(z, v); put(z, v); }
        if (za > 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                s_lo[s * NT + tid] = A.uvals[(int64_t)(4 + s) * n + base0 + P * (za - 1)];
                s_lo[(4 + s) * NT + tid] = A.uvals[(int64_t)(4 + s) * n + base1 + P * (za - 1)];
            }
        }
    }
    __syncthreads();
    for (int z = za; z < zb; ++z) {
        double vn[3] = {0.0, 0.0, 0.0};
        if (z + 2 <= zb) fetch(z + 2, vn);                  // plane zb + 1 is never read
        const int64_t r0 = base0 + P * z, r1 = base1 + P * z;
        double u0[8], u1[8];
        u0[0] = u1[0] = 1.0;                                // unit diagonal of the scaled operator: 56 instead of 64 B of slots per row
        if (!A.unit_diag) { u0[0] = A.uvals[r0]; u1[0] = A.uvals[r1]; }
#pragma unroll
        for (int s = 1; s < 8; ++s) { u0[s] = A.uvals[(int64_t)s * n + r0]; u1[s] = A.uvals[(int64_t)s * n + r1]; }
        // the rows' own vector entries of the cycle's epilogues (EPI 1: x = the right-hand side; EPI 2: eb)
        double w0 = 0.0, w1 = 0.0, e0 = 0.0, e1 = 0.0;
        if constexpr (EPI != 0) {
            w0 = A.ew[r0]; w1 = A.ew[r1];
            e0 = EPI == 1 ? A.x[r0] : A.eb[r0]; e1 = EPI == 1 ? A.x[r1] : A.eb[r1];
        }
        // in-plane lower couplings from the neighbouring rows' slots (L1 / L2); (0, -1) of the upper row = u0[2]
        const double t1a = A.uvals[1 * n + (inx0 ? r0 - 1 : r0)];
        const double t2a = A.uvals[2 * n + (iny0 ? r0 - nx : r0)];
        const double t3a = A.uvals[3 * n + ((inx0 && iny0) ? r0 - nx - 1 : r0)];
        const double t1b = A.uvals[1 * n + (inx1 ? r1 - 1 : r1)];
        const double t3b = A.uvals[3 * n + (inx1 ? r1 - nx - 1 : r1)];
        double a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0, b4 = 0.0, b5 = 0.0, b6 = 0.0, b7 = 0.0;
        if (z > 0) {                                        // uniform
            a4 = live0 ? s_lo[tid] : 0.0;
            b4 = live1 ? s_lo[4 * NT + tid] : 0.0;
            if (inx0) a5 = ldx ? s_lo[NT + tid - 1] : A.uvals[5 * n + r0 - P - 1];
            if (inx1) b5 = ldx ? s_lo[5 * NT + tid - 1] : A.uvals[5 * n + r1 - P - 1];
            if (iny0) a6 = ldy ? s_lo[6 * NT + tid - 64] : A.uvals[6 * n + r0 - P - nx];      // row below the pair: upper row of wave - 1
            if (live1) b6 = s_lo[2 * NT + tid];                                                // the pair's own lower row
            if (inx0 && iny0) a7 = (ldx && ldy) ? s_lo[7 * NT + tid - 65] : A.uvals[7 * n + r0 - P - nx - 1];
            if (inx1) b7 = ldx ? s_lo[3 * NT + tid - 1] : A.uvals[7 * n + r1 - P - nx - 1];
        }
        const double a1 = inx0 ? t1a : 0.0, a2 = iny0 ? t2a : 0.0, a3 = (inx0 && iny0) ? t3a : 0.0;
        const double b1 = inx1 ? t1b : 0.0, b2 = live1 ? u0[2] : 0.0, b3 = inx1 ? t3b : 0.0;
        const int sl0 = ((z - 1) % 3 + 3) % 3;
        const double *xm = s_x + sl0 * SLICE + centre;
        const double *xc = s_x + ((sl0 + 1) % 3) * SLICE + centre;
        const double *xp = s_x + ((sl0 + 2) % 3) * SLICE + centre;
        const double xa = xc[0], xb = xc[DM_HX];
        double acc0 = a7 * xm[-DM_HX - 1];
        acc0 = fma(a6, xm[-DM_HX], acc0);
        acc0 = fma(a5, xm[-1], acc0);
        acc0 = fma(a4, xm[0], acc0);
        acc0 = fma(a3, xc[-DM_HX - 1], acc0);
        acc0 = fma(a2, xc[-DM_HX], acc0);
        acc0 = fma(a1, xc[-1], acc0);
        acc0 = fma(u0[0], xa, acc0);
        acc0 = fma(u0[1], xc[1], acc0);
        acc0 = fma(u0[2], xc[DM_HX], acc0);
        acc0 = fma(u0[3], xc[DM_HX + 1], acc0);
        acc0 = fma(u0[4], xp[0], acc0);
        acc0 = fma(u0[5], xp[1], acc0);
        acc0 = fma(u0[6], xp[DM_HX], acc0);
        acc0 = fma(u0[7], xp[DM_HX + 1], acc0);
        double acc1 = b7 * xm[-1];
        acc1 = fma(b6, xm[0], acc1);
        acc1 = fma(b5, xm[DM_HX - 1], acc1);
        acc1 = fma(b4, xm[DM_HX], acc1);
        acc1 = fma(b3, xc[-1], acc1);
        acc1 = fma(b2, xc[0], acc1);
        acc1 = fma(b1, xc[DM_HX - 1], acc1);
        acc1 = fma(u1[0], xb, acc1);
        acc1 = fma(u1[1], xc[DM_HX + 1], acc1);
        acc1 = fma(u1[2], xc[2 * DM_HX], acc1);
        acc1 = fma(u1[3], xc[2 * DM_HX + 1], acc1);
        acc1 = fma(u1[4], xp[DM_HX], acc1);
        acc1 = fma(u1[5], xp[DM_HX + 1], acc1);
        acc1 = fma(u1[6], xp[2 * DM_HX], acc1);
        acc1 = fma(u1[7], xp[2 * DM_HX + 1], acc1);
        if constexpr (EPI == 0) {
            if (STORE && live0) A.y[r0] = acc0;
            if (STORE && live1) A.y[r1] = acc1;
            if (DOT && live0) { dot = fma(acc0, xa, dot); dot2 = fma(acc0, acc0, dot2); }
            if (DOT && live1) { dot = fma(acc1, xb, dot); dot2 = fma(acc1, acc1, dot2); }
        } else {
            double o0, o1;
            if (EPI == 1) { o0 = w0 != 0.0 ? e0 - acc0 : 0.0; o1 = w1 != 0.0 ? e1 - acc1 : 0.0; }
            else { o0 = w0 != 0.0 ? fma(w0, e0 - acc0, xa) : 0.0; o1 = w1 != 0.0 ? fma(w1, e1 - acc1, xb) : 0.0; }
            if (live0) A.y[r0] = o0;
            if (live1) A.y[r1] = o1;
            if (DOT && live0) dot = fma(e0, o0, dot);
            if (DOT && live1) dot = fma(e1, o1, dot);
        }
        lds_barrier();
        put(z + 2, vn);
#pragma unroll
        for (int s = 0; s < 4; ++s) { s_lo[s * NT + tid] = u0[4 + s]; s_lo[(4 + s) * NT + tid] = u1[4 + s]; }
        lds_barrier();
    }
    if (DOT) {
        const int qq = EPI == 0 ? A.qq : 0;
        for (int pass = 0; pass < (qq ? 2 : 1); ++pass) {
            const double sum = wave_sum(pass ? dot2 : dot);
            __syncthreads();
            if (lane == 0) s_red[wv] = sum;
            __syncthreads();
            if (tid == 0) A.partials[qq ? 2 * b + pass : b] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        }
    }
}

}  // namespace pgd
