// Gram blocks of two families of long vectors: out[i][j] = sum_{lo <= r < hi} x_i[r] y_j[r], every vector read ONCE.  The second
// dense product of this library and the second kernel on the matrix unit (v_mfma_f64_16x16x4_f64): a tall-skinny X^T Y whose long
// index is the k index of the fragments.
//
//   * A workgroup of four waves stages GM_RB = 32 consecutive rows of all kx (+ ky) vectors in LDS: 32 consecutive doubles per
//     vector and half wave (coalesced), zero beyond the segment's last row and beyond kx / ky (both padded to a multiple of 16).
//   * Vector v's rows sit at s[v * GM_ST + d] with GM_ST = 34 doubles.  A fragment load is one ds_read_b64 per lane of
//     x_{16 I + (l & 15)}[4 q + (l >> 4)]; that instruction is served in two groups of 32 lanes over 64 banks of 4 bytes, a double
//     takes a bank pair, so a group is conflict-free when its 32 double indices differ mod 32: they are 34 i + {0, 1} + const
//     = 2 i + {0, 1} + const (mod 32) for i = 0 .. 15 - all different (the second group adds 2).  A stride of 32 would put all 16
//     vectors of a group on one bank pair; k_eval_norm_mfma's "16 mod 32" is for its k-major pattern, this one is vector-major.
//     The staging stores of a 32-lane group are 32 consecutive doubles: conflict-free as well.
//   * The waves split the 16 x 16 output tiles (tile t belongs to wave t & 3; the symmetric case holds only the tiles J >= I) and
//     keep their accumulators in registers over all row blocks of a segment: at most 52 tiles per launch, 13 per wave, 4 doubles per lane
//     each (a cross block of more than 52 tiles goes in two launches over the columns: 13 tiles per wave is what 256 registers hold).
//     A[i][kk] = x_{16 I + i}[r + kk] and B[kk][j] = y_{16 J + j}[r + kk] are the same lane map read from the two families;
//     a diagonal tile of the symmetric case passes one register twice.
//   * No atomics.  The rows are cut into segments of a whole number of row blocks whose boundaries depend on (lo, hi) alone
//     (gram_segments: at most 1024); persistent workgroups take segments grid-stride, each segment leaves one kxp x kyp partial in
//     the context's reduction scratch, k_gram_finish adds them in ascending segment order.  Every output is bit-identical for any
//     grid size.  In the symmetric case the finish takes entry (i, j), i > j, from (j, i): the block is symmetric bit for bit.
//
// k_gram_plain stages the same way and runs one fma chain per output entry over ascending rows: the cross-check of the tests
// and the baseline that shows what the matrix unit buys (PGD_TUNE_GRAM_VARIANT).
#include "pgd_internal.h"

#include <algorithm>
#include <vector>

namespace pgd {

constexpr int GM_KMAX = 128;            // vectors per side and call
constexpr int GM_RB = 32;               // rows per staged block
constexpr int GM_ST = 34;               // doubles between two vectors in LDS (2 mod 32: see above)
constexpr int GM_SEG_MAX = 1024;        // segments per call
constexpr int GM_TPW_MAX = 13;          // tiles per wave the MFMA kernel is compiled for: 256 vector registers, two waves per SIMD
constexpr int GM_SEG_MIN_BLOCKS = 8;    // row blocks per segment at least (a partial is written per segment)


struct GramVecs { const double *p[2 * GM_KMAX]; };   // x_0 .. at 0, y_0 .. at GM_KMAX

// rows [rb, rb + GM_RB) of the nv = kxp (+ kyp) padded vectors into s[v * GM_ST + d]; four loads in flight per lane
__device__ __forceinline__ void gram_stage(const GramVecs &V, int kx, int ky, int kxp, int nv, int64_t rb, int64_t r1, double *s) {
    const int nit = nv >> 3;            // nv * GM_RB / TPB
    const int d = threadIdx.x & (GM_RB - 1), v0 = threadIdx.x >> 5;
    const bool rv = rb + d < r1;
    for (int it0 = 0; it0 < nit; it0 += 4) {
        double val[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int v = v0 + 8 * (it0 + u);
            val[u] = 0.0;
            if (it0 + u < nit && rv) {
                if (v < kxp) { if (v < kx) val[u] = V.p[v][rb + d]; }
                else if (v - kxp < ky) val[u] = V.p[GM_KMAX + v - kxp][rb + d];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (it0 + u < nit) s[(v0 + 8 * (it0 + u)) * GM_ST + d] = val[u];
    }
}

// The same in two halves for the kernels that fetch the next row block while the matrix unit works on this one: NIT values per
// lane (nv <= 8 NIT) wait in registers from gram_fetch to gram_store
template <int NIT>
__device__ __forceinline__ void gram_fetch(const GramVecs &V, int kx, int ky, int kxp, int nv, int64_t rb, int64_t r1, double (&val)[NIT]) {
    const int nit = nv >> 3;
    const int d = threadIdx.x & (GM_RB - 1), v0 = threadIdx.x >> 5;
    const bool rv = rb + d < r1;
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int v = v0 + 8 * u;
        val[u] = 0.0;
        if (u < nit && rv) {
            if (v < kxp) { if (v < kx) val[u] = V.p[v][rb + d]; }
            else if (v - kxp < ky) val[u] = V.p[GM_KMAX + v - kxp][rb + d];
        }
    }
}

template <int NIT>
__device__ __forceinline__ void gram_store(int nv, const double (&val)[NIT], double *s) {
    const int nit = nv >> 3;
    const int d = threadIdx.x & (GM_RB - 1), v0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < NIT; ++u)
        if (u < nit) s[(v0 + 8 * u) * GM_ST + d] = val[u];
}

// TPW: tiles per wave the kernel is compiled for, ceil(tiles / 4): 1 .. GM_TPW_MAX; NIT > 0: the next row block is fetched into NIT registers per
// lane before this block's products (nv <= 8 NIT), 0: one block at a time (gram_stage)
template <int TPW, int NIT>
__global__ __launch_bounds__(TPB, NIT > 0 ? (TPW <= 3 ? 4 : 2) : TPW <= 6 ? 4 : TPW <= 8 ? 3 : 2) void k_gram_mfma(GramVecs V, int kx, int ky, int sym, int64_t lo, int64_t hi, int64_t seg_rows, int nseg,
                                                   double *__restrict__ part) {
    extern __shared__ double s_dyn[];
    __shared__ int s_tab[64];
    const int kxp = (kx + 15) & ~15, kyp = sym ? kxp : (ky + 15) & ~15;
    const int nv = sym ? kxp : kxp + kyp;
    const double *s_x = s_dyn, *s_y = sym ? s_dyn : s_dyn + kxp * GM_ST;
    const int tI = kxp >> 4, tJ = kyp >> 4;
    const int ntile = sym ? tI * (tI + 1) / 2 : tI * tJ;
    if (threadIdx.x < 64) {             // tile t -> (I, J): row-major, the symmetric case over J >= I
        int t = threadIdx.x, I, J;
        if (sym) {
            I = 0;
            while (I < tI - 1 && t >= tI - I) { t -= tI - I; ++I; }
            J = I + t;
        } else {
            I = t / tJ;
            J = t - I * tJ;
        }
        s_tab[threadIdx.x] = (int)threadIdx.x < ntile ? (I << 8) | J : -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lr = lane & 15, lq = lane >> 4;
    int cnt = 0, aoff[TPW], boff[TPW], tI_[TPW], tJ_[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        const int code = __builtin_amdgcn_readfirstlane(s_tab[wv + 4 * s]);
        tI_[s] = code < 0 ? 0 : code >> 8;
        tJ_[s] = code < 0 ? 0 : code & 255;
        aoff[s] = (16 * tI_[s] + lr) * GM_ST + lq;
        boff[s] = (16 * tJ_[s] + lr) * GM_ST + lq;
        if (code >= 0) cnt = s + 1;      // a wave's tiles are its first cnt slots
    }
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    const int64_t pstride = (int64_t)kxp * kyp;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t r0 = lo + (int64_t)seg * seg_rows, r1 = r0 + seg_rows < hi ? r0 + seg_rows : hi;
        d4_t acc[TPW];
#pragma unroll
        for (int s = 0; s < TPW; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        double val[NIT > 0 ? NIT : 1];
        if constexpr (NIT > 0) gram_fetch<NIT>(V, kx, ky, kxp, nv, r0, r1, val);
        for (int64_t rb = r0; rb < r1; rb += GM_RB) {
            __syncthreads();            // the last block's fragments are read
            if constexpr (NIT > 0) gram_store<NIT>(nv, val, s_dyn);
            else gram_stage(V, kx, ky, kxp, nv, rb, r1, s_dyn);
            __syncthreads();
            if constexpr (NIT > 0) {
                if (rb + GM_RB < r1) gram_fetch<NIT>(V, kx, ky, kxp, nv, rb + GM_RB, r1, val);
            }
#pragma unroll
            for (int q = 0; q < GM_RB / 4; ++q) {
#pragma unroll
                for (int s = 0; s < TPW; ++s) {
                    // (a slot beyond the wave's tiles runs on tile (0, 0) and is never written: a test here would keep two
                    // copies of every accumulator alive)
                    const double a = s_x[aoff[s] + 4 * q];
                    const double b = (sym && tI_[s] == tJ_[s]) ? a : s_y[boff[s] + 4 * q];
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
                }
            }
        }
        // lane holds D[lq + 4 r][lr] of its tiles
        double *ps = part + (int64_t)seg * pstride;
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
            if (s < cnt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) ps[(int64_t)(16 * tI_[s] + lq + 4 * r) * kyp + 16 * tJ_[s] + lr] = acc[s][r];
            }
        }
    }
}

// EPT: entries per thread the kernel is compiled for; thread (ti, tj) = (threadIdx.x >> 4, threadIdx.x & 15) holds entry (ti, tj) of
// the 16 x 16 tiles m = 0 .. tiles - 1, row-major (all of them in the symmetric case too: the finish reads J >= I)
template <int EPT>
__global__ __launch_bounds__(TPB) void k_gram_plain(GramVecs V, int kx, int ky, int sym, int64_t lo, int64_t hi, int64_t seg_rows, int nseg,
                                                    double *__restrict__ part) {
    extern __shared__ double s_dyn[];
    const int kxp = (kx + 15) & ~15, kyp = sym ? kxp : (ky + 15) & ~15;
    const int nv = sym ? kxp : kxp + kyp;
    const int tJ = kyp >> 4, ntile = (kxp >> 4) * tJ;
    const double *s_x = s_dyn + (threadIdx.x >> 4) * GM_ST, *s_y = (sym ? s_dyn : s_dyn + kxp * GM_ST) + (threadIdx.x & 15) * GM_ST;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t r0 = lo + (int64_t)seg * seg_rows, r1 = r0 + seg_rows < hi ? r0 + seg_rows : hi;
        double acc[EPT];
#pragma unroll
        for (int m = 0; m < EPT; ++m) acc[m] = 0.0;
        for (int64_t rb = r0; rb < r1; rb += GM_RB) {
            __syncthreads();
            gram_stage(V, kx, ky, kxp, nv, rb, r1, s_dyn);
            __syncthreads();
#pragma unroll 2
            for (int d = 0; d < GM_RB; ++d) {
#pragma unroll
                for (int m = 0; m < EPT; ++m) {
                    if (m < ntile) {
                        const int I = m / tJ, J = m - I * tJ;
                        acc[m] = fma(s_x[16 * GM_ST * I + d], s_y[16 * GM_ST * J + d], acc[m]);
                    }
                }
            }
        }
        double *ps = part + (int64_t)seg * kxp * kyp + (int64_t)(threadIdx.x >> 4) * kyp + (threadIdx.x & 15);
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            if (m < ntile) {
                const int I = m / tJ, J = m - I * tJ;
                ps[(int64_t)16 * I * kyp + 16 * J] = acc[m];
            }
        }
    }
}

// out[i][j] = the segments' partials of entry (i, j) in ascending order; symmetric case: entry (i, j), i > j, is entry (j, i)
// (ldo, j0: the block is columns [j0, j0 + ky) of rows of ldo entries)
__global__ __launch_bounds__(TPB) void k_gram_finish(const double *__restrict__ part, int nseg, int kx, int ky, int kyp, int64_t pstride,
                                                     int sym, double *__restrict__ out, int ldo, int j0) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= kx * ky) return;
    int i = e / ky, j = e - i * ky;
    if (sym && i > j) { const int t = i; i = j; j = t; }
    const double *p = part + (int64_t)i * kyp + j;
    double t = 0.0;
    for (int seg0 = 0; seg0 < nseg; seg0 += 32) {       // 32 loads in flight, added in ascending order
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = seg0 + u < nseg ? p[(int64_t)(seg0 + u) * pstride] : 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (seg0 + u < nseg) t += v[u];
    }
    out[(e / ky) * ldo + j0 + (e - (e / ky) * ky)] = t;
}

__global__ __launch_bounds__(TPB) void k_copy_range(double *__restrict__ dst, const double *__restrict__ src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) dst[i] = src[i];
}

// segments of [lo, hi): a whole number of row blocks each, a function of the range alone
static void gram_segments(int64_t lo, int64_t hi, int64_t *seg_rows, int *nseg) {
    const int64_t nblk = (hi - lo + GM_RB - 1) / GM_RB;
    const int64_t bps = std::max<int64_t>(GM_SEG_MIN_BLOCKS, (nblk + GM_SEG_MAX - 1) / GM_SEG_MAX);
    *seg_rows = bps * GM_RB;
    *nseg = (int)((nblk + bps - 1) / bps);
}

template <class K>
static int gram_launch(Ctx *c, K kern, size_t lds, int nseg, const GramVecs &V, int kx, int ky, int sym, int64_t lo, int64_t hi,
                       int64_t seg_rows, double *part) {
    PGD_TRY(raise_lds(c, (const void *)kern, lds, "vec_gram"));
    return launch_persistent(c, kern, TPB, lds, nseg, c->gram_grid_max, 0, nullptr, V, kx, ky, sym, lo, hi, seg_rows, nseg, part);
}

// One launch of the variant's kernel on the block and its finish into columns [j0, j0 + ky) of res (rows of ldo entries)
static int gram_block(Ctx *c, const GramVecs &V, int kx, int ky, int sym, int64_t lo, int64_t hi, int64_t seg_rows, int nseg, double *res,
                      int ldo, int j0) {
    const int kxp = (kx + 15) & ~15, kyp = sym ? kxp : (ky + 15) & ~15;
    const int64_t pstride = (int64_t)kxp * kyp;
    PGD_TRY(ensure_partials(c, (int64_t)nseg * pstride));
    const size_t lds = (size_t)(sym ? kxp : kxp + kyp) * GM_ST * sizeof(double);
    if (c->gram_variant != 0) {
        const int tI = kxp >> 4, tJ = kyp >> 4;
        const int tpw = ((sym ? tI * (tI + 1) / 2 : tI * tJ) + 3) / 4;
        const int nv = sym ? kxp : kxp + kyp;
#define GM_CASE(T, N) case T: PGD_TRY(gram_launch(c, k_gram_mfma<T, N>, lds, nseg, V, kx, ky, sym, lo, hi, seg_rows, c->partials)); break;
        if (nv <= 32) {
            switch (tpw) {
                GM_CASE(1, 4)
                default: return fail(c, PGD_ERR_LIMIT, "vec_gram: %d tiles per wave", tpw);
            }
        } else if (nv <= 96) {                  // at most 21 tiles (96 symmetric), 9 in a cross block
            switch (tpw) {
                GM_CASE(1, 12) GM_CASE(2, 12) GM_CASE(3, 12) GM_CASE(4, 12) GM_CASE(5, 12) GM_CASE(6, 12)
                default: return fail(c, PGD_ERR_LIMIT, "vec_gram: %d tiles per wave", tpw);
            }
        } else {
            switch (tpw) {
                GM_CASE(1, 0) GM_CASE(2, 0) GM_CASE(3, 0) GM_CASE(4, 0) GM_CASE(5, 0) GM_CASE(6, 0) GM_CASE(7, 0) GM_CASE(8, 0)
                GM_CASE(9, 0) GM_CASE(10, 0) GM_CASE(11, 0) GM_CASE(12, 0) GM_CASE(13, 0)
                default: return fail(c, PGD_ERR_LIMIT, "vec_gram: %d tiles per wave", tpw);
            }
        }
#undef GM_CASE
    } else {
        const int ept = (int)(pstride / TPB);   // 16 x 16 tiles
        if (ept <= 1) PGD_TRY(gram_launch(c, k_gram_plain<1>, lds, nseg, V, kx, ky, sym, lo, hi, seg_rows, c->partials));
        else if (ept <= 4) PGD_TRY(gram_launch(c, k_gram_plain<4>, lds, nseg, V, kx, ky, sym, lo, hi, seg_rows, c->partials));
        else if (ept <= 16) PGD_TRY(gram_launch(c, k_gram_plain<16>, lds, nseg, V, kx, ky, sym, lo, hi, seg_rows, c->partials));
        else PGD_TRY(gram_launch(c, k_gram_plain<64>, lds, nseg, V, kx, ky, sym, lo, hi, seg_rows, c->partials));
    }
    k_gram_finish<<<(kx * ky + TPB - 1) / TPB, TPB, 0, c->stream>>>(c->partials, nseg, kx, ky, kyp, pstride, sym, res, ldo, j0);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_vec_gram(pgd_handle h, const pgd_handle *xs, int kx, const pgd_handle *ys, int ky, int64_t lo, int64_t hi, double *out) {
    PGD_CTX(c, h);
    if (!xs || !out) return fail(c, PGD_ERR_INVALID, "vec_gram: null handles or output");
    if (kx < 1 || kx > GM_KMAX || ky < 1 || ky > GM_KMAX) return fail(c, PGD_ERR_INVALID, "vec_gram: kx, ky must be 1 .. %d", GM_KMAX);
    const int sym = ys ? 0 : 1;
    if (sym && ky != kx) return fail(c, PGD_ERR_INVALID, "vec_gram: the symmetric case (no ys) needs ky == kx");
    GramVecs V;
    for (int q = 0; q < 2 * GM_KMAX; ++q) V.p[q] = nullptr;
    int64_t n = -1;
    for (int q = 0; q < kx + (sym ? 0 : ky); ++q) {
        Vec *v = get_vec(c, q < kx ? xs[q] : ys[q - kx]);
        if (!v) return fail(c, PGD_ERR_INVALID, "vec_gram: invalid vector %s[%d]", q < kx ? "xs" : "ys", q < kx ? q : q - kx);
        if (n < 0) n = v->n;
        if (v->n != n) return fail(c, PGD_ERR_INVALID, "vec_gram: vectors of different lengths (%lld, %lld)", (long long)n, (long long)v->n);
        V.p[q < kx ? q : GM_KMAX + q - kx] = v->d;
    }
    if (hi < 0) hi = n;
    if (lo < 0 || lo > hi || hi > n) return fail(c, PGD_ERR_INVALID, "vec_gram: bad range");
    for (int e = 0; e < kx * ky; ++e) out[e] = 0.0;
    if (hi == lo) return PGD_OK;
    int64_t seg_rows;
    int nseg;
    gram_segments(lo, hi, &seg_rows, &nseg);
    PGD_TRY(ensure_work(c, 6, (int64_t)GM_KMAX * GM_KMAX));
    double *res = c->work[6];
    const int tI = (kx + 15) >> 4, tJ = (ky + 15) >> 4;
    if (c->gram_variant != 0 && !sym && tI * tJ > 4 * GM_TPW_MAX) {
        // more tiles than four waves hold beside a second workgroup on the CU: the columns in two launches (x is read twice, the
        // matrix unit is the bound at this size; an entry's chain is over the rows, so the split changes no bit)
        const int k0 = 16 * ((tJ + 1) / 2);
        GramVecs W = V;
        for (int q = 0; q < GM_KMAX; ++q) W.p[GM_KMAX + q] = q + k0 < GM_KMAX ? V.p[GM_KMAX + q + k0] : nullptr;
        PGD_TRY(gram_block(c, V, kx, k0, 0, lo, hi, seg_rows, nseg, res, ky, 0));
        PGD_TRY(gram_block(c, W, kx, ky - k0, 0, lo, hi, seg_rows, nseg, res, ky, k0));
    } else {
        PGD_TRY(gram_block(c, V, kx, ky, sym, lo, hi, seg_rows, nseg, res, ky, 0));
    }
    PGD_HIP(c, hipMemcpyAsync(out, res, (size_t)kx * ky * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    return PGD_OK;
}

int pgd_vec_copy_range(pgd_handle h, pgd_handle dsth, int64_t dst_off, pgd_handle srch, int64_t src_off, int64_t count) {
    PGD_CTX(c, h);
    Vec *dst = get_vec(c, dsth), *src = get_vec(c, srch);
    if (!dst || !src) return fail(c, PGD_ERR_INVALID, "vec_copy_range: invalid handles");
    if (count < 0 || dst_off < 0 || src_off < 0 || dst_off > dst->n - count || src_off > src->n - count)
        return fail(c, PGD_ERR_INVALID, "vec_copy_range: range outside the vectors");
    if (dst == src && dst_off < src_off + count && src_off < dst_off + count && count > 0)
        return fail(c, PGD_ERR_INVALID, "vec_copy_range: overlapping ranges of one vector");
    if (count == 0) return PGD_OK;
    k_copy_range<<<grid_for(count), TPB, 0, c->stream>>>(dst->d + dst_off, src->d + src_off, count);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // extern "C"
