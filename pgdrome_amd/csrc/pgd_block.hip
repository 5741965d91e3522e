// Column blocks: k <= 64 vectors of n rows in ONE allocation, stored as fp32 or f64, with the two tall-skinny products a
// projection onto their span needs - all k dots Y_j . r in one pass over the block, and x = base + Y c in one pass.  Both are
// pure streams whose cost is the bytes of Y (the spectral start space of pgdrome_amd/spectral.py: 48 columns of 256^3 rows, read
// twice per spatial solve), so Y is read 16 B per lane with non-temporal loads - every byte is used once per pass - while r
// and x keep the default policy.  Products and sums are f64 whatever the storage.
#include "pgd_internal.h"

#include <algorithm>

namespace pgd {

constexpr int BLOCK_MAXK = 64;
constexpr int DOTS_CPW = BLOCK_MAXK / 4;     // columns per wave of k_block_dots
constexpr int DOTS_GROUP = 8;                // ... taken this many at a time
constexpr int COMBINE_GROUP = 8;             // columns in flight per lane of k_block_combine

template <typename T> struct BlockVec;
template <> struct BlockVec<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int V = 4; };
template <> struct BlockVec<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int V = 2; };
typedef double d2_t __attribute__((ext_vector_type(2)));

template <typename T>
__global__ __launch_bounds__(TPB) void k_block_set(T *__restrict__ col, const double *__restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) col[i] = (T)v[i];   // round to nearest
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_block_get(const T *__restrict__ col, double *__restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) v[i] = (double)col[i];
}

// partials[b][j] = workgroup b's share of sum_{lo <= i < hi} Y_ij r_i.  A workgroup walks over tiles of 64 V rows (V = rows per
// 16 bytes); its four waves take the SAME rows and a quarter of the columns each, so a wave carries at most 16 accumulators, r
// comes from HBM once (the other three waves find it in the cache) and a column's sum never leaves its wave: no LDS, no barrier.
// Tiles are aligned to row 0, not to lo; the lanes across the ends of [lo, hi) go row by row.  Fixed order throughout.
template <typename T>
__global__ __launch_bounds__(TPB) void k_block_dots(const T *__restrict__ Y, int64_t stride, int k, const double *__restrict__ r,
                                                    int64_t lo, int64_t hi, int64_t tile0, int64_t tile1,
                                                    double *__restrict__ partials) {
    typedef typename BlockVec<T>::type vec_t;
    constexpr int V = BlockVec<T>::V;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = (k + 3) >> 2, j0 = wv * per;
    const int nc = (k - j0 < per) ? k - j0 : per;      // uniform per wave
    if (nc <= 0) return;
    const T *col0 = Y + (int64_t)j0 * stride;
    double acc[DOTS_CPW];
#pragma unroll
    for (int u = 0; u < DOTS_CPW; ++u) acc[u] = 0.0;
    for (int64_t t = tile0 + blockIdx.x; t < tile1; t += gridDim.x) {
        const int64_t i0 = (t * 64 + lane) * V;
        if (i0 >= lo && i0 + V <= hi) {
            double rv[V];
#pragma unroll
            for (int e = 0; e < V; e += 2) {
                const d2_t t2 = *reinterpret_cast<const d2_t *>(r + i0 + e);
                rv[e] = t2.x; rv[e + 1] = t2.y;
            }
#pragma unroll
            for (int h = 0; h < DOTS_CPW; h += DOTS_GROUP) {       // DOTS_GROUP loads in flight per lane
                vec_t y[DOTS_GROUP];
#pragma unroll
                for (int u = 0; u < DOTS_GROUP; ++u)
                    if (h + u < nc) y[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(col0 + (int64_t)(h + u) * stride + i0));
#pragma unroll
                for (int u = 0; u < DOTS_GROUP; ++u)
                    if (h + u < nc) {
#pragma unroll
                        for (int e = 0; e < V; ++e) acc[h + u] = fma((double)y[u][e], rv[e], acc[h + u]);
                    }
            }
        } else if (i0 < hi && i0 + V > lo) {
            for (int e = 0; e < V; ++e) {
                const int64_t i = i0 + e;
                if (i < lo || i >= hi) continue;
                const double ri = r[i];
#pragma unroll
                for (int u = 0; u < DOTS_CPW; ++u)
                    if (u < nc) acc[u] = fma((double)col0[(int64_t)u * stride + i], ri, acc[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < DOTS_CPW; ++u)
        if (u < nc) {
            const double s = wave_sum(acc[u]);
            if (lane == 0) partials[(int64_t)blockIdx.x * k + j0 + u] = s;
        }
}

struct BlockCoefs { double c[BLOCK_MAXK]; };

// x_i = base_i + sum_j c_j Y_ij as the chain s = base_i (0 without a base); s = fma(c_j, Y_ij, s) for j ascending - what
// k_lincomb computes for the terms [base, Y_0, ...] with coefficients [1, c_0, ...], since fma(1, base_i, 0) = base_i.  A lane
// reads its rows of base before it writes them to x: base may be x.
template <typename T>
__global__ __launch_bounds__(TPB) void k_block_combine(const T *__restrict__ Y, int64_t stride, int k, BlockCoefs C,
                                                       const double *base, double *x, int64_t n) {
    typedef typename BlockVec<T>::type vec_t;
    constexpr int V = BlockVec<T>::V;
    const int64_t ngroups = (n + V - 1) / V;
    for (int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * TPB) {
        const int64_t i0 = g * V;
        if (i0 + V <= n) {
            double s[V];
#pragma unroll
            for (int e = 0; e < V; e += 2) {
                d2_t t2; t2.x = 0.0; t2.y = 0.0;
                if (base) t2 = *reinterpret_cast<const d2_t *>(base + i0 + e);
                s[e] = t2.x; s[e + 1] = t2.y;
            }
            for (int j0 = 0; j0 < k; j0 += COMBINE_GROUP) {
                vec_t y[COMBINE_GROUP];
#pragma unroll
                for (int u = 0; u < COMBINE_GROUP; ++u)
                    if (j0 + u < k) y[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(Y + (int64_t)(j0 + u) * stride + i0));
#pragma unroll
                for (int u = 0; u < COMBINE_GROUP; ++u)
                    if (j0 + u < k) {
                        const double cj = C.c[j0 + u];
#pragma unroll
                        for (int e = 0; e < V; ++e) s[e] = fma(cj, (double)y[u][e], s[e]);
                    }
            }
#pragma unroll
            for (int e = 0; e < V; e += 2) {
                d2_t t2; t2.x = s[e]; t2.y = s[e + 1];
                *reinterpret_cast<d2_t *>(x + i0 + e) = t2;
            }
        } else {
            for (int64_t i = i0; i < n; ++i) {
                double s = base ? base[i] : 0.0;
                for (int j = 0; j < k; ++j) s = fma(C.c[j], (double)Y[(int64_t)j * stride + i], s);
                x[i] = s;
            }
        }
    }
}

static int block_col_check(Ctx *c, const Block *b, int j, const Vec *v, const char *who) {
    if (!b || !v || j < 0 || j >= b->k || v->n != b->n) return fail(c, PGD_ERR_INVALID, "%s: invalid handles, column out of range or size mismatch", who);
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_block_storage(pgd_handle h, int *dtype) {
    PGD_CTX(c, h);
    if (!dtype) return fail(c, PGD_ERR_INVALID, "block_storage: bad arguments");
    *dtype = c->block_storage == 1 ? PGD_BLOCK_F32 : c->block_storage == 2 ? PGD_BLOCK_F64 : -1;
    return PGD_OK;
}

int pgd_block_create(pgd_handle h, int64_t n, int k, int dtype, pgd_handle *out) {
    PGD_CTX(c, h);
    if (!out || n < 1 || k < 1 || k > BLOCK_MAXK || (dtype != PGD_BLOCK_F32 && dtype != PGD_BLOCK_F64))
        return fail(c, PGD_ERR_INVALID, "block_create: bad arguments (1 <= k <= %d, dtype PGD_BLOCK_F32 or PGD_BLOCK_F64)", BLOCK_MAXK);
    std::unique_ptr<Block> b(new Block);
    b->kind = Obj::BLOCK;
    b->n = n; b->k = k; b->dtype = dtype;
    // every column starts on a 256-byte boundary (16-byte loads at any multiple of V rows) and ends with the slack of every device array
    b->stride = (n + 255) / 256 * 256 + (int64_t)PAD_BYTES / 4;
    b->bytes = (size_t)k * (size_t)b->stride * (dtype == PGD_BLOCK_F32 ? sizeof(float) : sizeof(double));
    void *p;
    PGD_TRY(dev_alloc(c, &p, b->bytes));
    b->d = p;
    b->ctx = c;
    PGD_HIP(c, hipMemsetAsync(p, 0, b->bytes, c->stream));
    *out = put_obj(c, b.release());
    return PGD_OK;
}

int pgd_block_free(pgd_handle h, pgd_handle bh) {
    PGD_CTX(c, h);
    return free_obj(c, bh, Obj::BLOCK);
}

int pgd_block_info(pgd_handle h, pgd_handle bh, int64_t *n, int *k, int *dtype, int64_t *bytes) {
    PGD_CTX(c, h);
    Block *b = get_block(c, bh);
    if (!b) return fail(c, PGD_ERR_INVALID, "block_info: invalid handle");
    if (n) *n = b->n;
    if (k) *k = b->k;
    if (dtype) *dtype = b->dtype;
    if (bytes) *bytes = (int64_t)b->bytes;
    return PGD_OK;
}

int pgd_block_set_column(pgd_handle h, pgd_handle bh, int j, pgd_handle vh) {
    PGD_CTX(c, h);
    Block *b = get_block(c, bh);
    Vec *v = get_vec(c, vh);
    PGD_TRY(block_col_check(c, b, j, v, "block_set_column"));
    const int g = grid_for(b->n);
    if (b->dtype == PGD_BLOCK_F32) k_block_set<float><<<g, TPB, 0, c->stream>>>((float *)b->d + (int64_t)j * b->stride, v->d, b->n);
    else k_block_set<double><<<g, TPB, 0, c->stream>>>((double *)b->d + (int64_t)j * b->stride, v->d, b->n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

int pgd_block_get_column(pgd_handle h, pgd_handle bh, int j, pgd_handle vh) {
    PGD_CTX(c, h);
    Block *b = get_block(c, bh);
    Vec *v = get_vec(c, vh);
    PGD_TRY(block_col_check(c, b, j, v, "block_get_column"));
    const int g = grid_for(b->n);
    if (b->dtype == PGD_BLOCK_F32) k_block_get<float><<<g, TPB, 0, c->stream>>>((const float *)b->d + (int64_t)j * b->stride, v->d, b->n);
    else k_block_get<double><<<g, TPB, 0, c->stream>>>((const double *)b->d + (int64_t)j * b->stride, v->d, b->n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

int pgd_block_dots(pgd_handle h, pgd_handle bh, pgd_handle rh, int64_t lo, int64_t hi, double *out) {
    PGD_CTX(c, h);
    Block *b = get_block(c, bh);
    Vec *r = get_vec(c, rh);
    if (!b || !r || !out || r->n != b->n) return fail(c, PGD_ERR_INVALID, "block_dots: invalid handles or size mismatch");
    if (hi < 0) hi = b->n;
    if (lo < 0 || lo > hi || hi > b->n) return fail(c, PGD_ERR_INVALID, "block_dots: bad range");
    for (int j = 0; j < b->k; ++j) out[j] = 0.0;
    if (hi == lo) return PGD_OK;
    const int64_t tile = 64 * (b->dtype == PGD_BLOCK_F32 ? 4 : 2);
    const int64_t tile0 = lo / tile, tile1 = (hi + tile - 1) / tile;
    const int g = (int)std::min<int64_t>(tile1 - tile0, MAX_VEC_BLOCKS);
    PGD_TRY(ensure_work(c, 6, BLOCK_MAXK));
    PGD_TRY(ensure_partials(c, std::max<int64_t>((int64_t)g * b->k, 4 * MAX_VEC_BLOCKS)));
    if (b->dtype == PGD_BLOCK_F32) k_block_dots<float><<<g, TPB, 0, c->stream>>>((const float *)b->d, b->stride, b->k, r->d, lo, hi, tile0, tile1, c->partials);
    else k_block_dots<double><<<g, TPB, 0, c->stream>>>((const double *)b->d, b->stride, b->k, r->d, lo, hi, tile0, tile1, c->partials);
    PGD_LAUNCH_CHECK(c);
    PGD_TRY(reduce_partials_to(c, c->partials, g, b->k, c->work[6], b->k));
    PGD_HIP(c, hipMemcpyAsync(out, c->work[6], (size_t)b->k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PGD_HIP(c, hipStreamSynchronize(c->stream));
    return PGD_OK;
}

int pgd_block_combine(pgd_handle h, pgd_handle bh, const double *coefs, pgd_handle baseh, pgd_handle xh) {
    PGD_CTX(c, h);
    Block *b = get_block(c, bh);
    Vec *x = get_vec(c, xh), *base = baseh ? get_vec(c, baseh) : nullptr;
    if (!b || !x || !coefs || x->n != b->n || (baseh && (!base || base->n != b->n)))
        return fail(c, PGD_ERR_INVALID, "block_combine: invalid handles or size mismatch");
    BlockCoefs C;
    for (int j = 0; j < BLOCK_MAXK; ++j) C.c[j] = j < b->k ? coefs[j] : 0.0;
    const int V = b->dtype == PGD_BLOCK_F32 ? 4 : 2;
    const int g = grid_for((b->n + V - 1) / V);
    if (b->dtype == PGD_BLOCK_F32) k_block_combine<float><<<g, TPB, 0, c->stream>>>((const float *)b->d, b->stride, b->k, C, base ? base->d : nullptr, x->d, b->n);
    else k_block_combine<double><<<g, TPB, 0, c->stream>>>((const double *)b->d, b->stride, b->k, C, base ? base->d : nullptr, x->d, b->n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // extern "C"
