// What pgd_post.hip and pgd_postmany.hip share: the tensor grid of the free coordinates (its offsets, the decoding of a sample, the
// coefficient and weight chains), the segments of the reductions and the fragment order of a.
#pragma once
#include "pgd_internal.h"

namespace pgd {

constexpr int PO_DMAX = 6;              // dimensions of the grid
constexpr int PO_NSEG = 1024;           // most segments of the reductions
constexpr int PO_SEGMIN = 4096;         // fewest samples of a segment (the last one excepted)

typedef double po_d4 __attribute__((ext_vector_type(4)));

// the grid: n[d] points per dimension, table d at tab[toff[d] + t n[d] + i], weights and abscissae of dimension d from woff[d] on
struct PostDims {
    int ndim;
    int n[PO_DMAX];
    long long toff[PO_DMAX];
    long long woff[PO_DMAX];
    long long inner[PO_DMAX];           // prod_{e > d} n[e]
};

// (loops over d are unrolled over all six dimensions with the test d < ndim inside: the index arrays stay in registers)
__device__ __forceinline__ void post_decode(const PostDims &P, unsigned s, int (&i)[PO_DMAX]) {
    unsigned r = s;
#pragma unroll
    for (int d = PO_DMAX - 1; d >= 0; --d) {
        i[d] = 0;
        if (d < P.ndim) {
            const unsigned nd = (unsigned)P.n[d], q = r / nd;
            i[d] = (int)(r - q * nd);
            r = q;
        }
    }
}

__device__ __forceinline__ double post_coef(const PostDims &P, const double *__restrict__ tab, const int (&i)[PO_DMAX], int t) {
    double c = 1.0;
#pragma unroll
    for (int d = 0; d < PO_DMAX; ++d)
        if (d < P.ndim) c *= tab[P.toff[d] + (long long)t * P.n[d] + i[d]];
    return c;
}

__device__ __forceinline__ double post_weight(const PostDims &P, const double *__restrict__ wts, const int (&i)[PO_DMAX]) {
    double w = 1.0;
#pragma unroll
    for (int d = 0; d < PO_DMAX; ++d)
        if (d < P.ndim) w *= wts[P.woff[d] + i[d]];
    return w;
}

__device__ __forceinline__ double post_e(double chi2, double shift, double w) { return w * exp(-0.5 * (chi2 - shift)); }

// k-steps of 4 of the misfit instance for k modes; it holds T = 4, 4, 4, 4, 2, 1 sample tiles per wave (quad_kt)
inline int post_kt(int k) { return k <= 16 ? 4 : k <= 32 ? 8 : k <= 48 ? 12 : k <= 64 ? 16 : k <= 128 ? 32 : 64; }

// entry (p, t) of a in fragment order: kt k-steps of 4 per tile of 16 rows
inline size_t post_af_index(int kt, int p, int t) { return ((size_t)(p >> 4) * kt + (t >> 2)) * 64 + ((t & 3) << 4) + (p & 15); }

// the segments of the reductions: a function of S alone
inline void post_segments(int64_t S, int *nseg, int64_t *seglen) {
    int64_t ns = (S + PO_SEGMIN - 1) / PO_SEGMIN;
    if (ns > PO_NSEG) ns = PO_NSEG;
    if (ns < 1) ns = 1;
    int64_t len = (S + ns - 1) / ns;
    len = (len + 255) / 256 * 256;
    *nseg = (int)((S + len - 1) / len);
    if (*nseg < 1) *nseg = 1;
    *seglen = len;
}

// the grid and its offsets from (n, ndim, k); false: a size is out of range or S >= 2^31
inline bool post_dims(const int *n, int ndim, int k, PostDims *P, int64_t *S, int64_t *ntab, int64_t *nw) {
    P->ndim = ndim;
    int64_t s = 1, to = 0, wo = 0;
    for (int d = 0; d < PO_DMAX; ++d) { P->n[d] = 1; P->toff[d] = 0; P->woff[d] = 0; P->inner[d] = 1; }
    for (int d = 0; d < ndim; ++d) {
        if (n[d] < 1) return false;
        s *= n[d];
        if (s >= ((int64_t)1 << 31)) return false;
        P->n[d] = n[d];
        P->toff[d] = to;
        P->woff[d] = wo;
        to += (int64_t)k * n[d];
        wo += n[d];
    }
    for (int d = ndim - 2; d >= 0; --d) P->inner[d] = P->inner[d + 1] * n[d + 1];
    *S = s;
    *ntab = to;
    *nw = wo;
    return true;
}

inline size_t pool_bytes(size_t n_doubles) { return (n_doubles * sizeof(double) + 65535) & ~(size_t)65535; }   // (whole 64 KiB: the pool takes them back)

}  // namespace pgd
