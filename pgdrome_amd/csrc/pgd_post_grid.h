// What pgd_post.hip, pgd_postmany.hip and pgd_design.hip share: the tensor grid of the free coordinates (its offsets, the decoding of a
// sample, the coefficient and weight chains), the ordered minimum, the segments of the reductions and their ascending sum.  (The
// launcher, the instance table, the fragment order of a and the call skeleton are pgd_internal.h's: the products that know no grid
// use them too.)
#pragma once
#include "pgd_internal.h"

namespace pgd {

constexpr int PO_DMAX = 6;              // dimensions of the grid
constexpr int PO_NSEG = 1024;           // most segments of the reductions
constexpr int PO_SEGMIN = 4096;         // fewest samples of a segment (the last one excepted)
constexpr int PM_SEGMIN = 1024;         // .. of pgd_grid_posterior_many, whose work items are (segment) x (data block): a few data sets already fill the device

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

// the order of the minima: the smaller value, among equal ones the lower index (as a double: S < 2^31 is exact)
__device__ __forceinline__ bool post_less(double omn, double oix, double mn, double ix) { return omn < mn || (omn == mn && oix < ix); }

// the wave's (min, lowest index of it) from the lanes'
__device__ __forceinline__ void wave_min_index(double &mn, double &ix) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double omn = __shfl_xor(mn, m, 64), oix = __shfl_xor(ix, m, 64);
        if (post_less(omn, oix, mn, ix)) { mn = omn; ix = oix; }
    }
}

// out[i] = scale times the sum over the segments, ascending, of part[seg * stride + i], i < n
static __global__ __launch_bounds__(TPB) void k_seg_sum(const double *__restrict__ part, int nseg, int64_t stride, int64_t n, double scale,
                                                        double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    double t = 0.0;
    for (int seg = 0; seg < nseg; ++seg) t += part[(size_t)seg * stride + i];
    out[i] = scale * t;
}

inline int seg_sum(Ctx *c, const double *part, int nseg, int64_t stride, int64_t n, double scale, double *out) {
    return launch_grid(c, k_seg_sum, (n + TPB - 1) / TPB, TPB, 0, part, nseg, stride, n, scale, out);
}

// the segments of the reductions, of segmin samples or more (the last one excepted): a function of S alone
inline void grid_segments(int64_t S, int segmin, int *nseg, int64_t *seglen) {
    int64_t ns = (S + segmin - 1) / segmin;
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

}  // namespace pgd
