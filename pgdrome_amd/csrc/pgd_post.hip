// Bayesian calibration on a tensor grid of the free coordinates: the misfits of ALL grid points as one dense product whose right-hand
// factor is never stored, and the reductions of the posterior over them.
//
// The sample s = (i_0 .. i_{D-1}), last index fastest, has the mode coefficients c_k(s) = 1 * T_0[k, i_0] * T_1[k, i_1] * .. (one
// chain in ascending d: the bits of model.py's mode_factors_many on the same tables); the tables are D small k x n[d] arrays.
//
// pgd_grid_misfit: chi2[s] = sum_p (y_p - sum_k a_pk c_k(s))^2, the fourth dense product of this library on v_mfma_f64_16x16x4_f64,
// in the orientation of k_eval_mfma / k_quad_mfma:
//   * B is the fragment of the coefficients of a tile of 16 samples (samples on the fragment's column index): lane (lq, lr) =
//     (lane >> 4, lane & 15) holds c_{4 q + lq}(sample 16 j + lr) in b[j][q], formed from the tables where it is needed (a lane decodes
//     its sample once per tile), zero beyond k.  A wave owns T tiles at a time; nothing is shared between waves: no LDS, no barrier.
//   * A holds 16 rows p of a: lane (lq, lr) holds a[16 mt + lr][4 q + lq]; the host lays a out in that fragment order, zero padded.
//   * D[p][s]: the lane holds D[16 mt + 4 r + lq][lr] in acc[r]; the residual y_p - D enters chi2 as one fma chain in ascending
//     (mt, r), then two __shfl_xor (16, 32) over lq - both sums of a xor step have the same two operands, all four lq hold the same bits.
//   * the minimum and its lowest index: per lane, per wave, then k_misfit_finish; neither depends on order.
// k_misfit_plain: the same from ordinary ascending fma chains, a lane per sample (PGD_TUNE_MISFIT_VARIANT = 0).
//
// pgd_grid_posterior: e_s = w_s exp(-(chi2[s] - shift) / 2), w_s = 1 * weights_0[i_0] * weights_1[i_1] * ..  No floating-point atomics:
//   * S is cut into nseg <= 1024 segments of seglen samples (grid_segments: a function of S alone); a workgroup forms the partial sums
//     of a segment in an order that depends on the segment alone, k_seg_sum adds the segments in ascending order.
//   * Z, sum e^2 and the parameter moments: k_post_sums, one accumulator set per thread.
//   * sum e c and sum e c c^T (k <= 64): k_post_coef_mfma.  The contraction runs over the SAMPLES, four per instruction: A = e c_i(s),
//     B = c_j(s), lane (lq, lr) holds mode 16 it + lr at sample s0 + lq.  A lane forms e for one sample of a batch of 64 and the lanes
//     fetch the batch's e and indices by __shfl; the wave's tiles (it <= jt) stay in registers over its batches; the four waves of a
//     workgroup are added in ascending order through LDS.  The host mirrors the upper triangle.  k_post_coef_plain: fma chains.
//   * the marginals: a workgroup per entry (d, i) runs over the S / n[d] samples with i_d = i in a fixed order - no partials at all.
// Every output is bit-identical from run to run and for any grid (PGD_TUNE_POST_GRID_MAX, PGD_TUNE_MISFIT_GRID_MAX).
#include "pgd_post_grid.h"

#include <cmath>
#include <vector>

namespace pgd {

constexpr int PO_KMAX = 256;            // modes per call of pgd_grid_misfit (QD_KMAX)
constexpr int PO_MMAX = 256;            // rows of a
constexpr int PO_COEF_KMAX = 64;        // modes of PGD_POST_COEF: 10 tiles of 16 x 16 per wave
constexpr int PO_NV = 32;               // Z, sum e^2, 6 first and 21 second parameter moments, padded
constexpr int PO_PLAIN_TPB = 64;        // k_misfit_plain: one wave per workgroup, one sample per lane
constexpr int PO_PLAIN_ACC = 17;        // k_post_coef_plain: (64 * 64 + 64) / 256 entries per thread, rounded up

// KT: k-steps of 4 the kernel is compiled for (4 KT >= k); T: sample tiles a wave holds at a time; mtn: tiles of 16 rows of a
template <int KT, int T>
__global__ __launch_bounds__(TPB) void k_misfit_mfma(PostDims P, const double *__restrict__ tab, int k, int mtn, const double *__restrict__ af,
                                                     const double *__restrict__ yp, int64_t S, double *__restrict__ chi2, double *__restrict__ part) {
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    double bmn = INF, bix = INF;
    const int64_t ntile = (S + 16 * T - 1) / (16 * T);
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        double b[T][KT];
        int64_t smp[T];
        bool sv[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            smp[j] = tile * (16 * T) + 16 * j + lr;
            sv[j] = smp[j] < S;
            int idx[PO_DMAX];
            post_decode(P, (unsigned)(sv[j] ? smp[j] : S - 1), idx);      // (a sample beyond S repeats the last one: its value is not stored)
            // post_coef for the lane's KT modes, a dimension at a time (the same chain per mode; at most 16 loads in flight)
#pragma unroll
            for (int q = 0; q < KT; ++q) b[j][q] = 1.0;
#pragma unroll
            for (int d = 0; d < PO_DMAX; ++d) {
                if (d < P.ndim) {
                    const double *tp = tab + P.toff[d] + idx[d] + (long long)lq * P.n[d];
#pragma unroll
                    for (int q = 0; q < KT; ++q) {
                        b[j][q] *= 4 * q + lq < k ? tp[(long long)(4 * q) * P.n[d]] : 0.0;
                        if ((q & 15) == 15) __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
        double v[T];
#pragma unroll
        for (int j = 0; j < T; ++j) v[j] = 0.0;
        for (int mt = 0; mt < mtn; ++mt) {
            d4_t acc[T];
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = d4_t{0.0, 0.0, 0.0, 0.0};
            const double *ap = af + (size_t)mt * KT * 64 + lane;
#pragma unroll
            for (int q = 0; q < KT; ++q) {
                const double a = ap[q * 64];
#pragma unroll
                for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j][q], acc[j], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double yv = yp[16 * mt + 4 * r + lq];
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const double res = yv - acc[j][r];
                    v[j] = fma(res, res, v[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            v[j] += __shfl_xor(v[j], 16, 64);
            v[j] += __shfl_xor(v[j], 32, 64);
            if (sv[j]) {
                if (lq == 0) chi2[smp[j]] = v[j];
                const double ix = (double)smp[j];
                if (post_less(v[j], ix, bmn, bix)) { bmn = v[j]; bix = ix; }
            }
        }
    }
    wave_min_index(bmn, bix);
    if (lane == 0) {
        const int64_t w = (int64_t)blockIdx.x * 4 + wv;
        part[2 * w] = bmn;
        part[2 * w + 1] = bix;
    }
}

// The same from ordinary fma chains; a: m x k row-major as the caller passed it; the k coefficients of the lane's sample in its own
// column of LDS (no lane reads another's: no barrier)
__global__ __launch_bounds__(PO_PLAIN_TPB) void k_misfit_plain(PostDims P, const double *__restrict__ tab, int k, int m, const double *__restrict__ a,
                                                               const double *__restrict__ y, int64_t S, double *__restrict__ chi2,
                                                               double *__restrict__ part) {
    extern __shared__ double s_c[];
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x;
    double bmn = INF, bix = INF;
    const int64_t nblk = (S + PO_PLAIN_TPB - 1) / PO_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t s = blk * PO_PLAIN_TPB + lane;
        const bool sv = s < S;
        int idx[PO_DMAX];
        post_decode(P, (unsigned)(sv ? s : S - 1), idx);
        for (int t = 0; t < k; ++t) s_c[t * PO_PLAIN_TPB + lane] = post_coef(P, tab, idx, t);
        double v = 0.0;
        for (int p = 0; p < m; ++p) {
            const double *arow = a + (size_t)p * k;
            double t = 0.0;
            for (int kk = 0; kk < k; ++kk) t = fma(arow[kk], s_c[kk * PO_PLAIN_TPB + lane], t);
            const double res = y[p] - t;
            v = fma(res, res, v);
        }
        if (sv) {
            chi2[s] = v;
            const double ix = (double)s;
            if (post_less(v, ix, bmn, bix)) { bmn = v; bix = ix; }
        }
    }
    wave_min_index(bmn, bix);
    if (lane == 0) {
        part[2 * (int64_t)blockIdx.x] = bmn;
        part[2 * (int64_t)blockIdx.x + 1] = bix;
    }
}

// one workgroup: out[0] = min over the nrows partial rows, out[1] = the lowest index among the rows that hold it
__global__ __launch_bounds__(TPB) void k_misfit_finish(const double *__restrict__ part, int64_t nrows, double *__restrict__ out) {
    __shared__ double s_mn[TPB], s_ix[TPB];
    const int tid = threadIdx.x;
    double mn = __builtin_huge_val(), ix = __builtin_huge_val();
    for (int64_t w = tid; w < nrows; w += TPB) {
        const double omn = part[2 * w], oix = part[2 * w + 1];
        if (post_less(omn, oix, mn, ix)) { mn = omn; ix = oix; }
    }
    s_mn[tid] = mn;
    s_ix[tid] = ix;
    __syncthreads();
    for (int h = TPB / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double omn = s_mn[tid + h], oix = s_ix[tid + h];
            if (post_less(omn, oix, s_mn[tid], s_ix[tid])) { s_mn[tid] = omn; s_ix[tid] = oix; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = s_mn[0];
        out[1] = s_ix[0];
    }
}

// ---- the reductions of the posterior
// part[seg * PO_NV + ..]: 0 Z, 1 sum e^2, 2 + d: sum e th_d, 8 + pair(d, f): sum e th_d th_f for d <= f in row order of the upper triangle
__global__ __launch_bounds__(TPB) void k_post_sums(PostDims P, const double *__restrict__ chi2, double shift, const double *__restrict__ wts,
                                                   const double *__restrict__ absc, int64_t S, int nseg, int64_t seglen, int theta,
                                                   double *__restrict__ part) {
    __shared__ double s_red[4];
    const int tid = threadIdx.x;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        double acc[PO_NV];
#pragma unroll
        for (int v = 0; v < PO_NV; ++v) acc[v] = 0.0;
        for (int64_t s = lo + tid; s < hi; s += TPB) {
            int idx[PO_DMAX];
            post_decode(P, (unsigned)s, idx);
            const double e = post_e(chi2[s], shift, post_weight(P, wts, idx));
            acc[0] += e;
            acc[1] = fma(e, e, acc[1]);
            if (theta) {
                double th[PO_DMAX];
#pragma unroll
                for (int d = 0; d < PO_DMAX; ++d) th[d] = d < P.ndim ? absc[P.woff[d] + idx[d]] : 0.0;
                int pr = 8;
#pragma unroll
                for (int d = 0; d < PO_DMAX; ++d) {
                    acc[2 + d] = fma(e, th[d], acc[2 + d]);
                    const double et = e * th[d];
#pragma unroll
                    for (int f = d; f < PO_DMAX; ++f, ++pr) acc[pr] = fma(et, th[f], acc[pr]);
                }
            }
        }
        const int nv = theta ? 29 : 2;
#pragma unroll
        for (int v = 0; v < PO_NV; ++v) {
            if (v < nv) {
                const double t = block_sum(acc[v], s_red);
                if (tid == 0) part[(size_t)seg * PO_NV + v] = t;
            }
        }
    }
}

// a workgroup per entry of the marginals: the sum of e over the samples with i_d = i, thread t takes the samples t, t + 256, .. of them
__global__ __launch_bounds__(TPB) void k_post_marginals(PostDims P, const double *__restrict__ chi2, double shift, const double *__restrict__ wts,
                                                        int64_t S, int64_t nent, double *__restrict__ out) {
    __shared__ double s_red[4];
    const int tid = threadIdx.x;
    for (int64_t ent = blockIdx.x; ent < nent; ent += gridDim.x) {
        unsigned nd = 1, i = 0, inner = 1;
#pragma unroll
        for (int d = 0; d < PO_DMAX; ++d)
            if (d < P.ndim && ent >= P.woff[d] && ent < P.woff[d] + P.n[d]) {
                nd = (unsigned)P.n[d];
                i = (unsigned)(ent - P.woff[d]);
                inner = (unsigned)P.inner[d];
            }
        const unsigned cnt = (unsigned)(S / nd);
        double acc = 0.0;
        for (unsigned r = tid; r < cnt; r += TPB) {
            const unsigned h = r / inner, l = r - h * inner;
            const unsigned s = (h * nd + i) * inner + l;
            int idx[PO_DMAX];
            post_decode(P, s, idx);
            acc += post_e(chi2[s], shift, post_weight(P, wts, idx));
        }
        const double t = block_sum(acc, s_red);
        if (tid == 0) out[ent] = t;
    }
}

// KB: tiles of 16 modes (16 KB >= k); part[seg * stride + i * 16 KB + j] = the segment's sum e c_i c_j for the tiles it <= jt (zeros in
// the others), part[seg * stride + (16 KB)^2 + i] = its sum e c_i
template <int KB>
__global__ __launch_bounds__(TPB) void k_post_coef_mfma(PostDims P, const double *__restrict__ tab, int k, const double *__restrict__ chi2,
                                                        double shift, const double *__restrict__ wts, int64_t S, int nseg, int64_t seglen,
                                                        int64_t stride, double *__restrict__ part) {
    constexpr int NT = KB * (KB + 1) / 2, KP = 16 * KB;
    __shared__ double s_acc[NT * 4 * 64 + KP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        const int64_t nbatch = (hi - lo + 63) / 64;
        d4_t acc[NT];
        double m1[KB];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int it = 0; it < KB; ++it) m1[it] = 0.0;
        for (int64_t bt = wv; bt < nbatch; bt += 4) {
            const int64_t s = lo + 64 * bt + lane;
            const bool sv = s < hi;
            int idx[PO_DMAX];
            post_decode(P, (unsigned)(sv ? s : hi - 1), idx);
            const double e_own = sv ? post_e(chi2[s], shift, post_weight(P, wts, idx)) : 0.0;
            for (int g = 0; g < 16; ++g) {
                const int src = 4 * g + lq;
                const double eg = __shfl(e_own, src, 64);
                int ig[PO_DMAX];
#pragma unroll
                for (int d = 0; d < PO_DMAX; ++d) ig[d] = d < P.ndim ? __shfl(idx[d], src, 64) : 0;
                double cv[KB], av[KB];
#pragma unroll
                for (int it = 0; it < KB; ++it) {
                    const int t = 16 * it + lr;
                    cv[it] = t < k ? post_coef(P, tab, ig, t) : 0.0;
                    av[it] = eg * cv[it];
                    m1[it] += av[it];
                }
                int u = 0;
#pragma unroll
                for (int it = 0; it < KB; ++it) {
#pragma unroll
                    for (int jt = it; jt < KB; ++jt, ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[it], cv[jt], acc[u], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < KB; ++it) {
            m1[it] += __shfl_xor(m1[it], 16, 64);
            m1[it] += __shfl_xor(m1[it], 32, 64);
        }
        // the waves 1, 2, 3 in turn through LDS, added by wave 0 in that order
        for (int w = 1; w < 4; ++w) {
            __syncthreads();
            if (wv == w) {
#pragma unroll
                for (int u = 0; u < NT; ++u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_acc[(u * 4 + r) * 64 + lane] = acc[u][r];
                }
                if (lq == 0) {
#pragma unroll
                    for (int it = 0; it < KB; ++it) s_acc[NT * 256 + 16 * it + lr] = m1[it];
                }
            }
            __syncthreads();
            if (wv == 0) {
#pragma unroll
                for (int u = 0; u < NT; ++u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[u][r] += s_acc[(u * 4 + r) * 64 + lane];
                }
#pragma unroll
                for (int it = 0; it < KB; ++it) m1[it] += s_acc[NT * 256 + 16 * it + lr];
            }
        }
        if (wv == 0) {
            double *o = part + (size_t)seg * stride;
            int u = 0;
#pragma unroll
            for (int it = 0; it < KB; ++it) {
#pragma unroll
                for (int jt = 0; jt < KB; ++jt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[(size_t)(16 * it + 4 * r + lq) * KP + 16 * jt + lr] = jt >= it ? acc[jt >= it ? u : 0][r] : 0.0;
                    if (jt >= it) ++u;
                }
            }
            if (lq == 0) {
#pragma unroll
                for (int it = 0; it < KB; ++it) o[(size_t)KP * KP + 16 * it + lr] = m1[it];
            }
        }
        __syncthreads();
    }
}

// The same partials (entries i <= j and the first moments; the rest of a segment's row is zeroed by the launcher) from fma chains over the
// segment's samples in ascending order: batches of 64 samples, their e and coefficients in LDS, thread t the entries t, t + 256, ..
__global__ __launch_bounds__(TPB) void k_post_coef_plain(PostDims P, const double *__restrict__ tab, int k, int kp, const double *__restrict__ chi2,
                                                         double shift, const double *__restrict__ wts, int64_t S, int nseg, int64_t seglen,
                                                         int64_t stride, double *__restrict__ part) {
    extern __shared__ double s_pl[];            // e of the 64 samples, then k rows of 64 coefficients
    double *s_e = s_pl, *s_c = s_pl + 64;
    const int tid = threadIdx.x, l = tid & 63;
    const int nent = k * k + k;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        double acc[PO_PLAIN_ACC];
#pragma unroll
        for (int u = 0; u < PO_PLAIN_ACC; ++u) acc[u] = 0.0;
        for (int64_t b0 = lo; b0 < hi; b0 += 64) {
            const int64_t s = b0 + l;
            const bool sv = s < hi;
            int idx[PO_DMAX];
            post_decode(P, (unsigned)(sv ? s : hi - 1), idx);
            __syncthreads();
            if (tid < 64) s_e[l] = sv ? post_e(chi2[s], shift, post_weight(P, wts, idx)) : 0.0;
            for (int t = tid >> 6; t < k; t += 4) s_c[t * 64 + l] = post_coef(P, tab, idx, t);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PO_PLAIN_ACC; ++u) {
                const int ent = tid + TPB * u;
                if (ent < k * k) {
                    const int i = ent / k, j = ent - i * k;
                    if (i <= j)
                        for (int x = 0; x < 64; ++x) acc[u] = fma(s_e[x] * s_c[i * 64 + x], s_c[j * 64 + x], acc[u]);
                } else if (ent < nent) {
                    const int t = ent - k * k;
                    for (int x = 0; x < 64; ++x) acc[u] += s_e[x] * s_c[t * 64 + x];
                }
            }
        }
        double *o = part + (size_t)seg * stride;
#pragma unroll
        for (int u = 0; u < PO_PLAIN_ACC; ++u) {
            const int ent = tid + TPB * u;
            if (ent < k * k) {
                const int i = ent / k, j = ent - i * k;
                if (i <= j) o[(size_t)i * kp + j] = acc[u];
            } else if (ent < nent) {
                o[(size_t)kp * kp + ent - k * k] = acc[u];
            }
        }
    }
}


// (a wave of the persistent grid leaves one row of partials: they are sized once the grid is known)
template <int KT, int T>
static int misfit_launch_mfma(Ctx *c, const PostDims &P, const double *tab, int k, int mtn, const double *af, const double *yp, int64_t S,
                              double *chi2, int64_t *nrows) {
    const int64_t ntile = (S + 16 * T - 1) / (16 * T);
    const int64_t g = persistent_grid(c, k_misfit_mfma<KT, T>, TPB, 0, (ntile + 3) / 4, c->misfit_grid_max);
    PGD_TRY(ensure_partials(c, g * 4 * 2));
    *nrows = g * 4;
    return launch_grid(c, k_misfit_mfma<KT, T>, g, TPB, 0, P, tab, k, mtn, af, yp, S, chi2, c->partials);
}

static int misfit_launch_plain(Ctx *c, const PostDims &P, const double *tab, int k, int m, const double *a, const double *y, int64_t S,
                               double *chi2, int64_t *nrows) {
    const size_t lds = (size_t)k * PO_PLAIN_TPB * sizeof(double);
    PGD_TRY(raise_lds(c, (const void *)k_misfit_plain, lds, "grid_misfit"));
    const int64_t g = persistent_grid(c, k_misfit_plain, PO_PLAIN_TPB, lds, (S + PO_PLAIN_TPB - 1) / PO_PLAIN_TPB, c->misfit_grid_max, 8);
    PGD_TRY(ensure_partials(c, g * 2));
    *nrows = g;
    return launch_grid(c, k_misfit_plain, g, PO_PLAIN_TPB, lds, P, tab, k, m, a, y, S, chi2, c->partials);
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_grid_misfit(pgd_handle h, const double *a, const double *y, int m, int k, const double *tables, const int *n, int ndim,
                    pgd_handle chi2h, double *min_out, int64_t *argmin_out) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (k < 1 || k > PO_KMAX) return fail(c, PGD_ERR_INVALID, "grid_misfit: k = %d modes, 1 .. %d are possible", k, PO_KMAX);
    if (m < 1 || m > PO_MMAX) return fail(c, PGD_ERR_INVALID, "grid_misfit: m = %d rows, 1 .. %d are possible", m, PO_MMAX);
    if (ndim < 1 || ndim > PO_DMAX) return fail(c, PGD_ERR_INVALID, "grid_misfit: ndim = %d, 1 .. %d are possible", ndim, PO_DMAX);
    if (!a || !y || !tables || !n) return fail(c, PGD_ERR_INVALID, "grid_misfit: a, y, tables or n missing");
    PostDims P;
    int64_t S = 0, ntab = 0, nw = 0;
    if (!post_dims(n, ndim, k, &P, &S, &ntab, &nw))
        return fail(c, PGD_ERR_INVALID, "grid_misfit: a dimension without points, or 2^31 samples or more");
    Vec *cv = get_vec(c, chi2h);
    if (!cv) return fail(c, PGD_ERR_INVALID, "grid_misfit: chi2 is not a vector");
    if (cv->n != S) return fail(c, PGD_ERR_INVALID, "grid_misfit: chi2 has %lld entries, the grid has %lld samples", (long long)cv->n, (long long)S);

    // ---- a and y in the order the variant reads them, behind the tables in one upload
    const bool mfma = c->misfit_variant != 0;
    const int kt = dense_kt(k), mtn = (m + 15) / 16;
    const size_t na = mfma ? (size_t)mtn * kt * 64 : (size_t)m * k, ny = mfma ? (size_t)16 * mtn : (size_t)m;
    std::vector<double> hbuf(na + ny, 0.0);                 // (the tables go up from the caller's array: no host copy of them)
    double *ha = hbuf.data(), *hy = ha + na;
    if (mfma) pack_a_fragments(ha, kt, a, m, k, k);
    else std::copy(a, a + (size_t)m * k, ha);
    std::copy(y, y + m, hy);
    double res[2] = {0.0, 0.0};
    const int rc = with_pool_input(c, pool_bytes((size_t)ntab + hbuf.size()), [&](void *p_in) -> int {
        PGD_TRY(ensure_work(c, 6, 2));
        PGD_HIP(c, hipMemcpyAsync(p_in, tables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync((double *)p_in + ntab, hbuf.data(), hbuf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        const double *tab = (const double *)p_in, *ad = tab + ntab, *yd = ad + na;
        int64_t nrows = 0;
        if (mfma) {
            PGD_TRY(dense_dispatch(kt, [&](auto KT, auto T) {
                return misfit_launch_mfma<decltype(KT)::value, decltype(T)::value>(c, P, tab, k, mtn, ad, yd, S, cv->d, &nrows);
            }));
        } else {
            PGD_TRY(misfit_launch_plain(c, P, tab, k, m, ad, yd, S, cv->d, &nrows));
        }
        k_misfit_finish<<<1, TPB, 0, c->stream>>>(c->partials, nrows, c->work[6]);
        PGD_LAUNCH_CHECK(c);
        PGD_HIP(c, hipMemcpyAsync(res, c->work[6], 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the call
        return PGD_OK;
    });
    if (rc != PGD_OK) return rc;
    if (min_out) *min_out = res[0];
    if (argmin_out) *argmin_out = res[1] < 2147483648.0 ? (int64_t)res[1] : -1;   // (-1: no value compares, every chi2 is NaN)
    return PGD_OK;
}

int pgd_grid_posterior(pgd_handle h, pgd_handle chi2h, double shift, const double *tables, const int *n, int ndim, int k,
                       const double *weights, const double *abscissae, int want, double *sums, double *marginals, double *theta1,
                       double *theta2, double *coef1, double *coef2) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    const int known = PGD_POST_MARGINALS | PGD_POST_THETA | PGD_POST_COEF;
    if (want & ~known) return fail(c, PGD_ERR_INVALID, "grid_posterior: want = %d holds unknown bits", want);
    if (ndim < 1 || ndim > PO_DMAX) return fail(c, PGD_ERR_INVALID, "grid_posterior: ndim = %d, 1 .. %d are possible", ndim, PO_DMAX);
    if (!n || !weights || !sums) return fail(c, PGD_ERR_INVALID, "grid_posterior: n, weights or sums missing");
    if (!std::isfinite(shift)) return fail(c, PGD_ERR_INVALID, "grid_posterior: the shift is not finite");
    const bool coef = (want & PGD_POST_COEF) != 0, theta = (want & PGD_POST_THETA) != 0, marg = (want & PGD_POST_MARGINALS) != 0;
    if (coef && (k < 1 || k > PO_COEF_KMAX))
        return fail(c, PGD_ERR_INVALID, "grid_posterior: k = %d modes, PGD_POST_COEF takes 1 .. %d", k, PO_COEF_KMAX);
    if (coef && (!tables || !coef1 || !coef2)) return fail(c, PGD_ERR_INVALID, "grid_posterior: PGD_POST_COEF without tables, coef1 or coef2");
    if (theta && (!abscissae || !theta1 || !theta2)) return fail(c, PGD_ERR_INVALID, "grid_posterior: PGD_POST_THETA without abscissae, theta1 or theta2");
    if (marg && !marginals) return fail(c, PGD_ERR_INVALID, "grid_posterior: PGD_POST_MARGINALS without marginals");
    const int kk = coef ? k : 0;
    PostDims P;
    int64_t S = 0, ntab = 0, nw = 0;
    if (!post_dims(n, ndim, kk, &P, &S, &ntab, &nw))
        return fail(c, PGD_ERR_INVALID, "grid_posterior: a dimension without points, or 2^31 samples or more");
    Vec *cv = get_vec(c, chi2h);
    if (!cv) return fail(c, PGD_ERR_INVALID, "grid_posterior: chi2 is not a vector");
    if (cv->n != S) return fail(c, PGD_ERR_INVALID, "grid_posterior: chi2 has %lld entries, the grid has %lld samples", (long long)cv->n, (long long)S);

    int nseg = 1;
    int64_t seglen = 0;
    grid_segments(S, PO_SEGMIN, &nseg, &seglen);
    const int kb = (kk + 15) / 16, kp = 16 * kb, ncoef = kp * kp + kp;
    // the outputs on the device: sums and moments (PO_NV), coefficient moments (ncoef), marginals (nw)
    const int64_t nout = PO_NV + ncoef + (marg ? nw : 0);
    const int64_t npart = (int64_t)nseg * (PO_NV + ncoef);
    std::vector<double> out((size_t)nout, 0.0);
    // uploads from the caller's arrays: tables (PGD_POST_COEF), weights, abscissae (PGD_POST_THETA)
    const int rc = with_pool_input(c, pool_bytes((size_t)ntab + 2 * (size_t)nw), [&](void *p_in) -> int {
        PGD_TRY(ensure_work(c, 6, nout));
        PGD_TRY(ensure_partials(c, npart));
        double *tab = (double *)p_in, *wd = tab + ntab, *xd = wd + nw;
        if (coef) PGD_HIP(c, hipMemcpyAsync(tab, tables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(wd, weights, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (theta) PGD_HIP(c, hipMemcpyAsync(xd, abscissae, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        double *part_s = c->partials, *part_c = c->partials + (size_t)nseg * PO_NV, *od = c->work[6];
        int64_t cap = (int64_t)c->num_cu * 4;
        if (c->post_grid_max > 0 && cap > c->post_grid_max) cap = c->post_grid_max;
        const int g = (int)(nseg < cap ? nseg : cap);
        k_post_sums<<<g, TPB, 0, c->stream>>>(P, cv->d, shift, wd, xd, S, nseg, seglen, theta ? 1 : 0, part_s);
        PGD_LAUNCH_CHECK(c);
        PGD_TRY(seg_sum(c, part_s, nseg, PO_NV, theta ? 29 : 2, 1.0, od));
        if (coef) {
            if (c->post_variant != 0) {
                switch (kb) {
                    case 1: PGD_TRY(launch_grid(c, k_post_coef_mfma<1>, g, TPB, 0, P, tab, k, cv->d, shift, wd, S, nseg, seglen, ncoef, part_c)); break;
                    case 2: PGD_TRY(launch_grid(c, k_post_coef_mfma<2>, g, TPB, 0, P, tab, k, cv->d, shift, wd, S, nseg, seglen, ncoef, part_c)); break;
                    case 3: PGD_TRY(launch_grid(c, k_post_coef_mfma<3>, g, TPB, 0, P, tab, k, cv->d, shift, wd, S, nseg, seglen, ncoef, part_c)); break;
                    default: PGD_TRY(launch_grid(c, k_post_coef_mfma<4>, g, TPB, 0, P, tab, k, cv->d, shift, wd, S, nseg, seglen, ncoef, part_c)); break;
                }
            } else {
                PGD_HIP(c, hipMemsetAsync(part_c, 0, (size_t)nseg * ncoef * sizeof(double), c->stream));
                const size_t lds = (size_t)(k + 1) * 64 * sizeof(double);
                k_post_coef_plain<<<g, TPB, lds, c->stream>>>(P, tab, k, kp, cv->d, shift, wd, S, nseg, seglen, ncoef, part_c);
                PGD_LAUNCH_CHECK(c);
            }
            PGD_TRY(seg_sum(c, part_c, nseg, ncoef, ncoef, 1.0, od + PO_NV));
        }
        if (marg) {
            const int gm = (int)(nw < cap ? nw : cap);
            k_post_marginals<<<gm, TPB, 0, c->stream>>>(P, cv->d, shift, wd, S, nw, od + PO_NV + ncoef);
            PGD_LAUNCH_CHECK(c);
        }
        PGD_HIP(c, hipMemcpyAsync(out.data(), od, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the call
        return PGD_OK;
    });
    if (rc != PGD_OK) return rc;
    // ---- the caller's arrays are written only now
    sums[0] = out[0];
    sums[1] = out[1];
    if (theta) {
        int pr = 8;
        for (int d = 0; d < PO_DMAX; ++d) {
            if (d < ndim) theta1[d] = out[2 + d];
            for (int f = d; f < PO_DMAX; ++f, ++pr)
                if (f < ndim) theta2[d * ndim + f] = theta2[f * ndim + d] = out[pr];
        }
    }
    if (coef) {
        const double *oc = out.data() + PO_NV;
        for (int i = 0; i < k; ++i) {
            coef1[i] = oc[(size_t)kp * kp + i];
            for (int j = i; j < k; ++j) coef2[(size_t)i * k + j] = coef2[(size_t)j * k + i] = oc[(size_t)i * kp + j];
        }
    }
    if (marg) std::copy(out.begin() + PO_NV + ncoef, out.end(), marginals);
    return PGD_OK;
}

}  // extern "C"
