// Posteriors of MANY data sets on one tensor grid in one pass: pgd_grid_posterior_many.
//
// For data set j (a row u_j of m doubles and the scalars alpha_j, beta_j) and the sample s of the grid (pgd_post_grid.h)
//     p_s = a c(s),   chi2[j, s] = beta_j - 2 u_j . p_s + alpha_j |p_s|^2,
// an nd x m by m x S product behind the m x k by k x S product of pgd_grid_misfit.  Neither factor nor the nd x S result is ever
// stored: chi2 is reduced where it is formed, in two passes of the same kernel,
//     pass A: shift_j = min_s chi2[j, s] and the lowest sample that holds it,
//     pass B: e_js = w_s exp(-(chi2[j, s] - shift_j) / 2) and its sums against 1, th_d, th_d th_f (the features), and sum e^2.
// Both passes form chi2 by the same instructions in the same order, so pass B sees the bits pass A took the minimum of:
// chi2 - shift >= 0 exactly, and the minimising sample contributes exactly w_s.
//
// k_postmany_mfma: three chained products on v_mfma_f64_16x16x4_f64.  Lane (lq, lr) = (lane >> 4, lane & 15); the instruction's
// A operand is A[row lr][k lq], its B operand B[k lq][col lr], and D[4 r + lq][lr] comes back in acc[r].
//   * stage 1 (the product of k_misfit_mfma with one sample tile per wave; the two kernels keep their own copy of these few lines - as a
//     shared inline function they came out of the register allocator differently): acc1[r] = P[p = 16 mt + 4 r + lq][sample lr] from a
//     in fragment order (A, pack_a_fragments) and the coefficients of the tile's 16 samples (B), formed from the tables.  pp = |p|^2
//     of sample lr: one fma chain in ascending (mt, r), two __shfl_xor.
//   * stage 2: acc1[r] IS the A operand of the k-step (mt, r) of chi2^T = P^T U~^T (row = sample lr, k = p): nothing moves.  The B
//     operand is -2 u[data set lr][p = 16 mt + 4 r + lq], laid out by the host.  One more k-step carries (pp, 1, 0, 0) against
//     (alpha_j, beta_j, 0, 0).  acc2[dt][r] = chi2[sample 4 r + lq][data set 16 dt + lr] for the DB data tiles a wave holds.
//   * stage 3 (pass B): acc2 turned into e IS the B operand (k = sample, col = data set) of M^T = Phi^T E^T; A holds the features
//     Phi[v = lr][sample 4 r + lq], which the lane forms itself from the abscissae of those four samples.  Feature v is the pair
//     (a, b), a <= b, of (1, th_0 .. th_{D-1}) in row order of the upper triangle: v = 0 is Z, 1 .. D the first moments, then the
//     second ones.  D <= 3: one tile of 16 features and DB = 8 data tiles per wave; D <= 6: two tiles (28 features) and DB = 4.
//     sum e^2 is a plain fma chain per lane, two __shfl_xor at the end.
// A workgroup takes one (block of 16 DB data sets, segment of samples) at a time; its four waves deal the segment's tiles of 16
// samples (wave w: tiles w, w + 4, ..) and are added in ascending order through LDS; the block's fragments of u are staged in LDS
// once per such item, those of a once per workgroup.  The segments are grid_segments' with PM_SEGMIN: a function of S alone.  k_seg_sum
// adds them in ascending order.  No floating-point atomics; a column of an MFMA result does not depend on the other columns -
// every output of a data set is the same bits from run to run, for any grid (PGD_TUNE_POSTMANY_GRID_MAX), alone or among others,
// in any position of any chunk.
// Skip (PGD_TUNE_POSTMANY_SKIP): when chi2 - shift > PM_SKIP for all 64 entries of a (sample tile, data tile), every e would be
// w * exp(< -750) = w * 0 = +-0 for the finite weights the call insists on, and adding +-0 to an accumulator that started at +0
// changes no bit: the exponentials and stage 3 of that tile are left out.
// k_postmany_plain (PGD_TUNE_POSTMANY_VARIANT = 0): the same formula from ascending fma chains, a thread per data set.
#include "pgd_post_grid.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pgd {

constexpr int PM_KMAX = 64;             // modes
constexpr int PM_MMAX = 64;             // rows of a
constexpr int PM_DB1 = 8;               // data tiles of 16 a wave holds with one feature tile (ndim <= 3)
constexpr int PM_DB2 = 4;               // .. with two feature tiles
constexpr double PM_SKIP = 1500.0;      // exp(-750) rounds to 0: the smallest subnormal is exp(-744.44..)
constexpr int64_t PM_PART_MAX = (int64_t)1 << 25;   // doubles of the partials of a chunk of data sets (256 MB)
constexpr int PM_PLAIN_SB = 16;         // k_postmany_plain: samples per batch

// th_{a-1} of the sample with the indices idx; a = 0: the constant 1
__device__ __forceinline__ double pm_theta(const PostDims &P, const double *__restrict__ absc, const int (&idx)[PO_DMAX], int a) {
    long long off = 0;
#pragma unroll
    for (int d = 0; d < PO_DMAX; ++d)
        if (a - 1 == d) off = P.woff[d] + idx[d];
    return a == 0 ? 1.0 : absc[off];
}

// the pair (a, b) of feature v for D dimensions; beyond the last feature (0, 0)
__device__ __forceinline__ void pm_feature(int D, int v, int &a, int &b) {
    a = b = 0;
    int cnt = 0;
#pragma unroll
    for (int aa = 0; aa <= PO_DMAX; ++aa) {
#pragma unroll
        for (int bb = aa; bb <= PO_DMAX; ++bb) {
            if (aa <= D && bb <= D) {
                if (cnt == v) { a = aa; b = bb; }
                ++cnt;
            }
        }
    }
}

// Stages 1 and 2 for the tile whose sample lr is s_lr: acc2[dt][r] = chi2[sample 4 r + lq of the tile][data set 16 dt + lr of the block].
// af, uf: a's and the block's fragments (both in LDS), nstep = 4 mtn + 1 k-steps of 64 doubles per data tile.
template <int KT, int DB>
__device__ __forceinline__ void pm_chi2_tile(const PostDims &P, const double *__restrict__ tab, int k, int mtn, const double *__restrict__ af,
                                             const double *__restrict__ uf, unsigned s_lr, int lane, d4_t (&acc2)[DB]) {
    const int lq = lane >> 4;
    const int nstep = 4 * mtn + 1;
    int idx[PO_DMAX];
    post_decode(P, s_lr, idx);
    double b[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) b[q] = 1.0;
#pragma unroll
    for (int d = 0; d < PO_DMAX; ++d) {
        if (d < P.ndim) {
            const double *tp = tab + P.toff[d] + idx[d] + (long long)lq * P.n[d];
#pragma unroll
            for (int q = 0; q < KT; ++q) b[q] *= 4 * q + lq < k ? tp[(long long)(4 * q) * P.n[d]] : 0.0;
        }
    }
#pragma unroll
    for (int dt = 0; dt < DB; ++dt) acc2[dt] = d4_t{0.0, 0.0, 0.0, 0.0};
    double pp = 0.0;
    for (int mt = 0; mt < mtn; ++mt) {
        d4_t acc1 = d4_t{0.0, 0.0, 0.0, 0.0};
        const double *ap = af + (size_t)mt * KT * 64 + lane;
#pragma unroll
        for (int q = 0; q < KT; ++q) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[q * 64], b[q], acc1, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pp = fma(acc1[r], acc1[r], pp);
            const double *up = uf + (size_t)(4 * mt + r) * 64 + lane;
#pragma unroll
            for (int dt = 0; dt < DB; ++dt) acc2[dt] = __builtin_amdgcn_mfma_f64_16x16x4f64(acc1[r], up[(size_t)dt * nstep * 64], acc2[dt], 0, 0, 0);
        }
    }
    pp += __shfl_xor(pp, 16, 64);
    pp += __shfl_xor(pp, 32, 64);
    const double av = lq == 0 ? pp : lq == 1 ? 1.0 : 0.0;
    const double *up = uf + (size_t)(4 * mtn) * 64 + lane;
#pragma unroll
    for (int dt = 0; dt < DB; ++dt) acc2[dt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, up[(size_t)dt * nstep * 64], acc2[dt], 0, 0, 0);
}

// KT: k-steps of 4 (4 KT >= k); DB: data tiles per wave; FT: feature tiles; SUMS: pass B (false: pass A)
// pass A: part[(seg * 2 + 0) * ndp + j] = the segment's min of data set j, part[(seg * 2 + 1) * ndp + j] = its lowest sample, as a double
// pass B: part[(seg * nvs + v) * ndp + j] = the segment's sum of e_js feature_v(s), v < nfeat; v = nfeat: its sum of e_js^2
template <int KT, int DB, int FT, bool SUMS>
__global__ __launch_bounds__(TPB) void k_postmany_mfma(PostDims P, const double *__restrict__ tab, int k, int mtn, const double *__restrict__ af,
                                                       const double *__restrict__ uf, const double *__restrict__ wts,
                                                       const double *__restrict__ absc, const double *__restrict__ shift, int64_t S, int nseg,
                                                       int64_t seglen, int ndblk, int64_t ndp, int nfeat, int skip, double *__restrict__ part) {
    extern __shared__ double s_dyn[];      // a's fragments (mtn KT 64 doubles), the data block's (DB nstep 64), then what the waves hand to wave 0
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    const int nstep = 4 * mtn + 1, nvs = nfeat + 1;
    double *s_af = s_dyn, *s_uf = s_af + (size_t)mtn * KT * 64, *s_acc = s_uf + (size_t)DB * nstep * 64;
    for (int i = threadIdx.x; i < mtn * KT * 64; i += TPB) s_af[i] = af[i];
    int fa[FT], fb[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) pm_feature(P.ndim, 16 * ft + lr < nfeat ? 16 * ft + lr : 0, fa[ft], fb[ft]);
    const int64_t nitem = (int64_t)ndblk * nseg;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int dblk = (int)(item / nseg), seg = (int)(item - (int64_t)dblk * nseg);
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        const int64_t ntile = (hi - lo + 15) / 16;
        const double *ufb = uf + (size_t)dblk * DB * nstep * 64;
        const int64_t j0 = (int64_t)dblk * DB * 16;
        for (int i = threadIdx.x; i < DB * nstep * 64; i += TPB) s_uf[i] = ufb[i];
        __syncthreads();
        d4_t M[FT][DB];
        double s2[DB], sh[DB], bmn[DB], bix[DB];
#pragma unroll
        for (int dt = 0; dt < DB; ++dt) {
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) M[ft][dt] = d4_t{0.0, 0.0, 0.0, 0.0};
            s2[dt] = 0.0;
            sh[dt] = SUMS ? shift[j0 + 16 * dt + lr] : 0.0;
            bmn[dt] = bix[dt] = INF;
        }
        for (int64_t t = wv; t < ntile; t += 4) {
            const int64_t base = lo + 16 * t;
            const int64_t s1 = base + lr < hi ? base + lr : hi - 1;        // (a sample beyond the segment repeats its last one: its e is 0)
            d4_t acc2[DB];
            pm_chi2_tile<KT, DB>(P, tab, k, mtn, s_af, s_uf, (unsigned)s1, lane, acc2);
            if (!SUMS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t s = base + 4 * r + lq;
                    if (s < hi) {
                        const double ix = (double)s;
#pragma unroll
                        for (int dt = 0; dt < DB; ++dt)
                            if (post_less(acc2[dt][r], ix, bmn[dt], bix[dt])) { bmn[dt] = acc2[dt][r]; bix[dt] = ix; }
                    }
                }
            } else {
                // the lane's own four samples 4 r + lq: weight and features
                double w[4], ph[FT][4];
                bool val[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t s = base + 4 * r + lq;
                    val[r] = s < hi;
                    int idx[PO_DMAX];
                    post_decode(P, (unsigned)(val[r] ? s : hi - 1), idx);
                    w[r] = post_weight(P, wts, idx);
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) ph[ft][r] = pm_theta(P, absc, idx, fa[ft]) * pm_theta(P, absc, idx, fb[ft]);
                }
#pragma unroll
                for (int dt = 0; dt < DB; ++dt) {
                    double tt[4];
                    bool far = true;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tt[r] = acc2[dt][r] - sh[dt];
                        far = far && tt[r] > PM_SKIP;
                    }
                    if (!(skip && __all(far))) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double e = val[r] ? w[r] * exp(-0.5 * tt[r]) : 0.0;
                            s2[dt] = fma(e, e, s2[dt]);
#pragma unroll
                            for (int ft = 0; ft < FT; ++ft) M[ft][dt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ph[ft][r], e, M[ft][dt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // ---- the lanes over lq, then the waves 1, 2, 3 in turn through LDS, added by wave 0 in that order
        if (!SUMS) {
#pragma unroll
            for (int dt = 0; dt < DB; ++dt) {
#pragma unroll
                for (int x = 16; x < 64; x <<= 1) {
                    const double omn = __shfl_xor(bmn[dt], x, 64), oix = __shfl_xor(bix[dt], x, 64);
                    if (post_less(omn, oix, bmn[dt], bix[dt])) { bmn[dt] = omn; bix[dt] = oix; }
                }
            }
        } else {
#pragma unroll
            for (int dt = 0; dt < DB; ++dt) {
                s2[dt] += __shfl_xor(s2[dt], 16, 64);
                s2[dt] += __shfl_xor(s2[dt], 32, 64);
            }
        }
        for (int w = 1; w < 4; ++w) {
            __syncthreads();
            if (wv == w) {
                if (!SUMS) {
#pragma unroll
                    for (int dt = 0; dt < DB; ++dt) {
                        s_acc[(2 * dt) * 64 + lane] = bmn[dt];
                        s_acc[(2 * dt + 1) * 64 + lane] = bix[dt];
                    }
                } else {
#pragma unroll
                    for (int dt = 0; dt < DB; ++dt) {
#pragma unroll
                        for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) s_acc[((ft * DB + dt) * 4 + r) * 64 + lane] = M[ft][dt][r];
                        }
                        s_acc[(FT * DB * 4 + dt) * 64 + lane] = s2[dt];
                    }
                }
            }
            __syncthreads();
            if (wv == 0) {
                if (!SUMS) {
#pragma unroll
                    for (int dt = 0; dt < DB; ++dt) {
                        const double omn = s_acc[(2 * dt) * 64 + lane], oix = s_acc[(2 * dt + 1) * 64 + lane];
                        if (post_less(omn, oix, bmn[dt], bix[dt])) { bmn[dt] = omn; bix[dt] = oix; }
                    }
                } else {
#pragma unroll
                    for (int dt = 0; dt < DB; ++dt) {
#pragma unroll
                        for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) M[ft][dt][r] += s_acc[((ft * DB + dt) * 4 + r) * 64 + lane];
                        }
                        s2[dt] += s_acc[(FT * DB * 4 + dt) * 64 + lane];
                    }
                }
            }
        }
        if (wv == 0) {
            if (!SUMS) {
                if (lq == 0) {
#pragma unroll
                    for (int dt = 0; dt < DB; ++dt) {
                        part[((size_t)seg * 2) * ndp + j0 + 16 * dt + lr] = bmn[dt];
                        part[((size_t)seg * 2 + 1) * ndp + j0 + 16 * dt + lr] = bix[dt];
                    }
                }
            } else {
#pragma unroll
                for (int dt = 0; dt < DB; ++dt) {
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int v = 16 * ft + 4 * r + lq;
                            if (v < nfeat) part[((size_t)seg * nvs + v) * ndp + j0 + 16 * dt + lr] = M[ft][dt][r];
                        }
                    }
                    if (lq == 0) part[((size_t)seg * nvs + nfeat) * ndp + j0 + 16 * dt + lr] = s2[dt];
                }
            }
        }
        __syncthreads();
    }
}

// The same two passes from ordinary fma chains: a workgroup takes (256 data sets, segment), a thread one data set over the segment's
// samples in ascending order, PM_PLAIN_SB at a time: their coefficients, predictions p (m x k chains in ascending k), |p|^2 (ascending
// p), weights and abscissae in LDS.  a: m x k row-major; ut: row p holds -2 u[j][p] for the ndp data sets, row m alpha, row m + 1 beta.
template <bool SUMS>
__global__ __launch_bounds__(TPB) void k_postmany_plain(PostDims P, const double *__restrict__ tab, int k, int m, const double *__restrict__ a,
                                                        const double *__restrict__ ut, const double *__restrict__ wts,
                                                        const double *__restrict__ absc, const double *__restrict__ shift, int64_t S, int nseg,
                                                        int64_t seglen, int ndblk, int64_t ndp, int nfeat, double *__restrict__ part) {
    constexpr int SB = PM_PLAIN_SB;
    __shared__ double s_c[PM_KMAX * SB], s_p[PM_MMAX * SB], s_pp[SB], s_w[SB], s_th[PO_DMAX * SB];
    const double INF = __builtin_huge_val();
    const int tid = threadIdx.x;
    const int nvs = nfeat + 1;
    const int64_t nitem = (int64_t)ndblk * nseg;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int dblk = (int)(item / nseg), seg = (int)(item - (int64_t)dblk * nseg);
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        const int64_t j = (int64_t)dblk * TPB + tid;
        const bool jv = j < ndp;
        const double alpha = jv ? ut[(size_t)m * ndp + j] : 0.0, beta = jv ? ut[(size_t)(m + 1) * ndp + j] : 0.0;
        const double sh = SUMS && jv ? shift[j] : 0.0;
        double bmn = INF, bix = INF;
        double z = 0.0, z2 = 0.0, t1[PO_DMAX], t2[PO_DMAX * (PO_DMAX + 1) / 2];
#pragma unroll
        for (int d = 0; d < PO_DMAX; ++d) t1[d] = 0.0;
#pragma unroll
        for (int u = 0; u < PO_DMAX * (PO_DMAX + 1) / 2; ++u) t2[u] = 0.0;
        for (int64_t b0 = lo; b0 < hi; b0 += SB) {
            __syncthreads();
            for (int ent = tid; ent < k * SB; ent += TPB) {
                const int kk = ent / SB, x = ent - kk * SB;
                int idx[PO_DMAX];
                post_decode(P, (unsigned)(b0 + x < hi ? b0 + x : hi - 1), idx);
                s_c[ent] = post_coef(P, tab, idx, kk);
            }
            if (SUMS && tid < SB) {
                int idx[PO_DMAX];
                post_decode(P, (unsigned)(b0 + tid < hi ? b0 + tid : hi - 1), idx);
                s_w[tid] = post_weight(P, wts, idx);
#pragma unroll
                for (int d = 0; d < PO_DMAX; ++d) s_th[d * SB + tid] = d < P.ndim && absc ? absc[P.woff[d] + idx[d]] : 0.0;
            }
            __syncthreads();
            for (int ent = tid; ent < m * SB; ent += TPB) {
                const int p = ent / SB, x = ent - p * SB;
                const double *arow = a + (size_t)p * k;
                double t = 0.0;
                for (int kk = 0; kk < k; ++kk) t = fma(arow[kk], s_c[kk * SB + x], t);
                s_p[ent] = t;
            }
            __syncthreads();
            if (tid < SB) {
                double t = 0.0;
                for (int p = 0; p < m; ++p) t = fma(s_p[p * SB + tid], s_p[p * SB + tid], t);
                s_pp[tid] = t;
            }
            __syncthreads();
            if (jv) {
                double c2[SB];
#pragma unroll
                for (int x = 0; x < SB; ++x) c2[x] = 0.0;
                for (int p = 0; p < m; ++p) {
                    const double u2 = ut[(size_t)p * ndp + j];
#pragma unroll
                    for (int x = 0; x < SB; ++x) c2[x] = fma(u2, s_p[p * SB + x], c2[x]);
                }
#pragma unroll
                for (int x = 0; x < SB; ++x) {
                    if (b0 + x < hi) {
                        const double chi2 = fma(alpha, s_pp[x], c2[x]) + beta;
                        if (!SUMS) {
                            const double ix = (double)(b0 + x);
                            if (post_less(chi2, ix, bmn, bix)) { bmn = chi2; bix = ix; }
                        } else {
                            const double e = s_w[x] * exp(-0.5 * (chi2 - sh));
                            z += e;
                            z2 = fma(e, e, z2);
                            if (nfeat > 1) {
                                int pr = 0;
#pragma unroll
                                for (int d = 0; d < PO_DMAX; ++d) {
                                    t1[d] = fma(e, s_th[d * SB + x], t1[d]);
                                    const double et = e * s_th[d * SB + x];
#pragma unroll
                                    for (int f = d; f < PO_DMAX; ++f, ++pr) t2[pr] = fma(et, s_th[f * SB + x], t2[pr]);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (jv) {
            if (!SUMS) {
                part[((size_t)seg * 2) * ndp + j] = bmn;
                part[((size_t)seg * 2 + 1) * ndp + j] = bix;
            } else {
                part[((size_t)seg * nvs) * ndp + j] = z;
                part[((size_t)seg * nvs + nfeat) * ndp + j] = z2;
                if (nfeat > 1) {
                    int pr = 0, v = 1 + P.ndim;
#pragma unroll
                    for (int d = 0; d < PO_DMAX; ++d) {
                        if (d < P.ndim) part[((size_t)seg * nvs + 1 + d) * ndp + j] = t1[d];
#pragma unroll
                        for (int f = d; f < PO_DMAX; ++f, ++pr)
                            if (f < P.ndim) part[((size_t)seg * nvs + v++) * ndp + j] = t2[pr];
                    }
                }
            }
        }
    }
}

// out[j] = the min over the segments of data set j, out[ndp + j] = the lowest sample that holds it
__global__ __launch_bounds__(TPB) void k_postmany_min(const double *__restrict__ part, int nseg, int64_t ndp, double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (j >= ndp) return;
    double mn = __builtin_huge_val(), ix = __builtin_huge_val();
    for (int seg = 0; seg < nseg; ++seg) {
        const double omn = part[((size_t)seg * 2) * ndp + j], oix = part[((size_t)seg * 2 + 1) * ndp + j];
        if (post_less(omn, oix, mn, ix)) { mn = omn; ix = oix; }
    }
    out[j] = mn;
    out[ndp + j] = ix;
}

struct PmArgs {
    PostDims P;
    const double *tab, *af, *uf, *wts, *absc, *shift;
    int k, m, mtn, nseg, ndblk, nfeat, skip;
    int64_t S, seglen, ndp;
    double *part;
};

template <int KT, int DB, int FT, bool SUMS>
static int postmany_launch(Ctx *c, const PmArgs &A) {
    const size_t lds = ((size_t)A.mtn * KT + (size_t)DB * (4 * A.mtn + 1) + (SUMS ? FT * DB * 4 + DB : 2 * DB)) * 64 * sizeof(double);
    PGD_TRY(raise_lds(c, (const void *)k_postmany_mfma<KT, DB, FT, SUMS>, lds, "grid_posterior_many"));
    return launch_persistent(c, k_postmany_mfma<KT, DB, FT, SUMS>, TPB, lds, (int64_t)A.ndblk * A.nseg, c->postmany_grid_max, 0, nullptr, A.P, A.tab, A.k,
                             A.mtn, A.af, A.uf, A.wts, A.absc, A.shift, A.S, A.nseg, A.seglen, A.ndblk, A.ndp, A.nfeat, A.skip, A.part);
}

// (k <= PM_KMAX = 64: the instances end at KT = 16)
template <int DB, int FT, bool SUMS>
static int postmany_launch_kt(Ctx *c, int kt, const PmArgs &A) {
    return dense_dispatch<16>(kt, [&](auto KT, auto) { return postmany_launch<decltype(KT)::value, DB, FT, SUMS>(c, A); });
}

template <bool SUMS>
static int postmany_launch_plain(Ctx *c, const PmArgs &A) {
    return launch_persistent(c, k_postmany_plain<SUMS>, TPB, 0, (int64_t)A.ndblk * A.nseg, c->postmany_grid_max, 4, nullptr, A.P, A.tab, A.k, A.m, A.af,
                             A.uf, A.wts, A.absc, A.shift, A.S, A.nseg, A.seglen, A.ndblk, A.ndp, A.nfeat, A.part);
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_postmany_data_block(int ndim) { return 16 * (ndim <= 3 ? PM_DB1 : PM_DB2); }

int pgd_grid_posterior_many(pgd_handle h, const double *a, int m, int k, const double *u, const double *alpha, const double *beta, int64_t nd,
                            const double *tables, const int *n, int ndim, const double *weights, const double *abscissae, int want,
                            double *chi2_min, int64_t *argmin, double *sums, double *theta1, double *theta2) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (want & ~PGD_POST_THETA) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: want = %d, PGD_POST_THETA is the only bit it takes", want);
    if (k < 1 || k > PM_KMAX || m < 1 || m > PM_MMAX)
        return fail(c, PGD_ERR_INVALID, "grid_posterior_many: k = %d modes and m = %d rows, 1 .. %d and 1 .. %d are possible: compress the solution "
                    "first (PGD.compress)", k, m, PM_KMAX, PM_MMAX);
    if (ndim < 1 || ndim > PO_DMAX) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: ndim = %d, 1 .. %d are possible", ndim, PO_DMAX);
    if (nd < 1 || nd >= ((int64_t)1 << 31)) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: %lld data sets, 1 .. 2^31 - 1 are possible", (long long)nd);
    if (!a || !u || !alpha || !beta || !tables || !n || !weights) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: a, u, alpha, beta, tables, n or weights missing");
    if (!chi2_min || !argmin || !sums) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: chi2_min, argmin or sums missing");
    const bool theta = (want & PGD_POST_THETA) != 0;
    if (theta && (!abscissae || !theta1 || !theta2)) return fail(c, PGD_ERR_INVALID, "grid_posterior_many: PGD_POST_THETA without abscissae, theta1 or theta2");
    PostDims P;
    int64_t S = 0, ntab = 0, nw = 0;
    if (!post_dims(n, ndim, k, &P, &S, &ntab, &nw))
        return fail(c, PGD_ERR_INVALID, "grid_posterior_many: a dimension without points, or 2^31 samples or more");
    for (int64_t i = 0; i < nw; ++i)
        if (!std::isfinite(weights[i]) || (theta && !std::isfinite(abscissae[i])))
            return fail(c, PGD_ERR_INVALID, "grid_posterior_many: a weight or an abscissa is not finite");

    int nseg = 1;
    int64_t seglen = 0;
    grid_segments(S, PM_SEGMIN, &nseg, &seglen);
    const bool mfma = c->postmany_variant != 0;
    const int kt = dense_kt(k), mtn = (m + 15) / 16, nstep = 4 * mtn + 1;
    const int db = ndim <= 3 ? PM_DB1 : PM_DB2, blk = 16 * db;
    const int nfeat = theta ? (ndim + 1) * (ndim + 2) / 2 : 1, nvs = nfeat + 1;
    // ---- the chunk of data sets whose partials stay below PM_PART_MAX doubles: whole blocks, at least one
    int64_t chunk = PM_PART_MAX / ((int64_t)nseg * nvs) / blk * blk;
    if (chunk < blk) chunk = blk;
    const int64_t ndp_max = std::min(chunk, (nd + blk - 1) / blk * blk);
    // a in the order the variant reads it; the data of a chunk: fragments (mfma) or rows (plain)
    const size_t na = mfma ? (size_t)mtn * kt * 64 : (size_t)m * k;
    const size_t nu_max = mfma ? (size_t)(ndp_max / 16) * nstep * 64 : (size_t)(m + 2) * ndp_max;
    std::vector<double> ha(na, 0.0), hu(nu_max, 0.0);
    if (mfma) pack_a_fragments(ha.data(), kt, a, m, k, k);
    else std::copy(a, a + (size_t)m * k, ha.begin());
    const int64_t nout_max = (int64_t)(2 + nvs) * ndp_max;
    std::vector<double> out((size_t)nout_max, 0.0);
    std::vector<double> r_min((size_t)nd), r_arg((size_t)nd), r_sum((size_t)nd * nvs);
    const int rc = with_pool_input(c, pool_bytes((size_t)ntab + 2 * (size_t)nw + na + nu_max), [&](void *p_in) -> int {
        double *tab = (double *)p_in, *wd = tab + ntab, *xd = wd + nw, *ad = xd + nw, *ud = ad + na;
        PGD_TRY(ensure_work(c, 6, nout_max));
        PGD_TRY(ensure_partials(c, (int64_t)nseg * nvs * ndp_max > 2 * (int64_t)nseg * ndp_max ? (int64_t)nseg * nvs * ndp_max : 2 * (int64_t)nseg * ndp_max));
        PGD_HIP(c, hipMemcpyAsync(tab, tables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(wd, weights, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (theta) PGD_HIP(c, hipMemcpyAsync(xd, abscissae, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(ad, ha.data(), na * sizeof(double), hipMemcpyHostToDevice, c->stream));
        for (int64_t c0 = 0; c0 < nd; c0 += chunk) {
            const int64_t cn = std::min(chunk, nd - c0), ndp = (cn + blk - 1) / blk * blk;
            const size_t nu = mfma ? (size_t)(ndp / 16) * nstep * 64 : (size_t)(m + 2) * ndp;
            std::fill(hu.begin(), hu.begin() + nu, 0.0);            // (data sets beyond cn: chi2 = 0 everywhere, never read back)
            for (int64_t j = 0; j < cn; ++j) {
                const double *uj = u + (size_t)(c0 + j) * m;
                if (mfma) {
                    double *f = hu.data() + (size_t)(j >> 4) * nstep * 64 + (j & 15);
                    for (int p = 0; p < m; ++p) f[(size_t)(p >> 2) * 64 + ((p & 3) << 4)] = -2.0 * uj[p];
                    f[(size_t)(4 * mtn) * 64] = alpha[c0 + j];
                    f[(size_t)(4 * mtn) * 64 + 16] = beta[c0 + j];
                } else {
                    for (int p = 0; p < m; ++p) hu[(size_t)p * ndp + j] = -2.0 * uj[p];
                    hu[(size_t)m * ndp + j] = alpha[c0 + j];
                    hu[(size_t)(m + 1) * ndp + j] = beta[c0 + j];
                }
            }
            PGD_HIP(c, hipMemcpyAsync(ud, hu.data(), nu * sizeof(double), hipMemcpyHostToDevice, c->stream));
            double *od = c->work[6];
            PmArgs A;
            A.P = P; A.tab = tab; A.af = ad; A.uf = ud; A.wts = wd; A.absc = theta ? xd : nullptr; A.shift = od;
            A.k = k; A.m = m; A.mtn = mtn; A.nseg = nseg; A.nfeat = nfeat; A.skip = c->postmany_skip;
            A.ndblk = mfma ? (int)(ndp / blk) : (int)((ndp + TPB - 1) / TPB);
            A.S = S; A.seglen = seglen; A.ndp = ndp; A.part = c->partials;
            // pass A, the minima, pass B, the sums
            if (!mfma) PGD_TRY(postmany_launch_plain<false>(c, A));
            else if (db == PM_DB1) PGD_TRY((postmany_launch_kt<PM_DB1, 1, false>(c, kt, A)));
            else PGD_TRY((postmany_launch_kt<PM_DB2, 2, false>(c, kt, A)));
            k_postmany_min<<<(int)((ndp + TPB - 1) / TPB), TPB, 0, c->stream>>>(c->partials, nseg, ndp, od);
            PGD_LAUNCH_CHECK(c);
            if (!mfma) PGD_TRY(postmany_launch_plain<true>(c, A));
            else if (db == PM_DB1) PGD_TRY((postmany_launch_kt<PM_DB1, 1, true>(c, kt, A)));
            else PGD_TRY((postmany_launch_kt<PM_DB2, 2, true>(c, kt, A)));
            const int64_t nsum = (int64_t)nvs * ndp;
            PGD_TRY(seg_sum(c, c->partials, nseg, nsum, nsum, 1.0, od + 2 * ndp));
            PGD_HIP(c, hipMemcpyAsync(out.data(), od, (size_t)(2 + nvs) * ndp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the chunk
            for (int64_t j = 0; j < cn; ++j) {
                r_min[c0 + j] = out[j];
                r_arg[c0 + j] = out[ndp + j];
                for (int v = 0; v < nvs; ++v) r_sum[(size_t)(c0 + j) * nvs + v] = out[(size_t)(2 + v) * ndp + j];
            }
        }
        return PGD_OK;
    });
    if (rc != PGD_OK) return rc;
    // ---- the caller's arrays are written only now
    for (int64_t j = 0; j < nd; ++j) {
        const double *o = r_sum.data() + (size_t)j * nvs;
        chi2_min[j] = r_min[j];
        argmin[j] = r_arg[j] < 2147483648.0 ? (int64_t)r_arg[j] : -1;   // (-1: no value compares, every chi2 is NaN)
        sums[2 * j] = o[0];
        sums[2 * j + 1] = o[nfeat];
        if (theta) {
            int v = 1 + ndim;
            for (int d = 0; d < ndim; ++d) {
                theta1[(size_t)j * ndim + d] = o[1 + d];
                for (int f = d; f < ndim; ++f, ++v) theta2[((size_t)j * ndim + d) * ndim + f] = theta2[((size_t)j * ndim + f) * ndim + d] = o[v];
            }
        }
    }
    return PGD_OK;
}

}  // extern "C"
