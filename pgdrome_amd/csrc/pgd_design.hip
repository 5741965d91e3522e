// Sensor placement by greedy expected information gain (Bayesian D-optimality, linearised): pgd_design_update and pgd_design_gains.
//
// The samples s = (i_0 .. i_{D-1}) of the tensor grid, the tables and the weights are pgd_post_grid.h's.  The derivative coefficient
// of mode t against coordinate d is the chain  cd_t(s) = 1 * U_0[t, i_0] * U_1[t, i_1] * ..  in ascending f, U_f = dtables_f for f == d
// and tables_f otherwise (the bits of model.py's mode_factor_derivatives_many on the same tables); the Jacobian of a row p of a is
// g_p,d(s) = sum_t a[p, t] cd_t(s).  No prefix or suffix products: every coefficient is its own chain.
//
// The state is one vector of 2 nh S doubles, nh = D (D + 1) / 2, plane-major: state[c S + s] is entry c of H_s, the UPPER triangle in row
// order (c = 0: (0, 0), 1: (0, 1), .. D - 1: (0, D - 1), D: (1, 1), ..), state[(nh + c) S + s] entry c of W_s = inverse of the lower
// Cholesky factor of H_s, the LOWER triangle in row order (c = i (i + 1) / 2 + j for j <= i).
//
// k_design_update<ND>: a thread per sample.  H_s (= h0 first, if given) += g_r g_r^T for the R rows, g from fma chains in ascending t,
// the products into H in ascending r; the Cholesky factor L (row by row, fma chains in ascending column), W by forward substitution
// of the columns of the identity; sums[0] += w_s (-2 sum_i log W_ii), sums[1 + c] += w_s (W^T W)_c (upper triangle, row order).
// H is only ever added to.  The partial sums of a segment (grid_segments: a function of S alone) are formed in an order that depends
// on the segment alone; k_seg_sum adds the segments in ascending order.
//
// k_design_gains_mfma<R, ND>: the Jacobians of ALL candidates at ALL samples as one dense product on v_mfma_f64_16x16x4_f64 that is
// never stored.  Lane (lq, lr) = (lane >> 4, lane & 15).  A: 16 candidates on the row index, lane holds a[row r of candidate 16 ct + lr]
// [t = 4 q + lq] (the host lays a out in fragment order per plane r: pack_a_fragments, zero padded).  B: 16 samples on the column index, lane
// holds cd_{4 q + lq}(sample lr).  acc[r][d][rr] = g_{r, d} of candidate 16 ct + 4 rr + lq at sample lr: a lane holds the same
// (candidate, sample) entry of all R ND tiles, the epilogue is lane-local (design_gain below), then w_s times it.
//   * A workgroup takes one (chunk of at most 2048 candidates, segment of the samples) at a time.  It stages the derivative coefficients
//     of a block of SB samples (32 for D <= 3, 16 above) for all D coordinates in LDS once, in the order the B operand is read in.
//   * For each of the block's tiles of 16 samples, in ascending order, the lane loads W_s of its sample once, and the four waves walk
//     the chunk's candidate tiles (wave w: tiles w, w + 4, ..): A from global memory (L2) four k-steps at a time, B from LDS.
//   * The 16 sample lanes are added by a fixed xor tree (1, 2, 4, 8), the lanes lr == 0 add into the candidate's accumulator in LDS:
//     one writer wave per accumulator, blocks and tiles in ascending order.  part[seg * Mp + j] = the segment's sum of candidate j.
//   * k_seg_sum: gains[j] = 1/2 of the sum over the segments in ascending order.
// No floating-point atomics.  A row of an MFMA result does not depend on the other rows, the order of a candidate's sum depends on the
// segment alone: every gain is the same bits from run to run, for any grid (PGD_TUNE_DESIGN_GRID_MAX), for any chunking, alone or among
// others, at any position.
// k_design_gains_plain<R, ND> (PGD_TUNE_DESIGN_VARIANT = 0): a thread per candidate, ordinary fma chains in ascending t, the samples of
// the segment in ascending order: the cross-check and the baseline (it agrees within rounding, not bit for bit).
#include "pgd_post_grid.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pgd {

constexpr int DS_KMAX = 64;             // modes
constexpr int DS_RMAX = 3;              // rows of a candidate
constexpr int DS_UPD_RMAX = 256;        // rows of one pgd_design_update
constexpr int DS_CHUNK = 2048;          // most candidates of a work item: their accumulators in LDS
constexpr int DS_CHUNK_MIN = 64;        // fewest: a tile of 16 per wave
constexpr int DS_PLAIN_SB = 16;         // k_design_gains_plain: samples per batch
constexpr int64_t DS_PART_MAX = (int64_t)1 << 25;   // doubles of the partials of a chunk of candidates (256 MB)

__host__ __device__ constexpr int ds_nh(int nd) { return nd * (nd + 1) / 2; }
// samples of a staged block of k_design_gains_mfma: with the accumulators at most 65 KB of LDS at 64 modes, two workgroups per CU or more -
// one wave's epilogue runs under another's products
__host__ __device__ constexpr int ds_sb(int nd) { return nd <= 3 ? 32 : 16; }

// cd_t of the sample with the indices idx for coordinate d: one chain in ascending f
template <int ND>
__device__ __forceinline__ double design_coef(const PostDims &P, const double *__restrict__ tab, const double *__restrict__ dtab,
                                              const int (&idx)[PO_DMAX], int t, int d) {
    double c = 1.0;
#pragma unroll
    for (int f = 0; f < ND; ++f) {
        const long long o = P.toff[f] + (long long)t * P.n[f] + idx[f];
        c *= f == d ? dtab[o] : tab[o];
    }
    return c;
}

// sum of log1p(pivot - 1) over the LDL^T pivots of I + V^T V, V = W [g_0 .. g_{R-1}]: twice the gain of one (candidate, sample)
template <int R, int ND>
__device__ __forceinline__ double design_gain(const double (&g)[R][ND], const double (&W)[ds_nh(ND)]) {
    double V[R][ND];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j <= i; ++j) t = fma(W[i * (i + 1) / 2 + j], g[r][j], t);
            V[r][i] = t;
        }
    }
    double G[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
#pragma unroll
        for (int b = a; b < R; ++b) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < ND; ++i) t = fma(V[a][i], V[b][i], t);
            G[a][b] = t;
        }
    }
    double v = log1p(G[0][0]);
    if constexpr (R >= 2) {
        const double d0 = 1.0 + G[0][0];
        const double l10 = G[0][1] / d0;
        const double e1 = fma(-l10, G[0][1], G[1][1]);                 // pivot 1, less 1
        v += log1p(e1);
        if constexpr (R >= 3) {
            const double l20 = G[0][2] / d0;
            const double m21 = fma(-l20, G[0][1], G[1][2]);
            const double l21 = m21 / (1.0 + e1);
            const double e2 = fma(-l21, m21, fma(-l20, G[0][2], G[2][2]));   // pivot 2, less 1
            v += log1p(e2);
        }
    }
    return v;
}

template <int ND>
__global__ __launch_bounds__(TPB) void k_design_update(PostDims P, const double *__restrict__ tab, const double *__restrict__ dtab, int k, int R,
                                                       const double *__restrict__ rows, const double *__restrict__ h0,
                                                       const double *__restrict__ wts, int64_t S, int nseg, int64_t seglen,
                                                       double *__restrict__ state, double *__restrict__ part) {
    constexpr int NH = ds_nh(ND);
    __shared__ double s_red[4];
    const int tid = threadIdx.x;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        double acc[1 + NH];
#pragma unroll
        for (int v = 0; v <= NH; ++v) acc[v] = 0.0;
        for (int64_t s = lo + tid; s < hi; s += TPB) {
            int idx[PO_DMAX];
            post_decode(P, (unsigned)s, idx);
            double H[NH];
#pragma unroll
            for (int c = 0; c < NH; ++c) H[c] = h0 ? h0[c] : state[(size_t)c * S + s];
            for (int r = 0; r < R; ++r) {
                double g[ND];
#pragma unroll
                for (int d = 0; d < ND; ++d) g[d] = 0.0;
                for (int t = 0; t < k; ++t) {
                    const double av = rows[(size_t)r * k + t];
#pragma unroll
                    for (int d = 0; d < ND; ++d) g[d] = fma(av, design_coef<ND>(P, tab, dtab, idx, t, d), g[d]);
                }
                int c = 0;
#pragma unroll
                for (int i = 0; i < ND; ++i) {
#pragma unroll
                    for (int j = i; j < ND; ++j, ++c) H[c] = fma(g[i], g[j], H[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < NH; ++c) state[(size_t)c * S + s] = H[c];
            // L L^T = H, row by row
            double L[ND][ND], W[ND][ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    double t = H[j * ND - j * (j - 1) / 2 + (i - j)];          // H[j][i], j <= i
#pragma unroll
                    for (int m = 0; m < j; ++m) t = fma(-L[i][m], L[j][m], t);
                    L[i][j] = i == j ? sqrt(t) : t / L[j][j];
                }
            }
            // W = L^-1: column j by forward substitution
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                W[j][j] = 1.0 / L[j][j];
#pragma unroll
                for (int i = j + 1; i < ND; ++i) {
                    double t = 0.0;
#pragma unroll
                    for (int m = j; m < i; ++m) t = fma(L[i][m], W[m][j], t);
                    W[i][j] = -t / L[i][i];
                }
            }
            double ld = 0.0;
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                ld += log(W[i][i]);
#pragma unroll
                for (int j = 0; j <= i; ++j) state[(size_t)(NH + i * (i + 1) / 2 + j) * S + s] = W[i][j];
            }
            const double w = post_weight(P, wts, idx);
            acc[0] += w * (-2.0 * ld);
            int c = 0;
#pragma unroll
            for (int i = 0; i < ND; ++i) {
#pragma unroll
                for (int j = i; j < ND; ++j, ++c) {
                    double t = 0.0;
#pragma unroll
                    for (int m = j; m < ND; ++m) t = fma(W[m][i], W[m][j], t);
                    acc[1 + c] = fma(w, t, acc[1 + c]);
                }
            }
        }
#pragma unroll
        for (int v = 0; v <= NH; ++v) {
            const double t = block_sum(acc[v], s_red);
            if (tid == 0) part[(size_t)seg * (1 + NH) + v] = t;
        }
    }
}

// af: R planes of (Mp / 16) tiles of kt k-steps of 64 doubles; ncc chunks of cc candidates (cc a multiple of 64, Mp of 16)
template <int R, int ND>
__global__ __launch_bounds__(TPB) void k_design_gains_mfma(PostDims P, const double *__restrict__ tab, const double *__restrict__ dtab, int k, int kt,
                                                           const double *__restrict__ af, int64_t plane, const double *__restrict__ wts,
                                                           const double *__restrict__ state, int64_t S, int nseg, int64_t seglen, int ncc, int cc,
                                                           int64_t Mp, double *__restrict__ part) {
    constexpr int NH = ds_nh(ND), SB = ds_sb(ND), NJ = SB / 16;
    extern __shared__ double s_dyn[];      // the block's coefficients [ND][4 kt][SB], its weights [SB], the chunk's accumulators [cc]
    const int kp = 4 * kt;
    double *s_b = s_dyn, *s_w = s_b + (size_t)ND * kp * SB, *s_gain = s_w + SB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int64_t nitem = (int64_t)ncc * nseg;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int ci = (int)(item / nseg), seg = (int)(item - (int64_t)ci * nseg);
        const int64_t c0 = (int64_t)ci * cc;
        const int ntile = (int)((Mp - c0 < cc ? Mp - c0 : cc) / 16);
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        for (int i = tid; i < cc; i += TPB) s_gain[i] = 0.0;
        for (int64_t b0 = lo; b0 < hi; b0 += SB) {
            __syncthreads();               // (the last block's readers are done; the accumulators are zeroed)
            {
                const int x = tid & (SB - 1);
                const bool sv = b0 + x < hi;
                int idx[PO_DMAX];
                post_decode(P, (unsigned)(sv ? b0 + x : hi - 1), idx);      // (a sample beyond the segment repeats its last one: its weight is 0)
                for (int dt = tid / SB; dt < ND * kp; dt += TPB / SB) {
                    const int d = dt / kp, t = dt - d * kp;
                    s_b[(size_t)dt * SB + x] = t < k ? design_coef<ND>(P, tab, dtab, idx, t, d) : 0.0;
                }
                if (tid < SB) s_w[x] = sv ? post_weight(P, wts, idx) : 0.0;
            }
            __syncthreads();
#pragma unroll 1
            for (int j = 0; j < NJ; ++j) {
                if (b0 + 16 * j >= hi) break;
                const int64_t s1 = b0 + 16 * j + lr < hi ? b0 + 16 * j + lr : hi - 1;
                double W[NH];
#pragma unroll
                for (int c = 0; c < NH; ++c) W[c] = state[(size_t)(NH + c) * S + s1];
                const double wj = s_w[16 * j + lr];
#pragma unroll 1
                for (int ct = wv; ct < ntile; ct += 4) {
                    d4_t acc[R][ND];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
#pragma unroll
                        for (int d = 0; d < ND; ++d) acc[r][d] = d4_t{0.0, 0.0, 0.0, 0.0};
                    }
                    const double *ap = af + ((size_t)(c0 / 16 + ct) * kt) * 64 + lane;
                    const double *bp = s_b + (size_t)lq * SB + 16 * j + lr;
#pragma unroll 1
                    for (int q0 = 0; q0 < kt; q0 += 4) {
                        double av[4][R], bv[4][ND];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
#pragma unroll
                            for (int r = 0; r < R; ++r) av[u][r] = ap[(size_t)r * plane + (size_t)(q0 + u) * 64];
#pragma unroll
                            for (int d = 0; d < ND; ++d) bv[u][d] = bp[((size_t)d * kp + 4 * (q0 + u)) * SB];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
#pragma unroll
                            for (int r = 0; r < R; ++r) {
#pragma unroll
                                for (int d = 0; d < ND; ++d) acc[r][d] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][r], bv[u][d], acc[r][d], 0, 0, 0);
                            }
                        }
                    }
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        double g[R][ND];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
#pragma unroll
                            for (int d = 0; d < ND; ++d) g[r][d] = acc[r][d][rr];
                        }
                        double v = wj * design_gain<R, ND>(g, W);
#pragma unroll
                        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
                        if (lr == 0) s_gain[16 * ct + 4 * rr + lq] += v;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < 16 * ntile; i += TPB) part[(size_t)seg * Mp + c0 + i] = s_gain[i];
        __syncthreads();
    }
}

// a: the M R rows of k entries as the caller passed them; a workgroup takes (256 candidates, segment)
template <int R, int ND>
__global__ __launch_bounds__(TPB) void k_design_gains_plain(PostDims P, const double *__restrict__ tab, const double *__restrict__ dtab, int k,
                                                            const double *__restrict__ a, const double *__restrict__ wts,
                                                            const double *__restrict__ state, int64_t S, int nseg, int64_t seglen, int ncb, int64_t M,
                                                            int64_t Mp, double *__restrict__ part) {
    constexpr int NH = ds_nh(ND), SB = DS_PLAIN_SB;
    __shared__ double s_c[ND * DS_KMAX * SB], s_w[SB], s_W[NH * SB];
    const int tid = threadIdx.x;
    const int64_t nitem = (int64_t)ncb * nseg;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int cb = (int)(item / nseg), seg = (int)(item - (int64_t)cb * nseg);
        const int64_t lo = seg * seglen, hi = lo + seglen < S ? lo + seglen : S;
        const int64_t j = (int64_t)cb * TPB + tid;
        const bool jv = j < M;
        double total = 0.0;
        for (int64_t b0 = lo; b0 < hi; b0 += SB) {
            __syncthreads();
            for (int ent = tid; ent < ND * k * SB; ent += TPB) {
                const int dt = ent / SB, x = ent - dt * SB, d = dt / k, t = dt - d * k;
                int idx[PO_DMAX];
                post_decode(P, (unsigned)(b0 + x < hi ? b0 + x : hi - 1), idx);
                s_c[ent] = design_coef<ND>(P, tab, dtab, idx, t, d);
            }
            if (tid < SB) {
                const int64_t s = b0 + tid < hi ? b0 + tid : hi - 1;
                int idx[PO_DMAX];
                post_decode(P, (unsigned)s, idx);
                s_w[tid] = b0 + tid < hi ? post_weight(P, wts, idx) : 0.0;
#pragma unroll
                for (int c = 0; c < NH; ++c) s_W[c * SB + tid] = state[(size_t)(NH + c) * S + s];
            }
            __syncthreads();
            if (jv) {
                for (int x = 0; x < SB && b0 + x < hi; ++x) {
                    double g[R][ND], W[NH];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double *arow = a + ((size_t)j * R + r) * k;
#pragma unroll
                        for (int d = 0; d < ND; ++d) g[r][d] = 0.0;
                        for (int t = 0; t < k; ++t) {
                            const double av = arow[t];
#pragma unroll
                            for (int d = 0; d < ND; ++d) g[r][d] = fma(av, s_c[(d * k + t) * SB + x], g[r][d]);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NH; ++c) W[c] = s_W[c * SB + x];
                    total += s_w[x] * design_gain<R, ND>(g, W);
                }
            }
        }
        if (jv) part[(size_t)seg * Mp + j] = total;
    }
}

struct DsArgs {
    PostDims P;
    const double *tab, *dtab, *a, *wts, *state;
    int k, kt, nseg, ncc, cc;
    int64_t plane, S, seglen, M, Mp;
    double *part;
};

template <int R, int ND>
static int design_launch_mfma(Ctx *c, const DsArgs &A) {
    constexpr int SB = ds_sb(ND);
    const size_t lds = ((size_t)ND * 4 * A.kt * SB + SB + A.cc) * sizeof(double);
    PGD_TRY(raise_lds(c, (const void *)k_design_gains_mfma<R, ND>, lds, "design_gains"));
    return launch_persistent(c, k_design_gains_mfma<R, ND>, TPB, lds, (int64_t)A.ncc * A.nseg, c->design_grid_max, 0, nullptr, A.P, A.tab, A.dtab, A.k, A.kt,
                             A.a, A.plane, A.wts, A.state, A.S, A.nseg, A.seglen, A.ncc, A.cc, A.Mp, A.part);
}

template <int R, int ND>
static int design_launch_plain(Ctx *c, const DsArgs &A) {
    const int ncb = (int)((A.M + TPB - 1) / TPB);
    return launch_persistent(c, k_design_gains_plain<R, ND>, TPB, 0, (int64_t)ncb * A.nseg, c->design_grid_max, 4, nullptr, A.P, A.tab, A.dtab, A.k, A.a,
                             A.wts, A.state, A.S, A.nseg, A.seglen, ncb, A.M, A.Mp, A.part);
}

template <int R>
static int design_launch_nd(Ctx *c, bool mfma, int ndim, const DsArgs &A) {
    switch (ndim) {
        case 1: return mfma ? design_launch_mfma<R, 1>(c, A) : design_launch_plain<R, 1>(c, A);
        case 2: return mfma ? design_launch_mfma<R, 2>(c, A) : design_launch_plain<R, 2>(c, A);
        case 3: return mfma ? design_launch_mfma<R, 3>(c, A) : design_launch_plain<R, 3>(c, A);
        case 4: return mfma ? design_launch_mfma<R, 4>(c, A) : design_launch_plain<R, 4>(c, A);
        case 5: return mfma ? design_launch_mfma<R, 5>(c, A) : design_launch_plain<R, 5>(c, A);
        default: return mfma ? design_launch_mfma<R, 6>(c, A) : design_launch_plain<R, 6>(c, A);
    }
}

template <int ND>
static void design_update_go(Ctx *c, int g, const PostDims &P, const double *tab, const double *dtab, int k, int R, const double *rows,
                             const double *h0, const double *wts, int64_t S, int nseg, int64_t seglen, double *state, double *part) {
    k_design_update<ND><<<g, TPB, 0, c->stream>>>(P, tab, dtab, k, R, rows, h0, wts, S, nseg, seglen, state, part);
}

// true: the ndim x ndim row-major matrix is finite, symmetric bit for bit and has a Cholesky factor
static bool design_spd(const double *h, int nd) {
    double L[PO_DMAX][PO_DMAX];
    for (int i = 0; i < nd; ++i)
        for (int j = 0; j < nd; ++j)
            if (!std::isfinite(h[i * nd + j]) || h[i * nd + j] != h[j * nd + i]) return false;
    for (int i = 0; i < nd; ++i) {
        for (int j = 0; j <= i; ++j) {
            double t = h[i * nd + j];
            for (int m = 0; m < j; ++m) t -= L[i][m] * L[j][m];
            if (i == j) {
                if (!(t > 0.0)) return false;
                L[i][i] = std::sqrt(t);
            } else {
                L[i][j] = t / L[j][j];
            }
        }
    }
    return true;
}

// the checks both calls share
static int design_check(Ctx *c, const char *who, int k, int ndim, const double *tables, const double *dtables, const int *n, const double *weights,
                        pgd_handle stateh, PostDims *P, int64_t *S, int64_t *ntab, int64_t *nw, Vec **sv) {
    if (k < 1 || k > DS_KMAX)
        return fail(c, PGD_ERR_INVALID, "%s: k = %d modes, 1 .. %d are possible: compress the solution first (PGD.compress)", who, k, DS_KMAX);
    if (ndim < 1 || ndim > PO_DMAX) return fail(c, PGD_ERR_INVALID, "%s: ndim = %d, 1 .. %d are possible", who, ndim, PO_DMAX);
    if (!tables || !dtables || !n || !weights) return fail(c, PGD_ERR_INVALID, "%s: tables, dtables, n or weights missing", who);
    if (!post_dims(n, ndim, k, P, S, ntab, nw)) return fail(c, PGD_ERR_INVALID, "%s: a dimension without points, or 2^31 samples or more", who);
    for (int64_t i = 0; i < *nw; ++i)
        if (!std::isfinite(weights[i])) return fail(c, PGD_ERR_INVALID, "%s: a weight is not finite", who);
    *sv = get_vec(c, stateh);
    if (!*sv) return fail(c, PGD_ERR_INVALID, "%s: the state is not a vector", who);
    const int64_t need = 2 * (int64_t)ds_nh(ndim) * *S;
    if ((*sv)->n != need)
        return fail(c, PGD_ERR_INVALID, "%s: the state has %lld entries, 2 nh S = %lld are needed", who, (long long)(*sv)->n, (long long)need);
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_design_update(pgd_handle h, const double *h0, const double *rows, int R, int k, const double *tables, const double *dtables, const int *n,
                      int ndim, const double *weights, pgd_handle stateh, double *sums) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (R < 0 || R > DS_UPD_RMAX) return fail(c, PGD_ERR_INVALID, "design_update: R = %d rows, 0 .. %d are possible", R, DS_UPD_RMAX);
    if ((R > 0 && !rows) || !sums) return fail(c, PGD_ERR_INVALID, "design_update: rows or sums missing");
    PostDims P;
    int64_t S = 0, ntab = 0, nw = 0;
    Vec *sv = nullptr;
    PGD_TRY(design_check(c, "design_update", k, ndim, tables, dtables, n, weights, stateh, &P, &S, &ntab, &nw, &sv));
    if (h0 && !design_spd(h0, ndim)) return fail(c, PGD_ERR_INVALID, "design_update: h0 is not symmetric positive definite");

    const int nh = ds_nh(ndim), nv = 1 + nh;
    int nseg = 1;
    int64_t seglen = 0;
    grid_segments(S, PO_SEGMIN, &nseg, &seglen);
    std::vector<double> hbuf((size_t)R * k + nh, 0.0);          // the rows, then the upper triangle of h0
    if (R > 0) std::copy(rows, rows + (size_t)R * k, hbuf.begin());
    if (h0) {
        int cc = 0;
        for (int i = 0; i < ndim; ++i)
            for (int j = i; j < ndim; ++j, ++cc) hbuf[(size_t)R * k + cc] = h0[i * ndim + j];
    }
    double out[1 + PO_DMAX * (PO_DMAX + 1) / 2];
    const int rc = with_pool_input(c, pool_bytes(2 * (size_t)ntab + (size_t)nw + hbuf.size()), [&](void *p_in) -> int {
        PGD_TRY(ensure_work(c, 6, nv));
        PGD_TRY(ensure_partials(c, (int64_t)nseg * nv));
        double *tab = (double *)p_in, *dtab = tab + ntab, *wd = dtab + ntab, *rd = wd + nw, *hd = rd + (size_t)R * k;
        PGD_HIP(c, hipMemcpyAsync(tab, tables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(dtab, dtables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(wd, weights, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(rd, hbuf.data(), hbuf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        int64_t cap = (int64_t)c->num_cu * 4;
        if (c->design_grid_max > 0 && cap > c->design_grid_max) cap = c->design_grid_max;
        const int g = (int)(nseg < cap ? nseg : cap);
        const double *h0d = h0 ? hd : nullptr;
        switch (ndim) {
            case 1: design_update_go<1>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
            case 2: design_update_go<2>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
            case 3: design_update_go<3>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
            case 4: design_update_go<4>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
            case 5: design_update_go<5>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
            default: design_update_go<6>(c, g, P, tab, dtab, k, R, rd, h0d, wd, S, nseg, seglen, sv->d, c->partials); break;
        }
        PGD_LAUNCH_CHECK(c);
        PGD_TRY(seg_sum(c, c->partials, nseg, nv, nv, 1.0, c->work[6]));
        PGD_HIP(c, hipMemcpyAsync(out, c->work[6], (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the call
        return PGD_OK;
    });
    if (rc != PGD_OK) return rc;
    std::copy(out, out + nv, sums);
    return PGD_OK;
}

int pgd_design_gains(pgd_handle h, const double *a, int64_t M, int R, int k, const double *tables, const double *dtables, const int *n, int ndim,
                     const double *weights, pgd_handle stateh, double *gains) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (R < 1 || R > DS_RMAX)
        return fail(c, PGD_ERR_INVALID, "design_gains: R = %d rows per candidate, 1 .. %d are possible (group=\"entry\" makes every entry a candidate)", R, DS_RMAX);
    if (M < 1 || M >= ((int64_t)1 << 31)) return fail(c, PGD_ERR_INVALID, "design_gains: %lld candidates, 1 .. 2^31 - 1 are possible", (long long)M);
    if (!a || !gains) return fail(c, PGD_ERR_INVALID, "design_gains: a or gains missing");
    PostDims P;
    int64_t S = 0, ntab = 0, nw = 0;
    Vec *sv = nullptr;
    PGD_TRY(design_check(c, "design_gains", k, ndim, tables, dtables, n, weights, stateh, &P, &S, &ntab, &nw, &sv));

    int nseg = 1;
    int64_t seglen = 0;
    grid_segments(S, PO_SEGMIN, &nseg, &seglen);
    const bool mfma = c->design_variant != 0;
    const int kt = dense_kt(k);
    // ---- the candidates of a work item (enough items for the device, a tile per wave at least), those of a chunk of device scratch
    int64_t cc = (M * nseg / (2 * (int64_t)c->num_cu) + 63) / 64 * 64;
    cc = std::min<int64_t>(std::max<int64_t>(cc, DS_CHUNK_MIN), DS_CHUNK);
    int64_t chunk = DS_PART_MAX / nseg / cc * cc;
    if (chunk < cc) chunk = cc;
    const int64_t mp_max = std::min(chunk, (M + 15) / 16 * 16);
    const size_t na_max = mfma ? (size_t)R * (mp_max / 16) * kt * 64 : (size_t)std::min(chunk, M) * R * k;
    std::vector<double> ha(mfma ? na_max : 0, 0.0), res((size_t)M);
    const int rc = with_pool_input(c, pool_bytes(2 * (size_t)ntab + (size_t)nw + na_max), [&](void *p_in) -> int {
        PGD_TRY(ensure_work(c, 6, mp_max));
        PGD_TRY(ensure_partials(c, (int64_t)nseg * mp_max));
        double *tab = (double *)p_in, *dtab = tab + ntab, *wd = dtab + ntab, *ad = wd + nw;
        PGD_HIP(c, hipMemcpyAsync(tab, tables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(dtab, dtables, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice, c->stream));
        PGD_HIP(c, hipMemcpyAsync(wd, weights, (size_t)nw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        for (int64_t j0 = 0; j0 < M; j0 += chunk) {
            const int64_t cn = std::min(chunk, M - j0), Mp = (cn + 15) / 16 * 16;
            const int64_t plane = (Mp / 16) * kt * 64;
            if (mfma) {
                std::fill(ha.begin(), ha.begin() + (size_t)R * plane, 0.0);
                for (int r = 0; r < R; ++r) pack_a_fragments(ha.data() + (size_t)r * plane, kt, a + ((size_t)j0 * R + r) * k, cn, k, (size_t)R * k);
                PGD_HIP(c, hipMemcpyAsync(ad, ha.data(), (size_t)R * plane * sizeof(double), hipMemcpyHostToDevice, c->stream));
            } else {
                PGD_HIP(c, hipMemcpyAsync(ad, a + (size_t)j0 * R * k, (size_t)cn * R * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
            }
            DsArgs A;
            A.P = P; A.tab = tab; A.dtab = dtab; A.a = ad; A.wts = wd; A.state = sv->d;
            A.k = k; A.kt = kt; A.nseg = nseg; A.cc = (int)cc; A.ncc = (int)((Mp + cc - 1) / cc);
            A.plane = plane; A.S = S; A.seglen = seglen; A.M = cn; A.Mp = Mp; A.part = c->partials;
            switch (R) {
                case 1: PGD_TRY(design_launch_nd<1>(c, mfma, ndim, A)); break;
                case 2: PGD_TRY(design_launch_nd<2>(c, mfma, ndim, A)); break;
                default: PGD_TRY(design_launch_nd<3>(c, mfma, ndim, A)); break;
            }
            PGD_TRY(seg_sum(c, c->partials, nseg, Mp, cn, 0.5, c->work[6]));
            PGD_HIP(c, hipMemcpyAsync(res.data() + j0, c->work[6], (size_t)cn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the chunk
        }
        return PGD_OK;
    });
    if (rc != PGD_OK) return rc;
    std::copy(res.begin(), res.end(), gains);    // ---- the caller's array is written only now
    return PGD_OK;
}

}  // extern "C"
