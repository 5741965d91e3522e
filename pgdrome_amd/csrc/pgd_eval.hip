// Batched online evaluation of a PGD solution: U[n x S] = F[n x K] C[K x S] for S samples at once, with the
// reductions users want formed in the kernel that holds the accumulators (n S doubles cannot be stored at
// bench size).  The one DENSE product of this library, and so the one kernel on the matrix unit:
// v_mfma_f64_16x16x4_f64 with dofs on the fragment's column index (B = F^T, A = C^T; D rows are samples, D
// columns are dofs), which puts fragment loads and field stores on 16 consecutive doubles of one vector.
//
//   * F is read from HBM once per sample chunk: a workgroup owns a block of 16 T rows, stages the block's k
//     mode values in LDS (zero padded to a multiple of 4 in k and beyond row n), every wave takes its B
//     fragments from there into registers and loops over the sample tiles of the chunk.
//   * The four waves of a workgroup split the SAMPLE tiles (tile st belongs to wave st & 3 in every row block),
//     so a sample's running min / max in LDS has one owner and the sample loop has no barrier; the C^T
//     fragments come from a copy of the chunk's coefficients that the host lays out in fragment order (one
//     coalesced 512-byte load per k-step, served by L2: the chunk's coefficients are at most 2 MB).
//   * No atomics: workgroups are persistent (grid = resident capacity), each leaves one row of per-sample
//     partial extrema, k_eval_finish takes them in a fixed order.  Envelopes and exceedance counts are per row
//     and need no step across workgroups; across sample chunks they accumulate in the output vectors.
//   * Every u comes from one fixed accumulation chain over k, a min or a max does not depend on the order, the
//     counts are integers: every output is bit-identical for any grid size and any chunk length.
//   * max |u| of a sample is max(|min u|, |max u|) - exact, so only two extrema are carried.
//   * Rows beyond n and samples beyond s never enter a reduction (a padded zero would be the minimum of an
//     all-positive field).  NaNs in the modes or coefficients give unspecified statistics.
//
// k_eval_plain has the same outputs and rules with ordinary fma chains over k in ascending order: the
// cross-check of the tests and the baseline that shows what the matrix unit buys (PGD_TUNE_EVAL_VARIANT).
//
// Further down: the same two kernels on q planes per entry with a Euclidean norm before the reductions (pgd_eval_batch_norm),
// the kernel that makes such planes from a nodal P1 mode (pgd_cell_gradient), and the two norm kernels once more with the planes
// formed inside them from the nodal modes, never stored (pgd_eval_batch_grad), and the last two for nodal P2 modes at given points of
// every cell (pgd_cell_gradient_p2, pgd_eval_batch_grad_p2).  What happens to a value once it is formed is the same in all of
// them: see "the reduction epilogue" below.  What the value IS - the norm of the planes, one plane with its sign, an eigenvalue of
// the symmetric tensor they are - is a compile-time kind of those six kernels (pgd_eval_quantity, eval_eig).
#include "pgd_internal.h"

#include <cmath>
#include <limits>

namespace pgd {

constexpr int EVAL_KMAX = 256;
constexpr int EVAL_QMAX = 9;               // planes per mode of pgd_eval_batch_norm, rows of L of pgd_cell_gradient
constexpr int EVAL_CHUNK_DEFAULT = 1024;   // samples per launch: 16 KiB of running extrema in LDS beside the <= 32 KiB mode block
constexpr int64_t EVAL_SMAX = (int64_t)1 << 24;
constexpr int EVAL_PLAIN_TPB = 64;         // k_eval_plain: one wave per workgroup, one row per lane
constexpr int EVAL_PLAIN_NS = 8;           // ... and this many samples per pass over the block's mode values


struct EvalModes { const double *p[EVAL_KMAX]; };

struct EvalOut {
    double *part;       // per workgroup: min row, max row, cs16 doubles each
    double *env_min, *env_max, *exceed, *fields;
};

// entry (t, j) of the chunk's coefficients in fragment order: tile j >> 4, k-step t >> 2, lane 16 (t & 3) + (j & 15)
__device__ __forceinline__ int64_t eval_cf_index(int kt, int t, int j) {
    return ((int64_t)(j >> 4) * kt + (t >> 2)) * 64 + ((t & 3) << 4) + (j & 15);
}

template <int KT, int T>
__global__ __launch_bounds__(TPB) void k_eval_mfma(EvalModes M, int k, int64_t n, const double *__restrict__ cf, int cs,
                                                   int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int RB = 16 * T, KP = 4 * KT;
    const double INF = __builtin_huge_val();
    const int cs16 = (cs + 15) & ~15, ntile = cs16 >> 4;
    double *s_f = s_dyn;                 // KP x RB mode values of the row block
    double *s_mn = s_f + KP * RB;        // running per-sample extrema over this workgroup's rows
    double *s_mx = s_mn + cs16;
    double *s_env = s_mx + cs16;         // 4 waves x 3 x RB: per-row extrema / counts over each wave's samples
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    for (int j = threadIdx.x; j < cs16; j += TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    const int64_t nblk = (n + RB - 1) / RB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * RB;
        __syncthreads();                 // the last block's s_f and s_env are read; first pass: the extrema are initialised
        for (int idx = threadIdx.x; idx < KP * RB; idx += TPB) {
            const int t = idx / RB, d = idx - t * RB;
            const int64_t row = row0 + d;
            s_f[idx] = (t < k && row < n) ? M.p[t][row] : 0.0;
        }
        __syncthreads();
        double b[T][KT];
        bool rv[T];
        double emn[T], emx[T];
        int ecnt[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
#pragma unroll
            for (int q = 0; q < KT; ++q) b[j][q] = s_f[(4 * q + lq) * RB + 16 * j + lr];
            rv[j] = row0 + 16 * j + lr < n;
            emn[j] = INF; emx[j] = -INF; ecnt[j] = 0;
        }
        for (int st = wv; st < ntile; st += 4) {
            d4_t acc[T];
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = d4_t{0.0, 0.0, 0.0, 0.0};
            const double *cp = cf + (int64_t)st * KT * 64 + lane;
#pragma unroll
            for (int q = 0; q < KT; ++q) {
                const double a = cp[q * 64];
#pragma unroll
                for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j][q], acc[j], 0, 0, 0);
            }
            // lane holds D[lq + 4 r][lr]: sample 16 st + lq + 4 r of the chunk, row row0 + 16 j + lr
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int js = 16 * st + lq + 4 * r;
                const bool sv = js < cs;
                double mn = INF, mx = -INF;
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const double u = acc[j][r];
                    if (rv[j] && sv) {
                        mn = fmin(mn, u);
                        mx = fmax(mx, u);
                        emn[j] = fmin(emn[j], u);
                        emx[j] = fmax(emx[j], u);
                        ecnt[j] += (u > thr) ? 1 : 0;
                        if (want & PGD_EVAL_FIELDS) O.fields[(j0 + js) * n + (row0 + 16 * j + lr)] = u;
                    }
                }
                if (want & PGD_EVAL_STATS) {
#pragma unroll
                    for (int m = 1; m < 16; m <<= 1) {
                        mn = fmin(mn, __shfl_xor(mn, m, 64));
                        mx = fmax(mx, __shfl_xor(mx, m, 64));
                    }
                    if (lr == 0 && sv) { s_mn[js] = fmin(s_mn[js], mn); s_mx[js] = fmax(s_mx[js], mx); }
                }
            }
        }
        if (want & (PGD_EVAL_ENVELOPE | PGD_EVAL_EXCEED)) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
#pragma unroll
                for (int m = 16; m < 64; m <<= 1) {
                    emn[j] = fmin(emn[j], __shfl_xor(emn[j], m, 64));
                    emx[j] = fmax(emx[j], __shfl_xor(emx[j], m, 64));
                    ecnt[j] += __shfl_xor(ecnt[j], m, 64);
                }
                if (lq == 0) {
                    s_env[(wv * 3 + 0) * RB + 16 * j + lr] = emn[j];
                    s_env[(wv * 3 + 1) * RB + 16 * j + lr] = emx[j];
                    s_env[(wv * 3 + 2) * RB + 16 * j + lr] = (double)ecnt[j];
                }
            }
            __syncthreads();
            const int d = threadIdx.x;
            if (d < RB && row0 + d < n) {
                double mn = INF, mx = -INF, ct = 0.0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    mn = fmin(mn, s_env[(w * 3 + 0) * RB + d]);
                    mx = fmax(mx, s_env[(w * 3 + 1) * RB + d]);
                    ct += s_env[(w * 3 + 2) * RB + d];
                }
                const int64_t row = row0 + d;
                if (want & PGD_EVAL_ENVELOPE) {
                    O.env_min[row] = first ? mn : fmin(O.env_min[row], mn);
                    O.env_max[row] = first ? mx : fmax(O.env_max[row], mx);
                }
                if (want & PGD_EVAL_EXCEED) O.exceed[row] = first ? ct : O.exceed[row] + ct;
            }
        }
    }
    if (want & PGD_EVAL_STATS) {
        __syncthreads();
        for (int j = threadIdx.x; j < cs16; j += TPB) {
            O.part[((int64_t)blockIdx.x * 2 + 0) * cs16 + j] = s_mn[j];
            O.part[((int64_t)blockIdx.x * 2 + 1) * cs16 + j] = s_mx[j];
        }
    }
}

// ---- the reduction epilogue of k_eval_norm_mfma, k_eval_plain and k_eval_norm_plain, once per kernel family in inlined functions:
// the per-tile step (field store, per-sample extrema into s_mn / s_mx, the lane's per-row state), the per-row-block step (envelope
// and count into the output vectors, across sample chunks with `first`), the workgroup's row of partial extrema.  The norm kernels
// pass sqrt of the sum of squares where the signed one passes u.  k_eval_mfma above keeps the same text inline, so a change to the
// padding, NaN or chunk rule goes in there too: called, it was slower than its own run-to-run spread allows (K = 48, 256^3 rows, 256
// samples, medians of three runs: 16.65 ms inline, spread 0.04; 16.69 with the state in arrays by reference, 16.89 in a struct).

// row `row` over the samples of this chunk, combined with what the chunks before it left in the output vectors
__device__ __forceinline__ void eval_row_accumulate(const EvalOut &O, int64_t row, double mn, double mx, double ct, int want, int first) {
    if (want & PGD_EVAL_ENVELOPE) {
        O.env_min[row] = first ? mn : fmin(O.env_min[row], mn);
        O.env_max[row] = first ? mx : fmax(O.env_max[row], mx);
    }
    if (want & PGD_EVAL_EXCEED) O.exceed[row] = first ? ct : O.exceed[row] + ct;
}

// the workgroup's (NT threads) running per-sample extrema become its partial rows
template <int NT>
__device__ __forceinline__ void eval_store_partials(const EvalOut &O, const double *s_mn, const double *s_mx, int cs16, int want) {
    if (!(want & PGD_EVAL_STATS)) return;
    __syncthreads();
    for (int j = threadIdx.x; j < cs16; j += NT) {
        O.part[((int64_t)blockIdx.x * 2 + 0) * cs16 + j] = s_mn[j];
        O.part[((int64_t)blockIdx.x * 2 + 1) * cs16 + j] = s_mx[j];
    }
}

// Matrix-unit family, sample tile st of the chunk: lane (lq = lane >> 4, lr = lane & 15) holds D[lq + 4 r][lr] of every fragment, so
// v[j][r] is the value of sample 16 st + lq + 4 r of the chunk at row row0 + 16 j + lr.  The lane's state for these rows over the
// sample tiles of its wave: rv[j] (the row exists), emn[j], emx[j], ecnt[j] (values above the threshold).  A sample's extrema in
// s_mn / s_mx belong to the wave of its tile.
template <int T>
__device__ __forceinline__ void eval_tile_step(const d4_t (&v)[T], const bool (&rv)[T], double (&emn)[T], double (&emx)[T], int (&ecnt)[T],
                                               int st, int cs, int64_t j0, int64_t n, int64_t row0, int want, double thr, const EvalOut &O,
                                               double *s_mn, double *s_mx) {
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int js = 16 * st + lq + 4 * r;
        const bool sv = js < cs;
        double mn = INF, mx = -INF;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const double u = v[j][r];
            if (rv[j] && sv) {
                mn = fmin(mn, u);
                mx = fmax(mx, u);
                emn[j] = fmin(emn[j], u);
                emx[j] = fmax(emx[j], u);
                ecnt[j] += (u > thr) ? 1 : 0;
                if (want & PGD_EVAL_FIELDS) O.fields[(j0 + js) * n + (row0 + 16 * j + lr)] = u;
            }
        }
        if (want & PGD_EVAL_STATS) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                mn = fmin(mn, __shfl_xor(mn, m, 64));
                mx = fmax(mx, __shfl_xor(mx, m, 64));
            }
            if (lr == 0 && sv) { s_mn[js] = fmin(s_mn[js], mn); s_mx[js] = fmax(s_mx[js], mx); }
        }
    }
}

// After the sample tiles of a row block: the four sample groups lq of a wave, then the four waves through s_env (4 waves x 3 x RB)
template <int T>
__device__ __forceinline__ void eval_block_step(double (&emn)[T], double (&emx)[T], int (&ecnt)[T], double *s_env, int64_t row0, int64_t n,
                                                int want, int first, const EvalOut &O) {
    if (!(want & (PGD_EVAL_ENVELOPE | PGD_EVAL_EXCEED))) return;
    constexpr int RB = 16 * T;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
        for (int m = 16; m < 64; m <<= 1) {
            emn[j] = fmin(emn[j], __shfl_xor(emn[j], m, 64));
            emx[j] = fmax(emx[j], __shfl_xor(emx[j], m, 64));
            ecnt[j] += __shfl_xor(ecnt[j], m, 64);
        }
        if (lq == 0) {
            s_env[(wv * 3 + 0) * RB + 16 * j + lr] = emn[j];
            s_env[(wv * 3 + 1) * RB + 16 * j + lr] = emx[j];
            s_env[(wv * 3 + 2) * RB + 16 * j + lr] = (double)ecnt[j];
        }
    }
    __syncthreads();
    const int d = threadIdx.x;
    if (d < RB && row0 + d < n) {
        double mn = __builtin_huge_val(), mx = -__builtin_huge_val(), ct = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            mn = fmin(mn, s_env[(w * 3 + 0) * RB + d]);
            mx = fmax(mx, s_env[(w * 3 + 1) * RB + d]);
            ct += s_env[(w * 3 + 2) * RB + d];
        }
        eval_row_accumulate(O, row0 + d, mn, mx, ct, want, first);
    }
}

// One-wave kernels: one row per lane, EVAL_PLAIN_NS samples jb .. of the chunk per pass over the row's mode values (which stay in
// L1 / L2 between the passes).  The fma chains over k in ascending order, the mode values at M.p[t][at]:
template <int NS>
__device__ __forceinline__ void eval_plain_chains(const EvalModes &M, int k, int kt, const double *__restrict__ cf, int jb, bool rv, int64_t at,
                                                  double (&acc)[NS]) {
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = 0.0;
    for (int t = 0; t < k; ++t) {
        const double f = rv ? M.p[t][at] : 0.0;
        const double *cp = cf + eval_cf_index(kt, t, jb);
#pragma unroll
        for (int c = 0; c < NS; ++c) acc[c] = fma(cp[c], f, acc[c]);
    }
}

// ... and what becomes of the values v of samples jb .. at the lane's row (emn, emx, ect: the row's state over the chunk)
template <int NS>
__device__ __forceinline__ void eval_plain_step(const double (&v)[NS], int jb, int cs, int64_t j0, int64_t n, int64_t row, bool rv,
                                                int want, double thr, const EvalOut &O, double *s_mn, double *s_mx, double &emn,
                                                double &emx, double &ect) {
    const double INF = __builtin_huge_val();
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const int js = jb + c;
        if (js >= cs) break;                 // uniform
        const double u = v[c];
        double mn = INF, mx = -INF;
        if (rv) {
            mn = mx = u;
            emn = fmin(emn, u);
            emx = fmax(emx, u);
            ect += (u > thr) ? 1.0 : 0.0;
            if (want & PGD_EVAL_FIELDS) O.fields[(j0 + js) * n + row] = u;
        }
        if (want & PGD_EVAL_STATS) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                mn = fmin(mn, __shfl_xor(mn, m, 64));
                mx = fmax(mx, __shfl_xor(mx, m, 64));
            }
            if (threadIdx.x == 0) { s_mn[js] = fmin(s_mn[js], mn); s_mx[js] = fmax(s_mx[js], mx); }
        }
    }
}

// The same outputs as k_eval_mfma from ordinary fma chains
__global__ __launch_bounds__(EVAL_PLAIN_TPB) void k_eval_plain(EvalModes M, int k, int kt, int64_t n, const double *__restrict__ cf,
                                                               int cs, int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    const double INF = __builtin_huge_val();
    const int cs16 = (cs + 15) & ~15;
    double *s_mn = s_dyn, *s_mx = s_dyn + cs16;
    const int lane = threadIdx.x;
    for (int j = lane; j < cs16; j += EVAL_PLAIN_TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    __syncthreads();
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row = blk * EVAL_PLAIN_TPB + lane;
        const bool rv = row < n;
        double emn = INF, emx = -INF, ect = 0.0;
        for (int jb = 0; jb < cs16; jb += EVAL_PLAIN_NS) {
            double acc[EVAL_PLAIN_NS];
            eval_plain_chains(M, k, kt, cf, jb, rv, row, acc);
            eval_plain_step(acc, jb, cs, j0, n, row, rv, want, thr, O, s_mn, s_mx, emn, emx, ect);
        }
        if (rv) eval_row_accumulate(O, row, emn, emx, ect, want, first);
    }
    eval_store_partials<EVAL_PLAIN_TPB>(O, s_mn, s_mx, cs16, want);
}

// ---- norms of q linear quantities (pgd_eval_batch_norm): every mode is q planes of m entries, the value of entry e and sample j
// is v = sqrt(sum_i u_i^2), u_i = sum_t C[t][j] modes[t][i m + e].  Per plane the u_i are the accumulators of k_eval_mfma /
// k_eval_plain (one fixed chain over k each); the sum of squares starts from 0 and takes fma(u_i, u_i, .) over ascending i, so v
// does not depend on the grid, the chunk or the row block either.  Everything after v - extrema, envelopes, counts, fields - is the
// reduction epilogue with v in the place of u.
//
// k_eval_norm_mfma stages the q planes of a row block (q x 4 kt x RB values) and reloads the B fragment of plane i, k-step s from
// LDS inside the sample-tile loop (q x kt fragments do not fit the registers as the kt of k_eval_mfma do): one ds_read_b64 per MFMA,
// rows padded to 16 (mod 32) doubles so that the two 16-lane row groups of a half wave sit on opposite halves of the bank row.
// kt is a run-time value here.  LDSB = false reads the fragments from global memory instead (L2: a row block's values are read by
// every sample tile): the launcher's last resort where q planes of 16 rows do not fit 160 KiB.
//
// What becomes of the q combined planes u_0 .. u_{q-1} of an entry and sample is a compile-time kind QK (pgd_eval_quantity) of all six
// value kernels: PGD_EVAL_Q_NORM is the text above, PGD_EVAL_Q_VALUE (q = 1) passes u_0 on with its sign, the three EIG kinds keep
// all q planes of a tile in registers and reduce the symmetric tensor [xx, yy, zz, xy, yz, xz] (q = 4: yz = xz = 0) with eval_eig.
// The value depends on the u_i alone, so it is as independent of grid, chunk and row block as they are.
constexpr int EVAL_TENSOR_Q = 6;
constexpr bool eval_kind_is_tensor(int kind) { return kind >= PGD_EVAL_Q_EIG_MAX; }

// An extreme eigenvalue (or their difference) of a symmetric 3 x 3 tensor.  The three roots of the characteristic polynomial from
// its invariants are NOT used: acos is ill-conditioned at +-1, so where two eigenvalues nearly coincide (uniaxial stress in any
// frame) the angle is off by sqrt(u) and the close pair with it.  Instead only the root the angle gives well - the one away from
// the other two: the largest for det >= 0, the smallest otherwise - is taken from the angle, and only to find its eigenvector w:
// the largest cross product of two rows of C - lambda I.  The other two eigenvalues are those of C on the plane orthogonal to w
// (a 2 x 2 problem in an orthonormal pair a, b: mean +- radius, no cancellation), the isolated one is taken again as w' C w; errors
// of w enter all three in second order only.  C = (sigma - m I) / p with m = tr / 3, p^2 = |sigma - m I|_F^2 / 6 has eigenvalues
// in [-2, 2], so nothing here over- or underflows once p is formed; p = 0 (a multiple of the identity) gives m, m, m.
template <int QK>
__device__ __forceinline__ double eval_eig(double xx, double yy, double zz, double xy, double yz, double xz) {
    static_assert(QK == PGD_EVAL_Q_EIG_MAX || QK == PGD_EVAL_Q_EIG_MIN || QK == PGD_EVAL_Q_EIG_SPREAD, "an eigenvalue kind");
    const double m = (xx + yy + zz) / 3.0;
    const double bx = xx - m, by = yy - m, bz = zz - m;
    const double p = sqrt((bx * bx + by * by + bz * bz + 2.0 * (xy * xy + yz * yz + xz * xz)) / 6.0);
    const double inv = p > 0.0 ? 1.0 / p : 0.0;
    const double cx = bx * inv, cy = by * inv, cz = bz * inv, cxy = xy * inv, cyz = yz * inv, cxz = xz * inv;
    const double det = cx * (cy * cz - cyz * cyz) - cxy * (cxy * cz - cyz * cxz) + cxz * (cxy * cyz - cy * cxz);
    const double h = fmin(fmax(0.5 * det, -1.0), 1.0);
    const double th = acos(h) / 3.0;
    const double lam = 2.0 * cos(h >= 0.0 ? th : th + 2.0943951023931954923);      // (2 pi / 3)
    // rows of C - lam I and their cross products
    const double r0x = cx - lam, r1y = cy - lam, r2z = cz - lam;
    const double u0 = cxy * cyz - cxz * r1y, u1 = cxz * cxy - r0x * cyz, u2 = r0x * r1y - cxy * cxy;          // r0 x r1
    const double v0 = r1y * r2z - cyz * cyz, v1 = cyz * cxz - cxy * r2z, v2 = cxy * cyz - r1y * cxz;          // r1 x r2
    const double t0 = cyz * cxz - r2z * cxy, t1 = r2z * r0x - cxz * cxz, t2 = cxz * cxy - cyz * r0x;          // r2 x r0
    const double nu = u0 * u0 + u1 * u1 + u2 * u2, nv = v0 * v0 + v1 * v1 + v2 * v2, nt = t0 * t0 + t1 * t1 + t2 * t2;
    double w0 = u0, w1 = u1, w2 = u2, nw = nu;
    if (nv > nw) { w0 = v0; w1 = v1; w2 = v2; nw = nv; }
    if (nt > nw) { w0 = t0; w1 = t1; w2 = t2; nw = nt; }
    if (nw > 0.0) {
        const double s = 1.0 / sqrt(nw);
        w0 *= s; w1 *= s; w2 *= s;
    } else {
        w0 = 1.0; w1 = 0.0; w2 = 0.0;
    }
    // a orthogonal to w from the larger of |w0|, |w1|; b = w x a
    const bool f = fabs(w0) >= fabs(w1);
    const double s = 1.0 / sqrt(f ? w0 * w0 + w2 * w2 : w1 * w1 + w2 * w2);
    const double a0 = f ? -w2 * s : 0.0, a1 = f ? 0.0 : w2 * s, a2 = f ? w0 * s : -w1 * s;
    const double b0 = w1 * a2 - w2 * a1, b1 = w2 * a0 - w0 * a2, b2 = w0 * a1 - w1 * a0;
    const double ca0 = cx * a0 + cxy * a1 + cxz * a2, ca1 = cxy * a0 + cy * a1 + cyz * a2, ca2 = cxz * a0 + cyz * a1 + cz * a2;
    const double cb0 = cx * b0 + cxy * b1 + cxz * b2, cb1 = cxy * b0 + cy * b1 + cyz * b2, cb2 = cxz * b0 + cyz * b1 + cz * b2;
    const double cw0 = cx * w0 + cxy * w1 + cxz * w2, cw1 = cxy * w0 + cy * w1 + cyz * w2, cw2 = cxz * w0 + cyz * w1 + cz * w2;
    const double m00 = a0 * ca0 + a1 * ca1 + a2 * ca2, m11 = b0 * cb0 + b1 * cb1 + b2 * cb2, m01 = a0 * cb0 + a1 * cb1 + a2 * cb2;
    const double mid = 0.5 * (m00 + m11), hd = 0.5 * (m00 - m11);
    const double rad = sqrt(hd * hd + m01 * m01);          // (entries of a matrix of norm <= 2: no scaling as in hypot is needed)
    const double iso = w0 * cw0 + w1 * cw1 + w2 * cw2;
    const double emx = fmax(iso, mid + rad), emn = fmin(iso, mid - rad);
    if constexpr (QK == PGD_EVAL_Q_EIG_MAX) return m + p * emx;
    else if constexpr (QK == PGD_EVAL_Q_EIG_MIN) return m + p * emn;
    else return p * (emx - emn);
}

template <int T>
struct EvalNormShape {
    static constexpr int RB = 16 * T;
    static constexpr int RS = RB + (T == 1 ? 0 : 16);      // row stride of the staged values in doubles
};

// A row block of the matrix-unit norm kernels once its B fragments are where they are read (s_f staged and the barrier passed, or
// global memory): the sample tiles of this wave, then the per-row step.  Whatever filled s_f, from here on the kernels are one text.
template <int T, bool LDSB, int QK>
__device__ __forceinline__ void eval_norm_tiles(const EvalModes &M, int k, int kt, int q, int64_t n, const double *__restrict__ cf, int cs,
                                                int64_t j0, int want, int first, double thr, const EvalOut &O, const double *s_f,
                                                double *s_mn, double *s_mx, double *s_env, int64_t row0) {
    constexpr int RS = EvalNormShape<T>::RS;
    const double INF = __builtin_huge_val();
    const int kp = 4 * kt, ntile = ((cs + 15) & ~15) >> 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    bool rv[T];
    double emn[T], emx[T];
    int ecnt[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        rv[j] = row0 + 16 * j + lr < n;
        emn[j] = INF; emx[j] = -INF; ecnt[j] = 0;
    }
    for (int st = wv; st < ntile; st += 4) {
        const double *cp = cf + (int64_t)st * kt * 64 + lane;
        // the combined plane i of this tile: one fixed chain over the k-steps per accumulator
        auto plane = [&](int i, d4_t (&acc)[T]) {
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = d4_t{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < kt; ++s) {
                const double a = cp[s * 64];
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    double b;
                    if (LDSB) {
                        b = s_f[(i * kp + 4 * s + lq) * RS + 16 * j + lr];
                    } else {
                        const int t = 4 * s + lq;
                        b = (t < k && rv[j]) ? M.p[t][(int64_t)i * n + row0 + 16 * j + lr] : 0.0;
                    }
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
                }
            }
        };
        d4_t v[T];
        if constexpr (QK == PGD_EVAL_Q_NORM) {
            d4_t ss[T];
#pragma unroll
            for (int j = 0; j < T; ++j) ss[j] = d4_t{0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < q; ++i) {
                d4_t acc[T];
                plane(i, acc);
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss[j][r] = fma(acc[j][r], acc[j][r], ss[j][r]);
            }
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[j][r] = sqrt(ss[j][r]);
        } else if constexpr (QK == PGD_EVAL_Q_VALUE) {
            plane(0, v);
        } else {
            d4_t u[EVAL_TENSOR_Q][T];                  // all planes of the tile at once: 8 q T registers
#pragma unroll
            for (int i = 0; i < EVAL_TENSOR_Q; ++i) {
                if (i < q) {
                    plane(i, u[i]);
                } else {
#pragma unroll
                    for (int j = 0; j < T; ++j) u[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
                }
            }
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[j][r] = eval_eig<QK>(u[0][j][r], u[1][j][r], u[2][j][r], u[3][j][r], u[4][j][r], u[5][j][r]);
        }
        eval_tile_step<T>(v, rv, emn, emx, ecnt, st, cs, j0, n, row0, want, thr, O, s_mn, s_mx);
    }
    eval_block_step<T>(emn, emx, ecnt, s_env, row0, n, want, first, O);
}

template <int T, bool LDSB, int QK>
__global__ __launch_bounds__(TPB) void k_eval_norm_mfma(EvalModes M, int k, int kt, int q, int64_t n, const double *__restrict__ cf, int cs,
                                                        int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int RB = EvalNormShape<T>::RB, RS = EvalNormShape<T>::RS;
    const double INF = __builtin_huge_val();
    const int kp = 4 * kt;
    const int cs16 = (cs + 15) & ~15;
    double *s_f = s_dyn;                                   // q x kp rows of RS: plane i, mode t at row i kp + t
    double *s_mn = s_f + (LDSB ? (size_t)q * kp * RS : 0);
    double *s_mx = s_mn + cs16;
    double *s_env = s_mx + cs16;
    for (int j = threadIdx.x; j < cs16; j += TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    const int64_t nblk = (n + RB - 1) / RB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * RB;
        __syncthreads();
        if (LDSB) {
            for (int idx = threadIdx.x; idx < q * kp * RB; idx += TPB) {
                const int pt = idx / RB, d = idx - pt * RB;
                const int i = pt / kp, t = pt - i * kp;
                const int64_t row = row0 + d;
                s_f[pt * RS + d] = (t < k && row < n) ? M.p[t][(int64_t)i * n + row] : 0.0;
            }
        }
        __syncthreads();
        eval_norm_tiles<T, LDSB, QK>(M, k, kt, q, n, cf, cs, j0, want, first, thr, O, s_f, s_mn, s_mx, s_env, row0);
    }
    eval_store_partials<TPB>(O, s_mn, s_mx, cs16, want);
}

// Samples per pass of the plain kernels of a kind: the eigenvalue kinds hold q planes per sample and the temporaries of eval_eig
constexpr int eval_plain_ns(int kind) { return eval_kind_is_tensor(kind) ? EVAL_PLAIN_NS / 2 : EVAL_PLAIN_NS; }

// The plain kernels that hold all planes of a pass (u[i][c]: plane i, sample c; planes from q on are zero): the values of a kind
// other than the norm, whose text stays where it was
template <int QK, int NS>
__device__ __forceinline__ void eval_plain_values(const double (&u)[EVAL_QMAX][NS], int q, double (&v)[NS]) {
    if constexpr (QK == PGD_EVAL_Q_VALUE) {
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] = u[0][c];
    } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) v[c] = eval_eig<QK>(u[0][c], u[1][c], u[2][c], u[3][c], u[4][c], u[5][c]);
    }
}

// k_eval_plain with the loop over the planes around its fma chains
template <int QK>
__global__ __launch_bounds__(EVAL_PLAIN_TPB) void k_eval_norm_plain(EvalModes M, int k, int kt, int q, int64_t n, const double *__restrict__ cf,
                                                                    int cs, int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int NS = eval_plain_ns(QK);
    const double INF = __builtin_huge_val();
    const int cs16 = (cs + 15) & ~15;
    double *s_mn = s_dyn, *s_mx = s_dyn + cs16;
    const int lane = threadIdx.x;
    for (int j = lane; j < cs16; j += EVAL_PLAIN_TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    __syncthreads();
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row = blk * EVAL_PLAIN_TPB + lane;
        const bool rv = row < n;
        double emn = INF, emx = -INF, ect = 0.0;
        for (int jb = 0; jb < cs16; jb += NS) {
            double ss[NS];
            if constexpr (QK == PGD_EVAL_Q_NORM) {
                double acc[NS];
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = 0.0;
                for (int i = 0; i < q; ++i) {
                    eval_plain_chains(M, k, kt, cf, jb, rv, (int64_t)i * n + row, acc);
#pragma unroll
                    for (int c = 0; c < NS; ++c) ss[c] = fma(acc[c], acc[c], ss[c]);
                }
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = sqrt(ss[c]);            // from here on the values
            } else if constexpr (QK == PGD_EVAL_Q_VALUE) {
                eval_plain_chains(M, k, kt, cf, jb, rv, row, ss);
            } else {
                double u[EVAL_QMAX][NS];
#pragma unroll
                for (int i = 0; i < EVAL_TENSOR_Q; ++i) {
                    if (i < q) {
                        eval_plain_chains(M, k, kt, cf, jb, rv, (int64_t)i * n + row, u[i]);
                    } else {
#pragma unroll
                        for (int c = 0; c < NS; ++c) u[i][c] = 0.0;
                    }
                }
                eval_plain_values<QK>(u, q, ss);
            }
            eval_plain_step(ss, jb, cs, j0, n, row, rv, want, thr, O, s_mn, s_mx, emn, emx, ect);
        }
        if (rv) eval_row_accumulate(O, row, emn, emx, ect, want, first);
    }
    eval_store_partials<EVAL_PLAIN_TPB>(O, s_mn, s_mx, cs16, want);
}

// Final pass: sample j of the chunk takes the g workgroups' partial extrema in a fixed order (a thread per sample,
// coalesced across samples); stats = 3 rows of s_total doubles: min, max, max |.|
__global__ __launch_bounds__(TPB) void k_eval_finish(const double *__restrict__ part, int g, int cs, double *__restrict__ stats,
                                                     int64_t j0, int64_t s_total) {
    const int cs16 = (cs + 15) & ~15;
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= cs) return;
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (int b = 0; b < g; ++b) {
        mn = fmin(mn, part[((int64_t)b * 2 + 0) * cs16 + j]);
        mx = fmax(mx, part[((int64_t)b * 2 + 1) * cs16 + j]);
    }
    stats[j0 + j] = mn;
    stats[s_total + j0 + j] = mx;
    stats[2 * s_total + j0 + j] = fmax(fabs(mn), fabs(mx));
}

// (the matrix-unit kernels are persistent over the row blocks of a call: launch_persistent with the occupancy the runtime reports)
template <int KT, int T>
static int eval_launch_mfma(Ctx *c, const EvalModes &M, int k, int64_t n, const double *cf, int cs, int64_t j0, int want,
                            int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const int cs16 = (cs + 15) & ~15;
    const size_t lds = ((size_t)4 * KT * 16 * T + 2 * (size_t)cs16 + 12 * 16 * T) * sizeof(double);
    return launch_persistent(c, k_eval_mfma<KT, T>, TPB, lds, (n + 16 * T - 1) / (16 * T), grid_cap, 0, grid_out, M, k, n, cf, cs, j0, want,
                                  first, thr, O);
}

// ---- k_eval_norm_mfma: the row block and where the B fragments come from, chosen once per call
constexpr size_t EVAL_LDS_PLAIN = 64 * 1024;      // dynamic LDS a kernel may ask for as it is; up to EVAL_LDS_MAX with the function attribute
constexpr size_t EVAL_LDS_MAX = 160 * 1024;

struct EvalNormCfg { int t = 1; bool ldsb = false; };

static size_t eval_norm_lds(int t, bool ldsb, int q, int kt, int cs16) {
    const size_t rb = 16 * (size_t)t, rs = rb + (t == 1 ? 0 : 16);
    return ((ldsb ? (size_t)q * 4 * kt * rs : 0) + 2 * (size_t)cs16 + 12 * rb) * sizeof(double);
}

// (the attribute belongs to one instantiation: every kernel that may run with more than 64 KiB raises its own)
static bool eval_raise_lds(const void *kern, size_t lds) {
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

template <int QK>
static bool eval_norm_raise_lds(size_t lds) { return eval_raise_lds((const void *)k_eval_norm_mfma<1, true, QK>, lds); }

// The eigenvalue kinds hold the q accumulator tiles of a sample tile at once (8 q T registers where the norm holds 8 T and a sum)
// beside the temporaries of eval_eig: their kernels exist for 16 rows per workgroup (about 200 vector registers, two workgroups
// per CU; 32 rows took 300, one wave per SIMD).  No vector register is spilled; scalar registers are - the constants of acos and
// cos are hoisted out of the sample loop, and in the fused kernels L arrives by value - DESIGN.md has the counts per kernel
constexpr int eval_kind_tmax(int kind) { return eval_kind_is_tensor(kind) ? 1 : 4; }

// 64, 32 or 16 rows per workgroup (from 16 tmax down), the largest whose q planes fit 64 KiB beside the extrema; else 16 rows in up
// to 160 KiB (the function attribute is raised for it, by `raise`: the 16-row kernel of the caller); else 16 rows with the
// fragments read from global memory, which the fused kernels do not have: they refuse
static EvalNormCfg eval_norm_choose(int q, int kt, int cs16_max, int tmax, bool (*raise)(size_t)) {
    EvalNormCfg cfg;
    for (int t = tmax; t >= 1; t >>= 1)
        if (eval_norm_lds(t, true, q, kt, cs16_max) <= EVAL_LDS_PLAIN) { cfg.t = t; cfg.ldsb = true; return cfg; }
    const size_t lds = eval_norm_lds(1, true, q, kt, cs16_max);
    if (lds <= EVAL_LDS_MAX && raise(lds)) cfg.ldsb = true;
    return cfg;
}

template <int T, bool LDSB, int QK>
static int eval_launch_norm(Ctx *c, const EvalModes &M, int k, int kt, int q, int64_t n, const double *cf, int cs, int64_t j0, int want,
                            int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const size_t lds = eval_norm_lds(T, LDSB, q, kt, (cs + 15) & ~15);
    return launch_persistent(c, k_eval_norm_mfma<T, LDSB, QK>, TPB, lds, (n + 16 * T - 1) / (16 * T), grid_cap, 0, grid_out, M, k, kt, q, n, cf,
                                  cs, j0, want, first, thr, O);
}

// One sample chunk of the stored planes with the kind's kernels: plain, or the matrix unit as cfg says
template <int QK>
static int eval_launch_norm_kind(Ctx *c, bool mfma, const EvalNormCfg &cfg, const EvalModes &M, int k, int kt, int q, int64_t n,
                                 const double *cf, int cs, int64_t j0, int want, int first, double thr, const EvalOut &O, int grid_cap,
                                 int *grid_out) {
    if (!mfma) {
        const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
        const int g = (int)(nblk < grid_cap ? nblk : grid_cap);
        const size_t lds = (size_t)2 * ((cs + 15) & ~15) * sizeof(double);
        k_eval_norm_plain<QK><<<g, EVAL_PLAIN_TPB, lds, c->stream>>>(M, k, kt, q, n, cf, cs, j0, want, first, thr, O);
        PGD_LAUNCH_CHECK(c);
        *grid_out = g;
        return PGD_OK;
    }
    if (!cfg.ldsb) return eval_launch_norm<1, false, QK>(c, M, k, kt, q, n, cf, cs, j0, want, first, thr, O, grid_cap, grid_out);
    if constexpr (eval_kind_tmax(QK) >= 4) {
        if (cfg.t == 4) return eval_launch_norm<4, true, QK>(c, M, k, kt, q, n, cf, cs, j0, want, first, thr, O, grid_cap, grid_out);
        if (cfg.t == 2) return eval_launch_norm<2, true, QK>(c, M, k, kt, q, n, cf, cs, j0, want, first, thr, O, grid_cap, grid_out);
    }
    return eval_launch_norm<1, true, QK>(c, M, k, kt, q, n, cf, cs, j0, want, first, thr, O, grid_cap, grid_out);
}

typedef int (*eval_norm_launch_t)(Ctx *, bool, const EvalNormCfg &, const EvalModes &, int, int, int, int64_t, const double *, int, int64_t,
                                  int, int, double, const EvalOut &, int, int *);
struct EvalNormFns { eval_norm_launch_t launch; bool (*raise)(size_t); };

template <int QK>
static EvalNormFns eval_norm_fns() { return {eval_launch_norm_kind<QK>, eval_norm_raise_lds<QK>}; }

static EvalNormFns eval_norm_pick(int kind) {
    switch (kind) {
        case PGD_EVAL_Q_VALUE: return eval_norm_fns<PGD_EVAL_Q_VALUE>();
        case PGD_EVAL_Q_EIG_MAX: return eval_norm_fns<PGD_EVAL_Q_EIG_MAX>();
        case PGD_EVAL_Q_EIG_MIN: return eval_norm_fns<PGD_EVAL_Q_EIG_MIN>();
        case PGD_EVAL_Q_EIG_SPREAD: return eval_norm_fns<PGD_EVAL_Q_EIG_SPREAD>();
        default: return eval_norm_fns<PGD_EVAL_Q_NORM>();
    }
}

static size_t eval_round(size_t bytes) { return (bytes + 65535) & ~(size_t)65535; }   // (whole 64 KiB: the pool takes them back)

void eval_release(Ctx *c) {
    if (c->eval_pin) (void)hipHostFree(c->eval_pin);
    c->eval_pin = nullptr;
    c->eval_pin_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        if (c->eval_ev[i]) (void)hipEventDestroy(c->eval_ev[i]);
        c->eval_ev[i] = nullptr;
        c->eval_ev_set[i] = false;
    }
}

// ---- pgd_cell_gradient: a nodal P1 mode to q cell-wise planes, out[i nc + e] = scale[e] sum_j L[i][j] g[j] with
// g[c G + a] = d u_c / d x_a on cell e (constant there).  A thread per cell: the int4 record, the vertices' coordinates (SoA) and
// the (G + 1) NC nodal values are gathered, the inverse of the edge matrix comes from its cofactors and determinant in registers -
// nothing is taken from the lattice description, so any mesh the layout accepts is right.  With x = x_0 + E^T xi (row a of E: the
// edge x_{a+1} - x_0) the basis function of vertex a + 1 is xi_a, so d u / d x_d = sum_a (u_{a+1} - u_0) inv(E^T)[a][d].
// L arrives by value.  No atomics; the stores of a plane are coalesced.
struct GradL { double a[EVAL_QMAX * EVAL_QMAX]; };      // row-major q x qin

// The per-cell arithmetic of k_cell_gradient and of the fused kernels further down, in two steps because the fused kernels walk many
// modes on one cell: cell_inverse (the record's used entries, the edge matrix, the cofactor inverse - once per cell) and cell_planes
// (du, g, L g and the scale - once per cell and mode; `put(i, value)` takes plane i).  The loop over the planes is unrolled to
// EVAL_QMAX with a guard, so a caller that keeps the planes in registers can.
template <int G>
__device__ __forceinline__ void cell_inverse(const int4 rec, const double *__restrict__ coords, int64_t nv, int (&v)[4], double (&J)[G][G]) {
    v[0] = rec.x; v[1] = rec.y; v[2] = rec.z; v[3] = rec.w;      // (entries above G are unused lanes of the record: never an index)
    double E[G][G];                                  // E[a][d] = x_{a+1}[d] - x_0[d]
#pragma unroll
    for (int d = 0; d < G; ++d) {
        const double *x = coords + (int64_t)d * nv;
        const double x0 = x[v[0]];
#pragma unroll
        for (int a = 0; a < G; ++a) E[a][d] = x[v[a + 1]] - x0;
    }
    // J[a][d] = d xi_a / d x_d: the inverse of E^T
    if constexpr (G == 1) {
        J[0][0] = 1.0 / E[0][0];
    } else if constexpr (G == 2) {
        const double inv = 1.0 / (E[0][0] * E[1][1] - E[0][1] * E[1][0]);
        J[0][0] = E[1][1] * inv;  J[0][1] = -E[1][0] * inv;
        J[1][0] = -E[0][1] * inv; J[1][1] = E[0][0] * inv;
    } else {
        double C[3][3];                              // cofactor of E[a][d]
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
                C[a][d] = E[a1][d1] * E[a2][d2] - E[a1][d2] * E[a2][d1];
            }
        }
        const double inv = 1.0 / (E[0][0] * C[0][0] + E[0][1] * C[0][1] + E[0][2] * C[0][2]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) J[a][d] = C[a][d] * inv;      // inv(E)[d][a] = C[a][d] / det, and J = inv(E^T) = inv(E)^T
    }
}

// (the tail of cell_planes from du on - g, L g, the scale - which the P2 kernels further down share: du[c][a] is d u_c / d xi_a)
template <int G, int NC, class Put>
__device__ __forceinline__ void grad_planes(const double (&du)[NC][G], const double (&J)[G][G], const GradL &L, int q, double sc, Put put) {
    double g[NC * G];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int d = 0; d < G; ++d) {
            double acc = du[c][0] * J[0][d];
#pragma unroll
            for (int a = 1; a < G; ++a) acc = fma(du[c][a], J[a][d], acc);
            g[c * G + d] = acc;
        }
    }
#pragma unroll
    for (int i = 0; i < EVAL_QMAX; ++i) {
        if (i < q) {
            const double *row = L.a + i * (NC * G);
            double acc = row[0] * g[0];
#pragma unroll
            for (int j = 1; j < NC * G; ++j) acc = fma(row[j], g[j], acc);
            put(i, sc * acc);
        }
    }
}

template <int G, int NC, class Put>
__device__ __forceinline__ void cell_planes(const int (&v)[4], const double (&J)[G][G], const double *__restrict__ u, const GradL &L, int q,
                                            double sc, Put put) {
    double du[NC][G];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double u0 = u[(int64_t)v[0] * NC + c];
#pragma unroll
        for (int a = 0; a < G; ++a) du[c][a] = u[(int64_t)v[a + 1] * NC + c] - u0;
    }
    grad_planes<G, NC>(du, J, L, q, sc, put);
}

template <int G, int NC>
__global__ __launch_bounds__(TPB) void k_cell_gradient(const int4 *__restrict__ cells, const double *__restrict__ coords, int64_t nv, int64_t nc,
                                                       const double *__restrict__ u, GradL L, int q, const double *__restrict__ scale,
                                                       double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= nc) return;
    int v[4];
    double J[G][G];
    cell_inverse<G>(cells[e], coords, nv, v, J);
    cell_planes<G, NC>(v, J, u, L, q, scale ? scale[e] : 1.0, [&](int i, double p) { out[(int64_t)i * nc + e] = p; });
}

template <int G, int NC>
static void cell_gradient_launch(Ctx *c, const Mesh *b, const double *u, const GradL &L, int q, const double *scale, double *out) {
    const int grid = (int)((b->nc + TPB - 1) / TPB);
    k_cell_gradient<G, NC><<<grid, TPB, 0, c->stream>>>(b->cells, b->coords, b->nv, b->nc, u, L, q, scale, out);
}

// ---- pgd_cell_gradient_p2: the same planes of a nodal P2 mode, taken at npt <= 4 points of every cell given by their barycentric
// coordinates lam (npt x (G + 1)): the gradient of a P2 field is affine on the cell, so the caller says where.  Entries are
// point-major, out[(i npt + a) nc + e] is plane i at point a of cell e: q planes of npt nc entries, what pgd_eval_batch_norm takes.
// The record is the frontend's: the G + 1 vertices, then the edge nodes in the order of p2_edge.  With N_i = l_i (2 l_i - 1) and
// N_ab = 4 l_a l_b, d u / d l_i = u_i (4 l_i - 1) + sum over the edges (i, b) of 4 u_ib l_b =: dl_i, and with l_0 = 1 - sum xi
// d u / d xi_a = dl_{a+1} - dl_0: the du of the P1 kernels, so g, L g and the scale are grad_planes.  The Jacobian comes from the
// vertices alone (the cells are straight): cell_inverse on the first G + 1 entries of the record.
constexpr int P2_NPT_MAX = 4;
struct P2Points { double lam[P2_NPT_MAX * 4]; int npt; };

__host__ __device__ constexpr int p2_nodes(int G) { return (G + 1) * (G + 2) / 2; }
// local edge k of a P2 triangle ((1,2), (0,2), (0,1)) or tetrahedron ((2,3), (1,3), (1,2), (0,3), (0,2), (0,1)): its two vertices
__host__ __device__ constexpr int p2_edge_a(int G, int k) { return G == 2 ? (k == 0 ? 1 : 0) : (k == 0 ? 2 : k < 3 ? 1 : 0); }
__host__ __device__ constexpr int p2_edge_b(int G, int k) { return G == 2 ? (k == 2 ? 1 : 2) : (k == 2 || k == 4 ? 2 : k == 5 ? 1 : 3); }

// the record of cell e, its vertices as the int4 of cell_inverse
template <int G>
__device__ __forceinline__ int4 p2_record(const int *__restrict__ cellsN, int64_t e, int (&r)[p2_nodes(G)]) {
    const int *rec = cellsN + e * p2_nodes(G);
#pragma unroll
    for (int j = 0; j < p2_nodes(G); ++j) r[j] = rec[j];
    return make_int4(r[0], r[1], r[2], G == 3 ? r[3] : 0);
}

// the nodal values of the cell, un[j NC + c] = component c at record entry j
template <int G, int NC>
__device__ __forceinline__ void p2_gather(const int (&r)[p2_nodes(G)], const double *__restrict__ u, double (&un)[p2_nodes(G) * NC]) {
#pragma unroll
    for (int j = 0; j < p2_nodes(G); ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) un[j * NC + c] = u[(int64_t)r[j] * NC + c];
}

// w_i = 4 l_i - 1 and l4_i = 4 l_i of point a (a select over the <= 4 points: the table stays in the kernel arguments)
template <int G>
__device__ __forceinline__ void p2_weights(const P2Points &P, int a, double (&w)[G + 1], double (&l4)[G + 1]) {
#pragma unroll
    for (int i = 0; i <= G; ++i) {
        double l = P.lam[i];
#pragma unroll
        for (int b = 1; b < P2_NPT_MAX; ++b) l = (a == b) ? P.lam[b * (G + 1) + i] : l;
        l4[i] = 4.0 * l;
        w[i] = l4[i] - 1.0;
    }
}

// the planes at one point.  du_a = dl_{a+1} - dl_0 with the one node both share, the edge (0, a + 1), taken out of the two sums and
// added as u_e (4 l_0 - 4 l_{a+1}): its two terms cancel (entirely at the barycentre), and summed apart they would leave rounding
// errors of the size of the terms, not of their difference.  So every du is off by a few units relative to
// sum_j |d N_j / d xi_a| |u_j|.  Order: the vertex's own term, then its edges in record order; vertex a + 1 minus vertex 0; the
// shared edge last.
template <int G, int NC, class Put>
__device__ __forceinline__ void p2_planes(const double (&un)[p2_nodes(G) * NC], const double (&w)[G + 1], const double (&l4)[G + 1],
                                          const double (&J)[G][G], const GradL &L, int q, double sc, Put put) {
    double du[NC][G];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int a = 0; a < G; ++a) {
            double hi = un[(a + 1) * NC + c] * w[a + 1], lo = un[c] * w[0], shared = 0.0;
#pragma unroll
            for (int k = 0; k < p2_nodes(G) - (G + 1); ++k) {
                const int ea = p2_edge_a(G, k), eb = p2_edge_b(G, k);      // ea < eb
                const double ue = un[(G + 1 + k) * NC + c];
                if (ea == 0 && eb == a + 1) shared = ue;
                else if (ea == 0) lo = fma(ue, l4[eb], lo);
                else if (ea == a + 1) hi = fma(ue, l4[eb], hi);
                else if (eb == a + 1) hi = fma(ue, l4[ea], hi);
            }
            du[c][a] = fma(shared, l4[0] - l4[a + 1], hi - lo);
        }
    }
    grad_planes<G, NC>(du, J, L, q, sc, put);
}

// A thread per cell: record, inverse and nodal values once, in registers; then the points.  The stores of a plane are coalesced.
template <int G, int NC>
__global__ __launch_bounds__(TPB) void k_cell_gradient_p2(const int *__restrict__ cellsN, const double *__restrict__ coords, int64_t nv,
                                                          int64_t nc, const double *__restrict__ u, P2Points P, GradL L, int q,
                                                          const double *__restrict__ scale, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= nc) return;
    int r[p2_nodes(G)], v[4];
    double J[G][G], un[p2_nodes(G) * NC];
    cell_inverse<G>(p2_record<G>(cellsN, e, r), coords, nv, v, J);
    p2_gather<G, NC>(r, u, un);
    const double sc = scale ? scale[e] : 1.0;
    for (int a = 0; a < P.npt; ++a) {
        double w[G + 1], l4[G + 1];
        p2_weights<G>(P, a, w, l4);
        p2_planes<G, NC>(un, w, l4, J, L, q, sc, [&](int i, double p) { out[((int64_t)i * P.npt + a) * nc + e] = p; });
    }
}

template <int G, int NC>
static void cell_gradient_p2_launch(Ctx *c, const Mesh *b, const double *u, const P2Points &P, const GradL &L, int q, const double *scale,
                                    double *out) {
    const int grid = (int)((b->nc + TPB - 1) / TPB);
    k_cell_gradient_p2<G, NC><<<grid, TPB, 0, c->stream>>>(b->cellsN, b->coords, b->nv, b->nc, u, P, L, q, scale, out);
}

// ---- pgd_eval_batch_grad: pgd_eval_batch_norm on planes that are never stored.  The planes of a cell are a local, linear function
// of the nodal mode (cell_inverse once, cell_planes per mode), so the kernels form them where the stored path reads them: the
// matrix-unit kernel in the staging step of a row block of cells (then it IS k_eval_norm_mfma: eval_norm_tiles), the plain kernel in
// front of its fma chains.  The nodal values are gathers through the cell record - each node is referenced by every cell around it,
// so they come from L2 / L1 rather than HBM - and every sample chunk gathers again.  The scalar layout holds cells and coordinates;
// nodal values sit at node * NC + c.  Cells beyond nc read no record and stage zeros, as the mode rows k <= t < kp do.
struct EvalGradSrc {
    const int4 *cells;
    const double *coords, *scale;      // scale: one entry per cell, or null
    int64_t nv;
    GradL L;
};
// ... and what the P2 kernels take: the flat records, the cell count (the rows are entries: point row / nc of cell row % nc) and
// the points
struct EvalGradP2Src : EvalGradSrc {
    const int *cellsN = nullptr;
    int64_t nc = 0;
    P2Points pts = {};
};
// (the kernel arguments are passed by value: modes, L, the points and the scalars must stay below the 4 KiB the runtime takes)
static_assert(sizeof(EvalModes) + sizeof(EvalGradP2Src) + sizeof(EvalOut) + 128 <= 4096, "kernel arguments of the fused kernels");

template <int T, int G, int NC, int QK>
__global__ __launch_bounds__(TPB) void k_eval_grad_mfma(EvalModes M, int k, int kt, int q, EvalGradSrc S, int64_t n, const double *__restrict__ cf,
                                                        int cs, int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int RB = EvalNormShape<T>::RB, RS = EvalNormShape<T>::RS, TPC = TPB / RB;      // TPC threads share a cell's modes
    const double INF = __builtin_huge_val();
    const int kp = 4 * kt;
    const int cs16 = (cs + 15) & ~15;
    double *s_f = s_dyn;                                   // q x kp rows of RS: plane i, mode t at row i kp + t
    double *s_mn = s_f + (size_t)q * kp * RS;
    double *s_mx = s_mn + cs16;
    double *s_env = s_mx + cs16;
    const int d = threadIdx.x % RB, part = threadIdx.x / RB;
    for (int j = threadIdx.x; j < cs16; j += TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    const int64_t nblk = (n + RB - 1) / RB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * RB, e = row0 + d;
        const bool cv = e < n;
        __syncthreads();
        int v[4] = {0, 0, 0, 0};
        double J[G][G];
        double sc = 1.0;
        if (cv) {
            cell_inverse<G>(S.cells[e], S.coords, S.nv, v, J);
            if (S.scale) sc = S.scale[e];
        }
        for (int t = part; t < kp; t += TPC) {
            double *col = s_f + (size_t)t * RS + d;
            if (cv && t < k) {
                cell_planes<G, NC>(v, J, M.p[t], S.L, q, sc, [&](int i, double p) { col[(size_t)i * kp * RS] = p; });
            } else {
                for (int i = 0; i < q; ++i) col[(size_t)i * kp * RS] = 0.0;
            }
        }
        __syncthreads();
        eval_norm_tiles<T, true, QK>(M, k, kt, q, n, cf, cs, j0, want, first, thr, O, s_f, s_mn, s_mx, s_env, row0);
    }
    eval_store_partials<TPB>(O, s_mn, s_mx, cs16, want);
}

// k_eval_norm_plain with the planes of mode t formed once per pass and used by all q chains: q x NS accumulators, the chains over t
// and the squares over i in ascending order as there
template <int G, int NC, int QK>
__global__ __launch_bounds__(EVAL_PLAIN_TPB) void k_eval_grad_plain(EvalModes M, int k, int kt, int q, EvalGradSrc S, int64_t n,
                                                                    const double *__restrict__ cf, int cs, int64_t j0, int want, int first,
                                                                    double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int NS = eval_plain_ns(QK);
    const double INF = __builtin_huge_val();
    const int cs16 = (cs + 15) & ~15;
    double *s_mn = s_dyn, *s_mx = s_dyn + cs16;
    const int lane = threadIdx.x;
    for (int j = lane; j < cs16; j += EVAL_PLAIN_TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    __syncthreads();
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row = blk * EVAL_PLAIN_TPB + lane;
        const bool rv = row < n;
        int v[4] = {0, 0, 0, 0};
        double J[G][G];
        double sc = 1.0;
        if (rv) {
            cell_inverse<G>(S.cells[row], S.coords, S.nv, v, J);
            if (S.scale) sc = S.scale[row];
        }
        double emn = INF, emx = -INF, ect = 0.0;
        for (int jb = 0; jb < cs16; jb += NS) {
            double acc[EVAL_QMAX][NS];
#pragma unroll
            for (int i = 0; i < EVAL_QMAX; ++i)
#pragma unroll
                for (int c = 0; c < NS; ++c) acc[i][c] = 0.0;
            for (int t = 0; t < k; ++t) {
                double p[EVAL_QMAX];
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i) p[i] = 0.0;
                if (rv) cell_planes<G, NC>(v, J, M.p[t], S.L, q, sc, [&](int i, double x) { p[i] = x; });
                const double *cp = cf + eval_cf_index(kt, t, jb);
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i)
                    if (i < q) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) acc[i][c] = fma(cp[c], p[i], acc[i][c]);
                    }
            }
            double ss[NS];
            if constexpr (QK == PGD_EVAL_Q_NORM) {
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = 0.0;
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i)
                    if (i < q) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) ss[c] = fma(acc[i][c], acc[i][c], ss[c]);
                    }
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = sqrt(ss[c]);            // from here on the values
            } else {
                eval_plain_values<QK>(acc, q, ss);
            }
            eval_plain_step(ss, jb, cs, j0, n, row, rv, want, thr, O, s_mn, s_mx, emn, emx, ect);
        }
        if (rv) eval_row_accumulate(O, row, emn, emx, ect, want, first);
    }
    eval_store_partials<EVAL_PLAIN_TPB>(O, s_mn, s_mx, cs16, want);
}

// The instantiations of one (gdim, ncomp): the matrix-unit kernel per row block, the plain kernel, the LDS attribute of the 16-row one
typedef int (*eval_grad_launch_t)(Ctx *, const EvalModes &, int, int, int, const EvalGradSrc &, int64_t, const double *, int, int64_t, int,
                                  int, double, const EvalOut &, int, int *);
struct EvalGradFns {
    eval_grad_launch_t mfma[3] = {nullptr, nullptr, nullptr};      // 16, 32, 64 cells per workgroup
    eval_grad_launch_t plain = nullptr;
    bool (*raise)(size_t) = nullptr;
};

// What pgd_eval_batch_grad hands to eval_batch_run beside the arguments of pgd_eval_batch_norm
struct EvalGrad {
    EvalGradP2Src src;          // (the P1 launchers pass its EvalGradSrc part)
    EvalGradFns fn;
    int64_t mode_len, entries;  // nodes x components; rows of the outputs: cells, times the points for P2
    const Vec *scale;
};

template <int T, int G, int NC, int QK>
static int eval_launch_grad(Ctx *c, const EvalModes &M, int k, int kt, int q, const EvalGradSrc &S, int64_t n, const double *cf, int cs,
                            int64_t j0, int want, int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const size_t lds = eval_norm_lds(T, true, q, kt, (cs + 15) & ~15);
    return launch_persistent(c, k_eval_grad_mfma<T, G, NC, QK>, TPB, lds, (n + 16 * T - 1) / (16 * T), grid_cap, 0, grid_out, M, k, kt, q, S, n, cf,
                                  cs, j0, want, first, thr, O);
}

template <int G, int NC, int QK>
static int eval_launch_grad_plain(Ctx *c, const EvalModes &M, int k, int kt, int q, const EvalGradSrc &S, int64_t n, const double *cf, int cs,
                                  int64_t j0, int want, int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    const int g = (int)(nblk < grid_cap ? nblk : grid_cap);
    const size_t lds = (size_t)2 * ((cs + 15) & ~15) * sizeof(double);
    k_eval_grad_plain<G, NC, QK><<<g, EVAL_PLAIN_TPB, lds, c->stream>>>(M, k, kt, q, S, n, cf, cs, j0, want, first, thr, O);
    PGD_LAUNCH_CHECK(c);
    *grid_out = g;
    return PGD_OK;
}

template <int G, int NC, int QK>
static bool eval_grad_raise_lds(size_t lds) { return eval_raise_lds((const void *)k_eval_grad_mfma<1, G, NC, QK>, lds); }

template <int G, int NC, int QK>
static EvalGradFns eval_grad_fns() {
    EvalGradFns f;
    f.mfma[0] = eval_launch_grad<1, G, NC, QK>;
    if constexpr (eval_kind_tmax(QK) >= 4) {
        f.mfma[1] = eval_launch_grad<2, G, NC, QK>;
        f.mfma[2] = eval_launch_grad<4, G, NC, QK>;
    }
    f.plain = eval_launch_grad_plain<G, NC, QK>;
    f.raise = eval_grad_raise_lds<G, NC, QK>;
    return f;
}

template <int G, int NC>
static EvalGradFns eval_grad_fns_kind(int kind) {
    switch (kind) {
        case PGD_EVAL_Q_VALUE: return eval_grad_fns<G, NC, PGD_EVAL_Q_VALUE>();
        case PGD_EVAL_Q_EIG_MAX: return eval_grad_fns<G, NC, PGD_EVAL_Q_EIG_MAX>();
        case PGD_EVAL_Q_EIG_MIN: return eval_grad_fns<G, NC, PGD_EVAL_Q_EIG_MIN>();
        case PGD_EVAL_Q_EIG_SPREAD: return eval_grad_fns<G, NC, PGD_EVAL_Q_EIG_SPREAD>();
        default: return eval_grad_fns<G, NC, PGD_EVAL_Q_NORM>();
    }
}

static bool eval_grad_pick(int G, int NC, int kind, EvalGradFns *f) {
    switch (G * 10 + NC) {
        case 11: *f = eval_grad_fns_kind<1, 1>(kind); return true;
        case 12: *f = eval_grad_fns_kind<1, 2>(kind); return true;
        case 13: *f = eval_grad_fns_kind<1, 3>(kind); return true;
        case 21: *f = eval_grad_fns_kind<2, 1>(kind); return true;
        case 22: *f = eval_grad_fns_kind<2, 2>(kind); return true;
        case 23: *f = eval_grad_fns_kind<2, 3>(kind); return true;
        case 31: *f = eval_grad_fns_kind<3, 1>(kind); return true;
        case 32: *f = eval_grad_fns_kind<3, 2>(kind); return true;
        case 33: *f = eval_grad_fns_kind<3, 3>(kind); return true;
        default: return false;
    }
}

// ---- pgd_eval_batch_grad_p2: the two fused kernels with the staging step of a P2 entry.  Row = entry: point row / nc of cell
// row % nc, as pgd_cell_gradient_p2 orders them, so a row block is 16 T consecutive cells at one point (or the seam of two points).
// Every entry of a cell forms the inverse and gathers the record's nodal values again - from L2, the npt entries of a cell sit nc
// rows apart - and from the barrier on the kernels are eval_norm_tiles / eval_plain_step.  Rows beyond the range read no record.
template <int T, int G, int NC, int QK>
__global__ __launch_bounds__(TPB) void k_eval_grad_p2_mfma(EvalModes M, int k, int kt, int q, EvalGradP2Src S, int64_t n,
                                                           const double *__restrict__ cf, int cs, int64_t j0, int want, int first, double thr,
                                                           EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int RB = EvalNormShape<T>::RB, RS = EvalNormShape<T>::RS, TPC = TPB / RB;      // TPC threads share an entry's modes
    const double INF = __builtin_huge_val();
    const int kp = 4 * kt;
    const int cs16 = (cs + 15) & ~15;
    double *s_f = s_dyn;                                   // q x kp rows of RS: plane i, mode t at row i kp + t
    double *s_mn = s_f + (size_t)q * kp * RS;
    double *s_mx = s_mn + cs16;
    double *s_env = s_mx + cs16;
    const int d = threadIdx.x % RB, part = threadIdx.x / RB;
    for (int j = threadIdx.x; j < cs16; j += TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    const int64_t nblk = (n + RB - 1) / RB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * RB, row = row0 + d;
        const bool cv = row < n;
        __syncthreads();
        int r[p2_nodes(G)], v[4];
        double J[G][G], w[G + 1], l4[G + 1];
        double sc = 1.0;
        if (cv) {
            const int64_t e = row % S.nc;
            cell_inverse<G>(p2_record<G>(S.cellsN, e, r), S.coords, S.nv, v, J);
            p2_weights<G>(S.pts, (int)(row / S.nc), w, l4);
            if (S.scale) sc = S.scale[e];
        }
        for (int t = part; t < kp; t += TPC) {
            double *col = s_f + (size_t)t * RS + d;
            if (cv && t < k) {
                double un[p2_nodes(G) * NC];
                p2_gather<G, NC>(r, M.p[t], un);
                p2_planes<G, NC>(un, w, l4, J, S.L, q, sc, [&](int i, double p) { col[(size_t)i * kp * RS] = p; });
            } else {
                for (int i = 0; i < q; ++i) col[(size_t)i * kp * RS] = 0.0;
            }
        }
        __syncthreads();
        eval_norm_tiles<T, true, QK>(M, k, kt, q, n, cf, cs, j0, want, first, thr, O, s_f, s_mn, s_mx, s_env, row0);
    }
    eval_store_partials<TPB>(O, s_mn, s_mx, cs16, want);
}

template <int G, int NC, int QK>
__global__ __launch_bounds__(EVAL_PLAIN_TPB) void k_eval_grad_p2_plain(EvalModes M, int k, int kt, int q, EvalGradP2Src S, int64_t n,
                                                                       const double *__restrict__ cf, int cs, int64_t j0, int want,
                                                                       int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int NS = eval_plain_ns(QK);
    const double INF = __builtin_huge_val();
    const int cs16 = (cs + 15) & ~15;
    double *s_mn = s_dyn, *s_mx = s_dyn + cs16;
    const int lane = threadIdx.x;
    for (int j = lane; j < cs16; j += EVAL_PLAIN_TPB) { s_mn[j] = INF; s_mx[j] = -INF; }
    __syncthreads();
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row = blk * EVAL_PLAIN_TPB + lane;
        const bool rv = row < n;
        int r[p2_nodes(G)], v[4];
        double J[G][G], w[G + 1], l4[G + 1];
        double sc = 1.0;
        if (rv) {
            const int64_t e = row % S.nc;
            cell_inverse<G>(p2_record<G>(S.cellsN, e, r), S.coords, S.nv, v, J);
            p2_weights<G>(S.pts, (int)(row / S.nc), w, l4);
            if (S.scale) sc = S.scale[e];
        }
        double emn = INF, emx = -INF, ect = 0.0;
        for (int jb = 0; jb < cs16; jb += NS) {
            double acc[EVAL_QMAX][NS];
#pragma unroll
            for (int i = 0; i < EVAL_QMAX; ++i)
#pragma unroll
                for (int c = 0; c < NS; ++c) acc[i][c] = 0.0;
            for (int t = 0; t < k; ++t) {
                double p[EVAL_QMAX];
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i) p[i] = 0.0;
                if (rv) {
                    double un[p2_nodes(G) * NC];
                    p2_gather<G, NC>(r, M.p[t], un);
                    p2_planes<G, NC>(un, w, l4, J, S.L, q, sc, [&](int i, double x) { p[i] = x; });
                }
                const double *cp = cf + eval_cf_index(kt, t, jb);
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i)
                    if (i < q) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) acc[i][c] = fma(cp[c], p[i], acc[i][c]);
                    }
            }
            double ss[NS];
            if constexpr (QK == PGD_EVAL_Q_NORM) {
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = 0.0;
#pragma unroll
                for (int i = 0; i < EVAL_QMAX; ++i)
                    if (i < q) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) ss[c] = fma(acc[i][c], acc[i][c], ss[c]);
                    }
#pragma unroll
                for (int c = 0; c < NS; ++c) ss[c] = sqrt(ss[c]);            // from here on the values
            } else {
                eval_plain_values<QK>(acc, q, ss);
            }
            eval_plain_step(ss, jb, cs, j0, n, row, rv, want, thr, O, s_mn, s_mx, emn, emx, ect);
        }
        if (rv) eval_row_accumulate(O, row, emn, emx, ect, want, first);
    }
    eval_store_partials<EVAL_PLAIN_TPB>(O, s_mn, s_mx, cs16, want);
}

// (the launchers take the EvalGradSrc of eval_grad_launch_t: pgd_eval_batch_grad_p2 hands them the EvalGradP2Src it filled)
template <int T, int G, int NC, int QK>
static int eval_launch_grad_p2(Ctx *c, const EvalModes &M, int k, int kt, int q, const EvalGradSrc &S, int64_t n, const double *cf, int cs,
                               int64_t j0, int want, int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const size_t lds = eval_norm_lds(T, true, q, kt, (cs + 15) & ~15);
    return launch_persistent(c, k_eval_grad_p2_mfma<T, G, NC, QK>, TPB, lds, (n + 16 * T - 1) / (16 * T), grid_cap, 0, grid_out, M, k, kt, q,
                                  static_cast<const EvalGradP2Src &>(S), n, cf, cs, j0, want, first, thr, O);
}

template <int G, int NC, int QK>
static int eval_launch_grad_p2_plain(Ctx *c, const EvalModes &M, int k, int kt, int q, const EvalGradSrc &S, int64_t n, const double *cf,
                                     int cs, int64_t j0, int want, int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
    const int g = (int)(nblk < grid_cap ? nblk : grid_cap);
    const size_t lds = (size_t)2 * ((cs + 15) & ~15) * sizeof(double);
    k_eval_grad_p2_plain<G, NC, QK><<<g, EVAL_PLAIN_TPB, lds, c->stream>>>(M, k, kt, q, static_cast<const EvalGradP2Src &>(S), n, cf, cs, j0,
                                                                      want, first, thr, O);
    PGD_LAUNCH_CHECK(c);
    *grid_out = g;
    return PGD_OK;
}

template <int G, int NC, int QK>
static bool eval_grad_p2_raise_lds(size_t lds) { return eval_raise_lds((const void *)k_eval_grad_p2_mfma<1, G, NC, QK>, lds); }

template <int G, int NC, int QK>
static EvalGradFns eval_grad_p2_fns() {
    EvalGradFns f;
    f.mfma[0] = eval_launch_grad_p2<1, G, NC, QK>;
    if constexpr (eval_kind_tmax(QK) >= 4) {
        f.mfma[1] = eval_launch_grad_p2<2, G, NC, QK>;
        f.mfma[2] = eval_launch_grad_p2<4, G, NC, QK>;
    }
    f.plain = eval_launch_grad_p2_plain<G, NC, QK>;
    f.raise = eval_grad_p2_raise_lds<G, NC, QK>;
    return f;
}

template <int G, int NC>
static EvalGradFns eval_grad_p2_fns_kind(int kind) {
    switch (kind) {
        case PGD_EVAL_Q_VALUE: return eval_grad_p2_fns<G, NC, PGD_EVAL_Q_VALUE>();
        case PGD_EVAL_Q_EIG_MAX: return eval_grad_p2_fns<G, NC, PGD_EVAL_Q_EIG_MAX>();
        case PGD_EVAL_Q_EIG_MIN: return eval_grad_p2_fns<G, NC, PGD_EVAL_Q_EIG_MIN>();
        case PGD_EVAL_Q_EIG_SPREAD: return eval_grad_p2_fns<G, NC, PGD_EVAL_Q_EIG_SPREAD>();
        default: return eval_grad_p2_fns<G, NC, PGD_EVAL_Q_NORM>();
    }
}

static bool eval_grad_p2_pick(int G, int NC, int kind, EvalGradFns *f) {
    switch (G * 10 + NC) {
        case 21: *f = eval_grad_p2_fns_kind<2, 1>(kind); return true;
        case 22: *f = eval_grad_p2_fns_kind<2, 2>(kind); return true;
        case 23: *f = eval_grad_p2_fns_kind<2, 3>(kind); return true;
        case 31: *f = eval_grad_p2_fns_kind<3, 1>(kind); return true;
        case 32: *f = eval_grad_p2_fns_kind<3, 2>(kind); return true;
        case 33: *f = eval_grad_p2_fns_kind<3, 3>(kind); return true;
        default: return false;
    }
}

// The checks pgd_cell_gradient_p2 and pgd_eval_batch_grad_p2 share (fn: the entry point's name): the layout - P2 triangles or
// tetrahedra, whose 6 / 10-node records are the flat ones; the 1-D P2 layout keeps its 3-node record in `cells` and is served by
// the host -, the points, L and the scale.  On success *bp is the scalar layout, P and Lv are filled.
static int grad_p2_check(Ctx *c, const char *fn, pgd_handle mh, const double *lam, int npt, const double *L, int q, pgd_handle scale_h,
                         Mesh **mp, Mesh **bp, Vec **scalep, P2Points *P, GradL *Lv) {
    Mesh *m = get_mesh(c, mh);
    if (!m) return fail(c, PGD_ERR_INVALID, "%s: invalid mesh handle", fn);
    Mesh *b = m->ncomp > 1 ? get_mesh(c, m->base) : m;          // the scalar layout holds the cells and the coordinates
    if (!b) return fail(c, PGD_ERR_INVALID, "%s: the blocked layout's base is gone", fn);
    const int G = b->gdim, NC = m->ncomp;
    if ((G != 2 && G != 3) || !b->cellsN || b->nvpc != p2_nodes(G) || !b->coords)
        return fail(c, PGD_ERR_INVALID, "%s: a layout of %d nodes per cell in %d-D: P2 triangles (6) or tetrahedra (10) only", fn, b->nvpc, G);
    if (NC < 1 || NC > 3) return fail(c, PGD_ERR_INVALID, "%s: gdim = %d with %d components", fn, G, NC);
    if (npt < 1 || npt > P2_NPT_MAX) return fail(c, PGD_ERR_INVALID, "%s: npt = %d points per cell, 1 .. %d are possible", fn, npt, P2_NPT_MAX);
    if (!lam) return fail(c, PGD_ERR_INVALID, "%s: lam is missing", fn);
    if (q < 1 || q > EVAL_QMAX) return fail(c, PGD_ERR_INVALID, "%s: q = %d rows of L, 1 .. %d are possible", fn, q, EVAL_QMAX);
    if (!L) return fail(c, PGD_ERR_INVALID, "%s: L is missing", fn);
    Vec *scale = scale_h ? get_vec(c, scale_h) : nullptr;
    if (scale_h && (!scale || scale->n != b->nc))
        return fail(c, PGD_ERR_INVALID, "%s: scale is a vector of one entry per cell (%lld), or 0", fn, (long long)b->nc);
    for (int i = 0; i < P2_NPT_MAX * 4; ++i) P->lam[i] = i < npt * (G + 1) ? lam[i] : 0.0;
    P->npt = npt;
    const int qin = NC * G;
    for (int i = 0; i < EVAL_QMAX * EVAL_QMAX; ++i) Lv->a[i] = i < q * qin ? L[i] : 0.0;
    *mp = m; *bp = b; *scalep = scale;
    return PGD_OK;
}

}  // namespace pgd

using namespace pgd;

extern "C" {

// The body of pgd_eval_batch (q == 0: the signed values, k_eval_mfma / k_eval_plain) and of pgd_eval_batch_norm (1 <= q <= 9: every
// mode is q planes, the norm kernels): the checks, the chunking and the coefficient staging are the same, only the launch differs.
// pgd_eval_batch_grad and pgd_eval_batch_grad_p2 are the second of these with `gs`: the modes are nodal, the planes are formed in
// the kernel, the outputs have gs->entries rows (one per cell; per point and cell for P2).  fn: the entry point's name for the messages.
static int eval_batch_run(Ctx *c, const char *fn, const EvalGrad *gs, const pgd_handle *modes, int k, int q, int kind, const double *coefs, int64_t s, int want,
                          double threshold, double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h,
                          pgd_handle fields_h) {
    // ---- every argument is checked before anything is launched
    if (k < 1 || k > EVAL_KMAX) return fail(c, PGD_ERR_INVALID, "%s: k = %d modes, 1 .. %d are possible", fn, k, EVAL_KMAX);
    if (s < 1 || s > EVAL_SMAX) return fail(c, PGD_ERR_INVALID, "%s: s = %lld samples, 1 .. 2^24 are possible", fn, (long long)s);
    if (!modes || !coefs) return fail(c, PGD_ERR_INVALID, "%s: modes or coefficients missing", fn);
    if (want < 1 || want > 15) return fail(c, PGD_ERR_INVALID, "%s: want = %d names no output (bits 1, 2, 4, 8)", fn, want);
    EvalModes M;
    std::vector<Vec *> mv((size_t)k);
    int64_t n = 0;
    for (int t = 0; t < k; ++t) {
        mv[t] = get_vec(c, modes[t]);
        if (!mv[t]) return fail(c, PGD_ERR_INVALID, "%s: mode %d is not a vector", fn, t);
        if (t == 0) n = mv[t]->n;
        if (mv[t]->n != n) return fail(c, PGD_ERR_INVALID, "%s: mode %d has %lld entries, mode 0 has %lld", fn, t, (long long)mv[t]->n, (long long)n);
        M.p[t] = mv[t]->d;
    }
    for (int t = k; t < EVAL_KMAX; ++t) M.p[t] = nullptr;
    if (gs) {                                        // nodal modes, values per cell
        if (n != gs->mode_len)
            return fail(c, PGD_ERR_INVALID, "%s: the modes have %lld entries, nodes x components = %lld are needed", fn, (long long)n,
                        (long long)gs->mode_len);
        n = gs->entries;
    } else if (q > 0) {                              // q planes of n entries each
        if (n % q) return fail(c, PGD_ERR_INVALID, "%s: the modes have %lld entries, no multiple of q = %d", fn, (long long)n, q);
        n /= q;
    }
    if ((want & PGD_EVAL_STATS) ? !sample_stats : sample_stats != nullptr)
        return fail(c, PGD_ERR_INVALID, "%s: sample_stats %s", fn, sample_stats ? "passed but not requested (bit 1)" : "requested (bit 1) but missing");
    Vec *outs[4] = {nullptr, nullptr, nullptr, nullptr};
    const pgd_handle oh[4] = {env_min_h, env_max_h, exceed_h, fields_h};
    const int obit[4] = {PGD_EVAL_ENVELOPE, PGD_EVAL_ENVELOPE, PGD_EVAL_EXCEED, PGD_EVAL_FIELDS};
    static const char *const oname[4] = {"env_min", "env_max", "exceed", "fields"};
    for (int i = 0; i < 4; ++i) {
        if (!(want & obit[i])) {
            if (oh[i] != 0) return fail(c, PGD_ERR_INVALID, "%s: %s passed but not requested (bit %d)", fn, oname[i], obit[i]);
            continue;
        }
        outs[i] = get_vec(c, oh[i]);
        if (!outs[i]) return fail(c, PGD_ERR_INVALID, "%s: %s requested (bit %d) but missing or not a vector", fn, oname[i], obit[i]);
        int64_t need = n;
        if (i == 3) {
            if (n > 0 && s > std::numeric_limits<int64_t>::max() / 8 / n)
                return fail(c, PGD_ERR_INVALID, "%s: s * n = %lld * %lld overflows the fields vector", fn, (long long)s, (long long)n);
            need = n * s;
        }
        if (outs[i]->n != need)
            return fail(c, PGD_ERR_INVALID, "%s: %s has %lld entries, %lld are needed", fn, oname[i], (long long)outs[i]->n, (long long)need);
        for (int t = 0; t < k; ++t)
            if (mv[t] == outs[i]) return fail(c, PGD_ERR_INVALID, "%s: mode %d aliases %s", fn, t, oname[i]);
        if (gs && gs->scale && gs->scale == outs[i]) return fail(c, PGD_ERR_INVALID, "%s: the scale aliases %s", fn, oname[i]);
        for (int i2 = 0; i2 < i; ++i2)
            if (outs[i2] == outs[i]) return fail(c, PGD_ERR_INVALID, "%s: %s aliases %s", fn, oname[i], oname[i2]);
    }
    if (!(want & PGD_EVAL_EXCEED) && threshold != 0.0)
        return fail(c, PGD_ERR_INVALID, "%s: a threshold without the exceedance output (bit 4)", fn);
    if (threshold != threshold) return fail(c, PGD_ERR_INVALID, "%s: the threshold is NaN", fn);
    if (n == 0) return PGD_OK;

    const bool mfma = c->eval_variant != 0;
    const int kt = (mfma && q == 0) ? dense_kt(k) : (k + 3) / 4;
    int64_t chunk = c->eval_chunk > 0 ? c->eval_chunk : EVAL_CHUNK_DEFAULT;
    if (chunk > s) chunk = s;
    const int cs16_max = (int)((chunk + 15) & ~(int64_t)15);
    const size_t cf_doubles = (size_t)(cs16_max / 16) * kt * 64;
    const int grid_cap = c->eval_grid_max > 0 ? c->eval_grid_max : (1 << 30);
    // most workgroups either kernel can be launched with: bounds the partial rows
    int64_t gmax = (int64_t)c->num_cu * 8;
    if (gmax > grid_cap) gmax = grid_cap;

    EvalNormCfg ncfg;
    const EvalNormFns nfn = eval_norm_pick(kind);
    if (mfma && q > 0) ncfg = eval_norm_choose(q, kt, cs16_max, eval_kind_tmax(kind), gs ? gs->fn.raise : nfn.raise);
    if (gs && mfma && !ncfg.ldsb)                    // (no fragments from global memory here: there are no planes to read)
        return fail(c, PGD_ERR_LIMIT, "%s: q = %d planes of k = %d modes do not fit a workgroup: 16 cells need %zu bytes of LDS "
                    "(8 q 4 ceil(k / 4) 16 and the extrema), the limit is %zu; PGD_TUNE_EVAL_VARIANT = 0 has no such limit", fn, q, k,
                    eval_norm_lds(1, true, q, kt, cs16_max), EVAL_LDS_MAX);

    // pinned staging of the coefficients in fragment order, two chunks deep (an event per half says when its copy is done)
    const size_t pin_bytes = 2 * cf_doubles * sizeof(double);
    if (c->eval_pin_bytes < pin_bytes) {
        for (int i = 0; i < 2; ++i)
            if (c->eval_ev_set[i]) { PGD_HIP(c, hipEventSynchronize(c->eval_ev[i])); c->eval_ev_set[i] = false; }
        if (c->eval_pin) (void)hipHostFree(c->eval_pin);
        c->eval_pin = nullptr;
        c->eval_pin_bytes = 0;
        void *p = nullptr;
        PGD_HIP(c, hipHostMalloc(&p, pin_bytes, hipHostMallocDefault));
        c->eval_pin = (double *)p;
        c->eval_pin_bytes = pin_bytes;
    }
    for (int i = 0; i < 2; ++i)
        if (!c->eval_ev[i]) PGD_HIP(c, hipEventCreateWithFlags(&c->eval_ev[i], hipEventDisableTiming));

    void *p_cf = nullptr, *p_part = nullptr, *p_stats = nullptr;
    const size_t cf_bytes = eval_round(cf_doubles * sizeof(double));
    const size_t part_bytes = (want & PGD_EVAL_STATS) ? eval_round((size_t)gmax * 2 * cs16_max * sizeof(double)) : 0;
    const size_t stats_bytes = (want & PGD_EVAL_STATS) ? eval_round((size_t)3 * s * sizeof(double)) : 0;
    int rc = dev_alloc(c, &p_cf, cf_bytes);
    if (rc == PGD_OK && part_bytes) rc = dev_alloc(c, &p_part, part_bytes);
    if (rc == PGD_OK && stats_bytes) rc = dev_alloc(c, &p_stats, stats_bytes);
    auto release = [&]() {
        dev_release(c, p_cf, cf_bytes);
        dev_release(c, p_part, part_bytes);
        dev_release(c, p_stats, stats_bytes);
    };
    if (rc != PGD_OK) { release(); return rc; }

    if (q > 0) {
        c->eval_norm_rows = mfma ? 16 * ncfg.t : EVAL_PLAIN_TPB;
        c->eval_norm_staged = !mfma ? 0 : !ncfg.ldsb ? 0 : eval_norm_lds(ncfg.t, true, q, kt, cs16_max) > EVAL_LDS_PLAIN ? 2 : 1;
    }

    EvalOut O;
    O.part = (double *)p_part;
    O.env_min = outs[0] ? outs[0]->d : nullptr;
    O.env_max = outs[1] ? outs[1]->d : nullptr;
    O.exceed = outs[2] ? outs[2]->d : nullptr;
    O.fields = outs[3] ? outs[3]->d : nullptr;

    auto run = [&]() -> int {
        int ci = 0;
        for (int64_t j0 = 0; j0 < s; j0 += chunk, ++ci) {
            const int cs = (int)((s - j0 < chunk) ? s - j0 : chunk);
            const int cs16 = (cs + 15) & ~15;
            const int par = ci & 1;
            double *pin = c->eval_pin + (size_t)par * cf_doubles;
            if (c->eval_ev_set[par]) { PGD_HIP(c, hipEventSynchronize(c->eval_ev[par])); c->eval_ev_set[par] = false; }
            const size_t used = (size_t)(cs16 / 16) * kt * 64;
            for (size_t i = 0; i < used; ++i) pin[i] = 0.0;
            for (int t = 0; t < k; ++t) {
                const double *src = coefs + (size_t)t * (size_t)s + (size_t)j0;
                const size_t base = (size_t)(t >> 2) * 64 + (size_t)((t & 3) << 4);
                for (int j = 0; j < cs; ++j) pin[(size_t)(j >> 4) * kt * 64 + base + (j & 15)] = src[j];
            }
            PGD_HIP(c, hipMemcpyAsync(p_cf, pin, used * sizeof(double), hipMemcpyHostToDevice, c->stream));
            PGD_HIP(c, hipEventRecord(c->eval_ev[par], c->stream));
            c->eval_ev_set[par] = true;
            const double *cf = (const double *)p_cf;
            const int first = j0 == 0;
            int g = 0;
            if (gs) {
                const eval_grad_launch_t launch = !mfma ? gs->fn.plain : gs->fn.mfma[ncfg.t == 4 ? 2 : ncfg.t == 2 ? 1 : 0];
                PGD_TRY(launch(c, M, k, kt, q, gs->src, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g));
            } else if (q > 0) {
                PGD_TRY(nfn.launch(c, mfma, ncfg, M, k, kt, q, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g));
            } else if (mfma) {
                // (KT k-steps with 16 T rows per workgroup: 64 up to 64 modes, 32 up to 128, 16 up to 256)
                PGD_TRY(dense_dispatch(kt, [&](auto KT, auto T) {
                    return eval_launch_mfma<decltype(KT)::value, decltype(T)::value>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g);
                }));
            } else {
                const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
                g = (int)(nblk < gmax ? nblk : gmax);
                k_eval_plain<<<g, EVAL_PLAIN_TPB, (size_t)2 * cs16 * sizeof(double), c->stream>>>(M, k, kt, n, cf, cs, j0, want, first, threshold, O);
                PGD_LAUNCH_CHECK(c);
            }
            if (want & PGD_EVAL_STATS) {
                k_eval_finish<<<(cs + TPB - 1) / TPB, TPB, 0, c->stream>>>(O.part, g, cs, (double *)p_stats, j0, s);
                PGD_LAUNCH_CHECK(c);
            }
        }
        if (want & PGD_EVAL_STATS) {
            PGD_HIP(c, hipMemcpyAsync(sample_stats, p_stats, (size_t)3 * s * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the call (host buffer is caller-owned)
        }
        return PGD_OK;
    };
    rc = run();
    release();
    return rc;
}

int pgd_eval_batch(pgd_handle h, const pgd_handle *modes, int k, const double *coefs, int64_t s, int want, double threshold,
                   double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_run(c, "eval_batch", nullptr, modes, k, 0, PGD_EVAL_Q_NORM, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

// The kind of a *_quantity call against its q (fn: the entry point's name)
static int eval_kind_check(Ctx *c, const char *fn, int q, int kind) {
    if (kind < PGD_EVAL_Q_NORM || kind > PGD_EVAL_Q_EIG_SPREAD)
        return fail(c, PGD_ERR_INVALID, "%s: kind = %d is no pgd_eval_quantity (0 .. %d)", fn, kind, (int)PGD_EVAL_Q_EIG_SPREAD);
    if (kind == PGD_EVAL_Q_VALUE && q != 1)
        return fail(c, PGD_ERR_INVALID, "%s: the signed value (kind 1) is that of one plane, q = %d", fn, q);
    if (eval_kind_is_tensor(kind) && q != 4 && q != EVAL_TENSOR_Q)
        return fail(c, PGD_ERR_INVALID, "%s: the eigenvalue kinds take the q = 6 planes xx, yy, zz, xy, yz, xz of a symmetric tensor or the "
                    "q = 4 planes xx, yy, zz, xy of plane strain, q = %d", fn, q);
    return PGD_OK;
}

// pgd_eval_batch_norm is kind 0 of pgd_eval_batch_quantity; likewise the two fused calls below (fn: the entry point's name)
static int eval_batch_planes(Ctx *c, const char *fn, const pgd_handle *modes, int k, int q, int kind, const double *coefs, int64_t s, int want,
                             double threshold, double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h,
                             pgd_handle fields_h) {
    if (q < 1 || q > EVAL_QMAX) return fail(c, PGD_ERR_INVALID, "%s: q = %d planes, 1 .. %d are possible", fn, q, EVAL_QMAX);
    PGD_TRY(eval_kind_check(c, fn, q, kind));
    return eval_batch_run(c, fn, nullptr, modes, k, q, kind, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

int pgd_eval_batch_norm(pgd_handle h, const pgd_handle *modes, int k, int q, const double *coefs, int64_t s, int want, double threshold,
                        double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_planes(c, "eval_batch_norm", modes, k, q, PGD_EVAL_Q_NORM, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h,
                             exceed_h, fields_h);
}

int pgd_eval_batch_quantity(pgd_handle h, const pgd_handle *modes, int k, int q, int kind, const double *coefs, int64_t s, int want,
                            double threshold, double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h,
                            pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_planes(c, "eval_batch_quantity", modes, k, q, kind, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h, exceed_h,
                             fields_h);
}

static int eval_batch_fused(Ctx *c, const char *fn, pgd_handle mh, const pgd_handle *modes, int k, const double *L, int q, int kind,
                            pgd_handle scale_h, const double *coefs, int64_t s, int want, double threshold, double *sample_stats,
                            pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    Mesh *m = get_mesh(c, mh);
    if (!m) return fail(c, PGD_ERR_INVALID, "%s: invalid mesh handle", fn);
    Mesh *b = m->ncomp > 1 ? get_mesh(c, m->base) : m;          // the scalar layout holds the cells and the coordinates
    if (!b) return fail(c, PGD_ERR_INVALID, "%s: the blocked layout's base is gone", fn);
    const int G = b->gdim, NC = m->ncomp;
    if (b->nvpc != G + 1) return fail(c, PGD_ERR_INVALID, "%s: a P2 layout (%d nodes per cell): P1 only", fn, b->nvpc);
    if (!b->cells || !b->coords) return fail(c, PGD_ERR_INVALID, "%s: the layout has no cell records", fn);
    if (q < 1 || q > EVAL_QMAX) return fail(c, PGD_ERR_INVALID, "%s: q = %d rows of L, 1 .. %d are possible", fn, q, EVAL_QMAX);
    if (!L) return fail(c, PGD_ERR_INVALID, "%s: L is missing", fn);
    Vec *scale = scale_h ? get_vec(c, scale_h) : nullptr;
    if (scale_h && (!scale || scale->n != b->nc))
        return fail(c, PGD_ERR_INVALID, "%s: scale is a vector of one entry per cell (%lld), or 0", fn, (long long)b->nc);
    PGD_TRY(eval_kind_check(c, fn, q, kind));
    EvalGrad gs;
    if (!eval_grad_pick(G, NC, kind, &gs.fn)) return fail(c, PGD_ERR_INVALID, "%s: gdim = %d with %d components", fn, G, NC);
    gs.src.cells = b->cells;
    gs.src.coords = b->coords;
    gs.src.scale = scale ? scale->d : nullptr;
    gs.src.nv = b->nv;
    const int qin = NC * G;
    for (int i = 0; i < EVAL_QMAX * EVAL_QMAX; ++i) gs.src.L.a[i] = i < q * qin ? L[i] : 0.0;
    gs.mode_len = b->nv * NC;
    gs.entries = b->nc;
    gs.scale = scale;
    return eval_batch_run(c, fn, &gs, modes, k, q, kind, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

int pgd_eval_batch_grad(pgd_handle h, pgd_handle mh, const pgd_handle *modes, int k, const double *L, int q, pgd_handle scale_h,
                        const double *coefs, int64_t s, int want, double threshold, double *sample_stats, pgd_handle env_min_h,
                        pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_fused(c, "eval_batch_grad", mh, modes, k, L, q, PGD_EVAL_Q_NORM, scale_h, coefs, s, want, threshold, sample_stats, env_min_h,
                            env_max_h, exceed_h, fields_h);
}

int pgd_eval_batch_grad_quantity(pgd_handle h, pgd_handle mh, const pgd_handle *modes, int k, const double *L, int q, int kind,
                                 pgd_handle scale_h, const double *coefs, int64_t s, int want, double threshold, double *sample_stats,
                                 pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_fused(c, "eval_batch_grad_quantity", mh, modes, k, L, q, kind, scale_h, coefs, s, want, threshold, sample_stats, env_min_h,
                            env_max_h, exceed_h, fields_h);
}

int pgd_eval_norm_last_shape(pgd_handle h, int *rows, int *staged) {
    PGD_CTX(c, h);
    if (!rows || !staged) return fail(c, PGD_ERR_INVALID, "eval_norm_last_shape: null output");
    *rows = c->eval_norm_rows;
    *staged = c->eval_norm_staged;
    return PGD_OK;
}

int pgd_cell_gradient(pgd_handle h, pgd_handle mh, pgd_handle uh, const double *L, int q, pgd_handle scale_h, pgd_handle out_h) {
    PGD_CTX(c, h);
    Mesh *m = get_mesh(c, mh);
    if (!m) return fail(c, PGD_ERR_INVALID, "cell_gradient: invalid mesh handle");
    Mesh *b = m->ncomp > 1 ? get_mesh(c, m->base) : m;          // the scalar layout holds the cells and the coordinates
    if (!b) return fail(c, PGD_ERR_INVALID, "cell_gradient: the blocked layout's base is gone");
    const int G = b->gdim, NC = m->ncomp;
    if (b->nvpc != G + 1) return fail(c, PGD_ERR_INVALID, "cell_gradient: a P2 layout (%d nodes per cell): P1 only", b->nvpc);
    if (!b->cells || !b->coords) return fail(c, PGD_ERR_INVALID, "cell_gradient: the layout has no cell records");
    if (q < 1 || q > EVAL_QMAX) return fail(c, PGD_ERR_INVALID, "cell_gradient: q = %d rows of L, 1 .. %d are possible", q, EVAL_QMAX);
    if (!L) return fail(c, PGD_ERR_INVALID, "cell_gradient: L is missing");
    Vec *u = get_vec(c, uh), *out = get_vec(c, out_h), *scale = scale_h ? get_vec(c, scale_h) : nullptr;
    if (!u || u->n != b->nv * NC)
        return fail(c, PGD_ERR_INVALID, "cell_gradient: u is a vector of %lld entries (nodes x components)", (long long)(b->nv * NC));
    if (!out || out->n != (int64_t)q * b->nc)
        return fail(c, PGD_ERR_INVALID, "cell_gradient: out is a vector of q * cells = %lld entries", (long long)((int64_t)q * b->nc));
    if (scale_h && (!scale || scale->n != b->nc))
        return fail(c, PGD_ERR_INVALID, "cell_gradient: scale is a vector of one entry per cell (%lld), or 0", (long long)b->nc);
    if (out == u || out == scale) return fail(c, PGD_ERR_INVALID, "cell_gradient: out aliases %s", out == u ? "u" : "scale");
    if (b->nc == 0) return PGD_OK;
    GradL Lv;
    const int qin = NC * G;
    for (int i = 0; i < EVAL_QMAX * EVAL_QMAX; ++i) Lv.a[i] = i < q * qin ? L[i] : 0.0;
    const double *sp = scale ? scale->d : nullptr;
    switch (G * 10 + NC) {
        case 11: cell_gradient_launch<1, 1>(c, b, u->d, Lv, q, sp, out->d); break;
        case 12: cell_gradient_launch<1, 2>(c, b, u->d, Lv, q, sp, out->d); break;
        case 13: cell_gradient_launch<1, 3>(c, b, u->d, Lv, q, sp, out->d); break;
        case 21: cell_gradient_launch<2, 1>(c, b, u->d, Lv, q, sp, out->d); break;
        case 22: cell_gradient_launch<2, 2>(c, b, u->d, Lv, q, sp, out->d); break;
        case 23: cell_gradient_launch<2, 3>(c, b, u->d, Lv, q, sp, out->d); break;
        case 31: cell_gradient_launch<3, 1>(c, b, u->d, Lv, q, sp, out->d); break;
        case 32: cell_gradient_launch<3, 2>(c, b, u->d, Lv, q, sp, out->d); break;
        case 33: cell_gradient_launch<3, 3>(c, b, u->d, Lv, q, sp, out->d); break;
        default: return fail(c, PGD_ERR_INVALID, "cell_gradient: gdim = %d with %d components", G, NC);
    }
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

int pgd_cell_gradient_p2(pgd_handle h, pgd_handle mh, pgd_handle uh, const double *lam, int npt, const double *L, int q, pgd_handle scale_h,
                         pgd_handle out_h) {
    PGD_CTX(c, h);
    Mesh *m, *b;
    Vec *scale;
    P2Points P;
    GradL Lv;
    PGD_TRY(grad_p2_check(c, "cell_gradient_p2", mh, lam, npt, L, q, scale_h, &m, &b, &scale, &P, &Lv));
    const int G = b->gdim, NC = m->ncomp;
    Vec *u = get_vec(c, uh), *out = get_vec(c, out_h);
    if (!u || u->n != b->nv * NC)
        return fail(c, PGD_ERR_INVALID, "cell_gradient_p2: u is a vector of %lld entries (nodes x components)", (long long)(b->nv * NC));
    const int64_t need = (int64_t)q * npt * b->nc;
    if (!out || out->n != need)
        return fail(c, PGD_ERR_INVALID, "cell_gradient_p2: out is a vector of q * npt * cells = %lld entries", (long long)need);
    if (out == u || out == scale) return fail(c, PGD_ERR_INVALID, "cell_gradient_p2: out aliases %s", out == u ? "u" : "scale");
    if (b->nc == 0) return PGD_OK;
    const double *sp = scale ? scale->d : nullptr;
    switch (G * 10 + NC) {
        case 21: cell_gradient_p2_launch<2, 1>(c, b, u->d, P, Lv, q, sp, out->d); break;
        case 22: cell_gradient_p2_launch<2, 2>(c, b, u->d, P, Lv, q, sp, out->d); break;
        case 23: cell_gradient_p2_launch<2, 3>(c, b, u->d, P, Lv, q, sp, out->d); break;
        case 31: cell_gradient_p2_launch<3, 1>(c, b, u->d, P, Lv, q, sp, out->d); break;
        case 32: cell_gradient_p2_launch<3, 2>(c, b, u->d, P, Lv, q, sp, out->d); break;
        default: cell_gradient_p2_launch<3, 3>(c, b, u->d, P, Lv, q, sp, out->d); break;      // (grad_p2_check left these six)
    }
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

static int eval_batch_fused_p2(Ctx *c, const char *fn, pgd_handle mh, const pgd_handle *modes, int k, const double *lam, int npt,
                               const double *L, int q, int kind, pgd_handle scale_h, const double *coefs, int64_t s, int want, double threshold,
                               double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    Mesh *m, *b;
    Vec *scale;
    EvalGrad gs;
    PGD_TRY(grad_p2_check(c, fn, mh, lam, npt, L, q, scale_h, &m, &b, &scale, &gs.src.pts, &gs.src.L));
    PGD_TRY(eval_kind_check(c, fn, q, kind));
    if (!eval_grad_p2_pick(b->gdim, m->ncomp, kind, &gs.fn))
        return fail(c, PGD_ERR_INVALID, "%s: gdim = %d with %d components", fn, b->gdim, m->ncomp);
    gs.src.cells = nullptr;
    gs.src.cellsN = b->cellsN;
    gs.src.coords = b->coords;
    gs.src.scale = scale ? scale->d : nullptr;
    gs.src.nv = b->nv;
    gs.src.nc = b->nc;
    gs.mode_len = b->nv * m->ncomp;
    gs.entries = (int64_t)npt * b->nc;
    gs.scale = scale;
    return eval_batch_run(c, fn, &gs, modes, k, q, kind, coefs, s, want, threshold, sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

int pgd_eval_batch_grad_p2(pgd_handle h, pgd_handle mh, const pgd_handle *modes, int k, const double *lam, int npt, const double *L, int q,
                           pgd_handle scale_h, const double *coefs, int64_t s, int want, double threshold, double *sample_stats,
                           pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_fused_p2(c, "eval_batch_grad_p2", mh, modes, k, lam, npt, L, q, PGD_EVAL_Q_NORM, scale_h, coefs, s, want, threshold,
                               sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

int pgd_eval_batch_grad_p2_quantity(pgd_handle h, pgd_handle mh, const pgd_handle *modes, int k, const double *lam, int npt, const double *L,
                                    int q, int kind, pgd_handle scale_h, const double *coefs, int64_t s, int want, double threshold,
                                    double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h,
                                    pgd_handle fields_h) {
    PGD_CTX(c, h);
    return eval_batch_fused_p2(c, "eval_batch_grad_p2_quantity", mh, modes, k, lam, npt, L, q, kind, scale_h, coefs, s, want, threshold,
                               sample_stats, env_min_h, env_max_h, exceed_h, fields_h);
}

}  // extern "C"
