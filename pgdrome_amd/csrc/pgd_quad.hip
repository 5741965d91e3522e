// Quadratic forms of the modes at every dof: outs[f][i] = f_i^T Q_f f_i with f_i = (modes[0][i] .. modes[k-1][i]) for nq small k x k
// matrices at once, every mode read ONCE per call.  The variance and Sobol fields of a separated solution are such forms
// (model.py: variance_decomposition); the intermediate F Q (n x k per form) is consumed where it is formed.  The third dense
// product of this library and the third kernel on the matrix unit (v_mfma_f64_16x16x4_f64), in the orientation of k_eval_mfma:
//
//   * B is the F^T fragment of a tile of 16 rows (dofs on the fragment's column index): lane (lq, lr) = (lane >> 4, lane & 15)
//     holds F[row 16 j + lr][k = 4 q' + lq] in b[j][q'], zero beyond k and beyond row n.  A WAVE owns its row tiles - T tiles of 16
//     rows at a time - so no value is summed across waves and nothing is shared between them: the fragments are loaded straight
//     from the mode vectors (per load instruction four runs of 16 consecutive doubles, whole 128-byte lines), not through LDS.
//     The kernel uses no LDS and has no barrier.
//   * A holds 16 rows l of Q: lane (lq, lr) holds Q[16 lt + lr][4 q' + lq].  The host lays the matrices out in that fragment
//     order (pack_a_fragments, kt / 4 tiles of 16 rows per form) and uploads them once per call; a fragment is one coalesced 512-byte load, served by L2, and is
//     used for the T row tiles the wave holds.
//   * D[l][dof] = (Q f)_l: the lane holds D[16 lt + 4 r + lq][lr] in acc[r], and the multiplier of that entry, F[dof lr][16 lt +
//     4 r + lq], is b[j][4 lt + r] - already in the lane's registers.  The value is sum_{lt, r} b[j][4 lt + r] acc[r] as one fma
//     chain in ascending (lt, r), then two __shfl_xor (16, 32) over lq.  Both sums of a xor step have the same two operands, so all
//     four lq hold the same bits.
//   * Extrema: lane f of a wave keeps the running min / max of form f over the wave's rows (nq <= 64 = the lanes of a wave), each
//     wave leaves one row of them, k_quad_finish reduces the rows, a workgroup per form.  Rows >= n never enter an extremum.
//   * Every value has one fixed chain that depends on (k, the row's data, Q_f) alone, min and max do not depend on order: every
//     output is bit-identical for any grid, and a form's field is the same bits alone or among others.
//
// k_quad_plain gives the same outputs from ordinary ascending fma chains, t_l = sum_k Q_lk f_k, then sum_l f_l t_l: the
// cross-check of the tests and the baseline that shows what the matrix unit buys (PGD_TUNE_QUAD_VARIANT).
#include "pgd_internal.h"

#include <limits>
#include <vector>

namespace pgd {

constexpr int QD_KMAX = 256;            // modes per call (EVAL_KMAX)
constexpr int QD_NQMAX = 64;            // forms per call: one lane of a wave per form
constexpr int QD_PLAIN_TPB = 64;        // k_quad_plain: one wave per workgroup, one row per lane

struct QuadModes { const double *p[QD_KMAX]; };
struct QuadOuts { double *p[QD_NQMAX]; };   // nullptr: the field of that form is not stored

// what becomes of the values v of form f at the wave's rows: clamp, store, the wave's running extrema (lane f holds form f's)
template <int NV>
__device__ __forceinline__ void quad_epilogue(double (&v)[NV], const bool (&rv)[NV], const int64_t (&row)[NV], bool writer, int nred,
                                              int f, int clamp, const QuadOuts &O, double &rmn, double &rmx) {
    const double INF = __builtin_huge_val();
    double *o = O.p[f];
    double mn = INF, mx = -INF;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (clamp && v[j] < 0.0) v[j] = 0.0;
        if (rv[j]) {
            mn = fmin(mn, v[j]);
            mx = fmax(mx, v[j]);
            if (o && writer) o[row[j]] = v[j];
        }
    }
    for (int m = 1; m < nred; m <<= 1) {
        mn = fmin(mn, __shfl_xor(mn, m, 64));
        mx = fmax(mx, __shfl_xor(mx, m, 64));
    }
    if ((int)(threadIdx.x & 63) == f) { rmn = fmin(rmn, mn); rmx = fmax(rmx, mx); }
}

// KT: k-steps of 4 the kernel is compiled for (4 KT >= k, KT a multiple of 4); T: row tiles a wave holds at a time
template <int KT, int T>
__global__ __launch_bounds__(TPB) void k_quad_mfma(QuadModes M, int k, int64_t n, const double *__restrict__ qf, int nq, int clamp,
                                                   QuadOuts O, double *__restrict__ part) {
    constexpr int LT = KT / 4;
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
    double rmn = INF, rmx = -INF;
    const int64_t ntile = (n + 16 * T - 1) / (16 * T);
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < ntile; tile += (int64_t)gridDim.x * 4) {
        double b[T][KT];
        bool rv[T];
        int64_t row[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            row[j] = tile * (16 * T) + 16 * j + lr;
            rv[j] = row[j] < n;
        }
#pragma unroll
        for (int q = 0; q < KT; ++q) {
            const int t = 4 * q + lq;
            const double *mp = t < k ? M.p[t] : nullptr;
#pragma unroll
            for (int j = 0; j < T; ++j) b[j][q] = (mp && rv[j]) ? mp[row[j]] : 0.0;
        }
        for (int f = 0; f < nq; ++f) {
            const double *qp = qf + (size_t)f * (LT * KT * 64) + lane;
            double v[T];
#pragma unroll
            for (int j = 0; j < T; ++j) v[j] = 0.0;
#pragma unroll
            for (int lt = 0; lt < LT; ++lt) {
                d4_t acc[T];
#pragma unroll
                for (int j = 0; j < T; ++j) acc[j] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < KT; ++q) {
                    const double a = qp[(lt * KT + q) * 64];
#pragma unroll
                    for (int j = 0; j < T; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j][q], acc[j], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int j = 0; j < T; ++j) v[j] = fma(b[j][4 * lt + r], acc[j][r], v[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < T; ++j) {
                v[j] += __shfl_xor(v[j], 16, 64);
                v[j] += __shfl_xor(v[j], 32, 64);
            }
            quad_epilogue<T>(v, rv, row, lq == 0, 16, f, clamp, O, rmn, rmx);
        }
    }
    const int64_t w = (int64_t)blockIdx.x * 4 + wv;
    part[(w * 2 + 0) * QD_NQMAX + lane] = rmn;
    part[(w * 2 + 1) * QD_NQMAX + lane] = rmx;
}

// The same outputs from ordinary fma chains; qd: the nq matrices row-major as the caller passed them; k x 64 mode values in LDS
__global__ __launch_bounds__(QD_PLAIN_TPB) void k_quad_plain(QuadModes M, int k, int64_t n, const double *__restrict__ qd, int nq, int clamp,
                                                             QuadOuts O, double *__restrict__ part) {
    extern __shared__ double s_f[];
    const double INF = __builtin_huge_val();
    const int lane = threadIdx.x;
    double rmn = INF, rmx = -INF;
    const int64_t nblk = (n + QD_PLAIN_TPB - 1) / QD_PLAIN_TPB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        int64_t row[1] = {blk * QD_PLAIN_TPB + lane};
        bool rv[1] = {row[0] < n};
        __syncthreads();
        for (int t = 0; t < k; ++t) s_f[t * QD_PLAIN_TPB + lane] = rv[0] ? M.p[t][row[0]] : 0.0;
        __syncthreads();
        for (int f = 0; f < nq; ++f) {
            double v[1] = {0.0};
            for (int l = 0; l < k; ++l) {
                const double *ql = qd + ((size_t)f * k + l) * k;
                double t = 0.0;
                for (int kk = 0; kk < k; ++kk) t = fma(ql[kk], s_f[kk * QD_PLAIN_TPB + lane], t);
                v[0] = fma(s_f[l * QD_PLAIN_TPB + lane], t, v[0]);
            }
            quad_epilogue<1>(v, rv, row, true, 64, f, clamp, O, rmn, rmx);
        }
    }
    part[((int64_t)blockIdx.x * 2 + 0) * QD_NQMAX + lane] = rmn;
    part[((int64_t)blockIdx.x * 2 + 1) * QD_NQMAX + lane] = rmx;
}

// a workgroup per form: its threads take the nrows partial rows of the form in turns, then halve through LDS (min and max do not
// depend on the order): ext[2 f] = min, ext[2 f + 1] = max
__global__ __launch_bounds__(TPB) void k_quad_finish(const double *__restrict__ part, int64_t nrows, double *__restrict__ ext) {
    __shared__ double s_mn[TPB], s_mx[TPB];
    const int f = blockIdx.x, tid = threadIdx.x;
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (int64_t w = tid; w < nrows; w += TPB) {
        mn = fmin(mn, part[(w * 2 + 0) * QD_NQMAX + f]);
        mx = fmax(mx, part[(w * 2 + 1) * QD_NQMAX + f]);
    }
    s_mn[tid] = mn;
    s_mx[tid] = mx;
    __syncthreads();
    for (int h = TPB / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_mn[tid] = fmin(s_mn[tid], s_mn[tid + h]);
            s_mx[tid] = fmax(s_mx[tid], s_mx[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        ext[2 * f] = s_mn[0];
        ext[2 * f + 1] = s_mx[0];
    }
}

__global__ __launch_bounds__(TPB) void k_vec_ratio(double *out, const double *num, const double *den, double floor, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const double d = den[i];
        out[i] = d > floor ? num[i] / d : 0.0;
    }
}

// persistent grid of the matrix-unit kernel: at most one wave per tile; a wave leaves one row of partials, sized once the grid is known
template <int KT, int T>
static int quad_launch_mfma(Ctx *c, const QuadModes &M, int k, int64_t n, const double *qf, int nq, int clamp, const QuadOuts &O, int64_t *nrows) {
    const int64_t ntile = (n + 16 * T - 1) / (16 * T);
    const int64_t g = persistent_grid(c, k_quad_mfma<KT, T>, TPB, 0, (ntile + 3) / 4, c->quad_grid_max);
    PGD_TRY(ensure_partials(c, g * 4 * 2 * QD_NQMAX));
    *nrows = g * 4;
    return launch_grid(c, k_quad_mfma<KT, T>, g, TPB, 0, M, k, n, qf, nq, clamp, O, c->partials);
}

static int quad_launch_plain(Ctx *c, const QuadModes &M, int k, int64_t n, const double *qd, int nq, int clamp, const QuadOuts &O, int64_t *nrows) {
    const size_t lds = (size_t)k * QD_PLAIN_TPB * sizeof(double);
    PGD_TRY(raise_lds(c, (const void *)k_quad_plain, lds, "quad_forms"));
    const int64_t g = persistent_grid(c, k_quad_plain, QD_PLAIN_TPB, lds, (n + QD_PLAIN_TPB - 1) / QD_PLAIN_TPB, c->quad_grid_max, 8);
    PGD_TRY(ensure_partials(c, g * 2 * QD_NQMAX));
    *nrows = g;
    return launch_grid(c, k_quad_plain, g, QD_PLAIN_TPB, lds, M, k, n, qd, nq, clamp, O, c->partials);
}

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_quad_forms(pgd_handle h, const pgd_handle *modes, int k, const double *q, int nq, int flags, const pgd_handle *outs, double *extrema) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (k < 1 || k > QD_KMAX) return fail(c, PGD_ERR_INVALID, "quad_forms: k = %d modes, 1 .. %d are possible", k, QD_KMAX);
    if (nq < 1 || nq > QD_NQMAX) return fail(c, PGD_ERR_INVALID, "quad_forms: nq = %d forms, 1 .. %d are possible", nq, QD_NQMAX);
    if (!modes || !q) return fail(c, PGD_ERR_INVALID, "quad_forms: modes or matrices missing");
    if (flags & ~PGD_QUAD_CLAMP) return fail(c, PGD_ERR_INVALID, "quad_forms: flags = %d, only PGD_QUAD_CLAMP is known", flags);
    QuadModes M;
    std::vector<Vec *> mv((size_t)k);
    int64_t n = 0;
    for (int t = 0; t < k; ++t) {
        mv[t] = get_vec(c, modes[t]);
        if (!mv[t]) return fail(c, PGD_ERR_INVALID, "quad_forms: mode %d is not a vector", t);
        if (t == 0) n = mv[t]->n;
        if (mv[t]->n != n)
            return fail(c, PGD_ERR_INVALID, "quad_forms: mode %d has %lld entries, mode 0 has %lld", t, (long long)mv[t]->n, (long long)n);
        M.p[t] = mv[t]->d;
    }
    for (int t = k; t < QD_KMAX; ++t) M.p[t] = nullptr;
    QuadOuts O;
    Vec *ov[QD_NQMAX];
    bool any = false;
    for (int f = 0; f < QD_NQMAX; ++f) { O.p[f] = nullptr; ov[f] = nullptr; }
    for (int f = 0; outs && f < nq; ++f) {
        if (outs[f] == 0) continue;
        ov[f] = get_vec(c, outs[f]);
        if (!ov[f]) return fail(c, PGD_ERR_INVALID, "quad_forms: output %d is not a vector", f);
        if (ov[f]->n != n)
            return fail(c, PGD_ERR_INVALID, "quad_forms: output %d has %lld entries, the modes have %lld", f, (long long)ov[f]->n, (long long)n);
        for (int t = 0; t < k; ++t)
            if (mv[t] == ov[f]) return fail(c, PGD_ERR_INVALID, "quad_forms: output %d aliases mode %d", f, t);
        for (int f2 = 0; f2 < f; ++f2)
            if (ov[f2] == ov[f]) return fail(c, PGD_ERR_INVALID, "quad_forms: output %d aliases output %d", f, f2);
        O.p[f] = ov[f]->d;
        any = true;
    }
    if (!any && !extrema) return fail(c, PGD_ERR_INVALID, "quad_forms: neither a field nor the extrema are asked for");
    if (n == 0) {
        for (int f = 0; extrema && f < nq; ++f) {
            extrema[2 * f] = std::numeric_limits<double>::infinity();
            extrema[2 * f + 1] = -std::numeric_limits<double>::infinity();
        }
        return PGD_OK;
    }

    // ---- the matrices in the order the variant reads them, uploaded once
    const bool mfma = c->quad_variant != 0;
    const int kt = dense_kt(k);
    const size_t qn = mfma ? (size_t)nq * (kt >> 2) * kt * 64 : (size_t)nq * k * k;
    std::vector<double> qh;
    const double *qsrc = q;
    if (mfma) {
        qh.assign(qn, 0.0);
        for (int f = 0; f < nq; ++f) pack_a_fragments(qh.data() + (size_t)f * (kt >> 2) * kt * 64, kt, q + (size_t)f * k * k, k, k, k);
        qsrc = qh.data();
    }
    const int clamp = (flags & PGD_QUAD_CLAMP) ? 1 : 0;
    return with_pool_input(c, pool_bytes(qn), [&](void *p_q) -> int {
        PGD_TRY(ensure_work(c, 6, 2 * QD_NQMAX));
        PGD_HIP(c, hipMemcpyAsync(p_q, qsrc, qn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        const double *qdev = (const double *)p_q;
        int64_t nrows = 0;
        if (mfma) {
            PGD_TRY(dense_dispatch(kt, [&](auto KT, auto T) {
                return quad_launch_mfma<decltype(KT)::value, decltype(T)::value>(c, M, k, n, qdev, nq, clamp, O, &nrows);
            }));
        } else {
            PGD_TRY(quad_launch_plain(c, M, k, n, qdev, nq, clamp, O, &nrows));
        }
        if (extrema) {
            k_quad_finish<<<nq, TPB, 0, c->stream>>>(c->partials, nrows, c->work[6]);
            PGD_LAUNCH_CHECK(c);
            PGD_HIP(c, hipMemcpyAsync(extrema, c->work[6], (size_t)2 * nq * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        PGD_HIP(c, hipStreamSynchronize(c->stream));   // the one synchronisation of the call (the host buffers are the caller's)
        return PGD_OK;
    });
}

int pgd_vec_ratio(pgd_handle h, pgd_handle outh, pgd_handle numh, pgd_handle denh, double floor) {
    PGD_CTX(c, h);
    Vec *out = get_vec(c, outh), *num = get_vec(c, numh), *den = get_vec(c, denh);
    if (!out || !num || !den) return fail(c, PGD_ERR_INVALID, "vec_ratio: invalid handles");
    if (out->n != num->n || den->n != num->n)
        return fail(c, PGD_ERR_INVALID, "vec_ratio: vectors of different lengths (%lld, %lld, %lld)", (long long)out->n, (long long)num->n, (long long)den->n);
    if (floor != floor) return fail(c, PGD_ERR_INVALID, "vec_ratio: the floor is NaN");
    if (num->n == 0) return PGD_OK;
    k_vec_ratio<<<grid_for(num->n), TPB, 0, c->stream>>>(out->d, num->d, den->d, floor, num->n);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

}  // extern "C"
