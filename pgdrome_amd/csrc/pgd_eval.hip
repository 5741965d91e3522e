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
#include "pgd_internal.h"

#include <cmath>
#include <limits>

namespace pgd {

constexpr int EVAL_KMAX = 256;
constexpr int EVAL_CHUNK_DEFAULT = 1024;   // samples per launch: 16 KiB of running extrema in LDS beside the <= 32 KiB mode block
constexpr int64_t EVAL_SMAX = (int64_t)1 << 24;
constexpr int EVAL_PLAIN_TPB = 64;         // k_eval_plain: one wave per workgroup, one row per lane
constexpr int EVAL_PLAIN_NS = 8;           // ... and this many samples per pass over the block's mode values

typedef double d4_t __attribute__((ext_vector_type(4)));

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

// The same outputs from ordinary fma chains over k in ascending order: one wave per workgroup, one row per lane,
// EVAL_PLAIN_NS samples per pass over the row's mode values (which stay in L1 / L2 between the passes).
__global__ __launch_bounds__(EVAL_PLAIN_TPB) void k_eval_plain(EvalModes M, int k, int kt, int64_t n, const double *__restrict__ cf,
                                                               int cs, int64_t j0, int want, int first, double thr, EvalOut O) {
    extern __shared__ double s_dyn[];
    constexpr int NS = EVAL_PLAIN_NS;
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
            double acc[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) acc[q] = 0.0;
            for (int t = 0; t < k; ++t) {
                const double f = rv ? M.p[t][row] : 0.0;
                const double *cp = cf + eval_cf_index(kt, t, jb);
#pragma unroll
                for (int q = 0; q < NS; ++q) acc[q] = fma(cp[q], f, acc[q]);
            }
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const int js = jb + q;
                if (js >= cs) break;                 // uniform
                const double u = acc[q];
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
                    if (lane == 0) { s_mn[js] = fmin(s_mn[js], mn); s_mx[js] = fmax(s_mx[js], mx); }
                }
            }
        }
        if (rv) {
            if (want & PGD_EVAL_ENVELOPE) {
                O.env_min[row] = first ? emn : fmin(O.env_min[row], emn);
                O.env_max[row] = first ? emx : fmax(O.env_max[row], emx);
            }
            if (want & PGD_EVAL_EXCEED) O.exceed[row] = first ? ect : O.exceed[row] + ect;
        }
    }
    if (want & PGD_EVAL_STATS) {
        __syncthreads();
        for (int j = lane; j < cs16; j += EVAL_PLAIN_TPB) {
            O.part[((int64_t)blockIdx.x * 2 + 0) * cs16 + j] = s_mn[j];
            O.part[((int64_t)blockIdx.x * 2 + 1) * cs16 + j] = s_mx[j];
        }
    }
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

template <int KT, int T>
static int eval_launch_mfma(Ctx *c, const EvalModes &M, int k, int64_t n, const double *cf, int cs, int64_t j0, int want,
                            int first, double thr, const EvalOut &O, int grid_cap, int *grid_out) {
    const int cs16 = (cs + 15) & ~15;
    const size_t lds = ((size_t)4 * KT * 16 * T + 2 * (size_t)cs16 + 12 * 16 * T) * sizeof(double);
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_eval_mfma<KT, T>, TPB, lds) != hipSuccess || occ < 1) {
        (void)hipGetLastError();
        occ = 1;
    }
    const int64_t nblk = (n + 16 * T - 1) / (16 * T);
    int64_t g = (int64_t)c->num_cu * occ;
    if (g > grid_cap) g = grid_cap;
    if (g > nblk) g = nblk;
    k_eval_mfma<KT, T><<<(int)g, TPB, lds, c->stream>>>(M, k, n, cf, cs, j0, want, first, thr, O);
    PGD_LAUNCH_CHECK(c);
    *grid_out = (int)g;
    return PGD_OK;
}

// k-steps of 4 the kernel is compiled for: k <= 16, 32, 48, 64 with 64 rows per workgroup, <= 128 with 32, <= 256 with 16
// (the B fragments of a wave are at most 64 doubles per lane)
static int eval_kt(int k) { return k <= 16 ? 4 : k <= 32 ? 8 : k <= 48 ? 12 : k <= 64 ? 16 : k <= 128 ? 32 : 64; }

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

}  // namespace pgd

using namespace pgd;

extern "C" {

int pgd_eval_batch(pgd_handle h, const pgd_handle *modes, int k, const double *coefs, int64_t s, int want, double threshold,
                   double *sample_stats, pgd_handle env_min_h, pgd_handle env_max_h, pgd_handle exceed_h, pgd_handle fields_h) {
    PGD_CTX(c, h);
    // ---- every argument is checked before anything is launched
    if (k < 1 || k > EVAL_KMAX) return fail(c, PGD_ERR_INVALID, "eval_batch: k = %d modes, 1 .. %d are possible", k, EVAL_KMAX);
    if (s < 1 || s > EVAL_SMAX) return fail(c, PGD_ERR_INVALID, "eval_batch: s = %lld samples, 1 .. 2^24 are possible", (long long)s);
    if (!modes || !coefs) return fail(c, PGD_ERR_INVALID, "eval_batch: modes or coefficients missing");
    if (want < 1 || want > 15) return fail(c, PGD_ERR_INVALID, "eval_batch: want = %d names no output (bits 1, 2, 4, 8)", want);
    EvalModes M;
    std::vector<Vec *> mv((size_t)k);
    int64_t n = 0;
    for (int t = 0; t < k; ++t) {
        mv[t] = get_vec(c, modes[t]);
        if (!mv[t]) return fail(c, PGD_ERR_INVALID, "eval_batch: mode %d is not a vector", t);
        if (t == 0) n = mv[t]->n;
        if (mv[t]->n != n) return fail(c, PGD_ERR_INVALID, "eval_batch: mode %d has %lld entries, mode 0 has %lld", t, (long long)mv[t]->n, (long long)n);
        M.p[t] = mv[t]->d;
    }
    for (int t = k; t < EVAL_KMAX; ++t) M.p[t] = nullptr;
    if ((want & PGD_EVAL_STATS) ? !sample_stats : sample_stats != nullptr)
        return fail(c, PGD_ERR_INVALID, "eval_batch: sample_stats %s", sample_stats ? "passed but not requested (bit 1)" : "requested (bit 1) but missing");
    Vec *outs[4] = {nullptr, nullptr, nullptr, nullptr};
    const pgd_handle oh[4] = {env_min_h, env_max_h, exceed_h, fields_h};
    const int obit[4] = {PGD_EVAL_ENVELOPE, PGD_EVAL_ENVELOPE, PGD_EVAL_EXCEED, PGD_EVAL_FIELDS};
    static const char *const oname[4] = {"env_min", "env_max", "exceed", "fields"};
    for (int i = 0; i < 4; ++i) {
        if (!(want & obit[i])) {
            if (oh[i] != 0) return fail(c, PGD_ERR_INVALID, "eval_batch: %s passed but not requested (bit %d)", oname[i], obit[i]);
            continue;
        }
        outs[i] = get_vec(c, oh[i]);
        if (!outs[i]) return fail(c, PGD_ERR_INVALID, "eval_batch: %s requested (bit %d) but missing or not a vector", oname[i], obit[i]);
        int64_t need = n;
        if (i == 3) {
            if (n > 0 && s > std::numeric_limits<int64_t>::max() / 8 / n)
                return fail(c, PGD_ERR_INVALID, "eval_batch: s * n = %lld * %lld overflows the fields vector", (long long)s, (long long)n);
            need = n * s;
        }
        if (outs[i]->n != need)
            return fail(c, PGD_ERR_INVALID, "eval_batch: %s has %lld entries, %lld are needed", oname[i], (long long)outs[i]->n, (long long)need);
        for (int t = 0; t < k; ++t)
            if (mv[t] == outs[i]) return fail(c, PGD_ERR_INVALID, "eval_batch: mode %d aliases %s", t, oname[i]);
        for (int i2 = 0; i2 < i; ++i2)
            if (outs[i2] == outs[i]) return fail(c, PGD_ERR_INVALID, "eval_batch: %s aliases %s", oname[i], oname[i2]);
    }
    if (!(want & PGD_EVAL_EXCEED) && threshold != 0.0)
        return fail(c, PGD_ERR_INVALID, "eval_batch: a threshold without the exceedance output (bit 4)");
    if (threshold != threshold) return fail(c, PGD_ERR_INVALID, "eval_batch: the threshold is NaN");
    if (n == 0) return PGD_OK;

    const bool mfma = c->eval_variant != 0;
    const int kt = mfma ? eval_kt(k) : (k + 3) / 4;
    int64_t chunk = c->eval_chunk > 0 ? c->eval_chunk : EVAL_CHUNK_DEFAULT;
    if (chunk > s) chunk = s;
    const int cs16_max = (int)((chunk + 15) & ~(int64_t)15);
    const size_t cf_doubles = (size_t)(cs16_max / 16) * kt * 64;
    const int grid_cap = c->eval_grid_max > 0 ? c->eval_grid_max : (1 << 30);
    // most workgroups either kernel can be launched with: bounds the partial rows
    int64_t gmax = (int64_t)c->num_cu * 8;
    if (gmax > grid_cap) gmax = grid_cap;

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
            if (mfma) {
                switch (kt) {
                    case 4: PGD_TRY((eval_launch_mfma<4, 4>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                    case 8: PGD_TRY((eval_launch_mfma<8, 4>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                    case 12: PGD_TRY((eval_launch_mfma<12, 4>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                    case 16: PGD_TRY((eval_launch_mfma<16, 4>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                    case 32: PGD_TRY((eval_launch_mfma<32, 2>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                    default: PGD_TRY((eval_launch_mfma<64, 1>(c, M, k, n, cf, cs, j0, want, first, threshold, O, (int)gmax, &g))); break;
                }
            } else {
                const int64_t nblk = (n + EVAL_PLAIN_TPB - 1) / EVAL_PLAIN_TPB;
                g = (int)(nblk < gmax ? nblk : gmax);
                k_eval_plain<<<g, EVAL_PLAIN_TPB, (size_t)2 * cs16 * sizeof(double), c->stream>>>(M, k, kt, n, cf, cs, j0, want, first,
                                                                                                 threshold, O);
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

}  // extern "C"
