// Row classes of an operator in diagonal form: how they are FOUND.  (How the products use them: k_spmv_diac_march2 and
// k_spmv_stencil_march, pgd_spmv.hip.)
//
// dia_classify() finds them per solve, LOSSLESSLY: the class table holds the slot values bit by bit and every row is compared
// with its class's tuple before its code is trusted - in full (classify_full: hash, table, codes), or from a structure the mesh
// remembers (classify_known, Mesh::cls_cache in pgd_internal.h).  Either way the classes may turn out to be ONE stencil +
// eliminated nodes (k_stencil_*, StencilInfo).  The file reads: kernels, then the host pieces, then the driver.
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "pgd_internal.h"

namespace pgd {

constexpr int CLS_SLOTS = 1024;          // hash slots of the classification

// Does the dictionary reduce to one stencil?  k_stencil_pick: base class = the class of the row in the middle of the planes
// [z_lo, z_hi), identity class = the tuple (1, 0 .. 0).  A row's tuple holds only the UPPER half of its row: a free node whose
// upper neighbours are all eliminated (the last free node before three faces) carries the identity tuple too.  k_stencil_split
// gives those rows a class id of their own (same tuple, a duplicate table row: the dictionary product does not care), so that
// "class == identity class" means an eliminated node: every coupling TO it is zero as well.  k_stencil_verify: every row of those
// planes, every slot, bit for bit.
struct StencilInfo { int ok, ident, base, split; double c[8]; int zm0, zm1, g_lo, g_hi; };     // g_lo / g_hi: the plane below / above the verified planes is a ghost DATA plane (k_stencil_ghost)

__global__ void k_stencil_pick(const uint8_t *__restrict__ cls, double *__restrict__ table, const int *__restrict__ info,
                               int nx, int ny, int z_lo, int z_hi, StencilInfo *S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    S->ok = 0; S->ident = -1; S->base = -1; S->split = 0;
    const int ncls = info[0];
    if (info[1] != 0 || ncls <= 0 || ncls >= CLS_MAX || z_hi <= z_lo) return;      // (room for one more class id)
    const int64_t mid = (int64_t)nx * ny * ((z_lo + z_hi) / 2) + (int64_t)nx * (ny / 2) + nx / 2;
    for (int k = 0; k < ncls; ++k) {
        bool id = table[k * 8 + cls_pos(0)] == 1.0;
        for (int s = 1; s < 8; ++s) id = id && table[k * 8 + cls_pos(s)] == 0.0;
        if (id) S->ident = k;
    }
    // base class: the tuple with the most couplings (the row in the middle of a thin grid sits next to a face); the middle row's on ties
    int base = cls[mid], best = -1;
    for (int k = 0; k < ncls; ++k) {
        int nzc = 0;
        for (int s = 1; s < 8; ++s) nzc += table[k * 8 + cls_pos(s)] != 0.0 ? 1 : 0;
        if (nzc > best || (nzc == best && k == (int)cls[mid])) { best = nzc; base = k; }
    }
    if (base == S->ident) return;                            // (nothing but identity rows: keep the dictionary form)
    S->base = base;
    for (int s = 0; s < 8; ++s) S->c[s] = table[base * 8 + cls_pos(s)];
    if (S->ident >= 0) {                                     // the duplicate row of the free nodes with the identity tuple, then the zero class
        for (int s = 0; s < 8; ++s) { table[ncls * 8 + s] = table[S->ident * 8 + s]; table[(ncls + 1) * 8 + s] = 0.0; }
    }
    S->ok = 1;
}

__global__ __launch_bounds__(TPB) void k_stencil_split(uint8_t *__restrict__ cls, const double *__restrict__ table, const int *__restrict__ info,
                                                       int nx, int ny, int64_t nv, StencilInfo *S) {
    if (!S->ok || S->ident < 0) return;
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= nv || (int)cls[i] != S->ident) return;
    const int64_t P = (int64_t)nx * ny;
    const int z = (int)(i / P), rem = (int)(i - (int64_t)z * P), y = rem / nx, x = rem - y * nx;
    bool coupled = false;
#pragma unroll
    for (int s = 1; s < 8; ++s) {                            // the lower neighbour whose slot s points at this row
        const int dx = s & 1, dy = (s >> 1) & 1, dz = s >> 2;
        if (x - dx < 0 || y - dy < 0 || z - dz < 0) continue;
        const int kc = cls[i - dx - (int64_t)nx * dy - P * dz];      // (a neighbour re-coded meanwhile carries the same tuple)
        coupled = coupled || table[kc * 8 + cls_pos(s)] != 0.0;
    }
    if (coupled) { cls[i] = (uint8_t)info[0]; S->split = 1; }
}

__global__ void k_stencil_commit(double *__restrict__ table, int *__restrict__ info, StencilInfo *S) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || !S->ok || S->ident < 0) return;
    const int n = info[0];
    if (S->split) info[0] = n + 1;                           // one more class; its zero class sits behind it
    else for (int s = 0; s < 8; ++s) table[n * 8 + s] = 0.0;      // unused: row n is the zero class again
}

// allid[z] = 1 iff plane z holds identity rows only; samem[z] = 1 iff the identity rows of plane z sit where those of plane z - 1 do
__global__ __launch_bounds__(TPB) void k_stencil_allid(const uint8_t *__restrict__ cls, int64_t plane, const StencilInfo *S, int *__restrict__ allid,
                                                       int *__restrict__ samem) {
    __shared__ int s_other, s_diff;
    const int z = blockIdx.x;
    if (threadIdx.x == 0) { s_other = 0; s_diff = 0; }
    __syncthreads();
    const uint8_t *a = cls + plane * z;
    const int ident = S->ident;
    bool other = false, diff = z == 0;
    for (int64_t i = threadIdx.x; i < plane; i += TPB) {
        const bool id = (int)a[i] == ident;
        other = other || !id;
        if (z > 0) diff = diff || id != ((int)a[i - plane] == ident);
    }
    if (other) s_other = 1;
    if (diff) s_diff = 1;
    __syncthreads();
    if (threadIdx.x == 0) { allid[z] = s_other ? 0 : 1; samem[z] = s_diff ? 0 : 1; }
}

// the planes of [z_lo, z_hi) must read [identity planes]* [one run of planes with the SAME identity rows] [identity planes]*
__global__ void k_stencil_planes(const int *__restrict__ same, const int *__restrict__ allid, int z_lo, int z_hi, StencilInfo *S) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || !S->ok) return;
    int a = z_lo, b = z_hi;
    while (a < z_hi && allid[a]) ++a;
    while (b > a && allid[b - 1]) --b;
    bool simple = true;
    for (int z = a; z < b; ++z) simple = simple && !allid[z] && (z == a || same[z] != 0);
    S->zm0 = a; S->zm1 = b;
    if (!simple) S->ok = 0;
}

// A sharded slab's ghost planes: the plane below z_lo (above z_hi - 1) lies inside the array, next to a main plane, and its
// eliminated nodes are exactly those of the main planes - then the march may stage it like a main plane (its rows hold the
// neighbour rank's x; couplings to its eliminated nodes are the exact zeros k_stencil_verify found in the owned rows next to it)
__global__ void k_stencil_ghost_init(StencilInfo *S, int z_lo, int z_hi, int nz, int zm0, int zm1) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (zm0 < 0) { zm0 = S->zm0; zm1 = S->zm1; }
    S->g_lo = (S->ok && z_lo > 0 && zm0 == z_lo && zm1 > zm0) ? 1 : 0;
    S->g_hi = (S->ok && z_hi < nz && zm1 == z_hi && zm1 > zm0) ? 1 : 0;
}
// The couplings between the LOWER ghost plane and the first owned plane live in the ghost rows' dz = 1 slots (half storage: a
// row holds its couplings to the rows behind it), which k_stencil_verify - owned rows only - never sees: they are compared here,
// bitwise, with the stencil's couplings (exact zeros where the target is eliminated or outside), so that the march applies
// c[s] to the neighbour rank's x on evidence, like everywhere else.  (The upper ghost plane is reached through
// the owned rows' own dz = 1 slots, which k_stencil_verify has compared.)
__global__ __launch_bounds__(TPB) void k_stencil_ghost(const uint8_t *__restrict__ cls, const double *__restrict__ table, int nx, int ny,
                                                       int z_lo, int z_hi, int zm0, StencilInfo *S) {
    const int64_t plane = (int64_t)nx * ny;
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= plane || !S->ok) return;
    if (zm0 < 0) zm0 = S->zm0;
    const int ident = S->ident;
    const bool id = (int)cls[plane * zm0 + i] == ident;
    if (S->g_lo) {
        const int k = cls[plane * (z_lo - 1) + i];
        bool good = (k == ident) == id;
        if (good && k != ident) {
            const int y = (int)(i / nx), x = (int)(i - (int64_t)y * nx);
            const double *t = table + k * 8;
#pragma unroll
            for (int s = 4; s < 8; ++s) {
                const int dx = s & 1, dy = (s >> 1) & 1;
                const bool live = x + dx < nx && y + dy < ny && (int)cls[plane * z_lo + i + dx + (int64_t)nx * dy] != ident;
                const double v = t[cls_pos(s)];
                good = good && (live ? __double_as_longlong(v) == __double_as_longlong(S->c[s]) : v == 0.0);
            }
        }
        if (!good) S->g_lo = 0;
    }
    if (S->g_hi && ((int)cls[plane * z_hi + i] == ident) != id) S->g_hi = 0;
}

__global__ __launch_bounds__(TPB) void k_stencil_verify(const uint8_t *__restrict__ cls, const double *__restrict__ table, int nx, int ny,
                                                        int nz, int z_lo, int z_hi, StencilInfo *S) {
    if (!S->ok) return;
    const int64_t P = (int64_t)nx * ny;
    const int64_t i = P * z_lo + (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= P * z_hi) return;
    const int k = cls[i];
    if (k == S->ident) return;
    const int z = (int)(i / P), rem = (int)(i - (int64_t)z * P), y = rem / nx, x = rem - y * nx;
    const double *t = table + k * 8;
    bool good = __double_as_longlong(t[cls_pos(0)]) == __double_as_longlong(S->c[0]);
#pragma unroll
    for (int s = 1; s < 8; ++s) {
        const int dx = s & 1, dy = (s >> 1) & 1, dz = s >> 2;
        const bool inside = x + dx < nx && y + dy < ny && z + dz < nz;
        const bool live = inside && (int)cls[i + dx + (int64_t)nx * dy + P * dz] != S->ident;
        const double v = t[cls_pos(s)];
        good = good && (live ? __double_as_longlong(v) == __double_as_longlong(S->c[s]) : v == 0.0);
    }
    if (!good) S->ok = 0;
}

// --- the classification (per solve, after the slot arrays got their final values)
__device__ __forceinline__ unsigned long long cls_hash(const double *__restrict__ uvals, int64_t stride, int64_t i) {
    unsigned long long h = 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        unsigned long long v = (unsigned long long)__double_as_longlong(uvals[(int64_t)s * stride + i]);
        v *= 0xff51afd7ed558ccdull; v ^= v >> 32;
        h = (h ^ v) * 0xc4ceb9fe1a85ec53ull; h ^= h >> 29;
    }
    return h ? h : 1ull;
}

struct ClsScratch {
    unsigned long long keys[CLS_SLOTS];     // 0 = empty
    int rep[CLS_SLOTS];                     // lowest row with that key
    int id[CLS_SLOTS];                      // class id of the slot (rank of its rep row)
    int info[4];                            // [0] distinct keys, [1] != 0: no dictionary (too many classes / a hash collision)
};

__global__ __launch_bounds__(TPB) void k_cls_insert(const double *__restrict__ uvals, int64_t stride, int64_t nv, ClsScratch *S) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (*(volatile int *)&S->info[1]) return;
    const bool active = i < nv;
    const unsigned long long h = active ? cls_hash(uvals, stride, i) : 0ull;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {                                          // one insertion per distinct key of the wavefront
        if (*(volatile int *)&S->info[1]) return;           // too many classes already: no point in probing a full table
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned long long h0 = __shfl(h, leader);
        todo &= ~__ballot(active && h == h0);
        if (lane != leader) continue;
        int slot = (int)(h0 & (CLS_SLOTS - 1));
        for (int probe = 0; probe < CLS_SLOTS; ++probe, slot = (slot + 1) & (CLS_SLOTS - 1)) {
            unsigned long long k = *(volatile unsigned long long *)&S->keys[slot];
            if (k == 0ull) {
                k = atomicCAS(&S->keys[slot], 0ull, h0);
                if (k == 0ull) {
                    k = h0;
                    if (atomicAdd(&S->info[0], 1) + 1 > CLS_MAX) atomicExch(&S->info[1], 1);
                }
            }
            if (k == h0) {
                if (*(volatile int *)&S->rep[slot] > (int)i) atomicMin(&S->rep[slot], (int)i);
                break;
            }
        }
    }
}

// class ids in the order of the representative rows (deterministic), the table in the products' layout
__global__ __launch_bounds__(CLS_SLOTS) void k_cls_table(const double *__restrict__ uvals, int64_t stride, ClsScratch *S,
                                                          double *__restrict__ table) {
    __shared__ int s_rep[CLS_SLOTS];
    const int t = threadIdx.x;
    const bool used = S->keys[t] != 0ull;
    s_rep[t] = used ? S->rep[t] : 0x7fffffff;
    __syncthreads();
    if (S->info[1]) return;
    int rank = 0;
    for (int k = 0; k < CLS_SLOTS; ++k) rank += (s_rep[k] < s_rep[t]) ? 1 : 0;
    S->id[t] = used ? rank : -1;
    if (used && rank <= CLS_MAX) {
#pragma unroll
        for (int s = 0; s < 8; ++s) table[rank * 8 + cls_pos(s)] = uvals[(int64_t)s * stride + s_rep[t]];
    }
    if (t < 8) table[min(S->info[0], CLS_MAX) * 8 + t] = 0.0;        // the zero class
}

__global__ __launch_bounds__(TPB) void k_cls_assign(const double *__restrict__ uvals, int64_t stride, int64_t nv, ClsScratch *S,
                                                    const double *__restrict__ table, uint8_t *__restrict__ cls) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= nv || S->info[1]) return;
    const unsigned long long h = cls_hash(uvals, stride, i);
    int slot = (int)(h & (CLS_SLOTS - 1)), id = -1;
    for (int probe = 0; probe < CLS_SLOTS; ++probe, slot = (slot + 1) & (CLS_SLOTS - 1)) {
        const unsigned long long k = S->keys[slot];
        if (k == h) { id = S->id[slot]; break; }
        if (k == 0ull) break;
    }
    bool same = id >= 0 && id <= CLS_MAX;
    if (same) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
            same = same && __double_as_longlong(uvals[(int64_t)s * stride + i]) == __double_as_longlong(table[id * 8 + cls_pos(s)]);
    }
    if (!same) { atomicExch(&S->info[1], 2); return; }       // two tuples under one key: keep the plain diagonal form
    cls[i] = (uint8_t)id;
}

// same[z] = 1 iff every row of plane z has the code of the row below it in plane z - 1 (same[0] = 0): the march keeps its
// couplings across such planes without looking at a code
__global__ __launch_bounds__(TPB) void k_cls_planes(const uint8_t *__restrict__ cls, int64_t plane, int nz, int *__restrict__ same) {
    __shared__ int s_diff;
    const int z = blockIdx.x;
    if (threadIdx.x == 0) s_diff = 0;
    __syncthreads();
    bool diff = z == 0;
    if (z > 0) {
        const uint8_t *a = cls + plane * z, *b = a - plane;
        for (int64_t i = threadIdx.x; i < plane; i += TPB) diff = diff || a[i] != b[i];
    }
    if (diff) s_diff = 1;
    __syncthreads();
    if (threadIdx.x == 0) same[z] = s_diff ? 0 : 1;
}

// ---- classification with known codes (Mesh::cls_cache)
__global__ void k_cls_table_known(const double *__restrict__ uvals, int64_t stride, int64_t nv, const int *__restrict__ reps, int ncls,
                                  double *__restrict__ table) {
    const int k = threadIdx.x;
    if (k < ncls) {
        const int64_t r = reps[k];
#pragma unroll
        for (int s = 0; s < 8; ++s) table[k * 8 + cls_pos(s)] = (r >= 0 && r < nv) ? uvals[(int64_t)s * stride + r] : 0.0;
    } else if (k == ncls) {
#pragma unroll
        for (int s = 0; s < 8; ++s) table[k * 8 + s] = 0.0;                 // the zero class
    }
}

__global__ __launch_bounds__(TPB) void k_cls_verify_known(const double *__restrict__ uvals, int64_t stride, int64_t nv,
                                                          const double *__restrict__ table, const uint8_t *__restrict__ cls, int ncls,
                                                          int *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= nv) return;
    const int k = cls[i];
    bool same = k < ncls;
    if (same) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
            same = same && __double_as_longlong(uvals[(int64_t)s * stride + i]) == __double_as_longlong(table[k * 8 + cls_pos(s)]);
    }
    if (!same) info[1] = 2;
}

struct ZeroPat { uint8_t b[256]; };

// the class-level relations of the stencil form for known codes: the identity tuple, and every class = the base tuple with
// exact zeros where (and only where) the structure - verified row by row when the codes were first seen - has them
// (`use`: the classes that occur on the verified planes - the incomplete ghost rows of a sharded slab have tuples of their own, which
// the full classification never holds against the stencil either: k_stencil_verify walks the verified planes only)
__global__ void k_stencil_known(const double *__restrict__ table, int ncls, int ident, int base, ZeroPat pat, ZeroPat use, StencilInfo *S) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int k = threadIdx.x;
    if (k < ncls && use.b[k]) {
        bool good = true;
        if (k == ident) {
            good = table[k * 8 + cls_pos(0)] == 1.0;
            for (int s = 1; s < 8; ++s) good = good && table[k * 8 + cls_pos(s)] == 0.0;
        } else {
            good = __double_as_longlong(table[k * 8 + cls_pos(0)]) == __double_as_longlong(table[base * 8 + cls_pos(0)]);
            for (int s = 1; s < 8; ++s) {
                const double v = table[k * 8 + cls_pos(s)];
                good = good && (((pat.b[k] >> s) & 1) ? v == 0.0
                                                      : __double_as_longlong(v) == __double_as_longlong(table[base * 8 + cls_pos(s)]));
            }
        }
        if (!good) s_bad = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        S->ok = s_bad ? 0 : 1; S->ident = ident; S->base = base; S->split = 0;
        for (int s = 0; s < 8; ++s) S->c[s] = table[base * 8 + cls_pos(s)];
    }
}

// after a full classification: a representative row per class, the zero patterns
__global__ __launch_bounds__(TPB) void k_cls_reps(const uint8_t *__restrict__ cls, int64_t nv, int *__restrict__ reps) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool active = i < nv;
    const int code = active ? (int)cls[i] : -1;
    // one atomic per distinct code of the wavefront (its lowest lane holds the lowest row), and none where the class already has
    // a representative further down: 16.7 M atomics on nine addresses took 188 ms
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(code, leader);
        todo &= ~__ballot(active && code == c0);
        if (lane == leader && reps[c0] > (int)i) atomicMin(&reps[c0], (int)i);
    }
}

// ------------------------------------------------------------------ the host side: dia_classify and its pieces
// One call: what the pieces share
struct ClsJob {
    Ctx *c; const Mesh *m; Csr *a;
    int64_t plane;                          // rows per plane
    int nzp, z_lo, z_hi, g;                 // planes of the grid, the planes the stencil is verified on, workgroups of a pass over all rows
    bool try_stencil, dbg_cls, dbg_stencil; // (PGD_DEBUG_CLS, PGD_DEBUG_STENCIL: read once per call)
    int scaled_key;                         // what besides the signature must match a remembered structure
    ClsScratch *S; StencilInfo *SI;         // on the device (Ctx::cls_scratch) ...
    int info[4]; StencilInfo si;            // ... and what the host read back of them
};

__attribute__((format(printf, 2, 3))) static void cls_debug(bool on, const char *fmt, ...) {
    if (!on) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

// per-plane flags (Csr::cls_same, ClsCache::same) in whole 64-byte lines
static size_t plane_flag_bytes(int nzp) { return ((size_t)nzp * sizeof(int) + 63) / 64 * 64; }

// ---- Mesh::cls_cache: at most four structures per mesh, least recently used out
constexpr size_t CLS_CACHE_MAX = 4, CLS_REPS_BYTES = 256 * sizeof(int);

// The entry's block and its views.  hipMalloc / hipFree, not the context's pool: a failure here must stay silent (dev_alloc records
// an error and, out of memory, synchronises the stream to empty the pool), and an entry lives as long as its mesh
static bool cls_cache_alloc(Mesh::ClsCache &E, int64_t nv, int nzp) {
    const size_t same_b = plane_flag_bytes(nzp);
    if (hipMalloc(&E.block, (size_t)nv + same_b + CLS_REPS_BYTES + 64 + PAD_BYTES) != hipSuccess) { E.block = nullptr; return false; }
    E.same = (int *)E.block;
    E.reps = (int *)((uint8_t *)E.block + same_b);
    E.codes = (uint8_t *)E.block + same_b + CLS_REPS_BYTES;
    return true;
}

static void cls_cache_touch(const Mesh *m, Mesh::ClsCache &E) { E.used = ++m->cls_clock; }

static void cls_cache_insert(const Mesh *m, Mesh::ClsCache &E) {
    cls_cache_touch(m, E);
    if (m->cls_cache.size() >= CLS_CACHE_MAX) {
        size_t old = 0;
        for (size_t e = 1; e < m->cls_cache.size(); ++e) if (m->cls_cache[e].used < m->cls_cache[old].used) old = e;
        m->cls_cache[old].release();
        m->cls_cache.erase(m->cls_cache.begin() + (long)old);
    }
    m->cls_cache.push_back(E);
}

// Key and buffers.  *go stays false where there is nothing to classify: no march on this grid anyway
static int cls_begin(ClsJob &J, Ctx *c, const Mesh *m, Csr *a, int zrange_lo, int zrange_hi, bool *go) {
    *go = false;
    if (!c->spmv_classes || m->sym_nx <= 0 || !(a->uvals && a->uvals_valid) || m->nv >= ((int64_t)1 << 31)) return PGD_OK;
    const int64_t plane = (int64_t)m->sym_nx * m->sym_ny;
    if (m->nv / plane < 3 || plane * 64 < c->spmv_grid_min_plane_bytes) return PGD_OK;
    if (m->nv / plane > 65536) return PGD_OK;                                // (plane flags of the stencil check: room for 2^16 planes)
    void *p;
    if (!c->cls_scratch) { PGD_TRY(dev_alloc(c, &p, sizeof(ClsScratch) + sizeof(StencilInfo) + 2 * 65536 * sizeof(int))); c->cls_scratch = p; }
    const int nzp = (int)(m->nv / plane);
    if (!a->cls) {
        const size_t table_b = (size_t)(CLS_MAX + 1) * 8 * sizeof(double), same_b = plane_flag_bytes(nzp);
        a->cls_bytes = (size_t)m->nv + table_b + same_b + 64;
        PGD_TRY(dev_alloc(c, &p, a->cls_bytes));
        a->cls_table = (double *)p;                          // the table first (aligned), then the plane flags, then the codes
        a->cls_same = (int *)((uint8_t *)p + table_b);
        a->cls = (uint8_t *)a->cls_same + same_b;
    }
    J.c = c; J.m = m; J.a = a;
    J.plane = plane; J.nzp = nzp;
    J.g = (int)((m->nv + TPB - 1) / TPB);
    J.z_lo = 0; J.z_hi = nzp;
    if (zrange_lo >= 0) { J.z_lo = std::max(0, zrange_lo); J.z_hi = std::min(nzp, zrange_hi); }
    J.S = (ClsScratch *)c->cls_scratch;
    J.SI = reinterpret_cast<StencilInfo *>(J.S + 1);
    J.try_stencil = c->spmv_stencil && J.z_hi - J.z_lo >= 3;
    J.scaled_key = (a->uvals_scaled ? 1 : 0) + (a->uvals_unit ? 2 : 0) + (J.try_stencil ? 4 : 0);
    J.dbg_cls = getenv("PGD_DEBUG_CLS") != nullptr;
    J.dbg_stencil = getenv("PGD_DEBUG_STENCIL") != nullptr;
    *go = true;
    return PGD_OK;
}

// the ONE place that writes the stencil fields of an operator
static void adopt_stencil(Csr *a, const StencilInfo &si, int z_lo, int z_hi) {
    a->st_ok = true;
    a->st_ident = si.ident;
    a->st_z0 = z_lo; a->st_z1 = z_hi;
    a->st_zm0 = si.zm0; a->st_zm1 = si.zm1;
    a->st_g_lo = si.g_lo != 0; a->st_g_hi = si.g_hi != 0;
    for (int s2 = 0; s2 < 8; ++s2) a->st_c[s2] = si.c[s2];
}

// The operator's slot values against the entry's structure: codes copied, table from the representative rows, EVERY row compared
// with its class bit by bit, then the class-level stencil relations.  One host synchronisation; the verdict in J.info / J.si
static int verify_known(ClsJob &J, const Mesh::ClsCache &E) {
    Ctx *c = J.c; const Mesh *m = J.m; Csr *a = J.a;
    hipStream_t st = c->stream;
    PGD_HIP(c, hipMemsetAsync(J.S->info, 0, sizeof J.S->info, st));
    PGD_HIP(c, hipMemcpyAsync(a->cls, E.codes, (size_t)m->nv, hipMemcpyDeviceToDevice, st));
    PGD_HIP(c, hipMemcpyAsync(a->cls_same, E.same, (size_t)J.nzp * sizeof(int), hipMemcpyDeviceToDevice, st));
    k_cls_table_known<<<1, 256, 0, st>>>(a->uvals, a->uvals_stride, m->nv, E.reps, E.ncls, a->cls_table);
    k_cls_verify_known<<<J.g, TPB, 0, st>>>(a->uvals, a->uvals_stride, m->nv, a->cls_table, a->cls, E.ncls, J.S->info);
    J.si.ok = 0;
    if (E.st_ok) {
        ZeroPat zp, use;
        memcpy(zp.b, E.zero_pat, sizeof zp.b);
        memcpy(use.b, E.in_range, sizeof use.b);
        k_stencil_known<<<1, 256, 0, st>>>(a->cls_table, E.ncls, E.ident, E.base, zp, use, J.SI);
        k_stencil_ghost_init<<<1, 1, 0, st>>>(J.SI, J.z_lo, J.z_hi, J.nzp, E.zm0, E.zm1);
        if (J.z_lo > 0 || J.z_hi < J.nzp)
            k_stencil_ghost<<<(int)((J.plane + TPB - 1) / TPB), TPB, 0, st>>>(a->cls, a->cls_table, m->sym_nx, m->sym_ny, J.z_lo, J.z_hi, E.zm0, J.SI);
    }
    J.info[1] = 1;
    PGD_HIP(c, hipMemcpyAsync(J.info, J.S->info, sizeof J.info, hipMemcpyDeviceToHost, st));
    if (E.st_ok) PGD_HIP(c, hipMemcpyAsync(&J.si, J.SI, sizeof(StencilInfo), hipMemcpyDeviceToHost, st));
    PGD_HIP(c, hipStreamSynchronize(st));
    PGD_LAUNCH_CHECK(c);
    if (E.st_ok) { J.si.zm0 = E.zm0; J.si.zm1 = E.zm1; }     // (the main run is the entry's: k_stencil_known leaves it alone)
    return PGD_OK;
}

// The mesh's first entry with the operator's key.  *hit: it verified, the operator has its classes; otherwise the entry - not
// that structure after all - is dropped and the caller classifies in full
static int classify_known(ClsJob &J, bool *hit) {
    Ctx *c = J.c; const Mesh *m = J.m; Csr *a = J.a;
    *hit = false;
    for (size_t e = 0; e < m->cls_cache.size(); ++e) {
        Mesh::ClsCache &E = m->cls_cache[e];
        if (E.sig != a->bc_sig || E.scaled != J.scaled_key || E.z_lo != J.z_lo || E.z_hi != J.z_hi || !E.codes) continue;
        PGD_TRY(verify_known(J, E));
        cls_debug(J.dbg_cls, "[dia_classify] known structure %zu of %zu: z %d..%d mismatches %d (info %d %d %d %d) stencil %d -> %d\n", e,
                  m->cls_cache.size(), J.z_lo, J.z_hi, J.info[1], J.info[0], J.info[1], J.info[2], J.info[3], (int)E.st_ok, J.si.ok);
        if (J.info[1] != 0 || (E.st_ok && !J.si.ok)) {
            E.release();
            m->cls_cache.erase(m->cls_cache.begin() + (long)e);
            return PGD_OK;
        }
        cls_cache_touch(m, E);
        c->cls_fast += 1;
        a->cls_count = E.ncls;
        if (E.st_ok) adopt_stencil(a, J.si, J.z_lo, J.z_hi);
        *hit = true;
        return PGD_OK;
    }
    return PGD_OK;
}

// Hash, table, codes and plane flags - and whether the classes are ONE stencil with eliminated nodes (k_spmv_stencil_march) on the
// planes [z_lo, z_hi): the whole grid, or the owned planes of a sharded rank's slab, whose ghost-plane rows are incomplete by
// construction.  One host synchronisation; a->cls_count > 0 afterwards where the dictionary exists, the stencil's verdict in J.si
static int classify_full(ClsJob &J) {
    Ctx *c = J.c; const Mesh *m = J.m; Csr *a = J.a;
    ClsScratch *S = J.S; StencilInfo *SI = J.SI;
    hipStream_t st = c->stream;
    const int g = J.g, nzp = J.nzp, z_lo = J.z_lo, z_hi = J.z_hi;
    c->cls_full += 1;
    PGD_HIP(c, hipMemsetAsync(S->keys, 0, sizeof S->keys, st));
    PGD_HIP(c, hipMemsetAsync(S->rep, 0x7f, sizeof S->rep, st));
    PGD_HIP(c, hipMemsetAsync(S->info, 0, sizeof S->info, st));
    k_cls_insert<<<g, TPB, 0, st>>>(a->uvals, a->uvals_stride, m->nv, S);
    k_cls_table<<<1, CLS_SLOTS, 0, st>>>(a->uvals, a->uvals_stride, S, a->cls_table);
    k_cls_assign<<<g, TPB, 0, st>>>(a->uvals, a->uvals_stride, m->nv, S, a->cls_table, a->cls);
    if (J.try_stencil) {
        k_stencil_pick<<<1, 64, 0, st>>>(a->cls, a->cls_table, S->info, m->sym_nx, m->sym_ny, z_lo, z_hi, SI);
        k_stencil_split<<<g, TPB, 0, st>>>(a->cls, a->cls_table, S->info, m->sym_nx, m->sym_ny, m->nv, SI);
        k_stencil_commit<<<1, 64, 0, st>>>(a->cls_table, S->info, SI);
    }
    k_cls_planes<<<nzp, TPB, 0, st>>>(a->cls, J.plane, nzp, a->cls_same);
    if (J.try_stencil) {
        const int64_t rows = J.plane * (z_hi - z_lo);
        k_stencil_verify<<<(int)((rows + TPB - 1) / TPB), TPB, 0, st>>>(a->cls, a->cls_table, m->sym_nx, m->sym_ny, nzp, z_lo, z_hi, SI);
        int *allid = reinterpret_cast<int *>(SI + 1);
        k_stencil_allid<<<nzp, TPB, 0, st>>>(a->cls, J.plane, SI, allid, allid + 65536);
        k_stencil_planes<<<1, 64, 0, st>>>(allid + 65536, allid, z_lo, z_hi, SI);
        k_stencil_ghost_init<<<1, 1, 0, st>>>(SI, z_lo, z_hi, nzp, -1, -1);
        if (z_lo > 0 || z_hi < nzp)
            k_stencil_ghost<<<(int)((J.plane + TPB - 1) / TPB), TPB, 0, st>>>(a->cls, a->cls_table, m->sym_nx, m->sym_ny, z_lo, z_hi, -1, SI);
    }
    J.info[0] = 0; J.info[1] = 1; J.si.ok = 0;
    PGD_HIP(c, hipMemcpyAsync(J.info, S->info, sizeof J.info, hipMemcpyDeviceToHost, st));
    if (J.try_stencil) PGD_HIP(c, hipMemcpyAsync(&J.si, SI, sizeof(StencilInfo), hipMemcpyDeviceToHost, st));
    PGD_HIP(c, hipStreamSynchronize(st));
    PGD_LAUNCH_CHECK(c);
    // (an operator without classes - a variable coefficient - costs 0.55 ms at 256^3 here: the insert pass gives up as soon as the
    // 256th class appears)
    if (J.info[1] != 0 || J.info[0] <= 0 || J.info[0] > CLS_MAX) return PGD_OK;
    a->cls_count = J.info[0];
    cls_debug(J.dbg_stencil, "[dia_classify] classes %d info1 %d try %d ok %d ident %d base %d c = %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g  z [%d, %d)\n",
              J.info[0], J.info[1], (int)J.try_stencil, J.si.ok, J.si.ident, J.si.base, J.si.c[0], J.si.c[1], J.si.c[2], J.si.c[3], J.si.c[4],
              J.si.c[5], J.si.c[6], J.si.c[7], z_lo, z_hi);
    cls_debug(J.dbg_stencil, "[dia_classify] main run [%d, %d)\n", J.si.zm0, J.si.zm1);
    return PGD_OK;
}

// The entry's device side from a finished classification: codes and plane flags copied, a representative row per class; reps_rng:
// the representatives within the verified planes (the same kernel on that range, first), tab: the class table.  Two host
// synchronisations; false: a copy failed
static bool cls_cache_fill(const ClsJob &J, Mesh::ClsCache &E, int (&reps_rng)[256], double *tab) {
    const Mesh *m = J.m; const Csr *a = J.a;
    hipStream_t st = J.c->stream;
    bool okc = hipMemcpyAsync(E.codes, a->cls, (size_t)m->nv, hipMemcpyDeviceToDevice, st) == hipSuccess &&
               hipMemcpyAsync(E.same, a->cls_same, (size_t)J.nzp * sizeof(int), hipMemcpyDeviceToDevice, st) == hipSuccess &&
               hipMemsetAsync(E.reps, 0x7f, CLS_REPS_BYTES, st) == hipSuccess;
    if (okc) {
        const int64_t r0 = (int64_t)J.z_lo * J.plane, r1 = std::min<int64_t>((int64_t)J.z_hi * J.plane, m->nv);
        if (r1 > r0) k_cls_reps<<<(int)((r1 - r0 + TPB - 1) / TPB), TPB, 0, st>>>(a->cls + r0, r1 - r0, E.reps);
        okc = hipMemcpyAsync(reps_rng, E.reps, sizeof reps_rng, hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipStreamSynchronize(st) == hipSuccess && hipMemsetAsync(E.reps, 0x7f, CLS_REPS_BYTES, st) == hipSuccess;
    }
    if (okc) {
        k_cls_reps<<<J.g, TPB, 0, st>>>(a->cls, m->nv, E.reps);
        okc = hipMemcpyAsync(tab, a->cls_table, (size_t)(E.ncls + 1) * 8 * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
              hipStreamSynchronize(st) == hipSuccess;
    }
    return okc;
}

// Remember the structure for the next operator with this signature.  A failed allocation or copy is swallowed: the solve goes on
// without an entry
static void remember(const ClsJob &J) {
    const Csr *a = J.a;
    const int ncls = a->cls_count;
    Mesh::ClsCache E;
    E.sig = a->bc_sig; E.scaled = J.scaled_key; E.z_lo = J.z_lo; E.z_hi = J.z_hi; E.ncls = ncls;
    if (!cls_cache_alloc(E, J.m->nv, J.nzp)) { (void)hipGetLastError(); return; }
    double tab[(CLS_MAX + 1) * 8];
    int reps_rng[256];
    if (!cls_cache_fill(J, E, reps_rng, tab)) {
        E.release();
        (void)hipGetLastError();
        return;
    }
    E.st_ok = a->st_ok; E.ident = a->st_ident; E.base = J.try_stencil ? J.si.base : -1; E.zm0 = a->st_zm0; E.zm1 = a->st_zm1;
    for (int k = 0; k < 256; ++k) E.in_range[k] = (k < ncls && reps_rng[k] >= 0 && reps_rng[k] < 0x7f000000) ? 1 : 0;
    for (int k = 0; k < 256; ++k) {
        uint8_t b = 0;
        if (k < ncls) for (int s2 = 1; s2 < 8; ++s2) if (tab[k * 8 + cls_pos(s2)] == 0.0) b |= (uint8_t)(1u << s2);
        E.zero_pat[k] = b;
    }
    // (a structural zero of the BASE tuple itself is no pattern bit: such a slot is compared with the base value)
    if (E.base >= 0) for (int k = 0; k < ncls; ++k) E.zero_pat[k] &= (uint8_t)~E.zero_pat[E.base];
    cls_cache_insert(J.m, E);
}

// Row classes of the operator's CURRENT slot values (a->uvals, diagonal form).  a->cls_count > 0 afterwards when the
// dictionary exists; any later change of the slot values must drop it (Csr::drop_classes: sym_scale, combine_dia, ensure_sym do).
int dia_classify(Ctx *c, const Mesh *m, Csr *a, int zrange_lo, int zrange_hi) {
    a->drop_classes();
    ClsJob J;
    bool go = false, hit = false;
    PGD_TRY(cls_begin(J, c, m, a, zrange_lo, zrange_hi, &go));
    if (!go) return PGD_OK;
    if (c->cls_cache_on) PGD_TRY(classify_known(J, &hit));
    if (hit) return PGD_OK;
    PGD_TRY(classify_full(J));
    if (a->cls_count <= 0) return PGD_OK;                    // no dictionary: the plain diagonal form
    if (J.try_stencil && J.si.ok) adopt_stencil(a, J.si, J.z_lo, J.z_hi);
    if (c->cls_cache_on) remember(J);
    return PGD_OK;
}

}  // namespace pgd
