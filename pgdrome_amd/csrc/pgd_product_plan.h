// Which kernel family runs a product with an operator held in symmetric storage, and the launch shape that kernel gets: decided HERE, once,
// from the operator's state and the knobs.  launch_spmv_op launches what the plan says; the predicates of the solves and the update launchers
// of the single-sync recurrence query the same plan.  plan_product is pure: it classifies nothing, counts nothing, allocates nothing.
#pragma once

#include "pgd_internal.h"

#include <algorithm>

namespace pgd {

constexpr int DIAC_MAXCHUNK = 1024;    // planes per march of the dictionary march at most

enum { PLAN_NOT_BY_FORM = -1 };        // no valid symmetric storage (or no valid row range): CSR kernels and the lattice offers, launch_spmv_op
enum { MARCH_WY8 = 0, MARCH_WY4 = 1, MARCH_2 = 2, MARCH_3 = 3 };   // KC_DIA_MARCH: k_spmv_dia_march<8>, <4>, k_spmv_dia_march2, k_spmv_dia_march3

struct ProductPlan {
    int form = PLAN_NOT_BY_FORM;       // KC_SYM_ROWS, KC_DIA_ROWS, KC_DIA_MARCH, KC_DIAC_MARCH or KC_STENCIL_MARCH
    int variant = 0;                   // KC_DIA_MARCH: MARCH_*
    int nblk = 0;                      // blocks of 64 rows: the grid of the row kernels
    int wgs = 0;                       // workgroups of the launch = partial sums (pairs) it leaves
    int z0 = 0, z1 = 0, zchunk = 0, tiles_x = 0, tiles_y = 0;   // structured grids: planes of the row range, planes per march, tiles
    int rows_per_thread = 0, depth = 0;   // KC_STENCIL_MARCH: the kernel's RWT and plane fetches in flight
    bool six = false;                  // KC_DIAC_MARCH: six plane fetches in flight (three otherwise)
};

// Shape of a launch of k_spmv_stencil_march over `planes` planes of an nx x ny grid, `depth` plane fetches in flight.
struct StencilShape { int rows_per_thread, tiles_x, tiles_y, zchunk, wgs; };
inline StencilShape stencil_shape(const Ctx *c, int nx, int ny, int planes, int depth) {
    StencilShape sh;
    sh.tiles_x = (nx + 63) / 64;
    sh.tiles_y = (ny + 15) / 16;
    const int64_t slots = (int64_t)c->stencil_wg_per_cu * c->num_cu;
    // rows per thread: four; two where the launch is so thin that marches of four-row patches would be shorter than 8
    // planes (a z-slab of a sharded solve: 256 x 256 x 32 = 8 marches of 4 planes against 4 of 8) - PGD_TUNE_STENCIL_ROWS
    const int64_t marches4 = std::max<int64_t>(1, slots / ((int64_t)sh.tiles_x * sh.tiles_y));
    const int zc4 = (int)((planes + marches4 - 1) / marches4);
    sh.rows_per_thread = (c->stencil_rows == 2 || (c->stencil_rows == 0 && zc4 < 8 && ny >= 16 && c->spmv_zchunk_stencil <= 0 && c->stencil_depth != 6)) ? 2 : 4;
    if (sh.rows_per_thread == 2) sh.tiles_y = (ny + 7) / 8;
    // march length: every resident workgroup slot filled once (two workgroups per CU), whole groups of the fetch depth
    const int64_t tiles = (int64_t)sh.tiles_x * sh.tiles_y;
    const int64_t marches = std::max<int64_t>(1, slots / tiles);
    int zc = (int)((planes + marches - 1) / marches);
    if (c->spmv_zchunk_stencil > 0) zc = c->spmv_zchunk_stencil;
    sh.zchunk = std::max(depth, zc);                   // (an incomplete last group of steps idles behind the march's last plane)
    sh.wgs = (int)(((planes + sh.zchunk - 1) / sh.zchunk) * tiles);
    return sh;
}

// The plan of the product over the rows [r0, r1) (r1 < 0: all).  pcg_like: a PCG product (w = x) or a plain one (no dot) - the marches
// fuse no other dot.  depth > 0: the fetch depth of the stencil march whatever PGD_TUNE_STENCIL_DEPTH says (the update launchers: 3).
inline ProductPlan plan_product(const Ctx *c, const Mesh *m, const Csr *a, int64_t r0, int64_t r1, bool pcg_like, int depth = 0) {
    ProductPlan P;
    if (!(c->spmv_sym && m->sym_w && a->uvals_valid && a->uvals)) return P;
    if (r1 < 0) r1 = m->nv;
    if (r0 < 0 || r0 > r1 || r1 > m->nv) return P;
    P.wgs = P.nblk = (int)((r1 - r0 + 63) / 64);
    P.form = KC_SYM_ROWS;
    if (m->sym_nx <= 0) return P;
    // structured vertex grid: the operator is held in diagonal form
    const int64_t plane = (int64_t)m->sym_nx * m->sym_ny;
    const int nx = m->sym_nx, ny = m->sym_ny, nz = (int)(m->nv / plane);
    P.z0 = (int)(r0 / plane); P.z1 = (int)(r1 / plane);
    const int wy = c->spmv_variant <= 1 ? 8 : 4;        // patch rows (0: 4 waves x two rows per thread; 1: 8 waves; 2: 4 waves, one row)
    P.tiles_x = (nx + 63) / 64; P.tiles_y = (ny + wy - 1) / wy;
    // plane-aligned row range, PCG product (w = x) or plain product, planes large enough: the LDS march
    const int64_t tile_planes = (int64_t)P.tiles_x * P.tiles_y * (P.z1 - P.z0);
    int chunks = 0;             // marches per column of the plain z-march (0: row order)
    if (pcg_like && r0 % plane == 0 && r1 % plane == 0 && c->spmv_zchunk > 0 && plane * 64 >= c->spmv_grid_min_plane_bytes) {
        // planes per march: as long as the launch still has ~4 workgroups per CU (measured on z-slabs of the 256 x 256
        // grid, tools/bench_spmv_slab.py: 30 planes - the interior of an 8-GPU rank - 31.9 us marching 8 planes vs 41.4 us
        // in row order; a march of fewer than 3 planes pays its prologue too often, and a single plane - the boundary
        // launches of the sharded solve - is faster in row order: 7.1 vs 8-14 us)
        P.zchunk = (int)std::min<int64_t>(c->spmv_zchunk, tile_planes * (wy / 4) / (4 * (int64_t)c->num_cu));
        if (c->spmv_zchunk_force > 0) P.zchunk = c->spmv_zchunk_force;       // tests: the march on any grid size
        chunks = (P.zchunk >= 3 || c->spmv_zchunk_force > 0) ? (P.z1 - P.z0 + P.zchunk - 1) / P.zchunk : 0;
    }
    const int64_t gg = (int64_t)chunks * P.tiles_x * P.tiles_y;
    P.form = KC_DIA_ROWS;
    if (!(gg > 0 && gg < ((int64_t)1 << 30))) return P;
    const int wgs = (int)gg;
    bool coded = c->spmv_variant == 0 && c->spmv_classes && a->cls_count > 0;
    int wgs_c = wgs, zchunk_c = P.zchunk;
    if (coded && c->spmv_zchunk_force <= 0) {
        // the coded march is unrolled six (three) planes at a time and its steps are light: longer marches (fewer halo planes
        // and prologues per row; 256^3: 24 planes 81 us, 12 planes 89 us, 6 planes 103 us), in whole sixes (threes)
        // (about one workgroup per CU is enough for this kernel - 128^3: marches of 18 planes = 256 workgroups 61.6 passes/s of
        // cfg3, 12 planes 59.9, 3 planes (four workgroups per CU, the rule of the plain march) 55.7, 24 planes 58.4)
        zchunk_c = (int)std::min<int64_t>(c->spmv_zchunk_coded, (tile_planes + c->num_cu / 2) / (int64_t)c->num_cu);
        zchunk_c = zchunk_c >= 9 ? std::max(12, (zchunk_c + 3) / 6 * 6) : std::max(3, zchunk_c / 3 * 3);
        // Large grids: a CU holds TWO of these workgroups (246 VGPRs), so with marches of 24 planes 256^3 is 1408 workgroups on
        // 512 slots - 2.75 rounds, the last one three quarters empty, and eleven prologues per column.  Where there is work for
        // at least 24 planes per slot the march is as long as it takes to fill every slot exactly once: 256^3 = 4 marches of 66
        // planes = 512 workgroups, 71 -> 63 us per product (8.87 -> 9.15 passes/s; one workgroup per CU - marches of 126 planes -
        // 102 us; 36 planes 68 us, 48 planes 72 us: `PGD_TUNE=21=...` before this rule)
        // (slabs of the sharded solve, tools/bench_coded_march.py 256x256xNZ: 32 planes 21.0 -> 17.9 us with 4 marches of 9,
        // 64 planes 29.9 -> 25.5 us with 4 of 18, 128 planes 41 us with 4 of 36 against 45-46 us with 18 or 24: the rule holds
        // from about 8 planes per slot on; marches under 12 planes run three steps at a time)
        const int64_t per_slot2 = (tile_planes + c->num_cu) / (2 * (int64_t)c->num_cu);
        if (c->spmv_zchunk_coded2 > 0 && per_slot2 >= 8)
            zchunk_c = (int)std::min<int64_t>(c->spmv_zchunk_coded2, per_slot2 >= 12 ? (per_slot2 + 5) / 6 * 6 : (per_slot2 + 2) / 3 * 3);
        wgs_c = (P.z1 - P.z0 + zchunk_c - 1) / zchunk_c * P.tiles_x * P.tiles_y;
    }
    coded = coded && zchunk_c <= DIAC_MAXCHUNK;
    // one stencil + eliminated nodes (dia_classify verified every row of the planes this launch reads couplings of: its
    // own and the plane below its first): couplings in scalar registers, four rows per thread, no table
    // (tests force the march onto small grids with PGD_TUNE_SPMV_ZCHUNK_FORCE, which selects the dictionary kernel - unless
    // PGD_TUNE_SPMV_ZCHUNK_STENCIL names a march length for this one)
    // Every plane the launch READS - its own and one halo plane either way - must be a verified plane or lie outside the grid
    // (the kernel stages what is outside the verified planes as zeros: right for the rim of the grid, wrong for a ghost plane
    // of a sharded slab, whose rows hold the neighbour rank's x)
    // (... or a ghost plane whose eliminated nodes are the main planes': staged as data, k_stencil_ghost)
    const bool st_lower = P.z0 == 0 ? a->st_z0 == 0 : (P.z0 - 1 >= a->st_z0 || (P.z0 == a->st_z0 && a->st_g_lo));
    const bool st_upper = P.z1 == nz ? a->st_z1 == nz : (P.z1 + 1 <= a->st_z1 || (P.z1 == a->st_z1 && a->st_g_hi));
    if (coded && c->spmv_stencil && a->st_ok && (c->spmv_zchunk_force <= 0 || c->spmv_zchunk_stencil > 0) && st_lower && st_upper &&
        plane < ((int64_t)1 << 26)) {
        P.form = KC_STENCIL_MARCH;
        P.depth = depth > 0 ? depth : c->stencil_depth > 0 ? c->stencil_depth : 3;      // (six plane fetches in flight: no faster, 60 registers more)
        const StencilShape sh = stencil_shape(c, nx, ny, P.z1 - P.z0, P.depth);
        P.rows_per_thread = (sh.rows_per_thread == 2 && P.depth != 6) ? 2 : 4;          // (the march of depth 6 exists with four rows only)
        P.tiles_y = sh.tiles_y; P.zchunk = sh.zchunk; P.wgs = sh.wgs;
    } else if (coded) {
        // the operator has a row-class dictionary (dia_classify): one byte per row instead of the slot values
        P.form = KC_DIAC_MARCH;
        P.zchunk = zchunk_c; P.wgs = wgs_c;
        // six plane fetches in flight where the march is long enough to run in sixes (a light kernel is paced by the bytes
        // a CU keeps in flight), three otherwise
        P.six = zchunk_c >= 12 && zchunk_c % 6 == 0 && c->spmv_fetch_depth != 3;
    } else {
        P.form = KC_DIA_MARCH;
        P.wgs = wgs;
        if (c->spmv_variant == 0 && c->dia_march3 && (int64_t)64 * a->uvals_stride < ((int64_t)1 << 31) && plane < ((int64_t)1 << 27)) P.variant = MARCH_3;
        else P.variant = c->spmv_variant == 0 ? MARCH_2 : wy == 8 ? MARCH_WY8 : MARCH_WY4;
    }
    return P;
}

}  // namespace pgd
