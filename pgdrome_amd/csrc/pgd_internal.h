// Internal declarations shared by the translation units of libpgd_amd.so.
// gfx950 (MI355X) only: 64-lane wavefronts, 256 CUs in 8 XCDs, 160 KiB LDS/CU.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pgd_amd.h"

namespace pgd {

constexpr int WAVE = 64;
constexpr int TPB = 256;            // threads per workgroup everywhere (4 waves)
constexpr int MAX_VEC_BLOCKS = 2048;  // grid cap of the grid-stride vector kernels (8 per CU)
constexpr int N_XCD = 8;
constexpr int DICT_MAXP = 256;      // patterns a mesh may have for the column dictionary
constexpr int DICT_DLEN = 32;       // max row length representable (ints per pattern, 128 B)
constexpr size_t PAD_BYTES = 256;   // slack after every device array (vector over-reads)

// slots of the device scalar bank used by the library's own PCG loop
enum { S_PQ = 2, S_TOL2 = 5, S_DMIN = 7 /* smallest diagonal entry (scaled PCG) */, S_TMP = 8 /* ..15: batched functionals */ };   // 16..22: PCG r.z / r.r / b.b
// single-sync recurrence (pgd_pcg.hip; the stencil march's update epilogue reads them too)
enum { S1_RZ = 24, S1_RR = 25, S1_ALPHA = 26, S1_BETA = 27, S1_PQ = 28, S1_QQ = 29,
       S1_ALPHA_PREV = 40, S1_BETA_PREV = 41, S1_PEND = 42 };      // the lagged x update
enum { S1F_ALPHA = 44 /* +parity */, S1F_BETA = 46 /* +parity */, S1F_EXACT = 48 /* +parity */ };   // scalar step inside the update kernel
constexpr double LAG_MIN_BETA = 0.01;

struct Ctx;
void dev_release(Ctx *c, void *p, size_t bytes);   // back to the context's buffer pool

struct Obj {
    enum Kind { FREE = 0, VEC, MESH, CSR, BLOCK, POINTS } kind = FREE;
    Ctx *ctx = nullptr;
    uint64_t serial = 0;        // unique per object of a context (handles are recycled, serials are not): put_obj
    virtual ~Obj() {}
};

struct Vec : Obj {
    double *d = nullptr;
    int64_t n = 0;
    ~Vec() override { if (d) dev_release(ctx, d, (size_t)(n > 0 ? n : 1) * sizeof(double)); }
};

// k columns of n rows in one allocation, as fp32 or f64 (pgd_block.hip): column j starts at element j * stride; the rows past n
// of every column are zeros and are never written
struct Block : Obj {
    void *d = nullptr;
    int64_t n = 0, stride = 0;
    int k = 0, dtype = 0;       // PGD_BLOCK_F32 / PGD_BLOCK_F64
    size_t bytes = 0;
    ~Block() override { if (d) dev_release(ctx, d, bytes); }
};

struct Mesh : Obj {
    int gdim = 0, nvpc = 0;
    int ncomp = 1;              // > 1: blocked (vector-valued) layout over the scalar layout `base`: pattern only
    pgd_handle base = 0;
    int64_t nv = 0, nc = 0, nnz = 0;
    double *coords = nullptr;   // SoA: gdim arrays of nv doubles (coalesced per component)
    int4 *cells = nullptr;      // one 16-byte record per cell, unused lanes = -1 (cells of <= 4 nodes)
    int *cellsN = nullptr;      // flat records of nvpc nodes (P2 triangles: 6, P2 tetrahedra: 10)
    int *v2c_ptr = nullptr;     // nv+1
    int *v2c = nullptr;         // nc*nvpc, sorted per vertex
    int *row_ptr = nullptr;     // nv+1
    int *cols = nullptr;        // nnz, sorted per row
    int max_row = 0, kl = 0, ku = 0;
    // Column-index dictionary (lossless): FEM rows repeat a handful of RELATIVE column patterns
    // (cols[k] - row); when a mesh has <= DICT_MAXP of them every row stores a 2-byte pattern id
    // and k_spmv_csr_dict rebuilds its column ids from the table instead of streaming 4 B/entry.
    // Symmetric half storage (pgd_spmv.hip, k_spmv_sym): per relative pattern a 16-int record
    // [packed(ulen, llen, 8 x 3-bit lower slots), 7 upper offsets, 8 lower distances]; sym_w = 4 or 8 upper
    // slots (diagonal first) per row, 0 = the mesh does not qualify (rows longer than 8 + 7, or the slot of a
    // row in its lower neighbours' rows is not a function of its own pattern)
    int *sym_tab = nullptr;
    int sym_w = 0;
    // full structured vertex grid (row = x + nx y + nx ny z, every column a grid neighbour on one of eight diagonals;
    // 0: not one): the slot arrays are then in DIAGONAL form - slot dx + 2 dy + 4 dz of row i = a(i, i + dx + nx dy + nx ny dz)
    // - and the products are k_spmv_dia_march / k_spmv_dia_rows (pgd_spmv.hip)
    int sym_nx = 0, sym_ny = 0;
    // the vertices sit on a uniform lattice origin + index * lat_h (checked at upload, pgd_mesh.hip): the P1 assembly takes
    // edge vectors as whole lattice steps, so congruent cells get identical local matrices
    bool lattice = false;
    bool lattice_unit = false;    // ... and every cell spans at most one step per axis: edge vectors from the vertex indices (k_lattice_cells_verify)
    // ... and the cells are numbered regularly: cell 6 q + t is tetrahedron t of cube q (cubes in vertex order), every cube cut the same way
    // (k_lattice_regular_verify): the cells around a vertex follow from its position - k_assemble_p1_regular gathers nothing
    bool lattice_regular = false;
    int pat_off[6][4] = {{0}};    // vertex offsets of tetrahedron t relative to its cube's first vertex
    int pat_loc[6][8] = {{0}};    // local index of cube corner (dx + 2 dy + 4 dz) in tetrahedron t, -1: not a vertex of it
    double lat_h[3] = {0.0, 0.0, 0.0};
    // What dia_classify learned about operators on this mesh (pgd_classify.hip): the class CODES of an operator depend on its atoms'
    // structure and its Dirichlet set, not on the coefficients it is combined with - every solve of a fixed-point pass classifies
    // "the same operator with other numbers".  A later classification with the same signature copies the codes, rebuilds the class
    // table from the representative rows and VERIFIES every row against its class bit by bit (+ the class-level stencil relations):
    // one pass over the slot values instead of three with hashing; any mismatch falls back to the full classification.
    // An entry owns ONE device allocation, `block`; same, reps and codes are views into it (cls_cache_alloc).  Entries are
    // copied around inside the vector: no destructor, whoever removes one calls release()
    struct ClsCache {
        uint64_t sig = 0; int scaled = 0, z_lo = 0, z_hi = 0, ncls = 0;
        void *block = nullptr;
        uint8_t *codes = nullptr; int *same = nullptr; int *reps = nullptr;
        bool st_ok = false; int ident = -1, base = -1, zm0 = 0, zm1 = 0;
        uint8_t zero_pat[256];      // per class: bit s = slot s is an exact zero (a coupling to an eliminated node / the rim)
        uint8_t in_range[256];      // per class: it occurs on the verified planes [z_lo, z_hi) (a slab's ghost rows carry classes of their own)
        uint64_t used = 0;          // Mesh::cls_clock at its last use: the least recently used entry makes room
        void release() { if (block) (void)hipFree(block); block = nullptr; codes = nullptr; same = reps = nullptr; }
    };
    mutable std::vector<ClsCache> cls_cache;
    mutable uint64_t cls_clock = 0;
    // the Dirichlet list of the last operator combined on this mesh (pgd_op_combine): every solve of a fixed-point pass brings the
    // same list again - compared on the host, word by word, it saves the range check, the upload (1.5 MB at 256^3) and the
    // host synchronisation behind it
    std::vector<int32_t> bc_host;
    int *bc_dev = nullptr;
    size_t bc_dev_bytes = 0;
    uint16_t *pids = nullptr;    // nv
    int *dict_off = nullptr;     // dict_count x DICT_DLEN relative offsets
    int dict_count = 0;          // 0: dictionary not available (irregular pattern) -> plain CSR kernel
    // A scalar P2 layout on tetrahedra bound to the box lattice of its vertices (pgd_mesh_p2_bind, pgd_pmg.hip): nodes 0 .. p2_nvert - 1
    // are the lattice's vertices in lattice order, every further node is the midpoint of an edge along one of the 14 pattern vectors.
    // p2_bound: 0 never asked, 1 bound, -1 refused (a check failed: solves under PGD_TUNE_PCG_PRECOND = 4 fall back)
    int p2_bound = 0;
    int p2_nx = 0, p2_ny = 0, p2_nz = 0;
    int64_t p2_nvert = 0;
    int *p2_par = nullptr;       // 2 arrays of nv ints: the two end vertices of a node's edge (equal for a vertex node)
    int *p2_v2e = nullptr;       // 14 arrays of p2_nvert ints: array t - 1 holds the node of the edge from a vertex along pattern vector t, -1: none
    // ... and whether the row-class form of pgd_p2lat.hip may be built on it: the edge list strictly ascending in (va, vb) with va < vb
    // (node ids ascend with the anchor vertex first, the class second), at least 3 vertices per axis.  0: no; otherwise the largest
    // component count (1..3) with ncomp * nv < 2^31
    int p2_lat = 0;
    // The bin index of pgd_points_locate (pgd_locate.hip, PGD_TUNE_LOCATE_INDEX) on a scalar 2-D or 3-D layout: a uniform grid of
    // n[0] n[1] n[2] bins over the bounding box, bin b holding the cells bin_cells[bin_ptr[b] .. bin_ptr[b + 1]).  Built by the first
    // indexed call, kept until the mesh goes, pgd_points_index_drop or a call under another PGD_TUNE_LOCATE_INDEX_TARGET
    struct LocIndex {
        bool built = false;
        int64_t builds = 0;          // since the mesh was uploaded or the index dropped
        int64_t target = 0;          // the knob's value it was built under
        double o[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
        int n[3] = {1, 1, 1};
        int *bin_ptr = nullptr;      // bins + 1
        int *bin_cells = nullptr;    // entries
        int64_t bins = 0, entries = 0, longest = 0;
        size_t bytes = 0;
        void release() {             // (the caller has synchronised the stream)
            if (bin_ptr) (void)hipFree(bin_ptr);
            if (bin_cells) (void)hipFree(bin_cells);
            bin_ptr = bin_cells = nullptr;
            built = false;
            bins = entries = longest = 0;
            bytes = 0;
        }
    };
    mutable LocIndex loc_index;
    ~Mesh() override {
        loc_index.release();
        for (void *p : {(void *)coords, (void *)cells, (void *)cellsN, (void *)v2c_ptr, (void *)v2c,
                        (void *)row_ptr, (void *)cols, (void *)pids, (void *)dict_off, (void *)sym_tab, (void *)p2_par, (void *)p2_v2e})
            if (p) (void)hipFree(p);
        for (ClsCache &e : cls_cache) e.release();
        if (bc_dev) (void)hipFree(bc_dev);
    }
};

struct Csr : Obj {
    pgd_handle mesh = 0;
    double *vals = nullptr;
    double *dinv = nullptr;    // lazily built inverse diagonal
    bool dinv_valid = false;
    // symmetric half storage of the same operator: sym_w arrays of nv doubles, slot s of row i at
    // uvals[s * nv + i] (slot 0 = diagonal, then the entries right of it; zero padded); on structured vertex grids
    // (Mesh::sym_nx > 0) the slots are the eight diagonals instead
    double *uvals = nullptr;
    bool uvals_valid = false;
    bool uvals_scaled = false;  // the slot arrays hold D^-1/2 A D^-1/2 (inside pgd_pcg_solve only)
    bool uvals_unit = false;    // ... in diagonal form, whose slot 0 is exactly 1 and is not loaded by the products
    int64_t uvals_stride = 0;  // doubles between two slot arrays (rows + padding)
    // row-class dictionary of the CURRENT slot values in diagonal form (dia_classify, pgd_classify.hip): a code per row and
    // the classes' slot tuples; cls_count = 0: none (every writer of the slot arrays calls drop_classes)
    uint8_t *cls = nullptr;
    int *cls_same = nullptr;       // per plane: same codes, row by row, as the plane below
    double *cls_table = nullptr;   // owns the allocation: table, then the codes
    int cls_count = 0;
    uint64_t bc_sig = 0;           // signature of the Dirichlet set the operator was combined with (a hint for Mesh::cls_cache)
    // the classes are ONE stencil + eliminated nodes on the planes [st_z0, st_z1) (dia_classify / k_stencil_verify): couplings
    // c[slot], identity class id; valid exactly as long as cls_count > 0
    bool st_ok = false;
    int st_ident = -1, st_z0 = 0, st_z1 = 0, st_zm0 = 0, st_zm1 = 0;   // (st_zm0 .. st_zm1: the run of planes with identical codes; the rest of the verified planes hold identity rows only)
    double st_c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool st_g_lo = false, st_g_hi = false;   // the plane below st_z0 / above st_z1 - 1 is a ghost DATA plane of a sharded slab (k_stencil_ghost)
    void drop_classes() { cls_count = 0; st_ok = false; st_g_lo = st_g_hi = false; }   // the slot values changed: no dictionary, no stencil
    bool st_virtual = false;       // st_c holds the couplings of D^-1/2 A D^-1/2 while slots, table and CSR values hold A (pgd_pcg_solve)
    bool cls_tried = false;        // atoms: the dictionary was looked for once for the current slot values (atom_fast_form)
    bool immutable = false;        // an ATOM (assembled / uploaded / embedded): its values change only through pgd_atom_embed(dst)
    uint64_t version = 0;          // bumped by every writer of `vals` after creation
    // pgd_op_combine on a structured grid forms the diagonal form only; the CSR values follow on first use (ensure_vals)
    // from this recipe: atoms by handle + serial + version (a freed or rewritten atom is an error, not a wrong product)
    bool vals_pending = false;
    std::vector<pgd_handle> rec_atoms;
    std::vector<uint64_t> rec_serials, rec_versions;
    std::vector<double> rec_coefs;
    int *rec_bc = nullptr;         // Dirichlet dofs of the combine (device copy)
    int64_t rec_nbc = 0;
    size_t rec_bc_bytes = 0;
    size_t vals_bytes = 0, dinv_bytes = 0, uvals_bytes = 0, cls_bytes = 0;
    // row-diagonal form of an operator on a blocked P1 layout over a box lattice (pgd_bdia.hip, PGD_TUNE_SPMV_BLOCK_DIA): 15 ncomp
    // arrays of bdia_stride doubles, array t * ncomp + d holds at row r = ncomp i + c the entry a(r, ncomp (i + off_t) + d), an exact
    // 0.0 where the row stores none.  It belongs to the values of `version` bdia_seen: bdia_ok says what was decided for them (the
    // form stands, or the operator keeps the CSR product); any other version has not been looked at yet
    double *bdia = nullptr;
    size_t bdia_bytes = 0;
    int64_t bdia_stride = 0;
    uint64_t bdia_seen = 0;
    bool bdia_ok = false;
    // row-class form of an operator on a P2 layout bound to a 3-D box lattice (pgd_p2lat.hip, PGD_TUNE_SPMV_P2_LATTICE): 65 ncomp arrays
    // of p2lat_sv doubles over the vertex rows, then 27 ncomp arrays of p2lat_se doubles over the edge rows; array s * ncomp + d holds
    // at its row the entry in slot s of the row's class table and column component d, an exact 0.0 where the row stores none.
    // Tied to `version` like bdia: p2lat_seen / p2lat_ok
    double *p2lat = nullptr;
    size_t p2lat_bytes = 0;
    int64_t p2lat_sv = 0, p2lat_se = 0;
    uint64_t p2lat_seen = 0;
    bool p2lat_ok = false;
    ~Csr() override {
        if (p2lat) dev_release(ctx, p2lat, p2lat_bytes);
        if (bdia) dev_release(ctx, bdia, bdia_bytes);
        if (rec_bc) dev_release(ctx, rec_bc, rec_bc_bytes);
        if (cls_table) dev_release(ctx, cls_table, cls_bytes);
        if (vals) dev_release(ctx, vals, vals_bytes);
        if (dinv) dev_release(ctx, dinv, dinv_bytes);
        if (uvals) dev_release(ctx, uvals, uvals_bytes);
    }
};

// Communication binding of a context for the row-sharded solve (pgd_comm.hip)
struct Comm {
    int kind = 0;                 // 0 none, 1 host callbacks, 2 RCCL
    int rank = 0, world = 1;
    pgd_halo_fn halo_cb = nullptr;
    pgd_allreduce_fn allreduce_cb = nullptr;
    void *user = nullptr;
    void *nccl = nullptr;         // ncclComm_t
    void *nccl_halo = nullptr;    // second communicator (ncclCommSplit) for the halo exchange on its own stream
    hipStream_t halo_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
    bool overlap = false;         // the halo exchange CAN run concurrently with the interior rows' product (second communicator + stream, self-test passed)
    // ... and does, in a solve whose ranks own at least this many rows on average.  Measured (tools/bench_self_periodic.py, one rank as
    // its own neighbour): the second stream costs two event hand-overs per iteration and LOSES 15 - 19 us against the exchange in
    // stream order + one march over all owned planes on the slabs of 8-, 4- and 2-GPU ranks of the 256^3 grid alike (72 / 92 / 130
    // against 54 / 75 / 114 us); what it can hide - a wire latency above that - is unknown here, so the default is "never" and
    // PGD_HALO_OVERLAP_MIN_ROWS / PGD_TUNE_HALO_OVERLAP_MIN_ROWS switch it on.  Decided from the all-reduced row count of the
    // setup vote: the same on every rank
    int64_t overlap_min_rows = (int64_t)1 << 40;
    bool overlap_used = false;    // what the last solve did
    bool self_periodic = false;   // tests only (PGD_TUNE_COMM_SELF_PERIODIC): ONE rank whose ghost planes are its own far boundary planes
    pgd_handle work[7] = {0, 0, 0, 0, 0, 0, 0};   // r, u, w, p, s, q, dinv of the sharded PCG
    int64_t work_n = 0;
    double timeout_s = 60.0;      // deadline of the host-side waits of the sharded solve (pgd_comm_timeout; <= 0: none)
    // boundary snapshots of the sharded loop (pinned): per slot 4 flag ints + the vote slot, and the event behind the copies
    int *snap_flags = nullptr;    // 2 x 4 ints
    double *snap_vote = nullptr;  // 2 doubles (same pinned allocation)
    hipEvent_t snap_ev[2] = {nullptr, nullptr};
    // phase timing (pgd_comm_prof): two sets of 7 markers, alternating with the parity of the chunk
    bool prof = false;
    hipEvent_t mark[2][7] = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
    bool mark_set[2] = {false, false};
    double prof_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // DIRECT halo of the sharded loop's search direction (pgd_comm_push_export / _attach; opt-in): the boundary planes of p are
    // stored straight into the neighbours' ghost planes through mapped pointers (hipIpcMemHandle; the rank itself where it is its
    // own neighbour) and a sequence number posted behind them; the product waits for the numbers of ITS ghost planes.  No RCCL
    // kernel in the iteration.  Geometry of the vector the export was made for: a solve with another one votes the exchange off.
    bool push = false;            // attached and self-tested
    bool push_used = false;       // what the last solve did
    int64_t push_n = 0, push_own0 = 0, push_own1 = 0, push_lo_g = 0, push_hi_g = 0;
    double *push_peer[2] = {nullptr, nullptr};                 // lower / upper neighbour's p (its base address in THIS process)
    int64_t push_peer_n[2] = {0, 0};                           // ... and its length: the upper ghost planes are its last rows
    unsigned long long *push_flags = nullptr;                  // own: [0] posted by the lower neighbour, [1] by the upper one, [2] ticket
    unsigned long long *push_peer_flags[2] = {nullptr, nullptr};
    void *push_mapped[4] = {nullptr, nullptr, nullptr, nullptr};   // what hipIpcOpenMemHandle returned (to close)
    unsigned long long push_seq = 0;
    // DIRECT all-reduce of the loop's five sums (pgd_comm_allreduce_attach; same opt-in, same flag block): every rank stores its sums
    // into every rank's mailbox - block + PUSH_BOX_OFF bytes: [parity][source rank][8 doubles] - posts the sequence number into
    // word PUSH_AR_FLAG0 + its rank of that block, waits for everybody's number in its own, and adds the contributions in rank
    // order: the same bits on every rank.  The iteration's local sums (k_pcg1_sums) are formed by the same kernel.
    bool ar = false, ar_used = false;
    unsigned long long *ar_peer[16] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *ar_mapped[16] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long ar_seq = 0;
};
constexpr int PUSH_BLOCK_BYTES = 4096, PUSH_AR_FLAG0 = 8, PUSH_BOX_OFF = 512, PUSH_AR_MAXW = 16;

// What the library counts per preconditioner cycle of pgd_pcg_solve (indexed by pgd_pcg_precond; the Jacobi entry stays zero) ...
struct CycleStats {
    int64_t solves = 0, fallbacks = 0;   // solves the cycle preconditioned; requests for it that took Jacobi instead
    int64_t marches = 0;                 // passes of its levels run in k_spmv_stencil_march / the z-march (not counted for the one-stencil cycle)
    double setup_ms = 0.0;               // time its setups took on the device, summed (not counted for the one-stencil cycle).  VMG: the Galerkin setups; CMG: extraction
                                         // of the diagonal blocks + their Galerkin setups; PMG: eliminated bytes + Galerkin blocks from the CSR values + their Galerkin chains
};
// ... and per product form that a knob switches on (PGD_TUNE_SPMV_BLOCK_DIA, PGD_TUNE_SPMV_P2_LATTICE)
struct FormStats {
    int64_t forms = 0, products = 0, fallbacks = 0;   // forms extracted, products launched from one, operators that kept the CSR product
    double extract_ms = 0.0;                          // time the extractions took on the device, summed
};
enum ProductForm { FORM_BDIA = 0, FORM_P2LAT = 1, FORM_COUNT = 2 };

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    std::vector<std::unique_ptr<Obj>> objs;   // handle = index + 1
    std::vector<int64_t> free_list;

    // Stream-ordered buffer pool: per-solve operators (2 GB) and work vectors (134 MB) are recycled
    // instead of paying hipMalloc/hipFree (~7 ms each) in every fixed-point pass.  Safe because all
    // work of a context is ordered on its one stream.
    std::multimap<size_t, void *> pool;
    size_t pool_bytes = 0;
    static constexpr size_t POOL_MAX = (size_t)24 << 30;

    double *slots = nullptr;      // PGD_NSLOTS doubles
    int *flags = nullptr;         // [0] done, [1] iters, [2] status
    double *partials = nullptr;   // reduction scratch
    int64_t partials_cap = 0;
    int64_t partials_off = 0;     // the product launchers write their partial sums from here on (several row ranges, one reduction)
    double *work[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t work_cap[7] = {0, 0, 0, 0, 0, 0, 0};
    uint8_t *mask = nullptr;      // Dirichlet column mask scratch
    int64_t mask_cap = 0;
    int *ibuf = nullptr;          // small int32 scratch (bc dofs, index lists)
    int64_t ibuf_cap = 0;
    // pgd_vec_set: the last index list and its values (host copies + what is on the device in ibuf / set_vals): the Dirichlet
    // values of every right-hand side of a fixed-point pass are the same 390 152 (index, value) pairs at 256^3
    std::vector<int32_t> set_idx_host;
    std::vector<double> set_val_host;
    int *set_idx = nullptr;
    double *set_vals = nullptr;
    int64_t set_idx_cap = 0, set_vals_cap = 0;
    int32_t set_idx_max = 0;
    bool set_idx_on_dev = false, set_val_on_dev = false;

    Comm comm;

    int num_cu = 256;
    int spmv_dict = 1;            // use the column dictionary when the mesh has one
    int spmv_rows = 64;           // rows (= threads) per k_spmv_csr workgroup: 64 (default), 128 or 256
    int64_t spmv_grid_min_plane_bytes = 0;   // structured grids whose planes of values are at least this large take the z-march (k_spmv_dia_march*)
    int spmv_zchunk_force = 0;    // > 0: exactly this many planes per march whatever the grid size (tests)
    int fault_iteration = -1;     // tests: pgd_pcg_solve_sharded fails on this rank in that iteration (once)
    int fault_stage = 0;          // tests: ... or at this stage of the solve outside the loop (PGD_TUNE_FAULT_STAGE), once
    int fault_stall_ms = 0;       // tests: ... or its stream stalls for this long in front of the first chunk (PGD_TUNE_FAULT_STALL_MS), once
    int64_t pcg_small_ss_rows = (int64_t)1 << 22;   // ... structured grids up to this many rows as well (PGD_TUNE_PCG_SMALL_ROWS; 128^3: +2 %, 256^3: a loss)
    int pcg_small_ss = 1;         // systems up to 2^20 rows: single-sync recurrence with the scalar step inside the update kernel (2 launches)
    int pcg_stream_hints = 1;     // single-sync recurrence: q, r, x non-temporal, p cached (PGD_TUNE_PCG_STREAM_HINTS)
    int pcg_lag_x = 1;            // single-sync recurrence: x is updated every other iteration, two terms at a time (PGD_TUNE_PCG_LAG_X)
    int pcg_recompute_q = 1;      // ... and on one-stencil grids A p is not stored: the update marches over p and forms it again (PGD_TUNE_PCG_RECOMPUTE_Q)
    int64_t pcg_recompute_launches = 0;   // launches of that update (k_spmv_stencil_march, EPI 3)
    int pcg_fold_march = 0;       // 1: every workgroup of it takes the scalar step itself, no k_pcg1_scalars launch (PGD_TUNE_PCG_FOLD_MARCH; measured: 0.3 ms of 48 per step, under the run-to-run spread - off)
    int64_t pcg_fused_launches = 0;       // launches of k_pcg1_fused_march (each is counted as an update and as a product as well)
    int pcg_fused_march = 1;      // 1: an iteration is k_pcg1_scalars + ONE march, the update with the next product's dots inside (k_pcg1_fused_march, PGD_TUNE_PCG_FUSED_MARCH; 256^3: 48.1 -> 45.0 ms per step)
    int pcg_scalar_s = 1;         // ... and divides by the two values s takes on such an operator instead of streaming it (PGD_TUNE_PCG_SCALAR_S)
    int asm_lattice = 1;          // lattice meshes: edge vectors as whole lattice steps in the assembly (PGD_TUNE_ASM_LATTICE)
    int spmv_fetch_depth = 6;     // plane fetches in flight per workgroup of k_spmv_diac_march2 (3 or 6; PGD_TUNE_SPMV_FETCH_DEPTH)
    int spmv_zchunk_coded2 = 96;  // ... and where every slot (two workgroups per CU) gets at least 24 planes: marches that fill the slots exactly once, at most this long (0: off)
    int spmv_zchunk_coded = 24;   // most planes per march of k_spmv_diac_march2 (PGD_TUNE_SPMV_ZCHUNK_CODED)
    int pcg_exact_phase = 1;      // sharded single-sync loop: the true r.r only near the end (one vector read per row less in the update)
    int pcg_fold_finish = 1;      // sharded single-sync loop: the scalar step inside the update kernel (one launch less per iteration)
    int atom_fast = 1;            // products with an atom whose diagonal form exists take the z-march (+ its own row classes, looked for once)
    int lazy_csr = 1;             // pgd_op_combine forms only the diagonal form where it can; CSR values on first use
    uint64_t next_serial = 1;
    int pcg_precond = 0;          // pgd_pcg_solve: 0 = Jacobi (the diagonal scaling), 1 = geometric multigrid V-cycle where the scaled operator is one
                                  // stencil on a lattice whose eliminated nodes are exactly its hull (pgd_mg.hip); anything else falls back to 0
    struct Mg *mg = nullptr;      // its levels and work vectors, kept across solves on the same lattice
    struct Mg *mg_slab = nullptr; // the same for a z-slab of a row-sharded lattice (pgd_mg_slab_*: levels >= 1 are whole and replicated)
    CycleStats cycle[PGD_PCG_PRECOND_PMG + 1];   // the counters behind pgd_{mg,vmg,cmg,pmg}_counts / _times
    struct Vmg *vmg = nullptr;    // pcg_precond = 2: the variable-coefficient hierarchy (pgd_vmg.hip), kept across solves on the same lattice
    struct Cmg *cmg = nullptr;    // pcg_precond = 3: one such hierarchy per component of a blocked P1 operator, kept across solves on the same lattice and ncomp
    struct Pmg *pmg = nullptr;    // pcg_precond = 4: one such hierarchy per component on P^T A P of a P2 operator over a bound box lattice (pgd_pmg.hip)
    // pgd_eval_batch (pgd_eval.hip): kernel variant (1 MFMA, 0 plain fma chains), grid cap and samples per launch (0: the launcher's choice);
    // the pinned staging of the coefficients in fragment order, two chunks deep, with the events behind the copies
    int eval_variant = 1, eval_grid_max = 0, eval_chunk = 0;
    int eval_norm_rows = 0, eval_norm_staged = -1;   // what the last pgd_eval_batch_norm ran with (pgd_eval_norm_last_shape)
    double *eval_pin = nullptr;
    size_t eval_pin_bytes = 0;
    hipEvent_t eval_ev[2] = {nullptr, nullptr};
    bool eval_ev_set[2] = {false, false};
    int mg_chunk = 2;             // iterations queued between two looks at the flags when the multigrid preconditioner is on (even: the slot parity of a replayed chunk)
    int mg_march_min = 64;        // levels with at least this many nodes along x and y run their stencil passes in k_spmv_stencil_march
    int cls_cache_on = 1;         // classification of an operator whose structure was seen before: codes copied, every row verified (PGD_TUNE_CLS_CACHE)
    int64_t cls_fast = 0, cls_full = 0;      // classifications served by the cache / done in full
    int spmv_stencil = 1;         // ... and its stencil form (couplings in scalar registers, four rows per thread) where every row verifies
    int spmv_zchunk_stencil = 0;  // > 0: planes per march of k_spmv_stencil_march (0: fill every workgroup slot once)
    int stencil_depth = 0;        // plane fetches in flight per workgroup of k_spmv_stencil_march (0: chosen from the march length; 3 or 6)
    int stencil_wg_per_cu = 2;    // resident workgroups per CU of k_spmv_stencil_march (sets the march length)
    int spmv_classes = 1;         // row-class dictionary of the scaled diagonal form (k_spmv_diac_march2) where the operator has one
    void *cls_scratch = nullptr;  // hash slots of dia_classify
    double *gram_w = nullptr;     // pgd_start_gram: the products A v_j, one vector each
    size_t gram_w_bytes = 0;
    pgd_handle gram_op = 0;       // ... of this operator, gram_k of them, each gram_n long (pgd_start_residual reads them; 0: none held)
    int gram_k = 0;
    int64_t gram_n = 0;
    int spmv_variant = 0;         // z-march: 0 = k_spmv_dia_march2 (64 x 8 patch, two rows per thread), 1 = 64 x 8 / 512 threads, 2 = 64 x 4 / 256 threads
    int spmv_zchunk = 8;          // k_spmv_dia_march: most planes a workgroup marches through (0: never use that kernel)
    int pcg_fold_reduce = 1;      // scaled recurrence: final reduction passes folded into the vector kernels (3 launches / iteration)
    int spmv_qq = 0;              // transient: the DIA products also leave y . y partial sums (pairs per workgroup)
    int pcg_single_sync = 1;      // scaled recurrence on structured grids above 2^20 rows: one reduction + one vector kernel per iteration
    int spmv_unit_diag = 1;       // scaled recurrence on structured grids: the unit diagonal is set to exactly 1 and not loaded
    int pcg_defer_x = 1;          // scaled recurrence, large systems: x += alpha p in the p kernel (8 vector passes per iteration, not 9)
    int pcg_scaled = 1;           // pgd_pcg_solve on the symmetrically scaled system (no dinv / z passes) when the symmetric storage applies
    int stencil_rows = 0;         // rows per thread of k_spmv_stencil_march: 0 = by the launch's shape (2 for thin slabs), 2, 4 (PGD_TUNE_STENCIL_ROWS)
    int dia_march3 = 0;           // 1: variant 0 of the plain z-march in k_spmv_dia_march3 (PGD_TUNE_DIA_MARCH3; bit-identical, measured 2 - 5 % slower at 256^3)
    int push_in_update = 1;       // direct halo: the boundary planes leave from the update kernel itself (PGD_TUNE_PUSH_IN_UPDATE); 0: k_halo_push
    int shard_one_march = 1;      // pgd_pcg_solve_sharded, exchange in stream order: all owned planes in one stencil march, ghost planes as data (PGD_TUNE_SHARD_ONE_MARCH)
    int pcg_derive_scaled = 1;    // ... whose stencil couplings are DERIVED from the verified stencil of A where that exists (PGD_TUNE_PCG_DERIVE_SCALED)
    int spmv_combine_dia = 1;     // structured grids: op_combine also forms the diagonal form from the atoms' diagonal forms
    int spmv_sym = 1;             // PCG products from the symmetric half storage when the mesh qualifies
    int spmv_block_dia = 0;       // 1: whole-range products of an operator on a blocked P1 layout over a 3-D box lattice from its row-diagonal form (k_spmv_bdia, PGD_TUNE_SPMV_BLOCK_DIA; bit-identical to k_spmv_csr)
    FormStats form[FORM_COUNT];   // the counters behind pgd_{bdia,p2lat}_counts / _times (p2lat: degree-2 operators that kept the CSR product)
    hipEvent_t bdia_ev[2] = {nullptr, nullptr};
    int spmv_p2_lattice = 0;      // 1: whole-range products of an operator on a P2 layout bound to a 3-D box lattice from its row-class form (k_spmv_p2lat, PGD_TUNE_SPMV_P2_LATTICE; bit-identical to k_spmv_csr)
    hipEvent_t p2lat_ev[2] = {nullptr, nullptr};
    uint16_t *p2lat_tab = nullptr; // class slot tables on the device (pgd_p2lat.hip), built once per context: (offset, class) of a slot ...
    int16_t *p2lat_slot = nullptr; // ... and the slot of (class, offset, class)
    int block_storage = 1;        // storage of the spectral start space (PGD_TUNE_BLOCK_STORAGE): 0 = f64 vectors, 1 = fp32 block, 2 = f64 block
    // pgd_points_locate (pgd_locate.hip): the one-thread-per-point path on regularly numbered box lattices (PGD_TUNE_LOCATE_LATTICE), the
    // grid cap of the general kernel (PGD_TUNE_LOCATE_GRID_MAX; 0: what is resident at once) and what the last call ran (pgd_points_last_path)
    int locate_lattice = 1, locate_grid_max = 0, locate_last_path = 0;
    int locate_index = 0;               // PGD_TUNE_LOCATE_INDEX
    int64_t locate_index_target = 0;    // PGD_TUNE_LOCATE_INDEX_TARGET
    // pgd_vec_gram (pgd_gram.hip): kernel variant (1 MFMA, 0 plain fma chains; PGD_TUNE_GRAM_VARIANT) and grid cap (PGD_TUNE_GRAM_GRID_MAX; 0: what is resident at once)
    int gram_variant = 1, gram_grid_max = 0;
    // pgd_quad_forms (pgd_quad.hip): kernel variant (1 MFMA, 0 plain fma chains; PGD_TUNE_QUAD_VARIANT) and grid cap (PGD_TUNE_QUAD_GRID_MAX; 0: what is resident at once)
    int quad_variant = 1, quad_grid_max = 0;
    // pgd_grid_misfit / pgd_grid_posterior (pgd_post.hip): kernel variants (1 MFMA, 0 plain fma chains; PGD_TUNE_MISFIT_VARIANT, PGD_TUNE_POST_VARIANT)
    // and grid caps (PGD_TUNE_MISFIT_GRID_MAX, PGD_TUNE_POST_GRID_MAX; 0: the launcher's choice)
    int misfit_variant = 1, misfit_grid_max = 0, post_variant = 1, post_grid_max = 0;
    // pgd_grid_posterior_many (pgd_postmany.hip): PGD_TUNE_POSTMANY_VARIANT, PGD_TUNE_POSTMANY_GRID_MAX, PGD_TUNE_POSTMANY_SKIP
    int postmany_variant = 1, postmany_grid_max = 0, postmany_skip = 1;
    // pgd_design_update / pgd_design_gains (pgd_design.hip): PGD_TUNE_DESIGN_VARIANT, PGD_TUNE_DESIGN_GRID_MAX
    int design_variant = 1, design_grid_max = 0;

    // SpMV launch timing (HIP events on `stream`)
    bool prof = false;
    bool prof_pcg_only = false;   // time only the PCG instance k_spmv_csr<dot,store>
    std::vector<hipEvent_t> ev;   // pairs
    // per pair: kind 0 = a product launch, 1 = the vector update of the single-sync recurrence; the bytes it is priced with; the
    // iteration of the PCG solve it belongs to (-1: not inside a solve's loop).  Launches queued behind the iteration that
    // converged are no-ops (every kernel returns on the done flag): their samples are dropped when the solve knows how far it
    // got (prof_commit), instead of entering the averages with full bytes and no time.
    struct ProfRec { uint8_t kind; int iter; double bytes, own, seconds; };
    std::vector<ProfRec> ev_rec;
    std::vector<ProfRec> prof_pend;   // measured, waiting for their solve's verdict
    int prof_iter = -1;               // iteration whose launches are being queued (set by the PCG loops)
    int64_t prof_dropped = 0;
    double prof_overhead = -1.0;      // seconds a pair of HIP events adds to the kernel it brackets (prof_calibrate; -1: not measured)
    size_t ev_used = 0;
    int64_t prof_upd_launches = 0, prof_upd_seen = 0;   // k_pcg1_update, timed like the products (one launch in four)
    double prof_upd_seconds = 0.0, prof_upd_bytes = 0.0;
    int64_t prof_launches = 0, prof_seen = 0;
    double prof_seconds = 0.0, prof_bytes = 0.0;
    double prof_own_bytes = 0.0;  // least bytes the kernels that were timed must move in their own storage form
    int64_t kcount[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // launches per product kernel family (KC_*)
    hipEvent_t timer_ev[2] = {nullptr, nullptr};     // pgd_timer_start / pgd_timer_stop
    int *flags_host = nullptr;                       // pinned: two snapshots of the device flags (the PCG loops look at one chunk's
    hipEvent_t flag_ev[2] = {nullptr, nullptr};      //   flags while the next chunk is already queued: pcg_flag_snapshots)
    int pcg_pipeline = 1;                            // 1: the next 16-iteration chunk is queued before the host looks at the flags of the last
    int pcg_last_form = -1, pcg_last_precond = -1;   // what the last pgd_pcg_solve ran (pgd_pcg_form / pgd_pcg_precond; pgd_pcg_last_form)
};

// the PCG loops name the iteration whose launches they queue (launch timing); on every way out of the solve it is "none" again
struct ProfIterGuard { Ctx *c; ~ProfIterGuard() { c->prof_iter = -1; } };
inline double host_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

enum { KC_CSR = 0, KC_CSR_DICT = 1, KC_SYM_ROWS = 2, KC_DIA_ROWS = 3, KC_DIA_MARCH = 4, KC_MULTI = 5, KC_DIAC_MARCH = 6, KC_STENCIL_MARCH = 7 };

// ---- helpers implemented in pgd_ctx.hip
Ctx *get_ctx(pgd_handle h);
int fail(Ctx *c, int code, const char *fmt, ...);
pgd_handle put_obj(Ctx *c, Obj *o);
Obj *get_obj(Ctx *c, pgd_handle h, Obj::Kind k);
int free_obj(Ctx *c, pgd_handle h, Obj::Kind k);
int dev_alloc(Ctx *c, void **p, size_t bytes);
int ensure_partials(Ctx *c, int64_t n);
int ensure_work(Ctx *c, int i, int64_t n);
int ensure_mask(Ctx *c, int64_t n);
int pcg_flag_snapshots(Ctx *c);                      // pgd_ctx.hip: the pinned flag buffers and their events exist
int ensure_ibuf(Ctx *c, int64_t n);
void prof_flush(Ctx *c);
void prof_commit(Ctx *c, int valid_products, int valid_updates);   // end of a solve: samples of iterations that ran are kept
void comm_release(Ctx *c);          // pgd_comm.hip
struct Mesh;
struct Csr;
int build_sym_tables(Ctx *c, Mesh *m);                       // pgd_spmv.hip
int ensure_sym(Ctx *c, const Mesh *m, Csr *a, bool *usable);  // pgd_spmv.hip: convert (once per operator)
int cg_init_s(Ctx *c, const double *b, const double *q, const double *sc, double *r, double *p, double *s, int64_t lo,
              int64_t hi, int base);                                   // pgd_pcg.hip: scaled sharded recurrence
int cg_update_s(Ctx *c, double *x, double *r, const double *w, double *p, double *s, const double *sc, int64_t lo, int64_t hi,
                int base);
int cg_update_s2(Ctx *c, double *x, double *r, const double *w, double *p, double *s, const double *sc, int64_t lo, int64_t hi,
                 int base, int parity, int *nblocks);
int reduce_two_slots(Ctx *c, int na, int nb, int base);
int pcg1_seed(Ctx *c, int npairs, int slot_rz, int slot_rr);          // single-sync recurrence, sharded form (pgd_pcg.hip)
int pcg1_tol(Ctx *c, int base, double rtol, double atol, int slot_p8);
int pcg1_aux(Ctx *c, const double *s, const double *r, int64_t lo, int64_t hi, int slot);
int pcg1_sums(Ctx *c, int nprod, int nvec, int base);
int pcg1_finish_slots(Ctx *c, int base);
// direct halo folded into the update (pgd_comm.hip): the rows [lo, lo_end) and [hi_begin, hi) of the new p also go - as write-through
// stores at system scope - to dst_lo / dst_hi, the workgroups that hold such rows take a ticket, the last one posts `seq` and polls
struct PushArgs {
    double *dst_lo = nullptr, *dst_hi = nullptr;
    int64_t lo_end = 0, hi_begin = 0;
    unsigned long long *post_lo = nullptr, *post_hi = nullptr;
    const unsigned long long *wait_a = nullptr, *wait_b = nullptr;
    unsigned long long seq = 0, *ticket = nullptr;
    unsigned int nblocks = 0;          // filled by pcg1_update: workgroups that take a ticket
    long long ticks = 0;
};
unsigned int pcg1_update_push_blocks(int g, int64_t lo, int64_t hi, int64_t lo_end, int64_t hi_begin);
int pcg1_update(Ctx *c, double *x, double *r, double *p, const double *q, const double *sc, int64_t lo, int64_t hi, int base,
                int *nblocks, int lag, int fold_par, const PushArgs *push = nullptr);
int pcg1_flush_x(Ctx *c, double *x, const double *p, const double *r, int64_t lo, int64_t hi, int base, int fold_par);
int vec_sqrt(Ctx *c, double *v, int64_t n);
int vec_div_mul(Ctx *c, double *x, const double *sc, int64_t n, int mul);
int ensure_vals(Ctx *c, const Mesh *m, Csr *a);                 // pgd_pcg.hip: CSR values of an operator whose combine was deferred
bool atom_fast_form(Ctx *c, const Mesh *m, Csr *a, int64_t r0, int64_t r1);   // pgd_spmv.hip
// pgd_classify.hip: row-class dictionary of the current slot values (+ its stencil form, verified on the planes [zlo, zhi) - whole grid: -1)
// A table row holds a class's slot values as [s1 s5 | s3 s7 | s2 s6 | s4 s0] (why: k_spmv_diac_march2, pgd_spmv.hip)
constexpr int CLS_MAX = 255;             // classes per operator (+ the zero class = 256 table rows of 64 B)
__host__ __device__ constexpr int cls_pos(int s) {      // position of slot s in a table row
    return s == 1 ? 0 : s == 5 ? 1 : s == 3 ? 2 : s == 7 ? 3 : s == 2 ? 4 : s == 6 ? 5 : s == 4 ? 6 : 7;
}
int dia_classify(Ctx *c, const Mesh *m, Csr *a, int zrange_lo = -1, int zrange_hi = -1);
bool stencil_row_range(const Ctx *c, const Mesh *m, const Csr *a, int64_t r0, int64_t r1);   // ... over the whole planes [r0, r1) of a slab
bool stencil_whole_grid(const Ctx *c, const Mesh *m, const Csr *a);   // pgd_spmv.hip: a product over all rows would run in k_spmv_stencil_march
// pgd_spmv.hip: the vector update of the single-sync recurrence as an epilogue of that march (stencil_whole_grid operators only): q = A p_in
// is formed in registers, x and r are updated in place, the new direction goes to p_out; one (r~.r~, true r.r) pair per workgroup in
// `pairs`, stencil_update_blocks of them.  s_free > 0: s is that number on every free row and 1 on the eliminated ones - it is not read.
// fold != nullptr: every workgroup takes the scalar step itself (StencilFold)
struct StencilFold {
    const double *prod; int nprod;      // the product's (p.q, q.q) pairs
    const double *vec_in; int nvec;     // the previous update's (r~.r~, true r.r) pairs: the other buffer than `pairs`
    int par;                            // parity of the iteration
};
int stencil_update_blocks(const Ctx *c, const Mesh *m, const Csr *a);
int launch_stencil_update(Ctx *c, const Mesh *m, const Csr *a, const double *p_in, double *p_out, double *x, double *r, const double *s,
                          double *pairs, int lag, double s_free = 0.0, const StencilFold *fold = nullptr);
// ... and with the dot-only product of the direction it writes in the same march (k_pcg1_fused_march): r is read from r_in and written
// to r_out, the product's (p.q, q.q) pairs go where launch_spmv_op leaves them.  stencil_fused_ok: the launch exists for this operator
bool stencil_fused_ok(const Ctx *c, const Mesh *m, const Csr *a);
int launch_stencil_fused(Ctx *c, const Mesh *m, const Csr *a, const double *p_in, double *p_out, double *x, const double *r_in, double *r_out,
                         const double *s, double *pairs, int lag, double s_free);
int launch_stencil_pass(Ctx *c, const uint8_t *cls, int ident, const double cst[8], int nx, int ny, int nz, int zm0, int zm1,
                        const double *x, const double *b, double *y, double w, int epi, bool dot, int *nparts, int z0 = 0, int z1 = -1);      // pgd_spmv.hip
// pgd_mg.hip: multigrid preconditioner of the scaled stencil operator
bool mg_prepare(Ctx *c, const Mesh *m, const Csr *a);                          // true: usable for this operator (levels built, buffers there)
int mg_fix_start(Ctx *c, const Csr *a, const double *b, double *x, int64_t n);    // x = b on the eliminated rows
int mg_vcycle(Ctx *c, const double *r, bool dot, int *nparts, double *z_out = nullptr);      // z = M r into z_out (default: mg_result(c)); partial sums of r.z into c->partials
double *mg_result(Ctx *c);
void mg_release(Ctx *c);
// pgd_vmg.hip: multigrid preconditioner of a scaled operator in diagonal form with per-row coefficients (PGD_TUNE_PCG_PRECOND = 2)
// (the functions take the hierarchy they work on: Ctx::vmg, or one component of Ctx::cmg)
struct Vmg;
bool vmg_prepare(Ctx *c, Vmg *&M, const Mesh *m, const Csr *a);                // true: usable for this operator (hierarchy formed from its current slot values)
int vmg_fix_start(Ctx *c, Vmg *M, const double *sc, const double *b, double *x, int64_t n);   // x = s b on the eliminated rows
int vmg_vcycle(Ctx *c, Vmg *M, const double *r, bool dot, int *nparts, double *z_out, int64_t *marches);
double *vmg_result(Vmg *M);
void vmg_note_setup(Ctx *c);
void vmg_release(Ctx *c);           // Ctx::vmg and Ctx::cmg
// ... and the component-wise cycle of a blocked P1 operator over such a lattice (PGD_TUNE_PCG_PRECOND = 3): z[c::ncomp] = s_c M_c (s_c r[c::ncomp])
bool cmg_prepare(Ctx *c, const Mesh *m, const Mesh *base, const Csr *a);       // true: usable (diagonal blocks extracted from the CSR values, hierarchies formed)
int cmg_fix_start(Ctx *c, const double *b, double *x, int64_t n);              // x = b on the dofs the component hierarchies have eliminated
int cmg_apply(Ctx *c, const double *r, double *z, int64_t n, int *nparts);     // partial sums of r . z into c->partials
void cmg_note_setup(Ctx *c);
// pgd_pmg.hip: p-multigrid for P2 operators over a bound box lattice (PGD_TUNE_PCG_PRECOND = 4): z = D^-1 r + P (M_c (P^T r)_c)_c with P the
// interpolation from P1 on the vertex lattice and M_c that V-cycle on the component's block of P^T A P
bool pmg_prepare(Ctx *c, const Mesh *m, const Csr *a);                         // true: usable (a->vals and a->dinv are current; blocks and hierarchies formed)
int pmg_fix_start(Ctx *c, const double *b, double *x, int64_t n);              // x = b on the eliminated dofs
int pmg_apply(Ctx *c, const Csr *a, const double *r, double *z, int64_t n, int *nparts);   // partial sums of r . z into c->partials
void pmg_note_setup(Ctx *c);
void pmg_release(Ctx *c);
void eval_release(Ctx *c);          // pgd_eval.hip: the pinned coefficient staging of pgd_eval_batch
int sym_scale(Ctx *c, const Mesh *m, Csr *a, const double *s);   // pgd_spmv.hip: slot values *= s_i s_j
int launch_spmv_dia_rows2(Ctx *c, const Mesh *m, const Csr *a, const double *x, double *y, const double *w, int64_t r0a,
                          int64_t r1a, int64_t r0b, int64_t r1b, bool dot, const int *flags, int *nparts_out, bool *done);
int combine_dia(Ctx *c, const Mesh *m, Csr *o, Csr *const *atoms, const double *coefs, int n, const uint8_t *mask);
int launch_spmv_op(Ctx *c, const Mesh *m, const Csr *a, const double *x, double *y, const double *w, int64_t r0,
                   int64_t r1, bool dot, bool store, const int *flags, int *nparts_out);
// pgd_bdia.hip: the product over all rows from the operator's row-diagonal form where the knob is on and the operator has or gets one
// (*done = true: launched); anything else leaves *done false for the CSR product, counted once per operator as a fallback
int launch_spmv_bdia(Ctx *c, const Mesh *m, Csr *a, const double *x, double *y, const double *w, bool dot, bool store,
                     const int *flags, int *nparts_out, bool *done);
// pgd_p2lat.hip: the same for an operator on a degree-2 layout and its row-class form (PGD_TUNE_SPMV_P2_LATTICE); p2lat_degree2: the
// layout is a P2 layout on simplices, scalar or blocked (the ones whose operators are counted)
bool p2lat_degree2(Ctx *c, const Mesh *m);
int launch_spmv_p2lat(Ctx *c, const Mesh *m, Csr *a, const double *x, double *y, const double *w, bool dot, bool store,
                      const int *flags, int *nparts_out, bool *done);
void p2lat_release(Ctx *c);
// pgd_spmv.hip: the launch-timing bracket of a product (HIP events around one launch in four)
int prof_begin(Ctx *c, bool dot, bool store, bool *timed);
int prof_end(Ctx *c, const Mesh *m, int64_t nrows, double own_per_row);

inline Vec *get_vec(Ctx *c, pgd_handle h) { return static_cast<Vec *>(get_obj(c, h, Obj::VEC)); }
inline Mesh *get_mesh(Ctx *c, pgd_handle h) { return static_cast<Mesh *>(get_obj(c, h, Obj::MESH)); }
inline Csr *get_csr(Ctx *c, pgd_handle h) { return static_cast<Csr *>(get_obj(c, h, Obj::CSR)); }
inline Block *get_block(Ctx *c, pgd_handle h) { return static_cast<Block *>(get_obj(c, h, Obj::BLOCK)); }

#define PGD_CTX(c, h)                         \
    pgd::Ctx *c = pgd::get_ctx(h);            \
    if (!c) return PGD_ERR_INVALID;           \
    (void)hipSetDevice(c->device)

// the bodies of the counter getters of the C ABI, one per record type (null pointers are skipped)
#define PGD_PUT(p, v) do { if (p) *(p) = (v); } while (0)
static inline int cycle_read(const CycleStats &s, int64_t *solves, int64_t *fallbacks, double *setup_ms, int64_t *march_passes) {
    PGD_PUT(solves, s.solves); PGD_PUT(fallbacks, s.fallbacks); PGD_PUT(setup_ms, s.setup_ms); PGD_PUT(march_passes, s.marches);
    return PGD_OK;
}
static inline int form_read(const FormStats &s, int64_t *forms_built, int64_t *products, int64_t *fallbacks, double *extract_ms) {
    PGD_PUT(forms_built, s.forms); PGD_PUT(products, s.products); PGD_PUT(fallbacks, s.fallbacks); PGD_PUT(extract_ms, s.extract_ms);
    return PGD_OK;
}

#define PGD_HIP(c, call)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return pgd::fail(c, PGD_ERR_HIP, "%s failed: %s (%s:%d)", #call,                \
                             hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

#define PGD_TRY(call)                \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != PGD_OK) return rc_; \
    } while (0)

#define PGD_LAUNCH_CHECK(c) PGD_HIP(c, hipGetLastError())

inline int grid_for(int64_t n, int per_block = TPB, int cap = MAX_VEC_BLOCKS) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// ---- what the dense products on v_mfma_f64_16x16x4_f64 share (pgd_eval, pgd_gram, pgd_quad, pgd_post, pgd_postmany, pgd_design)
typedef double d4_t __attribute__((ext_vector_type(4)));       // the accumulator of one instruction

// Dynamic LDS beyond 64 KiB has to be asked for, kernel by kernel (the attribute belongs to one instantiation); who: the call's name
inline int raise_lds(Ctx *c, const void *kern, size_t lds, const char *who) {
    if (lds <= 64 * 1024 || hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) return PGD_OK;
    (void)hipGetLastError();
    return fail(c, PGD_ERR_HIP, "%s: %zu bytes of LDS refused", who, lds);
}

// Workgroups of a persistent kernel over nitems work items: what is resident at once - `resident` workgroups per CU, or with
// resident = 0 the occupancy the runtime reports for this kernel, block and LDS size (1 where it reports none) - at most grid_cap
// (<= 0: no cap) and at most one per item
template <class... P>
int64_t persistent_grid(Ctx *c, void (*kern)(P...), int tpb, size_t lds, int64_t nitems, int64_t grid_cap, int resident = 0) {
    if (resident < 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, tpb, lds) != hipSuccess || resident < 1)) {
        (void)hipGetLastError();
        resident = 1;
    }
    int64_t g = (int64_t)c->num_cu * resident;
    if (grid_cap > 0 && g > grid_cap) g = grid_cap;
    return g < nitems ? g : nitems;
}

template <class... P, class... A>
int launch_grid(Ctx *c, void (*kern)(P...), int64_t g, int tpb, size_t lds, const A &...args) {
    kern<<<(int)g, tpb, lds, c->stream>>>(args...);
    PGD_LAUNCH_CHECK(c);
    return PGD_OK;
}

// ... both at once, for the callers whose buffers do not depend on the grid (it comes back in *grid_out, if asked for)
template <class... P, class... A>
int launch_persistent(Ctx *c, void (*kern)(P...), int tpb, size_t lds, int64_t nitems, int64_t grid_cap, int resident, int *grid_out,
                      const A &...args) {
    const int64_t g = persistent_grid(c, kern, tpb, lds, nitems, grid_cap, resident);
    if (grid_out) *grid_out = (int)g;
    return launch_grid(c, kern, g, tpb, lds, args...);
}

// k-steps of 4 of the instance for k modes: k <= 16, 32, 48, 64, 128, 256.  An instance holds T = 4, 4, 4, 4, 2, 1 tiles of 16 per
// wave: the B fragments are at most 64 doubles per lane
inline int dense_kt(int k) { return k <= 16 ? 4 : k <= 32 ? 8 : k <= 48 ? 12 : k <= 64 ? 16 : k <= 128 ? 32 : 64; }

// f(KT, T) for the instance of kt k-steps, both as std::integral_constant; KTMAX = 16: the callers that stop at 64 modes instantiate
// nothing beyond it
template <int KTMAX = 64, class F>
int dense_dispatch(int kt, F &&f) {
    static_assert(KTMAX == 16 || KTMAX == 64, "the instances end at 64 or at 256 modes");
    using std::integral_constant;
    switch (kt) {
        case 4: return f(integral_constant<int, 4>(), integral_constant<int, 4>());
        case 8: return f(integral_constant<int, 8>(), integral_constant<int, 4>());
        case 12: return f(integral_constant<int, 12>(), integral_constant<int, 4>());
    }
    if constexpr (KTMAX > 16) {
        if (kt == 32) return f(integral_constant<int, 32>(), integral_constant<int, 2>());
        if (kt != 16) return f(integral_constant<int, 64>(), integral_constant<int, 1>());
    }
    return f(integral_constant<int, 16>(), integral_constant<int, 4>());
}

// The A operand of a row-major block, nrows rows of k entries ld apart, in fragment order: kt k-steps of 4 per tile of 16 rows, lane
// (lq, lr) of k-step q of tile i reads entry (16 i + lr, 4 q + lq) at ((i kt + q) 64 + 16 lq + lr).  dst is zeroed by the caller
inline void pack_a_fragments(double *dst, int kt, const double *rows, int64_t nrows, int k, size_t ld) {
    for (int64_t p = 0; p < nrows; ++p) {
        double *f = dst + ((size_t)(p >> 4) * kt) * 64 + (p & 15);
        for (int t = 0; t < k; ++t) f[(size_t)(t >> 2) * 64 + ((t & 3) << 4)] = rows[(size_t)p * ld + t];
    }
}

inline size_t pool_bytes(size_t n_doubles) { return (n_doubles * sizeof(double) + 65535) & ~(size_t)65535; }   // (whole 64 KiB: the pool takes them back)

// The skeleton of a call whose inputs go up in one pooled buffer: run(p) queues the call's work and returns after its one
// synchronisation; after a failure the stream is drained first - nothing reads the inputs once they go back to the pool.  The caller
// writes its output arrays after this has returned PGD_OK
template <class F>
int with_pool_input(Ctx *c, size_t bytes, F &&run) {
    void *p = nullptr;
    PGD_TRY(dev_alloc(c, &p, bytes));
    const int rc = run(p);
    if (rc != PGD_OK) (void)hipStreamSynchronize(c->stream);
    dev_release(c, p, bytes);
    return rc;
}

// ---- launchers implemented across translation units
// pgd_vec.hip
int scan_exclusive_i32(Ctx *c, const int *in, int *out, int64_t n);   // out has n+1 entries
int reduce_partials(Ctx *c, const double *partials, int nparts, int nvals, int slot0, int check_mode,
                    int slot_rr, int slot_tol2);
int reduce_partials_to(Ctx *c, const double *partials, int nparts, int nvals, double *dest, int blocks = 1);   // blocks > 1: the values dealt over that many workgroups (same order per value)
int k_reduce_stage1_pub(Ctx *c, const double *partials, int nparts, int nvals, double *out);
int vec_dot_range(Ctx *c, const double *x, const double *y, int64_t lo, int64_t hi, int slot);
// pgd_spmv.hip
int launch_spmv(Ctx *c, const Mesh *m, const double *vals, const double *x, double *y,
                const double *w, int64_t r0, int64_t r1, bool dot, bool store, const int *flags,
                int *nparts_out);
int launch_spmv_multi(Ctx *c, const Mesh *m, const double *vals, const double *x,
                      const double *const *ys, int ny, int64_t r0, int64_t r1, double *out_host);
// pgd_pcg.hip
int csr_diag_inv(Ctx *c, const Mesh *m, Csr *a);

}  // namespace pgd

// ---- device helpers --------------------------------------------------------------
namespace pgd {

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an
// L2).  Give every XCD one contiguous chunk of the logical tile range so that
// neighbouring row blocks - which gather the same x planes - hit the same L2.
// Bijective for any grid size; placement only affects speed, never results.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, rem = nblk & 7, k = bid & 7;
    return k * q + (k < rem ? k : rem) + (bid >> 3);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The scalar step of the single-sync recurrence on values every thread holds (what pcg1_finish does on the scalar bank): the stop
// test on the residual the sums belong to, the switch to the exact phase, alpha and beta for the update that follows
struct Pcg1Scalars { double alpha, beta; int exact, done, status; double pq, qq, rz, rr; };
__device__ __forceinline__ void pcg1_local_step(Pcg1Scalars &S, const double *__restrict__ slots, int exact_cur) {
    S.alpha = S.beta = 0.0; S.exact = exact_cur; S.done = 0; S.status = 0;
    const double tol2 = slots[S_TOL2];
    if (!(S.rz == S.rz) || !(S.pq == S.pq)) { S.done = 1; S.status = PGD_ERR_SINGULAR; return; }
    if (exact_cur) { if (S.rr <= tol2) { S.done = 1; return; } }
    else if (S.rz * slots[S_DMIN] <= 1e4 * tol2) S.exact = 1;
    if (!(S.rz > 0.0)) { S.done = 1; return; }
    S.alpha = S.rz / S.pq;
    double rnew = S.alpha * S.alpha * S.qq - S.rz;
    if (!(rnew > 0.0)) rnew = 0.0;
    S.beta = rnew / S.rz;
}

// Sum over an NW-wave workgroup in a fixed order; result valid in thread 0.
template <int NW>
__device__ __forceinline__ double block_sum_n(double v, double *s_red /* >= NW */) {
    v = wave_sum(v);
    if (NW == 1) return v;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wv] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) t += s_red[k];
    }
    return t;
}

// Sum over a 256-thread workgroup in a fixed order; result valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double *s_red /* >= 4 */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wv] = v;
    __syncthreads();
    return (threadIdx.x == 0) ? ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) : 0.0;
}

}  // namespace pgd
