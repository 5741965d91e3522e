/*
 * pgd_amd.h - C ABI of the MI355X-native PGD fixed-point engine (libpgd_amd.so).
 *
 * This is the drop-in boundary for the hot path of BAMresearch/PGDrome:
 * PGDProblem.solve_PGD -> FP_solve -> one FEM assemble + solve per separated
 * dimension (reference pgdrome/solver.py:306-506, 508-881).  The reference has
 * no FFI of its own - it is pure Python that delegates every numeric step to
 * FEniCS (dolfin/PETSc/MUMPS).  Each entry point below therefore names the
 * reference call site(s) whose delegated native stage it replaces; the ctypes
 * binding a maintainer would add on the reference side is in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; all objects are opaque 64-bit handles (> 0 valid);
 *   - every function returns 0 (PGD_OK) or a negative error code, never throws
 *     or aborts across the ABI; pgd_last_error() gives the message;
 *   - host buffers are caller-owned, C-contiguous (f64 / i32) and are copied;
 *     device buffers are library-owned and freed by the matching *_free;
 *   - one context per device and process; calls on one context are serialised
 *     by the caller; all work is enqueued on the context's single HIP stream
 *     (the caller may hand in its own stream, e.g. torch's current stream, so
 *     RCCL collectives issued through torch.distributed order with it);
 *   - all arithmetic is float64, indices are int32 (nnz < 2^31 is checked).
 */
#ifndef PGD_AMD_H
#define PGD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t pgd_handle;

enum {
    PGD_OK = 0,
    PGD_ERR_INVALID = -1,   /* bad handle / argument / shape mismatch            */
    PGD_ERR_HIP = -2,       /* a HIP runtime call failed                         */
    PGD_ERR_NOMEM = -3,
    PGD_ERR_LIMIT = -4,     /* a structural limit was exceeded (row too long...) */
    PGD_ERR_SINGULAR = -5,  /* zero pivot / PCG breakdown                        */
    PGD_ERR_NODEVICE = -6,
    PGD_ERR_TIMEOUT = -7,   /* sharded solve: no progress on the stream within the deadline (pgd_comm_timeout)  */
    PGD_ERR_PEER = -8       /* sharded solve: another rank reported a rank-local failure; every rank leaves with an error */
};

/* element-matrix kinds ("atoms"); row = test, col = trial */
enum {
    PGD_ATOM_MASS = 0,    /* int u v                                              */
    PGD_ATOM_STIFF = 1,   /* int grad u . grad v                                  */
    PGD_ATOM_DUDV = 2,    /* int u_{,da} v_{,db}                                  */
    PGD_ATOM_CONV = 3,    /* int u_{,da} v        (time derivative term)          */
    PGD_ATOM_CONVT = 4,   /* int u v_{,db}                                        */
    PGD_ATOM_WMASS = 5,   /* int w u v,  w a P1 vertex field                      */
    PGD_ATOM_WSTIFF = 6,  /* int w grad u . grad v                                */
    PGD_ATOM_WDUDV = 7,   /* int w u_{,da} v_{,db}                                */
    PGD_ATOM_WCONV = 8,   /* int w u_{,da} v   (convection by a velocity field)   */
    PGD_ATOM_WCONVT = 9   /* int w u v_{,db}                                      */
};

/* ----------------------------------------------------------------- context --- */
/* stream: NULL -> the library creates its own HIP stream; otherwise a
 * hipStream_t owned by the caller.                                              */
int pgd_ctx_create(int device, void *stream, pgd_handle *ctx);
int pgd_ctx_destroy(pgd_handle ctx);
int pgd_sync(pgd_handle ctx);
const char *pgd_last_error(pgd_handle ctx);
int pgd_version(void);
int pgd_device_count(void);

/* ------------------------------------------------------------------ meshes --- */
/* Replaces dolfin's Mesh + DofMap + sparsity-pattern build behind
 * FunctionSpace(mesh,"CG",1) (callers: tests/integration/test_heat1D.py:26-40).
 * coords: nv x gdim row-major; cells: nc x nvpc.  P1: nvpc = gdim+1 simplex vertices.  P2
 * (FunctionSpace(mesh,"CG",2), tests/integration/test_elastic.py:33, test_laplace.py:880):
 * nvpc = 3 / 6 / 10 for gdim = 1 / 2 / 3; "coords" are the NODES (vertices and edge midpoints),
 * a cell record = its vertices followed by its edge nodes in the UFC local edge order
 * (interval: (v0, v1, mid); triangle edges (1,2),(0,2),(0,1); tetrahedron (2,3),(1,3),(1,2),
 * (0,3),(0,2),(0,1)); straight-sided geometry is taken from the vertices.
 * Builds on the device: vertex->cell adjacency (sorted) and the CSR pattern of
 * "vertices sharing a cell" with sorted columns.                                */
int pgd_mesh_upload(pgd_handle ctx, const double *coords, int64_t nv, int gdim,
                    const int32_t *cells, int64_t nc, int nvpc, pgd_handle *mesh);
/* Vector-valued Lagrange space on a scalar layout (VectorFunctionSpace(mesh,"P",k),
 * tests/integration/test_solver_problem.py:74): dof (node i, component c) = ncomp*i + c; the CSR
 * pattern couples all components of neighbouring nodes.  The result is a layout like any other
 * (vectors of ncomp*nv entries; pgd_op_combine, pgd_spmv, pgd_pcg_solve, ... apply unchanged); its atoms
 * are built from atoms of the scalar layout with pgd_atom_embed.                                 */
int pgd_mesh_blocked(pgd_handle ctx, pgd_handle scalar_mesh, int ncomp, pgd_handle *mesh);
/* Bind a scalar P2 layout on tetrahedra (nodes: the mesh vertices in their order, then one node per edge) to the box lattice of its
 * vertices, for PGD_TUNE_PCG_PRECOND = 4.  p1_mesh: the P1 layout of the same mesh - a 3-D lattice in diagonal form, which
 * supplies the lattice dimensions; edge_vertices: host, n_edges pairs of end vertices, edge e being node nv(p1) + e.  Checked on
 * the host: nv(p2) = nv(p1) + n_edges, every edge joins two vertices that differ by one of the 14 non-zero pattern vectors
 * +-(dx, dy, dz), d in {0,1}^3, and no (vertex, pattern vector) slot is taken twice.  *bound = 1: two parent ints per node and a
 * vertex -> edge-node table of 14 arrays are on the device; 0: a check failed - no error, the layout is remembered as refused and
 * its solves fall back.  Blocked layouts use the binding of their scalar layout.  A later call decides anew.
 * The CALLER guarantees that edge_vertices is the edge list of p2_mesh itself (edge e = its node nv(p1) + e, as its cell records
 * number them) and that p1_mesh holds its vertices: the cell connectivity is not compared with the list, and a consistent list
 * of another mesh of the same sizes would bind and give wrong blocks without raising the off-pattern flag.                   */
int pgd_mesh_p2_bind(pgd_handle ctx, pgd_handle p2_mesh, pgd_handle p1_mesh, const int32_t *edge_vertices, int64_t n_edges, int *bound);
int pgd_mesh_info(pgd_handle ctx, pgd_handle mesh, int64_t *nv, int64_t *nc, int64_t *nnz,
                  int32_t *max_row_len, int32_t *kl, int32_t *ku);
int pgd_mesh_pattern_download(pgd_handle ctx, pgd_handle mesh, int32_t *row_ptr, int32_t *cols);
/* number of distinct relative column patterns held in the mesh's column dictionary
 * (0: the pattern is too irregular, SpMV streams the column ids)                   */
int pgd_mesh_dict_count(pgd_handle ctx, pgd_handle mesh, int32_t *count);
/* Which form of the SPD product the mesh's patterns allow: slots = 0 (CSR kernels only), 4 or 8 upper slots
 * per row of the symmetric half storage (k_spmv_sym); nx, ny > 0 when the rows also form a full structured
 * vertex grid (row = x + nx y + nx ny z): k_spmv_dia_march2 / k_spmv_diac_march2 march along z with x planes in LDS. */
int pgd_mesh_sym_info(pgd_handle ctx, pgd_handle mesh, int32_t *slots, int32_t *nx, int32_t *ny);
/* *is_lattice = 1 when the mesh is a 3-D structured vertex grid whose coordinates are origin + index * steps[axis] to within
 * 8 ulp (see PGD_TUNE_ASM_LATTICE); steps: 3 doubles (zeros otherwise).                                       */
int pgd_mesh_lattice(pgd_handle ctx, pgd_handle mesh, int32_t *is_lattice, double *steps);
int pgd_mesh_free(pgd_handle ctx, pgd_handle mesh);

/* ----------------------------------------------------------------- vectors --- */
int pgd_vec_alloc(pgd_handle ctx, int64_t n, pgd_handle *vec);
int pgd_vec_free(pgd_handle ctx, pgd_handle vec);
int pgd_vec_size(pgd_handle ctx, pgd_handle vec, int64_t *n);
int pgd_vec_upload(pgd_handle ctx, pgd_handle vec, const double *host, int64_t offset, int64_t count);
int pgd_vec_download(pgd_handle ctx, pgd_handle vec, double *host, int64_t offset, int64_t count);
int pgd_vec_ptr(pgd_handle ctx, pgd_handle vec, void **device_ptr);
int pgd_vec_fill(pgd_handle ctx, pgd_handle vec, double value);
int pgd_vec_copy(pgd_handle ctx, pgd_handle dst, pgd_handle src);
/* dst[dst_off .. dst_off + count) = src[src_off .. src_off + count), on the stream (no synchronisation): cuts the sample-major
 * fields vector of pgd_eval_batch into vectors that own their storage.  PGD_ERR_INVALID for a range outside either vector or
 * overlapping ranges of one vector. */
int pgd_vec_copy_range(pgd_handle ctx, pgd_handle dst, int64_t dst_off, pgd_handle src, int64_t src_off, int64_t count);
int pgd_vec_scale(pgd_handle ctx, pgd_handle vec, double a);                 /* v *= a      */
int pgd_vec_mul(pgd_handle ctx, pgd_handle y, pgd_handle a, pgd_handle x);   /* y = a .* x entry by entry (y may be x or a): the Jacobi
                                                                               * scaling of the sharded BiCGStab, pgdrome_amd/dist.py */
int pgd_vec_axpy(pgd_handle ctx, pgd_handle y, double a, pgd_handle x);      /* y += a x    */
int pgd_vec_set(pgd_handle ctx, pgd_handle vec, const int32_t *idx, const double *val, int64_t n);
/* y = sum_k coefs[k] * xs[k]: the online reconstruction u = sum_k c_k F^k of a PGD solution
 * on its large dimension (replaces the numpy loop of model.py:822-842).  One launch per 64 terms, the fma chain from 0
 * through the terms in ascending order; no term may be y.                                                          */
int pgd_vec_lincomb(pgd_handle ctx, pgd_handle y, const pgd_handle *xs, const double *coefs, int k);
/* The same combination (same chain, same bits) where xs[0] may be y itself, k <= 64: y = coefs[0] y + sum_{t >= 1} coefs[t] xs[t]
 * in one launch - every entry of the terms is read before that entry of y is written.  The Galerkin start of a solve
 * (pgdrome_amd/fem.py: _rescale_start, in front of the solve that replaces solver.py:636,716) rewrites its first vector so.  */
int pgd_vec_lincomb_inplace(pgd_handle ctx, pgd_handle y, const pgd_handle *xs, const double *coefs, int k);
/* dot over [lo,hi) (hi < 0 -> whole vector); deterministic two-stage reduction.
 * Replaces Vector.inner / the Euclidean residual norm of solver.py:388.         */
int pgd_vec_dot(pgd_handle ctx, pgd_handle x, pgd_handle y, int64_t lo, int64_t hi, double *out);

/* ------------------------------------------------------------------- atoms --- */
/* Replaces FFC tabulate_tensor + dolfin Assembler for one bilinear "atom" on
 * one separated dimension (triggered from solver.py:636,716 and from every
 * dolfin.assemble inside the callbacks, e.g. test_heat1D.py:59-62).  Values
 * are laid out over the mesh's CSR pattern.  wvec: the nodal weight w of the
 * weighted kinds (WMASS, WSTIFF, WDUDV, WCONV, WCONVT), a vector of nv entries in
 * the layout's own space (P1 or P2, like u and v), 0 otherwise; a weighted kind
 * without it, or with a vector of another length, is PGD_ERR_INVALID.  One weight
 * per atom, never differentiated; weights of another Lagrange degree are the
 * caller's to interpolate.  P1 entries are closed forms (exact for a P1 weight),
 * P2 entries Gauss quadrature exact to degree 7 (the integrands reach degree 6).
 * Deterministic (owner-computes, no atomics).                                   */
int pgd_atom_assemble(pgd_handle ctx, pgd_handle mesh, int kind, int da, int db,
                      pgd_handle wvec, pgd_handle *atom);
/* The atom of pgd_atom_assemble (same kinds, weights, axis checks and kernels) over a subset of the cells:
 * int_Omega_s ... dx, the cell-subdomain integral dx(id) of a multi-material domain.  cell_mask: nc bytes in
 * the cell order of the upload, non-zero = the cell belongs to the subset; it is copied into a temporary
 * device buffer that is freed before the call returns.  The atom lies on the mesh's own pattern (entries that
 * no marked cell touches are exact zeros), so pgd_op_combine, pgd_spmv and pgd_atom_embed take it unchanged.
 * Every cell marked: bit-identical to pgd_atom_assemble; none: all zeros.  PGD_ERR_INVALID, with no atom left
 * behind, for nc other than the mesh's cell count, a blocked layout (pgd_atom_embed builds those from the
 * scalar atom) or cell_mask = NULL with nc > 0.  Deterministic (owner-computes, no atomics).             */
int pgd_atom_assemble_cells(pgd_handle ctx, pgd_handle mesh, int kind, int da, int db, pgd_handle wvec,
                            const uint8_t *cell_mask, int64_t nc, pgd_handle *atom);
/* The atom of pgd_atom_assemble_cells with a cell-wise constant (DG0) coefficient: sum over the cells c of
 * cvec[c] * (local matrix of c), the operator of  kappa * ... * dx  for a material field with one value per
 * cell.  cvec: a library vector of nc doubles in the cell order of the upload; it stays resident, so one field
 * serves every atom made from it.  The weight multiplies each finished local entry once as it is added - same
 * kinds, nodal weight wvec, axis checks, kernels and order of summation as pgd_atom_assemble (a cell weight,
 * unlike a nodal one, keeps the gather-free kernel of regular lattices: six weights per cube, 48 contiguous
 * bytes).  cell_mask: NULL = every cell, else nc bytes as in pgd_atom_assemble_cells; the weight of an
 * unmarked cell never enters.  The atom lies on the mesh's own pattern.  cvec = 1 everywhere: bit-identical to
 * pgd_atom_assemble (to pgd_atom_assemble_cells with a mask).  PGD_ERR_INVALID, with no atom left behind,
 * for nc other than the mesh's cell count, cvec not a vector of nc entries, a blocked layout, an unknown kind,
 * a weighted kind without wvec or an axis out of range.  Deterministic (owner-computes, no atomics).       */
int pgd_atom_assemble_cellwise(pgd_handle ctx, pgd_handle mesh, int kind, int da, int db, pgd_handle wvec,
                               pgd_handle cvec, const uint8_t *cell_mask, int64_t nc, pgd_handle *atom);
/* Boundary mass  int_Gamma phi_i phi_j ds  over nf facets (the Robin term c*u*v*ds of a form), on the
 * mesh's own pattern: an atom like any other.  facets: nf records of nvpf node ids of the layout, the
 * facet's vertices first, then for P2 the nodes of its edges in the UFC local order - interval layouts
 * nvpf = 1 (a point: 1 on the diagonal), triangle layouts 2 (P1) / 3 (P2) (an edge), tetrahedron layouts
 * 3 (P1) / 6 (P2) (a triangle).  Measures come from the vertex coordinates of the mesh.  PGD_ERR_INVALID
 * for a node out of range, nvpf not matching the layout, a blocked layout (pgd_atom_embed builds those
 * from the scalar atom) or a facet whose nodes the pattern does not couple (no atom is left behind).
 * Deterministic (owner-computes, no atomics).                                                    */
int pgd_atom_assemble_facets(pgd_handle ctx, pgd_handle mesh, const int32_t *facets, int64_t nf, int nvpf,
                             pgd_handle *atom);
/* dst[(ncomp*i + cv), (ncomp*j + cu)] += coef * src[i, j]: the scalar atom `src` (e.g. DUDV(a,b)) placed
 * in the (test component cv, trial component cu) block of an atom of the blocked layout.  dst = 0
 * creates a zero atom first; *out is the destination.  One term of inner(C*eps(u), eps(v))*dx
 * (test_solver_problem.py:127-150) is one call.                                                  */
int pgd_atom_embed(pgd_handle ctx, pgd_handle blocked_mesh, pgd_handle src, int cv, int cu, double coef,
                   pgd_handle dst, pgd_handle *out);
int pgd_atom_upload(pgd_handle ctx, pgd_handle mesh, const double *vals, pgd_handle *atom);
int pgd_atom_download(pgd_handle ctx, pgd_handle atom, double *vals);
int pgd_atom_free(pgd_handle ctx, pgd_handle atom);

/* --------------------------------------------------------------- operators --- */
/* A = sum_t coefs[t] * atoms[t] with symmetric Dirichlet elimination of
 * bc_dofs (rows and columns -> identity).  Replaces the per-solve global
 * re-assembly + DirichletBC.apply inside LinearVariationalSolver.solve()
 * (solver.py:627-636, 704-716).  *op == 0 allocates, otherwise the storage of
 * the existing operator (same mesh) is reused.  The result is an atom handle.   */
int pgd_op_combine(pgd_handle ctx, pgd_handle mesh, const pgd_handle *atoms, const double *coefs,
                   int n, const int32_t *bc_dofs, int64_t nbc, pgd_handle *op);

/* y[r0:r1) = (A x)[r0:r1)  (r1 < 0 -> all rows).  The gated kernel k_spmv_csr.  */
int pgd_spmv(pgd_handle ctx, pgd_handle A, pgd_handle x, pgd_handle y, int64_t r0, int64_t r1);
/* out = sum_{i in [r0,r1)} x_i (A y)_i.  Replaces assemble(F*A*G*dx) scalars
 * (callbacks; solver.py:443, 839-841) and dolfin.norm (solver.py:342,754,837).  */
int pgd_bilinear(pgd_handle ctx, pgd_handle A, pgd_handle x, pgd_handle y, int64_t r0, int64_t r1,
                 double *out);
/* out[m] = sum_i x_i (A y_m)_i for m < ny: one pass over A for a whole family of
 * stored modes (the O(n_enr) scalar functionals of rhs_fct, test_heat1D.py:141-165). */
int pgd_bilinear_many(pgd_handle ctx, pgd_handle A, pgd_handle x, const pgd_handle *ys, int ny,
                      int64_t r0, int64_t r1, double *out);

/* ----------------------------------------------------------------- solvers --- */
/* Jacobi-preconditioned CG, x holds the start vector and receives the solution.
 * Stops when ||r||_2 <= max(rtol ||b||_2, atol) on the TRUE residual (PETSc's CG tests the preconditioned
 * norm by default; the reference solves directly, so either is a tolerance on an exact answer).  Replaces
 * PETSc/MUMPS behind solver.solve() (solver.py:592-595, 633-636) for the SPD spatial systems.
 * Reaching maxit is NOT an error here (iters == maxit, relres > rtol: the caller decides - pgdrome_amd.fem raises
 * like dolfin's error_on_nonconvergence).  On an error return (a failing launch or copy in mid-loop) x is handed
 * back in its own coordinates, never in the scaled ones the recurrence works in, and the operator's symmetric
 * copy is dropped.                                                                                         */
int pgd_pcg_solve(pgd_handle ctx, pgd_handle op, pgd_handle b, pgd_handle x, double rtol,
                  double atol, int maxit, int *iters, double *relres);
/* Which recurrence and which preconditioner the last pgd_pcg_solve of this context ran (-1, -1 before the first one).  Both
 * are decided once per solve, from the operator and the PGD_TUNE_PCG_* knobs; every form computes the same iteration.   */
typedef enum {
    PGD_PCG_FORM_PRECOND = 0,               /* textbook recurrence around a multigrid cycle (see pgd_pcg_precond) */
    PGD_PCG_FORM_TEXTBOOK = 1,              /* unscaled Jacobi-PCG: no symmetric storage, or PGD_TUNE_PCG_SCALED = 0 */
    PGD_PCG_FORM_TWO_LAUNCH = 2,            /* single-sync, the scalar step inside the update (PGD_TUNE_PCG_SMALL_SINGLE_SYNC) */
    PGD_PCG_FORM_FOLDED = 3,                /* two reductions, folded into their consumers (PGD_TUNE_PCG_FOLD_REDUCE) */
    PGD_PCG_FORM_SINGLE_SYNC = 4,           /* one reduction + one vector update (PGD_TUNE_PCG_SINGLE_SYNC) */
    PGD_PCG_FORM_SINGLE_SYNC_RECOMPUTE = 5, /* ... whose update forms A p again (PGD_TUNE_PCG_RECOMPUTE_Q) */
    PGD_PCG_FORM_DEFERRED_X = 6,            /* two reductions, x += alpha p in the p kernel (PGD_TUNE_PCG_DEFER_X) */
    PGD_PCG_FORM_PLAIN = 7                  /* two reductions, scaled */
} pgd_pcg_form;
typedef enum {
    PGD_PCG_PRECOND_JACOBI = 0, PGD_PCG_PRECOND_MG = 1, PGD_PCG_PRECOND_VMG = 2, PGD_PCG_PRECOND_CMG = 3,
    PGD_PCG_PRECOND_PMG = 4
} pgd_pcg_precond;
int pgd_pcg_last_form(pgd_handle ctx, int *form, int *precond);
/* Banded LU with partial pivoting in one workgroup, for the small and possibly
 * non-symmetric 1-D systems (time: u'v) and the FD-mode solve (solver.py:939).  */
int pgd_band_solve(pgd_handle ctx, pgd_handle op, pgd_handle b, pgd_handle x);

/* ------------------------------------------------- distributed PCG pieces --- */
/* Row-sharded solve: the host drives the recurrence and places the RCCL halo
 * exchange / all-reduce between these calls (pgdrome_amd/dist.py).  Scalars
 * live in a device bank of PGD_NSLOTS doubles so nothing round-trips to the
 * host inside an iteration; every kernel is a no-op once the done flag is set.
 *
 * What holds for every piece below:
 *   - a row range [r0, r1) has 0 <= r0 <= r1 <= n; r1 < 0 means n.  Rows outside it are neither read for the sums nor written.
 *   - every slot index a piece takes must lie in [0, PGD_NSLOTS) - for the pieces that write two, three or nine consecutive
 *     slots, the last one as well.  Anything else is PGD_ERR_INVALID, like a bad range or vectors of different lengths: the
 *     call is refused before anything is launched, and slots, flags and vectors stay as they were.
 *   - an EMPTY range (r0 == r1) writes 0 into the slots of its sums - a caller all-reduces them unconditionally - unless the
 *     piece is a no-op because the done flag is set.
 *   - the done flag turns pgd_spmv_dot_slot, pgd_pcg_xr_slot, pgd_pcg_check_slot, pgd_pcg_p_slot, pgd_cg_update_slot and
 *     pgd_cg_scalars_slot into no-ops (vectors, slots and flags untouched).  pgd_pcg_init_slot, pgd_cg_init_slot and
 *     pgd_pcg_tol_slot act regardless: they start a solve (after pgd_flags_reset).
 *   - a NaN in a residual sum is a breakdown: done = 1, status = PGD_ERR_SINGULAR.
 *   - slots written besides the ones a call names - keep `slot`, `base` and the indices passed clear of them:
 *       S[5]        tol^2, by pgd_cg_scalars_slot(init = 1) (pgd_pcg_tol_slot writes the index it is given)
 *       S[6]        the last live r.r, by pgd_pcg_check_slot and pgd_cg_scalars_slot
 *       S[40..42]   scratch of pgd_cg_init_slot (overwritten with its three sums before they are placed)          */
#define PGD_NSLOTS 64
int pgd_slots_ptr(pgd_handle ctx, void **device_ptr);
int pgd_slots_download(pgd_handle ctx, double *out, int first, int count);
int pgd_slots_upload(pgd_handle ctx, const double *in, int first, int count);
int pgd_flags_reset(pgd_handle ctx);
int pgd_flags_download(pgd_handle ctx, int32_t *done, int32_t *iters, int32_t *status);
int pgd_op_diag_inv(pgd_handle ctx, pgd_handle op, pgd_handle dinv);
/* Build the symmetric half storage of an SPD operator for the products of a host-driven solve
 * (the library solves do this themselves): *used = 1 if the mesh's patterns qualify and
 * a_ij == a_ji held to rounding, else 0 and the CSR kernels stay in use.          */
int pgd_op_symmetrize(pgd_handle ctx, pgd_handle op, int *used);
/* Which storage form a product with this ATOM reads right now: 0 = the CSR kernels, 1 = the z-march over its diagonal form,
 * 2 = the z-march over its row-class dictionary (one code byte per row).  Forms 1 / 2 exist on structured vertex grids once
 * pgd_op_combine has put the atom into an operator; the first call looks for the atom's row classes (once: atoms do not
 * change).  The frontend asks before it trades a fused product-dot (fem._bilinear_scalar, the functionals of
 * solver.py:547-569) for product + dot with the product kept.  y is bit-identical in all three forms. */
int pgd_atom_product_form(pgd_handle ctx, pgd_handle A, int *form);
/* Which kernel family a product over the rows [r0, r1) (r1 < 0: all) of this operator would run in right now - its current storage, the
 * current knobs - and with which launch shape; nothing is launched, classified or counted.  pcg_like: the product of a PCG (w = x)
 * or a plain one, as opposed to a product fused with the dot against a third vector.  out[0..7) = family (index of pgd_kernel_counts,
 * -1: not decided by form - no symmetric storage, the CSR kernels or a lattice form), workgroups, planes per march, tiles in x,
 * tiles in y, rows per thread, plane fetches in flight (the last two: the stencil march only, else 0).  n >= 7. */
int pgd_product_plan(pgd_handle ctx, pgd_handle op, int64_t r0, int64_t r1, int pcg_like, int64_t *out, int n);

/* Look for the lossless row-class dictionary of the operator's diagonal form (structured vertex grids, after
 * pgd_op_symmetrize / pgd_op_combine; PGD_TUNE_SPMV_ROW_CLASSES): *classes = number of distinct 8-tuples of slot values
 * (1..255) when every row was verified bit by bit against its class - the z-march of later products then reads one code
 * byte per row (k_spmv_diac_march2) - or 0: none (more than 255 classes, not a grid, too few planes).  The library solves
 * call this themselves for the scaled operator; any later change of the operator's values drops the dictionary.   */
int pgd_op_classify(pgd_handle ctx, pgd_handle op, int *classes);
/* y = A x on [r0,r1), slot <- sum w_i y_i (local part; 0 for an empty range)    */
int pgd_spmv_dot_slot(pgd_handle ctx, pgd_handle A, pgd_handle x, pgd_handle y, pgd_handle w,
                      int64_t r0, int64_t r1, int slot);
/* r = b - q, z = dinv r, p = z on [r0,r1); slots s..s+2 <- (r.z, r.r, b.b)       */
int pgd_pcg_init_slot(pgd_handle ctx, pgd_handle b, pgd_handle q, pgd_handle dinv, pgd_handle r,
                      pgd_handle z, pgd_handle p, int64_t r0, int64_t r1, int slot);
/* tol2 slot <- max(rtol^2 S[bb], atol^2); done <- S[rr] <= tol2 (or breakdown: S[rr] is NaN); not gated by the done flag */
int pgd_pcg_tol_slot(pgd_handle ctx, double rtol, double atol, int slot_rr, int slot_bb,
                     int slot_tol2);
/* alpha = S[rz]/S[pq]; x += alpha p; r -= alpha q; z = dinv r;
 * slots out..out+1 <- (r.z, r.r)                                                */
int pgd_pcg_xr_slot(pgd_handle ctx, pgd_handle x, pgd_handle r, pgd_handle p, pgd_handle q,
                    pgd_handle dinv, pgd_handle z, int64_t r0, int64_t r1, int slot_rz,
                    int slot_pq, int slot_out);
/* iters += 1; S[6] <- S[rr]; done <- S[rr] <= S[tol2] (or breakdown)             */
int pgd_pcg_check_slot(pgd_handle ctx, int slot_rr, int slot_tol2);
/* beta = S[num]/S[den]; p = z + beta p                                           */
int pgd_pcg_p_slot(pgd_handle ctx, pgd_handle p, pgd_handle z, int64_t r0, int64_t r1,
                   int slot_num, int slot_den);

/* Single-reduction (Chronopoulos-Gear) form of the same recurrence: one all-reduce of
 * S[base..base+4] = (r.u, r.r, w.u interior / low / high boundary rows) per iteration.
 * S[base+5] alpha, S[base+6] beta, S[base+7] previous r.u, S[base+8] b.b.  base + 8 < PGD_NSLOTS.
 * pgd_cg_init_slot: r = b - q, u = dinv r, p = s = 0 on [r0,r1); S[base], S[base+1], S[base+8] <- (r.u, r.r, b.b); S[40..42]
 * are its scratch.                                                                       */
int pgd_cg_init_slot(pgd_handle ctx, pgd_handle b, pgd_handle q, pgd_handle dinv, pgd_handle r,
                     pgd_handle u, pgd_handle p, pgd_handle s, int64_t r0, int64_t r1, int base);
/* p = u + beta p; s = w + beta s; x += alpha p; r -= alpha s; u = dinv r; S[base..+1] <- (r.u, r.r) */
int pgd_cg_update_slot(pgd_handle ctx, pgd_handle x, pgd_handle r, pgd_handle u, pgd_handle w,
                       pgd_handle p, pgd_handle s, pgd_handle dinv, int64_t r0, int64_t r1, int base);
/* after the all-reduce: with g = S[base], d = S[base+2] + S[base+3] + S[base+4]: init: S[5] <- max(rtol^2 S[base+8], atol^2),
 * otherwise iters += 1; S[6] <- S[base+1]; done <- S[base+1] <= S[5], or breakdown (S[base+1] or d is NaN); then
 * beta = g / S[base+7] (init: 0), alpha = g / (d - beta g / S[base+5]) (init: g / d), S[base+5..7] <- (alpha, beta, g) */
int pgd_cg_scalars_slot(pgd_handle ctx, int base, int init, double rtol, double atol);

/* ----------------------------------------------- sharded solve, in-library --- */
/* The same single-reduction recurrence with the ITERATION LOOP AND THE COMMUNICATION inside the
 * library (no host language between two iterations): per iteration one halo exchange of the
 * boundary planes with the z-neighbours (rank-1, rank+1) and one all-reduce of 5 slots, issued on
 * the context's stream.  A context is bound to its communication once:
 *   - RCCL (one process per GPU, xGMI): rank 0 calls pgd_comm_unique_id, the 128 bytes travel to
 *     the other ranks by any means (torch.distributed broadcast), every rank calls
 *     pgd_comm_bind_rccl; the binding is checked on the spot (ring shift + all-reduce of rank ids).
 *     librccl is resolved at run time from the copy already loaded in the process.
 *   - callbacks: the library calls back for the two steps (several ranks sharing one GPU in tests:
 *     host-staged gloo).  A callback returns 0 on success.
 * Local numbering of a rank's vectors: [0, lo_ghost) ghost plane below, [own0, own1) owned rows,
 * [own1, own1 + hi_ghost) ghost plane above; own0 == lo_ghost.                                     */
typedef int (*pgd_halo_fn)(void *user, pgd_handle vec, int64_t own0, int64_t own1, int64_t lo_ghost,
                           int64_t hi_ghost);
typedef int (*pgd_allreduce_fn)(void *user, int first_slot, int count);
int pgd_comm_bind_callbacks(pgd_handle ctx, pgd_halo_fn halo, pgd_allreduce_fn allreduce, void *user,
                            int rank, int world);
int pgd_comm_unique_id(pgd_handle ctx, uint8_t *out128);
int pgd_comm_bind_rccl(pgd_handle ctx, const uint8_t *id128, int rank, int world);
/* Halo exchange concurrent with the product of the rows that read no ghost entry: a second
 * communicator (ncclCommSplit) on its own HIP stream, ordered against the compute stream by two events.
 * mode 1: try to enable - COLLECTIVE, call on every rank after all ranks bound successfully; the ranks must then
 * agree (e.g. MIN all-reduce of *state) and call mode 0 everywhere if any rank reports 0.  mode 0: disable.
 * mode -1: query.  *state: 1 = the sharded solve CAN overlap, 0 = the exchange stays on the compute stream.  A solve uses the
 * second stream only above PGD_TUNE_HALO_OVERLAP_MIN_ROWS rows per rank (default: never); mode -2: *state = did the last solve. */
int pgd_comm_overlap(pgd_handle ctx, int mode, int *state);
int pgd_comm_unbind(pgd_handle ctx);
/* Deadline of the host-side waits inside pgd_pcg_solve_sharded (the look at the flags after every chunk of iterations, the
 * closing agreement): the stream is polled with hipEventQuery, and after `seconds` without completion the call returns
 * PGD_ERR_TIMEOUT with "rank r/w: iteration i, last collective <name> #n" in pgd_last_error (also written to stderr) - a
 * neighbour that died, a collective nobody matches.  The stream is then stuck for good: the caller ends the PROCESS
 * (pgdrome_amd/dist.py exits non-zero).  Default 60 s, or PGD_COMM_TIMEOUT_S from the environment at bind time; <= 0: wait for ever. */
int pgd_comm_timeout(pgd_handle ctx, double seconds);
/* Phase timing of the sharded loop (bench.py's N > 1 line): mode 1 = on + reset, 0 = off, -1 = read only.  One iteration per
 * chunk of 16 is bracketed with HIP events on the compute stream.  out[0..7] = samples, then SECONDS summed over the samples:
 * [1] compute stream waiting for the ghost planes after the interior rows' product (exposed halo time), [2] interior product,
 * [3] boundary rows' product, [4] local sums, [5] the all-reduce (incl. waiting for the slowest rank), [6] vector update,
 * [7] host time spent waiting at the chunk boundaries (all chunks, not sampled).  out may be NULL.        */
int pgd_comm_prof(pgd_handle ctx, int mode, double *out8);
int pgd_comm_info(pgd_handle ctx, int *kind /* 0 none, 1 callbacks, 2 rccl */, int *rank, int *world);
int pgd_comm_halo(pgd_handle ctx, pgd_handle vec, int64_t own0, int64_t own1, int64_t lo_ghost,
                  int64_t hi_ghost);
int pgd_comm_allreduce_slots(pgd_handle ctx, int first_slot, int count);

/* DIRECT HALO of the sharded PCG loop (opt-in; no reference counterpart - /root/reference/pgdrome/solver.py:538-540 is serial).  The
 * boundary planes of the search direction are stored straight into the neighbours' ghost planes through mapped device pointers
 * (hipIpcMemHandle between processes; plain addresses inside one) with a sequence number posted behind them, and the product waits
 * for the numbers of its own ghost planes: no RCCL send / receive kernel in the iteration (14 of 54 us on the slab of an 8-GPU rank).
 * pgd_comm_push_export sizes the loop's work vectors for a vector of n rows partitioned [0, lo) ghost | [own0, own1) | ghost and
 * writes PGD_PUSH_BLOB_BYTES describing them; the caller carries every rank's blob to its neighbours (any transport) and hands the
 * lower / upper neighbour's blob (NULL where there is none) to pgd_comm_push_attach - collective over neighbours, ends with a
 * checked exchange; *state = 1 if the direct halo is usable on this rank.  pgd_pcg_solve_sharded uses it when EVERY rank has it
 * for exactly that partition (its setup vote) and the single-sync recurrence runs; otherwise the binding's exchange.  A number that
 * does not arrive within pgd_comm_timeout ends the solve with PGD_ERR_TIMEOUT.  pgd_comm_push: mode 1 / 0 switch it on / off,
 * -1 reads the state, -2 what the last solve did, 2 queues ONE exchange of the loop's search direction as it stands (probes: timing). */
#define PGD_PUSH_BLOB_BYTES 256
int pgd_comm_push_export(pgd_handle ctx, int64_t n, int64_t own0, int64_t own1, int64_t lo_ghost, int64_t hi_ghost,
                         uint8_t *blob /* PGD_PUSH_BLOB_BYTES */);
int pgd_comm_push_attach(pgd_handle ctx, const uint8_t *lower_blob, const uint8_t *upper_blob, int *state);
int pgd_comm_push(pgd_handle ctx, int mode, int *state);
/* DIRECT ALL-REDUCE of the loop's five sums (same opt-in, behind pgd_comm_push_export): all_blobs = every rank's export blob in rank
 * order (world x PGD_PUSH_BLOB_BYTES, world <= 16).  Every rank maps every rank's flag block; in the loop ONE kernel forms the
 * iteration's local sums, stores them into all mailboxes, posts, waits for everybody's and adds the contributions in rank order
 * (the same bits on every rank): neither k_pcg1_sums nor an RCCL kernel is left in the iteration.  Collective, ends with a checked
 * exchange; used by a solve only if every rank voted for it.  pgd_comm_allreduce_direct: mode as pgd_comm_push (2: one direct
 * all-reduce of slots 48 .. 52). */
int pgd_comm_allreduce_attach(pgd_handle ctx, const uint8_t *all_blobs, int *state);
int pgd_comm_allreduce_direct(pgd_handle ctx, int mode, int *state);
/* Jacobi-PCG on the rows [own0, own1) of this rank's slab of A (replaces the KSP solve of
 * solver.py:636,716 for the row-partitioned spatial dimension); b, x are local slab vectors, x holds
 * the start value and returns with current ghost planes.  iters / rel_res are global.            */
int pgd_pcg_solve_sharded(pgd_handle ctx, pgd_handle A, pgd_handle b, pgd_handle x, int64_t own0,
                          int64_t own1, int64_t lo_ghost, int64_t hi_ghost, double rtol, double atol,
                          int maxit, int *iters, double *rel_res);

/* BiCGStab with Jacobi scaling on the CSR product, for operators that are NOT symmetric (a convection atom
 * u.dx(a) * v * dx on a 2-D / 3-D space, or a 1-D system too long for pgd_band_solve): replaces the MUMPS solve of
 * LinearVariationalSolver for such systems (solver.py:627-636, 704-716).  x holds the start value; stop test
 * ||b - A x|| <= max(rtol ||b||, atol), confirmed on the true residual; *rel_res is ||b - A x|| / ||b|| recomputed from
 * the x returned (after a third second leg of 50 iterations: the recurrence's, started from the true one), also where maxit ran
 * out (PGD_OK with *iters == maxit).  x after maxit = k is the k-th iterate.  PGD_ERR_SINGULAR on the fifth breakdown of
 * a call (rhat . v, t . t, omega or rho exactly zero or not a number, each answered by a restart from the current x): x
 * then holds the iterate the last restart started from (with the half step x += alpha y of a t . t breakdown) - the start
 * value if no iteration completed, e.g. with a zero on the diagonal - and *iters and *rel_res are NOT reported (they read
 * 0).  PGD_ERR_INVALID (b and x the same vector, a length that is not the operator's, maxit < 0) is returned before
 * anything is launched.  */
int pgd_bicgstab_solve(pgd_handle ctx, pgd_handle A, pgd_handle b, pgd_handle x, double rtol, double atol,
                       int maxit, int *iters, double *rel_res);

/* Gram data of the Galerkin start of a PCG solve (the warm start x0 = sum_j c_j v_j with G c = g; this library's
 * addition in front of the solve that replaces solver.py:636,716): out[i*k + j] = v_i . (A v_j) over rows
 * [r0, r1), out[k*k + j] = v_j . b, k <= 17.  k products from the operator's fastest storage form, every dot on
 * the device, ONE host synchronisation; a sharded caller all-reduces `out` once.                        */
int pgd_start_gram(pgd_handle ctx, pgd_handle A, const pgd_handle *vecs, int k, pgd_handle b, int64_t r0,
                   int64_t r1, double *out);
/* r = b - sum_j coefs[j] (A v_j), j < k, from the products A v_j the library still holds from the pgd_start_gram call
 * that came right before (same operator, all rows, k <= 9): the residual of the Galerkin start x0 = sum_j coefs[j] v_j
 * without another product - input of the second level of the start over the spectral vectors
 * (pgdrome_amd/spectral.py; the solve it prepares replaces solver.py:636,716).  PGD_ERR_INVALID if the products are
 * not held.                                                                                               */
int pgd_start_residual(pgd_handle ctx, pgd_handle A, int k, const double *coefs, pgd_handle b, pgd_handle r);

/* out[j] = x . y_j over entries [lo, hi) for k <= 256 vectors: ceil(k / 17) passes over x and ONE host
 * synchronisation.  Serves the functionals of one iterate against all stored modes of its dimension
 * (the scalar assemble() calls inside solver.py:568-612 when the products A y_j are already stored). */
int pgd_vec_multidot(pgd_handle ctx, pgd_handle x, const pgd_handle *ys, int k, int64_t lo, int64_t hi,
                     double *out);

/* Two left factors against the same k <= 128 vectors: out[j] = x0 . y_j, out[k + j] = x1 . y_j over [lo, hi); every y_j is
 * read once for both (ceil(k / 16) passes over x0 and x1), ONE host synchronisation.  The functionals of an iterate F against
 * the stored modes m_j of its dimension under two symmetric atoms (solver.py:568-612: F^T K m_j and F^T M m_j inside the
 * callbacks) as (K F) . m_j and (M F) . m_j: k + 2 vector reads where F . (K m_j), F . (M m_j) take 2 k + 1.            */
int pgd_vec_multidot_pair(pgd_handle ctx, pgd_handle x0, pgd_handle x1, const pgd_handle *ys, int k, int64_t lo,
                          int64_t hi, double *out);

/* Gram block of two families of vectors: out[i * ky + j] = sum_{lo <= r < hi} x_i[r] y_j[r] (hi < 0: the whole vector), every
 * vector read ONCE (v_mfma_f64_16x16x4_f64 on row blocks staged in LDS; PGD_TUNE_GRAM_VARIANT = 0: plain fma chains) and ONE
 * host synchronisation.  ys == NULL (then ky must equal kx) is the symmetric case X^T X: only the tiles on and above the
 * diagonal are computed and mirrored, out is symmetric bit for bit.  1 <= kx, ky <= 128 per call (the binding blocks larger
 * families).  No atomics: the rows are cut into at most 1024 segments that depend on (lo, hi) alone, their partials are added
 * in ascending order - every output is bit-identical for any grid (PGD_TUNE_GRAM_GRID_MAX).  It replaces the kx calls of
 * pgd_vec_multidot behind a Gram matrix ((ceil(k / 17) + k) k vector reads where k are needed), spectral.py's _gram over
 * separate vectors, and it is the l2 statistic of a batch of fields that pgd_eval_batch leaves outside: |u_s|^2 = c_s^T G c_s
 * with the modes' Gram G.  PGD_ERR_INVALID with a message, before anything is launched: null xs or out, kx or ky out of range,
 * ky != kx without ys, an invalid handle, vectors of different lengths, a range outside the vectors.  An empty range gives
 * zeros and PGD_OK.                                                                                                        */
int pgd_vec_gram(pgd_handle ctx, const pgd_handle *xs, int kx, const pgd_handle *ys_or_null, int ky, int64_t lo, int64_t hi,
                 double *out);

/* Quadratic forms of the modes at every entry: outs[q][i] = f_i^T Q_q f_i for nq matrices (q: nq row-major k x k doubles on the
 * host, any matrix, symmetric or not), f_i = (modes[0][i] .. modes[k-1][i]); every mode read once per call.  outs[q] == 0: that
 * field is not stored (outs may be NULL: none is).  flags & PGD_QUAD_CLAMP: values below 0 are stored (and reduced) as 0.
 * extrema (may be NULL): min over the rows of form q in extrema[2 q], max in extrema[2 q + 1], of the values as stored.
 * 1 <= k <= 256, 1 <= nq <= 64 (the binding blocks more forms).  The partial variances of a separated solution with independent
 * parameters are such forms (model.py: variance_decomposition).  v_mfma_f64_16x16x4_f64 with the dofs on the fragment's column
 * index as in pgd_eval_batch: a wave owns its rows, F Q is consumed in registers, each value is one fixed chain and the extrema
 * do not depend on order - every output is bit-identical for any grid (PGD_TUNE_QUAD_GRID_MAX), and a form's field is the same
 * bits alone or among others.  PGD_TUNE_QUAD_VARIANT = 0: plain fma chains.  ONE host synchronisation.  PGD_ERR_INVALID with a
 * message, before anything is launched and with the outputs untouched: null modes or q, k or nq out of range, unknown flags, an
 * invalid handle, vectors of different lengths, an output that is also a mode or another output, neither a field nor extrema.
 * Vectors of length 0: PGD_OK, extrema (+inf, -inf).  NaNs give unspecified extrema.                                          */
enum { PGD_QUAD_CLAMP = 1 };
int pgd_quad_forms(pgd_handle ctx, const pgd_handle *modes, int k, const double *q, int nq, int flags, const pgd_handle *outs,
                   double *extrema);
/* out[i] = den[i] > floor ? num[i] / den[i] : 0 (out may be num or den).  The ratio fields of the forms above: a Sobol index
 * where the variance is above a floor.  PGD_ERR_INVALID: invalid handles, different lengths, a NaN floor.  No synchronisation. */
int pgd_vec_ratio(pgd_handle ctx, pgd_handle out, pgd_handle num, pgd_handle den, double floor);

/* Misfits of sensor data on a tensor grid of the free coordinates: chi2[s] = sum_p (y_p - sum_t a[p * k + t] c_t(s))^2 for every
 * sample s = (i_0 .. i_{ndim-1}), last index fastest, S = prod n[d] of them, with c_t(s) = 1 * T_0[t, i_0] * T_1[t, i_1] * .. formed
 * in ascending d where it is used (the bits of model.py's mode_factors_many on the same tables): the K x S coefficient matrix is
 * never stored.  a: m x k row-major on the host (the whitened sensor modes), y: m values (the whitened data), tables: the ndim
 * tables one after the other, table d being k x n[d] row-major, n: ndim point counts; chi2: a vector of S entries.  min_out /
 * argmin_out (either may be NULL): the smallest chi2 and the lowest sample that holds it (-1 if no value compares: all NaN).
 * 1 <= k <= 256, 1 <= m <= 256, 1 <= ndim <= 6, S < 2^31.  v_mfma_f64_16x16x4_f64 with 16 samples on the fragment's column index as
 * in pgd_eval_batch and pgd_quad_forms, a laid out in fragment order by the library: a wave owns its samples, each chi2 value is
 * one fixed chain and the minimum does not depend on order - every output is bit-identical for any grid
 * (PGD_TUNE_MISFIT_GRID_MAX).  PGD_TUNE_MISFIT_VARIANT = 0: plain fma chains.  ONE host synchronisation.  PGD_ERR_INVALID with a
 * message, before anything is launched and with the outputs untouched: a null a, y, tables or n, k, m or ndim out of range, a
 * dimension without points, S >= 2^31, chi2 not a vector or not of S entries.  Scattered samples are one dimension whose table
 * is the k x S coefficient matrix itself.                                                                                     */
int pgd_grid_misfit(pgd_handle ctx, const double *a, const double *y, int m, int k, const double *tables, const int *n, int ndim,
                    pgd_handle chi2, double *min_out, int64_t *argmin_out);
/* Reductions of the posterior over those misfits: with e_s = w_s exp(-(chi2[s] - shift) / 2), w_s = 1 * weights_0[i_0] * weights_1[i_1] * ..
 * (weights, abscissae: the ndim arrays of n[d] entries one after the other; tables, n, ndim, k as in pgd_grid_misfit),
 *   sums[0] = Z = sum e_s, sums[1] = sum e_s^2                                                         (always)
 *   PGD_POST_MARGINALS: marginals[off_d + i] = the sum of e_s over the samples with i_d = i, off_d = n[0] + .. + n[d-1]
 *   PGD_POST_THETA:     theta1[d] = sum e_s th_d, theta2[d * ndim + f] = sum e_s th_d th_f, th_d = abscissae_d[i_d]
 *   PGD_POST_COEF:      coef1[t] = sum e_s c_t(s), coef2[t * k + u] = sum e_s c_t(s) c_u(s) - a product over the samples on the
 *                       matrix unit, 1 <= k <= 64 (PGD_ERR_INVALID above); symmetric bit for bit (the upper triangle, mirrored).
 * Outputs that are not asked for, and tables / abscissae they alone need, may be NULL (k is ignored without PGD_POST_COEF).  No
 * floating-point atomics: the samples are cut into at most 1024 segments that depend on S alone, a segment's partial sums are
 * formed in an order that depends on the segment alone and the segments are added in ascending order; an entry of the
 * marginals is summed by one workgroup in a fixed order - every output is bit-identical from run to run and for any grid
 * (PGD_TUNE_POST_GRID_MAX).  PGD_TUNE_POST_VARIANT = 0: the coefficient moments from plain fma chains.  ONE host synchronisation.
 * PGD_ERR_INVALID with a message, before anything is launched and with the outputs untouched: unknown bits in want, a shift that
 * is not finite, ndim out of range, a null n, weights or sums, a requested output (or what it needs) that is missing, k out of
 * range with PGD_POST_COEF, a dimension without points, S >= 2^31, chi2 not a vector or not of S entries.  A shift equal to the
 * smallest chi2 keeps Z >= the weight of that sample however far off the others are (their e underflows to 0).             */
enum { PGD_POST_MARGINALS = 1, PGD_POST_THETA = 2, PGD_POST_COEF = 4 };
int pgd_grid_posterior(pgd_handle ctx, pgd_handle chi2, double shift, const double *tables, const int *n, int ndim, int k,
                       const double *weights, const double *abscissae, int want, double *sums, double *marginals, double *theta1,
                       double *theta2, double *coef1, double *coef2);
/* Posteriors of nd data sets on the same grid in one pass (samples, tables, weights, abscissae and sample order as above; c_t(s) by
 * the same chain).  Data set j is a row u_j (u: nd x m row-major on the host) and the scalars alpha[j], beta[j]:
 *   p_s = a c(s) (m entries),  chi2[j, s] = beta_j - 2 u_j . p_s + alpha_j |p_s|^2
 *   chi2_min[j] = shift_j = min_s chi2[j, s],  argmin[j] = the lowest sample that holds it (-1: no value compares)
 *   e_js = w_s exp(-(chi2[j, s] - shift_j) / 2),  sums[2 j] = sum_s e_js,  sums[2 j + 1] = sum_s e_js^2
 *   PGD_POST_THETA: theta1[j * ndim + d] = sum e_js th_d, theta2[(j * ndim + d) * ndim + f] = sum e_js th_d th_f (symmetric bit for
 *                   bit: the upper triangle, mirrored); without the bit abscissae, theta1 and theta2 may be NULL.
 * Independent data sets y_j are the rows (y_j, 1, |y_j|^2); "all data up to step j" is (sum_{i<=j} y_i, j + 1, sum_{i<=j} |y_i|^2).
 * The nd x S misfits are never stored: three chained products on v_mfma_f64_16x16x4_f64 (a c, then u against it, then e against
 * the features 1, th_d, th_d th_f) in two passes, the minima first.  No floating-point atomics; the segments of the samples depend
 * on S alone: every output of a data set is bit-identical from run to run, for any grid (PGD_TUNE_POSTMANY_GRID_MAX), with or
 * without the skip of underflowed tiles (PGD_TUNE_POSTMANY_SKIP), alone or among others, in any position.  The data sets are
 * taken in chunks whose device scratch stays below 256 MB: ONE host synchronisation per chunk.  PGD_TUNE_POSTMANY_VARIANT = 0:
 * plain fma chains (the cross-check; it agrees within rounding, not bit for bit).  1 <= k <= 64, 1 <= m <= 64 (compress the
 * solution first otherwise), 1 <= ndim <= 6, S < 2^31, 1 <= nd < 2^31.  PGD_ERR_INVALID with a message, before anything is
 * launched and with the outputs untouched: a bit of want other than PGD_POST_THETA, k, m, ndim or nd out of range, a null input
 * or output that is needed, a dimension without points, S >= 2^31, a weight or (with PGD_POST_THETA) an abscissa that is not
 * finite.  pgd_postmany_data_block: the data sets a wave of the matrix-unit kernel holds for ndim dimensions.                 */
int pgd_grid_posterior_many(pgd_handle ctx, const double *a, int m, int k, const double *u, const double *alpha, const double *beta,
                            int64_t nd, const double *tables, const int *n, int ndim, const double *weights, const double *abscissae,
                            int want, double *chi2_min, int64_t *argmin, double *sums, double *theta1, double *theta2);
int pgd_postmany_data_block(int ndim);
/* Sensor placement by greedy expected information gain (Bayesian D-optimality in the linearised form) on the same grid (samples,
 * tables, weights and sample order as above).  dtables: the derivatives of the tables, laid out like them; the derivative
 * coefficient of mode t against coordinate d is the chain cd_t(s) = 1 * U_0[t, i_0] * U_1[t, i_1] * .. in ascending f with
 * U_f = dtables_f for f == d and tables_f otherwise, and the Jacobian of a row p (k entries) is g_p,d(s) = sum_t p[t] cd_t(s), an fma
 * chain in ascending t.  state: a vector of 2 nh S doubles, nh = ndim (ndim + 1) / 2, plane-major: state[c S + s] is entry c of
 * H_s, the UPPER triangle in row order (c = 0: (0, 0), 1: (0, 1) .. ndim: (1, 1) ..), state[(nh + c) S + s] entry c of W_s, the
 * inverse of the lower Cholesky factor of H_s, the LOWER triangle in row order (c = i (i + 1) / 2 + j, j <= i).
 *   pgd_design_update: with h0 (ndim x ndim row-major, symmetric positive definite; may be NULL) every H_s is first set to it;
 *     then H_s += sum_r g_r(s) g_r(s)^T for the 0 <= R <= 256 rows (added, never downdated); W_s is recomputed;
 *     sums[0] = sum_s w_s log det H_s, formed as -2 sum log diag W_s; sums[1 .. nh] = sum_s w_s (W_s^T W_s), the expected posterior
 *     covariance, packed like H.  R = 0 with h0 is the reset.  A thread per sample; ONE host synchronisation.
 *   pgd_design_gains: gains[j] = 1/2 sum_s w_s log det(I_R + V^T V), V = W_s [g_jR(s) .. g_jR+R-1(s)], for the M candidates whose
 *     rows are a[(j R + r) k + t] (a: M R x k row-major on the host), from the LDL^T pivots of I + V^T V as log1p(pivot - 1).  The
 *     M x S x R x ndim Jacobian is never stored: v_mfma_f64_16x16x4_f64 with 16 samples on the fragment's column index as in
 *     pgd_grid_misfit and 16 candidates on its row index, a laid out in fragment order per plane r by the library; the epilogue is
 *     lane-local.  1 <= k <= 64 (compress first otherwise), 1 <= R <= 3, 1 <= ndim <= 6, S < 2^31, 1 <= M < 2^31.  The candidates
 *     are taken in chunks whose device scratch stays below 256 MB: ONE host synchronisation per chunk.
 * No floating-point atomics; the samples are cut by the segments of pgd_grid_posterior (a function of S alone), a partial sum of a
 * segment is formed in an order that depends on the segment alone and the segments are added in ascending order: every gain and
 * every entry of sums is bit-identical from run to run, for any grid (PGD_TUNE_DESIGN_GRID_MAX), and a candidate's gain alone or
 * among others at any position.  PGD_TUNE_DESIGN_VARIANT = 0: the gains from plain fma chains (the cross-check; it agrees within
 * rounding, not bit for bit).  PGD_ERR_INVALID with a message, before anything is launched and with the outputs untouched: a null
 * input or output, k, R, ndim or M out of range, a dimension without points, S >= 2^31, a state that is not a vector of 2 nh S
 * entries, a weight that is not finite, an h0 that is not symmetric positive definite.                                          */
int pgd_design_update(pgd_handle ctx, const double *h0_or_null, const double *rows, int R, int k, const double *tables,
                      const double *dtables, const int *n, int ndim, const double *weights, pgd_handle state, double *sums);
int pgd_design_gains(pgd_handle ctx, const double *a, int64_t M, int R, int k, const double *tables, const double *dtables,
                     const int *n, int ndim, const double *weights, pgd_handle state, double *gains);

/* ------------------------------------------------------------ column blocks --- */
/* k <= 64 columns of n rows in ONE library-owned allocation, stored as fp32 or f64: the start space of the spatial solves
 * (pgdrome_amd/spectral.py; this library's addition in front of the solve that replaces solver.py:636,716), whose cost per
 * solve is the bytes of its two passes.  Every column is padded like every device array.  Products and sums are f64
 * whatever the storage.
 *   pgd_block_set_column: column j = vec, rounded to nearest for fp32;  pgd_block_get_column: vec = column j, exactly.
 *   pgd_block_dots: out[j] = sum_{lo <= i < hi} Y_ij r_i for all k columns (hi < 0: n) - one kernel, one pass over the block
 *     and r, per-workgroup partial sums and the fixed-order final pass of every reduction (the same bits in every call), one
 *     D2H copy and ONE host synchronisation.
 *   pgd_block_combine: x_i = base_i + sum_j coefs[j] Y_ij in one kernel, as the chain s = base_i (0 with base = 0);
 *     s = fma(coefs[j], Y_ij, s) for j ascending; base may be x.  With f64 storage this is, bit for bit, pgd_vec_lincomb of
 *     [base, Y_0, ...] with [1, coefs...].
 * pgd_block_storage: the storage PGD_TUNE_BLOCK_STORAGE selects for the start space, -1: none (the caller keeps vectors).   */
enum { PGD_BLOCK_F32 = 0, PGD_BLOCK_F64 = 1 };
int pgd_block_create(pgd_handle ctx, int64_t n, int k, int dtype, pgd_handle *block);
int pgd_block_free(pgd_handle ctx, pgd_handle block);
int pgd_block_info(pgd_handle ctx, pgd_handle block, int64_t *n, int *k, int *dtype, int64_t *bytes);
int pgd_block_storage(pgd_handle ctx, int *dtype);
int pgd_block_set_column(pgd_handle ctx, pgd_handle block, int j, pgd_handle vec);
int pgd_block_get_column(pgd_handle ctx, pgd_handle block, int j, pgd_handle vec);
int pgd_block_dots(pgd_handle ctx, pgd_handle block, pgd_handle vec_r, int64_t lo, int64_t hi, double *out);
int pgd_block_combine(pgd_handle ctx, pgd_handle block, const double *coefs, pgd_handle vec_base_or_0, pgd_handle vec_x);

/* ------------------------------------------------- batched online evaluation --- */
/* U[n x s] = F[n x k] C[k x s]: s samples of the online reconstruction u_j = sum_t C[t][j] F_t in ONE pass over the k mode
 * vectors (pgd_vec_lincomb reads them again for every sample), with the reductions formed in the kernel that holds the
 * accumulators - n s doubles are never stored unless the fields themselves are asked for.  The product runs on the f64
 * matrix unit (v_mfma_f64_16x16x4_f64; PGD_TUNE_EVAL_VARIANT = 0: plain fma chains over k in ascending order).
 *   modes: k vectors of the same size n, 1 <= k <= 256;  coefs: host, k x s row-major, coefs[t*s + j] = C[t][j], 1 <= s <= 2^24;
 *   want: bit mask of PGD_EVAL_*;  threshold: of the exceedance count (must be 0 without PGD_EVAL_EXCEED);
 *   sample_stats: host, 3 x s: min, max and max |.| of every sample over the n entries;
 *   env_min / env_max: vectors of size n, min / max over the s samples per entry;
 *   exceed: vector of size n, the number of samples with u > threshold, as a double;
 *   fields: vector of size n*s, sample-major: sample j at [j*n, (j+1)*n).
 * PGD_ERR_INVALID with a message, before anything is launched, for: a requested output that is missing, an output (or a
 * threshold) that is passed but not requested, wrong sizes, a mode aliasing an output, two outputs aliasing each other, k or s
 * out of range, an s*n that overflows.  n == 0 is PGD_OK with sample_stats untouched.  Large s runs in chunks of samples
 * (PGD_TUNE_EVAL_SAMPLE_CHUNK); every output is bit-identical for any chunk length and any grid size (no atomics: persistent
 * workgroups, one row of partial extrema each, a fixed-order final pass).  The call synchronises with the host once, at its
 * end, if and only if PGD_EVAL_STATS is set.  NaNs in the modes or coefficients give unspecified statistics.             */
enum { PGD_EVAL_STATS = 1, PGD_EVAL_ENVELOPE = 2, PGD_EVAL_EXCEED = 4, PGD_EVAL_FIELDS = 8 };
int pgd_eval_batch(pgd_handle ctx, const pgd_handle *modes, int k, const double *coefs, int64_t s, int want,
                   double threshold, double *sample_stats, pgd_handle env_min, pgd_handle env_max, pgd_handle exceed,
                   pgd_handle fields);

/* ----------------------------------- batched evaluation of gradient quantities --- */
/* Quantities of the spatial gradient of a P1 field - a flux magnitude, a von Mises stress - are Euclidean norms of a few
 * components that are LINEAR in the field, and the P1 gradient is constant per cell.  Two stages: pgd_cell_gradient turns a
 * nodal mode into q cell-wise planes, once per mode; pgd_eval_batch_norm is pgd_eval_batch on the q planes of a cell,
 * combined with a square root before the reductions.
 *
 * pgd_cell_gradient: out[i*nc + cell] = scale[cell] * sum_j L[i][j] g[j], g[c*gdim + a] = d u_c / d x_a on the cell.
 *   mesh: a P1 layout on intervals, triangles or tetrahedra, scalar or blocked (pgd_mesh_blocked: ncomp components);
 *   u: nv*ncomp entries, node*ncomp + c;  L: host, q x (ncomp*gdim) row-major, 1 <= q <= 9;
 *   scale: a vector of nc entries in cell order, or 0 for a scale of 1;  out: q*nc entries, plane-major.
 * A thread per cell; the inverse Jacobian is formed from the cell's own vertices (cofactors and determinant), whatever the mesh.
 * PGD_ERR_INVALID with a message, before anything is launched, for: a P2 layout, q out of range, a null L, wrong vector sizes,
 * out aliasing u or scale.  nc == 0 is PGD_OK.  No atomics, no host synchronisation.                                      */
int pgd_cell_gradient(pgd_handle ctx, pgd_handle mesh, pgd_handle u, const double *L, int q, pgd_handle scale_or_0,
                      pgd_handle out);

/* pgd_eval_batch_norm: every mode has q*m entries (q planes of m, as pgd_cell_gradient writes them); the value of entry e and
 * sample j is v = sqrt(sum_i u_i^2) with u_i = sum_t C[t][j] modes[t][i*m + e]; the sum of squares starts from 0 and takes
 * fma(u_i, u_i, .) over ascending i.  1 <= q <= 9; q = 1 gives |u|.  Every output has m entries (fields: m*s, sample-major),
 * max |.| equals max.  Everything pgd_eval_batch states holds here: the argument checks (and: q out of range, mode sizes that
 * are no multiple of q), the sample chunks, the pinned coefficient staging, one host synchronisation if and only if
 * PGD_EVAL_STATS is set, no atomics, every output bit-identical for any grid size and chunk length, both variants of
 * PGD_TUNE_EVAL_VARIANT.  The matrix-unit kernel keeps the q planes of a block of 64, 32 or 16 entries in LDS (up to 160 KiB
 * for 16) and reads them from global memory where even that does not fit (q * k above about 1100): slower, same bits.
 * Signed components and eigenvalues of the planes: pgd_eval_batch_quantity, further down.                                */
int pgd_eval_batch_norm(pgd_handle ctx, const pgd_handle *modes, int k, int q, const double *coefs, int64_t s, int want,
                        double threshold, double *sample_stats, pgd_handle env_min, pgd_handle env_max, pgd_handle exceed,
                        pgd_handle fields);
/* pgd_eval_batch_grad: pgd_cell_gradient and pgd_eval_batch_norm in one call, with the planes never stored.  Per cell e and sample
 * j the value is sqrt(sum_i u_i^2), u_i = sum_t C[t][j] P_t[i][e], P_t[i][e] exactly what pgd_cell_gradient(mesh, modes[t], L, q,
 * scale) would have written; the kernels form P_t from the nodal values where the stored path reads it (the matrix-unit kernel when
 * it stages a block of cells in LDS, the plain kernel in front of its fma chains), so the call needs no memory beyond the nodal modes.
 *   mesh, L, q, scale_or_0: as pgd_cell_gradient;  modes: k nodal vectors of nv*ncomp entries;
 *   coefs .. fields: as pgd_eval_batch_norm, every output with one entry per cell (fields: nc*s, sample-major).
 * Everything pgd_eval_batch_norm states holds: the want bits, the sample chunks, no atomics, one host synchronisation if and only if
 * PGD_EVAL_STATS is set, max |.| equals max, outputs bit-identical for any grid size and chunk length, both variants.  PGD_ERR_INVALID
 * with a message, before anything is launched, for everything pgd_eval_batch and pgd_cell_gradient refuse (a P2 layout, a layout
 * without cell records, q out of range, a null L, modes of another length than nv*ncomp, a scale of another length than nc) and for
 * an output aliasing a mode or the scale.  nc == 0 is PGD_OK.
 * Limits: P1 layouts; the matrix-unit kernel has no fallback to global memory, so where the q planes of 16 cells do not
 * fit 160 KiB of LDS (q * 4 ceil(k / 4) above about 1250) the call is refused with PGD_ERR_LIMIT before anything is launched
 * (PGD_TUNE_EVAL_VARIANT = 0 has no such limit); every sample chunk gathers the nodal values and forms the planes again, so calls
 * of few samples are dominated by the gathers - where the planes fit in memory and are reused, the two-stage path reads less. */
int pgd_eval_batch_grad(pgd_handle ctx, pgd_handle mesh, const pgd_handle *modes, int k, const double *L, int q,
                        pgd_handle scale_or_0, const double *coefs, int64_t s, int want, double threshold, double *sample_stats,
                        pgd_handle env_min, pgd_handle env_max, pgd_handle exceed, pgd_handle fields);
/* How the last pgd_eval_batch_norm, pgd_eval_batch_grad or pgd_eval_batch_grad_p2 call that launched laid out its work: rows = entries per workgroup (64, 32 or 16 on the matrix
 * unit, 64 in the plain variant), staged = 1 the planes of a row block in at most 64 KiB of LDS, 2 in more (up to 160 KiB), 0 read
 * from global memory (always in the plain variant; never on the matrix unit for pgd_eval_batch_grad); rows = 0, staged = -1
 * before the first call.                                                                                                      */
int pgd_eval_norm_last_shape(pgd_handle ctx, int *rows, int *staged);

/* The same two for a P2 field.  Its gradient is affine on a cell, so the caller names npt points of the cell by their barycentric
 * coordinates lam (host, npt x (gdim+1) row-major, 1 <= npt <= 4; rows that sum to 1) and gets the quantity at every one of them.
 * Entries are point-major: entry a*nc + e is point a of cell e, so one point's slice is a cell-wise vector.
 *
 * pgd_cell_gradient_p2: out[(i*npt + a)*nc + e] = scale[e] * sum_j L[i][j] g[j], g[c*gdim + d] = d u_c / d x_d at point a of cell e:
 * q planes of m = npt*nc entries, what pgd_eval_batch_norm takes.
 *   mesh: a P2 layout on triangles or tetrahedra (records of 6 / 10 nodes: the vertices, then the edge nodes of the local edges
 *   (1,2) (0,2) (0,1) resp. (2,3) (1,3) (1,2) (0,3) (0,2) (0,1)), scalar or blocked;  u: nv*ncomp entries, node*ncomp + c;
 *   L, q, scale: as pgd_cell_gradient (scale: one entry per CELL);  out: q*npt*nc entries.
 * With dl_i = u_i (4 lam_i - 1) + sum over the edges (i,b) of 4 u_ib lam_b the reference derivatives are dl_{a+1} - dl_0 (the node
 * of the edge (0,a+1), which both sums hold with cancelling coefficients, enters once with 4 lam_0 - 4 lam_{a+1}); the
 * inverse Jacobian comes from the cell's vertices alone, as in pgd_cell_gradient, and so do L g and the scale.  A thread per cell.
 * PGD_ERR_INVALID with a message, before anything is launched, for: any other layout (P1, the 1-D P2 layout), npt or q out of
 * range, a null lam or L, wrong vector sizes, out aliasing u or scale.  nc == 0 is PGD_OK.  No atomics, no host synchronisation. */
int pgd_cell_gradient_p2(pgd_handle ctx, pgd_handle mesh, pgd_handle u, const double *lam, int npt, const double *L, int q,
                         pgd_handle scale_or_0, pgd_handle out);
/* pgd_eval_batch_grad_p2: pgd_cell_gradient_p2 and pgd_eval_batch_norm in one call, the planes never stored - pgd_eval_batch_grad
 * with an entry (point row / nc of cell row % nc) where that has a cell.  Every output has npt*nc entries (fields: npt*nc*s,
 * sample-major); P_t is exactly what pgd_cell_gradient_p2 would have written.  Everything pgd_eval_batch_grad states holds, the
 * PGD_ERR_LIMIT rule included; refusals as pgd_cell_gradient_p2 and pgd_eval_batch.  Every entry of a cell forms the inverse and
 * gathers the record's nodal values again.                                                                                  */
int pgd_eval_batch_grad_p2(pgd_handle ctx, pgd_handle mesh, const pgd_handle *modes, int k, const double *lam, int npt,
                           const double *L, int q, pgd_handle scale_or_0, const double *coefs, int64_t s, int want, double threshold,
                           double *sample_stats, pgd_handle env_min, pgd_handle env_max, pgd_handle exceed, pgd_handle fields);

/* --------------------------------------- other values of the combined planes --- */
/* What becomes of the q combined planes u_0 .. u_{q-1} of an entry and sample before the reductions.  The norm is one choice;
 * failure criteria that tell tension from compression (the largest principal stress of a brittle material, Tresca) are
 * eigenvalue functions of the stress tensor, which a sum of squares taken plane by plane cannot form.
 *   PGD_EVAL_Q_NORM        sqrt(sum_i u_i^2): what the three calls above compute, bit for bit.
 *   PGD_EVAL_Q_VALUE       q = 1: u_0 with its sign - the accumulator of pgd_eval_batch on that plane, bit for bit.
 *   PGD_EVAL_Q_EIG_MAX     the largest eigenvalue of the symmetric tensor whose planes are xx, yy, zz, xy, yz, xz (q = 6) or
 *   PGD_EVAL_Q_EIG_MIN     xx, yy, zz, xy with yz = xz = 0 (q = 4: plane strain);  the smallest;
 *   PGD_EVAL_Q_EIG_SPREAD  largest minus smallest (twice the largest shear stress: Tresca), never negative.
 * The eigenvalues come from a deflating form: with m = tr / 3, p^2 = |sigma - m I|_F^2 / 6, C = (sigma - m I) / p only the root
 * of the characteristic polynomial that is separated from the other two is taken from the angle acos(det C / 2) / 3, its
 * eigenvector from the largest cross product of two rows of C - lambda I, the other two eigenvalues from the 2 x 2 problem on
 * the plane orthogonal to it, the isolated one again as a Rayleigh quotient.  Every eigenvalue is off by a few units of
 * 2^-53 |sigma|_F beyond what the errors of the u_i move it by (Weyl: at most their Frobenius norm), also where two eigenvalues
 * coincide - where the three roots taken from the angle alone lose half the digits.  p = 0 gives m.  Tensors whose squares
 * over- or underflow are not served.
 * With signed values max |.| (row 2 of sample_stats) is max(|min|, |max|) and no copy of max. */
enum pgd_eval_quantity {
    PGD_EVAL_Q_NORM = 0, PGD_EVAL_Q_VALUE = 1, PGD_EVAL_Q_EIG_MAX = 2, PGD_EVAL_Q_EIG_MIN = 3, PGD_EVAL_Q_EIG_SPREAD = 4
};
/* pgd_eval_batch_norm, pgd_eval_batch_grad and pgd_eval_batch_grad_p2 with the kind (a pgd_eval_quantity) after q; those three are
 * kind 0 of these.  Everything they state holds - arguments, outputs, want bits, chunks, no atomics, bit-identical outputs for
 * any grid size and chunk length, both variants of PGD_TUNE_EVAL_VARIANT, the PGD_ERR_LIMIT rule of the fused calls,
 * pgd_eval_norm_last_shape - with the value of the kind in the place of the norm.  The eigenvalue kinds keep the q accumulator
 * tiles of a sample tile in registers, so their matrix-unit kernels take 16 entries per workgroup, never 32 or 64.
 * PGD_ERR_INVALID with a message, before anything is launched, also for: a kind out of range, PGD_EVAL_Q_VALUE with q != 1, an
 * eigenvalue kind with q other than 4 or 6. */
int pgd_eval_batch_quantity(pgd_handle ctx, const pgd_handle *modes, int k, int q, int kind, const double *coefs, int64_t s, int want,
                            double threshold, double *sample_stats, pgd_handle env_min, pgd_handle env_max, pgd_handle exceed,
                            pgd_handle fields);
int pgd_eval_batch_grad_quantity(pgd_handle ctx, pgd_handle mesh, const pgd_handle *modes, int k, const double *L, int q, int kind,
                                 pgd_handle scale_or_0, const double *coefs, int64_t s, int want, double threshold,
                                 double *sample_stats, pgd_handle env_min, pgd_handle env_max, pgd_handle exceed, pgd_handle fields);
int pgd_eval_batch_grad_p2_quantity(pgd_handle ctx, pgd_handle mesh, const pgd_handle *modes, int k, const double *lam, int npt,
                                    const double *L, int q, int kind, pgd_handle scale_or_0, const double *coefs, int64_t s, int want,
                                    double threshold, double *sample_stats, pgd_handle env_min, pgd_handle env_max,
                                    pgd_handle exceed, pgd_handle fields);

/* ------------------------------------------------------- point sets (sensors) --- */
/* The field at a few points of the large dimension - what a calibration compares with measurements (reference
 * pgdrome/model.py: evaluate_sensor_response, evaluate_derivative_sensor_response, which load fenicstools.Probes for it).  A
 * point set holds, on the device, the cell of every point and its barycentric coordinates there; sampling a nodal field at the
 * set gathers through the cell records, so a mode never leaves the device.
 *
 * pgd_points_locate: pts: host, npts x gdim row-major;  mesh: any layout with cell records - intervals, triangles, tetrahedra,
 * P1 or P2, scalar or blocked; only the vertex part of the records and the vertex coordinates are used.
 *   The cell of a point is the one with the LARGEST SMALLEST barycentric coordinate; among cells whose minima are equal as
 *   doubles the lowest cell index wins.  A maximum below -tol gives cell -1 (lam is then zeros), so does a point with a NaN
 *   coordinate.  A cell whose determinant is zero or not finite is never chosen.  The barycentric coordinates come from the cell's
 *   own vertices - edge matrix, cofactors, determinant, as pgd_cell_gradient forms its inverse Jacobian - and lam_0 = 1 - sum of
 *   the others.  Cells and lam do not depend on the launch shape, bit for bit: (minimum, cell) pairs are compared, never added
 *   (no atomics: persistent workgroups, one row of pairs each, a fixed-order final pass); the points go in tiles of 32, one pair
 *   of launches per tile.  On regularly numbered 3-D box lattices (cell 6 q + t, see PGD_TUNE_ASM_LATTICE) and tol <= 1/8 a thread
 *   per point tests the tetrahedra of the up to 27 cubes around the point instead (PGD_TUNE_LOCATE_LATTICE): the same cells and
 *   lam, bit for bit.  PGD_ERR_INVALID for tol < 0 or not finite and for a null pts with npts > 0.
 *   npts == 0 gives an empty set.  The call synchronises with the host once.
 * pgd_points_from: the set of known (cell, lam) pairs - cells: host int32, lam: host, npts x (gdim + 1).  Cells are checked on the
 *   host against [-1, nc) (PGD_ERR_INVALID, like null cells or lam with npts > 0); -1 is kept.  lam is taken as it is, and so is the cell: the caller answers for a degenerate one (zero
 *   determinant), where sampled gradients are not numbers.
 * pgd_points_download: cells_out (npts) and lam_out (npts x (gdim + 1)), host arrays; either may be NULL.
 * pgd_points_info: the number of points, gdim and the first point whose cell is -1 (-1: none); null outputs are skipped.
 * pgd_points_last_path: what the last pgd_points_locate of the context ran: 0 nothing, 1 the general kernel, 2 the lattice path,
 *   3 the bin index.
 *
 * The bin index (PGD_TUNE_LOCATE_INDEX = 1; 2-D and 3-D meshes, tol <= 2^-10; the lattice path keeps precedence where it applies):
 *   a uniform grid of bins over the bounding box of the mesh, every cell registered in the bins that its bounding box, inflated
 *   by (gdim + 1) (2^-10 + 2^-20) of its extent per axis, touches; a thread per point tests the cells of the point's bin only.
 *   The same cells and lam as the general kernel, bit for bit, on meshes whose edge matrices have a condition below about 2^30.
 *   The index belongs to the scalar layout behind `mesh`: the first indexed call builds it on the device (about 48 cells per bin in
 *   3-D, 8 in 2-D, or PGD_TUNE_LOCATE_INDEX_TARGET; coarsened while it holds more than 16 entries per cell), later calls use it,
 *   a call under another target rebuilds it; pgd_mesh_free or pgd_points_index_drop free it.  A build waits for the host three
 *   times and once more per coarsening (the box, the number of entries, the end); a build that fails leaves no index and no memory.
 * pgd_points_index_info: out[8] = built (0/1), builds so far, bins along x, y, z (1 for a missing axis), entries, the longest
 *   list, device bytes held; all 0 before a build and after a drop.
 * pgd_points_index_download: bin_ptr (bins + 1), bin_cells (entries), geom[9] = origin, inv = bins / extent, bins per axis (as
 *   doubles), 3 each; any may be NULL.  PGD_ERR_INVALID without an index.
 * pgd_points_index_drop: frees the index of the mesh; PGD_OK without one.
 *
 * pgd_points_sample: layout: any P1 or P2 layout, scalar or blocked, over a mesh with the point set's number of cells and gdim
 * (the caller guarantees it is the same mesh);  u: nv*ncomp entries, node*ncomp + c.
 *   what = 0: out[p*ncomp + c] = sum_a N_a(lam_p) u[node_a*ncomp + c], the fma chain from 0 over the record's nodes in
 *   ascending local order; P2: N = l (2 l - 1) at the vertices, 4 l_a l_b on the edges in the order pgd_mesh_upload states
 *   (interval: the one edge).  A point at a node returns the nodal value bit for bit.
 *   what = 1: out[(p*ncomp + c)*gdim + d] = d u_c / d x_d at the point: the cell's constant gradient for P1, the affine one at lam
 *   with the formulas of pgd_cell_gradient_p2 for P2 (the 1-D P2 layout included: its records hold all that is needed).  The
 *   gradient of a point on a face, an edge or a vertex is that of the cell the rule above chose - one-sided.
 *   PGD_ERR_INVALID with a message, before anything is launched, for: a set that holds a cell -1 (the first such point is named:
 *   no gather can go out of range), a layout of another cell count or gdim, u or out of the wrong size (out: npts*ncomp, times
 *   gdim for gradients), out aliasing u, what out of range.  npts == 0 is PGD_OK.  A thread per point; no atomics, no host
 *   synchronisation.                                                                                                          */
int pgd_points_locate(pgd_handle ctx, pgd_handle mesh, const double *pts, int64_t npts, double tol, pgd_handle *points);
int pgd_points_from(pgd_handle ctx, pgd_handle mesh, const int32_t *cells, const double *lam, int64_t npts, pgd_handle *points);
int pgd_points_download(pgd_handle ctx, pgd_handle points, int32_t *cells_out, double *lam_out);
int pgd_points_info(pgd_handle ctx, pgd_handle points, int64_t *npts, int *gdim, int64_t *first_outside);
int pgd_points_last_path(pgd_handle ctx, int *path);
int pgd_points_index_info(pgd_handle ctx, pgd_handle mesh, int64_t *out);
int pgd_points_index_download(pgd_handle ctx, pgd_handle mesh, int32_t *bin_ptr, int32_t *bin_cells, double *geom);
int pgd_points_index_drop(pgd_handle ctx, pgd_handle mesh);
int pgd_points_sample(pgd_handle ctx, pgd_handle points, pgd_handle layout, pgd_handle u, int what, pgd_handle out);
int pgd_points_free(pgd_handle ctx, pgd_handle points);

/* ------------------------------------------------------------------ tuning --- */
/* Launch-shape knobs; they change speed (and the order of the dot's partial
 * sums), never which result is computed (PGD_TUNE_FAULT_ITERATION excepted: a test hook).  */
enum {
    PGD_TUNE_DESIGN_GRID_MAX = 76, /* pgd_design_gains, pgd_design_update: > 0: at most this many (persistent) workgroups per kernel; 0 (default):
                                as many as are resident at once (update: four per CU).  The same bits either way. */
    PGD_TUNE_DESIGN_VARIANT = 75, /* pgd_design_gains: 1 (default) the Jacobians on the f64 matrix unit (k_design_gains_mfma), 0 ordinary fma
                                chains (k_design_gains_plain): the cross-check and the baseline. */
    PGD_TUNE_POSTMANY_SKIP = 74, /* pgd_grid_posterior_many: 1 (default) the exponentials and the third product of a (sample tile, data tile) whose
                                e all underflow to 0 are left out, 0: never.  The same bits either way. */
    PGD_TUNE_POSTMANY_GRID_MAX = 73, /* pgd_grid_posterior_many: > 0: at most this many (persistent) workgroups per kernel; 0 (default): as many
                                as are resident at once.  The same bits either way. */
    PGD_TUNE_POSTMANY_VARIANT = 72, /* pgd_grid_posterior_many: 1 (default) the chained products on the f64 matrix unit (k_postmany_mfma),
                                0 ordinary fma chains (k_postmany_plain): the cross-check and the baseline. */
    PGD_TUNE_POST_GRID_MAX = 71, /* pgd_grid_posterior: > 0: at most this many (persistent) workgroups per kernel; 0 (default): four per CU.  The
                                same bits either way: the segments and the order of their partials do not depend on the grid. */
    PGD_TUNE_POST_VARIANT = 70, /* pgd_grid_posterior, PGD_POST_COEF: 1 (default) the product over the samples on the f64 matrix unit
                                (k_post_coef_mfma), 0 ordinary fma chains (k_post_coef_plain): the cross-check and the baseline. */
    PGD_TUNE_MISFIT_GRID_MAX = 69, /* pgd_grid_misfit: > 0: at most this many (persistent) workgroups; 0 (default): as many as are resident at
                                once.  The same bits either way. */
    PGD_TUNE_MISFIT_VARIANT = 68, /* pgd_grid_misfit: 1 (default) the product on the f64 matrix unit (k_misfit_mfma), 0 ordinary fma chains
                                (k_misfit_plain): the cross-check and the baseline. */
    PGD_TUNE_LOCATE_INDEX_TARGET = 67, /* the bin index of pgd_points_locate: > 0: this many cells per bin; 0 (default): 48 in 3-D, 8 in 2-D.  A
                                call under another value than the index of the mesh was built with rebuilds it.  Same cells and lam. */
    PGD_TUNE_LOCATE_INDEX = 66, /* 1: pgd_points_locate on a 2-D or 3-D mesh with tol <= 2^-10, where the lattice path does not apply, tests a
                                point against the cells of its bin of a uniform grid over the mesh (built on first use, kept with the
                                mesh); 0 (default): never.  Same cells and lam as the general kernel, bit for bit. */
    PGD_TUNE_QUAD_GRID_MAX = 65, /* pgd_quad_forms: > 0: at most this many (persistent) workgroups; 0 (default): as many as are resident at once.
                                The same bits either way. */
    PGD_TUNE_QUAD_VARIANT = 64, /* pgd_quad_forms: 1 (default) the product on the f64 matrix unit (k_quad_mfma), 0 ordinary fma chains
                                (k_quad_plain): the cross-check and the baseline. */
    PGD_TUNE_GRAM_GRID_MAX = 63, /* pgd_vec_gram: > 0: at most this many (persistent) workgroups; 0 (default): as many as are resident at once.
                                The same bits either way: the segments and the order of their partials do not depend on the grid. */
    PGD_TUNE_GRAM_VARIANT = 62, /* pgd_vec_gram: 1 (default) the product on the f64 matrix unit (k_gram_mfma), 0 one fma chain per entry
                                (k_gram_plain): the cross-check and the baseline. */
    PGD_TUNE_LOCATE_GRID_MAX = 61, /* pgd_points_locate, general kernel: > 0: at most this many (persistent) workgroups; 0 (default): as many as
                                are resident at once.  Same cells and lam either way (tests reach the loop over the cells and the final
                                pass over several rows with it). */
    PGD_TUNE_LOCATE_LATTICE = 60, /* 1 (default): pgd_points_locate on a regularly numbered 3-D box lattice with tol <= 1/8 runs a thread per
                                point over the tetrahedra of the cubes around it; 0: the general kernel over all cells.  Same cells and
                                lam, bit for bit. */
    PGD_TUNE_SPMV_P2_LATTICE = 59, /* 1: an OPERATOR (pgd_op_combine) on a P2 layout that pgd_mesh_p2_bind has bound to the 3-D box lattice of its
                                vertices - scalar, or pgd_mesh_blocked of one with 2 or 3 components; at least 3 vertices per axis, the
                                edge list ascending - multiplies over its whole row range from a row-class form in k_spmv_p2lat: every
                                node is (anchor vertex, class 0..7), the columns of a row are a fixed table per class (65 / 27 / 19 slots,
                                built from the six tetrahedra of the unit cube), and the values are one double per (row, slot, column
                                component) in arrays indexed by row - 65 ncomp over the vertex rows, 27 ncomp over the edge rows.  No
                                column stream, every value load coalesced; the form is extracted from the CSR values once per operator
                                and set of values and costs about 1.12 times the CSR value array on top.  Same fma chain per row, same rows
                                per workgroup: y, the partial sums and every pgd_pcg_solve on top (Jacobi or PGD_TUNE_PCG_PRECOND = 4) are
                                those of 0, bit for bit (a zero may change its sign).  A degree-2 operator that gets no form - never
                                bound, refused, 2-D, 2 vertices along an axis, an entry off the table, no memory - keeps k_spmv_csr and
                                is counted (pgd_p2lat_counts); partial row ranges, atoms, pgd_bicgstab_solve and degree-1 layouts are not
                                asked.  With PGD_TUNE_SPMV_BLOCK_DIA on as well an operator that takes this form is not offered to that
                                one.  0 (default): k_spmv_csr.  Measured
                                (profiles/p2_lattice_bench_n1.jsonl): elastic_block of degree 2 31569 -> 2199 us per product at 65^3 vertices,
                                4220 -> 300 us at 33^3, the scalar stiffness 3619 -> 430 and 478 -> 66 us; the "pmg" solve 2653 -> 293 ms and
                                379 -> 60 ms; extraction 21.5 and 2.9 ms per operator */
    PGD_TUNE_SPMV_BLOCK_DIA = 58, /* 1: an OPERATOR (pgd_op_combine) on a blocked layout of 2 or 3 components over a scalar 3-D P1 box lattice
                                (pgd_mesh_blocked of a layout in diagonal form, at least 2 nodes per axis) multiplies over its whole row
                                range from a row-diagonal form - 15 ncomp arrays of one double per row, array (t, d) holding at row
                                ncomp i + c the entry a(row, ncomp (i + off_t) + d) for the 15 lattice offsets in ascending order - in
                                k_spmv_bdia: no column stream, every value load coalesced.  The form is extracted from the CSR values
                                once per operator and set of values (a second pgd_op_combine into the handle extracts again) and costs
                                the CSR value array's size a second time.  Same fma chain per row, same rows per workgroup: y, the partial
                                sums and every pgd_pcg_solve on top are those of 0, bit for bit (a zero may change its sign).  Anything
                                else - P2, 2-D or crossed bases, partial row ranges, atoms, pgd_bicgstab_solve, an entry off the
                                pattern, no memory - keeps k_spmv_csr; pgd_bdia_counts says which.  0 (default): k_spmv_csr.  Measured
                                (profiles/block_dia_bench_n1.jsonl, elastic_block): 7358 -> 533 us per product at 129^3 nodes, 1206 -> 68 us
                                at 65^3; the "cmg" solve 1098 -> 233 ms and 160.7 -> 56.5 ms; extraction 10.7 and 1.4 ms per operator */
    PGD_TUNE_PCG_FUSED_MARCH = 57, /* 1 (default): an iteration of PGD_PCG_FORM_SINGLE_SYNC_RECOMPUTE is k_pcg1_scalars + ONE march (k_pcg1_fused_march):
                                the update on overlapped tiles - a one-cell ring of q, r' and p' is formed redundantly, r alternates
                                between two buffers - and, two planes behind it, the dots p'.Ap' and Ap'.Ap' of the direction it has just
                                written.  The solve issues one stand-alone dot-only product, of p0.  Same operations and summation orders:
                                iterates, iteration counts and residuals are those of 0, bit for bit.  Takes precedence over
                                PGD_TUNE_PCG_FOLD_MARCH.  0: the three-launch loop.  Measured at 256^3 (profiles/pcg_fused_bench.jsonl):
                                48.09 -> 44.99 ms per step, 161.3 -> 150.5 us per iteration; the three-launch loop's own spread is 0.70 ms */
    PGD_TUNE_PCG_SCALAR_S = 56, /* 1 (default): where pgd_pcg_solve holds the scaled operator as a derived stencil (A itself is one stencil plus
                                eliminated nodes), s = d^-1/2 takes exactly two values - (1 / c0)^1/2 on the free rows, 1 on the eliminated
                                ones - and the update march of PGD_TUNE_PCG_RECOMPUTE_Q divides by them in its exact phase instead of
                                reading s (8 B per row less there).  The same quotients, bit for bit.  0: s is streamed */
    PGD_TUNE_PCG_FOLD_MARCH = 55, /* 1: PGD_PCG_FORM_SINGLE_SYNC_RECOMPUTE runs two launches per iteration - every workgroup of
                                the update march sums the product's and the previous update's partial sums itself, in the order of
                                k_pcg1_scalars, and takes the stop test / alpha / beta step on local values (workgroup 0 keeps the scalar
                                bank and the flags).  Same alpha, beta, stop decisions and iterates, bit for bit.  0 (default): k_pcg1_scalars is a
                                launch of its own between the product and the update.  Measured at 256^3: 161.3 -> 160.1 us per
                                iteration, 0.33 ms of 48 per step - less than the run-to-run spread, so it is off */
    PGD_TUNE_BLOCK_STORAGE = 54, /* how pgdrome_amd/spectral.py keeps the Ritz vectors of its start space (pgd_block_storage): 1 (default) a column
                                block in fp32 - the correction is an exact Galerkin projection onto the span that is stored, its Gram
                                matrix is formed from the rounded columns, and only the start vector of a solve depends on it; 2: a
                                column block in f64; 0: k separate f64 vectors, pgd_vec_multidot and pgd_vec_lincomb over them */
    PGD_TUNE_PCG_RECOMPUTE_Q = 53, /* 1 (default): in the three-launch single-sync recurrence of pgd_pcg_solve (PGD_TUNE_PCG_SINGLE_SYNC) on an
                                operator whose products run in k_spmv_stencil_march over the whole grid, q = A p is never stored: the
                                product leaves only its two dots (8 B per row instead of 16) and the vector update is an epilogue of the
                                same march over p that forms q in registers (32 / 48 B per row instead of 40 / 56) and writes the new
                                direction to a second buffer.  Same q, same per-row operations; only the grouping of the residual's
                                partial sums differs.  0: the product stores q and k_pcg1_update reads it */
    PGD_TUNE_EVAL_SAMPLE_CHUNK = 52, /* pgd_eval_batch: samples per launch, 1 .. 1024 (0, default: 1024 - the running per-sample extrema
                                of a workgroup live in LDS beside its block of mode values).  Envelopes and counts accumulate
                                across the chunks; the outputs do not depend on it, bit for bit. */
    PGD_TUNE_EVAL_GRID_MAX = 51, /* pgd_eval_batch: > 0: at most this many (persistent) workgroups; 0 (default): as many as are
                                resident at once.  Same bits either way (tests reach the loop over row blocks with it). */
    PGD_TUNE_EVAL_VARIANT = 50, /* pgd_eval_batch: 1 (default) the product on the f64 matrix unit (k_eval_mfma), 0 ordinary fma chains
                                over k in ascending order (k_eval_plain): the cross-check and the baseline of
                                tools/bench_eval_batch.py.  The two differ by rounding (another summation order), not more. */
    PGD_TUNE_PUSH_IN_UPDATE = 49, /* direct halo (pgd_comm_push_*): 1 (default) the boundary planes of the new search direction leave from the
                                update kernel of the iteration itself - no launch for the exchange at all; 0: k_halo_push in front of
                                every product.  Same stores, same iterates. */
    PGD_TUNE_STENCIL_ROWS = 48, /* rows per thread of k_spmv_stencil_march: 4 (64 x 16 patches), 2 (64 x 8: twice the patches per plane, marches
                                 * twice as long on thin z-slabs), 0 (default): 2 where four-row patches would march fewer than 8 planes.   */
    PGD_TUNE_DIA_MARCH3 = 47, /* 1: the plain z-march of the diagonal form (variant 0: no row classes - variable coefficients, graded meshes) runs
                               * in k_spmv_dia_march3: buffer addressing with lane offsets that never change, the next plane's slot values
                               * loaded while the current plane is multiplied; bit-identical to k_spmv_dia_march2 (0, the default: half the vector
                               * instructions, no faster - the march runs at 0.86-0.92 of what the memory system gives ANY kernel for its nine
                               * streams, profiles/r04_dia_march_counters.txt).                                                            */
    PGD_TUNE_SHARD_ONE_MARCH = 46, /* 1 (default): where the halo exchange of pgd_pcg_solve_sharded runs in stream order and the rank's operator is one
                                stencil whose ghost planes hold the same eliminated nodes as its own (checked per solve), the product is ONE march
                                over all owned planes with the ghost planes staged as data; 0: interior march + the boundary planes in row
                                order (what the overlapped exchange always does).  The same y; the fused dots are grouped differently. */
    PGD_TUNE_HALO_OVERLAP_MIN_ROWS = 45, /* pgd_pcg_solve_sharded sends the halo exchange of its products through the second communicator and
                                stream (pgd_comm_overlap) only where the ranks own at least this many rows on average (default 2^40: never;
                                environment: PGD_HALO_OVERLAP_MIN_ROWS; a property of the current binding).  Measured with one rank as its own
                                neighbour: the second stream loses 15 - 19 us per iteration against the exchange in stream order + one march
                                over all owned planes on the slabs of 8-, 4- and 2-GPU ranks of the 256^3 grid; it pays only where the wire
                                adds more than that.  Decided from the all-reduced row count: the same on every rank. */
    PGD_TUNE_COMM_SELF_PERIODIC = 44, /* tests only: with ONE rank, pgd_pcg_solve_sharded and pgd_comm_halo accept ghost planes on both sides
                                and the rank is its own neighbour - the ghost plane below receives the rank's top plane, the one above its
                                bottom plane (a problem periodic in z): the halo communicator, its stream and events, the overlap with the
                                interior rows' product and real RCCL send / receive run inside the iteration loop on a single GPU */
    PGD_TUNE_PCG_DERIVE_SCALED = 43, /* 1 (default): where the operator of pgd_pcg_solve is itself ONE stencil + eliminated nodes on the whole
                                grid (every row verified, PGD_TUNE_SPMV_STENCIL) the couplings of D^-1/2 A D^-1/2 are derived from A's with
                                the arithmetic the scaling pass would apply to every row - no pass over the slot arrays, no second
                                classification, the slot arrays keep A.  0: scale the slot arrays and classify them (the same couplings,
                                bit for bit). */
    PGD_TUNE_MG_MARCH_MIN = 42, /* multigrid levels with at least this many nodes along x and y run their stencil passes in
                                k_spmv_stencil_march (default 64); smaller ones in the plain kernels of pgd_mg.hip.  The same bound
                                decides between k_vmg_march (the march body of k_spmv_dia_march2 with the cycle's epilogues, pgd_dia_march.h) and
                                the plain kernels of pgd_vmg.hip (PGD_TUNE_PCG_PRECOND = 2). */
    PGD_TUNE_MG_CHUNK = 41, /* PCG iterations queued between two looks at the convergence flags when the multigrid preconditioner is on
                                (even, default 2: an iteration is ~50 launches, the next chunk is queued while the flags of the last travel; the Jacobi form queues 16) */
    PGD_TUNE_PCG_PRECOND = 40, /* preconditioner of pgd_pcg_solve: 0 (default) Jacobi = the symmetric diagonal scaling; 1 a geometric
                                multigrid V(1,1) cycle on the scaled operator WHERE it is one stencil on a lattice whose eliminated
                                nodes are exactly the hull (every row verified, pgd_mg.hip), Jacobi everywhere else.  Changes the
                                iterates (same stop test, same tolerance), not the system solved.  The frontend sets it from
                                settings["preconditioner"] (solver.py:593-594: forwarded to the linear solver).
                                2 (opt-in, the frontend's "vmg"): a geometric multigrid V(1,1) cycle on the scaled operator in DIAGONAL
                                form with per-row coefficients (pgd_vmg.hip) - any scalar P1 operator on a structured vertex lattice
                                (weighted atoms, several materials, Robin terms), any set of eliminated nodes: the coarse operators
                                are the Galerkin products P^T A P, formed on the device once per solve, the smoother is l1-Jacobi.
                                Operators that are one stencil take this cycle as well under 2 (value 1 keeps the cycle of
                                pgd_mg.hip, bit for bit).  Anything else - no lattice, vector-valued or P2 layouts, lattices with
                                fewer than 8 nodes along an axis - takes Jacobi and is counted by pgd_vmg_counts.
                                3 (opt-in, the frontend's "cmg"): BLOCKED (vector-valued) P1 layouts over a 3-D box lattice - one such
                                V-cycle per component on the diagonal blocks of D^-1/2 A D^-1/2, which are scalar operators on the
                                base lattice (separate-displacement-component preconditioning of elasticity); the blocks are read
                                from the CSR values once per solve, the iteration stays the unscaled recurrence on the CSR product.
                                Anything else - scalar or P2 layouts, no lattice, at most 4096 nodes - takes Jacobi and is counted
                                by pgd_cmg_counts.
                                4 (opt-in, the frontend's "pmg"): P2 layouts on tetrahedra, scalar or BLOCKED with 2 or 3 components, whose
                                scalar layout pgd_mesh_p2_bind has bound to the 3-D box lattice of its vertices - p-multigrid:
                                z = D^-1 r + P (M_c (P^T r)_c)_c, P the interpolation from P1 on the same mesh (1 at a vertex, 1/2 from
                                each end of an edge), M_c one such V-cycle on the component's block of P^T A P, a 15-point operator
                                on the vertex lattice formed from the CSR values once per solve; additive, so an iteration has no
                                product beyond its own.  The unscaled recurrence on the CSR product.  Anything else - P1 or unbound
                                layouts, at most 4096 vertices or fewer than 8 along an axis, a term off the pattern, no memory -
                                takes Jacobi and is counted by pgd_pmg_counts. */
    PGD_TUNE_CLS_CACHE = 39, /* 1 (default): a mesh remembers the class codes of the operators classified on it (by the signature of their
                                Dirichlet set, scaled or not): the next operator with that structure - the same atoms with other
                                coefficients, every solve of a fixed-point pass - copies the codes, rebuilds the table from the classes'
                                representative rows and verifies EVERY row against its class bit by bit (any mismatch: full classification);
                                0: always the full classification */
    PGD_TUNE_STENCIL_DEPTH = 38, /* plane fetches in flight per workgroup of k_spmv_stencil_march: 3 or 6 (0, default: chosen by the launcher) */
    PGD_TUNE_STENCIL_WG_PER_CU = 37, /* resident workgroups per CU assumed for k_spmv_stencil_march (default 2): sets the march length */
    PGD_TUNE_SPMV_ZCHUNK_STENCIL = 36, /* > 0: planes per march of k_spmv_stencil_march; 0 (default): as many as fill every resident
                                workgroup slot exactly once, in whole groups of the fetch depth */
    PGD_TUNE_SPMV_STENCIL = 35, /* 1 (default): where the row classes of an operator are ONE 8-tuple plus the rows it becomes next to eliminated
                                (Dirichlet) nodes and the rim of the grid - every row and slot verified bit by bit - the z-march takes the
                                couplings from scalar registers, four rows per thread, and reads the code byte only where the codes of a plane
                                differ from the plane below (k_spmv_stencil_march: 16 B per row); bit-identical y; 0: the dictionary form */
    PGD_TUNE_FAULT_STALL_MS = 34, /* tests only: the next pgd_pcg_solve_sharded queues, once, a kernel that spins for this many
                                milliseconds (bounded: at most 20 000) in front of its first chunk - a stream that makes no progress,
                                for the deadline of pgd_comm_timeout */
    PGD_TUNE_FAULT_STAGE = 33, /* tests only: where the NEXT pgd_pcg_solve_sharded fails on this rank, once: 1 = right after the setup
                                vote, 2 = between the setup's halo exchanges, 3 = between the setup all-reduce and the loop, 4 = after the
                                loop, before the closing agreement (0: nowhere; PGD_TUNE_FAULT_ITERATION: inside the loop) */
    PGD_TUNE_SPMV_ZCHUNK_CODED2 = 32, /* k_spmv_diac_march2 on grids with at least 8 planes of work per resident workgroup slot (two per CU): marches long
                                enough that the launch fills every slot exactly once, at most this many planes (default 96, whole sixes; 0: the
                                PGD_TUNE_SPMV_ZCHUNK_CODED rule everywhere) */
    PGD_TUNE_PCG_PIPELINE = 31, /* 1 (default): pgd_pcg_solve and pgd_pcg_solve_sharded queue the next 16-iteration chunk before the host looks at the
                                flags of the previous one (snapshots into pinned memory, one event each): the GPU does not wait for the
                                host's round trip; a chunk queued behind the iteration that converged consists of no-op launches.  Same
                                iterates, same iteration count.  0: look, then queue */
    PGD_TUNE_PCG_EXACT_PHASE = 30, /* 1 (default): the single-sync recurrence of pgd_pcg_solve_sharded measures the true residual norm (one more
                                vector read per row in the update) only near the end, like pgd_pcg_solve: once d_lb r~.r~ comes within 10^4 of
                                the tolerance, d_lb = (all-reduced sum of d_i^-8)^(-1/8) <= d_min, the same number on every rank; the stop test
                                is the true norm either way.  0: the true norm in every iteration */
    PGD_TUNE_PCG_FOLD_FINISH = 29, /* 1 (default): in the single-sync recurrence of pgd_pcg_solve_sharded every workgroup of the vector update
                                forms the stop decision, alpha and beta itself from the five all-reduced sums (workgroup 0 keeps the books):
                                one launch less per iteration, bit-identical iterates; 0: k_pcg1_finish in a launch of its own */
    PGD_TUNE_LAZY_CSR = 28,  /* 1 (default): where pgd_op_combine can form the operator's diagonal form (structured grids, symmetric atoms) it
                                leaves the CSR values to the first reader that asks for them - the solve, its start and its products read
                                the diagonal form only (1.5 ms less per solve at 256^3); 0: both forms at once */
    PGD_TUNE_ATOM_FAST = 27, /* 1 (default): pgd_spmv with an atom whose diagonal form exists takes the z-march, over the atom's own row
                                classes where it has them (looked for once per atom); 0: always the CSR kernels.  Bit-identical y */
    PGD_TUNE_SPMV_ROWS = 1,  /* rows (= threads) per k_spmv_csr workgroup: 64 (default), 128 or 256 */
    PGD_TUNE_SPMV_GRID_MIN_BYTES = 8, /* ... used when a grid plane of values has at least this many bytes (default 0) */
    PGD_TUNE_PCG_FOLD_REDUCE = 12, /* 1 (default): the scaled recurrence sums its reduction partials inside the vector kernels
                                      (3 dependent launches per iteration instead of 5) for systems of up to 2^20 rows */
    PGD_TUNE_PCG_SCALED = 10,   /* 1 (default): pgd_pcg_solve runs CG on D^-1/2 A D^-1/2 (the same iterates as Jacobi-PCG,
                                   two vector passes per iteration fewer) when the symmetric storage applies; 0: unscaled */
    PGD_TUNE_SPMV_ZCHUNK_FORCE = 7, /* > 0: exactly this many planes per march on any grid size (0: adaptive) */
    PGD_TUNE_PCG_SMALL_ROWS = 26, /* structured grids of up to this many rows take the two-launch form as well (default 2^22: +2 % at 128^3; at 256^3 the redundant sums cost more than the launch they save) */
    PGD_TUNE_PCG_SMALL_SINGLE_SYNC = 25, /* 1 (default): systems of up to 2^20 rows - where the launches, not the bytes, set the pace - run the
                                single-sync recurrence in TWO launches per iteration: the product, and an update kernel whose every workgroup sums
                                the partial sums and forms alpha, beta and the stop decision itself (k_pcg1_step); 0: the two-reduction
                                recurrence in three launches (k_pcg_xr_s2 / k_pcg_p_s2) */
    PGD_TUNE_SPMV_FETCH_DEPTH = 24, /* k_spmv_diac_march2: plane fetches in flight per workgroup, 6 (default, marches of 12+ planes in whole sixes) or 3 */
    PGD_TUNE_PCG_STREAM_HINTS = 23, /* 1 (default): in the single-sync recurrence q, r and x - vectors no other kernel of the iteration touches -
                                are read and written with non-temporal hints, p (read by the product next) keeps the default policy and so its
                                place in the Infinity Cache; same arithmetic, bit-identical results */
    PGD_TUNE_PCG_LAG_X = 22,   /* 1 (default): in the single-sync recurrence of pgd_pcg_solve x - an output accumulator that nothing of the
                                recurrence reads - is updated every OTHER iteration with two terms, the earlier direction taken back out of
                                p = r + beta' p' (5 + 7 instead of 7 + 7 vector passes per two iterations); residuals, directions, alpha, beta and
                                iteration counts are bit-identical to 0, x agrees to the rounding of its own updates */
    PGD_TUNE_SPMV_ZCHUNK_CODED = 21, /* k_spmv_diac_march2: most planes per workgroup march (default 24; whole threes, fewer while that keeps
                                ~2 launches of workgroups per slot); PGD_TUNE_SPMV_ZCHUNK_FORCE overrides it too */
    PGD_TUNE_ASM_LATTICE = 20, /* 1 (default): on a 3-D structured vertex grid whose coordinates are origin + index * step per axis (to 8 ulp,
                                checked at pgd_mesh_upload) the P1 assembly takes every edge component as a whole number of steps instead of
                                the difference of two rounded coordinates: congruent cells get identical local matrices, the rows of a uniform
                                grid repeat bit for bit (relative change of the entries ~ 1e-16) - read off the vertex INDICES where every cell spans at most
                                one step per axis (no coordinate is gathered; the same numbers), and where the cells are numbered regularly - cell 6 q + t =
                                tetrahedron t of cube q - the unweighted atoms gather nothing at all (k_assemble_p1_regular); 3: index steps in the general
                                kernel; 2: the steps from the rounded coordinates (r03);
                                0: coordinate differences as they are */
    PGD_TUNE_SPMV_ROW_CLASSES = 19, /* 1 (default): after scaling, pgd_pcg_solve(_sharded) looks for a lossless ROW-CLASS dictionary of the
                                operator's diagonal form (uniform grids repeat a few 8-tuples of slot values; every row verified bit by
                                bit against its class, at most 255 classes, otherwise none) and the z-march then streams one code byte
                                per row instead of 56 B of slot values (k_spmv_diac_march2): same values, same order, same bits */
    PGD_TUNE_PCG_SINGLE_SYNC = 18, /* 1 (default): scaled recurrence on structured grids above 2^20 rows with ONE reduction and ONE
                                      vector kernel per iteration: the product also leaves q.q, beta comes from
                                      r'.r' = alpha^2 q.q - r.r (exact in exact arithmetic; every alpha and the stop test use the
                                      measured r.r); 7 vector passes and 3 launches per iteration instead of 8 and 5 - 6 passes
                                      where the operator is one stencil and q is formed again by the update instead of stored
                                      (PGD_TUNE_PCG_RECOMPUTE_Q).  0: off */
    PGD_TUNE_UNIT_DIAG = 17,   /* 1 (default): the scaled operator D^-1/2 A D^-1/2 of pgd_pcg_solve(_sharded) gets its diagonal set to
                                  exactly 1 on structured grids and the products do not load it (7 instead of 8 slot values per row);
                                  0: diagonal s_i^2 a_ii stored and loaded */
    PGD_TUNE_PCG_DEFER_X = 16, /* 1 (default): in the scaled recurrence on systems above 2^20 rows the update x += alpha p is done by
                                  the kernel that forms p = r + beta p (which reads p anyway): 8 vector passes per iteration instead
                                  of 9, bit-identical iterates; 0: the x / r kernel + p kernel pair */
    PGD_TUNE_FAULT_ITERATION = 15, /* tests only: pgd_pcg_solve_sharded fails on this rank in that iteration, once (-1: never) -
                                      the other ranks must come out of the solve with an error instead of waiting for it */
    PGD_TUNE_COMBINE_DIA = 14, /* 1 (default): on structured vertex grids pgd_op_combine also forms the operator's diagonal
                                  (symmetric half) storage from the atoms' diagonal forms; 0: converted from CSR per solve */
    PGD_TUNE_SPMV_VARIANT = 13, /* the z-march: 0 (default) k_spmv_dia_march2, 64 x 8 patches, 256 threads, two rows per thread;
                                   1: k_spmv_dia_march<8>, 64 x 8 patches, 512 threads; 2: k_spmv_dia_march<4>, 64 x 4 patches, 256 threads */
    PGD_TUNE_SPMV_ZCHUNK = 6,   /* k_spmv_dia_march* (structured vertex grids, x planes in LDS): most planes per
                                   workgroup march (default 8; fewer while that keeps 4 workgroups per CU); 0 = off */
    PGD_TUNE_SPMV_SYM = 3,   /* 1 (default): the products of the SPD solves (pgd_pcg_solve, pgd_pcg_solve_sharded,
                                pgd_spmv_dot_slot after pgd_op_symmetrize) read the operator from its symmetric
                                half storage when the mesh qualifies (k_spmv_sym); 0: always the CSR kernels */
    PGD_TUNE_SPMV_DICT = 2   /* 1 (default): decode column ids from the mesh's relative-pattern
                                dictionary when it has one (k_spmv_csr_dict16 for rows <= 16 entries, else
                                k_spmv_csr_dict); 2: dictionary, generic kernel only; 0: always stream them */
};
int pgd_tune(pgd_handle ctx, int knob, int64_t value);

/* --------------------------------------------------------------- measuring --- */
/* HIP-event timing of k_spmv_csr launches on the context's stream (SURVEY.md
 * section 8d: roofline.achieved = algorithmic bytes / launch time).
 * on = 1: every launch; on = 2: only the PCG instance (fused dot, stores y).     */
int pgd_prof_enable(pgd_handle ctx, int on);
int pgd_prof_read(pgd_handle ctx, int64_t *launches, double *seconds, double *alg_bytes);
/* ... and the least bytes the timed kernels must move in the storage form they actually read (diagonal /
 * symmetric half storage: 8 W + 16..18 B per row; CSR forms: 12 or 8 B per entry + 20..22 B per row): the
 * physical numerator of roofline.frac when the kernel does not stream the CSR arrays.              */
int pgd_prof_read_own(pgd_handle ctx, double *own_bytes);
/* ... and the same for the vector update of the single-sync recurrence (k_pcg1_update: x += alpha p, r -= alpha q,
 * p = r + beta p and the partial sums of r.r in ONE kernel): launches timed, their seconds, and 56 B per row (4 vectors
 * read, 3 written; 40 where x is left alone) - the kernel that takes most of a PCG iteration once the product reads a code
 * byte per row.  Where the update forms q itself (PGD_TUNE_PCG_RECOMPUTE_Q) it is priced with 48 / 32 B per row.   */
int pgd_prof_read_update(pgd_handle ctx, int64_t *launches, double *seconds, double *bytes);
/* Timed launches that were NOT counted: queued behind the iteration in which their solve converged, every kernel of them returned
 * on the done flag (full bytes, no time - they would bias the averages).  The counts above are the samples that were kept.   */
int pgd_prof_read_dropped(pgd_handle ctx, int64_t *dropped);
/* Seconds a pair of HIP events adds to the kernel it brackets on this context's stream: t(n kernels in one pair) = overhead + n t,
 * measured with n = 1, 2 when the timing is first switched on.  The seconds of pgd_prof_read* are raw event times; bench.py
 * subtracts launches x overhead so that its averages are kernel durations, as rocprofv3 --kernel-trace reports them.       */
int pgd_prof_event_overhead(pgd_handle ctx, double *seconds);
/* Launch counts per product kernel family since the context was created: [0] k_spmv_csr, [1] k_spmv_csr_dict*,
 * [2] k_spmv_sym (row order), [3] k_spmv_dia_rows, [4] k_spmv_dia_march*, [5] k_spmv_multi, [6] k_spmv_diac_march2, [7] k_spmv_stencil_march; tests use them to
 * prove which kernel a call reached, bench.py for its per-kernel breakdown.                          */
int pgd_kernel_counts(pgd_handle ctx, int64_t *out, int n);
/* Launches of the vector update that forms q = A p itself (PGD_TUNE_PCG_RECOMPUTE_Q) since the context was created; they are not
 * product launches and do not enter pgd_kernel_counts.  A chunk of iterations that is replayed as a graph counts once.  */
int pgd_pcg_recompute_counts(pgd_handle ctx, int64_t *updates);
/* Launches of k_pcg1_fused_march (PGD_TUNE_PCG_FUSED_MARCH), counted the same way.  Each of them is an update and a product: it enters
 * pgd_pcg_recompute_counts and family [7] of pgd_kernel_counts as well, and the stand-alone product of p0 does not enter the latter - a
 * solve of k iterations reports k updates and k + 1 stencil marches with the knob at either setting.  */
int pgd_pcg_fused_counts(pgd_handle ctx, int64_t *marches);
/* Row-class classifications since the context was created: done in full (three passes over the slot values with hashing) / served
 * by the mesh's structure cache (codes copied, every row verified against its class: one pass) - PGD_TUNE_CLS_CACHE.   */
int pgd_classify_counts(pgd_handle ctx, int64_t *full, int64_t *cached);
/* Solves that asked for the multigrid preconditioner (PGD_TUNE_PCG_PRECOND = 1) since the context was created: preconditioned by
 * the V-cycle / fallen back to Jacobi because the operator is not one stencil with an eliminated hull.                  */
int pgd_mg_counts(pgd_handle ctx, int64_t *solves, int64_t *fallbacks);
/* The same for PGD_TUNE_PCG_PRECOND = 2 (a solve under 2 does not touch the counters of pgd_mg_counts): solves preconditioned by the
 * variable-coefficient V-cycle / fallen back to Jacobi; levels of the hierarchy the context holds (0: none).              */
int pgd_vmg_counts(pgd_handle ctx, int64_t *solves, int64_t *fallbacks, int64_t *levels);
/* ... and what they cost: device time of the Galerkin setups (eliminated bytes, weights, P^T A P level by level; once per solve) of
 * all those solves in ms, and the number of level passes issued to the z-march kernel k_vmg_march (a chunk of iterations that is
 * replayed as a graph counts once).                                                                                        */
int pgd_vmg_times(pgd_handle ctx, double *setup_ms, int64_t *march_passes);
/* The same pair for PGD_TUNE_PCG_PRECOND = 3 (the counters of pgd_mg_counts and pgd_vmg_counts stay untouched): solves preconditioned
 * by the component-wise V-cycles / fallen back to Jacobi, levels of one component's hierarchy (0: none held); device time of the
 * setups (extraction of the diagonal blocks + ncomp Galerkin chains) in ms and the level passes issued to k_vmg_march.       */
int pgd_cmg_counts(pgd_handle ctx, int64_t *solves, int64_t *fallbacks, int64_t *levels);
int pgd_cmg_times(pgd_handle ctx, double *setup_ms, int64_t *march_passes);
/* ... and for PGD_TUNE_PCG_PRECOND = 4 (the other three pairs of counters stay untouched): solves preconditioned by the p-multigrid
 * cycle / fallen back to Jacobi, levels of one component's hierarchy (0: none held); device time of the setups (eliminated bytes,
 * the blocks of P^T A P from the CSR values, ncomp Galerkin chains) in ms and the level passes issued to k_vmg_march.
 * pgd_pmg_coarse reads back what the last such solve built for component comp: the 8 slot arrays of level 0 (8 nvert doubles, slot
 * dx + 2 dy + 4 dz of vertex I = the entry (I, I + (dx, dy, dz)) of the block) and its eliminated bytes (nvert).                 */
int pgd_pmg_counts(pgd_handle ctx, int64_t *solves, int64_t *fallbacks, int64_t *levels);
int pgd_pmg_times(pgd_handle ctx, double *setup_ms, int64_t *march_passes);
int pgd_pmg_coarse(pgd_handle ctx, int comp, double *slots_out, uint8_t *el_out);
/* PGD_TUNE_SPMV_BLOCK_DIA since the context was created: row-diagonal forms extracted, product launches that read one (a chunk of
 * iterations that is replayed as a graph counts once), operators on a blocked layout that were asked for a whole-range product with
 * the knob on and kept the CSR kernel (each counted once per set of values); device time of the extractions in ms.           */
int pgd_bdia_counts(pgd_handle ctx, int64_t *forms_built, int64_t *products, int64_t *fallbacks);
int pgd_bdia_times(pgd_handle ctx, double *extract_ms);
/* PGD_TUNE_SPMV_P2_LATTICE since the context was created: row-class forms extracted, product launches that read one, operators on
 * a degree-2 layout that were asked for a whole-range product with the knob on and kept the CSR kernel (each counted once per set
 * of values); device time of the extractions in ms.  The counters of PGD_TUNE_SPMV_BLOCK_DIA and of the preconditioners stay untouched. */
int pgd_p2lat_counts(pgd_handle ctx, int64_t *forms_built, int64_t *products, int64_t *fallbacks);
int pgd_p2lat_times(pgd_handle ctx, double *extract_ms);
/* The V-cycle of the multigrid preconditioner on a z-slab of a ROW-SHARDED lattice: settings["preconditioner"] = "amg"
 * (forwarded by the reference into its solver, solver.py:593-594, 634-635) on a sharded spatial dimension.  Level 0 stays
 * with the rows (this rank's planes + one ghost plane per side), levels >= 1 are whole on every rank.  The caller owns the
 * PCG loop and the collectives: per cycle  halo(r) -> pgd_mg_slab_down(r, t) -> halo(t) -> pgd_mg_slab_restrict(t, b1) ->
 * all-reduce(b1) -> pgd_mg_coarse(b1, x1) -> pgd_mg_slab_up(r, x1, t, z, slot, &dot) with r . z over the owned rows.
 *   setup: A (unscaled) must be one stencil + eliminated nodes on the owned planes [own0, own1) of the local array (whole planes),
 *   the eliminated nodes exactly the hull of the global lattice of nz_global planes, local plane 0 = global plane z_first;
 *   *applies = 0 where it is not (the caller keeps Jacobi), *n_coarse = entries of a level-1 vector.                      */
int pgd_mg_slab_setup(pgd_handle ctx, pgd_handle A, int nz_global, int z_first, int64_t own0, int64_t own1,
                      int64_t *n_coarse, int *applies);
int pgd_mg_slab_fix_start(pgd_handle ctx, pgd_handle A, pgd_handle b, pgd_handle x, int64_t own0, int64_t own1);   /* x = b on eliminated owned rows */
int pgd_mg_slab_down(pgd_handle ctx, pgd_handle r, pgd_handle t);
int pgd_mg_slab_restrict(pgd_handle ctx, pgd_handle t, pgd_handle b1);
int pgd_mg_coarse(pgd_handle ctx, pgd_handle b1, pgd_handle x1);
int pgd_mg_slab_up(pgd_handle ctx, pgd_handle r, pgd_handle x1, pgd_handle t, pgd_handle z, int slot, double *dot);   /* slot >= 0: r . z into that scalar slot, no host synchronisation (dot may be NULL) */
/* One HIP-event stopwatch on the context's stream (bench.py's micro-sections: N launches between start
 * and stop; stop synchronises on its event).                                                        */
/* Calibration of the PMC byte model: one pass over `vec` with 8- or 16-byte loads (store = 0) or stores (store = 1)
 * per lane - a known byte count to read FETCH_SIZE / WRITE_SIZE against (tools/pmc_calib.py).         */
int pgd_calib_stream(pgd_handle ctx, pgd_handle vec, int bytes_per_lane, int store);
int pgd_timer_start(pgd_handle ctx);
int pgd_timer_stop(pgd_handle ctx, double *seconds);

#ifdef __cplusplus
}
#endif
#endif /* PGD_AMD_H */
