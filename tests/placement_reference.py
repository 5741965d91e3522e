"""The longdouble restatement of sensor placement (pgd_design_update, pgd_design_gains, PGD.sensor_placement) and the rounding bounds
the tests hold the library to.  Nothing here calls the code under test.

The problem.  Samples s of a tensor grid (last index fastest), weights w_s = prod_d weights_d[i_d], derivative coefficients
cd_t(s) = prod_f U_f[t, i_f] (U_f = dtables_f for f == d, tables_f otherwise), Jacobian of a row p: g_p,d(s) = sum_t a[p, t] cd_t(s),
H_s = H0 + sum_rows g g^T, gain of a candidate (R rows G = [g ..], D x R) = 1/2 sum_s w_s [log det(H_s + G G^T) - log det H_s].  With W
any matrix with W^T W = H^-1 this is 1/2 sum_s w_s log det(I_D + (W G)(W G)^T): ``gains_exact`` evaluates that form by a longdouble
Cholesky factorisation of the D x D matrix - not by the R x R pivots the library takes - for the W it is given.

The bounds (u = 2^-53; first order in u, the neglected O(u^2) terms are covered by the factor 1 + 2^-20; every n u here is < 2^-40).
  g:  cd is a chain of D factors (D - 1 roundings), the sum an accumulation of k products in some order, fused or not:
        |dg_p,d| <= C_G gbar_p,d,   C_G = (k + D) u,   gbar_p,d = sum_t |a[p, t]| |cd_t|.
  V = W g (row i: i + 1 products):  |dV_i| <= (C_G + D u) vbar_i,  vbar_i = sum_j |W_ij| gbar_j.
  G = V^T V (D products):  |dG_ab| <= C_GG Gbar_ab,  C_GG = 2 (C_G + D u) + D u = (2 k + 5 D) u,  Gbar_ab = sum_i vbar_i^a vbar_i^b.
  f = sum_p log(pivot_p) of M = I + G.  The data error: df = tr(M^-1 dG), so |df| <= sum_ab |M^-1|_ab dG_ab.  The elimination is
     backward stable: its pivots are exact for M + dM with |dM| <= (R + 2) u |L||D||L|^T (Higham, Accuracy and Stability, Thm 10.3,
     one more rounding for d = 1 + e), and (|L||D||L|^T)_ab <= sqrt(M_aa M_bb) for a positive definite M.  log1p(e) against log(fl(1 + e)):
     u per pivot; the library's log1p: 4 u |log1p| assumed (a few ulp).
        |df| <= sum_ab |M^-1|_ab (C_GG Gbar_ab + (R + 2) u sqrt(M_aa M_bb)) + R u + 4 u f.
  w_s (D - 1 roundings) times f and the sum over S samples in any order:  (D + 1) u w f per term, S u sum_s w_s f_s.
  gain bound = 1/2 [sum_s w_s (|df_s| + (D + 1) u f_s) + S u sum_s w_s f_s] (1 + 2^-20).
The update.  H_s: R_tot products added to h0 one by one,
        |dH_ij| <= (2 C_G + u) sum_r gbar_i gbar_j + (R_tot + 1) u (|h0_ij| + sum_r gbar_i gbar_j).
  Cholesky: Lc Lc^T = H + dHc, |dHc| <= (D + 2) u |L||L|^T (Thm 10.3); forward substitution of the columns of I: Lc Wc = I + Dl,
  |Dl| <= (D + 2) u |L||W| (Thm 8.5).  Then Wc Lc = I + F, |F| <= (D + 2) u |W||L||W||L| =: (D + 2) u B, and
        |Wc H Wc^T - I| <= (D + 2) u (B + B^T + |W||L||L|^T|W|^T) (1 + 2^-20)         (``w_backward_bound``; L from H in longdouble).
  Wc^T Wc is the exact inverse of H + dH_eff, |dH_eff| <= dH + (D + 2) u (|L||L|^T + |L||W||H| + |H||W|^T|L|^T)   (``state_error``).
  log det: -2 sum log Wc_ii = log det(H + dH') - roundings:  sum_ij |H^-1|_ij (dH_ij + (D + 2) u (|L||L|^T)_ij) + 2 D u +
  (8 + 2 D) u sum_i |log W_ii| per sample; the expected covariance sum w H^-1: |H^-1| dH_eff |H^-1| + (D + 1) u |W|^T|W| per sample;
  both then (D + 1 + S) u sum_s w_s |value_s| for the weights and the sum.
A gain formed at a state with the error dH_eff differs from the gain at the exact state by at most
        1/2 sum_s w_s sum_ij sqrt(Hinv_ii Hinv_jj) dH_eff_ij        (``state_term``)
because d/dH [log det(H + G G^T) - log det H] = (H + G G^T)^-1 - H^-1, a negative semi-definite matrix whose entries are bounded by
sqrt(Hinv_ii Hinv_jj).  The constants are derived, not fitted; the tests print error / bound."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20


def recipe(grid, k, M, R, seed=None):
    """The seeded inputs of a shape (grid, k, M, R): tables 1 + 0.5 N(0, 1), dtables N(0, 1), rows N(0, 1) / sqrt(k) times a
    per-candidate scale in [0.3, 3], weights uniform in [0.2, 1] normalised, H0 = B B^T + D I."""
    D = len(grid)
    rng = np.random.default_rng(1000 * D + 10 * k + M + 7 * R + sum(grid) if seed is None else seed)
    tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
    dtables = [rng.standard_normal((k, n)) for n in grid]
    scale = rng.uniform(0.3, 3.0, M)
    a = np.ascontiguousarray((rng.standard_normal((M, R, k)) / np.sqrt(k) * scale[:, None, None]).reshape(M * R, k))
    weights = []
    for n in grid:
        w = rng.uniform(0.2, 1.0, n)
        weights.append(w / w.sum())
    B = rng.standard_normal((D, D))
    H0 = B @ B.T + D * np.eye(D)
    return dict(grid=tuple(grid), k=k, M=M, R=R, D=D, tables=tables, dtables=dtables, a=a, weights=weights, H0=0.5 * (H0 + H0.T))


def grid_of(tables, dtables, weights):
    """The derivative coefficients (longdouble and absolute), weights and sizes of a grid."""
    n = [t.shape[1] for t in tables]
    D, k, S = len(n), tables[0].shape[0], int(np.prod(n, dtype=np.int64))
    idx = np.unravel_index(np.arange(S), n)
    CD = np.ones((D, k, S), dtype=LD)
    for d in range(D):
        for f in range(D):
            CD[d] *= np.asarray(dtables[f] if f == d else tables[f], dtype=LD)[:, idx[f]]
    w = np.ones(S, dtype=LD)
    for d in range(D):
        w *= np.asarray(weights[d], dtype=LD)[idx[d]]
    return dict(n=n, D=D, k=k, S=S, CD=CD, CDabs=np.abs(CD).astype(np.float64), w=w)


def jacobians(g, rows):
    """(G, Gbar): G[d] (P, S) longdouble Jacobians of the rows, Gbar[d] = |rows| |cd| (float64, rounded up)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, g["k"])
    G = np.stack([rows.astype(LD) @ g["CD"][d] for d in range(g["D"])])
    Gbar = np.stack([np.abs(rows) @ g["CDabs"][d] for d in range(g["D"])]) * (1.0 + 1e-12)
    return G, Gbar


def chol_inv(H):
    """(L, W): the lower Cholesky factors of the matrices H (.., D, D) and their inverses, in H's precision."""
    D = H.shape[-1]
    L, W = np.zeros_like(H), np.zeros_like(H)
    for i in range(D):
        for j in range(i + 1):
            t = H[..., i, j] - (L[..., i, :j] * L[..., j, :j]).sum(axis=-1)
            L[..., i, j] = np.sqrt(t) if i == j else t / L[..., j, j]
    for j in range(D):
        W[..., j, j] = 1 / L[..., j, j]
        for i in range(j + 1, D):
            W[..., i, j] = -(L[..., i, j:i] * W[..., j:i, j]).sum(axis=-1) / L[..., i, i]
    return L, W


def logdet(H):
    L, _ = chol_inv(H)
    return 2 * np.log(np.einsum("...ii->...i", L)).sum(axis=-1)


def unpack_state(state, D, S):
    """(H, W) as (S, D, D) arrays from the plane-major packed state vector (H symmetric, W lower)."""
    nh = D * (D + 1) // 2
    st = np.asarray(state).reshape(2 * nh, S)
    H, W = np.zeros((S, D, D)), np.zeros((S, D, D))
    iu, il = np.triu_indices(D), np.tril_indices(D)
    H[:, iu[0], iu[1]] = st[:nh].T
    H[:, iu[1], iu[0]] = st[:nh].T
    W[:, il[0], il[1]] = st[nh:].T
    return H, W


def pack_state(H, W):
    """The packed state vector of (S, D, D) arrays H and W."""
    D = H.shape[-1]
    iu, il = np.triu_indices(D), np.tril_indices(D)
    return np.ascontiguousarray(np.concatenate([H[:, iu[0], iu[1]].T, W[:, il[0], il[1]].T]).reshape(-1))


def gains_exact(g, a, R, W, block=32):
    """(gains, bounds) of the M candidates (rows of a: M R x k) at the state W (S, D, D), W^T W = H^-1: the longdouble gains from the
    D x D form and the derived rounding bound of each (module docstring)."""
    D, S, k = g["D"], g["S"], g["k"]
    a = np.asarray(a, dtype=np.float64).reshape(-1, k)
    M = a.shape[0] // R
    Wl, Wa = np.asarray(W, dtype=LD), np.abs(np.asarray(W, dtype=np.float64))
    w = g["w"]
    wf = w.astype(np.float64)
    c_gg = (2 * k + 5 * D) * U
    gains, bounds = np.zeros(M, dtype=LD), np.zeros(M)
    for j0 in range(0, M, block):
        j1 = min(M, j0 + block)
        m = j1 - j0
        G, Gbar = jacobians(g, a[j0 * R:j1 * R])                               # (D, m R, S)
        V = np.stack([np.einsum("sj,jps->ps", Wl[:, i, :i + 1], G[:i + 1]) for i in range(D)]).reshape(D, m, R, S)
        Bm = np.einsum("imrs,jmrs->msij", V, V) + np.eye(D, dtype=LD)
        f = logdet(Bm)                                                          # (m, S)
        gains[j0:j1] = 0.5 * (f * w).sum(axis=1)
        # ---- the bound
        vbar = np.stack([np.einsum("sj,jps->ps", Wa[:, i, :i + 1], Gbar[:i + 1]) for i in range(D)]).reshape(D, m, R, S)
        Gb = np.einsum("imas,imbs->msab", vbar, vbar)
        Vf = V.astype(np.float64)
        Mm = np.einsum("imas,imbs->msab", Vf, Vf) + np.eye(R)
        Minv = np.abs(np.linalg.inv(Mm))
        dg = np.einsum("msaa->msa", Mm)
        dM = c_gg * Gb + (R + 2) * U * np.sqrt(dg[..., :, None] * dg[..., None, :])
        ff = f.astype(np.float64)
        df = (Minv * dM).sum(axis=(2, 3)) + R * U + 4 * U * ff
        tot = (wf * ff).sum(axis=1)
        bounds[j0:j1] = 0.5 * ((wf * (df + (D + 1) * U * ff)).sum(axis=1) + S * U * tot) * SLACK
    return gains, bounds


def h_exact(g, h0, rows):
    """(H, dH): H_s = h0 + sum_rows g g^T in longdouble (S, D, D) and the rounding bound of its entries after one or many updates."""
    D, S, k = g["D"], g["S"], g["k"]
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, k)
    H = np.broadcast_to(np.asarray(h0, dtype=LD), (S, D, D)).copy()
    dH = np.zeros((S, D, D))
    habs = np.broadcast_to(np.abs(np.asarray(h0, dtype=np.float64)), (S, D, D)).copy()
    if rows.shape[0]:
        G, Gbar = jacobians(g, rows)
        H += np.einsum("irs,jrs->sij", G, G)
        gg = np.einsum("irs,jrs->sij", Gbar, Gbar)
        dH = (2 * (k + D) * U + U) * gg
        habs += gg
    return H, (dH + (rows.shape[0] + 1) * U * habs) * SLACK


def state_error(H, dH):
    """dH_eff: W^T W of a computed state is the exact inverse of H + E, |E| <= dH_eff."""
    D = H.shape[-1]
    Hf = np.asarray(H, dtype=np.float64)
    L, W = chol_inv(Hf)
    La, Wa, Ha = np.abs(L), np.abs(W), np.abs(Hf)
    LW = La @ Wa
    return dH + (D + 2) * U * (La @ La.transpose(0, 2, 1) + LW @ Ha + Ha @ LW.transpose(0, 2, 1)) * SLACK


def state_term(g, H, dH_eff):
    """What the error of a state adds to the bound of every gain formed at it."""
    Hinv = np.linalg.inv(np.asarray(H, dtype=np.float64))
    dg = np.sqrt(np.einsum("sii->si", Hinv))
    per = (dg[:, :, None] * dg[:, None, :] * dH_eff).sum(axis=(1, 2))
    return 0.5 * float((g["w"].astype(np.float64) * per).sum()) * SLACK


def w_backward_bound(Hk, Wk):
    """(E, bound): E = W H W^T - I in longdouble for a state (H, W) as the library left it, and the bound of its entries."""
    D = Hk.shape[-1]
    Hl, Wl = np.asarray(Hk, dtype=LD), np.asarray(Wk, dtype=LD)
    E = Wl @ Hl @ Wl.transpose(0, 2, 1) - np.eye(D, dtype=LD)
    L, _ = chol_inv(Hl)
    La, Wa = np.abs(L).astype(np.float64), np.abs(np.asarray(Wk, dtype=np.float64))
    B = Wa @ La @ Wa @ La
    return E, (D + 2) * U * (B + B.transpose(0, 2, 1) + Wa @ La @ La.transpose(0, 2, 1) @ Wa.transpose(0, 2, 1)) * SLACK


def sums_exact(g, H, dH):
    """(logdet, bound, cov, bound): sum_s w_s log det H_s and sum_s w_s H_s^-1 in longdouble with the bounds of what the update reports."""
    D, S = g["D"], g["S"]
    w, wf = g["w"], g["w"].astype(np.float64)
    L, W = chol_inv(np.asarray(H, dtype=LD))
    ld = 2 * np.log(np.einsum("sii->si", L)).sum(axis=1)
    Hinv = W.transpose(0, 2, 1) @ W
    Hia, La, Wa = np.abs(Hinv).astype(np.float64), np.abs(L).astype(np.float64), np.abs(W).astype(np.float64)
    LLt = La @ La.transpose(0, 2, 1)
    lw = np.abs(np.log(np.einsum("sii->si", Wa))).sum(axis=1)
    d_ld = (Hia * (dH + (D + 2) * U * LLt)).sum(axis=(1, 2)) + 2 * D * U + (8 + 2 * D) * U * lw
    ldf = ld.astype(np.float64)
    b_ld = ((wf * d_ld).sum() + (D + 1 + S) * U * (wf * np.abs(ldf)).sum()) * SLACK
    d_cov = Hia @ state_error(H, dH) @ Hia + (D + 1) * U * (Wa.transpose(0, 2, 1) @ Wa)
    b_cov = (np.einsum("s,sij->ij", wf, d_cov) + (D + 1 + S) * U * np.einsum("s,sij->ij", wf, Hia)) * SLACK
    return (w * ld).sum(), float(b_ld), np.einsum("s,sij->ij", w, Hinv), b_cov


def greedy(g, a, R, H0, n_select, installed=(), exclude=()):
    """The greedy selection in longdouble.  Returns a dict: ``selected``; per free step ``gains`` (M,) and ``bounds`` (M,) of all
    candidates (the bound of a gain formed by the library at ITS state: the gain's own bound plus the state's term), ``gap``: the
    relative distance between the best and the runner-up on offer; ``installed_gains`` / ``installed_bounds``; ``logdet`` /
    ``logdet_bound`` and ``cov`` / ``cov_bound`` after 0, 1, .. sensors."""
    k = g["k"]
    a = np.asarray(a, dtype=np.float64).reshape(-1, k)
    M = a.shape[0] // R
    rows = np.zeros((0, k))
    out = dict(selected=[], gains=[], bounds=[], gap=[], installed_gains=[], installed_bounds=[], logdet=[], logdet_bound=[], cov=[], cov_bound=[])
    taken = np.zeros(M, dtype=bool)
    taken[list(exclude)] = True
    taken[list(installed)] = True

    def at_state():
        H, dH = h_exact(g, H0, rows)
        ld, b_ld, cov, b_cov = sums_exact(g, H, dH)
        out["logdet"].append(ld), out["logdet_bound"].append(b_ld), out["cov"].append(cov), out["cov_bound"].append(b_cov)
        _, W = chol_inv(H)
        return W, state_term(g, H, state_error(H, dH))

    W, st = at_state()
    for j in installed:
        gj, bj = gains_exact(g, a[j * R:(j + 1) * R], R, W)
        out["installed_gains"].append(gj[0]), out["installed_bounds"].append(bj[0] + st)
        rows = np.concatenate([rows, a[j * R:(j + 1) * R]])
        W, st = at_state()
    for _ in range(n_select):
        gains, bounds = gains_exact(g, a, R, W)
        offered = np.where(taken, -np.inf, gains.astype(np.float64))
        order = np.argsort(-offered, kind="stable")
        j = int(order[0])
        out["gap"].append(float((gains[j] - gains[order[1]]) / gains[j]) if (~taken).sum() > 1 else np.inf)
        out["selected"].append(j), out["gains"].append(gains), out["bounds"].append(bounds + st)
        taken[j] = True
        rows = np.concatenate([rows, a[j * R:(j + 1) * R]])
        W, st = at_state()
    return out
