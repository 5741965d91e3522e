"""The host-driven PCG pieces of the C ABI (pgd_pcg_*_slot, pgd_cg_*_slot, pgd_spmv_dot_slot) and the vector kernels next to
them, each called on uploaded device state and compared with the plain reference (tests/slot_reference.py) applied to the same
inputs.  Every step starts from uploaded state, so no error accumulates into a bar.

Elementwise results are exact (one IEEE division per scalar, explicit fmas and plain products per entry): bit for bit.  A sum
is held to D * 2^-53 * sum |a_i b_i| with D counted from the kernels (``reduce_depth``).
"""
import functools

import numpy as np
import pytest

from tests import slot_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LDU = 2.0 ** -64            # unit roundoff of np.longdouble (64-bit significand), the format the long case's bounds are formed in
ERR_INVALID = -1
TPB, MAX_BLOCKS = 256, 2048         # pgd_internal.h: threads per workgroup, grid cap of the grid-stride kernels


def reduce_depth(count, pair=False):
    """Additions (roundings) on the longest path from a product to the slot, counted from the code:
      - the lane's chain of fmas over its grid-stride trips (k_pcg_init, k_cg_init, k_cg_update, k_pcg_xr<false>: one entry per
        trip; k_pcg_xr<true>: two per trip, and lane 0 of workgroup 0 takes the odd tail entry as well);
      - block_sum: 6 shuffle steps of wave_sum, then (s0 + s1) + (s2 + s3) from LDS: 2;
      - k_reduce_partials (at most 2048 partials: no first stage): 1 into one of the 8 accumulators, 3 for their tree, 6 shuffle
        steps, 16 for the sequential sum over the waves."""
    if count <= 0:
        return 0
    if pair:
        items = (count + 1) // 2
        lanes = min((items + TPB - 1) // TPB, MAX_BLOCKS) * TPB
        npair = count // 2
        chain = 2 * ((npair + lanes - 1) // lanes) + (count & 1)
    else:
        lanes = min((count + TPB - 1) // TPB, MAX_BLOCKS) * TPB
        chain = (count + lanes - 1) // lanes
    return chain + 6 + 2 + 1 + 3 + 6 + 16


assert reduce_depth(R.LONG, pair=True) == 39 and reduce_depth(R.LONG) == 37 and 39 * U <= 1e-13      # within the bar of the project's dots


# ------------------------------------------------------------------ device state
class OpRef:
    """An operator argument: the device handle for the library, the scipy matrix for the reference."""

    def __init__(self, handle, A):
        self.handle, self.A = handle, A


def set_flags(ctx, flags):
    """Bring the device flags to (done, iterations, status) with the pieces themselves (the ABI has only a reset): `check` on a
    residual above its bar counts, `tol` on a start that meets the bar - or on a NaN - raises done.  Uses slots 0 and 1."""
    done, iters, status = flags
    ctx.flags_reset()
    ctx.slots_upload(np.array([1.0, 0.0]), 0)
    for _ in range(iters):
        ctx.pcg_check_slot(0, 1)                      # r.r = 1 > tol^2 = 0: live
    if status == R.ERR_SINGULAR:
        ctx.slots_upload(np.array([np.nan, 0.0]), 0)
        ctx.pcg_tol_slot(1.0, 0.0, 0, 1, 1)
    elif done:
        ctx.slots_upload(np.array([0.0, 1.0]), 0)
        ctx.pcg_tol_slot(1.0, 0.0, 0, 1, 1)          # tol^2 = 1 >= r.r = 0
    assert ctx.flags() == tuple(flags)


def device_run(ctx, st, calls):
    """Upload the vectors the calls name, the flags and the slots of ``st``; make the calls; download everything."""
    names = sorted({a for _, args in calls for a in args if isinstance(a, str)})
    h = {k: ctx.vec_from(st.v[k]) for k in names}
    try:
        set_flags(ctx, st.flags)
        ctx.slots_upload(st.S, 0)
        for name, args in calls:
            getattr(ctx, name)(*[h[a] if isinstance(a, str) else a.handle if isinstance(a, OpRef) else a for a in args])
        out = R.State({k: ctx.vec_download(h[k]) for k in names}, ctx.slots_download(0, R.NSLOTS), ctx.flags())
    finally:
        for v in h.values():
            ctx.vec_free(v)
    return out


REF_FN = {"pcg_init_slot": R.pcg_init, "pcg_tol_slot": R.pcg_tol, "pcg_xr_slot": R.pcg_xr, "pcg_check_slot": R.pcg_check,
          "pcg_p_slot": R.pcg_p, "cg_init_slot": R.cg_init, "cg_update_slot": R.cg_update, "cg_scalars_slot": R.cg_scalars,
          "spmv_dot_slot": R.spmv_dot_slot}


def reference_run(st, calls):
    ref = st.copy()
    for name, args in calls:
        REF_FN[name](ref, *[a.A if isinstance(a, OpRef) else a for a in args])
    return ref


def check_slots(got, ref, sums, what):
    """Slots that hold a sum: within D * 2^-53 * sum |a_i b_i| of the exact sum of the DEVICE's own entries.  Every other slot -
    scalar results, and the sentinels of the slots the piece does not own - bit for bit."""
    memo = {}
    for i in range(R.NSLOTS):
        if i in sums and i in ref.mag:
            a, b, k, depth = sums[i]
            if (a, b, k.start, k.stop) not in memo:
                memo[a, b, k.start, k.stop] = R.exact_dot(got.v[a][k], got.v[b][k]), R.abs_dot(got.v[a][k], got.v[b][k])
            exact, mag = memo[a, b, k.start, k.stop]
            bar = (1e-13 if depth is None else depth * U) * mag
            assert abs(got.S[i] - exact) <= bar, (what, "slot", i, got.S[i], exact, abs(got.S[i] - exact) / (mag * U + 1e-300))
            if k.stop == k.start:
                assert R.same_bits(got.S[i], 0.0), (what, "slot", i, "an empty range writes +0")
        else:
            assert R.same_bits(got.S[i], ref.S[i]), (what, "slot", i, got.S[i], ref.S[i])
    assert tuple(got.flags) == tuple(ref.flags), (what, "flags", got.flags, ref.flags)


# ------------------------------------------------------------------ the vector pieces
def _k(n, lo, hi):
    return slice(lo, n if hi < 0 else hi)


def vector_pieces(n, lo, hi):
    """name -> (arguments, {slot: (a, b, range, depth)} of the sums it writes, pure outputs)."""
    k = _k(n, lo, hi)
    cnt = k.stop - k.start
    d1, dx = reduce_depth(cnt), reduce_depth(cnt, pair=(lo % 2 == 0))
    return {
        "pcg_init_slot": (("b", "q", "dinv", "r", "z", "p", lo, hi, 30),
                          {30: ("r", "z", k, d1), 31: ("r", "r", k, d1), 32: ("b", "b", k, d1)}, ("r", "z", "p")),
        "pcg_xr_slot": (("x", "r", "p", "q", "dinv", "z", lo, hi, 9, 10, 33), {33: ("r", "z", k, dx), 34: ("r", "r", k, dx)}, ("z",)),
        "pcg_p_slot": (("p", "z", lo, hi, 9, 10), {}, ()),
        # (slots 40..42: the scratch triple holds the same sums)
        "cg_init_slot": (("b", "q", "dinv", "r", "u", "p", "s", lo, hi, 24),
                         {24: ("r", "u", k, d1), 25: ("r", "r", k, d1), 32: ("b", "b", k, d1),
                          40: ("r", "u", k, d1), 41: ("r", "r", k, d1), 42: ("b", "b", k, d1)}, ("r", "u", "p", "s")),
        "cg_update_slot": (("x", "r", "u", "w", "p", "s", "dinv", lo, hi, 24), {24: ("r", "u", k, d1), 25: ("r", "r", k, d1)}, ()),
    }


WRITES = {"pcg_init_slot": ("r", "z", "p"), "pcg_xr_slot": ("x", "r", "z"), "pcg_p_slot": ("p",),
          "cg_init_slot": ("r", "u", "p", "s"), "cg_update_slot": ("x", "r", "u", "p", "s")}
GATED = ("pcg_xr_slot", "pcg_p_slot", "cg_update_slot")        # no-ops once the done flag is set (init and cg_init still write)


@functools.lru_cache(maxsize=2)
def _base_state(n):
    return R.make_state(n, 1000 + n % 997)


def prepared(n, outputs=(), flags=(0, 0, 0)):
    st = _base_state(n).copy()
    for k in outputs:
        st.v[k][:] = R.SENTINEL
    st.S[9], st.S[10] = 0.8125, 1.75          # alpha (xr) / beta (p): a quotient that is not a float
    st.S[29], st.S[30] = 0.6, -0.35           # alpha, beta of the single-reduction update (base 24)
    st.flags = list(flags)
    return st


@pytest.mark.parametrize("piece", ["pcg_init_slot", "pcg_xr_slot", "pcg_p_slot", "cg_init_slot", "cg_update_slot"])
@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_vector_piece_small(ctx, case, piece):
    n, label, lo, hi = case
    args, sums, outputs = vector_pieces(n, lo, hi)[piece]
    for flags in ((0, 2, 0), (1, 2, 0)):
        st = prepared(n, outputs, flags)
        calls = [(piece, args)]
        ref, got = reference_run(st, calls), device_run(ctx, st, calls)
        what = (piece, label, flags)
        for name in got.v:
            # inside the range: the reference, bit for bit (explicit fmas, plain products, one division per scalar);
            # outside it, and in every input vector: untouched, bit for bit (the reference leaves them as they were)
            assert R.same_bits(got.v[name], ref.v[name]), (what, name, np.flatnonzero(R.bits(got.v[name]) != R.bits(ref.v[name]))[:8])
        check_slots(got, ref, sums, what)
        if flags[0] and piece in GATED:                # the done flag: vectors, slots and flags exactly as uploaded
            assert all(R.same_bits(got.v[name], st.v[name]) for name in got.v) and R.same_bits(got.S, st.S)
        if sums:                                       # a reduction run twice gives identical bits (fixed-order sums)
            again = device_run(ctx, st, calls)
            assert R.same_bits(again.S, got.S), what


def sample_indices(n):
    """The entries of the long case that are compared bit for bit with the exact reference: every 257th, 600 around the start
    of the second grid-stride trip of the one-entry-per-lane kernels (2048 * 256) and of the two-entries-per-lane kernels
    (2 * 2048 * 256), and the last 600."""
    parts = [np.arange(0, n, 257), np.arange(524288 - 300, 524288 + 300), np.arange(1048576 - 300, min(1048576 + 300, n)),
             np.arange(n - 600, n)]
    return np.unique(np.concatenate(parts))


def fma_within_bound(got, a, b, c, what):
    """got = fma(a, b, c) entry by entry to ONE rounding of the exact a b + c: (2^-53 + 2 * 2^-64) (|a b| + |c|), the second term
    for the two roundings of the np.longdouble evaluation it is compared with."""
    ld = np.longdouble
    ab = np.asarray(a, dtype=ld) * np.asarray(b, dtype=ld)
    c = np.asarray(c, dtype=ld)
    err = np.abs(np.asarray(got, dtype=ld) - (ab + c))
    bar = (ld(U) + 2 * ld(LDU)) * (np.abs(ab) + np.abs(c))
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, (what, bad[:8])


def long_entries(piece, st, got, k):
    """All entries of the long case: each output against the values it is formed from - the uploaded inputs, or the device's own
    intermediate where the kernel feeds one forward - so that every comparison spans one rounding, or none."""
    v0, v, S = st.v, got.v, st.S
    if piece in ("pcg_init_slot", "cg_init_slot"):          # one IEEE subtraction, one product: numpy's are the same operations
        z = "z" if piece == "pcg_init_slot" else "u"
        assert R.same_bits(v["r"][k], v0["b"][k] - v0["q"][k]) and R.same_bits(v[z][k], v0["dinv"][k] * v["r"][k])
        if piece == "pcg_init_slot":
            assert R.same_bits(v["p"][k], v["z"][k])
        else:
            assert R.same_bits(v["p"][k], np.zeros(k.stop - k.start)) and R.same_bits(v["s"][k], np.zeros(k.stop - k.start))
    elif piece == "pcg_xr_slot":
        alpha = S[9] / S[10]
        fma_within_bound(v["x"][k], alpha, v0["p"][k], v0["x"][k], "x")
        fma_within_bound(v["r"][k], -alpha, v0["q"][k], v0["r"][k], "r")
        assert R.same_bits(v["z"][k], v0["dinv"][k] * v["r"][k])
    elif piece == "pcg_p_slot":
        fma_within_bound(v["p"][k], S[9] / S[10], v0["p"][k], v0["z"][k], "p")
    else:
        alpha, beta = S[29], S[30]
        fma_within_bound(v["p"][k], beta, v0["p"][k], v0["u"][k], "p")
        fma_within_bound(v["s"][k], beta, v0["s"][k], v0["w"][k], "s")
        fma_within_bound(v["x"][k], alpha, v["p"][k], v0["x"][k], "x")
        fma_within_bound(v["r"][k], -alpha, v["s"][k], v0["r"][k], "r")
        assert R.same_bits(v["u"][k], v0["dinv"][k] * v["r"][k])


@pytest.mark.parametrize("piece", ["pcg_init_slot", "pcg_xr_slot", "pcg_p_slot", "cg_init_slot", "cg_update_slot"])
@pytest.mark.parametrize("case", R.all_cases((R.LONG,)), ids=R.case_id)
def test_vector_piece_long(ctx, case, piece):
    """Past the grid cap: the second (third) trip of every grid-stride loop and its ragged tail."""
    n, label, lo, hi = case
    args, sums, outputs = vector_pieces(n, lo, hi)[piece]
    st = prepared(n, outputs)
    used = [a for a in args if isinstance(a, str)]
    calls = [(piece, args)]
    got = device_run(ctx, st, calls)
    k = _k(n, lo, hi)
    what = (piece, label)
    # the sampled entries: the exact reference on the gathered sub-vectors (every entry is formed from its own index alone)
    idx = sample_indices(n)
    idx = idx[(idx >= k.start) & (idx < k.stop)]
    sub = R.State({a: st.v[a][idx] for a in used}, st.S, st.flags)
    j = [i for i, a in enumerate(args) if not isinstance(a, str)][:2]          # (lo, hi) are the first two numbers of every piece
    sub_args = tuple(0 if i == j[0] else -1 if i == j[1] else a for i, a in enumerate(args))
    REF_FN[piece](sub, *sub_args)
    for name in used:
        assert R.same_bits(got.v[name][idx], sub.v[name]), (what, name, "sampled entries")
    long_entries(piece, st, got, k)
    for name in used:                                  # outside the range, and input vectors: untouched
        if name in WRITES[piece]:
            assert R.same_bits(got.v[name][:k.start], st.v[name][:k.start]) and R.same_bits(got.v[name][k.stop:], st.v[name][k.stop:]), (what, name)
        else:
            assert R.same_bits(got.v[name], st.v[name]), (what, name, "an input")
    ref = st.copy()
    ref.mag = dict.fromkeys(sums, 0.0)                 # (check_slots forms the exact sums from the device's entries)
    check_slots(got, ref, sums, what)
    if sums and label in ("whole", "odd_lo"):
        assert R.same_bits(device_run(ctx, st, calls).S, got.S), what


# ------------------------------------------------------------------ the scalar pieces
def scalar_state(rr, bb, d_hi, flags=(0, 4, 0)):
    st = R.State({}, 1000.0 + np.arange(R.NSLOTS), flags)
    st.S[11], st.S[12], st.S[13] = rr, bb, 1e-6 * 100.0
    st.S[24:33] = [2.5, rr, 1.25, 0.5, d_hi, 0.6, 0.3, 3.5, bb]
    st.S[5] = 1e-6 * 100.0
    return st


SCALAR_CALLS = [("pcg_tol_slot", (1e-3, 0.0, 11, 12, 13)), ("pcg_tol_slot", (1e-9, 1.0, 11, 12, 13)), ("pcg_check_slot", (11, 13)),
                ("cg_scalars_slot", (24, 1, 1e-3, 0.0)), ("cg_scalars_slot", (24, 0, 1e-3, 0.0)), ("cg_scalars_slot", (24, 0, 1e-9, 1.0))]
NAN = float("nan")


@pytest.mark.parametrize("call", SCALAR_CALLS, ids=lambda c: "%s%s" % (c[0], "-".join(str(a) for a in c[1])))
def test_scalar_pieces_bit_for_bit(ctx, call):
    """tol, check and cg_scalars: every slot bit for bit (one IEEE operation after the other, in the kernel's order), the slots
    they do not own untouched - S[5] and S[6] are owned as the header says - and the flags as in the reference: live, bar met,
    NaN in r.r, NaN in the summed w.u, NaN in b.b, and under the done flag (tol alone still acts)."""
    for rr, bb, d_hi in ((3.0, 100.0, 0.125), (9e-5, 100.0, 0.125), (0.5, 100.0, 0.125), (NAN, 100.0, 0.125), (3.0, 100.0, NAN),
                         (3.0, NAN, 0.125), (1e-9, NAN, 0.125), (0.0, 0.0, 0.0)):
        for flags in ((0, 4, 0), (1, 4, 0)):
            st = scalar_state(rr, bb, d_hi, flags)
            ref, got = reference_run(st, [call]), device_run(ctx, st, [call])
            check_slots(got, ref, {}, (call, rr, bb, d_hi, flags))
            if flags[0] and call[0] != "pcg_tol_slot":
                assert R.same_bits(got.S, st.S)


# ------------------------------------------------------------------ the product, and sequences of pieces
@pytest.fixture(scope="module")
def box(ctx):
    from oracle import fem_numpy as F
    P = R.hull_problem("box")
    mh = ctx.mesh_upload(P["coords"], P["cells"])
    ak, am = ctx.atom_assemble(mh, F.STIFF), ctx.atom_assemble(mh, F.MASS)
    op = ctx.op_combine(mh, [ak, am], [1.0, 1.0], P["bc"])
    P["op"] = OpRef(op, P["A"])
    P["rowabs"] = abs(P["A"])
    yield P
    for a in (op, ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(mh)


def check_product(got, st, P, x, y, k, what):
    """y = A x on the rows of the range to the bar of the project's products (4e-15 of sum |a_ij x_j|: the order in which a
    product kernel adds a row's terms is its own); outside the range untouched."""
    ref, rowabs = P["A"] @ st.v[x], P["rowabs"] @ np.abs(st.v[x])
    worst = float(np.max(np.abs(got.v[y][k] - ref[k]) / (rowabs[k] + 1e-300))) if k.stop > k.start else 0.0
    assert worst <= 4e-15, (what, worst)
    assert R.same_bits(got.v[y][:k.start], st.v[y][:k.start]) and R.same_bits(got.v[y][k.stop:], st.v[y][k.stop:]), what
    assert R.same_bits(got.v[x], st.v[x]), what


@pytest.mark.parametrize("rng", [(0, -1), (2, 499), (3, 500), (251, 252), (252, 252), (504, 504)], ids=str)
def test_spmv_dot_slot(ctx, box, rng):
    """The product piece: rows of the range only, the sum of w_i y_i over them to the bar of the project's dots, zero for an empty
    range, nothing at all once the done flag is set."""
    lo, hi = rng
    n = box["n"]
    k = _k(n, lo, hi)
    for flags in ((0, 0, 0), (1, 0, 0)):
        st = prepared(1000, flags=flags)
        st.v = {a: b[:n].copy() for a, b in st.v.items()}
        st.v["q"][:] = R.SENTINEL
        # (x of like-sized entries: the bar of the product is relative to sum |a_ij x_j| with the ORACLE's matrix, whose entries
        # differ from the assembled ones by the roundings of cell contributions that cancel; w keeps its wide range)
        st.v["p"] = np.random.default_rng(99).uniform(-1.0, 1.0, n)
        calls = [("spmv_dot_slot", (box["op"], "p", "q", "w", lo, hi, 31))]
        got = device_run(ctx, st, calls)
        what = ("spmv_dot_slot", rng, flags)
        if flags[0]:
            assert all(R.same_bits(got.v[a], st.v[a]) for a in got.v) and R.same_bits(got.S, st.S) and got.flags == list(flags), what
            continue
        check_product(got, st, box, "p", "q", k, what)
        assert R.same_bits(got.v["w"], st.v["w"])
        ref = st.copy()
        ref.mag[31] = 0.0
        check_slots(got, ref, {31: ("w", "q", k, None)}, what)


def test_breakdown_stops_every_piece(ctx, box):
    """A NaN in S[rr] (check, tol), then in S[base + 1] and S[base + 2] (cg_scalars): done = 1, status = PGD_ERR_SINGULAR, the
    iteration count as in the reference, and every later piece a no-op.  Ordinary arithmetic on the 64-slot bank."""
    n = box["n"]
    later = [("pcg_xr_slot", ("x", "r", "p", "q", "dinv", "z", 0, -1, 9, 10, 33)), ("pcg_check_slot", (34, 13)),
             ("pcg_p_slot", ("p", "z", 1, n, 9, 10)), ("cg_update_slot", ("x", "r", "u", "w", "p", "s", "dinv", 0, n, 24)),
             ("cg_scalars_slot", (24, 0, 1e-3, 0.0)), ("spmv_dot_slot", (box["op"], "p", "q", "p", 0, n, 31)),
             ("pcg_xr_slot", ("x", "r", "p", "q", "dinv", "z", 7, 7, 9, 10, 33))]
    firsts = [(11, ("pcg_check_slot", (11, 13)), (1, 3, R.ERR_SINGULAR)), (11, ("pcg_tol_slot", (1e-3, 0.0, 11, 12, 13)), (1, 2, R.ERR_SINGULAR)),
              (25, ("cg_scalars_slot", (24, 0, 1e-3, 0.0)), (1, 3, R.ERR_SINGULAR)), (26, ("cg_scalars_slot", (24, 0, 1e-3, 0.0)), (1, 3, R.ERR_SINGULAR)),
              (27, ("cg_scalars_slot", (24, 1, 1e-3, 0.0)), (1, 2, R.ERR_SINGULAR))]
    for slot, first, flags_want in firsts:
        st = prepared(1000, flags=(0, 2, 0))
        st.v = {a: b[:n].copy() for a, b in st.v.items()}
        st.S[slot] = NAN
        stopped = reference_run(st, [first])
        assert tuple(stopped.flags) == flags_want
        got = device_run(ctx, st, [first] + later)
        for a in got.v:
            assert R.same_bits(got.v[a], st.v[a]), (first, a)
        check_slots(got, stopped, {}, first)          # (the reference of the FIRST call alone: the later ones changed nothing)


def test_done_flag_raised_by_tol(ctx, box):
    """The flag raised the way a solve raises it - tol on a start that meets the bar - turns xr, check, p, cg_update, cg_scalars
    and spmv_dot_slot into no-ops; init and cg_init still write."""
    n = box["n"]
    st = prepared(1000)
    st.v = {a: b[:n].copy() for a, b in st.v.items()}
    st.S[11], st.S[12] = 1e-7, 100.0                  # r.r <= (1e-3)^2 b.b
    tol = ("pcg_tol_slot", (1e-3, 0.0, 11, 12, 13))
    gated = [("pcg_xr_slot", ("x", "r", "p", "q", "dinv", "z", 0, -1, 9, 10, 33)), ("pcg_check_slot", (34, 13)),
             ("pcg_p_slot", ("p", "z", 1, n, 9, 10)), ("cg_update_slot", ("x", "r", "u", "w", "p", "s", "dinv", 0, n, 24)),
             ("cg_scalars_slot", (24, 0, 1e-3, 0.0)), ("spmv_dot_slot", (box["op"], "p", "q", "p", 0, n, 31)),
             ("cg_update_slot", ("x", "r", "u", "w", "p", "s", "dinv", 5, 5, 24))]
    ref = reference_run(st, [tol])
    assert ref.flags == [1, 0, 0]
    got = device_run(ctx, st, [tol] + gated)
    assert all(R.same_bits(got.v[a], st.v[a]) for a in got.v)
    check_slots(got, ref, {}, "gated")
    k1, k2 = slice(3, n - 2), slice(2, n - 3)
    d = reduce_depth(n)
    writers = [(("pcg_init_slot", ("b", "q", "dinv", "r", "z", "p", 3, n - 2, 50)),
                {50: ("r", "z", k1, d), 51: ("r", "r", k1, d), 52: ("b", "b", k1, d)}),
               (("cg_init_slot", ("b", "q", "dinv", "r", "u", "p", "s", 2, n - 3, 24)),
                {24: ("r", "u", k2, d), 25: ("r", "r", k2, d), 32: ("b", "b", k2, d),
                 40: ("r", "u", k2, d), 41: ("r", "r", k2, d), 42: ("b", "b", k2, d)})]
    for writer, sums in writers:
        got, ref = device_run(ctx, st, [tol, writer]), reference_run(st, [tol, writer])
        assert ref.flags == [1, 0, 0] and all(R.same_bits(got.v[a], ref.v[a]) for a in got.v), writer
        assert not R.same_bits(got.v["r"], st.v["r"])
        check_slots(got, ref, sums, writer)


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch(ctx, box):
    """Slot indices outside [0, PGD_NSLOTS) - for the pair and triple writers, the last slot written - vectors of another size
    and bad ranges: PGD_ERR_INVALID, and slots, flags and vectors exactly as they were."""
    from pgdrome_amd import _lib
    n = 300
    st = prepared(1000, flags=(0, 3, 0))
    st.v = {a: b[:n].copy() for a, b in st.v.items()}
    names = sorted(st.v)
    h = {a: ctx.vec_from(st.v[a]) for a in names}
    short = ctx.vec_from(st.v["x"][:n - 1])
    set_flags(ctx, st.flags)
    ctx.slots_upload(st.S, 0)
    good = {
        "pcg_init_slot": [h["b"], h["q"], h["dinv"], h["r"], h["z"], h["p"], 1, n - 1, 30],
        "pcg_tol_slot": [1e-3, 0.0, 11, 12, 13],
        "pcg_xr_slot": [h["x"], h["r"], h["p"], h["q"], h["dinv"], h["z"], 1, n - 1, 9, 10, 33],
        "pcg_check_slot": [11, 13],
        "pcg_p_slot": [h["p"], h["z"], 1, n - 1, 9, 10],
        "cg_init_slot": [h["b"], h["q"], h["dinv"], h["r"], h["u"], h["p"], h["s"], 1, n - 1, 24],
        "cg_update_slot": [h["x"], h["r"], h["u"], h["w"], h["p"], h["s"], h["dinv"], 1, n - 1, 24],
        "cg_scalars_slot": [24, 0, 1e-3, 0.0],
    }
    # position of every slot argument and the number of consecutive slots written from it on
    slot_args = {"pcg_init_slot": {8: 3}, "pcg_tol_slot": {2: 1, 3: 1, 4: 1}, "pcg_xr_slot": {8: 1, 9: 1, 10: 2}, "pcg_check_slot": {0: 1, 1: 1},
                 "pcg_p_slot": {4: 1, 5: 1}, "cg_init_slot": {9: 9}, "cg_update_slot": {9: 9}, "cg_scalars_slot": {0: 9}}
    range_at = {"pcg_init_slot": 6, "pcg_xr_slot": 6, "pcg_p_slot": 2, "cg_init_slot": 7, "cg_update_slot": 7}
    refused = 0
    try:
        for name, args in good.items():
            bad = []
            for pos, width in slot_args[name].items():
                for value in {R.NSLOTS, -1, R.NSLOTS - width + 1}:      # 64, -1, and the first index whose LAST slot is out of range
                    bad.append(args[:pos] + [value] + args[pos + 1:])
            if name in range_at:
                pos = range_at[name]
                bad.append(args[:pos] + [n - 1, 1] + args[pos + 2:])        # lo > hi
                bad.append(args[:pos] + [0, n + 1] + args[pos + 2:])        # hi > n
                bad.append(args[:pos] + [-1, n] + args[pos + 2:])           # lo < 0
                for i in range(pos):                                        # every vector argument: another size
                    bad.append(args[:i] + [short] + args[i + 1:])
            for a in bad:
                with pytest.raises(_lib.PgdError) as e:
                    getattr(ctx, name)(*a)
                assert e.value.code == ERR_INVALID, (name, a)
                refused += 1
        for value in (R.NSLOTS, -1):
            with pytest.raises(_lib.PgdError) as e:
                ctx.spmv_dot_slot(box["op"].handle, h["x"], h["q"], h["x"], 0, 0, value)
            assert e.value.code == ERR_INVALID
        assert refused >= 70
        assert ctx.flags() == tuple(st.flags) and R.same_bits(ctx.slots_download(0, R.NSLOTS), st.S)
        for a in names:
            assert R.same_bits(ctx.vec_download(h[a]), st.v[a]), a
        for name, args in good.items():                # ... and the same calls with good arguments are accepted
            getattr(ctx, name)(*args)
    finally:
        for v in list(h.values()) + [short]:
            ctx.vec_free(v)


# ------------------------------------------------------------------ two ranges in one process
class CtxBackend:
    """_lib.Context under the names the drivers of tests/slot_reference.py use."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.slots_get, self.slots_set = ctx.slots_download, ctx.slots_upload

    def __getattr__(self, name):
        return getattr(self.ctx, name)


@pytest.mark.parametrize("form", ["pcg", "cg"])
def test_two_ranges_in_one_process(ctx, box, form):
    """Both recurrences with the rows split at an odd row (not plane-aligned): every piece once per half with its own slot
    indices, the halves' slots added on the host in place of the all-reduce.  The same stop iteration +-2 as the whole-range
    run, x within 1e-8 of the direct solve, and after the stop one more full round of calls changes nothing."""
    P, be = box, CtxBackend(ctx)
    n = P["n"]
    m = (n // 2) | 1
    names = ("x", "b", "r", "z", "u", "w", "p", "s", "q", "dinv")
    rounds, xs = [], []
    for ranges in ([(0, n, 0)], [(0, m, 0), (m, n, R.HALF)]):
        V = {a: ctx.vec_from(P["b"] if a == "b" else np.zeros(n)) for a in names}
        try:
            ctx.slots_upload(1000.0 + np.arange(R.NSLOTS), 0)
            ctx.op_diag_inv(P["op"].handle, V["dinv"])
            assert np.allclose(ctx.vec_download(V["dinv"]), 1.0 / P["A"].diagonal(), rtol=1e-12, atol=0.0)
            if form == "pcg":
                k, rz = R.drive_pcg(be, P["op"].handle, V, ranges, 1e-10, 0.0, 500)
            else:
                k = R.drive_cg(be, P["op"].handle, V, ranges, 1e-10, 0.0, 500)
            assert ctx.flags() == (1, k, 0)
            before = ({a: ctx.vec_download(V[a]) for a in names}, ctx.slots_download(0, R.NSLOTS))
            allreduce = R.HostAllreduce(be, [0])       # (library calls only: a host sum of the frozen slots WOULD change them)
            if form == "pcg":
                R.pcg_round(be, P["op"].handle, V, ranges, allreduce, k, rz)
            else:
                R.cg_round(be, P["op"].handle, V, ranges, allreduce, 1e-10, 0.0)
            assert ctx.flags() == (1, k, 0) and R.same_bits(ctx.slots_download(0, R.NSLOTS), before[1])
            for a in names:
                assert R.same_bits(ctx.vec_download(V[a]), before[0][a]), (a, "changed after the stop")
            rounds.append(k)
            xs.append(before[0]["x"])
        finally:
            for v in V.values():
                ctx.vec_free(v)
    assert abs(rounds[0] - rounds[1]) <= 2 and 0 < rounds[0] < 500, rounds
    for x in xs:
        assert np.linalg.norm(x - P["sol"]) <= 1e-8 * np.linalg.norm(P["sol"])


# ------------------------------------------------------------------ the vector kernels next to them
@pytest.mark.parametrize("n", R.SIZES + (R.LONG,))
def test_vec_mul(ctx, n):
    """y = a .* x: one IEEE product per entry, also with y aliasing x and y aliasing a."""
    rng = np.random.default_rng(n)
    a, x = R.wide(rng, n), R.wide(rng, n)
    av, xv, yv = ctx.vec_from(a), ctx.vec_from(x), ctx.vec_from(np.full(n, R.SENTINEL))
    ctx.vec_mul(yv, av, xv)
    assert R.same_bits(ctx.vec_download(yv), a * x) and R.same_bits(ctx.vec_download(av), a) and R.same_bits(ctx.vec_download(xv), x)
    ctx.vec_mul(xv, av, xv)
    assert R.same_bits(ctx.vec_download(xv), a * x) and R.same_bits(ctx.vec_download(av), a)
    ctx.vec_upload(xv, x)
    ctx.vec_mul(av, av, xv)
    assert R.same_bits(ctx.vec_download(av), a * x) and R.same_bits(ctx.vec_download(xv), x)
    short = ctx.vec_alloc(n + 1)
    from pgdrome_amd import _lib
    with pytest.raises(_lib.PgdError):
        ctx.vec_mul(yv, av, short)
    for v in (av, xv, yv, short):
        ctx.vec_free(v)


def lincomb_terms(n, k, seed):
    """k distinct vectors cut from one random stream, each with its own scale, and k coefficients."""
    rng = np.random.default_rng(seed)
    stream = R.wide(rng, n + 7 * k)
    scale = 10.0 ** rng.uniform(-2, 2, k)
    return [stream[7 * t:7 * t + n] * scale[t] for t in range(k)], rng.uniform(-2.0, 2.0, k)


def fma_chain(xs, coefs, idx):
    s = np.zeros(idx.size)
    for x, c in zip(xs, coefs):
        s = R.fma_vec(c, x[idx], s)
    return s


@pytest.mark.parametrize("k", [64, 65, 128, 130])
def test_lincomb_across_launches(ctx, k):
    """More than 64 terms take another launch that accumulates into y: still ONE fma chain from 0 through all terms in
    ascending order, bit for bit (the header's promise)."""
    n = 257
    xs, coefs = lincomb_terms(n, k, 40 + k)
    hs = [ctx.vec_from(x) for x in xs]
    yv = ctx.vec_from(np.full(n, R.SENTINEL))
    ctx.vec_lincomb(yv, hs, coefs)
    assert R.same_bits(ctx.vec_download(yv), fma_chain(xs, coefs, np.arange(n)))
    for t in (0, k - 1):
        assert R.same_bits(ctx.vec_download(hs[t]), xs[t])
    for v in hs + [yv]:
        ctx.vec_free(v)


def test_lincomb_long(ctx):
    """65 terms past the grid cap: the sampled entries bit for bit, the rest within 65 roundings of the chain (+ the 130 of the
    np.longdouble evaluation it is compared with), relative to sum |c_t x_t|."""
    n, k = R.LONG, 65
    xs, coefs = lincomb_terms(n, k, 7)
    hs = [ctx.vec_from(x) for x in xs]
    yv = ctx.vec_from(np.full(n, R.SENTINEL))
    ctx.vec_lincomb(yv, hs, coefs)
    y = ctx.vec_download(yv)
    for v in hs + [yv]:
        ctx.vec_free(v)
    idx = sample_indices(n)
    assert R.same_bits(y[idx], fma_chain(xs, coefs, idx))
    ld = np.longdouble
    s, mag = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    for x, c in zip(xs, coefs):
        t = ld(c) * x.astype(ld)
        s += t
        mag += np.abs(t)
    assert np.all(np.abs(y.astype(ld) - s) <= (k * ld(U) + 2 * k * ld(LDU)) * mag)


def test_lincomb_inplace_refuses_a_second_launch(ctx):
    from pgdrome_amd import _lib
    n, k = 257, 65
    xs, coefs = lincomb_terms(n, k, 3)
    hs = [ctx.vec_from(x) for x in xs]
    with pytest.raises(_lib.PgdError) as e:
        ctx.vec_lincomb_inplace(hs[0], hs, coefs)
    assert e.value.code == ERR_INVALID and R.same_bits(ctx.vec_download(hs[0]), xs[0])
    ctx.vec_lincomb_inplace(hs[0], hs[:64], coefs[:64])          # 64 terms, the first one y itself: one launch
    assert R.same_bits(ctx.vec_download(hs[0]), fma_chain(xs[:64], coefs[:64], np.arange(n)))
    for v in hs:
        ctx.vec_free(v)


def test_vector_ops_past_the_grid_cap(ctx):
    """axpy, scale, fill, copy and dot at a size where every grid-stride loop takes a third trip with a ragged tail, to the bars of
    test_vector_ops (elementwise: exact up to the fma's single rounding; the dot: 1e-13 of sum |x_i y_i|)."""
    n = R.LONG
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    xv, yv = ctx.vec_from(x), ctx.vec_from(y)
    ctx.vec_axpy(yv, -0.75, xv)
    got = ctx.vec_download(yv)
    assert np.allclose(got, y - 0.75 * x, rtol=1e-15, atol=1e-15)
    fma_within_bound(got, -0.75, x, y, "axpy")
    idx = sample_indices(n)
    assert R.same_bits(got[idx], R.fma_vec(-0.75, x[idx], y[idx]))
    for lo, hi in ((0, -1), (3, n - 2)):
        k = _k(n, lo, hi)
        d = ctx.vec_dot(xv, yv, lo, hi)
        assert abs(d - R.exact_dot(x[k], got[k])) <= 1e-13 * R.abs_dot(x[k], got[k])
        assert abs(d - R.exact_dot(x[k], got[k])) <= reduce_depth(k.stop - k.start) * U * R.abs_dot(x[k], got[k])
        assert d == ctx.vec_dot(xv, yv, lo, hi)
    ctx.vec_scale(xv, 3.0)
    assert np.array_equal(ctx.vec_download(xv), 3.0 * x)
    ctx.vec_fill(yv, 2.5)
    assert np.all(ctx.vec_download(yv) == 2.5)
    ctx.vec_copy(yv, xv)
    assert np.array_equal(ctx.vec_download(yv), 3.0 * x)
    ctx.vec_free(xv)
    ctx.vec_free(yv)
