"""The vertical diffusivity per interface and cell: the numpy twin (tests/tracer_vfield_twin.py) against its long-double restatement within
the counted bounds, forwards, backwards and in the density; the transpose identity; the consequences include/moka_hip.h states (a uniform
field is the scalar bit for bit, a zero interface decouples the column, an all-zero field keeps every bit); D[k,c] against central
differences of a long-double forward in single field entries; the twin's scan of a field; the sheared mesh.  No GPU needed.  The counted constants (C_BR_F, C_LV_F) and
their derivation are in the twin's docstring; every bounded test prints the largest ratio to its bound."""
import os
import re

import numpy as np
import pytest

import tracer_biharmonic_twin as tb
import tracer_cases as tc
import tracer_kgrad_twin as tk
import tracer_vfield_twin as tf
import tracer_vgrad_twin as tg
import tracer_vmix_twin as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tv.LD
U = tv.U53
NAMES = ("moka_tracer_vertical_field_upload", "moka_tracer_vertical_field_download", "moka_tracer_has_vertical_field")
NCOL, K = 40, 60
DEPTHS = np.array([0, 1, 2, 2, 3, 3, 5, 17, 34, 59] + [60] * 30)
SH2 = (1e-9, 1e-3, 0.3, 2.0, 36.0, 1e3, 1e5)             # dt f / h^2 at the top of the field's range
DT = 8.0
STEP = (("A", None, None), None)                          # the GPU cases' model: tracer 0 a field, tracer 1 scalar 0, tracer 2 a scalar


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_exist():
    from moka_hip import lib as L
    for name in NAMES:
        assert hasattr(L.lib(), name) and name in L.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "moka_hip.h")).read()
    assert re.search(r"int\s+moka_tracer_vertical_field_upload\(moka_state \*st, int32_t j, const double \*host\);", hdr)
    assert re.search(r"int\s+moka_tracer_vertical_field_download\(moka_state \*st, int32_t j, double \*host\);", hdr)
    assert re.search(r"int\s+moka_tracer_has_vertical_field\(const moka_state \*st, int32_t j, int \*out\);", hdr)
    assert "s[k] = dt * f_j[k,c]" in hdr and "w[k] = s[k] / (0.5 * (h[k] + h[k+1]))" in hdr
    assert "only the derivative at the uniform point is delivered" not in hdr
    jl = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "julia", "MokaHIP.jl")).read()
    for name in NAMES:
        assert f"(:{name}, lib)" in jl, name
    src = open(os.path.join(ROOT, "mpas-ocean.jl_amd", "csrc", "tracer_vmix.hip")).read()
    assert "Y[q] = a.dt * vs[u].x" in src                 # the in-place staging into set 2: the three-set rule of the plain instances stands
    assert "vmix_kernel(a.K, generic, 4)" in src and src.count("vmix_kernel(a.K, generic)") == 1


# ---- columns ------------------------------------------------------------------------------------------------------------------------
def columns(seed=3):
    """test_tracer_vmix_twin.py's 40 columns of K = 60 with mixed depths, and a diffusivity per interface in [0, 1] with every seventh
    entry an exact zero."""
    rng = np.random.default_rng(seed)
    h = 10.0 * rng.uniform(0.5, 2.0, (NCOL, K))
    x, X = rng.uniform(0.5, 1.5, (NCOL, K)), rng.uniform(-1.0, 1.0, (NCOL, K))
    f = rng.uniform(0.0, 1.0, (NCOL, K))
    f.ravel()[::7] = 0.0
    return h, x, X, f


def groups():
    for n in np.unique(DEPTHS):
        if n >= 2:
            yield int(n), np.nonzero(DEPTHS == n)[0]


def solve_with_bounds(h, r, dt, f):
    """(z^, A, Ainv, res, fwd, w): the twin's solve with s = dt * f, and res = |A||z^| + |r|, fwd = |A^-1| res in long double."""
    w = tv.weights(h, np.float64(dt) * f)
    z = tv.solve(w, tv.diagonal(h, w), r)
    A, inv = tf.dense_ld_field(h, dt, f)
    res = tv.mv(np.abs(A), np.abs(z)) + np.abs(r).astype(LD)
    return z, A, inv, res, tv.mv(np.abs(inv), res), w


def test_dense_restatement_is_the_scalar_one_for_a_uniform_field():
    h = columns()[0][:5, :9]
    A, inv = tf.dense_ld_field(h, 1.0, np.full((5, 8), 37.5))
    B, binv = tv.dense_ld(h, 37.5)
    assert np.array_equal(A, B) and np.array_equal(inv, binv)
    assert np.array_equal(A, np.transpose(A, (0, 2, 1)))
    off = np.abs(A).sum(axis=2) - np.abs(A[:, np.arange(9), np.arange(9)])
    assert np.all(A[:, np.arange(9), np.arange(9)] > off)                 # strictly diagonally dominant


def test_forward_and_reverse_within_the_counted_bounds():
    """Both lines of the recipe against S = A^-1 diag(h) and S^T = diag(h) A^-1 of the long-double matrix, per element, and the
    transpose identity <X, S x> = <S^T X, x> within the two bounds."""
    h, x, X, f0 = columns()
    worst = [0.0, 0.0, 0.0, 0.0]
    for sh2 in SH2:
        f = f0 * (sh2 * 100.0 / DT)
        for n, idx in groups():
            hh, xx, XX, ff = h[idx, :n], x[idx, :n], X[idx, :n], f[idx, :n - 1]
            s = np.float64(DT) * ff
            w = tv.weights(hh, s)
            r = tv.Lv(w, xx)
            z, A, inv, res, fwd, _ = solve_with_bounds(hh, r, DT, ff)
            resid = np.abs(tv.mv(A, z) - r.astype(LD))
            assert np.all(resid <= tf.C_BR_F * U * res), (sh2, n)
            worst[0] = max(worst[0], float((resid / np.where(res > 0, U * res, 1)).max()))    # (res == 0: a decoupled level with r == 0)
            Sx = tv.forward_cols(hh, xx, s)
            assert np.array_equal(Sx, xx + z)
            errF = U * (tf.C_BR_F * fwd + tf.C_LV_F * tv.mv(np.abs(inv), tv.Lv_abs(w, xx)) + np.abs(Sx))
            zr, _, _, _, fwdr, _ = solve_with_bounds(hh, XX, DT, ff)
            StX = tv.reverse_cols(hh, XX, s)
            errR = U * (tf.C_BR_F * tv.Lv_abs(w, fwdr) + tf.C_LV_F * tv.Lv_abs(w, zr) + np.abs(StX))
            hl = hh.astype(LD)
            eF, eR = np.abs(Sx - tv.mv(inv, hl * xx)), np.abs(StX - hl * tv.mv(inv, XX))
            assert np.all(eF <= errF) and np.all(eR <= errR), (sh2, n)
            worst[1] = max(worst[1], float((eF / errF).max()))
            worst[2] = max(worst[2], float((eR / errR).max()))
            lhs, rhs = (XX.astype(LD) * Sx).sum(axis=1), (StX.astype(LD) * xx).sum(axis=1)
            bound = (np.abs(XX) * errF).sum(axis=1) + (errR * np.abs(xx)).sum(axis=1)
            assert np.all(np.abs(lhs - rhs) <= bound), (sh2, n)
            worst[3] = max(worst[3], float((np.abs(lhs - rhs) / bound).max()))
    print(f"residual / (2^-53 (|A||z| + |r|)) = {worst[0]:.2f} (C_BR_F = {tf.C_BR_F}); forward / bound = {worst[1]:.3f}; reverse / bound = "
          f"{worst[2]:.3f}; |<X, S x> - <S^T X, x>| / bound = {worst[3]:.3f}")


def test_unit_column_range_and_content():
    """The unit tracer stays exactly 1.0; the column content is conserved within tracer_vmix_twin's content bound (with the field's
    counts); every value stays inside its column's former range up to the forward error."""
    h, x, _, f0 = columns()
    worst_c = worst_m = 0.0
    for sh2 in SH2:
        f = f0 * (sh2 * 100.0 / DT)
        assert np.all(tf.apply_field(h, np.ones((NCOL, K)), DEPTHS, DT, f) == 1.0)
        for n, idx in groups():
            hh, xx, ff = h[idx, :n], x[idx, :n], f[idx, :n - 1]
            w = tv.weights(hh, np.float64(DT) * ff)
            z, A, inv, res, fwd, _ = solve_with_bounds(hh, tv.Lv(w, xx), DT, ff)
            new = xx + z
            hl = hh.astype(LD)
            drift = np.abs((hl * new).sum(axis=1) - (hl * xx).sum(axis=1))
            bound = U * (tf.C_BR_F * res + tf.C_LV_F * tv.Lv_abs(w, xx) + hl * np.abs(new)).sum(axis=1)
            assert np.all(drift <= bound), (sh2, n)
            worst_c = max(worst_c, float((drift / bound).max()))
            slack = U * (tf.C_BR_F * fwd + tf.C_LV_F * tv.mv(np.abs(inv), tv.Lv_abs(w, xx)) + np.abs(new))
            over = np.maximum(new - xx.max(axis=1)[:, None], xx.min(axis=1)[:, None] - new)
            assert np.all(over <= slack), (sh2, n)
            worst_m = max(worst_m, float((over / slack).max()))
    print(f"content drift / bound: {worst_c:.3f}; largest excursion beyond the column's range / slack: {worst_m:.3f}")


def test_a_zero_interface_decouples_the_column():
    """f == 0 at interface m: w[m] = g[m] = 0, the parts above and below are the solves of the two shorter columns, bit for bit, and
    each part conserves its own content within the content bound."""
    h, x, X, f0 = columns()
    n, m = 60, 23
    idx = np.nonzero(DEPTHS == n)[0]
    worst = 0.0
    for sh2 in SH2:
        f = f0 * (sh2 * 100.0 / DT) + 1e-300                              # no other zero in these columns
        f[:, m] = 0.0
        hh, xx, XX, ff = h[idx, :n], x[idx, :n], X[idx, :n], f[idx, :n - 1]
        s = np.float64(DT) * ff
        for fn, v in ((tv.forward_cols, xx), (tv.reverse_cols, XX)):
            whole = fn(hh, v, s)
            assert np.array_equal(whole[:, :m + 1], fn(hh[:, :m + 1], v[:, :m + 1], s[:, :m]))
            assert np.array_equal(whole[:, m + 1:], fn(hh[:, m + 1:], v[:, m + 1:], s[:, m + 1:]))
        w = tv.weights(hh, s)
        assert np.all(w[:, m] == 0.0)
        z, A, inv, res, fwd, _ = solve_with_bounds(hh, tv.Lv(w, xx), DT, ff)
        new = xx + z
        hl = hh.astype(LD)
        per = U * (tf.C_BR_F * res + tf.C_LV_F * tv.Lv_abs(w, xx) + hl * np.abs(new))
        for part in (slice(0, m + 1), slice(m + 1, n)):
            drift = np.abs((hl * new)[:, part].sum(axis=1) - (hl * xx)[:, part].sum(axis=1))
            assert np.all(drift <= per[:, part].sum(axis=1)), (sh2, part)
            worst = max(worst, float((drift / per[:, part].sum(axis=1)).max()))
        assert not np.array_equal(new, xx)
    print(f"content drift of a part / its bound: {worst:.3f}")


# ---- whole steps --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["forward", "reverse", "density"])
@pytest.mark.parametrize("meshname,Kc,partial", [("planar", 6, False), ("planar", 34, "floor"), ("tiny-4-4", 5, False)])
def test_uniform_field_is_the_scalar_bit_for_bit(meshname, Kc, partial, kind):
    """Every tracer with a field that equals its kappaV at every active interface (NaN below): the forward steps, X and D of the
    scalar twin -- the zero scalar of tracer 1 as an all-zero field included."""
    a = tf.reference(meshname, Kc, partial, ((("uniform",) * 3, None),) * 3, (0, 1, 2))
    b = tg.reference(meshname, Kc, "linear", partial, 3, 3, (0, 1, 2))
    assert a["steps"][0][0][0] is not None and np.isnan(a["steps"][0][0][0]).any() and a["twin"].tape[0]["fieldV"][1] is None
    for j in range(3):
        if kind == "forward":
            assert all(np.array_equal(x[1][j], y[1][j]) and np.array_equal(x[0][j], y[0][j]) for x, y in zip(a["forward"], b["forward"]))
            assert not np.array_equal(a["forward"][-1][1][j], a["fields"][j])
        elif kind == "reverse":
            assert np.array_equal(a["grad"][j], b["grad"][j])
        else:
            assert np.array_equal(a["D"][j], b["D"][j]) and a["D"][j].any()


@pytest.mark.parametrize("meshname,Kc,partial", [("planar", 6, False), ("planar", 6, "floor"), ("tiny-4-4", 5, False), ("planar", 34, "floor")])
def test_density_against_long_double(meshname, Kc, partial):
    """Three recorded steps -- field A, field B, then the scalar -- all three tracers flagged: every element of D within the counted
    bound, and the scalar view within their sum."""
    plan = (STEP, (("B", None, None), None), ((None, None, None), None))
    ref = tf.reference(meshname, Kc, partial, plan, (0, 1, 2))
    adj = tf.VfieldAdjointTwin(ref["twin"])
    assert ref["twin"].tape[0]["fieldV"][0] is not None and ref["twin"].tape[2]["fieldV"][0] is None
    for j, D in ref["D"].items():
        Dl, B = tf.density_ld_field(adj, ref["twin"].tape, ref["X"], j)
        err = np.abs(D.astype(LD) - Dl)
        assert np.all(err <= B), (j, float((err - B).max()))
        s, sl = tk.host_sum(D.ravel()), Dl.sum()
        print(f"{meshname} K = {Kc} {partial} tracer {j}: max |D - D_ld| = {float(err.max()):.3e}, worst element at "
              f"{float((err / np.where(B > 0, B, 1)).max()):.3f} of its bound; scalar {s:.15e} against {float(sl):.15e}")
        assert abs(LD(s) - sl) <= B.sum() + U * abs(sl)
        assert np.abs(Dl).sum() > 1e3 * B.sum()
        assert not D[np.arange(Kc)[None, :] >= (ref["nlev"] - 1)[:, None]].any() and np.isfinite(D).all()


def test_all_zero_field_keeps_every_bit():
    """Tracer 0 with an all-zero field (NaN below) and a nonzero scalar that is not read, -0.0 among its values: the step leaves the bits
    of the run without the term, signs included; X likewise; the density is the derivative at zero."""
    plan = ((("zero", None, None), None),) * 2
    ref = tf.reference("planar", 6, "floor", plan, (0,))
    twin = ref["twin"]
    assert twin.tape[0]["fieldV"][0] is None and twin.tape[0]["kappaV"][0] == 0.0 and ref["steps"][0][1][0] != 0.0
    off = tg.reference("planar", 6, "linear", "floor", 3, ((tuple([0.0] + ref["steps"][0][1][1:]), None),) * 2, (0,))
    for a, b in zip(ref["forward"], off["forward"]):
        assert all(np.array_equal(a[1][j], b[1][j]) for j in range(3))
    assert np.array_equal(ref["grad"][0], off["grad"][0]) and np.array_equal(ref["D"][0], off["D"][0]) and ref["D"][0].any()
    # bit for bit means signs too: -0.0 == 0.0 under array_equal, so compare the words, and let a column of -0.0 pass an off field
    for a, b in zip(ref["forward"], off["forward"]):
        assert np.array_equal(a[1][0].view(np.uint64), b[1][0].view(np.uint64))
    nlev = ref["nlev"]
    x = np.random.default_rng(2).uniform(-1, 1, (len(nlev), 6))
    x[::3] = -0.0
    zero = np.where(np.arange(6)[None, :] >= (nlev - 1)[:, None], 9.0, 0.0)      # anything in the never-read entries
    assert not tf.field_on(zero, nlev) and not tf.field_on(-zero * 0.0, nlev) and tf.field_on(np.where(zero == 0.0, 1e-300, zero), nlev)
    ran = x + tv.solve(np.zeros((len(x), 5)), x * 0 + 7.0, np.zeros_like(x))      # what running the recipe with w == 0 would do
    assert np.signbit(x[0]).all() and not np.signbit(ran[0]).any()                # ... it loses the sign: hence the skip, not a solve


def test_the_twins_scan_of_a_field():
    """The twin's own restatement of the upload's host scan (check_field, field_on; the library's refusals are
    tests/test_gpu_tracer_vfield.py::test_interface): a negative, NaN or infinite value at an active interface fails it; the never-read
    entries are not inspected; -0.0 is a zero."""
    nlev = np.array([0, 1, 2, 4, 6])
    ok = np.full((5, 6), 2.0)
    assert tf.check_field(ok, nlev)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        f = ok.copy()
        f[3, 2] = bad                                     # the last active interface of a column of depth 4
        assert not tf.check_field(f, nlev)
        f = ok.copy()
        f[3, 3] = f[4, 5] = f[0, 0] = f[1, 0] = f[2, 1] = bad
        assert tf.check_field(f, nlev)
    assert tf.check_field(-0.0 * ok, nlev) and not tf.field_on(-0.0 * ok, nlev)


# ---- D[k,c] against differences in a single field entry ---------------------------------------------------------------------------
def J_of(ref, j, fields):
    """J = <X_j, phi_N,j> with the vertical pass of record n solved in long double for the field fields[n] ((nCells, K), or None: no
    pass); the RK4 part is the twin's replay in doubles (test_tracer_vgrad_twin.J_of)."""
    twin = ref["twin"]
    nlev = twin.nlev(ref["X"][j].shape[1])
    phi, new = ref["fields"][j], None
    for n, rec in enumerate(twin.tape):
        star = twin.replay(rec, j, np.asarray(phi, dtype=np.float64))[1]
        new = star.astype(LD) if fields[n] is None else tg.forward_ld_kfield(rec["hn"], star, nlev, rec["dt"], fields[n])
        phi = new
    return (ref["X"][j].astype(LD) * new).sum()


def eps_J(ref, meshname, j):
    """test_tracer_vgrad_twin.eps_J: nsteps (C_STEP_B + 1) 2^-53 sum |X| W."""
    twin, mesh = ref["twin"], tc.get_mesh(meshname)
    W = np.abs(ref["fields"][j]).astype(LD)
    for rec in twin.tape:
        W = tb.forward_magnitude(mesh, twin.mlt, rec, W, rec["kappa"][j], rec["kappa4"][j])
        W = np.repeat(W.max(axis=1)[:, None], W.shape[1], axis=1)
    return len(twin.tape) * (tb.C_STEP_B + 1) * U * (np.abs(ref["X"][j]).astype(LD) * W).sum()


def decay(ref, meshname, j, direction, grad, bound, d0, order, label):
    """test_tracer_vgrad_twin.decay's acceptance rule along `direction` ((nCells, K), added to the field of every step; one entry 1.0 and
    the rest 0.0 for a single entry of the field): differences at d0, d0 / 2,
    d0 / 4; central (order 2: the discrepancy falls by 3 .. 5 per halving) or one-sided (order 1: by 1.5 .. 2.5), unless the smaller
    discrepancy is at the floor bound + 2 eps_J / delta; the decay must be seen at least once."""
    base = [np.nan_to_num(f, nan=0.0) for f, _, _ in ((s[0][j], 0, 0) for s in ref["steps"])]
    eJ = eps_J(ref, meshname, j)

    def moved(d):
        return [b + d * direction for b in base]
    J0 = J_of(ref, j, base) if order == 1 else None
    disc = []
    for i in range(3):
        d = d0 / 2 ** i
        up = J_of(ref, j, moved(d))
        fd = (up - J0) / LD(d) if order == 1 else (up - J_of(ref, j, moved(-d))) / (2 * LD(d))
        disc.append((abs(fd - LD(grad)), bound + 2 * eJ / LD(d)))
    ratios = [float(disc[i][0] / disc[i + 1][0]) for i in range(2)]
    lo, hi = (3.0, 5.0) if order == 2 else (1.5, 2.5)
    print(f"{label}: gradient {float(grad):.6e}, discrepancies {[f'{float(x[0]):.3e}' for x in disc]}, ratios "
          f"{[f'{r:.3f}' for r in ratios]}, floors {[f'{float(x[1]):.3e}' for x in disc]}")
    for i in range(2):
        assert lo <= ratios[i] <= hi or disc[i + 1][0] <= disc[i + 1][1]
    assert lo <= ratios[0] <= hi
    assert disc[2][0] < 0.05 * abs(grad)


def unit(D, c, k):
    e = np.zeros(D.shape)
    e[c, k] = 1.0
    return e


@pytest.mark.parametrize("meshname,Kc", [("planar", 6), ("tiny-4-4", 5)])
def test_single_entries_against_differences(meshname, Kc):
    """Field A in all three steps.  Entries (c, k) at the top, in the middle and at the last active interface, central with delta from
    f[c,k] / 8; the exact zeros (0, 0) and (1, 2) one-sided from 1 / 4096 of the field's scale, as the existing test does at zero."""
    ref = tf.reference(meshname, Kc, False, (STEP,) * 3, (0,))
    f = ref["steps"][0][0][0]
    adj = tf.VfieldAdjointTwin(ref["twin"])
    _, B = tf.density_ld_field(adj, ref["twin"].tape, ref["X"], 0)
    D = ref["D"][0]
    scale = tv.kappavs(meshname, Kc, 3)[0]
    for c, k in ((2, 0), (4, 2), (9, Kc - 2), (11, 1)):
        assert f[c, k] > 0.0
        decay(ref, meshname, 0, unit(D, c, k), D[c, k], B[c, k], f[c, k] / 8, 2, f"{meshname} central D[{k},{c}]")
    for c, k in ((0, 0), (1, 2)):
        assert f[c, k] == 0.0 and D[c, k] != 0.0
        decay(ref, meshname, 0, unit(D, c, k), D[c, k], B[c, k], scale / 4096, 1, f"{meshname} one-sided at f = 0 D[{k},{c}]")


def test_scalar_view_is_the_derivative_along_the_all_ones_field():
    """sum D against central differences of J with every entry of the field of every step moved by delta.  The field holds exact zeros
    and values down to zero, and J is rational in the field: about f = 0 its nearest poles are where a row of A loses its diagonal,
    h + 4 w = 0 at the earliest (an interior row has two neighbours, each weight enters two rows), w = -h / 4, f = -hm^2 / (4 dt) =
    -(kappavs' first value / 30) / 4.  delta starts at an eighth of that radius, so f - delta < 0 at the zeros stays well inside."""
    meshname, Kc = "tiny-4-4", 5
    ref = tf.reference(meshname, Kc, False, (STEP,) * 3, (0,))
    adj = tf.VfieldAdjointTwin(ref["twin"])
    _, B = tf.density_ld_field(adj, ref["twin"].tape, ref["X"], 0)
    grad = tk.host_sum(ref["D"][0].ravel())
    live = np.arange(Kc)[None, :] < (ref["nlev"] - 1)[:, None]
    d0 = tv.kappavs(meshname, Kc, 3)[0] / tv.VFACT9[0] / 4 / 8
    decay(ref, meshname, 0, live.astype(np.float64), grad, B.sum() + U * abs(grad), d0, 2, f"{meshname} all-ones")


# ---- the odd mesh -------------------------------------------------------------------------------------------------------------------
def test_sheared_mesh_is_a_closed_hex_mesh_with_an_odd_cell_count():
    """Every cell has six distinct neighbours, every slot's edge joins the cell and that neighbour, every vertex its three mutually
    adjacent cells; the staggered mesh is what it was; the twin conserves the unit tracer and the content on it."""
    from moka_hip import meshgen as mg
    name = tf.sheared_mesh(7, 5)
    m = tc.get_mesh(name)
    assert m.nCells == 35 and m.nEdges == 105 and m.nVertices == 70
    coe, eoc, coc, cov, eov, voe = (np.asarray(a) - 1 for a in (m.cellsOnEdge, m.edgesOnCell, m.cellsOnCell, m.cellsOnVertex, m.edgesOnVertex,
                                                                 m.verticesOnEdge))
    for c in range(m.nCells):
        assert len(set(coc[c])) == 6 and c not in coc[c]
        assert all(set(coe[eoc[c, i]]) == {c, coc[c, i]} for i in range(6))
    for v in range(m.nVertices):
        assert len(set(cov[v])) == 3 and all(set(coe[e]) <= set(cov[v]) and v in voe[e] for e in eov[v])
    with pytest.raises(ValueError):
        mg.planar_hex_mesh(7, 5, 1000.0)
    a, b = mg.planar_hex_mesh(6, 4, 1000.0, f0=1e-4), mg.planar_hex_mesh(6, 4, 1000.0, f0=1e-4, sheared=False)
    assert np.array_equal(a.cellsOnCell, b.cellsOnCell) and np.array_equal(a.xCell, b.xCell)
    assert not np.array_equal(a.cellsOnCell, mg.planar_hex_mesh(6, 4, 1000.0, sheared=True).cellsOnCell)
    ref = tf.reference(name, 5, False, (((None, "A", "B"), None),) * 3, (1, 2))
    assert ref["twin"].tape[0]["fieldV"][1] is not None and ref["D"][1].any() and ref["D"][2].any()
    area = np.asarray(m.areaCell)[:, None]
    for j in range(3):
        before = (area * ref["forward"][0][3] * ref["forward"][0][1][j]).sum()
        after = (area * ref["forward"][2][3] * ref["forward"][2][1][j]).sum()
        assert abs(after - before) <= 1e-12 * abs(before)                # transport and vertical mixing both conserve the content
