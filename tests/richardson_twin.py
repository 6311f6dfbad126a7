"""Numpy twin of the Richardson-number closure of the two vertical passes (moka_set_richardson_mixing; csrc/vmix_closure.hip), a
long-double restatement with a counted bound, the twin of a whole step with the closure on, and the cases the tests share.

Recipe (include/moka_hip.h), host layout: u (nEdges, K), h and b (nCells, K), column k of F (nEdges, K) and G (nCells, K) the interface
between levels k and k+1.  Every operation rounded once.  EPS = 1e-20.
  edge e, n = min(maxLevelEdgeTop[e], K), (c1, c2) = cellsOnEdge[e], k = 0 .. n-2:
    hE[k] = 0.5 * (h[c1,k] + h[c2,k]);  hm = 0.5 * (hE[k] + hE[k+1])
    db = 0.5 * ((b[c1,k] - b[c1,k+1]) + (b[c2,k] - b[c2,k+1]));  du = u[e,k] - u[e,k+1]
    Ri = (db * hm) / (du * du + EPS)
    Ri > 0:  t = 1.0 + alpha * Ri;  m = nu0 / (t * t);  F = nuB + m          else:  F = nuB + nu0 (+ conv if db < 0)
  cell c, n = nLev[c] (the largest n_e of its edges), k = 0 .. n-2:
    hm = 0.5 * (h[c,k] + h[c,k+1]);  db = b[c,k] - b[c,k+1]
    acc = 0.0;  slots i of edgesOnCell[c] in order, e' the edge:  if min(maxLevelEdgeTop[e'], K) > k+1:
        du = u[e',k] - u[e',k+1];  acc = acc + (kc[e'] * du) * du            kc = (0.25 * dcEdge) * dvEdge
    S2 = 2.0 * (acc * invArea[c]);  Ri = (db * hm) / (S2 + EPS)              invArea = 1 / areaCell
    Ri > 0:  t = 1.0 + alpha * Ri;  m = nu0 / (t * t);  G = kB + (nuB + m) / t      else:  G = kB + (nuB + nu0) (+ conv if db < 0)
Rows k >= n-1 are never written (0.0 here, as from allocation on the device).  A slot that fails the depth test contributes no operand
(`cell_field` puts 0.0 in its place before any arithmetic; `cell_field_wrong` is the deliberate mistake that reads it); u at k >= n_e
and b, h at k >= nLev[c] are never read.

Long double (`edge_ld`, `cell_ld`).  The two differences du and db are the recipe's doubles -- every cancellation of the recipe
happens in them -- and everything after them is formed in long double from the inputs: hm from the two or four thicknesses, S2 with
dcEdge dvEdge / 4 / areaCell, Ri, and F = nuB + nu0 / (1 + alpha Ri)^2, G = kB + (nuB + nu0 / (1 + alpha Ri)^2) / (1 + alpha Ri) where
db > 0, the constants (+ conv where db < 0) elsewhere.  Round-off count of the twin against that, to first order, in units of 2^-53 of
the result -- every sum below has non-negative terms (h > 0, du^2 >= 0, EPS > 0, db > 0 on this branch, all parameters >= 0), so a
sum's relative error is at most the larger one of its terms plus its own rounding, and nothing cancels:
  edge:  hE[k], hE[k+1]: one addition each (the product with 0.5 is exact): 1;  hm: 2;  db * hm: 3;  du * du: 1, + EPS: 2;
         Ri: 3 + 2 + 1 = 6;  alpha * Ri: 7;  t: 8;  t * t: 17;  m: 18;  F: 19.                                  C_F = 19 + 1
  cell:  hm: 1;  db * hm: 2;  a term (kc du) du: kc 1 (0.25 * dcEdge is exact), two products: 3;  acc over m = maxEdges slots: the
         first addition, to 0.0, is exact: 3 + (m - 1);  invArea and the product with it: m + 4 (the product with 2.0 is exact);
         + EPS: m + 5;  Ri: 2 + (m + 5) + 1 = m + 8;  alpha * Ri: m + 9;  t: m + 10;  t * t: 2 m + 21;  m: 2 m + 22;  nuB + m: 2 m + 23;
         the division by t: 3 m + 34;  G: 3 m + 35.                                                          C_G = 3 m + 35 + 1
  the other branch is one or two additions of constants.  The last + 1 of both counts stands for every second-order term ((1 + u)^57
  - 1 < 57 u (1 + 2^-46)) and for the long-double model's own roundings, some dozens of 2^-64.
Nothing here is measured from the twin or the device."""
import numpy as np

import momentum_vmix_twin as mv
import poison_cases as pc
import quadratic_drag_twin as qd
import tracer_cases as tc
import tracer_vfield_twin as tf
import tracer_vmix_twin as tv
from del4_twin import TwinState

LD = tv.LD
U53 = tv.U53
EPS = 1e-20
C_F = 19 + 1


def c_g(mesh):
    return 3 * int(np.asarray(mesh.edgesOnCell).shape[1]) + 35 + 1


class Params:
    """The five parameters of the closure (MPAS-Ocean's defaults), the buoyancy tracer and the set (None: every tracer)."""

    def __init__(self, buoyancy=1, nu0=0.005, alpha=5.0, nuB=1e-4, kB=1e-5, conv=1.0, tracers=None):
        self.buoyancy, self.tracers = int(buoyancy), (None if tracers is None else sorted(int(j) for j in tracers))
        self.nu0, self.alpha, self.nuB, self.kB, self.conv = (np.float64(v) for v in (nu0, alpha, nuB, kB, conv))

    def key(self):
        return (self.buoyancy, None if self.tracers is None else tuple(self.tracers)) + tuple(float(v) for v in (self.nu0, self.alpha, self.nuB, self.kB, self.conv))

    def in_set(self, j):
        return self.tracers is None or j in self.tracers

    def kwargs(self):
        """The keyword arguments of moka_hip.set_richardson_mixing."""
        return dict(nu0=float(self.nu0), alpha=float(self.alpha), background_viscosity=float(self.nuB), background_diffusivity=float(self.kB),
                    convective=float(self.conv), tracers=self.tracers)


# ---- the recipe -----------------------------------------------------------------------------------------------------------------------
def depths(mlt, nE, K):
    return np.minimum(np.asarray(mlt, dtype=np.int64) * np.ones(nE, dtype=np.int64), K)


def cell_depth(mesh, nn):
    """nLev[c]: the largest n_e over the cell's slots."""
    eoc, cnt, _, _ = qd._stencil(mesh)
    valid = (np.arange(eoc.shape[1])[None, :] < cnt[:, None]) & (eoc >= 0)
    return np.where(valid, nn[np.where(valid, eoc, 0)], 0).max(axis=1)


def coefficient(ri, db, P, cell):
    pos = ri > 0.0
    t = 1.0 + P.alpha * np.where(pos, ri, 0.0)
    m = P.nu0 / (t * t)
    stable = P.kB + (P.nuB + m) / t if cell else P.nuB + m
    base = P.kB + (P.nuB + P.nu0) if cell else P.nuB + P.nu0
    return np.where(pos, stable, np.where(db < 0.0, base + P.conv, base))


def _pairs(a, rows, live):
    """(a[rows, k], a[rows, k+1]) over the interfaces, 1.0 where the interface is not live (what lies there is never read)."""
    return np.where(live, a[rows, :-1], 1.0), np.where(live, a[rows, 1:], 1.0)


def edge_parts(u, h, b, mlt, c1, c2):
    """(live, (h1k, h1n, h2k, h2n), db, du) of the edge recipe, (nEdges, K-1) each: the operands and the two differences."""
    nE, K = u.shape
    live = np.arange(K - 1)[None, :] < (depths(mlt, nE, K) - 1)[:, None]
    e = np.arange(nE)
    h1k, h1n = _pairs(h, c1, live)
    h2k, h2n = _pairs(h, c2, live)
    b1k, b1n = _pairs(b, c1, live)
    b2k, b2n = _pairs(b, c2, live)
    uk, un = _pairs(u, e, live)
    db = 0.5 * ((b1k - b1n) + (b2k - b2n))
    return live, (h1k, h1n, h2k, h2n), db, uk - un


def edge_field(u, h, b, mlt, c1, c2, P):
    """(F, RiEdge), (nEdges, K) each, 0.0 in the rows that are never written."""
    nE, K = u.shape
    F, Ri = np.zeros((nE, K)), np.zeros((nE, K))
    if K < 2:
        return F, Ri
    live, (h1k, h1n, h2k, h2n), db, du = edge_parts(u, h, b, mlt, c1, c2)
    hm = 0.5 * (0.5 * (h1k + h2k) + 0.5 * (h1n + h2n))
    ri = (db * hm) / (du * du + EPS)
    F[:, :-1] = np.where(live, coefficient(ri, db, P, False), 0.0)
    Ri[:, :-1] = np.where(live, ri, 0.0)
    return F, Ri


def cell_parts(u, h, b, mlt, mesh, depth_test=True):
    """(live, (hk, hn), db, [(ok, kc, du) per slot], invArea) of the cell recipe."""
    nC, K = h.shape
    nn = depths(mlt, u.shape[0], K)
    eoc, cnt, kc, inv = qd._stencil(mesh)
    live = np.arange(K - 1)[None, :] < (cell_depth(mesh, nn) - 1)[:, None]
    c = np.arange(nC)
    hk, hn = _pairs(h, c, live)
    bk, bn = _pairs(b, c, live)
    kk = np.arange(K - 1)[None, :]
    slots = []
    for i in range(eoc.shape[1]):
        valid = (i < cnt) & (eoc[:, i] >= 0)
        ep = np.where(valid, eoc[:, i], 0)
        ok = valid[:, None] & live & ((nn[ep][:, None] > kk + 1) if depth_test else True)
        xk = np.where(ok, u[ep, :-1], 0.0)                # a slot that fails the test contributes no operand at all
        xn = np.where(ok, u[ep, 1:], 0.0)
        slots.append((ok, kc[ep][:, None], xk - xn))
    return live, (hk, hn), bk - bn, slots, inv[:, None]


def _cell_field(u, h, b, mlt, mesh, P, depth_test):
    nC, K = h.shape
    G, Ri = np.zeros((nC, K)), np.zeros((nC, K))
    if K < 2:
        return G, Ri
    live, (hk, hn), db, slots, inv = cell_parts(u, h, b, mlt, mesh, depth_test)
    hm = 0.5 * (hk + hn)
    acc = np.zeros((nC, K - 1))
    for ok, kc, du in slots:
        acc = np.where(ok, acc + (kc * du) * du, acc)
    ri = (db * hm) / (2.0 * (acc * inv) + EPS)
    G[:, :-1] = np.where(live, coefficient(ri, db, P, True), 0.0)
    Ri[:, :-1] = np.where(live, ri, 0.0)
    return G, Ri


def cell_field(u, h, b, mlt, mesh, P):
    """(G, RiCell), (nCells, K) each, 0.0 in the rows that are never written."""
    return _cell_field(u, h, b, mlt, mesh, P, True)


def cell_field_wrong(u, h, b, mlt, mesh, P):
    """The deliberate mistake: the depth test of the slots is dropped, u[e',k] and u[e',k+1] are read at every listed edge."""
    return _cell_field(u, h, b, mlt, mesh, P, False)


# ---- long double ------------------------------------------------------------------------------------------------------------------
def _coefficient_ld(ri, db, P, cell):
    nu0, al, nuB, kB, conv = (LD(float(v)) for v in (P.nu0, P.alpha, P.nuB, P.kB, P.conv))
    t = 1 + al * np.where(db > 0, ri, 0)
    stable = kB + (nuB + nu0 / (t * t)) / t if cell else nuB + nu0 / (t * t)
    base = kB + nuB + nu0 if cell else nuB + nu0
    return np.where(db > 0, stable, np.where(db < 0, base + conv, base))


def edge_ld(u, h, b, mlt, c1, c2, P):
    """(F in long double on the live interfaces, live), (nEdges, K-1)."""
    live, hs, db, du = edge_parts(u, h, b, mlt, c1, c2)
    hm = sum(x.astype(LD) for x in hs) / 4
    ri = db.astype(LD) * hm / (du.astype(LD) ** 2 + LD(EPS))
    return _coefficient_ld(ri, db, P, False), live


def cell_ld(u, h, b, mlt, mesh, P):
    """(G in long double on the live interfaces, live), (nCells, K-1).  S2 is summed over the slots that pass, in long double, with
    the metric factors formed in long double."""
    live, (hk, hn), db, slots, _ = cell_parts(u, h, b, mlt, mesh)
    eoc, cnt, _, _ = qd._stencil(mesh)
    w = np.asarray(mesh.dcEdge).astype(LD) * np.asarray(mesh.dvEdge).astype(LD) / 4
    s2 = np.zeros(hk.shape, dtype=LD)
    for i, (ok, _, du) in enumerate(slots):
        ep = np.where((i < cnt) & (eoc[:, i] >= 0), eoc[:, i], 0)
        s2 += np.where(ok, w[ep][:, None] * du.astype(LD) ** 2, 0)
    s2 = 2 * s2 / np.asarray(mesh.areaCell).astype(LD)[:, None]
    hm = (hk.astype(LD) + hn.astype(LD)) / 2
    ri = db.astype(LD) * hm / (s2 + LD(EPS))
    return _coefficient_ld(ri, db, P, True), live


def census(ri, db_sign_source, live):
    """Shares of the three branches among the live interfaces: (Ri > 0, Ri == 0 with db == 0, db < 0)."""
    n = max(int(live.sum()), 1)
    return (float((live & (ri > 0)).sum()) / n, float((live & (db_sign_source == 0)).sum()) / n, float((live & (db_sign_source < 0)).sum()) / n)


# ---- the step -------------------------------------------------------------------------------------------------------------------------
class RichardsonTwin:
    """The twin chain's step with the closure: the transport step of the tracer chain (`tw`: a tracer_vfield_twin.VfieldTwin) without
    its vertical pass, the closure, the field form of the tracer pass with G for the tracers of the set (their own field or scalar for
    the others), the field form of the momentum pass with F.  `params` = None: the closure is off and the step is that of the chain
    (QuadraticDragTwin over the VfieldTwin) with the set-aside coefficients, which live where they always did: tw.kappaV, tw.fieldV,
    and nu, drag, tau, cd, fld here.  F, G: what the last step computed (zeros when it ran without the closure or launched nothing)."""

    def __init__(self, tw, nu=0.0, drag=0.0, tau=None, cd=0.0, fld=None, params=None):
        self.tw, self.params = tw, params
        self.mq = qd.QuadraticDragTwin(mv.MomentumVmixTwin(tw, nu, drag, tau), cd, fld=fld)
        self.mesh = tw.om.mesh
        self.F, self.G = None, None

    @property
    def mlt(self):
        return self.mq.mt.mlt

    def fields(self, u, h, b):
        m = self.mq.mt
        return edge_field(u, h, b, m.mlt, m.c1, m.c2, self.params)[0], cell_field(u, h, b, m.mlt, self.mesh, self.params)[0]

    def numbers(self, u, h, b):
        """(RiEdge, RiCell) of a state, as moka_richardson_diagnose forms them."""
        m = self.mq.mt
        return edge_field(u, h, b, m.mlt, m.c1, m.c2, self.params)[1], cell_field(u, h, b, m.mlt, self.mesh, self.params)[1]

    def step_rk4(self, st, phis, dt):
        """st: a del4_twin.TwinState; phis = [previous, current] tracer lists."""
        nE, K = st.u[1].shape
        self.F, self.G = np.zeros((nE, K)), np.zeros(st.h[1].shape)
        if self.params is None:
            self.mq.step_rk4(st, phis, dt)
            return
        assert dt >= 0.0, "the device refuses dt < 0 while the closure is on"
        tw, P, m = self.tw, self.params, self.mq.mt
        kv, fv = tw.kappaV, tw.fieldV
        tw.kappaV, tw.fieldV = [], []
        try:
            tw.step_rk4(st, phis, dt)                      # the transport step alone: stage 4 and the tracers' stage 4
        finally:
            tw.kappaV, tw.fieldV = kv, fv
        if K < 2 or dt == 0.0:                             # nothing of the closure is launched; the momentum pass is the one it was
            st.u[1] = self.mq.mix(st.u[1], st.h[1], dt)
            return
        nlev = tw.nlev(K)
        self.F, self.G = self.fields(st.u[1], st.h[1], phis[1][P.buoyancy])
        for j in range(len(phis[1])):
            own = tw.field_of(j)
            if P.in_set(j):
                phis[1][j] = tf.apply_field(st.h[1], phis[1][j], nlev, dt, self.G)
            elif own is not None:
                if tf.field_on(own, nlev):
                    phis[1][j] = tf.apply_field(st.h[1], phis[1][j], nlev, dt, own)
            elif tw.kappaV_of(j) != 0.0:
                phis[1][j] = tv.apply(st.h[1], phis[1][j], nlev, np.float64(dt) * np.float64(tw.kappaV_of(j)))
        st.u[1], sp = qd.apply(st.u[1], st.h[1], m.mlt, m.c1, m.c2, dt, 0.0, m.drag, m.tau, self.mq.cd, self.mesh, self.mq.speed, self.F)
        if self.mq.cd != 0.0:
            self.mq.sp = sp

    def step_s13(self, st, dt, nl=None):
        """As the other momentum twins have it -- for the closure off only: the 13-stream form never carries tracers
        (mk::rk13_usable), and the closure needs one."""
        assert self.params is None
        self.mq.step_s13(st, dt, nl)


def richardson_twin(meshname, K, mode="linear", mlt=None, **kw):
    return RichardsonTwin(tf.vfield_twin(meshname, K, mode, False, mlt), **kw)


# ---- shared cases -------------------------------------------------------------------------------------------------------------------
NT = 3
JB = 1
_CASES = {}


def mask_of(meshname, K, mask):
    """None (full columns), "partial" (tc.partial_mlt) or "basin" (poison_cases.mask_of), as an array of nEdges depths."""
    mesh = tc.get_mesh(meshname)
    if not mask:
        return np.full(mesh.nEdges, K, dtype=np.int32)
    return np.asarray(pc.mask_of(meshname, K) if mask == "basin" else tc.partial_mlt(mesh, K))


def buoyancy(meshname, K, alpha=5.0, seed=5):
    """A stable linear profile plus noise, scaled so that over tc.state_of's shear (u uniform in [-1, 1]: the median of du^2 is
    (2 - sqrt 2)^2 = 0.343) and hm = 1000 / K the median Ri of an ordinary interface is near 1 / alpha; built downwards interface by
    interface so that the kind of each is exact: an ordinary one has b[k+1] = b[k] - step, step in [0.4, 1.6] of the mean; a copy has
    b[k+1] = b[k] exactly (db == 0); an inversion has b[k+1] = b[k] + step / 2 (db < 0).  Copies: the interfaces k % 5 == 2 of every
    cell, and interface 0 of the first eighth of the cells (consecutive cells are neighbours: many edges have both cells there, so the
    edge recipe meets db == 0 at K = 2 too).  Inversions: k % 5 == 4 of every cell, interface 0 of the second eighth, and where
    (c + 3 k) % 11 == 0."""
    mesh = tc.get_mesh(meshname)
    nC = mesh.nCells
    rng = np.random.default_rng(seed + K)
    mean = (1.0 / alpha) * 0.343 / (1000.0 / max(K, 1))
    b = np.empty((nC, K))
    b[:, 0] = 0.02 + mean * rng.uniform(0.0, 1.0, nC)
    c = np.arange(nC)
    for k in range(K - 1):
        step = mean * rng.uniform(0.4, 1.6, nC)
        copy = np.full(nC, k % 5 == 2) | ((k == 0) & (c < nC // 8))
        inv = ~copy & (np.full(nC, k % 5 == 4) | ((k == 0) & (c >= nC // 8) & (c < nC // 4)) | ((c + 3 * k) % 11 == 0))
        b[:, k + 1] = np.where(copy, b[:, k], np.where(inv, b[:, k] + 0.5 * step, b[:, k] - step))
    return b


def case(meshname, K, mask=None, poison=None, mode="linear"):
    """The shared case: mesh, mlt, nlev, (ssh, u, h, rest) of tc.state_of, NT tracers -- the unit tracer, the buoyancy (index JB), one of
    tc.distinct_fields -- and Params().  poison: None; "strict": NaN in u at k >= n_e and in every tracer at k >= nLev[c], the levels
    the closure never reads (for the closure alone); "step": NaN on poison_cases' sets of the dycore `mode`, the levels no launch of a
    whole step reads."""
    key = (meshname, K, mask, poison, mode)
    if key not in _CASES:
        mesh = tc.get_mesh(meshname)
        mlt = mask_of(meshname, K, mask)
        nn = depths(mlt, mesh.nEdges, K)
        nlev = cell_depth(mesh, nn)
        ssh, u, h, rest = tc.state_of(meshname, K)
        f = [np.ones((mesh.nCells, K)), buoyancy(meshname, K), tc.distinct_fields(mesh, K, 3)[2]]
        if poison == "strict":
            u = np.where(np.arange(K)[None, :] >= nn[:, None], np.nan, u)
            f = [np.where(np.arange(K)[None, :] >= nlev[:, None], np.nan, a) for a in f]
        elif poison == "step":
            u = pc.put(u, pc.edge_poison(mesh, mlt, K, pc.RINGS[mode]), "nan")
            f = [pc.put(a, pc.cell_poison(mesh, mlt, K), "nan") for a in f]
        _CASES[key] = {"mesh": mesh, "mlt": mlt, "nn": nn, "nlev": nlev, "state": (ssh, u, h, rest), "fields": f, "params": Params(JB)}
    return _CASES[key]


def run(meshname, K, plan, mask=None, poison=None, mode="linear", settings=None, tag=""):
    """The twin's state after every step of `plan` = one Params (or None: the closure off) per step, over `case`; settings: a dict of
    nu, drag, tau, cd, fld, kappaV, fieldV -- the set-aside coefficients, fixed over the run -- and `tag` the name that tells one such dict from another.  Computed once and shared.  A list of
    (phis previous, phis current, u, h, ssh, F, G, RiEdge, RiCell); the last two are None for a step with the closure off."""
    settings = settings or {}
    key = ("run", meshname, K, tuple(p.key() if p is not None else None for p in plan), mask, poison, mode, tag)
    if key not in _CASES:
        cs = case(meshname, K, mask, poison, mode)
        tw = richardson_twin(meshname, K, mode, cs["mlt"], **{k: v for k, v in settings.items() if k in ("nu", "drag", "tau", "cd", "fld")})
        tw.tw.kappa, tw.tw.kappa4, tw.tw.source = [0.0] * NT, [0.0] * NT, [None] * NT
        tw.tw.kappaV, tw.tw.fieldV = list(settings.get("kappaV", [])), list(settings.get("fieldV", []))
        ssh, u, h, _ = cs["state"]
        st = TwinState(ssh, u, h)
        phis = [[a.copy() for a in cs["fields"]], [a.copy() for a in cs["fields"]]]
        out = []
        for P in plan:
            tw.params = P
            tw.step_rk4(st, phis, tc.dt_of(meshname))
            ri = tw.numbers(st.u[1], st.h[1], phis[1][P.buoyancy]) if P is not None else (None, None)
            out.append(([a.copy() for a in phis[0]], [a.copy() for a in phis[1]], st.u[1].copy(), st.h[1].copy(), st.ssh[1].copy(),
                        tw.F.copy(), tw.G.copy(), ri[0], ri[1]))
        _CASES[key] = out
    return _CASES[key]
