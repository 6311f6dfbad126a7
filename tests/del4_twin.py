"""Numpy twin of Del4 (biharmonic) momentum mixing on top of the oracle's nonlinear tendencies (moka_set_viscosity_del4).

L(u) is the Del2 bracket the library already applies (horizontal_momentum_mixing.jl:75-78), exactly 0 above maxLevelEdgeTop:
    L(u)[k,e] = (div(u)[k,c2] - div(u)[k,c1]) * (1/dcEdge) - (curl(u)[k,v2] - curl(u)[k,v1]) * (1/dvEdge)
with div / curl the oracle's own operators (OracleMesh.divergence_on_cell / curl_on_vertex, bit-identical to the preparation pass's
velocityDivCell / relativeVorticity).  The Del4 tendency is the nonlinear (+ Del2) tendency minus L(L(u)) * coef4, the last operation,
on the levels k < maxLevelEdgeTop.  The RK4 step restates oracle_step_rk4_nonlinear_del2's stage loop (same operations, same order)."""
import numpy as np

import oracle as orc


class TwinState:
    """Two time levels (index 0 = previous, 1 = current) of normalVelocity, layerThickness and ssh."""

    def __init__(self, ssh, u, h):
        self.ssh = [np.array(ssh, dtype=np.float64), np.array(ssh, dtype=np.float64)]
        self.u = [np.array(u, dtype=np.float64), np.array(u, dtype=np.float64)]
        self.h = [np.array(h, dtype=np.float64), np.array(h, dtype=np.float64)]
        self.tendU = self.tendH = None


class Del4Twin:
    def __init__(self, om: orc.OracleMesh, visc_del2: float = 0.0, visc_del4: float = 0.0, scaling=None):
        m, K = om.mesh, om.K
        self.om = om
        self.nl = orc.OracleNonlinear(om, visc_del2=visc_del2) if visc_del2 else orc.OracleNonlinear(om)
        self.c1, self.c2 = m.cellsOnEdge[:, 0] - 1, m.cellsOnEdge[:, 1] - 1
        self.v1, self.v2 = m.verticesOnEdge[:, 0] - 1, m.verticesOnEdge[:, 1] - 1
        self.invDc, self.invDv = (1.0 / m.dcEdge)[:, None], (1.0 / m.dvEdge)[:, None]
        self.mask = np.arange(K)[None, :] < om.arrays["maxLevelEdgeTop"][:, None]
        self.visc_del4 = float(visc_del4)
        # formed once in double, as the library forms it at set time (no multiply by 1 without a scaling array)
        self.coef4 = (self.visc_del4 * np.asarray(scaling, dtype=np.float64) if scaling is not None
                      else np.full(m.nEdges, self.visc_del4))[:, None]

    def bracket(self, div, curl):
        return (div[self.c2] - div[self.c1]) * self.invDc - (curl[self.v2] - curl[self.v1]) * self.invDv

    def L(self, u):
        return np.where(self.mask, self.bracket(self.om.divergence_on_cell(u), self.om.curl_on_vertex(u)), 0.0)

    def del4_bracket(self, u):
        """T = L(L(u)) on the active levels: the bracket before coef4 and the minus sign."""
        return self.L(self.L(u))

    def tendencies(self, u, h):
        tu, th, ssh, _ = self.nl.tendencies(u, h)
        if self.visc_del4 != 0.0:
            tu = np.where(self.mask, tu - self.del4_bracket(u) * self.coef4, tu)
        return tu, th, ssh

    def step_rk4(self, st: TwinState, dt):
        a = (dt / 2., dt / 2., dt)
        b = (dt / 6., dt / 3., dt / 3., dt / 6.)
        st.ssh[0], st.u[0], st.h[0] = st.ssh[1].copy(), st.u[1].copy(), st.h[1].copy()
        cu, ch = st.u[0], st.h[0]
        newU, newH = st.u[1].copy(), st.h[1].copy()
        pu, ph = st.u[1], st.h[1]
        for s in range(4):
            tu, th, _ = self.tendencies(pu, ph)
            if s < 3:
                pu, ph = cu + a[s] * tu, ch + a[s] * th
            newU, newH = newU + b[s] * tu, newH + b[s] * th
        st.tendU, st.tendH = tu, th
        st.u[1], st.h[1] = newU, newH
        st.ssh[1] = self.om.update_ssh(newH)
