"""The MacCormack step (scheme 2) written out in Python on the oracle's exported operators, through
oracle_lib: the yardstick of the scheme, independent of the C++ host solver.  One step is the reference CPU solver's
advanceMacCormack (BimocqSolver.cpp:282-364): one CFL bound, MacCormack advection of rho, T, u, v, w over -dt / +dt
through the step's old velocity with the limiter over dt, the legacy emitters, buoyancy, 20 diffusion sweeps per
component when the viscosity is not 0, the Jacobi projection.  Single domain, no obstacles, no shaped sources.
Test infrastructure."""
import numpy as np

import fields as F
from oracle_lib import fp, lib

f32 = np.float32
STAGGERS = {"rho": (0, 0, 0), "T": (0, 0, 0), "u": (1, 0, 0), "v": (0, 1, 0), "w": (0, 0, 1)}


class MacCormackRef:
    def __init__(self, ni, nj, nk, L=1.0, viscosity=0.0):
        self.l = lib()
        self.dims = (ni, nj, nk)
        self.h = f32(L) / f32(ni)
        self.nu = f32(viscosity)
        n, nu, nv, nw = F.sizes(ni, nj, nk)
        self.f = {"rho": np.zeros(n, f32), "T": np.zeros(n, f32), "u": np.zeros(nu, f32), "v": np.zeros(nv, f32),
                  "w": np.zeros(nw, f32)}
        self.emitters, self.alpha, self.beta = [], f32(0), f32(0)
        self.iters, self.halfrdx = 100, f32(0.5)
        self.cfldt = f32(0)
        self.limited = {"scalar": 0, "velocity": 0}     # values the limiter replaced so far

    def set_smoke(self, drop, rise, emitters):
        """emitters: (cx, cy, cz, radius, density, temperature, emiter, emit_frames)"""
        self.alpha, self.beta, self.emitters = f32(drop), f32(rise), list(emitters)

    def set_projection(self, iters, halfrdx):
        self.iters, self.halfrdx = iters, f32(halfrdx)

    def field(self, name):
        return self.f[name]

    def _maccormack(self, name, cfldt, dt):
        """the advected field `name` (a new array); the velocity the traces run through is the step's old one"""
        ni, nj, nk = self.dims
        dx, dy, dz = STAGGERS[name]
        u, v, w = (fp(self.f[c]) for c in "uvw")
        field = self.f[name]
        first, back = np.zeros_like(field), np.zeros_like(field)
        self.l.orc_semilag(fp(first), fp(field), u, v, w, dx, dy, dz, self.h, ni, nj, nk, cfldt, -dt)
        self.l.orc_semilag(fp(back), fp(first), u, v, w, dx, dy, dz, self.h, ni, nj, nk, cfldt, dt)
        self.l.orc_add(fp(first), fp(back), -0.5, first.size)
        self.l.orc_add(fp(first), fp(field), 0.5, first.size)
        before = first.copy()
        self.l.orc_clamp_extrema(fp(field), fp(first), u, v, w, ni + dx, nj + dy, nk + dz, dx, dy, dz,
                                 0.5 * dx, 0.5 * dy, 0.5 * dz, self.h, dt)
        changed = int(np.count_nonzero(before.view(np.uint32) != first.view(np.uint32)))
        self.limited["scalar" if name in ("rho", "T") else "velocity"] += changed
        return first

    def advance(self, frame, dt):
        ni, nj, nk = self.dims
        dt = f32(dt)
        f = self.f
        vmax = f32(self.l.orc_max_abs3(fp(f["u"]), fp(f["v"]), fp(f["w"]), ni, nj, nk))
        self.cfldt = cfldt = self.h / vmax
        new = {name: self._maccormack(name, cfldt, dt) for name in ("rho", "T", "u", "v", "w")}
        f.update(new)
        for cx, cy, cz, radius, density, temperature, emiter, frames in self.emitters:
            if frame < frames:
                self.l.orc_emit_smoke(fp(f["u"]), fp(f["v"]), fp(f["w"]), fp(f["rho"]), fp(f["T"]), self.h, ni, nj, nk,
                                      cx, cy, cz, radius, density, temperature, emiter)
        self.l.orc_add_buoyancy(fp(f["v"]), fp(f["rho"]), fp(f["T"]), ni, nj, nk, self.alpha, self.beta, dt)
        if self.nu != 0:
            coef = self.nu * (dt / (self.h * self.h))
            for name, (dx, dy, dz) in (("u", (1, 0, 0)), ("v", (0, 1, 0)), ("w", (0, 0, 1))):
                t0, t1 = np.zeros_like(f[name]), np.zeros_like(f[name])
                self.l.orc_diffuse_field(fp(f[name]), fp(t0), fp(t1), ni + dx, nj + dy, nk + dz, 20, coef)
        n = ni * nj * nk
        div, p, p_temp, debug = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(4096, f32)
        self.l.orc_projection_jacobi(fp(f["u"]), fp(f["v"]), fp(f["w"]), fp(div), fp(p), fp(p_temp), fp(debug), ni, nj, nk,
                                     self.iters, self.halfrdx, -1.0, f32(1.0 / 6.0))
