"""Needle-shaped grids and the smallest accepted grids (no tests here): shapes, a cheap input generator, the far end of an
array, the non-vacuity condition, and one table of operator cases -- the oracle's reference and the call on an implementation of
include/bimocq_gpu.h -- shared by tests/test_needle_grids_cpu.py (oracle and CPU stand-in) and tests/test_gpu_needle_grids.py.

The needles put one index beyond what every other test reaches: x columns past 65536 (1025 x-blocks of 64), rows past 262144
(grid.y = 65540, a plane of 2.9 M elements), nk + 1 = 65535 planes (the largest grid.z the launchers accept).  A cross-section of
10 leaves the gather operators (interior 3 .. n - 4) four cells per axis; below 8 every output would be empty.

Outputs start as 7.0 everywhere on both sides; the bar is value equality (fields.same) over the whole array."""
import functools

import numpy as np

import fields as F
from host_entry_case import PREFILL, ptrs, stag
from oracle_lib import fp, lib as oracle

f32 = np.float32
LONG_X, LONG_Y, LONG_Z = (65560, 10, 10), (10, 262160, 10), (10, 10, 65534)
NEEDLES = [LONG_X, LONG_Y, LONG_Z]
# the same lengths on the thinnest cross-section the host solver takes (8): the step cases of the CPU file, whose cost is the oracle's
STEP_NEEDLES = [(65560, 8, 8), (8, 262160, 8), (8, 8, 65534)]
SMALL = [(1, 1, 1), (2, 3, 4), (7, 6, 5), (8, 8, 8), (9, 10, 8)]
H_POW2, H_TABLED = 0.125, float(f32(0.1))          # the structured power-of-two path; host-built tables / the generic path
SPACINGS = [H_POW2, H_TABLED]
FAR_FROM = {0: 65536, 1: 262144}                   # first index of the far end on LONG_X / LONG_Y
FAR_PLANES = 16                                    # LONG_Z: the last 16 planes
MIN_MOVED = 16                                     # non-vacuity: fixed in advance, not measured
ALPHA, BETA = -1.0, 1.0 / 6.0                      # the Jacobi coefficients of the step (tests/test_gpu_projection.py)


def ident(dims):
    return "x".join(map(str, dims))


def long_axis(dims):
    """0 / 1 / 2 for a needle, None for any other shape"""
    return int(np.argmax(dims)) if max(dims) >= 65534 else None


def far_end(a, dims, axis=-1):
    """The part of the flat array `a` (component `axis` of the grid `dims`: -1 scalar, 0 / 1 / 2 = u / v / w) at or beyond index
    65536 on LONG_X, 262144 on LONG_Y, within the last 16 planes on LONG_Z; the whole array on a shape that is no needle."""
    bi, bj, bk = stag(*dims, axis)
    a3 = a.reshape(bk, bj, bi)
    la = long_axis(dims)
    if la is None:
        return a3
    if la == 0:
        return a3[:, :, FAR_FROM[0]:]
    if la == 1:
        return a3[:, FAR_FROM[1]:, :]
    return a3[bk - FAR_PLANES:]


def moved(ref, start, dims, axis=-1):
    """elements of the far end in which the reference differs from what the output started as (an array, or the pre-fill), and
    is not zero either: a cleared border does not count"""
    fr = far_end(ref, dims, axis)
    fs = far_end(start, dims, axis) if isinstance(start, np.ndarray) else start
    return int(((fr != fs) & (fr != 0)).sum())


def assert_not_vacuous(ref, start, dims, axis=-1, what=""):
    """on a needle: the oracle's output differs from its start in at least 16 elements of the far end.  Asserted on the reference,
    before anything else is looked at.  The SMALL shapes are exempt: an empty interior is what they are for."""
    if long_axis(dims) is not None:
        n = moved(ref, start, dims, axis)
        assert n >= MIN_MOVED, (what, ident(dims), axis, n)


class Inputs:
    """everything an operator case reads, frozen"""


@functools.lru_cache(maxsize=2)
def inputs(dims, h):
    """vectorised random inputs: velocity and scalars uniform in [0, 1), maps = identity + a displacement of at most 1.3 h per
    axis, everywhere (border nodes included: an operator must match the oracle on any finite map)"""
    ni, nj, nk = dims
    h = float(f32(h))
    rng = np.random.default_rng(ni * 1000003 + nj * 1009 + nk)
    rnd = lambda n: rng.random(n, dtype=f32)
    c = Inputs()
    c.dims, c.h, c.ni, c.nj, c.nk = dims, h, ni, nj, nk
    c.n, c.nu, c.nv, c.nw = c.sizes = F.sizes(ni, nj, nk)
    c.vel = [rnd(n) for n in c.sizes[1:]]
    c.cur = [rnd(n) for n in c.sizes[1:]]
    c.rho, c.rho2 = rnd(c.n), rnd(c.n)
    base = F.identity_maps(ni, nj, nk, h)
    amp = f32(1.3) * f32(h)
    for name in ("fwd", "back", "backp"):
        setattr(c, name, [(m + amp * (f32(2) * rnd(c.n) - f32(1))).astype(f32) for m in base])
    for v in vars(c).values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


def far_emitter(dims, h):
    """centre and radius of a sphere of radius 3 h, 6 cells from the far end of the long axis (mid-domain on a SMALL shape)"""
    la = long_axis(dims)
    centre = [0.5 * n * h for n in dims]
    if la is not None:
        centre[la] = (dims[la] - 6) * h
    return (*centre, 3.0 * h)


class Runner:
    """one (shape, spacing) on one backend (host_entry_case.Backend): the inputs, uploaded once and on demand"""

    def __init__(self, be, dims, h):
        self.be, self.c, self._dev = be, inputs(dims, h), {}

    def d(self, name):
        """device pointers of an input by name"""
        if name not in self._dev:
            v = getattr(self.c, name)
            self._dev[name] = self.be.dev(*(v if isinstance(v, list) else [v]))
        return ptrs(self._dev[name])

    def free(self):
        self._dev.clear()


def fill(sizes):
    return [np.full(n, PREFILL, f32) for n in sizes]


# ---------------------------------------------------------------------------------------------------------------------------
# The cases.  Each returns (axes, start, ref, call): the staggering of every output, what the outputs start as, the oracle's
# result from that start, and call(lib, out, d) that runs the entry point on device pointers `out` (d(name): pointers of an input).
# ---------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, lerp=False):
    """lerp: the case evaluates trilinear lerps, so FL_OPT_FAST_LERP changes its values"""
    def reg(fn):
        fn.lerp = lerp
        CASES[name] = fn
        return fn
    return reg


@case("init_maps")
def _(c):
    start = fill([c.n] * 3)
    ref = F.identity_maps(*c.dims, c.h)
    return (-1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_init_maps(*out, c.h, *c.dims)


def _forward(c, hint):
    cfldt, dt = 0.9 * c.h, 2.0 * c.h                  # |u| < 1: three RK sub-steps
    start = [a.copy() for a in c.fwd]
    ref = [a.copy() for a in c.fwd]
    oracle().orc_solve_forward(*map(fp, c.vel), *map(fp, ref), c.h, *c.dims, cfldt, dt)
    if hint is None:
        return (-1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_solve_forward(*d("vel"), *out, c.h, *c.dims, cfldt, dt)
    return (-1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_solve_forward_hint(*d("vel"), *out, c.h, *c.dims, cfldt, dt, hint)


def _backward(c, hint):
    sub = 0.8 * c.h
    start = fill([c.n] * 3)
    ref = fill([c.n] * 3)
    oracle().orc_solve_backwardDMC(*map(fp, c.vel), *map(fp, c.back), *map(fp, ref), c.h, *c.dims, sub)
    if hint is None:
        return (-1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_solve_backwardDMC(*d("vel"), *d("back"), *out, c.h, *c.dims, sub)
    return (-1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_solve_backwardDMC_hint(*d("vel"), *d("back"), *out, c.h, *c.dims, sub, hint)


CASES["solve_forward"] = lambda c: _forward(c, None)
CASES["solve_forward_hint"] = lambda c: _forward(c, 1)            # FL_MAP_HINT_FINITE: true of these inputs
CASES["solve_backwardDMC"] = lambda c: _backward(c, None)
CASES["solve_backwardDMC_hint"] = lambda c: _backward(c, 1)
for _n in ("solve_forward", "solve_forward_hint", "solve_backwardDMC", "solve_backwardDMC_hint"):
    CASES[_n].lerp = True
MAPS = ["init_maps", "solve_forward", "solve_forward_hint", "solve_backwardDMC", "solve_backwardDMC_hint"]


@case("advect_velocity", lerp=True)
def _(c):
    start, ref = fill(c.sizes[1:]), fill(c.sizes[1:])
    oracle().orc_advect_velocity(*map(fp, ref), *map(fp, c.vel), *map(fp, c.back), c.h, *c.dims, 0)
    return (0, 1, 2), start, ref, lambda lib, out, d: lib.gpu_advect_velocity(*out, *d("vel"), *d("back"), c.h, *c.dims, False)


@case("advect_field", lerp=True)
def _(c):
    start, ref = fill([c.n]), fill([c.n])
    oracle().orc_advect_field(fp(ref[0]), fp(c.rho), *map(fp, c.back), c.h, *c.dims, 0)
    return (-1,), start, ref, lambda lib, out, d: lib.gpu_advect_field(*out, *d("rho"), *d("back"), c.h, *c.dims, False)


@case("advect_vel_double", lerp=True)
def _(c):
    start, ref = [a.copy() for a in c.cur], [a.copy() for a in c.cur]
    oracle().orc_advect_vel_double(*map(fp, ref), *map(fp, c.vel), *map(fp, c.back), *map(fp, c.backp), c.h, *c.dims, 0, 0.6)
    return (0, 1, 2), start, ref, lambda lib, out, d: lib.gpu_advect_vel_double(*out, *d("vel"), *d("back"), *d("backp"), c.h, *c.dims, False, 0.6)


@case("accumulate_velocity", lerp=True)
def _(c):
    start, ref = [a.copy() for a in c.cur], [a.copy() for a in c.cur]
    oracle().orc_accumulate_velocity(*map(fp, c.vel), *map(fp, ref), *map(fp, c.fwd), c.h, *c.dims, 0, -0.5)
    return (0, 1, 2), start, ref, lambda lib, out, d: lib.gpu_accumulate_velocity(*d("vel"), *out, *d("fwd"), c.h, *c.dims, False, -0.5)


@case("accumulate_field", lerp=True)
def _(c):
    start, ref = [c.rho2.copy()], [c.rho2.copy()]
    oracle().orc_accumulate_field(fp(c.rho), fp(ref[0]), *map(fp, c.fwd), c.h, *c.dims, 0, 2.0)
    return (-1,), start, ref, lambda lib, out, d: lib.gpu_accumulate_field(*d("rho"), *out, *d("fwd"), c.h, *c.dims, False, 2.0)


@case("compensate_velocity", lerp=True)
def _(c):
    """outputs: the compensated field, the clobbered init, the scratch"""
    mk = lambda: [a.copy() for a in c.cur] + [a.copy() for a in c.vel] + [np.zeros(n, f32) for n in c.sizes[1:]]
    start, ref = mk(), mk()
    oracle().orc_compensate_velocity(*map(fp, ref), *map(fp, c.fwd), *map(fp, c.back), c.h, *c.dims, 0)
    return (0, 1, 2) * 3, start, ref, lambda lib, out, d: lib.gpu_compensate_velocity(*out, *d("fwd"), *d("back"), c.h, *c.dims, False)


@case("compensate_field", lerp=True)
def _(c):
    mk = lambda: [c.rho.copy(), c.rho2.copy(), np.zeros(c.n, f32)]
    start, ref = mk(), mk()
    oracle().orc_compensate_field(*map(fp, ref), *map(fp, c.fwd), *map(fp, c.back), c.h, *c.dims, 0)
    return (-1,) * 3, start, ref, lambda lib, out, d: lib.gpu_compensate_field(*out, *d("fwd"), *d("back"), c.h, *c.dims, False)


@case("estimate_distortion", lerp=True)
def _(c):
    start, ref = fill([c.n]), fill([c.n])
    oracle().orc_estimate_distortion(fp(ref[0]), *map(fp, c.back), *map(fp, c.fwd), c.h, *c.dims)
    return (-1,), start, ref, lambda lib, out, d: lib.gpu_estimate_distortion(*out, *d("back"), *d("fwd"), c.h, *c.dims)


def _semilag(c, axis):
    d3 = (int(axis == 0), int(axis == 1), int(axis == 2))
    cfldt, dt = 0.9 * c.h, -1.5 * c.h
    n = c.sizes[1 + axis]
    start, ref = fill([n]), fill([n])
    oracle().orc_semilag(fp(ref[0]), fp(c.cur[axis]), *map(fp, c.vel), *d3, c.h, *c.dims, cfldt, dt)
    return (axis,), start, ref, lambda lib, out, d: lib.gpu_semilag(*out, d("cur")[axis], *d("vel"), *d3, c.h, *c.dims, cfldt, dt)


def _clamp(c, axis):
    """gpu_clamp_extrema on one staggered component: the candidate overshoots the field by up to 0.3 either way"""
    d3 = (int(axis == 0), int(axis == 1), int(axis == 2))
    bi, bj, bk = stag(*c.dims, axis)
    dt = 1.7 * c.h
    field = c.vel[axis]
    cand = (field + f32(0.6) * (c.cur[axis] - f32(0.5))).astype(f32)
    start, ref = [cand], [cand.copy()]
    off = [0.5 * x for x in d3]
    oracle().orc_clamp_extrema(fp(field), fp(ref[0]), *map(fp, c.vel), bi, bj, bk, *d3, *off, c.h, dt)
    return (axis,), start, ref, lambda lib, out, d: lib.gpu_clamp_extrema(d("vel")[axis], *out, *d("vel"), bi, bj, bk, *d3, *off, c.h, dt)


def _maccormack(c, axis):
    """gpu_maccormack on one staggered component against its definition on the oracle (include/bimocq_gpu.h; the composition of
    tests/test_gpu_maccormack.py): semi-Lagrangian pass back, two additions, the limiter.  Every node of `out` is written."""
    o = oracle()
    d3 = (int(axis == 0), int(axis == 1), int(axis == 2))
    bi, bj, bk = stag(*c.dims, axis)
    cfldt, dt = 0.9 * c.h, 1.5 * c.h
    f1, f_adv = c.cur[axis], c.vel[axis]
    n = f1.size
    back = np.zeros(n, f32)
    o.orc_semilag(fp(back), fp(f1), *map(fp, c.vel), *d3, c.h, *c.dims, cfldt, dt)
    ref = f1.copy()
    o.orc_add(fp(ref), fp(back), -0.5, n)
    o.orc_add(fp(ref), fp(f_adv), 0.5, n)
    o.orc_clamp_extrema(fp(f_adv), fp(ref), *map(fp, c.vel), bi, bj, bk, *d3, *[0.5 * x for x in d3], c.h, dt)
    return (axis,), fill([n]), [ref], lambda lib, out, d: lib.gpu_maccormack(*out, d("cur")[axis], d("vel")[axis], d("vel")[axis], *d("vel"),
                                                                             *d3, c.h, *c.dims, cfldt, dt, dt)


for _a in range(3):
    CASES["maccormack_%s" % "uvw"[_a]] = functools.partial(_maccormack, axis=_a)
    CASES["maccormack_%s" % "uvw"[_a]].lerp = True
for _a in range(3):
    CASES["semilag_%s" % "uvw"[_a]] = functools.partial(_semilag, axis=_a)
    CASES["semilag_%s" % "uvw"[_a]].lerp = True
    CASES["clamp_extrema_%s" % "uvw"[_a]] = functools.partial(_clamp, axis=_a)
    CASES["clamp_extrema_%s" % "uvw"[_a]].lerp = True
GATHERS = ["advect_velocity", "advect_field", "advect_vel_double", "accumulate_velocity", "accumulate_field", "compensate_velocity",
           "compensate_field", "estimate_distortion", "semilag_u", "semilag_v", "semilag_w", "clamp_extrema_u", "clamp_extrema_v",
           "clamp_extrema_w", "maccormack_u", "maccormack_v", "maccormack_w"]


@case("emit_smoke")
def _(c):
    sizes = list(c.sizes[1:]) + [c.n, c.n]
    args = (*far_emitter(c.dims, c.h), 1.0, 50.0, 1.0)
    start, ref = fill(sizes), fill(sizes)
    oracle().orc_emit_smoke(*map(fp, ref), c.h, *c.dims, *args)
    return (0, 1, 2, -1, -1), start, ref, lambda lib, out, d: lib.gpu_emit_smoke(*out, c.h, *c.dims, *args)


@case("add_buoyancy")
def _(c):
    start, ref = [c.vel[1].copy()], [c.vel[1].copy()]
    oracle().orc_add_buoyancy(fp(ref[0]), fp(c.rho), fp(c.rho2), *c.dims, 0.3, 1.1, 2 * c.h)
    return (1,), start, ref, lambda lib, out, d: lib.gpu_add_buoyancy(*out, *d("rho"), *d("rho2"), *c.dims, 0.3, 1.1, 2 * c.h)


def _diffuse(c, axis):
    """gpu_diffuse_field on one component's buffer: field, tmp0, tmp1 (three sweeps: the stale border of tmp1 reaches the result)"""
    nb = stag(*c.dims, axis)
    mk = lambda: [c.vel[axis].copy(), c.cur[axis].copy(), fill([c.sizes[1 + axis]])[0]]
    start, ref = mk(), mk()
    oracle().orc_diffuse_field(*map(fp, ref), *nb, 3, 0.37)
    return (axis,) * 3, start, ref, lambda lib, out, d: lib.gpu_diffuse_field(*out, *nb, 3, 0.37)


def _diffuse_sweeps_w(c):
    """gpu_diffuse_sweeps on the w buffer, the tallest of a grid (nk + 1 planes): both ping-pong buffers after three sweeps"""
    nb = stag(*c.dims, 2)
    mk = lambda: [c.cur[2].copy(), fill([c.nw])[0]]
    start, ref = mk(), mk()
    assert oracle().orc_diffuse_sweeps(fp(c.vel[2]), *map(fp, ref), *nb, 3, 0.37) == 1

    def call(lib, out, d):
        assert lib.gpu_diffuse_sweeps(d("vel")[2], *out, *nb, 3, 0.37) == 1
    return (2, 2), start, ref, call


def _clamp_box_w(c, w_form):
    """gpu_clamp_extrema_box / _box_w on the w buffer: the candidate overshoots the field by up to 0.3 either way"""
    nb = stag(*c.dims, 2)
    cand = (c.vel[2] + f32(0.6) * (c.cur[2] - f32(0.5))).astype(f32)
    start, ref = [cand], [cand.copy()]
    (oracle().orc_clamp_extrema_box_w if w_form else oracle().orc_clamp_extrema_box)(fp(c.vel[2]), fp(ref[0]), *nb)
    if w_form:
        return (2,), start, ref, lambda lib, out, d: lib.gpu_clamp_extrema_box_w(d("vel")[2], *out, *nb)
    return (2,), start, ref, lambda lib, out, d: lib.gpu_clamp_extrema_box(d("vel")[2], *out, *nb)


for _a in range(3):
    CASES["diffuse_field_%s" % "uvw"[_a]] = functools.partial(_diffuse, axis=_a)
CASES["diffuse_sweeps_w"] = _diffuse_sweeps_w
CASES["clamp_extrema_box_on_w"] = functools.partial(_clamp_box_w, w_form=False)
CASES["clamp_extrema_box_w"] = functools.partial(_clamp_box_w, w_form=True)
# the entry points that take a component's own dims, on every component: w has nk + 1 planes
BUFFER_DIMS = ["diffuse_field_u", "diffuse_field_v", "diffuse_field_w", "diffuse_sweeps_w", "clamp_extrema_box_on_w", "clamp_extrema_box_w"]
for _n in BUFFER_DIMS:
    CASES[_n].lerp = False
STREAMING = ["emit_smoke", "add_buoyancy"] + BUFFER_DIMS


@case("divergence")
def _(c):
    start, ref = fill([c.n]), fill([c.n])
    oracle().orc_divergence(*map(fp, c.vel), fp(ref[0]), *c.dims, 0.5)
    return (-1,), start, ref, lambda lib, out, d: lib.gpu_divergence(*d("vel"), *out, *c.dims, 0.5)


def _sweeps(c, sweeps):
    """p and p_temp after `sweeps` ping-pong sweeps; p_temp starts as the pre-fill, whose boundary layer must survive"""
    mk = lambda: [c.rho.copy(), fill([c.n])[0]]
    start = mk()
    a, b = mk()
    for _ in range(sweeps):
        oracle().orc_jacobi_sweep(fp(a), fp(c.rho2), fp(b), *c.dims, ALPHA, BETA)
        a, b = b, a
    ref = [a, b] if sweeps % 2 == 0 else [b, a]           # in the order (p, p_temp)

    def call(lib, out, d):
        assert lib.gpu_jacobi_sweeps(out[0], *d("rho2"), out[1], *c.dims, sweeps, ALPHA, BETA) == sweeps % 2
    return (-1, -1), start, ref, call


for _s in (1, 4, 7):
    CASES["jacobi_sweeps_%d" % _s] = functools.partial(_sweeps, sweeps=_s)
    CASES["jacobi_sweeps_%d" % _s].lerp = False


@case("gradient")
def _(c):
    start, ref = [a.copy() for a in c.vel], [a.copy() for a in c.vel]
    for ax, a in enumerate(ref):
        oracle().orc_gradient(fp(a), fp(c.rho), *stag(*c.dims, ax), int(ax == 0), int(ax == 1), int(ax == 2), 0.5)
    return (0, 1, 2), start, ref, lambda lib, out, d: lib.gpu_gradient(*out, *d("rho"), *c.dims, 0.5)


@case("projection_jacobi")
def _(c):
    """the raw entry point, five iterations from a warm p: u, v, w, div, p, p_temp"""
    mk = lambda: [a.copy() for a in c.vel] + [np.zeros(c.n, f32), c.rho.copy(), c.rho.copy()]
    start, ref = mk(), mk()
    oracle().orc_projection_jacobi(*map(fp, ref), None, *c.dims, 5, 0.5, ALPHA, BETA)
    return (0, 1, 2, -1, -1, -1), start, ref, lambda lib, out, d: lib.gpu_projection_jacobi(*out, None, *c.dims, 5, 0.5, ALPHA, BETA)


PROJECTION = ["divergence", "jacobi_sweeps_1", "jacobi_sweeps_4", "jacobi_sweeps_7", "gradient", "projection_jacobi"]


# the outputs on which non-vacuity is judged, where not on all: the first of several that move together; not the v and w an
# emitter without swirl zeroes; not the buffer a single sweep only reads
JUDGED = {"compensate_velocity": (0,), "compensate_field": (0,), "projection_jacobi": (0, 3), "diffuse_field_u": (0,),
          "diffuse_field_v": (0,), "diffuse_field_w": (0,), "diffuse_sweeps_w": (1,), "emit_smoke": (0, 3, 4), "jacobi_sweeps_1": (1,)}


def reference(c, name, fast=0):
    """(axes, start, ref, call) of a case, the oracle in the asked-for lerp arithmetic; non-vacuity asserted on the reference"""
    o = oracle()
    o.orc_set_fast_lerp(fast)
    try:
        axes, start, ref, call = CASES[name](c)
    finally:
        o.orc_set_fast_lerp(0)
    for q in JUDGED.get(name, range(len(ref))):
        assert_not_vacuous(ref[q], start[q], c.dims, axes[q], name)
    return axes, start, ref, call


def compare(r, name, start, ref, call, tag=()):
    """run the call on fresh copies of `start` and hold every output to the reference in value, over the whole array"""
    out = r.be.dev(*start)
    call(r.be.lib, ptrs(out), r.d)
    r.be.check()
    for q, (want, buf) in enumerate(zip(ref, out)):
        got = buf.numpy()
        if not F.same(want, got):
            bad = np.flatnonzero(~((want == got) | (np.isnan(want) & np.isnan(got))))
            raise AssertionError((name, tag, ident(r.c.dims), r.c.h, "output", q, "differing", bad.size, "first", bad[:4].tolist(),
                                  "last", bad[-4:].tolist(), "max |diff|", F.maxdiff(want, got)))


def run_case(r, name, fast=0, windows=(None,), opt_window=18):
    """one case in one lerp arithmetic: the reference once, the backend once per FL_OPT_FIELD_WINDOW value (None: as it is)"""
    from host_entry_case import options
    axes, start, ref, call = reference(r.c, name, fast)
    r.be.fast_lerp(fast)
    try:
        for w in windows:
            if w is None:
                compare(r, name, start, ref, call, (fast,))
            else:
                with options(r.be, {opt_window: w}):
                    compare(r, name, start, ref, call, (fast, "window", w))
    finally:
        r.be.fast_lerp(0)


# ---------------------------------------------------------------------------------------------------------------------------
# The operators with size rules of their own: gpu_flow_stats, gpu_emit_sources, gpu_render_density, gpu_obstacle_loads.  Their
# references are the C restatements and numpy terms of tests/diag_case.py, source_case.py, render_case.py and loads_case.py; here
# are the inputs at the far end, the references at needle size and their non-vacuity.
# ---------------------------------------------------------------------------------------------------------------------------
LD = np.longdouble
U53 = 2.0 ** -53


def blocked_sum(a):
    """The sum of a float64 array in extended precision, 128 terms at a time, level by level.  Each level adds 128 numbers in
    some order with one rounding of 2^-64 per addition: at most 127 * 2^-64 sum|term| of error (Higham, section 4.2), and four
    levels hold 128^4 = 2.7e8 terms.  The result therefore lies within 508 * 2^-64 sum|term| < 2^-53 sum|term| of the exact sum:
    the share tests/diag_case.py's bound sets aside for math.fsum's own rounding.  It stands in for math.fsum where a Python list
    of 26 M floats per sum is too slow; the bound n 2^-53 sum|term| holds against it unchanged."""
    assert np.finfo(LD).nmant >= 63 and a.size < 128 ** 4
    a = a.astype(LD).ravel()
    while a.size > 1:
        pad = (-a.size) % 128
        if pad:
            a = np.concatenate([a, np.zeros(pad, LD)])
        a = a.reshape(-1, 128).sum(axis=1)
    return a[0]


def flow_stats_reference(cpu, c):
    """(val {stat: longdouble}, bound {stat: float}, mag) of gpu_flow_stats on the inputs c, from the restatement's per-cell terms
    (diag_case.terms) as diag_case.exact forms them; every term here is >= 0, so sum|term| is the sum.  Non-vacuity: the
    vorticity magnitude, which the operator writes to every cell, moves at the far end."""
    import diag_case as D
    ni, nj, nk = c.dims
    e2, m2, d, mag = D.terms(cpu, *c.vel, c.h, c.dims)
    assert_not_vacuous(mag, PREFILL, c.dims, -1, "flow_stats")
    d64 = d.astype(np.float64)
    r = c.rho.astype(np.float64).reshape(nk, nj, ni)
    idx = [np.arange(n, dtype=np.float64) for n in c.dims]
    t = {"e2": lambda: e2, "m2": lambda: m2, "d2": lambda: d64 * d64, "rho": lambda: r, "rho_i": lambda: r * idx[0][None, None, :],
         "rho_j": lambda: r * idx[1][None, :, None], "rho_k": lambda: r * idx[2][:, None, None], "T": lambda: c.rho2.astype(np.float64)}
    val, bound = {}, {}
    for s in D.SUMS:                                       # one at a time: each is an array of n doubles
        terms = t[s]()
        assert terms.min() >= 0
        val[s] = blocked_sum(terms)
        bound[s] = c.n * U53 * float(np.nextafter(np.float64(val[s]), 0.0))
    with np.errstate(invalid="ignore"):
        val["div_max"] = float(np.fmax.reduce(np.abs(d), initial=f32(0)))
        val["vort_max"] = float(np.fmax.reduce(mag, initial=f32(0)))
    return val, bound, mag


def far_sources(dims, h):
    """a thin box with a jet along the whole long axis (on LONG_Z 98 % of it: box and sphere together must stay within the 65535
    planes one call takes), so that the launch covers every block row of the needle, then the far-end sphere with a jet and a spin"""
    from gpufluidsimulation_amd.solver import Source
    la = long_axis(dims)
    centre = [0.5 * n * h for n in dims]
    half = [1.2 * h] * 3
    if la is not None:
        half[la] = (0.49 if la == 2 else 1.0) * dims[la] * h
    cx, cy, cz, radius = far_emitter(dims, h)
    return [Source(("box", tuple(half)), tuple(centre), 0.5, 0.25, 10, velocity=(0.2, -0.1, 0.3)),
            Source(("sphere", radius), (cx, cy, cz), 1.0, 2.0, 10, velocity=(0.1, 0.5, -0.2), spin=(0.3, 1.5, -0.7))]


def sources_reference(cpu, c):
    """(sources, {name: flat array}) of gpu_emit_sources on fields that start as the pre-fill, by the C restatement"""
    import source_case as SC
    sources = far_sources(c.dims, c.h)
    start = dict(zip(SC.NAMES, fill([c.n, c.n, c.nu, c.nv, c.nw])))
    want = SC.emit_c(cpu, start, sources, c.h, c.dims)
    for name in SC.NAMES:
        assert_not_vacuous(want[name], PREFILL, c.dims, {"u": 0, "v": 1, "w": 2}.get(name, -1), "emit_sources " + name)
    return sources, want


def loads_reference(cpu, c):
    """(p, solid (nk, nj, ni), rows (nk, nj), centres, n, owner, terms) of gpu_obstacle_loads: the far-end sphere's flags by the
    restated gpu_obstacle_flags, a random pressure, the restatement's per-face terms (loads_case.abi_terms).  Non-vacuity: the
    obstacle lies wholly inside the far end and has at least 16 wetted faces."""
    import ctypes as C

    import loads_case as LC
    from gpufluidsimulation_amd.solver import boundary_array
    ni, nj, nk = c.dims
    sphere = far_emitter(c.dims, c.h)
    arr, n = boundary_array([(0, *sphere, 0.0, 0.0, 0.0, 0.0, 0.0)])
    solid, rows = np.zeros(c.n, np.uint8), np.zeros(nj * nk, np.uint8)
    cpu.gpu_obstacle_flags(solid.ctypes.data, rows.ctypes.data, C.addressof(arr), n, c.h, ni, nj, nk)
    p = (c.rho - f32(0.5)).reshape(nk, nj, ni)
    solid3 = solid.reshape(nk, nj, ni)
    centres = np.array([sphere[:3]], f32)
    owner, _, terms = LC.abi_terms(cpu, p, solid3, centres, n, c.h)
    if long_axis(c.dims) is not None:
        assert len(owner) >= MIN_MOVED and int((far_end(solid, c.dims) != 0).sum()) == int((solid != 0).sum()) >= MIN_MOVED
    return p, solid3, rows.reshape(nk, nj), centres, n, owner, terms


# (view, light, sigma h): along x lit from +z's far side; along -z lit along +y; along +z through cells that all clamp at d = 32,
# where the optical depth of a ray reaches nk * 32 * 2^32, just below 2^53 (why the operator takes no dimension above 65534)
RENDER_CASES = [(0, 5, 0.4), (5, 2, 0.4), (4, -1, 40.0)]


def render_reference(cpu, dims, h, view, light, sigma_h):
    """(rho, image, shadow) of gpu_render_density by the C restatement on render_case.density.  Non-vacuity on LONG_Z: with a
    light the shadow field moves in the last 16 planes; an image along x has its last 16 rows written; the opaque case is
    judged on the depth it exists for"""
    import render_case as RC
    rho = RC.density(dims, 3)
    if sigma_h > 32:
        rho = np.fmax(rho, f32(0.9))                                     # sigma h rho >= 36: every cell clamps at d = 32
    rc, img, shadow = RC.restate(cpu, rho, dims, h, view, light, float(f32(sigma_h) / f32(h)))
    assert rc == 0
    if long_axis(dims) == 2:
        if light >= 0:
            assert_not_vacuous(shadow.ravel(), PREFILL, dims, -1, "render shadow")
        if view // 2 == 0:
            assert int((img[:, dims[2] - FAR_PLANES:] > 0).sum()) >= MIN_MOVED
        if sigma_h > 32:
            assert img[1].max() >= 2.0 ** 52
    return rho, img, shadow


# ---------------------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------------------
STEP_FIELDS = ("rho", "T", "u", "v", "w", "p")
STEP_SWEEPS = 8


def step_scene(dims, h=H_POW2):
    """(L, emitters): L = ni h, and one emitter of radius 3 h, 6 cells from the far end of the long axis, active in both frames"""
    cx, cy, cz, radius = far_emitter(dims, h)
    return dims[0] * h, [(cx, cy, cz, radius, 1.0, 1.0, 0.0, 2)]


def run_steps(dims, scheme, h=H_POW2, steps=2, viscosity=0.0, **solver_kw):
    """`steps` steps of the host solver (BimocqGPUSolver(..., **solver_kw): the HIP library, or lib= / errlib= a CPU stand-in) and
    of OracleSolver, side by side: every field of every step equal in value; after the last step the oracle's rho and v are
    non-zero inside the far end."""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    from oracle_lib import OracleSolver
    L, emitters = step_scene(dims, h)
    o = OracleSolver(*dims, L, viscosity, 1.0)
    s = None
    try:
        s = BimocqGPUSolver(*dims, L, viscosity, 1.0, scheme=scheme, **solver_kw)
        o.set_smoke(0.0, 1.0, emitters)
        o.set_projection(STEP_SWEEPS, 0.5)
        if scheme:
            o.set_option(3, scheme)
        s.setSmoke(0.0, 1.0, emitters)
        s.setProjection(STEP_SWEEPS, 0.5)
        dt = 2.0 * float(o.h)
        for f in range(steps):
            o.advance(f, dt)
            s.advance(f, dt)
            s._check()
            assert s.cfldt == o.cfldt, (f, s.cfldt, o.cfldt)
            for name in STEP_FIELDS:
                a = o.field(name)
                if f == steps - 1 and name in ("rho", "v") and long_axis(dims) is not None:
                    live = int((far_end(a, dims, 1 if name == "v" else -1) != 0).sum())
                    assert live >= MIN_MOVED, (name, ident(dims), live)
                b = s.field(name)
                assert F.same(a, b), (ident(dims), scheme, f, name, int((a != b).sum()), F.maxdiff(a, b))
    finally:
        if s is not None:
            s.close()
        o.close()
