"""
What the thermal-emitter tests share (test_thermal_sources_host.py, test_gpu_thermal_sources.py): the fixture of the reference's
outputs (tests/golden/thermal_sources.npz, written by tests/golden/make_golden_thermal.py), its tables, the CDF of the polar angle
restated in NumPy from a raw table, and the host build of the per-ray code (tests/hostcheck/thermal_check.cpp).
"""
import ctypes as C
import os
import subprocess

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = N.load(os.path.join(ROOT, 'tests', 'golden', 'thermal_sources.npz'))
SEEDS = [int(s) for s in GOLD['seeds']]
NS = int(GOLD['ns'])
TABLES = ('dir', 'gray', 'gray2', 'cone', 'gap', 'steep')
REFERENCE_TABLES = ('dir', 'gray', 'cone', 'gap', 'steep')     # (the reference's weights are NaN on gray2)
T_WALL, BAND, REF_INDEX = float(GOLD['T']), [float(x) for x in GOLD['band']], float(GOLD['ref_index'])
_p = C.POINTER(C.c_double)


def ptr(a):
    return a.ctypes.data_as(_p)


def raw_table(name):
    """(thetas, emittances) as the fixture's generator made them: rounded to 8 decimals"""
    return GOLD[name + '_xs'], GOLD[name + '_ys']


def table(name):
    """the table as the library reads it: a last angle that states pi/2 to 8 decimals (1.57079633) is pi/2"""
    from tracer_amd import sources
    return sources.check_emittance_table(*raw_table(name))


def shape_kwargs(name):
    """the reference sampler's arguments of a fixture shape ('disk', 'triangle', 'cylinder', 'frustum_wide', 'frustum_narrow',
    'sphere'), as make_golden_thermal.SHAPES has them"""
    pre = 'shape_%s_' % name
    kw = dict((k[len(pre):], GOLD[k]) for k in GOLD.files if k.startswith(pre))
    return dict((k, (v.tolist() if k == 'angular_span' else v if v.ndim else float(v))) for k, v in kw.items())


def shape_dict(name, **extra):
    return {'type': name.split('_')[0], 'kwargs': dict(shape_kwargs(name), **extra)}


def shape_size(name):
    return max(float(N.abs(N.asarray(v)).max()) for v in shape_kwargs(name).values())


# -- the CDF of the polar angle, restated: F(theta) = integral of eps cos sin up to theta over the whole -----------------------------
def _H(a, b, t):
    """antiderivative of (a t + b) cos t sin t"""
    return (a * t + b) / 2. * N.sin(t) ** 2 - a / 4. * (t - N.sin(t) * N.cos(t))


def interval_masses(xs, ys):
    a = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1])
    b = ys[:-1] - a * xs[:-1]
    return _H(a, b, xs[1:]) - _H(a, b, xs[:-1]), a, b


def cdf_at(xs, ys, theta):
    """F at the angles theta (within the table), every interval with its own slope at both its ends"""
    m, a, b = interval_masses(xs, ys)
    cum = N.r_[0., N.cumsum(m)]
    i = N.clip(N.searchsorted(xs, theta, side='right') - 1, 0, xs.size - 2)
    return (cum[i] + _H(a[i], b[i], theta) - _H(a[i], b[i], xs[i])) / cum[-1]


def gauss_cdf(xs, ys):
    """the CDF at the nodes by a 16-point Gauss-Legendre rule per interval on (a theta + b) cos theta sin theta"""
    g, w = N.polynomial.legendre.leggauss(16)
    m = N.zeros(xs.size - 1)
    for i in range(xs.size - 1):
        h = 0.5 * (xs[i + 1] - xs[i])
        t = xs[i] + h * (g + 1.)
        eps = ys[i] + (ys[i + 1] - ys[i]) * (t - xs[i]) / (xs[i + 1] - xs[i])
        m[i] = h * N.sum(w * eps * N.cos(t) * N.sin(t))
    return N.r_[0., N.cumsum(m)] / N.sum(m), N.sum(m)


def gauss_cdf_at(xs, ys, theta):
    """F at the angles theta by a 16-point Gauss-Legendre rule per interval, the interval that holds theta taken up to theta: a
    yardstick that shares nothing with the sampler's antiderivative"""
    g, w = N.polynomial.legendre.leggauss(16)

    def integral(lo, hi, i):
        h = 0.5 * (hi - lo)
        t = lo[:, None] + h[:, None] * (g + 1.)
        eps = ys[i][:, None] + (ys[i + 1] - ys[i])[:, None] * (t - xs[i][:, None]) / (xs[i + 1] - xs[i])[:, None]
        return h * N.sum(w * eps * N.cos(t) * N.sin(t), axis=1)

    cum = N.r_[0., N.cumsum(integral(xs[:-1], xs[1:], N.arange(xs.size - 1)))]
    i = N.clip(N.searchsorted(xs, theta, side='right') - 1, 0, xs.size - 2)
    return (cum[i] + integral(xs[i], theta, i)) / cum[-1]


def inversion_grid(cdf_nodes, seed=12, m=100000):
    """the uniforms of the inversion check: m seeded ones, the first 6 + n replaced by 0, 2^-33, 2^-32, 1/2, 1 - 2^-32, 1 - 2^-53 and
    the n - 1 leading nodes of the table's CDF"""
    u = N.random.RandomState(seed).uniform(size=m)
    u[:6] = [0., 2. ** -33, 2. ** -32, 0.5, 1. - 2. ** -32, 1. - 2. ** -53]
    u[6:6 + cdf_nodes.size - 1] = cdf_nodes[:-1]
    return u


# -- the host build ------------------------------------------------------------------------------------------------------------------
def load_hostcheck():
    from tracer_amd import _cabi
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_thermal_check.so'))
    sd = C.POINTER(_cabi.SourceDesc)
    pi = C.POINTER(C.c_int)
    lib.ht_sizeof_source_desc.restype = C.c_long
    lib.ht_theta_max.restype = C.c_double
    lib.ht_pack.argtypes = [C.c_int, _p, _p, _p, _p]
    lib.ht_table_fault.argtypes = [C.c_int, _p, _p]
    lib.ht_table_fault.restype = C.c_char_p
    lib.ht_theta.argtypes = [_p, C.c_int, C.c_long, _p, _p, pi]
    lib.ht_points_u.argtypes = [_p, C.c_long, _p] + [_p] * 6
    lib.ht_dirs.argtypes = [C.c_long] + [_p] * 8
    lib.ht_rays.argtypes = [sd, _p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long] + [_p] * 10
    return lib


def pack(ht, xs, ys):
    """(packed table theta | eps / M | cdf, M) of the host build"""
    xs, ys = N.ascontiguousarray(xs, dtype=float), N.ascontiguousarray(ys, dtype=float)
    tab, mass = N.zeros(3 * xs.size), C.c_double()
    assert ht.ht_table_fault(xs.size, ptr(xs), ptr(ys)) == b''
    assert ht.ht_pack(xs.size, ptr(xs), ptr(ys), ptr(tab), C.byref(mass)) == 1
    return tab, mass.value


def theta_of(ht, tab, u):
    u = N.ascontiguousarray(u, dtype=float)
    th, it = N.zeros(u.size), N.zeros(u.size, dtype=N.int32)
    ht.ht_theta(ptr(tab), tab.size // 3, u.size, ptr(u), ptr(th), it.ctypes.data_as(C.POINTER(C.c_int)))
    return th, it


def points_u(ht, p, u):
    """(points, normals) of the shape with descriptor parameters p from the uniforms u (2, m)"""
    u = N.ascontiguousarray(u, dtype=float)
    p = N.ascontiguousarray(p, dtype=float)
    m = u.shape[1]
    out = [N.zeros(m) for _ in range(6)]
    ht.ht_points_u(ptr(p), m, ptr(u), *[ptr(o) for o in out])
    return N.array(out[:3]), N.array(out[3:])


def host_rays(ht, desc, tab, seed, rid0, m):
    """(points, directions, normals, uniforms (4, m)) of rays rid0 .. rid0 + m - 1 of a thermal descriptor by the host build; the
    normals are those the directions are drawn about, in the source's own frame (the descriptor's rot_dir poses them)"""
    out = [N.zeros(m) for _ in range(9)]
    u = N.zeros((4, m))
    ht.ht_rays(C.byref(desc), ptr(tab), tab.size // 3, seed, rid0, m, *([ptr(o) for o in out] + [ptr(u)]))
    return N.array(out[:3]), N.array(out[3:6]), N.array(out[6:]), u


def host_dirs(ht, theta, u3, normals):
    theta, u3 = N.ascontiguousarray(theta, dtype=float), N.ascontiguousarray(u3, dtype=float)
    n = [N.ascontiguousarray(normals[k]) for k in range(3)]
    out = [N.zeros(theta.size) for _ in range(3)]
    ht.ht_dirs(theta.size, ptr(theta), ptr(u3), ptr(n[0]), ptr(n[1]), ptr(n[2]), *[ptr(o) for o in out])
    return N.array(out)
