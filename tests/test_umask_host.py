"""
The footprint map's mask over the uniforms on the host (no GPU): tests/umaskcheck, the header the kernels are made of compiled by
g++, against a float64 brute-force trace.  k_s_ucull decides from the top bits of a ray's two position uniforms, k_s_fresh2 finds
the list cell from the float32 start point: no ray that hits may be lost by either.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

import umask_cases as U

ROOT = U.ROOT
_p = C.POINTER(C.c_double)


@pytest.fixture(scope='module')
def uc():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'umaskcheck', 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'umaskcheck', 'libtrc_umask_check.so'))
    lib.uc_umask.restype = C.c_int
    lib.uc_generic.restype = C.c_long
    lib.uc_generic.argtypes = [C.c_int, C.c_double, C.c_long, C.POINTER(C.c_uint32), _p, C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope='module')
def cases(uc):
    hs = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_sunshape_check.so'))
    return U.host_cases(hs)


def _run(uc, cs, desc, n, M, seed=77, offset=0):
    out = N.zeros(14)
    why = C.create_string_buffer(128)
    extra = N.ascontiguousarray(cs.extra if len(cs.extra) else N.zeros(1))
    rc = uc.uc_umask(cs.n_surf, cs.descs, extra.ctypes.data_as(_p), C.byref(desc), C.c_long(n), C.c_uint64(seed), C.c_uint64(offset), M,
                     out.ctypes.data_as(_p), why, 128)
    return rc, out, why.value.decode()


def test_hit_rays_are_listed(uc, cases):
    """
    Every ray of a seeded sample whose brute-force trace hits a surface and that does not take the general path: its umask bit is
    set, and the Cartesian list cell of its float32 start point lists the surface.  No violation is allowed.  NSTTF under its Buie
    disc (2e5 rays) and three plates (centre, rim, seam) under each of the six source kinds, the pillbox rectangle with its swap
    and without.  Pass shares of NSTTF (profiles/umask.txt): ucoverage against the Cartesian mask's coverage * 4 / pi.
    """
    for name, cs, desc, tab, n, M in cases:
        rc, o, why = _run(uc, cs, desc, n, M)
        assert rc == 0, (name, rc, why)
        print('%-22s umask %4d x %4d  ucoverage %.4f  rays with the bit set %.4f | Cartesian coverage %.4f (x 4/pi: %.4f) rays %.4f | hits %.4f general %.5f seam hits %d'
              % (name, o[8], o[9], o[6], o[2] / o[0], o[7], o[7] * 4 / N.pi, o[10] / o[0], o[3] / o[0], o[1] / o[0], o[13]))
        assert o[4] == 0 and o[5] == 0, (name, list(o))
        assert o[11] == 0 and o[12] == 0, (name, list(o))
        assert o[8] >= 32 and o[8] * o[9] == M * M, (name, list(o))
        assert o[3] > 1000, (name, list(o))                    # the sample does hit
        assert abs(o[2] / o[0] - o[6]) < 0.01, (name, list(o))    # the set share of the bits is the share of the rays listed
        if name == 'nsttf':
            assert o[6] < 0.35                                 # the mask still culls most of the disc
        elif 'disc' in name:
            assert o[13] > 0, (name, list(o))                  # rays in the first and the last sector hit the plate across the seam


def test_coarse_and_odd_maps(uc, cases):
    """the smallest budget (M = 32: 64 x 16 bits) and an M that is no power of two (96: the budget of 64 x 64 bits) stay conservative"""
    for name, cs, desc, tab, n, M in cases[1:]:
        for m, budget in ((32, 1024), (96, 4096)):
            rc, o, why = _run(uc, cs, desc, 20000, m, seed=5)
            assert rc == 0 and o[4] == 0 and o[5] == 0 and o[11] == 0, (name, m, why, list(o))
            assert o[8] >= 64 and o[8] * o[9] == budget, (name, m, list(o))


def test_integer_generic_test_matches(uc, cases):
    """trc_fp_generic as one unsigned compare: equal at and around the threshold, at 0 and at 2^32 - 1, for cdf_end of the NSTTF
    table, of 1 (no ray is general: the test is off) and of 0 (every ray is)"""
    desc = cases[0][2]
    from tracer_amd import _cabi
    ne = _cabi.TRC_BUIE_NELEM
    cdf_end = desc.buie[2 * (ne + 1) + ne]      # the last entry of the table's cdf (trc_fp_source)
    assert 0.9 < cdf_end < 1.
    for ce, want_on in ((cdf_end, 1), (1., 0), (0., 1), (0.5, 1), (1. - 2. ** -34, 0), (1. - 2. ** -33, 1), (1. - 2. ** -32, 1), (2. ** -33, 1), (3. * 2. ** -33, 1)):
        thr, on = C.c_double(), C.c_int()
        uc.uc_generic(1, ce, 0, None, C.byref(thr), C.byref(on))
        assert on.value == want_on, (ce, on.value)
        t = int(thr.value)
        vals = sorted(set(v % 2 ** 32 for v in (0, 1, 2, 2 ** 32 - 1, 2 ** 32 - 2, t - 2, t - 1, t, t + 1, t + 2, 2 ** 31)))
        o2 = N.array(vals, dtype=N.uint32)
        assert uc.uc_generic(1, ce, len(o2), o2.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(thr), C.byref(on)) == 0, ce
    # a source without a general path
    o2 = N.array([0, 2 ** 32 - 1], dtype=N.uint32)
    thr, on = C.c_double(), C.c_int()
    assert uc.uc_generic(0, 0.3, 2, o2.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(thr), C.byref(on)) == 0 and on.value == 0
