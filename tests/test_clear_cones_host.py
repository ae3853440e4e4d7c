"""
The clear cones on the host (no GPU): tests/clearcheck, the builder of csrc/trc_bounds.h and the tile and cone tests of trc_core.h
compiled by g++, against brute force over the boxes a walking ray is tested with.  k_s_bounce leaves the grid walk out for a ray
inside the cone of the tile it left: no such ray may pass both boxes of any surface the grid lists.
"""
import ctypes as C
import os
import subprocess

import pytest

import clear_cases as K

ROOT = K.ROOT


@pytest.fixture(scope='module')
def cc():
    lib = K.load_check()
    lib.cc_T.restype = C.c_int
    return lib


@pytest.fixture(scope='module')
def scenes(cc):
    return {name: K.compiled(make) for name, make in K.SCENES}


def test_no_ray_inside_a_cone_meets_a_listed_box(cc, scenes):
    """
    Per scene 1.2e5 rays that start on the plates -- inside the tiles, on their seams, on the plates' edges and corners, on the plane
    and delta off it -- with directions inside the stored cones, uniform in angle and a fifth of them at 0.999 of the boundary: not
    one of the rays the kernel's test lets skip the walk passes both boxes of a listed surface.  The scene without a surface set apart
    has no cone at all.
    """
    T = cc.cc_T()
    for name, (cs, src) in scenes.items():
        rc, o = K.sound(cc, cs, T, 120000)
        print('%-20s T %d: %d cones on %d tiles (apart %d), half-angle %.4f / %.4f / %.4f rad, %d rays, %d skip, %d violations, build %.2f ms'
              % (name, T, o[3], o[4], o[6], o[7], o[8], o[9], o[0], o[1], o[2], 1e3 * o[5]))
        assert rc == 0 and o[10] == 0, (name, rc, list(o))
        assert o[2] == 0, (name, list(o))
        if name == 'no_apart':
            assert o[6] == 0 and o[3] == 0, (name, list(o))
        else:
            assert o[6] >= 1 and o[3] > 0 and o[0] == 120000 and o[1] > 0.9 * o[0], (name, list(o))


def test_wider_cones_are_caught(cc, scenes):
    """the same run with every stored k times 2.25 (cones 1.5 x wider) reports violations where plates stand in each other's beams"""
    T = cc.cc_T()
    for name in ('shadowing', 'nsttf'):
        rc, o = K.sound(cc, scenes[name][0], T, 120000, kscale=2.25)
        print('%-20s k x 2.25: %d rays, %d skip, %d violations' % (name, o[0], o[1], o[2]))
        assert rc == 0 and o[2] > 0, (name, list(o))


def test_nsttf_share_of_rays_that_still_walk(cc, scenes):
    """
    The rays that go on from the first hits of 3e6 NSTTF source rays (slope error 1 mrad): the share that still walks, per T.  At
    most 0.15 for the T the library is built with (one cone per plate measured 0.142 in the prototype of the bound, 0.1465 here; 8 x 8 tiles 0.0056),
    and no ray skips while a listed surface passes both boxes.  Measured shares: profiles/clear_cones.txt.
    """
    Ts = [1, 2, 4, 8]
    cs, src = scenes['nsttf']
    rc, shares, tail = K.walk_share(cc, cs, src, 3e6, Ts)
    assert rc == 0 and tail[2] > 1.5e5, (rc, list(tail))
    print('NSTTF: %d source rays, %d first hits, %d rays go on, %d of them meet a listed box' % tuple(tail))
    for T, (n, walk, bad, sec) in zip(Ts, shares):
        print('  T %d: %d continued rays, %d still walk = %.4f; skipped though a listed box is met: %d; build %.2f ms' % (T, n, walk, walk / n, bad, 1e3 * sec))
        assert bad == 0, (T, bad)
    n, walk, bad, sec = shares[Ts.index(cc.cc_T())]
    assert walk / n <= 0.15, (cc.cc_T(), walk / n)


def test_builder_under_the_sanitizers(cc, scenes, tmp_path):
    """tests/clearcheck/clear_check, the same source as a program of its own built with the address and undefined-behaviour
    sanitizers: it builds the tables of every scene, runs a short soundness pass and exits clean"""
    path = os.path.join(str(tmp_path), 'cases.bin')
    K.write_cases(path, [scenes[name][0] for name, _ in K.SCENES], cc.cc_T(), 5000)
    p = subprocess.run([os.path.join(ROOT, 'tests', 'clearcheck', 'clear_check'), path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0 and '%d cases, ok' % len(K.SCENES) in p.stdout, p.stdout
