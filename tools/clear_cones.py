#!/usr/bin/env python3
"""
The clear cones of the LDS-sized grid (csrc/trc_bounds.h: trc_clear_build) on the host, no GPU: per scene of tests/clear_cases.py and
per T (tiles per side of a plate) the build time, how many tiles get a cone, the distribution of the half-angles, a soundness pass
against brute force over the boxes, and the share of sampled continued rays that still walk the grid.

usage: clear_cones.py [--rays N] [--sound N] [--scenes a,b] [--T 1,2,4,8]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=float, default=3e6, help='source rays of the walk statistic')
    ap.add_argument('--sound', type=float, default=1e5, help='rays of the soundness pass')
    ap.add_argument('--scenes', default='')
    ap.add_argument('--T', default='1,2,4,8')
    args = ap.parse_args()
    import ctypes as C
    import clear_cases as K
    lib = K.load_check()
    Ts = [int(t) for t in args.T.split(',')]
    want = [s for s in args.scenes.split(',') if s]
    for name, make in K.SCENES:
        if want and name not in want:
            continue
        cs, src = K.compiled(make)
        rc, shares, tail = K.walk_share(lib, cs, src, args.rays, Ts)
        print('%s: %d surfaces; %d source rays, %d first hits, %d rays go on, %d of them meet a listed box (rc %d)'
              % (name, cs.n_surf, tail[0], tail[1], tail[2], tail[3], rc))
        for j, T in enumerate(Ts):
            rc, o = K.sound(lib, cs, T, int(args.sound))
            n, walk, bad, sec = shares[j]
            print('  T %d: build %.2f ms, table %d bytes, cones on %d of %d tiles, half-angle min / median / max %.4f / %.4f / %.4f rad; '
                  'soundness %d rays %d skip %d violations; continued rays %d, still walking %d = %.4f, skipped though blocked %d'
                  % (T, 1e3 * o[5], cs.n_surf * T * T * 16, o[3], o[4], o[7], o[8], o[9], o[0], o[1], o[2], n, walk, walk / max(n, 1.), bad))
    cones = C.c_int(0)
    for T in Ts:
        t = lib.cc_build_time(4095, T, C.byref(cones))
        print('regular field of 4095 plates and a receiver, T %d: build %.1f ms, %d cones' % (T, 1e3 * t, cones.value))


if __name__ == '__main__':
    main()
