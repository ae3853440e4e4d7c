"""
GPU test of the streaming kernels that read their arguments again in every turn of their loops (kernel_args_again,
csrc/trc_device.h: k_s_bounce for continued rays, k_s_fresh2).  Run with -m gpu on the MI355X box.

Every case of lean_args_cases.py -- the smallest scenes that reach the instances: footprint-listed fresh rays of a Buie and of a
pillbox source, the grid in LDS with terminal hits finished inside k_s_bounce or behind its list (TRC_STREAM_ABSORB=1), surface by
surface, two shading classes, a curved surface, a given bundle -- is traced by the streaming form and, as the reference, by the
megakernel (stream=False), which has no kernel in common with it: search, shading and hit bookkeeping of the reference are other
code over the same per-ray core.  Every draw is a pure function of (seed, ray, event), so the two agree ray for ray: hit counts
per surface and the statistics exactly, the captured hits and the energies to the order of summation of float64 atomics.  The
library's knobs are environment variables: each setting gets one fresh child process, which traces all its cases (three
processes in all).
"""
import json
import os
import subprocess
import sys

import numpy as N
import pytest

import lean_args_cases as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12        # energies: the same per-ray values added in another order (at most 2e4 terms of one sign: 2e4 * 2^-53 = 2e-12
                    # is the bound for the worst order, 1e-14 what random orders give)


def _child(form, names, knobs):
    env = dict(os.environ)
    env.update((k, str(v)) for k, v in knobs.items())
    p = subprocess.run([sys.executable, os.path.join(HERE, 'lean_args_cases.py'), form] + list(names), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


@pytest.fixture(scope='module')
def runs():
    """{case: (streaming form, megakernel)}, computed once and left unchanged"""
    plain = [n for n in sorted(L.CASES) if not L.CASES[n][3]]
    stream = _child('stream', plain, {})
    mega = _child('mega', plain, {})
    out = dict((n, (stream[n], mega[n])) for n in plain)
    for n in sorted(L.CASES):
        knobs = L.CASES[n][3]
        if knobs:
            twin = [m for m in plain if L.CASES[m][:3] == L.CASES[n][:3] and L.CASES[m][4] == L.CASES[n][4]][0]
            out[n] = (_child('stream', [n], knobs)[n], mega[twin])
    return out


@pytest.mark.parametrize('name', sorted(L.CASES))
def test_streaming_form_equals_the_megakernel(runs, name):
    got, ref = runs[name]
    plate = got['plate']
    h = N.array(got['h'])
    print(name, 'hits per surface', h.astype(int), 'segments', got['segments'], 'largest differences: absorbed %.3g received %.3g flux map %.3g'
          % (N.abs(N.array(got['a']) - ref['a']).max(), N.abs(N.array(got['r']) - ref['r']).max(), N.abs(N.array(got['fm']) - ref['fm']).max()))
    # the case is what it says: every surface is hit, the plate by reflected rays too, rays go on after the first bounce
    assert (h > 0).all() and got['segments'] > L.N_RAYS + h[:plate].sum() // 2 and got['dropped'] == 0
    assert N.array_equal(h, ref['h']), name
    assert (got['segments'], got['hits']) == (ref['segments'], ref['hits']), name
    assert N.allclose(got['a'], ref['a'], rtol=RTOL, atol=0.), name
    assert N.allclose(got['r'], ref['r'], rtol=RTOL, atol=0.), name
    # the flux map: bin for bin, and its sum is what the plate absorbed (bench.py's check: 1e-6 of it)
    fm = N.array(got['fm'])
    assert N.allclose(fm, ref['fm'], rtol=RTOL, atol=RTOL * fm.max()), name
    assert abs(fm.sum() - got['a'][plate]) <= 1e-6 * got['a'][plate] and got['a'][plate] > 0, name
    # the captured hits (the plate's, and the diffuse plate's where there is one), sorted by surface and point: the same hits
    capturing = sorted(set(got['hit_surf']))
    assert plate in capturing and len(got['hit_surf']) == h[capturing].sum(), name
    assert got['hit_surf'] == ref['hit_surf'], name
    assert N.allclose(got['hit_points'], ref['hit_points'], rtol=RTOL, atol=1e-12), name
    assert N.allclose(got['hit_e'], ref['hit_e'], rtol=RTOL, atol=0.), name
