"""
What can be said of the ray-splitting cases (split_cases.py) without a device: the oracle's figures for the scenes, the slot arithmetic
of the ray table that grows (trc_split_room_need and trc_split_grow of csrc/trc_bounds.h, by the program of tests/splitcheck built with
the sanitizers), and where TracerEngine.ray_tracer(engine='auto') sends a scene whose optics split rays.
"""
import os
import subprocess

import numpy as N
import pytest

import split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', sorted(sc.ORACLE))
def test_oracle_figures(name):
    """hits per surface, segments, rays left, captured hits and the largest live population of the oracle's trace, pinned"""
    hits, segments, left, captured, max_live = sc.ORACLE[name]
    c, o = sc.case(name), sc.reference(name)
    assert [int(h) for h in o['hits']] == hits
    assert (o['segments'], o['last_energy'].size, o['max_live']) == (segments, left, max_live)
    H = o['hit_list']
    assert len(H['surf']) == sum(hits) == o['events']
    assert int(N.isin(H['surf'], c.captured).sum()) == captured
    # the hit list (one entry per hit, whatever it sent on) holds what the surfaces absorbed
    assert N.allclose(N.bincount(H['surf'], weights=H['e_abs'], minlength=c.cs.n_surf), o['absorbed'], rtol=1e-12, atol=1e-18)


def test_the_cases_are_what_they_are_for():
    """slab_recv captures more than the default room of 2 n + 1024 hits; mixed outgrows a ray table of 2048 slots several times over;
    the *_global cases keep the shading kernel's tables out of LDS; every case's map sees hits inside and outside"""
    assert sc.ORACLE['slab_recv'][3] > 2 * 256 + 1024
    assert sc.ORACLE['mixed'][4] > 4 * 2048
    for name in ('slab_global', 'mixed_global'):
        assert len(sc.case(name).cs.extra) * 8 > 72 * 1024
    for name in sorted(sc.CASES):
        Hm, e_out, n_out, n_hits = sc.reference(name)['maps'][sc.case(name).map_surf]
        assert Hm.sum() > 0. and n_hits > 0, name
        if not name.startswith('wave'):          # (normal incidence: every hit lands inside the map)
            assert n_out > 0 and (Hm > 0).mean() > 0.5, name
    # every splitting hit of slab takes one new slot: 256 + 2048
    o = sc.reference('slab')
    two = sum(int((N.bincount(N.asarray(L['parents'], dtype=int)) == 2).sum()) for L in o['levels'][1:])
    assert 256 + two == 2304


def test_room_arithmetic_under_the_sanitizers():
    """tests/splitcheck/split_check: need >= slots + live + tails on a grid, monotone, reached by doubling, nothing wraps past 64 bits"""
    subprocess.check_call(['make', '-s', '-C', ROOT, 'splitcheck'])
    p = subprocess.run([os.path.join(ROOT, 'tests', 'splitcheck', 'split_check')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert ' 0 violations' in p.stdout


class _Dev(object):
    """what ray_tracer reads of a device scene before it picks an engine"""
    def __init__(self, compiled):
        self.compiled = compiled
        self.n_surf = compiled.n_surf


def _route(monkeypatch, asm, bundle, **kw):
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.scene import compile_scene
    eng = TracerEngine(asm)
    went = []
    monkeypatch.setattr(eng, '_device_scene', lambda unchanged=False: _Dev(compile_scene(asm)))
    monkeypatch.setattr(eng, '_trace_fast', lambda *a, **k: went.append('fast'))
    monkeypatch.setattr(eng, '_trace_ordered', lambda *a, **k: went.append('ordered'))
    eng.ray_tracer(bundle, reps=4, min_energy=1e-9, seed=1, **kw)
    assert len(went) == 1
    return went[0]


def test_routing_of_scenes_that_split_rays(monkeypatch):
    """engine='auto': tree=False with 64 rays or more goes to the fast engine; fewer rays, the ray tree and a pending source with a
    spectrum stay with the ordered engine"""
    from tracer_amd import sources
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.source_spectrum import SourceSpectrum
    from tracer_amd.tracer_engine import TracerEngine
    asm = sc.scene('slab')[0]

    def given(n):
        v, d, e = sc.rays(n)
        return RayBundle(vertices=v, directions=d, energy=e)

    pending = lambda spectrum: sources.rect_bundle(256, N.c_[[0., 0., 2.]], N.r_[0., 0., -1.], 2., 2., 0.3, flux=1., seed=3, spectrum=spectrum)
    wl = N.linspace(0.3e-6, 2.5e-6, 9)
    assert TracerEngine.SPLIT_ON_FAST           # (set by the measurement of profiles/gpu_split.txt)
    assert _route(monkeypatch, asm, given(64), tree=False) == 'fast'
    assert _route(monkeypatch, asm, given(256), tree=False) == 'fast'
    assert _route(monkeypatch, asm, pending(None), tree=False) == 'fast'
    assert _route(monkeypatch, asm, given(63), tree=False) == 'ordered'
    assert _route(monkeypatch, asm, given(256), tree=True) == 'ordered'
    assert _route(monkeypatch, asm, pending(SourceSpectrum.tabulated(wl, 1. + N.sin(4e6 * wl) ** 2)), tree=False) == 'ordered'
    # a scene whose optics send one ray on is routed as before
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd import optics_callables as opt
    one = Assembly(objects=[AssembledObject(surfs=[Surface(RectPlateGM(8., 8.), opt.RefractiveHomogenous(1., 1.5))])])
    assert _route(monkeypatch, one, given(40), tree=False) == 'fast' and _route(monkeypatch, one, given(40), tree=True) == 'ordered'
