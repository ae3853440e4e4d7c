"""
GPU tests of the shading kernel instances of the streaming engine (k_s_shade_c, k_s_shade, k_s_shade_x: 26 compiled kernels, one
picked per launch by trc_stream_form_shade), run with -m gpu on the MI355X box.

Every case of shade_cases.py -- the smallest scene that selects its target instances; test_shade_cases_host.py checks the selection
and the conditions on the inputs without a device -- is traced by the streaming form and compared with oracle.engine on the same
Philox streams: per-surface tallies and the call's statistics, every surviving ray, every captured hit (a lean and a full capture),
and the flux map against numpy.histogram2d of the oracle's hits.  No ray is excluded: the reference has no near tie.  The
megakernel is held to the same assertions, which places a failure in the streaming path or in the shared per-ray core.  Which
instances these calls launched is recorded in profiles/shade_instances.txt from a kernel trace of this file.
"""
import os

import numpy as N
import pytest

import shade_cases as sc
from test_gpu_parity import RT, AT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


class env(object):
    """environment knobs of the library for the duration of a block (read at every call)"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = dict((k, os.environ.get(k)) for k in self.kw)
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reference(c):
    """the oracle's trace of the case; a SPEC case's wavelengths are the pending bundle's own, drawn on the device (shade_cases keeps
    that reference apart from the one made of the host sampler's draws)"""
    return sc.reference(c.name, wavelengths=N.array(c.source().get_wavelengths()) if c.spec else None)


def _by_point(points):
    return N.lexsort((points[2], points[1], points[0]))


def _check(ctx, c, o, given, stream, what, accel=True, kd=None, scene_knobs=None, warm_up=False, chart=None, reps=None, **knobs):
    """accel, kd: trace_fast's accel, a Kd-tree set on the scene; scene_knobs: knobs around the scene's creation (the library reads them
    there); warm_up: the call is made twice on the scene -- tallies, hits and maps reset in between -- and checked the second time;
    chart: (surface, chart, u edges, v edges) of a second flux map, in another chart than XY, held to the host histogram of the oracle's
    hits in that chart (fluxmap_chart_scene.host_maps; the case then has `frames`); reps: interactions, if not shade_cases.REPS"""
    from tracer_amd.scene import DeviceScene
    reps = sc.REPS if reps is None else reps
    with env(**(scene_knobs or {})):
        dev = DeviceScene(c.cs, ctx)
    if kd is not None:
        dev.set_kdtree(kd)
    dev.set_fluxmap(c.map_surf, *c.edges[c.map_surf])
    if chart is not None:
        dev.set_fluxmap(chart[0], chart[2], chart[3], chart=chart[1])
    dev.set_hit_capacity(8 * sc.N_RAYS + 65536)
    with env(**knobs):
        if warm_up:
            dev.trace_fast(c.bundle(given), reps, c.min_energy, sc.SEED, accel=accel, keep_last=True, stream=stream)
            dev.reset_tallies()
        st, last = dev.trace_fast(c.bundle(given), reps, c.min_energy, sc.SEED, accel=accel, keep_last=True, stream=stream)
    a, r, h = dev.get_tallies()
    hits = dev.get_hits()
    nx = dev.hit_spectral_columns()
    fm = dev.get_fluxmap(c.map_surf)
    fm_chart = dev.get_fluxmap(chart[0]) if chart is not None else None
    dev.close()
    assert st.hits_dropped == 0, what
    # tallies and statistics
    wrong = N.nonzero(h != o['hits'])[0]
    print('%s: %d segments, %d hits, %d left; largest differences: absorbed %.3g, received %.3g of %.3g' %
          (what, st.segments, st.hits, st.rays_left, N.abs(a - o['absorbed']).max(), N.abs(r - o['received']).max(), o['received'].max()))
    assert len(wrong) == 0, (what, 'hit counts differ on surfaces', wrong[:10], h[wrong[:10]], o['hits'][wrong[:10]])
    assert (st.segments, st.hits, st.rays_left) == (o['segments'], o['events'], o['last_energy'].size), what
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-12), (what, N.abs(a - o['absorbed']).argmax())
    assert N.allclose(r, o['received'], rtol=1e-9, atol=1e-12), (what, N.abs(r - o['received']).argmax())
    assert N.isclose(st.energy_left, o['last_energy'].sum(), rtol=1e-9, atol=1e-12), (what, st.energy_left, o['last_energy'].sum())
    # the surviving rays, matched as test_engines_vs_oracle_monte_carlo matches them
    mine = N.vstack(last)
    mine = mine[:, N.lexsort(N.round(mine[:3], 6))]
    theirs = N.vstack((o['last_vertices'], o['last_directions'], o['last_energy'][None, :]))
    theirs = theirs[:, N.lexsort(N.round(o['last_vertices'], 6))]
    assert mine.shape == theirs.shape, what
    assert N.allclose(mine[:3], theirs[:3], rtol=RT, atol=AT), (what, 'start points of the survivors')
    assert N.allclose(mine[3:6], theirs[3:6], rtol=1e-8, atol=1e-8), (what, 'directions of the survivors')
    assert N.allclose(mine[6], theirs[6], rtol=RT, atol=1e-12), (what, 'energies of the survivors')
    # the captured hits, per capturing surface, matched on sorted hit points
    H = o['hit_list']
    assert len(hits['surf']) == h[c.captured].sum() and hits['directions'] is not None, what
    assert nx == 3 * c.W, (what, nx)
    for s in c.captured:
        km, kt = N.nonzero(hits['surf'] == s)[0], N.nonzero(H['surf'] == s)[0]
        assert len(km) == len(kt) == h[s], (what, s)
        km, kt = km[_by_point(hits['points'][:, km])], kt[_by_point(H['points'][:, kt])]
        assert N.allclose(hits['points'][:, km], H['points'][:, kt], rtol=RT, atol=AT), (what, s)
        assert N.allclose(hits['e_abs'][km], H['e_abs'][kt], rtol=RT, atol=1e-12), (what, s)
        if s == c.full_surf:
            assert N.allclose(hits['e_in'][km], H['e_in'][kt], rtol=RT, atol=1e-12), (what, s)
            assert N.allclose(hits['directions'][:, km], H['directions'][:, kt], rtol=1e-8, atol=1e-8), (what, s)
        else:           # lean: the incident energy reads back as the absorbed one, the directions as 0
            assert N.array_equal(hits['e_in'][km], hits['e_abs'][km]) and not hits['directions'][:, km].any(), (what, s)
        if c.W:
            got = N.vstack((hits['spectra'][2], hits['spectra'][0], hits['spectra'][1]))[:, km]        # wavelengths, arrived, left
            assert N.array_equal(got[:c.W], H['x'][:c.W, kt]), (what, s)
            assert N.allclose(got[c.W:], H['x'][c.W:, kt], rtol=RT, atol=1e-12 * H['x'][c.W:].max()), (what, s)
    # the flux map against the host histogram of the oracle's hits
    Hm, e_out, n_out, n_hits = o['maps'][c.map_surf]
    tol = 1e-9 * Hm.max()
    assert fm.shape == Hm.shape and n_hits == h[c.map_surf]
    assert N.allclose(fm, Hm, rtol=1e-9, atol=tol), (what, N.abs(fm - Hm).max(), Hm.max())
    assert N.isclose(a[c.map_surf] - fm.sum(), e_out, rtol=1e-9, atol=tol), (what, a[c.map_surf] - fm.sum(), e_out)
    if chart is not None:           # the map in another chart, at the same tolerances
        import fluxmap_chart_scene as fc
        Hc, e_out, n_out, n_hits, n_edge = fc.host_maps(o['hit_list'], c.frames, {chart[0]: (chart[1], False, chart[2], chart[3])})[chart[0]]
        tol = 1e-9 * Hc.max()
        assert fm_chart.shape == Hc.shape and n_hits == h[chart[0]] and n_edge == 0 and Hc.max() > 0., what
        assert N.allclose(fm_chart, Hc, rtol=1e-9, atol=tol), (what, N.abs(fm_chart - Hc).max(), Hc.max())
        assert N.isclose(a[chart[0]] - fm_chart.sum(), e_out, rtol=1e-9, atol=tol), (what, a[chart[0]] - fm_chart.sum(), e_out)


def _ids(name):
    return '%s[%s]' % (name, '+'.join(t.replace(' ', '') for t in sc.CASES[name][5]))


@pytest.mark.parametrize('name', sorted(sc.CASES), ids=_ids)
def test_streaming_form_against_the_oracle(ctx, name):
    """fresh rays of the descriptor source (footprint route); the carry cases: their bundle with spectra, or with wavelengths and
    complex indices against a pane between two materials"""
    c = sc.case(name)
    _check(ctx, c, _reference(c), False, True, (name, 'stream'))


@pytest.mark.parametrize('name', sc.GIVEN, ids=_ids)
def test_streaming_form_on_the_given_rays(ctx, name):
    """the same rays handed over as a bundle (the general route of fresh rays): the same reference"""
    c = sc.case(name)
    _check(ctx, c, _reference(c), True, True, (name, 'stream, given'))


@pytest.mark.parametrize('name', [n for n in sorted(sc.CASES) if not sc.CASES[n][0].startswith('carry')], ids=_ids)
def test_megakernel_against_the_oracle(ctx, name):
    """the same call with stream=False (rays that carry spectra or complex indices are the streaming form's alone)"""
    c = sc.case(name)
    _check(ctx, c, _reference(c), False, False, (name, 'megakernel'))


@pytest.mark.parametrize('knob', ['TRC_STREAM_STATIC', 'TRC_STREAM_ABSORB'])
@pytest.mark.parametrize('name', sc.KNOBS, ids=_ids)
def test_streaming_knobs_on_tables_in_global_memory(ctx, name, knob):
    """one LDS = false case of each kernel family with the pre-assigned chunks of the active list, and the split of terminal hits,
    switched off"""
    c = sc.case(name)
    _check(ctx, c, _reference(c), False, True, (name, knob + '=0'), **{knob: 0})
