"""
GPU tests of the clear cones (k_s_bounce<1, .., FRESH = false> leaves the grid walk out for a continued ray inside the cone of the
tile it left; csrc/trc_bounds.h: trc_clear_build, trc_stream.inc): every scene of clear_cases.py is traced by the streaming form once
with TRC_STREAM_CLEAR=0 (no table, every continued ray walks) and once with the table.  The knob is read at every call
(stream_knobs), so one process serves both.  The skip changes no result: the segment count, the hit counts per surface and the
captured hits (as a sorted list: the order in which waves append is not fixed) are byte-identical.  The energy sums are float64
atomic sums of the same terms in another order: they agree within what two runs of the same setting differ by, or, where those two
happen to agree more closely, within hits * 2^-52 of the sum (the bound on reordering a sum of that many terms).
"""
import os

import numpy as N
import pytest

import clear_cases as K

pytestmark = pytest.mark.gpu

RAYS = 200000


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


def _trace(ctx, cs, src, clear, reps=20, n=RAYS, seed=7):
    from tracer_amd import scenes
    from tracer_amd.scene import DeviceScene
    old = os.environ.get('TRC_STREAM_CLEAR')
    os.environ['TRC_STREAM_CLEAR'] = '1' if clear else '0'
    try:
        dev = DeviceScene(cs, ctx)
        st, _ = dev.trace_fast(scenes.nsttf_source(n, src, seed=seed, ray_offset=4321), reps, 1e-10, seed, accel=True, stream=True)
        a, r, h = dev.get_tallies()
        hits = dev.get_hits()
        rows = N.vstack([hits['surf'].astype(float), hits['e_abs'], hits['points'][0], hits['points'][1], hits['points'][2]]).T
        rows = rows[N.lexsort(rows.T[::-1])] if len(rows) else rows
        out = dict(a=a.copy(), r=r.copy(), h=h.copy(), segments=st.segments, hits=st.hits, rows=N.ascontiguousarray(rows))
        dev.close()
    finally:
        if old is None:
            del os.environ['TRC_STREAM_CLEAR']
        else:
            os.environ['TRC_STREAM_CLEAR'] = old
    return out


def _same(off, off2, on, what):
    assert on['segments'] == off['segments'] and on['hits'] == off['hits'], (what, on['segments'], off['segments'])
    assert N.array_equal(on['h'], off['h']), (what, on['h'], off['h'])
    assert on['rows'].shape == off['rows'].shape and on['rows'].tobytes() == off['rows'].tobytes(), what
    for k in ('a', 'r'):
        spread = N.abs(off[k] - off2[k]).max()
        tol = N.maximum(spread, off['h'] * 2. ** -52 * N.abs(off[k]))
        print('%s %s: spread of two runs without the table %.3e, with the table off by at most %.3e' % (what, k, spread, N.abs(on[k] - off[k]).max()))
        assert (N.abs(on[k] - off[k]) <= tol).all(), (what, k, on[k] - off[k], tol)


def _both(ctx, make, what, reps=20):
    cs, src = K.compiled(make)
    off, off2, on = _trace(ctx, cs, src, False, reps), _trace(ctx, cs, src, False, reps), _trace(ctx, cs, src, True, reps)
    _same(off, off2, on, what)
    return cs, src, off, on


def test_shadowing_plates(ctx):
    """three plates in a column, each in the beam of the one behind it: rays are blocked with both settings (the plates are hit by
    more rays than arrive from the sun), and the hit counts equal the oracle's"""
    cs, src, off, on = _both(ctx, K.shadowing, 'shadowing')
    for out, clear in ((off, False), (on, True)):
        first = _trace(ctx, cs, src, clear, reps=1)
        blocked = out['h'][:3].sum() - first['h'][:3].sum()
        print('clear %d: first hits on the three plates %d, hits of continued rays on them %d' % (clear, first['h'][:3].sum(), blocked))
        assert blocked > 100, (clear, out['h'], first['h'])
    from tracer_amd import scenes
    from oracle import engine as oracle_engine
    ref = oracle_engine.trace_from_compiled(cs, scenes.nsttf_source(RAYS, src, seed=7, ray_offset=4321).source_args(), reps=20, min_energy=1e-10)
    assert N.array_equal(ref['hits'], on['h']) and N.array_equal(ref['hits'], off['h']), (ref['hits'], on['h'], off['h'])


def test_nsttf_forty(ctx):
    """forty heliostats of NSTTF and the receiver"""
    cs, src, off, on = _both(ctx, lambda: K.nsttf(40), 'nsttf 40', reps=100)
    assert on['h'][0] > 0.01 * RAYS or on['h'][-1] > 0.01 * RAYS, on['h']


def test_nsttf_forty_after_tracking(ctx):
    """the same field after track_sun to another zenith: the table follows the pose"""
    def make():
        plant, field, src = K.nsttf(40)
        from tracer_amd import scenes
        from tracer_amd.models.heliostat_field import solar_vector
        pos = scenes.nsttf_positions()[:40]
        zen = 55. * N.pi / 180.
        field.track_sun(0.3, zen, aim_points=N.tile(N.array([0., 0., 60.]), (40, 1)))
        sun = solar_vector(0.3, zen)
        src = dict(src, center=N.vstack(300. * sun + N.r_[pos[:, :2].mean(axis=0), 0.]), direction=-sun)
        return plant, field, src
    cs, src, off, on = _both(ctx, make, 'nsttf 40, tracked', reps=100)
    assert on['hits'] > 0.01 * RAYS, on['hits']


def test_scene_without_a_surface_set_apart(ctx):
    """six plates and no receiver: no cones, and the same results"""
    _both(ctx, K.no_apart, 'no surface set apart')


def test_quadric_blocker(ctx):
    """a sphere and a cylinder in front of a plate"""
    cs, src, off, on = _both(ctx, K.quadric_neighbours, 'quadric neighbours')
    assert on['h'].sum() > 0.01 * RAYS, on['h']
