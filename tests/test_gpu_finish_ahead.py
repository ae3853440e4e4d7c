"""
GPU tests of the segments finished ahead (k_s_shade_c<MIRROR, flat, LDS> finishes the next segment of a continued ray inside the
clear cone of the tile it leaves: csrc/trc_shade.hip, trc_stream_form_ahead in csrc/trc_forms.h).  Every scene is traced by the
streaming form twice with TRC_STREAM_AHEAD=0 (every continued ray goes to k_s_bounce) and once with 1.  The knob is read at every call
(stream_knobs), so one process serves both.  The path changes no result: segments, hits, rays left, hits dropped, bounces, the hit
counts per surface and the captured hits (as a sorted list: the order in which waves append is not fixed) are byte-identical.  The
energy sums and the flux-map bins are float64 atomic sums of the same terms in another order: they agree within what the two runs
without the path differ by, or, where those two happen to agree more closely, within hits * 2^-52 of the sum (the bound on
reordering a sum of that many terms).
"""
import os

import numpy as N
import pytest

import ahead_cases as A
import clear_cases as K

pytestmark = pytest.mark.gpu

RAYS = 200000


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


def _trace(ctx, cs, src, ahead, reps=20, n=RAYS, seed=7, min_energy=1e-10, fluxmap=None, capacity=None, env=None):
    """fluxmap: (surface, u edges, v edges); capacity: of the hit buffer (None: room for a hit per ray -- without a capacity the
    scene captures nothing); env: further knobs of the call"""
    from tracer_amd import scenes
    from tracer_amd.scene import DeviceScene
    knobs = dict(env or {}, TRC_STREAM_AHEAD='1' if ahead else '0')
    old = dict((k, os.environ.get(k)) for k in knobs)
    os.environ.update(knobs)
    try:
        dev = DeviceScene(cs, ctx)
        if fluxmap is not None:
            dev.set_fluxmap(*fluxmap)
        dev.set_hit_capacity(n if capacity is None else capacity)
        st, _ = dev.trace_fast(scenes.nsttf_source(n, src, seed=seed, ray_offset=4321), reps, min_energy, seed, accel=True, stream=True)
        a, r, h = dev.get_tallies()
        hits = dev.get_hits()
        rows = N.vstack([hits['surf'].astype(float), hits['e_abs'], hits['points'][0], hits['points'][1], hits['points'][2]]).T
        rows = rows[N.lexsort(rows.T[::-1])] if len(rows) else rows
        out = dict(a=a.copy(), r=r.copy(), h=h.copy(), segments=st.segments, hits=st.hits, left=st.rays_left, dropped=st.hits_dropped,
                   e_left=st.energy_left, bounces=st.bounces, launches=st.launches, rows=N.ascontiguousarray(rows))
        if fluxmap is not None:
            out['fm'] = dev.get_fluxmap(fluxmap[0]).copy()
        dev.close()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return out


def _same(off, off2, on, what, rows=True, sums=True):
    for k in ('segments', 'hits', 'left', 'dropped', 'bounces'):
        assert on[k] == off[k], (what, k, on[k], off[k])
    assert N.array_equal(on['h'], off['h']), (what, on['h'], off['h'])
    if rows:
        assert on['rows'].shape == off['rows'].shape and on['rows'].tobytes() == off['rows'].tobytes(), what
    if not sums:
        return
    for k in ('a', 'r'):
        spread = N.abs(off[k] - off2[k]).max()
        tol = N.maximum(spread, off['h'] * 2. ** -52 * N.abs(off[k]))
        print('%s %s: spread of two runs without the path %.3e, with the path off by at most %.3e' % (what, k, spread, N.abs(on[k] - off[k]).max()))
        assert (N.abs(on[k] - off[k]) <= tol).all(), (what, k, on[k] - off[k], tol)
    tol = max(abs(off['e_left'] - off2['e_left']), off['left'] * 2. ** -52 * abs(off['e_left']))
    assert abs(on['e_left'] - off['e_left']) <= tol, (what, on['e_left'], off['e_left'], tol)
    if 'fm' in off:
        spread = N.abs(off['fm'] - off2['fm']).max()
        tol = N.maximum(spread, off['hits'] * 2. ** -52 * N.abs(off['fm']))
        print('%s flux map: spread of two runs without the path %.3e, with the path off by at most %.3e' % (what, spread, N.abs(on['fm'] - off['fm']).max()))
        assert off['fm'].sum() > 0. and (N.abs(on['fm'] - off['fm']) <= tol).all(), (what, N.abs(on['fm'] - off['fm']).max())


def _three(ctx, make, what, rows=True, sums=True, **kw):
    cs, src = make if isinstance(make, tuple) else K.compiled(make)
    off, off2, on = _trace(ctx, cs, src, False, **kw), _trace(ctx, cs, src, False, **kw), _trace(ctx, cs, src, True, **kw)
    print('%s: segments %d, hits %d, bounces %d; launches without the path %d, with it %d' % (what, on['segments'], on['hits'], on['bounces'], off['launches'], on['launches']))
    _same(off, off2, on, what, rows, sums)
    return cs, src, off, on


@pytest.fixture(scope='module')
def forty():
    return K.compiled(lambda: K.nsttf(40))


def test_nsttf_forty(ctx, forty):
    """forty heliostats of NSTTF and the receiver, with the bench's flux map on it"""
    cs, src, off, on = _three(ctx, forty, 'nsttf 40', reps=100, fluxmap=(A.receiver_index(forty[0]),) + A.fluxmap_edges(50))
    assert on['h'][-1] > 0.01 * RAYS and len(on['rows']) == on['h'][-1], (on['h'], len(on['rows']))        # (only the receiver captures)
    assert on['launches'] <= off['launches'], (on['launches'], off['launches'])


def test_nsttf_forty_after_tracking(ctx):
    """the same field after track_sun to another zenith: the path follows the pose's cones"""
    cs, src, off, on = _three(ctx, A.nsttf_tracked, 'nsttf 40, tracked', reps=100)
    assert on['hits'] > 0.01 * RAYS, on['hits']


def test_one_plate_every_ray_ahead(ctx):
    """every continued ray is inside its cone: the bounce behind the first shading is not launched at all, which proves that the
    path ran; segments and bounces count it as before"""
    cs, src, off, on = _three(ctx, A.one_plate, 'one plate')
    assert on['launches'] < off['launches'], (on['launches'], off['launches'])
    assert on['h'][-1] > 100 and len(on['rows']) == on['h'][-1], (on['h'], len(on['rows']))
    assert on['segments'] > RAYS + on['h'][-1] // 2, (on['segments'], on['h'])      # (the plates' rays to the receiver are a segment each)


def test_shadowing_plates(ctx):
    """rays go plate -> plate -> receiver, so the second shading launch takes the path too; the hit counts equal the oracle's"""
    cs, src, off, on = _three(ctx, K.shadowing, 'shadowing')
    from tracer_amd import scenes
    from oracle import engine as oracle_engine
    ref = oracle_engine.trace_from_compiled(cs, scenes.nsttf_source(RAYS, src, seed=7, ray_offset=4321).source_args(), reps=20, min_energy=1e-10)
    assert N.array_equal(ref['hits'], on['h']) and N.array_equal(ref['hits'], off['h']), (ref['hits'], on['h'], off['h'])


@pytest.mark.parametrize('reps', [1, 2, 3])
def test_last_iteration(ctx, forty, reps):
    """reps = 1: every reflected ray is left over and none is finished ahead; 2: the segment finished ahead is the last; 3"""
    cs, src, off, on = _three(ctx, forty, 'nsttf 40, reps %d' % reps, reps=reps)
    if reps == 1:           # (the receiver's hits are those of rays that come straight from the sun)
        assert on['left'] > 0.01 * RAYS and on['segments'] == RAYS, (on['left'], on['segments'])
    else:
        assert on['h'][-1] > 0.01 * RAYS, on['h']


def test_reflective_receiver(ctx):
    """no surface ends every ray: the path stays out, and the results are the same"""
    cs, src, off, on = _three(ctx, A.reflective_receiver, 'reflective receiver')
    assert on['launches'] == off['launches'], (on['launches'], off['launches'])


def test_no_surface_set_apart(ctx):
    """six plates and no receiver: no cones, the path stays out"""
    cs, src, off, on = _three(ctx, K.no_apart, 'no surface set apart')
    assert on['launches'] == off['launches'], (on['launches'], off['launches'])


def test_mirror_before_receiver(ctx):
    """a mirror in front of a part of the receiver: rays that meet it first go on from it"""
    cs, src, off, on = _three(ctx, A.mirror_before_receiver, 'mirror before the receiver')
    assert (on['h'][-2:] > 100).all(), on['h']


def test_two_receivers(ctx):
    """two surfaces that end every ray, one partly in front of the other: the nearest takes the hit"""
    cs, src, off, on = _three(ctx, A.two_receivers, 'two receivers')
    assert (on['h'][-2:] > 100).all() and len(on['rows']) == on['h'][-2:].sum(), (on['h'], len(on['rows']))     # (both capture)


def test_capture_off(ctx):
    cs, src, off, on = _three(ctx, A.no_capture, 'no capture')
    assert len(on['rows']) == 0 and on['h'][-1] > 100, (len(on['rows']), on['h'])


def test_hit_buffer_too_small(ctx, forty):
    """a hit buffer asked for 1000 hits where the receiver takes thousands: the same number counts as dropped with and without the
    path (_same), and every hit of the receiver is either read back or counted as dropped -- none is written over.  (The buffer
    keeps room beyond what was asked for, a chunk per wave that can hold one open, HitBuffer::set_capacity: a call of this size
    drops none.)"""
    cs, src, off, on = _three(ctx, forty, 'small hit buffer', reps=100, capacity=1000)
    for out in (off, on):
        assert out['h'][-1] > 1000 and len(out['rows']) + out['dropped'] == out['h'][-1], (len(out['rows']), out['dropped'], out['h'])


def test_fluxmap_beyond_lds(ctx, forty):
    """a flux map whose bins do not fit LDS (fluxmap_scene.FLOOR_BINS['large']: 300 x 200): terminal hits are not finished in the
    search then, and the path stays out"""
    import fluxmap_scene as FS
    nu, nv = FS.FLOOR_BINS['large']
    fm = (A.receiver_index(forty[0]), N.linspace(-5.5, 5.5, nu + 1), N.linspace(-5.5, 5.5, nv + 1))
    _three(ctx, forty, 'flux map beyond LDS', reps=100, fluxmap=fm)


def test_energy_cut(ctx):
    """min_energy between what the two kinds of mirrors keep of a ray (ahead_cases.two_mirror_kinds): the rays of the dull plate end
    at it, the others go on -- fewer segments than with every ray going on, and the receiver still hit"""
    cs, src = K.compiled(A.two_mirror_kinds)
    first = _trace(ctx, cs, src, False, reps=1)
    e = first['r'].sum() / first['h'].sum()
    cs, src, off, on = _three(ctx, (cs, src), 'energy cut', min_energy=0.7 * e)
    full = _trace(ctx, cs, src, True)
    assert 0 < on['segments'] < full['segments'] - 100 and on['h'][-1] > 100, (on['segments'], full['segments'], on['h'])


def test_two_batches(ctx, forty):
    """2^23 + 64 rays: two batches in flight, hit chunks resumed across launches; counts and sorted hits only"""
    cs, src, off, on = _three(ctx, forty, 'two batches', sums=False, reps=100, n=(1 << 23) + 64)
    assert on['dropped'] == 0 and len(on['rows']) == on['h'][-1], (len(on['rows']), on['h'][-1])       # (no captured hit written over)
