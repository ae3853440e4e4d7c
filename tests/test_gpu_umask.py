"""
GPU tests of the footprint map's mask over the uniforms (k_s_ucull in front of k_s_fresh2; csrc/trc_footprint.h, trc_stream.inc): the
scenes of umask_cases.py traced by the streaming form against the same call through the megakernel.  Every draw is a pure function
of (seed, ray, event), so the two agree ray for ray: hit counts per surface and the segment count exactly, the absorbed sums to
the order-of-summation noise of the float64 atomics (1e-9, as the rest of the suite).
"""
import numpy as N
import pytest

import umask_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


def _trace(ctx, cs, bundle, stream, reps=20):
    from tracer_amd.scene import DeviceScene
    dev = DeviceScene(cs, ctx)
    st, _ = dev.trace_fast(bundle(), reps, 1e-10, 1, accel=True, stream=stream)
    a, r, h = dev.get_tallies()
    out = dict(a=a.copy(), r=r.copy(), h=h.copy(), segments=st.segments, hits=st.hits)
    dev.close()
    return out


def _same(x, y, what):
    assert N.array_equal(x['h'], y['h']), (what, x['h'], y['h'])
    assert x['segments'] == y['segments'] and x['hits'] == y['hits'], (what, x['segments'], y['segments'])
    assert N.allclose(x['a'], y['a'], rtol=1e-9, atol=1e-12) and N.allclose(x['r'], y['r'], rtol=1e-9, atol=1e-12), what


@pytest.mark.parametrize('name,direction', U.KINDS, ids=[k[0] for k in U.KINDS])
def test_three_plates_stream_equals_megakernel(ctx, name, direction):
    """three plates (centre, rim, seam) under each source kind, 2^18 rays: every plate is hit, and the two forms agree"""
    asm, cs = U.three_plates(name, direction)
    n = 1 << 18
    bundle = lambda: U.source(name, n, direction, seed=11, ray_offset=12345)
    s, m = _trace(ctx, cs, bundle, True), _trace(ctx, cs, bundle, False)
    assert (m['h'] > 100).all() and m['segments'] > n, (name, m['h'])
    _same(s, m, name)


def test_three_plates_stream_ids_cross_2_32(ctx):
    """the Buie disc over the three plates with ray_offset placed so that the batch's stream ids cross a multiple of 2^32: the
    high word of the Philox counter changes inside the batch, in k_s_ucull as in k_s_fresh2"""
    name, direction = 'buie_disc', U.TILTED
    asm, cs = U.three_plates(name, direction)
    n = 1 << 18
    bundle = lambda: U.source(name, n, direction, seed=11, ray_offset=3 * 2 ** 32 - n // 2 - 77)
    s, m = _trace(ctx, cs, bundle, True), _trace(ctx, cs, bundle, False)
    assert (m['h'] > 100).all()
    _same(s, m, 'stream ids across 2^32')


def test_nsttf_stream_equals_megakernel(ctx):
    """NSTTF under its Buie disc, 2^20 rays"""
    from tracer_amd import scenes
    from tracer_amd.scene import compile_scene
    plant, field, rec, src = scenes.nsttf_field()
    cs = compile_scene(plant)
    n = 1 << 20
    bundle = lambda: scenes.nsttf_source(n, src, seed=5, ray_offset=987654321)
    s, m = _trace(ctx, cs, bundle, True, reps=100), _trace(ctx, cs, bundle, False, reps=100)
    assert m['h'][218] > 0.05 * n and m['h'][:218].sum() > 0.05 * n
    _same(s, m, 'NSTTF')
