"""
GPU tests of ray-splitting optics on the streaming form of the fast engine (k_s_shade_x<.., SPLIT>, the ray table that grows), run with
-m gpu on the MI355X box.

Every case of split_cases.py is traced through the C-ABI (trc_trace_fast_x with TRC_TRACE_STREAM | TRC_TRACE_KEEP_LAST) and compared
with oracle.engine on the same Philox streams: hit counts per surface, segments, events and rays left exactly; tallies, energy left,
every surviving ray, every captured hit and a 6 x 6 flux map to the project's allowance for float64 atomics.  No ray is excluded.
The Python engine is held to the ordered engine's answers on the same seed.
"""
import os

import numpy as N
import pytest

import fluxmap_chart_scene as fcs
import split_cases as sc

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


def _order(*keys):
    """lexicographic order of columns rounded to 1e-7 (first key first)"""
    return N.lexsort([N.round(k, 7) for k in reversed(keys)])


CYL_EDGES = (N.array([-0.5, 0.5]), N.linspace(0., 2. * N.pi, 7))        # the floor in the cylinder chart: (local z, azimuth), 1 x 6


def _check(ctx, name, what, chart=False, stream=True, **knobs):
    from tracer_amd.scene import DeviceScene
    c, o = sc.case(name), sc.reference(name)
    dev = DeviceScene(c.cs, ctx)
    if chart:
        dev.set_fluxmap(c.map_surf, *CYL_EDGES, chart='cylinder')
    else:
        dev.set_fluxmap(c.map_surf, *c.edges[c.map_surf])
    dev.set_hit_capacity(o['events'] + 1024)
    with env(**knobs):
        st, last = dev.trace_fast(c.bundle(), c.reps, c.min_energy, c.seed, accel=True, keep_last=True, stream=stream,
                                  last_capacity=o['last_energy'].size + 64)
    a, r, h = dev.get_tallies()
    hits = dev.get_hits()
    nx = dev.hit_spectral_columns()
    fm = dev.get_fluxmap(c.map_surf)
    dev.close()
    print('%s: %d segments, %d hits, %d left, %d launches; largest differences: absorbed %.3g, received %.3g of %.3g, energy left %.3g of %.3g' %
          (what, st.segments, st.hits, st.rays_left, st.launches, N.abs(a - o['absorbed']).max(), N.abs(r - o['received']).max(), o['received'].max(),
           abs(st.energy_left - o['last_energy'].sum()), o['last_energy'].sum()))
    assert st.launches > 1 and st.hits_dropped == 0, what
    # tallies and statistics
    assert N.array_equal(h, o['hits']), (what, h, o['hits'])
    assert (st.segments, st.hits, st.rays_left) == (o['segments'], o['events'], o['last_energy'].size), what
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-15), (what, a, o['absorbed'])
    assert N.allclose(r, o['received'], rtol=1e-9, atol=1e-15), (what, r, o['received'])
    assert N.isclose(st.energy_left, o['last_energy'].sum(), rtol=1e-9, atol=0.), (what, st.energy_left, o['last_energy'].sum())
    # the surviving rays as multisets: the two rays of one hit start at one point and differ in direction
    mine = N.vstack(last)
    theirs = N.vstack((o['last_vertices'], o['last_directions'], o['last_energy'][None, :]))
    assert mine.shape == theirs.shape, (what, mine.shape, theirs.shape)
    mine, theirs = mine[:, _order(*mine[:6])], theirs[:, _order(*theirs[:6])]
    assert N.allclose(mine[:6], theirs[:6], rtol=1e-9, atol=1e-9), (what, 'survivors', N.abs(mine[:6] - theirs[:6]).max())
    assert N.allclose(mine[6], theirs[6], rtol=1e-9, atol=0.), (what, 'energies of the survivors')
    # the captured hits as multisets, per capturing surface: one entry per hit, whatever it sent on
    H = o['hit_list']
    assert len(hits['surf']) == h[c.captured].sum(), (what, len(hits['surf']), h[c.captured].sum())
    assert nx == 3 * c.W, (what, nx)
    lean = hits['directions'] is None
    for s in c.captured:
        km, kt = N.nonzero(hits['surf'] == s)[0], N.nonzero(H['surf'] == s)[0]
        assert len(km) == len(kt) == h[s], (what, s)
        if lean:
            km, kt = km[_order(*hits['points'][:, km])], kt[_order(*H['points'][:, kt])]
        else:
            km = km[_order(*N.vstack((hits['points'][:, km], hits['directions'][:, km])))]
            kt = kt[_order(*N.vstack((H['points'][:, kt], H['directions'][:, kt])))]
            assert N.allclose(hits['directions'][:, km], H['directions'][:, kt], rtol=1e-9, atol=1e-9), (what, s)
            assert N.allclose(hits['e_in'][km], H['e_in'][kt], rtol=1e-9, atol=0.), (what, s)
        assert N.allclose(hits['points'][:, km], H['points'][:, kt], rtol=1e-9, atol=1e-9), (what, s)
        print('%s: surface %d, largest difference of the absorbed energies %.3g of %.3g' %
              (what, s, N.abs(hits['e_abs'][km] - H['e_abs'][kt]).max() if len(km) else 0., N.abs(H['e_abs'][kt]).max() if len(kt) else 0.))
        # rtol 1e-9 on what a hit absorbed.  Where the surface absorbs nothing the oracle's own figure -- the incident energy less
        # what the rays take along -- is no energy but the rounding of that difference, 0 or a few units in the last place of the
        # incident energy (measured: 2.7e-20 of 3.9e-3, and 0 on the device or the other way round); no relative bound can hold
        # between two such residues, so there both must be residues: at most 8 units in the last place of the incident energy.
        residue = N.abs(H['e_abs'][kt]) <= 8. * 2. ** -52 * H['e_in'][kt]
        assert N.allclose(hits['e_abs'][km][~residue], H['e_abs'][kt][~residue], rtol=1e-9, atol=0.), (what, s)
        assert (N.abs(hits['e_abs'][km][residue]) <= 8. * 2. ** -52 * H['e_in'][kt][residue]).all(), (what, s)
        if c.W:
            got = N.vstack((hits['spectra'][2], hits['spectra'][0], hits['spectra'][1]))[:, km]        # wavelengths, arrived, left
            assert N.allclose(got, H['x'][:, kt], rtol=1e-12, atol=0.), (what, s, N.abs(got - H['x'][:, kt]).max())
    # the flux map against the host histogram of the oracle's hits
    if chart:
        Hm = fcs.host_maps(H, c.frames, {c.map_surf: ('cylinder', False) + CYL_EDGES})[c.map_surf][0]
        assert (Hm > 0).all()
    else:
        Hm = o['maps'][c.map_surf][0]
    assert fm.shape == Hm.shape, what
    assert N.allclose(fm, Hm, rtol=1e-9, atol=1e-15), (what, N.abs(fm - Hm).max(), Hm.max())
    return st


@pytest.mark.parametrize('name', ['slab', 'slab_recv', 'slab_sigma', 'mixed', 'wave', 'source', 'material', 'poly'])
def test_streaming_form_against_the_oracle(ctx, name):
    _check(ctx, name, (name, 'stream'))


def test_flags_0_take_the_streaming_form(ctx):
    """trc_trace_fast without TRC_TRACE_STREAM on a scene that splits rays (256 rays: below the size from which other scenes go to the
    streaming form): the streaming form all the same, never the megakernel, which drops the second ray"""
    st = _check(ctx, 'slab', ('slab', 'flags 0'), stream=None)
    assert st.launches > 1


def test_every_ray_splits_in_the_first_bounce(ctx):
    """16384 rays at normal incidence, lists of 2048 entries to start from: in bounce 0 the search stage hands out a slot per ray
    and the shading kernel a second one per ray"""
    _check(ctx, 'wave_big', ('wave_big', 'TRC_STREAM_ROOM=2048'), TRC_STREAM_ROOM=2048)
    _check(ctx, 'wave_big', ('wave_big', 'default room'))


@pytest.mark.parametrize('name', ['slab_global', 'mixed_global'])
def test_tables_in_global_memory(ctx, name):
    """one surface more with a long optics table: k_s_shade_x<false, .., SPLIT> reads every table from global memory"""
    _check(ctx, name, (name, 'tables in global memory'))


def test_chart_map_on_the_floor(ctx):
    """a flux map in the cylinder chart on a surface of the scene: the SPLIT x CHART instances"""
    _check(ctx, 'slab', ('slab', 'cylinder chart'), chart=True)
    _check(ctx, 'slab_global', ('slab_global', 'cylinder chart'), chart=True)


def test_ray_table_grows(ctx):
    """mixed with lists of 2048 entries to start from: the population grows to 19914 live rays in 23116 slots, so the ray table
    and the lists are grown several times between bounces; without growth the call ends with ERR_CAPACITY"""
    assert sc.ORACLE['mixed'][4] > 4 * 2048
    _check(ctx, 'mixed', ('mixed', 'TRC_STREAM_ROOM=2048'), TRC_STREAM_ROOM=2048)
    _check(ctx, 'mixed', ('mixed', 'TRC_STREAM_ROOM=2048, no pre-assigned chunks'), TRC_STREAM_ROOM=2048, TRC_STREAM_STATIC=0)
    _check(ctx, 'mixed', ('mixed', 'default room again'))


def test_what_stays_with_the_ordered_engine(ctx):
    """the megakernel and calls below 64 rays: ERR_UNSUPPORTED, and the message names trc_trace_ordered"""
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene
    c = sc.case('slab')
    dev = DeviceScene(c.cs, ctx)
    with pytest.raises(_cabi.TracerAmdError) as err:
        dev.trace_fast(c.bundle(), c.reps, c.min_energy, c.seed, keep_last=True, stream=False, last_capacity=1024)
    assert err.value.status == _cabi.ERR_UNSUPPORTED and 'trc_trace_ordered' in str(err.value)
    few = sc.Case('slab', n=40)
    with pytest.raises(_cabi.TracerAmdError) as err:
        dev.trace_fast(few.bundle(), c.reps, c.min_energy, c.seed, keep_last=True, stream=True, last_capacity=1024)
    assert err.value.status == _cabi.ERR_UNSUPPORTED and 'trc_trace_ordered' in str(err.value)
    a, r, h = dev.get_tallies()
    assert not h.any()
    dev.close()


def _surface_hits(asm):
    """[(energies, points) sorted by point] of the assembly's capturing surfaces"""
    out = []
    for s in asm.get_surfaces():
        mgr = s.get_optics_manager()
        if not hasattr(mgr, 'get_all_hits'):
            continue
        e, p = mgr.get_all_hits()
        k = _order(*p)
        out.append((N.asarray(e)[k], N.asarray(p)[:, k]))
    return out


@pytest.fixture(scope='module')
def slab_recv_engines():
    """slab_recv through TracerEngine with the default hit capacity, engine='auto' and engine='ordered' on the same seed"""
    from tracer_amd.tracer_engine import TracerEngine
    c = sc.case('slab_recv')
    engines = []
    for which in ('auto', 'ordered'):
        asm = sc.scene('slab_recv')[0]
        eng = TracerEngine(asm)
        eng.ray_tracer(c.bundle(), reps=c.reps, min_energy=c.min_energy, tree=False, seed=c.seed, engine=which)
        engines.append((eng, asm))
    return engines


def test_engine_captures_more_hits_than_the_default_room(slab_recv_engines):
    """slab_recv through TracerEngine with the default capacity: 2816 captured hits from 256 rays, more than 2 n + 1024.  The call is
    made again with room for them; tallies are taken after that and are not doubled; the tallies, and the hits of the floor, equal
    the ordered engine's.  Room the caller sets is taken literally, and the megakernel still refuses the scene."""
    from tracer_amd.tracer_engine import TracerEngine
    c = sc.case('slab_recv')
    (fast, asm_f), (ordered, asm_o) = slab_recv_engines
    assert fast.stats['engine'] == 'fast' and fast.stats['form'] == 'stream' and ordered.stats['engine'] == 'ordered'
    (af, rf, hf), (ao, ro, ho) = fast.get_tallies(), ordered.get_tallies()
    assert N.array_equal(hf, ho) and list(hf) == sc.ORACLE['slab_recv'][0]
    assert N.allclose(af, ao, rtol=1e-9, atol=1e-15) and N.allclose(rf, ro, rtol=1e-9, atol=1e-15)
    Hf, Ho = _surface_hits(asm_f), _surface_hits(asm_o)
    assert len(Hf) == len(Ho) == 3 and sum(len(e) for e, p in Hf) == sc.ORACLE['slab_recv'][3]
    (ef, pf), (eo, po) = Hf[2], Ho[2]
    assert pf.shape == po.shape == (3, 768) and N.allclose(pf, po, rtol=1e-9, atol=1e-9) and N.allclose(ef, eo, rtol=1e-9, atol=1e-15)
    eng = TracerEngine(sc.scene('slab_recv')[0])
    with pytest.raises(RuntimeError) as err:
        eng.ray_tracer(c.bundle(), reps=c.reps, min_energy=c.min_energy, tree=False, seed=c.seed, engine='fast', fast_kernel='megakernel')
    assert 'trc_trace_ordered' in str(err.value)
    # room the caller sets is not made larger and the call is not made again: 2^19 rays capture 5.7e6 hits, beyond 1000 entries and
    # what the buffer's open chunks may leave unused (1.3e6), so the library drops hits
    big = sc.Case('slab_recv', n=1 << 19)
    with pytest.raises(RuntimeError) as err:
        eng.ray_tracer(big.bundle(), reps=c.reps, min_energy=c.min_energy, tree=False, seed=c.seed, hit_capacity=1000)
    assert 'hits were not captured' in str(err.value)


def test_a_hit_capacity_of_1000_raises():
    """slab_recv (256 rays, 2816 captured hits) through ray_tracer(tree=False, hit_capacity=1000) raises 'hits were not captured':
    room the caller sets is taken literally for a scene that splits rays, although the room the library leaves beside a buffer for
    the unused ends of its chunks (64 entries for each of 20480 waves) would have held these hits"""
    from tracer_amd.tracer_engine import TracerEngine
    c = sc.case('slab_recv')
    eng = TracerEngine(sc.scene('slab_recv')[0])
    with pytest.raises(RuntimeError) as err:
        eng.ray_tracer(c.bundle(), reps=c.reps, min_energy=c.min_energy, tree=False, seed=c.seed, hit_capacity=1000)
    assert 'hits were not captured' in str(err.value)


def test_accountants_of_every_surface_equal_the_ordered_engine(slab_recv_engines):
    """get_all_hits() of the three surfaces of slab_recv, fast engine against ordered engine on the same seed, as multisets: a hit
    that sends two rays on is one entry of its surface's accountants -- its point once, and what neither ray takes along as the
    absorbed energy -- in both engines (1024 + 1024 + 768 entries)"""
    (fast, asm_f), (ordered, asm_o) = slab_recv_engines
    Hf, Ho = _surface_hits(asm_f), _surface_hits(asm_o)
    print('entries per surface: fast %s, ordered %s' % ([len(e) for e, p in Hf], [len(e) for e, p in Ho]))
    assert len(Hf) == len(Ho) == 3 and [len(e) for e, p in Ho] == sc.ORACLE['slab_recv'][0]
    for (ef, pf), (eo, po) in zip(Hf, Ho):
        assert pf.shape == po.shape and N.allclose(pf, po, rtol=1e-9, atol=1e-9)
        assert N.allclose(ef, eo, rtol=1e-9, atol=1e-15)
    # ... and each of them equals the oracle's hits of its surface: their points, and what they absorbed
    H = sc.reference('slab_recv')['hit_list']
    for s, ((ef, pf), (eo, po)) in enumerate(zip(Hf, Ho)):
        k = N.nonzero(H['surf'] == s)[0]
        k = k[_order(*H['points'][:, k])]
        for what, e, p in (('fast', ef, pf), ('ordered', eo, po)):
            assert p.shape == (3, len(k)) and N.allclose(p, H['points'][:, k], rtol=1e-9, atol=1e-9), (what, s)
            assert N.allclose(e, H['e_abs'][k], rtol=1e-9, atol=1e-15), (what, s)


def test_engines_agree_on_the_mixed_scene():
    """mixed through TracerEngine: tallies and transfer matrix of the fast and the ordered engine (19914 rays left from 256)"""
    from tracer_amd.tracer_engine import TracerEngine
    c = sc.case('mixed')
    got = []
    for which in ('auto', 'ordered'):
        eng = TracerEngine(sc.scene('mixed')[0])
        eng.enable_transfer_matrix()
        v, d = eng.ray_tracer(c.bundle(), reps=c.reps, min_energy=c.min_energy, tree=False, seed=c.seed, engine=which)
        got.append((eng.stats['engine'], eng.get_tallies(), eng.get_transfer_matrix(), v.shape[1]))
    (ef, (af, rf, hf), Tf, nf), (eo, (ao, ro, ho), To, no) = got
    assert (ef, eo) == ('fast', 'ordered') and nf == no == sc.ORACLE['mixed'][2]
    assert N.array_equal(hf, ho) and list(hf) == sc.ORACLE['mixed'][0]
    assert N.allclose(af, ao, rtol=1e-9, atol=1e-15) and N.allclose(rf, ro, rtol=1e-9, atol=1e-15)
    assert Tf.shape == To.shape and To.sum() > 0. and N.allclose(Tf, To, rtol=1e-9, atol=1e-15)
    # ... and with the oracle's trace: every segment once (the bundle's energy, 1, leaves the source row)
    Tr = sc.transfer_of_levels(sc.reference('mixed')['levels'], c.cs.n_surf)
    assert N.isclose(Tr[-1].sum(), 1., rtol=1e-12) and N.isclose(To[-1].sum(), 1., rtol=1e-9) and N.isclose(Tf[-1].sum(), 1., rtol=1e-9)
    assert N.allclose(To, Tr, rtol=1e-9, atol=1e-15) and N.allclose(Tf, Tr, rtol=1e-9, atol=1e-15)
