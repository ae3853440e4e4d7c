"""
GPU tests of the persistent megakernel (k_trace_coop<512 | 256, SPEC, SUN, CHART>, k_trace_fast<256, SPEC, SUN, CHART>: 24 compiled
kernels, one picked per call by mega_plan), run with -m gpu on the MI355X box.

Every case of mega_cases.py -- a scene, a source or given rays, a Kd-tree or none, a chart map or none;
test_mega_cases_host.py checks the selection, the branch the case is there for and the conditions on the inputs without a device --
is traced with stream=False and held to oracle.engine on the same Philox streams by the assertions of
test_gpu_shade_instances._check: hit counts per surface exactly, the call's statistics, every surviving ray, every captured hit (a
lean and a full capture), the flux map -- and a second one in a cylinder chart -- against the host histogram of the oracle's hits.
No ray is excluded.  The cases reach both thread counts of the cooperative kernel, its packed Kd walk down to the last stack row, the
drains in the middle of a search, always-relevant lists and leaves beyond 32 entries, unbounded planes on both sides of an exact
tie, ray counts around a wave, and the three staging forms of k_trace_fast with its float64 walk down to the last stack entry.  A
tree one level deeper is refused by the host.  The ordered engine's generic search, selected by trees too deep for its LDS stack,
is held to the oracle level by level on the same hand-made trees.  Which instances these calls launched is recorded in
profiles/mega_instances.txt from a kernel trace of this file.
"""
import numpy as N
import pytest

import mega_cases as M
from test_gpu_parity import RT, AT
from test_gpu_shade_instances import _check, ctx        # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu


def _ids(name):
    c = M.CASE[name]
    return '%s[%s]' % (name, '+'.join([c.target.replace(' ', '')] + [b.replace(' ', '') for b in c.branches]))


def _reference(c):
    """the oracle's trace of the case; a SPEC case's wavelengths are the pending bundle's own, drawn on the device"""
    return M.reference(c, wavelengths=N.array(c.source().get_wavelengths()) if c.spec else None)


@pytest.mark.parametrize('name', [c.name for c in M.CASES], ids=_ids)
def test_megakernel_case_against_the_oracle(ctx, name):
    c = M.CASE[name]
    _check(ctx, c, _reference(c), c.given, False, (name, 'megakernel'), accel=c.accel, kd=M.tree(c), chart=c.chart_map, reps=c.reps)


def test_tree_deeper_than_the_stack_is_refused(ctx):
    """chain(33): trc_scene_set_kdtree refuses it before any launch, and the scene goes on without a tree"""
    from tracer_amd import _cabi
    from tracer_amd.scene import DeviceScene
    c = M.CASE['row/boxes']
    dev = DeviceScene(c.cs, ctx)
    with pytest.raises(_cabi.TracerAmdError) as err:
        dev.set_kdtree(M.scene('row').chain(M.REFUSED_DEPTH))
    assert err.value.status == _cabi.ERR_UNSUPPORTED
    assert str(err.value) == 'Kd-tree depth %d exceeds the traversal stack (%d)' % (M.REFUSED_DEPTH, M.TRC_KD_STACK)
    st, last = dev.trace_fast(c.bundle(True), c.reps, c.min_energy, M.SEED, accel=True, keep_last=True, stream=False)
    a, r, h = dev.get_tallies()
    dev.close()
    o = M.reference(c)
    assert N.array_equal(h, o['hits']) and (st.segments, st.hits, st.rays_left) == (o['segments'], o['events'], o['last_energy'].size)
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-12) and N.allclose(r, o['received'], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('depth,chart,kernel', M.ORDERED, ids=[k.replace(' ', '') for D, ch, k in M.ORDERED])
def test_ordered_engine_on_the_chains(ctx, depth, chart, kernel):
    """the row under chain(22) -- the deepest tree the ordered engine's LDS stack takes, k_ord_bounce<1> -- and under chain(23), its
    generic search, without and with a chart map on the scene: every level equals the oracle's in order, parents, surfaces, live count,
    vertices, directions and energies (the assertions of test_engines_vs_oracle_monte_carlo, at its tolerances)"""
    from tracer_amd.scene import DeviceScene
    c = M.CASE['row/boxes']
    s = M.scene('row')
    tree = s.chain(depth)
    assert (M.S.kd_depth(tree.flat()) + 2 <= M.ORD_STACK_DEPTH) == kernel.startswith('k_ord_bounce<1,')
    dev = DeviceScene(c.cs, ctx)
    dev.set_kdtree(tree)
    if chart:
        dev.set_fluxmap(s.terminal, N.linspace(0., 1.8, 7), N.linspace(0., 2. * N.pi, 9), chart='polar')
    res, stats = dev.trace_ordered(c.bundle(True), c.reps, c.min_energy, M.SEED, accel=True)
    levels = [res.level(k) for k in range(res.num_levels())]
    a, r, h = dev.get_tallies()
    fm = dev.get_fluxmap(s.terminal) if chart else None
    res.close()
    dev.close()
    o = M.reference(c)
    assert [l['vertices'].shape[1] for l in levels] == [l['vertices'].shape[1] for l in o['levels']]
    for k in range(1, len(levels)):
        L, O = levels[k], o['levels'][k]
        assert N.array_equal(L['parents'], O['parents']), k
        assert N.array_equal(L['surf'], O['surf']), k
        assert L['n_live'] == O['n_live'], k
        assert N.allclose(L['vertices'], O['vertices'], rtol=RT, atol=AT), k
        assert N.allclose(L['directions'], O['directions'], rtol=1e-8, atol=1e-8), k
        assert N.allclose(L['energy'], O['energy'], rtol=RT, atol=1e-12), k
    assert N.array_equal(h, o['hits'])
    assert N.allclose(a, o['absorbed'], rtol=1e-9, atol=1e-9)
    assert stats.segments == o['segments']
    if chart:
        import fluxmap_chart_scene as fc
        Hc, e_out, n_out, n_hits, n_edge = fc.host_maps(o['hit_list'], s.frames, {s.terminal: ('polar', False, N.linspace(0., 1.8, 7), N.linspace(0., 2. * N.pi, 9))})[s.terminal]
        assert n_hits == h[s.terminal] and n_edge == 0 and Hc.max() > 0.
        assert N.allclose(fm, Hc, rtol=1e-9, atol=1e-9 * Hc.max())


def test_kd_tree_set_replaced_dropped_and_refused(ctx):
    """The row with 2e4 rays through the ordered engine, the megakernel and the streaming form in five states of the scene's
    Kd-tree: chain(24) set; chain(5), of other leaves, in its place; set_kdtree(None); update_frames with the same poses, which
    drops a tree set before it; the refused chain(33) after a tree.  A tree changes no ray: every state gives every engine the
    per-surface hit counts of the first and its energies to 1e-9.  Without a tree the ordered engine refuses accel=True (it is
    then traced without); the fast engine's forms search all boxes or their own grid."""
    from tracer_amd import _cabi
    from tracer_amd.ray_bundle import RayBundle
    from tracer_amd.scene import DeviceScene
    c, s, n = M.CASE['row/boxes'], M.scene('row'), 20000
    rng = N.random.RandomState(M.SEED)
    up = N.arange(n) % 2 == 0
    rad, ph = M.ROW_BEAM * N.sqrt(rng.uniform(size=n)), rng.uniform(0., 2. * N.pi, n)
    v, d, e, _ = s.to_global(N.vstack((N.where(up, -0.5, M.ROW_PLATES * M.ROW_PITCH + 0.5), rad * N.cos(ph), rad * N.sin(ph))),
                             N.vstack((N.where(up, 1., -1.), 0.025 * rng.uniform(-1., 1., n), 0.025 * rng.uniform(-1., 1., n))))
    dev = DeviceScene(c.cs, ctx)
    dev.set_hit_capacity(n * (c.reps + 1))

    def trace(has_tree):
        out = {}
        for form in ('ordered', 'megakernel', 'stream'):
            dev.reset_tallies()
            b = RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())
            if form == 'ordered':
                if not has_tree:
                    with pytest.raises(_cabi.TracerAmdError) as err:
                        dev.trace_ordered(b, c.reps, c.min_energy, M.SEED, accel=True)
                    assert err.value.status == _cabi.ERR_INVALID
                res, st = dev.trace_ordered(b, c.reps, c.min_energy, M.SEED, accel=has_tree)
                res.close()
            else:
                dev.trace_fast(b, c.reps, c.min_energy, M.SEED, accel=True, stream=form == 'stream')
            out[form] = [N.array(x) for x in dev.get_tallies()]
        return out

    def refused():
        dev.set_kdtree(s.chain(7))
        with pytest.raises(_cabi.TracerAmdError) as err:
            dev.set_kdtree(s.chain(M.REFUSED_DEPTH))
        assert err.value.status == _cabi.ERR_UNSUPPORTED

    states = [('chain(24)', lambda: dev.set_kdtree(s.chain(M.COOP_MAX_DEPTH)), True), ('chain(5)', lambda: dev.set_kdtree(s.chain(5)), True),
              ('no tree', lambda: dev.set_kdtree(None), False), ('update_frames', lambda: (dev.set_kdtree(s.chain(9)), dev.update_frames(c.cs)), False),
              ('refused', refused, False)]
    first = None
    for name, enter, has_tree in states:
        enter()
        got = trace(has_tree)
        first = first or got
        for form, (a, r, h) in got.items():
            a0, r0, h0 = first[form]
            assert h0.sum() > n and N.array_equal(h, h0), (name, form)
            assert N.allclose(a, a0, rtol=1e-9, atol=1e-12) and N.allclose(r, r0, rtol=1e-9, atol=1e-12), (name, form)
    dev.close()
