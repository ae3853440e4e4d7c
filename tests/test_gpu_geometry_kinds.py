"""
GPU tests of the 30 geometry kinds inside the engines, run with -m gpu on the MI355X box.

test_gpu_parity.py holds every kind to the fixtures one surface at a time (k_gm_intersect, k_gm_normals).  Here every call of
geometry_cases.py -- a gallery of every bounded kind, the same over fillers that push its tables out of LDS, a packed scene of flat
kinds only, every kind with the seven unbounded ones inside an absorbing sphere, and 30 scenes in which a kind is the widest of its
table; test_geometry_cases_host.py checks the selection and the conditions on the inputs without a device -- is traced by the
streaming form or by the megakernel and held to oracle.engine on the same Philox streams by the assertions of
test_gpu_shade_instances._check, unchanged: hit counts per surface exactly, the call's statistics, absorbed and received energy per
surface, every surviving ray, every captured hit (lean and full), and the flux map against the host histogram of the oracle's hits.
No ray is excluded.  The ordered engine traces the mixed scenes under a built tree, with and without accel, and under a tree too
deep for its LDS stack, and is held to the oracle level by level.
"""
import numpy as N
import pytest

import geometry_cases as G
from test_gpu_parity import RT, AT
from test_gpu_shade_instances import _check, ctx        # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu


def _ids(name):
    c = G.CALL[name]
    return '%s[%s]' % (name, '+'.join(t.replace(' ', '') for t in c.targets))


@pytest.mark.parametrize('name', [c.name for c in G.CALLS], ids=_ids)
def test_fast_engine_call_against_the_oracle(ctx, name):
    c = G.CALL[name]
    s = G.scene(c.scene)
    _check(ctx, c, G.reference(c.scene, c.src), c.given, c.stream, (name, 'stream' if c.stream else 'megakernel'), accel=c.accel, kd=s.tree(c.kd),
           scene_knobs=dict(c.scene_env), reps=s.reps, **dict(c.env))


@pytest.mark.parametrize('scn,kd,accel,kernel', G.ORDERED, ids=['%s/%s/accel=%d[%s]' % (scn, kd if kd == 'built' else 'deep%d' % kd[1], accel, k.replace(' ', ''))
                                                                 for scn, kd, accel, k in G.ORDERED])
def test_ordered_engine_against_the_oracle(ctx, scn, kd, accel, kernel):
    """every level equals the oracle's in order: parents, surfaces, live count, vertices, directions and energies, then the tallies
    and the segments (the assertions of test_gpu_mega_instances.test_ordered_engine_on_the_chains, at its tolerances)"""
    from tracer_amd.scene import DeviceScene
    s = G.scene(scn)
    c = G.CALL[scn + '/given']
    dev = DeviceScene(s.cs, ctx)
    dev.set_kdtree(s.tree(kd))
    res, stats = dev.trace_ordered(c.bundle(True), s.reps, c.min_energy, G.SEED, accel=accel)
    levels = [res.level(k) for k in range(res.num_levels())]
    a, r, h = dev.get_tallies()
    res.close()
    dev.close()
    o = G.reference(scn, 'given')
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
