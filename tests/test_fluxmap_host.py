"""
What the flux-map tests of the device (test_gpu_fluxmap.py) take for granted about their inputs, checked without one: the host
reference alone -- hits of the cavity traced by oracle.engine, projected and binned by numpy -- fills the maps, leaves part of
the hits of the clipped maps outside and accounts for every surface's absorbed energy; the hand-written table of the hits on
edges is what numpy.histogram2d says; and the bins chosen for the three storage regimes lie where the streaming engine's byte
limits put them.
"""
import numpy as N
import pytest

import fluxmap_scene as fs


@pytest.mark.parametrize('regime', ['small', 'middle', 'large'])
def test_host_histograms_of_the_cavity_meet_the_conditions_on_the_inputs(regime):
    from tracer_amd.scene import compile_scene
    from oracle import engine
    asm, objs, T = fs.cavity()
    cs = compile_scene(asm)
    n = 20000               # a tenth of the smallest device case: what is filled here is filled there
    o = engine.trace_from_compiled(cs, fs.source(n, T, seed=11).source_args(), 12, 1e-10)
    frames = [s._temp_frame for s in cs.surfaces]
    for f in frames:        # no frame is axis aligned
        assert (N.abs(f[:3, :3]) > 1e-3).sum() >= 8 and N.abs(f[:3, 3]).min() > 1.
    edges = fs.map_edges(regime)
    assert sorted(edges) == sorted(fs.MAPPED) and all(len(u) != len(v) for u, v in edges.values())
    assert not N.allclose(N.diff(edges[fs.FLOOR][0]), N.diff(edges[fs.FLOOR][0])[0])
    ref = fs.host_maps(fs.hits_of_levels(o['levels']), frames, edges)
    fs.check_inputs(ref, edges)
    for s, (H, e_out, n_out, n_hits) in ref.items():
        assert n_hits == o['hits'][s] > 0.05 * n
        assert N.isclose(H.sum() + e_out, o['absorbed'][s], rtol=1e-12)
        if s not in fs.CLIPPED:
            assert n_out == 0
    # the mirror wall is hit again by rays it has reflected before, and the unmapped surfaces take part
    assert o['hits'][3] > 0.05 * n and o['hits'][fs.MOVING] > 0.02 * n and len(o['levels']) > 8


def test_regime_bins_against_the_byte_limits_of_the_streaming_engine():
    """The arithmetic of fluxmap_scene.FLOOR_BINS, so that a change of the maps there cannot move a case out of its regime unnoticed:
    bins * 8 + 16 plus the tables against the 78 KiB and 150 KiB of trc_stream_form_shade, restated here.  This says nothing about the
    library: that the regimes are reached on the device is asserted there (test_gpu_fluxmap.py, from the launches the library
    reports).  The tables: below 8 KiB for seven surfaces (fluxmap_scene.py); the scene has no optics or geometry tables (n_extra = 0)."""
    from tracer_amd.scene import compile_scene
    assert len(compile_scene(fs.cavity()[0]).extra) == 0
    tables = 8 * 1024
    total = dict((k, (nu * nv + fs.OTHER_BINS) * 8 + 16) for k, (nu, nv) in fs.FLOOR_BINS.items())
    others = fs.map_edges('small')
    assert sum((len(u) - 1) * (len(v) - 1) for s, (u, v) in others.items() if s != fs.FLOOR) == fs.OTHER_BINS
    assert total['small'] // 8 < 4000 and total['small'] + tables <= 78 * 1024
    assert 78 * 1024 < total['middle'] and total['middle'] + tables <= 150 * 1024
    assert 150 * 1024 < total['large']


def test_hand_written_edge_table_is_numpys():
    x, y, e, want, outside = fs.edge_cases()
    H = N.histogram2d(x, y, bins=[fs.EDGE_U, fs.EDGE_V], weights=e)[0]
    assert N.array_equal(H, want)
    assert outside == e.sum() - want.sum() > 0 and (want > 0).mean() >= 0.5
