"""
What the tests of the shading kernel instances (test_gpu_shade_instances.py) take for granted about their cases, checked without
a device from the oracle and the restated sums of stream_form_shade alone (shade_cases.py): every case is predicted to select
the instances it is there for, with its byte sum on the intended side of the limit; its rays hit every optics kind of its classes,
its curved surfaces, its captured surfaces inside and outside the map; some rays are culled on the way and some survive; and no
ray is near a tie -- two surfaces at nearly the same distance, an energy nearly at min_energy -- so that the device tests exclude
no ray at all.  This says nothing about the library: which instances ran on a device is recorded in profiles/shade_instances.txt.
"""
import os
import subprocess

import numpy as N
import pytest

import shade_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hostcheck():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])          # (the wavelength sampler of the SPEC cases)


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_case_selects_its_instances_and_exercises_them(hostcheck, name):
    c = sc.case(name)
    o = sc.reference(name)
    opt, gm = sc._names('OPT_'), sc._names('GM_')
    # the prediction: the case's targets among what stream_form_shade would launch, each on its side of its limit
    for inst in c.targets:
        assert inst in c.instances, (inst, sorted(c.instances))
        total, limit, in_lds, bins_in_lds = c.instances[inst]
        print('%s: %s sums %d bytes against %d: tables %s, bins %s' % (name, inst, total, limit, 'in LDS' if in_lds else 'global',
                                                                      'in LDS' if bins_in_lds else 'global'))
        assert in_lds == (total <= limit) and in_lds == ('global' not in name) and bins_in_lds == in_lds
    # every optics kind listed for the case is hit at least 30 times; curved surfaces take more than a tenth of the hits
    by_kind = {}
    for i in range(c.cs.n_surf):
        k = opt[c.cs.descs[i].optics_kind]
        by_kind[k] = by_kind.get(k, 0) + int(o['hits'][i])
    for k in sc.KINDS_HIT[c.kind]:
        assert by_kind.get(k, 0) >= 30, (k, by_kind)
    if c.kind in ('simple', 'general'):          # the general class of the case: the surfaces with an incidence-angle modifier / the panes
        general = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_GENERAL]
        assert len(general) == 2 and all(o['hits'][i] >= 30 for i in general)
    flat = all(gm[c.cs.descs[i].gm_kind] in sc.FLAT_KINDS for i in range(c.cs.n_surf))
    assert flat == (c.kind not in ('curved', 'general'))
    if not flat:
        curved = sum(int(o['hits'][i]) for i in range(c.cs.n_surf) if gm[c.cs.descs[i].gm_kind] in sc.CURVED_GM)
        assert curved > 0.1 * o['hits'].sum() and all(o['hits'][i] >= 30 for i in range(c.cs.n_surf) if gm[c.cs.descs[i].gm_kind] in sc.CURVED_GM)
    if c.n_fill:        # the fillers are hit through the gaps of the floor, a few hits each: sums added per lane
        assert (o['hits'][:c.n_fill] > 0).sum() > 100 and o['hits'][:c.n_fill].max() < 16
    # survivors, and rays culled before the last repetition
    assert len(o['levels']) == sc.REPS + 1 and o['last_energy'].size > 50
    assert sum(L['vertices'].shape[1] - L['n_live'] for L in o['levels'][1:-1]) > 50
    # the captured surfaces: the mapped tile inside and outside its map, the wall captured in full
    H, e_out, n_out, n_hits = o['maps'][c.map_surf]
    assert n_hits == o['hits'][c.map_surf] and 30 <= n_out <= n_hits - 30 and (H > 0).mean() > 0.3
    assert N.isclose(H.sum() + e_out, o['absorbed'][c.map_surf], rtol=1e-12)
    assert o['hits'][c.full_surf] > 300
    for f in c.frames[c.n_fill:]:       # no frame of the room is axis aligned
        assert (N.abs(f[:3, :3]) > 1e-3).sum() >= 8
    # SPEC: rays that meet the mirror class first and a wavelength-reading surface second, and rays that meet one first
    if c.spec:
        reads = [i for i in range(c.cs.n_surf) if opt[c.cs.descs[i].optics_kind] in ('OPT_REFLECTIVE_SPECTRAL', 'OPT_FRESNEL_CONDUCTOR')]
        mirror = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_MIRROR]
        L1, L2 = o['levels'][1], o['levels'][2]
        if c.kind != 'simple':
            assert N.isin(L1['surf'], reads).sum() > 100
            assert (N.isin(L2['surf'], reads) & N.isin(L1['surf'][L2['parents']], mirror)).sum() > 100
        if c.kind == 'general':     # ... and rays that meet a pane of the general class first: the wavelength k_s_shade hands on is read
            panes = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_GENERAL]
            assert (N.isin(L2['surf'], reads) & N.isin(L1['surf'][L2['parents']], panes)).sum() > 50
    if c.carry:         # the periodic pane moves rays that go on and survive: the shift is in what the device is compared with
        periodic = [i for i in range(c.cs.n_surf) if opt[c.cs.descs[i].optics_kind] == 'OPT_PERIODIC_BOUNDARY']
        last = o['levels'][-1]
        assert o['hits'][periodic[0]] > 300 and (N.isin(last['surf'][:last['n_live']], periodic)).sum() >= 5        # (each survivor is compared on its own: a handful is enough)
    # no near tie: the cap on rays a device test may exclude is zero, and the reference stays within it
    gap, e_gap = sc.near_ties(name)
    print('%s: smallest gap between nearest and second-nearest surface %.3g, of an energy from min_energy %.3g (relative)' % (name, gap, e_gap))
    assert gap > 1e-9 and e_gap > 1e-9


def test_cases_cover_every_instance_that_can_be_selected():
    """26 instances; every one is the target of a case"""
    targets = set(t for v in sc.CASES.values() for t in v[5])
    assert len(sc.ALL_INSTANCES) == 26 and targets == set(sc.ALL_INSTANCES)
    assert set(sc.GIVEN) <= set(sc.CASES) and all(not sc.CASES[n][3] and not sc.CASES[n][4] for n in sc.GIVEN)
