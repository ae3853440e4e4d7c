"""
What the tests of the geometry kinds inside the engines (test_gpu_geometry_kinds.py) take for granted about their scenes and calls,
checked without a device from the oracle and the host-compiled check library alone (geometry_cases.py): the restated parameter
counts and record strides are the library's; for the live rays of every level of every reference, the single-precision searches
built from the kinds' boxes -- all boxes, the trees of the calls, the uniform grid, the large grid -- find the surface the oracle's
next level records, at the brute-force distance, with no mismatch at all; no ray is near a tie, so that the device tests exclude no
ray; every surface is hit, every kind is hit late in a trace and is left by rays that hit again; every call selects the kernel
instances it names, and between them the calls select the FLAT and the general instance of every search kernel, tables in LDS and
in global memory, both lean shading classes and both searches of the ordered engine; and the footprint maps lose no hit.

Every assertion here is a condition on the inputs: a scene that fails one gets another pose or seed, never a weaker assertion.
"""
import ctypes as C

import numpy as N
import pytest

import geometry_cases as G
import mega_cases as M
import search_cases as S
import shade_cases as sc

MIXED = ('gallery', 'flats', 'open')
REFS = sorted(set((c.scene, c.src) for c in G.CALLS))
MIN_LEFT = 50           # rays that go from a copy of the kind to a next hit, alone/<kind>
_ip = C.POINTER(C.c_int)


def _kinds_of(s, surfaces):
    return set(s.kinds[i] for i in surfaces if s.makers[i] in G.MAKERS)


def test_parameter_counts_and_strides_are_the_librarys():
    """NPARAMS is trc_gm_nparams for all 30 kinds; the stride of every scene is the one trc_scene_facts_fill reads off the library's own
    table; every alone/<kind> has the stride of its kind, the gallery that of SPHERE_CUT, `open` that of PARAB_RECT_OFFAXIS"""
    hc = S.hostcheck()[0]
    gm = sc._names('GM_')
    assert sorted(gm.values()) == sorted(G.NPARAMS) and len(G.NPARAMS) == 30
    for number, name in sorted(gm.items()):
        assert hc.hc_gm_nparams(number) == G.NPARAMS[name], name
    assert hc.hc_gm_nparams(len(gm)) == -1 and hc.hc_gm_nparams(-1) == -1
    for name in G.SCENES:
        s = G.scene(name)
        assert s.facts(None)['stride'] == s.stride == sc.record_stride(s.cs), name
        assert s.facts(None)['n_unbounded'] == len(s.unbounded) and s.facts(None)['all_flat'] == int(s.flat), name
        for fr in s.frames:         # no frame is axis aligned
            assert (N.abs(fr[:3, :3]) > 1e-3).sum() >= 8, name
    for name in G.ALONE:
        kind = 'GM_' + name[len('alone/'):]
        s = G.scene(name)
        assert s.kinds == [kind, kind, 'GM_SPHERE'] and s.stride == (G.REC_HDR + G.NPARAMS[kind]) | 1, name
    assert len(G.ALONE) == 30 and G.scene('gallery').stride == 29 == G.scene('gallery-full').stride and G.scene('open').stride == 31
    assert G.scene('flats').flat and len(G.scene('open').unbounded) == 7 == len(G.UNBOUNDED)
    assert set(G.scene('open').kinds) == set(G.NPARAMS) and _kinds_of(G.scene('gallery'), range(60)) == set(G.NPARAMS) - set(G.UNBOUNDED)


def _search(s, which, f, v, d):
    """(t, surface) of a search of the check library: 'brute', 'f32' (all boxes, or the tree `f`), 'grid', 'grid32'; None: no such grid"""
    hc = S.hostcheck()[0]
    n = v.shape[1]
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    head = [s.cs.n_surf, s.cs.descs, S._ptr(extra)]
    cols = [C.c_long(n)] + [S._ptr(N.ascontiguousarray(r)) for r in list(v) + list(d)]
    t, k, st = N.zeros(n), N.zeros(n, dtype=N.int32), N.zeros(8)
    if which == 'brute':
        rc = hc.hc_nearest(*(head + [None] + cols + [S._ptr(t), k.ctypes.data_as(_ip), None, None]))
    elif which == 'f32':
        kd = S.kd_desc(f) if f is not None else None
        rc = hc.hc_nearest32(*(head + [C.byref(kd) if kd is not None else None] + cols + [S._ptr(t), k.ctypes.data_as(_ip)]))
    else:
        rc = getattr(hc, 'hc_nearest_' + which)(*(head + cols + [S._ptr(t), k.ctypes.data_as(_ip), S._ptr(st)]))
        if rc == -2:
            return None
    assert rc == 0, (which, rc)
    return t, k


_conditions = {}


def conditions(scn, src):
    """the near ties of a reference, once per reference"""
    if (scn, src) not in _conditions:
        s = G.scene(scn)
        _conditions[scn, src] = sc.near_ties(None, given=(s.cs, G.reference(scn, src), s.min_energy(src)))
    return _conditions[scn, src]


@pytest.mark.parametrize('scn,src', REFS, ids=['%s:%s' % k for k in REFS])
def test_searches_find_the_oracles_surface_for_every_live_ray(scn, src):
    """trc_nearest_accel32 over all boxes, over the built tree and over the deep one, the uniform grid with its DDA, and the large grid
    of the scenes that are forced onto it: the surface of the oracle's next level (or none) and the brute-force distance, for the
    live rays of every level that is traced on.  Zero mismatches; and no near tie"""
    s = G.scene(scn)
    trees = {'all boxes': None}
    if any(c.kd == 'built' for c in G.CALLS if c.scene == scn) or scn in MIXED:
        trees['built tree'] = s.kdtree().flat()
    if scn in MIXED:
        trees['deep tree'] = s.deep_tree(G.DEEP[1]).flat()
        assert S.kd_depth(trees['deep tree']) == G.DEEP[1] == M.ORD_STACK_DEPTH - 1 and S.kd_depth(trees['built tree']) + 2 <= M.ORD_STACK_DEPTH
    for f in trees.values():
        if f is not None:           # every surface is listed in a leaf or always relevant, the unbounded ones always
            assert set(f['leaf_surfs'].tolist()) | set(f['always_relevant'].tolist()) == set(range(s.cs.n_surf))
            assert set(s.unbounded) <= set(f['always_relevant'].tolist())
    forced = any(dict(c.scene_env).get('TRC_GRID_FORCE32') for c in G.CALLS if (c.scene, c.src) == (scn, src))
    counts, total = [], 0
    for v, d, hit in G.levels(scn, src):
        tb, sb = _search(s, 'brute', None, v, d)
        bad = int((sb != hit).sum())
        assert bad == 0, (scn, src, 'brute force against the oracle', [(s.makers[a], s.makers[b]) for a, b in zip(hit[sb != hit][:5], sb[sb != hit][:5])])
        got = dict((name, _search(s, 'f32', f, v, d)) for name, f in trees.items())
        got['grid'] = _search(s, 'grid', None, v, d)
        assert got['grid'] is not None
        if forced:
            got['large grid'] = _search(s, 'grid32', None, v, d)
            assert got['large grid'] is not None
        for name, (t, k) in got.items():
            wrong = N.nonzero((k != hit) | ((t != tb) & (sb >= 0)))[0]
            assert len(wrong) == 0, (scn, src, name, len(wrong), wrong[:5], [s.makers[i] for i in hit[wrong[:5]]])
        counts.append(len(hit))
        total += len(hit)
    gap, e_gap = conditions(scn, src)
    print('%s, %s rays: 0 mismatches of %s live rays per level (%d) in %s; smallest gap between nearest and second-nearest surface %.3g, of an '
          'energy from min_energy %.3g (relative)' % (scn, src, counts, total, ', '.join(sorted(got)), gap, e_gap))
    assert total >= s.n_rays and gap > 1e-9 and e_gap > 1e-9


@pytest.mark.parametrize('scn', MIXED)
def test_oriented_boxes_reject_no_hit_of_the_traced_rays(scn):
    """trc_obb_hit32 (float32, the candidate test in front of every exact test) on the rays of every level of the reference, those
    that leave a surface included: a ray that the exact float64 test of a surface accepts passes that surface's oriented box"""
    hc = S.hostcheck()[0]
    hc.hc_obb.restype = C.c_long
    s = G.scene(scn)
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    lv = G.levels(scn, 'given')
    v, d = [N.ascontiguousarray(N.hstack([L[k] for L in lv])) for k in (0, 1)]
    hit = N.concatenate([L[2] for L in lv])
    leaving = sum(len(L[2]) for L in lv[1:])
    tested = 0
    for i in range(s.cs.n_surf):
        passed = C.c_long(0)
        bad = hc.hc_obb(C.byref(s.cs.descs[i]), S._ptr(extra), C.c_long(v.shape[1]), *([S._ptr(N.ascontiguousarray(r)) for r in list(v) + list(d)] + [C.byref(passed)]))
        assert bad == 0, (scn, i, s.makers[i], bad)
        assert (passed.value == -1) == (i in s.unbounded) and (i in s.unbounded or passed.value >= (hit == i).sum()), (scn, i, s.makers[i])
        tested += int((hit == i).sum()) if i not in s.unbounded else 0
    print('%s: %d rays (%d of them leave a surface), %d hits on bounded surfaces' % (scn, v.shape[1], leaving, tested))
    assert leaving >= 1000 and tested >= 1000


def _left(s, o):
    """{surface: rays that leave it alive and hit something at the next level}"""
    lv = o['levels']
    out = N.zeros(s.cs.n_surf, dtype=int)
    for L, nxt in zip(lv[1:-1], lv[2:]):
        N.add.at(out, N.asarray(L['surf'])[nxt['parents']], 1)
    return out


def test_every_kind_is_hit_late_and_left():
    """the given-ray references of the mixed scenes: every surface is hit; every kind is hit at the third interaction or later; every
    kind but the hex dish (it ends every ray) is left by rays that hit again -- from a surface that is not the enclosure's"""
    late, left = set(), set()
    for scn in MIXED + ('gallery-full',):
        s, o = G.scene(scn), G.reference(scn, 'given')
        own = [i for i in range(s.cs.n_surf) if s.makers[i] != 'filler']
        assert (o['hits'][own] >= 1).all(), (scn, [s.makers[i] for i in own if o['hits'][i] == 0])
        lv = o['levels']
        assert len(lv) == s.reps + 1 and lv[3]['n_live'] >= 100 and o['last_energy'].size >= 1, scn
        late |= _kinds_of(s, N.concatenate([L['surf'] for L in lv[3:]]))
        n_left = _left(s, o)
        left |= _kinds_of(s, [i for i in own if n_left[i] >= 1 and i not in s.terminal])
        # what _check compares beside the tallies: the mapped surface inside and outside its map, the full capture
        H, e_out, n_out, n_hits = o['maps'][s.map_surf]
        print('%s: hits per surface %d..%d, live rays per level %s; %d hits on the map (%d outside), %d captured in full'
              % (scn, o['hits'][own].min(), o['hits'][own].max(), [L['n_live'] for L in lv], n_hits, n_out, o['hits'][s.full_surf]))
        assert n_hits == o['hits'][s.map_surf] >= 10 and 1 <= n_out < n_hits and o['hits'][s.full_surf] >= 30, scn
    assert late == set(G.NPARAMS), sorted(set(G.NPARAMS) - late)
    assert left == set(G.NPARAMS) - set([G.HEX]), sorted(set(G.NPARAMS) - left)
    for scn in ('gallery', 'flats'):        # the sources' references: every level traced on, rays left, the map and the capture hit
        for src in ('disk', 'buie'):
            s, o = G.scene(scn), G.reference(scn, src)
            H, e_out, n_out, n_hits = o['maps'][s.map_surf]
            assert len(o['levels']) == s.reps + 1 and o['last_energy'].size >= 1 and n_hits >= 5 and o['hits'][s.full_surf] >= 30, (scn, src)


@pytest.mark.parametrize('scn', G.ALONE)
def test_alone_both_copies_are_hit_and_left(scn):
    s, o = G.scene(scn), G.reference(scn, 'given')
    n_left = _left(s, o)
    print('%s: stride %d, hits %s, rays that leave a copy and hit again %d' % (scn, s.stride, o['hits'], n_left[:2].sum()))
    assert (o['hits'][:2] >= 20).all() and o['hits'][2] >= 100
    if s.kinds[0] == G.HEX:
        assert s.terminal == [0, 1, 2] and n_left.sum() == 0 and s.full_surf == 0
    else:
        assert n_left[:2].sum() >= MIN_LEFT and s.terminal == [2] and s.full_surf == 0 and o['hits'][0] >= 20
    H, e_out, n_out, n_hits = o['maps'][s.map_surf]
    assert s.map_surf == 2 and n_hits == o['hits'][2] and 30 <= n_out <= n_hits - 30


def _launched(call):
    """(the header's decisions for the call, the kernels it launches by name): geometry_cases.launched, with the restated decisions
    (mega_cases.decide) held to the header's and the predicted search stages to the stages the header names"""
    d, p = G.launched(call)
    mine = M.decide(G.facts(call))
    assert mine == d, (call.name, sorted((k, mine.get(k), d.get(k)) for k in set(mine) | set(d) if mine.get(k) != d.get(k)))
    assert bool(d['use_stream']) == call.stream and (d['decided'] or not call.stream), call.name
    if call.stream:
        stages = set(d[st][0] for st in S.STAGES if d[st][0])
        assert set(p) - set(x[0] for x in d['shk']) <= stages, (call.name, sorted(set(p) - stages))
    return d, set(p)


@pytest.mark.parametrize('name', [c.name for c in G.CALLS])
def test_call_selects_its_instances(name):
    call = G.CALL[name]
    s = G.scene(call.scene)
    d, launched = _launched(call)
    print('%s: %s' % (name, ', '.join(sorted(launched))))
    assert set(call.targets) <= launched, (name, sorted(set(call.targets) - launched))
    if call.stream:
        flat, full = s.flat, s.n_fill > 0
        forced = bool(dict(call.scene_env).get('TRC_GRID_FORCE32', 0))
        assert d['mode'] == (0 if not call.accel else 3 if forced else 2) and d['lds_tables'] == (not full) and d['lds_recs'] == (not full)
        assert all(x[0].startswith('k_s_shade_c<') and (', true, ' in x[0][:22]) == flat for x in d['shk']), d['shk']
        assert len(d['shk']) == (1 if s.kinds[0] == G.HEX else 2), d['shk']         # (two hex dishes in the sphere: no mirror at all)
        assert (d['gridm'] == 3) == s.alone and d['use_absorb'] == (not full)       # (the terminal hits: k_s_absorb where its tables fit)
        if not call.given:
            assert d['use_fp'] and call.scene in ('gallery', 'flats', 'gallery-full')
    else:
        assert d['mega'] == G.MEGA and d['m32']


def test_calls_select_every_form_between_them():
    """the FLAT and the general instance of k_s_fresh, k_s_fresh2, k_s_bounce on all boxes, on the grid and on the large grid, and of
    k_s_bounce_coop; tables in LDS and in global memory; the lean shading kernels of both classes, normal from the frame and from the
    kind; the megakernel; both searches of the ordered engine -- by the library's own names.  Every kind is traced by the streaming
    form and by the megakernel as the widest of its scene and in a mixed scene, and by the ordered engine in a mixed scene"""
    selected = set()
    for call in G.CALLS:
        selected |= _launched(call)[1]
    for scn, kd, accel, kernel in G.ORDERED:
        d = S.library_decide([G.ordered_facts(scn, kd, accel)])[0]
        assert d['ord'] == kernel == M.ordered(G.ordered_facts(scn, kd, accel))[1], (scn, kd, accel, d['ord'])
        selected.add(d['ord'])
    names = set(S.library_ids())
    assert set(G.MUST_SELECT) <= names, sorted(set(G.MUST_SELECT) - names)
    assert set(G.MUST_SELECT) <= selected, sorted(set(G.MUST_SELECT) - selected)
    for stream in (True, False):
        alone = set(c.scene for c in G.CALLS if c.stream == stream and c.scene in G.ALONE)
        mixed = set(c.scene for c in G.CALLS if c.stream == stream and c.scene in MIXED)
        assert alone == set(G.ALONE) and mixed == set(MIXED)
    assert set(scn for scn, kd, accel, kernel in G.ORDERED) == set(MIXED)
    assert len(REFS) <= 40


@pytest.mark.parametrize('scn,src', [k for k in REFS if k[1] != 'given'], ids=['%s:%s' % k for k in REFS if k[1] != 'given'])
def test_footprint_maps_lose_no_hit(scn, src):
    """hc_footprint on the scenes the sources hang over: the map applies, every ray that hits starts in a set cell, finds its surface
    in the cell's list and passes the surface's oriented box"""
    hc = S.hostcheck()[0]
    s = G.scene(scn)
    out = N.zeros(10)
    why = C.create_string_buffer(128)
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    d = s.desc(src)
    rc = hc.hc_footprint(s.cs.n_surf, s.cs.descs, S._ptr(extra), C.byref(d), C.c_long(s.n_rays), C.c_uint64(G.SEED), C.c_uint64(0), S.FP_CELLS,
                         S._ptr(out), why, 128)
    print('%s, %s: %d rays, %d generic, %d with their bit set, %d hits, %d lost' % (scn, src, out[0], out[1], out[2], out[3], out[4]))
    assert rc == 0, why.value
    assert out[0] == s.n_rays and out[4] == 0 and out[3] > 400 and out[3] == len(G.reference(scn, src)['levels'][1]['surf'])
    assert out[2] < out[0]          # (the map culls rays)


def test_unbounded_scene_has_no_footprint_map():
    """the library refuses a map over `open`: its calls trace given rays"""
    hc = S.hostcheck()[0]
    s = G.scene('open')
    out = N.zeros(10)
    why = C.create_string_buffer(128)
    d = G.scene('gallery').desc('disk')
    rc = hc.hc_footprint(s.cs.n_surf, s.cs.descs, S._ptr(N.ascontiguousarray(s.cs.extra)), C.byref(d), C.c_long(10), C.c_uint64(G.SEED), C.c_uint64(0),
                         S.FP_CELLS, S._ptr(out), why, 128)
    assert rc == -3 and b'unbounded' in why.value and all(c.given for c in G.CALLS if c.scene == 'open')
