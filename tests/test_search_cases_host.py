"""
What the tests of the search kernel instances (test_gpu_search_instances.py) take for granted about their calls, checked without a
device from the oracle, the host-compiled check library and the restated choice of kernels alone (search_cases.py): every call is
predicted to launch the instances it is there for, each sum on the side of its limit that the call's scene stands for; its rays hit
every geometry kind of the scene, the twin on the first bounce and later, the receiver that ends every ray on the first bounce and
later; rays are culled on the way and some survive; the footprint map culls rays, lists rays that hit nothing, and leaves rays to
the general side; and apart from the twin no ray is near a tie, so that the device tests exclude no ray at all.  The calls' targets
are the 79 search-stage kernels of the library, by name.  Which ran on a device is recorded in profiles/search_instances.txt.

The restated LDS image is held to the library's (trc_search_lds_layout, exported by the check library) to the byte, and the large
grid of every scene that is forced onto it is held to brute force on the calls' rays before such a scene meets a device.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as N
import pytest

import search_cases as S
import shade_cases as sc

ROOT = S.ROOT
_conditions = {}


def conditions(call):
    """what the reference of (scene, rays) shows, computed once per reference"""
    key = (call.scene, call.src)
    if key in _conditions:
        return _conditions[key]
    s, o = S.scene(call.scene), S.reference(call)
    gm = sc._names('GM_')
    lv = o['levels']
    by_kind = {}
    for i in range(s.cs.n_surf):
        k = gm[s.cs.descs[i].gm_kind]
        by_kind[k] = by_kind.get(k, 0) + int(o['hits'][i])
    # what k_s_cull decides for every ray of the source, against the rays the reference sees hit something
    hc = S.hostcheck()[0]
    bit, generic = N.zeros(S.N_RAYS, dtype=N.uint8), N.zeros(S.N_RAYS, dtype=N.uint8)
    d = S.resolved(s.desc(call.src))
    u8 = C.POINTER(C.c_ubyte)
    assert hc.hc_footprint_bits(s.cs.n_surf, s.cs.descs, C.byref(d), C.c_long(S.N_RAYS), C.c_uint64(S.SEED), C.c_uint64(0), S.FP_CELLS,
                                bit.ctypes.data_as(u8), generic.ctypes.data_as(u8)) == 0
    counts = N.zeros(10)
    why = C.create_string_buffer(128)
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    assert hc.hc_footprint(s.cs.n_surf, s.cs.descs, S._ptr(extra), C.byref(d), C.c_long(S.N_RAYS), C.c_uint64(S.SEED), C.c_uint64(0),
                           S.FP_CELLS, S._ptr(counts), why, 128) == 0, why.value
    hit = N.zeros(S.N_RAYS, dtype=bool)
    hit[lv[1]['parents']] = True
    bit, generic = bit.astype(bool), generic.astype(bool)
    out = dict(by_kind=by_kind,
               twin_first=int(N.isin(lv[1]['surf'], s.twin).sum()), twin_later=sum(int(N.isin(L['surf'], s.twin).sum()) for L in lv[2:]),
               twin_high=int(o['hits'][s.twin[1]]),
               term_first=int((lv[1]['surf'] == s.terminal).sum()), term_later=sum(int((L['surf'] == s.terminal).sum()) for L in lv[2:]),
               culled=sum(L['vertices'].shape[1] - L['n_live'] for L in lv[1:-1]), left=o['last_energy'].size, levels=len(lv),
               counts=counts, fp_bits=int(bit.sum()), fp_culled=int((~bit & ~generic).sum()), fp_listed_miss=int((bit & ~generic & ~hit).sum()),
               fp_general=int(generic.sum()), fp_general_hits=int((generic & hit).sum()), fp_hits=int(hit.sum()),
               ties=S.near_ties(call))
    _conditions[key] = out
    return out


@pytest.mark.parametrize('name', [c.name for c in S.CALLS])
def test_call_selects_its_instances_and_exercises_them(name):
    call = S.CALL[name]
    s, f, p = S.scene(call.scene), S.forms(S.facts(call)), S.predict(call)
    # the prediction: the call's targets among what the host would launch
    for inst in call.targets:
        assert inst in p, (inst, sorted(p))
    print('%s: mode %d, gridm %d, %s' % (name, f['mode'], f['gridm'], ', '.join('%s x %d' % kv for kv in sorted(p.items()))))
    # ... each sum on the side of its limit that the scene and the knobs of the call stand for
    S_ = s.cs.n_surf
    full, mid, small, tiny = call.scene.endswith('-full'), call.scene.endswith('-mid'), call.scene in ('flat', 'curved'), call.scene.startswith('wedge')
    forced = dict(call.scene_env).get('TRC_GRID_FORCE32', 0)
    assert f['lds_recs'] == (S_ * s.stride * 8 <= S.LIMIT_RECS) == (not full)
    assert (S_ <= S.TINY_SURFACES) == tiny and (S_ <= S.SMALL_SURFACES) == (tiny or small)
    assert f['mode'] == (0 if not call.accel else 1 if call.kd else 3 if forced else 2)
    assert f['walk_ok'] == (not forced)
    assert f['small_scene'] == ((tiny or small) and not forced) and f['gridm'] == (2 if forced else 0 if f['mode'] < 2 else 3 if tiny else 1)
    if f['use_fp']:
        q = s.sizes(call.src)
        print('    k_s_fresh: %d bytes against %d, %d list entries against %d' % (f['need_fresh'], S.LIMIT_LDS, q['n_list'], S.LIMIT_LIST))
        assert f['fresh_in_lds'] == (not full) and (f['need_fresh'] > S.LIMIT_LDS) == full
        assert q['n_list'] < S.LIMIT_LIST or full
        assert f['fresh_two'] == (call.src in ('buie', 'rbuie'))
    else:
        assert call.given or dict(call.env).get('TRC_STREAM_FRESH') == 0
    if 'in_lds' in f:
        print('    k_s_bounce: %d bytes against %d' % (f['need_bounce'], S.LIMIT_LDS))
        assert f['in_lds'] == (f['gridm'] in (0, 1) and not full) and (f['need_bounce'] > S.LIMIT_LDS) == full
        assert f['coop'] == (bool(forced) and dict(call.env).get('TRC_STREAM_COOP', 1) != 0)
    if call.second:         # the inequality of launch_bounce holds after the first call: the second one is k_s_fresh's
        assert p[f['fresh'][0]] == 1 and p[f['fresh_one'][0]] == 1 and f['fresh'] != f['fresh_one']
    # the per-ray conditions
    c = conditions(call)
    gm = sc._names('GM_')
    for k in set(gm[s.cs.descs[i].gm_kind] for i in range(S_)):
        assert c['by_kind'].get(k, 0) >= 30, (k, c['by_kind'])
    assert c['twin_first'] >= 100 and c['twin_later'] >= 30 and c['twin_high'] == 0, c
    assert c['term_first'] >= 30 and c['term_later'] >= 30, c
    assert c['levels'] == S.REPS + 1 and c['culled'] >= 64 and c['left'] >= 64, c
    for fr in s.frames:         # no frame is axis aligned
        assert (N.abs(fr[:3, :3]) > 1e-3).sum() >= 8
    # the captured surfaces: the mapped one inside and outside its map, the one captured in full
    o = S.reference(call)
    H, e_out, n_out, n_hits = o['maps'][s.map_surf]
    assert n_hits == o['hits'][s.map_surf] and 30 <= n_out <= n_hits - 30 and o['hits'][s.full_surf] > 300
    # the footprint map's three kinds of ray
    counts = c['counts']
    print('    footprint: %d rays, %d generic, %d with their bit set, %d hits; culled %d, listed without a hit %d, general side %d (%d hits)' %
          (counts[0], counts[1], counts[2], counts[3], c['fp_culled'], c['fp_listed_miss'], c['fp_general'], c['fp_general_hits']))
    if f['use_fp']:
        assert counts[0] == S.N_RAYS and counts[4] == 0 and counts[1] == c['fp_general'] and counts[3] == c['fp_hits']
        assert S.FP_CELLS % 32 == 0 and counts[2] == c['fp_bits']         # (the two exports read the same mask the same way)
        assert c['fp_culled'] >= 100 and c['fp_listed_miss'] >= 100, c
        if call.src in ('buie', 'rbuie'):
            assert c['fp_general'] >= 64 and c['fp_general_hits'] >= 64
        if call.src in ('sun', 'rsun'):
            # The tail of a packed table holds 1 - u_c of the rays (trc_sunshape_pack keeps at most TRC_SUNSHAPE_CORE_TAIL of the mass
            # there, for every table of tests/golden/sunshape.npz), so the 64 of the Buie kinds cannot be had at N_RAYS: the count
            # expected from sun_table() is below it.  Every one of these rays is compared on its own by the device tests; the
            # bound here is the one the hit counts get
            expected = (1. - S.sun_table()[4]) * S.N_RAYS
            print('    general side expected of the table: (1 - %.5f) * %d = %.1f rays' % (S.sun_table()[4], S.N_RAYS, expected))
            assert expected < 64 and abs(c['fp_general'] - expected) < 4. * N.sqrt(expected)
            assert c['fp_general'] >= 30 and c['fp_general_hits'] >= 30, c
    # no near tie but the twin's exact one
    gap, e_gap = c['ties']
    print('    smallest gap between nearest and second-nearest surface %.3g, of an energy from min_energy %.3g (relative)' % (gap, e_gap))
    assert gap > 1e-9 and e_gap > 1e-9


def test_calls_cover_every_instance():
    """79 instances; every one that an input can select is the target of a call, and the calls rest on at most 30 oracle traces"""
    targets = set(t for c in S.CALLS for t in c.targets)
    assert len(S.ALL_INSTANCES) == 79 == len(set(S.ALL_INSTANCES))
    assert set(S.UNREACHABLE) <= set(S.ALL_INSTANCES)
    assert targets == set(S.ALL_INSTANCES) - set(S.UNREACHABLE), (sorted(set(S.ALL_INSTANCES) - targets), sorted(targets - set(S.ALL_INSTANCES)))
    for inst in S.ALL_INSTANCES:
        print('%-52s %s' % (inst, S.UNREACHABLE.get(inst) or ' '.join(c.name for c in S.CALLS if inst in c.targets)))
    assert len(set((c.scene, c.src) for c in S.CALLS)) <= 30


def test_library_holds_the_instances_by_name():
    """the search-stage kernels of the built library, names only (nm -C), are ALL_INSTANCES"""
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    if not os.path.exists(lib) or shutil.which('nm') is None:
        pytest.skip('no built library, or no nm')
    squeeze = lambda x: re.sub(r'\s+', '', x)
    names = set()
    for line in subprocess.check_output(['nm', '-C', lib]).decode().splitlines():
        m = re.search(r'\b(%s)(<[^>]*>)?\((StreamParams|CullParams)\)' % '|'.join(S.FAMILIES), line)
        if m and '__device_stub__' not in line:
            names.add(squeeze(m.group(1) + (m.group(2) or '')))
    assert names == set(squeeze(i) for i in S.ALL_INSTANCES), (sorted(names ^ set(squeeze(i) for i in S.ALL_INSTANCES)))


# -- the library's description of the LDS image against the restated one ----------------------------------------------------------------
def library_layout(rows):
    rows = N.ascontiguousarray(rows, dtype=N.int32).reshape(-1, 13)
    out = N.zeros((len(rows), 14), dtype=N.uint64)
    hc = S.hostcheck()[0]
    hc.hc_search_lds_layout.argtypes = [C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
    assert hc.hc_search_lds_layout(len(rows), rows.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_ulonglong))) == 0
    return out.astype(N.int64)


def same_layout(parts):
    lib = library_layout([[int(x) for x in p] for p in parts])
    for p, row in zip(parts, lib):
        mine = S.lds_layout(p)
        assert [mine[k] for k in S.LAYOUT] == list(row), (p, mine, row)


def test_library_layout_is_the_restated_one_for_every_call():
    """the images behind every decision and every launch of the calls: with the tables and without"""
    parts = []
    for call in S.CALLS:
        s, f = S.scene(call.scene), S.forms(S.facts(call))
        S_, q = s.cs.n_surf, s.sizes(None if call.given else call.src)
        assert q['buie_bytes'] == S.BUIE_BYTES
        if f['use_fp']:
            qw = ((1024 if s.flat else 768) // 64) if f['fresh_two'] else 0
            bb = q['buie_bytes'] if f['fresh_two'] else 0
            parts += [S.fresh_lds_parts(S_, s.stride, q['Mc'], q['n_list'], bb, lds, w) for lds in (True, False) for w in (qw, 0)]
        if 'in_lds' in f:
            g = q['grid_cells'] if f['mode'] == 2 else 0
            occ = q['occ_words'] if f['gridm'] == 2 else 0
            cw = S.SB_THREADS // 64 if f['coop'] else 0
            parts += [S.bounce_lds_parts(S_, s.stride, bb, lds, lds and not bb, g if lds else 0, q['grid_list'], occ, cw)
                      for lds in (True, False) for bb in (q['buie_bytes'], 0)]
            parts.append(S.bounce_lds_parts(S_, s.stride, q['buie_bytes'], True, True, g, q['grid_list'], 0, 0))      # (the decision's image)
    assert len(parts) > 300
    same_layout(parts)


def test_library_layout_is_the_restated_one_for_random_parts():
    """2e4 seeded part sets -- half of them k_s_fresh's, half k_s_bounce's; half drawn freely, half with the surface count solved so that
    the image ends within 2 KiB of 150 KiB, and footprint lists on both sides of 65536 entries -- equal to the byte"""
    rng = N.random.RandomState(20261)
    parts, near, lists = [], [0, 0], [0, 0]
    for i in range(20000):
        stride = (17, 21)[rng.randint(2)]
        bb = (0, 9472)[rng.randint(2)]
        S_ = rng.randint(1, 1200)
        if i % 2:
            Mc = (64, 128, 256)[rng.randint(3)]
            n_list = rng.randint(65536 - 3000, 65536 + 3000) if i % 4 == 1 else rng.randint(0, 40000)
            qw = (0, 12, 16)[rng.randint(3)]
            mk = lambda n: S.fresh_lds_parts(n, stride, Mc, n_list, bb, True, qw)
        else:
            cells, glist = rng.randint(0, 3000), rng.randint(0, 9000)
            occ, cw, flags = rng.randint(0, 2) * rng.randint(1, 500), rng.randint(0, 2) * 16, bool(rng.randint(2))
            mk = lambda n: S.bounce_lds_parts(n, stride, bb, True, flags, cells, glist, occ, cw)
        if i % 4 >= 2:          # the surface count that puts the image at 150 KiB + d, |d| <= 2 KiB
            d = rng.randint(-2 * S.KiB, 2 * S.KiB + 1)
            per = S.lds_need(mk(101)) - S.lds_need(mk(100))
            S_ = max((S.LIMIT_LDS + d - S.lds_need(mk(0))) // max(per, 1), 1)
        p = mk(int(S_))
        need = S.lds_need(p)
        if abs(need - S.LIMIT_LDS) <= 2 * S.KiB:
            near[need > S.LIMIT_LDS] += 1
        if p.fp_offs and abs(p.fp_list - S.LIMIT_LIST) <= 3000:
            lists[p.fp_list >= S.LIMIT_LIST] += 1
        parts += [p, p._replace(tables=False, sbox=False, flags=False, fp_offs=0, fp_list=0, grid_cells=0, grid_list=0)]
    print('within 2 KiB of 150 KiB: %s; lists within 3000 entries of 65536: %s' % (near, lists))
    assert min(near) >= 100 and min(lists) >= 100
    same_layout(parts)


# -- the large grid of the scenes forced onto it --------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', sorted(set((c.scene, c.src) for c in S.CALLS if dict(c.scene_env).get('TRC_GRID_FORCE32'))))
def test_large_grid_agrees_with_brute_force(key):
    """hc_nearest_grid32 -- the grid trc_scene_create builds when the LDS-sized one is refused, walked as k_s_bounce<2> and
    k_s_bounce_coop walk it -- finds the brute-force surface and distance for the rays of every bounce of the reference, the twin's
    ties included"""
    call = [c for c in S.CALLS if (c.scene, c.src) == key][0]
    s, o = S.scene(call.scene), S.reference(call)
    hc = S.hostcheck()[0]
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    total = 0
    for L in o['levels'][:-1]:
        n = L['n_live']
        v, d = [N.ascontiguousarray(a[:, :n]) for a in (L['vertices'], L['directions'])]
        cols = [N.ascontiguousarray(r) for r in list(v) + list(d)]
        tb, tg = N.zeros(n), N.zeros(n)
        sb, sg = N.zeros(n, dtype=N.int32), N.zeros(n, dtype=N.int32)
        stats = N.zeros(5)
        ip = C.POINTER(C.c_int)
        assert hc.hc_nearest(s.cs.n_surf, s.cs.descs, S._ptr(extra), None, C.c_long(n), *([S._ptr(c) for c in cols] +
                             [S._ptr(tb), sb.ctypes.data_as(ip), None, None])) == 0
        assert hc.hc_nearest_grid32(s.cs.n_surf, s.cs.descs, S._ptr(extra), C.c_long(n), *([S._ptr(c) for c in cols] +
                                    [S._ptr(tg), sg.ctypes.data_as(ip), S._ptr(stats)])) == 0
        assert N.array_equal(sb, sg) and N.array_equal(tb, tg), (key, N.nonzero(sb != sg)[0][:10])
        assert not (sb == s.twin[1]).any()
        total += int((sb == s.twin[0]).sum())
    assert total >= 130


# -- the library's choice of kernels (csrc/trc_forms.h) against the restated one ----------------------------------------------------
def test_header_decides_every_call_as_restated():
    """all calls, none left out: every decision of the header for the call's facts -- the plan, the forms, each stage's kernel by name,
    threads and LDS bytes -- is the restated one (mega_cases.decide: forms() here, with the shading and terminal stages of
    shade_cases); and predict()'s kernels are the header's names"""
    import mega_cases as M
    blocks = [S.facts(call) for call in S.CALLS]
    lib = S.library_decide(blocks)
    for call, f, d in zip(S.CALLS, blocks, lib):
        mine = M.decide(f)
        assert mine == d, (call.name, sorted((k, mine.get(k), d.get(k)) for k in set(mine) | set(d) if mine.get(k) != d.get(k)))
        assert d['use_stream'] and d['decided'], call.name
        launched = set(d[st][0] for st in S.STAGES if d[st][0]) - set([d['absorb'][0]])
        assert set(S.predict(call)) <= launched and set(call.targets) <= launched, (call.name, sorted(launched))


def test_header_names_every_instance():
    """the ids the header can produce in the search families, over their argument ranges, are ALL_INSTANCES"""
    names = S.library_ids()
    assert sorted(n for n in names if n.split('<')[0] in S.FAMILIES) == sorted(S.ALL_INSTANCES)
