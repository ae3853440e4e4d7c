"""
What the tests of the megakernel's instances and search branches (test_gpu_mega_instances.py) take for granted about their cases,
checked without a device from the oracle, float64 geometry, the host-compiled check library and the restated plan alone
(mega_cases.py): every case is predicted to launch its target instance, each LDS sum on the side of its limit the case stands for;
the branch a case is there for is taken by its rays -- the exact queue overflows, a lane lists more leaves than it holds, the stack
gets as deep as the tree, surfaces win through list positions beyond 32, an unbounded plane wins and loses an exact tie, rays meet a
plane without entering the scene box; and apart from the intended exact ties no ray is near a tie, so that the device tests exclude
no ray.  The hand-made trees are held to brute force on the cases' rays before they meet a device.  The cases' targets are the 24
megakernel instances of the library, by name.  Which ran on a device is recorded in profiles/mega_instances.txt.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as N
import pytest

import mega_cases as M
import search_cases as S
import shade_cases as sc

ROOT = S.ROOT
MIN_RAYS = 64           # rays that must take a branch
MIN_HITS = 30           # hits that must fall on a surface a case is there for
_ties = {}


def ties(c):
    """the near ties of a trace, once per trace: (gap between nearest and second-nearest surface, of an energy from min_energy)"""
    key = M.trace_key(c)
    if key not in _ties:
        s = M.scene(c.scene)
        _ties[key] = M.near_ties_of(s, M.reference(c), c.min_energy, c.reps)
    return _ties[key]


def _levels(c):
    """(vertices, directions, surfaces hit or -1) of the live rays of every level of the case's reference that is traced on"""
    o = M.reference(c)
    lv = o['levels']
    out = []
    for k, L in enumerate(lv[:-1] if len(lv) > c.reps else lv):
        n = L['n_live']
        if n == 0:
            continue
        hit = N.full(n, -1)
        if k + 1 < len(lv):
            hit[lv[k + 1]['parents']] = lv[k + 1]['surf']
        out.append((N.ascontiguousarray(L['vertices'][:, :n]), N.ascontiguousarray(L['directions'][:, :n]), hit))
    return out


@pytest.mark.parametrize('name', [c.name for c in M.CASES])
def test_case_selects_its_instance_and_takes_its_branches(name):
    c = M.CASE[name]
    s, p = M.scene(c.scene), c.plan()
    q = s.sizes(None)
    # the prediction, with every part of every sum
    print('%s -> %s, staging (%d, %d), %d bytes of dynamic LDS' % (name, M.instance(p['kernel'], c.spec, c.src == 'sun', c.chart), p['lds_tally'], p['lds_scene'], p['lds']))
    print('    S %d (brute list %d, unbounded %d), tree: %d nodes, %d leaf entries, %d always, depth %d; buie %d + tallies %d + search %d + waves x %d'
          % (p['n_surf'], q['brute_list'], q['unbounded'], p['nodes'], p['nleaf'], p['nalways'], p['depth'], p['b_buie'], p['b_tally'], p['b_acc'], p['b_wave']))
    print('    512 threads: %d, 256 threads: %d against %d%s' % (p['lds512'], p['lds256'], M.LDS_MAX_ALLOWED,
          '; tallies %d, + scene %d against %d' % (p['need_tally'], p['need_scene'], M.LDS_MAX_PLAIN) if p['kernel'] == 'fast256' else ''))
    assert p['kernel'] == c.kernel and (p['lds_tally'], p['lds_scene']) == tuple(c.staging)
    assert c.target == M.instance(p['kernel'], c.spec, c.src == 'sun', c.chart) and c.target in M.ALL_INSTANCES
    assert p['b_buie'] == (0 if c.given else M.TRC_BUIE_STAGED * 8) and p['use_kd'] == (c.kd is not None and c.accel)
    if c.kernel == 'coop512':
        assert p['coop_ok'] and p['lds512'] <= M.LDS_MAX_ALLOWED
    elif c.kernel == 'coop256':
        assert p['coop_ok'] and p['lds256'] <= M.LDS_MAX_ALLOWED < p['lds512']
    else:
        too_deep = p['use_kd'] and p['depth'] > M.COOP_MAX_DEPTH
        assert too_deep == (c.kd is not None) and (too_deep or p['lds256'] > M.LDS_MAX_ALLOWED) and p['nodes'] <= M.COOP_MAX_NODES
        assert (p['need_tally'] <= M.LDS_MAX_PLAIN) == bool(c.staging[0]) and (p['need_scene'] <= M.LDS_MAX_PLAIN) == bool(c.staging[1])
    if c.kd is not None:
        assert p['depth'] <= M.TRC_KD_STACK
    # the wave partition: every ray in one wave, no wave beyond the chunk
    part = M.partition(c.n, p['threads'])
    print('    %d rays over %d waves of %d threads: %s' % (c.n, len(part), p['threads'], part if len(part) <= 8 else '%d x %d, then %d' % (len(part) - 1, part[0], part[-1])))
    assert sum(part) == c.n and min(part) >= 1 and max(part) == part[0]
    # the scene: general rotation, the twin's tie goes to the lower index, the receiver ends rays, rays are culled and survive
    o = M.reference(c)
    for fr in s.frames:
        assert (N.abs(fr[:3, :3]) > 1e-3).sum() >= 8
    if s.twin is not None and c.n == M.N_RAYS:
        assert o['hits'][s.twin[0]] >= MIN_HITS and o['hits'][s.twin[1]] == 0 and o['hits'][s.terminal] >= MIN_HITS
    if c.n == M.N_RAYS:
        H, e_out, n_out, n_hits = o['maps'][s.map_surf]
        assert n_hits == o['hits'][s.map_surf] >= MIN_HITS and n_out >= 1 and o['hits'][s.full_surf] >= MIN_HITS
    if c.chart:
        surf = c.chart_map[0]
        Hc = o['chart_maps'][surf]
        assert Hc[3] == o['hits'][surf] >= MIN_HITS and (Hc[0] > 0).mean() >= 0.1 and Hc[4] == 0       # (no hit within 1e-12 of an edge)
    # no near tie but the exact ones
    gap, e_gap = ties(c)
    print('    smallest gap between nearest and second-nearest surface %.3g, of an energy from min_energy %.3g (relative)' % (gap, e_gap))
    assert gap > 1e-9 and e_gap > 1e-9
    # the branches
    for b in c.branches:
        BRANCH[b.split(' = ')[0] if b.startswith(('n =', 'reps =')) else b](c, s, p, o)


# -- the conditions that prove a branch taken ------------------------------------------------------------------------------------------
def _staging(c, s, p, o):
    assert p['kernel'] == 'fast256'


def _count(c, s, p, o):
    part = M.partition(c.n, p['threads'])
    assert {1: [1], 63: [8] * 7 + [7], 64: [8] * 8, 65: [9] * 7 + [2]}[c.n] == part


def _reps(c, s, p, o):
    assert c.reps == 1 and len(o['levels']) == 2 and o['last_energy'].size == o['levels'][1]['n_live'] >= MIN_RAYS


def _walks(c):
    f = M.tree(c).flat()
    v, d, e, rid = M.rays_of(c)
    nonempty = f['leaf_cnt'] > 0
    w = [M.leaves_crossed(f, v[:, i], d[:, i]) for i in range(c.n)]
    return f, N.array([int(nonempty[lv].sum()) for lv, deep in w]), N.array([deep for lv, deep in w])


def _stack_depth(c, s, p, o):
    """rays from the high end hold a pending child at every level: the stack gets as deep as the tree"""
    f, crossed, deepest = _walks(c)
    print('    deepest stack %d in a tree of depth %d, on %d rays' % (deepest.max(), p['depth'], (deepest == p['depth']).sum()))
    assert deepest.max() == p['depth'] == c.kd[1] and (deepest == p['depth']).sum() >= MIN_RAYS


def _leaf_drain(c, s, p, o):
    """in each direction rays cross more non-empty leaves than a lane lists between two drains"""
    f, crossed, deepest = _walks(c)
    up = N.arange(c.n) % 2 == 0
    many = crossed > M.COOP_LEAFCAP
    print('    rays that cross more than %d non-empty leaves: %d from the low end, %d from the high end' % (M.COOP_LEAFCAP, (many & up).sum(), (many & ~up).sum()))
    assert (many & up).sum() >= MIN_RAYS and (many & ~up).sum() >= MIN_RAYS
    near = (s.hi[s.order()[1:c.kd[1]:2], s.axis] - f['split'][2:2 * c.kd[1]:4])
    assert (N.abs(near) <= M.ROW_NEAR * abs(s.T[s.axis, 0]) * M.ROW_PITCH).all() and len(near) >= 8


def _exact_drain(c, s, p, o):
    """every ray's line crosses the boxes of three surfaces at the least, so the first rays of a wave queue more than COOP_E tests"""
    v, d, e, rid = M.rays_of(c)
    crossed = s.boxes_crossed(v, d)
    for threads in (512, 256):
        part = M.partition(c.n, threads)
        first = min(part[0], 64)
        print('    %d threads: %d rays in a wave\'s first round (the last wave: %d) x %d boxes at the least = %d against %d'
              % (threads, first, part[-1], crossed.min(), first * crossed.min(), M.COOP_E))
        # (the last wave takes the remainder of the rays, fewer than the others)
        assert crossed.min() >= 3 and first * 3 > M.COOP_E and all(x == part[0] for x in part[:-1])
    assert p['use_kd'] is False and s.sizes(None)['brute_list'] == s.cs.n_surf


def _always(c, s, p, o):
    alw = M.tree(c).flat()['always_relevant']
    beyond = alw[32:]
    print('    %d always-relevant surfaces; hits on those beyond position 32: %s' % (len(alw), o['hits'][beyond]))
    assert len(alw) == M.ALWAYS_FILL + M.ALWAYS_OWN == 40 and (o['hits'][beyond] >= MIN_HITS).sum() >= 8


def _big_leaf(c, s, p, o):
    """hits on surfaces that stand at position 32 or beyond in every leaf that lists them"""
    f = M.tree(c).flat()
    assert f['leaf_cnt'].max() > 32 and p['use_kd']
    early = set()
    for node in N.nonzero(f['flag'] == 3)[0]:
        early |= set(f['leaf_surfs'][f['leaf_off'][node]:f['leaf_off'][node] + min(f['leaf_cnt'][node], 32)].tolist())
    late = sorted(set(f['leaf_surfs'].tolist()) - early)
    print('    a leaf of %d surfaces; listed at position 32 or beyond only: %s, hit %s times' % (f['leaf_cnt'].max(), late, o['hits'][late]))
    assert len(late) >= 1 and o['hits'][late].sum() >= MIN_HITS


def _interval_end(c, s, p, o):
    """rays that hit the target and for which the end of the pending child's interval, cut to the 16 bits a stack entry keeps, falls
    before the plane in front of the target's cell -- by more than the walk's margins (delta = 1e-3 over the direction cosine, taken
    as 2e-3 here): rounded down instead of up, the walk passes the cell by"""
    sA, sB, sC = s.planes()
    v, d, hit = _levels(c)[0]
    tA, tC = (sA - v[0]) / d[0], (sC - v[0]) / d[0]
    cut = (N.float32(tA + 2e-3).view(N.uint32) & N.uint32(0xFFFF0000)).view(N.float32).astype(float)
    lost = (hit == 0) & (cut < tC - 2e-3)
    inside = M.ray_in_box(s.lo.min(axis=0), s.hi.max(axis=0), v, N.zeros_like(d) + d)
    print('    %d of the %d rays that hit the target would pass its cell by with the interval end rounded down' % (lost.sum(), (hit == 0).sum()))
    assert lost.sum() >= MIN_RAYS and p['use_kd'] and p['kernel'] == 'coop512'
    assert (v[0] > s.lo[:, 0].min()).all() and inside.all()         # (the rays start inside the scene box: t counts from the start point)


def _packed_walk(c, s, p, o):
    f, crossed, deepest = _walks(c)
    print('    tree of depth %d: deepest stack %d, up to %d non-empty leaves crossed' % (p['depth'], deepest.max(), crossed.max()))
    assert p['use_kd'] and p['kernel'] == 'coop512' and deepest.max() >= 3 and (crossed >= 2).sum() >= MIN_RAYS


def _on_planes(c, s, p, o):
    f = M.tree(c).flat()
    v, d, e, rid = M.rays_of(c)
    on = N.zeros(c.n, dtype=bool)
    for a in range(3):
        planes = f['split'][f['flag'] == a]
        if len(planes):
            on |= N.abs(v[a][:, None] - planes[None, :]).min(axis=1) <= 1.5e-3
    print('    %d of %d rays start within 1.5e-3 of a split plane' % (on.sum(), c.n))
    assert on.sum() >= c.n // 8


def _tie_hits(c, s, o):
    return [(int(o['hits'][lo]), int(o['hits'][hi])) for lo, hi in s.ties]


def _inline_over_queue(c, s, p, o):
    (lo, hi), n = s.ties[0], _tie_hits(c, s, o)[0]
    assert not s.bounded[lo] and s.bounded[hi] and n[0] >= MIN_HITS and n[1] == 0, n
    # ... among them rays that enter the scene box, so that the plate is a candidate of the queue
    v, d, hit = _levels(c)[0]
    inside = M.ray_in_box(s.lo[s.bounded].min(axis=0), s.hi[s.bounded].max(axis=0), v, d)
    over = M.ray_in_box(s.lo[hi], s.hi[hi], v, d)
    assert ((hit == lo) & inside & over).sum() >= MIN_HITS


def _queue_over_inline(c, s, p, o):
    (lo, hi), n = s.ties[1], _tie_hits(c, s, o)[1]
    # (the plane goes on beside the plate: none of its hits lies on the plate)
    H = o['hit_list']
    q = N.dot(N.linalg.inv(s.frames[lo]), N.vstack((H['points'][:, H['surf'] == hi], N.ones((H['surf'] == hi).sum()))))
    on_plate = (N.abs(q[0]) <= PLATE_HALF[0]) & (N.abs(q[1]) <= PLATE_HALF[1])
    assert s.bounded[lo] and not s.bounded[hi] and n[0] >= MIN_HITS and on_plate.sum() == 0 and len(on_plate) == n[1], n
    print('    hits on the surfaces that share a plane (lower index, higher index): %s' % (_tie_hits(c, s, o),))


def _outside(c, s, p, o):
    """rays whose half line stays 0.1 clear of the box of the bounded surfaces and that hit a plane"""
    v, d, hit = _levels(c)[0]
    inside = M.ray_in_box(s.lo[s.bounded].min(axis=0) - 0.1, s.hi[s.bounded].max(axis=0) + 0.1, v, d)
    planes = N.nonzero(~s.bounded)[0]
    n = (~inside & N.isin(hit, planes)).sum()
    print('    %d rays never enter the scene box and hit a plane' % n)
    assert n >= MIN_HITS and s.sizes(None)['unbounded'] == len(planes) == 2


def _unbounded_only(c, s, p, o):
    q = s.sizes(None)
    assert q['unbounded'] == s.cs.n_surf == 2 and q['brute_list'] == 0 and (o['hits'] >= MIN_HITS).all()


PLATE_HALF = (1.3, 1.3)         # of the plate in the upper plane (mega_cases.Planes)
BRANCH = {'staging 11': _staging, 'staging 10': _staging, 'staging 00': _staging, 'n': _count, 'reps': _reps, 'stack depth 24': _stack_depth,
          'stack depth 32': _stack_depth, 'leaf drain': _leaf_drain, 'exact drain': _exact_drain, 'always > 32': _always, 'leaf > 32': _big_leaf, 'interval end': _interval_end,
          'packed walk': _packed_walk, 'origins on split planes': _on_planes, 'inline over queue': _inline_over_queue,
          'queue over inline': _queue_over_inline, 'outside the box': _outside, 'unbounded only': _unbounded_only}
# the branches the cases must name between them
BRANCHES = ('exact drain', 'leaf drain', 'leaf > 32', 'always > 32', 'inline over queue', 'queue over inline', 'outside the box', 'unbounded only',
            'stack depth 24', 'stack depth 32', 'staging 11', 'staging 10', 'staging 00', 'n = 1', 'n = 63', 'n = 64', 'n = 65', 'packed walk',
            'origins on split planes', 'interval end', 'COOP_MAX_NODES nodes')


def test_cases_cover_every_instance_and_branch():
    """24 instances; every one that an input can select is the target of a case, every branch is named by a case, and the cases rest on
    at most 24 oracle traces"""
    targets = set(c.target for c in M.CASES)
    assert len(M.ALL_INSTANCES) == 24 == len(set(M.ALL_INSTANCES))
    assert set(M.UNREACHABLE) <= set(M.ALL_INSTANCES) | set(BRANCHES)
    assert targets == set(M.ALL_INSTANCES) - set(M.UNREACHABLE), (sorted(set(M.ALL_INSTANCES) - targets), sorted(targets - set(M.ALL_INSTANCES)))
    for inst in M.ALL_INSTANCES:
        print('%-44s %s' % (inst, M.UNREACHABLE.get(inst) or ' '.join(c.name for c in M.CASES if c.target == inst)))
    named = set(b for c in M.CASES for b in c.branches)
    for b in BRANCHES:
        print('%-28s %s' % (b, M.UNREACHABLE.get(b) or ' '.join(c.name for c in M.CASES if b in c.branches)))
    assert set(BRANCHES) - set(M.UNREACHABLE) <= named
    assert len(set(M.trace_key(c) for c in M.CASES)) <= 24
    # the one branch held to be unreachable: the largest tree below the bound, at its least depth, without a surface
    nodes = M.COOP_MAX_NODES - 1
    depth = int(N.ceil(N.log2(nodes + 1))) - 1
    need = nodes * 8 + 4 * M.coop_wave_bytes(depth)
    assert list(M.UNREACHABLE) == ['COOP_MAX_NODES nodes'] and depth == 13 and need == 163832 > M.LDS_MAX_ALLOWED == 163328
    assert '%d' % need in M.UNREACHABLE['COOP_MAX_NODES nodes']
    # the depths at which the host code takes another path
    assert [c.kd[1] for c in M.CASES if c.kd and c.kd[0] == 'chain'] == [M.COOP_MAX_DEPTH, M.COOP_MAX_DEPTH + 1, M.TRC_KD_STACK, 1]
    assert M.REFUSED_DEPTH == M.TRC_KD_STACK + 1 and S.kd_depth(M.scene('row').chain(M.REFUSED_DEPTH).flat()) == M.REFUSED_DEPTH
    assert [(D + 2 <= M.ORD_STACK_DEPTH) for D, chart, kern in M.ORDERED] == [True, False, False]


def test_wave_partition():
    """chunk = ceil(n / waves) with ceil(n / threads) workgroups: every ray in exactly one wave, at both thread counts; the resident
    grid's cap never binds at these ray counts"""
    for n in (1, 63, 64, 65, 511, 512, 513, M.ONPLANES_RAYS, M.N_RAYS):
        for threads in (512, 256):
            part = M.partition(n, threads)
            grid = (n + threads - 1) // threads
            assert grid <= M.N_CU and sum(part) == n and len(part) <= grid * threads // 64 and all(x == part[0] for x in part[:-1]) and 1 <= part[-1] <= part[0]


def test_library_holds_the_instances_by_name():
    """the megakernel's kernels in the built library, names only (nm -C), are ALL_INSTANCES"""
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    if not os.path.exists(lib) or shutil.which('nm') is None:
        pytest.skip('no built library, or no nm')
    squeeze = lambda x: re.sub(r'\s+', '', x)
    names = set()
    for line in subprocess.check_output(['nm', '-C', lib]).decode().splitlines():
        m = re.search(r'\b(k_trace_\w+)(<[^>]*>)?\(FastParams\)', line)
        if m and '__device_stub__' not in line:
            names.add(squeeze(m.group(1) + (m.group(2) or '')))
    assert names == set(squeeze(i) for i in M.ALL_INSTANCES), sorted(names ^ set(squeeze(i) for i in M.ALL_INSTANCES))


# -- the trees against brute force ----------------------------------------------------------------------------------------------------
TREES = [c.name for c in M.CASES if c.kd is not None and not (c.spec or c.chart or c.src == 'sun')]


def _nearest(s, f, v, d):
    """(brute force, float64 walk, single-precision walk): (t, surface) each, from the check library"""
    hc = S.hostcheck()[0]
    n = v.shape[1]
    kd = M.kd_desc(f)
    extra = N.ascontiguousarray(s.cs.extra if len(s.cs.extra) else N.zeros(1))
    cols = [S._ptr(N.ascontiguousarray(r)) for r in list(v) + list(d)]
    t = [N.zeros(n) for _ in range(3)]
    k = [N.zeros(n, dtype=N.int32) for _ in range(3)]
    ip = C.POINTER(C.c_int)
    assert hc.hc_nearest(s.cs.n_surf, s.cs.descs, S._ptr(extra), C.byref(kd), C.c_long(n), *(cols + [S._ptr(t[0]), k[0].ctypes.data_as(ip), S._ptr(t[1]), k[1].ctypes.data_as(ip)])) == 0
    assert hc.hc_nearest32(s.cs.n_surf, s.cs.descs, S._ptr(extra), C.byref(kd), C.c_long(n), *(cols + [S._ptr(t[2]), k[2].ctypes.data_as(ip)])) == 0
    return list(zip(t, k))


@pytest.mark.parametrize('name', TREES + ['row/chain%d' % D for D in sorted(set(D for D, chart, kern in M.ORDERED))])
def test_tree_agrees_with_brute_force(name):
    """trc_nearest_kd (float64, the walk of k_trace_fast) and trc_nearest_accel32 (the conservative single-precision search) over the
    case's tree find the brute-force surface and distance, and the oracle's surface, for the rays of every level of the reference,
    the exact ties included"""
    if name in M.CASE:
        c = M.CASE[name]
        f = M.tree(c).flat()
    else:
        c = M.CASE['row/boxes']
        f = M.scene('row').chain(int(name[len('row/chain'):])).flat()
    s = M.scene(c.scene)
    assert S.kd_depth(f) <= M.TRC_KD_STACK
    # every surface is listed in a leaf or always relevant
    listed = set(f['leaf_surfs'].tolist()) | set(f['always_relevant'].tolist())
    assert listed == set(range(s.cs.n_surf))
    total = 0
    for v, d, hit in _levels(c):
        (tb, sb), (tk, sk), (t32, s32) = _nearest(s, f, v, d)
        assert N.array_equal(sb, sk) and N.array_equal(tb, tk), (name, 'float64 walk', N.nonzero(sb != sk)[0][:10])
        assert N.array_equal(sb, s32) and N.array_equal(tb, t32), (name, 'single-precision walk', N.nonzero(sb != s32)[0][:10])
        assert N.array_equal(sb, hit), (name, 'oracle', N.nonzero(sb != hit)[0][:10])
        total += len(sb)
    assert total >= c.n


# -- the library's choice of kernels (csrc/trc_forms.h) against the restated one ----------------------------------------------------
def same_decisions(blocks):
    """every decision of the header for the fact blocks equals M.decide's: field by field, LDS byte sums and kernel names included"""
    for f, lib in zip(blocks, S.library_decide(blocks)):
        mine = M.decide(f)
        assert mine == lib, (sorted((k, mine.get(k), lib.get(k)) for k in set(mine) | set(lib) if mine.get(k) != lib.get(k)), f)


def test_header_decides_every_case_as_restated():
    """all cases, none left out: plan() and instance() are mega_plan of the library's own facts; and the target is the header's name"""
    blocks = [c.facts() for c in M.CASES]
    same_decisions(blocks)
    for c, d in zip(M.CASES, S.library_decide(blocks)):
        assert d['mega'] == c.target and not d['use_stream'], c.name
    for depth, chart, kernel in M.ORDERED:          # the ordered engine under the row's chains: the instance of test_gpu_mega_instances
        f = dict(M.CASE['row/chain25'].facts(), kd_depth=depth, chart=int(chart))
        assert S.library_decide([f])[0]['ord'] == kernel[:-1] + ', false>' == M.ordered(f)[1]


def test_header_names_every_instance():
    """the ids the header can produce in the megakernel's families, over their argument ranges, are ALL_INSTANCES; k_ord_bounce's nine"""
    names = S.library_ids()
    assert len(names) == len(set(names))
    assert sorted(n for n in names if n.split('<')[0] in M.FAMILIES) == sorted(M.ALL_INSTANCES)
    assert sorted(n for n in names if n.startswith('k_ord_bounce<')) == sorted(
        'k_ord_bounce<%d, %s, %s>' % (m, M._t(c), M._t(t)) for m in (0, 1, 2) for c, t in ((0, 0), (1, 0), (0, 1)))


# every threshold of the choice: (name, the fact that is moved across it, its range, the decision that flips there, facts held fixed)
_STREAM, _BIG = dict(flags=S.TRACE_ACCEL | S.TRACE_STREAM, n=5000), dict(grid_ok=0, big_ok=1)
THRESHOLDS = [
    ('fewest rays of a streaming call', 'n', (1, 200), 'use_stream', dict(flags=S.TRACE_STREAM)),
    ('TRC_STREAM_MIN_RAYS', 'n', (64, 1 << 21), 'use_stream', dict(flags=S.TRACE_ACCEL, grid_ok=1)),
    ('4096 rays on the large grid', 'n', (64, 1 << 21), 'use_stream', dict(_BIG, flags=S.TRACE_ACCEL)),
    ('65535 surfaces, all boxes', 'n_surf', (60000, 70000), 'plan_ok', dict(flags=0)),
    ('65535 surfaces, k_ord_bounce', 'n_surf', (60000, 70000), 'ord_mode', dict(flags=0)),
    ('STREAM_SMALL_SURFACES', 'n_surf', (5, 60), 'small_scene', dict(_STREAM, grid_ok=1)),
    ('four surfaces', 'n_surf', (1, 24), 'gridm', dict(_STREAM, grid_ok=1)),
    ('40 KiB of records', 'n_surf', (1, 2000), 'lds_recs', dict(_STREAM, grid_ok=1)),
    ('LDS_MAX_ALLOWED, k_s_walk on the grid', 'grid_list', (0, 100000), 'walk_ok', dict(_STREAM, grid_ok=1)),
    ('LDS_MAX_ALLOWED, k_s_walk on all boxes', 'brute_list', (0, 100000), 'walk_ok', dict(_STREAM, flags=S.TRACE_STREAM)),
    ('LDS_MAX_ALLOWED, k_s_walk on the tree', 'kd_nleaf', (0, 100000), 'mode', dict(_STREAM, has_kd=1, accel_kd_ok=1, k_search=1, grid_ok=1)),
    ('150 KiB, k_s_bounce', 'grid_list', (0, 60000), 'bounce', dict(_STREAM, grid_ok=1, n_surf=30, grid_cells=500)),
    ('150 KiB, k_s_fresh', 'fp_n_list', (0, 65000), 'fresh', dict(_STREAM, grid_ok=1, n_surf=30, src_kind=2, fp_use=1, fp_M=512, fp_Mc=128, fp_coverage=.5)),
    ('65536 list entries, k_s_fresh', 'fp_n_list', (60000, 70000), 'fresh', dict(_STREAM, grid_ok=1, n_surf=5, src_kind=0, fp_use=1, fp_M=128, fp_Mc=32, fp_coverage=.5)),
    ('LDS_MAX_ALLOWED, k_s_cull', 'fp_M', (32, 2048), 'use_fp', dict(_STREAM, grid_ok=1, n_surf=5, src_kind=0, fp_use=1, fp_Mc=8, fp_coverage=.5)),
    ('80 KiB of occupancy bits', 'big_occ_words', (1, 40000), lambda d: d.get('bg_occ_words', 0) > 0, dict(_STREAM, accel_ok=1, **_BIG)),
    ('96 KiB of occupancy bits', 'big_occ_words', (1, 40000), lambda d: d.get('bg_occ_words', 0) > 0, dict(_STREAM, accel_ok=1, k_coop=0, **_BIG)),
    ('LDS_MAX_ALLOWED, k_trace_coop<512>', 'brute_list', (0, 100000), 'mega_threads', dict(flags=0)),
    ('LDS_MAX_ALLOWED, k_trace_coop<256>', 'brute_list', (40000, 100000), 'm32', dict(flags=0)),
    ('COOP_MAX_NODES', 'kd_nodes', (1, 20000), 'm32', dict(flags=S.TRACE_ACCEL, has_kd=1, accel_kd_ok=1, n_surf=2, kd_depth=1)),
    ('COOP_MAX_DEPTH', 'kd_depth', (1, 40), 'm32', dict(flags=S.TRACE_ACCEL, has_kd=1, accel_kd_ok=1, kd_nodes=31)),
    ('ORD_STACK_DEPTH', 'kd_depth', (1, 40), 'ord_mode', dict(flags=S.TRACE_ACCEL, has_kd=1, accel_kd_ok=1, kd_nodes=31)),
    ('LDS_MAX_PLAIN, tallies of k_trace_fast', 'n_surf', (1, 5000), 'mega_lds_tally', dict(flags=0, accel_ok=0)),
    ('LDS_MAX_PLAIN, scene of k_trace_fast', 'n_surf', (1, 5000), 'mega_lds_scene', dict(flags=0, accel_ok=0)),
    ('72 KiB, k_s_shade', 'n_extra', (0, 20000), 'lds_tables', dict(_STREAM, grid_ok=1, cls_moving=4, cls_all=4)),
    ('72 KiB, k_s_shade_x', 'n_extra', (0, 20000), 'lds_tables', dict(_STREAM, grid_ok=1, carry=1, cls_all=4)),
    ('78 KiB with bins, k_s_shade', 'fm_bins', (1, 20000), 'lds_fm_bins', dict(_STREAM, grid_ok=1, cls_moving=4, cls_all=4, n_fm_edges=40, fms_bytes=136)),
    ('120 KiB, lean kernels', 'n_extra', (0, 30000), 'shk', dict(_STREAM, grid_ok=1, cls_moving=2, cls_all=2)),
    ('150 KiB with bins, lean kernels', 'fm_bins', (1, 30000), 'shk', dict(_STREAM, grid_ok=1, cls_moving=1, cls_all=1, n_fm_edges=40, fms_bytes=136)),
    ('158 KiB, terminal hits inside k_s_bounce', 'grid_list', (0, 60000), 'absorb_inline',
     dict(_STREAM, accel_ok=1, grid_ok=1, grid_cells=500, n_surf=30, stride=15, n_extra=0, cls_moving=1, cls_all=1, any_term=1, n_fm_edges=40, fms_bytes=136,
          fm_bins=8000, carry=0, splits=0, chart=0, transfer=0, term_ok=1, k_absorb=-1, k_bounce=1, k_search=2)),
]
# Two limits of the header are not in the list because no fact block is decided by them: S <= 65535 of mega_plan (the tallies of
# 65536 surfaces alone are 1.5 MB, beyond LDS_MAX_ALLOWED) and k_s_absorb's 78 KiB (its image is part of k_s_shade's, which has passed
# 72 KiB, or 78 KiB with the bins, before).  The free blocks of the sweep agree on them all the same.


def random_block(rng):
    """a fact block drawn freely: scenes of 1..3000 surfaces (now and then beyond 65535) on either grid, on a tree or on their boxes,
    with and without maps, terminal surfaces and a source with its footprint map; every flag and knob of a call"""
    b, r = lambda p=.5: int(rng.rand() < p), rng.randint
    n_surf = r(1, 40) if b(.3) else r(65000, 66000) if b(.03) else r(1, 3001)
    has_kd, maps, src = b(), r(0, 3), (-1, 0, 1, 2, 3, 7, 8)[r(7)]
    cls_all = r(1, 8)
    f = S.blank_facts(n_surf=n_surf, stride=(15, 17, 21)[r(3)], accel_ok=b(.95), has_kd=has_kd, accel_kd_ok=has_kd and b(.9),
                      kd_nodes=has_kd * (2 * r(1, 9000) + 1), kd_nleaf=has_kd * r(0, 90000), kd_nalways=has_kd * r(0, 50), kd_depth=has_kd * r(1, 33),
                      grid_ok=b(.6), big_ok=b(.7), grid_cells=r(1, 4000), grid_list=r(0, 60000), brute_list=r(0, n_surf + 1), n_unbounded=b(.1) * r(1, 4),
                      big_occ_words=r(0, 40000), n_fm_edges=maps * r(4, 80), fms_bytes=maps * sc.SIZEOF_FLUXMAPDEV, n_extra=b() * r(1, 12000),
                      fm_bins=maps * r(1, 4000), chart=maps and b(.2), transfer=b(.1), splits=b(.1), all_flat=b(), cls_all=cls_all,
                      cls_moving=cls_all & r(0, 8), any_term=b(),
                      n=(r(1, 200), r(3000, 6000), r(1000000, 1100000), r(1, 1 << 22))[r(4)], flags=r(0, 16) & ~2, src_kind=src, spec=src >= 0 and b(.3),
                      carry=b(.15), mat_dev=b(.1), term_ok=b(.9),
                      k_search=(1, 2)[b(.8)], k_fresh=b(.9), k_bounce=b(.8), k_first=b(.3), k_coop=b(.7), k_absorb=(-1, 0, 1)[r(3)], k_umask=b(.8))
    f['simple'] = f['all_flat'] and b()
    if src >= 0 and b(.8):
        Mc = (32, 64, 128, 256)[r(4)]
        f.update(fp_use=1, fp_n_list=r(0, 70000), fp_M=4 * Mc, fp_Mc=Mc, fp_has_generic=b(), fp_cdf_end=rng.rand() * 1.1, fp_coverage=rng.rand(),
                 fp_ucoverage=rng.rand() * 1.1, fp_umask_words=b(.8) * r(64, 8193), fp_Mu=1 << r(6, 11), fp_Mv=1 << r(0, 11))
    return dict((k, (v if isinstance(v, float) else int(v))) for k, v in f.items())


def test_header_decides_random_calls_as_restated():
    """
    1e5 seeded fact blocks: three quarters drawn freely (random_block), a quarter in pairs one step apart across one of THRESHOLDS --
    a random block with the threshold's fixed facts, the moved fact found by bisection of the restated decision -- so that every
    threshold named in csrc/trc_forms.h is straddled at least 100 times; the header's decisions equal the restated ones for all of them
    """
    rng = N.random.RandomState(20262)
    blocks, crossed = [], dict((t[0], 0) for t in THRESHOLDS)
    while len(blocks) < 75000:
        blocks.append(random_block(rng))
    while len(blocks) < 100000:
        name, key, (lo, hi), what, fixed = THRESHOLDS[rng.randint(len(THRESHOLDS))]
        f = dict(random_block(rng), **fixed)
        at = lambda v: what(M.decide(dict(f, **{key: v}))) if callable(what) else M.decide(dict(f, **{key: v})).get(what)
        first = at(lo)
        if at(hi) == first:         # (this block does not reach the threshold: its other facts decide)
            blocks += [dict(f, **{key: lo}), dict(f, **{key: hi})]
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if at(mid) == first else (lo, mid)
        blocks += [dict(f, **{key: lo}), dict(f, **{key: hi})]
        crossed[name] += 1
    print(crossed)
    assert all(n >= 100 for n in crossed.values()), crossed
    for k in range(0, len(blocks), 10000):
        same_decisions(blocks[k:k + 10000])
