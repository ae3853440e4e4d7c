"""
Calls that select every instance and every search branch of the persistent megakernel, and their host reference
(test_mega_cases_host.py for what can be said without a device, test_gpu_mega_instances.py on one).

The megakernel is three kernels, k_trace_coop<512 | 256, SPEC, SUN, CHART> and k_trace_fast<256, SPEC, SUN, CHART>
(csrc/trc_kernels.hip): 24 compiled instances.  mega_plan picks the kernel and k_trace_fast's staging form from byte sums over the
scene, the Kd-tree set on it and the source; its id takes SPEC, SUN and CHART from the source and the scene's flux maps.
plan() restates the first, instance() the second, partition() the slice of the ray range every wave takes; engine() and ordered()
restate the choice between the engines and k_ord_bounce's search.  They take a fact block (search_cases.FACT_KEYS), and decide()
puts them together with the restatements of search_cases.py and shade_cases.py.  What holds them to the library: the decisions of
csrc/trc_forms.h itself, exported by the check library (search_cases.library_decide), must equal decide() field by field -- for every
case, and for 1e5 random fact blocks across every threshold (test_mega_cases_host.py).

The scenes are the rooms of search_cases.py -- general rotation, a twin whose exact tie the reference gives to the lower index, a
receiver that ends every ray, a lean and a full capture, a flux map -- with filler counts taken from plan(), Kd-trees over them that
change no result (the reference's build, and hand-made ones that are deeper than any build of these scenes gets), and a row of small
plates under hand-made chains of every depth at which the host code takes another path.  Every call over one scene and one set of
rays shares one oracle trace: a tree, accel and a chart map change no ray.
"""
import collections
import ctypes as C
import functools

import numpy as N

import fluxmap_chart_scene as fc
import fluxmap_scene as fs
import search_cases as S
import shade_cases as sc

N_RAYS, REPS, SEED, E_MIN_SHARE = sc.N_RAYS, sc.REPS, sc.SEED, sc.E_MIN_SHARE
KiB = 1024
COOP_LEAFCAP = 16               # csrc/trc_forms.h: leaves listed per lane between two drains
COOP_E = 128                    # ... exact-test queue entries per wave
COOP_MAX_NODES = 16384          # ... mega_plan: `sc->kd_nodes <= COOP_MAX_NODES` (14 bits of a stack entry)
COOP_MAX_DEPTH = 24             # ... mega_plan: `sc->accel.kd_depth <= COOP_MAX_DEPTH`
COOP_FIXED_BYTES = COOP_E * 8 + 64 * 8 + COOP_E * 4 + 64 * 4 + 64 * 4 + 64 * 4 + COOP_LEAFCAP * 64 * 2
LDS_MAX_ALLOWED = 160 * KiB - 512           # ... mega_plan: `lds <= LDS_MAX_ALLOWED`
LDS_MAX_PLAIN = 64 * KiB        # ... mega_plan: `M.lds + b_tally <= LDS_MAX_PLAIN`, `M.lds + b_scene <= LDS_MAX_PLAIN`
TRC_KD_STACK = 32               # csrc/trc_core.h; trc_scene_set_kdtree: `max_depth > TRC_KD_STACK` is refused
ORD_STACK_DEPTH = 24            # csrc/trc_forms.h, trc_ordered_choose: `kd_depth + 2 <= ORD_STACK_DEPTH`
TRC_BUIE_NELEM = 210            # include/tracer_amd.h
TRC_BUIE_STAGED = 3 * (TRC_BUIE_NELEM + 1) + 6 + 3          # csrc/trc_core.h: TRC_BUIE_TABLE + 3
MAX_SURFACES = 65535            # mega_plan: `S <= 65535`
N_CU = 256                      # compute units of the device: the resident grid is at least one workgroup on each


def coop_wave_bytes(depth):
    """COOP_WAVE_BYTES(depth): a wave's queues and lists, and `depth` rows of its packed stack"""
    return depth * 64 * 4 + COOP_FIXED_BYTES


# -- mega_plan, its instance and the wave partition restated -----------------------------------------------------------------------
def plan(f):
    """
    mega_plan (csrc/trc_forms.h) restated for a fact block (search_cases.FACT_KEYS): the tree set on the scene, trace_fast's accel
    (flags), whether a source descriptor travels with the call (src_kind >= 0: its Buie table is staged whatever the source kind).
    Returns dict(kernel 'coop512' | 'coop256' | 'fast256', threads, lds_tally, lds_scene, lds: the dynamic LDS asked for, and the sums
    behind every decision).
    """
    Sn = f['n_surf']
    has_kd = bool(f['has_kd'])
    use_kd = has_kd and bool(f['flags'] & S.TRACE_ACCEL)
    nodes, nleaf, nalways, depth = f['kd_nodes'], f['kd_nleaf'], f['kd_nalways'], f['kd_depth']
    p = dict(n_surf=Sn, use_kd=use_kd, nodes=nodes, nleaf=nleaf, nalways=nalways, depth=depth)
    p['b_buie'] = b_buie = TRC_BUIE_STAGED * 8 if f['src_kind'] >= 0 else 0
    p['b_tally'] = b_tally = (3 * Sn + 2) * 8
    p['coop_ok'] = bool(f['accel_ok']) and Sn <= MAX_SURFACES and (not use_kd or (bool(f['accel_kd_ok']) and nodes <= COOP_MAX_NODES and depth <= COOP_MAX_DEPTH))
    p['b_acc'] = 6 * Sn * 4 + ((2 * nodes * 4 + nalways * 4 + nleaf * 2) if use_kd else (8 + f['brute_list'] * 2)) + f['n_unbounded'] * 4 + 32
    p['b_wave'] = coop_wave_bytes((depth if depth > 0 else 1) if use_kd else 1)
    p['lds512'], p['lds256'] = [b_buie + b_tally + p['b_acc'] + (t // 64) * p['b_wave'] for t in (512, 256)]
    p['threads'] = 256
    if p['coop_ok'] and p['lds512'] <= LDS_MAX_ALLOWED:
        p.update(kernel='coop512', threads=512, lds=p['lds512'], lds_tally=1, lds_scene=0)
    elif p['coop_ok'] and p['lds256'] <= LDS_MAX_ALLOWED:
        p.update(kernel='coop256', lds=p['lds256'], lds_tally=1, lds_scene=0)
    else:
        p['b_scene'] = b_scene = Sn * f['stride'] * 8 + ((nodes * 8 + (nodes * 2 + nleaf + nalways) * 4 + 8) if has_kd else 0)
        lds = b_buie
        p['need_tally'] = lds + b_tally
        p['lds_tally'] = int(p['need_tally'] <= LDS_MAX_PLAIN)
        lds += b_tally if p['lds_tally'] else 0
        p['need_scene'] = lds + b_scene
        p['lds_scene'] = int(p['need_scene'] <= LDS_MAX_PLAIN)
        lds += b_scene if p['lds_scene'] else 0
        p.update(kernel='fast256', lds=lds)
    return p


STREAM_MIN_RAYS, STREAM_MIN_RAYS_BIG, STREAM_FEWEST_RAYS = 1048576, 4096, 64         # csrc/trc_forms.h


def engine(f, forms):
    """trc_fast_choose_engine restated, from the streaming plan of search_cases.forms(f): dict(use_stream, refused, engine_mode)"""
    stream_ok = f['n'] >= STREAM_FEWEST_RAYS and bool(forms['plan_ok'])
    mode = forms['mode'] if stream_ok else 0
    only = bool(f['carry'] or f['splits'])
    force_stream = bool(f['flags'] & S.TRACE_STREAM) or only
    force_mega = not only and bool(f['flags'] & S.TRACE_MEGAKERNEL)
    use = stream_ok and (force_stream or (not force_mega and f['n'] >= (STREAM_MIN_RAYS_BIG if mode == 3 else STREAM_MIN_RAYS)))
    return dict(use_stream=int(use), refused=int(only and not use), engine_mode=mode)


def ordered(f):
    """trc_ordered_choose restated: (mode of the search, instance of k_ord_bounce)"""
    use_kd = bool(f['has_kd']) and bool(f['flags'] & S.TRACE_ACCEL)
    mode = 0
    if f['accel_ok'] and f['big_ok'] and not use_kd:
        mode = 2
    elif f['accel_ok'] and f['n_surf'] <= MAX_SURFACES and (not use_kd or (f['accel_kd_ok'] and f['kd_depth'] + 2 <= ORD_STACK_DEPTH)):
        mode = 1
    return mode, 'k_ord_bounce<%d, %s, %s>' % (mode, _t(f['chart']), _t(f['mat_dev'] and not f['chart']))


def decide(f):
    """every decision of csrc/trc_forms.h restated for a fact block, in the shape of search_cases.library_decide: plan() / instance(),
    engine(), ordered() here, search_cases.forms(), shade_cases.shade_forms() and absorb_forms()"""
    d = S.forms(f)
    out = engine(f, d)
    p = plan(f)
    out.update(m32=int(p['kernel'] != 'fast256'), mega_threads=p['threads'], mega_lds=p['lds'], mega_lds_tally=p['lds_tally'], mega_lds_scene=p['lds_scene'],
               mega=instance(p['kernel'], f['spec'], f['src_kind'] in (7, 8), f['chart']))
    out['ord_mode'], out['ord'] = ordered(f)
    out.update(plan_ok=d['plan_ok'], mode=d.get('mode', 0), lds_walk=d.get('lds_walk', 0), walk_ok=d.get('walk_ok', 1), decided=0)
    sh = sc.shade_forms(f) if d['plan_ok'] else None
    if sh is None:
        return out
    d.update(sh)
    d.update(sc.absorb_forms(f, d))
    out.update((k, d[k]) for k in S.FORM_KEYS + S.STAGES + ('shk',))
    out['decided'] = 1
    return out


def _t(x):
    return 'true' if x else 'false'


KERNEL = {'coop512': 'k_trace_coop<512, %s, %s, %s>', 'coop256': 'k_trace_coop<256, %s, %s, %s>', 'fast256': 'k_trace_fast<256, %s, %s, %s>'}


def instance(kernel, spec, sun, chart):
    """the id of mega_plan: the instance as a kernel trace names it"""
    return KERNEL[kernel] % (_t(spec), _t(sun), _t(chart))


ALL_INSTANCES = [instance(k, sp, su, ch) for k in ('coop512', 'coop256', 'fast256') for sp in (0, 1) for su in (0, 1) for ch in (0, 1)]
# instances and branches that no input selects: {instance or branch: the condition in the host code that excludes it, with its sum}
UNREACHABLE = {
    # mega_plan's `sc->kd_nodes <= COOP_MAX_NODES` never decides: a binary tree of 16383 nodes (the most an odd count allows below the
    # bound) is 13 deep at the least, and its nodes alone (8 bytes each) with four waves' regions pass LDS_MAX_ALLOWED before a
    # surface is counted; test_mega_cases_host.py repeats the sum
    'COOP_MAX_NODES nodes': '16383 nodes x 8 + 4 x COOP_WAVE_BYTES(13) = 131064 + 32768 = 163832 > 163328 = LDS_MAX_ALLOWED',
}
FAMILIES = ('k_trace_coop', 'k_trace_fast')


def partition(n, threads):
    """mega_launch and the kernels' first lines: the rays of every wave that gets any, in wave order.  The grid is the resident grid
    capped at ceil(n / threads) workgroups; at these ray counts the cap decides, whatever the occupancy"""
    max_grid = (n + threads - 1) // threads
    assert 1 <= max_grid <= N_CU            # (one workgroup per compute unit is resident at the least)
    n_waves = max_grid * (threads // 64)
    chunk = (n + n_waves - 1) // n_waves
    return [min(chunk, n - w * chunk) for w in range(n_waves) if w * chunk < n]


# -- the rooms ------------------------------------------------------------------------------------------------------------------
ROOM_OWN = {'flat': 13, 'curved': 16}           # shade_cases.room's own surfaces; + 3 with ends=True
ROOM_STRIDE = 21                                # (14 + the polygon's 6 parameters) | 1


def _room_plan(n_surf):
    """plan() of a room traced from a descriptor source without a tree, every surface bounded (brute_list = S): what decides the filler
    counts; test_mega_cases_host.py repeats the sums with the sizes the library reads off the scene"""
    return plan(S.blank_facts(n_surf=n_surf, stride=ROOM_STRIDE, brute_list=n_surf, flags=S.TRACE_ACCEL, src_kind=S.SRC_KIND['buie']))


def fill_for(what, kind='curved'):
    """the filler count of a room, from plan() alone: 'coop256' the middle of the band of surface counts whose image fits with 256
    threads and not with 512; 'fast256' an eighth of the band's width beyond its end"""
    own = ROOM_OWN[kind] + 3
    Sn = own
    while _room_plan(Sn)['kernel'] == 'coop512':
        Sn += 1
    first = Sn
    while _room_plan(Sn)['kernel'] == 'coop256':
        Sn += 1
    last = Sn - 1
    assert last > first
    if what == 'coop256':
        return (first + last) // 2 - own
    assert what == 'fast256'
    return last + 1 + (last - first) // 8 - own


S.SCENES.setdefault('curved-256', ('room', 'curved', fill_for('coop256')))
S.SCENES.setdefault('curved-fast', ('room', 'curved', fill_for('fast256')))
CHART_SURF, CHART = 14, 'cylinder'          # the finite cylinder among the curved room's own surfaces, binned in (z, azimuth)
CHART_EDGES = (N.linspace(-0.7, 0.7, 8), N.linspace(0., 2. * N.pi, 13))


# -- the row: 34 small plates under hand-made chains --------------------------------------------------------------------------------
ROW_PLATES, ROW_PITCH, ROW_SIZE, ROW_BEAM = 34, 0.5, 0.2, 0.45
ROW_NEAR = 1e-3                 # every second plate's box ends this share of the pitch before its split plane


class Hand(object):
    """a scene put together by hand under the room's rotation, with attributes as search_cases.Scene's: parts: (geometry, optics,
    transform in the room's frame (or in T), half sizes of a plate or None for an unbounded plane); given rays of energy 1 only"""
    kind, n_fill, W, spec, flat = 'flat', 0, 0, False, True

    def build(self, name, parts, map_surf, full_surf, edges, twin, terminal, T=None):
        from tracer_amd.assembly import Assembly
        from tracer_amd.object import AssembledObject
        from tracer_amd.surface import Surface
        from tracer_amd.scene import compile_scene
        from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
        self.name = name
        self.T = T = N.dot(translate(-3.7, 5.2, 1.9), N.dot(rotx(-0.5), N.dot(roty(0.8), rotz(-0.9)))) if T is None else T
        asm = Assembly(objects=[AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr, h in parts])
        self.cs = compile_scene(asm)
        Sn = self.cs.n_surf
        assert Sn == len(parts)
        self.frames = [N.array(s._temp_frame) for s in self.cs.surfaces]
        self.map_surf, self.full_surf, self.twin, self.terminal = map_surf, full_surf, twin, terminal
        self.edges = {map_surf: edges}
        self.captured = [i for i in range(Sn) if self.cs.capture[i]]
        self.stride = sc.record_stride(self.cs)
        # the boxes of the plates, from their corners in global coordinates; a plane has none
        c = N.array([[sx, sy, 0., 1.] for sx in (-1, 1) for sy in (-1, 1)]).T
        self.bounded = N.array([h is not None for gm, o, tr, h in parts])
        self.lo, self.hi = N.full((Sn, 3), -N.inf), N.full((Sn, 3), N.inf)
        for i, F in enumerate(self.frames):
            if self.bounded[i]:
                q = N.dot(F, c * N.r_[parts[i][3], 1., 1.][:, None])[:3]
                self.lo[i], self.hi[i] = q.min(axis=1), q.max(axis=1)

    def source(self, src):
        raise AssertionError('traced with given rays only')

    def min_energy(self, src):
        return E_MIN_SHARE * 1.

    def to_global(self, v, d):
        R = self.T[:3, :3]
        d = d / N.sqrt((d ** 2).sum(axis=0))
        return (N.ascontiguousarray(N.dot(R, v) + self.T[:3, 3:4]), N.ascontiguousarray(N.dot(R, d)), N.ones(v.shape[1]),
                N.arange(v.shape[1], dtype=N.uint64))

    def sizes(self, src):
        out = N.zeros(14)
        S.hostcheck()[0].hc_search_sizes(self.cs.n_surf, self.cs.descs, None, S.FP_CELLS, S._ptr(out))
        return dict(brute_list=int(out[5]), unbounded=int(out[6]))

    def boxes_crossed(self, v, d, margin=0.):
        """per ray, the boxes of bounded surfaces its half line crosses (float64 slab test on the surfaces' own boxes: what the
        conservative single-precision test passes at the least)"""
        return sum(ray_in_box(self.lo[i] - margin, self.hi[i] + margin, v, d).astype(int) for i in N.nonzero(self.bounded)[0])


def ray_in_box(lo, hi, v, d):
    """rays (3, n) whose half line t >= 0 meets the box"""
    with N.errstate(all='ignore'):
        t0, t1 = (lo[:, None] - v) / d, (hi[:, None] - v) / d
    tmin = N.maximum(N.nanmax(N.minimum(t0, t1), axis=0), 0.)
    tmax = N.nanmin(N.maximum(t0, t1), axis=0)
    return tmin <= tmax


class Row(Hand):
    """
    34 small tilted partial mirrors on a line along the first axis of the room's rotated frame, a twin in front of the first and a
    receiver behind the last.  Given rays run along the line in both directions: from the low end they cross the leaves of a chain
    one after the other; from the high end they hold a pending child at every level, so the stack gets as deep as the tree.
    """
    def __init__(self):
        from tracer_amd.flat_surface import RectPlateGM
        from tracer_amd import optics_callables as opt
        from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
        half = N.pi / 2.
        parts = []
        for i in range(ROW_PLATES):
            # the plates face along the line, tilted by up to 0.4 rad about axes that turn from plate to plate
            tilt = N.dot(rotx(0.25 * N.cos(1.3 * i)), roty(half + 0.3 * N.sin(0.9 * i + 0.4)))
            o = opt.ReflectiveDetector(0.1) if i == 0 else opt.Lambertian(0.4) if i % 3 == 1 else opt.Reflective(0.3)
            off = 0.25 * N.cos(2.1 * i), 0.25 * N.sin(1.7 * i)
            parts.append((RectPlateGM(ROW_SIZE, ROW_SIZE), o, N.dot(translate((i + 0.5) * ROW_PITCH, off[0], off[1]), tilt), [ROW_SIZE / 2.] * 2))
        twin = N.dot(translate(-0.8, 0., 0.), N.dot(rotz(0.2), roty(half)))
        parts += [(RectPlateGM(2.2, 2.2), opt.Reflective(0.3), twin, [1.1, 1.1]), (RectPlateGM(2.2, 2.2), opt.Lambertian(1.), twin, [1.1, 1.1]),
                  (RectPlateGM(2.4, 2.4), opt.LambertianReceiver(1.), N.dot(translate(ROW_PLATES * ROW_PITCH + 0.8, 0., 0.), N.dot(rotx(0.3), roty(-half))),
                   [1.2, 1.2])]
        Sn = len(parts)
        self.build('row', parts, Sn - 1, 0, (fs.nonuniform(-0.6, 0.5, 9), N.linspace(-0.5, 0.7, 7)), (Sn - 3, Sn - 2), Sn - 1)
        assert sorted(self.captured) == sorted([self.full_surf, self.terminal])
        self.axis = int(N.abs(self.T[:3, 0]).argmax())            # the global axis the line runs along the most

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """(vertices, directions, energy, ray ids): seeded rays of energy 1 along the line, alternately from the two ends, starting
        within ROW_BEAM of the line and turned by up to 25 mrad"""
        assert src == 'row'
        rng = N.random.RandomState(SEED)
        up = N.arange(N_RAYS) % 2 == 0
        r, ph = ROW_BEAM * N.sqrt(rng.uniform(size=N_RAYS)), rng.uniform(0., 2. * N.pi, N_RAYS)
        v = N.vstack((N.where(up, -0.5, ROW_PLATES * ROW_PITCH + 0.5), r * N.cos(ph), r * N.sin(ph)))
        d = N.vstack((N.where(up, 1., -1.), 0.025 * rng.uniform(-1., 1., N_RAYS), 0.025 * rng.uniform(-1., 1., N_RAYS)))
        return self.to_global(v, d)

    @functools.lru_cache(maxsize=None)
    def order(self):
        """the plates in the order of their place on the tree's axis"""
        mid = (self.lo[:ROW_PLATES, self.axis] + self.hi[:ROW_PLATES, self.axis]) / 2.
        o = N.argsort(mid)
        assert (self.hi[o[:-1], self.axis] < self.lo[o[1:], self.axis]).all()       # (a plane of the axis separates neighbours)
        return o

    def chain(self, D):
        """a tree of depth D as an object with flat(): node i splits the slab of the i-th plate off as a leaf and the rest hangs below"""
        assert 1 <= D < ROW_PLATES
        a, o = self.axis, self.order()
        pitch = abs(self.T[a, 0]) * ROW_PITCH
        split = N.empty(D)
        for k in range(D):
            gap_lo, gap_hi = self.hi[o[k], a], self.lo[o[k + 1], a]
            # every second plate reaches to within ROW_NEAR of the pitch of the plane behind it
            split[k] = gap_lo + 0.5 * ROW_NEAR * pitch if k % 2 else (gap_lo + gap_hi) / 2.
            assert gap_lo < split[k] < gap_hi
        n = 2 * D + 1
        flag, child, sp = N.full(n, 3, dtype=N.int32), N.zeros(n, dtype=N.int32), N.zeros(n)
        leaf_off, leaf_cnt, leaf_surfs = N.zeros(n, dtype=N.int32), N.zeros(n, dtype=N.int32), []
        cells = {}
        for k in range(D):          # interior node 2k: children 2k + 1 (the slab, a leaf) and 2k + 2 (the rest)
            flag[2 * k], child[2 * k], sp[2 * k] = a, 2 * k + 1, split[k]
            cells[2 * k + 1] = (split[k - 1] if k else -N.inf, split[k])
        cells[2 * D] = (split[D - 1], N.inf)
        for node in sorted(cells):
            lo, hi = cells[node]
            inside = [i for i in range(self.cs.n_surf) if self.hi[i, a] >= lo and self.lo[i, a] <= hi]
            leaf_off[node], leaf_cnt[node] = len(leaf_surfs), len(inside)
            leaf_surfs += inside
        return HandTree(dict(flag=flag, split=sp, child=child, leaf_off=leaf_off, leaf_cnt=leaf_cnt,
                             leaf_surfs=N.array(leaf_surfs, dtype=N.int32), always_relevant=N.zeros(0, dtype=N.int32),
                             bounds=N.r_[self.lo.min(axis=0), self.hi.max(axis=0)]))


class Stack(Hand):
    """
    Large parallel plates behind one another -- a pane the rays pass, a mirror captured in full, a diffuse plate and, last, the
    twin -- under a receiver.  Given rays come down through all of them: every ray's line crosses the boxes of at least three, so a
    wave's first 64 rays queue more exact tests than the queue of COOP_E holds, and it is drained in the middle of the search.
    """
    def __init__(self):
        from tracer_amd.flat_surface import RectPlateGM
        from tracer_amd import optics_callables as opt
        from tracer_amd.spatial_geometry import translate, rotz
        last = N.dot(translate(0., 0., 0.), rotz(0.3))
        parts = [(RectPlateGM(3., 3.), opt.Transparent(), translate(0.5, 0., 1.2), [1.5, 1.5]),
                 (RectPlateGM(3., 3.), opt.ReflectiveDetector(0.1), N.dot(translate(-0.4, 0.3, 0.8), rotz(0.2)), [1.5, 1.5]),
                 (RectPlateGM(3., 3.), opt.Lambertian(0.4), N.dot(translate(0.3, -0.5, 0.4), rotz(-0.4)), [1.5, 1.5]),
                 (RectPlateGM(3.4, 3.4), opt.Reflective(0.3), last, [1.7, 1.7]), (RectPlateGM(3.4, 3.4), opt.Lambertian(1.), last, [1.7, 1.7]),
                 (RectPlateGM(6., 6.), opt.LambertianReceiver(1.), translate(0., 0., 2.8), [3., 3.])]
        self.build('stack', parts, 5, 1, (fs.nonuniform(-2.2, 1.9, 11), N.linspace(-1.8, 2.4, 8)), (3, 4), 5)
        assert sorted(self.captured) == [1, 5]

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """seeded rays of energy 1 from a disc of radius 1.6 under the receiver, down onto the plates, turned by up to 0.15 rad"""
        assert src == 'stack'
        rng = N.random.RandomState(SEED + 1)
        r, ph = 1.6 * N.sqrt(rng.uniform(size=N_RAYS)), rng.uniform(0., 2. * N.pi, N_RAYS)
        v = N.vstack((r * N.cos(ph), r * N.sin(ph), N.full(N_RAYS, 2.3)))
        d = N.vstack((0.15 * rng.uniform(-1., 1., N_RAYS), 0.15 * rng.uniform(-1., 1., N_RAYS), -N.ones(N_RAYS)))
        return self.to_global(v, d)


PLANES_OUTSIDE = 4              # every fourth ray of the planes' bundle starts and runs beside the scene box


class Planes(Hand):
    """
    Two unbounded planes (FlatGeometryManager) that close a space below and above, and between them plates: one in the lower plane
    at a higher index than the plane (the plane, tested inline, wins the tie over the queue's winner), one in the upper plane at a lower
    index than the plane (the queue's winner keeps the tie), a mirror captured in full, a twin and a receiver.  Every fourth given ray
    starts far beside the plates and meets a plane without entering the scene box.  alone: the two planes and nothing else.
    """
    def __init__(self, alone):
        from tracer_amd.flat_surface import FlatGeometryManager, RectPlateGM
        from tracer_amd import optics_callables as opt
        from tracer_amd.spatial_geometry import translate, rotx, roty
        self.alone = alone
        floor, ceiling = translate(-0.2, 0.4, 0.), N.dot(translate(0., 0., 3.), rotx(N.pi))
        if alone:
            parts = [(FlatGeometryManager(), opt.LambertianReceiver(0.6), floor, None), (FlatGeometryManager(), opt.ReflectiveDetector(0.2), ceiling, None)]
            self.build('planes-alone', parts, 0, 1, (fs.nonuniform(-2.5, 2.2, 11), N.linspace(-2., 2.6, 8)), None, None)
            self.ties = ()
        else:
            twin = N.dot(translate(1.2, -0.8, 1.1), N.dot(rotx(-0.45), roty(-0.35)))
            parts = [(FlatGeometryManager(), opt.Lambertian(0.5), floor, None),                                         # 0: the lower plane
                     (RectPlateGM(2.6, 2.6), opt.Reflective(0.3), N.dot(ceiling, translate(0.3, 0.2, 0.)), [1.3, 1.3]),  # 1: in the upper plane
                     (RectPlateGM(2.8, 2.8), opt.Lambertian(1.), floor, [1.4, 1.4]),                                    # 2: in the lower plane
                     (RectPlateGM(2., 2.), opt.ReflectiveDetector(0.1), N.dot(translate(-1.6, 0., 1.4), roty(1.2)), [1., 1.]),
                     (RectPlateGM(1.4, 1.4), opt.Reflective(0.3), twin, [0.7, 0.7]), (RectPlateGM(1.4, 1.4), opt.Lambertian(1.), twin, [0.7, 0.7]),
                     (RectPlateGM(1.6, 1.6), opt.LambertianReceiver(1.), N.dot(translate(1.5, 1.3, 0.9), N.dot(rotx(0.4), roty(-0.5))), [0.8, 0.8]),
                     (FlatGeometryManager(), opt.Reflective(0.4), N.dot(ceiling, translate(0.3, 0.2, 0.)), None)]       # 7: the upper plane
            self.build('planes', parts, 6, 3, (fs.nonuniform(-0.7, 0.6, 9), N.linspace(-0.6, 0.8, 7)), (4, 5), 6)
            self.ties = ((0, 2), (1, 7))            # (lower index, higher index) of the surfaces that share a plane
            assert sorted(self.captured) == [3, 6]

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """seeded rays of energy 1 between the planes: from a disc of radius 1.5 at half height, up and down in turn and turned by up
        to 0.5 rad; every fourth from 9 to 12 beside the plates"""
        assert src == self.name
        rng = N.random.RandomState(SEED + 2)
        r, ph = 1.5 * N.sqrt(rng.uniform(size=N_RAYS)), rng.uniform(0., 2. * N.pi, N_RAYS)
        far = N.arange(N_RAYS) % PLANES_OUTSIDE == PLANES_OUTSIDE - 1
        r = N.where(far, rng.uniform(9., 12., N_RAYS), r)
        v = N.vstack((r * N.cos(ph), r * N.sin(ph), N.full(N_RAYS, 1.5)))
        d = N.vstack((0.5 * rng.uniform(-1., 1., N_RAYS), 0.5 * rng.uniform(-1., 1., N_RAYS), N.where(N.arange(N_RAYS) % 2 == 0, -1., 1.)))
        return self.to_global(v, d)


SLIVER_GAP = 0.004              # from the target's box to the split planes before and behind it


class Sliver(Hand):
    """
    A small plate that faces the rays almost squarely, 15 along the first global axis from where they start, in a cell of the tree that
    is 0.045 thick: between a plane just behind its box (the root's) and a plane just before it, two levels further down.  The walk
    reaches that cell through a pending child whose interval ends at the root's plane; the 16 bits a packed stack entry keeps of that
    end are 0.0625 apart at 15, so an end rounded down instead of up falls before the second plane for a share of the start points,
    and the walk then passes the cell by.  Behind the plate the twin takes what gets past it.  The scene is moved, not turned: the
    planes of a tree stand on the global axes, and the plates are each turned a little about all three.
    """
    def __init__(self):
        from tracer_amd.flat_surface import RectPlateGM
        from tracer_amd import optics_callables as opt
        from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
        half = N.pi / 2.
        turn = lambda a, b, c: N.dot(rotx(a), N.dot(roty(b), rotz(c)))
        twin = N.dot(translate(16.5, 0.1, 0.), turn(0.07, half - 0.1, 0.3))
        parts = [(RectPlateGM(0.5, 0.5), opt.ReflectiveDetector(0.1), N.dot(translate(15.035, 0., 0.), turn(0.05, half - 0.06, 0.2)), [0.25, 0.25]),
                 (RectPlateGM(2., 2.), opt.Reflective(0.3), twin, [1., 1.]), (RectPlateGM(2., 2.), opt.Lambertian(1.), twin, [1., 1.]),
                 (RectPlateGM(9., 9.), opt.LambertianReceiver(1.), N.dot(translate(-1., 0., 0.1), turn(-0.06, half + 0.08, 0.15)), [4.5, 4.5]),
                 (RectPlateGM(1., 1.), opt.Lambertian(0.4), N.dot(translate(5., 1.3, 0.2), turn(0.3, 0.4, 0.5)), [0.5, 0.5])]
        self.build('sliver', parts, 3, 0, (fs.nonuniform(-1.2, 1.1, 9), N.linspace(-1., 1.3, 7)), (1, 2), 3, T=translate(2.1, -1.3, 0.6))
        assert sorted(self.captured) == [0, 3]

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """seeded rays of energy 1 along the first axis, from start points spread over a length of 1, 0.8 wide (some pass the target by) and 0.24 high,
        turned by up to 4 mrad"""
        assert src == 'sliver'
        rng = N.random.RandomState(SEED + 4)
        v = N.vstack((rng.uniform(0., 1., N_RAYS), rng.uniform(-0.4, 0.4, N_RAYS), rng.uniform(-0.12, 0.12, N_RAYS)))
        d = N.vstack((N.ones(N_RAYS), 0.004 * rng.uniform(-1., 1., N_RAYS), 0.004 * rng.uniform(-1., 1., N_RAYS)))
        return self.to_global(v, d)

    def planes(self):
        """(behind the target's box, well before it, just before it) on the first global axis"""
        return self.hi[0, 0] + SLIVER_GAP, self.lo[0, 0] - 1., self.lo[0, 0] - SLIVER_GAP

    def tree(self):
        """root: the plane behind the target; below it the plane well before the target, and below that, on the far side, the plane just
        before the target: nodes 0 root, 1 / 2 its children, 3 / 4 those of 1, 5 / 6 those of 4 -- the target is listed in leaf 6 alone"""
        sA, sB, sC = self.planes()
        flag = N.array([0, 0, 3, 3, 0, 3, 3], dtype=N.int32)
        child = N.array([1, 3, 0, 0, 5, 0, 0], dtype=N.int32)
        split = N.array([sA, sB, 0., 0., sC, 0., 0.])
        cells = {2: (sA, N.inf), 3: (-N.inf, sB), 5: (sB, sC), 6: (sC, sA)}
        leaf_off, leaf_cnt, leaf_surfs = N.zeros(7, dtype=N.int32), N.zeros(7, dtype=N.int32), []
        for node in sorted(cells):
            inside = [i for i in range(self.cs.n_surf) if self.hi[i, 0] >= cells[node][0] and self.lo[i, 0] <= cells[node][1]]
            leaf_off[node], leaf_cnt[node] = len(leaf_surfs), len(inside)
            leaf_surfs += inside
        assert leaf_surfs[leaf_off[6]:leaf_off[6] + leaf_cnt[6]] == [0] and leaf_surfs.count(0) == 1 and leaf_cnt[5] == 0
        return HandTree(dict(flag=flag, split=split, child=child, leaf_off=leaf_off, leaf_cnt=leaf_cnt, leaf_surfs=N.array(leaf_surfs, dtype=N.int32),
                             always_relevant=N.zeros(0, dtype=N.int32), bounds=N.r_[self.lo.min(axis=0), self.hi.max(axis=0)]))


class HandTree(object):
    """what DeviceScene.set_kdtree takes: an object with flat()"""
    def __init__(self, flat):
        self._flat = flat

    def flat(self):
        return self._flat


def nested(s, D):
    """a valid tree of depth D over any scene: D planes across the box of the room, on its three axes in turn, every leaf listing every
    surface (a tree is valid when every leaf lists the surfaces whose boxes touch its cell; listing more changes no result)"""
    corners = N.array([[x, y, z, 1.] for x in (-2.6, 2.6) for y in (-2.6, 2.6) for z in (-0.6, 3.2)]).T
    p = N.dot(s.T, corners)[:3]
    lo, hi = p.min(axis=1), p.max(axis=1)
    n, Sn = 2 * D + 1, s.cs.n_surf
    flag, child, sp = N.full(n, 3, dtype=N.int32), N.zeros(n, dtype=N.int32), N.zeros(n)
    leaf_off, leaf_cnt = N.zeros(n, dtype=N.int32), N.zeros(n, dtype=N.int32)
    for k in range(D):
        a = k % 3
        flag[2 * k], child[2 * k] = a, 2 * k + 1
        sp[2 * k] = lo[a] + (hi[a] - lo[a]) * (k // 3 + 1.) / (D // 3 + 2.)
    leaves = [i for i in range(n) if flag[i] == 3]
    for j, node in enumerate(leaves):
        leaf_off[node], leaf_cnt[node] = j * Sn, Sn
    return HandTree(dict(flag=flag, split=sp, child=child, leaf_off=leaf_off, leaf_cnt=leaf_cnt,
                         leaf_surfs=N.tile(N.arange(Sn, dtype=N.int32), len(leaves)), always_relevant=N.zeros(0, dtype=N.int32),
                         bounds=N.r_[lo, hi]))


ALWAYS_FILL, ALWAYS_OWN = 32, 8         # 'always40': objects without a box -- fillers first, then the floor and the walls
ALWAYS_LEAF = 24                        # 'always40': ... of at most this many, so that the tree stays with the cooperative kernel
BIG_LEAF = 40                           # 'bigleaf': the build stops at leaves of at most this many boxes


@functools.lru_cache(maxsize=None)
def built(name, without=0, min_leaf=1):
    """the reference's build over a room whose fillers bring the box of their plate and whose own objects the box of the room;
    without: 32 fillers and the room's first 8 surfaces bring none"""
    from tracer_amd.accel_tree import KdTree
    from tracer_amd.boundary_shape import BoundaryBox
    builder, kind, n_fill = S.SCENES[name]
    asm = sc.room(kind, n_fill, ends=True)[0]
    side = int(N.ceil(N.sqrt(n_fill))) if n_fill else 1
    h = 0.45 * 4. / side
    skip = set(list(range(ALWAYS_FILL)) + list(range(n_fill, n_fill + ALWAYS_OWN))) if without else set()
    for i, o in enumerate(asm.get_objects()):
        if i not in skip:
            o.add_boundary(BoundaryBox([[-h, -h, -0.01], [h, h, 0.01]] if i < n_fill else [[-2.1, -2.1, -1.4], [2.1, 2.1, 1.4]]))
    return KdTree(asm, 8 + 1.3 * N.log(len(asm.get_objects())), min_leaf=min_leaf)


@functools.lru_cache(maxsize=None)
def scene(name):
    hand = {'row': Row, 'stack': Stack, 'sliver': Sliver, 'planes': lambda: Planes(False), 'planes-alone': lambda: Planes(True)}
    return hand[name]() if name in hand else S.scene(name)


def tree(c):
    """the Kd-tree of a case: None, ('chain', D) over the row, ('sliver',), ('nested', D), ('built',) the reference's build of search_cases.Scene.kdtree, ('always40',), ('bigleaf',)"""
    if c.kd is None:
        return None
    s = scene(c.scene)
    if c.kd[0] == 'chain':
        return s.chain(c.kd[1])
    if c.kd[0] == 'sliver':
        return s.tree()
    if c.kd[0] == 'nested':
        return nested(s, c.kd[1])
    if c.kd[0] == 'built':
        return s.kdtree()
    if c.kd[0] == 'always40':
        return built(c.scene, without=1, min_leaf=ALWAYS_LEAF)
    assert c.kd[0] == 'bigleaf'
    return built(c.scene, min_leaf=BIG_LEAF)


# -- the cases -------------------------------------------------------------------------------------------------------------------
_Case = collections.namedtuple('Case', 'name scene src spec chart given n reps accel kd kernel staging branches')


class Case(_Case):
    """scene: of search_cases.SCENES, or 'row'; src: 'buie' | 'sun' (descriptor sources) | 'row'; spec: the source has a spectrum; chart: a
    chart map on the cylinder; given: the rays go in as a bundle; n: the first n rays; kd: see tree(); kernel, staging: what plan() must
    say; branches: the branches of the search the case is there for.  The attributes below are what test_gpu_shade_instances._check reads."""
    cs = property(lambda self: scene(self.scene).cs)
    frames = property(lambda self: scene(self.scene).frames)
    edges = property(lambda self: scene(self.scene).edges)
    map_surf = property(lambda self: scene(self.scene).map_surf)
    full_surf = property(lambda self: scene(self.scene).full_surf)
    captured = property(lambda self: scene(self.scene).captured)
    min_energy = property(lambda self: scene(self.scene).min_energy('buie' if self.src == 'onplanes' else self.src))
    W = 0

    @property
    def target(self):
        return instance(self.kernel, self.spec, self.src == 'sun', self.chart)

    @property
    def chart_map(self):
        """(surface, chart, u edges, v edges) of the case's chart map, or None"""
        return (scene(self.scene).n_fill + CHART_SURF, CHART) + CHART_EDGES if self.chart else None

    def source(self):
        """the pending bundle of the descriptor source: search_cases.Scene.source with the spectrum of shade_cases"""
        s = scene(self.scene)
        b = s.source(self.src)
        if not self.spec:
            return b
        from tracer_amd import sources
        return sources._new_bundle(b._src_desc, b._src_n, b._src_seed, b._src_offset, spectrum=sc.spectrum(), table=b._src_table)

    def bundle(self, given):
        from tracer_amd.ray_bundle import RayBundle
        if not given:
            assert self.n == N_RAYS
            return self.source()
        v, d, e, rid = rays_of(self)
        return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())

    def facts(self):
        """the fact block of the call: the scene with its maps and the case's tree as the library gathers them (search_cases.scene_facts),
        a call of n rays that leaves the engine to the library"""
        s = scene(self.scene)
        kd = tree(self)
        edges = dict(s.edges)
        if self.chart:
            edges[self.chart_map[0]] = CHART_EDGES
        f = S.scene_facts(s.cs, kd.flat() if kd is not None else None, None, edges, chart=self.chart)
        f.update(n=self.n, flags=S.TRACE_ACCEL if self.accel else 0, src_kind=-1 if self.given else S.SRC_KIND[self.src], spec=int(self.spec),
                 term_ok=int(self.min_energy >= 0.))
        return f

    def plan(self):
        return plan(self.facts())


def _case(name, scn, src, kernel, staging=(1, 0), spec=False, chart=False, given=False, n=N_RAYS, reps=REPS, accel=True, kd=None, branches=()):
    return Case(name, scn, src, spec, chart, given, n, reps, accel, kd, kernel, staging, tuple(branches))


def _cases():
    out = []
    # the 24 instances: a Buie disc and a tabulated sunshape, with and without a spectrum, with and without a chart map, over the small
    # room (k_trace_coop<512>), the same room under a tree too deep for the cooperative walk (k_trace_fast, tallies and scene in LDS:
    # the float64 walk with its private stack) and the room in the band of k_trace_coop<256>
    for tag, scn, kernel, staging, kd in (('small', 'curved', 'coop512', (1, 0), None), ('small/deep', 'curved', 'fast256', (1, 1), ('nested', COOP_MAX_DEPTH + 1)),
                                          ('band', 'curved-256', 'coop256', (1, 0), None)):
        for src in ('buie', 'sun'):
            for spec in (False, True):
                for chart in (False, True):
                    name = '%s/%s%s%s' % (tag, src, '/spec' if spec else '', '/chart' if chart else '')
                    out.append(_case(name, scn, src, kernel, staging, spec=spec, chart=chart, kd=kd, branches=('staging %d%d' % staging,) if kd else ()))
    # k_trace_fast's other staging forms: the records beyond 64 KiB under the deep tree (tallies in LDS, the walk reads global memory);
    # the room beyond the band (nothing in LDS, tallies by global atomics, brute force over the records)
    out += [_case('full/deep/buie', 'curved-full', 'buie', 'fast256', (1, 0), kd=('nested', COOP_MAX_DEPTH + 1), branches=('staging 10',)),
            _case('beyond/buie', 'curved-fast', 'buie', 'fast256', (0, 0), branches=('staging 00',))]
    # ray counts around a wave, and one interaction only
    for n in (1, 63, 64, 65):
        out.append(_case('small/given/%d' % n, 'curved', 'buie', 'coop512', given=True, n=n, branches=('n = %d' % n,)))
    out.append(_case('small/buie/reps1', 'curved', 'buie', 'coop512', reps=1, branches=('reps = 1',)))
    # the cooperative kernel's own Kd walk: the reference's build over the mid room; a list of always-relevant surfaces longer than
    # 32, and the build stopped at leaves of up to 40 boxes, over the full room
    out += [_case('mid/buie/kd', 'curved-mid', 'buie', 'coop512', kd=('built',), branches=('packed walk',)),
            _case('full/buie/always40', 'curved-full', 'buie', 'coop512', kd=('always40',), branches=('always > 32',)),
            _case('full/buie/bigleaf', 'curved-full', 'buie', 'coop512', kd=('bigleaf',))]
    # the chains over the row: the last depth the cooperative walk takes (every stack row used, more leaves than a lane lists between
    # two drains), the first it leaves to k_trace_fast, the last trc_scene_set_kdtree accepts
    out += [_case('row/chain24', 'row', 'row', 'coop512', given=True, kd=('chain', COOP_MAX_DEPTH), branches=('stack depth 24', 'leaf drain')),
            _case('row/chain25', 'row', 'row', 'fast256', (1, 1), given=True, kd=('chain', COOP_MAX_DEPTH + 1), branches=('staging 11',)),
            _case('row/chain32', 'row', 'row', 'fast256', (1, 1), given=True, kd=('chain', TRC_KD_STACK), branches=('stack depth 32',)),
            _case('row/boxes', 'row', 'row', 'coop512', given=True, accel=False, branches=())]
    # a Kd leaf of more than 32 surfaces whose last entries are listed nowhere else: chain(1), the first slab and all the rest; the
    # interval end of a packed stack entry (see Sliver)
    out += [_case('row/chain1', 'row', 'row', 'coop512', given=True, kd=('chain', 1), branches=('leaf > 32',)),
            _case('sliver', 'sliver', 'sliver', 'coop512', given=True, kd=('sliver',), branches=('interval end',))]
    # the exact queue drained in the middle of a search; unbounded planes: both operands of the tie rule, rays that never enter the
    # scene box, and a scene without a bounded surface
    out += [_case('stack', 'stack', 'stack', 'coop512', given=True, branches=('exact drain',)),
            _case('planes', 'planes', 'planes', 'coop512', given=True, branches=('inline over queue', 'queue over inline', 'outside the box')),
            _case('planes-alone', 'planes-alone', 'planes-alone', 'coop512', given=True, branches=('unbounded only',))]
    # the general Kd case on given rays: the oracle's second-level rays, a fifth of them moved onto split planes of the tree
    out.append(_case('mid/onplanes/kd', 'curved-mid', 'onplanes', 'coop512', given=True, n=ONPLANES_RAYS, kd=('built',), branches=('origins on split planes',)))
    assert len(set(c.name for c in out)) == len(out)
    return out


ONPLANES_RAYS = 2048


@functools.lru_cache(maxsize=None)
def onplanes_rays():
    """(vertices, directions, energy, ray ids): the first ONPLANES_RAYS rays that leave the first hit of the oracle's trace of the mid
    room, a fifth of them moved onto a split plane of the built tree (within 1.5e-3, the construction of tests/fuzz_searches.py: the
    single-precision walk takes both children there)"""
    L = reference(CASE['mid/buie/kd'])['levels'][1]
    assert L['n_live'] >= ONPLANES_RAYS
    v, d, e = [N.array(L[k][..., :ONPLANES_RAYS]) for k in ('vertices', 'directions', 'energy')]
    f = S.scene('curved-mid').kdtree().flat()
    rng = N.random.RandomState(SEED + 3)
    for a in range(3):
        planes = N.unique(f['split'][f['flag'] == a])
        if len(planes):
            pick = rng.uniform(size=ONPLANES_RAYS) < 0.2 / 3.
            j = N.clip(N.searchsorted(planes, v[a, pick]), 0, len(planes) - 1)
            v[a, pick] = planes[j] + rng.uniform(-1.5e-3, 1.5e-3, pick.sum())
    return N.ascontiguousarray(v), N.ascontiguousarray(d), N.ascontiguousarray(e), N.arange(ONPLANES_RAYS, dtype=N.uint64)


def rays_of(c):
    """(vertices, directions, energy, ray ids) of the case's first n rays"""
    r = onplanes_rays() if c.src == 'onplanes' else scene(c.scene).rays(c.src)
    return [a[..., :c.n] for a in r]


CASES = _cases()
CASE = dict((c.name, c) for c in CASES)
REFUSED_DEPTH = TRC_KD_STACK + 1            # chain(33): refused by trc_scene_set_kdtree with TRC_ERR_UNSUPPORTED
ORDERED = ((ORD_STACK_DEPTH - 2, False, 'k_ord_bounce<1, false>'), (ORD_STACK_DEPTH - 1, False, 'k_ord_bounce<0, false>'), (ORD_STACK_DEPTH - 1, True, 'k_ord_bounce<0, true>'))


def trace_key(c):
    """what an oracle trace depends on: a tree, accel and a chart map change no ray"""
    return (c.scene, c.src, c.spec, c.n, c.reps)


# -- the references ----------------------------------------------------------------------------------------------------------------
_REF = {}


def host_wavelengths(c):
    """the wavelengths the device draws for the case's rays, from the host-compiled sampler (as shade_cases.host_wavelengths: the draw
    depends on the seed and the ray's number alone)"""
    import os
    S.hostcheck()
    lib = C.CDLL(os.path.join(S.ROOT, 'tests', 'hostcheck', 'libtrc_spectrum_check.so'))
    p = C.POINTER(C.c_double)
    lib.hs_spectrum_draw.argtypes = [p, p, p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long, p, p]
    wl, val, cdf = [N.ascontiguousarray(a, dtype=float) for a in sc.spectrum().table()]
    out = N.empty(c.n)
    lib.hs_spectrum_draw(S._ptr(wl), S._ptr(val), S._ptr(cdf), wl.size, SEED, 0, c.n, None, S._ptr(out))
    return out


def reference(c, wavelengths=None):
    """The oracle's trace of the case's scene and rays, computed once per trace_key and shared (nobody changes it); a SPEC case's is
    kept per source of its wavelengths (the host sampler's draws, or those handed in: the pending bundle's, drawn on a device)"""
    from oracle import engine
    key = trace_key(c) + (('given' if wavelengths is not None else 'host') if c.spec else '',)
    if key not in _REF:
        s = scene(c.scene)
        v, d, e, rid = rays_of(c)
        with N.errstate(all='ignore'):
            if c.spec:
                wl = host_wavelengths(c) if wavelengths is None else N.asarray(wavelengths, dtype=float)
                o = engine.trace(engine.scene_from_compiled(s.cs), v, d, e, N.ones(c.n), wl, rid, c.reps, c.min_energy, SEED)
            else:
                o = engine.trace_bundle(s.cs, v, d, e, c.reps, c.min_energy, SEED, offset=0)
        o['hit_list'] = sc.hit_list(o['levels'], s)
        o['maps'] = fs.host_maps(o['hit_list'], s.frames, s.edges)
        if isinstance(s, S.Scene) and s.kind == 'curved':
            m = (s.n_fill + CHART_SURF, CHART) + CHART_EDGES
            o['chart_maps'] = fc.host_maps(o['hit_list'], s.frames, {m[0]: (m[1], False, m[2], m[3])})
        _REF[key] = o
    return _REF[key]


def filler_boxes(s):
    """{filler: (lo, hi)} of a room: the boxes of shade_cases.room's filler plates, from their frames and their size"""
    if not s.n_fill:
        return {}
    h = 0.45 * 4. / int(N.ceil(N.sqrt(s.n_fill)))
    c = N.array([[sx * h, sy * h, 0., 1.] for sx in (-1, 1) for sy in (-1, 1)]).T
    out = {}
    for i in range(s.n_fill):
        q = N.dot(s.frames[i], c)[:3]
        out[i] = (q.min(axis=1), q.max(axis=1))
    return out


def near_ties_of(s, o, min_energy, reps):
    """shade_cases.near_ties for a scene of this module: (smallest relative gap between a ray's nearest and second-nearest
    intersection, smallest relative distance of an outgoing energy from min_energy) over every level of the reference that is traced
    on.  The higher index of every pair of surfaces that share their plane on purpose -- the twin, a plate in an unbounded plane --
    is left out: those ties are exact, and the reference decides them by index"""
    from oracle import engine, geometry
    scn = engine.scene_from_compiled(s.cs)
    skip = ([s.twin[1]] if s.twin is not None else []) + [hi for lo, hi in getattr(s, 'ties', ())]
    seen, same = set(), []          # (shade_cases.identical_surfaces, by hashing: these rooms have thousands of surfaces)
    for k, x in enumerate(scn):
        key = (x['kind'], N.asarray(x['frame'], dtype=float).tobytes(), N.asarray(x['gm'], dtype=float).tobytes())
        same += [k] if key in seen else []
        seen.add(key)
    assert same == ([s.twin[1]] if s.twin is not None else [])
    boxes = filler_boxes(s)
    gap, lv = N.inf, o['levels']
    for L in lv[:-1] if len(lv) > reps else lv:
        n = L['n_live']
        if n == 0:
            continue
        v, d = L['vertices'][:, :n], L['directions'][:, :n]
        first, second = N.full(n, N.inf), N.full(n, N.inf)
        for k, x in enumerate(scn):
            if k in skip:
                continue
            if k in boxes:          # (a filler: only the rays whose half line meets its box can meet the plate)
                m = ray_in_box(boxes[k][0] - 1e-6, boxes[k][1] + 1e-6, v, d)
                if not m.any():
                    continue
                t = N.full(n, N.inf)
                t[m] = geometry.intersect(x['kind'], x['frame'], x['gm'], x['extra'], v[:, m], d[:, m])
            else:
                t = geometry.intersect(x['kind'], x['frame'], x['gm'], x['extra'], v, d)
            t[t == 0.] = N.inf
            second = N.minimum(second, N.maximum(first, t))
            first = N.minimum(first, t)
        both = N.isfinite(second)
        if both.any():
            gap = min(gap, ((second[both] - first[both]) / second[both]).min())
    e = N.concatenate([L['energy'] for L in lv[1:]])
    return gap, (N.abs(e / min_energy - 1.).min() if len(e) else N.inf)


# -- walking a flat tree on the host -------------------------------------------------------------------------------------------------
kd_desc = S.kd_desc


def leaves_crossed(f, v, d):
    """the leaves a ray's line crosses inside the tree's box, in the order of the walk, and the deepest stack on the way: the walk of
    trc_nearest_kd in float64 without its early end (the cooperative walk has none)"""
    lo, hi = f['bounds'][:3], f['bounds'][3:]
    with N.errstate(all='ignore'):
        inv = 1. / d
        t0, t1 = (lo - v) * inv, (hi - v) * inv
    tmin, tmax = max(0., N.nanmax(N.minimum(t0, t1))), N.nanmin(N.maximum(t0, t1))
    if not (tmax > 0. and tmin <= tmax):
        return [], 0
    out, stack, node, deepest = [], [], 0, 0
    while True:
        if f['flag'][node] != 3:
            a = f['flag'][node]
            with N.errstate(all='ignore'):
                tp = (f['split'][node] - v[a]) * inv[a]
            c1, c2 = f['child'][node], f['child'][node] + 1
            if not (v[a] < f['split'][node] or (v[a] == f['split'][node] and d[a] <= 0.)):
                c1, c2 = c2, c1
            if tp > tmax or tp <= 0.:
                node = c1
            elif tp < tmin:
                node = c2
            else:
                stack.append((c2, tmax))
                deepest = max(deepest, len(stack))
                node, tmax = c1, tp
        else:
            out.append(node)
            if not stack:
                return out, deepest
            tmin = tmax
            node, tmax = stack.pop()
