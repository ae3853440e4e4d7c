"""
Calls that select every search kernel instance of the streaming engine, and their host reference (test_search_cases_host.py for
what can be said without a device, test_gpu_search_instances.py on one).

A call is (scene, source or given rays, accel, Kd-tree or none, environment knobs, first or second call on the scene).  The host
driver (csrc/trc_stream.inc) picks its search kernels per call from 79 template instances:

  k_s_cull<KIND>                            the footprint map's cull, per source kind (0, 1 pillbox disc / rect, 2, 3 Buie, 7, 8 tabulated)
  k_s_fresh<KIND, FLAT, LDS>                the listed fresh rays; k_s_fresh2<KIND, FLAT, LDS>: its two-phase form for the Buie kinds
  k_s_bounce<GRIDM, LDS, FRESH, FLAT, SUN>  continued rays, and fresh rays outside the map; k_s_bounce_coop<FRESH, FLAT, SUN> on the large grid
  k_s_gen<FRESH, KIND>, k_s_gen_src<KIND>, k_s_walk<256, GRID>, k_s_exact      the general path

forms() restates that choice -- stream_plan and the search stages of trc_stream_decide (csrc/trc_forms.h) -- for a fact block: the
plain numbers the choice reads, which facts() takes for a call from the host-compiled check library (hc_scene_facts: the search
structures as trc_scene_create builds them, the footprint map).  predict() adds the per-bounce choice of plan_bounce / launch_bounce,
and lds_layout() restates trc_search_lds_layout (csrc/trc_bounds.h) with fresh_lds_parts / bounce_lds_parts to the byte.  What holds
the restatement to the library: the check library exports the header's own decisions (library_decide) and names (kernel_name,
library_ids), and test_search_cases_host.py / test_mega_cases_host.py compare them with forms() field by field -- for every call,
for 1e5 random fact blocks across every threshold, and ALL_INSTANCES with the ids the header can produce.

The scenes are shade_cases.room() -- general rotation, fillers in front of the room's own surfaces -- and a wedge of four surfaces,
each with a receiver that ends every ray and a twin: two plates of one frame and one size, a partial mirror at the lower index and
an absorber at the higher.  Every hit on the twin is an exact tie, which the reference's strict `<` gives to the lower index.
The sources hang over the scene, so that k_s_cull culls rays.  Every route over the same scene and rays shares one oracle trace.
"""
import collections
import ctypes as C
import functools
import os
import subprocess

import numpy as N

import fluxmap_scene as fs
import shade_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, REPS, SEED, E_MIN_SHARE = sc.N_RAYS, sc.REPS, sc.SEED, sc.E_MIN_SHARE
KiB = 1024
LIMIT_LDS = 150 * KiB               # trc_stream_form_fresh, trc_stream_form_bounce: `lds_need(...) <= 150 * 1024`
LIMIT_LIST = 65536                  # trc_stream_form_fresh: `n_list < 65536`
LIMIT_RECS = 40 * KiB               # trc_stream_form_general: `b_recs <= 40 * 1024`
LDS_MAX_ALLOWED = 160 * KiB - 512   # csrc/trc_forms.h
SMALL_SURFACES, TINY_SURFACES = 24, 4           # STREAM_SMALL_SURFACES; trc_stream_decide: STREAM_TINY_SURFACES
FP_CELLS = 512                      # stream_fp_prepare: M of a scene of at most 4096 surfaces
SFQ_CAP, SBC_CELLS, SBC_PAIRS, LDS_SLACK, OBB_LSTRIDE = 128, 4, 256, 16, 20         # csrc/trc_bounds.h
SBC_WAVE_BYTES = 2 * SBC_CELLS * 64 * 4 + 64 * 4 + SBC_PAIRS * 4 + 64 * 8 + 64 * 4
SB_THREADS, SW_THREADS, SW_LEAFCAP = 1024, 256, 16                                  # csrc/trc_forms.h
SRC_KIND = {'disk': 0, 'rect': 1, 'buie': 2, 'rbuie': 3, 'sun': 7, 'rsun': 8}      # trc_source_kind of the sources below
CSR = 0.3
PILLBOX_CONE = 0.02                 # half angle of the pillbox sources, rad
# from the source to the middle of the scene.  The margin of the footprint map is the cone's half angle times the distance: a wide one
# culls nothing beside the scene, a narrow one lists no ray that misses; the Buie disc (4.65 mrad) is moved away for the second
SOURCE_DISTANCE = {'disk': 6., 'rect': 6., 'sun': 6., 'rsun': 6., 'buie': 14., 'rbuie': 14.}
WEDGE_HALF_ANGLE = 0.17
SUN_TABLE = 'buie05'                # of tests/golden/sunshape.npz


# -- trc_search_lds_layout restated --------------------------------------------------------------------------------------------
PARTS = ('n_surf', 'stride', 'buie_bytes', 'occ_words', 'tables', 'sbox', 'flags', 'fp_offs', 'fp_list', 'grid_cells', 'grid_list',
         'queue_waves', 'coop_waves')
LdsParts = collections.namedtuple('LdsParts', PARTS)
LAYOUT = ('buie', 'occ', 'recs', 'obb', 'sbox', 'flags', 'fp_off', 'fp_list', 'grid_off', 'grid_list', 'queues', 'coop', 'end', 'slack')


def _r16(b):
    return (b + 15) & ~15


def lds_layout(p):
    """trc_search_lds_layout (csrc/trc_bounds.h): the byte offsets of LAYOUT for the parts p"""
    S, cur, slack, L = p.n_surf, 0, 0, {}
    L['buie'] = cur; cur += _r16(p.buie_bytes)
    L['occ'] = cur; cur += _r16(p.occ_words * 4)
    L['recs'] = cur; cur += S * p.stride * 8 if p.tables else 0
    L['obb'] = cur
    if p.tables:
        cur += _r16(S * OBB_LSTRIDE * 4); slack += LDS_SLACK
    L['sbox'] = cur; cur += S * 6 * 4 if p.sbox else 0
    L['flags'] = cur; cur += _r16(S * 4) if p.flags else 0
    L['fp_off'] = cur; cur += _r16(p.fp_offs * 2) if p.fp_offs else 0
    L['fp_list'] = cur
    if p.fp_offs:
        cur += p.fp_list * 2; slack += LDS_SLACK
    L['grid_off'] = cur; cur += ((p.grid_cells + 2) & ~1) * 2 if p.grid_cells else 0
    L['grid_list'] = cur
    if p.grid_cells:
        cur += p.grid_list * 2; slack += LDS_SLACK // 2 + (4 if p.grid_cells & 1 else 0)
    if p.queue_waves:
        cur = _r16(cur); slack += LDS_SLACK
    L['queues'] = cur; cur += p.queue_waves * (2 * SFQ_CAP * 4)
    L['coop'] = cur; cur += p.coop_waves * SBC_WAVE_BYTES
    L['end'], L['slack'] = cur, slack
    return L


def lds_need(p):
    """lds_need (csrc/trc_stream.inc): what a fits-in-LDS decision compares with its limit"""
    L = lds_layout(p)
    return L['end'] + L['slack']


def fresh_lds_parts(S, stride, Mc, n_list, buie_bytes, lds, queue_waves):
    """fresh_lds_parts (csrc/trc_stream.inc); buie_bytes: sizeof(trc_buie_fast) for a Buie kind, else 0"""
    return LdsParts(S, stride, buie_bytes, 0, lds, False, False, Mc * Mc + 1 if lds else 0, n_list if lds else 0, 0, 0, queue_waves, 0)


def bounce_lds_parts(S, stride, buie_bytes, lds, flags, grid_cells, grid_list, occ_words, coop_waves):
    """bounce_lds_parts (csrc/trc_stream.inc); buie_bytes: sizeof(trc_buie_fast) for a FRESH instance, else 0"""
    return LdsParts(S, stride, buie_bytes, occ_words, lds, lds, flags, 0, 0, grid_cells, grid_list if grid_cells else 0, 0, coop_waves)


# -- the host-compiled check libraries -------------------------------------------------------------------------------------------
_p = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_p)


@functools.lru_cache(maxsize=None)
def hostcheck():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    hc = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_hostcheck.so'))
    hs = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_sunshape_check.so'))
    hs.hs_sunshape_pack.restype = C.c_int
    hs.hs_sunshape_pack.argtypes = [C.c_int, _p, _p, _p, _p, _p]
    hs.hs_sunshape_rays.argtypes = [C.c_void_p, _p, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_long] + [_p] * 6
    return hc, hs


# -- the library's choice of kernel instances (csrc/trc_forms.h), through the check library -----------------------------------------
# A fact block: what the choice reads -- of the scene, of the call, of the footprint map, of the knobs -- in the order hostcheck.cpp
# takes it (hc_facts_of).  forms() here, shade_cases.shade_forms() / absorb_forms() and mega_cases.plan() / engine() / ordered() restate
# the choice from such a block; library_decide() is what the header itself makes of it, and test_*_cases_host.py hold the two together.
FACT_KEYS = ('n_surf', 'stride', 'accel_ok', 'accel_kd_ok', 'has_kd', 'kd_nodes', 'kd_nleaf', 'kd_nalways', 'kd_depth', 'grid_ok', 'big_ok',
             'grid_cells', 'grid_list', 'brute_list', 'n_unbounded', 'big_occ_words', 'n_fm_edges', 'fms_bytes', 'n_extra', 'fm_bins', 'chart',
             'transfer', 'splits', 'all_flat', 'simple', 'cls_moving', 'cls_all', 'any_term',
             'n', 'flags', 'src_kind', 'spec', 'carry', 'mat_dev', 'term_ok',
             'fp_use', 'fp_n_list', 'fp_M', 'fp_Mc', 'fp_has_generic', 'fp_cdf_end', 'fp_coverage', 'fp_ucoverage', 'fp_umask_words', 'fp_Mu', 'fp_Mv',
             'k_search', 'k_fresh', 'k_bounce', 'k_first', 'k_coop', 'k_absorb', 'k_umask')
TRACE_ACCEL, TRACE_STREAM, TRACE_MEGAKERNEL = 1, 4, 8          # include/tracer_amd.h
ENGINE_KEYS = ('use_stream', 'refused', 'engine_mode')
MEGA_KEYS = ('m32', 'mega_threads', 'mega_lds', 'mega_lds_tally', 'mega_lds_scene')
PLAN_KEYS = ('plan_ok', 'mode', 'lds_walk', 'walk_ok', 'decided')
FORM_KEYS = ('src_kind', 'gridm', 'small_scene', 'n_shk', 'multi', 'cull_lu', 'cull_lv', 'ulisted_share', 'coop', 'use_fp', 'use_fused', 'use_first',
             'use_absorb', 'absorb_inline', 'lds_inline', 'general_share', 'listed_share', 'search', 'lds_recs', 'lds_tally', 'lds_tables', 'lds_extra',
             'lds_fm_bins', 'bg_occ_words', 'shade_term_cls', 'split_terminal')
STAGES = ('gen0', 'gen', 'walk', 'exact', 'cull', 'cull_u', 'fresh', 'fresh_one', 'bounce', 'first', 'absorb')
NO_STAGE = (None, 0, 0)             # (kernel name, threads, bytes of dynamic LDS) of a stage the call does not have
FLOAT_KEYS = ('ulisted_share', 'general_share', 'listed_share')


def blank_facts(**kw):
    """a fact block of a scene with its boxes built, no tree, no grid, no map, given rays and the knobs unset"""
    f = dict((k, 0) for k in FACT_KEYS)
    f.update(accel_ok=1, src_kind=-1, term_ok=1, k_search=2, k_fresh=1, k_bounce=1, k_coop=1, k_absorb=-1, k_umask=1)
    f.update(kw)
    return f


def kd_desc(f):
    """the flattened tree as the check library takes it (the arrays stay with `f`)"""
    from tracer_amd import _cabi
    kd = _cabi.KdTreeDesc()
    kd.n_nodes, kd.n_leaf_surfs, kd.n_always = len(f['flag']), len(f['leaf_surfs']), len(f['always_relevant'])
    i32 = C.POINTER(C.c_int32)
    for k in ('flag', 'child', 'leaf_off', 'leaf_cnt', 'leaf_surfs', 'always_relevant'):
        setattr(kd, k, f[k].ctypes.data_as(i32))
    kd.split = _ptr(f['split'])
    for k in range(6):
        kd.bounds[k] = f['bounds'][k]
    return kd


def scene_facts(cs, kd=None, desc=None, edges=None, chart=False, force32=False):
    """the fact block of a compiled scene as the library gathers it (hc_scene_facts: trc_scene_facts_fill on the structures of
    trc_scene_create, the tree `kd` flattened, the footprint map of the descriptor `desc`), with the flux maps `edges` = {surface: (u
    edges, v edges)}; the call and the knobs are left blank"""
    f = blank_facts()
    v = N.array([float(f[k]) for k in FACT_KEYS])
    hc = hostcheck()[0]
    d = resolved(desc) if desc is not None else None
    assert hc.hc_scene_facts(cs.n_surf, cs.descs, C.byref(kd_desc(kd)) if kd is not None else None, C.byref(d) if d is not None else None,
                             FP_CELLS, int(force32), _ptr(v)) == 0
    f = dict((k, (float(x) if k.startswith('fp_c') or k == 'fp_ucoverage' else int(x))) for k, x in zip(FACT_KEYS, v))
    edges = edges or {}
    f.update(n_fm_edges=sum(len(u) + len(w) for u, w in edges.values()), fms_bytes=len(edges) * sc.SIZEOF_FLUXMAPDEV, n_extra=len(cs.extra),
             fm_bins=sum((len(u) - 1) * (len(w) - 1) for u, w in edges.values()), chart=int(chart))
    return f


_NAMES = {}


def kernel_name(ident):
    """trc_kernel_name of (family, five arguments); None: no kernel"""
    ident = tuple(int(x) for x in ident)
    if ident not in _NAMES:
        buf = C.create_string_buffer(96)
        n = hostcheck()[0].hc_kernel_name((C.c_int * 6)(*ident), buf, 96)
        assert 0 <= n < 96
        _NAMES[ident] = buf.value.decode() or None
    return _NAMES[ident]


def library_decide(blocks):
    """every decision of trc_forms.h for the fact blocks: per block a dict of ENGINE_KEYS, MEGA_KEYS + 'mega', 'ord_mode', 'ord', PLAN_KEYS and,
    where 'decided', FORM_KEYS, the STAGES as (kernel name, threads, LDS bytes) and 'shk': per shading kernel (name, threads, LDS bytes,
    class, tables in LDS, bins in LDS)"""
    hc = hostcheck()[0]
    rows = N.ascontiguousarray([[float(b[k]) for k in FACT_KEYS] for b in blocks])
    per = 3 + 11 + 7 + 5 + len(FORM_KEYS) + 8 * len(STAGES) + 3 * 11
    out = N.zeros((len(rows), per))
    assert hc.hc_forms_decide(C.c_long(len(rows)), _ptr(rows), _ptr(out)) == per
    res = []
    for r in out:
        it = iter(r)
        take = lambda n: [next(it) for _ in range(n)]
        num = lambda keys: dict((k, (v if k in FLOAT_KEYS else int(v))) for k, v in zip(keys, take(len(keys))))
        d = num(ENGINE_KEYS)
        d.update(num(MEGA_KEYS))
        d['mega'] = kernel_name(take(6))
        d.update(num(('ord_mode',)))
        d['ord'] = kernel_name(take(6))
        d.update(num(PLAN_KEYS))
        if d['decided']:
            d.update(num(FORM_KEYS))
            for st in STAGES:
                d[st] = (kernel_name(take(6)),) + tuple(int(x) for x in take(2))
            shk = [(kernel_name(take(6)),) + tuple(int(x) for x in take(5)) for _ in range(3)]
            d['shk'] = shk[:d['n_shk']]
            assert all(x == (None, 0, 0, 0, 0, 0) for x in shk[d['n_shk']:])
        res.append(d)
    return res


def library_ids(ints=(-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 128, 256, 512, 1024)):
    """the names of every kernel id trc_forms.h can produce (trc_kernel_id_valid), integer arguments tried over `ints`"""
    hc = hostcheck()[0]
    cap = 4096
    out = (C.c_int * (6 * cap))()
    n = hc.hc_kernel_ids((C.c_int * len(ints))(*ints), len(ints), out, cap)
    assert 0 < n <= cap
    return [kernel_name(out[6 * i:6 * i + 6]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def sun_table():
    """(angles, intensities, packed table, theta_c, u_c) of the tabulated sunshape, packed by the host build of the library's packer"""
    g = N.load(os.path.join(ROOT, 'tests', 'golden', 'sunshape.npz'))
    a = N.ascontiguousarray(g[SUN_TABLE + '_angles'], dtype=float)
    I = N.ascontiguousarray(g[SUN_TABLE + '_intensity'], dtype=float)
    tab = N.empty(3 * a.size)
    tc, uc = C.c_double(), C.c_double()
    assert hostcheck()[1].hs_sunshape_pack(a.size, _ptr(a), _ptr(I), _ptr(tab), C.byref(tc), C.byref(uc)) == 1
    return a, I, tab, tc.value, uc.value


def resolved(desc):
    """a sunshape descriptor as the library resolves it (p[5..7], the table's address in buie[0]); the others as they are"""
    from tracer_amd import _cabi
    if desc.kind not in (SRC_KIND['sun'], SRC_KIND['rsun']):
        return desc
    a, I, tab, tc, uc = sun_table()
    d = _cabi.SourceDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    d.p[5], d.p[6], d.p[7] = tc, uc, float(a.size)
    d.buie[0] = N.array([tab.ctypes.data], dtype=N.uint64).view(N.float64)[0]
    return d


# -- the scenes ------------------------------------------------------------------------------------------------------------------
def wedge(dish):
    """(assembly, T): four surfaces under the room's rotation -- the twin and, facing it, a mirror captured in full (a plate, or a
    shallow dish), above the receiver that ends every ray"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.paraboloid import ParabolicDishGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    T = N.dot(translate(-3.7, 5.2, 1.9), N.dot(rotx(-0.5), N.dot(roty(0.8), rotz(-0.9))))
    # a groove of half angle WEDGE_HALF_ANGLE, open at the top and at the bottom, turned about z: a ray that enters is sent from side to
    # side up to six times, and leaves at the top, or through the slit onto the receiver
    half, alpha, h = N.pi / 2., WEDGE_HALF_ANGLE, 2.4
    x, z = 0.15 + h / 2. * N.sin(alpha), h / 2. * N.cos(alpha) + 0.1
    twin = N.dot(rotz(1.2), N.dot(translate(-x, 0., z), roty(half - alpha)))
    facing = N.dot(rotz(1.2), N.dot(translate(x + (0.05 if dish else 0.), 0.03, z), N.dot(roty(alpha - half), rotz(0.1))))
    parts = [(ParabolicDishGM(h, 5.) if dish else RectPlateGM(h, 2.4), opt.ReflectiveDetector(0.04), facing),         # (captured in full)
             (RectPlateGM(h, 2.2), opt.Reflective(0.3), twin), (RectPlateGM(h, 2.2), opt.Lambertian(1.), twin),
             (RectPlateGM(1.2, 1.6), opt.LambertianReceiver(1.), N.dot(translate(0.05, -0.6, 0.), rotz(1.6)))]
    return Assembly(objects=[AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr in parts]), T


def fill_for(what, kind):
    """
    The filler count of a room, from the restated sums alone (S = fillers + the room's own surfaces; every sum below leaves out parts
    that only add -- grid, footprint lists, Buie table -- so the scene is on the intended side whatever those come to, which
    test_search_cases_host.py then checks with them in):
      'mid'   the fewest that leave `small_scene` (S > 24); its records stay within 40 KiB (k_s_exact's lds_recs = 1)
      'full'  the fewest that put the records alone beyond 40 KiB, and the tables of k_s_fresh (records, oriented boxes, 32 KiB of
              cell offsets at M = 512) and of k_s_bounce (records, oriented boxes, boxes) beyond 150 KiB
    """
    own = {'flat': 13, 'curved': 16}[kind] + 3
    stride = 21             # (14 + the polygon's 6 parameters) | 1
    if what == 'mid':
        S = SMALL_SURFACES + 1
        assert S * stride * 8 <= LIMIT_RECS
        return S - own
    S = own
    while not (S * stride * 8 > LIMIT_RECS and
               lds_need(fresh_lds_parts(S, stride, FP_CELLS // 4, 0, 0, True, 0)) > LIMIT_LDS and
               lds_need(bounce_lds_parts(S, stride, 0, True, False, 0, 0, 0, 0)) > LIMIT_LDS):
        S += 1
    return S - own


# name: (builder, kind of room, fillers)
SCENES = {
    'wedge': ('wedge', 'flat', 0), 'wedge-dish': ('wedge', 'curved', 0),
    'flat': ('room', 'flat', 0), 'curved': ('room', 'curved', 0),
    'curved-mid': ('room', 'curved', fill_for('mid', 'curved')),
    'flat-full': ('room', 'flat', fill_for('full', 'flat')), 'curved-full': ('room', 'curved', fill_for('full', 'curved')),
}


class Scene(object):
    """a scene built: compiled table, frames, the mapped surface, the surface captured in full, the twin and the receiver"""
    def __init__(self, name):
        from tracer_amd.scene import compile_scene
        self.name = name
        builder, self.kind, self.n_fill = SCENES[name]
        if builder == 'wedge':
            asm, self.T = wedge(self.kind == 'curved')
            self.full_surf, self.twin, self.terminal = 0, (1, 2), 3
            self.map_surf = self.terminal
            self.edges = {self.map_surf: (fs.nonuniform(-0.5, 0.6, 13), N.linspace(-0.8, 0.5, 10))}
            self.reach = 1.5
        else:
            asm, self.T = sc.room(self.kind, self.n_fill, ends=True)
            self.map_surf, self.full_surf = self.n_fill + sc.MAP_TILE, self.n_fill + sc.FULL_WALL
            self.edges = {self.map_surf: sc.MAP_EDGES}
            self.reach = 2.7
        self.cs = compile_scene(asm)
        S = self.cs.n_surf
        if builder == 'room':
            self.twin, self.terminal = (S - 3, S - 2), S - 1
        self.frames = [N.array(s._temp_frame) for s in self.cs.surfaces]
        self.captured = [i for i in range(S) if self.cs.capture[i]]
        assert sorted(self.captured) == sorted(set([self.map_surf, self.full_surf, self.terminal]))
        self.stride = sc.record_stride(self.cs)
        gm = sc._names('GM_')
        self.flat = all(gm[self.cs.descs[i].gm_kind] in sc.FLAT_KINDS for i in range(S))
        self.W, self.spec = 0, False

    def source(self, src):
        """the pending bundle of source kind `src` over the open top, aimed like fluxmap_scene.source and hanging over the scene on every
        side (its own seed travels with it)"""
        from tracer_amd import sources
        d = N.r_[0.32, 0.22, -1.]
        d = d / N.linalg.norm(d)
        c = N.r_[0., 0., 1.2] - SOURCE_DISTANCE[src] * d
        centre, d = N.c_[N.dot(self.T[:3, :3], c) + self.T[:3, 3]], N.dot(self.T[:3, :3], d)
        R, kw = self.reach, dict(flux=1000., seed=SEED)
        if src == 'disk':
            return sources.disk_bundle(N_RAYS, centre, d, R, PILLBOX_CONE, **kw)
        if src == 'rect':
            return sources.rect_bundle(N_RAYS, centre, d, 1.9 * R, 1.8 * R, PILLBOX_CONE, **kw)
        if src == 'buie':
            return sources.buie_sunshape(N_RAYS, centre, d, R, CSR, **kw)
        if src == 'rbuie':
            return sources.rect_buie_sunshape(N_RAYS, centre, d, 1.9 * R, 1.8 * R, CSR, **kw)
        a, I = sun_table()[:2]
        if src == 'sun':
            return sources.tabulated_sunshape(N_RAYS, centre, d, R, a, I, **kw)
        assert src == 'rsun'
        return sources.rect_tabulated_sunshape(N_RAYS, centre, d, 1.9 * R, 1.8 * R, a, I, **kw)

    def desc(self, src):
        """the source's descriptor without a device (a tabulated sunshape's table is named on one only)"""
        return self.source(src)._src_desc

    def min_energy(self, src):
        return E_MIN_SHARE * self.desc(src).energy

    @functools.lru_cache(maxsize=None)
    def rays(self, src):
        """(vertices, directions, energy, ray ids) of the source's rays: the oracle's, or the host-compiled sampler's for a tabulated
        sunshape (the oracle has no generator for it; test_sunshape.py holds the sampler to the table)"""
        from oracle import engine, sources
        desc = self.desc(src)
        if src in ('sun', 'rsun'):
            a, I, tab, tc, uc = sun_table()
            out = [N.empty(N_RAYS) for _ in range(6)]
            hostcheck()[1].hs_sunshape_rays(C.addressof(desc), _ptr(tab), a.size, tc, uc, SEED, 0, N_RAYS, *[_ptr(o) for o in out])
            return N.array(out[:3]), N.array(out[3:]), N.full(N_RAYS, desc.energy), N.arange(N_RAYS, dtype=N.uint64)
        return sources.generate(engine.source_from_desc(desc), N_RAYS, SEED, 0)

    @functools.lru_cache(maxsize=None)
    def sizes(self, src):
        """hc_search_sizes of the scene and the source (None: no source): what the choice of search kernels reads off them"""
        out = N.zeros(14)
        d = resolved(self.desc(src)) if src else None
        hostcheck()[0].hc_search_sizes(self.cs.n_surf, self.cs.descs, C.byref(d) if d is not None else None, FP_CELLS, _ptr(out))
        keys = ('grid_ok', 'grid_cells', 'grid_list', 'big_ok', 'occ_words', 'brute_list', 'unbounded', 'fp_ok', 'Mc', 'n_list', 'coverage',
                'has_generic', 'cdf_end', 'buie_bytes')
        return dict((k, (float(v) if k in ('coverage', 'cdf_end') else int(v))) for k, v in zip(keys, out))

    @functools.lru_cache(maxsize=None)
    def facts(self, src, kd=False, force32=False):
        """scene_facts of the scene with its flux map, the source (None: no source) and its Kd-tree (kd): nobody changes it"""
        return scene_facts(self.cs, self.kdtree().flat() if kd else None, self.desc(src) if src else None, self.edges, force32=force32)

    @functools.lru_cache(maxsize=None)
    def kdtree(self):
        from tracer_amd.accel_tree import KdTree
        builder, kind, n_fill = SCENES[self.name]
        from tracer_amd.boundary_shape import BoundaryBox
        asm = wedge(kind == 'curved')[0] if builder == 'wedge' else sc.room(kind, n_fill, ends=True)[0]
        for o in asm.get_objects():         # (the tree is built from boxes the objects bring: one per object, around the largest piece)
            o.add_boundary(BoundaryBox([[-2.1, -2.1, -1.4], [2.1, 2.1, 1.4]]))
        return KdTree(asm, 8 + 1.3 * N.log(self.cs.n_surf), min_leaf=1)


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name)


# -- the calls -------------------------------------------------------------------------------------------------------------------
_Call = collections.namedtuple('Call', 'name scene src given accel kd env scene_env second targets')


class Call(_Call):
    """scene: of SCENES; src: of SRC_KIND; given: the source's rays handed over as a bundle; accel, kd: trace_fast's accel, a Kd-tree set on
    the scene; env: knobs around the trace; scene_env: knobs around the scene's creation; second: the call is made twice on one scene
    and checked the second time; targets: the instances the call is there for.  The attributes below are what
    test_gpu_shade_instances._check reads of a case."""
    cs = property(lambda self: scene(self.scene).cs)
    edges = property(lambda self: scene(self.scene).edges)
    map_surf = property(lambda self: scene(self.scene).map_surf)
    full_surf = property(lambda self: scene(self.scene).full_surf)
    captured = property(lambda self: scene(self.scene).captured)
    min_energy = property(lambda self: scene(self.scene).min_energy(self.src))
    W, spec = 0, False

    def bundle(self, given):
        from tracer_amd.ray_bundle import RayBundle
        if not given:
            return scene(self.scene).source(self.src)
        v, d, e, rid = scene(self.scene).rays(self.src)
        return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())


def _call(name, scn, src, targets, given=False, accel=True, kd=False, env=None, scene_env=None, second=False):
    return Call(name, scn, src, given, accel, kd, tuple(sorted((env or {}).items())), tuple(sorted((scene_env or {}).items())), second,
                tuple(targets))


def _t(x):
    return 'true' if x else 'false'


def _bounce(gridm, lds, fresh, flat, sun):
    return 'k_s_bounce<%d, %s, %s, %s, %s>' % (gridm, _t(lds), _t(fresh), _t(flat), _t(sun))


def _coop(fresh, flat, sun):
    return 'k_s_bounce_coop<%s, %s, %s>' % (_t(fresh), _t(flat), _t(sun))


def _calls():
    out = []
    F32, NOCOOP, FIRST = dict(TRC_GRID_FORCE32=1), dict(TRC_STREAM_COOP=0), dict(TRC_STREAM_FIRST=1)
    # the footprint route: six source kinds over a room of flat / of curved surfaces, tables in LDS (no fillers) / in global memory.
    # The rays the map leaves out (a Buie aureole, a table's tail) go through k_s_bounce<.., FRESH> in the small rooms and through
    # the general path in the filled ones (k_s_exact with its records in global memory)
    more = {'flat/sun': [_bounce(1, True, True, False, True)], 'flat/buie': [_bounce(1, True, True, False, False)],
            'flat-full/buie': ['k_s_gen_src<2>', 'k_s_walk<256, true>', 'k_s_exact'], 'flat-full/rbuie': ['k_s_gen<true, 3>'],
            'flat-full/sun': ['k_s_gen<true, 7>'], 'flat-full/rsun': ['k_s_gen<true, 8>']}
    for scn, flat, lds in (('flat', True, True), ('curved', False, True), ('flat-full', True, False), ('curved-full', False, False)):
        for src, k in sorted(SRC_KIND.items(), key=lambda x: x[1]):
            name = '%s/%s' % (scn, src)
            fresh = 'k_s_fresh%s<%d, %s, %s>' % ('2' if k in (2, 3) else '', k, _t(flat), _t(lds))
            out.append(_call(name, scn, src, ['k_s_cull<%d>' % k, fresh, _bounce(1, lds, False, flat, False)] + more.get(name, [])))
            if k in (2, 3):         # most listed rays hit: the second call on the scene goes back to k_s_fresh
                out.append(_call(name + '/second', scn, src, ['k_s_fresh<%d, %s, %s>' % (k, _t(flat), _t(lds))], second=True))
    # fresh rays outside the map through k_s_bounce<.., FRESH> in a scene that is not small (TRC_STREAM_FIRST=1)
    out += [_call('flat-full/given/first', 'flat-full', 'buie', [_bounce(1, False, True, False, False)], given=True, env=FIRST),
            _call('flat-full/sun/first', 'flat-full', 'sun', [_bounce(1, False, True, False, True)], env=FIRST)]
    # the general path: given rays; the pillbox kinds without a map; continued rays; records in LDS (the mid room); the Kd walk; all boxes
    out += [_call('flat-full/disk/nomap', 'flat-full', 'disk', ['k_s_gen_src<0>'], env=dict(TRC_STREAM_FRESH=0)),
            _call('flat-full/rect/nomap', 'flat-full', 'rect', ['k_s_gen_src<1>'], env=dict(TRC_STREAM_FRESH=0)),
            _call('curved-mid/given', 'curved-mid', 'buie', ['k_s_gen<true, -1>', 'k_s_walk<256, true>', 'k_s_exact'], given=True),
            _call('curved-mid/buie/nobounce', 'curved-mid', 'buie', ['k_s_gen<false, -1>', 'k_s_exact'], env=dict(TRC_STREAM_BOUNCE=0)),
            _call('curved-mid/buie/kd', 'curved-mid', 'buie', ['k_s_walk<256, false>'], kd=True, env=dict(TRC_STREAM_SEARCH=1)),
            _call('curved-mid/given/boxes', 'curved-mid', 'buie', ['k_s_walk<256, false>'], given=True, accel=False)]
    # every bounded surface (accel = False): tables in LDS / in global memory, continued and fresh rays
    out += [_call('flat/given/boxes', 'flat', 'buie', [_bounce(0, True, True, False, False), _bounce(0, True, False, True, False)], given=True, accel=False),
            _call('flat/sun/boxes', 'flat', 'sun', [_bounce(0, True, True, False, True)], accel=False),
            _call('curved/buie/boxes', 'curved', 'buie', [_bounce(0, True, False, False, False)], accel=False),
            _call('flat-full/given/boxes', 'flat-full', 'buie', [_bounce(0, False, True, False, False), _bounce(0, False, False, True, False)],
                  given=True, accel=False, env=FIRST),
            _call('flat-full/sun/boxes', 'flat-full', 'sun', [_bounce(0, False, True, False, True)], accel=False, env=FIRST),
            _call('curved-full/disk/boxes', 'curved-full', 'disk', [_bounce(0, False, False, False, False)], accel=False)]
    # surface by surface (at most four surfaces)
    out += [_call('wedge/buie', 'wedge', 'buie', [_bounce(3, False, True, False, False), _bounce(3, False, False, True, False)]),
            _call('wedge/given', 'wedge', 'buie', [_bounce(3, False, True, False, False)], given=True),
            _call('wedge/sun', 'wedge', 'sun', [_bounce(3, False, True, False, True)]),
            _call('wedge-dish/buie', 'wedge-dish', 'buie', [_bounce(3, False, False, False, False)])]
    # the large grid, forced at the scene's creation: waves that share their rays' tests, or (TRC_STREAM_COOP=0) every lane its own ray
    out += [_call('flat/given/grid32', 'flat', 'buie', [_coop(True, True, False), _coop(False, True, False)], given=True, scene_env=F32),
            _call('flat/sun/grid32', 'flat', 'sun', [_coop(True, True, True)], scene_env=F32),
            _call('curved/given/grid32', 'curved', 'buie', [_coop(True, False, False), _coop(False, False, False)], given=True, scene_env=F32),
            _call('curved/sun/grid32', 'curved', 'sun', [_coop(True, False, True)], scene_env=F32),
            _call('flat/given/grid32/lanes', 'flat', 'buie', [_bounce(2, False, True, False, False), _bounce(2, False, False, True, False)],
                  given=True, env=NOCOOP, scene_env=F32),
            _call('flat/sun/grid32/lanes', 'flat', 'sun', [_bounce(2, False, True, False, True)], env=NOCOOP, scene_env=F32),
            _call('curved/disk/grid32/lanes', 'curved', 'disk', [_bounce(2, False, False, False, False)], env=NOCOOP, scene_env=F32)]
    # the terminal split crossed with k_s_bounce: the list finished by k_s_absorb, and no list
    out += [_call('flat/disk/absorb-list', 'flat', 'disk', [_bounce(1, True, False, True, False)], env=dict(TRC_STREAM_ABSORB=1)),
            _call('curved-full/buie/absorb-off', 'curved-full', 'buie', [_bounce(1, False, False, False, False)], env=dict(TRC_STREAM_ABSORB=0))]
    # the pillbox kinds through k_s_bounce<.., FRESH> / k_s_bounce_coop<true, ..>: no map (TRC_STREAM_FRESH=0) in a small room and on
    # the large grid, where the FRESH instance takes every fresh ray (the source kind is a run-time switch of these instances)
    NOMAP = dict(TRC_STREAM_FRESH=0)
    out += [_call('flat/disk/nomap', 'flat', 'disk', [_bounce(1, True, True, False, False)], env=NOMAP),
            _call('curved/rect/nomap', 'curved', 'rect', [_bounce(1, True, True, False, False)], env=NOMAP),
            _call('flat/rect/grid32/nomap', 'flat', 'rect', [_coop(True, True, False)], env=NOMAP, scene_env=F32),
            _call('curved/disk/grid32/nomap', 'curved', 'disk', [_coop(True, False, False)], env=NOMAP, scene_env=F32),
            _call('flat/disk/grid32/lanes/nomap', 'flat', 'disk', [_bounce(2, False, True, False, False)], env=dict(NOCOOP, **NOMAP), scene_env=F32),
            _call('flat/rect/boxes/nomap', 'flat', 'rect', [_bounce(0, True, True, False, False)], accel=False, env=NOMAP)]
    # the terminal split crossed with the other forms of the search -- all boxes, surface by surface, the large grid lane by lane: the
    # list behind k_s_bounce, and no split; k_s_bounce_coop never finishes terminal hits itself (the list is its default): no split
    LIST, OFF = dict(TRC_STREAM_ABSORB=1), dict(TRC_STREAM_ABSORB=0)
    out += [_call('flat/given/boxes/absorb-list', 'flat', 'buie', [_bounce(0, True, False, True, False)], given=True, accel=False, env=LIST),
            _call('curved/buie/boxes/absorb-off', 'curved', 'buie', [_bounce(0, True, False, False, False)], accel=False, env=OFF),
            _call('wedge/buie/absorb-list', 'wedge', 'buie', [_bounce(3, False, False, True, False)], env=LIST),
            _call('wedge-dish/buie/absorb-off', 'wedge-dish', 'buie', [_bounce(3, False, False, False, False)], env=OFF),
            _call('flat/given/grid32/lanes/absorb-list', 'flat', 'buie', [_bounce(2, False, False, True, False)], given=True,
                  env=dict(NOCOOP, **LIST), scene_env=F32),
            _call('curved/disk/grid32/lanes/absorb-off', 'curved', 'disk', [_bounce(2, False, False, False, False)], env=dict(NOCOOP, **OFF),
                  scene_env=F32),
            _call('curved/given/grid32/absorb-off', 'curved', 'buie', [_coop(False, False, False)], given=True, env=OFF, scene_env=F32),
            _call('flat/sun/grid32/absorb-off', 'flat', 'sun', [_coop(False, True, False)], env=OFF, scene_env=F32)]
    assert len(set(c.name for c in out)) == len(out)
    return out


CALLS = _calls()
CALL = dict((c.name, c) for c in CALLS)

ALL_INSTANCES = ['k_s_cull<%d>' % k for k in (0, 1, 2, 3, 7, 8)] + \
    ['k_s_fresh<%d, %s, %s>' % (k, _t(f), _t(l)) for k in (0, 1, 2, 3, 7, 8) for f in (1, 0) for l in (1, 0)] + \
    ['k_s_fresh2<%d, %s, %s>' % (k, _t(f), _t(l)) for k in (2, 3) for f in (1, 0) for l in (1, 0)] + \
    [_bounce(g, l, False, f, False) for g, l in ((0, 1), (0, 0), (1, 1), (1, 0), (2, 0), (3, 0)) for f in (1, 0)] + \
    [_bounce(g, l, True, False, s) for g, l in ((0, 1), (0, 0), (1, 1), (1, 0), (2, 0), (3, 0)) for s in (0, 1)] + \
    [_coop(*x) for x in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))] + \
    ['k_s_walk<256, true>', 'k_s_walk<256, false>'] + \
    ['k_s_gen<false, -1>', 'k_s_gen<true, -1>', 'k_s_gen<true, 3>', 'k_s_gen<true, 7>', 'k_s_gen<true, 8>'] + \
    ['k_s_gen_src<%d>' % k for k in (0, 1, 2)] + ['k_s_exact']
# instances that no input selects: {instance: the condition in the host code that excludes it}
UNREACHABLE = {}
FAMILIES = ('k_s_cull', 'k_s_fresh', 'k_s_fresh2', 'k_s_bounce', 'k_s_bounce_coop', 'k_s_walk', 'k_s_gen', 'k_s_gen_src', 'k_s_exact')


# -- the choice of kernels restated ---------------------------------------------------------------------------------------------------
def facts(call):
    """the fact block of a call: the scene and the footprint map as the library gathers them (scene_facts), the call and the knobs as the test makes it (the streaming engine forced: a call of N_RAYS rays)"""
    s = scene(call.scene)
    env, senv = dict(call.env), dict(call.scene_env)
    src = None if call.given else call.src
    f = dict(s.facts(src, call.kd, bool(int(senv.get('TRC_GRID_FORCE32', 0)))))
    f.update(n=N_RAYS, flags=TRACE_STREAM | (TRACE_ACCEL if call.accel else 0), src_kind=SRC_KIND[call.src] if src else -1,
             term_ok=int(s.min_energy(call.src) >= 0.))
    f.update(k_search=int(env.get('TRC_STREAM_SEARCH', 2)), k_fresh=int(int(env.get('TRC_STREAM_FRESH', 1)) != 0),
             k_bounce=int(int(env.get('TRC_STREAM_BOUNCE', 1)) != 0), k_first=int(int(env.get('TRC_STREAM_FIRST', 0)) != 0),
             k_coop=int(int(env.get('TRC_STREAM_COOP', 1)) != 0), k_absorb=int(env.get('TRC_STREAM_ABSORB', -1)),
             k_umask=int(int(env.get('TRC_STREAM_UMASK', 1)) != 0))
    if not f['k_fresh']:            # stream_fp_prepare: TRC_STREAM_FRESH=0 makes no map
        f.update((k, 0) for k in FACT_KEYS if k.startswith('fp_'))
    return f


BUIE_BYTES = 9472                   # sizeof(trc_buie_fast) (csrc/trc_core.h); hc_search_sizes reports it, test_search_cases_host.py compares
SC_THREADS, SC_GEN_CAP = 512, 1024  # csrc/trc_forms.h: k_s_cull's threads, the general-path rays its workgroup collects
OCC_COOP, OCC_LANES = 80 * KiB, 96 * KiB        # ... the occupancy bits of the large grid in LDS, beside k_s_bounce_coop's blocks / in k_s_bounce<2>


def forms(f):
    """
    stream_plan and the search stages of trc_stream_decide (csrc/trc_forms.h: general, fresh, bounce) restated for a fact block: a dict
    of the decisions -- PLAN_KEYS without 'decided', the FORM_KEYS they set, the STAGES but 'absorb' as (kernel name, threads, LDS bytes)
    -- with the byte sums behind the two fits-in-LDS decisions (need_fresh, need_bounce) and what predict() reads beside them (grid,
    kind, fresh_two, fresh_in_lds, in_lds, sun).  Only 'plan_ok' where the scene has no streaming form.
    """
    S, stride = f['n_surf'], f['stride']
    d = {}
    # stream_plan
    waves = SW_THREADS // 64

    def walk_lds(mode):
        depth = 1
        if mode == 1:
            shared = 6 * S * 4 + 2 * f['kd_nodes'] * 4 + f['kd_nleaf'] * 2 + 32
            depth = max(f['kd_depth'], 1)
        elif mode == 2:
            shared = 6 * S * 4 + (f['grid_cells'] + 1 + 2 + f['grid_list']) * 2 + 32
        else:
            shared = 6 * S * 4 + 8 + f['brute_list'] * 2 + 32
        return shared + waves * (depth * 64 * 4 + SW_LEAFCAP * 64 * 2 + 64 * 4)
    mode = 0
    if f['accel_ok'] and f['flags'] & TRACE_ACCEL:
        kd_fits = f['accel_kd_ok'] and S <= 65535 and walk_lds(1) <= LDS_MAX_ALLOWED
        mode = 1 if f['k_search'] == 1 and kd_fits else 2 if f['grid_ok'] else 3 if f['big_ok'] else 1 if kd_fits else 0
    d['plan_ok'] = int(bool(f['accel_ok']) and not (mode == 0 and S > 65535))
    if not d['plan_ok']:
        return d
    d['mode'] = mode
    walk_ok = mode != 3 and walk_lds(mode) <= LDS_MAX_ALLOWED
    d['walk_ok'] = int(walk_ok)
    d['lds_walk'] = walk_lds(mode) if walk_ok else 0
    # trc_stream_decide
    gridm = 1 if mode == 2 else 2 if mode == 3 else 0
    small = S <= SMALL_SURFACES and mode != 1 and walk_ok
    d['small_scene'] = int(small)
    if small and S <= TINY_SURFACES:
        gridm = 3
    d['gridm'] = gridm
    d['search'] = mode if walk_ok else 2
    # the general path
    kind = d['src_kind'] = d['kind'] = f['src_kind']
    recs = S * stride * 8
    d['lds_recs'] = int(0 < recs <= LIMIT_RECS)
    d['grid'] = mode == 2                                   # ... k_s_walk<256, GRID>
    d['gen0'] = ({2: 'k_s_gen_src<2>', 3: 'k_s_gen<true, 3>', 0: 'k_s_gen_src<0>', 1: 'k_s_gen_src<1>', 7: 'k_s_gen<true, 7>',
                  8: 'k_s_gen<true, 8>'}.get(kind, 'k_s_gen<true, -1>'), 256, 0)
    d['gen'] = ('k_s_gen<false, -1>', 256, 0)
    d['walk'] = ('k_s_walk<256, %s>' % _t(d['grid']), SW_THREADS, d['lds_walk'])
    d['exact'] = ('k_s_exact', 256, recs if d['lds_recs'] else 0)
    # the footprint route
    flat = bool(f['all_flat'])
    d['use_fp'] = int(bool(f['fp_use']))
    d['general_share'], d['listed_share'], d['ulisted_share'] = 0., 1., 0.
    d['cull_lu'] = d['cull_lv'] = 0
    d['cull'] = d['cull_u'] = d['fresh'] = d['fresh_one'] = NO_STAGE
    if d['use_fp']:
        buie = kind in (2, 3)
        threads = 1024 if flat else 768                     # SF_THREADS(flat)
        qw = threads // 64 if buie else 0
        bb = BUIE_BYTES if buie else 0
        d['need_fresh'] = lds_need(fresh_lds_parts(S, stride, f['fp_Mc'], f['fp_n_list'], bb, True, qw))
        in_lds = f['fp_n_list'] < LIMIT_LIST and d['need_fresh'] <= LIMIT_LDS
        request = lds_need(fresh_lds_parts(S, stride, f['fp_Mc'], f['fp_n_list'], bb, in_lds, qw)) + 16
        lds_cull = f['fp_M'] * f['fp_M'] // 8 + (SC_GEN_CAP + 4) * 4
        if lds_cull > LDS_MAX_ALLOWED or request > LDS_MAX_ALLOWED:
            d['use_fp'] = 0
        else:
            d['fresh_two'], d['fresh_in_lds'] = buie, in_lds
            d['general_share'] = max(1. - f['fp_cdf_end'], 0.) if f['fp_has_generic'] else 0.
            d['listed_share'] = min(f['fp_coverage'] * (4. / N.pi if kind in (0, 2, 7) else 1.), 1.)
            d['ulisted_share'] = 1.
            args = (kind, _t(flat), _t(in_lds))
            d['cull'] = ('k_s_cull<%d>' % kind, SC_THREADS, lds_cull)
            d['fresh_one'] = ('k_s_fresh<%d, %s, %s>' % args, threads, request)
            d['fresh'] = ('k_s_fresh2<%d, %s, %s>' % args, threads, request) if buie else d['fresh_one']
            if buie and (flat or in_lds) and f['k_umask'] and f['fp_umask_words'] > 0:      # SF2_DERIVES_CELL
                d['cull_u'] = ('k_s_ucull<%d>' % kind, SC_THREADS, f['fp_umask_words'] * 4 + (SC_GEN_CAP + 4) * 4)
                d['cull_lu'], d['cull_lv'] = [max(int(m) - 1, 0).bit_length() for m in (f['fp_Mu'], f['fp_Mv'])]
                d['ulisted_share'] = min(f['fp_ucoverage'], 1.)
    # k_s_bounce
    big = not walk_ok
    d['use_fused'] = int(mode != 1 and bool(f['k_bounce'] or big))
    d['use_first'] = int(big or small or bool(f['k_first'] and mode != 1))
    d['coop'], d['bg_occ_words'] = 0, 0
    d['bounce'] = d['first'] = NO_STAGE
    if d['use_fused'] or d['use_first']:
        g_cells = f['grid_cells'] if mode == 2 else 0
        d['need_bounce'] = lds_need(bounce_lds_parts(S, stride, BUIE_BYTES, True, True, g_cells, f['grid_list'], 0, 0))
        d['in_lds'] = in_lds = gridm not in (2, 3) and d['need_bounce'] <= LIMIT_LDS
        coop = gridm == 2 and bool(f['k_coop'])
        d['coop'] = int(coop)
        if gridm == 2 and f['big_occ_words'] * 4 <= (OCC_COOP if coop else OCC_LANES):
            d['bg_occ_words'] = f['big_occ_words']
        d['sun'] = sun = kind in (7, 8)
        request = lambda bb: lds_need(bounce_lds_parts(S, stride, bb, in_lds, in_lds, g_cells if in_lds else 0, f['grid_list'], d['bg_occ_words'],
                                                       SB_THREADS // 64 if coop else 0)) + 16
        d['bounce'] = (_coop(False, flat, False) if coop else _bounce(gridm, in_lds, False, flat, False), SB_THREADS, request(0))
        d['first'] = (_coop(True, flat, sun) if coop else _bounce(gridm, in_lds, True, False, sun), SB_THREADS, request(BUIE_BYTES))
    return d



def kd_depth(kd):
    """accel.kd_depth (trc_accel_build_kd, csrc/trc_bounds.h) of a flattened Kd-tree: the depth of its deepest node"""
    depth = N.zeros(len(kd['flag']), dtype=int)
    for i in range(len(depth)):         # (children follow their parent in the flat arrays)
        if kd['flag'][i] != 3:
            c = kd['child'][i]
            depth[c] = depth[c + 1] = depth[i] + 1
    return int(depth.max())


def predict(call):
    """{search-stage kernel as a kernel trace names it: launches} of a call (a second call: of the two), from forms(), the per-bounce
    choice of plan_bounce / launch_bounce, and the reference's rays alive at every bounce"""
    return launches(forms(facts(call)), reference(call)['levels'], N_RAYS, REPS, call.second)


def launches(f, levels, n_rays, reps, second=False):
    """predict() for the decisions `f` of forms() and the levels of a reference of n_rays rays traced for reps interactions"""
    # bounces run: b = 0, then one more while rays are alive and b + 1 < reps (advance)
    n_bounces = 1
    for L in levels[1:]:
        if L['n_live'] == 0 or n_bounces >= reps:
            break
        n_bounces += 1
    out = collections.Counter()
    hit_rate = 0.
    for turn in range(2 if second else 1):
        for b in range(n_bounces):
            fresh = f['use_fp'] and b == 0
            fused = f['use_fused'] and b > 0
            first = f['use_first'] and b == 0 and (not fresh or f['general_share'] > 0.)
            general = not fused and not first and (not fresh or f['general_share'] > 0.)
            if fresh:
                mostly_hits = hit_rate > 0. and hit_rate > 0.6 * 1.15 * f['listed_share']
                out[f['cull'][0]] += 1
                out[(f['fresh_one'] if mostly_hits else f['fresh'])[0]] += 1
            if fused:
                out[f['bounce'][0]] += 1
            if first:
                out[f['first'][0]] += 1
            if general:
                for stage in ('gen0' if b == 0 else 'gen', 'walk', 'exact'):
                    out[f[stage][0]] += 1
        if f['use_fp']:         # advance: what the next call on the scene expects of the listed rays
            hit_rate = 1.15 * len(levels[1]['surf']) / float(n_rays) + 256. / n_rays
    return dict(out)


# -- the references ----------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(call):
    """The oracle's trace of (scene, rays), computed once and shared by every route over them (nobody changes it): a descriptor source
    and the same rays given are one reference, as in shade_cases."""
    from oracle import engine
    key = (call.scene, call.src)
    if key not in _REF:
        s = scene(call.scene)
        v, d, e, rid = s.rays(call.src)
        with N.errstate(all='ignore'):
            o = engine.trace_bundle(s.cs, v, d, e, REPS, s.min_energy(call.src), SEED, offset=0)
        o['hit_list'] = sc.hit_list(o['levels'], s)
        o['maps'] = fs.host_maps(o['hit_list'], s.frames, s.edges)
        _REF[key] = o
    return _REF[key]


def near_ties(call):
    """shade_cases.near_ties of the call's scene and reference with the twin counted as one surface: its tie is exact, and the
    reference decides it by index"""
    from oracle import engine
    s = scene(call.scene)
    assert sc.identical_surfaces(engine.scene_from_compiled(s.cs)) == [s.twin[1]]
    return sc.near_ties(None, given=(s.cs, reference(call), s.min_energy(call.src)), identical_as_one=True)
