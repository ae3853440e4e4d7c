"""
Scenes that select every shading kernel instance of the streaming engine, and their host reference (test_shade_cases_host.py for what
can be said without a device, test_gpu_shade_instances.py on one).

trc_stream_form_shade (csrc/trc_forms.h) picks, per launch, one of

  k_s_shade_c<CLS, FLATN, LDS, SPEC>   CLS 0 mirror / 1 diffuse: the lean kernels of a scene traced without carried columns
  k_s_shade<SIMPLE, 2, LDS, SPEC>      the general class of such a scene
  k_s_shade_x<LDS>                     every hit of a call whose rays carry spectra or complex indices

from the bytes of the tables the kernel would stage in LDS (shade_table_bytes), whether every surface is flat, whether the source has
a spectrum, and whether the rays carry more than the fast engine's record.  The sums are restated here (table_bytes, predict) and
each case below is the room -- one scene, see room() -- with the fewest additions that put its target instance's sum on the
intended side of its limit:

  lean kernels      120 KiB; the mirror class does not count the optics tables (n_extra), so only surfaces cross it: filler plates
                    under the floor (hit through the gaps between the floor tiles, a few hits each: the per-lane tally path)
  k_s_shade         72 KiB, n_extra counted: a long Reflective_spectral table crosses it with the lean kernels still in LDS; its SIMPLE
                    instances admit no optics table (no kind of TRC_OPT_SIMPLE_MASK has one), so fillers again
  k_s_shade_x       72 KiB, the table again

predict() keeps the sums as they were first written; shade_forms() / absorb_forms() restate the shading and terminal stages of
trc_stream_decide (csrc/trc_forms.h) for a fact block (search_cases.FACT_KEYS), and test_shade_cases_host.py holds both to the
header's own decisions, which the check library exports (search_cases.library_decide): field by field for every case, the instance
names included.  The cases spell an instance without the CHART / SPLIT / MAT arguments added since (short_name).

Every case has one flux map (on a Lambertian floor tile, lean capture) and a second capturing surface (a mirror wall, full capture);
no surface absorbs everything, so that every hit goes through a shading kernel and none through k_s_absorb / k_s_bounce's finish.
"""
import ctypes as C
import functools
import os

import numpy as N

import fluxmap_scene as fs

N_RAYS = 4096 + 37          # the last wave is partial
REPS = 6
SEED = 20251
E_MIN_SHARE = 0.1137        # min_energy as a share of a source ray's energy (no product of the room's reflectances): culls from the second hit on, leaves survivors

KiB = 1024
LIMIT_LEAN, LIMIT_LEAN_BINS = 120 * KiB, 150 * KiB          # trc_stream_form_shade: `need <= 120 * 1024`, `K.lds + bins * 8 + 16 <= 150 * 1024`
LIMIT_SHADE, LIMIT_SHADE_BINS = 72 * KiB, 78 * KiB          # ... `all <= 72 * 1024`, `lds_shade + bins * 8 + 16 <= 78 * 1024`

# (trc_gm_nparams of the geometry kinds, by _cabi.GM_* name: geometry_cases.NPARAMS, all 30 of them, held to the library by
# test_geometry_cases_host.py; record_stride reads it there)
REC_HDR = 14                # TRC_REC_HDR
SIZEOF_FLUXMAPDEV = 4 * 4 + 3 * 8 + 12 * 8          # struct FluxMapDev (csrc/trc_device.h)
FLAT_KINDS = ('GM_FLAT_INF', 'GM_RECT', 'GM_RECT_EXTRUDED', 'GM_RECT_PERFORATED', 'GM_ROUND', 'GM_ROUND_CUT', 'GM_TRIANGLE', 'GM_POLYGON')

MIRROR_KINDS = ('OPT_TRANSPARENT', 'OPT_REFLECTIVE', 'OPT_ONE_SIDED_REFLECTIVE', 'OPT_REAL_REFLECTIVE', 'OPT_ONE_SIDED_REAL_REFLECTIVE')
DIFFUSE_KINDS = ('OPT_LAMBERTIAN', 'OPT_LAMBERTIAN_SPECULAR', 'OPT_SEMI_LAMBERTIAN', 'OPT_REFLECTIVE_SPECTRAL', 'OPT_LAMBERTIAN_DIRECTIONAL',
                 'OPT_LAMBERTIAN_DIRECTIONAL_SPECTRAL', 'OPT_FRESNEL_CONDUCTOR')
SIMPLE_KINDS = MIRROR_KINDS + ('OPT_LAMBERTIAN', 'OPT_LAMBERTIAN_SPECULAR')        # TRC_OPT_SIMPLE_MASK (csrc/trc_forms.h)
CLS_MIRROR, CLS_DIFFUSE, CLS_GENERAL = 0, 1, 2

MAP_TILE, FULL_WALL = 0, 4          # places among the room's own surfaces (behind the fillers): the mapped tile, the wall captured in full
MAP_EDGES = (fs.nonuniform(-0.7, 0.9, 13), N.linspace(-0.9, 0.6, 10))           # 12 x 9 of a tile of +-0.9: clipped on three sides
TWIN_AT, TWIN_SIZE = (1.2, -1.3, 1.9), (1.35, 1.35)           # room(ends=True): the twin and the receiver, in the room's own coordinates
TERMINAL_AT, TERMINAL_SIZE = (-1.3, 1.25, 1.8), (1.3, 1.3)


def _kinds():
    from tracer_amd import _cabi
    return _cabi


def _names(prefix):
    K = _kinds()
    return dict((getattr(K, k), k) for k in dir(K) if k.startswith(prefix) and isinstance(getattr(K, k), int))


# -- the sums of trc_stream_form_shade ------------------------------------------------------------------------------------------------
def record_stride(cs):
    """doubles per surface record (trc_scene_create): TRC_REC_HDR + the parameters of the widest geometry kind, made odd"""
    from geometry_cases import NPARAMS         # (that module imports this one)
    gm = _names('GM_')
    return (REC_HDR + max(NPARAMS[gm[cs.descs[i].gm_kind]] for i in range(cs.n_surf))) | 1


def shade_class_of(desc):
    """trc_shade_class_of (csrc/trc_forms.h)"""
    K = _kinds()
    ok, o = desc.optics_kind, list(desc.opt)
    name = _names('OPT_').get(ok)
    if name in MIRROR_KINDS:
        iam = (ok in (K.OPT_REFLECTIVE, K.OPT_ONE_SIDED_REFLECTIVE) and o[1] != 0.) or \
              (ok in (K.OPT_REAL_REFLECTIVE, K.OPT_ONE_SIDED_REAL_REFLECTIVE) and o[3] != 0.)
        return CLS_GENERAL if iam else CLS_MIRROR
    if name in DIFFUSE_KINDS:
        return CLS_GENERAL if (ok == K.OPT_LAMBERTIAN and (o[2] != 0. or o[4] != 0.)) else CLS_DIFFUSE
    return CLS_GENERAL


def ends_every_ray(desc):
    """surface_ends_every_ray (csrc/trc_forms.h)"""
    K = _kinds()
    ok, o = desc.optics_kind, list(desc.opt)
    plain = (ok in (K.OPT_REFLECTIVE, K.OPT_ONE_SIDED_REFLECTIVE) and o[1] == 0.) or \
            (ok in (K.OPT_REAL_REFLECTIVE, K.OPT_ONE_SIDED_REAL_REFLECTIVE) and o[3] == 0.) or \
            (ok == K.OPT_LAMBERTIAN and o[2] == 0. and o[4] == 0.) or ok == K.OPT_LAMBERTIAN_SPECULAR
    return plain and o[0] == 1.


def table_bytes(cs, edges):
    """shade_table_bytes (csrc/trc_stream.inc): (tallies, records, optics parameters, maps and flags) in bytes; edges: {surface:
    (u edges, v edges)} of the flux maps set on the scene"""
    S = cs.n_surf
    n_edges = sum(len(u) + len(v) for u, v in edges.values())
    maps = n_edges * 8 + ((len(edges) * SIZEOF_FLUXMAPDEV + 7) // 8) * 8 + 2 * S * 4 + 16
    return (3 * S + 2) * 8, S * record_stride(cs) * 8, 8 * S * 8, maps


def predict(cs, edges, spec, carry):
    """trc_stream_form_shade restated: {kernel instance as a kernel trace names it: (bytes summed, limit, tables in LDS, bins in LDS)} of the
    shading kernels a streaming call on the scene launches"""
    gm, opt = _names('GM_'), _names('OPT_')
    S = cs.n_surf
    b = sum(table_bytes(cs, edges))
    n_extra = len(cs.extra)
    bins = sum((len(u) - 1) * (len(v) - 1) for u, v in edges.values())
    t = lambda x: 'true' if x else 'false'
    out = {}
    all_ = b + n_extra * 8
    shade_lds = all_ <= LIMIT_SHADE
    shade_bins = bins > 0 and shade_lds and all_ + bins * 8 + 16 <= LIMIT_SHADE_BINS
    if carry:
        out['k_s_shade_x<%s>' % t(shade_lds)] = (all_, LIMIT_SHADE, shade_lds, shade_bins)
        return out
    assert not any(ends_every_ray(cs.descs[i]) for i in range(S))           # (no case routes a hit around the shading kernels)
    flat = all(gm[cs.descs[i].gm_kind] in FLAT_KINDS for i in range(S))
    simple = flat and all(opt[cs.descs[i].optics_kind] in SIMPLE_KINDS for i in range(S))
    present = set(shade_class_of(cs.descs[i]) for i in range(S))
    for c in (CLS_MIRROR, CLS_DIFFUSE):
        if c in present:
            need = b + (0 if c == CLS_MIRROR else n_extra * 8)
            in_lds = need <= LIMIT_LEAN
            out['k_s_shade_c<%d, %s, %s, %s>' % (c, t(flat), t(in_lds), t(spec))] = \
                (need, LIMIT_LEAN, in_lds, bins > 0 and in_lds and need + bins * 8 + 16 <= LIMIT_LEAN_BINS)
    if CLS_GENERAL in present:
        out['k_s_shade<%s, 2, %s, %s>' % (t(simple), t(shade_lds), t(spec))] = (all_, LIMIT_SHADE, shade_lds, shade_bins)
    return out


# -- the shading stage of trc_stream_decide (csrc/trc_forms.h) restated for a fact block (search_cases.FACT_KEYS) ----------------------
IMG_SHADE, IMG_SHADE_X, IMG_LEAN, IMG_LEAN_MIRROR = range(4)            # enum trc_shade_img (csrc/trc_bounds.h)
BARE = {IMG_SHADE: 8, IMG_SHADE_X: 16, IMG_LEAN: 16, IMG_LEAN_MIRROR: 16}         # a launch with nothing staged: the count words (k_s_shade keeps one)
LIMIT_ABSORB, LIMIT_INLINE, INLINE_MARGIN = 78 * KiB, 158 * KiB, 64     # k_s_absorb's tables; k_s_bounce's LDS with them behind its own, and the margin between
SHC_THREADS, SH_THREADS, SA_THREADS = 1024, 256, 1024                   # k_s_shade_c / k_s_shade_x, k_s_shade, k_s_absorb


def fact_bytes(f):
    """table_bytes of a fact block: (tallies, records, optics parameters, maps and flags) in bytes"""
    S = f['n_surf']
    return (3 * S + 2) * 8, S * f['stride'] * 8, 8 * S * 8, f['n_fm_edges'] * 8 + ((f['fms_bytes'] + 7) // 8) * 8 + 2 * S * 4 + 16


def lds_choose(f, img):
    """trc_shade_lds_choose: (tables in LDS, bins in LDS, bytes the launch asks for) of an image of the scene's tables"""
    need = sum(fact_bytes(f)) + (0 if img == IMG_LEAN_MIRROR else f['n_extra'] * 8)
    limit, limit_bins = (LIMIT_LEAN, LIMIT_LEAN_BINS) if img in (IMG_LEAN, IMG_LEAN_MIRROR) else (LIMIT_SHADE, LIMIT_SHADE_BINS)
    bins = f['fm_bins']
    in_lds = need <= limit
    bins_in = bins > 0 and in_lds and need + bins * 8 + 16 <= limit_bins
    return in_lds, bins if bins_in else 0, (need + (bins * 8 + 16 if bins_in else 0)) if in_lds else BARE[img]


def shade_forms(f):
    """
    trc_stream_form_shade restated: dict(shk: per shading kernel of the call (kernel name with every template argument, threads, LDS
    bytes, class or -1, tables in LDS, bins in LDS), n_shk, multi, lds_tally, lds_tables, lds_extra, lds_fm_bins, shade_term_cls); None:
    no instance.  `carry` as the streaming engine takes it: with the calls on a scene whose optics split rays.
    """
    t = lambda x: 'true' if x else 'false'
    carry, spec, chart = bool(f['carry'] or f['splits']), bool(f['spec']), bool(f['chart'])
    in_lds, bins_in, request = lds_choose(f, IMG_SHADE_X if carry else IMG_SHADE)
    d = dict(lds_tally=int(in_lds), lds_tables=int(in_lds), lds_extra=int(in_lds), lds_fm_bins=bins_in, shade_term_cls=-1)
    shk = []
    if carry:
        if f['mat_dev'] and chart:
            return None
        shk.append(('k_s_shade_x<%s, %s, %s, %s>' % (t(in_lds), t(chart), t(f['splits']), t(f['mat_dev'])), SHC_THREADS, request, -1, int(in_lds), bins_in))
    else:
        present = f['cls_moving'] if f['term_ok'] else f['cls_all']
        if f['term_ok'] and f['any_term']:
            d['shade_term_cls'] = CLS_MIRROR if present & 1 else CLS_DIFFUSE if present & 2 else -1
            if d['shade_term_cls'] < 0:
                present = f['cls_all']
        for c, img in ((CLS_MIRROR, IMG_LEAN_MIRROR), (CLS_DIFFUSE, IMG_LEAN)):
            if present >> c & 1:
                l, b, r = lds_choose(f, img)
                shk.append(('k_s_shade_c<%d, %s, %s, %s, %s>' % (c, t(f['all_flat'] and not chart), t(l), t(spec), t(chart)), SHC_THREADS, r, c, int(l), b))
        if present >> CLS_GENERAL & 1:
            shk.append(('k_s_shade<%s, 2, %s, %s, %s>' % (t(f['simple'] and not chart), t(in_lds), t(spec), t(chart)), SH_THREADS, request, CLS_GENERAL,
                        int(in_lds), bins_in))
    d.update(shk=shk, n_shk=len(shk), multi=int(len(shk) > 1))
    return d


def absorb_forms(f, d):
    """trc_stream_form_absorb restated, from the decisions `d` made so far (search_cases.forms, shade_forms): dict(use_absorb,
    absorb_inline, lds_inline, split_terminal, absorb, bounce)"""
    out = dict(use_absorb=0, absorb_inline=0, lds_inline=0, split_terminal=0, absorb=(None, 0, 0), bounce=d['bounce'])
    if not (d['use_fused'] and d['lds_tables'] and not (f['carry'] or f['splits'])):
        return out
    t, r, o, m = fact_bytes(f)
    lds_absorb = t + m + d['lds_fm_bins'] * 8 + 16
    fm_ok = f['fm_bins'] == 0 or d['lds_fm_bins'] > 0
    if not (f['any_term'] and fm_ok and not f['chart'] and lds_absorb <= LIMIT_ABSORB and not f['transfer'] and f['term_ok'] and f['k_absorb'] != 0):
        return out
    out.update(use_absorb=1, split_terminal=1, absorb=('k_s_absorb', SA_THREADS, lds_absorb))
    extra = lds_absorb + INLINE_MARGIN
    if f['k_absorb'] != 1 and not (d['gridm'] == 2 and d['coop']) and d['bounce'][2] + extra <= LIMIT_INLINE:
        out.update(absorb_inline=1, lds_inline=extra, split_terminal=2, bounce=d['bounce'][:2] + (d['bounce'][2] + extra,))
    return out


def short_name(inst):
    """a shading instance as the cases spell it: without the CHART argument of k_s_shade / k_s_shade_c and the CHART, SPLIT, MAT arguments of
    k_s_shade_x, which every case holds at false (the 'carry-mat' rooms, whose materials are on the device: MAT true)"""
    head, args = inst[:-1].split('<')
    args = args.split(', ')
    return '%s<%s>' % (head, ', '.join(args[:1] if head == 'k_s_shade_x' else args[:4]))


ALL_INSTANCES = ['k_s_shade_c<%d, %s, %s, %s>' % (c, f, l, s) for c in (0, 1) for f in ('true', 'false') for l in ('true', 'false')
                 for s in ('true', 'false')] + \
                ['k_s_shade<%s, 2, %s, %s>' % (m, l, s) for m in ('true', 'false') for l in ('true', 'false') for s in ('true', 'false')] + \
                ['k_s_shade_x<true>', 'k_s_shade_x<false>']


# -- the room -------------------------------------------------------------------------------------------------------------------
def _tables():
    th = N.linspace(0., N.pi / 2., 7)
    wl = N.linspace(0.3e-6, 2.5e-6, 6)
    grid = 0.15 + 0.5 * N.outer(N.cos(th) ** 0.5, 1. / (1. + (wl * 1e6 - 1.) ** 2))
    return th, wl, grid


def room(kind, n_fill=0, table_len=12, ends=False):
    """
    (assembly, T): a box of 4 x 4 x 3 open at the top -- a floor of four tiles with gaps between them, four walls -- with flat pieces
    hanging inside, turned by a general rotation T and moved off the origin, so that no frame is axis aligned.

    kind      'flat'     plates, discs, a triangle, a pentagon; every optics kind of the mirror and the diffuse class
              'curved'   ... and a sphere, a finite cylinder and a parabolic dish
              'general'  'curved' with two panes of RefractiveHomogenous (one with a perturbed normal)
              'simple'   'flat' with every optics kind taken from TRC_OPT_SIMPLE_MASK, two of them with an incidence-angle modifier
                         (Reflective_IAM, Lambertian_IAM: the general class in a scene k_s_shade's SIMPLE instances serve)
              'carry'    'flat' with a polychromatic wall, for bundles that carry spectra, and a periodic pane (PeriodicBoundary with a
                         negative period: the ray goes on one period behind the pane, so it does not meet the pane again)
              'carry-mat' 'flat' with a pane between two tabulated materials that attenuate (RefractiveAbsorbant), for bundles that carry
                         wavelengths and complex indices, and the periodic pane
    n_fill    filler plates in a grid under the floor, mirrors and Lambertian plates in turn, in front of the room's own surfaces in
              the table (the room's surfaces then sit at offsets of hundreds of records)
    table_len points of the Reflective_spectral disc's table (2 doubles each in n_extra)
    ends      (search_cases.py) three plates more, behind the room's own surfaces in the table: a twin -- two plates of one frame and one
              size, a partial mirror and, at the higher index, an absorber: every hit on them is an exact tie -- and a receiver that
              ends every ray
    """
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd.triangular_face import TriangularFace
    from tracer_amd.polygon import FlatSimplePolygonGM
    from tracer_amd.sphere_surface import SphericalGM
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd.paraboloid import ParabolicDishGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx, roty, rotz
    T = N.dot(translate(-3.7, 5.2, 1.9), N.dot(rotx(-0.5), N.dot(roty(0.8), rotz(-0.9))))
    half = N.pi / 2.
    th, wl, grid = _tables()
    simple = kind == 'simple'
    metal = opt.TabulatedMaterial(wl, [1.4, 1.1, 0.9, 1.3, 2.0, 2.6], [1.9, 2.9, 4.2, 5.5, 6.6, 7.9])
    lam = N.linspace(0.2e-6, 2.6e-6, table_len)
    spectral = opt.Reflective_spectral(0.2 + 0.5 * N.sin(3e6 * lam) ** 2, lam)
    pick = lambda full, plain: plain if simple else full
    pent = N.array([[0.55 * N.cos(a), 0.55 * N.sin(a)] for a in 2. * N.pi * N.arange(5) / 5. + 0.3]).T
    parts = [
        # the floor: four tiles of 1.8 x 1.8 with a cross of 0.2 between them
        (RectPlateGM(1.8, 1.8), opt.LambertianReceiver(0.4), translate(-1., -1., 0.)),                                  # MAP_TILE
        (RectPlateGM(1.8, 1.8), pick(opt.SemiLambertian(0.3), opt.Lambertian_IAM(0.3, 0.2)), translate(1., -1., 0.)),
        (RectPlateGM(1.8, 1.8), pick(opt.Lambertian_directional_axisymmetric_piecewise(th, 0.2 + 0.4 * N.cos(th)), opt.Lambertian(0.5)),
         translate(-1., 1., 0.)),
        (RectPlateGM(1.8, 1.8), opt.LambertianSpecular(0.3, 0.5), translate(1., 1., 0.)),
        # the walls
        (RectPlateGM(3., 4.), opt.ReflectiveDetector(0.1), N.dot(translate(2., 0., 1.5), roty(half))),                 # FULL_WALL
        (RectPlateGM(3., 4.), opt.RealReflective(0.2, 3e-3), N.dot(translate(-2., 0., 1.5), roty(half))),
        (RectPlateGM(4., 3.), opt.OneSidedReflective(0.15), N.dot(translate(0., 2., 1.5), rotx(half))),
        (RectPlateGM(4., 3.), pick(opt.Reflective(0.3), opt.Reflective_IAM(0.3, 0.2)), N.dot(translate(0., -2., 1.5), rotx(half))),
        # inside: a pane under the source that the rays pass (the mirror class sees them first), two discs that read the wavelength
        (RectPlateGM(2.2, 2.2), opt.Transparent(), N.dot(translate(0.2, 0.1, 2.3), rotx(0.15))),
        (RoundPlateGM(0.85), pick(spectral, opt.Reflective(0.25)), N.dot(translate(-0.5, 0.5, 1.5), N.dot(rotx(0.3), roty(-0.2)))),
        (RoundPlateGM(0.6), pick(opt.FresnelConductorHomogenous(1., metal), opt.RealReflective(0.3, 2e-3)),
         N.dot(translate(0.9, -0.6, 1.2), N.dot(roty(0.4), rotx(-0.2)))),
        # (the pentagon's outline is a geometry table: its optics has none)
        (TriangularFace(N.c_[[1.5, 0.1, 0.], [0.3, 1.4, 0.]]),
         pick(opt.Lambertian_directional_axisymmetric_piecewise_spectral(th, grid, wl), opt.Lambertian(0.35)),
         N.dot(translate(0.1, 0.5, 0.5), N.dot(rotx(0.4), rotz(0.3)))),
        (FlatSimplePolygonGM(pent), opt.OneSidedRealReflective(0.2, 2e-3), N.dot(translate(-0.9, -0.9, 0.9), N.dot(roty(-0.4), rotx(0.3)))),
    ]
    if kind in ('curved', 'general'):
        parts += [(SphericalGM(0.6), opt.RealReflective(0.15, 2e-3), translate(1.1, 1.0, 0.8)),
                  (FiniteCylinder(0.9, 1.3), opt.Lambertian(0.4), N.dot(translate(-1.1, 0.2, 0.75), rotx(0.2))),
                  (ParabolicDishGM(1.6, 0.7), opt.Reflective(0.2), N.dot(translate(0.3, -1.1, 0.25), roty(0.15)))]
    if kind == 'general':
        parts += [(RectPlateGM(1.3, 1.3), opt.RefractiveHomogenous(1., 1.5), N.dot(translate(-1.1, -0.9, 2.0), roty(0.3))),
                  (RectPlateGM(0.9, 0.9), opt.RefractiveHomogenous(1., 1.5, sigma=2e-3), N.dot(translate(-1.3, 0.3, 2.1), rotx(-0.2)))]       # (above the spectral disc, beside the pane the rays pass)
    if kind == 'carry':
        parts += [(RectPlateGM(1.6, 1.6), opt.Lambertian_directional_axisymmetric_piecewise_Polychromatic(th, grid, wl),
                   N.dot(translate(0.9, 0.8, 1.7), rotx(0.2)))]
    if kind == 'carry-mat':
        air, glass = materials()
        parts += [(RectPlateGM(1.6, 1.6), opt.RefractiveAbsorbant(air, glass, attenuation_coefficient_1=1.),
                   N.dot(translate(0.9, 0.8, 1.7), rotx(0.2)))]
    if kind in ('carry', 'carry-mat'):
        parts += [(RectPlateGM(1.3, 1.3), opt.PeriodicBoundary(-0.35), N.dot(translate(-1.1, -0.3, 1.9), roty(0.25)))]
    if ends:
        twin = N.dot(translate(*TWIN_AT), N.dot(rotx(-0.45), roty(-0.35)))
        parts += [(RectPlateGM(*TWIN_SIZE), opt.Reflective(0.3), twin), (RectPlateGM(*TWIN_SIZE), opt.Lambertian(1.), twin),
                  (RectPlateGM(*TERMINAL_SIZE), opt.LambertianReceiver(1.), N.dot(translate(*TERMINAL_AT), N.dot(rotx(0.4), roty(0.3))))]
    fill = []
    side = int(N.ceil(N.sqrt(n_fill))) if n_fill else 0
    for k in range(n_fill):
        pitch = 4. / side
        x, y = -2. + (k % side + 0.5) * pitch, -2. + (k // side + 0.5) * pitch
        fill.append((RectPlateGM(0.9 * pitch, 0.9 * pitch), opt.Reflective(0.2) if k % 2 else opt.Lambertian(0.5), translate(x, y, -0.4)))
    objs = [AssembledObject(surfs=[Surface(gm, o)], transform=N.dot(T, tr)) for gm, o, tr in fill + parts]
    return Assembly(objects=objs), T


def materials():
    from tracer_amd import optics_callables as opt
    tl = N.linspace(0.3e-6, 2.5e-6, 6)
    return (opt.TabulatedMaterial(tl, N.ones(6), N.zeros(6)),
            opt.TabulatedMaterial(tl, [1.55, 1.53, 1.51, 1.50, 1.49, 1.47], [3e-8, 2e-8, 1e-8, 5e-8, 2e-7, 6e-7]))


def spectrum():
    from tracer_amd.source_spectrum import SourceSpectrum
    wl = N.linspace(0.3e-6, 2.5e-6, 23)
    return SourceSpectrum.tabulated(wl, 1. + N.sin(4e6 * wl) ** 2)


# name: (kind of room, fillers, table points, source spectrum, spectral samples per ray, the instances the case is there for)
CASES = {
    'c-flat-lds': ('flat', 0, 12, False, 0, ['k_s_shade_c<0, true, true, false>', 'k_s_shade_c<1, true, true, false>']),
    'c-flat-lds-spec': ('flat', 0, 12, True, 0, ['k_s_shade_c<0, true, true, true>', 'k_s_shade_c<1, true, true, true>']),
    'c-flat-global': ('flat', 460, 12, False, 0, ['k_s_shade_c<0, true, false, false>', 'k_s_shade_c<1, true, false, false>']),
    'c-flat-global-spec': ('flat', 460, 12, True, 0, ['k_s_shade_c<0, true, false, true>', 'k_s_shade_c<1, true, false, true>']),
    'c-curved-lds': ('curved', 0, 12, False, 0, ['k_s_shade_c<0, false, true, false>', 'k_s_shade_c<1, false, true, false>']),
    'c-curved-lds-spec': ('curved', 0, 12, True, 0, ['k_s_shade_c<0, false, true, true>', 'k_s_shade_c<1, false, true, true>']),
    'c-curved-global': ('curved', 460, 12, False, 0, ['k_s_shade_c<0, false, false, false>', 'k_s_shade_c<1, false, false, false>']),
    'c-curved-global-spec': ('curved', 460, 12, True, 0, ['k_s_shade_c<0, false, false, true>', 'k_s_shade_c<1, false, false, true>']),
    'g-lds': ('general', 0, 12, False, 0, ['k_s_shade<false, 2, true, false>']),
    'g-lds-spec': ('general', 0, 12, True, 0, ['k_s_shade<false, 2, true, true>']),
    'g-global': ('general', 0, 4500, False, 0, ['k_s_shade<false, 2, false, false>']),
    'g-global-spec': ('general', 0, 4500, True, 0, ['k_s_shade<false, 2, false, true>']),
    'g-simple-lds': ('simple', 0, 12, False, 0, ['k_s_shade<true, 2, true, false>']),
    'g-simple-lds-spec': ('simple', 0, 12, True, 0, ['k_s_shade<true, 2, true, true>']),
    'g-simple-global': ('simple', 280, 12, False, 0, ['k_s_shade<true, 2, false, false>']),
    'g-simple-global-spec': ('simple', 280, 12, True, 0, ['k_s_shade<true, 2, false, true>']),
    'x-lds': ('carry', 0, 12, False, 3, ['k_s_shade_x<true>']),
    'x-global': ('carry', 0, 4500, False, 3, ['k_s_shade_x<false>']),
    'x-mat-lds': ('carry-mat', 0, 12, False, 0, ['k_s_shade_x<true>']),
    'x-mat-global': ('carry-mat', 0, 4500, False, 0, ['k_s_shade_x<false>']),
}
# (the carry cases trace a given bundle: spectra over sample wavelengths, or wavelengths and complex indices)
# the cases whose rays also go in as a given bundle (the general route of fresh rays): one per kernel family and address space
GIVEN = ('c-flat-lds', 'c-curved-global', 'g-lds', 'g-global', 'g-simple-global')
# the cases traced with a knob of the streaming engine switched off: one LDS = false case of each kernel family, both carry bundles
KNOBS = ('c-flat-global', 'g-global', 'x-global', 'x-mat-global')
# the optics kinds every case must hit (at least 30 times each), by kind of room
KINDS_HIT = {'flat': MIRROR_KINDS + DIFFUSE_KINDS, 'curved': MIRROR_KINDS + DIFFUSE_KINDS,
             'general': MIRROR_KINDS + DIFFUSE_KINDS + ('OPT_REFRACTIVE_HOMOGENOUS',), 'simple': SIMPLE_KINDS,
             'carry': MIRROR_KINDS + DIFFUSE_KINDS + ('OPT_LAMBERTIAN_POLYCHROMATIC', 'OPT_PERIODIC_BOUNDARY'),
             'carry-mat': MIRROR_KINDS + DIFFUSE_KINDS + ('OPT_REFRACTIVE_MATERIAL', 'OPT_PERIODIC_BOUNDARY')}
CURVED_GM = ('GM_SPHERE', 'GM_CYL_FINITE', 'GM_PARAB_DISH')


class Case(object):
    """a case built: compiled scene, frames, maps, source, and what trc_stream_form_shade is predicted to pick for it"""
    def __init__(self, name):
        from tracer_amd.scene import compile_scene
        self.name = name
        self.kind, self.n_fill, table_len, self.spec, self.W, self.targets = CASES[name]
        asm, self.T = room(self.kind, self.n_fill, table_len)
        self.cs = compile_scene(asm)
        self.frames = [N.array(s._temp_frame) for s in self.cs.surfaces]
        self.map_surf, self.full_surf = self.n_fill + MAP_TILE, self.n_fill + FULL_WALL
        self.edges = {self.map_surf: MAP_EDGES}
        self.carry = self.kind in ('carry', 'carry-mat')
        self.instances = predict(self.cs, self.edges, self.spec, self.carry)
        self.captured = [i for i in range(self.cs.n_surf) if self.cs.capture[i]]
        assert self.captured == [self.map_surf, self.full_surf]

    def source(self):
        """the pending bundle of the case's descriptor source (its own seed travels with it)"""
        return fs.source(N_RAYS, self.T, SEED, spectrum=spectrum() if self.spec else None)

    @property
    def min_energy(self):
        return E_MIN_SHARE * self.source().source_args()[0].energy

    def rays(self):
        """(vertices, directions, energy, ray ids) of the source's rays, made by the oracle"""
        from oracle import engine, sources
        desc, n, seed, off = self.source().source_args()
        return sources.generate(engine.source_from_desc(desc), n, seed, off)

    def spectra(self):
        """(sample wavelengths, spectra), (W, n) each, of the carry cases' bundle: every ray its own grid, its energy the integral"""
        v, d, e, rid = self.rays()
        rng = N.random.RandomState(6)
        swl = N.sort(rng.uniform(0.3e-6, 2.5e-6, size=(self.W, N_RAYS)), axis=0)
        spec = rng.uniform(0.5, 2., size=(self.W, N_RAYS))
        spec *= e / _trapz(spec, swl)
        return swl, spec

    def wavelengths(self):
        """(wavelengths, complex indices) of the 'carry-mat' cases' bundle: every ray its own wavelength, in air"""
        wl = N.random.RandomState(7).uniform(0.4e-6, 2.4e-6, N_RAYS)
        return wl, materials()[0].m(wl)

    def bundle(self, given):
        """what the device traces: the pending source bundle, the same rays as a given bundle, or (carry) the bundle with spectra /
        with wavelengths and indices"""
        from tracer_amd.ray_bundle import RayBundle
        if self.kind == 'carry-mat':
            v, d, e, rid = self.rays()
            wl, ref = self.wavelengths()
            return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy(), ref_index=ref, wavelengths=wl)
        if self.carry:
            v, d, e, rid = self.rays()
            swl, spec = self.spectra()
            return RayBundle(vertices=v.copy(), directions=d.copy(), energy=_trapz(spec, swl), spectra=spec.copy(), wavelengths=swl.copy())
        if not given:
            return self.source()
        v, d, e, rid = self.rays()
        return RayBundle(vertices=v.copy(), directions=d.copy(), energy=e.copy())


def _trapz(y, x):
    return N.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2., axis=0)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def host_wavelengths(c):
    """the wavelengths the device draws for the rays of a case's source, from the host-compiled sampler of the per-ray core
    (tests/hostcheck, `make hostcheck`; test_draws_leave_the_rays_as_they_are pins the device's draws to it)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = C.CDLL(os.path.join(root, 'tests', 'hostcheck', 'libtrc_spectrum_check.so'))
    p = C.POINTER(C.c_double)
    lib.hs_spectrum_draw.argtypes = [p, p, p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_long, p, p]
    wl, val, cdf = [N.ascontiguousarray(a, dtype=float) for a in spectrum().table()]
    desc, n, seed, off = c.source().source_args()
    out = N.empty(n)
    lib.hs_spectrum_draw(wl.ctypes.data_as(p), val.ctypes.data_as(p), cdf.ctypes.data_as(p), wl.size, seed, off, n, None, out.ctypes.data_as(p))
    return out


_REF = {}


def reference(name, wavelengths=None):
    """the reference of a case, kept per source of a SPEC case's wavelengths (the host sampler's draws, or those handed in)"""
    key = (name, 'host' if wavelengths is None else 'given')
    if key not in _REF:
        _REF[key] = _reference(name, wavelengths)
    return _REF[key]


def _reference(name, wavelengths):
    """The oracle's trace of a case, computed once and shared (nobody changes it).  A descriptor source and the same rays given
    are one reference: trace_from_compiled and trace_bundle run the same loop on the same rays and Philox streams.  wavelengths: of
    the rays of a SPEC case (the pending bundle's get_wavelengths() on a device; the host sampler's draws otherwise)."""
    from oracle import engine
    c = case(name)
    with N.errstate(all='ignore'):
        if c.kind == 'carry-mat':
            v, d, e, rid = c.rays()
            wl, ref = c.wavelengths()
            o = engine.trace_bundle(c.cs, v, d, e, REPS, c.min_energy, SEED, ref_index=ref, wavelengths=wl)
        elif c.carry:
            v, d, e, rid = c.rays()
            swl, spec = c.spectra()
            o = engine.trace_bundle(c.cs, v, d, _trapz(spec, swl), REPS, c.min_energy, SEED, wavelengths=swl, spectra=spec)
        elif c.spec:
            v, d, e, rid = c.rays()
            wl = host_wavelengths(c) if wavelengths is None else N.asarray(wavelengths, dtype=float)
            o = engine.trace(engine.scene_from_compiled(c.cs), v, d, e, N.ones(len(e)), wl, rid, REPS, c.min_energy, SEED)
        else:
            o = engine.trace_from_compiled(c.cs, c.source().source_args(), REPS, c.min_energy)
    o['hit_list'] = hit_list(o['levels'], c)
    o['maps'] = fs.host_maps(o['hit_list'], c.frames, c.edges)
    return o


def hit_list(levels, c):
    """fluxmap_scene.hits_of_levels with, for rays that carry spectra, the 3 W spectral columns of a captured hit: sample wavelengths,
    the spectrum that arrived, the spectrum that left"""
    K = _kinds()
    periodic = [i for i in range(c.cs.n_surf) if c.cs.descs[i].optics_kind == K.OPT_PERIODIC_BOUNDARY]
    # (a periodic pane sends a stub of energy 0 on beside the ray, as the reference does: the stub is no hit of its own)
    keep = lambda L: ~(N.isin(L['surf'], periodic) & (N.asarray(L['energy']) == 0.))
    hits = fs.hits_of_levels(levels, keep)
    assert 'directions' in hits         # (the oracle's levels carry them: a full capture is compared with them)
    if c.W:
        swl0, spec0 = c.spectra()
        x = []
        for k, (prev, L) in enumerate(zip(levels[:-1], levels[1:])):
            m = keep(L)
            par = N.asarray(L['parents'])[m]
            arrived = (spec0 if k == 0 else prev['spectra'])[:, par]
            x.append(N.vstack((L['swl'][:, m], arrived, L['spectra'][:, m])))
        hits['x'] = N.hstack(x)
    return hits


def identical_surfaces(scene):
    """surfaces of an oracle scene table whose geometry descriptor (kind, frame, parameters) is that of a surface of lower index: a
    ray meets the two at exactly the same distance, and the reference gives the hit to the lower index"""
    same = lambda a, b: a['kind'] == b['kind'] and N.array_equal(a['frame'], b['frame']) and N.array_equal(a['gm'], b['gm'])
    return [k for k in range(len(scene)) if any(same(scene[k], scene[j]) for j in range(k))]


def near_ties(name, given=None, identical_as_one=False):
    """(smallest relative gap between a ray's nearest and second-nearest intersection, smallest relative distance of an outgoing
    energy from min_energy) over every bounce of the reference: what decides whether a ray could end elsewhere on a device.
    given: (compiled scene, reference, min_energy) instead of those of the case `name` (search_cases.py); identical_as_one: a pair of
    surfaces with identical descriptors counts as one surface -- their tie is exact and decided by index, not a near tie"""
    from oracle import engine, geometry
    cs, o, min_energy = (case(name).cs, reference(name), case(name).min_energy) if given is None else given
    scene = engine.scene_from_compiled(cs)
    skip = identical_surfaces(scene) if identical_as_one else []
    gap = N.inf
    for L in o['levels'][:-1] if len(o['levels']) > REPS else o['levels']:
        n = L['n_live']
        if n == 0:
            continue
        v, d = L['vertices'][:, :n], L['directions'][:, :n]
        first, second = N.full(n, N.inf), N.full(n, N.inf)
        for k, s in enumerate(scene):
            if k in skip:
                continue
            t = geometry.intersect(s['kind'], s['frame'], s['gm'], s['extra'], v, d)
            t[t == 0.] = N.inf
            second = N.minimum(second, N.maximum(first, t))
            first = N.minimum(first, t)
        both = N.isfinite(second)
        if both.any():
            gap = min(gap, ((second[both] - first[both]) / second[both]).min())
    e = N.concatenate([L['energy'] for L in o['levels'][1:]])
    return gap, N.abs(e / min_energy - 1.).min()
