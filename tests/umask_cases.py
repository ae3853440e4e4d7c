"""
The scenes of the tests of the footprint map's mask over the uniforms (csrc/trc_footprint.h: umask; k_s_ucull, k_s_fresh2), shared by
tests/test_umask_host.py and tests/test_gpu_umask.py: NSTTF under its Buie disc, and three plates under a source of every kind the
map applies to -- one plate under the centre of the start shape (the wedge cells a = 0 of a disc), one on its rim, one across the
line where a disc's angle uniform wraps from 1 to 0.  The pillbox rectangle is taken twice: facing (0, 0, -1), where the source
swaps its two extents, and tilted, where it does not.
"""
import ctypes as C
import os
import struct

import numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILTED = N.r_[0.3, -0.2, -1.] / N.linalg.norm([0.3, -0.2, -1.])
DOWN = N.r_[0., 0., -1.]
RADIUS, DEPTH, PLATE = 3., 20., 0.5
# (name, direction): the six kinds of k_s_cull and the rectangle's other orientation
KINDS = [('pillbox_disc', TILTED), ('pillbox_rect', TILTED), ('pillbox_rect_swapped', DOWN), ('buie_disc', TILTED),
         ('buie_rect', TILTED), ('sunshape_disc', TILTED), ('sunshape_rect', TILTED)]


def _table():
    g = N.load(os.path.join(ROOT, 'tests', 'golden', 'sunshape.npz'))
    return g['buie05_angles'], g['buie05_intensity']


def source(name, n, direction, seed=11, ray_offset=0):
    """a bundle of n rays of the named kind, its start shape centred DEPTH above the origin along -direction"""
    from tracer_amd import sources
    center = N.c_[-DEPTH * direction]
    kw = dict(flux=1., seed=seed, ray_offset=ray_offset)
    if name == 'pillbox_disc':
        return sources.disk_bundle(n, center, direction, RADIUS, 0.004, **kw)
    if name.startswith('pillbox_rect'):
        return sources.rect_bundle(n, center, direction, 2. * RADIUS, 5., 0.004, **kw)
    if name == 'buie_disc':
        return sources.buie_sunshape(n, center, direction, RADIUS, 0.05, **kw)
    if name == 'buie_rect':
        return sources.rect_buie_sunshape(n, center, direction, 2. * RADIUS, 5., 0.05, **kw)
    a, I = _table()
    if name == 'sunshape_disc':
        return sources.tabulated_sunshape(n, center, direction, RADIUS, a, I, **kw)
    assert name == 'sunshape_rect'
    return sources.rect_tabulated_sunshape(n, center, direction, 2. * RADIUS, 5., a, I, **kw)


def three_plates(name, direction):
    """the three plates in the frame of the source's start shape, DEPTH in front of it: (assembly, compiled scene)"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.scene import compile_scene
    from tracer_amd import optics_callables as opt
    desc = source(name, 10, direction)._src_desc
    rot = N.array(list(desc.rot_pos)).reshape(3, 3)
    e1, e2 = rot[:, 0], rot[:, 1]
    # under the centre, on the rim (for a rectangle: across its edge), across the seam phi = 0
    spots = [(0., 0.), (RADIUS * N.cos(2.), RADIUS * N.sin(2.)), (1.6, 0.)]
    objs = []
    for lx, ly in spots:
        tr = N.eye(4)
        tr[:3, :3] = rot
        tr[:3, 3] = lx * e1 + ly * e2
        objs.append(AssembledObject(surfs=[Surface(RectPlateGM(PLATE, PLATE), opt.Reflective(0.3))], transform=tr))
    asm = Assembly(objects=objs)
    return asm, compile_scene(asm)


def resolved(bundle, hs):
    """(descriptor as the library resolves it, the packed table or None): the tabulated kinds carry their table's address"""
    from tracer_amd import _cabi
    desc = bundle._src_desc          # (a tabulated kind binds its table through the device context: not on the host)
    if desc.kind not in (_cabi.SRC_SUNSHAPE_DISK, _cabi.SRC_SUNSHAPE_RECT):
        return bundle.source_args()[0], None
    a, I = [N.ascontiguousarray(x, dtype=float) for x in _table()]
    p = C.POINTER(C.c_double)
    tab = N.empty(3 * a.size)
    tc, uc = C.c_double(), C.c_double()
    hs.hs_sunshape_pack.restype = C.c_int
    hs.hs_sunshape_pack.argtypes = [C.c_int, p, p, p, p, p]
    assert hs.hs_sunshape_pack(a.size, a.ctypes.data_as(p), I.ctypes.data_as(p), tab.ctypes.data_as(p), C.byref(tc), C.byref(uc)) == 1
    d = _cabi.SourceDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    d.p[5], d.p[6], d.p[7] = tc.value, uc.value, float(tab.size // 3)
    d.buie[0] = N.array([tab.ctypes.data], dtype=N.uint64).view(N.float64)[0]
    return d, tab


def host_cases(hs):
    """[(name, compiled scene, resolved descriptor, table, rays, M)]: NSTTF and the seven three-plate scenes"""
    from tracer_amd import scenes
    from tracer_amd.scene import compile_scene
    plant, field, rec, src = scenes.nsttf_field()
    out = [('nsttf', compile_scene(plant), scenes.nsttf_source(10, src, seed=1).source_args()[0], None, 200000, 512)]
    for name, direction in KINDS:
        d, tab = resolved(source(name, 10, direction), hs)
        out.append((name, three_plates(name, direction)[1], d, tab, 200000, 512))
    return out


def write_cases(path, cases, seed=77, offset=0):
    """the cases in the form tests/umaskcheck/umask_check reads as a program of its own"""
    with open(path, 'wb') as f:
        for name, cs, desc, tab, n, M in cases:
            extra = N.ascontiguousarray(cs.extra, dtype=float)
            f.write(struct.pack('<iii', cs.n_surf, M, 0 if tab is None else tab.size))
            f.write(struct.pack('<qqQQ', extra.size, n, seed, offset))
            f.write(bytes(C.string_at(C.addressof(cs.descs), C.sizeof(cs.descs))))
            f.write(extra.tobytes())
            f.write(bytes(C.string_at(C.addressof(desc), C.sizeof(desc))))
            if tab is not None:
                f.write(N.ascontiguousarray(tab).tobytes())
