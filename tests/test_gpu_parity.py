"""
GPU parity tests (run with -m gpu on the MI355X box).  Everything here goes through the C-ABI of
include/tracer_amd.h: the HIP path is compared (1) directly with the reference's outputs stored in tests/golden,
(2) ray by ray with the oracle on identical Philox seeds, (3) at full benchmark sizes through size-independent
properties.  Tolerances: the device computes in float64 like the reference; differences come from FMA
contraction, R^T(p-c) instead of inv(frame).p and the device libm -- 1e-9 relative / 1e-8 m absolute on lengths
of up to a few hundred metres is asserted, and hit/miss patterns, parents and orderings are exact.
"""
import ctypes as C

import os
import numpy as N
import pytest

from helpers import load, case_names, oracle_scene, table_scene, source_dict

pytestmark = pytest.mark.gpu

RT, AT = 1e-9, 1e-8


@pytest.fixture(scope='module')
def ctx():
    from tracer_amd import _cabi
    return _cabi.get_context(0)


def _desc(kind, frame, gm, extra, opt_kind=0, opt=()):
    from tracer_amd import _cabi
    from tracer_amd.geometry_manager import fill_desc
    d = _cabi.SurfaceDesc()
    fill_desc(d, frame, kind, list(gm), opt_kind, list(opt), extra_off=0 if len(extra) else -1, extra_len=len(extra))
    return d


def gm_intersect(ctx, kind, frame, gm, extra, v, d):
    from tracer_amd import _cabi
    desc = _desc(kind, frame, gm, extra)
    v = _cabi.f64(v); d = _cabi.f64(d); extra = _cabi.f64(extra)
    n = v.shape[1]
    rays = _cabi.make_rays(n, v[0], v[1], v[2], d[0], d[1], d[2])
    t = N.empty(n); h = N.empty((3, n))
    _cabi.check(ctx.lib.trc_gm_find_intersections(ctx.handle, C.byref(desc), len(extra), _cabi.ptr(extra) if len(extra) else None,
                                                  C.byref(rays), _cabi.ptr(t), _cabi.ptr(h[0]), _cabi.ptr(h[1]), _cabi.ptr(h[2])))
    return t, h


def gm_normals(ctx, kind, frame, gm, hits, dirs):
    from tracer_amd import _cabi
    desc = _desc(kind, frame, gm, [])
    if kind == _cabi.GM_RECT_PERFORATED:
        desc.gm_kind = _cabi.GM_RECT
    h = _cabi.f64(hits); d = _cabi.f64(dirs)
    out = N.empty_like(h)
    _cabi.check(ctx.lib.trc_gm_get_normals(ctx.handle, C.byref(desc), h.shape[1], _cabi.ptr(h[0]), _cabi.ptr(h[1]), _cabi.ptr(h[2]),
                                           _cabi.ptr(d[0]), _cabi.ptr(d[1]), _cabi.ptr(d[2]), _cabi.ptr(out[0]), _cabi.ptr(out[1]),
                                           _cabi.ptr(out[2])))
    return out


def test_geometry_vs_reference_fixtures(ctx):
    """every native kind: t, hit points and normals against the reference's own outputs"""
    g = load('geometry.npz')
    names = case_names(g)
    for ci in range(int(g['n_cases'])):
        pre = 'g%d_' % ci
        kind = int(g[pre + 'kind'])
        t, h = gm_intersect(ctx, kind, g[pre + 'frame'], g[pre + 'gm'], g[pre + 'extra'], g[pre + 'v'], g[pre + 'd'])
        t_ref = g[pre + 't']
        assert N.array_equal(N.isfinite(t), N.isfinite(t_ref)), names[ci]
        idx = g[pre + 'hit_idx']
        assert N.allclose(t[idx], t_ref[idx], rtol=RT, atol=AT), names[ci]
        if len(idx):
            assert N.allclose(h[:, idx], g[pre + 'hits'], rtol=RT, atol=AT), names[ci]
            nrm = gm_normals(ctx, kind, g[pre + 'frame'], g[pre + 'gm'], g[pre + 'hits'], g[pre + 'd'][:, idx])
            ok = N.all(N.isclose(nrm, g[pre + 'normals'], rtol=RT, atol=1e-9) | (N.isnan(nrm) & N.isnan(g[pre + 'normals'])), axis=0)
            assert ok.all(), (names[ci], N.nonzero(~ok)[0][:5])


def test_geometry_vs_oracle_large_fans(ctx):
    """2e4 random rays per kind against the oracle (denser coverage of apertures and root choices)"""
    from oracle import geometry
    g = load('geometry.npz')
    rng = N.random.RandomState(99)
    done = set()
    for ci in range(int(g['n_cases'])):
        pre = 'g%d_' % ci
        kind = int(g[pre + 'kind'])
        frame = g[pre + 'frame']
        key = (kind, ci % 3)
        if ci % 3 != 1 or key in done:       # the rotated + translated frame of each kind
            continue
        done.add(key)
        n = 20000
        c, R = frame[:3, 3], frame[:3, :3]
        o = N.dot(R, rng.uniform(-1, 1, size=(3, n)) * 6.) + c[:, None]
        tg = N.dot(R, rng.uniform(-1, 1, size=(3, n)) * 1.5) + c[:, None]
        d = tg - o
        d /= N.sqrt(N.sum(d ** 2, axis=0))
        t, h = gm_intersect(ctx, kind, frame, g[pre + 'gm'], g[pre + 'extra'], o, d)
        with N.errstate(all='ignore'):
            t_o = geometry.intersect(kind, frame, list(g[pre + 'gm']), g[pre + 'extra'], o, d)
        fin = N.isfinite(t_o)
        mism = N.isfinite(t) != fin
        # a ray grazing an aperture edge or a threshold within rounding may flip; none is expected in 2e4 random rays
        assert mism.sum() == 0, (kind, int(mism.sum()))
        assert N.allclose(t[fin], t_o[fin], rtol=RT, atol=AT), kind
        if fin.any():
            pts = o[:, fin] + t_o[fin] * d[:, fin]
            with N.errstate(all='ignore'):
                n_o = geometry.normals(kind, frame, list(g[pre + 'gm']), pts, d[:, fin])
            n_d = gm_normals(ctx, kind, frame, g[pre + 'gm'], pts, d[:, fin])
            # the flip test `d.n > 0` can go either way for a ray tangent to the surface within rounding
            close = N.all(N.isclose(n_d, n_o, rtol=RT, atol=1e-9), axis=0) | N.all(N.isclose(n_d, -n_o, rtol=RT, atol=1e-9), axis=0) & (N.abs(N.sum(n_o * d[:, fin], axis=0)) < 1e-7)
            assert close.all(), (kind, int((~close).sum()))


def optics_apply(ctx, kind, opt, extra, frame, d, e, ref, wl, nrm, pts, seed, event, path=None, mat=None, spec=None, swl=None):
    """trc_optics_apply on one surface's hits.  ref may be complex; mat (K, n) complex: the materials at the rays' wavelengths;
    spec, swl (W, n): a polychromatic bundle.  Returns dirs, energy, parents, ref, rid[, spectra]."""
    from tracer_amd import _cabi
    desc = _desc(0, frame, [], extra, kind, opt)
    n = d.shape[1]
    cplx = N.iscomplexobj(ref) or mat is not None
    ref = N.asarray(ref)
    d = _cabi.f64(d); e = _cabi.f64(e); wl = _cabi.f64(wl); nrm = _cabi.f64(nrm); pts = _cabi.f64(pts)
    re_in, im_in = _cabi.f64(ref.real), (_cabi.f64(ref.imag) if cplx else None)
    extra = _cabi.f64(extra)
    rid = N.arange(n, dtype=N.uint64) + N.uint64(1000)
    org = _cabi.f64(pts - d * (N.ones(n) if path is None else path))      # ray origins: the attenuating optics measure the path
    matr = None
    if mat is not None:
        matr = N.empty((2 * len(mat), n))
        matr[0::2], matr[1::2] = N.real(mat), N.imag(mat)
    rin = _cabi.make_rays(n, org[0], org[1], org[2], dx=d[0], dy=d[1], dz=d[2], e=e, ref_index=re_in, wavelength=wl, rid=rid,
                          ref_index_im=im_in, mat=matr, spec_wl=None if spec is None else _cabi.f64(swl),
                          spectra=None if spec is None else _cabi.f64(spec))
    m = 2 * n
    o = dict((k, N.empty(m)) for k in ('x', 'y', 'z', 'dx', 'dy', 'dz', 'e', 'ref'))
    par = N.empty(m, dtype=N.int64)
    oim = N.empty(m) if cplx else None
    osp = N.empty((spec.shape[0], m)) if spec is not None else None
    oswl = N.empty((spec.shape[0], m)) if spec is not None else None
    rout = _cabi.make_rays(m, o['x'], o['y'], o['z'], o['dx'], o['dy'], o['dz'], o['e'], parent=par, ref_index=o['ref'],
                           ref_index_im=oim, spec_wl=oswl, spectra=osp)
    _cabi.check(ctx.lib.trc_optics_apply(ctx.handle, C.byref(desc), len(extra), _cabi.ptr(extra) if len(extra) else None, C.byref(rin),
                                         _cabi.ptr(pts[0]), _cabi.ptr(pts[1]), _cabi.ptr(pts[2]), _cabi.ptr(nrm[0]), _cabi.ptr(nrm[1]),
                                         _cabi.ptr(nrm[2]), seed, event, C.byref(rout)))
    k = rout.n
    ref_out = o['ref'][:k] + 1j * oim[:k] if cplx else o['ref'][:k]
    res = (N.vstack((o['dx'][:k], o['dy'][:k], o['dz'][:k])), o['e'][:k], par[:k], ref_out, rid)
    if spec is not None:
        assert N.array_equal(oswl[:, :k], swl[:, par[:k]])
        res = res + (osp[:, :k],)
    return res


def test_optics_vs_reference_and_oracle(ctx):
    """deterministic kinds against the reference fixtures; random kinds ray by ray against the oracle on the same Philox streams"""
    from oracle import optics
    o = load('optics.npz')
    frame, nrm, d, pts, e, wl = o['frame'], o['normals'], o['dirs'], o['points'], o['energy'], o['wavelengths']
    up = frame[:3, 2]
    names = case_names(o)
    deterministic = ('transparent', 'reflective', 'one_sided_reflective', 'real_reflective_sigma0', 'reflective_spectral',
                     'refractive_split', 'fresnel_conductor', 'refractive_transmissive_split', 'refractive_transmissive_one_coefficient',
                     # SURVEY 8(f)2, rest: complex indices of tabulated materials, attenuation from Im m; polychromatic bundles
                     'material_split', 'material_absorbant_split', 'material_absorbant_scaled',
                     'poly_transparent', 'poly_reflective', 'poly_one_sided_reflective', 'poly_real_reflective', 'poly_refractive_split',
                     # the periodic boundary as a native kind (stub + the ray one period along the normal)
                     'periodic_boundary', 'poly_periodic_boundary')
    seen = 0
    for i, name in enumerate(names):
        pre = 'o%d_' % i
        kind, opt, extra, ref_in = int(o[pre + 'kind']), list(o[pre + 'opt']), o[pre + 'extra'], o[pre + 'ref_in']
        path = o[pre + 'path']
        mat = o[pre + 'mat'] if (pre + 'mat') in o.files else None
        spec = o[pre + 'spec_in'] if (pre + 'spec_in') in o.files else None
        swl = o[pre + 'spec_wl'] if spec is not None else None
        wl_i = N.zeros_like(wl) if spec is not None else wl          # a polychromatic bundle has no single wavelength per ray
        res = optics_apply(ctx, kind, opt, extra, frame, d, e, ref_in, wl_i, nrm, pts, 4242, 3, path=path, mat=mat, spec=spec, swl=swl)
        dirs, en, par, ref, rid = res[:5]
        if name in deterministic:
            seen += 1
            assert N.array_equal(par, o[pre + 'out_parents']), name
            assert N.allclose(dirs, o[pre + 'out_dirs'], rtol=RT, atol=1e-9), name
            assert N.allclose(en, o[pre + 'out_energy'], rtol=RT, atol=1e-12), name
            if (pre + 'out_ref') in o.files:
                assert N.allclose(ref, o[pre + 'out_ref'], rtol=1e-12, atol=0), name
                assert N.iscomplexobj(o[pre + 'out_ref']) == (mat is not None), name
            if spec is not None:
                assert N.allclose(res[5], o[pre + 'out_spectra'], rtol=1e-12, atol=0), name
        if name.startswith('lambertian_absorbant'):       # energies are deterministic: against the reference's own
            assert N.allclose(en, o[pre + 'out_energy'], rtol=RT, atol=1e-12), name
        if name in ('polychromatic_wall', 'poly_lambertian', 'poly_lambertian_absorbant', 'poly_lambertian_directional', 'poly_lambertian_specular'):
            # the directions are drawn; spectra and energies are not
            assert N.allclose(res[5], o[pre + 'out_spectra'], rtol=1e-12, atol=0), name
            assert N.allclose(en, o[pre + 'out_energy'], rtol=RT, atol=1e-12), name
        ext = {}
        if mat is not None:
            ext['mat'] = mat
        if spec is not None:
            ext.update(spec=spec, swl=swl)
        blocks = optics.shade(kind, opt, extra, up, d, e, ref_in, wl_i, nrm, 4242, rid, 3, path=path, ext=ext)
        assert N.array_equal(par, N.hstack([b['sel'] for b in blocks])), name
        # trig of ~2*pi*u on the device vs numpy differ in the last bits; 1e-9 still holds
        assert N.allclose(dirs, N.hstack([b['directions'] for b in blocks]), rtol=RT, atol=1e-9), name
        assert N.allclose(en, N.hstack([b['energy'] for b in blocks]), rtol=RT, atol=1e-12), name
        assert N.allclose(ref, N.hstack([b['ref'] for b in blocks])), name
        if spec is not None:
            assert N.allclose(res[5], N.hstack([b['spectra'] for b in blocks]), rtol=1e-12, atol=0), name
    assert seen == len(deterministic)


def test_sources_vs_oracle(ctx):
    """trc_source_generate against the oracle generator on the same seeds, every source kind of the fixtures"""
    from oracle import sources
    from tracer_amd import _cabi
    s = load('sources.npz')
    for i, name in enumerate(case_names(s)):
        pre = 's%d_' % i
        src = source_dict(s, pre)
        desc = _cabi.SourceDesc()
        desc.kind = src['kind']
        for k in range(3):
            desc.center[k] = src['center'][k]
        for k in range(9):
            desc.rot_pos[k] = src['rot_pos'].ravel()[k]
            desc.rot_dir[k] = src['rot_dir'].ravel()[k]
        for k in range(8):
            desc.p[k] = src['p'][k]
        desc.energy = src['energy']
        for k in range(_cabi.BUIE_LEN):
            desc.buie[k] = src['buie'][k]
        n = 50000
        v = N.empty((3, n)); d = N.empty((3, n)); e = N.empty(n)
        rays = _cabi.make_rays(n, v[0], v[1], v[2], d[0], d[1], d[2], e)
        _cabi.check(ctx.lib.trc_source_generate(ctx.handle, C.byref(desc), n, 777, 123456789012, C.byref(rays)))
        vo, do, eo, rid = sources.generate(src, n, 777, 123456789012)
        assert N.allclose(v, vo, rtol=1e-10, atol=1e-8), name
        assert N.allclose(d, do, rtol=1e-9, atol=1e-11), name
        assert N.allclose(e, eo, rtol=1e-14), name
        assert N.allclose(N.sum(d ** 2, axis=0), 1., atol=1e-12), name
        if name == 'disk_bundle':
            # x_cut (sources.py:216-228): rejected positions are redrawn from the ray's own stream; device == oracle,
            # every position qualifies, and what is left is still uniform over the remaining part of the annulus
            desc.p[5], desc.p[6] = 1., 0.4
            src_cut = dict(src, p=list(src['p'][:5]) + [1., 0.4, 0.])
            _cabi.check(ctx.lib.trc_source_generate(ctx.handle, C.byref(desc), n, 777, 5, C.byref(rays)))
            vo, do, eo, rid = sources.generate(src_cut, n, 777, 5)
            assert N.allclose(v, vo, rtol=1e-10, atol=1e-8) and N.allclose(d, do, rtol=1e-9, atol=1e-11)
            loc = N.dot(src['rot_pos'].T, v - N.asarray(src['center']).reshape(3, 1))
            assert N.all(loc[0] < 0.4) and N.allclose(loc[2], 0., atol=1e-9)
            r2 = loc[0] ** 2 + loc[1] ** 2
            assert 0.3 ** 2 - 1e-9 <= r2.min() and r2.max() <= 1.5 ** 2 + 1e-9
            frac = N.mean(loc[0] < -0.5)                       # area of {x < -0.5} over area of {x < 0.4}, both inside the annulus
            def seg(a, R):                                     # area of the disc of radius R with x < a
                a = N.clip(a, -R, R)
                return R * R * (N.pi - N.arccos(a / R)) + a * N.sqrt(R * R - a * a)
            expect = (seg(-0.5, 1.5) - seg(-0.5, 0.3)) / (seg(0.4, 1.5) - seg(0.4, 0.3))
            assert abs(frac - expect) < 4. * N.sqrt(expect * (1. - expect) / n), (frac, expect)


def _ordered(ctx, ts, v, d, e, reps, min_energy, seed, accel=False, ref_index=None, kd=None):
    from tracer_amd.scene import DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    dev = DeviceScene(ts, ctx)
    if kd is not None:
        dev.set_kdtree(kd)
    kw = {} if ref_index is None else dict(ref_index=ref_index)
    res, stats = dev.trace_ordered(RayBundle(vertices=v, directions=d, energy=e, **kw), reps, min_energy, seed, accel=accel)
    levels = [res.level(k) for k in range(res.num_levels())]
    tallies = dev.get_tallies()
    res.close()
    dev.close()
    return levels, stats, tallies


def test_ordered_engine_vs_reference_trees(ctx):
    """deterministic scenes: every RayTree level (order, parents, vertices, directions, energies) equals the reference's"""
    g = load('engine.npz')
    for i, name in enumerate(case_names(g)):
        pre = 'e%d_' % i
        if int(g[pre + 'accel']):
            continue
        ts = table_scene(g, pre)
        ref = g[pre + 'ref_index'] if (pre + 'ref_index') in g.files else None
        levels, stats, _ = _ordered(ctx, ts, g[pre + 'v'], g[pre + 'd'], g[pre + 'e'], int(g[pre + 'reps']), float(g[pre + 'min_energy']), 5,
                                    ref_index=ref)
        nlev = int(g[pre + 'n_levels'])
        assert len(levels) == nlev, (name, [l['vertices'].shape[1] for l in levels])
        for k in range(1, nlev):
            L = levels[k]
            assert L['vertices'].shape == g[pre + 'L%d_vertices' % k].shape, (name, k)
            assert N.array_equal(L['parents'], g[pre + 'L%d_parents' % k]), (name, k)
            assert N.allclose(L['vertices'], g[pre + 'L%d_vertices' % k], rtol=RT, atol=AT), (name, k)
            assert N.allclose(L['directions'], g[pre + 'L%d_directions' % k], rtol=RT, atol=1e-9), (name, k)
            assert N.allclose(L['energy'], g[pre + 'L%d_energy' % k], rtol=RT, atol=1e-12), (name, k)
        n_last = g[pre + 'last_vertices'].shape[1]
        assert stats.rays_left == n_last, name
        if n_last:
            assert N.allclose(levels[-1]['vertices'][:, :n_last], g[pre + 'last_vertices'], rtol=RT, atol=AT), name


def _mc_scene():
    """every random optics kind in one scene"""
    from tracer_amd import _cabi as K
    from tracer_amd.scene import TableScene
    from tracer_amd.spatial_geometry import rotx, roty, translate
    frames = [translate(0, 0, -2.), N.dot(translate(0, 0, 3.), rotx(N.pi)), N.dot(translate(3., 0, 0.), roty(-N.pi / 2.)),
              N.dot(translate(-3., 0, 0.), roty(N.pi / 2.)), N.dot(translate(0., 3., 0.), rotx(N.pi / 2.)),
              N.dot(translate(0., -3., 0.), rotx(-N.pi / 2.))]
    gm_kind = [K.GM_RECT, K.GM_PARAB_DISH, K.GM_ROUND, K.GM_RECT, K.GM_RECT, K.GM_RECT]
    gm = N.zeros((6, 16))
    gm[0, :2] = 3.5, 3.5
    gm[1, :3] = 1. / (4 * 2.), 1. / (4 * 2.), (3. / (2 * N.sqrt(2.))) ** 2
    gm[2, :2] = 3., -1.
    gm[3, :2] = 3.5, 3.5
    gm[4, :2] = 3.5, 3.5
    gm[5, :2] = 3.5, 3.5
    ok = [K.OPT_REAL_REFLECTIVE, K.OPT_REAL_REFLECTIVE, K.OPT_LAMBERTIAN, K.OPT_LAMBERTIAN_SPECULAR,
          K.OPT_ONE_SIDED_REAL_REFLECTIVE, K.OPT_REFRACTIVE_HOMOGENOUS]
    opt = N.zeros((6, 8))
    opt[0, :3] = 0.1, 5e-3, 1.
    opt[1, :3] = 0.1, 5e-3, 0.
    opt[2, :2] = 0.3, N.pi / 2.
    opt[3, :2] = 0.2, 0.5
    opt[4, :3] = 0.15, 2e-3, 1.
    opt[5, :4] = 1.0, 1.5, 1., 1e-3      # single-ray refraction with normal perturbation
    return TableScene(gm_kind, ok, frames, gm, opt, N.zeros(0), -N.ones(6, dtype=int), N.zeros(6, dtype=int))


def test_engines_vs_oracle_monte_carlo(ctx):
    """slope error / Lambertian / mixed / refractive sampling: both device engines against the oracle, ray by ray"""
    from oracle import engine
    from tracer_amd.scene import DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    ts = _mc_scene()
    rng = N.random.RandomState(1)
    n = 6000
    v = rng.uniform(-0.5, 0.5, size=(3, n))
    d = rng.normal(size=(3, n)); d /= N.sqrt(N.sum(d ** 2, axis=0))
    e = rng.uniform(0.5, 1.5, n)
    seed, reps, emin = 20240901, 8, 0.02
    levels, stats, tallies = _ordered(ctx, ts, v, d, e, reps, emin, seed, ref_index=N.ones(n))
    ref = engine.trace_bundle(ts, v, d, e, reps, emin, seed, ref_index=N.ones(n))
    assert [l['vertices'].shape[1] for l in levels] == [l['vertices'].shape[1] for l in ref['levels']]
    for k in range(1, len(levels)):
        L, O = levels[k], ref['levels'][k]
        assert N.array_equal(L['parents'], O['parents']), k
        assert N.array_equal(L['surf'], O['surf']), k
        assert L['n_live'] == O['n_live'], k
        assert N.allclose(L['vertices'], O['vertices'], rtol=RT, atol=AT), k
        assert N.allclose(L['directions'], O['directions'], rtol=1e-8, atol=1e-8), k
        assert N.allclose(L['energy'], O['energy'], rtol=RT, atol=1e-12), k
    assert N.array_equal(tallies[2], ref['hits'])
    assert N.allclose(tallies[0], ref['absorbed'], rtol=1e-9, atol=1e-9)
    assert stats.segments == ref['segments']
    # fast engine: same per-surface tallies, same surviving rays (as a set)
    dev = DeviceScene(ts, ctx)
    st, last = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e, ref_index=N.ones(n)), reps, emin, seed, keep_last=True)
    a, r, h = dev.get_tallies()
    dev.close()
    assert N.array_equal(h, ref['hits'])
    assert N.allclose(a, ref['absorbed'], rtol=1e-9, atol=1e-9)
    assert N.allclose(r, ref['received'], rtol=1e-9, atol=1e-9)
    assert st.segments == ref['segments'] and st.rays_left == ref['last_vertices'].shape[1]
    # the streaming form of the fast engine (separate kernels + HBM queues): same tallies
    dev = DeviceScene(ts, ctx)
    st2, last2 = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e, ref_index=N.ones(n)), reps, emin, seed, keep_last=True, stream=True)
    a2, r2, h2 = dev.get_tallies()
    dev.close()
    assert N.array_equal(h2, ref['hits']) and N.allclose(a2, ref['absorbed'], rtol=1e-9, atol=1e-9) and N.allclose(r2, ref['received'], rtol=1e-9, atol=1e-9)
    assert st2.segments == ref['segments'] and st2.rays_left == st.rays_left and st2.hits == st.hits
    if st.rays_left:
        theirs = N.vstack((ref['last_vertices'], ref['last_directions'], ref['last_energy'][None, :]))
        theirs = theirs[:, N.lexsort(N.round(ref['last_vertices'], 6))]
        for form, left in (('megakernel', last), ('stream', last2)):
            mine = N.vstack(left)[:, N.lexsort(N.round(N.vstack(left[:3]), 6))]
            assert mine.shape == theirs.shape, form
            assert N.allclose(mine, theirs, rtol=1e-8, atol=1e-7), form


def test_kd_accel_equals_brute_and_reference(ctx):
    """accel=True gives the brute-force results (and the reference's) on the NSTTF subset fixture, both engines"""
    from tracer_amd import scenes
    from tracer_amd.accel_tree import KdTree
    from tracer_amd.scene import compile_scene, DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    g = load('engine.npz')
    names = case_names(g)
    pre = 'e%d_' % names.index('nsttf30_accel')
    plant, field, rec, src = scenes.nsttf_field(sigma=0., n_heliostats=30)
    cs = compile_scene(plant)
    assert N.allclose(N.array([list(d.frame) for d in cs.descs]), g[pre + 'scene_frames'][:, :3].reshape(31, 12))
    kd = KdTree(plant, 8 + 1.3 * N.log(31), min_leaf=1)
    v, d, e = g[pre + 'v'], g[pre + 'd'], g[pre + 'e']
    lv_b, st_b, tl_b = _ordered(ctx, cs, v, d, e, 100, 1e-10, 1)
    lv_a, st_a, tl_a = _ordered(ctx, cs, v, d, e, 100, 1e-10, 1, accel=True, kd=kd)
    assert len(lv_a) == len(lv_b) == int(g[pre + 'n_levels'])
    for k in range(1, len(lv_a)):
        for key in ('vertices', 'directions', 'energy', 'parents', 'surf'):
            assert N.array_equal(lv_a[k][key], lv_b[k][key]), (k, key)
        assert N.array_equal(lv_a[k]['parents'], g[pre + 'L%d_parents' % k])
        assert N.allclose(lv_a[k]['vertices'], g[pre + 'L%d_vertices' % k], rtol=RT, atol=AT)
        assert N.allclose(lv_a[k]['energy'], g[pre + 'L%d_energy' % k], rtol=RT)
    # receiver accountant of the reference = absorbed energies and hit points on surface 30
    acc_e = g[pre + 'acc_s30_0']
    assert N.isclose(tl_a[0][30], acc_e.sum(), rtol=1e-9)
    dev = DeviceScene(cs, ctx)
    dev.set_kdtree(kd)
    st, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e), 100, 1e-10, 1, accel=True)
    a, r, h = dev.get_tallies()
    dev.close()
    assert N.array_equal(h, tl_b[2]) and N.allclose(a, tl_b[0], rtol=1e-12, atol=1e-9)
    # a candidate queue that is too small: the bounce is run again with twice the room, same results
    os.environ['TRC_STREAM_Q3_ENTRIES'] = '2048'
    try:
        dev = DeviceScene(cs, ctx)
        dev.set_kdtree(kd)
        st_small, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e), 100, 1e-10, 1, accel=True, stream=True)
        a_s, r_s, h_s = dev.get_tallies()
        dev.close()
    finally:
        del os.environ['TRC_STREAM_Q3_ENTRIES']
    assert N.array_equal(h_s, tl_b[2]) and N.allclose(a_s, tl_b[0], rtol=1e-12, atol=1e-9) and st_small.segments == st.segments
    # hit capture of the streaming form: chunks of the hit buffer stay open between launches; repeated calls append,
    # clearing forgets, and what comes back is what the tallies counted (receiver = surface 30 captures)
    dev = DeviceScene(cs, ctx)
    dev.set_kdtree(kd)
    dev.set_hit_capacity(4 * v.shape[1])
    bundle = lambda: RayBundle(vertices=v, directions=d, energy=e)
    dev.trace_fast(bundle(), 100, 1e-10, 1, accel=True, stream=True)
    h1 = dev.get_hits()
    dev.trace_fast(bundle(), 100, 1e-10, 1, accel=True, stream=True)
    dev.trace_fast(bundle(), 100, 1e-10, 1, accel=True, stream=False)        # the megakernel appends behind the chunks
    h3 = dev.get_hits()
    n_cap = int(tl_b[2][30])
    assert len(h1['surf']) == n_cap and N.all(h1['surf'] == 30) and N.isclose(h1['e_abs'].sum(), tl_b[0][30], rtol=1e-12)
    assert len(h3['surf']) == 3 * n_cap and N.isclose(h3['e_abs'].sum(), 3 * tl_b[0][30], rtol=1e-12)
    key = lambda h: N.sort(N.round(h['points'][0] * 1e6) + 1e3 * N.round(h['points'][1] * 1e6))
    assert N.array_equal(key(h3)[::3], key(h1))                             # the same hit points three times
    _cabi_check = __import__('tracer_amd')._cabi.check
    _cabi_check(dev.lib.trc_scene_clear_hits(dev.handle))
    assert len(dev.get_hits()['surf']) == 0
    dev.trace_fast(bundle(), 100, 1e-10, 1, accel=True, stream=True)
    h4 = dev.get_hits()
    assert len(h4['surf']) == n_cap and N.array_equal(key(h4), key(h1))
    dev.close()
    # the streaming kernels walking the caller's Kd-tree instead of the grid (TRC_STREAM_SEARCH=1)
    os.environ['TRC_STREAM_SEARCH'] = '1'
    try:
        dev = DeviceScene(cs, ctx)
        dev.set_kdtree(kd)
        st_kd, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e), 100, 1e-10, 1, accel=True, stream=True)
        a_k, r_k, h_k = dev.get_tallies()
        dev.close()
    finally:
        del os.environ['TRC_STREAM_SEARCH']
    assert N.array_equal(h_k, tl_b[2]) and N.allclose(a_k, tl_b[0], rtol=1e-12, atol=1e-9) and st_kd.segments == st.segments
    for accel in (True, False):      # streaming engine, with the tree and with the single-leaf brute form
        dev = DeviceScene(cs, ctx)
        dev.set_kdtree(kd)
        st, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e), 100, 1e-10, 1, accel=accel, stream=True)
        a, r, h = dev.get_tallies()
        dev.close()
        assert N.array_equal(h, tl_b[2]) and N.allclose(a, tl_b[0], rtol=1e-12, atol=1e-9), accel


def test_kdtree_traversal_standalone(ctx):
    """KdTree.traversal(bundle) on the device == the reference's own relevancy matrix (fixture) and == the oracle on 20000 more rays"""
    from tracer_amd import scenes
    from tracer_amd.accel_tree import KdTree
    from tracer_amd.ray_bundle import RayBundle
    from oracle import accel
    g = load('kdtree_nsttf.npz')
    plant, field, rec, src = scenes.nsttf_field(sigma=0.)
    S = len(plant.get_surfaces())
    kd = KdTree(plant, 8 + 1.3 * N.log(S), min_leaf=1)
    v, d = g['trav_vertices'], g['trav_directions']
    any_inter, rel = kd.traversal(RayBundle(vertices=v, directions=d, energy=N.ones(v.shape[1])))
    assert rel.dtype == bool and rel.shape == (S, v.shape[1])
    assert any_inter == bool(g['trav_any'])
    assert N.array_equal(rel, N.unpackbits(g['trav_relevancy_bits'], axis=1)[:, :v.shape[1]].astype(bool))
    # more rays, against the restatement: the sun's rays over the whole field
    b = scenes.nsttf_source(20000, src, seed=5)
    any2, rel2 = kd.traversal(b)
    with N.errstate(all='ignore'):
        any_o, rel_o = accel.traversal(kd.flat(), S, N.asarray(b.get_vertices()), N.asarray(b.get_directions()))
    assert any2 == any_o and N.array_equal(rel2, rel_o)
    assert rel2[:-1].any(axis=0).sum() > 5000
    # lightweight=True (accel_tree.py:227-233, :281-286, :301-305): per surface, batches of ray numbers in the order of the leaves a
    # ray passes.  Every (surface, ray) pair the matrix marks appears in exactly one batch, and nothing else does; a ray's batch
    # number for a surface is the count of leaves it passed before the first one that lists the surface.
    sub = RayBundle(vertices=v[:, :300], directions=d[:, :300], energy=N.ones(300))
    any_l, lists = kd.traversal(sub, lightweight=True)
    assert any_l == any_inter and len(lists) == S
    back = N.zeros((S, 300), dtype=bool)
    first_batch = N.full((S, 300), -1)
    for s_i, batches in enumerate(lists):
        flat = [r for bt in batches for r in bt]
        assert len(flat) == len(set(flat)), "a ray is listed once per surface"
        for k, bt in enumerate(batches):
            back[s_i, bt] = True
            first_batch[s_i, bt] = k
    assert N.array_equal(back, rel[:, :300])
    always = N.asarray(kd.always_relevant, dtype=int)
    assert (first_batch[always] == 0).all()
    crossing = N.nonzero(rel[:-1, :300].any(axis=0))[0]
    assert len(crossing) > 20 and first_batch[:-1][:, crossing].max() >= 1, "some rays meet a mirror in the second leaf they cross or later"


def test_full_size_properties(ctx):
    """
    Benchmark-size run (NSTTF, 1e7 rays -- the per-GPU share of configs[3]) checked through size-independent
    properties: energy conservation, accel == brute force, flux map == receiver tally, hit buffer == tally, and
    the Monte-Carlo mean against the reference's own runs (tests/golden/mc_reference.npz, 3 sigma).
    """
    from tracer_amd import scenes
    from tracer_amd.tracer_engine import TracerEngine
    n = 10 ** 7
    plant, field, rec, src = scenes.nsttf_field()
    eng = TracerEngine(plant)
    ue, ve = scenes.nsttf_fluxmap_edges()
    eng.set_fluxmap(218, ue, ve)
    out = {}
    # brute force and accelerated on the streaming kernels (the default at this size), accelerated on the megakernel
    for key, accel, kern in (('brute', False, 'auto'), ('mega', True, 'megakernel'), ('accel', True, 'auto')):
        eng.reset_tallies(); plant.reset_all_optics()
        eng.ray_tracer(scenes.nsttf_source(n, src, seed=31), reps=100, min_energy=1e-10, tree=False, accel=accel, seed=31,
                       fast_kernel=kern)
        a, r, h = eng.get_tallies()
        out[key] = (a.copy(), r.copy(), h.copy(), eng.get_fluxmap(218).copy(), dict(eng.stats))
    (a0, r0, h0, f0, s0), (a1, r1, h1, f1, s1) = out['brute'], out['accel']
    assert N.array_equal(h0, h1) and s0['segments'] == s1['segments']
    assert N.allclose(a0, a1, rtol=1e-10) and N.allclose(f0, f1, rtol=1e-9, atol=1e-9)
    # the same rays handed over as a host bundle (two batches in flight index the caller's arrays by batch offset)
    from tracer_amd.ray_bundle import RayBundle
    lazy = scenes.nsttf_source(n, src, seed=31)
    given = RayBundle(vertices=lazy.get_vertices(), directions=lazy.get_directions(), energy=lazy.get_energy())
    eng.reset_tallies(); plant.reset_all_optics()
    eng.ray_tracer(given, reps=100, min_energy=1e-10, tree=False, accel=True, seed=31)
    a3, r3, h3 = eng.get_tallies()
    assert N.array_equal(h3, h1) and N.allclose(a3, a1, rtol=1e-10) and eng.stats['segments'] == s1['segments']
    del given, lazy
    a2, r2, h2, f2, s2 = out['mega']
    assert N.array_equal(h2, h1) and s2['segments'] == s1['segments'] and s2['launches'] == 1 and s1['launches'] > 1
    assert N.allclose(a2, a1, rtol=1e-10) and N.allclose(f2, f1, rtol=1e-9, atol=1e-9)
    # energy: what a surface received is absorbed or reflected; reflected energy is received downstream or escapes
    assert N.all(a1 <= r1 * (1 + 1e-12))
    e_ray = 1000. * N.pi * src['radius'] ** 2 / n
    # every ray that lands anywhere carries e_ray (straight from the source) or 0.96 e_ray (one mirror reflection):
    # one-sided mirrors absorb everything on their back and the receiver absorbs everything
    assert N.all(r1 >= 0.96 * e_ray * h1 * (1 - 1e-12)) and N.all(r1 <= e_ray * h1 * (1 + 1e-12))
    assert n <= s1['segments'] <= n + h1[:218].sum()                         # only mirror hits can spawn another segment
    assert N.isclose(f1.sum(), a1[218], rtol=1e-9)                           # all receiver hits fall on the 11 x 11 m map
    hits = rec.get_surfaces()[0].get_optics_manager().get_all_hits()
    assert len(hits[0]) == h1[218] and N.isclose(hits[0].sum(), a1[218], rtol=1e-9)
    loc = rec.get_surfaces()[0].global_to_local(hits[1])
    assert N.abs(loc[0]).max() <= 5.5 + 1e-9 and N.abs(loc[1]).max() <= 5.5 + 1e-9 and N.abs(loc[2]).max() < 1e-6
    H2 = N.histogram2d(loc[0], loc[1], bins=[ue, ve], weights=hits[0])[0]
    assert N.allclose(H2, f1, rtol=1e-9, atol=1e-6)                           # device flux map == caller-side histogram2d
    mc = load('mc_reference.npz')
    p_ref, se_ref = mc['nsttf_receiver_mean'], mc['nsttf_receiver_se']
    # per-ray variance of the receiver power from the hit list -> standard error of this run
    se_gpu = N.sqrt(N.sum(hits[0] ** 2))
    assert abs(a1[218] - p_ref) <= 3. * N.sqrt(se_gpu ** 2 + se_ref ** 2), (a1[218], p_ref, se_gpu, se_ref)
    # flux map against the reference's own flux maps (mean of its 10 runs), in 5 x 5 groups of bins: configs[2] "flux map vs
    # reference".  Standard error here from the per-hit energies, there from the scatter of the runs (a 10-run estimate, so 5 sigma)
    grp = lambda m: m.reshape(10, 5, 10, 5).sum(axis=(1, 3))
    var_gpu = N.histogram2d(loc[0], loc[1], bins=[ue, ve], weights=hits[0] ** 2)[0]
    se_map = N.sqrt(grp(var_gpu) + grp(mc['nsttf_flux_se'] ** 2))
    dev_map = N.abs(grp(f1) - grp(mc['nsttf_flux_mean']))
    assert N.all(dev_map <= 5. * se_map + 1e-9), float((dev_map / N.maximum(se_map, 1e-30)).max())
    assert N.corrcoef(grp(f1).ravel(), grp(mc['nsttf_flux_mean']).ravel())[0, 1] > 0.995
    frac_ref, frac_se = mc['nsttf_bounce_fractions_mean'], mc['nsttf_bounce_fractions_se']
    frac = N.array([h1[:218].sum() / n, h1[218] / n])
    assert N.all(N.abs(frac - frac_ref) <= 4. * N.sqrt(frac_se ** 2 + frac * (1 - frac) / n)), (frac, frac_ref)


def test_mc_scenes_vs_reference_runs(ctx):
    """
    configs[1] (dish + Buie sunshape + radial slope error) and configs[0] (flat mirror, bi-variate slope error,
    pillbox source, Lambertian receiver) against the reference's own Monte-Carlo runs (tests/golden/mc_reference.npz):
    receiver power and focal-spot second moments within 3 sigma of the combined standard errors.
    """
    from tracer_amd import scenes
    from tracer_amd.tracer_engine import TracerEngine
    mc = load('mc_reference.npz')
    # dish, 1e7 rays (the size of configs[1])
    n = 10 ** 7
    asm, dish_s, rec_s, src = scenes.dish()
    eng = TracerEngine(asm)
    eng.ray_tracer(scenes.dish_source(n, src, seed=77), reps=10, min_energy=1e-10, tree=False, seed=77, hit_capacity=n + 1024)
    a, r, h = eng.get_tallies()
    en = rec_s.get_optics_manager().get_all_hits()[0]
    assert len(en) == h[1] and N.isclose(en.sum(), a[1], rtol=1e-9)
    se_gpu = N.sqrt(N.sum(en ** 2) * (1. - h[1] / float(n)))          # binomial thinning of n equal-energy rays
    assert abs(a[1] - mc['dish_receiver_mean']) <= 3. * N.sqrt(se_gpu ** 2 + mc['dish_receiver_se'] ** 2), (a[1], float(mc['dish_receiver_mean']))
    assert N.isclose(a[0], 0.06 * r[0], rtol=1e-9)                       # the dish absorbs 6 % of what it receives
    # flat pair, 1e6 rays: power and rms spot size on the receiver (slope error + sunshape broadening)
    n = 10 ** 6
    asm, mirror, rec, src = scenes.flat_pair()
    eng = TracerEngine(asm)
    eng.ray_tracer(scenes.flat_pair_source(n, src, seed=5), reps=10, min_energy=1e-10, tree=False, seed=5, hit_capacity=n + 1024)
    en, pts = rec.get_optics_manager().get_all_hits()
    loc = rec.global_to_local(pts)
    got = N.array([en.sum(), N.sqrt(N.mean(loc[0] ** 2)), N.sqrt(N.mean(loc[1] ** 2))])
    ref, se = mc['flat_receiver_mean'], mc['flat_receiver_se']
    # standard errors of this run: power from the hit list; rms from the fourth moment
    k = len(en)
    se_run = N.array([N.sqrt(N.sum(en ** 2) * (1. - k / float(n))),
                      N.sqrt(N.var(loc[0] ** 2) / k) / (2. * got[1]), N.sqrt(N.var(loc[1] ** 2) / k) / (2. * got[2])])
    assert N.all(N.abs(got - ref) <= 3. * N.sqrt(se ** 2 + se_run ** 2)), (got, ref, se, se_run)


def _cavity_scene():
    """configs[4]-like cavity: aperture annulus, frustum, cylinder and cone walls with angle/wavelength-dependent Lambertian
    optics, a conductor (metal) back plate and a spectrally selective mirror ring -- every table-driven optics kind"""
    from tracer_amd import _cabi as K
    from tracer_amd.scene import TableScene
    from tracer_amd.spatial_geometry import rotx, translate
    ths = N.linspace(0., N.pi / 2., 7)
    abth = N.array([0.9, 0.88, 0.85, 0.8, 0.7, 0.5, 0.1])
    wls = N.linspace(0.25e-6, 2.6e-6, 5)
    grid = 0.2 + 0.7 * N.outer(N.cos(ths) ** 0.5, 1. / (1. + (wls * 1e6 - 1.) ** 2))
    mlam = N.linspace(0.2e-6, 3e-6, 8)
    mn = N.array([0.1, 0.13, 0.2, 0.4, 0.9, 1.5, 2.4, 3.6])
    mk = N.array([2.0, 3.5, 5.0, 7.0, 9.5, 13., 18., 24.])
    slam = N.linspace(0.2e-6, 3e-6, 9)
    sab = N.array([0.1, 0.2, 0.15, 0.4, 0.9, 0.5, 0.3, 0.2, 0.25])
    tables = [N.concatenate((ths, abth)), N.concatenate(([len(ths), len(wls)], ths, wls, grid.ravel())),
              N.concatenate((mlam, mn, mk)), N.concatenate((slam, sab))]
    offs = N.concatenate(([0], N.cumsum([len(t) for t in tables])))
    extra = N.concatenate(tables)
    #            frustum 0<z<1 (r 1 -> 1.4)   cylinder 1<z<2.5 (r 1.4)                 cone back (apex at z=3.5)                    annulus at z=0           metal ring plate           spectral mirror disc
    gm_kind = [K.GM_FRUSTUM, K.GM_CYL_FINITE, K.GM_CONE_FINITE, K.GM_ROUND, K.GM_ROUND, K.GM_ROUND]
    frames = [N.eye(4), translate(0, 0, 1.75), N.dot(translate(0, 0, 3.5), rotx(N.pi)), N.eye(4), translate(0, 0, 2.2), translate(0.2, 0., 1.2)]
    gm = N.zeros((6, 16))
    c = (1.4 - 1.0) / (1.0 - 0.0)
    gm[0, :4] = c, (1.4 * 0. - 1.0 * 1.0) / (1.4 - 1.0), 0., 1.
    gm[1, :4] = 1.4, 0.75, 0., 2. * N.pi
    gm[2, :3] = 1.4 / 1.0, 0., 1.0
    gm[3, :2] = 1.6, 1.0
    gm[4, :2] = 0.6, 0.2
    gm[5, :2] = 0.3, -1.
    ok = [K.OPT_LAMBERTIAN_DIRECTIONAL_SPECTRAL, K.OPT_LAMBERTIAN_DIRECTIONAL, K.OPT_LAMBERTIAN_DIRECTIONAL_SPECTRAL, K.OPT_SEMI_LAMBERTIAN,
          K.OPT_FRESNEL_CONDUCTOR, K.OPT_REFLECTIVE_SPECTRAL]
    opt = N.zeros((6, 8))
    opt[3, :2] = 0.6, 0.9           # the aperture annulus: mirror beyond 0.9 rad of incidence, Lambertian (into 0.9 rad) below
    opt[4, 0] = 1.0
    which = [1, 0, 1, -1, 2, 3]
    eoff = N.array([offs[w] if w >= 0 else -1 for w in which])
    elen = N.array([len(tables[w]) if w >= 0 else 0 for w in which])
    return TableScene(gm_kind, ok, frames, gm, opt, extra, eoff, elen)


def test_minidish_example_vs_reference_runs(ctx):
    """
    The scene of examples/test_case.py (models/tau_minidish.py: tilted dish, homogenizer duct, one-sided receiver) against ten
    runs of the reference itself on it (tests/golden/mc_minidish.npz, made by make_golden.py --mc-minidish): power on the plate,
    power absorbed by each duct wall, the 20 x 20 flux map bin by bin, the size of every level of the ray tree.
    """
    import math
    from tracer_amd.models.tau_minidish import MiniDish
    from tracer_amd.sources import solar_disk_bundle
    from tracer_amd.spatial_geometry import rotx
    from tracer_amd.tracer_engine import TracerEngine
    mc = load('mc_minidish.npz')
    x = -1 / math.sqrt(2)

    def scene():
        dish = MiniDish(5., 6.25, 0.9, 6.95, 0.4, 0.7, 0.9)
        dish.set_transform(rotx(-N.pi / 4))
        return dish, dish.get_receiver_surf().get_surfaces()[0]

    # fast engine, 2e7 rays, flux map binned on the device: its own Monte-Carlo error is a seventh of the reference's
    n = 20000000
    dish, plate = scene()
    eng = TracerEngine(dish)
    edges = N.linspace(-0.2, 0.2, 21)
    eng.set_fluxmap(plate, edges, edges)
    eng.ray_tracer(solar_disk_bundle(n, N.c_[[0, 7., 7.]], N.array([0, x, x]), 3., 0.005, flux=1000., seed=41), 100, 1e-6,
                   tree=False, feed=False, seed=41)
    a, r, h = eng.get_tallies()
    surfs = dish.get_surfaces()
    ip = surfs.index(plate)
    shrink = math.sqrt(10 * float(mc['rays_per_run']) / n)
    se = float(mc['receiver_se']) * math.sqrt(1. + shrink ** 2)
    assert abs(a[ip] - float(mc['receiver_mean'])) <= 4. * se, (a[ip], float(mc['receiver_mean']), se)
    walls = [surfs.index(w) for w in dish.get_homogenizer().get_surfaces()]
    assert N.all(N.abs(a[walls] - mc['walls_mean']) <= 4. * mc['walls_se'] * math.sqrt(1. + shrink ** 2)), (a[walls], mc['walls_mean'])
    # the map: bins the sun reaches, each against the reference's mean with the reference's standard error (9 degrees of freedom)
    got = eng.get_fluxmap(plate)
    assert abs(got.sum() - a[ip]) < 1e-6 * a[ip]
    lit = mc['map_se'] > 0
    z = (got[lit] - mc['map_mean'][lit]) / (mc['map_se'][lit] * math.sqrt(1. + shrink ** 2))
    assert lit.sum() > 300 and abs(z.mean()) < 0.3 and N.mean(z ** 2) < 2.2 and N.abs(z).max() < 8., (z.mean(), N.mean(z ** 2), N.abs(z).max())
    # ordered engine, the call of the script word for word: level sizes of the ray tree, and the same power through histogram_hits
    n = 1000000
    dish, plate = scene()
    eng = TracerEngine(dish)
    eng.ray_tracer(solar_disk_bundle(n, N.c_[[0, 7., 7.]], N.array([0, x, x]), 3., 0.005, flux=1000., seed=42), 100, 1e-6, seed=42)
    sizes = N.array([b.get_num_rays() for b in eng.tree._bunds][:5], dtype=float)
    frac, frac_ref = sizes / n, mc['levels_mean'] / float(mc['rays_per_run'])
    frac_se = N.sqrt((mc['levels_se'] / float(mc['rays_per_run'])) ** 2 + frac * (1 - frac) / n)
    assert N.all(N.abs(frac - frac_ref) <= 4. * frac_se + 1e-12), (frac, frac_ref)
    hist = dish.histogram_hits(bins=20)[0]
    assert abs(hist.sum() - float(mc['receiver_mean'])) <= 4. * float(mc['receiver_se']) * math.sqrt(2.), hist.sum()


def test_plates_example_vs_reference_runs(ctx):
    """
    examples/accel_tree_example.py (a thousand Lambertian plates in ten layers over a slab; up to a dozen diffuse bounces per ray)
    against eight runs of the reference itself (tests/golden/mc_plates.npz, make_golden.py --mc-plates): power absorbed in total,
    by the slab, by each layer -- the ordered engine with the example's own call, the fast engine in both forms.
    """
    import math
    from helpers import plates_scene, plates_source
    from tracer_amd.tracer_engine import TracerEngine
    mc = load('mc_plates.npz')
    asm, layers, side = plates_scene()
    eng = TracerEngine(asm)

    def rows(per):
        return N.r_[per.sum(), per[1], per[2:].reshape(10, 100).sum(axis=1)]

    def check(got, n, what):
        grow = math.sqrt(1. + 8 * float(mc['rays_per_run']) / n)
        z = (got - mc['mean']) / (mc['se'] * grow)
        assert N.abs(z).max() < 4.5, (what, z)

    # min_energy is an energy per ray: the example's default of 0.05 W on 2e4 rays of 6.05 W each is kept in proportion
    n = 400000
    asm.reset_all_optics()
    eng.ray_tracer(plates_source(n, layers, side, 51), 1000, 0.05 * float(mc['rays_per_run']) / n, accel=True, seed=51)
    assert eng.stats['engine'] == 'ordered'
    check(rows(N.array([N.sum(s.get_optics_manager().get_all_hits()[0]) for s in asm.get_surfaces()])), n, 'ordered')
    n = 4000000
    for form in ('megakernel', 'stream'):
        asm.reset_all_optics()
        eng.reset_tallies()
        eng.ray_tracer(plates_source(n, layers, side, 52), 1000, 0.05 * float(mc['rays_per_run']) / n, accel=True, seed=52, tree=False,
                       fast_kernel=form, feed=False)
        a, r, h = eng.get_tallies()
        check(rows(a), n, form)


def test_cavity_spectral_engines_vs_oracle(ctx):
    """cavity scene (frustum / cylinder / cone / plates, table-driven spectral and directional optics, per-ray wavelengths):
    ordered and fast engines against the oracle, ray by ray, on identical Philox streams"""
    from oracle import engine
    from tracer_amd.scene import DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    ts = _cavity_scene()
    rng = N.random.RandomState(12)
    n = 5000
    # rays entering through the aperture (r < 1 at z = -0.5) with a spread of directions and wavelengths
    rr, ph = N.sqrt(rng.uniform(0, 0.9, n)), rng.uniform(0, 2 * N.pi, n)
    v = N.vstack((rr * N.cos(ph), rr * N.sin(ph), -0.5 * N.ones(n)))
    d = N.vstack((rng.normal(scale=0.35, size=n), rng.normal(scale=0.35, size=n), N.ones(n)))
    d /= N.sqrt(N.sum(d ** 2, axis=0))
    e = rng.uniform(0.5, 1.5, n)
    wl = rng.uniform(0.3e-6, 2.5e-6, n)
    seed, reps, emin = 99, 12, 1e-3
    dev = DeviceScene(ts, ctx)
    res, stats = dev.trace_ordered(RayBundle(vertices=v, directions=d, energy=e, wavelengths=wl), reps, emin, seed)
    levels = [res.level(k, with_wavelength=True) for k in range(res.num_levels())]
    res.close()
    a_o, r_o, h_o = dev.get_tallies()
    ref = engine.trace_bundle(ts, v, d, e, reps, emin, seed, wavelengths=wl)
    assert [l['vertices'].shape[1] for l in levels] == [l['vertices'].shape[1] for l in ref['levels']]
    assert len(levels) >= 6 and (ref['hits'] > 50).all(), "every surface kind of the cavity takes part"
    for k in range(1, len(levels)):
        L, O = levels[k], ref['levels'][k]
        assert N.array_equal(L['parents'], O['parents']) and N.array_equal(L['surf'], O['surf']), k
        assert N.allclose(L['vertices'], O['vertices'], rtol=RT, atol=AT), k
        assert N.allclose(L['directions'], O['directions'], rtol=1e-8, atol=1e-8), k
        assert N.allclose(L['energy'], O['energy'], rtol=RT, atol=1e-12), k
        assert N.allclose(L['wavelengths'], O['wl']), k
    assert N.array_equal(h_o, ref['hits']) and N.allclose(a_o, ref['absorbed'], rtol=1e-9, atol=1e-9)
    dev.reset_tallies()
    st, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e, wavelengths=wl), reps, emin, seed)
    a, r, h = dev.get_tallies()
    dev.close()
    assert N.array_equal(h, ref['hits']) and N.allclose(a, ref['absorbed'], rtol=1e-9, atol=1e-9) and st.segments == ref['segments']
    dev = DeviceScene(ts, ctx)
    st, _ = dev.trace_fast(RayBundle(vertices=v, directions=d, energy=e, wavelengths=wl), reps, emin, seed, stream=True)
    a, r, h = dev.get_tallies()
    dev.close()
    assert N.array_equal(h, ref['hits']) and N.allclose(a, ref['absorbed'], rtol=1e-9, atol=1e-9) and st.segments == ref['segments']


def test_random_scenes_all_searches_agree(ctx):
    """
    Scenes of 60 surfaces of mixed kinds at random poses -- clustered, with a few far outliers and two infinite planes --
    traced with every candidate search of the fast engine: brute force on the megakernel (the reference's default
    semantics), brute force and the uniform grid on the streaming kernels.  Per-surface hit counts must be identical and
    energies equal to rounding: the single-precision searches may only ever add candidates, never lose one.
    """
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM, FlatGeometryManager
    from tracer_amd.triangular_face import TriangularFace
    from tracer_amd.paraboloid import ParabolicDishGM, RectangularParabolicDishGM
    from tracer_amd.sphere_surface import SphericalGM, HemisphereGM, CutSphereGM
    from tracer_amd.boundary_shape import BoundaryPlane
    from tracer_amd.cylinder import FiniteCylinder
    from tracer_amd.cone import FiniteCone, ConicalFrustum
    from tracer_amd.ellipsoid import EllipsoidGM
    from tracer_amd.polygon import FlatSimplePolygonGM
    from tracer_amd.spatial_geometry import general_axis_rotation
    from tracer_amd import optics_callables as opt
    from tracer_amd.scene import compile_scene, DeviceScene
    from tracer_amd.ray_bundle import RayBundle

    makers = [lambda r: RectPlateGM(r.uniform(0.5, 3.), r.uniform(0.5, 3.)),
              lambda r: RoundPlateGM(r.uniform(0.5, 2.)),
              lambda r: TriangularFace(N.array([[r.uniform(1, 2), 0.], [r.uniform(-0.5, 0.5), r.uniform(1, 2)], [0., 0.]])),
              lambda r: ParabolicDishGM(r.uniform(1., 3.), r.uniform(1., 4.)),
              lambda r: RectangularParabolicDishGM(r.uniform(1., 2.), r.uniform(1., 2.), r.uniform(2., 5.)),
              lambda r: SphericalGM(r.uniform(0.3, 1.5)),
              lambda r: HemisphereGM(r.uniform(0.5, 1.5)),
              lambda r: CutSphereGM(2., BoundaryPlane(location=N.r_[0., 0., r.uniform(0.5, 1.5)])),
              lambda r: FiniteCylinder(r.uniform(0.5, 2.), r.uniform(0.5, 3.)),
              lambda r: FiniteCone(r.uniform(0.3, 1.), r.uniform(0.5, 2.)),
              lambda r: ConicalFrustum(0., r.uniform(0.3, 1.), r.uniform(0.5, 2.), r.uniform(1.1, 2.)),
              lambda r: EllipsoidGM(r.uniform(0.5, 1.5), r.uniform(0.5, 1.5), r.uniform(0.5, 1.5), zlim=[-0.5, 0.4]),
              lambda r: FlatSimplePolygonGM(N.array([[-1., -1., 0.2, 0.2, 1.2, 1.2], [-0.8, 1., 1., 0.1, 0.1, -0.8]]) * r.uniform(0.8, 2.))]
    for seed in (1, 2, 3):
        r = N.random.RandomState(seed)
        objs = []
        for k in range(60):
            gm = makers[k % len(makers)](r)
            optics = opt.Reflective(0.3) if k % 3 else opt.Lambertian(0.5)
            axis = r.normal(size=3)
            axis /= N.linalg.norm(axis)
            # most surfaces in a 24 m cube, every 20th far away (set apart from the grid or stretching it)
            centre = r.uniform(-12., 12., size=3) if k % 20 else r.uniform(-1., 1., size=3) * 25. + N.r_[0., 0., 90.]
            objs.append(AssembledObject(surfs=[Surface(gm, optics)], transform=N.vstack((
                N.hstack((general_axis_rotation(axis, r.uniform(0, 2 * N.pi)), centre[:, None])), N.r_[[0., 0., 0., 1.]]))))
        for z, a in ((-14., 1.), (110., 0.6)):         # two unbounded planes closing the scene below and above
            objs.append(AssembledObject(surfs=[Surface(FlatGeometryManager(), opt.Reflective(a))],
                                        transform=N.vstack((N.hstack((N.eye(3), N.c_[[0., 0., z]])), N.r_[[0., 0., 0., 1.]]))))
        cs = compile_scene(Assembly(objects=objs))
        n = 300000
        o = r.normal(size=(3, n))
        o = o / N.sqrt((o ** 2).sum(axis=0)) * 40.
        tgt = r.uniform(-14., 14., size=(3, n))
        d = tgt - o
        d /= N.sqrt((d ** 2).sum(axis=0))
        d[:, :3] = N.eye(3)                          # axis-parallel rays too
        e = N.ones(n)
        res = {}
        for key, accel, stream in (('mega_brute', False, False), ('stream_brute', False, True), ('stream_grid', True, True)):
            dev = DeviceScene(cs, ctx)
            st, _ = dev.trace_fast(RayBundle(vertices=o, directions=d, energy=e), 12, 1e-6, 5, accel=accel, stream=stream)
            res[key] = dev.get_tallies() + (st.segments,)
            dev.close()
        a0, r0, h0, s0 = res['mega_brute']
        assert h0.sum() > n and (h0[:60] > 0).sum() > 40          # the scene is actually hit, many bounces
        for key in ('stream_brute', 'stream_grid'):
            a1, r1, h1, s1 = res[key]
            assert N.array_equal(h1, h0) and s1 == s0, (seed, key, N.nonzero(h1 != h0)[0][:5])
            assert N.allclose(a1, a0, rtol=1e-9, atol=1e-9) and N.allclose(r1, r0, rtol=1e-9, atol=1e-9), (seed, key)


def test_streaming_edge_scenes(ctx):
    """the streaming form on scenes without any bounded surface, with a single bounded surface, reps=1 and odd ray counts"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, FlatGeometryManager
    from tracer_amd.spatial_geometry import translate, rotx
    from tracer_amd import optics_callables as opt
    from tracer_amd.scene import compile_scene, DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    r = N.random.RandomState(4)
    planes = [AssembledObject(surfs=[Surface(FlatGeometryManager(), opt.Reflective(0.1))], transform=translate(0, 0, -1.)),
              AssembledObject(surfs=[Surface(FlatGeometryManager(), opt.Reflective(0.1))], transform=N.dot(translate(0, 0, 1.), rotx(N.pi)))]
    plate = AssembledObject(surfs=[Surface(RectPlateGM(1., 1.), opt.Reflective(0.5))])
    for objs, n, reps in ((planes, 1001, 7), (planes + [plate], 777, 5), ([plate], 130, 1), ([plate], 64, 3)):
        cs = compile_scene(Assembly(objects=objs))
        o = N.vstack((r.uniform(-2, 2, n), r.uniform(-2, 2, n), r.uniform(-0.9, 0.9, n)))
        d = r.normal(size=(3, n))
        d /= N.sqrt((d ** 2).sum(axis=0))
        res = []
        for accel, stream in ((False, False), (True, True), (False, True)):
            dev = DeviceScene(cs, ctx)
            st, last = dev.trace_fast(RayBundle(vertices=o, directions=d, energy=N.ones(n)), reps, 1e-3, 9, accel=accel, stream=stream, keep_last=True)
            res.append(dev.get_tallies() + (st.segments, st.rays_left, N.sort(last[6]) if st.rays_left else N.zeros(0)))
            dev.close()
        for k in (1, 2):
            assert N.array_equal(res[k][2], res[0][2]) and res[k][3] == res[0][3] and res[k][4] == res[0][4], (len(objs), n, reps, k)
            assert N.allclose(res[k][0], res[0][0], rtol=1e-12) and N.allclose(res[k][5], res[0][5], rtol=1e-12)


def test_many_surfaces_scene(ctx):
    """1500 small plates: the per-workgroup tables of the streaming kernels need more than 64 KB of LDS (boxes, grid,
    records, tallies); grid search == brute force on both forms of the fast engine"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd.spatial_geometry import general_axis_rotation
    from tracer_amd import optics_callables as opt
    from tracer_amd.scene import compile_scene, DeviceScene
    from tracer_amd.ray_bundle import RayBundle
    r = N.random.RandomState(11)
    objs = []
    for k in range(1500):
        gm = RectPlateGM(r.uniform(0.5, 2.), r.uniform(0.5, 2.)) if k % 2 else RoundPlateGM(r.uniform(0.4, 1.2))
        axis = r.normal(size=3)
        axis /= N.linalg.norm(axis)
        tr = N.vstack((N.hstack((general_axis_rotation(axis, r.uniform(0, 2 * N.pi)), r.uniform(-30., 30., size=(3, 1)))), N.r_[[0., 0., 0., 1.]]))
        objs.append(AssembledObject(surfs=[Surface(gm, opt.Reflective(0.4) if k % 5 else opt.Lambertian(0.6))], transform=tr))
    cs = compile_scene(Assembly(objects=objs))
    n = 200000
    o = r.normal(size=(3, n))
    o = o / N.sqrt((o ** 2).sum(axis=0)) * 70.
    d = r.uniform(-30., 30., size=(3, n)) - o
    d /= N.sqrt((d ** 2).sum(axis=0))
    res = {}
    for key, accel, stream in (('mega_brute', False, False), ('stream_grid', True, True), ('stream_brute', False, True)):
        dev = DeviceScene(cs, ctx)
        st, _ = dev.trace_fast(RayBundle(vertices=o, directions=d, energy=N.ones(n)), 6, 1e-6, 3, accel=accel, stream=stream)
        res[key] = dev.get_tallies() + (st.segments, st.launches)
        dev.close()
    a0, r0, h0, s0, l0 = res['mega_brute']
    assert h0.sum() > 0.25 * n and l0 == 1
    for key in ('stream_grid', 'stream_brute'):
        a1, r1, h1, s1, l1 = res[key]
        assert l1 > 1 and N.array_equal(h1, h0) and s1 == s0, key
        assert N.allclose(a1, a0, rtol=1e-9, atol=1e-9), key


@pytest.mark.gpu
def test_transfer_matrix_equals_the_tree_of_the_oracle():
    """
    Surface-to-surface energy transfer (the blocking / shading post-process of the reference's NSTTF example,
    examples/Sandia_NSTTF_field example.py:229-290): the matrix the fast engine accumulates while shading -- streaming form
    and megakernel -- equals the one read off the oracle's ray tree (parents and producing surfaces) for the same Philox
    streams, and the ordered engine's tree gives it too.  Then the example's per-heliostat quantities.
    """
    from oracle import engine as oeng
    from tracer_amd import scenes
    from tracer_amd.scene import compile_scene
    from tracer_amd.tracer_engine import TracerEngine
    from tracer_amd.models.heliostat_field import field_losses
    plant, field, rec, src = scenes.nsttf_field()
    cs = compile_scene(plant)
    S = cs.n_surf
    n = 200000
    bundle = scenes.nsttf_source(n, src, seed=21)
    ref = oeng.trace_from_compiled(cs, bundle.source_args(), 100, 1e-10)
    T_ref = N.zeros((S + 1, S))
    left = N.full(n, S)
    for lv in range(1, len(ref['levels'])):
        L, P = ref['levels'][lv], ref['levels'][lv - 1]
        N.add.at(T_ref, (left[L['parents']], L['surf']), P['energy'][L['parents']])
        left = L['surf']
    assert N.isclose(T_ref.sum(), ref['received'].sum(), rtol=1e-12) and T_ref[S].sum() > 0 and T_ref[:S].sum() > 0

    eng = TracerEngine(plant)
    eng.enable_transfer_matrix()
    for kernel in ('megakernel', 'stream'):
        eng.reset_tallies()
        eng.ray_tracer(scenes.nsttf_source(n, src, seed=21), reps=100, min_energy=1e-10, tree=False, accel=True, seed=21, fast_kernel=kernel)
        T = eng.get_transfer_matrix()
        assert T.shape == (S + 1, S)
        assert N.array_equal(T != 0., T_ref != 0.), kernel
        assert N.allclose(T, T_ref, rtol=1e-9, atol=1e-9), (kernel, N.abs(T - T_ref).max())
        a, r, h = eng.get_tallies()
        assert N.allclose(T.sum(axis=0), r, rtol=1e-9)                  # what lands on a surface is what it receives
    eng.reset_tallies()
    eng.ray_tracer(scenes.nsttf_source(n, src, seed=21), reps=100, min_energy=1e-10, tree=True, seed=21)
    assert N.allclose(eng.get_transfer_matrix(), T_ref, rtol=1e-9, atol=1e-9)

    # per-heliostat quantities of the example: every heliostat is one surface, the receiver is the last one
    surfaces = plant.get_surfaces()
    rec_idx = [surfaces.index(s) for s in rec.get_surfaces()] if hasattr(rec, 'get_surfaces') else [S - 1]
    hel_idx = [i for i in range(S) if i not in rec_idx]
    res = field_losses(T_ref, hel_idx, rec_idx, flux=1000., projected_areas=N.ones(len(hel_idx)))
    assert res['incoming'].sum() == T_ref[S, hel_idx].sum() and (res['incoming'] > 0).sum() > 200
    assert res['blocking'].sum() > 0 and res['blocking'].sum() < 0.05 * res['incoming'].sum()
    assert N.isclose(res['to_receiver'].sum(), T_ref[:S, rec_idx].sum())
    assert N.allclose(res['shading'], 1000. - res['incoming'])
    # switching it off frees the rows: the plain tallies are unchanged by it
    eng.enable_transfer_matrix(False)
    with pytest.raises(ValueError):
        eng.get_transfer_matrix()


_EXCHANGE_SCRIPT = r"""
import sys
import numpy as N
import torch
torch.cuda.init()                 # torch's HIP runtime first, as in bench.py: initialised second it finds no GPU
sys.path.insert(0, sys.argv[1])
from tracer_amd import _cabi, scenes
from tracer_amd.scene import compile_scene, DeviceScene
ctx = _cabi.get_context(0)
plant, field, rec, src = scenes.nsttf_field(n_heliostats=30)
cs = compile_scene(plant)
dev = DeviceScene(cs, ctx)
ue, ve = scenes.nsttf_fluxmap_edges()
rec_index = plant.get_surfaces().index(rec.get_surfaces()[0])
dev.set_fluxmap(rec_index, ue, ve)
dev.enable_transfer(True)
dev.trace_fast(scenes.nsttf_source(300000, src, seed=3), 100, 1e-10, 3, accel=True)
a0, r0, h0 = dev.get_tallies()
fm0, T0 = dev.get_fluxmap(rec_index), dev.get_transfer()
n = dev.tally_size()
S = cs.n_surf
assert n == 3 * S + 2 + (len(ue) - 1) * (len(ve) - 1) + (S + 1) * S
assert a0.sum() > 0 and fm0.sum() > 0 and T0.sum() > 0
t = torch.empty(n, dtype=torch.float64, device='cuda')
dev.export_tallies(out=t.data_ptr())
torch.cuda.synchronize()
host = dev.export_tallies()
assert N.array_equal(t.cpu().numpy(), host)
t += t                                   # the "all-reduce" with a second rank that traced the same
torch.cuda.synchronize()
dev.import_tallies(t.data_ptr())
a1, r1, h1 = dev.get_tallies()
assert N.array_equal(a1, 2 * a0) and N.array_equal(r1, 2 * r0) and N.array_equal(h1, 2 * h0)
assert N.array_equal(dev.get_fluxmap(rec_index), 2 * fm0) and N.array_equal(dev.get_transfer(), 2 * T0)
dev.import_tallies(host)
assert N.array_equal(dev.get_tallies()[0], a0)
dev.close()
print('EXCHANGE OK')
"""


@pytest.mark.gpu
def test_packed_tallies_round_trip_through_device_memory():
    """
    The exchange step of the multi-GPU path without the other GPUs: the packed tally buffer (per-surface energies and counts,
    segment / hit totals, flux-map bins, transfer matrix) exported into a torch tensor on the device -- what
    distributed.reduce_scene_tallies hands to the RCCL all-reduce -- summed with itself there and imported again doubles every
    tally; through a host array the same.  In a process of its own, torch first (the order bench.py uses).
    """
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, '-c', _EXCHANGE_SCRIPT, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'EXCHANGE OK' in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.mark.gpu
def test_staged_buie_inversion_across_csr(ctx):
    """
    The generation kernel of the streaming form inverts the Buie distribution from per-bin folded records and a first-guess
    table (trc_buie_theta_fast); the megakernel uses the plain bisection (trc_buie_theta).  Same scene, same Philox streams,
    CSR from 0 (no aureole) to 0.3, disc and rectangular sources: identical hit counts, tallies equal to rounding.
    """
    from tracer_amd import scenes, sources
    from tracer_amd.scene import compile_scene, DeviceScene
    plant, field, rec, src = scenes.nsttf_field(n_heliostats=40)
    cs = compile_scene(plant)
    n = 400000
    for csr, pre in ((0., True), (0.01, False), (0.05, True), (0.3, True)):
        for shape in ('disc', 'rect'):
            def bundle():
                if shape == 'disc':
                    return sources.buie_sunshape(n, src['center'], src['direction'], 60., csr, flux=1000., pre_process_CSR=pre, seed=17)
                return sources.rect_buie_sunshape(n, src['center'], src['direction'], 100., 80., csr, flux=1000., pre_process_CSR=pre, seed=17)
            res = []
            for stream in (False, True):
                dev = DeviceScene(cs, ctx)
                st, _ = dev.trace_fast(bundle(), 100, 1e-10, 17, accel=True, stream=stream)
                a, r, h = dev.get_tallies()
                dev.close()
                res.append((st.segments, h.copy(), a.copy()))
            assert res[0][0] == res[1][0] and N.array_equal(res[0][1], res[1][1]), (csr, shape)
            assert N.allclose(res[0][2], res[1][2], rtol=1e-9, atol=1e-9), (csr, shape)
            assert res[0][1].sum() > 1000
