"""
Scenes whose optics send two rays on from a hit (RefractiveHomogenous(single_ray=False) and its family), for the streaming form of the
fast engine (k_s_shade_x<.., SPLIT>, csrc/trc_shade.hip), and their host reference: test_split_cases_host.py for what can be said
without a device, test_gpu_split.py on one.

Every bundle starts uniformly in [-1, 1]^2 at z = 2, tilted by up to 0.3 in x and y about -z, with energy 1 / n.

  slab         two RectPlateGM(8, 8) faces of RefractiveHomogenous(1, 1.5, single_ray=False) at z = 0.5 and z = 0 over a black floor
               (LambertianReceiver(1.), RectPlateGM(12, 12), z = -1) that captures.  n = 256, reps 8: every hit on a face splits
  slab_recv    the same with RefractiveHomogenousReceiver faces: more captured hits than the default room of 2 n + 1024
  slab_sigma   slab with a slope error on the faces (sigma = 2e-3), n = 200 (no multiple of 64): the draws use the children's streams
  mixed        slab_sigma's faces between a mirror with slope error (RealReflective(0.1, 3e-3), z = -1) and a diffuse wall that captures
               (LambertianReceiver(0.5), z = 2.5, facing down).  n = 256, reps 10: the population grows from bounce to bounce
  wave         slab at normal incidence, n = 64, reps 3: every lane of the one wave splits in the same turn
  wave_big     the same with n = 16384: every ray of the batch takes a slot from the search stage and a second one from the shading
               kernel in the first bounce
  source       slab under a pending rect_bundle: stream ids of the first bounce are ray_offset + the ray's number
  material     RefractiveAbsorbant(single_ray=False) between tabulated materials: complex indices go with both rays.  n = 256, reps 6
  poly         slab under a polychromatic bundle (W = 5), n = 128, reps 4: the spectrum goes with both rays
  *_global     slab and mixed with one surface more, out of the rays' way, whose optics table is long enough to keep the shading
               kernel's tables out of LDS (as shade_cases.py's 'g-global' does)

No scene has coincident or near-tied surfaces, and no ray is left out of any comparison.
"""
import functools

import numpy as N

import fluxmap_scene as fs

MIN_ENERGY = 1e-12
SEED = 4
MAP_EDGES = (N.linspace(-1.5, 1.8, 7), N.linspace(-1.7, 1.5, 7))         # 6 x 6, clipped: some hits land outside
TABLE_LEN = 6000        # points of the long table: 96 000 bytes, beyond the 72 KiB up to which k_s_shade_x stages its tables

# name: (kind of scene, n, reps, kind of bundle)
CASES = {
    'slab': ('slab', 256, 8, 'given'),
    'slab_recv': ('slab_recv', 256, 8, 'given'),
    'slab_sigma': ('slab_sigma', 200, 8, 'given'),
    'mixed': ('mixed', 256, 10, 'given'),
    'wave': ('slab', 64, 3, 'normal'),
    'wave_big': ('slab', 16384, 3, 'normal'),
    'source': ('slab', 256, 8, 'source'),
    'material': ('material', 256, 6, 'material'),
    'poly': ('slab', 128, 4, 'poly'),
    'slab_global': ('slab+table', 256, 8, 'given'),
    'mixed_global': ('mixed+table', 256, 10, 'given'),
}
# the oracle's figures: hits per surface, segments, rays left, captured hits, largest number of live rays of a level
ORACLE = {
    'slab': ([1024, 1024, 768], 3840, 256, 768, 512),
    'slab_recv': ([1024, 1024, 768], 3840, 256, 2816, 512),
    'slab_sigma': ([800, 800, 600], 3000, 200, 600, 400),
    'mixed': ([8909, 13974, 6897, 8827], 41082, 19914, 8827, 19914),
}
W_POLY = 5


def materials():
    from tracer_amd import optics_callables as opt
    tl = N.linspace(0.3e-6, 2.5e-6, 6)
    return (opt.TabulatedMaterial(tl, N.ones(6), N.zeros(6)),
            opt.TabulatedMaterial(tl, [1.55, 1.53, 1.51, 1.50, 1.49, 1.47], [3e-8, 2e-8, 1e-8, 5e-8, 2e-7, 6e-7]))


def scene(kind):
    """(assembly, index of the surface that carries the flux map)"""
    from tracer_amd.assembly import Assembly
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM, RoundPlateGM
    from tracer_amd import optics_callables as opt
    from tracer_amd.spatial_geometry import translate, rotx
    kind, _, table = kind.partition('+')
    if kind == 'material':
        air, glass = materials()
        face = lambda: opt.RefractiveAbsorbant(air, glass, single_ray=False, attenuation_coefficient_1=1.)
        size = 40.
    else:
        cls = opt.RefractiveHomogenousReceiver if kind == 'slab_recv' else opt.RefractiveHomogenous
        sigma = 2e-3 if kind in ('slab_sigma', 'mixed') else None
        face = lambda: cls(1., 1.5, single_ray=False, sigma=sigma)
        size = 8.
    parts = [(RectPlateGM(size, size), face(), translate(0., 0., 0.5)), (RectPlateGM(size, size), face(), translate(0., 0., 0.))]
    if kind == 'mixed':
        parts += [(RectPlateGM(12., 12.), opt.RealReflective(0.1, 3e-3), translate(0., 0., -1.)),
                  (RectPlateGM(12., 12.), opt.LambertianReceiver(0.5), N.dot(translate(0., 0., 2.5), rotx(N.pi)))]
        map_surf = 3
    else:
        parts += [(RectPlateGM(60., 60.) if kind == 'material' else RectPlateGM(12., 12.), opt.LambertianReceiver(1.), translate(0., 0., -1.))]
        map_surf = 2
    if table:
        lam = N.linspace(0.2e-6, 2.6e-6, TABLE_LEN)
        parts += [(RoundPlateGM(0.5), opt.Reflective_spectral(0.2 + 0.5 * N.sin(3e6 * lam) ** 2, lam), translate(40., 40., 0.25))]
    return Assembly(objects=[AssembledObject(surfs=[Surface(gm, o)], transform=tr) for gm, o, tr in parts]), map_surf


def rays(n, normal=False, seed=3):
    rng = N.random.RandomState(seed)
    v = N.vstack((rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), N.full(n, 2.)))
    d = N.vstack((rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), -N.ones(n)))
    if normal:
        d[:2] = 0.
    d /= N.sqrt(N.sum(d ** 2, axis=0))
    return v, d, N.ones(n) / n


def _trapz(y, x):
    return N.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2., axis=0)


class Case(object):
    def __init__(self, name, n=None):
        from tracer_amd.scene import compile_scene
        self.name = name
        self.kind, self.n, self.reps, self.how = CASES[name]
        if n is not None:
            self.n = n
        self.asm, self.map_surf = scene(self.kind)
        self.cs = compile_scene(self.asm)
        assert self.cs.splits
        self.frames = [N.array(s._temp_frame) for s in self.cs.surfaces]
        self.edges = {self.map_surf: MAP_EDGES}
        self.captured = [i for i in range(self.cs.n_surf) if self.cs.capture[i]]
        self.W = W_POLY if self.how == 'poly' else 0
        self.min_energy = MIN_ENERGY

    def source(self):
        from tracer_amd import sources
        return sources.rect_bundle(self.n, N.c_[[0., 0., 2.]], N.r_[0., 0., -1.], 2., 2., 0.3, flux=1., seed=SEED, ray_offset=1000)

    def columns(self):
        """what the given bundle of the case is made of: dict(v, d, e) and, by kind, wl + ref (material) or swl + spec (poly)"""
        v, d, e = rays(self.n, normal=self.how == 'normal')
        c = dict(v=v, d=d, e=e)
        if self.how == 'material':
            c['wl'] = N.random.RandomState(7).uniform(0.4e-6, 2.4e-6, self.n)
            c['ref'] = materials()[0].m(c['wl'])
        if self.how == 'poly':
            rng = N.random.RandomState(6)
            c['swl'] = N.sort(rng.uniform(0.3e-6, 2.5e-6, size=(self.W, self.n)), axis=0)
            spec = rng.uniform(0.5, 2., size=(self.W, self.n))
            c['spec'] = spec * (e / _trapz(spec, c['swl']))
            c['e'] = _trapz(c['spec'], c['swl'])
        return c

    def bundle(self):
        """what the device traces"""
        from tracer_amd.ray_bundle import RayBundle
        if self.how == 'source':
            return self.source()
        c = self.columns()
        kw = {}
        if self.how == 'material':
            kw = dict(ref_index=c['ref'], wavelengths=c['wl'])
        if self.how == 'poly':
            kw = dict(spectra=c['spec'].copy(), wavelengths=c['swl'].copy())
        return RayBundle(vertices=c['v'].copy(), directions=c['d'].copy(), energy=c['e'].copy(), **kw)

    @property
    def seed(self):
        return SEED


@functools.lru_cache(maxsize=None)
def case(name, n=None):
    return Case(name, n)


_REF = {}


def reference(name):
    """the oracle's trace of a case, computed once and shared (nobody changes it), with its hit list and the host histogram of the map"""
    if name not in _REF:
        from oracle import engine
        c = case(name)
        with N.errstate(all='ignore'):
            if c.how == 'source':
                o = engine.trace_from_compiled(c.cs, c.source().source_args(), c.reps, c.min_energy)
            else:
                k = c.columns()
                kw = {}
                if c.how == 'material':
                    kw = dict(ref_index=k['ref'], wavelengths=k['wl'])
                if c.how == 'poly':
                    kw = dict(wavelengths=k['swl'], spectra=k['spec'])
                o = engine.trace_bundle(c.cs, k['v'], k['d'], k['e'], c.reps, c.min_energy, SEED, **kw)
        o['hit_list'] = hit_list(o['levels'], c)
        o['maps'] = fs.host_maps(o['hit_list'], c.frames, c.edges)
        o['max_live'] = max(L['n_live'] for L in o['levels'])
        _REF[name] = o
    return _REF[name]


def hit_list(levels, c):
    """one entry per hit of a recorded trace whose hits may send two rays on: the rays of level k + 1 with one parent stand for one
    hit of that parent -- where they start, on `surf`; what the parent brought less what they take along was absorbed.  With
    spectra: the 3 W columns of a captured hit (sample wavelengths, the spectrum that arrived, the sum of the spectra that left)."""
    surf, e_in, e_abs, pts, dirs, x = [], [], [], [], [], []
    spec0 = c.columns().get('spec') if c.W else None
    for k, (prev, L) in enumerate(zip(levels[:-1], levels[1:])):
        par = N.asarray(L['parents'])
        if len(par) == 0:
            continue
        uniq, first, inv = N.unique(par, return_index=True, return_inverse=True)
        out = N.zeros(len(uniq))
        N.add.at(out, inv, N.asarray(L['energy']))
        assert N.bincount(inv).max() <= 2
        surf.append(N.asarray(L['surf'])[first])
        e_in.append(N.asarray(prev['energy'])[uniq])
        e_abs.append(e_in[-1] - out)
        pts.append(N.asarray(L['vertices'])[:, first])
        dirs.append(N.asarray(prev['directions'])[:, uniq])
        if c.W:
            left = N.zeros((c.W, len(uniq)))
            for w in range(c.W):
                N.add.at(left[w], inv, L['spectra'][w])
            arrived = (spec0 if k == 0 else prev['spectra'])[:, uniq]
            x.append(N.vstack((L['swl'][:, first], arrived, left)))
    H = dict(surf=N.concatenate(surf), e_in=N.concatenate(e_in), e_abs=N.concatenate(e_abs), points=N.hstack(pts), directions=N.hstack(dirs))
    if c.W:
        H['x'] = N.hstack(x)
    return H


def transfer_of_levels(levels, n_surf):
    """(n_surf + 1, n_surf): the energy carried by the segments that leave surface `row` (last row: the source) and land on surface
    `column`, from a recorded trace -- every hit once, whatever it sent on"""
    T = N.zeros((n_surf + 1, n_surf))
    left = N.full(len(levels[0]['energy']), n_surf)
    for prev, L in zip(levels[:-1], levels[1:]):
        par = N.asarray(L['parents'], dtype=int)
        if len(par) == 0:
            break
        uniq, first = N.unique(par, return_index=True)
        N.add.at(T, (left[uniq], N.asarray(L['surf'])[first]), N.asarray(prev['energy'])[uniq])
        left = N.asarray(L['surf'])
    return T
