"""
Source bundles.  Function names and arguments follow the reference's tracer/sources.py
(:88-117 direction samplers, :175-239 disk_bundle, :241-264 rect_bundle, :330-384 Buie sampling,
:412-464 buie_sunshape, :466-515 rect_buie_sunshape).

Everything that does not depend on the random draws -- the rotation_to_z frames, the per-ray
energy, the 210-interval Buie CDF table -- is evaluated here on the host once per call and packed
into a trc_source_desc; the rays themselves are sampled on the GPU (csrc/trc_core.h,
trc_source_ray), either materialised as a bundle (trc_source_generate) or fused into the trace
kernel.  The functions return a LazySourceBundle: a RayBundle whose columns appear on first access.
"""
import ctypes as C

import numpy as N

from . import _cabi, rng
from .ray_bundle import RayBundle, concatenate_rays
from .spatial_geometry import rotation_to_z


class LazySourceBundle(RayBundle):
    """
    A source bundle described by (descriptor, n, seed, ray_offset).  Ray i has random stream id
    ray_offset + i.  Any column access generates the rays on the device; an engine that receives an
    untouched LazySourceBundle generates them inside its own kernel instead.
    """
    def __init__(self, desc, n, seed, ray_offset=0, constant_columns=None, spectrum=None, spectral_columns=('wavelengths', 'ref_index'),
                 table=None):
        """spectrum: a source_spectrum.SourceSpectrum -- every ray gets a wavelength drawn on the device (the columns
        `spectral_columns` of the materialised bundle); the bundle stays pending.  A spectrum that is carried
        (SourceSpectrum.polychromatic) makes the bundle polychromatic instead: materialised, it has `wavelengths` and `spectra`
        of shape (W, n) and `ref_index`.  table: the SunshapeTable a tabulated
        sunshape's descriptor names (made on the device when the rays are first needed, kept alive with the bundle)."""
        if spectrum is not None and constant_columns:
            raise ValueError("a source bundle takes a spectrum or constant columns, not both")
        spectral_columns = tuple(spectral_columns) if spectrum is not None else ()
        if spectrum is not None and spectrum.is_carried():
            spectral_columns = ('wavelengths', 'spectra', 'ref_index')
        RayBundle.__init__(self, **dict((k, None) for k in tuple(constant_columns or {}) + spectral_columns))
        object.__setattr__(self, '_src_const', dict(constant_columns or {}))
        object.__setattr__(self, '_src_desc', desc)
        object.__setattr__(self, '_src_n', int(n))
        object.__setattr__(self, '_src_seed', int(seed))
        object.__setattr__(self, '_src_offset', int(ray_offset))
        object.__setattr__(self, '_src_spectrum', spectrum)
        object.__setattr__(self, '_src_spec_cols', spectral_columns)
        object.__setattr__(self, '_src_table', table)
        object.__setattr__(self, '_src_done', False)

    def is_pending(self):
        # bundles carrying extra per-ray constant columns are materialised before tracing (a spectrum travels with the descriptor)
        return not self._src_done and not self._src_const

    def source_spectrum(self):
        """the SourceSpectrum the rays' wavelengths are drawn from, or None"""
        return self._src_spectrum

    def spectral_columns(self):
        """the columns the spectrum fills when the bundle is materialised ('wavelengths', 'ref_index')"""
        return self._src_spec_cols

    def get_num_rays(self):
        if not self._src_done:
            return self._src_n
        return RayBundle.get_num_rays(self)

    def _bound_desc(self):
        if self._src_table is not None:
            self._src_desc.table = self._src_table.table_id()
        return self._src_desc

    def source_args(self):
        return self._bound_desc(), self._src_n, self._src_seed, self._src_offset

    def _materialize(self):
        if self._src_done:
            return
        object.__setattr__(self, '_src_done', True)
        n = self._src_n
        ctx = _cabi.get_context()
        # (page-locked for large bundles: 1e7 rays are 560 MB, 11 ms over the link instead of 40 through pageable memory)
        v = _cabi.pinned_empty((3, n))
        d = _cabi.pinned_empty((3, n))
        e = _cabi.pinned_empty(n)
        spec = self._src_spectrum
        carried = spec is not None and spec.is_carried()
        wl = _cabi.pinned_empty(n) if ('wavelengths' in self._src_spec_cols and not carried) else None
        ref = _cabi.pinned_empty(n) if 'ref_index' in self._src_spec_cols else None
        if carried:     # every ray carries the W points of the table: `wavelengths` and `spectra` are (W, n)
            W = spec.wavelengths.size
            wl = _cabi.pinned_empty((W, n))
            spectra = _cabi.pinned_empty((W, n))
            rays = _cabi.make_rays(n, v[0], v[1], v[2], d[0], d[1], d[2], e, ref_index=ref, spec_wl=wl, spectra=spectra)
        else:
            rays = _cabi.make_rays(n, v[0], v[1], v[2], d[0], d[1], d[2], e, ref_index=ref, wavelength=wl)
        _cabi.check(ctx.lib.trc_source_generate_x(ctx.handle, C.byref(self._bound_desc()),
                                                  C.byref(spec.desc()) if spec is not None else None, n, self._src_seed,
                                                  self._src_offset, C.byref(rays)))
        self._cols['vertices'] = v
        self._cols['directions'] = d
        self._cols['energy'] = e
        if wl is not None:
            self._cols['wavelengths'] = wl
        if ref is not None:
            self._cols['ref_index'] = ref
        if carried:
            self._cols['spectra'] = spectra
        for k, val in self._src_const.items():
            self._cols[k] = N.ones(n) * val


def _fill_source(kind, center, rot_pos, rot_dir, params, energy, buie=None):
    s = _cabi.SourceDesc()
    s.kind = kind

    def put(field, values):
        # block copy into the ctypes array (element-wise assignment of the 639-entry Buie table was most of the
        # cost of making a bundle)
        a = N.ascontiguousarray(N.ravel(N.asarray(values, dtype=float)))
        C.memmove(field, a.ctypes.data, a.nbytes)

    put(s.center, center)
    put(s.rot_pos, rot_pos)
    put(s.rot_dir, rot_dir)
    if len(params):
        put(s.p, [float(p) for p in params])
    s.energy = float(energy)
    if buie is not None:
        put(s.buie, buie)
    return s


def _new_bundle(desc, num_rays, seed, ray_offset, constant_columns=None, spectrum=None, spectral_columns=('wavelengths', 'ref_index'),
                table=None):
    if seed is None:
        seed = rng.next_seed()
    if spectrum is not None:
        from .source_spectrum import SourceSpectrum
        if not isinstance(spectrum, SourceSpectrum):
            raise TypeError("spectrum must be a SourceSpectrum, got %r" % (type(spectrum).__name__,))
    return LazySourceBundle(desc, int(num_rays), seed, ray_offset, constant_columns, spectrum, spectral_columns, table)


def _tilt_cos(rays_direction, direction):
    """cos of the angle between the bundle axis and the emitting plane normal (sources.py:235, :445)."""
    chord = N.sqrt(N.sum((N.asarray(rays_direction, dtype=float) - N.asarray(direction, dtype=float)) ** 2))
    return N.cos(2. * N.sin(chord / 2.))


def disk_bundle(num_rays, center, direction, radius, ang_range, flux=None, radius_in=0., angular_span=[0., 2. * N.pi],
                x_cut=None, procs=1, rays_direction=None, seed=None, ray_offset=0, spectrum=None):
    """
    Pillbox/Lambertian-cone rays leaving an annular disc.  center: 3x1 column, direction: 3-vector
    normal of the disc; energies flux*area/N*cos(tilt), or 1/N/procs without flux.  x_cut keeps the part of the disc
    with local x < x_cut (positions are redrawn until they qualify; the energy still refers to the whole disc, as in
    the reference).
    """
    radius, radius_in = float(radius), float(radius_in)
    if x_cut is not None and not x_cut > -radius:
        raise ValueError("disk_bundle: x_cut leaves no part of the disc")
    if rays_direction is None:
        rays_direction = direction
    if flux is not None:
        energy = N.pi * (radius ** 2. - radius_in ** 2.) / num_rays * flux * _tilt_cos(rays_direction, direction)
    else:
        energy = 1. / float(num_rays) / procs
    rot = rotation_to_z(rays_direction)
    desc = _fill_source(_cabi.SRC_PILLBOX_DISK, center, rot, rot,
                        [radius, radius_in, angular_span[0], angular_span[1], ang_range,
                         0. if x_cut is None else 1., 0. if x_cut is None else float(x_cut)], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def rect_bundle(num_rays, center, direction, x, y, ang_range, flux=None, procs=1, seed=None, ray_offset=0, spectrum=None):
    """Pillbox rays leaving an x by y rectangle normal to `direction` (sources.py:241-264)."""
    direction = N.asarray(direction)
    swap = bool((direction == N.array([0, 0, -1])).all())
    energy = x * y / num_rays * flux if flux is not None else 1. / float(num_rays) / procs
    rot = rotation_to_z(direction)
    desc = _fill_source(_cabi.SRC_PILLBOX_RECT, center, rot, rot, [x, y, ang_range, 1. if swap else 0.], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def oblique_solar_rect_bundle(num_rays, center, source_direction, rays_direction, x, y, ang_range, flux=None, procs=1,
                              wavelength=None, ref_index=None, seed=None, ray_offset=0, spectrum=None):
    """Pillbox rays about `rays_direction` leaving an x by y rectangle normal to `source_direction`
    (sources.py:268-302); optional constant wavelength / ref_index columns."""
    source_direction = N.asarray(source_direction, dtype=float)
    rays_direction = N.asarray(rays_direction, dtype=float)
    swap = bool((source_direction == N.array([0, 0, -1])).all())
    if flux is not None:
        cosangle = 2. * N.arcsin(0.5 * N.sqrt(N.sum((rays_direction - source_direction) ** 2)))
        energy = x * y / num_rays * flux * N.cos(cosangle)
    else:
        energy = 1. / float(num_rays) / procs
    desc = _fill_source(_cabi.SRC_PILLBOX_RECT, center, rotation_to_z(source_direction), rotation_to_z(rays_direction),
                        [x, y, ang_range, 1. if swap else 0.], energy)
    if wavelength is not None:
        # a monochromatic spectrum: the bundle stays pending, its materialised columns are the constants
        if spectrum is not None:
            raise ValueError("oblique_solar_rect_bundle: give a wavelength or a spectrum, not both")
        from .source_spectrum import SourceSpectrum
        spectrum = SourceSpectrum.monochromatic(wavelength, 1. if ref_index is None else ref_index)
        cols = ('wavelengths',) if ref_index is None else ('wavelengths', 'ref_index')
        return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum, spectral_columns=cols)
    if ref_index is not None:
        if spectrum is not None:
            raise ValueError("oblique_solar_rect_bundle: the spectrum carries the index of the rays' medium (ref_index=)")
        return _new_bundle(desc, num_rays, seed, ray_offset, {'ref_index': ref_index})
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def triangular_bundle(num_rays, A, B, C, direction=None, ang_range=N.pi / 2., flux=None, procs=1, seed=None, ray_offset=0, spectrum=None):
    """Pillbox rays leaving the triangle ABC (uniform point picking), about `direction` (default: the triangle
    normal AB x AC) -- sources.py:544-597."""
    A, B, C = [N.ravel(N.asarray(q, dtype=float)) for q in (A, B, C)]
    AB, AC = B - A, C - A
    normal = N.cross(AB, AC)
    normal = normal / N.sqrt(N.sum(normal ** 2))
    if direction is None:
        direction = normal
    direction = N.ravel(N.asarray(direction, dtype=float))
    l1, l2, l3 = N.sqrt(N.sum(AB ** 2)), N.sqrt(N.sum(AC ** 2)), N.sqrt(N.sum((-AB + AC) ** 2))
    sp = (l1 + l2 + l3) / 2.
    area = N.sqrt(sp * (sp - l1) * (sp - l2) * (sp - l3))
    if flux is not None:
        cosangle = 2. * N.arcsin(0.5 * N.sqrt(N.sum((direction - normal) ** 2)))
        energy = area / num_rays * flux * N.cos(cosangle)
    else:
        energy = 1. / float(num_rays) / procs
    rot_pos = N.zeros((3, 3))
    rot_pos[:, 0] = AB
    rot_pos[:, 1] = AC
    desc = _fill_source(_cabi.SRC_PILLBOX_TRIANGLE, A, rot_pos, rotation_to_z(direction), [ang_range], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def vf_cylinder_bundle(num_rays, rc, lc, center, direction, flux=None, rays_in=True, angular_span=[0., 2. * N.pi],
                       ang_range=N.pi / 2., seed=None, ray_offset=0, spectrum=None):
    """
    Lambertian emitter on the wall of a cylinder of radius rc and length lc centred on `center` with its axis along
    `direction`, firing towards the axis (rays_in) or away from it (sources.py:716-769; the view-factor workload of
    emissive_losses).  Energies flux*area/N, or 1/N without flux.
    """
    rc, lc = float(rc), float(lc)
    if flux is None:
        energy = 1. / float(num_rays)
    else:
        energy = flux * rc * (angular_span[1] - angular_span[0]) * lc / float(num_rays)
    rot = rotation_to_z(direction)
    desc = _fill_source(_cabi.SRC_VF_CYLINDER, center, rot, rot,
                        [rc, lc, angular_span[0], angular_span[1], ang_range, 1. if rays_in else -1.], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def vf_frustum_bundle(num_rays, r0, r1, depth, center, direction, flux=None, rays_in=True, angular_span=[0., 2. * N.pi],
                      angular_range=N.pi / 2., seed=None, ray_offset=0, spectrum=None):
    """
    Lambertian emitter on the wall of a frustum: radius r0 at the base centred on `center`, r1 at `depth` along
    `direction` (sources.py:644-714).  r0 == r1 is a cylinder and must use vf_cylinder_bundle (the reference divides
    by the wall slope).
    """
    r0, r1, depth = float(r0), float(r1), float(depth)
    if r0 == r1:
        raise ValueError("vf_frustum_bundle needs r0 != r1; use vf_cylinder_bundle for a cylinder")
    if flux is None:
        energy = 1. / float(num_rays)
    else:
        area = (angular_span[1] - angular_span[0]) * (r1 + r0) / 2. * N.sqrt(abs(r1 - r0) ** 2. + depth ** 2.)
        energy = flux * area / float(num_rays)
    rot = rotation_to_z(direction)
    desc = _fill_source(_cabi.SRC_VF_FRUSTUM, center, rot, rot,
                        [r0, r1, depth, angular_span[0], angular_span[1], angular_range, 1. if rays_in else -1.], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def Lambertian_directions(num_rays, ang_range, normals=None):
    """
    (3, num_rays) unit directions about +z (or about `normals`), cosine-weighted within ang_range of it
    (sources.py:88-101).  A host sampler on numpy's global generator, drawing what the reference draws in its order -- the
    bundles above sample on the device from Philox streams instead.
    """
    xi1 = N.random.uniform(low=0., high=2. * N.pi, size=num_rays)
    if ang_range == 0.:
        dirs = N.zeros((3, num_rays))
        dirs[2] = 1.
    else:
        xi2 = N.random.uniform(size=num_rays)
        sinsqrt = N.sin(ang_range) * N.sqrt(xi2)
        dirs = N.vstack((N.cos(xi1) * sinsqrt, N.sin(xi1) * sinsqrt, N.sqrt(1. - sinsqrt ** 2.)))
    if normals is not None:
        from .vector_manipulations import rotate_z_to_normal
        dirs = rotate_z_to_normal(dirs, normals)
    return dirs


def pillbox_sunshape_directions(num_rays, ang_range):
    """pillbox sunshape about +z: the cone-limited Lambertian distribution (sources.py:103-117)"""
    return Lambertian_directions(num_rays, ang_range)


def edge_rays_directions(num_rays, ang_range):
    """directions on the rim of the cone of half-angle ang_range about +z (sources.py:152-173)"""
    xi1 = N.random.uniform(high=2. * N.pi, size=num_rays)
    sin_th = N.ones(num_rays) * N.sin(ang_range)
    return N.vstack((N.cos(xi1) * sin_th, N.sin(xi1) * sin_th, N.cos(N.ones(num_rays) * ang_range)))


def edge_rays_bundle(num_rays, center, direction, radius, ang_range, flux=None, radius_in=0.):
    """annular disc source whose rays all leave at exactly ang_range from `direction` (sources.py:304-328); host-generated"""
    radius, radius_in = float(radius), float(radius_in)
    a = edge_rays_directions(num_rays, ang_range)
    perp_rot = rotation_to_z(direction)
    directions = N.sum(perp_rot[..., None] * a[None, ...], axis=1)
    xi1 = N.random.uniform(size=num_rays)
    thetas = N.random.uniform(high=2. * N.pi, size=num_rays)
    rs = N.sqrt(radius_in ** 2. + xi1 * (radius ** 2. - radius_in ** 2.))
    vertices_local = N.vstack((rs * N.cos(thetas), rs * N.sin(thetas), N.zeros(num_rays)))
    rayb = RayBundle(vertices=N.dot(perp_rot, vertices_local) + center, directions=directions)
    if flux is not None:
        rayb.set_energy(N.pi * (radius ** 2. - radius_in ** 2.) / num_rays * flux * N.ones(num_rays))
    return rayb


def trapezoid_bundle(num_rays, A, B, C, direction=None, ang_range=N.pi / 2., flux=None, procs=1, seed=None, ray_offset=0, spectrum=None):
    """
    Isosceles trapezoid ABCD (AB the first base, C the third vertex, D by symmetry) as two triangular bundles sharing the
    rays in proportion to their areas (sources.py:599-642).
    """
    A, B, C = [N.asarray(v, dtype=float) for v in (A, B, C)]
    AB, AC = B - A, C - A
    l1, l2 = N.sqrt(N.sum(AB ** 2)), N.sqrt(N.sum(AC ** 2))
    cos_theta = N.dot(AC, AB) / (l1 * l2)
    cB = AB * (1. - 1. / l1 * l2 * cos_theta)
    AD = AC - (AB - 2. * cB)
    D = A + AD
    l3, l4, l5 = N.sqrt(N.sum(AD ** 2)), N.sqrt(N.sum((AC - AB) ** 2)), N.sqrt(N.sum((AD - AC) ** 2))
    s1, s2 = (l1 + l2 + l4) / 2., (l2 + l3 + l5) / 2.
    area_ABC = N.sqrt(s1 * (s1 - l1) * (s1 - l2) * (s1 - l4))      # Heron
    area_ACD = N.sqrt(s2 * (s2 - l2) * (s2 - l3) * (s2 - l5))
    n_ABC = int(area_ABC / (area_ABC + area_ACD) * num_rays)
    first = triangular_bundle(n_ABC, A, B, C, direction, ang_range, flux, seed=seed, ray_offset=ray_offset, spectrum=spectrum)
    second = triangular_bundle(num_rays - n_ABC, A, C, D, direction, ang_range, flux, seed=seed, ray_offset=ray_offset + n_ABC,
                               spectrum=spectrum)
    rayb = concatenate_rays([first, second])
    if flux is None:
        rayb.set_energy(N.ones(num_rays) / float(num_rays) / procs)
    return rayb


def regular_square_bundle(num_rays, center, direction, width):
    """Parallel rays on a regular square grid of half-width `width` normal to `direction` (sources.py:518-542);
    deterministic, no energy column -- built on the host."""
    direction = N.asarray(direction, dtype=float)
    rot = rotation_to_z(direction)
    rng_ = N.s_[-width:width:float(2 * width) / N.sqrt(num_rays)]
    xs, ys = N.mgrid[rng_, rng_]
    local = N.array([xs.flatten(), ys.flatten(), N.zeros(len(xs.flatten()))])
    rayb = RayBundle()
    rayb.set_vertices(N.dot(rot, local) + center)
    rayb.set_directions(N.tile(direction[:, None], (1, local.shape[1])))
    return rayb


def solar_disk_bundle(num_rays, center, direction, radius, ang_range, flux=None, radius_in=0., angular_span=[0., 2. * N.pi],
                      procs=1, seed=None, ray_offset=0, spectrum=None):
    """Older name of disk_bundle still used by scene scripts."""
    return disk_bundle(num_rays, center, direction, radius, ang_range, flux, radius_in, angular_span, None, procs,
                       None, seed, ray_offset, spectrum)


_buie_tables = {}


def buie_table(CSR, pre_process_CSR=True):
    """the table of _buie_table, computed once per (CSR, pre_process_CSR): Monte-Carlo loops make one bundle per batch"""
    key = (float(CSR), bool(pre_process_CSR))
    if key not in _buie_tables:
        if len(_buie_tables) > 64:
            _buie_tables.clear()
        _buie_tables[key] = _buie_table(*key)
    return _buie_tables[key]


def _buie_table(CSR, pre_process_CSR=True):
    """
    The Buie sunshape sampling table of the reference (sources.py:333-361): 211 polar angles up to
    4.65 mrad, g = phi*cos*sin with phi = cos(0.326 theta)/cos(0.308 theta) (theta in mrad), the
    trapezoid CDF of the disc part, and the aureole constants kappa, gamma for CSR > 0.
    Layout: trc_source_desc.buie.
    """
    theta_dni = 4.65e-3
    theta_tot = 43.6e-3
    nelem = _cabi.TRC_BUIE_NELEM
    theta = N.linspace(0., theta_dni, nelem + 1)
    phi = N.cos(0.326 * theta * 1e3) / N.cos(0.308 * theta * 1e3)
    g = phi * N.cos(theta) * N.sin(theta)
    integ = 0.5 * (phi[:-1] * N.cos(theta[:-1]) * N.sin(theta[:-1]) + phi[1:] * N.cos(theta[1:]) * N.sin(theta[1:])) * \
        (theta[1:] - theta[:-1])
    I_dni = N.sum(integ)
    gamma = kappa = 0.
    if CSR == 0.:
        total = I_dni
    else:
        if pre_process_CSR:
            if CSR <= 0.1:
                CSR = -2.245e+03 * CSR ** 4. + 5.207e+02 * CSR ** 3. - 3.939e+01 * CSR ** 2. + 1.891e+00 * CSR + 8e-03
            else:
                CSR = 1.973 * CSR ** 4. - 2.481 * CSR ** 3. + 0.607 * CSR ** 2. + 1.151 * CSR - 0.020
        kappa = 0.9 * N.log(13.5 * CSR) * CSR ** (-0.3)
        gamma = 2.2 * N.log(0.52 * CSR) * CSR ** (0.43) - 0.1
        I_csr = 1e-6 * N.exp(kappa) / (gamma + 2.) * ((theta_tot * 1000.) ** (gamma + 2.) - (theta_dni * 1000.) ** (gamma + 2.))
        total = I_dni + I_csr
    cdf = N.add.accumulate(N.hstack(([0], integ / total)))
    return N.concatenate((theta, g, cdf, [I_dni, gamma, kappa, theta_dni, theta_tot, 1. if CSR > 0. else 0.]))


def buie_sunshape(num_rays, center, direction, radius, CSR, flux=None, pre_process_CSR=True, rays_direction=None,
                  seed=None, ray_offset=0, spectrum=None):
    """
    Disc source with the Buie sunshape (sources.py:412-464): start points uniform on a disc of
    `radius` normal to `direction`, directions about `rays_direction` (default `direction`).
    """
    direction = N.asarray(direction, dtype=float)
    if rays_direction is None:
        rays_direction = direction
    energy = flux * (N.pi * radius ** 2.) / num_rays * _tilt_cos(rays_direction, direction)
    desc = _fill_source(_cabi.SRC_BUIE_DISK, center, rotation_to_z(direction), rotation_to_z(rays_direction),
                        [radius], energy, buie_table(CSR, pre_process_CSR))
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def rect_buie_sunshape(num_rays, center, direction, width, height, CSR, flux=None, pre_process_CSR=True,
                       rays_direction=None, seed=None, ray_offset=0, spectrum=None):
    """Rectangular source with the Buie sunshape (sources.py:466-515)."""
    direction = N.asarray(direction, dtype=float)
    if rays_direction is None:
        rays_direction = direction
    energy = flux * (width * height) / num_rays * _tilt_cos(rays_direction, direction)
    desc = _fill_source(_cabi.SRC_BUIE_RECT, center, rotation_to_z(direction), rotation_to_z(rays_direction),
                        [width, height], energy, buie_table(CSR, pre_process_CSR))
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def sunshape_to_ray_directions(angles, norm_intensity, num_rays):
    """
    Directions about +z drawn from a tabulated sunshape on the host (sources.py:386-410), with numpy's global generator and
    in the reference's order (all polar uniforms, then all azimuths), so that under the same numpy.random.seed it returns the
    reference's (3, num_rays) array.  The polar angle has the density that interpolates g = I cos(theta) sin(theta) linearly
    between the points.  As in the reference, draws at or beyond the last entry of its CDF (which can round below 1) keep
    theta = 0; the device sources (tabulated_sunshape) use a CDF that ends at exactly 1.
    """
    angles = N.asarray(angles, dtype=float)
    norm_intensity = N.asarray(norm_intensity, dtype=float)
    num_rays = int(num_rays)
    thetas = N.zeros(num_rays)
    R_thetas = N.random.uniform(size=num_rays)
    g = norm_intensity * N.cos(angles) * N.sin(angles)
    integ = 0.5 * (g[:-1] + g[1:]) * (angles[1:] - angles[:-1])
    total = N.sum(integ)
    CDF = N.add.accumulate(N.hstack(([0.], integ / total)))
    for i in range(len(CDF) - 1):
        sl = N.logical_and(R_thetas >= CDF[i], R_thetas < CDF[i + 1])
        if not N.any(sl):
            continue
        A, B = g[i], g[i + 1]
        if A == B:
            thetas[sl] = angles[i] + total * (R_thetas[sl] - CDF[i]) / A
        else:
            Cq = 2. * total * (R_thetas[sl] - CDF[i]) * (angles[i + 1] - angles[i])
            thetas[sl] = -(-A * angles[i + 1] + B * angles[i] + N.sqrt(((angles[i] - angles[i + 1]) * A) ** 2. + Cq * (B - A))) / (A - B)
    phis = N.random.uniform(high=2. * N.pi, size=num_rays)
    sin_th = N.sin(thetas)
    return N.vstack((N.cos(phis) * sin_th, N.sin(phis) * sin_th, N.cos(thetas)))


def check_sunshape_table(angles, norm_intensity):
    """The table of a tabulated sunshape as two float64 arrays; ValueError unless it has 2..4096 points, finite angles
    strictly increasing in [0, pi/2), finite non-negative intensities and a positive mass (the checks of trc_sunshape_create)."""
    a = N.ascontiguousarray(N.ravel(N.asarray(angles, dtype=float)))
    I = N.ascontiguousarray(N.ravel(N.asarray(norm_intensity, dtype=float)))
    if a.shape != I.shape:
        raise ValueError("sunshape table: %d angles but %d intensities" % (a.size, I.size))
    if not 2 <= a.size <= _cabi.SUNSHAPE_MAX_POINTS:
        raise ValueError("sunshape table: 2..%d points, got %d" % (_cabi.SUNSHAPE_MAX_POINTS, a.size))
    if not N.all(N.isfinite(a)) or not N.all(a[1:] > a[:-1]):
        raise ValueError("sunshape table: the angles must be finite and strictly increasing")
    if not (a[0] >= 0. and a[-1] < N.pi / 2.):
        raise ValueError("sunshape table: the angles must lie in [0, pi/2)")
    if not N.all(N.isfinite(I)) or N.any(I < 0.):
        raise ValueError("sunshape table: the intensities must be finite and non-negative")
    g = I * N.cos(a) * N.sin(a)
    mass = N.sum(0.5 * (g[:-1] + g[1:]) * (a[1:] - a[:-1]))
    if not (mass > 0. and N.isfinite(mass)):
        raise ValueError("sunshape table: the table has no mass")
    return a, I


class SunshapeTable(object):
    """
    A checked tabulated sunshape.  Its packed table (include/tracer_amd.h, trc_sunshape) is made on the device on first use
    and freed with the object; sunshape_table() hands out one object per content, so that a Monte-Carlo loop that makes a bundle
    per batch uploads the table once.
    """
    def __init__(self, angles, norm_intensity):
        self.angles, self.intensity = check_sunshape_table(angles, norm_intensity)
        self._handle = None
        self._lib = None
        self._id = 0

    def _create(self, ctx, handle):
        return ctx.lib.trc_sunshape_create(ctx.handle, self.angles.size, _cabi.ptr(self.angles), _cabi.ptr(self.intensity),
                                           C.byref(handle))

    def table_id(self):
        """the id a descriptor names the device table by (trc_sunshape_create on the current device on first call)"""
        if self._handle is None:
            ctx = _cabi.get_context()
            h = C.c_void_p()
            _cabi.check(self._create(ctx, h))
            i = C.c_int32()
            _cabi.check(ctx.lib.trc_sunshape_id(h, C.byref(i)))
            self._handle, self._lib, self._id = h, ctx.lib, int(i.value)
        return self._id

    def packed(self):
        """(theta, g, cdf, theta_c, u_c) of the device table, as the library packed them"""
        self.table_id()
        n = self.angles.size
        tab = N.empty(3 * n)
        tc, uc = C.c_double(), C.c_double()
        _cabi.check(self._lib.trc_sunshape_get(self._handle, None, _cabi.ptr(tab), C.byref(tc), C.byref(uc)))
        return tab[:n], tab[n:2 * n], tab[2 * n:], tc.value, uc.value

    def destroy(self):
        if self._handle is not None:
            h, lib = self._handle, self._lib
            self._handle = self._lib = None
            lib.trc_sunshape_destroy(h)

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


_sunshape_tables = {}


def sunshape_table(angles, norm_intensity):
    """the SunshapeTable of this content (cached like buie_table)"""
    a, I = check_sunshape_table(angles, norm_intensity)
    key = (a.tobytes(), I.tobytes())
    t = _sunshape_tables.get(key)
    if t is None:
        if len(_sunshape_tables) > 64:
            _sunshape_tables.clear()        # (bundles still hold theirs)
        t = _sunshape_tables[key] = SunshapeTable(a, I)
    return t


def tabulated_sunshape(num_rays, center, direction, radius, angles, norm_intensity, flux=None, rays_direction=None, seed=None,
                       ray_offset=0, spectrum=None):
    """
    Disc source with a tabulated sunshape (sources.py:386-410): start points and energies as buie_sunshape, polar angles drawn
    on the device from the table (angles in rad, intensities per unit solid angle), azimuths uniform.  Draws of ray i (event 0,
    block 0): u0, u1 the position, u2 the polar angle, u3 the azimuth -- the Buie source's, so that the Buie CSR-0 nodes as a
    table give buie_sunshape(CSR=0)'s rays.
    """
    table = sunshape_table(angles, norm_intensity)
    direction = N.asarray(direction, dtype=float)
    if rays_direction is None:
        rays_direction = direction
    energy = flux * (N.pi * radius ** 2.) / num_rays * _tilt_cos(rays_direction, direction)
    desc = _fill_source(_cabi.SRC_SUNSHAPE_DISK, center, rotation_to_z(direction), rotation_to_z(rays_direction), [radius], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum, table=table)


def rect_tabulated_sunshape(num_rays, center, direction, width, height, angles, norm_intensity, flux=None, rays_direction=None,
                            seed=None, ray_offset=0, spectrum=None):
    """Rectangular source with a tabulated sunshape: start points and energies as rect_buie_sunshape (sources.py:466-515)."""
    table = sunshape_table(angles, norm_intensity)
    direction = N.asarray(direction, dtype=float)
    if rays_direction is None:
        rays_direction = direction
    energy = flux * (width * height) / num_rays * _tilt_cos(rays_direction, direction)
    desc = _fill_source(_cabi.SRC_SUNSHAPE_RECT, center, rotation_to_z(direction), rotation_to_z(rays_direction),
                        [width, height], energy)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum, table=table)


# -- arc-lamp sources (models/solar_simulator.py): rays from a volume, or from a curved surface about its local normal ------------
from .sampling import isotropic_directions_sampling     # noqa: E402,F401  (the reference's model imports it from here)

_EMIT_LAWS = {'lambertian': _cabi.EMIT_LAMBERTIAN, 'isotropic': _cabi.EMIT_ISOTROPIC}


def check_angle_table(thetas, density):
    """The polar table of an arc lamp as two float64 arrays; ValueError unless it has 2..4096 points, finite angles strictly
    increasing within [0, pi], finite non-negative densities and a positive integral (the checks of trc_angle_table_create)."""
    a = N.ascontiguousarray(N.ravel(N.asarray(thetas, dtype=float)))
    d = N.ascontiguousarray(N.ravel(N.asarray(density, dtype=float)))
    if a.shape != d.shape:
        raise ValueError("angle table: %d angles but %d densities" % (a.size, d.size))
    if not 2 <= a.size <= _cabi.SUNSHAPE_MAX_POINTS:
        raise ValueError("angle table: 2..%d points, got %d" % (_cabi.SUNSHAPE_MAX_POINTS, a.size))
    if not N.all(N.isfinite(a)) or not N.all(a[1:] > a[:-1]):
        raise ValueError("angle table: the angles must be finite and strictly increasing")
    if not (a[0] >= 0. and a[-1] <= N.pi):
        raise ValueError("angle table: the angles must lie in [0, pi]")
    if not N.all(N.isfinite(d)) or N.any(d < 0.):
        raise ValueError("angle table: the densities must be finite and non-negative")
    mass = N.sum((a[1:] - a[:-1]) * (d[1:] + d[:-1]) / 2.)
    if not (mass > 0. and N.isfinite(mass)):
        raise ValueError("angle table: the table has no mass")
    return a, d


class AngleTable(SunshapeTable):
    """A checked polar table of an arc lamp: the density of the polar angle over [0, pi], taken as given.  On the device it is a
    table like a sunshape's (trc_angle_table_create: the same object, the same ids), packed as a source spectrum's."""
    def __init__(self, thetas, density):
        self.angles, self.intensity = check_angle_table(thetas, density)
        self._handle = None
        self._lib = None
        self._id = 0

    def _create(self, ctx, handle):
        return ctx.lib.trc_angle_table_create(ctx.handle, self.angles.size, _cabi.ptr(self.angles), _cabi.ptr(self.intensity),
                                              C.byref(handle))


_angle_tables = {}


def angle_table(thetas, density):
    """the AngleTable of this content (cached like sunshape_table)"""
    a, d = check_angle_table(thetas, density)
    key = (a.tobytes(), d.tobytes())
    t = _angle_tables.get(key)
    if t is None:
        if len(_angle_tables) > 64:
            _angle_tables.clear()
        t = _angle_tables[key] = AngleTable(a, d)
    return t


def _lamp_frame(direction, rotation):
    """the rotation a lamp source is posed by: `rotation` (3, 3) as given, else the minimal rotation that takes +z to `direction`
    (vector_manipulations.rotate_z_to_normal, as the lamps of the model pose their rays)"""
    if rotation is not None:
        rot = N.asarray(rotation, dtype=float)
        if rot.shape != (3, 3):
            raise ValueError("rotation must be a 3 x 3 matrix")
        return rot
    from .vector_manipulations import rotate_z_to_normal
    d = N.ravel(N.asarray(direction, dtype=float))
    return rotate_z_to_normal(N.eye(3), d / N.sqrt(N.sum(d ** 2)))


def _lamp_checks(what, num_rays, power, **lengths):
    if int(num_rays) < 0:
        raise ValueError("%s: num_rays must not be negative" % what)
    for name, val in lengths.items():
        if not (N.isfinite(val) and val > 0.):
            raise ValueError("%s: %s must be positive and finite, got %r" % (what, name, val))
    if not N.isfinite(power):
        raise ValueError("%s: power must be finite" % what)


def arc_volume_bundle(num_rays, r_c, l_c, thetas, density, center, direction, power, seed=None, ray_offset=0, spectrum=None,
                      rotation=None):
    """
    The arc of a lamp as a cylinder volume of radius r_c and length l_c about `direction`, centred on `center` (a 3x1 column): start
    points uniform in the volume, polar angles about `direction` drawn on the device from the tabulated density (thetas within
    [0, pi], density of the polar angle itself, linear between the points), azimuths uniform.  Each ray carries power / num_rays.
    What SimulatorLampBader.generate_rays samples on the host (solar_simulator.py:237-258), drawn per ray from its Philox stream:
    event 0, block 0 for the height, the azimuth and the radius of the point and for the polar angle; the first uniform of block 1
    for the azimuth of the direction.  rotation: the (3, 3) pose in place of the minimal rotation of +z to `direction`.
    """
    r_c, l_c = float(r_c), float(l_c)
    _lamp_checks('arc_volume_bundle', num_rays, power, r_c=r_c, l_c=l_c)
    table = angle_table(thetas, density)
    rot = _lamp_frame(direction, rotation)
    desc = _fill_source(_cabi.SRC_ARC_VOLUME, center, rot, rot, [r_c, l_c], float(power) / max(int(num_rays), 1))
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum, table=table)


def _emitter_params(what, ang_range, law, rays_in):
    if law not in _EMIT_LAWS:
        raise ValueError("%s: law must be 'lambertian' or 'isotropic', got %r" % (what, law))
    ang_range = float(ang_range)
    if not 0. <= ang_range <= N.pi / 2.:
        raise ValueError("%s: ang_range must lie in [0, pi/2]" % what)
    return [ang_range, float(_EMIT_LAWS[law]), -1. if rays_in else 1.]


def sphere_emitter_bundle(num_rays, radius, center, direction, power, ang_range=N.pi / 2., law='lambertian', rays_in=False, seed=None,
                          ray_offset=0, spectrum=None, rotation=None):
    """
    Rays leaving a sphere of `radius` centred on `center`, uniformly over its surface (sampling.sphere_sampling), each within
    ang_range of the local normal -- outwards, or inwards with rays_in -- by the Lambertian law or uniformly in solid angle
    (law='isotropic': isotropic_directions_sampling), turned from +z to the normal by the minimal rotation.  Each ray carries
    power / num_rays.  Draws of a ray: event 0, block 0 -- azimuth and cosine of the point, azimuth and polar uniform of the direction.
    """
    radius = float(radius)
    _lamp_checks('sphere_emitter_bundle', num_rays, power, radius=radius)
    rot = _lamp_frame(direction, rotation)
    desc = _fill_source(_cabi.SRC_EMIT_SPHERE, center, rot, rot, [radius] + _emitter_params('sphere_emitter_bundle', ang_range, law, rays_in),
                        float(power) / max(int(num_rays), 1))
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


def cylinder_emitter_bundle(num_rays, radius, height, center, direction, power, ang_range=N.pi / 2., law='lambertian', rays_in=False,
                            seed=None, ray_offset=0, spectrum=None, rotation=None):
    """
    Rays leaving the wall of a cylinder of `radius` and `height` about `direction`, centred on `center`, uniformly over the wall
    (sampling.cylinder_sampling), each about the local normal as sphere_emitter_bundle's.  Draws of a ray: event 0, block 0 --
    height and azimuth of the point, azimuth and polar uniform of the direction.
    """
    radius, height = float(radius), float(height)
    _lamp_checks('cylinder_emitter_bundle', num_rays, power, radius=radius, height=height)
    rot = _lamp_frame(direction, rotation)
    desc = _fill_source(_cabi.SRC_EMIT_CYLINDER, center, rot, rot,
                        [radius, height] + _emitter_params('cylinder_emitter_bundle', ang_range, law, rays_in), float(power) / max(int(num_rays), 1))
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum)


# -- thermal emitters: rays from a surface with a tabulated directional band emittance --------------------------------------------
def _trapezoid(y, x):
    return N.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.)


def _emittance_G(a, e0, x0, th):
    """the integral of (e0 + a (t - x0)) cos(t) sin(t) over [x0, th], written in d = th - x0 so that no two large terms cancel
    (trc_emittance_G, csrc/trc_core.h: the same expression)"""
    d = th - x0
    s0, c0, s, c = N.sin(x0), N.cos(x0), N.sin(th), N.cos(th)
    x = 2. * d
    x2 = x * x
    small = d < 0.0625
    w = N.where(small, 0.5 * x * x2 * (-1. / 6. + x2 * (1. / 120. + x2 * (-1. / 5040. + x2 * (1. / 362880. - x2 * (1. / 39916800.))))),
                N.sin(d) * N.cos(d) - d)                                      # sin(d) cos(d) - d
    sd = N.where(small, d * (1. + d * d * (-1. / 6. + d * d * (1. / 120. + d * d * (-1. / 5040. + d * d * (1. / 362880.))))), s * c0 - c * s0)
    return e0 / 2. * sd * (s * c0 + c * s0) + a / 4. * ((c - s) * (c + s) * w + sd * sd * (2. * s * c))


def check_emittance_table(thetas, emittance):
    """The emittance table of a thermal emitter as two float64 arrays; ValueError unless it has 2..4096 points, finite angles strictly
    increasing within [0, pi/2], finite non-negative emittances and a positive mass (the checks of trc_emittance_table_create).  A
    last angle up to 5e-9 beyond pi/2 -- pi/2 as a table of 8 decimals states it -- is returned as pi/2, as the library reads it."""
    a = N.ascontiguousarray(N.ravel(N.asarray(thetas, dtype=float)))
    e = N.ascontiguousarray(N.ravel(N.asarray(emittance, dtype=float)))
    if a.shape != e.shape:
        raise ValueError("emittance table: %d angles but %d emittances" % (a.size, e.size))
    if not 2 <= a.size <= _cabi.SUNSHAPE_MAX_POINTS:
        raise ValueError("emittance table: 2..%d points, got %d" % (_cabi.SUNSHAPE_MAX_POINTS, a.size))
    if not N.all(N.isfinite(a)):
        raise ValueError("emittance table: the angles must be finite and strictly increasing")
    if not (a[0] >= 0. and a[-1] <= _cabi.EMITTANCE_THETA_MAX):
        raise ValueError("emittance table: the angles must lie in [0, pi/2]")
    a = N.minimum(a, N.pi / 2.)
    if not N.all(a[1:] > a[:-1]):
        raise ValueError("emittance table: the angles must be finite and strictly increasing")
    if not N.all(N.isfinite(e)) or N.any(e < 0.):
        raise ValueError("emittance table: the emittances must be finite and non-negative")
    mass = _emittance_mass(a, e)
    if not (mass > 0. and N.isfinite(mass)):
        raise ValueError("emittance table: the table has no mass")
    return a, e


def _emittance_mass(a, e):
    """the integral of eps(theta) cos(theta) sin(theta) over the table, eps linear between the points: every interval with its own
    slope at both its ends (trc_emittance_pack's M)"""
    slope = (e[1:] - e[:-1]) / (a[1:] - a[:-1])
    return N.sum(N.maximum(_emittance_G(slope, e[:-1], a[:-1], a[1:]), 0.))


class EmittanceTable(SunshapeTable):
    """A checked emittance table of a thermal emitter: the directional band emittance over [0, pi/2], linear between the points.  On
    the device it is a table like a sunshape's (trc_emittance_table_create: the same object, the same ids), packed as theta | eps / M
    | cdf with the analytic integrals of eps cos sin."""
    def __init__(self, thetas, emittance):
        self.angles, self.intensity = check_emittance_table(thetas, emittance)
        self.mass = float(_emittance_mass(self.angles, self.intensity))
        self._handle = None
        self._lib = None
        self._id = 0

    def _create(self, ctx, handle):
        return ctx.lib.trc_emittance_table_create(ctx.handle, self.angles.size, _cabi.ptr(self.angles), _cabi.ptr(self.intensity),
                                                  C.byref(handle))


_emittance_tables = {}


def emittance_table(thetas, emittance):
    """the EmittanceTable of this content (cached like angle_table)"""
    a, e = check_emittance_table(thetas, emittance)
    key = (a.tobytes(), e.tobytes())
    t = _emittance_tables.get(key)
    if t is None:
        if len(_emittance_tables) > 64:
            _emittance_tables.clear()
        t = _emittance_tables[key] = EmittanceTable(a, e)
    return t


def _shape_kwargs(what, kwargs, names, flip_name):
    """the shape's arguments by the reference samplers' names; (values, -1. if the flag that turns the normal is set else 1.)"""
    kwargs = dict(kwargs or {})
    flip = kwargs.pop(flip_name, flip_name == 'normal_up')
    for k in ('ns', 'normals'):
        kwargs.pop(k, None)
    if kwargs.pop('volume', False):
        raise ValueError("%s: a thermal emitter is a surface, not a volume" % what)
    missing = [k for k in names if k not in kwargs and k != 'angular_span']
    extra = [k for k in kwargs if k not in names]
    if missing or extra:
        raise ValueError("%s: the shape takes %s; missing %s, unknown %s" % (what, list(names), missing, extra))
    turned = (not flip) if flip_name == 'normal_up' else bool(flip)
    return kwargs, (-1. if turned else 1.)


def _thermal_shape(what, shape):
    """(p[0..5] of the descriptor, the area, the offset of the local origin) of gray_source's shape dictionary {'type': ..., 'kwargs':
    {...}} -- the kwargs by the names of the reference's ray_trace_utils.sampling.<type>_sampling -- and the sign its normal flag gives"""
    try:
        kind, kwargs = shape['type'], shape.get('kwargs', {})
    except (TypeError, KeyError):
        raise ValueError("%s: shape must be a dictionary {'type': ..., 'kwargs': {...}}" % what)
    origin = N.zeros(3)

    def positive(**lengths):
        for name, val in lengths.items():
            if not (N.isfinite(val) and val > 0.):
                raise ValueError("%s: %s must be positive and finite, got %r" % (what, name, val))

    if kind == 'disk':
        kw, sign = _shape_kwargs(what, kwargs, ('r_ext',), 'normal_up')
        R = float(kw['r_ext'])
        positive(r_ext=R)
        p, area = [_cabi.THERMAL_DISK, R, 0., 0., 0., 0.], N.pi * R ** 2.
    elif kind == 'rectangle':
        kw, sign = _shape_kwargs(what, kwargs, ('x', 'y'), 'normal_up')
        X, Y = float(kw['x']), float(kw['y'])
        positive(x=X, y=Y)
        p, area = [_cabi.THERMAL_RECT, X, Y, 0., 0., 0.], X * Y
    elif kind == 'triangle':
        kw, sign = _shape_kwargs(what, kwargs, ('A', 'B', 'C'), 'normal_up')
        A, B, Cc = (N.ravel(N.asarray(kw[k], dtype=float)) for k in ('A', 'B', 'C'))
        if not (A.shape == B.shape == Cc.shape == (3,)) or not N.all(N.isfinite(N.hstack((A, B, Cc)))):
            raise ValueError("%s: A, B and C are three finite 3-vectors" % what)
        if not (A[2] == B[2] == Cc[2]):
            raise ValueError("%s: the triangle must lie in a plane of constant local z (its normal is +z whatever it is)" % what)
        AB, AC = B - A, Cc - A
        area = 0.5 * abs(AB[0] * AC[1] - AB[1] * AC[0])
        positive(area=area)
        p, origin = [_cabi.THERMAL_TRIANGLE, AB[0], AB[1], AC[0], AC[1], 0.], A
    elif kind == 'cylinder':
        kw, sign = _shape_kwargs(what, kwargs, ('r_ext', 'h'), 'normal_in')
        R, h = float(kw['r_ext']), float(kw['h'])
        positive(r_ext=R, h=h)
        p, area = [_cabi.THERMAL_CYLINDER, R, h, 0., 0., 0.], 2. * N.pi * R * h
    elif kind == 'frustum':
        kw, sign = _shape_kwargs(what, kwargs, ('r0', 'r1', 'z0', 'z1', 'angular_span'), 'normal_in')
        r0, r1, depth = float(kw['r0']), float(kw['r1']), float(kw['z1']) - float(kw['z0'])
        s0, s1 = (float(v) for v in kw.get('angular_span', (0., 2. * N.pi)))
        if not (N.isfinite(r0) and N.isfinite(r1) and r0 >= 0. and r1 >= 0.):
            raise ValueError("%s: r0 and r1 must be finite and not negative" % what)
        if r0 == r1:
            raise ValueError("%s: a frustum needs r0 != r1; use the cylinder" % what)
        positive(depth=depth, angular_span=s1 - s0)
        p = [_cabi.THERMAL_FRUSTUM, r0, r1, depth, s0, s1]
        area = (s1 - s0) / 2. * (r0 + r1) * N.sqrt((r1 - r0) ** 2. + depth ** 2.)
    elif kind == 'sphere':
        kw, sign = _shape_kwargs(what, kwargs, ('r_ext',), 'normal_in')
        R = float(kw['r_ext'])
        positive(r_ext=R)
        p, area = [_cabi.THERMAL_SPHERE, R, 0., 0., 0., 0.], 4. * N.pi * R ** 2.
    else:
        raise ValueError("%s: shape type %r is not one of disk, rectangle, triangle, cylinder, frustum, sphere" % (what, kind))
    return p, float(area), origin, sign


def _thermal_desc(what, shape, table, center, rot_pos, rot_dir, energy, rays_in):
    p, area, origin, sign = _thermal_shape(what, shape)
    if rays_in:
        sign = -sign
    center = N.ravel(N.asarray(center, dtype=float))
    if center.shape != (3,):
        raise ValueError("%s: the location is a 3-vector" % what)
    center = center + N.dot(rot_pos, origin)
    return _fill_source(_cabi.SRC_EMIT_THERMAL, center, rot_pos, rot_dir, p + [sign, 0.], energy(area)), area


def band_radiance(T, band):
    """(L_band, wl_avg, wls) of a black body at T (K) in band = (lo, hi) (m) as the reference computes them (sources.py:788-790,
    :808): Planck's law on linspace(lo, hi, int((hi - lo) / 1e-9)), its trapezoid integral, and the radiance-weighted mean of the
    grid's wavelengths"""
    from .source_spectrum import planck
    T = float(T)
    lo, hi = float(band[0]), float(band[1])
    if not T > 0.:
        raise ValueError("band_radiance: T must be positive")
    if not (hi > lo > 0.) or int((hi - lo) / 1e-9) < 2:
        raise ValueError("band_radiance: the band must be 0 < lo < hi, at least 2e-9 m wide")
    wls = N.linspace(lo, hi, int((hi - lo) / 1e-9))
    B = planck(wls, T)
    return _trapezoid(B, wls), N.sum(wls * B) / N.sum(B), wls


def thermal_emitter_bundle(num_rays, shape, thetas, band_emittance, T, band, center, direction, ref_index=1., rays_in=False,
                           spectrum='band_average', quadrature='trapezoid', seed=None, ray_offset=0, rotation=None):
    """
    Thermal emission of a wall at temperature T (K) with the directional band emittance eps(theta) in the spectral band (lo, hi) (m),
    into the medium of index ref_index: what the reference's spectral_band_axisymmetrical_thermal_emission_source (sources.py:771-813)
    models, with the points, normals and directions of every ray drawn on the device from its Philox stream -- the bundle stays
    pending.  shape: gray_source's dictionary {'type': 'disk' | 'rectangle' | 'triangle' | 'cylinder' | 'frustum' | 'sphere',
    'kwargs': {...}}, the kwargs by the names of ray_trace_utils.sampling.<type>_sampling; the shape is posed at `center` by the
    minimal rotation of +z to `direction`, or by `rotation` (3, 3).  Rays leave along the shape's normal, against it with rays_in.

    thetas, band_emittance: the table, eps linear between its points; a scalar band_emittance is a constant table over thetas.  The
    polar angle about the normal has the density eps(theta) cos(theta) sin(theta).  The reference draws it from a piecewise-linear
    proposal and weights the rays; here the analytic CDF is inverted per ray, so every ray carries the same energy:
    exitance * area / num_rays, exitance = 2 pi L_band * integral of eps cos sin, L_band the reference's (band_radiance).
    quadrature='trapezoid' takes the integral as the reference does (:798, the trapezoid rule over the nodes -- the default, for
    parity), 'exact' the analytic integral of the table.  A table whose node trapezoid is not positive (two points over [0, pi/2])
    is a ValueError under 'trapezoid'.

    spectrum: 'band_average' -- every ray has the reference's wl_avg (:808); 'planck' -- one wavelength per ray drawn from Planck's law
    in the band (SourceSpectrum.planck); a SourceSpectrum or None is taken as given.
    Draws of ray i (event 0, block 0): u0, u1 the point in the sampler's draw order, u2 the polar angle, u3 the azimuth.
    """
    what = 'thermal_emitter_bundle'
    if int(num_rays) < 0:
        raise ValueError("%s: num_rays must not be negative" % what)
    thetas = N.ravel(N.asarray(thetas, dtype=float))
    eps = N.asarray(band_emittance, dtype=float)
    eps = N.full(thetas.shape, float(eps)) if eps.ndim == 0 else N.ravel(eps)
    table = emittance_table(thetas, eps)
    L_band, wl_avg, _ = band_radiance(T, band)
    if quadrature == 'trapezoid':
        integral = _trapezoid(eps * N.cos(thetas) * N.sin(thetas), thetas)
    elif quadrature == 'exact':
        integral = table.mass
    else:
        raise ValueError("%s: quadrature must be 'trapezoid' or 'exact', got %r" % (what, quadrature))
    if not integral > 0.:       # (two points over [0, pi/2]: both nodes of the trapezoid are 0 -- or below, pi/2 written to 8 decimals)
        raise ValueError("%s: the node trapezoid of eps cos sin over this table is %g: no power to emit; quadrature='exact' "
                         "integrates the table" % (what, integral))
    exitance = 2. * N.pi * L_band * integral
    if isinstance(spectrum, str):
        from .source_spectrum import SourceSpectrum
        if spectrum == 'band_average':
            spectrum = SourceSpectrum.monochromatic(wl_avg, ref_index)
        elif spectrum == 'planck':
            spectrum = SourceSpectrum.planck(T, band, ref_index=ref_index)
        else:
            raise ValueError("%s: spectrum must be 'band_average', 'planck', a SourceSpectrum or None, got %r" % (what, spectrum))
    rot = _lamp_frame(direction, rotation)
    desc, _ = _thermal_desc(what, shape, table, center, rot, rot, lambda area: exitance * area / max(int(num_rays), 1), rays_in)
    return _new_bundle(desc, num_rays, seed, ray_offset, spectrum=spectrum, table=table)


def spectral_band_axisymmetrical_thermal_emission_source(positions, normals, area, thetas, band_emittance, T, nrays, band, ref_index):
    """
    The reference's function of this name (sources.py:771-813) on host-given points: a materialised bundle of nrays rays leaving
    `positions` (3, nrays) about `normals` (3, nrays), drawn from numpy's global generator as the reference draws them -- the polar
    angles by its weighted sampler (sampling.PW_lincossin_distribution), then the azimuths -- with its energies (the weights over
    their sum, times exitance times area), its wl_avg and ref_index columns.  thermal_emitter_bundle is the device form.
    """
    from .sampling import PW_lincossin_distribution
    from .vector_manipulations import rotate_z_to_normal
    thetas = N.asarray(thetas, dtype=float)
    L_band, wl_avg, _ = band_radiance(T, band)
    source_radiance = N.asarray(band_emittance, dtype=float) * L_band
    thetas_rays, weights = PW_lincossin_distribution(thetas, source_radiance).sample(nrays)
    source_exitance = _trapezoid(source_radiance * N.cos(thetas) * N.sin(thetas), thetas) * 2. * N.pi
    phis_rays = N.random.uniform(size=nrays) * 2. * N.pi
    directions = N.array([N.sin(thetas_rays) * N.cos(phis_rays), N.sin(thetas_rays) * N.sin(phis_rays), N.cos(thetas_rays)])
    directions = rotate_z_to_normal(directions, normals)
    energy = weights / N.sum(weights) * source_exitance * area
    rayb = RayBundle(vertices=positions, directions=directions, energy=energy)
    rayb._create_property('wavelengths', N.ones(nrays) * wl_avg)
    rayb._create_property('ref_index', N.ones(nrays) * ref_index)
    return rayb


def gray_source(shape, location, direction, num_rays, directions_distribution, energy, rays_direction=None, seed=None, ray_offset=0):
    """
    The reference's general gray source (sources.py:44-66) -- a shape sampler composed with a direction law, of which it has the
    Lambertian one -- as a pending bundle: a thermal descriptor with the constant emittance table over [0, ang_range], which the
    device samples by the closed form of the Lambertian law.  shape: {'type': ..., 'kwargs': {...}} as thermal_emitter_bundle's;
    directions_distribution: {'type': 'Lambertian', 'kwargs': {'ang_range': ...}}.  The points are posed by the minimal rotation of
    +z to `direction` and moved to `location`, the directions by that of +z to rays_direction (direction when None).  Each ray carries
    energy / num_rays -- times cos(dot(rays_direction, direction)) when rays_direction is given: the reference's expression at :63
    as written (the cosine of the scalar product, not the scalar product), kept for parity.
    """
    what = 'gray_source'
    try:
        law, law_kwargs = directions_distribution['type'], dict(directions_distribution.get('kwargs', {}))
    except (TypeError, KeyError):
        raise ValueError("%s: directions_distribution must be a dictionary {'type': ..., 'kwargs': {...}}" % what)
    if law != 'Lambertian':
        raise ValueError("%s: the directions distribution %r is not offered (the reference has Lambertian alone)" % (what, law))
    for k in ('ns', 'normals'):
        law_kwargs.pop(k, None)
    if sorted(law_kwargs) != ['ang_range']:
        raise ValueError("%s: the Lambertian law takes ang_range" % what)
    ang_range = float(law_kwargs['ang_range'])
    if ang_range == 0.:
        raise ValueError("%s: ang_range == 0 has no table (every ray along the normal): not offered" % what)
    if not 0. < ang_range <= N.pi / 2.:
        raise ValueError("%s: ang_range must lie in (0, pi/2]" % what)
    if int(num_rays) < 0:
        raise ValueError("%s: num_rays must not be negative" % what)
    table = emittance_table([0., ang_range], [1., 1.])
    direction = N.ravel(N.asarray(direction, dtype=float))
    per_ray = float(energy) / max(int(num_rays), 1)
    if rays_direction is None:
        rays_direction = direction
    else:
        rays_direction = N.ravel(N.asarray(rays_direction, dtype=float))
        per_ray *= N.cos(N.dot(rays_direction, direction))      # (sources.py:63, as written)
    desc, _ = _thermal_desc(what, shape, table, location, _lamp_frame(direction, None), _lamp_frame(rays_direction, None),
                            lambda area: per_ray, False)
    return _new_bundle(desc, num_rays, seed, ray_offset, table=table)


def single_ray_source(position, direction, flux=None):
    """One ray (sources.py:68-86)."""
    d = N.array(direction, dtype=float).reshape(3, 1)
    d /= N.sqrt(N.sum(d ** 2, axis=0))
    b = RayBundle(vertices=N.asarray(position, dtype=float).reshape(3, 1), directions=d)
    b.set_energy(flux * N.ones(1))
    return b
