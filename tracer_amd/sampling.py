"""
Host samplers with the names, arguments and return values of the reference's ray_trace_utils/sampling.py that the arc-lamp model
(models/solar_simulator.py) and scene scripts import: PW_linear_distribution (:6-52), disk_sampling (:286-295), cylinder_sampling
(:365-382), sphere_sampling (:426-444, the surface only), Lambertian_directions_sampling (:446-459) -- and
isotropic_directions_sampling, which the model calls and the reference defines nowhere (defined here by its name: uniform in solid
angle over the cone).  For the thermal emitters (sources.spectral_band_axisymmetrical_thermal_emission_source): PW_lincos_distribution
(:99-122), PW_lincossin_distribution (:124-148), triangle_sampling (:308-331), frustum_sampling (:384-400, the surface only) and
rectangle_sampling (:297-306) as it is meant -- the reference's raises NameError.

Functions of numpy's global generator that draw what the reference draws, in its order, so that under the same numpy.random.seed
they return its arrays.  The device sources (sources.arc_volume_bundle, sphere_emitter_bundle, cylinder_emitter_bundle) sample the
same distributions per ray from Philox streams instead; these are for scripts that want the arrays, and for the tests that pin both.

Not offered: volume sampling of a sphere and of a frustum (broken in the reference), polygon_sampling (shapely), the bilinear and
BDRF distributions.
"""
import numpy as N

from .vector_manipulations import rotate_z_to_normal


class PW_linear_distribution(object):
    """
    A density that interpolates (xs, ys) linearly, not normalised: value, PDF, CDF, and inverse-CDF sampling.  xs and ys are rounded
    to 8 decimals as the reference rounds them; the integrals of the intervals come from the values as given.
    """
    def __init__(self, xs, ys):
        xs, ys = N.asarray(xs, dtype=float), N.asarray(ys, dtype=float)
        self.xs = N.round(xs, decimals=8)
        self.ys = N.round(ys, decimals=8)
        self.a = (self.ys[1:] - self.ys[:-1]) / (self.xs[1:] - self.xs[:-1])       # slope and intercept per interval
        self.b = self.ys[:-1] - self.a * self.xs[:-1]
        self.integ = (xs[1:] - xs[:-1]) * (ys[1:] + ys[:-1]) / 2.
        self.tot_integ = N.sum(self.integ)
        self.PDF_def = self.ys / self.tot_integ
        self.CDF_def = N.add.accumulate(N.hstack([[0], self.integ])) / self.tot_integ

    def find_slice(self, x):
        """the interval of each x: the number of points below it, less one"""
        return N.sum((x > N.vstack(self.xs)).T, axis=1) - 1

    def __call__(self, x):
        loc = self.find_slice(x)
        return self.a[loc] * x + self.b[loc]

    def PDF(self, x):
        return self(x) / self.tot_integ

    def CDF(self, x):
        loc = self.find_slice(x)
        return self.CDF_def[loc] + (x - self.xs[loc]) * (self.PDF(x) + self.PDF_def[loc]) / 2.

    def sample(self, ns):
        """(ns samples, their weights -- all 1): one uniform each, inverted interval by interval"""
        x_samples = N.zeros(ns)
        R = N.random.uniform(size=ns)
        a = self.a / (2. * self.tot_integ)
        b = self.b / self.tot_integ
        c = self.CDF_def[:-1] - a * self.xs[:-1] ** 2 - b * self.xs[:-1]
        for i in range(len(self.CDF_def) - 1):
            here = N.logical_and(R >= self.CDF_def[i], R < self.CDF_def[i + 1])
            if not here.any():
                continue
            if a[i] == 0.:
                x_samples[here] = self.xs[i] + (R[here] - self.CDF_def[i]) / b[i]
            else:
                D = b[i] ** 2. - 4. * a[i] * (c[i] - R[here])
                x_samples[here] = (-b[i] + N.sqrt(D)) / (2. * a[i])
        return x_samples, N.ones(len(R))


class PW_lincos_distribution(PW_linear_distribution):
    """
    The density ys(x) cos(x), ys linear between the points, sampled as the reference samples it: x from the piecewise-linear
    interpolation of the nodes' ys cos(xs), each sample weighted by the true density over that proposal, the weights rescaled to
    the sum ns.
    """
    def __init__(self, xs, ys):
        xs, ys = N.asarray(xs, dtype=float), N.asarray(ys, dtype=float)
        PW_linear_distribution.__init__(self, xs, ys * N.cos(xs))
        self.a_cos = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1])
        self.b_cos = ys[:-1] - self.a_cos * xs[:-1]
        self.integ_cos = ys[1:] * N.sin(xs[1:]) - ys[:-1] * N.sin(xs[:-1]) + self.a_cos * (N.cos(xs[1:]) - N.cos(xs[:-1]))
        self.tot_integ_cos = N.sum(self.integ_cos)

    def f(self, x):
        loc = self.find_slice(x)
        return (self.a_cos[loc] * x + self.b_cos[loc]) * N.cos(x)

    def PDF_cos(self, x):
        return self.f(x) / self.tot_integ_cos

    def sample(self, ns):
        x_s, weights_s = PW_linear_distribution.sample(self, ns)
        weights = weights_s * self.PDF_cos(x_s) / self.PDF(x_s)
        weights *= ns / N.sum(weights)
        return x_s, weights


class PW_lincossin_distribution(PW_linear_distribution):
    """
    The density ys(x) cos(x) sin(x) -- the polar angle of a surface of directional emittance ys -- sampled as the reference samples
    it: x from the piecewise-linear interpolation of the nodes' ys cos sin, weighted by the true density over that proposal, the
    weights rescaled to the sum ns.

    tot_integ_cossin is kept as the reference computes it: the antiderivative at every node with the slope of the interval to the
    node's right (the last node: to its left), for both ends of an interval.  Where the slope changes between intervals this is not
    the integral (0.9690 for a table whose integral is 0.3504).  It only scales weights that sample() renormalises,
    so the samples and weights are the reference's; nothing here takes it for the mass -- sources.EmittanceTable.mass is that.
    """
    def __init__(self, xs, ys):
        xs, ys = N.asarray(xs, dtype=float), N.asarray(ys, dtype=float)
        PW_linear_distribution.__init__(self, xs, ys * N.cos(xs) * N.sin(xs))
        self.a_cossin = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1])
        self.b_cossin = ys[:-1] - self.a_cossin * xs[:-1]
        slope_at_node = N.hstack([self.a_cossin, self.a_cossin[-1]])
        integral = ys / 2. * N.sin(xs) ** 2. - slope_at_node / 4. * (xs - N.sin(xs) * N.cos(xs))
        self.integ_cossin = integral[1:] - integral[:-1]
        self.tot_integ_cossin = N.sum(self.integ_cossin)

    def f(self, x):
        loc = self.find_slice(x)
        return (self.a_cossin[loc] * x + self.b_cossin[loc]) * N.cos(x) * N.sin(x)

    def PDF_cossin(self, x):
        return self.f(x) / self.tot_integ_cossin

    def sample(self, ns):
        x_s, weights_s = PW_linear_distribution.sample(self, ns)
        weights = weights_s * self.PDF_cossin(x_s) / self.PDF(x_s)
        weights *= ns / N.sum(weights)
        return x_s, weights


def _flat_normals(ns, normal_up):
    normals = N.vstack([N.zeros(ns), N.zeros(ns), N.ones(ns)])
    return normals if normal_up else -normals


def disk_sampling(r_ext, ns, normals=False, normal_up=True):
    """(3, ns) points uniform on the disc of radius r_ext in the plane z = 0 (draws: azimuths, then radii); with normals=True also
    their normals, +z or -z"""
    ths = N.random.uniform(size=ns) * 2. * N.pi
    rs = N.sqrt(N.random.uniform(size=ns)) * r_ext
    positions = N.vstack([rs * N.cos(ths), rs * N.sin(ths), N.zeros(ns)])
    if normals:
        return positions, _flat_normals(ns, normal_up)
    return positions


def rectangle_sampling(x, y, ns, normals=False, normal_up=True):
    """(3, ns) points uniform on the rectangle of x by y about the origin in the plane z = 0 (draws: xs over [-x/2, x/2], then ys over
    [-y/2, y/2]; the points are (xs, ys, 0), as the device's rectangle, TRC_THERMAL_RECT, has them); with normals=True also their
    normals.  The reference's function names variables it does not have and raises NameError, so it has no behaviour to keep: this
    is what its arguments say."""
    xs = N.random.uniform(low=-x / 2., high=x / 2., size=ns)
    ys = N.random.uniform(low=-y / 2., high=y / 2., size=ns)
    positions = N.vstack((xs, ys, N.zeros(ns)))
    if normals:
        return positions, _flat_normals(ns, normal_up)
    return positions


def triangle_sampling(A, B, C, ns, normals=False, normal_up=True):
    """(3, ns) points uniform on the triangle A, B, C (draws: r1, then r2; the point A + sqrt(r1) (1 - r2) AB + r2 sqrt(r1) AC);
    with normals=True also the normals, which are +z or -z whatever the triangle: it is meant to lie in a plane of constant z."""
    A, B, C = (N.asarray(v, dtype=float) for v in (A, B, C))
    r1 = N.vstack(N.random.uniform(size=ns))
    r2 = N.vstack(N.random.uniform(size=ns))
    sqrtr1 = N.sqrt(r1)
    positions = (A + sqrtr1 * (1. - r2) * (B - A) + r2 * sqrtr1 * (C - A)).T
    if normals:
        return positions, _flat_normals(ns, normal_up)
    return positions


def frustum_sampling(r0, r1, z0, z1, ns, normals=False, normal_in=False, volume=False, angular_span=[0., 2. * N.pi]):
    """(3, ns) points uniform on the wall of the frustum of radius r0 at height 0 and r1 at height z1 - z0 about z, within the
    angular span (draws: R, then the azimuths): r = sqrt((r1^2 - r0^2) R + r0^2), z = (r - r0) / c with c = (r1 - r0) / (z1 - z0).
    With normals=True also the wall's normals, as the reference gives them: (cos phi sin ts, sin phi sin ts, cos ts) with ts =
    arctan(c) - pi/2 for normal_in, its opposite otherwise.  The volume form does not run in the reference and is not offered."""
    if volume:
        raise NotImplementedError("frustum_sampling(volume=True) does not run in the reference (undefined names); not offered")
    c = (r1 - r0) / (z1 - z0)
    R = N.random.uniform(size=ns)
    phi = N.random.uniform(low=angular_span[0], high=angular_span[1], size=ns)
    rs = N.sqrt((r1 ** 2. - r0 ** 2.) * R + r0 ** 2.)
    positions = N.array([rs * N.cos(phi), rs * N.sin(phi), (rs - r0) / c])
    if normals:
        theta_s = N.arctan(c) - N.pi / 2.
        norms = N.array([N.cos(phi) * N.sin(theta_s), N.sin(phi) * N.sin(theta_s), N.ones(ns) * N.cos(theta_s)])
        return positions, (norms if normal_in else -norms)
    return positions


def cylinder_sampling(r_ext, h, ns, normals=False, normal_in=False, volume=False):
    """
    (3, ns) points uniform on the wall of the cylinder of radius r_ext and height h about z, centred on the origin (draws: heights,
    azimuths) -- with normals=True also the wall's normals there, outwards or inwards -- or, volume=True, uniform in its volume
    (draws: heights, then disk_sampling's).
    """
    zs = N.random.uniform(size=ns) * h - h / 2.
    if volume:
        positions = disk_sampling(r_ext, ns)
        positions[2] = zs
        return positions
    ths = N.random.uniform(size=ns) * 2. * N.pi
    positions = N.vstack([r_ext * N.cos(ths), r_ext * N.sin(ths), zs])
    if normals:
        norms = N.vstack([N.cos(ths), N.sin(ths), N.zeros(ns)])
        return positions, (-norms if normal_in else norms)
    return positions


def sphere_sampling(r_ext, ns, normals=False, normal_in=False, volume=False):
    """(3, ns) points uniform on the sphere of radius r_ext (draws: azimuths, then cosines of the polar angle); with normals=True
    also the normals there, outwards or inwards.  The volume form is broken in the reference and not offered."""
    if volume:
        raise NotImplementedError("sphere_sampling(volume=True) does not run in the reference (N.cuberoot); not offered")
    phis = N.random.uniform(size=ns) * 2. * N.pi
    cosths = N.random.uniform(low=-1., high=1., size=ns)
    sinths = N.sqrt(1. - cosths ** 2)
    norms = N.vstack([sinths * N.cos(phis), sinths * N.sin(phis), cosths])
    positions = r_ext * norms
    if normals:
        return positions, (-norms if normal_in else norms)
    return positions


def Lambertian_directions_sampling(ns, ang_range, normals=None):
    """(3, ns) unit directions, cosine-weighted within ang_range of +z (draws: azimuths, then -- unless ang_range is 0 -- the polar
    uniforms), turned to `normals` (3, ns) by the minimal rotation when given"""
    xi1 = N.random.uniform(low=0., high=2. * N.pi, size=ns)
    if ang_range == 0.:
        dirs = N.zeros((3, ns))
        dirs[2] = 1.
    else:
        xi2 = N.random.uniform(size=ns)
        sinsqrt = N.sin(ang_range) * N.sqrt(xi2)
        dirs = N.vstack((N.cos(xi1) * sinsqrt, N.sin(xi1) * sinsqrt, N.sqrt(1. - sinsqrt ** 2.)))
    if normals is not None:
        dirs = rotate_z_to_normal(dirs, normals)
    return dirs


def isotropic_directions_sampling(num_rays, ang_range, normals=None):
    """
    (3, num_rays) unit directions uniform in solid angle within ang_range of +z: azimuth xi1 ~ U(0, 2 pi), then xi2 ~ U(0, 1) -- the
    order of the Lambertian sampler -- with cos(theta) = 1 - xi2 (1 - cos(ang_range)); turned to `normals` by the minimal rotation
    when given.  The reference's solar-simulator model calls a function of this name and defines none: this is its definition here.
    """
    xi1 = N.random.uniform(low=0., high=2. * N.pi, size=num_rays)
    xi2 = N.random.uniform(size=num_rays)
    cosths = 1. - xi2 * (1. - N.cos(ang_range))
    sinths = N.sqrt((1. - cosths) * (1. + cosths))
    dirs = N.vstack((N.cos(xi1) * sinths, N.sin(xi1) * sinths, cosths))
    if normals is not None:
        dirs = rotate_z_to_normal(dirs, normals)
    return dirs
