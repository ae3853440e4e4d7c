"""
High-flux solar simulator: modules of a truncated ellipsoidal reflector lit by a xenon arc lamp at the first focus, and target plates
that carry flux maps with a confidence interval per bin (classes and constructor arguments of the reference's
tracer/models/solar_simulator.py).

The lamps are device sources: SimulatorLampBader is sources.arc_volume_bundle, SimulatorLampZhu a sphere_emitter_bundle and two
cylinder_emitter_bundles.  A lamp's sources() are pending bundles -- the engines draw every ray from its own Philox stream, nothing of
the size of the bundle is made on the host -- and generate_rays() is the same rays materialised.  SolarSimulator.simulate traces them
with tree=False; tallies and flux maps accumulate on the device, and each Target's map per batch goes into its Estimator.

Where the reference's text cannot run as written it is built as it documents itself: the `homegenizer`
argument is `homogenizer`; the Zhu lamp takes the normals of its surfaces (the text unpacks them from calls made without
normals=True) and directions from isotropic_directions_sampling's law; Estimator.update gets the batch's ray count; a lamp's
theta_CDF is a path or an (N, 2) array; a Target ends the rays it maps, since a device flux map bins absorbed energy -- unless it
is made with transmitting=True, the reference's TransparentTransmitter plate, whose map per batch is TracerEngine.histogram_hits of
the incident energy (section 14.15).
"""
import os
from copy import copy

import numpy as N

from .. import rng
from ..assembly import Assembly
from ..object import AssembledObject
from ..surface import Surface
from ..flat_surface import RectPlateGM
from ..sphere_surface import SphericalGM
from ..ellipsoid import EllipsoidGM
from ..optics_callables import RealReflective, Reflective, TransparentTransmitter
from ..ray_bundle import concatenate_rays
from ..spatial_geometry import general_axis_rotation
from ..vector_manipulations import axes_and_angles_between
from ..estimator import Estimator
from ..tracer_engine import TracerEngine
from ..sources import arc_volume_bundle, sphere_emitter_bundle, cylinder_emitter_bundle


def rotation_z_to(normal):
    """the minimal rotation that takes +z to the unit vector `normal` (rotate_z_to_normal's, as one matrix)"""
    normal = N.ravel(N.asarray(normal, dtype=float))
    axis, ang = axes_and_angles_between(N.array([0., 0., 1.]), normal)
    return N.eye(3) if ang == 0. else general_axis_rotation(axis, ang)


class Target(AssembledObject):
    def __init__(self, width, height, location, normal, binx, biny, transmitting=False):
        """
        A plate for flux mapping whose map is an Estimator: a running mean over the batches with a confidence interval per bin.
        location, normal: position and surface normal of the plate; binx, biny: the bin edges of its local x and y (numpy
        histogram edges), which also size the plate, as in the reference (width and height are kept for the signature).
        The plate absorbs what it maps; with transmitting=True it is the reference's TransparentTransmitter: a virtual plane
        whose map is of the energy that arrives, and the rays go on behind it (an aperture plane, a target in front of a
        homogenizer).
        """
        binx, biny = N.asarray(binx, dtype=float), N.asarray(biny, dtype=float)
        geom = RectPlateGM(binx[-1] - binx[0], biny[-1] - biny[0])
        self.transmitting = bool(transmitting)
        AssembledObject.__init__(self, surfs=[Surface(geometry=geom, optics=TransparentTransmitter() if self.transmitting else Reflective(1.))],
                                 location=location, rotation=rotation_z_to(normal))
        self.binx, self.biny = binx, biny
        self.areas = N.vstack(binx[1:] - binx[:-1]) * (biny[1:] - biny[:-1])
        self.fluxmap = Estimator()
        self._powermap = None       # the device map read last: maps accumulate there, a batch's is the difference

    def evaluate_fluxmap(self, engine, num_samples):
        """the power the plate took since the last call, per bin area, into the estimator (weight: the batch's ray count)"""
        if self.transmitting:
            # nothing is absorbed, so no device flux map: the incident energy of the batch's hits, binned where they lie on the
            # device; the optics are reset as the reference's evaluate_fluxmap resets them, and the next batch starts an empty buffer
            surf = self.get_surfaces()[0]
            batch = engine.histogram_hits(surf, self.binx, self.biny, weight='incident')
            surf.get_optics_manager().reset()
            self.fluxmap.update(batch / self.areas, num_samples=num_samples)
            return self.fluxmap
        total = N.asarray(engine.get_fluxmap(self.get_surfaces()[0]), dtype=float)
        batch = total if self._powermap is None else total - self._powermap
        self._powermap = total
        self.fluxmap.update(batch / self.areas, num_samples=num_samples)
        return self.fluxmap


class SimulatorReflector(AssembledObject):
    def __init__(self, a, b, c, zlim, location, rotation, reflectivity=0.9, slope_error=2.5e-3, bi_var=False):
        """
        An ellipsoidal reflector by its semi-axes a, b, c, cut to zlim along z, with its first focus at `location`;
        slope_error: the standard deviation of the surface's slope error.
        """
        excentricity = N.sqrt(1. - a ** 2 / c ** 2)
        half_focal_dist = c * excentricity
        geom = EllipsoidGM(a, b, c, zlim=zlim)
        opt = RealReflective(absorptivity=1. - reflectivity, sigma=slope_error, bi_var=bi_var)
        AssembledObject.__init__(self, surfs=[Surface(geometry=geom, optics=opt, location=N.array([0., 0., half_focal_dist]))],
                                 location=location, rotation=rotation)
        self.excentricity = excentricity
        self.focal_dist = 2. * half_focal_dist


class _Lamp(object):
    """what the two lamps share: the pose of their parts, and their rays materialised"""
    def _pose(self, pose, local_center=(0., 0., 0.)):
        """(centre column, rotation) of a part whose centre is `local_center` in the lamp's frame, for a lamp at self.loc about
        self.dir inside a module posed by `pose` = (rotation, location), or in the lamp's own referential (pose None)"""
        rot = rotation_z_to(N.asarray(self.dir, dtype=float) / N.sqrt(N.sum(N.asarray(self.dir, dtype=float) ** 2)))
        center = N.dot(rot, N.asarray(local_center, dtype=float)) + N.ravel(N.asarray(self.loc, dtype=float))
        if pose is not None:
            rot, center = N.dot(pose[0], rot), N.dot(pose[0], center) + N.ravel(N.asarray(pose[1], dtype=float))
        return N.vstack(center), rot

    def generate_rays(self, n_rays, part_load=1., seed=None):
        """the lamp's rays in its local referential as one bundle: sources() materialised and concatenated"""
        parts = self.sources(n_rays, part_load, seed)
        for p in parts:
            p.get_vertices()
        return parts[0] if len(parts) == 1 else concatenate_rays(parts)


class SimulatorLampBader(_Lamp):
    def __init__(self, P_elec=2.5e3, eff_el=0.6, r_c=7.5e-4, l_c=4.5e-3, theta_CDF=None, location=[0, 0, 0], direction=[0, 0, 1]):
        """
        The arc as a cylinder volume (Bader et al., doi 10.1115/1.4028702).  P_elec, eff_el: electrical power and its share turned
        into radiation; r_c, l_c: radius and length of the cylinder; theta_CDF: the cumulative distribution of the polar angle
        (rad, within [0, pi], 0 on the lamp's +z) as a file of two columns or an (N, 2) array of (theta, CDF); location,
        direction: centre and axis of the arc in the module's referential, whose origin is the first focus.
        """
        if theta_CDF is None:
            raise ValueError("SimulatorLampBader needs theta_CDF: a file or an (N, 2) array of (theta, CDF)")
        self.P = eff_el * P_elec
        self.r_c, self.l_c = r_c, l_c
        self.loc, self.dir = location, direction
        data = N.loadtxt(theta_CDF) if isinstance(theta_CDF, (str, bytes, os.PathLike)) else N.asarray(theta_CDF, dtype=float)
        if data.ndim != 2 or data.shape[1] != 2 or data.shape[0] < 3:
            raise ValueError("theta_CDF must have two columns (theta, CDF) and three rows or more")
        dths = N.diff(data[:, 0])
        # the density between two points of the CDF, held at their middle; rounded as PW_linear_distribution rounds its table
        self.ths = N.round(data[:-1, 0] + dths / 2., decimals=8)
        self.ths_PDF = N.round(N.diff(data[:, 1]) / dths, decimals=8)

    def sources(self, n_rays, part_load=1., seed=None, pose=None, ray_offset=0):
        center, rot = self._pose(pose)
        return [arc_volume_bundle(int(n_rays), self.r_c, self.l_c, self.ths, self.ths_PDF, center, None, self.P * part_load,
                                  seed=seed, ray_offset=ray_offset, rotation=rot)]


class SimulatorLampZhu(_Lamp):
    def __init__(self, P_elec=7e3, eff_el=0.6, alpha_s=0.3, beta_c1=0.0412, gamma_c2=0.6588, location=[0, 0, 0], direction=[0, 0, 1]):
        """
        The arc as a sphere at the cathode tip and two coaxial cylinder walls (Zhu et al., doi 10.1016/j.apenergy.2020.115165), each
        emitting uniformly in solid angle about its outward normal.  alpha_s, beta_c1, gamma_c2: the shares of the power given
        to the sphere, the inner and the outer cylinder.
        """
        self.a_s, self.b_c1, self.g_c2 = alpha_s, beta_c1, gamma_c2
        self.r_s = (0.5e-3) / 2.
        self.r_c2 = (2e-3) / 2.
        self.l_c = 10e-3
        self.P = eff_el * (alpha_s + beta_c1 + gamma_c2) * P_elec
        self.loc, self.dir = location, direction

    def sources(self, n_rays, part_load=1., seed=None, pose=None, ray_offset=0):
        """sphere, inner cylinder, outer cylinder: int(n_rays x share) rays each, on consecutive stream ids of one seed"""
        P = part_load * self.P
        if seed is None:
            seed = rng.next_seed()
        counts = [int(n_rays * share) for share in (self.a_s, self.b_c1, self.g_c2)]
        offs = [ray_offset, ray_offset + counts[0], ray_offset + counts[0] + counts[1]]
        kw = dict(ang_range=N.pi / 2., law='isotropic', rays_in=False, seed=seed)
        c_s, rot = self._pose(pose, (0., 0., -(self.l_c / 2. - self.r_s)))
        c_c, rot = self._pose(pose)
        return [sphere_emitter_bundle(counts[0], self.r_s, c_s, None, P * self.a_s, ray_offset=offs[0], rotation=rot, **kw),
                cylinder_emitter_bundle(counts[1], self.r_s, self.l_c, c_c, None, P * self.b_c1, ray_offset=offs[1], rotation=rot, **kw),
                cylinder_emitter_bundle(counts[2], self.r_c2, self.l_c, c_c, None, P * self.g_c2, ray_offset=offs[2], rotation=rot, **kw)]


_LAMPS = {'Bader': SimulatorLampBader, 'Zhu': SimulatorLampZhu}


class SolarSimulatorModule(Assembly):
    def __init__(self, a, b, c, zlim, reflectivity=0.9, slope_error=2.5e-3, bi_var=False, lampdict=None,
                 first_focus_location=N.array([0, 0, 0]), aiming_vector=N.array([0, 0, 1])):
        """
        An ellipsoidal reflector (SimulatorReflector's a, b, c, zlim, reflectivity, slope_error) and its lamp.  lampdict: 'model'
        ('Bader' or 'Zhu') and the arguments of that lamp's class; first_focus_location: where the module's first focus is;
        aiming_vector: the unit vector from the first focus to the second.
        """
        if lampdict is None or lampdict.get('model') not in _LAMPS:
            raise ValueError("lampdict needs a 'model': one of %s" % sorted(_LAMPS))
        self.location = N.ravel(N.asarray(first_focus_location, dtype=float))
        self.aiming_vector = N.ravel(N.asarray(aiming_vector, dtype=float))
        self.rotation = rotation_z_to(self.aiming_vector)
        self.reflector = SimulatorReflector(a, b, c, zlim, self.location, self.rotation, reflectivity, slope_error, bi_var)
        Assembly.__init__(self, objects=[self.reflector])
        lamp_params = copy(lampdict)
        self.lamp = _LAMPS[lamp_params.pop('model')](**lamp_params)

    def lamp_sources(self, nrays, part_load=1., seed=None):
        """the lamp's pending bundles posed in the general referential"""
        return self.lamp.sources(nrays, part_load, seed, pose=(self.rotation, self.location))

    def fire_lamp(self, nrays, lamp_mapper=False, part_load=1., seed=None):
        """the lamp's rays posed in the general referential, as one bundle; lamp_mapper: adds a transparent sphere around the arc
        that records what crosses it"""
        if lamp_mapper:
            mapper = AssembledObject(surfs=[Surface(geometry=SphericalGM(radius=2. * self.lamp.l_c), optics=TransparentTransmitter())],
                                     location=self.location, rotation=self.rotation)
            self.add_object(mapper)
        parts = self.lamp_sources(nrays, part_load, seed)
        for p in parts:
            p.get_vertices()
        return parts[0] if len(parts) == 1 else concatenate_rays(parts)


class SolarSimulator(Assembly):
    def __init__(self, modules_positions, modules_directions, modules_dicts, targets, homogenizer=None):
        """
        modules_positions, modules_directions: per module the position of its first focus and the unit vector of its optical axis
        (first to second focus); modules_dicts: per module the arguments of SolarSimulatorModule; targets: Target objects;
        homogenizer: objects added behind them.
        """
        self.modules = [SolarSimulatorModule(first_focus_location=modules_positions[i], aiming_vector=modules_directions[i], **modules_dicts[i])
                        for i in range(len(modules_positions))]
        self.targets = list(targets)
        objects = list(targets)
        if homogenizer is not None:
            self.homogenizer = homogenizer
            objects += list(homogenizer)
        Assembly.__init__(self, subassemblies=self.modules, objects=objects)
        self.engine = None

    def simulate(self, nrays, part_load=1., lamp_mapper=False, rendering=False, ray_batch=1e4, save_dir=None, seed=None):
        """
        Traces nrays rays per module in batches of ray_batch; after each batch every target's map of that batch goes into its
        Estimator.  Returns the targets' estimators.  save_dir: where fluxmap_<j>.csv and confidence_intervals_<j>.csv are
        written after each batch (None: nowhere).  seed: of the first lamp of the first batch (the others follow it).
        """
        if rendering:
            raise NotImplementedError('tracer_amd has no Coin3D viewer: trace with it, render with the reference')
        if lamp_mapper:
            raise NotImplementedError('lamp_mapper changes the scene between batches; map a lamp with fire_lamp(lamp_mapper=True)')
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
        ray_batch = int(min(ray_batch, nrays))
        engine = self.engine = TracerEngine(self)
        for t in self.targets:
            t._powermap = None
            if t.transmitting:      # (its batch map comes from the hits themselves: Target.evaluate_fluxmap)
                t.get_surfaces()[0].get_optics_manager().reset()
            else:
                engine.set_fluxmap(t.get_surfaces()[0], t.binx, t.biny)
        call = 0
        for i in range(int(nrays / ray_batch)):
            for m in self.modules:
                for bundle in m.lamp_sources(ray_batch, part_load, None if seed is None else seed + call):
                    if bundle.get_num_rays() > 0:
                        engine.ray_tracer(bundle, tree=False)
                call += 1
            for j, t in enumerate(self.targets):
                t.evaluate_fluxmap(engine, ray_batch)
                if save_dir is not None:
                    _write_map(os.path.join(save_dir, 'fluxmap_%i.csv' % j), t, t.fluxmap.mean)
                    _write_map(os.path.join(save_dir, 'confidence_intervals_%i.csv' % j), t, t.fluxmap.get_CI())
        return [t.fluxmap for t in self.targets]


def _write_map(path, target, values):
    with open(path, 'w') as fo:
        for name, edges in (('bins_x', target.binx), ('bins_y', target.biny)):
            fo.write(name + ',' + ''.join(str(e) + ',' for e in edges) + '\n')
        for row in N.atleast_2d(values):
            fo.write(''.join(str(f) + ',' for f in row) + '\n')
