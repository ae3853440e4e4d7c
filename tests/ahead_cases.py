"""
The scenes of the tests of the segments finished ahead (csrc/trc_shade.hip: k_s_shade_c's AHEAD; csrc/trc_forms.h:
trc_stream_form_ahead), shared by tests/test_gpu_finish_ahead.py and tests/test_finish_ahead_host.py.  They are the fields of
clear_cases.py -- heliostats that track the sun onto a receiver the grid sets apart -- with what stands at the tower varied: the
path finishes a continued ray inside its clear cone only when the nearest surface set apart that it meets ends every ray, or when it
meets none.
"""
import numpy as N

import clear_cases as K

PLATE = [[0., 36., 0.]]


def _plate(w, h, optics, y, z, x=0.):
    """a plate of w x h at (x, y, z) that faces the field (its normal along +y), with the optics given"""
    from tracer_amd.object import AssembledObject
    from tracer_amd.surface import Surface
    from tracer_amd.flat_surface import RectPlateGM
    from tracer_amd.spatial_geometry import rotx, translate
    return AssembledObject(surfs=[Surface(RectPlateGM(w, h), optics)], transform=N.dot(translate(x, y, z), rotx(-N.pi / 2.)))


def one_plate():
    """one plate (and the four that stand clear of everything): every continued ray is inside its cone -- the Buie aureole ends at
    43.6 mrad, the cones of plates without a neighbour are capped at 0.2 rad -- so no ray is left for k_s_bounce"""
    return K._plant(PLATE + K.BYSTANDERS, sigma=1e-4)


def nsttf_tracked(n=40):
    """the first n heliostats of NSTTF after track_sun to another azimuth and zenith"""
    from tracer_amd import scenes
    from tracer_amd.models.heliostat_field import solar_vector
    plant, field, src = K.nsttf(n)
    pos = scenes.nsttf_positions()[:n]
    zen = 55. * N.pi / 180.
    field.track_sun(0.3, zen, aim_points=N.tile(N.array([0., 0., 60.]), (n, 1)))
    sun = solar_vector(0.3, zen)
    return plant, field, dict(src, center=N.vstack(300. * sun + N.r_[pos[:, :2].mean(axis=0), 0.]), direction=-sun)


def reflective_receiver():
    """the receiver sends half of every ray on: no surface ends every ray, terminal hits are not finished in the search, the path
    stays out"""
    from tracer_amd.models.one_sided_mirror import one_sided_receiver
    from tracer_amd.spatial_geometry import rotx, translate
    rec = one_sided_receiver(11., 11., absorptivity=0.5)
    rec.set_transform(N.dot(translate(0., 0., K.TOWER), rotx(-N.pi / 2.)))
    return K._plant([[0., 30., 0.], [0., 34.2, 0.], [0., 38.4, 0.]] + K.BYSTANDERS, extra_objects=[rec], receiver=False)


def mirror_before_receiver():
    """a receiver that ends every ray and, 2 m in front of its lower half, a mirror plate that does not: a ray whose nearest surface
    at the tower is the mirror is not finished ahead, whether the grid sets the mirror apart or lists it"""
    from tracer_amd import optics_callables as opt
    return K._plant(PLATE + [[4., 33., 0.]] + K.BYSTANDERS, extra_objects=[_plate(6., 3., opt.Reflective(0.3), 2., K.TOWER - 3.)])


def two_receivers():
    """two surfaces that end every ray at the tower, the smaller one 1.5 m in front of the right half of the other (its edge crosses
    the image of the field): nearest hit, and the lower index on equal distance"""
    from tracer_amd import optics_callables as opt
    front = _plate(5., 11., opt.OneSidedReflectiveReceiver(1.), 1.5, K.TOWER, x=2.5)
    return K._plant(PLATE + [[4., 33., 0.], [-5., 39., 0.]] + K.BYSTANDERS, extra_objects=[front])


def no_capture():
    """the receiver ends every ray and captures nothing: no hit buffer, no chunks of it to carry"""
    from tracer_amd import optics_callables as opt
    rec = _plate(11., 11., opt.OneSidedReflective(1.), 0., K.TOWER)
    return K._plant([[0., 30., 0.], [0., 34.2, 0.], [0., 38.4, 0.]] + K.BYSTANDERS, extra_objects=[rec], receiver=False)


def two_mirror_kinds():
    """two plates, one of which keeps 96 % of a ray and the other half of it: a min_energy between the two ends the rays of the one at
    their mirror and lets those of the other go on"""
    plant, field, src = K._plant(PLATE + [[4., 33., 0.]] + K.BYSTANDERS)
    field.get_heliostats()[1].get_surfaces()[0].get_optics_manager()._abs = 0.5
    return plant, field, src


def receiver_index(cs):
    """the receiver of K.nsttf, and of K._plant without extra objects: the field's surfaces come first, the receiver is the last"""
    return cs.n_surf - 1


def fluxmap_edges(bins):
    """bins x bins over the receiver's 11 m x 11 m"""
    e = N.linspace(-5.5, 5.5, bins + 1)
    return e, e
