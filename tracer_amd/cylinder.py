"""
Cylinders about the local z axis: infinite, finite (height and angular range), rectangular-cut.
Constructors as in the reference's tracer/cylinder.py (:12-18, :59-68, :161-168).
"""
import numpy as N
from . import _cabi
from .quadric import QuadricGM
from .flat_surface import _grid_flux


class InfiniteCylinder(QuadricGM):
    def __init__(self, diameter):
        self._R = diameter / 2.
        QuadricGM.__init__(self)

    def _native(self):
        return _cabi.GM_CYL_INF, [self._R], []


class FiniteCylinder(InfiniteCylinder):
    def __init__(self, diameter, height, ang_range=[0., 2. * N.pi]):
        self._half_h = height / 2.
        assert len(ang_range) == 2
        self._ang_range = ang_range
        InfiniteCylinder.__init__(self, diameter)

    def _native(self):
        return _cabi.GM_CYL_FINITE, [self._R, self._half_h, self._ang_range[0], self._ang_range[1]], []

    def fluxmap_grid(self, resolution):
        """(chart, swap_xy, u_edges, v_edges, areas): the grid of get_fluxmap -- height by azimuth over ang_range
        (cylinder.py:139-159) -- for a flux map binned on the device (TracerEngine.set_surface_fluxmap)."""
        zs = N.linspace(-self._half_h, self._half_h, resolution + 1)
        angs = N.linspace(self._ang_range[0], self._ang_range[1], resolution + 1)
        areas = N.diff(zs)[:, None] * (self._R * N.diff(angs))[None, :]
        return 'cylinder', False, zs, angs, areas

    def get_fluxmap(self, eners, local_coords, resolution):
        """Energy per area on a (z, azimuth) grid of the wall."""
        az = N.arctan2(local_coords[1], local_coords[0])
        az[az < 0.] += 2. * N.pi
        return _grid_flux(self.fluxmap_grid(resolution), local_coords[2], az, eners)


class RectCutCylinder(FiniteCylinder):
    def __init__(self, diameter, height, w, h):
        FiniteCylinder.__init__(self, diameter, height)
        self.half_dims = N.array([w / 2., h / 2.])
        if N.sqrt(N.sum(self.half_dims ** 2)) <= self._R:
            raise ValueError('Bad rectangular cut cylinder shape, width and height too small')

    def _native(self):
        return _cabi.GM_CYL_RECTCUT, [self._R, self._half_h, self.half_dims[0], self.half_dims[1]], []
