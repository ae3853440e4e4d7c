"""
Spectra of sources: every ray of a source descriptor gets one wavelength, drawn on the device from the spectrum attached to
the descriptor (include/tracer_amd.h, trc_source_spectrum; csrc/trc_core.h, trc_spectrum_draw).  The usual spectral Monte
Carlo: a source with a spectrum stays a pending LazySourceBundle, and the engines trace it without host wavelength columns.

A spectrum can also be CARRIED (SourceSpectrum.polychromatic, .as_polychromatic()): no wavelength is drawn, every source ray is
polychromatic and carries all W points of the table as its sample wavelengths, with the spectrum energy_of_ray * table()[1] --
one ray integrates the whole spectrum.  Such a bundle stays pending too; the device makes the (W, n) columns when they are needed.

The table is a piecewise-linear spectral density, sampled by the inverse of its CDF as the reference's
ray_trace_utils/sampling.py:35-52 (PW_linear_distribution.sample) does -- without its rounding of the abscissae to 8 decimals,
which snaps wavelengths given in metres to 10 nm.
"""
import ctypes as C

import numpy as N

from . import _cabi

MAX_POINTS = _cabi.SPECTRUM_MAX_POINTS


def planck(wl, T):
    """Planck's law, spectral radiance per unit wavelength (W / m^2 / sr / m) at wavelengths wl (m), temperature T (K): the
    reference's ray_trace_utils/electromagnetics.py:3-14, with its constants."""
    h = 6.626070040e-34
    c = 299792458.
    k = 1.38064852e-23
    wl = N.asarray(wl, dtype=float)
    hc_kTwl = h * c / (k * T * wl)
    return (2. * h * c ** 2.) / (wl ** 5.) / (N.exp(hc_kTwl) - 1.)


class SourceSpectrum(object):
    """
    A spectrum for a source descriptor: monochromatic (every ray has one wavelength), tabulated (piecewise-linear density a
    wavelength is drawn from per ray) or polychromatic (the same table, carried whole by every ray).
    ref_index is the index of the medium the rays start in.  Inputs are checked here (ValueError); desc() packs the
    trc_source_spectrum the C-ABI takes and keeps its arrays alive with the object.
    """
    def __init__(self, kind, wavelength=0., wavelengths=None, values=None, ref_index=1.):
        ref_index = float(ref_index)
        if not N.isfinite(ref_index) or not ref_index > 0.:
            raise ValueError("SourceSpectrum: ref_index must be finite and positive, got %r" % ref_index)
        self.kind = kind
        self.ref_index = ref_index
        self.wavelength = float(wavelength)
        self.wavelengths = self.values = None
        if kind == _cabi.SPECTRUM_CONSTANT:
            if not N.isfinite(self.wavelength):
                raise ValueError("SourceSpectrum: the wavelength must be finite")
        elif kind in (_cabi.SPECTRUM_TABLE, _cabi.SPECTRUM_CARRIED):
            wl = N.ascontiguousarray(N.ravel(N.asarray(wavelengths, dtype=float)))
            val = N.ascontiguousarray(N.ravel(N.asarray(values, dtype=float)))
            if wl.shape != val.shape:
                raise ValueError("SourceSpectrum: %d wavelengths but %d values" % (wl.size, val.size))
            if not 2 <= wl.size <= MAX_POINTS:
                raise ValueError("SourceSpectrum: a table has 2..%d points, got %d" % (MAX_POINTS, wl.size))
            if not N.all(N.isfinite(wl)) or not N.all(wl[1:] > wl[:-1]):
                raise ValueError("SourceSpectrum: the wavelengths must be finite and strictly increasing")
            if not N.all(N.isfinite(val)) or N.any(val < 0.):
                raise ValueError("SourceSpectrum: the values must be finite and non-negative")
            if not self.integral(wl, val) > 0.:
                raise ValueError("SourceSpectrum: the spectrum integrates to zero")
            self.wavelengths, self.values = wl, val
        else:
            raise ValueError("SourceSpectrum: unknown kind %r" % (kind,))
        self._desc = None

    # -- constructors ---------------------------------------------------------------------------------
    @classmethod
    def monochromatic(cls, wavelength, ref_index=1.):
        return cls(_cabi.SPECTRUM_CONSTANT, wavelength=wavelength, ref_index=ref_index)

    @classmethod
    def tabulated(cls, wavelengths, values, ref_index=1.):
        """spectral density `values` at `wavelengths`, linear in between, zero outside"""
        return cls(_cabi.SPECTRUM_TABLE, wavelengths=wavelengths, values=values, ref_index=ref_index)

    @classmethod
    def polychromatic(cls, wavelengths, values, ref_index=1.):
        """the table of `tabulated`, carried: every source ray brings all W points as its sample wavelengths and the spectrum
        energy_of_ray * table()[1] (its trapezoid integral is the ray's energy); the ray's scalar wavelength is 0"""
        return cls(_cabi.SPECTRUM_CARRIED, wavelengths=wavelengths, values=values, ref_index=ref_index)

    def as_polychromatic(self):
        """this tabulated spectrum (planck(...), uniform(...)), carried by every ray instead of sampled"""
        if not self.has_table():
            raise ValueError("SourceSpectrum.as_polychromatic: a monochromatic spectrum has no table to carry")
        return SourceSpectrum.polychromatic(self.wavelengths, self.values, self.ref_index)

    def has_table(self):
        return self.kind in (_cabi.SPECTRUM_TABLE, _cabi.SPECTRUM_CARRIED)

    def is_carried(self):
        """every ray carries the whole table (polychromatic) instead of one wavelength drawn from it"""
        return self.kind == _cabi.SPECTRUM_CARRIED

    @classmethod
    def uniform(cls, lo, hi, ref_index=1.):
        lo, hi = float(lo), float(hi)
        if not hi > lo:
            raise ValueError("SourceSpectrum.uniform: needs lo < hi")
        return cls.tabulated([lo, hi], [1., 1.], ref_index)

    @classmethod
    def planck(cls, T, band, step=1e-9, ref_index=1.):
        """
        Black body at T (K) within band = (lo, hi) (m), on the grid of the reference's
        spectral_band_axisymmetrical_thermal_emission_source (tracer/sources.py:788): linspace(lo, hi, int((hi - lo) / step)).
        """
        T = float(T)
        if not T > 0.:
            raise ValueError("SourceSpectrum.planck: T must be positive")
        lo, hi = float(band[0]), float(band[1])
        if not (hi > lo > 0.):
            raise ValueError("SourceSpectrum.planck: the band must be 0 < lo < hi")
        npts = int((hi - lo) / step)
        if npts > MAX_POINTS:
            raise ValueError("SourceSpectrum.planck: %d points on a step of %g m exceed %d: pass a larger step "
                             "(at least %g)" % (npts, step, MAX_POINTS, (hi - lo) / MAX_POINTS))
        if npts < 2:
            raise ValueError("SourceSpectrum.planck: the step leaves fewer than 2 points in the band: pass a smaller step")
        wls = N.linspace(lo, hi, npts)
        return cls.tabulated(wls, planck(wls, T), ref_index)

    # -- the packed table -------------------------------------------------------------------------------
    @staticmethod
    def integral(wl, val):
        return float(N.sum((wl[1:] - wl[:-1]) * (val[1:] + val[:-1]) / 2.))

    def table(self):
        """(wavelengths, density normalised to a unit trapezoid integral, its running integral): the table the device samples,
        packed as the library packs it (the running sum in order, divided by its last entry, which makes the CDF end at 1)."""
        if not self.has_table():
            raise ValueError("SourceSpectrum.table: a monochromatic spectrum has no table")
        wl, v = self.wavelengths, self.values
        cum = N.concatenate(([0.], N.cumsum((wl[1:] - wl[:-1]) * (v[1:] + v[:-1]) / 2.)))
        return wl.copy(), v / cum[-1], cum / cum[-1]

    def desc(self):
        """the trc_source_spectrum of this spectrum (valid while this object lives)"""
        if self._desc is None:
            d = _cabi.SourceSpectrumDesc()
            d.kind = self.kind
            d.ref_index = self.ref_index
            d.wavelength = self.wavelength
            if self.has_table():
                d.n = self.wavelengths.size
                d.wl = self.wavelengths.ctypes.data_as(C.POINTER(C.c_double))
                d.value = self.values.ctypes.data_as(C.POINTER(C.c_double))
            self._desc = d
        return self._desc

    def __repr__(self):
        if self.kind == _cabi.SPECTRUM_CONSTANT:
            return 'SourceSpectrum.monochromatic(%r, ref_index=%r)' % (self.wavelength, self.ref_index)
        return 'SourceSpectrum.%s(<%d points, %g..%g>, ref_index=%r)' % (
            'polychromatic' if self.is_carried() else 'tabulated', self.wavelengths.size, self.wavelengths[0], self.wavelengths[-1], self.ref_index)
