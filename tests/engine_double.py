"""
A device double for TracerEngine: what the engine uses of scene.DeviceScene, without ctypes and without the library.

Double appends every call it gets, with its arguments, to `log`, and answers trace_fast / trace_ordered from a script the test
gives it (one dict per call: stats fields, `last` = how many rays are left or None for "no room", `gained` = entries the hit buffer
gains, `tally` = hits added per surface).  The scene (Compiled) and the rays (Bundle) are plain numbers, so that every threshold of
a call's plan is reached with tiny arrays.  tests/test_call_plan_host.py drives TracerEngine.ray_tracer with it.
"""
import numpy as N


class Acc(object):
    """an accountant as deferred.Delivery sees it: a list of chunks and marks; reset() drops them"""
    def __init__(self):
        self._data = []

    def reset(self):
        self._data = []


class Optic(object):
    def __init__(self, accountants):
        self.accountants = list(accountants)


class Compiled(object):
    """what the engine reads of scene.CompiledScene"""
    def __init__(self, n_surf=2, capture=(), accountants=(), carries=False, splits=False, materials=(), material_tables=None):
        self.n_surf = n_surf
        self.capture = [i in capture for i in range(n_surf)]
        self.capturing_optics = [Optic(accountants)] if capture else []
        self.carries = carries
        self.splits = splits
        self.materials = list(materials)
        self.material_tables = material_tables
        self.surfaces = []
        self.optics = []
        self.descs = []


class Bundle(object):
    """a ray bundle of `n` rays that holds none: given, or (pending=True) a source still described by its generator"""
    def __init__(self, n, pending=False, polychromatic=False, complex_index=False, spectrum=None, spectral_columns=()):
        self.n, self.pending, self.polychromatic, self.complex_index = n, pending, polychromatic, complex_index
        self.spectrum, self.columns = spectrum, tuple(spectral_columns)

    def get_num_rays(self):
        return self.n

    def is_pending(self):
        return self.pending

    def is_polychromatic(self):
        return self.polychromatic

    def has_complex_index(self):
        return self.complex_index

    def source_spectrum(self):
        return self.spectrum

    def spectral_columns(self):
        return self.columns

    def _has_column(self, name):
        return (name == 'spectra' and self.polychromatic) or (name == 'ref_index' and self.complex_index)

    def get_spectra(self):
        return N.zeros((3, 0))

    def get_energy(self):
        return N.ones(1)


class Stats(object):
    """the fields of _cabi.TraceStats the engine reads"""
    def __init__(self, **fields):
        self.segments = self.hits = self.rays_left = self.bounces = self.hits_dropped = 0
        self.energy_left = self.kernel_ms = 0.
        self.launches = 1
        self.__dict__.update(fields)


class Levels(object):
    """the trc_result of an ordered trace: level sizes only, or level 0 alone (a depleted bundle)"""
    def __init__(self, sizes):
        self.sizes = list(sizes)

    def num_levels(self):
        return len(self.sizes)

    def level_size(self, lv):
        return self.sizes[lv]

    def level(self, lv, **kw):
        n, live = self.sizes[lv]
        return dict(vertices=N.zeros((3, n)), directions=N.zeros((3, n)), n_live=live)

    def close(self):
        pass


class _Lib(object):
    def __init__(self, dev):
        self._dev = dev

    def trc_scene_clear_hits(self, handle):
        self._dev.log.append(('clear_hits',))
        self._dev.reserved = 0


class Double(object):
    def __init__(self, compiled, script=()):
        self.compiled = compiled
        self.n_surf = compiled.n_surf
        self.hit_capacity = 0
        self.capture_rate = None
        self.form_rate = {}
        self.pending_hits = None
        self.handle = object()
        self.lib = _Lib(self)
        self.log = []
        self.script = list(script)
        self.reserved = 0               # entries of the hit buffer reserved so far
        self.spectral = 0               # spectral columns per hit the buffer holds
        self.on_device = False          # materials_on_device()
        self.hit_tally = N.zeros(self.n_surf, dtype=N.int64)
        self._exports = 0

    def named(self, *names):
        """the recorded calls of these names, in order"""
        return [c for c in self.log if c[0] in names]

    # -- queries ----------------------------------------------------------------------------------
    def hits_reserved(self):
        self.log.append(('hits_reserved',))
        return self.reserved, self.hit_capacity

    def hit_spectral_columns(self):
        self.log.append(('hit_spectral_columns',))
        return self.spectral

    def materials_on_device(self):
        self.log.append(('materials_on_device',))
        return self.on_device

    def get_tallies(self):
        self.log.append(('get_tallies',))
        return N.zeros(self.n_surf), N.zeros(self.n_surf), self.hit_tally.copy()

    def get_hits(self):
        """(what scene.PendingHits fetches when a read or an emptied buffer settles it: the double holds no hits)"""
        return dict(surf=N.zeros(0, dtype=N.int32), e_abs=N.zeros(0), e_in=N.zeros(0), points=N.zeros((3, 0)), directions=None)

    # -- the hit buffer -----------------------------------------------------------------------------
    def _settle(self):
        p, self.pending_hits = self.pending_hits, None
        if p is not None:
            p.settle()

    def settle_pending(self):
        self.log.append(('settle_pending',))
        self._settle()

    def set_hit_capacity(self, capacity):
        self.log.append(('set_hit_capacity', capacity))
        self._settle()
        self.hit_capacity = int(capacity)

    def reserve_hits(self, capacity):
        self.log.append(('reserve_hits', capacity))
        self.hit_capacity = max(self.hit_capacity, int(capacity))

    def export_tallies(self):
        self._exports += 1
        self.log.append(('export_tallies', self._exports))
        return N.array([float(self._exports)])

    def import_tallies(self, src):
        self.log.append(('import_tallies', int(src[0])))

    def set_kdtree(self, tree):
        self.log.append(('set_kdtree', tree))

    # -- tracing ------------------------------------------------------------------------------------
    def _next(self):
        s = dict(self.script.pop(0)) if self.script else {}
        last, gained, tally = s.pop('last', 0), s.pop('gained', 0), s.pop('tally', None)
        self.reserved += gained
        if tally is not None:
            self.hit_tally += N.asarray(tally, dtype=N.int64)
        return Stats(**s), last

    def trace_fast(self, bundle, reps, min_energy, seed, accel=False, keep_last=False, stream=None, last_capacity=None, short_last_ok=False):
        n = bundle.get_num_rays()
        # rows the library is given for the last rays (DeviceScene.trace_fast): at most one ray left per ray given, unless the
        # optics split rays
        rows = n if last_capacity is None else max(1, int(last_capacity) if self.compiled.splits else min(int(last_capacity), n))
        self.log.append(('trace_fast', dict(n=n, reps=reps, min_energy=min_energy, seed=seed, accel=accel, keep_last=keep_last, stream=stream,
                                            last_capacity=last_capacity, short_last_ok=short_last_ok, rows=rows)))
        stats, last = self._next()
        if last is None:
            assert short_last_ok, "the script leaves more rays than the call has room for, and the call does not take that"
            return stats, None
        return stats, [N.zeros(min(last, rows)) for _ in range(7)]

    def trace_ordered(self, bundle, reps, min_energy, seed, accel=False):
        self.log.append(('trace_ordered', dict(n=bundle.get_num_rays(), reps=reps, min_energy=min_energy, seed=seed, accel=accel)))
        stats, last = self._next()
        return Levels([(bundle.get_num_rays(), 0)] + ([(last, last)] if last else [])), stats
