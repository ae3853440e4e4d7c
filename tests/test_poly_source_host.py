"""
Polychromatic sources without a device: SourceSpectrum.polychromatic / as_polychromatic (validation, the packed descriptor, the birth
spectrum's integral), what call_plan.py decides for a pending bundle that carries its spectrum -- and that every other kind of
bundle is decided as before --, and what k_s_shade_p rests on in the headers: trc_interp2_at against trc_interp2 bit for bit, the
eight ids of the family, and the LDS decision for grid, birth vector and cells (tests/polycheck, a program of its own built with the
sanitizers).
"""
import os
import subprocess

import numpy as N
import pytest

import shade_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- SourceSpectrum ------------------------------------------------------------------------------------------------------------------
def test_polychromatic_spectrum():
    from tracer_amd import _cabi
    from tracer_amd.source_spectrum import SourceSpectrum
    wl = N.array([0.3e-6, 0.5e-6, 0.9e-6, 2.5e-6])
    val = N.array([0.2, 1.0, 0.7, 0.])
    s = SourceSpectrum.polychromatic(wl, val, ref_index=1.3)
    d = s.desc()
    assert _cabi.SPECTRUM_CARRIED == 3 and d.kind == _cabi.SPECTRUM_CARRIED and d.n == 4 and d.ref_index == 1.3 and d.wavelength == 0.
    assert [d.wl[i] for i in range(4)] == list(wl) and [d.value[i] for i in range(4)] == list(val)
    assert s.is_carried() and not SourceSpectrum.tabulated(wl, val).is_carried()
    # the same table as `tabulated` packs
    for a, b in zip(s.table(), SourceSpectrum.tabulated(wl, val).table()):
        assert N.array_equal(a, b)
    # the spectrum a ray of energy e is born with integrates to e
    for e in (1., 3.7e-4, 812.5):
        assert N.isclose(N.trapezoid(e * s.table()[1], s.table()[0]), e, rtol=1e-12, atol=0.)
    assert 'polychromatic' in repr(s)


def test_polychromatic_spectrum_validation():
    from tracer_amd.source_spectrum import SourceSpectrum, MAX_POINTS
    P = SourceSpectrum.polychromatic
    with pytest.raises(ValueError):
        P([1e-6], [1.])                                     # fewer than 2 points
    with pytest.raises(ValueError):
        P(N.linspace(1e-7, 1e-6, MAX_POINTS + 1), N.ones(MAX_POINTS + 1))
    with pytest.raises(ValueError):
        P([1e-6, 1e-6], [1., 1.])                           # not strictly increasing
    with pytest.raises(ValueError):
        P([1e-6, 2e-6, N.nan], [1., 1., 1.])
    with pytest.raises(ValueError):
        P([1e-6, 2e-6], [1., -1.])
    with pytest.raises(ValueError):
        P([1e-6, 2e-6], [1., N.inf])
    with pytest.raises(ValueError):
        P([1e-6, 2e-6], [0., 0.])                           # integrates to zero
    with pytest.raises(ValueError):
        P([1e-6, 2e-6], [1.], 1.)
    with pytest.raises(ValueError):
        P([1e-6, 2e-6], [1., 1.], ref_index=0.)
    assert P(N.linspace(1e-7, 1e-6, MAX_POINTS), N.ones(MAX_POINTS)).desc().n == MAX_POINTS


def test_as_polychromatic():
    from tracer_amd.source_spectrum import SourceSpectrum
    for s in (SourceSpectrum.planck(5777., (0.3e-6, 2.5e-6), 1e-7), SourceSpectrum.uniform(0.4e-6, 0.7e-6, ref_index=1.2)):
        p = s.as_polychromatic()
        assert p.is_carried() and not s.is_carried() and p.ref_index == s.ref_index
        for a, b in zip(p.table(), s.table()):
            assert N.array_equal(a, b)
        assert p.as_polychromatic().is_carried()
    with pytest.raises(ValueError):
        SourceSpectrum.monochromatic(0.5e-6).as_polychromatic()


def test_sources_take_a_carried_spectrum():
    """the bundle stays pending, and says what its materialised columns will be"""
    from tracer_amd import sources
    from tracer_amd.source_spectrum import SourceSpectrum
    s = SourceSpectrum.polychromatic([0.3e-6, 1e-6, 2e-6], [1., 2., 1.])
    b = sources.rect_bundle(100, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 1., 1., 0.1, flux=1., seed=1, spectrum=s)
    assert b.is_pending() and b.source_spectrum() is s and b.spectral_columns() == ('wavelengths', 'spectra', 'ref_index')
    assert b.has_property('spectra') and b.has_property('wavelengths') and b.is_pending()


# -- call_plan -----------------------------------------------------------------------------------------------------------------------
class Lim(object):
    SPLIT_ON_FAST = True
    KD_BUILD_MAX = 8192
    KD_WORTH_IT = 2e9
    TUNE_MIN_RAYS = 1 << 21
    TUNE_MAX_SURFACES = 512
    SLOW_STREAM = 1.5e6


class Spec(object):
    def __init__(self, carried):
        self.carried = carried

    def is_carried(self):
        return self.carried


def _rays(n, carried=True):
    from tracer_amd.call_plan import Rays
    return Rays(n, True, carried, False, Spec(carried), ('wavelengths', 'spectra', 'ref_index') if carried else ('wavelengths', 'ref_index'))


def _scene(splits=False, capture=False, carries=True, materials=False, on_device=False):
    from tracer_amd.call_plan import Scene
    return Scene(5, carries, splits, capture, materials, on_device)


def test_ray_facts_of_a_pending_carried_bundle():
    from tracer_amd import call_plan, sources
    from tracer_amd.source_spectrum import SourceSpectrum
    mk = lambda s: sources.rect_bundle(100, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 1., 1., 0.1, flux=1., seed=1, spectrum=s)
    b = mk(SourceSpectrum.polychromatic([0.3e-6, 1e-6], [1., 2.]))
    r = call_plan.ray_facts(b)
    assert (r.n, r.pending, r.polychromatic, r.complex_index) == (100, True, True, False) and call_plan.carried(r) and b.is_pending()
    r = call_plan.ray_facts(mk(SourceSpectrum.tabulated([0.3e-6, 1e-6], [1., 2.])))
    assert (r.pending, r.polychromatic) == (True, False) and not call_plan.carried(r)
    r = call_plan.ray_facts(mk(None))
    assert (r.pending, r.polychromatic, r.spectrum) == (True, False, None) and not call_plan.carried(r)


def test_engine_of_a_pending_carried_bundle():
    from tracer_amd import call_plan as cp
    L = Lim()
    for splits in (False, True):
        sc = _scene(splits=splits)
        assert cp.choose_engine(L, _rays(64), sc, False) == 'fast'
        assert cp.choose_engine(L, _rays(63), sc, False) == 'ordered'
        assert cp.choose_engine(L, _rays(4096), sc, True) == 'ordered'
        assert cp.choose_engine(L, _rays(63), sc, True) == 'ordered'
    # the streaming form, whatever fast_kernel='auto' would pick by size
    assert cp.fast_form(L, _rays(64), _scene(), 'auto', False, {}) == (True, False)
    assert cp.fast_form(L, _rays(1 << 22), _scene(), 'auto', False, {}) == (True, False)
    assert cp.fast_form(L, _rays(64), _scene(), 'megakernel', False, {})[0] is False          # (the library refuses it)
    # its hits have spectral columns: the buffer does not go on filling
    assert cp.may_keep_hits(_rays(64), _scene(capture=True), True, None, True) is False
    assert cp.last_room(64, False) == 64 and cp.last_room(64, True) == 2 * 64 + 1024 and cp.last_room(293, False, 1000) == 293


def test_other_bundles_are_decided_as_before():
    """the decisions of the parent commit, spelled out: given bundles, pending sources without a spectrum and with one that is drawn"""
    from tracer_amd import call_plan as cp
    from tracer_amd.call_plan import Rays
    L = Lim()
    plain = lambda n: Rays(n, True, False, False, None, ())
    drawn = lambda n: _rays(n, carried=False)
    given = lambda n, poly=False, cplx=False: Rays(n, False, poly, cplx, None, ())
    bare, carry, split = _scene(carries=False), _scene(), _scene(carries=False, splits=True)
    cases = [
        (plain(1000), bare, False, 'fast'), (plain(1000), bare, True, 'ordered'), (plain(10), bare, False, 'fast'),
        (plain(1000), carry, False, 'ordered'), (plain(1000), split, False, 'fast'), (plain(63), split, False, 'ordered'),
        (drawn(1000), bare, False, 'fast'), (drawn(1000), carry, False, 'ordered'), (drawn(1000), split, False, 'ordered'),
        (drawn(1000), _scene(materials=True, on_device=True), False, 'fast'), (drawn(63), _scene(materials=True, on_device=True), False, 'ordered'),
        (drawn(1000), _scene(carries=False, splits=True, materials=True, on_device=True), False, 'fast'),
        (given(1000), bare, False, 'fast'), (given(1000, poly=True), bare, False, 'fast'), (given(63, poly=True), bare, False, 'ordered'),
        (given(1000, cplx=True), bare, False, 'fast'), (given(1000), carry, False, 'fast'), (given(63), carry, False, 'ordered'),
        (given(1000, poly=True), split, False, 'fast'), (given(1000, poly=True), bare, True, 'ordered'),
    ]
    for rays, scene, tree, want in cases:
        assert cp.choose_engine(L, rays, scene, tree) == want, (rays, scene, tree)
    assert cp.fast_form(L, plain(1000), bare, 'auto', False, {}) == (None, False)
    assert cp.fast_form(L, drawn(1000), bare, 'auto', False, {}) == (None, False)
    assert cp.fast_form(L, given(1000, poly=True), bare, 'auto', False, {}) == (None, False)
    assert cp.fast_form(L, plain(1000), split, 'auto', False, {}) == (True, False)
    assert cp.fast_form(L, plain(1 << 21), bare, 'auto', False, {}) == (None, True)
    assert cp.may_keep_hits(plain(1000), _scene(capture=True), True, None, True) is True
    assert cp.may_keep_hits(drawn(1000), _scene(capture=True), True, None, True) is True
    assert cp.may_keep_hits(given(1000, poly=True), _scene(capture=True), True, None, True) is False
    assert cp.may_keep_hits(plain(1000), _scene(capture=True, splits=True), True, None, True) is False


# -- the headers: trc_interp2_at, the family's ids, the LDS decision -------------------------------------------------------------------
def _facts(kind, table_len, W, walls=1, splits=0, mat_dev=0, chart=0, bins=0):
    """the eleven integers poly_check takes for a room of shade_cases.py"""
    from tracer_amd.scene import compile_scene
    cs = compile_scene(shade_cases.room(kind, 0, table_len)[0])
    return [cs.n_surf, shade_cases.record_stride(cs), 0, 0, len(cs.extra), bins, chart, splits, W, walls, mat_dev]


@pytest.fixture(scope='module')
def polycheck():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'polycheck'])

    def run(*blocks):
        args = [str(v) for b in blocks for v in b]
        p = subprocess.run([os.path.join(ROOT, 'tests', 'polycheck', 'poly_check')] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True)
        assert p.returncode == 0, p.stdout          # (the sanitizers end the program with a report and a status)
        return p.stdout.splitlines()
    return run


def test_interp2_at_equals_interp2_bit_for_bit(polycheck):
    lines = [l.split() for l in polycheck() if l.startswith('interp')]
    assert [(int(l[1]), int(l[2])) for l in lines] == [(2, 2), (3, 5), (64, 64)]
    for l in lines:
        assert int(l[3]) == 100000 and int(l[4]) == 0, l


def test_header_holds_the_eight_instances(polycheck):
    ids = sorted(l[3:] for l in polycheck() if l.startswith('id '))
    t = ('false', 'true')
    assert ids == sorted('k_s_shade_p<%s, %s, %s>' % (a, b, c) for a in t for b in t for c in t)


def test_kernel_choice(polycheck):
    KiB = 1024
    x_lds, x_global = _facts('carry', 12, 17), _facts('carry', 4500, 4096)
    small = _facts('carry', 12, 17)
    out = [l for l in polycheck(
        x_lds,                                      # everything fits: the LDS instance with the wall's cells
        x_global,                                   # the long optics table and the longest grid: the global instance
        _facts('carry', 12, 4096),                  # the longest grid beside small tables: 64 KiB + the image still fit 72 KiB
        _facts('carry', 2300, 4096),                # tables that fit on their own (36 KiB) but not with the grid: all global
        _facts('carry', 12, 17, splits=1, chart=1),
        _facts('carry', 12, 0, splits=1),           # poly_src off: k_s_shade_x, whatever else the call carries
        _facts('carry', 12, 0, walls=0, mat_dev=1),
        _facts('carry', 4500, 0, splits=1, chart=1),
        _facts('carry', 12, 17, mat_dev=1),         # no MAT instance of k_s_shade_p
    ) if l.startswith('choose')]
    name = lambda l: l.split(' | ')[0][len('choose '):]
    nums = lambda l: [int(v) for v in l.split(' | ')[1].split()]
    assert [name(l) for l in out[:8]] == [
        'k_s_shade_p<true, false, false>', 'k_s_shade_p<false, false, false>', 'k_s_shade_p<true, false, false>',
        'k_s_shade_p<false, false, false>', 'k_s_shade_p<true, true, true>', 'k_s_shade_x<true, false, true, false>',
        'k_s_shade_x<true, false, false, true>', 'k_s_shade_x<false, true, true, false>']
    assert out[8] == 'choose none'
    # the bytes: the image of k_s_shade_x, 16 W for grid and birth vector, and per wall and sample a weight and a cell, a word per surface
    S, W = small[0], 17
    base = nums([l for l in polycheck(_facts('carry', 12, 0, splits=1)) if l.startswith('choose')][0])[0]
    lds, tables, bins, cells = nums(out[0])
    assert (tables, bins, cells) == (1, 0, 1) and lds == base + 16 * W + W * 8 + ((W + 1) // 2) * 8 + ((S + 1) // 2) * 8
    assert nums(out[1]) == [16, 0, 0, 0]            # nothing staged: the two count words
    lds, tables, bins, cells = nums(out[2])
    assert (tables, cells) == (1, 0) and base + 16 * 4096 == lds <= 72 * KiB       # (the cells of 4096 samples no longer fit)
    assert nums(out[3]) == [16, 0, 0, 0]


def test_library_holds_the_eight_instances():
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    if not os.path.exists(lib):
        pytest.skip('the library is not built')
    names = subprocess.run(['nm', '-C', lib], stdout=subprocess.PIPE, universal_newlines=True).stdout
    t = ('false', 'true')
    for a in t:
        for b in t:
            for c in t:
                assert 'void k_s_shade_p<%s, %s, %s>(StreamParams)' % (a, b, c) in names
    assert 'k_source_carried' in names
