"""
What csrc/trc_forms.h decides for the arc-lamp source kinds, from the host-compiled header (tests/hostcheck/lamp_check.cpp), without a
device: no footprint path, fresh rays through the general path by a generation kernel with the kind compiled in, a megakernel
instance that knows the lamps, every id one the library holds -- and, for every kind there was before them, the ids the existing case
tables expect.

The lamp kinds have kernels of their own names -- k_s_gen_lamp<KIND> (k_s_gen<true, KIND>'s body) and k_lamp_coop / k_lamp_fast<THREADS,
SPEC, CHART> (the megakernel's text) -- and not further instances of k_s_gen and k_trace_*: test_search_cases_host.py and
test_mega_cases_host.py hold those families, in the header and in the built library, to exactly the instances they had.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import search_cases as S

ROOT = S.ROOT
ARC, SPHERE, CYLINDER = 9, 10, 11
LAMPS = (ARC, SPHERE, CYLINDER)
OLD = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8)
TRACE_ACCEL, TRACE_STREAM, TRACE_MEGAKERNEL = S.TRACE_ACCEL, S.TRACE_STREAM, 8
_t = lambda b: 'true' if b else 'false'


@pytest.fixture(scope='module')
def hl():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_lamp_check.so'))
    lib.hl_decide.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int] + \
        [C.POINTER(C.c_int)] * 3
    return lib


def decide(hl, kind, n_surf=3, n=200000, flags=TRACE_ACCEL, spec=0, walk_ok=1):
    bufs = [C.create_string_buffer(96) for _ in range(3)]
    ints = [C.c_int() for _ in range(3)]
    use_stream = hl.hl_decide(kind, n_surf, n, flags, spec, walk_ok, bufs[0], bufs[1], bufs[2], 96, *[C.byref(i) for i in ints])
    return dict(use_stream=bool(use_stream), mega=bufs[0].value.decode(), gen0=bufs[1].value.decode(), first=bufs[2].value.decode(),
                has_map=bool(ints[0].value), use_first=ints[1].value, valid=bool(ints[2].value))


def test_trace_flags_are_the_headers():
    import tracer_amd._cabi as _cabi
    assert (TRACE_ACCEL, TRACE_STREAM, TRACE_MEGAKERNEL) == (_cabi.TRACE_ACCEL, _cabi.TRACE_STREAM, _cabi.TRACE_MEGAKERNEL)


@pytest.mark.parametrize('kind', LAMPS)
@pytest.mark.parametrize('n_surf', [3, 20, 200])       # surface by surface, a small scene, one on the grid
def test_a_lamp_takes_the_general_path_and_its_own_megakernel(hl, kind, n_surf):
    for spec in (0, 1):
        d = decide(hl, kind, n_surf=n_surf, spec=spec)
        assert not d['has_map']                         # no source plane: no footprint path
        assert d['gen0'] == 'k_s_gen_lamp<%d>' % kind   # the kind compiled in: k_s_gen<true, KIND>'s body
        assert d['use_first'] == 0                      # never k_s_bounce<.., FRESH>, which does not know the kinds
        assert d['mega'] == 'k_lamp_coop<512, %s, false>' % _t(spec)
        assert d['valid']
    # the engine: the megakernel below 2^20 rays and whenever asked; the streaming form from 64 rays on when asked, and by itself
    # from 2^20; never below 64
    assert not decide(hl, kind, n_surf=n_surf, n=200000)['use_stream']
    assert not decide(hl, kind, n_surf=n_surf, n=50, flags=TRACE_ACCEL | TRACE_STREAM)['use_stream']
    assert decide(hl, kind, n_surf=n_surf, n=64, flags=TRACE_ACCEL | TRACE_STREAM)['use_stream']
    assert decide(hl, kind, n_surf=n_surf, n=1 << 20)['use_stream']
    assert not decide(hl, kind, n_surf=n_surf, n=1 << 20, flags=TRACE_ACCEL | TRACE_MEGAKERNEL)['use_stream']


@pytest.mark.parametrize('kind', LAMPS)
def test_a_scene_without_a_general_path_gives_a_lamp_to_the_megakernel(hl, kind):
    """the large grid: fresh rays of the other kinds go through k_s_bounce<.., FRESH> there; a lamp's call runs the megakernel"""
    assert decide(hl, 5, n_surf=200, n=1 << 20, walk_ok=0)['use_stream']
    assert decide(hl, 5, n_surf=200, n=1 << 20, walk_ok=0)['use_first'] == 1
    for flags in (TRACE_ACCEL, TRACE_ACCEL | TRACE_STREAM):
        assert not decide(hl, kind, n_surf=200, n=1 << 20, flags=flags, walk_ok=0)['use_stream']


@pytest.mark.parametrize('kind', OLD)
def test_every_kind_of_before_keeps_its_ids(hl, kind):
    """the megakernel's instance and gen0 as mega_cases.py / search_cases.py restate them"""
    gen0 = {2: 'k_s_gen_src<2>', 3: 'k_s_gen<true, 3>', 0: 'k_s_gen_src<0>', 1: 'k_s_gen_src<1>', 7: 'k_s_gen<true, 7>',
            8: 'k_s_gen<true, 8>'}.get(kind, 'k_s_gen<true, -1>')
    for spec in (0, 1) if kind >= 0 else (0,):
        for n_surf in (3, 200):
            d = decide(hl, kind, n_surf=n_surf, spec=spec)
            assert d['mega'] == 'k_trace_coop<512, %s, %s, false>' % (_t(spec), _t(kind in (7, 8)))
            assert d['gen0'] == gen0 and d['valid']
            assert d['has_map'] == (kind in (0, 1, 2, 3, 7, 8))
            assert d['use_first'] == (1 if n_surf == 3 else 0)
            if d['use_first']:
                assert d['first'] == 'k_s_bounce<3, false, true, false, %s>' % _t(kind in (7, 8))


def test_the_header_holds_the_lamp_ids_and_no_other_new_one():
    names = S.library_ids(ints=(-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 128, 256, 512, 1024))
    lamp = sorted(n for n in names if n.split('<')[0] in ('k_s_gen_lamp', 'k_lamp_coop', 'k_lamp_fast'))
    assert lamp == sorted(['k_s_gen_lamp<%d>' % k for k in LAMPS] +
                          ['k_lamp_coop<%d, %s, %s>' % (t, _t(s), _t(c)) for t in (512, 256) for s in (0, 1) for c in (0, 1)] +
                          ['k_lamp_fast<256, %s, %s>' % (_t(s), _t(c)) for s in (0, 1) for c in (0, 1)])
    # no instance of the other families names a lamp kind
    assert not [n for n in names if n not in lamp and re.search(r'[<, ](9|10|11)[,>]', n)]
    assert sorted(n for n in names if n.split('<')[0] in S.FAMILIES) == sorted(S.ALL_INSTANCES)


def test_library_holds_the_lamp_kernels_by_name():
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    if not os.path.exists(lib) or shutil.which('nm') is None:
        pytest.skip('no built library, or no nm')
    squeeze = lambda x: re.sub(r'\s+', '', x)
    held = set()
    for line in subprocess.check_output(['nm', '-C', lib]).decode().splitlines():
        m = re.search(r'\b(k_s_gen_lamp|k_lamp_coop|k_lamp_fast)(<[^>]*>)\((StreamParams|FastParams)\)', line)
        if m and '__device_stub__' not in line:
            held.add(squeeze(m.group(1) + m.group(2)))
    want = ['k_s_gen_lamp<%d>' % k for k in LAMPS] + ['k_lamp_coop<%d, %s, %s>' % (t, _t(s), _t(c)) for t in (512, 256) for s in (0, 1) for c in (0, 1)] + \
        ['k_lamp_fast<256, %s, %s>' % (_t(s), _t(c)) for s in (0, 1) for c in (0, 1)]
    assert held == set(squeeze(w) for w in want), sorted(held ^ set(squeeze(w) for w in want))
