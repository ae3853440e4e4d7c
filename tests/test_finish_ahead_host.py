"""
Host test (no GPU) of trc_stream_form_ahead (csrc/trc_forms.h): the shading kernel k_s_shade_c<MIRROR, flat, LDS> finishes the next
segment of the continued rays inside their clear cones exactly when
  - the next bounce's search is k_s_bounce<1, .., FRESH = false> (the LDS-sized grid, TRC_STREAM_BOUNCE not 0),
  - that kernel finishes the hits on surfaces that end every ray itself (split_terminal == 2),
  - the scene has clear cones and TRC_STREAM_CLEAR is not 0,
  - no surface is without a box,
  - the mirrors' shading instance is <0, true, true, false, false>,
  - TRC_STREAM_AHEAD is not 0.
The fact blocks and the other decisions come through the host check's entry points (search_cases.library_decide); the three facts
those blocks do not name -- the cones and the two knobs -- come beside them (tests/aheadcheck/ahead_check.cpp).  For the facts of
every existing search, geometry and shading case, which name none of them, the path stays off.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

import ahead_cases as A
import clear_cases as K
import search_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNCE = 'k_s_bounce<1, true, false, true, false>'
SHADE = 'k_s_shade_c<0, true, true, false, false>'


@pytest.fixture(scope='module')
def lib():
    S.hostcheck()
    subprocess.check_call(['make', '-s', '-C', ROOT, 'aheadcheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'aheadcheck', 'libtrc_ahead_check.so'))
    p = C.POINTER(C.c_double)
    lib.ac_ahead.restype = C.c_int
    lib.ac_ahead.argtypes = [C.c_long, p, p, p]
    return lib


def ahead(lib, blocks, more=None):
    """per block (decided, the path is on); more: per block (clear cones, TRC_STREAM_CLEAR, TRC_STREAM_AHEAD), None: not named"""
    p = C.POINTER(C.c_double)
    rows = N.ascontiguousarray([[float(b[k]) for k in S.FACT_KEYS] for b in blocks])
    out = N.zeros((len(rows), 2))
    m = None if more is None else N.ascontiguousarray(more, dtype=float)
    assert m is None or m.shape == (len(rows), 3)
    assert lib.ac_ahead(len(rows), rows.ctypes.data_as(p), m.ctypes.data_as(p) if m is not None else None, out.ctypes.data_as(p)) == 2
    return [(bool(a), bool(b)) for a, b in out]


@pytest.fixture(scope='module')
def field():
    """the facts of a streaming call on forty heliostats of NSTTF and the receiver, with the bench's flux map, from its Buie source"""
    from tracer_amd import scenes
    cs, src = K.compiled(lambda: K.nsttf(40))
    desc = scenes.nsttf_source(10, src, seed=1).source_args()[0]
    f = S.scene_facts(cs, None, desc, {A.receiver_index(cs): A.fluxmap_edges(50)})
    f.update(n=1000000, flags=S.TRACE_ACCEL | S.TRACE_STREAM, src_kind=S.SRC_KIND['buie'], term_ok=1)
    return f


def test_on_for_an_aimed_field(lib, field):
    d = S.library_decide([field])[0]
    assert d['decided'] and d['use_fused'] and d['gridm'] == 1 and d['split_terminal'] == 2 and field['n_unbounded'] == 0, d
    assert d['bounce'][0] == BOUNCE and [k[0] for k in d['shk']] == [SHADE], (d['bounce'], d['shk'])
    assert ahead(lib, [field], [(1, 1, 1)]) == [(True, True)]
    # the cones and the knobs one by one, and a block that does not name them
    assert ahead(lib, [field] * 4, [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]) == [(True, False)] * 4
    assert ahead(lib, [field]) == [(True, False)]


# what takes one of the conditions away, with the decision of the header that shows it
OFF = [('a surface without a box', dict(n_unbounded=1), lambda d: True),
       ('terminal hits behind a list (TRC_STREAM_ABSORB=1)', dict(k_absorb=1), lambda d: d['split_terminal'] == 1),
       ('no list of terminal hits (TRC_STREAM_ABSORB=0)', dict(k_absorb=0), lambda d: d['split_terminal'] == 0),
       ('no surface ends every ray', dict(any_term=0), lambda d: d['split_terminal'] == 0),
       ('a ray of energy 0 goes on', dict(term_ok=0), lambda d: d['split_terminal'] == 0),
       ('continued rays through the general path (TRC_STREAM_BOUNCE=0)', dict(k_bounce=0), lambda d: not d['use_fused']),
       ('the Kd walk (TRC_STREAM_SEARCH=1)', dict(k_search=1, accel_kd_ok=1, has_kd=1, kd_nodes=15, kd_nleaf=41, kd_depth=4), lambda d: not d['use_fused']),
       ('no LDS-sized grid', dict(grid_ok=0, grid_cells=0, grid_list=0), lambda d: d['gridm'] != 1),
       ('a source with a spectrum', dict(spec=1), lambda d: d['shk'][0][0] == 'k_s_shade_c<0, true, true, true, false>'),
       ('a surface that is not flat', dict(all_flat=0, simple=0), lambda d: d['shk'][0][0] == 'k_s_shade_c<0, false, true, false, false>'),
       ('a flux map in another chart', dict(chart=1), lambda d: d['shk'][0][0] == 'k_s_shade_c<0, false, true, false, true>'),
       ('rays that carry more', dict(carry=1, src_kind=-1), lambda d: d['shk'][0][0].startswith('k_s_shade_x')),
       ('flux-map bins beyond LDS', dict(fm_bins=60000, n_fm_edges=502), lambda d: d['split_terminal'] != 2),
       ('no mirror among the surfaces that go on', dict(cls_moving=2, cls_all=3), lambda d: all('k_s_shade_c<0' not in k[0] for k in d['shk']))]


@pytest.mark.parametrize('what,change,shows', OFF, ids=[o[0] for o in OFF])
def test_off_without_a_condition(lib, field, what, change, shows):
    f = dict(field, **change)
    d = S.library_decide([f])[0]
    assert d['decided'] and shows(d), (what, d)
    assert ahead(lib, [f], [(1, 1, 1)]) == [(True, False)], what


def test_off_for_every_existing_case(lib):
    """the fact blocks of the existing cases name neither cones nor the new knob: the path is off for all of them, so the decisions
    their tests restate are the ones the library makes"""
    import geometry_cases as G
    import shade_cases as sc
    from test_shade_cases_host import case_facts
    blocks = [S.facts(c) for c in S.CALLS] + [G.facts(c) for c in G.CALLS]
    for name in sorted(sc.CASES):
        blocks += [case_facts(sc.case(name), given) for given in ((False, True) if name in sc.GIVEN else (False,))]
    res = ahead(lib, blocks)
    assert len(res) > 60 and any(d for d, _ in res), len(res)
    assert not any(on for _, on in res), [k for k, r in enumerate(res) if r[1]]
