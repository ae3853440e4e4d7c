"""
What the tests of the shading kernel instances (test_gpu_shade_instances.py) take for granted about their cases, checked without
a device from the oracle and the restated sums of trc_stream_form_shade alone (shade_cases.py): every case is predicted to select
the instances it is there for, with its byte sum on the intended side of the limit; its rays hit every optics kind of its classes,
its curved surfaces, its captured surfaces inside and outside the map; some rays are culled on the way and some survive; and no
ray is near a tie -- two surfaces at nearly the same distance, an energy nearly at min_energy -- so that the device tests exclude
no ray at all.  Which instances ran on a device is recorded in profiles/shade_instances.txt.

The sums themselves are held to the library: trc_shade_lds_layout (csrc/trc_bounds.h), the one description of the LDS image the
kernels carve from and the host sizes launches by, exported by the host-compiled check library, must give the restated sums of
shade_cases.py to the byte -- for the cases, and for random scenes on both sides of every limit.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as N
import pytest

import shade_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hostcheck():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'hostcheck'])          # (the wavelength sampler of the SPEC cases, the LDS layout)
    return C.CDLL(os.path.join(ROOT, 'tests', 'hostcheck', 'libtrc_hostcheck.so'))


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_case_selects_its_instances_and_exercises_them(hostcheck, name):
    c = sc.case(name)
    o = sc.reference(name)
    opt, gm = sc._names('OPT_'), sc._names('GM_')
    # the prediction: the case's targets among what trc_stream_form_shade would launch, each on its side of its limit
    for inst in c.targets:
        assert inst in c.instances, (inst, sorted(c.instances))
        total, limit, in_lds, bins_in_lds = c.instances[inst]
        print('%s: %s sums %d bytes against %d: tables %s, bins %s' % (name, inst, total, limit, 'in LDS' if in_lds else 'global',
                                                                      'in LDS' if bins_in_lds else 'global'))
        assert in_lds == (total <= limit) and in_lds == ('global' not in name) and bins_in_lds == in_lds
    # every optics kind listed for the case is hit at least 30 times; curved surfaces take more than a tenth of the hits
    by_kind = {}
    for i in range(c.cs.n_surf):
        k = opt[c.cs.descs[i].optics_kind]
        by_kind[k] = by_kind.get(k, 0) + int(o['hits'][i])
    for k in sc.KINDS_HIT[c.kind]:
        assert by_kind.get(k, 0) >= 30, (k, by_kind)
    if c.kind in ('simple', 'general'):          # the general class of the case: the surfaces with an incidence-angle modifier / the panes
        general = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_GENERAL]
        assert len(general) == 2 and all(o['hits'][i] >= 30 for i in general)
    flat = all(gm[c.cs.descs[i].gm_kind] in sc.FLAT_KINDS for i in range(c.cs.n_surf))
    assert flat == (c.kind not in ('curved', 'general'))
    if not flat:
        curved = sum(int(o['hits'][i]) for i in range(c.cs.n_surf) if gm[c.cs.descs[i].gm_kind] in sc.CURVED_GM)
        assert curved > 0.1 * o['hits'].sum() and all(o['hits'][i] >= 30 for i in range(c.cs.n_surf) if gm[c.cs.descs[i].gm_kind] in sc.CURVED_GM)
    if c.n_fill:        # the fillers are hit through the gaps of the floor, a few hits each: sums added per lane
        assert (o['hits'][:c.n_fill] > 0).sum() > 100 and o['hits'][:c.n_fill].max() < 16
    # survivors, and rays culled before the last repetition
    assert len(o['levels']) == sc.REPS + 1 and o['last_energy'].size > 50
    assert sum(L['vertices'].shape[1] - L['n_live'] for L in o['levels'][1:-1]) > 50
    # the captured surfaces: the mapped tile inside and outside its map, the wall captured in full
    H, e_out, n_out, n_hits = o['maps'][c.map_surf]
    assert n_hits == o['hits'][c.map_surf] and 30 <= n_out <= n_hits - 30 and (H > 0).mean() > 0.3
    assert N.isclose(H.sum() + e_out, o['absorbed'][c.map_surf], rtol=1e-12)
    assert o['hits'][c.full_surf] > 300
    for f in c.frames[c.n_fill:]:       # no frame of the room is axis aligned
        assert (N.abs(f[:3, :3]) > 1e-3).sum() >= 8
    # SPEC: rays that meet the mirror class first and a wavelength-reading surface second, and rays that meet one first
    if c.spec:
        reads = [i for i in range(c.cs.n_surf) if opt[c.cs.descs[i].optics_kind] in ('OPT_REFLECTIVE_SPECTRAL', 'OPT_FRESNEL_CONDUCTOR')]
        mirror = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_MIRROR]
        L1, L2 = o['levels'][1], o['levels'][2]
        if c.kind != 'simple':
            assert N.isin(L1['surf'], reads).sum() > 100
            assert (N.isin(L2['surf'], reads) & N.isin(L1['surf'][L2['parents']], mirror)).sum() > 100
        if c.kind == 'general':     # ... and rays that meet a pane of the general class first: the wavelength k_s_shade hands on is read
            panes = [i for i in range(c.cs.n_surf) if sc.shade_class_of(c.cs.descs[i]) == sc.CLS_GENERAL]
            assert (N.isin(L2['surf'], reads) & N.isin(L1['surf'][L2['parents']], panes)).sum() > 50
    if c.carry:         # the periodic pane moves rays that go on and survive: the shift is in what the device is compared with
        periodic = [i for i in range(c.cs.n_surf) if opt[c.cs.descs[i].optics_kind] == 'OPT_PERIODIC_BOUNDARY']
        last = o['levels'][-1]
        assert o['hits'][periodic[0]] > 300 and (N.isin(last['surf'][:last['n_live']], periodic)).sum() >= 5        # (each survivor is compared on its own: a handful is enough)
    # no near tie: the cap on rays a device test may exclude is zero, and the reference stays within it
    gap, e_gap = sc.near_ties(name)
    print('%s: smallest gap between nearest and second-nearest surface %.3g, of an energy from min_energy %.3g (relative)' % (name, gap, e_gap))
    assert gap > 1e-9 and e_gap > 1e-9


def test_cases_cover_every_instance_that_can_be_selected():
    """26 instances; every one is the target of a case"""
    targets = set(t for v in sc.CASES.values() for t in v[5])
    assert len(sc.ALL_INSTANCES) == 26 and targets == set(sc.ALL_INSTANCES)
    assert set(sc.GIVEN) <= set(sc.CASES) and all(not sc.CASES[n][3] and not sc.CASES[n][4] for n in sc.GIVEN)


# -- the library's description of the LDS image against the restated sums ----------------------------------------------------------
# enum trc_shade_img (csrc/trc_bounds.h)
IMG_SHADE, IMG_SHADE_X, IMG_LEAN, IMG_LEAN_MIRROR, IMG_ABSORB, IMG_INLINE = range(6)
PARTS = ('tally', 'recs', 'opt', 'fm_edges', 'fms', 'fm_of', 'flags', 'extra', 'bins')
END, SLACK, LIMIT, LIMIT_BINS, IN_LDS, BINS_IN, REQUEST = 9, 10, 11, 12, 13, 14, 15
# what a launch of each image asks for when nothing is staged: the count words (k_s_shade keeps one)
BARE = {IMG_SHADE: 8, IMG_SHADE_X: 16, IMG_LEAN: 16, IMG_LEAN_MIRROR: 16}
INLINE_MARGIN = 64          # trc_stream_form_absorb, as it was: `extra_lds = lds_absorb + 64`
LIMIT_ABSORB, LIMIT_INLINE = 78 * sc.KiB, 158 * sc.KiB         # ... `lds_absorb <= 78 * 1024`, `F.bounce.lds + extra_lds <= 158 * 1024`


def lds_layout(hc, rows):
    """trc_shade_lds_layout of rows (image, tables staged, surfaces, record stride, map edges, descriptor bytes, table doubles, bins in
    LDS): (n, 16) -- the offsets of PARTS, end, slack, the two limits of the image, and what the host's own decision
    (trc_shade_lds_choose, the code trc_stream_form_shade calls) makes of a scene with that many bins: tables in LDS, bins in LDS, the bytes
    its launch asks for"""
    rows = N.ascontiguousarray(rows, dtype=N.int32).reshape(-1, 8)
    out = N.zeros((len(rows), 16), dtype=N.uint64)
    hc.hc_shade_lds_layout.argtypes = [C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
    assert hc.hc_shade_lds_layout(len(rows), rows.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_ulonglong))) == 0
    return out.astype(N.int64)


def check_images(hc, S, stride, n_edges, n_maps, n_extra, bins, old):
    """
    The library's images of scenes (arrays, one entry per scene) against the sums `old` = (tallies, records, optics parameters, maps)
    of shade_cases.table_bytes.  Returns per image the old sum without bins, for the caller to count the scenes near each limit.
    """
    n = len(S)
    fms = n_maps * sc.SIZEOF_FLUXMAPDEV
    t, r, o, m = [N.asarray(a, dtype=N.int64) for a in old]
    rows = lambda img, lds, b: N.stack([N.full(n, img), N.full(n, 1) * lds, S, stride, n_edges, fms, n_extra, b], axis=1)
    sums = {}
    for img in (IMG_SHADE, IMG_SHADE_X, IMG_LEAN, IMG_LEAN_MIRROR):
        # trc_stream_form_shade as predict() restates it: tables by `need`, bins by `need + bins * 8 + 16`
        need = t + r + o + m + (0 if img == IMG_LEAN_MIRROR else n_extra * 8)
        limit, limit_bins = (sc.LIMIT_LEAN, sc.LIMIT_LEAN_BINS) if img in (IMG_LEAN, IMG_LEAN_MIRROR) else (sc.LIMIT_SHADE, sc.LIMIT_SHADE_BINS)
        in_lds = need <= limit
        bins_in = (bins > 0) & in_lds & (need + bins * 8 + 16 <= limit_bins)
        request = N.where(in_lds, need + N.where(bins_in, bins * 8 + 16, 0), BARE[img])
        # the library: its image with everything staged, without and with the bins, and the decision the host makes of the scene
        L0 = lds_layout(hc, rows(img, 1, 0 * bins))
        L1 = lds_layout(hc, rows(img, 1, bins))
        assert (L0[:, LIMIT] == limit).all() and (L0[:, LIMIT_BINS] == limit_bins).all()
        assert N.array_equal(L0[:, END] + L0[:, SLACK], need)
        assert N.array_equal(L1[:, END] + L1[:, SLACK], need + N.where(bins > 0, bins * 8 + 16, 0))
        lib_in, lib_bins = L1[:, IN_LDS] == 1, L1[:, BINS_IN] > 0
        assert N.array_equal(lib_in, in_lds) and N.array_equal(lib_bins, bins_in) and N.array_equal(L1[:, BINS_IN], N.where(bins_in, bins, 0))
        assert N.array_equal(L1[:, REQUEST], request)
        L = lds_layout(hc, rows(img, lib_in.astype(int), N.where(lib_bins, bins, 0)))
        assert N.array_equal(L[:, END] + L[:, SLACK], request)
        check_parts(L, img, lib_in, S, stride, n_edges, fms, n_extra, N.where(lib_bins, bins, 0), request)
        sums[img] = (need, need + bins * 8 + 16, bins > 0)
    # trc_stream_form_absorb, as it was: `b.tally + b.maps + (lds_fm_bins ? bins * 8 : 0) + 16`, with the bins k_s_shade took or none
    for b_in in (bins, 0 * bins):
        old_absorb = t + m + b_in * 8 + 16
        La = lds_layout(hc, rows(IMG_ABSORB, 1, b_in))
        Li = lds_layout(hc, rows(IMG_INLINE, 1, b_in))
        assert N.array_equal(La[:, END] + La[:, SLACK], old_absorb) and (La[:, LIMIT_BINS] == LIMIT_ABSORB).all()
        assert N.array_equal(Li[:, END] + Li[:, SLACK], old_absorb + INLINE_MARGIN) and (Li[:, LIMIT_BINS] == LIMIT_INLINE).all()
        check_parts(La, IMG_ABSORB, N.ones(n, bool), S, stride, n_edges, fms, n_extra, b_in, old_absorb)
        # (the inline image starts on the next 16 bytes behind the search image, inside what the launch asks for the two)
        check_parts(Li, IMG_INLINE, N.ones(n, bool), S, stride, n_edges, fms, n_extra, b_in, old_absorb + INLINE_MARGIN - 15)
    sums[IMG_ABSORB] = (t + m + bins * 8 + 16, None, None)
    return sums


def check_parts(L, img, in_lds, S, stride, n_edges, fms, n_extra, bins_in, request):
    """every part behind the one before with room for what the kernel writes there, doubles on 8 bytes, the end inside the request"""
    terminal = img in (IMG_ABSORB, IMG_INLINE)
    has = in_lds.astype(N.int64)
    size = {'tally': (3 * S * has + (1 if img == IMG_SHADE else 2) * (1 - has) + 2 * has) * 8,
            'recs': 0 if terminal else S * stride * 8 * has, 'opt': 0 if terminal else S * 64 * has,
            'fm_edges': n_edges * 8 * has, 'fms': fms * has, 'fm_of': S * 4 * has, 'flags': 0 if img == IMG_INLINE else S * 4 * has,
            'extra': 0 if terminal or img == IMG_LEAN_MIRROR else n_extra * 8 * has, 'bins': bins_in * 8}
    assert (L[:, 0] == 0).all()
    for k, name in enumerate(PARTS):
        nxt = L[:, k + 1] if k + 1 < len(PARTS) else L[:, END]
        assert (L[:, k] + size[name] <= nxt).all(), name
        assert (L[:, k] % (4 if name == 'flags' else 8) == 0).all(), name
    assert (L[:, END] <= request).all()


def test_library_layout_gives_the_cases_their_restated_sums(hostcheck):
    """all 20 cases: predict()'s sum, limit and decisions per instance are those of the library's image of the instance"""
    for name in sorted(sc.CASES):
        c = sc.case(name)
        S = c.cs.n_surf
        n_edges = sum(len(u) + len(v) for u, v in c.edges.values())
        bins = sum((len(u) - 1) * (len(v) - 1) for u, v in c.edges.values())
        one = lambda x: N.array([x], dtype=N.int64)
        check_images(hostcheck, one(S), one(sc.record_stride(c.cs)), one(n_edges), one(len(c.edges)), one(len(c.cs.extra)), one(bins),
                     [one(x) for x in sc.table_bytes(c.cs, c.edges)])
        for inst, (total, limit, in_lds, bins_in) in c.instances.items():
            img = IMG_SHADE_X if inst.startswith('k_s_shade_x') else IMG_SHADE if inst.startswith('k_s_shade<') else \
                IMG_LEAN_MIRROR if inst.startswith('k_s_shade_c<0') else IMG_LEAN
            row = [img, 1, S, sc.record_stride(c.cs), n_edges, len(c.edges) * sc.SIZEOF_FLUXMAPDEV, len(c.cs.extra)]
            L0, L1 = lds_layout(hostcheck, [row + [0], row + [bins]])
            assert L0[END] + L0[SLACK] == total and L0[LIMIT] == limit
            assert (L1[IN_LDS] == 1) == in_lds and (L1[BINS_IN] > 0) == bins_in         # (the host's own decision)


def test_library_layout_gives_random_scenes_their_restated_sums(hostcheck, monkeypatch):
    """
    1e5 seeded scenes -- 1..3000 surfaces, both record strides of the cases, 0..4 maps of differing edge counts, 0..4000 doubles of
    optics tables -- half of them drawn freely, half with the surface count solved so that one of the sums lands within 2 KiB of one
    of its limits: the library's image against shade_cases.table_bytes, to the byte, with the same decisions on both sides of each
    limit.  (table_bytes as it stands; only its record stride is handed in, where it would walk 3000 descriptors per scene.)
    """
    monkeypatch.setattr(sc, 'record_stride', lambda cs: cs.stride)
    rng = N.random.RandomState(20260)
    n = 100000
    targets = [(IMG_SHADE, False), (IMG_SHADE, True), (IMG_LEAN, False), (IMG_LEAN, True), (IMG_ABSORB, False)]
    limit_of = {(IMG_SHADE, False): sc.LIMIT_SHADE, (IMG_SHADE, True): sc.LIMIT_SHADE_BINS, (IMG_LEAN, False): sc.LIMIT_LEAN,
                (IMG_LEAN, True): sc.LIMIT_LEAN_BINS, (IMG_ABSORB, False): LIMIT_ABSORB}
    S, stride, n_edges, n_maps, n_extra, bins, old = [N.zeros(n, dtype=N.int64) for _ in range(6)] + [N.zeros((4, n), dtype=N.int64)]
    for i in range(n):
        stride[i] = (17, 21)[rng.randint(2)]
        img, with_bins = targets[rng.randint(len(targets))]
        # (a scene aimed at a limit of the bins has a map; at the lean kernels' one, maps of the 30 KiB between their two limits)
        n_maps[i] = rng.randint(1 if (i % 2 and with_bins) else 0, 5)
        big = i % 2 and with_bins and img == IMG_LEAN
        shape = [(rng.randint(30, 80), rng.randint(30, 80)) if big else (rng.randint(1, 40), rng.randint(1, 40)) for _ in range(n_maps[i])]        # (nu, nv)
        n_extra[i] = rng.randint(4001)
        n_edges[i] = sum(nu + nv + 2 for nu, nv in shape)
        bins[i] = sum(nu * nv for nu, nv in shape)
        S[i] = rng.randint(1, 3001)
        if i % 2:           # the surface count that puts the target's sum at its limit + d, |d| <= 2 KiB
            d = rng.randint(-2 * sc.KiB, 2 * sc.KiB + 1)
            fixed = 2 * 8 + n_edges[i] * 8 + n_maps[i] * sc.SIZEOF_FLUXMAPDEV + 16
            per = 3 * 8 + 2 * 4
            if img != IMG_ABSORB:
                fixed += n_extra[i] * 8
                per += stride[i] * 8 + 8 * 8
            if with_bins or img == IMG_ABSORB:
                fixed += bins[i] * 8 + 16
            S[i] = min(max((limit_of[(img, with_bins)] + d - fixed) // per, 1), 3000)
        cs = types.SimpleNamespace(n_surf=int(S[i]), stride=int(stride[i]))
        edges = dict((k, (range(nu + 1), range(nv + 1))) for k, (nu, nv) in enumerate(shape))
        old[:, i] = sc.table_bytes(cs, edges)
    assert (S % 2 == 1).sum() > n // 4 and (S % 2 == 0).sum() > n // 4
    sums = check_images(hostcheck, S, stride, n_edges, n_maps, n_extra, bins, old)
    # scenes within 2 KiB of every limit, on both sides
    near = lambda x, limit, ok: (((x > limit - 2 * sc.KiB) & (x <= limit) & ok).sum(), ((x > limit) & (x <= limit + 2 * sc.KiB) & ok).sum())
    every = N.ones(n, bool)
    counts = {'72 KiB': near(sums[IMG_SHADE][0], sc.LIMIT_SHADE, every),
              '78 KiB, bins': near(sums[IMG_SHADE][1], sc.LIMIT_SHADE_BINS, sums[IMG_SHADE][2] & (sums[IMG_SHADE][0] <= sc.LIMIT_SHADE)),
              '120 KiB': near(sums[IMG_LEAN][0], sc.LIMIT_LEAN, every),
              '150 KiB, bins': near(sums[IMG_LEAN][1], sc.LIMIT_LEAN_BINS, sums[IMG_LEAN][2] & (sums[IMG_LEAN][0] <= sc.LIMIT_LEAN)),
              '78 KiB, k_s_absorb': near(sums[IMG_ABSORB][0], LIMIT_ABSORB, every)}
    # 158 KiB: k_s_bounce's own request (any, a multiple of 16) + the inline image, with requests drawn to put the total within 2 KiB of
    # the limit.  The image's bytes were compared above, so this holds the library's limit for it and no more: the addition and the
    # comparison themselves are host text of trc_stream_form_absorb that no host-compiled code reaches (the device tests of the terminal
    # surfaces do)
    d = rng.randint(-2 * sc.KiB, 2 * sc.KiB + 1, size=n)
    inline_old = sums[IMG_ABSORB][0] + INLINE_MARGIN
    bounce = N.maximum((LIMIT_INLINE + d - inline_old) // 16 * 16, 16)
    Li = lds_layout(hostcheck, N.stack([N.full(n, IMG_INLINE), N.ones(n, int), S, stride, n_edges, n_maps * sc.SIZEOF_FLUXMAPDEV, n_extra, bins], axis=1))
    assert N.array_equal(bounce + Li[:, END] + Li[:, SLACK] <= Li[:, LIMIT_BINS], bounce + inline_old <= LIMIT_INLINE)
    counts['158 KiB, inline'] = near(bounce + inline_old, LIMIT_INLINE, every)
    print(counts)
    assert all(lo >= 100 and hi >= 100 for lo, hi in counts.values()), counts


# -- the library's choice of kernels (csrc/trc_forms.h) against the restated one ----------------------------------------------------
SHADE_FAMILIES = ('k_s_shade', 'k_s_shade_c', 'k_s_shade_x')


def case_facts(c, given=False):
    """the fact block of a case's streaming call: the scene with its map as the library gathers it, the case's source or (carry, given)
    its bundle; 'carry-mat': the materials' tables are on the device"""
    import search_cases as S
    f = S.scene_facts(c.cs, None, None, c.edges)
    src = -1 if (c.carry or given) else c.source().source_args()[0].kind
    f.update(n=sc.N_RAYS, flags=S.TRACE_ACCEL | S.TRACE_STREAM, src_kind=src, spec=int(c.spec and src >= 0), carry=int(c.carry),
             mat_dev=int(c.kind == 'carry-mat'), term_ok=1)
    return f


def test_header_decides_every_case_as_restated(hostcheck):
    """all 20 cases, none left out: every decision of the header for the case's facts is the restated one (mega_cases.decide, whose
    shading stage is shade_forms()), and its shading kernels are predict()'s, with predict()'s tables and bins in LDS"""
    import mega_cases as M
    import search_cases as S
    for name in sorted(sc.CASES):
        c = sc.case(name)
        for given in ((False, True) if name in sc.GIVEN else (False,)):
            f = case_facts(c, given)
            mine, lib = M.decide(f), S.library_decide([f])[0]
            assert mine == lib, (name, sorted((k, mine.get(k), lib.get(k)) for k in set(mine) | set(lib) if mine.get(k) != lib.get(k)))
            assert lib['use_stream'] and lib['decided']
            shk = dict((sc.short_name(k[0]), k) for k in lib['shk'])
            assert set(shk) == set(c.instances), (name, sorted(shk))
            for inst, (total, limit, in_lds, bins_in) in c.instances.items():
                assert shk[inst][4] == int(in_lds) and (shk[inst][5] > 0) == bins_in


def test_header_names_every_instance(hostcheck):
    """the ids the header can produce in the shading families with the CHART, SPLIT and MAT arguments off -- what the cases hold them at --
    are ALL_INSTANCES as the cases spell them; with those arguments, the kernels of the built library by name"""
    import search_cases as S
    names = [n for n in S.library_ids() if n.split('<')[0] in SHADE_FAMILIES]
    off = [n for n in names if n.endswith(', false>') and not (n.startswith('k_s_shade_x') and n != 'k_s_shade_x<%s, false, false, false>' % n[12:-22])]
    assert sorted(sc.short_name(n) for n in off) == sorted(sc.ALL_INSTANCES)
    lib = os.path.join(ROOT, 'tracer_amd', 'lib', 'libtracer_amd.so')
    import re
    import shutil
    if not os.path.exists(lib) or shutil.which('nm') is None:
        pytest.skip('no built library, or no nm')
    squeeze = lambda x: re.sub(r'\s+', '', x)
    held = set()
    for line in subprocess.check_output(['nm', '-C', lib]).decode().splitlines():
        m = re.search(r'\b(k_s_shade(_c|_x)?)(<[^>]*>)\(StreamParams\)', line)
        if m and '__device_stub__' not in line:
            held.add(squeeze(m.group(1) + m.group(3)))
    assert held == set(squeeze(n) for n in names), sorted(held ^ set(squeeze(n) for n in names))
