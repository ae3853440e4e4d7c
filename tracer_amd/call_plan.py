"""
What a TracerEngine.ray_tracer call will do, decided apart from doing it: the engine, what becomes of the reference's Kd-tree, whether
the hit buffer goes on filling and how much room the call gets, the form of the fast engine, the room for the last rays, and whether a
call of a scene that splits rays is made once more.

Plain functions of the facts of a call -- what the bundle says (Rays), what the scene and the device say (Scene) -- and of the call's
keywords; each returns a value the engine acts on.  The thresholds are TracerEngine's attributes, read from the engine handed in
(`lim`), so that one set on the class or on an instance holds.  Nothing here touches the device or the library:
tests/test_call_plan_host.py holds the decisions to account through TracerEngine on a device double.
"""
from collections import namedtuple

# columns: those a pending source's spectrum fills when the bundle is made ('wavelengths', 'ref_index')
# A pending source whose spectrum is carried (SourceSpectrum.polychromatic) is pending AND polychromatic: every ray brings the whole
# table, and the device makes the (W, n) columns where an engine needs them (carried()).
Rays = namedtuple('Rays', 'n pending polychromatic complex_index spectrum columns')
# splits: optics that send two rays on from a hit: the streaming form alone (k_s_shade_x<.., SPLIT>)
# materials_on_device: the device evaluates the scene's materials for this call's source (asked for a source with a spectrum only)
Scene = namedtuple('Scene', 'n_surf carries splits capture materials materials_on_device')


def ray_facts(bundle):
    if hasattr(bundle, 'is_pending') and bundle.is_pending():
        spectrum = bundle.source_spectrum()
        poly = bool(getattr(spectrum, 'is_carried', lambda: False)())       # (SourceSpectrum.polychromatic: the rays carry the table)
        return Rays(bundle.get_num_rays(), True, poly, False, spectrum, bundle.spectral_columns() if spectrum is not None else ())
    return Rays(bundle.get_num_rays(), False, bool(bundle.is_polychromatic()), bool(bundle.has_complex_index()), None, ())


def carried(rays):
    """the rays are those of a pending source that carries its spectrum"""
    return bool(rays.pending and rays.polychromatic)


def scene_facts(dev, rays=None):
    c = dev.compiled
    # A source with a spectrum stays pending on a scene whose materials' tables are on the device (TabulatedMaterial(...,
    # device=True)): the kernels evaluate m(lambda) per ray and draw the wavelengths themselves.
    dev_mats = rays is not None and rays.spectrum is not None and getattr(c, 'material_tables', None) is not None and \
        dev.materials_on_device()
    return Scene(dev.n_surf, bool(c.carries), bool(c.splits), any(c.capture), bool(c.materials), dev_mats)


def choose_engine(lim, rays, scene, tree):
    """engine='auto': 'ordered' or 'fast'"""
    # Complex refractive indices, materials evaluated at the rays' wavelengths and spectra travel with the rays of the
    # ordered engine and of the streaming form of the fast engine (64 rays or more of a given bundle; k_s_shade_x).  A
    # captured hit of a polychromatic ray keeps its sample wavelengths and its spectrum before and after the surface (what
    # PolychromaticAccountant collects).
    # A pending source that carries its spectrum goes the same way without ever being made on the host (k_s_shade_p, DESIGN.md
    # section 14.13): the streaming form from 64 rays on, scenes that split rays included, the ordered engine otherwise.
    carries = scene.carries or rays.polychromatic or rays.complex_index
    if carries:
        carries = (rays.pending and not scene.materials_on_device and not carried(rays)) or rays.n < 64
    # Optics that send two rays on from a hit (single_ray=False) are traced by the streaming form too (k_s_shade_x<.., SPLIT>,
    # DESIGN.md section 14.11): 64 rays or more, no source spectrum.  The ray tree, smaller calls and sources with a
    # spectrum stay with the ordered engine.
    splits = scene.splits and not (lim.SPLIT_ON_FAST and rays.n >= 64 and
                                   not (rays.spectrum is not None and not scene.materials_on_device and not carried(rays)))
    return 'ordered' if (tree or splits or carries) else 'fast'


def kd_action(lim, rays, scene, engine, accel, Kd_Tree):
    """the reference's Kd-tree of an accel=... call: 'none' (no accel), 'given' (the caller's), 'build' (now, for the device),
    'defer' (until engine.Kd_Tree is read) or 'never'"""
    if not accel:
        return 'none'
    if Kd_Tree is not None:
        return 'given'
    # The fast engine does not walk the reference's Kd-tree: large calls search the library's own uniform grid over the same
    # geometry boxes (csrc/trc_bounds.h), small ones test the boxes themselves.  Building the tree -- the reference's SAH
    # build, Python: 38 ms for the 219 surfaces of the NSTTF field, minutes for a mesh of 1e5 faces -- before every trace
    # of a scene that moves (a day of sun positions) cost more than the traces.  engine.Kd_Tree builds it when it is read.
    # The ordered engine walks it, but below KD_WORTH_IT box tests per bounce (rays x surfaces: a millisecond of the GPU)
    # testing every surface's box costs less than the build: 1e5 rays on the NSTTF field took 30 ms with the tree, 3 without.
    # Beyond KD_BUILD_MAX surfaces (a mesh) the tree is never built for a trace: the scene stands on the library's large grid,
    # which the ordered engine walks too (trc_nearest_grid32).
    if scene.n_surf > lim.KD_BUILD_MAX and engine in ('fast', 'ordered'):
        return 'never'
    if engine == 'fast' or (engine == 'ordered' and scene.n_surf <= 65535 and rays.n * scene.n_surf <= lim.KD_WORTH_IT):
        return 'defer'
    return 'build'


def hit_room(n, hit_capacity, capture_rate):
    """entries of the hit buffer this call is given"""
    # Room for the hits of this call: two per ray unless the caller says otherwise -- or, once the scene in its present
    # poses has been traced, four times the share of captured hits per ray seen so far (a field sends 6 % of its rays to
    # the receiver: successive calls then fit the buffer of the first many times over before it has to grow).
    if hit_capacity is not None:
        return int(hit_capacity)
    need = 2 * n + 1024
    return need if capture_rate is None else min(need, int(4. * capture_rate * n) + 65536)


def may_keep_hits(rays, scene, feed, hit_capacity, marks_held):
    """the call may go on filling the hit buffer, as far as can be said without asking the device"""
    # The hits stay in the device's buffer until an accountant is read (scene.PendingHits).  A call that finds the hits
    # of the calls before still unread there -- every accountant concerned still holds its mark -- goes on filling the
    # same buffer, grown if need be; otherwise what it holds is delivered (or dropped, when nobody waits for it any more)
    # and the buffer emptied.  An explicit hit_capacity is taken literally: an empty buffer of that size.
    keep = bool(feed and hit_capacity is None and marks_held)
    if keep and rays.polychromatic:
        keep = False        # (all hits in the buffer have the same spectral columns: hits waiting there with spectra, or
                            # before a call that brings spectra, are delivered first)
    if keep and scene.splits:
        keep = False        # (a call whose hits do not fit is made again on an empty buffer: see split_retry)
    return keep


def fast_form(lim, rays, scene, fast_kernel, accel, form_rate):
    """(the `stream` argument of the fast engine: True, False or None for the library's choice; whether the call is tuned)"""
    stream = {'auto': None, 'stream': True, 'megakernel': False}[fast_kernel]
    if stream is None and (scene.splits or carried(rays)):
        stream = True       # (fast_kernel='megakernel' is refused by the library, which names trc_trace_ordered)
    if stream is None and accel and scene.n_surf > lim.KD_BUILD_MAX:
        stream = True       # the streaming form has the grid for large scenes; the megakernel would test every box
    # Large calls go to the streaming form.  On a scene where it turns out slow -- every segment a hit on overlapping curved
    # shapes, several bounces deep: below SLOW_STREAM segments per ms, a fortieth of its rate on a heliostat field -- the next
    # large call tries the megakernel, whose rays stay in registers, and the faster of the two serves the scene from then on.
    # Both forms end every ray alike (test_forms_of_the_fast_engine_end_every_ray_alike).
    tuned = stream is None and rays.n >= lim.TUNE_MIN_RAYS and scene.n_surf <= lim.TUNE_MAX_SURFACES
    if tuned and 'stream' in form_rate and form_rate['stream'] < lim.SLOW_STREAM:
        stream = False if ('megakernel' not in form_rate or form_rate['megakernel'] > form_rate['stream']) else True
    return stream, tuned


def last_room(n, splits, last_capacity=None):
    """rows for the rays still alive after `reps` interactions"""
    # Rays still alive after `reps` interactions come back as the call's result (tracer_engine.py:293-295).  Bundles beyond
    # 2^24 rays get room for 2^22 of them unless the caller says otherwise (last_capacity=...): 1e8 rays would cost 5.6 GB
    # of host arrays per call for a result that is empty in most scenes.  More rays left than room is an error of the
    # call (status ERR_CAPACITY), raised after the trace: tallies and flux maps of the scene then hold it, the accountants do not.
    if last_capacity is not None:
        cap = int(last_capacity)
    elif n > (1 << 24):
        cap = 1 << 22
    else:
        cap = 2 * n + 1024 if splits else n     # (two rays may leave a hit: room as for the hits; beyond it the call is made again)
    # (at most one ray left per ray given, unless the optics split rays)
    return max(1, cap if splits else min(cap, n))


def split_retry(scene, hit_capacity, hits_dropped, no_room):
    """(a call of a scene that splits rays is undone and made once more; its hit buffer grows first)"""
    # A scene that splits rays can capture more hits than the default room of two per ray, and leave more rays than it was
    # given; the ordered engine has neither limit, and nothing grows in the middle of a call.  So before a call that
    # captures the packed tally buffer (tallies, flux maps, transfer matrix) is kept aside, and a call that dropped hits
    # or had no room for its last rays is undone -- hit buffer emptied, tallies put back -- and made once more, with the
    # same seed, with room for every hit it counted (captured or not: an upper bound; the library adds what the buffer's
    # open chunks can leave unused) and every ray it left.  A scene that captures nothing pays for no snapshot: there
    # only the last rays can lack room, the tallies of such a call are complete, and they are put back behind the
    # second call.  Room the caller set (hit_capacity, last_capacity) is taken literally.
    grow = bool(hits_dropped and scene.capture and hit_capacity is None)
    return grow or no_room, grow
