"""
The table path of the library against its host header, and the one device block cache behind both units of the library.
  * trc_sunshape_create, trc_angle_table_create and trc_emittance_table_create refuse a bad table with the status and the words of
    csrc/trc_source_host.h (through the host check library of tests/sourcecheck), and give their tables ids from one sequence;
  * device blocks taken by trc_source_generate (trc_protocol.hip) wait in the cache that trc_ctx_destroy (trc_scene.hip) trims.
"""
import ctypes as C

import numpy as N
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_api import _child
from test_source_tables_host import K_SUNSHAPE, K_ANGLE, K_EMITTANCE, header_says, source_check_library

nan, inf = N.nan, N.inf
# one table per kind of refusal (None: the array is not handed over), for every create function
BAD_TABLES = [
    ('one point', [0.1], [1.]),
    ('too many points', N.linspace(1e-4, 0.4097, 4097), N.ones(4097)),
    ('no ordinates', [0.1, 0.2], None),
    ('an abscissa not finite', [0.1, nan, 0.3], [1., 1., 1.]),
    ('abscissae not increasing', [0.1, 0.3, 0.2], [1., 1., 1.]),
    ('a negative ordinate', [0.1, 0.2], [1., -1.]),
    ('an ordinate not finite', [0.1, 0.2], [inf, 1.]),
    ('outside the domain', [-0.001, 0.2], [1., 1.]),
    ('no mass', [0.1, 0.2, 0.3], [0., 0., 0.]),
]
CREATE = [(K_SUNSHAPE, 'trc_sunshape_create'), (K_ANGLE, 'trc_angle_table_create'), (K_EMITTANCE, 'trc_emittance_table_create')]


def _f64(a):
    return None if a is None else N.ascontiguousarray(a, dtype=float)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def test_create_functions_refuse_as_the_header_does_and_share_their_ids():
    from tracer_amd import _cabi
    ctx = _cabi.get_context(0)
    lib = ctx.lib
    hc = source_check_library()
    for kind, name in CREATE:
        create = getattr(lib, name)
        for what, x, y in BAD_TABLES:
            x, y = _f64(x), _f64(y)
            out = C.c_void_p(1)
            st = create(ctx.handle, x.size, _ptr(x), _ptr(y), C.byref(out))
            said = lib.trc_last_error().decode()
            msg = C.create_string_buffer(512)
            want = hc.sc_table(kind, x.size, _ptr(x), _ptr(y), msg, 512)
            print('%-28s %-26s %d %s' % (name, what, st, said))
            assert want == _cabi.ERR_INVALID and msg.value.startswith(name.encode()), (name, what, want, msg.value)
            assert (st, said) == (want, msg.value.decode()), (name, what)
            assert out.value is None, (name, what)
    # three tables, one of each kind: ids in the order they were made
    x, y = _f64([0.1, 0.2, 0.3]), _f64([1., 2., 1.])
    assert header_says(hc, K_SUNSHAPE, x, y) == (0, '')
    ids, handles = [], []
    for kind, name in CREATE:
        out, i = C.c_void_p(), C.c_int32(0)
        _cabi.check(getattr(lib, name)(ctx.handle, x.size, _ptr(x), _ptr(y), C.byref(out)))
        _cabi.check(lib.trc_sunshape_id(out, C.byref(i)))
        handles.append(out)
        ids.append(i.value)
    for h in handles:
        _cabi.check(lib.trc_sunshape_destroy(h))
    assert ids[0] >= 1 and ids == [ids[0], ids[0] + 1, ids[0] + 2], ids


_GENERATED_THEN_TRIMMED = (
    "import ctypes as C, json\n"
    "import numpy as N\n"
    "from tracer_amd import _cabi, sources\n"
    "lib = _cabi.load_library()\n"
    "hip = C.CDLL('libamdhip64.so')\n"
    "def free_bytes():\n"
    "    free, total = C.c_size_t(0), C.c_size_t(0)\n"
    "    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0\n"
    "    return free.value\n"
    "ctx = C.c_void_p()\n"
    "_cabi.check(lib.trc_ctx_create(0, C.byref(ctx)))\n"
    "def generate(n):\n"
    "    desc, _, seed, off = sources.disk_bundle(n, N.c_[[0., 0., 1.]], N.r_[0., 0., -1.], 1., 0.005, seed=3).source_args()\n"
    "    col = N.empty((7, n))\n"
    "    rid = N.empty(n, dtype=N.uint64)\n"
    "    rays = _cabi.make_rays(n, *col, rid=rid)\n"
    "    _cabi.check(lib.trc_source_generate(ctx, C.byref(desc), n, seed, off, C.byref(rays)))\n"
    "    return bool(N.all(rid == N.arange(n, dtype=N.uint64)) and N.all(col[2] == 1.))\n"
    "generate(256)\n"                      # (the kernels are on the device before the first count)
    "r = {'f0': free_bytes()}\n"
    "r['ok'] = generate(4000000)\n"
    "r['f1'] = free_bytes()\n"
    "_cabi.check(lib.trc_ctx_destroy(ctx))\n"
    "r['ctx_gone'] = free_bytes()\n"
    "print(json.dumps(r))\n")


def test_blocks_of_source_generation_wait_in_the_cache_the_context_trims():
    """trc_source_generate for 4e6 rays into host columns takes eight device columns of 32 MB (seven of the bundle and the stream
    ids), by the driver's count of free memory: they stay taken after the call -- the blocks wait in the library's one cache -- and
    come back when the context goes, which trims it; with TRC_DEV_POOL=0 they are back straight after the call.  (The quarters allow
    for the driver's own granularity, as in test_device_blocks_wait_in_the_cache_until_the_context_goes.)"""
    r = _child(_GENERATED_THEN_TRIMMED)
    A = r['f0'] - r['f1']
    print('cache on: held after the call %d, back after the context %d' % (A, r['ctx_gone'] - r['f1']))
    assert r['ok']
    assert A >= 128 << 20
    assert r['ctx_gone'] - r['f1'] > 3 * A / 4
    off = _child(_GENERATED_THEN_TRIMMED, TRC_DEV_POOL='0')
    print('cache off: held after the call %d' % (off['f0'] - off['f1']))
    assert off['ok']
    assert off['f0'] - off['f1'] < A / 4
