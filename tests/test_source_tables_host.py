"""
The host side of the tabulated sources (csrc/trc_source_host.h) without a device.  The program of tests/sourcecheck holds the one
table check to the messages the create functions always gave, the packing to the pack functions bit for bit, the id registry to its
order, its exhaustion and its books after eight threads, and the descriptor arithmetic to its writes and refusals -- built once with
the address and undefined-behaviour sanitizers and once with the thread sanitizer.  The same check, as a library, is held to the
Python checks of the table classes on the bad tables their own tests list: both refuse, or both accept.
"""
import ctypes as C
import os
import subprocess

import numpy as N
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SUNSHAPE, K_ANGLE, K_EMITTANCE, K_SPECTRUM = range(4)


@pytest.mark.parametrize('target,exe', [('sourcecheck', 'source_check'), ('sourcecheck-tsan', 'source_check_tsan')])
def test_source_host_under_the_sanitizers(target, exe):
    subprocess.check_call(['make', '-s', '-C', ROOT, target])
    p = subprocess.run([os.path.join(ROOT, 'tests', 'sourcecheck', exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert ' 0 violations' in p.stdout


def source_check_library():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'sourcecheck'])
    lib = C.CDLL(os.path.join(ROOT, 'tests', 'sourcecheck', 'libtrc_source_check.so'))
    lib.sc_table.restype = C.c_int
    lib.sc_table.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_int]
    return lib


def header_says(lib, kind, x, y):
    """(status, message) of the header's check-and-pack function of `kind` for the table (x, y)"""
    x = N.ascontiguousarray(x, dtype=float)
    y = N.ascontiguousarray(y, dtype=float)
    assert x.shape == y.shape
    msg = C.create_string_buffer(512)
    st = lib.sc_table(kind, x.size, x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)), msg, 512)
    return st, msg.value.decode()


@pytest.fixture(scope='module')
def lib():
    return source_check_library()


def python_refuses(check, x, y):
    try:
        check(x, y)
    except ValueError:
        return True
    return False


# tests/test_sunshape.py::test_invalid_tables_raise (the tables whose two columns have one length: the C side has one count), and
# tables either side accepts
ANGLE_TABLES = [
    ([0.], [1.]),
    (N.linspace(0., 0.01, 4097), N.ones(4097)),
    ([0., N.nan, 0.01], [1., 1., 1.]),
    ([0., 0.02, 0.01], [1., 1., 1.]),
    ([0., 0.01, 0.01], [1., 1., 1.]),
    ([-0.001, 0.01], [1., 1.]),
    ([0., N.pi / 2.], [1., 1.]),
    ([0., 0.01], [1., -1.]),
    ([0., 0.01], [1., N.inf]),
    ([0., 0.01], [0., 0.]),
    ([0., 0.01, 0.02], [0., 0., 0.]),
    ([0., N.pi], [1., 1.]),
    ([0., N.nextafter(N.pi, 4.)], [1., 1.]),
    ([0., 0.01], [1., 1.]),
    (N.linspace(0., 0.01, 4096), N.ones(4096)),
]


@pytest.mark.parametrize('i', range(len(ANGLE_TABLES)))
def test_sunshape_and_angle_tables_as_python_checks_them(lib, i):
    from tracer_amd import sources
    x, y = ANGLE_TABLES[i]
    for kind, check in ((K_SUNSHAPE, sources.check_sunshape_table), (K_ANGLE, sources.check_angle_table)):
        st, msg = header_says(lib, kind, x, y)
        assert (st != 0) == python_refuses(check, x, y), (kind, st, msg)
        assert (st == 0) == (msg == '')


# tests/test_source_spectrum.py::test_invalid_tables_raise and tests/test_poly_source_host.py::test_polychromatic_spectrum_validation
# (again the tables of one length), and tables either side accepts
SPECTRUM_TABLES = [
    ([0.5], [1.]),
    ([0.5, 0.4], [1., 1.]),
    ([0.4, 0.4], [1., 1.]),
    ([0.4, 0.5], [1., -1.]),
    ([0.4, 0.5], [1., N.nan]),
    ([0.4, N.inf], [1., 1.]),
    ([0.4, 0.5], [0., 0.]),
    (N.linspace(1., 2., 4097), N.ones(4097)),
    ([1e-6], [1.]),
    ([1e-6, 1e-6], [1., 1.]),
    ([1e-6, 2e-6, N.nan], [1., 1., 1.]),
    ([1e-6, 2e-6], [1., -1.]),
    ([1e-6, 2e-6], [1., N.inf]),
    ([1e-6, 2e-6], [0., 0.]),
    ([0.4, 0.5], [1., 1.]),
    (N.linspace(1e-7, 1e-6, 4096), N.ones(4096)),
]


@pytest.mark.parametrize('i', range(len(SPECTRUM_TABLES)))
def test_spectrum_tables_as_python_checks_them(lib, i):
    from tracer_amd.source_spectrum import SourceSpectrum
    x, y = SPECTRUM_TABLES[i]
    st, msg = header_says(lib, K_SPECTRUM, x, y)
    for make in (SourceSpectrum.tabulated, SourceSpectrum.polychromatic):
        assert (st != 0) == python_refuses(make, x, y), (st, msg)
