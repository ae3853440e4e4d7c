import os
import sys

import pytest
# torch before any test loads libtracer_amd.so: the library then binds to the HIP runtime torch has already loaded.  Loaded the
# other way round, the process holds two HIP runtimes, and once a test has initialised torch's the library sees no GPU
# ("torch in the same process").  Importing torch opens no device.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope='session')
def golden_dir():
    return GOLDEN


@pytest.fixture(autouse=True)
def _reproducible_streams(request):
    """Every test starts from the same process-wide seeds (the product seeds itself from os.urandom when none is given): the
    statistical checks see the same rays on every run."""
    import zlib
    import numpy
    key = zlib.crc32(request.node.nodeid.encode())
    numpy.random.seed(key % (2 ** 31))
    try:
        from tracer_amd import rng
        rng.seed(0x5EED0000 + key)
    except Exception:           # the package itself is under test for importability elsewhere
        pass
    yield
