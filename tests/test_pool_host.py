"""
The block cache behind device memory and pinned host memory (csrc/trc_pool.h) without a device: the program of tests/poolcheck drives
it through a fake backend -- classes, reuse, caps, eviction order, the retry after a refused allocation, the device key, the wait
before a block is kept, and the books after eight threads -- built once with the address and undefined-behaviour sanitizers and once
with the thread sanitizer.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('target,exe', [('poolcheck', 'pool_check'), ('poolcheck-tsan', 'pool_check_tsan')])
def test_block_cache_under_the_sanitizers(target, exe):
    subprocess.check_call(['make', '-s', '-C', ROOT, target])
    p = subprocess.run([os.path.join(ROOT, 'tests', 'poolcheck', exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert ' 0 violations' in p.stdout
