"""
The host side of a scene (csrc/trc_scene_host.h) without a device: the program of tests/scenecheck holds the one validation of a
caller's Kd-tree to a hand-made tree and to the malformed ones that used to reach the host's indexing, its packing to hand-written
words, the tally layout to sums written out and the search tables to their build order -- built with the address and
undefined-behaviour sanitizers.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_host_under_the_sanitizers():
    subprocess.check_call(['make', '-s', '-C', ROOT, 'scenecheck'])
    p = subprocess.run([os.path.join(ROOT, 'tests', 'scenecheck', 'scene_check')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout
    assert ' 0 violations' in p.stdout
