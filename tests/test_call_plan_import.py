"""tracer_amd/call_plan.py decides without the library: it imports on a machine that has none"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_plan_imports_without_the_library():
    code = ("import sys\n"
            "before = set(sys.modules)\n"
            "from tracer_amd import call_plan\n"
            "assert call_plan.last_room(1000, False) == 1000 and call_plan.last_room(1000, True) == 3024\n"
            "new = set(sys.modules) - before\n"
            "bad = [k for k in new if k in ('ctypes', 'torch') or k.startswith('tracer_amd.') and k.split('.')[1] in ('_cabi', 'scene')]\n"
            "assert not bad, bad\n")
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)
