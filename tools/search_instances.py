"""One line per search kernel instance of the streaming engine (the 79 of tests/search_cases.py) from a rocprofv3 --kernel-trace --stats
output directory of tests/test_gpu_search_instances.py: its calls in the trace, the calls tests/search_cases.predict() expects of
the file's streaming calls, and the cases predicted to launch it.  The trace is of the whole file, so the cases are the
prediction's, not read from the trace: what ties them to the calls is the count -- predict() gives the launches of every search
kernel per case (one per bounce the reference's rays live through; a second call counts both).  A line whose calls differ from that,
or a kernel of these families that is not one of the 79, is flagged: the prediction is then wrong.  Instances that no input selects
are listed with the condition that excludes them.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m pytest tests/test_gpu_search_instances.py -q
    python tools/search_instances.py OUT > profiles/search_instances.txt
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import search_cases as S        # noqa: E402

squeeze = lambda s: re.sub(r'\s+', '', s)
family = re.compile(r'\b(%s)(<[^>]*>)?\(' % '|'.join(sorted(S.FAMILIES, key=len, reverse=True)))
calls = {}
for fn in glob.glob(sys.argv[1] + '/**/*kernel_stats.csv', recursive=True):
    with open(fn) as f:
        for r in csv.DictReader(f):
            m = family.search(r['Name'] if '(' in r['Name'] else r['Name'] + '(')
            if m:
                k = squeeze(m.group(1) + (m.group(2) or ''))
                calls[k] = calls.get(k, 0) + int(r['Calls'])
expected, cases = {}, {}
for c in S.CALLS:
    for inst, n in S.predict(c).items():
        expected[squeeze(inst)] = expected.get(squeeze(inst), 0) + n
        cases.setdefault(squeeze(inst), []).append(c.name)
print('%-50s %6s %8s  %s' % ('instance', 'calls', 'expected', 'cases predicted to launch it (tests/search_cases.py)'))
bad = 0
for inst in S.ALL_INSTANCES:
    k = squeeze(inst)
    n, want = calls.pop(k, 0), expected.get(k, 0)
    if inst in S.UNREACHABLE:
        flag = '' if n == 0 else '   <-- launched, but held to be unreachable'
        print('%-50s %6d %8d  unreachable: %s%s' % (inst, n, want, S.UNREACHABLE[inst], flag))
    else:
        flag = '' if n == want and n > 0 else '   <-- prediction and trace disagree'
        print('%-50s %6d %8d  %s%s' % (inst, n, want, ' '.join(cases.get(k, [])) or '-', flag))
    bad += bool(flag)
for k, n in sorted(calls.items()):
    print('%-50s %6d  not one of the 79   <-- unexpected' % (k, n))
    bad += 1
sys.exit(1 if bad else 0)
