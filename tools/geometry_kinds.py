"""One line per kernel instance that the calls of tests/geometry_cases.py are predicted to launch, from a rocprofv3 --kernel-trace
--stats output directory of tests/test_gpu_geometry_kinds.py: its calls in the trace, the calls predicted (geometry_cases.launched:
the search stages from the restated forms and the reference's live rays, one megakernel launch per megakernel call; one k_ord_bounce
launch per level with live rays) and the calls of geometry_cases.py behind them.  The shading kernels and k_s_absorb are launched per
bounce as the active lists turn out: for them the line says only that the instance ran.  A line whose calls differ from the
prediction, and a kernel of these families that no call predicts, is flagged; the streaming engine's bookkeeping kernels (HELPERS)
are listed without a prediction.  The trace is a run of its own, without counters.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m pytest tests/test_gpu_geometry_kinds.py -q -m gpu
    python tools/geometry_kinds.py OUT > profiles/geometry_kinds.txt
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import geometry_cases as G      # noqa: E402
import search_cases as S        # noqa: E402

squeeze = lambda s: re.sub(r'\s+', '', s)
family = re.compile(r'\b(k_s_\w+|k_trace_\w+|k_ord_bounce)(<[^>]*>)?\(')
calls = {}
for fn in glob.glob(sys.argv[1] + '/**/*kernel_stats.csv', recursive=True):
    with open(fn) as f:
        for r in csv.DictReader(f):
            m = family.search(r['Name'] if '(' in r['Name'] else r['Name'] + '(')
            if m:
                k = squeeze(m.group(1) + (m.group(2) or ''))
                calls[k] = calls.get(k, 0) + int(r['Calls'])
expected, counted, cases = {}, {}, {}
HELPERS = ('k_s_add2', 'k_s_merge_tallies', 'k_s_partition')


def note(kernel, n, case):
    k = squeeze(kernel)
    counted[k] = counted.get(k, True) and n is not None
    expected[k] = expected.get(k, 0) + (n or 0)
    cases.setdefault(k, []).append(case)


for c in G.CALLS:
    for kernel, n in G.launched(c)[1].items():
        note(kernel, n, c.name)
for scn, kd, accel, kernel in G.ORDERED:
    s = G.scene(scn)
    bounces = sum(1 for L in G.reference(scn, 'given')['levels'][:s.reps] if L['n_live'] > 0)
    note(S.library_decide([G.ordered_facts(scn, kd, accel)])[0]['ord'], bounces, '%s under %s, accel %s' % (scn, kd if kd == 'built' else 'a tree of depth %d' % kd[1], accel))
print('%-46s %6s %8s  %s' % ('instance', 'calls', 'expected', 'calls of tests/geometry_cases.py predicted to launch it'))
bad = 0
short = lambda names: ', '.join(names) if len(names) <= 8 else '%s, ... (%d calls)' % (', '.join(names[:6]), len(names))
for k in sorted(expected):
    n = calls.pop(k, 0)
    if counted[k]:
        flag = '' if n == expected[k] and n > 0 else '   <-- prediction and trace disagree'
        print('%-46s %6d %8d  %s%s' % (k, n, expected[k], short(cases[k]), flag))
    else:
        flag = '' if n > 0 else '   <-- predicted, not launched'
        print('%-46s %6d %8s  %s%s' % (k, n, '> 0', short(cases[k]), flag))
    bad += bool(flag)
for k, n in sorted(calls.items()):
    if k in HELPERS:
        print('%-46s %6d %8s  (bookkeeping of the streaming engine: active lists, tallies)' % (k, n, '-'))
    else:
        print('%-46s %6d  predicted by no call   <-- unexpected' % (k, n))
        bad += 1
sys.exit(1 if bad else 0)
