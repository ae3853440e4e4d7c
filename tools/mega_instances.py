"""One line per megakernel instance (the 24 of tests/mega_cases.py) from a rocprofv3 --kernel-trace --stats output directory of
tests/test_gpu_mega_instances.py: its calls in the trace, the calls predicted -- one launch per case whose restated plan
(mega_cases.plan, mega_cases.instance) names the instance, and the one trace that follows the refused tree -- and those cases.  The
ordered engine's search kernels on the hand-made chains follow: one launch per level of the reference that has live rays.  A line
whose calls differ from the prediction, or a k_trace_* kernel that is not one of the 24, is flagged: the prediction is then wrong.
Instances that no input selects are listed with the condition that excludes them.  The trace is a run of its own, without counters.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m pytest tests/test_gpu_mega_instances.py -q
    python tools/mega_instances.py OUT > profiles/mega_instances.txt
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import mega_cases as M          # noqa: E402

squeeze = lambda s: re.sub(r'\s+', '', s)
family = re.compile(r'\b(k_trace_\w+|k_ord_bounce)(<[^>]*>)?\(')
calls = {}
for fn in glob.glob(sys.argv[1] + '/**/*kernel_stats.csv', recursive=True):
    with open(fn) as f:
        for r in csv.DictReader(f):
            m = family.search(r['Name'] if '(' in r['Name'] else r['Name'] + '(')
            if m:
                k = squeeze(m.group(1) + (m.group(2) or ''))
                calls[k] = calls.get(k, 0) + int(r['Calls'])
expected, cases = {}, {}
for c in M.CASES:
    p = c.plan()
    k = squeeze(M.instance(p['kernel'], c.spec, c.src == 'sun', c.chart))
    expected[k] = expected.get(k, 0) + 1
    cases.setdefault(k, []).append(c.name + ('' if p['kernel'] != 'fast256' else ' (%d%d)' % (p['lds_tally'], p['lds_scene'])))
k = squeeze(M.CASE['row/boxes'].target)         # test_tree_deeper_than_the_stack_is_refused traces the row without a tree
expected[k] = expected.get(k, 0) + 1
cases.setdefault(k, []).append('row after chain(%d) is refused' % M.REFUSED_DEPTH)
print('%-44s %6s %8s  %s' % ('instance', 'calls', 'expected', 'cases predicted to launch it (tests/mega_cases.py; k_trace_fast: its staging form)'))
bad = 0
for inst in M.ALL_INSTANCES:
    k = squeeze(inst)
    n, want = calls.pop(k, 0), expected.get(k, 0)
    if inst in M.UNREACHABLE:
        flag = '' if n == 0 else '   <-- launched, but held to be unreachable'
        print('%-44s %6d %8d  unreachable: %s%s' % (inst, n, want, M.UNREACHABLE[inst], flag))
    else:
        flag = '' if n == want and n > 0 else '   <-- prediction and trace disagree'
        print('%-44s %6d %8d  %s%s' % (inst, n, want, ', '.join(cases.get(k, [])) or '-', flag))
    bad += bool(flag)
bounces = sum(1 for L in M.reference(M.CASE['row/boxes'])['levels'][:M.REPS] if L['n_live'] > 0)
for depth, chart, kern in M.ORDERED:
    n = calls.pop(squeeze(kern), 0)
    flag = '' if n == bounces else '   <-- prediction and trace disagree'
    print('%-44s %6d %8d  row under chain(%d)%s%s' % (kern, n, bounces, depth, ', a chart map on the scene' if chart else '', flag))
    bad += bool(flag)
for b in M.UNREACHABLE:
    if b not in M.ALL_INSTANCES:
        print('%-44s %6s %8s  unreachable: %s' % (b, '-', '-', M.UNREACHABLE[b]))
for k, n in sorted(calls.items()):
    print('%-44s %6d  not one of the %d   <-- unexpected' % (k, n, len(M.ALL_INSTANCES)))
    bad += 1
sys.exit(1 if bad else 0)
