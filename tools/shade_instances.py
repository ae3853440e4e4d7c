"""One line per shading kernel instance of the streaming engine (the 26 of trc_stream_form_shade) from a rocprofv3 --kernel-trace --stats
output directory of tests/test_gpu_shade_instances.py: its calls in the trace, and the cases of tests/shade_cases.py whose restated
sums predict it.  The trace is of the whole file, so the cases are the prediction's, not read from the trace: what ties them to
the calls is the count -- every streaming call launches each of its shading kernels once per repetition (shade_cases.REPS), and the
`expected` column gives the calls the predicted cases of the test file add up to.  A line whose calls differ from that, or a shading
kernel launched that is not one of the 26, is flagged: the prediction is then wrong.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m pytest tests/test_gpu_shade_instances.py -q
    python tools/shade_instances.py OUT > profiles/shade_instances.txt
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import shade_cases as sc        # noqa: E402

squeeze = lambda s: re.sub(r'\s+', '', s)
calls = {}
for fn in glob.glob(sys.argv[1] + '/**/*kernel_stats.csv', recursive=True):
    with open(fn) as f:
        for r in csv.DictReader(f):
            m = re.search(r'k_s_shade(_c|_x)?<[^>]*>', r['Name'])
            if m:
                calls[squeeze(m.group(0))] = calls.get(squeeze(m.group(0)), 0) + int(r['Calls'])
predicted = {}
for name in sorted(sc.CASES):
    for inst in sc.case(name).instances:
        predicted.setdefault(squeeze(inst), []).append(name)
# streaming calls per case in tests/test_gpu_shade_instances.py: the source (or carry) bundle, the given rays, the two knob variants
n_calls = dict((n, 1 + (n in sc.GIVEN) + 2 * (n in sc.KNOBS)) for n in sc.CASES)
print('%-42s %6s %8s  %s' % ('instance', 'calls', 'expected', 'cases predicted to launch it (tests/shade_cases.py)'))
bad = 0
for inst in sc.ALL_INSTANCES:
    k = squeeze(inst)
    n, cases = calls.pop(k, 0), predicted.get(k, [])
    want = sc.REPS * sum(n_calls[c] for c in cases)
    flag = '' if n == want else '   <-- prediction and trace disagree'
    bad += bool(flag)
    print('%-42s %6d %8d  %s%s' % (inst, n, want, ' '.join(cases) if cases else '-', flag))
for k, n in sorted(calls.items()):
    print('%-42s %6d  not one of the 26   <-- unexpected' % (k, n))
    bad += 1
sys.exit(1 if bad else 0)
