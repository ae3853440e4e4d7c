"""
tools/asm_compare.py on tiny hand-written `make asm` trees: an identical pair (labels numbered otherwise, other comments and
.loc lines), a pair in which one figure of one kernel changed, a pair in which a kernel moved to another unit unchanged, and a
pair in which one instruction changed.  CPU only.
"""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIGURES = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Dynamic Stack', 'Occupancy [waves/SIMD]', 'SGPRs Spill',
           'VGPRs Spill', 'LDS Size [bytes/block]')


def tool():
    spec = importlib.util.spec_from_file_location('asm_compare', os.path.join(ROOT, 'tools', 'asm_compare.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def remark(name, **changed):
    fig = dict(zip(FIGURES, ('24', '12', '0', '0', 'False', '8', '0', '0', '0')))
    fig.update(changed)
    head = 'a.hip:7:1: remark: '
    return head + 'Function Name: %s [-Rpass-analysis=kernel-resource-usage]\n' % name + ''.join(
        head + '    %s: %s [-Rpass-analysis=kernel-resource-usage]\n' % kv for kv in fig.items())


def listing(name, first_label=0, op='v_add_f64', line=10):
    a, b = '.LBB%d_1' % first_label, '.LBB%d_2' % first_label
    return ('\t.globl\t{n}\n\t.type\t{n},@function\n{n}:                                   ; @{n}\n'
            '\t.cfi_startproc\n\t.loc\t1 {ln} 0                          ; a.hip:{ln}:0\n'
            '\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n{a}:                                 ; %loop\n'
            '\t{op} v[0:1], v[0:1], v[2:3]\n\ts_cbranch_scc1 {a}\n{b}:\n\ts_endpgm\n'
            '.Lfunc_end{f}:\n\t.size\t{n}, .Lfunc_end{f}-{n}\n\t.cfi_endproc\n'
            '\t.section\t.rodata\n\t.amdhsa_kernel {n}\n\t.end_amdhsa_kernel\n\t.text\n').format(n=name, a=a, b=b, op=op, ln=line, f=first_label)


def write_tree(root, units):
    """units: {unit: [(kernel, remark keywords, listing keywords)]}"""
    os.makedirs(root)
    for unit, kernels in units.items():
        with open(os.path.join(root, unit + '.resources.txt'), 'w') as f:
            f.write('clang: warning: something unrelated\n' + ''.join(remark(k, **r) for k, r, _ in kernels))
        with open(os.path.join(root, unit + '.s'), 'w') as f:
            f.write('\t.text\n' + ''.join(listing(k, **l) for k, _, l in kernels))


def run(tmp_path, parent, change):
    write_tree(str(tmp_path / 'p'), parent)
    write_tree(str(tmp_path / 'c'), change)
    out = io.StringIO()
    status = tool().compare(str(tmp_path / 'p'), str(tmp_path / 'c'), out)
    return status, out.getvalue()


PARENT = {'u_one': [('k_a', {}, {}), ('k_b', {}, {'first_label': 1})], 'u_two': [('k_c', {}, {})]}


def test_an_identical_pair_agrees_whatever_its_labels_comments_and_lines(tmp_path):
    change = {'u_one': [('k_b', {}, {'first_label': 0, 'line': 99}), ('k_a', {}, {'first_label': 5, 'line': 3})], 'u_two': [('k_c', {}, {})]}
    status, out = run(tmp_path, PARENT, change)
    assert status == 0, out
    assert 'u_one         parent    2 kernels, change    2' in out
    assert 'parent names 3 change names 3' in out
    assert 'figures per remark: [9]' in out
    assert 'names whose figures differ: 0' in out
    assert 'names that changed unit: 0' in out
    assert 'kernels whose instruction text differs: 0 of 3' in out


def test_a_changed_figure_is_named(tmp_path):
    change = {'u_one': [('k_a', {}, {}), ('k_b', {'VGPRs': '13'}, {'first_label': 1})], 'u_two': [('k_c', {}, {})]}
    status, out = run(tmp_path, PARENT, change)
    assert status == 1
    assert 'names whose figures differ: 1' in out
    assert "k_b\n" in out and "'VGPRs': '13'" in out and "'VGPRs': '12'" in out
    assert 'kernels whose instruction text differs: 0 of 3' in out


def test_a_kernel_that_moved_between_units_is_compared_with_itself(tmp_path):
    change = {'u_one': [('k_a', {}, {})], 'u_two': [('k_c', {}, {}), ('k_b', {}, {'first_label': 1})]}
    status, out = run(tmp_path, PARENT, change)
    assert status == 0, out
    assert 'u_one         parent    2 kernels, change    1' in out
    assert 'u_two         parent    1 kernels, change    2' in out
    assert 'only at the parent: []' in out and 'new on the change: []' in out
    assert 'names that changed unit: 1' in out and 'k_b  u_one -> u_two' in out
    assert 'kernels whose instruction text differs: 0 of 3' in out


def test_changed_text_a_lost_name_and_a_name_listed_twice_are_found(tmp_path):
    change = {'u_one': [('k_a', {}, {'op': 'v_mul_f64'}), ('k_c', {}, {})], 'u_two': [('k_c', {}, {}), ('k_d', {}, {})]}
    status, out = run(tmp_path, PARENT, change)
    assert status == 1
    assert "only at the parent: ['k_b']" in out and "new on the change: ['k_d']" in out
    assert "listed more than once on the change: ['k_c']" in out
    assert 'kernels whose instruction text differs: 1 of 2' in out and '   k_a (' in out
