"""Summarise the measured pairs of tests/test_gpu_train_step_space.py.

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_train_step_space.py -m gpu -s -q > run.log
    python tools/train_step_budget_report.py run.log profiles/train_step_space_budget.txt [case,case,... to leave out]

Reads the BUDGET lines conftest.ErrorBudget prints (hip = max|hip - fp64| / max|fp64|, ref32 = the same for the float32
restatement) and writes, per family and geometry class, the largest hip / ref32 and the largest hip; then one line per
judged tensor of the table, one line per tensor and RUN for the twelve-step runs (worst step), one per tensor for the
ties and the walk.  The calls the refusal tests make after a refusal are left out."""
import re
import sys

FAMILIES = ['outputs', 'losses', 'param grads', 'first moments', 'second moments', 'updates', 'blocks']
CLASSES = ['bx1-idle', 'bx1-full', 'ragged', 'bx8', 'bx32', 'stride2', 'stride8', 'batch', 'headline']
LINE = re.compile(r'BUDGET (\S+) \[(\S+)\] (.*?)\s+hip (\S+)\s+ref32 (\S+)\s+ratio\s+\S+\s+family (.*?)\s+\S+e[-+]\d+\s*(<-- OVER)?')


def main(log, out_path, leave_out=''):
    leave_out = [c for c in leave_out.split(',') if c]
    rows = []                                # (case, class, step or 0, tensor, hip, ref32, family, over)
    for line in open(log):
        for m in LINE.finditer(line):
            case, geo, label, hip, ref, fam, over = m.groups()
            if case == 'refusal' or case in leave_out:
                continue
            step = re.match(r'step (\d+) (.*)', label)
            rows.append((case, geo, int(step.group(1)) if step else 0, step.group(2) if step else label, float(hip), float(ref),
                         fam.strip(), bool(over)))
    ratio = lambda r: r[4] / r[5]
    out = []
    w = out.append
    w('risp_chain_train_step against the float64 restatement: tests/test_gpu_train_step_space.py with RISP_BUDGET_REPORT=1')
    w('table (%d cases), walk (%d seeds), twelve-step runs (%s), ties (%s): %d judged tensors, %d over their bound' % (
        len({r[0] for r in rows if not r[2] and not r[0].startswith(('walk', 'tie'))}), len({r[0] for r in rows if r[0].startswith('walk')}),
        ', '.join(sorted({r[0] for r in rows if r[2]})), ', '.join(sorted({r[0] for r in rows if r[0].startswith('tie')})),
        len(rows), sum(r[7] for r in rows)))
    if leave_out:
        w('left out (not measured on the inputs of the present table): %s' % ', '.join(leave_out))
    w('hip = max|hip - fp64| / max|fp64| of a tensor, ref32 = the same for the restatement in float32, ratio = hip / ref32')
    w('(a tensor the float32 restatement reproduces exactly, ref32 == 0, has no ratio and is counted apart)')
    w('')
    w('largest ratio and largest hip per family and geometry class')
    for fam in FAMILIES:
        w('')
        w(fam)
        for geo in CLASSES + ['all']:
            sel = [r for r in rows if r[6] == fam and geo in (r[1], 'all')]
            if not sel:
                w('  %-9s -' % geo)
                continue
            fin, zero = [r for r in sel if r[5] > 0], [r for r in sel if r[5] == 0]
            big = max(sel, key=lambda r: r[4])
            name = lambda r: '%s%s %s' % (r[0], ' step %d' % r[2] if r[2] else '', r[3])
            s = '  %-9s n=%-4d' % (geo, len(sel))
            if fin:
                worst = max(fin, key=ratio)
                s += ' ratio %6.2f (hip %.2e, ref32 %.2e) %s;' % (ratio(worst), worst[4], worst[5], name(worst))
            s += ' largest hip %.2e (ref32 %.2e) %s' % (big[4], big[5], name(big))
            if zero:
                s += '; ref32 == 0 on %d, largest hip there %.2e' % (len(zero), max(r[4] for r in zero))
            w(s)
    w('')
    w('table, first call of each case: one line per judged tensor')
    for r in rows:
        if not r[2] and not r[0].startswith(('walk', 'tie')):
            w('  %-11s %-9s %-14s hip %.2e ref32 %.2e' % (r[0], r[1], r[3], r[4], r[5]))
    w('')
    w('twelve-step runs: per tensor the step with the largest hip, and the range of ref32 over the steps')
    for case in sorted({r[0] for r in rows if r[2]}):
        for tensor in dict.fromkeys(r[3] for r in rows if r[0] == case and r[2]):
            sel = [r for r in rows if r[0] == case and r[2] and r[3] == tensor]
            big = max(sel, key=lambda r: r[4])
            w('  %-11s %-14s %2d steps, largest hip %.2e at step %2d (ref32 %.2e there); ref32 %.2e .. %.2e' % (
                case, tensor, len(sel), big[4], big[2], big[5], min(r[5] for r in sel), max(r[5] for r in sel)))
    w('')
    w('ties and walk: one line per judged tensor')
    for r in rows:
        if r[0].startswith(('walk', 'tie')):
            w('  %-11s %-9s %-14s hip %.2e ref32 %.2e' % (r[0], r[1], r[3], r[4], r[5]))
    with open(out_path, 'w') as f:
        f.write('\n'.join(out) + '\n')
    print('%d judged tensors -> %s' % (len(rows), out_path))


if __name__ == '__main__':
    main(*sys.argv[1:4])
