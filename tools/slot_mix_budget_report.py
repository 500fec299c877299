"""profiles/slot_mix_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_slot_mix_space.py -m gpu -q -s > LOG
    python tools/slot_mix_budget_report.py LOG > profiles/slot_mix_budget.txt

One line per case and family instead of one per judged tensor (the parameter gradients are judged row by row: 600 rows
per operand in the largest batch): how many tensors, the largest hip error with the restatement's own fp32 error on that
tensor and the bound conftest.ErrorBudget gave it, and the largest hip / ref32 among the tensors whose hip error is above
1e-7 (below that a ratio compares two roundings)."""
import re
import sys

LINE = re.compile(r'BUDGET (.+?)\s+hip (\S+)\s+ref32 (\S+)\s+ratio\s+\S+\s+family (.+?)\s+(\d\.\d\de[-+]\d\d)(.*)$')
FAMILIES = ('outputs', 'architecture terms', 'input gradients', 'operand gradients', 'parameter gradients')


def main(path):
    groups, over, total = {}, 0, 0
    for line in open(path):
        m = LINE.search(line.rstrip())
        if not m:
            continue
        what, hip, ref, family, fam_ref, tail = m.group(1), float(m.group(2)), float(m.group(3)), m.group(4), float(m.group(5)), m.group(6)
        case = re.match(r'(mix \S+|after a refusal|\S+ autograd|\S+)', what).group(1)
        label = what[len(case):].strip()
        bound = max(min(2.0 * fam_ref, 1e-4), 2.0 * ref if ref > 1e-4 else 0.0) + 4e-6
        total, over = total + 1, over + ('OVER' in tail)
        g = groups.setdefault((case, family), dict(n=0, hip=(-1.0, 0.0, 0.0, ''), ratio=(0.0, '')))
        g['n'] += 1
        g['hip'] = max(g['hip'], (hip, ref, bound, label))
        if hip > 1e-7 and ref > 0:
            g['ratio'] = max(g['ratio'], (hip / ref, label))
    print('risp_slot_mix_fwd / _bwd and risp_mix_fwd / _bwd against the float64 restatement: tests/test_gpu_slot_mix_space.py with')
    print('RISP_BUDGET_REPORT=1, one MI355X; %d judged tensors, %d over their bound.  hip = max|hip - fp64| / max|fp64| of a tensor,' % (total, over))
    print('ref32 = the same for the restatement in float32, bound = min(2 x ref32 of the family in that call, 1e-4) + 4e-6.')
    print('"NAME autograd": the same case through functional.slot_mix; "mix NAME": risp_mix directly.')
    for family in FAMILIES:
        rows = [(case, g) for (case, fam), g in groups.items() if fam == family]
        if not rows:
            continue
        worst = max(rows, key=lambda r: r[1]['hip'][0] / r[1]['hip'][2])
        print('\n%s: %d tensors; nearest to its bound %s %s at %.0f %% of it' % (
            family, sum(g['n'] for _, g in rows), worst[0], worst[1]['hip'][3], 100 * worst[1]['hip'][0] / worst[1]['hip'][2]))
        for case, g in rows:
            hip, ref, bound, label = g['hip']
            ratio = ', largest ratio %.2f (%s)' % g['ratio'] if g['ratio'][0] else ''
            print('  %-34s n=%-5d hip %.2e (ref32 %.2e, bound %.2e) %s%s' % (case, g['n'], hip, ref, bound, label, ratio))


if __name__ == '__main__':
    main(sys.argv[1])
