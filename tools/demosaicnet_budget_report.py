"""profiles/demosaicnet_space_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_demosaicnet_space.py -m gpu -q -s > LOG
    python tools/demosaicnet_budget_report.py LOG > profiles/demosaicnet_space_budget.txt

One line per form with the tensor nearest to the bar, then one line per row and tensor: the device's error against the float64 referee
(network rows: relative to max|ref|, bar 1e-4; kernel rows: relative to the RMS of ref, bar 1e-5), the error of the fp32 CPU
restatement of the same graph with the same ReLU decisions (the yardstick), their ratio, the decisions of the row that differ from
float64's own, the undecided head units (at most 4), and the conv entries that ran."""
import re
import sys

LINE = re.compile(r'DMSPACE (\S+) \| (\S+) dev (\S+) fp32 (\S+) flips (\d+) undecided (\d+) entries (\S*)')
BAR, KERNEL_BAR, MAX_UNDECIDED = 1e-4, 1e-5, 4


def main(path):
    rows = []
    for line in open(path):
        m = LINE.search(line)
        if m:
            rows.append((m.group(1), m.group(2), float(m.group(3)), None if m.group(4) == '-' else float(m.group(4)), int(m.group(5)),
                         int(m.group(6)), m.group(7)))
    bar = lambda r: KERNEL_BAR if r[0].startswith('kernel') else BAR
    cases = sorted({r[0] for r in rows}, key=[r[0] for r in rows].index)
    over = sum(not r[2] <= bar(r) for r in rows)
    print('DemosaicNet against the float64 referee: tests/test_gpu_demosaicnet_space.py with RISP_BUDGET_REPORT=1, one MI355X;')
    print('%d rows, %d tensors, %d over the bar (%.0e of max|ref| for the network rows, %.0e of the RMS of ref for the kernel rows), %d rows with more' % (
        len(cases), len(rows), over, BAR, KERNEL_BAR, len({r[0] for r in rows if r[5] > MAX_UNDECIDED})))
    print('than %d undecided head units.  dev / fp32 = the error of the device and of the fp32 CPU restatement with the same ReLU decisions;' % MAX_UNDECIDED)
    print('flips = decisions of the row that differ from float64\'s own; und = head units within TAU_HEAD of zero, enumerated.')
    print('\nper form: tensors, the largest device error, the fp32 yardstick on that tensor, the largest ratio to the yardstick')
    form = lambda r: r[0].split('-')[0]
    for f in sorted({form(r) for r in rows}):
        mine = [r for r in rows if form(r) == f]
        worst = max(mine, key=lambda r: r[2])
        ratio = max((r[2] / r[3] for r in mine if r[3]), default=0.0)
        print('  %-8s n=%-4d max %.2e  fp32 %s  largest dev/fp32 %5.2f  flips %-3d und %-2d (%s | %s)' % (
            f, len(mine), worst[2], '%.2e' % worst[3] if worst[3] is not None else '-', ratio, sum({r[0]: r[4] for r in mine}.values()),
            max(r[5] for r in mine), worst[0], worst[1]))
    print('\nper row and tensor')
    for case, what, e, e32, flips, und, ent in rows:
        print('  %-40s %-32s dev %.2e  fp32 %s  ratio %s  flips %-2d und %d %s%s' % (
            case, what, e, '%.2e' % e32 if e32 is not None else '-       ', '%5.2f' % (e / e32) if e32 else '    -', flips, und, ent,
            '' if e <= bar((case,)) else '  <-- OVER'))


if __name__ == '__main__':
    main(sys.argv[1])
