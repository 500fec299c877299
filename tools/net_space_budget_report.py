"""profiles/net_space_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_net_space.py -m gpu -q -s > LOG
    python tools/net_space_budget_report.py LOG > profiles/net_space_budget.txt

One line per family and form with the tensor nearest to the bar, then one line per case and tensor: the device's error against the
float64 referee relative to max|ref|, the error of the fp32 CPU restatement of the same graph with the same ReLU decisions (the
yardstick), their ratio, the decisions of the case that differ from float64's own, and the conv entries that ran."""
import re
import sys

LINE = re.compile(r'NETSPACE (\S+) \| (\S+) dev (\S+) fp32 (\S+) flips (\d+) entries (\S*)')
BAR = 1e-4


def main(path):
    rows = []
    for line in open(path):
        m = LINE.search(line)
        if m:
            rows.append((m.group(1), m.group(2), float(m.group(3)), None if m.group(4) == '-' else float(m.group(4)), int(m.group(5)), m.group(6)))
    cases = sorted({r[0] for r in rows}, key=[r[0] for r in rows].index)
    over = sum(not r[2] <= BAR for r in rows)
    print('convnets.py\'s autograd Functions against the float64 referee: tests/test_gpu_net_space.py with RISP_BUDGET_REPORT=1, one MI355X;')
    print('%d cases, %d tensors, %d over the bar of %.0e.  dev / fp32 = max|got - ref64| / max|ref64| of the device and of the fp32 CPU restatement' % (
        len(cases), len(rows), over, BAR))
    print('with the same ReLU decisions; flips = decisions of the case that differ from float64\'s own (bounded by the forward check alone).')
    print('\nper family and form: tensors, the largest device error, the fp32 yardstick on that tensor, the largest ratio to the yardstick')
    fam = lambda r: re.match(r'[a-z0-9_]+-[a-z]+(?:-[a-z]+)?(?=-(?:P\d|x\d|\d))', r[0]).group(0)      # kind-form of the case id
    for f in sorted({fam(r) for r in rows}):
        mine = [r for r in rows if fam(r) == f]
        worst = max(mine, key=lambda r: r[2])
        ratio = max((r[2] / r[3] for r in mine if r[3]), default=0.0)
        print('  %-28s n=%-4d max %.2e  fp32 %s  largest dev/fp32 %5.2f  flips %-3d (%s | %s)' % (
            f, len(mine), worst[2], '%.2e' % worst[3] if worst[3] is not None else '-', ratio, sum({r[0]: r[4] for r in mine}.values()), worst[0], worst[1]))
    print('\nper case and tensor')
    for case, what, e, e32, flips, ent in rows:
        print('  %-58s %-22s dev %.2e  fp32 %s  ratio %s  flips %-2d %s%s' % (
            case, what, e, '%.2e' % e32 if e32 is not None else '-       ', '%5.2f' % (e / e32) if e32 else '    -', flips, ent,
            '' if e <= BAR else '  <-- OVER'))


if __name__ == '__main__':
    main(sys.argv[1])
