"""profiles/conv_space_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_conv_space.py -m gpu -q -s > LOG
    python tools/conv_budget_report.py LOG > profiles/conv_space_budget.txt

One line per entry point with the case nearest to its bound and, for the fp32 entries, the largest e_gpu / E32, then one line per case:
the entry ``conv`` launched, the rms and the largest error against the float64 restatement relative to max|ref|, the error E32 of the
CPU float32 yardstick of the same algorithm class, the bound (the bar of the kernel's own file for the split-precision entries,
min(2 * E32, 1e-4) + 4e-6 for the fp32 ones) and e_gpu / E32."""
import re
import sys

LINE = re.compile(r'CONV(?:SPACE|BATCH) (.+?)\s+\| (\S+)\s+rms (\d\S+) max (\d\S+) E32 (\d\S+) bound (\d\S+) ratio (\d\S+)')
SPLIT = ('risp_conv2d_f16x2', 'risp_conv2d_thin5', 'risp_conv2d_toep_first', 'risp_conv2d_toep_first_exact')


def main(path):
    rows = []
    for line in open(path):
        m = LINE.search(line)
        if m:
            rows.append((m.group(1), m.group(2)) + tuple(float(m.group(i)) for i in range(3, 8)))
    over = sum(r[3] > r[5] for r in rows)
    print('convnets.conv against the float64 restatement: tests/test_gpu_conv_space.py with RISP_BUDGET_REPORT=1, one MI355X;')
    print('%d cases, %d over their bound.  rms / max = error relative to max|ref| of the case; E32 = the CPU float32 yardstick of the entry\'s' % (len(rows), over))
    print('algorithm class on the same case; bound = the bar of the kernel\'s own test file (split precision) or min(2 * E32, 1e-4) + 4e-6 (fp32).')
    print('\nper entry: cases, the largest max error with its bound, the largest ratio to the bound; fp32 entries: e_gpu / E32 (median, largest)')
    for entry in sorted({r[1] for r in rows}):
        mine = [r for r in rows if r[1] == entry]
        worst = max(mine, key=lambda r: r[3] / r[5])
        big = max(mine, key=lambda r: r[3])
        ratios = sorted(r[6] for r in mine)
        tail = '' if entry in SPLIT else '  e_gpu/E32 median %.2f max %.2f' % (ratios[len(ratios) // 2], ratios[-1])
        print('  %-28s n=%-4d max %.2e (bound %.2e)  nearest its bound %.2f (%s)%s' % (entry, len(mine), big[3], big[5], worst[3] / worst[5], worst[0], tail))
    print('\nper case')
    for name, entry, rms, mx, e32, bound, ratio in rows:
        print('  %-72s %-28s rms %.2e  max %.2e  E32 %.2e  bound %.2e  e_gpu/E32 %.2f%s' % (name, entry, rms, mx, e32, bound, ratio,
                                                                                        '  <-- OVER' if mx > bound else ''))


if __name__ == '__main__':
    main(sys.argv[1])
