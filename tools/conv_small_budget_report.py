"""profiles/conv_small_space_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_conv_small_space.py -m gpu -q -s > LOG
    python tools/conv_small_budget_report.py LOG > profiles/conv_small_space_budget.txt

One line per route with the case nearest to its bar, then one line per case: the entry point conv_small launched, the rms and the
largest error against the float64 restatement relative to max|ref|, the bar of the kernel's own file and the ratio to it."""
import re
import sys

LINE = re.compile(r'CONVSMALL (.+?)\s+\| (\S+)\s+rms (\d\S+) max (\d\S+) bar (\d\S+)')


def main(path):
    rows = []
    for line in open(path):
        m = LINE.search(line)
        if m:
            rows.append((m.group(1), m.group(2), float(m.group(3)), float(m.group(4)), float(m.group(5))))
    over = sum(mx >= bar for _, _, _, mx, bar in rows)
    print('convnets.conv_small against the float64 restatement: tests/test_gpu_conv_small_space.py with RISP_BUDGET_REPORT=1, one MI355X;')
    print('%d cases, %d over their bar.  rms / max = error relative to max|ref| of the case; bar = the bar of the kernel\'s own test file.' % (len(rows), over))
    print('\nper route: cases, the largest max error, the largest ratio to the bar')
    for entry in sorted({r[1] for r in rows}):
        mine = [r for r in rows if r[1] == entry]
        worst = max(mine, key=lambda r: r[3] / r[4])
        print('  %-24s n=%-4d max %.2e  bar %.1e  ratio %.2f  (%s)' % (entry, len(mine), worst[3], worst[4], worst[3] / worst[4], worst[0]))
    print('\nper case')
    for name, entry, rms, mx, bar in rows:
        print('  %-70s %-24s rms %.2e  max %.2e  bar %.1e  ratio %.2f%s' % (name, entry, rms, mx, bar, mx / bar, '  <-- OVER' if mx >= bar else ''))


if __name__ == '__main__':
    main(sys.argv[1])
