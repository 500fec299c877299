"""profiles/wgrad_space_budget.txt from the output of

    RISP_BUDGET_REPORT=1 python -m pytest tests/test_gpu_wgrad_space.py -m gpu -q -s > LOG
    python tools/wgrad_budget_report.py LOG > profiles/wgrad_space_budget.txt

One line per form of risp_conv2d_wgrad (k1, plain, thin_in, thin_out; 'shortcut+' in front where conv_wgrad sends the constant planes of a
first layer through risp_rect_sums) with the case nearest to the bar, then one line per case: the form launched, the rms and the largest
error of dW against the float64 restatement relative to max|ref|, the bar and the ratio to it."""
import re
import sys

LINE = re.compile(r'WGRAD (.+?)\s+\| (\S+)\s+rms (\d\S+) max (\d\S+) bar (\d\S+)')


def main(path):
    rows = []
    for line in open(path):
        m = LINE.search(line)
        if m:
            rows.append((m.group(1), m.group(2), float(m.group(3)), float(m.group(4)), float(m.group(5))))
    over = sum(mx > bar for _, _, _, mx, bar in rows)
    print('convnets.conv_wgrad against the float64 restatement: tests/test_gpu_wgrad_space.py with RISP_BUDGET_REPORT=1, one MI355X;')
    print('%d cases, %d over the bar.  rms / max = error of dW relative to max|ref| of the case; bar = 3e-6, that of the fp32-accumulating conv kernels.' % (len(rows), over))
    print('\nper form: cases, the largest max error, its ratio to the bar')
    for form in sorted({r[1] for r in rows}):
        mine = [r for r in rows if r[1] == form]
        worst = max(mine, key=lambda r: r[3] / r[4])
        print('  %-18s n=%-4d max %.2e  bar %.1e  ratio %.2f  (%s)' % (form, len(mine), worst[3], worst[4], worst[3] / worst[4], worst[0]))
    print('\nper case')
    for name, form, rms, mx, bar in rows:
        print('  %-56s %-18s rms %.2e  max %.2e  bar %.1e  ratio %.2f%s' % (name, form, rms, mx, bar, mx / bar, '  <-- OVER' if mx > bar else ''))


if __name__ == '__main__':
    main(sys.argv[1])
