"""profiles/serve_space_budget.txt from the output of

    python -m pytest tests/test_gpu_serve_space.py -m gpu -q -s > LOG
    python tools/serve_space_budget_report.py LOG > profiles/serve_space_budget.txt

and profiles/serve_denoise_space_budget.txt in the same way from tests/test_gpu_serve_denoise_space.py (its lines carry the
tag SERVE_DENOISE_SPACE; the tag found in the log chooses the heading).

One line per case: the bytes that differ from the float64 reference (tests/serve_reference.py), their share, the largest tie
distance among them (in codes: how far from a decision boundary the reference was where the kernel decided otherwise), and
the input's own shares of inner-tie pixels and of bytes under the +-1 rule (caps: serve_reference.TIE_CAP, FINAL_CAP)."""
import os
import re
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), d) for d in ('tests', 'oracle')]
from serve_reference import FINAL_CAP, TIE_CAP  # noqa: E402

LINE = re.compile(r'(SERVE_SPACE|SERVE_DENOISE_SPACE) (.+?)\s+draws (\d+) differ\s+(\d+) share (\S+) worst-tie (\S+) inner-tie-pixels (\S+) final-tie-bytes (\S+) (OK|OUTSIDE THE RULE)')


def main(path):
    rows = [m.groups() for m in (LINE.search(line) for line in open(path)) if m]
    tags = {r[0] for r in rows}
    assert len(tags) <= 1, 'one log, one suite: %s' % sorted(tags)
    rows = [r[1:] for r in rows]
    outside = sum(r[7] != 'OK' for r in rows)
    over = sum(float(r[5]) > TIE_CAP or float(r[6]) > FINAL_CAP for r in rows)
    if tags == {'SERVE_DENOISE_SPACE'}:
        print('risp_serve_denoise_u8, the composed route of the same lists (rows "composed ...") and serve() / serve(fast_denoise=True) of the')
        print('pipelines against the float64 reference from the sensor frame: tests/test_gpu_serve_denoise_space.py, one MI355X;')
        print('%d rows, %d outside the rule, %d over a cap.' % (len(rows), outside, over))
    else:
        print('risp_serve_u8, risp_serve_u8_cfa, risp_serve_classical_u8 and serve() of the pipelines against the float64 reference from')
        print('the sensor frame: tests/test_gpu_serve_space.py, one MI355X; %d cases, %d outside the rule, %d over a cap.' % (len(rows), outside, over))
    print('Caps: %g of a case\'s pixels at an inner tie, %g of its bytes under the +-1 rule.' % (TIE_CAP, FINAL_CAP))
    print('%d cases differ from the reference in at least one byte; the largest tie distance among all differing bytes is %.3e codes.' % (
        sum(int(r[2]) > 0 for r in rows), max([float(r[4]) for r in rows] or [0.0])))
    print()
    print('%-100s %5s %7s %10s %10s %10s %10s' % ('case', 'draws', 'differ', 'share', 'worst tie', 'inner ties', '+-1 bytes'))
    for what, draws, differ, share, worst, inner, loose, verdict in rows:
        print('%-100s %5s %7s %10s %10s %10s %10s%s' % (what, draws, differ, share, worst, inner, loose, '' if verdict == 'OK' else '  <-- ' + verdict))


if __name__ == '__main__':
    main(sys.argv[1])
