"""profiles/serve_scene_budget.txt from the output of

    python -m pytest tests/test_gpu_serve_scene.py -m gpu -q -s > LOG
    python tools/serve_scene_budget_report.py LOG > profiles/serve_scene_budget.txt

One line per case of the scene route (risp_serve_scene_stats / _finish / _u8): the bytes that differ from the float64 reference
(tests/serve_scene_reference.py), their share, the largest tie distance among them (in codes), the input's own shares of
inner-tie pixels and of bytes under the +-1 rule (caps: serve_reference.TIE_CAP, FINAL_CAP), and for the table cases the
kernels' constants against the float64 statistics as a fraction of their bound (serve_scene_cases.CONST_TAU)."""
import os
import re
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), d) for d in ('tests', 'oracle')]
from serve_reference import FINAL_CAP, TIE_CAP  # noqa: E402

LINE = re.compile(r'SERVE_SCENE (.+?)\s+draws (\d+) differ\s+(\d+) share (\S+) worst-tie (\S+) inner-tie-pixels (\S+) final-tie-bytes (\S+) '
                  r'(?:consts/bound (\S+)|differ-from-composed (\d+)) (OK|OUTSIDE THE RULE)')


def main(path):
    rows = [m.groups() for m in (LINE.search(line) for line in open(path)) if m]
    outside = sum(r[9] != 'OK' for r in rows)
    over = sum(float(r[5]) > TIE_CAP or float(r[6]) > FINAL_CAP for r in rows)
    print('The scene route (risp_serve_scene_stats, _finish, _u8 and serve(fast_scene=True)) against the float64 reference from the')
    print('sensor frame: tests/test_gpu_serve_scene.py, one MI355X; %d cases, %d outside the rule, %d over a cap.' % (len(rows), outside, over))
    print('Caps: %g of a case\'s pixels at an inner tie, %g of its bytes under the +-1 rule.' % (TIE_CAP, FINAL_CAP))
    print('%d cases differ from the reference in at least one byte; the largest tie distance among all differing bytes is %.3e codes;' % (
        sum(int(r[2]) > 0 for r in rows), max([float(r[4]) for r in rows] or [0.0])))
    print('the constants reach at most %.3f of their bound.' % max([float(r[7]) for r in rows if r[7]] or [0.0]))
    print()
    print('%-92s %5s %7s %10s %10s %10s %10s %12s' % ('case', 'draws', 'differ', 'share', 'worst tie', 'inner ties', '+-1 bytes', 'consts/bound'))
    for what, draws, differ, share, worst, inner, loose, cst, comp, verdict in rows:
        print('%-92s %5s %7s %10s %10s %10s %10s %12s%s' % (what, draws, differ, share, worst, inner, loose,
                                                          cst or 'vs composed %s' % comp, '' if verdict == 'OK' else '  <-- ' + verdict))


if __name__ == '__main__':
    main(sys.argv[1])
