"""No GPU: what tools/serve_bench.py decides for the eighteen tools/bench_serve*.py scripts - the statistics and the rule behind the
measured tables of pipeline_fusion on hand-worked lists, the round runner under a fake clock, the verdict line against the five
recorded profiles and against the reader the tests use (tests/serve_verdicts.py), and that no script grew its own copy again."""
import ast
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, 'tools'))              # behind everything else: tools/ must not shadow a test helper
import serve_bench as SB  # noqa: E402
from serve_verdicts import read_verdict  # noqa: E402


def test_median_is_the_upper_median_and_spread_is_max_minus_min():
    assert SB.median([3.0, 1.0, 2.0]) == 2.0
    assert SB.median([4.0, 1.0, 3.0, 2.0]) == 3.0            # even length: the upper of the two middle values, not 2.5
    assert SB.median([5.0]) == 5.0
    assert SB.median([1.0, 9.0]) == 9.0
    assert SB.spread([3.0, 1.0, 2.0]) == 2.0
    assert SB.spread([5.0]) == 0.0


def test_beats_asks_for_more_than_the_larger_of_the_two_spreads():
    # medians 10 and 14, spreads 2 and 1: a gain of 4 over a noise of 2
    assert SB.margin([9.0, 10.0, 11.0], [13.5, 14.0, 14.5]) == (4.0, 2.0)
    assert SB.beats([9.0, 10.0, 11.0], [13.5, 14.0, 14.5])
    assert not SB.beats([13.5, 14.0, 14.5], [9.0, 10.0, 11.0])
    # a gain of exactly the larger spread does not beat: medians 10 and 12, spreads 2 and 1
    assert SB.margin([9.0, 10.0, 11.0], [11.5, 12.0, 12.5]) == (2.0, 2.0)
    assert not SB.beats([9.0, 10.0, 11.0], [11.5, 12.0, 12.5])
    # a gain of 3 that clears the fast leg's spread (1) but not the slow leg's (4) does not beat, and neither the other way round
    assert not SB.beats([9.5, 10.0, 10.5], [11.0, 13.0, 15.0])
    assert not SB.beats([8.0, 10.0, 12.0], [12.5, 13.0, 13.5])
    # equal legs do not beat each other
    assert not SB.beats([10.0, 11.0], [10.0, 11.0])


def _clock():
    calls = []

    def timed(leg, reps):
        calls.append((leg, reps))
        return float(len(calls))
    return calls, timed


def test_rounds_are_interleaved_in_dict_order():
    calls, timed = _clock()
    res = SB.rounds_of({'b': 'B', 'a': 'A', 'c': 'C'}, 7, 2, False, timed)
    assert calls == [('B', 7), ('A', 7), ('C', 7)] * 2       # every leg once per round, not leg by leg
    assert res == {'b': [1.0, 4.0], 'a': [2.0, 5.0], 'c': [3.0, 6.0]}
    assert list(res) == ['b', 'a', 'c']


def test_a_warm_round_is_one_more_visit_per_leg_and_is_not_kept():
    calls, timed = _clock()
    res = SB.rounds_of({'b': 'B', 'a': 'A'}, 3, 2, True, timed)
    assert calls == [('B', 3), ('A', 3)] * 3
    assert res == {'b': [3.0, 5.0], 'a': [4.0, 6.0]}         # the values 1 and 2 of the round in front are dropped


def test_reps_per_leg_are_passed_through():
    calls, timed = _clock()
    SB.rounds_of({'a': 'A', 'torch': 'T'}, {'a': 300, 'torch': 30}, 2, False, timed)
    assert calls == [('A', 300), ('T', 30)] * 2


def test_the_default_clock_is_timed():
    import inspect
    assert inspect.signature(SB.rounds_of).parameters['timed'].default is SB.timed
    assert inspect.signature(SB.timed).parameters['warm'].default == 3


def test_builds_are_compared_on_shared_buffers_then_timed_in_interleaved_rounds():
    """``compare_builds`` under a fake clock: the entry point is rebound per build for the first calls and for every timing, the
    results must agree before anything is timed, a warm round is dropped, the lines carry the rule's outcome, and the tree's
    function is bound again afterwards - also when the builds disagree"""
    import torch
    from reconfigisp_amd import lib as L
    entry, out, state = 'risp_no_such_entry', torch.zeros(4), torch.zeros(1)
    builds = {'tree': {entry: 'T'}, 'fast': {entry: 'F'}, 'slow': {entry: 'S'}, 'same': {entry: 'E'}}
    us = {'T': 20.0, 'F': 10.0, 'S': 30.0, 'E': 20.5}
    seen, resets, lines = [], [], []

    def leg():
        seen.append(L._FN[entry])
        out.copy_(state.expand(4) + 1)
        state.add_(1)

    def timed(fn, reps):
        assert fn is leg
        seen.append((L._FN[entry], reps))
        return us[L._FN[entry]] + 0.25 * (len(seen) % 3)        # spreads of at most 0.5

    won = SB.compare_builds(lines.append, 'a row', builds, entry, leg, (out,), 5, 3, lambda: (resets.append(1), state.zero_()), timed)
    assert won == ['fast'] and len(resets) == 4 and L._FN[entry] == 'T'
    assert seen == ['T', 'F', 'S', 'E'] + [('T', 5), ('F', 5), ('S', 5), ('E', 5)] * 4      # one call each, then 1 + 3 rounds
    assert lines[0] == ' a row, 5 calls per round; us per call' and len(lines) == 5
    assert [line.split()[0] for line in lines[1:]] == ['tree', 'fast', 'slow', 'same']
    assert 'tree - ' not in lines[1] and lines[1].count('.') == 3 + 3       # median, min, spread and three kept rounds
    assert lines[2].endswith(': BEATS the tree') and lines[3].endswith(': loses') and lines[4].endswith(': level')
    assert 'tree - fast = +10.0 us against a spread of 0.5 us' in lines[2]
    # a build whose first call gives other bytes: nothing is timed
    seen.clear()
    with pytest.raises(AssertionError, match='the builds disagree: a row'):
        SB.compare_builds(lines.append, 'a row', builds, entry, leg, (out,), 5, 3, timed=timed)      # no reset: the state moves on
    assert seen == ['T', 'F', 'S', 'E'] and L._FN.pop(entry) == 'T'
    assert SB.beaten_line([]) == 'rows in which another build beats the tree: none'
    assert SB.beaten_line(['a row by fast', 'b by fast']) == 'rows in which another build beats the tree: a row by fast; b by fast'


def _tables():
    """(profile, table name, the table's members as the script words them, in the order the script emits them)"""
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    return [('serve_shade.txt', '_FUSED_SHADE', ['/'.join(k) for k in [('classical', 'u16')] if k in PF._FUSED_SHADE]),
            ('serve_defect.txt', '_DEFECT_SHADE_FUSED', [f for f in ('u16', 'raw10', 'raw12') if f in PF._DEFECT_SHADE_FUSED]),
            ('serve_resize.txt', '_RESIZE_NV12_FUSED', [f for f in ('nv12',) if f in PF._RESIZE_NV12_FUSED]),
            ('serve_warp.txt', '_WARP_STAGED', [k for k in ('bilinear', 'bicubic') if k in PF._WARP_STAGED]),
            ('serve_sharpen.txt', '_SHARPEN_NV12_FUSED', [f for f in ('nv12',) if f in PF._SHARPEN_NV12_FUSED])]


def test_verdict_line_writes_what_the_profiles_hold_and_read_verdict_reads():
    from reconfigisp_amd.codes.models.modules import pipeline_fusion as PF
    assert SB.verdict_line('_T', []) == 'verdict: _T = none'
    assert SB.verdict_line('_T', ['u16', 'raw10', 'raw12']) == 'verdict: _T = u16 raw10 raw12'       # the order given
    for profile, name, members in _tables():
        table = getattr(PF, name)
        assert len(members) == len(table), name
        text = open(os.path.join(ROOT, 'profiles', profile)).read().split('\n')
        assert SB.verdict_line(name, members) in text, (profile, SB.verdict_line(name, members))
        assert read_verdict(profile, name) == frozenset(members)


def test_read_verdict_asks_for_exactly_one_line():
    with pytest.raises(AssertionError, match='one line'):
        read_verdict('serve_shade.txt', '_NO_SUCH_TABLE')


def test_no_script_defines_its_own_copy_of_a_shared_helper():
    scripts = sorted(glob.glob(os.path.join(ROOT, 'tools', 'bench_serve*.py')))
    assert len(scripts) >= 18
    shared = {'timed', 'frames_u16', 'frames_int', 'pack', 'vignette', 'load_parent'}
    for path in scripts:
        tree = ast.parse(open(path).read())
        own = {node.name for node in tree.body if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef))}
        assert not own & shared, (os.path.basename(path), sorted(own & shared))
