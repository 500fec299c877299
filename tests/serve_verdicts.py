"""The line that carries a measured verdict from a recorded profile into a CPU test: `verdict: NAME = member member ..` or
`verdict: NAME = none`, as tools/serve_bench.verdict_line writes it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_verdict(profile_name, table_name):
    """the members that profiles/<profile_name> states for ``table_name``, as a frozenset of the words of its one verdict line"""
    text = open(os.path.join(ROOT, 'profiles', profile_name)).read()
    lines = re.findall(r'^verdict: %s = (.*)$' % re.escape(table_name), text, flags=re.M)
    assert len(lines) == 1, 'profiles/%s states the verdict in one line' % profile_name
    return frozenset() if lines[0].strip() == 'none' else frozenset(lines[0].split())
