#!/usr/bin/env python3
"""Regenerate profiles/traffic.json from the FETCH_SIZE / WRITE_SIZE passes of tools/profile_bench.sh <tag>: reads
summary.txt (written by tools/summarize_prof.py) in the output directory that script printed, for the kernel instance
risp_bilateral_chain_kernel() names - bench.py reports roofline.traffic only while that is the kernel it launches.

    python tools/collect_traffic.py <tag> <profile directory> [bench arguments of the counter passes, for the record]

The point-wise kernel's entry is refreshed when the passes ran it (bench.py --full) and carried over otherwise."""
import json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG, SUMMARY = sys.argv[1], os.path.join(os.path.abspath(sys.argv[2]), 'summary.txt')
how = ' '.join(sys.argv[3:]) or '--full --steps 200 --warmup 20 --no-cpu --no-cnn --no-search'
os.chdir(ROOT)
sys.path.insert(0, ROOT)
from reconfigisp_amd import lib as L          # noqa: E402  (the name query touches no GPU)
kernel = L.load().risp_bilateral_chain_kernel(1, 3, 0).decode()           # what a bench step launches, as rocprofv3 prints it


def per_launch(counter, name, required=True):
    """average raw counter value (KiB) per launch of the kernel whose rocprofv3 name - spaces aside - starts with `name`"""
    want, section = name.replace(' ', ''), None
    for ln in open(SUMMARY):
        if ln.startswith('== '):
            section = ln.split()[1]
        elif section == counter and ln.replace(' ', '').replace('void(anonymousnamespace)::', '').startswith(want):
            m = re.search(r'launches\s+(\d+)\s+avg\s+([\d.]+) KiB', ln)
            return float(m.group(2)), int(m.group(1))
    if required:
        raise SystemExit('no %s row for %s in %s' % (counter, name, SUMMARY))
    return None, 0


fetch, nf = per_launch('FETCH_SIZE', kernel)
write, nw = per_launch('WRITE_SIZE', kernel)
old = json.load(open('profiles/traffic.json'))
alg = 64 * 64 * 256 * 256                       # bench.py: BYTES_PER_PIX_ISP x the pixels of one launch (batch 64 of 256 x 256)
traffic = {
    '_comment': 'HBM bytes per launch of the dominant kernel from rocprofv3 PMC passes (tools/profile_bench.sh %s: separate --pmc FETCH_SIZE and --pmc WRITE_SIZE runs of '
                '`bench.py %s`), written by tools/collect_traffic.py.  Counter units are KiB.  WRITE_SIZE is exact for 16-byte-per-lane stores; FETCH_SIZE is multiplied by 2 '
                '(calibrated on this chip with tools/fetch_calib.hip: factor 2.000 for 4-, 8- and 16-byte loads, profiles/r02_fetch_size_calibration.txt).  `kernel` is what '
                'risp_bilateral_chain_kernel() names for the bench launch: bench.py reports these bytes only while that is the kernel it launches.' % (TAG, how),
    'round': TAG, 'kernel': kernel, 'launches_averaged': [nf, nw],
    'fetch_size_kib_raw': round(fetch, 1), 'fetch_size_factor_calibrated': 2.0, 'write_size_kib_raw': round(write, 1),
    'traffic_bytes_per_launch': int(round((2.0 * fetch + write) * 1024)), 'algorithmic_bytes_per_launch': alg,
    'before_xcd_aware_order': old.get('before_xcd_aware_order'),
}
if old.get('kernel') != kernel:                 # the form this one replaced, for comparison
    traffic['previous_form'] = {k: old[k] for k in ('round', 'kernel', 'fetch_size_kib_raw', 'write_size_kib_raw', 'traffic_bytes_per_launch') if k in old}
elif 'previous_form' in old:
    traffic['previous_form'] = old['previous_form']
pw_fetch, _ = per_launch('FETCH_SIZE', 'chain_kernel<2,false>', required=False)
pw_write, _ = per_launch('WRITE_SIZE', 'chain_kernel<2,false>', required=False)
if pw_fetch is not None and pw_write is not None:
    traffic['pointwise_kernel'] = {'kernel': 'chain_kernel<2,false>', 'fetch_size_kib_raw': round(pw_fetch, 1), 'write_size_kib_raw': round(pw_write, 1),
                                   'traffic_bytes_per_launch': int(round((2.0 * pw_fetch + pw_write) * 1024)), 'algorithmic_bytes_per_launch': 52 * 64 * 256 * 256}
else:
    traffic['pointwise_kernel'] = old.get('pointwise_kernel')
json.dump(traffic, open('profiles/traffic.json', 'w'), indent=1)
print('traffic.json: %s, %.1f MB per launch = %.3f x algorithmic (fetch 2 x %.1f KiB = %.1f MB)'
      % (kernel, traffic['traffic_bytes_per_launch'] / 1e6, traffic['traffic_bytes_per_launch'] / alg, fetch, 2 * fetch * 1024 / 1e6))
