"""The dispatch records of the kernel census (tests/kernel_census.py), from kernel traces; names in the census's own form (template
arguments kept, return type, namespace, parameter list and clone suffix dropped).

profiles/kernel_census_dispatched.txt -- the sorted set of kernels one run of the census module dispatched, one per line:

    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python -m pytest tests/test_gpu_kernel_census.py -m gpu
    python tools/kernel_census_dispatched.py TRACE_DIR

profiles/kernel_census_covered.txt -- per covering test of COVERED_ELSEWHERE, traced on its own into a directory of its own that
holds a file TEST with the test's id: the kernels it maps to that test which the run dispatched, one `kernel<TAB>test` per line:

    rocprofv3 --kernel-trace --output-format csv -d ROOT_DIR/0 -- python -m pytest tests/test_gpu_ode.py::test_x -m gpu  (etc.)
    python tools/kernel_census_dispatched.py --covered ROOT_DIR

A trace directory is searched for *kernel_trace.csv files (one per traced process)."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.kernel_census import COVERED, COVERED_ELSEWHERE, DISPATCHED, census_name  # noqa: E402


def dispatched_names(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True))
    if not files:
        raise SystemExit('no *kernel_trace.csv under %s' % trace_dir)
    names = set()
    for path in files:
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                names.add(census_name(row['Kernel_Name']))
    return sorted(n for n in names if n)


def covered_pairs(root_dir):
    pairs = set()
    for test_file in sorted(glob.glob(os.path.join(root_dir, '*', 'TEST'))):
        with open(test_file) as f:
            test = f.read().strip()
        names = set(dispatched_names(os.path.dirname(test_file)))
        pairs |= {(k, t) for k, t in COVERED_ELSEWHERE.items() if t == test and k in names}
    return sorted(pairs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('trace_dir')
    ap.add_argument('--covered', action='store_true', help='trace_dir holds one traced directory per covering test')
    ap.add_argument('-o', '--output')
    args = ap.parse_args()
    if args.covered:
        lines = ['%s\t%s' % kv for kv in covered_pairs(args.trace_dir)]
        out = args.output or COVERED
    else:
        lines = dispatched_names(args.trace_dir)
        out = args.output or DISPATCHED
    with open(out, 'w') as f:
        f.write(''.join(n + '\n' for n in lines))
    print('%d lines -> %s' % (len(lines), out))


if __name__ == '__main__':
    main()
