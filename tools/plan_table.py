"""Answers of the conv planning queries (tests/plan_queries.py) of ONE build of the library, as JSON.

    PSEG_LIB_PATH=/path/to/libpseg_amd.so python tools/plan_table.py --grid full --out answers.json
    PSEG_LIB_PATH=... python tools/plan_table.py --grid pinned --settings "" PSEG_CONV_NOSKIP=1 --out tests/golden/plan_table.json

A change that must not move a planning decision is checked by writing the table with the library of the commit before it and
with the new one (under every PSEG_CONV_* setting of interest, one process each: some switches are read once) and comparing the
files; tests/golden/plan_table.json pins a subset.  It is written with the build BEFORE such a change, never with the code under
test.  Runs without a GPU.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def rows(which):
    import plan_queries
    from pytorch_segmentation_amd import _lib
    lib = _lib.load()
    probs = plan_queries.grid() if which == 'full' else plan_queries.pinned()
    return [[list(p), plan_queries.answers(lib, p)] for p in probs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', choices=('full', 'pinned'), default='pinned')
    ap.add_argument('--settings', nargs='*', default=None, help='NAME=VALUE[,NAME=VALUE] per table; "" = default environment')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    if args.settings is None:
        table = rows(args.grid)
    else:
        table = {}
        for setting in args.settings:
            env = dict(os.environ)
            env.update(kv.split('=') for kv in setting.split(',') if kv)
            tmp = args.out + '.part'
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--grid', args.grid, '--out', tmp], env=env)
            table[setting] = json.load(open(tmp))
            os.remove(tmp)
    with open(args.out, 'w') as f:
        json.dump(table, f, separators=(',', ':'))
    print('%s: %s' % (args.out, {k: len(v) for k, v in table.items()} if isinstance(table, dict) else len(table)))


if __name__ == '__main__':
    main()
