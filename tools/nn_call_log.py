"""The library calls of nn.Conv2d / BatchNorm2d / ConvNormAct / the ResNet bottleneck over the cases of tests/nn_calls.py, as JSON.

    python tools/nn_call_log.py --out tests/golden/nn_calls.json

A change to the Python layer that must launch what it launched before is checked by writing the file with the commit before it
and comparing: tests/test_nn_calls_cpu.py does that against tests/golden/nn_calls.json, which is written with the code BEFORE such
a change, never with the code under test.  Two runs give the same bytes.  Runs without a GPU (the library must be built).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    import nn_calls
    table = {}
    for case in nn_calls.cases():
        assert case[0] not in table, case[0]
        table[case[0]] = log = nn_calls.run_case(case)
        nn_calls.check_presence(case, log)
    with open(args.out, 'w') as f:
        f.write('{\n' + ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in table.items()) + '\n}\n')
    print('%s: %d cases, %d calls' % (args.out, len(table), sum(len(v) for v in table.values())))


if __name__ == '__main__':
    main()
