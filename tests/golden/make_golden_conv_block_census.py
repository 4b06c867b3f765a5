#!/usr/bin/env python
"""Generate tests/golden/conv_block_census.json: for every case of tests/conv_block_cases.py the ordered C-ABI entry points of
one training forward + backward (and of one eval forward where the case has one).  Needs the GPU.

    python tests/golden/make_golden_conv_block_census.py [output.json]

The file is a behaviour lock for refactors of ops.conv_block / ops.conv_block_bf16 / FusedBackbone: generate it at the commit
whose launch sequence is to be kept, commit it, and do NOT regenerate it on the refactored code to make the test pass.  It holds
names only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_block_cases as cases      # noqa: E402


def main(path):
    from capsyolo_amd import ops
    out = {}
    for name in cases.CASES:
        old = {}

        def set_switch(obj, attr, value):
            old.setdefault(attr, getattr(obj, attr))
            setattr(obj, attr, value)
        try:
            out[name] = cases.census(name, set_switch)
        finally:
            for attr, value in old.items():
                setattr(ops, attr, value)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %s' % (path, ', '.join('%s %d' % (n, sum(len(v) for v in c.values())) for n, c in out.items())))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'conv_block_census.json'))
