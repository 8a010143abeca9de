#!/usr/bin/env python3
"""Recording of the generation host path's launches for tests/test_gpu_generation_launches.py.

Runs every case of test_gpu_generation_launches.CASES on the GPU under the recorder and writes generation_launches.json: per case the number of
launches, the run-length-encoded op names, the sha256 of the canonical text and the sha256 of the token ids.  The committed fixture was
written at the commit BEFORE the host path was folded into one sampling step, one per-request runner and one graph runner; regenerate it
only when a change alters launches on purpose.

    python tests/golden/make_generation_launches.py [--out FILE] [--dump DIR]

--dump DIR also writes the full text of every case to DIR/<case>.txt, so that two commits' records can be diffed.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch

from test_gpu_generation_launches import CASES, record_case

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'generation_launches.json'))
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    dev, fixture = torch.device('cuda:0'), {}
    for name in sorted(CASES):
        fixture[name], text = record_case(name, dev)
        print(f'{name}: {fixture[name]["launches"]} launches, ids {str(fixture[name]["ids_sha256"])[:12]}', flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + '.txt'), 'w') as f:
                f.write(text)
    with open(args.out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(fixture[k], sort_keys=True)}' for k in sorted(fixture)) + '\n}\n')          # one line per case
    print(f'wrote {args.out}  {os.path.getsize(args.out) / 1024:.1f} KiB')
