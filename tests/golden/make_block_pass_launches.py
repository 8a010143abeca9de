#!/usr/bin/env python3
"""Recording of the transformer pass's and the VQVAE walk's launches for tests/test_gpu_block_pass_launches.py.

Runs every case of test_gpu_block_pass_launches.CASES on the GPU under the recorder and writes block_pass_launches.json: per case the number of
launches, the run-length-encoded op names, the sha256 of the canonical text, the sha256 of the token ids and of the fp32 values the case produced, and
the peak of allocated device memory over the case.  The committed fixture was written at the commit BEFORE the per-mode copies of the pass and of the
encoder were folded into one walk each; regenerate it only when a change alters launches on purpose.

    python tests/golden/make_block_pass_launches.py [--out FILE] [--dump DIR]

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

from test_gpu_block_pass_launches import CASES, record_case

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'block_pass_launches.json'))
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    dev, fixture = torch.device('cuda:0'), {}
    for name in sorted(CASES):
        fixture[name], text = record_case(name, dev)
        e = fixture[name]
        print(f'{name}: {e["launches"]} launches, ids {str(e["ids_sha256"])[:12]}, bytes {str(e["bytes_sha256"])[:12]}, peak {e["peak_bytes"]}', flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + '.txt'), 'w') as f:
                f.write(text)
    with open(args.out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(fixture[k], sort_keys=True)}' for k in sorted(fixture)) + '\n}\n')          # one line per case
    print(f'wrote {args.out}  {os.path.getsize(args.out) / 1024:.1f} KiB')
