#!/usr/bin/env python3
"""Recording of the training engine's launches for tests/test_gpu_train_launches.py.

Runs every case of test_gpu_train_launches.CASES on the GPU under the recorder and writes train_launches.json: per case the number of launches, the
run-length-encoded op names, the sha256 of the canonical text, the sha256 of the fp32 values the case produced, the branch its weight gradients and
its word-embedding gradient took, and the peak of allocated device memory over the case.  The committed fixture was written at the commit BEFORE the
full and the LoRA copy of the buffer plan, the forward block body and the backward walk were folded into one each; regenerate it only when a change
alters launches on purpose.

    python tests/golden/make_train_launches.py [--out FILE] [--dump DIR]

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

from test_gpu_train_launches import CASES, record_case


def expected_paths(name):
    """what TrainEngine's conditions say for the recorded shapes: cvar_gemm_tn takes bf16 operands whose dimensions are multiples of 128 (qkv / proj /
    fc1 / fc2 at C = 128, hid = 512), fp32 goes through the two transposes; the one-pass word-embedding kernel takes cvae = 32, C % 64 = 0 and fp32
    tokens, which every full case here has (the per-sample path needs another cvae or width); a LoRA model computes neither"""
    if name.startswith('lora_'):
        return dict(wgrad=None, word_embed=None)
    return dict(wgrad='gemm_tn' if 'bf16' in name else 'transposes', word_embed='one_pass')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'train_launches.json'))
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    dev, fixture = torch.device('cuda:0'), {}
    for name in sorted(CASES):
        fixture[name], text = record_case(name, dev)
        e = fixture[name]
        print(f'{name}: {e["launches"]} launches, bytes {str(e["bytes_sha256"])[:12]}, paths {e["paths"]}, peak {e["peak_bytes"]}', flush=True)
        assert e['paths'] == expected_paths(name), (name, e['paths'], expected_paths(name))
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + '.txt'), 'w') as f:
                f.write(text)
    with open(args.out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(fixture[k], sort_keys=True)}' for k in sorted(fixture)) + '\n}\n')          # one line per case
    print(f'wrote {args.out}  {os.path.getsize(args.out) / 1024:.1f} KiB')
