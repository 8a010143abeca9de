#!/usr/bin/env python3
"""A/B of controlvar_amd/train.py against another commit's copy of it, in one process on one GPU (profiles/train_walk_parent_ab.txt).

Only train.py differs between the two sides (same kernels, same ops, same model object), so the other side is that file loaded a second time as a
module of this package - twice, as `parent_a` and `parent_b`, to get the spread between two copies of the same code.  The three variants take turns,
repetition by repetition, in an order that rotates; each turn builds its own Trainer / TrainEngine (one set of activation buffers alive at a time), warms it up and times a
window that ends in a device synchronise (host clock).  Medians over the repetitions are reported.

    git show <commit>:controlvar_amd/train.py > /tmp/train_parent.py
    python tools/train_walk_ab.py --parent /tmp/train_parent.py --what d24     (d24 bf16 B = 32 Trainer.step, as tools/train_bench.py 24 32)
    python tools/train_walk_ab.py --parent /tmp/train_parent.py --what lora    (the same model after lora.add_lora, as tools/lora_bench.py)
    python tools/train_walk_ab.py --parent /tmp/train_parent.py --what d2      (depth 2, B = 1 forward_backward, full and LoRA: host time per launch)
"""
import argparse
import gc
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from controlvar_amd import lora, models  # noqa: E402
from controlvar_amd import train as this_train  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402


def load(path, tag):
    spec = importlib.util.spec_from_file_location(f'controlvar_amd._train_{tag}', path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def turns(variants, rep):
    """the variants in an order that rotates with the repetition, so that none always runs behind the same other one"""
    items = list(variants.items())
    return items[rep % len(items):] + items[:rep % len(items)]


def report(what, unit, times, extra=None):
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {'what': what, 'unit': unit, 'reps': len(next(iter(times.values()))), 'median': {k: round(v, 3) for k, v in med.items()},
           'min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           'parent_vs_parent': round(abs(med['parent_a'] - med['parent_b']), 3),
           'this_minus_parent_mean': round(med['this'] - (med['parent_a'] + med['parent_b']) / 2, 3),
           'this_within_parent_spread': min(med['parent_a'], med['parent_b']) <= med['this'] <= max(med['parent_a'], med['parent_b'])}
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def step_ab(a, variants, dev, with_lora):
    vae = models.build_vae(ch=160).to(dev)
    var = models.build_control_var(vae, depth=24, mask_type='interleave_append', multi_cond=True).to(dev).train()
    if with_lora:
        lora.add_lora(var)
    B = 32
    images, masks = synth_images(B, 256, seed=0).to(dev), synth_images(B, 256, seed=100).to(dev)
    cls = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(0))
    types = torch.arange(B) % 4
    times = {k: [] for k in variants}
    for rep in range(a.reps + 1):                   # the first round carries the process's cold start: dropped
        for k, T in turns(variants, rep):
            tr = T.Trainer(var, vae, peak_lr=8e-5 * B / 512, weight_decay=0.08, sche='lin0', warmup_it=10, max_it=1000, clip=2.0)
            dt = timed(lambda: tr.step(images, masks, cls, types, mask_first=True), 1, a.steps)
            if rep:
                times[k].append(dt * 1e3)
            del tr
            gc.collect()
            torch.cuda.empty_cache()
    report('d24 bf16 B=32 Trainer.step' + (' after add_lora' if with_lora else ''), 'ms per step', times, {'steps_per_window': a.steps})


def d2_ab(a, variants, dev):
    F = torch.bfloat16
    vae = models.build_vae(ch=32, compute_dtype=F).to(dev)
    images, masks = synth_images(1, 256, seed=6).to(dev), synth_images(1, 256, seed=7).to(dev)
    cls, types = torch.tensor([17]), torch.tensor([2])
    for mode in ('full', 'lora'):
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=F, cond_drop_rate=0.0).to(dev).eval()
        if mode == 'lora':
            lora.add_lora(m, r=16, dropout=0.0, seed=1)
        x, labels = this_train.Trainer(m, vae, peak_lr=1e-3, weight_decay=0.0).tokenize(images, masks)
        times = {k: [] for k in variants}
        for rep in range(a.reps + 1):
            for k, T in turns(variants, rep):
                eng = T.TrainEngine(m, drop_path=False)
                dt = timed(lambda: eng.forward_backward(cls, x, types, labels), 20, a.d2_steps)
                if rep:
                    times[k].append(dt * 1e6)
                del eng
        leaf_calls = 7 + 2 * (4 if mode == 'full' else 3)        # forward: 3 per block + the generator; backward: one per linear with a parameter gradient
        report(f'depth 2 bf16 B=1 forward_backward, {mode}', 'us per step', times, {'steps_per_window': a.d2_steps, 'leaf_calls_per_step': leaf_calls})


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help="the other commit's controlvar_amd/train.py")
    ap.add_argument('--what', required=True, choices=['d24', 'lora', 'd2'])
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--d2-steps', type=int, default=200)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    variants = {'parent_a': load(a.parent, 'parent_a'), 'this': this_train, 'parent_b': load(a.parent, 'parent_b')}
    if a.what == 'd2':
        d2_ab(a, variants, dev)
    else:
        step_ab(a, variants, dev, a.what == 'lora')
