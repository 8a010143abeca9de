"""LoRA vs full fine-tuning step of d24 (bf16, B = 32) in one process on one GPU: samples/s of Trainer.step for both, and - from a
separate ``rocprofv3 --kernel-trace --stats`` run of the LoRA step alone (--lora-only) - the share of the csrc/lora.hip kernels.

    python tools/lora_bench.py --out profiles/lora_d24_b32.json
    rocprofv3 --kernel-trace --stats -d <dir> -o lora -- python tools/lora_bench.py --lora-only --steps 3
    python tools/lora_bench.py --stats <dir>/.../lora_kernel_stats.csv --out profiles/lora_d24_b32.json     (adds the kernel share)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def time_steps(tr, batch, steps, warmup):
    import torch
    images, masks, cls, types = batch
    for i in range(warmup):
        tr.step(images, masks, cls, types, drop_seed=i, mask_first=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(images, masks, cls, types, drop_seed=warmup + i, mask_first=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run(a):
    import torch
    from controlvar_amd import lora, models
    from controlvar_amd import train as T
    from controlvar_amd.synth import synth_images
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    B = a.batch
    g = torch.Generator().manual_seed(0)
    batch = (synth_images(B, 256, seed=1).to(dev), synth_images(B, 256, seed=2).to(dev), torch.randint(0, 1000, (B,), generator=g),
             torch.randint(0, 4, (B,), generator=g))
    kw = dict(peak_lr=8e-5 * B / 512, weight_decay=0.08, sche='lin0', warmup_it=10, max_it=10000, clip=2.0, train_mode=True)
    out = {'config': f'd{a.depth} ControlVAR training step, bf16, B = {B}, frozen tokenizer inside the step, one GPU', 'lib_digest': lib_digest()}
    if not a.lora_only:
        var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev)
        dt = time_steps(T.Trainer(var, vae, **kw), batch, a.steps, a.warmup)
        out['full'] = {'samples_per_s': round(B / dt, 2), 'ms_per_step': round(dt * 1e3, 2)}
        del var
        torch.cuda.empty_cache()
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev)
    lora.add_lora(var)
    tr = T.Trainer(var, vae, **kw)
    dt = time_steps(tr, batch, a.steps, a.warmup)
    out['lora'] = {'samples_per_s': round(B / dt, 2), 'ms_per_step': round(dt * 1e3, 2), 'trainable': lora.trainable_parameters(var)[0]}
    if 'full' in out:
        out['lora_over_full'] = round(out['lora']['samples_per_s'] / out['full']['samples_per_s'], 3)
    return out


def kernel_share(path):
    """(ms of the lora_* kernels, ms of all kernels, per-kernel rows) from a rocprofv3 --stats kernel table"""
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r['TotalDurationNs']) for r in rows) / 1e6
    mine = [(r['Name'], round(float(r['TotalDurationNs']) / 1e6, 3), int(r['Calls'])) for r in rows if 'lora_' in r['Name']]
    return sum(m[1] for m in mine), tot, mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--lora-only', action='store_true', help='time the LoRA step alone (the profiled run)')
    ap.add_argument('--stats', help='rocprofv3 kernel stats CSV of a --lora-only run: add the lora kernel share to --out')
    ap.add_argument('--out', help='JSON file to write (or to update with --stats)')
    a = ap.parse_args()
    if a.stats:
        out = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        ms, tot, rows = kernel_share(a.stats)
        out['lora_kernels'] = {'ms_total': round(ms, 3), 'all_kernels_ms': round(tot, 3), 'share': round(ms / tot, 4),
                               'kernels': [{'name': n, 'ms': t, 'calls': c} for n, t, c in rows],
                               'note': 'rocprofv3 --kernel-trace --stats over a --lora-only run (warm-up steps included)'}
    else:
        out = run(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
